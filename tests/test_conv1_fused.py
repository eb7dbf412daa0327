"""gemm_bw_c1 (conv2 implicit GEMM that forms its conv1 operand from the fbank in the tile staging: no conv1 launch, no y1 slab)
against conv1_relu_rows + gemm_bw over the slab, in two contexts of one process (RNNT_CONV1_FUSE=0 restores the two launches; a
context reads the knob at rnnt_create).  The producer is conv1's own fmaf chain in conv1's order, so every y1 value -- and with it
everything downstream -- is the same number: encoder frames are compared with np.array_equal, not a tolerance.  Bit-equality cannot
show which kernel ran, so the conv1 launch site is counted as well.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T

pytestmark = pytest.mark.gpu

SPLIT_MODES = ["bf16x3", "f16x3"]
TAG_CONV1 = 1                                            # launch-site tag of rnnt_profile_begin (include/rnnt_hip.h)


@pytest.fixture(params=SPLIT_MODES)
def split_mode(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    monkeypatch.setenv("RNNT_FUSE_AFTER_NORM", "0")   # materialise the encoder frames (greedy decode alone reads only their projection)
    return request.param


def _uniform(np_state_dict, mode, n, frames, cache, seed):
    """One whole-utterance call of n streams x frames (chunk 16) -> tokens, encoder frames, conv1 launches (main chunk class)."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    from ctc_vr_amd.layout import chunk_plan
    x = torch.from_numpy(T.synth_fbank(n, frames, seed=seed)).cuda().contiguous()
    s = torch.cuda.current_stream().cuda_stream
    sb = StreamingBatch(np_state_dict(0), n, max_chunk_frames=64, max_cache_frames=cache, max_enc_frames=cache, numerics=mode,
                        max_tokens=4 * frames)
    sb.reset()
    plan = [(a, b) for a, b in chunk_plan(frames, 16) if b - a >= 7]
    offs, o = [], 0
    for a, b in plan:
        offs.append(o)
        o += (b - a) // 4
    sb.engine.profile_begin(TAG_CONV1)
    sb.engine.encoder_chunks(x.data_ptr(), frames, [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s, greedy=True)
    torch.cuda.synchronize()
    _, conv1_launches = sb.engine.profile_end()
    enc = np.array(sb.engine.enc_frames(s), copy=True)
    assert enc.shape[1] > 0
    sb.engine.frames_consume(s)
    toks = sb.engine.tokens(s)
    assert toks == sb.decode_script(x, 16, pipelined=True)
    return toks, enc, conv1_launches


def _both(np_state_dict, mode, monkeypatch, n, frames, cache, seed):
    fused = _uniform(np_state_dict, mode, n, frames, cache, seed)
    monkeypatch.setenv("RNNT_CONV1_FUSE", "0")
    plain = _uniform(np_state_dict, mode, n, frames, cache, seed)
    return fused, plain


def test_fused_equals_slab_10s(np_state_dict, split_mode, monkeypatch):
    """12 streams x 1000 frames: conv2 M = 12 x 61 x 3 x 19 = 41724 >= 32768.  Frames bit-equal, tokens equal, every stream
    emits; the main class launches no conv1 with the knob on and one with it off."""
    fused, plain = _both(np_state_dict, split_mode, monkeypatch, 12, 1000, 256, 77)
    assert np.array_equal(fused[1], plain[1])
    assert fused[0] == plain[0]
    assert min(len(t) for t in plain[0]) > 0
    assert fused[2] == 0 and plain[2] == 1


def test_fused_partial_last_tile(np_state_dict, split_mode, monkeypatch):
    """16 streams x 700 frames, another seed: M = 16 x 42 x 3 x 19 = 38304 = 299 tiles of 128 + 32 rows, so the last tile's
    stager rows beyond M are clamped."""
    fused, plain = _both(np_state_dict, split_mode, monkeypatch, 16, 700, 256, 31)
    assert 38304 % 128 != 0
    assert np.array_equal(fused[1], plain[1])
    assert fused[0] == plain[0]
    assert min(len(t) for t in plain[0]) > 0
    assert fused[2] == 0 and plain[2] == 1


def test_below_threshold_takes_unfused_path(np_state_dict, split_mode, monkeypatch):
    """4 streams x 300 frames (M = 4 x 17 x 3 x 19 = 3876 < 32768): conv1 is launched whatever the knob says, same result."""
    fused, plain = _both(np_state_dict, split_mode, monkeypatch, 4, 300, 256, 5)
    assert np.array_equal(fused[1], plain[1])
    assert fused[0] == plain[0]
    assert fused[2] == 1 and plain[2] == 1


def _full(np_state_dict, mode, B, Tn, lens, seed):
    from ctc_vr_amd.lib import RnntEngine
    tq = ((Tn - 3) // 2 + 1 - 3) // 2 + 1
    eng = RnntEngine(max_streams=B, max_chunk_frames=Tn, max_cache_frames=tq + 11, max_enc_frames=8, vocab_size=T.VOCAB, blank_id=T.BLANK)
    eng.load_state_dict(np_state_dict(0), numerics=mode)
    x = torch.from_numpy(T.synth_fbank(B, Tn, seed=seed))
    for b in range(B):
        x[b, lens[b]:] = 0
    xd = x.cuda().contiguous()
    out = torch.zeros(B, tq, 256, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    eng.profile_begin(TAG_CONV1)
    assert eng.encoder_full(xd.data_ptr(), np.asarray(lens, np.int32), B, Tn, out.data_ptr(), s) == tq
    torch.cuda.synchronize()
    _, conv1_launches = eng.profile_end()
    return out.cpu().numpy(), conv1_launches


def test_full_context_fused(np_state_dict, split_mode, monkeypatch):
    """rnnt_encoder_full, 4 streams x 2000 frames of unequal lengths (M = 4 x 499 x 19 = 37924): no chunk starts, one long chunk,
    padded rows masked downstream."""
    lens = [2000, 1733, 1200, 1999]
    fused = _full(np_state_dict, split_mode, 4, 2000, lens, 13)
    monkeypatch.setenv("RNNT_CONV1_FUSE", "0")
    plain = _full(np_state_dict, split_mode, 4, 2000, lens, 13)
    assert np.all(np.isfinite(plain[0]))
    assert np.array_equal(fused[0], plain[0])
    assert fused[1] == 0 and plain[1] == 1
