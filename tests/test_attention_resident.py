"""rel_attention_lm_res (one workgroup per stream-head, every key resident in LDS) against the tiled rel_attention_lm_bf it replaces
where the keys fit: the same inputs through both kernels, in two contexts each (RNNT_ATTN_RESIDENT=0 forces the tiled kernel; a
context reads the knob at rnnt_create).  Both kernels compute the same split-operand products, f32 softmax and the same 64-key
rescale steps; only the order of the f32 row reductions differs, so tokens are equal and encoder frames agree to rounding.  Shapes
whose keys do not fit the resident plan must take the tiled kernel.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T

pytestmark = pytest.mark.gpu

ENC_TOL = 2e-5
SPLIT_MODES = ["bf16x3", "f16x3"]


@pytest.fixture(params=SPLIT_MODES)
def split_mode(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    monkeypatch.setenv("RNNT_FUSE_AFTER_NORM", "0")   # materialise the encoder frames (greedy decode alone reads only their projection)
    return request.param


def _uniform(np_state_dict, mode, n, frames, cache, seed):
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    x = torch.from_numpy(T.synth_fbank(n, frames, seed=seed)).cuda().contiguous()
    s = torch.cuda.current_stream().cuda_stream
    sb = StreamingBatch(np_state_dict(0), n, max_chunk_frames=64, max_cache_frames=cache, max_enc_frames=cache, numerics=mode,
                        max_tokens=4 * frames)
    # decode_script(pipelined=True), reading the frames before they are consumed
    from ctc_vr_amd.layout import chunk_plan
    sb.reset()
    plan = [(a, b) for a, b in chunk_plan(frames, 16) if b - a >= 7]
    offs, o = [], 0
    for a, b in plan:
        offs.append(o)
        o += (b - a) // 4
    sb.engine.encoder_chunks(x.data_ptr(), frames, [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s, greedy=True)
    enc = np.array(sb.engine.enc_frames(s), copy=True)
    assert enc.shape[1] > 0
    sb.engine.frames_consume(s)
    toks = sb.engine.tokens(s)
    assert toks == sb.decode_script(x, 16, pipelined=True)
    return toks, enc


def _maxdiff(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def test_resident_equals_tiled_10s(np_state_dict, split_mode, monkeypatch):
    """10 s utterances (188 encoder frames: 186 keys plus chunk 0's parked rows, 7 units): tokens equal, frames within 2e-5, and
    two runs of the resident kernel bit-equal.  The frames are not bit-equal to the tiled kernel's: the resident kernel ran."""
    res1 = _uniform(np_state_dict, split_mode, 8, 1000, 256, 77)
    res2 = _uniform(np_state_dict, split_mode, 8, 1000, 256, 77)
    monkeypatch.setenv("RNNT_ATTN_RESIDENT", "0")
    tiled = _uniform(np_state_dict, split_mode, 8, 1000, 256, 77)
    assert res1[0] == tiled[0]
    assert min(len(t) for t in tiled[0]) > 0
    assert _maxdiff(res1[1], tiled[1]) < ENC_TOL
    assert not np.array_equal(res1[1], tiled[1])
    assert res1[0] == res2[0] and np.array_equal(res1[1], res2[1])


def test_resident_equals_tiled_short(np_state_dict, split_mode, monkeypatch):
    """A short batch (3 s: two key units after chunk 0) with a different seed."""
    res = _uniform(np_state_dict, split_mode, 4, 300, 256, 5)
    monkeypatch.setenv("RNNT_ATTN_RESIDENT", "0")
    tiled = _uniform(np_state_dict, split_mode, 4, 300, 256, 5)
    assert res[0] == tiled[0]
    assert _maxdiff(res[1], tiled[1]) < ENC_TOL
    assert not np.array_equal(res[1], tiled[1])                    # the resident kernel ran


@pytest.mark.parametrize("frames,cache", [(900, 177), (700, 171)])
def test_parked_rows_near_last_tile(np_state_dict, split_mode, monkeypatch, frames, cache):
    """A cache just larger than the utterance (bench.py sizes it encoder frames + 8) parks chunk 0's K/V rows within 64 keys of the
    main segment's last tile origin: 900 frames -> keys [0, 166) and parked rows 174..176 (inside the last tile's second unit);
    700 frames -> keys [0, 129) and parked rows 168..170 (in the last tile's absent second half).  Rows of one segment must never
    be live in another segment's tile."""
    res = _uniform(np_state_dict, split_mode, 4, frames, cache, 31)
    monkeypatch.setenv("RNNT_ATTN_RESIDENT", "0")
    tiled = _uniform(np_state_dict, split_mode, 4, frames, cache, 31)
    assert np.all(np.isfinite(res[1]))
    assert res[0] == tiled[0]
    assert _maxdiff(res[1], tiled[1]) < ENC_TOL
    assert not np.array_equal(res[1], tiled[1])


def test_resident_ragged_64_lengths(np_state_dict, split_mode, monkeypatch):
    """64 distinct lengths (40 .. 1000 frames) in one ragged call (per-stream tables): same tokens through both kernels, every
    stream's encoder frames within 2e-5, and two runs of the resident kernel bit-equal."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    n = 64
    rng = np.random.default_rng(5)
    lens = sorted(rng.choice(np.arange(40, 1001), size=n, replace=False).tolist(), reverse=True)
    lens[0], lens[-1] = 1000, 40
    lens = [lens[i] for i in rng.permutation(n)]
    full = torch.from_numpy(T.synth_fbank(n, 1000, seed=4321))
    x = torch.zeros(n, 1000, 80)
    for b in range(n):
        x[b, :lens[b]] = full[b, :lens[b]]
    xd = x.cuda().contiguous()
    s = torch.cuda.current_stream().cuda_stream

    def run():
        sb = StreamingBatch(np_state_dict(0), n, max_chunk_frames=48, max_cache_frames=256, max_enc_frames=256, numerics=split_mode)
        toks = sb.decode_script_ragged(xd, torch.tensor(lens), 16)
        sb.reset()
        fo = sb.engine.encode_ragged(xd.data_ptr(), 1000, lens, 16, s)   # (every length has two chunks or more)
        enc = np.array(sb.engine.enc_frames(s), copy=True)
        assert enc.shape[1] > 0
        return toks, enc, fo

    t1, e1, fo = run()
    t2, e2, _ = run()
    assert t1 == t2 and np.array_equal(e1, e2)
    monkeypatch.setenv("RNNT_ATTN_RESIDENT", "0")
    t3, e3, _ = run()
    assert t3 == t1
    same = True
    for b in range(n):
        k = int(fo[b])
        if k:
            assert _maxdiff(e1[b, :k], e3[b, :k]) < ENC_TOL, b
            same = same and np.array_equal(e1[b, :k], e3[b, :k])
    assert not same                                                 # the resident kernel ran


def test_long_utterance_takes_tiled_kernel(np_state_dict, split_mode, monkeypatch):
    """30 s utterances (562 keys: more than the resident plan holds) run the tiled kernel whatever the knob says: bit-equal frames."""
    res = _uniform(np_state_dict, split_mode, 2, 3000, 800, 9)
    monkeypatch.setenv("RNNT_ATTN_RESIDENT", "0")
    tiled = _uniform(np_state_dict, split_mode, 2, 3000, 800, 9)
    assert res[0] == tiled[0]
    assert np.array_equal(res[1], tiled[1])
