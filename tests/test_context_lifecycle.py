"""Memory of a context through the C ABI: every device buffer is counted when it is allocated and given back by rnnt_destroy, and a
refused allocation is an error return that leaves nothing behind.  Needs a real MI355X: `pytest -m gpu`.

The instrument is rnnt_live_device_bytes(): the bytes held through the library's buffer owners, process-wide.  Engines of other test
modules may be alive, so every assertion is relative to a baseline read after gc.collect().  Numerics are other files' business:
the only values compared here are greedy tokens against themselves."""
import gc

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_OOM, RnntEngine, RnntError

pytestmark = pytest.mark.gpu

SMALL = dict(max_streams=2, max_chunk_frames=32, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=2)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _live():
    return rlib.live_device_bytes()


def _baseline():
    gc.collect()
    return _live()


def _greedy(eng, x):
    """two 32-frame chunks through the per-chunk API -> the tokens of every stream"""
    s = _stream()
    eng.reset(2, s)
    off = 0
    for ci in range(2):
        off += eng.encoder_chunk(x[:, ci * 32:(ci + 1) * 32].contiguous().data_ptr(), 32, off, off, s)
        eng.greedy_decode(s)
        eng.frames_consume(s)
    return eng.tokens(s)


def _chunks(eng, x):
    plan = [(a, b) for a, b in T.chunk_plan(x.size(1), 16) if b - a >= 7]
    offs, o = [], 0
    for a, b in plan:
        offs.append(o)
        o += (b - a) // 4
    s = _stream()
    eng.reset(2, s)
    return eng.encoder_chunks(x.data_ptr(), x.size(1), [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s, greedy=False)


def _walk(np_state_dict, monkeypatch):
    """One call of every entry point that allocates lazily, each twice, on two fresh engines that are closed at the end.
    Returns (the greedy tokens, the largest count seen above the baseline)."""
    base = _baseline()
    s = _stream()
    x = torch.from_numpy(T.synth_fbank(2, 64, seed=5)).cuda()
    enc = torch.randn(2, 15, 256, generator=torch.Generator().manual_seed(3)).cuda()
    pred = torch.randn(2, 3, 256, generator=torch.Generator().manual_seed(4)).cuda()
    lat = torch.empty(2, 15, 3, T.VOCAB, device="cuda")
    wave = torch.randn(2, 63 * 512, generator=torch.Generator().manual_seed(6)).cuda()
    feats = torch.empty(2, 64, 80, device="cuda")
    Tb, Ub = np.array([15, 9], np.int32), np.array([4, 2], np.int32)
    tg = np.array([[1, 2, 3, 4], [6, 7, 0, 0]], np.int32)                # no blank (5) inside a row's length
    lens = [64, 40]                                                       # two chunk plans with different tails

    eng = RnntEngine(**SMALL)
    assert _live() > base                                                 # the create-time buffers are counted
    peak = [_live()]
    tokens = []

    def step(name, fn, owns, e=eng):
        """owns: the path has buffers of its own, so its first call must raise the count; the identical call again must not move it"""
        before = _live()
        fn(e)
        first = _live()
        fn(e)
        torch.cuda.synchronize()
        assert first > before if owns else first >= before, (name, before, first)
        assert _live() == first, (name, first, _live())
        peak.append(first)

    def per_chunk(e):
        tokens.append(_greedy(e, x))

    def ragged_beam(e):
        e.reset(2, s)
        e.beam_decode(0, e.encode_ragged(x.data_ptr(), 64, lens, 16, s), 2, s)

    def advance(e):
        e.reset(2, s)
        e.beam_advance(0, e.encoder_chunk(x[:, :32].contiguous().data_ptr(), 32, 0, 0, s), 2, s)

    def opened(e):
        e.reset(2, s)
        e.stream_open(0, s)

    def pool(e, beam):
        opened(e)
        row = x[:1, :32].contiguous()
        if beam:
            e.pool_chunk_beam([0], row.data_ptr(), 32, [0], [0], 2, s)
        else:
            e.pool_chunk([0], row.data_ptr(), 32, [0], [0], True, s)

    step("load_state_dict(bf16x3)", lambda e: e.load_state_dict(np_state_dict(0), numerics="bf16x3"), True)
    step("encoder_chunk + greedy_decode", per_chunk, False)
    step("encoder_chunks", lambda e: _chunks(e, x), True)
    step("decode_ragged", lambda e: (e.reset(2, s), e.decode_ragged(x.data_ptr(), 64, lens, 16, s)), True)
    step("encode_ragged + beam_decode", ragged_beam, True)
    step("beam_advance", advance, False)
    step("stream_open", opened, True)
    step("pool_chunk", lambda e: pool(e, False), False)
    step("pool_chunk_beam", lambda e: pool(e, True), True)
    step("joint", lambda e: e.joint(enc.data_ptr(), pred.data_ptr(), 2, 15, 3, 1, lat.data_ptr(), s), False)
    step("transducer_nll", lambda e: e.transducer_nll(enc.data_ptr(), Tb, tg, Ub, 2, 15, None, s), True)
    step("ctc_nll", lambda e: e.ctc_nll(enc.data_ptr(), Tb, tg, Ub, 2, 15, s), True)
    step("transducer_align", lambda e: e.transducer_align(enc.data_ptr(), Tb, tg, Ub, 2, 15, stream=s), True)
    step("ctc_align", lambda e: e.ctc_align(enc.data_ptr(), Tb, tg, Ub, 2, 15, s), True)
    step("prefix_beam_decode", lambda e: e.prefix_beam_decode(enc.data_ptr(), Tb, 2, 15, 2, stream=s), True)
    step("context_set", lambda e: e.context_set([[1, 2], [3]], 3.0), True)
    step("ctc_prefix_beam_decode", lambda e: e.ctc_prefix_beam_decode(enc.data_ptr(), Tb, 2, 15, 2, True, False, s), True)
    step("fbank", lambda e: e.fbank(wave.data_ptr(), 2, wave.size(1), 16000, feats.data_ptr(), stream=s), True)
    before = _live()
    step("load_state_dict(fp32)", lambda e: e.load_state_dict(np_state_dict(0), numerics="fp32"), False)
    assert _live() == before                                              # same architecture: every weight buffer is kept

    with monkeypatch.context() as m:                                      # the knob is read at rnnt_create
        m.setenv("RNNT_LM", "0")
        wf = RnntEngine(**SMALL)
    step("wavefront: load_state_dict", lambda e: e.load_state_dict(np_state_dict(0), numerics="bf16x3"), True, wf)
    step("wavefront: encoder_chunks", lambda e: _chunks(e, x), True, wf)

    torch.cuda.synchronize()
    eng.close()
    assert base < _live() < peak[-1]
    wf.close()
    assert _live() == base, (_live(), base)
    assert tokens[0] == tokens[1]
    return tokens[0], max(peak) - base


def test_every_buffer_is_returned(np_state_dict, monkeypatch):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    tok_a, peak_a = _walk(np_state_dict, monkeypatch)
    tok_b, peak_b = _walk(np_state_dict, monkeypatch)
    assert sum(len(t) for t in tok_a) > 0
    assert tok_a == tok_b
    assert peak_a == peak_b, (peak_a, peak_b)


def test_create_out_of_memory_is_clean(np_state_dict):
    """rnnt_create whose K/V cache alone is at least twice the device's memory: RNNT_ERR_OOM, nothing kept, and the next launch of
    another context on this thread does not inherit the refused hipMalloc as its own error.  The buffers allocated before the K/V
    cache (about 150 KiB per stream) are held for milliseconds."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    x = torch.from_numpy(T.synth_fbank(2, 64, seed=5)).cuda()
    start = _baseline()
    eng = RnntEngine(**SMALL)
    eng.load_state_dict(np_state_dict(0), numerics="bf16x3")
    want = _greedy(eng, x)
    assert sum(len(t) for t in want) > 0
    torch.cuda.synchronize()
    base = _baseline()
    total = torch.cuda.mem_get_info()[1]
    per_stream = 12 * 5000 * 1024                                         # bytes of one stream's rows in the K (or V) cache
    B = -(-2 * total // per_stream)
    with pytest.raises(RnntError) as ei:
        RnntEngine(max_streams=B, max_chunk_frames=7, max_cache_frames=5000, max_enc_frames=1, max_tokens=1)
    assert ei.value.status == ERR_OOM, ei.value
    assert _baseline() == base
    assert _greedy(eng, x) == want
    eng.close()
    fresh = RnntEngine(**SMALL)
    fresh.load_state_dict(np_state_dict(0), numerics="bf16x3")
    assert _greedy(fresh, x) == want
    fresh.close()
    assert _baseline() == start
