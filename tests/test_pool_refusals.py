"""The slot-list refusals of the stream pool, pinned per entry point: an empty list, one row more than the limit, slot -1, slot =
limit and a slot listed twice are RNNT_ERR_ARG with the entry point's own function name, wording and limit (n_streams for the
encoder forms and rnnt_pool_rescore, max_streams for the prefix-frames, CTC-log-probabilities and wave seams); a second advancing call
with another beam size names the search in progress; and none of them changes anything.  The expected texts are written out here.
Needs a real MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, RnntEngine, RnntError, _np_ptr

pytestmark = pytest.mark.gpu

MAX_STREAMS, N_STREAMS = 3, 2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _engine(sd):
    eng = RnntEngine(max_streams=MAX_STREAMS, max_chunk_frames=32, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=2)
    eng.load_state_dict(sd)
    eng.reset(N_STREAMS, _stream())
    return eng


def _rescore(eng, slots, s):
    """rnnt_pool_rescore with one one-token hypothesis per listed slot (the wrapper cannot shape an n-best for an empty list)"""
    a = np.ascontiguousarray(slots, np.int32)
    n = max(a.size, 1)
    nh, hl, ht, nll = np.ones(n, np.int32), np.ones((n, 1), np.int32), np.ones((n, 1, 1), np.int32), np.zeros((n, 1), np.float64)
    eng._chk(eng.lib.rnnt_pool_rescore(eng.ctx, a.size, _np_ptr(a), _np_ptr(nh), _np_ptr(hl), _np_ptr(ht), 1, 1, _np_ptr(nll), s), "rnnt_pool_rescore")


@pytest.fixture(scope="module")
def world(np_state_dict):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    sd = np_state_dict(0)
    g = torch.Generator().manual_seed(5)
    w = {"eng": _engine(sd), "clean": _engine(sd),
         "x": torch.from_numpy(T.synth_fbank(4, 16, seed=17)).cuda().contiguous(),                       # [4, 16, 80]: up to limit + 1 rows
         "enc": torch.randn(4, 3, 256, generator=g).cuda(),
         "lp": torch.log_softmax(torch.randn(4, 3, T.VOCAB, generator=g), -1).cuda().contiguous(),
         "wave": torch.randn(4, 10, generator=g).cuda(), "fb": torch.zeros(4, 4, 80, device="cuda")}
    torch.cuda.synchronize()
    yield w
    w["eng"].close()
    w["clean"].close()


def _calls(w):
    """entry point -> (the C function's name in its messages, its wording of the row count, its limit, call(slots))"""
    eng, s = w["eng"], _stream()
    x, enc, lp, wave, fb = (w[k].data_ptr() for k in ("x", "enc", "lp", "wave", "fb"))
    z = lambda slots: [0] * len(slots)
    return {
        "pool_chunk": ("rnnt_pool_chunk", "active slots", N_STREAMS, lambda sl: eng.pool_chunk(sl, x, 16, z(sl), z(sl), True, s)),
        "pool_chunk_beam": ("rnnt_pool_chunk_beam", "active slots", N_STREAMS, lambda sl: eng.pool_chunk_beam(sl, x, 16, z(sl), z(sl), 2, s)),
        "pool_chunk_ctc_prefix": ("rnnt_pool_chunk_ctc_prefix", "active slots", N_STREAMS,
                                  lambda sl: eng.pool_chunk_ctc_prefix(sl, x, 16, z(sl), z(sl), 4, False, s)),
        "pool_chunk_prefix": ("rnnt_pool_chunk_prefix", "active slots", N_STREAMS,
                              lambda sl: eng.pool_chunk_prefix(sl, x, 16, z(sl), z(sl), 4, 0.3, 0.7, s)),
        "pool_prefix_frames": ("rnnt_pool_prefix_frames", "active slots", MAX_STREAMS, lambda sl: eng.pool_prefix_frames(sl, enc, 3, 4, 0.3, 0.7, s)),
        "pool_ctc_prefix_logprobs": ("rnnt_pool_ctc_prefix_logprobs", "active slots", MAX_STREAMS,
                                     lambda sl: eng.pool_ctc_prefix_logprobs(sl, lp, 3, 4, False, s)),
        "pool_wave": ("rnnt_pool_wave", "active slots", MAX_STREAMS, lambda sl: eng.pool_wave(sl, wave, 10, [10] * len(sl), z(sl), fb, 4, stream=s)),
        "pool_rescore": ("rnnt_pool_rescore", "slots", N_STREAMS, lambda sl: _rescore(eng, sl, s)),
    }


ENTRY_POINTS = ("pool_chunk", "pool_chunk_beam", "pool_chunk_ctc_prefix", "pool_chunk_prefix", "pool_prefix_frames", "pool_ctc_prefix_logprobs",
                "pool_wave", "pool_rescore")


def _refused(eng, call, slots):
    n0 = eng.counters()[0]
    with pytest.raises(RnntError) as e:
        call(slots)
    assert e.value.status == ERR_ARG, e.value
    assert eng.counters()[0] == n0, "a refused call launched something"
    return eng.lib.rnnt_last_error(eng.ctx).decode()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_slot_list_refusals(world, name):
    fn, what, limit, call = _calls(world)[name]
    eng = world["eng"]
    assert _refused(eng, call, []) == f"{fn}: 0 {what} of {limit}"
    assert _refused(eng, call, list(range(limit)) + [0]) == f"{fn}: {limit + 1} {what} of {limit}"
    assert _refused(eng, call, [-1]) == f"{fn}: row 0: slot -1 outside [0, {limit})"
    assert _refused(eng, call, [limit]) == f"{fn}: row 0: slot {limit} outside [0, {limit})"
    assert _refused(eng, call, [0, 0]) == f"{fn}: slot 0 listed twice"


def _advance_and_read(w, eng, in_progress):
    """both seams over slots [0, 1], 3 frames, beam 4; in_progress: a second call with another beam size on each search first refuses"""
    s = _stream()
    eng.pool_prefix_frames([0, 1], w["enc"].data_ptr(), 3, 4, 0.3, 0.7, s)
    eng.pool_ctc_prefix_logprobs([0, 1], w["lp"].data_ptr(), 3, 4, False, s)
    if in_progress:
        for call in (lambda: eng.pool_prefix_frames([1], w["enc"].data_ptr(), 3, 5, 0.3, 0.7, s),
                     lambda: eng.pool_ctc_prefix_logprobs([1], w["lp"].data_ptr(), 3, 5, False, s)):
            assert "differ from the search in progress" in _refused(eng, lambda _: call(), None)
    return [(eng.stream_prefix(b, True, s), eng.stream_ctc_prefix(b, False, True, stream=s)) for b in (0, 1)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def test_refusals_change_nothing(world):
    """after every refusal above (run them here too, so the test stands alone), the searches of an engine that was refused equal,
    bit for bit, those of an engine that saw no refused call"""
    for name in ENTRY_POINTS:
        _, _, limit, call = _calls(world)[name]
        for slots in ([], list(range(limit)) + [0], [-1], [limit], [0, 0]):
            _refused(world["eng"], call, slots)
    got = _advance_and_read(world, world["eng"], True)
    want = _advance_and_read(world, world["clean"], False)
    for b, (((gh, g_h, g_c), (gc_h, gc_raw, gc_fr)), ((wh, w_h, w_c), (wc_h, wc_raw, wc_fr))) in enumerate(zip(got, want)):
        assert len(gh) == 4 and [t for t, _ in gh] == [t for t, _ in wh], f"slot {b}: prefix tokens"
        assert np.array_equal(_bits(np.array([sc for _, sc in gh])), _bits(np.array([sc for _, sc in wh]))), f"slot {b}: prefix score bits"
        assert np.array_equal(_bits(g_h), _bits(w_h)) and np.array_equal(_bits(g_c), _bits(w_c)), f"slot {b}: prefix state bits"
        assert gc_fr == wc_fr == 3 and len(gc_h) == len(wc_h) > 0, f"slot {b}: CTC prefix frames / hypotheses"
        for k, (ga, wa) in enumerate(zip(gc_raw, wc_raw)):
            assert ga.shape == wa.shape and np.array_equal(_bits(ga), _bits(wa)), f"slot {b}: CTC prefix result array {k}"
