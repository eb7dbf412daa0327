"""CTC prefix beam search with a context graph on the device (rnnt_ctc_prefix_beam_logprobs / _decode: one launch per call) against
the host seam rnnt_ctc_prefix_beam_host, the reference's recorded n-best lists, and itself across batch compositions.  Tokens,
times, order, hypothesis counts and zero-fill exact, scores within SCORE_TOL; cases, tolerance and gap condition: ctc_prefix_cases.py."""
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_STATE, RnntEngine, RnntError, ctc_prefix_beam_host
import ctc_prefix_cases as C

pytestmark = pytest.mark.gpu

GOLD = C.golden_cases()
CASES = {**{k: v[0] for k, v in GOLD.items()}, **C.crafted_cases()}
FBANK_SEED = 45      # chosen on the CPU with the oracle: smallest prune / top gap 2.8e-4 at beam 4 (with and without the graph
                     # below), smallest arg-max margin 8.8e-3


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def engines():
    """Contexts without weights and with max_beam = 0, one per (vocabulary, blank)."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    cache = {}

    def get(vocab, blank):
        if (vocab, blank) not in cache:
            cache[vocab, blank] = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=vocab,
                                             blank_id=blank, max_beam=0)
        return cache[vocab, blank]
    yield get
    for e in cache.values():
        e.close()


def device(eng, case, raw=False):
    lp, lens, blank, beam, phrases, score = case
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    eng.context_set(phrases or [], score)
    out = eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), lens, lp.shape[0], lp.shape[1], beam, bool(phrases), raw, _stream())
    del lp_d
    return out


def host(case):
    lp, lens, blank, beam, phrases, score = case
    return ctc_prefix_beam_host(lp, lens, blank, beam, phrases, score)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_host_seam(name, engines):
    case = CASES[name]
    got, raw = device(engines(case[0].shape[2], case[2]), case, raw=True)
    C.assert_same(got, host(case), name)
    C.assert_zero_fill(raw)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_device_equals_the_reference(name, engines):
    case, want = GOLD[name]
    C.assert_same(device(engines(case[0].shape[2], case[2]), case), want, name)


def _same_bits(x, y):
    """bitwise equal; token / time arrays of different widths agree on the common part and are zero beyond it"""
    if x.ndim == 3:
        n = min(x.shape[2], y.shape[2])
        if x[..., n:].any() or y[..., n:].any():
            return False
        x, y = np.ascontiguousarray(x[..., :n]), np.ascontiguousarray(y[..., :n])
    return np.array_equal(x.view(np.uint8), y.view(np.uint8))


def test_batch_independence(engines):
    """a row of the B = 2 call is bitwise its B = 1 call; frames past a row's end (NaN here) and a larger T change nothing"""
    lp, lens, blank, beam, phrases, score = GOLD["v412_blank5_beam4_ctx"][0]
    eng = engines(lp.shape[2], blank)
    _, both = device(eng, (lp, lens, blank, beam, phrases, score), raw=True)
    wide = np.full((2, 40, lp.shape[2]), np.nan, np.float32)
    for b in range(2):
        wide[b, :lens[b]] = lp[b, :lens[b]]
        _, one = device(eng, (lp[b:b + 1], lens[b:b + 1], blank, beam, phrases, score), raw=True)
        assert all(_same_bits(x[b:b + 1], y) for x, y in zip(both, one)), b
    _, grown = device(eng, (wide, lens, blank, beam, phrases, score), raw=True)
    _, again = device(eng, (lp, lens, blank, beam, phrases, score), raw=True)         # a smaller call in the grown buffers
    assert all(_same_bits(x, y) and _same_bits(x, z) for x, y, z in zip(both, grown, again))


def test_graph_lifecycle(np_state_dict):
    """set, search, replace, search, clear; a cleared graph refuses use_context; streaming state is not touched by any of it"""
    eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=T.VOCAB,
                     blank_id=T.BLANK, max_beam=0)
    try:
        eng.load_state_dict(np_state_dict(0))
        lp, lens, blank, beam, phrases, score = GOLD["v412_blank5_beam4_ctx"][0]
        assert (lp.shape[2], blank) == (T.VOCAB, T.BLANK)
        x = torch.from_numpy(T.synth_fbank(1, 64, seed=21)).cuda()
        other = [[10, 11], [7]]

        def stream(between):
            s = _stream()
            eng.reset(1, s)
            for ci in range(2):
                chunk = x[:, ci * 32:(ci + 1) * 32].contiguous()
                eng.encoder_chunk(chunk.data_ptr(), 32, ci * 8, ci * 8, s)
                eng.greedy_decode(s)
                eng.frames_consume(s)
                if ci == 0:
                    between()
            return eng.tokens(s)[0]

        def searches():
            C.assert_same(device(eng, (lp, lens, blank, beam, phrases, score)), host((lp, lens, blank, beam, phrases, score)), "first graph")
            C.assert_same(device(eng, (lp, lens, blank, beam, other, 2.0)), host((lp, lens, blank, beam, other, 2.0)), "second graph")
            lp_d = torch.from_numpy(lp).cuda()
            plain = eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), lens, 2, lp.shape[1], beam, False, False, _stream())   # graph set, not used
            C.assert_same(plain, host((lp, lens, blank, beam, None, 0.0)), "use_context = 0")
            eng.context_set([])
            with pytest.raises(RnntError) as e:
                eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), lens, 2, lp.shape[1], beam, True, False, _stream())
            assert e.value.status == ERR_STATE
        assert stream(lambda: None) == stream(searches)
    finally:
        eng.close()


def _model(np_state_dict):
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=T.BLANK, streaming=False, predictor_dropout=0, ctc_weight=0.3,
                        max_streams=2, max_chunk_frames=128, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=0)
    m.load_state_dict(np_state_dict(0))
    return m


def _encode(m, x, lens):
    """the full-context encoder and the CTC log-probabilities of a padded batch: (enc on the device, valid frames, lp on the host)"""
    enc, enc_lens, _, _ = m._encode_for_scoring(x, lens, torch.zeros(x.size(0), 0, dtype=torch.long), torch.zeros(x.size(0), dtype=torch.long))
    B, tq = enc.size(0), enc.size(1)
    lp_d = torch.empty(B, tq, T.VOCAB, device="cuda")
    m._engine.ctc_logprobs(enc.data_ptr(), B * tq, lp_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    return enc, enc_lens, lp_d.cpu().numpy()


def test_decode_from_encoder_frames(np_state_dict):
    """rnnt_ctc_prefix_beam_decode on seeded weights against rnnt_ctc_logprobs + the host seam on the downloaded log-probabilities,
    with and without a graph; the gap condition is checked on those log-probabilities by the restatement alone"""
    from ctc_vr_amd.online_rnnt_model import ContextBias
    m = _model(np_state_dict)
    x, lens = torch.from_numpy(T.synth_fbank(2, 100, seed=FBANK_SEED)), torch.tensor([100, 77])
    enc, enc_lens, lp = _encode(m, x, lens)
    assert enc_lens.tolist() == [24, 18]
    bias = ContextBias([[101, 211, 223], [111, 281], [223]], 2.0)       # pieces of the unbiased best hypotheses: the search does meet them
    for phrases, score in ((None, 0.0), (bias.phrases, bias.context_score)):
        case, st = (lp, enc_lens, T.BLANK, 4, phrases, score), {}
        C.reference_of(case, st)
        assert st["nonzero_gap"] >= C.MIN_GAP and not st.get("top_ties") and not st.get("prune_ties")
        m._engine.context_set(phrases or [], score)
        got = m._engine.ctc_prefix_beam_decode(enc.data_ptr(), enc_lens, 2, enc.size(1), 4, bool(phrases), False, _stream())
        C.assert_same(got, host(case), "decode")
        assert len(got[0][0][0]) > 5
    got = m.ctc_prefix_beam_search(x, lens, beam_size=4, context=bias)
    C.assert_same(got, host((lp, enc_lens, T.BLANK, 4, bias.phrases, bias.context_score)), "facade")
    assert any(c != 0.0 for _, _, _, c in host((lp, enc_lens, T.BLANK, 4, bias.phrases, bias.context_score))[0])


def test_facade_beam_one_is_greedy(np_state_dict):
    """beam_size = 1 without a context is greedy decoding with merging.  It gives ctc_greedy_search's tokens when every frame's arg-max
    is decided by more than the two calls' log-probabilities can differ by: the smallest top-2 margin over the valid frames is checked
    on the device's own log-probabilities against 5e-4, the bound test_ctc_greedy_search_matches_reference uses."""
    m = _model(np_state_dict)
    x, lens = torch.from_numpy(T.synth_fbank(2, 100, seed=FBANK_SEED)), torch.tensor([100, 77])
    _, enc_lens, lp = _encode(m, x, lens)
    top2 = np.sort(lp, axis=2)[:, :, -2:]
    assert min(float((top2[b, :n, 1] - top2[b, :n, 0]).min()) for b, n in enumerate(enc_lens)) > 5e-4
    got = m.ctc_prefix_beam_search(x, lens, beam_size=1)
    assert [[h[0] for h in row] for row in got] == [[hyp] for hyp in m.ctc_greedy_search(x, lens)]
    assert all(len(row[0][0]) > 5 and len(row[0][2]) == len(row[0][0]) and row[0][2] == sorted(row[0][2]) for row in got)


def test_refusals(engines):
    """decided before any launch: the launch counter does not move"""
    import ctypes
    eng = engines(6, 0)
    lp_d = torch.zeros(2, 3, 6, device="cuda")
    launches = lambda: eng.counters()[0]                                          # noqa: E731
    ok = dict(enc_lens=[3, 2], B=2, T=3, beam_size=2)
    eng.context_set([])
    eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), **ok)
    n0 = launches()
    for bad in (dict(enc_lens=[4, 2]), dict(enc_lens=[-1, 2]), dict(beam_size=0), dict(beam_size=7), dict(beam_size=17)):
        with pytest.raises(RnntError) as e:
            eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), **{**ok, **bad})
        assert e.value.status == ERR_ARG
    with pytest.raises(RnntError) as e:
        eng.ctc_prefix_beam_logprobs(None, **ok)
    assert e.value.status == ERR_ARG
    with pytest.raises(RnntError) as e:
        eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), use_context=True, **ok)
    assert e.value.status == ERR_STATE
    with pytest.raises(RnntError) as e:                                           # no weights: the decode entry point is a state error
        eng.ctc_prefix_beam_decode(lp_d.data_ptr(), **ok)
    assert e.value.status == ERR_STATE
    for phrases in ([[6]], [[0]], [[]], [[1] * 5000]):
        with pytest.raises(RnntError) as e:
            eng.context_set(phrases, 1.0)
        assert e.value.status == ERR_ARG
    # raw call: B < 1, null outputs, cap_tokens below the longest length
    el, nh, ln, sc = np.array([3, 2], np.int32), np.zeros(2, np.int32), np.zeros((2, 2), np.int32), np.zeros((2, 2), np.float64)
    tk, tm = np.zeros((2, 2, 3), np.int32), np.zeros((2, 2, 3), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                               # noqa: E731
    f = eng.lib.rnnt_ctc_prefix_beam_logprobs
    assert f(eng.ctx, lp_d.data_ptr(), p(el), 0, 3, 2, 0, 3, p(nh), p(ln), p(tk), p(tm), p(sc), None, _stream()) == ERR_ARG
    assert f(eng.ctx, lp_d.data_ptr(), p(el), 2, 3, 2, 0, 2, p(nh), p(ln), p(tk), p(tm), p(sc), None, _stream()) == ERR_ARG
    assert f(eng.ctx, lp_d.data_ptr(), p(el), 2, 3, 2, 0, 3, p(nh), p(ln), p(tk), None, p(sc), None, _stream()) == ERR_ARG
    assert f(eng.ctx, lp_d.data_ptr(), p(el), 2, 3, 2, 0, 3, p(nh), p(ln), p(tk), p(tm), p(sc), None, _stream()) == 0   # ctx scores optional
    assert launches() == n0 + 1
    big = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=600, max_beam=0)
    try:
        wide = torch.zeros(1, 1, 600, device="cuda")
        with pytest.raises(RnntError) as e:
            big.ctc_prefix_beam_logprobs(wide.data_ptr(), [1], 1, 1, 2)
        assert e.value.status == ERR_ARG
    finally:
        big.close()
