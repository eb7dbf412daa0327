"""Hot-word biasing in the transducer prefix beam search on the device (rnnt_prefix_beam_decode_ctx, rnnt_prefix_merge_ctx_device;
OnlineRNNTModel.prefix_beam_search_batch(context=...)).  Oracles: rnnt_prefix_merge_ctx_host for the merge seam (itself held to the
Python restatement by test_prefix_context_cpu.py), the facade's host loop prefix_beam_search(context=...) -- the same semantics in
plain Python and f64 on testing.context_graph_ref -- end to end, B = 1 calls for batch independence, and the unbiased call for a
graph whose score is 0.  Utterances of 96 fbank frames = 23 encoder frames.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from prefix_cases import BLANK, SCORE_TOL as MERGE_TOL
from prefix_context_cases import PHRASES, SCORE, assert_same_ctx, cases

pytestmark = pytest.mark.gpu

SCORE_TOL = 2e-3                        # test_prefix_beam.py's bar for the device loop against the host loop
FRAMES, TQ = 96, 23
_MODEL, _PICK = {}, {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)


def model(np_state_dict):
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    if 0 not in _MODEL:
        m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=BLANK, max_streams=8, max_chunk_frames=256,
                            max_cache_frames=128, max_enc_frames=128, max_beam=0)
        m.load_state_dict(np_state_dict(1))
        _MODEL[0] = m
    return _MODEL[0]


def contains(seq, run):
    return any(seq[i:i + len(run)] == run for i in range(len(seq) - len(run) + 1))


def phrases_from(unbiased):
    """the issue's recipe on an unbiased n-best [(tokens incl. the leading blank, score)]: a token run of hypothesis #2 that is not in
    #1 (shortest first; of the next hypothesis that has one when #2 is contained in #1), and [last token of the best, x] with x in
    none of the n-best, so that a survivor ends mid-phrase (a best without a token: the run's first token in its place).  None when
    every hypothesis is contained in the best."""
    first = unbiased[0][0][1:]
    runs = (seq[i:i + n] for seq in (toks[1:] for toks, _ in unbiased[1:]) for n in (1, 2, 3) for i in range(len(seq) - n + 1)
            if not contains(first, seq[i:i + n]))
    run = next(runs, None)
    if run is None:
        return None
    used = {t for toks, _ in unbiased for t in toks} | {BLANK}
    x = next(t for t in range(T.VOCAB) if t not in used)
    return [run, [first[-1] if first else run[0], x]]


def pick(m):
    """(fbank, lens, ContextBias, unbiased host-loop result at beam 4, biased one): the first (fbank seed, context score) for which the
    HOST LOOP alone gives both conditions the test needs -- the biased best differs from the unbiased best, and a survivor's finalized
    context score differs from its running one.  Decided on the Python oracle, never on the device search."""
    from ctc_vr_amd.online_rnnt_model import ContextBias
    if 0 in _PICK:
        return _PICK[0]
    lens = torch.tensor([FRAMES])
    for seed in (73, 74, 75, 76):
        x = torch.from_numpy(T.synth_fbank(1, FRAMES, seed=seed))
        unbiased = m.prefix_beam_search(x, lens, beam_size=4)
        phrases = phrases_from(unbiased) if len(unbiased) >= 2 and len(unbiased[0][0]) >= 2 else None
        if phrases is None:
            continue
        for score in (6.0, 12.0, 24.0):
            g = ContextBias(phrases, score)
            biased = m.prefix_beam_search(x, lens, beam_size=4, context=g)
            cs = list(m._prefix_context_scores)
            if biased[0][0] != unbiased[0][0] and any(run != fin for run, fin in cs):
                print("picked fbank seed", seed, "context score", score, "phrases", phrases)
                _PICK[0] = (x, lens, g, unbiased, biased, cs)
                return _PICK[0]
    raise AssertionError("no seeded input gives both conditions under the Python oracle")


# ---- 1. merge seam ---------------------------------------------------------------------------------------------------------------------
def test_device_merge_equals_host_merge():
    """prefix_merge with the graph (one launch through rnnt_prefix_merge_ctx_device) against rnnt_prefix_merge_ctx_host on the CPU
    test's cases: survivors, order, source slots, context states and context scores exact, fused scores within 1e-12"""
    from ctc_vr_amd.lib import RnntEngine, prefix_merge_ctx_host
    eng = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, max_beam=0)
    try:
        eng.context_set(PHRASES, SCORE)
        for name, (hyps, top_lp, top_tok, beam) in sorted(cases()[0].items()):
            want = prefix_merge_ctx_host(hyps, top_lp, top_tok, BLANK, beam, PHRASES, SCORE)
            got = eng.prefix_merge_ctx_device(hyps, top_lp, top_tok, BLANK, beam, _stream())
            print(name, len(want), max([abs(g[1] - w[1]) for g, w in zip(got, want) if np.isfinite(w[1])] or [0.0]))
            assert_same_ctx(got, want, MERGE_TOL)
    finally:
        eng.close()


# ---- 2. the batched call against the host loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [1, 4, 16])
def test_device_loop_equals_host_loop(beam, np_state_dict):
    """prefix_beam_search_batch(context=g) at B = 1 against the host loop on the same context: tokens, order and context scores
    exact, totals within 2e-3.  The graph comes from the unbiased run at beam 4; under it the host loop's best differs from the
    unbiased best and a survivor's finalized context score differs from its running one (beam 4, where the graph was made)."""
    m = model(np_state_dict)
    x, lens, g, unbiased, biased4, cs4 = pick(m)
    assert biased4[0][0] != unbiased[0][0], "the biased best equals the unbiased best: the case shows nothing"
    assert any(run != fin for run, fin in cs4), "no survivor ends inside a phrase: finalize shows nothing"
    want = m.prefix_beam_search(x, lens, beam_size=beam, context=g)
    want_cs = [fin for _, fin in m._prefix_context_scores]
    got = m.prefix_beam_search_batch(x, lens, beam_size=beam, context=g, with_context_scores=True)[0]
    print(beam, [v for _, v in want], [v for _, v, _ in got], want_cs)
    assert [t for t, _, _ in got] == [t for t, _ in want]
    assert [c for _, _, c in got] == want_cs
    assert max(abs(a - b) for (_, a, _), (_, b) in zip(got, want)) < SCORE_TOL
    plain = m.prefix_beam_search_batch(x, lens, beam_size=beam, context=g)[0]
    assert plain == [(t, v) for t, v, _ in got], "with_context_scores changes only the shape of a hypothesis"


def test_rows_equal_their_single_calls(np_state_dict):
    """B = 3 with lengths 0, 5 and 17 over one rnnt_encoder_full output, beam 16, biased: every row equals its own B = 1 call bit for
    bit (tokens, totals, context scores, h, c); the empty row is [blank] with total 0, context score 0 and the zero state"""
    m = model(np_state_dict)
    _, _, g, _, _, _ = pick(m)
    eng, s = m._engine, _stream()
    m._set_context(g)
    x = torch.from_numpy(T.synth_fbank(3, FRAMES, seed=73)).cuda().contiguous()
    enc = torch.empty(3, TQ, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [FRAMES] * 3, 3, FRAMES, enc.data_ptr(), s) == TQ
    lens = [0, 5, 17]
    hyps, h, c = eng.prefix_beam_decode_ctx(enc.data_ptr(), lens, 3, TQ, 16, 0.3, 0.7, True, True, s)
    assert hyps[0] == [([BLANK], 0.0, 0.0)] and not h[0].any() and not c[0].any()
    assert len(hyps[2]) == 16 and max(len(t) for t, _, _ in hyps[2]) > 1
    for b in range(3):
        one, h1, c1 = eng.prefix_beam_decode_ctx(enc[b:b + 1].contiguous().data_ptr(), lens[b:b + 1], 1, TQ, 16, 0.3, 0.7, True, True, s)
        assert [t for t, _, _ in one[0]] == [t for t, _, _ in hyps[b]], b
        for k in (1, 2):
            assert np.array_equal(bits(np.array([v[k] for v in one[0]])), bits(np.array([v[k] for v in hyps[b]]))), (b, k)
        assert np.array_equal(bits(h1[0]), bits(h[b])) and np.array_equal(bits(c1[0]), bits(c[b])), b


# ---- 3. a graph that scores nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [4, 16])
def test_zero_score_graph_is_the_unbiased_search(beam, np_state_dict):
    """context_score = 0.0: tokens and the bits of the scores of prefix_beam_search_batch() without a context; every context score 0"""
    from ctc_vr_amd.online_rnnt_model import ContextBias
    m = model(np_state_dict)
    x, lens, g, _, _, _ = pick(m)
    want = m.prefix_beam_search_batch(x, lens, beam_size=beam)[0]
    got = m.prefix_beam_search_batch(x, lens, beam_size=beam, context=ContextBias(g.phrases, 0.0), with_context_scores=True)[0]
    assert [t for t, _, _ in got] == [t for t, _ in want]
    assert np.array_equal(bits(np.array([v for _, v, _ in got])), bits(np.array([v for _, v in want])))
    assert all(c == 0.0 for _, _, c in got)
    none = m.prefix_beam_search_batch(x, lens, beam_size=beam, with_context_scores=True)[0]      # no graph at all: the same, context scores 0
    assert [(t, v) for t, v, _ in none] == want and all(c == 0.0 for _, _, c in none)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_use_context_without_a_graph_is_refused_and_changes_nothing(np_state_dict):
    """use_context with no graph set: RNNT_ERR_STATE from the batched call, the merge seam and the pool call, no launch; what the
    context's streaming, beam and pool getters return does not change"""
    from ctc_vr_amd.lib import ERR_STATE, RnntError
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    sb = StreamingBatch(np_state_dict(0), 3, max_chunk_frames=48, max_cache_frames=64, max_enc_frames=64, max_tokens=64, max_beam=16)
    eng, s = sb.engine, _stream()
    try:
        x = torch.from_numpy(T.synth_fbank(3, 40, seed=81)).cuda().contiguous()
        enc = torch.empty(3, 9, 256, device="cuda")
        assert eng.encoder_full(x.data_ptr(), [40, 40, 40], 3, 40, enc.data_ptr(), s) == 9
        sb.reset()
        tq = eng.encoder_chunk(x[:, :23].contiguous().data_ptr(), 23, 0, 0, s)
        eng.greedy_decode(s)
        eng.beam_advance(0, tq, 4, s)
        eng.pool_prefix_frames([1], enc[1:2, :3].contiguous().data_ptr(), 3, 4, 0.3, 0.7, s)      # a pool search in progress, unbiased

        def getters():
            rows = sum(len(eng.beam_hyps(b)) for b in range(3))
            out = [eng.token_counts(s), np.array(sum(eng.tokens(s), [])), eng.enc_frames(s), *eng.beam_states(rows, s)]
            for b in range(3):
                h, c, tok = eng.predictor_state(b, s)
                hy, ph, pc = eng.stream_prefix(b, True, s)
                out += [h, c, np.array([tok]), eng.att_cache(b, s), eng.cnn_cache(b, s), np.array([v for _, v in eng.beam_hyps(b)]),
                        np.array(sum([t for t, _ in eng.beam_hyps(b)], [])), ph, pc, np.array([v for _, v in hy]), np.array(sum([t for t, _ in hy], [])),
                        np.array(eng.stream_prefix_size(b))]
            return out
        before = getters()
        n0 = eng.counters()[0]
        calls = (lambda: eng.prefix_beam_decode_ctx(enc.data_ptr(), [9, 0, 5], 3, 9, 4, 0.3, 0.7, True, False, s),
                 lambda: eng.prefix_merge_ctx_device([([BLANK], 0.0, 0, 0.0)], np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32), BLANK, 1, s),
                 lambda: eng.pool_prefix_frames_ctx([0], enc[:1, :2].contiguous().data_ptr(), 2, 4, 0.3, 0.7, True, s),
                 lambda: eng.pool_prefix_frames_ctx([1], enc[1:2, 3:5].contiguous().data_ptr(), 2, 4, 0.3, 0.7, True, s))
        for call in calls:
            with pytest.raises(RnntError) as e:
                call()
            assert e.value.status == ERR_STATE, e.value
        n1 = eng.counters()[0]
        after = getters()
        assert n1 == n0, "a refused call launched something"
        assert len(before) == len(after) and all(np.array_equal(p, q) for p, q in zip(before, after))
        # the same context still searches, unbiased through either entry point
        a = eng.prefix_beam_decode(enc.data_ptr(), [9, 0, 5], 3, 9, 4, 0.3, 0.7, False, s)
        b = eng.prefix_beam_decode_ctx(enc.data_ptr(), [9, 0, 5], 3, 9, 4, 0.3, 0.7, False, False, s)
        assert [[(t, v) for t, v, _ in row] for row in b] == a and all(cs == 0.0 for row in b for _, _, cs in row)
    finally:
        eng.close()
