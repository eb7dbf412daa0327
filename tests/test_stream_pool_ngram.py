"""N-gram shallow fusion per slot of the stream pool on the device (rnnt_pool_ctc_prefix_logprobs_ngram, rnnt_pool_chunk_ctc_prefix_ngram,
rnnt_stream_get_ctc_prefix_ngram; StreamPool.open(ctc_prefix_beam=..., ngram=...)).

The contract under test is the pool search's own: a search fed in pieces is, bit for bit, the one-launch search
(rnnt_ctc_prefix_beam_logprobs_ngram) over the same device rows, whatever the split -- both run the same device function on the same
numbers, so results are compared as bytes.  Needs a real MI355X.  Every refusal here is a host-side check."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_STATE, RnntEngine, RnntError, ngram_walk_host
import ngram_cases as N

pytestmark = pytest.mark.gpu

CHUNK, N_CHUNKS, BEAM, FRAMES = 16, 4, 4, 12        # 16-frame chunks (t' = 3): 12 encoder frames
BIAS = ([[101, 211, 223], [111, 281], [223]], 2.0)
SPLITS = {2: [12], 3: [1] * 12, 4: [5, 7], 5: [3, 3, 3, 3]}
TOKENS = [101, 111, 211, 223, 281, 7, 8, 9]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def _rows_case():
    """[12, VOCAB] rows and an order-3 model over tokens the rows favour, chosen on the CPU by the restatement alone (gap condition
    over the totals with the graph and the model)"""
    model = N.order3(TOKENS, T.VOCAB, 4)
    for seed in range(200):
        x = 2.0 * np.random.default_rng(seed).standard_normal((1, FRAMES, T.VOCAB))
        x[0, :, TOKENS] += 4.0                                       # the search meets the model's tokens and the phrases
        x[0, :, T.BLANK] += 4.0
        lp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
        st = {}
        res = N.reference_of((lp, [FRAMES], T.BLANK, BEAM, BIAS[0], BIAS[1], model), st)
        if N.gap_ok(st) and any(h[3] != 0.0 for h in res[0]) and all(h[4] != 0.0 for h in res[0]):
            return lp, model
    raise AssertionError("no seed satisfies the gap condition")


@pytest.fixture(scope="module")
def world(np_state_dict):
    """seeded weights with a CTC head in a six-slot context, one utterance of four chunks, seeded log-probability rows and a model"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    sd = np_state_dict(0)
    eng = RnntEngine(max_streams=6, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=T.VOCAB,
                     blank_id=T.BLANK, max_beam=0)
    eng.load_state_dict(sd)
    x = torch.from_numpy(T.synth_fbank(1, CHUNK * N_CHUNKS, seed=46))[0].cuda()
    lp, model = _rows_case()
    yield {"sd": sd, "eng": eng, "x": x, "lp": lp, "lp_d": torch.from_numpy(lp[0]).cuda(), "model": model}
    eng.close()


def one_launch(eng, rows, use_ctx, use_ngram=True):
    """the oracle: rnnt_ctc_prefix_beam_logprobs_ngram over device rows [n, V], raw arrays"""
    rows = rows[None].contiguous()
    return eng.ctc_prefix_beam_logprobs_ngram(rows.data_ptr(), [rows.size(1)], 1, rows.size(1), BEAM, use_ctx, use_ngram, True, _stream())[1]


def advance(eng, keep, slot, rows, use_ctx, use_ngram):
    rows = rows[None].contiguous()
    keep.append(rows)                                                # the call does not synchronise: the rows live until the read
    if use_ngram:
        eng.pool_ctc_prefix_logprobs_ngram([slot], rows.data_ptr(), rows.size(1), BEAM, use_ctx, True, _stream())
    else:
        eng.pool_ctc_prefix_logprobs([slot], rows.data_ptr(), rows.size(1), BEAM, use_ctx, _stream())


def test_split_invariance_beside_other_slots(world):
    """four slots that fuse the graph and the model over the same 12 rows in the splits 12 / 12 x 1 / 5 + 7 / 4 x 3, a greedy slot and
    a hot-word-only CTC slot advancing in between"""
    eng, x, lp_d, model = world["eng"], world["x"], world["lp_d"], world["model"]
    s = _stream()
    eng.context_set(*BIAS)
    eng.ngram_set(model)

    def run(with_lm):
        eng.reset(6, s)
        eng.stream_open(0, s)
        keep, at = [], {slot: 0 for slot in SPLITS}
        for k in range(N_CHUNKS):
            chunk = x[k * CHUNK:(k + 1) * CHUNK][None].contiguous()
            keep.append(chunk)
            assert eng.pool_chunk([0], chunk.data_ptr(), CHUNK, [4 * k], [4 * k], True, s) == 3
            if with_lm:
                for slot, split in SPLITS.items():
                    while at[slot] < len(split) and sum(split[:at[slot] + 1]) <= 3 * (k + 1):
                        a = sum(split[:at[slot]])
                        advance(eng, keep, slot, lp_d[a:a + split[at[slot]]], True, True)
                        at[slot] += 1
            advance(eng, keep, 1, lp_d[3 * k:3 * k + 3], True, False)
        hot = eng.stream_ctc_prefix(1, True, True, stream=s)
        return eng.stream_tokens(0, 0, s), hot[1], hot[2], keep

    tokens, hot, hot_frames, _ = run(False)
    tokens_lm, hot_lm, hot_frames_lm, keep = run(True)
    assert tokens == tokens_lm and len(tokens) > 0 and hot_frames == hot_frames_lm == FRAMES
    assert all(same_bits(p, q) for p, q in zip(hot, hot_lm)), "the hot-word slot changed beside slots that fuse a model"
    want = one_launch(eng, lp_d, True)
    assert want[6].all() and want[5].any(), "every hypothesis carries an n-gram score, some a context score"
    for slot in SPLITS:
        hyps, fin, frames = eng.stream_ctc_prefix_ngram(slot, True, True, s)
        assert frames == FRAMES
        for k, (p, q) in enumerate(zip(fin, want)):
            assert same_bits(p, q), f"slot {slot} (split {SPLITS[slot]}): array {k} differs\n{p}\n{q}"
        run_h, run, _ = eng.stream_ctc_prefix_ngram(slot, False, True, s)
        assert all(same_bits(p, q) for p, q in zip(run[:4], fin[:4])), "final = 0: hypotheses, lengths, tokens, times and order"
        for (tok, sc, _, cs, ls), (_, fsc, _, fcs, fls) in zip(run_h, hyps):
            steps, _, eos, _ = ngram_walk_host(model, T.VOCAB, T.BLANK, tok)
            acc = 0.0
            for v in steps:
                acc += float(v)
            assert ls == acc and fls == acc + eos, (slot, tok)           # the running score, and the one with the end term
            assert abs((sc - cs - ls) - (fsc - fcs - fls)) <= 1e-12      # the same log_add(s, ns) under either
    # the old getter reads such a slot with the same totals
    old = eng.stream_ctc_prefix(2, True, True, stream=s)[1]
    assert all(same_bits(p, q) for p, q in zip(old, want[:6]))
    # the model set but not used: bit for bit the entry point without it
    eng.stream_ctc_prefix_reset(3, s)
    whole = lp_d[None].contiguous()
    eng.pool_ctc_prefix_logprobs_ngram([3], whole.data_ptr(), FRAMES, BEAM, True, False, s)
    off = eng.stream_ctc_prefix_ngram(3, True, True, s)[1]
    assert all(same_bits(p, q) for p, q in zip(off[:6], hot)) and not off[6].any()
    del keep


def test_stale_model_generation(world):
    """rnnt_ngram_set mid-utterance: the slot that fuses the model is refused (advance, and the final read) until it is reset, with
    no launch and no state change; the slot that does not goes on; a reset slot runs under the new model"""
    eng, lp_d, model = world["eng"], world["lp_d"], world["model"]
    s = _stream()
    other = N.order3(TOKENS[:5], T.VOCAB, 9, lm_weight=0.9)
    eng.context_set([])
    eng.ngram_set(model)
    eng.stream_ctc_prefix_reset(-1, s)
    keep = []
    advance(eng, keep, 0, lp_d[:5], False, True)
    advance(eng, keep, 1, lp_d[:5], False, False)
    launches = lambda: eng.counters()[0]                                            # noqa: E731
    for bad in (dict(use_ngram=False), dict(beam_size=BEAM - 1)):                    # fixed by the first advancing call
        with pytest.raises(RnntError) as e:
            eng.pool_ctc_prefix_logprobs_ngram([0], lp_d.data_ptr(), 1, **{**dict(beam_size=BEAM, use_context=False, use_ngram=True, stream=s), **bad})
        assert e.value.status == ERR_ARG
    with pytest.raises(RnntError) as e:
        eng.pool_ctc_prefix_logprobs_ngram([1], lp_d.data_ptr(), 1, BEAM, False, True, s)
    assert e.value.status == ERR_ARG
    before = eng.stream_ctc_prefix_ngram(0, False, True, s)
    eng.ngram_set(other)
    n0 = launches()
    with pytest.raises(RnntError) as e:
        eng.pool_ctc_prefix_logprobs_ngram([0], lp_d[5:].contiguous().data_ptr(), 7, BEAM, False, True, s)
    assert e.value.status == ERR_STATE
    with pytest.raises(RnntError) as e:
        eng.pool_ctc_prefix_logprobs_ngram([2, 0], lp_d[5:].contiguous().data_ptr(), 1, BEAM, False, True, s)   # one stale slot refuses the call
    assert e.value.status == ERR_STATE
    with pytest.raises(RnntError) as e:
        eng.stream_ctc_prefix_ngram(0, True, True, s)
    assert e.value.status == ERR_STATE and launches() == n0
    after = eng.stream_ctc_prefix_ngram(0, False, True, s)                           # the running scores are still there
    assert after[2] == before[2] == 5 and all(same_bits(p, q) for p, q in zip(after[1], before[1]))
    assert eng.stream_ctc_prefix_ngram(2, False, True, s)[2] == 0
    advance(eng, keep, 1, lp_d[5:], False, False)
    plain = one_launch(eng, lp_d, False, False)
    assert all(same_bits(p, q) for p, q in zip(eng.stream_ctc_prefix_ngram(1, True, True, s)[1], plain)), "the slot without the model"
    eng.ngram_set(None)
    with pytest.raises(RnntError) as e:
        eng.pool_ctc_prefix_logprobs_ngram([2], lp_d.data_ptr(), 1, BEAM, False, True, s)
    assert e.value.status == ERR_STATE
    eng.ngram_set(other)
    eng.stream_ctc_prefix_reset(0, s)
    advance(eng, keep, 0, lp_d[:5], False, True)
    advance(eng, keep, 0, lp_d[5:], False, True)
    want = one_launch(eng, lp_d, False)
    got = eng.stream_ctc_prefix_ngram(0, True, True, s)[1]
    assert all(same_bits(p, q) for p, q in zip(got, want)), "the reset slot under the new model"
    eng.ngram_set(model)
    assert not all(same_bits(p, q) for p, q in zip(one_launch(eng, lp_d, False), want)), "the two models give the same result"
    del keep


def test_segment_restarts_a_model_slot(world):
    """rnnt_pool_segment puts the start marker back: the next segment equals a fresh slot's search over the same later frames"""
    eng, lp_d, model = world["eng"], world["lp_d"], world["model"]
    s = _stream()
    eng.context_set(*BIAS)
    eng.ngram_set(model)
    eng.reset(6, s)
    keep = []
    advance(eng, keep, 2, lp_d[:6], True, True)
    eng.pool_segment([2], True, s)
    assert eng.stream_ctc_prefix_ngram(2, False, True, s)[2] == 0
    advance(eng, keep, 2, lp_d[6:9], True, True)
    advance(eng, keep, 2, lp_d[9:], True, True)
    advance(eng, keep, 3, lp_d[6:], True, True)
    want = one_launch(eng, lp_d[6:], True)
    seg, fresh = eng.stream_ctc_prefix_ngram(2, True, True, s)[1], eng.stream_ctc_prefix_ngram(3, True, True, s)[1]
    for k, (p, q, w) in enumerate(zip(seg, fresh, want)):
        assert same_bits(p, q) and same_bits(p, w), k
    # rnnt_stream_open and rnnt_streams_reset likewise
    eng.stream_open(2, s)
    advance(eng, keep, 2, lp_d[6:], True, True)
    assert all(same_bits(p, w) for p, w in zip(eng.stream_ctc_prefix_ngram(2, True, True, s)[1], want)), "after rnnt_stream_open"
    eng.reset(6, s)
    assert eng.stream_ctc_prefix_ngram(2, False, True, s)[2] == 0
    advance(eng, keep, 3, lp_d[6:], True, True)
    assert all(same_bits(p, w) for p, w in zip(eng.stream_ctc_prefix_ngram(3, True, True, s)[1], want)), "after rnnt_streams_reset"
    del keep


def test_stream_pool_end_to_end(world):
    """StreamPool in 16-frame chunks: a slot that fuses a model closes with the one-launch search over the rows a one-slot context
    computes for its utterance chunk by chunk; the greedy and the hot-word slot beside it are what they are without it"""
    from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool
    eng, x = world["eng"], world["x"]
    s = _stream()
    eng.reset(1, s)
    rows = torch.empty(3 * N_CHUNKS, T.VOCAB, device="cuda")
    for k in range(N_CHUNKS):
        chunk = x[k * CHUNK:(k + 1) * CHUNK][None].contiguous()
        assert eng.pool_chunk([0], chunk.data_ptr(), CHUNK, [4 * k], [4 * k], False, s) == 3
        nf, stride = ctypes.c_int32(0), ctypes.c_int32(0)
        ptr = eng.lib.rnnt_enc_frames_dev(eng.ctx, ctypes.byref(nf), ctypes.byref(stride))
        assert nf.value == 3
        eng.ctc_logprobs(ptr, 3, rows[3 * k:3 * k + 3].data_ptr(), s)
        eng.frames_discard(s)
    torch.cuda.synchronize()
    eng.context_set([])
    plain = eng.ctc_prefix_beam_logprobs(rows[None].contiguous().data_ptr(), [3 * N_CHUNKS], 1, 3 * N_CHUNKS, BEAM, False, False, s)[0]
    seen = sorted({t for h in plain for t in h[0]})
    assert len(seen) >= 3
    model, bias = N.order3(seen, T.VOCAB, 6, lm_weight=1.0), ContextBias(BIAS[0], BIAS[1])
    pool = StreamPool(world["sd"], 3, vocab_size=T.VOCAB, blank_id=T.BLANK, max_chunk_frames=64, max_cache_frames=256, max_tokens=512, max_beam=0)
    try:
        def run(with_lm):
            pool.reset()
            g, c = pool.open(), pool.open(ctc_prefix_beam=BEAM, context=bias)
            m = pool.open(ctc_prefix_beam=BEAM, ngram=model) if with_lm else None
            inc = []
            for k in range(N_CHUNKS):
                for slot in (g, c) + ((m,) if with_lm else ()):
                    pool.feed(slot, x[k * CHUNK:(k + 1) * CHUNK])
                inc.append(pool.step())
            mid = pool.ctc_hyps(m) if with_lm else None
            return inc, pool.close(g), pool.close(c), mid, pool.close(m) if with_lm else None
        alone, beside = run(False), run(True)
        assert beside[:3] == alone[:3] and len(alone[1]) > 0, "the greedy and the hot-word slot changed beside a slot that fuses a model"
        eng.ngram_set(model)
        want = eng.ctc_prefix_beam_logprobs_ngram(rows[None].contiguous().data_ptr(), [3 * N_CHUNKS], 1, 3 * N_CHUNKS, BEAM, False, True, False, s)[0]
        assert beside[4] == [(h[0], h[1], h[2]) for h in want]
        assert [(h[0], h[2]) for h in beside[3]] == [(h[0], h[2]) for h in beside[4]]
        assert any(h[4] != 0.0 for h in want) and [(h[0], h[1]) for h in want] != [(h[0], h[1]) for h in plain], "the model changed nothing"
    finally:
        pool.engine.close()
