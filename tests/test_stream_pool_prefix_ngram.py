"""N-gram shallow fusion in the transducer prefix beam search per slot of the stream pool (rnnt_pool_prefix_frames_ngram,
rnnt_pool_chunk_prefix_ngram, rnnt_stream_get_prefix_ngram; StreamPool.open(prefix_beam=k, prefix_ngram=NgramLM)).

The contract under test is test_stream_pool_prefix_context.py's with a model: a fused search fed in pieces is, bit for bit, the B = 1
one-call search (rnnt_prefix_beam_decode_ngram) over the same frames, whatever the split and whatever the other slots do; a non-final
read returns the running n-gram score and a final one adds the end term; a segment starts the next utterance from the start marker;
and the generation rule: after rnnt_ngram_set a search fused under the older model is refused until its slot is reset.  Results are
compared as bytes.  max_streams <= 4; 15 encoder frames per seam utterance; through the chunk form 96 fbank frames in 16-, 20- and
24-frame chunks (3, 4 and 5 encoder frames each).  Needs a real MI355X.  Nothing here provokes a device fault: every refusal is a host-side check."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_STATE, RnntError
import ngram_cases as NC
import test_prefix_context as PC
import test_stream_pool_prefix as SP

pytestmark = pytest.mark.gpu

BLANK = T.BLANK
N = 15                                  # encoder frames of 64 fbank frames
W = (0.3, 0.7)
SPLITS = {"one_call": [15], "two_calls": [7, 8], "odd_even": [1, 4, 3, 2, 5], "ones": [1] * 15}
bits = PC.bits


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def world(np_state_dict):
    """seeded weights, a three-slot context, the encoder frames [3, 15, 256] of one rnnt_encoder_full call, the model -- order3 over
    the tokens of the unfused beam-4 n-best of the three utterances -- and a graph from the first utterance that gives one"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    sd = np_state_dict(0)
    eng = SP._engine(sd, 3)
    x = torch.from_numpy(T.synth_fbank(3, 64, seed=91)).cuda().contiguous()
    enc = torch.empty(3, N, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [64, 64, 64], 3, 64, enc.data_ptr(), _stream()) == N
    seen, phrases = set(), None
    for utt in range(3):
        unfused = eng.prefix_beam_decode(enc[utt:utt + 1].contiguous().data_ptr(), [N], 1, N, 4, W[0], W[1], False, _stream())[0]
        seen |= {t for toks, _ in unfused for t in toks[1:]}
        phrases = phrases or PC.phrases_from(unfused)
    assert len(seen) >= 3 and phrases is not None
    w = {"sd": sd, "eng": eng, "enc": enc, "x": x, "lm": NC.order3(sorted(seen), T.VOCAB, 5, lm_weight=1.0),
         "other": NC.order3(sorted(seen)[:3], T.VOCAB, 9, lm_weight=0.4), "phrases": phrases, "score": 6.0}
    yield w
    eng.close()


def one_call(eng, rows, beam, use_context=False, use_ngram=True):
    """the oracle: B = 1 rnnt_prefix_beam_decode_ngram over rows [n, 256] -> (hyps [(tokens, total, context score, n-gram score)], h, c)"""
    n = rows.size(0)
    buf = rows[None].contiguous() if n else torch.zeros(1, 1, 256, device="cuda")
    hyps, h, c = eng.prefix_beam_decode_ngram(buf.data_ptr(), [n], 1, max(n, 1), beam, W[0], W[1], use_context, use_ngram, True, _stream())
    return hyps[0], h[0, :len(hyps[0])].copy(), c[0, :len(hyps[0])].copy()


def assert_same(got, want, what):
    (gh, g_h, g_c), (wh, w_h, w_c) = got, want
    assert [v[0] for v in gh] == [v[0] for v in wh], f"{what}: tokens\n{gh}\n{wh}"
    for k, name in ((1, "total"), (2, "context score"), (3, "n-gram score")):
        assert np.array_equal(bits(np.array([v[k] for v in gh])), bits(np.array([v[k] for v in wh]))), f"{what}: {name} bits\n{gh}\n{wh}"
    assert g_h.shape == w_h.shape and np.array_equal(bits(g_h), bits(w_h)), f"{what}: h bits"
    assert np.array_equal(bits(g_c), bits(w_c)), f"{what}: c bits"


def adv(eng, slots, rows, beam, use_context, use_ngram, keep):
    x = torch.stack(rows, 0).contiguous()
    keep.append(x)
    eng.pool_prefix_frames_ngram(slots, x.data_ptr(), x.size(1), beam, W[0], W[1], use_context, use_ngram, _stream())


# ---- 1. split invariance through the seam ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,use_context", [(4, False), (16, True)])
def test_split_invariance(beam, use_context, world):
    """one slot fed the same frames in 1 call, 2 calls, odd and even pieces and one frame per call: the final read of every split is the
    one-call fused search bit for bit (tokens, the three f64 arrays, LSTM states); the running reads are the same bytes for every
    split; final adds the end term to the running n-gram score and nothing else"""
    eng, enc, keep, s, u = world["eng"], world["enc"], [], _stream(), 0
    eng.context_set(world["phrases"], world["score"])
    eng.ngram_set(world["lm"])
    want = one_call(eng, enc[u], beam, use_context)
    running = {}
    for split, cuts in SPLITS.items():
        eng.stream_prefix_reset(-1, s)
        at = 0
        for t in cuts:
            adv(eng, [1], [enc[u, at:at + t]], beam, use_context, True, keep)
            at += t
        assert eng.stream_prefix_size(1) == (beam, N, N + 1)
        assert_same(eng.stream_prefix_ngram(1, True, True, s), want, f"beam {beam} {split}, final")
        running[split] = eng.stream_prefix_ngram(1, False, True, s)
        assert_same(eng.stream_prefix_ngram(1, True, True, s), want, f"beam {beam} {split}, final after a running read")
    for split in SPLITS:
        assert_same(running[split], running["one_call"], f"beam {beam} {split}, running")
    run, fin = running["one_call"][0], want[0]
    ref = NC.ref_model(world["lm"], T.VOCAB, BLANK)
    assert [v[0] for v in run] == [v[0] for v in fin]
    for (toks, rt, rc, rg), (_, ft, fc, fg) in zip(run, fin):
        steps, states, eos = ref.walk(toks[1:])
        acc = 0.0
        for v in steps:
            acc = acc + v
        assert rg == acc and fg == acc + eos, "the running score is the walk's sum, the final one adds the end term"
        assert abs((rt - rc - rg) - (ft - fc - fg)) < 1e-9               # the same fused score under either read
    assert any(f[3] != r[3] for r, f in zip(run, fin)) and any(r[3] != 0.0 for r in run)
    # the getters without the n-gram argument read the same totals
    assert [(t, v, c) for t, v, c, _ in fin] == eng.stream_prefix_ctx(1, True, False, s)
    assert [(t, v) for t, v, _, _ in run] == eng.stream_prefix(1, False, s)


def test_fresh_slot_reads_blank_with_zero_scores(world):
    eng, s = world["eng"], _stream()
    eng.ngram_set(world["lm"])
    eng.stream_prefix_reset(-1, s)
    for final in (False, True):
        hyps, h, c = eng.stream_prefix_ngram(0, final, True, s)
        assert [(v[0], v[1], v[3]) for v in hyps] == [([BLANK], 0.0, 0.0)] and not h.any() and not c.any()


# ---- 2. the chunk form and mixed slots ----------------------------------------------------------------------------------------------------------
def test_chunks_and_mixed_slots_equal_their_solo_runs(world):
    """StreamPool over 96 fbank frames: a fused slot in 16-frame chunks (3 encoder frames each), a fused and biased slot in 24-frame
    chunks (5), an unfused slot in 20- and 16-frame chunks (4 and 3: odd and even frame counts in one pool step) and a greedy slot
    advance in the same step() rounds; each is byte for byte its stand-alone run; a
    fused slot's close() is the one-call fused search over its kept frames; prefix_hyps reads running / final; rescore() takes the
    final totals"""
    from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool
    beam = 5
    x = torch.from_numpy(T.synth_fbank(2, 96, seed=92)).cuda().contiguous()
    g, lm = ContextBias(world["phrases"], world["score"]), world["lm"]
    pool = StreamPool(world["sd"], 4, vocab_size=T.VOCAB, blank_id=BLANK, max_chunk_frames=64, max_cache_frames=256, max_tokens=512)
    cuts = {"fused": [16] * 6, "both": [24] * 4, "plain": [20, 16, 20, 16, 20], "greedy": [16] * 6}
    try:
        def run(kinds):
            pool.reset()
            slots = {}
            for kind in kinds:
                slots[kind] = (pool.open(prefix_beam=beam, prefix_ngram=lm, keep_frames=True) if kind == "fused" else
                               pool.open(prefix_beam=beam, prefix_ngram=lm, prefix_context=g, keep_frames=True) if kind == "both" else
                               pool.open(prefix_beam=beam) if kind == "plain" else pool.open())
            at, mid = {k: 0 for k in kinds}, []
            for k in range(6):
                for kind, slot in slots.items():
                    if k < len(cuts[kind]):
                        t = cuts[kind][k]
                        pool.feed(slot, x[1 if kind == "plain" else 0, at[kind]:at[kind] + t].contiguous())
                        at[kind] += t
                pool.step()
                if "fused" in slots:
                    mid.append((pool.prefix_hyps(slots["fused"], False, True, True), pool.prefix_hyps(slots["fused"], True, True, True)))
            out = {"mid": mid}
            for kind in ("fused", "both"):
                if kind in slots:
                    out[kind + "_frames"] = pool.frames(slots[kind])
                    out[kind + "_rescore"] = pool.rescore([slots[kind]], 0.3, 0.7)[slots[kind]]
            for kind, slot in slots.items():
                out[kind] = pool.close(slot)
            return out
        mixed = run(("fused", "both", "plain", "greedy"))
        for kind in ("fused", "both", "plain", "greedy"):
            alone = run((kind,))
            assert alone[kind] == mixed[kind], kind
            if kind == "fused":
                assert alone["mid"] == mixed["mid"]
        assert len(mixed["fused"]) == beam and len(mixed["plain"]) == beam and len(mixed["greedy"]) > 0
        for kind, use_context in (("fused", False), ("both", True)):
            frames = mixed[kind + "_frames"]
            assert frames.shape == ({"fused": 6 * 3, "both": 4 * 5}[kind], 256)
            want = one_call(pool.engine, frames, beam, use_context)[0]
            assert mixed[kind] == [(t, v) for t, v, _, _ in want], kind
            assert [r[1] for r in mixed[kind + "_rescore"][1]] == [v for _, v, _, _ in want], "rescore() takes the final totals as first scores"
        want = one_call(pool.engine, mixed["fused_frames"], beam)[0]
        run_, fin = mixed["mid"][-1]
        assert fin == want and [v[0] for v in run_] == [v[0] for v in fin]
        assert any(r[3] != f[3] for r, f in zip(run_, fin)), "final adds the end term"
        assert mixed["fused"] != one_call(pool.engine, mixed["fused_frames"], beam, False, False)[0]
    finally:
        pool.engine.close()


# ---- 3. segments ----------------------------------------------------------------------------------------------------------------------------------
def test_segment_starts_the_next_utterance_from_the_start_marker(world):
    """rnnt_pool_segment: the next segment equals the one-call search over the later frames alone; rnnt_stream_open and
    rnnt_streams_reset likewise"""
    eng, enc, keep, s, beam = world["eng"], world["enc"], [], _stream(), 4
    eng.ngram_set(world["lm"])
    eng.reset(3, s)
    for b in range(3):
        eng.stream_open(b, s)
    adv(eng, [2], [enc[0, 0:6]], beam, False, True, keep)
    eng.pool_segment([2], True, s)
    assert eng.stream_prefix_size(2)[1] == 0
    adv(eng, [2], [enc[0, 6:9]], beam, False, True, keep)
    adv(eng, [2], [enc[0, 9:]], beam, False, True, keep)
    want = one_call(eng, enc[0, 6:], beam)
    assert_same(eng.stream_prefix_ngram(2, True, True, s), want, "after rnnt_pool_segment")
    eng.stream_open(2, s)
    adv(eng, [2], [enc[0, 6:]], beam, False, True, keep)
    assert_same(eng.stream_prefix_ngram(2, True, True, s), want, "after rnnt_stream_open")
    eng.reset(3, s)
    adv(eng, [1], [enc[0, 6:]], beam, False, True, keep)
    assert_same(eng.stream_prefix_ngram(1, True, True, s), want, "after rnnt_streams_reset")
    eng.reset(3, s)


# ---- 4. rules -------------------------------------------------------------------------------------------------------------------------------------
def test_ngram_set_mid_utterance_refuses_the_fused_slot_only(world):
    """use_ngram that differs from the slot's search is RNNT_ERR_ARG; after a second rnnt_ngram_set a fused slot's advance and its final
    read are RNNT_ERR_STATE while its running read and an unfused slot go on; nothing is launched by a refusal and every getter's
    output stays; after the slot's reset both work again under the new model"""
    eng, enc, keep, s, beam = world["eng"], world["enc"], [], _stream(), 4
    eng.context_set([], 0.0)
    eng.ngram_set(world["lm"])
    eng.reset(3, s)
    for b in range(3):
        eng.stream_open(b, s)
    adv(eng, [0], [enc[0, 0:4]], beam, False, True, keep)              # slot 0 fused, 4 frames in
    adv(eng, [1], [enc[1, 0:4]], beam, False, False, keep)             # slot 1 unfused
    launches = lambda: eng.counters()[0]                               # noqa: E731
    sizes = lambda: [eng.stream_prefix_size(k) for k in range(3)]      # noqa: E731
    snap = [eng.stream_prefix_ngram(k, False, True, s) for k in range(3)]

    def refused(status, call):
        f0, n0 = sizes(), launches()
        with pytest.raises(RnntError) as e:
            call()
        assert e.value.status == status, e.value
        assert launches() == n0 and sizes() == f0
        for k in range(3):
            assert_same(eng.stream_prefix_ngram(k, False, True, s), snap[k], f"slot {k}, running read after a refusal")
    refused(ERR_ARG, lambda: adv(eng, [0], [enc[0, 4:6]], beam, False, False, keep))                       # the slot's search is fused
    refused(ERR_ARG, lambda: adv(eng, [1], [enc[1, 4:6]], beam, False, True, keep))                        # and this one is not
    refused(ERR_ARG, lambda: adv(eng, [2, 0], [enc[2, 0:2], enc[0, 4:6]], beam, False, False, keep))       # one bad slot refuses the call
    assert "differ" in eng.lib.rnnt_last_error(eng.ctx).decode()
    fin0 = eng.stream_prefix_ngram(0, True, True, s)
    eng.ngram_set(world["other"])                                      # a new generation
    refused(ERR_STATE, lambda: adv(eng, [0], [enc[0, 4:6]], beam, False, True, keep))
    refused(ERR_STATE, lambda: adv(eng, [2, 0], [enc[2, 0:2], enc[0, 4:6]], beam, False, True, keep))
    refused(ERR_STATE, lambda: eng.stream_prefix_ngram(0, True, True, s))
    adv(eng, [1], [enc[1, 4:9]], beam, False, False, keep)             # the unfused slot goes on
    hy, h, c = eng.stream_prefix(1, True, s)
    want = eng.prefix_beam_decode(enc[1:2, :9].contiguous().data_ptr(), [9], 1, 9, beam, W[0], W[1], True, s)
    assert hy == want[0][0] and np.array_equal(bits(h), bits(want[1][0, :len(hy)])) and np.array_equal(bits(c), bits(want[2][0, :len(hy)]))
    snap[1] = eng.stream_prefix_ngram(1, False, True, s)
    eng.ngram_set(None)                                                # no model at all: still refused, still readable
    refused(ERR_STATE, lambda: adv(eng, [0], [enc[0, 4:6]], beam, False, True, keep))
    eng.ngram_set(world["other"])
    eng.stream_prefix_reset(0, s)                                      # the slot restarts: both work again, under the new model
    adv(eng, [0], [enc[0, 0:6]], beam, False, True, keep)
    assert_same(eng.stream_prefix_ngram(0, True, True, s), one_call(eng, enc[0, :6], beam), "slot 0 under the new model")
    eng.ngram_set(world["lm"])                                         # and the first model again gives the first result
    eng.stream_prefix_reset(0, s)
    adv(eng, [0], [enc[0, 0:4]], beam, False, True, keep)
    assert_same(eng.stream_prefix_ngram(0, True, True, s), fin0, "slot 0 under the first model again")
    eng.reset(3, s)


def test_live_device_bytes_return_after_close(np_state_dict):
    """the pool rows, the n-gram rows among them, are counted by rnnt_live_device_bytes and released by rnnt_destroy"""
    base = rlib.live_device_bytes()
    eng = SP._engine(np_state_dict(0), 2)
    s = _stream()
    loaded = rlib.live_device_bytes()
    eng.ngram_set(NC.bi(T.VOCAB, BLANK))
    x = torch.from_numpy(T.synth_fbank(1, 64, seed=93)).cuda().contiguous()
    enc = torch.empty(1, N, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [64], 1, 64, enc.data_ptr(), s) == N
    before = rlib.live_device_bytes()
    eng.pool_prefix_frames_ngram([1], enc[:, :4].contiguous().data_ptr(), 4, 4, W[0], W[1], False, True, s)
    rows = 2 * 16
    assert rlib.live_device_bytes() - before >= 2 * rows * (4 + 8), "the n-gram rows: an int and a double per row and set"
    assert len(eng.stream_prefix_ngram(1, True, False, s)) == 4 and rlib.live_device_bytes() > loaded
    eng.close()
    assert rlib.live_device_bytes() == base
