"""N-gram shallow fusion in the transducer prefix beam search, without a GPU: the merge of one frame with a model (and a graph) as a
pure function (rnnt_prefix_merge_ngram_host against its Python restatement testing.prefix_merge_ngram_ref), the zero-weight model and
"no model" against rnnt_prefix_merge_ctx_host bit for bit, the new C-ABI symbols against the header and the ctypes table, and the
facade over a recording engine.  Survivors, order, source row / slot, context and n-gram states exact; context and n-gram scores
compare with == (both sides form the same f64 sums in the same order); fused scores within prefix_cases.SCORE_TOL."""
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.ngram import NgramLM
from ctc_vr_amd.online_rnnt_model import ContextBias, Decoder, StreamPool, _PLAN_ORDER, pool_plan
import prefix_context_cases as PC
import prefix_ngram_cases as PN
from prefix_ngram_cases import BLANK, MIN_GAP, SCORE_TOL, VOCAB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, SEEDS = PN.cases()
NEW = ("rnnt_prefix_beam_decode_ngram", "rnnt_prefix_merge_ngram_host", "rnnt_prefix_merge_ngram_device", "rnnt_pool_prefix_frames_ngram",
       "rnnt_pool_chunk_prefix_ngram", "rnnt_stream_get_prefix_ngram")
REFS = {m: PN.ref_model(m) for m in PN.MODELS}
LMS = {m: PN.model(m) for m in PN.MODELS}


# ---- the merge: host against Python ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CASES), ids=PN.case_id)
def test_host_merge_equals_python_restatement(key):
    name, mname, with_graph = key
    hyps, top_lp, top_tok, beam = CASES[key]
    want = T.prefix_merge_ngram_ref(hyps, top_lp, top_tok, BLANK, beam, PC.graph() if with_graph else None, REFS[mname])
    assert 1 <= len(want) <= beam
    got = rlib.prefix_merge_ngram_host(hyps, top_lp, top_tok, BLANK, beam, PN.PHRASES if with_graph else None, PN.SCORE, LMS[mname], VOCAB)
    PN.assert_same_ngram(got, want, SCORE_TOL)


def test_every_case_keeps_its_totals_apart():
    """the condition that defines the order on both sides, checked on the Python restatement alone; most cases need no re-seeding"""
    g = PC.graph()
    assert len(CASES) == 2 * len(PN.MODELS) * len(PC.cases()[0]) and len(PN.MODELS) == 5
    for key, (hyps, top_lp, top_tok, _) in CASES.items():
        assert PN.total_gap(g if key[2] else None, REFS[key[1]], hyps, top_lp, top_tok) >= MIN_GAP, key
    assert sum(1 for r in SEEDS.values() if r == 0) * 2 >= len(SEEDS)


def test_hypotheses_hold_walked_states_and_the_blank_holds_the_marker():
    seen_marker = seen_walked = False
    for (name, mname, _), (hyps, _, _, _) in CASES.items():
        for toks, _, _, _, nst, ns in hyps:
            steps, states, _ = REFS[mname].walk(toks[1:])
            if len(toks) == 1:
                assert (nst, ns) == (T.NG_START, 0.0)
                seen_marker = True
            else:
                assert nst == states[-1] and nst >= 0
                seen_walked = True
    assert seen_marker and seen_walked


def test_the_model_term_moves_the_order_and_backs_off():
    """what the new key is for: with a model some case's survivors differ from the unfused ones, and some candidate's step backs off"""
    moved = deep_backoff = 0
    for (name, mname, with_graph), (hyps, top_lp, top_tok, beam) in CASES.items():
        if mname == "weight0":
            continue
        g = PC.graph() if with_graph else None
        a = T.prefix_merge_ngram_ref(hyps, top_lp, top_tok, BLANK, beam, g, REFS[mname])
        b = T.prefix_merge_ngram_ref(hyps, top_lp, top_tok, BLANK, beam, g, None)
        moved += [x[0] for x in a] != [x[0] for x in b]
        deep_backoff += any(x[3] == 1 and x[6] == 0 for x in a)      # a token the model has no n-gram for lands in the root
    assert moved > 10 and deep_backoff > 10


@pytest.mark.parametrize("key", sorted(k for k in CASES if k[1] == "weight0"), ids=PN.case_id)
def test_zero_weight_model_and_no_model_are_the_context_merge(key):
    """lm_weight = 0, length_bonus = 0 and n_ngrams = 0: survivors, order, source slots, context values and the BITS of the scores of
    rnnt_prefix_merge_ctx_host (with the graph) or rnnt_prefix_merge_host (without); all n-gram scores 0"""
    name, _, with_graph = key
    hyps, top_lp, top_tok, beam = CASES[key]
    if with_graph:
        want = rlib.prefix_merge_ctx_host([h[:4] for h in hyps], top_lp, top_tok, BLANK, beam, PN.PHRASES, PN.SCORE)
    else:
        want = [w + (0, 0.0) for w in rlib.prefix_merge_host([h[:2] for h in hyps], top_lp, top_tok, BLANK, beam)]
    for lm in (LMS["weight0"], None):
        got = rlib.prefix_merge_ngram_host(hyps, top_lp, top_tok, BLANK, beam, PN.PHRASES if with_graph else None, PN.SCORE, lm, VOCAB)
        assert [g[0] for g in got] == [w[0] for w in want] and [g[2:5] for g in got] == [w[2:5] for w in want]
        bits = lambda rows, i: np.array([r[i] for r in rows], np.float64).view(np.int64)
        assert np.array_equal(bits(got, 1), bits(want, 1)) and np.array_equal(bits(got, 5), bits(want, 5))
        assert all(g[7] == 0.0 for g in got)
        if lm is None:
            assert all(g[6] == T.NG_START for g in got)


def test_host_merge_refuses_bad_arguments():
    lp, tok = np.zeros((1, 1), np.float32), np.array([[1]], np.int32)
    ok = [([BLANK], 0.0, 0, 0.0, T.NG_START, 0.0)]
    assert len(rlib.prefix_merge_ngram_host(ok, lp, tok, BLANK, 1, None, 0.0, LMS["bi"], VOCAB)) == 1
    nodes = len(REFS["bi"].W)
    for hyps, t, beam in (([([BLANK], 0.0, 0, 0.0, nodes, 0.0)], tok, 1), ([([BLANK], 0.0, 0, 0.0, -2, 0.0)], tok, 1), (ok, tok, 0),
                          (ok, np.array([[VOCAB]], np.int32), 1), (ok, np.array([[-1]], np.int32), 1)):
        with pytest.raises(rlib.RnntError):
            rlib.prefix_merge_ngram_host(hyps, lp, t, BLANK, beam, None, 0.0, LMS["bi"], VOCAB)
    with pytest.raises(rlib.RnntError):                                # a context state outside the graph
        rlib.prefix_merge_ngram_host([([BLANK], 0.0, 99, 0.0, T.NG_START, 0.0)], lp, tok, BLANK, 1, PN.PHRASES, PN.SCORE, LMS["bi"], VOCAB)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_signatures_and_library():
    src = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = rlib.load()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rnnt_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in rlib.SIGNATURES, f"{name} is missing from lib.SIGNATURES"
        res, args = rlib.SIGNATURES[name]
        assert res is rlib.c_i32 and len(args) == n_args, f"{name}: header has {n_args} arguments, SIGNATURES {len(args)}"
        assert hasattr(lib, name), f"librnnt_hip.so does not export {name}"
    assert lib.rnnt_abi_version() == 3
    for w in ("prefix_beam_decode_ngram", "prefix_merge_ngram_device", "pool_prefix_frames_ngram", "pool_chunk_prefix_ngram", "stream_prefix_ngram"):
        assert callable(getattr(rlib.RnntEngine, w))
    assert lib.rnnt_prefix_beam_decode_ngram(None, None, None, 1, 1, 1, 0.3, 0.7, 0, 1, 2, *[None] * 9) == rlib.ERR_ARG
    assert lib.rnnt_pool_prefix_frames_ngram(None, 1, None, None, 1, 4, 0.3, 0.7, 0, 1, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_prefix_ngram(None, 0, 1, 1, 1, *[None] * 9) == rlib.ERR_ARG


# ---- the facade over a recording engine -------------------------------------------------------------------------------------------------
GRAMS = [((1,), -1.0, -0.5), ((2,), -2.0, -0.25), ((1, 2), -0.5, 0.0)]


class Engine:
    """The engine methods StreamPool drives for transducer prefix and CTC prefix slots, with the positional arguments the facade passes;
    one ordered log (data pointers and streams left out)."""

    def __init__(self):
        self.log, self.n = [], {}

    def _say(self, *entry):
        self.log.append(entry)

    def reset(self, n, stream):
        self._say("reset", n)

    def context_set(self, phrases, context_score):
        self._say("context_set", [list(p) for p in phrases], context_score)

    def ngram_set(self, ngram):
        self._say("ngram_set", ngram.lm_weight)

    def stream_open(self, slot, stream):
        self._say("stream_open", slot)
        self.n[slot] = 0

    def stream_keep_frames(self, slot, keep, stream):
        self._say("stream_keep_frames", slot, keep)

    def _advance(self, name, slots, ptr, length, offsets, required, *rest):
        assert ptr != 0
        self._say(name, list(slots), length, list(offsets), list(required), *rest)
        for s in slots:
            self.n[s] += 1

    def pool_chunk_ctc_prefix_ngram(self, slots, ptr, length, offsets, required, beam_size, use_context, use_ngram, stream):
        self._advance("pool_chunk_ctc_prefix_ngram", slots, ptr, length, offsets, required, beam_size, use_context, use_ngram)

    def pool_chunk_prefix(self, slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, stream):
        self._advance("pool_chunk_prefix", slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight)

    def pool_chunk_prefix_ctx(self, slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context, stream):
        self._advance("pool_chunk_prefix_ctx", slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context)

    def pool_chunk_prefix_ngram(self, slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context, use_ngram, stream):
        self._advance("pool_chunk_prefix_ngram", slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context, use_ngram)

    def _tokens(self, slot):
        return [5] + [10 * slot + k for k in range(self.n[slot])]

    def stream_ctc_prefix_ngram(self, slot, final, *, stream):
        self._say("stream_ctc_prefix_ngram", slot, final)
        return [(self._tokens(slot)[1:], 2.0 if final else -1.0, list(range(self.n[slot])), 0.5, -0.25)]

    def stream_prefix(self, slot, *, stream):
        self._say("stream_prefix", slot)
        return [(self._tokens(slot), -1.5)]

    def stream_prefix_ctx(self, slot, final, *, stream):
        self._say("stream_prefix_ctx", slot, final)
        c = 9.0 if final else 6.0
        return [(self._tokens(slot), -1.5 + c, c)]

    def stream_prefix_ngram(self, slot, final, *, stream):
        self._say("stream_prefix_ngram", slot, final)
        c, g = (9.0, -3.0) if final else (6.0, -2.0)
        return [(self._tokens(slot), -1.5 + c + g, c, g), (self._tokens(slot) + [7], -2.5 + g, 0.0, g)]

    def pool_segment(self, slots, keep_encoder, stream):
        self._say("pool_segment", list(slots), keep_encoder)

    def pool_rescore(self, slots, n_hyp, hyp_lens, hyp_tokens, stream):
        self._say("pool_rescore", list(slots), np.asarray(n_hyp).tolist())
        return np.ones((len(slots), int(max(n_hyp))), np.float64)


def test_a_fused_prefix_slot_is_opened_advanced_and_read_through_the_ngram_calls():
    eng = Engine()
    pool = StreamPool(None, 4, engine=eng)
    lm = NgramLM(GRAMS, lm_weight=0.4)
    f0 = pool.open(prefix_beam=4, prefix_ngram=lm)
    u1 = pool.open(prefix_beam=4)
    f2 = pool.open(prefix_beam=4, prefix_ngram=lm, prefix_context=ContextBias([[1, 2]], 6.0))
    assert (f0, u1, f2) == (0, 1, 2)
    assert pool._slots[f0].decoder == Decoder("prefix", 4, False, (0.3, 0.7), True) == ("prefix", 4, False, (0.3, 0.7), True)
    assert pool._slots[f0].decoder.plan_kind == "prefix_ngram" and _PLAN_ORDER[-1] == "prefix_ngram"
    assert [e for e in eng.log if e[0] == "ngram_set"] == [("ngram_set", 0.4)]                # once: the pool's one model serves both slots
    for _ in range(2):
        for s in (f0, u1, f2):
            assert pool.feed(s, torch.zeros(16, 80))
    pool.step()
    calls = [e for e in eng.log if e[0].startswith("pool_chunk")]
    assert calls == [
        ("pool_chunk_prefix", [1], 16, [0], [0], 4, 0.3, 0.7),
        ("pool_chunk_prefix_ngram", [0], 16, [0], [0], 4, 0.3, 0.7, False, True),            # fused and unfused: two calls, prefix_ngram last
        ("pool_chunk_prefix_ngram", [2], 16, [0], [0], 4, 0.3, 0.7, True, True),
        ("pool_chunk_prefix", [1], 16, [4], [4], 4, 0.3, 0.7),
        ("pool_chunk_prefix_ngram", [0], 16, [4], [4], 4, 0.3, 0.7, False, True),
        ("pool_chunk_prefix_ngram", [2], 16, [4], [4], 4, 0.3, 0.7, True, True)]
    eng.log.clear()
    assert pool.prefix_hyps(u1) == [([5, 10, 11], -1.5)]
    assert pool.prefix_hyps(f0) == [([5, 0, 1], 2.5), ([5, 0, 1, 7], -4.5)]
    assert pool.prefix_hyps(f0, final=True) == [([5, 0, 1], 4.5), ([5, 0, 1, 7], -5.5)]
    assert pool.prefix_hyps(f0, final=True, with_ngram_scores=True) == [([5, 0, 1], 4.5, -3.0), ([5, 0, 1, 7], -5.5, -3.0)]
    assert pool.prefix_hyps(f2, True, True, True) == [([5, 20, 21], 4.5, 9.0, -3.0), ([5, 20, 21, 7], -5.5, 0.0, -3.0)]
    assert pool.close(f0) == [([5, 0, 1], 4.5), ([5, 0, 1, 7], -5.5)]
    assert eng.log == [("stream_prefix", 1), ("stream_prefix_ngram", 0, False), ("stream_prefix_ngram", 0, True), ("stream_prefix_ngram", 0, True),
                       ("stream_prefix_ngram", 2, True), ("stream_prefix_ngram", 0, True)], "every read of a fused slot, close()'s included"


def test_the_new_refusals_and_the_one_model_rule():
    eng = Engine()
    pool = StreamPool(None, 4, engine=eng)
    lm, lm2 = NgramLM(GRAMS, lm_weight=0.4), NgramLM(GRAMS, lm_weight=0.9)
    for kw, msg in ((dict(prefix_ngram=lm), "stream pool: prefix_ngram needs prefix_beam"),
                    (dict(beam_size=2, prefix_ngram=lm), "stream pool: prefix_ngram needs prefix_beam"),
                    (dict(ctc_prefix_beam=4, prefix_ngram=lm), "stream pool: prefix_ngram needs prefix_beam"),
                    (dict(prefix_beam=4, ngram=lm), "stream pool: ngram needs ctc_prefix_beam")):
        with pytest.raises(rlib.RnntError) as e:
            pool.open(**kw)
        assert str(e.value) == msg and not [x for x in eng.log if x[0] in ("stream_open", "ngram_set")], kw
    f0 = pool.open(prefix_beam=4, prefix_ngram=lm)
    one_model = "stream pool: another n-gram model is in use by an open slot (one model per pool at a time)"
    for kw in (dict(prefix_beam=4, prefix_ngram=lm2), dict(ctc_prefix_beam=4, ngram=lm2)):  # a second model while a fused slot is open
        with pytest.raises(rlib.RnntError) as e:
            pool.open(**kw)
        assert str(e.value) == one_model and pool._free == [1, 2, 3]
    c1 = pool.open(ctc_prefix_beam=4, ngram=lm)                        # the current model serves both searches
    assert c1 == 1 and len([x for x in eng.log if x[0] == "ngram_set"]) == 1
    pool.close(f0)
    with pytest.raises(rlib.RnntError):
        pool.open(prefix_beam=4, prefix_ngram=lm2)                     # the fused CTC slot still holds the model
    pool.close(c1)
    assert pool.open(prefix_beam=4, prefix_ngram=lm2) == 0 and [x for x in eng.log if x[0] == "ngram_set"][-1] == ("ngram_set", 0.9)


def test_rescore_reads_the_final_totals_of_a_fused_slot():
    eng = Engine()
    pool = StreamPool(None, 2, engine=eng)
    f0 = pool.open(prefix_beam=4, prefix_ngram=NgramLM(GRAMS), keep_frames=True)
    out = pool.rescore([f0], 0.5, 0.5)
    assert ("stream_prefix_ngram", 0, True) in eng.log
    assert [r[:2] for r in out[f0][1]] == [([], 4.5), ([7], -5.5)]


def test_pool_plan_is_unchanged_without_the_fifth_element():
    queue = [(s, 16) for s in range(5)] + [(0, 24)]
    prefix = {0: (4, 0.3, 0.7), 1: (4, 0.3, 0.7, True), 2: (4, 0.3, 0.7, False), 3: (2, 0.0, 1.0)}
    calls, offs, index = pool_plan(queue, {}, {4: 3}, {}, prefix)
    assert calls == [(16, [4], [0], 3, "beam", False, None), (16, [3], [0], 2, "prefix", False, (0.0, 1.0)),
                     (16, [0, 2], [0, 0], 4, "prefix", False, (0.3, 0.7)), (16, [1], [0], 4, "prefix", True, (0.3, 0.7)),
                     (24, [0], [4], 4, "prefix", False, (0.3, 0.7))]
    assert offs == {0: 10, 1: 4, 2: 4, 3: 4, 4: 4} and index == [(2, 0), (3, 0), (2, 1), (1, 0), (0, 0), (4, 0)]
    # with it: a class of its own, after every other kind of the same length
    fused = {**prefix, 2: (4, 0.3, 0.7, False, True), 5: (4, 0.3, 0.7, True, True)}
    calls, _, _ = pool_plan(queue + [(5, 16), (6, 16)], {}, {4: 3}, {6: (4, False)}, fused, ngram={6})
    assert [c[4] for c in calls if c[0] == 16] == ["beam", "prefix", "prefix", "prefix", "ctc_prefix_ngram", "prefix_ngram", "prefix_ngram"]
    assert [(c[1], c[5]) for c in calls if c[4] == "prefix_ngram"] == [([2], False), ([5], True)]
    assert _PLAN_ORDER[:5] == ("greedy", "beam", "ctc_prefix", "prefix", "ctc_prefix_ngram")
