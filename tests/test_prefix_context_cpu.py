"""Hot-word biasing in the transducer prefix beam search, without a GPU: the merge of one frame with a context graph as a pure
function (rnnt_prefix_merge_ctx_host against its Python restatement testing.prefix_merge_ctx_ref), the zero-score graph against the
unbiased merge bit for bit, the new C-ABI symbols against the header and the ctypes table, and the facade over a recording fake
engine.  Survivors, order, source row / slot, context states and context scores exact (both sides form the same f64 sums in the same
order); fused scores within prefix_cases.SCORE_TOL."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.online_rnnt_model import ContextBias, OnlineRNNTModel, StreamPool, pool_plan
from prefix_cases import BLANK, MIN_GAP, SCORE_TOL, cases as plain_cases
from prefix_context_cases import PHRASES, RANDOM, SCORE, assert_same_ctx, cases, graph, total_gap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, DROPPED = cases()
NEW = ("rnnt_prefix_beam_decode_ctx", "rnnt_prefix_merge_ctx_host", "rnnt_prefix_merge_ctx_device", "rnnt_pool_prefix_frames_ctx",
       "rnnt_pool_chunk_prefix_ctx", "rnnt_stream_get_prefix_ctx")


# ---- the merge: host against Python ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_merge_equals_python_restatement(name):
    hyps, top_lp, top_tok, beam = CASES[name]
    want = T.prefix_merge_ctx_ref(hyps, top_lp, top_tok, BLANK, beam, graph())
    assert 1 <= len(want) <= beam
    assert_same_ctx(rlib.prefix_merge_ctx_host(hyps, top_lp, top_tok, BLANK, beam, PHRASES, SCORE), want, SCORE_TOL)


def test_random_cases_keep_their_totals_apart():
    """the condition that defines the order on both sides, checked on the Python restatement alone; at most one case in ten dropped"""
    g = graph()
    kept = [n for n in CASES if n.rsplit("_", 1)[0] in RANDOM] + ["full_16x16x16"]
    assert len(kept) >= 20 and len(DROPPED) * 10 <= len(kept) + len(DROPPED), DROPPED
    for name in kept:
        assert total_gap(g, *CASES[name][:3]) >= MIN_GAP, name


def test_cases_are_what_they_claim():
    """The properties the crafted cases are named for hold for the restatement itself."""
    g = graph()
    ref = lambda name: T.prefix_merge_ctx_ref(*CASES[name][:3], BLANK, CASES[name][3], g)
    plain = lambda name: T.prefix_merge_ref([(h[0], h[1]) for h in CASES[name][0]], *CASES[name][1:3], BLANK, CASES[name][3])
    r = ref("boost_reorders")
    assert [x[0] for x in plain("boost_reorders")] == [[BLANK, 9], [BLANK, 7]] and [x[0] for x in r] == [[BLANK, 7], [BLANK, 9]]
    assert r[0][5] == SCORE + SCORE and r[1][5] == 0.0 and r[1][4] == 0
    r = {tuple(x[0]): x for x in ref("fail_arc_negative")}
    assert CASES["fail_arc_negative"][0][0][3] == SCORE + SCORE
    assert r[(BLANK, 3, 4, 9)][4] == 0 and r[(BLANK, 3, 4, 9)][5] == (SCORE + SCORE) + (0.0 - (SCORE + SCORE)) and g.step(CASES["fail_arc_negative"][0][0][2], 9)[0] < 0
    assert r[(BLANK, 3, 4)][4:] == tuple(CASES["fail_arc_negative"][0][0][2:])                          # the blank copies
    r = {tuple(x[0]): x for x in ref("phrase_completes")}
    done = r[(BLANK, 1, 2, 3)]
    assert g.is_end[done[4]] and g.output[done[4]] >= 0 and done[5] > 3 * SCORE + 1.0                      # token score + two output scores
    for name, src in (("ab_meets_a_plus_b", (0, 0)), ("a_plus_b_meets_ab", (0, 1))):
        hyps = CASES[name][0]
        ab = next(h for h in hyps if h[0] == [BLANK, 1, 2])
        a = next(h for h in hyps if h[0] == [BLANK, 1])
        step, state = g.step(a[2], 2)
        assert (state, a[3] + step) == (ab[2], ab[3]), "both candidates arrive with equal context state and score"
        top = ref(name)[0]
        assert top[0] == [BLANK, 1, 2] and top[2:4] == src and top[4:] == (ab[2], ab[3])
    for name, first in (("equal_totals_low_first", 20), ("equal_totals_high_first", 21)):
        r = ref(name)
        assert [x[1] + x[5] for x in r] == [-1.0, -1.0] and r[0][0][1] == first and [x[2] for x in r] == [0, 1]
    hyps, top_lp, top_tok, beam = CASES["full_16x16x16"]
    assert len(hyps) == 16 and np.asarray(top_lp).shape == (16, 16) and beam == 16 and len(ref("full_16x16x16")) == 16
    assert len({x[4] for x in ref("full_16x16x16")}) > 3                                                  # survivors in several graph states


@pytest.mark.parametrize("name", sorted(plain_cases()))
def test_zero_score_graph_is_the_unbiased_merge(name):
    """context_score = 0.0: survivors, order, source slots and the BITS of the scores of rnnt_prefix_merge_host; all context scores 0"""
    hyps, top_lp, top_tok, beam = plain_cases()[name]
    want = rlib.prefix_merge_host(hyps, top_lp, top_tok, BLANK, beam)
    got = rlib.prefix_merge_ctx_host([(t, s, 0, 0.0) for t, s in hyps], top_lp, top_tok, BLANK, beam, PHRASES, 0.0)
    assert [g[0] for g in got] == [w[0] for w in want] and [g[2:4] for g in got] == [w[2:4] for w in want]
    assert np.array_equal(np.array([g[1] for g in got]).view(np.int64), np.array([w[1] for w in want]).view(np.int64))
    assert all(g[5] == 0.0 for g in got)


def test_host_merge_refuses_bad_arguments():
    one = ([([BLANK], 0.0, 0, 0.0)], np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32), BLANK)
    for kw in (dict(beam=0), dict(phrases=[]), dict(phrases=[[]]), dict(state=99), dict(state=-1)):
        hyps = [([BLANK], 0.0, kw.get("state", 0), 0.0)]
        with pytest.raises(rlib.RnntError):
            rlib.prefix_merge_ctx_host(hyps, *one[1:], kw.get("beam", 1), kw.get("phrases", PHRASES), SCORE)


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
    for w in ("prefix_beam_decode_ctx", "prefix_merge_ctx_device", "pool_prefix_frames_ctx", "pool_chunk_prefix_ctx", "stream_prefix_ctx"):
        assert callable(getattr(rlib.RnntEngine, w))
    assert lib.rnnt_prefix_beam_decode_ctx(None, None, None, 1, 1, 1, 0.3, 0.7, 1, 2, None, None, None, None, None, None, None, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_prefix_frames_ctx(None, 1, None, None, 1, 4, 0.3, 0.7, 1, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_prefix_ctx(None, 0, 1, 1, 1, None, None, None, None, None, None, None, None) == rlib.ERR_ARG


# ---- the facade over a recording fake engine ------------------------------------------------------------------------------------------
class FakeEngine:
    """Records what StreamPool asks of the library; the unbiased calls have the signatures of the engines of the older CPU tests."""

    def __init__(self):
        self.calls, self.graphs, self.opened, self.reads = [], [], [], []

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        self.opened.append(slot)

    def stream_keep_frames(self, slot, keep=True, stream=None):
        pass

    def context_set(self, phrases, context_score=6.0):
        self.graphs.append(([list(p) for p in phrases], context_score))

    def pool_chunk_ctc_prefix(self, slots, ptr, length, offsets, required, beam_size=10, use_context=False, stream=None):
        self.calls.append(("ctc_prefix", list(slots), int(beam_size), bool(use_context)))

    def pool_chunk_prefix(self, slots, ptr, length, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, stream=None):
        self.calls.append(("prefix", list(slots), int(beam_size), (ctc_weight, transducer_weight)))

    def pool_chunk_prefix_ctx(self, slots, ptr, length, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=True, stream=None):
        self.calls.append(("prefix_ctx", list(slots), int(beam_size), (ctc_weight, transducer_weight), bool(use_context)))

    def stream_prefix(self, slot, states=False, stream=None):
        self.reads.append(("plain", slot))
        return [([5, 1], -1.5)]

    def stream_prefix_ctx(self, slot, final=False, states=False, stream=None):
        self.reads.append(("ctx", slot, bool(final)))
        return [([5, 1], -1.5 + (9.0 if final else 6.0), 9.0 if final else 6.0)]

    def stream_ctc_prefix(self, slot, final=False, raw=False, cap_hyps=16, cap_tokens=None, stream=None):
        return [([1], -0.25, [0], 0.0)]

    def pool_rescore(self, slots, n_hyp, hyp_lens, hyp_tokens, stream=None):
        return np.ones((len(slots), int(max(n_hyp))), np.float64)


def test_plan_splits_biased_and_unbiased_prefix_slots():
    prefix = {0: (4, 0.3, 0.7), 1: (4, 0.3, 0.7, True), 2: (4, 0.3, 0.7, False), 3: (4, 0.3, 0.7, True)}
    calls, _, index = pool_plan([(s, 16) for s in range(4)], {}, None, None, prefix)
    assert calls == [(16, [0, 2], [0, 0], 4, "prefix", False, (0.3, 0.7)), (16, [1, 3], [0, 0], 4, "prefix", True, (0.3, 0.7))]
    assert index == [(0, 0), (1, 0), (0, 1), (1, 1)]


def test_stream_pool_routes_biased_prefix_slots():
    fake = FakeEngine()
    pool = StreamPool(None, 4, engine=fake)
    g, g2 = ContextBias([[1, 2]], 6.0), ContextBias([[3]], 2.0)
    b0 = pool.open(prefix_beam=4, prefix_context=g)
    u1 = pool.open(prefix_beam=4)
    assert (b0, u1) == (0, 1) and fake.graphs == [([[1, 2]], 6.0)] and pool._slots[b0].decoder == ("prefix", 4, True, (0.3, 0.7), False)
    for s in (b0, u1):
        assert pool.feed(s, torch.zeros(16, 80))
    pool.step()
    assert fake.calls == [("prefix", [1], 4, (0.3, 0.7)), ("prefix_ctx", [0], 4, (0.3, 0.7), True)]
    # reads: an unbiased slot through the old call, a biased one through the new one
    assert pool.prefix_hyps(u1) == [([5, 1], -1.5)] and pool.prefix_hyps(b0) == [([5, 1], 4.5)]
    assert pool.prefix_hyps(b0, final=True, with_context_scores=True) == [([5, 1], 7.5, 9.0)]
    assert fake.reads == [("plain", 1), ("ctx", 0, False), ("ctx", 0, True)]
    # a second graph is refused without taking a slot while a biased slot of EITHER kind is open
    for kw in (dict(prefix_beam=4, prefix_context=g2), dict(ctc_prefix_beam=4, context=g2)):
        with pytest.raises(rlib.RnntError):
            pool.open(**kw)
        assert fake.opened == [0, 1] and pool._free == [2, 3] and len(fake.graphs) == 1, kw
    c2 = pool.open(ctc_prefix_beam=4, context=g)                      # the current graph serves both kinds
    assert c2 == 2 and len(fake.graphs) == 1
    assert pool.close(b0) == [([5, 1], 7.5)] and b0 not in pool._slots        # close() reads the final totals
    with pytest.raises(rlib.RnntError):
        pool.open(prefix_beam=4, prefix_context=g2)                   # the biased CTC slot still holds the graph
    assert pool._free == [0, 3]
    pool.close(c2)
    assert pool.open(prefix_beam=4, prefix_context=g2) == 0 and fake.graphs[-1] == ([[3]], 2.0)
    # wrong keywords take no slot
    n_open = len(fake.opened)
    for kw in (dict(prefix_context=g2), dict(beam_size=2, prefix_context=g2), dict(ctc_prefix_beam=4, prefix_context=g2),
               dict(prefix_beam=4, context=g2)):
        with pytest.raises(rlib.RnntError):
            pool.open(**kw)
        assert len(fake.opened) == n_open, kw


def test_rescore_reads_the_final_totals_of_a_biased_slot():
    fake = FakeEngine()
    pool = StreamPool(None, 2, engine=fake)
    b0 = pool.open(prefix_beam=4, prefix_context=ContextBias([[1]], 6.0), keep_frames=True)
    out = pool.rescore([b0], 0.5, 0.5)
    assert fake.reads == [("ctx", 0, True)]
    assert out[b0][1][0][:2] == ([1], 7.5)


def test_rescoring_batch_accepts_a_context_for_the_transducer_search(monkeypatch):
    """no ValueError any more: the graph is set, the biased search is called, and its totals are the first-pass scores, as for "ctc" """
    import ctc_vr_amd.online_rnnt_model as M

    class Engine:
        def __init__(self):
            self.calls = []

        def context_set(self, phrases, context_score=6.0):
            self.calls.append(("context_set", [list(p) for p in phrases], context_score))

        def prefix_beam_decode_ctx(self, enc_ptr, enc_lens, B, T, beam_size, cw, tw, use_context, want_states, stream):
            self.calls.append(("prefix_beam_decode_ctx", B, T, beam_size, cw, tw, use_context, want_states))
            return [[([BLANK, 1, 2], -1.0 + 12.0, 12.0), ([BLANK, 9], -0.5, 0.0)]]

        def transducer_nll_nbest(self, enc_ptr, enc_lens, nh, hl, ht, B, T, out, stream):
            return np.array([[2.0, 3.0]])

    monkeypatch.setattr(M, "_stream_ptr", lambda: None)
    m = object.__new__(OnlineRNNTModel)
    m._engine, m._context_bias = Engine(), None
    m._encode_for_scoring = lambda *a: (torch.zeros(1, 3, 256), np.array([3], np.int32), None, None)
    g = ContextBias([[1, 2]], 6.0)
    best, rows = m.rescoring_batch(torch.zeros(1, 19, 80), torch.tensor([19]), beam_size=4, ctc_weight=0.5, transducer_weight=0.5,
                                   beam_search_type="transducer", context=g, search_ctc_weight=0.3, search_transducer_weight=0.7)[0]
    assert m._engine.calls == [("context_set", [[1, 2]], 6.0), ("prefix_beam_decode_ctx", 1, 3, 4, 0.3, 0.7, True, False)]
    assert [(r[0], r[1], r[2]) for r in rows] == [([1, 2], 11.0, -2.0), ([9], -0.5, -3.0)] and best == 0
    assert m._context_bias is g
