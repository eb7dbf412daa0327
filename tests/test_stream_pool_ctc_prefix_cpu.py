"""CTC prefix beam search per slot of the stream pool, without a GPU: the four new C-ABI symbols agree with the header and the ctypes
table, pool_plan keeps CTC prefix slots in calls of their own -- one per (length, kind, beam, use_context) -- without disturbing feed
order or the results of the old argument forms, StreamPool over a recording fake engine routes the three slot kinds, uploads each
ContextBias once and reads final hypotheses on close, and ctc_prefix_beam_ref(finalize=False) returns the running context scores."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool, pool_plan
import ctc_prefix_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_stream_ctc_prefix_reset", "rnnt_pool_ctc_prefix_logprobs", "rnnt_pool_chunk_ctc_prefix", "rnnt_stream_get_ctc_prefix")


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


def test_null_context_is_an_argument_error():
    lib = rlib.load()
    one = np.zeros(1, np.int32)
    p = one.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int32(0)
    assert lib.rnnt_stream_ctc_prefix_reset(None, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_ctc_prefix_logprobs(None, 1, p, p, 1, 4, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_chunk_ctc_prefix(None, 1, p, p, 16, p, p, 4, 0, ctypes.byref(n), None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_ctc_prefix(None, 0, 1, 1, 1, p, p, p, p, p, p, ctypes.byref(n), None) == rlib.ERR_ARG


# ---- pool_plan -------------------------------------------------------------------------------------------------------------------
def test_plan_one_call_per_length_kind_beam_and_use_context():
    # equal lengths: slot 0 greedy, 1 RNN-T beam 4, 2 and 5 CTC prefix (10, biased), 3 CTC prefix (10, plain), 4 CTC prefix (4, biased), 6 greedy
    beams = {0: 0, 1: 4, 6: 0}
    ctc = {2: (10, True), 3: (10, False), 4: (4, True), 5: (10, True)}
    calls, offs, index = pool_plan([(s, 16) for s in range(7)], {s: 8 * s for s in range(7)}, beams, ctc)
    assert calls == [(16, [0, 6], [0, 48], 0, "greedy", False), (16, [1], [8], 4, "beam", False), (16, [4], [32], 4, "ctc_prefix", True),
                     (16, [3], [24], 10, "ctc_prefix", False), (16, [2, 5], [16, 40], 10, "ctc_prefix", True)]
    assert index == [(0, 0), (1, 0), (4, 0), (3, 0), (2, 0), (4, 1), (0, 1)]
    assert offs == {s: 8 * s + 4 for s in range(7)}
    # two lengths of one class are two calls
    calls, _, _ = pool_plan([(2, 16), (5, 24)], {}, beams, ctc)
    assert calls == [(16, [2], [0], 10, "ctc_prefix", True), (24, [5], [0], 10, "ctc_prefix", True)]
    # a slot listed in ctc_prefix is a CTC prefix slot whatever `beams` says of it
    calls, _, _ = pool_plan([(2, 16)], {}, {2: 4}, ctc)
    assert calls == [(16, [2], [0], 10, "ctc_prefix", True)]


def test_plan_keeps_feed_order_and_skips_short_chunks():
    ctc = {0: (10, True), 2: (10, True)}
    queue = [(0, 16), (1, 16), (0, 5), (2, 32), (0, 24), (1, 24), (2, 6), (0, 16)]
    calls, offs, index = pool_plan(queue, {0: 0, 1: 100, 2: 7}, {}, ctc)
    assert calls == [(16, [1], [100], 0, "greedy", False), (16, [0], [0], 10, "ctc_prefix", True), (32, [2], [7], 10, "ctc_prefix", True),
                     (24, [1], [104], 0, "greedy", False), (24, [0], [4], 10, "ctc_prefix", True), (16, [0], [10], 10, "ctc_prefix", True)]
    assert index == [(1, 0), (0, 0), None, (2, 0), (4, 0), (3, 0), None, (5, 0)]
    assert offs == {0: 14, 1: 110, 2: 15}                     # the 5- and 6-frame chunks moved no offset
    seen = {}
    for length, slots, call_offs, *_ in calls:                # per slot: offsets grow in call order = feed order
        for s, o in zip(slots, call_offs):
            assert o >= seen.get(s, -1)
            seen[s] = o


@pytest.mark.parametrize("queue,offsets,beams", [
    ([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40}, {0: 4, 3: 2}),
    ([], {}, {}),
    ([(0, 6), (0, 7), (0, 7)], {0: 3}, {0: 3}),
    ([(s, 16 + 4 * (s % 3)) for s in range(8)] * 2, {s: s for s in range(8)}, {s: s % 3 for s in range(8)}),
])
def test_plan_old_argument_forms_unchanged(queue, offsets, beams):
    """without the new keyword the planner returns what it returned: pinned results, and for every form the calls of the new form
    (an empty ctc_prefix) cut back to the old tuple"""
    full = pool_plan(queue, offsets, beams, {})
    assert all(c[5] is False and c[4] == ("beam" if c[3] > 0 else "greedy") for c in full[0])
    assert pool_plan(queue, offsets, beams) == ([c[:4] for c in full[0]], full[1], full[2])
    plain = pool_plan(queue, offsets, None, {})
    assert pool_plan(queue, offsets) == ([c[:3] for c in plain[0]], plain[1], plain[2])
    assert all(c[3] == 0 and c[4] == "greedy" for c in plain[0])


def test_plan_pinned_results_of_the_old_forms():
    calls, offs, index = pool_plan([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40})
    assert calls == [(16, [2, 0], [0, 8]), (24, [3], [40]), (24, [2], [4]), (31, [0], [12])]
    assert offs == {0: 19, 1: 0, 2: 10, 3: 46}
    assert index == [(0, 0), (0, 1), (2, 0), None, (3, 0), (1, 0)]
    beams = {0: 0, 1: 4, 2: 2, 3: 0, 4: 4}
    calls, offs, index = pool_plan([(s, 16) for s in range(5)], {s: 8 * s for s in range(5)}, beams)
    assert calls == [(16, [0, 3], [0, 24], 0), (16, [2], [16], 2), (16, [1, 4], [8, 32], 4)]
    assert index == [(0, 0), (2, 0), (1, 0), (0, 1), (2, 1)]


# ---- StreamPool over a recording fake engine --------------------------------------------------------------------------------------
class FakeEngine:
    """Records what StreamPool asks of the library.  Greedy: one token per call and slot.  RNN-T beam: one hypothesis growing by a token
    per call.  CTC prefix: one hypothesis growing by a token per call, its score 1.0 when read with final, else 0.0."""

    def __init__(self):
        self.calls = []          # (kind, slots, length, offsets, required, beam, use_context)
        self.reads = []          # (slot, final)
        self.graphs = []         # (phrases, score) of every context_set
        self.opened = []
        self.tokens, self.hyps, self.ctc = {}, {}, {}

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        assert 0 <= slot < self.n
        self.opened.append(slot)
        self.tokens[slot], self.hyps[slot], self.ctc[slot] = [], [([], 0.0)], []

    def context_set(self, phrases, context_score=6.0):
        self.graphs.append(([list(p) for p in phrases], context_score))

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        assert ptr != 0 and greedy
        self.calls.append(("greedy", list(slots), int(length), list(offsets), list(required), 0, False))
        for s in slots:
            self.tokens[s].append(100 * s + len(self.tokens[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def pool_chunk_beam(self, slots, ptr, length, offsets, required, beam_size=4, stream=None):
        assert ptr != 0 and beam_size > 0
        self.calls.append(("beam", list(slots), int(length), list(offsets), list(required), int(beam_size), False))
        for s in slots:
            t, lp = self.hyps[s][0]
            self.hyps[s] = [(t + [1000 * s + len(t)], lp - 0.5)]
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def pool_chunk_ctc_prefix(self, slots, ptr, length, offsets, required, beam_size=10, use_context=False, stream=None):
        assert ptr != 0 and beam_size > 0
        self.calls.append(("ctc_prefix", list(slots), int(length), list(offsets), list(required), int(beam_size), bool(use_context)))
        for s in slots:
            self.ctc[s].append(10 * s + len(self.ctc[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_tokens(self, slot, start=0, stream=None):
        return self.tokens[slot][start:]

    def stream_beam(self, slot, stream=None):
        return list(self.hyps[slot])

    def stream_ctc_prefix(self, slot, final=False, raw=False, cap_hyps=16, cap_tokens=None, stream=None):
        self.reads.append((slot, bool(final)))
        t = list(self.ctc[slot])
        return [(t, 1.0 if final else 0.0, list(range(len(t))), 0.5)]


def test_stream_pool_routes_the_three_slot_kinds():
    fake = FakeEngine()
    pool = StreamPool(None, 5, engine=fake, max_beam=4)
    bias = ContextBias([[7, 8], [9]], 3.0)
    g0 = pool.open()
    b1 = pool.open(beam_size=4)
    c2 = pool.open(ctc_prefix_beam=10, context=bias)
    c3 = pool.open(ctc_prefix_beam=10)
    c4 = pool.open(ctc_prefix_beam=10, context=bias)
    assert (g0, b1, c2, c3, c4) == (0, 1, 2, 3, 4) and fake.opened == [0, 1, 2, 3, 4]
    assert fake.graphs == [([[7, 8], [9]], 3.0)], "one context_set per distinct ContextBias"
    assert pool.ctc_hyps(c2) == [([], 0.0, [])]
    for s in range(5):
        assert pool.feed(s, torch.zeros(16, 80))
    assert not pool.feed(c2, torch.zeros(6, 80))               # the < 7-frame rule of process_single_chunk
    assert pool.feed(c4, torch.zeros(24, 80))
    assert pool.step() == {0: [0]}, "step() returns tokens of the greedy slots only"
    assert fake.calls == [("greedy", [0], 16, [0], [0], 0, False), ("beam", [1], 16, [0], [0], 4, False),
                          ("ctc_prefix", [3], 16, [0], [0], 10, False), ("ctc_prefix", [2, 4], 16, [0, 0], [0, 0], 10, True),
                          ("ctc_prefix", [4], 24, [4], [4], 10, True)]
    fake.reads.clear()
    assert pool.ctc_hyps(c4) == [([40, 41], 0.0, [0, 1])] and pool.ctc_hyps(c3, final=True) == [([30], 1.0, [0])]
    assert fake.reads == [(4, False), (3, True)]
    assert [h.tokens for h in pool.beams(b1)] == [[1000]]
    with pytest.raises(rlib.RnntError):
        pool.ctc_hyps(g0)
    with pytest.raises(rlib.RnntError):
        pool.beams(c2)
    # close() processes a queued chunk first and reads final = True
    n_calls = len(fake.calls)
    pool.feed(c2, torch.zeros(16, 80))
    fake.reads.clear()
    assert pool.close(c2) == [([20, 21], 1.0, [0, 1])]
    assert fake.calls[n_calls:] == [("ctc_prefix", [2], 16, [4], [4], 10, True)] and fake.reads == [(2, True)]
    # the freed slot is reused, as any kind
    assert pool.open() == 2 and pool.step() == {}


def test_context_graphs_of_a_pool():
    fake = FakeEngine()
    pool = StreamPool(None, 3, engine=fake)
    a, b = ContextBias([[1, 2]], 2.0), ContextBias([[3]], 4.0)
    s0 = pool.open(ctc_prefix_beam=4, context=a)
    with pytest.raises(rlib.RnntError):
        pool.open(ctc_prefix_beam=4, context=b)                # a second graph while a biased slot is open
    assert fake.opened == [0] and len(fake.graphs) == 1, "a refused open() takes no slot and uploads nothing"
    s1 = pool.open(ctc_prefix_beam=4)                           # unbiased slots are always welcome
    assert pool.open(ctc_prefix_beam=4, context=a) == 2         # the same graph again: no upload
    assert len(fake.graphs) == 1
    pool.close(s0), pool.close(2)
    assert pool.open(ctc_prefix_beam=4, context=b) == 0         # no biased slot left: the graph is replaced
    assert fake.graphs == [([[1, 2]], 2.0), ([[3]], 4.0)]
    pool.close(0)
    assert pool.open(ctc_prefix_beam=4, context=b) == 0 and len(fake.graphs) == 2
    assert s1 == 1
    # refusals at once
    for bad in (dict(ctc_prefix_beam=4, beam_size=2), dict(ctc_prefix_beam=17), dict(ctc_prefix_beam=-1), dict(context=a)):
        with pytest.raises(rlib.RnntError):
            pool.open(**bad)
    assert pool.open(ctc_prefix_beam=16) == 2
    wide = StreamPool(None, 1, engine=FakeEngine(), vocab_size=600)
    with pytest.raises(rlib.RnntError):
        wide.open(ctc_prefix_beam=4)                            # vocabulary > 512


def test_open_refused_by_the_library_takes_no_slot():
    """a graph the library rejects (an empty phrase, the blank, a token outside the vocabulary) or a slot it cannot open: the pool
    is as before the call -- no slot taken, no graph recorded -- and the next open() gets the slot"""
    class Refusing(FakeEngine):
        bad_graph = bad_open = False

        def context_set(self, phrases, context_score=6.0):
            if self.bad_graph:
                raise rlib.RnntError("rnnt_context_set: phrase 0 is empty (status -1)", rlib.ERR_ARG)
            super().context_set(phrases, context_score)

        def stream_open(self, slot, stream=None):
            if self.bad_open:
                raise rlib.RnntError("rnnt_stream_open: refused (status -5)", rlib.ERR_STATE)
            super().stream_open(slot, stream)
    fake = Refusing()
    pool = StreamPool(None, 2, engine=fake)
    good = ContextBias([[1, 2]], 2.0)
    assert pool.open(ctc_prefix_beam=4, context=good) == 0
    pool.close(0)
    free, opened, ctx = list(pool._free), list(fake.opened), pool._context
    fake.bad_graph = True
    for _ in range(3):                                          # more refusals than the pool has slots
        with pytest.raises(rlib.RnntError):
            pool.open(ctc_prefix_beam=4, context=ContextBias([[]], 2.0))
        assert pool._free == free and fake.opened == opened and pool._context is ctx and pool._slots == {}
    fake.bad_graph, fake.bad_open = False, True
    with pytest.raises(rlib.RnntError):
        pool.open(ctc_prefix_beam=4)
    assert pool._free == free and pool._slots == {}
    fake.bad_open = False
    assert pool.open(ctc_prefix_beam=4, context=good) == 0 and pool.open() == 1 and len(fake.graphs) == 1
    assert pool.close(0) == [([], 1.0, [])]


# ---- the restatement's running context scores ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_ctx", "beam_sixteen"])
def test_ref_running_context_scores(name):
    """finalize=False: every context score is the left-to-right f64 sum of rnnt_context_walk_host's step scores over the hypothesis'
    tokens, exactly; tokens, times and order are those of the default call, whose behaviour is unchanged"""
    lp, lens, blank, beam, phrases, score = C.crafted_cases()[name]
    g = T.context_graph_ref(phrases, score)
    checked = 0
    for b in range(len(lens)):
        fin = T.ctc_prefix_beam_ref(lp[b], lens[b], blank, beam, g)[0]
        assert fin == T.ctc_prefix_beam_ref(lp[b], lens[b], blank, beam, g, None, True)[0]
        run = T.ctc_prefix_beam_ref(lp[b], lens[b], blank, beam, g, finalize=False)[0]
        assert [(h[0], h[2]) for h in run] == [(h[0], h[2]) for h in fin]
        for (tok, sc, _, cs), (_, fsc, _, fcs) in zip(run, fin):
            steps, _, fin_walk = rlib.context_walk_host(phrases, score, tok)
            want = 0.0
            for x in steps:
                want += float(x)
            assert cs == want, (name, b, tok)
            assert fcs == fin_walk
            assert sc - cs == pytest.approx(fsc - fcs, abs=1e-12)   # the same log_add(s, ns) under either context score
            checked += cs != 0.0
    assert checked > 0, "no hypothesis met a phrase"
    plain = T.ctc_prefix_beam_ref(lp[0], lens[0], blank, beam, None, finalize=False)[0]
    assert plain == T.ctc_prefix_beam_ref(lp[0], lens[0], blank, beam, None)[0] and all(h[3] == 0.0 for h in plain)
