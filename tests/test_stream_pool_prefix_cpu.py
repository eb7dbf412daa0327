"""Transducer prefix beam search per slot of the stream pool, without a GPU: the four new C-ABI symbols agree with the header and the
ctypes table, pool_plan keeps prefix slots in calls of their own -- one per (length, beam, weights) -- without disturbing the results
of the old argument forms, and StreamPool over a recording fake engine opens, routes, reads, closes and re-scores such slots."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool, pool_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_stream_prefix_reset", "rnnt_pool_prefix_frames", "rnnt_pool_chunk_prefix", "rnnt_stream_get_prefix")


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
    for w in ("pool_prefix_frames", "pool_chunk_prefix", "stream_prefix", "stream_prefix_reset"):
        assert callable(getattr(rlib.RnntEngine, w))


def test_null_context_is_an_argument_error():
    lib = rlib.load()
    one = np.zeros(3, np.int32)
    p = one.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int32(0)
    assert lib.rnnt_stream_prefix_reset(None, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_prefix_frames(None, 1, p, p, 1, 4, 0.3, 0.7, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_chunk_prefix(None, 1, p, p, 16, p, p, 4, 0.3, 0.7, ctypes.byref(n), None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_prefix(None, 0, 1, 1, p, p, p, p, None, None, None) == rlib.ERR_ARG


# ---- pool_plan -------------------------------------------------------------------------------------------------------------------
def test_plan_one_call_per_length_beam_and_weights():
    # equal lengths: slot 0 greedy, 1 RNN-T beam 4, 2 CTC prefix, 3 and 6 prefix (5, .3, .7), 4 prefix (5, 0, 1), 5 prefix (10, .3, .7)
    beams = {0: 0, 1: 4}
    ctc = {2: (10, True)}
    prefix = {3: (5, 0.3, 0.7), 4: (5, 0.0, 1.0), 5: (10, 0.3, 0.7), 6: (5, 0.3, 0.7)}
    calls, offs, index = pool_plan([(s, 16) for s in range(7)], {s: 8 * s for s in range(7)}, beams, ctc, prefix)
    assert calls == [(16, [0], [0], 0, "greedy", False, None), (16, [1], [8], 4, "beam", False, None), (16, [2], [16], 10, "ctc_prefix", True, None),
                     (16, [4], [32], 5, "prefix", False, (0.0, 1.0)), (16, [3, 6], [24, 48], 5, "prefix", False, (0.3, 0.7)),
                     (16, [5], [40], 10, "prefix", False, (0.3, 0.7))]
    assert index == [(0, 0), (1, 0), (2, 0), (4, 0), (3, 0), (5, 0), (4, 1)]
    assert offs == {s: 8 * s + 4 for s in range(7)}
    # two lengths of one class are two calls; feed order per slot is kept across rounds; a short chunk moves nothing
    calls, offs, index = pool_plan([(3, 16), (6, 24), (3, 5), (3, 24)], {3: 0, 6: 0}, beams, ctc, prefix)
    assert calls == [(16, [3], [0], 5, "prefix", False, (0.3, 0.7)), (24, [6], [0], 5, "prefix", False, (0.3, 0.7)),
                     (24, [3], [4], 5, "prefix", False, (0.3, 0.7))]
    assert index == [(0, 0), (1, 0), None, (2, 0)] and offs == {3: 10, 6: 6}
    # a slot listed in prefix is a prefix slot whatever the other tables say of it
    calls, _, _ = pool_plan([(3, 16)], {}, {3: 4}, {3: (10, False)}, prefix)
    assert calls == [(16, [3], [0], 5, "prefix", False, (0.3, 0.7))]
    # weights that differ only in one of the two split the call
    calls, _, _ = pool_plan([(0, 16), (1, 16), (2, 16)], {}, None, None, {0: (4, 0.3, 0.7), 1: (4, 0.3, 0.6), 2: (4, 0.2, 0.7)})
    assert [c[1] for c in calls] == [[2], [1], [0]] and [c[6] for c in calls] == [(0.2, 0.7), (0.3, 0.6), (0.3, 0.7)]


@pytest.mark.parametrize("queue,offsets,beams", [
    ([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40}, {0: 4, 3: 2}),     # test_stream_pool_cpu.py's
    ([], {}, {}),
    ([(0, 6), (0, 7), (0, 7)], {0: 3}, {0: 3}),
    ([(s, 16 + 4 * (s % 3)) for s in range(8)] * 2, {s: s for s in range(8)}, {s: s % 3 for s in range(8)}),
])
def test_plan_old_argument_forms_unchanged(queue, offsets, beams):
    """without the new argument the planner returns what it returned: for every older form, the calls of the new form (an empty
    prefix) cut back to the older tuple"""
    ctc = {2: (10, True)}
    full = pool_plan(queue, offsets, beams, ctc, {})
    assert all(c[6] is None and c[4] != "prefix" for c in full[0])
    assert pool_plan(queue, offsets, beams, ctc) == ([c[:6] for c in full[0]], full[1], full[2])
    nob = pool_plan(queue, offsets, beams, None, {})
    assert pool_plan(queue, offsets, beams) == ([c[:4] for c in nob[0]], nob[1], nob[2])
    plain = pool_plan(queue, offsets, None, None, {})
    assert pool_plan(queue, offsets) == ([c[:3] for c in plain[0]], plain[1], plain[2])


def test_plan_pinned_results_of_the_old_forms():
    calls, offs, index = pool_plan([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40})
    assert calls == [(16, [2, 0], [0, 8]), (24, [3], [40]), (24, [2], [4]), (31, [0], [12])]
    assert offs == {0: 19, 1: 0, 2: 10, 3: 46}
    assert index == [(0, 0), (0, 1), (2, 0), None, (3, 0), (1, 0)]
    beams = {0: 0, 1: 4, 2: 2, 3: 0, 4: 4}
    calls, _, index = pool_plan([(s, 16) for s in range(5)], {s: 8 * s for s in range(5)}, beams)
    assert calls == [(16, [0, 3], [0, 24], 0), (16, [2], [16], 2), (16, [1, 4], [8, 32], 4)]
    assert index == [(0, 0), (2, 0), (1, 0), (0, 1), (2, 1)]
    calls, _, _ = pool_plan([(0, 16), (1, 16)], {}, {0: 0}, {1: (10, True)})
    assert calls == [(16, [0], [0], 0, "greedy", False), (16, [1], [0], 10, "ctc_prefix", True)]


# ---- StreamPool over a recording fake engine --------------------------------------------------------------------------------------
class FakeEngine:
    """Records what StreamPool asks of the library.  Greedy: one token per call and slot.  Prefix: two hypotheses per slot, both with
    the leading blank 5, growing by a token per call; scores -1.5 and -2.5.  CTC prefix: one hypothesis growing by a token per call."""

    def __init__(self):
        self.calls, self.reads, self.opened, self.kept, self.rescored = [], [], [], [], []
        self.tokens, self.pre, self.ctc = {}, {}, {}

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        assert 0 <= slot < self.n
        self.opened.append(slot)
        self.tokens[slot], self.pre[slot], self.ctc[slot] = [], [], []

    def stream_keep_frames(self, slot, keep=True, stream=None):
        self.kept.append(slot)

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        self.calls.append(("greedy", list(slots), int(length), list(offsets), list(required), 0, None))
        for s in slots:
            self.tokens[s].append(100 * s + len(self.tokens[s]))

    def pool_chunk_ctc_prefix(self, slots, ptr, length, offsets, required, beam_size=10, use_context=False, stream=None):
        self.calls.append(("ctc_prefix", list(slots), int(length), list(offsets), list(required), int(beam_size), None))
        for s in slots:
            self.ctc[s].append(10 * s + len(self.ctc[s]))

    def pool_chunk_prefix(self, slots, ptr, length, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, stream=None):
        assert ptr != 0 and beam_size > 0
        self.calls.append(("prefix", list(slots), int(length), list(offsets), list(required), int(beam_size), (ctc_weight, transducer_weight)))
        for s in slots:
            self.pre[s].append(10 * s + len(self.pre[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_tokens(self, slot, start=0, stream=None):
        return self.tokens[slot][start:]

    def stream_prefix(self, slot, states=False, stream=None):
        self.reads.append(slot)
        t = [5] + list(self.pre[slot])
        return [(t, -1.5), (t + [7], -2.5)]

    def stream_ctc_prefix(self, slot, final=False, raw=False, cap_hyps=16, cap_tokens=None, stream=None):
        t = list(self.ctc[slot])
        return [(t, -0.25, list(range(len(t))), 0.0)]

    def pool_rescore(self, slots, n_hyp, hyp_lens, hyp_tokens, stream=None):
        self.rescored.append((list(slots), np.array(n_hyp).tolist(), np.array(hyp_lens).tolist(), np.array(hyp_tokens).tolist()))
        nll = np.zeros((len(slots), int(max(n_hyp))), np.float64)
        nll[:, 0], nll[:, 1:] = 9.0, 1.0                      # the second hypothesis is the likelier one
        return nll


def test_open_exclusivity_and_range_errors_take_no_slot():
    fake = FakeEngine()
    pool = StreamPool(None, 2, engine=fake, max_beam=4)
    bad = [dict(prefix_beam=4, beam_size=2), dict(prefix_beam=4, ctc_prefix_beam=4), dict(prefix_beam=4, context=ContextBias([[1]], 2.0)),
           dict(prefix_beam=17), dict(prefix_beam=-1), dict(prefix_beam=4, ctc_weight=-0.1), dict(prefix_beam=4, transducer_weight=-1.0),
           dict(prefix_beam=4, ctc_weight=0.0, transducer_weight=0.0), dict(prefix_beam=4, ctc_weight=float("nan"))]
    for kw in bad:
        with pytest.raises(rlib.RnntError):
            pool.open(**kw)
        assert fake.opened == [] and pool._free == [0, 1] and pool._slots == {}, kw
    assert pool.open(prefix_beam=16, ctc_weight=0.0, transducer_weight=1.0) == 0
    assert {s: r.decoder for s, r in pool._slots.items()} == {0: ("prefix", 16, False, (0.0, 1.0), False)}
    wide = StreamPool(None, 1, engine=FakeEngine(), vocab_size=600)
    with pytest.raises(rlib.RnntError):
        wide.open(prefix_beam=4)                               # vocabulary > 512
    small = StreamPool(None, 1, engine=FakeEngine(), vocab_size=8)
    with pytest.raises(rlib.RnntError):
        small.open(prefix_beam=9)                              # beam <= vocabulary
    assert small.open(prefix_beam=8) == 0


def test_stream_pool_routes_prefix_slots():
    fake = FakeEngine()
    pool = StreamPool(None, 5, engine=fake)
    g0 = pool.open()
    p1 = pool.open(prefix_beam=5)
    p2 = pool.open(prefix_beam=5, ctc_weight=0.0, transducer_weight=1.0)
    p3 = pool.open(prefix_beam=5, keep_frames=True)
    c4 = pool.open(ctc_prefix_beam=10)
    assert (g0, p1, p2, p3, c4) == (0, 1, 2, 3, 4) and fake.kept == [3]
    assert pool.prefix_hyps(p1) == [([5], -1.5), ([5, 7], -2.5)]
    for s in range(5):
        assert pool.feed(s, torch.zeros(16, 80))
    assert not pool.feed(p1, torch.zeros(6, 80))               # the < 7-frame rule of process_single_chunk
    assert pool.feed(p3, torch.zeros(24, 80))
    assert pool.step() == {0: [0]}, "step() returns tokens of the greedy slots only"
    assert fake.calls == [("greedy", [0], 16, [0], [0], 0, None), ("ctc_prefix", [4], 16, [0], [0], 10, None),
                          ("prefix", [2], 16, [0], [0], 5, (0.0, 1.0)), ("prefix", [1, 3], 16, [0, 0], [0, 0], 5, (0.3, 0.7)),
                          ("prefix", [3], 24, [4], [4], 5, (0.3, 0.7))]
    fake.reads.clear()
    assert pool.prefix_hyps(p3) == [([5, 30, 31], -1.5), ([5, 30, 31, 7], -2.5)] and fake.reads == [3]
    for wrong in (g0, c4):
        with pytest.raises(rlib.RnntError):
            pool.prefix_hyps(wrong)
    with pytest.raises(rlib.RnntError):
        pool.ctc_hyps(p1)
    with pytest.raises(rlib.RnntError):
        pool.token_times(p3)                                   # not a greedy slot
    # close() processes a queued chunk first and returns the engine's rows
    n_calls = len(fake.calls)
    pool.feed(p1, torch.zeros(16, 80))
    assert pool.close(p1) == [([5, 10, 11], -1.5), ([5, 10, 11, 7], -2.5)]
    assert fake.calls[n_calls:] == [("prefix", [1], 16, [4], [4], 5, (0.3, 0.7))]
    assert 1 not in pool._slots and pool.open() == 1 and pool.step() == {}      # the freed slot is reused, as any kind


def test_rescore_takes_prefix_slots():
    fake = FakeEngine()
    pool = StreamPool(None, 3, engine=fake)
    p0 = pool.open(prefix_beam=5, keep_frames=True)
    c1 = pool.open(ctc_prefix_beam=4, keep_frames=True)
    p2 = pool.open(prefix_beam=5)                              # keeps no frames
    for s in (p0, c1):
        pool.feed(s, torch.zeros(16, 80))
    pool.step()
    with pytest.raises(rlib.RnntError):
        pool.rescore([p2], 0.3, 0.7)
    out = pool.rescore([p0, c1], 0.5, 0.5)
    # one library call for both slots; the prefix slot's lists without the leading blank, in the search's order
    assert fake.rescored == [([0, 1], [2, 1], [[1, 2], [1, 0]], [[[0, 0], [0, 7]], [[10, 0], [0, 0]]])]
    best, rows = out[p0]
    assert [r[0] for r in rows] == [[0], [0, 7]] and [r[1] for r in rows] == [-1.5, -2.5], "first scores are the search's scores"
    assert [r[2] for r in rows] == [-9.0, -1.0] and best == 1
    assert rows[1][3] == pytest.approx(-2.5 * 0.5 + -1.0 * 0.5)
    assert out[c1] == (0, [([10], -0.25, -9.0, pytest.approx(-0.25 * 0.5 - 9.0 * 0.5))])       # CTC slots as before
