"""Per-slot beam search of the stream pool without a GPU: the three new C-ABI symbols exist and agree with the header and the ctypes
table, pool_plan keeps greedy slots and every beam size in calls of their own without disturbing feed order or today's results,
and StreamPool -- over a recording fake engine -- issues rnnt_pool_chunk_beam for beam slots, rnnt_pool_chunk for greedy slots and
reads the hypotheses of the right slots."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.online_rnnt_model import BeamHypothesis, StreamPool, pool_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_pool_chunk_beam", "rnnt_stream_get_beam", "rnnt_stream_get_beam_states")


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
    assert lib.rnnt_pool_chunk_beam(None, 1, p, p, 16, p, p, 4, ctypes.byref(n), None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_beam(None, 0, 1, 1, ctypes.byref(n), p, p, p, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_beam_states(None, 0, 1, p, p, None) == rlib.ERR_ARG


# ---- pool_plan -------------------------------------------------------------------------------------------------------------------
def test_plan_separates_greedy_and_beam_sizes():
    # equal lengths everywhere: slot 0 greedy, slots 1 and 4 beam 4, slot 2 beam 2, slot 3 greedy
    beams = {0: 0, 1: 4, 2: 2, 3: 0, 4: 4}
    calls, offs, index = pool_plan([(s, 16) for s in range(5)], {s: 8 * s for s in range(5)}, beams)
    assert calls == [(16, [0, 3], [0, 24], 0), (16, [2], [16], 2), (16, [1, 4], [8, 32], 4)]
    assert index == [(0, 0), (2, 0), (1, 0), (0, 1), (2, 1)]
    assert offs == {s: 8 * s + 4 for s in range(5)}
    for _, slots, _, beam in calls:
        assert len({beams[s] for s in slots}) == 1 and beams[slots[0]] == beam, "greedy and beam slots, or two beam sizes, share a call"


def test_plan_keeps_feed_order_and_skips_short_chunks():
    beams = {0: 4, 1: 0, 2: 4}
    queue = [(0, 16), (1, 16), (0, 5), (2, 32), (0, 24), (1, 24), (2, 6), (0, 16)]
    calls, offs, index = pool_plan(queue, {0: 0, 1: 100, 2: 7}, beams)
    # round 0: slot 1 greedy (16), slot 0 beam (16), slot 2 beam (32); round 1: slot 1 greedy (24), slot 0 beam (24); round 2: slot 0 (16)
    assert calls == [(16, [1], [100], 0), (16, [0], [0], 4), (32, [2], [7], 4), (24, [1], [104], 0), (24, [0], [4], 4), (16, [0], [10], 4)]
    assert index == [(1, 0), (0, 0), None, (2, 0), (4, 0), (3, 0), None, (5, 0)]
    assert offs == {0: 14, 1: 110, 2: 15}                     # the 5- and 6-frame chunks moved no offset
    seen = {}
    for c, (length, slots, call_offs, _) in enumerate(calls):   # per slot: offsets grow in call order = feed order
        for s, o in zip(slots, call_offs):
            assert o >= seen.get(s, -1)
            seen[s] = o


@pytest.mark.parametrize("queue,offsets", [
    ([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40}),
    ([], {}),
    ([(0, 6), (0, 7), (0, 7)], {0: 3}),
    ([(1, 64), (0, 16), (1, 16), (0, 64), (2, 16)], {}),
    ([(s, 16 + 4 * (s % 3)) for s in range(8)] * 2, {s: s for s in range(8)}),
])
def test_plan_without_beams_is_todays(queue, offsets):
    """no beam argument, an empty one or all zeros: the calls, offsets and index of the greedy-only planner (3-tuples when the
    argument is absent), here re-derived from its documented rule"""
    offs, rounds, depth, index = dict(offsets), [], {}, [None] * len(queue)
    for k, (slot, length) in enumerate(queue):
        if length < 7:
            continue
        r = depth.get(slot, 0)
        depth[slot] = r + 1
        while len(rounds) <= r:
            rounds.append({})
        rounds[r].setdefault(length, []).append((slot, k))
    want = []
    for rnd in rounds:
        for length in sorted(rnd):
            slots, co = [], []
            for slot, k in rnd[length]:
                index[k] = (len(want), len(slots))
                slots.append(slot)
                co.append(offs.get(slot, 0))
                offs[slot] = offs.get(slot, 0) + length // 4
            want.append((length, slots, co))
    assert pool_plan(queue, offsets) == (want, offs, index)
    assert pool_plan(queue, offsets, None) == (want, offs, index)
    for b in ({}, {s: 0 for s, _ in queue}):
        calls, o2, i2 = pool_plan(queue, offsets, b)
        assert [c[:3] for c in calls] == want and all(c[3] == 0 for c in calls) and (o2, i2) == (offs, index)


def test_plan_pinned_result_without_beams():
    calls, offs, index = pool_plan([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40})
    assert calls == [(16, [2, 0], [0, 8]), (24, [3], [40]), (24, [2], [4]), (31, [0], [12])]
    assert offs == {0: 19, 1: 0, 2: 10, 3: 46}
    assert index == [(0, 0), (0, 1), (2, 0), None, (3, 0), (1, 0)]


# ---- StreamPool over a recording fake engine --------------------------------------------------------------------------------------
class FakeEngine:
    """Records what StreamPool asks of the library.  Greedy: one token per call and slot.  Beam: per slot one hypothesis that grows
    by one token per call, and a second one from the second call on."""

    def __init__(self):
        self.calls = []          # ("greedy" | "beam", slots, length, offsets, required, beam)
        self.beam_reads = []
        self.opened = []
        self.tokens, self.hyps = {}, {}

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        assert 0 <= slot < self.n
        self.opened.append(slot)
        self.tokens[slot] = []
        self.hyps[slot] = [([], 0.0)]

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        assert ptr != 0 and greedy
        self.calls.append(("greedy", list(slots), int(length), list(offsets), list(required), 0))
        for s in slots:
            self.tokens[s].append(100 * s + len(self.tokens[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def pool_chunk_beam(self, slots, ptr, length, offsets, required, beam_size=4, stream=None):
        assert ptr != 0 and beam_size > 0
        self.calls.append(("beam", list(slots), int(length), list(offsets), list(required), int(beam_size)))
        for s in slots:
            t, lp = self.hyps[s][0]
            self.hyps[s] = [(t + [1000 * s + len(t)], lp - 0.5), (t, lp - 1.0)][:beam_size]
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_tokens(self, slot, start=0, stream=None):
        return self.tokens[slot][start:]

    def stream_beam(self, slot, stream=None):
        self.beam_reads.append(slot)
        return list(self.hyps[slot])


def test_stream_pool_beam_and_greedy_slots():
    fake = FakeEngine()
    pool = StreamPool(None, 4, engine=fake, max_beam=4)
    g0 = pool.open()                       # slot 0 greedy
    b1 = pool.open(beam_size=4)            # slot 1 beam 4
    b2 = pool.open(beam_size=2)            # slot 2 beam 2
    b3 = pool.open(beam_size=4)            # slot 3 beam 4
    assert (g0, b1, b2, b3) == (0, 1, 2, 3)
    first = pool.beams(b1)
    assert len(first) == 1 and isinstance(first[0], BeamHypothesis) and first[0].tokens == [] and first[0].log_prob == 0.0
    for s in (g0, b1, b2, b3):
        assert pool.feed(s, torch.zeros(16, 80))
    assert not pool.feed(b1, torch.zeros(5, 80))               # skipped as in process_single_chunk_beam_search (:616-619)
    assert pool.feed(b3, torch.zeros(24, 80))                  # a second chunk of slot 3 before the step
    new = pool.step()
    assert new == {0: [0]}, "step() returns tokens of the greedy slots only"
    assert fake.calls == [("greedy", [0], 16, [0], [0], 0), ("beam", [2], 16, [0], [0], 2), ("beam", [1, 3], 16, [0, 0], [0, 0], 4),
                          ("beam", [3], 24, [4], [4], 4)]
    fake.beam_reads.clear()
    h1 = pool.beams(b1)
    assert fake.beam_reads == [1]
    assert [h.tokens for h in h1] == [[1000], []] and [h.log_prob for h in h1] == [-0.5, -1.0]
    assert [h.tokens for h in pool.beams(b3)] == [[3000, 3001], [3000]]
    assert [h.tokens for h in pool.beams(b2)] == [[2000], []]
    with pytest.raises(rlib.RnntError):
        pool.beams(g0)                                         # not a beam slot
    # a chunk shorter than 7 frames changes nothing: same hypotheses, no library call
    n_calls = len(fake.calls)
    assert not pool.feed(b1, torch.zeros(6, 80))
    assert pool.step() == {}
    assert len(fake.calls) == n_calls and [h.tokens for h in pool.beams(b1)] == [[1000], []]
    # close() with a queued chunk processes it first and returns the final hypotheses; the greedy neighbour's increment is carried
    pool.feed(b1, torch.zeros(16, 80))
    pool.feed(g0, torch.zeros(16, 80))
    fake.beam_reads.clear()
    final = pool.close(b1)
    assert fake.calls[n_calls:] == [("greedy", [0], 16, [4], [4], 0), ("beam", [1], 16, [4], [4], 4)]
    assert fake.beam_reads == [1] and [h.tokens for h in final] == [[1000, 1001], [1000]]
    assert pool.step() == {0: [1]}
    assert pool.close(g0) == [0, 1]
    # the freed slots are reused, in either mode
    assert pool.open(beam_size=3) == 0 and pool.open() == 1
    assert [h.tokens for h in pool.beams(0)] == [[]]


def test_open_beam_refused_at_once():
    fake = FakeEngine()
    pool = StreamPool(None, 2, engine=fake)                    # max_beam = 0: greedy only, as before
    with pytest.raises(rlib.RnntError):
        pool.open(beam_size=4)
    assert fake.opened == [] and pool.open() == 0, "a refused open() takes no slot"
    pool = StreamPool(None, 2, engine=FakeEngine(), max_beam=8)
    with pytest.raises(rlib.RnntError):
        pool.open(beam_size=9)                                 # above max_beam
    assert pool.open(beam_size=8) == 0
    pool = StreamPool(None, 2, engine=FakeEngine(), max_beam=32)
    with pytest.raises(rlib.RnntError):
        pool.open(beam_size=17)                                # above the device merge's 16
    pool = StreamPool(None, 2, engine=FakeEngine(), max_beam=4, vocab_size=600)
    with pytest.raises(rlib.RnntError):
        pool.open(beam_size=4)                                 # vocabulary > 512
    assert pool.open() == 0
