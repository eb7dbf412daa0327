"""Stream pool without a GPU: the three new C-ABI symbols exist and agree with the header and the ctypes table, a null context is
refused, and StreamPool's planner -- driven through a recording fake engine with a staggered arrival script -- hands every utterance
exactly the chunk boundaries of testing.chunk_plan and the offsets StreamingBatch.process_chunk would pass, one chunk length per
library call and no slot twice in a call."""
import ctypes
import os
import re

import numpy as np
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.online_rnnt_model import StreamPool, pool_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_stream_open", "rnnt_pool_chunk", "rnnt_stream_get_tokens")
CHUNK = 16


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
    assert ctypes.sizeof(rlib.RnntConfig) == 10 * 4


def test_null_context_is_an_argument_error():
    lib = rlib.load()
    one = np.zeros(1, np.int32)
    p = one.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int32(0)
    assert lib.rnnt_stream_open(None, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_chunk(None, 1, p, p, 16, p, p, 1, ctypes.byref(n), None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_tokens(None, 0, 0, 1, p, ctypes.byref(n), None) == rlib.ERR_ARG


class FakeEngine:
    """Records what StreamPool asks of the library; emits one token per call and slot so that the token plumbing is exercised."""

    def __init__(self):
        self.calls = []          # (slots, length, offsets, required, greedy)
        self.opened = []
        self.tokens = {}

    def reset(self, n, stream=None):
        self.n = n

    def stream_open(self, slot, stream=None):
        assert 0 <= slot < self.n
        self.opened.append(slot)
        self.tokens[slot] = []

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        assert ptr != 0
        self.calls.append((list(slots), int(length), list(offsets), list(required), bool(greedy)))
        for s in slots:
            self.tokens[s].append(100 * s + len(self.tokens[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_tokens(self, slot, start=0, stream=None):
        return self.tokens[slot][start:]


def _expected(frames):
    """(length, offset) of every chunk the decode script / StreamingBatch.process_chunk encodes for an utterance of `frames` frames"""
    out, off = [], 0
    for a, b in T.chunk_plan(frames, CHUNK):
        if b - a < 7:
            continue
        out.append((b - a, off))
        off += (b - a) // 4
    return out


def test_planner_staggered_arrivals():
    # (arrival step, frames): lengths below two chunks, with a merged tail of every size class, one < 7-frame utterance, slots reused
    script = [(0, 200), (0, 37), (1, 112), (1, 5), (2, 20), (3, 331), (3, 48), (5, 64), (6, 31), (8, 100), (9, 16), (9, 203), (12, 90), (13, 7)]
    fake = FakeEngine()
    pool = StreamPool(None, 4, engine=fake)
    waiting = list(enumerate(script))
    live = {}                                  # slot -> [utt, remaining chunk plan, got tokens]
    seen = {u: [] for u in range(len(script))}  # utt -> [(length, offset)] as the library saw them
    tokens = {}
    step = 0
    while waiting or live:
        while waiting and waiting[0][1][0] <= step and len(live) < 4:
            u, (_, frames) = waiting.pop(0)
            slot = pool.open()
            assert slot == min(set(range(4)) - set(live)), "open() must hand out the lowest free slot"
            live[slot] = [u, list(T.chunk_plan(frames, CHUNK)), []]
        n_calls = len(fake.calls)
        fed = {}
        for slot, st in live.items():
            a, b = st[1].pop(0)
            ok = pool.feed(slot, torch.zeros(b - a, 80))
            assert ok == (b - a >= 7)
            if ok:
                fed[slot] = b - a
            if step % 3 == 2 and st[1]:          # a caller that delivers two chunks before the next step
                a, b = st[1].pop(0)
                assert pool.feed(slot, torch.zeros(b - a, 80)) == (b - a >= 7)
        new = pool.step()
        assert set(new) == set(fed)
        for slots, length, offsets, required, greedy in fake.calls[n_calls:]:
            assert greedy and offsets == required
            assert len(set(slots)) == len(slots), "a slot twice in one call"
            for s, o in zip(slots, offsets):
                seen[live[s][0]].append((length, o))
        for slot, t in new.items():
            live[slot][2].extend(t)
        for slot in [s for s, st in live.items() if not st[1]]:
            u = live[slot][0]
            tokens[u] = pool.close(slot)
            assert tokens[u] == live[slot][2], "step() increments must add up to close()'s tokens"
            del live[slot]
        step += 1
    for u, (_, frames) in enumerate(script):
        assert seen[u] == _expected(frames), (u, frames)
    assert len({length for _, length, _, _, _ in fake.calls}) >= 5     # the script really mixes length classes
    assert sorted(set(fake.opened)) == [0, 1, 2, 3] and len(fake.opened) == len(script)


def test_pool_plan_pure():
    calls, offs, index = pool_plan([(2, 16), (0, 16), (2, 24), (1, 5), (0, 31), (3, 24)], {0: 8, 1: 0, 2: 0, 3: 40})
    # round 0: slot 2 (16), slot 0 (16), slot 3 (24); round 1: slot 2 (24), slot 0 (31); the 5-frame chunk is skipped
    assert calls == [(16, [2, 0], [0, 8]), (24, [3], [40]), (24, [2], [4]), (31, [0], [12])]
    assert offs == {0: 8 + 4 + 7, 1: 0, 2: 4 + 6, 3: 46}
    assert index == [(0, 0), (0, 1), (2, 0), None, (3, 0), (1, 0)]
    for length, slots, _ in calls:
        assert len(set(slots)) == len(slots)


def test_pool_full_and_closed_slot():
    import pytest
    pool = StreamPool(None, 2, engine=FakeEngine())
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1)
    with pytest.raises(rlib.RnntError):
        pool.open()
    pool.close(a)
    with pytest.raises(rlib.RnntError):
        pool.feed(a, torch.zeros(16, 80))
    assert pool.open() == 0
