"""Segments of the stream pool, the parts that need no GPU: the two entry points are declared, bound and exported; StreamPool on a
recording fake engine makes ONE endpoint read and ONE rnnt_pool_segment call per flavour per step(), keeps or restarts the offsets,
hands the Segments out in order, and with on_endpoint=None asks of the engine exactly what it asked before the feature."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.lib import RnntError
from ctc_vr_amd.online_rnnt_model import Endpoint, EndpointConfig, Segment, StreamPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnnt_hip.h")).read(), flags=re.S)
    lib = rlib.load()
    for name, n_args in (("rnnt_pool_segment", 5), ("rnnt_stream_get_segment", 4)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rnnt_hip.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in rlib.SIGNATURES, f"{name} is missing from lib.SIGNATURES"
        res, args = rlib.SIGNATURES[name]
        assert res is rlib.c_i32 and len(args) == n_args
        assert hasattr(lib, name), f"librnnt_hip.so does not export {name}"
    assert lib.rnnt_abi_version() == 3                          # additive change
    assert ctypes.sizeof(rlib.RnntConfig) == 40
    assert lib.rnnt_pool_segment(None, 1, None, 1, None) == rlib.ERR_ARG and lib.rnnt_stream_get_segment(None, 0, None, None) == rlib.ERR_ARG


# ---- StreamPool with a recording fake engine ---------------------------------------------------------------------------------------
class FakeEngine:
    """records every call; pool_endpoints reports a fired rule (3, at frame 6) for the slots in `fire`, once they have advanced"""

    def __init__(self, fire=()):
        self.log, self.fire = [], set(fire)
        self.frames, self.seg = {}, {}                          # slot -> encoder frames since open, (index, start_frame)
        self.since = {}                                         # slot -> frames since the segment began

    def reset(self, n, stream=None):
        self.log.append(("reset", n))

    def stream_open(self, slot, stream=None):
        self.log.append(("open", slot))
        self.frames[slot], self.seg[slot], self.since[slot] = 0, (0, 0), 0

    def stream_endpoint(self, slot, cfg, stream=None):
        self.log.append(("endpoint", slot, tuple(cfg)))

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        self.log.append(("chunk", list(slots), length, list(offsets)))
        for s in slots:
            self.frames[s] += 3
            self.since[s] += 3
        return 3

    def stream_tokens(self, slot, start=0, stream=None):
        self.log.append(("tokens", slot, start))
        return [7] * max(self.since[slot] // 3 - start, 0)      # one token per chunk of the segment

    def pool_endpoints(self, slots, stream=None):
        self.log.append(("endpoints", list(slots)))
        return np.asarray([[self.since[s], 0, self.since[s], 3 if s in self.fire and self.since[s] >= 6 else 0,
                            6 if s in self.fire and self.since[s] >= 6 else 0] for s in slots], np.int32)

    def pool_segment(self, slots, keep_encoder=True, stream=None):
        self.log.append(("segment", list(slots), bool(keep_encoder)))
        for s in slots:
            self.seg[s] = (self.seg[s][0] + 1, self.frames[s])
            self.since[s] = 0

    def stream_segment(self, slot):
        return self.seg[slot]


class OldFakeEngine:
    """an engine from before the feature: no pool_segment, no stream_segment"""

    def __init__(self):
        self.log = []

    def reset(self, n, stream=None):
        self.log.append(("reset", n))

    def stream_open(self, slot, stream=None):
        self.log.append(("open", slot))

    def stream_endpoint(self, slot, cfg, stream=None):
        self.log.append(("endpoint", slot, tuple(cfg)))

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        self.log.append(("chunk", list(slots), length, list(offsets)))
        return 3

    def stream_tokens(self, slot, start=0, stream=None):
        self.log.append(("tokens", slot, start))
        return []


CFG = EndpointConfig(0.5, 0, 0, 6 * 40, 1)                      # rule 3 at 6 frames
CHUNK = torch.zeros(16, 80)


def _run(pool, slots, steps):
    for _ in range(steps):
        for s in slots:
            assert pool.feed(s, CHUNK)
        pool.step()


@pytest.mark.parametrize("flavour", ["keep", "fresh"])
def test_step_segments_fired_slots_with_one_read_and_one_call(flavour):
    fake = FakeEngine(fire=(0, 2))
    pool = StreamPool(None, 3, engine=fake)
    slots = [pool.open(endpoint=CFG, on_endpoint=flavour) for _ in range(3)]
    assert slots == [0, 1, 2]
    del fake.log[:]
    _run(pool, slots, 1)                                        # 3 frames: nothing fires
    assert [e[0] for e in fake.log] == ["chunk", "tokens", "tokens", "tokens", "endpoints"] and fake.log[-1] == ("endpoints", [0, 1, 2])
    del fake.log[:]
    _run(pool, slots, 1)                                        # 6 frames: slots 0 and 2 fire
    assert [e for e in fake.log if e[0] in ("endpoints", "segment")] == [("endpoints", [0, 1, 2]), ("segment", [0, 2], flavour == "keep")]
    assert fake.log[0] == ("chunk", [0, 1, 2], 16, [4, 4, 4])
    # the step's increments were read before the boundary, the segments' results (all tokens) between the read and the segment call
    assert [e[0] for e in fake.log] == ["chunk", "tokens", "tokens", "tokens", "endpoints", "tokens", "tokens", "segment"]
    assert fake.log[5:7] == [("tokens", 0, 0), ("tokens", 2, 0)]
    del fake.log[:]
    _run(pool, slots, 1)
    # the offsets of the next chunk call: they run on with the encoder kept and restart at 0 with a fresh one; slot 1 never segmented
    assert fake.log[0] == ("chunk", [0, 1, 2], 16, [8, 8, 8] if flavour == "keep" else [0, 8, 0])
    assert ("tokens", 0, 0) in fake.log and ("tokens", 1, 2) in fake.log      # the token cursor of a segmented slot restarted
    assert sum(e[0] == "endpoints" for e in fake.log) == 1 and not any(e[0] == "segment" for e in fake.log)
    _run(pool, slots, 1)                                        # 6 frames into the second segment: they fire again
    for s in (0, 2):
        got = pool.segments(s)
        assert [g.index for g in got] == [0, 1] and [g.start_frame for g in got] == [0, 6] and [g.frames for g in got] == [6, 6]
        assert all(isinstance(g, Segment) and g.result == [7, 7] for g in got)
        assert got[0].endpoint == Endpoint(rule=3, at_frame=6, frames=6, trailing=0, speech=6)
        assert pool.segments(s) == []                           # drained
    assert pool.segments(1) == []


def test_mixed_flavours_one_call_each():
    fake = FakeEngine(fire=(0, 1, 2))
    pool = StreamPool(None, 3, engine=fake)
    pool.open(endpoint=CFG, on_endpoint="keep"), pool.open(endpoint=CFG, on_endpoint="fresh"), pool.open(endpoint=CFG, on_endpoint="keep")
    _run(pool, [0, 1, 2], 2)
    assert [e for e in fake.log if e[0] in ("endpoints", "segment")] == [("endpoints", [0, 1, 2]), ("endpoints", [0, 1, 2]),
                                                                           ("segment", [0, 2], True), ("segment", [1], False)]


def test_on_endpoint_needs_endpoint_and_a_known_flavour():
    pool = StreamPool(None, 2, engine=FakeEngine())
    with pytest.raises(RnntError):
        pool.open(on_endpoint="keep")
    with pytest.raises(RnntError):
        pool.open(endpoint=CFG, on_endpoint="both")
    assert pool.open(endpoint=CFG, on_endpoint="fresh") == 0    # the refused opens took no slot


def test_without_on_endpoint_the_engine_is_asked_what_it_was_asked_before():
    """the call list of this script on an engine that has neither pool_segment nor stream_segment, written out as it was recorded
    before segments existed"""
    old = OldFakeEngine()
    pool = StreamPool(None, 2, engine=old)
    a, b = pool.open(endpoint=CFG), pool.open()
    _run(pool, [a, b], 2)
    pool.feed(a, CHUNK)
    assert pool.close(a) == [] and pool.close(b) == []
    assert pool.segments(a) == []
    assert old.log == [("reset", 2), ("open", 0), ("endpoint", 0, (0.5, 1, 0, 0, 6)), ("open", 1),
                       ("chunk", [0, 1], 16, [0, 0]), ("tokens", 0, 0), ("tokens", 1, 0),
                       ("chunk", [0, 1], 16, [4, 4]), ("tokens", 0, 0), ("tokens", 1, 0),
                       ("chunk", [0], 16, [8]), ("tokens", 0, 0), ("tokens", 0, 0), ("tokens", 1, 0)]


def test_next_segment():
    fake = FakeEngine()
    pool = StreamPool(None, 2, engine=fake)
    with pytest.raises(RnntError):
        pool.next_segment(0)                                    # not open
    a, b = pool.open(endpoint=CFG), pool.open()
    _run(pool, [a, b], 1)
    pool.feed(a, CHUNK)                                         # still queued: stepped first, as in close()
    del fake.log[:]
    seg = pool.next_segment(a)
    assert [e[0] for e in fake.log] == ["chunk", "tokens", "endpoints", "tokens", "segment"] and fake.log[-1] == ("segment", [0], True)
    assert seg == Segment(0, 0, 6, [7, 7], Endpoint(0, 0, 6, 0, 6))
    seg = pool.next_segment(b, keep_encoder=False)
    assert seg == Segment(0, 0, 3, [7], None) and fake.log[-1] == ("segment", [1], False)
    del fake.log[:]
    _run(pool, [a, b], 1)
    assert fake.log[0] == ("chunk", [0, 1], 16, [8, 0])
    assert pool.next_segment(a).index == 1 and pool.next_segment(a) == Segment(2, 9, 0, [], Endpoint(0, 0, 0, 0, 0))
    pool.close(a)
    with pytest.raises(RnntError):
        pool.next_segment(a)
