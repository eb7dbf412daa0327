"""CPU-side checks of endpoint detection: the new entry points exist at every layer of the boundary, the host twin of the rule
(rnnt_endpoint_scan_host -- the very function the kernel runs) equals the Python restatement in endpoint_cases.py, StreamPool drives an
engine as documented (a recording fake), and the pool case of test_endpoint.py has the properties its GPU test relies on -- asserted
here on the float64 oracle, so the GPU test cannot hide a miss."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.lib import RnntError
from ctc_vr_amd.online_rnnt_model import Endpoint, EndpointConfig, OnlineRNNTModel, StreamPool

import endpoint_cases as C

NEW = {"rnnt_stream_endpoint": 4, "rnnt_pool_endpoint_frames": 6, "rnnt_pool_get_endpoints": 5, "rnnt_ctc_blank_logprob": 5,
       "rnnt_endpoint_scan_host": 4}
NAN = float("nan")


def test_abi_symbols_struct_and_version():
    lib = rlib.load()
    for s, n in NEW.items():
        assert hasattr(lib, s), f"librnnt_hip.so does not export {s}"
        assert s in rlib.SIGNATURES and len(rlib.SIGNATURES[s][1]) == n, s
    assert lib.rnnt_abi_version() == 3                                   # additive change
    assert ctypes.sizeof(rlib.RnntEndpointConfig) == 20
    assert [f[0] for f in rlib.RnntEndpointConfig._fields_] == ["blank_threshold", "min_speech_frames", "rule1_trailing", "rule2_trailing", "rule3_frames"]
    for w in ("stream_endpoint", "pool_endpoint_frames", "pool_endpoints", "ctc_blank_logprob", "endpoint_scan_host"):
        assert callable(getattr(rlib.RnntEngine, w)), w
    assert lib.rnnt_stream_endpoint(None, 0, None, None) == rlib.ERR_ARG      # a null context is refused
    one = np.zeros(8, np.int32)
    assert lib.rnnt_pool_endpoint_frames(None, 1, one.ctypes.data, one.ctypes.data, 1, None) == rlib.ERR_ARG
    assert lib.rnnt_pool_get_endpoints(None, 1, one.ctypes.data, one.ctypes.data, None) == rlib.ERR_ARG
    assert lib.rnnt_ctc_blank_logprob(None, one.ctypes.data, 1, one.ctypes.data, None) == rlib.ERR_ARG


# ---- the host twin against the Python restatement ---------------------------------------------------------------------------------
THR = 0.5
LT = float(C.log_thr(THR))           # the float both sides compare against
B, S_ = LT + 1.0, LT - 1.0           # a blank frame, a speech frame

HAND = {
    # name: (cfg, lp, expected state [frames, trailing, speech, rule, at])
    "rule1_before_any_speech": ((THR, 1, 3, 2, 0), [B, B, B, B], [4, 4, 0, 1, 3]),
    "rule2_after_speech": ((THR, 1, 5, 2, 0), [B, S_, B, B, B], [5, 3, 1, 2, 4]),
    "rule3_alone": ((THR, 1, 0, 0, 3), [S_, B, S_, S_], [4, 0, 3, 3, 3]),
    "rules_1_and_3_at_one_frame": ((THR, 1, 2, 0, 2), [B, B], [2, 2, 0, 1, 2]),
    "rules_2_and_3_at_one_frame": ((THR, 1, 0, 2, 3), [S_, B, B], [3, 2, 1, 2, 3]),
    "sticky_counters_run_on": ((THR, 1, 2, 1, 4), [B, B, S_, B, B, B, S_], [7, 0, 2, 1, 2]),
    "nan_is_speech": ((THR, 1, 2, 0, 0), [B, NAN, B, B], [4, 2, 1, 0, 0]),
    "equal_to_threshold_is_speech": ((THR, 1, 2, 0, 0), [B, LT, B, B], [4, 2, 1, 0, 0]),
    "just_above_threshold_is_blank": ((THR, 1, 2, 0, 0), [float(np.nextafter(np.float32(LT), np.float32(1)))] * 2, [2, 2, 0, 1, 2]),
    "min_speech_zero_skips_rule1": ((THR, 0, 1, 2, 0), [B, B], [2, 2, 0, 2, 2]),
    "min_speech_three": ((THR, 3, 0, 1, 0), [S_, B, S_, B, S_, B], [6, 1, 3, 2, 6]),
    "all_rules_off_only_counts": ((THR, 1, 0, 0, 0), [B, S_, B, B], [4, 2, 1, 0, 0]),
    "no_frames": ((THR, 1, 1, 1, 1), [], [0, 0, 0, 0, 0]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_scan_host_hand_cases(name):
    cfg, lp, want = HAND[name]
    assert C.scan_ref(lp, cfg) == want                       # the restatement says what the case's name says
    assert rlib.endpoint_scan_host(lp, cfg).tolist() == want


def _seeded():
    g = np.random.Generator(np.random.Philox(key=[23, 0xE9D]))
    for i in range(300):
        n = int(g.integers(0, 201))
        thr = float(g.uniform(0.05, 0.95))
        lt = float(C.log_thr(thr))
        # values around the threshold, a long blank run somewhere, a few exact ties and NaNs
        lp = (lt + g.standard_normal(n) * (0.2 + 2.0 * g.uniform())).astype(np.float32)
        if n > 20 and i % 3 == 0:
            a = int(g.integers(0, n - 10))
            lp[a:a + int(g.integers(5, 60))] = lt + 0.5
        for k in g.integers(0, max(n, 1), size=3):
            if n and i % 5 == 0:
                lp[k] = np.float32(lt) if k % 2 else np.float32(NAN)
        cfg = (thr, int(g.choice([0, 1, 3])), int(g.choice([0, 1, 4, 12])), int(g.choice([0, 1, 3, 9])), int(g.choice([0, 1, 50, 150])))
        yield lp, cfg, g


def test_scan_host_equals_the_restatement_whatever_the_split():
    fired = set()
    for lp, cfg, g in _seeded():
        want = C.scan_ref(lp, cfg)
        assert rlib.endpoint_scan_host(lp, cfg).tolist() == want, cfg
        cuts = sorted(int(c) for c in g.integers(0, lp.size + 1, size=int(g.integers(1, 6))))
        st = None
        for a, b in zip([0] + cuts, cuts + [lp.size]):        # empty pieces included
            st = rlib.endpoint_scan_host(lp[a:b], cfg, st)
        assert st.tolist() == want, (cfg, cuts)
        fired.add(want[3])
    assert fired == {0, 1, 2, 3}                              # the seeded cases reach every outcome


def test_scan_host_refusals():
    lib = rlib.load()
    good = rlib.RnntEndpointConfig(0.5, 1, 1, 1, 1)
    lp, st = np.zeros(4, np.float32), np.zeros(5, np.int32)
    args = lambda c: (lp.ctypes.data, 4, ctypes.byref(c), st.ctypes.data)   # noqa: E731
    assert lib.rnnt_endpoint_scan_host(*args(good)) == 0
    before = st.copy()
    for bad in ((0.0, 1, 1, 1, 1), (1.0, 1, 1, 1, 1), (-0.5, 1, 1, 1, 1), (1.5, 1, 1, 1, 1), (NAN, 1, 1, 1, 1), (0.5, -1, 1, 1, 1), (0.5, 1, -1, 1, 1),
                (0.5, 1, 1, -1, 1), (0.5, 1, 1, 1, -1)):
        assert lib.rnnt_endpoint_scan_host(*args(rlib.RnntEndpointConfig(*bad))) == rlib.ERR_ARG, bad
        with pytest.raises(RnntError) as e:
            rlib.endpoint_scan_host(lp, bad)
        assert e.value.status == rlib.ERR_ARG
    assert lib.rnnt_endpoint_scan_host(lp.ctypes.data, 4, None, st.ctypes.data) == rlib.ERR_ARG
    assert lib.rnnt_endpoint_scan_host(lp.ctypes.data, 4, ctypes.byref(good), None) == rlib.ERR_ARG
    assert lib.rnnt_endpoint_scan_host(None, 4, ctypes.byref(good), st.ctypes.data) == rlib.ERR_ARG
    assert lib.rnnt_endpoint_scan_host(lp.ctypes.data, -1, ctypes.byref(good), st.ctypes.data) == rlib.ERR_ARG
    assert (st == before).all()                               # a refusal changes nothing
    assert lib.rnnt_endpoint_scan_host(None, 0, ctypes.byref(good), st.ctypes.data) == 0      # t = 0 needs no values
    assert (st == before).all()


# ---- StreamPool with a recording fake engine ---------------------------------------------------------------------------------------
class FakeEngine:
    def __init__(self, refuse_endpoint=False):
        self.log, self.refuse = [], refuse_endpoint

    def reset(self, n, stream=None):
        self.log.append(("reset", n))

    def stream_open(self, slot, stream=None):
        self.log.append(("open", slot))

    def stream_keep_frames(self, slot, keep=True, stream=None):
        self.log.append(("keep", slot))

    def stream_endpoint(self, slot, cfg, stream=None):
        if self.refuse:
            raise RnntError("rnnt_stream_endpoint: refused", rlib.ERR_ARG)
        self.log.append(("endpoint", slot, tuple(cfg)))

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy=True, stream=None):
        self.log.append(("chunk", list(slots), length))
        return 3

    def stream_tokens(self, slot, start=0, stream=None):
        return []

    def pool_endpoints(self, slots, stream=None):
        self.log.append(("endpoints", list(slots)))
        return np.asarray([[10 + s, 2, 3, 1 + s % 3, 7] for s in slots], np.int32)


class OldFakeEngine:
    """an engine from before the feature: no stream_endpoint, no pool_endpoints"""

    def __init__(self):
        self.log = []

    def reset(self, n, stream=None):
        pass

    def stream_open(self, slot, stream=None):
        self.log.append(("open", slot))

    def stream_tokens(self, slot, start=0, stream=None):
        return []


def test_endpoint_config_ms_to_frames():
    assert OnlineRNNTModel.FRAME_SECONDS == 0.04
    assert EndpointConfig().as_tuple() == (0.8, 1, 125, 25, 500)                 # WeNet's usual 5 s / 1 s / 20 s
    assert EndpointConfig(0.5, 79, 40, 39, 3).as_tuple() == (0.5, 3, 1, 1, 0)    # floor division; below one frame a rule is off
    assert EndpointConfig(rule1_ms=0, rule2_ms=0, rule3_ms=0).as_tuple()[2:] == (0, 0, 0)


def test_pool_call_order_and_one_read():
    fake = FakeEngine()
    pool = StreamPool(None, 4, engine=fake)
    cfg = EndpointConfig(0.6, 400, 200, 2000, 2)
    a = pool.open(keep_frames=True, endpoint=cfg)
    b = pool.open()
    c = pool.open(endpoint=EndpointConfig())
    assert (a, b, c) == (0, 1, 2)
    assert fake.log == [("reset", 4), ("open", 0), ("keep", 0), ("endpoint", 0, (0.6, 2, 10, 5, 50)), ("open", 1), ("open", 2),
                        ("endpoint", 2, (0.8, 1, 125, 25, 500))]
    del fake.log[:]
    assert pool.feed(a, torch.zeros(16, 80)) and pool.feed(b, torch.zeros(16, 80))
    pool.step()                                              # step() itself asks nothing new of the engine
    assert [e[0] for e in fake.log] == ["chunk"]
    del fake.log[:]
    got = pool.endpoints()
    assert fake.log == [("endpoints", [0, 2])]               # ONE engine call, the endpoint slots only
    assert got == {0: Endpoint(rule=1, at_frame=7, frames=10, trailing=2, speech=3), 2: Endpoint(3, 7, 12, 2, 3)}
    del fake.log[:]
    assert pool.endpoints([2]) == {2: Endpoint(3, 7, 12, 2, 3)} and fake.log == [("endpoints", [2])]
    with pytest.raises(RnntError):
        pool.endpoints([1])                                  # not an endpoint slot
    pool.close(a)
    del fake.log[:]
    assert set(pool.endpoints()) == {2}                      # close() forgot slot 0's flag
    with pytest.raises(RnntError):
        pool.endpoints([a])
    pool.close(c)
    del fake.log[:]
    assert pool.endpoints() == {} and fake.log == []         # nothing to read: no engine call
    again = pool.open()                                      # the slot's next caller did not ask
    assert again == 0 and [e[0] for e in fake.log] == ["open"] and pool.endpoints() == {}
    pool.reset()
    assert pool.endpoints() == {}


def test_refused_endpoint_takes_no_slot():
    fake = FakeEngine(refuse_endpoint=True)
    pool = StreamPool(None, 2, engine=fake)
    with pytest.raises(RnntError):
        pool.open(endpoint=EndpointConfig(blank_threshold=1.5))
    assert pool.endpoints() == {}
    fake.refuse = False
    assert pool.open(endpoint=EndpointConfig()) == 0         # the lowest slot is still free
    assert set(pool.endpoints()) == {0}


def test_open_without_endpoint_never_asks():
    old = OldFakeEngine()
    pool = StreamPool(None, 2, engine=old)
    assert pool.open() == 0 and pool.open() == 1
    assert pool.endpoints() == {}
    assert old.log == [("open", 0), ("open", 1)]


# ---- conditions of the pool case, on the float64 oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.BIAS_C)
def test_pool_case_conditions(c):
    thr, half, lp = C.threshold(c)
    per_utt = [sum(p.size for p in per) for per in C.oracle_lp(c)]
    assert per_utt == [30, 35, 45] and lp.size == 110        # every encoder frame of the three utterances is in the comparison
    lt = float(C.log_thr(thr))
    dist = np.abs(lp - lt)
    blank = float((lp > lt).mean())
    print(f"c = {c}: threshold {thr:.4f}, half-gap {half:.3e}, nearest frame {dist.min():.3e} from log_thr, {100 * blank:.0f} % blank frames")
    assert 0.0 < thr < 1.0
    assert half >= C.MIN_HALF_GAP and dist.min() >= C.MIN_HALF_GAP - 1e-6     # no frame within 10 x LOGIT_TOL of the float the device compares against
    assert 0.1 <= blank <= 0.9                               # both classes >= 10 % of the frames
    ends = [tuple(C.oracle_states(c, u)[-1][3:]) for u in range(3)]
    assert ends == list(C.EXPECT[c])
    for u in range(3):                                       # and the states count every frame
        assert [st[0] for st in C.oracle_states(c, u)] == list(np.cumsum([p.size for p in C.oracle_lp(c)[u]]))


def test_pool_case_reaches_every_outcome():
    rules = {C.oracle_states(c, u)[-1][3] for c in C.BIAS_C for u in range(3)}
    assert rules == {0, 1, 2, 3}
    # a rule fires in the middle of a call somewhere: per-frame evaluation shows
    mid = [st for c in C.BIAS_C for u in range(3) for st in C.oracle_states(c, u) if st[3] and st[4] != st[0]]
    assert mid
    assert math.isclose(C.threshold(6.0)[0], 0.4206, abs_tol=5e-4) and math.isclose(C.threshold(6.5)[0], 0.5448, abs_tol=5e-4)
