"""Plans, bookkeeping and float64 references shared by test_encoder_window_cpu.py and test_encoder_window.py: the streaming encoder
under every window policy of forward_chunk's (offset, required_cache_size) pair (wenet/transformer/encoder.py:254-264), at chunk
lengths on both sides of the attention / row-tile dispatch boundaries.  No GPU is touched here."""
import numpy as np

import ctc_vr_amd.testing as T

LOGIT_TOL = 1e-3        # the project's encoder bar against the reference (BASELINE.json north star)
SCHED_TOL = 1e-4        # whole-utterance call vs per-chunk API (test_wavefront_encoder_matches_chunk_by_chunk)
SEED_W = 0
LORDER, WF_MERGE_MAX = 30, 4

# chunk lengths in fbank frames -> t' (the issue's eight, plus 15 -> t' = 3 so that every policy meets t' = 3, 4 and 5):
# t' <= 4 takes the direct-stream attention, t' <= 8 NQ = 2, above that NQ = 4; 17 > 16 cannot take the fused half-blocks
LENGTHS = (7, 11, 15, 19, 23, 35, 39, 67, 71)
POLICIES = ("all", "zero", "one", "two", "r64", "off")
TRUNCATING = ("one", "two", "r64")


def sub_len(t):
    return ((t - 3) // 2 + 1 - 3) // 2 + 1


def max_chunk_frames(length):
    return length + 1                                   # just above the chunk; the same t'


def ring_cap(length):
    return LORDER + WF_MERGE_MAX * sub_len(max_chunk_frames(length))


def required_of(policy, tq, offset):
    return {"all": -1, "zero": 0, "one": tq, "two": 2 * tq + 1, "r64": 64, "off": offset}[policy]


class SlotPos:
    """The library's position bookkeeping (rnnt_api.hip: SlotPos::plan / advance), restated."""

    def __init__(self):
        self.cache_len = self.kv_start = self.conv_pos = 0

    def plan(self, tq, offset, tcap):
        t2, pos_start = self.cache_len + tq, offset - self.cache_len
        ok = pos_start >= 0 and pos_start + t2 <= T.MAX_LEN and self.kv_start + t2 <= tcap
        return {"tq": tq, "T2": t2, "pos_start": pos_start, "kv_row0": self.kv_start, "ring_pos": self.conv_pos, "ok": ok}

    def advance(self, t2, tq, required):
        nxt = 0 if required < 0 else (t2 if required == 0 else max(t2 - required, 0))
        self.kv_start += nxt
        self.cache_len = t2 - nxt
        if self.cache_len == 0:
            self.kv_start = 0
        self.conv_pos += tq


def walk(plan, tcap=1 << 30):
    """SlotPos over a plan -> the per-chunk windows (plan() dicts, plus "cache_after")."""
    pos, out = SlotPos(), []
    for _, length, offset, required in plan:
        k = pos.plan(sub_len(length), offset, tcap)
        pos.advance(k["T2"], k["tq"], required)
        k["cache_after"] = pos.cache_len
        out.append(k)
    return out


def n_chunks_for(length, policy):
    """Enough chunks that the last chunk's ring position has passed the ring capacity twice and, where the policy truncates,
    its key window starts beyond row 64 with a saturated window."""
    tq, n = sub_len(length), 2
    while True:
        last = walk(make_plan(length, policy, n))[-1]
        if last["ring_pos"] >= 2 * ring_cap(length) and (policy not in TRUNCATING or last["kv_row0"] > 64):
            return n
        n += 1
        assert n * tq <= 256, (length, policy)


def make_plan(length, policy, n=None, tail=None):
    """[(start, length, offset, required)]: n chunks of `length` frames (then one of `tail` frames), offsets advancing by the true t'."""
    n = n_chunks_for(length, policy) if n is None else n
    tq, plan, start, offset = sub_len(length), [], 0, 0
    for ln in [length] * n + ([tail] if tail else []):
        plan.append((start, ln, offset, required_of(policy, tq, offset)))
        start += ln
        offset += sub_len(ln)
    return plan


# every length meets R = t' and R = 2t' + 1; every policy meets t' = 3, 4 and 5
CASES = [(ln, p) for ln in LENGTHS for p in ("one", "two")] + [(ln, p) for ln in (15, 19, 23) for p in ("all", "zero", "r64", "off")]
RAGGED = (23, "two", 11)        # chunks of t' = 5 under R = 11, the last one of 11 frames (t' = 2)
N_STREAMS = 2


def case_plan(case):
    return make_plan(case[0], case[1], tail=case[2] if len(case) > 2 else None)


def case_id(case):
    return "-".join(str(v) for v in case)


def plan_frames(plan):
    return plan[-1][0] + plan[-1][1], sum(sub_len(p[1]) for p in plan)


_CACHE = {}


def state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = T.make_state_dict(SEED_W)
    return _CACHE["sd"]


def case_input(case, n_streams=N_STREAMS):
    """[n_streams, total frames, 80] float32, a different utterance per stream and per chunk length"""
    key = ("x", case, n_streams)
    if key not in _CACHE:
        _CACHE[key] = T.synth_fbank(n_streams, plan_frames(case_plan(case))[0], seed=4000 + case[0])
    return _CACHE[key]


def case_ref(case, stream, dtype=None, x=None):
    """encoder_stream_ref of one stream of a case (float64 unless dtype says otherwise), computed once per session"""
    key = ("ref", case, stream, dtype)
    if key not in _CACHE or x is not None:
        xs = case_input(case, max(N_STREAMS, stream + 1))[stream] if x is None else x
        ref = T.encoder_stream_ref(state_dict(), xs, case_plan(case), dtype)
        if x is not None:
            return ref
        _CACHE[key] = ref
    return _CACHE[key]


def maxdiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) if a.size else 0.0


def ref_distance(got, ref):
    """max |difference| of per-chunk results {"frames", "att", "cnn"} against a reference's -> (frames, att, cnn)"""
    return tuple(max(maxdiff(g[k], r[k]) for g, r in zip(got, ref)) for k in ("frames", "att", "cnn"))
