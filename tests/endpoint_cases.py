"""What test_endpoint_cpu.py and test_endpoint.py share: a Python restatement of the endpoint rule (include/rnnt_hip.h), and the pool
case -- three utterances whose float64-oracle CTC blank posteriors straddle a threshold with a gap the device cannot cross.

The pool case.  Weights make_state_dict(0) with ctc_head.ctc_lo.bias[blank] += c: the seeded head leaves the blank posterior near
1 / 412, so the bias is what makes frames straddle a threshold.  Utterances synth_fbank seeds 10, 11, 12 of 160, 160, 192 frames, fed
in 16-, 32- and 64-frame chunks with required = -1: 30 + 35 + 45 = 110 encoder frames.  The oracle is testing.encoder_stream_ref (float64)
followed by the head in float64.  The threshold is exp of the midpoint of the widest gap between consecutive sorted oracle blank
log-posteriors, taken between the 10 % and 90 % quantiles of all pooled frames (both values of a gap inside them); test_endpoint_cpu.py asserts on the oracle that the
half-gap is >= 1e-2 (10 x the project's LOGIT_TOL), so a device value within LOGIT_TOL has the oracle's class, and no frame is excluded
from any comparison.  Both c = 6.0 and c = 6.5 are used.  With this oracle the widest gap lies between the same two frames for both:
c = 6.0 gives threshold 0.4206, half-gap 2.3e-2; c = 6.5 gives threshold 0.5448, half-gap 1.8e-2; 27 % of the frames are blank, in
runs up to 9 long (the first nine frames of the first utterance).
"""
import math

import numpy as np

import ctc_vr_amd.testing as T

V, BLANK = T.VOCAB, T.BLANK
BIAS_C = (6.0, 6.5)
UTTS = ((10, 160, 16), (11, 160, 32), (12, 192, 64))      # (synth_fbank seed, fbank frames, chunk frames)
MIN_HALF_GAP = 1e-2
# per (c, utterance): (min_speech_frames, rule1_trailing, rule2_trailing, rule3_frames), small so that the oracle fires every rule
# somewhere and none somewhere (asserted in test_endpoint_cpu.py); the threshold is the case's own
RULES = {
    6.0: ((1, 5, 0, 0), (3, 0, 2, 0), (1, 50, 10, 0)),      # rule 1 at frame 5, rule 2 at frame 13, none
    6.5: ((1, 0, 0, 20), (1, 0, 2, 30), (0, 0, 0, 0)),      # rule 3 at frame 20, rule 2 at frame 5, none (all rules off: the slot only counts)
}
EXPECT = {6.0: ((1, 5), (2, 13), (0, 0)), 6.5: ((3, 20), (2, 5), (0, 0))}   # (rule, at) at the end of each utterance, on the oracle


def log_thr(threshold):
    """(float)log((double)blank_threshold), blank_threshold a C float"""
    return np.float32(math.log(float(np.float32(threshold))))


def scan_ref(lp, cfg, state=None):
    """The rule of include/rnnt_hip.h restated: cfg = (blank_threshold, S, R1, R2, R3), lp float32 values, state [frames, trailing,
    speech, rule, at] (None: zeros).  Returns the new state as a list of ints."""
    thr, S, R1, R2, R3 = cfg
    lt = log_thr(thr)
    frames, trailing, speech, rule, at = [0] * 5 if state is None else [int(v) for v in state]
    for x in np.asarray(lp, np.float32).reshape(-1):
        frames += 1
        if x > lt:                      # NaN compares false: speech
            trailing += 1
        else:
            trailing = 0
            speech += 1
        if rule == 0:
            r = 1 if (R1 > 0 and speech < S and trailing >= R1) else 2 if (R2 > 0 and speech >= S and trailing >= R2) else \
                3 if (R3 > 0 and frames >= R3) else 0
            if r:
                rule, at = r, frames
    return [frames, trailing, speech, rule, at]


def sub_len(frames):
    return ((frames - 3) // 2 + 1 - 3) // 2 + 1


def plan(frames, chunk):
    """[(start, length, offset, required = -1)]: equal chunks, the offset counting the encoder frames before each"""
    assert frames % chunk == 0
    return [(a, chunk, (a // chunk) * sub_len(chunk), -1) for a in range(0, frames, chunk)]


_CACHE = {}


def base_state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = T.make_state_dict(0)
    return _CACHE["sd"]


def state_dict(c):
    """the base weights with the head's blank bias raised by c (the other tensors are the base's own arrays)"""
    key = ("sd", c)
    if key not in _CACHE:
        sd = dict(base_state_dict())
        b = sd["ctc_head.ctc_lo.bias"].copy()
        b[BLANK] += np.float32(c)
        sd["ctc_head.ctc_lo.bias"] = b
        _CACHE[key] = sd
    return _CACHE[key]


def fbank(u):
    seed, frames, _ = UTTS[u]
    return T.synth_fbank(1, frames, seed=seed)[0]


def oracle_frames():
    """per utterance: the float64 oracle's encoder frames per chunk, [[t', 256] ...] (computed once: the encoder does not see c)"""
    if "enc" not in _CACHE:
        _CACHE["enc"] = [[r["frames"] for r in T.encoder_stream_ref(base_state_dict(), fbank(u), plan(UTTS[u][1], UTTS[u][2]))]
                         for u in range(len(UTTS))]
    return _CACHE["enc"]


def oracle_lp(c):
    """per utterance: the float64 blank log-posterior of every encoder frame per chunk, [[t'] ...]"""
    key = ("lp", c)
    if key not in _CACHE:
        sd = state_dict(c)
        w, b = sd["ctc_head.ctc_lo.weight"].astype(np.float64), sd["ctc_head.ctc_lo.bias"].astype(np.float64)
        out = []
        for chunks in oracle_frames():
            per = []
            for f in chunks:
                z = f @ w.T + b
                m = z.max(-1, keepdims=True)
                per.append(z[:, BLANK] - (m[:, 0] + np.log(np.exp(z - m).sum(-1))))
            out.append(per)
        _CACHE[key] = out
    return _CACHE[key]


def threshold(c):
    """(threshold, half-gap in log-posterior, pooled sorted log-posteriors)"""
    lp = np.sort(np.concatenate([np.concatenate(per) for per in oracle_lp(c)]))
    q10, q90 = np.quantile(lp, [0.1, 0.9])
    inside = np.nonzero((lp >= q10) & (lp <= q90))[0]                # consecutive indices: lp is sorted
    gaps = lp[inside[1:]] - lp[inside[:-1]]
    i = int(inside[1 + int(np.argmax(gaps))])
    return float(math.exp(0.5 * (lp[i - 1] + lp[i]))), float(0.5 * (lp[i] - lp[i - 1])), lp


def config(c, u):
    """(blank_threshold, S, R1, R2, R3) of utterance u under bias c"""
    return (threshold(c)[0],) + RULES[c][u]


def oracle_states(c, u, cfg=None):
    """the state after every chunk of utterance u under its config, by the Python restatement on the oracle's values as float32"""
    cfg = cfg or config(c, u)
    st, out = None, []
    for per in oracle_lp(c)[u]:
        st = scan_ref(per.astype(np.float32), cfg, st)
        out.append(st)
    return out
