"""CPU checks of forced alignment: the float64 restatements of the two Viterbi recursions (ctc_vr_amd.testing) against explicit
enumeration of every path -- score bitwise, path equal, ties resolved by the rule that is part of the contract -- the host helpers
against the reference's recorded outputs (tests/golden/timestamps_cases.npz), and the ABI table."""
import math
import os

import numpy as np
import pytest

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.online_rnnt_model import peaks_from_ctc_alignment, timestamps_from_peaks

V, BLANK = 12, 4          # a small vocabulary: the recursions only index it

TRANSDUCER_SHAPES = [(1, 0), (1, 3), (2, 1), (3, 0), (4, 2), (5, 5), (6, 4), (6, 5), (3, 5), (6, 1)]   # (T_b, U_b): T_b = 1 and U_b = 0 included
CTC_CASES = [          # (T_b, transcript): adjacent repeats, L = 0, and pairs with no frame to spare
    (1, []), (4, []), (1, [7]), (3, [7]), (5, [7, 9]), (7, [7, 7]), (7, [1, 1, 2]), (6, [3, 5, 3]), (7, [9, 9, 9]), (5, [2, 2, 6]), (3, [1, 2, 3]),
]


def _rng(*key):
    return np.random.Generator(np.random.Philox(key=list(key)))


def _lattice(T_b, U_b, seed, quantised=False):
    """[T_b + 1, U_b + 2, 2] float32: one row and one column of NaN padding around the valid cells (never read)"""
    g = _rng(seed, 0xA1)
    shape = (T_b + 1, U_b + 2, 2)
    p = (-0.25 * g.integers(0, 8, shape)).astype(np.float32) if quantised else (-g.random(shape, dtype=np.float32) * 6).astype(np.float32)
    p[T_b:] = np.nan
    p[:, U_b + 1:] = np.nan
    p[:, U_b, 1] = np.nan           # no label slot at u = U_b
    return p


def _logprobs(T_b, seed, quantised=False):
    g = _rng(seed, 0xC7)
    return (-0.25 * g.integers(0, 6, (T_b, V))).astype(np.float32) if quantised else (-g.random((T_b, V), dtype=np.float32) * 6).astype(np.float32)


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("shape", TRANSDUCER_SHAPES)
def test_transducer_ref_vs_bruteforce(shape):
    T_b, U_b = shape
    for seed in range(6):
        p = _lattice(T_b, U_b, 100 * T_b + 10 * U_b + seed)
        best, emit, margin = T.transducer_align_ref(p, T_b, U_b)
        paths = T.transducer_align_bruteforce(p, T_b, U_b)
        assert len(paths) == math.comb(T_b - 1 + U_b, U_b)
        if len(paths) > 1:
            assert paths[0][0] != paths[1][0], "seed gives a tie: choose another"
        assert _bits(best) == _bits(paths[0][0])
        assert tuple(emit) == paths[0][1] and emit.dtype == np.int32
        assert all(emit[i] <= emit[i + 1] for i in range(U_b - 1)) and all(0 <= t < T_b for t in emit)
        # every cell of a T_b = 1 or U_b = 0 lattice lies on the only path: no margin
        if T_b == 1 or U_b == 0:
            assert margin == math.inf
        else:
            assert 0 < margin < math.inf


def test_transducer_margin_is_the_gap_to_the_best_path_elsewhere():
    """margin against the enumeration: the best score among the paths that leave the best path's cells"""
    for seed in range(8):
        T_b, U_b = 5, 3
        p = _lattice(T_b, U_b, 900 + seed).astype(np.float64)
        best, emit, margin = T.transducer_align_ref(p, T_b, U_b)
        others = [s for s, e in T.transducer_align_bruteforce(p, T_b, U_b) if e != tuple(emit)]
        assert margin == pytest.approx(best - max(others), abs=1e-12)


@pytest.mark.parametrize("shape", TRANSDUCER_SHAPES)
def test_transducer_tie_rule_on_quantised_lattices(shape):
    """multiples of 0.25: every sum is exact, ties are everywhere, and the path is the one the rule names"""
    T_b, U_b = shape
    tied = 0
    for seed in range(12):
        p = _lattice(T_b, U_b, 5000 + 100 * T_b + 10 * U_b + seed, quantised=True)
        best, emit, _ = T.transducer_align_ref(p, T_b, U_b)
        paths = T.transducer_align_bruteforce(p, T_b, U_b)       # equal scores: sorted by the tie rule
        tied += len(paths) > 1 and paths[0][0] == paths[1][0]
        assert _bits(best) == _bits(paths[0][0]) and tuple(emit) == paths[0][1]
    if T_b > 1 and U_b > 0 and math.comb(T_b - 1 + U_b, U_b) > 4:
        assert tied > 0, "no tie among the cases: the rule was not exercised"


def _feasible(T_b, y):
    return T_b >= len(y) + sum(a == b for a, b in zip(y, y[1:]))


@pytest.mark.parametrize("case", CTC_CASES, ids=lambda c: f"T{c[0]}_{'-'.join(map(str, c[1])) or 'empty'}")
def test_ctc_ref_vs_bruteforce(case):
    T_b, y = case
    for seed in range(6):
        lp = _logprobs(T_b, 10 * T_b + len(y) + 1000 * seed)
        best, align = T.ctc_align_ref(lp, y, T_b, BLANK)
        paths = T.ctc_align_bruteforce(lp, y, T_b, BLANK)
        assert bool(paths) == _feasible(T_b, y)
        if len(paths) > 1:
            assert paths[0][0] != paths[1][0], "seed gives a tie: choose another"
        ext = T._ctc_ext(y, BLANK)
        assert _bits(best) == _bits(paths[0][0])
        assert align.tolist() == [ext[s] for s in paths[0][1]] and align.dtype == np.int32
        collapsed = [int(a) for i, a in enumerate(align) if a != BLANK and (i == 0 or a != align[i - 1])]
        assert collapsed == y


@pytest.mark.parametrize("case", [(6, [8, 8, 8, 8, 8]), (2, [1, 1]), (1, [3, 5]), (3, [7, 7, 9])], ids=str)
def test_ctc_infeasible(case):
    T_b, y = case
    assert not _feasible(T_b, y)
    best, align = T.ctc_align_ref(_logprobs(T_b, 77), y, T_b, BLANK)
    assert best == -math.inf and align.tolist() == [-1] * T_b
    assert T.ctc_align_bruteforce(_logprobs(T_b, 77), y, T_b, BLANK) == []


@pytest.mark.parametrize("case", [c for c in CTC_CASES if _feasible(*c)], ids=lambda c: f"T{c[0]}_{'-'.join(map(str, c[1])) or 'empty'}")
def test_ctc_tie_rule_on_quantised_logprobs(case):
    T_b, y = case
    ext = T._ctc_ext(y, BLANK)
    tied = 0
    for seed in range(12):
        lp = _logprobs(T_b, 7000 + 10 * T_b + len(y) + 1000 * seed, quantised=True)
        best, align = T.ctc_align_ref(lp, y, T_b, BLANK)
        paths = T.ctc_align_bruteforce(lp, y, T_b, BLANK)
        tied += len(paths) > 1 and paths[0][0] == paths[1][0]
        assert _bits(best) == _bits(paths[0][0]) and align.tolist() == [ext[s] for s in paths[0][1]]
    if len(T.ctc_align_bruteforce(_logprobs(T_b, 1), y, T_b, BLANK)) > 4:
        assert tied > 0, "no tie among the cases: the rule was not exercised"


@pytest.mark.parametrize("shape", TRANSDUCER_SHAPES)
def test_best_path_against_the_total_likelihood(shape):
    """the best path is one term of the sum over all alignments: best <= -nll <= best + log(number of alignments)"""
    T_b, U_b = shape
    p = _lattice(T_b, U_b, 31 + T_b + 10 * U_b)
    best, _, _ = T.transducer_align_ref(p, T_b, U_b)
    total = -T.transducer_nll_ref(p, T_b, U_b)
    n = math.comb(T_b - 1 + U_b, U_b)
    assert best <= total <= best + math.log(n)


# ---- host helpers against the reference's recorded outputs -------------------------------------------------------------------------
def _rows(flat, off):
    return [flat[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def test_peaks_reproduce_the_reference(golden):
    z = golden("timestamps_cases.npz")
    hyps, want = _rows(z["hyp_flat"], z["hyp_off"]), _rows(z["peak_flat"], z["peak_off"])
    assert len(hyps) >= 100 and [] in hyps
    for hyp, blank, w in zip(hyps, z["hyp_blank"].tolist(), want):
        assert peaks_from_ctc_alignment(hyp, blank) == w
        assert peaks_from_ctc_alignment(np.array(hyp, np.int32), blank) == w      # the engine's rows are arrays


def test_timestamps_reproduce_the_reference(golden):
    z = golden("timestamps_cases.npz")
    peaks = _rows(z["ts_peaks_flat"], z["ts_peaks_off"])
    off, want = z["ts_peaks_off"], z["ts_times_flat"]
    assert len(peaks) >= 100 and [] in peaks and any(len(p) == 1 for p in peaks)
    clipped = far = near = 0
    for i, (pk, (max_duration, frame_rate, max_tok)) in enumerate(zip(peaks, z["ts_args"].tolist())):
        got = timestamps_from_peaks(pk, max_duration, frame_rate, max_tok)
        w = want[off[i]:off[i + 1]]
        assert len(got) == len(pk)
        for (s, e), (ws, we) in zip(got, w.tolist()):
            assert s == ws and e == we                       # float equality: same operations in the same order
        if pk:
            clipped += got[-1][1] == max_duration
            gaps = np.diff(pk) * frame_rate
            far += bool((gaps > max_tok).any())
            near += bool((gaps < max_tok).any())
    assert clipped > 0 and far > 0 and near > 0              # the cases the fixture was generated for are in it
    assert timestamps_from_peaks([5], 10.0) == [(0, 0.7)] and timestamps_from_peaks([], 1.0) == []


def test_signatures_cover_the_alignment_symbols():
    import ctypes
    want = {"rnnt_transducer_align": 13, "rnnt_transducer_align_pick": 10, "rnnt_ctc_align": 11, "rnnt_ctc_align_logprobs": 11}
    for name, n in want.items():
        res, args = rlib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == n
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rnnt_hip.h")).read()
    for name in want:
        assert f"int {name}(" in header
