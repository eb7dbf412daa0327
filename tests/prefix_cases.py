"""Inputs of the prefix-beam-search merge seam (rnnt_prefix_merge_host / rnnt_prefix_merge_device), shared by
test_prefix_beam_cpu.py and test_prefix_beam.py.  A case is (hyps [(tokens, score)], top_lp [n][k] f32, top_tok [n][k], beam_size);
the blank is BLANK and every hypothesis starts with it, as in the search."""
import itertools
import math

import numpy as np

import ctc_vr_amd.testing as T

BLANK = T.BLANK
MIN_GAP = 1e-6          # distinct survivor scores of the random cases differ by at least this after merging
SCORE_TOL = 1e-12       # both sides evaluate the same double formula with libm-grade exp / log


def _gap(hyps, top_lp, top_tok):
    sc = sorted(s for _, s, _, _ in T.prefix_merge_ref(hyps, top_lp, top_tok, BLANK, 10 ** 6))
    return min((b - a for a, b in zip(sc, sc[1:])), default=math.inf)


def _random(make, salt=0):
    """The first seed whose case keeps all survivor scores MIN_GAP apart (a condition on the inputs, checked with the Python
    restatement alone)."""
    for seed in range(100):
        hyps, top_lp, top_tok = make(np.random.default_rng([salt, seed]))
        if _gap(hyps, top_lp, top_tok) >= MIN_GAP:
            return hyps, top_lp, top_tok
    raise AssertionError("no seed gives well separated scores")


def _top(rng, n, k, pool):
    """top_lp [n][k] descending per row as a top-k is, top_tok [n][k] distinct per row, drawn from `pool`"""
    lp = -np.sort(rng.uniform(0.01, 12.0, size=(n, k)).astype(np.float32), axis=1)
    tok = np.stack([rng.permutation(pool)[:k] for _ in range(n)]).astype(np.int32)
    return lp, tok


def _distinct16(rng):
    hyps = [([BLANK, 100 + j], float(-rng.uniform(0.0, 30.0))) for j in range(16)]
    return (hyps,) + _top(rng, 16, 16, np.arange(0, 40))


def _merging16(rng):
    seqs = [list(s) for n in range(4) for s in itertools.product((1, 2, 3), repeat=n)][:16]     # prefixes of one another
    hyps = [([BLANK] + s, float(-rng.uniform(0.0, 30.0))) for s in seqs]
    return (hyps,) + _top(rng, 16, 16, np.arange(0, 16))                                         # every row holds blank, 1, 2 and 3


def _fuzz(rng):
    n, k = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    seqs = [list(s) for m in range(4) for s in itertools.product((1, 2), repeat=m)]
    pick = rng.permutation(len(seqs))[:n]
    hyps = [([BLANK] + seqs[i], float(-rng.uniform(0.0, 30.0))) for i in pick]
    return (hyps,) + _top(rng, n, k, np.array([BLANK, 1, 2, 3, 4, 6, 7, 8]))


def _f32(rows):
    return np.asarray(rows, np.float32)


def _i32(rows):
    return np.asarray(rows, np.int32)


NINF = -math.inf


def cases():
    c = {}
    c["minimal_n1_k1"] = ([([BLANK], 0.0)], _f32([[-0.5]]), _i32([[7]]), 1)
    c["distinct_16x16"] = _random(_distinct16) + (16,)
    c["merging_16x16"] = _random(_merging16) + (16,)
    # [5,1,2] + blank, [5,1] + 2 and a second [5,1,2] + blank: three candidates fold into the first, log-added in candidate order
    c["three_way_merge"] = ([([BLANK, 1, 2], -1.25), ([BLANK, 1], -0.75), ([BLANK, 1, 2], -2.5)],
                            _f32([[-0.3, -2.0], [-0.9, -1.1], [-0.2, -3.0]]), _i32([[BLANK, 9], [2, BLANK], [BLANK, 8]]), 3)
    # A = B + tok: (A + blank) listed first keeps A's slot 0; with the hypotheses swapped (B + tok) comes first and keeps B's slot 1
    c["merge_keeps_first_a_blank"] = ([([BLANK, 3, 4], -2.0), ([BLANK, 3], -1.0)], _f32([[-0.1, -4.0], [-0.2, -5.0]]), _i32([[BLANK, 1], [4, BLANK]]), 2)
    c["merge_keeps_first_b_tok"] = ([([BLANK, 3], -1.0), ([BLANK, 3, 4], -2.0)], _f32([[-0.2, -5.0], [-0.1, -4.0]]), _i32([[4, BLANK], [BLANK, 1]]), 2)
    c["all_minus_inf"] = ([([BLANK, 1], NINF), ([BLANK], NINF)], _f32([[-0.5, -1.0, -2.0], [-0.25, -1.5, -3.0]]), _i32([[BLANK, 2, 3], [1, BLANK, 4]]), 3)
    c["minus_inf_top_values"] = ([([BLANK], -1.0), ([BLANK, 2], -3.0)], _f32([[-0.5, NINF, NINF], [NINF, NINF, NINF]]), _i32([[1, BLANK, 2], [BLANK, 3, 4]]), 3)
    # exact f32 sums, no log-add: 0 - 1 = -0.5 - 0.5 = -0.25 - 0.75; equal scores keep candidate order
    c["ties_stable_order"] = ([([BLANK, 1], 0.0), ([BLANK, 2], -0.5), ([BLANK, 3], -0.25)],
                              _f32([[-1.0, -1.0, -2.0], [-0.5, -0.5, -1.5], [-0.75, -0.75, -1.75]]), _i32([[7, 8, 9], [7, 8, 9], [7, 8, 9]]), 3 * 3)
    c["truncate_at_tie"] = ([([BLANK, 1], 0.0), ([BLANK, 2], -0.5)], _f32([[-0.25, -1.0], [-0.5, -0.5]]), _i32([[7, 8], [7, 8]]), 2)
    c["k_above_n"] = _random(lambda rng: ([([BLANK, 1], -0.5), ([BLANK], -0.125)],) + _top(rng, 2, 5, np.arange(0, 8))) + (5,)
    c["beam_below_k"] = _random(lambda rng: ([([BLANK, 1], -0.5), ([BLANK], -0.125), ([BLANK, 1, 2], -3.0)],) + _top(rng, 3, 6, np.arange(0, 8))) + (2,)
    c["first_frame"] = ([([BLANK], 0.0)], _f32([[-0.01, -5.0, -6.5, -7.25]]), _i32([[BLANK, 17, 3, 411]]), 4)
    for i in range(8):
        c[f"fuzz{i}"] = _random(_fuzz, salt=1 + i) + (1 + 2 * i,)
    return c


def assert_same(got, want, exact_scores=False):
    """survivors, order and source slots exact; scores within SCORE_TOL (equal infinities are equal)"""
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[2:] for g in got] == [tuple(w[2:]) for w in want]
    for g, w in zip(got, want):
        assert g[1] == w[1] or abs(g[1] - w[1]) <= (0.0 if exact_scores else SCORE_TOL), (g[1], w[1])
