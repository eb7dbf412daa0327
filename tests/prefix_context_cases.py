"""Inputs of the prefix-beam-search merge seam with a context graph (rnnt_prefix_merge_ctx_host / rnnt_prefix_merge_ctx_device), shared
by test_prefix_context_cpu.py and test_prefix_context.py.  A case is (hyps [(tokens, score, context state, context score)], top_lp
[n][k] f32, top_tok [n][k], beam_size); all cases share ONE graph (PHRASES, SCORE), so the device test uploads it once.

The cases of prefix_cases.py come twice: "walk" gives every hypothesis the context state and score its own tokens lead to (what a
search would hold), "seed" gives it a seeded random node and score (any state the kernel may be handed, deep fail chains included).
The random ones among them are kept only if the totals of all their distinct survivors are MIN_GAP apart under the Python
restatement, so that the order is defined on both sides; the crafted ones are below."""
import math

import numpy as np

import ctc_vr_amd.testing as T
from prefix_cases import BLANK, MIN_GAP, _f32, _i32, cases as plain_cases

# tokens of prefix_cases.py: 0 .. 40 and 100 .. 115; none is the blank (5).  SCORE is not a dyadic rational: the sums round.
PHRASES = [[1, 2, 3], [2, 3], [3, 4, 6], [7], [1, 2, 4], [100, 7], [8, 9, 1], [3, 4, 6, 8, 2]]
SCORE = 1.7
RANDOM = ("distinct_16x16", "merging_16x16", "k_above_n", "beam_below_k") + tuple(f"fuzz{i}" for i in range(8))


def graph():
    return T.context_graph_ref(PHRASES, SCORE)


def walked(g, hyps):
    """(tokens, score) -> (tokens, score, state, context score) after the tokens behind the leading blank went through the graph"""
    out = []
    for toks, score in hyps:
        steps, states, _ = g.walk(toks[1:])
        cs = 0.0
        for s in steps:
            cs = cs + s
        out.append((list(toks), score, states[-1] if states else 0, cs))
    return out


def seeded(g, hyps, rng):
    n = len(g.token)
    return [(list(toks), score, int(rng.integers(0, n)), float(rng.uniform(-8.0, 8.0))) for toks, score in hyps]


def total_gap(g, hyps, top_lp, top_tok):
    tot = sorted(r[1] + r[5] for r in T.prefix_merge_ctx_ref(hyps, top_lp, top_tok, BLANK, 10 ** 6, g) if math.isfinite(r[1]))
    return min((b - a for a, b in zip(tot, tot[1:])), default=math.inf)


def cases():
    """-> (cases, dropped): the random cases whose totals come closer than MIN_GAP are dropped and listed"""
    g = graph()
    c, dropped = {}, []
    for i, (name, (hyps, top_lp, top_tok, beam)) in enumerate(sorted(plain_cases().items())):
        for kind, hy in (("walk", walked(g, hyps)), ("seed", seeded(g, hyps, np.random.default_rng([7, i])))):
            if name in RANDOM and total_gap(g, hy, top_lp, top_tok) < MIN_GAP:
                dropped.append(f"{name}_{kind}")
                continue
            c[f"{name}_{kind}"] = (hy, top_lp, top_tok, beam)
    w = lambda hyps: walked(g, hyps)
    # [7] is a phrase: + SCORE for entering, + SCORE again for completing it (output score); 9 is in no phrase.  -0.5 < -3.0 + 3.4
    c["boost_reorders"] = (w([([BLANK], 0.0)]), _f32([[-0.5, -3.0]]), _i32([[9, 7]]), 2)
    # [3, 4] is two tokens into [3, 4, 6]: token 9 leaves through the fail arc to the root and gives the 2 * SCORE back
    c["fail_arc_negative"] = (w([([BLANK, 3, 4], -1.0)]), _f32([[-0.25, -0.5, -4.0]]), _i32([[9, 6, BLANK]]), 3)
    # [1, 2] + 3 completes [1, 2, 3] whose fail arc [2, 3] is a phrase too: token score + both output scores
    c["phrase_completes"] = (w([([BLANK, 1, 2], -1.0), ([BLANK, 1], -0.5)]), _f32([[-0.5, -1.0], [-0.75, -2.0]]), _i32([[3, 9], [9, 2]]), 4)
    # blank-kept [1, 2] meets [1] + 2: both arrive with the same context state and score; the first one's stay, either way round
    c["ab_meets_a_plus_b"] = (w([([BLANK, 1, 2], -2.0), ([BLANK, 1], -1.0)]), _f32([[-0.1, -4.0], [-0.2, -5.0]]), _i32([[BLANK, 9], [2, BLANK]]), 2)
    c["a_plus_b_meets_ab"] = (w([([BLANK, 1], -1.0), ([BLANK, 1, 2], -2.0)]), _f32([[-0.2, -5.0], [-0.1, -4.0]]), _i32([[2, BLANK], [BLANK, 9]]), 2)
    # exactly equal totals without a log-add: 0 - 1 + 0 = -3 - 0.5 + 2.5 (context score given, not walked) = -1; candidate order decides
    c["equal_totals_low_first"] = ([([BLANK, 20], 0.0, 0, 0.0), ([BLANK, 21], -3.0, 0, 2.5)], _f32([[-1.0, -9.0], [-0.5, -9.5]]), _i32([[30, 31], [30, 31]]), 2)
    c["equal_totals_high_first"] = ([([BLANK, 21], -3.0, 0, 2.5), ([BLANK, 20], 0.0, 0, 0.0)], _f32([[-0.5, -9.5], [-1.0, -9.0]]), _i32([[30, 31], [30, 31]]), 2)
    # n_hyp = k = beam = 16 with every hypothesis inside or next to a phrase and every row holding phrase tokens
    rng = np.random.default_rng(16)
    for seed in range(100):
        rng = np.random.default_rng([16, seed])
        seqs = [[1], [1, 2], [2], [3], [3, 4], [3, 4, 6], [3, 4, 6, 8], [8], [8, 9], [100], [7], [1, 2, 4], [2, 3], [9], [4], []]
        hyps = w([([BLANK] + s, float(-rng.uniform(0.0, 10.0))) for s in seqs])
        lp = -np.sort(rng.uniform(0.01, 12.0, size=(16, 16)).astype(np.float32), axis=1)
        tok = np.stack([rng.permutation(np.array([BLANK, 1, 2, 3, 4, 6, 7, 8, 9, 100, 10, 11, 12, 13, 14, 15, 16, 17]))[:16] for _ in range(16)]).astype(np.int32)
        if total_gap(g, hyps, lp, tok) >= MIN_GAP:
            break
    else:
        raise AssertionError("no seed gives well separated totals")
    c["full_16x16x16"] = (hyps, lp, tok, 16)
    return c, dropped


def assert_same_ctx(got, want, score_tol):
    """survivors, order, source row / slot and context states exact; context scores exactly equal; fused scores within score_tol"""
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[2:5] for g in got] == [tuple(w[2:5]) for w in want]
    assert [g[5] for g in got] == [w[5] for w in want]
    for g, w in zip(got, want):
        assert g[1] == w[1] or abs(g[1] - w[1]) <= score_tol, (g[1], w[1])
