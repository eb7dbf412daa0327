"""Cases of the CTC prefix beam search tests (test_ctc_prefix_cpu.py, test_ctc_prefix.py): the golden fixtures recorded from the
reference, and crafted cases with exact ties whose expected result is the library's own definition, ctc_vr_amd.testing.ctc_prefix_beam_ref.

A case is (lp [B, T, V] float32, lens, blank, beam, phrases or None, context_score).

SCORE_TOL: both sides evaluate the same f64 recursion; they differ in the exp / log of each log-add only.  At most 64 frames times a
few ulp of an f64 log-add on magnitudes below 1e3 (ulp(1e3) ~ 1.1e-13) stays under 1e-10; 1e-9 leaves a decade.  Nothing is measured.
MIN_GAP: an order decided by two totals closer than the log-add error could differ between libm and the device; every case keeps the
non-tie differences of its top values and total scores (as the restatement alone computes them) at or above it.  Exact ties are
planted only between entries that run the same operations on the same numbers, which any implementation evaluates to the same bits."""
import math
import os

import numpy as np

import ctc_vr_amd.testing as T

SCORE_TOL = 1e-9
MIN_GAP = 1e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_SEARCH = ("v412_blank5_beam4", "v412_blank0_beam1", "v8_beam8")
NINF = -math.inf


def load(name):
    return np.load(os.path.join(GOLDEN, f"ctc_prefix_{name}.npz"), allow_pickle=False)


def phrases_of(z):
    off = np.cumsum([0] + z["phrase_lens"].tolist())
    return [z["phrase_tokens"][a:b].tolist() for a, b in zip(off, off[1:])]


def golden_cases():
    """name -> (case, want): want per utterance [(tokens, score, times)] as the reference returned them."""
    out = {}
    for name in GOLDEN_SEARCH:
        z = load(name)
        for tag in ("plain", "ctx"):
            case = (z["lp"], z["lens"].tolist(), int(z["blank"]), int(z["beam"]), phrases_of(z) if tag == "ctx" else None, float(z["context_score"]))
            want = [[(z[f"{tag}_tok"][b, i, :z[f"{tag}_len"][b, i]].tolist(), float(z[f"{tag}_score"][b, i]),
                      z[f"{tag}_times"][b, i, :z[f"{tag}_len"][b, i]].tolist()) for i in range(z[f"{tag}_n_hyp"][b])] for b in range(len(z["lens"]))]
            out[f"{name}_{tag}"] = (case, want)
    return out


def _rows(seed, B, T, V):
    x = 2.0 * np.random.default_rng(seed).standard_normal((B, T, V))
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def _seeded(B, T, V, lens, blank, beam, phrases, score):
    """log-softmax rows of the first seed whose case has no finite tie and no difference below MIN_GAP, judged by the restatement alone"""
    for seed in range(1000):
        lp = _rows(seed, B, T, V)
        case, st = (lp, lens, blank, beam, phrases, score), {}
        reference_of(case, st)
        if st.get("nonzero_gap", math.inf) >= MIN_GAP and not st.get("top_ties") and not st.get("prune_ties"):
            return case
    raise AssertionError("no seed satisfies the gap condition")


def crafted_cases():
    c = {}
    # every value of every frame equal: the top list is the lowest indices, and symmetric entries tie at every prune
    c["equal_frame_values"] = (np.full((1, 3, 6), -1.5, np.float32), [3], 0, 3, None, 0.0)
    # tokens 1, 2, 3 equal and ahead of the blank: [1] and [2] tie (insertion order), 3 is cut from the top list at a tie
    lp = np.full((1, 3, 5), -6.0, np.float32)
    lp[0, :, 1:4] = -1.0
    lp[0, :, 0] = -4.0
    c["ties_at_the_cut"] = (lp, [3], 0, 2, None, 0.0)
    # -inf almost everywhere: fewer finite values than the beam, totals of -inf ordered by insertion
    lp = np.full((2, 4, 5), NINF, np.float32)
    lp[0, :, 0], lp[0, :, 2] = -0.5, -1.25
    lp[1, :, 3] = -0.25
    lp[1, 1:3, 0] = -2.0
    c["minus_inf"] = (lp, [4, 3], 0, 4, None, 0.0)
    c["length_zero"] = _seeded(2, 3, 5, [0, 3], 0, 3, None, 0.0)
    c["length_zero_ctx"] = _seeded(2, 3, 5, [0, 3], 0, 3, [[1, 2]], 2.0)
    c["beam_one"] = _seeded(1, 7, 6, [7], 2, 1, None, 0.0)
    # the repeat branch raises v_ns of [1, 3] after the extension of [1] by 3 set its times: times_ns keeps the extension's
    lp = np.array([[[-3.0, -2.0, -3.5, -5.25], [-5.5, -1.5, -3.75, -1.25], [-3.75, -5.0, -5.75, -1.0], [-1.75, -2.0, -2.25, -1.0],
                    [-4.5, -3.25, -5.75, -5.5]]], np.float32)
    c["stale_times"] = (lp, [5], 0, 3, None, 0.0)
    c["ragged_ctx"] = _seeded(3, 9, 7, [9, 4, 6], 0, 5, [[1, 2], [2, 3, 1], [2], [1, 2]], 1.0)
    c["ragged_plain"] = _seeded(3, 9, 7, [9, 4, 6], 0, 5, None, 0.0)
    # a prefix is pruned and comes back while its extension stays live (seeds found with the restatement's "rebuilt_parent" count)
    c["rebuilt_parent_a"] = (_rows(1745, 1, 8, 4), [8], 0, 2, None, 0.0)
    c["rebuilt_parent_b"] = (_rows(29300, 1, 8, 4), [8], 0, 2, None, 0.0)
    c["beam_sixteen"] = _seeded(2, 6, 40, [6, 5], 39, 16, [[3, 4], [4]], 0.75)
    return c


def reference_of(case, stats=None):
    """the restatement per utterance: [(tokens, score, times, context score)]"""
    lp, lens, blank, beam, phrases, score = case
    g = T.context_graph_ref(phrases, score) if phrases else None
    return [T.ctc_prefix_beam_ref(lp[b], lens[b], blank, beam, g, stats)[0] for b in range(len(lens))]


def assert_same(got, want, what=""):
    """got [(tokens, score, times, ...)] of the library against want [(tokens, score, times, ...)]: tokens, times and order exact (a
    times list shorter than its tokens -- possible only with -inf values -- is zero-filled by the library), scores within SCORE_TOL"""
    assert len(got) == len(want), f"{what}: {len(got)} utterances, want {len(want)}"
    for b, (g, w) in enumerate(zip(got, want)):
        assert [h[0] for h in g] == [h[0] for h in w], f"{what} row {b}: tokens / order"
        assert [h[2] for h in g] == [list(h[2]) + [0] * (len(h[0]) - len(h[2])) for h in w], f"{what} row {b}: times"
        for i, (x, y) in enumerate(zip(g, w)):
            assert x[1] == y[1] or abs(x[1] - y[1]) <= SCORE_TOL, f"{what} row {b} hyp {i}: score {x[1]!r} != {y[1]!r}"
            if len(x) > 3 and len(y) > 3:
                assert x[3] == y[3], f"{what} row {b} hyp {i}: context score {x[3]!r} != {y[3]!r}"


def assert_zero_fill(raw):
    """entries of hypotheses i >= n_hyp[b], and of a row beyond its length, are zero"""
    nh, lens, toks, times, sc, cs = raw
    for b in range(len(nh)):
        assert not lens[b, nh[b]:].any() and not sc[b, nh[b]:].any() and not cs[b, nh[b]:].any()
        for i in range(lens.shape[1]):
            n = lens[b, i] if i < nh[b] else 0
            assert not toks[b, i, n:].any() and not times[b, i, n:].any()
