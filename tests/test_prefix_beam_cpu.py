"""The merge of the device prefix beam search as a pure function: rnnt_prefix_merge_host (the C++ statement of one frame of
wenet/transducer/search/prefix_beam_search.py:105-145 for one utterance) against its Python restatement
ctc_vr_amd.testing.prefix_merge_ref.  Survivors, order and source slots exact; scores within 1e-12 absolute: both sides evaluate the
same double formula with libm-grade exp / log, and a few ulp at |score| < 1e3 is far below that.  No GPU."""
import math

import numpy as np
import pytest

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import RnntError, prefix_merge_host
from prefix_cases import BLANK, MIN_GAP, assert_same, cases

CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_merge_equals_python_restatement(name):
    hyps, top_lp, top_tok, beam = CASES[name]
    want = T.prefix_merge_ref(hyps, top_lp, top_tok, BLANK, beam)
    assert 1 <= len(want) <= beam
    assert_same(prefix_merge_host(hyps, top_lp, top_tok, BLANK, beam), want)


def test_cases_are_what_they_claim():
    """The properties the cases are named for hold for the restatement itself: merges happen where they should, the planted ties
    are exact, the first candidate's source slot stays, the log-add runs in candidate order."""
    ref = lambda name, beam=None: T.prefix_merge_ref(*CASES[name][:3], BLANK, CASES[name][3] if beam is None else beam)
    assert len(ref("distinct_16x16", 10 ** 6)) == 256
    assert len(ref("merging_16x16", 10 ** 6)) == 256 - 15                       # every hypothesis but [blank] is also (its parent + token)
    for name in ("distinct_16x16", "merging_16x16", "k_above_n", "beam_below_k"):
        sc = sorted(s for _, s, _, _ in ref(name, 10 ** 6))
        assert min(b - a for a, b in zip(sc, sc[1:])) >= MIN_GAP
    a, b, c = np.float32(-1.25) + np.float32(-0.3), np.float32(-0.75) + np.float32(-0.9), np.float32(-2.5) + np.float32(-0.2)
    lse = lambda x, y: max(x, y) + math.log(math.exp(x - max(x, y)) + math.exp(y - max(x, y)))
    top = ref("three_way_merge")[0]
    assert top[0] == [BLANK, 1, 2] and top[2:] == (0, 0) and top[1] == lse(lse(float(a), float(b)), float(c))
    assert ref("merge_keeps_first_a_blank")[0][0] == [BLANK, 3, 4] and ref("merge_keeps_first_a_blank")[0][2:] == (0, 0)
    assert ref("merge_keeps_first_b_tok")[0][0] == [BLANK, 3, 4] and ref("merge_keeps_first_b_tok")[0][2:] == (0, 1)
    assert [s for _, s, _, _ in ref("all_minus_inf")] == [-math.inf] * 3
    assert [r[2:] for r in ref("all_minus_inf")] == [(0, 0), (0, 1), (0, 1)]          # [5,1] twice: hypothesis 0 + blank, then 1 + tok 1
    assert [s for _, s, _, _ in ref("ties_stable_order")] == [-1.0] * 6 + [-2.0] * 3
    assert [r[2] for r in ref("ties_stable_order")] == [0, 0, 1, 1, 2, 2, 0, 1, 2]
    assert [(r[0], r[1]) for r in ref("truncate_at_tie")] == [([BLANK, 1, 7], -0.25), ([BLANK, 1, 8], -1.0)]
    assert ref("first_frame")[0] == ([BLANK], float(np.float32(-0.01)), 0, 0)


def test_host_merge_refuses_bad_arguments():
    with pytest.raises(RnntError):
        prefix_merge_host([([BLANK], 0.0)], np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int32), BLANK, 0)
