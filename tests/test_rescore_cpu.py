"""CPU-side checks of two-pass decoding: the five device entry points and the host one exist at every layer of the boundary with
matching signatures, the choice among re-scored hypotheses (rnnt_rescore_select_host) equals a Python restatement of the reference's
loop bit for bit, and the facade says what it cannot do before it needs an engine."""
import ctypes
import math
import os
import re
import struct

import numpy as np
import pytest

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# parameters per entry point as the issue states them (context included)
N_ARGS = {"rnnt_transducer_nll_nbest": 13, "rnnt_rescore_select_host": 7, "rnnt_stream_keep_frames": 4, "rnnt_stream_get_frames": 7,
          "rnnt_pool_rescore": 10}


def _header_params(src, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"include/rnnt_hip.h does not declare {name}"
    return [p.strip() for p in m.group(1).split(",")]


def _ctype_of(param):
    if "*" in param:
        return "ptr"
    return "double" if param.startswith("double") else "i32"


def test_symbols_in_header_library_and_table_with_matching_signatures():
    src = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = rlib.load()
    for s, n in N_ARGS.items():
        params = _header_params(src, s)
        assert hasattr(lib, s), f"librnnt_hip.so does not export {s}"
        assert s in rlib.SIGNATURES, f"lib.SIGNATURES has no {s}"
        res, args = rlib.SIGNATURES[s]
        assert res is rlib.c_i32 and len(args) == len(params) == n, (s, len(args), len(params))
        for a, p in zip(args, params):
            want = _ctype_of(p)
            got = "double" if a is ctypes.c_double else ("i32" if a is rlib.c_i32 else "ptr")
            assert got == want, (s, p, a)
    assert lib.rnnt_abi_version() == 3                          # additive change
    for w in ("transducer_nll_nbest", "rescore_select", "stream_keep_frames", "stream_frames", "pool_rescore"):
        assert callable(getattr(rlib.RnntEngine, w)), w


def test_a_null_context_is_refused():
    lib = rlib.load()
    one = np.ones(4, np.int32)
    nll = np.zeros(4, np.float64)
    p = one.ctypes.data
    n = ctypes.c_int32(0)
    assert lib.rnnt_transducer_nll_nbest(None, p, p, p, p, p, 1, 1, 1, 1, nll.ctypes.data, None, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_keep_frames(None, 0, 1, None) == rlib.ERR_ARG
    assert lib.rnnt_stream_get_frames(None, 0, 0, 0, None, ctypes.byref(n), None) == rlib.ERR_ARG
    assert lib.rnnt_pool_rescore(None, 1, p, p, p, p, 1, 1, nll.ctypes.data, None) == rlib.ERR_ARG


def _bits(x):
    return [struct.pack("<d", float(v)) for v in x]


def _seeded_lists():
    g = np.random.Generator(np.random.Philox(key=[11, 0x5E]))
    for n in (2, 5, 10, 16):
        for _ in range(6):
            first = -np.abs(g.standard_normal(n)) * 40.0
            nll = np.abs(g.standard_normal(n)) * 60.0 + 1.0
            yield first, nll, float(g.uniform(0, 1)), float(g.uniform(0, 1))


INF, NAN = math.inf, math.nan
SELECT_CASES = {
    # name: (first scores, nll, first weight, transducer weight, expected best or None)
    "exact_tie_first_wins": ([-3.0, -1.0, -1.0, -2.0], [4.0, 2.0, 2.0, 0.5], 0.5, 0.25, 1),
    "tie_everywhere": ([-1.0, -1.0, -1.0], [2.0, 2.0, 2.0], 0.3, 0.7, 0),
    "minus_inf_times_zero_is_nan_never_chosen": ([-INF, -5.0, -INF, -4.0], [1.0, 2.0, 0.1, 9.0], 0.0, 1.0, 1),
    "minus_inf_first_with_weight": ([-INF, -5.0], [1.0, 2.0], 0.5, 1.0, 1),
    "all_nan": ([NAN, NAN, NAN], [1.0, 2.0, 3.0], 0.3, 0.7, 0),
    "all_nan_from_zero_weights": ([-INF, -INF], [INF, INF], 0.0, 0.0, 0),
    "both_weights_zero": ([-3.0, -1.0, -2.0], [4.0, 2.0, 8.0], 0.0, 0.0, 0),
    "one_hypothesis": ([-7.5], [12.25], 0.3, 0.7, 0),
    "one_hypothesis_nan": ([-INF], [1.0], 0.0, 1.0, 0),
    "infinite_nll": ([-1.0, -2.0], [INF, 3.0], 0.3, 0.7, 1),
}


def _check_select(first, nll, fw, tw, expect=None):
    best, total = rlib.rescore_select(first, nll, fw, tw)
    want_best, want_total = T.rescore_select_ref(first, nll, fw, tw)
    assert _bits(total) == _bits(want_total), (first, nll, fw, tw, total, want_total)
    assert best == want_best
    if expect is not None:
        assert best == expect


def test_select_matches_the_reference_loop_on_seeded_lists():
    k = 0
    for first, nll, fw, tw in _seeded_lists():
        _check_select(first, nll, fw, tw)
        k += 1
    assert k == 24


@pytest.mark.parametrize("case", sorted(SELECT_CASES))
def test_select_edge_cases(case):
    first, nll, fw, tw, expect = SELECT_CASES[case]
    _check_select(np.array(first), np.array(nll), fw, tw, expect)
    if case == "minus_inf_times_zero_is_nan_never_chosen":
        _, total = rlib.rescore_select(first, nll, fw, tw)
        assert math.isnan(total[0]) and math.isnan(total[2]) and total[1] == -2.0


def test_select_is_not_contracted_into_a_fused_multiply_add():
    """a * b + c * d with a fused multiply-add rounds once instead of twice: operands chosen so that the two differ"""
    first, fw = np.array([1.0 + 2.0 ** -30]), 1.0 + 2.0 ** -30          # the product needs 61 bits
    nll, tw = np.array([1.0 + 2.0 ** -29]), 1.0
    _check_select(first, nll, fw, tw)
    _, total = rlib.rescore_select(first, nll, fw, tw)
    assert total[0] == 0.0                                      # fused: 2^-60, the bits the rounded product drops


def test_select_refuses_bad_arguments():
    lib = rlib.load()
    a = np.zeros(2, np.float64)
    best = ctypes.c_int32(0)
    p = a.ctypes.data
    assert lib.rnnt_rescore_select_host(0, p, p, 1.0, 1.0, p, ctypes.byref(best)) == rlib.ERR_ARG
    assert lib.rnnt_rescore_select_host(2, None, p, 1.0, 1.0, p, ctypes.byref(best)) == rlib.ERR_ARG
    assert lib.rnnt_rescore_select_host(2, p, None, 1.0, 1.0, p, ctypes.byref(best)) == rlib.ERR_ARG
    assert lib.rnnt_rescore_select_host(2, p, p, 1.0, 1.0, p, None) == rlib.ERR_ARG


def test_pack_nbest():
    nh, hl, ht = rlib.pack_nbest([[[3, 4], []], [[7]]])
    assert nh.tolist() == [2, 1] and hl.tolist() == [[2, 0], [1, 0]] and ht.shape == (2, 2, 2)
    assert ht[0, 0].tolist() == [3, 4] and ht[1, 0, 0] == 7
    nh, hl, ht = rlib.pack_nbest([[[]]], N=3, umax=5)
    assert nh.tolist() == [1] and hl.shape == (1, 3) and ht.shape == (1, 3, 5)


def test_facade_says_no_before_any_engine_exists():
    """The object is not even initialised (no context, no GPU): the three refusals come first."""
    import torch
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    m = OnlineRNNTModel.__new__(OnlineRNNTModel)
    assert not hasattr(m, "_engine")
    x, n = torch.zeros(1, 40, 80), torch.tensor([40])
    with pytest.raises(ValueError, match="attention decoder"):
        m.transducer_attention_rescoring(x, n, 4, attn_weight=0.5)
    with pytest.raises(ValueError, match="attention decoder"):
        m.transducer_attention_rescoring(x, n, 4, reverse_weight=0.3)
    with pytest.raises(ValueError, match="full-context"):
        m.transducer_attention_rescoring(x, n, 4, decoding_chunk_size=16)
    with pytest.raises(ValueError, match="beam_search_type"):
        m.transducer_attention_rescoring(x, n, 4, beam_search_type="attention")
    with pytest.raises(ValueError, match="beam_search_type"):
        m.rescoring_batch(x, n, beam_search_type="greedy")


def test_select_rescored_shapes_an_utterance():
    from ctc_vr_amd.online_rnnt_model import select_rescored
    best, rows = select_rescored([[1, 2], [3]], [-1.0, -2.0], np.array([10.0, 4.0]), 0.5, 0.5)
    assert best == 1 and rows[1] == ([3], -2.0, -4.0, -2.0 * 0.5 + -4.0 * 0.5) and rows[0][3] == -1.0 * 0.5 + -10.0 * 0.5
    best, rows = select_rescored([[1]], [-1.0], None, 0.5, 0.5)
    assert best == 0 and rows[0][0] == [1] and math.isnan(rows[0][2]) and math.isnan(rows[0][3])
