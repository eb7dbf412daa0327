"""CPU-side checks of teacher-forced scoring: the two entry points exist at every layer of the boundary, the float64 dynamic
programme equals an explicit sum over alignments, and the facade's loss composition is the reference's."""
import math
import os
import re

import numpy as np
import pytest

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rnnt_transducer_nll", "rnnt_ctc_nll")


def test_scoring_symbols_in_header_library_and_table():
    src = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = rlib.load()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"include/rnnt_hip.h does not declare {s}"
        assert hasattr(lib, s), f"librnnt_hip.so does not export {s}"
        assert s in rlib.SIGNATURES, f"lib.SIGNATURES has no {s}"
    assert len(rlib.SIGNATURES["rnnt_transducer_nll"][1]) == 11 and len(rlib.SIGNATURES["rnnt_ctc_nll"][1]) == 10
    assert lib.rnnt_abi_version() == 3                          # additive change


def test_scoring_refuses_a_null_context():
    lib = rlib.load()
    nll = np.zeros(1, np.float64)
    assert lib.rnnt_transducer_nll(None, None, None, None, None, 1, 1, 0, nll.ctypes.data, None, None) == rlib.ERR_ARG
    assert lib.rnnt_ctc_nll(None, None, None, None, None, 1, 1, 0, nll.ctypes.data, None) == rlib.ERR_ARG


@pytest.mark.parametrize("shape", [(1, 0), (1, 2), (3, 2), (4, 3), (5, 0)])
def test_dp_equals_sum_over_alignments(shape):
    Tn, U = shape
    g = np.random.Generator(np.random.Philox(key=[17, 100 * Tn + U]))
    for trial in range(4):
        # random log-probabilities with the spread of a real lattice; two padded frames / labels around the valid cells, set to
        # NaN: neither function may read them
        pick = np.full((Tn + 2, U + 3, 2), np.nan)
        pick[:Tn, :U + 1] = -np.abs(g.standard_normal((Tn, U + 1, 2))) * (1.0 + 4.0 * trial)
        pick[:Tn, U, 1] = np.nan                                # the label slot at u = U_b is not a valid cell
        dp = T.transducer_nll_ref(pick, Tn, U)
        bf = T.transducer_nll_bruteforce(pick, Tn, U)
        assert math.isfinite(dp) and math.isfinite(bf)
        assert abs(dp - bf) <= 1e-12 * abs(bf), (shape, trial, dp, bf)


def test_dp_single_path_is_the_plain_sum():
    pick = np.log(np.array([[[0.5, 0.0]], [[0.25, 0.0]], [[0.125, 0.0]]]) + 1e-300)   # T = 3, U = 0: one alignment, three blanks
    assert T.transducer_nll_ref(pick, 3, 0) == pytest.approx(-math.log(0.5 * 0.25 * 0.125), rel=1e-15)


def test_loss_composition():
    from ctc_vr_amd.online_rnnt_model import compose_losses
    nll_r = np.array([3.0, 5.0, 10.0, 2.0])
    nll_c = np.array([8.0, math.inf, 6.0, 1.5])
    lens = np.array([4, 2, 3, 0])
    w = 0.3
    total, d = compose_losses(nll_r, nll_c, lens, w)
    loss_rnnt = (3.0 + 5.0 + 10.0 + 2.0) / 4                     # reduction="mean" over the batch
    loss_ctc = (8.0 / 4 + 0.0 + 6.0 / 3 + 1.5 / 1) / 4          # per-utterance / max(L, 1), the infinite term zeroed, batch mean
    assert set(d) == {"loss_rnnt", "loss_ctc"}
    assert d["loss_rnnt"] == loss_rnnt and d["loss_ctc"] == loss_ctc
    assert total == (1.0 - w) * loss_rnnt + w * loss_ctc
    # no CTC term (ctc_weight = 0 or no head): one key, total = (1 - w) * loss_rnnt
    total0, d0 = compose_losses(nll_r, None, lens, 0.0)
    assert set(d0) == {"loss_rnnt"} and total0 == loss_rnnt
    total1, d1 = compose_losses(nll_r, None, lens, w)
    assert set(d1) == {"loss_rnnt"} and total1 == (1.0 - w) * loss_rnnt
    # the composition agrees with torch's own CTCLoss reduction on the same per-utterance values
    import torch
    lp = torch.randn(6, 2, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).log_softmax(2)
    tg = torch.tensor([[1, 2, 0], [3, 3, 3]])
    il, tl = torch.tensor([6, 4]), torch.tensor([2, 3])         # row 1: three repeats need 5 frames, has 4 -> infinite
    per = torch.nn.functional.ctc_loss(lp, tg, il, tl, blank=4, reduction="none")
    want = torch.nn.functional.ctc_loss(lp, tg, il, tl, blank=4, reduction="mean", zero_infinity=True)
    assert torch.isinf(per[1])
    _, dd = compose_losses(np.zeros(2), per.numpy(), tl.numpy(), 0.5)
    assert dd["loss_ctc"] == pytest.approx(float(want), rel=1e-15)
