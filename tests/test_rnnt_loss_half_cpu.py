"""rnnt_loss on bfloat16 and float16 lattices, without a GPU: CPU tensors widen exactly to float32, run the host twin
(rnnt_transducer_loss_host, f64) and round its gradient f64 -> float32 -> E.  Everything here is bitwise: the only arithmetic of
the 16-bit path on the CPU is those two roundings and, in the backward, one rounding of a float32 product.  The returned loss is
float32 whatever the logits' dtype.  Also: the dtypes that stay refused, and the element code of rnnt_transducer_loss_elem, which
is refused before any pointer is followed (so without a GPU)."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
from ctc_vr_amd.functional import rnnt_loss

DTYPES = [torch.bfloat16, torch.float16]
V, BLANK = 412, 5
ROWS = [(3, 7, 4), (4, 33, 12)]   # (index in test_rnnt_loss_cpu.CASES, T_b, U_b): its two V = 412 rows, same seeds, same values


def _bits(t):
    return t.contiguous().view(torch.int16)


_PACK = {}


def _pack(dtype):
    """The V = 412 ragged batch of test_rnnt_loss_cpu.py (one frame and one label longer than its longest row, NaN in every padding
    cell, -1 in the target padding), rounded to dtype; with the host twin's (nll, grad) on the widened values.  Built once, shared."""
    if dtype not in _PACK:
        Tn, Umax = max(r[1] for r in ROWS) + 1, max(r[2] for r in ROWS) + 1
        x = np.full((len(ROWS), Tn, Umax + 1, V), np.nan, np.float32)
        y = np.full((len(ROWS), Umax), -1, np.int32)
        for b, (i, Tb, Ub) in enumerate(ROWS):
            g = np.random.Generator(np.random.Philox(key=[i, 0x105]))
            x[b, :Tb, :Ub + 1] = (3.0 * g.standard_normal((Tb, Ub + 1, V))).astype(np.float32)
            lab = g.integers(0, V - 1, Ub)
            y[b, :Ub] = np.where(lab >= BLANK, lab + 1, lab)
        x16 = torch.from_numpy(x).to(dtype)
        Tb, Ub = np.array([r[1] for r in ROWS], np.int32), np.array([r[2] for r in ROWS], np.int32)
        nll, grad = rlib.transducer_loss_host(x16.float().numpy(), y, Tb, Ub, BLANK)
        pad = torch.from_numpy(np.isnan(x).all(-1))
        assert bool(pad.any()) and bool(torch.isnan(x16[pad]).all())
        _PACK[dtype] = (x16, torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Ub), nll, grad, pad)
    return _PACK[dtype]


def _backward(dtype, loss_fn):
    x16, y, Tb, Ub = _pack(dtype)[:4]
    x = x16.clone().requires_grad_(True)
    loss = loss_fn(x, y, Tb, Ub)
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("dtype", DTYPES)
def test_loss_is_float32_and_the_host_twins_on_the_widened_logits(dtype):
    x16, y, Tb, Ub, nll, _, _ = _pack(dtype)
    none = rnnt_loss(x16, y, Tb, Ub, blank=BLANK, reduction="none")
    assert none.dtype == torch.float32 and none.shape == (len(ROWS),)
    assert torch.equal(none, torch.from_numpy(nll).float())
    assert rnnt_loss(x16, y, Tb, Ub, blank=BLANK).dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_is_the_host_twins_rounded_f32_then_e(dtype):
    _, _, _, _, _, grad, pad = _pack(dtype)
    want = torch.from_numpy(grad.astype(np.float32)).to(dtype)
    _, got = _backward(dtype, lambda *a: rnnt_loss(*a, blank=BLANK, reduction="sum"))
    assert got.dtype == dtype
    assert torch.equal(_bits(got), _bits(want))
    assert not bool(_bits(got)[pad].any()), "a padding cell's gradient is not bitwise 0"


@pytest.mark.parametrize("dtype", DTYPES)
def test_upstream_gradient_is_one_rounding_of_a_float32_product(dtype):
    _, _, _, _, _, grad, pad = _pack(dtype)
    g16 = torch.from_numpy(grad.astype(np.float32)).to(dtype)
    s = torch.tensor([1.0 / 3.0, 3.0])
    want = (g16.float() * s.view(-1, 1, 1, 1)).to(dtype)
    _, got = _backward(dtype, lambda *a: (rnnt_loss(*a, blank=BLANK, reduction="none") * s).sum())
    assert got.dtype == dtype and torch.equal(_bits(got), _bits(want))
    rounded_scale = g16 * s.to(dtype).view(-1, 1, 1, 1)              # what rounding 1/3 to 16 bits first would give
    assert not torch.equal(_bits(rounded_scale), _bits(want)), "the case does not tell a rounded scale from a float32 one"
    assert not bool(_bits(got)[pad].any())


def test_other_dtypes_stay_refused():
    x16, y, Tb, Ub = _pack(torch.float16)[:4]
    x = torch.nan_to_num(x16.float())
    for bad in (x.double(), x.to(torch.int32)):
        with pytest.raises(TypeError):
            rnnt_loss(bad, y, Tb, Ub, blank=BLANK)


def test_unknown_element_code_is_refused_before_anything_is_touched():
    """elem = 3 with device pointers that point nowhere (non-null, 16-byte aligned integers): ERR_ARG, and the host arrays untouched."""
    fn = rlib.load().rnnt_transducer_loss_elem
    tg, ll, tl = np.array([[1, 2]], np.int32), np.array([3], np.int32), np.array([2], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for elem in (3, -1, 1 << 20):
        rc = fn(0x1000, p(tg), p(ll), p(tl), 1, 3, 2, 8, 0, elem, 1, -1.0, 0x2000, 0x3000, 0x4000, 1 << 20, None)
        assert rc == rlib.ERR_ARG, (elem, rc)
    assert (rlib.LOSS_F32, rlib.LOSS_BF16, rlib.LOSS_F16) == (0, 1, 2)
    assert tg.tolist() == [[1, 2]] and ll.tolist() == [3] and tl.tolist() == [2]
