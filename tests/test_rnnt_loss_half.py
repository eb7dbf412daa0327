"""The transducer loss over bfloat16 and float16 lattices on the device (rnnt_transducer_loss_elem, ctc_vr_amd.functional.rnnt_loss
on 16-bit CUDA tensors).  Needs a real MI355X: `pytest -m gpu`.

Yardstick and factor are those of test_rnnt_loss.py.  Per dtype E the inputs are float32 values rounded to E and widened back, so
the float64 reference (ctc_vr_amd.testing.transducer_loss_ref) and the CPU emulation of the arithmetic contract
(transducer_loss_f32_emulation) see exactly the values the device widens.  E_nll and E_grad are the emulation's largest errors over
this file's cases, measured at run time; the device is held to 8 x E, and its gradient to 8 E_grad plus the ONE rounding to E the
contract allows: |got - want| <= 8 E_grad + 1/2 ulp_E(|want| + 8 E_grad), ulp_E(x) = 2^(floor(log2 x) - m), m = 7 (bfloat16) or 10
(float16, x floored at 2^-14).  A truncating store violates that bound on about 0.5 % of the elements; rounding to nearest does not."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import rnnt_loss
from ctc_vr_amd.lib import RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
SCALES = [1.0, 30.0]              # 30: logits of +-100, the max-subtraction has to hold
DTYPES = {"bf16": (torch.bfloat16, rlib.LOSS_BF16, 7), "f16": (torch.float16, rlib.LOSS_F16, 10)}   # torch dtype, element code, mantissa bits
# name: (T, Umax, V, blank, [(T_b, U_b)])
SHAPES = {
    "v2": (4, 2, 2, 1, [(4, 2), (3, 0)]),                        # a row shorter than any head
    "v7": (5, 3, 7, 6, [(5, 3), (4, 0), (2, 2)]),                # all eight phases, no body
    "v8": (5, 3, 8, 0, [(5, 3), (4, 0), (2, 2)]),                # exactly one vector per row
    "v9": (5, 3, 9, 0, [(5, 3), (2, 2)]),                        # head plus tail, no body at most phases
    "v15": (5, 3, 15, 3, [(5, 3), (2, 2)]),                      # head 7 + tail up to 7
    "v413": (5, 3, 413, 5, [(5, 3), (4, 0), (2, 2)]),            # all phases with a body of several vectors per lane
    "v4336": (5, 3, 4336, 4335, [(5, 3), (2, 2)]),               # more than one batch per lane
    "ragged": (9, 6, 412, 5, [(1, 0), (1, 6), (9, 0), (9, 6), (7, 4)]),   # one frame, no labels, the final-blank-only cell
    "umax255": (3, 255, 8, 0, [(3, 255), (2, 0)]),               # every thread of the wavefront live
}
CASES = [(d, n, s) for d in DTYPES for n in SHAPES for s in SCALES]


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _ulp(x, m):
    """ulp_E of |x| for an element type with m mantissa bits (float16: no finer than its subnormal spacing 2^-24)"""
    x = np.maximum(np.abs(x), 2.0 ** -14 if m == 10 else 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - m)


def _grad_bound(want, e_grad, m):
    return FACTOR * e_grad + 0.5 * _ulp(np.abs(want) + FACTOR * e_grad, m)


_INPUTS = {}


def _inputs(dt, name, scale):
    """(x of dtype E [B, T, U1, V] with NaN in all the padding, targets, T_b, U_b): float32 draws rounded to E.  Built once.
    The stream constant is not arbitrary in one respect: at V = 2 and scale 30 every step of a path has probability ~0 or ~1, and one
    draw in eight makes the only path of the (3, 0) row certain (nll = 2.5e-3, as 0x1600 did), where a RELATIVE nll error measures
    nothing: the emulation itself is then 2.2e-5 off and the yardstick's E_nll < 1e-5 fails before the device is asked anything."""
    key = (dt, name, scale)
    if key not in _INPUTS:
        Tn, Umax, V, blank, rows = SHAPES[name]
        g = np.random.Generator(np.random.Philox(key=[sorted(SHAPES).index(name), 0x1700 + int(scale)]))
        x = np.full((len(rows), Tn, Umax + 1, V), np.nan, np.float32)
        y = np.full((len(rows), Umax), -1, np.int32)
        for b, (Tb, Ub) in enumerate(rows):
            x[b, :Tb, :Ub + 1] = (scale * g.standard_normal((Tb, Ub + 1, V))).astype(np.float32)
            lab = g.integers(0, V - 1, Ub)
            y[b, :Ub] = np.where(lab >= blank, lab + 1, lab)
        _INPUTS[key] = (torch.from_numpy(x).to(DTYPES[dt][0]), y, np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32))
    return _INPUTS[key]


def _pad(x, Tb, Ub):
    pad = np.ones(tuple(x.shape[:3]), bool)
    for b in range(len(Tb)):
        pad[b, :Tb[b], :Ub[b] + 1] = False
    return pad


@pytest.fixture(scope="module")
def yardstick():
    """Per case the float64 reference (nll [B], grad [B, T, U1, V]) on the widened inputs and, per dtype over its cases, E_nll and
    E_grad of the emulation.  Computed once on the CPU, shared, never written to."""
    refs, e_nll, e_grad = {}, {d: 0.0 for d in DTYPES}, {d: 0.0 for d in DTYPES}
    for dt, name, scale in CASES:
        x16, y, Tb, Ub = _inputs(dt, name, scale)
        x = x16.float().numpy()
        blank = SHAPES[name][3]
        nll, grad = np.zeros(len(Tb)), np.zeros(x.shape)
        for b in range(len(Tb)):
            nll[b], grad[b] = T.transducer_loss_ref(x[b], y[b], int(Tb[b]), int(Ub[b]), blank)
            en, eg = T.transducer_loss_f32_emulation(x[b], y[b], int(Tb[b]), int(Ub[b]), blank)
            e_nll[dt] = max(e_nll[dt], abs(en - nll[b]) / abs(nll[b]))
            e_grad[dt] = max(e_grad[dt], float(np.abs(eg - grad[b]).max()))
        nll.setflags(write=False)
        grad.setflags(write=False)
        refs[(dt, name, scale)] = (nll, grad)
    for dt in DTYPES:
        print(f"{dt}: emulation vs float64: E_nll = {e_nll[dt]:.3e} (relative), E_grad = {e_grad[dt]:.3e} (absolute)")
        assert 0.0 < e_nll[dt] < 1e-5 and 0.0 < e_grad[dt] < 1e-3
    return refs, e_nll, e_grad


def _device(x_d, y, Tb, Ub, blank, elem, want_grad=True, fused=True, clamp=-1.0):
    """one rnnt_transducer_loss_elem call through the C ABI: (nll [B], nll from alpha [B], grad as a CPU tensor of E or None)"""
    B, Tn, U1, V = x_d.shape
    nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full_like(x_d, float("nan")) if want_grad else None
    rlib.transducer_loss_device(x_d.data_ptr(), tuple(x_d.shape), y, Tb, Ub, blank, fused, clamp, nll.data_ptr(), grad.data_ptr() if want_grad else None,
                                work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream, elem=elem)
    torch.cuda.synchronize()
    return nll.cpu().numpy(), work[:8 * B].cpu().numpy().view(np.float64), (grad.cpu() if want_grad else None)


@pytest.mark.parametrize("dt,name,scale", CASES)
def test_loss_and_gradient_vs_float64(dt, name, scale, yardstick):
    refs, e_nll, e_grad = yardstick
    want_nll, want_grad = refs[(dt, name, scale)]
    x16, y, Tb, Ub = _inputs(dt, name, scale)
    dtype, elem, m = DTYPES[dt]
    blank = SHAPES[name][3]
    x_d = x16.cuda()
    nll, nll_alpha, grad = _device(x_d, y, Tb, Ub, blank, elem)
    assert grad.dtype == dtype
    got = grad.float().numpy().astype(np.float64)
    r_nll = float((np.abs(nll - want_nll) / np.abs(want_nll)).max())
    excess = np.abs(got - want_grad) - _grad_bound(want_grad, e_grad[dt], m)
    print(f"{dt} {name} x{scale:g}: nll error {r_nll:.3e} = {r_nll / e_nll[dt]:.2f} E_nll, grad error {np.abs(got - want_grad).max():.3e}, "
          f"elements over the bound {int((excess > 0).sum())} of {excess.size}, alpha vs beta {float((np.abs(nll - nll_alpha) / np.abs(nll)).max()):.3e}")
    assert np.isfinite(nll).all() and np.isfinite(got).all()
    assert r_nll <= FACTOR * e_nll[dt]
    assert (excess <= 0).all()
    pad = _pad(x16, Tb, Ub)
    assert pad.any() and not _bits16(grad)[pad].any(), "a padding cell's gradient is not bitwise 0"
    assert (np.abs(nll - nll_alpha) <= 1e-9 * np.abs(nll)).all(), "-beta[0,0] and -(alpha[T_b-1,U_b] + pick_blank) disagree"
    nll2, nll_alpha2, grad2 = _device(x_d, y, Tb, Ub, blank, elem)
    assert np.array_equal(_bits64(nll), _bits64(nll2)) and np.array_equal(_bits64(nll_alpha), _bits64(nll_alpha2))
    assert np.array_equal(_bits16(grad), _bits16(grad2))
    nll3, _, _ = _device(x_d, y, Tb, Ub, blank, elem, want_grad=False)
    assert np.array_equal(_bits64(nll), _bits64(nll3)), "value-only nll differs"


def test_float32_through_the_new_entry_is_the_old_entry_bit_for_bit():
    x16, y, Tb, Ub = _inputs("bf16", "v413", 1.0)
    x_d = (4.0 * x16.float()).cuda()                               # the v413 x 4 case as a float32 lattice
    B, Tn, U1, V = x_d.shape
    nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
    out = []
    for elem in (None, rlib.LOSS_F32):
        work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        nll = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
        grad = torch.full_like(x_d, float("nan"))
        rlib.transducer_loss_device(x_d.data_ptr(), tuple(x_d.shape), y, Tb, Ub, 5, True, -1.0, nll.data_ptr(), grad.data_ptr(), work.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream, elem=elem)
        torch.cuda.synchronize()
        out.append((nll.cpu().numpy(), grad.cpu().numpy()))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][1]).all()
    assert np.array_equal(_bits64(out[0][0]), _bits64(out[1][0]))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_log_probabilities_and_clamp_on_the_device(dt, yardstick):
    """the two switches of the entry point against the host twin (f64) on the widened values"""
    _, _, e_grad = yardstick
    dtype, elem, m = DTYPES[dt]
    x16, y, Tb, Ub = _inputs(dt, "v413", 1.0)
    x = x16.float()
    lp16 = torch.where(torch.isnan(x), x, torch.log_softmax(x.double(), -1).float()).to(dtype)   # 16-bit log-probabilities, NaN padding kept
    lp = lp16.float().numpy()
    want_nll, want_grad = rlib.transducer_loss_host(lp, y, Tb, Ub, 5, fused_log_softmax=False)
    nll, _, grad = _device(lp16.cuda(), y, Tb, Ub, 5, elem, fused=False)
    assert (np.abs(nll - want_nll) <= 1e-9 * np.abs(want_nll)).all()      # no lse: the picks are the inputs, the recursion is f64
    got = grad.float().numpy().astype(np.float64)
    assert (np.abs(got - want_grad) <= _grad_bound(want_grad, e_grad[dt], m)).all()
    _, want_c = rlib.transducer_loss_host(x.numpy(), y, Tb, Ub, 5, clamp=0.05)
    _, _, grad_c = _device(x16.cuda(), y, Tb, Ub, 5, elem, clamp=0.05)
    got_c = grad_c.float().numpy().astype(np.float64)
    assert np.abs(want_c).max() == np.float32(0.05), "the case does not exercise the clamp"
    assert np.abs(got_c).max() == float(torch.tensor(0.05).to(dtype))     # the float32 clamp, rounded to E
    assert (np.abs(got_c - want_c) <= _grad_bound(want_c, e_grad[dt], m)).all()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_rnnt_loss_backward_on_16_bit_cuda_tensors(dt, yardstick):
    """rnnt_loss(reduction="mean") with B = 5 on the device against the float64 gradient / B.  logits.grad has had TWO roundings to
    E: the kernel's store of g, and the backward's store of the float32 product g16 * (1 / B).  Their exact bound is
    (8 E_grad + 1/2 ulp_E(g)) / B + 1/2 ulp_E(g / B), which is what is asserted.  It is within "8 E_grad / B + 1 ulp_E" when the ulp
    is that of the saved gradient g (asserted too), and NOT when it is that of g / B: with g just above a power of two, g / 5 lies
    three binades lower, ulp_E(g) / 5 = 1.6 ulp_E(g / 5), and the two roundings add up to 0.8 + 0.5 = 1.3 ulp_E(g / 5).  Any path
    that keeps the saved gradient in 16 bits reaches that, the CPU path included; the count of such elements is printed."""
    refs, e_nll, e_grad = yardstick
    dtype, _, m = DTYPES[dt]
    x16, y, Tb, Ub = _inputs(dt, "ragged", 1.0)
    _, want_grad = refs[(dt, "ragged", 1.0)]
    B = len(Tb)
    assert B == 5                                                  # "mean": a scale that is no power of two
    args = (torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Ub))
    xc = x16.clone().requires_grad_(True)
    loss_c = rnnt_loss(xc, *args, blank=5, reduction="mean")
    xg = x16.cuda().requires_grad_(True)
    loss_g = rnnt_loss(xg, *(a.cuda() for a in args), blank=5, reduction="mean")
    loss_g.backward()
    assert loss_g.is_cuda and loss_g.dtype == torch.float32 and loss_c.dtype == torch.float32
    assert xg.grad.is_cuda and xg.grad.dtype == dtype
    lg, lc = float(loss_g.detach()), float(loss_c.detach())
    assert abs(lg - lc) <= (FACTOR * e_nll[dt] + 2.0 ** -22) * abs(lc)        # (float32 results: two roundings)
    got = xg.grad.float().cpu().numpy().astype(np.float64)
    want = want_grad / B
    first = _grad_bound(want_grad, e_grad[dt], m) / B              # the saved gradient: 8 E_grad + its one rounding, then scaled
    bound = first + 0.5 * _ulp(np.abs(want) + first, m)           # the product's one rounding
    err = np.abs(got - want)
    one_ulp_scaled = FACTOR * e_grad[dt] / B + _ulp(np.abs(want) + FACTOR * e_grad[dt] / B, m)
    print(f"{dt}: max error / bound {float((err / bound).max()):.3f}; elements beyond 8 E_grad / B + 1 ulp_E taken at |gradient / B|: "
          f"{int((err > one_ulp_scaled).sum())} of {err.size}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert (bound <= FACTOR * e_grad[dt] / B + _ulp(np.abs(want_grad) + FACTOR * e_grad[dt], m)).all()   # within 1 ulp_E of the saved gradient
    assert not _bits16(xg.grad)[_pad(x16, Tb, Ub)].any()


def test_a_refusal_launches_nothing():
    x16, y, Tb, Ub = _inputs("bf16", "v8", 1.0)
    x_d = x16.cuda()
    B, Tn, U1, V = x_d.shape
    nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    flat = torch.full((x_d.numel() + 8,), 7.0, dtype=torch.bfloat16, device="cuda")
    grad = flat[:x_d.numel()]
    assert grad.data_ptr() % 16 == 0
    y_blank = y.copy()
    y_blank[0, 1] = 0                                              # the blank inside row 0's length
    s = torch.cuda.current_stream().cuda_stream

    def call(tg=y, grad_ptr=grad.data_ptr(), bytes_=nbytes, elem=rlib.LOSS_BF16):
        with pytest.raises(RnntError) as e:
            rlib.transducer_loss_device(x_d.data_ptr(), tuple(x_d.shape), tg, Tb, Ub, 0, True, -1.0, nll.data_ptr(), grad_ptr, work.data_ptr(), bytes_, s,
                                        elem=elem)
        return e.value.status

    assert call(grad_ptr=flat[1:].data_ptr()) == rlib.ERR_ARG       # 2 bytes past a 16-byte boundary
    assert call(tg=y_blank) == rlib.ERR_ARG
    assert call(bytes_=nbytes - 1) == rlib.ERR_SHAPE
    assert call(elem=3) == rlib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((nll == 7.0).all()) and bool((flat == 7.0).all()) and not bool(work.any())
