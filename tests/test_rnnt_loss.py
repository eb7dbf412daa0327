"""The transducer loss with gradients on the device (rnnt_transducer_loss, ctc_vr_amd.functional.rnnt_loss on CUDA tensors).
Needs a real MI355X: `pytest -m gpu`.

The yardstick is ctc_vr_amd.testing.transducer_loss_ref (float64 autograd).  The device owes float32 lse and picks followed by
float64 recursions, which is what transducer_loss_f32_emulation does on the CPU.  So the bound is measured, not chosen: E_nll is
the emulation's largest relative nll error against the float64 reference over the cases of this file, E_grad its largest absolute
gradient error, and the device is held to 8 x E: the factor covers another summation tree over V and device exp / log within a
couple of ulps."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import rnnt_loss
from ctc_vr_amd.lib import RnntEngine, RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
SCALES = [1.0, 4.0, 30.0]         # 30: logits of +-100, the max-subtraction has to hold
# name: (T, Umax, V, blank, [(T_b, U_b)])
SHAPES = {
    "ragged": (33, 12, 412, 5, [(1, 0), (1, 12), (33, 0), (33, 12), (7, 4)]),   # one frame, no labels, the cell where only the final blank exists
    "v7": (5, 3, 7, 6, [(5, 3), (4, 0), (2, 2)]),                # rows start at every phase of 16 bytes
    "v8": (5, 3, 8, 0, [(5, 3), (4, 0), (2, 2)]),
    "v413": (5, 3, 413, 5, [(5, 3), (4, 0), (2, 2)]),            # rows not 16-byte aligned, more than one float4 per lane
    "v4336": (5, 3, 4336, 4335, [(5, 3), (4, 0), (2, 2)]),       # several strides per row
    "umax255": (3, 255, 8, 0, [(3, 255), (2, 0)]),               # every thread of the wavefront is live
}
CASES = [(n, s) for n in SHAPES for s in SCALES]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _inputs(name, scale):
    Tn, Umax, V, blank, rows = SHAPES[name]
    g = np.random.Generator(np.random.Philox(key=[sorted(SHAPES).index(name), int(scale)]))
    B = len(rows)
    x = np.full((B, Tn, Umax + 1, V), np.nan, np.float32)          # NaN in all the padding
    y = np.full((B, Umax), -1, np.int32)
    for b, (Tb, Ub) in enumerate(rows):
        x[b, :Tb, :Ub + 1] = (scale * g.standard_normal((Tb, Ub + 1, V))).astype(np.float32)
        lab = g.integers(0, V - 1, Ub)
        y[b, :Ub] = np.where(lab >= blank, lab + 1, lab)
    return x, y, np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32)


@pytest.fixture(scope="module")
def yardstick():
    """Per case the float64 reference (nll [B], grad [B, T, U1, V]) and, over all cases, E_nll and E_grad of the emulation.
    Computed once on the CPU, shared, never written to."""
    refs, e_nll, e_grad = {}, 0.0, 0.0
    for name, scale in CASES:
        x, y, Tb, Ub = _inputs(name, scale)
        blank = SHAPES[name][3]
        nll, grad = np.zeros(len(Tb)), np.zeros(x.shape)
        for b in range(len(Tb)):
            nll[b], grad[b] = T.transducer_loss_ref(x[b], y[b], int(Tb[b]), int(Ub[b]), blank)
            en, eg = T.transducer_loss_f32_emulation(x[b], y[b], int(Tb[b]), int(Ub[b]), blank)
            e_nll = max(e_nll, abs(en - nll[b]) / abs(nll[b]))
            e_grad = max(e_grad, float(np.abs(eg - grad[b]).max()))
        nll.setflags(write=False)
        grad.setflags(write=False)
        refs[(name, scale)] = (nll, grad)
    print(f"emulation vs float64: E_nll = {e_nll:.3e} (relative), E_grad = {e_grad:.3e} (absolute)")
    assert 0.0 < e_nll < 1e-5 and 0.0 < e_grad < 1e-3            # float32 picks cost something, and not more than float32 can
    return refs, e_nll, e_grad


def _device(x_d, y, Tb, Ub, blank, want_grad=True, fused=True, clamp=-1.0, fill=float("nan")):
    """one rnnt_transducer_loss call through the C ABI: (nll [B], nll from alpha [B], grad or None), as numpy"""
    B, Tn, U1, V = x_d.shape
    nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), fill, dtype=torch.float64, device="cuda")
    grad = torch.full_like(x_d, fill) if want_grad else None
    rlib.transducer_loss_device(x_d.data_ptr(), tuple(x_d.shape), y, Tb, Ub, blank, fused, clamp, nll.data_ptr(), grad.data_ptr() if want_grad else None,
                                work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nll.cpu().numpy(), work[:8 * B].cpu().numpy().view(np.float64), (grad.cpu().numpy() if want_grad else None)


@pytest.mark.parametrize("name,scale", CASES)
def test_loss_and_gradient_vs_float64(name, scale, yardstick):
    refs, e_nll, e_grad = yardstick
    want_nll, want_grad = refs[(name, scale)]
    x, y, Tb, Ub = _inputs(name, scale)
    blank = SHAPES[name][3]
    x_d = torch.from_numpy(x).cuda()
    nll, nll_alpha, grad = _device(x_d, y, Tb, Ub, blank)
    r_nll = float((np.abs(nll - want_nll) / np.abs(want_nll)).max())
    r_grad = float(np.abs(grad - want_grad).max())
    print(f"{name} x{scale:g}: nll error {r_nll:.3e} = {r_nll / e_nll:.2f} E_nll, grad error {r_grad:.3e} = {r_grad / e_grad:.2f} E_grad, "
          f"alpha vs beta {float((np.abs(nll - nll_alpha) / np.abs(nll)).max()):.3e}")
    assert np.isfinite(nll).all() and np.isfinite(grad).all()
    assert r_nll <= FACTOR * e_nll
    assert r_grad <= FACTOR * e_grad
    pad = np.ones(x.shape[:3], bool)
    for b in range(len(Tb)):
        pad[b, :Tb[b], :Ub[b] + 1] = False
    assert pad.any() and not _bits(grad)[pad].any(), "a padding cell's gradient is not bitwise 0"
    assert (np.abs(nll - nll_alpha) <= 1e-9 * np.abs(nll)).all(), "-beta[0,0] and -(alpha[T_b-1,U_b] + pick_blank) disagree"
    nll2, nll_alpha2, grad2 = _device(x_d, y, Tb, Ub, blank)
    assert np.array_equal(_bits(nll), _bits(nll2)) and np.array_equal(_bits(nll_alpha), _bits(nll_alpha2)) and np.array_equal(_bits(grad), _bits(grad2))
    nll3, _, _ = _device(x_d, y, Tb, Ub, blank, want_grad=False)
    assert np.array_equal(_bits(nll), _bits(nll3)), "value-only nll differs"


def test_log_probabilities_and_clamp_on_the_device(yardstick):
    """the two switches of the entry point against the host twin (f64), within the same bound"""
    _, _, e_grad = yardstick
    x, y, Tb, Ub = _inputs("v413", 4.0)
    lp = np.where(np.isnan(x), np.nan, torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy())
    want_nll, want_grad = rlib.transducer_loss_host(lp, y, Tb, Ub, 5, fused_log_softmax=False)
    nll, _, grad = _device(torch.from_numpy(lp).cuda(), y, Tb, Ub, 5, fused=False)
    assert (np.abs(nll - want_nll) <= 1e-9 * np.abs(want_nll)).all()      # no lse: the picks are the inputs, the recursion is f64
    assert np.abs(grad - want_grad).max() <= FACTOR * e_grad
    _, want_c = rlib.transducer_loss_host(x, y, Tb, Ub, 5, clamp=0.05)
    _, _, grad_c = _device(torch.from_numpy(x).cuda(), y, Tb, Ub, 5, clamp=0.05)
    assert np.abs(grad_c).max() == np.float32(0.05) and np.abs(grad_c - want_c).max() <= FACTOR * e_grad


def test_agrees_with_rnnt_transducer_nll_over_a_joint_lattice(yardstick, np_state_dict):
    """logits = rnnt_joint(mode 0) of a small fp32-mode engine; rnnt_transducer_nll scores the same frames and transcript itself."""
    _, e_nll, _ = yardstick
    V, BLANK = T.VOCAB, T.BLANK
    B, Tn, Umax = 3, 21, 6
    eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=V, blank_id=BLANK, max_beam=0)
    try:
        eng.load_state_dict(np_state_dict(0), numerics="fp32")
        s = torch.cuda.current_stream().cuda_stream
        Tb, Ub = np.array([21, 13, 8], np.int32), np.array([6, 3, 5], np.int32)
        g = np.random.Generator(np.random.Philox(key=[31, 7]))
        lab = g.integers(0, V - 1, (B, Umax))
        y = np.where(lab >= BLANK, lab + 1, lab).astype(np.int32)
        enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(31)).cuda()
        h, c = torch.zeros(B, 256, device="cuda"), torch.zeros(B, 256, device="cuda")
        pred = torch.empty(B, Umax + 1, 256, device="cuda")
        for u in range(Umax + 1):                                  # the predictor over [blank, y_1 .. y_Umax] from the zero state
            tok = torch.tensor([int(y[b, u - 1]) if 1 <= u <= Ub[b] else BLANK for b in range(B)], dtype=torch.int32, device="cuda")
            out, h2, c2 = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
            eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), B, out.data_ptr(), h2.data_ptr(), c2.data_ptr(), s)
            pred[:, u] = out
            h, c = h2, c2
        lat = torch.empty(B, Tn, Umax + 1, V, device="cuda")
        eng.joint(enc_d.data_ptr(), pred.data_ptr(), B, Tn, Umax + 1, 0, lat.data_ptr(), s)
        want = eng.transducer_nll(enc_d.data_ptr(), Tb, y, Ub, B, Tn, None, s)
        nll, _, _ = _device(lat, y, Tb, Ub, BLANK, want_grad=False)
        print("loss over the joint lattice", nll, "rnnt_transducer_nll", want)
        assert np.isfinite(want).all() and (np.abs(nll - want) <= FACTOR * e_nll * np.abs(want)).all()
    finally:
        eng.close()


def test_rnnt_loss_backward_on_cuda_tensors(yardstick):
    _, _, e_grad = yardstick
    x, y, Tb, Ub = _inputs("ragged", 4.0)
    B = len(Tb)
    args = (torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Ub))
    xc = torch.from_numpy(x).requires_grad_(True)
    loss_c = rnnt_loss(xc, *args, blank=5, reduction="mean")
    loss_c.backward()
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    loss_g = rnnt_loss(xg, *(a.cuda() for a in args), blank=5, reduction="mean")
    loss_g.backward()
    assert loss_g.is_cuda and xg.grad.is_cuda and loss_g.dtype == torch.float32
    lg, lc = float(loss_g.detach()), float(loss_c.detach())
    assert abs(lg - lc) <= (FACTOR * yardstick[1] + 2.0 ** -22) * abs(lc)     # (float32 results: two roundings)
    assert float((xg.grad.cpu() - xc.grad).abs().max()) <= FACTOR * e_grad / B
    assert not _bits(xg.grad.cpu().numpy())[np.isnan(x)].any()


def test_a_refusal_launches_nothing():
    x, y, Tb, Ub = _inputs("v8", 1.0)
    y = y.copy()
    y[0, 1] = 0                                                    # the blank inside row 0's length
    x_d = torch.from_numpy(x).cuda()
    B, Tn, U1, V = x.shape
    nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    grad = torch.full_like(x_d, 7.0)
    with pytest.raises(RnntError) as e:
        rlib.transducer_loss_device(x_d.data_ptr(), x.shape, y, Tb, Ub, 0, True, -1.0, nll.data_ptr(), grad.data_ptr(), work.data_ptr(), nbytes,
                                    torch.cuda.current_stream().cuda_stream)
    assert e.value.status == rlib.ERR_ARG
    with pytest.raises(RnntError) as e:                            # a workspace one byte short
        rlib.transducer_loss_device(x_d.data_ptr(), x.shape, _inputs("v8", 1.0)[1], Tb, Ub, 0, True, -1.0, nll.data_ptr(), grad.data_ptr(), work.data_ptr(),
                                    nbytes - 1, torch.cuda.current_stream().cuda_stream)
    assert e.value.status == rlib.ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((nll == 7.0).all()) and bool((grad == 7.0).all()) and not bool(work.any())
