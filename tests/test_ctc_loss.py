"""The CTC loss with gradients on the device (rnnt_ctc_loss, ctc_vr_amd.functional.ctc_loss and CTCHead on CUDA tensors).
Needs a real MI355X: `pytest -m gpu`.

The yardstick is ctc_vr_amd.testing.ctc_loss_ref (float64 autograd).  The device owes float32 lse and picks followed by float64
recursions, which is what ctc_loss_f32_emulation does on the CPU.  So the bound is measured, not chosen, as in test_rnnt_loss.py:
E_nll is the emulation's largest relative nll error against the float64 reference over the cases of this file (the infeasible row
aside), E_grad its largest absolute gradient error, and the device is held to 8 x E: the factor covers another summation tree over
V and device exp / log within a couple of ulps."""
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import CTCHead, ctc_loss
from ctc_vr_amd.lib import RnntEngine, RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
SCALES = [1.0, 4.0, 30.0]         # 30: logits of +-100, the max-subtraction has to hold
A, Bb, C = 3, 5, 6                # the labels a, b, c of the small shapes
ALT = [A if i % 2 == 0 else Bb for i in range(255)]
# name: (T, Lmax, V, blank, [(T_b, labels)]); labels None: L random labels, drawn with the inputs
SHAPES = {
    "ragged": (33, 12, 412, 5, [(1, 0), (1, 1), (33, 0), (33, 12), (7, 4)]),    # S = 1, one frame, the longest recursion
    "repeats": (9, 4, 8, 0, [(9, [A] * 4), (7, [A] * 4), (9, [A, Bb, A, Bb]), (8, [A, A, Bb, Bb])]),   # four states on a column; 7 = L + repeats: one path
    # the second row needs 5 frames (3 labels + 2 adjacent repeats; `aab` would need only 4): +inf and zeros; blank = V - 1
    "tight": (4, 3, 8, 7, [(3, [A, Bb, C]), (4, [A, A, A]), (4, [A, Bb, C])]),
    "v7": (5, 3, 7, 6, [(5, [1, 0, 1]), (4, []), (2, [2, 3])]),                  # rows start at every phase of 16 bytes
    "v413": (5, 3, 413, 5, [(5, [400, 400, 7]), (4, []), (2, [0, 412])]),        # more than one vector per lane, unaligned rows, the last column
    "v4336": (5, 3, 4336, 0, [(5, [4335, 17, 2000]), (4, []), (2, [1, 4000])]),  # several strides per row
    "l255": (256, 255, 8, 0, [(256, ALT), (2, [])]),                             # all 511 state threads live
}
CASES = [(n, s) for n in SHAPES for s in SCALES]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


def _inputs(name, scale):
    """x [B, T, V] float32 with NaN in every frame t >= T_b, targets [B, Lmax] with -1 beyond L_b, T_b [B], L_b [B]"""
    Tn, Lmax, V, blank, rows = SHAPES[name]
    g = np.random.Generator(np.random.Philox(key=[sorted(SHAPES).index(name), int(scale)]))
    B = len(rows)
    x = np.full((B, Tn, V), np.nan, np.float32)
    y = np.full((B, Lmax), -1, np.int32)
    Lb = np.zeros(B, np.int32)
    for b, (Tb, labels) in enumerate(rows):
        x[b, :Tb] = (scale * g.standard_normal((Tb, V))).astype(np.float32)
        if isinstance(labels, int):
            lab = g.integers(0, V - 1, labels)
            labels = np.where(lab >= blank, lab + 1, lab)
        Lb[b] = len(labels)
        y[b, :Lb[b]] = labels
    return x, y, np.array([r[0] for r in rows], np.int32), Lb


def _feasible(y, Tb, Lb):
    return np.array([Tb[b] >= Lb[b] + sum(y[b, i] == y[b, i - 1] for i in range(1, Lb[b])) for b in range(len(Tb))])


@pytest.fixture(scope="module")
def yardstick():
    """Per case the float64 reference (nll [B], grad [B, T, V]) and, over all cases, E_nll and E_grad of the emulation.  Computed once
    on the CPU, shared, never written to."""
    refs, e_nll, e_grad = {}, 0.0, 0.0
    for name, scale in CASES:
        x, y, Tb, Lb = _inputs(name, scale)
        blank = SHAPES[name][3]
        ok = _feasible(y, Tb, Lb)
        assert ok.tolist() == ([True, False, True] if name == "tight" else [True] * len(Tb)), name
        nll, grad = np.zeros(len(Tb)), np.zeros(x.shape)
        for b in range(len(Tb)):
            nll[b], grad[b] = T.ctc_loss_ref(x[b], y[b, :Lb[b]], int(Tb[b]), blank)
            en, eg = T.ctc_loss_f32_emulation(x[b], y[b, :Lb[b]], int(Tb[b]), blank)
            assert math.isfinite(nll[b]) == bool(ok[b]) and math.isfinite(en) == bool(ok[b])
            if ok[b]:
                e_nll = max(e_nll, abs(en - nll[b]) / abs(nll[b]))
            e_grad = max(e_grad, float(np.abs(eg - grad[b]).max()))
        nll.setflags(write=False)
        grad.setflags(write=False)
        refs[(name, scale)] = (nll, grad)
    print(f"emulation vs float64: E_nll = {e_nll:.3e} (relative), E_grad = {e_grad:.3e} (absolute)")
    assert 0.0 < e_nll < 1e-5 and 0.0 < e_grad < 1e-3            # float32 picks cost something, and not more than float32 can
    return refs, e_nll, e_grad


def _device(x_d, layout, y, Tb, Lb, blank, want_grad=True, fused=True, elem=None, fill=float("nan")):
    """one rnnt_ctc_loss call through the C ABI over the storage of x_d; layout = (stride_b, stride_t, T, V), None for a contiguous
    [B, T, V]: (nll [B], nll from beta [B], grad as a tensor shaped and laid out like x_d, or None)"""
    B = len(Tb)
    sb, st, Tn, V = (x_d.shape[1] * x_d.shape[2], x_d.shape[2], x_d.shape[1], x_d.shape[2]) if layout is None else layout
    strides = (sb, st)
    nbytes = rlib.ctc_loss_workspace(B, Tn, y.shape[1])
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), fill, dtype=torch.float64, device="cuda")
    grad = torch.full_like(x_d, fill) if want_grad else None
    rlib.ctc_loss_device(x_d.data_ptr(), (B, Tn, V), strides, y, Tb, Lb, blank, fused, nll.data_ptr(), grad.data_ptr() if want_grad else None,
                         work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream, elem=elem)
    torch.cuda.synchronize()
    return nll.cpu().numpy(), work[:8 * B].cpu().numpy().view(np.float64), grad


@pytest.mark.parametrize("name,scale", CASES)
def test_loss_and_gradient_vs_float64(name, scale, yardstick):
    refs, e_nll, e_grad = yardstick
    want_nll, want_grad = refs[(name, scale)]
    x, y, Tb, Lb = _inputs(name, scale)
    blank = SHAPES[name][3]
    ok = np.isfinite(want_nll)
    x_d = torch.from_numpy(x).cuda()
    nll, nll_beta, grad_d = _device(x_d, None, y, Tb, Lb, blank)
    grad = grad_d.cpu().numpy()
    r_nll = float((np.abs(nll[ok] - want_nll[ok]) / np.abs(want_nll[ok])).max())
    r_grad = float(np.abs(grad - want_grad).max())
    print(f"{name} x{scale:g}: nll error {r_nll:.3e} = {r_nll / e_nll:.2f} E_nll, grad error {r_grad:.3e} = {r_grad / e_grad:.2f} E_grad, "
          f"alpha vs beta {float((np.abs(nll[ok] - nll_beta[ok]) / np.abs(nll[ok])).max()):.3e}")
    assert np.array_equal(np.isfinite(nll), ok) and (nll[~ok] == math.inf).all() and (nll_beta[~ok] == math.inf).all()
    assert np.isfinite(grad).all()
    assert r_nll <= FACTOR * e_nll
    assert r_grad <= FACTOR * e_grad
    zero = np.isnan(x).any(-1) | ~ok[:, None]                      # padding frames and the infeasible row
    assert zero.any() and not _bits(grad)[zero].any(), "a padding frame's or an infeasible row's gradient is not bitwise 0"
    assert (np.abs(nll[ok] - nll_beta[ok]) <= 1e-9 * np.abs(nll[ok])).all(), "the alpha side and the beta side disagree"
    nll2, nll_beta2, grad2 = _device(x_d, None, y, Tb, Lb, blank)
    assert np.array_equal(_bits(nll), _bits(nll2)) and np.array_equal(_bits(nll_beta), _bits(nll_beta2)) and np.array_equal(_bits(grad), _bits(grad2.cpu().numpy()))
    nll3, _, _ = _device(x_d, None, y, Tb, Lb, blank, want_grad=False)
    assert np.array_equal(_bits(nll), _bits(nll3)), "value-only nll differs"


def test_layouts_agree_bit_for_bit(yardstick):
    """contiguous [B, T, V], contiguous [T, B, V], frames padded to an odd stride (rows at every alignment), and the transposed view
    through functional.ctc_loss: one reduction order, so one set of bits"""
    x, y, Tb, Lb = _inputs("ragged", 4.0)
    B, Tn, V = x.shape
    blank = SHAPES["ragged"][3]
    x_d = torch.from_numpy(x).cuda()
    nll, _, grad = _device(x_d, None, y, Tb, Lb, blank)
    grad = grad.cpu().numpy()
    x_tbv = x_d.transpose(0, 1).contiguous()
    nll_t, _, grad_t = _device(x_tbv, (V, B * V, Tn, V), y, Tb, Lb, blank)
    assert np.array_equal(_bits(nll), _bits(nll_t)) and np.array_equal(_bits(grad), _bits(grad_t.transpose(0, 1).cpu().numpy()))
    wide = torch.full((B, Tn, V + 3), float("nan"), device="cuda")
    wide[:, :, :V] = x_d
    nll_w, _, grad_w = _device(wide, (Tn * (V + 3), V + 3, Tn, V), y, Tb, Lb, blank)
    assert np.array_equal(_bits(nll), _bits(nll_w)) and np.array_equal(_bits(grad), _bits(grad_w[:, :, :V].cpu().numpy()))
    assert bool(torch.isnan(grad_w[:, :, V:]).all()), "elements between the frames were written"
    args = (torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Lb))
    for xt in (x_d.transpose(0, 1), x_tbv):                        # the view the reference passes, and the contiguous [T, B, V]
        xt = xt.detach().requires_grad_(True)
        loss = ctc_loss(xt, *args, blank=blank, reduction="none", fused_log_softmax=True)
        loss.sum().backward()
        assert loss.is_cuda and np.array_equal(loss.detach().cpu().numpy(), nll.astype(np.float32))
        assert np.array_equal(_bits(xt.grad.transpose(0, 1).cpu().numpy()), _bits(grad))


def test_inputs_the_kernels_cannot_address_are_copied():
    """a stride over V that is not 1, and a base 4 bytes past a 16-byte boundary: functional.ctc_loss copies, the result is the same"""
    x, y, Tb, Lb = _inputs("v7", 4.0)
    B, Tn, V = x.shape
    args = (torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Lb))
    kw = dict(blank=SHAPES["v7"][3], reduction="none", fused_log_softmax=True)
    x_tbv = torch.from_numpy(x).cuda().transpose(0, 1).contiguous()
    want = ctc_loss(x_tbv.clone().requires_grad_(True), *args, **kw)
    every_other = torch.zeros(Tn, B, 2 * V, device="cuda")
    every_other[..., ::2] = x_tbv
    flat = torch.zeros(Tn * B * V + 1, device="cuda")
    flat[1:] = x_tbv.reshape(-1)
    shifted = flat[1:].view(Tn, B, V)
    assert shifted.data_ptr() % 16 == 4 and every_other[..., ::2].stride(2) == 2
    grads = []
    for xin in (x_tbv.clone(), every_other[..., ::2], shifted):
        xin = xin.detach().requires_grad_(True)
        got = ctc_loss(xin, *args, **kw)
        got.sum().backward()
        assert torch.equal(got, want) and xin.grad.shape == (Tn, B, V)
        grads.append(xin.grad.contiguous())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2]) and bool(grads[0].any())


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("name", ["ragged", "v413"])
def test_16_bit_input_is_the_float32_call_on_the_widened_input(dt, name):
    dtype, elem = (torch.bfloat16, rlib.LOSS_BF16) if dt == "bfloat16" else (torch.float16, rlib.LOSS_F16)
    x, y, Tb, Lb = _inputs(name, 4.0)
    blank = SHAPES[name][3]
    x16 = torch.from_numpy(x).cuda().to(dtype)
    nll16, beta16, grad16 = _device(x16, None, y, Tb, Lb, blank, elem=elem)
    nll32, beta32, grad32 = _device(x16.float(), None, y, Tb, Lb, blank)
    assert grad16.dtype == dtype and np.isfinite(nll16).all()
    assert np.array_equal(_bits(nll16), _bits(nll32)) and np.array_equal(_bits(beta16), _bits(beta32))
    assert np.array_equal(_bits(grad16.view(torch.int16).cpu().numpy()), _bits(grad32.to(dtype).view(torch.int16).cpu().numpy())), \
        "the 16-bit gradient is not the float32 gradient rounded once to nearest even"
    assert bool((grad16 != 0).any())


def test_log_probabilities_on_the_device(yardstick):
    """fused_log_softmax = 0 against the host twin (f64): no lse, so the picks are the inputs and the value is f64 over the same numbers"""
    _, _, e_grad = yardstick
    x, y, Tb, Lb = _inputs("v413", 4.0)
    lp = np.where(np.isnan(x), np.nan, torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()).astype(np.float32)
    want_nll, want_grad = rlib.ctc_loss_host(lp, y, Tb, Lb, 5, fused_log_softmax=False)
    nll, _, grad = _device(torch.from_numpy(lp).cuda(), None, y, Tb, Lb, 5, fused=False)
    assert (np.abs(nll - want_nll) <= 1e-9 * np.abs(want_nll)).all()
    assert np.abs(grad.cpu().numpy() - want_grad).max() <= FACTOR * e_grad


def test_agrees_with_rnnt_ctc_nll(np_state_dict):
    """lp = rnnt_ctc_logprobs of a small fp32-mode engine; rnnt_ctc_nll scores the same frames and transcripts itself"""
    V, BLANK = T.VOCAB, T.BLANK
    B, Tn, Lmax = 3, 21, 6
    eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=V, blank_id=BLANK, max_beam=0)
    try:
        eng.load_state_dict(np_state_dict(0), numerics="fp32")
        s = torch.cuda.current_stream().cuda_stream
        Tb, Lb = np.array([21, 13, 8], np.int32), np.array([6, 3, 5], np.int32)
        g = np.random.Generator(np.random.Philox(key=[31, 8]))
        lab = g.integers(0, V - 1, (B, Lmax))
        y = np.where(lab >= BLANK, lab + 1, lab).astype(np.int32)
        enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(32)).cuda()
        lp_d = torch.empty(B, Tn, V, device="cuda")
        eng.ctc_logprobs(enc_d.data_ptr(), B * Tn, lp_d.data_ptr(), s)
        want = eng.ctc_nll(enc_d.data_ptr(), Tb, y, Lb, B, Tn, s)
        nll, _, _ = _device(lp_d, None, y, Tb, Lb, BLANK, want_grad=False, fused=False)
        print("loss over rnnt_ctc_logprobs", nll, "rnnt_ctc_nll", want)
        assert np.isfinite(want).all() and (np.abs(nll - want) <= 1e-9 * np.abs(want)).all()
    finally:
        eng.close()


def test_ctc_loss_backward_on_cuda_tensors(yardstick):
    _, e_nll, e_grad = yardstick
    x, y, Tb, Lb = _inputs("tight", 4.0)
    args = (torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Lb))
    kw = dict(blank=SHAPES["tight"][3], reduction="mean", zero_infinity=True, fused_log_softmax=True)
    xc = torch.from_numpy(x).transpose(0, 1).detach().requires_grad_(True)
    loss_c = ctc_loss(xc, *args, **kw)
    loss_c.backward()
    xg = torch.from_numpy(x).cuda().transpose(0, 1).detach().requires_grad_(True)
    loss_g = ctc_loss(xg, *(a.cuda() for a in args), **kw)
    loss_g.backward()
    assert loss_g.is_cuda and xg.grad.is_cuda and loss_g.dtype == torch.float32
    lg, lc = float(loss_g.detach()), float(loss_c.detach())
    assert math.isfinite(lc) and abs(lg - lc) <= (FACTOR * e_nll + 2.0 ** -22) * abs(lc)     # (float32 results: two roundings)
    smallest = min(len(Tb) * max(int(l), 1) for l in Lb)           # d loss / d nll_b = 1 / (B max(L_b, 1))
    assert float((xg.grad.cpu() - xc.grad).abs().max()) <= FACTOR * e_grad / smallest
    gg = xg.grad.transpose(0, 1).cpu().numpy()
    assert not _bits(gg)[np.isnan(x).any(-1)].any() and not _bits(gg[1]).any() and gg[0].any() and gg[2].any()


def test_ctc_head_on_the_device_vs_the_cpu(yardstick):
    """With G = d loss / d logits, the head's three gradients are d hs = G W, d W = G^T hs, d bias = sum over frames of G.  The loss
    kernels owe |G_device - G_cpu| <= e = 8 E_grad / (B min_b max(L_b, 1)) per element, so each gradient is within e times the largest
    of the three 1-norms it is contracted with: max_d sum_v |W[v, d]|, max_d sum_{b, t < T_b} |hs[b, t, d]|, and the number of valid
    frames.  (The projection itself is torch's on both sides; float32 GEMM rounding is orders below e.)"""
    _, e_nll, e_grad = yardstick
    x, y, Tb, Lb = _inputs("tight", 1.0)
    B, Tn, V = x.shape
    D = 16
    head_c = CTCHead(V, D, blank_id=SHAPES["tight"][3])
    head_g = CTCHead(V, D, blank_id=SHAPES["tight"][3]).cuda()
    head_g.load_state_dict(head_c.state_dict())
    hs = torch.randn(B, Tn, D, generator=torch.Generator().manual_seed(9))
    args = (torch.from_numpy(Tb), torch.from_numpy(y), torch.from_numpy(Lb))
    hc = hs.clone().requires_grad_(True)
    loss_c, _ = head_c(hc, *args)
    loss_c.backward()
    hg = hs.cuda().requires_grad_(True)
    loss_g, lp_g = head_g(hg, *args, return_log_probs=True)
    loss_g.backward()
    assert lp_g.shape == (B, Tn, V) and lp_g.is_cuda
    lc = float(loss_c.detach())
    assert abs(float(loss_g.detach()) - lc) <= (FACTOR * e_nll + 2.0 ** -22) * abs(lc)
    e = FACTOR * e_grad / min(B * max(int(l), 1) for l in Lb)
    valid = torch.arange(Tn)[None, :] < torch.from_numpy(Tb)[:, None]
    norm = max(float(head_c.ctc_lo.weight.detach().abs().sum(0).max()), float((hs.abs() * valid[:, :, None]).sum((0, 1)).max()), float(valid.sum()))
    assert norm >= 1.0
    for got, want in ((hg.grad, hc.grad), (head_g.ctc_lo.weight.grad, head_c.ctc_lo.weight.grad), (head_g.ctc_lo.bias.grad, head_c.ctc_lo.bias.grad)):
        assert got.is_cuda and bool(want.abs().max() > 0) and float((got.cpu() - want).abs().max()) <= e * norm


def test_a_refusal_launches_nothing():
    x, y, Tb, Lb = _inputs("tight", 1.0)
    B, Tn, V = x.shape
    blank = SHAPES["tight"][3]
    y_blank = y.copy()
    y_blank[0, 1] = blank                                          # the blank inside row 0's length
    flat = torch.full((B * Tn * V + 8,), 7.0, device="cuda")
    x_d = torch.from_numpy(x).cuda()
    nbytes = rlib.ctc_loss_workspace(B, Tn, y.shape[1])
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    assert flat.data_ptr() % 16 == 0

    def call(tg=y, grad_ptr=None, bytes_=nbytes, elem=None, strides=(Tn * V, V), x_ptr=None):
        try:
            rlib.ctc_loss_device(x_ptr or x_d.data_ptr(), (B, Tn, V), strides, tg, Tb, Lb, blank, True, nll.data_ptr(), grad_ptr or flat.data_ptr(),
                                 work.data_ptr(), bytes_, torch.cuda.current_stream().cuda_stream, elem=elem)
        except RnntError as e:
            return e.status
        return 0
    assert call(grad_ptr=flat[1:].data_ptr()) == rlib.ERR_ARG       # 4 bytes past a 16-byte boundary
    assert call(x_ptr=x_d.data_ptr() + 4) == rlib.ERR_ARG
    assert call(tg=y_blank) == rlib.ERR_ARG
    assert call(strides=(Tn * V, V - 1)) == rlib.ERR_ARG            # a stride below V
    assert call(strides=(Tn * V - 1, V)) == rlib.ERR_ARG            # rows overlap
    assert call(bytes_=nbytes - 1) == rlib.ERR_SHAPE
    assert call(elem=3) == rlib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((nll == 7.0).all()) and bool((flat == 7.0).all()) and not bool(work.any())
    assert call() == 0                                             # and the same arguments unrefused do run
    torch.cuda.synchronize()
    assert not bool((nll == 7.0).any())
