"""The joint lattice with gradients on the device (rnnt_joint_lattice_forward / _backward, ctc_vr_amd.functional.transducer_joint on
CUDA tensors).  Needs a real MI355X: `pytest -m gpu`.

The yardstick is float64 torch autograd of tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ W.T + b on the CPU (testing.joint_backward_ref).
The device owes bf16x3 contractions, float32 tanh and float32 sums, which is what testing.joint_backward_emulation does on the CPU.
So the bound is measured, not chosen: E_x is the emulation's largest absolute distance from float64 over the cases of
joint_grad_cases.py for x in (de, dp, dW, db), and the device is held to 8 E_x: the factor covers another summation tree and device
exp2 / rcp within a couple of ulps.  `tiles` is the shape at which every workgroup of joint_grad_dz and joint_grad_dw takes several
tiles and every slab reduce adds several partials (joint_grad_cases.py says which counts)."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
import joint_grad_cases as C
from ctc_vr_amd.functional import TransducerJoint, rnnt_loss, transducer_joint
from ctc_vr_amd.lib import RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
LOGIT_TOL = 1e-3
GUARD = 64                        # floats behind every output, which no kernel may touch
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def yardstick():
    E = C.yardstick()
    print("emulation vs float64: " + ", ".join(f"E_{x} = {E[x]:.3e}" for x in C.NAMES))
    for x in C.NAMES:
        assert 0.0 < E[x] < 1e-2, f"E_{x} = {E[x]}: an emulation that costs nothing (or everything) measures nothing"
    return E


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(n):
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _backward(dev, shape, g_d, ll=None, tl=None):
    """one rnnt_joint_lattice_backward call into NaN-filled, guarded outputs: ([de, dp, dW, db] as numpy, guards intact)"""
    B, Tn, U1, V = shape
    e_d, p_d, w_d = dev
    nbytes = rlib.joint_lattice_workspace(B, Tn, U1, V)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    sizes = (B * Tn * C.D, B * U1 * C.D, V * C.D, V)
    outs = [_guarded(n) for n in sizes]
    rlib.joint_lattice_backward_device(e_d.data_ptr(), p_d.data_ptr(), w_d.data_ptr(), g_d.data_ptr(), ll, tl, shape, *(o.data_ptr() for o in outs),
                                       work.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs]
    intact = all(bool((h[n:] == np.float32(SENTINEL)).all()) for h, n in zip(host, sizes))
    shapes = ((B, Tn, C.D), (B, U1, C.D), (V, C.D), (V,))
    return [h[:n].reshape(s) for h, n, s in zip(host, sizes, shapes)], intact


@pytest.mark.parametrize("name,scale", C.CASES)
def test_backward_vs_float64(name, scale, yardstick):
    E = yardstick
    B, Tn, U1, V, _ = C.SHAPES[name]
    shape = (B, Tn, U1, V)
    e, p, w, _, g = C.inputs(name, scale)
    dev = tuple(torch.from_numpy(a).cuda() for a in (e, p, w))
    # without lengths every cell counts: the reference includes what the length tests call padding
    got, intact = _backward(dev, shape, torch.from_numpy(g).cuda())
    assert intact, "something was written behind an output"
    ratios = {}
    for x, a, want in zip(C.NAMES, got, C.reference(name, scale, False)):
        assert np.isfinite(a).all(), f"{x}: an element was not written (or is not finite)"
        ratios[x] = float(np.abs(a - want).max()) / E[x]
    print(f"{name} x{scale:g} all cells: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items()))
    again, _ = _backward(dev, shape, torch.from_numpy(g).cuda())
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again)), "two calls on the same inputs differ"
    # with lengths: the padding of g, e and p holds NaN and must never reach a result; the result equals the run over zero padding, bit for bit
    ll, tl = C.rows(name)
    live = T.joint_live_cells(B, Tn, U1, ll, tl)[..., None]
    e_nan, p_nan = e.copy(), p.copy()                              # frames and labels beyond a row's lengths hold NaN as well
    for i in range(B):
        e_nan[i, ll[i]:] = np.nan
        p_nan[i, tl[i] + 1:] = np.nan
    dev_nan = (torch.from_numpy(e_nan).cuda(), torch.from_numpy(p_nan).cuda(), dev[2])
    got_nan, intact = _backward(dev_nan, shape, torch.from_numpy(np.where(live, g, np.float32("nan")).astype(np.float32)).cuda(), ll, tl)
    got_zero, _ = _backward(dev, shape, torch.from_numpy(np.where(live, g, np.float32(0.0)).astype(np.float32)).cuda(), ll, tl)
    assert intact
    lratios = {}
    for x, a, z, want in zip(C.NAMES, got_nan, got_zero, C.reference(name, scale, True)):
        assert np.isfinite(a).all(), f"{x}: padding was read"
        assert np.array_equal(_bits(a), _bits(z)), f"{x}: NaN padding and zero padding differ"
        lratios[x] = float(np.abs(a - want).max()) / E[x]
    print(f"{name} x{scale:g} with lengths: " + ", ".join(f"{x} {r:.3f} E" for x, r in lratios.items()))
    for x in C.NAMES:
        assert ratios[x] <= FACTOR and lratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E / {lratios[x]:.2f} E, the bound is {FACTOR:g} E"
    if scale == 30.0:                                              # far beyond saturation (and beyond exp2's range) h = +-1 exactly: dz is exactly 0
        sat = (np.abs(T.JR_PRESCALE * e[:, :, None, :] + T.JR_PRESCALE * p[:, None, :, :]) > 40.0).all(axis=2)     # every u of the frame
        assert (sat.any() or name != "one") and not got[0][sat].any(), "1 - h^2 is not exactly 0 where h has saturated"


@pytest.mark.parametrize("name,scale", C.CASES)
def test_forward_vs_float64(name, scale):
    B, Tn, U1, V, _ = C.SHAPES[name]
    e, p, w, b, _ = C.inputs(name, scale)
    e_d, p_d, w_d, b_d = (torch.from_numpy(a).cuda() for a in (e, p, w, b))
    nbytes = rlib.joint_lattice_workspace(B, Tn, U1, V)
    work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = _guarded(B * Tn * U1 * V)
    rlib.joint_lattice_forward_device(e_d.data_ptr(), p_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), (B, Tn, U1, V), out.data_ptr(), work.data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out[B * Tn * U1 * V:] == SENTINEL).all())
    got = out[:B * Tn * U1 * V].view(B, Tn, U1, V)
    err = 0.0
    w64, b64 = torch.from_numpy(w).double(), torch.from_numpy(b).double()
    for i in range(B):                                             # float64, one batch row at a time
        want = torch.tanh(torch.from_numpy(e[i]).double().unsqueeze(1) + torch.from_numpy(p[i]).double().unsqueeze(0)) @ w64.T + b64
        row = got[i].cpu().double()
        assert bool(torch.isfinite(row).all())
        err = max(err, float((row - want).abs().max()))
    print(f"{name} x{scale:g}: forward error {err:.3e}")
    assert err <= LOGIT_TOL
    via = transducer_joint(e_d, p_d, w_d, b_d)                       # the autograd function runs the same entry: the same bits
    assert torch.equal(via, got)


# ---- the chain joint -> rnnt_loss -> backward ------------------------------------------------------------------------------------
CHAIN = ["ragged", "u28"]


def _chain_inputs(name):
    B, Tn, U1, V, _ = C.SHAPES[name]
    e, p, w, b, _ = C.inputs(name, 1.0)
    ll, tl = C.rows(name)
    r = np.random.Generator(np.random.Philox(key=[77, sorted(C.SHAPES).index(name)]))
    blank = 5
    lab = r.integers(0, V - 1, (B, U1 - 1))
    y = np.where(lab >= blank, lab + 1, lab).astype(np.int32)
    return e, p, w, b, y, ll, tl, blank


def _loss_grad(fn, logits, y, ll, tl, blank):
    """d mean(nll) / d logits [B, T, U1, V] float64 through fn = transducer_loss_ref or transducer_loss_f32_emulation"""
    B = logits.shape[0]
    return np.stack([fn(logits[b], y[b], int(ll[b]), int(tl[b]), blank)[1] for b in range(B)]) / B


@pytest.fixture(scope="module")
def chain_yardstick():
    """Per chain case the float64 chain's four gradients, and E_chain per output: the composed emulation (split-plane forward,
    transducer_loss_f32_emulation, the backward emulation on its float32 gradient) against it."""
    refs, E = {}, dict.fromkeys(C.NAMES, 0.0)
    for name in CHAIN:
        e, p, w, b, y, ll, tl, blank = _chain_inputs(name)
        logits64 = (torch.tanh(torch.from_numpy(e).double().unsqueeze(2) + torch.from_numpy(p).double().unsqueeze(1)) @ torch.from_numpy(w).double().T
                    + torch.from_numpy(b).double()).numpy()
        want = T.joint_backward_ref(e, p, w, _loss_grad(T.transducer_loss_ref, logits64, y, ll, tl, blank), ll, tl)
        g_emu = _loss_grad(T.transducer_loss_f32_emulation, T.joint_forward_emulation(e, p, w, b), y, ll, tl, blank).astype(np.float32)
        emu = T.joint_backward_emulation(e, p, w, g_emu, ll, tl)
        for x, a, ref in zip(C.NAMES, emu, want):
            E[x] = max(E[x], float(np.abs(a - ref).max()))
        refs[name] = want
    print("chain emulation vs float64: " + ", ".join(f"E_{x} = {E[x]:.3e}" for x in C.NAMES))
    for x in C.NAMES:
        assert 0.0 < E[x] < 1e-2
    return refs, E


@pytest.mark.parametrize("name", CHAIN)
def test_chain_joint_loss_backward(name, chain_yardstick):
    refs, E = chain_yardstick
    e, p, w, b, y, ll, tl, blank = _chain_inputs(name)
    leaves = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (e, p, w, b)]
    lens = (torch.from_numpy(ll).cuda(), torch.from_numpy(tl).cuda())
    logits = transducer_joint(*leaves, *lens)
    loss = rnnt_loss(logits, torch.from_numpy(y).cuda(), *lens, blank=blank, reduction="mean")
    loss.backward()
    ratios = {x: float(np.abs(t.grad.cpu().numpy() - want).max()) / E[x] for x, t, want in zip(C.NAMES, leaves, refs[name])}
    print(f"{name}: chain " + ", ".join(f"{x} {r:.3f} E_chain" for x, r in ratios.items()))
    for x, t in zip(C.NAMES, leaves):
        assert t.grad.is_cuda and bool(torch.isfinite(t.grad).all())
        assert ratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E_chain"


def test_module_on_the_device_saves_only_its_inputs():
    B, Tn, U1, V = 2, 7, 28, 412
    m = TransducerJoint(V, 256, 256).cuda()
    enc, pred = torch.randn(B, Tn, 256, device="cuda"), torch.randn(B, U1, 256, device="cuda")
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t.numel()), t)[1], lambda t: t):
        out = m(enc, pred)
    assert out.shape == (B, Tn, U1, V) and out.is_cuda
    assert max(saved) <= max(B * Tn, B * U1, V) * 256, saved
    out.sum().backward()
    for prm in m.parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all())
    ref = torch.tanh(m.enc_ffn(enc).unsqueeze(2) + m.pred_ffn(pred).unsqueeze(1)) @ m.ffn_out.weight.T + m.ffn_out.bias
    assert float((out - ref).detach().abs().max()) <= LOGIT_TOL


def test_a_refusal_launches_nothing():
    B, Tn, U1, V = 2, 5, 3, 20
    e, p, w, b, g = C.inputs("v20", 1.0)
    e_d, p_d, w_d, b_d, g_d = (torch.from_numpy(a).cuda() for a in (e, p, w, b, g))
    nbytes = rlib.joint_lattice_workspace(B, Tn, U1, V)
    work = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), 7.0, device="cuda") for n in (B * Tn * 256, B * U1 * 256, V * 256, V)]
    lat = torch.full((B, Tn, U1, V), 7.0, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ptrs = [o.data_ptr() for o in outs]

    def back(shape=(B, Tn, U1, V), ll=None, tl=None, nb=nbytes, g_ptr=g_d.data_ptr()):
        rlib.joint_lattice_backward_device(e_d.data_ptr(), p_d.data_ptr(), w_d.data_ptr(), g_ptr, ll, tl, shape, *ptrs, work.data_ptr(), nb, s)

    for kw, status in (({"ll": [6, 5]}, rlib.ERR_ARG), ({"ll": [0, 5]}, rlib.ERR_ARG), ({"tl": [3, 0]}, rlib.ERR_ARG), ({"tl": [-1, 0]}, rlib.ERR_ARG),
                       ({"g_ptr": g_d.data_ptr() + 4}, rlib.ERR_ARG), ({"g_ptr": None}, rlib.ERR_ARG), ({"shape": (0, Tn, U1, V)}, rlib.ERR_ARG),
                       ({"shape": (B, Tn, U1, 18)}, rlib.ERR_SHAPE), ({"shape": (B, Tn, U1, 420)}, rlib.ERR_SHAPE), ({"nb": nbytes - 1}, rlib.ERR_SHAPE)):
        with pytest.raises(RnntError) as err:
            back(**kw)
        assert err.value.status == status, kw
    for kw, status in (({"nb": nbytes - 1}, rlib.ERR_SHAPE), ({"shape": (B, Tn, U1, 0)}, rlib.ERR_SHAPE), ({"shape": (B, 0, U1, V)}, rlib.ERR_ARG)):
        with pytest.raises(RnntError) as err:
            rlib.joint_lattice_forward_device(e_d.data_ptr(), p_d.data_ptr(), w_d.data_ptr(), b_d.data_ptr(), kw.get("shape", (B, Tn, U1, V)), lat.data_ptr(),
                                              work.data_ptr(), kw.get("nb", nbytes), s)
        assert err.value.status == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((lat == 7.0).all()) and not bool(work.any())
    with pytest.raises(TypeError):
        transducer_joint(e_d.double(), p_d, w_d, b_d)
    with pytest.raises(RnntError) as err:
        transducer_joint(e_d, p_d, w_d[:18].contiguous(), b_d[:18].contiguous())
    assert err.value.status == rlib.ERR_SHAPE
