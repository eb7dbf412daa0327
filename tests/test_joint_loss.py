"""The fused joint and loss on the device (rnnt_joint_loss_forward / _backward, ctc_vr_amd.functional.transducer_joint_loss on CUDA
tensors).  Needs a real MI355X: `pytest -m gpu`.

The yardstick is the float64 chain tanh(e + p) W^T + b -> testing.transducer_loss_ref -> backward on the CPU
(joint_loss_cases.reference).  The device owes a bf16x3 lattice with float32 tanh, float32 lse and picks, float64 recursions, a float32
g, bf16x3 contractions and float32 sums: what joint_loss_cases.emulation composes on the CPU from testing.joint_forward_emulation,
transducer_loss_f32_emulation and joint_backward_emulation.  So the bound is measured, not chosen: E_x is the emulation's largest
distance from float64 over the cases of joint_loss_cases.py for x in (nll, de, dp, dW, db) -- relative for nll, absolute for the
gradients -- and the device is held to 8 E_x, the project's factor for another summation tree and device exp2 / rcp.  The backward
recomputes the logits in another accumulation order than the forward; that distance lies inside the same contract."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import joint_loss_cases as C
from ctc_vr_amd.functional import TransducerJoint, rnnt_loss, transducer_joint, transducer_joint_loss
from ctc_vr_amd.lib import RnntError
from ctc_vr_amd.testing import JR_PRESCALE

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GUARD = 64                        # floats behind every output, which no kernel may touch
SENTINEL = 12345.0


def _yardstick(kind):
    E = C.yardstick(kind)
    print(f"composed emulation vs float64 ({kind}): " + ", ".join(f"E_{x} = {E[x]:.3e}" for x in C.NAMES))
    for x in C.NAMES:
        assert 0.0 < E[x] < 1e-2, f"E_{x} = {E[x]}: an emulation that costs nothing (or everything) measures nothing"
    return E


@pytest.fixture(scope="module")
def yardstick():
    return _yardstick("mean")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _guarded(n):
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _intact(bufs, sizes):
    return all(bool((b[n:] == SENTINEL).all()) for b, n in zip(bufs, sizes))


def _run(name, scale, row_scale, clamp=-1.0, arrays=None):
    """One rnnt_joint_loss_forward and one rnnt_joint_loss_backward into NaN-filled, guarded nll, state and outputs:
    ([nll, de, dp, dW, db] as numpy, the state as float32, guards intact)"""
    B, Tn, U1, V, _ = C.SHAPES[name]
    e, p, w, b, y, ll, tl, blank = arrays or C.case(name, scale)
    shape = (B, Tn, U1, V)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (e, p, w, b)]
    ptrs = [t.data_ptr() for t in dev]
    wbytes, sbytes = rlib.joint_loss_workspace(*shape)
    assert sbytes % 4 == 0
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    sizes = (2 * B, sbytes // 4, B * Tn * C.D, B * U1 * C.D, V * C.D, V)
    nll, state, *outs = [_guarded(n) for n in sizes]
    rs = torch.from_numpy(np.asarray(row_scale, np.float32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    rlib.joint_loss_forward_device(*ptrs, y, ll, tl, shape, blank, nll.data_ptr(), state.data_ptr(), sbytes, work.data_ptr(), wbytes, s)
    rlib.joint_loss_backward_device(*ptrs, state.data_ptr(), sbytes, rs.data_ptr(), clamp, shape, blank, *(o.data_ptr() for o in outs), work.data_ptr(), wbytes, s)
    torch.cuda.synchronize()
    intact = _intact([nll, state] + outs, sizes)
    host = [nll[:2 * B].cpu().numpy().view(np.float64)] + [o[:n].cpu().numpy().reshape(sh) for o, n, sh in
                                                           zip(outs, sizes[2:], ((B, Tn, C.D), (B, U1, C.D), (V, C.D), (V,)))]
    return host, state[:sbytes // 4].cpu().numpy(), intact


def _ratios(got, want, E):
    return {x: C.distance(x, a, ref) / E[x] for x, a, ref in zip(C.NAMES, got, want)}


@pytest.mark.parametrize("name,scale", [(n, s) for n, s, _ in C.CASES])
def test_fused_vs_float64(name, scale, yardstick):
    E = yardstick
    rs = C.mean_scale(name)
    got, state, intact = _run(name, scale, rs)
    assert intact, "something was written behind nll, the state or an output"
    assert np.isfinite(state).all(), "an element of the state was not written"
    for x, a in zip(C.NAMES, got):
        assert np.isfinite(a).all(), f"{x}: an element was not written (or is not finite)"
    ratios = _ratios(got, C.reference(name, scale), E)
    print(f"{name} x{scale:g}: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items()))
    again, state2, _ = _run(name, scale, rs)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again)) and np.array_equal(_bits(state), _bits(state2)), "two calls differ"
    for x in C.NAMES:
        assert ratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E, the bound is {FACTOR:g} E"
    if scale == 30.0:                                              # far beyond saturation h = +-1 exactly: dz, and so de, is exactly 0
        e, p = C.case(name, scale)[:2]
        sat = (np.abs(JR_PRESCALE * e[:, :, None, :] + JR_PRESCALE * p[:, None, :, :]) > 40.0).all(axis=2)     # every u of the frame
        assert sat.any() and not got[1][sat].any(), "1 - h^2 is not exactly 0 where h has saturated"


def _function(name, reduction, clamp=-1.0, grad_out=None):
    """transducer_joint_loss on CUDA tensors and .backward(): (costs, [de, dp, dW, db]) as numpy"""
    e, p, w, b, y, ll, tl, blank = C.case(name)
    leaves = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (e, p, w, b)]
    cost = transducer_joint_loss(*leaves, torch.from_numpy(y).cuda(), torch.from_numpy(ll).cuda(), torch.from_numpy(tl).cuda(), blank=blank, clamp=clamp,
                                 reduction=reduction)
    assert cost.is_cuda and cost.dtype == torch.float32
    cost.backward(None if grad_out is None else torch.from_numpy(grad_out).cuda())
    assert all(t.grad.is_cuda and t.grad.shape == t.shape for t in leaves)
    return cost.detach().cpu().numpy(), [t.grad.cpu().numpy() for t in leaves]


F32 = 2.0 ** -24                  # costs come back as float32: one rounding on top of the double the entry point writes


@pytest.mark.parametrize("name", ["ragged", "u28"])
def test_row_scale_of_reduction_none(name):
    """a non-uniform incoming gradient: dW and db sum over batch rows, so a scale applied behind those sums would show here.  The
    gradients are linear in the row scale and these scales reach 2, so the yardstick is the emulation's on these very runs."""
    E = _yardstick("none")
    go = C.grad_out(C.SHAPES[name][0])
    costs, grads = _function(name, "none", grad_out=go.astype(np.float32))
    want = C.reference(name, 1.0, go)
    ratios = _ratios([want[0]] + grads, want, E)
    print(f"{name} none, grad_out {go.tolist()}: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items() if x != "nll"))
    assert C.distance("nll", costs, want[0]) <= FACTOR * E["nll"] + F32
    for x in C.NAMES[1:]:
        assert ratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E"


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_reductions(reduction):
    E = _yardstick(reduction)
    B = C.SHAPES["ragged"][0]
    cost, grads = _function("ragged", reduction)
    want = C.reference("ragged", 1.0, np.full(B, 1.0 / B if reduction == "mean" else 1.0))
    ref = want[0].mean() if reduction == "mean" else want[0].sum()
    assert abs(float(cost) - ref) <= (FACTOR * E["nll"] + 4 * F32) * abs(ref)      # B float32 costs and their float32 sum
    ratios = _ratios([want[0]] + grads, want, E)
    print(f"ragged {reduction}: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items() if x != "nll"))
    for x in C.NAMES[1:]:
        assert ratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E"


def test_clamp():
    """clamp = 0.01 applies to d nll_b / d logits, before the row scale: against the float64 chain clamped there"""
    E = _yardstick("clamp")
    _, grads = _function("ragged", "mean", clamp=0.01)
    want = C.reference("ragged", 1.0, clamp=C.CLAMP)
    ratios = _ratios([want[0]] + grads, want, E)
    print("ragged clamp 0.01: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items() if x != "nll"))
    for x in C.NAMES[1:]:
        assert ratios[x] <= FACTOR, f"{x}: {ratios[x]:.2f} E"
    assert np.abs(grads[3] - C.reference("ragged", 1.0)[4]).max() > 1e-4, "a clamp of 0.01 changes db"


@pytest.mark.parametrize("name", ["ragged", "u28"])
def test_padding_is_never_read(name):
    """e and p beyond each row's lengths hold NaN, targets beyond U_b hold V + 7: finite, and bit-equal to zeros / valid labels there"""
    e, p, w, b, y, ll, tl, blank = C.case(name)
    V = w.shape[0]
    e0, p0, y0, e1, p1, y1 = e.copy(), p.copy(), y.copy(), e.copy(), p.copy(), y.copy()
    for i in range(len(ll)):
        e0[i, ll[i]:], p0[i, tl[i] + 1:], y0[i, tl[i]:] = 0.0, 0.0, (blank + 1) % V
        e1[i, ll[i]:], p1[i, tl[i] + 1:], y1[i, tl[i]:] = np.nan, np.nan, V + 7
    rs = C.grad_out(len(ll))
    zero, _, _ = _run(name, 1.0, rs, arrays=(e0, p0, w, b, y0, ll, tl, blank))
    nan, _, intact = _run(name, 1.0, rs, arrays=(e1, p1, w, b, y1, ll, tl, blank))
    assert intact
    for x, a, z in zip(C.NAMES, nan, zero):
        assert np.isfinite(a).all(), f"{x}: padding was read"
        assert np.array_equal(_bits(a), _bits(z)), f"{x}: NaN padding and zero padding differ"


def test_nothing_lattice_sized_exists():
    B, Tn, U1, V = 16, 249, 28, 412
    M = B * Tn * U1
    _, sbytes = rlib.joint_loss_workspace(B, Tn, U1, V)
    m = TransducerJoint(V, 256, 256).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    enc, pred = torch.randn(B, Tn, 256, device="cuda", generator=g), torch.randn(B, U1, 256, device="cuda", generator=g)
    y = torch.randint(0, V - 1, (B, U1 - 1), device="cuda", generator=g)
    ll, tl = torch.full((B,), Tn, device="cuda"), torch.full((B,), U1 - 1, device="cuda")
    # torch's BLAS workspaces (76 MiB each, one for the forward's thread and one for autograd's) are allocated at a thread's first GEMM
    # and kept for the life of the process: the two nn.Linear run once, forward and backward, before anything is measured
    (m.enc_ffn(enc).sum() + m.pred_ffn(pred).sum()).backward()
    m.zero_grad(set_to_none=True)
    saved = []
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t.numel()), t)[1], lambda t: t):
        loss = m.loss(enc, pred, y, ll, tl)
    assert max(saved) <= max(sbytes, B * Tn * 256, B * U1 * 256, V * 256), saved
    loss.backward()
    torch.cuda.synchronize()
    fused = torch.cuda.max_memory_allocated() - before
    assert bool(torch.isfinite(loss)) and all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for prm in m.parameters())
    m.zero_grad(set_to_none=True)
    del loss
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rnnt_loss(m(enc, pred, ll, tl), y, ll, tl).backward()
    torch.cuda.synchronize()
    unfused = torch.cuda.max_memory_allocated() - before
    print(f"peak memory above the inputs at B {B} x T {Tn} x U1 {U1} x V {V}: fused {fused / 1e6:.1f} MB, unfused chain {unfused / 1e6:.1f} MB, "
          f"lattice {4 * M * V / 1e6:.1f} MB")
    assert fused <= 4 * M * V // 2


def test_a_refusal_launches_nothing():
    B, Tn, U1, V, _ = C.SHAPES["v20"]
    e, p, w, b, y, ll, tl, blank = C.case("v20")
    dev = [torch.from_numpy(a).cuda() for a in (e, p, w, b)]
    wbytes, sbytes = rlib.joint_loss_workspace(B, Tn, U1, V)
    work = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")
    state = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    nll = torch.full((B,), 7.0, dtype=torch.float64, device="cuda")
    rs = torch.ones(B, device="cuda")
    outs = [torch.full((n,), 7.0, device="cuda") for n in (B * Tn * 256, B * U1 * 256, V * 256, V)]
    s = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in dev]

    def fwd(shape=(B, Tn, U1, V), y=y, ll=ll, tl=tl, blank=blank, sb=sbytes, wb=wbytes, e_ptr=ptrs[0], state_ptr=state.data_ptr()):
        rlib.joint_loss_forward_device(e_ptr, *ptrs[1:], y, ll, tl, shape, blank, nll.data_ptr(), state_ptr, sb, work.data_ptr(), wb, s)

    def bwd(shape=(B, Tn, U1, V), blank=blank, sb=sbytes, wb=wbytes, e_ptr=ptrs[0], rs_ptr=rs.data_ptr()):
        rlib.joint_loss_backward_device(e_ptr, *ptrs[1:], state.data_ptr(), sb, rs_ptr, -1.0, shape, blank, *(o.data_ptr() for o in outs), work.data_ptr(), wb, s)

    bad_y = y.copy()
    bad_y[0, 0] = blank
    for kw, status in (({"ll": [6, 5]}, rlib.ERR_ARG), ({"ll": [0, 5]}, rlib.ERR_ARG), ({"tl": [3, 0]}, rlib.ERR_ARG), ({"tl": [-1, 0]}, rlib.ERR_ARG),
                       ({"y": bad_y}, rlib.ERR_ARG), ({"blank": V}, rlib.ERR_ARG), ({"e_ptr": ptrs[0] + 4}, rlib.ERR_ARG), ({"e_ptr": None}, rlib.ERR_ARG),
                       ({"state_ptr": None}, rlib.ERR_ARG), ({"shape": (0, Tn, U1, V), "y": y[:0], "ll": ll[:0], "tl": tl[:0]}, rlib.ERR_ARG),
                       ({"shape": (B, Tn, U1, 18)}, rlib.ERR_SHAPE), ({"shape": (B, Tn, U1, 420)}, rlib.ERR_SHAPE),
                       ({"shape": (B, Tn, 257, V), "y": np.ones((B, 256), np.int32), "tl": [0, 0]}, rlib.ERR_SHAPE),
                       ({"wb": wbytes - 1}, rlib.ERR_SHAPE), ({"sb": sbytes - 1}, rlib.ERR_SHAPE)):
        with pytest.raises(RnntError) as err:
            fwd(**kw)
        assert err.value.status == status, kw
    for kw, status in (({"blank": -1}, rlib.ERR_ARG), ({"e_ptr": ptrs[0] + 4}, rlib.ERR_ARG), ({"rs_ptr": None}, rlib.ERR_ARG), ({"shape": (B, 0, U1, V)}, rlib.ERR_ARG),
                       ({"shape": (B, Tn, U1, 18)}, rlib.ERR_SHAPE), ({"shape": (B, Tn, U1, 420)}, rlib.ERR_SHAPE), ({"shape": (B, Tn, 257, V)}, rlib.ERR_SHAPE),
                       ({"wb": wbytes - 1}, rlib.ERR_SHAPE), ({"sb": sbytes - 1}, rlib.ERR_SHAPE)):
        with pytest.raises(RnntError) as err:
            bwd(**kw)
        assert err.value.status == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and bool((nll == 7.0).all()) and not bool(work.any()) and not bool(state.any())
    with pytest.raises(TypeError):
        transducer_joint_loss(dev[0].double(), *dev[1:], torch.from_numpy(y).cuda(), torch.from_numpy(ll).cuda(), torch.from_numpy(tl).cuda())
    with pytest.raises(RnntError) as err:
        transducer_joint_loss(*dev[:2], dev[2][:18].contiguous(), dev[3][:18].contiguous(), torch.from_numpy(y).cuda(), torch.from_numpy(ll).cuda(),
                              torch.from_numpy(tl).cuda())
    assert err.value.status == rlib.ERR_SHAPE


def test_fused_against_the_unfused_chain_printed():
    """no assertion on the distance: both sides are held to float64 elsewhere; the figure goes into DESIGN.md"""
    e, p, w, b, y, ll, tl, blank = C.case("u28")
    _, fused = _function("u28", "mean")
    leaves = [torch.from_numpy(a).cuda().requires_grad_(True) for a in (e, p, w, b)]
    lens = (torch.from_numpy(ll).cuda(), torch.from_numpy(tl).cuda())
    rnnt_loss(transducer_joint(*leaves, *lens), torch.from_numpy(y).cuda(), *lens, blank=blank, reduction="mean").backward()
    diffs = {x: float(np.abs(a - t.grad.cpu().numpy()).max()) for x, a, t in zip(C.NAMES[1:], fused, leaves)}
    print("u28, fused against transducer_joint -> rnnt_loss -> backward: " + ", ".join(f"{x} {d:.3e}" for x, d in diffs.items()))
    assert all(np.isfinite(d) for d in diffs.values())
