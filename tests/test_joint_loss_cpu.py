"""The fused joint and loss without a GPU: ctc_vr_amd.functional.transducer_joint_loss on CPU tensors and its float64 twin
rnnt_joint_loss_host against float64 torch autograd of the chain tanh(e + p) W^T + b -> testing.transducer_loss_ref -> backward
(joint_loss_cases.reference), the memory formula of rnnt_joint_loss_workspace, and every refusal the host decides, with its status.

The bound is the project's 1e-9 for float64 code against its float64 restatement (test_joint_grad_cpu.py, test_rnnt_loss_cpu.py).
The twin's float64 outputs are held to exactly that.  The autograd function returns float32 tensors, so on top of it stands the one
rounding of each result to float32, 2^-24 relative (a float32 cannot hold a loss of 50 to 1e-9): the convention those two files use
for float32 results of a float64 twin."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import joint_loss_cases as C
from ctc_vr_amd.functional import TransducerJoint, transducer_joint_loss
from ctc_vr_amd.lib import RnntError

REC_RTOL = 1e-9
F32 = 2.0 ** -24                  # one rounding to float32, relative


def _close(got, want, what, rel=0.0):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = REC_RTOL * np.maximum(1.0, np.abs(want)) + rel * np.abs(want)
    assert (err <= bound).all(), f"{what}: max error {err.max():.3e}"


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("name", ["one", "ragged", "v20"])
def test_cpu_path_vs_float64_autograd(name, reduction):
    e, p, w, b, y, ll, tl, blank = C.case(name)
    B = len(ll)
    rs = {"none": C.grad_out(B), "mean": np.full(B, 1.0 / B), "sum": np.ones(B)}[reduction]
    want = C.reference(name, 1.0, rs)
    # the float64 twin: nothing is rounded anywhere
    nll, outs = rlib.joint_loss_host(e, p, w, b, y, ll, tl, blank, row_scale=rs)
    for x, a, ref in zip(C.NAMES, (nll,) + outs, want):
        assert a.dtype == np.float64 and np.isfinite(a).all()
        _close(a, ref, f"{name} {reduction} twin {x}")
    # the autograd function on CPU tensors: the same values, each rounded once to float32.  What it is handed as d loss / d nll_b is a
    # float32 (torch's mean gives it float32(1 / B), not 1 / B), so that is the scale of its reference
    want = C.reference(name, 1.0, rs.astype(np.float32).astype(np.float64))
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (e, p, w, b)]
    cost = transducer_joint_loss(*leaves, torch.from_numpy(y), torch.from_numpy(ll), torch.from_numpy(tl), blank=blank, reduction=reduction)
    assert cost.dtype == torch.float32
    if reduction == "none":
        assert cost.shape == (B,)
        _close(cost.detach().numpy(), want[0], "costs", rel=F32)
        cost.backward(torch.from_numpy(rs).float())
    else:
        assert cost.dim() == 0
        _close(float(cost.detach()), want[0].mean() if reduction == "mean" else want[0].sum(), "cost", rel=4 * F32)   # B roundings and the sum's
        cost.backward()
    for x, t, ref in zip(C.NAMES[1:], leaves, want[1:]):
        assert t.grad.dtype == torch.float32 and t.grad.shape == t.shape
        _close(t.grad.numpy(), ref, f"{name} {reduction} {x}", rel=F32)


def test_cpu_path_clamp_and_padding():
    e, p, w, b, y, ll, tl, blank = C.case("ragged")
    want = C.reference("ragged", 1.0, clamp=C.CLAMP)
    e, p, y = e.copy(), p.copy(), y.copy()
    for i in range(len(ll)):                                       # what lies outside a row's lengths is never read
        e[i, ll[i]:] = np.nan
        p[i, tl[i] + 1:] = np.nan
        y[i, tl[i]:] = w.shape[0] + 7
    nll, outs = rlib.joint_loss_host(e, p, w, b, y, ll, tl, blank, clamp=C.CLAMP, row_scale=C.mean_scale("ragged"))
    for x, a, ref in zip(C.NAMES, (nll,) + outs, want):
        assert np.isfinite(a).all()
        _close(a, ref, "clamped " + x)
    assert np.abs(outs[3] - C.reference("ragged", 1.0)[4]).max() > 1e-4, "a clamp of 0.01 changes db"


def test_module_loss_on_cpu_saves_only_its_inputs():
    B, Tn, U1, V, _ = C.SHAPES["u28"]
    _, _, _, _, y, ll, tl, _ = C.case("u28")
    m = TransducerJoint(V, 256, 256)
    enc, pred = torch.randn(B, Tn, 256), torch.randn(B, U1, 256)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t.numel()), t)[1], lambda t: t):
        loss = m.loss(enc, pred, torch.from_numpy(y), torch.from_numpy(ll), torch.from_numpy(tl), blank=0)
    assert max(saved) <= max(B * Tn, B * U1, V) * 256, saved
    loss.backward()
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for prm in m.parameters())


def _formula(B, Tn, U1, V):
    """include/rnnt_hip.h, restated: (work_bytes, state_bytes)"""
    cdiv = lambda a, b: -(-a // b)
    M = B * Tn * U1
    NUB = cdiv(U1, 16)
    TC = 4 * cdiv(cdiv(Tn, max(1, 512 // (B * NUB))), 4)
    NC = cdiv(Tn, TC)
    CS = 32 * cdiv(cdiv(M, 32), max(1, 512 // cdiv(V, 64)))
    NS = cdiv(M, CS)
    fwd = 8 * (B + B % 2) + 16 * M + 425984 + 4 * (256 * B * (Tn + U1) + 4 + 2 * M + 4 * cdiv(M, 4))
    bwd = 65536 * cdiv(V, 32) + 4 * (256 * (NUB * B * Tn + NC * B * U1 + NS * V) + NS * V)
    return max(fwd, bwd), 16 * M + 16 * cdiv(2 * B + B * max(U1 - 1, 1), 4)


def test_memory_formula():
    for shape in [s[:4] for s in C.SHAPES.values()] + [(16, 249, 28, 412), (64, 249, 28, 412), (1, 2000, 256, 416), (700, 3, 17, 8)]:
        assert rlib.joint_loss_workspace(*shape) == _formula(*shape), shape
    B, Tn, U1, V = 64, 249, 28, 412
    work, state = rlib.joint_loss_workspace(B, Tn, U1, V)
    lattice = 4 * B * Tn * U1 * V
    print(f"B 64 x T 249 x U1 28 x V 412: work {work} + state {state} = {(work + state) / 1e6:.1f} MB against a lattice of {lattice / 1e6:.1f} MB")
    assert work + state <= lattice // 4
    # no term in M V: doubling V at fixed M adds only the V-sized slabs and streams
    w1, s1 = rlib.joint_loss_workspace(B, Tn, U1, 208)
    assert s1 == state and work - w1 < 40e6
    n, k = ctypes.c_int64(-7), ctypes.c_int64(-7)
    lib = rlib.load()
    for args, status in (((0, 1, 1, 4), rlib.ERR_ARG), ((1, 0, 1, 4), rlib.ERR_ARG), ((1, 1, 0, 4), rlib.ERR_ARG), ((1, 1, 1, 0), rlib.ERR_SHAPE),
                         ((1, 1, 1, 18), rlib.ERR_SHAPE), ((1, 1, 1, 420), rlib.ERR_SHAPE), ((1, 1, 257, 4), rlib.ERR_SHAPE),
                         ((3000, 3000, 250, 412), rlib.ERR_SHAPE)):
        assert lib.rnnt_joint_loss_workspace(*args, ctypes.byref(n), ctypes.byref(k)) == status and n.value == -7 and k.value == -7, args
    assert lib.rnnt_joint_loss_workspace(1, 1, 1, 4, None, ctypes.byref(k)) == rlib.ERR_ARG
    assert lib.rnnt_joint_loss_workspace(1, 1, 1, 4, ctypes.byref(n), None) == rlib.ERR_ARG


def test_device_entries_refuse_on_the_host_before_any_launch():
    """bad lengths, the blank inside a transcript, V 18 / 420, Umax 256, a null or misaligned pointer, a short workspace, a short state:
    decided before the first HIP call, with the statuses of the rnnt_joint_lattice_* and rnnt_transducer_loss families; needs no GPU"""
    lib = rlib.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data % 16)                  # a 16-byte aligned (host) address: never followed
    B, Tn, Umax, V, blank = 2, 5, 2, 20, 5
    work, state = rlib.joint_loss_workspace(B, Tn, Umax + 1, V)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    good_y, good_ll, good_tl = np.array([[1, 2], [3, 4]], np.int32), np.array([5, 4], np.int32), np.array([2, 1], np.int32)
    wide_y, wide_tl = np.ones((B, 256), np.int32), np.array([256, 0], np.int32)

    def fwd(**k):
        return lib.rnnt_joint_loss_forward(k.get("e", a), a, a, a, ptr(k.get("y", good_y)), ptr(k.get("ll", good_ll)), ptr(k.get("tl", good_tl)), k.get("B", B), Tn,
                                           k.get("Umax", Umax), k.get("V", V), k.get("blank", blank), k.get("nll", a), k.get("state", a), k.get("sb", state),
                                           k.get("work", a), k.get("wb", work), None)

    def bwd(**k):
        return lib.rnnt_joint_loss_backward(k.get("e", a), a, a, a, k.get("state", a), k.get("sb", state), k.get("rs", a), -1.0, k.get("B", B), Tn,
                                            k.get("Umax", Umax), k.get("V", V), k.get("blank", blank), a, a, a, k.get("db", a), k.get("work", a), k.get("wb", work), None)

    for call in (fwd, bwd):
        assert call(e=None) == rlib.ERR_ARG and call(work=None) == rlib.ERR_ARG and call(state=None) == rlib.ERR_ARG
        assert call(e=a + 4) == rlib.ERR_ARG and call(work=a + 8) == rlib.ERR_ARG and call(state=a + 4) == rlib.ERR_ARG
        assert call(B=0) == rlib.ERR_ARG and call(Umax=-1) == rlib.ERR_ARG
        assert call(blank=V) == rlib.ERR_ARG and call(blank=-1) == rlib.ERR_ARG
        assert call(V=18) == rlib.ERR_SHAPE and call(V=420) == rlib.ERR_SHAPE
        assert call(Umax=256, y=wide_y, tl=wide_tl) == rlib.ERR_SHAPE
        assert call(wb=work - 1) == rlib.ERR_SHAPE and call(sb=state - 1) == rlib.ERR_SHAPE
    assert fwd(nll=None) == rlib.ERR_ARG and bwd(rs=None) == rlib.ERR_ARG and bwd(db=None) == rlib.ERR_ARG and bwd(rs=a + 4) == rlib.ERR_ARG
    for kw in ({"ll": np.array([6, 5], np.int32)}, {"ll": np.array([0, 5], np.int32)}, {"tl": np.array([3, 0], np.int32)}, {"tl": np.array([0, -1], np.int32)},
               {"y": np.array([[1, blank], [3, 4]], np.int32)}, {"y": np.array([[1, V], [3, 4]], np.int32)}, {"y": np.array([[-1, 2], [3, 4]], np.int32)}):
        assert fwd(**kw) == rlib.ERR_ARG, kw
    assert not buf.any()


def test_host_twin_and_function_refusals():
    e, p, w, b, y, ll, tl, blank = C.case("v20")
    for kw, status in (({"ll": [6, 5]}, rlib.ERR_ARG), ({"tl": [3, 0]}, rlib.ERR_ARG), ({"blank": 20}, rlib.ERR_ARG), ({"y": np.full_like(y, blank)}, rlib.ERR_ARG)):
        with pytest.raises(RnntError) as err:
            rlib.joint_loss_host(e, p, w, b, kw.get("y", y), kw.get("ll", ll), kw.get("tl", tl), kw.get("blank", blank), row_scale=np.ones(2))
        assert err.value.status == status, kw
    with pytest.raises(RnntError) as err:
        rlib.joint_loss_host(e, p, w[:18], b[:18], y, ll, tl, blank)
    assert err.value.status == rlib.ERR_SHAPE
    leaves = [torch.from_numpy(a) for a in (e, p, w, b)]
    rest = (torch.from_numpy(y), torch.from_numpy(ll), torch.from_numpy(tl))
    with pytest.raises(TypeError):
        transducer_joint_loss(leaves[0].double(), *leaves[1:], *rest)
    with pytest.raises(TypeError):
        transducer_joint_loss(*leaves[:3], leaves[3].half(), *rest)
    with pytest.raises(ValueError):
        transducer_joint_loss(*leaves, *rest, reduction="batchmean")
    for args in ((leaves[0][:, :, :128], *leaves[1:], *rest), (*leaves, rest[0][:, :1], *rest[1:]), (*leaves, rest[0], torch.tensor([6, 5]), rest[2])):
        with pytest.raises(RnntError) as err:
            transducer_joint_loss(*args)
        assert err.value.status == rlib.ERR_ARG
    with pytest.raises(RnntError) as err:
        transducer_joint_loss(leaves[0], leaves[1], leaves[2][:18], leaves[3][:18], *rest)
    assert err.value.status == rlib.ERR_SHAPE
