"""The joint lattice with gradients, without a GPU: rnnt_joint_lattice_backward_host (the plain C++ float64 twin of the device
entry) against float64 torch autograd of the eager formula, ctc_vr_amd.functional.transducer_joint on CPU tensors (an upstream
gradient, the chain into rnnt_loss, lengths, what it saves), TransducerJoint's parameter names, the workspace formula and every
refusal with its status."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
import joint_grad_cases as C
from ctc_vr_amd.functional import TransducerJoint, rnnt_loss, transducer_joint
from ctc_vr_amd.layout import state_dict_spec
from ctc_vr_amd.lib import RnntError

REC_RTOL = 1e-9                   # the project's bar for f64 code against its float64 restatement (test_rnnt_loss_cpu.py)
F32 = 2.0 ** -24                  # one rounding to float32, relative


def _close(got, want, what, rel=0.0):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = REC_RTOL * np.maximum(1.0, np.abs(want)) + rel * np.abs(want)
    assert (err <= bound).all(), f"{what}: max error {err.max():.3e}"


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("name,scale", C.CASES)
def test_host_twin_vs_float64_autograd(name, scale, with_lens):
    e, p, w, _, g = C.inputs(name, scale)
    ll, tl = C.rows(name) if with_lens else (None, None)
    if with_lens:                                                  # what lies outside the lengths is never read
        g = np.where(T.joint_live_cells(*g.shape[:3], ll, tl)[..., None], g, np.float32("nan")).astype(np.float32)
        for i in range(len(ll)):
            e[i, ll[i]:] = np.nan
            p[i, tl[i] + 1:] = np.nan
    got = rlib.joint_lattice_backward_host(e, p, w, g, ll, tl)
    for x, a, want in zip(C.NAMES, got, C.reference(name, scale, with_lens)):
        assert a.dtype == np.float64 and np.isfinite(a).all()
        _close(a, want, f"{name} x{scale:g} {x}")
    if scale == 30.0:                                              # tanh(+-40) = +-1 in float64 too: those dz are exactly 0
        with np.errstate(invalid="ignore"):
            sat = (np.abs(e[:, :, None, :].astype(np.float64) + p[:, None, :, :]) > 40.0).all(axis=2)
        assert (sat.any() or name != "one") and not got[0][sat].any()


def _leaves(name, scale=1.0):
    e, p, w, b, g = C.inputs(name, scale)
    return [torch.from_numpy(a).requires_grad_(True) for a in (e, p, w, b)], g


@pytest.mark.parametrize("name", ["one", "ragged", "u28", "v20"])
def test_transducer_joint_on_cpu_tensors_with_an_upstream_gradient(name):
    leaves, g = _leaves(name)
    out = transducer_joint(*leaves)
    e, p, w, b = (t.detach().double() for t in leaves)
    want = torch.tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ w.T + b
    assert out.dtype == torch.float32 and out.shape == want.shape
    _close(out.detach().numpy(), want.numpy(), "logits", rel=F32)
    out.backward(torch.from_numpy(g))
    for x, t, ref in zip(C.NAMES, leaves, C.reference(name, 1.0, False)):
        assert t.grad.dtype == torch.float32
        _close(t.grad.numpy(), ref, x, rel=F32)                    # the twin's float64, rounded once
    # with lengths the incoming gradient's padding is never read
    leaves, _ = _leaves(name)
    ll, tl = C.rows(name)
    live = T.joint_live_cells(*g.shape[:3], ll, tl)[..., None]
    transducer_joint(*leaves, torch.from_numpy(ll), torch.from_numpy(tl)).backward(torch.from_numpy(np.where(live, g, np.float32("nan")).astype(np.float32)))
    for x, t, ref in zip(C.NAMES, leaves, C.reference(name, 1.0, True)):
        _close(t.grad.numpy(), ref, x + " with lengths", rel=F32)


def _chain_case(name):
    B, Tn, U1, V, _ = C.SHAPES[name]
    ll, tl = C.rows(name)
    r = np.random.Generator(np.random.Philox(key=[78, sorted(C.SHAPES).index(name)]))
    blank = 5
    lab = r.integers(0, V - 1, (B, U1 - 1))
    return ll, tl, np.where(lab >= blank, lab + 1, lab).astype(np.int32), blank


def _chain_f64(e, p, w, b, y, ll, tl, blank, store):
    """The chain in float64 numpy / torch: logits, d mean(nll) / d logits through transducer_loss_ref, the joint's gradients.  `store`
    is applied wherever the CPU path stores a tensor (its float32 lattice, its float32 lattice gradient, its float32 results)."""
    logits = store((torch.tanh(torch.from_numpy(e).double().unsqueeze(2) + torch.from_numpy(p).double().unsqueeze(1)) @ torch.from_numpy(w).double().T
                    + torch.from_numpy(b).double()).numpy())
    B = len(ll)
    rows = [T.transducer_loss_ref(logits[i], y[i], int(ll[i]), int(tl[i]), blank) for i in range(B)]
    g = store(store(np.stack([r[1] for r in rows])) * store(np.float64(1.0 / B)))       # the saved gradient, then times d mean / d nll_b
    return float(np.mean([r[0] for r in rows])), [store(a) for a in T.joint_backward_ref(e, p, w, g, ll, tl)]


@pytest.mark.parametrize("name", ["ragged", "u28"])
def test_chain_into_rnnt_loss_on_cpu_tensors(name):
    """rnnt_loss(transducer_joint(...)).backward() on CPU tensors against the float64 chain.  The CPU path computes in float64 and
    stores float32 between its stages; E is what exactly those roundings cost (the same float64 chain with each stored tensor
    rounded to float32), measured here, and the path is held to 8 E per output: another order of the same roundings."""
    leaves, _ = _leaves(name)
    e, p, w, b = (t.detach().numpy() for t in leaves)
    ll, tl, y, blank = _chain_case(name)
    want_loss, want = _chain_f64(e, p, w, b, y, ll, tl, blank, lambda a: a)
    _, rounded = _chain_f64(e, p, w, b, y, ll, tl, blank, lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64))
    lens = (torch.from_numpy(ll), torch.from_numpy(tl))
    loss = rnnt_loss(transducer_joint(*leaves, *lens), torch.from_numpy(y), *lens, blank=blank, reduction="mean")
    loss.backward()
    assert abs(float(loss.detach()) - want_loss) <= 1e-6 * abs(want_loss)      # float32 lattice and float32 loss: a few 2^-24
    for x, t, ref, rnd in zip(C.NAMES, leaves, want, rounded):
        E = float(np.abs(rnd - ref).max())
        err = float(np.abs(t.grad.numpy() - ref).max())
        print(f"{name} {x}: E = {E:.3e}, chain error {err:.3e} = {err / E:.2f} E")
        assert E > 0.0 and err <= 8.0 * E


def test_transducer_joint_saves_only_its_four_inputs():
    B, Tn, U1, V, _ = C.SHAPES["u28"]
    leaves, _ = _leaves("u28")
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        transducer_joint(*leaves)
    assert len(saved) == 4 and all(any(s.data_ptr() == t.data_ptr() for t in leaves) for s in saved)
    assert max(s.numel() for s in saved) <= max(B * Tn, B * U1, V) * 256


def test_module_has_the_reference_joint_parameter_names():
    V = 412
    m = TransducerJoint(V, 256, 256)
    want = {n[len("joint."):]: tuple(shape) for n, shape, _ in state_dict_spec(V) if n.startswith("joint.")}
    assert want and {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    sd = T.make_state_dict(0)
    m.load_state_dict({k: torch.from_numpy(sd["joint." + k]) for k in want})      # the reference's joint.* entries load as they are
    enc, pred = torch.randn(2, 3, 256), torch.randn(2, 4, 256)
    out = m(enc, pred)
    ref = torch.tanh(m.enc_ffn(enc).double().unsqueeze(2) + m.pred_ffn(pred).double().unsqueeze(1)) @ m.ffn_out.weight.double().T + m.ffn_out.bias.double()
    _close(out.detach().numpy(), ref.detach().numpy(), "module forward", rel=F32)
    out.sum().backward()
    assert all(prm.grad is not None and bool(torch.isfinite(prm.grad).all()) for prm in m.parameters())
    with pytest.raises(RnntError):
        TransducerJoint(V, 256, 256, join_dim=320)


def _workspace_formula(B, Tn, U1, V):
    """include/rnnt_hip.h, restated"""
    cdiv = lambda a, b: -(-a // b)
    M = B * Tn * U1
    NUB = cdiv(U1, 16)
    TC = 4 * cdiv(cdiv(Tn, max(1, 512 // (B * NUB))), 4)
    NC = cdiv(Tn, TC)
    CS = 32 * cdiv(cdiv(M, 32), max(1, 512 // cdiv(V, 64)))
    NS = cdiv(M, CS)
    return 425984 + 4 * max(256 * B * (Tn + U1) + 4, 4 * cdiv(B, 2) + 256 * (NUB * B * Tn + NC * B * U1 + NS * V) + NS * V)


def test_workspace_formula_and_refusals():
    for B, Tn, U1, V in [s[:4] for s in C.SHAPES.values()] + [(16, 249, 28, 412), (64, 249, 28, 412), (1, 2000, 300, 416), (700, 3, 17, 8)]:
        assert rlib.joint_lattice_workspace(B, Tn, U1, V) == _workspace_formula(B, Tn, U1, V), (B, Tn, U1, V)
    n = ctypes.c_int64(-7)
    lib = rlib.load()
    for args, status in (((0, 1, 1, 4), rlib.ERR_ARG), ((1, 0, 1, 4), rlib.ERR_ARG), ((1, 1, 0, 4), rlib.ERR_ARG), ((1, 1, 1, 0), rlib.ERR_SHAPE),
                         ((1, 1, 1, 18), rlib.ERR_SHAPE), ((1, 1, 1, 420), rlib.ERR_SHAPE), ((1300, 1300, 1300, 412), rlib.ERR_SHAPE)):
        assert lib.rnnt_joint_lattice_workspace(*args, ctypes.byref(n)) == status and n.value == -7, args
    assert lib.rnnt_joint_lattice_workspace(1, 1, 1, 4, None) == rlib.ERR_ARG


def test_host_twin_refusals_write_nothing():
    e, p, w, _, g = C.inputs("v20", 1.0)
    B, Tn, U1, V = g.shape
    outs = tuple(np.full(s, 7.0) for s in ((B, Tn, 256), (B, U1, 256), (V, 256), (V,)))
    for kw, status in (({"logit_lens": [6, 5]}, rlib.ERR_ARG), ({"logit_lens": [0, 5]}, rlib.ERR_ARG), ({"target_lens": [3, 0]}, rlib.ERR_ARG),
                       ({"target_lens": [0, -1]}, rlib.ERR_ARG)):
        with pytest.raises(RnntError) as err:
            rlib.joint_lattice_backward_host(e, p, w, g, out=outs, **kw)
        assert err.value.status == status, kw
    with pytest.raises(RnntError) as err:                          # V = 18
        rlib.joint_lattice_backward_host(e, p, w[:18], g[..., :18], out=outs)
    assert err.value.status == rlib.ERR_SHAPE
    lib = rlib.load()
    ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (e, p, w, g)]
    optr = [a.ctypes.data_as(ctypes.c_void_p) for a in outs]
    assert lib.rnnt_joint_lattice_backward_host(*ptr, None, None, 0, Tn, U1, V, *optr) == rlib.ERR_ARG
    assert lib.rnnt_joint_lattice_backward_host(*ptr, None, None, B, Tn, U1, 420, *optr) == rlib.ERR_SHAPE
    assert lib.rnnt_joint_lattice_backward_host(*ptr, None, None, 1300, 1300, 1300, V, *optr) == rlib.ERR_SHAPE
    for k in range(4):
        assert lib.rnnt_joint_lattice_backward_host(*(None if i == k else q for i, q in enumerate(ptr)), None, None, B, Tn, U1, V, *optr) == rlib.ERR_ARG
        assert lib.rnnt_joint_lattice_backward_host(*ptr, None, None, B, Tn, U1, V, *(None if i == k else q for i, q in enumerate(optr))) == rlib.ERR_ARG
    assert all((a == 7.0).all() for a in outs)
    rlib.joint_lattice_backward_host(e, p, w, g, out=outs)         # and an accepted call writes every element
    assert not any((a == 7.0).any() for a in outs)


def test_device_entries_refuse_on_the_host_before_any_launch():
    """null, misaligned, out-of-range and short-workspace calls are decided before the first HIP call: they need no GPU and touch nothing"""
    lib = rlib.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data % 16)                  # a 16-byte aligned (host) address: never followed
    need = rlib.joint_lattice_workspace(2, 5, 3, 20)
    fwd = lambda **k: lib.rnnt_joint_lattice_forward(k.get("e", a), a, a, a, k.get("B", 2), 5, 3, k.get("V", 20), a, k.get("work", a), k.get("nb", need), None)
    bwd = lambda **k: lib.rnnt_joint_lattice_backward(k.get("e", a), a, a, a, k.get("ll"), None, k.get("B", 2), 5, 3, k.get("V", 20), a, a, a, a,
                                                      k.get("work", a), k.get("nb", need), None)
    six = np.array([6, 5], np.int32)
    for call in (fwd, bwd):
        assert call(e=None) == rlib.ERR_ARG and call(work=None) == rlib.ERR_ARG and call(e=a + 4) == rlib.ERR_ARG and call(work=a + 8) == rlib.ERR_ARG
        assert call(B=0) == rlib.ERR_ARG
        assert call(V=18) == rlib.ERR_SHAPE and call(V=420) == rlib.ERR_SHAPE and call(nb=need - 1) == rlib.ERR_SHAPE
    assert bwd(ll=six.ctypes.data_as(ctypes.c_void_p)) == rlib.ERR_ARG
    assert not buf.any()


def test_transducer_joint_argument_errors():
    leaves, _ = _leaves("v20")
    with pytest.raises(TypeError):
        transducer_joint(leaves[0].double(), *leaves[1:])
    with pytest.raises(TypeError):
        transducer_joint(leaves[0].half(), *leaves[1:])
    with pytest.raises(RnntError) as err:
        transducer_joint(leaves[0], leaves[1], leaves[2][:18], leaves[3][:18])
    assert err.value.status == rlib.ERR_SHAPE
    with pytest.raises(RnntError) as err:
        transducer_joint(*leaves, torch.tensor([6, 5]), None)
    assert err.value.status == rlib.ERR_ARG
    with pytest.raises(RnntError) as err:
        transducer_joint(leaves[0][:, :, :128], *leaves[1:])
    assert err.value.status == rlib.ERR_ARG
