"""An encoder layer's attention core with gradients, without a GPU: rnnt_rel_attention_host (the plain C++ float64 twin of both
directions) against float64 torch autograd of the formula, testing.chunk_visible against a loop restatement of the reference's mask,
ctc_vr_amd.functional.rel_attention on CPU tensors, RelPositionMultiHeadedAttention against the reference's golden vectors, the
workspace formula, every refusal with its status, and the sanity of the yardstick the device tests use."""
import ctypes

import numpy as np
import pytest
import torch

import attention_grad_cases as C
import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from conftest import load_golden
from ctc_vr_amd.functional import RelPositionMultiHeadedAttention, rel_attention
from ctc_vr_amd.lib import RnntError

REC_RTOL = 1e-9                   # the project's bar for f64 code against its float64 restatement (test_rnnt_loss_cpu.py)
F32 = 2.0 ** -24                  # one rounding to float32, relative
GOLDEN_TOL = 1e-6                 # absolute: the reference casts its scores to float32 inside forward_attention
YARD_REL = 1e-3                   # the emulation may stand at most this far from float64, relative to max |reference|
WEIGHTS = ("linear_q.weight", "linear_k.weight", "linear_v.weight", "linear_out.weight", "linear_pos.weight")
SMALL = ("linear_q.bias", "linear_k.bias", "linear_v.bias", "linear_out.bias", "pos_bias_u", "pos_bias_v")


def _close(got, want, what, rel=0.0):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = REC_RTOL * np.maximum(1.0, np.abs(want)) + rel * np.abs(want)
    assert (err <= bound).all(), f"{what}: max error {err.max():.3e}"


def _head(a):
    return a["q"], a["k"], a["v"], a["p"], a["u"], a["vb"]


def _nan_padding(a, lens):
    """k and v with NaN at j >= len_b: what lies there is never read"""
    k, v = a["k"].copy(), a["v"].copy()
    for i, n in enumerate(lens):
        k[i, n:] = np.nan
        v[i, n:] = np.nan
    return k, v


@pytest.mark.parametrize("name,scale", C.CASES)
def test_host_twin_vs_float64_autograd(name, scale):
    a = C.inputs(name, scale)
    lens, chunk, left = C.mask(name)
    got = rlib.rel_attention_host(*_head(a), lens, chunk, left, dout=a["dout"])
    for what, g, w in zip(C.NAMES, got, C.reference(name, scale)):
        assert g.dtype == np.float64 and g.shape == w.shape and np.isfinite(g).all(), what
        _close(g, w, f"{name} x{scale:g} {what}")
    fwd = rlib.rel_attention_host(*_head(a), lens, chunk, left)    # forward only: the same out, nothing else
    assert len(fwd) == 1 and np.array_equal(fwd[0], got[0])


def _visible_loops(T_, lens, chunk, left):
    """subsequent_chunk_mask (wenet/utils/mask.py:88-123) & ~make_pad_mask(lengths), restated as plain loops"""
    vis = np.zeros((len(lens), T_, T_), bool)
    for b, n in enumerate(lens):
        for i in range(T_):
            start, ending = 0, T_
            if chunk > 0:
                if left >= 0:
                    start = max((i // chunk - left) * chunk, 0)
                ending = min((i // chunk + 1) * chunk, T_)
            for j in range(start, ending):
                vis[b, i, j] = j < n
    return vis


@pytest.mark.parametrize("name", list(C.SHAPES))
def test_chunk_visible_vs_the_mask_loops(name):
    B, T_, _, chunk, left = C.SHAPES[name]
    lens = C.mask(name)[0]
    lens = np.full(B, T_) if lens is None else lens
    got = T.chunk_visible(T_, lens, chunk, left)
    assert got.dtype == bool and got.shape == (B, T_, T_) and np.array_equal(got, _visible_loops(T_, lens, chunk, left))
    if name == "dead":                                             # the case is there for its rows without a visible key
        assert int((~got.any(-1)).sum()) == 6
    assert np.array_equal(T.chunk_visible(T_, None, chunk, left), _visible_loops(T_, [T_], chunk, left))


def test_one_key_gives_exact_zeros():
    for scale in C.SCALES:
        a = C.inputs("one", scale)
        out, dq, dk, dv, dp, du, dvb = rlib.rel_attention_host(*_head(a), dout=a["dout"])
        assert np.array_equal(out, a["v"].astype(np.float64)) and np.array_equal(dv, a["dout"].astype(np.float64))
        for what, g in zip(("dq", "dk", "dp", "du", "dvb"), (dq, dk, dp, du, dvb)):
            assert not g.any(), f"{what} is not exactly 0"


@pytest.mark.parametrize("name", ["dead", "c16", "c25", "work"])
def test_hidden_keys_and_values_are_never_read(name):
    a = C.inputs(name, 1.0)
    lens, chunk, left = C.mask(name)
    k, v = _nan_padding(a, lens)
    live = (np.arange(k.shape[1])[None, :] < lens[:, None])[..., None]
    z = np.float32(0.0)
    got = rlib.rel_attention_host(a["q"], k, v, a["p"], a["u"], a["vb"], lens, chunk, left, dout=a["dout"])
    ref0 = rlib.rel_attention_host(a["q"], np.where(live, a["k"], z), np.where(live, a["v"], z), a["p"], a["u"], a["vb"], lens, chunk, left, dout=a["dout"])
    for what, g, w in zip(C.NAMES, got, ref0):
        assert np.isfinite(g).all(), f"{what}: padding was read"
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), f"{what}: NaN padding and zero padding differ"
    for i, n in enumerate(lens):
        assert not got[2][i, n:].any() and not got[3][i, n:].any(), "dk and dv at hidden keys are exactly 0"
    if name == "dead":                                             # rows without a visible key: out = 0, dq = 0
        dead = ~T.chunk_visible(k.shape[1], lens, chunk, left).any(-1)
        assert dead.sum() == 6 and not got[0][dead].any() and not got[1][dead].any()


def test_yardstick_sanity():
    """Per scale and output, E (the emulation's largest distance from float64 over the cases) is at most 1e-3 of max |reference|, so a
    broken emulation cannot widen the device's tolerance; and it is not 0, so it measures something."""
    E, R = C.yardstick(), C.reference_scale()
    for scale in C.SCALES:
        print(f"scale {scale:g}: " + ", ".join(f"E_{x} = {E[scale][x]:.3e} ({E[scale][x] / R[scale][x]:.1e} of {R[scale][x]:.3g})" for x in C.NAMES))
        for x in C.NAMES:
            assert 0.0 < E[scale][x] <= YARD_REL * R[scale][x], f"E_{x} = {E[scale][x]} at scale {scale:g}, max |reference| = {R[scale][x]}"


@pytest.mark.parametrize("name", ["one", "dead", "c16"])
def test_rel_attention_on_cpu_tensors_with_an_upstream_gradient(name):
    a = C.inputs(name, 1.0)
    lens, chunk, left = C.mask(name)
    leaves = [torch.from_numpy(v).requires_grad_(True) for v in _head(a)]
    out = rel_attention(*leaves, lengths=None if lens is None else torch.from_numpy(lens), chunk_size=chunk, num_left_chunks=left)
    want = C.reference(name, 1.0)
    assert out.dtype == torch.float32 and out.requires_grad
    _close(out.detach().numpy(), want[0], "out", rel=F32)
    out.backward(torch.from_numpy(a["dout"]))
    for what, t, ref in zip(C.NAMES[1:], leaves, want[1:]):
        assert t.grad is not None and t.grad.dtype == torch.float32 and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all()), what
        _close(t.grad.numpy(), ref, what, rel=F32)                 # the twin's float64, rounded once


def _module(g=None):
    m = RelPositionMultiHeadedAttention(4, 256, 0.0)
    if g is not None:
        m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}, strict=True)
    return m


def test_module_has_the_reference_parameter_names():
    m = _module()
    want = {n: (256, 256) for n in WEIGHTS}
    want.update({n: (256,) for n in SMALL[:4]})
    want.update({"pos_bias_u": (4, 64), "pos_bias_v": (4, 64)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    for args in ((8, 256, 0.0), (4, 512, 0.0), (4, 256, 0.1)):
        with pytest.raises(RnntError) as err:
            RelPositionMultiHeadedAttention(*args)
        assert err.value.status == rlib.ERR_SHAPE, args
    with pytest.raises(RnntError) as err:
        m(torch.zeros(2, 5, 256), torch.zeros(2, 5, 256))
    assert err.value.status == rlib.ERR_ARG


def test_module_vs_the_reference_golden():
    """tests/golden/attention_ref.npz (gen_attention_golden.py): the reference module in float64 eval mode with the mask of
    subsequent_chunk_mask & ~make_pad_mask, forward and the gradients of (out * dout).sum(), for dead-, c16- and causal-like shapes.
    The module here runs the float64 host twin on float32 tensors behind float32 Linears, and the reference casts its scores to
    float32 inside forward_attention, so the two part near float32 rounding; everything is held to 1e-6 absolute.  The fixture holds
    out and dx rounded to float32, the small gradients whole, and of each [256, 256] weight gradient G three rows, all row and column
    sums, and G r and l G for two seeded sign vectors (the fixture's size limit; every element enters one sum and one projection of
    each kind, errors that cancel in a plain sum do not cancel under random signs, and all are held to the same 1e-6).

    Measured (largest absolute distance, cases dead / c16 / causal): out 3.1e-07 / 1.5e-07 / 2.7e-07; dx 7.5e-08 / 1.9e-08 / 5.2e-08;
    bias and pos_bias gradients 5.9e-08 / 1.3e-07 / 7.3e-08; weight-gradient rows 3.9e-08 / 5.6e-08 / 4.8e-08; row and column sums
    5.0e-07 / 6.6e-07 / 3.7e-07; sign projections 3.8e-07 / 7.3e-07 / 4.0e-07."""
    g = load_golden("attention_ref.npz")
    m = _module(g).eval()
    pr, pl = g["proj.r"].astype(np.float64), g["proj.l"].astype(np.float64)
    for ci in range(3):
        c = f"c{ci}."
        x = torch.from_numpy(g[c + "x"]).requires_grad_(True)
        chunk, left = (int(v) for v in g[c + "args"])
        m.zero_grad()
        out = m(x, torch.from_numpy(g[c + "pos_emb"]), torch.from_numpy(g[c + "lengths"]), chunk, left)
        out.backward(torch.from_numpy(g[c + "dout"]))
        grads = {n: p.grad.numpy().astype(np.float64) for n, p in m.named_parameters()}
        err = {"out": np.abs(out.detach().numpy().astype(np.float64) - g[c + "out"]).max(), "dx": np.abs(x.grad.numpy().astype(np.float64) - g[c + "dx"]).max(),
               "small": max(np.abs(grads[n] - g[f"{c}g.{n}"]).max() for n in SMALL),
               "rows": max(np.abs(grads[n][[0, 96, 192]] - g[f"{c}g.{n}.rows"]).max() for n in WEIGHTS),
               "sums": max(max(np.abs(grads[n].sum(1) - g[f"{c}g.{n}.rowsum"]).max(), np.abs(grads[n].sum(0) - g[f"{c}g.{n}.colsum"]).max()) for n in WEIGHTS),
               "proj": max(max(np.abs(grads[n] @ pr - g[f"{c}g.{n}.proj_r"]).max(), np.abs(pl @ grads[n] - g[f"{c}g.{n}.proj_l"]).max()) for n in WEIGHTS)}
        print(f"case {ci} (B x T {tuple(x.shape[:2])}, chunk {chunk}, left {left}): " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
        for k, v in err.items():
            assert v <= GOLDEN_TOL, f"case {ci} {k}: {v:.3e}"


def _workspace_formula(B, T_):
    return 4 * (4 * ((B + 3) // 4) + 260 * B * T_ + 512 * B * ((T_ + 15) // 16)), 16 * B * T_


def test_workspace_formula_and_refusals():
    for B, T_ in ((1, 1), (3, 13), (2, 249), (64, 249), (5, 4096)):
        assert rlib.rel_attention_workspace(B, T_) == _workspace_formula(B, T_), (B, T_)
    lib = rlib.load()
    wb, sb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for args, status in (((0, 1), rlib.ERR_ARG), ((1, 0), rlib.ERR_ARG), ((1, 4097), rlib.ERR_SHAPE), ((2048, 4096), rlib.ERR_SHAPE)):
        assert lib.rnnt_rel_attention_workspace(*args, ctypes.byref(wb), ctypes.byref(sb)) == status and wb.value == -7 and sb.value == -7, args
    assert rlib.rel_attention_workspace(1, 2048)[1] == 16 * 2048   # the cap on T is at least 2048
    assert lib.rnnt_rel_attention_workspace(1, 1, None, ctypes.byref(sb)) == rlib.ERR_ARG
    assert lib.rnnt_rel_attention_workspace(1, 1, ctypes.byref(wb), None) == rlib.ERR_ARG


def test_host_twin_refusals_write_nothing():
    a = C.inputs("dead", 1.0)
    B, T_ = a["q"].shape[:2]
    outs = [np.full(s, 7.0) for s in ((B, T_, 256),) * 4 + ((T_, 256), (4, 64), (4, 64))]
    lib = rlib.load()
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    ptr, optr = [p(v) for v in _head(a)], [p(v) for v in outs]
    i32 = lambda v: p(np.array(v, np.int32))

    def call(ptr=ptr, lens=None, B=B, T_=T_, chunk=4, left=1, dout=p(a["dout"]), optr=optr):
        return lib.rnnt_rel_attention_host(*ptr, lens, B, T_, chunk, left, dout, *optr)

    assert call(B=0) == rlib.ERR_ARG and call(T_=0) == rlib.ERR_ARG and call(chunk=0, left=0) == rlib.ERR_ARG and call(chunk=-1, left=2) == rlib.ERR_ARG
    assert call(T_=4097) == rlib.ERR_SHAPE and call(B=2048, T_=4096) == rlib.ERR_SHAPE
    for lens in ([14, 5, 1], [13, 0, 1], [13, 5, -1]):
        assert call(lens=i32(lens)) == rlib.ERR_ARG, lens
    for k in range(6):
        assert call(ptr=[None if i == k else q for i, q in enumerate(ptr)]) == rlib.ERR_ARG
    for k in range(7):                                             # out, and with dout the six gradients
        assert call(optr=[None if i == k else q for i, q in enumerate(optr)]) == rlib.ERR_ARG
    assert all((v == 7.0).all() for v in outs)
    assert call(lens=i32([13, 5, 1])) == 0                         # and an accepted call writes every element
    assert not any((v == 7.0).any() for v in outs)
    with pytest.raises(RnntError) as err:
        rlib.rel_attention_host(*_head(a), [13, 5], 4, 1)
    assert err.value.status == rlib.ERR_ARG


def test_device_entries_refuse_on_the_host_before_any_launch():
    """null, misaligned, out-of-range and short-buffer calls are decided before the first HIP call: they need no GPU and touch nothing"""
    lib = rlib.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data % 16)                  # a 16-byte aligned (host) address: never followed
    wbytes, sbytes = rlib.rel_attention_workspace(3, 13)
    long_, zero = (np.array(v, np.int32) for v in ([14, 5, 1], [13, 0, 1]))
    lp = lambda v: v.ctypes.data_as(ctypes.c_void_p)

    def fwd(**k):
        return lib.rnnt_rel_attention_forward(k.get("q", a), a, k.get("v", a), a, a, k.get("vb", a), k.get("lens"), k.get("B", 3), k.get("T", 13), k.get("chunk", 4),
                                              k.get("left", 1), k.get("out", a), k.get("state", a), k.get("sb", sbytes), k.get("work", a), k.get("wb", wbytes), None)

    def bwd(**k):
        return lib.rnnt_rel_attention_backward(k.get("q", a), a, k.get("v", a), a, a, k.get("vb", a), k.get("out", a), k.get("state", a), k.get("sb", sbytes), a,
                                               k.get("lens"), k.get("B", 3), k.get("T", 13), k.get("chunk", 4), k.get("left", 1), a, a, a, k.get("dp", a), a, a,
                                               k.get("work", a), k.get("wb", wbytes), None)

    for call in (fwd, bwd):
        assert call(q=None) == rlib.ERR_ARG and call(vb=None) == rlib.ERR_ARG and call(out=None) == rlib.ERR_ARG and call(work=None) == rlib.ERR_ARG
        assert call(q=a + 4) == rlib.ERR_ARG and call(v=a + 8) == rlib.ERR_ARG and call(work=a + 8) == rlib.ERR_ARG and call(state=a + 4) == rlib.ERR_ARG
        assert call(B=0) == rlib.ERR_ARG and call(T=0) == rlib.ERR_ARG and call(lens=lp(long_)) == rlib.ERR_ARG and call(lens=lp(zero)) == rlib.ERR_ARG
        assert call(chunk=0, left=0) == rlib.ERR_ARG and call(chunk=-3, left=1) == rlib.ERR_ARG
        assert call(T=4097) == rlib.ERR_SHAPE and call(B=2048, T=4096) == rlib.ERR_SHAPE
        assert call(wb=wbytes - 1) == rlib.ERR_SHAPE and call(sb=sbytes - 1) == rlib.ERR_SHAPE
    assert bwd(state=None) == rlib.ERR_ARG and bwd(dp=None) == rlib.ERR_ARG and bwd(dp=a + 4) == rlib.ERR_ARG
    assert not buf.any()


def test_rel_attention_argument_errors():
    a = C.inputs("dead", 1.0)
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    names = ("q", "k", "v", "p", "pos_bias_u", "pos_bias_v")
    args = [t[k] for k in ("q", "k", "v", "p", "u", "vb")]
    for k in range(6):
        for cast in (torch.Tensor.double, torch.Tensor.half):
            with pytest.raises(TypeError):
                rel_attention(*(cast(v) if i == k else v for i, v in enumerate(args)))
    with pytest.raises(TypeError):
        rel_attention(args[0].numpy(), *args[1:])
    bad = ({"q": t["q"][:, :, :128]}, {"q": t["q"][0]}, {"k": t["k"][:2]}, {"v": t["v"][:, :12]}, {"p": t["p"][:12]}, {"pos_bias_u": t["u"].reshape(256)},
           {"pos_bias_v": t["vb"][:2]}, {"lengths": torch.tensor([13, 5])}, {"lengths": torch.tensor([14, 5, 1])}, {"lengths": torch.tensor([13, 0, 1])},
           {"num_left_chunks": 0}, {"chunk_size": -1, "num_left_chunks": 3})
    for kw in bad:
        call = dict(zip(names, args))
        call.update(kw)
        with pytest.raises(RnntError) as err:
            rel_attention(**call)
        assert err.value.status == rlib.ERR_ARG, list(kw)
    with pytest.raises(RnntError) as err:
        rel_attention(*(torch.zeros(1, 4097, 256),) * 3, torch.zeros(4097, 256), *args[4:])
    assert err.value.status == rlib.ERR_SHAPE
    # a non-contiguous q (a slice of a fused qkv tensor) is the contiguous call
    qkv = torch.cat([t["q"], t["k"], t["v"]], dim=2)
    got = rel_attention(qkv[..., :256], qkv[..., 256:512], qkv[..., 512:], *args[3:], lengths=[13, 5, 1], chunk_size=4, num_left_chunks=1)
    assert torch.equal(got, rel_attention(*args, lengths=[13, 5, 1], chunk_size=4, num_left_chunks=1))
