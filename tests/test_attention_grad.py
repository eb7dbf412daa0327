"""An encoder layer's attention core with gradients on the device (rnnt_rel_attention_forward / _backward,
ctc_vr_amd.functional.rel_attention and RelPositionMultiHeadedAttention on CUDA tensors).  Needs a real MI355X: `pytest -m gpu`.

The yardstick is float64 torch autograd of the formula on the CPU (testing.rel_attention_ref).  The device owes float32 products
accumulated in float32, a float32 online softmax over tiles of 16 keys and float32 delta / ds, which is what
testing.rel_attention_emulation does on the CPU.  So the bound is measured, not chosen: per scale (1 and 3) and output, E is the
emulation's largest absolute distance from float64 over the cases of attention_grad_cases.py at that scale
(test_attention_grad_cpu.py holds E itself to 1e-3 of max |reference|), and the device is held to 8 E: the factor test_joint_grad.py
and test_lstm_grad.py use, for their reason -- another summation tree, and device exp / log within a couple of ulps."""
import numpy as np
import pytest
import torch

import attention_grad_cases as C
import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import RelPositionMultiHeadedAttention, rel_attention
from ctc_vr_amd.lib import RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GUARD = 64                        # floats behind every output, which no kernel may touch
SENTINEL = 12345.0
OUTS = C.NAMES                    # out, dq, dk, dv, dp, du, dvb
# The module chain on the device against float64: three float32 contraction stages forward (the Linears in, the attention, linear_out)
# and three backward, each a sum of at most 260 terms (256 features; B T = 260 rows for a weight gradient), so each stage is within
# 260 * 2^-24 = 1.6e-5 of its result's scale in the worst case; six stages: 9.3e-5, rounded to 1e-4 of max |reference| per tensor
# (of the cancelling terms' sum for linear_k.bias, whose gradient is 0 in exact arithmetic).
MODULE_REL = 1e-4


@pytest.fixture(scope="module")
def yardstick():
    E = C.yardstick()
    for scale in C.SCALES:
        print(f"emulation vs float64 at scale {scale:g}: " + ", ".join(f"E_{x} = {E[scale][x]:.3e}" for x in C.NAMES))
        for x in C.NAMES:
            assert E[scale][x] > 0.0
    return E


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(n):
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _run(a, mask, k=None, v=None, backward=True, with_state=True):
    """one rnnt_rel_attention_forward (+ _backward) through the raw lib calls into NaN-filled, guarded outputs:
    ({name: numpy}, lse [B, 4, T], guards intact)"""
    lens, chunk, left = mask
    B, Tn, D = a["q"].shape
    src = dict(a, k=a["k"] if k is None else k, v=a["v"] if v is None else v)
    dev = {n: torch.from_numpy(np.ascontiguousarray(x)).cuda() for n, x in src.items()}
    wbytes, sbytes = rlib.rel_attention_workspace(B, Tn)
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    shapes = dict(zip(OUTS, ((B, Tn, D),) * 4 + ((Tn, D), (4, 64), (4, 64))))
    names = OUTS if backward else OUTS[:1]
    buf = {n: _guarded(int(np.prod(shapes[n]))) for n in names}
    state = _guarded(sbytes // 4)
    s = torch.cuda.current_stream().cuda_stream
    head = [dev[n].data_ptr() for n in ("q", "k", "v", "p", "u", "vb")]
    rlib.rel_attention_forward_device(*head, lens, (B, Tn), chunk, left, buf["out"].data_ptr(), state.data_ptr() if with_state else None, sbytes,
                                      work.data_ptr(), wbytes, s)
    if backward:
        rlib.rel_attention_backward_device(*head, buf["out"].data_ptr(), state.data_ptr(), sbytes, dev["dout"].data_ptr(), lens, (B, Tn), chunk, left,
                                           *(buf[n].data_ptr() for n in OUTS[1:]), work.data_ptr(), wbytes, s)
    torch.cuda.synchronize()
    host = {n: x.cpu().numpy() for n, x in buf.items()}
    st = state.cpu().numpy()
    size = {n: int(np.prod(shapes[n])) for n in names}
    intact = all(bool((host[n][size[n]:] == np.float32(SENTINEL)).all()) for n in names) and bool((st[sbytes // 4:] == np.float32(SENTINEL)).all())
    return {n: host[n][:size[n]].reshape(shapes[n]) for n in names}, st[:sbytes // 4].reshape(B, 4, Tn), intact


def _ratios(got, want, E):
    return {x: float(np.abs(got[x] - w).max()) / E[x] for x, w in zip(C.NAMES, want)}


@pytest.mark.parametrize("name,scale", C.CASES)
def test_forward_and_backward_vs_float64(name, scale, yardstick):
    E = yardstick[scale]
    a, mask = C.inputs(name, scale), C.mask(name)
    got, lse, intact = _run(a, mask)
    assert intact, "something was written behind an output"
    for x in OUTS:
        assert np.isfinite(got[x]).all(), f"{x}: an element was not written (or is not finite)"
    ratios = _ratios(got, C.reference(name, scale), E)
    print(f"{name} x{scale:g}: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items()))
    again, lse2, _ = _run(a, mask)
    assert all(np.array_equal(_bits(got[x]), _bits(again[x])) for x in OUTS) and np.array_equal(_bits(lse), _bits(lse2)), "two calls on the same inputs differ"
    fwd, untouched, intact = _run(a, mask, backward=False, with_state=False)      # forward only (state = NULL): the same out, no state written
    assert intact and np.array_equal(_bits(got["out"]), _bits(fwd["out"])) and np.isnan(untouched).all()
    B, Tn = a["q"].shape[:2]
    vis = T.chunk_visible(Tn, np.full(B, Tn) if mask[0] is None else mask[0], mask[1], mask[2])
    dead = ~vis.any(-1)                                            # [B, T]: rows with no visible key carry the mark, the others a finite lse
    assert np.isposinf(lse[np.broadcast_to(dead[:, None], lse.shape)]).all() and np.isfinite(lse[np.broadcast_to(~dead[:, None], lse.shape)]).all()
    assert not got["out"][dead].any() and not got["dq"][dead].any()
    for x, r in ratios.items():
        assert r <= FACTOR, f"{x}: {r:.2f} E, the bound is {FACTOR:g} E"


@pytest.mark.parametrize("name", ["dead", "c16", "c25", "work"])
def test_hidden_keys_and_values_are_never_read(name):
    a, mask = C.inputs(name, 1.0), C.mask(name)
    lens = mask[0]
    live = (np.arange(a["k"].shape[1])[None, :] < lens[:, None])[..., None]
    nan, zero = np.float32("nan"), np.float32(0.0)
    got, _, intact = _run(a, mask, np.where(live, a["k"], nan).astype(np.float32), np.where(live, a["v"], nan).astype(np.float32))
    ref0, _, _ = _run(a, mask, np.where(live, a["k"], zero).astype(np.float32), np.where(live, a["v"], zero).astype(np.float32))
    assert intact
    for x in OUTS:
        assert np.isfinite(got[x]).all(), f"{x}: padding was read"
        assert np.array_equal(_bits(got[x]), _bits(ref0[x])), f"{x}: NaN padding and zero padding differ"
    for i, n in enumerate(lens):
        assert not got["dk"][i, n:].any() and not got["dv"][i, n:].any(), "dk and dv at hidden keys are exactly 0"


@pytest.mark.parametrize("name", ["dead", "c16"])
def test_rel_attention_on_cuda_and_cpu_tensors_agree(name, yardstick):
    E = yardstick[1.0]
    a, (lens, chunk, left) = C.inputs(name, 1.0), C.mask(name)

    def through(device):
        leaves = [torch.from_numpy(a[n]).to(device).requires_grad_(True) for n in ("q", "k", "v", "p", "u", "vb")]
        out = rel_attention(*leaves, lengths=torch.from_numpy(lens), chunk_size=chunk, num_left_chunks=left)
        out.backward(torch.from_numpy(a["dout"]).to(device))
        return [out.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in leaves]

    got, want = through("cuda"), through("cpu")
    raw, _, _ = _run(a, (lens, chunk, left))
    for x, g, w in zip(C.NAMES, got, want):
        assert np.array_equal(_bits(g), _bits(raw[x])), f"{x}: the autograd function and the raw calls differ"
        err = float(np.abs(g.astype(np.float64) - w).max())
        print(f"{name} {x}: |cuda - cpu| = {err:.3e} = {err / E[x]:.3f} E")
        assert err <= FACTOR * E[x], x


def test_rel_attention_saves_its_inputs_out_and_one_state_tensor():
    a, (lens, chunk, left) = C.inputs("c16", 1.0), C.mask("c16")
    B, Tn = a["q"].shape[:2]
    leaves = [torch.from_numpy(a[n]).cuda().requires_grad_(True) for n in ("q", "k", "v", "p", "u", "vb")]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        out = rel_attention(*leaves, lens, chunk, left)
    assert out.is_cuda and out.requires_grad
    assert len(saved) == 8 and all(any(s.data_ptr() == t.data_ptr() for s in saved) for t in leaves + [out])
    assert sum(s.dtype == torch.uint8 and s.numel() == 16 * B * Tn for s in saved) == 1       # the state: one log-sum-exp per (b, h, i)
    assert sum(s.numel() * s.element_size() for s in saved) < 8 * B * Tn * 256 * 4            # nothing of T x T size


def test_a_slice_of_a_fused_qkv_tensor_gives_the_contiguous_bits():
    a, (lens, chunk, left) = C.inputs("c16", 1.0), C.mask("c16")
    t = {n: torch.from_numpy(x).cuda() for n, x in a.items()}

    def through(q, k, v):
        leaves = [x.detach().requires_grad_(True) for x in (q, k, v, t["p"], t["u"], t["vb"])]
        out = rel_attention(*leaves, lens, chunk, left)
        out.backward(t["dout"])
        return [out.detach().cpu().numpy()] + [x.grad.cpu().numpy() for x in leaves]

    qkv = torch.cat([t["q"], t["k"], t["v"]], dim=2).requires_grad_(True)
    parts = (qkv[..., :256], qkv[..., 256:512], qkv[..., 512:])
    assert not parts[0].is_contiguous()
    out = rel_attention(*parts, t["p"], t["u"], t["vb"], lens, chunk, left)
    out.backward(t["dout"])
    want = through(t["q"], t["k"], t["v"])
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(want[0]))
    g = qkv.grad.cpu().numpy()
    for i, x in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(_bits(g[..., 256 * i:256 * (i + 1)]), _bits(want[1 + i])), x


def _attention64(q, k, v, p, u, vb, vis):
    """the formula in float64 torch, dense (vis [B, T, T] bool)"""
    B, Tn = q.shape[:2]
    hd = lambda x: x.view(x.shape[0], Tn, 4, 64).transpose(1, 2)
    qh, kh, vh, ph = hd(q), hd(k), hd(v), hd(p[None])
    s = ((qh + u[None, :, None]) @ kh.transpose(-1, -2) + (qh + vb[None, :, None]) @ ph.transpose(-1, -2)) / 8.0
    w = vis[:, None]
    m = s.detach().masked_fill(~w, -float("inf")).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(w, torch.exp(torch.where(w, s, m) - m), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    return ((e / torch.where(l > 0, l, torch.ones_like(l))) @ vh).transpose(1, 2).reshape(B, Tn, 256)


def test_module_on_the_device_vs_float64_on_the_cpu():
    B, Tn, lens, chunk, left = C.SHAPES["c25"]
    r = np.random.Generator(np.random.Philox(key=[310, 0]))
    x = torch.from_numpy(r.standard_normal((B, Tn, 256)).astype(np.float32))
    dout = torch.from_numpy((0.05 * r.standard_normal((B, Tn, 256))).astype(np.float32))
    pos_emb = torch.from_numpy(T.positional_table(Tn, 256))                      # [1, T, 256]
    torch.manual_seed(310)
    m = RelPositionMultiHeadedAttention(4, 256)
    m64 = RelPositionMultiHeadedAttention(4, 256).double()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()}, strict=True)
    x64 = x.double().requires_grad_(True)
    vis = torch.from_numpy(T.chunk_visible(Tn, lens, chunk, left))
    k64 = m64.linear_k(x64)
    k64.retain_grad()
    want_out = m64.linear_out(_attention64(m64.linear_q(x64), k64, m64.linear_v(x64), m64.linear_pos(pos_emb[0].double()), m64.pos_bias_u, m64.pos_bias_v, vis))
    want_out.backward(dout.double())
    want = {"out": want_out.detach().numpy(), "dx": x64.grad.numpy(), **{k: p.grad.numpy() for k, p in m64.named_parameters()}}
    # d linear_k.bias = sum over the rows of dk is 0 in exact arithmetic (a softmax does not see a shift of its keys: every row of ds
    # sums to 0), so its error has no result to be relative to: it is measured against the scale of the terms that cancel
    scales = {k: float(np.abs(w).max()) for k, w in want.items()}
    scales["linear_k.bias"] = float(k64.grad.abs().sum((0, 1)).max())
    md = m.cuda()
    xd = x.cuda().requires_grad_(True)
    out = md(xd, pos_emb.cuda(), torch.tensor(lens), chunk, left)
    out.backward(dout.cuda())
    got = {"out": out.detach().cpu().numpy(), "dx": xd.grad.cpu().numpy(), **{k: p.grad.cpu().numpy() for k, p in md.named_parameters()}}
    assert set(got) == set(want) and len(got) == 13
    for k, w in want.items():
        err, scale = float(np.abs(got[k] - w).max()), scales[k]
        print(f"{k}: |device - float64| = {err:.3e}, {err / scale:.1e} of its scale {scale:.3g}")
        assert np.isfinite(got[k]).all() and scale > 0 and err <= MODULE_REL * scale, k


def test_a_refusal_launches_nothing():
    a = C.inputs("dead", 1.0)
    B, Tn = a["q"].shape[:2]
    d = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    wbytes, sbytes = rlib.rel_attention_workspace(B, Tn)
    work = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")
    state = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), 7.0, device="cuda") for n in (B * Tn * 256,) * 4 + (Tn * 256, 256, 256)]
    p = [o.data_ptr() for o in outs]
    s = torch.cuda.current_stream().cuda_stream
    head = lambda q: [q] + [d[n].data_ptr() for n in ("k", "v", "p", "u", "vb")]

    def fwd(lens=None, shape=(B, Tn), chunk=4, left=1, wb=wbytes, sb=sbytes, q=d["q"].data_ptr()):
        rlib.rel_attention_forward_device(*head(q), lens, shape, chunk, left, p[0], state.data_ptr(), sb, work.data_ptr(), wb, s)

    def bwd(lens=None, shape=(B, Tn), chunk=4, left=1, wb=wbytes, sb=sbytes, q=d["q"].data_ptr()):
        rlib.rel_attention_backward_device(*head(q), p[0], state.data_ptr(), sb, d["dout"].data_ptr(), lens, shape, chunk, left, *p[1:], work.data_ptr(), wb, s)

    for call in (fwd, bwd):
        for kw, status in (({"lens": [14, 5, 1]}, rlib.ERR_ARG), ({"lens": [13, 0, 1]}, rlib.ERR_ARG), ({"q": d["q"].data_ptr() + 4}, rlib.ERR_ARG),
                           ({"q": None}, rlib.ERR_ARG), ({"shape": (0, Tn)}, rlib.ERR_ARG), ({"shape": (B, 0)}, rlib.ERR_ARG), ({"chunk": 0, "left": 0}, rlib.ERR_ARG),
                           ({"shape": (B, 4097)}, rlib.ERR_SHAPE), ({"wb": wbytes - 1}, rlib.ERR_SHAPE), ({"sb": sbytes - 1}, rlib.ERR_SHAPE)):
            with pytest.raises(RnntError) as err:
                call(**kw)
            assert err.value.status == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and not bool(work.any()) and not bool(state.any())
