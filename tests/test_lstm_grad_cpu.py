"""The predictor's LSTM with gradients, without a GPU: rnnt_lstm_host (the plain C++ float64 twin of both directions) against float64
torch autograd of the step loop, ctc_vr_amd.functional.lstm_predictor on CPU tensors, RNNPredictor against the reference's golden
vectors and against a torch stand-in through TransducerJoint.loss, the workspace formula and every refusal with its status."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
import lstm_grad_cases as C
from conftest import load_golden
from ctc_vr_amd.functional import RNNPredictor, TransducerJoint, lstm_predictor
from ctc_vr_amd.layout import state_dict_spec
from ctc_vr_amd.lib import RnntError

REC_RTOL = 1e-9                   # the project's bar for f64 code against its float64 restatement (test_rnnt_loss_cpu.py)
F32 = 2.0 ** -24                  # one rounding to float32, relative
GOLDEN_TOL = 1e-4                 # the bar test_predictor_and_joint_step_api holds the device to


def _close(got, want, what, rel=0.0):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = REC_RTOL * np.maximum(1.0, np.abs(want)) + rel * np.abs(want)
    assert (err <= bound).all(), f"{what}: max error {err.max():.3e}"


def _nan_padding(a, lens):
    """x and dout with NaN beyond every row's length: what lies there is never read"""
    x, dout = a["x"].copy(), a["dout"].copy()
    for i, n in enumerate(lens):
        x[i, n:] = np.nan
        dout[i, n:] = np.nan
    return x, dout


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("name,scale", C.CASES)
def test_host_twin_vs_float64_autograd(name, scale, with_state, with_lens):
    a = C.inputs(name, scale)
    lens = C.lens(name) if with_lens else None
    x, dout = _nan_padding(a, lens) if with_lens else (a["x"], a["dout"])
    h0, c0 = (a["h0"], a["c0"]) if with_state else (None, None)
    got = rlib.lstm_host(x, a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], h0, c0, lens, dout=dout)
    want = C.reference(name, scale, with_state, with_lens)
    out, hn, cn, dx, dwi, dwh, db, dh0, dc0 = got
    for what, g, w in zip(C.NAMES + ("hN", "cN"), (out, dx, dwi, dwh, db, dh0, dc0, hn, cn), want):
        assert g.dtype == np.float64 and np.isfinite(g).all(), what
        _close(g, w, f"{name} x{scale:g} {what}")
    if with_lens:
        for i, n in enumerate(lens):
            assert not out[i, n:].any() and not dx[i, n:].any()
            assert np.array_equal(hn[i], out[i, n - 1])
    fwd = rlib.lstm_host(x, a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], h0, c0, lens)       # forward only: the same out, nothing else
    assert len(fwd) == 3 and all(np.array_equal(p, q) for p, q in zip(fwd, (out, hn, cn)))


@pytest.mark.parametrize("with_lens", [False, True])
@pytest.mark.parametrize("name", ["one", "ragged", "u29"])
def test_lstm_predictor_on_cpu_tensors_with_an_upstream_gradient(name, with_lens):
    a = C.inputs(name, 1.0)
    lens = C.lens(name) if with_lens else None
    x, dout = _nan_padding(a, lens) if with_lens else (a["x"], a["dout"])
    leaves = [torch.from_numpy(v).requires_grad_(True) for v in (x, a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], a["h0"], a["c0"])]
    out, hn, cn = lstm_predictor(*leaves, lengths=None if lens is None else torch.from_numpy(lens))
    want = C.reference(name, 1.0, True, with_lens)
    assert out.dtype == torch.float32 and out.requires_grad and not hn.requires_grad and not cn.requires_grad
    _close(out.detach().numpy(), want[0], "out", rel=F32)
    _close(hn.numpy(), want[7], "hN", rel=F32)
    _close(cn.numpy(), want[8], "cN", rel=F32)
    out.backward(torch.from_numpy(dout))
    dx, dwi, dwh, db, dh0, dc0 = want[1:7]
    for what, t, ref in zip(("dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0", "dc0"), leaves, (dx, dwi, dwh, db, db, dh0, dc0)):
        assert t.grad is not None and t.grad.dtype == torch.float32 and bool(torch.isfinite(t.grad).all()), what
        _close(t.grad.numpy(), ref, what, rel=F32)                 # the twin's float64, rounded once
    # without h0 / c0 the zero state is implied and five gradients come back
    leaves = [torch.from_numpy(v).requires_grad_(True) for v in (x, a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"])]
    lstm_predictor(*leaves, lengths=None if lens is None else lens)[0].backward(torch.from_numpy(dout))
    for what, t, ref in zip(("dx", "dW_ih", "dW_hh", "db_ih", "db_hh"), leaves, [C.reference(name, 1.0, False, with_lens)[k] for k in (1, 2, 3, 4, 4)]):
        _close(t.grad.numpy(), ref, what + " from the zero state", rel=F32)


def _predictor(seed=None):
    m = RNNPredictor(T.VOCAB, 256, 256, 0.1, 256, 1)
    if seed is not None:
        sd = T.make_state_dict(seed)
        m.load_state_dict({k[len("predictor."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("predictor.")}, strict=True)
    return m


def test_module_has_the_reference_predictor_parameter_names():
    want = {n[len("predictor."):]: tuple(shape) for n, shape, _ in state_dict_spec(T.VOCAB) if n.startswith("predictor.")}
    m = _predictor()
    assert set(want) == {"embed.weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0", "projection.weight", "projection.bias"}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert m.output_size() == 256
    st = m.init_state(3, torch.device("cpu"))
    assert len(st) == 2 and all(s.shape == (1, 3, 256) and not s.any() for s in st)
    for kw in ({"embed_size": 128}, {"output_size": 320}, {"hidden_size": 512}, {"num_layers": 2}, {"bias": False}, {"rnn_type": "gru"}):
        args = dict(voca_size=T.VOCAB, embed_size=256, output_size=256, embed_dropout=0.1, hidden_size=256, num_layers=1)
        args.update(kw)
        with pytest.raises(RnntError) as err:
            RNNPredictor(**args)
        assert err.value.status == rlib.ERR_SHAPE, kw


@pytest.mark.parametrize("seed", [0, 1])
def test_rnn_predictor_vs_the_reference_golden(seed):
    g = load_golden(f"modules_seed{seed}.npz")
    m = _predictor(seed).eval()
    tok = torch.from_numpy(g["pred_tokens"])[None]
    with torch.no_grad():
        out = m(tok)
        _, hn, cn = m.lstm(tok)
        assert hn.shape == (1, 1, 256) and cn.shape == (1, 1, 256)
        err = [float(np.abs(out[0].numpy() - g["pred_out"]).max()), float(np.abs(hn[0, 0].numpy() - g["pred_h"][-1]).max()),
               float(np.abs(cn[0, 0].numpy() - g["pred_c"][-1]).max())]
        # the cache has the reference's meaning: the second half of the string from the state after the first half
        k = tok.shape[1] // 2
        cache = [torch.from_numpy(g["pred_h"][k - 1])[None, None], torch.from_numpy(g["pred_c"][k - 1])[None, None]]
        err.append(float(np.abs(m(tok[:, k:], cache)[0].numpy() - g["pred_out"][k:]).max()))
    print(f"seed {seed}: out {err[0]:.2e}, hN {err[1]:.2e}, cN {err[2]:.2e}, from a cache {err[3]:.2e}")
    assert max(err) < GOLDEN_TOL


class _TorchPredictor(torch.nn.Module):
    """the reference's predictor out of torch's own modules (eval: no dropout)"""

    def __init__(self, vocab):
        super().__init__()
        self.embed = torch.nn.Embedding(vocab, 256)
        self.rnn = torch.nn.LSTM(256, 256, 1, batch_first=True)
        self.projection = torch.nn.Linear(256, 256)

    def forward(self, tok):
        return self.projection(self.rnn(self.embed(tok))[0])


def test_rnn_predictor_vs_a_torch_stand_in_through_the_joint_loss():
    """d loss / d (predictor parameters) of RNNPredictor -> TransducerJoint.loss on CPU tensors (the float64 host twins, float32 between
    the stages) against the same chain with a float64 torch.nn.LSTM in the predictor's place.  The chain stores out, the projection
    and pred_ffn's output in float32, so the bar is a small multiple of float32 rounding relative to the largest gradient entry."""
    V, B, Tn, U = 20, 2, 6, 4
    r = np.random.Generator(np.random.Philox(key=[91, 0]))
    mine = _predictor(0).eval()
    ref = _TorchPredictor(T.VOCAB).double().eval()
    assert {k: tuple(v.shape) for k, v in ref.state_dict().items()} == {k: tuple(v.shape) for k, v in mine.state_dict().items()}
    ref.load_state_dict({k: v.double() for k, v in mine.state_dict().items()}, strict=True)
    joint = TransducerJoint(V, 256, 256)
    enc = torch.from_numpy(r.standard_normal((B, Tn, 256)).astype(np.float32))
    lab = torch.from_numpy(r.integers(1, V, (B, U)).astype(np.int64))
    tok = torch.cat([torch.zeros(B, 1, dtype=torch.int64), lab], dim=1)            # add_blank(texts), blank 0
    ll, tl = torch.tensor([Tn, Tn - 2]), torch.tensor([U, U - 1])
    loss = joint.loss(enc, mine(tok, lengths=tl + 1), lab, ll, tl, blank=0)
    loss.backward()
    joint64 = TransducerJoint(V, 256, 256).double()
    joint64.load_state_dict({k: v.double() for k, v in joint.state_dict().items()})
    pred64 = ref(tok)
    logits = torch.tanh(joint64.enc_ffn(enc.double()).unsqueeze(2) + joint64.pred_ffn(pred64).unsqueeze(1)) @ joint64.ffn_out.weight.T + joint64.ffn_out.bias
    want = torch.stack([torch.from_numpy(np.asarray(T.transducer_loss_ref(logits[i].detach().numpy(), lab[i].numpy().astype(np.int32), int(ll[i]), int(tl[i]), 0)[1]))
                        for i in range(B)]) / B
    logits.backward(want)
    for (name, p), q in zip(mine.named_parameters(), ref.parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        err, top = float((p.grad.double() - q.grad).abs().max()), float(q.grad.abs().max())
        print(f"{name}: error {err:.3e} of {top:.3e}")
        assert top > 0.0 and err <= 64 * F32 * top, name


def _workspace_formula(B, U1):
    """include/rnnt_hip.h, restated"""
    cdiv = lambda a, b: -(-a // b)
    return 4 * (4 * cdiv(B, 4) + 262144 + 1024 * B * U1 + 525312 * cdiv(B * U1, 256)), 5120 * B * U1


def test_workspace_formula_and_refusals():
    for B, U1 in [s[:2] for s in C.SHAPES.values()] + [(16, 29), (5, 256), (700, 3)]:
        assert rlib.lstm_workspace(B, U1) == _workspace_formula(B, U1), (B, U1)
    lib = rlib.load()
    wb, sb = ctypes.c_int64(-7), ctypes.c_int64(-7)
    for args, status in (((0, 1), rlib.ERR_ARG), ((1, 0), rlib.ERR_ARG), ((1, 257), rlib.ERR_SHAPE), ((6554, 256), rlib.ERR_SHAPE)):
        assert lib.rnnt_lstm_workspace(*args, ctypes.byref(wb), ctypes.byref(sb)) == status and wb.value == -7 and sb.value == -7, args
    assert lib.rnnt_lstm_workspace(1, 1, None, ctypes.byref(sb)) == rlib.ERR_ARG and lib.rnnt_lstm_workspace(1, 1, ctypes.byref(wb), None) == rlib.ERR_ARG


def test_host_twin_refusals_write_nothing():
    a = C.inputs("ragged", 1.0)
    B, U1 = a["x"].shape[:2]
    outs = [np.full(s, 7.0) for s in ((B, U1, 256), (B, 256), (B, 256), (B, U1, 256), (1024, 256), (1024, 256), (1024,), (B, 256), (B, 256))]
    head = (a["x"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], a["h0"], a["c0"])
    for lens in ([6, 1, 3], [5, 0, 3], [5, 1, -1]):
        with pytest.raises(RnntError) as err:
            rlib.lstm_host(*head, lens, dout=a["dout"], out=outs)
        assert err.value.status == rlib.ERR_ARG, lens
    lib = rlib.load()
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)
    ptr, optr = [p(v) for v in head[:5]], [p(v) for v in outs]
    call = lambda ptr=ptr, B=B, U1=U1, dout=p(a["dout"]), optr=optr: lib.rnnt_lstm_host(*ptr, None, None, None, B, U1, dout, *optr)
    assert call(B=0) == rlib.ERR_ARG and call(U1=0) == rlib.ERR_ARG and call(U1=257) == rlib.ERR_SHAPE and call(B=6554, U1=256) == rlib.ERR_SHAPE
    for k in range(5):
        assert call(ptr=[None if i == k else q for i, q in enumerate(ptr)]) == rlib.ERR_ARG
    for k in (0, 3, 4, 5, 6):                                      # out, and with dout the four required gradients
        assert call(optr=[None if i == k else q for i, q in enumerate(optr)]) == rlib.ERR_ARG
    assert all((v == 7.0).all() for v in outs)
    rlib.lstm_host(*head, dout=a["dout"], out=outs)                # and an accepted call writes every element
    assert not any((v == 7.0).any() for v in outs)


def test_device_entries_refuse_on_the_host_before_any_launch():
    """null, misaligned, out-of-range and short-buffer calls are decided before the first HIP call: they need no GPU and touch nothing"""
    lib = rlib.load()
    buf = np.zeros(64, np.float32)
    a = buf.ctypes.data + (-buf.ctypes.data % 16)                  # a 16-byte aligned (host) address: never followed
    wbytes, sbytes = rlib.lstm_workspace(3, 5)
    six = np.array([6, 1, 3], np.int32).ctypes.data_as(ctypes.c_void_p)
    zero = np.array([5, 0, 3], np.int32).ctypes.data_as(ctypes.c_void_p)

    def fwd(**k):
        return lib.rnnt_lstm_forward(k.get("x", a), a, a, a, a, k.get("h0", a), a, k.get("lens"), k.get("B", 3), k.get("U1", 5), k.get("out", a), a, a,
                                     k.get("state", a), k.get("sb", sbytes), k.get("work", a), k.get("wb", wbytes), None)

    def bwd(**k):
        return lib.rnnt_lstm_backward(k.get("x", a), a, a, k.get("h0", a), a, k.get("out", a), k.get("state", a), k.get("sb", sbytes), a, k.get("lens"),
                                      k.get("B", 3), k.get("U1", 5), a, a, a, a, a, a, k.get("work", a), k.get("wb", wbytes), None)

    for call in (fwd, bwd):
        assert call(x=None) == rlib.ERR_ARG and call(out=None) == rlib.ERR_ARG and call(work=None) == rlib.ERR_ARG
        assert call(x=a + 4) == rlib.ERR_ARG and call(h0=a + 8) == rlib.ERR_ARG and call(work=a + 8) == rlib.ERR_ARG and call(state=a + 4) == rlib.ERR_ARG
        assert call(B=0) == rlib.ERR_ARG and call(U1=0) == rlib.ERR_ARG and call(lens=six) == rlib.ERR_ARG and call(lens=zero) == rlib.ERR_ARG
        assert call(U1=257) == rlib.ERR_SHAPE and call(B=6554, U1=256) == rlib.ERR_SHAPE
        assert call(wb=wbytes - 1) == rlib.ERR_SHAPE and call(sb=sbytes - 1) == rlib.ERR_SHAPE
    assert bwd(state=None) == rlib.ERR_ARG
    assert not buf.any()


def test_lstm_predictor_argument_errors():
    a = C.inputs("ragged", 1.0)
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    args = [t[k] for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh")]
    for k in range(5):
        for cast in (torch.Tensor.double, torch.Tensor.half):
            with pytest.raises(TypeError):
                lstm_predictor(*(cast(v) if i == k else v for i, v in enumerate(args)))
    with pytest.raises(TypeError):
        lstm_predictor(*args, h0=t["h0"].double())
    with pytest.raises(TypeError):
        lstm_predictor(args[0].numpy(), *args[1:])
    bad = ({"x": t["x"][:, :, :128]}, {"x": t["x"][0]}, {"w_ih": t["w_ih"][:512]}, {"w_hh": t["w_hh"].T}, {"b_ih": t["b_ih"][:256]}, {"h0": t["h0"][:2]},
           {"c0": t["c0"][:, :128]}, {"lengths": torch.tensor([5, 1])}, {"lengths": torch.tensor([6, 1, 3])}, {"lengths": torch.tensor([5, 0, 3])})
    for kw in bad:
        call = dict(zip(("x", "w_ih", "w_hh", "b_ih", "b_hh"), args))
        call.update(kw)
        with pytest.raises(RnntError) as err:
            lstm_predictor(**call)
        assert err.value.status == rlib.ERR_ARG, list(kw)
    with pytest.raises(RnntError) as err:
        lstm_predictor(torch.zeros(1, 257, 256), *args[1:])
    assert err.value.status == rlib.ERR_SHAPE
