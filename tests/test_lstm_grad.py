"""The predictor's LSTM with gradients on the device (rnnt_lstm_forward / _backward, ctc_vr_amd.functional.lstm_predictor and
RNNPredictor on CUDA tensors).  Needs a real MI355X: `pytest -m gpu`.

The yardstick is float64 torch autograd of the step loop on the CPU (testing.lstm_ref).  The device owes float32 products, sums and
activations with the library's logistic formula, which is what testing.lstm_f32_emulation does on the CPU.  So the bound is measured,
not chosen: per scale (1 and 30) and output, E is the emulation's largest absolute distance from float64 over the cases of
lstm_grad_cases.py at that scale, and the device is held to 8 E: the factor test_joint_grad.py uses, for its reason -- another
summation tree, and device exp2 / rcp within a couple of ulps.  The yardstick stays per scale: one maximum over both would let the
unit-scale cases pass at a hundred times their own error."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
import joint_loss_cases as JL
import lstm_grad_cases as C
from ctc_vr_amd.functional import RNNPredictor, TransducerJoint
from ctc_vr_amd.lib import RnntError

pytestmark = pytest.mark.gpu

FACTOR = 8.0
GUARD = 64                        # floats behind every output, which no kernel may touch
SENTINEL = 12345.0
STEP_TOL = 1e-4                   # the bar test_predictor_and_joint_step_api holds the step call to
OUTS = ("out", "hn", "cn", "dx", "dW_ih", "dW_hh", "db", "dh0", "dc0")


@pytest.fixture(scope="module")
def yardstick():
    E = C.yardstick()
    for scale in C.SCALES:
        print(f"emulation vs float64 at scale {scale:g}: " + ", ".join(f"E_{x} = {E[scale][x]:.3e}" for x in C.NAMES))
        for x in C.NAMES:
            assert 0.0 < E[scale][x] < 1e-2, f"E_{x} = {E[scale][x]} at scale {scale:g}: an emulation that costs nothing (or everything) measures nothing"
    return E


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(n):
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _run(a, with_state, lens=None, x=None, dout=None, backward=True):
    """one rnnt_lstm_forward (+ rnnt_lstm_backward) through the raw lib calls into NaN-filled, guarded outputs:
    ({name: numpy}, state [B, U1, 5, 256], guards intact)"""
    x = a["x"] if x is None else x
    dout = a["dout"] if dout is None else dout
    B, U1, D = x.shape
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (("x", x), ("w_ih", a["w_ih"]), ("w_hh", a["w_hh"]), ("b_ih", a["b_ih"]),
                                                                             ("b_hh", a["b_hh"]), ("h0", a["h0"]), ("c0", a["c0"]), ("dout", dout))}
    h0 = dev["h0"].data_ptr() if with_state else None
    c0 = dev["c0"].data_ptr() if with_state else None
    wbytes, sbytes = rlib.lstm_workspace(B, U1)
    work = torch.empty(wbytes, dtype=torch.uint8, device="cuda")
    sizes = dict(zip(OUTS, (B * U1 * D, B * D, B * D, B * U1 * D, 4 * D * D, 4 * D * D, 4 * D, B * D, B * D)))
    shapes = dict(zip(OUTS, ((B, U1, D), (B, D), (B, D), (B, U1, D), (4 * D, D), (4 * D, D), (4 * D,), (B, D), (B, D))))
    names = OUTS if backward else OUTS[:3]
    buf = {k: _guarded(sizes[k]) for k in names}
    state = _guarded(sbytes // 4)
    s = torch.cuda.current_stream().cuda_stream
    rlib.lstm_forward_device(dev["x"].data_ptr(), dev["w_ih"].data_ptr(), dev["w_hh"].data_ptr(), dev["b_ih"].data_ptr(), dev["b_hh"].data_ptr(), h0, c0, lens,
                             (B, U1), buf["out"].data_ptr(), buf["hn"].data_ptr(), buf["cn"].data_ptr(), state.data_ptr(), sbytes, work.data_ptr(), wbytes, s)
    if backward:
        rlib.lstm_backward_device(dev["x"].data_ptr(), dev["w_ih"].data_ptr(), dev["w_hh"].data_ptr(), h0, c0, buf["out"].data_ptr(), state.data_ptr(), sbytes,
                                  dev["dout"].data_ptr(), lens, (B, U1), *(buf[k].data_ptr() for k in OUTS[3:]), work.data_ptr(), wbytes, s)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    st = state.cpu().numpy()
    intact = all(bool((host[k][sizes[k]:] == np.float32(SENTINEL)).all()) for k in names) and bool((st[sbytes // 4:] == np.float32(SENTINEL)).all())
    return {k: host[k][:sizes[k]].reshape(shapes[k]) for k in names}, st[:sbytes // 4].reshape(B, U1, 5, D), intact


def _ratios(got, want, E):
    """{x: error / E_x} of the seven yardstick outputs (want: lstm_grad_cases.reference)"""
    return {x: float(np.abs(got[k] - w).max()) / E[x] for x, k, w in zip(C.NAMES, ("out",) + OUTS[3:], want)}


@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("name,scale", C.CASES)
def test_forward_and_backward_vs_float64(name, scale, with_state, yardstick):
    E = yardstick[scale]
    a = C.inputs(name, scale)
    got, _, intact = _run(a, with_state)
    assert intact, "something was written behind an output"
    for k in OUTS:
        assert np.isfinite(got[k]).all(), f"{k}: an element was not written (or is not finite)"
    want = C.reference(name, scale, with_state, False)
    ratios = _ratios(got, want, E)
    print(f"{name} x{scale:g} {'with' if with_state else 'without'} h0 / c0: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items()))
    again, _, _ = _run(a, with_state)
    assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in OUTS), "two calls on the same inputs differ"
    fwd, _, intact = _run(a, with_state, backward=False)           # the forward alone leaves the same three outputs
    assert intact and all(np.array_equal(_bits(got[k]), _bits(fwd[k])) for k in OUTS[:3])
    assert float(np.abs(got["hn"] - want[7]).max()) <= FACTOR * E["out"] and np.array_equal(got["hn"], got["out"][:, -1])
    for x, r in ratios.items():                                    # (without h0 / c0, dh0 and dc0 are the gradients at the zero state)
        assert r <= FACTOR, f"{x}: {r:.2f} E, the bound is {FACTOR:g} E"


@pytest.mark.parametrize("name,scale", C.CASES)
def test_with_lengths_the_padding_is_never_read(name, scale, yardstick):
    E = yardstick[scale]
    a = C.inputs(name, scale)
    lens = C.lens(name)
    B, U1 = a["x"].shape[:2]
    live = (np.arange(U1)[None, :] < lens[:, None])[..., None]
    nan, zero = np.float32("nan"), np.float32(0.0)
    got, st, intact = _run(a, True, lens, np.where(live, a["x"], nan).astype(np.float32), np.where(live, a["dout"], nan).astype(np.float32))
    ref0, _, _ = _run(a, True, lens, np.where(live, a["x"], zero).astype(np.float32), np.where(live, a["dout"], zero).astype(np.float32))
    assert intact
    for k in OUTS:
        assert np.isfinite(got[k]).all(), f"{k}: padding was read"
        assert np.array_equal(_bits(got[k]), _bits(ref0[k])), f"{k}: NaN padding and zero padding differ"
    for i, n in enumerate(lens):
        assert not got["out"][i, n:].any() and not got["dx"][i, n:].any(), "out and dx beyond a row's length are exactly 0"
        assert np.array_equal(got["hn"][i], got["out"][i, n - 1]) and np.array_equal(got["cn"][i], st[i, n - 1, 4]), "hN / cN are the last valid step's"
    ratios = _ratios(got, C.reference(name, scale, True, True), E)
    print(f"{name} x{scale:g} with lengths {lens.tolist() if B <= 4 else '...'}: " + ", ".join(f"{x} {r:.3f} E" for x, r in ratios.items()))
    for x, r in ratios.items():
        assert r <= FACTOR, f"{x}: {r:.2f} E, the bound is {FACTOR:g} E"


@pytest.mark.parametrize("bias", [200.0, -200.0])
def test_saturated_gates_give_exact_zeros(bias):
    a = dict(C.inputs("ragged", 1.0))
    a["b_ih"] = np.full(1024, bias, np.float32)
    got, st, intact = _run(a, True)
    assert intact and all(np.isfinite(got[k]).all() for k in OUTS), "nothing may be NaN"
    if bias > 0:                                                   # sigmoid = 1 and tanh(g) = 1 exactly: every derivative factor is exactly 0
        assert (st[:, :, :4] == 1.0).all()
        for k in ("dx", "dW_ih", "dW_hh", "db", "dh0"):
            assert not got[k].any(), f"{k} is not exactly 0"
        c = a["c0"][:, None, :] + np.arange(1, 6, dtype=np.float32)[None, :, None]            # c grows by exactly i g = 1 per step
        assert np.abs(st[:, :, 4] - c).max() <= 1e-5 and np.abs(got["out"] - np.tanh(c)).max() <= 1e-5
    else:                                                          # every sigmoid is exactly 0: out = 0 * tanh(c)
        assert not st[:, :, [0, 1, 3]].any() and (st[:, :, 2] == -1.0).all() and not got["out"].any() and not got["hn"].any()
        for k in ("dx", "dW_ih", "dW_hh", "db", "dh0"):
            assert not got[k].any(), f"{k} is not exactly 0"


def _predictor(sd, device):
    m = RNNPredictor(T.VOCAB, 256, 256, 0.1, 256, 1)
    m.load_state_dict({k[len("predictor."):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("predictor.")}, strict=True)
    return m.to(device).eval()


def test_sequence_forward_vs_the_inference_predictor(np_state_dict):
    """rnnt_predictor_step over a 10-token string for 3 rows against RNNPredictor on the same weights: the two differ in summation
    order only"""
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    sd = np_state_dict(0)
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=T.BLANK, streaming=True, static_chunk_size=16, predictor_dropout=0)
    m.load_state_dict(sd)
    dev, eng = m.device, m._engine
    r = np.random.Generator(np.random.Philox(key=[92, 0]))
    tok = torch.from_numpy(r.integers(0, T.VOCAB, (3, 10)).astype(np.int64)).to(dev)
    h, c = torch.zeros(3, 256, device=dev), torch.zeros(3, 256, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for u in range(10):
        t = tok[:, u].to(torch.int32).contiguous()
        out, h2, c2 = torch.empty(3, 256, device=dev), torch.empty(3, 256, device=dev), torch.empty(3, 256, device=dev)
        eng.predictor_step(t.data_ptr(), h.data_ptr(), c.data_ptr(), 3, out.data_ptr(), h2.data_ptr(), c2.data_ptr(), s)
        torch.cuda.synchronize()
        outs.append(out)
        h, c = h2, c2
    pred = _predictor(sd, dev)
    with torch.no_grad():
        got = pred(tok)
        _, hn, cn = pred.lstm(tok)
    err = [float((got - torch.stack(outs, dim=1)).abs().max()), float((hn[0] - h).abs().max()), float((cn[0] - c).abs().max())]
    print(f"sequence forward vs step loop: out {err[0]:.2e}, h {err[1]:.2e}, c {err[2]:.2e}")
    assert max(err) < STEP_TOL


def test_autograd_chain_into_the_joint_loss(yardstick, np_state_dict):
    """RNNPredictor -> TransducerJoint.loss(...).backward() on CUDA tensors at the shape of `u29` against the same chain on CPU tensors
    (the float64 host twins).  Two device stages stand between the two chains, and the bound is the sum of their measured bounds:
      LSTM stage   8 E_x of this file's yardstick at scale 1, x the gradient the parameter takes (dW_ih, dW_hh, db, db; dx for the
                   embedding; out for the projection, whose gradient sees the LSTM's forward error),
      loss stage   8 E_dp of the fused joint-and-loss yardstick (joint_loss_cases.yardstick("mean")), the error of d loss / d pred_proj,
    times n, the number of rows the parameter's gradient adds up with weights of at most 1: 1 for the LSTM's own parameters (their E
    already is that of whole sums), the largest count of one token for embed.weight, B U1 for the projection.  The test prints every
    error beside its bound."""
    B, U1 = C.SHAPES["u29"][:2]
    V, Tn, blank = 412, 9, 5
    E, E_dp = yardstick[1.0], JL.yardstick("mean")["dp"]
    r = np.random.Generator(np.random.Philox(key=[93, 0]))
    lab = r.integers(0, V - 1, (B, U1 - 1))
    lab = torch.from_numpy(np.where(lab >= blank, lab + 1, lab).astype(np.int64))
    tok = torch.cat([torch.full((B, 1), blank, dtype=torch.int64), lab], dim=1)
    enc = torch.from_numpy(r.standard_normal((B, Tn, 256)).astype(np.float32))
    ll, tl = torch.tensor([Tn, Tn - 2]), torch.tensor([U1 - 1, U1 - 4])
    sd = np_state_dict(0)
    joint0 = TransducerJoint(V, 256, 256)

    def chain(device):
        pred = _predictor(sd, device)
        joint = TransducerJoint(V, 256, 256).to(device)
        joint.load_state_dict(joint0.state_dict())
        loss = joint.loss(enc.to(device), pred(tok.to(device), lengths=tl + 1), lab.to(device), ll, tl, blank=blank)
        loss.backward()
        return float(loss.detach()), {k: p.grad.detach().cpu().numpy() for k, p in pred.named_parameters()}

    loss_d, got = chain("cuda")
    _, again = chain("cuda")
    loss_h, want = chain("cpu")
    assert abs(loss_d - loss_h) <= 1e-4 * abs(loss_h)
    count = int(np.bincount(tok.numpy().ravel()).max())
    stage = {"embed.weight": ("dx", count), "rnn.weight_ih_l0": ("dW_ih", 1), "rnn.weight_hh_l0": ("dW_hh", 1), "rnn.bias_ih_l0": ("db", 1),
             "rnn.bias_hh_l0": ("db", 1), "projection.weight": ("out", B * U1), "projection.bias": ("out", B * U1)}
    assert set(stage) == set(got)
    bad = []
    for k, (x, n) in stage.items():
        assert np.isfinite(got[k]).all() and got[k].any(), k
        assert np.array_equal(_bits(got[k]), _bits(again[k])), f"{k}: two backward passes differ"
        err, bound = float(np.abs(got[k].astype(np.float64) - want[k]).max()), n * (FACTOR * E[x] + FACTOR * E_dp)
        print(f"{k}: |device - host chain| = {err:.3e}, bound {n} x (8 E_{x} + 8 E_dp) = {bound:.3e}")
        if err > bound:
            bad.append(k)
    assert not bad, bad


def test_lstm_predictor_saves_its_inputs_out_and_one_state_tensor():
    from ctc_vr_amd.functional import lstm_predictor
    a = C.inputs("u29", 1.0)
    B, U1 = a["x"].shape[:2]
    leaves = [torch.from_numpy(a[k]).cuda().requires_grad_(True) for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")]
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
        out, hn, cn = lstm_predictor(*leaves)
    assert out.is_cuda and out.requires_grad and not hn.requires_grad and not cn.requires_grad
    assert len(saved) == 9 and all(any(s.data_ptr() == t.data_ptr() for s in saved) for t in leaves + [out])
    assert sum(s.dtype == torch.uint8 and s.numel() == 5120 * B * U1 for s in saved) == 1    # the state: gates and c of every step
    got, _, _ = _run(a, True)                                     # the autograd function runs the same entries: the same bits
    assert np.array_equal(_bits(out.detach().cpu().numpy()), _bits(got["out"]))
    out.backward(torch.from_numpy(a["dout"]).cuda())
    for t, k in zip(leaves, ("dx", "dW_ih", "dW_hh", "db", "db", "dh0", "dc0")):
        assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(got[k])), k


def test_a_refusal_launches_nothing():
    a = C.inputs("ragged", 1.0)
    B, U1 = a["x"].shape[:2]
    d = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    wbytes, sbytes = rlib.lstm_workspace(B, U1)
    work = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")
    state = torch.zeros(sbytes, dtype=torch.uint8, device="cuda")
    outs = [torch.full((n,), 7.0, device="cuda") for n in (B * U1 * 256, B * 256, B * 256, B * U1 * 256, 1024 * 256, 1024 * 256, 1024, B * 256, B * 256)]
    p = [o.data_ptr() for o in outs]
    s = torch.cuda.current_stream().cuda_stream

    def fwd(lens=None, shape=(B, U1), wb=wbytes, sb=sbytes, x=d["x"].data_ptr()):
        rlib.lstm_forward_device(x, d["w_ih"].data_ptr(), d["w_hh"].data_ptr(), d["b_ih"].data_ptr(), d["b_hh"].data_ptr(), None, None, lens, shape, p[0], p[1],
                                 p[2], state.data_ptr(), sb, work.data_ptr(), wb, s)

    def bwd(lens=None, shape=(B, U1), wb=wbytes, sb=sbytes, x=d["x"].data_ptr()):
        rlib.lstm_backward_device(x, d["w_ih"].data_ptr(), d["w_hh"].data_ptr(), None, None, p[0], state.data_ptr(), sb, d["dout"].data_ptr(), lens, shape,
                                  *p[3:], work.data_ptr(), wb, s)

    for call in (fwd, bwd):
        for kw, status in (({"lens": [6, 1, 3]}, rlib.ERR_ARG), ({"lens": [5, 0, 3]}, rlib.ERR_ARG), ({"x": d["x"].data_ptr() + 4}, rlib.ERR_ARG),
                           ({"x": None}, rlib.ERR_ARG), ({"shape": (0, U1)}, rlib.ERR_ARG), ({"shape": (B, 0)}, rlib.ERR_ARG), ({"shape": (B, 257)}, rlib.ERR_SHAPE),
                           ({"wb": wbytes - 1}, rlib.ERR_SHAPE), ({"sb": sbytes - 1}, rlib.ERR_SHAPE)):
            with pytest.raises(RnntError) as err:
                call(**kw)
            assert err.value.status == status, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and not bool(work.any()) and not bool(state.any())
