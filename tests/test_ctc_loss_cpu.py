"""The CTC loss with gradients, everything that needs no GPU: the C++ host twin (rnnt_ctc_loss_host), the float64 yardstick
(ctc_vr_amd.testing.ctc_loss_ref), functional.ctc_loss and CTCHead on CPU tensors, and every refusal.

torch.nn.functional.ctc_loss on float64 CPU tensors is the outside reference.  Two of its habits matter here.  Its backward returns
exp(lp) - occupancy for the gradient with respect to the log-probabilities -- the gradient with respect to the LOGITS behind a
log-softmax, which is what fused_log_softmax=True returns -- so gradients are compared through log_softmax, and the gradient with
respect to log-probabilities as they stand (-occupancy) is compared against ctc_loss_ref's plain autograd.  And without zero_infinity
it writes NaN into the gradient of a row whose frames cannot hold its transcript, where this project writes exact zeros."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import CTCHead, ctc_loss
from ctc_vr_amd.lib import RnntError

# the issue's row set: row 1 needs 5 frames and has 4
TB, LB, V, BLANK = (6, 4, 1), (3, 3, 1), 8, 0
TARGETS = np.array([[1, 1, 2], [3, 3, 3], [4, -1, -1]], np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _rows(seed=3, scale=2.0):
    g = np.random.Generator(np.random.Philox(key=[seed, 17]))
    return (scale * g.standard_normal((len(TB), max(TB), V))).astype(np.float32)            # [B, T, V], finite everywhere


def _torch_f64(x_btv, targets, tb, lb, blank, **kw):
    """F.ctc_loss on float64 behind a float64 log_softmax: (loss, d loss / d logits [B, T, V])"""
    x = torch.from_numpy(x_btv).double().requires_grad_(True)
    loss = F.ctc_loss(torch.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(np.maximum(targets, 0).astype(np.int64)), torch.tensor(tb),
                      torch.tensor(lb), blank=blank, **kw)
    (loss if loss.dim() == 0 else loss.sum()).backward()
    return loss.detach().numpy(), x.grad.numpy()


CASES = {
    "issue rows": (TB, LB, TARGETS, V, BLANK),
    "no labels, one frame, repeats": ((1, 7, 9, 9), (0, 4, 4, 0), np.array([[1, 1, 1, 1], [2, 2, 2, 2], [1, 2, 1, 2], [3, 3, 3, 3]], np.int32), 5, 4),
    "long": ((40, 33), (12, 9), np.random.Generator(np.random.Philox(key=[5, 5])).integers(1, 30, (2, 12)).astype(np.int32), 30, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_and_reference_vs_torch_float64(name):
    tb, lb, tg, v, blank = CASES[name]
    B, Tn = len(tb), max(tb)
    g = np.random.Generator(np.random.Philox(key=[sorted(CASES).index(name), 1]))
    x = (3.0 * g.standard_normal((B, Tn, v))).astype(np.float32)
    want_nll, want_grad = _torch_f64(x, tg, tb, lb, blank, reduction="none")
    nll, grad = rlib.ctc_loss_host(x, tg, tb, lb, blank, fused_log_softmax=True)
    feasible = np.isfinite(want_nll)
    assert np.array_equal(np.isfinite(nll), feasible) and (nll[~feasible] == math.inf).all()
    if name == "issue rows":
        assert feasible.tolist() == [True, False, True]
    assert (np.abs(nll[feasible] - want_nll[feasible]) <= 1e-9 * np.abs(want_nll[feasible])).all()
    assert np.abs(grad - want_grad)[feasible].max() <= 1e-9
    assert not _bits(grad)[~feasible].any(), "the gradient of an infeasible row is not bitwise 0"
    for b in range(B):
        assert not _bits(grad[b, tb[b]:]).any(), "the gradient of a padding frame is not bitwise 0"
        r_nll, r_grad = T.ctc_loss_ref(x[b], tg[b, :lb[b]], tb[b], blank)
        e_nll, e_grad = T.ctc_loss_f32_emulation(x[b], tg[b, :lb[b]], tb[b], blank)
        if feasible[b]:
            assert abs(r_nll - want_nll[b]) <= 1e-9 * abs(want_nll[b]) and np.abs(r_grad - want_grad[b]).max() <= 1e-9
            # float32 picks, no more: each of the T_b picks on a path is off by 2^-24 of its lse, an ABSOLUTE error (nll may be near 0)
            assert abs(e_nll - r_nll) <= 1e-5 * max(abs(r_nll), 1.0) and np.abs(e_grad - r_grad).max() <= 1e-3
        else:
            assert r_nll == math.inf and not r_grad.any() and e_nll == math.inf and not e_grad.any()
    # log-probabilities as they stand: the true gradient -occupancy, against plain autograd
    lp = torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()
    nll_lp, grad_lp = rlib.ctc_loss_host(lp, tg, tb, lb, blank, fused_log_softmax=False)
    for b in range(B):
        r_nll, r_grad = T.ctc_loss_ref(lp[b], tg[b, :lb[b]], tb[b], blank, fused_log_softmax=False)
        if feasible[b]:
            assert abs(nll_lp[b] - r_nll) <= 1e-9 * abs(r_nll) and np.abs(grad_lp[b] - r_grad).max() <= 1e-9
            assert (grad_lp[b] <= 0).all()
        else:
            assert nll_lp[b] == math.inf and not _bits(grad_lp[b]).any()
    # value only: the same bits
    assert np.array_equal(_bits(rlib.ctc_loss_host(x, tg, tb, lb, blank, want_grad=False)[0]), _bits(nll))


def test_host_twin_strides():
    """a contiguous [B, T, V] array and the transposed view of a contiguous [T, B, V] one: the same values, the gradient laid out
    like its input"""
    x = _rows()
    nll, grad = rlib.ctc_loss_host(x, TARGETS, TB, LB, BLANK)
    xt = np.ascontiguousarray(x.transpose(1, 0, 2)).transpose(1, 0, 2)
    assert not xt.flags.c_contiguous
    nll_t, grad_t = rlib.ctc_loss_host(xt, TARGETS, TB, LB, BLANK)
    assert grad_t.strides == (V * 8, len(TB) * V * 8, 8)
    assert np.array_equal(_bits(nll), _bits(nll_t)) and np.array_equal(_bits(grad), _bits(grad_t))


BRUTE = [(5, [1, 1]), (5, [1, 2]), (4, [2]), (3, []), (2, [1, 1]), (3, [1, 1]), (1, [2]), (1, [])]   # (T_b, labels): V = 3, blank 0


@pytest.mark.parametrize("tb,labels", BRUTE)
def test_against_the_sum_over_all_paths(tb, labels):
    g = np.random.Generator(np.random.Philox(key=[tb, 10 * len(labels) + sum(labels)]))
    x = g.standard_normal((1, tb, 3)).astype(np.float32)
    lmax = max(len(labels), 1)
    tg = np.zeros((1, lmax), np.int32)
    tg[0, :len(labels)] = labels

    def brute(xd):
        return T.ctc_loss_bruteforce(torch.log_softmax(torch.from_numpy(xd), -1).numpy(), labels, tb, 0)
    want = brute(x[0].astype(np.float64))
    nll, grad = rlib.ctc_loss_host(x, tg, [tb], [len(labels)], 0)
    r_nll, r_grad = T.ctc_loss_ref(x[0], labels, tb, 0)
    if not math.isfinite(want):
        assert (tb, labels) == (2, [1, 1]) and nll[0] == math.inf and r_nll == math.inf and not grad.any()
        return
    assert abs(nll[0] - want) <= 1e-12 * max(abs(want), 1.0) and abs(r_nll - want) <= 1e-12 * max(abs(want), 1.0)
    h = 1e-5
    fd = np.zeros((tb, 3))
    for t in range(tb):
        for k in range(3):
            xp, xm = x[0].astype(np.float64), x[0].astype(np.float64)
            xp[t, k] += h
            xm[t, k] -= h
            fd[t, k] = (brute(xp) - brute(xm)) / (2 * h)
    # central differences: h^2 / 6 times a third derivative of order 1, and 2^-52 |nll| / h of rounding: both below 1e-8
    assert np.abs(grad[0] - fd).max() <= 1e-8 and np.abs(r_grad - fd).max() <= 1e-8


def _ours(x_tbv, targets, **kw):
    x = x_tbv.clone().requires_grad_(True) if x_tbv.is_contiguous() else x_tbv.detach().requires_grad_(True)
    loss = ctc_loss(x, targets, torch.tensor(TB), torch.tensor(LB), blank=BLANK, fused_log_softmax=True, **kw)
    (loss if loss.dim() == 0 else loss.sum()).backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("zero_infinity", [False, True])
def test_functional_on_cpu_tensors_vs_torch(reduction, zero_infinity):
    x = _rows()                                                    # [B, T, V]
    want, want_grad = _torch_f64(x, TARGETS, TB, LB, BLANK, reduction=reduction, zero_infinity=zero_infinity)
    padded = torch.from_numpy(TARGETS)
    concat = torch.tensor([1, 1, 2, 3, 3, 3, 4])
    x_tbv = torch.from_numpy(x).transpose(0, 1).contiguous()       # contiguous [T, B, V]
    x_view = torch.from_numpy(x).transpose(0, 1)                   # the transposed view of [B, T, V]: what the reference passes
    assert not x_view.is_contiguous()
    outs = [_ours(x_tbv, padded, reduction=reduction, zero_infinity=zero_infinity),
            _ours(x_tbv, concat, reduction=reduction, zero_infinity=zero_infinity),
            _ours(x_view, padded, reduction=reduction, zero_infinity=zero_infinity)]
    for loss, grad in outs:
        assert loss.dtype == torch.float32 and grad.dtype == torch.float32 and grad.shape == x_tbv.shape
        assert torch.equal(loss, outs[0][0]) and torch.equal(grad, outs[0][1])       # targets' form and layout change nothing
    loss, grad = outs[0]
    got, g = loss.numpy().astype(np.float64), grad.transpose(0, 1).numpy().astype(np.float64)
    if zero_infinity:
        assert np.isfinite(want).all() and np.allclose(got, want, rtol=2e-7, atol=0)
        if reduction == "none":
            assert got[1] == 0.0
    else:
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.isinf(want).any()
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=2e-7, atol=0)
        assert np.isnan(want_grad[1, :TB[1]]).all(),"torch no longer writes NaN into an infeasible row: the departure in ctc_loss's docstring is stale"
    assert not _bits(grad.transpose(0, 1).numpy()[1]).any(), "the infeasible row's gradient is not bitwise 0"
    for b in (0, 2):                                               # float32 results of a float64 computation: one rounding
        assert np.abs(g[b] - want_grad[b]).max() <= 2.0 ** -23
        assert not _bits(grad.transpose(0, 1).numpy()[b, TB[b]:]).any()


def test_functional_reads_no_padding_and_takes_16_bit_and_log_probabilities():
    x = _rows()
    for b, tb in enumerate(TB):
        x[b, tb:] = np.nan
    xt = torch.from_numpy(x).transpose(0, 1)
    want = ctc_loss(xt, torch.from_numpy(TARGETS), TB, LB, reduction="none", zero_infinity=True, fused_log_softmax=True)
    assert torch.isfinite(want).all() and want[1] == 0
    lp = torch.log_softmax(torch.from_numpy(_rows()).double(), -1).float().transpose(0, 1)
    got = ctc_loss(lp, torch.from_numpy(TARGETS), TB, LB, reduction="none", zero_infinity=True)      # torch's meaning: log-probabilities
    assert torch.allclose(got, want, rtol=1e-6, atol=0)
    for dt in (torch.bfloat16, torch.float16):
        x16 = torch.from_numpy(_rows()).to(dt).transpose(0, 1).requires_grad_(True)
        loss = ctc_loss(x16, torch.from_numpy(TARGETS), TB, LB, zero_infinity=True, fused_log_softmax=True)
        loss.backward()
        x32 = x16.detach().float().requires_grad_(True)
        loss32 = ctc_loss(x32, torch.from_numpy(TARGETS), TB, LB, zero_infinity=True, fused_log_softmax=True)
        loss32.backward()
        assert loss.dtype == torch.float32 and x16.grad.dtype == dt and torch.equal(loss, loss32)
        assert float((x16.grad.float() - x32.grad).abs().max()) <= 2.0 ** (-8 if dt == torch.bfloat16 else -11)     # |g| <= 1: half an ulp at most, twice
    with pytest.raises(TypeError):
        ctc_loss(xt.double(), torch.from_numpy(TARGETS), TB, LB)
    with pytest.raises(ValueError):
        ctc_loss(xt, torch.from_numpy(TARGETS), TB, LB, reduction="avg")


def test_ctc_head_vs_the_reference_head_restated():
    """OnlineCTC restated in eager torch: dropout, ctc_lo, transpose, log_softmax, nn.CTCLoss(blank, "mean", zero_infinity=True)"""
    B, Tn, D = len(TB), max(TB), 16
    head = CTCHead(V, D, dropout_rate=0.0, blank_id=BLANK)
    assert sorted(n for n, _ in head.named_parameters()) == ["ctc_lo.bias", "ctc_lo.weight"]
    lo = torch.nn.Linear(D, V).double()
    lo.load_state_dict({k: v.double() for k, v in head.ctc_lo.state_dict().items()})
    hs = torch.randn(B, Tn, D, generator=torch.Generator().manual_seed(4))
    ys, hl, yl = torch.from_numpy(TARGETS), torch.tensor(TB), torch.tensor(LB)
    hs_ours = hs.clone().requires_grad_(True)
    loss, ys_hat = head(hs_ours, hl, ys, yl)
    assert ys_hat is None
    loss.backward()
    hs_ref = hs.double().requires_grad_(True)
    lp = lo(F.dropout(hs_ref, p=0.0)).transpose(0, 1).log_softmax(2)
    want = torch.nn.CTCLoss(blank=BLANK, reduction="mean", zero_infinity=True)(lp, ys.clamp(min=0).long(), hl, yl)
    want.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= 2e-7 * abs(float(want.detach()))
    for got, ref in ((hs_ours.grad, hs_ref.grad), (head.ctc_lo.weight.grad, lo.weight.grad), (head.ctc_lo.bias.grad, lo.bias.grad)):
        assert torch.isfinite(got).all() and float((got.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    _, ys_hat = head(hs, hl, ys, yl, return_log_probs=True)
    assert ys_hat.shape == (B, Tn, V) and torch.allclose(ys_hat.double(), lp.transpose(0, 1).detach(), atol=1e-6)
    assert torch.equal(head.log_softmax(hs), ys_hat) and torch.equal(head.argmax(hs), head.ctc_lo(hs).argmax(2))


def _host_call(x, sb, st, tg, tb, lb, B, Tn, lmax, v, blank, nll, grad):
    return rlib.load().rnnt_ctc_loss_host(x.ctypes.data if x is not None else None, sb, st, tg.ctypes.data if tg is not None else None,
                                          tb.ctypes.data if tb is not None else None, lb.ctypes.data if lb is not None else None, B, Tn, lmax, v, blank, 1,
                                          nll.ctypes.data if nll is not None else None, grad.ctypes.data)


def test_every_refusal_leaves_the_outputs_untouched():
    x = np.ascontiguousarray(_rows())
    B, Tn = len(TB), max(TB)
    tb, lb = np.array(TB, np.int32), np.array(LB, np.int32)
    nll, grad = np.full(B, 7.0), np.full(x.shape, 7.0)
    ok = dict(x=x, sb=Tn * V, st=V, tg=TARGETS, tb=tb, lb=lb, B=B, Tn=Tn, lmax=3, v=V, blank=BLANK, nll=nll, grad=grad)
    bad_label, blank_label = TARGETS.copy(), TARGETS.copy()
    bad_label[0, 2], blank_label[2, 0] = V, BLANK
    arg = [dict(x=None), dict(tg=None), dict(tb=None), dict(lb=None), dict(nll=None), dict(B=0), dict(v=1), dict(blank=-1), dict(blank=V),
           dict(tb=np.array([6, 0, 1], np.int32)), dict(tb=np.array([7, 4, 1], np.int32)), dict(lb=np.array([3, 4, 1], np.int32)),
           dict(lb=np.array([3, -1, 1], np.int32)), dict(tg=bad_label), dict(tg=blank_label), dict(st=V - 1), dict(sb=V - 1),
           dict(sb=Tn * V - 1), dict(sb=V, st=B * V - 1), dict(lmax=-1)]
    for change in arg:
        assert _host_call(**{**ok, **change}) == rlib.ERR_ARG, change
    big = np.zeros((1, 256), np.int32)
    assert _host_call(x, Tn * V, V, big, tb[:1], np.array([0], np.int32), 1, Tn, 256, V, BLANK, nll, grad) == rlib.ERR_SHAPE       # Lmax > 255
    assert _host_call(x, 8, 8 * 70000, big, np.array([1] * 70000, np.int32), np.zeros(70000, np.int32), 70000, 70000, 0, V, BLANK, nll,
                      grad) == rlib.ERR_SHAPE                      # B T (2 Lmax + 1) >= 2^31 - 1, refused before a length is read
    assert (nll == 7.0).all() and (grad == 7.0).all()
    assert _host_call(**ok) == 0 and not (nll == 7.0).any()
    n = rlib.ctypes.c_int64(7)
    lib = rlib.load()
    assert lib.rnnt_ctc_loss_workspace(0, 4, 3, rlib.ctypes.byref(n)) == rlib.ERR_ARG and lib.rnnt_ctc_loss_workspace(2, 4, 256, rlib.ctypes.byref(n)) == rlib.ERR_SHAPE
    assert lib.rnnt_ctc_loss_workspace(2, 4, 3, None) == rlib.ERR_ARG and n.value == 7
    assert lib.rnnt_ctc_loss_workspace(2, 4, 3, rlib.ctypes.byref(n)) == 0 and n.value > 2 * 8 * (2 * 4 * 7)
    # the device entry points decide `elem` first and pointers next, before anything touches a GPU
    assert lib.rnnt_ctc_loss_elem(None, 32, 8, None, None, None, 1, 4, 0, 8, 0, 3, 1, None, None, None, 0, None) == rlib.ERR_ARG
    assert lib.rnnt_ctc_loss(None, 32, 8, None, None, None, 1, 4, 0, 8, 0, 1, None, None, None, 0, None) == rlib.ERR_ARG
    # functional: the library's status, or Python's own errors, before any result exists
    xt = torch.from_numpy(x).transpose(0, 1)
    for kw, status in ((dict(targets=torch.from_numpy(blank_label)), rlib.ERR_ARG), (dict(input_lengths=[7, 4, 1]), rlib.ERR_ARG),
                       (dict(target_lengths=[3, 3]), rlib.ERR_ARG), (dict(targets=torch.tensor([1, 1, 2])), rlib.ERR_ARG),
                       (dict(blank=V), rlib.ERR_ARG), (dict(targets=torch.zeros(B, 256, dtype=torch.int64)), rlib.ERR_SHAPE)):
        args = dict(targets=torch.from_numpy(TARGETS), input_lengths=list(TB), target_lengths=list(LB), blank=BLANK)
        args.update(kw)
        with pytest.raises(RnntError) as e:
            ctc_loss(xt, **args)
        assert e.value.status == status, kw
    with pytest.raises(RnntError):
        ctc_loss(xt[0], torch.from_numpy(TARGETS), TB, LB)
