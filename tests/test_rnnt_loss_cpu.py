"""The transducer loss with gradients, without a GPU: rnnt_transducer_loss_host (the plain C++ twin of the device entry point)
against float64 autograd through the alpha recursion, against the enumeration of all alignments, and ctc_vr_amd.functional.rnnt_loss
on CPU tensors (reductions, blank = -1, clamp, fused_log_softmax=False, an upstream gradient, refusals)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.functional import rnnt_loss
from ctc_vr_amd.lib import RnntError

REC_RTOL = 1e-9                   # the project's bar for an f64 recursion against its float64 restatement (test_score.py)

# (T_b, U_b, V, blank): one frame, an empty transcript, V odd / even / unaligned rows / the constructor default
CASES = [(1, 0, 8, 0), (1, 3, 8, 0), (5, 0, 7, 6), (7, 4, 412, 5), (33, 12, 412, 5), (5, 3, 413, 5), (4, 2, 4336, 4335)]
TINY = [c for c in CASES if math.comb(c[0] - 1 + c[1], c[1]) <= 1000]


def _labels(g, n, V, blank):
    y = g.integers(0, V - 1, n)
    return np.where(y >= blank, y + 1, y).astype(np.int32)         # uniform over the non-blank labels


def _case(i, fused=True):
    Tb, Ub, V, blank = CASES[i]
    g = np.random.Generator(np.random.Philox(key=[i, 0x105]))
    x = (3.0 * g.standard_normal((Tb, Ub + 1, V))).astype(np.float32)
    if not fused:
        x = torch.log_softmax(torch.from_numpy(x).double(), -1).float().numpy()
    return x, _labels(g, Ub, V, blank)


_REF = {}


def _ref(i, fused=True):
    """(logits, targets, nll, grad) of case i by float64 autograd: computed once, shared, never written to"""
    if (i, fused) not in _REF:
        x, y = _case(i, fused)
        Tb, Ub, V, blank = CASES[i]
        nll, grad = T.transducer_loss_ref(x, y, Tb, Ub, blank, fused)
        for a in (x, y, grad):
            a.setflags(write=False)
        _REF[(i, fused)] = (x, y, nll, grad)
    return _REF[(i, fused)]


def _close(got, want, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    bound = REC_RTOL * np.maximum(1.0, np.abs(want))
    assert (err <= bound).all(), f"{what}: max error {err.max():.3e}"


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_host_twin_single_rows_vs_float64_autograd(i, fused):
    x, y, want_nll, want_grad = _ref(i, fused)
    Tb, Ub, V, blank = CASES[i]
    nll, grad = rlib.transducer_loss_host(x[None], y.reshape(1, Ub), [Tb], [Ub], blank, fused)
    print(f"case {CASES[i]} fused={fused}: nll {nll[0]!r} ref {want_nll!r}, max |grad - ref| {np.abs(grad[0] - want_grad).max():.3e}")
    _close(nll[0], want_nll, "nll")
    _close(grad[0], want_grad, "grad")
    nll_only, none = rlib.transducer_loss_host(x[None], y.reshape(1, Ub), [Tb], [Ub], blank, fused, want_grad=False)
    assert none is None and nll_only[0] == nll[0]


GROUPS = sorted({c[2:] for c in CASES})                          # cases that share (V, blank) can share a batch


def _packed(V=412, blank=5):
    """the cases of one (V, blank) as rows of one ragged batch, one frame and one label longer than its longest row: NaN in every
    padding cell, -1 in the target padding"""
    rows = [i for i, c in enumerate(CASES) if c[2:] == (V, blank)]
    Tn, Umax = max(CASES[i][0] for i in rows) + 1, max(CASES[i][1] for i in rows) + 1
    x = np.full((len(rows), Tn, Umax + 1, V), np.nan, np.float32)
    y = np.full((len(rows), Umax), -1, np.int32)
    for b, i in enumerate(rows):
        xi, yi = _case(i)
        Tb, Ub = CASES[i][:2]
        x[b, :Tb, :Ub + 1] = xi
        y[b, :Ub] = yi
    return rows, x, y, np.array([CASES[i][0] for i in rows], np.int32), np.array([CASES[i][1] for i in rows], np.int32)


@pytest.mark.parametrize("group", GROUPS)
def test_host_twin_ragged_batch_with_nan_padding(group):
    rows, x, y, Tb, Ub = _packed(*group)
    assert np.isnan(x).any()
    nll, grad = rlib.transducer_loss_host(x, y, Tb, Ub, group[1])
    for b, i in enumerate(rows):
        _, _, want_nll, want_grad = _ref(i)
        _close(nll[b], want_nll, f"nll of row {b}")
        _close(grad[b, :Tb[b], :Ub[b] + 1], want_grad, f"grad of row {b}")
        pad = np.ones(grad.shape[1:3], bool)
        pad[:Tb[b], :Ub[b] + 1] = False
        assert pad.any() and not grad[b][pad].view(np.uint64).any(), "a padding cell's gradient is not exactly 0"
    assert np.isfinite(grad).all()


@pytest.mark.parametrize("i", [CASES.index(c) for c in TINY])
def test_nll_vs_enumeration_of_alignments(i):
    x, y, _, _ = _ref(i)
    Tb, Ub, V, blank = CASES[i]
    lp = torch.log_softmax(torch.from_numpy(x.copy()).double(), -1).numpy()
    pick = np.zeros((Tb, Ub + 1, 2))
    pick[..., 0] = lp[..., blank]
    for u in range(Ub):
        pick[:, u, 1] = lp[:, u, y[u]]
    want = T.transducer_nll_bruteforce(pick, Tb, Ub)
    nll, _ = rlib.transducer_loss_host(x[None], y.reshape(1, Ub), [Tb], [Ub], blank, want_grad=False)
    assert abs(nll[0] - want) <= REC_RTOL * abs(want), (nll[0], want)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_gradient_sums_to_zero_per_cell(i):
    x, y, _, _ = _ref(i)
    Tb, Ub, V, blank = CASES[i]
    _, grad = rlib.transducer_loss_host(x[None], y.reshape(1, Ub), [Tb], [Ub], blank)
    assert np.abs(grad[0].sum(-1)).max() <= 1e-12


# ---- rnnt_loss on CPU tensors ---------------------------------------------------------------------------------------------------------
def _batch():
    rows, x, y, Tb, Ub = _packed()
    return torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(Tb), torch.from_numpy(Ub)


def _grad_of(loss_fn):
    x, y, Tb, Ub = _batch()
    x.requires_grad_(True)
    loss = loss_fn(x, y, Tb, Ub)
    loss.backward()
    return loss.detach(), x.grad


def test_rnnt_loss_reductions_and_upstream_gradient():
    x, y, Tb, Ub = _batch()
    none = rnnt_loss(x, y, Tb, Ub, blank=5, reduction="none")
    assert none.shape == (2,) and none.dtype == torch.float32
    nll, grad = rlib.transducer_loss_host(x.numpy(), y.numpy(), Tb.numpy(), Ub.numpy(), 5)
    assert torch.equal(none, torch.from_numpy(nll).float())
    assert torch.equal(rnnt_loss(x, y, Tb, Ub, blank=5, reduction="mean"), none.mean()) and torch.equal(rnnt_loss(x, y, Tb, Ub, blank=5), none.mean())
    assert torch.equal(rnnt_loss(x, y, Tb, Ub, blank=5, reduction="sum"), none.sum())
    g32 = torch.from_numpy(grad.astype(np.float32))
    _, g_sum = _grad_of(lambda *a: rnnt_loss(*a, blank=5, reduction="sum"))
    assert torch.equal(g_sum, g32)
    _, g_mean = _grad_of(lambda *a: rnnt_loss(*a, blank=5, reduction="mean"))
    assert torch.equal(g_mean, g32 * 0.5)                         # 1 / B, B = 2 (the two V = 412 rows)
    _, g_none = _grad_of(lambda *a: (rnnt_loss(*a, blank=5, reduction="none") * torch.tensor([1.0, 3.0])).sum())
    assert torch.equal(g_none[0], g32[0]) and torch.equal(g_none[1], g32[1] * 3.0)
    _, g_up = _grad_of(lambda *a: 2.5 * rnnt_loss(*a, blank=5, reduction="sum"))
    assert torch.equal(g_up, g32 * 2.5)
    with pytest.raises(ValueError):
        rnnt_loss(x, y, Tb, Ub, blank=5, reduction="batchmean")
    with pytest.raises(TypeError):
        rnnt_loss(x.double(), y, Tb, Ub, blank=5)
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)           # same values, not contiguous
    assert not xt.is_contiguous() and torch.equal(rnnt_loss(xt, y, Tb, Ub, blank=5, reduction="none"), none)


def test_rnnt_loss_blank_default_is_last_label():
    i = CASES.index((4, 2, 4336, 4335))
    x, y, want_nll, _ = _ref(i)
    got = rnnt_loss(torch.from_numpy(x.copy())[None], torch.from_numpy(y.copy())[None], torch.tensor([4]), torch.tensor([2]), reduction="none")
    assert abs(float(got[0]) - want_nll) <= 2.0 ** -23 * want_nll
    with pytest.raises(RnntError):                                # 4335 as a label is the blank now
        rnnt_loss(torch.from_numpy(x.copy())[None], torch.tensor([[4335, 1]]), torch.tensor([4]), torch.tensor([2]))


def test_rnnt_loss_clamp_acts_before_the_batch_scaling():
    loss, g = _grad_of(lambda *a: rnnt_loss(*a, blank=5, reduction="mean"))
    loss_c, g_c = _grad_of(lambda *a: rnnt_loss(*a, blank=5, clamp=0.1, reduction="mean"))
    assert torch.equal(loss, loss_c)
    assert (g.abs() * 2 > 0.1).any(), "the case does not exercise the clamp"
    _, g_sum = _grad_of(lambda *a: rnnt_loss(*a, blank=5, reduction="sum"))
    assert float((g_c * 2).abs().max()) == np.float32(0.1)
    assert torch.equal(g_c, g_sum.clamp(-0.1, 0.1) * 0.5)


def test_rnnt_loss_on_log_probabilities():
    """fused_log_softmax=False on log_softmax(logits): the gradient is the float64 autograd gradient with respect to the
    log-probabilities (the host-twin test above, through rnnt_loss here), and nll is the fused call's up to the float32 rounding of
    the log-probabilities: 2^-24 |lp| on each of the T_b + U_b terms of a path, plus half an ulp of the float32 results."""
    i = CASES.index((7, 4, 412, 5))
    x, y, _, _ = _ref(i)
    lp, _, want_nll, want_grad = _ref(i, fused=False)
    args = (torch.from_numpy(y.copy())[None], torch.tensor([7]), torch.tensor([4]))
    fused = rnnt_loss(torch.from_numpy(x.copy())[None], *args, blank=5, reduction="none")
    lpt = torch.from_numpy(lp.copy())[None].requires_grad_(True)
    plain = rnnt_loss(lpt, *args, blank=5, reduction="none", fused_log_softmax=False)
    plain.sum().backward()
    bound = (7 + 4) * 2.0 ** -24 * float(np.abs(lp).max()) + 2.0 ** -23 * float(fused[0])
    assert abs(float(plain[0].detach()) - float(fused[0])) <= bound
    assert abs(float(plain[0].detach()) - want_nll) <= 2.0 ** -23 * want_nll
    assert np.abs(lpt.grad[0].numpy() - want_grad).max() <= 2.0 ** -24      # float32 storage of values in [-1, 1]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def _raw_host(x, tg, ll, tl, B, Tn, Umax, V, blank, nll, grad):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return rlib.load().rnnt_transducer_loss_host(p(x), p(tg), p(ll), p(tl), B, Tn, Umax, V, blank, 1, -1.0, p(nll), p(grad))


def test_refusals():
    B, Tn, Umax, V, blank = 2, 4, 3, 8, 2
    g = np.random.Generator(np.random.Philox(key=[9, 9]))
    x = g.standard_normal((B, Tn, Umax + 1, V)).astype(np.float32)
    ll, tl = np.array([4, 2], np.int32), np.array([3, 1], np.int32)
    tg = np.array([[7, 0, 3], [1, -5, blank]], np.int32)           # row 1's entries beyond its length are invalid on purpose
    base = dict(x=x, tg=tg, ll=ll, tl=tl, B=B, Tn=Tn, Umax=Umax, V=V, blank=blank)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        nll, grad = np.full(a["B"], 7.0), np.full(x.shape, 7.0)
        rc = _raw_host(a["x"], a["tg"], a["ll"], a["tl"], a["B"], a["Tn"], a["Umax"], a["V"], a["blank"], None if kw.get("no_nll") else nll, grad)
        return rc, nll, grad

    rc, nll, grad = call()
    assert rc == 0 and np.isfinite(nll).all() and not (grad == 7.0).any()
    A, S = rlib.ERR_ARG, rlib.ERR_SHAPE
    refusals = [(A, dict(x=None)), (A, dict(tg=None)), (A, dict(ll=None)), (A, dict(tl=None)), (A, dict(no_nll=True)), (A, dict(B=0)),
                (A, dict(ll=np.array([0, 2], np.int32))), (A, dict(ll=np.array([4, 5], np.int32))),
                (A, dict(tl=np.array([-1, 1], np.int32))), (A, dict(tl=np.array([3, 4], np.int32))),
                (A, dict(V=1, blank=0)), (A, dict(blank=-1)), (A, dict(blank=V)),
                (A, dict(tg=np.array([[7, V, 3], [1, 0, 0]], np.int32))), (A, dict(tg=np.array([[7, -1, 3], [1, 0, 0]], np.int32))),
                (A, dict(tg=np.array([[7, blank, 3], [1, 0, 0]], np.int32))),
                (S, dict(Umax=256, tg=np.ones((B, 256), np.int32)))]
    for code, kw in refusals:
        rc, nll, grad = call(**kw)
        assert rc == code, (list(kw), rc)
        assert (nll == 7.0).all() and (grad == 7.0).all(), f"a refused call wrote something: {list(kw)}"
    xt, yt = torch.from_numpy(x), torch.from_numpy(np.maximum(tg, 0))
    for kw, code in [(dict(logit_lengths=torch.tensor([4, 5])), A), (dict(target_lengths=torch.tensor([3, 4])), A), (dict(blank=V), A),
                     (dict(targets=torch.tensor([[7, blank, 3], [1, 0, 0]])), A)]:
        a = dict(targets=yt, logit_lengths=torch.from_numpy(ll), target_lengths=torch.from_numpy(tl), blank=blank)
        a.update(kw)
        with pytest.raises(RnntError) as e:
            rnnt_loss(xt, **a)
        assert e.value.status == code and "status" in str(e.value)


def test_umax_255_is_accepted_and_256_refused():
    g = np.random.Generator(np.random.Philox(key=[255, 1]))
    for Umax, code in [(255, 0), (256, rlib.ERR_SHAPE)]:
        x = g.standard_normal((1, 2, Umax + 1, 3)).astype(np.float32)
        tg = (np.arange(Umax, dtype=np.int32) % 2)[None]           # labels 0 and 1, blank 2
        nll = np.full(1, np.nan)
        rc = _raw_host(x, tg, np.array([2], np.int32), np.array([Umax], np.int32), 1, 2, Umax, 3, 2, nll, None)
        assert rc == code and np.isfinite(nll[0]) == (code == 0)
    with pytest.raises(RnntError) as e:
        rnnt_loss(torch.zeros(1, 2, 257, 3), torch.zeros(1, 256, dtype=torch.int32), torch.tensor([2]), torch.tensor([256]))
    assert e.value.status == rlib.ERR_SHAPE


def test_workspace_size():
    n = rlib.transducer_loss_workspace(3, 5, 4)
    cells = 3 * 5 * 4
    assert n == 8 * (4 + 2 * cells) + 4 * (7 * cells) + 4 * (2 * 3 + 3 * 3) and n % 4 == 0
    with pytest.raises(RnntError):
        rlib.transducer_loss_workspace(1, 1, 257)
