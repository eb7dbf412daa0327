"""Cases, seeded inputs and yardsticks of the fused joint-and-loss tests (test_joint_loss_cpu.py, test_joint_loss.py), computed once
per process and shared read-only.  Shapes, e / p / w / b and the per-row lengths are joint_grad_cases.py's; the new kernels meet
them the same way:
  one     a single cell, the smallest V, no labels
  ragged  135 cells: a partial last forward tile, tiles that straddle batch rows, a last vocabulary tile 12 wide (a k-step of
          joint_loss_dz with 20 zero columns), per-row lengths with an empty transcript; joint_loss_dw's one step is partial
  u28     U1 = 28: two u-blocks of 16 in joint_loss_dz (the second 12 wide: de sums two partial slabs)
  v416    whole vocabulary tiles, 13 whole k-steps
  v20     two vocabulary tiles, one partial; one k-step with 12 zero columns
  tiles   35840 cells = 560 forward row tiles (> 512: the persistent multi-tile path of the lse form).  joint_loss_dz runs
          B NUB NC = 8 x 2 x 20 workgroups of TC = 8 frames (two iterations each; dp sums 20 partial slabs, de two); joint_loss_dw runs
          7 x 70 workgroups of 512 cells (16 steps each; dW and db sum 70 partial slabs).  Its float64 reference reads the 21672
          cells inside the rows' lengths and takes about ten seconds, once.
Every case runs with the per-row lengths of rows(name); the blank is spread over {0, 5, V - 1}; labels are drawn as the chain test of
test_joint_grad.py draws them."""
import numpy as np
import torch

import ctc_vr_amd.testing as T
import joint_grad_cases as G

D = G.D
SHAPES = G.SHAPES
# (name, scale, blank)
CASES = [("one", 1.0, 3), ("ragged", 1.0, 5), ("u28", 1.0, 0), ("v416", 1.0, 415), ("v20", 1.0, 5), ("ragged", 30.0, 5), ("tiles", 1.0, 0)]
BLANK = {(n, s): k for n, s, k in CASES}
NAMES = ("nll",) + G.NAMES
CLAMP = float(np.float32(0.01))   # the clamp of the clamp tests: the entry points take a float32, so the reference clamps at that value
_ROWS, _REF, _YARD = {}, {}, {}


def case(name, scale=1.0):
    """e, p, w, b float32; y [B, U1 - 1] int32 labels without the blank; (T_b, U_b) int32; blank"""
    B, Tn, U1, V, _ = SHAPES[name]
    e, p, w, b, _ = G.inputs(name, scale)
    ll, tl = G.rows(name)
    blank = BLANK[(name, scale)]
    r = np.random.Generator(np.random.Philox(key=[77, sorted(SHAPES).index(name)]))
    lab = r.integers(0, V - 1, (B, U1 - 1))
    y = np.where(lab >= blank, lab + 1, lab).astype(np.int32)
    return e, p, w, b, y, ll, tl, blank


def logits64(e, p, w, b):
    return (torch.tanh(torch.from_numpy(e).double().unsqueeze(2) + torch.from_numpy(p).double().unsqueeze(1)) @ torch.from_numpy(w).double().T
            + torch.from_numpy(b).double()).numpy()


def _rows64(name, scale):
    """per batch row (nll_b, d nll_b / d logits) in float64 through testing.transducer_loss_ref: the expensive part, once per case"""
    key = (name, scale)
    if key not in _ROWS:
        e, p, w, b, y, ll, tl, blank = case(name, scale)
        z = logits64(e, p, w, b)
        rows = [T.transducer_loss_ref(z[i], y[i], int(ll[i]), int(tl[i]), blank) for i in range(len(ll))]
        nll, g = np.array([r[0] for r in rows]), np.stack([r[1] for r in rows])
        nll.setflags(write=False)
        g.setflags(write=False)
        _ROWS[key] = (nll, g)
    return _ROWS[key]


def mean_scale(name):
    B = SHAPES[name][0]
    return np.full(B, 1.0 / B)


def reference(name, scale, row_scale=None, clamp=0.0):
    """(nll [B], de, dp, dW, db) float64 of sum_b row_scale[b] nll_b (row_scale None: the mean's 1 / B): tanh(e + p) W^T + b ->
    transducer_loss_ref -> clamp of d nll_b / d logits -> times row_scale[b] -> the joint's float64 autograd.  Shared, never written to."""
    rs = mean_scale(name) if row_scale is None else np.asarray(row_scale, np.float64)
    key = (name, scale, tuple(rs.tolist()), float(clamp))
    if key not in _REF:
        e, p, w, _, _, ll, tl, _ = case(name, scale)
        nll, g = _rows64(name, scale)
        g = np.clip(g, -clamp, clamp) if clamp > 0 else g
        want = (nll,) + tuple(T.joint_backward_ref(e, p, w, g * rs[:, None, None, None], ll, tl))
        for a in want:
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def grad_out(B):
    """a non-uniform d loss / d nll_b for reduction="none": exact in float32"""
    return np.array([1.0, -0.5, 2.0, 0.25, -1.5, 3.0, 0.75, -2.0][:B])


def emulation(name, scale, row_scale=None, clamp=0.0):
    """(nll, de, dp, dW, db) of the device's arithmetic contract on the CPU: joint_forward_emulation -> transducer_loss_f32_emulation
    -> g rounded to float32, clamped and scaled in float32 -> joint_backward_emulation.  row_scale None: the mean's 1 / B."""
    e, p, w, b, y, ll, tl, blank = case(name, scale)
    B = len(ll)
    rs = (mean_scale(name) if row_scale is None else np.asarray(row_scale)).astype(np.float32)
    z = T.joint_forward_emulation(e, p, w, b)
    rows = [T.transducer_loss_f32_emulation(z[i], y[i], int(ll[i]), int(tl[i]), blank) for i in range(B)]
    g32 = np.stack([r[1] for r in rows]).astype(np.float32)
    g32 = np.clip(g32, np.float32(-clamp), np.float32(clamp)) if clamp > 0 else g32
    return (np.array([r[0] for r in rows]),) + tuple(T.joint_backward_emulation(e, p, w, g32 * rs[:, None, None, None], ll, tl))


def distance(x, got, want):
    """relative for nll (per row), absolute for the gradients; the largest over the elements"""
    d = np.abs(np.asarray(got, np.float64) - want)
    return float((d / np.abs(want)).max() if x == "nll" else d.max())


def variants(kind):
    """(name, scale, row_scale or None, clamp) of a yardstick: "mean" is CASES with the mean's 1 / B; the others are the runs of the
    row-scale, sum and clamp tests, whose gradients (linear in the row scale) are of another size and get a yardstick of their own"""
    if kind == "mean":
        return [(n, s, None, 0.0) for n, s, _ in CASES]
    if kind == "none":
        return [(n, 1.0, grad_out(SHAPES[n][0]), 0.0) for n in ("ragged", "u28")]
    if kind == "sum":
        return [("ragged", 1.0, np.ones(SHAPES["ragged"][0]), 0.0)]
    assert kind == "clamp"
    return [("ragged", 1.0, None, CLAMP)]


def yardstick(kind="mean"):
    """{x: E_x}: the largest distance of emulation() from reference() over variants(kind)"""
    if kind not in _YARD:
        E = dict.fromkeys(NAMES, 0.0)
        for name, scale, rs, clamp in variants(kind):
            for x, a, want in zip(NAMES, emulation(name, scale, rs, clamp), reference(name, scale, rs, clamp)):
                assert np.isfinite(a).all()
                E[x] = max(E[x], distance(x, a, want))
        _YARD[kind] = E
    return dict(_YARD[kind])
