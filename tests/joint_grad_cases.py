"""Shapes and seeded inputs of the joint-lattice gradient tests (test_joint_grad_cpu.py, test_joint_grad.py), and the float64
yardstick with the measured error of the device's arithmetic contract, computed once per process and shared read-only.

Each shape is the smallest at which something specific can break (M = B T U1 cells, u fastest):
  one     a single cell, the smallest V
  ragged  135 cells: a partial last forward tile, tiles that straddle batch rows, a last vocabulary tile 12 wide; per-row lengths
  u28     U1 = 28: two u-blocks of 16 in joint_grad_dz (the second 12 wide: de sums two partial slabs), frames span forward tiles
  v416    whole vocabulary tiles, 13 whole k-steps of dh
  v20     two vocabulary tiles, one partial; one k-step of dh with 12 zero columns
  tiles   35840 cells = 560 forward tiles (> 2 x 256 workgroups: the persistent multi-tile path).  For the backward: joint_grad_dz
          runs B NUB NC = 8 x 2 x 20 workgroups of TC = 8 frames (two iterations each, dp sums 20 partial slabs, de two);
          joint_grad_dw runs 7 x 70 workgroups of 512 cells (16 k-steps each, dW and db sum 70 partial slabs).  So this shape is
          the one at which every workgroup of either backward kernel takes several tiles and every slab reduce several partials.
rows (T_b, U_b) are the issue's for `ragged`; the other shapes get a derived ragged set for the length tests, full lengths otherwise."""
import numpy as np

import ctc_vr_amd.testing as T

D = 256
# name: (B, T, U1, V, rows or None)
SHAPES = {
    "one": (1, 1, 1, 4, None),
    "ragged": (3, 9, 5, 412, [(9, 4), (1, 0), (5, 2)]),
    "u28": (2, 7, 28, 412, None),
    "v416": (2, 5, 3, 416, None),
    "v20": (2, 5, 3, 20, None),
    "tiles": (8, 160, 28, 412, None),
}
SCALES = [1.0, 30.0]              # 30: exp2 overflows, h = +-1 exactly, 1 - h^2 must be exactly 0
CASES = [(n, s) for n in SHAPES for s in SCALES]


def rows(name):
    """(T_b [B], U_b [B]) int32 of the length tests: the stated rows, or row b shortened by 2 b frames and 3 b labels"""
    B, Tn, U1, _, given = SHAPES[name]
    r = given or [(max(1, Tn - 2 * b), max(0, U1 - 1 - 3 * b)) for b in range(B)]
    return np.array([x[0] for x in r], np.int32), np.array([x[1] for x in r], np.int32)


def inputs(name, scale):
    """e [B, T, 256], p [B, U1, 256] ~ scale N(0, 1); w [V, 256] ~ N(0, 1 / 16^2); b [V]; g [B, T, U1, V] ~ 0.05 N(0, 1); float32"""
    B, Tn, U1, V, _ = SHAPES[name]
    r = np.random.Generator(np.random.Philox(key=[sorted(SHAPES).index(name), int(scale)]))
    f = np.float32
    e = (scale * r.standard_normal((B, Tn, D))).astype(f)
    p = (scale * r.standard_normal((B, U1, D))).astype(f)
    w = (r.standard_normal((V, D)) / 16.0).astype(f)
    b = (0.3 * r.standard_normal(V)).astype(f)
    g = (0.05 * r.standard_normal((B, Tn, U1, V))).astype(f)
    return e, p, w, b, g


NAMES = ("de", "dp", "dW", "db")
_REF, _YARD = {}, {}


def reference(name, scale, with_lens):
    """(de, dp, dW, db) float64 of a case by float64 torch autograd on the CPU: computed once, shared, never written to"""
    key = (name, scale, with_lens)
    if key not in _REF:
        e, p, w, _, g = inputs(name, scale)
        ll, tl = rows(name) if with_lens else (None, None)
        want = T.joint_backward_ref(e, p, w, g, ll, tl)
        for a in want:
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def yardstick():
    """{x: E_x}: per output the largest absolute distance of joint_backward_emulation from reference() over every case, with and
    without lengths."""
    if not _YARD:
        E = dict.fromkeys(NAMES, 0.0)
        for name, scale in CASES:
            e, p, w, _, g = inputs(name, scale)
            for with_lens in (False, True):
                ll, tl = rows(name) if with_lens else (None, None)
                emu = T.joint_backward_emulation(e, p, w, g, ll, tl)
                for x, a, b in zip(NAMES, emu, reference(name, scale, with_lens)):
                    assert np.isfinite(a).all()
                    E[x] = max(E[x], float(np.abs(a - b).max()))
        _YARD.update(E)
    return dict(_YARD)
