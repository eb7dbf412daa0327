"""Shapes and seeded inputs of the attention gradient tests (test_attention_grad_cpu.py, test_attention_grad.py), and the float64
yardstick with the measured error of the device's arithmetic contract, computed once per process and shared read-only.

Each case is the smallest at which something specific can break.  The kernels take 16 query rows and 16 keys per tile, the tile the
issue's table assumes, so the tile-edge cases stand as it states them:
  one     1 x 1: one key -- ds and dq, dk, dp, du, dvb are exactly 0 in exact arithmetic
  t17     1 x 17: a second query tile and a second key tile with one row
  causal  2 x 9, chunk 1: the window's upper edge moves every row
  dead    3 x 13, lengths (13, 5, 1), chunk 4, one left chunk: rows with no visible key; a window whose lower edge moves
  c16     2 x 70, lengths (70, 33), chunk 16: chunk edge = tile edge; a length inside a tile
  c25     2 x 130, lengths (130, 77), chunk 25, two left chunks: chunk edges off the tile grid; leading key tiles skipped
  work    2 x 249, lengths (249, 200), chunk 16: the workload's T
  workf   the same, full context
  batch   16 x 64, chunk 16: the dp reduce over 16 rows, du / dvb over all 64 (row, tile) partials
Every case runs at scales 1 (scores of order 1) and 3 (near one-hot rows)."""
import numpy as np

import ctc_vr_amd.testing as T

D = 256
# name: (B, T, lengths or None, chunk_size, num_left_chunks)
SHAPES = {
    "one": (1, 1, None, 0, -1),
    "t17": (1, 17, None, 0, -1),
    "causal": (2, 9, None, 1, -1),
    "dead": (3, 13, [13, 5, 1], 4, 1),
    "c16": (2, 70, [70, 33], 16, -1),
    "c25": (2, 130, [130, 77], 25, 2),
    "work": (2, 249, [249, 200], 16, -1),
    "workf": (2, 249, [249, 200], 0, -1),
    "batch": (16, 64, None, 16, -1),
}
SCALES = [1.0, 3.0]
CASES = [(n, s) for n in SHAPES for s in SCALES]
NAMES = T.ATTN_NAMES


def mask(name):
    """(lengths [B] int32 or None, chunk_size, num_left_chunks)"""
    _, _, lens, chunk, left = SHAPES[name]
    return None if lens is None else np.array(lens, np.int32), chunk, left


def inputs(name, scale):
    """q, k [B, T, 256], p [T, 256] ~ scale N(0, 1); v ~ N(0, 1); u, vb [4, 64] ~ 0.3 scale N(0, 1); dout ~ 0.05 N(0, 1); float32"""
    B, Tn = SHAPES[name][:2]
    r = np.random.Generator(np.random.Philox(key=[300 + sorted(SHAPES).index(name), int(scale)]))
    f = np.float32
    q = (scale * r.standard_normal((B, Tn, D))).astype(f)
    k = (scale * r.standard_normal((B, Tn, D))).astype(f)
    p = (scale * r.standard_normal((Tn, D))).astype(f)
    v = r.standard_normal((B, Tn, D)).astype(f)
    u = (0.3 * scale * r.standard_normal((4, 64))).astype(f)
    vb = (0.3 * scale * r.standard_normal((4, 64))).astype(f)
    dout = (0.05 * r.standard_normal((B, Tn, D))).astype(f)
    return {"q": q, "k": k, "v": v, "p": p, "u": u, "vb": vb, "dout": dout}


def _args(name, scale):
    a = inputs(name, scale)
    return (a["q"], a["k"], a["v"], a["p"], a["u"], a["vb"], a["dout"]) + mask(name)


_REF, _EMU, _YARD = {}, {}, {}


def reference(name, scale):
    """(out, dq, dk, dv, dp, du, dvb) float64 of a case by float64 torch autograd on the CPU: computed once, shared, never written to"""
    key = (name, scale)
    if key not in _REF:
        want = T.rel_attention_ref(*_args(*key))
        for a in want:
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def emulation(name, scale):
    key = (name, scale)
    if key not in _EMU:
        _EMU[key] = T.rel_attention_emulation(*_args(*key))
    return _EMU[key]


def yardstick():
    """{scale: {x: E_x}}: per scale and output the largest absolute distance of rel_attention_emulation from reference() over every
    case of that scale."""
    if not _YARD:
        for scale in SCALES:
            E = dict.fromkeys(NAMES, 0.0)
            for name in SHAPES:
                for x, a, b in zip(NAMES, emulation(name, scale), reference(name, scale)):
                    assert np.isfinite(a).all()
                    E[x] = max(E[x], float(np.abs(a - b).max()))
            _YARD[scale] = E
    return {s: dict(E) for s, E in _YARD.items()}


def reference_scale():
    """{scale: {x: max |reference|}} over the cases: what the yardstick-sanity bound of 1e-3 is relative to"""
    return {s: {x: max(float(np.abs(reference(n, s)[i]).max()) for n in SHAPES) for i, x in enumerate(NAMES)} for s in SCALES}
