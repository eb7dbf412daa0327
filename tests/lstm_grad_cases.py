"""Shapes and seeded inputs of the predictor-LSTM gradient tests (test_lstm_grad_cpu.py, test_lstm_grad.py), and the float64 yardstick
with the measured error of the device's arithmetic contract, computed once per process and shared read-only.

Each shape is the smallest at which something specific can break (the recurrence kernels take 4 batch rows per workgroup):
  one     1 x 1: a single step, one live row in a tile
  ragged  3 x 5, lengths (5, 1, 3): rows stop at different steps inside one tile
  tile17  17 x 4: a second (here: fifth) row tile with one row
  u29     2 x 29: the workload's label count, a real chain
  long    2 x 256: the largest U1 the library accepts; two 256-row slabs in the dW / db reduce
  batch   64 x 29: several row tiles; dW and db reduce 1856 rows, so every slab reduce adds 8 partials
Every case runs with and without h0 / c0, and at scales 1 and 30 (pre-activations of order 30: most gates on the flat parts).
The other shapes get a derived ragged set for the length tests."""
import numpy as np

import ctc_vr_amd.testing as T

D = 256
# name: (B, U1, lengths or None)
SHAPES = {
    "one": (1, 1, None),
    "ragged": (3, 5, [5, 1, 3]),
    "tile17": (17, 4, None),
    "u29": (2, 29, None),
    "long": (2, 256, None),
    "batch": (64, 29, None),
}
SCALES = [1.0, 30.0]
CASES = [(n, s) for n in SHAPES for s in SCALES]
NAMES = T.LSTM_NAMES


def lens(name):
    """[B] int32 of the length tests: the stated lengths, or row b shortened by 3 b steps (cyclically, never below 1)"""
    B, U1, given = SHAPES[name]
    return np.array(given or [1 + (U1 - 1 - 3 * b) % U1 for b in range(B)], np.int32)


def inputs(name, scale):
    """x [B, U1, 256] ~ scale N(0, 1); w_ih, w_hh [1024, 256] ~ N(0, 1 / 16^2); b_ih, b_hh [1024] ~ 0.3 N(0, 1); h0, c0 [B, 256] ~
    0.5 N(0, 1); dout [B, U1, 256] ~ 0.05 N(0, 1); float32"""
    B, U1, _ = SHAPES[name]
    r = np.random.Generator(np.random.Philox(key=[100 + sorted(SHAPES).index(name), int(scale)]))
    f = np.float32
    x = (scale * r.standard_normal((B, U1, D))).astype(f)
    w_ih = (r.standard_normal((4 * D, D)) / 16.0).astype(f)
    w_hh = (r.standard_normal((4 * D, D)) / 16.0).astype(f)
    b_ih = (0.3 * r.standard_normal(4 * D)).astype(f)
    b_hh = (0.3 * r.standard_normal(4 * D)).astype(f)
    h0 = (0.5 * r.standard_normal((B, D))).astype(f)
    c0 = (0.5 * r.standard_normal((B, D))).astype(f)
    dout = (0.05 * r.standard_normal((B, U1, D))).astype(f)
    return {"x": x, "w_ih": w_ih, "w_hh": w_hh, "b_ih": b_ih, "b_hh": b_hh, "h0": h0, "c0": c0, "dout": dout}


def _args(name, scale, with_state, with_lens):
    a = inputs(name, scale)
    return (a["x"], a["w_ih"], a["w_hh"], a["b_ih"], a["b_hh"], a["dout"], a["h0"] if with_state else None, a["c0"] if with_state else None,
            lens(name) if with_lens else None)


_REF, _YARD = {}, {}


def reference(name, scale, with_state, with_lens):
    """(out, dx, dW_ih, dW_hh, db, dh0, dc0, hN, cN) float64 of a case by float64 torch autograd on the CPU: computed once, shared,
    never written to"""
    key = (name, scale, with_state, with_lens)
    if key not in _REF:
        want = T.lstm_ref(*_args(*key), final=True)
        for a in want:
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def yardstick():
    """{scale: {x: E_x}}: per scale and output the largest absolute distance of lstm_f32_emulation from reference() over every case of
    that scale, with and without h0 / c0 (lengths off: the cases as the table states them, plus `ragged` with its lengths)."""
    if not _YARD:
        for scale in SCALES:
            E = dict.fromkeys(NAMES, 0.0)
            for name in SHAPES:
                for with_state in (False, True):
                    for with_lens in ((False, True) if SHAPES[name][2] else (False,)):
                        emu = T.lstm_f32_emulation(*_args(name, scale, with_state, with_lens))
                        for x, a, b in zip(NAMES, emu, reference(name, scale, with_state, with_lens)):
                            assert np.isfinite(a).all()
                            E[x] = max(E[x], float(np.abs(a - b).max()))
            _YARD[scale] = E
    return {s: dict(E) for s, E in _YARD.items()}
