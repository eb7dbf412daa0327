"""Generates tests/golden/timestamps_cases.npz: inputs and outputs of the reference's gen_ctc_peak_time and
gen_timestamps_from_peak (wenet/utils/ctc_utils.py) on seeded cases.  Run where the read-only reference is present (the build
container); never imported by tests, bench or the product.

ctc_utils.py imports torchaudio.functional at the top (for force_align, a torchaudio call that cannot be pinned this way);
torchaudio is absent, so stub modules are registered first.  Only data goes into the fixture.

Layout of the fixture (ragged lists flattened, case i = [off[i], off[i + 1])):
  hyp_flat / hyp_off, hyp_blank [Nh]          -> peak_flat / peak_off                       (gen_ctc_peak_time)
  ts_peaks_flat / ts_peaks_off, ts_args [Nt, 3] = (max_duration, frame_rate, max_token_duration) -> ts_times_flat [sum, 2] float64
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "timestamps_cases.npz")


def load_ctc_utils():
    for name in ("torchaudio", "torchaudio.functional"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchaudio"].functional = sys.modules["torchaudio.functional"]
    spec = importlib.util.spec_from_file_location("ref_ctc_utils", f"{REF}/wenet/utils/ctc_utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def flatten(lists, dtype):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int64)
    flat = np.array([v for x in lists for v in x], dtype)
    return flat, off


def main():
    cu = load_ctc_utils()
    g = np.random.Generator(np.random.Philox(key=[2024, 0xA11]))
    # per-frame alignments: runs of blanks and labels, adjacent repeats separated by a blank or not, empty and all-blank rows
    hyps, blanks = [[]], [0]
    for i in range(100):
        blank = int(g.integers(0, 4))
        n = int(g.integers(1, 40))
        hyp = []
        while len(hyp) < n:
            hyp += [int(g.integers(0, 5))] * int(g.integers(1, 5))
        hyps.append(hyp[:n] if i % 10 else [blank] * n)
        blanks.append(blank)
    peaks_out = [cu.gen_ctc_peak_time(h, b) for h, b in zip(hyps, blanks)]
    # peak lists: empty, single, closer and farther apart than max_token_duration, max_duration clipping the last end
    peak_lists, args = [], []
    for i in range(100):
        frame_rate = [0.04, 0.04, 0.01, 0.08][i % 4]
        max_tok = [1.0, 1.0, 0.5, 2.0, 0.3][i % 5]
        n = [0, 1, 2, 3, 7, 20][i % 6]
        wide = int(2 * max_tok / frame_rate) + 2                  # gaps up to twice the token duration
        gaps = g.integers(0 if i % 3 == 0 else 1, wide, n)        # i % 3 == 0: equal neighbouring peaks too (transducer emissions)
        pk = (int(g.integers(0, 30)) + np.cumsum(gaps)).tolist()
        last = pk[-1] * frame_rate if pk else 1.0
        max_duration = [last + 10.0, last + 0.1 * max_tok, last, (pk[-1] + 1) * frame_rate if pk else 0.0][(i // 6) % 4]
        peak_lists.append([int(v) for v in pk])
        args.append((float(max_duration), frame_rate, max_tok))
    times = [cu.gen_timestamps_from_peak(p, a[0], a[1], a[2]) for p, a in zip(peak_lists, args)]
    assert any(len(p) == 0 for p in peak_lists) and any(len(p) == 1 for p in peak_lists)
    hyp_flat, hyp_off = flatten(hyps, np.int64)
    peak_flat, peak_off = flatten(peaks_out, np.int64)
    tp_flat, tp_off = flatten(peak_lists, np.int64)
    tt = np.array([[float(s), float(e)] for ts in times for s, e in ts], np.float64).reshape(-1, 2)
    np.savez_compressed(OUT, hyp_flat=hyp_flat, hyp_off=hyp_off, hyp_blank=np.array(blanks, np.int64), peak_flat=peak_flat, peak_off=peak_off,
                        ts_peaks_flat=tp_flat, ts_peaks_off=tp_off, ts_args=np.array(args, np.float64), ts_times_flat=tt)
    print(f"wrote {OUT}: {len(hyps)} alignments, {len(peak_lists)} peak lists, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
