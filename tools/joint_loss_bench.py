"""The fused joint and loss at training shapes: what transducer_joint_loss costs forward, backward and as a whole step, against the
unfused chain transducer_joint -> rnnt_loss -> backward of the same build in the same process, with the peak memory of each.

Shapes: B16 and B64 x T249 x U28 x V412, full-length rows, seeded inputs.  Each shape runs in a child process of its own under
`timeout -k 10` (a shape that faults or hangs ends the run: nothing more is started).  Per shape, whole calls by device events over
`--iters` calls after `--warmup` calls, `--reps` repetitions with the legs alternating (36 samples per leg by default; median, min, max):
  * forward:  the loss from e, p, W, b (fused: no gradient is formed; unfused: rnnt_loss forms d nll / d logits eagerly, as it does);
  * backward: torch.autograd.grad of a held loss;
  * step:     forward and the gradients of the four leaves.
The two entry points of the fused path are also timed alone over preallocated buffers (rnnt_joint_loss_forward, rnnt_joint_loss_backward):
their share of the fused step is what the kernels cost, the rest is allocation and autograd.
What the algorithm needs, from the shapes: three bf16x3 contractions of the lattice (forward, and its recomputation in joint_loss_dz and
joint_loss_dw: 3 x 3 x 2 M V 256 FLOPs) plus dh = g W and dW = g^T h (2 x 3 x 2 M V 256); bytes: e, p and W read three times, coef
written once and read twice (16 M each), pick and lse, alpha and beta (f64), the partial slabs written and read once.  `floor_ms` is
the larger of those bytes at the HBM rate a float4 copy reaches on this part and those FLOPs at the bf16 MFMA peak.
Peak memory: torch.cuda.max_memory_allocated over one step, above what was allocated before it.  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/joint_loss_bench.py [--out profiles/joint_loss_bench.json] [--iters 12] [--warmup 3] [--reps 3] [--limit 240]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BPS = 6.29e12            # measured float4 copy rate of the MI355X (8.0 TB/s spec)
MFMA_BF16_FLOPS = 2.5e15          # bf16 MFMA peak (16 x the 157.3 TFLOPS of f32)
SHAPES = [(16, 249, 28, 412), (64, 249, 28, 412)]
D = 256


def one_shape(B, Tn, U1, V, args):
    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib
    from ctc_vr_amd.functional import rnnt_loss, transducer_joint, transducer_joint_loss

    assert torch.cuda.is_available(), "joint_loss_bench needs a GPU: there is no CPU timing"
    dev = torch.device("cuda", 0)
    r = np.random.Generator(np.random.Philox(key=[B, 0x102]))
    f = np.float32
    leaves = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (
        r.standard_normal((B, Tn, D)).astype(f), r.standard_normal((B, U1, D)).astype(f), (r.standard_normal((V, D)) / 16.0).astype(f),
        (0.3 * r.standard_normal(V)).astype(f))]
    blank = 5
    lab = r.integers(0, V - 1, (B, U1 - 1))
    y_np = np.where(lab >= blank, lab + 1, lab).astype(np.int32)
    y = torch.from_numpy(y_np).to(dev)
    ll, tl = torch.full((B,), Tn, dtype=torch.int32, device=dev), torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
    losses = {"fused": lambda: transducer_joint_loss(*leaves, y, ll, tl, blank=blank, reduction="mean"),
              "unfused": lambda: rnnt_loss(transducer_joint(*leaves, ll, tl), y, ll, tl, blank=blank, reduction="mean")}
    legs, held = {}, {}
    for k, loss in losses.items():
        held[k] = loss()                                           # one graph per side, kept for the backward leg
        legs[k + "_forward"] = loss
        legs[k + "_backward"] = (lambda k=k: torch.autograd.grad(held[k], leaves, retain_graph=True))
        legs[k + "_step"] = (lambda loss=loss: torch.autograd.grad(loss(), leaves))
    # the two entry points alone, over buffers allocated once
    wbytes, sbytes = rlib.joint_loss_workspace(B, Tn, U1, V)
    work, state = torch.empty(wbytes, dtype=torch.uint8, device=dev), torch.empty(sbytes, dtype=torch.uint8, device=dev)
    nll, rs = torch.empty(B, dtype=torch.float64, device=dev), torch.full((B,), 1.0 / B, device=dev)
    outs = [torch.empty_like(t) for t in leaves]
    ptrs = [t.data_ptr() for t in leaves]
    ll_np, tl_np = np.full(B, Tn, np.int32), np.full(B, U1 - 1, np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    legs["entry_forward"] = lambda: rlib.joint_loss_forward_device(*ptrs, y_np, ll_np, tl_np, (B, Tn, U1, V), blank, nll.data_ptr(), state.data_ptr(), sbytes,
                                                                   work.data_ptr(), wbytes, stream)
    legs["entry_backward"] = lambda: rlib.joint_loss_backward_device(*ptrs, state.data_ptr(), sbytes, rs.data_ptr(), -1.0, (B, Tn, U1, V), blank,
                                                                     *(o.data_ptr() for o in outs), work.data_ptr(), wbytes, stream)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    first = [t.clone() for t in legs["fused_backward"]()]
    agree = {n: float((a - b).abs().max()) for n, a, b in zip(("de", "dp", "dW", "db"), first, legs["unfused_backward"]())}
    loss_agree = abs(float(held["fused"]) - float(held["unfused"]))
    times = {k: [] for k in legs}
    for _ in range(args.reps):
        for k, fn in legs.items():
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
                del out
    assert all(torch.equal(a, b) for a, b in zip(first, legs["fused_backward"]())), "the fused backward changed between calls"
    held.clear()
    peak = {}
    for k in losses:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = legs[k + "_step"]()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
        del out
    M = B * Tn * U1
    flops = 15 * 2 * M * V * D
    slabs = wbytes                                                 # the backward's workspace is its slabs and the packed stream
    nbytes = 3 * 4 * (B * Tn * D + B * U1 * D + V * D) + 3 * 16 * M + 2 * 12 * M + 2 * 16 * M + 2 * slabs
    row = {"B": B, "T": Tn, "U1": U1, "V": V, "cells": M, "lattice_bytes": 4 * M * V, "work_bytes": wbytes, "state_bytes": sbytes,
           "samples_per_leg": args.iters * args.reps, "floor_flops": flops, "floor_bytes": nbytes,
           "floor_ms": 1e3 * max(flops / MFMA_BF16_FLOPS, nbytes / HBM_COPY_BPS), "peak_step_bytes": peak,
           "fused_vs_unfused_max_abs": agree, "fused_vs_unfused_loss_abs": loss_agree}
    for k, v in times.items():
        row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for leg in ("forward", "backward", "step"):
        row[f"{leg}_fused_over_unfused"] = row[f"fused_{leg}_ms"]["median"] / row[f"unfused_{leg}_ms"]["median"]
    row["entries_share_of_fused_step"] = (row["entry_forward_ms"]["median"] + row["entry_backward_ms"]["median"]) / row["fused_step_ms"]["median"]
    row["peak_fused_over_unfused"] = peak["fused"] / peak["unfused"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--one", type=int, default=None, help="(internal) run the shape of this batch size in this process and print its row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_loss_bench.json"))
    args = ap.parse_args()
    if args.one is not None:
        shape = next(s for s in SHAPES if s[0] == args.one)
        print("ROW " + json.dumps(one_shape(*shape, args)))
        return 0
    doc = {"hbm_copy_bytes_per_s": HBM_COPY_BPS, "mfma_bf16_flops_per_s": MFMA_BF16_FLOPS, "iters": args.iters, "reps": args.reps, "shapes": []}
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(shape[0]), "--iters", str(args.iters),
               "--warmup", str(args.warmup), "--reps", str(args.reps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        rows = [ln[4:] for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
        if res.returncode != 0 or not rows:
            sys.stderr.write(res.stdout + res.stderr)
            print(f"shape {shape}: exit status {res.returncode}; nothing more is started")
            return 1
        doc["shapes"].append(json.loads(rows[0]))
        print(rows[0])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
