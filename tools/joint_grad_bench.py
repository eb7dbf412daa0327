"""The joint lattice with gradients at training shapes: what transducer_joint costs forward, backward and in the chain
transducer_joint -> rnnt_loss -> backward, against the bytes and FLOPs the algorithm needs and against the eager restatement
tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ W.T + b under torch autograd, on the same device in the same process.

Shapes: B16 x T249 x U28 x V412 and the project's joint shape B64 x T249 x U28 x V412, full-length rows, seeded inputs.  Per shape,
whole calls by device events over `--iters` calls after `--warmup` calls, `--reps` repetitions with the legs alternating (60 samples
per leg by default; median, min, max):
  * forward:   logits from e, p, W, b (workspace and output allocation included: whole calls);
  * backward:  torch.autograd.grad of the logits for a given lattice gradient (ours: rnnt_joint_lattice_backward; eager: torch's
               two GEMMs and the elementwise passes over its saved [B, T, U1, 256] tensors);
  * chain:     forward, rnnt_loss(reduction="mean") and the gradients of the four leaves.
What the algorithm needs, from the shapes: the forward writes the lattice once (4 M V bytes) and multiplies 2 M V 256 FLOPs; the backward
reads the lattice gradient once (4 M V bytes; this implementation reads it twice, once per contraction) and multiplies 4 M V 256 FLOPs;
e, p, W and the four results are smaller by two orders.  `floor_ms` is those bytes at the HBM rate a float4 copy reaches on this
part (6.29 TB/s); the bf16x3 form spends three MFMA products per useful one.  Peak memory: torch.cuda.max_memory_allocated over one
chain, above what was allocated before it.  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/joint_grad_bench.py [--out profiles/joint_grad_bench.json] [--iters 20] [--warmup 3] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BPS = 6.29e12            # measured float4 copy rate of the MI355X (8.0 TB/s spec)
SHAPES = [(16, 249, 28, 412), (64, 249, 28, 412)]
D = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_grad_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from ctc_vr_amd.functional import rnnt_loss, transducer_joint

    assert torch.cuda.is_available(), "joint_grad_bench needs a GPU: there is no CPU timing"
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0), "hbm_copy_bytes_per_s": HBM_COPY_BPS, "iters": args.iters, "reps": args.reps, "shapes": []}

    def eager_joint(e, p, w, b):
        return torch.tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ w.T + b

    for B, Tn, U1, V in SHAPES:
        r = np.random.Generator(np.random.Philox(key=[B, 0x101]))
        f = np.float32
        leaves = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (
            r.standard_normal((B, Tn, D)).astype(f), r.standard_normal((B, U1, D)).astype(f), (r.standard_normal((V, D)) / 16.0).astype(f),
            (0.3 * r.standard_normal(V)).astype(f))]
        g = torch.from_numpy((0.05 / B * r.standard_normal((B, Tn, U1, V))).astype(f)).to(dev)
        blank = 5
        lab = r.integers(0, V - 1, (B, U1 - 1))
        y = torch.from_numpy(np.where(lab >= blank, lab + 1, lab).astype(np.int32)).to(dev)
        ll, tl = torch.full((B,), Tn, dtype=torch.int32, device=dev), torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
        joints = {"ours": lambda: transducer_joint(*leaves, ll, tl), "eager": lambda: eager_joint(*leaves)}

        def chain(joint):
            loss = rnnt_loss(joint(), y, ll, tl, blank=blank, reduction="mean")
            return torch.autograd.grad(loss, leaves)

        legs, held = {}, {}
        for k, joint in joints.items():
            held[k] = joint()                                      # one graph per side, kept for the backward leg
            legs[k + "_forward"] = joint
            legs[k + "_backward"] = (lambda k=k: torch.autograd.grad(held[k], leaves, g, retain_graph=True))
            legs[k + "_chain"] = (lambda joint=joint: chain(joint))
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        first = [t.clone() for t in legs["ours_backward"]()]
        agree = {n: float((a - b).abs().max()) for n, a, b in zip(("de", "dp", "dW", "db"), first, legs["eager_backward"]())}
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
        assert all(torch.equal(a, b) for a, b in zip(first, legs["ours_backward"]())), "the backward changed between calls"
        held.clear()
        peak = {}
        for k, joint in joints.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = chain(joint)
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated() - base
            del out
        M = B * Tn * U1
        lattice = 4 * M * V
        row = {"B": B, "T": Tn, "U1": U1, "V": V, "cells": M, "lattice_bytes": lattice, "forward_flops": 2 * M * V * D, "backward_flops": 4 * M * V * D,
               "forward_floor_ms": 1e3 * lattice / HBM_COPY_BPS, "backward_floor_ms": 1e3 * lattice / HBM_COPY_BPS,
               "peak_chain_bytes": peak, "ours_vs_eager_max_abs": agree}
        for k, v in times.items():
            row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        for leg in ("forward", "backward", "chain"):
            row[f"{leg}_ours_over_eager"] = row[f"ours_{leg}_ms"]["median"] / row[f"eager_{leg}_ms"]["median"]
        row["forward_floor_fraction"] = row["forward_floor_ms"] / row["ours_forward_ms"]["median"]
        row["backward_floor_fraction"] = row["backward_floor_ms"] / row["ours_backward_ms"]["median"]
        row["backward_useful_tflops"] = row["backward_flops"] / (1e9 * row["ours_backward_ms"]["median"])
        doc["shapes"].append(row)
        print(json.dumps(row))
        del leaves, g, legs, joints, first
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
