"""The transducer loss with gradients at training-shaped lattices: what rnnt_transducer_loss costs, value only and value plus
gradient, against the bytes it cannot avoid and against torch's own log_softmax forward + backward on the same tensor.

Shapes: B16 x T249 x U28 x V412 and the project's joint shape B64 x T249 x U28 x V412, full-length rows, seeded normal logits.
Per shape and per lattice dtype (`--dtype`, default float32, bfloat16 and float16: the 16-bit ones through rnnt_transducer_loss_elem,
reading and writing 16-bit elements), device-event times over `--iters` calls after `--warmup` calls (median, min, max), legs
alternating per repetition:
  * value:  the loss with grad_dev = NULL (loss_pick, transducer_alpha_beta);
  * grad:   the same with the gradient (+ loss_coef, loss_grad);
  * torch:  (float32) torch.log_softmax(x, -1) and its backward with a ones gradient, alone: the floor of any unfused
            implementation, which still has the recursions and the gradient assembly to add;
  * cast_workaround:  (16-bit) what a caller under autocast had to do while the loss took float32 only: x.float(), the float32
            call with its gradient, grad.to(E).  24 bytes per lattice element against the 16-bit call's 6.
The floor of the fused form is three lattice traversals (read, read, write) = 3 sizeof(E) B T U1 V bytes: 12 per element in
float32, 6 in 16 bits; `floor_fraction` is that many bytes over the measured time, over the HBM rate a float4 copy reaches on this
part (6.29 TB/s).  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/rnnt_loss_bench.py [--out profiles/rnnt_loss_bench.json] [--dtype float32,bfloat16,float16] [--iters 20] [--warmup 5] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BPS = 6.29e12            # measured float4 copy rate of the MI355X (8.0 TB/s spec)
SHAPES = [(16, 249, 28, 412), (64, 249, 28, 412)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="float32,bfloat16,float16", help="comma-separated lattice dtypes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_loss_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib

    assert torch.cuda.is_available(), "rnnt_loss_bench needs a GPU: there is no CPU timing"
    elems = {"float32": (torch.float32, None), "bfloat16": (torch.bfloat16, rlib.LOSS_BF16), "float16": (torch.float16, rlib.LOSS_F16)}
    dtypes = [d for d in args.dtype.split(",") if d]
    assert dtypes and all(d in elems for d in dtypes), f"--dtype: any of {sorted(elems)}"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    doc = {"device": torch.cuda.get_device_name(0), "hbm_copy_bytes_per_s": HBM_COPY_BPS, "iters": args.iters, "reps": args.reps, "shapes": []}
    for B, Tn, U1, V in SHAPES:
        blank, Umax = 5, U1 - 1
        g = np.random.Generator(np.random.Philox(key=[B, 0x1055]))
        x32 = torch.from_numpy(g.standard_normal((B, Tn, U1, V), dtype=np.float32)).to(dev)
        lab = g.integers(0, V - 1, (B, Umax))
        y = np.where(lab >= blank, lab + 1, lab).astype(np.int32)
        Tb, Ub = np.full(B, Tn, np.int32), np.full(B, Umax, np.int32)
        shape = (B, Tn, U1, V)
        nbytes = rlib.transducer_loss_workspace(B, Tn, U1)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nll = torch.empty(B, dtype=torch.float64, device=dev)
        for name in dtypes:
            dtype, elem = elems[name]
            x = x32.to(dtype)
            grad = torch.empty_like(x)

            def loss(x_ptr, grad_ptr, elem):
                rlib.transducer_loss_device(x_ptr, shape, y, Tb, Ub, blank, True, -1.0, nll.data_ptr(), grad_ptr, work.data_ptr(), nbytes, stream, elem=elem)

            def value():
                loss(x.data_ptr(), None, elem)

            def with_grad():
                loss(x.data_ptr(), grad.data_ptr(), elem)

            legs = {"value": value, "grad": with_grad}
            if elem is None:
                ones = torch.ones_like(x)

                def torch_floor():
                    lp = torch.log_softmax(x, -1)
                    torch.ops.aten._log_softmax_backward_data(ones, lp, -1, torch.float32)

                legs["torch_log_softmax_fwd_bwd"] = torch_floor
            else:
                def cast_workaround():
                    xf = x.float()
                    gf = torch.empty_like(xf)
                    loss(xf.data_ptr(), gf.data_ptr(), None)
                    return gf.to(dtype)

                legs["cast_workaround"] = cast_workaround
            times = {k: [] for k in legs}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            with_grad()
            torch.cuda.synchronize()
            first = nll.cpu().numpy().copy()
            for _ in range(args.reps):
                for k, fn in legs.items():
                    for _ in range(args.iters):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        times[k].append(e0.elapsed_time(e1))
            with_grad()
            torch.cuda.synchronize()
            assert np.array_equal(first.view(np.uint64), nll.cpu().numpy().view(np.uint64)), "nll changed between calls"
            lattice = x.element_size() * B * Tn * U1 * V
            floor_bytes = 3 * lattice
            row = {"B": B, "T": Tn, "U1": U1, "V": V, "dtype": name, "lattice_bytes": lattice, "floor_bytes": floor_bytes,
                   "floor_ms_at_hbm_copy_rate": 1e3 * floor_bytes / HBM_COPY_BPS, "nll_mean": float(first.mean())}
            for k, v in times.items():
                row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            row["floor_fraction"] = row["floor_ms_at_hbm_copy_rate"] / row["grad_ms"]["median"]
            row["value_fraction_of_one_read"] = (1e3 * lattice / HBM_COPY_BPS) / row["value_ms"]["median"]
            if elem is None:
                row["grad_over_torch"] = row["grad_ms"]["median"] / row["torch_log_softmax_fwd_bwd_ms"]["median"]
            else:
                row["grad_over_cast_workaround"] = row["grad_ms"]["median"] / row["cast_workaround_ms"]["median"]
            doc["shapes"].append(row)
            print(json.dumps(row))
            del x, grad, legs
            if elem is None:
                del ones
            torch.cuda.empty_cache()
        del x32, work
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
