"""The CTC loss with gradients at training shapes: what rnnt_ctc_loss costs, value only and value plus gradient, against the bytes the
algorithm cannot avoid and against torch's own chain on the device, log_softmax -> F.ctc_loss -> backward.

Shapes: B 16 / 64 x T 249 x L 28, V 412 (this tokenizer) and V 4336 (the reference's default vocab_size), full-length rows, seeded
normal logits in a contiguous [B, T, V] tensor (what ctc_lo writes), addressed through its strides: no transposed copy on our side.
Per shape and dtype (`--dtype`, default float32 and bfloat16; the 16-bit one through rnnt_ctc_loss_elem), device-event times around
whole calls, host part included, over `--iters` calls after `--warmup` calls (median, min, max), legs alternating per repetition:
  * value:     rnnt_ctc_loss with grad_dev = NULL into a preallocated workspace (ctc_loss_pick, the forward ctc_alpha_beta);
  * grad:      the same with the gradient (both recursions, + ctc_loss_occ, ctc_loss_grad);
  * autograd:  functional.ctc_loss(x.transpose(0, 1), fused_log_softmax=True, "mean", zero_infinity).backward(): the same launches
               plus torch's allocations and the per-row scaling of the saved gradient;
  * torch:     torch.log_softmax(x, -1, float32).transpose(0, 1) -> F.ctc_loss("mean", zero_infinity) -> backward() to x: what a
               trainer runs without this project.  It does not change with this project, so it is the baseline.
The floor is the algorithm's bytes, one read and one write of [B, T, V] = 2 sizeof(E) B T V, at the HBM rate a float4 copy reaches on
this part (6.29 TB/s).  Peak memory: torch.cuda.max_memory_allocated over one autograd / torch call, above what was allocated before
it (x and the targets).  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/ctc_loss_bench.py [--out profiles/ctc_loss_bench.json] [--dtype float32,bfloat16] [--iters 20] [--warmup 5] [--reps 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BPS = 6.29e12            # measured float4 copy rate of the MI355X (8.0 TB/s spec)
SHAPES = [(16, 249, 28, 412), (64, 249, 28, 412), (16, 249, 28, 4336), (64, 249, 28, 4336)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="float32,bfloat16", help="comma-separated input dtypes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    import ctc_vr_amd.lib as rlib
    from ctc_vr_amd.functional import ctc_loss

    assert torch.cuda.is_available(), "ctc_loss_bench needs a GPU: there is no CPU timing"
    elems = {"float32": (torch.float32, None), "bfloat16": (torch.bfloat16, rlib.LOSS_BF16), "float16": (torch.float16, rlib.LOSS_F16)}
    dtypes = [d for d in args.dtype.split(",") if d]
    assert dtypes and all(d in elems for d in dtypes), f"--dtype: any of {sorted(elems)}"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    doc = {"device": torch.cuda.get_device_name(0), "hbm_copy_bytes_per_s": HBM_COPY_BPS, "iters": args.iters, "reps": args.reps, "shapes": []}
    for B, Tn, Lmax, V in SHAPES:
        blank = 0
        g = np.random.Generator(np.random.Philox(key=[B, V]))
        x32 = torch.from_numpy(g.standard_normal((B, Tn, V), dtype=np.float32)).to(dev)
        y = g.integers(1, V, (B, Lmax)).astype(np.int32)
        Tb, Lb = np.full(B, Tn, np.int32), np.full(B, Lmax, np.int32)
        y_d, Tb_d, Lb_d = torch.from_numpy(y).to(dev).long(), torch.from_numpy(Tb).to(dev).long(), torch.from_numpy(Lb).to(dev).long()
        nbytes = rlib.ctc_loss_workspace(B, Tn, Lmax)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        nll = torch.empty(B, dtype=torch.float64, device=dev)
        for name in dtypes:
            dtype, elem = elems[name]
            x = x32.to(dtype)
            grad = torch.empty_like(x)

            def loss(grad_ptr):
                rlib.ctc_loss_device(x.data_ptr(), (B, Tn, V), (Tn * V, V), y, Tb, Lb, blank, True, nll.data_ptr(), grad_ptr, work.data_ptr(), nbytes,
                                     stream, elem=elem)

            def value():
                loss(None)

            def with_grad():
                loss(grad.data_ptr())

            def autograd():
                xr = x.detach().requires_grad_(True)
                out = ctc_loss(xr.transpose(0, 1), y, Tb, Lb, blank=blank, reduction="mean", zero_infinity=True, fused_log_softmax=True)
                out.backward()
                return out.detach(), xr.grad

            def torch_chain():
                xr = x.detach().requires_grad_(True)
                lp = torch.log_softmax(xr, -1, dtype=torch.float32).transpose(0, 1)
                out = F.ctc_loss(lp, y_d, Tb_d, Lb_d, blank=blank, reduction="mean", zero_infinity=True)
                out.backward()
                return out.detach(), xr.grad

            legs = {"value": value, "grad": with_grad, "autograd": autograd, "torch": torch_chain}
            times = {k: [] for k in legs}
            for fn in legs.values():
                for _ in range(args.warmup):
                    fn()
            with_grad()
            torch.cuda.synchronize()
            first = nll.cpu().numpy().copy()
            (la, ga), (lt, gt) = autograd(), torch_chain()
            agree = {"loss_ours": float(la), "loss_torch": float(lt), "grad_max_abs_difference": float((ga.float() - gt.float()).abs().max())}
            del ga, gt
            peak = {}
            for k in ("autograd", "torch"):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                legs[k]()
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - before
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
            tensor_bytes = x.element_size() * B * Tn * V
            floor_bytes = 2 * tensor_bytes
            row = {"B": B, "T": Tn, "L": Lmax, "V": V, "dtype": name, "tensor_bytes": tensor_bytes, "floor_bytes": floor_bytes,
                   "floor_ms_at_hbm_copy_rate": 1e3 * floor_bytes / HBM_COPY_BPS, "nll_mean": float(first.mean()), "workspace_bytes": nbytes,
                   "peak_bytes_above_input": peak, **agree}
            for k, v in times.items():
                row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            row["floor_fraction"] = row["floor_ms_at_hbm_copy_rate"] / row["grad_ms"]["median"]
            row["grad_over_torch"] = row["grad_ms"]["median"] / row["torch_ms"]["median"]
            row["autograd_over_torch"] = row["autograd_ms"]["median"] / row["torch_ms"]["median"]
            doc["shapes"].append(row)
            print(json.dumps(row))
            del x, grad, legs
            torch.cuda.empty_cache()
        del x32, work
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
