"""An encoder layer's attention core with gradients: what rnnt_rel_attention_forward and rnnt_rel_attention_backward cost against the
eager restatement of the reference's formula on the device, in time and in peak memory, and against the op's own bytes and FLOPs.

Shapes: B 16 and 64 x T 249 (the trainer's), with chunk 16 (unbounded left context) and with full context; lengths run from T down
to about T / 2.  Seeded N(0, 1) inputs.  Device-event times around whole calls, host part included, over `--iters` calls after
`--warmup` calls (median, min, max), legs alternating per repetition:
  * forward:        rnnt_rel_attention_forward saving the log-sum-exp, into preallocated buffers (ONE launch);
  * backward:       rnnt_rel_attention_backward (delta, the key-owned pass, the query-owned pass, two reduces);
  * step:           both, through functional.rel_attention(...).backward(), torch's allocator and autograd included;
  * eager_forward / eager_step: matrix_ac, matrix_bd, scores, masked_fill, float32 softmax, masked_fill, attn @ v as the reference
                    writes them (wenet/transformer/attention.py:364-420, forward_attention) with a dense [B, T, T] mask.
Peak memory: torch.cuda.max_memory_allocated over one step above what is allocated before it, for either path.
Own bytes and FLOPs: the tensors each call must read and write once (q, k, v, p, out, lse forward; those, dout and the four big
gradients backward), and 2 x 64 x (visible (i, j) pairs per head) x the contractions per pair (3 forward: two score terms and a v;
6 + 5 in the two backward passes), beside the rates the medians imply.  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/attention_grad_bench.py [--out profiles/attention_grad_bench.json] [--iters 20] [--warmup 5] [--reps 3]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 249, 16), (16, 249, 0), (64, 249, 16), (64, 249, 0)]              # (B, T, chunk_size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_grad_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.functional import rel_attention

    assert torch.cuda.is_available(), "attention_grad_bench needs a GPU: there is no CPU timing"
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "shapes": []}
    for B, Tn, chunk in SHAPES:
        g = np.random.Generator(np.random.Philox(key=[1000 * B + Tn, chunk]))
        rnd = lambda *s, scale=1.0: torch.from_numpy((scale * g.standard_normal(s)).astype(np.float32)).to(dev)
        q, k, v, p, dout = rnd(B, Tn, 256), rnd(B, Tn, 256), rnd(B, Tn, 256), rnd(Tn, 256), rnd(B, Tn, 256, scale=0.05)
        u, vb = rnd(4, 64, scale=0.3), rnd(4, 64, scale=0.3)
        lens = np.array([Tn - (b * (Tn // 2)) // max(B - 1, 1) for b in range(B)], np.int32)
        vis_np = T.chunk_visible(Tn, lens, chunk, -1)
        pairs = int(vis_np.sum())                                  # visible (i, j) per head
        mask = torch.from_numpy(vis_np).to(dev)                    # [B, T, T]: the dense mask the reference builds per step
        wbytes, sbytes = rlib.rel_attention_workspace(B, Tn)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        state = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out, dq, dk, dv, dp, du, dvb = new(B, Tn, 256), new(B, Tn, 256), new(B, Tn, 256), new(B, Tn, 256), new(Tn, 256), new(4, 64), new(4, 64)
        head = [t.data_ptr() for t in (q, k, v, p, u, vb)]

        def forward():
            rlib.rel_attention_forward_device(*head, lens, (B, Tn), chunk, -1, out.data_ptr(), state.data_ptr(), sbytes, work.data_ptr(), wbytes, stream)

        def backward():
            rlib.rel_attention_backward_device(*head, out.data_ptr(), state.data_ptr(), sbytes, dout.data_ptr(), lens, (B, Tn), chunk, -1, dq.data_ptr(),
                                               dk.data_ptr(), dv.data_ptr(), dp.data_ptr(), du.data_ptr(), dvb.data_ptr(), work.data_ptr(), wbytes, stream)

        def leaves():
            return [t.detach().requires_grad_(True) for t in (q, k, v, p, u, vb)]

        def step():
            ls = leaves()
            rel_attention(*ls, lens, chunk, -1).backward(dout)
            return ls

        def eager(ls):
            qq, kk, vv, pp, uu, vvb = ls
            qh = qq.view(B, Tn, 4, 64)
            kh, vh = kk.view(B, Tn, 4, 64).transpose(1, 2), vv.view(B, Tn, 4, 64).transpose(1, 2)
            ph = pp.view(1, Tn, 4, 64).transpose(1, 2)
            matrix_bd = torch.matmul((qh + vvb).transpose(1, 2), ph.transpose(-2, -1))
            matrix_ac = torch.matmul((qh + uu).transpose(1, 2), kh.transpose(-2, -1))
            scores = (matrix_ac + matrix_bd) / math.sqrt(64)
            hidden = mask.unsqueeze(1).eq(0)
            scores = scores.masked_fill(hidden, -float("inf"))
            attn = torch.softmax(scores.float(), dim=-1).type_as(vh).masked_fill(hidden, 0.0)
            return torch.matmul(attn, vh).transpose(1, 2).contiguous().view(B, Tn, 256)

        def eager_forward():
            with torch.no_grad():
                return eager((q, k, v, p, u, vb))

        def eager_step():
            ls = leaves()
            eager(ls).backward(dout)
            return ls

        legs = {"forward": forward, "backward": backward, "step": step, "eager_forward": eager_forward, "eager_step": eager_step}
        forward()
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the two paths compute the same thing (rows without a visible key do not occur without a bounded left context)
        a, b = step(), eager_step()
        torch.cuda.synchronize()
        agree = {"out_vs_eager": float((out - eager_forward()).abs().max()),
                 **{f"d{n}_vs_eager": float((x.grad - y.grad).abs().max()) for n, x, y in zip(("q", "k", "v", "p", "u", "vb"), a, b)}}
        del a, b
        peak = {}
        for name, fn in (("step", step), ("eager_step", eager_step)):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ls = fn()
            torch.cuda.synchronize()
            peak[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
            del ls
        times = {n: [] for n in legs}
        for _ in range(args.reps):
            for n, fn in legs.items():
                if n == "backward":
                    forward()
                for _ in range(args.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[n].append(e0.elapsed_time(e1))
        big = 4 * B * Tn * 256
        own = {"forward_bytes": 4 * big + 4 * Tn * 256 + sbytes, "backward_bytes": 8 * big + 2 * 4 * Tn * 256 + sbytes,
               "forward_flops": 2 * 64 * 4 * pairs * 3, "backward_flops": 2 * 64 * 4 * pairs * 11}
        row = {"B": B, "T": Tn, "chunk_size": chunk, "visible_pairs_per_head": pairs, "dense_pairs_per_head": B * Tn * Tn, "work_bytes": wbytes,
               "state_bytes": sbytes, "tt_tensor_bytes": 4 * B * 4 * Tn * Tn, **agree, **peak, **own}
        for n, t in times.items():
            row[n + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        for n in ("forward", "backward"):
            s = row[n + "_ms"]["median"] * 1e-3
            row[n + "_implied_bytes_per_s"] = own[n + "_bytes"] / s
            row[n + "_implied_flops_per_s"] = own[n + "_flops"] / s
        row["step_over_eager_step"] = row["step_ms"]["median"] / row["eager_step_ms"]["median"]
        row["forward_over_eager_forward"] = row["forward_ms"]["median"] / row["eager_forward_ms"]["median"]
        doc["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
