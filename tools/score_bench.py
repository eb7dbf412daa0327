"""Teacher-forced scoring at the training-shaped lattice (B64 x T249 x U28 x V412, bf16x3 by default): what the fused pick
kernel costs against the only way to get the same two columns without it.

Three alternating repetitions, each in the same process on the same seeded inputs, device-synchronised after warm-up:
  * score:   rnnt_transducer_nll (predictor steps + two small GEMMs + joint_lattice_rows<.., PICK> + transducer_alpha + copy),
             host clock around the synchronising call;
  * lattice: rnnt_joint(mode=1) into a [B, T, U, V] tensor followed by a torch gather of the (blank, target) columns;
  * kernels: HIP-event times (rnnt_profile_begin / _end) of the pick kernel (tag 40), of transducer_alpha (tag 41) and of the
             log-softmax lattice kernel inside rnnt_joint (tag 23), each in a call of its own.
The check: the pick kernel is no slower than the log-softmax lattice kernel by more than the spread (max - min) of the lattice
kernel's three repetitions.  Both nll vectors must agree bit for bit across repetitions.  Writes one JSON document.

usage: python tools/score_bench.py [--out profiles/score_bench.json] [--numerics bf16x3] [--reps 3] [--iters 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=249, help="encoder frames T")
    ap.add_argument("--u1", type=int, default=28, help="lattice rows per frame, Umax + 1")
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5, help="timed calls per repetition and leg (median reported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "score_bench needs a GPU: there is no CPU timing"
    B, Tn, U1 = args.batch, args.frames, args.u1
    Umax, V, blank = U1 - 1, T.VOCAB, T.BLANK
    need = B * Tn * 256 + B * U1 * 256                            # rnnt_joint's scratch: e and p
    cache = max(64, -(-need // (12 * 4 * 128)))
    eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=cache, max_enc_frames=16, max_tokens=16, vocab_size=V, blank_id=blank)
    eng.load_state_dict(T.make_state_dict(0), numerics=args.numerics)
    dev = torch.device("cuda", 0)
    g = np.random.Generator(np.random.Philox(key=[2024, 7]))
    enc = torch.from_numpy(g.standard_normal((B, Tn, 256), dtype=np.float32)).to(dev)
    y = g.integers(0, V - 1, (B, Umax)).astype(np.int32)
    tg = np.where(y >= blank, y + 1, y).astype(np.int32)
    el, tl = np.full(B, Tn, np.int32), np.full(B, Umax, np.int32)
    s = torch.cuda.current_stream().cuda_stream

    # predictor outputs for the lattice leg (the step API a caller has today), outside the timed window
    h = torch.zeros(B, 256, device=dev)
    c = torch.zeros(B, 256, device=dev)
    pred = torch.empty(B, U1, 256, device=dev)
    for u in range(U1):
        tok = torch.from_numpy(np.ascontiguousarray(tg[:, u - 1]) if u else np.full(B, blank, np.int32)).to(dev)
        out, h2, c2 = torch.empty(B, 256, device=dev), torch.empty(B, 256, device=dev), torch.empty(B, 256, device=dev)
        eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), B, out.data_ptr(), h2.data_ptr(), c2.data_ptr(), s)
        pred[:, u] = out
        h, c = h2, c2
    lat = torch.empty(B, Tn, U1, V, device=dev)
    col = torch.from_numpy(np.concatenate([tg, np.full((B, 1), blank, np.int32)], 1).astype(np.int64)).to(dev)
    idx = torch.stack([torch.full_like(col, blank), col], -1)[:, None].expand(B, Tn, U1, 2).contiguous()
    pick = torch.empty(B, Tn, U1, 2, device=dev)

    def score():
        return eng.transducer_nll(enc.data_ptr(), el, tg, tl, B, Tn, pick.data_ptr(), s)

    def lattice():
        eng.joint(enc.data_ptr(), pred.data_ptr(), B, Tn, U1, 1, lat.data_ptr(), s)
        return lat.gather(3, idx)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def kernel_us(tag, fn):
        eng.profile_begin(tag)
        fn()
        torch.cuda.synchronize()
        ms, n = eng.profile_end()
        assert n == 1, (tag, n)
        return ms * 1e3

    for _ in range(2):
        nll0 = score().copy()
        got0 = lattice()
    torch.cuda.synchronize()
    valid = torch.ones(B, Tn, U1, 2, dtype=torch.bool, device=dev)
    valid[:, :, Umax, 1] = False                                  # the label slot at u = U_b is not a cell
    same_cols = bool(torch.equal(pick[valid], got0[valid]))
    med = lambda v: float(np.median(v))
    reps, identical = [], True
    for _ in range(args.reps):
        ts, tl_ = [], []
        for _ in range(args.iters):
            ms, nll = timed(score)
            ts.append(ms)
            identical = identical and np.array_equal(nll.view(np.uint64), nll0.view(np.uint64))
            tl_.append(timed(lattice)[0])
        reps.append({"score_call_ms": round(med(ts), 4), "lattice_gather_ms": round(med(tl_), 4),
                     "pick_kernel_us": round(kernel_us(40, score), 2), "alpha_kernel_us": round(kernel_us(41, score), 2),
                     "lattice_kernel_us": round(kernel_us(23, lattice), 2)})
    pk = [r["pick_kernel_us"] for r in reps]
    lk = [r["lattice_kernel_us"] for r in reps]
    spread = max(lk) - min(lk)
    res = {"workload": f"B{B} x T{Tn} x U{U1} x V{V}, {args.numerics}, full lengths", "reps": reps,
           "score_call_ms": med([r["score_call_ms"] for r in reps]), "lattice_gather_ms": med([r["lattice_gather_ms"] for r in reps]),
           "pick_kernel_us": med(pk), "alpha_kernel_us": med([r["alpha_kernel_us"] for r in reps]), "lattice_kernel_us": med(lk),
           "lattice_kernel_spread_us": round(spread, 2), "pick_over_lattice": round(med(pk) / med(lk), 4),
           "pick_no_slower_than_lattice": bool(med(pk) <= med(lk) + spread),
           "bytes": {"pick_out": B * Tn * U1 * 2 * 4, "lattice_out": B * Tn * U1 * V * 4},
           "nll_identical_across_calls": bool(identical), "pick_equals_lattice_columns": same_cols,
           "nll_mean": float(nll0.mean()), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
