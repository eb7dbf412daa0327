"""Two-pass decoding at a serving shape (10 s utterances: T' = 249 encoder frames, N = 10 hypotheses of 20 to 28 labels, bf16x3 by
default), B = 1 and B = 32 in one process: what the n-best transducer likelihood costs against the only way to get the same numbers
without it.

  * nbest:    rnnt_transducer_nll_nbest -- joint.enc_ffn over the B*T frames once, the hypotheses side by side along U;
  * repeated: rnnt_transducer_nll over B*N rows with every utterance's frames repeated N times (the context is sized so that this
              fits its scratch);
both timed with the host clock around the synchronising call, alternating after a warm-up, median of --iters calls per repetition.
`repeated` is also timed against itself (a second series in every repetition): the run-to-run spread the comparison is read
against.  The check: nbest is no slower than repeated by more than that spread at B = 32.  The two nll tables are compared beside
the bound (T_b + U_b) * delta, delta = max |difference of the two picked lattices| over the valid cells.  The per-phase split of
nbest comes from the launch-site tags (rnnt_profile_begin / _end): 20 + 21 the predictor steps, 13 + 22 the two projections, 40 the
pick, 41 the recursion.  Last, StreamPool.rescore of 64 CTC prefix slots (10 s each) against the 64 ctc_hyps(final=True) reads it
contains.  Writes one JSON document.

usage: python tools/rescore_bench.py [--out profiles/rescore_bench.json] [--numerics bf16x3] [--reps 3] [--iters 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = {"predictor_lstm": 20, "predictor_proj": 21, "enc_ffn": 13, "pred_ffn": 22, "pick": 40, "alpha": 41}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=249, help="encoder frames T' (10 s)")
    ap.add_argument("--nbest", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5, help="timed calls per repetition and leg (median reported)")
    ap.add_argument("--pool-slots", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine
    from ctc_vr_amd.online_rnnt_model import StreamPool

    assert torch.cuda.is_available(), "rescore_bench needs a GPU: there is no CPU timing"
    Tn, N, Umax, V, blank = args.frames, args.nbest, 28, T.VOCAB, T.BLANK
    U1 = Umax + 1
    Bmax = max(args.batches)
    need = Bmax * N * Tn * 256 + Bmax * N * U1 * 256             # the repeated form's scratch: e and p of B*N rows
    cache = max(64, -(-need // (12 * 4 * 128)))
    eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=cache, max_enc_frames=16, max_tokens=16, vocab_size=V, blank_id=blank)
    sd = T.make_state_dict(0)
    eng.load_state_dict(sd, numerics=args.numerics)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    med = lambda v: float(np.median(v))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    res = {"workload": f"T'{Tn} x N{N} x 20..{Umax} labels x V{V}, {args.numerics}", "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in args.batches:
        g = np.random.Generator(np.random.Philox(key=[2025, B]))
        enc = torch.from_numpy(g.standard_normal((B, Tn, 256), dtype=np.float32)).to(dev)
        hl = g.integers(20, Umax + 1, (B, N)).astype(np.int32)
        y = g.integers(0, V - 1, (B, N, Umax))
        ht = np.where(y >= blank, y + 1, y).astype(np.int32)
        el, nh = np.full(B, Tn, np.int32), np.full(B, N, np.int32)
        rep = enc[:, None].expand(B, N, Tn, 256).reshape(B * N, Tn, 256).contiguous()
        rel, rtg, rtl = np.repeat(el, N), ht.reshape(B * N, Umax), hl.reshape(B * N)

        def nbest(pick=None):
            return eng.transducer_nll_nbest(enc.data_ptr(), el, nh, hl, ht, B, Tn, pick, s)

        def repeated(pick=None):
            return eng.transducer_nll(rep.data_ptr(), rel, rtg, rtl, B * N, Tn, pick, s).reshape(B, N)

        # warm-up, and the two picked lattices once for the bound
        pa = torch.empty(B, Tn, N, U1, 2, device=dev)
        pb = torch.empty(B, N, Tn, U1, 2, device=dev)
        na, nb = nbest(pa.data_ptr()).copy(), repeated(pb.data_ptr()).copy()
        nbest(), repeated()
        torch.cuda.synchronize()
        d = (pa.double() - pb.permute(0, 2, 1, 3, 4).double()).abs().cpu().numpy()
        u = np.arange(U1)[None, None, None, :]
        ub = hl[:, None, :, None]
        delta = max(float(d[..., 0][np.broadcast_to(u <= ub, d.shape[:4])].max()), float(d[..., 1][np.broadcast_to(u < ub, d.shape[:4])].max()))
        diff, bound = np.abs(na - nb), (Tn + hl) * delta
        del pa, pb
        reps, identical = [], True
        for _ in range(args.reps):
            ta, tb, tb2 = [], [], []
            for _ in range(args.iters):
                ms, nll = timed(nbest)
                ta.append(ms)
                identical = identical and np.array_equal(nll.view(np.uint64), na.view(np.uint64))
                tb.append(timed(repeated)[0])
                tb2.append(timed(repeated)[0])
            reps.append({"nbest_ms": round(med(ta), 4), "repeated_ms": round(med(tb), 4), "repeated_again_ms": round(med(tb2), 4)})
        phases = {}
        for name, tag in PHASES.items():
            eng.profile_begin(tag)
            nbest()
            ms, n = eng.profile_end()
            phases[name] = {"us": round(ms * 1e3, 2), "launches": int(n)}
        rb = [r["repeated_ms"] for r in reps] + [r["repeated_again_ms"] for r in reps]
        spread = max(rb) - min(rb)
        a_ms, b_ms = med([r["nbest_ms"] for r in reps]), med(rb)
        res["batches"][str(B)] = {
            "reps": reps, "nbest_ms": a_ms, "repeated_ms": b_ms, "repeated_spread_ms": round(spread, 4), "nbest_over_repeated": round(a_ms / b_ms, 4),
            "nbest_no_slower_than_repeated": bool(a_ms <= b_ms + spread), "phases_us": phases,
            "phase_sum_us": round(sum(p["us"] for p in phases.values()), 2),
            "predictor_share_of_phases": round((phases["predictor_lstm"]["us"] + phases["predictor_proj"]["us"]) / sum(p["us"] for p in phases.values()), 4),
            "max_abs_nll_diff": float(diff.max()), "bound_at_that_entry": float(bound.reshape(-1)[diff.argmax()]), "pick_delta": delta,
            "nll_within_bound": bool((diff <= bound).all()), "nll_identical_across_calls": bool(identical),
            "scratch_rows": {"nbest": B * Tn + B * N * U1, "repeated": B * N * (Tn + U1)}, "nll_mean": float(na.mean())}
        print(f"B={B}: nbest {a_ms:.3f} ms, repeated {b_ms:.3f} ms (spread {spread:.3f} ms); max |nll diff| {diff.max():.3e} beside bound "
              f"{bound.reshape(-1)[diff.argmax()]:.3e}", file=sys.stderr)
        del enc, rep
    eng.close()

    # ---- the pool: rescore of --pool-slots CTC prefix slots against the final reads it contains ---------------------------------------
    # The seeded CTC head emits a label on most frames; a blank bias brings its hypotheses to the 20-odd labels of the first part.
    # max_cache_frames sizes the context scratch the rescoring lattice lives in (and the kept history: that many KB per slot).
    S, chunk, pool_cache = args.pool_slots, 64, 4096
    n_fb = 4 * Tn + 3                                             # 10 s of fbank frames, fed in chunks of 64
    sd = dict(sd)
    sd["ctc_head.ctc_lo.bias"] = sd["ctc_head.ctc_lo.bias"].copy()
    sd["ctc_head.ctc_lo.bias"][blank] += np.float32(4.5)
    pool = StreamPool(sd, S, vocab_size=V, blank_id=blank, max_chunk_frames=chunk, max_cache_frames=pool_cache, numerics=args.numerics)
    x = torch.from_numpy(T.synth_fbank(S, n_fb, seed=7)).to(dev)
    slots = [pool.open(ctc_prefix_beam=N, keep_frames=True) for _ in range(S)]
    for a in range(0, n_fb, chunk):
        for slot in slots:
            pool.feed(slot, x[slot, a:a + chunk].contiguous())
        pool.step()
    frames = [int(pool.frames(slot).size(0)) for slot in slots]
    pool.rescore(slots, 0.3, 0.7)                                 # warm-up (grows the staging buffer)
    t_res, t_reads = [], []
    for _ in range(args.iters):
        t_res.append(timed(lambda: pool.rescore(slots, 0.3, 0.7))[0])
        t_reads.append(timed(lambda: [pool.ctc_hyps(slot, final=True) for slot in slots])[0])
    out = pool.rescore(slots, 0.3, 0.7)
    res["pool"] = {"slots": S, "frames_per_slot": [min(frames), max(frames)], "beam": N, "rescore_ms": round(med(t_res), 4),
                   "final_reads_ms": round(med(t_reads), 4), "rescore_minus_reads_ms": round(med(t_res) - med(t_reads), 4),
                   "hyps_per_slot": [min(len(r[1]) for r in out.values()), max(len(r[1]) for r in out.values())],
                   "labels_per_hyp": [min(len(h[0]) for r in out.values() for h in r[1]), max(len(h[0]) for r in out.values() for h in r[1])],
                   "kept_history_bytes_per_slot": pool_cache * 256 * 4}
    pool.engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
