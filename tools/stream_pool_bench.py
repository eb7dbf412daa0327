"""Stream-pool measurements on one GPU (bench.py's seeded weights; bf16x3 unless told otherwise), every comparison inside ONE process,
three alternating repetitions.  Prints one JSON line; --out writes it to a file as well (profiles/stream_pool_*.json).

  in_phase   64 slots, chunk 16, every slot active every step: rnnt_pool_chunk (encode + greedy decode + consume in one call)
             against rnnt_encoder_chunk + rnnt_greedy_decode + rnnt_frames_consume of a lock-step context.  With --parent-lib the
             lock-step side runs on THAT library (the parent commit's, built beside this one); without it on this library.
  sparse     4 of the 64 slots active every step, the rest idle mid-utterance: ms per step beside the in-phase figure.
  staggered  64 slots, utterances of 2-12 s with uniformly random phase arriving continuously: ms per step and the per-chunk real-time
             factor in the reference's definition (online_rnnt_delay.evaluate_rtf_pool); and the same load served the only way
             possible without the pool -- one context per caller, each at B = 1 -- for --callers callers.

usage: python tools/stream_pool_bench.py [--parent-lib PATH] [--steps 60] [--reps 3] [--callers 8] [--numerics bf16x3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="librnnt_hip.so of the parent commit for the lock-step side of in_phase")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--steps", type=int, default=60, help="timed steps per repetition (after the warm-up steps)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--callers", type=int, default=8, help="contexts of the one-context-per-caller leg")
    ap.add_argument("--stagger-steps", type=int, default=150)
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--blank-bias", type=float, default=12.0, help="as bench.py")
    ap.add_argument("--skip", default="", help="comma list of legs to skip: in_phase,sparse,staggered")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_delay import _stats, evaluate_rtf_pool
    from ctc_vr_amd.online_rnnt_model import StreamingBatch, StreamPool

    B, cf = args.slots, args.chunk
    skip = set(args.skip.split(",")) if args.skip else set()
    sd = T.make_state_dict(0, blank_bias=args.blank_bias)
    s = torch.cuda.current_stream().cuda_stream
    n_chunks = args.warmup + args.steps
    x = torch.from_numpy(T.synth_fbank(B, n_chunks * cf, seed=5)).cuda()
    cache = 4 * n_chunks + 64
    res = {"tool": "stream_pool_bench", "numerics": args.numerics, "slots": B, "chunk": cf, "steps": args.steps, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}

    def lock_step_batch(lib_path):
        """a lock-step context of B streams; lib_path: another build of the library (bound to the symbols it exports)"""
        if lib_path is None:
            return StreamingBatch(sd, B, max_chunk_frames=64, max_cache_frames=cache, numerics=args.numerics)
        rlib.load()                                         # this tree's library first (and the HIP runtime torch uses)
        other = ctypes.CDLL(os.path.abspath(lib_path))
        for name, (rt, at) in rlib.SIGNATURES.items():
            fn = getattr(other, name, None)                # the parent lacks the pool entry points
            if fn is not None:
                fn.restype, fn.argtypes = rt, at
        mine, rlib._LIB = rlib._LIB, other
        try:
            return StreamingBatch(sd, B, max_chunk_frames=64, max_cache_frames=cache, numerics=args.numerics)
        finally:
            rlib._LIB = mine

    def time_steps(step_fn, first):
        """mean ms per step over args.steps steps starting at chunk `first`, device-synchronised"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(first, first + args.steps):
            step_fn(c)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    # ---- in phase: pool vs lock step, alternating -----------------------------------------------------------------------------------
    if "in_phase" not in skip or "sparse" not in skip:
        pool = StreamPool(sd, B, max_chunk_frames=64, max_cache_frames=cache, numerics=args.numerics)
        eng = pool.engine
        all_slots = list(range(B))

        def pool_step(c, slots=all_slots, xs=x):
            offs = [4 * c] * len(slots)
            eng.pool_chunk(slots, xs[:, c * cf:(c + 1) * cf].contiguous().data_ptr(), cf, offs, offs, True, s)

    if "in_phase" not in skip:
        sb = lock_step_batch(args.parent_lib)

        def lock_step(c):
            sb.process_chunk(x[:, c * cf:(c + 1) * cf].contiguous())

        pool_ms, lock_ms = [], []
        for _ in range(args.reps):
            pool.reset()
            for b in all_slots:
                eng.stream_open(b, s)
            for c in range(args.warmup):
                pool_step(c)
            pool_ms.append(time_steps(pool_step, args.warmup))
            sb.reset()
            for c in range(args.warmup):
                lock_step(c)
            lock_ms.append(time_steps(lock_step, args.warmup))
        same = eng.tokens(s) == sb.engine.tokens(s)
        res["in_phase"] = {"pool_ms_per_step": pool_ms, "lock_step_ms_per_step": lock_ms, "lock_step_lib": "parent" if args.parent_lib else "this",
                           "lock_step_spread_ms": max(lock_ms) - min(lock_ms), "pool_minus_lock_step_ms": float(np.mean(pool_ms) - np.mean(lock_ms)),
                           "tokens_identical": bool(same), "launches_per_pool_step": None}
        l0 = eng.counters()[0]
        pool.reset()
        eng.stream_open(0, s)
        l0 = eng.counters()[0]
        pool_step(0)
        res["in_phase"]["launches_per_pool_step"] = eng.counters()[0] - l0
        del sb

    # ---- sparse: 4 of 64 active -------------------------------------------------------------------------------------------------------
    if "sparse" not in skip:
        act = [3, 17, 40, 62][:min(4, B)] if B >= 63 else list(range(min(4, B)))
        xs = x[act].contiguous()
        sparse_ms = []
        for _ in range(args.reps):
            pool.reset()
            for b in all_slots:
                eng.stream_open(b, s)
            for c in range(4):                              # every slot mid-utterance, then only `act` goes on
                pool_step(c)
            for c in range(4, args.warmup):
                pool_step(c, act, xs)
            sparse_ms.append(time_steps(lambda c: pool_step(c, act, xs), args.warmup))
        res["sparse"] = {"active": len(act), "ms_per_step": sparse_ms}
    if "in_phase" not in skip or "sparse" not in skip:
        del pool, eng

    # ---- staggered load --------------------------------------------------------------------------------------------------------------
    if "staggered" not in skip:
        g = np.random.Generator(np.random.Philox(key=[7, 0x5747]))
        n_utt = max(B, int(args.stagger_steps * B / 44))    # 2-12 s at 100 frames/s and 16-frame chunks: ~44 chunks per utterance
        lens = g.integers(200, 1201, n_utt)
        arrivals = np.concatenate([g.integers(0, 44, B), g.integers(0, args.stagger_steps, n_utt - B)])   # uniformly random phase
        big = torch.from_numpy(T.synth_fbank(1, 1200 + 16 * 64, seed=9))[0].cuda()
        starts = g.integers(0, 16 * 64, n_utt)
        utts = [big[int(a):int(a) + int(n)] for a, n in zip(starts, lens)]
        pool = StreamPool(sd, B, max_chunk_frames=64, max_cache_frames=512, numerics=args.numerics)
        evaluate_rtf_pool(pool, utts[:B // 4], [0] * (B // 4), cf)                 # warm-up
        pool.reset()
        r = evaluate_rtf_pool(pool, utts, [int(a) for a in arrivals], cf)
        res["staggered"] = {"utterances": n_utt, "rtf": r["greedy"], "step_ms": r["step_ms"]}
        del pool
        # the same load without the pool: one context per caller, each at B = 1 (per chunk: encoder_chunk + greedy_decode + consume)
        n_c = min(args.callers, n_utt)
        ctxs = [StreamingBatch(sd, 1, max_chunk_frames=64, max_cache_frames=512, numerics=args.numerics) for _ in range(n_c)]
        order = sorted(range(n_utt), key=lambda k: (int(arrivals[k]), k))
        waiting, live, rtfs, step_ms, t = order[:4 * n_c], {}, [], [], 0
        while waiting or live:
            while waiting and int(arrivals[waiting[0]]) <= t and len(live) < n_c:
                k = waiting.pop(0)
                i = min(set(range(n_c)) - set(live))
                ctxs[i].reset()
                live[i] = [k, list(T.chunk_plan(int(lens[k]), cf))]
            t0 = time.time()
            durs = []
            for i, (k, plan) in live.items():
                a, b = plan.pop(0)
                if b - a >= 7:
                    ctxs[i].process_chunk(utts[k][a:b][None].contiguous())
                    ctxs[i].engine.token_counts(s)       # the caller reads its tokens: synchronous, as in the pool
                    durs.append((b - a) * 0.01)
            dt = time.time() - t0
            if durs:
                step_ms.append(dt * 1e3)
                rtfs.extend(dt / d for d in durs)
            for i in [i for i, (_, plan) in live.items() if not plan]:
                del live[i]
            t += 1
        res["one_context_per_caller"] = {"callers": n_c, "rtf": _stats(rtfs), "step_ms": _stats(step_ms)}

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
