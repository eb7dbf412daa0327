"""Per-slot beam search of the stream pool, measured on one GPU with stream_pool_bench.py's method (bench.py's seeded weights; bf16x3
unless told otherwise; every comparison inside ONE process, three alternating repetitions).  Prints one JSON line; --out writes it
to a file as well (profiles/stream_pool_beam_bench.json).

  in_phase   64 slots, chunk 16, beam 4, every slot active every step: ms per step of rnnt_pool_chunk_beam against the lock-step
             rnnt_encoder_chunk + rnnt_beam_decode + rnnt_frames_discard of a 64-stream context.  With --parent-lib the lock-step side
             runs on THAT library (the parent commit's, built beside this one); the final hypotheses must be identical.
  sparse     4 of the 64 slots active every step, the other 60 idle mid-utterance.
  mixed      half the slots greedy, half beam 4, utterances of 2-12 s with uniformly random phase arriving continuously (the
             staggered load of stream_pool_bench.py): ms per StreamPool.step.

usage: python tools/stream_pool_beam_bench.py [--parent-lib PATH] [--steps 60] [--reps 3] [--beam 4] [--numerics bf16x3] [--out FILE]"""
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
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--steps", type=int, default=60, help="timed steps per repetition (after the warm-up steps)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stagger-steps", type=int, default=100)
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--blank-bias", type=float, default=12.0, help="as bench.py")
    ap.add_argument("--skip", default="", help="comma list of legs to skip: in_phase,sparse,mixed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_delay import _stats
    from ctc_vr_amd.online_rnnt_model import StreamingBatch, StreamPool

    B, cf, K = args.slots, args.chunk, args.beam
    skip = set(args.skip.split(",")) if args.skip else set()
    sd = T.make_state_dict(0, blank_bias=args.blank_bias)
    s = torch.cuda.current_stream().cuda_stream
    n_chunks = args.warmup + args.steps
    x = torch.from_numpy(T.synth_fbank(B, n_chunks * cf, seed=5)).cuda()
    cache = 4 * n_chunks + 64
    res = {"tool": "stream_pool_beam_bench", "numerics": args.numerics, "slots": B, "chunk": cf, "beam": K, "steps": args.steps,
           "reps": args.reps, "device": torch.cuda.get_device_name(0)}

    def lock_step_batch(lib_path):
        """a lock-step context of B streams; lib_path: another build of the library (bound to the symbols it exports)"""
        kw = dict(max_chunk_frames=64, max_cache_frames=cache, max_enc_frames=16, numerics=args.numerics, max_beam=K)
        if lib_path is None:
            return StreamingBatch(sd, B, **kw)
        rlib.load()                                         # this tree's library first (and the HIP runtime torch uses)
        other = ctypes.CDLL(os.path.abspath(lib_path))
        for name, (rt, at) in rlib.SIGNATURES.items():
            fn = getattr(other, name, None)                # the parent lacks the pool's beam entry points
            if fn is not None:
                fn.restype, fn.argtypes = rt, at
        mine, rlib._LIB = rlib._LIB, other
        try:
            return StreamingBatch(sd, B, **kw)
        finally:
            rlib._LIB = mine

    def time_steps(step_fn, first):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for c in range(first, first + args.steps):
            step_fn(c)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    pool = StreamPool(sd, B, max_chunk_frames=64, max_cache_frames=cache, numerics=args.numerics, max_beam=K)
    eng = pool.engine
    all_slots = list(range(B))

    def pool_step(c, slots=all_slots, xs=x):
        offs = [4 * c] * len(slots)
        eng.pool_chunk_beam(slots, xs[:, c * cf:(c + 1) * cf].contiguous().data_ptr(), cf, offs, offs, K, s)

    if "in_phase" not in skip:
        sb = lock_step_batch(args.parent_lib)

        def lock_step(c):
            xs = x[:, c * cf:(c + 1) * cf].contiguous()
            tq = sb.engine.encoder_chunk(xs.data_ptr(), cf, 4 * c, 4 * c, s)
            sb.engine.beam_decode(0, None, K, s)
            sb.engine.frames_discard(s)
            return tq

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
        same = all([(t, np.float64(v).tobytes()) for t, v in eng.stream_beam(b, s)] == [(t, np.float64(v).tobytes()) for t, v in sb.engine.beam_hyps(b)]
                   for b in all_slots)
        res["in_phase"] = {"pool_ms_per_step": pool_ms, "lock_step_ms_per_step": lock_ms, "lock_step_lib": "parent" if args.parent_lib else "this",
                           "lock_step_spread_ms": max(lock_ms) - min(lock_ms), "pool_minus_lock_step_ms": float(np.mean(pool_ms) - np.mean(lock_ms)),
                           "hypotheses_identical": bool(same)}
        l0 = eng.counters()[0]
        pool_step(n_chunks - 1)
        res["in_phase"]["launches_per_pool_step"] = eng.counters()[0] - l0
        del sb

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
    del pool, eng

    if "mixed" not in skip:
        g = np.random.Generator(np.random.Philox(key=[7, 0x5747]))
        n_utt = max(B, int(args.stagger_steps * B / 44))    # 2-12 s at 100 frames/s and 16-frame chunks: ~44 chunks per utterance
        lens = g.integers(200, 1201, n_utt)
        arrivals = np.concatenate([g.integers(0, 44, B), g.integers(0, args.stagger_steps, n_utt - B)])
        big = torch.from_numpy(T.synth_fbank(1, 1200 + 16 * 64, seed=9))[0].cuda()
        starts = g.integers(0, 16 * 64, n_utt)
        utts = [big[int(a):int(a) + int(n)] for a, n in zip(starts, lens)]
        pool = StreamPool(sd, B, max_chunk_frames=64, max_cache_frames=512, numerics=args.numerics, max_beam=K)
        order = sorted(range(n_utt), key=lambda k: (int(arrivals[k]), k))
        waiting, live, step_ms, t = list(order), {}, [], 0
        while (waiting or live) and t < args.stagger_steps:
            while waiting and int(arrivals[waiting[0]]) <= t and pool._free:
                k = waiting.pop(0)
                slot = pool.open(beam_size=K if k % 2 else 0)           # every second caller beam-searched
                live[slot] = [k, list(T.chunk_plan(int(lens[k]), cf))]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for slot, (k, plan) in live.items():
                a, b = plan.pop(0)
                pool.feed(slot, utts[k][a:b])
            pool.step()
            for slot, (k, _) in live.items():
                if k % 2:
                    pool.beams(slot)                                     # the caller reads its hypotheses, as a greedy one its tokens
            torch.cuda.synchronize()
            if t >= 10:
                step_ms.append((time.perf_counter() - t0) * 1e3)
            for slot in [sl for sl, (_, plan) in live.items() if not plan]:
                pool.close(slot)
                del live[slot]
            t += 1
        res["mixed"] = {"steps": len(step_ms), "step_ms": _stats(step_ms)}

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
