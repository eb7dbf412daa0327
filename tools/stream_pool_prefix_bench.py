"""Transducer prefix beam search (CTC-fused) per slot of the stream pool, measured on one GPU in ONE process on seeded weights.
Prints one JSON line; --out writes it to a file as well.

  pool_prefix_b<K>   rnnt_pool_chunk_prefix per call (encode + CTC + search of t' = 3 new frames per slot) at every --beams beam and
                     every --slots count of active slots
  pool_greedy        rnnt_pool_chunk(greedy=1) of the same rows: what the pool costs per call today
  rerun_b<K>         what a live caller had to do before, for ONE stream: after every chunk rnnt_prefix_beam_decode from frame 0 over
                     all encoder frames so far (the encoder's cost is not in it); summed over the utterance, against the summed
                     pool_prefix calls of one slot less the summed encode-only calls (rnnt_pool_chunk(greedy=0) + discard)
  step_*_us          HIP-event time per frame of prefix_step_pool (profile tag 49) over one pass of n slots -- step_pool4: up to 4
                     hypotheses of a slot per workgroup (a context created with RNNT_PREFIX_GROUP=4), step_pool1: one per workgroup
                     (RNNT_PREFIX_GROUP=1), step_pool: the library's own choice by the size of the launch -- against prefix_step (tag
                     43: one hypothesis per workgroup) of one rnnt_prefix_beam_decode call over the same n utterances at the same
                     beam; merge_*_us likewise for tags 50 and 44

An utterance is --seconds of 10 ms frames in --chunk-frame chunks.  Every variant walks whole utterances; the variants alternate inside
every repetition; a call's wall time ends synchronised; medians over the calls after the first --skip chunks of every pass and over
--reps repetitions.

usage: python tools/stream_pool_prefix_bench.py [--slots 1,32,64] [--beams 4,10] [--seconds 10] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,32,64")
    ap.add_argument("--beams", default="4,10")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--ctc-weight", type=float, default=0.3)
    ap.add_argument("--transducer-weight", type=float, default=0.7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "stream_pool_prefix_bench needs a GPU"
    counts = [int(v) for v in args.slots.split(",")]
    beams = [int(v) for v in args.beams.split(",")]
    N, C, V, blank, cw, tw = max(counts), args.chunk, T.VOCAB, T.BLANK, args.ctc_weight, args.transducer_weight
    n_chunks = int(args.seconds * 100) // C
    tq = ((C - 3) // 2 + 1 - 3) // 2 + 1
    F = n_chunks * tq
    eng = RnntEngine(max_streams=N, max_chunk_frames=64, max_cache_frames=max(512, 2 * F), max_enc_frames=64, max_tokens=8192, vocab_size=V,
                     blank_id=blank, max_beam=0)
    eng.load_state_dict(T.make_state_dict(0))
    s = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(T.synth_fbank(N, n_chunks * C, seed=7)).cuda()

    def walk(n, call):
        """one utterance in every one of n slots through `call(slots, chunk tensor, offsets)`; per-call wall times in ms"""
        eng.reset(N, s)
        slots, out = list(range(n)), []
        for k in range(n_chunks):
            chunk = x[:n, k * C:(k + 1) * C].contiguous()
            offs = [4 * k] * n
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(slots, chunk, offs)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def encode_only(slots, chunk, offs):
        eng.pool_chunk(slots, chunk.data_ptr(), C, offs, offs, False, s)
        eng.frames_discard(s)

    def prefix(K):
        return lambda sl, c, o: eng.pool_chunk_prefix(sl, c.data_ptr(), C, o, o, K, cw, tw, s)

    variants = {"pool_greedy": lambda sl, c, o: eng.pool_chunk(sl, c.data_ptr(), C, o, o, True, s), "encode_only": encode_only}
    variants.update({f"pool_prefix_b{K}": prefix(K) for K in beams})
    per_call = {(name, n): [] for name in variants for n in counts}
    totals = {name: [] for name in variants}
    # the frames of every stream, for the re-run and the batch kernels: rnnt_pool_chunk(greedy=0) chunk by chunk
    enc = torch.empty(N, F, 256, device="cuda")

    def grab(slots, chunk, offs):
        eng.pool_chunk(slots, chunk.data_ptr(), C, offs, offs, False, s)
        k = offs[0] // 4
        enc[:, k * tq:(k + 1) * tq] = torch.from_numpy(eng.enc_frames()).cuda()
        eng.frames_discard(s)
    walk(N, grab)
    rerun = {K: [] for K in beams}
    for rep in range(1 + args.reps):                                  # repetition 0 warms up
        for name, call in variants.items():
            for n in counts:
                ts = walk(n, call)
                if rep:
                    per_call[name, n] += ts[args.skip:]
                    if n == 1:
                        totals[name].append(sum(ts))
        for K in beams:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(1, n_chunks + 1):
                eng.prefix_beam_decode(enc.data_ptr(), [k * tq], 1, F, K, cw, tw, False, s)
            if rep:
                rerun[K].append((time.perf_counter() - t0) * 1e3)
    kernel = {}
    main = eng
    for group in ("1", "4"):                                          # the two shapes of the step kernel, forced: contexts of their own
        os.environ["RNNT_PREFIX_GROUP"] = group
        eng = RnntEngine(max_streams=N, max_chunk_frames=64, max_cache_frames=max(512, 2 * F), max_enc_frames=64, max_tokens=8192, vocab_size=V,
                         blank_id=blank, max_beam=0)
        del os.environ["RNNT_PREFIX_GROUP"]
        eng.load_state_dict(T.make_state_dict(0))
        for K in beams:
            for n in counts:
                walk(n, prefix(K))                                    # warm: the first call allocates
                eng.profile_begin(49)
                walk(n, prefix(K))
                ms, launches = eng.profile_end()
                assert launches == F, launches
                kernel["step_pool" + group, K, n] = ms * 1e3 / launches
        eng.profile_begin(0)
        eng.close()
    eng = main
    for K in beams:
        for n in counts:
            for tag, name in ((49, "step_pool"), (50, "merge_pool")):
                eng.profile_begin(tag)
                walk(n, variants[f"pool_prefix_b{K}"])
                ms, launches = eng.profile_end()
                assert launches == F, launches
                kernel[name, K, n] = ms * 1e3 / launches
            for tag, name in ((43, "step_batch"), (44, "merge_batch")):
                eng.profile_begin(tag)
                eng.prefix_beam_decode(enc.data_ptr(), [F] * n, n, F, K, cw, tw, False, s)
                ms, launches = eng.profile_end()
                assert launches == F, launches
                kernel[name, K, n] = ms * 1e3 / launches
            eng.profile_begin(0)
    med = statistics.median
    res = {"tool": "stream_pool_prefix_bench", "device": torch.cuda.get_device_name(0), "chunk_frames": C, "frames_per_call": tq,
           "chunks": n_chunks, "beams": beams, "vocab": V, "ctc_weight": cw, "transducer_weight": tw, "reps": args.reps}
    enc_total = med(totals["encode_only"])
    for n in counts:
        g = med(per_call["pool_greedy", n])
        res[f"pool_greedy_n{n}_ms"] = round(g, 3)
        res[f"encode_only_n{n}_ms"] = round(med(per_call["encode_only", n]), 3)
        for K in beams:
            name = f"pool_prefix_b{K}"
            res[f"{name}_n{n}_ms"] = round(med(per_call[name, n]), 3)
            res[f"{name}_over_greedy_n{n}"] = round(med(per_call[name, n]) / g, 3)
            for kn in ("step_pool", "step_pool1", "step_pool4", "step_batch", "merge_pool", "merge_batch"):
                res[f"{kn}_b{K}_n{n}_us"] = round(kernel[kn, K, n], 2)
    for K in beams:
        res[f"utterance_rerun_b{K}_ms"] = round(med(rerun[K]), 1)
        res[f"utterance_pool_search_b{K}_ms"] = round(med(totals[f"pool_prefix_b{K}"]) - enc_total, 1)
    res["utterance_encode_only_ms"] = round(enc_total, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
