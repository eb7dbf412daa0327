"""CTC prefix beam search with hot-word biasing per slot of the stream pool, measured on one GPU in ONE process on seeded weights.
Prints one JSON line; --out writes it to a file as well.

  pool_ctc / pool_ctc_ctx   rnnt_pool_chunk_ctc_prefix per call (encode + CTC + search of t' = 3 new frames per slot), without a graph and
                            with a graph of --phrases random phrases, at every --slots count of active slots
  pool_greedy               rnnt_pool_chunk(greedy=1) of the same rows: what the pool costs per call today
  rerun                     what a user had to do before, for ONE stream: after every chunk rnnt_ctc_prefix_beam_decode from frame 0 over
                            all encoder frames so far (the encoder's cost is not in it); summed over the utterance, against the summed
                            pool_ctc calls of one slot less the summed encode-only calls (rnnt_pool_chunk(greedy=0) + discard)

An utterance is --seconds of 10 ms frames in --chunk-frame chunks.  Every variant walks whole utterances; the variants alternate inside
every repetition; a call's wall time ends synchronised; medians over the calls after the first --skip chunks of every pass and over
--reps repetitions.  kernel_us_per_frame: HIP-event time of ctc_prefix_search_pool (profile tag 46) over one pass / launches / t'.

usage: python tools/stream_pool_ctc_prefix_bench.py [--slots 1,32,64] [--seconds 10] [--beam 10] [--phrases 100] [--reps 3] [--out FILE]"""
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
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--phrases", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "stream_pool_ctc_prefix_bench needs a GPU"
    counts = [int(v) for v in args.slots.split(",")]
    N, C, K, V, blank = max(counts), args.chunk, args.beam, T.VOCAB, T.BLANK
    n_chunks = int(args.seconds * 100) // C
    tq = ((C - 3) // 2 + 1 - 3) // 2 + 1
    rng = np.random.default_rng(2026)
    hot = np.array([v for v in range(40, 81) if v != blank][:40])
    phrases = [hot[rng.integers(0, hot.size, rng.integers(2, 7))].tolist() for _ in range(args.phrases)]
    eng = RnntEngine(max_streams=N, max_chunk_frames=64, max_cache_frames=max(512, 2 * n_chunks * tq), max_enc_frames=64, max_tokens=8192,
                     vocab_size=V, blank_id=blank, max_beam=0)
    eng.load_state_dict(T.make_state_dict(0))
    eng.context_set(phrases, 3.0)
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

    variants = {"pool_greedy": lambda sl, c, o: eng.pool_chunk(sl, c.data_ptr(), C, o, o, True, s),
                "pool_ctc": lambda sl, c, o: eng.pool_chunk_ctc_prefix(sl, c.data_ptr(), C, o, o, K, False, s),
                "pool_ctc_ctx": lambda sl, c, o: eng.pool_chunk_ctc_prefix(sl, c.data_ptr(), C, o, o, K, True, s),
                "encode_only": encode_only}
    per_call = {(name, n): [] for name in variants for n in counts}
    totals = {name: [] for name in variants}
    # the frames of stream 0, for the re-run: rnnt_pool_chunk(greedy=0) chunk by chunk
    enc = torch.empty(1, n_chunks * tq, 256, device="cuda")

    def grab(slots, chunk, offs):
        eng.pool_chunk(slots, chunk.data_ptr(), C, offs, offs, False, s)
        k = offs[0] // 4
        enc[0, k * tq:(k + 1) * tq] = torch.from_numpy(eng.enc_frames()[0]).cuda()
        eng.frames_discard(s)
    walk(1, grab)
    rerun = {False: [], True: []}
    for rep in range(1 + args.reps):                                  # repetition 0 warms up
        for name, call in variants.items():
            for n in counts:
                ts = walk(n, call)
                if rep:
                    per_call[name, n] += ts[args.skip:]
                    if n == 1:
                        totals[name].append(sum(ts))
        for ctx in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(1, n_chunks + 1):
                eng.ctc_prefix_beam_decode(enc.data_ptr(), [k * tq], 1, n_chunks * tq, K, ctx, False, s)
            if rep:
                rerun[ctx].append((time.perf_counter() - t0) * 1e3)
    kernel = {}
    for ctx in (False, True):
        for n in counts:
            eng.profile_begin(46)
            walk(n, variants["pool_ctc_ctx" if ctx else "pool_ctc"])
            ms, launches = eng.profile_end()
            eng.profile_begin(0)
            assert launches == n_chunks, launches
            kernel[ctx, n] = ms * 1e3 / launches / tq
    med = statistics.median
    res = {"tool": "stream_pool_ctc_prefix_bench", "device": torch.cuda.get_device_name(0), "chunk_frames": C, "frames_per_call": tq,
           "chunks": n_chunks, "beam": K, "vocab": V, "phrases": args.phrases, "reps": args.reps}
    for n in counts:
        g = med(per_call["pool_greedy", n])
        res[f"pool_greedy_n{n}_ms"] = round(g, 3)
        for name in ("pool_ctc", "pool_ctc_ctx"):
            res[f"{name}_n{n}_ms"] = round(med(per_call[name, n]), 3)
            res[f"{name}_over_greedy_n{n}"] = round(med(per_call[name, n]) / g, 3)
        res[f"kernel_n{n}_us_per_frame"] = round(kernel[False, n], 2)
        res[f"kernel_ctx_n{n}_us_per_frame"] = round(kernel[True, n], 2)
    enc_total = med(totals["encode_only"])
    for ctx, name in ((False, "pool_ctc"), (True, "pool_ctc_ctx")):
        tag = "_ctx" if ctx else ""
        res[f"utterance_rerun{tag}_ms"] = round(med(rerun[ctx]), 1)
        res[f"utterance_pool_search{tag}_ms"] = round(med(totals[name]) - enc_total, 1)
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
