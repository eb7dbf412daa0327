"""Hot-word biasing in the transducer prefix beam search: what the context graph costs, measured on one GPU in ONE process on seeded
weights and features.  Prints one JSON line; --out writes it to a file as well.

  decode_b<B>      rnnt_prefix_beam_decode_ctx with a graph of --phrases seeded phrases (2 to 4 tokens each) against the unbiased
                   call on the same encoder frames, at B = 1 and B = --batch, beam --beam: ms per call and us per frame
  pool_n<N>        rnnt_pool_prefix_frames_ctx over --slots slots, 3 frames per call, biased against unbiased: ms per call, us per frame
  merge_b<B>       HIP-event time per frame of prefix_merge alone (profile tag 44) with and without the graph, from runs of their own

Every wall time is around a call that ends synchronised; the biased and the unbiased variant alternate inside every repetition;
medians over --reps repetitions after --warmup untimed ones.

usage: python tools/prefix_context_bench.py [--frames 400] [--batch 32] [--slots 64] [--beam 8] [--phrases 100] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--phrases", type=int, default=100)
    ap.add_argument("--context-score", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "prefix_context_bench needs a GPU"
    B, N, F, K = args.batch, args.slots, args.frames, args.beam
    tq = ((F - 3) // 2 + 1 - 3) // 2 + 1
    eng = RnntEngine(max_streams=max(B, N), max_chunk_frames=F, max_cache_frames=tq + 8, max_enc_frames=tq + 8, vocab_size=T.VOCAB, blank_id=T.BLANK,
                     max_beam=0)
    eng.load_state_dict(T.make_state_dict(0))
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(2026)
    vocab = np.array([t for t in range(T.VOCAB) if t != T.BLANK])
    phrases = [rng.choice(vocab, size=int(rng.integers(2, 5))).tolist() for _ in range(args.phrases)]
    eng.context_set(phrases, args.context_score)
    n_enc = max(B, N)
    enc = torch.empty(n_enc, tq, 256, device="cuda")
    for b0 in range(0, n_enc, B):                                     # the encoder frames of every utterance, B at a time
        n = min(B, n_enc - b0)
        x = torch.from_numpy(T.synth_fbank(n, F, seed=2026 + b0)).cuda().contiguous()
        part = torch.empty(n, tq, 256, device="cuda")
        eng.encoder_full(x.data_ptr(), np.full(n, F, np.int32), n, F, part.data_ptr(), s)
        enc[b0:b0 + n] = part
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    med = statistics.median
    res = {"tool": "prefix_context_bench", "device": torch.cuda.get_device_name(0), "frames": F, "enc_frames": tq, "beam": K, "phrases": len(phrases),
           "context_score": args.context_score, "reps": args.reps, "warmup": args.warmup}
    for n in (1, B):
        rows, lens = enc[:n].contiguous(), np.full(n, tq, np.int32)
        plain = lambda: eng.prefix_beam_decode(rows.data_ptr(), lens, n, tq, K, 0.3, 0.7, False, s)
        biased = lambda: eng.prefix_beam_decode_ctx(rows.data_ptr(), lens, n, tq, K, 0.3, 0.7, True, False, s)
        t_p, t_b = [], []
        for i in range(args.warmup + args.reps):
            tp, hp = timed(plain)
            tb, hb = timed(biased)
            if i >= args.warmup:
                t_p.append(tp), t_b.append(tb)
        res[f"decode_b{n}_unbiased_ms"], res[f"decode_b{n}_biased_ms"] = round(med(t_p), 3), round(med(t_b), 3)
        res[f"decode_b{n}_unbiased_us_per_frame"], res[f"decode_b{n}_biased_us_per_frame"] = round(med(t_p) * 1e3 / tq, 2), round(med(t_b) * 1e3 / tq, 2)
        res[f"decode_b{n}_biased_over_unbiased"] = round(med(t_b) / med(t_p), 4)
        res[f"decode_b{n}_best_differs"] = sum(hp[b][0][0] != hb[b][0][0] for b in range(n))
        for name, fn in (("unbiased", plain), ("biased", biased)):
            eng.profile_begin(44)
            fn()
            ms, launches = eng.profile_end()
            eng.profile_begin(0)
            assert launches == tq, (launches, tq)
            res[f"merge_b{n}_{name}_us_per_frame"] = round(ms * 1e3 / tq, 2)
    slots, t = list(range(N)), 3
    calls = tq // t

    def walk(use_context):
        eng.stream_prefix_reset(-1, s)
        out = []
        for k in range(calls):
            rows = enc[:N, k * t:(k + 1) * t].contiguous()
            ms, _ = timed(lambda: eng.pool_prefix_frames_ctx(slots, rows.data_ptr(), t, K, 0.3, 0.7, use_context, s))
            out.append(ms)
        return out[2:]                                                # the first calls of a pass allocate
    t_p, t_b = [], []
    for i in range(1 + max(args.reps // 3, 1)):                       # pass 0 warms up
        p, b = walk(False), walk(True)
        if i:
            t_p += p
            t_b += b
    res[f"pool_n{N}_unbiased_ms"], res[f"pool_n{N}_biased_ms"] = round(med(t_p), 3), round(med(t_b), 3)
    res[f"pool_n{N}_unbiased_us_per_frame"], res[f"pool_n{N}_biased_us_per_frame"] = round(med(t_p) * 1e3 / t, 2), round(med(t_b) * 1e3 / t, 2)
    res[f"pool_n{N}_biased_over_unbiased"] = round(med(t_b) / med(t_p), 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
