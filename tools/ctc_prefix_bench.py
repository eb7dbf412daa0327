"""CTC prefix beam search with contextual biasing: the one-launch device search against the Python loop, measured on one GPU in ONE
process.  Needs no weights: the log-probabilities are seeded (log-softmax of normal logits x --peak, a hot alphabet of 40 tokens and the
blank raised so that prefixes collide as they do on speech).  Prints one JSON line; --out writes it to a file as well.

  device_b1 / device_bN   rnnt_ctc_prefix_beam_logprobs on log-probabilities already on the device, B = 1 and B = --batch, T = --frames,
                          without a graph and with a graph of --phrases random phrases of 2..6 hot tokens
  python_b1               ctc_vr_amd.testing.ctc_prefix_beam_ref (the restatement of the reference's loop) over the downloaded row 0

Wall time around a call that ends synchronised, median of --reps repetitions after --warmup untimed ones, the variants alternating
inside every repetition.  kernel_us: HIP-event time of ctc_prefix_search (profile tag 45) from runs of their own; per frame = / T.
Row 0 of every device call must give the Python loop's tokens and times; the tool exits with status 1 when it does not.

usage: python tools/ctc_prefix_bench.py [--frames 249] [--batch 32] [--beam 10] [--phrases 100] [--reps 10] [--warmup 2] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--phrases", type=int, default=100)
    ap.add_argument("--peak", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "ctc_prefix_bench needs a GPU"
    B, F, K, V, blank = args.batch, args.frames, args.beam, T.VOCAB, T.BLANK
    rng = np.random.default_rng(2026)
    hot = np.array([v for v in range(40, 81) if v != blank][:40])
    x = args.peak * rng.standard_normal((B, F, V)).astype(np.float32)
    x[..., hot] += 4.0
    x[..., blank] += 6.0
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).contiguous()
    phrases = [hot[rng.integers(0, hot.size, rng.integers(2, 7))].tolist() for _ in range(args.phrases)]
    score = 3.0
    eng = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=V, blank_id=blank, max_beam=0)
    s = torch.cuda.current_stream().cuda_stream
    lp_d = lp.cuda()
    lp1_d = lp_d[:1].contiguous()
    lens = {1: np.full(1, F, np.int32), B: np.full(B, F, np.int32)}
    dev = {1: lp1_d, B: lp_d}
    graph = T.context_graph_ref(phrases, score)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def device(n, ctx):
        return eng.ctc_prefix_beam_logprobs(dev[n].data_ptr(), lens[n], n, F, K, ctx, False, s)

    variants = [(n, ctx) for ctx in (False, True) for n in (1, B)]
    times = {v: [] for v in variants}
    t_py = {False: [], True: []}
    got, want = {}, {}
    eng.context_set(phrases, score)                                  # set once: use_context chooses per call
    for i in range(args.warmup + args.reps):
        for v in variants:
            ms, got[v] = timed(lambda: device(*v))
            if i >= args.warmup:
                times[v].append(ms)
        if i >= args.warmup and len(t_py[False]) < max(3, args.reps // 2):   # the Python loop is slow: fewer repetitions, still alternating
            for ctx in (False, True):
                t0 = time.perf_counter()
                want[ctx] = T.ctc_prefix_beam_ref(lp[0].numpy(), F, blank, K, graph if ctx else None)[0]
                t_py[ctx].append((time.perf_counter() - t0) * 1e3)
    agree = all([(h[0], h[2]) for h in got[v][0]] == [(h[0], h[2]) for h in want[v[1]]] for v in variants)
    kernel = {}
    for v in variants:
        eng.profile_begin(45)
        device(*v)
        ms, launches = eng.profile_end()
        eng.profile_begin(0)
        assert launches == 1, launches
        kernel[v] = ms * 1e3
    med = statistics.median
    res = {"tool": "ctc_prefix_bench", "device": torch.cuda.get_device_name(0), "frames": F, "batch": B, "beam": K, "vocab": V,
           "phrases": args.phrases, "graph_nodes": len(graph.token), "reps": args.reps, "warmup": args.warmup, "python_reps": len(t_py[False])}
    for (n, ctx), ts in times.items():
        tag = f"b{n}" + ("_ctx" if ctx else "")
        res[f"device_{tag}_ms"] = round(med(ts), 3)
        res[f"device_{tag}_min_max_ms"] = [round(min(ts), 3), round(max(ts), 3)]
        res[f"kernel_{tag}_us"] = round(kernel[n, ctx], 1)
        res[f"kernel_{tag}_us_per_frame"] = round(kernel[n, ctx] / F, 2)
    for ctx in (False, True):
        tag = "_ctx" if ctx else ""
        res[f"python_b1{tag}_ms"] = round(med(t_py[ctx]), 1)
        res[f"python_over_device_b1{tag}"] = round(med(t_py[ctx]) / med(times[1, ctx]), 1)
    res[f"device_b{B}_ms_per_utterance"] = round(med(times[B, False]) / B, 3)
    res["best_tokens_b1"] = len(want[False][0][0])
    res["context_changes_best"] = want[False][0][0] != want[True][0][0]
    res["rows_agree"] = bool(agree)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
