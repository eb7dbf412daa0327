"""N-gram shallow fusion in the CTC prefix beam search: what the model costs, measured on one GPU in ONE process.  Needs no weights:
the log-probabilities are seeded as in tools/ctc_prefix_bench.py, the model is a synthetic order-3 back-off model over the whole
vocabulary (every unigram, --bigrams random bigrams, --trigrams random extensions of them, BOS and EOS).  Prints one JSON line; --out
writes it to a file as well.

  device_b1 / device_bN   rnnt_ctc_prefix_beam_logprobs_ngram on log-probabilities already on the device, B = 1 and B = --batch,
                          T = --frames, with use_ngram off and on (the model is set either way)
  pool_N                  one rnnt_pool_ctc_prefix_logprobs_ngram call that advances --slots slots by --pool-frames frames, off and on
  ngram_score             one rnnt_ngram_score call over --batch sequences of --frames / 4 tokens

Wall time around a call that ends synchronised, median of --reps repetitions after --warmup untimed ones, the variants alternating
inside every repetition.  kernel_us: HIP-event time of ctc_prefix_search (profile tag 45) / ctc_prefix_search_pool (tag 46) from runs
of their own; per frame = / T.  Row 0 of the device call with the model must give the f64 restatement's tokens and times, and the
call without it the plain entry point's bytes; the tool exits with status 1 when they do not.

usage: python tools/ctc_prefix_ngram_bench.py [--frames 249] [--batch 32] [--beam 10] [--slots 64] [--pool-frames 16] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_model(rng, vocab, blank, n_bi, n_tri, hot):
    """order 3 over the whole vocabulary; half of the bigrams and trigrams stay inside the hot alphabet, where the search walks"""
    from ctc_vr_amd.ngram import NgramLM
    real = [t for t in range(vocab) if t != blank]
    grams = [((vocab,), -2.0, -0.3)] + [((t,), -float(rng.uniform(2, 8)), -float(rng.uniform(0, 1))) for t in real] + [((vocab + 1,), -3.0, 0.0)]
    pairs = set()
    while len(pairs) < n_bi:
        pool = hot if len(pairs) % 2 else real
        pairs.add((int(rng.choice(pool)), int(rng.choice(pool))))
    pairs = sorted(pairs)
    grams += [(p, -float(rng.uniform(0.5, 5)), -float(rng.uniform(0, 1))) for p in pairs]
    tris = set()
    while len(tris) < n_tri:
        a, b = pairs[int(rng.integers(0, len(pairs)))]
        tris.add((a, b, int(rng.choice(hot if len(tris) % 2 else real))))
    grams += [(t, -float(rng.uniform(0.2, 4)), 0.0) for t in sorted(tris)]
    return NgramLM(grams, lm_weight=0.5, length_bonus=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--pool-frames", type=int, default=16)
    ap.add_argument("--bigrams", type=int, default=20000)
    ap.add_argument("--trigrams", type=int, default=40000)
    ap.add_argument("--peak", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "ctc_prefix_ngram_bench needs a GPU"
    B, F, K, V, blank, S, PF = args.batch, args.frames, args.beam, T.VOCAB, T.BLANK, args.slots, args.pool_frames
    rng = np.random.default_rng(2026)
    hot = np.array([v for v in range(40, 81) if v != blank][:40])
    x = args.peak * rng.standard_normal((max(B, S), F, V)).astype(np.float32)
    x[..., hot] += 4.0
    x[..., blank] += 6.0
    lp = torch.log_softmax(torch.from_numpy(x), dim=-1).contiguous()
    model = synthetic_model(rng, V, blank, args.bigrams, args.trigrams, hot)
    eng = RnntEngine(max_streams=S, max_chunk_frames=16, max_cache_frames=max(PF * (args.reps + args.warmup + 4), 16), max_enc_frames=16, vocab_size=V,
                     blank_id=blank, max_beam=0)
    s = torch.cuda.current_stream().cuda_stream
    lp_d = lp.cuda()
    dev = {1: lp_d[:1].contiguous(), B: lp_d[:B].contiguous()}
    lens = {1: np.full(1, F, np.int32), B: np.full(B, F, np.int32)}
    pool_rows = lp_d[:S, :PF].contiguous()
    slots = {False: list(range(0, S)), True: list(range(0, S))}
    seqs = [hot[rng.integers(0, hot.size, max(F // 4, 1))].tolist() for _ in range(B)]
    t0 = time.perf_counter()
    eng.ngram_set(model)
    set_ms = (time.perf_counter() - t0) * 1e3

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def device(n, on):
        return eng.ctc_prefix_beam_logprobs_ngram(dev[n].data_ptr(), lens[n], n, F, K, False, on, True, s)

    def pool(on):
        eng.pool_ctc_prefix_logprobs_ngram(slots[on], pool_rows.data_ptr(), PF, K, False, on, s)

    variants = [(n, on) for on in (False, True) for n in (1, B)]
    times = {v: [] for v in variants}
    t_pool, t_score, got = {False: [], True: []}, [], {}
    for i in range(args.warmup + args.reps):
        for v in variants:
            ms, got[v] = timed(lambda: device(*v))
            if i >= args.warmup:
                times[v].append(ms)
        for on in (False, True):                                      # the slots start over so that every call walks the same frames
            eng.stream_ctc_prefix_reset(-1, s)
            ms, _ = timed(lambda: pool(on))
            if i >= args.warmup:
                t_pool[on].append(ms)
        ms, _ = timed(lambda: eng.ngram_score(seqs, True, s))
        if i >= args.warmup:
            t_score.append(ms)
    want = T.ctc_prefix_beam_ngram_ref(lp[0].numpy(), F, blank, K, None, T.ngram_ref(model.ngrams, V, blank, model.lm_weight, model.length_bonus,
                                                                                       model.unk_logp))[0]
    plain = eng.ctc_prefix_beam_logprobs(dev[B].data_ptr(), lens[B], B, F, K, False, True, s)[1]
    agree = [(h[0], h[2]) for h in got[1, True][0][0]] == [(h[0], h[2]) for h in want]
    agree = agree and [h[4] for h in got[1, True][0][0]] == [h[4] for h in want]
    agree = agree and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got[B, False][1][:6], plain))
    kernel, kernel_pool = {}, {}
    for v in variants:
        eng.profile_begin(45)
        device(*v)
        ms, launches = eng.profile_end()
        eng.profile_begin(0)
        assert launches == 1, launches
        kernel[v] = ms * 1e3
    for on in (False, True):
        eng.stream_ctc_prefix_reset(-1, s)
        eng.profile_begin(46)
        pool(on)
        torch.cuda.synchronize()
        ms, launches = eng.profile_end()
        eng.profile_begin(0)
        assert launches == 1, launches
        kernel_pool[on] = ms * 1e3
    med = statistics.median
    res = {"tool": "ctc_prefix_ngram_bench", "device": torch.cuda.get_device_name(0), "frames": F, "batch": B, "beam": K, "vocab": V, "slots": S,
           "pool_frames": PF, "ngrams": len(model.ngrams), "ngram_set_ms": round(set_ms, 1), "reps": args.reps, "warmup": args.warmup}
    for (n, on), ts in times.items():
        tag = f"b{n}" + ("_ngram" if on else "")
        res[f"device_{tag}_ms"] = round(med(ts), 3)
        res[f"device_{tag}_min_max_ms"] = [round(min(ts), 3), round(max(ts), 3)]
        res[f"kernel_{tag}_us"] = round(kernel[n, on], 1)
        res[f"kernel_{tag}_us_per_frame"] = round(kernel[n, on] / F, 2)
    for on in (False, True):
        tag = f"pool_{S}" + ("_ngram" if on else "")
        res[f"{tag}_ms"] = round(med(t_pool[on]), 3)
        res[f"{tag}_min_max_ms"] = [round(min(t_pool[on]), 3), round(max(t_pool[on]), 3)]
        res[f"kernel_{tag}_us"] = round(kernel_pool[on], 1)
        res[f"kernel_{tag}_us_per_frame"] = round(kernel_pool[on] / PF, 2)
    for n in (1, B):
        res[f"ngram_over_off_b{n}_us_per_frame"] = round((kernel[n, True] - kernel[n, False]) / F, 2)
    res[f"ngram_over_off_pool_{S}_us_per_frame"] = round((kernel_pool[True] - kernel_pool[False]) / PF, 2)
    res["ngram_score_ms"] = round(med(t_score), 3)
    res["ngram_score_min_max_ms"] = [round(min(t_score), 3), round(max(t_score), 3)]
    res["ngram_score_tokens"] = sum(map(len, seqs))
    res["model_changes_best"] = got[1, True][0][0][0][0] != got[1, False][0][0][0][0]
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
