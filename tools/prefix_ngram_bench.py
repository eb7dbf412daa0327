"""N-gram shallow fusion in the transducer prefix beam search: what the model costs, measured on one GPU in ONE process on seeded
weights and features.  Prints one JSON line; --out writes it to a file as well.

  decode_b<B>      rnnt_prefix_beam_decode_ngram with a seeded order-3 model (every unigram, --bigrams bigrams, --trigrams trigrams)
                   against the call without it on the same encoder frames, at B = 1 and B = --batch, beam --beam: ms per call and
                   us per frame
  pool_n<N>        rnnt_pool_prefix_frames_ngram over --slots slots, 3 frames per call, fused against unfused: ms per call, us per frame
  merge_b<B>       HIP-event time per frame of prefix_merge alone (profile tag 44) with and without the model, from runs of their own
  merge_pool_n<N>  the same for prefix_merge_pool (profile tag 50)
  backoff_longest  the longest back-off chain (fail arcs followed in one step) over the tokens of every returned hypothesis, EOS included

Every wall time is around a call that ends synchronised; the fused and the unfused variant alternate inside every repetition;
medians over --reps repetitions after --warmup untimed ones.  --unfused-only: only the merge times of the unfused search (tags 44
and 50), --reps values each -- what a comparison against another build of the library needs.

usage: python tools/prefix_ngram_bench.py [--frames 400] [--batch 32] [--slots 64] [--beam 8] [--reps 10] [--unfused-only] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def seeded_model(rng, vocab, blank, n_bi, n_tri, lm_weight):
    """every unigram with BOS and EOS, seeded bigrams and trigrams that extend them; values as ngram_cases draws them"""
    from ctc_vr_amd.ngram import NgramLM
    tk = [t for t in range(vocab) if t != blank]
    s = [(vocab,)] + [(t,) for t in tk] + [(vocab + 1,)]
    pairs = sorted({(int(a), int(b)) for a, b in rng.choice(tk, size=(n_bi, 2))})
    s += [(vocab, t) for t in tk[:32]] + pairs + [(t, vocab + 1) for t in tk[:32]]
    s += sorted({pairs[int(i)] + (int(c),) for i, c in zip(rng.integers(0, len(pairs), n_tri), rng.choice(tk, size=n_tri))})
    logp, bow = -rng.uniform(0.1, 5.0, len(s)), -rng.uniform(0.0, 2.0, len(s))
    return NgramLM([(g, float(p), float(b)) for g, p, b in zip(s, logp, bow)], lm_weight=lm_weight, length_bonus=0.5)


def longest_backoff(ref, seqs):
    """fail arcs followed in one step of testing.ngram_ref, at most, over the given token sequences from the start state, EOS included"""
    worst = 0
    for seq in seqs:
        state = ref.start
        for tok in list(seq) + [ref.eos_tok]:
            node, n = state, 0
            while tok not in ref.next[node] and node != 0:
                node, n = ref.fail[node], n + 1
            worst = max(worst, n)
            if tok != ref.eos_tok:
                state = ref.step(state, tok)[1]
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--bigrams", type=int, default=20000)
    ap.add_argument("--trigrams", type=int, default=20000)
    ap.add_argument("--lm-weight", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unfused-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "prefix_ngram_bench needs a GPU"
    B, N, F, K = args.batch, args.slots, args.frames, args.beam
    tq = ((F - 3) // 2 + 1 - 3) // 2 + 1
    eng = RnntEngine(max_streams=max(B, N), max_chunk_frames=F, max_cache_frames=tq + 8, max_enc_frames=tq + 8, vocab_size=T.VOCAB, blank_id=T.BLANK,
                     max_beam=0)
    eng.load_state_dict(T.make_state_dict(0))
    s = torch.cuda.current_stream().cuda_stream
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

    def merge_us(tag, fn, launches_want):
        eng.profile_begin(tag)
        fn()
        ms, launches = eng.profile_end()
        eng.profile_begin(0)
        assert launches == launches_want, (launches, launches_want)
        return ms * 1e3 / launches_want

    med = statistics.median
    slots, t = list(range(N)), 3
    calls = tq // t
    res = {"tool": "prefix_ngram_bench", "device": torch.cuda.get_device_name(0), "frames": F, "enc_frames": tq, "beam": K, "reps": args.reps,
           "warmup": args.warmup}

    def pool_pass(advance):
        eng.stream_prefix_reset(-1, s)
        out = []
        for k in range(calls):
            rows = enc[:N, k * t:(k + 1) * t].contiguous()
            ms, _ = timed(lambda: advance(rows))
            out.append(ms)
        return out[2:]                                                # the first calls of a pass allocate

    unfused_pool = lambda rows: eng.pool_prefix_frames(slots, rows.data_ptr(), t, K, 0.3, 0.7, s)           # noqa: E731
    if args.unfused_only:
        for n in (1, B):
            rows, lens = enc[:n].contiguous(), np.full(n, tq, np.int32)
            plain = lambda: eng.prefix_beam_decode(rows.data_ptr(), lens, n, tq, K, 0.3, 0.7, False, s)     # noqa: E731
            for _ in range(args.warmup):
                plain()
            res[f"merge_b{n}_unfused_us_per_frame"] = [round(merge_us(44, plain, tq), 3) for _ in range(args.reps)]
        pool_pass(unfused_pool)
        res[f"merge_pool_n{N}_unfused_us_per_frame"] = [round(merge_us(50, lambda: pool_pass(unfused_pool), calls * t), 3) for _ in range(args.reps)]
    else:
        lm = seeded_model(np.random.default_rng(2026), T.VOCAB, T.BLANK, args.bigrams, args.trigrams, args.lm_weight)
        eng.ngram_set(lm)
        ref = T.ngram_ref(lm.ngrams, T.VOCAB, T.BLANK, lm.lm_weight, lm.length_bonus, lm.unk_logp)
        res.update({"ngrams": len(lm.ngrams), "lm_weight": lm.lm_weight})
        seqs = []
        for n in (1, B):
            rows, lens = enc[:n].contiguous(), np.full(n, tq, np.int32)
            plain = lambda: eng.prefix_beam_decode(rows.data_ptr(), lens, n, tq, K, 0.3, 0.7, False, s)     # noqa: E731
            fused = lambda: eng.prefix_beam_decode_ngram(rows.data_ptr(), lens, n, tq, K, 0.3, 0.7, False, True, False, s)   # noqa: E731
            t_p, t_f = [], []
            for i in range(args.warmup + args.reps):
                tp, hp = timed(plain)
                tf, hf = timed(fused)
                if i >= args.warmup:
                    t_p.append(tp), t_f.append(tf)
            res[f"decode_b{n}_unfused_ms"], res[f"decode_b{n}_fused_ms"] = round(med(t_p), 3), round(med(t_f), 3)
            res[f"decode_b{n}_unfused_us_per_frame"], res[f"decode_b{n}_fused_us_per_frame"] = round(med(t_p) * 1e3 / tq, 2), round(med(t_f) * 1e3 / tq, 2)
            res[f"decode_b{n}_fused_over_unfused"] = round(med(t_f) / med(t_p), 4)
            res[f"decode_b{n}_best_differs"] = sum(hp[b][0][0] != hf[b][0][0] for b in range(n))
            seqs += [h[0][1:] for row in hf for h in row]
            for name, fn in (("unfused", plain), ("fused", fused)):
                res[f"merge_b{n}_{name}_us_per_frame"] = round(med([merge_us(44, fn, tq) for _ in range(3)]), 2)
        fused_pool = lambda rows: eng.pool_prefix_frames_ngram(slots, rows.data_ptr(), t, K, 0.3, 0.7, False, True, s)   # noqa: E731
        t_p, t_f = [], []
        for i in range(1 + max(args.reps // 3, 1)):                   # pass 0 warms up
            p, f = pool_pass(unfused_pool), pool_pass(fused_pool)
            if i:
                t_p += p
                t_f += f
        res[f"pool_n{N}_unfused_ms"], res[f"pool_n{N}_fused_ms"] = round(med(t_p), 3), round(med(t_f), 3)
        res[f"pool_n{N}_unfused_us_per_frame"], res[f"pool_n{N}_fused_us_per_frame"] = round(med(t_p) * 1e3 / t, 2), round(med(t_f) * 1e3 / t, 2)
        res[f"pool_n{N}_fused_over_unfused"] = round(med(t_f) / med(t_p), 4)
        for name, fn in (("unfused", unfused_pool), ("fused", fused_pool)):
            res[f"merge_pool_n{N}_{name}_us_per_frame"] = round(med([merge_us(50, lambda: pool_pass(fn), calls * t) for _ in range(3)]), 2)
        seqs += [h[0][1:] for b in range(N) for h in eng.stream_prefix_ngram(b, True, False, s)]
        res["backoff_longest"] = longest_backoff(ref, seqs)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
