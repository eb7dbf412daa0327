"""Forced alignment at the training-shaped lattice (B64 x T249 x U28, bf16x3 by default): what the Viterbi launches cost,
back-trace included, against the alpha recursions over the same inputs.

Three alternating repetitions in one process on the same seeded inputs, after warm-up, all timed with HIP events:
  * transducer_viterbi (tag 42) against transducer_alpha (tag 41), both inside rnnt_transducer_align with nll_host given, so they
    run over the same picked lattice;
  * ctc_viterbi (tag 42, rnnt_ctc_align) against ctc_alpha (tag 41, rnnt_ctc_nll) over the same encoder frames;
  * the whole rnnt_transducer_align call (without nll) against the whole rnnt_transducer_nll call, events around the
    synchronising call.
The expectation to check: a Viterbi launch is not slower than its alpha launch by more than the spread (max - min) of the
alpha's three repetitions.  Scores and paths must agree across repetitions.  Writes one JSON document.

usage: python tools/align_bench.py [--out profiles/align_bench.json] [--numerics bf16x3] [--reps 3] [--iters 5]"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    assert torch.cuda.is_available(), "align_bench needs a GPU: there is no CPU timing"
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

    def align(want_nll=False):
        return eng.transducer_align(enc.data_ptr(), el, tg, tl, B, Tn, want_nll=want_nll, stream=s)

    def score():
        return eng.transducer_nll(enc.data_ptr(), el, tg, tl, B, Tn, None, s)

    def ctc_align():
        return eng.ctc_align(enc.data_ptr(), el, tg, tl, B, Tn, s)

    def ctc_score():
        return eng.ctc_nll(enc.data_ptr(), el, tg, tl, B, Tn, s)

    def call_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def kernel_us(tag, fn):
        eng.profile_begin(tag)
        fn()
        torch.cuda.synchronize()
        ms, n = eng.profile_end()
        assert n == 1, (tag, n)
        return ms * 1e3

    for _ in range(2):
        best0, emit0, nll0 = align(True)
        score()
        cbest0, cal0 = ctc_align()
        ctc_score()
    torch.cuda.synchronize()
    med = lambda v: float(np.median(v))
    reps, identical = [], True
    for _ in range(args.reps):
        ta, tn = [], []
        for _ in range(args.iters):
            ms, (best, emit) = call_ms(align)
            ta.append(ms)
            identical = identical and np.array_equal(best.view(np.uint64), best0.view(np.uint64)) and np.array_equal(emit, emit0)
            tn.append(call_ms(score)[0])
        reps.append({"align_call_ms": round(med(ta), 4), "nll_call_ms": round(med(tn), 4),
                     "transducer_alpha_us": round(kernel_us(41, lambda: align(True)), 2),
                     "transducer_viterbi_us": round(kernel_us(42, lambda: align(True)), 2),
                     "ctc_alpha_us": round(kernel_us(41, ctc_score), 2), "ctc_viterbi_us": round(kernel_us(42, ctc_align), 2)})
    col = lambda k: [r[k] for r in reps]
    spread = lambda k: max(col(k)) - min(col(k))
    res = {"workload": f"B{B} x T{Tn} x U{U1} (V{V}), {args.numerics}, full lengths", "reps": reps}
    for k in reps[0]:
        res[k] = med(col(k))
    res.update({
        "transducer_alpha_spread_us": round(spread("transducer_alpha_us"), 2), "ctc_alpha_spread_us": round(spread("ctc_alpha_us"), 2),
        "nll_call_spread_ms": round(spread("nll_call_ms"), 4),
        "transducer_viterbi_over_alpha": round(res["transducer_viterbi_us"] / res["transducer_alpha_us"], 4),
        "ctc_viterbi_over_alpha": round(res["ctc_viterbi_us"] / res["ctc_alpha_us"], 4),
        "transducer_viterbi_no_slower_than_alpha": bool(res["transducer_viterbi_us"] <= res["transducer_alpha_us"] + spread("transducer_alpha_us")),
        "ctc_viterbi_no_slower_than_alpha": bool(res["ctc_viterbi_us"] <= res["ctc_alpha_us"] + spread("ctc_alpha_us")),
        "align_call_no_slower_than_nll_call": bool(res["align_call_ms"] <= res["nll_call_ms"] + spread("nll_call_ms")),
        "identical_across_calls": bool(identical), "best_le_minus_nll": bool((best0 <= -nll0).all()),
        "best_mean": float(best0.mean()), "nll_mean": float(nll0.mean()), "ctc_best_mean": float(cbest0.mean()),
        "device": torch.cuda.get_device_name(0)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
