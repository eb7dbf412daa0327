"""WeNet prefix beam search, host loop against device loop, measured on one GPU in ONE process (seeded weights and features; bf16x3
unless told otherwise).  Prints one JSON line; --out writes it to a file as well.

  host_loop   OnlineRNNTModel.prefix_beam_search, B = 1: the frame loop in Python over rnnt_predictor_step / rnnt_joint with two host
              synchronisations per frame (the baseline)
  device_b1   OnlineRNNTModel.prefix_beam_search_batch on the same utterance: one rnnt_encoder_full + one rnnt_prefix_beam_decode
  device_bN   the same for a batch of --batch utterances (row 0 is the B = 1 utterance)

Every time is wall time around a call that ends synchronised, median of --reps repetitions after --warmup untimed ones, the two B = 1
paths alternating.  Both paths run the same full-context encoder first; encoder_ms is that part alone and decode_ms is
rnnt_prefix_beam_decode alone on frames already encoded.  step_us / merge_us: HIP-event time of prefix_step / prefix_merge per frame
(profile tags 43 / 44), each from a run of its own.  The hypotheses of the two B = 1 paths must agree (tokens exact, scores within
2e-3) and row 0 of the batch must give the B = 1 tokens; the tool exits with status 1 when they do not.

usage: python tools/prefix_beam_bench.py [--frames 1000] [--batch 32] [--beam 5] [--reps 10] [--warmup 2] [--numerics bf16x3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel

    assert torch.cuda.is_available(), "prefix_beam_bench needs a GPU"
    B, F, K = args.batch, args.frames, args.beam
    tq = ((F - 3) // 2 + 1 - 3) // 2 + 1
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=T.BLANK, max_streams=B, max_chunk_frames=F,
                        max_cache_frames=tq + 8, max_enc_frames=tq + 8, max_beam=0, numerics=args.numerics)
    m.load_state_dict(T.make_state_dict(0))
    x = torch.from_numpy(T.synth_fbank(B, F, seed=2026)).cuda().contiguous()
    x1, lens1, lensB = x[:1].contiguous(), torch.tensor([F]), torch.full((B,), F)
    eng, s = m._engine, torch.cuda.current_stream().cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    host = lambda: m.prefix_beam_search(x1, lens1, beam_size=K)
    dev1 = lambda: m.prefix_beam_search_batch(x1, lens1, beam_size=K)
    devB = lambda: m.prefix_beam_search_batch(x, lensB, beam_size=K)
    for _ in range(args.warmup):
        host(), dev1(), devB()
    t_host, t_dev1, t_devB = [], [], []
    for _ in range(args.reps):
        th, want = timed(host)
        td, got = timed(dev1)
        tb, gotB = timed(devB)
        t_host.append(th), t_dev1.append(td), t_devB.append(tb)
    agree = [t for t, _ in got[0]] == [t for t, _ in want] and max(abs(a - b) for (_, a), (_, b) in zip(got[0], want)) < 2e-3
    agree_batch = [t for t, _ in gotB[0]] == [t for t, _ in got[0]]

    def decode_only(n):
        """encoder once, then rnnt_prefix_beam_decode alone: (encoder ms, decode ms, prefix_step us / frame, prefix_merge us / frame)"""
        xs, ls = x[:n].contiguous(), np.full(n, F, np.int32)
        enc = torch.empty(n, tq, 256, device="cuda")
        t_enc, t_dec = [], []
        for i in range(args.warmup + args.reps):
            te, _ = timed(lambda: eng.encoder_full(xs.data_ptr(), ls, n, F, enc.data_ptr(), s))
            tdc, _ = timed(lambda: eng.prefix_beam_decode(enc.data_ptr(), np.full(n, tq, np.int32), n, tq, K, 0.3, 0.7, True, s))
            if i >= args.warmup:
                t_enc.append(te), t_dec.append(tdc)
        per_frame = []
        for tag in (43, 44):
            eng.profile_begin(tag)
            eng.prefix_beam_decode(enc.data_ptr(), np.full(n, tq, np.int32), n, tq, K, 0.3, 0.7, True, s)
            ms, launches = eng.profile_end()
            eng.profile_begin(0)
            assert launches == tq, (tag, launches, tq)
            per_frame.append(ms * 1e3 / tq)
        return statistics.median(t_enc), statistics.median(t_dec), per_frame[0], per_frame[1]
    e1, d1, s1, g1 = decode_only(1)
    eB, dB, sB, gB = decode_only(B)
    med = statistics.median
    res = {"tool": "prefix_beam_bench", "device": torch.cuda.get_device_name(0), "numerics": args.numerics, "frames": F, "enc_frames": tq,
           "batch": B, "beam": K, "reps": args.reps, "warmup": args.warmup,
           "host_loop_ms": round(med(t_host), 3), "host_loop_min_max_ms": [round(min(t_host), 3), round(max(t_host), 3)],
           "device_b1_ms": round(med(t_dev1), 3), "device_b1_min_max_ms": [round(min(t_dev1), 3), round(max(t_dev1), 3)],
           f"device_b{B}_ms": round(med(t_devB), 3), f"device_b{B}_min_max_ms": [round(min(t_devB), 3), round(max(t_devB), 3)],
           "host_over_device_b1": round(med(t_host) / med(t_dev1), 3),
           f"device_b{B}_ms_per_utterance": round(med(t_devB) / B, 3),
           "encoder_b1_ms": round(e1, 3), "decode_b1_ms": round(d1, 3), f"encoder_b{B}_ms": round(eB, 3), f"decode_b{B}_ms": round(dB, 3),
           "host_decode_b1_ms": round(med(t_host) - e1, 3), "host_over_device_decode_b1": round((med(t_host) - e1) / d1, 3),
           "step_us_per_frame_b1": round(s1, 2), "merge_us_per_frame_b1": round(g1, 2),
           f"step_us_per_frame_b{B}": round(sB, 2), f"merge_us_per_frame_b{B}": round(gB, 2),
           "best_tokens_b1": len(got[0][0][0]), "hyps_agree": bool(agree), "batch_row0_agrees": bool(agree_batch)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if agree and agree_batch else 1


if __name__ == "__main__":
    sys.exit(main())
