"""What endpoint detection costs a stream pool on one GPU (bench.py's seeded weights with the CTC head's blank bias raised; bf16x3 unless
told otherwise), every comparison inside ONE process.  Prints one JSON line; --out writes it to a file as well
(profiles/stream_pool_endpoint_bench.json).

  per chunk length (16 and 64 frames): 64 slots on 10 s utterances, every slot active in every greedy rnnt_pool_chunk call (which
  synchronises: a host clock around it times the call).  Whole utterances alternate between endpointing OFF for all slots -- the
  library's behaviour before the feature: no extra launch -- and ON for all 64; every shape is warmed up by one utterance of each kind
  first.  Reported: mean ms per call of every repetition, on minus off, the spread of the off runs, the launches per call of either
  kind, and the time of one endpoints read of the 64 slots (rnnt_pool_get_endpoints: one download).

The kernel's own time comes from a separate run under `rocprofv3 --kernel-trace --stats` (--trace-run: one ON utterance per chunk
length and nothing else).

usage: python tools/stream_pool_endpoint_bench.py [--slots 64] [--frames 1000] [--reps 3] [--numerics bf16x3] [--trace-run] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000, help="fbank frames per utterance (10 ms each)")
    ap.add_argument("--chunks", default="16,64")
    ap.add_argument("--reps", type=int, default=3, help="alternating (off, on) pairs of whole utterances per chunk length")
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--blank-bias", type=float, default=12.0, help="as bench.py")
    ap.add_argument("--ctc-blank-bias", type=float, default=6.0, help="added to ctc_head.ctc_lo.bias[blank]: frames on both sides of the threshold")
    ap.add_argument("--trace-run", action="store_true", help="one ON utterance per chunk length, for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine

    B = args.slots
    sd = T.make_state_dict(0, blank_bias=args.blank_bias)
    sd["ctc_head.ctc_lo.bias"] = sd["ctc_head.ctc_lo.bias"].copy()
    sd["ctc_head.ctc_lo.bias"][T.BLANK] += np.float32(args.ctc_blank_bias)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(T.synth_fbank(B, args.frames, seed=5)).cuda()
    eng = RnntEngine(max_streams=B, max_chunk_frames=64, max_cache_frames=args.frames // 4 + 64, max_enc_frames=16, max_tokens=4096)
    eng.load_state_dict(sd, numerics=args.numerics)
    slots = list(range(B))
    cfg = (0.42, 1, 125, 25, 500)                            # WeNet's usual rules; the threshold splits this head's frames
    res = {"tool": "stream_pool_endpoint_bench", "numerics": args.numerics, "slots": B, "frames": args.frames, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "config": cfg, "chunks": {}}

    def utterance(cf, on):
        """every slot through one utterance in chunks of cf frames -> (ms of every call, launches of the last call, read ms, states)"""
        tq = ((cf - 3) // 2 + 1 - 3) // 2 + 1
        eng.reset(B, s)
        for b in slots:
            eng.stream_open(b, s)
            if on:
                eng.stream_endpoint(b, cfg, s)
        torch.cuda.synchronize()
        ms, launches = [], 0
        for c in range(args.frames // cf):
            xs = x[:, c * cf:(c + 1) * cf].contiguous()
            offs = [tq * c] * B
            torch.cuda.synchronize()
            l0 = eng.counters()[0]
            t0 = time.perf_counter()
            eng.pool_chunk(slots, xs.data_ptr(), cf, offs, offs, True, s)      # synchronises (the greedy decode's last step)
            ms.append((time.perf_counter() - t0) * 1e3)
            launches = eng.counters()[0] - l0
        read_ms, st = None, None
        if on:
            t0 = time.perf_counter()
            st = eng.pool_endpoints(slots, s)
            read_ms = (time.perf_counter() - t0) * 1e3
        return ms, launches, read_ms, st

    for cf in [int(v) for v in args.chunks.split(",")]:
        if args.trace_run:
            utterance(cf, True)
            continue
        utterance(cf, False)                                 # warm-up of this shape, both kinds
        utterance(cf, True)
        off, on, reads, tokens = [], [], [], {}
        for _ in range(args.reps):
            for kind in (False, True):
                ms, launches, read_ms, st = utterance(cf, kind)
                (on if kind else off).append(float(np.mean(ms)))
                tokens[kind] = eng.tokens(s)
                res["chunks"].setdefault(str(cf), {})["launches_per_call_on" if kind else "launches_per_call_off"] = launches
                if kind:
                    reads.append(read_ms)
                    fired = np.bincount(st[:, 3], minlength=4).tolist()
        r = res["chunks"][str(cf)]
        r.update({"calls_per_utterance": args.frames // cf, "off_ms_per_call": off, "on_ms_per_call": on,
                  "on_minus_off_ms": float(np.mean(on) - np.mean(off)), "off_spread_ms": float(max(off) - min(off)),
                  "endpoints_read_ms": reads, "slots_by_rule_0123": fired,
                  "tokens_identical_on_off": bool(tokens[True] == tokens[False])})
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
