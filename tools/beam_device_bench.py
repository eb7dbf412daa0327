"""BASELINE configs[2] beam leg (64 streams x 1000 fbank frames, chunk 16, beam 4, bench.py's seeded weights and inputs): the
host-merge path (beam_script(pipelined=True): one rnnt_encoder_chunks call + rnnt_beam_advance, a host round trip per encoder
frame) against the device-resident path (the same with device_merge=True: rnnt_beam_decode), timed in the same process,
alternating, device-synchronised after warm-up; the hypotheses must be identical.  Then the ragged batch of 64 distinct lengths
(40 .. 1000 frames): beam_script_ragged (one rnnt_encode_ragged + one rnnt_beam_decode) against the length-class loop (one
whole-utterance call per length).  Prints one JSON line.

usage: python tools/beam_device_bench.py [--steps 5] [--warmup 1] [--numerics bf16x3] [--no-ragged]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--blank-bias", type=float, default=12.0, help="as bench.py")
    ap.add_argument("--no-ragged", action="store_true", help="skip the ragged-batch comparison")
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_model import StreamingBatch

    sub_len = lambda t: ((t - 3) // 2 + 1 - 3) // 2 + 1
    B, cf, beam = args.batch, args.chunk, args.beam
    sd = T.make_state_dict(0, blank_bias=args.blank_bias)
    plan = T.chunk_plan(args.frames, cf)
    ef = sum(sub_len(b - a) for a, b in plan)
    x = torch.from_numpy(T.synth_fbank(B, args.frames, seed=1234)).cuda().contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.set_stream(side)
    sb = StreamingBatch(sd, B, max_chunk_frames=max(b - a for a, b in plan), max_cache_frames=ef + 8, max_enc_frames=ef + 8, max_tokens=16,
                        max_beam=beam, numerics=args.numerics)
    sig = lambda beams: [[(tuple(h.tokens), h.log_prob) for h in bm] for bm in beams]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    host = lambda: sb.beam_script(x, cf, beam, pipelined=True)
    dev = lambda: sb.beam_script(x, cf, beam, pipelined=True, device_merge=True)
    plan7 = [(a, b) for a, b in plan if b - a >= 7]
    offs = [sum((b - a) // 4 for a, b in plan7[:i]) for i in range(len(plan7))]
    s = torch.cuda.current_stream().cuda_stream

    def enc():
        sb.reset()
        sb.engine.encoder_chunks(x.data_ptr(), x.size(1), [a for a, _ in plan7], [b - a for a, b in plan7], offs, offs, s, greedy=False)
    for _ in range(args.warmup):
        host(); dev(); enc()
    th, td, te = [], [], []
    identical = True
    for _ in range(args.steps):
        ms, bh = timed(host)
        th.append(ms)
        ms, bd = timed(dev)
        td.append(ms)
        identical = identical and sig(bh) == sig(bd)
        te.append(timed(enc)[0])
    med = lambda v: float(np.median(v))
    l0, _ = sb.engine.counters()
    dev()
    l1, _ = sb.engine.counters()
    res = {"workload": f"configs[2]: {B} x {args.frames} frames, chunk {cf}, beam {beam}, {args.numerics}", "enc_frames": ef,
           "host_merge_ms": round(med(th), 3), "device_merge_ms": round(med(td), 3), "encoder_only_ms": round(med(te), 3),
           "speedup": round(med(th) / med(td), 2), "hyps_identical": identical,
           "beam_part_ms": {"host_merge": round(med(th) - med(te), 3), "device_merge": round(med(td) - med(te), 3)},
           "launches_per_call_device": l1 - l0, "host_ms_all": [round(v, 3) for v in th], "device_ms_all": [round(v, 3) for v in td]}

    if not args.no_ragged:
        n = 64
        rng = np.random.default_rng(5)
        lens = sorted(rng.choice(np.arange(40, 1001), size=n, replace=False).tolist(), reverse=True)
        lens[0], lens[-1] = 1000, 40
        perm = rng.permutation(n)
        lens = [lens[i] for i in perm]
        full = torch.from_numpy(T.synth_fbank(n, 1000, seed=4321))
        xr = torch.zeros(n, 1000, 80)
        for b in range(n):
            xr[b, :lens[b]] = full[b, :lens[b]]
        xr = xr.cuda().contiguous()
        sr = StreamingBatch(sd, n, max_chunk_frames=48, max_cache_frames=256, max_enc_frames=256, max_tokens=16, max_beam=beam, numerics=args.numerics)

        def classes():
            out = [None] * n
            for T_ in sorted(set(lens), reverse=True):
                idx = [b for b in range(n) if lens[b] == T_]
                sr.n = len(idx)
                try:
                    bm = sr.beam_script(xr[torch.tensor(idx, device=xr.device), :T_].contiguous(), cf, beam, pipelined=True, device_merge=True)
                finally:
                    sr.n = n
                for b, h in zip(idx, bm):
                    out[b] = h
            return out
        ragged = lambda: sr.beam_script_ragged(xr, torch.tensor(lens), cf, beam)
        ragged(); classes()
        tr, tc = [], []
        same = True
        for _ in range(max(1, args.steps // 2)):
            ms, a = timed(ragged)
            tr.append(ms)
            ms, c = timed(classes)
            tc.append(ms)
            same = same and [[tuple(h.tokens) for h in bm] for bm in a] == [[tuple(h.tokens) for h in bm] for bm in c]
        res["ragged64"] = {"one_call_ms": round(med(tr), 3), "length_classes_ms": round(med(tc), 3), "speedup": round(med(tc) / med(tr), 2),
                           "tokens_identical": same}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
