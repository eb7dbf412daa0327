"""What a segment boundary costs a stream pool on one GPU (bench.py's seeded weights; bf16x3 unless told otherwise), every comparison
inside ONE process.  Prints one JSON line; --out writes it to a file as well (profiles/stream_pool_segment_bench.json).

  the call: rnnt_pool_segment for 1 and for all slots, encoder kept and fresh, against the only way to start the next utterance
  before it, one rnnt_stream_open per slot.  The slots are greedy slots that keep their frames and detect their endpoint and have
  advanced by one chunk.  Per case: the host time to enqueue (the call does not synchronise) and the time until the device has
  finished, medians over --reps repetitions that alternate between the cases, and the launches of one call.

  the step: StreamPool.step() with every slot active on 16-frame chunks, three ways that alternate utterance by utterance -- slots
  opened with endpoint= only (what step() did before the feature), with on_endpoint="keep" and a rule that never fires (the cost of
  looking: one endpoints read per step), and with a rule that fires in every slot at every step (the read, one result per slot, one
  rnnt_pool_segment call).  Mean ms per step after one warm-up utterance of each kind.

usage: python tools/stream_pool_segment_bench.py [--slots 64] [--reps 20] [--steps 20] [--numerics bf16x3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20, help="repetitions of every case of the call comparison")
    ap.add_argument("--steps", type=int, default=20, help="steps per utterance of the step comparison")
    ap.add_argument("--utterances", type=int, default=3, help="utterances of every kind of the step comparison")
    ap.add_argument("--numerics", default="bf16x3", choices=["fp32", "bf16x3", "f16x3", "bf16"])
    ap.add_argument("--blank-bias", type=float, default=12.0, help="as bench.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.lib import RnntEngine
    from ctc_vr_amd.online_rnnt_model import EndpointConfig, StreamPool

    B, CF = args.slots, 16
    sd = T.make_state_dict(0, blank_bias=args.blank_bias)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(T.synth_fbank(B, CF * args.steps, seed=5)).cuda()
    res = {"tool": "stream_pool_segment_bench", "numerics": args.numerics, "slots": B, "reps": args.reps, "steps": args.steps,
           "device": torch.cuda.get_device_name(0), "call": {}, "step": {}}

    # ---- the call ----------------------------------------------------------------------------------------------------------------
    eng = RnntEngine(max_streams=B, max_chunk_frames=CF, max_cache_frames=64, max_enc_frames=16, max_tokens=4096)
    eng.load_state_dict(sd, numerics=args.numerics)
    slots = list(range(B))
    x0 = x[:, :CF].contiguous()

    def prepare():
        eng.reset(B, s)
        for b in slots:
            eng.stream_open(b, s)
            eng.stream_keep_frames(b, True, s)
            eng.stream_endpoint(b, (0.5, 1, 0, 0, 500), s)
        eng.pool_chunk(slots, x0.data_ptr(), CF, [0] * B, [0] * B, True, s)
        torch.cuda.synchronize()

    def open_all():
        for b in slots:
            eng.stream_open(b, s)

    cases = {"segment_keep_1": lambda: eng.pool_segment([0], True, s), f"segment_keep_{B}": lambda: eng.pool_segment(slots, True, s),
             "segment_fresh_1": lambda: eng.pool_segment([0], False, s), f"segment_fresh_{B}": lambda: eng.pool_segment(slots, False, s),
             f"stream_open_x{B}": open_all}
    times = {k: ([], []) for k in cases}
    for rep in range(args.reps + 2):                         # two warm-up rounds
        for name, call in cases.items():
            prepare()
            l0 = eng.counters()[0]
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rep >= 2:
                times[name][0].append((t1 - t0) * 1e3)
                times[name][1].append((t2 - t0) * 1e3)
            res["call"].setdefault(name, {})["launches"] = eng.counters()[0] - l0
    for name, (host, done) in times.items():
        res["call"][name].update({"host_ms_median": float(np.median(host)), "done_ms_median": float(np.median(done)),
                                  "done_ms_min": float(np.min(done)), "done_ms_max": float(np.max(done))})
    eng.close()

    # ---- the step ----------------------------------------------------------------------------------------------------------------
    pool = StreamPool(sd, B, max_chunk_frames=CF, max_cache_frames=CF * args.steps // 4 + 64, max_tokens=4096, numerics=args.numerics)
    never, always = EndpointConfig(0.5, 0, 0, 0), EndpointConfig(0.5, 0, 0, 3 * 40)      # no rule at all / rule 3 at 3 frames: every step
    kinds = {"endpoint_only": (never, None), "on_endpoint_idle": (never, "keep"), "on_endpoint_firing": (always, "keep")}

    def utterance(kind):
        cfg, on = kinds[kind]
        pool.reset()
        for _ in range(B):
            pool.open(endpoint=cfg, on_endpoint=on)
        torch.cuda.synchronize()
        ms, segs = [], 0
        for c in range(args.steps):
            for b in range(B):
                pool.feed(b, x[b, c * CF:(c + 1) * CF])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pool.step()                                      # synchronises (the token read of the last slot, or the last result)
            ms.append((time.perf_counter() - t0) * 1e3)
            segs += sum(len(pool.segments(b)) for b in range(B))
        return float(np.mean(ms)), segs

    for kind in kinds:
        utterance(kind)                                      # warm-up
    per = {k: [] for k in kinds}
    for _ in range(args.utterances):
        for kind in kinds:
            ms, segs = utterance(kind)
            per[kind].append(ms)
            res["step"].setdefault(kind, {})["segments_per_utterance"] = segs
    for kind in kinds:
        res["step"][kind]["ms_per_step"] = per[kind]
    base = float(np.mean(per["endpoint_only"]))
    res["step"]["idle_minus_off_ms"] = float(np.mean(per["on_endpoint_idle"])) - base
    res["step"]["firing_minus_off_ms"] = float(np.mean(per["on_endpoint_firing"])) - base
    res["step"]["off_spread_ms"] = float(max(per["endpoint_only"]) - min(per["endpoint_only"]))
    pool.engine.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
