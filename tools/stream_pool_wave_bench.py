"""Audio in for the stream pool (rnnt_pool_wave, StreamPool.feed_wave), measured on one GPU in ONE process on seeded weights.
Prints one JSON line; --out writes it to a file as well.

  wave_<ms>ms     rnnt_pool_wave per call with --slots active rows of <ms> ms packets at 16 kHz (20 ms = 320 samples, 100 ms = 1600): the
                  median synchronised wall time of a call, and the summed time of an utterance over the frames it emitted
  fbank           the same waveforms through ONE whole-utterance rnnt_fbank call: the floor per frame
  step_<ms>ms     an utterance through StreamPool.feed_wave + step() per packet against the same pool fed, through feed() + step() per
                  chunk, the chunks sliced from rnnt_fbank of the whole waves: what the front-end adds to a live utterance, in total and
                  per chunk step (packet tensors are on the device already; the facade's row gathering is in the figure)

An utterance is --seconds of audio per slot.  A call's wall time ends synchronised; medians over --reps repetitions after one warm-up.

usage: python tools/stream_pool_wave_bench.py [--slots 64] [--seconds 4] [--packets-ms 20,100] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--packets-ms", default="20,100")
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.features import extract_audio_features
    from ctc_vr_amd.online_rnnt_model import StreamPool

    assert torch.cuda.is_available(), "stream_pool_wave_bench needs a GPU"
    N, C, rate, n_fft = args.slots, args.chunk, 16000, 1024
    n = int(args.seconds * rate)
    sizes = {int(ms): rate * int(ms) // 1000 for ms in args.packets_ms.split(",")}
    rng = np.random.default_rng(2026)
    w = 0.1 * rng.standard_normal((N, n)) + 0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / rate)[None, :]
    wave = torch.from_numpy(w.astype(np.float32)).cuda()
    n_frames = 1 + n // 512
    pool = StreamPool(T.make_state_dict(0), N, vocab_size=T.VOCAB, blank_id=T.BLANK, max_chunk_frames=64, max_cache_frames=512, max_tokens=8192,
                      sample_rate=rate, n_fft=n_fft, chunk_frames=C)
    eng = pool.engine
    s = torch.cuda.current_stream().cuda_stream
    slots = list(range(N))
    out = torch.empty(N, 8, 80, device="cuda")

    def walk_wave(size):
        """the utterances of all slots through rnnt_pool_wave in packets of `size` samples -> (per-call ms, frames emitted per slot)"""
        eng.stream_wave_reset(-1, s)
        ts, frames = [], 0
        for a in range(0, n, size):
            pk = wave[:, a:a + size].contiguous()
            k = pk.size(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = eng.pool_wave(slots, pk.data_ptr(), k, [k] * N, [a + size >= n] * N, out.data_ptr(), out.size(1), rate, n_fft, s)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            frames += int(got[0])
        assert frames == n_frames, (frames, n_frames)
        return ts

    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = extract_audio_features(eng, wave, rate, n_fft=n_fft, stream=s)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, f

    def utterance_wave(size):
        pool.reset()
        for _ in slots:
            pool.open()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, n, size):
            for b in slots:
                pool.feed_wave(b, wave[b, a:a + size], final=a + size >= n)
            pool.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def utterance_feed(feats):
        pool.reset()
        for _ in slots:
            pool.open()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a in range(0, n_frames, C):
            if min(C, n_frames - a) >= 7:
                for b in slots:
                    pool.feed(b, feats[b, a:a + C])
                pool.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    per_call = {ms: [] for ms in sizes}
    total = {ms: [] for ms in sizes}
    step_wave = {ms: [] for ms in sizes}
    floor, step_feed = [], []
    for rep in range(1 + args.reps):                                  # repetition 0 warms up
        for ms, size in sizes.items():
            ts = walk_wave(size)
            if rep:
                per_call[ms] += ts
                total[ms].append(sum(ts))
        t, feats = whole()
        tf = utterance_feed(feats)
        if rep:
            floor.append(t)
            step_feed.append(tf)
        for ms, size in sizes.items():
            tw = utterance_wave(size)
            if rep:
                step_wave[ms].append(tw)
    med = statistics.median
    n_steps = sum(1 for a in range(0, n_frames, C) if min(C, n_frames - a) >= 7)
    res = {"tool": "stream_pool_wave_bench", "device": torch.cuda.get_device_name(0), "slots": N, "seconds": args.seconds, "sample_rate": rate,
           "n_fft": n_fft, "frames_per_slot": n_frames, "chunk_frames": C, "reps": args.reps}
    for ms in sizes:
        res[f"wave_{ms}ms_call_ms"] = round(med(per_call[ms]), 4)
        res[f"wave_{ms}ms_us_per_frame"] = round(med(total[ms]) * 1e3 / (N * n_frames), 3)
    res["fbank_whole_ms"] = round(med(floor), 3)
    res["fbank_whole_us_per_frame"] = round(med(floor) * 1e3 / (N * n_frames), 3)
    res["utterance_feed_ms"] = round(med(step_feed), 1)
    for ms in sizes:
        res[f"utterance_feed_wave_{ms}ms_ms"] = round(med(step_wave[ms]), 1)
        res[f"front_end_adds_{ms}ms_ms_per_chunk_step"] = round((med(step_wave[ms]) - med(step_feed)) / n_steps, 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
