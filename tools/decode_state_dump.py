"""Tokens and predictor state after a whole-utterance decode of the bench workload, dumped as .npy for the build this runs on.

    python tools/decode_state_dump.py DIR [--batch 64] [--frames 1000] [--chunk 16] [--numerics bf16x3] [--blank-bias 12.0]

writes DIR/tokens.npy [B, max] (padded with -1), DIR/token_counts.npy [B], DIR/h.npy and DIR/c.npy [B, 256] float32 and
DIR/last_token.npy [B].  Two builds decode the same seeded inputs (bench.py's: weights seed 0 with its blank bias, fbank seed 1234, its headline numerics), so a change of the decoder
that claims the same bits is checked by dumping on both and comparing the files:

    python tools/decode_state_dump.py --compare DIR_A DIR_B

exits 0 iff every file is byte for byte the same."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FILES = ("tokens", "token_counts", "h", "c", "last_token")


def compare(a, b):
    bad = 0
    for f in FILES:
        x, y = np.load(os.path.join(a, f + ".npy")), np.load(os.path.join(b, f + ".npy"))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        print(f"{f}: {'identical' if same else 'DIFFERENT'} {x.shape} {x.dtype}")
        bad += not same
    return bad


def dump(out, batch, frames, chunk, numerics, blank_bias):
    import torch
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    sb = StreamingBatch(T.make_state_dict(0, blank_bias=blank_bias), batch, max_chunk_frames=max(24, chunk), max_cache_frames=frames // 4 + 8,
                        max_enc_frames=frames // 4 + 8, max_tokens=frames // 4 * 10 + 16, numerics=numerics)
    x = torch.from_numpy(T.synth_fbank(batch, frames, seed=1234)).cuda().contiguous()
    toks = sb.decode_script(x, chunk, pipelined=True)
    s = torch.cuda.current_stream().cuda_stream
    counts = np.asarray(sb.engine.token_counts(s), dtype=np.int64)
    tokens = np.full((batch, max(1, int(counts.max()))), -1, dtype=np.int64)
    for b, t in enumerate(toks):
        tokens[b, :len(t)] = t
    h, c, last = np.zeros((batch, 256), np.float32), np.zeros((batch, 256), np.float32), np.zeros(batch, np.int64)
    for b in range(batch):
        hb, cb, tb = sb.engine.predictor_state(b, s)
        h[b], c[b], last[b] = hb, cb, tb
    sb.engine.close()
    os.makedirs(out, exist_ok=True)
    for f, a in zip(FILES, (tokens, counts, h, c, last)):
        np.save(os.path.join(out, f + ".npy"), a)
    print(f"{out}: {int(counts.sum())} tokens over {batch} streams, most {int(counts.max())}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--numerics", default="bf16x3")
    ap.add_argument("--blank-bias", type=float, default=12.0)
    a = ap.parse_args()
    if a.compare:
        assert len(a.dirs) == 2, "--compare takes two directories"
        sys.exit(1 if compare(*a.dirs) else 0)
    dump(a.dirs[0], a.batch, a.frames, a.chunk, a.numerics, a.blank_bias)
