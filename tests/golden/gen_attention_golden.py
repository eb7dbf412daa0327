"""Generates tests/golden/attention_ref.npz: the reference's RelPositionMultiHeadedAttention (wenet/transformer/attention.py) with the
mask of subsequent_chunk_mask & ~make_pad_mask (wenet/utils/mask.py), forward and backward in float64 eval mode, on seeded cases.
Run where the read-only reference is present (the build container); never imported by tests, bench or the product.  Only data goes
into the fixture.

One state dict serves every case (keys sd.<parameter name>).  Its values and x are multiples of 1/128 and 1/16, so that they
compress: five full-entropy 256 x 256 float32 matrices alone would pass the fixture limit.  For the same reason each case holds
  out, dx                            float32 (the float64 results rounded once: 6e-8 relative, the test's bound is 1e-6 absolute)
  g.<bias or pos_bias name>          float64, whole
  g.<weight name>.rows               float64, rows 0, 96, 192 of the [256, 256] gradient
  g.<weight name>.rowsum / .colsum   float64, the sums over all columns / all rows: every element of the gradient enters both
  g.<weight name>.proj_r / .proj_l   float64, G r and l G for the seeded sign vectors proj.r, proj.l [256] (+-1): errors that cancel
                                     in a plain row or column sum do not cancel under random signs
per case c (keys c<i>.<name>), next to x, pos_emb, lengths, args = (chunk_size, num_left_chunks) and dout.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_loader import load_reference  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "attention_ref.npz")
ROWS = (0, 96, 192)
# (B, T, lengths, chunk_size, num_left_chunks): dead-like (rows without a visible key, a moving lower edge), c16-like (chunk edge =
# tile edge, a length inside a tile), causal-like (chunk 1)
CASES = ((3, 13, (13, 5, 1), 4, 1), (2, 35, (35, 20), 16, -1), (2, 9, (9, 9), 1, -1))


def main():
    load_reference()
    from wenet.transformer.attention import RelPositionMultiHeadedAttention
    from wenet.transformer.embedding import RelPositionalEncoding
    from wenet.utils.mask import make_pad_mask, subsequent_chunk_mask
    g = np.random.Generator(np.random.Philox(key=[2026, 0xA77]))
    ref = RelPositionMultiHeadedAttention(4, 256, 0.1).double().eval()
    sd = {}
    for name, t in ref.state_dict().items():
        span = 24 if name.startswith("pos_bias") else 8          # +-24/128 for the biases, +-8/128 = +-1/16 (torch's Linear range) otherwise
        sd[name] = (g.integers(-span, span + 1, tuple(t.shape)) / 128.0).astype(np.float32)
    ref.load_state_dict({n: torch.from_numpy(a).double() for n, a in sd.items()}, strict=True)
    pe = RelPositionalEncoding(256, 0.0).double().eval()
    fix = {f"sd.{n}": a for n, a in sd.items()}
    proj_r, proj_l = (g.integers(0, 2, 256) * 2.0 - 1.0 for _ in range(2))
    fix.update({"proj.r": proj_r.astype(np.float32), "proj.l": proj_l.astype(np.float32)})
    for ci, (B, T, lens, chunk, left) in enumerate(CASES):
        x32 = (g.integers(-16, 17, (B, T, 256)) / 16.0).astype(np.float32)
        dout32 = (g.integers(-32, 33, (B, T, 256)) / 256.0).astype(np.float32)
        pos_emb = pe.position_encoding(0, T).to(torch.float32)                  # [1, T, 256], rounded once: the module under test takes float32
        x = torch.from_numpy(x32).double().requires_grad_(True)
        lengths = torch.tensor(lens)
        mask = (~make_pad_mask(lengths, T)).unsqueeze(1) & subsequent_chunk_mask(T, chunk, left).unsqueeze(0)       # [B, T, T]
        ref.zero_grad()
        out, _ = ref(x, x, x, mask, pos_emb.double())
        (out * torch.from_numpy(dout32).double()).sum().backward()
        assert torch.isfinite(out).all() and all(torch.isfinite(p.grad).all() for p in ref.parameters()) and torch.isfinite(x.grad).all()
        c = f"c{ci}."
        fix.update({c + "x": x32, c + "pos_emb": pos_emb.numpy(), c + "lengths": np.array(lens, np.int32), c + "args": np.array([chunk, left], np.int32),
                    c + "dout": dout32, c + "out": out.detach().numpy().astype(np.float32), c + "dx": x.grad.numpy().astype(np.float32)})
        for name, p_ in ref.named_parameters():
            gr = p_.grad.numpy()
            if gr.shape == (256, 256):
                fix.update({f"{c}g.{name}.rows": gr[list(ROWS)].copy(), f"{c}g.{name}.rowsum": gr.sum(1), f"{c}g.{name}.colsum": gr.sum(0),
                            f"{c}g.{name}.proj_r": gr @ proj_r, f"{c}g.{name}.proj_l": proj_l @ gr})
            else:
                fix[f"{c}g.{name}"] = gr.copy()
    np.savez_compressed(OUT, **fix)
    print(f"wrote {OUT}: {len(CASES)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
