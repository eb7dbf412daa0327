"""The predictor's LSTM over a whole label sequence: what rnnt_lstm_forward and rnnt_lstm_backward cost against the step loop they
replace, against torch.nn.LSTM on the device, and against the weight stream a step cannot avoid.

Shapes: B 16 and 64 x U1 29 (the workload's label count), and B 2 x U1 256 (the per-step slope).  Seeded weights of
testing.make_state_dict(0), random tokens; x is their embedding, formed once outside the timed region.  Device-event times around whole
calls, host part included, over `--iters` calls after `--warmup` calls (median, min, max), legs alternating per repetition:
  * forward:       rnnt_lstm_forward with state_dev = NULL into a preallocated workspace (pack, xg GEMM, ONE recurrence launch);
  * forward_state: the same saving the gates and c for a backward;
  * backward:      rnnt_lstm_backward (ONE recurrence launch, the dx / dW GEMMs, the slab reduces);
  * step_loop:     the parent's only device path: U1 iterations of rnnt_predictor_step (two launches per label: the LSTM cell GEMM with the
                   embedding table folded in, and the projection) on a context with the same weights;
  * torch / torch_fwd_bwd: torch.nn.LSTM(256, 256, batch_first) forward, and forward + backward of out.sum(), when this torch build
                   runs it on the device (reported as unavailable otherwise).
Per step: forward median / U1, beside the floor of one pass over W_hh (1 MiB) per row tile at the 64 B / clock a CU's vector L1 takes
from L2 (153.6 GB/s at 2.4 GHz), and the stream rate the measured step implies.  No pass / fail number.
Needs a GPU: there is no CPU timing.  Writes one JSON document.

usage: python tools/predictor_grad_bench.py [--out profiles/predictor_grad_bench.json] [--iters 20] [--warmup 5] [--reps 3] [--no-torch]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L1_FILL_BPS = 64 * 2.4e9          # bytes per second one CU's vector L1 takes from L2
WHH_BYTES = 4 * 1024 * 256
SHAPES = [(16, 29), (64, 29), (2, 256)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.nn.LSTM legs out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_grad_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import ctc_vr_amd.lib as rlib
    import ctc_vr_amd.testing as T
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel

    assert torch.cuda.is_available(), "predictor_grad_bench needs a GPU: there is no CPU timing"
    sd = T.make_state_dict(0)
    model = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=T.BLANK, streaming=True, static_chunk_size=16, predictor_dropout=0)
    model.load_state_dict(sd)
    dev, eng = model.device, model._engine
    stream = torch.cuda.current_stream().cuda_stream
    w = {k: torch.from_numpy(sd["predictor.rnn." + k]).to(dev) for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")}
    embed = torch.from_numpy(sd["predictor.embed.weight"]).to(dev)
    ref = torch.nn.LSTM(256, 256, 1, batch_first=True).to(dev)
    ref.load_state_dict(w)
    doc = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "reps": args.reps, "l1_fill_bytes_per_s": L1_FILL_BPS, "shapes": []}
    for B, U1 in SHAPES:
        g = np.random.Generator(np.random.Philox(key=[B, U1]))
        tok = torch.from_numpy(g.integers(0, T.VOCAB, (B, U1)).astype(np.int32)).to(dev)
        tok_steps = [tok[:, u].contiguous() for u in range(U1)]
        x = embed[tok.long()].contiguous()
        dout = torch.from_numpy((0.05 * g.standard_normal((B, U1, 256))).astype(np.float32)).to(dev)
        wbytes, sbytes = rlib.lstm_workspace(B, U1)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        state = torch.empty(sbytes, dtype=torch.uint8, device=dev)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out, hn, cn = new(B, U1, 256), new(B, 256), new(B, 256)
        dx, dwi, dwh, db, dh0, dc0 = new(B, U1, 256), new(1024, 256), new(1024, 256), new(1024), new(B, 256), new(B, 256)
        hc = [new(B, 256) for _ in range(4)]
        hc_out = [new(B, 256) for _ in range(U1)]

        def forward(state_ptr=None):
            rlib.lstm_forward_device(x.data_ptr(), w["weight_ih_l0"].data_ptr(), w["weight_hh_l0"].data_ptr(), w["bias_ih_l0"].data_ptr(),
                                     w["bias_hh_l0"].data_ptr(), None, None, None, (B, U1), out.data_ptr(), hn.data_ptr(), cn.data_ptr(), state_ptr, sbytes,
                                     work.data_ptr(), wbytes, stream)

        def forward_state():
            forward(state.data_ptr())

        def backward():
            rlib.lstm_backward_device(x.data_ptr(), w["weight_ih_l0"].data_ptr(), w["weight_hh_l0"].data_ptr(), None, None, out.data_ptr(), state.data_ptr(),
                                      sbytes, dout.data_ptr(), None, (B, U1), dx.data_ptr(), dwi.data_ptr(), dwh.data_ptr(), db.data_ptr(), dh0.data_ptr(),
                                      dc0.data_ptr(), work.data_ptr(), wbytes, stream)

        def step_loop():
            hc[0].zero_(), hc[1].zero_()
            h, c, h2, c2 = hc
            for u in range(U1):
                eng.predictor_step(tok_steps[u].data_ptr(), h.data_ptr(), c.data_ptr(), B, hc_out[u].data_ptr(), h2.data_ptr(), c2.data_ptr(), stream)
                h, c, h2, c2 = h2, c2, h, c
            return h

        legs = {"forward": forward, "forward_state": forward_state, "backward": backward, "step_loop": step_loop}
        torch_note = "ran"
        try:
            if args.no_torch:
                raise RuntimeError("--no-torch")

            def torch_fwd():
                with torch.no_grad():
                    return ref(x)[0]

            def torch_fwd_bwd():
                xr = x.detach().requires_grad_(True)
                ref.zero_grad(set_to_none=True)
                ref(xr)[0].sum().backward()
                return xr.grad

            torch_fwd(), torch_fwd_bwd()
            torch.cuda.synchronize()
            legs["torch"], legs["torch_fwd_bwd"] = torch_fwd, torch_fwd_bwd
        except Exception as e:   # this torch build has no device LSTM
            torch_note = f"unavailable: {type(e).__name__}: {str(e)[:200]}"
        times = {k: [] for k in legs}
        forward_state()
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        # the three paths compute the same thing
        forward()
        h_last = step_loop()
        torch.cuda.synchronize()
        agree = {"hN_vs_step_loop": float((hn - h_last).abs().max())}
        if "torch" in legs:
            agree["out_vs_torch"] = float((out - legs["torch"]()).abs().max())
        for _ in range(args.reps):
            for k, fn in legs.items():
                if k == "backward":
                    forward_state()
                for _ in range(args.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1))
        row = {"B": B, "U1": U1, "row_tiles": -(-B // 4), "work_bytes": wbytes, "state_bytes": sbytes, "torch_lstm": torch_note, **agree}
        for k, v in times.items():
            row[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        row["forward_over_step_loop"] = row["forward_ms"]["median"] / row["step_loop_ms"]["median"]
        step_us = 1e3 * row["forward_ms"]["median"] / U1
        row["forward_us_per_step"] = step_us
        row["floor_us_per_step"] = 1e6 * WHH_BYTES / L1_FILL_BPS
        row["implied_stream_bytes_per_s"] = WHH_BYTES / (step_us * 1e-6)
        doc["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
