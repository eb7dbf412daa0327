"""Decoder and joint kernels at the edges of the model's configuration space: vocabulary sizes on both sides of every code-path
boundary (greedy_multi's four parts of ceil(V / 4) rows, the joint rows kernel's 26 vocabulary tiles, the beam chain's 512), blank
first / inside / last, symbol rates from almost no symbol per frame to the n_steps cap on every frame, lattices large enough for
the joint kernel's persistent row-tile queue, and exact argmax ties.  Everything runs through the C ABI (RnntEngine /
StreamingBatch) and is checked against the CPU oracle (oracle/rnnt_oracle.py) or its formulas in float64.  Needs a real MI355X.

Symbol-rate regimes are realised by (seed, blank_bias) and asserted from the oracle's per-frame symbol counts, and every greedy
comparison first asserts that the oracle's smallest top-2 logit margin is >= MARGIN, so a token flip is a bug, not a near-tie."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3
MARGIN = 1e-3
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
N_STEPS = 10
CHUNK = 16
FRAMES = 200                      # fbank frames per utterance: 12 chunks (the last one 24 frames), 38 encoder frames
ENC_SEED = 0                      # weights seed: the encoder weights (and so the oracle's encoder frames) do not depend on V / blank
RAGGED_LENS = [200, 160, 112]     # chunk plans that are prefixes of the 200-frame plan: 38, 30, 21 encoder frames

KERNEL_W = (11.0, 4.0)           # (blank_bias, out_gain) of the kernel-level tests: make_state_dict's defaults
JOINT_W = (0.0, 1.0)             # logits of order 1 for the lattice tests: a padded column that leaks into the log-sum-exp shows
# (V, blank) -> {regime: (blank_bias, out_gain)}; with weights seed ENC_SEED and the inputs of _inputs() the oracle gives the regime below
# (asserted by _assert_regime) and a smallest top-2 margin >= MARGIN
CONFIGS = {
    (412, 0): {"sparse": (6.0, 8.0), "mixed": (0.0, 8.0), "saturated": (-8.0, 8.0)},
    (412, 411): {"sparse": (14.0, 4.0), "mixed": (10.5, 4.0), "saturated": (-8.0, 4.0)},
    (416, 5): {"sparse": (14.0, 4.0), "mixed": (7.0, 4.0), "saturated": (-8.0, 4.0)},
    (512, 0): {"sparse": (4.0, 4.0), "mixed": (1.0, 4.0), "saturated": (-6.0, 4.0)},
    (513, 0): {"sparse": (4.0, 4.0), "mixed": (1.0, 4.0), "saturated": (-6.0, 4.0)},
    (129, 128): {"sparse": (16.0, 4.0), "mixed": (12.0, 4.0), "saturated": (-24.0, 6.0)},
    (6, 0): {"sparse": (-3.0, 4.0), "mixed": (-8.0, 4.0), "saturated": (-14.0, 4.0)},
    (4336, 0): {"sparse": (12.0, 8.0), "mixed": (2.0, 8.0), "saturated": (-24.0, 8.0)},
    (64, 0): {"sparse": (1.0, 4.0), "mixed": (-2.0, 4.0), "saturated": (-30.0, 4.0)},
}
GREEDY_CONFIGS = [(412, 0), (412, 411), (416, 5), (512, 0), (513, 0), (129, 128), (6, 0), (4336, 0)]


@pytest.fixture(params=PARITY_MODES)
def numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    return request.param


_SD = {}


def _sd(V, blank, w=KERNEL_W, seed=ENC_SEED, twins=()):
    """seeded weights; w = (blank_bias, out_gain); twins: (a, b, heads) -> row (and bias) a of every head copied to b"""
    key = (V, blank, w, seed, tuple(twins))
    if key not in _SD:
        sd = T.make_state_dict(seed, vocab=V, blank=blank, blank_bias=w[0], out_gain=w[1])
        for a, b, heads in twins:
            for w in heads:
                sd[w + ".weight"][b] = sd[w + ".weight"][a]
                if w + ".bias" in sd:
                    sd[w + ".bias"][b] = sd[w + ".bias"][a]
        _SD[key] = sd
    return _SD[key]


def _inputs(n=3, frames=FRAMES):
    return torch.from_numpy(T.synth_fbank(3, FRAMES, seed=11))[:n, :frames]


def _enc_len(frames):
    return sum(((b - a - 3) // 2 + 1 - 3) // 2 + 1 for a, b in T.chunk_plan(frames, CHUNK) if b - a >= 7)


_ENC = {}


def _oracle_enc(b):
    """the oracle's encoder frames of input stream b (chunk loop of decode_script_greedy), [1, 38, 256]"""
    if b not in _ENC:
        from oracle import rnnt_oracle as O
        sd = O.to_torch_sd(T.make_state_dict(ENC_SEED))
        x = _inputs()[b:b + 1]
        st = O.OracleStream(sd, 0, CHUNK)
        outs, off = [], 0
        for a, e in T.chunk_plan(FRAMES, CHUNK):
            if e - a < 7:
                continue
            y, st.att_cache, st.cnn_cache = O.forward_chunk(sd, x[:, a:e], off, off, st.att_cache, st.cnn_cache)
            off += (e - a) // 4
            outs.append(y)
        _ENC[b] = torch.cat(outs, 1)
        assert _ENC[b].shape[1] == _enc_len(FRAMES)
    return _ENC[b]


_GREEDY = {}


def _oracle_greedy(V, blank, w, twins=()):
    """O.greedy_frames frame by frame on the oracle's encoder frames of the three inputs -> per stream the list of per-frame token
    lists, and the smallest top-2 margin of all decisions.  With twins (a, b) the reference decision on a tie is torch.argmax's
    first index, a; the oracle's float32 CPU GEMM does not promise bit-equal twin columns, so the oracle runs with b's output bias
    lowered by 1e4 (b is never best): the tokens the tie rule gives, and as margin the one between the best logit and the best
    one outside the pair."""
    key = (V, blank, w, tuple(twins))
    if key not in _GREEDY:
        from oracle import rnnt_oracle as O
        sd = O.to_torch_sd(_sd(V, blank, w, twins=twins))
        if twins:
            sd = dict(sd)
            sd["joint.ffn_out.bias"] = sd["joint.ffn_out.bias"].clone()
            for a, b, _ in twins:
                sd["joint.ffn_out.bias"][b] -= 1e4
        per, margins = [], []
        for s in range(3):
            enc = _oracle_enc(s)
            frames, st, tok = [], None, blank
            for t in range(enc.size(1)):
                hyp, st, tok = O.greedy_frames(sd, enc[:, t:t + 1], st, tok, blank, N_STEPS, margins=margins)
                frames.append(hyp)
            per.append(frames)
        _GREEDY[key] = (per, min(margins))
    return _GREEDY[key]


def _tokens(frames, n_frames=None):
    return [t for f in frames[:n_frames] for t in f]


def _assert_regime(per, regime):
    counts = np.array([len(f) for frames in per for f in frames])
    empty, cap = float(np.mean(counts == 0)), float(np.mean(counts == N_STEPS))
    if regime == "sparse":
        assert empty >= 0.8 and counts.sum() > 0, (empty, cap)
    elif regime == "mixed":
        assert empty >= 0.2 and cap >= 0.2, (empty, cap)
    else:
        assert cap >= 0.8, (empty, cap)
    assert len({len(_tokens(f)) for f in per}) > 1 or regime != "mixed"     # the streams diverge in symbol count


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


# ---- A. joint lattice ----------------------------------------------------------------------------------------------------------

_ENG = {}


def _engine(V, blank, numerics, w=KERNEL_W, max_streams=16, max_cache=256, twins=(), max_beam=0, tag=None):
    """tag: names the per-context knobs the caller has put into the environment (a context reads them at rnnt_create)"""
    from ctc_vr_amd.lib import RnntEngine
    key = (V, blank, numerics, w, max_streams, max_cache, tuple(twins), max_beam, tag)
    if key not in _ENG:
        e = RnntEngine(max_streams=max_streams, max_chunk_frames=32, max_cache_frames=max_cache, max_enc_frames=64, vocab_size=V,
                       blank_id=blank, max_beam=max_beam)
        e.load_state_dict(_sd(V, blank, w, twins=twins), numerics=numerics)
        _ENG[key] = e
    return _ENG[key]


def _w64(sd, *names):
    return [torch.from_numpy(sd[n]).cuda().double() for n in names]


def _joint64(sd, enc, prd):
    """TransducerJoint.forward (oracle.joint) in float64 on the device: [B, T, U, V] logits"""
    we, be, wp, bp, wo, bo = _w64(sd, "joint.enc_ffn.weight", "joint.enc_ffn.bias", "joint.pred_ffn.weight", "joint.pred_ffn.bias",
                                  "joint.ffn_out.weight", "joint.ffn_out.bias")
    e = enc.double() @ we.T + be
    p = prd.double() @ wp.T + bp
    return torch.tanh(e[:, :, None, :] + p[:, None, :, :]) @ wo.T + bo


SENTINEL = 1234.5


def _out_buffer(n, tail=1024):
    buf = torch.full((n + tail,), float("nan"), device="cuda")
    buf[n:] = SENTINEL
    return buf


def _check_out(buf, n, ref, tol=LOGIT_TOL):
    out = buf[:n].view(ref.shape)
    assert bool(torch.isfinite(out).all()), int((~torch.isfinite(out)).sum())
    assert bool((buf[n:] == SENTINEL).all())                                       # nothing written behind the output
    assert maxdiff(out, ref) < tol, maxdiff(out, ref)
    top = ref.topk(2, dim=-1).values
    clear = (top[..., 0] - top[..., 1]) > 2 * tol
    assert clear.float().mean() > 0.5
    assert torch.equal(out.argmax(-1)[clear], ref.argmax(-1)[clear])
    return out


def _run_joint(V, blank, numerics, shape, seed, tag=None):
    """-> the [B, T, U, V] outputs of mode 0 and mode 1"""
    B, Tn, U = shape
    eng = _engine(V, blank, numerics, w=JOINT_W, max_cache=max(256, -(-B * (Tn + U) * 256 // 6144)), tag=tag)   # rnnt_joint's scratch: 12 x 4 x 128 floats per cache frame
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, Tn, 256, generator=g).cuda()
    prd = (torch.randn(B, U, 256, generator=g) * 0.5).cuda()
    ref = _joint64(_sd(V, blank, JOINT_W), enc, prd)
    s = torch.cuda.current_stream().cuda_stream
    n = B * Tn * U * V
    outs = []
    for mode, want in ((0, ref), (1, torch.log_softmax(ref, dim=-1))):
        buf = _out_buffer(n)
        eng.joint(enc.data_ptr(), prd.data_ptr(), B, Tn, U, mode, buf.data_ptr(), s)
        torch.cuda.synchronize()
        out = _check_out(buf, n, want)
        again = _out_buffer(n)
        eng.joint(enc.data_ptr(), prd.data_ptr(), B, Tn, U, mode, again.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(again[:n].view(out.shape), out)                         # the tile queue hands out tiles in another order
        outs.append(out.clone())
    return outs


def _multi_tile_shapes():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    f = max(1.0, ncu / 256)
    return [(8, int(160 * f), 28), (16, int(250 * f), 32), (4, int(250 * f), 33)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_joint_lattice_multi_tile(which, numerics):
    """Lattices of more 64-row tiles than the persistent grid has workgroups (2 per CU): in the split modes every workgroup of
    joint_lattice_rows takes further tiles from the queue (jr_queue_pop, the nxt_lds ping-pong, the W_out DMA ring across tiles).
    ~560 and ~2000 tiles on 256 CUs, and 516 tiles whose last one is partial (33000 rows)."""
    shape = _multi_tile_shapes()[which]
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = shape[0] * shape[1] * shape[2]
    assert (rows + 63) // 64 > 2 * ncu, (shape, ncu)
    if which == 2:
        assert rows % 64 != 0
    _run_joint(412, 5, numerics, shape, 7 + which)


@pytest.mark.parametrize("V", [412, 416, 404, 8, 413, 600, 4336])
def test_joint_lattice_vocab(V, numerics):
    """V = 412, 416 (whole last tile), 404 (partial last tile: padded columns carry a -inf bias) and 8 take the rows kernel in the
    split modes; V = 413 (V % 4 != 0), 600 and 4336 take the gemm_ns + log_softmax_rows fallback, as does every V in fp32."""
    _run_joint(V, 0, numerics, (3, 37, 11), V)


def test_joint_lattice_prefetch_depth_one(monkeypatch):
    """exact-f32 joint lattice (gemm_ns with the tanh operand, 1221 rows: 19 full 64-row tiles and one of 5) in a context created under
    RNNT_GEMM_PD=1: within LOGIT_TOL of float64 like the default depth, and the form log names the launch ...;pd1) -- the default
    context logs the plain name.  Printed: whether the two depths give the same bits."""
    monkeypatch.setenv("RNNT_NUMERICS", "fp32")
    logs, outs = {}, {}
    for tag, pd in (("pd2", None), ("pd1", "1")):
        monkeypatch.delenv("RNNT_GEMM_PD", raising=False)
        if pd:
            monkeypatch.setenv("RNNT_GEMM_PD", pd)
        eng = _engine(412, 0, "fp32", w=JOINT_W, max_cache=256, tag=tag)
        eng.form_log_begin()
        outs[tag] = _run_joint(412, 0, "fp32", (3, 37, 11), 412, tag=tag)
        logs[tag] = eng.form_log_end()
    print(f"joint lattice: depth 2 {logs['pd2']}; depth 1 {logs['pd1']}; bit-identical: {[torch.equal(a, b) for a, b in zip(outs['pd1'], outs['pd2'])]}")
    assert "gemm_ns(joint lattice;pd1)" in logs["pd1"] and "gemm_ns(joint lattice)" not in logs["pd1"]
    assert "gemm_ns(joint lattice)" in logs["pd2"] and "gemm_ns(joint lattice;pd1)" not in logs["pd2"]


# ---- B. predictor step ---------------------------------------------------------------------------------------------------------

def _lstm64(sd, tok, h, c):
    emb, wih, whh, bih, bhh, wpr, bpr = _w64(sd, "predictor.embed.weight", "predictor.rnn.weight_ih_l0", "predictor.rnn.weight_hh_l0",
                                             "predictor.rnn.bias_ih_l0", "predictor.rnn.bias_hh_l0", "predictor.projection.weight",
                                             "predictor.projection.bias")
    g = emb[tok.long()] @ wih.T + bih + h.double() @ whh.T + bhh
    i, f, gg, o = g.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c.double() + torch.sigmoid(i) * torch.tanh(gg)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2 @ wpr.T + bpr, h2, c2


@pytest.mark.parametrize("V", [412, 4336])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096])
def test_predictor_step_rows(rows, V, numerics):
    """rnnt_predictor_step (EPI_LSTM GEMM + projection) at row counts around the GEMM tile, tokens over the whole vocabulary
    (0, blank and V - 1 included), h ~ N(0, 1), c ~ N(0, 3^2): out / h / c within 1e-4 of a float64 LSTM step, nothing written
    behind the outputs, the inputs untouched."""
    blank = 5 if V == 412 else 0
    eng = _engine(V, blank, numerics)
    g = torch.Generator().manual_seed(rows * 7 + V)
    tok = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    special = [0, blank, V - 1][:rows]
    tok[:len(special)] = torch.tensor(special, dtype=torch.int32)
    tok = tok.cuda()
    h = torch.randn(rows, 256, generator=g).cuda()
    c = (torch.randn(rows, 256, generator=g) * 3).cuda()
    h0, c0 = h.clone(), c.clone()
    outs = [torch.full((rows + 2, 256), SENTINEL, device="cuda") for _ in range(3)]
    s = torch.cuda.current_stream().cuda_stream
    eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), rows, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), s)
    torch.cuda.synchronize()
    want = _lstm64(_sd(V, blank), tok, h, c)
    for o, w in zip(outs, want):
        assert maxdiff(o[:rows], w) < 1e-4, maxdiff(o[:rows], w)
        assert bool((o[rows:] == SENTINEL).all())
    assert torch.equal(h, h0) and torch.equal(c, c0)


# ---- C. CTC log-probs ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [6, 412, 413, 4336])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_ctc_logprobs(rows, V, numerics):
    """rnnt_ctc_logprobs = log_softmax(ctc_lo(enc)) within LOGIT_TOL of float64, every element written, nothing behind."""
    eng = _engine(V, 0, numerics)
    enc = torch.randn(rows, 256, generator=torch.Generator().manual_seed(rows + V)).cuda()
    w, b = _w64(_sd(V, 0), "ctc_head.ctc_lo.weight", "ctc_head.ctc_lo.bias")
    ref = torch.log_softmax(enc.double() @ w.T + b, dim=-1)
    n = rows * V
    buf = _out_buffer(n)
    eng.ctc_logprobs(enc.data_ptr(), rows, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check_out(buf, n, ref)


# ---- D. greedy decode ----------------------------------------------------------------------------------------------------------

def _decode_all(V, blank, w, entries=("per_chunk", "whole", "ragged"), numerics="fp32", twins=()):
    """HIP tokens of the three inputs through each entry point -> {entry: [tokens per stream]}"""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    x = _inputs().cuda().contiguous()
    sb = StreamingBatch(_sd(V, blank, w, twins=twins), 3, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128,
                        max_enc_frames=64, max_tokens=512, numerics=numerics)
    got = {}
    for entry in entries:
        if entry == "per_chunk":
            got[entry] = sb.decode_script(x, CHUNK, per_chunk_decode=True)
        elif entry == "whole":
            got[entry] = sb.decode_script(x, CHUNK, pipelined=True)
        else:
            got[entry] = sb.decode_script_ragged(x, torch.tensor(RAGGED_LENS), CHUNK)
    return got


def _check_greedy(V, blank, regime, entries, numerics="fp32"):
    w = CONFIGS[(V, blank)][regime]
    per, margin = _oracle_greedy(V, blank, w)
    _assert_regime(per, regime)
    assert margin >= MARGIN, margin
    got = _decode_all(V, blank, w, entries, numerics)
    for entry, toks in got.items():
        for s in range(3):
            n = _enc_len(RAGGED_LENS[s]) if entry == "ragged" else None
            assert toks[s] == _tokens(per[s], n), (entry, s, len(toks[s]), len(_tokens(per[s], n)))
    return per


@pytest.mark.parametrize("regime", ["sparse", "mixed", "saturated"])
@pytest.mark.parametrize("cfg", GREEDY_CONFIGS, ids=lambda c: f"V{c[0]}_blank{c[1]}")
def test_greedy_decode_grid(cfg, regime):
    """Default decoder path, fp32: per-chunk, whole-utterance and ragged calls on three streams equal the oracle exactly, for
    every (vocabulary, blank) configuration in every symbol-rate regime.  V = 512 is greedy_multi's largest size (128 rows per
    part), 513 takes greedy_stream, 129 leaves the last part ragged, 6 leaves it empty, 4336 is the reference's default."""
    _check_greedy(cfg[0], cfg[1], regime, ("per_chunk", "whole", "ragged"))


PATHS = {"bf16x3": {}, "f16x3": {}, "dec_multi0": {"RNNT_DEC_MULTI": "0"}, "persistent0": {"RNNT_PERSISTENT": "0"}}


@pytest.mark.parametrize("regime", ["mixed", "saturated"])
@pytest.mark.parametrize("cfg", [(6, 0), (129, 128), (512, 0), (513, 0), (4336, 0)], ids=lambda c: f"V{c[0]}_blank{c[1]}")
@pytest.mark.parametrize("path", list(PATHS))
def test_greedy_decode_paths(path, cfg, regime, monkeypatch):
    """The split numerics modes and the alternative decoders (greedy_stream for every V, the launched evaluation
    batches) on the configurations at greedy_multi's boundaries, at the high symbol rates where multi-frame
    speculation is redone and the n_steps cap carries token and state across frames."""
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    numerics = path if path in PARITY_MODES else "fp32"
    entries = ("per_chunk", "whole") if path == "persistent0" else ("per_chunk", "whole", "ragged")
    _check_greedy(cfg[0], cfg[1], regime, entries, numerics)


# per-context step budgets of the graph decoder (RNNT_PERSISTENT=0): id -> knobs beside RNNT_PERSISTENT=0.  RNNT_DEC_SLACK is read by the
# wavefront's per-stage decode batches (RNNT_LM=0), RNNT_DRAIN_STEPS by greedy_drain behind either schedule.
BUDGETS = {
    "wavefront-slack0": {"RNNT_LM": "0", "RNNT_DEC_SLACK": "0"}, "wavefront-slack3": {"RNNT_LM": "0", "RNNT_DEC_SLACK": "3"},
    "wavefront-drain1": {"RNNT_LM": "0", "RNNT_DRAIN_STEPS": "1"}, "wavefront-drain7": {"RNNT_LM": "0", "RNNT_DRAIN_STEPS": "7"},
    "layer-major-drain1": {"RNNT_DRAIN_STEPS": "1"}, "layer-major-drain7": {"RNNT_DRAIN_STEPS": "7"},
    # RNNT_NO_GRAPH=1: the same step batches enqueued launch by launch instead of as captured graphs
    "wavefront-nograph": {"RNNT_LM": "0", "RNNT_NO_GRAPH": "1"}, "layer-major-nograph": {"RNNT_NO_GRAPH": "1"},
}
_BUDGET = {}


def _graph_decode(knobs, monkeypatch):
    """the three 200-frame inputs through rnnt_encoder_chunks with greedy decoding in a context created under RNNT_PERSISTENT=0 and
    `knobs` (every other budget knob unset) -> tokens per stream, token counts, (h, c, last token) per stream, the call's (launches,
    evaluation steps enqueued)"""
    key = tuple(sorted(knobs.items()))
    if key not in _BUDGET:
        from ctc_vr_amd.online_rnnt_model import StreamingBatch
        for k in ("RNNT_LM", "RNNT_DEC_SLACK", "RNNT_DRAIN_STEPS", "RNNT_NO_GRAPH"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("RNNT_PERSISTENT", "0")
        monkeypatch.setenv("RNNT_NUMERICS", "fp32")
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        V, blank = 412, 0
        sb = StreamingBatch(_sd(V, blank, CONFIGS[(V, blank)]["mixed"]), 3, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128,
                            max_enc_frames=64, max_tokens=512, numerics="fp32")
        c0 = sb.engine.counters()
        toks = sb.decode_script(_inputs().cuda().contiguous(), CHUNK, pipelined=True)
        s = torch.cuda.current_stream().cuda_stream
        _BUDGET[key] = (toks, sb.engine.token_counts(s).tolist(), [sb.engine.predictor_state(b, s) for b in range(3)],
                        tuple(a - b for a, b in zip(sb.engine.counters(), c0)))
        sb.engine.close()
    return _BUDGET[key]


@pytest.mark.parametrize("budget", list(BUDGETS))
def test_graph_decoder_step_budget(budget, monkeypatch):
    """RNNT_DEC_SLACK in {0, 3} and RNNT_DRAIN_STEPS in {1, 7} change how many evaluation steps the graph decoder enqueues per
    wavefront stage and per drain round, RNNT_NO_GRAPH=1 how a batch of steps is enqueued, never what a step computes: tokens, counts and the predictor's (h, c, last token) are
    bit-identical to the same context with the default budgets (8 and 4), whose tokens are the oracle's; the context's launch and
    step counters show that the budget did change"""
    knobs = BUDGETS[budget]
    base = {k: v for k, v in knobs.items() if k == "RNNT_LM"}
    want, got = _graph_decode(base, monkeypatch), _graph_decode(knobs, monkeypatch)
    per, margin = _oracle_greedy(412, 0, CONFIGS[(412, 0)]["mixed"])
    assert margin >= MARGIN, margin
    assert want[0] == [_tokens(per[s]) for s in range(3)]
    print(f"{budget}: (launches, steps enqueued) {got[3]} against {want[3]} with the default budgets; tokens per stream {got[1]}")
    assert got[0] == want[0] and got[1] == want[1]
    for b in range(3):
        assert np.array_equal(got[2][b][0], want[2][b][0]) and np.array_equal(got[2][b][1], want[2][b][1]) and got[2][b][2] == want[2][b][2], b
    if "RNNT_NO_GRAPH" in knobs:
        assert got[3][1] == want[3][1], "the same batches, so the same number of steps enqueued"
    else:
        assert got[3] != want[3], "the knob changed neither the launches nor the steps enqueued"


def test_token_buffer_isolation():
    """A stream that emits more than max_tokens: rnnt_get_tokens reports its full count and its row holds the oracle's first
    max_tokens tokens; the other stream of the same call (short, below the bound) is exact; the facade raises RnntError."""
    from ctc_vr_amd.lib import RnntError, _np_ptr
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    V, blank = 416, 5
    w = CONFIGS[(V, blank)]["saturated"]
    per, margin = _oracle_greedy(V, blank, w)
    assert margin >= MARGIN
    lens = [FRAMES, 48]
    want = [_tokens(per[0]), _tokens(per[1], _enc_len(48))]
    max_tokens = len(want[1]) + 3
    assert len(want[0]) > max_tokens + 100
    x = _inputs(2).cuda().contiguous()
    sb = StreamingBatch(_sd(V, blank, w), 2, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128, max_enc_frames=64,
                        max_tokens=max_tokens)
    with pytest.raises(RnntError):
        sb.decode_script_ragged(x, torch.tensor(lens), CHUNK)
    counts = np.zeros(2, np.int32)
    toks = np.full((2, max_tokens), -1, np.int32)
    rc = sb.engine.lib.rnnt_get_tokens(sb.engine.ctx, _np_ptr(counts), _np_ptr(toks), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert counts.tolist() == [len(want[0]), len(want[1])]
    assert toks[0].tolist() == want[0][:max_tokens]
    assert toks[1, :counts[1]].tolist() == want[1]


# ---- E. beam search ------------------------------------------------------------------------------------------------------------

BEAM_FRAMES = 112                 # 21 encoder frames per stream, two streams


_BEAM = {}


def _oracle_beam(V, blank, w, beam):
    from oracle import rnnt_oracle as O
    key = (V, blank, w, beam)
    if key not in _BEAM:
        sd = O.to_torch_sd(_sd(V, blank, w))
        n = _enc_len(BEAM_FRAMES)
        _BEAM[key] = [[(h.tokens, h.log_prob) for h in O.beam_frames(sd, _oracle_enc(s)[:, :n], None, blank, beam, N_STEPS)] for s in range(2)]
    return _BEAM[key]


@pytest.mark.parametrize("regime", ["sparse", "saturated"])
@pytest.mark.parametrize("cfg", [(412, 0), (64, 0), (6, 0), (513, 0)], ids=lambda c: f"V{c[0]}_blank{c[1]}")
def test_beam_search_edges(cfg, regime):
    """rnnt_beam_decode and rnnt_beam_advance (rnnt_beam_decode refuses V > 512) against the oracle's beam search, beams 4 and
    16 where V - 1 >= 16: hypotheses exact, scores within 2e-3.  Saturated, every chain runs all n_steps evaluations and leaves
    its state in the last pool slot.  beam_k > V - 1 is refused with RNNT_ERR_ARG and the context stays usable."""
    from ctc_vr_amd.lib import ERR_ARG, RnntError
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    V, blank = cfg
    w = CONFIGS[cfg][regime]
    per, _ = _oracle_greedy(V, blank, w)
    _assert_regime(per, regime)
    x = _inputs(2, BEAM_FRAMES).cuda().contiguous()
    sb = StreamingBatch(_sd(V, blank, w), 2, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128, max_enc_frames=64,
                        max_tokens=64, max_beam=16)
    s = torch.cuda.current_stream().cuda_stream
    plan = [(a, b) for a, b in T.chunk_plan(BEAM_FRAMES, CHUNK) if b - a >= 7]
    offs = [sum((b - a) // 4 for a, b in plan[:i]) for i in range(len(plan))]

    def encode():
        sb.reset()
        return sb.engine.encoder_chunks(x.data_ptr(), BEAM_FRAMES, [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s)

    for beam in ([4, 16] if V - 1 >= 16 else [4]):
        want = _oracle_beam(V, blank, w, beam)
        for entry in ("advance", "decode"):
            F = encode()
            assert F == _enc_len(BEAM_FRAMES)
            if entry == "decode" and V > 512:
                with pytest.raises(RnntError) as e:
                    sb.engine.beam_decode(0, None, beam, s)
                assert e.value.status == ERR_ARG
                continue
            if entry == "decode":
                sb.engine.beam_decode(0, None, beam, s)
            else:
                sb.engine.beam_advance(0, F, beam, s)
            for b in range(2):
                got = sb.engine.beam_hyps(b)
                assert [t for t, _ in got] == [t for t, _ in want[b]], (beam, entry, b)
                assert max(abs(p - q) for (_, p), (_, q) in zip(got, want[b])) < 2e-3, (beam, entry, b)
    F = encode()
    with pytest.raises(RnntError) as e:
        sb.engine.beam_frame(0, [0], [blank], V)                                   # beam_k = V > V - 1
    assert e.value.status == ERR_ARG
    sb.engine.beam_advance(0, F, 4, s)
    assert [t for t, _ in sb.engine.beam_hyps(0)] == [t for t, _ in _oracle_beam(V, blank, w, 4)[0]]


# ---- F. argmax ties ------------------------------------------------------------------------------------------------------------

TWIN_HEADS = ("joint.ffn_out", "predictor.embed")


def _twin_pairs(V, blank, w):
    """(a, b) pairs for the three placements relative to greedy_multi's parts (ceil(V / 4) rows each, 64-row waves in the logit
    finish), a being a token the oracle emits often on the inputs"""
    per, _ = _oracle_greedy(V, blank, w)
    toks = np.array([t for frames in per for t in _tokens(frames)])
    rp = (V + 3) // 4
    counts = np.bincount(toks, minlength=V)
    order = [int(t) for t in np.argsort(-counts, kind="stable") if counts[t] > 0]
    pick = {}
    for a in order:
        part, r = divmod(a, rp)
        base = part * rp
        if "wave" not in pick and r < 60:
            pick["wave"] = (a, base + 63 if a != base + 63 else base + 62)
        if "waves" not in pick and r < 64 and base + 64 < min(V, base + rp):
            pick["waves"] = (a, min(V, base + rp) - 1)
        if "parts" not in pick and part < 3 and base + rp < V:
            pick["parts"] = (a, min(V - 1, (part + 2) * rp + 5) if part + 2 < 4 else V - 1)
    return pick


@pytest.mark.parametrize("placement", ["wave", "waves", "parts"])
@pytest.mark.parametrize("path", ["default", "dec_multi0", "persistent0"])
def test_argmax_ties(path, placement, monkeypatch):
    """Exact twin tokens a < b (joint.ffn_out row and bias and predictor.embed row copied from a to b, so either one leaves the same
    predictor state): the
    reference's rule is torch.argmax, the first index, so the decoders never emit b -- within one 64-row wave of a greedy_multi
    part, across its two waves and across parts -- and the tokens equal the oracle's.  The tie is confirmed on the device first: rnnt_joint's two columns are bit-identical in fp32."""
    V, blank = 412, 0
    w = CONFIGS[(V, blank)]["mixed"]
    a, b = _twin_pairs(V, blank, w)[placement]
    assert a < b and b != blank and a != blank
    twins = ((a, b, TWIN_HEADS),)
    per, margin = _oracle_greedy(V, blank, w, twins)
    assert margin >= MARGIN, margin
    want = [_tokens(f) for f in per]
    assert sum(t == a for w in want for t in w) >= 3 and all(t != b for w in want for t in w)
    eng = _engine(V, blank, "fp32", w=w, twins=twins)
    enc = torch.randn(2, 9, 256, generator=torch.Generator().manual_seed(3)).cuda()
    prd = torch.randn(2, 5, 256, generator=torch.Generator().manual_seed(4)).cuda()
    out = torch.empty(2, 9, 5, V, device="cuda")
    eng.joint(enc.data_ptr(), prd.data_ptr(), 2, 9, 5, 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(out[..., a], out[..., b])
    if path == "dec_multi0":
        monkeypatch.setenv("RNNT_DEC_MULTI", "0")
    if path == "persistent0":
        monkeypatch.setenv("RNNT_PERSISTENT", "0")
    got = _decode_all(V, blank, w, ("per_chunk", "whole"), twins=twins)
    for entry, toks in got.items():
        for s in range(3):
            assert b not in toks[s], (entry, s)
            assert [a if t == b else t for t in toks[s]] == want[s], (entry, s)
            assert toks[s] == want[s], (entry, s)


def test_ctc_argmax_ties():
    """rnnt_ctc_argmax (EPI_ARGMAX key = value | ~index) on exact twins in ctc_head.ctc_lo (row and bias of a copied to b > a, a the
    most frequent frame decision): the first index wins as in torch.argmax, so b never appears and every other frame keeps its id.
    The tie is confirmed on the device first: rnnt_ctc_logprobs's two columns are bit-identical in fp32."""
    from ctc_vr_amd.lib import RnntEngine
    V, blank = 412, 0
    e2 = RnntEngine(max_streams=2, max_chunk_frames=320, max_cache_frames=128, max_enc_frames=128, vocab_size=V, blank_id=blank)
    x = torch.from_numpy(T.synth_fbank(2, 300, seed=5)).cuda().contiguous()
    lens = np.array([300, 300], np.int32)
    s = torch.cuda.current_stream().cuda_stream
    e2.load_state_dict(_sd(V, blank), numerics="fp32")
    plain = e2.ctc_argmax(x.data_ptr(), lens, 2, 300, s)
    counts = np.bincount(plain.ravel(), minlength=V)
    counts[blank] = 0
    a = int(np.argmax(counts))
    for b in (a + 1 if a // 64 == (a + 1) // 64 else a - 1, (a + 200) % V):
        lo, hi = min(a, b), max(a, b)
        if lo == blank:
            continue
        twins = ((lo, hi, ("ctc_head.ctc_lo",)),)
        e2.load_state_dict(_sd(V, blank, twins=twins), numerics="fp32")
        enc = torch.randn(50, 256, generator=torch.Generator().manual_seed(9)).cuda()
        lp = torch.empty(50, V, device="cuda")
        e2.ctc_logprobs(enc.data_ptr(), 50, lp.data_ptr(), s)
        torch.cuda.synchronize()
        assert torch.equal(lp[:, lo], lp[:, hi])
        tied = e2.ctc_argmax(x.data_ptr(), lens, 2, 300, s)
        assert not (tied == hi).any(), (lo, hi)
        assert (tied[plain == a] == lo).all(), (lo, hi)                              # a's frames now tie: the lower index
        keep = (plain != hi) & (plain != lo)
        assert np.array_equal(tied[keep], plain[keep]), (lo, hi)
