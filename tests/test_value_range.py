"""Operand magnitudes outside the range of the seeded weights and inputs, against float64: the streaming encoder on every profile
of range_cases.py (function-preserving power-of-two rescales, checkpoint-like LayerNorm / BatchNorm / attention statistics, an
outlier channel, digital silence and a loud input) through the per-chunk API and through rnnt_encoder_chunks with and without the
layer-major and fused schedules, the full-context encoder, the joint with saturated tanh arguments and the scoring pick on it, the
predictor step with saturated gates, CTC log-probabilities with a logit spread in the hundreds, and the greedy decode on two
profiles.  test_value_range_cpu.py holds the CPU side: the float32 oracle's share of the bars, the sensitivity of the profiles and
the split-alone predictions.  Beyond the declared operand range of the f16x3 mode (include/rnnt_hip.h) rnnt_finalize_weights
refuses the mode, naming the tensor; the tests assert that refusal.  Needs a real MI355X.  Nothing here provokes a device fault."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
import range_cases as R
import window_cases as W
from ctc_vr_amd.lib import ERR_ARG, RnntEngine, RnntError
from ctc_vr_amd.online_rnnt_model import StreamingBatch
from test_decode_edges import _lstm64, _w64
from test_score import _bits, _pred_rows, _ragged, _score, _targets, _valid_masks

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3", "f16x3"]
VARIANTS = {"default": {}, "nolm_nofused": {"RNNT_LM": "0", "RNNT_FUSED": "0"}}
KNOBS = ("RNNT_ATTN_RESIDENT", "RNNT_FUSED", "RNNT_LM")
PATHS = ("chunk", "whole", "whole_nolm_nofused")
FULL_PROFILES, FULL_T, FULL_LENS = ("sharp", "outlier"), 47, [47, 46, 23, 7]
GREEDY_PROFILES = tuple(R.GREEDY_SEEDS)
CTX_CHUNK = 48                                          # largest chunk of a context: the 47-frame full-context call and the decode script's 24-frame tail
LOGIT_TOL = R.LOGIT_TOL


@pytest.fixture(params=MODES)
def numerics(request):
    return request.param


@contextlib.contextmanager
def _env(mode, variant="default"):
    """a context reads its knobs at rnnt_create: the mode, materialised encoder frames, and the variant's schedule knobs"""
    want = {"RNNT_NUMERICS": mode, "RNNT_FUSE_AFTER_NORM": "0", **{k: None for k in KNOBS}, **VARIANTS[variant]}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _weights_of(profile):
    return profile if R.PROFILES[profile][0] is not None else "base"


def _refused(mode, profile):
    return mode == "f16x3" and profile in R.FAMILY_A_BEYOND


def _batch(mode, variant, weights, n=R.N_STREAMS):
    with _env(mode, variant):
        return StreamingBatch(R.state_dict(weights), n, max_chunk_frames=CTX_CHUNK, max_cache_frames=256, max_enc_frames=256, numerics=mode)


def _caches(eng, n):
    s = _stream()
    return [eng.att_cache(b, s) for b in range(n)], [eng.cnn_cache(b, s) for b in range(n)]


def _per_chunk(sb, profile, plan):
    """rnnt_encoder_chunk chunk by chunk; after EVERY chunk the new frames and both caches of every stream against that stream's
    float64 oracle -> (largest |difference| per tensor, largest share of a bar per tensor)"""
    eng, s, n = sb.engine, _stream(), sb.n
    x = torch.from_numpy(R.plan_input(profile, plan)).cuda().contiguous()
    refs = [R.case_ref(profile, plan, b) for b in range(n)]
    d, share = np.zeros(3), np.zeros(3)
    sb.reset()
    for c, (st, ln, off, req) in enumerate(R.plan_of(plan)):
        tq = eng.encoder_chunk(x[:, st:st + ln].contiguous().data_ptr(), ln, off, req, s)
        fr = np.array(eng.enc_frames(s), copy=True)
        assert fr.shape == (n, tq, 256) and tq == W.sub_len(ln)
        eng.frames_discard(s)
        att, cnn = _caches(eng, n)
        for b in range(n):
            assert att[b].shape == refs[b][c]["att"].shape, (c, b, att[b].shape)
            assert all(np.isfinite(a).all() for a in (fr[b], att[b], cnn[b])), (profile, plan, c, b)
            dc, sc = R.chunk_distance({"frames": fr[b], "att": att[b], "cnn": cnn[b]}, refs[b][c])
            d, share = np.maximum(d, dc), np.maximum(share, sc)
    return d, share


def _whole(sb, profile, plan):
    """ONE rnnt_encoder_chunks call over the plan: the frames of all chunks and the caches after the last one against float64"""
    eng, s, n = sb.engine, _stream(), sb.n
    x = torch.from_numpy(R.plan_input(profile, plan)).cuda().contiguous()
    p = R.plan_of(plan)
    sb.reset()
    got = eng.encoder_chunks(x.data_ptr(), x.shape[1], *[[c[i] for c in p] for i in range(4)], s)
    assert got == W.plan_frames(p)[1]
    frames = np.array(eng.enc_frames(s), copy=True)
    att, cnn = _caches(eng, n)
    d, share = np.zeros(3), np.zeros(3)
    for b in range(n):
        last = R.case_ref(profile, plan, b)[-1]
        assert att[b].shape == last["att"].shape, (b, att[b].shape)
        assert all(np.isfinite(a).all() for a in (frames[b], att[b], cnn[b])), (profile, plan, b)
        dc, sc = R.chunk_distance({"frames": frames[b], "att": att[b], "cnn": cnn[b]}, {**last, "frames": R.ref_frames(profile, plan, b)})
        d, share = np.maximum(d, dc), np.maximum(share, sc)
    return d, share


def _full_ref(profile):
    key = ("full", profile)
    if key not in R._CACHE:
        from oracle import rnnt_oracle as O
        x = T.synth_fbank(len(FULL_LENS), FULL_T, seed=4700 + FULL_T)
        with torch.no_grad():
            want, mask = O.encoder_full(T.ref_state_dict(R.state_dict(profile), share=W.state_dict()), torch.from_numpy(x).double(), torch.tensor(FULL_LENS))
        R._CACHE[key] = (x, want.numpy(), mask[:, 0].sum(1).tolist())
    return R._CACHE[key]


def _full(sb, profile):
    x, want, valid = _full_ref(profile)
    n, tq = len(FULL_LENS), W.sub_len(FULL_T)
    out = torch.empty(n, tq, 256, device="cuda")
    assert sb.engine.encoder_full(torch.from_numpy(x).cuda().contiguous().data_ptr(), FULL_LENS, n, FULL_T, out.data_ptr(), _stream()) == tq
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert all(np.isfinite(got[b, :valid[b]]).all() for b in range(n))
    return [W.maxdiff(got[b, :valid[b]], want[b, :valid[b]]) for b in range(n)]


_RES = {}


def _run(mode, variant, weights):
    """Everything one context (mode, variant, weights) is asked: both plans of every profile on these weights through the per-chunk
    API (default variant) and one rnnt_encoder_chunks call; in the default variant also the full-context call and the greedy
    decode where the profile has them.  The context is closed afterwards.  -> {(profile, plan, path) | ("full" | "greedy", profile): result}"""
    key = (mode, variant, weights)
    if key not in _RES:
        out = {}
        sb = _batch(mode, variant, weights, n=max(R.N_STREAMS, len(FULL_LENS)) if variant == "default" and weights in FULL_PROFILES else R.N_STREAMS)
        n_ctx, sb.n = sb.n, R.N_STREAMS
        for profile in [p for p in R.GRID if _weights_of(p) == weights]:
            for plan in R.PLANS:
                if variant == "default":
                    out[(profile, plan, "chunk")] = _per_chunk(sb, profile, plan)
                    out[(profile, plan, "whole")] = _whole(sb, profile, plan)
                else:
                    out[(profile, plan, "whole_" + variant)] = _whole(sb, profile, plan)
        if variant == "default" and weights in GREEDY_PROFILES:
            x = torch.from_numpy(R.greedy_input(weights)).cuda()
            out[("greedy", weights)] = sb.decode_script(x.expand(R.N_STREAMS, -1, -1).contiguous(), R.GREEDY_CHUNK)
        if variant == "default" and weights in FULL_PROFILES:
            sb.n = n_ctx
            sb.reset()
            out[("full", weights)] = _full(sb, weights)
        sb.engine.close()
        _RES[key] = out
    return _RES[key]


def _expect_refusal(mode, variant, profile):
    """rnnt_finalize_weights(F16X3) refuses weights beyond the declared range: RNNT_ERR_ARG and a message naming a tensor the
    CPU restatement of the limit (range_cases.f16x3_refused) refuses too"""
    key = ("refused", mode, variant, profile)
    if key not in _RES:
        with pytest.raises(RnntError) as e:
            _batch(mode, variant, profile)
        names = [k for k, _, _ in R.f16x3_refused(R.state_dict(profile))]
        assert e.value.status == ERR_ARG and "f16x3" in str(e.value) and any(k in str(e.value) for k in names), str(e.value)
        _RES[key] = str(e.value)
    return _RES[key]


# ---- 1. the encoder grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("plan", list(R.PLANS))
@pytest.mark.parametrize("profile", R.GRID)
def test_encoder_grid(numerics, profile, plan, path):
    """Every profile x both plans x every parity mode, two streams of different audio, through the per-chunk API (frames and both
    caches after EVERY chunk), one rnnt_encoder_chunks call in a default context (layer-major; resident attention in the split
    modes) and one with RNNT_LM=0 RNNT_FUSED=0 (wavefront, unfused half-blocks): frames within LOGIT_TOL of that stream's float64
    oracle, att_cache and cnn_cache within LOGIT_TOL * max(1, max |reference tensor|).  The envelope profiles hold in all three
    modes, the beyond-envelope rescales in fp32 and bf16x3; f16x3 refuses those at rnnt_finalize_weights."""
    variant = "nolm_nofused" if path == "whole_nolm_nofused" else "default"
    if _refused(numerics, profile):
        print(f"[{numerics}] {profile}: refused: {_expect_refusal(numerics, variant, profile)}")
        return
    d, share = _run(numerics, variant, _weights_of(profile))[(profile, plan, path)]
    print(f"[{numerics}] {profile} {plan} {path}: max |diff| to float64: frames {d[0]:.3e}, att_cache {d[1]:.3e}, cnn_cache {d[2]:.3e}; "
          f"share of the bars {share[0]:.3f} {share[1]:.3f} {share[2]:.3f}")
    assert share.max() <= 1.0, (profile, plan, path, d, share)


def test_f16x3_refusal_leaves_the_other_modes(numerics):
    """One context: the vo-9 weights are refused in f16x3 (the largest predicted split error, 1.5e-3 on the frames before any kernel
    arithmetic), nothing was launched for them, and the same loaded tensors finalize in this test's mode when that is not f16x3 --
    or, in f16x3, the base weights loaded over them do -- and run a plan within the bars."""
    with _env(numerics):
        sb = StreamingBatch(R.state_dict("base"), R.N_STREAMS, max_chunk_frames=CTX_CHUNK, max_cache_frames=256, max_enc_frames=256, numerics=numerics)
    eng = sb.engine
    with pytest.raises(RnntError) as e:
        eng.load_state_dict(R.state_dict("vo-9"), numerics="f16x3")
    assert e.value.status == ERR_ARG and "linear_out.weight" in str(e.value) and "RNNT_F16X3_SPLIT_LIMIT" in str(e.value), str(e.value)
    profile = "base" if numerics == "f16x3" else "vo-9"
    eng.load_state_dict(R.state_dict(profile), numerics=numerics)
    d, share = _whole(sb, profile, "19-all")
    eng.close()
    print(f"[{numerics}] {profile} after the refusal: frames {d[0]:.3e}, att_cache {d[1]:.3e}, cnn_cache {d[2]:.3e}")
    assert share.max() <= 1.0, (d, share)


# ---- 2. full context --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", FULL_PROFILES)
def test_full_context(numerics, profile):
    """rnnt_encoder_full on sharpened scores and on the outlier channels, T = 47 with lens [47, 46, 23, 7]: the valid frames within
    LOGIT_TOL of encoder_full in float64."""
    err = _run(numerics, "default", profile)[("full", profile)]
    print(f"[{numerics}] full context {profile}: max |diff| to float64 per stream {' '.join(f'{e:.3e}' for e in err)}")
    assert max(err) <= LOGIT_TOL, err


# ---- 3. joint, scoring, predictor, CTC on saturating weights ----------------------------------------------------------------------
_SD, _ENG = {}, {}


def _dec_sd(V, what):
    """make_state_dict(0, vocab=V) with one group of decoder-side weights scaled"""
    if (V, what) not in _SD:
        sd = dict(T.make_state_dict(0, vocab=V))
        scale = {"joint": [("joint.enc_ffn.weight", 16), ("joint.enc_ffn.bias", 16), ("joint.pred_ffn.weight", 16), ("joint.pred_ffn.bias", 16)],
                 "lstm": [("predictor.rnn.weight_ih_l0", 8), ("predictor.rnn.weight_hh_l0", 8), ("predictor.embed.weight", 10)],
                 "ctc": [("ctc_head.ctc_lo.weight", 40), ("ctc_head.ctc_lo.bias", 40)]}[what]
        for name, f in scale:
            sd[name] = sd[name] * np.float32(f)
        _SD[(V, what)] = sd
    return _SD[(V, what)]


def _dec_engine(V, what, mode):
    key = (V, what, mode)
    if key not in _ENG:
        with _env(mode):
            e = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=V, blank_id=T.BLANK, max_beam=0)
            e.load_state_dict(_dec_sd(V, what), numerics=mode)
        _ENG[key] = e
    return _ENG[key]


JOINT_SHAPE = (2, 37, 11)


def _joint_inputs(V):
    g = torch.Generator().manual_seed(900 + V)
    B, Tn, U = JOINT_SHAPE
    return torch.randn(B, Tn, 256, generator=g).cuda(), (torch.randn(B, U, 256, generator=g) * 0.5).cuda()


def _joint64(sd, enc, prd):
    we, be, wp, bp, wo, bo = _w64(sd, "joint.enc_ffn.weight", "joint.enc_ffn.bias", "joint.pred_ffn.weight", "joint.pred_ffn.bias",
                                  "joint.ffn_out.weight", "joint.ffn_out.bias")
    arg = (enc.double() @ we.T + be)[:, :, None, :] + (prd.double() @ wp.T + bp)[:, None, :, :]
    return arg, torch.tanh(arg) @ wo.T + bo


@pytest.mark.parametrize("V", [412, 413])
def test_joint_tanh_saturation(V, numerics):
    """joint.enc_ffn / joint.pred_ffn weight and bias x16 drive the tanh arguments past +-44, where 1 - tanh underflows in float32
    and exp(2x) of a clamp-free tanh is beyond e^88: rnnt_joint modes 0 and 1 at (2, 37, 11) -- V = 412 the rows kernel in the split
    modes, 413 the GEMM + log-softmax fallback -- within LOGIT_TOL of the float64 formula on the logits and on every log-probability
    whose reference is above -30, and no NaN or inf anywhere."""
    B, Tn, U = JOINT_SHAPE
    eng, sd = _dec_engine(V, "joint", numerics), _dec_sd(V, "joint")
    enc, prd = _joint_inputs(V)
    arg, ref = _joint64(sd, enc, prd)
    assert float(arg.abs().max()) > 88.0 and float((arg.abs() > 44.0).float().mean()) > 0.25, float(arg.abs().max())
    assert float((arg.abs() < 1.0).float().mean()) > 1e-3                                       # and some arguments stay in the linear part
    for mode, want in ((0, ref), (1, torch.log_softmax(ref, dim=-1))):
        out = torch.full((B, Tn, U, V), float("nan"), device="cuda")
        eng.joint(enc.data_ptr(), prd.data_ptr(), B, Tn, U, mode, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()), int((~torch.isfinite(out)).sum())
        keep = want > -30.0 if mode == 1 else torch.ones_like(want, dtype=torch.bool)
        err = float((out.double() - want).abs()[keep].max())
        print(f"[{numerics}] joint V={V} mode {mode}: max |tanh argument| {float(arg.abs().max()):.1f}, max |diff| to float64 {err:.3e} over {float(keep.float().mean()):.3f} of the lattice")
        assert err <= LOGIT_TOL, (mode, err)


def test_pick_on_the_saturated_joint(numerics):
    """On the same weights rnnt_transducer_nll's pick equals rnnt_joint(mode=1) at (blank, target) on every valid cell, bit for bit
    (the contract of test_score.py::test_pick_is_the_lattice_bitwise), and the likelihoods are finite."""
    B, Tn, U1 = 3, 37, 11
    eng, dev = _dec_engine(412, "joint", numerics), torch.device("cuda", 0)
    Tb, Ub = _ragged(B, Tn, U1 - 1)
    tg = _targets(B, U1 - 1, Ub, seed=100 * B + Tn)
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(977)).to(dev)
    nll, pick = _score(eng, enc_d, Tb, tg, Ub)
    assert np.isfinite(nll).all()
    pred = _pred_rows(eng, tg, Ub, dev)
    lat = torch.full((B, Tn, U1, 412), float("nan"), device=dev)
    eng.joint(enc_d.data_ptr(), pred.data_ptr(), B, Tn, U1, 1, lat.data_ptr(), _stream())
    torch.cuda.synchronize()
    col = np.full((B, U1), T.BLANK, np.int64)
    for b in range(B):
        col[b, :Ub[b]] = tg[b, :Ub[b]]
    idx = torch.from_numpy(col).to(dev)[:, None, :, None].expand(B, Tn, U1, 1)
    want_blank, want_label = lat[..., T.BLANK].cpu().numpy(), lat.gather(3, idx)[..., 0].cpu().numpy()
    vb, vl = _valid_masks(B, Tn, U1, Tb, Ub)
    assert np.isfinite(pick[..., 0][vb]).all() and np.isfinite(pick[..., 1][vl]).all()
    assert np.array_equal(_bits(pick[..., 0])[vb], _bits(want_blank)[vb]) and np.array_equal(_bits(pick[..., 1])[vl], _bits(want_label)[vl])


def _lstm32(sd, tok, h, c):
    """the LSTM step in plain float32 on the device: the share of the bar float32 arithmetic uses by itself"""
    w = [torch.from_numpy(sd[n]).cuda() for n in ("predictor.embed.weight", "predictor.rnn.weight_ih_l0", "predictor.rnn.weight_hh_l0", "predictor.rnn.bias_ih_l0",
                                                   "predictor.rnn.bias_hh_l0", "predictor.projection.weight", "predictor.projection.bias")]
    g = w[0][tok.long()] @ w[1].T + w[3] + h @ w[2].T + w[4]
    i, f, gg, o = g.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    h2 = torch.sigmoid(o) * torch.tanh(c2)
    return h2 @ w[5].T + w[6], h2, c2


@pytest.mark.parametrize("rows", [1, 65])
def test_predictor_step_saturated_gates(rows, numerics):
    """rnnt_predictor_step with the LSTM weights x8 and the embedding x10 (gate pre-activations of several hundred: sigmoid and tanh
    of +-inf-like arguments), h ~ N(0, 1), c ~ N(0, 3^2), one row and one more than a 64-row tile: out / h / c finite and within
    LOGIT_TOL of a float64 LSTM step.  The bar is what float32 allows here, not a looser one: the pre-activations reach 1800, where
    a float32 ulp is 1.2e-4, so a sum of 512 products carries a few 1e-4; a gate on its linear part passes at most a quarter of
    that on, times |c| up to 10, into c'.  A float32 torch step is printed beside the kernel's figures (measured: c' 2.7e-4 for
    torch, 9.5e-5 for the kernel at 65 rows)."""
    V = 412
    eng, sd = _dec_engine(V, "lstm", numerics), _dec_sd(V, "lstm")
    g = torch.Generator().manual_seed(rows * 7 + 1)
    tok = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    tok[0] = T.BLANK
    tok = tok.cuda()
    h, c = torch.randn(rows, 256, generator=g).cuda(), (torch.randn(rows, 256, generator=g) * 3).cuda()
    outs = [torch.full((rows + 2, 256), 1234.5, device="cuda") for _ in range(3)]
    eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), rows, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _stream())
    torch.cuda.synchronize()
    want = _lstm64(sd, tok, h, c)
    emb, wih, whh = _w64(sd, "predictor.embed.weight", "predictor.rnn.weight_ih_l0", "predictor.rnn.weight_hh_l0")
    pre = emb[tok.long()] @ wih.T + h.double() @ whh.T
    assert float(pre.abs().max()) > 200.0 and float((pre.abs() > 20.0).float().mean()) > 0.5       # saturated gates
    base = [float((a.double() - b).abs().max()) for a, b in zip(_lstm32(sd, tok, h, c), want)]
    err = [float((o[:rows].double() - w).abs().max()) for o, w in zip(outs, want)]
    print(f"[{numerics}] predictor step rows={rows}: max |pre-activation| {float(pre.abs().max()):.0f}; out / h / c vs float64 "
          f"{err[0]:.3e} {err[1]:.3e} {err[2]:.3e}; float32 torch {base[0]:.3e} {base[1]:.3e} {base[2]:.3e}")
    for o in outs:
        assert bool(torch.isfinite(o[:rows]).all()) and bool((o[rows:] == 1234.5).all())
    assert max(err) <= LOGIT_TOL, err


def ctc_bar(ref):
    """LOGIT_TOL on every log-probability a decode can use (above -30, p > 1e-13), LOGIT_TOL / 30 of the value below: 3.3e-5
    relative, a few hundred float32 ulps, where the values are in the hundreds"""
    return LOGIT_TOL * torch.clamp(ref.abs() / 30.0, min=1.0)


@pytest.mark.parametrize("V", [412, 413])
@pytest.mark.parametrize("rows", [1, 65])
def test_ctc_logprobs_wide_logits(rows, V, numerics):
    """rnnt_ctc_logprobs with ctc_lo weight and bias x40 (logits spread over several hundred, one class holding nearly all the
    mass): finite, within ctc_bar of log_softmax in float64, and every row sums to 1 within 1e-5 in float64."""
    eng, sd = _dec_engine(V, "ctc", numerics), _dec_sd(V, "ctc")
    enc = torch.randn(rows, 256, generator=torch.Generator().manual_seed(rows + V)).cuda()
    w, b = _w64(sd, "ctc_head.ctc_lo.weight", "ctc_head.ctc_lo.bias")
    logits = enc.double() @ w.T + b
    ref = torch.log_softmax(logits, dim=-1)
    assert float(logits.max() - logits.min()) > 200.0
    out = torch.full((rows, V), float("nan"), device="cuda")
    eng.ctc_logprobs(enc.data_ptr(), rows, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    excess = float(((out.double() - ref).abs() / ctc_bar(ref)).max())
    total = torch.exp(out.double()).sum(-1)
    print(f"[{numerics}] ctc log-probs rows={rows} V={V}: logit spread {float(logits.max() - logits.min()):.0f}, max |diff| to float64 "
          f"{float((out.double() - ref).abs().max()):.3e}, largest share of the bar {excess:.3f}, row sums within {float((total - 1).abs().max()):.2e} of 1")
    assert excess <= 1.0, excess
    assert float((total - 1).abs().max()) <= 1e-5


# ---- 4. greedy decode -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", GREEDY_PROFILES)
def test_greedy_tokens(numerics, profile):
    """One 200-frame stream at chunk 16 on sharpened scores and on checkpoint-like LayerNorm statistics: the oracle's smallest top-2
    margin is >= 1e-3 (the fbank seed was chosen on the CPU so that it is; test_value_range_cpu.py asserts it too), so the tokens of
    every mode equal the oracle's."""
    toks, _, margin = R.greedy_oracle(profile)
    assert margin >= R.GREEDY_MARGIN and len(toks) > 0, margin
    got = _run(numerics, "default", profile)[("greedy", profile)]
    print(f"[{numerics}] greedy {profile}: {len(toks)} tokens, oracle's smallest top-2 margin {margin:.3e}")
    assert got[0] == got[1] == toks, (len(got[0]), len(toks))
