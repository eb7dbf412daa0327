"""Profiles, plans, bars and float64 references shared by test_value_range_cpu.py and test_value_range.py: the encoder on weights
and inputs whose operand magnitudes leave the range of testing.make_state_dict / synth_fbank.  Every profile is a pure function of
make_state_dict(0) (Philox-seeded where it draws), so both files and every later run see the same tensors.  No GPU is touched here.

Family A rescales an operand pair by exact powers of two and leaves the float64 function unchanged; family B changes the function
towards the statistics of a trained checkpoint; family C changes the input on the base weights."""
import numpy as np

import ctc_vr_amd.testing as T
import window_cases as W

LOGIT_TOL = W.LOGIT_TOL          # frames: absolute (O(4) after after_norm); caches: times max(1, max |reference tensor|)
SEED_W = W.SEED_W
N_STREAMS = 2
ENVELOPE_S = 6
L = T.L

# the declared limit of rnnt_finalize_weights(F16X3) (include/rnnt_hip.h RNNT_F16X3_SPLIT_LIMIT), restated: relative r.m.s. error of
# the hi + lo planes of a GEMM weight
F16X3_SPLIT_LIMIT = 1e-4
F16_MAX = 65504.0


def _layers(suffix):
    return [f"encoder.encoders.{i}.{suffix}" for i in range(L)]


def _scaled(sd, factors):
    """a shallow copy of sd with sd[name] * factor for every (name, factor); untouched entries stay the same array objects"""
    out = dict(sd)
    for name, f in factors.items():
        out[name] = np.ascontiguousarray(sd[name] * np.float32(f))
    return out


def rescale(sd, pair, s):
    """Family A.  qk, s: linear_q.{weight,bias}, pos_bias_u, pos_bias_v by 2^-s and linear_k.{weight,bias}, linear_pos.weight by 2^s
    (every score q.k and q.p unchanged); vo, s: linear_v.{weight,bias} by 2^-s and linear_out.weight by 2^s."""
    down, up = 2.0 ** -s, 2.0 ** s
    f = {}
    if pair == "qk":
        for n in ("linear_q.weight", "linear_q.bias", "pos_bias_u", "pos_bias_v"):
            f.update({k: down for k in _layers("self_attn." + n)})
        for n in ("linear_k.weight", "linear_k.bias", "linear_pos.weight"):
            f.update({k: up for k in _layers("self_attn." + n)})
    else:
        assert pair == "vo", pair
        for n in ("linear_v.weight", "linear_v.bias"):
            f.update({k: down for k in _layers("self_attn." + n)})
        f.update({k: up for k in _layers("self_attn.linear_out.weight")})
    return _scaled(sd, f)


def _log_uniform(key, lo, hi, n):
    g = np.random.Generator(np.random.Philox(key=[SEED_W, key]))
    return np.exp(g.uniform(np.log(lo), np.log(hi), n)).astype(np.float32)


def _sharp(sd):
    f = {}
    for n in ("linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_k.bias", "linear_pos.weight", "pos_bias_u", "pos_bias_v"):
        f.update({k: 3.0 for k in _layers("self_attn." + n)})
    return _scaled(sd, f)


LN_NAMES = ("norm_ff_macaron", "norm_mha", "norm_conv", "norm_ff", "norm_final")


def _ln_affine(sd):
    out = dict(sd)
    for i in range(L):
        for j, n in enumerate(LN_NAMES):
            p = f"encoder.encoders.{i}.{n}."
            out[p + "weight"] = np.ascontiguousarray(sd[p + "weight"] * _log_uniform(0x1A000 + 8 * i + j, 0.05, 6.0, T.D))
            out[p + "bias"] = np.ascontiguousarray(sd[p + "bias"] * np.float32(10.0))
    return out


def _bn_wide(sd):
    out = dict(sd)
    for i in range(L):
        p = f"encoder.encoders.{i}.conv_module.norm."
        out[p + "running_var"] = _log_uniform(0xB2000 + i, 1e-4, 10.0, T.D)
        out[p + "running_mean"] = np.ascontiguousarray(sd[p + "running_mean"] * np.float32(5.0))
    return out


OUTLIER_CHANNELS, OUTLIER = [7, 200], 300.0


def _outlier(sd):
    out = dict(sd)
    b = sd["encoder.embed.out.0.bias"].copy()
    b[OUTLIER_CHANNELS] += np.float32(OUTLIER / 16.0)          # +300 on two residual channels after the x16 embed scale
    out["encoder.embed.out.0.bias"] = b
    return out


SILENCE = (20, 60, -100.0)       # frames [20, 60) of every stream: -100 dB digital silence across a chunk boundary
LOUD = 45.0


def _silence(x):
    x = x.copy()
    x[:, SILENCE[0]:SILENCE[1]] = np.float32(SILENCE[2])
    return x


def _loud(x):
    return (x + np.float32(LOUD)).astype(np.float32)


def _a(pair, s):
    return lambda sd: rescale(sd, pair, s)


# name -> (weights from the base state dict or None, input from the base fbank or None)
PROFILES = {
    "base": (None, None),
    "qk+6": (_a("qk", 6), None), "qk-6": (_a("qk", -6), None), "vo+6": (_a("vo", 6), None), "vo-6": (_a("vo", -6), None),
    "qk+10": (_a("qk", 10), None), "qk-10": (_a("qk", -10), None), "vo+9": (_a("vo", 9), None), "vo-9": (_a("vo", -9), None),
    "sharp": (_sharp, None), "ln_affine": (_ln_affine, None), "bn_wide": (_bn_wide, None), "outlier": (_outlier, None),
    "silence": (None, _silence), "loud": (None, _loud),
}
FAMILY_A_ENVELOPE = ("qk+6", "qk-6", "vo+6", "vo-6")
FAMILY_A_BEYOND = ("qk+10", "qk-10", "vo+9", "vo-9")
FAMILY_A = FAMILY_A_ENVELOPE + FAMILY_A_BEYOND
FAMILY_B = ("sharp", "ln_affine", "bn_wide", "outlier")
FAMILY_C = ("silence", "loud")
ENVELOPE = FAMILY_A_ENVELOPE + FAMILY_B + FAMILY_C          # must pass in fp32, bf16x3 and f16x3
GRID = tuple(p for p in PROFILES if p != "base")

# (chunk length, policy): t' = 4 is the direct-stream attention, t' = 9 the NQ = 4 one; 4 chunks each
PLANS = {"19-all": (19, "all"), "39-two": (39, "two")}
N_CHUNKS = 4
MAX_CHUNK_FRAMES = 40            # one context serves both plans (t' of 40 frames is 9, as of 39)


def plan_of(plan):
    length, policy = PLANS[plan]
    return W.make_plan(length, policy, N_CHUNKS)


_CACHE = {}


def state_dict(profile="base"):
    key = ("sd", profile)
    if key not in _CACHE:
        base = W.state_dict()
        fn = PROFILES[profile][0]
        _CACHE[key] = base if fn is None else fn(base)
    return _CACHE[key]


def plan_input(profile, plan):
    """[N_STREAMS, frames, 80] float32: a different utterance per stream and per plan, the profile's input change applied"""
    fn = PROFILES[profile][1]
    key = ("x", profile if fn else "base", plan)
    if key not in _CACHE:
        if fn is None:
            _CACHE[key] = T.synth_fbank(N_STREAMS, W.plan_frames(plan_of(plan))[0], seed=5000 + PLANS[plan][0])
        else:
            _CACHE[key] = fn(plan_input("base", plan))
    return _CACHE[key]


def stream_ref(sd, x, plan, dtype=None):
    """encoder_stream_ref on a variant of the base weights; the cast copies of untouched tensors are the base's"""
    T.ref_state_dict(sd, dtype, share=W.state_dict())
    return T.encoder_stream_ref(sd, x, plan_of(plan), dtype)


def case_ref(profile, plan, stream=0, dtype=None):
    """the oracle over one stream of (profile, plan): float64 unless dtype says otherwise, computed once per session"""
    key = ("ref", profile, plan, stream, dtype)
    if key not in _CACHE:
        _CACHE[key] = stream_ref(state_dict(profile), plan_input(profile, plan)[stream], plan, dtype)
    return _CACHE[key]


def ref_frames(profile, plan, stream=0):
    return np.concatenate([r["frames"] for r in case_ref(profile, plan, stream)], 0)


def bars(ref_chunk):
    """(frames, att_cache, cnn_cache) bars against one chunk of a float64 reference"""
    rel = [max(1.0, float(np.abs(ref_chunk[k]).max())) if ref_chunk[k].size else 1.0 for k in ("att", "cnn")]
    return np.array([LOGIT_TOL, LOGIT_TOL * rel[0], LOGIT_TOL * rel[1]])


def chunk_distance(got, ref_chunk):
    """one chunk {"frames", "att", "cnn"} against a float64 reference chunk -> (|difference| per tensor, the same as a share of its bar)"""
    d = np.array([W.maxdiff(got[k], ref_chunk[k]) for k in ("frames", "att", "cnn")])
    return d, d / bars(ref_chunk)


def ref_distance(got, ref):
    """per-chunk results against a float64 reference -> (largest |difference| per tensor, largest share of a bar per tensor)"""
    d, s = zip(*[chunk_distance(g, r) for g, r in zip(got, ref)])
    return np.max(d, 0), np.max(s, 0)


# ---- the split of the encoder's weights, restated (test_value_range_cpu.py's predictions) ---------------------------------------
def is_split_weight(name, a):
    """the encoder-block weights a split mode carries as 16-bit planes: every >= 2-D tensor except the depthwise conv"""
    return name.startswith("encoder.encoders.") and np.asarray(a).ndim >= 2 and "depthwise_conv" not in name


def split_state_dict(sd, kind):
    """sd with every split weight replaced by its hi + lo planes (float64 arrays; everything else untouched)"""
    out = dict(sd)
    for k, v in sd.items():
        if is_split_weight(k, v):
            out[k] = T.split_planes_ref(v, kind)
    return out


# the GEMM weights rnnt_finalize_weights(F16X3) examines (api_lifecycle.hip.inc f16x3_refusal), restated
def is_f16x3_checked(name, a):
    skip = ("depthwise_conv", "linear_pos", "pos_enc", "pos_bias", "embed.conv.0", "predictor.embed", "weight_ih")
    return np.asarray(a).ndim >= 2 and np.asarray(a).dtype.kind == "f" and not any(s in name for s in skip)


_SPLIT_ERR = {}


def f16_split_error(a):
    """(split_error_ref(a, "f16"), max |a|), kept per array object (the profiles share every tensor they do not change)"""
    if id(a) not in _SPLIT_ERR:
        _SPLIT_ERR[id(a)] = (a, T.split_error_ref(a, "f16"), float(np.abs(a).max()))
    return _SPLIT_ERR[id(a)][1:]


def f16x3_refused(sd):
    """[(tensor name, split error, max |w|)] of the tensors rnnt_finalize_weights(F16X3) refuses, in state-dict order"""
    out = []
    for k, v in sd.items():
        if is_f16x3_checked(k, v):
            e, m = f16_split_error(v)
            if e > F16X3_SPLIT_LIMIT or m > F16_MAX:
                out.append((k, e, m))
    return out


# ---- greedy decode on two profiles (one 200-frame stream at chunk 16) ------------------------------------------------------------
GREEDY_FRAMES, GREEDY_CHUNK, GREEDY_MARGIN = 200, 16, 1e-3
# profile -> fbank seed, chosen on the CPU among 11 .. 34 so that the oracle's smallest top-2 logit margin is >= GREEDY_MARGIN and the
# stream emits: sharp gives 79 tokens at a margin of 4.0e-2; the ln_affine frames leave the blank (bias 11) on top almost everywhere
# on every one of those seeds, and seed 22 is the one with an emitted token and the widest margin (1.2e-1)
GREEDY_SEEDS = {"sharp": 13, "ln_affine": 22}
GREEDY_TOKENS = {"sharp": 79, "ln_affine": 1}


def greedy_input(profile, seed=None):
    """[1, 200, 80] float32"""
    return T.synth_fbank(1, GREEDY_FRAMES, seed=GREEDY_SEEDS[profile] if seed is None else seed)


def greedy_oracle(profile, seed=None):
    """the float32 oracle's decode-script greedy run of the profile's stream -> (tokens, encoder frames [1, F, 256], the smallest
    top-2 logit margin of its decisions in a float64 replay)"""
    key = ("greedy", profile, seed)
    if key not in _CACHE:
        import torch
        from oracle import rnnt_oracle as O
        sd = state_dict(profile)
        x = torch.from_numpy(greedy_input(profile, seed))
        st = O.OracleStream(O.to_torch_sd(sd), T.BLANK, GREEDY_CHUNK)
        toks, encs = [], []
        with torch.no_grad():
            for a, b in T.chunk_plan(GREEDY_FRAMES, GREEDY_CHUNK):
                tr = {}
                toks += st.process_single_chunk(x[:, a:b], trace=tr)
                if "enc_out" in tr:
                    encs.append(tr["enc_out"])
        enc = torch.cat(encs, 1)
        m, ok = T.greedy_margins(sd, enc.numpy(), [toks], blank=T.BLANK, device="cpu")
        assert ok.all(), f"{profile}: the float64 replay does not reproduce the oracle's tokens"
        _CACHE[key] = (toks, enc.numpy(), float(m[0]))
    return _CACHE[key]
