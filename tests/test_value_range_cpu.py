"""The value-range profiles of test_value_range.py without a GPU: how much of the bars plain float32 uses on every profile, that the
power-of-two rescales leave the function alone and the checkpoint-like profiles move it, and what the split of the weights into
two 16-bit planes alone does to the encoder frames under each rescale -- the predictions the device results are read against, and
the ground of the limit below which rnnt_finalize_weights refuses the f16x3 mode."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
import range_cases as R
import window_cases as W

SENSITIVITY = 10 * R.LOGIT_TOL
PLAN_IDS = list(R.PLANS)


@pytest.fixture(params=PLAN_IDS)
def plan(request):
    return request.param


def test_profiles_are_what_they_say():
    """the rescales are exact powers of two of the base tensors (biases with their weights), the other profiles touch only the
    tensors they name, every draw is reproducible, and the plans reach both attention kernels"""
    base = R.state_dict("base")
    assert [W.sub_len(R.PLANS[p][0]) for p in PLAN_IDS] == [4, 9] and W.sub_len(R.MAX_CHUNK_FRAMES) == 9
    for name in R.FAMILY_A:
        sd, s = R.state_dict(name), int(name[2:])
        changed = {k for k in sd if sd[k] is not base[k]}
        per_layer = 7 if name.startswith("qk") else 3
        assert len(changed) == per_layer * R.L, (name, len(changed))
        for k in changed:
            ratio = np.unique(sd[k][base[k] != 0] / base[k][base[k] != 0])
            assert ratio.size == 1 and ratio[0] in (2.0 ** s, 2.0 ** -s), (name, k, ratio)
            up = any(n in k for n in ("linear_k", "linear_pos", "linear_out"))
            assert ratio[0] == (2.0 ** s if up else 2.0 ** -s), (name, k)
    for name, keys in (("sharp", 7 * R.L), ("ln_affine", 10 * R.L), ("bn_wide", 2 * R.L), ("outlier", 1)):
        sd = R.state_dict(name)
        assert sum(sd[k] is not base[k] for k in sd) == keys, name
        again = R.PROFILES[name][0](base)
        assert all(np.array_equal(sd[k], again[k]) for k in sd), name
    g = R.state_dict("ln_affine")["encoder.encoders.3.norm_mha.weight"] / base["encoder.encoders.3.norm_mha.weight"]
    assert 0.05 <= g.min() < 0.1 and 3.0 < g.max() <= 6.0 + 1e-5          # two decades
    v = np.concatenate([R.state_dict("bn_wide")[f"encoder.encoders.{i}.conv_module.norm.running_var"] for i in range(R.L)])
    assert 1e-4 <= v.min() < 2e-4 and 5.0 < v.max() <= 10.0
    for p in PLAN_IDS:
        x, xs, xl = R.plan_input("base", p), R.plan_input("silence", p), R.plan_input("loud", p)
        assert not np.array_equal(x[0], x[1])
        lo, hi, val = R.SILENCE
        assert (xs[:, lo:hi] == val).all() and np.array_equal(xs[:, :lo], x[:, :lo]) and np.array_equal(xs[:, hi:], x[:, hi:])
        starts = [c[0] for c in R.plan_of(p)]
        assert any(lo < s < hi for s in starts)                               # the silence crosses a chunk boundary
        assert np.array_equal(xl, x + np.float32(R.LOUD))


@pytest.mark.parametrize("profile", list(R.PROFILES))
def test_float32_baseline(profile, plan):
    """How much of the bars plain float32 uses: the float32 oracle against the float64 oracle on every profile, under a quarter of
    each bar (frames absolute, caches relative to the largest reference value where that exceeds 1)."""
    ref = R.case_ref(profile, plan)
    d, share = R.ref_distance(R.case_ref(profile, plan, 0, torch.float32), ref)
    mag = [max(float(np.abs(r[k]).max()) for r in ref) for k in ("att", "cnn")]
    print(f"{profile} {plan}: float32 oracle vs float64 oracle: frames {d[0]:.3e}, att_cache {d[1]:.3e} (max |ref| {mag[0]:.3g}), "
          f"cnn_cache {d[2]:.3e} (max |ref| {mag[1]:.3g}); largest share of a bar {share.max():.3f}")
    assert np.isfinite(d).all() and share.max() < 0.25, (d, share)


@pytest.mark.parametrize("profile", R.FAMILY_A)
def test_rescales_preserve_the_function(profile, plan):
    """Family A: the float64 frames and cnn_cache equal the base profile's to 1e-9 and the float32 oracle's equal them bitwise
    (the scale factors are exact in both formats), so whatever a mode loses on these weights is lost by the mode."""
    for dtype, exact in ((None, False), (torch.float32, True)):
        got, base = R.case_ref(profile, plan, 0, dtype), R.case_ref("base", plan, 0, dtype)
        for c, (g, b) in enumerate(zip(got, base)):
            for k in ("frames", "cnn"):
                if exact:
                    assert g[k].tobytes() == b[k].tobytes(), (profile, c, k)
                else:
                    assert W.maxdiff(g[k], b[k]) <= 1e-9, (profile, c, k, W.maxdiff(g[k], b[k]))
    s = int(profile[2:])
    if profile.startswith("qk"):
        k, kb = R.case_ref(profile, plan)[-1]["att"][..., :64], R.case_ref("base", plan)[-1]["att"][..., :64]
        assert np.array_equal(k, kb * 2.0 ** s)                                # the cached keys carry the scale


@pytest.mark.parametrize("profile", R.FAMILY_B + R.FAMILY_C)
def test_profiles_move_the_function(profile, plan):
    """Families B and C: the float64 frames differ from the base profile's by at least 10 * LOGIT_TOL, so a kernel that mishandles
    the parameter (a LayerNorm gain, a BatchNorm variance, a sharpened score, an outlier channel, an input level) cannot pass."""
    moved = W.maxdiff(R.ref_frames(profile, plan), R.ref_frames("base", plan))
    print(f"{profile} {plan}: float64 frames move by {moved:.3e} from the base profile's")
    assert moved >= SENSITIVITY, moved


# ---- the split alone -----------------------------------------------------------------------------------------------------------
def test_split_planes_ref():
    """split_planes_ref against the formats: values both planes hold exactly, the f16 lower limit (|x| < 2^-3 leaves a subnormal lo
    plane with an absolute error up to 2^-25), the f16 upper limit, and bf16's 16 significant bits at any magnitude."""
    exact = np.array([0.0, 1.0, -2.5, 1.0 + 2.0 ** -10 + 2.0 ** -20, 1024.0 + 2.0 ** -11], np.float32)
    assert np.array_equal(T.split_planes_ref(exact, "f16"), exact.astype(np.float64))
    g = np.random.Generator(np.random.Philox(key=[7, 7]))
    x = g.standard_normal(4096, dtype=np.float32)
    for s in (0, -3, -9, -13):
        xs = x * np.float32(2.0 ** s)
        e16 = np.abs(T.split_planes_ref(xs, "f16") - xs)
        assert (e16 <= np.maximum(2.0 ** -25, 2.0 ** -22 * np.abs(xs))).all(), (s, e16.max())
        eb = np.abs(T.split_planes_ref(xs, "bf16") - xs)
        assert (eb <= 2.0 ** -17 * np.abs(xs)).all(), s                       # 8 + 8 bits, no lower limit in this range
    assert T.split_error_ref(x, "f16") < 2.0 ** -21 and T.split_error_ref(x * np.float32(2.0 ** -13), "f16") > 2.0 ** -14
    assert T.split_error_ref(x, "bf16") == T.split_error_ref(x * np.float32(2.0 ** -13), "bf16")
    tiny = np.full(8, 3 * 2.0 ** -13, np.float32) * np.float32(1 + 2.0 ** -12)
    assert np.abs(T.split_planes_ref(tiny, "f16") - tiny).max() > 0          # the lo plane cannot hold a residual below 2^-24
    assert T.split_error_ref(np.array([7e4], np.float32), "f16") == np.inf and T.split_error_ref(np.zeros(4, np.float32), "f16") == 0.0
    assert T.split_error_ref(np.array([7e4], np.float32), "bf16") <= 2.0 ** -16


# the issue's table: the frames' distance from float64 through the split of the encoder-block weights alone, length-19 plan
SPLIT_TABLE = {
    "none": ("base", 1.4e-5, 4.3e-6),
    "qk+7": (("qk", 7), 1.4e-5, 1.3e-5), "qk-7": (("qk", -7), 1.4e-5, 1.3e-5),
    "qk+10": ("qk+10", 1.4e-5, 1.3e-4),
    "vo+9": ("vo+9", 1.4e-5, 5.0e-4),
    "vo-9": ("vo-9", 1.4e-5, 1.5e-3),
}


@pytest.mark.parametrize("row", list(SPLIT_TABLE))
def test_split_prediction(row):
    """Every >= 2-D encoder-block weight except the depthwise conv replaced by its hi + lo planes in float64, the float64 oracle run
    on them: the frames' distance from the float64 oracle on the weights themselves reproduces the recorded table to a factor of 2.
    bf16 planes do not notice a power-of-two rescale; f16 planes lose with every halving of a weight below 2^-3, and vo-9 is over
    LOGIT_TOL before any kernel arithmetic is counted."""
    which, want_bf, want_f16 = SPLIT_TABLE[row]
    sd = R.state_dict(which) if isinstance(which, str) else R.rescale(R.state_dict("base"), *which)
    x, want = R.plan_input("base", "19-all")[0], R.ref_frames("base", "19-all")
    got = {}
    for kind in ("bf16", "f16"):
        ref = R.stream_ref(R.split_state_dict(sd, kind), x, "19-all")
        got[kind] = W.maxdiff(np.concatenate([r["frames"] for r in ref], 0), want)
    print(f"split alone, {row}: frames vs float64: bf16 planes {got['bf16']:.2e} (table {want_bf:.1e}), f16 planes {got['f16']:.2e} (table {want_f16:.1e})")
    assert want_bf / 2 <= got["bf16"] <= want_bf * 2 and want_f16 / 2 <= got["f16"] <= want_f16 * 2, got
    if row == "vo-9":
        assert got["f16"] > R.LOGIT_TOL


@pytest.mark.parametrize("profile", ("base",) + R.FAMILY_A + R.FAMILY_B)
def test_f16x3_limit_separates_the_envelope(profile):
    """The limit rnnt_finalize_weights(F16X3) declares (relative r.m.s. error of a GEMM weight's two f16 planes <= 1e-4, |w| <=
    65504), restated on the CPU: nothing in the envelope is refused, every profile beyond it is, and by a tensor the rescale shrank."""
    sd = R.state_dict(profile)
    refused = R.f16x3_refused(sd)
    worst = max((R.f16_split_error(v)[0], k) for k, v in sd.items() if R.is_f16x3_checked(k, v))
    print(f"{profile}: largest f16 split error {worst[0]:.3e} ({worst[1]}), {len(refused)} tensors over the limit {R.F16X3_SPLIT_LIMIT:.0e}")
    if profile in R.FAMILY_A_BEYOND:
        small = {"qk+10": "linear_q", "qk-10": "linear_k", "vo+9": "linear_v", "vo-9": "linear_out"}[profile]
        assert len(refused) == R.L and all(small in k for k, _, _ in refused), refused[:2]
    else:
        assert not refused, refused[:2]
        assert worst[0] <= R.F16X3_SPLIT_LIMIT / 1.5                          # not at the edge of the limit either


@pytest.mark.parametrize("profile", list(R.GREEDY_SEEDS))
def test_greedy_streams_have_a_margin(profile):
    """The streams test_value_range.py decodes: the oracle's smallest top-2 logit margin is at least 1e-3, so a token that differs
    on the device is a bug and not a near-tie, and the stream emits the recorded number of tokens."""
    toks, enc, margin = R.greedy_oracle(profile)
    print(f"{profile} (fbank seed {R.GREEDY_SEEDS[profile]}): {len(toks)} tokens over {enc.shape[1]} frames, smallest top-2 margin {margin:.3e}")
    assert margin >= R.GREEDY_MARGIN and len(toks) == R.GREEDY_TOKENS[profile] > 0
