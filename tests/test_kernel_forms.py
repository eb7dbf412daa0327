"""Every launch form of the encoder at its dispatch threshold, against the float64 oracle: rnnt_encoder_full on ragged batches whose
row counts sit just above and just below selM = 1024 (layer and embed GEMMs), conv2 M = 32768 (gemm_bw / gemm_bw_c1) and conv2
M = 2048 (exact-f32 gemm_ns), in the three numerics modes, in a default context and under RNNT_AS=0, RNNT_LM=0 and
RNNT_CONV1_FUSE=0; one wavefront call whose single-descriptor stages take the larger gemm16_tab tiles; and three small cases for
forms no other float64 test dispatches (the ragged call's tail gather / scatter, rel_attention<1>, the 48-row fused half-blocks);
and the kernel forms, tile maps, stage plans and prefetch depths behind per-context knobs (RNNT_FFN_NW, RNNT_BW_NW, RNNT_GEMM_NS,
RNNT_XCD_X, ...: kernel_forms.KNOB_CASES), each in a context created under its value beside the default context of the same shape.
The launch-form log
(rnnt_form_log_begin / _end) shows which kernels a call dispatched, so a test at a threshold shows that it ran the form it names
(kernel_forms.COVERAGE).  Shapes, references and the coverage table: kernel_forms.py; what the frame bar can see of a wrong tile:
test_kernel_forms_cpu.py.  Needs a real MI355X.  Nothing here provokes a device fault."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
import kernel_forms as K
import window_cases as W
from ctc_vr_amd.lib import RnntEngine
from ctc_vr_amd.online_rnnt_model import StreamingBatch

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(mode, variant):
    """a context reads its knobs at rnnt_create: the mode, materialised encoder frames, and the variant's knobs (every other knob
    of any variant unset)"""
    want = {"RNNT_NUMERICS": mode, "RNNT_FUSE_AFTER_NORM": "0", **{k: None for k in K.KNOBS}, **K.VARIANTS[variant]}
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


_RES = {}


def run_case(pair, side, mode, variant):
    """the case's rnnt_encoder_full call three times on one context -> {"frames": three [B, t', 256] arrays, "log": the form log of
    the first call}"""
    key = (pair, side, mode, variant)
    if key not in _RES:
        B, Tn, tq, lens, _, _ = K.shape(pair, side)
        with _env(mode, variant):
            eng = RnntEngine(max_streams=B, max_chunk_frames=Tn, max_cache_frames=tq + 11, max_enc_frames=8, vocab_size=T.VOCAB, blank_id=T.BLANK)
            eng.load_state_dict(K.state_dict(), numerics=mode)
        xd = torch.from_numpy(K.case_input(pair, side).copy()).cuda().contiguous()
        frames, log, s = [], None, _stream()
        for rep in range(3):
            out = torch.zeros(B, tq, 256, device="cuda")
            if rep == 0:
                eng.form_log_begin()
            assert eng.encoder_full(xd.data_ptr(), np.asarray(lens, np.int32), B, Tn, out.data_ptr(), s) == tq
            torch.cuda.synchronize()
            if rep == 0:
                log = eng.form_log_end()
            frames.append(out.cpu().numpy())
        eng.close()
        _RES[key] = {"frames": frames, "log": log}
    return _RES[key]


def run_wf(kind, mode, variant):
    """one wavefront shape (kernel_forms.wf_cfg) through rnnt_encoder_chunks three times, from a reset each time, on one context
    created under the variant's knobs -> {"frames": three [B, chunks * t', 256] arrays, "log": the form log of the first call}"""
    key = ("wf", kind, mode, variant)
    if key not in _RES:
        cfg, plan = K.wf_cfg(kind), K.wf_kind_plan(kind)
        with _env(mode, variant):
            sb = StreamingBatch(K.state_dict(), cfg["B"], max_chunk_frames=cfg["len"] + 1, max_cache_frames=64, max_enc_frames=64, numerics=mode)
        x = torch.from_numpy(K.wf_kind_input(kind).copy()).cuda().contiguous()
        frames, log, s = [], None, _stream()
        for rep in range(3):
            sb.reset()
            if rep == 0:
                sb.engine.form_log_begin()
            got = sb.engine.encoder_chunks(x.data_ptr(), x.shape[1], *[[p[i] for p in plan] for i in range(4)], s)
            torch.cuda.synchronize()
            if rep == 0:
                log = sb.engine.form_log_end()
            assert got == W.plan_frames(plan)[1]
            frames.append(np.array(sb.engine.enc_frames(s), copy=True))
        sb.engine.close()
        _RES[key] = {"frames": frames, "log": log}
    return _RES[key]


def run_wavefront():
    """the wavefront case: rnnt_encoder_chunks in an exact-f32 context created under RNNT_LM=0 -> frames [B, 2 t', 256], log"""
    r = run_wf("wf", "fp32", "nolm")
    return {"frames": r["frames"][0], "log": r["log"]}


case = pytest.mark.parametrize("pair,side,mode,variant", K.CASES, ids=[K.case_id(*c) for c in K.CASES])


@case
def test_forms_ran(pair, side, mode, variant):
    """the log of the call holds every form the coverage table assigns to this case, and no form the table assigns to the case on
    the other side of the threshold only"""
    cid, other = K.case_id(pair, side, mode, variant), K.case_id(pair, "below" if side == "above" else "above", mode, variant)
    log = run_case(pair, side, mode, variant)["log"]
    print(f"{cid}: {log}")
    want = K.expected_forms(cid)
    assert want, f"the coverage table assigns no form to {cid}"
    assert want <= set(log), (cid, sorted(want - set(log)))
    assert not (K.expected_forms(other) - want) & set(log), (cid, sorted((K.expected_forms(other) - want) & set(log)))


@case
def test_accuracy_vs_float64(pair, side, mode, variant):
    """every stream's valid frames are finite and within LOGIT_TOL of encoder_full in float64; printed: the error on the frames of
    the last partial tile and on the rest, beside the float32 oracle's own distance from float64"""
    got = run_case(pair, side, mode, variant)["frames"][0]
    want, valid = K.case_ref(pair, side)
    f32 = K.case_ref(pair, side, torch.float32)[0]
    B, _, tq, lens, _, _ = K.shape(pair, side)
    assert valid == [K.klen(n) for n in lens] and valid[-1] == tq
    nt = K.tail_frames(pair, side)
    last = [0] * (B - 1) + [tq]                                                # the last stream alone
    tail = K.valid_diff(got[B - 1:], want[B - 1:], [tq], tq - nt)
    rest = max(K.valid_diff(got[:B - 1], want[:B - 1], valid[:B - 1]), K.valid_diff(got[B - 1:], want[B - 1:], [tq], 0, tq - nt))
    print(f"{K.case_id(pair, side, mode, variant)}: max |diff| to float64: last partial tile ({nt} frames of stream {B - 1}) {tail:.3e}, "
          f"the rest {rest:.3e}; float32 oracle {K.valid_diff(f32, want, valid):.3e} (tail {K.valid_diff(f32, want, last, tq - nt):.3e})")
    for b in range(B):
        assert np.isfinite(got[b, :valid[b]]).all(), b
    assert max(tail, rest) <= W.LOGIT_TOL, (tail, rest)


@case
def test_repeatable(pair, side, mode, variant):
    """the same call three times on one context: bit-identical frames (a race in a tile's statistics would show here)"""
    fr = run_case(pair, side, mode, variant)["frames"]
    assert np.array_equal(fr[0], fr[1]) and np.array_equal(fr[0], fr[2])


@case
def test_position_independent(pair, side, mode, variant):
    """streams 0 and B - 1 hold the same audio at the same length: bit-identical valid frames, wherever a row sits in a tile"""
    got = run_case(pair, side, mode, variant)["frames"][0]
    B, _, tq, _, _, _ = K.shape(pair, side)
    d = W.maxdiff(got[0], got[B - 1])
    print(f"{K.case_id(pair, side, mode, variant)}: stream 0 vs stream {B - 1}: max |diff| {d:.3e}")
    assert np.array_equal(got[0, :tq], got[B - 1, :tq])


def test_wavefront_vs_float64():
    """64 streams x two chunks of 67 frames through the wavefront schedule in exact f32: streams 0 and 63 within LOGIT_TOL of
    encoder_stream_ref, and the log holds the gemm16_tab forms the coverage table claims for the single-descriptor stages"""
    r = run_wavefront()
    print(f"{K.WF_ID}: {r['log']}")
    for b in K.WF["streams"]:
        d = W.maxdiff(r["frames"][b], K.wf_ref(b))
        print(f"{K.WF_ID}: stream {b}: max |diff| to float64 {d:.3e}")
        assert np.isfinite(r["frames"][b]).all() and d <= W.LOGIT_TOL, (b, d)
    want = K.expected_forms(K.WF_ID)
    assert any(f.startswith("gemm16_tab") for f in want)
    assert want <= set(r["log"]), sorted(want - set(r["log"]))


# ---- three small cases for forms that no other float64 test dispatches -----------------------------------------------------------------
def _batch(mode, variant, n, chunk, cache=256, enc=256, knobs=None):
    with _env(mode, variant):
        old = {k: os.environ.get(k) for k in (knobs or {})}
        os.environ.update(knobs or {})
        try:
            return StreamingBatch(K.state_dict(), n, max_chunk_frames=chunk, max_cache_frames=cache, max_enc_frames=enc, numerics=mode)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("mode", K.MODES)
def test_ragged_call_vs_float64(mode):
    """rnnt_encode_ragged, three streams whose tail chunks (16, 23 and 20 frames) form three classes: every stream's frames are
    within LOGIT_TOL of its own chunk plan through the float64 oracle; the log holds the gather and scatter launches of the tails"""
    lens, cf = K.RAGGED["lens"], K.RAGGED["chunk"]
    sb, s = _batch(mode, "default", len(lens), 48), _stream()
    x = torch.from_numpy(K.ragged_input().copy()).cuda().contiguous()
    sb.reset()
    sb.engine.form_log_begin()
    fo = sb.engine.encode_ragged(x.data_ptr(), x.shape[1], lens, cf, s)
    torch.cuda.synchronize()
    log = sb.engine.form_log_end()
    enc = np.array(sb.engine.enc_frames(s), copy=True)
    sb.engine.close()
    print(f"ragged-{mode}: {log}")
    for b in range(len(lens)):
        want = K.ragged_ref(b)
        assert int(fo[b]) == want.shape[0], (b, fo[b], want.shape)
        d = W.maxdiff(enc[b, :want.shape[0]], want)
        print(f"ragged-{mode}: stream {b} ({lens[b]} frames -> {want.shape[0]}): max |diff| to float64 {d:.3e}")
        assert np.isfinite(enc[b, :want.shape[0]]).all() and d <= W.LOGIT_TOL, (b, d)
    assert K.expected_forms(f"ragged-{mode}") <= set(log), log


@pytest.mark.parametrize("mode", K.MODES)
def test_tiled_attention_small_chunks_vs_float64(mode):
    """rnnt_encoder_chunk with chunks of t' = 4 in a context created under RNNT_ATTN_STREAM=0: the tiled kernel with one query row
    per wave (rel_attention<1>) instead of the direct-stream kernel, both streams within LOGIT_TOL of float64 after every chunk"""
    case = K.TILED
    plan = W.case_plan(case)
    sb, s = _batch(mode, "default", W.N_STREAMS, W.max_chunk_frames(case[0]), knobs={"RNNT_ATTN_STREAM": "0"}), _stream()
    x = torch.from_numpy(W.case_input(case)).cuda().contiguous()
    sb.reset()
    sb.engine.form_log_begin()
    err = 0.0
    for c, (st, ln, off, req) in enumerate(plan):
        tq = sb.engine.encoder_chunk(x[:, st:st + ln].contiguous().data_ptr(), ln, off, req, s)
        fr = np.array(sb.engine.enc_frames(s), copy=True)
        sb.engine.frames_discard(s)
        assert fr.shape == (W.N_STREAMS, tq, 256) and np.isfinite(fr).all()
        err = max([err] + [W.maxdiff(fr[b], W.case_ref(case, b)[c]["frames"]) for b in range(W.N_STREAMS)])
    log = sb.engine.form_log_end()
    sb.engine.close()
    print(f"attn-tiled-{mode}: {len(plan)} chunks, max |diff| to float64 {err:.3e}; {log}")
    assert err <= W.LOGIT_TOL, err
    assert K.expected_forms(f"attn-tiled-{mode}") <= set(log) and "rel_attention_stream" not in log, log


@pytest.mark.parametrize("mode", K.SPLIT)
def test_fused_wavefront_three_streams_vs_float64(mode):
    """three streams x two chunks of 67 frames through the fused wavefront (RNNT_LM=0): 3 x 16 frames fill the 48-row tile of the
    fused half-blocks (block_front<3> / block_back<3>; two streams stop at <2>); every stream within LOGIT_TOL of float64"""
    B, plan = K.FUSED_WF["B"], K.fused_wf_plan()
    sb, s = _batch(mode, "nolm", B, K.FUSED_WF["len"] + 1, cache=64, enc=64), _stream()
    x = torch.from_numpy(K.fused_wf_input().copy()).cuda().contiguous()
    sb.reset()
    sb.engine.form_log_begin()
    got = sb.engine.encoder_chunks(x.data_ptr(), x.shape[1], *[[p[i] for p in plan] for i in range(4)], s)
    torch.cuda.synchronize()
    log = sb.engine.form_log_end()
    assert got == W.plan_frames(plan)[1]
    fr = np.array(sb.engine.enc_frames(s), copy=True)
    sb.engine.close()
    print(f"wavefront-fused-{mode}: {log}")
    for b in range(B):
        d = W.maxdiff(fr[b], K.fused_wf_ref(b))
        print(f"wavefront-fused-{mode}: stream {b}: max |diff| to float64 {d:.3e}")
        assert np.isfinite(fr[b]).all() and d <= W.LOGIT_TOL, (b, d)
    assert K.expected_forms(f"wavefront-fused-{mode}") <= set(log), log


# ---- the launch-form knobs that were process-static: a context per value, beside the default context of the same shape ---------------
def _forms(cid, log, present=(), absent=()):
    """the log holds the forms the coverage table assigns to the case and the ones named here; no form with one of the `absent`
    prefixes appears"""
    print(f"{cid}: {log}")
    want = K.expected_forms(cid) | set(present)
    assert want <= set(log), (cid, sorted(want - set(log)))
    bad = [f for f in log if f.startswith(tuple(absent))] if absent else []
    assert not bad, (cid, bad)


def _full_knob_case(pair, mode, variant, present=(), absent=()):
    """one rnnt_encoder_full case of kernel_forms.KNOB_FULL: its forms from the log; valid frames finite and within LOGIT_TOL of
    float64; three calls bit-identical; streams 0 and B - 1 bit-identical; and, where the table names a default-knob case, frames
    bit-identical to that case's (printed either way) -> the distance to the default-knob case"""
    case = (pair, "above", mode, variant)
    cid, base = K.KNOB_FULL_IDS[case], K.KNOB_FULL[case]
    r = run_case(*case)
    _forms(cid, r["log"], present, absent)
    fr = r["frames"]
    want, valid = K.case_ref(pair, "above")
    B, _, tq, _, _, _ = K.shape(pair, "above")
    err = K.valid_diff(fr[0], want, valid)
    ref = run_case(pair, "above", mode, base or ("nofuse" if variant.endswith("nofuse") else "default"))["frames"][0]
    dist = K.valid_diff(fr[0], ref, valid)
    print(f"{cid}: max |diff| to float64 {err:.3e}; to the default-knob case {dist:.3e} (bit-identical: {np.array_equal(fr[0], ref)})")
    for b in range(B):
        assert np.isfinite(fr[0][b, :valid[b]]).all(), b
    assert err <= W.LOGIT_TOL, err
    assert np.array_equal(fr[0], fr[1]) and np.array_equal(fr[0], fr[2]), "three calls differ"
    assert np.array_equal(fr[0][0, :tq], fr[0][B - 1, :tq]), "streams 0 and B - 1 differ"
    if base:
        assert np.array_equal(fr[0], ref), (cid, base, dist)
    return dist


def _wf_knob_case(cid, present=(), absent=()):
    """one wavefront case of kernel_forms.KNOB_WF, held as _full_knob_case holds its cases (the twin stream exists in the 64-stream
    shape only; there streams 0, 1, 2 and 63 -- one per 16-row subtile of a 64-row tile -- are held to float64 and all 64 to the
    base context's frames within LOGIT_TOL) -> the result and the distance to the variant it is compared with"""
    kind, mode, variant, base, equal = K.KNOB_WF[cid]
    cfg = K.wf_cfg(kind)
    r = run_wf(kind, mode, variant)
    _forms(cid, r["log"], present, absent)
    fr = r["frames"]
    for b in (K.WF_KNOB_STREAMS if kind == "wf" else range(cfg["B"])):
        d = W.maxdiff(fr[0][b], K.wf_kind_ref(kind, b))
        print(f"{cid}: stream {b}: max |diff| to float64 {d:.3e}")
        assert np.isfinite(fr[0][b]).all() and d <= W.LOGIT_TOL, (b, d)
    assert np.array_equal(fr[0], fr[1]) and np.array_equal(fr[0], fr[2]), "three calls differ"
    if kind == "wf":
        assert np.array_equal(fr[0][0], fr[0][cfg["B"] - 1]), "streams 0 and B - 1 differ"
    dist = None
    if base:
        ref = run_wf(kind, mode, base)["frames"][0]
        dist = W.maxdiff(fr[0], ref)
        print(f"{cid}: max |diff| to {base}, all streams: {dist:.3e} (bit-identical: {np.array_equal(fr[0], ref)})")
        # every stream: finite, and no further from the base context's frames than the bar that holds a context to its reference
        assert np.isfinite(fr[0]).all() and dist <= W.LOGIT_TOL, (cid, base, dist)
        if equal:
            assert np.array_equal(fr[0], ref), (cid, base, dist)
    return r, dist


split = pytest.mark.parametrize("mode", K.SPLIT)


@split
def test_gemm_bw_c1_four_waves(mode):
    """RNNT_BW_NW=4 at 32851 conv2 rows: gemm_bw_c1<4>, no 8-wave form; bit-identical to gemm_bw_c1<8> (the code's claim: a wave
    owns twice the columns, every column's products in the same order)"""
    _full_knob_case("conv2-32768", mode, "bw4", ["gemm_bw_c1<4>"], ["gemm_bw_c1<8>", "gemm_bw<"])


@split
def test_gemm_bw_four_waves(mode):
    """RNNT_BW_NW=4 with RNNT_CONV1_FUSE=0: conv1_relu_rows + gemm_bw<4>, bit-identical to gemm_bw<8>"""
    _full_knob_case("conv2-32768", mode, "bw4-nofuse", ["gemm_bw<4>", "conv1_relu_rows"], ["gemm_bw<8>", "gemm_bw_c1"])


@split
@pytest.mark.parametrize("pair", ["layer-1024", "conv2-2048"])
def test_ffn_as_four_waves(pair, mode):
    """RNNT_FFN_NW=4 at 1028 rows (the last 48-row workgroup holds 20) and at 108: ffn_as<4> for every FFN launch, bit-identical
    to ffn_as<8> (the code's claim)"""
    _full_knob_case(pair, mode, "ffn4", ["ffn_as<4>"], ["ffn_as<8>", "ffn_as<16>"])


@split
@pytest.mark.parametrize("pair", ["layer-1024", "conv2-2048"])
def test_ffn_as_sixteen_waves(pair, mode):
    """RNNT_FFN_NW=16 (1024-thread workgroups, one 16-column tile per wave): ffn_as<16> within LOGIT_TOL of float64 and bit-identical
    to ffn_as<8> (a column's sums do not depend on the wave that owns it: the claim of host_lm.hip.inc)"""
    _full_knob_case(pair, mode, "ffn16", ["ffn_as<16>"], ["ffn_as<8>", "ffn_as<4>"])


@split
def test_conv2_without_gemm_bw(mode):
    """RNNT_CONV2_BW=0: conv2 of 32851 rows with the three-segment A map through launch_gemm (gemm_bf<2,2>, conv1_relu_rows in
    front); no gemm_bw / gemm_bw_c1 launch"""
    _full_knob_case("conv2-32768", mode, "nobw", ["gemm_bf<2,2>", "conv1_relu_rows"], ["gemm_bw"])


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_conv1_relu_at_a_rows_shape(mode):
    """RNNT_CONV1_ROWS=0 at 4 x 1031 frames, where conv1_relu_rows runs by default: conv1_relu, bit-identical frames (both kernels
    form an output from the same nine fmaf in the same order)"""
    _full_knob_case("layer-1024", mode, "norows", ["conv1_relu"], ["conv1_relu_rows"])


@split
def test_attention_exact_f32_in_a_split_mode(mode):
    """RNNT_ATTN_BF=0 at 4 x 111 frames: rel_attention_lm_mfma instead of the 16-bit attention kernels"""
    _full_knob_case("conv2-2048", mode, "attnf32", ["rel_attention_lm_mfma"], ["rel_attention_lm_res", "rel_attention_lm_bf"])


def test_prefetch_depth_one_layer_major():
    """RNNT_GEMM_PD=1 at 1028 rows in exact f32: every gemm_ns launch logs its pd1 name and none its default name"""
    _full_knob_case("layer-1024", "fp32", "pd1", ["gemm_ns<2,2;pd1>", "gemm_ns<1,2;pd1>"], ["gemm_ns<2,2>", "gemm_ns<1,2>"])


def test_prefetch_depth_one_wavefront():
    """RNNT_GEMM_PD=1 in the wavefront case: gemm_ns and gemm_ns_tab under their pd1 names only"""
    _wf_knob_case("wavefront-fp32-nolm-pd1", absent=["gemm_ns<2,2>", "gemm_ns<1,2>", "gemm_ns_tab<1,1,32>", "gemm_ns_tab<1,1,64>", "gemm_ns_tab<1,2,32>"])


def test_gemm_ns_nontemporal():
    """RNNT_CONV2_LDS=2 in the wavefront case (two chunks per subsampling slab, conv2 M = 19456): gemm_ns<2,2,nt>; a non-temporal
    load changes no arithmetic, so the frames are bit-identical to the default context's"""
    _wf_knob_case("wavefront-fp32-nolm-lds2", ["gemm_ns<2,2,nt>"])


def test_gemm_ns_nontemporal_prefetch_depth_one():
    """both knobs: gemm_ns<2,2,nt;pd1>"""
    _wf_knob_case("wavefront-fp32-nolm-lds2-pd1", ["gemm_ns<2,2,nt;pd1>"], ["gemm_ns<2,2,nt>"])


def test_conv2_lds_off():
    """RNNT_CONV2_LDS=0: the exact-f32 conv2 goes through launch_gemm (N = 256 < 512: gemm_ns<1,2>), no gemm_ns<2,2> launch"""
    r, _ = _wf_knob_case("wavefront-fp32-nolm-lds0", ["gemm_ns<1,2>"], ["gemm_ns<2,2"])
    d = run_wavefront()["log"]
    assert r["log"]["gemm_ns<1,2>"] == d["gemm_ns<1,2>"] + d["gemm_ns<2,2>"]                # the conv2 launches moved over, nothing else


def test_gemm16_tab_4_4_4():
    """RNNT_GEMM_NS=0: the two-descriptor stages' ffn w_1 (2 x 1024 x 1024 outputs, K = 256) on gemm16_tab<4,4,4>, no gemm_ns_tab"""
    _wf_knob_case("wavefront-fp32-nolm-ns0", ["gemm16_tab<4,4,4>"], ["gemm_ns_tab"])


def test_gemm16_tab_8_2_4():
    """RNNT_GEMM_NS=0: the two-descriptor stages' ffn w_2 (2 x 1024 x 256 outputs, K = 1024) on gemm16_tab<8,2,4>"""
    _wf_knob_case("wavefront-fp32-nolm-ns0", ["gemm16_tab<8,2,4>"], ["gemm_ns_tab"])


def test_ns_min_groups_one():
    """RNNT_NS_MIN_GROUPS=1: the single-descriptor stages too on gemm_ns_tab, no gemm16_tab launch"""
    _wf_knob_case("wavefront-fp32-nolm-nsmin1", absent=["gemm16_tab"])


@pytest.mark.parametrize("x", [1, 2, 4, 8])
def test_xcd_split_gemm_ns_tab(x):
    """RNNT_XCD_X deals the tiles of gemm_ns_tab to other workgroups: the same launches, bit-identical frames"""
    r, _ = _wf_knob_case(f"wavefront-fp32-nolm-x{x}")
    assert r["log"] == run_wavefront()["log"]


@split
def test_unfused_wavefront_three_streams_vs_float64(mode):
    """FUSED_WF's three streams under RNNT_LM=0 RNNT_FUSED=0: the split-mode stage GEMMs on gemm_bf_tab, no fused half-block"""
    _wf_knob_case(f"wavefront-unfused-{mode}", ["gemm_bf_tab<1,1>", "gemm_bf_tab<1,2>"], ["block_front", "block_back", "gemm_ns_tab", "gemm16_tab"])


@split
@pytest.mark.parametrize("x", [1, 2, 4, 8])
def test_xcd_split_gemm_bf_tab(x, mode):
    """RNNT_XCD_X on gemm_bf_tab: the same launches, frames bit-identical to the context that lets launch_gemm_tab choose X"""
    r, _ = _wf_knob_case(f"wavefront-unfused-{mode}-x{x}", ["gemm_bf_tab<1,1>", "gemm_bf_tab<1,2>"])
    assert r["log"] == run_wf("fwf", mode, "nolm-unfused")["log"]


@split
def test_wf_merge_one(mode):
    """RNNT_WF_MERGE=1 on the unfused three-stream wavefront: the two chunks no longer share a stage, 13 stages instead of 12 (one
    dwconv_bn_silu_tab launch per stage)"""
    r, _ = _wf_knob_case(f"wavefront-unfused-{mode}-merge1")
    assert (run_wf("fwf", mode, "nolm-unfused")["log"]["dwconv_bn_silu_tab"], r["log"]["dwconv_bn_silu_tab"]) == (12, 13)


def test_subsampling_on_the_callers_stream():
    """RNNT_WF_SUB_ASYNC=0: the wavefront's subsampling launches in line instead of on the side stream; the same launches, same bits"""
    r, _ = _wf_knob_case("wavefront-fp32-nolm-subsync")
    assert r["log"] == run_wavefront()["log"]


def test_attention_head_major():
    """RNNT_ATTN_PAIR_MAJOR=0 in the 64-stream wavefront case: its chunks of t' = 16 take the tiled table kernel, which the knob does
    not reach -- the same launches, and (asserted by the case table) the same bits"""
    r, _ = _wf_knob_case("wavefront-fp32-nolm-apm0", ["rel_attention_tab<4>"], ["rel_attention_stream_tab"])
    assert r["log"] == run_wavefront()["log"]


def test_attention_head_major_direct_stream():
    """RNNT_ATTN_PAIR_MAJOR=0 where it acts: three streams x 8 chunks of t' = 4 in exact f32, whose stages run
    rel_attention_stream_tab with its workgroups head-major instead of pair-major; the same launches as the default order"""
    r, _ = _wf_knob_case("wavefront-t4-fp32-nolm-apm0", ["rel_attention_stream_tab"])
    assert r["log"] == _wf_knob_case("wavefront-t4-fp32-nolm", ["rel_attention_stream_tab"])[0]["log"]


@split
@pytest.mark.parametrize("variant", list(K.FUSE_PLANS))
def test_fuse_knobs_move_the_stage_plan(variant, mode):
    """RNNT_FUSE_MERGE / RNNT_FUSE_FRAMES on three streams x 8 chunks of t' = 4: 1, 2, 3 (default) or 4 chunks of a layer per
    fused stage -> 19, 15, 14 or 13 block_front and block_back launches, the full stages with 1, 2, 3 or 3 row tiles"""
    cid = f"fuse-knobs-{mode}" + ("" if variant == "nolm" else "-" + variant[5:])
    r, _ = _wf_knob_case(cid)
    stages, mt = K.fuse_launches(variant)
    for k in ("block_front", "block_back"):
        n = {f: c for f, c in r["log"].items() if f.startswith(k)}
        assert sum(n.values()) == stages and f"{k}<{mt}>" in n, (cid, n, stages, mt)
