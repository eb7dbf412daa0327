"""Every launch form of the encoder at its dispatch threshold, against the float64 oracle: rnnt_encoder_full on ragged batches whose
row counts sit just above and just below selM = 1024 (layer and embed GEMMs), conv2 M = 32768 (gemm_bw / gemm_bw_c1) and conv2
M = 2048 (exact-f32 gemm_ns), in the three numerics modes, in a default context and under RNNT_AS=0, RNNT_LM=0 and
RNNT_CONV1_FUSE=0; one wavefront call whose single-descriptor stages take the larger gemm16_tab tiles; and three small cases for
forms no other float64 test dispatches (the ragged call's tail gather / scatter, rel_attention<1>, the 48-row fused half-blocks).
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


def run_wavefront():
    """the wavefront case: one rnnt_encoder_chunks call in an exact-f32 context created under RNNT_LM=0 -> frames [B, 2 t', 256], log"""
    if "wf" not in _RES:
        B, plan = K.WF["B"], K.wf_plan()
        with _env("fp32", "nolm"):
            sb = StreamingBatch(K.state_dict(), B, max_chunk_frames=K.WF["len"] + 1, max_cache_frames=64, max_enc_frames=64, numerics="fp32")
        x = torch.from_numpy(K.wf_input().copy()).cuda().contiguous()
        sb.reset()
        sb.engine.form_log_begin()
        got = sb.engine.encoder_chunks(x.data_ptr(), x.shape[1], *[[p[i] for p in plan] for i in range(4)], _stream())
        torch.cuda.synchronize()
        log = sb.engine.form_log_end()
        assert got == W.plan_frames(plan)[1]
        frames = np.array(sb.engine.enc_frames(_stream()), copy=True)
        sb.engine.close()
        _RES["wf"] = {"frames": frames, "log": log}
    return _RES["wf"]


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
