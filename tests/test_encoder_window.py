"""The streaming encoder under every window policy of (offset, required_cache_size), against the float64 oracle
(testing.encoder_stream_ref): rnnt_encoder_chunk chunk by chunk, rnnt_encoder_chunks under its schedules, two whole-utterance
calls back to back, the stream pool with a different policy per slot, the linear K/V buffer's capacity and refusals, and two
small full-context shapes.  The plans (window_cases.py) saturate the window, move it beyond row 64 of the K/V buffer and wrap the
conv ring twice; test_encoder_window_cpu.py shows that a window, positional or conv off-by-one moves the frames by >= 10x the bar.
Needs a real MI355X.  Nothing here provokes a device fault: every refusal is a host-side argument check."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
import window_cases as W
from ctc_vr_amd.lib import ERR_SHAPE, RnntError
from ctc_vr_amd.online_rnnt_model import StreamingBatch

pytestmark = pytest.mark.gpu

MODES = ["fp32", "bf16x3", "f16x3"]
VARIANTS = {"default": {}, "noresident": {"RNNT_ATTN_RESIDENT": "0"}, "nolm": {"RNNT_LM": "0"}, "nolm_nofused": {"RNNT_LM": "0", "RNNT_FUSED": "0"}}
KNOBS = sorted({k for v in VARIANTS.values() for k in v})
FUSE_MAXF = 16                                         # frames of one stream a fused half-block tile holds (rnnt_fused.hip.h)


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


def _batch(mode, length, variant="default", n=W.N_STREAMS, cache=256, enc=256, chunk=None):
    with _env(mode, variant):
        return StreamingBatch(W.state_dict(), n, max_chunk_frames=chunk or W.max_chunk_frames(length), max_cache_frames=cache, max_enc_frames=enc,
                              numerics=mode)


def _cases_of(length):
    return [c for c in W.CASES if c[0] == length] + ([W.RAGGED] if length == W.RAGGED[0] else [])


def _x_dev(case, n=W.N_STREAMS):
    return torch.from_numpy(W.case_input(case, n)).cuda().contiguous()


def _caches(eng, n):
    s = _stream()
    return [eng.att_cache(b, s) for b in range(n)], [eng.cnn_cache(b, s) for b in range(n)]


def _drive_chunks(sb, x, plan, refs=None):
    """rnnt_encoder_chunk chunk by chunk from the context's present position; after every chunk the new frames and both caches of
    every stream are read (and the frames discarded).  refs[b] (encoder_stream_ref results): the largest distances are kept
    and every att_cache shape is checked.  -> {"frames" [B, F, 256], "att", "cnn" (per stream, after the last chunk), "err"}"""
    eng, s, n = sb.engine, _stream(), sb.n
    frames, err = [], np.zeros(3)
    for c, (st, ln, off, req) in enumerate(plan):
        xc = x[:, st:st + ln].contiguous()
        tq = eng.encoder_chunk(xc.data_ptr(), ln, off, req, s)
        fr = np.array(eng.enc_frames(s), copy=True)
        assert fr.shape == (n, tq, 256) and tq == W.sub_len(ln)
        eng.frames_discard(s)
        att, cnn = _caches(eng, n)
        for b in range(n if refs is not None else 0):
            r = refs[b][c]
            assert att[b].shape == r["att"].shape, (c, b, att[b].shape, r["att"].shape)
            err = np.maximum(err, [W.maxdiff(fr[b], r["frames"]), W.maxdiff(att[b], r["att"]), W.maxdiff(cnn[b], r["cnn"])])
        frames.append(fr)
    return {"frames": np.concatenate(frames, 1), "att": att, "cnn": cnn, "err": err}


_RES = {}


def _per_chunk(mode, case):
    """one case through the per-chunk API in a default context, checked against float64 after every chunk -> _drive_chunks result"""
    key = ("chunk", mode, case)
    if key not in _RES:
        sb = _batch(mode, case[0])
        sb.reset()
        _RES[key] = _drive_chunks(sb, _x_dev(case), W.case_plan(case), [W.case_ref(case, b) for b in range(W.N_STREAMS)])
        sb.engine.close()
    return _RES[key]


def _whole(mode, length, variant):
    """every case of one chunk length through ONE rnnt_encoder_chunks call each, in a context created under the variant's knobs
    -> {case: {"frames", "att", "cnn", "launches"}}"""
    key = ("whole", mode, length, variant)
    if key not in _RES:
        sb, out, s = _batch(mode, length, variant), {}, _stream()
        for case in _cases_of(length):
            plan, x = W.case_plan(case), _x_dev(case)
            sb.reset()
            l0 = sb.engine.counters()[0]
            got = sb.engine.encoder_chunks(x.data_ptr(), x.shape[1], *[[p[i] for p in plan] for i in range(4)], s)
            assert got == W.plan_frames(plan)[1]
            att, cnn = _caches(sb.engine, sb.n)
            out[case] = {"frames": np.array(sb.engine.enc_frames(s), copy=True), "att": att, "cnn": cnn, "launches": sb.engine.counters()[0] - l0}
        sb.engine.close()
        _RES[key] = out
    return _RES[key]


def _ref_frames(case, b):
    return np.concatenate([r["frames"] for r in W.case_ref(case, b)], 0)


def _vs_ref(res, case):
    """distance of a whole run (frames of all chunks, caches after the last) from the float64 oracle, over the streams"""
    d = np.zeros(3)
    for b in range(W.N_STREAMS):
        last = W.case_ref(case, b)[-1]
        assert res["att"][b].shape == last["att"].shape, (case, b, res["att"][b].shape)
        d = np.maximum(d, [W.maxdiff(res["frames"][b], _ref_frames(case, b)), W.maxdiff(res["att"][b], last["att"]), W.maxdiff(res["cnn"][b], last["cnn"])])
    return d


def _vs_run(a, b):
    return max([W.maxdiff(a["frames"], b["frames"])] + [W.maxdiff(x, y) for k in ("att", "cnn") for x, y in zip(a[k], b[k])])


def _same(a, b):
    return np.array_equal(a["frames"], b["frames"]) and all(np.array_equal(x, y) for k in ("att", "cnn") for x, y in zip(a[k], b[k]))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES + [W.RAGGED], ids=W.case_id)
def test_per_chunk_api_vs_float64(numerics, case):
    """rnnt_encoder_chunk chunk by chunk, two streams with different audio: after EVERY chunk the new frames, att_cache (shape and
    value) and cnn_cache of each stream are within LOGIT_TOL of that stream's float64 oracle.  The exact-f32 run also prints the
    float32 oracle's own distance from the float64 oracle (the share of the bar that float32 arithmetic uses by itself)."""
    r = _per_chunk(numerics, case)
    print(f"[{numerics}] per-chunk {W.case_id(case)} ({len(W.case_plan(case))} chunks): max |diff| to float64: frames {r['err'][0]:.3e}, "
          f"att_cache {r['err'][1]:.3e}, cnn_cache {r['err'][2]:.3e}")
    if numerics == "fp32":
        d = W.ref_distance(W.case_ref(case, 0, torch.float32), W.case_ref(case, 0))
        print(f"    float32 oracle vs float64 oracle (stream 0): frames {d[0]:.3e}, att_cache {d[1]:.3e}, cnn_cache {d[2]:.3e}")
    assert r["err"].max() <= W.LOGIT_TOL, (case, r["err"])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("length", W.LENGTHS)
def test_whole_utterance_call_vs_float64(numerics, length, variant):
    """The same plans through one rnnt_encoder_chunks call: layer-major by default (resident attention in the split modes), with
    RNNT_ATTN_RESIDENT=0, with RNNT_LM=0 (wavefront, fused half-blocks in the split modes up to 16 frames per chunk) and with
    RNNT_LM=0 RNNT_FUSED=0.  Each stays within LOGIT_TOL of float64 and within SCHED_TOL of the per-chunk API's frames and caches.
    That the intended schedule ran shows in the launch counts of the call (layer-major: independent of the chunk count; wavefront:
    3 or 11 launches per stage) and, for the resident attention, in frames that are close to but not bit-equal to the knob-off run.
    R = 0 on every chunk restarts the cache at row 0 each time, which the layer-major schedule cannot run (lm_plan): it goes
    through the wavefront schedule whatever the knob says, and must still be right."""
    split = numerics != "fp32"
    chunk = {case: _per_chunk(numerics, case) for case in _cases_of(length)}
    base = _whole(numerics, length, "default")
    run = _whole(numerics, length, variant)
    nolm = _whole(numerics, length, "nolm") if variant == "nolm_nofused" else None
    res_differs = []
    for case in _cases_of(length):
        r = run[case]
        d = _vs_ref(r, case)
        step = _vs_run(r, chunk[case])
        print(f"[{numerics}] whole-utterance {variant} {W.case_id(case)}: {r['launches']} launches; max |diff| to float64: frames {d[0]:.3e}, "
              f"att_cache {d[1]:.3e}, cnn_cache {d[2]:.3e}; to the per-chunk API {step:.3e}")
        assert d.max() <= W.LOGIT_TOL, (case, d)
        assert step <= W.SCHED_TOL, (case, step)
        lm_can_run = case[1] != "zero"
        if variant == "noresident":
            assert r["launches"] == base[case]["launches"]
            if not split or not lm_can_run:
                assert _same(r, base[case]), case                     # the knob only chooses between two split-mode kernels of the layer-major schedule
            elif case[1] in ("all", "r64", "off"):
                res_differs.append(not _same(r, base[case]))
        elif variant == "nolm":
            if lm_can_run:
                assert r["launches"] > base[case]["launches"], (case, r["launches"], base[case]["launches"])
            else:
                assert r["launches"] == base[case]["launches"] and _same(r, base[case]), case      # the default fell back to the wavefront
        elif variant == "nolm_nofused":
            if split and W.sub_len(length) <= FUSE_MAXF:
                assert r["launches"] > nolm[case]["launches"], (case, r["launches"], nolm[case]["launches"])
            else:
                assert r["launches"] == nolm[case]["launches"] and _same(r, nolm[case]), case      # exact f32 and chunks of 17 frames: unfused anyway
    if res_differs:
        assert any(res_differs), "RNNT_ATTN_RESIDENT=0 changed nothing: the resident kernel did not run in the default context"


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["default", "nolm"])
@pytest.mark.parametrize("case", [(23, "two"), (19, "r64")], ids=W.case_id)
def test_continuation_of_a_whole_utterance_call(numerics, case, variant):
    """Two rnnt_encoder_chunks calls back to back on one utterance, the frames decoded and consumed in between: the second call
    starts at a non-zero cache_len, kv_start and conv_pos.  Frames and caches equal one call over all chunks to SCHED_TOL and
    float64 to LOGIT_TOL."""
    one = _whole(numerics, case[0], variant)[case]
    sb, s, plan, x = _batch(numerics, case[0], variant), _stream(), W.case_plan(case), _x_dev(case)
    cut = len(plan) // 2 + 1
    assert W.walk(plan)[cut]["kv_row0"] > 0 and W.walk(plan)[cut]["ring_pos"] > 0
    sb.reset()
    parts = []
    for part in (plan[:cut], plan[cut:]):
        got = sb.engine.encoder_chunks(x.data_ptr(), x.shape[1], *[[p[i] for p in part] for i in range(4)], s)
        assert got == W.plan_frames(part)[1]
        parts.append(np.array(sb.engine.enc_frames(s), copy=True))
        sb.engine.greedy_decode(s)
        sb.engine.frames_consume(s)
    att, cnn = _caches(sb.engine, sb.n)
    two = {"frames": np.concatenate(parts, 1), "att": att, "cnn": cnn}
    sb.engine.close()
    d, step = _vs_ref(two, case), _vs_run(two, one)
    print(f"[{numerics}] continuation {variant} {W.case_id(case)}: max |diff| to float64 {d.max():.3e}, to one call {step:.3e}")
    assert d.max() <= W.LOGIT_TOL and step <= W.SCHED_TOL, (d, step)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
POOL_LEN, POOL_POLICIES, POOL_OPEN = 19, ("all", "one", "r64"), (0, 3, 7)


def _pool_refs():
    if "pool" not in _RES:
        plans = [W.make_plan(POOL_LEN, p, W.n_chunks_for(POOL_LEN, "r64")) for p in POOL_POLICIES]
        x = T.synth_fbank(3, W.plan_frames(plans[0])[0], seed=4321)
        _RES["pool"] = (plans, x, [T.encoder_stream_ref(W.state_dict(), x[i], plans[i]) for i in range(3)])
    return _RES["pool"]


def _pool_run(sb, slots, refs=None):
    """slot i opens at step POOL_OPEN[i] and then takes one chunk per call under its own policy -> per slot the frames of its
    chunks and its caches after its last chunk (+ the largest distances from refs, checked after every call)"""
    plans, x, _ = _pool_refs()
    eng, s = sb.engine, _stream()
    xd = torch.from_numpy(x).cuda()
    sb.reset()
    out = {i: {"frames": [], "err": np.zeros(3)} for i in slots}
    for step in range(max(POOL_OPEN) + len(plans[0])):
        for i in slots:
            if POOL_OPEN[i] == step:
                eng.stream_open(i, s)
        act = [i for i in slots if 0 <= step - POOL_OPEN[i] < len(plans[i])]
        if not act:
            continue
        ch = [plans[i][step - POOL_OPEN[i]] for i in act]
        rows = torch.stack([xd[i, c[0]:c[0] + c[1]] for i, c in zip(act, ch)], 0).contiguous()
        tq = eng.pool_chunk(act, rows.data_ptr(), POOL_LEN, [c[2] for c in ch], [c[3] for c in ch], False, s)
        fr = np.array(eng.enc_frames(s), copy=True)
        assert fr.shape[1] == tq == W.sub_len(POOL_LEN)
        eng.frames_discard(s)
        for i in act:
            out[i]["frames"].append(fr[i])
            out[i]["att"], out[i]["cnn"] = eng.att_cache(i, s), eng.cnn_cache(i, s)
            if refs is not None:
                r = refs[i][step - POOL_OPEN[i]]
                assert out[i]["att"].shape == r["att"].shape, (i, step)
                out[i]["err"] = np.maximum(out[i]["err"], [W.maxdiff(fr[i], r["frames"]), W.maxdiff(out[i]["att"], r["att"]), W.maxdiff(out[i]["cnn"], r["cnn"])])
    for i in slots:
        out[i]["frames"] = np.concatenate(out[i]["frames"], 0)
    return out


def test_pool_slots_hold_different_policies(numerics):
    """One rnnt_pool_chunk sequence, three slots opened at steps 0, 3 and 7, holding R = -1, R = t' and R = 64 in the same calls:
    after every call each slot's frames and caches are within LOGIT_TOL of its own float64 stream, and each slot is bitwise the
    same slot run alone."""
    plans, _, refs = _pool_refs()
    for p, plan in zip(POOL_POLICIES, plans):
        last = W.walk(plan)[-1]
        assert last["ring_pos"] >= 2 * W.ring_cap(POOL_LEN) and (p == "all" or last["kv_row0"] > 64)
    sb = _batch(numerics, POOL_LEN, n=3)
    busy = _pool_run(sb, [0, 1, 2], refs)
    for i in range(3):
        print(f"[{numerics}] pool slot {i} (R {POOL_POLICIES[i]}): max |diff| to float64: frames {busy[i]['err'][0]:.3e}, att_cache {busy[i]['err'][1]:.3e}, "
              f"cnn_cache {busy[i]['err'][2]:.3e}")
        assert busy[i]["err"].max() <= W.LOGIT_TOL, (i, busy[i]["err"])
    for i in range(3):
        alone = _pool_run(sb, [i])[i]
        for k in ("frames", "att", "cnn"):
            assert alone[k].shape == busy[i][k].shape and alone[k].tobytes() == busy[i][k].tobytes(), f"slot {i}: {k} differs from the slot run alone"
    sb.engine.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _refused(call):
    with pytest.raises(RnntError) as e:
        call()
    assert e.value.status == ERR_SHAPE, (e.value.status, str(e.value))


def _assert_state(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} changed"


def test_linear_buffer_capacity_and_refusals(numerics):
    """A bounded window (R = t' = 4) still slides through a linear K/V buffer: with max_cache_frames = 40 the chunk that would
    write rows [40, 44) is refused with RNNT_ERR_SHAPE by rnnt_encoder_chunk, rnnt_encoder_chunks and rnnt_pool_chunk, and so is
    a chunk whose offset is smaller than the cache length.  A refusal leaves frames, both caches and tokens bitwise as they were;
    rnnt_streams_reset / rnnt_stream_open make the stream usable again, and right against float64."""
    case, cap = (19, "one"), 40
    plan, x, s = W.case_plan(case), _x_dev(case), _stream()
    fits = cap // 4
    assert all(k["kv_row0"] + k["T2"] <= cap for k in W.walk(plan)[:fits]) and W.walk(plan)[fits]["kv_row0"] + W.walk(plan)[fits]["T2"] == cap + 4
    sb = _batch(numerics, 19, cache=cap, enc=64)
    eng = sb.engine
    over, four = plan[fits], [[plan[fits][i]] for i in range(4)]
    xo = x[:, over[0]:over[0] + over[1]].contiguous()
    # lock step: the frames stay buffered, the tokens come from a greedy decode of them
    sb.reset()
    for st, ln, off, req in plan[:fits]:
        eng.encoder_chunk(x[:, st:st + ln].contiguous().data_ptr(), ln, off, req, s)
    eng.greedy_decode(s)

    def lock_state():
        att, cnn = _caches(eng, sb.n)
        toks = eng.tokens(s)
        return {"frames": np.array(eng.enc_frames(s), copy=True), **{f"att{b}": att[b] for b in range(sb.n)}, **{f"cnn{b}": cnn[b] for b in range(sb.n)},
                **{f"tokens{b}": np.asarray(toks[b], np.int32) for b in range(sb.n)}}

    before = lock_state()
    assert before["frames"].shape[1] == cap and before["att0"].shape[2] == 4
    for call in (lambda: eng.encoder_chunk(xo.data_ptr(), over[1], over[2], over[3], s),
                 lambda: eng.encoder_chunks(x.data_ptr(), x.shape[1], *four, s),
                 lambda: eng.encoder_chunk(xo.data_ptr(), over[1], 3, over[3], s),                     # offset 3 < cache_len 4
                 lambda: eng.encoder_chunks(x.data_ptr(), x.shape[1], four[0], four[1], [3], four[3], s)):
        _refused(call)
        _assert_state(before, lock_state(), "lock-step state after a refused chunk")
    sb.reset()
    again = _drive_chunks(sb, x, plan[:fits], [W.case_ref(case, b) for b in range(W.N_STREAMS)])
    assert again["err"].max() <= W.LOGIT_TOL, again["err"]
    # stream pool: slot 1 alone, greedy calls
    sb.reset()
    eng.stream_open(1, s)
    for st, ln, off, req in plan[:fits]:
        eng.pool_chunk([1], x[1:2, st:st + ln].contiguous().data_ptr(), ln, [off], [req], True, s)

    def pool_state():
        return {"att": eng.att_cache(1, s), "cnn": eng.cnn_cache(1, s), "tokens": np.asarray(eng.stream_tokens(1, 0, s), np.int32)}

    before = pool_state()
    assert before["att"].shape[2] == 4
    for off in (over[2], 3):
        _refused(lambda: eng.pool_chunk([1], xo[1:2].contiguous().data_ptr(), over[1], [off], [over[3]], True, s))
        _assert_state(before, pool_state(), "slot state after a refused pool chunk")
    eng.stream_open(1, s)
    ref = W.case_ref(case, 1)
    for c, (st, ln, off, req) in enumerate(plan[:3]):
        eng.pool_chunk([1], x[1:2, st:st + ln].contiguous().data_ptr(), ln, [off], [req], False, s)
        fr = np.array(eng.enc_frames(s), copy=True)[1]
        eng.frames_discard(s)
        assert max(W.maxdiff(fr, ref[c]["frames"]), W.maxdiff(eng.att_cache(1, s), ref[c]["att"]), W.maxdiff(eng.cnn_cache(1, s), ref[c]["cnn"])) <= W.LOGIT_TOL
    eng.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,lens", [(7, [7]), (47, [47, 46, 23, 7])], ids=["T7", "T47"])
def test_full_context_small_shapes(numerics, frames, lens):
    """rnnt_encoder_full at t' = 1 and on a ragged batch whose lengths fall on both sides of the subsampled mask's rounding (47 and
    46 frames -> 11 and 10 valid frames) with one stream of a single valid key: the valid frames are within LOGIT_TOL of
    encoder_full in float64, and their count is the oracle mask's."""
    from oracle import rnnt_oracle as O
    n, tq = len(lens), W.sub_len(frames)
    x = T.synth_fbank(n, frames, seed=4700 + frames)
    with torch.no_grad():
        want, mask = O.encoder_full(T.ref_state_dict(W.state_dict()), torch.from_numpy(x).double(), torch.tensor(lens))
    valid = mask[:, 0].sum(1).tolist()
    assert valid == [((ln - 1) // 2 - 1) // 2 for ln in lens] and tuple(want.shape) == (n, tq, 256)      # the library's klen (rnnt_encoder_full)
    sb = _batch(numerics, frames, n=n, cache=64, enc=16, chunk=frames)
    out = torch.empty(n, tq, 256, device="cuda")
    assert sb.engine.encoder_full(torch.from_numpy(x).cuda().contiguous().data_ptr(), lens, n, frames, out.data_ptr(), _stream()) == tq
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sb.engine.close()
    for b in range(n):
        err = W.maxdiff(got[b, :valid[b]], want[b, :valid[b]].numpy())
        print(f"[{numerics}] full context T={frames} stream {b} ({valid[b]} valid frames): max |diff| to float64 {err:.3e}")
        assert np.isfinite(got[b, :valid[b]]).all() and err <= W.LOGIT_TOL, (b, err)
