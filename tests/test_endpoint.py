"""Endpoint detection per slot of the stream pool on the device (rnnt_ctc_blank_logprob, rnnt_stream_endpoint, rnnt_pool_endpoint_frames,
rnnt_pool_get_endpoints, the hook in the pool calls).  Needs a real MI355X: `pytest -m gpu`.

A. the blank log-posterior against float64 within the project's LOGIT_TOL (largest error seen: see DESIGN.md section 7);
B. the seam on rows whose class is beyond doubt: device state == the Python restatement, exactly, whatever the split;
C. through the pool calls on the case of endpoint_cases.py (its conditions are asserted on the oracle in test_endpoint_cpu.py): after
   every step the states equal the host twin run on the float64 oracle's posteriors, the greedy tokens are those of a run without
   endpointing, and a call costs exactly one launch more when -- and only when -- it lists an endpoint slot;
D. lifecycle, E. refusals.  Nothing here provokes a device fault: every refusal is a host-side argument check."""
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import RnntEngine, RnntError
from ctc_vr_amd.online_rnnt_model import EndpointConfig, StreamPool

import endpoint_cases as C

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3                  # the project's logits bar (test_gpu_parity.py)
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
V, BLANK = T.VOCAB, T.BLANK
SENTINEL = 1234.5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _status(fn, *a):
    with pytest.raises(RnntError) as e:
        fn(*a)
    return e.value.status


# ---- A. rnnt_ctc_blank_logprob -----------------------------------------------------------------------------------------------------
BLANK_ROWS = [1, 3, 15, 16, 17, 64, 961]
# test_decode_edges.py's vocabularies for rnnt_ctc_logprobs, the blank first, last and in the middle
BLANK_CFGS = [(6, 0), (6, 5), (6, 3), (412, 0), (412, 411), (412, 5), (413, 206), (4336, 0), (4336, 4335), (4336, 2168)]
_SEEN = {"max": 0.0}


def _head_engine(v, blank, mode="fp32"):
    sd = T.make_state_dict(0, vocab=v, blank=blank)
    eng = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=32, max_enc_frames=16, max_tokens=64, vocab_size=v, blank_id=blank)
    eng.load_state_dict(sd, numerics=mode)
    return eng, sd


def _blank_ref(sd, enc, blank):
    w, b = (torch.from_numpy(sd[n]).cuda().double() for n in ("ctc_head.ctc_lo.weight", "ctc_head.ctc_lo.bias"))
    return torch.log_softmax(enc.double() @ w.T + b, dim=-1)[:, blank]


def _blank_run(eng, enc):
    rows = enc.size(0)
    buf = torch.full((rows + 256,), float("nan"), device="cuda")
    buf[rows:] = SENTINEL
    eng.ctc_blank_logprob(enc.data_ptr(), rows, buf.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool((buf[rows:] == SENTINEL).all())              # nothing written behind the output
    assert bool(torch.isfinite(buf[:rows]).all())            # every element written
    return buf[:rows]


@pytest.mark.parametrize("cfg", BLANK_CFGS, ids=lambda c: f"V{c[0]}_blank{c[1]}")
def test_blank_logprob_vs_float64(cfg):
    v, blank = cfg
    eng, sd = _head_engine(v, blank)
    try:
        worst = 0.0
        for rows in BLANK_ROWS:
            base = torch.randn(rows, 256, generator=torch.Generator().manual_seed(rows + v)).cuda()
            for scale in (1.0, 30.0):                        # x 30: logits reach tens, the max-subtraction matters
                enc = (base * scale).contiguous()
                ref = _blank_ref(sd, enc, blank)
                d = float((_blank_run(eng, enc).double() - ref).abs().max())
                worst = max(worst, d)
                assert d < LOGIT_TOL, (rows, scale, d)
        _SEEN["max"] = max(_SEEN["max"], worst)
        print(f"rnnt_ctc_blank_logprob V={v} blank={blank}: max |diff| to float64 {worst:.3e} (so far over all cases {_SEEN['max']:.3e})")
    finally:
        eng.close()


def test_blank_logprob_is_f32_in_every_mode_and_matches_logprobs():
    """the same bits in every numerics mode (decode arithmetic is f32 everywhere), and within LOGIT_TOL of column `blank` of
    rnnt_ctc_logprobs"""
    enc = (torch.randn(83, 256, generator=torch.Generator().manual_seed(7)) * 5).cuda()
    outs = []
    for mode in PARITY_MODES:
        eng, _ = _head_engine(V, BLANK, mode)
        try:
            outs.append(_blank_run(eng, enc).clone())
            if mode == "fp32":
                full = torch.empty(83, V, device="cuda")
                eng.ctc_logprobs(enc.data_ptr(), 83, full.data_ptr(), _stream())
                torch.cuda.synchronize()
                assert float((full[:, BLANK] - outs[0]).abs().max()) < LOGIT_TOL
                # a frame's value does not depend on its place in a call, nor on the tile form that took it (4 or 16 frames)
                assert torch.equal(_blank_run(eng, enc[:3].contiguous()), outs[0][:3])
                assert torch.equal(_blank_run(eng, enc[18:22].contiguous()), outs[0][18:22])
                assert torch.equal(_blank_run(eng, enc[5:40].contiguous()), outs[0][5:40])
        finally:
            eng.close()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ---- B. the seam -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_engine(np_state_dict):
    eng = RnntEngine(max_streams=6, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=16, max_tokens=256, vocab_size=V, blank_id=BLANK)
    eng.load_state_dict(np_state_dict(0), numerics="fp32")
    yield eng
    eng.close()


ALPHA = 40.0
SEAM_THR = 0.5
# slot -> (config, pattern of 23 frames: 1 blank, 0 speech); slot 4 is listed in no call of the comparison, slot 5 has no endpointing
SEAM = {
    0: ((SEAM_THR, 1, 4, 2, 0), "11111110110001111100011"),      # rule 1 at frame 4
    1: ((SEAM_THR, 2, 3, 3, 0), "01101110001111111101111"),      # rule 2 at frame 7 (speech reaches 2 at frame 4)
    2: ((0.9, 1, 0, 0, 18), "01010101010101010101010"),          # rule 3 at frame 18, in a later tile of a 23-frame call
    3: ((0.1, 3, 0, 0, 0), "11100011100011100011100"),           # all rules off: the slot only counts
}
SEAM_T = 23


def _seam_rows(np_state_dict, slots):
    """[len(slots), 23, 256] rows +-ALPHA * W[blank], and the check that their class is beyond doubt under every threshold used"""
    sd = np_state_dict(0)
    wb = torch.from_numpy(sd["ctc_head.ctc_lo.weight"][BLANK])
    sign = torch.tensor([[1.0 if ch == "1" else -1.0 for ch in SEAM[s][1]] for s in slots])
    rows = (sign[:, :, None] * ALPHA * wb[None, None, :]).contiguous().cuda()
    lp = _blank_ref(sd, rows.view(-1, 256), BLANK).view(len(slots), SEAM_T).cpu()
    for thr in (0.1, 0.5, 0.9):
        assert float((lp - math.log(thr)).abs().min()) > 0.1     # 100 x LOGIT_TOL from every threshold
        assert torch.equal(lp > math.log(thr), sign > 0)
    return rows


def _seam_open(eng, slots=(0, 1, 2, 3, 4)):
    s = _stream()
    eng.reset(6, s)
    for slot in range(6):
        eng.stream_open(slot, s)
    for slot in slots:
        eng.stream_endpoint(slot, SEAM[slot][0] if slot in SEAM else (0.5, 1, 2, 2, 2), s)


def _seam_expected(slot, upto=SEAM_T):
    return C.scan_ref([1.0 if ch == "1" else -50.0 for ch in SEAM[slot][1][:upto]], (0.5,) + SEAM[slot][0][1:])   # class in, class out


def test_seam_states_exact_whatever_the_split(seam_engine, np_state_dict):
    eng, s = seam_engine, _stream()
    slots = [2, 0, 3, 1]                                        # per-slot configs that differ within one call, rows not in slot order
    rows = _seam_rows(np_state_dict, slots)
    want = np.asarray([_seam_expected(x) for x in slots], np.int32)
    assert sorted(want[:, 3].tolist()) == [0, 1, 2, 3]          # every rule, and none
    assert want[slots.index(0)].tolist()[3:] == [1, 4] and want[slots.index(1)].tolist()[3:] == [2, 7] and want[slots.index(2)].tolist()[3:] == [3, 18]
    got = {}
    for split in ("one", "ones", "3+rest"):
        _seam_open(eng)
        other = torch.full((1, 5, 256), 0.25, device="cuda")
        eng.pool_endpoint_frames([4], other.data_ptr(), 5, s)    # slot 4 moves first and is then left alone
        before4 = eng.pool_endpoints([4], s).copy()
        cuts = {"one": [0, SEAM_T], "ones": list(range(SEAM_T + 1)), "3+rest": [0, 3, SEAM_T]}[split]
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = rows[:, a:b].contiguous()
            eng.pool_endpoint_frames(slots, part.data_ptr(), b - a, s)
            if split == "3+rest" and b == 3:                     # mid-way: the state after 3 frames
                assert (eng.pool_endpoints(slots, s) == np.asarray([_seam_expected(x, 3) for x in slots], np.int32)).all()
        got[split] = eng.pool_endpoints(slots, s).copy()
        assert (got[split] == want).all(), (split, got[split], want)
        assert (eng.pool_endpoints([4], s) == before4).all() and before4[0, 0] == 5      # the unlisted slot is bitwise unchanged
    assert (got["one"] == got["ones"]).all() and (got["one"] == got["3+rest"]).all()


def test_seam_refusals_change_nothing(seam_engine, np_state_dict):
    eng, s = seam_engine, _stream()
    _seam_open(eng)
    rows = _seam_rows(np_state_dict, [0, 1])
    eng.pool_endpoint_frames([0, 1], rows.data_ptr(), SEAM_T, s)
    on = [0, 1, 2, 3, 4]
    before = eng.pool_endpoints(on, s).copy()
    p = rows.data_ptr()
    assert _status(eng.pool_endpoint_frames, [0, 0], p, 1, s) == rlib.ERR_ARG            # a slot listed twice
    assert _status(eng.pool_endpoint_frames, [0, 6], p, 1, s) == rlib.ERR_ARG            # a slot out of range
    assert _status(eng.pool_endpoint_frames, [-1], p, 1, s) == rlib.ERR_ARG
    assert _status(eng.pool_endpoint_frames, [], p, 1, s) == rlib.ERR_ARG                # no rows
    assert _status(eng.pool_endpoint_frames, [0, 1], p, 0, s) == rlib.ERR_ARG            # no frames
    assert _status(eng.pool_endpoint_frames, [0, 1], None, 1, s) == rlib.ERR_ARG         # null frames
    assert _status(eng.pool_endpoint_frames, [0, 5], p, 1, s) == rlib.ERR_STATE          # slot 5 has endpointing off
    assert _status(eng.pool_endpoints, [0, 5], s) == rlib.ERR_STATE
    assert _status(eng.pool_endpoints, [1, 1], s) == rlib.ERR_ARG
    assert _status(eng.pool_endpoints, [], s) == rlib.ERR_ARG
    assert (eng.pool_endpoints(on, s) == before).all()


# ---- C. through the pool calls -----------------------------------------------------------------------------------------------------
OPEN_AT = (0, 2, 1, 3)            # the step at which slot i's caller connects; slot 3 replays utterance 0 without endpointing
SLOT_UTT = (0, 1, 2, 0)
EP_SLOTS = (0, 1, 2)

_POOL_ENG = {}


def _pool_engine(mode, c):
    """one context per (mode, c), kept for the module; no test other than _pool_case touches its endpoint entry points"""
    if (mode, c) not in _POOL_ENG:
        eng = RnntEngine(max_streams=4, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=16, max_tokens=1024, vocab_size=V, blank_id=BLANK)
        eng.load_state_dict(C.state_dict(c), numerics=mode)
        _POOL_ENG[(mode, c)] = eng
    return _POOL_ENG[(mode, c)]


@pytest.fixture(scope="module", autouse=True)
def _close_pool_engines():
    yield
    for e in _POOL_ENG.values():
        e.close()
    _POOL_ENG.clear()


def _pool_call(eng, kind, slots, x, length, offs, s):
    req = [-1] * len(slots)
    if kind == "greedy":
        return eng.pool_chunk(slots, x.data_ptr(), length, offs, req, True, s)
    if kind == "encode":
        t = eng.pool_chunk(slots, x.data_ptr(), length, offs, req, False, s)
        return t
    return eng.pool_chunk_ctc_prefix(slots, x.data_ptr(), length, offs, req, 4, False, s)


def _pool_run(eng, c, kind, endpoint, expect=None):
    """The interleaved schedule: at every step one pool call per chunk length over the slots that have a chunk.  endpoint: "never" (the
    entry point is not called), "on", or "off" (turned on at open and off again at once).  Returns (launches per call keyed by
    (step, length), the slots each call listed, tokens per slot).  expect: per endpoint slot the twin's state after each of its chunks,
    compared after every step."""
    s = _stream()
    fb = [torch.from_numpy(C.fbank(u)).cuda() for u in range(3)]
    plans = [C.plan(C.UTTS[u][1], C.UTTS[u][2]) for u in SLOT_UTT]
    eng.reset(4, s)
    launches, listed, done = {}, {}, [0, 0, 0, 0]
    for step in range(max(o + len(p) for o, p in zip(OPEN_AT, plans))):
        for slot in range(4):
            if OPEN_AT[slot] == step:
                eng.stream_open(slot, s)
                if endpoint != "never" and slot in EP_SLOTS:
                    eng.stream_endpoint(slot, C.config(c, SLOT_UTT[slot]), s)
                    if endpoint == "off":
                        eng.stream_endpoint(slot, None, s)
        active = [slot for slot in range(4) if 0 <= step - OPEN_AT[slot] < len(plans[slot])]
        for length in sorted({plans[slot][0][1] for slot in active}):
            slots = [slot for slot in active if plans[slot][0][1] == length]
            ch = [plans[slot][step - OPEN_AT[slot]] for slot in slots]
            x = torch.stack([fb[SLOT_UTT[slot]][k[0]:k[0] + k[1]] for slot, k in zip(slots, ch)], 0).contiguous()
            l0 = eng.counters()[0]
            t = _pool_call(eng, kind, slots, x, length, [k[2] for k in ch], s)
            launches[(step, length)] = eng.counters()[0] - l0
            listed[(step, length)] = slots
            assert t == C.sub_len(length)
            if kind == "encode":
                eng.frames_discard(s)
            for slot in slots:
                done[slot] += 1
        if expect is not None:
            live = [slot for slot in EP_SLOTS if OPEN_AT[slot] <= step]
            got = eng.pool_endpoints(live, s)
            for slot, st in zip(live, got):
                want = expect[slot][done[slot] - 1] if done[slot] else [0] * 5
                assert st.tolist() == want, (step, slot, st.tolist(), want)
    tokens = {slot: eng.stream_tokens(slot, 0, s) for slot in range(4)} if kind == "greedy" else {}
    return launches, listed, tokens


def _twin_states(c):
    """per endpoint slot: rnnt_endpoint_scan_host over the oracle's posteriors (as float32), the state after each chunk"""
    out = {}
    for slot in EP_SLOTS:
        st, per = None, []
        for lp in C.oracle_lp(c)[SLOT_UTT[slot]]:
            st = rlib.endpoint_scan_host(lp.astype(np.float32), C.config(c, SLOT_UTT[slot]), st)
            per.append(st.tolist())
        assert per == C.oracle_states(c, SLOT_UTT[slot])         # the twin and the restatement agree on the oracle
        out[slot] = per
    return out


def _pool_case(mode, c, kind):
    eng = _pool_engine(mode, c)
    expect = _twin_states(c)
    _pool_run(eng, c, kind, "never")                             # warm-up: first-use allocations of this kind of call
    never, listed, tok_never = _pool_run(eng, c, kind, "never")
    on, listed_on, tok_on = _pool_run(eng, c, kind, "on", expect)
    off, _, tok_off = _pool_run(eng, c, kind, "off")
    assert listed == listed_on and set(on) == set(off) == set(never)
    n_with = 0
    for call, slots in listed.items():
        extra = 1 if any(slot in EP_SLOTS for slot in slots) else 0
        n_with += extra
        assert on[call] == off[call] + extra, (call, slots, on[call], off[call])     # exactly one launch more, and only then
        assert off[call] == never[call], (call, off[call], never[call])              # endpointing off: what the call always cost
    assert 0 < n_with < len(listed)                              # both kinds of call occurred
    if kind == "greedy":
        assert tok_on == tok_never == tok_off and all(len(tok_on[slot]) > 0 for slot in range(4))
        assert tok_on[0] == tok_on[3]                            # the replayed utterance, with and without endpointing in one call


@pytest.mark.parametrize("c", C.BIAS_C)
@pytest.mark.parametrize("mode", PARITY_MODES)
def test_pool_greedy(mode, c):
    _pool_case(mode, c, "greedy")


@pytest.mark.parametrize("kind", ["ctc_prefix", "encode"])
def test_pool_other_modes(kind):
    _pool_case("fp32", C.BIAS_C[0], kind)


def test_facade_on_the_device():
    """StreamPool.open(endpoint=) / endpoints() on a real engine: what the facade returns is what the engine holds"""
    pool = StreamPool(C.state_dict(6.0), 3, numerics="fp32")
    try:
        cfg = EndpointConfig(C.threshold(6.0)[0], rule1_ms=5 * 40, rule2_ms=0, rule3_ms=0)
        a, b = pool.open(endpoint=cfg), pool.open()
        x = torch.from_numpy(C.fbank(0)).cuda()
        assert pool.endpoints() == {a: (0, 0, 0, 0, 0)}
        for k in range(3):
            pool.feed(a, x[16 * k:16 * k + 16])
            pool.feed(b, x[16 * k:16 * k + 16])
            pool.step()
        got = pool.endpoints()
        raw = pool.engine.pool_endpoints([a], pool._stream(None))[0].tolist()
        assert set(got) == {a} and list(got[a]) == [raw[3], raw[4], raw[0], raw[1], raw[2]]
        assert got[a].frames == 9 and got[a].trailing + got[a].speech <= 9 and got[a].at_frame <= 9
        pool.close(a)
        assert pool.endpoints() == {}
        assert pool.open() == a and _status(pool.engine.pool_endpoints, [a], None) == rlib.ERR_STATE   # the next caller inherits nothing
    finally:
        pool.engine.close()


# ---- D. lifecycle ------------------------------------------------------------------------------------------------------------------
def test_lifecycle(np_state_dict):
    s = _stream()
    start = rlib.live_device_bytes()
    eng = RnntEngine(max_streams=3, max_chunk_frames=16, max_cache_frames=32, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    try:
        eng.load_state_dict(np_state_dict(0), numerics="fp32")
        eng.reset(3, s)
        for slot in range(3):
            eng.stream_open(slot, s)
        torch.cuda.synchronize()
        b0 = rlib.live_device_bytes()
        eng.stream_endpoint(0, (0.5, 1, 2, 0, 0), s)
        b1 = rlib.live_device_bytes()
        assert b1 > b0                                           # the tables, on the first use
        eng.stream_endpoint(1, (0.5, 1, 0, 0, 3), s)
        assert rlib.live_device_bytes() == b1                    # and only then
        wb = torch.from_numpy(np_state_dict(0)["ctc_head.ctc_lo.weight"][BLANK]).cuda()
        rows = (ALPHA * wb)[None, None, :].repeat(2, 4, 1).contiguous()           # four blank frames for both slots
        eng.pool_endpoint_frames([0, 1], rows.data_ptr(), 4, s)
        assert eng.pool_endpoints([0, 1], s).tolist() == [[4, 4, 0, 1, 2], [4, 4, 0, 3, 3]]
        eng.stream_open(0, s)                                    # the next caller in slot 0
        assert _status(eng.pool_endpoints, [0], s) == rlib.ERR_STATE              # the flag is gone
        assert _status(eng.pool_endpoint_frames, [0], rows.data_ptr(), 1, s) == rlib.ERR_STATE
        assert eng.pool_endpoints([1], s).tolist() == [[4, 4, 0, 3, 3]]           # the neighbour is untouched
        eng.stream_endpoint(0, (0.5, 1, 0, 0, 0), s)
        assert eng.pool_endpoints([0], s).tolist() == [[0] * 5]                   # and so is the state: nothing inherited
        eng.pool_endpoint_frames([0], rows.data_ptr(), 4, s)
        assert eng.pool_endpoints([0], s).tolist() == [[4, 4, 0, 0, 0]]           # under the new config only
        eng.stream_endpoint(1, None, s)                          # off, any time
        assert _status(eng.pool_endpoints, [1], s) == rlib.ERR_STATE
        eng.reset(3, s)                                          # rnnt_streams_reset clears all
        for slot in range(3):
            assert _status(eng.pool_endpoints, [slot], s) == rlib.ERR_STATE
        assert rlib.live_device_bytes() == b1
    finally:
        eng.close()
    assert rlib.live_device_bytes() == start


# ---- E. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(np_state_dict):
    s = _stream()
    eng = RnntEngine(max_streams=2, max_chunk_frames=16, max_cache_frames=32, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    bare = RnntEngine(max_streams=2, max_chunk_frames=16, max_cache_frames=32, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    try:
        good = (0.5, 1, 2, 2, 2)
        assert _status(eng.stream_endpoint, 0, good, s) == rlib.ERR_STATE            # weights not finalized
        eng.load_state_dict(np_state_dict(0), numerics="fp32")
        eng.reset(2, s)
        eng.stream_open(0, s)
        eng.stream_open(1, s)
        for bad in ((0.0, 1, 2, 2, 2), (1.0, 1, 2, 2, 2), (-0.1, 1, 2, 2, 2), (float("nan"), 1, 2, 2, 2), (0.5, -1, 2, 2, 2), (0.5, 1, -2, 2, 2),
                    (0.5, 1, 2, -2, 2), (0.5, 1, 2, 2, -2)):
            assert _status(eng.stream_endpoint, 0, bad, s) == rlib.ERR_ARG, bad
        assert _status(eng.stream_endpoint, 2, good, s) == rlib.ERR_ARG              # a slot out of range
        assert _status(eng.stream_endpoint, -1, good, s) == rlib.ERR_ARG
        assert _status(eng.pool_endpoints, [0], s) == rlib.ERR_STATE                 # none of the refused calls turned it on
        x = torch.from_numpy(T.synth_fbank(1, 16, seed=3)).cuda()
        eng.pool_chunk([0], x.data_ptr(), 16, [0], [-1], False, s)                   # slot 0 advances
        eng.frames_discard(s)
        assert _status(eng.stream_endpoint, 0, good, s) == rlib.ERR_STATE            # an advanced slot: its first frames are gone
        eng.stream_endpoint(0, None, s)                                              # off is accepted any time
        eng.stream_endpoint(1, good, s)                                              # its neighbour has not advanced
        assert eng.pool_endpoints([1], s).tolist() == [[0] * 5]
        bare.load_state_dict({k: v for k, v in np_state_dict(0).items() if not k.startswith("ctc_head.ctc_lo.")}, numerics="fp32")
        bare.reset(2, s)
        bare.stream_open(0, s)
        assert _status(bare.stream_endpoint, 0, good, s) == rlib.ERR_STATE           # ctc_head.ctc_lo.* not loaded
        out = torch.zeros(16, device="cuda")
        assert _status(bare.ctc_blank_logprob, x.data_ptr(), 1, out.data_ptr(), s) == rlib.ERR_STATE
        assert _status(eng.ctc_blank_logprob, x.data_ptr(), 0, out.data_ptr(), s) == rlib.ERR_ARG
    finally:
        eng.close()
        bare.close()
