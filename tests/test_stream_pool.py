"""Stream pool on the GPU: slots of one context that open, advance and close independently (rnnt_stream_open, rnnt_pool_chunk,
rnnt_stream_get_tokens; StreamPool).  The contract under test: the tokens, encoder frames and cached state of an utterance that
runs in a slot are those of the same utterance run alone through the per-chunk API, bit for bit, whatever the other slots do.
Everything runs through the C ABI and is checked against the CPU oracle (oracle/rnnt_oracle.py) or against a one-stream context.
Needs a real MI355X.  Nothing here provokes a device fault: every refusal is a host-side argument check."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntError
from ctc_vr_amd.online_rnnt_model import StreamingBatch, StreamPool, pool_plan

pytestmark = pytest.mark.gpu

ENC_TOL = 1e-3                    # the project's encoder tolerance against the oracle
MARGIN = 1e-3
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
CHUNK = 16
BLANK = T.BLANK
SEED_W = 0
# (fbank frames, input seed): 12 utterances of 10 different lengths; 20, 31 and 16 frames are shorter than two chunks (a single,
# tail-merged chunk), 1100 frames reach 204 cached encoder frames, 200 appears twice with different audio
UTTS = [(1100, 101), (200, 102), (20, 103), (31, 104), (112, 105), (160, 106), (47, 107), (200, 108), (75, 109), (333, 110), (16, 111), (130, 112)]
ARRIVALS = [0, 0, 0, 1, 2, 3, 5, 5, 8, 9, 12, 14]


@pytest.fixture(params=PARITY_MODES)
def numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    return request.param


_CACHE = {}


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = T.make_state_dict(SEED_W)
    return _CACHE["sd"]


def _x(u, dev=True):
    key = ("x", u, dev)
    if key not in _CACHE:
        frames, seed = UTTS[u] if isinstance(u, int) else u
        x = torch.from_numpy(T.synth_fbank(1, frames, seed=seed))[0]
        _CACHE[key] = x.cuda() if dev else x
    return _CACHE[key]


def _pool(numerics, n_slots, max_cache_frames=512):
    """one context per (mode, size), reused across tests: reset() frees every slot and resets the context"""
    key = ("pool", numerics, n_slots, max_cache_frames)
    if key not in _CACHE:
        _CACHE[key] = StreamPool(_sd(), n_slots, max_cache_frames=max_cache_frames, numerics=numerics)
    _CACHE[key].reset()
    return _CACHE[key]


def _batch(numerics, n):
    key = ("batch", numerics, n)
    if key not in _CACHE:
        _CACHE[key] = StreamingBatch(_sd(), n, numerics=numerics)
    return _CACHE[key]


def _b1(numerics, u):
    """the utterance alone (B = 1) through the existing per-chunk API: rnnt_encoder_chunk + rnnt_greedy_decode + rnnt_frames_consume"""
    key = ("b1", numerics, u)
    if key not in _CACHE:
        sb = _batch(numerics, 1)
        _CACHE[key] = sb.decode_script(_x(u)[None].contiguous(), CHUNK, per_chunk_decode=True)[0]
    return _CACHE[key]


def oracle_run(u):
    """oracle B = 1 decode-script greedy run of utterance u -> (tokens, encoder frames [1, F, 256])"""
    key = ("oracle", u)
    if key not in _CACHE:
        from oracle import rnnt_oracle as O
        if "osd" not in _CACHE:
            _CACHE["osd"] = O.to_torch_sd(_sd())
        x = _x(u, dev=False)[None]
        st = O.OracleStream(_CACHE["osd"], BLANK, CHUNK)
        toks, encs = [], []
        for a, b in T.chunk_plan(x.size(1), CHUNK):
            tr = {}
            toks += st.process_single_chunk(x[:, a:b], trace=tr)
            if "enc_out" in tr:
                encs.append(tr["enc_out"])
        _CACHE[key] = (toks, torch.cat(encs, 1))
    return _CACHE[key]


def oracle_min_margin(utts=None, device="cpu"):
    """smallest top-2 logit margin of the oracle's greedy decisions over the utterances (testing.greedy_margins)"""
    utts = range(len(UTTS)) if utts is None else utts
    worst = float("inf")
    for u in utts:
        toks, enc = oracle_run(u)
        m, ok = T.greedy_margins(_sd(), enc.numpy(), [toks], blank=BLANK, device=device)
        assert ok.all(), f"utterance {u}: the float64 replay does not reproduce the oracle's tokens"
        worst = min(worst, float(m[0]))
    return worst


def schedule(n_slots, utts, arrivals, chunk=CHUNK, busy=()):
    """Steps of a staggered arrival script.  Utterance k (index into `utts`) arrives at step arrivals[k], takes the lowest free
    slot (waits if none), delivers one chunk of its chunk plan per step and is closed after the step of its last chunk.
    -> [{"open": [(k, slot)], "feed": [(k, slot, a, b)], "close": [(k, slot)]}]"""
    free = [s for s in range(n_slots) if s not in busy]
    waiting = list(range(len(utts)))
    live, steps, t = {}, [], 0
    while waiting or live:
        st = {"open": [], "feed": [], "close": []}
        while waiting and arrivals[waiting[0]] <= t and free:
            k = waiting.pop(0)
            slot = free.pop(0)
            live[slot] = [k, list(T.chunk_plan(UTTS[utts[k]][0], chunk))]
            st["open"].append((k, slot))
        for slot in sorted(live):
            k, plan = live[slot]
            a, b = plan.pop(0)
            st["feed"].append((k, slot, a, b))
            if not plan:
                st["close"].append((k, slot))
        for k, slot in st["close"]:
            del live[slot]
            free.append(slot)
            free.sort()
        steps.append(st)
        t += 1
    return steps


def run_greedy(pool, utts, steps, before_close=None, max_steps=None):
    """drive a StreamPool through the steps; -> tokens per utterance index (None while unfinished)"""
    toks = [None] * len(utts)
    inc = {k: [] for k in range(len(utts))}
    for st in steps[:max_steps]:
        for k, slot in st["open"]:
            assert pool.open() == slot
        slot_utt = {}
        for k, slot, a, b in st["feed"]:
            pool.feed(slot, _x(utts[k])[a:b])
            slot_utt[slot] = k
        for slot, new in pool.step().items():
            inc[slot_utt[slot]].extend(new)
        for k, slot in st["close"]:
            if before_close:
                before_close(k, slot)
            toks[k] = pool.close(slot)
            assert toks[k] == inc[k], "the increments of step() add up to the tokens of close()"
    return toks


def run_encoder_only(engine, utts, steps):
    """the same steps through rnnt_pool_chunk(greedy = 0) + rnnt_get_enc_frames + rnnt_frames_discard -> per utterance the list of
    its chunks' encoder frames [t', 256]"""
    s = torch.cuda.current_stream().cuda_stream
    offs, out = {}, {k: [] for k in range(len(utts))}
    for st in steps:
        for k, slot in st["open"]:
            engine.stream_open(slot, s)
            offs[slot] = 0
        feeds = [f for f in st["feed"] if f[3] - f[2] >= 7]
        calls, offs, index = pool_plan([(slot, b - a) for _, slot, a, b in feeds], offs)
        for c, (length, slots, call_offs) in enumerate(calls):
            rows = [f for f, at in zip(feeds, index) if at[0] == c]
            x = torch.stack([_x(utts[k])[a:b] for k, _, a, b in rows], 0).contiguous()
            tq = engine.pool_chunk(slots, x.data_ptr(), length, call_offs, call_offs, False, s)
            fr = engine.enc_frames(s)
            assert fr.shape[1] == tq
            for (k, slot, _, _) in rows:
                out[k].append(fr[slot].copy())
            engine.frames_discard(s)
    return out


def snapshot(engine, slot):
    s = torch.cuda.current_stream().cuda_stream
    h, c, tok = engine.predictor_state(slot, s)
    return {"att": engine.att_cache(slot, s), "cnn": engine.cnn_cache(slot, s), "h": h, "c": c, "tok": tok,
            "tokens": np.asarray(engine.stream_tokens(slot, 0, s), np.int32)}


def assert_same_state(a, b, what):
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape, f"{what}: {key} has shape {x.shape} vs {y.shape}"
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs (max abs {np.abs(x.astype(np.float64) - y.astype(np.float64)).max() if x.size else 0})"


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
def test_staggered_arrivals_vs_oracle(numerics):
    """12 utterances of 10 lengths through a pool of 8 slots, opened at different steps, slots reused after close: every
    utterance's tokens equal the oracle's B = 1 decode-script tokens, its encoder frames are within 1e-3 of the oracle's.
    Margin guard: the oracle's smallest top-2 margin over these utterances (weights seed 0, blank bias 11, the input seeds of
    UTTS) is 1.04e-2 (utterance 0; computed on the CPU), asserted >= 1e-3 below, so a token flip is a bug and not a near-tie."""
    worst = oracle_min_margin(device="cuda")
    print(f"oracle min top-2 margin over the {len(UTTS)} utterances: {worst:.3e}")
    assert worst >= MARGIN, worst
    utts = list(range(len(UTTS)))
    steps = schedule(8, utts, ARRIVALS)
    opened = [slot for st in steps for _, slot in st["open"]]
    assert len(opened) == 12 and len(set(opened)) < 12, "the script must reuse slots"
    assert max(len(st["feed"]) for st in steps) >= 6 and len({b - a for st in steps for _, _, a, b in st["feed"]}) >= 5
    pool = _pool(numerics, 8)
    toks = run_greedy(pool, utts, steps)
    for u in utts:
        assert toks[u] == oracle_run(u)[0], f"utterance {u} ({UTTS[u][0]} frames): tokens differ from the oracle"
    pool.reset()
    encs = run_encoder_only(pool.engine, utts, steps)
    worst_err = 0.0
    for u in utts:
        got = np.concatenate(encs[u], 0)
        ref = oracle_run(u)[1][0].numpy()
        assert got.shape == ref.shape, (u, got.shape, ref.shape)
        err = float(np.abs(got - ref).max())
        worst_err = max(worst_err, err)
        print(f"utterance {u}: {got.shape[0]} encoder frames, max |diff| to the oracle {err:.3e}")
        assert err <= ENC_TOL, (u, err)
    print(f"[{numerics}] worst encoder error {worst_err:.3e}")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_neighbour_invariance_bitwise(numerics):
    """utterance 9 (333 frames) in slot 5 of a busy staggered pool and alone in slot 0 of an otherwise idle pool: tokens, every
    chunk's encoder frames, att cache, cnn cache and predictor state after the last chunk are bit-identical."""
    U = 9
    busy_utts = [0, 1, 4, 5, 7, U, 2, 3, 6, 8, 10, 11]
    busy_arr = [0, 0, 0, 0, 0, 0, 1, 2, 3, 5, 7, 9]
    steps_busy = schedule(8, busy_utts, busy_arr)
    assert (5, 5) in steps_busy[0]["open"], "utterance 9 must sit in slot 5"
    steps_alone = schedule(8, [U], [0])
    assert steps_alone[0]["open"] == [(0, 0)]
    state = {}
    pool = _pool(numerics, 8)
    tb = run_greedy(pool, busy_utts, steps_busy, before_close=lambda k, slot: state.__setitem__(("busy", k), snapshot(pool.engine, slot)))
    pool.reset()
    eb = run_encoder_only(pool.engine, busy_utts, steps_busy)
    pool.reset()
    ta = run_greedy(pool, [U], steps_alone, before_close=lambda k, slot: state.__setitem__(("alone", k), snapshot(pool.engine, slot)))
    pool.reset()
    ea = run_encoder_only(pool.engine, [U], steps_alone)
    assert tb[5] == ta[0] and len(ta[0]) > 0
    assert state[("busy", 5)]["att"].shape[2] > 50
    assert_same_state(state[("busy", 5)], state[("alone", 0)], "slot 5 of a busy pool vs slot 0 of an idle pool")
    assert len(eb[5]) == len(ea[0]) == len(T.chunk_plan(UTTS[U][0], CHUNK))
    for c, (x, y) in enumerate(zip(eb[5], ea[0])):
        assert x.tobytes() == y.tobytes(), f"encoder frames of chunk {c} differ (max abs {np.abs(x - y).max()})"
    for k, u in enumerate(busy_utts):                      # and every neighbour is still its own B = 1 run
        assert tb[k] == _b1(numerics, u), f"utterance {u}"


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 32])
def test_in_phase_equals_lock_step_bitwise(numerics, chunk):
    """all slots opened together and stepped together give bit-identical tokens and caches to StreamingBatch.process_chunk on a second
    context (chunk 16: rel_attention_stream; chunk 32: 7 new frames, rel_attention<2>)."""
    n, frames = 4, 200
    x = torch.from_numpy(T.synth_fbank(n, frames, seed=77)).cuda()
    pool = _pool(numerics, n)
    sb = _batch(numerics, n)
    sb.reset()
    slots = [pool.open() for _ in range(n)]
    assert slots == list(range(n))
    for a, b in T.chunk_plan(frames, chunk):
        for s in slots:
            pool.feed(s, x[s, a:b])
        pool.step()
        sb.process_chunk(x[:, a:b].contiguous())
    s_ = torch.cuda.current_stream().cuda_stream
    ref_toks = sb.engine.tokens(s_)
    for s in slots:
        got = snapshot(pool.engine, s)
        h, c, tok = sb.engine.predictor_state(s, s_)
        ref = {"att": sb.engine.att_cache(s, s_), "cnn": sb.engine.cnn_cache(s, s_), "h": h, "c": c, "tok": tok, "tokens": np.asarray(ref_toks[s], np.int32)}
        assert len(ref_toks[s]) > 0 and ref["att"].shape[2] > 0
        assert_same_state(got, ref, f"slot {s}, chunk {chunk}: pool vs lock step")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_idle_slot_untouched(numerics):
    """a mid-utterance slot that is left out of 20 pool steps, while neighbours open, run and close around it, keeps its K/V cache,
    rings, predictor state and tokens bitwise; continued afterwards, its final tokens equal its B = 1 run."""
    A = 9
    plan = T.chunk_plan(UTTS[A][0], CHUNK)
    pool = _pool(numerics, 8)
    slot = pool.open()
    assert slot == 0
    for a, b in plan[:6]:
        pool.feed(slot, _x(A)[a:b])
        pool.step()
    before = snapshot(pool.engine, slot)
    assert before["att"].shape[2] == 15 and len(before["tokens"]) > 0
    others = [0, 2, 3, 4, 6, 10, 8, 11, 1, 5]
    steps = schedule(8, others, [0, 0, 0, 1, 1, 2, 3, 4, 6, 8], busy=(0,))
    assert len(steps) > 20
    run_greedy(pool, others, steps, max_steps=20)
    head = steps[:20]
    assert sum(len(st["open"]) for st in head) >= 8 and sum(len(st["close"]) for st in head) >= 5
    assert all(s != 0 for st in head for _, s, _, _ in st["feed"])
    after = snapshot(pool.engine, slot)
    assert_same_state(before, after, "idle slot across 20 pool steps of its neighbours")
    for a, b in plan[6:]:
        pool.feed(slot, _x(A)[a:b])
        pool.step()
    assert pool.close(slot) == _b1(numerics, A)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_reopen_after_long_utterance(numerics):
    """a slot closed after a long utterance (204 cached frames) and reopened gives the short next utterance its B = 1 result: stale
    K/V rows, ring rows, LSTM state and tokens are all dead."""
    pool = _pool(numerics, 2)
    long_toks = run_greedy(pool, [0], schedule(2, [0], [0]))[0]
    assert long_toks == _b1(numerics, 0) and len(long_toks) > 0
    for u in (6, 2, 1):
        slot = pool.open()
        assert slot == 0
        for a, b in T.chunk_plan(UTTS[u][0], CHUNK):
            pool.feed(slot, _x(u)[a:b])
            pool.step()
        st = snapshot(pool.engine, slot)
        toks = pool.close(slot)
        assert toks == _b1(numerics, u), f"utterance {u} in a reopened slot"
        sb = _batch(numerics, 1)                                # _b1 may be cached: run the one-stream context again for its state
        sb.decode_script(_x(u)[None].contiguous(), CHUNK, per_chunk_decode=True)
        s_ = torch.cuda.current_stream().cuda_stream
        h, c, tok = sb.engine.predictor_state(0, s_)
        ref = {"att": sb.engine.att_cache(0, s_), "cnn": sb.engine.cnn_cache(0, s_), "h": h, "c": c, "tok": tok, "tokens": np.asarray(toks, np.int32)}
        assert_same_state(st, ref, f"utterance {u} in a reopened slot vs a one-stream context")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(numerics):
    """duplicate slot, slot >= n, 6-frame chunk, a slot whose K/V cache would overflow listed beside healthy ones, and a lock-step
    call in pool mode: the documented status, no slot's state changes, and a following valid run still gives B = 1 results."""
    CAP = 62                                                   # K/V rows per slot: chunk 22 of a 16-frame-chunk stream needs 63
    full = (336, 120)                                          # 21 chunks of 16 frames: 60 keys at its last chunk
    utts = [4, 5, 8, full]
    pool = _pool(numerics, 4, max_cache_frames=CAP)
    eng = pool.engine
    s_ = torch.cuda.current_stream().cuda_stream
    slots = [pool.open() for _ in range(4)]
    plans = [list(T.chunk_plan(UTTS[u][0] if isinstance(u, int) else u[0], CHUNK)) for u in utts]
    assert len(plans[3]) == 21
    done = [0, 0, 0, 0]

    def advance(k, n_chunks):
        for a, b in plans[k][done[k]:done[k] + n_chunks]:
            pool.feed(slots[k], _x(utts[k])[a:b])
            pool.step()
        done[k] += n_chunks

    advance(3, 21)                                             # slot 3: its utterance is complete, the cache holds 60 frames
    for k in range(3):
        advance(k, 2)
    before = [snapshot(eng, s) for s in slots]
    offs = [4 * d for d in done]
    x16 = torch.stack([_x(utts[k])[:16] for k in range(4)], 0).contiguous()

    def refused(status, sl, frames=16):
        rows = x16[:len(sl), :frames].contiguous()
        with pytest.raises(RnntError) as e:
            eng.pool_chunk(sl, rows.data_ptr(), frames, [offs[s] if s < 4 else 0 for s in sl], [offs[s] if s < 4 else 0 for s in sl], True, s_)
        assert e.value.status == status, (e.value.status, str(e.value))
        for s in slots:
            assert_same_state(before[s], snapshot(eng, s), f"slot {s} after a refused call")

    refused(ERR_ARG, [0, 0])
    refused(ERR_ARG, [0, 4])
    refused(ERR_ARG, [-1])
    refused(ERR_SHAPE, [0, 1], frames=6)
    refused(ERR_SHAPE, [0, 1, 3])                              # slot 3 would need 63 K/V rows of 62
    with pytest.raises(RnntError) as e:
        eng.encoder_chunk(x16.data_ptr(), 16, 0, 0, s_)
    assert e.value.status == ERR_STATE
    with pytest.raises(RnntError) as e:
        eng.encoder_chunks(x16.data_ptr(), 16, [0], [16], [0], [0], s_, greedy=True)
    assert e.value.status == ERR_STATE
    for s in slots:
        assert_same_state(before[s], snapshot(eng, s), f"slot {s} after a refused lock-step call")
    # an encoder-only call leaves frames buffered: the next pool call refuses until they are discarded
    snap3 = snapshot(eng, 3)
    a, b = plans[0][done[0]]
    row = _x(utts[0])[a:b][None].contiguous()
    eng.pool_chunk([0], row.data_ptr(), b - a, [offs[0]], [offs[0]], False, s_)
    with pytest.raises(RnntError) as e:
        eng.pool_chunk([1], x16.data_ptr(), 16, [offs[1]], [offs[1]], True, s_)
    assert e.value.status == ERR_STATE
    eng.frames_discard(s_)
    assert_same_state(snap3, snapshot(eng, 3), "slot 3 after an encoder-only call of slot 0")
    # slot 0's chunk above was encoded but not decoded: restart that slot's utterance, finish everything, compare with B = 1
    pool.close(0)
    assert pool.open() == 0
    done[0] = 0
    for k in range(3):
        advance(k, len(plans[k]) - done[k])
    for k in range(4):
        assert pool.close(slots[k]) == _b1(numerics, utts[k]), f"slot {k} after the refusals"
