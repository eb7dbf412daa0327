"""Segments of the stream pool on the device (rnnt_pool_segment, rnnt_stream_get_segment; StreamPool.next_segment / on_endpoint).
Needs a real MI355X: `pytest -m gpu`.

The contract under test is stated against twins, so every comparison is of bit patterns: a slot that segments with the encoder kept
encodes what a slot that never segments encodes, and decodes what a slot decodes whose decoder only joined at the boundary; a slot
that segments with a fresh encoder is a newly opened slot, except for what the caller configured and the audio front-end.  Shapes are
the smallest that go wrong: 16-frame chunks (t' = 3), three or four slots, beam 2 / 4.  Nothing here provokes a device fault: every
refusal is a host-side argument check."""
import struct

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntEngine, RnntError
from ctc_vr_amd.online_rnnt_model import EndpointConfig, StreamPool

pytestmark = pytest.mark.gpu

V, BLANK = T.VOCAB, T.BLANK
CHUNK, TQ = 16, 3
KINDS = ["greedy", "beam", "ctc", "ctc_ctx", "prefix"]
PHRASES = [[7, 8], [9]]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _status(fn, *a):
    with pytest.raises(RnntError) as e:
        fn(*a)
    return e.value.status


def _engine(sd, streams=3, cache=64, n_streams=None):
    eng = RnntEngine(max_streams=streams, max_chunk_frames=CHUNK, max_cache_frames=cache, max_enc_frames=16, max_tokens=256, vocab_size=V, blank_id=BLANK,
                     max_beam=2)
    eng.load_state_dict(sd, numerics="fp32")
    eng.reset(streams if n_streams is None else n_streams, _stream())
    return eng


@pytest.fixture(scope="module")
def sd(np_state_dict):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return np_state_dict(0)


@pytest.fixture(scope="module")
def fbank():
    """two utterances of six 16-frame chunks, [2, 96, 80] on the device; read only"""
    x = torch.from_numpy(T.synth_fbank(2, 6 * CHUNK, seed=29)).cuda().contiguous()
    torch.cuda.synchronize()
    return x


def _chunk(eng, kind, slot, fbank, k, off, utt=0):
    """chunk k of utterance utt into `slot` at encoder offset off, the whole cache kept"""
    s = _stream()
    x = fbank[utt:utt + 1, CHUNK * k:CHUNK * (k + 1)].contiguous()
    a = ([slot], x.data_ptr(), CHUNK, [off], [-1])
    if kind == "encode":
        t = eng.pool_chunk(*a, False, s)
        rows = eng.enc_frames(s)[slot].copy()
        eng.frames_discard(s)
        assert t == TQ and rows.shape == (TQ, 256)
        return rows
    t = {"greedy": lambda: eng.pool_chunk(*a, True, s), "beam": lambda: eng.pool_chunk_beam(*a, 2, s),
         "ctc": lambda: eng.pool_chunk_ctc_prefix(*a, 4, False, s), "ctc_ctx": lambda: eng.pool_chunk_ctc_prefix(*a, 4, True, s),
         "prefix": lambda: eng.pool_chunk_prefix(*a, 4, 0.3, 0.7, s)}[kind]()
    assert t == TQ
    return None


def _read(eng, kind, slot):
    """everything the slot kind's getters return: tokens, hypothesis order, f64 scores, LSTM states, CTC times"""
    s = _stream()
    if kind == "greedy":
        return eng.stream_tokens(slot, 0, s), eng.predictor_state(slot, s)
    if kind == "beam":
        return eng.stream_beam(slot, s), eng.stream_beam_states(slot, s)
    if kind in ("ctc", "ctc_ctx"):
        return eng.stream_ctc_prefix(slot, True, True, stream=s)
    return eng.stream_prefix(slot, True, s)


def _same(a, b):
    """equal bit patterns, through lists, tuples and dicts"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and struct.pack("d", a) == struct.pack("d", b)
    return a == b


def _open_all(eng, n=3):
    for slot in range(n):
        eng.stream_open(slot, _stream())


# ---- 3. the encoder is untouched (keep) ---------------------------------------------------------------------------------------------
def test_keep_leaves_encoder_and_neighbours_alone(sd, fbank):
    A, B = _engine(sd), _engine(sd)
    s = _stream()
    try:
        _open_all(A), _open_all(B)
        for k in range(2):                                       # the neighbour, slot 1 of A, is mid-utterance
            _chunk(A, "greedy", 1, fbank, k, TQ * k, utt=1)
        assert A.stream_segment(0) == (0, 0)
        for k in range(6):
            ra, rb = _chunk(A, "encode", 0, fbank, k, TQ * k), _chunk(B, "encode", 0, fbank, k, TQ * k)
            assert _same(ra, rb), f"chunk {k}: encoder frames differ"
            if k in (1, 3):                                      # after chunks 2 and 4
                before = (A.predictor_state(1, s), A.stream_tokens(1, 0, s), A.att_cache(1, s), A.cnn_cache(1, s), A.stream_segment(1))
                A.pool_segment([0], True, s)
                after = (A.predictor_state(1, s), A.stream_tokens(1, 0, s), A.att_cache(1, s), A.cnn_cache(1, s), A.stream_segment(1))
                assert _same(before, after), "the neighbour slot changed"
                assert A.stream_segment(0) == ((k + 1) // 2, TQ * (k + 1))
        assert A.att_cache(0, s).shape[2] == 6 * TQ
        assert _same(A.att_cache(0, s), B.att_cache(0, s)) and _same(A.cnn_cache(0, s), B.cnn_cache(0, s))
        _chunk(A, "greedy", 1, fbank, 2, TQ * 2, utt=1)          # and the neighbour goes on as the same stream in B does
        for k in range(3):
            _chunk(B, "greedy", 1, fbank, k, TQ * k, utt=1)
        assert _same(_read(A, "greedy", 1), _read(B, "greedy", 1)) and len(A.stream_tokens(1, 0, s)) > 0
    finally:
        A.close(), B.close()


# ---- 4. the decoders start over (keep), per slot kind -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_keep_restarts_the_decoder(sd, fbank, kind):
    A, B = _engine(sd), _engine(sd)
    s = _stream()
    try:
        if kind == "ctc_ctx":
            A.context_set(PHRASES, 3.0), B.context_set(PHRASES, 3.0)
        _open_all(A), _open_all(B)
        for k in range(3):
            _chunk(A, kind, 0, fbank, k, TQ * k)
            _chunk(B, "encode", 0, fbank, k, TQ * k)
        first = _read(A, kind, 0)
        A.pool_segment([0], True, s)
        # straight after the call: what a slot that was opened and never advanced reads (slot 2)
        h, c, tok = A.predictor_state(0, s)
        assert not h.any() and not c.any() and tok == BLANK and A.stream_tokens(0, 0, s) == []
        if kind == "beam":
            assert A.stream_beam(0, s) == [([], 0.0)] and not A.stream_beam_states(0, s)[0].any() and not A.stream_beam_states(0, s)[1].any()
        if kind in ("ctc", "ctc_ctx"):
            hyps, raw, frames = A.stream_ctc_prefix(0, False, True, stream=s)
            assert frames == 0 and [(t, sc) for t, sc, _, _ in hyps] == [([], 0.0)]
            assert _same((hyps, raw, frames), A.stream_ctc_prefix(2, False, True, stream=s))
        if kind == "prefix":
            hyps, ph, pc = A.stream_prefix(0, True, s)
            assert hyps == [([BLANK], 0.0)] and not ph.any() and not pc.any() and A.stream_prefix_size(0)[:2] == (1, 0)
            assert _same((hyps, ph, pc), A.stream_prefix(2, True, s))
        for k in range(3, 6):
            _chunk(A, kind, 0, fbank, k, TQ * k)
            _chunk(B, kind, 0, fbank, k, TQ * k)
        second, twin = _read(A, kind, 0), _read(B, kind, 0)
        assert _same(second, twin), f"{kind}: the second segment is not the twin's utterance\n{second}\n{twin}"
        assert not _same(first, second)                          # the comparison is of something
        if kind == "greedy":
            assert len(second[0]) > 0
        assert A.stream_segment(0) == (1, 3 * TQ) and B.stream_segment(0) == (0, 0)
    finally:
        A.close(), B.close()


# ---- 5. the fresh flavour -----------------------------------------------------------------------------------------------------------
def test_fresh_is_a_newly_opened_slot(sd, fbank):
    A, B = _engine(sd), _engine(sd)
    s = _stream()
    try:
        _open_all(A), _open_all(B)
        A.stream_keep_frames(0, True, s), B.stream_keep_frames(0, True, s)
        for k in range(3):
            _chunk(A, "greedy", 0, fbank, k, TQ * k)
        A.pool_segment([0], False, s)
        assert A.att_cache(0, s).shape[2] == 0 and A.stream_frames_len(0) == 0
        assert _same(A.cnn_cache(0, s), B.cnn_cache(0, s))       # the rings of a fresh stream, all layers
        for k in range(3, 6):
            _chunk(A, "greedy", 0, fbank, k, TQ * (k - 3))       # offsets from 0
            _chunk(B, "greedy", 0, fbank, k, TQ * (k - 3))
        assert _same(_read(A, "greedy", 0), _read(B, "greedy", 0)) and len(A.stream_tokens(0, 0, s)) > 0
        fa, fb = A.stream_frames(0, 0, s).cpu().numpy(), B.stream_frames(0, 0, s).cpu().numpy()
        assert fa.shape == (3 * TQ, 256) and _same(fa, fb)
        assert A.att_cache(0, s).shape[2] == 3 * TQ
        assert _same(A.att_cache(0, s), B.att_cache(0, s)) and _same(A.cnn_cache(0, s), B.cnn_cache(0, s))
        assert A.stream_segment(0) == (1, 3 * TQ)                # the session's frames run on
    finally:
        A.close(), B.close()


def test_fresh_keeps_the_audio_front_end(sd):
    eng = _engine(sd)
    s = _stream()
    try:
        _open_all(eng)
        g = torch.Generator().manual_seed(3)
        packets = [(torch.randn(2000, generator=g) * 0.1).repeat(2, 1).contiguous().cuda() for _ in range(3)]     # both slots hear the same
        out = [torch.zeros(2, 8, 80, device="cuda") for _ in range(3)]
        got = [eng.pool_wave([0, 1], packets[k].data_ptr(), 2000, [2000, 2000], [False, False], out[k].data_ptr(), 8, stream=s) for k in range(2)]
        before = eng.wave_state(0, s)
        eng.pool_segment([0], False, s)
        after = eng.wave_state(0, s)
        assert _same(before, after) and before["samples"] == 4000 and before["n_fft"] == 1024 and before["carry"].size > 0
        got.append(eng.pool_wave([0, 1], packets[2].data_ptr(), 2000, [2000, 2000], [False, False], out[2].data_ptr(), 8, stream=s))
        torch.cuda.synchronize()
        n0, n1 = (int(v) for v in got[2])
        assert n0 == n1 > 0 and torch.equal(out[2][0, :n0], out[2][1, :n1])      # the seam of the third packet: as in a slot that never segmented
        assert _same(eng.wave_state(0, s), eng.wave_state(1, s))
    finally:
        eng.close()


# ---- 6. endpoint and history across a boundary --------------------------------------------------------------------------------------
EP_CFG = (0.5, 1, 0, 0, 6)                                       # rule 3 at 6 frames: deterministic, independent of the posteriors


def test_endpoint_and_history_across_a_boundary(sd, fbank):
    A, B = _engine(sd), _engine(sd)
    s = _stream()
    try:
        _open_all(A), _open_all(B)
        for e in (A, B):
            e.stream_keep_frames(0, True, s)
            e.stream_endpoint(0, EP_CFG, s)
        for k in range(3):
            _chunk(A, "greedy", 0, fbank, k, TQ * k)
        st = A.pool_endpoints([0], s)[0].tolist()
        assert st[0] == 9 and st[3:] == [3, 6] and A.stream_frames_len(0) == 9
        A.pool_segment([0], True, s)
        assert A.pool_endpoints([0], s)[0].tolist() == [0] * 5 and A.stream_frames_len(0) == 0
        assert A.stream_frames(0, 0, s).shape == (0, 256)
        for k in range(3, 5):
            _chunk(A, "greedy", 0, fbank, k, TQ * k)
        for k in range(5):
            _chunk(B, "greedy", 0, fbank, k, TQ * k)
        rows = A.stream_frames(0, 0, s)
        twin = B.stream_frames(0, 0, s)
        assert rows.shape == (6, 256) and twin.shape == (15, 256) and torch.equal(rows, twin[9:15])
        lp = torch.empty(6, device="cuda")
        A.ctc_blank_logprob(rows.data_ptr(), 6, lp.data_ptr(), s)
        torch.cuda.synchronize()
        want = rlib.endpoint_scan_host(lp.cpu().numpy().astype(np.float32), EP_CFG, None)
        got = A.pool_endpoints([0], s)[0]
        assert got.tolist() == np.asarray(want).tolist() and got.tolist()[0] == 6 and got.tolist()[3:] == [3, 6]      # the config survived: rule 3 again
        assert A.stream_segment(0) == (1, 9)
    finally:
        A.close(), B.close()


# ---- 7. a session longer than the cache ---------------------------------------------------------------------------------------------
def test_session_longer_than_the_cache(sd):
    """the slot keeps its frames, so max_cache_frames bounds its utterance twice: the K/V cache and the history, which holds every frame
    since the boundary (a slot without a history gets one chunk more from the facade, whose first chunk keeps no cache)"""
    x = torch.from_numpy(T.synth_fbank(1, 12 * CHUNK, seed=31)).cuda()[0]
    cfg = EndpointConfig(0.5, rule1_ms=0, rule2_ms=0, rule3_ms=9 * 40)
    pool = StreamPool(sd, 3, vocab_size=V, blank_id=BLANK, max_chunk_frames=CHUNK, max_cache_frames=12, max_tokens=256, numerics="fp32")
    try:
        a = pool.open(keep_frames=True, endpoint=cfg, on_endpoint="fresh")
        tokens, segs = [], []
        for k in range(12):                                      # 36 encoder frames through a 12-frame cache
            pool.feed(a, x[CHUNK * k:CHUNK * (k + 1)])
            tokens += pool.step().get(a, [])
            segs += pool.segments(a)
        assert [g.index for g in segs] == [0, 1, 2, 3] and [g.start_frame for g in segs] == [0, 9, 18, 27] and [g.frames for g in segs] == [9] * 4
        assert all(g.endpoint.rule == 3 and g.endpoint.at_frame == 9 for g in segs)
        assert sum((g.result for g in segs), []) == tokens and len(tokens) > 0     # step()'s increments are the segments' tokens
        assert pool.close(a) == [] and pool.engine.stream_segment(a) == (4, 36)
        b = pool.open(keep_frames=True, endpoint=cfg)                          # today's behaviour, for contrast: the fifth chunk no longer fits
        assert b == a
        for k in range(4):
            pool.feed(b, x[CHUNK * k:CHUNK * (k + 1)])
            pool.step()
        pool.feed(b, x[CHUNK * 4:CHUNK * 5])
        assert _status(pool.step) == ERR_SHAPE
    finally:
        pool.engine.close()


# ---- 8. searches may be re-fixed ----------------------------------------------------------------------------------------------------
def test_searches_may_be_refixed_after_a_boundary(sd, fbank):
    eng = _engine(sd)
    s = _stream()
    try:
        eng.context_set(PHRASES, 3.0)
        _open_all(eng)
        x = fbank[0:1, :CHUNK].contiguous()
        plain = lambda beam, off: eng.pool_chunk_ctc_prefix([0], x.data_ptr(), CHUNK, [off], [-1], beam, False, s)
        biased = lambda off: eng.pool_chunk_ctc_prefix([1], x.data_ptr(), CHUNK, [off], [-1], 4, True, s)
        fused = lambda beam, cw, off: eng.pool_chunk_prefix([2], x.data_ptr(), CHUNK, [off], [-1], beam, cw, 1.0 - cw, s)
        plain(4, 0), biased(0), fused(4, 0.3, 0)
        eng.context_set([[11, 12, 13]], 2.0)                     # slot 1's graph is gone
        n0 = eng.counters()[0]
        assert _status(plain, 3, TQ) == ERR_ARG and "differ from the search in progress" in eng.lib.rnnt_last_error(eng.ctx).decode()
        assert _status(fused, 3, 0.5, TQ) == ERR_ARG and "differ from the search in progress" in eng.lib.rnnt_last_error(eng.ctx).decode()
        assert _status(biased, TQ) == ERR_STATE and "context graph changed" in eng.lib.rnnt_last_error(eng.ctx).decode()
        assert eng.counters()[0] == n0
        eng.pool_segment([0, 1, 2], True, s)
        plain(3, TQ), biased(TQ), fused(3, 0.5, TQ)              # the same calls
        hyps, _, frames = eng.stream_ctc_prefix(0, True, True, stream=s)
        assert frames == TQ and 0 < len(hyps) <= 3
        hyps, _, frames = eng.stream_ctc_prefix(1, True, True, stream=s)      # final: finalized under the graph that is set now
        assert frames == TQ and 0 < len(hyps) <= 4
        assert eng.stream_prefix_size(2)[:2] == (3, TQ) and 0 < len(eng.stream_prefix(2, False, s)) <= 3
    finally:
        eng.close()


# ---- 9. refusals and cost -----------------------------------------------------------------------------------------------------------
N_STREAMS = 3


def _advance_searches(eng, enc, lp):
    s = _stream()
    eng.pool_prefix_frames([0, 1], enc.data_ptr(), 3, 4, 0.3, 0.7, s)
    eng.pool_ctc_prefix_logprobs([0, 1], lp.data_ptr(), 3, 4, False, s)
    return [(eng.stream_prefix(b, True, s), eng.stream_ctc_prefix(b, False, True, stream=s)) for b in (0, 1)]


def test_refusals_change_nothing(sd, fbank):
    eng, clean = _engine(sd, streams=4, n_streams=N_STREAMS), _engine(sd, streams=4, n_streams=N_STREAMS)
    bare = RnntEngine(max_streams=2, max_chunk_frames=CHUNK, max_cache_frames=32, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    s = _stream()
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 3, 256, generator=g).cuda()
    lp = torch.log_softmax(torch.randn(2, 3, V, generator=g), -1).cuda().contiguous()
    try:
        assert _status(bare.pool_segment, [0], True, s) == ERR_STATE              # no weights
        _open_all(eng), _open_all(clean)
        first = _advance_searches(eng, enc, lp)
        assert _same(first, _advance_searches(clean, enc, lp))
        fn, limit = "rnnt_pool_segment", N_STREAMS
        for keep in (True, False):
            for slots, text in (([], f"{fn}: 0 slots of {limit}"), (list(range(limit)) + [0], f"{fn}: {limit + 1} slots of {limit}"),
                                ([-1], f"{fn}: row 0: slot -1 outside [0, {limit})"), ([limit], f"{fn}: row 0: slot {limit} outside [0, {limit})"),
                                ([0, 0], f"{fn}: slot 0 listed twice")):
                n0 = eng.counters()[0]
                assert _status(eng.pool_segment, slots, keep, s) == ERR_ARG
                assert eng.lib.rnnt_last_error(eng.ctx).decode() == text
                assert eng.counters()[0] == n0, "a refused call launched something"
        x = fbank[0:1, :CHUNK].contiguous()
        for e in (eng, clean):
            e.pool_chunk([2], x.data_ptr(), CHUNK, [0], [-1], False, s)           # frames stay buffered
        n0 = eng.counters()[0]
        assert _status(eng.pool_segment, [0], True, s) == ERR_STATE and _status(eng.pool_segment, [2], False, s) == ERR_STATE
        assert eng.counters()[0] == n0 and eng.stream_segment(0) == (0, 0) and eng.stream_segment(2) == (0, 0)
        for e in (eng, clean):
            e.frames_discard(s)
        # the searches go on as on the engine that saw no refused call
        assert _same(_advance_searches(eng, enc, lp), _advance_searches(clean, enc, lp))
        assert eng.stream_prefix_size(0)[1] == 6
        assert _status(eng.stream_segment, 4) == ERR_ARG and _status(eng.stream_segment, -1) == ERR_ARG
    finally:
        eng.close(), clean.close(), bare.close()


def test_one_launch_whatever_the_number_of_slots(sd, fbank):
    eng = _engine(sd)
    s = _stream()
    try:
        _open_all(eng)
        for slot in range(3):
            eng.stream_keep_frames(slot, True, s)
            eng.stream_endpoint(slot, EP_CFG, s)
        for kind, slot in (("beam", 0), ("ctc", 1), ("prefix", 2), ("greedy", 0)):      # every state kind exists
            _chunk(eng, kind, slot, fbank, 0, TQ * (1 if kind == "greedy" else 0))
        cost = {}
        for keep in (True, False):
            for slots in ([1], [0, 1, 2]):
                n0 = eng.counters()[0]
                eng.pool_segment(slots, keep, s)
                cost[(keep, len(slots))] = eng.counters()[0] - n0
        print(f"launches of one rnnt_pool_segment call (keep_encoder, n): {cost}")
        assert len(set(cost.values())) == 1 and cost[(True, 1)] == 1
        assert [eng.stream_segment(slot) for slot in range(3)] == [(2, TQ * 2), (4, TQ), (2, TQ)]
        for slot in range(3):
            assert eng.pool_endpoints([slot], s)[0].tolist() == [0] * 5 and eng.stream_frames_len(slot) == 0
            assert eng.stream_beam(slot, s) == [([], 0.0)] and eng.stream_prefix(slot, False, s) == [([BLANK], 0.0)]
    finally:
        eng.close()


# ---- 10. the facade end to end ------------------------------------------------------------------------------------------------------
def test_facade_on_endpoint_equals_next_segment_by_hand(sd):
    cfg = EndpointConfig(0.5, rule1_ms=0, rule2_ms=0, rule3_ms=6 * 40)
    wave = (torch.randn(3, 8 * 8192, generator=torch.Generator().manual_seed(11)) * 0.1).cuda()      # 8 packets = 8 chunks of 16 frames each

    def run(auto):
        pool = StreamPool(sd, 3, vocab_size=V, blank_id=BLANK, max_chunk_frames=CHUNK, max_cache_frames=64, max_tokens=256, numerics="fp32",
                          chunk_frames=CHUNK)
        try:
            on = "keep" if auto else None
            slots = [pool.open(keep_frames=True, endpoint=cfg, on_endpoint=on), pool.open(ctc_prefix_beam=4, endpoint=cfg, on_endpoint=on),
                     pool.open(prefix_beam=4, endpoint=cfg, on_endpoint=on)]
            segs = {slot: [] for slot in slots}
            seen = None
            for k in range(8):
                for slot in slots:
                    pool.feed_wave(slot, wave[slot, 8192 * k:8192 * (k + 1)])
                out = pool.step()
                for slot in slots:
                    if auto:
                        segs[slot] += pool.segments(slot)
                    elif k % 2 == 1:                             # rule 3 at 6 frames fires after every second chunk
                        assert pool.endpoints([slot])[slot].rule == 3
                        segs[slot].append(pool.next_segment(slot))
                if k == 4:                                       # one chunk into the third segment of the greedy slot
                    assert pool.engine.stream_frames_len(slots[0]) == TQ
                    tt = pool.token_times(slots[0])
                    assert len(tt) == len(out.get(slots[0], [])) == len(pool.engine.stream_tokens(slots[0], 0, pool._stream(None)))
                    assert all(0.0 <= a <= b <= TQ * 0.04 + 1e-9 for a, b in tt)
                    seen = (tt, out.get(slots[0], []))
            return segs, seen
        finally:
            pool.engine.close()

    auto, seen_auto = run(True)
    hand, seen_hand = run(False)
    for slot in range(3):
        assert [g.index for g in auto[slot]] == [0, 1, 2, 3] and [g.start_frame for g in auto[slot]] == [0, 6, 12, 18]
        assert all(g.frames == 6 and g.endpoint.rule == 3 and g.endpoint.at_frame == 6 for g in auto[slot])
        assert _same([tuple(g) for g in auto[slot]], [tuple(g) for g in hand[slot]]), f"slot {slot}: step() and next_segment() disagree"
    assert _same(seen_auto, seen_hand)
    assert sum(len(g.result) for g in auto[0]) > 0                                 # the greedy slot said something
    assert all(len(g.result) > 0 and g.result[0][2] == sorted(g.result[0][2]) and all(0 <= t < 6 for t in g.result[0][2]) for g in auto[1])   # CTC times: segment-relative
