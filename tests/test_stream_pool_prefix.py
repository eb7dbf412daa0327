"""Transducer prefix beam search per slot of the stream pool on the device (rnnt_pool_prefix_frames, rnnt_pool_chunk_prefix,
rnnt_stream_get_prefix, rnnt_stream_prefix_reset; StreamPool.open(prefix_beam=...)).

The contract under test: a search fed in pieces is, bit for bit, the B = 1 one-call search (rnnt_prefix_beam_decode) over the same
frames, whatever the split and whatever the other slots do.  Both run the same device functions on the same numbers, so results are
compared as bytes (tokens, bit patterns of the f64 scores, of h and of c); the only tolerances here are those of test_prefix_beam.py
against the CPU oracle.  The step kernel has two shapes with the same bits -- one hypothesis per workgroup, or up to four of a slot --
and picks by the size of the launch; launches this small would always take the first, so the multi-slot contexts here are created
with RNNT_PREFIX_GROUP=4 (always four) and the one-slot contexts they are compared with are left to the choice (one).  Needs a real MI355X.  Nothing here provokes a device fault: every refusal is a host-side argument check."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntEngine, RnntError, pack_nbest, rescore_select
import test_prefix_beam as PB

pytestmark = pytest.mark.gpu

BLANK = T.BLANK
LENS = (15, 9, 12)            # encoder frames of the three utterances walked (of the 15 that 64 fbank frames give)
SPLITS = {"ones": (), "one_and_rest": (1,), "uneven": (2, 3)}     # the splits of test_stream_pool_ctc_prefix.py
W_FUSED, W_RNNT = (0.3, 0.7), (0.0, 1.0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return PB.bits(a)


def chunks_of(length, split):
    out, left = [], length
    for want in SPLITS[split]:
        if left > 0:
            out.append(min(want, left))
            left -= out[-1]
    if split == "ones":
        return [1] * length
    return out + ([left] if left > 0 else [])


def _create(group, **kw):
    """a context whose step kernel takes `group` hypotheses per workgroup (None: by the size of the launch); the knob is read at rnnt_create"""
    old = os.environ.pop("RNNT_PREFIX_GROUP", None)
    try:
        if group is not None:
            os.environ["RNNT_PREFIX_GROUP"] = str(group)
        return RnntEngine(**kw)
    finally:
        os.environ.pop("RNNT_PREFIX_GROUP", None)
        if old is not None:
            os.environ["RNNT_PREFIX_GROUP"] = old


def _engine(sd, slots, vocab=T.VOCAB, frames=64, max_beam=0, group=4):
    eng = _create(group, max_streams=slots, max_chunk_frames=64, max_cache_frames=frames, max_enc_frames=64, max_tokens=256, vocab_size=vocab,
                  blank_id=BLANK, max_beam=max_beam)
    eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope="module")
def world(np_state_dict):
    """seeded weights; a three-slot context (with the lock-step and pool beams), a one-slot context, a three-slot context without the
    CTC head, a vocabulary-8 context; per context the encoder frames [3, 15, 256] of one rnnt_encoder_full call over 64 fbank frames,
    and a cache of the one-call references"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    sd = np_state_dict(0)
    sd8 = T.make_state_dict(0, vocab=8)
    engs = {"full": _engine(sd, 3, max_beam=16), "solo": _engine(sd, 1, group=None),
            "no_ctc": _engine({k: v for k, v in sd.items() if not k.startswith("ctc_head.")}, 3), "v8": _engine(sd8, 3, vocab=8)}
    x = torch.from_numpy(T.synth_fbank(3, 64, seed=91)).cuda().contiguous()
    enc = {}
    for name in ("full", "no_ctc", "v8"):
        e = torch.empty(3, 15, 256, device="cuda")
        assert engs[name].encoder_full(x.data_ptr(), [64, 64, 64], 3, 64, e.data_ptr(), _stream()) == 15
        enc[name] = e
    enc["solo"] = enc["full"]
    torch.cuda.synchronize()
    w = {"sd": sd, "eng": engs, "enc": enc, "x": x, "ref": {}}
    yield w
    for e in engs.values():
        e.close()


def one_call(w, name, utt, n, beam, weights):
    """the oracle: B = 1 rnnt_prefix_beam_decode over frames [0, n) of utterance utt -> (hyps, h [n_hyp, 256], c)"""
    key = (name if name != "solo" else "full", utt, n, beam, weights)
    if key not in w["ref"]:
        eng = w["eng"][key[0]]
        rows = w["enc"][name][utt:utt + 1, :max(n, 1)].contiguous()
        hyps, h, c = eng.prefix_beam_decode(rows.data_ptr(), [n], 1, rows.size(1), beam, weights[0], weights[1], True, _stream())
        w["ref"][key] = (hyps[0], h[0, :len(hyps[0])].copy(), c[0, :len(hyps[0])].copy())
    return w["ref"][key]


def assert_same(got, want, what):
    (gh, g_h, g_c), (wh, w_h, w_c) = got, want
    assert [t for t, _ in gh] == [t for t, _ in wh], f"{what}: tokens\n{gh}\n{wh}"
    assert np.array_equal(bits(np.array([s for _, s in gh])), bits(np.array([s for _, s in wh]))), f"{what}: score bits\n{gh}\n{wh}"
    assert g_h.shape == w_h.shape and np.array_equal(bits(g_h), bits(w_h)), f"{what}: h bits"
    assert np.array_equal(bits(g_c), bits(w_c)), f"{what}: c bits"


def read(eng, slot):
    return eng.stream_prefix(slot, True, _stream())


def adv(eng, slots, rows, beam, weights, keep):
    """one rnnt_pool_prefix_frames call over rows (one [t, 256] tensor per listed slot); the call does not synchronise: rows stay in keep"""
    x = torch.stack(rows, 0).contiguous()
    keep.append(x)
    eng.pool_prefix_frames(slots, x.data_ptr(), x.size(1), beam, weights[0], weights[1], _stream())


def feed(eng, enc, lens, split, beam, weights, keep):
    """utterance b through slot b in the split's chunks; the utterances whose k-th chunks have one length share a call"""
    plan = [chunks_of(n, split) for n in lens]
    at = [0] * len(lens)
    for k in range(max(len(p) for p in plan)):
        for t in sorted({p[k] for p in plan if k < len(p)}):
            rows = [b for b in range(len(lens)) if k < len(plan[b]) and plan[b][k] == t]
            adv(eng, rows, [enc[b, at[b]:at[b] + t] for b in rows], beam, weights, keep)
            for b in rows:
                at[b] += t


# ---- 1. split invariance, seam form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("beam", [1, 4, 5, 9, 16])
@pytest.mark.parametrize("name,weights", [("full", W_FUSED), ("no_ctc", W_RNNT)])
def test_split_invariance(name, weights, beam, split, world):
    eng, enc, keep = world["eng"][name], world["enc"][name], []
    eng.stream_prefix_reset(-1, _stream())
    feed(eng, enc, LENS, split, beam, weights, keep)
    for b, n in enumerate(LENS):
        assert eng.stream_prefix_size(b) == (beam, n, n + 1)
        assert_same(read(eng, b), one_call(world, name, b, n, beam, weights), f"{name} beam {beam} {split} utterance {b}")
    assert beam == 1 or max(len(t) for t, _ in read(eng, 0)[0]) > 1, "no symbol in any hypothesis: the case shows nothing"


@pytest.mark.parametrize("split", sorted(SPLITS))
def test_split_invariance_whole_vocabulary(split, world):
    """vocabulary 8, beam 8: the top-k takes the whole vocabulary"""
    eng, enc, keep = world["eng"]["v8"], world["enc"]["v8"], []
    eng.stream_prefix_reset(-1, _stream())
    feed(eng, enc, LENS, split, 8, W_FUSED, keep)
    for b, n in enumerate(LENS):
        assert_same(read(eng, b), one_call(world, "v8", b, n, 8, W_FUSED), f"v8 {split} utterance {b}")


# ---- 2. partial reads --------------------------------------------------------------------------------------------------------------------
def test_partial_reads(world):
    """after every 1-frame call the read is the one-call search over the frames so far; reading twice gives the same bytes and does not
    disturb the next frame"""
    eng, enc, keep, beam = world["eng"]["full"], world["enc"]["full"], [], 5
    eng.stream_prefix_reset(-1, _stream())
    lens = (9, 6)
    assert_same(read(eng, 0), one_call(world, "full", 0, 0, beam, W_FUSED), "a fresh slot")
    assert read(eng, 0)[0] == [([BLANK], 0.0)] and eng.stream_prefix_size(0) == (1, 0, 1)
    for t in range(max(lens)):
        rows = [b for b, n in enumerate(lens) if n > t]
        adv(eng, rows, [enc[b, t:t + 1] for b in rows], beam, W_FUSED, keep)
        for b, n in enumerate(lens):
            first, again = read(eng, b), read(eng, b)
            assert_same(first, one_call(world, "full", b, min(n, t + 1), beam, W_FUSED), f"frame {t} utterance {b}")
            assert_same(again, first, f"frame {t} utterance {b}, second read")


# ---- 3. slot independence and set parity ---------------------------------------------------------------------------------------------
def test_slot_independence_and_set_parity(world):
    """three slots; one idle while two advance in one call, those two having walked an odd and an even number of frames (so their
    current buffer sets differ); one opened two calls late.  Each slot equals its run in a one-slot context, the idle slot reads as
    before, and rnnt_stream_prefix_reset restarts one slot only."""
    eng, solo, enc, keep, beam = world["eng"]["full"], world["eng"]["solo"], world["enc"]["full"], [], 4
    s = _stream()
    eng.reset(3, s)
    solo.reset(1, s)
    eng.stream_open(0, s)
    eng.stream_open(1, s)
    adv(eng, [0], [enc[0, 0:2]], beam, W_FUSED, keep)                                # slot 0: 2 frames (even)
    adv(eng, [1], [enc[1, 0:1]], beam, W_FUSED, keep)                                # slot 1: 1 frame
    eng.stream_open(2, s)                                                            # two calls late
    adv(eng, [2], [enc[2, 0:3]], beam, W_FUSED, keep)                                # slot 2: 3 frames (odd)
    idle = read(eng, 1)
    adv(eng, [2, 0], [enc[2, 3:5], enc[0, 2:4]], beam, W_FUSED, keep)                # odd and even in one call, slot 1 idle
    adv(eng, [0, 2], [enc[0, 4:7], enc[2, 5:8]], beam, W_FUSED, keep)                # and again after an even step, 3 frames
    assert_same(read(eng, 1), idle, "the idle slot")
    assert_same(idle, one_call(world, "full", 1, 1, beam, W_FUSED), "the idle slot against the one-call search")
    for slot, cuts in ((0, (0, 2, 4, 7)), (2, (0, 3, 5, 8))):
        solo.stream_prefix_reset(0, s)
        for a, b in zip(cuts, cuts[1:]):
            adv(solo, [0], [enc[slot, a:b]], beam, W_FUSED, keep)
        assert solo.stream_prefix_size(0) == eng.stream_prefix_size(slot) == (beam, cuts[-1], cuts[-1] + 1)
        assert_same(read(eng, slot), read(solo, 0), f"slot {slot} against a one-slot context")
        assert_same(read(eng, slot), one_call(world, "full", slot, cuts[-1], beam, W_FUSED), f"slot {slot} against the one-call search")
    two = read(eng, 2)
    eng.stream_prefix_reset(0, s)
    assert eng.stream_prefix_size(0) == (1, 0, 1) and read(eng, 0)[0] == [([BLANK], 0.0)] and not read(eng, 0)[1].any()
    assert_same(read(eng, 2), two, "the neighbour of the reset slot")
    assert_same(read(eng, 1), idle, "the idle slot after the reset")
    adv(eng, [0], [enc[1, 0:9]], 9, W_RNNT, keep)                                    # another beam, other weights: accepted after the reset
    assert_same(read(eng, 0), one_call(world, "full", 1, 9, 9, W_RNNT), "the reset slot")
    adv(eng, [2, 1], [enc[2, 8:12], enc[1, 1:5]], beam, W_FUSED, keep)               # the others go on
    assert_same(read(eng, 2), one_call(world, "full", 2, 12, beam, W_FUSED), "slot 2, finished")
    assert_same(read(eng, 1), one_call(world, "full", 1, 5, beam, W_FUSED), "slot 1, resumed")
    eng.stream_open(1, s)                                                            # rnnt_stream_open restarts its slot's search alone
    assert eng.stream_prefix_size(1) == (1, 0, 1) and eng.stream_prefix_size(2) == (beam, 12, 13)
    eng.reset(3, s)                                                                  # rnnt_streams_reset all of them
    assert [eng.stream_prefix_size(b) for b in range(3)] == [(1, 0, 1)] * 3 and read(eng, 2)[0] == [([BLANK], 0.0)]


# ---- 4. other state untouched ----------------------------------------------------------------------------------------------------------
def test_other_state_is_left_alone(world):
    """greedy tokens, the RNN-T beam, the CTC prefix hypotheses, the caches and predictor states of the slots, and a
    rnnt_prefix_beam_decode result taken before and after: all unchanged by pool prefix calls on the same slots of the same context"""
    eng, enc, x, keep = world["eng"]["full"], world["enc"]["full"], world["x"], []
    s = _stream()
    eng.reset(3, s)
    for b in range(3):
        eng.stream_open(b, s)
    rows = [x[b:b + 1, :32].contiguous() for b in range(3)]
    eng.pool_chunk([0], rows[0].data_ptr(), 32, [0], [0], True, s)
    eng.pool_chunk_beam([1], rows[1].data_ptr(), 32, [0], [0], 4, s)
    eng.pool_chunk_ctc_prefix([2], rows[2].data_ptr(), 32, [0], [0], 4, False, s)

    def getters():
        out = [np.array(eng.stream_tokens(0, 0, s)), *eng.stream_beam_states(1, s), np.array([v for _, v in eng.stream_beam(1, s)]),
               np.array(sum([t for t, _ in eng.stream_beam(1, s)], [])), *eng.stream_ctc_prefix(2, True, True, stream=s)[1]]
        for b in range(3):
            h, c, tok = eng.predictor_state(b, s)
            out += [h, c, np.array([tok]), eng.att_cache(b, s), eng.cnn_cache(b, s)]
        hyps, h, c = eng.prefix_beam_decode(enc.data_ptr(), [15, 0, 7], 3, 15, 6, 0.3, 0.7, True, s)
        out += [h, c, np.array([v for row in hyps for _, v in row]), np.array(sum([t for row in hyps for t, _ in row], []))]
        return out
    before = getters()
    eng.stream_prefix_reset(-1, s)
    feed(eng, enc, LENS, "uneven", 6, W_FUSED, keep)
    for b, n in enumerate(LENS):
        assert_same(read(eng, b), one_call(world, "full", b, n, 6, W_FUSED), f"utterance {b}")
    after = getters()
    assert len(before) == len(after) and all(np.asarray(p).shape == np.asarray(q).shape and np.asarray(p).tobytes() == np.asarray(q).tobytes()
                                             for p, q in zip(before, after))
    for b, n in enumerate(LENS):                                                     # and the pool searches outlived the getters
        assert_same(read(eng, b), one_call(world, "full", b, n, 6, W_FUSED), f"utterance {b} after the getters")


# ---- 5. chunk form -------------------------------------------------------------------------------------------------------------------------
CHUNKS = (16, 16, 7, 16, 24)            # t' = 3, 3, 1, 3, 5
LATE = 2                                # the second slot opens before call 2 and takes the last three chunks


def _pool_engine(sd, slots, group):
    eng = _create(group, max_streams=slots, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=T.VOCAB,
                  blank_id=BLANK, max_beam=4)
    eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope="module")
def pools(world):
    pool, solo = _pool_engine(world["sd"], 2, 4), _pool_engine(world["sd"], 1, None)
    xs = [torch.from_numpy(T.synth_fbank(1, sum(CHUNKS), seed=seed))[0].cuda() for seed in (45, 46)]
    yield {"pool": pool, "solo": solo, "xs": xs}
    pool.close()
    solo.close()


def _decode_frames(eng, frames, beam, weights):
    n = frames.size(0)
    hyps, h, c = eng.prefix_beam_decode(frames[None].contiguous().data_ptr(), [n], 1, n, beam, weights[0], weights[1], True, _stream())
    return hyps[0], h[0, :len(hyps[0])], c[0, :len(hyps[0])]


def test_chunk_form(pools):
    """two slots through rnnt_pool_chunk_prefix, with a 7-frame chunk (t' = 1) and a 24-frame tail; slot 1 keeps its frames and is
    opened two calls late.  frames_out is right and each slot's final hypotheses are bitwise rnnt_prefix_beam_decode over the frames
    the slot consumed: its own kept frames for slot 1, for slot 0 the frames a one-slot context keeps for the same chunks."""
    eng, solo, xs, beam = pools["pool"], pools["solo"], pools["xs"], 5
    s = _stream()
    keep = []
    starts = np.concatenate([[0], np.cumsum(CHUNKS)])

    def run(e, slot_of_utt, late):
        e.reset(max(slot_of_utt.values()) + 1, s)
        offs = {u: 0 for u in slot_of_utt}
        for k, T_ in enumerate(CHUNKS):
            if k == 0 or k == late:
                for u, slot in slot_of_utt.items():
                    if (late if u == 1 else 0) == k:
                        e.stream_open(slot, s)
                        if u == 1 or e is solo:
                            e.stream_keep_frames(slot, True, s)
            utts = [u for u in slot_of_utt if k >= (late if u == 1 else 0)]
            # utterance 1 is fed chunks LATE.. of its own audio, so both rows of a call have the call's length
            x = torch.stack([xs[u][starts[k]:starts[k] + T_] for u in utts], 0).contiguous()
            keep.append(x)
            o = [offs[u] for u in utts]
            got = e.pool_chunk_prefix([slot_of_utt[u] for u in utts], x.data_ptr(), T_, o, o, beam, 0.3, 0.7, s)
            assert got == ((T_ - 3) // 2 + 1 - 3) // 2 + 1
            for u in utts:
                offs[u] += T_ // 4
    run(eng, {0: 0, 1: 1}, LATE)
    both = [read(eng, 0), read(eng, 1)]
    assert eng.stream_prefix_size(0)[1] == 15 and eng.stream_prefix_size(1)[1] == 9
    kept1 = eng.stream_frames(1, 0, s)
    assert kept1.shape == (9, 256)
    assert_same(both[1], _decode_frames(eng, kept1, beam, W_FUSED), "slot 1 against the one-call search over its kept frames")
    with pytest.raises(RnntError):
        eng.stream_frames(0, 0, s)                                                   # slot 0 keeps none
    run(solo, {0: 0}, LATE)
    kept0 = solo.stream_frames(0, 0, s)
    assert kept0.shape == (15, 256)
    assert_same(read(solo, 0), both[0], "slot 0 against a one-slot context")
    assert_same(both[0], _decode_frames(eng, kept0, beam, W_FUSED), "slot 0 against the one-call search over the frames it consumed")
    assert max(len(t) for t, _ in both[0][0]) > 1


def test_two_launches_per_frame_whatever_n_active(pools):
    """launches of a chunk-form call = those of the encoder-only call of the same rows (its scatter launch aside), of rnnt_ctc_logprobs
    over the compact rows, and 2 * t' for the search"""
    eng, xs = pools["pool"], pools["xs"]
    s = _stream()
    launches = lambda: eng.counters()[0]                                              # noqa: E731
    scratch = torch.empty(2 * 5, T.VOCAB, device="cuda")
    rows_in = torch.zeros(2 * 5, 256, device="cuda")
    for slots, T_ in (([0], 16), ([0, 1], 16), ([1, 0], 24), ([1], 7)):
        tq = ((T_ - 3) // 2 + 1 - 3) // 2 + 1
        x = torch.stack([xs[b][:T_] for b in slots], 0).contiguous()
        zero = [0] * len(slots)
        eng.reset(2, s)
        for b in slots:
            eng.stream_open(b, s)
        eng.pool_chunk_prefix(slots, x.data_ptr(), T_, zero, zero, 4, 0.3, 0.7, s)   # the state exists from here on
        eng.reset(2, s)
        for b in slots:
            eng.stream_open(b, s)
        n0 = launches()
        eng.pool_chunk(slots, x.data_ptr(), T_, zero, zero, False, s)
        n_enc = launches() - n0 - 1                                                  # pool_scatter_frames is the encoder-only form's own
        eng.frames_discard(s)
        n0 = launches()
        eng.ctc_logprobs(rows_in.data_ptr(), len(slots) * tq, scratch.data_ptr(), s)
        n_ctc = launches() - n0
        eng.reset(2, s)
        for b in slots:
            eng.stream_open(b, s)
        n0 = launches()
        assert eng.pool_chunk_prefix(slots, x.data_ptr(), T_, zero, zero, 4, 0.3, 0.7, s) == tq
        assert launches() - n0 - n_enc - n_ctc == 2 * tq, (slots, T_, launches() - n0, n_enc, n_ctc)
        n0 = launches()
        rows = torch.zeros(len(slots), 2, 256, device="cuda")
        eng.pool_prefix_frames(slots, rows.data_ptr(), 2, 4, 0.3, 0.7, s)            # the seam form: enc_ffn + CTC + 2 per frame
        assert launches() - n0 == 1 + n_ctc + 4, (slots, launches() - n0)
        torch.cuda.synchronize()


# ---- 6. against the CPU oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [PB.E2E[2], PB.E2E[3]], ids=lambda c: "s%d_f%d_v%d_b%d" % c[:4])
def test_matches_cpu_oracle(case, np_state_dict):
    """rnnt_encoder_full's frames through the seam in chunks of 3 against oracle.rnnt_oracle.prefix_beam_search_full under the
    tolerances of test_prefix_beam.py: tokens exact, scores within 2e-3, h within 1e-3"""
    seed, frames, valid, beam, _ = case
    m = PB.model(np_state_dict, seed)
    eng, s = m._engine, _stream()
    x = PB.fbank(case).cuda().contiguous()
    tq = ((frames - 3) // 2 + 1 - 3) // 2 + 1
    enc = torch.empty(1, tq, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [valid], 1, frames, enc.data_ptr(), s) == tq
    eng.stream_prefix_reset(-1, s)
    keep = []
    for a in range(0, tq, 3):
        adv(eng, [0], [enc[0, a:min(a + 3, tq)]], beam, W_FUSED, keep)
    hyps, h, _ = read(eng, 0)
    want = PB.oracle(np_state_dict, case)
    print(case, [v for _, v in hyps], [v for _, v, _ in want])
    PB.assert_matches_oracle(hyps, h, want)


# ---- 7. refusals change nothing ---------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(world, np_state_dict):
    """each refusal of the seam form, of the chunk form and of the read is decided before any launch: the launch counter, the slots'
    frames and what they compute next are as if the call had not been made"""
    sd, enc, keep, beam = world["sd"], world["enc"]["full"], [], 4
    eng = _engine(sd, 3, frames=8)                                                   # a small max_cache_frames
    s = _stream()
    try:
        eng.reset(3, s)
        for b in range(3):
            eng.stream_open(b, s)
        adv(eng, [0, 1], [enc[0, 0:2], enc[1, 0:2]], beam, W_FUSED, keep)           # slots 0 and 1 two frames in, slot 2 fresh
        rows = enc[:2, 2:4].contiguous()
        launches = lambda: eng.counters()[0]                                          # noqa: E731
        sizes = lambda: [eng.stream_prefix_size(k) for k in range(3)]                 # noqa: E731
        snap = [read(eng, k) for k in range(3)]

        def refused(status, slots, t=1, beam_size=beam, cw=0.3, tw=0.7, ptr=rows.data_ptr()):
            f0, n0 = sizes(), launches()
            with pytest.raises(RnntError) as e:
                eng.pool_prefix_frames(slots, ptr, t, beam_size, cw, tw, s)
            assert e.value.status == status, e.value
            assert launches() == n0 and sizes() == f0

        refused(ERR_ARG, [0], ptr=None)
        refused(ERR_ARG, [0, 0])
        refused(ERR_ARG, [3])
        refused(ERR_ARG, [-1])
        refused(ERR_ARG, [0], t=0)
        refused(ERR_ARG, [2], beam_size=0)
        refused(ERR_ARG, [2], beam_size=17)
        refused(ERR_ARG, [2], cw=-0.1)
        refused(ERR_ARG, [2], tw=-1.0)
        refused(ERR_ARG, [2], cw=0.0, tw=0.0)
        refused(ERR_ARG, [2], cw=float("nan"))
        refused(ERR_ARG, [0], beam_size=beam + 1)                                    # differs from the search in progress
        refused(ERR_ARG, [0], cw=0.2)
        refused(ERR_ARG, [0], tw=0.8)
        refused(ERR_ARG, [2, 0], beam_size=beam + 1)                                 # one bad slot refuses the whole call: slot 2 stays fresh
        refused(ERR_SHAPE, [0], t=7)                                                 # 2 + 7 > 8
        refused(ERR_SHAPE, [2, 0], t=7)
        one = np.zeros(4, np.int32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                              # noqa: E731
        n0 = launches()
        assert eng.lib.rnnt_pool_prefix_frames(eng.ctx, 1, None, rows.data_ptr(), 1, beam, 0.3, 0.7, s) == ERR_ARG
        assert eng.lib.rnnt_pool_prefix_frames(eng.ctx, 0, p(one), rows.data_ptr(), 1, beam, 0.3, 0.7, s) == ERR_ARG
        assert eng.lib.rnnt_pool_prefix_frames(eng.ctx, 4, p(one), rows.data_ptr(), 1, beam, 0.3, 0.7, s) == ERR_ARG
        assert eng.lib.rnnt_stream_prefix_reset(eng.ctx, 3, s) == ERR_ARG and eng.lib.rnnt_stream_prefix_reset(eng.ctx, -2, s) == ERR_ARG
        # the read: room for the slot's beam and 1 + its frames, both states or neither, no null outputs
        nh, ln, sc = np.zeros(3, np.int32), np.zeros(beam, np.int32), np.zeros(beam, np.float64)
        tk, hc = np.zeros((beam, 8), np.int32), np.zeros((beam, 256), np.float32)
        get = eng.lib.rnnt_stream_get_prefix
        assert get(eng.ctx, 0, beam - 1, 8, p(nh), p(ln), p(tk), p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 2, p(nh), p(ln), p(tk), p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, p(nh), p(ln), p(tk), p(sc), p(hc), None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, p(nh), p(ln), p(tk), p(sc), None, p(hc), s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, None, p(ln), p(tk), p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, p(nh), None, p(tk), p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, p(nh), p(ln), None, p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, beam, 8, p(nh), p(ln), p(tk), None, None, None, s) == ERR_ARG
        assert get(eng.ctx, 3, beam, 8, p(nh), p(ln), p(tk), p(sc), None, None, s) == ERR_ARG
        assert get(eng.ctx, 0, 0, 0, p(nh), None, None, None, None, None, s) == 0 and nh.tolist() == [beam, 2, 3]     # the size query
        assert launches() == n0
        # the chunk form: its own refusals and rnnt_pool_chunk's, one caused by another listed slot included
        x = world["x"][:2, :16].contiguous()

        def chunk_refused(status, slots=(2,), frames=16, beam_size=beam, cw=0.3, tw=0.7, offs=None):
            f0, n0 = sizes(), launches()
            o = list(offs) if offs is not None else [0] * len(slots)
            with pytest.raises(RnntError) as e:
                eng.pool_chunk_prefix(list(slots), x.data_ptr(), frames, o, o, beam_size, cw, tw, s)
            assert e.value.status == status, e.value
            assert launches() == n0 and sizes() == f0
        chunk_refused(ERR_ARG, beam_size=0)
        chunk_refused(ERR_ARG, cw=0.0, tw=0.0)
        chunk_refused(ERR_ARG, slots=(2, 2))
        chunk_refused(ERR_ARG, slots=(3,))
        chunk_refused(ERR_SHAPE, frames=6)
        chunk_refused(ERR_ARG, slots=(2, 0), beam_size=beam + 1)                     # slot 0's search in progress refuses slot 2's call too
        chunk_refused(ERR_ARG, slots=(2, 1), tw=0.6)
        chunk_refused(ERR_SHAPE, slots=(2, 0), frames=32)                            # slot 0: 2 + 7 > 8 frames
        chunk_refused(ERR_SHAPE, slots=(2, 0), offs=(0, 6000))                       # slot 0's positional window leaves the table
        eng.pool_chunk([2], x.data_ptr(), 16, [0], [0], False, s)                    # frames still buffered
        chunk_refused(ERR_STATE, slots=(1,))
        eng.frames_discard(s)
        for k in range(3):
            assert_same(read(eng, k), snap[k], f"slot {k} after the refusals")
        # and the slots go on as if nothing had been: slot 0 to its capacity, slot 2 from the start
        adv(eng, [0, 2], [enc[0, 2:8], enc[2, 0:6]], beam, W_FUSED, keep)
        refused(ERR_SHAPE, [0], t=1)                                                 # full: 8 + 1 > 8
        assert_same(read(eng, 0), one_call(world, "full", 0, 8, beam, W_FUSED), "slot 0 after the refusals")
        assert_same(read(eng, 2), one_call(world, "full", 2, 6, beam, W_FUSED), "slot 2 after the refusals")
    finally:
        eng.close()
    no_ctc, v8 = world["eng"]["no_ctc"], world["eng"]["v8"]
    for e_, args, status in ((no_ctc, (1, 0.3, 0.7), ERR_STATE), (v8, (9, 0.3, 0.7), ERR_ARG)):
        e_.stream_prefix_reset(-1, s)
        n0 = e_.counters()[0]
        with pytest.raises(RnntError) as err:                                        # ctc_weight > 0 without the head; beam > vocabulary
            e_.pool_prefix_frames([0], enc[:1, :1].contiguous().data_ptr(), 1, *args, s)
        assert err.value.status == status and e_.counters()[0] == n0 and e_.stream_prefix_size(0) == (1, 0, 1)
    big = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=600, max_beam=0)
    try:
        with pytest.raises(RnntError) as err:                                        # weights not finalized
            big.pool_prefix_frames([0], enc[:1, :1].contiguous().data_ptr(), 1, 2, 0.3, 0.7, s)
        assert err.value.status == ERR_STATE
        big.load_state_dict(T.make_state_dict(0, vocab=600))
        with pytest.raises(RnntError) as err:                                        # vocabulary > 512
            big.pool_prefix_frames([0], enc[:1, :1].contiguous().data_ptr(), 1, 2, 0.3, 0.7, s)
        assert err.value.status == ERR_ARG
    finally:
        big.close()


# ---- 8. StreamPool end to end -------------------------------------------------------------------------------------------------------------
def test_stream_pool_end_to_end(world, pools):
    """a greedy slot, an RNN-T beam slot, a CTC prefix slot and a transducer prefix slot side by side: the first three are bitwise what
    they are without the fourth; the prefix slot's close() is rnnt_prefix_beam_decode over its kept frames; rescore() picks what the
    same selection over rnnt_transducer_nll_nbest picks; and a prefix slot fed audio gives what the same slot fed its frames gives"""
    from ctc_vr_amd.online_rnnt_model import StreamPool
    xs, beam, n = pools["xs"], 5, 4
    pool = StreamPool(world["sd"], 4, vocab_size=T.VOCAB, blank_id=BLANK, max_chunk_frames=64, max_cache_frames=256, max_tokens=512, max_beam=4)
    try:
        def run(with_prefix):
            pool.reset()
            g, b, c = pool.open(), pool.open(beam_size=4), pool.open(ctc_prefix_beam=4)
            p = pool.open(prefix_beam=beam, keep_frames=True) if with_prefix else None
            inc = []
            for k in range(n):
                pool.feed(g, xs[0][k * 16:(k + 1) * 16])
                pool.feed(b, xs[1][k * 16:(k + 1) * 16])
                pool.feed(c, xs[1][k * 16:(k + 1) * 16])
                if with_prefix:
                    pool.feed(p, xs[1][k * 16:(k + 1) * 16])
                inc.append(pool.step())
            extra = None
            if with_prefix:
                mid = pool.prefix_hyps(p)
                frames = pool.frames(p)
                res = pool.rescore([p], 0.3, 0.7)[p]
                extra = (mid, frames, res, pool.close(p))
            beams = [(h.tokens, h.log_prob) for h in pool.close(b)]
            return (inc, pool.close(g), beams, pool.close(c)), extra
        alone, _ = run(False)
        beside, (mid, frames, (best, rows), final) = run(True)
        assert beside == alone, "the greedy, RNN-T beam or CTC prefix slot changed beside a transducer prefix slot"
        assert len(alone[2]) > 1 and len(alone[3]) > 0
        eng, s = pool.engine, _stream()
        assert frames.shape == (3 * n, 256)
        want = _decode_frames(eng, frames, beam, W_FUSED)[0]
        assert final == mid and [t for t, _ in final] == [t for t, _ in want]
        assert np.array_equal(bits(np.array([v for _, v in final])), bits(np.array([v for _, v in want])))
        # the second pass: first pass = the hypotheses without the leading blank, first score = the search's score
        assert [r[0] for r in rows] == [t[1:] for t, _ in final] and [r[1] for r in rows] == [v for _, v in final]
        nh, hl, ht = pack_nbest([[t[1:] for t, _ in final]])
        nll = eng.transducer_nll_nbest(frames[None].contiguous().data_ptr(), [3 * n], nh, hl, ht, 1, 3 * n, None, s)[0, :nh[0]]
        want_best, want_total = rescore_select([v for _, v in final], nll, 0.3, 0.7)
        assert best == want_best and np.array_equal(bits(np.array([r[3] for r in rows])), bits(want_total))
        assert np.array_equal(bits(np.array([-r[2] for r in rows])), bits(nll))
        # audio in: the frames rnnt_fbank gives for the waveform, fed in chunk_frames pieces, against the packets of feed_wave
        wave = torch.randn(16 * 512 * 3, generator=torch.Generator().manual_seed(7)).cuda() * 0.1
        fb = torch.empty(1, 1 + wave.numel() // 512, 80, device="cuda")
        eng.fbank(wave[None].contiguous().data_ptr(), 1, wave.numel(), 16000, fb.data_ptr(), stream=s)
        pool.reset()
        a = pool.open(prefix_beam=beam)
        for k in range(0, fb.size(1), pool.chunk_frames):
            pool.feed(a, fb[0, k:k + pool.chunk_frames].contiguous())
            pool.step()
        by_frames = pool.close(a)
        pool.reset()
        a = pool.open(prefix_beam=beam)
        cuts = [0, 5000, 5001, 12345, wave.numel()]
        for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            pool.feed_wave(a, wave[lo:hi].contiguous(), final=i == len(cuts) - 2)
            pool.step()
        by_wave = pool.close(a)
        assert len(by_frames) == beam and by_wave == by_frames
    finally:
        pool.engine.close()
