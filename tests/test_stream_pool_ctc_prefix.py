"""CTC prefix beam search per slot of the stream pool on the device (rnnt_pool_ctc_prefix_logprobs, rnnt_pool_chunk_ctc_prefix,
rnnt_stream_get_ctc_prefix, rnnt_stream_ctc_prefix_reset; StreamPool.open(ctc_prefix_beam=...)).

The contract under test: a search fed in pieces is, bit for bit, the one-launch search (rnnt_ctc_prefix_beam_logprobs) over the same
device rows, whatever the split.  Both run the same device function on the same numbers, so results are compared as bytes; the only
tolerance here (SCORE_TOL of ctc_prefix_cases.py) is for final = 0 scores against the Python restatement.  Needs a real MI355X.
Nothing here provokes a device fault: every refusal is a host-side argument check."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntEngine, RnntError, context_walk_host
import ctc_prefix_cases as C

pytestmark = pytest.mark.gpu

GOLD = C.golden_cases()
CASES = {**{k: v[0] for k, v in GOLD.items()}, **C.crafted_cases()}
MAX_FRAMES = 64               # max_cache_frames of the weightless contexts: every case is shorter
SPLITS = {"ones": (), "one_and_rest": (1,), "uneven": (2, 3)}     # chunk sizes taken first; "ones" is all 1, the others then take the rest


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def engines():
    """Contexts without weights, one per (vocabulary, blank, slots, max_cache_frames)."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    cache = {}

    def get(vocab, blank, slots=3, frames=MAX_FRAMES):
        key = (vocab, blank, slots, frames)
        if key not in cache:
            cache[key] = RnntEngine(max_streams=slots, max_chunk_frames=16, max_cache_frames=frames, max_enc_frames=16, vocab_size=vocab,
                                    blank_id=blank, max_beam=0)
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def chunks_of(length, split):
    """the chunk lengths of an utterance of `length` frames under a split"""
    out, left = [], length
    for want in SPLITS[split]:
        if left > 0:
            out.append(min(want, left))
            left -= out[-1]
    if split == "ones":
        return [1] * length
    return out + ([left] if left > 0 else [])


def same_bits(x, y):
    """bitwise equal; token / time arrays of different widths agree on the common part and are zero beyond it"""
    if x.ndim == 3:
        n = min(x.shape[2], y.shape[2])
        if x[..., n:].any() or y[..., n:].any():
            return False
        x, y = np.ascontiguousarray(x[..., :n]), np.ascontiguousarray(y[..., :n])
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def one_launch(eng, lp_d, lens, beam, use_ctx):
    """the oracle: rnnt_ctc_prefix_beam_logprobs over the device rows lp_d [B, T, V], raw arrays"""
    return eng.ctc_prefix_beam_logprobs(lp_d.data_ptr(), lens, lp_d.size(0), lp_d.size(1), beam, use_ctx, True, _stream())[1]


def read(eng, slot, final, beam, cap):
    hyps, raw, frames = eng.stream_ctc_prefix(slot, final, True, beam, cap, _stream())
    return hyps, raw, frames


def assert_row(raw, want, b, what):
    """the B = 1 arrays of one slot against row b of a batch's arrays, as bytes"""
    for k, (x, y) in enumerate(zip(raw, want)):
        assert same_bits(x, y[b:b + 1]), f"{what}: array {k} (n_hyp, lens, tokens, times, scores, context scores) differs\n{x}\n{y[b:b + 1]}"


def feed(eng, lp_d, lens, split, beam, use_ctx, slots=None, upto=None):
    """every utterance b of lp_d through slot slots[b] in the split's chunks; the utterances whose k-th chunks have one length share a call"""
    B = lp_d.size(0)
    slots = list(range(B)) if slots is None else slots
    plan = [chunks_of(n, split) for n in lens]
    at, keep = [0] * B, []
    for k in range(max((len(p) for p in plan), default=0)):
        for t in sorted({p[k] for p in plan if k < len(p)}):
            rows = [b for b in range(B) if k < len(plan[b]) and plan[b][k] == t]
            x = torch.stack([lp_d[b, at[b]:at[b] + t] for b in rows], 0).contiguous()
            keep.append(x)                                        # the call does not synchronise: the rows live until the read
            eng.pool_ctc_prefix_logprobs([slots[b] for b in rows], x.data_ptr(), t, beam, use_ctx, _stream())
            for b in rows:
                at[b] += t
    return keep


@pytest.mark.parametrize("split", sorted(SPLITS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_invariance(name, split, engines):
    lp, lens, blank, beam, phrases, score = CASES[name]
    assert lp.shape[1] <= MAX_FRAMES
    eng = engines(lp.shape[2], blank)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    eng.context_set(phrases or [], score)
    want = one_launch(eng, lp_d, lens, beam, bool(phrases))
    eng.stream_ctc_prefix_reset(-1, _stream())
    keep = feed(eng, lp_d, lens, split, beam, bool(phrases))
    for b, n in enumerate(lens):
        _, raw, frames = read(eng, b, True, beam, want[2].shape[2])
        assert frames == n
        assert_row(raw, want, b, f"{name} {split} utterance {b}")
        C.assert_zero_fill(raw)
    del keep


@pytest.mark.parametrize("name", ["ragged_ctx", "ragged_plain"])
def test_partial_reads(name, engines):
    """after every 1-frame call final = 1 is the one-launch search over the frames so far; final = 0 has the same hypotheses with the
    running context scores (exactly the walk's sums) and, without a graph, the same bytes; reading disturbs nothing"""
    lp, lens, blank, beam, phrases, score = CASES[name]
    eng = engines(lp.shape[2], blank)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    eng.context_set(phrases or [], score)
    g = T.context_graph_ref(phrases, score) if phrases else None
    eng.stream_ctc_prefix_reset(-1, _stream())
    keep = []
    for t in range(max(lens)):
        rows = [b for b, n in enumerate(lens) if n > t]
        x = torch.stack([lp_d[b, t:t + 1] for b in rows], 0).contiguous()
        keep.append(x)
        eng.pool_ctc_prefix_logprobs(rows, x.data_ptr(), 1, beam, bool(phrases), _stream())
        sofar = [min(n, t + 1) for n in lens]
        want = one_launch(eng, lp_d, sofar, beam, bool(phrases))
        for b in range(len(lens)):
            fin_h, fin, frames = read(eng, b, True, beam, want[2].shape[2])
            assert frames == sofar[b]
            assert_row(fin, want, b, f"{name} frame {t} utterance {b}")
            run_h, run, _ = read(eng, b, False, beam, want[2].shape[2])
            assert all(same_bits(x, y) for x, y in zip(run[:4], fin[:4])), "final = 0: hypotheses, lengths, tokens, times and order"
            if not phrases:
                assert all(same_bits(x, y) for x, y in zip(run, fin)), "without a graph final = 0 is final = 1"
                continue
            ref = T.ctc_prefix_beam_ref(lp[b], sofar[b], blank, beam, g, finalize=False)[0]
            assert [h[0] for h in run_h] == [h[0] for h in ref]
            for (tok, sc, _, cs), (_, rsc, _, _) in zip(run_h, ref):
                want_cs = 0.0
                for s in context_walk_host(phrases, score, tok)[0]:
                    want_cs += float(s)
                assert cs == want_cs, (t, b, tok)
                assert sc == rsc or abs(sc - rsc) <= C.SCORE_TOL
    full = one_launch(eng, lp_d, lens, beam, bool(phrases))
    for b in range(len(lens)):
        assert_row(read(eng, b, True, beam, full[2].shape[2])[1], full, b, f"{name} after the reads, utterance {b}")


def test_slot_independence(engines):
    """three slots at different positions, one idle while two advance in one call: the idle slot reads as before (and later finishes
    as if nothing had happened), each active slot reads as in a context that holds only that slot.  The library has no call that
    returns a slot's stored record, so the record is observed only through the packer: its final = 0 and final = 1 reads, which show
    every field but the split of score() into s and ns and the Viterbi pair, and the slot's later frames, which depend on those."""
    lp, lens, blank, beam, phrases, score = CASES["ragged_ctx"]
    eng, solo = engines(lp.shape[2], blank), engines(lp.shape[2], blank, slots=1)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    for e in (eng, solo):
        e.context_set(phrases, score)
        e.stream_ctc_prefix_reset(-1, _stream())
    cap = max(lens)

    def adv(e, slots, rows, t):
        x = torch.stack(rows, 0).contiguous()
        e.pool_ctc_prefix_logprobs(slots, x.data_ptr(), t, beam, True, _stream())
        return x
    keep = [adv(eng, [0], [lp_d[0, 0:2]], 2), adv(eng, [1], [lp_d[1, 0:1]], 1), adv(eng, [2], [lp_d[2, 0:3]], 3)]
    idle = [read(eng, 1, f, beam, cap)[1:] for f in (False, True)]
    keep.append(adv(eng, [2, 0], [lp_d[2, 3:5], lp_d[0, 2:4]], 2))                 # slot 1 idle
    for f, (raw, frames) in zip((False, True), idle):
        again, frames2 = read(eng, 1, f, beam, cap)[1:]
        assert frames2 == frames == 1 and all(same_bits(x, y) for x, y in zip(again, raw)), "the idle slot changed"
    for slot, utt, cuts in ((0, 0, (0, 2, 4)), (2, 2, (0, 3, 5))):
        solo.stream_ctc_prefix_reset(0, _stream())
        for a, b in zip(cuts, cuts[1:]):
            keep.append(adv(solo, [0], [lp_d[utt, a:b]], b - a))
        for f in (False, True):
            mine, alone = read(eng, slot, f, beam, cap), read(solo, 0, f, beam, cap)
            assert mine[2] == alone[2] == cuts[-1] and all(same_bits(x, y) for x, y in zip(mine[1], alone[1])), (slot, f)
    keep.append(adv(eng, [1], [lp_d[1, 1:lens[1]]], lens[1] - 1))
    want = one_launch(eng, lp_d, lens, beam, True)
    assert_row(read(eng, 1, True, beam, want[2].shape[2])[1], want, 1, "the idle slot, finished")


def test_fresh_slot_reads(engines):
    """a slot that has walked no frames has fixed no use_context.  Its final = 1 read is the one-launch search over no frames under
    the graph that is set: context score -0.0 with a graph (finalize of the root, as use_context = 1 returns it), +0.0 without one;
    final = 0 never reads the graph.  The size query gives the room a read needs without a launch."""
    lp, lens, blank, beam, phrases, score = CASES["ragged_ctx"]
    eng = engines(lp.shape[2], blank)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    s = _stream()
    for graph in (phrases, []):
        eng.context_set(graph, score)
        eng.stream_ctc_prefix_reset(-1, s)
        want = one_launch(eng, lp_d[:1], [0], beam, bool(graph))
        hyps, raw, frames = read(eng, 0, True, beam, 1)
        assert frames == 0 and hyps == [([], 0.0, [], 0.0)]
        assert_row(raw, want, 0, f"fresh slot, graph {bool(graph)}")
        assert bool(np.signbit(raw[5][0, 0])) == bool(graph) and not np.signbit(raw[4][0, 0])
        run = read(eng, 0, False, beam, 1)[1]
        assert not np.signbit(run[5][0, 0]) and all(same_bits(x, y) for x, y in zip(run[:5], raw[:5]))
    eng.context_set(phrases, score)
    n0 = eng.counters()[0]
    assert eng.stream_ctc_prefix(1, True, True, stream=s)[1][1].shape == (1, 1)           # sized by the query: one row for a fresh slot
    x = lp_d[1:2, :3].contiguous()
    eng.pool_ctc_prefix_logprobs([1], x.data_ptr(), 3, beam, True, s)
    n1 = eng.counters()[0]
    need, frames = ctypes.c_int32(0), ctypes.c_int32(0)
    assert eng.lib.rnnt_stream_get_ctc_prefix(eng.ctx, 1, 1, 0, 0, ctypes.byref(need), None, None, None, None, None, ctypes.byref(frames), s) == 0
    assert (need.value, frames.value) == (beam, 3) and eng.counters()[0] == n1 and n1 == n0 + 2
    hyps, raw, frames = eng.stream_ctc_prefix(1, True, True, stream=s)
    assert raw[2].shape == (1, beam, 3) and frames == 3
    assert_row(raw, one_launch(eng, lp_d[1:2], [3], beam, True), 0, "a read sized by the query")


def test_reset_restarts_one_slot(engines):
    lp, lens, blank, beam, phrases, score = CASES["ragged_ctx"]
    eng = engines(lp.shape[2], blank)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    eng.context_set(phrases, score)
    eng.stream_ctc_prefix_reset(-1, _stream())
    s = _stream()
    head = lp_d[:2, :3].contiguous()
    eng.pool_ctc_prefix_logprobs([0, 1], head.data_ptr(), 3, beam, True, s)
    with pytest.raises(RnntError) as e:                                             # fixed until the reset
        eng.pool_ctc_prefix_logprobs([0], head.data_ptr(), 3, 3, False, s)
    assert e.value.status == ERR_ARG
    eng.stream_ctc_prefix_reset(0, s)
    assert read(eng, 0, False, 1, 1)[2] == 0 and read(eng, 1, False, beam, 9)[2] == 3
    whole = lp_d[2:3, :lens[2]].contiguous()
    eng.pool_ctc_prefix_logprobs([0], whole.data_ptr(), lens[2], 3, False, s)       # another beam, no context: accepted
    want = one_launch(eng, lp_d[2:3], lens[2:3], 3, False)
    assert_row(read(eng, 0, True, 3, want[2].shape[2])[1], want, 0, "the reset slot")
    tail = lp_d[1:2, 3:lens[1]].contiguous()
    eng.pool_ctc_prefix_logprobs([1], tail.data_ptr(), lens[1] - 3, beam, True, s)  # its neighbour went on
    want = one_launch(eng, lp_d, lens, beam, True)
    assert_row(read(eng, 1, True, beam, want[2].shape[2])[1], want, 1, "the neighbour of the reset slot")


def test_one_launch_per_call(engines):
    lp, lens, blank, beam, phrases, score = CASES["ragged_plain"]
    eng = engines(lp.shape[2], blank)
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    eng.context_set([])
    s = _stream()
    eng.stream_ctc_prefix_reset(-1, s)
    eng.pool_ctc_prefix_logprobs([0], lp_d.data_ptr(), 1, beam, False, s)            # the state exists from here on
    for slots, t in (([1], 1), ([2, 0, 1], 4), ([0], 3), ([1, 2], 1)):
        x = lp_d[:len(slots), :t].contiguous()
        n0 = eng.counters()[0]
        eng.pool_ctc_prefix_logprobs(slots, x.data_ptr(), t, beam, False, s)
        assert eng.counters()[0] == n0 + 1, (slots, t)
    torch.cuda.synchronize()


def test_refusals_change_nothing(engines):
    """each refusal of the log-probability form and of the read, decided before any launch: the launch counter, the slot's frames and
    what it computes next are as if the call had not been made"""
    lp, lens, blank, beam, phrases, score = CASES["ragged_ctx"]
    V = lp.shape[2]
    eng = engines(V, blank, slots=3, frames=8)                                      # a small max_cache_frames
    lp_d = torch.from_numpy(np.ascontiguousarray(lp)).cuda()
    s = _stream()
    eng.context_set(phrases, score)
    eng.stream_ctc_prefix_reset(-1, s)
    rows = lp_d[:2, :2].contiguous()
    eng.pool_ctc_prefix_logprobs([0], rows.data_ptr(), 2, beam, True, s)             # slot 0 biased, slot 1 not, both 2 frames in
    eng.pool_ctc_prefix_logprobs([1], rows[1:].data_ptr(), 2, beam, False, s)
    frames = lambda slot: read(eng, slot, False, beam, 8)[2]                         # noqa: E731
    launches = lambda: eng.counters()[0]                                              # noqa: E731

    def refused(status, slots, t=1, beam_size=beam, ctx=True, ptr=rows.data_ptr()):
        f0 = [frames(k) for k in range(3)]
        n0 = launches()
        with pytest.raises(RnntError) as e:
            eng.pool_ctc_prefix_logprobs(slots, ptr, t, beam_size, ctx, s)
        assert e.value.status == status, e.value
        assert launches() == n0 and [frames(k) for k in range(3)] == f0

    refused(ERR_ARG, [0], ptr=None)
    refused(ERR_ARG, [0, 0])
    refused(ERR_ARG, [3])
    refused(ERR_ARG, [-1])
    refused(ERR_ARG, [0], t=0)
    refused(ERR_ARG, [2], beam_size=0)
    refused(ERR_ARG, [2], beam_size=V + 1)
    refused(ERR_ARG, [2], beam_size=17)
    refused(ERR_ARG, [0], beam_size=beam - 1)                                        # differs from the search in progress
    refused(ERR_ARG, [0], ctx=False)
    refused(ERR_ARG, [1], ctx=True)
    refused(ERR_ARG, [2, 0], ctx=False)                                              # one bad slot refuses the whole call: slot 2 stays fresh
    refused(ERR_SHAPE, [0], t=7)                                                     # 2 + 7 > 8
    refused(ERR_SHAPE, [2, 0], t=7)
    one = np.zeros(1, np.int32)
    assert eng.lib.rnnt_pool_ctc_prefix_logprobs(eng.ctx, 1, None, rows.data_ptr(), 1, beam, 1, s) == ERR_ARG
    assert eng.lib.rnnt_pool_ctc_prefix_logprobs(eng.ctx, 0, one.ctypes.data_as(ctypes.c_void_p), rows.data_ptr(), 1, beam, 1, s) == ERR_ARG
    # the read: room for the slot's beam and its frames, no null outputs
    n0 = launches()
    for kw in (dict(cap_hyps=beam - 1, cap_tokens=8), dict(cap_hyps=beam, cap_tokens=1)):
        with pytest.raises(RnntError) as e:
            eng.stream_ctc_prefix(0, True, True, stream=s, **kw)
        assert e.value.status == ERR_ARG
    with pytest.raises(RnntError) as e:
        eng.stream_ctc_prefix(3, True, True, beam, 8, s)
    assert e.value.status == ERR_ARG
    nh, ln, sc = np.zeros(1, np.int32), np.zeros(beam, np.int32), np.zeros(beam, np.float64)
    tk = np.zeros((beam, 8), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                  # noqa: E731
    get = eng.lib.rnnt_stream_get_ctc_prefix
    assert get(eng.ctx, 0, 1, beam, 8, p(nh), p(ln), p(tk), None, p(sc), None, None, s) == ERR_ARG
    assert get(eng.ctx, 0, 1, beam, 8, None, p(ln), p(tk), p(tk), p(sc), None, None, s) == ERR_ARG
    assert launches() == n0
    # a new graph mid-utterance: the biased slot is refused until it is reset, the unbiased one goes on
    eng.context_set([[3, 1]], 2.0)
    refused(ERR_STATE, [0])
    refused(ERR_STATE, [2, 0])
    n0 = launches()
    with pytest.raises(RnntError) as e:
        eng.stream_ctc_prefix(0, True, True, beam, 8, s)                             # finalize would read the graph that is gone
    assert e.value.status == ERR_STATE and launches() == n0
    assert read(eng, 0, False, beam, 8)[2] == 2                                      # the running scores are still there
    tail = lp_d[1:2, 2:lens[1]].contiguous()
    eng.pool_ctc_prefix_logprobs([1], tail.data_ptr(), lens[1] - 2, beam, False, s)
    want = one_launch(eng, lp_d[1:2], lens[1:2], beam, False)
    assert_row(read(eng, 1, True, beam, want[2].shape[2])[1], want, 0, "the unbiased slot across rnnt_context_set")
    eng.context_set([])                                                              # no graph at all
    refused(ERR_STATE, [2], ctx=True)
    refused(ERR_STATE, [0])
    # after all of it slot 0 still computes what it would have: put its graph back (a new generation all the same), reset, rerun
    eng.context_set(phrases, score)
    refused(ERR_STATE, [0])
    eng.stream_ctc_prefix_reset(0, s)
    whole = lp_d[0:1, :8].contiguous()
    eng.pool_ctc_prefix_logprobs([0], whole.data_ptr(), 8, beam, True, s)
    refused(ERR_SHAPE, [0], t=1)                                                     # full: 8 + 1 > 8
    want = one_launch(eng, lp_d[0:1], [8], beam, True)
    assert_row(read(eng, 0, True, beam, 8)[1], want, 0, "slot 0 after the refusals")
    assert frames(2) == 0
    big = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=600, max_beam=0)
    try:
        wide = torch.zeros(1, 1, 600, device="cuda")
        with pytest.raises(RnntError) as e:
            big.pool_ctc_prefix_logprobs([0], wide.data_ptr(), 1, 2, False, s)
        assert e.value.status == ERR_ARG
    finally:
        big.close()


# ---- with weights: the encoder form and StreamPool ---------------------------------------------------------------------------------
CHUNK, N_CHUNKS, LATE = 16, 6, 2            # 16-frame chunks (t' = 3); the second slot opens two chunks after the first
BEAM = 4
BIAS = ([[101, 211, 223], [111, 281], [223]], 2.0)
FBANK_SEEDS = (45, 46)


def _engine(sd, slots, max_beam=0):
    eng = RnntEngine(max_streams=slots, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=T.VOCAB,
                     blank_id=T.BLANK, max_beam=max_beam)
    eng.load_state_dict(sd)
    return eng


@pytest.fixture(scope="module")
def weights(np_state_dict):
    """seeded weights with a CTC head, a two-slot context, a one-slot context, two utterances and the rows a one-slot context yields for
    each of them chunk by chunk: rnnt_pool_chunk(greedy = 0) + rnnt_enc_frames_dev + rnnt_ctc_logprobs + rnnt_frames_discard"""
    sd = np_state_dict(0)
    pool, solo = _engine(sd, 2), _engine(sd, 1)
    s = _stream()
    xs = [torch.from_numpy(T.synth_fbank(1, CHUNK * n, seed=seed))[0].cuda() for n, seed in zip((N_CHUNKS, N_CHUNKS - LATE), FBANK_SEEDS)]
    rows = []
    for x in xs:
        solo.reset(1, s)
        n = x.size(0) // CHUNK
        lp = torch.empty(n * 3, T.VOCAB, device="cuda")
        for k in range(n):
            chunk = x[k * CHUNK:(k + 1) * CHUNK][None].contiguous()
            assert solo.pool_chunk([0], chunk.data_ptr(), CHUNK, [4 * k], [4 * k], False, s) == 3
            nf, stride = ctypes.c_int32(0), ctypes.c_int32(0)
            ptr = solo.lib.rnnt_enc_frames_dev(solo.ctx, ctypes.byref(nf), ctypes.byref(stride))
            assert nf.value == 3
            solo.ctc_logprobs(ptr, 3, lp[3 * k:3 * k + 3].data_ptr(), s)
            solo.frames_discard(s)
        torch.cuda.synchronize()
        rows.append(lp)
    yield {"sd": sd, "pool": pool, "solo": solo, "xs": xs, "rows": rows}
    pool.close()
    solo.close()


def _guard(lp_d, phrases, score):
    """as test_decode_from_encoder_frames: the case counts only if the restatement alone finds every gap >= MIN_GAP and no tie"""
    lp = lp_d.cpu().numpy()[None]
    st = {}
    C.reference_of((lp, [lp.shape[1]], T.BLANK, BEAM, phrases, score), st)
    assert st["nonzero_gap"] >= C.MIN_GAP and not st.get("top_ties") and not st.get("prune_ties"), st


@pytest.mark.parametrize("biased", [False, True])
def test_encoder_form(weights, biased):
    """two slots fed 16-frame chunks through rnnt_pool_chunk_ctc_prefix, one opened two chunks late: each slot's final result is the
    one-launch search over the rows a one-slot context computes for its utterance"""
    eng, xs, rows = weights["pool"], weights["xs"], weights["rows"]
    phrases, score = BIAS if biased else (None, 0.0)
    for lp in rows:
        _guard(lp, phrases, score)
    s = _stream()
    eng.reset(2, s)
    eng.context_set(phrases or [], score)
    keep = []
    eng.stream_open(0, s)
    for k in range(N_CHUNKS):
        if k == LATE:
            eng.stream_open(1, s)
        slots = [0] if k < LATE else [0, 1]
        x = torch.stack([xs[b][(k - LATE * b) * CHUNK:(k - LATE * b + 1) * CHUNK] for b in slots], 0).contiguous()
        keep.append(x)
        offs = [4 * (k - LATE * b) for b in slots]
        assert eng.pool_chunk_ctc_prefix(slots, x.data_ptr(), CHUNK, offs, offs, BEAM, biased, s) == 3
    for b in range(2):
        n = rows[b].size(0)
        want = one_launch(eng, rows[b][None].contiguous(), [n], BEAM, biased)
        hyps, raw, frames = read(eng, b, True, BEAM, n)
        assert frames == n == 3 * (N_CHUNKS - LATE * b)
        assert_row(raw, want, 0, f"slot {b}")
        assert len(hyps[0][0]) > 0 and hyps[0][2] == sorted(hyps[0][2])
    # rnnt_stream_open restarts its slot's search alone, rnnt_streams_reset all of them
    eng.stream_open(0, s)
    assert read(eng, 0, True, 1, 1)[2] == 0 and read(eng, 1, True, BEAM, 64)[2] == 3 * (N_CHUNKS - LATE)
    one = rows[0][None, :2].contiguous()
    eng.pool_ctc_prefix_logprobs([0], one.data_ptr(), 2, BEAM + 1, False, s)         # another beam and use_context: accepted
    eng.reset(2, s)
    assert [read(eng, b, True, 1, 1)[2] for b in range(2)] == [0, 0]
    eng.pool_ctc_prefix_logprobs([1], one.data_ptr(), 2, 2, False, s)
    assert read(eng, 1, True, 2, 2)[2] == 2


def test_encoder_form_refusals(weights, np_state_dict):
    eng, xs = weights["pool"], weights["xs"]
    s = _stream()
    eng.reset(2, s)
    eng.context_set([])
    x = xs[0][None, :CHUNK].contiguous()
    assert eng.pool_chunk_ctc_prefix([0], x.data_ptr(), CHUNK, [0], [0], BEAM, False, s) == 3

    def refused(e_, status, slots=(0,), frames=CHUNK, beam=BEAM, ctx=False, offs=(4,)):
        f0 = read(e_, 0, False, 16, 64)[2]
        n0 = e_.counters()[0]
        with pytest.raises(RnntError) as err:
            e_.pool_chunk_ctc_prefix(list(slots), x.data_ptr(), frames, list(offs), list(offs), beam, ctx, s)
        assert err.value.status == status, err.value
        assert e_.counters()[0] == n0 and read(e_, 0, False, 16, 64)[2] == f0
    refused(eng, ERR_ARG, beam=BEAM + 1)                                             # differs from the search in progress
    refused(eng, ERR_ARG, beam=0)
    refused(eng, ERR_STATE, ctx=True)                                                # no graph set
    refused(eng, ERR_ARG, slots=(0, 0), offs=(4, 4))                                 # rnnt_pool_chunk's own refusals
    refused(eng, ERR_ARG, slots=(2,))
    refused(eng, ERR_SHAPE, frames=6)
    eng.pool_chunk([1], x.data_ptr(), CHUNK, [0], [0], False, s)                     # frames still buffered
    refused(eng, ERR_STATE)
    eng.frames_discard(s)
    x2 = xs[0][None, CHUNK:2 * CHUNK].contiguous()
    assert eng.pool_chunk_ctc_prefix([0], x2.data_ptr(), CHUNK, [4], [4], BEAM, False, s) == 3   # and the slot goes on as if nothing had been
    want = one_launch(eng, weights["rows"][0][None, :6].contiguous(), [6], BEAM, False)
    assert_row(read(eng, 0, True, BEAM, 6)[1], want, 0, "after the refusals")
    bare = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=64, vocab_size=T.VOCAB, blank_id=T.BLANK, max_beam=0)
    try:
        with pytest.raises(RnntError) as err:                                        # weights not finalized
            bare.pool_chunk_ctc_prefix([0], x.data_ptr(), CHUNK, [0], [0], BEAM, False, s)
        assert err.value.status == ERR_STATE
        bare.load_state_dict({k: v for k, v in np_state_dict(0).items() if not k.startswith("ctc_head.ctc_lo.")})
        bare.reset(1, s)
        n0 = bare.counters()[0]
        with pytest.raises(RnntError) as err:                                        # ctc_head.ctc_lo.* not loaded
            bare.pool_chunk_ctc_prefix([0], x.data_ptr(), CHUNK, [0], [0], BEAM, False, s)
        assert err.value.status == ERR_STATE and bare.counters()[0] == n0
    finally:
        bare.close()


def test_stream_pool_end_to_end(weights):
    """StreamPool with a ContextBias whose phrase changes the best hypothesis, and a greedy slot, an RNN-T beam slot and a CTC prefix
    slot side by side: the first two are bitwise what they are without the third"""
    from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool
    xs, rows = weights["xs"], weights["rows"]
    n = N_CHUNKS - LATE
    pool = StreamPool(weights["sd"], 3, vocab_size=T.VOCAB, blank_id=T.BLANK, max_chunk_frames=64, max_cache_frames=256, max_tokens=512, max_beam=4)
    try:
        def run(with_ctc, bias=None):
            pool.reset()
            g, b = pool.open(), pool.open(beam_size=4)
            c = pool.open(ctc_prefix_beam=BEAM, context=bias) if with_ctc else None
            inc = []
            for k in range(n):
                pool.feed(g, xs[0][k * CHUNK:(k + 1) * CHUNK])
                pool.feed(b, xs[1][k * CHUNK:(k + 1) * CHUNK])
                if with_ctc:
                    pool.feed(c, xs[1][k * CHUNK:(k + 1) * CHUNK])
                inc.append(pool.step())
            mid = pool.ctc_hyps(c) if with_ctc else None
            beams = [(h.tokens, h.log_prob) for h in pool.close(b)]
            return inc, pool.close(g), beams, mid, pool.close(c) if with_ctc else None
        alone = run(False)
        plain = run(True)
        assert plain[:3] == alone[:3], "the greedy and the RNN-T beam slot changed beside a CTC prefix slot"
        assert len(alone[1]) > 0 and len(alone[2]) > 1
        eng = weights["pool"]
        lp1 = rows[1][None].contiguous()
        eng.context_set([])
        want = eng.ctc_prefix_beam_logprobs(lp1.data_ptr(), [3 * n], 1, 3 * n, BEAM, False, False, _stream())[0]
        assert plain[4] == [(t, s, tm) for t, s, tm, _ in want] and plain[3] == plain[4]
        # a phrase that changes the best hypothesis: a runner-up that is no prefix of the best one, as a hot word
        best = plain[4][0][0]
        other = max((h[0] for h in plain[4][1:] if h[0] != best[:len(h[0])]), key=len)
        bias = ContextBias([other], 6.0)
        _guard(rows[1], bias.phrases, bias.context_score)
        biased = run(True, bias)
        assert biased[:3] == alone[:3]
        eng.context_set(bias.phrases, bias.context_score)
        want = eng.ctc_prefix_beam_logprobs(lp1.data_ptr(), [3 * n], 1, 3 * n, BEAM, True, False, _stream())[0]
        assert biased[4] == [(t, s, tm) for t, s, tm, _ in want]
        assert biased[4][0][0] != best, "the hot word did not change the best hypothesis"
        assert [h[0] for h in biased[3]] == [h[0] for h in biased[4]] and [h[2] for h in biased[3]] == [h[2] for h in biased[4]]
    finally:
        pool.engine.close()
