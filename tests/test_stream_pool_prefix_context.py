"""Hot-word biasing in the transducer prefix beam search per slot of the stream pool (rnnt_pool_prefix_frames_ctx,
rnnt_pool_chunk_prefix_ctx, rnnt_stream_get_prefix_ctx; StreamPool.open(prefix_beam=k, prefix_context=ContextBias)).

The contract under test is test_stream_pool_prefix.py's with a graph: a biased search fed in pieces is, bit for bit, the B = 1 one-call
search (rnnt_prefix_beam_decode_ctx) over the same frames, whatever the split and whatever the other slots do; and the generation
rule of the CTC pool search: after rnnt_context_set a search biased under the older graph is refused until its slot is reset.  Results
are compared as bytes.  15 encoder frames per utterance.  Needs a real MI355X.  Nothing here provokes a device fault: every refusal is
a host-side check."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, ERR_STATE, RnntError
import test_prefix_context as PC
import test_stream_pool_prefix as SP

pytestmark = pytest.mark.gpu

BLANK = T.BLANK
N = 15                                  # encoder frames of 64 fbank frames
W = (0.3, 0.7)
SPLITS = {"one_call": [15], "two_calls": [7, 8], "ones": [1] * 15}


def _stream():
    return torch.cuda.current_stream().cuda_stream


bits = PC.bits


@pytest.fixture(scope="module")
def world(np_state_dict):
    """seeded weights, a three-slot context (four hypotheses per step workgroup) and a one-slot one, the encoder frames [3, 15, 256] of
    one rnnt_encoder_full call, and the graph: PC.phrases_from on the UNBIASED one-call search of an utterance at beam 4"""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    sd = np_state_dict(0)
    eng, solo = SP._engine(sd, 3), SP._engine(sd, 1, group=None)
    x = torch.from_numpy(T.synth_fbank(3, 64, seed=91)).cuda().contiguous()
    enc = torch.empty(3, N, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [64, 64, 64], 3, 64, enc.data_ptr(), _stream()) == N
    for utt in range(3):                                              # the first utterance whose unbiased n-best gives the two phrases
        unbiased = eng.prefix_beam_decode(enc[utt:utt + 1].contiguous().data_ptr(), [N], 1, N, 4, W[0], W[1], False, _stream())[0]
        phrases = PC.phrases_from(unbiased)
        if phrases is not None:
            break
    assert phrases is not None, "no utterance has a hypothesis outside its best one"
    print("utterance", utt, "phrases", phrases)
    w = {"sd": sd, "eng": eng, "solo": solo, "enc": enc, "x": x, "phrases": phrases, "score": 6.0, "utt": utt}
    yield w
    eng.close()
    solo.close()


def one_call(eng, rows, beam):
    """the oracle: B = 1 rnnt_prefix_beam_decode_ctx over rows [n, 256] -> (hyps [(tokens, total, final context score)], h, c)"""
    n = rows.size(0)
    buf = rows[None].contiguous() if n else torch.zeros(1, 1, 256, device="cuda")
    hyps, h, c = eng.prefix_beam_decode_ctx(buf.data_ptr(), [n], 1, max(n, 1), beam, W[0], W[1], True, True, _stream())
    return hyps[0], h[0, :len(hyps[0])].copy(), c[0, :len(hyps[0])].copy()


def assert_same(got, want, what):
    (gh, g_h, g_c), (wh, w_h, w_c) = got, want
    assert [t for t, _, _ in gh] == [t for t, _, _ in wh], f"{what}: tokens\n{gh}\n{wh}"
    for k, name in ((1, "total"), (2, "context score")):
        assert np.array_equal(bits(np.array([v[k] for v in gh])), bits(np.array([v[k] for v in wh]))), f"{what}: {name} bits\n{gh}\n{wh}"
    assert g_h.shape == w_h.shape and np.array_equal(bits(g_h), bits(w_h)), f"{what}: h bits"
    assert np.array_equal(bits(g_c), bits(w_c)), f"{what}: c bits"


def adv(eng, slots, rows, beam, use_context, keep):
    x = torch.stack(rows, 0).contiguous()
    keep.append(x)
    eng.pool_prefix_frames_ctx(slots, x.data_ptr(), x.size(1), beam, W[0], W[1], use_context, _stream())


# ---- 1. split invariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [4, 16])
def test_split_invariance(beam, world):
    """one slot fed the same frames in 1 call, 2 calls and one frame per call: the final read of every split is the one-call biased
    search bit for bit (tokens, totals, final context scores, LSTM states); the running reads (totals, running context scores,
    states) are the same bytes for every split; and the graph did something: the biased best differs from the unbiased best or some
    context score is not 0"""
    eng, enc, keep, s, u = world["eng"], world["enc"], [], _stream(), world["utt"]
    eng.context_set(world["phrases"], world["score"])
    want = one_call(eng, enc[u], beam)
    unbiased = eng.prefix_beam_decode(enc[u:u + 1].contiguous().data_ptr(), [N], 1, N, beam, W[0], W[1], False, s)[0]
    running = {}
    for split, cuts in SPLITS.items():
        eng.stream_prefix_reset(-1, s)
        at = 0
        for t in cuts:
            adv(eng, [1], [enc[u, at:at + t]], beam, True, keep)
            at += t
        assert eng.stream_prefix_size(1) == (beam, N, N + 1)
        assert_same(eng.stream_prefix_ctx(1, True, True, s), want, f"beam {beam} {split}, final")
        running[split] = eng.stream_prefix_ctx(1, False, True, s)
        assert_same(eng.stream_prefix_ctx(1, True, True, s), want, f"beam {beam} {split}, final after a running read")
    for split in ("two_calls", "ones"):
        assert_same(running[split], running["one_call"], f"beam {beam} {split}, running")
    run, fin = running["one_call"][0], want[0]
    assert [t for t, _, _ in run] == [t for t, _, _ in fin]
    for (_, rt, rc), (_, ft, fc) in zip(run, fin):                    # the same unbiased score under either context score
        assert abs((rt - rc) - (ft - fc)) < 1e-9
    assert [t for t, _, _ in fin][0] != unbiased[0][0] or any(c != 0.0 for _, _, c in run), "the graph changed nothing: the case shows nothing"
    print(beam, run[:2], fin[:2])


def test_zero_frames_and_fresh_slot(world):
    """a fresh slot reads as [blank] with total 0 and context score 0; its final read is the one-call search over no frames, bit for bit"""
    eng, s = world["eng"], _stream()
    eng.context_set(world["phrases"], world["score"])
    eng.stream_prefix_reset(-1, s)
    want = one_call(eng, world["enc"][0, :0], 4)
    assert want[0] == [([BLANK], 0.0, 0.0)]
    assert_same(eng.stream_prefix_ctx(0, True, True, s), want, "fresh slot, final")
    hyps, h, c = eng.stream_prefix_ctx(0, False, True, s)
    assert hyps == [([BLANK], 0.0, 0.0)] and not h.any() and not c.any()


# ---- 2. mixed slots through the facade ------------------------------------------------------------------------------------------------------
def test_mixed_slots_equal_their_stand_alone_runs(world):
    """a biased prefix slot, an unbiased prefix slot and a greedy slot advance in the same step() rounds through feed(): each is
    byte for byte its stand-alone run in the same pool, and the biased slot's close() is the one-call biased search over its kept
    frames"""
    from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool
    x, beam, n = world["x"], 5, 4
    g = ContextBias(world["phrases"], world["score"])
    pool = StreamPool(world["sd"], 3, vocab_size=T.VOCAB, blank_id=BLANK, max_chunk_frames=64, max_cache_frames=256, max_tokens=512)
    try:
        def run(kinds):
            pool.reset()
            slots = {}
            for kind in kinds:
                slots[kind] = (pool.open(prefix_beam=beam, prefix_context=g, keep_frames=True) if kind == "biased" else
                               pool.open(prefix_beam=beam) if kind == "plain" else pool.open())
            inc, mid = [], []
            for k in range(n):
                for kind, slot in slots.items():
                    pool.feed(slot, x[1 if kind == "plain" else 0, k * 16:(k + 1) * 16].contiguous())
                inc.append(pool.step())
                if "biased" in slots:
                    mid.append((pool.prefix_hyps(slots["biased"], with_context_scores=True), pool.prefix_hyps(slots["biased"], True, True)))
            out = {"inc": [{kind: i.get(slot) for kind, slot in slots.items() if kind == "greedy"} for i in inc], "mid": mid}
            if "biased" in slots:
                out["frames"] = pool.frames(slots["biased"])
                out["rescore"] = pool.rescore([slots["biased"]], 0.3, 0.7)[slots["biased"]]
            for kind, slot in slots.items():
                out[kind] = pool.close(slot)
            return out
        mixed = run(("biased", "plain", "greedy"))
        for kind in ("biased", "plain", "greedy"):
            alone = run((kind,))
            assert alone[kind] == mixed[kind], kind
            if kind == "biased":
                assert alone["mid"] == mixed["mid"]
            if kind == "greedy":
                assert alone["inc"] == mixed["inc"] and len(mixed["greedy"]) > 0
        assert len(mixed["biased"]) == beam and len(mixed["plain"]) == beam
        # close() of the biased slot: the final totals of the one-call biased search over the frames it consumed
        frames = mixed["frames"]
        assert frames.shape == (3 * n, 256)
        want = one_call(pool.engine, frames, beam)[0]
        assert mixed["biased"] == [(t, v) for t, v, _ in want]
        assert mixed["mid"][-1][1] == want                                                       # the final read before close()
        assert [r[1] for r in mixed["rescore"][1]] == [v for _, v, _ in want], "rescore() takes the final totals as first scores"
        assert any(c != 0.0 for run_, _ in mixed["mid"] for _, _, c in run_) or mixed["biased"] != mixed["plain"]
    finally:
        pool.engine.close()


# ---- 3. lifecycle ------------------------------------------------------------------------------------------------------------------------------
def test_context_set_mid_utterance_refuses_the_biased_slot_only(world):
    """rnnt_context_set while a biased slot is mid-utterance: that slot's next call and its final read are refused with RNNT_ERR_STATE,
    nothing is launched and no slot moves (frames, hypotheses); the running read still works; the unbiased slot goes on; after a
    reset the slot works under the new graph; a use_context that differs from the slot's search is RNNT_ERR_ARG"""
    eng, enc, keep, s, beam = world["eng"], world["enc"], [], _stream(), 4
    eng.context_set(world["phrases"], world["score"])
    eng.reset(3, s)
    for b in range(3):
        eng.stream_open(b, s)
    adv(eng, [0], [enc[0, 0:4]], beam, True, keep)                     # slot 0 biased, 4 frames in
    adv(eng, [1], [enc[1, 0:4]], beam, False, keep)                    # slot 1 unbiased
    launches = lambda: eng.counters()[0]                               # noqa: E731
    sizes = lambda: [eng.stream_prefix_size(k) for k in range(3)]      # noqa: E731

    def refused(status, slots, rows, use_context, b=beam):
        f0, n0 = sizes(), launches()
        with pytest.raises(RnntError) as e:
            adv(eng, slots, rows, b, use_context, keep)
        assert e.value.status == status, e.value
        assert launches() == n0 and sizes() == f0
    refused(ERR_ARG, [0], [enc[0, 4:6]], False)                        # the slot's search is biased
    refused(ERR_ARG, [1], [enc[1, 4:6]], True)                         # and this one is not
    refused(ERR_ARG, [2, 0], [enc[2, 0:2], enc[0, 4:6]], False)        # one bad slot refuses the whole call: slot 2 stays fresh
    snap = [eng.stream_prefix_ctx(k, False, True, s) for k in range(3)]
    fin0 = eng.stream_prefix_ctx(0, True, True, s)
    other = [[world["phrases"][0][0], world["phrases"][1][1]]]
    eng.context_set(other, 3.0)                                        # a new generation
    refused(ERR_STATE, [0], [enc[0, 4:6]], True)
    refused(ERR_STATE, [2, 0], [enc[2, 0:2], enc[0, 4:6]], True)
    f0, n0 = sizes(), launches()
    with pytest.raises(RnntError) as e:
        eng.stream_prefix_ctx(0, True, True, s)
    assert e.value.status == ERR_STATE and launches() == n0 and sizes() == f0
    for k in range(3):
        assert_same(eng.stream_prefix_ctx(k, False, True, s), snap[k], f"slot {k}, running read after the refusals")
    adv(eng, [1], [enc[1, 4:9]], beam, False, keep)                    # the unbiased slot goes on
    hy, h, c = eng.stream_prefix(1, True, s)
    want = eng.prefix_beam_decode(enc[1:2, :9].contiguous().data_ptr(), [9], 1, 9, beam, W[0], W[1], True, s)
    assert hy == want[0][0] and np.array_equal(bits(h), bits(want[1][0, :len(hy)])) and np.array_equal(bits(c), bits(want[2][0, :len(hy)]))
    eng.context_set([], 0.0)                                           # no graph at all: still refused, still readable
    refused(ERR_STATE, [0], [enc[0, 4:6]], True)
    assert_same(eng.stream_prefix_ctx(0, False, True, s), snap[0], "slot 0 without a graph")
    eng.context_set(other, 3.0)
    eng.stream_open(0, s)                                              # close() + open() of the facade: the slot restarts
    adv(eng, [0], [enc[0, 0:6]], beam, True, keep)
    assert_same(eng.stream_prefix_ctx(0, True, True, s), one_call(eng, enc[0, :6], beam), "slot 0 under the new graph")
    eng.context_set(world["phrases"], world["score"])                  # and the first graph again gives the first result
    eng.stream_prefix_reset(0, s)
    adv(eng, [0], [enc[0, 0:4]], beam, True, keep)
    assert_same(eng.stream_prefix_ctx(0, True, True, s), fin0, "slot 0 under the first graph again")
    eng.reset(3, s)
