"""Prefix beam search on the device (rnnt_prefix_beam_decode: prefix_step + prefix_merge per frame, no host round trip inside the
frame loop), batched over ragged utterances.  Oracles: rnnt_prefix_merge_host for the merge seam, the CPU restatement
oracle.rnnt_oracle.prefix_beam_search_full (pinned to the reference class by prefix_beam_seed*.npz) end to end, B = 1 calls for
batch independence, and the facade's host loop (OnlineRNNTModel.prefix_beam_search) on the same device.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from prefix_cases import BLANK, assert_same, cases

pytestmark = pytest.mark.gpu

SCORE_TOL, STATE_TOL = 2e-3, 1e-3       # the tolerances of test_prefix_beam_search_matches_reference
# (seed, frames, valid, beam, fbank_seed); the oracle's smallest top-(k+1) gap / smallest gap between adjacent sorted scores at the
# cut over all frames: 3.7e-3 / 2.8e-3, 1.6e-4 / 1.5e-4, 2.8e-4 / 3.5e-4, 6.0e-4 / 6.0e-4, 5.3e-3 / n.a.; 16, 29, 15, 0, 0 merges
E2E = [(0, 160, 160, 3, 71), (0, 160, 120, 5, 72), (1, 96, 96, 4, 73), (1, 64, 64, 2, 74), (1, 160, 160, 1, 76)]

_MODELS, _ORACLE = {}, {}


def model(np_state_dict, seed):
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    if seed not in _MODELS:
        m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=T.VOCAB, blank_id=BLANK, max_streams=8, max_chunk_frames=256,
                            max_cache_frames=128, max_enc_frames=128, max_beam=0)
        m.load_state_dict(np_state_dict(seed))
        _MODELS[seed] = m
    return _MODELS[seed]


def fbank(case):
    return torch.from_numpy(T.synth_fbank(1, case[1], seed=case[4]))


def oracle(np_state_dict, case):
    """[(tokens, score, h [256])] of the CPU oracle, computed once per case"""
    from oracle import rnnt_oracle as O
    if case not in _ORACLE:
        seed, _, valid, beam, _ = case
        out = O.prefix_beam_search_full(O.to_torch_sd(np_state_dict(seed)), fbank(case), torch.tensor([valid]), BLANK, beam_size=beam)
        _ORACLE[case] = [(t, s, st[0].reshape(256).numpy()) for t, s, st in out]
    return _ORACLE[case]


def assert_matches_oracle(hyps, h, want):
    assert [t for t, _ in hyps] == [t for t, _, _ in want]
    assert max(abs(s - w) for (_, s), (_, w, _) in zip(hyps, want)) < SCORE_TOL
    assert max(float(np.abs(h[i] - w).max()) for i, (_, _, w) in enumerate(want)) < STATE_TOL


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)


# ---- 1. merge seam -----------------------------------------------------------------------------------------------------------------
def test_device_merge_equals_host_merge():
    """prefix_merge (one launch through rnnt_prefix_merge_device) against rnnt_prefix_merge_host on the CPU test's cases: survivors,
    order and source slots exact, scores within 1e-12 (device double exp / log are within an ulp or two of libm)."""
    from ctc_vr_amd.lib import RnntEngine, prefix_merge_host
    eng = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, max_beam=0)
    for name, (hyps, top_lp, top_tok, beam) in sorted(cases().items()):
        want = prefix_merge_host(hyps, top_lp, top_tok, BLANK, beam)
        got = eng.prefix_merge_device(hyps, top_lp, top_tok, BLANK, beam)
        print(name, len(want), max([abs(g[1] - w[1]) for g, w in zip(got, want) if np.isfinite(w[1])] or [0.0]))
        assert_same(got, want)


# ---- 2. end to end against the CPU oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E2E, ids=lambda c: "s%d_f%d_v%d_b%d" % c[:4])
def test_matches_cpu_oracle(case, np_state_dict):
    """prefix_beam_search_batch (B = 1, walking every encoder frame as the reference does) against prefix_beam_search_full: tokens
    exact, scores within 2e-3, final h within 1e-3."""
    m = model(np_state_dict, case[0])
    hyps = m.prefix_beam_search_batch(fbank(case), torch.tensor([case[2]]), beam_size=case[3])
    want = oracle(np_state_dict, case)
    print(case, [s for _, s in hyps[0]], [s for _, s, _ in want])
    assert len(hyps) == 1
    assert_matches_oracle(hyps[0], m._prefix_states_batch[0][0].numpy(), want)


# ---- 3. batch independence, bitwise -----------------------------------------------------------------------------------------------------
def test_rows_are_independent_and_state_is_left_alone(np_state_dict):
    """One call with B = 3, beam 16, enc_lens = [9, 0, 5] over frames of one rnnt_encoder_full output (T = 9): every row equals the
    B = 1 call on its own frames (tokens, bit patterns of the double scores, of h and of c); the length-0 row is [[blank]] with
    score 0; a second call is identical; what the context's streaming and beam getters return does not change."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    sb = StreamingBatch(np_state_dict(0), 3, max_chunk_frames=48, max_cache_frames=64, max_enc_frames=64, max_tokens=64, max_beam=16)
    eng, s = sb.engine, torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(T.synth_fbank(3, 40, seed=81)).cuda().contiguous()
    enc = torch.empty(3, 9, 256, device="cuda")
    assert eng.encoder_full(x.data_ptr(), [40, 40, 40], 3, 40, enc.data_ptr(), s) == 9
    sb.reset()                                                       # streaming, greedy and lock-step beam state to compare afterwards
    tq = eng.encoder_chunk(x[:, :23].contiguous().data_ptr(), 23, 0, 0, s)
    eng.greedy_decode(s)
    eng.beam_advance(0, tq, 4, s)

    def getters():
        rows = sum(len(eng.beam_hyps(b)) for b in range(3))
        out = [eng.token_counts(s), np.array(sum(eng.tokens(s), [])), eng.enc_frames(s), *eng.beam_states(rows, s)]
        for b in range(3):
            h, c, tok = eng.predictor_state(b, s)
            out += [h, c, np.array([tok]), eng.att_cache(b, s), eng.cnn_cache(b, s), np.array([v for _, v in eng.beam_hyps(b)]),
                    np.array(sum([t for t, _ in eng.beam_hyps(b)], []))]
        return out
    before = getters()
    lens = [9, 0, 5]
    hyps, h, c = eng.prefix_beam_decode(enc.data_ptr(), lens, 3, 9, 16, 0.3, 0.7, True, s)
    hyps2, h2, c2 = eng.prefix_beam_decode(enc.data_ptr(), lens, 3, 9, 16, 0.3, 0.7, True, s)
    assert hyps2 == hyps and np.array_equal(bits(h2), bits(h)) and np.array_equal(bits(c2), bits(c))
    assert hyps[1] == [([BLANK], 0.0)] and not h[1].any() and not c[1].any()
    assert len(hyps[0]) == 16 and len(hyps[2]) == 16 and max(len(t) for t, _ in hyps[0]) > 1
    for b in range(3):
        one, h1, c1 = eng.prefix_beam_decode(enc[b:b + 1].contiguous().data_ptr(), lens[b:b + 1], 1, 9, 16, 0.3, 0.7, True, s)
        assert [t for t, _ in one[0]] == [t for t, _ in hyps[b]], b
        assert np.array_equal(bits(np.array([v for _, v in one[0]])), bits(np.array([v for _, v in hyps[b]]))), b
        assert np.array_equal(bits(h1[0]), bits(h[b])) and np.array_equal(bits(c1[0]), bits(c[b])), b
    after = getters()
    assert len(before) == len(after) and all(np.array_equal(p, q) for p, q in zip(before, after))


# ---- 4. same device, two paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [E2E[0], E2E[2]], ids=lambda c: "s%d_f%d_v%d_b%d" % c[:4])
def test_device_loop_equals_host_loop(case, np_state_dict):
    """prefix_beam_search_batch at B = 1 against the facade's host loop prefix_beam_search on the same context: tokens exact, scores
    within 2e-3."""
    m = model(np_state_dict, case[0])
    x, lens = fbank(case), torch.tensor([case[2]])
    want = m.prefix_beam_search(x, lens, beam_size=case[3])
    got = m.prefix_beam_search_batch(x, lens, beam_size=case[3])[0]
    assert [t for t, _ in got] == [t for t, _ in want]
    assert max(abs(a - b) for (_, a), (_, b) in zip(got, want)) < SCORE_TOL


def test_ragged_batch_equals_single_runs(np_state_dict):
    """B = 2 with different lengths, each row stopping at its own last valid frame: every row equals its B = 1 run through
    prefix_beam_search_batch (tokens exact, scores within 2e-3: the encoder's summation order depends on the batch)."""
    m = model(np_state_dict, 0)
    x = torch.cat([fbank(E2E[0]), fbank(E2E[1])], 0)
    lens = torch.tensor([160, 120])
    got = m.prefix_beam_search_batch(x, lens, beam_size=3, walk_padding=False)
    states = m._prefix_states_batch
    assert len(got) == 2 and [tuple(h.shape) for h, _ in states] == [(len(g), 256) for g in got]
    for b in range(2):
        want = m.prefix_beam_search_batch(x[b:b + 1], lens[b:b + 1], beam_size=3, walk_padding=False)[0]
        assert [t for t, _ in got[b]] == [t for t, _ in want], b
        assert max(abs(p - q) for (_, p), (_, q) in zip(got[b], want)) < SCORE_TOL, b
        assert float((states[b][0] - m._prefix_states_batch[0][0]).abs().max()) < STATE_TOL, b
    assert max(len(t) for t, _ in got[1]) <= 1 + 29                  # 120 valid fbank frames are 29 encoder frames: one symbol per frame


# ---- 5. weights ------------------------------------------------------------------------------------------------------------------------------
def _no_ctc_engine(np_state_dict):
    from ctc_vr_amd.lib import RnntEngine
    eng = RnntEngine(max_streams=2, max_chunk_frames=256, max_cache_frames=128, max_enc_frames=128, max_beam=0)
    eng.load_state_dict({k: v for k, v in np_state_dict(1).items() if not k.startswith("ctc_head.")})
    return eng


def test_transducer_only_is_the_per_frame_argmax(np_state_dict):
    """ctc_weight = 0, transducer_weight = 1 on a context without the CTC head, beam_size = 1: the tokens are those of a Python loop
    over rnnt_predictor_step + rnnt_joint(mode 1) that takes one argmax per frame; ctc_weight > 0 is refused with RNNT_ERR_STATE."""
    from ctc_vr_amd.lib import ERR_STATE, RnntError
    eng, s, dev = _no_ctc_engine(np_state_dict), torch.cuda.current_stream().cuda_stream, "cuda"
    x = torch.from_numpy(T.synth_fbank(2, 160, seed=77)).cuda().contiguous()
    tq = 39
    enc = torch.empty(2, tq, 256, device=dev)
    assert eng.encoder_full(x.data_ptr(), [160, 160], 2, 160, enc.data_ptr(), s) == tq
    got = eng.prefix_beam_decode(enc.data_ptr(), [tq, tq], 2, tq, 1, 0.0, 1.0, False, s)
    hyp, h, c = [BLANK], torch.zeros(1, 256, device=dev), torch.zeros(1, 256, device=dev)
    for t in range(tq):
        tok = torch.tensor([hyp[-1]], dtype=torch.int32, device=dev)
        pred, h2, c2 = (torch.empty(1, 256, device=dev) for _ in range(3))
        lp = torch.empty(1, T.VOCAB, device=dev)
        eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), 1, pred.data_ptr(), h2.data_ptr(), c2.data_ptr(), s)
        eng.joint(enc[0:1, t:t + 1].contiguous().data_ptr(), pred.data_ptr(), 1, 1, 1, 1, lp.data_ptr(), s)
        a = int(lp.argmax())
        if a != BLANK:
            hyp.append(a)
            h, c = h2, c2
    assert len(got[0]) == 1 and got[0][0][0] == hyp and len(hyp) > 1
    with pytest.raises(RnntError) as e:
        eng.prefix_beam_decode(enc.data_ptr(), [tq, tq], 2, tq, 1, 0.3, 0.7, False, s)
    assert e.value.status == ERR_STATE


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(np_state_dict):
    """Every refusal returns its status before anything is launched, and a valid call right after still gives the oracle's result."""
    from ctc_vr_amd.lib import ERR_ARG, ERR_STATE, RnntEngine, RnntError
    case = E2E[0]
    m = model(np_state_dict, case[0])
    eng, s = m._engine, torch.cuda.current_stream().cuda_stream
    enc = torch.zeros(2, 9, 256, device="cuda")
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def raw(e=eng, enc_ptr=enc.data_ptr(), lens=(9, 4), B=2, Tq=9, beam=4, cw=0.3, tw=0.7, cap=10, null=None, states=0):
        el = np.asarray(lens, np.int32)
        out = {"nh": np.zeros(max(B, 1), np.int32), "lens": np.zeros(64, np.int32), "toks": np.zeros(64 * max(cap, 1), np.int32),
               "sc": np.zeros(64, np.float64), "h": np.zeros((64, 256), np.float32) if states & 1 else None,
               "c": np.zeros((64, 256), np.float32) if states & 2 else None, "el": el}
        if null:
            out[null] = None
        return e.lib.rnnt_prefix_beam_decode(e.ctx, enc_ptr, p(out["el"]), B, Tq, beam, cw, tw, cap, p(out["nh"]), p(out["lens"]), p(out["toks"]),
                                             p(out["sc"]), p(out["h"]), p(out["c"]), s)
    assert raw() == 0 and raw(states=3) == 0
    refused = [dict(enc_ptr=None), dict(null="el"), dict(null="nh"), dict(null="lens"), dict(null="toks"), dict(null="sc"), dict(states=1),
               dict(states=2), dict(B=0), dict(B=-1), dict(lens=(10, 4)), dict(lens=(9, -1)), dict(beam=0), dict(beam=17), dict(cw=-0.1),
               dict(tw=-1.0), dict(cw=0.0, tw=0.0), dict(cap=9)]
    for kw in refused:
        assert raw(**kw) == ERR_ARG, kw
    assert eng.lib.rnnt_prefix_beam_decode(None, enc.data_ptr(), None, 1, 1, 1, 0.3, 0.7, 2, None, None, None, None, None, None, s) == ERR_ARG
    small = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=8, max_beam=0)
    assert raw(e=small) == ERR_STATE                                 # weights not finalized
    small.load_state_dict(T.make_state_dict(0, vocab=8))
    assert raw(e=small, beam=8) == 0 and raw(e=small, beam=9) == ERR_ARG          # beam_size <= vocab
    big = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, vocab_size=600, max_beam=0)
    big.load_state_dict(T.make_state_dict(0, vocab=600))
    assert raw(e=big) == ERR_ARG                                     # vocab > 512
    no_ctc = _no_ctc_engine(np_state_dict)
    assert raw(e=no_ctc) == ERR_STATE and raw(e=no_ctc, cw=0.0, tw=1.0) == 0
    with pytest.raises(RnntError) as e:
        eng.prefix_beam_decode(enc.data_ptr(), [9, 10], 2, 9, 4, stream=s)
    assert e.value.status == ERR_ARG and "outside [0, 9]" in str(e.value)
    hyps = m.prefix_beam_search_batch(fbank(case), torch.tensor([case[2]]), beam_size=case[3])
    assert_matches_oracle(hyps[0], m._prefix_states_batch[0][0].numpy(), oracle(np_state_dict, case))
