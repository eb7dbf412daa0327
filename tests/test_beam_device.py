"""Device-resident beam search (rnnt_beam_decode: beam_chain + beam_merge_dev per frame, no host round trip inside the frame
loop) and ragged beam batches (rnnt_encode_ragged + one rnnt_beam_decode).  The host merge (rnnt_beam_merge_host /
rnnt_beam_advance) is the oracle: same hypotheses, bitwise the same double scores and LSTM states.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from conftest import load_golden

pytestmark = pytest.mark.gpu

PARITY_MODES = ["fp32", "bf16x3", "f16x3"]


@pytest.fixture(params=PARITY_MODES)
def numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    return request.param


def stream_input(name):
    src = name.split("_")[0]
    if src.startswith("syn"):
        return torch.from_numpy(T.synth_fbank(2, 1000))[int(src[3:]):int(src[3:]) + 1]
    g = load_golden("inputs_example1.npz")
    return torch.from_numpy(g[src])[None]


def host_merge(lib, hyps, steps, blank_lp, top_lp, top_tok, beam_size):
    """rnnt_beam_merge_host on the same flat inputs as RnntEngine.beam_merge_device -> [(tokens, score, src_row, src_step)]."""
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = len(hyps)
    hl = np.array([len(t) for t, _ in hyps], np.int32)
    ht = np.array([x for t, _ in hyps for x in t] or [0], np.int32)
    hs = np.array([s for _, s in hyps], np.float64)
    n_steps, k = top_lp.shape[1], top_lp.shape[2]
    cap = max(n, beam_size) * n_steps * (k + 1)
    ol, ot = np.zeros(cap, np.int32), np.zeros(cap * (int(hl.max(initial=0)) + n_steps) + 1, np.int32)
    osc, orow, ostep = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    m = lib.rnnt_beam_merge_host(n, p(hl), p(ht), p(hs), p(np.ascontiguousarray(steps, np.int32)), p(np.ascontiguousarray(blank_lp, np.float32)),
                                 p(np.ascontiguousarray(top_lp, np.float32)), p(np.ascontiguousarray(top_tok, np.int32)), n_steps, k, beam_size,
                                 p(ol), p(ot), p(osc), p(orow), p(ostep))
    assert m >= 1
    out, o = [], 0
    for a in range(m):
        out.append((ot[o:o + ol[a]].tolist(), float(osc[a]), int(orow[a]), int(ostep[a])))
        o += ol[a]
    return out


def beams_of(eng):
    return [eng.beam_hyps(b) for b in range(eng.n_streams)]


def bits(x):
    return np.float64(x).view(np.int64)


def assert_same_beams(a, b):
    """tokens equal, scores bitwise equal"""
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert [t for t, _ in x] == [t for t, _ in y], s
        assert [bits(v) for _, v in x] == [bits(v) for _, v in y], s


def test_device_merge_equals_host_merge_fuzzed():
    """beam_merge_dev (one launch through rnnt_beam_merge_device) against beam_merge_stream (rnnt_beam_merge_host) on 2400 seeded
    adversarial cases: quantised log-probs (ties everywhere), a 3-symbol alphabet and hypotheses that are prefixes of one another
    (duplicate sequences everywhere).  Same survivors, tokens, bitwise scores and source pool slots."""
    from ctc_vr_amd.lib import RnntEngine
    eng = RnntEngine(max_streams=1, max_chunk_frames=16, max_cache_frames=16, max_enc_frames=16, max_beam=16)
    rng = np.random.default_rng(20261016)
    ns = 10
    n_dups = n_ties = 0
    for case in range(2400):
        beam = int(rng.choice([1, 2, 4, 8, 16]))
        k = beam
        n_hyp = int(rng.integers(1, beam + 1))
        alpha = int(rng.integers(2, 4))
        base = rng.integers(0, alpha, size=int(rng.integers(0, 6))).tolist()
        hyps = []
        for _ in range(n_hyp):
            cut = int(rng.integers(0, len(base) + 1))
            toks = base[:cut] + rng.integers(0, alpha, size=int(rng.integers(0, 3))).tolist()
            hyps.append((toks, float(rng.choice([0.0, -0.5, -1.0, -1.5, -2.25]))))
        steps = rng.integers(1, ns + 1, size=n_hyp).astype(np.int32)
        q = np.array([-0.25, -0.5, -1.0, -2.0, -3.0], np.float32)
        blank_lp = rng.choice(q, size=(n_hyp, ns)).astype(np.float32)
        top_lp = np.sort(rng.choice(q, size=(n_hyp, ns, k)), axis=-1)[..., ::-1].astype(np.float32)
        top_tok = rng.integers(0, alpha, size=(n_hyp, ns, k)).astype(np.int32)
        want = host_merge(eng.lib, hyps, steps, blank_lp, top_lp, top_tok, beam)
        got = eng.beam_merge_device(hyps, steps, blank_lp, top_lp, top_tok, beam)
        assert len(got) == len(want), case
        for a, (g, w) in enumerate(zip(got, want)):
            assert g[0] == w[0], (case, a)
            assert bits(g[1]) == bits(w[1]), (case, a, g[1], w[1])
            assert g[2:] == w[2:], (case, a)
        seqs = []                                                    # every candidate's token sequence, as the merge forms them
        for i, (toks, _) in enumerate(hyps):
            for st in range(int(steps[i])):
                chain = toks + top_tok[i, :st, 0].tolist()
                seqs += [tuple(chain)] + [tuple(chain + [int(t)]) for t in top_tok[i, st]]
        n_dups += len(set(seqs)) < len(seqs)
        n_ties += len({s for _, s, _, _ in want}) < len(want)
    assert n_dups > 200 and n_ties > 200, (n_dups, n_ties)      # the adversarial cases really are adversarial


def _encode(sb, x, chunk):
    """one rnnt_encoder_chunks call over the whole utterance (beam_script(pipelined=True)'s encoder half) -> encoder frames"""
    plan = [(a, b) for a, b in T.chunk_plan(x.size(1), chunk) if b - a >= 7]
    offs, o = [], 0
    for a, b in plan:
        offs.append(o)
        o += (b - a) // 4
    sb.reset()
    s = torch.cuda.current_stream().cuda_stream
    return sb.engine.encoder_chunks(x.data_ptr(), x.size(1), [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s, greedy=False)


@pytest.mark.parametrize("B", [3, 64])
def test_whole_call_equals_beam_advance(B, np_state_dict, numerics):
    """Same buffered encoder frames (1000 fbank frames, chunk 16, beam 4): rnnt_beam_decode leaves the hypotheses, bitwise scores and
    bitwise LSTM states (rnnt_beam_get_states) that rnnt_beam_advance leaves; a second call and a call on another stream agree."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    x = torch.from_numpy(T.synth_fbank(B, 1000, seed=1234)).cuda().contiguous()
    sb = StreamingBatch(np_state_dict(0), B, max_chunk_frames=32, max_cache_frames=256, max_enc_frames=256, max_tokens=64, max_beam=4)
    s = torch.cuda.current_stream().cuda_stream
    F = _encode(sb, x, 16)
    sb.engine.beam_advance(0, F, 4, s)
    want = beams_of(sb.engine)
    rows = sum(len(b) for b in want)
    want_h, want_c = sb.engine.beam_states(rows, s)
    for on_side in (False, True):
        assert _encode(sb, x, 16) == F
        if on_side:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                sb.engine.beam_decode(0, None, 4, side.cuda_stream)
            torch.cuda.current_stream().wait_stream(side)
        else:
            sb.engine.beam_decode(0, None, 4, s)
        assert_same_beams(beams_of(sb.engine), want)
        h, c = sb.engine.beam_states(rows, s)
        assert np.array_equal(h.view(np.int32), want_h.view(np.int32)) and np.array_equal(c.view(np.int32), want_c.view(np.int32))
    assert max(len(t) for bm in want for t, _ in bm) > 0


@pytest.mark.parametrize("name", ["beam_ex6_c16_s0", "beam_syn0_c16_s1_f320"])
def test_mixed_entry_points_match_reference(name, np_state_dict, numerics):
    """A per-chunk loop that alternates rnnt_beam_advance and rnnt_beam_decode chunk by chunk equals either entry point alone
    (bitwise) and the reference's beams after every chunk (golden: tokens exact, scores within 2e-3)."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    g = load_golden(f"{name}.npz")
    chunk, beam = int(g["chunk"]), int(g["beam"])
    x = stream_input(name[5:])[:, :int(g["frames"])].cuda().contiguous()
    sb = StreamingBatch(np_state_dict(int(g["seed"])), 1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_beam=beam)
    runs = {}
    for mode in ("advance", "decode", "mixed"):
        sb.reset()
        seq = []
        for ci, (a, b) in enumerate(T.chunk_plan(x.shape[1], chunk)):
            dm = mode == "decode" or (mode == "mixed" and ci % 2 == 1)
            hyps = sb.process_chunk_beam(x[:, a:b].contiguous(), beam, device_merge=dm)
            seq.append([(h.tokens, h.log_prob) for h in hyps[0]])
        runs[mode] = seq
    assert_same_beams(runs["mixed"], runs["advance"])
    assert_same_beams(runs["decode"], runs["advance"])
    for ci, hyps in enumerate(runs["mixed"]):
        assert len(hyps) == int(g[f"c{ci}_n"]), ci
        for hi, (toks, lp) in enumerate(hyps):
            assert toks == g[f"c{ci}_h{hi}_tokens"].tolist(), (ci, hi)
            assert abs(lp - float(g[f"c{ci}_h{hi}_logp"])) < 2e-3, (ci, hi)


_ORACLE = {}


def _ragged_batch():
    n = 64
    rng = np.random.default_rng(5)
    lens = sorted(rng.choice(np.arange(40, 1001), size=n, replace=False).tolist(), reverse=True)
    lens[0], lens[-1] = 1000, 40
    perm = rng.permutation(n)
    lens = [lens[i] for i in perm]                                   # long and short utterances interleaved over the batch positions
    full = torch.from_numpy(T.synth_fbank(n, 1000, seed=4321))
    x = torch.zeros(n, 1000, 80)
    for b in range(n):
        x[b, :lens[b]] = full[b, :lens[b]]
    return lens, x


def test_ragged_beam_batch_one_call(np_state_dict, numerics):
    """64 utterances of 64 distinct lengths (40 .. 1000 frames) in one padded batch: beam_script_ragged makes exactly one
    rnnt_encode_ragged call and one rnnt_beam_decode call; every stream's beam equals its own B = 1 beam_script(pipelined=True)
    run (tokens exact, scores within 1e-3); the longest and the shortest stream equal the CPU oracle's chunk-by-chunk beam search;
    a second call is bit-identical."""
    from oracle import rnnt_oracle as O
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    lens, x = _ragged_batch()
    n = len(lens)
    xd = x.cuda().contiguous()
    sb = StreamingBatch(np_state_dict(0), n, max_chunk_frames=48, max_cache_frames=256, max_enc_frames=256, max_tokens=64, max_beam=4)
    calls = {"encode_ragged": 0, "beam_decode": 0, "encoder_chunks": 0, "beam_advance": 0}

    def count(name):
        orig = getattr(sb.engine, name)

        def f(*a, **k):
            calls[name] += 1
            return orig(*a, **k)
        setattr(sb.engine, name, f)
    for name in calls:
        count(name)
    got = sb.beam_script_ragged(xd, torch.tensor(lens), 16, beam_size=4)
    assert calls == {"encode_ragged": 1, "beam_decode": 1, "encoder_chunks": 0, "beam_advance": 0}
    sig = lambda beams: [[(tuple(h.tokens), bits(h.log_prob)) for h in bm] for bm in beams]
    assert sig(sb.beam_script_ragged(xd, torch.tensor(lens), 16, beam_size=4)) == sig(got)
    one = StreamingBatch(np_state_dict(0), 1, max_chunk_frames=48, max_cache_frames=256, max_enc_frames=256, max_tokens=64, max_beam=4)
    for b in range(n):
        want = one.beam_script(xd[b:b + 1, :lens[b]].contiguous(), 16, 4, pipelined=True)[0]
        assert [h.tokens for h in got[b]] == [h.tokens for h in want], (b, lens[b])
        assert max(abs(p.log_prob - q.log_prob) for p, q in zip(got[b], want)) < 1e-3, (b, lens[b])
    sd = O.to_torch_sd(np_state_dict(0))
    for b in (int(np.argmax(lens)), int(np.argmin(lens))):
        if b not in _ORACLE:
            st = O.OracleStream(sd, T.BLANK, 16)
            for (a, e) in T.chunk_plan(lens[b], 16):
                ob = st.process_single_chunk_beam_search(x[b:b + 1, a:e], beam_size=4)
            _ORACLE[b] = [(h.tokens, h.log_prob) for h in ob]
        assert [h.tokens for h in got[b]] == [t for t, _ in _ORACLE[b]], b
        assert max(abs(h.log_prob - s) for h, (_, s) in zip(got[b], _ORACLE[b])) < 2e-3, b
    assert len(got[int(np.argmax(lens))][0].tokens) > 0


def test_no_host_in_frame_loop(np_state_dict):
    """Over an F-frame call rnnt_beam_decode enqueues at most 2F + 2 launches (one beam_chain and one beam_merge_dev per frame, the
    scatter into fixed slots and the compaction), and a per-stream frame range gives what the same range through
    rnnt_beam_advance gives."""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    B = 4
    x = torch.from_numpy(T.synth_fbank(B, 400, seed=99)).cuda().contiguous()
    sb = StreamingBatch(np_state_dict(1), B, max_chunk_frames=32, max_cache_frames=256, max_enc_frames=128, max_beam=4)
    s = torch.cuda.current_stream().cuda_stream
    F = _encode(sb, x, 16)
    l0, _ = sb.engine.counters()
    sb.engine.beam_decode(0, None, 4, s)
    l1, _ = sb.engine.counters()
    assert l1 - l0 <= 2 * F + 2, (l1 - l0, F)
    # frames [0, ends[b]) per stream through one call == per-stream rnnt_beam_advance over the same ranges
    ends = [F, F // 3, 0, F - 5]
    _encode(sb, x, 16)
    sb.engine.beam_decode(0, ends, 4, s)
    got = beams_of(sb.engine)
    for b in range(B):
        _encode(sb, x, 16)
        sb.engine.beam_advance(0, ends[b], 4, s)
        assert_same_beams([got[b]], [sb.engine.beam_hyps(b)])


def test_refusals_fall_back(np_state_dict, monkeypatch):
    """beam_size > 16, vocab > 512 and RNNT_BEAM_CHAIN=0 are refused by rnnt_beam_decode with an error status, and
    beam_script_ragged still returns every stream's B = 1 beam through its length-class fallback (rnnt_beam_advance)."""
    from ctc_vr_amd.lib import RnntError
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    lens = [300, 97, 160, 20, 5]
    full = torch.from_numpy(T.synth_fbank(len(lens), 300, seed=7))
    x = torch.zeros(len(lens), 300, 80)
    for b, t in enumerate(lens):
        x[b, :t] = full[b, :t]
    xd = x.cuda().contiguous()

    def check(sd, beam, vocab, expect_status):
        kw = dict(vocab_size=vocab, max_chunk_frames=48, max_cache_frames=128, max_enc_frames=128, max_tokens=64, max_beam=beam)
        sb = StreamingBatch(sd, len(lens), **kw)
        _encode(sb, xd, 16)
        with pytest.raises(RnntError) as e:
            sb.engine.beam_decode(0, None, beam, torch.cuda.current_stream().cuda_stream)
        assert e.value.status == expect_status
        got = sb.beam_script_ragged(xd, torch.tensor(lens), 16, beam_size=beam)
        one = StreamingBatch(sd, 1, **kw)
        for b, t in enumerate(lens):
            if t < 7:
                assert got[b] == []
                continue
            want = one.beam_script(xd[b:b + 1, :t].contiguous(), 16, beam, pipelined=True)[0]
            assert [h.tokens for h in got[b]] == [h.tokens for h in want], b
            assert max(abs(p.log_prob - q.log_prob) for p, q in zip(got[b], want)) < 1e-3, b
    check(np_state_dict(0), 17, T.VOCAB, -1)                                   # beam_size > 16
    check(T.make_state_dict(0, vocab=600), 4, 600, -1)                         # vocab > 512
    monkeypatch.setenv("RNNT_BEAM_CHAIN", "0")
    check(np_state_dict(0), 4, T.VOCAB, -5)                                    # launched extension steps
