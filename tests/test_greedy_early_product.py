"""greedy_multi forms the next predictor step's W_hh x h' inside the argmax exchange of the pass that made h' (g_next / have_g in
rnnt_decode.hip.h); the first predictor step of a call forms it in front of the pass loop.  Both run the same loop on the same bits, so
where a call starts must not show: an utterance decoded in ONE call (every product but the first formed early and carried, over
any number of passes that leave the candidate alone) and the same utterance decoded one chunk per call (per-chunk API, pool slot:
every call starts with a product formed in front of its loop) give the same tokens and the same predictor state, bit for bit.

One seeded model (weights seed 0; the encoder weights do not depend on the vocabulary or the blank bias), three inputs of 200 / 160 /
112 fbank frames (38 / 30 / 21 encoder frames).  The oracle's encoder frames are computed once and its greedy loop runs on them frame
by frame, which gives the per-frame symbol counts that the pass patterns are asserted from.  Every comparison with the oracle first
asserts a smallest top-2 margin >= MARGIN, so a token flip is a bug and not a near-tie.  The C ABI does not expose nsym (symbols
emitted on the current frame); it is covered through the tokens of the calls that follow.  Needs a real MI355X."""
import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from ctc_vr_amd.online_rnnt_model import StreamingBatch, StreamPool

pytestmark = pytest.mark.gpu

MARGIN = 1e-3
N_STEPS = 10
CHUNK = 16
SEED = 0
LENS = [200, 160, 112]            # chunk plans that are prefixes of the 200-frame plan
DEFAULT_BIAS, BURST_BIAS, SILENT_BIAS = 11.0, 7.0, 20.0
# (V, blank) -> (blank_bias, out_gain): symbols from every part that has rows, blank in the first / the last part
VOCAB_EDGES = {(5, 0): (-8.0, 4.0), (5, 4): (0.0, 4.0), (412, 0): (1.0, 8.0), (412, 411): (10.5, 4.0), (512, 0): (0.0, 4.0), (512, 511): (10.5, 4.0)}

_CACHE = {}


def _x():
    if "x" not in _CACHE:
        _CACHE["x"] = torch.from_numpy(T.synth_fbank(3, LENS[0], seed=11))
    return _CACHE["x"]


def _sd(bias=DEFAULT_BIAS, V=T.VOCAB, blank=T.BLANK, gain=4.0):
    key = ("sd", bias, V, blank, gain)
    if key not in _CACHE:
        _CACHE[key] = T.make_state_dict(SEED, vocab=V, blank=blank, blank_bias=bias, out_gain=gain)
    return _CACHE[key]


def _oracle_enc(b):
    """the oracle's encoder frames of input b over its own LENS[b] frames (the chunk loop of decode_script_greedy), and the tokens
    that loop gives with the default weights"""
    key = ("enc", b)
    if key not in _CACHE:
        from oracle import rnnt_oracle as O
        st = O.OracleStream(O.to_torch_sd(_sd()), T.BLANK, CHUNK)
        x = _x()[b:b + 1, :LENS[b]]
        outs, toks = [], []
        for a, e in T.chunk_plan(LENS[b], CHUNK):
            tr = {}
            toks += st.process_single_chunk(x[:, a:e], trace=tr)
            if "enc_out" in tr:
                outs.append(tr["enc_out"])
        _CACHE[key] = (torch.cat(outs, 1), toks)
    return _CACHE[key]


def _timeline(b, bias=DEFAULT_BIAS, V=T.VOCAB, blank=T.BLANK, gain=4.0):
    """oracle.greedy_frames frame by frame -> the per-frame token lists of input b and the smallest top-2 margin"""
    key = ("tl", b, bias, V, blank, gain)
    if key not in _CACHE:
        from oracle import rnnt_oracle as O
        sd = O.to_torch_sd(_sd(bias, V, blank, gain))
        enc = _oracle_enc(b)[0]
        frames, st, tok, margins = [], None, blank, []
        for t in range(enc.size(1)):
            hyp, st, tok = O.greedy_frames(sd, enc[:, t:t + 1], st, tok, blank, N_STEPS, margins=margins)
            frames.append(hyp)
        _CACHE[key] = (frames, min(margins))
    return _CACHE[key]


def _flat(frames):
    return [t for f in frames for t in f]


def _state(engine, b):
    h, c, tok = engine.predictor_state(b, torch.cuda.current_stream().cuda_stream)
    return h.copy(), c.copy(), tok


def _batch(n, bias=DEFAULT_BIAS, V=T.VOCAB, blank=T.BLANK, gain=4.0):
    return StreamingBatch(_sd(bias, V, blank, gain), n, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128, max_enc_frames=64,
                          max_tokens=512, numerics="fp32")


def _one_call(streams, **w):
    """every listed input over its own length in ONE decoder call -> per stream (tokens, count, h, c, tok)"""
    sb = _batch(len(streams), **w)
    x = torch.stack([_x()[b] for b in streams], 0).cuda().contiguous()
    lens = [LENS[b] for b in streams]
    if len(set(lens)) == 1:
        toks = sb.decode_script(x[:, :lens[0]].contiguous(), CHUNK, pipelined=True)
    else:
        toks = sb.decode_script_ragged(x, torch.tensor(lens), CHUNK)
    counts = sb.engine.token_counts(torch.cuda.current_stream().cuda_stream).tolist()
    out = [(toks[i], counts[i]) + _state(sb.engine, i) for i in range(len(streams))]
    sb.engine.close()
    return out


def _per_chunk(streams, **w):
    """each listed input alone through the per-chunk API: one decoder call per chunk"""
    out = []
    sb = _batch(1, **w)
    for b in streams:
        toks = sb.decode_script(_x()[b:b + 1, :LENS[b]].cuda().contiguous(), CHUNK, per_chunk_decode=True)[0]
        out.append((toks, int(sb.engine.token_counts(torch.cuda.current_stream().cuda_stream)[0])) + _state(sb.engine, 0))
    sb.engine.close()
    return out


def _pool(streams, bias=DEFAULT_BIAS, V=T.VOCAB, blank=T.BLANK, gain=4.0):
    """the listed inputs in the slots of one pool, each fed its own chunk plan: one decoder call per pool step, the shorter ones
    finished (but not closed) while the longer ones go on"""
    pool = StreamPool(_sd(bias, V, blank, gain), len(streams), vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128, max_tokens=512,
                      numerics="fp32")
    slots = [pool.open() for _ in streams]
    plans = [list(T.chunk_plan(LENS[b], CHUNK)) for b in streams]
    for i in range(max(len(p) for p in plans)):
        for slot, b, plan in zip(slots, streams, plans):
            if i < len(plan):
                pool.feed(slot, _x()[b, plan[i][0]:plan[i][1]].cuda().contiguous())
        pool.step()
    s = torch.cuda.current_stream().cuda_stream
    out = []
    for slot in slots:
        toks = pool.engine.stream_tokens(slot, 0, s)
        out.append((toks, len(toks)) + _state(pool.engine, slot))
    pool.engine.close()
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0] and g[1] == w[1], f"{what}, stream {i}: tokens / count differ ({g[1]} vs {w[1]})"
        assert g[2].tobytes() == w[2].tobytes(), f"{what}, stream {i}: h differs (max abs {np.abs(g[2] - w[2]).max()})"
        assert g[3].tobytes() == w[3].tobytes(), f"{what}, stream {i}: c differs (max abs {np.abs(g[3] - w[3]).max()})"
        assert g[4] == w[4], f"{what}, stream {i}: last token {g[4]} vs {w[4]}"


def _counts(frames):
    return [len(f) for f in frames]


@pytest.mark.parametrize("streams", [[1], [0, 1, 2]], ids=["B1", "B3"])
def test_resume_equals_one_call(streams):
    """One call against one call per chunk, through the per-chunk API and through pool slots: tokens, counts, final h, c and token
    bitwise equal, B = 1 and B = 3 with a different length per stream; the tokens are the oracle's."""
    for b in streams:
        frames, margin = _timeline(b)
        assert margin >= MARGIN, (b, margin)
        assert _flat(frames) == _oracle_enc(b)[1], "the frame-by-frame oracle run is the decode-script loop"
        assert len(_flat(frames)) >= 3, b
    one = _one_call(streams)
    for i, b in enumerate(streams):
        assert one[i][0] == _flat(_timeline(b)[0]), f"stream {b}: tokens differ from the oracle"
    _assert_same(_per_chunk(streams), one, "per-chunk calls vs one call")
    _assert_same(_pool(streams), one, "pool slots vs one call")


def test_bursts_and_silence():
    """A blank bias low enough that frames hit the n_steps cap (predictor passes follow predictor passes, the cap commits) and one so
    high that a stream emits nothing (the product formed once and never used): asserted from the oracle's timeline, tokens equal
    oracle.rnnt_oracle.decode_script_greedy's, and the split runs agree bitwise."""
    from oracle import rnnt_oracle as O
    burst, m_burst = _timeline(1, BURST_BIAS)
    silent, m_silent = _timeline(1, SILENT_BIAS)
    assert min(m_burst, m_silent) >= MARGIN, (m_burst, m_silent)
    cb = _counts(burst)
    assert cb.count(N_STEPS) >= 1 and any(0 < n < N_STEPS for n in cb) and cb.count(0) >= 1, cb
    assert any(cb[t] == N_STEPS and cb[t + 1] > 0 for t in range(len(cb) - 1)), "a capped frame followed at once by another symbol"
    assert sum(_counts(silent)) == 0
    x = _x()[1:2, :LENS[1]]
    for bias, frames in ((BURST_BIAS, burst), (SILENT_BIAS, silent)):
        want = O.decode_script_greedy(O.to_torch_sd(_sd(bias)), x, CHUNK, T.BLANK)[0]
        assert want == _flat(frames)
        one = _one_call([1], bias=bias)
        assert one[0][0] == want, f"blank bias {bias}: tokens differ from the oracle"
        _assert_same(_per_chunk([1], bias=bias), one, f"blank bias {bias}: per-chunk calls vs one call")
        _assert_same(_pool([1], bias=bias), one, f"blank bias {bias}: pool slot vs one call")


def test_product_carried_over_blank_passes():
    """Predictor pass -> blank -> a four-frame pass of blanks only -> a symbol found by a multi-frame pass (commit without a predictor
    step in that pass) -> predictor pass: the product formed in the first of these is the one the last consumes, carried over the
    passes between.  The pattern is asserted from the oracle's timeline of input 0; tokens and state equal the split runs bitwise."""
    frames, margin = _timeline(0)
    assert margin >= MARGIN, margin
    c = _counts(frames)
    hits = [t for t in range(len(c) - 5) if 0 < c[t] < N_STEPS and c[t + 1:t + 5] == [0, 0, 0, 0] and any(c[t + 5:])]
    assert hits, c
    one = _one_call([0])
    assert one[0][0] == _flat(frames)
    _assert_same(_per_chunk([0]), one, "per-chunk calls vs one call")
    _assert_same(_pool([0]), one, "pool slot vs one call")


@pytest.mark.parametrize("cfg", list(VOCAB_EDGES), ids=lambda c: f"V{c[0]}_blank{c[1]}")
def test_vocabulary_edges_of_the_part_split(cfg):
    """rows_per = ceil(V / 4) at V = 5 (two rows per part, the last part empty), 412 and 512 (128 rows, the largest), blank first and
    blank last: one call and per-chunk calls give the oracle's tokens."""
    V, blank = cfg
    bias, gain = VOCAB_EDGES[cfg]
    frames, margin = _timeline(0, bias, V, blank, gain)
    assert margin >= MARGIN, margin
    want = _flat(frames)
    c = _counts(frames)
    assert len(want) >= 10 and any(0 < n < N_STEPS for n in c), c
    w = dict(bias=bias, V=V, blank=blank, gain=gain)
    one = _one_call([0], **w)
    assert one[0][0] == want
    _assert_same(_per_chunk([0], **w), one, "per-chunk calls vs one call")
