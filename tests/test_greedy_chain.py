"""greedy_multi's per-symbol chain: what its hand-offs inside a pass can get wrong.  The committed and the candidate h share a
ping-pong pair of LDS buffers whose roles swap with every symbol, no barrier closes a pass, the gates reach the cell through lane
exchanges, and a one-frame pass is finished by one wave.  test_decode_edges.py covers the symbol-rate regimes against the oracle; this
file adds, on 3 streams x 21 encoder frames (112 fbank frames in 16-frame chunks, one decoder call per chunk):
  * runs of frames at the n_steps cap, a blank frame, a cap frame again, with h / c / last token read back after EVERY call;
  * calls that end on odd and on even symbol counts (which half of the ping-pong pair is the committed one at kernel exit), each
    followed by a call that continues from that state;
  * vocabularies 412 (ragged last part), 129 (33-row parts), 6 (an empty last part) and 512 (128-row parts, the largest), with exact
    twin rows across the two 64-row halves of a part and across parts;
  * repeatability: the same calls twice on one context, and on two contexts driven by two host threads.
Symbol patterns and parities are asserted from the CPU oracle, and every comparison first asserts the oracle's smallest top-2 margin.
nsym (symbols on the current frame) is not part of the state API: a call decodes whole frames, so it is 0 at every call's end, and a
wrong one shows as a wrong frame advance in the next call's tokens.  Needs a real MI355X."""
import gc
import re
import threading

import numpy as np
import pytest
import torch

import ctc_vr_amd.testing as T
from test_decode_edges import CHUNK, CONFIGS, MARGIN, N_STEPS, TWIN_HEADS, _inputs, _oracle_enc, _oracle_greedy, _sd, _tokens, _twin_pairs

pytestmark = pytest.mark.gpu

FRAMES = 112                      # 7 chunks of 16 fbank frames: 7 decoder calls of 3 encoder frames each
STATE_TOL = 1e-4                  # h / c against the oracle: the bar of test_gpu_parity.py's predictor-state checks, which see |c| of order 1
VOCABS = [(412, 0), (129, 128), (6, 0), (512, 0)]
MODES = ["fp32", "bf16x3"]


def _calls():
    """(fbank start, end, encoder frames) of every decoder call of the per-chunk script"""
    return [(a, b, ((b - a - 3) // 2 + 1 - 3) // 2 + 1) for a, b in T.chunk_plan(FRAMES, CHUNK) if b - a >= 7]


N_ENC = sum(n for _, _, n in _calls())

_ORACLE = {}


def _oracle(V, blank, w, twins=()):
    """greedy_frames frame by frame on the oracle's encoder frames, as test_decode_edges._oracle_greedy runs it (twin b's output bias
    lowered so that the first index wins), keeping the state: per stream (tokens per frame, [(h, c, tok) after each frame]), and the
    smallest top-2 margin"""
    key = (V, blank, w, tuple(twins))
    if key not in _ORACLE:
        from oracle import rnnt_oracle as O
        sd = O.to_torch_sd(_sd(V, blank, w, twins=twins))
        if twins:
            sd = dict(sd)
            sd["joint.ffn_out.bias"] = sd["joint.ffn_out.bias"].clone()
            for a, b, _ in twins:
                sd["joint.ffn_out.bias"][b] -= 1e4
        out, margins = [], []
        for s in range(3):
            enc = _oracle_enc(s)
            frames, states, st, tok = [], [], None, blank
            for t in range(N_ENC):
                hyp, st, tok = O.greedy_frames(sd, enc[:, t:t + 1], st, tok, blank, N_STEPS, margins=margins)
                frames.append(hyp)
                states.append((st[0].reshape(-1).numpy().copy(), st[1].reshape(-1).numpy().copy(), tok))
            out.append((frames, states))
        _ORACLE[key] = (out, min(margins))
    return _ORACLE[key]


@pytest.fixture
def batch():
    """factory of 3-stream StreamingBatch contexts, destroyed when the test ends: later tests that compare rnnt_live_device_bytes before
    and after themselves must not see these contexts go at a collection of their own"""
    from ctc_vr_amd.online_rnnt_model import StreamingBatch
    made = []

    def make(V, blank, w, numerics, twins=()):
        made.append(StreamingBatch(_sd(V, blank, w, twins=twins), 3, vocab_size=V, blank_id=blank, max_chunk_frames=48, max_cache_frames=128,
                                   max_enc_frames=64, max_tokens=512, numerics=numerics))
        return made[-1]
    yield make
    torch.cuda.synchronize()
    for sb in made:
        sb.engine.close()
    gc.collect()


def _run_calls(sb, x):
    """one decoder call per chunk -> after every call (tokens so far per stream, [(h, c, tok) per stream])"""
    s = torch.cuda.current_stream().cuda_stream
    sb.reset()
    snaps = []
    for a, b, _ in _calls():
        sb.process_chunk(x[:, a:b].contiguous())
        snaps.append((sb.engine.tokens(s), [sb.engine.predictor_state(i, s) for i in range(3)]))
    return snaps


def _x():
    return _inputs(3, FRAMES).cuda().contiguous()


def _state_close(got, want):
    """h within STATE_TOL (|h| < 1).  c is unbounded -- at high symbol rates it reaches several tens here, where float32 numbers lie
    4e-6 apart and the two implementations add a step's 256 products in different orders -- so its bar is relative to the largest
    |c| of the oracle's state once that exceeds 1: STATE_TOL * max(1, max |c|)."""
    (h, c, tok), (wh, wc, wtok) = got, want
    return tok == wtok and float(np.abs(h - wh).max()) < STATE_TOL and float(np.abs(c - wc).max()) < STATE_TOL * max(1.0, float(np.abs(wc).max()))


@pytest.mark.parametrize("numerics", MODES)
@pytest.mark.parametrize("cfg", VOCABS, ids=lambda c: f"V{c[0]}_blank{c[1]}")
def test_state_after_every_call(cfg, numerics, batch):
    """Mixed symbol rate: some stream has two or more cap frames in a row, blank frames, then a cap frame; at some call boundary
    before the last one stream has emitted an odd and another an even number of symbols, overall and within that call.  After every
    call: tokens exactly the oracle's, last token equal, h and c within the bars of _state_close."""
    V, blank = cfg
    w = CONFIGS[cfg]["mixed"]
    want, margin = _oracle(V, blank, w)
    assert margin >= MARGIN, margin
    shape = ["".join("X" if len(f) == N_STEPS else "0" if not f else "s" for f in frames) for frames, _ in want]
    assert any(re.search("XX+0+X", p) for p in shape), shape
    ends = np.cumsum([n for _, _, n in _calls()])
    cum = np.array([[len(_tokens(frames, e)) for e in ends] for frames, _ in want])          # [stream][call]
    per_call = np.diff(cum, axis=1, prepend=0)
    assert any(len(set(cum[:, j] % 2)) == 2 for j in range(len(ends) - 1)), cum
    assert any(len(set(per_call[:, j] % 2)) == 2 for j in range(len(ends) - 1)), per_call
    snaps = _run_calls(batch(V, blank, w, numerics), _x())
    for j, (toks, states) in enumerate(snaps):
        for s in range(3):
            frames, st = want[s]
            assert toks[s] == _tokens(frames, ends[j]), (j, s, len(toks[s]), int(cum[s, j]))
            assert _state_close(states[s], st[ends[j] - 1]), (j, s)


@pytest.mark.parametrize("numerics", MODES)
@pytest.mark.parametrize("cfg", [(412, 0), (512, 0)], ids=lambda c: f"V{c[0]}")
def test_saturated_runs(cfg, numerics, batch):
    """Every frame at the cap (10 symbols, then the frame advances without a blank): 210 commits per stream in 21 one-frame passes
    each, the state carried across the cap and across calls."""
    V, blank = cfg
    w = CONFIGS[cfg]["saturated"]
    want, margin = _oracle(V, blank, w)
    assert margin >= MARGIN, margin
    assert any(all(len(f) == N_STEPS for f in frames) for frames, _ in want)
    toks, states = _run_calls(batch(V, blank, w, numerics), _x())[-1]
    for s in range(3):
        frames, st = want[s]
        assert toks[s] == _tokens(frames), s
        assert _state_close(states[s], st[-1]), s


def _tie_cases():
    out = []
    for V, blank in VOCABS:
        rp = (V + 3) // 4
        for placement in (["waves", "parts"] if rp > 64 else ["parts"]):      # 129 and 6: a part's rows all sit in its first 64-row half
            out.append(pytest.param(V, blank, placement, id=f"V{V}_{placement}"))
    return out


@pytest.mark.parametrize("V,blank,placement", _tie_cases())
def test_ties_to_smaller_index(V, blank, placement, batch):
    """Exact twin rows a < b, b in the second 64-row half of a's part ("waves": the two rows one lane of the one-frame finish compares
    in registers, and the two waves the multi-frame finish merges) or in another part ("parts"): b is never emitted and the tokens
    are the oracle's, call by call."""
    w = CONFIGS[(V, blank)]["mixed"]
    a, b = _twin_pairs(V, blank, w)[placement]
    rp = (V + 3) // 4
    assert a < b and a != blank and b != blank
    if placement == "waves":
        assert a // rp == b // rp and a % rp < 64 <= b % rp
    else:
        assert a // rp != b // rp
    twins = ((a, b, TWIN_HEADS),)
    _, full_margin = _oracle_greedy(V, blank, w, twins)                        # the twin weights leave every decision clear of a near-tie
    want, margin = _oracle(V, blank, w, twins)
    assert min(margin, full_margin) >= MARGIN
    assert sum(t == a for frames, _ in want for t in _tokens(frames)) >= 2
    ends = np.cumsum([n for _, _, n in _calls()])
    snaps = _run_calls(batch(V, blank, w, "fp32", twins), _x())
    for j, (toks, _) in enumerate(snaps):
        for s in range(3):
            assert b not in toks[s], (j, s)
            assert toks[s] == _tokens(want[s][0], ends[j]), (j, s)


def _bits(snaps):
    return [(toks, [(h.tobytes(), c.tobytes(), tok) for h, c, tok in states]) for toks, states in snaps]


@pytest.mark.parametrize("numerics", MODES)
def test_repeatable(numerics, batch):
    """The same call sequence twice on one context, then on two contexts from two host threads on two streams at the same time:
    identical tokens and bit-identical h / c after every call."""
    V, blank = 412, 0
    w = CONFIGS[(V, blank)]["mixed"]
    x = _x()
    sbs = [batch(V, blank, w, numerics) for _ in range(2)]
    first = _bits(_run_calls(sbs[0], x))
    assert sum(len(t) for t in first[-1][0]) > 100
    assert _bits(_run_calls(sbs[0], x)) == first
    torch.cuda.synchronize()
    got, streams = [None, None], [torch.cuda.Stream() for _ in range(2)]

    def worker(k):
        with torch.cuda.stream(streams[k]):
            got[k] = _bits(_run_calls(sbs[k], x))
        streams[k].synchronize()

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got[0] == first and got[1] == first
