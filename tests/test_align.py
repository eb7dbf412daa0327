"""Forced alignment on the device (rnnt_transducer_align / rnnt_ctc_align, their _pick / _logprobs forms and the facade over them)
through the C ABI.  Needs a real MI355X: `pytest -m gpu`.

The pin is the definition: both Viterbi recursions are f64 additions and comparisons, so score and path must be BITWISE their
float64 restatements (ctc_vr_amd.testing.transducer_align_ref / ctc_align_ref, themselves checked against enumeration in
test_align_cpu.py) on the lattice or log-probabilities the device used, ties included; the whole call is held to the CPU oracle
within what the project's logits tolerance allows, the path wherever the oracle's margin exceeds that."""
import ctypes

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import RnntEngine

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3                  # the project's logits bar (test_gpu_parity.py)
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
ALL_MODES = PARITY_MODES + ["bf16"]
V, BLANK = T.VOCAB, T.BLANK


@pytest.fixture(params=PARITY_MODES)
def numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    return request.param


@pytest.fixture(params=ALL_MODES)
def any_numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)
    return request.param


@pytest.fixture(scope="module")
def engines(np_state_dict):
    """One small one-stream context per numerics mode (scratch: 12 * 4 * 256 * 128 floats, enough for every lattice below)."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    cache = {}

    def get(mode):
        if mode not in cache:
            eng = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=256, max_enc_frames=64, max_tokens=512, vocab_size=V,
                             blank_id=BLANK, max_beam=0)
            eng.load_state_dict(np_state_dict(0), numerics=mode)
            cache[mode] = eng
        return cache[mode]
    yield get
    for e in cache.values():
        e.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rng(k0, k1):
    """a Philox stream of its own per (k0, k1): the key is exactly two 64-bit words"""
    return np.random.Generator(np.random.Philox(key=[k0, k1]))


def _targets(B, Umax, Ub, seed, pad=-1):
    """[B, Umax] int32: row b holds Ub[b] seeded labels != blank, `pad` beyond its length (never validated, never used)"""
    g = _rng(seed, 0x5C)
    tg = np.full((B, Umax), pad, np.int32)
    for b in range(B):
        y = g.integers(0, V - 1, Ub[b])
        tg[b, :Ub[b]] = np.where(y >= BLANK, y + 1, y)
    return tg


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _align(eng, enc_d, Tb, tg, Ub, want_nll=False):
    """rnnt_transducer_align with the lattice kept -> (best, emit, nll or None, pick on the host)"""
    B, Tn = enc_d.size(0), enc_d.size(1)
    pick = torch.full((B, Tn, tg.shape[1] + 1, 2), float("nan"), device=enc_d.device)
    out = eng.transducer_align(enc_d.data_ptr(), Tb, tg, Ub, B, Tn, want_nll=want_nll, pick_ptr=pick.data_ptr(), stream=_stream())
    torch.cuda.synchronize()
    return out[0], out[1], (out[2] if want_nll else None), pick.cpu().numpy()


def _check_rows(best, emit, pick, Tb, Ub, tag):
    """score bitwise, path identical, -1 beyond U_b, against transducer_align_ref on the lattice the device used"""
    for b in range(len(Tb)):
        want, want_emit, _ = T.transducer_align_ref(pick[b], int(Tb[b]), int(Ub[b]))
        assert np.isfinite(want), (tag, b)
        assert _bits(np.float64(best[b])) == _bits(np.float64(want)), (tag, b, best[b], want)
        assert emit[b, :Ub[b]].tolist() == want_emit.tolist(), (tag, b)
        assert (emit[b, Ub[b]:] == -1).all(), (tag, b)


# ---- 1. recursion bitwise on the device's own lattice ----------------------------------------------------------------------------------
REC_CASES = {
    # name: (T, Umax, T_b, U_b): test_score.py's recursion shapes, and lengths that cross the 32-frame back-pointer words
    "u1_64": (12, 63, [12, 1, 7, 12], [63, 63, 0, 30]),
    "u1_65": (9, 64, [9, 5], [64, 33]),
    "umax_255": (6, 255, [6, 3], [255, 100]),
    "ragged": (23, 9, [23, 17, 1, 9, 20], [9, 0, 4, 9, 1]),
    "single_cell": (1, 0, [1], [0]),
    "bp_words": (65, 5, [31, 32, 33, 65, 64], [5, 3, 5, 2, 0]),
}


@pytest.mark.parametrize("case", sorted(REC_CASES))
def test_recursion_bitwise_on_device_lattice(case, engines, any_numerics):
    Tn, Umax, Tb, Ub = REC_CASES[case]
    B = len(Tb)
    eng = engines(any_numerics)
    Tb, Ub = np.array(Tb, np.int32), np.array(Ub, np.int32)
    tg = _targets(B, Umax, Ub, seed=7 + Umax)
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(1000 + Umax)).cuda()
    best, emit, _, pick = _align(eng, enc_d, Tb, tg, Ub)
    assert emit.shape == (B, max(Umax, 1)) and emit.dtype == np.int32
    _check_rows(best, emit, pick, Tb, Ub, case)


# ---- 2. ties through the seam ------------------------------------------------------------------------------------------------------------
TIE_GROUPS = [
    # (T, Umax, rows, lengths every group must contain): 204 cases in all
    (12, 63, 34, [(12, 63), (1, 63), (7, 0), (12, 30)]),
    (9, 64, 34, [(9, 64), (5, 33)]),
    (6, 255, 8, [(6, 255), (3, 100)]),
    (23, 9, 50, [(23, 9), (17, 0), (1, 4)]),
    (1, 0, 4, [(1, 0)]),
    (65, 5, 74, [(31, 5), (32, 5), (33, 5), (65, 5), (64, 0), (32, 1)]),
]


@pytest.mark.parametrize("group", TIE_GROUPS, ids=lambda g: f"T{g[0]}_U{g[1]}")
def test_transducer_ties_through_the_seam(group, engines):
    """rnnt_transducer_align_pick on uploaded lattices of multiples of 0.25 (ties everywhere); cells outside a row's lengths are NaN"""
    Tn, Umax, B, fixed = group
    eng = engines("bf16x3")
    g = _rng(Tn * 1000 + Umax, 0x71E)
    Tb = np.array([f[0] for f in fixed] + [int(g.integers(1, Tn + 1)) for _ in range(B - len(fixed))], np.int32)
    Ub = np.array([f[1] for f in fixed] + [int(g.integers(0, Umax + 1)) for _ in range(B - len(fixed))], np.int32)
    pick = (-0.25 * g.integers(0, 8, (B, Tn, Umax + 1, 2))).astype(np.float32)
    for b in range(B):
        pick[b, Tb[b]:] = np.nan
        pick[b, :, Ub[b] + 1:] = np.nan
        pick[b, :, Ub[b], 1] = np.nan
    pick_d = torch.from_numpy(pick).cuda()
    best, emit = eng.transducer_align_pick(pick_d.data_ptr(), Tb, Ub, B, Tn, Umax, _stream())
    _check_rows(best, emit, pick, Tb, Ub, "ties")


CTC_T_EDGES = [15, 16, 17, 33]


def _ctc_tie_rows(seed, B, Tn, Umax):
    """rows over a 3-label alphabet (adjacent repeats are common), lengths over the 16-frame pack edges, some infeasible"""
    g = _rng(seed, 0xC7C)
    Tb = np.array([CTC_T_EDGES[b % 4] if b < 16 else int(g.integers(1, Tn + 1)) for b in range(B)], np.int32)
    tl = np.array([b % (Umax + 1) for b in range(B)], np.int32)
    tg = np.full((B, Umax), -1, np.int32)
    for b in range(B):
        tg[b, :tl[b]] = g.choice([7, 9, 3], tl[b])
    return Tb, tg, tl


def _check_ctc_rows(best, align, lp, Tb, tg, tl, tag):
    feasible = 0
    for b in range(len(Tb)):
        y = tg[b, :tl[b]].tolist()
        want, want_align = T.ctc_align_ref(lp[b], y, int(Tb[b]), BLANK)
        assert _bits(np.float64(best[b])) == _bits(np.float64(want)), (tag, b, best[b], want)
        assert align[b, :Tb[b]].tolist() == want_align.tolist(), (tag, b)
        assert (align[b, Tb[b]:] == -1).all(), (tag, b)
        if np.isfinite(want):
            feasible += 1
            a = align[b, :Tb[b]]
            assert [int(v) for i, v in enumerate(a) if v != BLANK and (i == 0 or v != a[i - 1])] == y, (tag, b)   # collapses to the transcript
        else:
            assert want == -np.inf and (align[b] == -1).all(), (tag, b)
    return feasible


@pytest.mark.parametrize("part", range(4))
def test_ctc_ties_through_the_seam(part, engines):
    """rnnt_ctc_align_logprobs on uploaded quantised "log-probabilities" (they need not normalise: the recursion only adds):
    4 x 50 seeded cases"""
    B, Tn, Umax = 50, 33, 12
    eng = engines("bf16x3")
    Tb, tg, tl = _ctc_tie_rows(part, B, Tn, Umax)
    g = _rng(part, 0x10)
    lp = (-0.25 * g.integers(0, 4, (B, Tn, V))).astype(np.float32)
    for b in range(B):
        lp[b, Tb[b]:] = np.nan
    lp_d = torch.from_numpy(lp).cuda()
    best, align = eng.ctc_align_logprobs(lp_d.data_ptr(), Tb, tg, tl, B, Tn, _stream())
    feasible = _check_ctc_rows(best, align, lp, Tb, tg, tl, "ctc ties")
    assert 0 < feasible < B            # both kinds of row are among the cases


# ---- 3. CTC on the device's own log-probabilities ----------------------------------------------------------------------------------------
def test_ctc_align_on_device_logprobs(engines, numerics):
    eng = engines(numerics)
    g = _rng(8, 8)
    long_row = g.integers(0, V - 1, 255)
    long_row = np.where(long_row >= BLANK, long_row + 1, long_row)
    rows = [list(long_row), [], [7, 7, 7, 9, 9, 3], [8, 8, 8, 8, 8], [6, 6, 11], [1, 2, 3, 4, 6, 7, 8], [9], [30, 30, 31, 31, 30]]
    el = np.array([300, 50, 20, 6, 15, 16, 17, 33], np.int32)         # row 3: five equal labels need 9 frames
    B, Tn, Umax = len(rows), 300, 255
    tl = np.array([len(r) for r in rows], np.int32)
    tg = np.full((B, Umax), -1, np.int32)
    for b, r in enumerate(rows):
        tg[b, :len(r)] = r
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(8)).cuda()
    best, align = eng.ctc_align(enc_d.data_ptr(), el, tg, tl, B, Tn, _stream())
    lp_d = torch.empty(B * Tn, V, device="cuda")
    eng.ctc_logprobs(enc_d.data_ptr(), B * Tn, lp_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    lp = lp_d.view(B, Tn, V).cpu().numpy()
    assert align.shape == (B, Tn) and align.dtype == np.int32
    assert _check_ctc_rows(best, align, lp, el, tg, tl, numerics) == B - 1
    assert best[3] == -np.inf and (align[3] == -1).all()
    nll = eng.ctc_nll(enc_d.data_ptr(), el, tg, tl, B, Tn, _stream())
    assert np.isposinf(nll[3]) and (best[np.isfinite(nll)] <= -nll[np.isfinite(nll)]).all()      # the best path is one term of the sum


# ---- 4. consistency with the scorer -------------------------------------------------------------------------------------------------------
def test_nll_of_the_same_call_is_the_scorers(engines, any_numerics):
    eng = engines(any_numerics)
    Tn, Umax = 23, 9
    Tb, Ub = np.array([23, 17, 1, 9, 20], np.int32), np.array([9, 0, 4, 9, 1], np.int32)
    B = len(Tb)
    tg = _targets(B, Umax, Ub, seed=3)
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(3)).cuda()
    best, emit, nll, pick = _align(eng, enc_d, Tb, tg, Ub, want_nll=True)
    want = eng.transducer_nll(enc_d.data_ptr(), Tb, tg, Ub, B, Tn, None, _stream())
    assert np.isfinite(nll).all() and np.array_equal(_bits(nll), _bits(want))
    assert (best <= -nll).all()
    best2, emit2 = eng.transducer_align(enc_d.data_ptr(), Tb, tg, Ub, B, Tn, stream=_stream())     # without nll, without a kept lattice
    assert np.array_equal(_bits(best2), _bits(best)) and np.array_equal(emit2, emit)


# ---- 5. end to end against the CPU oracle -------------------------------------------------------------------------------------------------
# test_score.py's end-to-end shapes; the seed is chosen on the CPU among 31..38 for the oracle's margins (the gap between the best
# path and the best path through any cell off it, transducer_align_ref over the oracle's lattice): 0.789, 1.631, 1.550 against
# the bound 2 (T_b + U_b) delta at delta = 2 LOGIT_TOL = 0.108, 0.064, 0.052.  (Seed 31 has an utterance with margin 6e-4.)
E2E = dict(B=3, Tn=21, Umax=6, Tb=[21, 13, 8], Ub=[6, 3, 5], seed=34)
E2E_MARGINS = [0.788698, 1.630545, 1.550076]


def _oracle_pick(np_state_dict, enc, tg, Ub):
    """test_score.py::test_end_to_end_vs_oracle's construction: O.predictor_step from the zero state, O.joint, log-softmax"""
    from oracle import rnnt_oracle as O
    B, Umax = tg.shape
    sd = O.to_torch_sd(np_state_dict(0))
    state = O.predictor_init_state(B)
    outs = []
    for u in range(Umax + 1):
        tok = torch.tensor([[int(tg[b, u - 1]) if 1 <= u <= Ub[b] else BLANK] for b in range(B)], dtype=torch.long)
        out, state = O.predictor_step(sd, tok, state)
        outs.append(out)
    lp = torch.log_softmax(O.joint(sd, enc, torch.cat(outs, 1)), dim=-1).numpy()      # [B, T, U1, V]
    want = np.zeros(lp.shape[:3] + (2,), np.float32)
    want[..., 0] = lp[..., BLANK]
    for b in range(B):
        for u in range(Ub[b]):
            want[b, :, u, 1] = lp[b, :, u, tg[b, u]]
    return want


def _e2e_inputs():
    c = E2E
    Tb, Ub = np.array(c["Tb"], np.int32), np.array(c["Ub"], np.int32)
    tg = _targets(c["B"], c["Umax"], Ub, seed=c["seed"])
    enc = torch.randn(c["B"], c["Tn"], 256, generator=torch.Generator().manual_seed(c["seed"]))
    return enc, Tb, tg, Ub


def test_end_to_end_vs_oracle(engines, numerics, np_state_dict):
    enc, Tb, tg, Ub = _e2e_inputs()
    B, Tn, U1 = enc.size(0), enc.size(1), tg.shape[1] + 1
    eng = engines(numerics)
    best, emit, _, pick = _align(eng, enc.cuda(), Tb, tg, Ub)
    want_pick = _oracle_pick(np_state_dict, enc, tg, Ub)
    t, u = np.arange(Tn)[None, :, None], np.arange(U1)[None, None, :]
    vb, vl = (t < Tb[:, None, None]) & (u <= Ub[:, None, None]), (t < Tb[:, None, None]) & (u < Ub[:, None, None])
    d = np.abs(pick.astype(np.float64) - want_pick.astype(np.float64))
    delta = max(float(d[..., 0][vb].max()), float(d[..., 1][vl].max()))
    print(f"{numerics}: delta = {delta:.3e}")
    assert delta <= 2 * LOGIT_TOL
    out_of_check = 0
    for b in range(B):
        n = int(Tb[b]) + int(Ub[b])
        want, want_emit, margin = T.transducer_align_ref(want_pick[b], int(Tb[b]), int(Ub[b]))
        assert margin == pytest.approx(E2E_MARGINS[b], abs=1e-3) and margin > 2 * n * 2 * LOGIT_TOL      # chosen on the CPU, see above
        bound = n * delta + 1e-9 * abs(best[b])
        print(f"{numerics} b={b}: best={best[b]!r} oracle={want!r} diff={abs(best[b] - want):.3e} bound={bound:.3e} margin={margin:.4f}")
        assert abs(best[b] - want) <= bound
        if margin > 2 * n * delta:
            assert emit[b, :Ub[b]].tolist() == want_emit.tolist(), (b, emit[b], want_emit)
        else:
            out_of_check += 1
            print(f"{numerics} b={b}: margin {margin:.4e} <= 2 (T_b + U_b) delta = {2 * n * delta:.4e}: path not compared")
    assert out_of_check <= 1


# ---- 6. padding is never read -------------------------------------------------------------------------------------------------------------
def test_padding_is_never_read(engines, numerics):
    B, Tn, Umax = 4, 35, 7
    eng = engines(numerics)
    Tb, Ub = np.array([35, 33, 20, 9], np.int32), np.array([7, 5, 0, 3], np.int32)
    clean_t = _targets(B, Umax, Ub, seed=5, pad=3)               # a valid label in the padding
    dirty_t = _targets(B, Umax, Ub, seed=5, pad=-1)
    enc = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(5))
    dirty = enc.clone()
    for b in range(B):
        dirty[b, Tb[b]:] = float("nan")
    s = _stream()
    best_c, emit_c, nll_c = eng.transducer_align(enc.cuda().data_ptr(), Tb, clean_t, Ub, B, Tn, want_nll=True, stream=s)
    best_d, emit_d, nll_d = eng.transducer_align(dirty.cuda().data_ptr(), Tb, dirty_t, Ub, B, Tn, want_nll=True, stream=s)
    assert np.isfinite(best_d).all()
    assert np.array_equal(_bits(best_d), _bits(best_c)) and np.array_equal(emit_d, emit_c) and np.array_equal(_bits(nll_d), _bits(nll_c))
    cb_c, al_c = eng.ctc_align(enc.cuda().data_ptr(), Tb, clean_t, Ub, B, Tn, s)
    cb_d, al_d = eng.ctc_align(dirty.cuda().data_ptr(), Tb, dirty_t, Ub, B, Tn, s)
    assert np.isfinite(cb_d).all()
    assert np.array_equal(_bits(cb_d), _bits(cb_c)) and np.array_equal(al_d, al_c)


# ---- 7. determinism and batch placement ---------------------------------------------------------------------------------------------------
def test_determinism_and_placement(engines, numerics):
    B, Tn, Umax = 5, 33, 8
    eng = engines(numerics)
    Tb, Ub = np.array([33, 28, 22, 17, 11], np.int32), np.array([8, 4, 1, 5, 0], np.int32)
    tg = _targets(B, Umax, Ub, seed=9)
    enc = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(9))
    perm = np.array([3, 0, 4, 2, 1])
    enc_p = enc[torch.from_numpy(perm)].contiguous().cuda()
    s = _stream()
    best, emit = eng.transducer_align(enc.cuda().data_ptr(), Tb, tg, Ub, B, Tn, stream=s)
    best2, emit2 = eng.transducer_align(enc.cuda().data_ptr(), Tb, tg, Ub, B, Tn, stream=s)
    best_p, emit_p = eng.transducer_align(enc_p.data_ptr(), Tb[perm], tg[perm], Ub[perm], B, Tn, stream=s)
    assert np.array_equal(_bits(best), _bits(best2)) and np.array_equal(emit, emit2)
    assert np.array_equal(_bits(best_p), _bits(best[perm])) and np.array_equal(emit_p, emit[perm])
    cb, al = eng.ctc_align(enc.cuda().data_ptr(), Tb, tg, Ub, B, Tn, s)
    cb2, al2 = eng.ctc_align(enc.cuda().data_ptr(), Tb, tg, Ub, B, Tn, s)
    cb_p, al_p = eng.ctc_align(enc_p.data_ptr(), Tb[perm], tg[perm], Ub[perm], B, Tn, s)
    assert np.isfinite(cb).all()
    assert np.array_equal(_bits(cb), _bits(cb2)) and np.array_equal(al, al2)
    assert np.array_equal(_bits(cb_p), _bits(cb[perm])) and np.array_equal(al_p, al[perm])


# ---- 8. streaming state is left alone -----------------------------------------------------------------------------------------------------
def test_streaming_state_is_left_alone(engines, numerics):
    """Two chunks through the per-chunk API of a one-stream context, with and without alignment calls between them: same tokens,
    same K/V cache, same conv cache, same predictor state."""
    eng = engines(numerics)
    x = torch.from_numpy(T.synth_fbank(1, 64, seed=21)).cuda()
    enc_d = torch.randn(2, 15, 256, generator=torch.Generator().manual_seed(2)).cuda()
    Tb, Ub = np.array([15, 9], np.int32), np.array([4, 2], np.int32)
    tg = _targets(2, 4, Ub, seed=2)

    def run(with_call):
        s = _stream()
        eng.reset(1, s)
        off = 0
        for ci in range(2):
            chunk = x[:, ci * 32:(ci + 1) * 32].contiguous()
            eng.encoder_chunk(chunk.data_ptr(), 32, off, off, s)
            eng.greedy_decode(s)
            eng.frames_consume(s)
            off += 32 // 4
            if with_call and ci == 0:
                best, _, nll = eng.transducer_align(enc_d.data_ptr(), Tb, tg, Ub, 2, 15, want_nll=True, stream=s)
                cbest, _ = eng.ctc_align(enc_d.data_ptr(), Tb, tg, Ub, 2, 15, s)
                assert np.isfinite(best).all() and np.isfinite(nll).all() and np.isfinite(cbest).all()
        return eng.tokens(s)[0], eng.att_cache(0, s), eng.cnn_cache(0, s), eng.predictor_state(0, s)
    tok_a, att_a, cnn_a, (h_a, c_a, last_a) = run(False)
    tok_b, att_b, cnn_b, (h_b, c_b, last_b) = run(True)
    assert att_a.shape[2] > 0
    assert tok_a == tok_b and last_a == last_b
    assert np.array_equal(_bits(att_a), _bits(att_b)) and np.array_equal(_bits(cnn_a), _bits(cnn_b))
    assert np.array_equal(_bits(h_a), _bits(h_b)) and np.array_equal(_bits(c_a), _bits(c_b))


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------------
FNS = ["rnnt_transducer_align", "rnnt_transducer_align_pick", "rnnt_ctc_align", "rnnt_ctc_align_logprobs"]


def _raw(eng, fn, dev, el, tg, tl, B, Tn, Umax, best, path):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    f = getattr(eng.lib, fn)
    if fn == "rnnt_transducer_align":
        return f(eng.ctx, dev, p(el), p(tg), p(tl), B, Tn, Umax, p(best), p(path), None, None, _stream())
    if fn == "rnnt_transducer_align_pick":
        return f(eng.ctx, dev, p(el), p(tl), B, Tn, Umax, p(best), p(path), _stream())
    return f(eng.ctx, dev, p(el), p(tg), p(tl), B, Tn, Umax, p(best), p(path), _stream())


@pytest.mark.parametrize("fn", FNS)
def test_refusals(fn, engines, numerics, np_state_dict):
    eng = engines(numerics)
    B, Tn, Umax = 2, 10, 3
    has_labels, ctc = fn != "rnnt_transducer_align_pick", "ctc" in fn
    g = torch.Generator().manual_seed(4)
    if fn == "rnnt_transducer_align_pick":
        dev_t = -torch.rand(B, Tn, Umax + 1, 2, generator=g).cuda()
    elif fn == "rnnt_ctc_align_logprobs":
        dev_t = -torch.rand(B, Tn, V, generator=g).cuda()
    else:
        dev_t = torch.randn(B, Tn, 256, generator=g).cuda()
    el, tl = np.array([10, 6], np.int32), np.array([3, 1], np.int32)
    tg = np.array([[7, 0, V - 1], [BLANK + 1, -5, BLANK]], np.int32)       # row 1's entries beyond its length are invalid on purpose
    n_path = Tn if ctc else Umax
    best, path = np.zeros(B, np.float64), np.zeros((B, n_path), np.int32)
    dp = dev_t.data_ptr()

    def valid():
        ob, op = np.full(B, np.nan), np.full((B, n_path), -7, np.int32)
        assert _raw(eng, fn, dp, el, tg, tl, B, Tn, Umax, ob, op) == 0, eng.lib.rnnt_last_error(eng.ctx)
        return ob, op
    base_b, base_p = valid()
    assert np.isfinite(base_b).all() and (base_p != -7).all()

    def refused(code, **kw):
        a = dict(dev=dp, el=el, tg=tg, tl=tl, B=B, Tn=Tn, Umax=Umax, best=best, path=path)
        a.update(kw)
        rc = _raw(eng, fn, a["dev"], a["el"], a["tg"], a["tl"], a["B"], a["Tn"], a["Umax"], a["best"], a["path"])
        assert rc == code, (kw.keys(), rc, eng.lib.rnnt_last_error(eng.ctx))
        assert eng.lib.rnnt_last_error(eng.ctx) != b""
        ob, op = valid()                                             # a following valid call is unaffected
        assert np.array_equal(_bits(ob), _bits(base_b)) and np.array_equal(op, base_p)
    A, S, ST = rlib.ERR_ARG, rlib.ERR_SHAPE, rlib.ERR_STATE
    for k in ("dev", "el", "tl", "best", "path") + (("tg",) if has_labels else ()):      # null pointers
        refused(A, **{k: None})
    refused(A, B=0)
    refused(A, el=np.array([0, 6], np.int32))                       # T_b outside [1, T]
    refused(A, el=np.array([10, 11], np.int32))
    refused(A, tl=np.array([-1, 1], np.int32))                      # U_b / L_b outside [0, Umax]
    refused(A, tl=np.array([3, 4], np.int32))
    if has_labels:
        refused(A, tg=np.array([[7, V, 1], [6, 0, 0]], np.int32))       # a label outside [0, V) inside the valid length
        refused(A, tg=np.array([[7, -1, 1], [6, 0, 0]], np.int32))
        refused(A, tg=np.array([[7, BLANK, 1], [6, 0, 0]], np.int32))   # the blank inside the valid length
    refused(S, tg=np.ones((B, 256), np.int32), Umax=256, path=np.zeros((B, max(n_path, 256)), np.int32))      # Umax > 255
    if fn == "rnnt_transducer_align":                               # lattice beyond the scratch: 64 * 128 frames of 256 floats > 12 * 4 * 256 * 128
        Bb = 64
        refused(S, B=Bb, Tn=128, el=np.full(Bb, 128, np.int32), tl=np.zeros(Bb, np.int32), tg=np.ones((Bb, Umax), np.int32),
                best=np.zeros(Bb, np.float64), path=np.zeros((Bb, Umax), np.int32))
    # weights not finalised
    fresh = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    try:
        assert _raw(fresh, fn, dp, el, tg, tl, B, Tn, Umax, best, path) == ST
        assert fresh.lib.rnnt_last_error(fresh.ctx) != b""
        if fn == "rnnt_ctc_align":                                  # the CTC head is optional: without it the call is a state error
            sd = {k: v for k, v in np_state_dict(0).items() if not k.startswith("ctc_head.")}
            fresh.load_state_dict(sd, numerics=numerics)
            assert _raw(fresh, fn, dp, el, tg, tl, B, Tn, Umax, best, path) == ST
            assert b"ctc_head" in fresh.lib.rnnt_last_error(fresh.ctx)
    finally:
        fresh.close()


# ---- 10. facade ---------------------------------------------------------------------------------------------------------------------------
def test_facade_align(numerics, np_state_dict):
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel, peaks_from_ctc_alignment
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=V, blank_id=BLANK, streaming=False, predictor_dropout=0, ctc_weight=0.3,
                        max_streams=2, max_chunk_frames=128, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=0)
    m.load_state_dict(np_state_dict(0))
    audios = torch.from_numpy(T.synth_fbank(2, 120, seed=41))
    lens = torch.tensor([120, 90])
    texts = torch.tensor([[7, 0, V - 1, 9], [BLANK + 1, 33, -1, -1]])
    text_lens = torch.tensor([4, 2])
    enc, enc_lens, tg, tl = m._encode_for_scoring(audios, lens, texts, text_lens)
    assert enc_lens[0] != enc_lens[1]
    s = _stream()
    want = {"rnnt": m._engine.transducer_align(enc.data_ptr(), enc_lens, tg, tl, 2, enc.size(1), stream=s),
            "ctc": m._engine.ctc_align(enc.data_ptr(), enc_lens, tg, tl, 2, enc.size(1), s)}
    for method in ("rnnt", "ctc"):
        out = m.align(audios, lens, texts, text_lens, method=method)
        assert len(out) == 2
        for b, r in enumerate(out):
            n, dur = int(text_lens[b]), int(enc_lens[b]) * 0.04
            assert set(r) == {"tokens", "frames", "times", "log_prob"}
            assert r["tokens"] == texts[b, :n].tolist() and len(r["frames"]) == n and len(r["times"]) == n
            assert all(0 <= f < enc_lens[b] for f in r["frames"]) and all(a <= c for a, c in zip(r["frames"], r["frames"][1:]))
            assert all(0 <= st <= en <= dur for st, en in r["times"])
            assert all(r["times"][i][1] <= r["times"][i + 1][0] for i in range(n - 1))           # ordered, non-overlapping
            assert r["log_prob"] == want[method][0][b] and np.isfinite(r["log_prob"])
            if method == "ctc":
                assert r["frames"] == peaks_from_ctc_alignment(want[method][1][b, :enc_lens[b]].tolist(), BLANK)
                assert all(f < g_ for f, g_ in zip(r["frames"], r["frames"][1:]))
            else:
                assert r["frames"] == want[method][1][b, :n].tolist()
    m._engine.close()
