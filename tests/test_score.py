"""Teacher-forced scoring on the device (rnnt_transducer_nll / rnnt_ctc_nll and the facade over them) through the C ABI.
Needs a real MI355X: `pytest -m gpu`.

The pin is the mathematical definition (minus the log of the sum over all monotonic alignments; nn.CTCLoss for the CTC term):
the picked lattice must be bitwise the lattice rnnt_joint(mode=1) writes at the two columns, the f64 recursion must agree with
its float64 restatement (ctc_vr_amd.testing.transducer_nll_ref, torch's CPU ctc_loss) to 1e-9 relative, and the whole call
with the CPU oracle within what the project's logits tolerance allows."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import RnntEngine, RnntError

pytestmark = pytest.mark.gpu

LOGIT_TOL = 1e-3                  # the project's logits bar (test_gpu_parity.py)
REC_RTOL = 1e-9                   # recursion vs its float64 restatement: <= ~400 contraction steps of a few f64 ulps at |alpha| <~ 1e3
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
ALL_MODES = PARITY_MODES + ["bf16"]     # plain bf16 has no parity bar against the oracle, but its kernels owe the same bitwise contracts
V, BLANK = T.VOCAB, T.BLANK


@pytest.fixture(params=PARITY_MODES)
def numerics(request, monkeypatch):
    monkeypatch.setenv("RNNT_NUMERICS", request.param)   # contexts created in the test pick it up (lib.numerics_id)
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


EDGE_LABELS = [0, V - 1, BLANK - 1, BLANK + 1]


def _targets(B, Umax, Ub, seed, pad=-1):
    """[B, Umax] int32: row b holds Ub[b] labels != blank -- the edge labels (0, V-1, the blank's neighbours) first, spread over the
    rows, then seeded random ones -- and `pad` beyond its length (never validated, never used)."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0x5C]))
    tg = np.full((B, Umax), pad, np.int32)
    k = 0
    for b in range(B):
        for u in range(Ub[b]):
            if (u + b) % 3 == 0:
                tg[b, u] = EDGE_LABELS[k % 4]
                k += 1
            else:
                y = int(g.integers(0, V - 1))
                tg[b, u] = y + 1 if y >= BLANK else y              # uniform over the non-blank labels
    return tg


def _ragged(B, Tn, Umax):
    """lengths that differ in both directions inside the batch; row 0 is full"""
    Tb = [max(1, Tn - (b * Tn) // (B + 1)) for b in range(B)]
    Ub = [Umax if b == 0 else (Umax * ((3 * b) % (B + 1))) // (B + 1) for b in range(B)]
    return np.array(Tb, np.int32), np.array(Ub, np.int32)


def _valid_masks(B, Tn, U1, Tb, Ub):
    """blank values are valid at t < T_b, u <= U_b; label values at t < T_b, u < U_b"""
    t = np.arange(Tn)[None, :, None]
    u = np.arange(U1)[None, None, :]
    tb, ub = np.asarray(Tb)[:, None, None], np.asarray(Ub)[:, None, None]
    return (t < tb) & (u <= ub), (t < tb) & (u < ub)


def _score(eng, enc_d, Tb, tg, Ub, want_pick=True):
    B, Tn = enc_d.size(0), enc_d.size(1)
    U1 = tg.shape[1] + 1
    pick = torch.full((B, Tn, U1, 2), float("nan"), device=enc_d.device) if want_pick else None
    nll = eng.transducer_nll(enc_d.data_ptr(), Tb, tg, Ub, B, Tn, pick.data_ptr() if want_pick else None, _stream())
    torch.cuda.synchronize()
    return nll, (pick.cpu().numpy() if want_pick else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _pred_rows(eng, tg, Ub, dev):
    """The predictor over [blank, y_1 .. y_Umax] from the zero state through rnnt_predictor_step: pred [B, U1, 256] on the device."""
    B, Umax = tg.shape
    h = torch.zeros(B, 256, device=dev)
    c = torch.zeros(B, 256, device=dev)
    pred = torch.empty(B, Umax + 1, 256, device=dev)
    for u in range(Umax + 1):
        tok = np.array([tg[b, u - 1] if 1 <= u <= Ub[b] else BLANK for b in range(B)], np.int32)
        tok_d = torch.from_numpy(tok).to(dev)
        out, h2, c2 = torch.empty(B, 256, device=dev), torch.empty(B, 256, device=dev), torch.empty(B, 256, device=dev)
        eng.predictor_step(tok_d.data_ptr(), h.data_ptr(), c.data_ptr(), B, out.data_ptr(), h2.data_ptr(), c2.data_ptr(), _stream())
        pred[:, u] = out
        h, c = h2, c2
    return pred


# ---- 1. pick = lattice, bitwise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 37, 11), (2, 129, 3), (8, 160, 28)])
def test_pick_is_the_lattice_bitwise(shape, engines, any_numerics):
    """pick_dev equals rnnt_joint(mode=1) gathered at (blank, target) on every valid cell, bit for bit; (8, 160, 28) is 560 row
    tiles, more than the persistent grid holds, so workgroups draw from the tile queue."""
    B, Tn, U1 = shape
    Umax = U1 - 1
    eng = engines(any_numerics)
    dev = torch.device("cuda", 0)
    Tb, Ub = _ragged(B, Tn, Umax)
    tg = _targets(B, Umax, Ub, seed=100 * B + Tn)
    if B >= 3:
        used = {int(tg[b, u]) for b in range(B) for u in range(Ub[b])}
        assert set(EDGE_LABELS) <= used and BLANK not in used
    g = torch.Generator().manual_seed(100 * B + Tn)
    enc_d = torch.randn(B, Tn, 256, generator=g).to(dev)
    nll, pick = _score(eng, enc_d, Tb, tg, Ub)
    assert np.isfinite(nll).all()
    pred = _pred_rows(eng, tg, Ub, dev)
    lat = torch.full((B, Tn, U1, V), float("nan"), device=dev)
    eng.joint(enc_d.data_ptr(), pred.data_ptr(), B, Tn, U1, 1, lat.data_ptr(), _stream())
    torch.cuda.synchronize()
    col = np.full((B, U1), BLANK, np.int64)
    for b in range(B):
        col[b, :Ub[b]] = tg[b, :Ub[b]]
    idx = torch.from_numpy(col).to(dev)[:, None, :, None].expand(B, Tn, U1, 1)
    want_blank = lat[..., BLANK].cpu().numpy()
    want_label = lat.gather(3, idx)[..., 0].cpu().numpy()
    vb, vl = _valid_masks(B, Tn, U1, Tb, Ub)
    assert np.isfinite(pick[..., 0][vb]).all() and np.isfinite(pick[..., 1][vl]).all()
    assert np.array_equal(_bits(pick[..., 0])[vb], _bits(want_blank)[vb])
    assert np.array_equal(_bits(pick[..., 1])[vl], _bits(want_label)[vl])


# ---- 2. recursion -----------------------------------------------------------------------------------------------------------------
REC_CASES = {
    # name: (T, Umax, T_b, U_b)
    "u1_64": (12, 63, [12, 1, 7, 12], [63, 63, 0, 30]),          # U1 = 64: one full wavefront; T_b = 1 and U_b = 0 rows
    "u1_65": (9, 64, [9, 5], [64, 33]),                          # U1 = 65: across a wavefront of 64 lanes
    "umax_255": (6, 255, [6, 3], [255, 100]),
    "ragged": (23, 9, [23, 17, 1, 9, 20], [9, 0, 4, 9, 1]),      # rows differ in both lengths
    "single_cell": (1, 0, [1], [0]),
}


@pytest.mark.parametrize("case", sorted(REC_CASES))
def test_recursion_matches_float64_dp(case, engines, any_numerics):
    Tn, Umax, Tb, Ub = REC_CASES[case]
    B = len(Tb)
    eng = engines(any_numerics)
    Tb, Ub = np.array(Tb, np.int32), np.array(Ub, np.int32)
    tg = _targets(B, Umax, Ub, seed=7 + Umax)
    g = torch.Generator().manual_seed(1000 + Umax)
    enc_d = torch.randn(B, Tn, 256, generator=g).cuda()
    nll, pick = _score(eng, enc_d, Tb, tg, Ub)
    for b in range(B):
        want = T.transducer_nll_ref(pick[b], int(Tb[b]), int(Ub[b]))
        print(f"{case} b={b} T_b={Tb[b]} U_b={Ub[b]} nll={nll[b]!r} dp={want!r} rel={abs(nll[b] - want) / abs(want):.3e}")
        assert math.isfinite(want)
        assert abs(nll[b] - want) <= REC_RTOL * abs(want), (case, b, nll[b], want)


# ---- 3. end to end against the oracle -----------------------------------------------------------------------------------------------
def test_end_to_end_vs_oracle(engines, numerics, np_state_dict):
    """CPU side: O.predictor_step from the zero state, O.joint, log-softmax, the f64 DP.  With delta = max |pick - oracle| over the
    valid cells: delta <= 2 LOGIT_TOL (the logits bar bounds the log-sum-exp by the same amount), and since every alignment is a
    sum of T_b + U_b cell terms, |nll - nll_oracle| <= (T_b + U_b) delta + 1e-9 |nll|."""
    from oracle import rnnt_oracle as O
    B, Tn, Umax = 3, 21, 6
    eng = engines(numerics)
    Tb, Ub = np.array([21, 13, 8], np.int32), np.array([6, 3, 5], np.int32)
    tg = _targets(B, Umax, Ub, seed=31)
    g = torch.Generator().manual_seed(31)
    enc = torch.randn(B, Tn, 256, generator=g)
    nll, pick = _score(eng, enc.cuda(), Tb, tg, Ub)
    sd = O.to_torch_sd(np_state_dict(0))
    state = O.predictor_init_state(B)
    outs = []
    for u in range(Umax + 1):
        tok = torch.tensor([[int(tg[b, u - 1]) if 1 <= u <= Ub[b] else BLANK] for b in range(B)], dtype=torch.long)
        out, state = O.predictor_step(sd, tok, state)
        outs.append(out)
    lp = torch.log_softmax(O.joint(sd, enc, torch.cat(outs, 1)), dim=-1).numpy()      # [B, T, U1, V]
    vb, vl = _valid_masks(B, Tn, Umax + 1, Tb, Ub)
    want_pick = np.zeros((B, Tn, Umax + 1, 2), np.float32)
    want_pick[..., 0] = lp[..., BLANK]
    for b in range(B):
        for u in range(Ub[b]):
            want_pick[b, :, u, 1] = lp[b, :, u, tg[b, u]]
    d = np.abs(pick.astype(np.float64) - want_pick.astype(np.float64))
    delta = max(float(d[..., 0][vb].max()), float(d[..., 1][vl].max()))
    print(f"{numerics}: delta = {delta:.3e}")
    assert delta <= 2 * LOGIT_TOL
    for b in range(B):
        want = T.transducer_nll_ref(want_pick[b], int(Tb[b]), int(Ub[b]))
        bound = (int(Tb[b]) + int(Ub[b])) * delta + 1e-9 * abs(nll[b])
        print(f"{numerics} b={b}: nll={nll[b]!r} oracle={want!r} diff={abs(nll[b] - want):.3e} bound={bound:.3e}")
        assert abs(nll[b] - want) <= bound


# ---- 4. padding is never read ---------------------------------------------------------------------------------------------------------
def test_padding_is_never_read(engines, numerics):
    B, Tn, Umax = 4, 19, 7
    eng = engines(numerics)
    Tb, Ub = _ragged(B, Tn, Umax)
    assert (Tb < Tn).any() and (Ub < Umax).any()
    clean_t = _targets(B, Umax, Ub, seed=5, pad=3)               # a valid label in the padding
    dirty_t = _targets(B, Umax, Ub, seed=5, pad=-1)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(B, Tn, 256, generator=g)
    dirty = enc.clone()
    for b in range(B):
        dirty[b, Tb[b]:] = float("nan")
    nll_clean, _ = _score(eng, enc.cuda(), Tb, clean_t, Ub, want_pick=False)
    nll_dirty, _ = _score(eng, dirty.cuda(), Tb, dirty_t, Ub, want_pick=False)
    assert np.isfinite(nll_dirty).all()
    assert np.array_equal(_bits(nll_dirty), _bits(nll_clean))


# ---- 5. determinism and placement -----------------------------------------------------------------------------------------------------
def test_determinism_and_placement(engines, numerics):
    B, Tn, Umax = 5, 33, 8
    eng = engines(numerics)
    Tb, Ub = _ragged(B, Tn, Umax)
    tg = _targets(B, Umax, Ub, seed=9)
    g = torch.Generator().manual_seed(9)
    enc = torch.randn(B, Tn, 256, generator=g)
    nll, pick = _score(eng, enc.cuda(), Tb, tg, Ub)
    nll2, pick2 = _score(eng, enc.cuda(), Tb, tg, Ub)
    vb, vl = _valid_masks(B, Tn, Umax + 1, Tb, Ub)
    assert np.array_equal(_bits(nll), _bits(nll2))
    assert np.array_equal(_bits(pick[..., 0])[vb], _bits(pick2[..., 0])[vb]) and np.array_equal(_bits(pick[..., 1])[vl], _bits(pick2[..., 1])[vl])
    perm = np.array([3, 0, 4, 2, 1])
    nll_p, pick_p = _score(eng, enc[torch.from_numpy(perm)].contiguous().cuda(), Tb[perm], tg[perm], Ub[perm])
    assert np.array_equal(_bits(nll_p), _bits(nll[perm]))
    assert np.array_equal(_bits(pick_p[..., 0])[vb[perm]], _bits(pick[perm][..., 0])[vb[perm]])
    assert np.array_equal(_bits(pick_p[..., 1])[vl[perm]], _bits(pick[perm][..., 1])[vl[perm]])


# ---- 6. state is left alone -------------------------------------------------------------------------------------------------------------
def test_streaming_state_is_left_alone(engines, numerics):
    """Two chunks through the per-chunk API of a one-stream context, with and without a scoring call between them: same tokens,
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
                nll = eng.transducer_nll(enc_d.data_ptr(), Tb, tg, Ub, 2, 15, None, s)
                assert np.isfinite(nll).all()
        return eng.tokens(s)[0], eng.att_cache(0, s), eng.cnn_cache(0, s), eng.predictor_state(0, s)
    tok_a, att_a, cnn_a, (h_a, c_a, last_a) = run(False)
    tok_b, att_b, cnn_b, (h_b, c_b, last_b) = run(True)
    assert att_a.shape[2] > 0
    assert tok_a == tok_b and last_a == last_b
    assert np.array_equal(_bits(att_a), _bits(att_b)) and np.array_equal(_bits(cnn_a), _bits(cnn_b))
    assert np.array_equal(_bits(h_a), _bits(h_b)) and np.array_equal(_bits(c_a), _bits(c_b))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _raw(eng, fn, enc_ptr, el, tg, tl, B, Tn, Umax, nll, pick=None):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    if fn == "rnnt_transducer_nll":
        return eng.lib.rnnt_transducer_nll(eng.ctx, enc_ptr, p(el), p(tg), p(tl), B, Tn, Umax, p(nll), pick, _stream())
    return eng.lib.rnnt_ctc_nll(eng.ctx, enc_ptr, p(el), p(tg), p(tl), B, Tn, Umax, p(nll), _stream())


@pytest.mark.parametrize("fn", ["rnnt_transducer_nll", "rnnt_ctc_nll"])
def test_refusals(fn, engines, numerics, np_state_dict):
    eng = engines(numerics)
    B, Tn, Umax = 2, 10, 3
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(4)).cuda()
    el, tl = np.array([10, 6], np.int32), np.array([3, 1], np.int32)
    tg = np.array([[7, 0, V - 1], [BLANK + 1, -5, BLANK]], np.int32)       # row 1's entries beyond its length are invalid on purpose
    nll = np.zeros(B, np.float64)
    ep = enc_d.data_ptr()

    def valid():
        out = np.full(B, np.nan)
        assert _raw(eng, fn, ep, el, tg, tl, B, Tn, Umax, out) == 0, eng.lib.rnnt_last_error(eng.ctx)
        return out
    base = valid()
    assert np.isfinite(base).all()

    def refused(code, **kw):
        a = dict(enc_ptr=ep, el=el, tg=tg, tl=tl, B=B, Tn=Tn, Umax=Umax, nll=nll)
        a.update(kw)
        rc = _raw(eng, fn, a["enc_ptr"], a["el"], a["tg"], a["tl"], a["B"], a["Tn"], a["Umax"], a["nll"])
        assert rc == code, (kw.keys(), rc, eng.lib.rnnt_last_error(eng.ctx))
        assert eng.lib.rnnt_last_error(eng.ctx) != b""
        assert np.array_equal(_bits(valid()), _bits(base))         # a following valid call is unaffected
    A, S, ST = rlib.ERR_ARG, rlib.ERR_SHAPE, rlib.ERR_STATE
    for k in ("enc_ptr", "el", "tg", "tl", "nll"):                  # null pointers
        refused(A, **{k: None})
    refused(A, B=0)
    refused(A, el=np.array([0, 6], np.int32))                       # T_b outside [1, T]
    refused(A, el=np.array([10, 11], np.int32))
    refused(A, tl=np.array([-1, 1], np.int32))                      # U_b / L_b outside [0, Umax]
    refused(A, tl=np.array([3, 4], np.int32))
    refused(A, tg=np.array([[7, V, 1], [6, 0, 0]], np.int32))       # a label outside [0, V) inside the valid length
    refused(A, tg=np.array([[7, -1, 1], [6, 0, 0]], np.int32))
    refused(A, tg=np.array([[7, BLANK, 1], [6, 0, 0]], np.int32))   # the blank inside the valid length
    big = np.ones((B, 256), np.int32)
    refused(S, tg=big, Umax=256)                                    # Umax > 255
    if fn == "rnnt_transducer_nll":                                 # lattice beyond the scratch: 64 * 128 frames of 256 floats > 12 * 4 * 256 * 128
        Bb = 64
        refused(S, B=Bb, Tn=128, el=np.full(Bb, 128, np.int32), tl=np.zeros(Bb, np.int32), tg=np.ones((Bb, Umax), np.int32),
                nll=np.zeros(Bb, np.float64))
    # weights not finalised
    fresh = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    try:
        assert _raw(fresh, fn, ep, el, tg, tl, B, Tn, Umax, nll) == ST
        assert fresh.lib.rnnt_last_error(fresh.ctx) != b""
        if fn == "rnnt_ctc_nll":                                    # the CTC head is optional: without it the call is a state error
            sd = {k: v for k, v in np_state_dict(0).items() if not k.startswith("ctc_head.")}
            fresh.load_state_dict(sd, numerics=numerics)
            assert _raw(fresh, fn, ep, el, tg, tl, B, Tn, Umax, nll) == ST
            assert b"ctc_head" in fresh.lib.rnnt_last_error(fresh.ctx)
    finally:
        fresh.close()


# ---- 8. CTC -----------------------------------------------------------------------------------------------------------------------------
def test_ctc_nll_vs_torch_float64(engines, numerics):
    """rnnt_ctc_nll against torch's CPU ctc_loss(reduction="none") in float64 over the device's own downloaded log-probabilities:
    adjacent repeated labels, an empty transcript, 255 labels, and one transcript its frames cannot hold (+inf, 0 in the facade)."""
    from ctc_vr_amd.online_rnnt_model import compose_losses
    eng = engines(numerics)
    B, Tn, Umax = 4, 300, 255
    g = np.random.Generator(np.random.Philox(key=[8, 8]))
    long_row = g.integers(0, V - 1, 255)
    long_row = np.where(long_row >= BLANK, long_row + 1, long_row)
    rows = [list(long_row), [], [7, 7, 7, 9, 9, 3], [8, 8, 8, 8, 8]]
    tl = np.array([len(r) for r in rows], np.int32)
    el = np.array([300, 50, 20, 6], np.int32)                    # row 3: five equal labels need 9 frames
    tg = np.full((B, Umax), -1, np.int32)
    for b, r in enumerate(rows):
        tg[b, :len(r)] = r
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(8)).cuda()
    nll = eng.ctc_nll(enc_d.data_ptr(), el, tg, tl, B, Tn, _stream())
    lp_d = torch.empty(B * Tn, V, device="cuda")
    eng.ctc_logprobs(enc_d.data_ptr(), B * Tn, lp_d.data_ptr(), _stream())
    torch.cuda.synchronize()
    lp = lp_d.view(B, Tn, V).cpu().double().transpose(0, 1).contiguous()          # (T, B, V)
    want = torch.nn.functional.ctc_loss(lp, torch.from_numpy(np.maximum(tg, 0)).long(), torch.from_numpy(el).long(), torch.from_numpy(tl).long(),
                                        blank=BLANK, reduction="none").numpy()
    for b in range(B):
        print(f"{numerics} b={b} L={tl[b]} T_b={el[b]} nll={nll[b]!r} torch={want[b]!r}")
    assert np.isposinf(want[3]) and np.isposinf(nll[3])
    for b in range(3):
        assert math.isfinite(want[b]) and abs(nll[b] - want[b]) <= REC_RTOL * abs(want[b]), (b, nll[b], want[b])
    _, d = compose_losses(np.zeros(B), nll, tl, 0.3)
    ref = torch.nn.functional.ctc_loss(lp, torch.from_numpy(np.maximum(tg, 0)).long(), torch.from_numpy(el).long(), torch.from_numpy(tl).long(),
                                       blank=BLANK, reduction="mean", zero_infinity=True)
    assert d["loss_ctc"] == pytest.approx(float(ref), rel=1e-9)
    assert d["loss_ctc"] == float((np.where(np.isfinite(nll), nll, 0.0) / np.maximum(tl, 1)).mean())   # the infinite row contributes 0


# ---- 9. facade ------------------------------------------------------------------------------------------------------------------------
def test_forward_with_texts(numerics, np_state_dict):
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel, compose_losses
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=V, blank_id=BLANK, streaming=False, predictor_dropout=0, ctc_weight=0.3,
                        max_streams=2, max_chunk_frames=128, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=0)
    m.load_state_dict(np_state_dict(0))
    audios = torch.from_numpy(T.synth_fbank(2, 120, seed=41))
    lens = torch.tensor([120, 90])
    texts = torch.tensor([[7, 0, V - 1, 9], [BLANK + 1, 33, -1, -1]])
    text_lens = torch.tensor([4, 2])
    out, loss, d = m.forward(audios, lens, texts, text_lens)
    assert out is None and isinstance(loss, torch.Tensor) and loss.dtype == torch.float64 and loss.dim() == 0
    assert set(d) == {"loss_rnnt", "loss_ctc"}
    nr, nc = m.transducer_nll(audios, lens, texts, text_lens), m.ctc_nll(audios, lens, texts, text_lens)
    assert nr.dtype == torch.float64 and nr.shape == (2,) and torch.isfinite(nr).all() and torch.isfinite(nc).all()
    total, dd = compose_losses(nr.numpy(), nc.numpy(), text_lens.numpy(), 0.3)
    assert float(loss) == total and d == dd
    assert d["loss_rnnt"] == float(nr.mean()) and math.isfinite(float(loss))
    m.ctc_weight = 0.0
    out0, loss0, d0 = m(audios, lens, texts, text_lens)
    assert out0 is None and set(d0) == {"loss_rnnt"} and float(loss0) == d["loss_rnnt"]
    m._engine.close()
