"""Two-pass decoding on the device through the C ABI: the transducer likelihood of an utterance's n-best over frames projected once
(rnnt_transducer_nll_nbest), the per-slot encoder-frame history of the stream pool (rnnt_stream_keep_frames / rnnt_stream_get_frames),
rescoring over it (rnnt_pool_rescore) and the facades.  Needs a real MI355X: `pytest -m gpu`.

The pins are those of test_score.py: the picked lattice is bitwise the lattice rnnt_joint(mode=1) writes over pred [B, N * U1, 256],
the f64 recursion agrees with its float64 restatement to 1e-9 relative, the whole call agrees with the CPU oracle within the
project's logits tolerance, and with rnnt_transducer_nll on frames repeated N times within what the difference of the two picked
lattices allows.  Nothing here provokes a device fault: every refusal is a host-side argument check."""
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
REC_RTOL = 1e-9                   # recursion vs its float64 restatement, as in test_score.py
PARITY_MODES = ["fp32", "bf16x3", "f16x3"]
ALL_MODES = PARITY_MODES + ["bf16"]
V, BLANK = T.VOCAB, T.BLANK
EDGE_LABELS = [0, V - 1, BLANK - 1, BLANK + 1]


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
    """One small one-stream context per numerics mode (scratch: 12 * 4 * 256 * 128 floats), as in test_score.py."""
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


@pytest.fixture(scope="module")
def pools(np_state_dict):
    """Multi-slot contexts per (mode, slots, max_cache_frames), reset by whoever takes one."""
    cache = {}

    def get(mode, slots, frames=64):
        key = (mode, slots, frames)
        if key not in cache:
            eng = RnntEngine(max_streams=slots, max_chunk_frames=64, max_cache_frames=frames, max_enc_frames=16, max_tokens=512, vocab_size=V,
                             blank_id=BLANK, max_beam=0)
            eng.load_state_dict(np_state_dict(0), numerics=mode)
            cache[key] = eng
        cache[key].reset(slots, _stream())
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _hyps(B, N, Umax, nh, lens, seed, pad=-1):
    """hyp_lens [B, N] and hyp_tokens [B, N, Umax] int32: hypothesis (b, n) holds lens[b][n] labels != blank -- the edge labels (0,
    V-1, the blank's neighbours) spread over the rows, then seeded random ones -- and `pad` beyond its length; rows n >= nh[b] hold
    length 0 and `pad` everywhere."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0x5D]))
    hl = np.zeros((B, N), np.int32)
    ht = np.full((B, N, Umax), pad, np.int32)
    k = 0
    for b in range(B):
        for n in range(int(nh[b])):
            hl[b, n] = lens[b][n]
            for u in range(hl[b, n]):
                if (u + b + n) % 3 == 0:
                    ht[b, n, u] = EDGE_LABELS[k % 4]
                    k += 1
                else:
                    y = int(g.integers(0, V - 1))
                    ht[b, n, u] = y + 1 if y >= BLANK else y
    return hl, ht


def _nbest(eng, enc_d, Tb, nh, hl, ht, want_pick=True):
    B, Tn = enc_d.size(0), enc_d.size(1)
    N, U1 = hl.shape[1], ht.shape[2] + 1
    pick = torch.full((B, Tn, N * U1, 2), float("nan"), device=enc_d.device) if want_pick else None
    nll = eng.transducer_nll_nbest(enc_d.data_ptr(), Tb, nh, hl, ht, B, Tn, pick.data_ptr() if want_pick else None, _stream())
    torch.cuda.synchronize()
    return nll, (pick.cpu().numpy().reshape(B, Tn, N, U1, 2) if want_pick else None)


def _valid_masks(B, Tn, N, U1, Tb, nh, hl):
    """[B, T, N, U1]: blank values are valid at n < n_hyp, t < T_b, u <= U_bn; label values at u < U_bn"""
    t = np.arange(Tn)[None, :, None, None]
    n = np.arange(N)[None, None, :, None]
    u = np.arange(U1)[None, None, None, :]
    tb, nb, ub = np.asarray(Tb)[:, None, None, None], np.asarray(nh)[:, None, None, None], np.asarray(hl)[:, None, :, None]
    live = (t < tb) & (n < nb)
    return live & (u <= ub), live & (u < ub)


# the (3, 21, 4, 7) case of the issue: n_hyp = [4, 1, 3], an empty hypothesis at n = 2
CASE_B = dict(B=3, Tn=21, N=4, U1=7, Tb=[21, 13, 8], nh=[4, 1, 3], lens=[[6, 3, 0, 5], [4, 0, 0, 0], [2, 6, 0, 0]])
PICK_CASES = {
    "single_cell": dict(B=1, Tn=1, N=1, U1=1, Tb=[1], nh=[1], lens=[[0]]),
    "ragged_3_21_4_7": CASE_B,
    "n16": dict(B=2, Tn=37, N=16, U1=5, Tb=[37, 20], nh=[16, 9], lens=[[(3 * n) % 5 for n in range(16)], [(n + 1) % 5 for n in range(16)]]),
}


def _case(c, seed):
    Tb, nh = np.array(c["Tb"], np.int32), np.array(c["nh"], np.int32)
    hl, ht = _hyps(c["B"], c["N"], c["U1"] - 1, nh, c["lens"], seed)
    enc = torch.randn(c["B"], c["Tn"], 256, generator=torch.Generator().manual_seed(seed))
    return Tb, nh, hl, ht, enc


def _pred_rows(eng, nh, hl, ht, dev):
    """The predictor over [blank, y_1 .. y_Umax] from the zero state through rnnt_predictor_step at B * N rows: pred [B, N * U1, 256]."""
    B, N, Umax = ht.shape
    R = B * N
    h, c = torch.zeros(R, 256, device=dev), torch.zeros(R, 256, device=dev)
    pred = torch.empty(R, Umax + 1, 256, device=dev)
    for u in range(Umax + 1):
        tok = np.array([ht[b, n, u - 1] if n < nh[b] and 1 <= u <= hl[b, n] else BLANK for b in range(B) for n in range(N)], np.int32)
        tok_d = torch.from_numpy(tok).to(dev)
        out, h2, c2 = torch.empty(R, 256, device=dev), torch.empty(R, 256, device=dev), torch.empty(R, 256, device=dev)
        eng.predictor_step(tok_d.data_ptr(), h.data_ptr(), c.data_ptr(), R, out.data_ptr(), h2.data_ptr(), c2.data_ptr(), _stream())
        pred[:, u] = out
        h, c = h2, c2
    return pred.view(B, N * (Umax + 1), 256)


# ---- 1. pick = lattice, bitwise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PICK_CASES))
def test_pick_is_the_lattice_bitwise(name, engines, any_numerics):
    c = PICK_CASES[name]
    B, Tn, N, U1 = c["B"], c["Tn"], c["N"], c["U1"]
    eng = engines(any_numerics)
    dev = torch.device("cuda", 0)
    Tb, nh, hl, ht, enc = _case(c, seed=200 + Tn)
    enc_d = enc.to(dev)
    nll, pick = _nbest(eng, enc_d, Tb, nh, hl, ht)
    pred = _pred_rows(eng, nh, hl, ht, dev).contiguous()
    lat = torch.full((B, Tn, N * U1, V), float("nan"), device=dev)
    eng.joint(enc_d.data_ptr(), pred.data_ptr(), B, Tn, N * U1, 1, lat.data_ptr(), _stream())
    torch.cuda.synchronize()
    col = np.full((B, N, U1), BLANK, np.int64)
    for b in range(B):
        for n in range(nh[b]):
            col[b, n, :hl[b, n]] = ht[b, n, :hl[b, n]]
    idx = torch.from_numpy(col.reshape(B, N * U1)).to(dev)[:, None, :, None].expand(B, Tn, N * U1, 1)
    want_blank = lat[..., BLANK].cpu().numpy().reshape(B, Tn, N, U1)
    want_label = lat.gather(3, idx)[..., 0].cpu().numpy().reshape(B, Tn, N, U1)
    vb, vl = _valid_masks(B, Tn, N, U1, Tb, nh, hl)
    assert np.isfinite(pick[..., 0][vb]).all() and np.isfinite(pick[..., 1][vl]).all()
    assert np.array_equal(_bits(pick[..., 0])[vb], _bits(want_blank)[vb])
    assert np.array_equal(_bits(pick[..., 1])[vl], _bits(want_label)[vl])
    for b in range(B):
        assert np.isfinite(nll[b, :nh[b]]).all() and (_bits(nll[b, nh[b]:]) == 0).all()


# ---- 2. recursion ---------------------------------------------------------------------------------------------------------------------
REC_CASES = {
    # name: (T, Umax, N, T_b, n_hyp, lens): the full-length hypotheses sit at n = 1 and n = N - 1
    "u1_64": (12, 63, 3, [12, 1, 7], [3, 3, 2], [[30, 63, 63], [0, 63, 63], [5, 63, 0]]),     # one full wavefront; T_b = 1 and U_b = 0 rows
    "u1_65": (9, 64, 3, [9, 5], [3, 3], [[1, 64, 64], [64, 33, 64]]),                         # across a wavefront of 64 lanes
    "umax_255": (6, 255, 2, [6], [2], [[100, 255]]),
    "ragged": (23, 9, 4, [23, 1, 17, 9], [4, 2, 3, 1], [[9, 0, 4, 9], [0, 9, 0, 0], [1, 9, 3, 0], [0, 0, 0, 0]]),
    "single_cell": (1, 0, 2, [1], [2], [[0, 0]]),
}


@pytest.mark.parametrize("case", sorted(REC_CASES))
def test_recursion_matches_float64_dp(case, engines, any_numerics):
    Tn, Umax, N, Tb, nh, lens = REC_CASES[case]
    B, U1 = len(Tb), Umax + 1
    eng = engines(any_numerics)
    Tb, nh = np.array(Tb, np.int32), np.array(nh, np.int32)
    hl, ht = _hyps(B, N, Umax, nh, lens, seed=7 + Umax)
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(2000 + Umax)).cuda()
    nll, pick = _nbest(eng, enc_d, Tb, nh, hl, ht)
    flat = pick.reshape(B, Tn, N * U1, 2)
    for b in range(B):
        for n in range(N):
            if n >= nh[b]:
                assert _bits(nll[b, n:n + 1])[0] == 0, (case, b, n, nll[b, n])      # exactly +0.0
                continue
            want = T.transducer_nll_ref(T.nbest_pick_slice(flat[b], n, U1), int(Tb[b]), int(hl[b, n]))
            print(f"{case} b={b} n={n} T_b={Tb[b]} U={hl[b, n]} nll={nll[b, n]!r} dp={want!r} rel={abs(nll[b, n] - want) / abs(want):.3e}")
            assert math.isfinite(want)
            assert abs(nll[b, n] - want) <= REC_RTOL * abs(want), (case, b, n, nll[b, n], want)


# ---- 3. end to end against the oracle --------------------------------------------------------------------------------------------------
def test_end_to_end_vs_oracle(engines, numerics, np_state_dict):
    """As test_score.test_end_to_end_vs_oracle, with the oracle's predictor over the B * N hypothesis rows and its joint over
    pred [B, N * U1, 256]: delta = max |pick - oracle| <= 2 LOGIT_TOL, |nll - oracle| <= (T_b + U_b) delta + 1e-9 |nll|."""
    from oracle import rnnt_oracle as O
    c = CASE_B
    B, Tn, N, U1 = c["B"], c["Tn"], c["N"], c["U1"]
    eng = engines(numerics)
    Tb, nh, hl, ht, enc = _case(c, seed=31)
    nll, pick = _nbest(eng, enc.cuda(), Tb, nh, hl, ht)
    sd = O.to_torch_sd(np_state_dict(0))
    state = O.predictor_init_state(B * N)
    outs = []
    for u in range(U1):
        tok = torch.tensor([[int(ht[b, n, u - 1]) if n < nh[b] and 1 <= u <= hl[b, n] else BLANK] for b in range(B) for n in range(N)], dtype=torch.long)
        out, state = O.predictor_step(sd, tok, state)
        outs.append(out)
    pred = torch.cat(outs, 1).reshape(B, N * U1, 256)
    lp = torch.log_softmax(O.joint(sd, enc, pred), dim=-1).numpy().reshape(B, Tn, N, U1, V)
    vb, vl = _valid_masks(B, Tn, N, U1, Tb, nh, hl)
    want_pick = np.zeros((B, Tn, N, U1, 2), np.float32)
    want_pick[..., 0] = lp[..., BLANK]
    for b in range(B):
        for n in range(nh[b]):
            for u in range(hl[b, n]):
                want_pick[b, :, n, u, 1] = lp[b, :, n, u, ht[b, n, u]]
    d = np.abs(pick.astype(np.float64) - want_pick.astype(np.float64))
    delta = max(float(d[..., 0][vb].max()), float(d[..., 1][vl].max()))
    print(f"{numerics}: delta = {delta:.3e}")
    assert delta <= 2 * LOGIT_TOL
    for b in range(B):
        for n in range(nh[b]):
            want = T.transducer_nll_ref(want_pick[b, :, n], int(Tb[b]), int(hl[b, n]))
            bound = (int(Tb[b]) + int(hl[b, n])) * delta + 1e-9 * abs(nll[b, n])
            print(f"{numerics} b={b} n={n}: nll={nll[b, n]!r} oracle={want!r} diff={abs(nll[b, n] - want):.3e} bound={bound:.3e}")
            assert abs(nll[b, n] - want) <= bound


# ---- 4. against repeated frames ----------------------------------------------------------------------------------------------------------
def _repeated(eng, enc_d, Tb, nh, hl, ht, want_pick=True):
    """The parent's way: rnnt_transducer_nll over B * N rows, every utterance's frames repeated N times (missing hypotheses: empty)."""
    B, Tn = enc_d.size(0), enc_d.size(1)
    N, Umax = hl.shape[1], ht.shape[2]
    rep = enc_d[:, None].expand(B, N, Tn, 256).reshape(B * N, Tn, 256).contiguous()
    tl = np.where(np.arange(N)[None, :] < np.asarray(nh)[:, None], hl, 0).astype(np.int32).reshape(B * N)
    pick = torch.full((B * N, Tn, Umax + 1, 2), float("nan"), device=enc_d.device) if want_pick else None
    nll = eng.transducer_nll(rep.data_ptr(), np.repeat(Tb, N), ht.reshape(B * N, Umax), tl, B * N, Tn, pick.data_ptr() if want_pick else None, _stream())
    torch.cuda.synchronize()
    return nll.reshape(B, N), (pick.cpu().numpy().reshape(B, N, Tn, Umax + 1, 2).transpose(0, 2, 1, 3, 4) if want_pick else None)


def test_against_repeated_frames(engines, numerics):
    """Not bitwise: launch_gemm chooses the projection kernel by its row count.  Every alignment is a sum of T_b + U_b cell terms,
    so with delta = max |pick - pick_repeated| over the valid cells, |nll - nll_repeated| <= (T_b + U_b) delta."""
    c = CASE_B
    B, Tn, N, U1 = c["B"], c["Tn"], c["N"], c["U1"]
    eng = engines(numerics)
    Tb, nh, hl, ht, enc = _case(c, seed=41)
    nll, pick = _nbest(eng, enc.cuda(), Tb, nh, hl, ht)
    nll_r, pick_r = _repeated(eng, enc.cuda(), Tb, nh, hl, ht)
    vb, vl = _valid_masks(B, Tn, N, U1, Tb, nh, hl)
    d = np.abs(pick.astype(np.float64) - pick_r.astype(np.float64))
    delta = max(float(d[..., 0][vb].max()), float(d[..., 1][vl].max()))
    print(f"{numerics}: delta between the two picks = {delta:.3e}")
    for b in range(B):
        for n in range(nh[b]):
            bound = (int(Tb[b]) + int(hl[b, n])) * delta
            print(f"{numerics} b={b} n={n}: nbest={nll[b, n]!r} repeated={nll_r[b, n]!r} diff={abs(nll[b, n] - nll_r[b, n]):.3e} bound={bound:.3e}")
            assert abs(nll[b, n] - nll_r[b, n]) <= bound


# ---- 5. capacity -----------------------------------------------------------------------------------------------------------------------------
def test_capacity_beyond_repeated_frames(engines, numerics):
    """8 utterances x 8 hypotheses x 128 frames: repeated, 64 * 128 frames of 256 floats exceed the context scratch (12 * 4 * 256 * 128
    floats) and rnnt_transducer_nll refuses; side by side the call needs 8 * 128 + 8 * 8 * 4 rows and runs."""
    B, Tn, N, Umax = 8, 128, 8, 3
    eng = engines(numerics)
    Tb, nh = np.full(B, Tn, np.int32), np.full(B, N, np.int32)
    hl, ht = _hyps(B, N, Umax, nh, [[(b + n) % (Umax + 1) for n in range(N)] for b in range(B)], seed=51)
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(51)).cuda()
    with pytest.raises(RnntError) as e:
        eng.transducer_nll(enc_d.data_ptr(), np.repeat(Tb, N), np.maximum(ht, 0).reshape(B * N, Umax), hl.reshape(B * N), B * N, Tn, None, _stream())
    assert e.value.status == rlib.ERR_SHAPE and "scratch" in str(e.value)
    nll, _ = _nbest(eng, enc_d, Tb, nh, hl, ht, want_pick=False)
    assert nll.shape == (B, N) and np.isfinite(nll).all() and (nll > 0).all()


# ---- 6. padding is never read; determinism and placement ------------------------------------------------------------------------------------
def test_padding_is_never_read(engines, numerics):
    c = CASE_B
    B, Tn, N, U1 = c["B"], c["Tn"], c["N"], c["U1"]
    eng = engines(numerics)
    Tb, nh, hl, _, enc = _case(c, seed=5)
    _, clean_t = _hyps(B, N, U1 - 1, nh, c["lens"], seed=5, pad=3)          # a valid label in the padding
    _, dirty_t = _hyps(B, N, U1 - 1, nh, c["lens"], seed=5, pad=-1)
    dirty_l = hl.copy()
    dirty = enc.clone()
    for b in range(B):
        dirty[b, Tb[b]:] = float("nan")
        for n in range(N):
            if n >= nh[b]:                                               # garbage rows: lengths and tokens the checks would refuse
                dirty_l[b, n] = [1000, -7][n % 2]
                dirty_t[b, n] = [V + 5, BLANK, -3][n % 3]
            else:
                dirty_t[b, n, hl[b, n]:] = [V, -1, BLANK][(b + n) % 3]
    nll_clean, _ = _nbest(eng, enc.cuda(), Tb, nh, hl, clean_t, want_pick=False)
    nll_dirty, _ = _nbest(eng, dirty.cuda(), Tb, nh, dirty_l, dirty_t, want_pick=False)
    assert np.isfinite(nll_dirty).all()
    assert np.array_equal(_bits(nll_dirty), _bits(nll_clean))
    nll_again, _ = _nbest(eng, dirty.cuda(), Tb, nh, dirty_l, dirty_t, want_pick=False)
    assert np.array_equal(_bits(nll_again), _bits(nll_dirty))             # deterministic
    perm = np.array([2, 0, 1])
    nll_p, _ = _nbest(eng, enc[torch.from_numpy(perm)].contiguous().cuda(), Tb[perm], nh[perm], hl[perm], clean_t[perm], want_pick=False)
    assert np.array_equal(_bits(nll_p), _bits(nll_clean[perm]))           # placement


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def _raw(eng, enc_ptr, el, nh, hl, ht, B, Tn, N, Umax, nll):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    return eng.lib.rnnt_transducer_nll_nbest(eng.ctx, enc_ptr, p(el), p(nh), p(hl), p(ht), B, Tn, N, Umax, p(nll), None, _stream())


def test_refusals(engines, numerics):
    eng = engines(numerics)
    B, Tn, N, Umax = 2, 10, 3, 3
    enc_d = torch.randn(B, Tn, 256, generator=torch.Generator().manual_seed(4)).cuda()
    el, nh = np.array([10, 6], np.int32), np.array([3, 2], np.int32)
    hl = np.array([[3, 0, 2], [1, 3, 99]], np.int32)                        # (1, 2) is beyond n_hyp: never looked at
    ht = np.array([[[7, 0, V - 1], [-5, BLANK, V], [BLANK + 1, 9, -1]], [[4, -5, BLANK], [1, 2, 3], [V, V, V]]], np.int32)
    nll = np.zeros((B, N), np.float64)
    ep = enc_d.data_ptr()

    def valid():
        out = np.full((B, N), np.nan)
        assert _raw(eng, ep, el, nh, hl, ht, B, Tn, N, Umax, out) == 0, eng.lib.rnnt_last_error(eng.ctx)
        return out
    base = valid()
    assert np.isfinite(base).all() and base[1, 2] == 0.0

    def refused(code, **kw):
        a = dict(enc_ptr=ep, el=el, nh=nh, hl=hl, ht=ht, B=B, Tn=Tn, N=N, Umax=Umax, nll=nll)
        a.update(kw)
        rc = _raw(eng, a["enc_ptr"], a["el"], a["nh"], a["hl"], a["ht"], a["B"], a["Tn"], a["N"], a["Umax"], a["nll"])
        assert rc == code, (list(kw), rc, eng.lib.rnnt_last_error(eng.ctx))
        assert eng.lib.rnnt_last_error(eng.ctx) != b""
        assert np.array_equal(_bits(valid()), _bits(base))         # a following valid call is unaffected
    A, S, ST = rlib.ERR_ARG, rlib.ERR_SHAPE, rlib.ERR_STATE
    for k in ("enc_ptr", "el", "nh", "hl", "ht", "nll"):            # null pointers
        refused(A, **{k: None})
    refused(A, B=0)
    refused(A, N=0)                                                 # N outside [1, 16]
    big_n = 17
    refused(A, N=big_n, hl=np.zeros((B, big_n), np.int32), ht=np.ones((B, big_n, Umax), np.int32), nll=np.zeros((B, big_n), np.float64))
    refused(A, nh=np.array([0, 2], np.int32))                       # n_hyp outside [1, N]
    refused(A, nh=np.array([3, 4], np.int32))
    refused(A, el=np.array([0, 6], np.int32))                       # T_b outside [1, T]
    refused(A, el=np.array([10, 11], np.int32))
    refused(A, hl=np.array([[3, -1, 2], [1, 3, 0]], np.int32))      # a length outside [0, Umax]
    refused(A, hl=np.array([[3, 0, 2], [1, 4, 0]], np.int32))
    bad = ht.copy(); bad[0, 0, 1] = V                               # noqa: E702  a label outside [0, V) inside a length
    refused(A, ht=bad)
    bad = ht.copy(); bad[1, 1, 2] = -1                              # noqa: E702
    refused(A, ht=bad)
    bad = ht.copy(); bad[0, 2, 0] = BLANK                           # noqa: E702  the blank inside a length
    refused(A, ht=bad)
    refused(S, Umax=256, ht=np.ones((B, N, 256), np.int32))         # Umax > 255
    Bb = 64                                                         # 64 * 128 frames of 256 floats > 12 * 4 * 256 * 128
    refused(S, B=Bb, Tn=128, el=np.full(Bb, 128, np.int32), nh=np.ones(Bb, np.int32), hl=np.zeros((Bb, N), np.int32),
            ht=np.ones((Bb, N, Umax), np.int32), nll=np.zeros((Bb, N), np.float64))
    refused(S, B=1, Tn=1 << 20, N=16, Umax=255, el=np.array([1 << 20], np.int32), nh=np.array([1], np.int32),   # 2^32 lattice cells
            hl=np.zeros((1, 16), np.int32), ht=np.ones((1, 16, 255), np.int32), nll=np.zeros((1, 16), np.float64))
    fresh = RnntEngine(max_streams=1, max_chunk_frames=64, max_cache_frames=64, max_enc_frames=16, max_tokens=64, vocab_size=V, blank_id=BLANK)
    try:                                                            # weights not finalised
        assert _raw(fresh, ep, el, nh, hl, ht, B, Tn, N, Umax, nll) == ST
        assert fresh.lib.rnnt_last_error(fresh.ctx) != b""
    finally:
        fresh.close()


# ---- 8. history ----------------------------------------------------------------------------------------------------------------------------
CHUNK = 32                        # fbank frames per chunk: 7 encoder frames


def _fb(slots, n_chunks, seed):
    return torch.from_numpy(T.synth_fbank(slots, CHUNK * n_chunks, seed=seed)).cuda()


def _snapshot(eng, slot):
    s = _stream()
    h, c, tok = eng.predictor_state(slot, s)
    return {"att": eng.att_cache(slot, s), "cnn": eng.cnn_cache(slot, s), "h": h, "c": c, "tok": np.int32(tok),
            "tokens": np.asarray(eng.stream_tokens(slot, 0, s), np.int32)}


def _same(a, b):
    return all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def _encode_chunks(eng, x, plan, offs, required=None):
    """plan: per chunk index the slots listed (in that order) -> {slot: [frames [t', 256] per chunk]} through
    rnnt_pool_chunk(greedy = 0) + rnnt_get_enc_frames + rnnt_frames_discard"""
    s = _stream()
    out = {}
    for ci, slots in enumerate(plan):
        rows = torch.stack([x[sl, ci * CHUNK:(ci + 1) * CHUNK] for sl in slots], 0).contiguous()
        o = [offs[sl] for sl in slots]
        tq = eng.pool_chunk(slots, rows.data_ptr(), CHUNK, o, o if required is None else [required] * len(slots), False, s)
        fr = eng.enc_frames(s)
        for sl in slots:
            out.setdefault(sl, []).append(fr[sl, :tq].copy())
            offs[sl] += tq
        eng.frames_discard(s)
    return out


def _state_error(fn, *a):
    with pytest.raises(RnntError) as e:
        fn(*a)
    return e.value.status


def test_history(numerics, np_state_dict):
    s = _stream()
    start = rlib.live_device_bytes()

    def make(frames=64):
        eng = RnntEngine(max_streams=4, max_chunk_frames=64, max_cache_frames=frames, max_enc_frames=16, max_tokens=512, vocab_size=V, blank_id=BLANK,
                         max_beam=0)
        eng.load_state_dict(np_state_dict(0), numerics=numerics)
        eng.reset(4, s)
        return eng
    a, b = make(), make()
    try:
        x = _fb(4, 4, seed=81)
        for eng in (a, b):
            for slot in range(4):
                eng.stream_open(slot, s)
        before_keep = rlib.live_device_bytes()
        a.stream_keep_frames(1, True, s)
        a.stream_keep_frames(3, True, s)
        assert rlib.live_device_bytes() >= before_keep + 2 * 64 * 256 * 4          # two histories [max_cache_frames][256] f32
        assert a.stream_frames_len(1) == 0 and a.stream_frames(3).shape == (0, 256)
        plan = [[0, 1, 2, 3], [3, 1, 0, 2], [3, 0, 1]]                             # the third chunk: permuted, slot 2 sits out
        offs_a, offs_b = {k: 0 for k in range(4)}, {k: 0 for k in range(4)}
        got = _encode_chunks(a, x, plan, offs_a)
        _encode_chunks(b, x, plan, offs_b)
        for slot in (1, 3):
            want = np.concatenate(got[slot], 0)
            hist = a.stream_frames(slot).cpu().numpy()
            assert hist.shape == want.shape == (21, 256)
            assert np.array_equal(_bits(hist), _bits(want)), slot
            assert np.array_equal(_bits(a.stream_frames(slot, 7).cpu().numpy()), _bits(want[7:]))
        for slot in (0, 2):
            assert _state_error(a.stream_frames_len, slot) == rlib.ERR_STATE
            assert _state_error(a.stream_keep_frames, slot, True, s) == rlib.ERR_STATE     # keep after a chunk
        # one greedy chunk on top: tokens and caches of every slot are those of the pool where nobody keeps frames
        for eng, offs in ((a, offs_a), (b, offs_b)):
            rows = x[:, 3 * CHUNK:4 * CHUNK].contiguous()
            o = [offs[k] for k in range(4)]
            eng.pool_chunk([0, 1, 2, 3], rows.data_ptr(), CHUNK, o, o, True, s)
        for slot in range(4):
            sa, sb = _snapshot(a, slot), _snapshot(b, slot)
            assert sa["att"].shape[2] > 0 and _same(sa, sb), slot
        assert a.stream_frames_len(1) == 28
        assert np.array_equal(_bits(a.stream_frames(1).cpu().numpy()[:21]), _bits(np.concatenate(got[1], 0)))
        # rnnt_stream_open: the length is 0 and the flag is cleared; the buffer stays for the slot's next utterance
        a.stream_open(1, s)
        assert _state_error(a.stream_frames_len, 1) == rlib.ERR_STATE
        held = rlib.live_device_bytes()
        a.stream_keep_frames(1, True, s)
        assert rlib.live_device_bytes() == held and a.stream_frames_len(1) == 0
        a.reset(4, s)                                                              # rnnt_streams_reset clears every flag
        assert _state_error(a.stream_frames_len, 3) == rlib.ERR_STATE

        # the same through rnnt_pool_chunk_ctc_prefix, against the twin run with greedy = 0
        b.reset(4, s)
        for eng in (a, b):
            for slot in range(3):
                eng.stream_open(slot, s)
        a.stream_keep_frames(0, True, s)
        a.stream_keep_frames(2, True, s)
        plan = [[0, 1, 2], [2, 0], [0, 2, 1]]
        offs = {k: 0 for k in range(3)}
        for ci, slots in enumerate(plan):
            rows = torch.stack([x[sl, ci * CHUNK:(ci + 1) * CHUNK] for sl in slots], 0).contiguous()
            o = [offs[sl] for sl in slots]
            tq = a.pool_chunk_ctc_prefix(slots, rows.data_ptr(), CHUNK, o, o, 4, False, s)
            for sl in slots:
                offs[sl] += tq
        want = _encode_chunks(b, x, plan, {k: 0 for k in range(3)})
        for slot in (0, 2):
            assert np.array_equal(_bits(a.stream_frames(slot).cpu().numpy()), _bits(np.concatenate(want[slot], 0))), slot
        assert _state_error(a.stream_frames_len, 1) == rlib.ERR_STATE
    finally:
        a.close()
        b.close()
    # a chunk that would pass max_cache_frames: refused, and no slot moves (no left context, so the K/V cache never fills)
    e = make(frames=16)
    try:
        x = _fb(2, 3, seed=82)
        e.stream_open(0, s)
        e.stream_open(1, s)
        e.stream_keep_frames(0, True, s)
        offs = {0: 0, 1: 0}
        _encode_chunks(e, x, [[0, 1], [0, 1]], offs, required=0)
        assert e.stream_frames_len(0) == 14
        snap = [_snapshot(e, 0), _snapshot(e, 1)]
        rows = x[:, 2 * CHUNK:3 * CHUNK].contiguous()
        with pytest.raises(RnntError) as err:
            e.pool_chunk([0, 1], rows.data_ptr(), CHUNK, [14, 14], [0, 0], False, s)
        assert err.value.status == rlib.ERR_SHAPE and "max_cache_frames" in str(err.value)
        assert e.stream_frames_len(0) == 14 and _same(snap[0], _snapshot(e, 0)) and _same(snap[1], _snapshot(e, 1))
        one = rows[1:2].contiguous()
        assert e.pool_chunk([1], one.data_ptr(), CHUNK, [14], [0], False, s) == 7   # the slot that keeps nothing goes on from where it was
        e.frames_discard(s)
    finally:
        e.close()
    assert rlib.live_device_bytes() == start


# ---- 9. pool rescoring -----------------------------------------------------------------------------------------------------------------------
def test_pool_rescore(numerics, pools):
    eng = pools(numerics, 3)
    s = _stream()
    x = _fb(3, 4, seed=91)
    n_chunks = {0: 3, 1: 2, 2: 1}                                               # slot 2 is mid-utterance

    def run(with_rescore):
        eng.reset(3, s)
        offs = {k: 0 for k in range(3)}

        def chunk(ci, slots):
            rows = torch.stack([x[sl, ci * CHUNK:(ci + 1) * CHUNK] for sl in slots], 0).contiguous()
            o = [offs[sl] for sl in slots]
            tq = eng.pool_chunk_ctc_prefix(slots, rows.data_ptr(), CHUNK, o, o, 4, False, s)
            for sl in slots:
                offs[sl] += tq
        for slot in range(3):
            eng.stream_open(slot, s)
            eng.stream_keep_frames(slot, True, s)
        for ci in range(3):
            chunk(ci, [sl for sl in range(3) if ci < n_chunks[sl]])
        res = None
        if with_rescore:
            order = [2, 0, 1]
            first = [eng.stream_ctc_prefix(slot, True, stream=s) for slot in order]
            nh, hl, ht = rlib.pack_nbest([[tok for tok, _, _, _ in row] for row in first])
            assert (nh >= 1).all() and hl.max() >= 1
            nll = eng.pool_rescore(order, nh, hl, ht, s)
            lens = np.array([eng.stream_frames_len(slot) for slot in order], np.int32)
            assert lens.tolist() == [7, 21, 14]
            dense = torch.zeros(3, int(lens.max()), 256, device="cuda")
            for i, slot in enumerate(order):
                dense[i, :lens[i]] = eng.stream_frames(slot)
            want = eng.transducer_nll_nbest(dense.data_ptr(), lens, nh, hl, ht, 3, dense.size(1), None, s)
            res = (nll, want, nh)
        chunk(n_chunks[2], [2])                                                 # the searches go on
        chunk(3, [0, 1])
        after = [eng.stream_ctc_prefix(slot, True, True, stream=s)[1] for slot in range(3)]
        return res, after
    (nll, want, nh), after = run(True)
    for i in range(3):
        assert np.isfinite(nll[i, :nh[i]]).all() and (nll[i, nh[i]:] == 0).all()
    assert np.array_equal(_bits(nll), _bits(want))
    _, twin = run(False)
    for slot in range(3):
        for k, (p, q) in enumerate(zip(after[slot], twin[slot])):
            assert p.shape == q.shape and p.tobytes() == q.tobytes(), (slot, k)
    with pytest.raises(RnntError) as e:                                         # a slot that keeps none
        eng.stream_open(1, s)
        eng.pool_rescore([0, 1], np.ones(2, np.int32), np.zeros((2, 1), np.int32), np.zeros((2, 1, 1), np.int32), s)
    assert e.value.status == rlib.ERR_STATE
    with pytest.raises(RnntError) as e:                                         # a duplicated slot
        eng.pool_rescore([0, 0], np.ones(2, np.int32), np.zeros((2, 1), np.int32), np.zeros((2, 1, 1), np.int32), s)
    assert e.value.status == rlib.ERR_ARG


# ---- 10. facade ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", ["ctc", "transducer"])
def test_rescoring_facade(search, numerics, np_state_dict):
    """transducer_attention_rescoring (B = 1) is rescoring_batch's answer for that utterance alone, bit for bit; inside a batch of two
    the same hypotheses come back, each td_score within (T_b + U_b) delta of the lone one's (delta: between the two picked lattices,
    as in test_against_repeated_frames) and each total within the weighted sum of the two passes' differences."""
    from ctc_vr_amd.online_rnnt_model import OnlineRNNTModel
    m = OnlineRNNTModel(input_dim=80, hidden_dim=256, vocab_size=V, blank_id=BLANK, streaming=False, predictor_dropout=0, ctc_weight=0.3,
                        max_streams=2, max_chunk_frames=128, max_cache_frames=64, max_enc_frames=64, max_tokens=256, max_beam=0)
    try:
        m.load_state_dict(np_state_dict(0))
        audios = torch.from_numpy(T.synth_fbank(2, 120, seed=41))
        lens = torch.tensor([120, 90])
        cw, tw, kw = 0.3, 0.7, dict(search_ctc_weight=0.3, search_transducer_weight=0.7)
        tokens, score = m.transducer_attention_rescoring(audios[:1], lens[:1], 4, ctc_weight=cw, transducer_weight=tw, beam_search_type=search, **kw)
        best1, rows1 = m.rescoring_batch(audios[:1], lens[:1], 4, cw, tw, search, **kw)[0]
        assert tokens == rows1[best1][0] and score == rows1[best1][3] and math.isfinite(score)
        both = m.rescoring_batch(audios, lens, 4, cw, tw, search, **kw)
        assert len(both) == 2
        best2, rows2 = both[0]
        assert [r[0] for r in rows2] == [r[0] for r in rows1] and 1 <= len(rows1) <= 4
        hyps = [r[0] for r in rows1]
        nh, hl, ht = rlib.pack_nbest([hyps])
        picks = []
        for a, n in ((audios[:1], lens[:1]), (audios, lens)):
            enc, enc_lens, _, _ = m._encode_for_scoring(a, n, torch.zeros(a.size(0), 0), torch.zeros(a.size(0)))
            pick = torch.full((1, enc.size(1), hl.shape[1] * (ht.shape[2] + 1), 2), float("nan"), device=enc.device)
            m._engine.transducer_nll_nbest(enc[:1].contiguous().data_ptr(), enc_lens[:1], nh, hl, ht, 1, enc.size(1), pick.data_ptr(), _stream())
            torch.cuda.synchronize()
            picks.append((pick.cpu().numpy().reshape(1, enc.size(1), hl.shape[1], ht.shape[2] + 1, 2), int(enc_lens[0])))
        (p1, t1), (p2, t2) = picks
        assert t1 == t2
        vb, vl = _valid_masks(1, p1.shape[1], hl.shape[1], ht.shape[2] + 1, [t1], nh, hl)
        d = np.abs(p1.astype(np.float64) - p2.astype(np.float64))
        delta = max(float(d[..., 0][vb].max()), float(d[..., 1][vl].max()) if vl.any() else 0.0)
        print(f"{numerics} {search}: delta between the lone and the batched pick = {delta:.3e}")
        for r1, r2 in zip(rows1, rows2):
            bound = (t1 + len(r1[0])) * delta
            print(f"  {r1[0]}: td {r1[2]!r} vs {r2[2]!r} (bound {bound:.3e}), first {r1[1]!r} vs {r2[1]!r}, total {r1[3]!r} vs {r2[3]!r}")
            assert abs(r1[2] - r2[2]) <= bound
            assert abs(r1[3] - r2[3]) <= cw * abs(r1[1] - r2[1]) + tw * bound + 1e-12 * abs(r1[3])
        if all(abs(r[3] - rows1[best1][3]) > 1e-6 for i, r in enumerate(rows1) if i != best1):
            assert best2 == best1                                     # a clear winner stays the winner inside the batch
    finally:
        m._engine.close()


def test_stream_pool_rescore_and_token_times(numerics, np_state_dict):
    from ctc_vr_amd.online_rnnt_model import StreamPool
    pool = StreamPool(np_state_dict(0), 3, vocab_size=V, blank_id=BLANK, max_cache_frames=64, numerics=numerics)
    try:
        x = _fb(3, 2, seed=95)
        s0, s1 = pool.open(ctc_prefix_beam=4, keep_frames=True), pool.open(ctc_prefix_beam=4, keep_frames=True)
        g = pool.open(keep_frames=True)
        for ci in range(2):
            for slot in (s0, g) if ci else (s0, s1, g):
                pool.feed(slot, x[slot, ci * CHUNK:(ci + 1) * CHUNK].contiguous())
            pool.step()
        assert pool.frames(s0).shape == (14, 256) and pool.frames(s1).shape == (7, 256)
        res = pool.rescore([s1, s0], 0.3, 0.7)
        assert sorted(res) == [s0, s1]
        for slot in (s0, s1):
            best, rows = res[slot]
            assert [r[0] for r in rows] == [tok for tok, _, _ in pool.ctc_hyps(slot, final=True)]
            want_best, want_total = rlib.rescore_select([r[1] for r in rows], [-r[2] for r in rows], 0.3, 0.7)
            assert best == want_best and np.array_equal(_bits(np.array([r[3] for r in rows])), _bits(want_total))
            assert all(math.isfinite(r[2]) and r[2] < 0 for r in rows)
        with pytest.raises(RnntError):
            pool.rescore([g], 0.3, 0.7)                                # not a CTC prefix slot
        tokens = pool.engine.stream_tokens(g, 0, _stream())
        times = pool.token_times(g)
        print(f"{numerics}: {len(tokens)} tokens, times {times}")
        assert len(tokens) >= 1 and len(times) == len(tokens)
        assert all(a <= b for a, b in times)
        assert all(times[i][0] <= times[i + 1][0] and times[i][1] <= times[i + 1][1] for i in range(len(times) - 1))
        assert times[0][0] >= 0 and times[-1][1] <= 14 * 0.04
        with pytest.raises(RnntError):
            pool.token_times(s0)                                       # not a greedy slot
        assert len(pool.close(g)) == len(tokens)
    finally:
        pool.engine.close()
