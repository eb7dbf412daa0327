"""The window plans of test_encoder_window.py without a GPU: the library's position bookkeeping (SlotPos, restated in
window_cases.py) against the float64 oracle's cache lengths and positional windows; what the plans reach (saturated window,
key window beyond row 64, conv ring wrapped twice); three deliberately wrong oracles per case, each of which must move the
encoder frames by at least 10x the GPU tests' tolerance; and the float32 oracle's own distance from the float64 oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import window_cases as W
from oracle import rnnt_oracle as O

ALL_CASES = W.CASES + [W.RAGGED]
SENSITIVITY = 10 * W.LOGIT_TOL


@pytest.fixture(params=ALL_CASES, ids=W.case_id)
def case(request):
    return request.param


def test_case_matrix():
    """every length meets R = t' and R = 2t' + 1; every policy meets t' = 3, 4 and 5; the lengths sit on both sides of the dispatch
    boundaries t' = 4 | 5 and 8 | 9, and 17 is beyond the fused half-blocks' 16 frames"""
    tqs = sorted(W.sub_len(ln) for ln in W.LENGTHS)
    assert tqs == [1, 2, 3, 4, 5, 8, 9, 16, 17]
    for ln in W.LENGTHS:
        assert (ln, "one") in W.CASES and (ln, "two") in W.CASES
        assert W.sub_len(W.max_chunk_frames(ln)) == W.sub_len(ln)
    for p in W.POLICIES:
        assert {3, 4, 5} <= {W.sub_len(ln) for ln, q in W.CASES if q == p}, p
    assert W.sub_len(W.RAGGED[2]) < W.sub_len(W.RAGGED[0])


def test_bookkeeping_matches_oracle(case):
    """SlotPos over the plan: the cache length after every chunk and every chunk's pos_start are the float64 oracle's, and the plan
    reaches what it is meant to: pos_start >= 0 throughout, the ring position passes the ring capacity twice, a truncating policy
    saturates its window and moves the key window beyond row 64, crossing a 32-key unit and a 64-key tile edge on the way."""
    plan = W.case_plan(case)
    ref = W.case_ref(case, 0)
    steps = W.walk(plan)
    total = W.plan_frames(plan)[1]
    assert total + 3 <= 256
    for c, (k, r) in enumerate(zip(steps, ref)):
        assert k["ok"] and k["pos_start"] >= 0
        assert k["pos_start"] == r["pos_start"], c
        assert k["cache_after"] == r["cache_len"] == r["att"].shape[2], c
        assert r["frames"].shape == (k["tq"], 256) and r["cnn"].shape == (12, 1, 256, 30)
    assert steps[-1]["ring_pos"] >= 2 * W.ring_cap(case[0])
    policy, tq = case[1], W.sub_len(case[0])
    rows0 = [k["kv_row0"] for k in steps]
    if policy in W.TRUNCATING:
        r = W.required_of(policy, tq, 0)
        assert steps[-1]["cache_after"] == r and steps[-1]["T2"] == r + steps[-1]["tq"]          # saturated
        assert rows0[-1] > 64
        assert any(a // 32 != b // 32 for a, b in zip(rows0, rows0[1:])) and any(a // 64 != b // 64 for a, b in zip(rows0, rows0[1:]))
        assert len(set(k["cache_after"] for k in steps[-3:])) == 1                               # cache_len stays flat
        if policy == "two" and tq > 1:
            assert r % tq != 0                                                                     # truncation falls inside a chunk
    else:
        assert max(rows0) == 0
        assert steps[-1]["cache_after"] == (0 if policy == "zero" else total - (steps[0]["tq"] if policy == "off" else 0))


# ---- three wrong oracles: module functions of the oracle replaced for one run --------------------------------------------------
def _shifted_keys_attention(sd, p, x, pos_emb, k_cache, v_cache, mask=None):
    """rel_attention reading the key window one row late: key j of the window is buffer row j + 1, the row behind the window is
    the zero row of a fresh buffer; positions and the rows written to the cache are untouched."""
    B, t, D = x.shape
    dk = D // O.HEADS
    q = F.linear(x, sd[p + ".linear_q.weight"], sd[p + ".linear_q.bias"]).view(B, t, O.HEADS, dk)
    k = F.linear(x, sd[p + ".linear_k.weight"], sd[p + ".linear_k.bias"]).view(B, t, O.HEADS, dk).transpose(1, 2)
    v = F.linear(x, sd[p + ".linear_v.weight"], sd[p + ".linear_v.bias"]).view(B, t, O.HEADS, dk).transpose(1, 2)
    if k_cache is not None:
        k = torch.cat([k_cache, k], dim=2)
        v = torch.cat([v_cache, v], dim=2)
    ks = torch.cat([k[:, :, 1:], torch.zeros_like(k[:, :, :1])], dim=2)
    vs = torch.cat([v[:, :, 1:], torch.zeros_like(v[:, :, :1])], dim=2)
    pp = F.linear(pos_emb, sd[p + ".linear_pos.weight"]).view(pos_emb.size(0), -1, O.HEADS, dk).transpose(1, 2)
    q_u = (q + sd[p + ".pos_bias_u"]).transpose(1, 2)
    q_v = (q + sd[p + ".pos_bias_v"]).transpose(1, 2)
    scores = (torch.matmul(q_u, ks.transpose(-2, -1)) + torch.matmul(q_v, pp.transpose(-2, -1))) / np.sqrt(dk)
    o = torch.matmul(torch.softmax(scores, dim=-1), vs).transpose(1, 2).contiguous().view(B, t, D)
    return F.linear(o, sd[p + ".linear_out.weight"], sd[p + ".linear_out.bias"]), k, v


def _wrong_oracle(monkeypatch, fault):
    if fault == "kv":
        monkeypatch.setattr(O, "rel_attention", _shifted_keys_attention)
    elif fault == "pos":
        good = O.position_encoding
        monkeypatch.setattr(O, "position_encoding", lambda sd, offset, size: good(sd, offset + 1, size))
    else:
        good, older = O.conv_module, {}

        def conv(sd, p, x, cache, mask_pad=None):
            """the left context one frame late: frames [-31, -1) of the stream's history instead of [-30, 0)"""
            _, new_cache = good(sd, p, x, cache, mask_pad)
            seen = torch.cat((cache if cache is not None else torch.zeros_like(new_cache), x.transpose(1, 2)), dim=2)
            wrong = None if cache is None else torch.cat((older[p], cache[:, :, :-1]), dim=2)
            older[p] = seen[:, :, -O.LORDER - 1:-O.LORDER]
            return good(sd, p, x, wrong, mask_pad)[0], new_cache
        monkeypatch.setattr(O, "conv_module", conv)


_F32 = {}


def _f32(case):
    if case not in _F32:
        _F32[case] = W.case_ref(case, 0, torch.float32)
    return _F32[case]


@pytest.mark.parametrize("fault", ["kv", "pos", "conv"])
def test_wrong_oracle_moves_the_frames(case, fault, monkeypatch):
    """A key window shifted by one row, pos_start shifted by one and a conv left context shifted by one frame each move the
    encoder frames of the plan by at least 10 * LOGIT_TOL (float32 runs of the oracle, right against wrong: the movement sought
    is four orders above float32 rounding).  A kernel with one of these faults cannot pass test_encoder_window.py."""
    right = _f32(case)
    _wrong_oracle(monkeypatch, fault)
    wrong = W.case_ref(case, 0, torch.float32, x=W.case_input(case)[0])
    moved = max(W.maxdiff(a["frames"], b["frames"]) for a, b in zip(right, wrong))
    print(f"{W.case_id(case)} fault {fault}: frames move by {moved:.3e} (last chunk {W.maxdiff(right[-1]['frames'], wrong[-1]['frames']):.3e})")
    assert moved >= SENSITIVITY, moved
    assert W.maxdiff(right[-1]["frames"], wrong[-1]["frames"]) >= SENSITIVITY


def test_float32_baseline(case):
    """How much of LOGIT_TOL plain float32 already uses: the float32 oracle against the float64 oracle over the whole plan
    (printed; DESIGN.md records the figures).  Must leave most of the bar to the kernels."""
    d = W.ref_distance(_f32(case), W.case_ref(case, 0))
    print(f"{W.case_id(case)}: float32 oracle vs float64 oracle: frames {d[0]:.3e}, att_cache {d[1]:.3e}, cnn_cache {d[2]:.3e}")
    assert max(d) < W.LOGIT_TOL / 4, d
