"""Deterministic synthetic weights and fbank for parity tests, smoke and bench.

No trained checkpoint ships with the reference (reference .gitignore:10,13 excludes
online_model.pt), so every parity artefact is pinned on seeded weights generated here
with NumPy's Philox bit generator (stream-stable across platforms).  The key set and
shapes are exactly the 504-entry state dict of the reference's OnlineRNNTModel
(model/online_rnnt_model.py:58-143).

Nothing here touches the reference; only encoder_stream_ref imports the CPU oracle (oracle/rnnt_oracle.py), when it is called.
"""
import math
import numpy as np

from .layout import D, H, FF, L, KDW, IDIM, FSUB, VOCAB, BLANK, MAX_LEN, state_dict_spec, chunk_plan  # noqa: F401  (re-exported for the tests)


def positional_table(max_len=MAX_LEN, d=D):
    """pe[pos,2i]=sin(pos/10000^(2i/d)), pe[pos,2i+1]=cos(..) in float32
    (wenet/transformer/embedding.py:50-58).  It is a persistent buffer of the
    reference state dict, so both sides load THIS table."""
    pos = np.arange(max_len, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * np.float32(-(math.log(10000.0) / d)))
    ang = (pos * div).astype(np.float32)
    pe = np.zeros((max_len, d), np.float32)
    pe[:, 0::2] = np.sin(ang)
    pe[:, 1::2] = np.cos(ang)
    return pe[None]


# Per-key gains on top of the 1/sqrt(fan_in) base scale.  Calibrated against the imported
# reference (tests/golden/gen_golden.py prints the achieved rates): residual-branch output
# projections are damped so frame-to-frame variation survives 12 blocks (un-damped random
# blocks collapse every frame onto one vector and greedy emits a single token forever);
# the joint/predictor gains make the logits depend on both encoder frame and label history.
GAINS = (
    (("w_2.weight", "linear_out.weight", "pointwise_conv2.weight"), 0.3),
    (("joint.enc_ffn.weight", "joint.pred_ffn.weight"), 4.0),
    (("predictor.embed.weight",), 2.0),
    (("predictor.rnn.weight_ih_l0", "predictor.rnn.weight_hh_l0"), 4.0),
)


def make_state_dict(seed=0, vocab=VOCAB, blank=BLANK, blank_bias=11.0, out_gain=4.0):
    """504-key state dict as float32 numpy arrays (num_batches_tracked: int64 scalar).

    `out_gain` widens the logit spread so greedy top-2 margins (min ~3e-3 on the fixtures)
    stay far above fp32 rounding; `blank_bias` is added to ffn_out.bias[blank] so greedy
    emits on the order of one symbol per encoder frame (un-biased random weights give the
    10-symbols-per-frame worst case)."""
    sd = {}
    for idx, (name, shape, kind) in enumerate(state_dict_spec(vocab)):
        g = np.random.Generator(np.random.Philox(key=[seed, idx]))
        if kind.startswith("w:"):
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(1.0 / math.sqrt(int(kind[2:])))
        elif kind == "b":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(0.05)
        elif kind == "g":
            a = np.float32(1.0) + g.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
        elif kind == "pb":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
        elif kind == "bn_mean":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(0.1)
        elif kind == "bn_var":
            a = g.uniform(0.5, 1.5, shape).astype(np.float32)
        elif kind == "nbt":
            a = np.array(100, dtype=np.int64)
        elif kind == "emb":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(0.5)
        elif kind == "lstm":
            a = g.uniform(-1.0 / 16, 1.0 / 16, shape).astype(np.float32) * np.float32(2.0)
        elif kind == "out":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(out_gain / math.sqrt(D))
        elif kind == "outb":
            a = g.standard_normal(shape, dtype=np.float32) * np.float32(0.3)
            a[blank] += np.float32(blank_bias)
        elif kind == "pe":
            a = positional_table()
        else:
            raise ValueError(kind)
        for suffixes, gain in GAINS:
            if name.endswith(suffixes):
                a = a * np.float32(gain)
        sd[name] = np.ascontiguousarray(a)
    return sd


FBANK_MEAN, FBANK_STD, FBANK_MIN, FBANK_MAX = -3.72, 5.01, -15.94, 7.01  # example1.pt stats


def synth_fbank(batch, frames, seed=1234):
    """[batch, frames, 80] float32 with the statistics of the reference's example1.pt."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0xFBA]))
    x = g.standard_normal((batch, frames, IDIM), dtype=np.float32) * np.float32(FBANK_STD) + np.float32(FBANK_MEAN)
    return np.clip(x, FBANK_MIN, FBANK_MAX).astype(np.float32)


def greedy_margins(sd_np, enc_frames, tokens, blank=BLANK, device="cuda", n_steps=10):
    """Top-2 logit margin of every decision of a greedy decode (a token flip must be attributable).

    Teacher-forced replay in float64 torch: `enc_frames` [B, F, 256] are the encoder frames the decode ran on, `tokens` the emitted
    tokens per stream; the predictor states come from the LSTM recurrence over each stream's own tokens
    (wenet/transducer/predictor.py:185-210), then the greedy walk (model/online_rnnt_model.py:193-220) evaluates
    joint(enc[t], pred[u]) at every cell it visits.  Returns (min margin per stream [B] float64 numpy, replay_ok [B] bool numpy:
    the replay emitted exactly `tokens`)."""
    import torch
    B = len(tokens)
    dev = torch.device(device)
    enc = torch.as_tensor(np.asarray(enc_frames)).to(dev, torch.float64)
    W = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dev, torch.float64) for k, v in sd_np.items() if k.startswith(("predictor.", "joint."))}
    F_ = enc.size(1)
    nmax = max([len(t) for t in tokens] + [0])
    tk = torch.full((B, nmax + 1), blank, dtype=torch.long, device=dev)       # input token of predictor step u: blank, then the emitted tokens
    for b, t in enumerate(tokens):
        if t:
            tk[b, 1:len(t) + 1] = torch.tensor(t, device=dev)
    h = torch.zeros(B, D, dtype=torch.float64, device=dev)
    c = torch.zeros_like(h)
    P = torch.empty(B, nmax + 1, D, dtype=torch.float64, device=dev)
    bias = W["predictor.rnn.bias_ih_l0"] + W["predictor.rnn.bias_hh_l0"]
    for u in range(nmax + 1):
        g = W["predictor.embed.weight"][tk[:, u]] @ W["predictor.rnn.weight_ih_l0"].T + h @ W["predictor.rnn.weight_hh_l0"].T + bias
        i_, f_, g_, o_ = g.chunk(4, dim=1)
        c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        P[:, u] = (h @ W["predictor.projection.weight"].T + W["predictor.projection.bias"]) @ W["joint.pred_ffn.weight"].T + W["joint.pred_ffn.bias"]
    E = enc @ W["joint.enc_ffn.weight"].T + W["joint.enc_ffn.bias"]
    ar = torch.arange(B, device=dev)
    t_ = torch.zeros(B, dtype=torch.long, device=dev)
    u_ = torch.zeros_like(t_)
    cnt = torch.zeros_like(t_)
    mmin = torch.full((B,), float("inf"), dtype=torch.float64, device=dev)
    ok = torch.ones(B, dtype=torch.bool, device=dev)
    nt = torch.tensor([len(t) for t in tokens], device=dev)
    for _ in range(F_ + nmax + 2):
        act = t_ < F_
        if not bool(act.any()):
            break
        lg = torch.tanh(E[ar, t_.clamp(max=F_ - 1)] + P[ar, u_.clamp(max=nmax)]) @ W["joint.ffn_out.weight"].T + W["joint.ffn_out.bias"]
        top = lg.topk(2, dim=1)
        k = top.indices[:, 0]
        mmin = torch.where(act, torch.minimum(mmin, top.values[:, 0] - top.values[:, 1]), mmin)
        emit = act & (k != blank)
        ok &= ~emit | ((u_ < nt) & (tk[ar, (u_ + 1).clamp(max=nmax)] == k))
        u_ = u_ + emit.long()
        cnt = cnt + emit.long()
        adv = act & ((k == blank) | (cnt >= n_steps))
        t_ = t_ + adv.long()
        cnt = torch.where(adv, torch.zeros_like(cnt), cnt)
    ok &= u_ == nt
    return mmin.cpu().numpy(), ok.cpu().numpy()



# ---- split-operand modes: the two 16-bit planes of an f32 operand (tests) -------------------------------------------------------
def _round16(x32, kind):
    """float32 -> the nearest bf16 / f16 value (ties to even), returned as float32"""
    if kind == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float32)
    assert kind == "bf16", kind
    u = np.ascontiguousarray(x32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(x32.shape)


def split_planes_ref(x, kind):
    """What a split-operand mode carries of an f32 operand: pack2_16 / split8_16 (rnnt_gemm_bf.hip.h) restated.  hi = round16(x),
    lo = round16(x - hi) with the residual formed in float32 as the kernel forms it; returns hi + lo in float64.  kind: "bf16"
    (8-bit planes, f32 exponent range) or "f16" (11-bit planes; a lo plane below 2^-14 is subnormal, its error absolute 2^-25;
    |x| > 65504 overflows)."""
    x32 = np.ascontiguousarray(np.asarray(x, np.float32))
    with np.errstate(invalid="ignore"):                                    # an overflowed hi plane: inf, and a nan sum
        hi = _round16(x32, kind)
        lo = _round16(x32 - hi, kind)
        return hi.astype(np.float64) + lo.astype(np.float64)


def split_error_ref(x, kind):
    """Relative root-mean-square error of split_planes_ref over a tensor: |hi + lo - x|_2 / |x|_2 (0 for an all-zero tensor, inf
    where a plane overflows).  rnnt_finalize_weights compares this figure of each GEMM weight with RNNT_F16X3_SPLIT_LIMIT."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    got = split_planes_ref(x, kind)
    if not np.isfinite(got).all():
        return math.inf
    den = float(np.sqrt((x64 * x64).sum()))
    return float(np.sqrt(((got - x64) ** 2).sum())) / den if den > 0 else 0.0


# ---- teacher-forced scoring: float64 restatements of the transducer likelihood (tests) -----------------------------------------
def _logaddexp(a, b):
    mx, mn = (a, b) if a >= b else (b, a)
    return mx if mx == -math.inf else mx + math.log1p(math.exp(mn - mx))


def transducer_nll_ref(pick, T_b, U_b):
    """-log of the sum over all monotonic alignments of one utterance, as a float64 dynamic programme.  pick [T, U1, 2]:
    pick[t, u, 0] = log P(blank | t, u), pick[t, u, 1] = log P(y_{u+1} | t, u); valid cells t < T_b, u <= U_b (label slot
    u < U_b), nothing else is read.  alpha[0,0] = 0; alpha[t,u] = logaddexp(alpha[t-1,u] + pick[t-1,u,0], alpha[t,u-1] +
    pick[t,u-1,1]); nll = -(alpha[T_b-1,U_b] + pick[T_b-1,U_b,0])."""
    p = np.asarray(pick, np.float64)
    alpha = np.full((T_b, U_b + 1), -math.inf)
    for t in range(T_b):
        for u in range(U_b + 1):
            if t == 0 and u == 0:
                alpha[t, u] = 0.0
                continue
            below = alpha[t - 1, u] + p[t - 1, u, 0] if t > 0 else -math.inf
            left = alpha[t, u - 1] + p[t, u - 1, 1] if u > 0 else -math.inf
            alpha[t, u] = _logaddexp(below, left)
    return -(alpha[T_b - 1, U_b] + p[T_b - 1, U_b, 0])


def nbest_pick_slice(pick, n, U1):
    """Hypothesis n's lattice [T, U1, 2] of one utterance's n-best picked lattice [T, N * U1, 2] (rnnt_transducer_nll_nbest lays the
    hypotheses side by side along U), the argument of transducer_nll_ref."""
    return np.asarray(pick)[:, n * U1:(n + 1) * U1]


def rescore_select_ref(first_scores, nll, first_weight, transducer_weight):
    """The choice of Transducer.transducer_attention_rescoring (wenet/transducer/transducer.py:372-393) with attn_weight = 0, in
    Python floats: score = beam_score[i] * ctc_weight + td_s * transducer_weight with td_s = -nll[i]; best_index starts at 0 with
    -inf and moves on `score > best_score` only, so -inf * 0.0 = nan is never chosen.  Returns (best_index, [score])."""
    best_score, best_index, totals = -float("inf"), 0, []
    for i in range(len(first_scores)):
        td_s = -float(nll[i])
        score = float(first_scores[i]) * float(first_weight) + td_s * float(transducer_weight)
        totals.append(score)
        if score > best_score:
            best_score = score
            best_index = i
    return best_index, totals


def transducer_nll_bruteforce(pick, T_b, U_b):
    """The same likelihood as an explicit sum over every alignment: each one is an order of T_b - 1 blanks and U_b labels
    (C(T_b - 1 + U_b, U_b) of them) followed by the final blank at (T_b - 1, U_b); exact summation (math.fsum) of the path
    probabilities relative to the best path."""
    from itertools import combinations
    p = np.asarray(pick, np.float64)
    n = T_b - 1 + U_b
    logs = []
    for labels_at in combinations(range(n), U_b):
        at, t, u, lp = set(labels_at), 0, 0, 0.0
        for k in range(n):
            if k in at:
                lp += p[t, u, 1]
                u += 1
            else:
                lp += p[t, u, 0]
                t += 1
        logs.append(lp + p[T_b - 1, U_b, 0])
    mx = max(logs)
    return -(mx + math.log(math.fsum(math.exp(v - mx) for v in logs)))


# ---- transducer loss with gradients: float64 yardstick and the device path's arithmetic contract (tests) ------------------------
def transducer_loss_ref(logits, targets, T_b, U_b, blank, fused_log_softmax=True):
    """(nll, grad) of one row by float64 torch autograd through log_softmax and the alpha recursion of transducer_nll_ref.
    logits [T, U1, V] (only t < T_b, u <= U_b is read), targets: at least U_b labels.  grad [T, U1, V] float64 = d nll / d logits,
    0 outside the valid cells.  fused_log_softmax=False: the input holds log-probabilities, differentiated as they stand."""
    import torch
    full = torch.as_tensor(np.asarray(logits))
    x = full[:T_b, :U_b + 1].double().clone().requires_grad_(True)
    lp = torch.log_softmax(x, -1) if fused_log_softmax else x
    ninf = torch.tensor(-math.inf, dtype=torch.float64)
    alpha = [[None] * (U_b + 1) for _ in range(T_b)]
    for t in range(T_b):
        for u in range(U_b + 1):
            if t == 0 and u == 0:
                alpha[t][u] = torch.zeros((), dtype=torch.float64)
                continue
            below = alpha[t - 1][u] + lp[t - 1, u, blank] if t > 0 else ninf
            left = alpha[t][u - 1] + lp[t, u - 1, int(targets[u - 1])] if u > 0 else ninf
            alpha[t][u] = below if u == 0 else (left if t == 0 else torch.logaddexp(below, left))
    nll = -(alpha[T_b - 1][U_b] + lp[T_b - 1, U_b, blank])
    nll.backward()
    grad = np.zeros(tuple(full.shape), np.float64)
    grad[:T_b, :U_b + 1] = x.grad.numpy()
    return float(nll.detach()), grad


def _loss_from_picks(x, lse, pb, pl, targets, T_b, U_b, blank, fused_log_softmax, shape):
    """The gradient formula of rnnt_transducer_loss in float64 from a valid region's logits x [T_b, U_b + 1, V], lse and the two
    picked values [T_b, U_b + 1]: both recursions, then g_k = p_k occ - blank term - label term."""
    al = np.full((T_b, U_b + 1), -math.inf)
    be = np.full((T_b, U_b + 1), -math.inf)
    for t in range(T_b):
        for u in range(U_b + 1):
            if t == 0 and u == 0:
                al[t, u] = 0.0
                continue
            al[t, u] = _logaddexp(al[t - 1, u] + pb[t - 1, u] if t > 0 else -math.inf, al[t, u - 1] + pl[t, u - 1] if u > 0 else -math.inf)
    for t in range(T_b - 1, -1, -1):
        for u in range(U_b, -1, -1):
            if t == T_b - 1 and u == U_b:
                be[t, u] = pb[t, u]
                continue
            be[t, u] = _logaddexp(be[t + 1, u] + pb[t, u] if t + 1 < T_b else -math.inf, be[t, u + 1] + pl[t, u] if u < U_b else -math.inf)
    logZ = be[0, 0]
    grad = np.zeros(shape, np.float64)
    for t in range(T_b):
        for u in range(U_b + 1):
            g = np.exp(x[t, u] - lse[t, u]) * math.exp(al[t, u] + be[t, u] - logZ) if fused_log_softmax else np.zeros(x.shape[-1])
            if t < T_b - 1:
                g[blank] -= math.exp(al[t, u] + pb[t, u] + be[t + 1, u] - logZ)
            elif u == U_b:
                g[blank] -= math.exp(al[t, u] + pb[t, u] - logZ)
            if u < U_b:
                g[int(targets[u])] -= math.exp(al[t, u] + pl[t, u] + be[t, u + 1] - logZ)
            grad[t, u] = g
    return -logZ, grad


def transducer_loss_f32_emulation(logits, targets, T_b, U_b, blank, fused_log_softmax=True):
    """The arithmetic contract of the device path, on the CPU: lse (torch's CPU logsumexp) and the two picked values logit - lse in
    float32, everything after them -- both recursions, p_k = exp(logit_k - lse), the three factors -- in float64.  Arguments and
    result as transducer_loss_ref.  Its distance from transducer_loss_ref is what float32 picks cost; the device is held to a
    small multiple of it."""
    import torch
    full = torch.as_tensor(np.asarray(logits))
    x32 = full[:T_b, :U_b + 1].float()
    lse32 = torch.logsumexp(x32, -1) if fused_log_softmax else torch.zeros(T_b, U_b + 1)
    tg = torch.as_tensor(np.asarray(targets)[:U_b].astype(np.int64))
    pb = (x32[..., blank] - lse32).double().numpy()
    pl = np.full((T_b, U_b + 1), -math.inf)
    if U_b:
        pl[:, :U_b] = (x32[:, :U_b].gather(2, tg[None, :, None].expand(T_b, U_b, 1))[..., 0] - lse32[:, :U_b]).double().numpy()
    return _loss_from_picks(x32.double().numpy(), lse32.double().numpy(), pb, pl, targets, T_b, U_b, blank, fused_log_softmax, tuple(full.shape))


# ---- forced alignment: float64 restatements of the two Viterbi recursions (tests) ----------------------------------------------
def _transducer_forward(p, T_b, U_b):
    """v[t, u] and the move into each cell (True: the label move from (t, u-1)); the blank move wins ties."""
    v = np.full((T_b, U_b + 1), -math.inf)
    label = np.zeros((T_b, U_b + 1), bool)
    for t in range(T_b):
        for u in range(U_b + 1):
            if t == 0 and u == 0:
                v[t, u] = 0.0
                continue
            below = v[t - 1, u] + p[t - 1, u, 0] if t > 0 else -math.inf
            left = v[t, u - 1] + p[t, u - 1, 1] if u > 0 else -math.inf
            label[t, u] = t == 0 or (u > 0 and not below >= left)
            v[t, u] = left if label[t, u] else below
    return v, label


def transducer_align_ref(pick, T_b, U_b):
    """The best monotonic alignment of one utterance over its picked lattice (layout and valid cells as transducer_nll_ref):
    v[0,0] = 0; v[t,u] = max(v[t-1,u] + pick[t-1,u,0], v[t,u-1] + pick[t,u-1,1]), the blank move (from (t-1,u)) taken when its
    value is >= the label move's; best = v[T_b-1,U_b] + pick[T_b-1,U_b,0].  Returns (best, emit, margin): emit [U_b] int32, the
    frame at which each label is emitted; margin = best minus the best score of any complete path through a cell off the best
    path (forward plus backward Viterbi), inf when every cell lies on it."""
    p = np.asarray(pick, np.float64)
    v, label = _transducer_forward(p, T_b, U_b)
    best = v[T_b - 1, U_b] + p[T_b - 1, U_b, 0]
    emit = np.full(U_b, -1, np.int32)
    on_path = np.zeros((T_b, U_b + 1), bool)
    t, u = T_b - 1, U_b
    on_path[t, u] = True
    while t > 0 or u > 0:
        if label[t, u]:
            u -= 1
            emit[u] = t
        else:
            t -= 1
        on_path[t, u] = True
    w = np.full((T_b, U_b + 1), -math.inf)          # best score from cell (t, u) to the end, final blank included
    for t in range(T_b - 1, -1, -1):
        for u in range(U_b, -1, -1):
            if t == T_b - 1 and u == U_b:
                w[t, u] = p[t, u, 0]
                continue
            up = p[t, u, 0] + w[t + 1, u] if t + 1 < T_b else -math.inf
            right = p[t, u, 1] + w[t, u + 1] if u < U_b else -math.inf
            w[t, u] = max(up, right)
    through = (v + w)[~on_path]
    margin = best - through.max() if through.size else math.inf
    return best, emit, margin


def transducer_align_bruteforce(pick, T_b, U_b):
    """Every alignment (an order of T_b - 1 blanks and U_b labels, then the final blank), each summed in path order from the
    start.  Returns [(score, emit tuple)] sorted best first; among equal scores the path the tie rule names comes first: walking
    back from the end, the blank move is preferred where two paths part, which leaves the label before that cell at an earlier
    frame -- the smaller emission frames, compared from the last label backwards."""
    from itertools import combinations
    p = np.asarray(pick, np.float64)
    n = T_b - 1 + U_b
    out = []
    for labels_at in combinations(range(n), U_b):
        at, t, u, lp, emit = set(labels_at), 0, 0, 0.0, []
        for k in range(n):
            if k in at:
                lp = lp + p[t, u, 1]
                emit.append(t)
                u += 1
            else:
                lp = lp + p[t, u, 0]
                t += 1
        out.append((lp + p[T_b - 1, U_b, 0], tuple(emit)))
    out.sort(key=lambda se: (-se[0], tuple(reversed(se[1]))))
    return out


def _ctc_ext(targets, blank):
    ext = [blank]
    for y in targets:
        ext += [int(y), blank]
    return ext


def ctc_align_ref(lp, targets, T_b, blank):
    """The best CTC path of one utterance: lp [T, V] log-probabilities, extended states (blank, y_1, blank, .., y_L, blank);
    v_t[s] = max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2] if s is a label that differs from the one before) + lp[t, ext s]; the
    largest wins and among equals staying beats s-1 beats s-2; the path ends in S-1 if v[S-1] >= v[S-2] (or S == 1), else in
    S-2.  Returns (best, align [T_b] int32: the label of each frame's state, blank included); (-inf, all -1) for a transcript
    its frames cannot hold."""
    p = np.asarray(lp, np.float64)
    ext = _ctc_ext(targets, blank)
    S = len(ext)
    v = np.full(S, -math.inf)
    for s in range(min(S, 2)):
        v[s] = p[0, ext[s]]
    step = np.zeros((T_b, S), np.int64)
    for t in range(1, T_b):
        nv = np.full(S, -math.inf)
        for s in range(S):
            m, k = v[s], 0
            if s >= 1 and v[s - 1] > m:
                m, k = v[s - 1], 1
            if s >= 3 and (s & 1) and ext[s - 2] != ext[s] and v[s - 2] > m:
                m, k = v[s - 2], 2
            nv[s] = m + p[t, ext[s]]
            step[t, s] = k
        v = nv
    s = S - 1 if S == 1 or v[S - 1] >= v[S - 2] else S - 2
    best = v[s]
    align = np.full(T_b, -1, np.int32)
    if best == -math.inf:
        return best, align
    for t in range(T_b - 1, -1, -1):
        align[t] = ext[s]
        s -= step[t, s]
    return float(best), align


def ctc_align_bruteforce(lp, targets, T_b, blank):
    """Every state sequence of T_b frames that starts in state 0 or 1, moves by 0, 1 or (between different labels) 2 states and
    ends in S-1 or S-2, each summed in frame order.  Returns [(score, state tuple)] sorted best first; among equal scores the one
    the tie rule names first: the last state S-1 before S-2, then, walking back, the higher earlier state (the smaller step)."""
    p = np.asarray(lp, np.float64)
    ext = _ctc_ext(targets, blank)
    S = len(ext)
    out = []

    def walk(t, s, score, path):
        if t == T_b - 1:
            if s >= S - 2:
                out.append((score, tuple(path)))
            return
        for k in (0, 1, 2):
            n = s + k
            if n >= S or (k == 2 and not ((n & 1) and ext[n] != ext[s])):
                continue
            path.append(n)
            walk(t + 1, n, score + p[t + 1, ext[n]], path)
            path.pop()
    for s0 in range(min(S, 2)):
        walk(0, s0, p[0, ext[s0]], [s0])
    out.sort(key=lambda sp: (-sp[0], tuple(-s for s in reversed(sp[1]))))
    return out


# ---- CTC loss with gradients: float64 yardstick, the device path's arithmetic contract and the sum over all paths (tests) ---------
def _ctc_skip(ext):
    """skip[s]: state s may be entered from s - 2 (a label that differs from the label before it)"""
    e = np.asarray(ext)
    skip = np.zeros(len(e), bool)
    skip[3::2] = e[3::2] != e[1:-2:2]
    return skip


def ctc_loss_ref(x, targets, T_b, blank, fused_log_softmax=True):
    """(nll, grad) of one row by float64 torch autograd through log_softmax and the forward recursion over the extended states,
    vectorised over the states with one step per frame.  x [T, V] (only t < T_b is read), targets: the row's L labels.  grad [T, V]
    float64 = d nll / d x, 0 for t >= T_b.  fused_log_softmax=False: x holds log-probabilities, differentiated as they stand.  A
    transcript the frames cannot hold: (inf, zeros)."""
    import torch
    full = torch.as_tensor(np.asarray(x))
    ext = _ctc_ext(np.asarray(targets), blank)
    S = len(ext)
    cols = torch.as_tensor(np.asarray(ext, np.int64))
    skip = torch.as_tensor(_ctc_skip(ext))
    xv = full[:T_b].double().clone().requires_grad_(True)
    lp = (torch.log_softmax(xv, -1) if fused_log_softmax else xv)[:, cols]        # [T_b, S]
    ninf = torch.full((S,), -math.inf, dtype=torch.float64)

    def lse(v):                                                    # logsumexp over dim 0 whose all -inf columns stay -inf without a NaN gradient
        dead = torch.isinf(v.detach().max(0).values)
        out = torch.logsumexp(torch.where(dead, torch.zeros_like(v), v), 0)
        return torch.where(dead, torch.full_like(out, -math.inf), out)
    alpha = torch.where(torch.arange(S) < 2, lp[0], ninf)
    for t in range(1, T_b):
        a1 = torch.cat([ninf[:1], alpha[:-1]])
        a2 = torch.where(skip, torch.cat([ninf[:2], alpha[:-2]])[:S], ninf)
        alpha = lse(torch.stack([alpha, a1, a2])) + lp[t]
    nll = -lse(alpha[max(S - 2, 0):].unsqueeze(1))[0]
    grad = np.zeros(tuple(full.shape), np.float64)
    if not math.isfinite(float(nll.detach())):
        return math.inf, grad
    nll.backward()
    grad[:T_b] = xv.grad.numpy()
    return float(nll.detach()), grad


def _ctc_lse3(a, a1, a2):
    mx = np.maximum(a, np.maximum(a1, a2))
    mx = np.where(np.isinf(mx), 0.0, mx)
    with np.errstate(divide="ignore"):
        return np.log(np.exp(a - mx) + np.exp(a1 - mx) + np.exp(a2 - mx)) + mx


def _ctc_loss_from_lp(lp, p, ext, shape):
    """Both recursions of rnnt_ctc_loss in float64 over lp [T_b, S] (the log-probabilities of the extended states' columns), then
    g = p - occupancy with p [T_b, V] (zeros when the input held log-probabilities)."""
    T_b, S = lp.shape
    skip = _ctc_skip(ext)
    ninf = np.full(S + 2, -math.inf)
    al, be = np.full((T_b, S), -math.inf), np.full((T_b, S), -math.inf)
    al[0, :2] = lp[0, :2]
    for t in range(1, T_b):
        prev = np.concatenate([ninf[:2], al[t - 1]])
        al[t] = _ctc_lse3(prev[2:], prev[1:-1], np.where(skip, prev[:-2], -math.inf)) + lp[t]
    be[T_b - 1, max(S - 2, 0):] = lp[T_b - 1, max(S - 2, 0):]
    skip_fwd = np.concatenate([skip[2:], [False, False]])[:S]     # s -> s + 2
    for t in range(T_b - 2, -1, -1):
        nxt = np.concatenate([be[t + 1], ninf[:2]])
        be[t] = _ctc_lse3(nxt[:-2], nxt[1:-1], np.where(skip_fwd, nxt[2:], -math.inf)) + lp[t]
    nll = -_logaddexp(al[T_b - 1, S - 1], al[T_b - 1, S - 2] if S > 1 else -math.inf)
    grad = np.zeros(shape, np.float64)
    if not math.isfinite(nll):
        return math.inf, grad
    ab = al + be
    with np.errstate(invalid="ignore"):
        occ = np.where(np.isinf(ab), 0.0, np.exp(ab - lp + nll))
    g = p.copy()
    for s in range(S):                                             # ascending states, as ctc_loss_occ adds them
        g[:, ext[s]] -= occ[:, s]
    grad[:T_b] = g
    return nll, grad


def ctc_loss_f32_emulation(x, targets, T_b, blank, fused_log_softmax=True):
    """The arithmetic contract of the device path, on the CPU: lse (torch's CPU logsumexp) and the picked values x - lse in float32,
    everything after them -- both recursions, p_k = exp(x_k - lse), the occupancies -- in float64.  Arguments and result as
    ctc_loss_ref.  Its distance from ctc_loss_ref is what float32 picks cost; the device is held to a small multiple of it."""
    import torch
    full = torch.as_tensor(np.asarray(x))
    x32 = full[:T_b].float()
    ext = _ctc_ext(np.asarray(targets), blank)
    lse32 = torch.logsumexp(x32, -1) if fused_log_softmax else torch.zeros(T_b)
    lp = (x32[:, torch.as_tensor(np.asarray(ext, np.int64))] - lse32[:, None]).double().numpy()
    p = np.exp(x32.double().numpy() - lse32.double().numpy()[:, None]) if fused_log_softmax else np.zeros(tuple(x32.shape))
    return _ctc_loss_from_lp(lp, p, ext, tuple(full.shape))


def ctc_loss_bruteforce(lp, targets, T_b, blank):
    """The same likelihood as an explicit sum over all V^T_b label sequences of T_b frames: those that collapse (merge repeats, drop
    blanks) to the transcript, summed exactly (math.fsum) relative to the best one.  lp [T, V] log-probabilities.  inf when none does."""
    from itertools import product
    p = np.asarray(lp, np.float64)
    want = [int(y) for y in targets]
    logs = []
    for path in product(range(p.shape[1]), repeat=T_b):
        got = [k for i, k in enumerate(path) if k != blank and (i == 0 or k != path[i - 1])]
        if got == want:
            logs.append(sum(p[t, k] for t, k in enumerate(path)))
    if not logs or max(logs) == -math.inf:
        return math.inf
    mx = max(logs)
    return -(mx + math.log(math.fsum(math.exp(v - mx) for v in logs)))


# ---- prefix beam search: one frame's merge for one utterance (tests) ------------------------------------------------------------
def _log_add(args):
    """wenet.utils.common.log_add in the list form its prefix-beam-search call site uses."""
    if all(a == -math.inf for a in args):
        return -math.inf
    a_max = max(args)
    return a_max + math.log(sum(math.exp(a - a_max) for a in args))


def prefix_merge_ref(hyps, top_lp, top_tok, blank, beam_size):
    """The merge of wenet/transducer/search/prefix_beam_search.py:105-145 for one utterance in Python lists and doubles.  hyps
    [(tokens, score)], top_lp / top_tok [n][k].  Candidates per hypothesis j, per rank t: the running double score rounded to f32
    (torch.tensor([s.score])), added to the f32 top value in f32 (:105), widened to double (.item()); a blank candidate keeps the
    tokens and state slot 0 of j, any other token appends and takes slot 1; a candidate whose tokens equal an earlier survivor's is
    log-added into it and the first one's tokens and state stay (:130-142); stable descending sort; truncation.
    Returns [(tokens, score, src_row, src_slot)]."""
    fused = []
    for j, (toks, score) in enumerate(hyps):
        s32 = np.float32(score)
        for lp, tok in zip(top_lp[j], top_tok[j]):
            tok = int(tok)
            cand = [list(toks) + ([] if tok == blank else [tok]), float(np.float32(s32 + np.float32(lp))), j, 0 if tok == blank else 1]
            for f in fused:
                if f[0] == cand[0]:
                    f[1] = _log_add([f[1], cand[1]])
                    break
            else:
                fused.append(cand)
    fused.sort(key=lambda v: v[1], reverse=True)
    return [tuple(f) for f in fused[:beam_size]]


# ---- CTC prefix beam search with a context graph (wenet/transformer/search.py:125-247, wenet/utils/context_graph.py) ------------
class context_graph_ref:
    """The Aho-Corasick automaton of context_graph.py:144-210 over phrases [[token, ...], ...] as flat Python lists indexed by node
    id (creation order, root = 0): token (-1 at the root), token_score, node_score (= depth * context_score by repeated addition),
    output_score, is_end, next (dict token -> child), fail, output (-1: none).  is_end is decided when a node is created, so a
    phrase that ends on a node an earlier phrase created does not mark it.  The fail arc of a node over `token` starts from its
    parent's fail arc f: f's child if there is one; else step to f's fail arc, and while that node has no child over the token keep
    stepping, stopping right AFTER a step that lands on the root; then take the child if there is one.  The output arc is the first
    is_end node on the fail chain (none once the chain reaches the root) and its output_score is added to the node's."""

    def __init__(self, phrases, context_score):
        self.context_score = float(context_score)
        self.token, self.token_score, self.node_score, self.output_score, self.is_end, self.next = [-1], [0.0], [0.0], [0.0], [False], [{}]
        for ph in phrases:
            node = 0
            for i, tok in enumerate(ph):
                tok = int(tok)
                if tok not in self.next[node]:
                    end = i == len(ph) - 1
                    ns = self.node_score[node] + self.context_score
                    self.next[node][tok] = len(self.token)
                    self.token.append(tok); self.token_score.append(self.context_score); self.node_score.append(ns)
                    self.output_score.append(ns if end else 0.0); self.is_end.append(end); self.next.append({})
                node = self.next[node][tok]
        n = len(self.token)
        self.fail, self.output = [0] * n, [-1] * n
        queue = list(self.next[0].values())
        while queue:
            cur = queue.pop(0)
            for tok, node in self.next[cur].items():
                f = self.fail[cur]
                if tok in self.next[f]:
                    f = self.next[f][tok]
                else:
                    f = self.fail[f]
                    while tok not in self.next[f]:
                        f = self.fail[f]
                        if f == 0:
                            break
                    f = self.next[f].get(tok, f)
                self.fail[node] = f
                out = f
                while out >= 0 and not self.is_end[out]:
                    out = self.fail[out]
                    if out == 0:
                        out = -1
                self.output[node] = out
                if out >= 0:
                    self.output_score[node] += self.output_score[out]
                queue.append(node)

    def step(self, state, tok):
        """forward_one_step (:212-247): (score of the step, node it lands in)."""
        if tok in self.next[state]:
            node = self.next[state][tok]
            score = self.token_score[node]
        else:
            node = self.fail[state]
            while tok not in self.next[node]:
                node = self.fail[node]
                if node == 0:
                    break
            node = self.next[node].get(tok, node)
            score = self.node_score[node] - self.node_score[state]
        return score + self.output_score[node], node

    def finalize(self, state):
        return -self.node_score[state]

    def walk(self, tokens):
        """tokens from the root -> (step scores, node ids, finalize's score of the last state)."""
        state, scores, states = 0, [], []
        for tok in tokens:
            sc, state = self.step(state, int(tok))
            scores.append(sc); states.append(state)
        return scores, states, self.finalize(state)


def prefix_merge_ctx_ref(hyps, top_lp, top_tok, blank, beam_size, graph):
    """prefix_merge_ref with hot-word biasing (wenet/transformer/search.py:95-104,169-171,214-235 carried over to the transducer
    frame step).  hyps [(tokens, score, context state, context score)], graph: a context_graph_ref.  A blank candidate copies its
    parent's context state and score (copy_context), any other token takes graph.step from the parent's state and adds the step's
    score to the parent's (update_context); fusion is prefix_merge_ref's and keeps the first candidate's context (a function of the
    token sequence alone); stable descending sort by fused score + context score; truncation.
    Returns [(tokens, fused score, src_row, src_slot, context state, context score)]."""
    k = len(top_lp[0])
    plain = prefix_merge_ref([(h[0], h[1]) for h in hyps], top_lp, top_tok, blank, len(hyps) * k)     # every fused survivor, keyed by its first candidate
    out = []
    for toks, score, j, slot in plain:
        state, cs = int(hyps[j][2]), float(hyps[j][3])
        if slot == 1:
            step, state = graph.step(state, int(toks[-1]))
            cs = cs + step
        out.append((toks, score, j, slot, state, cs))
    first = {}
    for j in range(len(hyps)):                                       # candidate order of the survivors: prefix_merge_ref's sort lost it
        for tok in top_tok[j]:
            key = tuple(hyps[j][0]) + (() if int(tok) == blank else (int(tok),))
            first.setdefault(key, len(first))
    out.sort(key=lambda v: first[tuple(v[0])])
    out.sort(key=lambda v: v[1] + v[5], reverse=True)
    return out[:beam_size]


def _log_add2(a, b):
    if a == -math.inf and b == -math.inf:
        return -math.inf
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


class _PrefixEntry:
    __slots__ = ("s", "ns", "v_s", "v_ns", "cur", "times_s", "times_ns", "ctx_state", "ctx_score", "touched")

    def __init__(self):
        self.s = self.ns = self.v_s = self.v_ns = self.cur = -math.inf
        self.times_s, self.times_ns, self.ctx_state, self.ctx_score, self.touched = [], [], 0, 0.0, False

    def score(self):
        return _log_add2(self.s, self.ns)

    def viterbi(self):
        return self.v_s if self.v_s > self.v_ns else self.v_ns

    def times(self):
        return self.times_s if self.v_s > self.v_ns else self.times_ns

    def total(self):
        return self.score() + self.ctx_score


def _gap_stats(stats, vals, beam_size, name):
    for i, (a, b) in enumerate(zip(vals, vals[1:])):
        if a == b == -math.inf:
            stats["inf_ties"] = stats.get("inf_ties", 0) + 1
        elif a == b:
            stats[name] = stats.get(name, 0) + 1
            if i == beam_size - 1:
                stats["cut_ties"] = stats.get("cut_ties", 0) + 1
        elif a > -math.inf:
            stats["nonzero_gap"] = min(stats.get("nonzero_gap", math.inf), a - b)


def ctc_prefix_beam_ref(lp, length, blank, beam_size, graph=None, stats=None, finalize=True):
    """WeNet's ctc_prefix_beam_search (search.py:139-236) for ONE utterance in plain Python: lp [T, vocab] float32, frames
    [0, length), graph a context_graph_ref or None.  Per frame: the top beam_size of the row, value descending and lower index first
    on equal values; outer loop over those tokens, inner over the hypotheses in their order; blank / repeat / other as the
    reference writes them (v_s and times_s ASSIGNED by a blank; strict `<` in the Viterbi updates; the repeat's times_ns[-1] = t
    only when the token's value also exceeds the entry's current one); an entry's context comes from the first contribution that
    touches it, and since it is a function of the token string alone every later contribution must agree, which is asserted; sort
    by score + context score descending, stable over first insertion, truncate.  At the end a graph REPLACES every context score
    by finalize's and the list is not re-sorted; finalize=False skips that and returns the running context scores (score =
    log_add(s, ns) + running), what a search that goes on holds at this frame (rnnt_stream_get_ctc_prefix with final = 0).
    Returns (hyps, prune_gap, top_gap): hyps [(tokens, score, times, context score)]; prune_gap the smallest difference between
    consecutive total scores of any frame's sorted entries, top_gap between consecutive values of any frame's top beam_size + 1
    (inf where there is nothing to compare).  stats: a dict whose "stale_times" counts the repeats that raised v_ns and kept the
    entry's times_ns, "both_live" the frames in which some hypothesis P and a hypothesis P + u were both live, "top_ties" / "prune_ties"
    the exact ties between consecutive finite top values / total scores ("inf_ties": between two -inf), "cut_ties" those of them that sit on the truncation boundary, and
    "nonzero_gap" the smallest difference that is not an exact tie (of either kind), and "rebuilt_parent" the extensions P + u that
    meet a live hypothesis P + u whose parent was a DIFFERENT incarnation of P (P was pruned and came back while P + u stayed
    live): an implementation that names prefixes by the node that created them must still merge the two."""
    lp = np.asarray(lp, np.float32)
    start = _PrefixEntry()
    start.s, start.v_s, start.v_ns = 0.0, 0.0, 0.0
    cur = [((), start)]
    prune_gap = top_gap = math.inf
    born = {(): 0}                      # stats only: the frame at which the live prefix was (last) created
    parent_born = {}                    # ... and the birth frame of the parent it was created from

    def context(entry, src, tok):
        if graph is None:
            return
        state, score = src.ctx_state, src.ctx_score
        if tok is not None:
            sc, state = graph.step(src.ctx_state, tok)
            score = src.ctx_score + sc
        if entry.touched:
            assert entry.ctx_state == state and entry.ctx_score == score, "the context is a function of the token string alone"
        else:
            entry.ctx_state, entry.ctx_score, entry.touched = state, score, True

    for t in range(int(length)):
        row = lp[t] + np.float32(0.0)
        order = sorted(range(row.size), key=lambda v: (-row[v], v))
        vals = [float(row[v]) for v in order[:beam_size + 1]]
        for a, b in zip(vals, vals[1:]):
            if a > -math.inf:
                top_gap = min(top_gap, a - b)
        if stats is not None:
            _gap_stats(stats, vals, beam_size, "top_ties")
        nxt = {}
        if stats is not None and any(q[:-1] == pfx for q, _ in cur for pfx, _ in cur if q):
            stats["both_live"] = stats.get("both_live", 0) + 1
        for u in order[:beam_size]:
            prob = float(row[u])
            for prefix, h in cur:
                last = prefix[-1] if prefix else None
                if u == blank:
                    e = nxt.setdefault(prefix, _PrefixEntry())
                    e.s = _log_add2(e.s, h.score() + prob)
                    e.v_s = h.viterbi() + prob
                    e.times_s = list(h.times())
                    context(e, h, None)
                    continue
                if u == last:
                    e = nxt.setdefault(prefix, _PrefixEntry())
                    e.ns = _log_add2(e.ns, h.ns + prob)
                    if e.v_ns < h.v_ns + prob:
                        e.v_ns = h.v_ns + prob
                        if e.cur < prob:
                            e.cur = prob
                            e.times_ns = list(h.times_ns)
                            e.times_ns[-1] = t
                        elif stats is not None:
                            stats["stale_times"] = stats.get("stale_times", 0) + 1
                    context(e, h, None)
                    add, vit, tm = h.s, h.v_s, h.times_s
                else:
                    add, vit, tm = h.score(), h.viterbi(), h.times()
                if stats is not None and prefix + (u,) in born and parent_born[prefix + (u,)] != born[prefix]:
                    stats["rebuilt_parent"] = stats.get("rebuilt_parent", 0) + 1
                e = nxt.setdefault(prefix + (u,), _PrefixEntry())
                e.ns = _log_add2(e.ns, add + prob)
                if e.v_ns < vit + prob:
                    e.v_ns, e.cur = vit + prob, prob
                    e.times_ns = list(tm) + [t]
                context(e, h, u)
        ranked = sorted(nxt.items(), key=lambda kv: kv[1].total(), reverse=True)
        tot = [e.total() for _, e in ranked]
        for a, b in zip(tot, tot[1:]):
            if a > -math.inf:
                prune_gap = min(prune_gap, a - b)
        if stats is not None:
            _gap_stats(stats, tot, beam_size, "prune_ties")
        cur = ranked[:beam_size]
        if stats is not None:
            old = born
            born = {q: old.get(q, t + 1) for q, _ in cur}
            parent_born = {q: parent_born[q] if q in old else old[q[:-1]] for q, _ in cur if q}
    out = []
    for prefix, h in cur:
        cs = 0.0 if graph is None else graph.finalize(h.ctx_state) if finalize else h.ctx_score
        out.append((list(prefix), h.score() + cs, list(h.times()), cs))
    return out, prune_gap, top_gap


# ---- back-off n-gram model fused in the CTC prefix beam search (semantics: include/rnnt_hip.h, rnnt_ngram_set) -------------------
class ngram_ref:
    """The automaton of rnnt_ngram_set over ngrams [(tokens, logp, bow), ...] in Python floats: a trie in list order (node i + 1 is
    n-gram i, the root node 0; every n-gram's prefix must be listed before it), BOS = vocab, EOS = vocab + 1, fail[c] the node of the
    longest proper suffix of c's n-gram that is listed (the root if none), and the prescaled values W = lm_weight * logp +
    length_bonus (no bonus for an n-gram that ends in EOS), B = lm_weight * bow, U = lm_weight * unk_logp + length_bonus -- each one
    multiplication then one addition.  step only adds, in the order the library adds."""

    def __init__(self, ngrams, vocab, blank, lm_weight, length_bonus, unk_logp):
        self.vocab, self.blank, self.bos, self.eos_tok = int(vocab), int(blank), int(vocab), int(vocab) + 1
        lm_weight, length_bonus = float(lm_weight), float(length_bonus)
        self.node = {(): 0}                                          # token string -> node
        self.next, self.W, self.B, strings = [{}], [0.0], [0.0], [()]
        self.has_eos = False
        for toks, logp, bow in ngrams:
            toks = tuple(int(t) for t in toks)
            assert 1 <= len(toks) <= 8 and toks not in self.node and toks[:-1] in self.node, toks
            assert all(0 <= t < vocab + 2 and t != blank for t in toks) and self.bos not in toks[1:] and self.eos_tok not in toks[:-1], toks
            c = len(self.W)
            self.node[toks] = c
            self.next[self.node[toks[:-1]]][toks[-1]] = c
            self.next.append({})
            strings.append(toks)
            w = lm_weight * float(logp)
            self.W.append(w if toks[-1] == self.eos_tok else w + length_bonus)
            self.B.append(lm_weight * float(bow))
            self.has_eos = self.has_eos or toks[-1] == self.eos_tok
        u = lm_weight * float(unk_logp)
        self.U = u + length_bonus
        self.fail = [0] * len(self.W)
        for c, toks in enumerate(strings):
            for i in range(1, len(toks)):
                if toks[i:] in self.node:
                    self.fail[c] = self.node[toks[i:]]
                    break
        self.start = self.next[0].get(self.bos, 0)

    def step(self, state, tok):
        """(score of the step, node it lands in)"""
        acc, node = 0.0, state
        while True:
            c = self.next[node].get(tok, -1)
            if c >= 0:
                return acc + self.W[c], c
            if node == 0:
                return acc + self.U, 0
            acc += self.B[node]
            node = self.fail[node]

    def eos(self, state):
        return self.step(state, self.eos_tok)[0] if self.has_eos else 0.0

    def walk(self, tokens):
        """tokens from the start state -> (step scores, node ids, the end term of the last state)"""
        state, scores, states = self.start, [], []
        for tok in tokens:
            sc, state = self.step(state, int(tok))
            scores.append(sc); states.append(state)
        return scores, states, self.eos(state)


class _NgramEntry(_PrefixEntry):
    __slots__ = ("ng_state", "ng_score")

    def __init__(self):
        super().__init__()
        self.ng_state, self.ng_score = 0, 0.0

    def total(self):
        return self.score() + self.ctx_score + self.ng_score


def ctc_prefix_beam_ngram_ref(lp, length, blank, beam_size, graph=None, ngram=None, stats=None, finalize=True):
    """ctc_prefix_beam_ref with an ngram_ref fused (either of graph and ngram may be None): every entry also carries an n-gram
    score and state, copied where the context is copied and advanced by ngram.step where the context is advanced, under the same
    first-touch flag; the second prune sorts by score + context score + n-gram score, the first prune stays acoustic; at the end
    (finalize) the n-gram score gains ngram.eos(state) and the list is not re-sorted.  The gap statistics are those of
    ctc_prefix_beam_ref, taken over the totals with the n-gram term.
    Returns (hyps, prune_gap, top_gap): hyps [(tokens, score, times, context score, n-gram score)]."""
    lp = np.asarray(lp, np.float32)
    start = _NgramEntry()
    start.s, start.v_s, start.v_ns = 0.0, 0.0, 0.0
    if ngram is not None:
        start.ng_state = ngram.start
    cur = [((), start)]
    prune_gap = top_gap = math.inf
    born, parent_born = {(): 0}, {}

    def context(entry, src, tok):
        if graph is None and ngram is None:
            return
        state, score, ng_state, ng_score = src.ctx_state, src.ctx_score, src.ng_state, src.ng_score
        if tok is not None:
            if graph is not None:
                sc, state = graph.step(src.ctx_state, tok)
                score = src.ctx_score + sc
            if ngram is not None:
                sc, ng_state = ngram.step(src.ng_state, tok)
                ng_score = src.ng_score + sc
        if entry.touched:
            assert (entry.ctx_state, entry.ctx_score, entry.ng_state, entry.ng_score) == (state, score, ng_state, ng_score), \
                "context and n-gram score are functions of the token string alone"
        else:
            entry.ctx_state, entry.ctx_score, entry.ng_state, entry.ng_score, entry.touched = state, score, ng_state, ng_score, True

    for t in range(int(length)):
        row = lp[t] + np.float32(0.0)
        order = sorted(range(row.size), key=lambda v: (-row[v], v))
        vals = [float(row[v]) for v in order[:beam_size + 1]]
        for a, b in zip(vals, vals[1:]):
            if a > -math.inf:
                top_gap = min(top_gap, a - b)
        if stats is not None:
            _gap_stats(stats, vals, beam_size, "top_ties")
        nxt = {}
        if stats is not None and any(q[:-1] == pfx for q, _ in cur for pfx, _ in cur if q):
            stats["both_live"] = stats.get("both_live", 0) + 1
        for u in order[:beam_size]:
            prob = float(row[u])
            for prefix, h in cur:
                last = prefix[-1] if prefix else None
                if u == blank:
                    e = nxt.setdefault(prefix, _NgramEntry())
                    e.s = _log_add2(e.s, h.score() + prob)
                    e.v_s = h.viterbi() + prob
                    e.times_s = list(h.times())
                    context(e, h, None)
                    continue
                if u == last:
                    e = nxt.setdefault(prefix, _NgramEntry())
                    e.ns = _log_add2(e.ns, h.ns + prob)
                    if e.v_ns < h.v_ns + prob:
                        e.v_ns = h.v_ns + prob
                        if e.cur < prob:
                            e.cur = prob
                            e.times_ns = list(h.times_ns)
                            e.times_ns[-1] = t
                        elif stats is not None:
                            stats["stale_times"] = stats.get("stale_times", 0) + 1
                    context(e, h, None)
                    add, vit, tm = h.s, h.v_s, h.times_s
                else:
                    add, vit, tm = h.score(), h.viterbi(), h.times()
                if stats is not None and prefix + (u,) in born and parent_born[prefix + (u,)] != born[prefix]:
                    stats["rebuilt_parent"] = stats.get("rebuilt_parent", 0) + 1
                e = nxt.setdefault(prefix + (u,), _NgramEntry())
                e.ns = _log_add2(e.ns, add + prob)
                if e.v_ns < vit + prob:
                    e.v_ns, e.cur = vit + prob, prob
                    e.times_ns = list(tm) + [t]
                context(e, h, u)
        ranked = sorted(nxt.items(), key=lambda kv: kv[1].total(), reverse=True)
        tot = [e.total() for _, e in ranked]
        for a, b in zip(tot, tot[1:]):
            if a > -math.inf:
                prune_gap = min(prune_gap, a - b)
        if stats is not None:
            _gap_stats(stats, tot, beam_size, "prune_ties")
        cur = ranked[:beam_size]
        if stats is not None:
            old = born
            born = {q: old.get(q, t + 1) for q, _ in cur}
            parent_born = {q: parent_born[q] if q in old else old[q[:-1]] for q, _ in cur if q}
    out = []
    for prefix, h in cur:
        cs = 0.0 if graph is None else graph.finalize(h.ctx_state) if finalize else h.ctx_score
        ls = 0.0 if ngram is None else h.ng_score + ngram.eos(h.ng_state) if finalize else h.ng_score
        out.append((list(prefix), h.score() + cs + ls, list(h.times()), cs, ls))
    return out, prune_gap, top_gap


# ---- n-gram shallow fusion in the transducer prefix beam search (semantics: include/rnnt_hip.h, rnnt_prefix_beam_decode_ngram) ----
NG_START = -1     # the n-gram state of a hypothesis before its first token: the start state of the model the search runs under


def ngram_step_ref(ngram, state, tok):
    """ngram.step with the start marker resolved: (score of the step, node it lands in)."""
    return ngram.step(ngram.start if state == NG_START else state, tok)


def ngram_eos_ref(ngram, state):
    return ngram.eos(ngram.start if state == NG_START else state)


def prefix_merge_ngram_ref(hyps, top_lp, top_tok, blank, beam_size, graph, ngram):
    """prefix_merge_ref with hot-word biasing (graph: a context_graph_ref or None) and n-gram shallow fusion (ngram: an ngram_ref or
    None).  hyps [(tokens, score, context state, context score, n-gram state, n-gram score)]; [blank] holds NG_START.  A blank
    candidate copies its parent's context and n-gram state and score; any other token takes graph.step / ngram.step from the
    parent's state and adds the step's score to the parent's; fusion is prefix_merge_ref's and keeps the first candidate's values
    (functions of the token sequence alone); stable descending sort by fused score + context score + n-gram score, left to right, a
    term whose feature is off left out; truncation.
    Returns [(tokens, fused score, src_row, src_slot, context state, context score, n-gram state, n-gram score)]."""
    k = len(top_lp[0])
    plain = prefix_merge_ref([(h[0], h[1]) for h in hyps], top_lp, top_tok, blank, len(hyps) * k)     # every fused survivor, keyed by its first candidate
    out = []
    for toks, score, j, slot in plain:
        cst, cs, nst, ns = int(hyps[j][2]), float(hyps[j][3]), int(hyps[j][4]), float(hyps[j][5])
        if slot == 1 and graph is not None:
            step, cst = graph.step(cst, int(toks[-1]))
            cs = cs + step
        if slot == 1 and ngram is not None:
            step, nst = ngram_step_ref(ngram, nst, int(toks[-1]))
            ns = ns + step
        out.append((toks, score, j, slot, cst, cs, nst, ns))
    first = {}
    for j in range(len(hyps)):                                       # candidate order of the survivors: prefix_merge_ref's sort lost it
        for tok in top_tok[j]:
            key = tuple(hyps[j][0]) + (() if int(tok) == blank else (int(tok),))
            first.setdefault(key, len(first))
    out.sort(key=lambda v: first[tuple(v[0])])
    out.sort(key=lambda v: prefix_total_ref(v[1], v[5] if graph is not None else None, v[7] if ngram is not None else None), reverse=True)
    return out[:beam_size]


def prefix_total_ref(score, ctx_score=None, ng_score=None):
    """The key of the second prune and the returned total: score + context score + n-gram score, left to right; None: feature off."""
    t = score
    if ctx_score is not None:
        t = t + ctx_score
    if ng_score is not None:
        t = t + ng_score
    return t


# ---- streaming encoder: one stream through the oracle's forward_chunk under any window policy (tests) ---------------------------
_REF_SD = {}


def ref_state_dict(np_sd, dtype=None, share=None):
    """The state dict as torch CPU tensors with every floating-point entry cast to `dtype` (default float64), kept per (dict, dtype).
    share: another state dict; an entry that is the very same array there takes that dict's cast tensor instead of a copy of its
    own (variants of one set of weights that differ in a few tensors)."""
    import torch
    dtype = dtype or torch.float64
    key = (id(np_sd), dtype)
    if key not in _REF_SD:
        shared = ref_state_dict(share, dtype) if share is not None else {}
        _REF_SD[key] = (np_sd, {k: shared[k] if share is not None and share.get(k) is v
                                else torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == "f" else torch.from_numpy(np.asarray(v))
                                for k, v in np_sd.items()})
    return _REF_SD[key][1]


def encoder_stream_ref(np_sd, x, plan, dtype=None):
    """One stream (B = 1) chunk by chunk through the oracle's forward_chunk (wenet/transformer/encoder.py:203-299) on the state
    dict cast to `dtype` (default float64; the cast dict is kept per (state dict, dtype)).  x [T, 80] fbank frames (numpy or
    torch); plan = [(start, length, offset, required_cache_size)], chunk c covering x[start:start + length].  The caches are
    carried from chunk to chunk as the reference's caller does.  Returns one dict per chunk in the reference's layouts, as numpy
    arrays of `dtype`: "frames" [t', 256] (after after_norm), "att" [12, 4, cache_len, 128] and "cnn" [12, 1, 256, 30] as they
    stand after the chunk, plus the chunk's "pos_start" (first row of its positional window) and "cache_len"."""
    import torch
    from oracle import rnnt_oracle as O
    dtype = dtype or torch.float64
    sd = ref_state_dict(np_sd, dtype)
    xs = torch.as_tensor(np.asarray(x)).to(dtype)
    assert xs.dim() == 2, "one stream per call: x is [T, 80]"
    att, cnn = torch.zeros((0, 0, 0, 0), dtype=dtype), torch.zeros((0, 0, 0, 0), dtype=dtype)
    out = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)     # rows are few (t' <= ~20): float64 matrix-vector products with many threads are very slow
    try:
        with torch.no_grad():
            for start, length, offset, required in plan:
                tr = {}
                y, att, cnn = O.forward_chunk(sd, xs[None, start:start + length], offset, required, att, cnn, tr)
                assert y.dtype == dtype and att.dtype == dtype and cnn.dtype == dtype
                out.append({"frames": y[0].numpy().copy(), "att": att.numpy().copy(), "cnn": cnn.numpy().copy(),
                            "pos_start": int(tr["pos_start"]), "cache_len": int(att.size(2))})
    finally:
        torch.set_num_threads(threads)
    return out


# ---- the joint lattice with gradients: float64 yardstick and the device path's arithmetic contract (tests) -----------------------
JR_PRESCALE = np.float32(2.8853900817779268)      # 2 log2(e): rnnt_joint.hip.h


def joint_live_cells(B, T, U1, logit_lens=None, target_lens=None):
    """[B, T, U1] bool: the cells a joint backward with these lengths reads (all of them without lengths)."""
    live = np.ones((B, T, U1), bool)
    for b in range(B):
        if logit_lens is not None:
            live[b, int(logit_lens[b]):] = False
        if target_lens is not None:
            live[b, :, int(target_lens[b]) + 1:] = False
    return live


def joint_backward_ref(e, p, w, g, logit_lens=None, target_lens=None):
    """(de, dp, dW, db) float64 by torch autograd of tanh(e.unsqueeze(2) + p.unsqueeze(1)) @ W.T + b in float64 on the CPU for a given
    g = d loss / d logits [B, T, U1, V]; with lengths, g outside the live cells is taken as 0 whatever it holds."""
    import torch
    g = np.asarray(g)
    B, T, U1, V = g.shape
    live = joint_live_cells(B, T, U1, logit_lens, target_lens)
    g64 = torch.from_numpy(np.where(live[..., None], g, 0.0).astype(np.float64))
    e64, p64, w64 = (torch.from_numpy(np.asarray(a, np.float32).astype(np.float64)).requires_grad_(True) for a in (e, p, w))
    b64 = torch.zeros(V, dtype=torch.float64, requires_grad=True)
    out = torch.tanh(e64.unsqueeze(2) + p64.unsqueeze(1)) @ w64.T + b64
    out.backward(g64)
    return tuple(a.grad.numpy() for a in (e64, p64, w64, b64))


def _bf16_planes(x):
    x32 = np.ascontiguousarray(np.asarray(x, np.float32))
    hi = _round16(x32, "bf16")
    return hi, _round16(x32 - hi, "bf16")


def _mm_bf16x3(a, b):
    """a [m, k] @ b [k, n] as the bf16x3 MFMA forms it: both operands as two bf16 planes (split_planes_ref's), the three products
    lo hi + hi lo + hi hi, each product exact in float32 and accumulated in float32 (three float32 matrix products)."""
    ah, al = _bf16_planes(a)
    bh, bl = _bf16_planes(b)
    return ((al @ bh) + (ah @ bl)) + (ah @ bh)


def joint_tanh_f32(e, p):
    """tanh(e + p) [B, T, U1, 256] as the lattice kernels form it, in float32: t = JR_PRESCALE e + JR_PRESCALE p (each product
    rounded), h = 1 - 2 / (exp2(t) + 1) -- exp2 overflow gives exactly 1, underflow exactly -1."""
    e32, p32 = np.asarray(e, np.float32), np.asarray(p, np.float32)
    with np.errstate(over="ignore"):
        t = (JR_PRESCALE * e32)[:, :, None, :] + (JR_PRESCALE * p32)[:, None, :, :]
        return (np.float32(1.0) - np.float32(2.0) / (np.exp2(t) + np.float32(1.0))).astype(np.float32)


def joint_forward_emulation(e, p, w, b):
    """The forward's arithmetic contract on the CPU: float32 tanh, the bf16x3 contraction with W, plus the bias; [B, T, U1, V] float32."""
    h = joint_tanh_f32(e, p)
    B, T, U1, D_ = h.shape
    w32 = np.asarray(w, np.float32)
    return (_mm_bf16x3(h.reshape(-1, D_), w32.T) + np.asarray(b, np.float32)).reshape(B, T, U1, w32.shape[0])


def joint_backward_emulation(e, p, w, g, logit_lens=None, target_lens=None):
    """The arithmetic contract of rnnt_joint_lattice_backward on the CPU, (de, dp, dW, db) float32: dh = g W and dW = g^T h as bf16x3
    contractions (operand planes via the split_planes_ref rounding, float32 products accumulated in float32), float32 tanh as the
    forward forms it, 1 - h^2 and dz in float32, and the sums over u (de), t (dp) and the cells (db) as plain float32 chains in
    memory order.  Its distance from joint_backward_ref is what this arithmetic costs; the device, which adds in another (fixed)
    order, is held to a small multiple of it.  Cells outside the lengths enter as g = 0, h = 0."""
    g = np.asarray(g)
    B, T, U1, V = g.shape
    live = joint_live_cells(B, T, U1, logit_lens, target_lens)[..., None]
    g0 = np.where(live, g, np.float32(0.0)).astype(np.float32).reshape(-1, V)
    h = np.where(live, joint_tanh_f32(e, p), np.float32(0.0)).astype(np.float32)
    w32 = np.asarray(w, np.float32)
    dh = _mm_bf16x3(g0, w32).reshape(h.shape)
    dz = np.where(live, dh * (np.float32(1.0) - h * h), np.float32(0.0)).astype(np.float32)
    de = np.cumsum(dz, axis=2, dtype=np.float32)[:, :, -1]
    dp = np.cumsum(dz, axis=1, dtype=np.float32)[:, -1]
    dw = _mm_bf16x3(g0.T, h.reshape(-1, h.shape[-1]))
    db = np.cumsum(g0, axis=0, dtype=np.float32)[-1]
    return de, dp, dw, db


# ---- the predictor's LSTM with gradients: float64 yardstick and the device path's arithmetic contract (tests) ---------------------
LSTM_NAMES = ("out", "dx", "dW_ih", "dW_hh", "db", "dh0", "dc0")


def _lstm_mask(B, U1, lens):
    """[B, U1] bool: the steps a row runs (all of them without lengths)"""
    return np.ones((B, U1), bool) if lens is None else np.arange(U1)[None, :] < np.asarray(lens).reshape(B, 1)


def lstm_ref(x, w_ih, w_hh, b_ih, b_hh, dout, h0=None, c0=None, lens=None, final=False):
    """(out, dx, dW_ih, dW_hh, db, dh0, dc0) float64 by torch autograd on the CPU of the step loop written out, gates (i, f, g, o) from
    x_u W_ih^T + b_ih + b_hh + h W_hh^T.  With lens a 0/1 mask freezes a row's state and zeroes its outputs and its dout beyond its
    length (whatever x and dout hold there).  final=True appends (hN, cN)."""
    import torch
    x = np.asarray(x)
    B, U1, Dn = x.shape
    live = _lstm_mask(B, U1, lens)
    t64 = lambda a, grad=True: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64)).requires_grad_(grad)
    x64 = t64(np.where(live[..., None], x, np.float32(0.0)))
    g64 = t64(np.where(live[..., None], dout, np.float32(0.0)), False)
    wi, wh, bi, bh = (t64(a) for a in (w_ih, w_hh, b_ih, b_hh))
    h_0 = t64(np.zeros((B, Dn), np.float32) if h0 is None else h0)
    c_0 = t64(np.zeros((B, Dn), np.float32) if c0 is None else c0)
    m = torch.from_numpy(live.astype(np.float64))
    h, c, outs = h_0, c_0, []
    for u in range(U1):
        gates = x64[:, u] @ wi.T + bi + bh + h @ wh.T
        gi, gf, gg, go = gates.chunk(4, dim=1)
        c_new = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h_new = torch.sigmoid(go) * torch.tanh(c_new)
        mu = m[:, u:u + 1]
        c = mu * c_new + (1.0 - mu) * c
        h = mu * h_new + (1.0 - mu) * h
        outs.append(mu * h_new)
    out = torch.stack(outs, dim=1)
    out.backward(g64)
    res = (out.detach().numpy(), x64.grad.numpy(), wi.grad.numpy(), wh.grad.numpy(), bi.grad.numpy(), h_0.grad.numpy(), c_0.grad.numpy())
    return res + (h.detach().numpy(), c.detach().numpy()) if final else res


def lstm_sigmoid_f32(v):
    """the library's logistic function in float32: 1 / (1 + exp2(-v log2 e)); exp2 overflow gives exactly 0, underflow exactly 1"""
    with np.errstate(over="ignore", under="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp2(np.float32(-1.4426950408889634) * np.asarray(v, np.float32)))).astype(np.float32)


def lstm_f32_emulation(x, w_ih, w_hh, b_ih, b_hh, dout, h0=None, c0=None, lens=None):
    """The arithmetic contract of rnnt_lstm_forward / _backward on the CPU, (out, dx, dW_ih, dW_hh, db, dh0, dc0) float32: every product,
    sum and activation in float32, the device's logistic formula, float32 tanh, the saved gates and c reused by the backward, plain
    float32 contractions and db as a float32 chain in memory order.  Its distance from lstm_ref is what this arithmetic costs; the
    device, which adds in another (fixed) order, is held to a small multiple of it."""
    f = np.float32
    x = np.asarray(x, f)
    B, U1, Dn = x.shape
    live = _lstm_mask(B, U1, lens)
    x0 = np.where(live[..., None], x, f(0.0)).astype(f)
    g0 = np.where(live[..., None], np.asarray(dout, f), f(0.0)).astype(f)
    wi, wh = np.asarray(w_ih, f), np.asarray(w_hh, f)
    xg = (x0.reshape(-1, Dn) @ wi.T + (np.asarray(b_ih, f) + np.asarray(b_hh, f))).reshape(B, U1, 4 * Dn)
    h = np.zeros((B, Dn), f) if h0 is None else np.asarray(h0, f).copy()
    c = np.zeros((B, Dn), f) if c0 is None else np.asarray(c0, f).copy()
    c_first = c.copy()
    out, hprev, st = np.zeros((B, U1, Dn), f), np.zeros((B, U1, Dn), f), np.zeros((B, U1, 5, Dn), f)
    for u in range(U1):
        m = live[:, u:u + 1]
        hprev[:, u] = np.where(m, h, f(0.0))
        pre = (xg[:, u] + h @ wh.T).astype(f)
        gi, gf, go = lstm_sigmoid_f32(pre[:, :Dn]), lstm_sigmoid_f32(pre[:, Dn:2 * Dn]), lstm_sigmoid_f32(pre[:, 3 * Dn:])
        gg = np.tanh(pre[:, 2 * Dn:3 * Dn]).astype(f)
        c_new = (gf * c + gi * gg).astype(f)
        h_new = (go * np.tanh(c_new)).astype(f)
        st[:, u] = np.stack([gi, gf, gg, go, c_new], axis=1)
        out[:, u] = np.where(m, h_new, f(0.0))
        c, h = np.where(m, c_new, c).astype(f), np.where(m, h_new, h).astype(f)
    dG = np.zeros((B, U1, 4 * Dn), f)
    dh, dc = np.zeros((B, Dn), f), np.zeros((B, Dn), f)
    one = f(1.0)
    for u in range(U1 - 1, -1, -1):
        m = live[:, u:u + 1]
        gi, gf, gg, go, cc = (st[:, u, k] for k in range(5))
        cprev = st[:, u - 1, 4] if u > 0 else c_first
        d = (g0[:, u] + dh).astype(f)
        tc = np.tanh(cc).astype(f)
        dct = (dc + d * go * (one - tc * tc)).astype(f)
        dg_u = np.concatenate([dct * gg * (gi * (one - gi)), dct * cprev * (gf * (one - gf)), dct * gi * (one - gg * gg), d * tc * (go * (one - go))], axis=1)
        dG[:, u] = np.where(m, dg_u, f(0.0))
        dc = np.where(m, dct * gf, dc).astype(f)
        dh = np.where(m, dG[:, u] @ wh, dh).astype(f)
    dG2 = dG.reshape(-1, 4 * Dn)
    return (out, (dG2 @ wi).reshape(B, U1, Dn), dG2.T @ x0.reshape(-1, Dn), dG2.T @ hprev.reshape(-1, Dn), np.cumsum(dG2, axis=0, dtype=f)[-1], dh, dc)


# ---- an encoder layer's attention core with gradients: float64 yardstick and the device path's arithmetic contract (tests) --------
ATTN_NAMES = ("out", "dq", "dk", "dv", "dp", "du", "dvb")
ATTN_TILE = 16                                   # keys per tile of the device's online softmax (rnnt_attn_grad.hip.h)


def chunk_visible(T, lengths, chunk_size, num_left_chunks):
    """bool [B, T, T]: visible[b, i, j] of rnnt_rel_attention_forward -- j < len_b, and with chunk_size > 0 also
    j < min(T, (i // chunk_size + 1) chunk_size) and, with num_left_chunks >= 0, j >= (i // chunk_size - num_left_chunks) chunk_size.
    lengths None: one row of T keys."""
    lens = np.full(1, T, np.int64) if lengths is None else np.asarray(lengths, np.int64).reshape(-1)
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    win = np.ones((T, T), bool)
    if chunk_size > 0:
        win = j < np.minimum(T, (i // chunk_size + 1) * chunk_size)
        if num_left_chunks >= 0:
            win = win & (j >= (i // chunk_size - num_left_chunks) * chunk_size)
    return win[None] & (j[None] < lens[:, None, None])


def _attn_heads(a, T):
    """[B, T, 256] -> [B, 4, T, 64] (a copy)"""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(a.shape[0], T, 4, 64).transpose(0, 2, 1, 3))


def _attn_args(q, k, v, lens):
    """(B, T, lens [B], k and v with zeros at j >= len_b: what lies there is never read)"""
    B, T = np.asarray(q).shape[:2]
    lens = np.full(B, T, np.int64) if lens is None else np.asarray(lens, np.int64).reshape(B)
    live = (np.arange(T)[None, :] < lens[:, None])[..., None]
    return B, T, lens, np.where(live, k, np.float32(0.0)).astype(np.float32), np.where(live, v, np.float32(0.0)).astype(np.float32)


def rel_attention_ref(q, k, v, p, u, vb, dout, lens=None, chunk_size=0, num_left_chunks=-1):
    """(out, dq, dk, dv, dp, du, dvb) float64 by torch autograd on the CPU of the formula written out densely:
    s = ((q + u) k^T + (q + vb) p^T) / 8 per head, softmax over the visible keys (0 at hidden ones, all 0 for a row without a visible
    key), out = a v, gradients of (out * dout).sum()."""
    import torch
    B, T, _, k0, v0 = _attn_args(q, k, v, lens)
    vis = torch.from_numpy(chunk_visible(T, np.full(B, T) if lens is None else lens, chunk_size, num_left_chunks))[:, None]       # [B, 1, T, T]
    t64 = lambda a, grad=True: torch.from_numpy(np.asarray(a, np.float32).astype(np.float64)).requires_grad_(grad)
    q64, k64, v64, p64, u64, vb64 = (t64(a) for a in (q, k0, v0, p, u, vb))
    g64 = t64(dout, False)
    hd = lambda a: a.view(a.shape[0], T, 4, 64).transpose(1, 2)                  # [B, 4, T, 64]
    qh, kh, vh, ph = hd(q64), hd(k64), hd(v64), p64.view(1, T, 4, 64).transpose(1, 2)
    s = ((qh + u64[None, :, None, :]) @ kh.transpose(-1, -2) + (qh + vb64[None, :, None, :]) @ ph.transpose(-1, -2)) / 8.0
    m = s.detach().masked_fill(~vis, -math.inf).amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(torch.where(vis, s, m) - m), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    a = e / torch.where(l > 0, l, torch.ones_like(l))
    out = (a @ vh).transpose(1, 2).reshape(B, T, 256)
    out.backward(g64)
    return (out.detach().numpy(),) + tuple(t.grad.numpy() for t in (q64, k64, v64, p64, u64, vb64))


def rel_attention_emulation(q, k, v, p, u, vb, dout, lens=None, chunk_size=0, num_left_chunks=-1):
    """The arithmetic contract of rnnt_rel_attention_forward / _backward on the CPU, (out, dq, dk, dv, dp, du, dvb) float32.  Every
    contraction is a float32 product (the device's exact-f32 MFMA: float32 products, float32 accumulation); the softmax runs online
    over tiles of 16 keys in float32 -- running max, exp, running sum, the rescaling of out -- and saves m + log(l) per row; the
    backward recomputes a = exp(s - lse) per key tile, delta = dout . out, ds = a (dout v^T - delta) / 8 in float32, and adds dp over
    the rows and du, dvb over rows and queries as float32 chains in index order.  A probability is formed from visible keys only.  Its
    distance from rel_attention_ref is what this arithmetic costs; the device, which adds in another (fixed) order, is held to a
    small multiple of it."""
    f = np.float32
    B, T, lens, k0, v0 = _attn_args(q, k, v, lens)
    vis = chunk_visible(T, lens, chunk_size, num_left_chunks)[:, None]           # [B, 1, T, T]
    qh, kh, vh, gh = (_attn_heads(np.asarray(a, f), T) for a in (q, k0, v0, dout))
    ph = _attn_heads(np.asarray(p, f)[None], T)                                  # [1, 4, T, 64]
    u32, vb32 = np.asarray(u, f)[None, :, None, :], np.asarray(vb, f)[None, :, None, :]
    qu, qv = (qh + u32).astype(f), (qh + vb32).astype(f)
    tr = lambda a: a.transpose(0, 1, 3, 2)
    tiles = [slice(j0, min(T, j0 + ATTN_TILE)) for j0 in range(0, T, ATTN_TILE)]
    scores = lambda sl: ((qu @ tr(kh[:, :, sl]) + qv @ tr(ph[:, :, sl])) * f(0.125)).astype(f)
    m, l, o = np.full((B, 4, T), -np.inf, f), np.zeros((B, 4, T), f), np.zeros((B, 4, T, 64), f)
    for sl in tiles:
        s, vt = scores(sl), vis[..., sl]
        mn = np.maximum(m, np.where(vt, s, f(-np.inf)).max(-1))
        alpha = np.exp(np.where(np.isinf(m), f(0.0), m - np.where(np.isinf(mn), f(0.0), mn))).astype(f)
        pe = np.where(vt, np.exp(np.where(vt, s - np.where(np.isinf(mn), f(0.0), mn)[..., None], f(0.0))), f(0.0)).astype(f)
        l = (l * alpha + pe.sum(-1, dtype=f)).astype(f)
        o = (o * alpha[..., None] + pe @ vh[:, :, sl]).astype(f)
        m = mn
    dead = np.isinf(m)
    l1 = np.where(dead, f(1.0), l)
    out = np.where(dead[..., None], f(0.0), o / l1[..., None]).astype(f)
    lse = np.where(dead, f(0.0), m + np.log(l1)).astype(f)
    delta = (gh * out).sum(-1, dtype=f)
    A, Bm = np.zeros((B, 4, T, 64), f), np.zeros((B, 4, T, 64), f)
    dk, dv, dpp = np.zeros_like(A), np.zeros_like(A), np.zeros_like(A)
    for sl in tiles:
        s, vt = scores(sl), vis[..., sl]
        a = np.where(vt, np.exp(np.where(vt, s - lse[..., None], f(0.0))), f(0.0)).astype(f)
        ds = (a * (gh @ tr(vh[:, :, sl]) - delta[..., None]) * f(0.125)).astype(f)
        A += ds @ kh[:, :, sl]
        Bm += ds @ ph[:, :, sl]
        dv[:, :, sl], dk[:, :, sl], dpp[:, :, sl] = tr(a) @ gh, tr(ds) @ qu, tr(ds) @ qv
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(a.shape[0], T, 256)
    chain = lambda a: np.cumsum(a, axis=0, dtype=f)[-1]
    return (back(out), back(A + Bm), back(dk), back(dv), chain(back(dpp)), chain(back(A).reshape(B * T, 4, 64)), chain(back(Bm).reshape(B * T, 4, 64)))
