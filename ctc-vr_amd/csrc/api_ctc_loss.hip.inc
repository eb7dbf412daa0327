// C ABI: the CTC loss with its gradient over a caller's logits or log-probabilities (torch.nn.functional.ctc_loss), and its pure
// C++ twin.  No context, like rnnt_transducer_loss: refusals are status codes without a message.  rnnt_ctc_loss_elem is the device
// entry point for float, bfloat16 and float16 input; rnnt_ctc_loss is its float case.
// Included by rnnt_api.hip inside extern "C" (the one template, ctc_loss_launch, steps out of it).  Kernels: rnnt_ctc_loss.hip.h.

// strides, lengths and labels of a CTC loss call, checked on the host before anything is launched or written
static int ctc_loss_check(const void* logits, int64_t sb, int64_t st, const int32_t* targets, const int32_t* logit_lens, const int32_t* target_lens,
                          int32_t B, int32_t T, int32_t Lmax, int32_t V, int32_t blank, const void* nll) {
    if (!logits || !logit_lens || !target_lens || !nll || (Lmax > 0 && !targets)) return RNNT_ERR_ARG;
    if (B < 1 || T < 1 || Lmax < 0 || V < 2 || blank < 0 || blank >= V) return RNNT_ERR_ARG;
    if (sb < V || st < V) return RNNT_ERR_ARG;
    if (!(sb / T >= st) && !(st / B >= sb)) return RNNT_ERR_ARG;   // rows overlap: neither stride_b >= T stride_t nor stride_t >= B stride_b
    if (Lmax > SCORE_UMAX) return RNNT_ERR_SHAPE;
    if ((long long)B * T * (2 * Lmax + 1) >= 0x7fffffffLL) return RNNT_ERR_SHAPE;   // frame and state indices are ints
    for (int b = 0; b < B; ++b) {
        if (logit_lens[b] < 1 || logit_lens[b] > T || target_lens[b] < 0 || target_lens[b] > Lmax) return RNNT_ERR_ARG;
        for (int u = 0; u < target_lens[b]; ++u) {
            const int y = targets[(size_t)b * Lmax + u];
            if (y < 0 || y >= V || y == blank) return RNNT_ERR_ARG;
        }
    }
    return RNNT_OK;
}

// The caller's workspace, carved from a 16-byte aligned base: nll_beta [B, rounded up to even] f64 | alpha, beta [B][T][S1] f64 |
// pick, occ [B][T][L1] | lse [B][T] (floats) | lens [2][B] | targets [B][ts] | cnt [B] | cols [B][L1] | ptr [B][L1 + 1] | pos [B][S1]
// (ints), L1 = Lmax + 1, S1 = 2 Lmax + 1, ts = max(Lmax, 1).
struct CtcLossWork { double *nll_beta, *alpha, *beta; float *pick, *occ, *lse; int *lens, *tg, *cnt, *cols, *ptr, *pos; size_t ints, total; };
static CtcLossWork ctc_loss_work(void* base, size_t B, size_t T, size_t Lmax) {
    const size_t L1 = Lmax + 1, S1 = 2 * Lmax + 1, ts = Lmax > 0 ? Lmax : 1;
    Carve<double> d{(double*)base};
    CtcLossWork w;
    w.nll_beta = d.take(B + (B & 1));
    w.alpha = d.take(B * T * S1);
    w.beta = d.take(B * T * S1);
    Carve<float> f{base ? (float*)((double*)base + d.off) : nullptr};
    w.pick = f.take(B * T * L1);
    w.occ = f.take(B * T * L1);
    w.lse = f.take(B * T);
    Carve<int> i{base ? (int*)((float*)((double*)base + d.off) + f.off) : nullptr};
    w.lens = i.take(2 * B);
    w.tg = i.take(B * ts);
    w.cnt = i.take(B);
    w.cols = i.take(B * L1);
    w.ptr = i.take(B * (L1 + 1));
    w.pos = i.take(B * S1);
    w.ints = i.off;
    w.total = d.off * sizeof(double) + f.off * sizeof(float) + i.off * sizeof(int);
    return w;
}

int rnnt_ctc_loss_workspace(int32_t B, int32_t T, int32_t Lmax, int64_t* bytes_out) {
    if (!bytes_out || B < 1 || T < 1 || Lmax < 0) return RNNT_ERR_ARG;
    if (Lmax > SCORE_UMAX || (long long)B * T * (2 * Lmax + 1) >= 0x7fffffffLL) return RNNT_ERR_SHAPE;
    *bytes_out = (int64_t)ctc_loss_work(nullptr, B, T, Lmax).total;
    return RNNT_OK;
}

// The launches over elements E; the recursions and the occupancies between the two streaming passes do not see E.
// (The TAG_CTC_LOSS_* numbers of host_launch.hip.inc name them; without a context there is no rnnt_profile_begin to select one.)
extern "C++" template <typename E>
static void ctc_loss_launch(const CtcLossWork& w, const void* logits, long long sb, long long st, void* grad, int B, int T, int L1, int V, int ts,
                            int blank, int fused, double* nll, hipStream_t s) {
    const dim3 frames((unsigned)((B * T + 256 / CTC_LOSS_LANES - 1) / (256 / CTC_LOSS_LANES)));   // 16 frames each, no loop
    const E* x = (const E*)logits;
    E* g = (E*)grad;
    const int both = g != nullptr;
    hipLaunchKernelGGL((ctc_loss_pick<E>), frames, dim3(256), 0, s, x, sb, st, w.tg, w.lens, B, T, L1, V, ts, blank, fused, w.lse, w.pick);   // TAG_CTC_LOSS_PICK
    hipLaunchKernelGGL(ctc_alpha_beta, dim3(both ? 2 * B : B), dim3(512), 0, s, w.pick, w.tg, w.lens, B, T, L1, ts, both, w.alpha, w.beta, nll,
                       w.nll_beta);                                                                                                             // TAG_CTC_LOSS_RECURSION
    if (g) {
        hipLaunchKernelGGL(ctc_loss_occ, dim3((unsigned)grid_for((long long)B * T * L1)), dim3(256), 0, s, w.pick, w.alpha, w.beta, nll, w.lens, w.cnt,
                           w.ptr, w.pos, B, T, L1, w.occ);                                                                                      // TAG_CTC_LOSS_OCC
        if (fused) hipLaunchKernelGGL((ctc_loss_grad<E, true>), frames, dim3(256), 0, s, x, sb, st, w.lens, w.cnt, w.cols, w.lse, w.occ, nll, B, T, L1, V, g);
        else hipLaunchKernelGGL((ctc_loss_grad<E, false>), frames, dim3(256), 0, s, x, sb, st, w.lens, w.cnt, w.cols, w.lse, w.occ, nll, B, T, L1, V, g);   // TAG_CTC_LOSS_GRAD
    }
}

// A row's entries: its distinct columns in ascending order (the blank and every distinct label) with the extended states on each,
// ascending.  n entries; cols [n], ptr [n + 1], pos [2 L + 1].
static int ctc_loss_entries(const int32_t* y, int L, int blank, int* cols, int* ptr, int* pos) {
    std::vector<int> order(L);
    for (int i = 0; i < L; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return y[a] < y[b]; });   // by label; equal labels keep their order
    int n = 0, np = 0, i = 0;
    bool blank_done = false;
    auto put_blank = [&]() {
        cols[n] = blank;
        ptr[n++] = np;
        for (int k = 0; k <= L; ++k) pos[np++] = 2 * k;
        blank_done = true;
    };
    while (i < L) {
        const int c = y[order[i]];
        if (!blank_done && blank < c) put_blank();
        cols[n] = c;
        ptr[n++] = np;
        for (; i < L && y[order[i]] == c; ++i) pos[np++] = 2 * order[i] + 1;
    }
    if (!blank_done) put_blank();
    ptr[n] = np;
    return n;
}

#define CTC_HIPCHK(expr)                            \
    do {                                            \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

int rnnt_ctc_loss_elem(const void* logits_dev, int64_t stride_b, int64_t stride_t, const int32_t* targets_host, const int32_t* logit_lens_host,
                       const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V, int32_t blank, int32_t elem,
                       int32_t fused_log_softmax, double* nll_dev, void* grad_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    int rc;
    if (elem != RNNT_LOSS_F32 && elem != RNNT_LOSS_BF16 && elem != RNNT_LOSS_F16) return RNNT_ERR_ARG;   // before any pointer is followed
    if ((rc = ctc_loss_check(logits_dev, stride_b, stride_t, targets_host, logit_lens_host, target_lens_host, B, T, Lmax, V, blank, nll_dev))) return rc;
    if (!workspace_dev || ((uintptr_t)logits_dev | (uintptr_t)grad_dev | (uintptr_t)workspace_dev) & 15 || (uintptr_t)nll_dev & 7) return RNNT_ERR_ARG;
    const int L1 = Lmax + 1, S1 = 2 * Lmax + 1, ts = Lmax > 0 ? Lmax : 1;
    const CtcLossWork w = ctc_loss_work(workspace_dev, B, T, Lmax);
    if (workspace_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    // lens | targets | entry tables in ONE copy; what lies beyond a row's length or its entries is the blank / 0: never used
    std::vector<int> host(w.ints, 0);
    int *tg = host.data() + (w.tg - w.lens), *cnt = host.data() + (w.cnt - w.lens), *cols = host.data() + (w.cols - w.lens),
        *ptr = host.data() + (w.ptr - w.lens), *pos = host.data() + (w.pos - w.lens);
    for (int b = 0; b < B; ++b) {
        const int Lb = target_lens_host[b];
        host[b] = logit_lens_host[b];
        host[B + b] = Lb;
        for (int u = 0; u < ts; ++u) tg[(size_t)b * ts + u] = u < Lb ? targets_host[(size_t)b * Lmax + u] : blank;
        cnt[b] = ctc_loss_entries(targets_host + (size_t)b * Lmax, Lb, blank, cols + (size_t)b * L1, ptr + (size_t)b * (L1 + 1), pos + (size_t)b * S1);
    }
    // (pageable source: the runtime has taken the bytes when the call returns, so `host` may go; what follows is launches only)
    CTC_HIPCHK(hipMemcpyAsync(w.lens, host.data(), w.ints * sizeof(int), hipMemcpyHostToDevice, s));
    const int fused = fused_log_softmax != 0;
    if (elem == RNNT_LOSS_F32) ctc_loss_launch<float>(w, logits_dev, stride_b, stride_t, grad_dev, B, T, L1, V, ts, blank, fused, nll_dev, s);
    else if (elem == RNNT_LOSS_BF16) ctc_loss_launch<loss_bf16>(w, logits_dev, stride_b, stride_t, grad_dev, B, T, L1, V, ts, blank, fused, nll_dev, s);
    else ctc_loss_launch<loss_f16>(w, logits_dev, stride_b, stride_t, grad_dev, B, T, L1, V, ts, blank, fused, nll_dev, s);
    CTC_HIPCHK(hipGetLastError());
    return RNNT_OK;
}
#undef CTC_HIPCHK

int rnnt_ctc_loss(const float* logits_dev, int64_t stride_b, int64_t stride_t, const int32_t* targets_host, const int32_t* logit_lens_host,
                  const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V, int32_t blank, int32_t fused_log_softmax,
                  double* nll_dev, float* grad_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    return rnnt_ctc_loss_elem(logits_dev, stride_b, stride_t, targets_host, logit_lens_host, target_lens_host, B, T, Lmax, V, blank, RNNT_LOSS_F32,
                              fused_log_softmax, nll_dev, grad_dev, workspace_dev, workspace_bytes, stream);
}

// The same loss in plain C++ (no GPU): f64 throughout over float logits, row by row, with ctc_alpha_beta's two recursions.
int rnnt_ctc_loss_host(const float* logits_host, int64_t stride_b, int64_t stride_t, const int32_t* targets_host, const int32_t* logit_lens_host,
                       const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V, int32_t blank, int32_t fused_log_softmax,
                       double* nll_host, double* grad_host) {
    int rc;
    if ((rc = ctc_loss_check(logits_host, stride_b, stride_t, targets_host, logit_lens_host, target_lens_host, B, T, Lmax, V, blank, nll_host))) return rc;
    const double ninf = -INFINITY;
    auto lse3 = [](double a, double a1, double a2) {
        double mx = std::max(a, std::max(a1, a2));
        if (mx == -INFINITY) mx = 0.0;
        return log(exp(a - mx) + exp(a1 - mx) + exp(a2 - mx)) + mx;
    };
    auto lae = [](double x, double y) {
        const double mx = std::max(x, y), mn = std::min(x, y);
        return mx == -INFINITY ? mx : mx + log1p(exp(mn - mx));
    };
    std::vector<double> lse(T), lp, al, be;
    std::vector<int> ext;
    for (int b = 0; b < B; ++b) {
        const int Tb = logit_lens_host[b], Lb = target_lens_host[b], S = 2 * Lb + 1;
        const float* xb = logits_host + (size_t)b * stride_b;
        const int32_t* yb = targets_host + (size_t)b * Lmax;
        ext.assign(S, blank);
        for (int i = 0; i < Lb; ++i) ext[2 * i + 1] = yb[i];
        auto skip = [&](int s, int s2) { return (s & 1) && s2 >= 0 && s2 < S && ext[s2] != ext[s]; };   // a move of two states between s and s2
        lp.assign((size_t)Tb * S, 0.0);
        al.assign((size_t)Tb * S, ninf);
        be.assign((size_t)Tb * S, ninf);
        for (int t = 0; t < Tb; ++t) {
            const float* x = xb + (size_t)t * stride_t;
            double l = 0.0;
            if (fused_log_softmax) {
                double mx = ninf, sum = 0.0;
                for (int k = 0; k < V; ++k) mx = std::max(mx, (double)x[k]);
                for (int k = 0; k < V; ++k) sum += exp((double)x[k] - mx);
                l = mx + log(sum);
            }
            lse[t] = l;
            for (int s = 0; s < S; ++s) lp[(size_t)t * S + s] = (double)x[ext[s]] - l;
        }
        for (int s = 0; s < S && s < 2; ++s) al[s] = lp[s];
        for (int t = 1; t < Tb; ++t)
            for (int s = 0; s < S; ++s) {
                const double* pv = &al[(size_t)(t - 1) * S];
                al[(size_t)t * S + s] = lse3(pv[s], s >= 1 ? pv[s - 1] : ninf, skip(s, s - 2) ? pv[s - 2] : ninf) + lp[(size_t)t * S + s];
            }
        for (int s = std::max(S - 2, 0); s < S; ++s) be[(size_t)(Tb - 1) * S + s] = lp[(size_t)(Tb - 1) * S + s];
        for (int t = Tb - 2; t >= 0; --t)
            for (int s = 0; s < S; ++s) {
                const double* pv = &be[(size_t)(t + 1) * S];
                be[(size_t)t * S + s] = lse3(pv[s], s + 1 < S ? pv[s + 1] : ninf, skip(s, s + 2) ? pv[s + 2] : ninf) + lp[(size_t)t * S + s];
            }
        const double* fin = &al[(size_t)(Tb - 1) * S];
        const double nll = -lae(fin[S - 1], S > 1 ? fin[S - 2] : ninf);
        nll_host[b] = nll;
        if (!grad_host) continue;
        double* gb = grad_host + (size_t)b * stride_b;
        for (int t = 0; t < T; ++t) {
            double* g = gb + (size_t)t * stride_t;
            std::fill(g, g + V, 0.0);
            if (t >= Tb || !(nll < INFINITY)) continue;
            const float* x = xb + (size_t)t * stride_t;
            if (fused_log_softmax)
                for (int k = 0; k < V; ++k) g[k] = exp((double)x[k] - lse[t]);
            for (int s = 0; s < S; ++s) {                      // ascending states: the order ctc_loss_occ adds a column's in
                const double ab = al[(size_t)t * S + s] + be[(size_t)t * S + s];
                if (ab > ninf) g[ext[s]] -= exp(ab - lp[(size_t)t * S + s] + nll);
            }
        }
    }
    return RNNT_OK;
}
