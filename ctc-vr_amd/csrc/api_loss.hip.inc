// C ABI: the transducer loss with its gradient over a caller's joint lattice (torchaudio.functional.rnnt_loss), and its pure C++
// twin.  No context: a loss needs no weights and no model, so refusals are status codes without a message.
// rnnt_transducer_loss_elem is the device entry point for float, bfloat16 and float16 lattices; rnnt_transducer_loss is its float case.
// Included by rnnt_api.hip inside extern "C" (the one template, loss_launch, steps out of it).  Kernels: rnnt_loss.hip.h.

// lengths and labels of a loss call, checked on the host before anything is launched or written
static int loss_check(const void* logits, const int32_t* targets, const int32_t* logit_lens, const int32_t* target_lens, int32_t B, int32_t T,
                      int32_t Umax, int32_t V, int32_t blank, const void* nll) {
    if (!logits || !logit_lens || !target_lens || !nll || (Umax > 0 && !targets)) return RNNT_ERR_ARG;
    if (B < 1 || T < 1 || Umax < 0 || V < 2 || blank < 0 || blank >= V) return RNNT_ERR_ARG;
    if (Umax > SCORE_UMAX) return RNNT_ERR_SHAPE;
    if ((long long)B * T * (Umax + 1) >= 0x7fffffffLL) return RNNT_ERR_SHAPE;   // cell indices are ints
    for (int b = 0; b < B; ++b) {
        if (logit_lens[b] < 1 || logit_lens[b] > T || target_lens[b] < 0 || target_lens[b] > Umax) return RNNT_ERR_ARG;
        for (int u = 0; u < target_lens[b]; ++u) {
            const int y = targets[(size_t)b * Umax + u];
            if (y < 0 || y >= V || y == blank) return RNNT_ERR_ARG;
        }
    }
    return RNNT_OK;
}

// The caller's workspace, carved from a 16-byte aligned base: nll_alpha [B, rounded up to even] f64 | alpha, beta [B][T][U1] f64 |
// coef [B][T][U1][4] (first among the floats, so its float4s stay aligned) | pick [B][T][U1][2] | lse [B][T][U1] (floats) |
// lens [2][B] | targets [B][ts] (ints), ts = max(U1 - 1, 1).
struct LossWork { double *nll_alpha, *alpha, *beta; float *coef, *pick, *lse; int *lens, *tg; size_t ints, total; };
static LossWork loss_work(void* base, size_t B, size_t T, size_t U1) {
    const size_t cells = B * T * U1, ts = U1 > 1 ? U1 - 1 : 1;
    Carve<double> d{(double*)base};
    LossWork w;
    w.nll_alpha = d.take(B + (B & 1));
    w.alpha = d.take(cells);
    w.beta = d.take(cells);
    Carve<float> f{base ? (float*)((double*)base + d.off) : nullptr};
    w.coef = f.take(4 * cells);
    w.pick = f.take(2 * cells);
    w.lse = f.take(cells);
    Carve<int> i{base ? (int*)(w.lse + cells) : nullptr};
    w.lens = i.take(2 * B);
    w.tg = i.take(B * ts);
    w.ints = i.off;
    w.total = d.off * sizeof(double) + f.off * sizeof(float) + i.off * sizeof(int);
    return w;
}

int rnnt_transducer_loss_workspace(int32_t B, int32_t T, int32_t U1, int64_t* bytes_out) {
    if (!bytes_out || B < 1 || T < 1 || U1 < 1) return RNNT_ERR_ARG;
    if (U1 > SCORE_UMAX + 1 || (long long)B * T * U1 >= 0x7fffffffLL) return RNNT_ERR_SHAPE;
    *bytes_out = (int64_t)loss_work(nullptr, B, T, U1).total;
    return RNNT_OK;
}

#define LOSS_HIPCHK(expr)                           \
    do {                                            \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

// The two lattice passes over elements E, with LP and LG lanes per cell; the recursions and the factors between them do not see E.
extern "C++" template <typename E, int LP, int LG>
static void loss_launch(const LossWork& w, const void* logits, void* grad, int B, int T, int U1, int V, int ts, int blank, int fused, float clamp,
                        double* nll, hipStream_t s) {
    const int ncell = B * T * U1;
    const dim3 pick((unsigned)((ncell + 256 / LP - 1) / (256 / LP))), lattice((unsigned)((ncell + 256 / LG - 1) / (256 / LG)));   // 256 / L cells each, no loop
    const dim3 cells((unsigned)grid_for(ncell));
    const E* x = (const E*)logits;
    E* g = (E*)grad;
    hipLaunchKernelGGL((loss_pick<E, LP>), pick, dim3(256), 0, s, x, w.tg, w.lens, B, T, U1, V, ts, blank, fused, w.lse, w.pick);
    hipLaunchKernelGGL(transducer_alpha_beta, dim3(2 * B), dim3(256), 0, s, w.pick, w.lens, B, T, U1, w.alpha, w.beta, w.nll_alpha, nll);
    if (g) {
        hipLaunchKernelGGL(loss_coef, cells, dim3(256), 0, s, w.pick, w.lse, w.alpha, w.beta, w.lens, B, T, U1, fused, w.coef);
        if (fused) hipLaunchKernelGGL((loss_grad<E, LG, true>), lattice, dim3(256), 0, s, x, w.tg, w.lens, w.coef, B, T, U1, V, ts, blank, clamp, g);
        else hipLaunchKernelGGL((loss_grad<E, LG, false>), lattice, dim3(256), 0, s, x, w.tg, w.lens, w.coef, B, T, U1, V, ts, blank, clamp, g);
    }
}

int rnnt_transducer_loss_elem(const void* logits_dev, const int32_t* targets_host, const int32_t* logit_lens_host, const int32_t* target_lens_host,
                              int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank, int32_t elem, int32_t fused_log_softmax, float clamp,
                              double* nll_dev, void* grad_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    int rc;
    if (elem != RNNT_LOSS_F32 && elem != RNNT_LOSS_BF16 && elem != RNNT_LOSS_F16) return RNNT_ERR_ARG;   // before any pointer is followed
    if ((rc = loss_check(logits_dev, targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, nll_dev))) return rc;
    if (!workspace_dev || ((uintptr_t)logits_dev | (uintptr_t)grad_dev | (uintptr_t)workspace_dev) & 15) return RNNT_ERR_ARG;
    const int U1 = Umax + 1, ts = Umax > 0 ? Umax : 1;
    const LossWork w = loss_work(workspace_dev, B, T, U1);
    if (workspace_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    // lens | targets in ONE copy; entries beyond a row's length become the blank: they are neither validated nor used
    std::vector<int> host(w.ints, blank);
    for (int b = 0; b < B; ++b) {
        host[b] = logit_lens_host[b];
        host[B + b] = target_lens_host[b];
        for (int u = 0; u < target_lens_host[b]; ++u) host[2 * (size_t)B + (size_t)b * ts + u] = targets_host[(size_t)b * Umax + u];
    }
    // (pageable source: the runtime has taken the bytes when the call returns, so `host` may go; what follows is launches only)
    LOSS_HIPCHK(hipMemcpyAsync(w.lens, host.data(), w.ints * sizeof(int), hipMemcpyHostToDevice, s));
    const int fused = fused_log_softmax != 0;
    if (elem == RNNT_LOSS_F32) loss_launch<float, LOSS_LANES, LOSS_LANES>(w, logits_dev, grad_dev, B, T, U1, V, ts, blank, fused, clamp, nll_dev, s);
    else if (elem == RNNT_LOSS_BF16) loss_launch<loss_bf16, LOSS_LANES_16BIT_PICK, LOSS_LANES_16BIT_GRAD>(w, logits_dev, grad_dev, B, T, U1, V, ts, blank, fused, clamp, nll_dev, s);
    else loss_launch<loss_f16, LOSS_LANES_16BIT_PICK, LOSS_LANES_16BIT_GRAD>(w, logits_dev, grad_dev, B, T, U1, V, ts, blank, fused, clamp, nll_dev, s);
    LOSS_HIPCHK(hipGetLastError());
    return RNNT_OK;
}

int rnnt_transducer_loss(const float* logits_dev, const int32_t* targets_host, const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B,
                         int32_t T, int32_t Umax, int32_t V, int32_t blank, int32_t fused_log_softmax, float clamp, double* nll_dev, float* grad_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream) {
    return rnnt_transducer_loss_elem(logits_dev, targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, RNNT_LOSS_F32, fused_log_softmax,
                                     clamp, nll_dev, grad_dev, workspace_dev, workspace_bytes, stream);
}
#undef LOSS_HIPCHK

// The same loss in plain C++ (no GPU): f64 throughout over logits of type X (float: rnnt_transducer_loss_host; double: the lattice
// rnnt_joint_loss_host forms for itself), row by row.
extern "C++" template <typename X>
static int loss_host_rows(const X* logits_host, const int32_t* targets_host, const int32_t* logit_lens_host, const int32_t* target_lens_host,
                          int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank, int32_t fused_log_softmax, float clamp, double* nll_host,
                          double* grad_host) {
    int rc;
    if ((rc = loss_check(logits_host, targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, nll_host))) return rc;
    const int U1 = Umax + 1;
    const size_t cells = (size_t)T * U1;
    const double ninf = -INFINITY;
    auto lae = [](double x, double y) {
        const double mx = std::max(x, y), mn = std::min(x, y);
        return mx == -INFINITY ? mx : mx + log1p(exp(mn - mx));
    };
    std::vector<double> lse(cells), pb(cells), pl(cells), al(cells), be(cells);
    for (int b = 0; b < B; ++b) {
        const int Tb = logit_lens_host[b], Ub = target_lens_host[b];
        const X* lb = logits_host + (size_t)b * cells * V;
        const int32_t* yb = targets_host + (size_t)b * Umax;
        auto at = [&](int t, int u) { return (size_t)t * U1 + u; };
        for (int t = 0; t < Tb; ++t)
            for (int u = 0; u <= Ub; ++u) {
                const X* x = lb + at(t, u) * V;
                double l = 0.0;
                if (fused_log_softmax) {
                    double mx = ninf, sum = 0.0;
                    for (int k = 0; k < V; ++k) mx = std::max(mx, (double)x[k]);
                    for (int k = 0; k < V; ++k) sum += exp((double)x[k] - mx);
                    l = mx + log(sum);
                }
                lse[at(t, u)] = l;
                pb[at(t, u)] = (double)x[blank] - l;
                pl[at(t, u)] = u < Ub ? (double)x[yb[u]] - l : ninf;
            }
        for (int t = 0; t < Tb; ++t)
            for (int u = 0; u <= Ub; ++u) {
                if (t == 0 && u == 0) { al[0] = 0.0; continue; }
                const double below = t > 0 ? al[at(t - 1, u)] + pb[at(t - 1, u)] : ninf, left = u > 0 ? al[at(t, u - 1)] + pl[at(t, u - 1)] : ninf;
                al[at(t, u)] = lae(below, left);
            }
        for (int t = Tb - 1; t >= 0; --t)
            for (int u = Ub; u >= 0; --u) {
                if (t == Tb - 1 && u == Ub) { be[at(t, u)] = pb[at(t, u)]; continue; }
                const double up = t + 1 < Tb ? be[at(t + 1, u)] + pb[at(t, u)] : ninf, right = u < Ub ? be[at(t, u + 1)] + pl[at(t, u)] : ninf;
                be[at(t, u)] = lae(up, right);
            }
        const double logZ = be[0];
        nll_host[b] = -logZ;
        if (!grad_host) continue;
        double* gb = grad_host + (size_t)b * cells * V;
        for (int t = 0; t < T; ++t)
            for (int u = 0; u < U1; ++u) {
                double* g = gb + at(t, u) * V;
                if (t >= Tb || u > Ub) {
                    std::fill(g, g + V, 0.0);
                    continue;
                }
                const size_t c = at(t, u);
                const X* x = lb + c * V;
                const double occ = exp(al[c] + be[c] - logZ);
                double tb = 0.0, tl = 0.0;
                if (t < Tb - 1) tb = exp(al[c] + pb[c] + be[at(t + 1, u)] - logZ);
                else if (u == Ub) tb = exp(al[c] + pb[c] - logZ);
                if (u < Ub) tl = exp(al[c] + pl[c] + be[at(t, u + 1)] - logZ);
                for (int k = 0; k < V; ++k) {
                    double v = fused_log_softmax ? exp((double)x[k] - lse[c]) * occ : 0.0;
                    if (k == blank) v -= tb;
                    if (u < Ub && k == yb[u]) v -= tl;
                    if (clamp > 0.0f) v = std::min(std::max(v, -(double)clamp), (double)clamp);
                    g[k] = v;
                }
            }
    }
    return RNNT_OK;
}

int rnnt_transducer_loss_host(const float* logits_host, const int32_t* targets_host, const int32_t* logit_lens_host, const int32_t* target_lens_host,
                              int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank, int32_t fused_log_softmax, float clamp, double* nll_host,
                              double* grad_host) {
    return loss_host_rows<float>(logits_host, targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, fused_log_softmax, clamp, nll_host,
                                 grad_host);
}
