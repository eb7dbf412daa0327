// C ABI: the predictor's LSTM layer over a whole label sequence with gradients -- forward, back-propagation through time, and the
// plain C++ float64 twin of both.  No context, like the loss calls: the caller brings weights (torch.nn.LSTM layout), workspace and
// state; refusals are status codes, decided on the host before anything is launched or written.
// Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_lstm.hip.h.

static int lstm_shape_check(int32_t B, int32_t U1) {
    if (B < 1 || U1 < 1) return RNNT_ERR_ARG;
    if (U1 > SCORE_UMAX + 1) return RNNT_ERR_SHAPE;
    if ((long long)B * U1 * LSTM_STATE >= 0x7fffffffLL) return RNNT_ERR_SHAPE;   // row and element indices are ints
    return RNNT_OK;
}
static int lstm_lens_check(const int32_t* lens, int32_t B, int32_t U1) {
    for (int b = 0; lens && b < B; ++b)
        if (lens[b] < 1 || lens[b] > U1) return RNNT_ERR_ARG;
    return RNNT_OK;
}

// The caller's workspace from a 16-byte aligned base, in floats: lens [B rounded up to 4] (ints) | whh_il [256][256][4] |
// xg (forward) or dG (backward) [B U1][1024] | dW_ih slabs [KS][1024][256] | dW_hh slabs [KS][1024][256] | db slabs [KS][1024],
// KS = ceil(B U1 / 256).
struct LstmWork { int* lens; float *whh_il, *g, *dwih_part, *dwhh_part, *db_part; int KS; size_t total; };
static LstmWork lstm_work(void* base, size_t B, size_t U1) {
    Carve<float> f{(float*)base};
    LstmWork w;
    w.KS = (int)((B * U1 + LSTM_KSLAB - 1) / LSTM_KSLAB);
    w.lens = (int*)f.take((B + 3) / 4 * 4);
    w.whh_il = f.take((size_t)LSTM_GATES * LSTM_HID);
    w.g = f.take(B * U1 * LSTM_GATES);
    w.dwih_part = f.take((size_t)w.KS * LSTM_GATES * LSTM_HID);
    w.dwhh_part = f.take((size_t)w.KS * LSTM_GATES * LSTM_HID);
    w.db_part = f.take((size_t)w.KS * LSTM_GATES);
    w.total = f.off * sizeof(float);
    return w;
}

int rnnt_lstm_workspace(int32_t B, int32_t U1, int64_t* work_bytes, int64_t* state_bytes) {
    if (!work_bytes || !state_bytes) return RNNT_ERR_ARG;
    if (int rc = lstm_shape_check(B, U1)) return rc;
    *work_bytes = (int64_t)lstm_work(nullptr, B, U1).total;
    *state_bytes = (int64_t)B * U1 * LSTM_STATE * (int64_t)sizeof(float);
    return RNNT_OK;
}

#define LSTM_HIPCHK(expr)                              \
    do {                                               \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

// the LDS the two recurrence kernels may ask for, settled on the first call per device (as joint_device does)
static int lstm_device() {
    static std::atomic<int> ready[64];
    int dev = 0;
    LSTM_HIPCHK(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && ready[dev].load()) return RNNT_OK;
    LSTM_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_seq_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, LSTM_FWD_LDS));
    LSTM_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&lstm_seq_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, LSTM_BWD_LDS));
    if (dev >= 0 && dev < 64) ready[dev].store(1);
    return RNNT_OK;
}

static int lstm_send_lens(const LstmWork& w, const int32_t* lens_host, int B, int U1, hipStream_t s) {
    std::vector<int> host((size_t)B);
    for (int b = 0; b < B; ++b) host[b] = lens_host ? lens_host[b] : U1;
    // (pageable source: the runtime has taken the bytes when the call returns; what follows is launches only)
    LSTM_HIPCHK(hipMemcpyAsync(w.lens, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return RNNT_OK;
}

int rnnt_lstm_forward(const float* x_dev, const float* w_ih_dev, const float* w_hh_dev, const float* b_ih_dev, const float* b_hh_dev,
                      const float* h0_dev, const float* c0_dev, const int32_t* lens_host, int32_t B, int32_t U1, float* out_dev, float* hn_dev,
                      float* cn_dev, void* state_dev, int64_t state_bytes, void* work_dev, int64_t work_bytes, void* stream) {
    if (!x_dev || !w_ih_dev || !w_hh_dev || !b_ih_dev || !b_hh_dev || !out_dev || !work_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)x_dev | (uintptr_t)w_ih_dev | (uintptr_t)w_hh_dev | (uintptr_t)b_ih_dev | (uintptr_t)b_hh_dev | (uintptr_t)h0_dev | (uintptr_t)c0_dev |
         (uintptr_t)out_dev | (uintptr_t)hn_dev | (uintptr_t)cn_dev | (uintptr_t)state_dev | (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc;
    if ((rc = lstm_shape_check(B, U1))) return rc;
    if ((rc = lstm_lens_check(lens_host, B, U1))) return rc;
    const LstmWork w = lstm_work(work_dev, B, U1);
    if (work_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    if (state_dev && state_bytes < (int64_t)B * U1 * LSTM_STATE * (int64_t)sizeof(float)) return RNNT_ERR_SHAPE;
    if ((rc = lstm_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lstm_send_lens(w, lens_host, B, U1, s))) return rc;
    const int M = B * U1;
    hipLaunchKernelGGL(lstm_pack_whh, dim3(LSTM_HID * LSTM_HID / 256), dim3(256), 0, s, w_hh_dev, w.whh_il);
    LstmGemmP g;
    memset(&g, 0, sizeof(g));
    g.a = x_dev; g.b = w_ih_dev; g.bias = b_ih_dev; g.bias2 = b_hh_dev; g.lens = w.lens; g.c = w.g; g.M = M; g.N = LSTM_GATES; g.K = LSTM_HID; g.U1 = U1;
    hipLaunchKernelGGL((lstm_gemm<0>), dim3(LSTM_GATES / 64, (unsigned)((M + 63) / 64)), dim3(256), 0, s, g);
    LstmP p;
    memset(&p, 0, sizeof(p));
    p.xg = w.g; p.whh_il = w.whh_il; p.h0 = h0_dev; p.c0 = c0_dev; p.lens = w.lens; p.out = out_dev; p.hn = hn_dev; p.cn = cn_dev;
    p.state = (float*)state_dev; p.B = B; p.U1 = U1;
    hipLaunchKernelGGL(lstm_seq_fwd, dim3((unsigned)((B + LSTM_ROWS - 1) / LSTM_ROWS)), dim3(LSTM_THREADS), LSTM_FWD_LDS, s, p);
    LSTM_HIPCHK(hipGetLastError());
    return RNNT_OK;
}

int rnnt_lstm_backward(const float* x_dev, const float* w_ih_dev, const float* w_hh_dev, const float* h0_dev, const float* c0_dev, const float* out_dev,
                       const void* state_dev, int64_t state_bytes, const float* dout_dev, const int32_t* lens_host, int32_t B, int32_t U1, float* dx_dev,
                       float* dw_ih_dev, float* dw_hh_dev, float* db_dev, float* dh0_dev, float* dc0_dev, void* work_dev, int64_t work_bytes, void* stream) {
    if (!x_dev || !w_ih_dev || !w_hh_dev || !out_dev || !state_dev || !dout_dev || !dx_dev || !dw_ih_dev || !dw_hh_dev || !db_dev || !work_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)x_dev | (uintptr_t)w_ih_dev | (uintptr_t)w_hh_dev | (uintptr_t)h0_dev | (uintptr_t)c0_dev | (uintptr_t)out_dev | (uintptr_t)state_dev |
         (uintptr_t)dout_dev | (uintptr_t)dx_dev | (uintptr_t)dw_ih_dev | (uintptr_t)dw_hh_dev | (uintptr_t)db_dev | (uintptr_t)dh0_dev | (uintptr_t)dc0_dev |
         (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc;
    if ((rc = lstm_shape_check(B, U1))) return rc;
    if ((rc = lstm_lens_check(lens_host, B, U1))) return rc;
    const LstmWork w = lstm_work(work_dev, B, U1);
    if (work_bytes < (int64_t)w.total || state_bytes < (int64_t)B * U1 * LSTM_STATE * (int64_t)sizeof(float)) return RNNT_ERR_SHAPE;
    if ((rc = lstm_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = lstm_send_lens(w, lens_host, B, U1, s))) return rc;
    const int M = B * U1;
    LstmP p;
    memset(&p, 0, sizeof(p));
    p.w_hh = w_hh_dev; p.c0 = c0_dev; p.dout = dout_dev; p.lens = w.lens; p.state = (float*)const_cast<void*>(state_dev); p.dg = w.g;
    p.dh0 = dh0_dev; p.dc0 = dc0_dev; p.B = B; p.U1 = U1;
    hipLaunchKernelGGL(lstm_seq_bwd, dim3((unsigned)((B + LSTM_ROWS - 1) / LSTM_ROWS)), dim3(LSTM_THREADS), LSTM_BWD_LDS, s, p);
    LstmGemmP g;
    memset(&g, 0, sizeof(g));
    g.a = w.g; g.b = w_ih_dev; g.lens = w.lens; g.c = dx_dev; g.M = M; g.N = LSTM_HID; g.K = LSTM_GATES; g.U1 = U1;
    hipLaunchKernelGGL((lstm_gemm<1>), dim3(LSTM_HID / 64, (unsigned)((M + 63) / 64)), dim3(256), 0, s, g);
    g.M = LSTM_GATES; g.K = M; g.kslab = LSTM_KSLAB;
    g.b = x_dev; g.c = w.dwih_part;
    hipLaunchKernelGGL((lstm_gemm<2>), dim3(LSTM_HID / 64, LSTM_GATES / 64, (unsigned)w.KS), dim3(256), 0, s, g);
    g.b = out_dev; g.h0 = h0_dev; g.c = w.dwhh_part;
    hipLaunchKernelGGL((lstm_gemm<3>), dim3(LSTM_HID / 64, LSTM_GATES / 64, (unsigned)w.KS), dim3(256), 0, s, g);
    hipLaunchKernelGGL(lstm_db_part, dim3(LSTM_GATES / 256, (unsigned)w.KS), dim3(256), 0, s, w.g, M, w.db_part);
    const long long w4 = (long long)LSTM_GATES * LSTM_HID / 4;
    hipLaunchKernelGGL(lstm_slab_reduce, dim3((unsigned)((w4 + 255) / 256)), dim3(256), 0, s, w.dwih_part, w.KS, w4, dw_ih_dev);
    hipLaunchKernelGGL(lstm_slab_reduce, dim3((unsigned)((w4 + 255) / 256)), dim3(256), 0, s, w.dwhh_part, w.KS, w4, dw_hh_dev);
    hipLaunchKernelGGL(lstm_slab_reduce, dim3(1), dim3(256), 0, s, w.db_part, w.KS, (long long)LSTM_GATES / 4, db_dev);
    LSTM_HIPCHK(hipGetLastError());
    return RNNT_OK;
}
#undef LSTM_HIPCHK

// Both directions in plain C++ (no GPU): f64 throughout over the float32 inputs, step by step.  dout_host null: forward only.
int rnnt_lstm_host(const float* x_host, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host, const float* b_hh_host, const float* h0_host,
                   const float* c0_host, const int32_t* lens_host, int32_t B, int32_t U1, const float* dout_host, double* out_host, double* hn_host,
                   double* cn_host, double* dx_host, double* dw_ih_host, double* dw_hh_host, double* db_host, double* dh0_host, double* dc0_host) {
    if (!x_host || !w_ih_host || !w_hh_host || !b_ih_host || !b_hh_host || !out_host) return RNNT_ERR_ARG;
    if (dout_host && (!dx_host || !dw_ih_host || !dw_hh_host || !db_host)) return RNNT_ERR_ARG;
    int rc;
    if ((rc = lstm_shape_check(B, U1))) return rc;
    if ((rc = lstm_lens_check(lens_host, B, U1))) return rc;
    const size_t H = LSTM_HID, G = LSTM_GATES;
    std::vector<double> wih(G * H), whh(G * H), bias(G), st((size_t)U1 * LSTM_STATE), hp((size_t)U1 * H), pre(G), dg(G), dh(H), dc(H), dhn(H);
    for (size_t k = 0; k < G * H; ++k) { wih[k] = (double)w_ih_host[k]; whh[k] = (double)w_hh_host[k]; }
    for (size_t n = 0; n < G; ++n) bias[n] = (double)b_ih_host[n] + (double)b_hh_host[n];
    auto sig = [](double v) { return 1.0 / (1.0 + exp(-v)); };
    std::fill(out_host, out_host + (size_t)B * U1 * H, 0.0);
    if (dout_host) {
        std::fill(dx_host, dx_host + (size_t)B * U1 * H, 0.0);
        std::fill(dw_ih_host, dw_ih_host + G * H, 0.0);
        std::fill(dw_hh_host, dw_hh_host + G * H, 0.0);
        std::fill(db_host, db_host + G, 0.0);
    }
    for (int b = 0; b < B; ++b) {
        const int len = lens_host ? lens_host[b] : U1;
        std::vector<double> h(H, 0.0), c(H, 0.0);
        for (size_t j = 0; j < H; ++j) {
            if (h0_host) h[j] = (double)h0_host[(size_t)b * H + j];
            if (c0_host) c[j] = (double)c0_host[(size_t)b * H + j];
        }
        const std::vector<double> cfirst = c;
        for (int u = 0; u < len; ++u) {
            const float* xr = x_host + ((size_t)b * U1 + u) * H;
            double* s = st.data() + (size_t)u * LSTM_STATE;
            for (size_t j = 0; j < H; ++j) hp[(size_t)u * H + j] = h[j];
            for (size_t n = 0; n < G; ++n) {
                double a = bias[n];
                const double *wi = wih.data() + n * H, *wh = whh.data() + n * H;
                for (size_t k = 0; k < H; ++k) a += (double)xr[k] * wi[k];
                for (size_t k = 0; k < H; ++k) a += h[k] * wh[k];
                pre[n] = a;
            }
            for (size_t j = 0; j < H; ++j) {
                const double gi = sig(pre[j]), gf = sig(pre[H + j]), gg = tanh(pre[2 * H + j]), go = sig(pre[3 * H + j]);
                c[j] = gf * c[j] + gi * gg;
                h[j] = go * tanh(c[j]);
                s[j] = gi; s[H + j] = gf; s[2 * H + j] = gg; s[3 * H + j] = go; s[4 * H + j] = c[j];
                out_host[((size_t)b * U1 + u) * H + j] = h[j];
            }
        }
        for (size_t j = 0; j < H; ++j) {
            if (hn_host) hn_host[(size_t)b * H + j] = h[j];
            if (cn_host) cn_host[(size_t)b * H + j] = c[j];
        }
        if (!dout_host) continue;
        std::fill(dh.begin(), dh.end(), 0.0);
        std::fill(dc.begin(), dc.end(), 0.0);
        for (int u = len - 1; u >= 0; --u) {
            const double* s = st.data() + (size_t)u * LSTM_STATE;
            const float* go_ = dout_host + ((size_t)b * U1 + u) * H;
            const float* xr = x_host + ((size_t)b * U1 + u) * H;
            const double* hpr = hp.data() + (size_t)u * H;
            for (size_t j = 0; j < H; ++j) {
                const double gi = s[j], gf = s[H + j], gg = s[2 * H + j], go = s[3 * H + j], tc = tanh(s[4 * H + j]);
                const double cprev = u > 0 ? s[4 * H + j - LSTM_STATE] : cfirst[j];
                const double d = (double)go_[j] + dh[j];
                const double dct = dc[j] + d * go * (1.0 - tc * tc);
                dg[3 * H + j] = d * tc * (go * (1.0 - go));
                dg[j] = dct * gg * (gi * (1.0 - gi));
                dg[2 * H + j] = dct * gi * (1.0 - gg * gg);
                dg[H + j] = dct * cprev * (gf * (1.0 - gf));
                dc[j] = dct * gf;
            }
            std::fill(dhn.begin(), dhn.end(), 0.0);
            double* dxr = dx_host + ((size_t)b * U1 + u) * H;
            for (size_t n = 0; n < G; ++n) {
                const double g = dg[n];
                const double *wi = wih.data() + n * H, *wh = whh.data() + n * H;
                double *dwi = dw_ih_host + n * H, *dwh = dw_hh_host + n * H;
                for (size_t k = 0; k < H; ++k) {
                    dxr[k] += g * wi[k];
                    dhn[k] += g * wh[k];
                    dwi[k] += g * (double)xr[k];
                    dwh[k] += g * hpr[k];
                }
                db_host[n] += g;
            }
            dh = dhn;
        }
        for (size_t j = 0; j < H; ++j) {
            if (dh0_host) dh0_host[(size_t)b * H + j] = dh[j];
            if (dc0_host) dc0_host[(size_t)b * H + j] = dc[j];
        }
    }
    return RNNT_OK;
}
