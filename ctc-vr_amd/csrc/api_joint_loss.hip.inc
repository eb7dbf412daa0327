// C ABI: the fused transducer joint and loss for a trainer -- nll_b of the lattice tanh(e + p) W^T + bias and, in a second call, its
// gradients with respect to e, p, W and bias -- without the [B, T, U1, V] lattice or its gradient ever being stored.
// No context: the caller brings the weights, the workspace and the state that carries the forward's per-cell factors to the backward.
// Included by rnnt_api.hip inside extern "C".  Kernels: joint_lattice_rows<2, false, true, true, true> (rnnt_joint.hip.h),
// transducer_alpha_beta and loss_coef (rnnt_loss.hip.h), rnnt_joint_loss.hip.h, joint_grad_reduce (rnnt_joint_grad.hip.h).

// state, from a 16-byte aligned base: coef [M][4] floats | lens [2][B] | targets [B][ts] (ints), ts = max(U1 - 1, 1); rounded up to 16 bytes
struct JointLossState { float* coef; int *lens, *tg; size_t ints, total; };
static JointLossState joint_loss_state(void* base, size_t B, size_t T, size_t U1) {
    const size_t cells = B * T * U1, ts = U1 > 1 ? U1 - 1 : 1;
    JointLossState st;
    st.coef = (float*)base;
    st.lens = base ? (int*)(st.coef + 4 * cells) : nullptr;
    st.tg = base ? st.lens + 2 * B : nullptr;
    st.ints = 2 * B + B * ts;
    st.total = 16 * cells + (st.ints + 3) / 4 * 16;
    return st;
}

// work, from a 16-byte aligned base.  forward: nll_alpha [B, rounded up to even] | alpha, beta [M] (f64) | packed W (425984 bytes) |
// e' [B T][256] | p' [B U1][256] | queue word [4] | pick [M][2] | lse [M] (floats).  backward, over the same bytes: joint_loss_pack_w's
// stream [KS][65536 bytes] | de_part | dp_part | dw_part | db_part (joint_geom's slabs, floats).
struct JointLossWork {
    double *nll_alpha, *alpha, *beta;
    unsigned char* wfrag;
    float *es, *ps;
    int* counter;
    float *pick, *lse;
    unsigned char* wz;
    float *de_part, *dp_part, *dw_part, *db_part;
    size_t total;
};
static JointLossWork joint_loss_work(void* base, size_t B, size_t T, size_t U, size_t V, const JointGeom& g) {
    const size_t cells = B * T * U, wbytes = (size_t)16 * JR_PIECES * 1024;
    JointLossWork w;
    Carve<double> d{(double*)base};
    w.nll_alpha = d.take(B + (B & 1));
    w.alpha = d.take(cells);
    w.beta = d.take(cells);
    w.wfrag = base ? (unsigned char*)base + d.off * sizeof(double) : nullptr;
    Carve<float> f{base ? (float*)(w.wfrag + wbytes) : nullptr};
    w.es = f.take(B * T * RNNT_D);
    w.ps = f.take(B * U * RNNT_D);
    w.counter = (int*)f.take(4);
    w.pick = f.take(2 * cells);
    w.lse = f.take((cells + 3) / 4 * 4);
    const size_t fwd = d.off * sizeof(double) + wbytes + f.off * sizeof(float);
    const size_t zbytes = (size_t)g.KS * JL_STAGE;
    w.wz = (unsigned char*)base;
    Carve<float> bw{base ? (float*)((unsigned char*)base + zbytes) : nullptr};
    w.de_part = bw.take((size_t)g.NUB * B * T * RNNT_D);
    w.dp_part = bw.take((size_t)g.NC * B * U * RNNT_D);
    w.dw_part = bw.take((size_t)g.NS * V * RNNT_D);
    w.db_part = bw.take((size_t)g.NS * V);
    w.total = std::max(fwd, zbytes + bw.off * sizeof(float));
    return w;
}

static int joint_loss_shape_check(int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank) {
    if (B < 1 || T < 1 || Umax < 0) return RNNT_ERR_ARG;
    if (int rc = joint_shape_check(B, T, Umax + 1, V)) return rc;
    if (Umax > SCORE_UMAX) return RNNT_ERR_SHAPE;
    if (blank < 0 || blank >= V) return RNNT_ERR_ARG;
    return RNNT_OK;
}

int rnnt_joint_loss_workspace(int32_t B, int32_t T, int32_t U1, int32_t V, int64_t* work_bytes, int64_t* state_bytes) {
    if (!work_bytes || !state_bytes) return RNNT_ERR_ARG;
    if (int rc = joint_loss_shape_check(B, T, U1 - 1, V, 0)) return rc;
    *work_bytes = (int64_t)joint_loss_work(nullptr, B, T, U1, V, joint_geom(B, T, U1, V)).total;
    *state_bytes = (int64_t)joint_loss_state(nullptr, B, T, U1).total;
    return RNNT_OK;
}

#define JLOSS_HIPCHK(expr)                             \
    do {                                               \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

// as joint_device: the CU count and the LDS the three kernels may ask for, settled on the first call per device
static int joint_loss_device(int* n_cus) {
    static std::atomic<int> ready[64];
    int dev = 0;
    JLOSS_HIPCHK(hipGetDevice(&dev));
    int n = dev >= 0 && dev < 64 ? ready[dev].load() : 0;
    if (n == 0) {
        JLOSS_HIPCHK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        if (n < 1) return RNNT_ERR_HIP;
        JLOSS_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_lattice_rows<2, false, true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, JR_LDS_ALLOC));
        JLOSS_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_loss_dz), hipFuncAttributeMaxDynamicSharedMemorySize, JL_DZ_LDS));
        JLOSS_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_loss_dw), hipFuncAttributeMaxDynamicSharedMemorySize, JL_DW_LDS));
        if (dev >= 0 && dev < 64) ready[dev].store(n);
    }
    *n_cus = n;
    return RNNT_OK;
}

int rnnt_joint_loss_forward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, const int32_t* targets_host,
                            const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V,
                            int32_t blank, double* nll_dev, void* state_dev, int64_t state_bytes, void* work_dev, int64_t work_bytes, void* stream) {
    if (!e_dev || !p_dev || !w_dev || !b_dev || !logit_lens_host || !target_lens_host || !nll_dev || !state_dev || !work_dev || (Umax > 0 && !targets_host))
        return RNNT_ERR_ARG;
    if (((uintptr_t)e_dev | (uintptr_t)p_dev | (uintptr_t)w_dev | (uintptr_t)b_dev | (uintptr_t)nll_dev | (uintptr_t)state_dev | (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc, n_cus = 0;
    if ((rc = joint_loss_shape_check(B, T, Umax, V, blank))) return rc;
    for (int b = 0; b < B; ++b) {
        if (logit_lens_host[b] < 1 || logit_lens_host[b] > T || target_lens_host[b] < 0 || target_lens_host[b] > Umax) return RNNT_ERR_ARG;
        for (int u = 0; u < target_lens_host[b]; ++u) {
            const int y = targets_host[(size_t)b * Umax + u];
            if (y < 0 || y >= V || y == blank) return RNNT_ERR_ARG;
        }
    }
    const int U1 = Umax + 1, ts = Umax > 0 ? Umax : 1;
    const JointGeom g = joint_geom(B, T, U1, V);
    const JointLossWork w = joint_loss_work(work_dev, B, T, U1, V, g);
    const JointLossState st = joint_loss_state(state_dev, B, T, U1);
    if (work_bytes < (int64_t)w.total || state_bytes < (int64_t)st.total) return RNNT_ERR_SHAPE;
    if ((rc = joint_loss_device(&n_cus))) return rc;
    hipStream_t s = (hipStream_t)stream;
    // lens | targets in ONE copy into the state; entries beyond a row's length become the blank: they are neither validated nor used
    std::vector<int> host((st.ints + 3) / 4 * 4, blank);
    for (int b = 0; b < B; ++b) {
        host[b] = logit_lens_host[b];
        host[B + b] = target_lens_host[b];
        for (int u = 0; u < target_lens_host[b]; ++u) host[2 * (size_t)B + (size_t)b * ts + u] = targets_host[(size_t)b * Umax + u];
    }
    // (pageable source: the runtime has taken the bytes when the call returns, so `host` may go; what follows is launches only)
    JLOSS_HIPCHK(hipMemcpyAsync(st.lens, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    JLOSS_HIPCHK(hipMemsetAsync(st.coef, 0, 16 * (size_t)g.M, s));   // loss_coef writes the valid cells only: the state leaves here with every byte defined
    hipLaunchKernelGGL((pack_joint_w<false, true>), dim3((16 * JR_PIECES * 64 + 255) / 256), dim3(256), 0, s, w_dev, (int)V, w.wfrag);
    const long long ne4 = (long long)B * T * (RNNT_D / 4), np4 = (long long)B * U1 * (RNNT_D / 4);
    hipLaunchKernelGGL(joint_prescale, dim3((unsigned)((ne4 + 255) / 256)), dim3(256), 0, s, e_dev, w.es, ne4);
    hipLaunchKernelGGL(joint_prescale, dim3((unsigned)((np4 + 255) / 256)), dim3(256), 0, s, p_dev, w.ps, np4);
    JLOSS_HIPCHK(hipMemsetAsync(w.counter, 0, 16, s));
    JointRP jp;
    memset(&jp, 0, sizeof(jp));
    jp.e = w.es; jp.p = w.ps; jp.wfrag = w.wfrag; jp.bias = b_dev; jp.out = w.lse; jp.M = g.M; jp.T = T; jp.U = U1; jp.V = V;
    jp.ntiles = (int)((g.M + JR_ROWS - 1) / JR_ROWS);
    jp.counter = w.counter;
    jp.stagger = JR_STAGGER;
    jp.targets = st.tg; jp.pick = w.pick; jp.tstride = ts; jp.blank = blank;
    // every cell, padding included: a padded cell's picks may be NaN; the recursions and loss_coef go through loss_cell and never read them
    hipLaunchKernelGGL((joint_lattice_rows<2, false, true, true, true>), dim3((unsigned)std::min(jp.ntiles, JR_WGS_PER_CU * n_cus)), dim3(256), JR_LDS_ALLOC, s, jp);
    const int ncell = (int)g.M;
    hipLaunchKernelGGL(transducer_alpha_beta, dim3(2 * B), dim3(256), 0, s, w.pick, st.lens, B, T, U1, w.alpha, w.beta, w.nll_alpha, nll_dev);
    hipLaunchKernelGGL(loss_coef, dim3((unsigned)grid_for(ncell)), dim3(256), 0, s, w.pick, w.lse, w.alpha, w.beta, st.lens, B, T, U1, 1, st.coef);
    JLOSS_HIPCHK(hipGetLastError());
    return RNNT_OK;
}

int rnnt_joint_loss_backward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, const void* state_dev, int64_t state_bytes,
                             const float* row_scale_dev, float clamp, int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank, float* de_dev,
                             float* dp_dev, float* dw_dev, float* db_dev, void* work_dev, int64_t work_bytes, void* stream) {
    if (!e_dev || !p_dev || !w_dev || !b_dev || !state_dev || !row_scale_dev || !de_dev || !dp_dev || !dw_dev || !db_dev || !work_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)e_dev | (uintptr_t)p_dev | (uintptr_t)w_dev | (uintptr_t)b_dev | (uintptr_t)state_dev | (uintptr_t)row_scale_dev | (uintptr_t)de_dev |
         (uintptr_t)dp_dev | (uintptr_t)dw_dev | (uintptr_t)db_dev | (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc, n_cus = 0;
    if ((rc = joint_loss_shape_check(B, T, Umax, V, blank))) return rc;
    const int U1 = Umax + 1, ts = Umax > 0 ? Umax : 1;
    const JointGeom g = joint_geom(B, T, U1, V);
    const JointLossWork w = joint_loss_work(work_dev, B, T, U1, V, g);
    const JointLossState st = joint_loss_state(const_cast<void*>(state_dev), B, T, U1);
    if (work_bytes < (int64_t)w.total || state_bytes < (int64_t)st.total) return RNNT_ERR_SHAPE;
    if ((rc = joint_loss_device(&n_cus))) return rc;
    hipStream_t s = (hipStream_t)stream;
    JointLossP P;
    memset(&P, 0, sizeof(P));
    P.e = e_dev; P.p = p_dev; P.w = w_dev; P.bias = b_dev; P.wz = w.wz; P.coef = st.coef; P.lens = st.lens; P.targets = st.tg; P.row_scale = row_scale_dev;
    P.de_part = w.de_part; P.dp_part = w.dp_part; P.dw_part = w.dw_part; P.db_part = w.db_part;
    P.M = g.M; P.CS = g.CS; P.B = B; P.T = T; P.U = U1; P.V = V; P.KS = g.KS; P.NUB = g.NUB; P.NC = g.NC; P.TC = g.TC; P.NVS = g.NVS;
    P.ts = ts; P.blank = blank; P.clamp = clamp;
    hipLaunchKernelGGL(joint_loss_pack_w, dim3((unsigned)(g.KS * 4096 / 256)), dim3(256), 0, s, w_dev, (int)V, g.KS, w.wz);
    hipLaunchKernelGGL(joint_loss_dz, dim3((unsigned)((long long)B * g.NUB * g.NC)), dim3(256), JL_DZ_LDS, s, P);
    hipLaunchKernelGGL(joint_loss_dw, dim3((unsigned)((long long)g.NVS * g.NS)), dim3(256), JL_DW_LDS, s, P);
    const long long de4 = (long long)B * T * (RNNT_D / 4), dp4 = (long long)B * U1 * (RNNT_D / 4), dw4 = (long long)V * (RNNT_D / 4), db4 = V / 4;
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((de4 + 255) / 256)), dim3(256), 0, s, w.de_part, g.NUB, de4, de4, de_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((dp4 + 255) / 256)), dim3(256), 0, s, w.dp_part, g.NC, dp4, dp4, dp_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((dw4 + 255) / 256)), dim3(256), 0, s, w.dw_part, g.NS, dw4, dw4, dw_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((db4 + 255) / 256)), dim3(256), 0, s, w.db_part, g.NS, db4, db4, db_dev);
    JLOSS_HIPCHK(hipGetLastError());
    return RNNT_OK;
}
#undef JLOSS_HIPCHK

// The same function in plain C++ (no GPU): the float64 host sides of the lattice, of rnnt_transducer_loss_host and of
// rnnt_joint_lattice_backward_host composed with nothing rounded in between -- here the lattice and its gradient DO exist, in f64.
// row_scale_host null: nll only, the four outputs are not touched.
int rnnt_joint_loss_host(const float* e_host, const float* p_host, const float* w_host, const float* b_host, const int32_t* targets_host,
                         const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank,
                         float clamp, const double* row_scale_host, double* nll_host, double* de_host, double* dp_host, double* dw_host, double* db_host) {
    if (!e_host || !p_host || !w_host || !b_host || !logit_lens_host || !target_lens_host || !nll_host || (Umax > 0 && !targets_host)) return RNNT_ERR_ARG;
    if (row_scale_host && (!de_host || !dp_host || !dw_host || !db_host)) return RNNT_ERR_ARG;
    int rc;
    if ((rc = joint_loss_shape_check(B, T, Umax, V, blank))) return rc;
    if ((rc = loss_check(e_host, targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, nll_host))) return rc;
    const int U1 = Umax + 1;
    const size_t Dn = RNNT_D, cells = (size_t)B * T * U1;
    std::vector<double> logits(cells * V, 0.0), grad(row_scale_host ? cells * V : 0), h(Dn);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < logit_lens_host[b]; ++t)
            for (int u = 0; u <= target_lens_host[b]; ++u) {
                const float* er = e_host + ((size_t)b * T + t) * Dn;
                const float* pr = p_host + ((size_t)b * U1 + u) * Dn;
                for (size_t k = 0; k < Dn; ++k) h[k] = tanh((double)er[k] + (double)pr[k]);
                double* z = logits.data() + (((size_t)b * T + t) * U1 + u) * V;
                for (int v = 0; v < V; ++v) {
                    const float* wr = w_host + (size_t)v * Dn;
                    double a = 0.0;
                    for (size_t k = 0; k < Dn; ++k) a += h[k] * (double)wr[k];
                    z[v] = a + (double)b_host[v];
                }
            }
    if ((rc = loss_host_rows<double>(logits.data(), targets_host, logit_lens_host, target_lens_host, B, T, Umax, V, blank, 1, clamp, nll_host,
                                     row_scale_host ? grad.data() : nullptr)))
        return rc;
    if (!row_scale_host) return RNNT_OK;
    for (int b = 0; b < B; ++b) {
        double* gb = grad.data() + (size_t)b * T * U1 * V;
        for (size_t k = 0; k < (size_t)T * U1 * V; ++k) gb[k] *= row_scale_host[b];
    }
    return joint_backward_host_cells<double>(e_host, p_host, w_host, grad.data(), logit_lens_host, target_lens_host, B, T, U1, V, de_host, dp_host, dw_host,
                                             db_host);
}
