// C ABI: the joint lattice with gradients for a trainer -- forward over raw (unpacked) weights, backward for a given d loss / d logits,
// and the backward's pure C++ twin.  No context: the caller brings the weights and the workspace; refusals are status codes.
// Included by rnnt_api.hip inside extern "C".  Kernels: joint_lattice_rows (rnnt_joint.hip.h, unchanged), rnnt_joint_grad.hip.h.

// static shares of the backward's launches: functions of the shape alone (never of the device), so the workspace formula is one
struct JointGeom { int KS, NUB, NC, TC, NVS, NS; long long CS, M; };
static JointGeom joint_geom(long long B, long long T, long long U, long long V) {
    JointGeom g;
    g.M = B * T * U;
    g.KS = (int)((V + 31) / 32);
    g.NUB = (int)((U + 15) / 16);
    const long long want = std::max(1LL, (long long)JG_TARGET_WGS / (B * g.NUB));      // frame chunks per (b, u-block)
    g.TC = (int)(4 * (((T + want - 1) / want + 3) / 4));
    g.NC = (int)((T + g.TC - 1) / g.TC);
    g.NVS = (int)((V + 63) / 64);
    const long long steps = (g.M + 31) / 32, slices = std::max(1LL, (long long)JG_TARGET_WGS / g.NVS);
    g.CS = 32 * ((steps + slices - 1) / slices);
    g.NS = (int)((g.M + g.CS - 1) / g.CS);
    return g;
}

// The caller's workspace from a 16-byte aligned base: the packed weight stream (425984 bytes in either direction), then the forward's
// regions or the backward's over the same bytes.  floats: forward e' [B T][256] | p' [B U1][256] | queue word [4];
// backward lens [2 B, rounded up to 4] | de_part [NUB][B T][256] | dp_part [NC][B U1][256] | dw_part [NS][V][256] | db_part [NS][V].
struct JointWork { unsigned char* wfrag; float *es, *ps; int* counter; int* lens; float *de_part, *dp_part, *dw_part, *db_part; size_t total; };
static JointWork joint_work(void* base, size_t B, size_t T, size_t U, size_t V, const JointGeom& g) {
    const size_t wbytes = (size_t)16 * JR_PIECES * 1024;       // = 13 * JG_STAGE
    static_assert((size_t)16 * JR_PIECES * 1024 == (size_t)13 * JG_STAGE, "one weight region serves both pack formats");
    JointWork w;
    w.wfrag = (unsigned char*)base;
    float* f0 = base ? (float*)((unsigned char*)base + wbytes) : nullptr;
    Carve<float> fw{f0}, bw{f0};
    w.es = fw.take(B * T * RNNT_D);
    w.ps = fw.take(B * U * RNNT_D);
    w.counter = (int*)fw.take(4);
    w.lens = (int*)bw.take((2 * B + 3) / 4 * 4);
    w.de_part = bw.take((size_t)g.NUB * B * T * RNNT_D);
    w.dp_part = bw.take((size_t)g.NC * B * U * RNNT_D);
    w.dw_part = bw.take((size_t)g.NS * V * RNNT_D);
    w.db_part = bw.take((size_t)g.NS * V);
    w.total = wbytes + std::max(fw.off, bw.off) * sizeof(float);
    return w;
}

static int joint_shape_check(int32_t B, int32_t T, int32_t U1, int32_t V) {
    if (B < 1 || T < 1 || U1 < 1) return RNNT_ERR_ARG;
    if (V < 4 || V > JR_NT * 16 || V % 4 != 0) return RNNT_ERR_SHAPE;
    if ((long long)B * T * U1 >= 0x7fffffffLL - JR_ROWS) return RNNT_ERR_SHAPE;
    return RNNT_OK;
}
static int joint_lens_check(const int32_t* logit_lens, const int32_t* target_lens, int32_t B, int32_t T, int32_t U1) {
    for (int b = 0; b < B; ++b) {
        if (logit_lens && (logit_lens[b] < 1 || logit_lens[b] > T)) return RNNT_ERR_ARG;
        if (target_lens && (target_lens[b] < 0 || target_lens[b] > U1 - 1)) return RNNT_ERR_ARG;
    }
    return RNNT_OK;
}

int rnnt_joint_lattice_workspace(int32_t B, int32_t T, int32_t U1, int32_t V, int64_t* bytes_out) {
    if (!bytes_out) return RNNT_ERR_ARG;
    if (int rc = joint_shape_check(B, T, U1, V)) return rc;
    *bytes_out = (int64_t)joint_work(nullptr, B, T, U1, V, joint_geom(B, T, U1, V)).total;
    return RNNT_OK;
}

#define JOINT_HIPCHK(expr)                             \
    do {                                               \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

// There is no context to remember a device in: its CU count, and the LDS the three kernels may ask for, are settled on the first call
// per device (two first calls at once settle the same thing twice).
static int joint_device(int* n_cus) {
    static std::atomic<int> ready[64];
    int dev = 0;
    JOINT_HIPCHK(hipGetDevice(&dev));
    int n = dev >= 0 && dev < 64 ? ready[dev].load() : 0;
    if (n == 0) {
        JOINT_HIPCHK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        if (n < 1) return RNNT_ERR_HIP;
        JOINT_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_lattice_rows<2, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, JR_LDS_ALLOC));
        JOINT_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_grad_dz), hipFuncAttributeMaxDynamicSharedMemorySize, JG_LDS));
        JOINT_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&joint_grad_dw), hipFuncAttributeMaxDynamicSharedMemorySize, JG_LDS));
        if (dev >= 0 && dev < 64) ready[dev].store(n);
    }
    *n_cus = n;
    return RNNT_OK;
}

int rnnt_joint_lattice_forward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, int32_t B, int32_t T, int32_t U1,
                               int32_t V, float* logits_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!e_dev || !p_dev || !w_dev || !b_dev || !logits_dev || !workspace_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)e_dev | (uintptr_t)p_dev | (uintptr_t)w_dev | (uintptr_t)b_dev | (uintptr_t)logits_dev | (uintptr_t)workspace_dev) & 15) return RNNT_ERR_ARG;
    int rc, n_cus = 0;
    if ((rc = joint_shape_check(B, T, U1, V))) return rc;
    const JointGeom g = joint_geom(B, T, U1, V);
    const JointWork w = joint_work(workspace_dev, B, T, U1, V, g);
    if (workspace_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    if ((rc = joint_device(&n_cus))) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((pack_joint_w<false, true>), dim3((16 * JR_PIECES * 64 + 255) / 256), dim3(256), 0, s, w_dev, (int)V, w.wfrag);
    const long long ne4 = (long long)B * T * (RNNT_D / 4), np4 = (long long)B * U1 * (RNNT_D / 4);
    hipLaunchKernelGGL(joint_prescale, dim3((unsigned)((ne4 + 255) / 256)), dim3(256), 0, s, e_dev, w.es, ne4);
    hipLaunchKernelGGL(joint_prescale, dim3((unsigned)((np4 + 255) / 256)), dim3(256), 0, s, p_dev, w.ps, np4);
    JOINT_HIPCHK(hipMemsetAsync(w.counter, 0, 16, s));
    JointRP jp;
    memset(&jp, 0, sizeof(jp));
    jp.e = w.es; jp.p = w.ps; jp.wfrag = w.wfrag; jp.bias = b_dev; jp.out = logits_dev; jp.M = g.M; jp.T = T; jp.U = U1; jp.V = V;
    jp.ntiles = (int)((g.M + JR_ROWS - 1) / JR_ROWS);
    jp.counter = w.counter;
    jp.stagger = JR_STAGGER;
    hipLaunchKernelGGL((joint_lattice_rows<2, false, false>), dim3((unsigned)std::min(jp.ntiles, JR_WGS_PER_CU * n_cus)), dim3(256), JR_LDS_ALLOC, s, jp);
    JOINT_HIPCHK(hipGetLastError());
    return RNNT_OK;
}

int rnnt_joint_lattice_backward(const float* e_dev, const float* p_dev, const float* w_dev, const float* g_dev, const int32_t* logit_lens_host,
                                const int32_t* target_lens_host, int32_t B, int32_t T, int32_t U1, int32_t V, float* de_dev, float* dp_dev,
                                float* dw_dev, float* db_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!e_dev || !p_dev || !w_dev || !g_dev || !de_dev || !dp_dev || !dw_dev || !db_dev || !workspace_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)e_dev | (uintptr_t)p_dev | (uintptr_t)w_dev | (uintptr_t)g_dev | (uintptr_t)de_dev | (uintptr_t)dp_dev | (uintptr_t)dw_dev |
         (uintptr_t)db_dev | (uintptr_t)workspace_dev) & 15)
        return RNNT_ERR_ARG;
    if (B < 1 || T < 1 || U1 < 1) return RNNT_ERR_ARG;
    int rc, n_cus = 0;
    if ((rc = joint_lens_check(logit_lens_host, target_lens_host, B, T, U1))) return rc;
    if ((rc = joint_shape_check(B, T, U1, V))) return rc;
    const JointGeom g = joint_geom(B, T, U1, V);
    const JointWork w = joint_work(workspace_dev, B, T, U1, V, g);
    if (workspace_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    if ((rc = joint_device(&n_cus))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> host(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        host[b] = logit_lens_host ? logit_lens_host[b] : T;
        host[B + b] = target_lens_host ? target_lens_host[b] : U1 - 1;
    }
    // (pageable source: the runtime has taken the bytes when the call returns; what follows is launches only)
    JOINT_HIPCHK(hipMemcpyAsync(w.lens, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    JointGradP P;
    memset(&P, 0, sizeof(P));
    P.e = e_dev; P.p = p_dev; P.g = g_dev; P.wt = w.wfrag; P.lens = w.lens;
    P.de_part = w.de_part; P.dp_part = w.dp_part; P.dw_part = w.dw_part; P.db_part = w.db_part;
    P.M = g.M; P.B = B; P.T = T; P.U = U1; P.V = V; P.KS = g.KS; P.NUB = g.NUB; P.NC = g.NC; P.TC = g.TC; P.NVS = g.NVS; P.CS = g.CS;
    hipLaunchKernelGGL(joint_grad_pack_wt, dim3((unsigned)((g.KS * 2048 + 255) / 256)), dim3(256), 0, s, w_dev, (int)V, g.KS, w.wfrag);
    hipLaunchKernelGGL(joint_grad_dz, dim3((unsigned)((long long)B * g.NUB * g.NC)), dim3(256), JG_LDS, s, P);
    hipLaunchKernelGGL(joint_grad_dw, dim3((unsigned)((long long)g.NVS * g.NS)), dim3(256), JG_LDS, s, P);
    const long long de4 = (long long)B * T * (RNNT_D / 4), dp4 = (long long)B * U1 * (RNNT_D / 4), dw4 = (long long)V * (RNNT_D / 4), db4 = V / 4;
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((de4 + 255) / 256)), dim3(256), 0, s, w.de_part, g.NUB, de4, de4, de_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((dp4 + 255) / 256)), dim3(256), 0, s, w.dp_part, g.NC, dp4, dp4, dp_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((dw4 + 255) / 256)), dim3(256), 0, s, w.dw_part, g.NS, dw4, dw4, dw_dev);
    hipLaunchKernelGGL(joint_grad_reduce, dim3((unsigned)((db4 + 255) / 256)), dim3(256), 0, s, w.db_part, g.NS, db4, db4, db_dev);
    JOINT_HIPCHK(hipGetLastError());
    return RNNT_OK;
}
#undef JOINT_HIPCHK

// The same gradients in plain C++ (no GPU): f64 throughout over the float32 inputs, cell by cell in memory order.  g of type G (float:
// rnnt_joint_lattice_backward_host; double: the gradient rnnt_joint_loss_host forms for itself).
extern "C++" template <typename G>
static int joint_backward_host_cells(const float* e_host, const float* p_host, const float* w_host, const G* g_host, const int32_t* logit_lens_host,
                                     const int32_t* target_lens_host, int32_t B, int32_t T, int32_t U1, int32_t V, double* de_host, double* dp_host,
                                     double* dw_host, double* db_host) {
    if (!e_host || !p_host || !w_host || !g_host || !de_host || !dp_host || !dw_host || !db_host) return RNNT_ERR_ARG;
    if (B < 1 || T < 1 || U1 < 1) return RNNT_ERR_ARG;
    int rc;
    if ((rc = joint_lens_check(logit_lens_host, target_lens_host, B, T, U1))) return rc;
    if ((rc = joint_shape_check(B, T, U1, V))) return rc;
    const size_t Dn = RNNT_D;
    std::fill(de_host, de_host + (size_t)B * T * Dn, 0.0);
    std::fill(dp_host, dp_host + (size_t)B * U1 * Dn, 0.0);
    std::fill(dw_host, dw_host + (size_t)V * Dn, 0.0);
    std::fill(db_host, db_host + (size_t)V, 0.0);
    std::vector<double> w64((size_t)V * Dn), h(Dn), dh(Dn);
    for (size_t k = 0; k < w64.size(); ++k) w64[k] = (double)w_host[k];
    for (int b = 0; b < B; ++b) {
        const int Tb = logit_lens_host ? logit_lens_host[b] : T, Ub = target_lens_host ? target_lens_host[b] : U1 - 1;
        for (int t = 0; t < Tb; ++t)
            for (int u = 0; u <= Ub; ++u) {
                const float* er = e_host + ((size_t)b * T + t) * Dn;
                const float* pr = p_host + ((size_t)b * U1 + u) * Dn;
                const G* gr = g_host + (((size_t)b * T + t) * U1 + u) * V;
                for (size_t k = 0; k < Dn; ++k) { h[k] = tanh((double)er[k] + (double)pr[k]); dh[k] = 0.0; }
                for (int v = 0; v < V; ++v) {
                    const double gv = (double)gr[v];
                    const double* wr = w64.data() + (size_t)v * Dn;
                    double* dwr = dw_host + (size_t)v * Dn;
                    for (size_t k = 0; k < Dn; ++k) { dh[k] += gv * wr[k]; dwr[k] += gv * h[k]; }
                    db_host[v] += gv;
                }
                double* der = de_host + ((size_t)b * T + t) * Dn;
                double* dpr = dp_host + ((size_t)b * U1 + u) * Dn;
                for (size_t k = 0; k < Dn; ++k) {
                    const double dz = dh[k] * (1.0 - h[k] * h[k]);
                    der[k] += dz;
                    dpr[k] += dz;
                }
            }
    }
    return RNNT_OK;
}

int rnnt_joint_lattice_backward_host(const float* e_host, const float* p_host, const float* w_host, const float* g_host, const int32_t* logit_lens_host,
                                     const int32_t* target_lens_host, int32_t B, int32_t T, int32_t U1, int32_t V, double* de_host, double* dp_host,
                                     double* dw_host, double* db_host) {
    return joint_backward_host_cells<float>(e_host, p_host, w_host, g_host, logit_lens_host, target_lens_host, B, T, U1, V, de_host, dp_host, dw_host, db_host);
}
