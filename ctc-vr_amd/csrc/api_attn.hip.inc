// C ABI: the attention core of an encoder layer (relative positions indexed by the key, chunk mask) with gradients -- forward,
// backward, and the plain C++ float64 twin of both.  No context, like the LSTM calls: the caller brings q, k, v, p and the two
// biases as they lie after the layer's Linears, a workspace and a state; refusals are status codes, decided on the host before
// anything is launched or written.
// Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_attn_grad.hip.h.

static int attn_shape_check(int32_t B, int32_t T, int32_t chunk, int32_t left) {
    if (B < 1 || T < 1) return RNNT_ERR_ARG;
    if (left >= 0 && chunk <= 0) return RNNT_ERR_ARG;              // a bounded left context counts in chunks
    if (T > ATTN_TMAX) return RNNT_ERR_SHAPE;
    if ((long long)B * T * RNNT_D >= 0x7fffffffLL) return RNNT_ERR_SHAPE;         // block and element indices are ints
    return RNNT_OK;
}
static int attn_lens_check(const int32_t* lens, int32_t B, int32_t T) {
    for (int b = 0; lens && b < B; ++b)
        if (lens[b] < 1 || lens[b] > T) return RNNT_ERR_ARG;
    return RNNT_OK;
}

// The caller's workspace from a 16-byte aligned base, in floats: lens [B rounded up to 4] (ints) | delta [B 4 T rounded up to 4] |
// dp partials [B][T][256] | du partials [B nt][256] | dvb partials [B nt][256], nt = ceil(T / 16).  The forward uses lens alone.
struct AttnWork { int* lens; float *delta, *dp_part, *du_part, *dvb_part; int nt; size_t total; };
static AttnWork attn_work(void* base, size_t B, size_t T) {
    Carve<float> f{(float*)base};
    AttnWork w;
    w.nt = (int)((T + ATTN_TILE - 1) / ATTN_TILE);
    w.lens = (int*)f.take((B + 3) / 4 * 4);
    w.delta = f.take((B * RNNT_H * T + 3) / 4 * 4);
    w.dp_part = f.take(B * T * RNNT_D);
    w.du_part = f.take(B * w.nt * RNNT_D);
    w.dvb_part = f.take(B * w.nt * RNNT_D);
    w.total = f.off * sizeof(float);
    return w;
}
static int64_t attn_state_bytes(int32_t B, int32_t T) { return (int64_t)B * RNNT_H * T * (int64_t)sizeof(float); }

int rnnt_rel_attention_workspace(int32_t B, int32_t T, int64_t* work_bytes, int64_t* state_bytes) {
    if (!work_bytes || !state_bytes) return RNNT_ERR_ARG;
    if (int rc = attn_shape_check(B, T, 0, -1)) return rc;
    *work_bytes = (int64_t)attn_work(nullptr, B, T).total;
    *state_bytes = attn_state_bytes(B, T);
    return RNNT_OK;
}

#define ATTN_HIPCHK(expr)                              \
    do {                                               \
        if ((expr) != hipSuccess) return RNNT_ERR_HIP; \
    } while (0)

static int attn_send_lens(const AttnWork& w, const int32_t* lens_host, int B, int T, hipStream_t s) {
    std::vector<int> host((size_t)B);
    for (int b = 0; b < B; ++b) host[b] = lens_host ? lens_host[b] : T;
    // Pageable source: the runtime has taken the bytes when the call returns, which holds as long as it stages the copy (as it does
    // for the few hundred bytes of a trainer's batch); a copy large enough to be pinned in place instead is waited for here, so that
    // `host` may go out of scope either way.  What follows is launches only.
    ATTN_HIPCHK(hipMemcpyAsync(w.lens, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    if (host.size() * sizeof(int) > 65536) ATTN_HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_rel_attention_forward(const float* q_dev, const float* k_dev, const float* v_dev, const float* p_dev, const float* u_dev, const float* vb_dev,
                               const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size, int32_t num_left_chunks, float* out_dev, void* state_dev,
                               int64_t state_bytes, void* work_dev, int64_t work_bytes, void* stream) {
    if (!q_dev || !k_dev || !v_dev || !p_dev || !u_dev || !vb_dev || !out_dev || !work_dev) return RNNT_ERR_ARG;
    if (((uintptr_t)q_dev | (uintptr_t)k_dev | (uintptr_t)v_dev | (uintptr_t)p_dev | (uintptr_t)u_dev | (uintptr_t)vb_dev | (uintptr_t)out_dev |
         (uintptr_t)state_dev | (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc;
    if ((rc = attn_shape_check(B, T, chunk_size, num_left_chunks))) return rc;
    if ((rc = attn_lens_check(lens_host, B, T))) return rc;
    const AttnWork w = attn_work(work_dev, B, T);
    if (work_bytes < (int64_t)w.total) return RNNT_ERR_SHAPE;
    if (state_dev && state_bytes < attn_state_bytes(B, T)) return RNNT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = attn_send_lens(w, lens_host, B, T, s))) return rc;
    AttnGradP a;
    memset(&a, 0, sizeof(a));
    a.q = q_dev; a.k = k_dev; a.v = v_dev; a.p = p_dev; a.u = u_dev; a.vb = vb_dev; a.lens = w.lens; a.out = out_dev; a.lse = (float*)state_dev;
    a.B = B; a.T = T; a.nt = w.nt; a.chunk = chunk_size; a.left = num_left_chunks;
    hipLaunchKernelGGL(attn_fwd, dim3((unsigned)(B * w.nt)), dim3(256), 0, s, a);
    ATTN_HIPCHK(hipGetLastError());
    return RNNT_OK;
}

int rnnt_rel_attention_backward(const float* q_dev, const float* k_dev, const float* v_dev, const float* p_dev, const float* u_dev, const float* vb_dev,
                                const float* out_dev, const void* state_dev, int64_t state_bytes, const float* dout_dev, const int32_t* lens_host, int32_t B,
                                int32_t T, int32_t chunk_size, int32_t num_left_chunks, float* dq_dev, float* dk_dev, float* dv_dev, float* dp_dev,
                                float* du_dev, float* dvb_dev, void* work_dev, int64_t work_bytes, void* stream) {
    if (!q_dev || !k_dev || !v_dev || !p_dev || !u_dev || !vb_dev || !out_dev || !state_dev || !dout_dev || !dq_dev || !dk_dev || !dv_dev || !dp_dev ||
        !du_dev || !dvb_dev || !work_dev)
        return RNNT_ERR_ARG;
    if (((uintptr_t)q_dev | (uintptr_t)k_dev | (uintptr_t)v_dev | (uintptr_t)p_dev | (uintptr_t)u_dev | (uintptr_t)vb_dev | (uintptr_t)out_dev |
         (uintptr_t)state_dev | (uintptr_t)dout_dev | (uintptr_t)dq_dev | (uintptr_t)dk_dev | (uintptr_t)dv_dev | (uintptr_t)dp_dev | (uintptr_t)du_dev |
         (uintptr_t)dvb_dev | (uintptr_t)work_dev) & 15)
        return RNNT_ERR_ARG;
    int rc;
    if ((rc = attn_shape_check(B, T, chunk_size, num_left_chunks))) return rc;
    if ((rc = attn_lens_check(lens_host, B, T))) return rc;
    const AttnWork w = attn_work(work_dev, B, T);
    if (work_bytes < (int64_t)w.total || state_bytes < attn_state_bytes(B, T)) return RNNT_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = attn_send_lens(w, lens_host, B, T, s))) return rc;
    const long long rows = (long long)B * T * RNNT_H;
    hipLaunchKernelGGL(attn_delta, dim3((unsigned)((rows * 16 + 255) / 256)), dim3(256), 0, s, out_dev, dout_dev, rows, T, w.delta);
    AttnGradP a;
    memset(&a, 0, sizeof(a));
    a.q = q_dev; a.k = k_dev; a.v = v_dev; a.p = p_dev; a.u = u_dev; a.vb = vb_dev; a.dout = dout_dev; a.lse_in = (const float*)state_dev; a.delta_in = w.delta;
    a.lens = w.lens; a.dq = dq_dev; a.dk = dk_dev; a.dv = dv_dev; a.dp_part = w.dp_part; a.du_part = w.du_part; a.dvb_part = w.dvb_part;
    a.B = B; a.T = T; a.nt = w.nt; a.chunk = chunk_size; a.left = num_left_chunks;
    hipLaunchKernelGGL(attn_bwd_k, dim3((unsigned)(B * w.nt)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn_bwd_q, dim3((unsigned)(B * w.nt)), dim3(256), 0, s, a);
    const long long p4 = (long long)T * RNNT_D / 4;
    hipLaunchKernelGGL(lstm_slab_reduce, dim3((unsigned)((p4 + 255) / 256)), dim3(256), 0, s, w.dp_part, B, p4, dp_dev);
    hipLaunchKernelGGL(attn_bias_reduce, dim3(8), dim3(64 * ATTN_RED_GROUPS), 0, s, w.du_part, w.dvb_part, B * w.nt, du_dev, dvb_dev);
    ATTN_HIPCHK(hipGetLastError());
    return RNNT_OK;
}
#undef ATTN_HIPCHK

// Both directions in plain C++ (no GPU): f64 throughout over the float32 inputs, one [T] row of scores at a time.  dout_host null:
// forward only.
int rnnt_rel_attention_host(const float* q_host, const float* k_host, const float* v_host, const float* p_host, const float* u_host, const float* vb_host,
                            const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size, int32_t num_left_chunks, const float* dout_host,
                            double* out_host, double* dq_host, double* dk_host, double* dv_host, double* dp_host, double* du_host, double* dvb_host) {
    if (!q_host || !k_host || !v_host || !p_host || !u_host || !vb_host || !out_host) return RNNT_ERR_ARG;
    if (dout_host && (!dq_host || !dk_host || !dv_host || !dp_host || !du_host || !dvb_host)) return RNNT_ERR_ARG;
    int rc;
    if ((rc = attn_shape_check(B, T, chunk_size, num_left_chunks))) return rc;
    if ((rc = attn_lens_check(lens_host, B, T))) return rc;
    const size_t D = RNNT_D, DK = RNNT_DK, n = (size_t)B * T * D;
    std::fill(out_host, out_host + n, 0.0);
    if (dout_host) {
        std::fill(dq_host, dq_host + n, 0.0);
        std::fill(dk_host, dk_host + n, 0.0);
        std::fill(dv_host, dv_host + n, 0.0);
        std::fill(dp_host, dp_host + (size_t)T * D, 0.0);
        std::fill(du_host, du_host + D, 0.0);
        std::fill(dvb_host, dvb_host + D, 0.0);
    }
    std::vector<double> a((size_t)T);
    for (int b = 0; b < B; ++b) {
        const int len = lens_host ? lens_host[b] : T;
        for (int h = 0; h < RNNT_H; ++h) {
            const float *u = u_host + h * DK, *vb = vb_host + h * DK;
            for (int i = 0; i < T; ++i) {
                int lo = 0, hi = T;
                if (chunk_size > 0) {
                    const int c = i / chunk_size;
                    hi = (int)std::min<long long>(T, ((long long)c + 1) * chunk_size);
                    if (num_left_chunks >= 0 && c > num_left_chunks) lo = (c - num_left_chunks) * chunk_size;
                }
                hi = std::min(hi, len);
                if (lo >= hi) continue;                            // no visible key: out = 0, no gradient
                const float* qi = q_host + ((size_t)b * T + i) * D + h * DK;
                double m = -INFINITY;
                for (int j = lo; j < hi; ++j) {
                    const float *kj = k_host + ((size_t)b * T + j) * D + h * DK, *pj = p_host + (size_t)j * D + h * DK;
                    double s = 0.0;
                    for (size_t d = 0; d < DK; ++d) s += ((double)qi[d] + (double)u[d]) * (double)kj[d] + ((double)qi[d] + (double)vb[d]) * (double)pj[d];
                    a[j] = s / 8.0;
                    m = std::max(m, a[j]);
                }
                double l = 0.0;
                for (int j = lo; j < hi; ++j) { a[j] = exp(a[j] - m); l += a[j]; }
                double* oi = out_host + ((size_t)b * T + i) * D + h * DK;
                for (int j = lo; j < hi; ++j) {
                    a[j] /= l;
                    const float* vj = v_host + ((size_t)b * T + j) * D + h * DK;
                    for (size_t d = 0; d < DK; ++d) oi[d] += a[j] * (double)vj[d];
                }
                if (!dout_host) continue;
                const float* gi = dout_host + ((size_t)b * T + i) * D + h * DK;
                double delta = 0.0;
                for (size_t d = 0; d < DK; ++d) delta += (double)gi[d] * oi[d];
                double* dqi = dq_host + ((size_t)b * T + i) * D + h * DK;
                for (int j = lo; j < hi; ++j) {
                    const size_t kv = ((size_t)b * T + j) * D + h * DK, pp = (size_t)j * D + h * DK;
                    double dpj = 0.0;
                    for (size_t d = 0; d < DK; ++d) dpj += (double)gi[d] * (double)v_host[kv + d];
                    const double ds = a[j] * (dpj - delta) / 8.0;
                    for (size_t d = 0; d < DK; ++d) {
                        const double kd = (double)k_host[kv + d], pd = (double)p_host[pp + d];
                        dv_host[kv + d] += a[j] * (double)gi[d];
                        dqi[d] += ds * (kd + pd);
                        dk_host[kv + d] += ds * ((double)qi[d] + (double)u[d]);
                        dp_host[pp + d] += ds * ((double)qi[d] + (double)vb[d]);
                        du_host[h * DK + d] += ds * kd;
                        dvb_host[h * DK + d] += ds * pd;
                    }
                }
            }
        }
    }
    return RNNT_OK;
}
