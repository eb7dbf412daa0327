// CTC loss with gradients over a caller's logits or log-probabilities (rnnt_ctc_loss; torch.nn.functional.ctc_loss): two
// streaming passes over [B][T][V] with the f64 recursions over the extended states between them.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
//   ctc_loss_pick    read every valid frame once: lse [B][T] and pick [B][T][L1], pick[0] = log P(blank), pick[1 + i] = log P(y_i)
//   ctc_alpha_beta   ctc_alpha's recursion storing its states, and its mirror image run from the last frame (f64)
//   ctc_loss_occ     per frame and distinct column the summed state occupancies, as floats: the f64 exponentials leave the streaming pass
//   ctc_loss_grad    read the frames again, write grad [B][T][V]
//
// A frame (b, t) is the V elements from element offset b * stride_b + t * stride_t of a 16-byte aligned base: [B, T, V], [T, B, V]
// and the transposed view of either are the same kernel.  The streaming passes give 16 lanes (one DPP row) to a frame, so a wave
// works on four frames.  A frame is cut into CHUNKS of 8 consecutive COLUMNS, chunk c belongs to lane c % 16, and a lane folds its
// chunks in ascending order with lse_take's fixed tree: which lane sums which columns, and in which order, depends on V alone --
// not on where the row starts, not on the element type.  So the layouts agree bit for bit, and a 16-bit input gives the bits of the
// float32 call on the widened input.  Only the ACCESS WIDTH follows the row's alignment: a chunk is read (and its gradient written)
// in pieces of the largest power of two of elements, at most 16 bytes, that the row's offset is a multiple of -- one or two
// 16-byte accesses for a row that starts on 16 bytes, single elements for an odd offset.
// No atomics anywhere: several extended states on one column (a repeated label, and always the blank) are summed by ONE thread of
// ctc_loss_occ in ascending state order, from a table the host builds from the host targets.  Two calls agree bit for bit.
// Frames t >= T_b are never read; ctc_loss_grad writes zeros there and in every frame of a row whose nll is +inf.
// Frame and state indices are ints (the host refuses B * T * (2 Lmax + 1) >= 2^31 - 1); element offsets are 64-bit.
#pragma once

#define CTC_LOSS_LANES 16        // lanes per frame, for every element type: the reduction order must not depend on it
#define CTC_LOSS_BATCH 4         // chunks a lane asks for before it uses the first
#define CTC_LOSS_STEPS 8         // recursion steps whose picks are loaded, and whose states are stored, together

// 8 consecutive elements as 8 / A accesses of A elements (A * sizeof(E) <= 16 bytes, p aligned to that)
template <typename E, int A>
__device__ __forceinline__ void ctc_ld_by(const E* p, float (&x)[8]) {
    if constexpr (A == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = loss_ld1(p + j);
    } else {
        typedef E ev __attribute__((ext_vector_type(A)));
#pragma unroll
        for (int i = 0; i < 8 / A; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
            const ev v = *(const RNNT_GAS ev*)(p + A * i);
#else
            const ev v = *reinterpret_cast<const ev*>(p + A * i);
#endif
#pragma unroll
            for (int j = 0; j < A; ++j) x[A * i + j] = (float)v[j];
        }
    }
}
template <typename E, int A>
__device__ __forceinline__ void ctc_st_by(E* p, const float (&x)[8]) {
    if constexpr (A == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) loss_st1(p + j, x[j]);
    } else {
        typedef E ev __attribute__((ext_vector_type(A)));
#pragma unroll
        for (int i = 0; i < 8 / A; ++i) {
            ev v;
#pragma unroll
            for (int j = 0; j < A; ++j) v[j] = (E)x[A * i + j];
#if defined(__HIP_DEVICE_COMPILE__)
            *(RNNT_GAS ev*)(p + A * i) = v;
#else
            *reinterpret_cast<ev*>(p + A * i) = v;
#endif
        }
    }
}
// gran: the largest power of two (at most 8) of elements that the row's offset is a multiple of; uniform over a frame's lanes
__device__ __forceinline__ int ctc_gran(long long e0) { return (int)((e0 | 8) & -(e0 | 8)); }
template <typename E>
__device__ __forceinline__ void ctc_ld8(const E* p, int gran, float (&x)[8]) {
    constexpr int MAXA = sizeof(E) == 4 ? 4 : 8;
    if (gran >= MAXA) ctc_ld_by<E, MAXA>(p, x);
    else if (MAXA == 8 && gran == 4) ctc_ld_by<E, 4>(p, x);
    else if (gran == 2) ctc_ld_by<E, 2>(p, x);
    else ctc_ld_by<E, 1>(p, x);
}
template <typename E>
__device__ __forceinline__ void ctc_st8(E* p, int gran, const float (&x)[8]) {
    constexpr int MAXA = sizeof(E) == 4 ? 4 : 8;
    if (gran >= MAXA) ctc_st_by<E, MAXA>(p, x);
    else if (MAXA == 8 && gran == 4) ctc_st_by<E, 4>(p, x);
    else if (gran == 2) ctc_st_by<E, 2>(p, x);
    else ctc_st_by<E, 1>(p, x);
}

// frame f -> (b, t), its element offset and whether t < T_b
struct CtcFrame { int b, t; long long e0; };
__device__ __forceinline__ bool ctc_frame(int f, const int* __restrict__ lens, int T, long long sb, long long st, CtcFrame& o) {
    o.b = f / T;
    o.t = f - o.b * T;
    o.e0 = o.b * sb + o.t * st;
    return o.t < ldgi(lens + o.b);
}

// lens [2][B]: T_b in [1, T], L_b in [0, L1 - 1]; targets [B][ts]; labels inside a row's length are in [0, V) (checked on the host).
// fused = 0: the input holds log-probabilities already, lse = 0 and only the picked values are read.
// Launched with ceil(B T / 16) workgroups of 256.
template <typename E>
__global__ __launch_bounds__(256) void ctc_loss_pick(const E* __restrict__ logits, long long sb, long long st, const int* __restrict__ targets,
                                                     const int* __restrict__ lens, int B, int T, int L1, int V, int ts, int blank, int fused,
                                                     float* __restrict__ lse, float* __restrict__ pick) {
    constexpr int L = CTC_LOSS_LANES;
    const int lane = threadIdx.x & (L - 1);
    const int f = blockIdx.x * (256 / L) + threadIdx.x / L;
    if (f >= B * T) return;
    CtcFrame q;
    if (!ctc_frame(f, lens, T, sb, st, q)) return;           // uniform over the frame's lanes
    const int Lb = ldgi(lens + B + q.b);
    const E* row = logits + q.e0;
    float l = 0.0f;
    if (fused) {
        const int gran = ctc_gran(q.e0), nfull = V >> 3, rem = V & 7;
        float m = -INFINITY, s = 0.0f;
        for (int c = lane; c < nfull; c += L * CTC_LOSS_BATCH) {
            float x[CTC_LOSS_BATCH][8];
#pragma unroll
            for (int j = 0; j < CTC_LOSS_BATCH; ++j) {
                const int cc = c + L * j;
                if (cc < nfull) ctc_ld8(row + 8 * (long long)cc, gran, x[j]);
                else {
#pragma unroll
                    for (int n = 0; n < 8; ++n) x[j][n] = -INFINITY;   // folds to nothing, exactly
                }
            }
#pragma unroll
            for (int j = 0; j < CTC_LOSS_BATCH; ++j) lse_take(m, s, x[j]);
        }
        if (rem && lane == (nfull & (L - 1))) {                // the last, short chunk: after its lane's whole ones
            float x[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) x[n] = n < rem ? loss_ld1(row + 8 * (long long)nfull + n) : -INFINITY;
            lse_take(m, s, x);
        }
        const float M = row_max<L>(m);
        const float Ms = M == -INFINITY ? 0.0f : M;
        const float S = row_sum<L>(s * loss_exp(m - Ms));
        l = Ms + logf(S);
    }
    float* pf = pick + (long long)f * L1;
    for (int j = lane; j <= Lb; j += L) {
        const int col = j ? ldgi(targets + (long long)q.b * ts + j - 1) : blank;
        stg1(pf + j, loss_ld1(row + col) - l);
    }
    if (lane == 0) stg1(lse + f, l);
}

// ctc_alpha (rnnt_score.hip.h) over the picked values, storing its states, and the backward recursion as its mirror image:
//   alpha_0[s] = lp_0[ext s] for s < 2;  alpha_t[s] = logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if y differs) + lp_t[ext s]
//   beta_{T_b-1}[s] = lp[ext s] for s >= S - 2;  beta_t[s] = logsumexp(beta_{t+1}[s], beta_{t+1}[s+1], beta_{t+1}[s+2] if y differs) + lp_t[ext s]
// (both hold their own frame's lp, torch's convention: alpha_t[s] + beta_t[s] - lp_t[ext s] is the log-mass of the paths through s
// at t).  nll[b] = -logaddexp(alpha[S-1], alpha[S-2]) at the last frame, nll_beta[b] = -logaddexp(beta[0], beta[1]) at the first:
// the same likelihood; +inf for a transcript its frames cannot hold.
// both = 1: 2 B workgroups, 2 b runs alpha of row b and 2 b + 1 its beta, states stored [B][T][S1] (valid ones only).  both = 0: B
// workgroups, alpha only, nothing stored but nll: the same bits.  Thread s owns state s, keeps it in a register and hands it to its
// neighbours through LDS (two buffers: one barrier per frame).  The picks of CTC_LOSS_STEPS frames are asked for together and the
// states of those frames stored together, so the chain waits for memory once per CTC_LOSS_STEPS barriers, not at every one.
// pick [B][T][L1]; S1 = 2 L1 - 1; launched with 512 threads.
__global__ __launch_bounds__(512) void ctc_alpha_beta(const float* __restrict__ pick, const int* __restrict__ targets, const int* __restrict__ lens,
                                                      int B, int T, int L1, int ts, int both, double* __restrict__ alpha, double* __restrict__ beta,
                                                      double* __restrict__ nll, double* __restrict__ nll_beta) {
    __shared__ double xa[2][2 * SCORE_UMAX + 2];
    const int b = both ? blockIdx.x >> 1 : blockIdx.x, s = threadIdx.x;
    const bool back = both && (blockIdx.x & 1);
    const int Tb = ldgi(lens + b), Lb = ldgi(lens + B + b);
    const int S = 2 * Lb + 1, S1 = 2 * L1 - 1;
    const bool live = s < S;
    int slot = 0, skip = 0;
    if (live && (s & 1)) {
        const int* yb = targets + (long long)b * ts;
        const int i = s >> 1, y = ldgi(yb + i);
        slot = 1 + i;
        skip = back ? (i + 1 < Lb && ldgi(yb + i + 1) != y) : (i >= 1 && ldgi(yb + i - 1) != y);
    }
    const int t0 = back ? Tb - 1 : 0, dir = back ? -1 : 1;       // step n works on frame t0 + dir * n
    const int d1 = back ? 1 : -1;                              // the neighbour states are s + d1 and (skip) s + 2 d1
    const bool has1 = back ? s + 1 < S : s >= 1;
    const float* pk = pick + (long long)b * T * L1 + slot;
    double* out = (back ? beta : alpha) + (long long)b * T * S1 + s;
    const bool store = both && live;
    double a = live && (back ? s >= S - 2 : s < 2) ? (double)ldg1(pk + (long long)t0 * L1) : -INFINITY;
    xa[0][s] = a;
    if (store) out[(long long)t0 * S1] = a;
    __syncthreads();
    for (int n0 = 1; n0 < Tb; n0 += CTC_LOSS_STEPS) {
        float lp[CTC_LOSS_STEPS];
        double av[CTC_LOSS_STEPS];
#pragma unroll
        for (int j = 0; j < CTC_LOSS_STEPS; ++j) lp[j] = live && n0 + j < Tb ? ldg1(pk + (long long)(t0 + dir * (n0 + j)) * L1) : 0.0f;
#pragma unroll
        for (int j = 0; j < CTC_LOSS_STEPS; ++j) {
            const int n = n0 + j;
            if (n < Tb) {                                      // uniform over the workgroup
                if (live) {
                    const double* pv = xa[(n - 1) & 1];
                    const double a1 = has1 ? pv[s + d1] : -INFINITY, a2 = skip ? pv[s + 2 * d1] : -INFINITY;
                    double mx = fmax(a, fmax(a1, a2));
                    if (mx == -INFINITY) mx = 0.0;
                    a = log(exp(a - mx) + exp(a1 - mx) + exp(a2 - mx)) + mx + (double)lp[j];
                }
                av[j] = a;
                xa[n & 1][s] = a;
                __syncthreads();
            }
        }
        if (store) {
#pragma unroll
            for (int j = 0; j < CTC_LOSS_STEPS; ++j)
                if (n0 + j < Tb) out[(long long)(t0 + dir * (n0 + j)) * S1] = av[j];
        }
    }
    const double* last = xa[(Tb - 1) & 1];
    if (!back && s == S - 1) nll[b] = -score_logaddexp(a, S > 1 ? last[S - 2] : -INFINITY);
    if (back && s == 0) nll_beta[b] = -score_logaddexp(a, S > 1 ? last[1] : -INFINITY);
}

// One thread per (frame, entry): the row's entries are its distinct columns in ascending order -- the blank and every distinct
// label -- cnt [B] of them, cols [B][L1]; entry j owns the extended states pos[b][ptr[b][j] .. ptr[b][j+1]), ascending (ptr [B][L1 + 1],
// pos [B][S1]; built on the host).
//   occ[f][j] = sum over those states of exp(alpha_t[s] + beta_t[s] - lp_t[col] + nll_b), added in that order.
// f64 sums and exponentials, the stored value float (in [0, 1] up to rounding).  Frames t >= T_b and rows with nll = +inf are skipped.
__global__ __launch_bounds__(256) void ctc_loss_occ(const float* __restrict__ pick, const double* __restrict__ alpha, const double* __restrict__ beta,
                                                    const double* __restrict__ nll, const int* __restrict__ lens, const int* __restrict__ cnt,
                                                    const int* __restrict__ ptr, const int* __restrict__ pos, int B, int T, int L1,
                                                    float* __restrict__ occ) {
    const int n = B * T * L1, S1 = 2 * L1 - 1;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        const int f = c / L1, j = c - f * L1, b = f / T, t = f - b * T;
        if (t >= ldgi(lens + b) || j >= ldgi(cnt + b)) continue;
        const double z = nll[b];
        if (!(z < INFINITY)) continue;
        const int* ps = pos + (long long)b * S1;
        const int i0 = ldgi(ptr + (long long)b * (L1 + 1) + j), i1 = ldgi(ptr + (long long)b * (L1 + 1) + j + 1);
        const long long sf = (long long)f * S1;
        const int s0 = ldgi(ps + i0);
        const double lp = (double)ldg1(pick + (long long)f * L1 + ((s0 & 1) ? 1 + (s0 >> 1) : 0));   // one column, one lp
        double sum = 0.0;
        for (int i = i0; i < i1; ++i) {
            const int s = ldgi(ps + i);
            const double ab = alpha[sf + s] + beta[sf + s];
            if (ab > -INFINITY) sum += exp(ab - lp + z);
        }
        occ[c] = (float)sum;
    }
}

// A lane walks its columns in ascending order, so it finds a column's occupancy with a cursor into the row's ascending entries.
struct CtcCursor { const int* cols; const float* occ; int n, cur, next; };
__device__ __forceinline__ void ctc_seek(CtcCursor& c, int k) {   // the first entry with column >= k
    while (c.next < k) {
        ++c.cur;
        c.next = c.cur < c.n ? ldgi(c.cols + c.cur) : 0x7fffffff;
    }
}
template <bool FUSED>
__device__ __forceinline__ float ctc_g(CtcCursor& c, float x, int k, float lse) {
    const float p = FUSED ? loss_exp(x - lse) : 0.0f;
    ctc_seek(c, k);
    return c.next == k ? p - ldg1(c.occ + c.cur) : p;
}

// g_k = p_k - occ_k with p_k = exp(logit_k - lse) (FUSED), or -occ_k (the input holds log-probabilities: it is not read).  occ_k is 0
// for a column that is no entry of the row.  Every element of a frame t >= T_b, and of a row whose nll is +inf, is 0.
// Launched with ceil(B T / 16) workgroups of 256: every element of [B][T][V] is written exactly once.
template <typename E, bool FUSED>
__global__ __launch_bounds__(256) void ctc_loss_grad(const E* __restrict__ logits, long long sb, long long st, const int* __restrict__ lens,
                                                     const int* __restrict__ cnt, const int* __restrict__ cols, const float* __restrict__ lse,
                                                     const float* __restrict__ occ, const double* __restrict__ nll, int B, int T, int L1, int V,
                                                     E* __restrict__ grad) {
    constexpr int L = CTC_LOSS_LANES;
    const int lane = threadIdx.x & (L - 1);
    const int f = blockIdx.x * (256 / L) + threadIdx.x / L;
    if (f >= B * T) return;
    CtcFrame q;
    const bool valid = ctc_frame(f, lens, T, sb, st, q) && nll[q.b] < INFINITY;   // uniform over the frame's lanes
    const int gran = ctc_gran(q.e0), nfull = V >> 3, rem = V & 7;
    const E* row = logits + q.e0;
    E* out = grad + q.e0;
    const bool last = rem && lane == (nfull & (L - 1));
    if (!valid) {
        const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int c = lane; c < nfull; c += L) ctc_st8(out + 8 * (long long)c, gran, z);
        if (last)
            for (int n = 0; n < rem; ++n) loss_st1(out + 8 * (long long)nfull + n, 0.0f);
        return;
    }
    const float l = ldg1(lse + f);
    CtcCursor cu;
    cu.cols = cols + (long long)q.b * L1;
    cu.occ = occ + (long long)f * L1;
    cu.n = ldgi(cnt + q.b);
    cu.cur = 0;
    cu.next = ldgi(cu.cols);                                   // every row has the blank's entry
    for (int c = lane; c < nfull; c += L * CTC_LOSS_BATCH) {
        float x[CTC_LOSS_BATCH][8];
#pragma unroll
        for (int j = 0; j < CTC_LOSS_BATCH; ++j) {
            const int cc = c + L * j;
            if (FUSED && cc < nfull) ctc_ld8(row + 8 * (long long)cc, gran, x[j]);
        }
#pragma unroll
        for (int j = 0; j < CTC_LOSS_BATCH; ++j) {
            const int cc = c + L * j, k = 8 * cc;
            if (cc < nfull) {
                float g[8];
                ctc_seek(cu, k);
                if (cu.next >= k + 8) {                        // no entry among these columns: the common case
#pragma unroll
                    for (int n = 0; n < 8; ++n) g[n] = FUSED ? loss_exp(x[j][n] - l) : 0.0f;
                } else {
#pragma unroll
                    for (int n = 0; n < 8; ++n) g[n] = ctc_g<FUSED>(cu, FUSED ? x[j][n] : 0.0f, k + n, l);
                }
                ctc_st8(out + 8 * (long long)cc, gran, g);
            }
        }
    }
    if (last)
        for (int n = 0; n < rem; ++n) {
            const int k = 8 * nfull + n;
            loss_st1(out + k, ctc_g<FUSED>(cu, FUSED ? loss_ld1(row + k) : 0.0f, k, l));
        }
}
