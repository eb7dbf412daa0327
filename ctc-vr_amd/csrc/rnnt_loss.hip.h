// Transducer loss with gradients over a caller's joint lattice logits [B][T][U1][V] (rnnt_transducer_loss; torchaudio's
// rnnt_loss): two streaming passes over the lattice with the f64 recursions between them.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
//   loss_pick              read the lattice once: lse [B][T][U1] and pick [B][T][U1][2] in rnnt_transducer_nll's layout
//   transducer_alpha_beta  transducer_alpha's wavefront and its mirror image, both storing their cells (f64)
//   loss_coef              per cell (lse, occ, blank term, label term) as floats: the f64 exponentials leave the streaming pass
//   loss_grad              read the lattice again, write grad [B][T][U1][V]
//
// The lattice passes give 16 lanes (one DPP row) to a cell, so a wave works on four consecutive cells at once: a cell's V logits
// are V * 4 contiguous bytes, read (and written) as float4 from the first 16-byte boundary of the row -- rows of a V that is no
// multiple of 4 start at any of the four phases -- with at most three single floats in front and three behind.  One wave per cell
// left a lane with at most two loads in flight at V = 412 and a chain of dependent latencies per cell (lengths, row, picked
// values): 61 % of the copy rate in loss_pick; the narrow groups put four rows' loads in flight per wave for every V.
// Which lane sums which elements, and in which order, depends only on (cell, V, element type): no atomics, so two launches agree
// bit for bit.
// Cells outside t < T_b, u <= U_b are never read; loss_grad writes zeros there.
// Cell indices are ints (the host refuses B * T * U1 >= 2^31); element offsets cell * V are 64-bit.
//
// The two passes are templates over the lattice element E: float, bfloat16 or float16, for logits AND gradient.  A 16-byte vector
// holds EPV = 16 / sizeof(E) elements, so a 16-bit row starts at any of EIGHT phases and has at most seven single elements in front
// and behind (still fewer than a cell's lanes).  Every element is widened to float exactly on load (a shift, a convert); lse, the
// picks, p_k and g_k are the float32 arithmetic of the float lattice; g_k is clamped in float32 and rounded once, to nearest even,
// by the plain cast at the store.  L is the lanes per cell (16, or 8: half a DPP row, the butterflies stop at xor 4).
#pragma once

#define LOSS_LANES 16            // lanes per cell of a float lattice: one DPP row, so the reductions below need no LDS and no bpermute
#ifndef LOSS_LANES_16BIT_PICK    // lanes per cell of a 16-bit lattice, per pass: 16 against 8 measured at the joint shape,
#define LOSS_LANES_16BIT_PICK 8  // loss_pick is faster with 8 (two batches of loads per lane at V = 412, eight cells per wave),
#endif
#ifndef LOSS_LANES_16BIT_GRAD
#define LOSS_LANES_16BIT_GRAD 16 // loss_grad with 16; -D overrides either for that measurement
#endif
#define LOSS_BATCH 4             // 16-byte loads a lane issues before it uses the first

typedef __bf16 loss_bf16;
typedef _Float16 loss_f16;

// all-reduce over the L lanes of a cell (xor_partner's ascending butterfly: every lane ends with the same bits)
template <int L>
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, xor_partner<1>(v));
    v = fmaxf(v, xor_partner<2>(v));
    v = fmaxf(v, xor_partner<4>(v));
    return L == 16 ? fmaxf(v, xor_partner<8>(v)) : v;
}
template <int L>
__device__ __forceinline__ float row_sum(float v) {
    v += xor_partner<1>(v);
    v += xor_partner<2>(v);
    v += xor_partner<4>(v);
    return L == 16 ? v + xor_partner<8>(v) : v;
}

// One 16-byte vector of the lattice as floats, and the loads and stores of an element type: single elements and whole vectors.
template <typename E>
struct LossVec {
    static constexpr int N = 16 / sizeof(E);
    float x[N];
};
template <typename E>
__device__ __forceinline__ float loss_ld1(const E* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)*(const RNNT_GAS E*)p;
#else
    return (float)*p;
#endif
}
template <typename E>
__device__ __forceinline__ void loss_st1(E* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(RNNT_GAS E*)p = (E)v;
#else
    *p = (E)v;
#endif
}
template <typename E>
__device__ __forceinline__ LossVec<E> loss_ldv(const E* p) {
    typedef E ev __attribute__((ext_vector_type(LossVec<E>::N)));
#if defined(__HIP_DEVICE_COMPILE__)
    const ev v = *(const RNNT_GAS ev*)p;
#else
    const ev v = *reinterpret_cast<const ev*>(p);
#endif
    LossVec<E> o;
#pragma unroll
    for (int j = 0; j < LossVec<E>::N; ++j) o.x[j] = (float)v[j];
    return o;
}
template <typename E>
__device__ __forceinline__ void loss_stv(E* p, const LossVec<E>& o) {
    typedef E ev __attribute__((ext_vector_type(LossVec<E>::N)));
    ev v;
#pragma unroll
    for (int j = 0; j < LossVec<E>::N; ++j) v[j] = (E)o.x[j];
#if defined(__HIP_DEVICE_COMPILE__)
    *(RNNT_GAS ev*)p = v;
#else
    *reinterpret_cast<ev*>(p) = v;
#endif
}
template <typename E>
__device__ __forceinline__ LossVec<E> loss_fill(float v) {
    LossVec<E> o;
#pragma unroll
    for (int j = 0; j < LossVec<E>::N; ++j) o.x[j] = v;
    return o;
}

// exp on v_exp_f32: |x| 2^-24 relative through the product with log2 e, which the terms that matter (x near 0) do not feel
__device__ __forceinline__ float loss_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// cell c -> (b, t, u) and its row's lengths; false for a cell outside the row's valid region
struct LossCell { int b, t, u, Tb, Ub; };
__device__ __forceinline__ bool loss_cell(int c, const int* __restrict__ lens, int B, int T, int U1, LossCell& o) {
    const int bt = c / U1;
    o.u = c - bt * U1;
    o.b = bt / T;
    o.t = bt - o.b * T;
    o.Tb = ldgi(lens + o.b);
    o.Ub = ldgi(lens + B + o.b);
    return o.t < o.Tb && o.u <= o.Ub;
}

// The pieces of row `e0 .. e0 + V` (element offsets from a 16-byte aligned base): head single elements, nvec vectors of EPV, tail
// elements.
struct LossRow { int head, nvec, tail; };
template <int EPV>
__device__ __forceinline__ LossRow loss_row(long long e0, int V) {
    LossRow r;
    r.head = min(V, (int)((EPV - (e0 & (EPV - 1))) & (EPV - 1)));
    r.nvec = (int)((unsigned)(V - r.head) / EPV);
    r.tail = V - r.head - EPV * r.nvec;
    return r;
}

// running (max, sum of exp(x - max)) of one lane; a lane that has seen nothing, or only -inf, holds (-inf, 0).
// One vector: the exponentials are summed as a fixed tree, four by four.  One element: the same with a single term (what a float4
// of (x, -inf, -inf, -inf) gives, bit for bit: its other three terms are +0).
template <int N>
__device__ __forceinline__ void lse_take(float& m, float& s, const float (&x)[N]) {
    static_assert(N == 4 || N == 8, "a 16-byte vector of 4- or 2-byte elements");
    float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if constexpr (N == 8) mx = fmaxf(mx, fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
    const float mn = fmaxf(m, mx);
    const float ms = mn == -INFINITY ? 0.0f : mn;
    float e = (loss_exp(x[0] - ms) + loss_exp(x[1] - ms)) + (loss_exp(x[2] - ms) + loss_exp(x[3] - ms));
    if constexpr (N == 8) e += (loss_exp(x[4] - ms) + loss_exp(x[5] - ms)) + (loss_exp(x[6] - ms) + loss_exp(x[7] - ms));
    s = s * loss_exp(m - ms) + e;
    m = mn;
}
__device__ __forceinline__ void lse_take1(float& m, float& s, float x) {
    const float mn = fmaxf(m, x);
    const float ms = mn == -INFINITY ? 0.0f : mn;
    s = s * loss_exp(m - ms) + loss_exp(x - ms);
    m = mn;
}

// lens [2][B]: T_b in [1, T], U_b in [0, U1 - 1]; targets [B][ts]; labels inside a row's length are in [0, V) (checked on the host).
// fused = 0: the input holds log-probabilities already, lse = 0 and only the two picked values are read.
template <typename E, int L>
__global__ __launch_bounds__(256) void loss_pick(const E* __restrict__ logits, const int* __restrict__ targets, const int* __restrict__ lens,
                                                 int B, int T, int U1, int V, int ts, int blank, int fused, float* __restrict__ lse,
                                                 float* __restrict__ pick) {
    constexpr int EPV = LossVec<E>::N;
    const int lane = threadIdx.x & (L - 1);
    const int ncell = B * T * U1;
    const int c = blockIdx.x * (256 / L) + threadIdx.x / L;    // launched with ceil(cells / (256 / L)) workgroups
    if (c >= ncell) return;
    LossCell q;
    if (!loss_cell(c, lens, B, T, U1, q)) return;              // uniform over the cell's lanes
    const long long e0 = (long long)c * V;
    const E* row = logits + e0;
    float xb = 0.0f, xl = 0.0f;                            // the two picked logits: asked for before the row, not after the reduction
    if (lane == 0) {
        xb = loss_ld1(row + blank);
        if (q.u < q.Ub) xl = loss_ld1(row + ldgi(targets + (long long)q.b * ts + q.u));
    }
    float l = 0.0f;
    if (fused) {
        const LossRow r = loss_row<EPV>(e0, V);
        float m = -INFINITY, s = 0.0f;
        if (lane < r.head) lse_take1(m, s, loss_ld1(row + lane));
        const E* body = row + r.head;
        for (int i = lane; i < r.nvec; i += L * LOSS_BATCH) {
            LossVec<E> v[LOSS_BATCH];
#pragma unroll
            for (int j = 0; j < LOSS_BATCH; ++j) {
                const int ii = i + L * j;
                v[j] = ii < r.nvec ? loss_ldv(body + EPV * (long long)ii) : loss_fill<E>(-INFINITY);
            }
#pragma unroll
            for (int j = 0; j < LOSS_BATCH; ++j) lse_take(m, s, v[j].x);
        }
        if (lane < r.tail) lse_take1(m, s, loss_ld1(body + EPV * (long long)r.nvec + lane));
        const float M = row_max<L>(m);
        const float Ms = M == -INFINITY ? 0.0f : M;
        const float S = row_sum<L>(s * loss_exp(m - Ms));
        l = Ms + logf(S);
    }
    if (lane == 0) {
        stg1(lse + c, l);
        stg1(pick + 2 * (long long)c, xb - l);
        if (q.u < q.Ub) stg1(pick + 2 * (long long)c + 1, xl - l);
    }
}

// transducer_alpha (rnnt_score.hip.h) storing every cell, and the backward recursion as the same wavefront run from the far corner:
//   beta[T_b-1,U_b] = pick[T_b-1,U_b][0];  beta[t,u] = logaddexp(beta[t+1,u] + pick[t,u][0], beta[t,u+1] + pick[t,u][1]).
// Workgroup 2 b runs alpha of row b, 2 b + 1 its beta: on diagonal d (counted from the far corner) thread u owns cell
// (T_b - 1 - (d - (U_b - u)), u), keeps its own beta in a register and reads thread u + 1's from LDS.  alpha, beta [B][T][U1] f64
// (valid cells only); nll_alpha[b] = -(alpha[T_b-1,U_b] + pick[T_b-1,U_b][0]) and nll[b] = -beta[0,0] are the same likelihood.
// Launched with 256 threads, U1 <= 256.
__global__ __launch_bounds__(256) void transducer_alpha_beta(const float* __restrict__ pick, const int* __restrict__ lens, int B, int T, int U1,
                                                             double* __restrict__ alpha, double* __restrict__ beta,
                                                             double* __restrict__ nll_alpha, double* __restrict__ nll) {
    __shared__ double xa[2][SCORE_UMAX + 1];
    const int b = blockIdx.x >> 1, u = threadIdx.x;
    const bool back = blockIdx.x & 1;
    const int Tb = ldgi(lens + b), Ub = ldgi(lens + B + b);
    const long long cb = (long long)b * T * U1;
    const float* pb = pick + cb * 2;
    const int nd = Tb + Ub;
    double a = -INFINITY;
    if (!back) {
        double* ab = alpha + cb;
        for (int d = 0; d < nd; ++d) {
            const int t = d - u;
            const bool live = u <= Ub && t >= 0 && t < Tb;
            if (live) {
                if (d == 0) a = 0.0;
                else {
                    const double below = t > 0 ? a + (double)ldg1(pb + ((long long)(t - 1) * U1 + u) * 2) : -INFINITY;
                    const double left = u > 0 ? xa[(d - 1) & 1][u - 1] + (double)ldg1(pb + ((long long)t * U1 + u - 1) * 2 + 1) : -INFINITY;
                    a = t == 0 ? left : (u == 0 ? below : score_logaddexp(below, left));
                }
                ab[(long long)t * U1 + u] = a;
            }
            xa[d & 1][u] = a;
            __syncthreads();
        }
        if (u == Ub) nll_alpha[b] = -(a + (double)ldg1(pb + ((long long)(Tb - 1) * U1 + Ub) * 2));
    } else {
        double* bb = beta + cb;
        for (int d = 0; d < nd; ++d) {
            const int t = Tb - 1 - (d - (Ub - u));
            const bool live = u <= Ub && t >= 0 && t < Tb;
            if (live) {
                const float* cell = pb + ((long long)t * U1 + u) * 2;
                const double blank = (double)ldg1(cell);
                if (d == 0) a = blank;
                else {
                    // `a` still holds beta[t+1,u] (the cell this thread owned on diagonal d - 1), the neighbour's beta[t,u+1] is in LDS
                    const double up = t + 1 < Tb ? a + blank : -INFINITY;
                    const double right = u < Ub ? xa[(d - 1) & 1][u + 1] + (double)ldg1(cell + 1) : -INFINITY;
                    a = t == Tb - 1 ? right : (u == Ub ? up : score_logaddexp(up, right));
                }
                bb[(long long)t * U1 + u] = a;
            }
            xa[d & 1][u] = a;
            __syncthreads();
        }
        if (u == 0) nll[b] = -a;
    }
}

// One thread per valid cell, with logZ = beta[0,0]:
//   coef[c] = (lse, occ = exp(alpha + beta - logZ), blank term = exp(alpha + pick[0] + beta[t+1,u] - logZ), label term =
//   exp(alpha + pick[1] + beta[t,u+1] - logZ)); at t = T_b - 1 the blank term exists only at u = U_b, with beta[T_b,U_b] := 0; the
//   label term only for u < U_b.  fused = 0 stores occ = 0: the p_k occ part of the gradient is dropped.
// The sums and the exponentials are f64, the stored values float (all in [0, 1]).
__global__ __launch_bounds__(256) void loss_coef(const float* __restrict__ pick, const float* __restrict__ lse, const double* __restrict__ alpha,
                                                 const double* __restrict__ beta, const int* __restrict__ lens, int B, int T, int U1, int fused,
                                                 float* __restrict__ coef) {
    const int ncell = B * T * U1;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += gridDim.x * blockDim.x) {
        LossCell q;
        if (!loss_cell(c, lens, B, T, U1, q)) continue;
        const double logZ = beta[(long long)q.b * T * U1];
        const double a = alpha[c];
        const double occ = fused ? exp(a + beta[c] - logZ) : 0.0;
        double tb = 0.0, tl = 0.0;
        const double pbl = (double)ldg1(pick + 2 * (long long)c);
        if (q.t < q.Tb - 1) tb = exp(a + pbl + beta[c + U1] - logZ);
        else if (q.u == q.Ub) tb = exp(a + pbl - logZ);
        if (q.u < q.Ub) tl = exp(a + (double)ldg1(pick + 2 * (long long)c + 1) + beta[c + 1] - logZ);
        stg4(coef + 4 * (long long)c, make_float4(ldg1(lse + c), (float)occ, (float)tb, (float)tl));
    }
}

// g_k = p_k occ - [k = blank] blank term - [k = y_{u+1}] label term with p_k = exp(logit_k - lse), clamped to [-clamp, clamp] when
// clamp > 0.  FUSED = false: no p_k occ part, the lattice is not read.  Every element of a cell outside the valid region is 0.
template <bool FUSED>
__device__ __forceinline__ float loss_g(float x, int k, float4 cf, int blank, int y, float clamp) {
    float g = FUSED ? loss_exp(x - cf.x) * cf.y : 0.0f;
    g -= k == blank ? cf.z : 0.0f;
    g -= k == y ? cf.w : 0.0f;
    return clamp > 0.0f ? fminf(fmaxf(g, -clamp), clamp) : g;
}

template <typename E, int L, bool FUSED>
__global__ __launch_bounds__(256) void loss_grad(const E* __restrict__ logits, const int* __restrict__ targets, const int* __restrict__ lens,
                                                 const float* __restrict__ coef, int B, int T, int U1, int V, int ts, int blank, float clamp,
                                                 E* __restrict__ grad) {
    constexpr int EPV = LossVec<E>::N;
    const int lane = threadIdx.x & (L - 1);
    const int ncell = B * T * U1;
    const int c = blockIdx.x * (256 / L) + threadIdx.x / L;    // launched with ceil(cells / (256 / L)) workgroups
    if (c >= ncell) return;
    LossCell q;
    const bool valid = loss_cell(c, lens, B, T, U1, q);
    const long long e0 = (long long)c * V;
    const LossRow r = loss_row<EPV>(e0, V);
    const E* row = logits + e0;
    E* out = grad + e0;
    const E* body = row + r.head;
    E* obody = out + r.head;
    const int t0 = r.head + EPV * r.nvec;                  // first element of the tail
    if (!valid) {                                          // uniform over the cell's lanes
        const LossVec<E> z = loss_fill<E>(0.0f);
        if (lane < r.head) loss_st1(out + lane, 0.0f);
        for (int i = lane; i < r.nvec; i += L) loss_stv(obody + EPV * (long long)i, z);
        if (lane < r.tail) loss_st1(out + t0 + lane, 0.0f);
        return;
    }
    const float4 cf = ldg4(coef + 4 * (long long)c);
    const int y = q.u < q.Ub ? ldgi(targets + (long long)q.b * ts + q.u) : -1;
    if (lane < r.head) loss_st1(out + lane, loss_g<FUSED>(FUSED ? loss_ld1(row + lane) : 0.0f, lane, cf, blank, y, clamp));
    for (int i = lane; i < r.nvec; i += L * LOSS_BATCH) {
        LossVec<E> v[LOSS_BATCH];
#pragma unroll
        for (int j = 0; j < LOSS_BATCH; ++j) {
            const int ii = i + L * j;
            v[j] = FUSED && ii < r.nvec ? loss_ldv(body + EPV * (long long)ii) : loss_fill<E>(0.0f);
        }
#pragma unroll
        for (int j = 0; j < LOSS_BATCH; ++j) {
            const int ii = i + L * j, k = r.head + EPV * ii;
            if (ii < r.nvec) {
                LossVec<E> g;
#pragma unroll
                for (int n = 0; n < EPV; ++n) g.x[n] = loss_g<FUSED>(v[j].x[n], k + n, cf, blank, y, clamp);
                loss_stv(obody + EPV * (long long)ii, g);
            }
        }
    }
    if (lane < r.tail) loss_st1(out + t0 + lane, loss_g<FUSED>(FUSED ? loss_ld1(row + t0 + lane) : 0.0f, t0 + lane, cf, blank, y, clamp));
}
