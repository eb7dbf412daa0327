// The predictor's LSTM layer over a whole label sequence, with its backward (rnnt_lstm_forward / rnnt_lstm_backward, api_lstm.hip.inc).
// Input 256, hidden 256, one layer, gate order i, f, g, o (torch.nn.LSTM).  float32 throughout; the activations are the inference
// predictor's (sigmoidf_, tanhf: EPI_LSTM of rnnt_gemm.hip.h), so the two differ in summation order only.
//
//   lstm_pack_whh   W_hh [1024][256] -> whh_il [256 k][256 j][4 gates]: a lane reads i, f, g, o of ONE hidden unit as one float4
//   lstm_gemm<MODE> the contractions outside the recurrence on v_mfma_f32_16x16x4_f32 (exact f32), 64 x 64 tiles, no LDS:
//                   0  xg = x W_ih^T + (b_ih + b_hh)   1  dx = dG W_ih   2  dW_ih slab = dG^T x   3  dW_hh slab = dG^T h_prev
//   lstm_seq_fwd    the recurrence u = 0 .. U1-1 in ONE launch: one workgroup per LSTM_ROWS batch rows, no workgroup waits on another
//   lstm_seq_bwd    back-propagation through time u = U1-1 .. 0 in ONE launch, same partition
//   lstm_db_part, lstm_slab_reduce   db slabs; slab partials summed in index order
//
// Row tile: LSTM_ROWS = 4 batch rows per workgroup of 1024 threads.  Every workgroup streams all of W_hh (1 MiB) from L2 once per
// step whatever its height, and that stream, not the arithmetic, bounds a step; 4 rows keep the 16 multiply-adds per loaded float4
// under it and spread B = 16 over 4 CUs and B = 64 over 16.  At that height a 16-row MFMA tile would be three quarters padding, so
// the recurrences' contractions are fmaf chains: thread (q, j) takes a quarter (forward: 64 k) or a sixteenth (backward: 64 gate
// columns) of the sum for 4 rows, the partials meet in LDS and are added in index order.  No atomics anywhere: two calls agree bit for bit.
#pragma once

#define LSTM_HID 256
#define LSTM_GATES 1024
#define LSTM_ROWS 4
#define LSTM_THREADS 1024
#define LSTM_KSLAB 256                                             // rows of dG per dW / db slab
#define LSTM_STATE 1280                                            // saved floats per row and step: i, f, g, o (activated), c
#define LSTM_FWD_LDS ((4 * 4 * 256 + 256) * 16)                    // partial gates [4 q][4 r][256 j] float4 | h [256 k] float4 (4 rows)
#define LSTM_BWD_LDS ((16 * 4 * 256) * 4 + 1024 * 16)              // partial dh [16 q][4 r][256 j] | dG [1024 n] float4 (4 rows)

struct LstmP {
    const float *xg, *whh_il, *w_hh, *h0, *c0, *dout;
    const int* lens;                                               // [B] valid steps per row (device)
    float *out, *hn, *cn, *state, *dg, *dh0, *dc0;
    int B, U1;
};

__global__ void lstm_pack_whh(const float* __restrict__ w_hh, float* __restrict__ whh_il) {
    const int idx = blockIdx.x * 256 + threadIdx.x;                // (j, k), k fastest: coalesced reads
    const int j = idx >> 8, k = idx & 255;
    stg4(whh_il + ((size_t)k * LSTM_HID + j) * 4, make_float4(ldg1(w_hh + (size_t)(0 * LSTM_HID + j) * LSTM_HID + k), ldg1(w_hh + (size_t)(1 * LSTM_HID + j) * LSTM_HID + k),
                                                              ldg1(w_hh + (size_t)(2 * LSTM_HID + j) * LSTM_HID + k), ldg1(w_hh + (size_t)(3 * LSTM_HID + j) * LSTM_HID + k)));
}

// the longest row of a workgroup's tile: steps beyond it are skipped by the whole workgroup
__device__ __forceinline__ int lstm_tile_steps(const int* lens, int B, int tile) {
    int t = 0;
#pragma unroll
    for (int r = 0; r < LSTM_ROWS; ++r) {
        const int b = tile * LSTM_ROWS + r;
        t = max(t, b < B ? ldgi(lens + b) : 0);
    }
    return t;
}

__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_fwd(LstmP p) {
    extern __shared__ float4 lstm_lds[];
    float4* red = lstm_lds;                                        // [q][r][j]: thread (q, j)'s quarter of row r's four gates of unit j
    float4* hs = lstm_lds + 4 * 4 * 256;                           // [k]: h[0..3][k]
    const int tid = threadIdx.x, q = tid >> 8, j = tid & 255;
    const int b = blockIdx.x * LSTM_ROWS + q;                      // the row whose cell (b, j) this thread keeps
    const int len = b < p.B ? ldgi(p.lens + b) : 0;
    const int steps = lstm_tile_steps(p.lens, p.B, blockIdx.x);
    float h = 0.f, c = 0.f;
    if (len > 0) {
        if (p.h0) h = ldg1(p.h0 + (size_t)b * LSTM_HID + j);
        if (p.c0) c = ldg1(p.c0 + (size_t)b * LSTM_HID + j);
    }
    ((float*)hs)[j * 4 + q] = h;
    __syncthreads();
    const float* wq = p.whh_il + ((size_t)(q * 64) * LSTM_HID + j) * 4;
    for (int u = 0; u < p.U1; ++u) {
        const size_t row = (size_t)b * p.U1 + u;
        if (u >= steps) {                                          // uniform: no row of the tile is live any more
            if (b < p.B) stg1(p.out + row * LSTM_HID + j, 0.f);
            continue;
        }
        const bool live = u < len;
        float xi = 0.f, xf = 0.f, xc = 0.f, xo = 0.f;
        if (live) {
            const float* xr = p.xg + row * LSTM_GATES + j;
            xi = ldg1(xr); xf = ldg1(xr + 256); xc = ldg1(xr + 512); xo = ldg1(xr + 768);
        }
        float acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[r][g] = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < 64; ++kk) {
            const float4 w = ldg4(wq + (size_t)kk * (LSTM_HID * 4));
            const float4 hv = hs[q * 64 + kk];
            const float hr[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[r][0] = fmaf(hr[r], w.x, acc[r][0]);
                acc[r][1] = fmaf(hr[r], w.y, acc[r][1]);
                acc[r][2] = fmaf(hr[r], w.z, acc[r][2]);
                acc[r][3] = fmaf(hr[r], w.w, acc[r][3]);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(q * 4 + r) * 256 + j] = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
        __syncthreads();
        float4 s = red[(0 * 4 + q) * 256 + j];
#pragma unroll
        for (int qq = 1; qq < 4; ++qq) {                           // quarters in index order
            const float4 t = red[(qq * 4 + q) * 256 + j];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        if (live) {
            const float gi = sigmoidf_(xi + s.x), gf = sigmoidf_(xf + s.y), gg = tanhf(xc + s.z), go = sigmoidf_(xo + s.w);
            c = gf * c + gi * gg;
            h = go * tanhf(c);
            stg1(p.out + row * LSTM_HID + j, h);
            if (p.state) {
                float* st = p.state + row * LSTM_STATE + j;
                stg1(st, gi); stg1(st + 256, gf); stg1(st + 512, gg); stg1(st + 768, go); stg1(st + 1024, c);
            }
            ((float*)hs)[j * 4 + q] = h;
        } else if (b < p.B) {
            stg1(p.out + row * LSTM_HID + j, 0.f);
        }
        __syncthreads();
    }
    if (len > 0) {
        if (p.hn) stg1(p.hn + (size_t)b * LSTM_HID + j, h);
        if (p.cn) stg1(p.cn + (size_t)b * LSTM_HID + j, c);
    }
}

__global__ __launch_bounds__(LSTM_THREADS) void lstm_seq_bwd(LstmP p) {
    extern __shared__ float4 lstm_lds[];
    float* red = (float*)lstm_lds;                                 // [q][r][j]: wave q's sixteenth of dh_rec[r][j]
    float4* gs = lstm_lds + 16 * 4 * 256 / 4;                      // [n]: dG[0..3][n], n = gate * 256 + unit
    const int tid = threadIdx.x, r = tid >> 8, j = tid & 255, wq = tid >> 6, j4 = tid & 63;
    const int b = blockIdx.x * LSTM_ROWS + r;
    const int len = b < p.B ? ldgi(p.lens + b) : 0;
    const int steps = lstm_tile_steps(p.lens, p.B, blockIdx.x);
    float dh_rec = 0.f, dc = 0.f;
    const float* wn = p.w_hh + (size_t)(wq * 64) * LSTM_HID + j4 * 4;
    for (int u = p.U1 - 1; u >= 0; --u) {
        const size_t row = (size_t)b * p.U1 + u;
        float* dgr = p.dg + row * LSTM_GATES + j;
        if (u >= steps) {                                          // uniform
            if (b < p.B) { stg1(dgr, 0.f); stg1(dgr + 256, 0.f); stg1(dgr + 512, 0.f); stg1(dgr + 768, 0.f); }
            continue;
        }
        const bool live = u < len;
        float d_i = 0.f, d_f = 0.f, d_g = 0.f, d_o = 0.f;
        if (live) {
            const float* st = p.state + row * LSTM_STATE + j;
            const float gi = ldg1(st), gf = ldg1(st + 256), gg = ldg1(st + 512), go = ldg1(st + 768), cc = ldg1(st + 1024);
            const float cprev = u > 0 ? ldg1(st - LSTM_STATE + 1024) : (p.c0 ? ldg1(p.c0 + (size_t)b * LSTM_HID + j) : 0.f);
            const float dh = ldg1(p.dout + row * LSTM_HID + j) + dh_rec;
            const float tc = tanhf(cc);
            const float dct = dc + dh * go * (1.f - tc * tc);
            d_o = dh * tc * (go * (1.f - go));
            d_i = dct * gg * (gi * (1.f - gi));
            d_g = dct * gi * (1.f - gg * gg);
            d_f = dct * cprev * (gf * (1.f - gf));
            dc = dct * gf;
        }
        if (b < p.B) { stg1(dgr, d_i); stg1(dgr + 256, d_f); stg1(dgr + 512, d_g); stg1(dgr + 768, d_o); }
        ((float*)gs)[(0 * 256 + j) * 4 + r] = d_i;
        ((float*)gs)[(1 * 256 + j) * 4 + r] = d_f;
        ((float*)gs)[(2 * 256 + j) * 4 + r] = d_g;
        ((float*)gs)[(3 * 256 + j) * 4 + r] = d_o;
        __syncthreads();
        float acc[4][4];                                           // dh_rec[rr][4 j4 + cidx] over gate columns wq * 64 .. + 63
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int cidx = 0; cidx < 4; ++cidx) acc[rr][cidx] = 0.f;
#pragma unroll 4
        for (int nn = 0; nn < 64; ++nn) {
            const float4 w = ldg4(wn + (size_t)nn * LSTM_HID);
            const float4 gv = gs[wq * 64 + nn];
            const float gr[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                acc[rr][0] = fmaf(gr[rr], w.x, acc[rr][0]);
                acc[rr][1] = fmaf(gr[rr], w.y, acc[rr][1]);
                acc[rr][2] = fmaf(gr[rr], w.z, acc[rr][2]);
                acc[rr][3] = fmaf(gr[rr], w.w, acc[rr][3]);
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            *(float4*)(red + (wq * 4 + rr) * 256 + j4 * 4) = make_float4(acc[rr][0], acc[rr][1], acc[rr][2], acc[rr][3]);
        __syncthreads();
        float s = red[(0 * 4 + r) * 256 + j];
#pragma unroll
        for (int qq = 1; qq < 16; ++qq) s += red[(qq * 4 + r) * 256 + j];      // sixteenths in index order
        dh_rec = s;
    }
    if (len > 0) {
        if (p.dh0) stg1(p.dh0 + (size_t)b * LSTM_HID + j, dh_rec);
        if (p.dc0) stg1(p.dc0 + (size_t)b * LSTM_HID + j, dc);
    }
}

// ---- the contractions outside the recurrence: exact-f32 MFMA, 64 x 64 tiles of four waves (32 x 32 each), operands straight from L2 ----
struct LstmGemmP {
    const float *a, *b, *bias, *bias2, *h0;
    const int* lens;                                               // row (bb, u) of x / h_prev counts only for u < lens[bb]
    float* c;
    int M, N, K, U1, kslab;
};

// Per 16-k block a lane holds k = k0 + 4 (lane >> 4) + jj, jj = 0..3, of row / column lane & 15 of both operands: the same
// assignment on either side, so the sum is complete; only its order differs from plain k order.
template <int MODE>
__global__ __launch_bounds__(256) void lstm_gemm(LstmGemmP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int m0 = blockIdx.y * 64 + (wave >> 1) * 32, n0 = blockIdx.x * 64 + (wave & 1) * 32;
    const int kbeg = (MODE >= 2) ? blockIdx.z * p.kslab : 0, kend = (MODE >= 2) ? min(p.K, kbeg + p.kslab) : p.K;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4 acc[2][2];
#pragma unroll
    for (int fi = 0; fi < 2; ++fi)
#pragma unroll
        for (int fj = 0; fj < 2; ++fj) acc[fi][fj] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        const int kb = k0 + 4 * l4;
        float a[2][4], bv[2][4];
        if (MODE >= 2) {                                           // per-k facts of the four rows kb .. kb + 3 of dG / x / h_prev
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int k = kb + jj;
                const bool in = k < kend;
                const int bb = in ? k / p.U1 : 0, u = in ? k - bb * p.U1 : 0;
                const bool live = in && u < ldgi(p.lens + bb);
#pragma unroll
                for (int fi = 0; fi < 2; ++fi) a[fi][jj] = in ? ldg1(p.a + (size_t)k * LSTM_GATES + m0 + 16 * fi + l15) : 0.f;
#pragma unroll
                for (int fj = 0; fj < 2; ++fj) {
                    const int n = n0 + 16 * fj + l15;
                    float v = 0.f;
                    if (MODE == 2) { if (live) v = ldg1(p.b + (size_t)k * LSTM_HID + n); }
                    else if (live) v = u > 0 ? ldg1(p.b + (size_t)(k - 1) * LSTM_HID + n) : (p.h0 ? ldg1(p.h0 + (size_t)bb * LSTM_HID + n) : 0.f);
                    bv[fj][jj] = v;
                }
            }
        } else {
#pragma unroll
            for (int fi = 0; fi < 2; ++fi) {
                const int m = m0 + 16 * fi + l15;
                bool in = m < p.M;
                if (MODE == 0 && in) { const int bb = m / p.U1; in = m - bb * p.U1 < ldgi(p.lens + bb); }
                const float4 v = in ? ldg4(p.a + (size_t)m * p.K + kb) : make_float4(0.f, 0.f, 0.f, 0.f);
                a[fi][0] = v.x; a[fi][1] = v.y; a[fi][2] = v.z; a[fi][3] = v.w;
            }
#pragma unroll
            for (int fj = 0; fj < 2; ++fj) {
                const int n = n0 + 16 * fj + l15;
                if (MODE == 0) {                                   // B(k, n) = W_ih[n][k]
                    const float4 v = ldg4(p.b + (size_t)n * LSTM_HID + kb);
                    bv[fj][0] = v.x; bv[fj][1] = v.y; bv[fj][2] = v.z; bv[fj][3] = v.w;
                } else {                                           // B(k, n) = W_ih[k][n]
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) bv[fj][jj] = ldg1(p.b + (size_t)(kb + jj) * LSTM_HID + n);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int fi = 0; fi < 2; ++fi)
#pragma unroll
                for (int fj = 0; fj < 2; ++fj) acc[fi][fj] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[fi][jj], bv[fj][jj], acc[fi][fj], 0, 0, 0);
    }
    float* c = p.c + (MODE >= 2 ? (size_t)blockIdx.z * p.M * p.N : 0);
#pragma unroll
    for (int fi = 0; fi < 2; ++fi)
#pragma unroll
        for (int fj = 0; fj < 2; ++fj) {
            const int n = n0 + 16 * fj + l15;
            const float add = MODE == 0 ? ldg1(p.bias + n) + ldg1(p.bias2 + n) : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + 16 * fi + 4 * l4 + e;
                if (m < p.M) stg1(c + (size_t)m * p.N + n, acc[fi][fj][e] + add);
            }
        }
}

// db slab s = the sum of dG rows s * LSTM_KSLAB .. in row order, one thread per gate column
__global__ void lstm_db_part(const float* __restrict__ dg, int rows, float* __restrict__ part) {
    const int n = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * LSTM_KSLAB, r1 = min(rows, r0 + LSTM_KSLAB);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += ldg1(dg + (size_t)r * LSTM_GATES + n);
    stg1(part + (size_t)blockIdx.y * LSTM_GATES + n, s);
}

// out[i] = part[0][i] + part[1][i] + ... in slab order (n4 float4 per slab)
__global__ void lstm_slab_reduce(const float* __restrict__ part, int ns, long long n4, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 s = ldg4(part + i * 4);
    for (int k = 1; k < ns; ++k) {
        const float4 t = ldg4(part + ((long long)k * n4 + i) * 4);
        s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    stg4(out + i * 4, s);
}
