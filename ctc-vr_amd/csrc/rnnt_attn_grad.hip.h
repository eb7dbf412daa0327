// The attention core of an encoder layer with its backward, flash-style (rnnt_rel_attention_forward / _backward, api_attn.hip.inc):
//   s[b,h,i,j] = ((q_i + u_h) . k_j + (q_i + vb_h) . p_j) / 8 over the visible keys, a = softmax(s), out_i = sum_j a_ij v_j
// H = 4 heads of 64; q, k, v, out and their gradients [B, T, 256] (head h at columns 64 h ..), p [T, 256], u, vb [4, 64].  visible
// (attn_hi, attn_lo below) is the reference's subsequent_chunk_mask & ~make_pad_mask as three integers and a length; no [T, T] value ever
// reaches memory, and keys and values at j >= len_b are never read.
//
//   attn_fwd      one WAVE per (row b, head h, tile of 16 queries); the four heads of a tile are one workgroup.  It walks the 16-key
//                 tiles between the tile's window bounds and len_b, online softmax in float32, writes out and one log-sum-exp per row
//   attn_delta    delta[b,h,i] = dout_i . out_i
//   attn_bwd_k    key-owned: one wave per (b, h, tile of 16 keys) loops over the query tiles that see it, recomputes a = exp(s - lse),
//                 ds = a (dout . v - delta) / 8, and forms dv = a^T dout, dk = ds^T (q + u), the row's dp partial ds^T (q + vb)
//   attn_bwd_q    query-owned: recomputes again, A = ds k, Bm = ds p; dq = A + Bm, column sums of A and Bm -> du / dvb partials
//   attn_bias_reduce, lstm_slab_reduce   du / dvb over (row, query tile) and dp over rows, added in index order
//
// Every contraction is v_mfma_f32_16x16x4_f32 (exact float32 products, float32 accumulation), and no wave shares anything with
// another: no LDS, no barrier, no atomics.  What makes that possible is computing the score tile TRANSPOSED relative to the output
// that consumes it.  An accumulator lane holds C[4 (lane >> 4) + e][lane & 15], e = 0..3, and an operand lane holds k-index lane >> 4
// of row / column lane & 15.  Per 16-wide block of the contracted index, step e pairs k-index 4 (lane >> 4) + e on BOTH operands
// (lstm_gemm's assignment: the sum is complete, only its order differs), so accumulator element e of one product is, as it lies,
// the B operand of step e of the next:
//   attn_fwd / attn_bwd_q   S^T[j][i] = [k ; p]_j . [q + u | q + vb]_i  -> lane holds query i = lane & 15, keys 4 (lane >> 4) + e;
//                           out^T[d][i] += v[j][d] a^T[j][i] and dq^T likewise contract over j with a^T / ds^T straight from registers
//   attn_bwd_k              S[i][j] -> lane holds key j = lane & 15, queries 4 (lane >> 4) + e; dv^T[d][j] += dout[i][d] a[i][j] etc.
// Row statistics (max, sum, lse, delta) then belong to lane & 15 and need two xor-shuffles (16, 32), not a 16-lane tree.
#pragma once

#define ATTN_TILE 16
#define ATTN_TMAX 4096                                             // cap on T (include/rnnt_hip.h states it)
#define ATTN_RED_GROUPS 16                                         // attn_bias_reduce: partial rows are dealt to 16 groups of 64 columns

typedef float attn_f4 __attribute__((ext_vector_type(4)));

struct AttnGradP {
    const float *q, *k, *v, *p, *u, *vb, *dout, *lse_in, *delta_in;
    const int* lens;                                               // [B] valid keys per row (device)
    float *out, *lse, *dq, *dk, *dv, *dp_part, *du_part, *dvb_part;
    int B, T, nt, chunk, left;                                     // nt = ceil(T / 16)
};

// the window of query i: keys lo <= j < hi (before the length cuts it); chunk <= 0: everything
__device__ __forceinline__ int attn_hi(int i, int T, int chunk) { return chunk > 0 ? min(T, (i / chunk + 1) * chunk) : T; }
__device__ __forceinline__ int attn_lo(int i, int chunk, int left) {
    if (chunk <= 0 || left < 0) return 0;
    const int n = i / chunk;
    return n > left ? (n - left) * chunk : 0;
}

#define ATTN_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// [q + u | q + vb] of query row i (zeros' worth of q beyond T) as 16 + 16 operand values: d = 16 blk + 4 (lane >> 4) + jj
__device__ __forceinline__ void attn_load_quv(const AttnGradP& p, int b, int i, int h, int l4, float* qu, float* qv) {
    const float* qrow = p.q + ((size_t)b * p.T + i) * RNNT_D + h * RNNT_DK + 4 * l4;
    const float *ur = p.u + h * RNNT_DK + 4 * l4, *vr = p.vb + h * RNNT_DK + 4 * l4;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const float4 qq = i < p.T ? ldg4(qrow + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 uu = ldg4(ur + 16 * blk), vv = ldg4(vr + 16 * blk);
        qu[4 * blk + 0] = qq.x + uu.x; qu[4 * blk + 1] = qq.y + uu.y; qu[4 * blk + 2] = qq.z + uu.z; qu[4 * blk + 3] = qq.w + uu.w;
        qv[4 * blk + 0] = qq.x + vv.x; qv[4 * blk + 1] = qq.y + vv.y; qv[4 * blk + 2] = qq.z + vv.z; qv[4 * blk + 3] = qq.w + vv.w;
    }
}

// 16 operand values of one head's row (row pointer already at the head's column 4 (lane >> 4)); dead: zeros, nothing is read
__device__ __forceinline__ void attn_load_row(const float* row, bool live, float* r) {
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const float4 t = live ? ldg4(row + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
        r[4 * blk + 0] = t.x; r[4 * blk + 1] = t.y; r[4 * blk + 2] = t.z; r[4 * blk + 3] = t.w;
    }
}

// S^T tile of keys j0 .. j0 + 15 against the wave's 16 queries: element e is s[i = lane & 15][j = j0 + 4 (lane >> 4) + e] * 8
__device__ __forceinline__ attn_f4 attn_scores_t(const AttnGradP& p, int b, int h, int j0, int len, int l15, int l4, const float* qu, const float* qv) {
    const int ja = j0 + l15;
    const bool live = ja < len;
    const float* krow = p.k + ((size_t)b * p.T + ja) * RNNT_D + h * RNNT_DK + 4 * l4;
    const float* prow = p.p + (size_t)ja * RNNT_D + h * RNNT_DK + 4 * l4;
    attn_f4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const float4 kk = live ? ldg4(krow + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 pp = live ? ldg4(prow + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
        s = ATTN_MFMA(kk.x, qu[4 * blk + 0], s); s = ATTN_MFMA(kk.y, qu[4 * blk + 1], s);
        s = ATTN_MFMA(kk.z, qu[4 * blk + 2], s); s = ATTN_MFMA(kk.w, qu[4 * blk + 3], s);
        s = ATTN_MFMA(pp.x, qv[4 * blk + 0], s); s = ATTN_MFMA(pp.y, qv[4 * blk + 1], s);
        s = ATTN_MFMA(pp.z, qv[4 * blk + 2], s); s = ATTN_MFMA(pp.w, qv[4 * blk + 3], s);
    }
    return s;
}

// the key tiles a query tile i0 .. walks: [jbeg rounded down to a tile, jend)
__device__ __forceinline__ void attn_key_range(const AttnGradP& p, int i0, int len, int& jbeg, int& jend) {
    jbeg = attn_lo(i0, p.chunk, p.left) / ATTN_TILE * ATTN_TILE;
    jend = min(attn_hi(min(i0 + ATTN_TILE - 1, p.T - 1), p.T, p.chunk), len);
}

__global__ __launch_bounds__(256) void attn_fwd(AttnGradP p) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int b = blockIdx.x / p.nt, i0 = (blockIdx.x - b * p.nt) * ATTN_TILE, i = i0 + l15;
    const int len = ldgi(p.lens + b);
    const bool iv = i < p.T;
    const int hi_i = attn_hi(min(i, p.T - 1), p.T, p.chunk), lo_i = attn_lo(min(i, p.T - 1), p.chunk, p.left);
    float qu[16], qv[16];
    attn_load_quv(p, b, i, h, l4, qu, qv);
    attn_f4 o[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) o[f] = (attn_f4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    int jbeg, jend;
    attn_key_range(p, i0, len, jbeg, jend);
    for (int j0 = jbeg; j0 < jend; j0 += ATTN_TILE) {
        const attn_f4 s = attn_scores_t(p, b, h, j0, len, l15, l4, qu, qv);
        bool vis[4];
        float sc[4], mt = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + 4 * l4 + e;
            vis[e] = iv && j < len && j < hi_i && j >= lo_i;
            sc[e] = s[e] * 0.125f;
            if (vis[e]) mt = fmaxf(mt, sc[e]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float mn = fmaxf(m, mt);
        const float alpha = m == -INFINITY ? 1.f : expf(m - mn);   // nothing summed yet: l and o are zeros, any finite factor does
        float pe[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) pe[e] = vis[e] ? expf(sc[e] - mn) : 0.f;      // a select: a hidden key never meets exp
        l = l * alpha + (((pe[0] + pe[1]) + pe[2]) + pe[3]);
#pragma unroll
        for (int f = 0; f < 4; ++f) o[f] *= alpha;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + 4 * l4 + e;
            const float* vrow = p.v + ((size_t)b * p.T + j) * RNNT_D + h * RNNT_DK + l15;
#pragma unroll
            for (int f = 0; f < 4; ++f) o[f] = ATTN_MFMA(j < len ? ldg1(vrow + 16 * f) : 0.f, pe[e], o[f]);
        }
        m = mn;
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (!iv) return;
    const bool dead = m == -INFINITY;                              // no visible key: out = 0, and the mark tells the backward
    float* orow = p.out + ((size_t)b * p.T + i) * RNNT_D + h * RNNT_DK + 4 * l4;
#pragma unroll
    for (int f = 0; f < 4; ++f)
        stg4(orow + 16 * f, dead ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(o[f][0] / l, o[f][1] / l, o[f][2] / l, o[f][3] / l));
    if (p.lse && l4 == 0) stg1(p.lse + ((size_t)b * RNNT_H + h) * p.T + i, dead ? INFINITY : m + logf(l));
}

// delta[b][h][i] = dout[b,i,h,:] . out[b,i,h,:]: 16 lanes per (b, i, h), four columns each, then an xor tree
__global__ __launch_bounds__(256) void attn_delta(const float* __restrict__ out, const float* __restrict__ dout, long long rows, int T, float* __restrict__ delta) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, r = idx >> 4;
    const int part = (int)(idx & 15);
    float s = 0.f;
    if (r < rows) {
        const float4 a = ldg4(out + r * RNNT_DK + part * 4), g = ldg4(dout + r * RNNT_DK + part * 4);
        s = ((a.x * g.x + a.y * g.y) + a.z * g.z) + a.w * g.w;
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    if (r < rows && part == 0) {
        const long long bt = r >> 2, b = bt / T;
        stg1(delta + ((size_t)b * RNNT_H + (size_t)(r & 3)) * T + (size_t)(bt - b * T), s);
    }
}

__global__ __launch_bounds__(256) void attn_bwd_q(AttnGradP p) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int b = blockIdx.x / p.nt, qt = blockIdx.x - b * p.nt, i0 = qt * ATTN_TILE, i = i0 + l15;
    const int len = ldgi(p.lens + b);
    const bool iv = i < p.T;
    const int hi_i = attn_hi(min(i, p.T - 1), p.T, p.chunk), lo_i = attn_lo(min(i, p.T - 1), p.chunk, p.left);
    float qu[16], qv[16], dor[16];
    attn_load_quv(p, b, i, h, l4, qu, qv);
    attn_load_row(p.dout + ((size_t)b * p.T + i) * RNNT_D + h * RNNT_DK + 4 * l4, iv, dor);
    const size_t srow = ((size_t)b * RNNT_H + h) * p.T + i;
    const float lse = iv ? ldg1(p.lse_in + srow) : 0.f, delta = iv ? ldg1(p.delta_in + srow) : 0.f;
    attn_f4 ak[4], ap[4];                                          // A^T = (ds k)^T and Bm^T = (ds p)^T: [d = 16 f + 4 l4 + e][i = l15]
#pragma unroll
    for (int f = 0; f < 4; ++f) ak[f] = ap[f] = (attn_f4){0.f, 0.f, 0.f, 0.f};
    int jbeg, jend;
    attn_key_range(p, i0, len, jbeg, jend);
    for (int j0 = jbeg; j0 < jend; j0 += ATTN_TILE) {
        const attn_f4 s = attn_scores_t(p, b, h, j0, len, l15, l4, qu, qv);
        attn_f4 dpt = {0.f, 0.f, 0.f, 0.f};                        // (dout v^T)^T[j][i]
        {
            float vr[16];
            attn_load_row(p.v + ((size_t)b * p.T + j0 + l15) * RNNT_D + h * RNNT_DK + 4 * l4, j0 + l15 < len, vr);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) dpt = ATTN_MFMA(vr[kk], dor[kk], dpt);
        }
        float ds[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + 4 * l4 + e;
            const bool vis = iv && j < len && j < hi_i && j >= lo_i;
            const float a = vis ? expf(s[e] * 0.125f - lse) : 0.f;
            ds[e] = a * (dpt[e] - delta) * 0.125f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + 4 * l4 + e;
            const bool live = j < len;
            const float* krow = p.k + ((size_t)b * p.T + j) * RNNT_D + h * RNNT_DK + l15;
            const float* prow = p.p + (size_t)j * RNNT_D + h * RNNT_DK + l15;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                ak[f] = ATTN_MFMA(live ? ldg1(krow + 16 * f) : 0.f, ds[e], ak[f]);
                ap[f] = ATTN_MFMA(live ? ldg1(prow + 16 * f) : 0.f, ds[e], ap[f]);
            }
        }
    }
    if (iv) {
        float* drow = p.dq + ((size_t)b * p.T + i) * RNNT_D + h * RNNT_DK + 4 * l4;
#pragma unroll
        for (int f = 0; f < 4; ++f) stg4(drow + 16 * f, make_float4(ak[f][0] + ap[f][0], ak[f][1] + ap[f][1], ak[f][2] + ap[f][2], ak[f][3] + ap[f][3]));
    }
    // column sums over the tile's 16 queries (rows beyond T and dead rows hold zeros): the tile's share of du and dvb
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = ak[f][e], c = ap[f][e];
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) { a += __shfl_xor(a, x); c += __shfl_xor(c, x); }
            ak[f][e] = a; ap[f][e] = c;
        }
    if (l15 == 0) {
        const size_t prow = (size_t)blockIdx.x * RNNT_D + h * RNNT_DK + 4 * l4;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            stg4(p.du_part + prow + 16 * f, make_float4(ak[f][0], ak[f][1], ak[f][2], ak[f][3]));
            stg4(p.dvb_part + prow + 16 * f, make_float4(ap[f][0], ap[f][1], ap[f][2], ap[f][3]));
        }
    }
}

__global__ __launch_bounds__(256) void attn_bwd_k(AttnGradP p) {
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int b = blockIdx.x / p.nt, j0 = (blockIdx.x - b * p.nt) * ATTN_TILE, j = j0 + l15;
    const int len = ldgi(p.lens + b), T = p.T;
    const bool jv = j < len;
    float kr[16], pr[16], vr[16];
    attn_load_row(p.k + ((size_t)b * T + j) * RNNT_D + h * RNNT_DK + 4 * l4, jv, kr);
    attn_load_row(p.p + (size_t)j * RNNT_D + h * RNNT_DK + 4 * l4, jv, pr);
    attn_load_row(p.v + ((size_t)b * T + j) * RNNT_D + h * RNNT_DK + 4 * l4, jv, vr);
    attn_f4 dk[4], dv[4], dp[4];                                   // transposed: [d = 16 f + 4 l4 + e][j = l15]
#pragma unroll
    for (int f = 0; f < 4; ++f) dk[f] = dv[f] = dp[f] = (attn_f4){0.f, 0.f, 0.f, 0.f};
    // the queries that see a key of this tile: from the first row of the first key's chunk to the last row of the window of the last live key
    int ibeg = 0, iend = j0 < len ? T : 0;
    if (p.chunk > 0 && j0 < len) {
        ibeg = j0 / p.chunk * p.chunk / ATTN_TILE * ATTN_TILE;
        if (p.left >= 0) iend = (int)min((long long)T, ((long long)(min(j0 + ATTN_TILE, len) - 1) / p.chunk + p.left + 1) * p.chunk);
    }
    const float *ur = p.u + h * RNNT_DK, *vbr = p.vb + h * RNNT_DK;
    for (int i0 = ibeg; i0 < iend; i0 += ATTN_TILE) {
        const int ia = i0 + l15;
        attn_f4 s = {0.f, 0.f, 0.f, 0.f}, dpv = {0.f, 0.f, 0.f, 0.f};             // s[i][j] * 8 and (dout v^T)[i][j], i = i0 + 4 l4 + e
        {
            const float* qrow = p.q + ((size_t)b * T + ia) * RNNT_D + h * RNNT_DK + 4 * l4;
            const float* drow = p.dout + ((size_t)b * T + ia) * RNNT_D + h * RNNT_DK + 4 * l4;
#pragma unroll
            for (int blk = 0; blk < 4; ++blk) {
                const float4 qq = ia < T ? ldg4(qrow + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 dd = ia < T ? ldg4(drow + 16 * blk) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 uu = ldg4(ur + 4 * l4 + 16 * blk), vv = ldg4(vbr + 4 * l4 + 16 * blk);
                s = ATTN_MFMA(qq.x + uu.x, kr[4 * blk + 0], s); s = ATTN_MFMA(qq.y + uu.y, kr[4 * blk + 1], s);
                s = ATTN_MFMA(qq.z + uu.z, kr[4 * blk + 2], s); s = ATTN_MFMA(qq.w + uu.w, kr[4 * blk + 3], s);
                s = ATTN_MFMA(qq.x + vv.x, pr[4 * blk + 0], s); s = ATTN_MFMA(qq.y + vv.y, pr[4 * blk + 1], s);
                s = ATTN_MFMA(qq.z + vv.z, pr[4 * blk + 2], s); s = ATTN_MFMA(qq.w + vv.w, pr[4 * blk + 3], s);
                dpv = ATTN_MFMA(dd.x, vr[4 * blk + 0], dpv); dpv = ATTN_MFMA(dd.y, vr[4 * blk + 1], dpv);
                dpv = ATTN_MFMA(dd.z, vr[4 * blk + 2], dpv); dpv = ATTN_MFMA(dd.w, vr[4 * blk + 3], dpv);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + 4 * l4 + e;
            const bool il = i < T;
            const int ic = min(i, T - 1);
            const bool vis = il && jv && j < attn_hi(ic, T, p.chunk) && j >= attn_lo(ic, p.chunk, p.left);
            const size_t srow = ((size_t)b * RNNT_H + h) * T + ic;
            const float lse = ldg1(p.lse_in + srow), delta = ldg1(p.delta_in + srow);
            const float a = vis ? expf(s[e] * 0.125f - lse) : 0.f;
            const float ds = a * (dpv[e] - delta) * 0.125f;
            const float* qrow = p.q + ((size_t)b * T + i) * RNNT_D + h * RNNT_DK + l15;
            const float* drow = p.dout + ((size_t)b * T + i) * RNNT_D + h * RNNT_DK + l15;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const float qq = il ? ldg1(qrow + 16 * f) : 0.f, dd = il ? ldg1(drow + 16 * f) : 0.f;
                dv[f] = ATTN_MFMA(dd, a, dv[f]);
                dk[f] = ATTN_MFMA(qq + ldg1(ur + l15 + 16 * f), ds, dk[f]);
                dp[f] = ATTN_MFMA(qq + ldg1(vbr + l15 + 16 * f), ds, dp[f]);
            }
        }
    }
    if (j < T) {
        const size_t o = ((size_t)b * T + j) * RNNT_D + h * RNNT_DK + 4 * l4;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            stg4(p.dk + o + 16 * f, make_float4(dk[f][0], dk[f][1], dk[f][2], dk[f][3]));
            stg4(p.dv + o + 16 * f, make_float4(dv[f][0], dv[f][1], dv[f][2], dv[f][3]));
            stg4(p.dp_part + o + 16 * f, make_float4(dp[f][0], dp[f][1], dp[f][2], dp[f][3]));
        }
    }
}

// du (blockIdx.x < 4) and dvb: out[c] = sum over the partial rows r of part[r][c].  Group g = threadIdx.x >> 6 adds rows g, g + 16, ..
// in that order; the 16 group sums meet in LDS and are added in group order.  The share of a thread depends on the shape alone.
__global__ __launch_bounds__(64 * ATTN_RED_GROUPS) void attn_bias_reduce(const float* __restrict__ du_part, const float* __restrict__ dvb_part, int rows,
                                                                          float* __restrict__ du, float* __restrict__ dvb) {
    __shared__ float red[ATTN_RED_GROUPS][64];
    const int g = threadIdx.x >> 6, c = (blockIdx.x & 3) * 64 + (threadIdx.x & 63);
    const float* part = blockIdx.x < 4 ? du_part : dvb_part;
    float s = 0.f;
#pragma unroll 8
    for (int r = g; r < rows; r += ATTN_RED_GROUPS) s += ldg1(part + (size_t)r * RNNT_D + c);
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0) {
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < ATTN_RED_GROUPS; ++k) t += red[k][threadIdx.x];
        stg1((blockIdx.x < 4 ? du : dvb) + c, t);
    }
}
