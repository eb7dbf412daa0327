// The joint's backward: gradients of the lattice  logits[b,t,u,:] = tanh(e[b,t,:] + p[b,u,:]) W^T + bias  (model/component/joint.py:48-69)
// for a given g = d loss / d logits [B, T, U1, V] float32, without any tensor of M x 256 or M x V elements (M = B T U1 cells, u fastest):
//     h = tanh(e + p)     dh = g W     dz = dh (1 - h^2)     d_e[b,t,:] = sum_u dz     d_p[b,u,:] = sum_t dz     dW = g^T h     db = sum_m g
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
// Arithmetic.  Both contractions run on v_mfma_f32_16x16x32_bf16 with BOTH operands carried as two bf16 planes and three products
// (hi hi + hi lo + lo hi, split8_16 / mfma16_: the forward's bf16x3 parity mode).  bf16 and not f16 planes: g carries the 1 / B of a
// mean reduction and the occupancies of the lattice, so its small entries lie below f16's range, and bf16 keeps float32's exponent.
// h is recomputed from e and p by the forward's own jr_tanh_pre on the forward's own argument (JR_PRESCALE e + JR_PRESCALE p, each
// product rounded), so 1 - h^2 = fma(-h, h, 1) belongs to the h the lattice was formed from and is exactly 0 once h saturates.
//
// Determinism.  No atomics, no dynamic queue: every workgroup's share is a function of its index, sums that cross workgroups go
// through partial slabs in the caller's workspace, and joint_grad_reduce adds the slabs in index order.
//
//   joint_grad_pack_wt   W [V][256] -> the A operand stream of dh: [k-step s][hidden tile t][plane][lane] x 8 bf16, lane (i, q) holding
//                        W[32 s + 8 q + 0..7][16 t + i] (rows >= V zero): one 32-KiB stage per k-step of 32 vocabulary entries.
//   joint_grad_dz        workgroup (b, u-block of 16, chunk of TC frames), wave w takes frame 4 it + w of the chunk.  The MFMA runs with
//                        the hidden dimension on its M side (A = a W^T fragment from LDS) and 16 cells -- 16 consecutive u of ONE frame
//                        -- on its N side (B = 8 consecutive floats of a g row, straight from global memory): in the C layout a lane
//                        owns one cell and four consecutive hidden entries per tile, so e, p load as float4, d_p accumulates in the
//                        lane's own registers over the chunk's frames, and d_e is a sum over the 16 lanes of a row (four butterfly
//                        steps).  W^T stages go global -> registers -> LDS, double buffered, one barrier per k-step, shared by the
//                        four waves.  Writes de_part[u-block][b t][256] and dp_part[chunk][b][u][256].
//   joint_grad_dw        workgroup (64 vocabulary columns, slice of the cells), wave w owns 16 columns x all 256 hidden entries (64
//                        accumulator registers).  K = cells, 32 per step: the workgroup forms tanh(e + p) of the step's 32 cells once,
//                        as bf16 planes in B-fragment order in LDS (double buffered, one barrier per step); each wave loads its
//                        g[32 cells][16 columns] as the A operand and sums db on the way.  Writes dw_part[slice][V][256], db_part[slice][V].
//   joint_grad_reduce    out[i] = sum_j part[j][i], j ascending, float4 per thread.
//   joint_prescale       JR_PRESCALE x, the forward's argument (context-free forward entry).
// Cells with t >= T_b or u > U_b are never read (g, and h is taken as 0): they contribute exact zeros.
#pragma once

#define JG_STAGE 32768                                       // one k-step of the W^T stream: 16 tiles x (hi, lo) x 1 KiB
#define JG_LDS (2 * JG_STAGE)                                // both kernels: two stages
#define JG_TARGET_WGS 512                                    // workgroups a launch aims at (two per CU of a 256-CU part); fixed, so slab sizes do not depend on the device

struct JointGradP {
    const float* e;              // [B*T][256]
    const float* p;              // [B*U][256]
    const float* g;              // [M][V]
    const unsigned char* wt;     // joint_grad_pack_wt stream
    const int* lens;             // [2][B]: T_b, U_b
    float* de_part;              // [NUB][B*T][256]
    float* dp_part;              // [NC][B*U][256]
    float* dw_part;              // [NS][V][256]
    float* db_part;              // [NS][V]
    long long M;
    int B, T, U, V;
    int KS;                      // k-steps of dh: ceil(V / 32)
    int NUB, NC, TC;             // u-blocks of 16, frame chunks, frames per chunk (a multiple of 4)
    int NVS;                     // vocabulary slabs of 64
    long long CS;                // cells per slice of dw (a multiple of 32)
};

__global__ void joint_prescale(const float* __restrict__ x, float* __restrict__ y, long long n4) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    const float4 v = ldg4(x + 4 * idx);
    stg4(y + 4 * idx, make_float4(__fmul_rn(JR_PRESCALE, v.x), __fmul_rn(JR_PRESCALE, v.y), __fmul_rn(JR_PRESCALE, v.z), __fmul_rn(JR_PRESCALE, v.w)));
}

// the forward's h from raw e and p: the same two rounded products and the same sum as joint_prescale + joint_lattice_rows form
__device__ __forceinline__ float jg_h(float e, float p) { return jr_tanh_pre(__fadd_rn(__fmul_rn(JR_PRESCALE, e), __fmul_rn(JR_PRESCALE, p))); }

__global__ void joint_grad_pack_wt(const float* __restrict__ w, int V, int KS, unsigned char* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;     // (s, t, plane, lane)
    if (idx >= KS * 16 * 2 * 64) return;
    const int lane = idx & 63, pl = (idx >> 6) & 1, t = (idx >> 7) & 15, s = idx >> 11;
    const int col = 16 * t + (lane & 15), v0 = 32 * s + 8 * (lane >> 4);
    auto ld = [&](int j) { return v0 + j < V ? ldg1(w + (long long)(v0 + j) * RNNT_D + col) : 0.f; };
    const float4 a = make_float4(ld(0), ld(1), ld(2), ld(3)), b = make_float4(ld(4), ld(5), ld(6), ld(7));
    uint4 h, l;
    split8_16<false, true>(a, b, h, l);
    *reinterpret_cast<uint4*>(dst + (long long)idx * 16) = make_uint4(pl ? l.x : h.x, pl ? l.y : h.y, pl ? l.z : h.z, pl ? l.w : h.w);   // (a select of whole uint4s goes through scratch)
}

__global__ __launch_bounds__(256, 2) void joint_grad_dz(JointGradP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int c = blockIdx.x % P.NC, ub = (blockIdx.x / P.NC) % P.NUB, b = blockIdx.x / (P.NC * P.NUB);
    const int Tb = ldgi(P.lens + b), Ub = ldgi(P.lens + P.B + b);
    const int u = 16 * ub + i, uc = min(u, P.U - 1);
    const bool ulive = u < P.U && u <= Ub;
    const float* prow = P.p + ((long long)b * P.U + uc) * RNNT_D + 4 * q;
    f32x4_ dpacc[16];
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) dpacc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
    // stage 0 of the W^T stream
    uint4 wreg[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) wreg[n] = *reinterpret_cast<const uint4*>(P.wt + (tid + 256 * n) * 16);
#pragma unroll
    for (int n = 0; n < 8; ++n) *reinterpret_cast<uint4*>(jg_smem + (tid + 256 * n) * 16) = wreg[n];
    __syncthreads();
    int par = 0;
    const int nit = P.TC / 4;
    for (int it = 0; it < nit; ++it) {
        const int t = c * P.TC + 4 * it + wave, tc = min(t, P.T - 1);
        const bool tin = t < P.T, live = tin && t < Tb && ulive;
        const float* grow = P.g + (((long long)b * P.T + tc) * P.U + uc) * P.V + 8 * q;
        f32x4_ acc[16];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) acc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 ga = live && 8 * q < P.V ? ldg4(grow) : z4, gb = live && 8 * q + 4 < P.V ? ldg4(grow + 4) : z4;
        for (int s = 0; s < P.KS; ++s) {
            const int ns = s + 1 == P.KS ? 0 : s + 1;            // (behind the very last k-step: stage 0 once more, unused)
#pragma unroll
            for (int n = 0; n < 8; ++n) wreg[n] = *reinterpret_cast<const uint4*>(P.wt + (long long)ns * JG_STAGE + (tid + 256 * n) * 16);
            uint4 gh, gl;
            split8_16<false, true>(ga, gb, gh, gl);
            if (s + 1 < P.KS) {                                  // the next k-step's 8 floats of the g row
                const int v0 = 32 * (s + 1) + 8 * q;
                ga = live && v0 < P.V ? ldg4(grow + 32 * (s + 1)) : z4;
                gb = live && v0 + 4 < P.V ? ldg4(grow + 32 * (s + 1) + 4) : z4;
            }
            const unsigned char* buf = jg_smem + par * JG_STAGE + lane * 16;
#pragma unroll
            for (int t16 = 0; t16 < 16; ++t16) {
                const uint4 wh = *reinterpret_cast<const uint4*>(buf + (2 * t16) * 1024), wl = *reinterpret_cast<const uint4*>(buf + (2 * t16 + 1) * 1024);
                acc[t16] = mfma16_<false>(wl, gh, acc[t16]);
                acc[t16] = mfma16_<false>(wh, gl, acc[t16]);
                acc[t16] = mfma16_<false>(wh, gh, acc[t16]);
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) *reinterpret_cast<uint4*>(jg_smem + (par ^ 1) * JG_STAGE + (tid + 256 * n) * 16) = wreg[n];
            __syncthreads();                                     // the next stage is in LDS, everyone is done reading this one
            par ^= 1;
        }
        // dz on the accumulators: lane = cell (frame t, u), hidden 16 t16 + 4 q + 0..3
        const float* erow = P.e + ((long long)b * P.T + tc) * RNNT_D + 4 * q;
        float* derow = P.de_part + (((long long)ub * P.B + b) * P.T + tc) * RNNT_D + 4 * q;
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) {
            const float4 e4 = ldg4(erow + 16 * t16), p4 = ldg4(prow + 16 * t16);
            const float h0 = jg_h(e4.x, p4.x), h1 = jg_h(e4.y, p4.y), h2 = jg_h(e4.z, p4.z), h3 = jg_h(e4.w, p4.w);
            f32x4_ dz;
            dz[0] = live ? acc[t16][0] * fmaf(-h0, h0, 1.0f) : 0.f;
            dz[1] = live ? acc[t16][1] * fmaf(-h1, h1, 1.0f) : 0.f;
            dz[2] = live ? acc[t16][2] * fmaf(-h2, h2, 1.0f) : 0.f;
            dz[3] = live ? acc[t16][3] * fmaf(-h3, h3, 1.0f) : 0.f;
            dpacc[t16] += dz;
            auto rowsum = [](float v) {                          // sum over the 16 cells of the row: a fixed butterfly
                v += __shfl_xor(v, 1, 64);
                v += __shfl_xor(v, 2, 64);
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 8, 64);
                return v;
            };
            const float4 de4 = make_float4(rowsum(dz[0]), rowsum(dz[1]), rowsum(dz[2]), rowsum(dz[3]));
            if (i == 0 && tin) stg4(derow + 16 * t16, de4);
        }
    }
    // d_p of the chunk: the four waves' sums (frames 4 it + w) added in wave order through LDS (free behind the last barrier)
    float* red = reinterpret_cast<float*>(jg_smem);
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) *reinterpret_cast<f32x4_*>(red + (wave * 16 + i) * RNNT_D + 16 * t16 + 4 * q) = dpacc[t16];
    __syncthreads();
    for (int r = 0; r < 16; ++r) {
        if (16 * ub + r >= P.U) break;                           // uniform
        const float v = ((red[r * RNNT_D + tid] + red[(16 + r) * RNNT_D + tid]) + red[(32 + r) * RNNT_D + tid]) + red[(48 + r) * RNNT_D + tid];
        stg1(P.dp_part + (((long long)c * P.B + b) * P.U + 16 * ub + r) * RNNT_D + tid, v);
    }
}

__global__ __launch_bounds__(256, 2) void joint_grad_dw(JointGradP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int vs = blockIdx.x % P.NVS, sl = blockIdx.x / P.NVS;
    const int tv = 4 * vs + wave, v = 16 * tv + i;
    const bool vlive = v < P.V;
    const long long m0 = (long long)sl * P.CS, m1 = min(P.M, m0 + P.CS);
    f32x4_ acc[16];
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) acc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
    int par = 0;
    for (long long c0 = m0; c0 < m1; c0 += 32) {
        float gj[8], hv[4][8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                            // cells c0 + 8 q + j: this lane's K entries in both operands
            const long long m = c0 + 8 * q + j;
            const int mc = (int)min(m, P.M - 1);
            const int bt = mc / P.U, uu = mc - bt * P.U, bb = bt / P.T, tt = bt - bb * P.T;
            const bool live = m < m1 && tt < ldgi(P.lens + bb) && uu <= ldgi(P.lens + P.B + bb);
            gj[j] = live && vlive ? ldg1(P.g + (long long)mc * P.V + v) : 0.f;
            const float* er = P.e + (long long)bt * RNNT_D + i;
            const float* pr = P.p + ((long long)bb * P.U + uu) * RNNT_D + i;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = 16 * (wave + 4 * n);
                hv[n][j] = live ? jg_h(ldg1(er + col), ldg1(pr + col)) : 0.f;
            }
        }
        unsigned char* buf = jg_smem + par * JG_STAGE + lane * 16;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            uint4 hh, hl;
            split8_16<false, true>(make_float4(hv[n][0], hv[n][1], hv[n][2], hv[n][3]), make_float4(hv[n][4], hv[n][5], hv[n][6], hv[n][7]), hh, hl);
            *reinterpret_cast<uint4*>(buf + (2 * (wave + 4 * n)) * 1024) = hh;
            *reinterpret_cast<uint4*>(buf + (2 * (wave + 4 * n) + 1) * 1024) = hl;
        }
        uint4 ah, al;
        split8_16<false, true>(make_float4(gj[0], gj[1], gj[2], gj[3]), make_float4(gj[4], gj[5], gj[6], gj[7]), ah, al);
        dbacc += ((gj[0] + gj[1]) + (gj[2] + gj[3])) + ((gj[4] + gj[5]) + (gj[6] + gj[7]));
        __syncthreads();                                         // the step's h planes are in LDS (the other buffer is free: its readers passed this barrier)
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) {
            const uint4 bh = *reinterpret_cast<const uint4*>(buf + (2 * t16) * 1024), bl = *reinterpret_cast<const uint4*>(buf + (2 * t16 + 1) * 1024);
            acc[t16] = mfma16_<false>(al, bh, acc[t16]);
            acc[t16] = mfma16_<false>(ah, bl, acc[t16]);
            acc[t16] = mfma16_<false>(ah, bh, acc[t16]);
        }
        par ^= 1;
    }
    // C layout: rows 16 tv + 4 q + r (vocabulary), column 16 t16 + i (hidden)
    float* slab = P.dw_part + (long long)sl * P.V * RNNT_D;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int vv = 16 * tv + 4 * q + r;
        if (vv < P.V) {
#pragma unroll
            for (int t16 = 0; t16 < 16; ++t16) stg1(slab + (long long)vv * RNNT_D + 16 * t16 + i, acc[t16][r]);
        }
    }
    dbacc += __shfl_xor(dbacc, 16, 64);
    dbacc += __shfl_xor(dbacc, 32, 64);
    if (q == 0 && vlive) stg1(P.db_part + (long long)sl * P.V + v, dbacc);
}

// out[i] = part[0][i] + part[1][i] + ... in that order; n4 float4s per part, parts `stride4` float4s apart
__global__ void joint_grad_reduce(const float* __restrict__ part, int nparts, long long stride4, long long n4, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n4) return;
    float4 a = ldg4(part + 4 * idx);
    for (int j = 1; j < nparts; ++j) {
        const float4 v = ldg4(part + 4 * ((long long)j * stride4 + idx));
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    stg4(out + 4 * idx, a);
}
