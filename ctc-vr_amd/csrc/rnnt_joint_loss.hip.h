// The fused transducer joint and loss: the backward of  nll_b = transducer loss of  logits[b,t,u,:] = tanh(e[b,t,:] + p[b,u,:]) W^T + bias
// without the lattice.  joint_grad_dz and joint_grad_dw (rnnt_joint_grad.hip.h) with the load of g = d loss / d logits replaced by its
// formation in registers: the tile's logits are recomputed by the forward's bf16x3 contraction, and
//     g_k = clamp(exp(z_k - lse) occ - [k = blank] tb - [k = y_{u+1}] tl) row_scale[b]        (loss_g<true>, rnnt_loss.hip.h)
// is a function of one logit and the four per-cell floats (lse, occ, tb, tl) that loss_coef left in `coef`.  Nothing of M x V or
// M x 256 elements is read or written.  Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
// Ownership, slabs and determinism are joint_grad_dz's and joint_grad_dw's: no atomics, no dynamic queue, partial slabs added by
// joint_grad_reduce in index order.  Cells with t >= T_b or u > U_b: g is 0 by a select, h is taken as 0, and neither e, p nor coef
// of such a cell is read.
//
//   joint_loss_pack_w   W [V][256] -> one 64-KiB stage per k-step s of 32 vocabulary entries, 64 pieces of 1 KiB (64 lanes x 8 bf16):
//                       pieces 0..31, the z half: piece ((tt 8 + ks) 2 + plane) is pack_joint_w's fragment of vocabulary tile 2 s + tt and
//                       hidden k-step ks: lane (i, q) holds W[32 s + 16 tt + i][32 ks + 8 q + 0..7];
//                       pieces 32..63, the dh half: piece 32 + 2 t + plane is joint_grad_pack_wt's fragment of hidden tile t under the K
//                       permutation of the z tile's C layout: slot j of lane (i, q) holds W[32 s + 16 (j / 4) + 4 q + j % 4][16 t + i].
//                       Rows >= V are zero.
//   joint_loss_dz       workgroup (b, u-block of 16, chunk of TC frames), wave w takes frame 4 it + w: joint_grad_dz's assignment.  Per
//                       frame the wave forms h of its 16 cells once as the forward's B operand (ah[8], al[8]: lane (i, q) holds
//                       h[cell i][32 ks + 8 q + 0..7]).  Per k-step: z = W h^T with the vocabulary on the M side (2 tiles x 8 hidden
//                       k-steps x 3 products); in that C layout lane (i, q) owns cell i and entries 16 tt + 4 q + 0..3, so after g is
//                       formed in place the eight registers ARE the B operand of dh = g W under the permutation above: no exchange.
//                       Stages go global -> registers -> LDS, double buffered (2 x 64 KiB: one workgroup per CU), one barrier per k-step.
//   joint_loss_dw       workgroup (64 vocabulary columns, slice of CS cells), wave w owns 16 columns x 256 hidden: joint_grad_dw's
//                       assignment.  The wave's 16 rows of W stay in registers as the B operand of z (lane (i, q): W[column i][32 ks +
//                       8 q + 0..7], two planes, 64 registers).  Per step of 32 cells the workgroup forms h once and stages it in both
//                       layouts: hidden along K (the A operand of z = h W^T, cells on the M side) and cells along K (the B operand of
//                       dW = g^T h) under the cell permutation of z's C layout -- slot j of lane group q is cell 16 (j / 4) + 4 q + j % 4
//                       -- so the lane's eight g are the A operand of dW directly, and db is summed from the same registers.
//                       2 x 32 KiB per step in one buffer, two barriers per step, TWO workgroups per CU: one forms h while the other
//                       runs its MFMAs (one workgroup per CU with a double buffer measured 4.17 ms at the joint shape).
#pragma once

#define JL_HALF 32768                                        // one half of a stage: 32 pieces of 1 KiB
#define JL_STAGE (2 * JL_HALF)                               // joint_loss_dz: z half | dh half of a k-step (two stages); joint_loss_dw: h along hidden | h along cells (one)
#define JL_BIAS 448                                          // floats of the bias table behind joint_loss_dz's stages (13 k-steps x 32, rounded up)
#define JL_DZ_LDS (2 * JL_STAGE + JL_BIAS * 4)
#define JL_DW_LDS JL_STAGE

struct JointLossP {
    const float* e;              // [B*T][256]
    const float* p;              // [B*U][256]
    const float* w;              // [V][256]
    const float* bias;           // [V]
    const unsigned char* wz;     // joint_loss_pack_w stream
    const float* coef;           // [M][4]: lse, occ, blank term, label term (loss_coef)
    const int* lens;             // [2][B]: T_b, U_b
    const int* targets;          // [B][ts]
    const float* row_scale;      // [B]: d loss / d nll_b
    float* de_part;              // [NUB][B*T][256]
    float* dp_part;              // [NC][B*U][256]
    float* dw_part;              // [NS][V][256]
    float* db_part;              // [NS][V]
    long long M;
    long long CS;                // cells per slice of dw (a multiple of 32)
    int B, T, U, V;
    int KS;                      // k-steps of the vocabulary: ceil(V / 32)
    int NUB, NC, TC;             // u-blocks of 16, frame chunks, frames per chunk (a multiple of 4)
    int NVS;                     // vocabulary slabs of 64
    int ts, blank;
    float clamp;
};

__global__ void joint_loss_pack_w(const float* __restrict__ w, int V, int KS, unsigned char* __restrict__ dst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;     // (s, piece, lane)
    if (idx >= KS * 64 * 64) return;
    const int lane = idx & 63, pc = (idx >> 6) & 63, s = idx >> 12, pl = pc & 1, i = lane & 15, q = lane >> 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (pc < 32) {
        const int tt = pc >> 4, ks = (pc >> 1) & 7, row = 32 * s + 16 * tt + i, k0 = 32 * ks + 8 * q;
        if (row < V) { a = ldg4(w + (long long)row * RNNT_D + k0); b = ldg4(w + (long long)row * RNNT_D + k0 + 4); }
    } else {
        const int col = 16 * ((pc - 32) >> 1) + i, v0 = 32 * s + 4 * q;
        auto ld = [&](int j) { const int v = v0 + 16 * (j >> 2) + (j & 3); return v < V ? ldg1(w + (long long)v * RNNT_D + col) : 0.f; };
        a = make_float4(ld(0), ld(1), ld(2), ld(3));
        b = make_float4(ld(4), ld(5), ld(6), ld(7));
    }
    uint4 h, l;
    split8_16<false, true>(a, b, h, l);
    *reinterpret_cast<uint4*>(dst + (long long)idx * 16) = make_uint4(pl ? l.x : h.x, pl ? l.y : h.y, pl ? l.z : h.z, pl ? l.w : h.w);   // (a select of whole uint4s goes through scratch)
}

// cell m -> its row's (b, t, u) and whether it lies inside the row's lengths; next() walks to cell m + 1 without dividing again
struct JointLossCell {
    long long m;
    int bt, b, t, u;
    bool live;
    __device__ __forceinline__ void look(long long m1, const JointLossP& P) {
        live = false;
        if (m < m1) live = t < ldgi(P.lens + b) && u <= ldgi(P.lens + P.B + b);      // m1 <= M: b < B wherever the lengths are read
    }
    __device__ __forceinline__ void at(long long m_, long long m1, const JointLossP& P) {
        m = m_;
        const int mc = (int)min(m, P.M - 1);
        bt = mc / P.U;
        u = mc - bt * P.U;
        b = bt / P.T;
        t = bt - b * P.T;
        look(m1, P);
    }
    __device__ __forceinline__ void next(long long m1, const JointLossP& P) {
        ++m;
        if (++u == P.U) {
            u = 0;
            ++bt;
            if (++t == P.T) { t = 0; ++b; }
        }
        look(m1, P);
    }
};

__global__ __launch_bounds__(256, 1) void joint_loss_dz(JointLossP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jl_smem[];
    float* biasl = reinterpret_cast<float*>(jl_smem + 2 * JL_STAGE);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int c = blockIdx.x % P.NC, ub = (blockIdx.x / P.NC) % P.NUB, b = blockIdx.x / (P.NC * P.NUB);
    const int Tb = ldgi(P.lens + b), Ub = ldgi(P.lens + P.B + b);
    const int u = 16 * ub + i, uc = min(u, P.U - 1);
    const bool ulive = u < P.U && u <= Ub;
    const float* prow = P.p + ((long long)b * P.U + uc) * RNNT_D;
    const int y = ulive && u < Ub ? ldgi(P.targets + (long long)b * P.ts + u) : -1;
    const float rs = ldg1(P.row_scale + b);
    f32x4_ dpacc[16];
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) dpacc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
    for (int v = tid; v < JL_BIAS; v += 256) biasl[v] = v < P.V ? ldg1(P.bias + v) : 0.f;
    // stage 0 of the stream
    uint4 wreg[8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
        for (int n = 0; n < 8; ++n) wreg[n] = *reinterpret_cast<const uint4*>(P.wz + hf * JL_HALF + (tid + 256 * n) * 16);
#pragma unroll
        for (int n = 0; n < 8; ++n) *reinterpret_cast<uint4*>(jl_smem + hf * JL_HALF + (tid + 256 * n) * 16) = wreg[n];
    }
    __syncthreads();
    int par = 0;
    const int nit = P.TC / 4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int it = 0; it < nit; ++it) {
        const int t = c * P.TC + 4 * it + wave, tc = min(t, P.T - 1);
        const bool tin = t < P.T, live = tin && t < Tb && ulive;
        const float* erow = P.e + ((long long)b * P.T + tc) * RNNT_D;
        // the frame's h as the forward's B operand: lane (i, q) holds h[cell i][32 ks + 8 q + 0..7]
        uint4 ah[8], al[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int k0 = 32 * ks + 8 * q;
            const float4 e0 = live ? ldg4(erow + k0) : z4, e1 = live ? ldg4(erow + k0 + 4) : z4;
            const float4 p0 = live ? ldg4(prow + k0) : z4, p1 = live ? ldg4(prow + k0 + 4) : z4;
            const float4 v0 = make_float4(live ? jg_h(e0.x, p0.x) : 0.f, live ? jg_h(e0.y, p0.y) : 0.f, live ? jg_h(e0.z, p0.z) : 0.f, live ? jg_h(e0.w, p0.w) : 0.f);
            const float4 v1 = make_float4(live ? jg_h(e1.x, p1.x) : 0.f, live ? jg_h(e1.y, p1.y) : 0.f, live ? jg_h(e1.z, p1.z) : 0.f, live ? jg_h(e1.w, p1.w) : 0.f);
            split8_16<false, true>(v0, v1, ah[ks], al[ks]);
        }
        const float4 cf = live ? ldg4(P.coef + 4 * (((long long)b * P.T + tc) * P.U + uc)) : z4;
        f32x4_ acc[16];
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) acc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < P.KS; ++s) {
            const int ns = s + 1 == P.KS ? 0 : s + 1;            // (behind the very last k-step: stage 0 once more, unused)
            const unsigned char* src = P.wz + (long long)ns * JL_STAGE;
            const unsigned char* buf = jl_smem + par * JL_STAGE + lane * 16;
            unsigned char* nbuf = jl_smem + (par ^ 1) * JL_STAGE;
#pragma unroll
            for (int n = 0; n < 8; ++n) wreg[n] = *reinterpret_cast<const uint4*>(src + (tid + 256 * n) * 16);
            // z of 16 cells x 32 vocabulary entries: rows 32 s + 16 tt + 4 q + r, column = cell i
            f32x4_ z[2];
            z[0] = *reinterpret_cast<const f32x4_*>(biasl + 32 * s + 4 * q);
            z[1] = *reinterpret_cast<const f32x4_*>(biasl + 32 * s + 16 + 4 * q);
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const uint4 wh = *reinterpret_cast<const uint4*>(buf + ((tt * 8 + ks) * 2) * 1024), wl = *reinterpret_cast<const uint4*>(buf + ((tt * 8 + ks) * 2 + 1) * 1024);
                    z[tt] = mfma16_<false>(wh, al[ks], z[tt]);
                    z[tt] = mfma16_<false>(wl, ah[ks], z[tt]);
                    z[tt] = mfma16_<false>(wh, ah[ks], z[tt]);
                }
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) *reinterpret_cast<uint4*>(nbuf + (tid + 256 * n) * 16) = wreg[n];
#pragma unroll
            for (int n = 0; n < 8; ++n) wreg[n] = *reinterpret_cast<const uint4*>(src + JL_HALF + (tid + 256 * n) * 16);
            // g in place: the lane's eight values are slots 0..7 of its K group in the dh half's permutation
            float gv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * s + 16 * (j >> 2) + 4 * q + (j & 3);
                const float g = loss_g<true>(z[j >> 2][j & 3], k, cf, P.blank, y, P.clamp) * rs;
                gv[j] = live && k < P.V ? g : 0.f;
            }
            uint4 gh, gl;
            split8_16<false, true>(make_float4(gv[0], gv[1], gv[2], gv[3]), make_float4(gv[4], gv[5], gv[6], gv[7]), gh, gl);
#pragma unroll
            for (int t16 = 0; t16 < 16; ++t16) {
                const uint4 wh = *reinterpret_cast<const uint4*>(buf + JL_HALF + (2 * t16) * 1024), wl = *reinterpret_cast<const uint4*>(buf + JL_HALF + (2 * t16 + 1) * 1024);
                acc[t16] = mfma16_<false>(wl, gh, acc[t16]);
                acc[t16] = mfma16_<false>(wh, gl, acc[t16]);
                acc[t16] = mfma16_<false>(wh, gh, acc[t16]);
            }
#pragma unroll
            for (int n = 0; n < 8; ++n) *reinterpret_cast<uint4*>(nbuf + JL_HALF + (tid + 256 * n) * 16) = wreg[n];
            __syncthreads();                                     // the next stage is in LDS, everyone is done reading this one
            par ^= 1;
        }
        // dz on the accumulators: lane = cell (frame t, u), hidden 16 t16 + 4 q + 0..3
        float* derow = P.de_part + (((long long)ub * P.B + b) * P.T + tc) * RNNT_D + 4 * q;
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) {
            const float4 e4 = live ? ldg4(erow + 16 * t16 + 4 * q) : z4, p4 = live ? ldg4(prow + 16 * t16 + 4 * q) : z4;
            const float h0 = jg_h(e4.x, p4.x), h1 = jg_h(e4.y, p4.y), h2 = jg_h(e4.z, p4.z), h3 = jg_h(e4.w, p4.w);
            f32x4_ dz;
            dz[0] = live ? acc[t16][0] * fmaf(-h0, h0, 1.0f) : 0.f;
            dz[1] = live ? acc[t16][1] * fmaf(-h1, h1, 1.0f) : 0.f;
            dz[2] = live ? acc[t16][2] * fmaf(-h2, h2, 1.0f) : 0.f;
            dz[3] = live ? acc[t16][3] * fmaf(-h3, h3, 1.0f) : 0.f;
            dpacc[t16] += dz;
            auto rowsum = [](float v) {                          // sum over the 16 cells of the row: joint_grad_dz's butterfly
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
    // d_p of the chunk: the four waves' sums added in wave order through LDS (free behind the last barrier)
    float* red = reinterpret_cast<float*>(jl_smem);
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) *reinterpret_cast<f32x4_*>(red + (wave * 16 + i) * RNNT_D + 16 * t16 + 4 * q) = dpacc[t16];
    __syncthreads();
    for (int r = 0; r < 16; ++r) {
        if (16 * ub + r >= P.U) break;                           // uniform
        const float v = ((red[r * RNNT_D + tid] + red[(16 + r) * RNNT_D + tid]) + red[(32 + r) * RNNT_D + tid]) + red[(48 + r) * RNNT_D + tid];
        stg1(P.dp_part + (((long long)c * P.B + b) * P.U + 16 * ub + r) * RNNT_D + tid, v);
    }
}

__global__ __launch_bounds__(256, 2) void joint_loss_dw(JointLossP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char jl_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
    const int vs = blockIdx.x % P.NVS, sl = blockIdx.x / P.NVS;
    const int tv = 4 * vs + wave, v = 16 * tv + i;
    const bool vlive = v < P.V;
    const long long m0 = (long long)sl * P.CS, m1 = min(P.M, m0 + P.CS);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // the wave's 16 rows of W, for the workgroup's life: the B operand of z (lane (i, q): W[column i][32 ks + 8 q + 0..7])
    uint4 wbh[8], wbl[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const float* wr = P.w + (long long)min(v, P.V - 1) * RNNT_D + 32 * ks + 8 * q;
        split8_16<false, true>(vlive ? ldg4(wr) : z4, vlive ? ldg4(wr + 4) : z4, wbh[ks], wbl[ks]);
    }
    const float bv = vlive ? ldg1(P.bias + v) : 0.f;
    f32x4_ acc[16];
#pragma unroll
    for (int t16 = 0; t16 < 16; ++t16) acc[t16] = (f32x4_){0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
    // forming h, a thread takes hidden entries 4 lane + 0..3 of the eight cells of K group `wave`
    const int fks = lane >> 3, fq = (lane >> 1) & 3, fhalf = lane & 1;
    // Both stagings are swizzled so that the writes spread over the banks while the reads stay lane-linear permutations: a piece's 16-byte
    // slot `sl` lies at sl ^ x, x a function of the piece -- z half: x = ks ^ 8 (fq & 1) on the cell bits of the slot (the 64 writers of
    // one cell differ in ks, fq and the half only); dW half: x = t16 & 3 (16 consecutive writers differ in t16 and two slot bits).
    unsigned char* buf = jl_smem;
    for (long long c0 = m0; c0 < m1; c0 += 32) {
        float hv[8][4];
        JointLossCell cl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {                            // cell c0 + 16 (j / 4) + 4 wave + j % 4
            if ((j & 3) == 0) cl.at(c0 + 16 * (j >> 2) + 4 * wave, m1, P); else cl.next(m1, P);
            const float4 e4 = cl.live ? ldg4(P.e + (long long)cl.bt * RNNT_D + 4 * lane) : z4;
            const float4 p4 = cl.live ? ldg4(P.p + ((long long)cl.b * P.U + cl.u) * RNNT_D + 4 * lane) : z4;
            hv[j][0] = cl.live ? jg_h(e4.x, p4.x) : 0.f;
            hv[j][1] = cl.live ? jg_h(e4.y, p4.y) : 0.f;
            hv[j][2] = cl.live ? jg_h(e4.z, p4.z) : 0.f;
            hv[j][3] = cl.live ? jg_h(e4.w, p4.w) : 0.f;
        }
        __syncthreads();                                         // everyone is done reading the previous step's planes
        // hidden along K (z's A operand): piece ((ct 8 + ks) 2 + plane), lane (i = cell % 16, q), 8 bytes of its 16
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float r0, r1, r2, r3, d0, d1;
            uint2 hh, hl;
            hh.x = pack2_16<false>(hv[j][0], hv[j][1], r0, r1);
            hh.y = pack2_16<false>(hv[j][2], hv[j][3], r2, r3);
            hl.x = pack2_16<false>(r0, r1, d0, d1);
            hl.y = pack2_16<false>(r2, r3, d0, d1);
            const int slot = (16 * fq + 4 * wave + (j & 3)) ^ (fks ^ ((fq & 1) << 3));
            unsigned char* dst = buf + (((j >> 2) * 8 + fks) * 2) * 1024 + slot * 16 + 8 * fhalf;
            *reinterpret_cast<uint2*>(dst) = hh;
            *reinterpret_cast<uint2*>(dst + 1024) = hl;
        }
        // cells along K (dW's B operand): piece 2 t16 + plane, lane (i = hidden % 16, q = K group)
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            uint4 hh, hl;
            split8_16<false, true>(make_float4(hv[0][n], hv[1][n], hv[2][n], hv[3][n]), make_float4(hv[4][n], hv[5][n], hv[6][n], hv[7][n]), hh, hl);
            const int slot = (16 * wave + 4 * (lane & 3) + n) ^ ((lane >> 2) & 3);
            unsigned char* dst = buf + JL_HALF + (2 * (lane >> 2)) * 1024 + slot * 16;
            *reinterpret_cast<uint4*>(dst) = hh;
            *reinterpret_cast<uint4*>(dst + 1024) = hl;
        }
        // the factors of this lane's eight cells (K group q) -- asked for in front of the barrier, behind the staging (h is dead by now)
        float4 cf[8];
        float rs[8];
        int yy[8];
        unsigned livem = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((j & 3) == 0) cl.at(c0 + 16 * (j >> 2) + 4 * q, m1, P); else cl.next(m1, P);
            const bool lv = cl.live && vlive;
            cf[j] = lv ? ldg4(P.coef + 4 * cl.m) : z4;
            rs[j] = lv ? ldg1(P.row_scale + cl.b) : 0.f;
            yy[j] = lv && cl.u < ldgi(P.lens + P.B + cl.b) ? ldgi(P.targets + (long long)cl.b * P.ts + cl.u) : -1;
            livem |= lv ? 1u << j : 0u;
        }
        __syncthreads();                                         // the step's h planes are in LDS
        // z of 32 cells x the wave's 16 columns: rows = cells 16 ct + 4 q + r, column i
        f32x4_ z[2] = {(f32x4_){bv, bv, bv, bv}, (f32x4_){bv, bv, bv, bv}};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const unsigned char* rd = buf + (lane ^ (ks ^ ((q & 1) << 3))) * 16;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const uint4 hh = *reinterpret_cast<const uint4*>(rd + ((ct * 8 + ks) * 2) * 1024), hl = *reinterpret_cast<const uint4*>(rd + ((ct * 8 + ks) * 2 + 1) * 1024);
                z[ct] = mfma16_<false>(hl, wbh[ks], z[ct]);
                z[ct] = mfma16_<false>(hh, wbl[ks], z[ct]);
                z[ct] = mfma16_<false>(hh, wbh[ks], z[ct]);
            }
        }
        float gj[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float g = loss_g<true>(z[j >> 2][j & 3], v, cf[j], P.blank, yy[j], P.clamp) * rs[j];
            gj[j] = (livem >> j) & 1u ? g : 0.f;
        }
        uint4 ah, al;
        split8_16<false, true>(make_float4(gj[0], gj[1], gj[2], gj[3]), make_float4(gj[4], gj[5], gj[6], gj[7]), ah, al);
        dbacc += ((gj[0] + gj[1]) + (gj[2] + gj[3])) + ((gj[4] + gj[5]) + (gj[6] + gj[7]));
#pragma unroll
        for (int t16 = 0; t16 < 16; ++t16) {
            const unsigned char* rd = buf + JL_HALF + (lane ^ (t16 & 3)) * 16;
            const uint4 bh = *reinterpret_cast<const uint4*>(rd + (2 * t16) * 1024), bl = *reinterpret_cast<const uint4*>(rd + (2 * t16 + 1) * 1024);
            acc[t16] = mfma16_<false>(al, bh, acc[t16]);
            acc[t16] = mfma16_<false>(ah, bl, acc[t16]);
            acc[t16] = mfma16_<false>(ah, bh, acc[t16]);
        }
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
