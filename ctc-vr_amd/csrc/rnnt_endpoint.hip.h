// Per-slot endpoint detection of the stream pool (api_pool_endpoint.hip.inc): the CTC head's blank log-posterior per encoder frame,
// and a trailing-blank rule in the shape of WeNet's runtime endpointer, kept per slot on the device.
//
// Semantics (the one statement of them; endpoint_scan below is the code, the kernel and rnnt_endpoint_scan_host both call it).
// State per slot: frames, trailing, speech, rule, at -- all 0 after open / reset.  For every new encoder frame, in order, with lp its
// blank log-posterior and log_thr = (float)log((double)blank_threshold):
//     frames += 1;  lp > log_thr ? trailing += 1 : (trailing = 0, speech += 1)          (a NaN compares false: speech)
//     if (rule == 0)  rule 1: R1 > 0, speech <  S, trailing >= R1      nothing said yet, and silence
//                     rule 2: R2 > 0, speech >= S, trailing >= R2      something said, then silence
//                     rule 3: R3 > 0, frames >= R3                     the utterance is too long
//                     the lowest-numbered true rule is recorded with at = frames
// Rules are evaluated per frame, the first to fire is sticky, the counters run on: a slot's state depends on its frames only, never on
// how they were split into calls.  "Something was said" is the CTC speech count, not "the decoder has tokens": one rule for every slot
// kind, and the device needs nothing from the decoders.  A caller who wants the decoder-based form applies it on the host from the
// returned frames / trailing and its own tokens.
#pragma once
#include "rnnt_common.hip.h"

// config of one slot as the device holds it (pool_endpoint_set writes it): the threshold already as a log, the on flag with it
struct EpCfg {
    float log_thr;
    int min_speech, r1, r2, r3, on;
};
constexpr int EP_STATE_INTS = 5;   // frames, trailing, speech, rule, at
constexpr int EP_TILE = 4;         // frames staged in LDS at a time (t' = 3 or 4 at 16-frame chunks)
constexpr int EP_ROWS = 8;         // weight rows a wave reduces side by side
constexpr int EP_WAVES = 8, EP_THREADS = 64 * EP_WAVES;

__host__ __device__ inline void endpoint_scan(const float* lp, int t, float log_thr, int S, int R1, int R2, int R3, int* st) {
    int frames = st[0], trailing = st[1], speech = st[2], rule = st[3], at = st[4];
    for (int f = 0; f < t; ++f) {
        frames += 1;
        if (lp[f] > log_thr) trailing += 1;
        else { trailing = 0; speech += 1; }
        if (rule == 0) {
            const int r = (R1 > 0 && speech < S && trailing >= R1) ? 1 : (R2 > 0 && speech >= S && trailing >= R2) ? 2 : (R3 > 0 && frames >= R3) ? 3 : 0;
            if (r) { rule = r; at = frames; }
        }
    }
    st[0] = frames; st[1] = trailing; st[2] = speech; st[3] = rule; st[4] = at;
}

// LDS of one workgroup: the staged frames, the per-wave (max, sum) of the online softmax and the blank logit per frame, the results
struct EpLds {
    alignas(16) float x[EP_TILE][RNNT_D];
    float m[EP_WAVES][EP_TILE], s[EP_WAVES][EP_TILE], zb[EP_TILE], lp[EP_TILE];
};

// lp[f] = log_softmax(W x_f + b)[blank] for the nf <= EP_TILE frames src[0 .. nf)[256] (16-byte aligned), left in L.lp[0 .. nf) and
// visible to every lane on return.  EP_THREADS lanes; the frames are staged in LDS once (rows beyond nf as zeros).  Wave w takes the
// vocabulary rows v = w, w + EP_WAVES, ..., EP_ROWS of them at a time so that neither a row's read nor its reduction is waited for
// alone: ONE coalesced 1 KB read of W[v] per row (a float4 per lane) against all staged frames, f32 FMAs, then a transposing
// butterfly over the EP_ROWS rows side by side -- each exchange hands over the half of the frames the partner keeps, over lanes ^32
// and ^16, then plain steps ^8 .. ^1 -- after which the 16 lanes of group g = lane >> 4 hold frame g's logits: 6 exchanges per row
// for 4 frames instead of 4 x 6.  Per frame that IS the descending butterfly of wave_sum, step for step.  Every lane keeps the online
// (max, sum) of its frame, updated in row order; the waves' pairs and the blank logit meet in LDS and are combined in wave order.
// Nothing of size rows x V leaves the CU.  The tree, the row order and the combine order are fixed, so a frame's value does not
// depend on its place in a tile or a call.
__device__ __forceinline__ void ctc_blank_tile(EpLds& L, const float* __restrict__ src, int nf, const float* __restrict__ W, const float* __restrict__ bias,
                                               int V, int blank) {
    constexpr int GROUP = 64 / EP_TILE;                            // lanes that end up with the same frame
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                               // the previous tile's readers are done with L
    for (int id = tid; id < EP_TILE * (RNNT_D / 4); id += EP_THREADS) {
        const int f = id >> 6, c4 = id & 63;
        *reinterpret_cast<float4*>(&L.x[f][c4 * 4]) = f < nf ? ldg4(src + (long long)f * RNNT_D + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int g = lane / GROUP;                                    // the frame this lane ends up with
    float m = -3.4028234e38f, s = 0.f, zb = 0.f;
    for (int v0 = wave; v0 < V; v0 += EP_WAVES * EP_ROWS) {
        float a[EP_ROWS][EP_TILE];
#pragma unroll
        for (int u = 0; u < EP_ROWS; ++u) {
            const int v = v0 + EP_WAVES * u;
            const float4 w = ldg4(W + (long long)(v < V ? v : V - 1) * RNNT_D + lane * 4);   // beyond the vocabulary: the last row again, unused
#pragma unroll
            for (int f = 0; f < EP_TILE; ++f) {
                const float4 x = *reinterpret_cast<const float4*>(&L.x[f][lane * 4]);
                a[u][f] = fmaf(w.w, x.w, fmaf(w.z, x.z, fmaf(w.y, x.y, w.x * x.x)));
            }
        }
        // lanes with bit 5 set keep the upper half of the frames, bit 4 picks a half of that half: frame = lane / GROUP
#pragma unroll
        for (int h = EP_TILE / 2, o = 32; h >= 1; h >>= 1, o >>= 1) {
            const bool up = (lane & o) != 0;
#pragma unroll
            for (int u = 0; u < EP_ROWS; ++u)
#pragma unroll
                for (int k = 0; k < h; ++k) {
                    const float keep = up ? a[u][k + h] : a[u][k], send = up ? a[u][k] : a[u][k + h];
                    a[u][k] = keep + __shfl_xor(send, o, 64);
                }
        }
#pragma unroll
        for (int o = GROUP / 2; o >= 1; o >>= 1)
#pragma unroll
            for (int u = 0; u < EP_ROWS; ++u) a[u][0] += __shfl_xor(a[u][0], o, 64);
#pragma unroll
        for (int u = 0; u < EP_ROWS; ++u) {
            const int v = v0 + EP_WAVES * u;
            if (v < V) {                                           // uniform over the wave
                const float z = a[u][0] + ldg1(bias + v);
                const float mn = fmaxf(m, z);
                s = s * expf(m - mn) + expf(z - mn);
                m = mn;
                if (v == blank) zb = z;
            }
        }
    }
    if ((lane & (GROUP - 1)) == 0) {
        L.m[wave][g] = m;
        L.s[wave][g] = s;
        if (blank % EP_WAVES == wave) L.zb[g] = zb;
    }
    __syncthreads();
    if (tid < EP_TILE) {
        float M = L.m[0][tid];
#pragma unroll
        for (int w = 1; w < EP_WAVES; ++w) M = fmaxf(M, L.m[w][tid]);
        float S = 0.f;
#pragma unroll
        for (int w = 0; w < EP_WAVES; ++w) S += L.s[w][tid] * expf(L.m[w][tid] - M);
        L.lp[tid] = L.zb[tid] - (M + logf(S));
    }
    __syncthreads();
}

// rnnt_ctc_blank_logprob: out[r] = log_softmax(ctc_lo(enc[r]))[blank] for rows rows of enc [rows][256]; one workgroup per EP_TILE rows
__global__ __launch_bounds__(EP_THREADS) void ctc_blank_rows(const float* __restrict__ enc, float* __restrict__ out, int rows, const float* __restrict__ W,
                                                             const float* __restrict__ bias, int V, int blank) {
    __shared__ EpLds L;
    const int r0 = blockIdx.x * EP_TILE;
    const int nf = rows - r0 < EP_TILE ? rows - r0 : EP_TILE;
    if (nf <= 0) return;
    ctc_blank_tile(L, enc + (long long)r0 * RNNT_D, nf, W, bias, V, blank);
    if ((int)threadIdx.x < nf) stg1(out + r0 + threadIdx.x, L.lp[threadIdx.x]);
}

// Every pool call that lists an endpoint slot (and rnnt_pool_endpoint_frames): the t compact rows src[i * t .. i * t + t)[256] of active
// row i advance the state of slot slots[i].  One workgroup per active row -- slots of a call are distinct, so a state has one reader
// and one writer (lane 0) -- which leaves at once when the slot's endpointing is off.  The frames go through ctc_blank_tile EP_TILE
// at a time; lane 0 runs endpoint_scan over each tile's log-posteriors with the state in registers and stores it once at the end.
__global__ __launch_bounds__(EP_THREADS) void pool_endpoint(const float* __restrict__ src, const int* __restrict__ slots, const EpCfg* __restrict__ cfg,
                                                            int* __restrict__ state, int t, const float* __restrict__ W, const float* __restrict__ bias,
                                                            int V, int blank) {
    __shared__ EpLds L;
    const int i = blockIdx.x, slot = ldgi(slots + i);
    const EpCfg c = cfg[slot];
    if (!c.on) return;                                             // uniform over the workgroup
    int st[EP_STATE_INTS];
    if (threadIdx.x == 0)
        for (int k = 0; k < EP_STATE_INTS; ++k) st[k] = state[slot * EP_STATE_INTS + k];
    for (int f0 = 0; f0 < t; f0 += EP_TILE) {
        const int nf = t - f0 < EP_TILE ? t - f0 : EP_TILE;
        ctc_blank_tile(L, src + ((long long)i * t + f0) * RNNT_D, nf, W, bias, V, blank);
        if (threadIdx.x == 0) endpoint_scan(L.lp, nf, c.log_thr, c.min_speech, c.r1, c.r2, c.r3, st);
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < EP_STATE_INTS; ++k) state[slot * EP_STATE_INTS + k] = st[k];
}

// config `value` (its on flag included) and a zero state for slots [slot0, slot0 + n)
__global__ void pool_endpoint_set(EpCfg* cfg, int* state, int slot0, int n, EpCfg value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cfg[slot0 + i] = value;
    for (int k = 0; k < EP_STATE_INTS; ++k) state[(slot0 + i) * EP_STATE_INTS + k] = 0;
}
