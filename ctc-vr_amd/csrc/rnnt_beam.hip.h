// Beam search kernels: per-step reduction (launched path), per-hypothesis extension chain, state-pool gather, lattice log-softmax.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
#pragma once

// ------------------------------------------------------------------------------------------------
// beam_reduce: one wave per hypothesis row, one step of the extension chain of
// _decode_chunk_beam_search (online_rnnt_model.py:446-499): log_softmax statistics, blank log-prob,
// top-k non-blank (value desc, index asc), stop test `blank >= max - 1e-6` in double (:486), else the
// row's next predictor input is its best non-blank token.
// ------------------------------------------------------------------------------------------------
struct BeamOut {
    int* active;      // [R]
    int* tok;         // [R] predictor input token (updated when the chain continues)
    int* steps;       // [R] steps evaluated so far
    float* blank_lp;  // [R][n_steps]
    float* top_lp;    // [R][n_steps][k]
    int* top_tok;     // [R][n_steps][k]
    int* n_active;    // [1]
};

// Any vocabulary size: strided passes over the row (the first version kept the row in 8 registers per lane and silently
// ignored tokens >= 512); k <= 64 winners are excluded through a small LDS list.
__global__ __launch_bounds__(64) void beam_reduce(const float* __restrict__ logits, int ldl, int vocab, int blank, int k, int step,
                                                int n_steps, BeamOut o) {
    __shared__ int chosen[64];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (!o.active[r]) return;
    const float* x = logits + (long long)r * ldl;
    float mx = -INFINITY;
    for (int idx = lane; idx < vocab; idx += 64) mx = fmaxf(mx, x[idx]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int idx = lane; idx < vocab; idx += 64) se += expf(x[idx] - mx);
    const float lse = logf(wave_sum(se));
    const float blank_lp = (x[blank] - mx) - lse;
    const float max_lp = (mx - mx) - lse;
    int best_tok = 0;
    for (int t = 0; t < k; ++t) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int idx = lane; idx < vocab; idx += 64) {
            if (idx == blank) continue;
            bool taken = false;
            for (int c = 0; c < t; ++c) taken = taken || chosen[c] == idx;
            if (taken) continue;
            const float lp = (x[idx] - mx) - lse;
            if (lp > bv) { bv = lp; bi = idx; }          // ascending scan: ties keep the lower index
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            chosen[t] = bi;
            o.top_lp[((long long)r * n_steps + step) * k + t] = bv;
            o.top_tok[((long long)r * n_steps + step) * k + t] = bi;
        }
        __syncthreads();
        if (t == 0) best_tok = bi;
    }
    if (lane == 0) {
        o.blank_lp[(long long)r * n_steps + step] = blank_lp;
        o.steps[r] = step + 1;
        const bool stop = ((double)blank_lp >= (double)max_lp - 1e-6) || (step + 1 >= n_steps);
        if (stop) {
            o.active[r] = 0;
            atomicSub(o.n_active, 1);
        } else {
            o.tok[r] = best_tok;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// beam_chain: the whole extension chain of ONE hypothesis row for one encoder frame as one workgroup (512 threads) --
// the loop of _decode_chunk_beam_search (online_rnnt_model.py:446-499) that the launched path runs as 5 kernels and one
// host synchronisation per step: predictor step (table row + W_hh product + cell), projection, joint.pred_ffn,
// tanh(enc_ffn(enc)[t] + .), vocabulary projection, log-softmax statistics, blank log-prob, top-k non-blank, stop test,
// next input token = best non-blank.  Rows are independent, so 64 streams x 4 hypotheses fill the 256 CUs; every
// intermediate LSTM state goes to the row's pool slots exactly as in the launched path.
// ------------------------------------------------------------------------------------------------
struct BeamChainP {
    const float* whh; const float* egate; const float* wpr; const float* bpr; const float* wpf; const float* bpf;
    const float* wout; const float* bout; const float* encp;
    float* pool;                 // [R][slots][512] (h | c); slot 0 = state before the first evaluation
    const int* frame;            // [R] row of encp
    const int* tok_in;           // [R] predictor input token of the first evaluation
    const int* live;             // [R] or nullptr: rows with live[r] == 0 do nothing (fixed-slot rows of rnnt_beam_decode)
    int* steps; float* blank_lp; float* top_lp; int* top_tok;
    int vocab, blank, k, n_steps, slots;
};

// The chain of row r (its outputs go to steps / blank_lp / top_lp / top_tok [r]): `pool` is the row's state slots, `tok` the predictor
// input of the first evaluation, `enc` the projected encoder frame.  One body for beam_chain and beam_chain_pool: the arithmetic of
// a row does not depend on how the row was found.
__device__ __forceinline__ void beam_chain_row(const BeamChainP& p, const int r, float* pool, int tok, const float* enc) {
    constexpr int NTH = 512;
    __shared__ __attribute__((aligned(16))) float hs[1][RNNT_D], cs[RNNT_D], h2[1][RNNT_D], pr[1][RNNT_D], zs[1][RNNT_D];
    __shared__ __attribute__((aligned(16))) float gates[4 * RNNT_D];
    __shared__ float lg[512];
    __shared__ int s_ctl[2];
    const int tid = threadIdx.x;
    if (tid < RNNT_D) { hs[0][tid] = ldg1(pool + tid); cs[tid] = ldg1(pool + RNNT_D + tid); }
    __syncthreads();
    int st = 0;
    for (; st < p.n_steps; ++st) {
        // predictor.forward_step (predictor.py:185-210): LSTM cell on (embed[tok], state slot st) -> slot st + 1
        dec_matvec<1, NTH>(p.whh, 4 * RNNT_D, hs, [&](int n, const float* acc) {
            gates[n] = acc[0] + ldg1(p.egate + (long long)tok * (4 * RNNT_D) + n);
        });
        __syncthreads();
        if (tid < RNNT_D) {
            const float4 gt = *reinterpret_cast<const float4*>(&gates[4 * tid]);
            const float cc = sigmoidf_(gt.y) * cs[tid] + sigmoidf_(gt.x) * tanhf(gt.z);
            const float hh = sigmoidf_(gt.w) * tanhf(cc);
            cs[tid] = cc;                                          // the chain continues from the new state
            h2[0][tid] = hh;
            stg1(pool + (long long)(st + 1) * 512 + tid, hh);
            stg1(pool + (long long)(st + 1) * 512 + RNNT_D + tid, cc);
        }
        __syncthreads();
        if (tid < RNNT_D) hs[0][tid] = h2[0][tid];
        dec_matvec<1, NTH>(p.wpr, RNNT_D, h2, [&](int n, const float* acc) { pr[0][n] = acc[0] + ldg1(p.bpr + n); });   // predictor.projection
        __syncthreads();
        dec_matvec<1, NTH>(p.wpf, RNNT_D, pr, [&](int n, const float* acc) {                                           // joint (joint.py:54-66)
            zs[0][n] = tanhf(acc[0] + ldg1(p.bpf + n) + ldg1(enc + n));
        });
        __syncthreads();
        dec_matvec<1, NTH>(p.wout, p.vocab, zs, [&](int n, const float* acc) { lg[n] = acc[0] + ldg1(p.bout + n); });
        __syncthreads();
        if (tid < 64) {   // log_softmax statistics, blank log-prob, top-k non-blank (value desc, index asc), stop test (:468,:486)
            const int lane = tid;
            float v[8];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = lane + 64 * j;
                v[j] = idx < p.vocab ? lg[idx] : -INFINITY;
                mx = fmaxf(mx, v[j]);
            }
            mx = wave_max(mx);
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) se += (lane + 64 * j) < p.vocab ? expf(v[j] - mx) : 0.f;
            const float lse = logf(wave_sum(se));
            const float blank_lp = (lg[p.blank] - mx) - lse;
            const float max_lp = (mx - mx) - lse;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int idx = lane + 64 * j;
                v[j] = (idx < p.vocab && idx != p.blank) ? (v[j] - mx) - lse : -INFINITY;
            }
            int best_tok = 0;
            for (int t = 0; t < p.k; ++t) {
                float bv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (v[j] > bv) { bv = v[j]; bi = lane + 64 * j; }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const float ov = __shfl_xor(bv, off, 64);
                    const int oi = __shfl_xor(bi, off, 64);
                    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                if ((bi & 63) == lane) v[bi >> 6] = -INFINITY;   // remove the winner
                if (lane == 0) {
                    p.top_lp[((long long)r * p.n_steps + st) * p.k + t] = bv;
                    p.top_tok[((long long)r * p.n_steps + st) * p.k + t] = bi;
                }
                if (t == 0) best_tok = bi;
            }
            if (lane == 0) {
                p.blank_lp[(long long)r * p.n_steps + st] = blank_lp;
                s_ctl[0] = ((double)blank_lp >= (double)max_lp - 1e-6) || (st + 1 >= p.n_steps) ? 1 : 0;
                s_ctl[1] = best_tok;
            }
        }
        __syncthreads();
        if (s_ctl[0]) { ++st; break; }
        tok = s_ctl[1];
        __syncthreads();
    }
    if (tid == 0) p.steps[r] = st;
}

__global__ __launch_bounds__(512) void beam_chain(BeamChainP p) {
    const int r = blockIdx.x;
    if (p.live && !ldgi(p.live + r)) return;                       // whole workgroup: before the first barrier
    beam_chain_row(p, r, p.pool + (long long)r * p.slots * 512, ldgi(p.tok_in + r), p.encp + (long long)ldgi(p.frame + r) * RNNT_D);
}

// new_pool[r][0] <- old_pool[src_row[r]][src_step[r]]  (state = [h(256) | c(256)])
__global__ void beam_gather(const float* __restrict__ old_pool, float* __restrict__ new_pool, const int* __restrict__ src_row,
                            const int* __restrict__ src_step, int n_new, int slots) {
    const int r = blockIdx.x;
    if (r >= n_new) return;
    const float* s = old_pool + ((long long)src_row[r] * slots + src_step[r]) * 512;
    float* d = new_pool + (long long)r * slots * 512;
    for (int i = threadIdx.x; i < 512; i += blockDim.x) d[i] = s[i];
}

// ------------------------------------------------------------------------------------------------
// beam_merge_dev: the host half of one encoder frame (beam_merge_stream in api_beam.hip.inc, which stays the oracle) on the
// device, one workgroup per stream, followed by the state gather of beam_gather -- so that rnnt_beam_decode never returns to the
// host inside its frame loop.  Rows are fixed slots: hypothesis i of stream b is row b * width + i.
//   candidates  in the reference's order: per hypothesis, per evaluation st < steps[r], the blank candidate (pool slot st), then
//               the k top non-blank ones (slot st + 1); the chain continues with the best non-blank while st < n - 1
//   scores      f64, the host's additions in the host's order: lp + (double)blank_lp, lp + (double)top_lp[j], lp += top_lp[0]
//   order       std::stable_sort descending: repeated block-wide argmax, ties to the lower candidate index
//   de-dup      first wins, on the full token sequence: 64-bit running hash first, then length, then every token
//   truncation  to `beam` survivors
// A stream past its last frame (f >= fend[b]) is carried over unchanged into the other buffers.
// ------------------------------------------------------------------------------------------------
constexpr int BM_MAX_BEAM = 16, BM_MAX_STEPS = 10, BM_MAX_CAND = BM_MAX_BEAM * BM_MAX_STEPS * (BM_MAX_BEAM + 1), BM_NT = 256;
constexpr unsigned long long BEAM_HASH0 = 0xcbf29ce484222325ull;
// running hash of a token sequence (FNV-1a over 32-bit tokens): extended one token at a time, host and device alike
__host__ __device__ inline unsigned long long beam_hash_step(unsigned long long h, int tok) {
    return (h ^ (unsigned long long)(unsigned)tok) * 0x100000001b3ull;
}

struct BeamMergeP {
    const float* pool_in; float* pool_out;      // state pools [rows][slots][512]; pool_in == nullptr: no state gather
    const int* tk_in; int* tk_out;              // token lists [rows][lcap]
    const int* len_in; int* len_out;            // [rows]
    const double* sc_in; double* sc_out;        // [rows]
    const unsigned long long* hs_in; unsigned long long* hs_out;   // [rows]
    int* nh;                                    // [B] hypotheses per stream (read, then rewritten)
    const int* fend;                            // [B] first frame a stream does not have
    const int* steps; const float* blank_lp; const float* top_lp; const int* top_tok;   // beam_chain's outputs, [rows][n_steps](...)
    int* tok_next; int* frame_next; int* live;  // [rows] inputs of the next frame's beam_chain
    int* src_row; int* src_step;                // [rows] pool slot each survivor came from
    int slots, lcap, n_steps, k, beam, width, blank, f, fstride;
};

// One stream's merge (rows row0 .. row0 + width of p's buffers; b: its entry of nh / fend and its frame-buffer row).  One body for
// beam_merge_dev and beam_merge_pool.  fend == nullptr: the stream has frame f; tok_next == nullptr: the next chain finds its own
// inputs (beam_chain_pool), so tok_next / frame_next / live / src_row / src_step are not written.
__device__ __forceinline__ void beam_merge_stream_dev(const BeamMergeP& p, const int b) {
    __shared__ double sc[BM_MAX_CAND];
    __shared__ unsigned char taken[BM_MAX_CAND];
    __shared__ int h_base[BM_MAX_BEAM + 1], h_len[BM_MAX_BEAM];
    __shared__ int chain[BM_MAX_BEAM][BM_MAX_STEPS];                 // chain tokens: best non-blank of evaluation st
    __shared__ unsigned long long h_hash[BM_MAX_BEAM][BM_MAX_STEPS];  // hash of parent + chain[0..st)
    __shared__ int acc[BM_MAX_BEAM], acc_len[BM_MAX_BEAM];
    __shared__ unsigned long long acc_hash[BM_MAX_BEAM];
    __shared__ double red_v[BM_NT / 64];
    __shared__ int red_i[BM_NT / 64];
    __shared__ int s_best;
    const int tid = threadIdx.x, K1 = p.k + 1, row0 = b * p.width;
    const int nh = p.nh[b];
    if (p.fend && p.f >= p.fend[b]) {                                          // stream finished: carry its rows over unchanged
        for (int i = 0; i < nh; ++i) {
            const int r = row0 + i, len = p.len_in[r];
            for (int q = tid; q < len; q += BM_NT) p.tk_out[(long long)r * p.lcap + q] = p.tk_in[(long long)r * p.lcap + q];
            if (p.pool_in)
                for (int e = tid; e < 512; e += BM_NT) p.pool_out[(long long)r * p.slots * 512 + e] = p.pool_in[(long long)r * p.slots * 512 + e];
            if (tid == 0) { p.len_out[r] = len; p.sc_out[r] = p.sc_in[r]; p.hs_out[r] = p.hs_in[r]; }
        }
        if (tid < p.width) p.live[row0 + tid] = 0;
        return;
    }
    if (tid < nh) h_len[tid] = p.len_in[row0 + tid];
    if (tid == 0) {
        int c = 0;
        for (int i = 0; i < nh; ++i) { h_base[i] = c; c += p.steps[row0 + i] * K1; }
        h_base[nh] = c;
    }
    __syncthreads();
    const int C = h_base[nh];
    if (tid < nh) {                                                  // one thread per hypothesis: the host's additions, in order
        const int i = tid, r = row0 + i, n = p.steps[r];
        double lp = p.sc_in[r];
        unsigned long long h = p.hs_in[r];
        for (int st = 0; st < n; ++st) {
            const long long o = (long long)r * p.n_steps + st;
            double* c = sc + h_base[i] + st * K1;
            c[0] = lp + (double)p.blank_lp[o];
            for (int j = 0; j < p.k; ++j) c[1 + j] = lp + (double)p.top_lp[o * p.k + j];
            h_hash[i][st] = h;
            const int t0 = p.top_tok[o * p.k];
            chain[i][st] = t0;
            if (st < n - 1) { h = beam_hash_step(h, t0); lp += (double)p.top_lp[o * p.k]; }
        }
    }
    for (int c = tid; c < C; c += BM_NT) taken[c] = 0;
    __syncthreads();
    // candidate c -> (hypothesis i, evaluation st, top index j; j = -1: blank)
    auto decode = [&](int c, int& i, int& st, int& j) {
        i = 0;
        while (c >= h_base[i + 1]) ++i;
        const int q = c - h_base[i];
        st = q / K1;
        j = q - st * K1 - 1;
    };
    auto top_tok = [&](int i, int st, int j) { return p.top_tok[((long long)(row0 + i) * p.n_steps + st) * p.k + j]; };
    auto tok_at = [&](int i, int st, int j, int q) {
        const int pl = h_len[i];
        if (q < pl) return p.tk_in[(long long)(row0 + i) * p.lcap + q];
        if (q < pl + st) return chain[i][q - pl];
        return top_tok(i, st, j);
    };
    const int lane = tid & 63, w = tid >> 6;
    int n_acc = 0;
    while (n_acc < p.beam) {
        double bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = tid; c < C; c += BM_NT)
            if (!taken[c] && (sc[c] > bv || (sc[c] == bv && c < bi))) { bv = sc[c]; bi = c; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[w] = bv; red_i[w] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < BM_NT / 64; ++q)
                if (red_v[q] > bv || (red_v[q] == bv && red_i[q] < bi)) { bv = red_v[q]; bi = red_i[q]; }
            s_best = bi;
            if (bi != 0x7fffffff) taken[bi] = 1;
        }
        __syncthreads();
        const int c = s_best;
        if (c == 0x7fffffff) break;                                  // candidates exhausted
        int i, st, j;
        decode(c, i, st, j);
        const int len = h_len[i] + st + (j >= 0 ? 1 : 0);
        const unsigned long long hc = j >= 0 ? beam_hash_step(h_hash[i][st], top_tok(i, st, j)) : h_hash[i][st];
        bool dup = false;
        for (int a = 0; a < n_acc && !dup; ++a) {
            if (acc_hash[a] != hc || acc_len[a] != len) continue;    // uniform across the workgroup
            int i2, st2, j2;
            decode(acc[a], i2, st2, j2);
            int diff = 0;
            for (int q = tid; q < len; q += BM_NT) diff |= tok_at(i, st, j, q) != tok_at(i2, st2, j2, q);
            dup = !__syncthreads_or(diff);                           // equal hashes of different sequences never merge
        }
        if (!dup) {
            if (tid == 0) { acc[n_acc] = c; acc_len[n_acc] = len; acc_hash[n_acc] = hc; }
            ++n_acc;
        }
        __syncthreads();
    }
    // survivors -> rows row0 + a of the other buffers: token list, score, hash, LSTM state, inputs of the next frame
    for (int a = 0; a < n_acc; ++a) {
        const int c = acc[a], nr = row0 + a, len = acc_len[a];
        int i, st, j;
        decode(c, i, st, j);
        const int sstep = j >= 0 ? st + 1 : st;
        for (int q = tid; q < len; q += BM_NT) p.tk_out[(long long)nr * p.lcap + q] = tok_at(i, st, j, q);
        if (p.pool_in) {
            const float* src = p.pool_in + ((long long)(row0 + i) * p.slots + sstep) * 512;
            float* dst = p.pool_out + (long long)nr * p.slots * 512;
            for (int e = tid; e < 512; e += BM_NT) dst[e] = src[e];
        }
        if (tid == 0) {
            p.len_out[nr] = len;
            p.sc_out[nr] = sc[c];
            p.hs_out[nr] = acc_hash[a];
            if (p.tok_next) {
                p.tok_next[nr] = len > 0 ? tok_at(i, st, j, len - 1) : p.blank;   // online_rnnt_model.py:429
                p.frame_next[nr] = b * p.fstride + p.f + 1;
                p.live[nr] = p.f + 1 < p.fend[b] ? 1 : 0;
                p.src_row[nr] = row0 + i;
                p.src_step[nr] = sstep;
            }
        }
    }
    if (p.tok_next && tid >= n_acc && tid < p.width) p.live[row0 + tid] = 0;
    if (tid == 0) p.nh[b] = n_acc;
}

__global__ __launch_bounds__(BM_NT) void beam_merge_dev(BeamMergeP p) { beam_merge_stream_dev(p, blockIdx.x); }

// ------------------------------------------------------------------------------------------------
// Stream pool (rnnt_pool_chunk_beam): every slot keeps its beam in HBM between calls, in FIXED rows -- hypothesis i of slot b is row
// b * W + i (W = max_beam) of two buffer sets (token lists [2][rows][lcap], lengths / scores / hashes [2][rows], state pools
// [2] x [rows][n_steps + 1][512]) -- and slots advance independently, so which set is current is per slot: cur0[a] at the call's
// first frame for active row a (host bookkeeping, sent with the call's table), flipped once per frame.  A launch covers the ACTIVE
// slots only: workgroup -> (active row, hypothesis) -> slot through the table; idle slots are neither read nor written.
// ------------------------------------------------------------------------------------------------
struct BeamPoolP {
    const int* slots;            // [n] slot of active row a (the decoder's slot list of the pool table)
    const int* cur0;             // [n] current buffer set of that slot at frame 0 of the call
    float* pool[2];              // state pools
    int* tk; int* len; double* sc; unsigned long long* hs;   // [2][rows](...)
    int* nh;                     // [slots] hypotheses per slot
    int rows, W, lcap, f, fstride;
};

// beam_chain for the live rows of the active slots at frame f of the call: input token = the hypothesis' last token (blank for the
// empty one, online_rnnt_model.py:429), encoder frame row slot * fstride + f, state pool of the slot's current set.
__global__ __launch_bounds__(512) void beam_chain_pool(BeamChainP p, BeamPoolP q) {
    const int a = blockIdx.x / q.W, i = blockIdx.x - a * q.W;
    const int slot = ldgi(q.slots + a);
    if (i >= ldgi(q.nh + slot)) return;                            // no hypothesis in this row: before the first barrier
    const int cur = (ldgi(q.cur0 + a) + q.f) & 1, r = slot * q.W + i;
    const long long cr = (long long)cur * q.rows + r;
    const int len = ldgi(q.len + cr);
    const int tok = len > 0 ? ldgi(q.tk + cr * q.lcap + len - 1) : p.blank;
    beam_chain_row(p, r, q.pool[cur] + (long long)r * p.slots * 512, tok, p.encp + ((long long)slot * q.fstride + q.f) * RNNT_D);
}

// beam_merge_dev's algorithm for one ACTIVE slot per workgroup: from the slot's current buffer set into its other one (the host
// flips its index once per frame).  p carries the call's scalars and beam_chain_pool's outputs; its buffer pointers are set here.
__global__ __launch_bounds__(BM_NT) void beam_merge_pool(BeamMergeP p, BeamPoolP q) {
    const int a = blockIdx.x, slot = ldgi(q.slots + a);
    const int cur = (ldgi(q.cur0 + a) + q.f) & 1, nxt = cur ^ 1;
    const long long ri = (long long)cur * q.rows, ro = (long long)nxt * q.rows;
    p.pool_in = q.pool[cur]; p.pool_out = q.pool[nxt];
    p.tk_in = q.tk + ri * q.lcap; p.tk_out = q.tk + ro * q.lcap;
    p.len_in = q.len + ri; p.len_out = q.len + ro;
    p.sc_in = q.sc + ri; p.sc_out = q.sc + ro;
    p.hs_in = q.hs + ri; p.hs_out = q.hs + ro;
    p.nh = q.nh;
    beam_merge_stream_dev(p, slot);
}

// rnnt_stream_open / rnnt_streams_reset for the per-slot beam state of slots [slot0, slot0 + gridDim.x): one empty hypothesis with
// score 0.0, the initial hash and the zero LSTM state (online_rnnt_model.py:407-415) in buffer set 0 (the host's index goes to 0
// with it).  Touches no other slot.  beam_slot_start: the same for one slot, by a workgroup of 256.
__device__ __forceinline__ void beam_slot_start(const BeamPoolP& q, int slot, int state_slots) {
    const int r0 = slot * q.W;
    for (int e = threadIdx.x; e < 512; e += 256) q.pool[0][(long long)r0 * state_slots * 512 + e] = 0.f;
    if (threadIdx.x < q.W) { q.len[r0 + threadIdx.x] = 0; q.sc[r0 + threadIdx.x] = 0.0; q.hs[r0 + threadIdx.x] = BEAM_HASH0; }
    if (threadIdx.x == 0) q.nh[slot] = 1;
}
__global__ __launch_bounds__(256) void beam_slot_reset(BeamPoolP q, int slot0, int state_slots) { beam_slot_start(q, slot0 + blockIdx.x, state_slots); }

// End of rnnt_beam_decode: fixed-slot row r = b * width + i (i < nh[b]) -> compacted row (hypotheses of streams < b) + i,
// LSTM state into slot 0 of the other pool, token list / length / score into the other token buffers.
__global__ __launch_bounds__(128) void beam_compact(const float* __restrict__ pool_in, float* __restrict__ pool_out, int slots,
                                                    const int* __restrict__ tk_in, int* __restrict__ tk_out, int lcap,
                                                    const int* __restrict__ len_in, int* __restrict__ len_out,
                                                    const double* __restrict__ sc_in, double* __restrict__ sc_out,
                                                    const int* __restrict__ nh, int width) {
    const int r = blockIdx.x, b = r / width, i = r - b * width;
    if (i >= nh[b]) return;
    int dst = i;
    for (int q = 0; q < b; ++q) dst += nh[q];
    const float* s = pool_in + (long long)r * slots * 512;
    float* d = pool_out + (long long)dst * slots * 512;
    for (int e = threadIdx.x; e < 512; e += blockDim.x) d[e] = s[e];
    const int len = len_in[r];
    for (int q = threadIdx.x; q < len; q += blockDim.x) tk_out[(long long)dst * lcap + q] = tk_in[(long long)r * lcap + q];
    if (threadIdx.x == 0) { len_out[dst] = len; sc_out[dst] = sc_in[r]; }
}

// log_softmax over the last dimension, in place, one wave per row (joint lattice mode 1).  A row (n <= 512 floats) is read
// ONCE into registers (8 values per lane), reduced, and written once: the pass is a pure HBM stream of 2 x rows x n x 4 B.
// Rows longer than 512 take the three-pass loop.
__global__ __launch_bounds__(256) void log_softmax_rows(float* __restrict__ x, long long rows, int n) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float* p = x + row * n;
    if (n <= 512) {
        float v[8];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = lane + 64 * j;
            v[j] = idx < n ? ldg1(p + idx) : -INFINITY;
            mx = fmaxf(mx, v[j]);
        }
        mx = wave_max(mx);
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) se += (lane + 64 * j) < n ? expf(v[j] - mx) : 0.f;
        const float lse = logf(wave_sum(se));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = lane + 64 * j;
            if (idx < n) stg1(p + idx, v[j] - mx - lse);
        }
        return;
    }
    float mx = -INFINITY;
    for (int v = lane; v < n; v += 64) mx = fmaxf(mx, p[v]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int v = lane; v < n; v += 64) s += expf(p[v] - mx);
    s = logf(wave_sum(s));
    for (int v = lane; v < n; v += 64) p[v] = p[v] - mx - s;
}
