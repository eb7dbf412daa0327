// Greedy decoding: launched decision kernel (greedy_decide), the two resident decoders' parameter block (DecP), the resident per-stream
// decoder (greedy_stream), control helpers, the resident four-CUs-per-stream decoder (greedy_multi).  Host side: host_decode.hip.inc.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
#pragma once

// ------------------------------------------------------------------------------------------------
// greedy_decide: one thread per stream applies the argmax of the previous evaluation (packed key written by the
// EPI_ARGMAX epilogue of joint.ffn_out) to the per-stream RNN-T greedy state machine of
// _decode_chunk_streaming_logic (online_rnnt_model.py:193-220):
//   blank      -> next frame, symbol counter reset
//   non-blank  -> emit, token <- k, the candidate LSTM state becomes the committed one (sel ^= 1: the two
//                 state buffers swap roles, no copy); after n_steps symbols on one frame move to the next frame.
// key == 0 means "no evaluation pending" (idle stream, or already applied).
// ------------------------------------------------------------------------------------------------
struct GreedyState {
    int* tok;        // [B] predictor input token
    int* fidx;       // [B] current frame index (relative to frame-buffer start)
    int* nsym;       // [B] symbols emitted on the current frame
    int* count;      // [B] tokens emitted so far
    int* tokens;     // [B][max_tokens]
    int* sel;        // [B] which LSTM state buffer is committed
    unsigned long long* key;   // [B]
    int* misc;       // [0] streams with frames left (greedy_decide with count != 0), [1] beam rows active, [2] decodable frames
    int* host_backlog;   // host-mapped pinned int: max over streams of (decodable frames - current frame), written every call
};

__global__ __launch_bounds__(64) void greedy_decide(int B, int blank, int n_steps, int max_tokens, int do_count, GreedyState st) {
    const int n_frames = st.misc[2];
    int act = 0, behind = 0;
    for (int b = threadIdx.x; b < B; b += 64) {
        const unsigned long long k64 = st.key[b];
        int f = st.fidx[b];
        if (k64 != 0ull) {
            st.key[b] = 0ull;
            const int k = (int)(0xFFFFFFFFu - (unsigned)(k64 & 0xFFFFFFFFull));
            if (k == blank) {
                f += 1;
                st.fidx[b] = f;
                st.nsym[b] = 0;
            } else {
                const int cnt = st.count[b];
                if (cnt < max_tokens) st.tokens[(long long)b * max_tokens + cnt] = k;
                st.count[b] = cnt + 1;
                st.tok[b] = k;
                st.sel[b] ^= 1;
                const int ns = st.nsym[b] + 1;
                if (ns >= n_steps) {
                    st.nsym[b] = 0;
                    f += 1;
                    st.fidx[b] = f;
                } else {
                    st.nsym[b] = ns;
                }
            }
        }
        act += f < n_frames ? 1 : 0;
        behind = max(behind, n_frames - f);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) behind = max(behind, __shfl_xor(behind, o, 64));
    if (threadIdx.x == 0 && st.host_backlog) *st.host_backlog = behind;   // stale-tolerant feedback for the host's step budgets
    if (do_count) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) act += __shfl_xor(act, o, 64);
        if (threadIdx.x == 0) st.misc[0] = act;
    }
}

// ------------------------------------------------------------------------------------------------
// Resident greedy decoder (kernel greedy_stream below): the whole greedy decode of an utterance batch as ONE kernel.
// One workgroup owns one stream for the whole call and runs their RNN-T greedy state machine
// (_decode_chunk_streaming_logic, online_rnnt_model.py:193-220) without any exchange with other workgroups:
//   LSTM cell      gates = E[tok] + W_hh h      (predictor.py:200-204; gate rows interleaved i,f,g,o per unit)
//   joint          z = tanh(enc_proj[t] + W_c h' + b_c), W_c = W_pf W_pr folded (joint.py:54-66)
//   vocabulary     logits = W_out z + b_out, argmax (first index on ties, online_rnnt_model.py:212)
//   decision       blank -> next frame; else emit, commit (h', c'), <= n_steps symbols per frame.
// Streams are independent, so there is no lock step between workgroups: a "runaway" stream (n_steps symbols on many
// frames) only delays itself.  The lock-stepped launch-per-evaluation path needed 4 dependent kernels (~21 us, ~30 us
// when the encoder's grids fill the dispatcher) per evaluation of the SLOWEST stream; here an evaluation is ~1.7 MB of
// weight rows streamed from L2 by one CU plus ~0.4 MFLOP of VALU dot products.
// Matrix-vector layout: 16 lanes per weight row (16 x float4 = 256 contiguous bytes per load instruction and row,
// 4 loads cover K = 256), 16 rows per pass of the 256 threads, partial sums reduced with 4 in-row shuffles.
// Frames arrive while the kernel runs: the encoder stream publishes `frames_ready` after each chunk's joint.enc_ffn
// projection (kernel boundary = release); thread 0 polls it with relaxed agent-scope loads and, when it grows, issues
// ONE agent-scope acquire fence before anyone reads the new enc_proj rows.  Every wait is bounded (wall clock).
// ------------------------------------------------------------------------------------------------
struct DecP {
    const float* whh;     // [1024][256] gate-interleaved
    const float* egate;   // [vocab][1024] gate-interleaved input table
    const float* wjc;     // [256][256] folded pred_ffn o projection
    const float* bjc;     // [256]
    const float* wout;    // [vocab][256]
    const float* bout;    // [vocab]
    const float* encp;    // [B][fstride][256] projected encoder frames
    float* h;             // [2][bstride] state buffers (committed one selected by sel[b])
    float* c;
    int* sel;
    int* tok;
    int* fidx;
    int* nsym;
    int* count;
    int* tokens;          // [B][max_tokens]
    int* ctrl;            // [0] frames_ready (published by the encoder stream), [1] error flag, [2] evaluations (stats), [4] abort (greedy_multi)
    long long fstride_f;  // floats between streams in encp
    long long bstride;    // floats between the two state buffers
    int B, vocab, blank, n_steps, max_tokens, n_total;
    long long timeout_ticks;   // s_memrealtime ticks (100 MHz)
    const int* nlim;           // optional per-stream frame count (offline search over padded batches); null = n_total for all
    const int* slots;          // stream pool: workgroup i decodes stream slots[i] over its frames [0, n_total), B = active rows; null = stream i
};
constexpr int GREEDY_KF = 4;   // frames per vocabulary pass of both resident decoders (the one instantiation of each)

template <int SPW, int NTH, int U = 2, typename Epi>
__device__ __forceinline__ void dec_matvec(const float* __restrict__ W, int nrows, const float (*x)[RNNT_D], Epi epi) {
    const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
    float4 xv[SPW][4];
#pragma unroll
    for (int s = 0; s < SPW; ++s)
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[s][j] = *reinterpret_cast<const float4*>(&x[s][4 * l + 64 * j]);
    // U weight rows in flight per lane group: U x NTH/16 KB per CU
    constexpr int RP = NTH / 16;    // rows per pass of the workgroup
    for (int r0 = 0; r0 < nrows; r0 += RP * U) {
        float4 w[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = min(r0 + RP * u + g, nrows - 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[u][j] = ldg4(W + (long long)n * RNNT_D + 4 * l + 64 * j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = r0 + RP * u + g;
            float acc[SPW];
#pragma unroll
            for (int s = 0; s < SPW; ++s) {
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a = fmaf(w[u][j].x, xv[s][j].x, a);
                    a = fmaf(w[u][j].y, xv[s][j].y, a);
                    a = fmaf(w[u][j].z, xv[s][j].z, a);
                    a = fmaf(w[u][j].w, xv[s][j].w, a);
                }
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 16);
                acc[s] = a;
            }
            if (l == 0 && n < nrows) epi(n, acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// greedy_stream<KF>: resident greedy decoder, one workgroup (512 threads) per stream, exploiting two facts of the
// reference's loop (online_rnnt_model.py:193-220) that make most of its evaluations redundant:
//   (1) a blank leaves (token, h, c) unchanged, so the predictor output -- and with it W_c h' + b_c, the predictor half
//       of the joint -- only changes when a symbol is emitted: the LSTM (1 MB of W_hh) and the folded projection (256 KB)
//       are recomputed only then ("dirty");
//   (2) while the predictor half is fixed, frames t, t+1, ... are independent of each other: KF frames go through the
//       vocabulary projection in ONE pass over W_out (412 KB), and the decisions are scanned in order -- blanks advance
//       the frame, the first non-blank emits, commits (h', c') and ends the scan (later frames' logits are discarded).
// The results are those of the sequential loop (same operands and summation order per logit).  The dependent chain is
// (#symbols) x (L + Jc + O) + (#blank runs / KF) x O instead of (#symbols + #frames) x (L + Jc + O).
// ------------------------------------------------------------------------------------------------
template <int KF, int UL = 2, int UO = 2>
__global__ __launch_bounds__(512) void greedy_stream(DecP p) {
    constexpr int NTH = 512;
    __shared__ __attribute__((aligned(16))) float hs[1][RNNT_D], cs[RNNT_D], h2[1][RNNT_D], c2[RNNT_D], pp[RNNT_D];
    __shared__ __attribute__((aligned(16))) float zs[KF][RNNT_D];
    __shared__ __attribute__((aligned(16))) float gates[4 * RNNT_D];
    __shared__ float redv[NTH / 16][KF];
    __shared__ int redi[NTH / 16][KF];
    __shared__ int s_ctl[4];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= p.B) return;
    const int b = p.slots ? ldgi(p.slots + blockIdx.x) : (int)blockIdx.x;   // the stream whose state this workgroup owns
    {
        const long long off = (long long)(ldgi(p.sel + b) & 1) * p.bstride + (long long)b * RNNT_D;
        if (tid < RNNT_D) { hs[0][tid] = ldg1(p.h + off + tid); cs[tid] = ldg1(p.c + off + tid); }
    }
    int tok = ldgi(p.tok + b), fidx = p.slots ? 0 : ldgi(p.fidx + b), nsym = ldgi(p.nsym + b), count = ldgi(p.count + b);   // uniform
    const int n_total = p.nlim ? min(p.n_total, ldgi(p.nlim + b)) : p.n_total;
    int evals = 0, seen_ready = 0;
    bool dirty = true;
    const float* encp = p.encp + (long long)b * p.fstride_f;
    __syncthreads();
    while (fidx < n_total) {
        // ---- frames available to this stream (bounded wait) ------------------------------------------------------------
        if (tid == 0) {
            int nf = __hip_atomic_load(p.ctrl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
            int err = 0;
            while (nf <= fidx) {
                if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > p.timeout_ticks) {
                    __hip_atomic_store(p.ctrl + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    err = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(32);
                nf = __hip_atomic_load(p.ctrl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (nf > seen_ready) {   // ONE acquire per publication: nobody reads stale enc_proj lines
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                seen_ready = nf;
            }
            s_ctl[0] = err;
            s_ctl[1] = nf;
        }
        __syncthreads();
        if (s_ctl[0]) break;
        // frames evaluated together: right after a symbol only the current frame (more symbols are likely on it and the
        // single-frame pass is cheaper), otherwise up to KF
        const int kf = dirty ? 1 : min(KF, min(s_ctl[1], n_total) - fidx);
        if (dirty) {
            // ---- predictor step: gates = E[tok] + W_hh h; candidate (h', c'); pp = W_c h' + b_c ---------------------------
            dec_matvec<1, NTH, UL>(p.whh, 4 * RNNT_D, hs, [&](int n, const float* acc) {
                gates[n] = acc[0] + ldg1(p.egate + (long long)tok * (4 * RNNT_D) + n);
            });
            __syncthreads();
            if (tid < RNNT_D) {
                const float4 gt = *reinterpret_cast<const float4*>(&gates[4 * tid]);
                const float cc = sigmoidf_(gt.y) * cs[tid] + sigmoidf_(gt.x) * tanhf(gt.z);
                c2[tid] = cc;
                h2[0][tid] = sigmoidf_(gt.w) * tanhf(cc);
            }
            __syncthreads();
            dec_matvec<1, NTH, UL>(p.wjc, RNNT_D, h2, [&](int n, const float* acc) { pp[n] = acc[0] + ldg1(p.bjc + n); });
            dirty = false;
            __syncthreads();
        }
        // ---- joint activations of kf frames --------------------------------------------------------------------------------
        for (int e = tid; e < (kf == 1 ? 1 : KF) * RNNT_D; e += NTH) {
            const int k = e >> 8, n = e & 255;
            zs[k][n] = k < kf ? tanhf(pp[n] + ldg1(encp + (long long)(fidx + k) * RNNT_D + n)) : 0.f;
        }
        __syncthreads();
        // ---- vocabulary projection of the kf frames + per-frame argmax (first index on ties) ----------------------------------
        float bv[KF];
        int bi[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) { bv[k] = -INFINITY; bi[k] = 0x7fffffff; }
        if (KF > 1 && kf == 1) {
            dec_matvec<1, NTH, UL>(p.wout, p.vocab, zs, [&](int n, const float* acc) {
                const float v = acc[0] + ldg1(p.bout + n);
                if (v > bv[0]) { bv[0] = v; bi[0] = n; }
            });
        } else {
            dec_matvec<KF, NTH, UO>(p.wout, p.vocab, zs, [&](int n, const float* acc) {
                const float bo = ldg1(p.bout + n);
#pragma unroll
                for (int k = 0; k < KF; ++k) {
                    const float v = acc[k] + bo;
                    if (v > bv[k]) { bv[k] = v; bi[k] = n; }
                }
            });
        }
        if ((tid & 15) == 0) {
#pragma unroll
            for (int k = 0; k < KF; ++k) { redv[tid >> 4][k] = bv[k]; redi[tid >> 4][k] = bi[k]; }
        }
        __syncthreads();
        // ---- decisions, in frame order (every thread computes the same uniform result) -----------------------------------------
        {
            const int k = tid >> 6 < KF ? tid >> 6 : 0;     // wave k reduces frame k (waves >= KF idle)
            const int ln = tid & 63;
            float best = -INFINITY;
            int ix = 0x7fffffff;
            if (ln < NTH / 16) { best = redv[ln][k]; ix = redi[ln][k]; }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(ix, o, 64);
                if (ov > best || (ov == best && oi < ix)) { best = ov; ix = oi; }
            }
            __syncthreads();                                  // redi fully read before it is reused for the winners
            if (ln == 0 && (tid >> 6) < KF) redi[0][tid >> 6] = ix;
        }
        __syncthreads();
        bool commit = false;
        for (int k = 0; k < kf; ++k) {
            const int w = redi[0][k];
            if (w == p.blank) { fidx += 1; nsym = 0; continue; }
            if (tid == 0 && count < p.max_tokens) p.tokens[(long long)b * p.max_tokens + count] = w;
            count += 1;
            tok = w;
            nsym += 1;
            if (nsym >= p.n_steps) { nsym = 0; fidx += 1; }
            commit = true;
            break;
        }
        if (commit) {
            if (tid < RNNT_D) { hs[0][tid] = h2[0][tid]; cs[tid] = c2[tid]; }
            dirty = true;
        }
        ++evals;
        __syncthreads();
    }
    // ---- write the state back (buffer 0 becomes the committed one) ----------------------------------------------------
    if (tid < RNNT_D) {
        stg1(p.h + (long long)b * RNNT_D + tid, hs[0][tid]);
        stg1(p.c + (long long)b * RNNT_D + tid, cs[tid]);
    }
    if (tid == 0) {
        p.sel[b] = 0; p.tok[b] = tok; p.fidx[b] = p.slots ? 0 : fidx; p.nsym[b] = nsym; p.count[b] = count;   // pool: frames consumed
        atomicAdd(p.ctrl + 2, evals);
    }
}

// packed argmax keys (EPI_ARGMAX) -> int32 indices (CTC head)
__global__ void unpack_keys(const unsigned long long* __restrict__ key, int* __restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (int)(0xFFFFFFFFu - (unsigned)(key[i] & 0xFFFFFFFFull));
}

// frames_ready <- n (one thread; the kernel boundary before it released the encoder's writes)
__global__ void publish_frames(int* ctrl, int n) {
    __hip_atomic_store(ctrl, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Do kernels of two streams really run at the same time?  ctrl[1] <- 1 if ctrl[0] becomes non-zero within `ticks`
// (100 MHz) while this kernel is resident.  A profiler that serialises dispatches, or two streams folded onto one
// hardware queue, make it time out; the resident decoder is then not used.
__global__ void probe_overlap_wait(int* ctrl, long long ticks) {
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    int seen = 0;
    while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
        if (__hip_atomic_load(ctrl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { seen = 1; break; }
        __builtin_amdgcn_s_sleep(32);
    }
    ctrl[1] = seen;
}

// ------------------------------------------------------------------------------------------------
// greedy_multi<KF>: the resident greedy decoder with FOUR workgroups (CUs) per stream and the weights STATIONARY on chip.
// greedy_stream streams 1.7 MB of weight rows through one CU per symbol (~23 us at the per-CU L2 fetch rate, ~2x that next to
// the encoder), and the utterance batch ends with its slowest stream's dependent chain.  Here part p of stream b keeps for
// the whole call
//   W_hh rows of hidden units [64 p, 64 p + 64)  (256 gate rows x 256)      in registers (128 per thread)
//   W_c  columns              [64 p, 64 p + 64)  (256 rows x 64, the folded pred_ffn o projection)  in registers (32 per thread)
//   W_out rows                [ceil(V/4) p, ...) (103 x 256 for V = 412)                             in LDS
// and a symbol costs two exchanges among the four parts instead of a weight stream:
//   X1  h' slice (64) + the part's partial sums of W_c h' over its 64 columns (256)  ->  every part has h' and
//       pp = b_c + sum of the four partials (added in part order, so all four hold the same bits)
//   XA  per frame of the pass: the part's (max logit, argmax) over its vocabulary rows  ->  every part takes the same decision
// (a run of blank frames costs one XA only: as in greedy_stream the predictor is re-evaluated only after a symbol and up to KF
// frames share a pass).  The W_hh x h product of a predictor step is formed one step early, inside the XA exchange of the pass that
// made h (its h' then): the committed h of a step is always an earlier candidate, whole in LDS long before the decision that commits
// it, and only egate[tok] needs that decision -- so the product is off the symbol chain (g_next / have_g in the kernel).  Every exchanged 32-bit value travels as one 8-byte word (payload | tag << 32) written with one
// write-through store and polled with L1-bypassing loads: valid iff the tag matches the exchange's sequence number; buffers
// alternate by that number's parity (a part can only be one exchange ahead of the slowest of its group).  Same state machine and
// per-logit operand order as the reference loop (online_rnnt_model.py:193-220); h' and pp are summed in a different (fixed)
// order than greedy_stream's, i.e. equal to float32 rounding.  Needs 4 * B workgroups resident at once (B <= 64 on 256 CUs);
// every wait is wall-clock bounded and an abort word releases the whole grid.
// ------------------------------------------------------------------------------------------------

// Agent-scope relaxed accesses of the exchange: L1-bypassing loads and write-through stores, one 8-byte word per value.
__device__ __forceinline__ int ld_sc1i(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1i(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_tag(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_tag(unsigned long long* p, unsigned payload, unsigned tag) {
    __hip_atomic_store(p, ((unsigned long long)tag << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define GM_PARTS 4
#define GM_X1 320            // words per part: 64 h' + 256 pp partials
#define GM_WLD 260           // LDS row stride of the W_out slice (floats)
#define GM_DBG_W 32          // stamp words per stream: [12 c + k] phase k of non-dirty (c = 0) / dirty (c = 1) passes, [12 c + 10] passes, [23] wave 0's / [26] wave 7's early W_hh product, [24] count, [25] stream, [27] / [28] marks inside the cell + W_c and the X1 phases of dirty passes
struct DecMP : DecP {           // slots: stream group i (mailboxes i) decodes stream slots[i]
    unsigned long long* x1;      // [2][B][4][GM_X1]
    unsigned long long* xa;      // [2][B][4][2 * KF]
    int rows_per;                // ceil(vocab / 4): vocabulary rows of a part (<= 128), resident in LDS
    long long* dbg;              // optional [B][GM_DBG_W]: phase timers of part 0 of every stream group, 100 MHz ticks (RNNT_GM_DBG=1)
};

// spin until the word carries `tag`; false on abort / timeout (sets the error and abort words)
__device__ __forceinline__ bool gm_poll(const DecMP& p, const unsigned long long* src, unsigned tag, unsigned& out) {
    unsigned long long v = ld_tag(src);
    if ((unsigned)(v >> 32) == tag) { out = (unsigned)v; return true; }
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    int it = 0;
    while (true) {
        v = ld_tag(src);
        if ((unsigned)(v >> 32) == tag) { out = (unsigned)v; return true; }
        if ((++it & 63) == 0) {
            if (ld_sc1i(p.ctrl + 4) != 0) return false;
            if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > p.timeout_ticks) {
                st_sc1i(p.ctrl + 1, 2);
                st_sc1i(p.ctrl + 4, 1);
                return false;
            }
        }
    }
}

// gm_poll for the three foreign words of one gather thread: the three loads are in flight together and ONE loop spins over whichever
// words are still missing, so a wait costs the arrival plus one L2 round trip (three gm_polls in a row are three dependent round
// trips: no load of the second can pass the first one's spin loop).  Every word keeps what gm_poll gives it: the tag test, the abort
// word and the wall-clock bound that sets the error and abort words.  A valid word stays valid for the whole exchange (the writer can
// only be one exchange ahead, in the buffer of the other parity), so a word that has arrived is not read again.
__device__ __forceinline__ bool gm_poll3(const DecMP& p, const unsigned long long* s0, const unsigned long long* s1, const unsigned long long* s2,
                                         unsigned tag, unsigned& o0, unsigned& o1, unsigned& o2) {
    unsigned long long v0 = ld_tag(s0), v1 = ld_tag(s1), v2 = ld_tag(s2);
    bool m0 = (unsigned)(v0 >> 32) != tag, m1 = (unsigned)(v1 >> 32) != tag, m2 = (unsigned)(v2 >> 32) != tag;
    if (m0 || m1 || m2) {
        const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
        int it = 0;
        while (true) {
            if (m0) v0 = ld_tag(s0);
            if (m1) v1 = ld_tag(s1);
            if (m2) v2 = ld_tag(s2);
            m0 = (unsigned)(v0 >> 32) != tag; m1 = (unsigned)(v1 >> 32) != tag; m2 = (unsigned)(v2 >> 32) != tag;
            if (!(m0 || m1 || m2)) break;
            if ((++it & 63) == 0) {
                if (ld_sc1i(p.ctrl + 4) != 0) return false;
                if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > p.timeout_ticks) {
                    st_sc1i(p.ctrl + 1, 2);
                    st_sc1i(p.ctrl + 4, 1);
                    return false;
                }
            }
        }
    }
    o0 = (unsigned)v0; o1 = (unsigned)v1; o2 = (unsigned)v2;
    return true;
}

// 512 threads.  Where the 423 KB of a part's weights live: the W_out rows in LDS (107 KB for V = 412), the W_hh slice in
// registers (128 per thread: row tid / 2, half of K) and the W_c columns in registers too (32 per thread): nothing is streamed
// after the launch.  (GM_WHH_REGS=0 streams the W_hh slice from L2 per symbol instead, 4 us.)  (Keeping W_hh in registers was tried: as
// plain arrays or parked in AGPRs through inline asm, hipcc spills the 128 weights of a thread to scratch at load time, which is
// the same L2 stream with worse coalescing.)  So a symbol costs a quarter of greedy_stream's weight stream plus two exchanges,
// and a run of blank frames one exchange and 15 KB.
#ifndef GM_WHH_REGS
#define GM_WHH_REGS 1
#endif
template <int KF>
__global__ __launch_bounds__(512) void greedy_multi(DecMP p) {
    extern __shared__ __attribute__((aligned(16))) float gm_smem[];
    long long* tsh = reinterpret_cast<long long*>(gm_smem);   // [GM_DBG_W] phase stamps (touched only under RNNT_GM_DBG)
    float* Wo = gm_smem + 2 * GM_DBG_W;                   // [rows_per][GM_WLD]  this part's vocabulary rows of W_out
    float* hb = Wo + p.rows_per * GM_WLD;                 // [2][256] h ping-pong: the committed h in one half, the candidate h' in the other; a commit swaps the roles
    float* pp = hb + 2 * RNNT_D;                          // [256] W_c h' + b_c
    float* mypp = pp + RNNT_D;                            // [256] this part's partial
    float* zs = mypp + RNNT_D;                            // [KF][256]
    float* redv = zs + KF * RNNT_D;                       // [8 waves][KF]
    int* redi = reinterpret_cast<int*>(redv + 8 * KF);    // [8][KF]
    unsigned* xav = reinterpret_cast<unsigned*>(redi + 8 * KF);   // [4 parts][2 KF] gathered partials
    int* s_bad = reinterpret_cast<int*>(xav + GM_PARTS * 2 * KF);
    float* lpart = reinterpret_cast<float*>(s_bad + 4);      // [KF][4 quarters][128 rows] partial logits
    static_assert(KF == 4, "thread (frame, row) mapping of the logit finish assumes KF * 128 == 512");
    const int tid0 = threadIdx.x;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int bi = (slot >> 2) * 8 + xcd, pw = slot & 3;  // the four parts of a stream share blockIdx % 8 (one XCD: speed hint only)
    if (bi >= p.B) return;
    const int b = p.slots ? ldgi(p.slots + bi) : bi;      // the stream whose state this group owns (stream pool: a slot); mailboxes stay at bi
    // ---- resident weights ------------------------------------------------------------------------------------------------
    const int cell_unit = 64 * pw + (tid0 >> 3);          // threads 0, 8, ... own the 64 hidden units of this part
    const bool cell = (tid0 & 7) == 0;
    const int v0 = p.rows_per * pw;                        // first vocabulary row of this part
    float cc = 0.f, cc2 = 0.f;
#if !GM_WHH_REGS
    float* gates = zs;                                     // [256] gate pre-activations of this part (zs is free during the predictor step)
#endif
#if GM_WHH_REGS
    float whh_r[128];                                      // W_hh[256 pw + tid / 2][128 (tid & 1) .. +128)
    {
        const float* src = p.whh + (long long)(256 * pw + (tid0 >> 1)) * RNNT_D + 128 * (tid0 & 1);
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float4 v = ldg4(src + 4 * j);
            whh_r[4 * j] = v.x; whh_r[4 * j + 1] = v.y; whh_r[4 * j + 2] = v.z; whh_r[4 * j + 3] = v.w;
        }
    }
#endif
    // this part's columns of W_c: thread (row tid / 2, half of the 64 columns) holds 32 weights
    float4 wcv[8];
    {
        const float* wc = p.wjc + (long long)(tid0 >> 1) * RNNT_D + 64 * pw + 32 * (tid0 & 1);
#pragma unroll
        for (int u = 0; u < 8; ++u) wcv[u] = ldg4(wc + 4 * u);
    }
    {
    const int tid = tid0;
    for (int e = tid; e < p.rows_per * 64; e += 512) {
        const int r = e >> 6, c4 = (e & 63) * 4;
        const int vr = v0 + r;
        *reinterpret_cast<float4*>(&Wo[r * GM_WLD + c4]) = vr < p.vocab ? ldg4(p.wout + (long long)vr * RNNT_D + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- state ---------------------------------------------------------------------------------------------------------------
    const long long soff = (long long)(ldgi(p.sel + b) & 1) * p.bstride + (long long)b * RNNT_D;
    if (tid < RNNT_D) hb[tid] = ldg1(p.h + soff + tid);
    cc = cell ? ldg1(p.c + soff + cell_unit) : 0.f;
    cc2 = cc;
    if (tid == 0) *s_bad = 0;
    if (tid < GM_DBG_W) tsh[tid] = 0;
    }
    // The bias words a thread adds on every pass, fetched once: b_out of its row in the logit finish (and, for wave 0, of the row 64
    // further on, which it finishes too in a one-frame pass), b_c of its pp element in the X1 gather.
    const int rfin = tid0 & 127;
    const float bout_r = (rfin < p.rows_per && v0 + rfin < p.vocab) ? ldg1(p.bout + v0 + rfin) : 0.f;
    const float bout_h = (tid0 < 64 && tid0 + 64 < p.rows_per && v0 + tid0 + 64 < p.vocab) ? ldg1(p.bout + v0 + tid0 + 64) : 0.f;
    const float bjc_r = tid0 < RNNT_D ? ldg1(p.bjc + tid0) : 0.f;
    int tok = ldgi(p.tok + b), fidx = p.slots ? 0 : ldgi(p.fidx + b), nsym = ldgi(p.nsym + b), count = ldgi(p.count + b);
    const int n_total = p.nlim ? min(p.n_total, ldgi(p.nlim + b)) : p.n_total;
    const float* encp = p.encp + (long long)b * p.fstride_f;
    unsigned long long* x1b = p.x1 + (long long)bi * GM_PARTS * GM_X1;
    unsigned long long* xab = p.xa + (long long)bi * GM_PARTS * 2 * KF;
    const unsigned x1par = (unsigned)p.B * GM_PARTS * GM_X1, xapar = (unsigned)p.B * GM_PARTS * 2 * KF;   // words between the two parities (4 B <= CUs: small)
    unsigned ev1 = 1, ev3 = 0;   // ev1: sequence number of the X1 exchange of the next predictor step = 1 + commits so far
    int seen_ready = 0;
    bool dirty = true, bad = false;
#if GM_WHH_REGS
    // W_hh x candidate h', formed ahead of the pass that needs it (see the one-frame branch of the argmax exchange).  Loop state: both
    // outlive the decision loop's continue / break and every pass that leaves the candidate alone.
    float g_next = 0.f;
    bool have_g = false;
#endif
    // Phase stamps (RNNT_GM_DBG): thread 0 of part 0 adds the ticks since its last stamp to an LDS word with a no-return atomic, so a
    // stamp costs one clock read and holds no registers; dirty and non-dirty passes are kept apart.  The first thread of wave 7 times
    // its early W_hh product the same way (word 26, its otherwise idle `tl`): wave 0's own share is stamp 11 of the dirty passes.
    long long tl = (long long)__builtin_amdgcn_s_memrealtime();
    const bool tdbg = p.dbg != nullptr && pw == 0 && tid0 == 0;
    const bool tdbg7 = p.dbg != nullptr && pw == 0 && tid0 == 448;
#define GM_T(k) { if (tdbg) { const long long t_ = (long long)__builtin_amdgcn_s_memrealtime(); \
                              (void)__hip_atomic_fetch_add(tsh + (dirty ? 12 : 0) + (k), t_ - tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); tl = t_; } }
    // A mark inside a phase: the ticks since the last stamp into word W_, the phase's own stamp untouched (word 27: the cell, of
    // "cell + W_c"; word 28: the arrival of the X1 words, of "wait X1", whose rest is the pp sum, the tanh and the barrier).
#define GM_TM(W_) { if (tdbg) (void)__hip_atomic_fetch_add(tsh + (W_), (long long)__builtin_amdgcn_s_memrealtime() - tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#if GM_WHH_REGS
    // G_ = this thread's half row of W_hh x the h buffer H_, both lanes of a row holding the same bits afterwards (the sum commutes).
    // One body for the two places that form the product, so the operand order is the same in both.  (A macro: through a lambda that
    // captures whh_r hipcc keeps the 128 weights in scratch.)
#define GM_WHH_DOT(G_, H_) { \
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f; \
        _Pragma("unroll") \
        for (int j = 0; j < 32; ++j) { \
            const float4 hv = *reinterpret_cast<const float4*>(&(H_)[128 * kh + 4 * j]); \
            a0 = fmaf(whh_r[4 * j], hv.x, a0); \
            a1 = fmaf(whh_r[4 * j + 1], hv.y, a1); \
            a2 = fmaf(whh_r[4 * j + 2], hv.z, a2); \
            a3 = fmaf(whh_r[4 * j + 3], hv.w, a3); \
            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0); \
        } \
        G_ = (a0 + a1) + (a2 + a3); \
        G_ += __shfl_xor(G_, 1, 64); }
#endif
    __syncthreads();
#if GM_WHH_REGS
    // The first predictor step of a call has no earlier pass to form its product in: form it here from the loaded h, once, so the loop
    // holds the product in ONE place (with a second, conditional copy at the head of the predictor step hipcc spills the weights).
    { const int kh = tid0 & 1; GM_WHH_DOT(g_next, hb) have_g = true; }
#endif
    while (fidx < n_total) {
        // Every index below is derived from an OPAQUE copy of the thread id made inside the iteration: with plain loop-invariant
        // indices LLVM hoists a few hundred LDS / global address computations out of this loop and then spills them (and the
        // resident weights) to scratch.
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6, row2 = tid >> 1, kh = tid & 1;
#if !GM_WHH_REGS
        float* hs = hb + (ev1 & 1 ? 0 : RNNT_D);             // committed h: the half changes with every commit
#endif
        float* h2 = hb + (ev1 & 1 ? RNNT_D : 0);             // candidate h'
        // ---- frames available (bounded wait; the sequential schedule publishes everything before the launch) -----------------
        int avail = seen_ready;
        if (avail <= fidx) {
            if (tid == 0) {
                int nf = ld_sc1i(p.ctrl);
                const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
                int err = 0;
                while (nf <= fidx) {
                    if (ld_sc1i(p.ctrl + 4) != 0 || (long long)__builtin_amdgcn_s_memrealtime() - t0 > p.timeout_ticks) {
                        st_sc1i(p.ctrl + 1, 1);
                        st_sc1i(p.ctrl + 4, 1);
                        err = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(16);
                    nf = ld_sc1i(p.ctrl);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // one acquire per publication seen
                redi[0] = err ? -1 : nf;
            }
            __syncthreads();
            avail = redi[0];
            __syncthreads();
            if (avail < 0) { bad = true; break; }
            seen_ready = avail;
        }
        const int kf = dirty ? 1 : min(KF, min(avail, n_total) - fidx);
        // the encoder-projection rows of the pass are fetched now and used after the predictor step
        float er[KF * RNNT_D / 512];
#pragma unroll
        for (int i2 = 0; i2 < KF * RNNT_D / 512; ++i2) {
            const int e = tid + 512 * i2, k = e >> 8;
            er[i2] = k < kf ? ldg1(encp + (long long)(fidx + k) * RNNT_D + (e & 255)) : 0.f;
        }
        if (tdbg) (void)__hip_atomic_fetch_add(tsh + (dirty ? 12 : 0) + 10, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        GM_T(0)
        if (dirty) {
            // ---- predictor step on this part's 64 units (predictor.py:200-204), then X1 ---------------------------------------
            unsigned long long* xw = x1b + (ev1 & 1) * x1par;
            float gi = 0.f, gf = 0.f, gg = 0.f, go = 0.f;     // gate activations of this lane group's hidden unit
#if GM_WHH_REGS
            {
                const float eg = ldg1(p.egate + (long long)tok * (4 * RNNT_D) + 256 * pw + row2);
                // W_hh x hs is not formed here: hs is the candidate that the commit before this pass made the committed h, and its
                // product was formed inside an earlier pass's argmax exchange (the first pass of a call: in front of the loop).
                const float g = g_next;                      // both lanes of a row hold the same bits
                // The i, f, g, o rows of a hidden unit sit in lane pairs 0-1, 2-3, 4-5, 6-7 of one group of eight lanes, so the unit's
                // first lane takes them through DPP and no LDS round trip or barrier stands between the product and the cell:
                // f from lane ^ 2, o from the mirror lane 7, g from the mirror of the quad swap (lane 5).
                gi = g + eg;
                // Each lane pair applies its own gate's activation first (tanh on the g rows, lanes 4-5; the logistic on i, f, o), so
                // the cell below is left with one product-sum and one tanh instead of five transcendentals in a row on one lane of
                // eight.  Same functions of the same inputs: the same bits.  From here on gi .. go hold ACTIVATIONS.
                gi = (tid & 6) == 4 ? tanhf(gi) : sigmoidf_(gi);
                gf = xor_partner<2>(gi);
                go = xor_partner<4>(gi);
                gg = xor_partner<4>(gf);
            }
#else
            {
                const float* eg = p.egate + (long long)tok * (4 * RNNT_D) + 256 * pw;
                dec_matvec<1, 512, 4>(p.whh + (long long)(256 * pw) * RNNT_D, RNNT_D, reinterpret_cast<const float (*)[RNNT_D]>(hs),
                                      [&](int n, const float* acc) { gates[n] = acc[0] + ldg1(eg + n); });
            }
            __syncthreads();
            if (cell) {
                const float4 gt = *reinterpret_cast<const float4*>(&gates[4 * (tid >> 3)]);     // i, f, g, o of this unit
                gi = sigmoidf_(gt.x); gf = sigmoidf_(gt.y); gg = tanhf(gt.z); go = sigmoidf_(gt.w);   // activations, as in the register form
            }
#endif
            GM_T(1)
#if GM_WHH_REGS
            have_g = false;                                   // the cell phase below writes a new candidate
#endif
            if (cell) {
                const int unit = 64 * pw + (tid >> 3);
                cc2 = gf * cc + gi * gg;                      // the same expression over the same values: contracts to the same fused operations
                const float hn = go * tanhf(cc2);
                h2[unit] = hn;
                st_tag(xw + pw * GM_X1 + (unit - 64 * pw), __float_as_uint(hn), ev1);
            }
            GM_TM(27)
            __syncthreads();
            {
                float q0 = 0.f, q1 = 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float4 hv = *reinterpret_cast<const float4*>(&h2[64 * pw + 32 * kh + 4 * u]);   // two addresses per wave: broadcast
                    q0 = fmaf(wcv[u].x, hv.x, q0);
                    q1 = fmaf(wcv[u].y, hv.y, q1);
                    q0 = fmaf(wcv[u].z, hv.z, q0);
                    q1 = fmaf(wcv[u].w, hv.w, q1);
                }
                float part = q0 + q1;
                part += __shfl_xor(part, 1, 64);
                if (!kh) {
                    mypp[row2] = part;
                    st_tag(xw + pw * GM_X1 + 64 + row2, __float_as_uint(part), ev1);
                }
            }
            __syncthreads();
            GM_T(2)
            // gather: threads 0..255 sum the four partials of pp[n] in part order, the three foreign ones polled together (gm_poll3);
            // threads 256..447 fetch the other parts' h'
            if (tid < RNNT_D) {
                const int q0 = pw == 0 ? 1 : 0, q1 = pw <= 1 ? 2 : 1, q2 = pw <= 2 ? 3 : 2;      // the other parts, ascending
                const unsigned long long* src = xw + 64 + tid;
                unsigned w0 = 0, w1 = 0, w2 = 0;
                if (!gm_poll3(p, src + q0 * GM_X1, src + q1 * GM_X1, src + q2 * GM_X1, ev1, w0, w1, w2)) bad = true;
                GM_TM(28)
                const float mine = mypp[tid], o0 = __uint_as_float(w0), o1 = __uint_as_float(w1), o2 = __uint_as_float(w2);
                const float v1 = pw == 0 ? o0 : (pw == 1 ? mine : o1), v2 = pw <= 1 ? o1 : (pw == 2 ? mine : o2);
                const float ppv = ((((pw == 0 ? mine : o0) + v1) + v2) + (pw == 3 ? mine : o2)) + bjc_r;
                pp[tid] = ppv;
                zs[tid] = tanhf(ppv + er[0]);                 // the one frame of this pass: its joint activations, formed by the thread that holds pp[n]
            } else if (tid < RNNT_D + 192) {
                const int idx = tid - RNNT_D;
                int q = idx >> 6;
                if (q >= pw) ++q;                              // the idx/64-th OTHER part
                unsigned w = 0;
                if (!gm_poll(p, xw + q * GM_X1 + (idx & 63), ev1, w)) bad = true;
                h2[64 * q + (idx & 63)] = __uint_as_float(w);
            }
            if (bad) *s_bad = 1;
            __syncthreads();
            if (*s_bad) { bad = true; break; }
            GM_T(3)
        }
        // ---- joint activations of kf frames (every part computes all 256).  A predictor pass has one frame and formed them in the X1
        // gather above, behind that phase's barrier: no second barrier and no trip of pp through LDS on the symbol chain. ---------------
        if (!dirty) {
#pragma unroll
            for (int i2 = 0; i2 < KF * RNNT_D / 512; ++i2) {
                const int e = tid + 512 * i2, k = e >> 8;
                zs[e] = k < kf ? tanhf(pp[e & 255] + er[i2]) : 0.f;
            }
            __syncthreads();
        }
        GM_T(4)
        // ---- logits of this part's vocabulary rows.  Thread (row = tid & 127, quarter of K = tid >> 7): a wave reads 64 consecutive
        // rows at one quarter, so the 16 lanes of a ds_read_b128 cycle hit 16 distinct slots (row stride 260 floats) and z is a
        // broadcast; the four quarter sums meet in LDS, then thread (frame, row) finishes the logit and the argmax runs per frame.
        {
            const int r = tid & 127, qk = tid >> 7;
            if (r < p.rows_per) {
                const float* wl = &Wo[r * GM_WLD + 64 * qk];
#pragma unroll
                for (int k = 0; k < KF; ++k) {
                    if (k < kf) {   // one frame at a time: with the frames innermost hipcc SLP-packs across frames and spills ~90 registers
                        const float* zk = &zs[k * RNNT_D + 64 * qk];
                        float a0 = 0.f, a1 = 0.f;
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const float4 w = *reinterpret_cast<const float4*>(wl + 4 * j);
                            const float4 z = *reinterpret_cast<const float4*>(zk + 4 * j);
                            a0 = fmaf(w.x, z.x, a0);
                            a1 = fmaf(w.y, z.y, a1);
                            a0 = fmaf(w.z, z.z, a0);
                            a1 = fmaf(w.w, z.w, a1);
                            if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                        }
                        lpart[(k * 4 + qk) * 128 + r] = a0 + a1;
                    }
                }
            }
        }
        __syncthreads();
        GM_T(5)
        ++ev3;
        unsigned long long* xq = xab + (ev3 & 1) * xapar;
        // ascending butterfly; DPP partners for 1..8 (xor_partner: the (value, index) pair is uniform in quads / 8-groups by then)
#define GM_STEP(O_) { const float ov = xor_partner<O_>(v); const int oi = __builtin_bit_cast(int, xor_partner<O_>(__builtin_bit_cast(float, ix))); \
                      if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; } }
        if (kf == 1) {
            // One frame (every pass after a symbol): wave 0 alone finishes the part's rows, lane l rows l and l + 64, compares the two in
            // registers, runs one butterfly and stores the XA words itself -- no second barrier and no trip through redv / redi.  The
            // order (larger value, then smaller index) is total, so the winner is the one the two-wave merge below would name.
            if (wave == 0) {
                float v = -INFINITY;
                int ix = 0x7fffffff;
                if (lane < p.rows_per && v0 + lane < p.vocab) {
                    v = ((lpart[lane] + lpart[128 + lane]) + (lpart[2 * 128 + lane] + lpart[3 * 128 + lane])) + bout_r;
                    ix = v0 + lane;
                }
                if (lane + 64 < p.rows_per && v0 + lane + 64 < p.vocab) {
                    const float ov = ((lpart[64 + lane] + lpart[128 + 64 + lane]) + (lpart[2 * 128 + 64 + lane] + lpart[3 * 128 + 64 + lane])) + bout_h;
                    const int oi = v0 + lane + 64;
                    if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
                }
                // Only the stores below need the winner, so the rows of 16 lanes meet by DPP row broadcasts instead of two LDS permutes:
                // lane 15 / 47 into rows 1 / 3, then lane 31 into rows 2 and 3; lane 63 holds the wave's best and is read back uniformly.
#define GM_BCAST(C_, M_) { const float ov = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), C_, M_, 0xF, false)); \
                           const int oi = __builtin_amdgcn_update_dpp(ix, ix, C_, M_, 0xF, false); \
                           if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; } }
                GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8) GM_BCAST(0x142, 0xA) GM_BCAST(0x143, 0xC)
#undef GM_BCAST
                v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
                ix = __builtin_amdgcn_readlane(ix, 63);
                GM_T(6)
                if (lane < KF) {                              // frames 1 .. KF - 1 of the pass carry "no row", as in the general form
                    unsigned u = 0u;
                    if (lane != 0) ix = 0x7fffffff;
                    if (ix != 0x7fffffff) {
                        u = __float_as_uint(v);
                        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // order-preserving; > 0 for every real value
                    }
                    st_tag(xq + pw * 2 * KF + 2 * lane, u, ev3);
                    st_tag(xq + pw * 2 * KF + 2 * lane + 1, (unsigned)ix, ev3);
                    xav[pw * 2 * KF + 2 * lane] = u;
                    xav[pw * 2 * KF + 2 * lane + 1] = (unsigned)ix;
                }
                GM_T(7)
            }
#if GM_WHH_REGS
            // ---- the NEXT predictor step's W_hh x h', in the window of this exchange.  The committed h of a predictor step is always
            // the candidate of the pass that emitted the symbol or of an earlier one, and the candidate has been whole in LDS since the
            // barrier that closed its X1 gather; only egate[tok] waits for a decision.  From the quarter-sum barrier above to the
            // exchange barrier below wave 0 alone finishes the rows, takes the argmax and stores the XA words, 24 threads of wave 1 poll
            // and the LDS pipe idles (>= 1.3 us against the product's 0.9), so waves 1-7 form the product at once, wave 1's pollers
            // before they poll (the other parts' words are at least as far away), wave 0 behind its stores.  Same loop, same operand
            // order, same bits as the product in place.  Hazards:
            //   * h2 is read here strictly between those two barriers.  The next writer of EITHER h buffer is the cell phase of a later
            //     predictor pass, behind this pass's exchange barrier; the last writer of h2 was this or an earlier predictor pass's X1
            //     gather, in front of the quarter-sum barrier.
            //   * A candidate is committed by whichever later pass emits the next symbol, so g_next is used exactly once per candidate
            //     (the last candidate of a call is formed for nothing).  After a commit the buffer roles swap and g_next belongs to what
            //     is now hs; without one the candidate stays and so does g_next: a non-predictor pass neither forms nor reads it (a
            //     one-frame pass of that kind finds have_g set).  The n_steps cap commits like any symbol.
            //   * The exchange is untouched: same words, tags, parity, bounded waits and abort word, and no barrier is added.
            //   * have_g is uniform over the workgroup: cleared by the cell phase, set here in the same pass (a predictor pass has one
            //     frame), so every predictor step finds its product ready; the first one of a call takes the one formed before the loop.
            if (!have_g) {
                if (tdbg7) tl = (long long)__builtin_amdgcn_s_memrealtime();
                GM_WHH_DOT(g_next, h2)
                have_g = true;
                if (tdbg7) (void)__hip_atomic_fetch_add(tsh + 26, (long long)__builtin_amdgcn_s_memrealtime() - tl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                GM_T(11)
            }
#endif
        } else {
            {
                const int k = tid >> 7, r = tid & 127;         // KF * 128 = 512 threads
                const bool vin = k < kf && r < p.rows_per && v0 + r < p.vocab;
                float v = -INFINITY;
                int ix = 0x7fffffff;
                if (vin) {
                    v = ((lpart[(k * 4) * 128 + r] + lpart[(k * 4 + 1) * 128 + r]) + (lpart[(k * 4 + 2) * 128 + r] + lpart[(k * 4 + 3) * 128 + r])) + bout_r;
                    ix = v0 + r;
                }
                GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8) GM_STEP(16) GM_STEP(32)
                if (lane == 0) { redv[wave] = v; redi[wave] = ix; }   // wave 2 k, 2 k + 1 = frame k
            }
            __syncthreads();
            GM_T(6)
            if (tid < KF) {
                float v = redv[2 * tid];
                int ix = redi[2 * tid];
                {
                    const float ov = redv[2 * tid + 1];
                    const int oi = redi[2 * tid + 1];
                    if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; }
                }
                unsigned u = 0u;
                if (ix != 0x7fffffff) {
                    u = __float_as_uint(v);
                    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // order-preserving; > 0 for every real value
                }
                st_tag(xq + pw * 2 * KF + 2 * tid, u, ev3);
                st_tag(xq + pw * 2 * KF + 2 * tid + 1, (unsigned)ix, ev3);
                xav[pw * 2 * KF + 2 * tid] = u;
                xav[pw * 2 * KF + 2 * tid + 1] = (unsigned)ix;
            }
            GM_T(7)
        }
#undef GM_STEP
        if (tid >= 64 && tid < 64 + (GM_PARTS - 1) * 2 * KF) {
            const int idx = tid - 64;
            int q = idx / (2 * KF);
            const int w = idx - q * 2 * KF;
            if (q >= pw) ++q;
            unsigned val = 0;
            if (!gm_poll(p, xq + q * 2 * KF + w, ev3, val)) *s_bad = 1;
            xav[q * 2 * KF + w] = val;
        }
        __syncthreads();
        GM_T(8)
        if (*s_bad) { bad = true; break; }
        // ---- decisions, in frame order (identical in every thread of every part) ---------------------------------------------------
        bool commit = false;
        for (int k = 0; k < kf; ++k) {
            unsigned bv = 0u;
            int w = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < GM_PARTS; ++q) {
                const unsigned v = xav[q * 2 * KF + 2 * k];
                const int ix = (int)xav[q * 2 * KF + 2 * k + 1];
                if (v > bv || (v == bv && ix < w)) { bv = v; w = ix; }
            }
            if (w == p.blank) { fidx += 1; nsym = 0; continue; }
            if (pw == 0 && tid == 0 && count < p.max_tokens) p.tokens[(long long)b * p.max_tokens + count] = w;
            count += 1;
            tok = w;
            nsym += 1;
            if (nsym >= p.n_steps) { nsym = 0; fidx += 1; }
            commit = true;
            break;
        }
        // No barrier closes the pass.  xav, redv / redi, lpart, zs and s_bad are next written behind at least one barrier of the next
        // pass (the tanh barrier; redi[0] of the frame wait is read before the exchange barrier above), and a commit copies nothing: the
        // candidate buffer becomes the committed one.  The buffer that turns candidate was last read by the W_hh product of an earlier
        // pass and is next written by the cell phase, so the predictor step of the next pass may start in a wave as soon as it is here.
        if (commit) {
            ++ev1;
            cc = cc2;
        }
        GM_T(9)
        dirty = commit;                                      // the predictor step runs again only after a symbol
    }
    if (tdbg) {
        tsh[24] = count; tsh[25] = b;
        long long* out = p.dbg + (long long)((blockIdx.x >> 5) * 8 + (blockIdx.x & 7)) * GM_DBG_W;   // row bi
        for (int k = 0; k < GM_DBG_W; ++k) out[k] = tsh[k];
    }
#undef GM_T
#if GM_WHH_REGS
#undef GM_WHH_DOT
#endif
    // ---- canonical state for the host / the next call (buffer 0 becomes the committed one) ---------------------------------
    if (pw == 0 && tid0 < RNNT_D) stg1(p.h + (long long)b * RNNT_D + tid0, hb[(ev1 & 1 ? 0 : RNNT_D) + tid0]);
    if (cell) stg1(p.c + (long long)b * RNNT_D + cell_unit, cc);
    if (pw == 0 && tid0 == 0) {
        p.sel[b] = 0; p.tok[b] = tok; p.fidx[b] = p.slots ? 0 : fidx; p.nsym[b] = nsym; p.count[b] = count;   // pool: frames consumed
        atomicAdd(p.ctrl + 2, (int)ev3);                   // passes = XA exchanges
    }
    (void)bad;
}
