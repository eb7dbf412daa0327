// Prefix beam search kernels (rnnt_prefix_beam_decode): WeNet's CTC-fused prefix beam search
// (wenet/transducer/search/prefix_beam_search.py:42-148) for a padded batch, two launches per encoder frame.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
// Rows are fixed: hypothesis i of utterance b is row b * beam + i of two buffer sets (token lists [rows][lcap], lengths, f64 scores,
// 64-bit running hashes as in beam_merge_stream_dev, context state and f64 context score (biased searches only), LSTM states
// [rows][2][512]: slot 0 = the hypothesis' state, slot 1 = the state after its last token went through the predictor).  prefix_step reads the current set and writes slot 1 and the row's
// top-k; prefix_merge reads the current set and writes the other one.  A hypothesis always holds its leading blank, so len >= 1.
#pragma once

constexpr int PB_MAX_BEAM = 16, PB_MAX_CAND = PB_MAX_BEAM * PB_MAX_BEAM, PB_NT = 256, PB_NONE = 0x7fffffff;

struct PrefixStepP {
    const float* whh; const float* egate; const float* wpr; const float* bpr; const float* wpf; const float* bpf;
    const float* wout; const float* bout;
    const float* encp;           // [B][T][256] joint.enc_ffn of the frames
    const float* ctc;            // [B][T][vocab] CTC log-probabilities, or nullptr (ctc_weight == 0: the term is 0.f)
    float* pool;                 // [rows][2][512] (h | c) of the current set
    const int* tk; const int* len;   // current set
    const int* nh;               // [B] hypotheses per utterance
    const int* lens;             // [B] frames per utterance
    float* top_lp; int* top_tok; // [rows][k]
    int vocab, k, beam, T, f, lcap;
    float tw, cw;
};

// One evaluation of beam_chain_row's arithmetic (same operands, same order) for one live hypothesis at frame f: LSTM cell on
// (embed[last token], slot 0) -> slot 1, predictor.projection, joint.pred_ffn + projected frame, tanh, vocabulary projection,
// log-softmax; then the shallow fusion log(tw * exp(lp) + cw * exp(ctc)) in f32 with separately rounded products and sum
// (prefix_beam_search.py:99-101) and the top-k over the WHOLE vocabulary, blank included (:104): value descending, lower index
// first on equal values.
//
// prefix_step_rows<G> is that evaluation for the cnt <= G hypotheses in rows r0 .. r0 + cnt - 1 (all of one utterance, all at frame
// row fr of encp / ctc) by one 512-thread workgroup: the four matrix-vector products read the weights ONCE for the G vectors
// (dec_matvec<G>: every vector's sum is formed in the same order whatever G is), the cell and the log-softmax / top-k are per
// hypothesis -- wave g does hypothesis g's.  Vectors beyond cnt repeat row r0's inputs and write nothing, so every barrier is
// reached by the whole workgroup.  Both the batch kernel (G = 1) and the pool kernel call it: the two cannot drift.
template <int G>
__device__ __forceinline__ void prefix_step_rows(const PrefixStepP& p, int r0, int cnt, long long fr) {
    constexpr int NTH = 512;
    __shared__ __attribute__((aligned(16))) float hs[G][RNNT_D], cs[G][RNNT_D], h2[G][RNNT_D], pr[G][RNNT_D], zs[G][RNNT_D];
    __shared__ __attribute__((aligned(16))) float gates[G][4 * RNNT_D];
    __shared__ float lg[G][512];
    const int tid = threadIdx.x;
    int tok[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int r = r0 + (g < cnt ? g : 0);
        tok[g] = ldgi(p.tk + (long long)r * p.lcap + ldgi(p.len + r) - 1);
    }
    const float* enc = p.encp + fr * RNNT_D;
    if (tid < RNNT_D) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float* pool = p.pool + (long long)(r0 + (g < cnt ? g : 0)) * 1024;
            hs[g][tid] = ldg1(pool + tid);
            cs[g][tid] = ldg1(pool + RNNT_D + tid);
        }
    }
    __syncthreads();
    dec_matvec<G, NTH>(p.whh, 4 * RNNT_D, hs, [&](int n, const float* acc) {                       // predictor.forward_step (predictor.py:185-210)
#pragma unroll
        for (int g = 0; g < G; ++g) gates[g][n] = acc[g] + ldg1(p.egate + (long long)tok[g] * (4 * RNNT_D) + n);
    });
    __syncthreads();
    if (tid < RNNT_D) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 gt = *reinterpret_cast<const float4*>(&gates[g][4 * tid]);
            const float cc = sigmoidf_(gt.y) * cs[g][tid] + sigmoidf_(gt.x) * tanhf(gt.z);
            const float hh = sigmoidf_(gt.w) * tanhf(cc);
            h2[g][tid] = hh;
            if (g < cnt) {
                float* pool = p.pool + (long long)(r0 + g) * 1024;
                stg1(pool + 512 + tid, hh);
                stg1(pool + 512 + RNNT_D + tid, cc);
            }
        }
    }
    __syncthreads();
    dec_matvec<G, NTH>(p.wpr, RNNT_D, h2, [&](int n, const float* acc) {                           // predictor.projection
#pragma unroll
        for (int g = 0; g < G; ++g) pr[g][n] = acc[g] + ldg1(p.bpr + n);
    });
    __syncthreads();
    dec_matvec<G, NTH>(p.wpf, RNNT_D, pr, [&](int n, const float* acc) {                           // joint (joint.py:54-66)
#pragma unroll
        for (int g = 0; g < G; ++g) zs[g][n] = tanhf(acc[g] + ldg1(p.bpf + n) + ldg1(enc + n));
    });
    __syncthreads();
    dec_matvec<G, NTH>(p.wout, p.vocab, zs, [&](int n, const float* acc) {
#pragma unroll
        for (int g = 0; g < G; ++g) lg[g][n] = acc[g] + ldg1(p.bout + n);
    });
    __syncthreads();
    const int w = tid >> 6, lane = tid & 63;
    if (w >= cnt) return;                                           // no barrier below; wave w: hypothesis w of the group
    const int r = r0 + w;
    const float* ctc = p.ctc ? p.ctc + fr * p.vocab : nullptr;
    float v[8];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = lane + 64 * j;
        v[j] = idx < p.vocab ? lg[w][idx] : -INFINITY;
        mx = fmaxf(mx, v[j]);
    }
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) se += (lane + 64 * j) < p.vocab ? expf(v[j] - mx) : 0.f;
    const float lse = logf(wave_sum(se));
    unsigned avail = 0;                                             // bit j: token lane + 64 j exists and is not chosen yet
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int idx = lane + 64 * j;
        if (idx < p.vocab) {
            const float lp = (v[j] - mx) - lse;
            const float c = ctc ? __fmul_rn(p.cw, expf(ldg1(ctc + idx))) : 0.f;
            v[j] = logf(__fadd_rn(__fmul_rn(p.tw, expf(lp)), c));
            avail |= 1u << j;
        }
    }
    for (int t = 0; t < p.k; ++t) {                                 // k <= vocab: a token is always left
        float bv = -INFINITY;
        int bi = PB_NONE;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (((avail >> j) & 1u) && (bi == PB_NONE || v[j] > bv)) { bv = v[j]; bi = lane + 64 * j; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != PB_NONE && (bi == PB_NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if ((bi & 63) == lane) avail &= ~(1u << (bi >> 6));         // remove the winner
        if (lane == 0) {
            p.top_lp[(long long)r * p.k + t] = bv;
            p.top_tok[(long long)r * p.k + t] = bi;
        }
    }
}

// the batch form: one workgroup per fixed row b * beam + i
__global__ __launch_bounds__(512) void prefix_step(PrefixStepP p) {
    const int r = blockIdx.x, b = r / p.beam, i = r - b * p.beam;
    if (i >= ldgi(p.nh + b) || p.f >= ldgi(p.lens + b)) return;    // whole workgroup: before the first barrier
    prefix_step_rows<1>(p, r, 1, (long long)b * p.T + p.f);
}

struct PrefixMergeP {
    const float* pool_in; float* pool_out;      // [rows][2][512]; pool_in == nullptr: no state gather (rnnt_prefix_merge_device)
    const int* tk_in; int* tk_out;              // [rows][lcap]
    const int* len_in; int* len_out;            // [rows]
    const double* sc_in; double* sc_out;        // [rows]
    const unsigned long long* hs_in; unsigned long long* hs_out;   // [rows]
    int* nh;                                    // [B] hypotheses per utterance (read, then rewritten)
    const int* lens;                            // [B] frames per utterance
    const float* top_lp; const int* top_tok;    // [rows][k]
    int* src_row; int* src_slot;                // [rows] where each survivor's state came from (hypothesis index, slot); both null: not wanted
    int lcap, k, beam, blank, f;
};
// hot-word biasing: the graph and, per row of either set, the context state and score.  The host launches the _ctx kernels
// (prefix_merge_rows<true>) when g.fail != nullptr and the plain ones otherwise, whose code and arguments are what they were.
struct PrefixCtxP {
    CpGraph g;
    const int* cst_in; int* cst_out;            // [rows] context state: the graph node of the hypothesis' token sequence
    const double* cs_in; double* cs_out;        // [rows] context score, kept beside the running score
};
// n-gram shallow fusion: the model and, per row of either set, the n-gram state and score.  The host launches the _ngram kernels
// (prefix_merge_rows<., true>) when the search fuses a model; the others neither take nor read this block.
struct PrefixNgP {
    NgTables g;
    const int* nst_in; int* nst_out;            // [rows] n-gram state: the model node of the token sequence, NG_START before the first token
    const double* ns_in; double* ns_out;        // [rows] n-gram score, kept beside the running score
};

// list form of wenet.utils.common.log_add for two values, as Python evaluates it: -inf if both are, else max + log(sum of exp)
__host__ __device__ inline double prefix_log_add(double a, double b) {
    if (a == -INFINITY && b == -INFINITY) return -INFINITY;
    const double m = a > b ? a : b;
    return m + log(exp(a - m) + exp(b - m));
}

// The host half of one frame of prefix_beam_search.py:105-145 for one utterance per workgroup:
//   candidates  c = j * k + t in the reference's order (per hypothesis j, per rank t): f64((f32)score_j + top_lp[j][t]); a blank
//               keeps row j's tokens and slot 0, any other token appends and takes slot 1
//   fusion      sequential in candidate order (:130-142): a candidate whose sequence equals an earlier survivor's is log-added
//               into it, the first one's tokens and state stay.  rep[c] = the first candidate with c's sequence (hash, then
//               length, then every token); every first candidate then adds its followers in ascending order
//   order       stable descending sort of the survivors: repeated block-wide argmax, ties to the lower candidate index
//   truncation  to `beam`; tokens, hashes and states gathered into rows row0 + a of the other set
// With a context graph (search.py:95-104,169-171,214-235 carried over): candidate c also takes its context state and score in its own
// thread -- a blank copies row j's, any other token is one cg_step from row j's state, its score added to row j's -- into two more
// LDS arrays (3 KB).  Both are functions of the token sequence alone, so fusion keeps the first candidate's.  The order is then by
// total = fused score + context score (ties to the lower candidate index as before) and the survivors' state and score are
// gathered with the rest.  The first prune (prefix_step) does not see the graph, as search.py:156 does not.  Without a graph
// (GRAPH = false: x is not read, the two arrays do not exist) the arithmetic is what it was: the key is the fused score itself.
// With an n-gram model (NG; the CTC search's rule, rnnt_ctc_prefix.hip.h, carried over): candidate c likewise takes its n-gram state and
// score in its own thread -- a blank copies row j's, any other token is one ng_step from row j's state (NG_START: the model's start
// state), its score added to row j's -- into two more LDS arrays (3 KB); fusion keeps the first candidate's; the order is by
// fused score + context score + n-gram score, left to right, a term whose feature is off left out.  NG = false: n is not read, the
// two arrays do not exist, the code is what it was.
// An utterance past its last frame (f >= lens[b]) is carried over unchanged.
// prefix_merge_rows: the merge of the utterance whose hypothesis count is nh[u] (and frame count lens[u], when lens is given) and
// whose rows start at row0 of either set; one workgroup.  Called by the batch kernel and by the pool kernel.
template <bool GRAPH, bool NG>
__device__ __forceinline__ void prefix_merge_rows(const PrefixMergeP& p, const PrefixCtxP& x, const PrefixNgP& n, int u, int row0) {
    __shared__ double sc[PB_MAX_CAND];
    __shared__ unsigned long long hsh[PB_MAX_CAND];
    __shared__ int clen[PB_MAX_CAND], ctok[PB_MAX_CAND], first[PB_MAX_CAND], rep[PB_MAX_CAND];
    __shared__ unsigned char taken[PB_MAX_CAND];
    __shared__ int h_len[PB_MAX_BEAM], acc[PB_MAX_BEAM];
    __shared__ double red_v[PB_NT / 64];
    __shared__ int red_i[PB_NT / 64];
    __shared__ int s_best;
    __shared__ double ccs[PB_MAX_CAND];
    __shared__ int ccst[PB_MAX_CAND];
    __shared__ double cns[PB_MAX_CAND];
    __shared__ int cnst[PB_MAX_CAND];
    const int tid = threadIdx.x;
    const int nh = p.nh[u];
    if (p.lens && p.f >= p.lens[u]) {                                // finished: carry the rows over unchanged
        for (int i = 0; i < nh; ++i) {
            const int r = row0 + i, len = p.len_in[r];
            for (int q = tid; q < len; q += PB_NT) p.tk_out[(long long)r * p.lcap + q] = p.tk_in[(long long)r * p.lcap + q];
            if (p.pool_in)
                for (int e = tid; e < 512; e += PB_NT) p.pool_out[(long long)r * 1024 + e] = p.pool_in[(long long)r * 1024 + e];
            if (tid == 0) {
                p.len_out[r] = len; p.sc_out[r] = p.sc_in[r]; p.hs_out[r] = p.hs_in[r];
                if constexpr (GRAPH) { x.cst_out[r] = x.cst_in[r]; x.cs_out[r] = x.cs_in[r]; }
                if constexpr (NG) { n.nst_out[r] = n.nst_in[r]; n.ns_out[r] = n.ns_in[r]; }
            }
        }
        return;
    }
    const int C = nh * p.k;                                          // <= 256 = PB_NT
    if (tid < nh) h_len[tid] = p.len_in[row0 + tid];
    if (tid < C) {
        const int j = tid / p.k, r = row0 + j;
        const int tok = p.top_tok[(long long)row0 * p.k + tid];
        const float s32 = (float)p.sc_in[r];                         // torch.tensor([s.score]): the running double rounded to f32
        sc[tid] = (double)__fadd_rn(s32, p.top_lp[(long long)row0 * p.k + tid]);   // f32 add (:105), widened by .item()
        const bool bl = tok == p.blank;
        ctok[tid] = tok;
        clen[tid] = p.len_in[r] + (bl ? 0 : 1);
        hsh[tid] = bl ? p.hs_in[r] : beam_hash_step(p.hs_in[r], tok);
        taken[tid] = 0;
        if constexpr (GRAPH) {                                       // copy_context / update_context; the fail chain diverges per lane, and is short
            int nx = x.cst_in[r];
            double cs = x.cs_in[r];
            if (!bl) cs += cg_step(x.g.fail, x.g.off, x.g.ctok, x.g.cid, x.g.tscore, x.g.nscore, x.g.oscore, nx, tok, &nx);
            ccst[tid] = nx;
            ccs[tid] = cs;
        }
        if constexpr (NG) {                                          // the back-off chain diverges per lane, and is at most the model's order long
            int nx = n.nst_in[r];
            double ns = n.ns_in[r];
            if (!bl) ns += ng_step(n.g, nx, tok, &nx);
            cnst[tid] = nx;
            cns[tid] = ns;
        }
    }
    __syncthreads();
    if (tid < C) {                                                   // first candidate with the same hash and length
        int m = tid;
        for (int c = 0; c < tid; ++c)
            if (hsh[c] == hsh[tid] && clen[c] == clen[tid]) { m = c; break; }
        first[tid] = m;
        rep[tid] = tid;
    }
    __syncthreads();
    auto tok_at = [&](int c, int q) {
        const int j = c / p.k;
        return q < h_len[j] ? p.tk_in[(long long)(row0 + j) * p.lcap + q] : ctok[c];
    };
    for (int c = 1; c < C; ++c) {                                    // uniform: everything the loop branches on is in LDS
        if (first[c] == c) continue;
        const int len = clen[c];
        for (int d = first[c]; d < c; ++d) {                         // equal hashes of different sequences never merge
            if (rep[d] != d || hsh[d] != hsh[c] || clen[d] != len) continue;
            int diff = 0;
            for (int q = tid; q < len; q += PB_NT) diff |= tok_at(c, q) != tok_at(d, q);
            if (!__syncthreads_or(diff)) {
                if (tid == 0) rep[c] = d;
                break;
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid < C && rep[tid] == tid) {                                // the followers' log_add, in candidate order
        double s = sc[tid];
        for (int c = tid + 1; c < C; ++c)
            if (rep[c] == tid) s = prefix_log_add(s, sc[c]);
        sc[tid] = s;
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    int n_acc = 0;
    while (n_acc < p.beam) {
        double bv = -INFINITY;
        int bi = PB_NONE;
        if (tid < C && rep[tid] == tid && !taken[tid]) {
            if constexpr (GRAPH) bv = sc[tid] + ccs[tid];
            else bv = sc[tid];
            if constexpr (NG) bv = bv + cns[tid];
            bi = tid;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != PB_NONE && (bi == PB_NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[w] = bv; red_i[w] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < PB_NT / 64; ++q)
                if (red_i[q] != PB_NONE && (bi == PB_NONE || red_v[q] > bv || (red_v[q] == bv && red_i[q] < bi))) { bv = red_v[q]; bi = red_i[q]; }
            s_best = bi;
            if (bi != PB_NONE) { taken[bi] = 1; acc[n_acc] = bi; }
        }
        __syncthreads();
        if (s_best == PB_NONE) break;                                // survivors exhausted
        ++n_acc;
    }
    for (int a = 0; a < n_acc; ++a) {
        const int c = acc[a], j = c / p.k, nr = row0 + a, len = clen[c], slot = ctok[c] == p.blank ? 0 : 1;
        for (int q = tid; q < len; q += PB_NT) p.tk_out[(long long)nr * p.lcap + q] = tok_at(c, q);
        if (p.pool_in) {
            const float* src = p.pool_in + ((long long)(row0 + j) * 2 + slot) * 512;
            float* dst = p.pool_out + (long long)nr * 1024;
            for (int e = tid; e < 512; e += PB_NT) dst[e] = src[e];
        }
        if (tid == 0) {
            p.len_out[nr] = len;
            p.sc_out[nr] = sc[c];
            p.hs_out[nr] = hsh[c];
            if constexpr (GRAPH) { x.cst_out[nr] = ccst[c]; x.cs_out[nr] = ccs[c]; }
            if constexpr (NG) { n.nst_out[nr] = cnst[c]; n.ns_out[nr] = cns[c]; }
            if (p.src_row) { p.src_row[nr] = j; p.src_slot[nr] = slot; }
        }
    }
    if (tid == 0) p.nh[u] = n_acc;
}

__global__ __launch_bounds__(PB_NT) void prefix_merge(PrefixMergeP p) { prefix_merge_rows<false, false>(p, PrefixCtxP{}, PrefixNgP{}, blockIdx.x, blockIdx.x * p.beam); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_ctx(PrefixMergeP p, PrefixCtxP x) { prefix_merge_rows<true, false>(p, x, PrefixNgP{}, blockIdx.x, blockIdx.x * p.beam); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_ngram(PrefixMergeP p, PrefixNgP n) { prefix_merge_rows<false, true>(p, PrefixCtxP{}, n, blockIdx.x, blockIdx.x * p.beam); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_ctx_ngram(PrefixMergeP p, PrefixCtxP x, PrefixNgP n) { prefix_merge_rows<true, true>(p, x, n, blockIdx.x, blockIdx.x * p.beam); }

// Start of a call: every utterance holds the one hypothesis [blank] with score 0 and the zero LSTM state (:68-77) in set 0.
__global__ __launch_bounds__(256) void prefix_init(float* pool, int* tk, int* len, double* sc, unsigned long long* hs, int* cst, double* cs, int* nst,
                                                   double* ns, int* nh, int beam, int lcap, int blank) {
    const int b = blockIdx.x, r = b * beam;
    for (int e = threadIdx.x; e < 512; e += 256) pool[(long long)r * 1024 + e] = 0.f;
    if (threadIdx.x == 0) {
        tk[(long long)r * lcap] = blank;
        len[r] = 1;
        sc[r] = 0.0;
        hs[r] = beam_hash_step(BEAM_HASH0, blank);
        cst[r] = 0;                                                  // the context root; the leading blank is never fed to the graph
        cs[r] = 0.0;
        nst[r] = NG_START;                                           // resolved by the first step under the model of the call; the blank is never fed to it
        ns[r] = 0.0;
        nh[b] = 1;
    }
}

// The n-gram part of a packed hypothesis: its running score, plus the end term (NG_START resolves to the start state) when the
// utterance has ended.
__device__ __forceinline__ double prefix_pack_ngram(const NgTables& g, int state, double score, bool fin) { return fin ? score + ng_eos(g, state) : score; }

// End of a call: the final set into ONE block for one download: scores f64 [rows] | context scores f64 [rows] | n-gram scores f64
// [rows] | n_hyp [B] | lengths [rows] | tokens [rows][lcap] | h [rows][256] | c [rows][256] (states only if with_states).  Rows
// without a hypothesis are zero.
// cst != nullptr: a biased search, whose returned score is the total; fin_nscore != nullptr: the utterance has ended and finalize
// (context_graph.py:264) REPLACES the context score (search.py:229-231), in the total too.  nst != nullptr: a search fused with the
// model ng; the utterance has ended, so the end term is added to the n-gram part and -- after the context part -- to the total.
__global__ __launch_bounds__(256) void prefix_pack(const float* pool, const int* tk, const int* len, const double* sc, const int* cst, const double* cs,
                                                   const double* fin_nscore, const int* nst, const double* ns, NgTables ng, const int* nh, int B, int beam,
                                                   int lcap, int with_states, double* out) {
    const int r = blockIdx.x, b = r / beam, i = r - b * beam, rows = B * beam, tid = threadIdx.x;
    int* oi = reinterpret_cast<int*>(out + 3 * rows);
    int* o_len = oi + B;
    int* o_tk = o_len + rows;
    float* o_h = reinterpret_cast<float*>(o_tk + (long long)rows * lcap);
    float* o_c = o_h + (long long)rows * RNNT_D;
    const bool live = i < nh[b];
    const int n = live ? len[r] : 0;
    for (int q = tid; q < lcap; q += 256) o_tk[(long long)r * lcap + q] = q < n ? tk[(long long)r * lcap + q] : 0;
    if (with_states) {
        o_h[(long long)r * RNNT_D + tid] = live ? pool[(long long)r * 1024 + tid] : 0.f;
        o_c[(long long)r * RNNT_D + tid] = live ? pool[(long long)r * 1024 + RNNT_D + tid] : 0.f;
    }
    if (tid == 0) {
        const double c = live && cst ? (fin_nscore ? -fin_nscore[cst[r]] : cs[r]) : 0.0;
        const double g = live && nst ? prefix_pack_ngram(ng, nst[r], ns[r], true) : 0.0;
        double tot = live ? (cst ? sc[r] + c : sc[r]) : 0.0;
        if (live && nst) tot = tot + g;
        out[r] = tot;
        out[rows + r] = c;
        out[2 * rows + r] = g;
        o_len[r] = n;
        if (i == 0) oi[b] = nh[b];
    }
}

// ------------------------------------------------------------------------------------------------
// Stream pool (rnnt_pool_prefix_frames / rnnt_pool_chunk_prefix): every slot keeps its search in HBM between calls, in FIXED rows --
// hypothesis i of slot b is row b * PB_MAX_BEAM + i (the stride is the largest beam, not the slot's) of two buffer sets (token
// lists [rows][lcap], lengths, f64 scores, hashes, states [rows][2][512]) plus nh[slot].  Slots advance independently, so which set
// is current is per slot: cur0[a] at the call's first frame for active row a (host bookkeeping, sent with the call's table),
// flipped once per frame.  A launch covers the ACTIVE slots only; idle slots are neither read nor written.  The frames of a call
// are compact: row a * t + f of encp / ctc is frame f of active row a.
// ------------------------------------------------------------------------------------------------
struct PrefixPoolP {
    const int* slots;            // [n] slot of active row a
    const int* cur0;             // [n] current buffer set of that slot at frame 0 of the call
    float* pool[2];
    int* tk[2]; int* len[2];
    double* sc[2];
    unsigned long long* hs[2];
    int* cst[2]; double* cs[2];  // context state and score per row (read and written by biased searches only)
    int* nst[2]; double* ns[2];  // n-gram state and score per row (read and written by searches that fuse a model only)
    int* nh;                     // [slots]
};
constexpr int PB_GROUP = 4;      // hypotheses of one slot per workgroup of the grouped prefix_step_pool: one pass over the weights for all of them

// prefix_step for the live hypotheses of the active slots at frame p.f of the call: workgroup -> (active row a, group of G rows); p
// carries the weights, the call's frames (T = frames per active row), top_lp / top_tok [all rows][k] and the scalars, the state
// pointers come from the slot's current set.  G = PB_GROUP: ~44 KB LDS, a quarter of the weight traffic; G = 1: the batch kernel's
// shape.  Both give the same bits (prefix_step_rows); the host picks by the size of the launch.
template <int G>
__global__ __launch_bounds__(512) void prefix_step_pool(PrefixStepP p, PrefixPoolP q, int groups) {
    const int a = blockIdx.x / groups, i0 = (blockIdx.x - a * groups) * G;
    const int slot = ldgi(q.slots + a), nh = ldgi(q.nh + slot);
    if (i0 >= nh) return;                                          // no hypothesis in this group: before the first barrier
    const int cur = (ldgi(q.cur0 + a) + p.f) & 1;
    p.pool = q.pool[cur]; p.tk = q.tk[cur]; p.len = q.len[cur];
    prefix_step_rows<G>(p, slot * PB_MAX_BEAM + i0, min(G, nh - i0), (long long)a * p.T + p.f);
}

// prefix_merge for one ACTIVE slot per workgroup: from the slot's current set into its other one.  p carries prefix_step_pool's
// outputs and the call's scalars (lens = nullptr: the slot has this frame); its buffer pointers are set here.  GRAPH: biased by g;
// NG: fused with the model ng.
template <bool GRAPH, bool NG>
__device__ __forceinline__ void prefix_merge_pool_rows(PrefixMergeP p, const PrefixPoolP& q, const CpGraph& g, const NgTables& ng) {
    const int a = blockIdx.x, slot = ldgi(q.slots + a);
    const int cur = (ldgi(q.cur0 + a) + p.f) & 1, nxt = cur ^ 1;
    p.pool_in = q.pool[cur]; p.pool_out = q.pool[nxt];
    p.tk_in = q.tk[cur]; p.tk_out = q.tk[nxt];
    p.len_in = q.len[cur]; p.len_out = q.len[nxt];
    p.sc_in = q.sc[cur]; p.sc_out = q.sc[nxt];
    p.hs_in = q.hs[cur]; p.hs_out = q.hs[nxt];
    p.nh = q.nh;
    PrefixCtxP x{};
    if constexpr (GRAPH) {
        x.g = g;
        x.cst_in = q.cst[cur]; x.cst_out = q.cst[nxt];
        x.cs_in = q.cs[cur]; x.cs_out = q.cs[nxt];
    }
    PrefixNgP n{};
    if constexpr (NG) {
        n.g = ng;
        n.nst_in = q.nst[cur]; n.nst_out = q.nst[nxt];
        n.ns_in = q.ns[cur]; n.ns_out = q.ns[nxt];
    }
    prefix_merge_rows<GRAPH, NG>(p, x, n, slot, slot * PB_MAX_BEAM);
}
__global__ __launch_bounds__(PB_NT) void prefix_merge_pool(PrefixMergeP p, PrefixPoolP q) { prefix_merge_pool_rows<false, false>(p, q, CpGraph{}, NgTables{}); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_pool_ctx(PrefixMergeP p, PrefixPoolP q, CpGraph g) { prefix_merge_pool_rows<true, false>(p, q, g, NgTables{}); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_pool_ngram(PrefixMergeP p, PrefixPoolP q, NgTables ng) { prefix_merge_pool_rows<false, true>(p, q, CpGraph{}, ng); }
__global__ __launch_bounds__(PB_NT) void prefix_merge_pool_ctx_ngram(PrefixMergeP p, PrefixPoolP q, CpGraph g, NgTables ng) { prefix_merge_pool_rows<true, true>(p, q, g, ng); }

// The reset of slots [slot0, slot0 + gridDim.x): prefix_init's start (hypothesis [blank], score 0, zero state) in set 0; the host's
// set index goes to 0 with it.  Touches no other slot.  prefix_slot_start: the same for one slot, by a workgroup of 256.
__device__ __forceinline__ void prefix_slot_start(const PrefixPoolP& q, int slot, int lcap, int blank) {
    const int r = slot * PB_MAX_BEAM;
    for (int e = threadIdx.x; e < 512; e += 256) q.pool[0][(long long)r * 1024 + e] = 0.f;
    if (threadIdx.x == 0) {
        q.tk[0][(long long)r * lcap] = blank;
        q.len[0][r] = 1;
        q.sc[0][r] = 0.0;
        q.hs[0][r] = beam_hash_step(BEAM_HASH0, blank);
        q.cst[0][r] = 0;
        q.cs[0][r] = 0.0;
        q.nst[0][r] = NG_START;
        q.ns[0][r] = 0.0;
        q.nh[slot] = 1;
    }
}
__global__ __launch_bounds__(256) void prefix_init_pool(PrefixPoolP q, int slot0, int lcap, int blank) { prefix_slot_start(q, slot0 + blockIdx.x, lcap, blank); }

// One slot's set `cur` into ONE block for one download (rnnt_stream_get_prefix), one workgroup per row i < beam: scores f64 [beam] |
// context scores f64 [beam] | n-gram scores f64 [beam] | n_hyp | lengths [beam] | tokens [beam][ocap] | h [beam][256] | c [beam][256]
// (states only if with_states).  Rows without a hypothesis are zero.  ocap >= every length (1 + the frames walked).  biased /
// fin_nscore: as prefix_pack's cst / fin_nscore.  fused: the search fuses a model, its n-gram scores are part of the totals;
// ng_final: with the end term under ng (the running score otherwise; ng is not read then).
__global__ __launch_bounds__(256) void prefix_pack_pool(PrefixPoolP q, int slot, int cur, int beam, int lcap, int ocap, int with_states, int biased,
                                                        const double* fin_nscore, int fused, int ng_final, NgTables ng, double* out) {
    const int i = blockIdx.x, r = slot * PB_MAX_BEAM + i, tid = threadIdx.x;
    int* oi = reinterpret_cast<int*>(out + 3 * beam);
    int* o_len = oi + 1;
    int* o_tk = o_len + beam;
    float* o_h = reinterpret_cast<float*>(o_tk + (long long)beam * ocap);
    float* o_c = o_h + (long long)beam * RNNT_D;
    const int nh = q.nh[slot];
    const bool live = i < nh;
    const int n = live ? min(q.len[cur][r], ocap) : 0;
    for (int e = tid; e < ocap; e += 256) o_tk[(long long)i * ocap + e] = e < n ? q.tk[cur][(long long)r * lcap + e] : 0;
    if (with_states) {
        o_h[(long long)i * RNNT_D + tid] = live ? q.pool[cur][(long long)r * 1024 + tid] : 0.f;
        o_c[(long long)i * RNNT_D + tid] = live ? q.pool[cur][(long long)r * 1024 + RNNT_D + tid] : 0.f;
    }
    if (tid == 0) {
        const double c = live && biased ? (fin_nscore ? -fin_nscore[q.cst[cur][r]] : q.cs[cur][r]) : 0.0;
        const double g = live && fused ? prefix_pack_ngram(ng, q.nst[cur][r], q.ns[cur][r], ng_final != 0) : 0.0;
        double tot = live ? (biased ? q.sc[cur][r] + c : q.sc[cur][r]) : 0.0;
        if (live && fused) tot = tot + g;
        out[i] = tot;
        out[beam + i] = c;
        out[2 * beam + i] = g;
        o_len[i] = n;
        if (i == 0) oi[0] = nh;
    }
}
