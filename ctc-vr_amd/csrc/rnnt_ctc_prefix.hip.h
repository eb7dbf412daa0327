// CTC prefix beam search with contextual biasing (rnnt_ctc_prefix_beam_logprobs / _decode): WeNet's ctc_prefix_beam_search
// (wenet/transformer/search.py:125-247) with its ContextGraph (wenet/utils/context_graph.py), ONE launch per call.
// Part of rnnt_kernels.hip.h (include that umbrella, not this file).
//
// One workgroup of 256 threads per utterance walks that utterance's frames with block barriers only.  State of the frame loop:
//   hypotheses   <= 16, in LDS: the four f64 scores (s, ns, v_s, v_ns), score() and viterbi_score(), context node and f64 context
//                score, and handles into two arenas in device memory that the loop only ever WRITES (the packer reads them):
//   prefix arena node 0 = the empty prefix, node 1 + t * beam + a = (parent node, token) created by survivor a of frame t.  "P + u is
//                the live hypothesis P'" is P'.token == u && P'.parent == P.node almost always, with no token compare.  Not always:
//                P can be pruned and come back under a new node while P + u stays live.  So a parent test that fails on the node ids
//                goes on to the 64-bit running hashes (beam_hash_step) and, when those agree, to an exact comparison: both chains are
//                walked towards the root until they meet.  That walk reads the arena, and happens only in the case above.
//   time arena   node t * beam + a = (parent node, frame); times_s / times_ns are node ids (-1 = the empty list) and lengths.
//                `list.copy()` shares the node, `append(t)` and `[-1] = t` are one new node each, and an entry of a frame changes
//                its times_ns to at most one new list, so survivor a of frame t owns exactly one slot of either arena.
// Per frame, four barriers:
//   top          the row's <= 512 f32 values as 64-bit keys (order-preserving value bits | ~index: value descending, lower index
//                first), two per thread, prefetched one frame ahead; every wave takes its own top-beam by repeated wave max, then
//                64 threads rank the 4 * beam wave winners by counting
//   entries      thread j < n_hyp forms the next-frame entry "P_j unchanged" by running ITS contributions in the reference's order
//                (outer loop over the top tokens, inner over the hypotheses): blank, repeat of the last token, and the extension
//                P_i + u == P_j of its live parent; thread i * beam + r forms the entry "P_i + top[r]" unless it is a live
//                hypothesis.  Entries stay in registers; only total score and first-insertion key go to LDS
//   prune        every entry counts the entries that precede it (greater total, or equal total and lower key): the stable
//                descending sort of search.py:220-223 without a loop of block arg-max steps; rank < beam survives and writes row rank
// The epilogue zero-fills the utterance's output rows, replaces the context score by finalize's -node_score, and walks both arenas.
#pragma once

constexpr int CP_NT = 256, CP_MAX_BEAM = 16, CP_SLOTS = CP_MAX_BEAM + CP_MAX_BEAM * CP_MAX_BEAM, CP_NOKEY = 0x7fffffff;
constexpr int CP_MAX_NODES = 4096;

struct CtcPrefixP {
    const float* lp;             // [B][T][V] log-probabilities
    const int* lens;             // [B]
    int T, V, blank, beam, lcap;
    // context graph (g_fail == nullptr: none): flat node arrays, children as a CSR of (token, child) sorted by token per node
    const int* g_fail; const int* g_off; const int* g_ctok; const int* g_cid;
    const double* g_tscore; const double* g_nscore; const double* g_oscore;
    int2* parena; int2* tarena;  // [B][T * beam + 1] each
    int* o_nh; int* o_len; int* o_tok; int* o_time; double* o_sc; double* o_cs;   // [B], [B][beam], [B][beam][lcap] x 2, [B][beam] x 2
};

// f32 value and index -> a key whose unsigned order is "value descending, then index ascending" read from the top; -0 counts as +0
__host__ __device__ inline unsigned long long cp_key(float v, int idx) {
    v += 0.f;
    unsigned b;
    memcpy(&b, &v, 4);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    return ((unsigned long long)b << 32) | (0xffffffffu - (unsigned)idx);
}
__host__ __device__ inline float cp_key_value(unsigned long long k) {
    unsigned b = (unsigned)(k >> 32);
    b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
    float v;
    memcpy(&v, &b, 4);
    return v;
}
__host__ __device__ inline int cp_key_index(unsigned long long k) { return (int)(0xffffffffu - (unsigned)k); }

// the child of `node` over `tok`, or -1: binary search in the node's sorted CSR row
__host__ __device__ inline int cg_child(const int* off, const int* ctok, const int* cid, int node, int tok) {
    int lo = off[node], hi = off[node + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, v = ctok[mid];
        if (v == tok) return cid[mid];
        if (v < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// ContextGraph.forward_one_step (context_graph.py:212-247) on the flat tables: returns the step's score, *next = the node it lands in
__host__ __device__ inline double cg_step(const int* fail, const int* off, const int* ctok, const int* cid, const double* tscore,
                                          const double* nscore, const double* oscore, int state, int tok, int* next) {
    int node = cg_child(off, ctok, cid, state, tok);
    double score;
    if (node >= 0) score = tscore[node];
    else {
        node = fail[state];
        while (cg_child(off, ctok, cid, node, tok) < 0) {
            node = fail[node];
            if (node == 0) break;                                    // root
        }
        const int c = cg_child(off, ctok, cid, node, tok);
        if (c >= 0) node = c;
        score = nscore[node] - nscore[state];                        // the score of the fail path
    }
    *next = node;
    return score + oscore[node];
}

__device__ inline unsigned long long cp_wave_max(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}

__global__ __launch_bounds__(CP_NT) void ctc_prefix_search(CtcPrefixP p) {
    __shared__ unsigned long long wtop[CP_NT / 64][CP_MAX_BEAM];
    __shared__ int top_tok[CP_MAX_BEAM];
    __shared__ double top_p[CP_MAX_BEAM];
    __shared__ double h_s[CP_MAX_BEAM], h_ns[CP_MAX_BEAM], h_vs[CP_MAX_BEAM], h_vns[CP_MAX_BEAM], h_cs[CP_MAX_BEAM], h_score[CP_MAX_BEAM],
        h_vit[CP_MAX_BEAM];
    __shared__ unsigned long long h_hash[CP_MAX_BEAM], h_phash[CP_MAX_BEAM];      // running hash of the prefix, and of the prefix less its last token
    __shared__ int h_cst[CP_MAX_BEAM], h_node[CP_MAX_BEAM], h_pnode[CP_MAX_BEAM], h_last[CP_MAX_BEAM], h_plen[CP_MAX_BEAM];
    __shared__ int h_tns[CP_MAX_BEAM], h_tls[CP_MAX_BEAM];                        // times_s: node, length
    __shared__ int h_tnn[CP_MAX_BEAM], h_tnp[CP_MAX_BEAM], h_tln[CP_MAX_BEAM];    // times_ns: node, its parent, length
    __shared__ int h_tn[CP_MAX_BEAM], h_tl[CP_MAX_BEAM];                          // times(): times_s if v_s > v_ns else times_ns
    __shared__ double e_tot[CP_SLOTS];
    __shared__ int e_key[CP_SLOTS];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int len = p.lens[b], beam = p.beam, V = p.V, blank = p.blank;
    const size_t astride = (size_t)p.T * beam + 1;
    int2* pa = p.parena + (size_t)b * astride;
    int2* ta = p.tarena + (size_t)b * astride;
    const float* rows = p.lp + (size_t)b * p.T * V;
    const bool graph = p.g_fail != nullptr;

    // is hypothesis i the prefix of hypothesis j less j's last token?
    auto is_parent = [&](int i, int j) -> bool {
        if (h_plen[j] != h_plen[i] + 1) return false;
        int x = h_pnode[j], y = h_node[i];
        if (x == y) return true;
        if (h_phash[j] != h_hash[i]) return false;
        while (x != y) {                                             // equal depth: the chains meet at the root at the latest
            const int2 ex = pa[x], ey = pa[y];
            if (ex.y != ey.y) return false;
            x = ex.x; y = ey.x;
        }
        return true;
    };
    // survivor `a` of frame t: hypothesis row a of the next frame
    auto put = [&](int a, int t, double s, double ns, double vs, double vns, double cs, int cst, int node, int pnode, int last, int plen,
                   unsigned long long hash, unsigned long long phash, int tns, int tls, int tnn, int tnp, int tln, bool tnew) {
        h_hash[a] = hash; h_phash[a] = phash;
        if (tnew) {
            tnn = t * beam + a;
            ta[tnn] = make_int2(tnp, t);
        }
        h_s[a] = s; h_ns[a] = ns; h_vs[a] = vs; h_vns[a] = vns; h_cs[a] = cs; h_cst[a] = cst;
        h_score[a] = prefix_log_add(s, ns);
        h_vit[a] = vs > vns ? vs : vns;
        h_node[a] = node; h_pnode[a] = pnode; h_last[a] = last; h_plen[a] = plen;
        h_tns[a] = tns; h_tls[a] = tls; h_tnn[a] = tnn; h_tnp[a] = tnp; h_tln[a] = tln;
        h_tn[a] = vs > vns ? tns : tnn;
        h_tl[a] = vs > vns ? tls : tln;
    };

    if (tid == 0) put(0, 0, 0.0, -INFINITY, 0.0, 0.0, 0.0, 0, 0, -1, -1, 0, BEAM_HASH0, 0ull, -1, 0, -1, -1, 0, false);   // search.py:142-149
    int nh = 1;
    float v0 = 0.f, v1 = 0.f;
    if (len > 0) {
        if (tid < V) v0 = rows[tid];
        if (tid + CP_NT < V) v1 = rows[tid + CP_NT];
    }
    __syncthreads();

    for (int t = 0; t < len; ++t) {
        // ---- first prune: top-beam of the frame ------------------------------------------------------------------------------
        unsigned long long k0 = tid < V ? cp_key(v0, tid) : 0ull, k1 = tid + CP_NT < V ? cp_key(v1, tid + CP_NT) : 0ull;
        if (t + 1 < len) {
            const float* nx = rows + (size_t)(t + 1) * V;
            if (tid < V) v0 = nx[tid];
            if (tid + CP_NT < V) v1 = nx[tid + CP_NT];
        }
        for (int q = 0; q < beam; ++q) {
            const unsigned long long w = cp_wave_max(k0 > k1 ? k0 : k1);
            if (lane == 0) wtop[wave][q] = w;
            if (k0 == w) k0 = 0ull;
            else if (k1 == w) k1 = 0ull;
        }
        __syncthreads();
        if (tid < 64) {
            const int q = tid & 15, w = tid >> 4;
            const unsigned long long my = q < beam ? wtop[w][q] : 0ull;
            if (my) {
                int rank = 0;
                for (int ww = 0; ww < CP_NT / 64; ++ww)
                    for (int qq = 0; qq < beam; ++qq) rank += wtop[ww][qq] > my;
                if (rank < beam) { top_tok[rank] = cp_key_index(my); top_p[rank] = (double)cp_key_value(my); }
            }
        }
        __syncthreads();

        // ---- expansion: the entry "P_j unchanged" (thread j) ---------------------------------------------------------------------
        int keyU = CP_NOKEY, Ucst = 0, Uts = -1, Utls = 0, Utnp = -1, Utln = 0;
        int Unode = 0, Upnode = -1, Ulast = -1, Uplen = 0;
        unsigned long long Uhash = 0ull, Uphash = 0ull, Nphash = 0ull;
        double Us = -INFINITY, Uns = -INFINITY, Uvs = -INFINITY, Uvns = -INFINITY, Uctp = -INFINITY, Ucs = 0.0, totU = 0.0;
        bool Uhas = false, Unew = false;
        if (tid < nh) {
            const int j = tid;
            Unode = h_node[j]; Upnode = h_pnode[j]; Ulast = h_last[j]; Uplen = h_plen[j]; Uhash = h_hash[j]; Uphash = h_phash[j];
            int par = -1;
            for (int i = 0; i < nh; ++i)
                if (is_parent(i, j)) par = i;
            // the extension P_par + u == P_j (search.py:188-201 when par ends in u, else :203-217)
            auto ext = [&](int r, int i, int u, double pr) {
                if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + i) * 2 + 1;
                const bool rep = h_last[i] == u;
                const double add = (rep ? h_s[i] : h_score[i]) + pr, vv = (rep ? h_vs[i] : h_vit[i]) + pr;
                Uns = prefix_log_add(Uns, add);
                if (Uvns < vv) {
                    Uvns = vv; Uctp = pr;
                    Unew = true; Utnp = rep ? h_tns[i] : h_tn[i]; Utln = (rep ? h_tls[i] : h_tl[i]) + 1;
                }
                if (!Uhas) {
                    Uhas = true;
                    Ucs = h_cs[i];
                    if (graph) {
                        int nx;
                        Ucs += cg_step(p.g_fail, p.g_off, p.g_ctok, p.g_cid, p.g_tscore, p.g_nscore, p.g_oscore, h_cst[i], u, &nx);
                        Ucst = nx;
                    }
                }
            };
            for (int r = 0; r < beam; ++r) {
                const int u = top_tok[r];
                const double pr = top_p[r];
                if (u == blank) {                                                    // :162-171
                    if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + j) * 2;
                    Us = prefix_log_add(Us, h_score[j] + pr);
                    Uvs = h_vit[j] + pr;
                    Uts = h_tn[j]; Utls = h_tl[j];
                    if (!Uhas) { Uhas = true; Ucs = h_cs[j]; Ucst = h_cst[j]; }
                } else if (u == Ulast) {
                    if (par >= 0 && par < j) ext(r, par, u, pr);
                    if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + j) * 2;          // :172-186
                    Uns = prefix_log_add(Uns, h_ns[j] + pr);
                    if (Uvns < h_vns[j] + pr) {
                        Uvns = h_vns[j] + pr;
                        if (Uctp < pr) {
                            Uctp = pr;
                            if (h_tln[j] > 0) { Unew = true; Utnp = h_tnp[j]; Utln = h_tln[j]; }   // times_ns[-1] = t
                        }
                    }
                    if (!Uhas) { Uhas = true; Ucs = h_cs[j]; Ucst = h_cst[j]; }
                    if (par > j) ext(r, par, u, pr);
                }
            }
            totU = prefix_log_add(Us, Uns) + Ucs;
        }
        if (tid < CP_MAX_BEAM) { e_key[tid] = keyU; e_tot[tid] = totU; }

        // ---- expansion: the entry "P_i + top[r]" (thread i * beam + r) unless that prefix is live ------------------------------------
        int keyN = CP_NOKEY, Ncst = 0, Ntnp = -1, Ntln = 0, Npnode = 0, Nlast = 0, Nplen = 0;
        double Nns = -INFINITY, Nvns = -INFINITY, Ncs = 0.0, totN = 0.0;
        bool Nnew = false;
        if (tid < nh * beam) {
            const int i = tid / beam, r = tid - i * beam, u = top_tok[r];
            bool live = u == blank;
            Npnode = h_node[i]; Nphash = h_hash[i];
            for (int j = 0; j < nh && !live; ++j) live = h_last[j] == u && is_parent(i, j);
            if (!live) {
                const double pr = top_p[r];
                const bool rep = h_last[i] == u;
                const double add = (rep ? h_s[i] : h_score[i]) + pr, vv = (rep ? h_vs[i] : h_vit[i]) + pr;
                keyN = (r * CP_MAX_BEAM + i) * 2 + 1;
                Nns = prefix_log_add(-INFINITY, add);
                if (-INFINITY < vv) { Nvns = vv; Nnew = true; Ntnp = rep ? h_tns[i] : h_tn[i]; Ntln = (rep ? h_tls[i] : h_tl[i]) + 1; }
                Ncs = h_cs[i];
                if (graph) {
                    int nx;
                    Ncs += cg_step(p.g_fail, p.g_off, p.g_ctok, p.g_cid, p.g_tscore, p.g_nscore, p.g_oscore, h_cst[i], u, &nx);
                    Ncst = nx;
                }
                Nlast = u; Nplen = h_plen[i] + 1;
                totN = prefix_log_add(-INFINITY, Nns) + Ncs;
            }
            e_key[CP_MAX_BEAM + tid] = keyN;
            e_tot[CP_MAX_BEAM + tid] = totN;
        }
        __syncthreads();

        // ---- second prune: rank by counting, stable over first-insertion order ---------------------------------------------------
        int rankU = 0, rankN = 0, nact = 0;
        const int nslots = CP_MAX_BEAM + nh * beam;
        for (int e = 0; e < nslots; ++e) {
            const int k = e_key[e];
            if (k == CP_NOKEY) continue;
            const double tt = e_tot[e];
            ++nact;
            rankU += (tt > totU) | ((tt == totU) & (k < keyU));
            rankN += (tt > totN) | ((tt == totN) & (k < keyN));
        }
        if (keyU != CP_NOKEY && rankU < beam)
            put(rankU, t, Us, Uns, Uvs, Uvns, Ucs, Ucst, Unode, Upnode, Ulast, Uplen, Uhash, Uphash, Uts, Utls, -1, Utnp, Utln, Unew);   // a fresh times_ns is []
        if (keyN != CP_NOKEY && rankN < beam) {
            const int node = 1 + t * beam + rankN;
            pa[node] = make_int2(Npnode, Nlast);
            put(rankN, t, -INFINITY, Nns, -INFINITY, Nvns, Ncs, Ncst, node, Npnode, Nlast, Nplen, beam_hash_step(Nphash, Nlast), Nphash, -1, 0, -1, Ntnp, Ntln, Nnew);
        }
        nh = nact < beam ? nact : beam;
        __syncthreads();
    }

    // ---- epilogue: this utterance's rows of the packed result -----------------------------------------------------------------------
    const size_t r0 = (size_t)b * beam;
    for (int q = tid; q < beam * p.lcap; q += CP_NT) { p.o_tok[r0 * p.lcap + q] = 0; p.o_time[r0 * p.lcap + q] = 0; }
    if (tid < beam) { p.o_len[r0 + tid] = 0; p.o_sc[r0 + tid] = 0.0; p.o_cs[r0 + tid] = 0.0; }
    if (tid == 0) p.o_nh[b] = nh;
    __syncthreads();
    if (tid < nh) {                                                  // scores and tokens
        const int a = tid, n = h_plen[a];
        const double cs = graph ? -p.g_nscore[h_cst[a]] : h_cs[a];    // finalize (context_graph.py:264) REPLACES the score (search.py:229-231)
        p.o_sc[r0 + a] = h_score[a] + cs;
        p.o_cs[r0 + a] = cs;
        p.o_len[r0 + a] = n;
        int node = h_node[a];
        for (int q = n - 1; q >= 0; --q) {
            const int2 e = pa[node];
            p.o_tok[(r0 + a) * p.lcap + q] = e.y;
            node = e.x;
        }
    } else if (tid >= 64 && tid < 64 + nh) {                         // times, on another wave
        const int a = tid - 64;
        int node = h_tn[a];
        for (int q = h_tl[a] - 1; q >= 0 && node >= 0; --q) {
            const int2 e = ta[node];
            p.o_time[(r0 + a) * p.lcap + q] = e.y;
            node = e.x;
        }
    }
}
