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
//
// The frame step (cp_frame), the hypothesis record (CpHyps, cp_put) and the packer (cp_pack) are ONE piece of code for two kernels:
//   ctc_prefix_search       the one-launch search above: frames [0, len) from the start hypothesis, packed by its epilogue
//   ctc_prefix_search_pool  the resumable form of the stream pool (rnnt_pool_ctc_prefix_logprobs): one workgroup per active row loads
//                           its slot's CpSlotState from device memory, walks the call's t new frames and stores the state back;
//                           ctc_prefix_pack packs a slot's hypotheses on demand.  Frames are absolute within the utterance and the
//                           arena nodes of frame t are 1 + t * CP_MAX_BEAM + rank / t * CP_MAX_BEAM + a, so the arena layout does
//                           not depend on the beam.  Node ids are only ever compared for equality, so the two numberings give the
//                           same search.
// Arenas of the pool: [max_streams][max_cache_frames * CP_MAX_BEAM + 1] int2 each, i.e. 1.28 MB per slot per arena at
// max_cache_frames = 5000, allocated on the first use of the pool's search.
#pragma once

constexpr int CP_NT = 256, CP_MAX_BEAM = 16, CP_SLOTS = CP_MAX_BEAM + CP_MAX_BEAM * CP_MAX_BEAM, CP_NOKEY = 0x7fffffff;
constexpr int CP_MAX_NODES = 4096;

// the context graph (CpGraph, cg_child, cg_step): rnnt_ctxgraph.hip.h; the n-gram model (NgTables, ng_step): rnnt_ngram.hip.h.
// The kernels are templates over NG, "an n-gram model is fused": NG = false compiles the search without it.

// packed results: [B], [B][beam], [B][beam][lcap] x 2, [B][beam] x 2, and (NG, optional) the n-gram scores [B][beam]
struct CpOutP { int* nh; int* len; int* tok; int* time; double* sc; double* cs; double* ls; };

struct CtcPrefixP {
    const float* lp;             // [B][T][V] log-probabilities
    const int* lens;             // [B]
    int T, V, blank, beam, lcap;
    CpGraph g;
    NgTables ng;
    int2* parena; int2* tarena;  // [B][T * beam + 1] each
    CpOutP o;
};

// The hypotheses of a search at a frame boundary: its whole state besides the two arenas.  In LDS while frames are walked; the
// stream pool keeps one per slot in device memory between calls (CpSlotState).
struct CpHyps {
    double s[CP_MAX_BEAM], ns[CP_MAX_BEAM], vs[CP_MAX_BEAM], vns[CP_MAX_BEAM], cs[CP_MAX_BEAM], score[CP_MAX_BEAM], vit[CP_MAX_BEAM];
    unsigned long long hash[CP_MAX_BEAM], phash[CP_MAX_BEAM];        // running hash of the prefix, and of the prefix less its last token
    int cst[CP_MAX_BEAM], node[CP_MAX_BEAM], pnode[CP_MAX_BEAM], last[CP_MAX_BEAM], plen[CP_MAX_BEAM];
    int tns[CP_MAX_BEAM], tls[CP_MAX_BEAM];                          // times_s: node, length
    int tnn[CP_MAX_BEAM], tnp[CP_MAX_BEAM], tln[CP_MAX_BEAM];        // times_ns: node, its parent, length
    int tn[CP_MAX_BEAM], tl[CP_MAX_BEAM];                            // times(): times_s if v_s > v_ns else times_ns
    double ls[CP_MAX_BEAM];                                          // n-gram score and state (NG_START until the first step)
    int lst[CP_MAX_BEAM];
};
struct CpSlotState { CpHyps h; int nh, pad; };                       // 8 f64, 2 u64 and 13 int per hypothesis + the count: 2120 bytes

// per-frame work area in LDS
struct CpWork {
    unsigned long long wtop[CP_NT / 64][CP_MAX_BEAM];
    int top_tok[CP_MAX_BEAM];
    double top_p[CP_MAX_BEAM];
    double e_tot[CP_SLOTS];
    int e_key[CP_SLOTS];
};

// the resumable search of the stream pool: row i of the call is slot slots[i], whose frames [t0[i], t0[i] + t) these are
struct CtcPrefixPoolP {
    const float* lp;             // [n][t][V] log-probabilities
    const int* slots;            // [n]
    const int* t0;               // [n] frames the slot's search has walked before this call
    int t, V, blank, beam;
    CpGraph g;
    NgTables ng;
    int2* parena; int2* tarena;  // [max_streams][astride] each, astride = max_cache_frames * CP_MAX_BEAM + 1
    size_t astride;
    CpSlotState* state;          // [max_streams]
};

// one slot's hypotheses as the one-launch search's epilogue packs them; fin_nscore != nullptr: finalize's context score; final: the
// n-gram end term is added (NG)
struct CtcPrefixPackP {
    const CpSlotState* state;    // the slot's record
    const int2* pa; const int2* ta;
    const double* fin_nscore;
    NgTables ng;
    int beam, lcap, final;
    CpOutP o;
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

__device__ inline unsigned long long cp_wave_max(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}

// is hypothesis i the prefix of hypothesis j less j's last token?
__device__ __forceinline__ bool cp_is_parent(const CpHyps& H, const int2* pa, int i, int j) {
    if (H.plen[j] != H.plen[i] + 1) return false;
    int x = H.pnode[j], y = H.node[i];
    if (x == y) return true;
    if (H.phash[j] != H.hash[i]) return false;
    while (x != y) {                                                 // equal depth: the chains meet at the root at the latest
        const int2 ex = pa[x], ey = pa[y];
        if (ex.y != ey.y) return false;
        x = ex.x; y = ey.x;
    }
    return true;
}

// survivor `a` of frame t: hypothesis row a of the next frame (stride: time-arena nodes per frame)
template <bool NG>
__device__ __forceinline__ void cp_put(CpHyps& H, int2* ta, int stride, int a, int t, double s, double ns, double vs, double vns, double cs, int cst,
                                       double ls, int lst, int node, int pnode, int last, int plen, unsigned long long hash, unsigned long long phash, int tns, int tls,
                                       int tnn, int tnp, int tln, bool tnew) {
    H.hash[a] = hash; H.phash[a] = phash;
    if (tnew) {
        tnn = t * stride + a;
        ta[tnn] = make_int2(tnp, t);
    }
    H.s[a] = s; H.ns[a] = ns; H.vs[a] = vs; H.vns[a] = vns; H.cs[a] = cs; H.cst[a] = cst;
    if (NG) { H.ls[a] = ls; H.lst[a] = lst; }
    H.score[a] = prefix_log_add(s, ns);
    H.vit[a] = vs > vns ? vs : vns;
    H.node[a] = node; H.pnode[a] = pnode; H.last[a] = last; H.plen[a] = plen;
    H.tns[a] = tns; H.tls[a] = tls; H.tnn[a] = tnn; H.tnp[a] = tnp; H.tln[a] = tln;
    H.tn[a] = vs > vns ? tns : tnn;
    H.tl[a] = vs > vns ? tls : tln;
}

// the start hypothesis (search.py:142-149): the empty prefix, s = 0, ns = -inf, v_s = v_ns = 0, context root, n-gram start marker
__device__ __forceinline__ void cp_put_start(CpHyps& H) {
    cp_put<true>(H, nullptr, 0, 0, 0, 0.0, -INFINITY, 0.0, 0.0, 0.0, 0, 0.0, NG_START, 0, -1, -1, 0, BEAM_HASH0, 0ull, -1, 0, -1, -1, 0, false);
}

// One frame of the search for the whole workgroup (CP_NT threads, four barriers): frame t of the utterance, whose row the caller
// holds in (v0, v1); next_row (or nullptr) is prefetched into them.  stride: arena nodes per frame.  nh: hypotheses before / after.
template <bool NG>
__device__ __forceinline__ void cp_frame(CpHyps& H, CpWork& W, const CpGraph& g, const NgTables& ng, int2* pa, int2* ta, const float* next_row, int t, int stride,
                                         int beam, int V, int blank, int& nh, float& v0, float& v1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool graph = g.fail != nullptr;
    // ---- first prune: top-beam of the frame ------------------------------------------------------------------------------
    unsigned long long k0 = tid < V ? cp_key(v0, tid) : 0ull, k1 = tid + CP_NT < V ? cp_key(v1, tid + CP_NT) : 0ull;
    if (next_row) {
        if (tid < V) v0 = next_row[tid];
        if (tid + CP_NT < V) v1 = next_row[tid + CP_NT];
    }
    for (int q = 0; q < beam; ++q) {
        const unsigned long long w = cp_wave_max(k0 > k1 ? k0 : k1);
        if (lane == 0) W.wtop[wave][q] = w;
        if (k0 == w) k0 = 0ull;
        else if (k1 == w) k1 = 0ull;
    }
    __syncthreads();
    if (tid < 64) {
        const int q = tid & 15, w = tid >> 4;
        const unsigned long long my = q < beam ? W.wtop[w][q] : 0ull;
        if (my) {
            int rank = 0;
            for (int ww = 0; ww < CP_NT / 64; ++ww)
                for (int qq = 0; qq < beam; ++qq) rank += W.wtop[ww][qq] > my;
            if (rank < beam) { W.top_tok[rank] = cp_key_index(my); W.top_p[rank] = (double)cp_key_value(my); }
        }
    }
    __syncthreads();

    // ---- expansion: the entry "P_j unchanged" (thread j) ---------------------------------------------------------------------
    int keyU = CP_NOKEY, Ucst = 0, Ulst = NG_START, Uts = -1, Utls = 0, Utnp = -1, Utln = 0;
    int Unode = 0, Upnode = -1, Ulast = -1, Uplen = 0;
    unsigned long long Uhash = 0ull, Uphash = 0ull, Nphash = 0ull;
    double Us = -INFINITY, Uns = -INFINITY, Uvs = -INFINITY, Uvns = -INFINITY, Uctp = -INFINITY, Ucs = 0.0, Uls = 0.0, totU = 0.0;
    bool Uhas = false, Unew = false;
    if (tid < nh) {
        const int j = tid;
        Unode = H.node[j]; Upnode = H.pnode[j]; Ulast = H.last[j]; Uplen = H.plen[j]; Uhash = H.hash[j]; Uphash = H.phash[j];
        int par = -1;
        for (int i = 0; i < nh; ++i)
            if (cp_is_parent(H, pa, i, j)) par = i;
        // the extension P_par + u == P_j (search.py:188-201 when par ends in u, else :203-217)
        auto ext = [&](int r, int i, int u, double pr) {
            if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + i) * 2 + 1;
            const bool rep = H.last[i] == u;
            const double add = (rep ? H.s[i] : H.score[i]) + pr, vv = (rep ? H.vs[i] : H.vit[i]) + pr;
            Uns = prefix_log_add(Uns, add);
            if (Uvns < vv) {
                Uvns = vv; Uctp = pr;
                Unew = true; Utnp = rep ? H.tns[i] : H.tn[i]; Utln = (rep ? H.tls[i] : H.tl[i]) + 1;
            }
            if (!Uhas) {
                Uhas = true;
                Ucs = H.cs[i];
                if (graph) {
                    int nx;
                    Ucs += cg_step(g.fail, g.off, g.ctok, g.cid, g.tscore, g.nscore, g.oscore, H.cst[i], u, &nx);
                    Ucst = nx;
                }
                if (NG) {
                    int nx;
                    Uls = H.ls[i] + ng_step(ng, H.lst[i], u, &nx);
                    Ulst = nx;
                }
            }
        };
        for (int r = 0; r < beam; ++r) {
            const int u = W.top_tok[r];
            const double pr = W.top_p[r];
            if (u == blank) {                                                    // :162-171
                if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + j) * 2;
                Us = prefix_log_add(Us, H.score[j] + pr);
                Uvs = H.vit[j] + pr;
                Uts = H.tn[j]; Utls = H.tl[j];
                if (!Uhas) { Uhas = true; Ucs = H.cs[j]; Ucst = H.cst[j]; Uls = H.ls[j]; Ulst = H.lst[j]; }
            } else if (u == Ulast) {
                if (par >= 0 && par < j) ext(r, par, u, pr);
                if (keyU == CP_NOKEY) keyU = (r * CP_MAX_BEAM + j) * 2;          // :172-186
                Uns = prefix_log_add(Uns, H.ns[j] + pr);
                if (Uvns < H.vns[j] + pr) {
                    Uvns = H.vns[j] + pr;
                    if (Uctp < pr) {
                        Uctp = pr;
                        if (H.tln[j] > 0) { Unew = true; Utnp = H.tnp[j]; Utln = H.tln[j]; }   // times_ns[-1] = t
                    }
                }
                if (!Uhas) { Uhas = true; Ucs = H.cs[j]; Ucst = H.cst[j]; Uls = H.ls[j]; Ulst = H.lst[j]; }
                if (par > j) ext(r, par, u, pr);
            }
        }
        totU = prefix_log_add(Us, Uns) + Ucs;
        if (NG) totU += Uls;
    }
    if (tid < CP_MAX_BEAM) { W.e_key[tid] = keyU; W.e_tot[tid] = totU; }

    // ---- expansion: the entry "P_i + top[r]" (thread i * beam + r) unless that prefix is live ------------------------------------
    int keyN = CP_NOKEY, Ncst = 0, Nlst = NG_START, Ntnp = -1, Ntln = 0, Npnode = 0, Nlast = 0, Nplen = 0;
    double Nns = -INFINITY, Nvns = -INFINITY, Ncs = 0.0, Nls = 0.0, totN = 0.0;
    bool Nnew = false;
    if (tid < nh * beam) {
        const int i = tid / beam, r = tid - i * beam, u = W.top_tok[r];
        bool live = u == blank;
        Npnode = H.node[i]; Nphash = H.hash[i];
        for (int j = 0; j < nh && !live; ++j) live = H.last[j] == u && cp_is_parent(H, pa, i, j);
        if (!live) {
            const double pr = W.top_p[r];
            const bool rep = H.last[i] == u;
            const double add = (rep ? H.s[i] : H.score[i]) + pr, vv = (rep ? H.vs[i] : H.vit[i]) + pr;
            keyN = (r * CP_MAX_BEAM + i) * 2 + 1;
            Nns = prefix_log_add(-INFINITY, add);
            if (-INFINITY < vv) { Nvns = vv; Nnew = true; Ntnp = rep ? H.tns[i] : H.tn[i]; Ntln = (rep ? H.tls[i] : H.tl[i]) + 1; }
            Ncs = H.cs[i];
            if (graph) {
                int nx;
                Ncs += cg_step(g.fail, g.off, g.ctok, g.cid, g.tscore, g.nscore, g.oscore, H.cst[i], u, &nx);
                Ncst = nx;
            }
            if (NG) {
                int nx;
                Nls = H.ls[i] + ng_step(ng, H.lst[i], u, &nx);
                Nlst = nx;
            }
            Nlast = u; Nplen = H.plen[i] + 1;
            totN = prefix_log_add(-INFINITY, Nns) + Ncs;
            if (NG) totN += Nls;
        }
        W.e_key[CP_MAX_BEAM + tid] = keyN;
        W.e_tot[CP_MAX_BEAM + tid] = totN;
    }
    __syncthreads();

    // ---- second prune: rank by counting, stable over first-insertion order ---------------------------------------------------
    int rankU = 0, rankN = 0, nact = 0;
    const int nslots = CP_MAX_BEAM + nh * beam;
    for (int e = 0; e < nslots; ++e) {
        const int k = W.e_key[e];
        if (k == CP_NOKEY) continue;
        const double tt = W.e_tot[e];
        ++nact;
        rankU += (tt > totU) | ((tt == totU) & (k < keyU));
        rankN += (tt > totN) | ((tt == totN) & (k < keyN));
    }
    if (keyU != CP_NOKEY && rankU < beam)
        cp_put<NG>(H, ta, stride, rankU, t, Us, Uns, Uvs, Uvns, Ucs, Ucst, Uls, Ulst, Unode, Upnode, Ulast, Uplen, Uhash, Uphash, Uts, Utls, -1, Utnp, Utln, Unew);   // a fresh times_ns is []
    if (keyN != CP_NOKEY && rankN < beam) {
        const int node = 1 + t * stride + rankN;
        pa[node] = make_int2(Npnode, Nlast);
        cp_put<NG>(H, ta, stride, rankN, t, -INFINITY, Nns, -INFINITY, Nvns, Ncs, Ncst, Nls, Nlst, node, Npnode, Nlast, Nplen, beam_hash_step(Nphash, Nlast), Nphash, -1, 0, -1, Ntnp,
               Ntln, Nnew);
    }
    nh = nact < beam ? nact : beam;
    __syncthreads();
}

// Row b of the packed result from the nh hypotheses in H (whole workgroup, CP_NT threads): zero fill, then scores and tokens on one
// wave and times on another.  fin_nscore != nullptr: finalize (context_graph.py:264) REPLACES the context score (search.py:229-231).
// NG: the score carries the n-gram score, with the end term when `final`.
template <bool NG>
__device__ __forceinline__ void cp_pack(const CpHyps& H, int nh, const int2* pa, const int2* ta, const double* fin_nscore, const NgTables& ng, bool final,
                                        const CpOutP& o, int b, int beam, int lcap) {
    const int tid = threadIdx.x;
    const size_t r0 = (size_t)b * beam;
    for (int q = tid; q < beam * lcap; q += CP_NT) { o.tok[r0 * lcap + q] = 0; o.time[r0 * lcap + q] = 0; }
    if (tid < beam) {
        o.len[r0 + tid] = 0; o.sc[r0 + tid] = 0.0; o.cs[r0 + tid] = 0.0;
        if (NG && o.ls) o.ls[r0 + tid] = 0.0;
    }
    if (tid == 0) o.nh[b] = nh;
    __syncthreads();
    if (tid < nh) {                                                  // scores and tokens
        const int a = tid, n = H.plen[a];
        const double cs = fin_nscore ? -fin_nscore[H.cst[a]] : H.cs[a];
        double sc = H.score[a] + cs;
        if (NG) {
            double ls = H.ls[a];
            if (final) ls += ng_eos(ng, H.lst[a]);
            sc += ls;
            if (o.ls) o.ls[r0 + a] = ls;
        }
        o.sc[r0 + a] = sc;
        o.cs[r0 + a] = cs;
        o.len[r0 + a] = n;
        int node = H.node[a];
        for (int q = n - 1; q >= 0; --q) {
            const int2 e = pa[node];
            o.tok[(r0 + a) * lcap + q] = e.y;
            node = e.x;
        }
    } else if (tid >= 64 && tid < 64 + nh) {                         // times, on another wave
        const int a = tid - 64;
        int node = H.tn[a];
        for (int q = H.tl[a] - 1; q >= 0 && node >= 0; --q) {
            const int2 e = ta[node];
            o.time[(r0 + a) * lcap + q] = e.y;
            node = e.x;
        }
    }
}

// element `i` of every array of a hypothesis record (threads i < CP_MAX_BEAM copy a record between LDS and device memory); the
// n-gram pair only where a model is fused or the record is made
template <bool NG>
__device__ __forceinline__ void cp_hyps_copy(CpHyps& d, const CpHyps& s, int i) {
    if (NG) { d.ls[i] = s.ls[i]; d.lst[i] = s.lst[i]; }
    d.s[i] = s.s[i]; d.ns[i] = s.ns[i]; d.vs[i] = s.vs[i]; d.vns[i] = s.vns[i]; d.cs[i] = s.cs[i]; d.score[i] = s.score[i]; d.vit[i] = s.vit[i];
    d.hash[i] = s.hash[i]; d.phash[i] = s.phash[i];
    d.cst[i] = s.cst[i]; d.node[i] = s.node[i]; d.pnode[i] = s.pnode[i]; d.last[i] = s.last[i]; d.plen[i] = s.plen[i];
    d.tns[i] = s.tns[i]; d.tls[i] = s.tls[i]; d.tnn[i] = s.tnn[i]; d.tnp[i] = s.tnp[i]; d.tln[i] = s.tln[i]; d.tn[i] = s.tn[i]; d.tl[i] = s.tl[i];
}

template <bool NG>
__global__ __launch_bounds__(CP_NT) void ctc_prefix_search(CtcPrefixP p) {
    __shared__ CpHyps H;
    __shared__ CpWork W;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = p.lens[b], beam = p.beam, V = p.V;
    const size_t astride = (size_t)p.T * beam + 1;
    int2* pa = p.parena + (size_t)b * astride;
    int2* ta = p.tarena + (size_t)b * astride;
    const float* rows = p.lp + (size_t)b * p.T * V;

    if (tid == 0) cp_put_start(H);
    int nh = 1;
    float v0 = 0.f, v1 = 0.f;
    if (len > 0) {
        if (tid < V) v0 = rows[tid];
        if (tid + CP_NT < V) v1 = rows[tid + CP_NT];
    }
    __syncthreads();
    for (int t = 0; t < len; ++t)
        cp_frame<NG>(H, W, p.g, p.ng, pa, ta, t + 1 < len ? rows + (size_t)(t + 1) * V : nullptr, t, beam, beam, V, p.blank, nh, v0, v1);
    // ---- epilogue: this utterance's rows of the packed result -----------------------------------------------------------------------
    cp_pack<NG>(H, nh, pa, ta, p.g.fail ? p.g.nscore : nullptr, p.ng, true, p.o, b, beam, p.lcap);
}

// The resumable form: workgroup i continues the search of slot slots[i] over the call's t rows, frames [t0[i], t0[i] + t) of its
// utterance.  The prefetch of the next row stays inside those rows.  No epilogue (ctc_prefix_pack).
template <bool NG>
__global__ __launch_bounds__(CP_NT) void ctc_prefix_search_pool(CtcPrefixPoolP p) {
    __shared__ CpHyps H;
    __shared__ CpWork W;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int slot = p.slots[i], t0 = p.t0[i], V = p.V;
    int2* pa = p.parena + (size_t)slot * p.astride;
    int2* ta = p.tarena + (size_t)slot * p.astride;
    const float* rows = p.lp + (size_t)i * p.t * V;
    CpSlotState* st = p.state + slot;

    if (tid < CP_MAX_BEAM) cp_hyps_copy<NG>(H, st->h, tid);
    int nh = st->nh;
    float v0 = 0.f, v1 = 0.f;
    if (tid < V) v0 = rows[tid];
    if (tid + CP_NT < V) v1 = rows[tid + CP_NT];
    __syncthreads();
    for (int f = 0; f < p.t; ++f)
        cp_frame<NG>(H, W, p.g, p.ng, pa, ta, f + 1 < p.t ? rows + (size_t)(f + 1) * V : nullptr, t0 + f, CP_MAX_BEAM, p.beam, V, p.blank, nh, v0, v1);
    if (tid < CP_MAX_BEAM) cp_hyps_copy<NG>(st->h, H, tid);
    if (tid == 0) st->nh = nh;
}

// one slot's hypotheses as they stand, in the layout of the one-launch search for B = 1; reads only
template <bool NG>
__global__ __launch_bounds__(CP_NT) void ctc_prefix_pack(CtcPrefixPackP p) {
    __shared__ CpHyps H;
    const int tid = threadIdx.x;
    if (tid < CP_MAX_BEAM) cp_hyps_copy<NG>(H, p.state->h, tid);
    const int nh = p.state->nh;
    __syncthreads();
    cp_pack<NG>(H, nh, p.pa, p.ta, p.fin_nscore, p.ng, p.final != 0, p.o, 0, p.beam, p.lcap);
}

// the start hypothesis in the record *st, every other entry of it zero; z: an LDS record of the workgroup (>= CP_MAX_BEAM threads,
// all of them here)
__device__ __forceinline__ void ctc_prefix_slot_start(CpSlotState* st, CpSlotState& z) {
    const int tid = threadIdx.x;
    for (int q = tid; q < (int)(sizeof(CpSlotState) / sizeof(int)); q += blockDim.x) reinterpret_cast<int*>(&z)[q] = 0;
    __syncthreads();
    if (tid == 0) { cp_put_start(z.h); z.nh = 1; }
    __syncthreads();
    if (tid < CP_MAX_BEAM) cp_hyps_copy<true>(st->h, z.h, tid);
    if (tid == 0) { st->nh = z.nh; st->pad = 0; }
}

// the start hypothesis in the records of slots [slot0, slot0 + gridDim.x)
__global__ __launch_bounds__(64) void ctc_prefix_slot_reset(CpSlotState* state, int slot0) {
    __shared__ CpSlotState z;
    ctc_prefix_slot_start(state + slot0 + blockIdx.x, z);
}
