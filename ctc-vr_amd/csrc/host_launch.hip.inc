// Host-side helpers of librnnt_hip.so: error/alloc utilities, GEMM descriptor preparation and launchers, per-layer descriptor
// builders, the encoder's frame emission and the stream pool's beam state helpers.  Included by rnnt_api.hip.

namespace {

int fail(rnnt_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(ctx, RNNT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the launch-error check alone: inside a launch macro whose call site then names the launch form with LAUNCHCHK
#define LAUNCHERR(name)                                                                                \
    do {                                                                                               \
        hipError_t e_ = hipGetLastError();                                                             \
        if (e_ != hipSuccess) return fail(ctx, RNNT_ERR_HIP, "launch %s failed: %s", name, hipGetErrorString(e_)); \
    } while (0)

// after every launch: the error check, the launch count and -- while a form log is open -- the form name of the site
#define LAUNCHCHK(name)                                                                                \
    do {                                                                                               \
        LAUNCHERR(name);                                                                               \
        ctx->launches++;                                                                               \
        if (ctx->form_log_on) ctx->form_log[name]++;                                                   \
    } while (0)

// launch-site tags (rnnt_profile_begin)
enum { TAG_NONE = 0, TAG_CONV1 = 1, TAG_CONV2 = 2, TAG_EMBED = 3, TAG_FFN1 = 4, TAG_FFN2 = 5, TAG_QKV = 6, TAG_ATTN = 7, TAG_ATTN_OUT = 8,
       TAG_PW1 = 9, TAG_DWCONV = 10, TAG_PW2 = 11, TAG_LN = 12, TAG_ENC_PROJ = 13, TAG_LSTM = 20, TAG_PRED_PROJ = 21,
       TAG_JOINT_TANH = 22, TAG_JOINT_OUT = 23, TAG_GREEDY_UPDATE = 24, TAG_BLOCK_FRONT = 30, TAG_BLOCK_BACK = 31, TAG_FFN_FUSED = 32, TAG_FFN_QKV = 33, TAG_OUT_PW1 = 34, TAG_FFN_MERGED = 35,
       TAG_CONV1_MINOR = 36, TAG_CONV2_MINOR = 37, TAG_EMBED_MINOR = 38,   // subsampling of the minor chunk classes of a whole-utterance call (the tail chunk)
       TAG_SCORE_PICK = 40, TAG_SCORE_ALPHA = 41,     // scoring: the picked lattice (fused kernel, or lattice + gather); transducer_alpha / ctc_alpha
       TAG_SCORE_VITERBI = 42,                        // forced alignment: transducer_viterbi / ctc_viterbi, back-trace included
       TAG_PREFIX_STEP = 43, TAG_PREFIX_MERGE = 44,   // prefix beam search: prefix_step / prefix_merge, one launch each per frame
       TAG_CTC_PREFIX = 45,                           // CTC prefix beam search: ctc_prefix_search, one launch per call
       TAG_CTC_PREFIX_POOL = 46, TAG_CTC_PREFIX_PACK = 47,     // its resumable form per slot of the stream pool: ctc_prefix_search_pool / ctc_prefix_pack
       TAG_WAVE_STAGE = 48,                           // streaming front-end of the stream pool: wave_stage of rnnt_pool_wave
       TAG_PREFIX_STEP_POOL = 49, TAG_PREFIX_MERGE_POOL = 50,     // prefix beam search per slot of the stream pool: prefix_step_pool / prefix_merge_pool, one launch each per frame
       TAG_CTC_LOSS_PICK = 51, TAG_CTC_LOSS_RECURSION = 52, TAG_CTC_LOSS_OCC = 53, TAG_CTC_LOSS_GRAD = 54 };   // rnnt_ctc_loss: ctc_loss_pick / ctc_alpha_beta / ctc_loss_occ / ctc_loss_grad, one launch each per call

struct ProfScope {   // records a start/stop event pair around one launch when its site is selected
    rnnt_ctx* ctx; hipStream_t s; bool on;
    ProfScope(rnnt_ctx* c, hipStream_t st, int tag) : ctx(c), s(st), on(c->prof_tag == tag && tag != TAG_NONE && !c->capturing) {
        if (on) {
            if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
                for (int i = 0; i < 2; ++i) { hipEvent_t e; (void)hipEventCreate(&e); ctx->prof_ev.push_back(e); }
            }
            (void)hipEventRecord(ctx->prof_ev[ctx->prof_used], s);
        }
    }
    ~ProfScope() {
        if (on) { (void)hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], s); ctx->prof_used += 2; }
    }
};

// n elements for an empty owner.  A refused allocation must not linger as HIP's per-thread last error: LAUNCHCHK of the next
// launch on this thread, in any context, would report it.
template <typename T, bool HOST>
int dmalloc(rnnt_ctx* ctx, DevBuf<T, HOST>& b, size_t n) {
    const size_t bytes = n * sizeof(T);
    void* q = nullptr;
    const hipError_t e = HOST ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, HOST ? RNNT_ERR_HIP : RNNT_ERR_OOM, "%s of %zu bytes failed", HOST ? "hipHostMalloc" : "hipMalloc", bytes);
    }
    b.p = static_cast<T*>(q);
    b.cap = q ? n : 0;
    if (!HOST) live_device_bytes += (int64_t)(b.cap * sizeof(T));
    return RNNT_OK;
}

// at least n elements: grow-only, contents are not preserved; a buffer that already holds n is left alone
template <typename T, bool HOST>
int reserve(rnnt_ctx* ctx, DevBuf<T, HOST>& b, size_t n) {
    if (n <= b.cap) return RNNT_OK;
    b.release();
    return dmalloc(ctx, b, n);
}

// exactly n elements: re-allocated when the size differs (the caller has synchronised the stream that may still read the old one)
template <typename T>
int reserve_exact(rnnt_ctx* ctx, DevBuf<T>& b, size_t n) {
    if (n != b.cap) b.release();
    return reserve(ctx, b, n);
}

// The layout of a carved buffer, written once: take(n) hands out consecutive regions of n elements.  Walk it without a base for the
// size to reserve (off), then over the buffer -- or over a host copy of the same block -- for the pointers.
template <typename T>
struct Carve {
    T* base = nullptr;
    size_t off = 0;
    T* take(size_t n) {
        T* r = base ? base + off : nullptr;
        off += n;
        return r;
    }
};

// ---- the call tables of the stream pool (CallTab): room for n ints on both sides and the event, once -----------------------------------
int calltab_alloc(rnnt_ctx* ctx, CallTab& t, size_t n) {
    int rc;
    if ((rc = reserve(ctx, t.dev, n))) return rc;
    if ((rc = reserve(ctx, t.host, n))) return rc;
    if (!t.ev) HIPCHK(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming));
    return RNNT_OK;
}
// the pinned copy, free to be filled: the previous call's copy has left it (normally long ago)
int calltab_fill(rnnt_ctx* ctx, CallTab& t, int*& host) {
    HIPCHK(hipEventSynchronize(t.ev));
    host = t.host;
    return RNNT_OK;
}
// its first n ints to the device: one async copy, no synchronisation before the launches that read it
int calltab_send(rnnt_ctx* ctx, CallTab& t, size_t n, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(t.dev, t.host, n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(t.ev, s));
    return RNNT_OK;
}

// the decoder and joint weights that the beam's and the prefix search's step kernels share (BeamChainP, PrefixStepP)
template <typename P>
void dec_weights(const rnnt_ctx* ctx, P& p) {
    p.whh = ctx->whh_il; p.egate = ctx->egate; p.wpr = ctx->wpr; p.bpr = ctx->bpr; p.wpf = ctx->wpf; p.bpf = ctx->bpf; p.wout = ctx->wout; p.bout = ctx->bout;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is per device: keep the "already raised" record in the context (one context = one
// device, one host thread at a time), not in a process-wide static (a second device, or a second host thread, would miss it).
int ensure_dyn_lds(rnnt_ctx* ctx, const void* fn, size_t bytes) {
    auto it = ctx->dyn_lds.find(fn);
    if (it != ctx->dyn_lds.end() && it->second >= (int)bytes) return RNNT_OK;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ctx->dyn_lds[fn] = (int)bytes;
    return RNNT_OK;
}

struct GemmCapScope {   // row-count dependent kernel choices as for one stream, for the launches of one pool call (or of a search that must not depend on its batch)
    rnnt_ctx* ctx;
    explicit GemmCapScope(rnnt_ctx* c) : ctx(c) { ctx->gemm_m_cap = 1023; }
    ~GemmCapScope() { ctx->gemm_m_cap = 0; }
};

constexpr int WF_MERGE_MAX = 4;   // chunks of one layer per wavefront stage (rnnt_encoder_chunks), upper bound
inline int sub_len(int T) { return ((T - 3) / 2 + 1 - 3) / 2 + 1; }   // subsampling.py:188-193
inline int sub1_len(int T) { return (T - 3) / 2 + 1; }

GemmP plain_gemm(const float* A, int lda, const float* W, int ldw, const float* bias, float* C, int ldc, int M, int N, int K,
                 int epi = EPI_BIAS, float alpha = 1.f) {
    GemmP p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.W = W; p.bias = bias; p.C = C; p.R = nullptr; p.ln_g = nullptr; p.ln_b = nullptr;
    p.M = M; p.N = N; p.K = K;
    p.a_n1 = BIG; p.a_n2 = BIG; p.a_s0 = 0; p.a_s1 = 0; p.a_s2 = lda; p.a_seg = BIG; p.a_seg_stride = 0;
    p.ldw = ldw;
    p.c_n = BIG; p.c_r0 = 0; p.c_mod = BIG; p.c_s0 = 0; p.c_s1 = ldc;
    p.epi = epi; p.alpha = alpha;
    p.x_n = 1;
    return p;
}

// q = umulhi(n, magic) >> shift, exact for 0 <= n < 2^31 (round-up method: magic = ceil(2^(32+shift) / d))
inline void div_magic(int d, unsigned& magic, int& shift) {
    if (d <= 1) { magic = 0; shift = 0; return; }
    int l = 0;
    while ((1ll << l) < d) ++l;          // l = ceil(log2 d)
    shift = l - 1;
    const unsigned long long num = 1ull << (32 + shift);
    magic = (unsigned)((num + (unsigned long long)d - 1) / (unsigned long long)d);
}

// fast-path flags and division magics of one GEMM descriptor (gemm16's a_row_off / c_row_off)
int prepare_gemm(rnnt_ctx* ctx, GemmP& g) {
    g.Wh = g.Wl = nullptr;
    if (ctx->numerics != RNNT_NUM_F32 && ctx->blob_hi && g.W >= ctx->blob && g.W < ctx->blob + ctx->blob.cap) {
        g.Wh = ctx->blob_hi + (g.W - ctx->blob);
        g.Wl = ctx->blob_lo + (g.W - ctx->blob);
    }
    g.a_plain = (g.a_n1 == BIG && g.a_n2 == BIG && g.a_seg == BIG) ? 1 : 0;
    g.c_plain = (g.c_n == BIG && g.c_r0 == 0) ? 1 : 0;
    if ((long long)g.M >= (1ll << 31) || (long long)g.K >= (1ll << 31)) return fail(ctx, RNNT_ERR_SHAPE, "gemm index range too large");
    if (!g.a_plain) {
        if (g.a_n1 == BIG) g.a_n1 = g.M > 0 ? g.M + 1 : 1;   // quotient 0, remainder m
        if (g.a_n2 == BIG) g.a_n2 = g.M > 0 ? g.M + 1 : 1;
        if (g.a_seg == BIG) { g.a_seg = g.K + 1; g.a_seg_stride = 0; }
    }
    if (!g.c_plain && g.c_n == BIG) g.c_n = g.M > 0 ? g.M + 1 : 1;
    div_magic(g.a_n1, g.a_n1_magic, g.a_n1_shift); div_magic(g.a_n2, g.a_n2_magic, g.a_n2_shift);
    div_magic(g.a_seg, g.a_seg_magic, g.a_seg_shift); div_magic(g.c_n, g.c_n_magic, g.c_n_shift);
    div_magic(g.x_n, g.x_n_magic, g.x_n_shift);
    return RNNT_OK;
}

template <int WK, int NT>
void launch_gemm16(hipStream_t s, const GemmBatch& gb, int maxM, int maxN, int ng) {
    dim3 grid((maxN + 16 * NT - 1) / (16 * NT), (maxM + 15) / 16, ng);
    hipLaunchKernelGGL((gemm16<WK, 1, NT>), grid, dim3(64 * WK), 0, s, gb);
}

// gemm_ns with the XCD-aware 1-D grid (see the kernel): ceil(ntm / 8) * 8 * ntn workgroups per descriptor
static int prefetch_depth(const rnnt_ctx* ctx) {   // K blocks in flight per workgroup (register ring of gemm_ns_body): 1 or 2
    return ctx->gemm_pd == 1 ? 1 : 2;
}
template <int MT, int NT, bool ATANH = false, bool ANT = false>
void launch_gemm_ns(const rnnt_ctx* ctx, hipStream_t s, const GemmBatch& gb, int maxM, int maxN, int ng) {
    const int ntn = (maxN + 32 * NT - 1) / (32 * NT), ntm = (maxM + 32 * MT - 1) / (32 * MT);
    dim3 grid(((ntm + 7) / 8) * 8 * ntn, 1, ng);
    switch (prefetch_depth(ctx)) {
        case 1: hipLaunchKernelGGL((gemm_ns<MT, NT, 32, 1, ATANH, ANT>), grid, dim3(256), 0, s, gb, ntn, ntm); break;
        default: hipLaunchKernelGGL((gemm_ns<MT, NT, 32, 2, ATANH, ANT>), grid, dim3(256), 0, s, gb, ntn, ntm); break;
    }
}
// the same launch on the 16-bit split-operand kernels (rnnt_gemm_bf.hip.h), by numerics mode
template <int MT, int NT, bool ATANH = false>
void launch_gemm_bf(int numerics, hipStream_t s, const GemmBatch& gb, int maxM, int maxN, int ng) {
    const int ntn = (maxN + 32 * NT - 1) / (32 * NT), ntm = (maxM + 32 * MT - 1) / (32 * MT);
    dim3 grid(((ntm + 7) / 8) * 8 * ntn, 1, ng);
    switch (numerics) {
        case RNNT_NUM_BF16: hipLaunchKernelGGL((gemm_bf<1, false, MT, NT, ATANH>), grid, dim3(256), 0, s, gb, ntn, ntm); break;
        case RNNT_NUM_F16X3: hipLaunchKernelGGL((gemm_bf<2, true, MT, NT, ATANH>), grid, dim3(256), 0, s, gb, ntn, ntm); break;
        default: hipLaunchKernelGGL((gemm_bf<2, false, MT, NT, ATANH>), grid, dim3(256), 0, s, gb, ntn, ntm); break;
    }
}
static bool all_planes(const GemmBatch& gb, int ng) {
    for (int i = 0; i < ng; ++i)
        if (!gb.g[i].Wh) return false;
    return true;
}

// One to three GEMM descriptors of one K in one launch.  Exact-f32 mode: gemm_ns (LDS-tiled) for large M, gemm16 (16-row
// tiles, split-K) otherwise.  Split-operand modes: gemm_bf for everything but the LSTM-cell / fused-argmax epilogues (greedy
// decode: matrix-vector shaped, weight-bandwidth bound, stays exact f32) and weights outside the blob.
int launch_gemm(rnnt_ctx* ctx, hipStream_t s, const GemmP* gs, int ng, int tag = TAG_NONE) {
    ProfScope prof(ctx, s, tag);
    GemmBatch gb;
    memset(&gb, 0, sizeof(gb));
    int maxM = 0, maxN = 0;
    for (int i = 0; i < ng; ++i) {
        gb.g[i] = gs[i];
        int rc = prepare_gemm(ctx, gb.g[i]);
        if (rc) return rc;
        if (gs[i].ln_g && gs[i].K != 256) return fail(ctx, RNNT_ERR_SHAPE, "LayerNorm prologue needs K=256");
        maxM = gs[i].M > maxM ? gs[i].M : maxM;
        maxN = gs[i].N > maxN ? gs[i].N : maxN;
    }
    if (maxM <= 0 || maxN <= 0) return RNNT_OK;
    const int K = gs[0].K;
    for (int i = 0; i < ng; ++i)
        if (gs[i].K != K) return fail(ctx, RNNT_ERR_SHAPE, "grouped gemm needs one K");
    const int epi0 = gs[0].epi;
    const bool dense_epi = epi0 != EPI_LSTM && epi0 != EPI_ARGMAX;
    // Stream pool: the kernel and tile are chosen as for ONE stream's rows (never the large-M forms), so that a slot's sums do not
    // depend on how many neighbours share the call.  The grids still cover all maxM rows.
    const int selM = ctx->gemm_m_cap && maxM > ctx->gemm_m_cap ? ctx->gemm_m_cap : maxM;
    if (ctx->numerics != RNNT_NUM_F32 && dense_epi && K % 32 == 0 && all_planes(gb, ng)) {
        const int nm = ctx->numerics;
        // Tile choice measured with tools/gemm_check.hip at M = 12032 (bf16x3): 64x64 tiles beat 128x128 / 128x64 on every shape
        // of the path (ffn w_2 36 vs 68 us, embed 150 vs 198 us, ffn w_1 60 vs 95 us).  Round 2 also carried 128-row tiles
        // (MT = 4): with the LayerNorm prologue they gave, rarely and run-to-run differently, four rows of bad statistics at
        // M = 12032 (the rows one statistics iteration of the workgroup's last wave covers).  The cause was not found (not
        // spills: 186 VGPRs, no scratch; not LDS size), so round 3 removed the MT = 4 instantiations and the RNNT_BF_TILE
        // override altogether (gemm_bf_body static_asserts MT <= 2): the default path never dispatched them (conv2 of a whole
        // batch runs gemm_bw), and a kernel with an unexplained race does not stay in the product.
        // (the name each branch logs is the launch form: kernel<MT,NT>, the tiles being 32 * MT rows by 32 * NT columns)
        if (gs[0].a_tanh) { launch_gemm_bf<2, 2, true>(nm, s, gb, maxM, maxN, ng); LAUNCHCHK("gemm_bf<2,2,tanh>"); }
        else if (selM >= 1024 && maxN >= 256) { launch_gemm_bf<2, 2>(nm, s, gb, maxM, maxN, ng); LAUNCHCHK("gemm_bf<2,2>"); }
        else if (maxN >= 512 || selM >= 1024) { launch_gemm_bf<1, 2>(nm, s, gb, maxM, maxN, ng); LAUNCHCHK("gemm_bf<1,2>"); }
        else { launch_gemm_bf<1, 1>(nm, s, gb, maxM, maxN, ng); LAUNCHCHK("gemm_bf<1,1>"); }
        return RNNT_OK;
    }
    if (selM >= 1024 && K % 32 == 0 && dense_epi) {
        // large M (full-context encoder, batched subsampling, joint lattice): LDS-tiled kernel, no split-K
        // (with one K block in flight, RNNT_GEMM_PD=1, the forms log names of their own)
        const bool pd1 = prefetch_depth(ctx) == 1;
        if (gs[0].a_tanh) { launch_gemm_ns<2, 2, true>(ctx, s, gb, maxM, maxN, ng); if (pd1) LAUNCHCHK("gemm_ns<2,2,tanh;pd1>"); else LAUNCHCHK("gemm_ns<2,2,tanh>"); }
        else if (maxN >= 512) { launch_gemm_ns<2, 2>(ctx, s, gb, maxM, maxN, ng); if (pd1) LAUNCHCHK("gemm_ns<2,2;pd1>"); else LAUNCHCHK("gemm_ns<2,2>"); }
        else { launch_gemm_ns<1, 2>(ctx, s, gb, maxM, maxN, ng); if (pd1) LAUNCHCHK("gemm_ns<1,2;pd1>"); else LAUNCHCHK("gemm_ns<1,2>"); }
        return RNNT_OK;
    }
    const bool wide = maxN >= 512;
    // 8 waves over K from 1024 on where K splits into eight multiples of 16; otherwise 4 (the front-end's K = n_fft or
    // roundup64(n_fft/2 + 1) is a multiple of 64 but, above 1024, often not of 128: 1088, 1600, 2112, ...)
    const int wkk = K >= 1024 && K % 128 == 0 ? 8 : 4;
    if (K % (wkk * 16) != 0) return fail(ctx, RNNT_ERR_SHAPE, "gemm16 K=%d not divisible by %d", K, wkk * 16);
    // gemm16<WK,NT>: WK waves over K, 16 rows by 16 * NT columns
    if (wide && wkk == 8) { launch_gemm16<8, 2>(s, gb, maxM, maxN, ng); LAUNCHCHK("gemm16<8,2>"); }
    else if (wide) { launch_gemm16<4, 2>(s, gb, maxM, maxN, ng); LAUNCHCHK("gemm16<4,2>"); }
    else if (wkk == 8) { launch_gemm16<8, 1>(s, gb, maxM, maxN, ng); LAUNCHCHK("gemm16<8,1>"); }
    else { launch_gemm16<4, 1>(s, gb, maxM, maxN, ng); LAUNCHCHK("gemm16<4,1>"); }
    return RNNT_OK;
}

// launch_gemm on the exact-f32 kernels whatever the context's mode (as rnnt_finalize_weights runs its derived tables).  For the two
// projections under the joint's tanh: their sum is an argument, not a product, so a split mode's RELATIVE operand error becomes an
// absolute one on tanh's linear part -- with joint.enc_ffn / pred_ffn weights 16x the seeded ones (|e + p| up to 330) the bf16 planes
// moved the argument by 1.4e-3 and the logits by 1.04e-3, over the 1e-3 bar.  (B*T + B*U) x 256 x 256 against a lattice of
// B*T*U x V x 256: the exact kernels cost nothing here.
int launch_gemm_f32(rnnt_ctx* ctx, hipStream_t s, const GemmP* gs, int ng, int tag = TAG_NONE) {
    const int nm = ctx->numerics;
    ctx->numerics = RNNT_NUM_F32;
    const int rc = launch_gemm(ctx, s, gs, ng, tag);
    ctx->numerics = nm;
    return rc;
}

inline int grid_for(long long n, int block = 256) {
    long long g = (n + block - 1) / block;
    return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}

const HostTensor* find(rnnt_ctx* ctx, const std::string& name) {
    auto it = ctx->host.find(name);
    return it == ctx->host.end() ? nullptr : &it->second;
}

// ---- descriptors of one Conformer block over rows [M = B*tq] of `x` ------------------------------------
// (ConformerEncoderLayer.forward, wenet/transformer/encoder_layer.py:188-265).  Shared by the eager per-chunk
// path (descriptors passed by value) and the wavefront path (descriptor tables in device memory).
struct LayerDescs {
    GemmP ffn1m, ffn2m, qkv[3], out, pw1, pw2, ffn1, ffn2;
    AttnP attn;
    DwP dw;
    LnP lnf;
};
struct LayerBufs { float *x, *hbuf, *qbuf, *abuf, *dbuf; };

int build_layer(rnnt_ctx* ctx, int l, int B, int tq, int T2, int kv_row0, int pos_start, int ring_pos, const int* klen_dev,
                const LayerBufs& bf, LayerDescs& d) {
    const LayerW& w = ctx->lw[l];
    const int M = B * tq;
    float* kc = ctx->kcache + (size_t)l * ctx->cfg.max_streams * ctx->tcap * D;
    float* vc = ctx->vcache + (size_t)l * ctx->cfg.max_streams * ctx->tcap * D;
    float* gr = ctx->gring + (size_t)l * ctx->cfg.max_streams * ctx->cap * D;
    float* xr = ctx->xring + (size_t)l * ctx->cfg.max_streams * ctx->cap * D;
    // x += 0.5 * FFN_macaron(LN(x))
    d.ffn1m = plain_gemm(bf.x, D, w.w1m, D, w.b1m, bf.hbuf, FF, M, FF, D, EPI_SILU);
    d.ffn1m.ln_g = w.ln_ffm_g; d.ffn1m.ln_b = w.ln_ffm_b;
    d.ffn2m = plain_gemm(bf.hbuf, FF, w.w2m, FF, w.b2m, bf.x, D, M, D, FF, EPI_RESID, 0.5f);
    d.ffn2m.R = bf.x;
    // x += linear_out(attention(LN(x))): q to a buffer, the new K/V rows appended behind the cached ones
    d.qkv[0] = plain_gemm(bf.x, D, w.wq, D, w.bq, bf.qbuf, D, M, D, D);
    d.qkv[1] = plain_gemm(bf.x, D, w.wk, D, w.bk, kc, D, M, D, D);
    d.qkv[2] = plain_gemm(bf.x, D, w.wv, D, w.bv, vc, D, M, D, D);
    for (int i = 0; i < 3; ++i) { d.qkv[i].ln_g = w.ln_mha_g; d.qkv[i].ln_b = w.ln_mha_b; }
    for (int i = 1; i < 3; ++i) {
        d.qkv[i].c_n = tq; d.qkv[i].c_s0 = (long long)ctx->tcap * D; d.qkv[i].c_r0 = kv_row0 + (T2 - tq); d.qkv[i].c_mod = BIG; d.qkv[i].c_s1 = D;
    }
    d.attn = AttnP{bf.qbuf, kc, vc, w.ptab, w.pu, w.pv, klen_dev, bf.abuf, tq, T2, kv_row0, pos_start, (long long)ctx->tcap};
    d.out = plain_gemm(bf.abuf, D, w.wo, D, w.bo, bf.x, D, M, D, D, EPI_RESID, 1.0f);
    d.out.R = bf.x;
    // x += conv_module(LN(x))
    d.pw1 = plain_gemm(bf.x, D, w.pw1, D, w.bpw1, gr, D, M, 2 * D, D, EPI_GLU);
    d.pw1.ln_g = w.ln_conv_g; d.pw1.ln_b = w.ln_conv_b;
    d.pw1.c_n = tq; d.pw1.c_s0 = (long long)ctx->cap * D; d.pw1.c_r0 = ring_pos % ctx->cap; d.pw1.c_mod = ctx->cap; d.pw1.c_s1 = D;
    d.dw = DwP{gr, w.wdw_t, w.bdw, w.bn_s, w.bn_t, bf.dbuf, bf.x, xr, B, tq, ctx->cap, ring_pos};
    d.pw2 = plain_gemm(bf.dbuf, D, w.pw2, D, w.bpw2, bf.x, D, M, D, D, EPI_RESID, 1.0f);
    d.pw2.R = bf.x;
    if (klen_dev) { d.pw2.rowlen = klen_dev; d.pw2.rowlen_n = tq; }   // full-context pass: conv-module output zero on padded frames
    // x += 0.5 * FFN(LN(x)); x = LN_final(x)
    d.ffn1 = plain_gemm(bf.x, D, w.w1, D, w.b1, bf.hbuf, FF, M, FF, D, EPI_SILU);
    d.ffn1.ln_g = w.ln_ff_g; d.ffn1.ln_b = w.ln_ff_b;
    d.ffn2 = plain_gemm(bf.hbuf, FF, w.w2, FF, w.b2, bf.x, D, M, D, FF, EPI_RESID, 0.5f);
    d.ffn2.R = bf.x;
    d.lnf = LnP{bf.x, w.ln_fin_g, w.ln_fin_b, bf.x, M, BIG, 0, 0LL, (long long)D};
    return RNNT_OK;
}

// streaming chunks (<= 4 new frames): direct-stream kernel; dynamic LDS = 4 score rows + the PV partial sums
static bool attn_stream_ok(const rnnt_ctx* ctx, int tq, int T2) {
    return ctx->attn_stream && tq <= 4 && T2 >= 1 && T2 <= 4096;
}
static int attn_t2cap(int T2) { return (T2 + 63) / 64 * 64; }
static size_t attn_stream_lds(int t2cap) { return (size_t)(4 * t2cap + 16 * 4 * RNNT_DK) * sizeof(float); }

// The LDS-tiled attention kernels (rel_attention, rel_attention_tab, rel_attention_pool): KERNEL<NQ> with NQ query rows per wave chosen
// by the most new frames `tq` of anything the launch serves, on the grid (gx, query tiles, gz); the rest are the kernel's arguments.
static int attn_nq(int tq) { return tq <= 4 ? 1 : (tq <= 8 ? 2 : 4); }
#define LAUNCH_ATTN_TILED(KERNEL, s, gx, tq, gz, ...)                                                  \
    do {                                                                                               \
        const int nq_ = attn_nq(tq);                                                                   \
        const dim3 grid_(gx, ((tq) + 4 * nq_ - 1) / (4 * nq_), gz);                                    \
        if (nq_ == 1) { hipLaunchKernelGGL(KERNEL<1>, grid_, dim3(256), 0, s, __VA_ARGS__); LAUNCHCHK(#KERNEL "<1>"); }      \
        else if (nq_ == 2) { hipLaunchKernelGGL(KERNEL<2>, grid_, dim3(256), 0, s, __VA_ARGS__); LAUNCHCHK(#KERNEL "<2>"); } \
        else { hipLaunchKernelGGL(KERNEL<4>, grid_, dim3(256), 0, s, __VA_ARGS__); LAUNCHCHK(#KERNEL "<4>"); }               \
    } while (0)

int launch_attn(rnnt_ctx* ctx, hipStream_t s, const AttnP& a, int B) {
    ProfScope prof(ctx, s, TAG_ATTN);
    if (attn_stream_ok(ctx, a.tq, a.T2)) {
        const int cap = attn_t2cap(a.T2);
        hipLaunchKernelGGL(rel_attention_stream, dim3(B * RNNT_H), dim3(256), attn_stream_lds(cap), s, a, cap);
        LAUNCHCHK("rel_attention_stream");
        return RNNT_OK;
    }
    LAUNCH_ATTN_TILED(rel_attention, s, B * RNNT_H, a.tq, 1, a);
    return RNNT_OK;
}
int launch_dw(rnnt_ctx* ctx, hipStream_t s, const DwP& d) {
    ProfScope prof(ctx, s, TAG_DWCONV);
    hipLaunchKernelGGL(dwconv_bn_silu, dim3(grid_for((long long)d.B * d.tq * D)), dim3(256), 0, s, d);
    LAUNCHCHK("dwconv_bn_silu");
    return RNNT_OK;
}
int launch_ln(rnnt_ctx* ctx, hipStream_t s, const LnP& p) {
    hipLaunchKernelGGL(layer_norm, dim3((p.M + 3) / 4), dim3(256), 0, s, p);
    LAUNCHCHK("layer_norm");
    return RNNT_OK;
}

int run_layer(rnnt_ctx* ctx, hipStream_t s, int l, int B, int tq, int T2, int kv_row0, int pos_start, int ring_pos,
              const int* klen_dev) {
    LayerDescs d;
    LayerBufs bf{ctx->x, ctx->hbuf, ctx->qbuf, ctx->abuf, ctx->dbuf};
    int rc = build_layer(ctx, l, B, tq, T2, kv_row0, pos_start, ring_pos, klen_dev, bf, d);
    if (rc) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn1m, 1, TAG_FFN1))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn2m, 1, TAG_FFN2))) return rc;
    if ((rc = launch_gemm(ctx, s, d.qkv, 3, TAG_QKV))) return rc;
    if ((rc = launch_attn(ctx, s, d.attn, B))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.out, 1, TAG_ATTN_OUT))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.pw1, 1, TAG_PW1))) return rc;
    if ((rc = launch_dw(ctx, s, d.dw))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.pw2, 1, TAG_PW2))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn1, 1, TAG_FFN1))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn2, 1, TAG_FFN2))) return rc;
    return launch_ln(ctx, s, d.lnf);
}

static bool conv2_bw_on(const rnnt_ctx* ctx) { return ctx->conv2_bw != 0; }
// conv2 of M rows forms its conv1 operand itself (gemm_bw_c1): no conv1 launch, no y1 slab.  The same condition as gemm_bw's, plus
// the per-context knob; the caller must also allow it (fuse_ok: the layer-major schedule's main classes).
static bool conv2_fused(const rnnt_ctx* ctx, long long M) {
    return ctx->conv1_fuse && ctx->numerics != RNNT_NUM_F32 && conv2_bw_on(ctx) && ctx->conv2_wp && M >= 32768 && M < (1ll << 31);
}
// Conv2dSubsampling4 (+ x16) (subsampling.py:203-228) of `nc` equal-length chunks of every stream at once:
// virtual stream v = c*B + b; output rows (v, r) -> xout[(v*tq + r)][256].  starts_dev == null: one chunk at 0.
// out_cn > 0 (layer-major encoder): virtual streams in stream-major order (v = b*nc + c) and output row m -> xout row
// (m / out_cn)*out_rows + (m % out_cn) + out_r0, i.e. the nc chunks' frames of stream b land at frames out_r0.. of its utterance.
// fuse_ok: y1 may be null where conv2_fused(ctx, nc * B * sub_len(T) * RNNT_FSUB) holds.
int run_subsample(rnnt_ctx* ctx, hipStream_t s, const float* fbank, int B, int Tstride, int T, const int* starts_dev, int nc,
                  float* y1, float* y2, float* xout, int out_cn = 0, int out_rows = 0, int out_r0 = 0, bool minor = false, bool fuse_ok = false) {
    // minor: not the call's main chunk class -- its launches are profiled under their own tags, so that a site's average launch time
    // is the average of launches of ONE kind (the bench's roofline is checked against the kernel's rocprof average)
    const int tag1 = minor ? TAG_CONV1_MINOR : TAG_CONV1, tag2 = minor ? TAG_CONV2_MINOR : TAG_CONV2, tag3 = minor ? TAG_EMBED_MINOR : TAG_EMBED;
    const int t1 = sub1_len(T), tq = sub_len(T);
    const int VB = nc * B;
    int rc;
    const bool fused = fuse_ok && conv2_fused(ctx, (long long)VB * tq * RNNT_FSUB);
    if (!fused) {
        if (!y1) return fail(ctx, RNNT_ERR_STATE, "run_subsample: no conv1 slab");
        ProfScope prof(ctx, s, tag1);
        if (ctx->conv1_rows && !ctx->gemm_m_cap && (long long)VB * ((t1 + C1_TB - 1) / C1_TB) >= 256) {   // enough (stream, 8-row block) pairs to fill the chip: coalesced row stores
            hipLaunchKernelGGL(conv1_relu_rows, dim3(VB, (t1 + C1_TB - 1) / C1_TB), dim3(256), 0, s, fbank, ctx->conv1_wt, ctx->conv1_b, y1, B, Tstride, t1,
                               starts_dev, nc, out_cn > 0 ? 1 : 0);
            LAUNCHCHK("conv1_relu_rows");
        } else {
            hipLaunchKernelGGL(conv1_relu, dim3(grid_for((long long)VB * t1 * RNNT_F1 * D)), dim3(256), 0, s, fbank, ctx->conv1_wt, ctx->conv1_b,
                               y1, B, Tstride, t1, starts_dev, nc, out_cn > 0 ? 1 : 0);
            LAUNCHCHK("conv1_relu");
        }
    }
    // conv2 as implicit GEMM: rows (v,t',f), K = (kh, kw, ci) = 3 segments of 768 contiguous floats of y1
    GemmP g = plain_gemm(y1, 0, ctx->conv2_w, 2304, ctx->conv2_b, y2, D, VB * tq * RNNT_FSUB, D, 2304, EPI_RELU);
    g.a_n1 = tq * RNNT_FSUB; g.a_n2 = RNNT_FSUB;
    g.a_s0 = (long long)t1 * RNNT_F1 * D; g.a_s1 = 2LL * RNNT_F1 * D; g.a_s2 = 2LL * D;
    g.a_seg = 768; g.a_seg_stride = (long long)RNNT_F1 * D;
    const int conv2_lds = ctx->conv2_lds;
    const bool conv2_bw = conv2_bw_on(ctx);
    // gemm_bw / gemm_bw_c1 of the numerics mode on `grid`, 8 waves (two per SIMD) or 4 (RNNT_BW_NW=4, same bits: test_kernel_forms.py)
    const bool nw8 = ctx->bw_nw == 8;
#define BW_LAUNCH_NUM(KERNEL, NUM_, ...) { if (nw8) hipLaunchKernelGGL((KERNEL<NUM_, 8>), grid, dim3(512), 0, s, __VA_ARGS__); \
                                           else hipLaunchKernelGGL((KERNEL<NUM_, 4>), grid, dim3(256), 0, s, __VA_ARGS__); }
#define BW_LAUNCH(KERNEL, ...)                                                                         \
    switch (ctx->numerics) {                                                                           \
        case RNNT_NUM_BF16: BW_LAUNCH_NUM(KERNEL, RNNT_NUM_BF16, __VA_ARGS__) break;                   \
        case RNNT_NUM_F16X3: BW_LAUNCH_NUM(KERNEL, RNNT_NUM_F16X3, __VA_ARGS__) break;                 \
        default: BW_LAUNCH_NUM(KERNEL, RNNT_NUM_BF16X3, __VA_ARGS__) break;                            \
    }                                                                                                  \
    LAUNCHERR(#KERNEL)   /* the call site counts the launch under its form name, KERNEL<waves> */
    if (fused) {
        // the same tiles with the conv1 operand formed from the fbank in the tile staging (gemm_bw_c1): g.A stays null
        ProfScope prof(ctx, s, tag2);
        g.A = nullptr;
        if ((rc = prepare_gemm(ctx, g))) return rc;
        const dim3 grid((g.M + 127) / 128);
        const Conv1Src src{fbank, ctx->conv1_wt, ctx->conv1_b, starts_dev, B, Tstride, nc, out_cn > 0 ? 1 : 0};
        BW_LAUNCH(gemm_bw_c1, g, ctx->conv2_wp, src);
        if (nw8) LAUNCHCHK("gemm_bw_c1<8>"); else LAUNCHCHK("gemm_bw_c1<4>");
    } else if (ctx->numerics != RNNT_NUM_F32 && conv2_bw && ctx->conv2_wp && g.M >= 32768 && !ctx->gemm_m_cap) {
        // whole-utterance slab: 128 x 256 tiles, weights streamed from L2 in fragment order, A rows four k-steps ahead (gemm_bw)
        ProfScope prof(ctx, s, tag2);
        if ((rc = prepare_gemm(ctx, g))) return rc;
        const dim3 grid((g.M + 127) / 128);
        BW_LAUNCH(gemm_bw, g, ctx->conv2_wp);
        if (nw8) LAUNCHCHK("gemm_bw<8>"); else LAUNCHCHK("gemm_bw<4>");
#undef BW_LAUNCH
#undef BW_LAUNCH_NUM
    } else if (ctx->numerics != RNNT_NUM_F32) {
        if ((rc = launch_gemm(ctx, s, &g, 1, tag2))) return rc;
    } else if (conv2_lds && g.M >= 2048 && !ctx->gemm_m_cap) {   // big M: LDS-tiled 64x64 tiles (full-line operand staging); N = 256 -> 4 column tiles
        ProfScope prof(ctx, s, tag2);
        GemmBatch gb;
        memset(&gb, 0, sizeof(gb));
        gb.g[0] = g;
        if ((rc = prepare_gemm(ctx, gb.g[0]))) return rc;
        const bool pd1 = prefetch_depth(ctx) == 1;
        if (conv2_lds == 2 && nc > 1) { launch_gemm_ns<2, 2, false, true>(ctx, s, gb, g.M, g.N, 1); if (pd1) LAUNCHCHK("gemm_ns<2,2,nt;pd1>"); else LAUNCHCHK("gemm_ns<2,2,nt>"); }   // experiment: non-temporal A
        else { launch_gemm_ns<2, 2>(ctx, s, gb, g.M, g.N, 1); if (pd1) LAUNCHCHK("gemm_ns<2,2;pd1>"); else LAUNCHCHK("gemm_ns<2,2>"); }
    } else if ((rc = launch_gemm(ctx, s, &g, 1, tag2))) return rc;
    // Linear(4864 -> 256) * sqrt(256); y2 is [VB*t', f*256 + c] (weight columns permuted to match)
    GemmP go = plain_gemm(y2, RNNT_FSUB * D, ctx->emb_w, RNNT_FSUB * D, ctx->emb_b, xout, D, VB * tq, D, RNNT_FSUB * D, EPI_SCALE, 16.0f);
    if (out_cn > 0) { go.c_n = out_cn; go.c_s0 = (long long)out_rows * D; go.c_r0 = out_r0; go.c_mod = BIG; go.c_s1 = D; }
    return launch_gemm(ctx, s, &go, 1, tag3);
}

// ---- fused Conformer-block kernels (rnnt_fused.hip.h) ---------------------------------------------------------------------
template <int NUM>
size_t fuse_lds(int MT, bool back) {
    const size_t R = 16 * MT, opb = FuseCfg<NUM>::OPB;
    return back ? R * 1024 + R * opb + R * 1024 + sizeof(FuseRows) : R * 1024 + 2 * R * opb + sizeof(FuseRows);
}
template <int NUM, int MT>
int launch_fused_t(rnnt_ctx* ctx, hipStream_t s, bool back, const FuseItem* tab, int n_items, int n_groups, int S, int B) {
    const size_t lds = fuse_lds<NUM>(MT, back);
    int rc_attr;
    const dim3 grid((unsigned)((n_items + 7) / 8 * 8 * n_groups));
    if (back) {
        if ((rc_attr = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&block_back<NUM, MT>), lds))) return rc_attr;
        hipLaunchKernelGGL((block_back<NUM, MT>), grid, dim3(FUSE_THREADS), lds, s, ctx->layers_dev, tab, ctx->wf_x, n_items, n_groups, S, B, ctx->cap);
        if (MT == 1) LAUNCHCHK("block_back<1>"); else if (MT == 2) LAUNCHCHK("block_back<2>"); else LAUNCHCHK("block_back<3>");
    } else {
        if ((rc_attr = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&block_front<NUM, MT>), lds))) return rc_attr;
        hipLaunchKernelGGL((block_front<NUM, MT>), grid, dim3(FUSE_THREADS), lds, s, ctx->layers_dev, tab, ctx->wf_x, n_items, n_groups, S, B, (long long)ctx->tcap);
        if (MT == 1) LAUNCHCHK("block_front<1>"); else if (MT == 2) LAUNCHCHK("block_front<2>"); else LAUNCHCHK("block_front<3>");
    }
    return RNNT_OK;
}
template <int NUM>
int launch_fused_n(rnnt_ctx* ctx, hipStream_t s, bool back, const FuseItem* tab, int n_items, int n_groups, int S, int B, int MT) {
    switch (MT) {
        case 1: return launch_fused_t<NUM, 1>(ctx, s, back, tab, n_items, n_groups, S, B);
        case 2: return launch_fused_t<NUM, 2>(ctx, s, back, tab, n_items, n_groups, S, B);
        default: return launch_fused_t<NUM, 3>(ctx, s, back, tab, n_items, n_groups, S, B);
    }
}
// one half block for all items of a stage; maxnf = most frames per stream of any item
int launch_fused(rnnt_ctx* ctx, hipStream_t s, bool back, const FuseItem* tab, int n_items, int maxnf, int B, int tag) {
    ProfScope prof(ctx, s, tag);
    int S = FUSE_ROWS / maxnf;
    if (S > B) S = B;
    if (S < 1) return fail(ctx, RNNT_ERR_SHAPE, "fused block: %d frames per stream exceed the %d-row tile", maxnf, FUSE_ROWS);
    const int n_groups = (B + S - 1) / S, MT = (S * maxnf + 15) / 16;
    switch (ctx->numerics) {
        case RNNT_NUM_BF16X3: return launch_fused_n<RNNT_NUM_BF16X3>(ctx, s, back, tab, n_items, n_groups, S, B, MT);
        case RNNT_NUM_BF16: return launch_fused_n<RNNT_NUM_BF16>(ctx, s, back, tab, n_items, n_groups, S, B, MT);
        case RNNT_NUM_F16X3: return launch_fused_n<RNNT_NUM_F16X3>(ctx, s, back, tab, n_items, n_groups, S, B, MT);
        default: return launch_fused_n<RNNT_NUM_F32>(ctx, s, back, tab, n_items, n_groups, S, B, MT);
    }
}

template <int WK, int MT, int NT>
void launch_gemm16_tab(hipStream_t s, const GemmP* tab, int n, int maxM, int maxN) {
    dim3 grid((maxN + 16 * NT - 1) / (16 * NT), (maxM + 16 * MT - 1) / (16 * MT), n);
    hipLaunchKernelGGL((gemm16_tab<WK, MT, NT>), grid, dim3(64 * WK), 0, s, tab);
}
// n descriptors of one shape class (same N, K) in device memory.  Tile choice: with n >= 6 groups there are enough
// workgroups to spend registers on operand reuse (64x64 / 32x64 tiles); few groups keep the 16-row tiles.
int launch_gemm_tab(rnnt_ctx* ctx, hipStream_t s, const GemmP* tab_dev, int n, int maxM, int N, int K, int tag) {
    ProfScope prof(ctx, s, tag);
    const int ns_mode = ctx->gemm_ns, ns_min = ctx->ns_min_groups;   // pipeline fill/drain stages have few pairs
    // XCDs per descriptor of the 1-D grids (see gemm_ns_tab): the largest split that keeps the groups balanced
    const int x_env = ctx->xcd_x;
    auto pick_x = [&](int ntn) {
        if (x_env == 1 || x_env == 2 || x_env == 4 || x_env == 8) return x_env;
        for (int X = 2; X < 8; X *= 2)
            if (n % (8 / X) == 0 && ntn % X == 0) return X;
        return 8;
    };
    auto grid_for_tab = [&](int ntn, int ntm, int X) {
        const int dpg = (n + 8 / X - 1) / (8 / X), cpx = (ntn + X - 1) / X;
        return dim3(8 * dpg * cpx * ntm);
    };
    const int ntn = N >= 512 ? (N + 63) / 64 : (N + 31) / 32, ntm = (maxM + 31) / 32, X = pick_x(ntn);   // 32-row tiles, 64 or 32 columns
    if (ctx->numerics != RNNT_NUM_F32 && K % 32 == 0) {   // split-operand modes: every stage GEMM on the 16-bit MFMA kernel
#define BF_TAB(MT_, NT_)                                                                                                   \
    switch (ctx->numerics) {                                                                                               \
        case RNNT_NUM_BF16: hipLaunchKernelGGL((gemm_bf_tab<1, false, MT_, NT_>), grid_for_tab(ntn, ntm, X), dim3(256), 0, s, tab_dev, n, ntn, ntm, X); break; \
        case RNNT_NUM_F16X3: hipLaunchKernelGGL((gemm_bf_tab<2, true, MT_, NT_>), grid_for_tab(ntn, ntm, X), dim3(256), 0, s, tab_dev, n, ntn, ntm, X); break; \
        default: hipLaunchKernelGGL((gemm_bf_tab<2, false, MT_, NT_>), grid_for_tab(ntn, ntm, X), dim3(256), 0, s, tab_dev, n, ntn, ntm, X); break; \
    }
        if (N >= 512) { BF_TAB(1, 2) LAUNCHCHK("gemm_bf_tab<1,2>"); } else { BF_TAB(1, 1) LAUNCHCHK("gemm_bf_tab<1,1>"); }
#undef BF_TAB
        return RNNT_OK;
    }
    if (ns_mode && n >= ns_min && K % 32 == 0) {   // enough groups: no split-K, epilogue from registers
        // tile choice from tools/microbench2.hip (12 groups x 192 rows): the kernel is occupancy/latency-bound, so the
        // narrow shapes want many small workgroups; only K = 1024 profits from 64-deep K blocks (half the barriers)
#define NS_TAB(MT_, NT_, BK_)                                                                                              \
    switch (prefetch_depth(ctx)) {                                                                                         \
        case 1: hipLaunchKernelGGL((gemm_ns_tab<MT_, NT_, BK_, 1>), grid_for_tab(ntn, ntm, X), dim3(256), 0, s, tab_dev, n, ntn, ntm, X); break; \
        default: hipLaunchKernelGGL((gemm_ns_tab<MT_, NT_, BK_, 2>), grid_for_tab(ntn, ntm, X), dim3(256), 0, s, tab_dev, n, ntn, ntm, X); break; \
    }
        const bool pd1 = prefetch_depth(ctx) == 1;
        if (N >= 512) { NS_TAB(1, 2, 32) if (pd1) LAUNCHCHK("gemm_ns_tab<1,2,32;pd1>"); else LAUNCHCHK("gemm_ns_tab<1,2,32>"); }        // ffn1 / pointwise_conv1: 32x64 tiles
        else if (K >= 1024) { NS_TAB(1, 1, 64) if (pd1) LAUNCHCHK("gemm_ns_tab<1,1,64;pd1>"); else LAUNCHCHK("gemm_ns_tab<1,1,64>"); }  // ffn2: 32x32 tiles, BK = 64
        else { NS_TAB(1, 1, 32) if (pd1) LAUNCHCHK("gemm_ns_tab<1,1,32;pd1>"); else LAUNCHCHK("gemm_ns_tab<1,1,32>"); }                 // q/k/v, linear_out, pointwise_conv2: 32x32 tiles
#undef NS_TAB
        return RNNT_OK;
    }
    const int wk = K >= 1024 ? 8 : 4;
    if (K % (wk * 16) != 0) return fail(ctx, RNNT_ERR_SHAPE, "gemm16 K=%d not divisible by %d", K, wk * 16);
    const long long out = (long long)n * maxM * N;
    // gemm16_tab<WK,MT,NT>: WK waves over K, 16 * MT rows by 16 * NT columns
    if (out >= 256ll * 64 * 64 * 2 && wk == 4) { launch_gemm16_tab<4, 4, 4>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<4,4,4>"); }
    else if (out >= 256ll * 32 * 64 && wk == 4) { launch_gemm16_tab<4, 2, 4>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<4,2,4>"); }
    else if (out >= 256ll * 32 * 64 && wk == 8) { launch_gemm16_tab<8, 2, 4>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<8,2,4>"); }
    else if (N >= 512 && wk == 8) { launch_gemm16_tab<8, 1, 2>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<8,1,2>"); }
    else if (N >= 512) { launch_gemm16_tab<4, 1, 2>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<4,1,2>"); }
    else if (wk == 8) { launch_gemm16_tab<8, 1, 1>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<8,1,1>"); }
    else { launch_gemm16_tab<4, 1, 1>(s, tab_dev, n, maxM, N); LAUNCHCHK("gemm16_tab<4,1,1>"); }
    return RNNT_OK;
}

// The encoder's last two launches for a chunk: after_norm of rows x [B * tq] into frames [fpos, fpos + tq) of every stream's frame
// buffer, then the joint's encoder projection of those frames.  ln_prologue (a greedy decode reads only enc_proj): after_norm runs in
// the projection's LayerNorm prologue instead and the normalised frames are not materialised.
int emit_frames(rnnt_ctx* ctx, hipStream_t s, const float* x, int B, int tq, int fpos, bool ln_prologue = false) {
    const long long fs = (long long)ctx->fstride * D;
    int rc;
    if (!ln_prologue && (rc = launch_ln(ctx, s, LnP{x, ctx->after_g, ctx->after_b, ctx->encbuf, B * tq, tq, fpos, fs, (long long)D}))) return rc;
    GemmP g = plain_gemm(ln_prologue ? x : ctx->encbuf + (size_t)fpos * D, D, ctx->wenc, D, ctx->benc, ctx->encp, D, B * tq, D, D);
    if (ln_prologue) { g.ln_g = ctx->after_g; g.ln_b = ctx->after_b; }
    else { g.a_n1 = tq; g.a_n2 = tq; g.a_s0 = fs; g.a_s1 = 0; g.a_s2 = D; }
    g.c_n = tq; g.c_s0 = fs; g.c_r0 = fpos; g.c_mod = BIG; g.c_s1 = D;
    return launch_gemm(ctx, s, &g, 1, TAG_ENC_PROJ);
}

// ---- per-slot beam state of the stream pool (rnnt_pool_chunk_beam; kernels in rnnt_beam.hip.h) --------------------------------------
BeamPoolP pool_beam_params(const rnnt_ctx* ctx) {
    BeamPoolP q;
    memset(&q, 0, sizeof(q));
    q.pool[0] = ctx->ps_pool[0]; q.pool[1] = ctx->ps_pool[1];
    q.tk = ctx->ps_tok; q.len = ctx->ps_len; q.sc = ctx->ps_sc; q.hs = ctx->ps_hs; q.nh = ctx->ps_nh;
    q.rows = ctx->max_rows; q.W = ctx->cfg.max_beam; q.lcap = ctx->cfg.max_tokens; q.fstride = ctx->fstride;
    return q;
}

// one empty hypothesis in buffer set 0 for slots [slot0, slot0 + n); no-op until the state is allocated (pool_beam_alloc resets all)
int pool_beam_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    if (!ctx->ps_nh) return RNNT_OK;
    hipLaunchKernelGGL(beam_slot_reset, dim3(n), dim3(256), 0, s, pool_beam_params(ctx), slot0, ctx->cfg.n_steps + 1);
    LAUNCHCHK("beam_slot_reset");
    for (int b = slot0; b < slot0 + n; ++b) { ctx->slot[b].beam_cur = 0; ctx->slot[b].beam_lbound = 0; }
    return RNNT_OK;
}

// ---- per-slot CTC prefix search of the stream pool (api_pool_ctc.hip.inc; kernels in rnnt_ctc_prefix.hip.h) ---------------------------
// the uploaded tables of rnnt_context_set as the kernels take them
CpGraph ctx_graph_dev(const rnnt_ctx* ctx) {
    const size_t n = ctx->cg.token.size(), m = ctx->cg.ctok.size();
    CpGraph g;
    g.fail = ctx->cg_i; g.off = ctx->cg_i + n; g.ctok = ctx->cg_i + 2 * n + 1; g.cid = g.ctok + m;
    g.tscore = ctx->cg_d; g.nscore = ctx->cg_d + n; g.oscore = ctx->cg_d + 2 * n;
    return g;
}

// the uploaded tables of rnnt_ngram_set as the kernels take them
NgTables ngram_dev(const rnnt_ctx* ctx) {
    const size_t n = ctx->ng.fail.size(), m = ctx->ng.ctok.size();
    NgTables g = ctx->ng.tables();
    g.fail = ctx->ng_i; g.off = ctx->ng_i + n; g.ctok = ctx->ng_i + 2 * n + 1; g.cid = g.ctok + m; g.root = g.cid + m;
    g.W = ctx->ng_d; g.B = ctx->ng_d + n;
    return g;
}

// The block of a CTC prefix search's results that is downloaded in one copy, on the device or in its host copy (the one-call search
// with its B, a slot's read with B = 1): n_hyp [B] | lens [R] | tokens [R][lcap] | times [R][lcap]; total: its ints.
struct CpOut { int *nh, *len, *tok, *time; size_t total; };
CpOut cp_out(Carve<int>& c, size_t B, size_t R, size_t lcap) {
    CpOut o;
    const size_t at = c.off;
    o.nh = c.take(B);
    o.len = c.take(R);
    o.tok = c.take(R * lcap);
    o.time = c.take(R * lcap);
    o.total = c.off - at;
    return o;
}
// its host copy h (and the scores | context scores | with ng_scores the n-gram scores, od [2 or 3][R]) into the caller's arrays: H >= R
// rows of cap_tokens, zero beyond what was found
void cp_out_copy(const CpOut& h, const double* od, size_t B, size_t R, size_t lcap, size_t H, size_t cap_tokens, int32_t* n_hyp, int32_t* lens,
                 int32_t* tokens, int32_t* times, double* scores, double* ctx_scores, double* ng_scores = nullptr) {
    if (ng_scores) { std::fill(ng_scores, ng_scores + H, 0.0); memcpy(ng_scores, od + 2 * R, R * sizeof(double)); }
    memcpy(n_hyp, h.nh, B * sizeof(int));
    std::fill(lens, lens + H, 0);
    std::fill(scores, scores + H, 0.0);
    std::fill(tokens, tokens + H * cap_tokens, 0);
    std::fill(times, times + H * cap_tokens, 0);
    memcpy(lens, h.len, R * sizeof(int));
    memcpy(scores, od, R * sizeof(double));
    if (ctx_scores) { std::fill(ctx_scores, ctx_scores + H, 0.0); memcpy(ctx_scores, od + R, R * sizeof(double)); }
    const size_t ncopy = std::min(lcap, cap_tokens);
    for (size_t r = 0; r < R; ++r) {
        memcpy(tokens + r * cap_tokens, h.tok + r * lcap, ncopy * sizeof(int));
        memcpy(times + r * cap_tokens, h.time + r * lcap, ncopy * sizeof(int));
    }
}

// the start hypothesis for slots [slot0, slot0 + n): the host record always, the device record once it exists (pool_ctc_alloc resets all)
int pool_ctc_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    for (int b = slot0; b < slot0 + n; ++b) ctx->slot[b].ctc = SearchSlot{};
    if (!ctx->pc_state) return RNNT_OK;
    hipLaunchKernelGGL(ctc_prefix_slot_reset, dim3(n), dim3(64), 0, s, ctx->pc_state.p, slot0);
    LAUNCHCHK("ctc_prefix_slot_reset");
    return RNNT_OK;
}

// ---- per-slot transducer prefix beam search of the stream pool (api_pool_prefix.hip.inc; kernels in rnnt_prefix.hip.h) -----------------
PrefixPoolP pool_prefix_params(const rnnt_ctx* ctx) {
    PrefixPoolP q;
    memset(&q, 0, sizeof(q));
    for (int t = 0; t < 2; ++t) { q.pool[t] = ctx->pp_pool[t]; q.tk[t] = ctx->pp_tk[t]; q.len[t] = ctx->pp_len[t]; q.sc[t] = ctx->pp_sc[t]; q.hs[t] = ctx->pp_hs[t]; q.cst[t] = ctx->pp_cst[t]; q.cs[t] = ctx->pp_cs[t]; q.nst[t] = ctx->pp_nst[t]; q.ns[t] = ctx->pp_ns[t]; }
    q.nh = ctx->pp_nh;
    return q;
}

// The block prefix_pack / prefix_pack_pool write and one copy downloads, on the device or in its host copy (the one-call search with
// its B, a slot's read with B = 1): scores [R] | context scores [R] | n-gram scores [R] as doubles, the ints n_hyp [B] | lens [R] |
// tokens [R][lcap], and with_states the floats h [R][256] | c [R][256].  bytes: its size.
struct PrefixOut { double *sc, *cs, *ns; int *nh, *len, *tk; float *h, *c; size_t bytes; };
PrefixOut prefix_out(double* base, size_t B, size_t R, size_t lcap, bool with_states) {
    Carve<char> b{reinterpret_cast<char*>(base)};
    auto take = [&](auto*& q, size_t n) { q = reinterpret_cast<std::remove_reference_t<decltype(q)>>(b.take(n * sizeof(*q))); };
    PrefixOut o;
    take(o.sc, R);
    take(o.cs, R);
    take(o.ns, R);
    take(o.nh, B);
    take(o.len, R);
    take(o.tk, R * lcap);
    take(o.h, with_states ? R * D : 0);
    take(o.c, with_states ? R * D : 0);
    o.bytes = b.off;
    return o;
}
// its host copy into the caller's arrays (rows of cap_tokens; a row's tokens up to its length)
void prefix_out_copy(const PrefixOut& o, size_t R, size_t lcap, size_t cap_tokens, int32_t* lens, int32_t* tokens, double* scores, double* ctx_scores,
                     double* ng_scores, float* h, float* c) {
    memcpy(lens, o.len, R * sizeof(int));
    memcpy(scores, o.sc, R * sizeof(double));
    if (ctx_scores) memcpy(ctx_scores, o.cs, R * sizeof(double));
    if (ng_scores) memcpy(ng_scores, o.ns, R * sizeof(double));
    for (size_t r = 0; r < R; ++r) memcpy(tokens + r * cap_tokens, o.tk + r * lcap, (size_t)o.len[r] * sizeof(int));
    if (h) { memcpy(h, o.h, R * D * sizeof(float)); memcpy(c, o.c, R * D * sizeof(float)); }
}

// the start hypothesis [blank] for slots [slot0, slot0 + n): the host record always, the device rows once they exist (pool_prefix_alloc resets all)
int pool_prefix_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    for (int b = slot0; b < slot0 + n; ++b) { ctx->slot[b].prefix = SearchSlot{}; ctx->slot[b].prefix_cur = 0; }
    if (!ctx->pp_nh) return RNNT_OK;
    hipLaunchKernelGGL(prefix_init_pool, dim3(n), dim3(256), 0, s, pool_prefix_params(ctx), slot0, ctx->cfg.max_cache_frames + 1, ctx->cfg.blank_id);
    LAUNCHCHK("prefix_init_pool");
    return RNNT_OK;
}

// ---- per-slot streaming front-end of the stream pool (api_pool_wave.hip.inc; kernels in rnnt_frontend.hip.h) ---------------------------
// a fresh utterance for slots [slot0, slot0 + n): host records only -- a fresh slot's carry is empty, so the device carry needs no reset
void pool_wave_reset(rnnt_ctx* ctx, int slot0, int n) {
    for (int b = slot0; b < slot0 + n; ++b) ctx->slot[b].wave = WvSlot{};
}

// ---- per-slot encoder-frame history of the stream pool (api_pool_hist.hip.inc; kernels in rnnt_encoder.hip.h) ----------------------------
// flag and length of slots [slot0, slot0 + n) cleared, on the host and (once the tables exist) on the device; buffers stay
int pool_hist_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    for (int b = slot0; b < slot0 + n; ++b) ctx->slot[b].hist = HsSlot{};
    if (!ctx->hs_len) return RNNT_OK;
    hipLaunchKernelGGL(pool_hist_set, dim3((n + 63) / 64), dim3(64), 0, s, ctx->hs_ptr.p, ctx->hs_len.p, slot0, n, (float*)nullptr);
    LAUNCHCHK("pool_hist_set");
    return RNNT_OK;
}

// with the other slot checks of a pool call: a kept slot whose history cannot take tq more rows refuses the call
int pool_hist_check(rnnt_ctx* ctx, const char* fn, int slot, int tq) {
    const HsSlot& h = ctx->slot[slot].hist;
    if (h.keep && h.len + tq > ctx->cfg.max_cache_frames)
        return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: kept frames %d + %d exceed max_cache_frames %d", fn, slot, h.len, tq, ctx->cfg.max_cache_frames);
    return RNNT_OK;
}

// after the call's after_norm: one launch, and only when a listed slot keeps frames
int pool_hist_append_rows(rnnt_ctx* ctx, hipStream_t s, int n, const int32_t* slots_host, const int* slots_dev, int tq) {
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!ctx->slot[slots_host[i]].hist.keep) continue;
        ctx->slot[slots_host[i]].hist.len += tq;
        any = true;
    }
    if (!any) return RNNT_OK;
    hipLaunchKernelGGL(pool_hist_append, dim3(n), dim3(256), 0, s, ctx->x.p, slots_dev, ctx->hs_ptr.p, ctx->hs_len.p, tq);
    LAUNCHCHK("pool_hist_append");
    return RNNT_OK;
}

// ---- per-slot endpoint detection of the stream pool (api_pool_endpoint.hip.inc; kernels in rnnt_endpoint.hip.h) --------------------------
// what rnnt_stream_endpoint and rnnt_endpoint_scan_host accept, and the one float both sides compare against
bool endpoint_config_ok(const rnnt_endpoint_config* c) {
    return c->blank_threshold > 0.f && c->blank_threshold < 1.f && c->min_speech_frames >= 0 && c->rule1_trailing >= 0 && c->rule2_trailing >= 0 &&
           c->rule3_frames >= 0;
}
float endpoint_log_thr(const rnnt_endpoint_config* c) { return (float)log((double)c->blank_threshold); }

// the on flag of slots [slot0, slot0 + n) cleared, on the host and -- when one of them was on -- on the device (one launch)
int pool_endpoint_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    bool any = false;
    for (int b = slot0; b < slot0 + n; ++b) { any = any || ctx->slot[b].ep; ctx->slot[b].ep = 0; }
    if (!any) return RNNT_OK;
    hipLaunchKernelGGL(pool_endpoint_set, dim3((n + 63) / 64), dim3(64), 0, s, ctx->ep_cfg.p, ctx->ep_state.p, slot0, n, EpCfg{});
    LAUNCHCHK("pool_endpoint_set");
    return RNNT_OK;
}

// t compact rows per active row at src advance the listed endpoint slots: one launch, and only when a listed slot has endpointing on
int pool_endpoint_rows(rnnt_ctx* ctx, hipStream_t s, int n, const int32_t* slots_host, const int* slots_dev, const float* src, int t) {
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || ctx->slot[slots_host[i]].ep;
    if (!any) return RNNT_OK;
    hipLaunchKernelGGL(pool_endpoint, dim3(n), dim3(EP_THREADS), 0, s, src, slots_dev, ctx->ep_cfg.p, ctx->ep_state.p, t, ctx->wctc, ctx->bctc, ctx->cfg.vocab_size,
                       ctx->cfg.blank_id);
    LAUNCHCHK("pool_endpoint");
    return RNNT_OK;
}

// ---- what the per-slot forms share ------------------------------------------------------------------------------------------------------
// every per-slot state of slots [slot0, slot0 + n) fresh (rnnt_stream_open: one slot; rnnt_streams_reset: all); the six write
// disjoint buffers, so this one order serves both
int pool_slot_reset(rnnt_ctx* ctx, hipStream_t s, int slot0, int n) {
    int rc;
    for (int b = slot0; b < slot0 + n; ++b) ctx->slot[b].seg = SegSlot{};
    if ((rc = pool_beam_reset(ctx, s, slot0, n)) || (rc = pool_ctc_reset(ctx, s, slot0, n)) || (rc = pool_prefix_reset(ctx, s, slot0, n))) return rc;
    pool_wave_reset(ctx, slot0, n);
    if ((rc = pool_endpoint_reset(ctx, s, slot0, n))) return rc;
    return pool_hist_reset(ctx, s, slot0, n);
}

// The one place that refuses the slot list of a pool call: a row count outside [1, limit], a slot outside [0, limit), a slot listed
// twice.  The limit is the entry point's own: n_streams for pool_chunk_run and rnnt_pool_rescore, max_streams for the seams
// (prefix frames, CTC log-probabilities, wave).  between() holds the refusals an entry point makes after the row count and before
// the first slot, row(i, slot) those of row i once its slot has passed, so the order of its refusals is its own.
template <typename Between, typename Row>
int pool_slots_check(rnnt_ctx* ctx, const char* fn, int n, const int32_t* slots, int limit, const char* what, Between between, Row row) {
    if (n < 1 || n > limit) return fail(ctx, RNNT_ERR_ARG, "%s: %d %s of %d", fn, n, what, limit);
    if (int rc = between()) return rc;
    std::vector<char> seen((size_t)limit, 0);
    for (int i = 0; i < n; ++i) {
        const int slot = slots[i];
        if (slot < 0 || slot >= limit) return fail(ctx, RNNT_ERR_ARG, "%s: row %d: slot %d outside [0, %d)", fn, i, slot, limit);
        if (seen[slot]) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d listed twice", fn, slot);
        seen[slot] = 1;
        if (int rc = row(i, slot)) return rc;
    }
    return RNNT_OK;
}
int pool_slots_check(rnnt_ctx* ctx, const char* fn, int n, const int32_t* slots, int limit, const char* what = "active slots") {
    return pool_slots_check(ctx, fn, n, slots, limit, what, [] { return (int)RNNT_OK; }, [](int, int) { return (int)RNNT_OK; });
}

// The rules of a search in progress (PoolSlot::ctc or ::prefix) for the listed slots advancing by t frames: the first advancing call
// fixed the parameters until the next reset; a search biased under an older graph generation holds node ids of a graph that no longer
// exists; max_cache_frames bounds a search.  weights: the transducer form's message carries them (the CTC search keeps 0).
int search_slot_check(rnnt_ctx* ctx, const char* fn, SearchSlot PoolSlot::*search, int n, const int* slots, int t, int beam_size, float cw, float tw,
                      int use_context, bool weights) {
    for (int i = 0; i < n; ++i) {
        const SearchSlot& q = ctx->slot[slots[i]].*search;
        if (q.beam != 0 && (q.beam != beam_size || q.cw != cw || q.tw != tw || (q.use_context != 0) != (use_context != 0))) {
            if (weights)
                return fail(ctx, RNNT_ERR_ARG,
                            "%s: slot %d: beam_size %d / weights %g, %g / use_context %d differ from the search in progress (%d / %g, %g / %d); reset the slot first", fn,
                            slots[i], beam_size, cw, tw, use_context != 0, q.beam, q.cw, q.tw, q.use_context);
            return fail(ctx, RNNT_ERR_ARG, "%s: slot %d: beam_size %d / use_context %d differ from the search in progress (%d / %d); reset the slot first", fn,
                        slots[i], beam_size, use_context != 0, q.beam, q.use_context);
        }
        if (q.beam != 0 && q.use_context && q.gen != ctx->cg_gen)
            return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the context graph changed since its search began; reset the slot first", fn, slots[i]);
        if ((long long)q.frames_done + t > ctx->cfg.max_cache_frames)
            return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: %d + %d frames exceed max_cache_frames %d", fn, slots[i], q.frames_done, t, ctx->cfg.max_cache_frames);
    }
    return RNNT_OK;
}

// after the launches: t more frames walked; the parameters are fixed by the first call (later ones passed the check with the same values)
void search_slot_commit(rnnt_ctx* ctx, SearchSlot PoolSlot::*search, int n, const int* slots, int t, int beam_size, float cw, float tw, int use_context) {
    for (int i = 0; i < n; ++i) {
        SearchSlot& q = ctx->slot[slots[i]].*search;
        q.frames_done += t;
        q.beam = beam_size; q.cw = cw; q.tw = tw; q.use_context = use_context != 0; q.gen = ctx->cg_gen;
    }
}

// What a read of a slot's search does about the context graph.  biased: it carries context scores (a fresh slot has fixed no graph
// and finalizes its root under the one that is set, if any).  fin: it finalizes, which needs the graph the search ran under.
struct SearchRead { bool biased, fin; };
int search_slot_read(rnnt_ctx* ctx, const char* fn, int slot, const SearchSlot& q, int final, SearchRead& r) {
    r.biased = q.beam > 0 ? q.use_context != 0 : (final != 0 && ctx->cg_on);
    r.fin = r.biased && final != 0;
    if (r.fin && q.beam > 0 && (!ctx->cg_on || q.gen != ctx->cg_gen))
        return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the context graph changed since its search began (final = 0 still reads it)", fn, slot);
    return RNNT_OK;
}

}  // namespace
