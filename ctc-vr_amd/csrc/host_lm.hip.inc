// Layer-major schedule of rnnt_encoder_chunks (kernels and rationale: rnnt_encoder_lm.hip.h).  Included by rnnt_api.hip.
//
// The chunk-by-chunk bookkeeping of the reference (encoder.py:254-264: per-chunk key window, positional window, cache
// truncation) is simulated on the host exactly as for the wavefront schedule; it only parameterises the attention units.
// Rows are stream-major (b*F + f, F = encoder frames of this call per stream), so every per-frame contraction of a layer is one
// plain GEMM over M = B*F rows, K/V rows go straight into the cache through the GEMM's output map, and the conv module sees
// one causal sequence per stream.

namespace {

// Is the plan one the layer-major schedule can run?  K/V rows of the call must have distinct homes in the cache:
//   (A) no cache reset between chunks: rows advance contiguously from the first chunk's append position;
//   (B) the usual fresh stream: the first chunk's K/V are dropped after it (required_cache_size = 0 -> the cache restarts at
//       row 0 with chunk 1, encoder.py:259-264) -- chunk 0's rows are parked in the last rows of the stream's cache buffer.
// Anything else (a reset in the middle of a call) keeps the wavefront schedule.
struct LmPlan { bool ok; int c_r0, c_mod, park0; };
LmPlan lm_plan(const rnnt_ctx* ctx, const std::vector<ChunkInfo>& ci, int F) {
    LmPlan p{false, 0, BIG, -1};
    const int C = (int)ci.size();
    auto wrow = [&](int c) { return ci[c].kv_w0(); };
    bool contiguous = true;
    for (int c = 1; c < C; ++c) contiguous = contiguous && wrow(c) == wrow(c - 1) + ci[c - 1].tq;
    if (contiguous) { p.ok = true; p.c_r0 = wrow(0); return p; }
    bool tail_contig = C >= 2 && wrow(1) == 0 && ci[0].T2 == ci[0].tq && wrow(0) == 0;
    for (int c = 2; c < C; ++c) tail_contig = tail_contig && wrow(c) == wrow(c - 1) + ci[c - 1].tq;
    if (tail_contig && F <= ctx->tcap) {
        p.ok = true; p.c_r0 = ctx->tcap - ci[0].tq; p.c_mod = ctx->tcap; p.park0 = ctx->tcap - ci[0].tq;
        return p;
    }
    return p;
}

// Ragged batch (rnnt_decode_ragged): the call's `ci` chunks are the COMMON full-size chunks, run for every stream; stream b uses
// the first nb[b] of them and then its own tail chunk (online_rnnt_decode.py:88-91).  Rows beyond a stream's frames hold
// unused values: a frame depends only on earlier frames of its own stream (cached keys, causal conv), never on later ones.
struct RaggedPlan {
    std::vector<int> nb;              // common chunks stream b really has (0: the stream does not take part)
    std::vector<ChunkInfo> tail;      // stream b's tail chunk (len 0: none); fpos = first frame of the tail in the stream's rows
    std::vector<int> frames;          // encoder frames of stream b in this call
    int F = 0;                        // rows per stream = max(frames)
};

int lm_res_upload(rnnt_ctx* ctx, hipStream_t s, const std::vector<std::vector<LmRow>>& tabs) {
    ctx->lm_res_ok = 0;
    if (!lm_res_plan(tabs, ctx->lm_rhdr_host, ctx->lm_rrows_host, ctx->lm_res_stride)) return RNNT_OK;
    int rc;
    if ((rc = reserve(ctx, ctx->lm_rhdr, ctx->lm_rhdr_host.size()))) return rc;
    if ((rc = reserve(ctx, ctx->lm_rrows, ctx->lm_rrows_host.size()))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->lm_rhdr, ctx->lm_rhdr_host.data(), ctx->lm_rhdr_host.size() * sizeof(LmResHdr), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->lm_rrows, ctx->lm_rrows_host.data(), ctx->lm_rrows_host.size() * sizeof(LmRow), hipMemcpyHostToDevice, s));
    ctx->lm_res_ok = 1;
    return RNNT_OK;
}

// ---- A-stationary kernels (rnnt_gemm_as.hip.h), split-operand modes ------------------------------------------------------------
constexpr int AS_MT = 3;     // 48 rows per workgroup: 251 workgroups at M = 12032 (64 streams x 188 frames), one per CU
template <int NUM>
int launch_gemm_as_t(rnnt_ctx* ctx, hipStream_t s, const AsBatch& ab) {
    const size_t lds = (size_t)FuseCfg<NUM>::PLANES * 16 * AS_MT * FuseCfg<NUM>::ROWB;
    { const int rc_attr = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&gemm_as<NUM, AS_MT>), lds); if (rc_attr) return rc_attr; }
    hipLaunchKernelGGL((gemm_as<NUM, AS_MT>), dim3((ab.g[0].M + 16 * AS_MT - 1) / (16 * AS_MT)), dim3(256), lds, s, ab);
    LAUNCHCHK("gemm_as");
    return RNNT_OK;
}
// ng descriptors sharing A (plain rows, K = 256, or K = 1024 with N = 256 and ng = 1), N % 64 == 0; wp[i] = packed fragments of g[i].W
int launch_gemm_as(rnnt_ctx* ctx, hipStream_t s, const GemmP* gs, const uint4* const* wp, int ng, int tag) {
    ProfScope prof(ctx, s, tag);
    AsBatch ab;
    memset(&ab, 0, sizeof(ab));
    ab.ng = ng;
    for (int i = 0; i < ng; ++i) {
        ab.g[i] = gs[i];
        ab.wp[i] = wp[i];
        int rc = prepare_gemm(ctx, ab.g[i]);
        if (rc) return rc;
        if (gs[i].N % 64 || gs[i].M != gs[0].M || gs[i].K != gs[0].K || gs[i].A != gs[0].A) return fail(ctx, RNNT_ERR_SHAPE, "gemm_as: descriptors do not share A / shape");
    }
    const int K = gs[0].K;
    if (!(K == 256 || (K % 256 == 0 && ng == 1 && gs[0].N == 256)) || !ab.g[0].a_plain) return fail(ctx, RNNT_ERR_SHAPE, "gemm_as: unsupported shape K=%d N=%d", K, gs[0].N);
    switch (ctx->numerics) {
        case RNNT_NUM_BF16X3: return launch_gemm_as_t<RNNT_NUM_BF16X3>(ctx, s, ab);
        case RNNT_NUM_F16X3: return launch_gemm_as_t<RNNT_NUM_F16X3>(ctx, s, ab);
        case RNNT_NUM_BF16: return launch_gemm_as_t<RNNT_NUM_BF16>(ctx, s, ab);
        default: return fail(ctx, RNNT_ERR_STATE, "gemm_as: exact-f32 mode has no packed 16-bit weights");
    }
}
template <int NUM, int NW>
int launch_ffn_as_t(rnnt_ctx* ctx, hipStream_t s, const FfnP& p) {
    const size_t lds = FFN_LDS(NUM, NW) + ((p.H0 || p.dw.g || p.w1p2) ? FFN_XROWS : 0);  // both operand images; result rows and the tail's image overlay them; the head's x' rows behind
    { const int rc_attr = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&ffn_as<NUM, AS_MT, NW>), lds); if (rc_attr) return rc_attr; }
    hipLaunchKernelGGL((ffn_as<NUM, AS_MT, NW>), dim3((p.M + 16 * AS_MT - 1) / (16 * AS_MT)), dim3(64 * NW), lds, s, p);
    if (NW == 16) LAUNCHCHK("ffn_as<16>"); else if (NW == 4) LAUNCHCHK("ffn_as<4>"); else LAUNCHCHK("ffn_as<8>");
    return RNNT_OK;
}
int launch_ffn_as(rnnt_ctx* ctx, hipStream_t s, const FfnP& p) {
    ProfScope prof(ctx, s, p.A0 ? TAG_OUT_PW1 : (p.w1p2 ? TAG_FFN_MERGED : (p.n_tail > 0 ? TAG_FFN_QKV : TAG_FFN_FUSED)));
    // waves per workgroup: 8 = two per SIMD, one wave's waits on weight fragments under the other's MFMAs (bitwise the same
    // results as 4; FFN 52 -> 47 us, FFN + q/k/v 102 -> 87 us, linear_out + pointwise_conv1 48 -> 39 us); RNNT_FFN_NW=4 reverts, =16
    // runs 1024-thread workgroups (the same bits too: a column's sums do not depend on the wave that owns it; test_kernel_forms.py)
    const int nw = ctx->ffn_nw;
#define FFN_NW_DISPATCH(NUM_) return nw == 16 ? launch_ffn_as_t<NUM_, 16>(ctx, s, p) : nw == 4 ? launch_ffn_as_t<NUM_, 4>(ctx, s, p) : launch_ffn_as_t<NUM_, 8>(ctx, s, p)
    switch (ctx->numerics) {
        case RNNT_NUM_BF16X3: FFN_NW_DISPATCH(RNNT_NUM_BF16X3);
        case RNNT_NUM_F16X3: FFN_NW_DISPATCH(RNNT_NUM_F16X3);
        case RNNT_NUM_BF16: FFN_NW_DISPATCH(RNNT_NUM_BF16);
        default: return fail(ctx, RNNT_ERR_STATE, "ffn_as: exact-f32 mode has no packed 16-bit weights");
    }
}

// out_plain != null (full-context pass, rnnt_encoder_full): after_norm of the B*F rows goes to out_plain [B*F][256] and nothing is
// appended to the frame buffer; klen_dev = per-stream valid keys (padding mask after subsampling, subsampling.py:228).
int encoder_chunks_lm(rnnt_ctx* ctx, hipStream_t s, const float* fbank_dev, int total_frames, const int32_t* chunk_start,
                      const std::vector<ChunkInfo>& ci, const std::vector<int>& plan_key, int greedy, bool* handled,
                      float* out_plain = nullptr, const int* klen_dev = nullptr, const RaggedPlan* rg = nullptr) {
    *handled = false;
    if (!ctx->use_lm) return RNNT_OK;
    const int B = ctx->n_streams, C = (int)ci.size(), Bm = ctx->cfg.max_streams;
    const int fb0 = ci[0].fpos;
    int F = 0;
    for (int c = 0; c < C; ++c) F += ci[c].tq;
    if (rg) F = std::max(F, rg->F);
    const LmPlan plan = lm_plan(ctx, ci, F);
    if (!plan.ok) return RNNT_OK;
    const long long M = (long long)B * F;
    if (M * RNNT_FSUB >= (1ll << 31)) return RNNT_OK;
    int rc;
    // ---- buffers (sized by the context limits so one allocation serves every call) ----------------------------------------------
    const int fmax = std::max(ctx->fcap, ctx->tmax);              // frames per stream a call can bring (a full-context pass: tmax)
    if (F > fmax) return RNNT_OK;
    const int gs = RNNT_LORDER + fmax;                            // rows per stream of a layer's linear post-GLU buffer
    const size_t rows = (size_t)Bm * fmax;
    if ((rc = reserve(ctx, ctx->lm_x, rows * D))) return rc;
    if ((rc = reserve(ctx, ctx->lm_h, rows * FF))) return rc;
    if ((rc = reserve(ctx, ctx->lm_q, rows * D))) return rc;
    if ((rc = reserve(ctx, ctx->lm_a, rows * D))) return rc;
    if ((rc = reserve(ctx, ctx->lm_d, rows * D))) return rc;
    if ((rc = reserve(ctx, ctx->lm_g, (size_t)L * Bm * gs * D))) return rc;
    float* x = ctx->lm_x;
    bool ctx_in_done = false;                                      // (c) already launched on the side stream
    // An error exit between the fork onto the side stream and the join still joins it: work already enqueued there writes x, lm_g
    // and the side slabs, and must not run on unordered with whatever the caller enqueues next on `s`.
    struct SideJoin {
        rnnt_ctx* ctx; hipStream_t s; bool armed;
        ~SideJoin() {
            if (!armed) return;
            (void)hipEventRecord(ctx->sub_ev[1], ctx->sub_stream);
            (void)hipStreamWaitEvent(s, ctx->sub_ev[1], 0);
        }
    } side_join{ctx, s, false};
    // ---- (a) subsampling: every run of equal-length chunks in one slab, stream-major ------------------------------------------
    if ((rc = reserve(ctx, ctx->wf_starts, (size_t)C))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->wf_starts, chunk_start, C * sizeof(int), hipMemcpyHostToDevice, s));
    {
        const size_t slab_bytes = 2048ull << 20;
        struct Cls { int c0, c1; };
        std::vector<Cls> cls;                                      // runs of equal-length chunks (one slab each)
        // (the bound is on the class's largest slab: y1 -- or y2 where conv2 forms the conv1 operand itself and no y1 exists; a run that
        // is cut by the y1 bound and whose pieces would still be fused is cut by the y2 bound instead, so fusing never adds a class)
        auto fused_cls = [&](int c0, int nc) { return conv2_fused(ctx, (long long)nc * B * ci[c0].tq * RNNT_FSUB); };
        for (int c0 = 0; c0 < C;) {
            int c1 = c0 + 1, e1 = c0 + 1;
            const size_t per1 = (size_t)B * sub1_len(ci[c0].len) * RNNT_F1 * D, per2 = (size_t)B * ci[c0].tq * RNNT_FSUB * D;
            while (c1 < C && ci[c1].len == ci[c0].len && (size_t)(c1 - c0 + 1) * per1 * sizeof(float) <= slab_bytes) ++c1;
            while (e1 < C && ci[e1].len == ci[c0].len && (size_t)(e1 - c0 + 1) * per2 * sizeof(float) <= slab_bytes) ++e1;
            if (e1 > c1 && fused_cls(c0, e1 - c0)) c1 = e1;
            cls.push_back({c0, c1});
            c0 = c1;
        }
        // The call's tail chunk is a class of its own: three small launches (conv1, conv2, embed of B x 5 frames: 33 + 77 + 89 us,
        // launch-bound) that nothing depends on until layer 0.  They run on a side stream, with their own slabs, beside the main
        // class's subsampling (RNNT_LM_SIDE=0: in line).
        const int lm_side = ctx->lm_side;                          // (per context, read at rnnt_create)
        const bool side = lm_side && cls.size() >= 2 && cls.back().c1 - cls.back().c0 == 1;
        size_t need1 = 0, need2 = 0, need1b = 0, need2b = 0;
        for (size_t k = 0; k < cls.size(); ++k) {
            const int c0 = cls[k].c0, nc = cls[k].c1 - cls[k].c0;
            const size_t per1 = (size_t)B * sub1_len(ci[c0].len) * RNNT_F1 * D, per2 = (size_t)B * ci[c0].tq * RNNT_FSUB * D;
            if (side && k + 1 == cls.size()) { need1b = per1 * nc; need2b = per2 * nc; }
            else { if (!fused_cls(c0, nc)) need1 = std::max(need1, per1 * nc); need2 = std::max(need2, per2 * nc); }
        }
        if ((rc = reserve(ctx, ctx->lm_y1, need1))) return rc;
        if ((rc = reserve(ctx, ctx->lm_y2, need2))) return rc;
        if (side) {
            if ((rc = reserve(ctx, ctx->lm_y1b, need1b))) return rc;
            if ((rc = reserve(ctx, ctx->lm_y2b, need2b))) return rc;
            if (!ctx->sub_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->sub_stream, hipStreamNonBlocking));
            if (!ctx->sub_ev[0]) {
                HIPCHK(hipEventCreateWithFlags(&ctx->sub_ev[0], hipEventDisableTiming));
                HIPCHK(hipEventCreateWithFlags(&ctx->sub_ev[1], hipEventDisableTiming));
            }
            HIPCHK(hipEventRecord(ctx->sub_ev[0], s));            // fbank, chunk starts and everything earlier on the caller's stream
            HIPCHK(hipStreamWaitEvent(ctx->sub_stream, ctx->sub_ev[0], 0));
            side_join.armed = true;
            // (c) the left context of every layer's conv module depends on nothing of this call either: it rides along
            hipLaunchKernelGGL(lm_ctx_in, dim3(grid_for((long long)L * B * RNNT_LORDER * D)), dim3(256), 0, ctx->sub_stream, ctx->gring, ctx->lm_g, B, Bm,
                               ctx->cap, gs, ci[0].ring_pos);
            LAUNCHCHK("lm_ctx_in");
            ctx_in_done = true;
            const int c0 = cls.back().c0;
            if ((long long)B * ci[c0].tq * RNNT_FSUB >= (1ll << 31)) return fail(ctx, RNNT_ERR_SHAPE, "subsampling slab too large");
            if ((rc = run_subsample(ctx, ctx->sub_stream, fbank_dev, B, total_frames, ci[c0].len, ctx->wf_starts + c0, 1, ctx->lm_y1b, ctx->lm_y2b, x,
                                    ci[c0].tq, F, ci[c0].fpos - fb0, true)))
                return rc;
            HIPCHK(hipEventRecord(ctx->sub_ev[1], ctx->sub_stream));
        }
        for (size_t k = 0; k < cls.size(); ++k) {
            if (side && k + 1 == cls.size()) break;
            const int c0 = cls[k].c0, nc = cls[k].c1 - cls[k].c0;
            if ((long long)nc * B * ci[c0].tq * RNNT_FSUB >= (1ll << 31)) return fail(ctx, RNNT_ERR_SHAPE, "subsampling slab too large");
            if ((rc = run_subsample(ctx, s, fbank_dev, B, total_frames, ci[c0].len, ctx->wf_starts + c0, nc, ctx->lm_y1, ctx->lm_y2, x,
                                    nc * ci[c0].tq, F, ci[c0].fpos - fb0, c0 != 0, true)))
                return rc;
        }
        if (side) {
            side_join.armed = false;
            HIPCHK(hipStreamWaitEvent(s, ctx->sub_ev[1], 0));     // join: layer 0 reads every class's rows of x
        }
    }
    // ---- (a') ragged batch: every stream's tail chunk, one subsampling pass per tail length ---------------------------------------
    if (rg) {
        std::map<int, std::vector<int>> classes;                   // tail length -> streams
        for (int b = 0; b < B; ++b)
            if (rg->tail[b].len >= 7) classes[rg->tail[b].len].push_back(b);
        size_t n_ent = 0, need_fb = 0, need_xt = 0, need1 = 0, need2 = 0;
        for (auto& kv : classes) {
            const size_t n = kv.second.size();
            n_ent += 2 * n;
            need_fb = std::max(need_fb, n * kv.first * RNNT_IDIM);
            need_xt = std::max(need_xt, n * sub_len(kv.first) * D);
            need1 = std::max(need1, n * sub1_len(kv.first) * RNNT_F1 * D);
            need2 = std::max(need2, n * sub_len(kv.first) * RNNT_FSUB * D);
        }
        if ((rc = reserve(ctx, ctx->lm_y1, need1))) return rc;
        if ((rc = reserve(ctx, ctx->lm_y2, need2))) return rc;
        if ((rc = reserve(ctx, ctx->rg_fb, need_fb))) return rc;
        if ((rc = reserve(ctx, ctx->rg_xt, need_xt))) return rc;
        if ((rc = reserve(ctx, ctx->rg_ent, n_ent))) return rc;
        std::vector<int2> ent;
        ent.reserve(n_ent);
        for (auto& kv : classes)                                    // per class: gather entries (stream, first fbank frame), then scatter entries (stream, first row)
            for (int pass = 0; pass < 2; ++pass)
                for (int b : kv.second) ent.push_back(pass == 0 ? make_int2(b, rg->nb[b] * ci[0].len) : make_int2(b, rg->tail[b].fpos - fb0));
        HIPCHK(hipMemcpyAsync(ctx->rg_ent, ent.data(), ent.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                            // `ent` dies at scope end
        size_t eo = 0;
        for (auto& kv : classes) {
            const int len = kv.first, n = (int)kv.second.size(), tqt = sub_len(len);
            hipLaunchKernelGGL(lm_gather_tails, dim3(grid_for((long long)n * len * RNNT_IDIM)), dim3(256), 0, s, fbank_dev, ctx->rg_fb, ctx->rg_ent + eo, n, len, total_frames);
            LAUNCHCHK("lm_gather_tails");
            if ((rc = run_subsample(ctx, s, ctx->rg_fb, n, len, len, nullptr, 1, ctx->lm_y1, ctx->lm_y2, ctx->rg_xt, 0, 0, 0, true))) return rc;
            hipLaunchKernelGGL(lm_scatter_rows, dim3(grid_for((long long)n * tqt * D)), dim3(256), 0, s, ctx->rg_xt, x, ctx->rg_ent + eo + n, n, tqt, F);
            LAUNCHCHK("lm_scatter_rows");
            eo += 2 * (size_t)n;
        }
    }
    // ---- (b) attention rows: every query frame with its chunk's key window, LM_ROWS consecutive rows per workgroup ---------------
    int rg_blocks = 0;
    if (rg) {
        // per-stream tables [B][n_blocks]: the common chunks a stream really has, then its tail (empty blocks pad the shorter streams)
        std::vector<std::vector<LmBlock>> per(B);
        for (int b = 0; b < B; ++b) {
            std::vector<LmBlock>& blocks = per[b];
            LmBlock cur;
            int pmax = 0;
            auto reset = [&]() { memset(&cur, 0, sizeof(cur)); for (int k = 0; k < LM_ROWS; ++k) cur.r[k].f = -1; };
            auto flush = [&]() { if (cur.n_rows) blocks.push_back(cur); reset(); };
            reset();
            const int nch = rg->nb[b] + (rg->tail[b].len >= 7 ? 1 : 0);
            for (int c = 0; c < nch; ++c) {
                const ChunkInfo& k = c < rg->nb[b] ? ci[c] : rg->tail[b];
                const int kv0 = (c == 0 && plan.park0 >= 0) ? plan.park0 : k.kv_row0;
                const int psh = k.pos_start - kv0;
                for (int q0 = 0; q0 < k.tq; ++q0) {
                    const LmRow rw{k.fpos - fb0 + q0, kv0, kv0 + k.T2, psh};
                    bool join = cur.n_rows > 0 && cur.n_rows < LM_ROWS && rw.ks <= cur.amax && rw.ke >= cur.amin;
                    if (join) {
                        const int lo = std::min(cur.pmin, psh), hi = std::max(pmax, psh);
                        join = hi - lo <= LM_PEXT;
                    }
                    if (!join) { flush(); cur.amin = rw.ks; cur.amax = rw.ke; cur.pmin = psh; pmax = psh; }
                    cur.amin = std::min(cur.amin, rw.ks); cur.amax = std::max(cur.amax, rw.ke);
                    cur.pmin = std::min(cur.pmin, psh); pmax = std::max(pmax, psh);
                    cur.r[cur.n_rows++] = rw;
                }
            }
            flush();
            rg_blocks = std::max(rg_blocks, (int)blocks.size());
        }
        if (rg_blocks < 1) rg_blocks = 1;
        std::vector<LmBlock>& flat = ctx->lm_blocks_host;
        LmBlock empty;
        memset(&empty, 0, sizeof(empty));
        for (int k = 0; k < LM_ROWS; ++k) empty.r[k].f = -1;
        flat.assign((size_t)B * rg_blocks, empty);
        for (int b = 0; b < B; ++b) std::copy(per[b].begin(), per[b].end(), flat.begin() + (size_t)b * rg_blocks);
        if ((rc = reserve(ctx, ctx->lm_blocks, flat.size()))) return rc;
        HIPCHK(hipMemcpyAsync(ctx->lm_blocks, flat.data(), flat.size() * sizeof(LmBlock), hipMemcpyHostToDevice, s));
        ctx->lm_key.clear();                                        // never equal to a uniform call's key
        std::vector<std::vector<LmRow>> tabs(B);
        for (int b = 0; b < B; ++b) tabs[b] = lm_rows_of(per[b].data(), per[b].size());
        if ((rc = lm_res_upload(ctx, s, tabs))) return rc;
    } else if (plan_key != ctx->lm_key) {
        std::vector<LmBlock>& blocks = ctx->lm_blocks_host;
        blocks.clear();
        LmBlock cur;
        int pmax = 0;
        auto reset = [&]() { memset(&cur, 0, sizeof(cur)); for (int k = 0; k < LM_ROWS; ++k) cur.r[k].f = -1; };
        auto flush = [&]() { if (cur.n_rows) blocks.push_back(cur); reset(); };
        reset();
        for (int c = 0; c < C; ++c) {
            const int kv0 = (c == 0 && plan.park0 >= 0) ? plan.park0 : ci[c].kv_row0;
            const int psh = ci[c].pos_start - kv0;
            for (int q0 = 0; q0 < ci[c].tq; ++q0) {
                const LmRow rw{ci[c].fpos - fb0 + q0, kv0, kv0 + ci[c].T2, psh};
                bool join = cur.n_rows > 0 && cur.n_rows < LM_ROWS && rw.ks <= cur.amax && rw.ke >= cur.amin;
                if (join) {
                    const int lo = std::min(cur.pmin, psh), hi = std::max(pmax, psh);
                    join = hi - lo <= LM_PEXT;
                }
                if (!join) { flush(); cur.amin = rw.ks; cur.amax = rw.ke; cur.pmin = psh; pmax = psh; }
                cur.amin = std::min(cur.amin, rw.ks); cur.amax = std::max(cur.amax, rw.ke);
                cur.pmin = std::min(cur.pmin, psh); pmax = std::max(pmax, psh);
                cur.r[cur.n_rows++] = rw;
            }
        }
        flush();
        if ((rc = reserve(ctx, ctx->lm_blocks, blocks.size()))) return rc;
        HIPCHK(hipMemcpyAsync(ctx->lm_blocks, blocks.data(), blocks.size() * sizeof(LmBlock), hipMemcpyHostToDevice, s));
        if ((rc = lm_res_upload(ctx, s, {lm_rows_of(blocks.data(), blocks.size())}))) return rc;
        ctx->lm_key = plan_key;
    }
    const int n_blocks = rg ? rg_blocks : (int)ctx->lm_blocks_host.size();
    if ((rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_mfma), LM2_LDS))) return rc;
    // rel_attention_lm_res when every table fits its plan (split-operand modes), else rel_attention_lm_bf
    const bool attn_res = ctx->lm_res_ok && ctx->attn_resident && ctx->attn_bf && ctx->numerics != RNNT_NUM_F32;
    if (attn_res) {
        if (ctx->numerics == RNNT_NUM_BF16X3) rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_res<2, false>), LMR_LDS);
        else if (ctx->numerics == RNNT_NUM_F16X3) rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_res<2, true>), LMR_LDS);
        else rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_res<1, false>), LMR_LDS);
    } else if (ctx->numerics == RNNT_NUM_BF16X3) rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_bf<2, false>), LMB_LDS);
    else if (ctx->numerics == RNNT_NUM_F16X3) rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_bf<2, true>), LMB_LDS);
    else if (ctx->numerics == RNNT_NUM_BF16) rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_lm_bf<1, false>), LMB_LDS);
    if (rc) return rc;
    // ---- (c) left context of every layer's conv module -------------------------------------------------------------------------
    if (!ctx_in_done) {
        hipLaunchKernelGGL(lm_ctx_in, dim3(grid_for((long long)L * B * RNNT_LORDER * D)), dim3(256), 0, s, ctx->gring, ctx->lm_g, B, Bm, ctx->cap, gs,
                           ci[0].ring_pos);
        LAUNCHCHK("lm_ctx_in");
    }
    // ---- (d) the 12 blocks, each over all B*F rows (ConformerEncoderLayer.forward, encoder_layer.py:188-265) ---------------------
    const int Mi = (int)M;
    static const bool lm_debug = getenv("RNNT_LM_DEBUG") != nullptr;
    auto dbg = [&](const char* what, int l, const float* p, long long n) {
        if (!lm_debug) return;
        unsigned long long* acc = reinterpret_cast<unsigned long long*>(ctx->dec_ctrl + 16);
        (void)hipMemsetAsync(acc, 0, 8, s);
        hipLaunchKernelGGL(debug_checksum, dim3(1024), dim3(256), 0, s, p, n, acc);
        unsigned long long h = 0;
        (void)hipMemcpyAsync(&h, acc, 8, hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        fprintf(stderr, "[lm debug] layer %2d %-8s %016llx\n", l, what, h);
    };
    dbg("y2", -1, ctx->lm_y2, (long long)B * ci[C - 1].tq * RNNT_FSUB * D);
    dbg("embed", -1, x, M * D);
    // q to a buffer, K / V rows of every chunk to their cache rows (attention.py:109-131, 180-245)
    auto qkv_desc = [&](int l, GemmP (&qkv)[3]) {
        const LayerW& w = ctx->lw[l];
        float* kc = ctx->kcache + (size_t)l * Bm * ctx->tcap * D;
        float* vc = ctx->vcache + (size_t)l * Bm * ctx->tcap * D;
        qkv[0] = plain_gemm(x, D, w.wq, D, w.bq, ctx->lm_q, D, Mi, D, D);
        qkv[1] = plain_gemm(x, D, w.wk, D, w.bk, kc, D, Mi, D, D);
        qkv[2] = plain_gemm(x, D, w.wv, D, w.bv, vc, D, Mi, D, D);
        for (int i = 0; i < 3; ++i) { qkv[i].ln_g = w.ln_mha_g; qkv[i].ln_b = w.ln_mha_b; }
        for (int i = 1; i < 3; ++i) {
            qkv[i].c_n = F; qkv[i].c_s0 = (long long)ctx->tcap * D; qkv[i].c_r0 = plan.c_r0; qkv[i].c_mod = plan.c_mod; qkv[i].c_s1 = D;
        }
    };
    bool macaron_done = false;   // layer l's macaron FFN + q/k/v already ran inside layer l - 1's last launch (RNNT_LM_FFN_MERGE)
    for (int l = 0; l < L; ++l) {
        const LayerW& w = ctx->lw[l];
        float* kc = ctx->kcache + (size_t)l * Bm * ctx->tcap * D;
        float* vc = ctx->vcache + (size_t)l * Bm * ctx->tcap * D;
        float* gl = ctx->lm_g + (size_t)l * B * gs * D;
        GemmP g;
        const bool as = ctx->use_as && ctx->numerics != RNNT_NUM_F32 && (int)ctx->layers_host.size() == L;   // packed 16-bit weights there
        const LayerDev* ld = as ? &ctx->layers_host[l] : nullptr;
        // x += 0.5 * FFN_macaron(LN(x))
        GemmP qkv[3];
        qkv_desc(l, qkv);
        const int qkv_tail = ctx->lm_qkv_tail;
        const bool tail = as && qkv_tail;
        if (macaron_done) {
            macaron_done = false;                                   // (the previous layer's last launch did this layer's macaron FFN + q/k/v)
        } else {
        if (as) {
            FfnP fp{x, x, w.ln_ffm_g, w.ln_ffm_b, ld->w1m, ld->w2m, w.b1m, w.b2m, nullptr, nullptr, 0.5f, Mi};
            fp.n_tail = 0;
            if (tail) {   // the self-attention projections ride on the macaron FFN's result rows while they are still in LDS
                fp.n_tail = 3; fp.lnt_g = w.ln_mha_g; fp.lnt_b = w.ln_mha_b;
                const uint4* wp3[3] = {ld->wq, ld->wk, ld->wv};
                for (int i = 0; i < 3; ++i) { fp.tg[i] = qkv[i]; if ((rc = prepare_gemm(ctx, fp.tg[i]))) return rc; fp.twp[i] = wp3[i]; }
            }
            if ((rc = launch_ffn_as(ctx, s, fp))) return rc;
        } else {
        g = plain_gemm(x, D, w.w1m, D, w.b1m, ctx->lm_h, FF, Mi, FF, D, EPI_SILU);
        g.ln_g = w.ln_ffm_g; g.ln_b = w.ln_ffm_b;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_FFN1))) return rc;
        dbg("ffn1m", l, ctx->lm_h, M * FF);
        g = plain_gemm(ctx->lm_h, FF, w.w2m, FF, w.b2m, x, D, Mi, D, FF, EPI_RESID, 0.5f);
        g.R = x;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_FFN2))) return rc;
        }
        dbg("ffn2m", l, x, M * D);
        if (tail) {
            // done by the macaron launch
        } else if (as) {
            const uint4* wp[3] = {ld->wq, ld->wk, ld->wv};
            if ((rc = launch_gemm_as(ctx, s, qkv, wp, 3, TAG_QKV))) return rc;
        } else if ((rc = launch_gemm(ctx, s, qkv, 3, TAG_QKV))) return rc;
        }
        dbg("q", l, ctx->lm_q, M * D);
        dbg("kcache", l, kc, (long long)B * ctx->tcap * D);
        {
            ProfScope prof(ctx, s, TAG_ATTN);
            LmAttnP a{ctx->lm_q, kc, vc, w.ptab, w.pu, w.pv, ctx->lm_a, ctx->lm_blocks, F, (long long)ctx->tcap, klen_dev, rg ? 1 : 0};
            const dim3 ag(B * RNNT_H, n_blocks);
            if (attn_res) {
                const LmResP r{ctx->lm_q, kc, vc, w.ptab, w.pu, w.pv, ctx->lm_a, ctx->lm_rhdr, ctx->lm_rrows, ctx->lm_res_stride, F, (long long)ctx->tcap,
                               klen_dev, rg ? 1 : 0};
                if (ctx->numerics == RNNT_NUM_BF16X3) hipLaunchKernelGGL((rel_attention_lm_res<2, false>), dim3(B * RNNT_H), dim3(64 * LMR_NW), LMR_LDS, s, r);
                else if (ctx->numerics == RNNT_NUM_F16X3) hipLaunchKernelGGL((rel_attention_lm_res<2, true>), dim3(B * RNNT_H), dim3(64 * LMR_NW), LMR_LDS, s, r);
                else hipLaunchKernelGGL((rel_attention_lm_res<1, false>), dim3(B * RNNT_H), dim3(64 * LMR_NW), LMR_LDS, s, r);
                LAUNCHCHK("rel_attention_lm_res");
            } else if (ctx->numerics == RNNT_NUM_F32 || !ctx->attn_bf) {
                hipLaunchKernelGGL(rel_attention_lm_mfma, ag, dim3(256), LM2_LDS, s, a);
                LAUNCHCHK("rel_attention_lm_mfma");
            } else {
                if (ctx->numerics == RNNT_NUM_BF16X3) hipLaunchKernelGGL((rel_attention_lm_bf<2, false>), ag, dim3(256), LMB_LDS, s, a);
                else if (ctx->numerics == RNNT_NUM_F16X3) hipLaunchKernelGGL((rel_attention_lm_bf<2, true>), ag, dim3(256), LMB_LDS, s, a);
                else hipLaunchKernelGGL((rel_attention_lm_bf<1, false>), ag, dim3(256), LMB_LDS, s, a);
                LAUNCHCHK("rel_attention_lm_bf");
            }
        }
        dbg("attn", l, ctx->lm_a, M * D);
        // x += conv_module(LN(x)) (convolution.py:98-153): pointwise_conv1 + GLU into the linear buffer behind the left context
        GemmP gpw1 = plain_gemm(x, D, w.pw1, D, w.bpw1, gl, D, Mi, 2 * D, D, EPI_GLU);
        gpw1.ln_g = w.ln_conv_g; gpw1.ln_b = w.ln_conv_b;
        gpw1.c_n = F; gpw1.c_s0 = (long long)gs * D; gpw1.c_r0 = RNNT_LORDER; gpw1.c_mod = BIG; gpw1.c_s1 = D;
        const int out_chain = ctx->lm_out_chain;
        if (as && out_chain) {
            // linear_out + residual, then norm_conv + pointwise_conv1 + GLU from the result rows while they are in LDS: one launch
            FfnP fp{x, x, nullptr, nullptr, nullptr, ld->wo, nullptr, w.bo, nullptr, nullptr, 1.0f, Mi};
            fp.n_tail = 1; fp.lnt_g = w.ln_conv_g; fp.lnt_b = w.ln_conv_b; fp.A0 = ctx->lm_a;
            fp.tg[0] = gpw1;
            if ((rc = prepare_gemm(ctx, fp.tg[0]))) return rc;
            fp.twp[0] = ld->pw1;
            if ((rc = launch_ffn_as(ctx, s, fp))) return rc;
            dbg("pw1", l, gl, (long long)B * gs * D);
        } else {
        g = plain_gemm(ctx->lm_a, D, w.wo, D, w.bo, x, D, Mi, D, D, EPI_RESID, 1.0f);
        g.R = x;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_ATTN_OUT))) return rc;
        dbg("out", l, x, M * D);
        g = gpw1;
        if (as) {
            const uint4* wp[1] = {ld->pw1};
            if ((rc = launch_gemm_as(ctx, s, &g, wp, 1, TAG_PW1))) return rc;
        } else if ((rc = launch_gemm(ctx, s, &g, 1, TAG_PW1))) return rc;
        dbg("pw1", l, gl, (long long)B * gs * D);
        }
        // pointwise_conv2 + residual in front of the FFN, inside its launch (x' stays in LDS): RNNT_LM_PW2_HEAD=0 keeps the two launches;
        // RNNT_LM_PW2_HEAD=2 (default) also forms the depthwise conv + BN + SiLU rows there instead of in a launch of their own
        const int pw2_head = ctx->lm_pw2_head;                     // (per context, read at rnnt_create)
        const DwLmP d{gl, w.wdw_t, w.bdw, w.bn_s, w.bn_t, ctx->lm_d, x, ctx->gring + (size_t)l * Bm * ctx->cap * D,
                      ctx->xring + (size_t)l * Bm * ctx->cap * D, B, F, gs, ctx->cap, ci[0].ring_pos};
        const bool dw_in_head = as && pw2_head == 2;
        if (!dw_in_head) {
            ProfScope prof(ctx, s, TAG_DWCONV);
            hipLaunchKernelGGL(dwconv_lm, dim3(grid_for((long long)B * ((F + LM_FB - 1) / LM_FB) * D)), dim3(256), 0, s, d);
            LAUNCHCHK("dwconv_lm");
            dbg("dw", l, ctx->lm_d, M * D);
        }
        if (as && pw2_head) {
            FfnP fp{x, x, w.ln_ff_g, w.ln_ff_b, ld->w1, ld->w2, w.b1, w.b2, w.ln_fin_g, w.ln_fin_b, 0.5f, Mi};
            if (dw_in_head) fp.dw = d; else fp.H0 = ctx->lm_d;
            fp.whp = ld->pw2; fp.bh = w.bpw2;
            if (klen_dev) { fp.hrowlen = klen_dev; fp.hrowlen_n = F; }   // full-context pass: the conv module's output is zero on padded frames (convolution.py:148-150)
            // RNNT_LM_FFN_MERGE=1: ... and continues into the NEXT layer's macaron FFN + q/k/v (both row-local): one launch per layer
            // boundary, 61 -> 50 launches.  Measured: one batch in flight 7.83 -> 7.75 ms (encoder 4.28 -> 4.17), but TWO batches in
            // flight 6.2 -> 6.65 ms per batch (a 130 us launch that holds every CU interleaves worse with the other context's
            // decoder than two 60 us ones: 191 us in the timed region against 68 + 72), so it is off by default.
            const int ffn_merge = ctx->lm_ffn_merge;
            if (ffn_merge && tail && l + 1 < L) {
                const LayerW& wn = ctx->lw[l + 1];
                const LayerDev* ldn = &ctx->layers_host[l + 1];
                fp.ln_g2 = wn.ln_ffm_g; fp.ln_b2 = wn.ln_ffm_b; fp.w1p2 = ldn->w1m; fp.w2p2 = ldn->w2m; fp.b1_2 = wn.b1m; fp.b2_2 = wn.b2m; fp.alpha2 = 0.5f;
                GemmP qn[3];
                qkv_desc(l + 1, qn);
                fp.n_tail = 3; fp.lnt_g = wn.ln_mha_g; fp.lnt_b = wn.ln_mha_b;
                const uint4* wp3[3] = {ldn->wq, ldn->wk, ldn->wv};
                for (int i = 0; i < 3; ++i) { fp.tg[i] = qn[i]; if ((rc = prepare_gemm(ctx, fp.tg[i]))) return rc; fp.twp[i] = wp3[i]; }
                macaron_done = true;
            }
            if ((rc = launch_ffn_as(ctx, s, fp))) return rc;
            dbg("pw2+ffn+ln", l, x, M * D);
            continue;
        }
        g = plain_gemm(ctx->lm_d, D, w.pw2, D, w.bpw2, x, D, Mi, D, D, EPI_RESID, 1.0f);
        g.R = x;
        if (klen_dev) { g.rowlen = klen_dev; g.rowlen_n = F; }   // full-context pass: the conv module's output is zero on padded frames (convolution.py:148-150)
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_PW2))) return rc;
        dbg("pw2", l, x, M * D);
        // x += 0.5 * FFN(LN(x)); x = LN_final(x)
        if (as) {
            if ((rc = launch_ffn_as(ctx, s, FfnP{x, x, w.ln_ff_g, w.ln_ff_b, ld->w1, ld->w2, w.b1, w.b2, w.ln_fin_g, w.ln_fin_b, 0.5f, Mi}))) return rc;
            dbg("ffn+ln", l, x, M * D);
            continue;
        }
        g = plain_gemm(x, D, w.w1, D, w.b1, ctx->lm_h, FF, Mi, FF, D, EPI_SILU);
        g.ln_g = w.ln_ff_g; g.ln_b = w.ln_ff_b;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_FFN1))) return rc;
        dbg("ffn1", l, ctx->lm_h, M * FF);
        g = plain_gemm(ctx->lm_h, FF, w.w2, FF, w.b2, x, D, Mi, D, FF, EPI_RESID, 0.5f);
        g.R = x;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_FFN2))) return rc;
        dbg("ffn2", l, x, M * D);
        if ((rc = launch_ln(ctx, s, LnP{x, w.ln_fin_g, w.ln_fin_b, x, Mi, BIG, 0, 0LL, (long long)D}))) return rc;
    }
    // ---- (e) after_norm into the frame buffer + joint.enc_ffn of every new frame ----------------------------------------------------
    if (out_plain) {
        if ((rc = launch_ln(ctx, s, LnP{x, ctx->after_g, ctx->after_b, out_plain, Mi, BIG, 0, 0LL, (long long)D}))) return rc;
    } else if ((rc = emit_frames(ctx, s, x, B, F, fb0, greedy && ctx->use_persistent && ctx->fuse_after_norm))) return rc;
    *handled = true;
    return RNNT_OK;
}

}  // namespace
