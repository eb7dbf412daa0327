// C ABI: rnnt_encoder_chunk (one chunk), the ragged whole-utterance calls, and rnnt_encoder_chunks (whole utterance: the layer-major
// schedule, or its fallback, the wavefront schedule on the caller's stream).  Included by rnnt_api.hip inside extern "C".

int rnnt_encoder_chunk(rnnt_ctx* ctx, const float* fbank_dev, int32_t T, int32_t offset, int32_t required_cache_size,
                       int32_t* frames_out, void* stream) {
    if (!ctx || !fbank_dev) return fail(ctx, RNNT_ERR_ARG, "rnnt_encoder_chunk: null argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunk: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunk: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    if (T < 7 || T > ctx->cfg.max_chunk_frames) return fail(ctx, RNNT_ERR_SHAPE, "chunk of %d frames outside [7, %d]", T, ctx->cfg.max_chunk_frames);
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->n_streams;
    const int tq = sub_len(T);
    ChunkInfo k;
    std::string err;
    if (!ctx->pos.plan(tq, offset, ctx->tcap, k, err)) return fail(ctx, RNNT_ERR_SHAPE, "%s", err.c_str());
    if (ctx->frames_buffered + tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
    int rc;
    if ((rc = run_subsample(ctx, s, fbank_dev, B, T, T, nullptr, 1, ctx->y1, ctx->y2, ctx->x))) return rc;
    for (int l = 0; l < L; ++l)
        if ((rc = run_layer(ctx, s, l, B, tq, k.T2, k.kv_row0, k.pos_start, k.ring_pos, nullptr))) return rc;
    if ((rc = emit_frames(ctx, s, ctx->x, B, tq, ctx->frames_buffered))) return rc;
    ctx->pos.advance(k.T2, tq, required_cache_size);
    ctx->frames_buffered += tq;
    if (frames_out) *frames_out = tq;
    return RNNT_OK;
}

namespace {
// Planning and encoder launches shared by rnnt_decode_ragged and rnnt_encode_ragged: every stream's chunk plan over its own
// lens_host[b] frames, the layer-major launches over the common chunks plus every stream's tail chunk, and the stream state a
// uniform call over the common chunks would leave.  greedy != 0: only enc_proj is formed (the greedy decoder reads nothing else);
// greedy == 0: after_norm frames (encbuf) and enc_proj (encp) of every stream's rows.
int ragged_encode(rnnt_ctx* ctx, const char* who, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                  int greedy, hipStream_t s, RaggedPlan& rg) {
    if (!ctx || !fbank_dev || !lens_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", who);
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "%s: no weights / no streams", who);
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "%s: the slots have positions of their own (stream pool); call rnnt_streams_reset first", who);
    if (ctx->pos.cache_len || ctx->pos.kv_start || ctx->pos.conv_pos || ctx->frames_buffered) return fail(ctx, RNNT_ERR_STATE, "%s needs freshly reset streams", who);
    if (!ctx->use_lm || (greedy && !ctx->use_persistent))
        return fail(ctx, RNNT_ERR_STATE, greedy ? "%s needs the layer-major schedule and the resident decoder" : "%s needs the layer-major schedule", who);
    const int cf = chunk_frames, minc = cf > 16 ? cf : 16;
    if (cf < 7 || cf + minc - 1 > ctx->cfg.max_chunk_frames)
        return fail(ctx, RNNT_ERR_SHAPE, "%s: chunk_frames %d (a merged last chunk has up to %d frames; max_chunk_frames %d)", who, cf, cf + minc - 1, ctx->cfg.max_chunk_frames);
    const int B = ctx->n_streams;
    rg.nb.assign(B, 0); rg.tail.assign(B, ChunkInfo{0, 0, 0, 0, 0, 0, 0, 0}); rg.frames.assign(B, 0);
    int Kmax = 0;
    std::vector<int> tail_len(B, 0);
    for (int b = 0; b < B; ++b) {
        const int T = lens_host[b];
        if (T < 0 || T > total_frames) return fail(ctx, RNNT_ERR_SHAPE, "%s: stream %d has %d of %d frames", who, b, T, total_frames);
        if (T < 7) continue;                                        // shorter than the conv front-end's receptive field: skipped (:356-359)
        int off = 0, n = 0;                                         // the decode script's slicing rule (:87-93)
        while (off < T) {
            int end = off + cf < T ? off + cf : T;
            if (T - end < minc && end < T) end = T;
            if (end >= T) { tail_len[b] = end - off; break; }
            ++n;
            off = end;
        }
        if (n < 1) return fail(ctx, RNNT_ERR_SHAPE, "%s: stream %d (%d frames) is a single chunk; use rnnt_encoder_chunks for it", who, b, T);
        rg.nb[b] = n;
        Kmax = n > Kmax ? n : Kmax;
    }
    if (Kmax < 2) return fail(ctx, RNNT_ERR_SHAPE, "%s: the longest utterance must have at least three chunks", who);
    // the common chunks from the (fresh) context position: offset = required_cache_size = c * (cf / 4)
    std::vector<ChunkInfo> ci(Kmax);
    struct St { SlotPos pos; int fb; };
    std::vector<St> after(Kmax);                                    // the state behind common chunk c
    std::vector<int32_t> starts(Kmax);
    std::string err;
    St st{ctx->pos, ctx->frames_buffered};
    for (int c = 0; c < Kmax; ++c) {
        ChunkInfo& k = ci[c];
        const int offset = c * (cf / 4);
        starts[c] = c * cf;
        k.len = cf; k.fpos = st.fb; k.xoff = 0;
        if (!st.pos.plan(sub_len(cf), offset, ctx->tcap, k, err)) return fail(ctx, RNNT_ERR_SHAPE, "chunk %d: %s", c, err.c_str());
        st.pos.advance(k.T2, k.tq, offset);
        st.fb += k.tq;
        after[c] = st;
    }
    for (int b = 0; b < B; ++b) {
        if (rg.nb[b] < 1) continue;
        const St& sb = after[rg.nb[b] - 1];                         // the stream's tail follows its last common chunk
        rg.frames[b] = sb.fb;
        if (tail_len[b] >= 7) {
            ChunkInfo& k = rg.tail[b];
            k.len = tail_len[b]; k.fpos = sb.fb; k.xoff = 0;
            if (!sb.pos.plan(sub_len(k.len), rg.nb[b] * (cf / 4), ctx->tcap, k, err)) return fail(ctx, RNNT_ERR_SHAPE, "stream %d: last chunk: %s", b, err.c_str());
            rg.frames[b] += k.tq;
        }
        if (rg.frames[b] > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
        rg.F = rg.frames[b] > rg.F ? rg.frames[b] : rg.F;
    }
    int rc;
    bool done = false;
    const std::vector<int> key = {-1};
    if ((rc = encoder_chunks_lm(ctx, s, fbank_dev, total_frames, starts.data(), ci, key, greedy, &done, nullptr, nullptr, &rg))) return rc;
    if (!done) return fail(ctx, RNNT_ERR_STATE, "%s: the layer-major schedule cannot run this plan", who);
    // the state a uniform call over the common chunks would leave (not meaningful for the shorter streams: reset before reuse)
    ctx->pos = after[Kmax - 1].pos;
    ctx->frames_buffered = rg.F;
    return RNNT_OK;
}
}  // namespace

// Greedy decode of a PADDED batch of whole utterances of different lengths in one call (utils/utils.py:29-50 pads a batch,
// online_rnnt_eval.py:86-94 decodes every utterance with its own audio_lens): stream b runs the decode script's chunk loop
// (online_rnnt_decode.py:81-117: chunks of chunk_frames, a remainder shorter than max(16, chunk_frames) merged into the last
// chunk, chunks under 7 frames skipped) over its own lens_host[b] frames, so its tokens are those of a B = 1 run.
// The common full-size chunks run for all streams at once in the layer-major schedule; every stream's last chunk is subsampled
// per tail-length class and takes part in the same launches with its own key window and positional offset (host_lm.hip.inc).
// Needs freshly reset streams; the stream state is not meaningful afterwards (reset before the next call).  Streams whose
// utterance is a single chunk (fewer than chunk_frames + max(16, chunk_frames) frames, but at least 7) are not supported by this
// entry point (RNNT_ERR_SHAPE): run them with rnnt_encoder_chunks.  frames_out [n_streams] (optional): encoder frames per stream.
int rnnt_decode_ragged(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                       int32_t* frames_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    RaggedPlan rg;
    int rc;
    if ((rc = ragged_encode(ctx, "rnnt_decode_ragged", fbank_dev, total_frames, lens_host, chunk_frames, 1, s, rg))) return rc;
    const int B = ctx->n_streams;
    HIPCHK(hipMemcpyAsync(ctx->klen, rg.frames.data(), B * sizeof(int), hipMemcpyHostToDevice, s));   // per-stream frame limits of the decoder
    HIPCHK(hipStreamSynchronize(s));                                // rg.frames dies at scope end
    if ((rc = decode_resident(ctx, s, rg.F, ctx->klen))) return rc;
    ctx->frames_decoded = rg.F;
    if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = rg.frames[b];
    return RNNT_OK;
}

// The planning and encoder launches of rnnt_decode_ragged without the greedy decoder: stream b's frames_out[b] encoder frames
// stay in the frame buffer (encbuf after_norm, encp joint-projected) for rnnt_beam_decode with frame_end_host = frames_out.
// Same preconditions and refusals as rnnt_decode_ragged; does not synchronise.
int rnnt_encode_ragged(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                       int32_t* frames_out, void* stream) {
    RaggedPlan rg;
    int rc;
    if ((rc = ragged_encode(ctx, "rnnt_encode_ragged", fbank_dev, total_frames, lens_host, chunk_frames, 0, (hipStream_t)stream, rg))) return rc;
    if (frames_out) for (int b = 0; b < ctx->n_streams; ++b) frames_out[b] = rg.frames[b];
    return RNNT_OK;
}

namespace {

// ---- rnnt_encoder_chunks in parts -------------------------------------------------------------------------------------------------

// Static schedule: the cursor run over the chunk list from (pos, fb), which end up behind the last chunk.  Nothing of the context changes.
int wf_plan(rnnt_ctx* ctx, int total_frames, int C, const int32_t* chunk_start, const int32_t* chunk_len, const int32_t* offsets,
            const int32_t* required, std::vector<ChunkInfo>& ci, SlotPos& pos, int& fb) {
    std::string err;
    size_t xrows = 0;
    ci.resize(C);
    for (int c = 0; c < C; ++c) {
        ChunkInfo& k = ci[c];
        k.len = chunk_len[c];
        if (k.len < 7 || k.len > ctx->cfg.max_chunk_frames || chunk_start[c] < 0 || chunk_start[c] + k.len > total_frames)
            return fail(ctx, RNNT_ERR_SHAPE, "chunk %d [%d,+%d) invalid for %d frames / max_chunk_frames %d", c, chunk_start[c], k.len,
                        total_frames, ctx->cfg.max_chunk_frames);
        k.fpos = fb;
        k.xoff = xrows;
        if (!pos.plan(sub_len(k.len), offsets[c], ctx->tcap, k, err)) return fail(ctx, RNNT_ERR_SHAPE, "chunk %d: %s", c, err.c_str());
        if (fb + k.tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
        pos.advance(k.T2, k.tq, required[c]);
        fb += k.tq;
        xrows += (size_t)ctx->n_streams * k.tq;
    }
    return RNNT_OK;
}

// per-chunk x rows, per-layer scratch and the subsampling slabs (once per context); the chunk-start table
int wf_buffers(rnnt_ctx* ctx, int C) {
    int rc;
    const size_t Bm = ctx->cfg.max_streams, Mmax = Bm * ctx->tmax;
    const size_t per_chunk = Bm * ctx->t1max * RNNT_F1 * D * sizeof(float);
    // context constants only: the same value on every call, so the wf_y1 / wf_y2 sizes below cannot drift between calls
    ctx->wf_slab = (int)std::min<size_t>(std::max<size_t>((192ull << 20) / per_chunk, 1), 16);
    if ((rc = reserve(ctx, ctx->wf_x, Bm * ctx->fcap * D))) return rc;
    if ((rc = reserve(ctx, ctx->wf_h, (size_t)L * WF_MERGE_MAX * Mmax * FF))) return rc;
    if ((rc = reserve(ctx, ctx->wf_q, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
    if ((rc = reserve(ctx, ctx->wf_a, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
    if ((rc = reserve(ctx, ctx->wf_d, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
    if ((rc = reserve(ctx, ctx->wf_y1, (size_t)ctx->wf_slab * Bm * ctx->t1max * RNNT_F1 * D))) return rc;
    if ((rc = reserve(ctx, ctx->wf_y2, (size_t)ctx->wf_slab * Mmax * RNNT_FSUB * D))) return rc;
    return reserve(ctx, ctx->wf_starts, (size_t)C);
}

// fused schedule (rnnt_fused.hip.h), 3 launches per stage: one FuseItem per active layer + the attention descriptor of every pair
int wf_build_fused(rnnt_ctx* ctx, const std::vector<ChunkInfo>& ci, int NS, std::vector<AttnP>& at, std::vector<FuseItem>& ft) {
    const std::vector<int>& sc_first = ctx->wf_sc_first;
    const int NSC = (int)sc_first.size() - 1, B = ctx->n_streams, Mmax = ctx->cfg.max_streams * ctx->tmax;
    int rc;
    for (int st = 0; st < NS; ++st) {
        int n_items = 0, n_pairs = 0, maxnf = 0, maxtq = 0, maxT2 = 0;
        const int f_off = (int)ft.size(), a_off = (int)at.size();
        for (int l = 0; l < L; ++l) {
            ctx->wf_lstart[st][l] = n_pairs;
            const int sc = st - l;
            if (sc < 0 || sc >= NSC) continue;
            FuseItem it;
            memset(&it, 0, sizeof(it));
            it.layer = l;
            for (int c = sc_first[sc]; c < sc_first[sc + 1]; ++c) {
                const int j = c - sc_first[sc];
                LayerDescs d;
                const size_t slot = (size_t)l * WF_MERGE_MAX + j;
                LayerBufs bf{ctx->wf_x + ci[c].xoff * D, ctx->wf_h, ctx->wf_q + slot * Mmax * D, ctx->wf_a + slot * Mmax * D, ctx->wf_d};
                if ((rc = build_layer(ctx, l, B, ci[c].tq, ci[c].T2, ci[c].kv_row0, ci[c].pos_start, ci[c].ring_pos, nullptr, bf, d))) return rc;
                at.push_back(d.attn);
                it.tq[j] = ci[c].tq; it.f0[j] = it.nf; it.nf += ci[c].tq;
                it.xrow[j] = (long long)ci[c].xoff;
                it.kvrow[j] = ci[c].kv_w0();
                it.ringpos[j] = ci[c].ring_pos;
                it.q[j] = bf.qbuf; it.a[j] = bf.abuf;
                ++it.n_chunks; ++n_pairs;
                if (ci[c].tq > maxtq) maxtq = ci[c].tq;
                if (ci[c].T2 > maxT2) maxT2 = ci[c].T2;
            }
            if (it.nf > maxnf) maxnf = it.nf;
            ft.push_back(it);
            ++n_items;
        }
        ctx->wf_lstart[st][L] = n_pairs;
        ctx->wf_seq.push_back({WF_BLOCK_FRONT, f_off, n_items, maxnf, 0});
        ctx->wf_seq.push_back({WF_ATTN, a_off, n_pairs, maxtq, maxT2});
        ctx->wf_seq.push_back({WF_BLOCK_BACK, f_off, n_items, maxnf, 0});
    }
    return RNNT_OK;
}

// unfused schedule, 11 launches per stage: the descriptors of every pair, grouped by launch
int wf_build_unfused(rnnt_ctx* ctx, const std::vector<ChunkInfo>& ci, int NS, std::vector<GemmP>& gt, std::vector<AttnP>& at,
                     std::vector<DwP>& dt, std::vector<LnP>& lt) {
    const std::vector<int>& sc_first = ctx->wf_sc_first;
    const int NSC = (int)sc_first.size() - 1, B = ctx->n_streams, Mmax = ctx->cfg.max_streams * ctx->tmax;
    std::vector<rnnt_ctx::WfLaunch>& seq = ctx->wf_seq;
    std::vector<LayerDescs> cur;
    int rc;
    for (int st = 0; st < NS; ++st) {
        cur.clear();
        int maxM = 0, maxtq = 0, maxT2 = 0;
        for (int l = 0; l < L; ++l) {
            ctx->wf_lstart[st][l] = (int)cur.size();
            const int sc = st - l;
            if (sc < 0 || sc >= NSC) continue;
            for (int c = sc_first[sc]; c < sc_first[sc + 1]; ++c) {
                LayerDescs d;
                const size_t slot = (size_t)l * WF_MERGE_MAX + (c - sc_first[sc]);
                LayerBufs bf{ctx->wf_x + ci[c].xoff * D, ctx->wf_h + slot * Mmax * FF, ctx->wf_q + slot * Mmax * D,
                             ctx->wf_a + slot * Mmax * D, ctx->wf_d + slot * Mmax * D};
                if ((rc = build_layer(ctx, l, B, ci[c].tq, ci[c].T2, ci[c].kv_row0, ci[c].pos_start, ci[c].ring_pos, nullptr, bf, d))) return rc;
                cur.push_back(d);
                if (B * ci[c].tq > maxM) maxM = B * ci[c].tq;
                if (ci[c].tq > maxtq) maxtq = ci[c].tq;
                if (ci[c].T2 > maxT2) maxT2 = ci[c].T2;
            }
        }
        ctx->wf_lstart[st][L] = (int)cur.size();
        const int n = (int)cur.size();
        auto add_g = [&](WfType type, GemmP LayerDescs::*f) -> int {
            seq.push_back({type, (int)gt.size(), n, maxM, 0});
            for (auto& d : cur) { GemmP g = d.*f; int r2 = prepare_gemm(ctx, g); if (r2) return r2; gt.push_back(g); }
            return 0;
        };
        if ((rc = add_g(WF_FFN1M, &LayerDescs::ffn1m))) return rc;
        if ((rc = add_g(WF_FFN2M, &LayerDescs::ffn2m))) return rc;
        seq.push_back({WF_QKV, (int)gt.size(), 3 * n, maxM, 0});
        for (auto& d : cur)
            for (int i = 0; i < 3; ++i) { GemmP g = d.qkv[i]; if ((rc = prepare_gemm(ctx, g))) return rc; gt.push_back(g); }
        seq.push_back({WF_ATTN, (int)at.size(), n, maxtq, maxT2});
        for (auto& d : cur) at.push_back(d.attn);
        if ((rc = add_g(WF_OUT, &LayerDescs::out))) return rc;
        if ((rc = add_g(WF_PW1, &LayerDescs::pw1))) return rc;
        seq.push_back({WF_DW, (int)dt.size(), n, maxM, 0});
        for (auto& d : cur) dt.push_back(d.dw);
        if ((rc = add_g(WF_PW2, &LayerDescs::pw2))) return rc;
        if ((rc = add_g(WF_FFN1, &LayerDescs::ffn1))) return rc;
        if ((rc = add_g(WF_FFN2, &LayerDescs::ffn2))) return rc;
        seq.push_back({WF_LN, (int)lt.size(), n, maxM, 0});
        for (auto& d : cur) lt.push_back(d.lnf);
    }
    return RNNT_OK;
}

// (b) wavefront tables: the stage sequence (ctx->wf_seq, wf_lstart, wf_sc_first) and the descriptor tables in device memory; `chunks`
// = the call's four chunk arrays.  The same plan from the same state: the tables of the last call are still valid (ctx->wf_key).
// Stage of pair (chunk c, layer l) = c / KM + l: KM consecutive chunks of a layer share a stage.  Everything but
// attention and the depthwise conv is per-frame, and those two only need the SAME layer's K/V rows / ring rows of the
// earlier chunks, which the stage's QKV / pointwise_conv1 launch has written before the attention / depthwise launch
// starts.  Fewer, fatter stages: the fixed cost of a launch (ramp, prologue, epilogue) is paid per 2 chunks.
int wf_build_tables(rnnt_ctx* ctx, hipStream_t s, int total_frames, const std::vector<int>& chunks, const std::vector<ChunkInfo>& ci) {
    const int C = (int)ci.size();
    const auto t_tab0 = std::chrono::steady_clock::now();
    // fused schedule: needs every chunk's frames to fit the depthwise-conv window (exact-f32 mode keeps the unfused schedule
    // unless RNNT_FUSED=2: its fused form is MFMA-bound at 3 row tiles and not tuned)
    bool fused = ctx->use_fused == 2 || (ctx->use_fused == 1 && ctx->numerics != RNNT_NUM_F32);
    for (int c = 0; c < C; ++c) fused = fused && ci[c].tq <= FUSE_MAXF;
    const int fuse_merge = ctx->fuse_merge, fuse_frames = ctx->fuse_frames;
    const int KM = fused ? (fuse_merge < 1 ? 1 : (fuse_merge > FUSE_MAXC ? FUSE_MAXC : fuse_merge)) : ctx->wf_merge;
    std::vector<int> key = {ctx->n_streams, C, KM, total_frames, ctx->pos.cache_len, ctx->pos.kv_start, ctx->pos.conv_pos,
                            ctx->frames_buffered, fused ? 1 + fuse_frames : 0};
    key.insert(key.end(), chunks.begin(), chunks.end());
    if (key == ctx->wf_key) return RNNT_OK;
    std::vector<int>& sc_first = ctx->wf_sc_first;
    ctx->wf_seq.clear(); sc_first.clear();
    ctx->wf_key.clear();
    // A chunk joins its predecessor's stage only if the K/V rows it appends lie behind everything the predecessor reads or
    // writes (the reference re-bases the cache at row 0 after the first chunk, whose K/V are dropped: chunk 1 would overwrite
    // chunk 0's rows inside one launch).
    for (int c = 0, cnt = 0, nfr = 0; c < C; ++c) {
        const bool behind = c > 0 && ci[c].kv_w0() >= ci[c - 1].kv_row0 + ci[c - 1].T2;
        const bool full = fused && nfr + ci[c].tq > (fuse_frames > FUSE_MAXF ? FUSE_MAXF : fuse_frames);   // frames per stream of one tile
        if (c == 0 || cnt == KM || !behind || full) { sc_first.push_back(c); cnt = 0; nfr = 0; }
        ++cnt;
        nfr += ci[c].tq;
    }
    sc_first.push_back(C);
    const int NS = (int)sc_first.size() - 1 + L - 1;         // stages = super-chunks + L - 1
    ctx->wf_lstart.assign((size_t)NS, std::array<int, 13>());   // per stage: first pair index of every layer (+ total)
    std::vector<GemmP> gt; std::vector<AttnP> at; std::vector<DwP> dt; std::vector<LnP> lt; std::vector<FuseItem> ft;
    gt.reserve((size_t)C * L * 12); at.reserve((size_t)C * L); dt.reserve((size_t)C * L); lt.reserve((size_t)C * (L + 1));
    int rc;
    if ((rc = fused ? wf_build_fused(ctx, ci, NS, at, ft) : wf_build_unfused(ctx, ci, NS, gt, at, dt, lt))) return rc;
    if ((rc = reserve(ctx, ctx->wf_gtab, gt.size()))) return rc;
    if ((rc = reserve(ctx, ctx->wf_atab, at.size()))) return rc;
    if ((rc = reserve(ctx, ctx->wf_dtab, dt.size()))) return rc;
    if ((rc = reserve(ctx, ctx->wf_ltab, lt.size()))) return rc;
    if ((rc = reserve(ctx, ctx->wf_ftab, ft.size()))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->wf_gtab, gt.data(), gt.size() * sizeof(GemmP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_atab, at.data(), at.size() * sizeof(AttnP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_dtab, dt.data(), dt.size() * sizeof(DwP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_ltab, lt.data(), lt.size() * sizeof(LnP), hipMemcpyHostToDevice, s));
    if (!ft.empty()) HIPCHK(hipMemcpyAsync(ctx->wf_ftab, ft.data(), ft.size() * sizeof(FuseItem), hipMemcpyHostToDevice, s));
    ctx->wf_fused_plan = fused ? 1 : 0;
    HIPCHK(hipStreamSynchronize(s));   // the host vectors die at return; tables are small (a few MB)
    if (getenv("RNNT_TIMING")) fprintf(stderr, "[rnnt timing] descriptor tables: %.3f ms on the host (%zu GEMM descriptors)\n",
                                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tab0).count(), gt.size());
    ctx->wf_key = key;
    return RNNT_OK;
}

// attention of the stage's pn pairs (tab[0 .. pn)).  The kernel is chosen PER PAIR exactly as rnnt_encoder_chunk chooses it, in runs of
// consecutive pairs: the tail-merged last chunk (5 frames) does not switch its whole stage to the tiled kernel
int wf_attention(rnnt_ctx* ctx, hipStream_t s, int st, const std::vector<ChunkInfo>& ci, const AttnP* tab, int pn) {
    ProfScope prof(ctx, s, TAG_ATTN);
    const int attn_pair_major = ctx->attn_pair_major;
    const std::vector<int>& sc_first = ctx->wf_sc_first;
    const int NSC = (int)sc_first.size() - 1, B = ctx->n_streams;
    std::vector<const ChunkInfo*> pq;                       // the stage's pairs in table order: layer-major
    for (int l = 0; l < L; ++l) {
        const int sc = st - l;
        if (sc < 0 || sc >= NSC) continue;
        for (int c = sc_first[sc]; c < sc_first[sc + 1]; ++c) pq.push_back(&ci[c]);
    }
    if ((int)pq.size() != pn) return fail(ctx, RNNT_ERR_STATE, "wavefront attention: pair list out of step");
    for (int r0 = 0; r0 < pn;) {
        const bool strm = attn_stream_ok(ctx, pq[r0]->tq, pq[r0]->T2);
        int r1 = r0, mtq = 0, mT2 = 1;
        while (r1 < pn && attn_stream_ok(ctx, pq[r1]->tq, pq[r1]->T2) == strm) {
            mtq = pq[r1]->tq > mtq ? pq[r1]->tq : mtq;
            mT2 = pq[r1]->T2 > mT2 ? pq[r1]->T2 : mT2;
            ++r1;
        }
        const int nr = r1 - r0;
        if (strm) {
            const int cap = attn_t2cap(mT2);
            hipLaunchKernelGGL(rel_attention_stream_tab, dim3((B * RNNT_H + 7) / 8 * 8 * nr), dim3(256), attn_stream_lds(cap), s,
                               tab + r0, cap, nr, B * RNNT_H, attn_pair_major);
            LAUNCHCHK("rel_attention_stream_tab");
        } else {
            LAUNCH_ATTN_TILED(rel_attention_tab, s, B * RNNT_H, mtq, nr, tab + r0);
        }
        r0 = r1;
    }
    return RNNT_OK;
}

// the launches of stage st: every active layer's pairs [p0, p0 + pn) of the stage, on the caller's stream
int wf_run_stage(rnnt_ctx* ctx, hipStream_t s, int st, const std::vector<ChunkInfo>& ci) {
    static const int gN[WF_FFN2 + 1] = {FF, D, D, D, 2 * D, D, FF, D};
    static const int gK[WF_FFN2 + 1] = {D, FF, D, D, D, D, D, FF};
    static const int gTag[WF_FFN2 + 1] = {TAG_FFN1, TAG_FFN2, TAG_QKV, TAG_ATTN_OUT, TAG_PW1, TAG_PW2, TAG_FFN1, TAG_FFN2};
    const std::array<int, 13>& ls = ctx->wf_lstart[st];
    const int p0 = ls[0], pn = ls[L] - ls[0], B = ctx->n_streams;
    if (pn <= 0) return RNNT_OK;
    const int nper = ctx->wf_fused_plan ? 3 : 11;
    int rc;
    for (int j = 0; j < nper; ++j) {
        const rnnt_ctx::WfLaunch& q = ctx->wf_seq[(size_t)st * nper + j];
        switch (q.type) {
            case WF_BLOCK_FRONT: case WF_BLOCK_BACK: {
                const bool back = q.type == WF_BLOCK_BACK;
                if ((rc = launch_fused(ctx, s, back, ctx->wf_ftab + q.off, q.n, q.maxM, B, back ? TAG_BLOCK_BACK : TAG_BLOCK_FRONT))) return rc;
                break;
            }
            case WF_ATTN:
                if ((rc = wf_attention(ctx, s, st, ci, ctx->wf_atab + q.off + p0, pn))) return rc;
                break;
            case WF_DW: {
                ProfScope prof(ctx, s, TAG_DWCONV);
                hipLaunchKernelGGL(dwconv_bn_silu_tab, dim3(grid_for((long long)q.maxM * D), 1, pn), dim3(256), 0, s, ctx->wf_dtab + q.off + p0);
                LAUNCHCHK("dwconv_bn_silu_tab");
                break;
            }
            case WF_LN:
                hipLaunchKernelGGL(layer_norm_tab, dim3((q.maxM + 3) / 4, 1, pn), dim3(256), 0, s, ctx->wf_ltab + q.off + p0);
                LAUNCHCHK("layer_norm_tab");
                break;
            default: {                                          // the GEMM shape classes WF_FFN1M .. WF_FFN2
                const int mult = q.type == WF_QKV ? 3 : 1;
                if ((rc = launch_gemm_tab(ctx, s, ctx->wf_gtab + q.off + mult * p0, mult * pn, q.maxM, gN[q.type], gK[q.type], gTag[q.type]))) return rc;
            }
        }
    }
    return RNNT_OK;
}

// decoder step behind a stage that finished chunks: frames [0, ready) are there, n_new of them new.  The overlapped resident decoder is
// told so; else (no stream overlap here, or RNNT_PERSISTENT=0) the decode stream runs hipGraph step batches behind the event e
int wf_decode_stage(rnnt_ctx* ctx, hipStream_t s, hipStream_t s2, bool resident, hipEvent_t e, int ready, int n_new, int& dec_steps) {
    if (resident) {
        hipLaunchKernelGGL(publish_frames, dim3(1), dim3(1), 0, s, ctx->dec_ctrl, ready);
        LAUNCHCHK("publish_frames");
        return RNNT_OK;
    }
    HIPCHK(hipEventRecord(e, s));
    HIPCHK(hipStreamWaitEvent(s2, e, 0));
    const int slack = ctx->dec_slack;
    const int budget = (n_new + slack + 3) / 4 * 4;   // the stage's frames + a little slack; few distinct graph sizes
    dec_steps += budget;
    return greedy_steps(ctx, s2, budget, ready);
}

}  // namespace

// Whole-utterance encoder: every chunk of every stream, same results as n_chunks calls of rnnt_encoder_chunk.  The layer-major
// schedule (host_lm.hip.inc) where it can run the plan, else (a cache reset in the middle of the call, RNNT_LM=0) the WAVEFRONT:
// (a) subsampling batched over runs of equal-length chunks; (b) wavefront over (chunk c, layer l): stage s runs
// all pairs with c + l = s as ONE grouped launch per kernel type (layer l of chunk c needs only layer l-1 of
// chunk c and layer l's K/V + conv caches after chunk c-1), so the dependent-launch chain is
// (n_chunks + 11) stages instead of 12 * n_chunks; (c) after_norm + joint.enc_ffn for the frames of every finished chunk.
// The stages run on the caller's stream; only the subsampling (side stream) and the greedy decoder (decode stream) run beside them.
int rnnt_encoder_chunks(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, int32_t n_chunks, const int32_t* chunk_start,
                        const int32_t* chunk_len, const int32_t* offsets, const int32_t* required, int32_t greedy, int32_t* frames_out,
                        void* stream) {
    if (!ctx || !fbank_dev || !chunk_start || !chunk_len || !offsets || !required || n_chunks < 1)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_encoder_chunks: bad argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunks: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunks: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->n_streams, C = n_chunks;
    int rc;
    // ---- plan and buffers: nothing of the context's state changes before every chunk is accepted ----------------------------------
    std::vector<ChunkInfo> ci;
    SlotPos pos = ctx->pos;
    const int fb0 = ctx->frames_buffered;
    int fb = fb0;
    if ((rc = wf_plan(ctx, total_frames, C, chunk_start, chunk_len, offsets, required, ci, pos, fb))) return rc;
    if ((rc = wf_buffers(ctx, C))) return rc;
    std::vector<int> chunks;                                // the tail of both plan-cache keys
    for (const int32_t* a : {chunk_start, chunk_len, offsets, required}) chunks.insert(chunks.end(), a, a + C);
    // ---- layer-major schedule ----------------------------------------------------------------------------------------------------
    {
        std::vector<int> lkey = {B, C, total_frames, ctx->pos.cache_len, ctx->pos.kv_start, ctx->pos.conv_pos, fb0, ctx->tcap};
        lkey.insert(lkey.end(), chunks.begin(), chunks.end());
        bool lm_done = false;
        if ((rc = encoder_chunks_lm(ctx, s, fbank_dev, total_frames, chunk_start, ci, lkey, greedy, &lm_done))) return rc;
        if (lm_done) {
            if (frames_out) *frames_out = fb - fb0;
            ctx->pos = pos; ctx->frames_buffered = fb;
            if (!greedy) return RNNT_OK;                                // else decode: nothing else is running, no overlap probe needed
            if ((rc = ctx->use_persistent ? decode_resident(ctx, s, fb) : greedy_drain(ctx, s, fb, 0))) return rc;
            ctx->frames_decoded = fb;
            return RNNT_OK;
        }
    }
    // ---- wavefront, (a) subsampling in slabs of equal-length chunks, on the side stream (RNNT_WF_SUB_ASYNC, the default: the big-M,
    //      MFMA-bound conv2 runs under the latency-bound stages, the first frames reach the decoder ~4 ms earlier) or in line -------
    // events: [c] the side-stream slab that starts at chunk c, [C] / [C + 1] its fork / join, [C + 2 + c] chunk c's frames are there
    // (launched decode path), [2C + 2] fork / join of the decode stream
    while ((int)ctx->ev_pool.size() < 2 * C + 3) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ev_pool.push_back(e);
    }
    const std::vector<hipEvent_t>& ev = ctx->ev_pool;
    if (ctx->wf_sub_async && !ctx->sub_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->sub_stream, hipStreamNonBlocking));
    hipStream_t ss = ctx->wf_sub_async ? ctx->sub_stream : s;
    if (ss != s) {                                          // fork: behind everything the caller enqueued before this call
        HIPCHK(hipEventRecord(ev[C], s));
        HIPCHK(hipStreamWaitEvent(ss, ev[C], 0));
    }
    HIPCHK(hipMemcpyAsync(ctx->wf_starts, chunk_start, C * sizeof(int), hipMemcpyHostToDevice, ss));
    std::vector<char> slab_first(C, 0);                     // chunk c starts a slab of the side stream: layer 0 waits for ev[c]
    for (int c0 = 0; c0 < C;) {
        int c1 = c0 + 1;
        const int slab = (c0 == 0 && ss != s) ? (ctx->wf_slab < 4 ? ctx->wf_slab : 4) : ctx->wf_slab;   // a short first slab: stage 0 starts sooner
        while (c1 < C && ci[c1].len == ci[c0].len && c1 - c0 < slab) ++c1;
        if ((rc = run_subsample(ctx, ss, fbank_dev, B, total_frames, ci[c0].len, ctx->wf_starts + c0, c1 - c0, ctx->wf_y1, ctx->wf_y2,
                                ctx->wf_x + ci[c0].xoff * D)))
            return rc;
        if (ss != s) { HIPCHK(hipEventRecord(ev[c0], ss)); slab_first[c0] = 1; }
        c0 = c1;
    }
    if ((rc = wf_build_tables(ctx, s, total_frames, chunks, ci))) return rc;
    const std::vector<int>& sc_first = ctx->wf_sc_first;
    const int NS = (int)sc_first.size() - 1 + L - 1;
    // ---- decoder start (greedy != 0): the resident decoder on the decode stream beside the stages; or, where greedy_multi owns every
    //      CU, behind them on the caller's stream (multi_seq; its chain is ~5x shorter); or launched step batches behind every stage ----
    hipStream_t s2 = s;
    bool resident = false, multi_seq = false;
    int dec_steps = 0;
    if (greedy) {
        if (!ctx->dec_stream) {   // decode = the latency-critical dependent chain: highest stream priority (own hardware queue)
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK(hipStreamCreateWithPriority(&ctx->dec_stream, hipStreamNonBlocking, hi));
        }
        s2 = ctx->dec_stream;
        ctx->pinned[8] = 0;
        if (ctx->use_persistent && ctx->overlap_ok < 0) {   // the resident decoder must not block ANY stream the encoder uses
            if ((rc = probe_overlap(ctx, s, s2))) return rc;
            if (ss != s && ctx->overlap_ok == 1 && (rc = probe_overlap(ctx, ss, s2))) return rc;
        }
        resident = ctx->use_persistent && ctx->overlap_ok == 1;
        multi_seq = resident && multi_decoder_ok(ctx, ctx->n_streams);
        if (resident && !multi_seq && (rc = init_decoder_ctrl(ctx, s, fb0))) return rc;
        HIPCHK(hipEventRecord(ev[2 * C + 2], s));          // everything enqueued before this call (reset, earlier decode)
        HIPCHK(hipStreamWaitEvent(s2, ev[2 * C + 2], 0));
        if (resident && !multi_seq && (rc = launch_persistent_decoder(ctx, s2, fb))) return rc;
    }
    // ---- (b) stages; (c) the frames of the super-chunk whose last block just ran go out and to the decoder -------------------------
    static const bool timing = getenv("RNNT_TIMING") != nullptr;
    double t_enc = 0, t_dec = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tl = now();
    for (int st = 0; st < NS; ++st) {
        if (ctx->wf_lstart[st][1] > ctx->wf_lstart[st][0])   // layer 0 runs: its chunks' slabs are subsampled
            for (int c = sc_first[st]; c < sc_first[st + 1]; ++c)
                if (slab_first[c]) HIPCHK(hipStreamWaitEvent(s, ev[c], 0));
        if ((rc = wf_run_stage(ctx, s, st, ci))) return rc;
        const int scl = st - (L - 1);
        if (scl < 0) continue;
        int stage_frames = 0;
        for (int c = sc_first[scl]; c < sc_first[scl + 1]; ++c) {
            if ((rc = emit_frames(ctx, s, ctx->wf_x + ci[c].xoff * D, B, ci[c].tq, ci[c].fpos, resident && ctx->fuse_after_norm))) return rc;
            stage_frames += ci[c].tq;
        }
        if (timing) { double t = now(); t_enc += t - tl; tl = t; }
        const int c_last = sc_first[scl + 1] - 1;
        if (c_last < sc_first[scl] || !greedy || multi_seq) continue;   // multi_seq: the decoder starts after the last stage
        if ((rc = wf_decode_stage(ctx, s, s2, resident, ev[C + 2 + c_last], ci[c_last].fpos + ci[c_last].tq, stage_frames, dec_steps))) return rc;
        if (timing && !resident) { double t = now(); t_dec += t - tl; tl = t; }
    }
    if (timing) fprintf(stderr, "[rnnt timing] host enqueue: encoder stages %.2f ms, decode batches %.2f ms\n", t_enc, t_dec);
    if (frames_out) *frames_out = fb - fb0;
    ctx->pos = pos; ctx->frames_buffered = fb;
    if (ss != s) {                                          // join: the caller's stream continues behind the side stream
        HIPCHK(hipEventRecord(ev[C + 1], ss));
        HIPCHK(hipStreamWaitEvent(s, ev[C + 1], 0));
    }
    // ---- decoder end: both waits synchronise the decode stream (=> the encoder is done too); the caller's stream continues behind it ----
    if (!greedy) return RNNT_OK;
    if (multi_seq) {
        if ((rc = decode_resident(ctx, s, fb))) return rc;                // every frame is there
    } else {
        if (resident && timing) (void)hipStreamSynchronize(s);
        const double t_e = now();
        if ((rc = resident ? finish_persistent_decoder(ctx, s2) : greedy_drain(ctx, s2, fb, dec_steps))) return rc;
        if (resident && timing) fprintf(stderr, "[rnnt timing] decoder finished %.3f ms after the encoder streams drained\n", now() - t_e);
        HIPCHK(hipEventRecord(ev[2 * C + 2], s2));
        HIPCHK(hipStreamWaitEvent(s, ev[2 * C + 2], 0));
    }
    ctx->frames_decoded = fb;
    return RNNT_OK;
}
