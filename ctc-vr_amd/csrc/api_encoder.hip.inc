// C ABI: rnnt_encoder_chunk (one chunk) and rnnt_encoder_chunks (whole utterance: wavefront schedule on several streams).
// Included by rnnt_api.hip inside extern "C".

int rnnt_encoder_chunk(rnnt_ctx* ctx, const float* fbank_dev, int32_t T, int32_t offset, int32_t required_cache_size,
                       int32_t* frames_out, void* stream) {
    if (!ctx || !fbank_dev) return fail(ctx, RNNT_ERR_ARG, "rnnt_encoder_chunk: null argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunk: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunk: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    if (T < 7 || T > ctx->cfg.max_chunk_frames) return fail(ctx, RNNT_ERR_SHAPE, "chunk of %d frames outside [7, %d]", T, ctx->cfg.max_chunk_frames);
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->n_streams;
    const int tq = sub_len(T);
    const int T2 = ctx->cache_len + tq;                 // attention_key_size (encoder.py:256)
    const int pos_start = offset - ctx->cache_len;      // encoder.py:257
    if (pos_start < 0 || pos_start + T2 > RNNT_PE_LEN)
        return fail(ctx, RNNT_ERR_SHAPE, "positional window [%d, %d) outside the 5000-entry table", pos_start, pos_start + T2);
    if (ctx->kv_start + T2 > ctx->tcap) return fail(ctx, RNNT_ERR_SHAPE, "K/V cache capacity %d exceeded", ctx->tcap);
    if (ctx->frames_buffered + tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
    int rc;
    if ((rc = run_subsample(ctx, s, fbank_dev, B, T, T, nullptr, 1, ctx->y1, ctx->y2, ctx->x))) return rc;
    for (int l = 0; l < L; ++l)
        if ((rc = run_layer(ctx, s, l, B, tq, T2, ctx->kv_start, pos_start, ctx->conv_pos, nullptr))) return rc;
    // after_norm straight into the frame buffer, then the joint's encoder projection for the new frames
    if ((rc = launch_ln(ctx, s, LnP{ctx->x, ctx->after_g, ctx->after_b, ctx->encbuf, B * tq, tq, ctx->frames_buffered,
                                    (long long)ctx->fstride * D, (long long)D}))) return rc;
    {
        GemmP g = plain_gemm(ctx->encbuf + (size_t)ctx->frames_buffered * D, D, ctx->wenc, D, ctx->benc, ctx->encp, D, B * tq, D, D);
        g.a_n1 = tq; g.a_n2 = tq; g.a_s0 = (long long)ctx->fstride * D; g.a_s1 = 0; g.a_s2 = D;
        g.c_n = tq; g.c_s0 = (long long)ctx->fstride * D; g.c_r0 = ctx->frames_buffered; g.c_mod = BIG; g.c_s1 = D;
        if ((rc = launch_gemm(ctx, s, 0, &g, 1, TAG_ENC_PROJ))) return rc;
    }
    // cache bookkeeping (encoder.py:259-264,288)
    int next_start;
    if (required_cache_size < 0) next_start = 0;
    else if (required_cache_size == 0) next_start = T2;
    else next_start = T2 - required_cache_size > 0 ? T2 - required_cache_size : 0;
    ctx->kv_start += next_start;
    ctx->cache_len = T2 - next_start;
    if (ctx->cache_len == 0) ctx->kv_start = 0;
    ctx->conv_pos += tq;
    ctx->frames_buffered += tq;
    if (frames_out) *frames_out = tq;
    return RNNT_OK;
}

namespace {
// Planning and encoder launches shared by rnnt_decode_ragged and rnnt_encode_ragged: every stream's chunk plan over its own
// lens_host[b] frames, the layer-major launches over the common chunks plus every stream's tail chunk, and the stream state a
// uniform call over the common chunks would leave.  greedy != 0: only enc_proj is formed (the greedy decoder reads nothing else);
// greedy == 0: after_norm frames (encbuf) and enc_proj (encp) of every stream's rows.  The caller has checked the context state.
int ragged_encode(rnnt_ctx* ctx, const char* who, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                  int greedy, hipStream_t s, RaggedPlan& rg) {
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
    // the reference's per-chunk bookkeeping (encoder.py:254-264) for the common chunks: offset = required_cache_size = c * (cf / 4)
    std::vector<ChunkInfo> ci(Kmax);
    struct St { int cache_len, kv_start, conv_pos, fb; };
    std::vector<St> after(Kmax);
    std::vector<int32_t> starts(Kmax);
    {
        int cache_len = 0, kv_start = 0, conv_pos = 0, fb = 0;
        for (int c = 0; c < Kmax; ++c) {
            ChunkInfo& k = ci[c];
            const int offset = c * (cf / 4);
            starts[c] = c * cf;
            k.len = cf; k.tq = sub_len(cf); k.T2 = cache_len + k.tq; k.pos_start = offset - cache_len; k.kv_row0 = kv_start;
            k.ring_pos = conv_pos; k.fpos = fb; k.xoff = 0;
            if (k.pos_start < 0 || k.pos_start + k.T2 > RNNT_PE_LEN) return fail(ctx, RNNT_ERR_SHAPE, "chunk %d: positional window outside the table", c);
            if (kv_start + k.T2 > ctx->tcap) return fail(ctx, RNNT_ERR_SHAPE, "K/V cache capacity %d exceeded", ctx->tcap);
            const int next_start = offset == 0 ? k.T2 : (k.T2 - offset > 0 ? k.T2 - offset : 0);
            kv_start += next_start;
            cache_len = k.T2 - next_start;
            if (cache_len == 0) kv_start = 0;
            conv_pos += k.tq;
            fb += k.tq;
            after[c] = St{cache_len, kv_start, conv_pos, fb};
        }
    }
    for (int b = 0; b < B; ++b) {
        if (rg.nb[b] < 1) continue;
        const St& st = after[rg.nb[b] - 1];
        rg.frames[b] = st.fb;
        if (tail_len[b] >= 7) {
            ChunkInfo& k = rg.tail[b];
            const int offset = rg.nb[b] * (cf / 4);
            k.len = tail_len[b]; k.tq = sub_len(k.len); k.T2 = st.cache_len + k.tq; k.pos_start = offset - st.cache_len; k.kv_row0 = st.kv_start;
            k.ring_pos = st.conv_pos; k.fpos = st.fb; k.xoff = 0;
            if (k.pos_start < 0 || k.pos_start + k.T2 > RNNT_PE_LEN) return fail(ctx, RNNT_ERR_SHAPE, "stream %d: positional window of the last chunk outside the table", b);
            if (st.kv_start + k.T2 > ctx->tcap) return fail(ctx, RNNT_ERR_SHAPE, "K/V cache capacity %d exceeded", ctx->tcap);
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
    ctx->cache_len = after[Kmax - 1].cache_len; ctx->kv_start = after[Kmax - 1].kv_start; ctx->conv_pos = after[Kmax - 1].conv_pos;
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
    if (!ctx || !fbank_dev || !lens_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_decode_ragged: null argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_decode_ragged: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_decode_ragged: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    if (ctx->cache_len || ctx->kv_start || ctx->conv_pos || ctx->frames_buffered)
        return fail(ctx, RNNT_ERR_STATE, "rnnt_decode_ragged needs freshly reset streams");
    if (!ctx->use_lm || !ctx->use_persistent) return fail(ctx, RNNT_ERR_STATE, "rnnt_decode_ragged needs the layer-major schedule and the resident decoder");
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->n_streams;
    RaggedPlan rg;
    int rc;
    if ((rc = ragged_encode(ctx, "rnnt_decode_ragged", fbank_dev, total_frames, lens_host, chunk_frames, 1, s, rg))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->klen, rg.frames.data(), B * sizeof(int), hipMemcpyHostToDevice, s));   // per-stream frame limits of the decoder
    HIPCHK(hipStreamSynchronize(s));                                // rg.frames dies at scope end
    if ((rc = init_decoder_ctrl(ctx, s, rg.F))) return rc;
    if ((rc = launch_persistent_decoder(ctx, s, rg.F, 0, ctx->klen))) return rc;
    if ((rc = finish_persistent_decoder(ctx, s))) return rc;
    ctx->frames_decoded = rg.F;
    if (frames_out) for (int b = 0; b < B; ++b) frames_out[b] = rg.frames[b];
    return RNNT_OK;
}

// The planning and encoder launches of rnnt_decode_ragged without the greedy decoder: stream b's frames_out[b] encoder frames
// stay in the frame buffer (encbuf after_norm, encp joint-projected) for rnnt_beam_decode with frame_end_host = frames_out.
// Same preconditions and refusals as rnnt_decode_ragged; does not synchronise.
int rnnt_encode_ragged(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                       int32_t* frames_out, void* stream) {
    if (!ctx || !fbank_dev || !lens_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_encode_ragged: null argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_encode_ragged: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_encode_ragged: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    if (ctx->cache_len || ctx->kv_start || ctx->conv_pos || ctx->frames_buffered)
        return fail(ctx, RNNT_ERR_STATE, "rnnt_encode_ragged needs freshly reset streams");
    if (!ctx->use_lm) return fail(ctx, RNNT_ERR_STATE, "rnnt_encode_ragged needs the layer-major schedule");
    RaggedPlan rg;
    int rc;
    if ((rc = ragged_encode(ctx, "rnnt_encode_ragged", fbank_dev, total_frames, lens_host, chunk_frames, 0, (hipStream_t)stream, rg))) return rc;
    if (frames_out) for (int b = 0; b < ctx->n_streams; ++b) frames_out[b] = rg.frames[b];
    return RNNT_OK;
}

// Whole-utterance encoder: every chunk of every stream, same results as n_chunks calls of rnnt_encoder_chunk.
// (a) subsampling batched over runs of equal-length chunks; (b) WAVEFRONT over (chunk c, layer l): stage s runs
// all pairs with c + l = s as ONE grouped launch per kernel type (layer l of chunk c needs only layer l-1 of
// chunk c and layer l's K/V + conv caches after chunk c-1), so the dependent-launch chain is
// (n_chunks + 11) stages instead of 12 * n_chunks; (c) after_norm + joint.enc_ffn for all new frames at once.
int rnnt_encoder_chunks(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, int32_t n_chunks, const int32_t* chunk_start,
                        const int32_t* chunk_len, const int32_t* offsets, const int32_t* required, int32_t greedy, int32_t* frames_out,
                        void* stream) {
    if (!ctx || !fbank_dev || !chunk_start || !chunk_len || !offsets || !required || n_chunks < 1)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_encoder_chunks: bad argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunks: no weights / no streams");
    if (ctx->pool_mode) return fail(ctx, RNNT_ERR_STATE, "rnnt_encoder_chunks: the slots have positions of their own (stream pool); call rnnt_streams_reset first");
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->n_streams, C = n_chunks;
    const int Mmax = ctx->cfg.max_streams * ctx->tmax;
    int rc;
    // ---- static schedule: simulate the reference's per-chunk bookkeeping (encoder.py:254-264) -------------
    using CI = ChunkInfo;
    std::vector<CI> ci(C);
    int cache_len = ctx->cache_len, kv_start = ctx->kv_start, conv_pos = ctx->conv_pos, fb = ctx->frames_buffered;
    size_t xrows = 0;
    for (int c = 0; c < C; ++c) {
        CI& k = ci[c];
        k.len = chunk_len[c];
        if (k.len < 7 || k.len > ctx->cfg.max_chunk_frames || chunk_start[c] < 0 || chunk_start[c] + k.len > total_frames)
            return fail(ctx, RNNT_ERR_SHAPE, "chunk %d [%d,+%d) invalid for %d frames / max_chunk_frames %d", c, chunk_start[c], k.len,
                        total_frames, ctx->cfg.max_chunk_frames);
        k.tq = sub_len(k.len);
        k.T2 = cache_len + k.tq;
        k.pos_start = offsets[c] - cache_len;
        k.kv_row0 = kv_start;
        k.ring_pos = conv_pos;
        k.fpos = fb;
        k.xoff = xrows;
        if (k.pos_start < 0 || k.pos_start + k.T2 > RNNT_PE_LEN) return fail(ctx, RNNT_ERR_SHAPE, "chunk %d: positional window outside the table", c);
        if (kv_start + k.T2 > ctx->tcap) return fail(ctx, RNNT_ERR_SHAPE, "K/V cache capacity %d exceeded", ctx->tcap);
        if (fb + k.tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
        int next_start;
        if (required[c] < 0) next_start = 0;
        else if (required[c] == 0) next_start = k.T2;
        else next_start = k.T2 - required[c] > 0 ? k.T2 - required[c] : 0;
        kv_start += next_start;
        cache_len = k.T2 - next_start;
        if (cache_len == 0) kv_start = 0;
        conv_pos += k.tq;
        fb += k.tq;
        xrows += (size_t)B * k.tq;
    }
    // ---- buffers ------------------------------------------------------------------------------------------------
    if (!ctx->wf_x) {
        const size_t Bm = ctx->cfg.max_streams;
        size_t per_chunk = Bm * ctx->t1max * RNNT_F1 * D * sizeof(float);
        ctx->wf_slab = (int)((192ull << 20) / per_chunk);
        if (ctx->wf_slab < 1) ctx->wf_slab = 1;
        if (ctx->wf_slab > 16) ctx->wf_slab = 16;
        if ((rc = dmalloc(ctx, &ctx->wf_x, Bm * ctx->fcap * D))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_h, (size_t)L * WF_MERGE_MAX * Mmax * FF))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_q, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_a, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_d, (size_t)L * WF_MERGE_MAX * Mmax * D))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_y1, (size_t)ctx->wf_slab * Bm * ctx->t1max * RNNT_F1 * D))) return rc;
        if ((rc = dmalloc(ctx, &ctx->wf_y2, (size_t)ctx->wf_slab * Mmax * RNNT_FSUB * D))) return rc;
    }
    if ((rc = grow(ctx, &ctx->wf_starts, &ctx->wf_starts_cap, (size_t)C))) return rc;
    // ---- layer-major schedule (host_lm.hip.inc): the whole call layer by layer, then the decoder; every plan it cannot run
    //      (a cache reset in the middle of the call) keeps the wavefront schedule below ----------------------------------------
    {
        std::vector<int> lkey = {B, C, total_frames, ctx->cache_len, ctx->kv_start, ctx->conv_pos, ctx->frames_buffered, ctx->tcap};
        lkey.insert(lkey.end(), chunk_start, chunk_start + C); lkey.insert(lkey.end(), chunk_len, chunk_len + C);
        lkey.insert(lkey.end(), offsets, offsets + C); lkey.insert(lkey.end(), required, required + C);
        bool lm_done = false;
        if ((rc = encoder_chunks_lm(ctx, s, fbank_dev, total_frames, chunk_start, ci, lkey, greedy, &lm_done))) return rc;
        if (lm_done) {
            if (frames_out) *frames_out = fb - ctx->frames_buffered;
            ctx->cache_len = cache_len; ctx->kv_start = kv_start; ctx->conv_pos = conv_pos; ctx->frames_buffered = fb;
            if (greedy) {
                if (ctx->use_persistent) {                               // nothing else is running: no overlap probe needed
                    if ((rc = init_decoder_ctrl(ctx, s, fb))) return rc;
                    if ((rc = launch_persistent_decoder(ctx, s, fb))) return rc;
                    if ((rc = finish_persistent_decoder(ctx, s))) return rc;
                } else if ((rc = greedy_drain(ctx, s, fb, 0))) return rc;
                ctx->frames_decoded = fb;
            }
            return RNNT_OK;
        }
    }
    // ---- streams ---------------------------------------------------------------------------------------------------
    // The layers are split into G groups of consecutive layers, one HIP stream each (group 0 = the caller's stream):
    // within a group the stages are stream-ordered; group g+1's stage st+1 waits for group g's stage st (layer lo(g+1)
    // of chunk c needs layer lo(g+1)-1 of the same chunk, nothing else crosses a group).  Kernels of different groups
    // run concurrently, so one group's MFMA phases fill the other's prologue / epilogue / launch ramps, and the
    // subsampling (big-M conv2, MFMA-bound) runs on its own stream under the latency-bound stages instead of in front
    // of them -- the first frames reach the decoder ~4 ms earlier.
    // Split-operand modes run ONE layer group: with two group streams their (much shorter) GEMM kernels overlap the other
    // group's kernels and the encoder output became run-to-run non-deterministic at the 1e-3 level (tools/numerics_probe.py;
    // every cross-group ordering -- RAW and WAR -- enforced by events still left it, full lock step or one group removes
    // it; exact-f32 mode is bit-reproducible with two groups).  Cause not established, so NO mode uses more than one group by
    // default since round 3 (an ordering bug that only the shorter 16-bit kernels expose would be latent in exact f32 too);
    // RNNT_WF_GROUPS / RNNT_WF_GROUPS_16 raise it for experiments.  The wavefront is only the fallback of the layer-major schedule.
    static const int g16 = getenv("RNNT_WF_GROUPS_16") ? atoi(getenv("RNNT_WF_GROUPS_16")) : 1;
    int G = ctx->numerics == RNNT_NUM_F32 ? ctx->wf_groups : (g16 < 1 ? 1 : (g16 > 4 ? 4 : g16));
    {   // the fused schedule (3 launches per stage, decided below from the chunk plan) runs on one stream
        bool fz = ctx->use_fused == 2 || (ctx->use_fused == 1 && ctx->numerics != RNNT_NUM_F32);
        for (int c = 0; c < C; ++c) fz = fz && ci[c].tq <= FUSE_MAXF;
        if (fz) G = 1;
    }
    hipStream_t gs[4] = {s, s, s, s};
    for (int g = 1; g < G; ++g) {
        if (!ctx->grp_stream[g]) HIPCHK(hipStreamCreateWithFlags(&ctx->grp_stream[g], hipStreamNonBlocking));
        gs[g] = ctx->grp_stream[g];
    }
    if (ctx->wf_sub_async && !ctx->sub_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->sub_stream, hipStreamNonBlocking));
    hipStream_t ss = ctx->wf_sub_async ? ctx->sub_stream : s;
    size_t ev_next = 0;
    auto new_event = [&](hipEvent_t* out) -> int {
        if (ev_next == ctx->ev_pool.size()) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->ev_pool.push_back(e);
        }
        *out = ctx->ev_pool[ev_next++];
        return RNNT_OK;
    };
    hipEvent_t e_in;
    if ((rc = new_event(&e_in))) return rc;
    HIPCHK(hipEventRecord(e_in, s));                       // everything the caller enqueued before this call
    for (int g = 0; g < G; ++g)
        if (gs[g] != s) HIPCHK(hipStreamWaitEvent(gs[g], e_in, 0));
    if (ss != s) HIPCHK(hipStreamWaitEvent(ss, e_in, 0));
    // ---- (a) subsampling, runs of equal-length chunks in slabs ------------------------------------------
    HIPCHK(hipMemcpyAsync(ctx->wf_starts, chunk_start, C * sizeof(int), hipMemcpyHostToDevice, ss));
    std::vector<hipEvent_t> slab_ev(C, nullptr);           // set on the first chunk of every slab
    for (int c0 = 0; c0 < C;) {
        int c1 = c0 + 1;
        const int slab = (c0 == 0 && ss != s) ? (ctx->wf_slab < 4 ? ctx->wf_slab : 4) : ctx->wf_slab;   // a short first slab: stage 0 starts sooner
        while (c1 < C && ci[c1].len == ci[c0].len && c1 - c0 < slab) ++c1;
        if ((rc = run_subsample(ctx, ss, fbank_dev, B, total_frames, ci[c0].len, ctx->wf_starts + c0, c1 - c0, ctx->wf_y1, ctx->wf_y2,
                                ctx->wf_x + ci[c0].xoff * D)))
            return rc;
        if (ss != s) {
            if ((rc = new_event(&slab_ev[c0]))) return rc;
            HIPCHK(hipEventRecord(slab_ev[c0], ss));
        }
        c0 = c1;
    }
    using Launch = rnnt_ctx::WfLaunch;
    const auto t_tab0 = std::chrono::steady_clock::now();
    // fused schedule (rnnt_fused.hip.h): 3 launches per stage; needs every chunk's frames to fit the depthwise-conv window
    // (exact-f32 mode keeps the unfused schedule unless RNNT_FUSED=2: its fused form is MFMA-bound at 3 row tiles and not tuned)
    bool fused = ctx->use_fused == 2 || (ctx->use_fused == 1 && ctx->numerics != RNNT_NUM_F32);
    for (int c = 0; c < C; ++c) fused = fused && ci[c].tq <= FUSE_MAXF;
    static const int fuse_merge = getenv("RNNT_FUSE_MERGE") ? atoi(getenv("RNNT_FUSE_MERGE")) : FUSE_MAXC;
    static const int fuse_frames = getenv("RNNT_FUSE_FRAMES") ? atoi(getenv("RNNT_FUSE_FRAMES")) : 12;
    const int KM = fused ? (fuse_merge < 1 ? 1 : (fuse_merge > FUSE_MAXC ? FUSE_MAXC : fuse_merge)) : ctx->wf_merge;
    std::vector<int> key = {B, C, KM, total_frames, ctx->cache_len, ctx->kv_start, ctx->conv_pos, ctx->frames_buffered, fused ? 1 + fuse_frames : 0};
    key.insert(key.end(), chunk_start, chunk_start + C); key.insert(key.end(), chunk_len, chunk_len + C);
    key.insert(key.end(), offsets, offsets + C); key.insert(key.end(), required, required + C);
    std::vector<rnnt_ctx::WfLaunch>& seq = ctx->wf_seq;
    std::vector<std::array<int, 13>>& lstart = ctx->wf_lstart;
    std::vector<int>& sc_first = ctx->wf_sc_first;
    if (key != ctx->wf_key) {                                // same plan from the same state: the device tables are still valid
    seq.clear(); sc_first.clear();
    ctx->wf_key.clear();
    // ---- (b) wavefront tables ---------------------------------------------------------------------------------
    std::vector<GemmP> gt; std::vector<AttnP> at; std::vector<DwP> dt; std::vector<LnP> lt;
    gt.reserve((size_t)C * L * 12); at.reserve((size_t)C * L); dt.reserve((size_t)C * L); lt.reserve((size_t)C * (L + 1));
    // Stage of pair (chunk c, layer l) = c / KM + l: KM consecutive chunks of a layer share a stage.  Everything but
    // attention and the depthwise conv is per-frame, and those two only need the SAME layer's K/V rows / ring rows of the
    // earlier chunks, which the stage's QKV / pointwise_conv1 launch has written before the attention / depthwise launch
    // starts.  Fewer, fatter stages: the fixed cost of a launch (ramp, prologue, epilogue) is paid per 2 chunks.
    // A chunk joins its predecessor's stage only if the K/V rows it appends lie behind everything the predecessor reads or
    // writes (the reference re-bases the cache at row 0 after the first chunk, whose K/V are dropped: chunk 1 would overwrite
    // chunk 0's rows inside one launch).
    for (int c = 0, cnt = 0, nfr = 0; c < C; ++c) {
        const bool behind = c > 0 && ci[c].kv_row0 + ci[c].T2 - ci[c].tq >= ci[c - 1].kv_row0 + ci[c - 1].T2;
        const bool full = fused && nfr + ci[c].tq > (fuse_frames > FUSE_MAXF ? FUSE_MAXF : fuse_frames);   // frames per stream of one tile
        if (c == 0 || cnt == KM || !behind || full) { sc_first.push_back(c); cnt = 0; nfr = 0; }
        ++cnt;
        nfr += ci[c].tq;
    }
    sc_first.push_back(C);
    const int NSC = (int)sc_first.size() - 1;                // super-chunks
    const int NS = NSC + L - 1;                              // stages
    std::vector<LayerDescs> cur;
    std::vector<FuseItem> ft;
    lstart.assign((size_t)NS, std::array<int, 13>());       // per stage: first pair index of every layer (+ total)
    for (int st = 0; st < NS && fused; ++st) {
        // fused schedule: per stage one FuseItem per active layer + the attention descriptor of every (chunk, layer) pair
        int n_items = 0, n_pairs = 0, maxnf = 0, maxtq = 0, maxT2 = 0;
        const int f_off = (int)ft.size(), a_off = (int)at.size();
        for (int l = 0; l < L; ++l) {
            lstart[st][l] = n_pairs;
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
                it.kvrow[j] = ci[c].kv_row0 + ci[c].T2 - ci[c].tq;
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
        lstart[st][L] = n_pairs;
        seq.push_back({20, f_off, n_items, maxnf, 0});
        seq.push_back({10, a_off, n_pairs, maxtq, maxT2});
        seq.push_back({21, f_off, n_items, maxnf, 0});
    }
    for (int st = 0; st < NS && !fused; ++st) {
        cur.clear();
        int maxM = 0, maxtq = 0, maxT2 = 0;
        for (int l = 0; l < L; ++l) {
            lstart[st][l] = (int)cur.size();
            const int sc = st - l;
            if (sc < 0 || sc >= NSC) continue;
            for (int c = sc_first[sc]; c < sc_first[sc + 1]; ++c) {
                const int j = c - sc_first[sc];
                LayerDescs d;
                const size_t slot = (size_t)l * WF_MERGE_MAX + j;
                LayerBufs bf{ctx->wf_x + ci[c].xoff * D, ctx->wf_h + slot * Mmax * FF, ctx->wf_q + slot * Mmax * D,
                             ctx->wf_a + slot * Mmax * D, ctx->wf_d + slot * Mmax * D};
                if ((rc = build_layer(ctx, l, B, ci[c].tq, ci[c].T2, ci[c].kv_row0, ci[c].pos_start, ci[c].ring_pos, nullptr, bf, d))) return rc;
                cur.push_back(d);
                if (B * ci[c].tq > maxM) maxM = B * ci[c].tq;
                if (ci[c].tq > maxtq) maxtq = ci[c].tq;
                if (ci[c].T2 > maxT2) maxT2 = ci[c].T2;
            }
        }
        lstart[st][L] = (int)cur.size();
        const int n = (int)cur.size();
        auto add_g = [&](int type, GemmP LayerDescs::*f) -> int {
            seq.push_back({type, (int)gt.size(), n, maxM, 0});
            for (auto& d : cur) { GemmP g = d.*f; int r2 = prepare_gemm(ctx, g); if (r2) return r2; gt.push_back(g); }
            return 0;
        };
        if ((rc = add_g(0, &LayerDescs::ffn1m))) return rc;
        if ((rc = add_g(1, &LayerDescs::ffn2m))) return rc;
        seq.push_back({2, (int)gt.size(), 3 * n, maxM, 0});
        for (auto& d : cur)
            for (int i = 0; i < 3; ++i) { GemmP g = d.qkv[i]; if ((rc = prepare_gemm(ctx, g))) return rc; gt.push_back(g); }
        seq.push_back({10, (int)at.size(), n, maxtq, maxT2});
        for (auto& d : cur) at.push_back(d.attn);
        if ((rc = add_g(3, &LayerDescs::out))) return rc;
        if ((rc = add_g(4, &LayerDescs::pw1))) return rc;
        seq.push_back({11, (int)dt.size(), n, maxM, 0});
        for (auto& d : cur) dt.push_back(d.dw);
        if ((rc = add_g(5, &LayerDescs::pw2))) return rc;
        if ((rc = add_g(6, &LayerDescs::ffn1))) return rc;
        if ((rc = add_g(7, &LayerDescs::ffn2))) return rc;
        seq.push_back({12, (int)lt.size(), n, maxM, 0});
        for (auto& d : cur) lt.push_back(d.lnf);
    }
    if ((rc = grow(ctx, &ctx->wf_gtab, &ctx->wf_gcap, gt.size()))) return rc;
    if ((rc = grow(ctx, &ctx->wf_atab, &ctx->wf_acap, at.size()))) return rc;
    if ((rc = grow(ctx, &ctx->wf_dtab, &ctx->wf_dcap, dt.size()))) return rc;
    if ((rc = grow(ctx, &ctx->wf_ltab, &ctx->wf_lcap, lt.size()))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->wf_gtab, gt.data(), gt.size() * sizeof(GemmP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_atab, at.data(), at.size() * sizeof(AttnP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_dtab, dt.data(), dt.size() * sizeof(DwP), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->wf_ltab, lt.data(), lt.size() * sizeof(LnP), hipMemcpyHostToDevice, s));
    if ((rc = grow(ctx, &ctx->wf_ftab, &ctx->wf_fcap, ft.size()))) return rc;
    if (!ft.empty()) HIPCHK(hipMemcpyAsync(ctx->wf_ftab, ft.data(), ft.size() * sizeof(FuseItem), hipMemcpyHostToDevice, s));
    ctx->wf_fused_plan = fused ? 1 : 0;
    HIPCHK(hipStreamSynchronize(s));   // the host vectors die at return; tables are small (a few MB)
    if (getenv("RNNT_TIMING")) fprintf(stderr, "[rnnt timing] descriptor tables: %.3f ms on the host (%zu GEMM descriptors)\n",
                                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tab0).count(), gt.size());
    ctx->wf_key = key;
    }
    const int NSC = (int)sc_first.size() - 1, NS = NSC + L - 1;   // super-chunks, stages
    static const int gN[8] = {FF, D, D, D, 2 * D, D, FF, D};
    static const int gK[8] = {D, FF, D, D, D, D, D, FF};
    static const int gTag[8] = {TAG_FFN1, TAG_FFN2, TAG_QKV, TAG_ATTN_OUT, TAG_PW1, TAG_PW2, TAG_FFN1, TAG_FFN2};
    {                                                       // the other streams read the tables copied on s
        hipEvent_t e_tab;
        if ((rc = new_event(&e_tab))) return rc;
        HIPCHK(hipEventRecord(e_tab, s));
        for (int g = 0; g < G; ++g)
            if (gs[g] != s) HIPCHK(hipStreamWaitEvent(gs[g], e_tab, 0));
    }
    hipStream_t sl = gs[G - 1];                             // the stream the last layer runs on
    // decode stream + events (greedy != 0): chunk c's frames are decodable once its layer-11 stage, after_norm and
    // joint.enc_ffn projection are done; the decoder runs on ctx->dec_stream concurrently with later stages.
    hipStream_t s2 = s;
    bool resident = false, multi_seq = false;
    if (greedy) {
        if (!ctx->dec_stream) {   // decode = the latency-critical dependent chain: highest stream priority (own hardware queue)
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIPCHK(hipStreamCreateWithPriority(&ctx->dec_stream, hipStreamNonBlocking, hi));
        }
        s2 = ctx->dec_stream;
        while ((int)ctx->wf_ev.size() < C + 1) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            ctx->wf_ev.push_back(e);
        }
        ctx->pinned[8] = 0;
        if (ctx->use_persistent && ctx->overlap_ok < 0) {   // the resident decoder must not block ANY stream the encoder uses
            if ((rc = probe_overlap(ctx, s, s2))) return rc;
            for (int g = 0; g < G && ctx->overlap_ok == 1; ++g)
                if (gs[g] != s && (rc = probe_overlap(ctx, gs[g], s2))) return rc;
            if (ss != s && ctx->overlap_ok == 1 && (rc = probe_overlap(ctx, ss, s2))) return rc;
        }
        resident = ctx->use_persistent && ctx->overlap_ok == 1;
        // greedy_multi owns every CU (4 per stream, weights in registers / LDS): it cannot share the chip with the encoder
        // stages, so it runs AFTER them on the caller's stream (sequential phases; its chain is ~5x shorter)
        multi_seq = resident && multi_decoder_ok(ctx);
        if (resident && !multi_seq && (rc = init_decoder_ctrl(ctx, s, ctx->frames_buffered))) return rc;
        HIPCHK(hipEventRecord(ctx->wf_ev[C], s));          // everything enqueued before this call (reset, earlier decode)
        HIPCHK(hipStreamWaitEvent(s2, ctx->wf_ev[C], 0));
        if (sl != s) HIPCHK(hipStreamWaitEvent(sl, ctx->wf_ev[C], 0));   // publish_frames comes after the control block's init
        if (resident && !multi_seq && (rc = launch_persistent_decoder(ctx, s2, fb))) return rc;
    }
    int dec_steps = 0;
    const int fb0 = ctx->frames_buffered;
    static const bool timing = getenv("RNNT_TIMING") != nullptr;
    double t_enc = 0, t_dec = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tl = now();
    std::vector<hipEvent_t> grp_ev((size_t)G * (NS + 1), nullptr);   // [g][st]: group g finished its part of stage st
    static const int wf_debug = getenv("RNNT_WF_DEBUG") ? atoi(getenv("RNNT_WF_DEBUG")) : 0;
    for (int st = 0; st < NS; ++st) {
        const std::array<int, 13>& ls = lstart[st];
        for (int g = 0; g < G; ++g) {
            const int lo = g * L / G, hi = (g + 1) * L / G;                                  // layers [lo, hi) of this group
            const int p0 = ls[lo], pn = ls[hi] - ls[lo];                                     // pairs [p0, p0 + pn) of the stage
            if (pn <= 0) continue;
            hipStream_t x = gs[g];
            if (lo == 0 && ls[1] > ls[0])                                                    // layer 0: its chunks' slabs are subsampled
                for (int c = sc_first[st]; c < sc_first[st + 1]; ++c)
                    if (slab_ev[c]) HIPCHK(hipStreamWaitEvent(x, slab_ev[c], 0));
            if (g > 0 && ls[lo + 1] > ls[lo] && st > 0 && grp_ev[(size_t)(g - 1) * (NS + 1) + st - 1])
                HIPCHK(hipStreamWaitEvent(x, grp_ev[(size_t)(g - 1) * (NS + 1) + st - 1], 0));
            const int nper = ctx->wf_fused_plan ? 3 : 11;
            for (int j = 0; j < nper; ++j) {
                const Launch& q = seq[(size_t)st * nper + j];
                if (q.type == 20 || q.type == 21) {
                    if ((rc = launch_fused(ctx, x, q.type == 21, ctx->wf_ftab + q.off, q.n, q.maxM, B, q.type == 21 ? TAG_BLOCK_BACK : TAG_BLOCK_FRONT))) return rc;
                } else if (q.type < 8) {
                    const int mult = q.type == 2 ? 3 : 1;
                    if ((rc = launch_gemm_tab(ctx, x, ctx->wf_gtab + q.off + mult * p0, mult * pn, q.maxM, gN[q.type], gK[q.type], gTag[q.type]))) return rc;
                } else if (q.type == 10) {
                    ProfScope prof(ctx, x, TAG_ATTN);
                    static const int attn_pair_major = getenv("RNNT_ATTN_PAIR_MAJOR") ? atoi(getenv("RNNT_ATTN_PAIR_MAJOR")) : 1;
                    // the kernel is chosen PER PAIR exactly as rnnt_encoder_chunk chooses it (streaming kernel for <= 4 new
                    // frames, LDS-tiled otherwise), in runs of consecutive pairs: the tail-merged last chunk (5 frames) no
                    // longer switches its whole stage to the tiled kernel, so a pair's arithmetic is the per-chunk API's
                    struct PairQ { int tq, T2; };
                    std::vector<PairQ> pq;
                    for (int l = lo; l < hi; ++l) {
                        const int sc = st - l;
                        if (sc < 0 || sc >= NSC) continue;
                        for (int c = sc_first[sc]; c < sc_first[sc + 1]; ++c) pq.push_back({ci[c].tq, ci[c].T2});
                    }
                    if ((int)pq.size() != pn) return fail(ctx, RNNT_ERR_STATE, "wavefront attention: pair list out of step");
                    for (int r0 = 0; r0 < pn;) {
                        const bool strm = attn_stream_ok(ctx, pq[r0].tq, pq[r0].T2);
                        int r1 = r0, mtq = 0, mT2 = 1;
                        while (r1 < pn && attn_stream_ok(ctx, pq[r1].tq, pq[r1].T2) == strm) {
                            mtq = pq[r1].tq > mtq ? pq[r1].tq : mtq;
                            mT2 = pq[r1].T2 > mT2 ? pq[r1].T2 : mT2;
                            ++r1;
                        }
                        const AttnP* tab = ctx->wf_atab + q.off + p0 + r0;
                        const int nr = r1 - r0;
                        if (strm) {
                            const int cap = attn_t2cap(mT2);
                            hipLaunchKernelGGL(rel_attention_stream_tab, dim3((B * RNNT_H + 7) / 8 * 8 * nr), dim3(256), attn_stream_lds(cap), x,
                                               tab, cap, nr, B * RNNT_H, attn_pair_major);
                            LAUNCHCHK("rel_attention_stream_tab");
                        } else {
                            const int nq = mtq <= 4 ? 1 : (mtq <= 8 ? 2 : 4);
                            dim3 grid(B * RNNT_H, (mtq + 4 * nq - 1) / (4 * nq), nr);
                            if (nq == 1) hipLaunchKernelGGL(rel_attention_tab<1>, grid, dim3(256), 0, x, tab);
                            else if (nq == 2) hipLaunchKernelGGL(rel_attention_tab<2>, grid, dim3(256), 0, x, tab);
                            else hipLaunchKernelGGL(rel_attention_tab<4>, grid, dim3(256), 0, x, tab);
                            LAUNCHCHK("rel_attention_tab");
                        }
                        r0 = r1;
                    }
                } else if (q.type == 11) {
                    ProfScope prof(ctx, x, TAG_DWCONV);
                    hipLaunchKernelGGL(dwconv_bn_silu_tab, dim3(grid_for((long long)q.maxM * D), 1, pn), dim3(256), 0, x, ctx->wf_dtab + q.off + p0);
                    LAUNCHCHK("dwconv_bn_silu_tab");
                } else {
                    hipLaunchKernelGGL(layer_norm_tab, dim3((q.maxM + 3) / 4, 1, pn), dim3(256), 0, x, ctx->wf_ltab + q.off + p0);
                    LAUNCHCHK("layer_norm_tab");
                }
            }
            if ((wf_debug & 4) && g == 0) {   // DEBUG: group 1 waits for group 0's SAME stage
                hipEvent_t e;
                if ((rc = new_event(&e))) return rc;
                HIPCHK(hipEventRecord(e, x));
                HIPCHK(hipStreamWaitEvent(gs[1], e, 0));
            }
            if ((wf_debug & 8) && g == 1) {   // DEBUG: group 0's next stage waits for group 1's stage
                hipEvent_t e;
                if ((rc = new_event(&e))) return rc;
                HIPCHK(hipEventRecord(e, x));
                HIPCHK(hipStreamWaitEvent(gs[0], e, 0));
            }
            if (wf_debug & 2) {   // DEBUG lock step: every other group waits for this group's stage
                hipEvent_t e;
                if ((rc = new_event(&e))) return rc;
                HIPCHK(hipEventRecord(e, x));
                for (int g2 = 0; g2 < G; ++g2)
                    if (g2 != g) HIPCHK(hipStreamWaitEvent(gs[g2], e, 0));
            }
            if (g < G - 1 && ls[hi] > ls[hi - 1]) {         // the next group's first layer reads this group's last layer
                hipEvent_t e;
                if ((rc = new_event(&e))) return rc;
                HIPCHK(hipEventRecord(e, x));
                grp_ev[(size_t)g * (NS + 1) + st] = e;
            }
        }
        if (wf_debug & 1) HIPCHK(hipDeviceSynchronize());
        const int scl = st - (L - 1);   // super-chunk whose last block just ran
        if (scl < 0) continue;
        int stage_frames = 0, c_last = -1;
        for (int c = sc_first[scl]; c < sc_first[scl + 1]; ++c) {
        // (c) after_norm straight into the frame buffer + joint.enc_ffn projection of the chunk's frames
        if (greedy && resident && ctx->fuse_after_norm) {
            // greedy decode reads only enc_proj: after_norm goes into the projection's LayerNorm prologue and the
            // normalised frames are not materialised (rnnt_get_enc_frames is not defined after such a call)
            const int F = ci[c].tq;
            GemmP g = plain_gemm(ctx->wf_x + ci[c].xoff * D, D, ctx->wenc, D, ctx->benc, ctx->encp, D, B * F, D, D);
            g.ln_g = ctx->after_g; g.ln_b = ctx->after_b;
            g.c_n = F; g.c_s0 = (long long)ctx->fstride * D; g.c_r0 = ci[c].fpos; g.c_mod = BIG; g.c_s1 = D;
            if ((rc = launch_gemm(ctx, sl, 0, &g, 1, TAG_ENC_PROJ))) return rc;
        } else {
            if ((rc = launch_ln(ctx, sl, LnP{ctx->wf_x + ci[c].xoff * D, ctx->after_g, ctx->after_b, ctx->encbuf, B * ci[c].tq, ci[c].tq, ci[c].fpos,
                                             (long long)ctx->fstride * D, (long long)D}))) return rc;
            const int F = ci[c].tq;
            GemmP g = plain_gemm(ctx->encbuf + (size_t)ci[c].fpos * D, D, ctx->wenc, D, ctx->benc, ctx->encp, D, B * F, D, D);
            g.a_n1 = F; g.a_n2 = F; g.a_s0 = (long long)ctx->fstride * D; g.a_s1 = 0; g.a_s2 = D;
            g.c_n = F; g.c_s0 = (long long)ctx->fstride * D; g.c_r0 = ci[c].fpos; g.c_mod = BIG; g.c_s1 = D;
            if ((rc = launch_gemm(ctx, sl, 0, &g, 1, TAG_ENC_PROJ))) return rc;
        }
            stage_frames += ci[c].tq;
            c_last = c;
        }
        if (timing) { double t = now(); t_enc += t - tl; tl = t; }
        if (c_last < 0) continue;
        if (greedy && resident && multi_seq) {
            // nothing to publish: the decoder starts after the last stage
        } else if (greedy && resident) {   // the resident decoder sees the stage's frames as soon as this lands
            hipLaunchKernelGGL(publish_frames, dim3(1), dim3(1), 0, sl, ctx->dec_ctrl, ci[c_last].fpos + ci[c_last].tq);
            LAUNCHCHK("publish_frames");
        } else if (greedy) {
            HIPCHK(hipEventRecord(ctx->wf_ev[c_last], sl));
            HIPCHK(hipStreamWaitEvent(s2, ctx->wf_ev[c_last], 0));
            // launched decode path: this stage's frames + a little slack, in hipGraph-captured batches
            static const int slack = getenv("RNNT_DEC_SLACK") ? atoi(getenv("RNNT_DEC_SLACK")) : 8;
            int budget = stage_frames + slack;
            budget = (budget + 3) / 4 * 4;   // few distinct graph sizes
            if ((rc = greedy_steps(ctx, s2, budget, ci[c_last].fpos + ci[c_last].tq))) return rc;
            dec_steps += budget;
            if (timing) { double t = now(); t_dec += t - tl; tl = t; }
        }
    }
    if (timing) fprintf(stderr, "[rnnt timing] host enqueue: encoder stages %.2f ms, decode batches %.2f ms\n", t_enc, t_dec);
    if (frames_out) *frames_out = fb - fb0;
    ctx->cache_len = cache_len; ctx->kv_start = kv_start; ctx->conv_pos = conv_pos; ctx->frames_buffered = fb;
    // ---- join: the caller's stream continues after every internal stream ---------------------------------------------
    for (int g = 0; g < G; ++g) {
        if (gs[g] == s) continue;
        hipEvent_t e;
        if ((rc = new_event(&e))) return rc;
        HIPCHK(hipEventRecord(e, gs[g]));
        HIPCHK(hipStreamWaitEvent(s, e, 0));
    }
    if (ss != s) {
        hipEvent_t e;
        if ((rc = new_event(&e))) return rc;
        HIPCHK(hipEventRecord(e, ss));
        HIPCHK(hipStreamWaitEvent(s, e, 0));
    }
    if (greedy && resident && multi_seq) {
        if ((rc = init_decoder_ctrl(ctx, s, fb))) return rc;                  // every frame is there
        if ((rc = launch_persistent_decoder(ctx, s, fb))) return rc;
        if ((rc = finish_persistent_decoder(ctx, s))) return rc;
        ctx->frames_decoded = fb;
    } else if (greedy && resident) {
        double t_e = 0;
        if (timing) { (void)hipStreamSynchronize(s); t_e = now(); }
        if ((rc = finish_persistent_decoder(ctx, s2))) return rc;      // synchronises the decode stream (=> encoder done too)
        if (timing) fprintf(stderr, "[rnnt timing] decoder finished %.3f ms after the encoder streams drained\n", now() - t_e);
        ctx->frames_decoded = fb;
        HIPCHK(hipEventRecord(ctx->wf_ev[C], s2));
        HIPCHK(hipStreamWaitEvent(s, ctx->wf_ev[C], 0));
    } else if (greedy) {
        if ((rc = greedy_drain(ctx, s2, fb, dec_steps))) return rc;   // synchronises the decode stream (=> encoder done too)
        ctx->frames_decoded = fb;
        HIPCHK(hipEventRecord(ctx->wf_ev[C], s2));                    // later work on the caller's stream sees the decode
        HIPCHK(hipStreamWaitEvent(s, ctx->wf_ev[C], 0));
    }
    return RNNT_OK;
}
