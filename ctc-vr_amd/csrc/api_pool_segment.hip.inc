// C ABI: segments of the stream pool -- the next utterance in a slot that stays open (rnnt_pool_segment, rnnt_stream_get_segment).
// Included by rnnt_api.hip inside extern "C".  Kernel: rnnt_segment.hip.h.
//
// An endpoint (rnnt_stream_endpoint) says the caller has stopped talking; a segment boundary is what follows it.  The decoders of the
// listed slots start over -- greedy state, beam, both prefix searches, the endpoint counters, the length of the frame history -- and
// what the caller configured stays: the endpoint config, the keep flag, the audio front-end with its carried samples.  keep_encoder
// != 0 is WeNet's continuous decoding (the encoder's caches and position are neither read nor written); keep_encoder == 0 also
// restarts the encoder of the listed slots, which is how a session outlives max_cache_frames and the 5000-entry positional table.
// Cost: ONE async copy of the slot list and ONE launch (pool_segment_reset), for any n and any set of state kinds; no synchronisation.
// Host per slot: PoolSlot::seg -- the segment index and the encoder frames before it, what the caller adds to the segment-relative
// frame indices of the getters.

int rnnt_pool_segment(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, int32_t keep_encoder, void* stream) {
    const char* fn = "rnnt_pool_segment";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "%s: no weights / no streams", fn);
    int rc;
    if ((rc = pool_slots_check(ctx, fn, n, slots_host, ctx->n_streams, "slots"))) return rc;
    if (ctx->frames_buffered != 0) return fail(ctx, RNNT_ERR_STATE, "%s: %d buffered frames (consume or discard them first)", fn, ctx->frames_buffered);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = calltab_alloc(ctx, ctx->seg_tab, (size_t)ctx->cfg.max_streams))) return rc;
    int* tab;
    if ((rc = calltab_fill(ctx, ctx->seg_tab, tab))) return rc;
    memcpy(tab, slots_host, (size_t)n * sizeof(int));
    if ((rc = calltab_send(ctx, ctx->seg_tab, (size_t)n, s))) return rc;
    SegmentP p;
    memset(&p, 0, sizeof(p));
    p.slots = ctx->seg_tab;
    p.h = ctx->h; p.c = ctx->c; p.sel = ctx->sel; p.key = ctx->key; p.fidx = ctx->fidx; p.nsym = ctx->nsym; p.count = ctx->count; p.tok = ctx->tok;
    p.B = ctx->cfg.max_streams; p.blank = ctx->cfg.blank_id;
    p.beam = pool_beam_params(ctx); p.beam_state_slots = ctx->cfg.n_steps + 1;
    p.prefix = pool_prefix_params(ctx); p.prefix_lcap = ctx->cfg.max_cache_frames + 1;
    p.ctc = ctx->pc_state; p.ep_state = ctx->ep_state; p.hs_len = ctx->hs_len;
    p.gring = ctx->gring; p.xring = ctx->xring; p.glu0 = ctx->glu0; p.cap = ctx->cap; p.fresh = keep_encoder ? 0 : 1;
    const int gx = p.fresh ? std::min(grid_for((long long)L * ctx->cap * D), 64) : 1;
    hipLaunchKernelGGL(pool_segment_reset, dim3(gx, n), dim3(256), 0, s, p);
    LAUNCHCHK("pool_segment_reset");
    pool_enter(ctx);
    for (int i = 0; i < n; ++i) {
        PoolSlot& q = ctx->slot[slots_host[i]];
        q.beam_cur = 0; q.beam_lbound = 0; q.prefix_cur = 0;
        q.ctc = SearchSlot{}; q.prefix = SearchSlot{};
        q.hist.len = 0;
        if (p.fresh) q.pos = SlotPos{0, 0, 0};
        q.seg.index += 1;
        q.seg.start = q.seg.frames;
    }
    return RNNT_OK;
}

int rnnt_stream_get_segment(rnnt_ctx* ctx, int32_t slot, int32_t* index_out, int32_t* start_frame_out) {
    if (!ctx) return RNNT_ERR_ARG;
    if (slot < 0 || slot >= ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_segment: slot %d outside [0, %d)", slot, ctx->cfg.max_streams);
    if (index_out) *index_out = ctx->slot[slot].seg.index;
    if (start_frame_out) *start_frame_out = ctx->slot[slot].seg.start;
    return RNNT_OK;
}
