// C ABI: frames that outlive their chunk -- the per-slot encoder-frame history of the stream pool (rnnt_stream_keep_frames,
// rnnt_stream_get_frames) and the second pass over it (rnnt_pool_rescore).  Included by rnnt_api.hip inside extern "C".
// pool_chunk_run checks and appends through pool_hist_check / pool_hist_append_rows (host_launch.hip.inc).
//
// A slot keeps nothing unless asked.  Asked (on a slot that has not advanced), every pool call that encodes it appends its t' compact
// after_norm rows -- the encoder output before the joint projection, what rnnt_get_enc_frames returns -- to an owning device buffer
// [max_cache_frames][256] of the slot: max_cache_frames KB, allocated on the first keep, reused by the slot's later utterances, freed
// with the context.  The device finds a row's destination through hs_ptr / hs_len [max_streams] (null / 0 while a slot keeps none);
// the host mirrors flag and length in PoolSlot::hist.  Kernels: pool_hist_set, pool_hist_append, pool_hist_gather (rnnt_encoder.hip.h).

int rnnt_stream_keep_frames(rnnt_ctx* ctx, int32_t slot, int32_t keep, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_stream_keep_frames: no weights / no streams");
    if (slot < 0 || slot >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_keep_frames: slot %d outside [0, %d)", slot, ctx->n_streams);
    hipStream_t s = (hipStream_t)stream;
    if (!keep) return pool_hist_reset(ctx, s, slot, 1);
    if ((ctx->pool_mode ? ctx->slot[slot].pos : ctx->pos).conv_pos != 0)
        return fail(ctx, RNNT_ERR_STATE, "rnnt_stream_keep_frames: slot %d has advanced since it was opened (its first frames are gone)", slot);
    const size_t B = ctx->cfg.max_streams;
    int rc;
    if ((rc = reserve(ctx, ctx->hs_buf[slot], (size_t)ctx->cfg.max_cache_frames * D))) return rc;
    if (!ctx->hs_len) {
        if ((rc = reserve(ctx, ctx->hs_ptr, B))) return rc;
        if ((rc = reserve(ctx, ctx->hs_len, B))) return rc;   // last: its presence says the tables exist (pool_hist_reset)
        if ((rc = pool_hist_reset(ctx, s, 0, (int)B))) return rc;
    }
    hipLaunchKernelGGL(pool_hist_set, dim3(1), dim3(64), 0, s, ctx->hs_ptr.p, ctx->hs_len.p, slot, 1, ctx->hs_buf[slot].p);
    LAUNCHCHK("pool_hist_set");
    ctx->slot[slot].hist = HsSlot{1, 0};
    pool_enter(ctx);   // from here on the slot's frames come through the pool's entry points only
    return RNNT_OK;
}

int rnnt_stream_get_frames(rnnt_ctx* ctx, int32_t slot, int32_t from, int32_t cap_frames, float* dst_dev, int32_t* n_out, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (slot < 0 || slot >= ctx->n_streams || from < 0 || cap_frames < 0 || (cap_frames > 0 && !dst_dev))
        return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_frames: bad argument");
    const HsSlot& h = ctx->slot[slot].hist;
    if (!h.keep) return fail(ctx, RNNT_ERR_STATE, "rnnt_stream_get_frames: slot %d keeps no frames", slot);
    const int avail = h.len > from ? h.len - from : 0;
    if (n_out) *n_out = avail;
    const int ncopy = avail < cap_frames ? avail : cap_frames;
    if (ncopy > 0)
        HIPCHK(hipMemcpyAsync(dst_dev, ctx->hs_buf[slot] + (size_t)from * D, (size_t)ncopy * D * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RNNT_OK;
}

int rnnt_pool_rescore(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, const int32_t* n_hyp_host, const int32_t* hyp_lens_host,
                      const int32_t* hyp_tokens_host, int32_t N, int32_t Umax, double* nll_host, void* stream) {
    const char* fn = "rnnt_pool_rescore";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    int rc;
    if ((rc = pool_slots_check(ctx, fn, n, slots_host, ctx->n_streams, "slots"))) return rc;
    std::vector<int32_t> lens((size_t)n);
    int Tmax = 0;
    for (int i = 0; i < n; ++i) {
        const HsSlot& h = ctx->slot[slots_host[i]].hist;
        if (!h.keep) return fail(ctx, RNNT_ERR_STATE, "%s: slot %d keeps no frames", fn, slots_host[i]);
        if (h.len < 1) return fail(ctx, RNNT_ERR_STATE, "%s: slot %d has no frames yet", fn, slots_host[i]);
        lens[i] = h.len;
        Tmax = std::max(Tmax, lens[i]);
    }
    if ((rc = nbest_check(ctx, fn, lens.data(), n_hyp_host, hyp_lens_host, hyp_tokens_host, n, Tmax, N, Umax, nll_host, nullptr))) return rc;
    if ((rc = reserve(ctx, ctx->hs_stage, (size_t)n * Tmax * D))) return rc;
    return nbest_run(ctx, nullptr, slots_host, lens.data(), n_hyp_host, hyp_lens_host, hyp_tokens_host, n, Tmax, N, Umax, nll_host, nullptr, stream);
}
