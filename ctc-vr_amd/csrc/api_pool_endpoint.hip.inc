// C ABI: "is the caller done?" -- endpoint detection per slot of the stream pool (rnnt_stream_endpoint, rnnt_pool_endpoint_frames,
// rnnt_pool_get_endpoints), the stateless blank log-posterior (rnnt_ctc_blank_logprob) and the host twin of the rule
// (rnnt_endpoint_scan_host).  Included by rnnt_api.hip inside extern "C".  Semantics and kernels: rnnt_endpoint.hip.h.
// pool_chunk_run advances the listed endpoint slots through pool_endpoint_rows (host_launch.hip.inc), directly after the history append.
//
// A slot detects nothing unless asked.  Asked (on a slot that has not advanced), every pool call that encodes it -- in any of the five
// modes -- runs ONE extra launch, pool_endpoint, over the call's compact after_norm rows: the CTC head's blank log-posterior of the
// slot's t' new frames (f32, online softmax, nothing of size rows x V written) and the rule's recursion over them.  Device state per
// slot: EpCfg (24 bytes) and five ints, in tables [max_streams] reserved on the first use; the host mirrors the on flag
// (PoolSlot::ep).  A read downloads the whole state table once and picks the listed rows on the host.

int rnnt_stream_endpoint(rnnt_ctx* ctx, int32_t slot, const rnnt_endpoint_config* cfg, void* stream) {
    const char* fn = "rnnt_stream_endpoint";
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "%s: no weights / no streams", fn);
    if (slot < 0 || slot >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->n_streams);
    hipStream_t s = (hipStream_t)stream;
    if (!cfg) return pool_endpoint_reset(ctx, s, slot, 1);
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "%s: ctc_head.ctc_lo.* not loaded", fn);
    if (!endpoint_config_ok(cfg))
        return fail(ctx, RNNT_ERR_ARG, "%s: blank_threshold %g outside (0, 1) or a negative count (%d, %d, %d, %d)", fn, (double)cfg->blank_threshold,
                    cfg->min_speech_frames, cfg->rule1_trailing, cfg->rule2_trailing, cfg->rule3_frames);
    if ((ctx->pool_mode ? ctx->slot[slot].pos : ctx->pos).conv_pos != 0)
        return fail(ctx, RNNT_ERR_STATE, "%s: slot %d has advanced since it was opened (its first frames are gone)", fn, slot);
    const size_t B = ctx->cfg.max_streams;
    int rc;
    if (!ctx->ep_state) {
        if ((rc = reserve(ctx, ctx->ep_cfg, B))) return rc;
        if ((rc = reserve(ctx, ctx->ep_host, B * EP_STATE_INTS))) return rc;
        if ((rc = calltab_alloc(ctx, ctx->ep_tab, B))) return rc;
        if ((rc = reserve(ctx, ctx->ep_state, B * EP_STATE_INTS))) return rc;   // last: its presence says the tables exist
        hipLaunchKernelGGL(pool_endpoint_set, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, ctx->ep_cfg.p, ctx->ep_state.p, 0, (int)B, EpCfg{});
        LAUNCHCHK("pool_endpoint_set");
    }
    const EpCfg c{endpoint_log_thr(cfg), cfg->min_speech_frames, cfg->rule1_trailing, cfg->rule2_trailing, cfg->rule3_frames, 1};
    hipLaunchKernelGGL(pool_endpoint_set, dim3(1), dim3(64), 0, s, ctx->ep_cfg.p, ctx->ep_state.p, slot, 1, c);
    LAUNCHCHK("pool_endpoint_set");
    ctx->slot[slot].ep = 1;
    pool_enter(ctx);   // from here on the slot's frames come through the pool's entry points only
    return RNNT_OK;
}

int rnnt_pool_endpoint_frames(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, void* stream) {
    const char* fn = "rnnt_pool_endpoint_frames";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !enc_dev) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    int rc = pool_slots_check(ctx, fn, n_active, slots_host, ctx->cfg.max_streams, "active slots", [&] {
        return t < 1 ? fail(ctx, RNNT_ERR_ARG, "%s: %d frames", fn, t) : (int)RNNT_OK;
    }, [&](int, int slot) {
        return ctx->slot[slot].ep ? (int)RNNT_OK : fail(ctx, RNNT_ERR_STATE, "%s: slot %d detects no endpoint (rnnt_stream_endpoint)", fn, slot);
    });
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* tab;
    if ((rc = calltab_fill(ctx, ctx->ep_tab, tab))) return rc;
    memcpy(tab, slots_host, (size_t)n_active * sizeof(int));
    if ((rc = calltab_send(ctx, ctx->ep_tab, (size_t)n_active, s))) return rc;
    return pool_endpoint_rows(ctx, s, n_active, slots_host, ctx->ep_tab, enc_dev, t);
}

int rnnt_pool_get_endpoints(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, int32_t* state_host, void* stream) {
    const char* fn = "rnnt_pool_get_endpoints";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !state_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    int rc = pool_slots_check(ctx, fn, n, slots_host, ctx->cfg.max_streams, "slots", [] { return (int)RNNT_OK; }, [&](int, int slot) {
        return ctx->slot[slot].ep ? (int)RNNT_OK : fail(ctx, RNNT_ERR_STATE, "%s: slot %d detects no endpoint (rnnt_stream_endpoint)", fn, slot);
    });
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t all = (size_t)ctx->cfg.max_streams * EP_STATE_INTS;
    HIPCHK(hipMemcpyAsync(ctx->ep_host, ctx->ep_state, all * sizeof(int), hipMemcpyDeviceToHost, s));   // the whole table: one copy per call
    HIPCHK(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) memcpy(state_host + (size_t)i * EP_STATE_INTS, ctx->ep_host + (size_t)slots_host[i] * EP_STATE_INTS, EP_STATE_INTS * sizeof(int));
    return RNNT_OK;
}

int rnnt_ctc_blank_logprob(rnnt_ctx* ctx, const float* enc_dev, int32_t rows, float* out_dev, void* stream) {
    if (!ctx || !enc_dev || !out_dev || rows < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_ctc_blank_logprob: bad argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_blank_logprob: ctc_head.ctc_lo.* not loaded");
    hipLaunchKernelGGL(ctc_blank_rows, dim3((unsigned)((rows + EP_TILE - 1) / EP_TILE)), dim3(EP_THREADS), 0, (hipStream_t)stream, enc_dev, out_dev, rows, ctx->wctc,
                       ctx->bctc, ctx->cfg.vocab_size, ctx->cfg.blank_id);
    LAUNCHCHK("ctc_blank_rows");
    return RNNT_OK;
}

int rnnt_endpoint_scan_host(const float* blank_lp, int32_t t, const rnnt_endpoint_config* cfg, int32_t* state) {
    if (!cfg || !state || t < 0 || (t > 0 && !blank_lp) || !endpoint_config_ok(cfg)) return RNNT_ERR_ARG;
    endpoint_scan(blank_lp, t, endpoint_log_thr(cfg), cfg->min_speech_frames, cfg->rule1_trailing, cfg->rule2_trailing, cfg->rule3_frames, state);
    return RNNT_OK;
}
