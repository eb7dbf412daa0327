// C ABI: greedy decode of the buffered frames, token read-back, frame hand-over.  Included by rnnt_api.hip inside extern "C".

int rnnt_greedy_decode(rnnt_ctx* ctx, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_greedy_decode: no weights / no streams");
    if (ctx->pool_mode && ctx->frames_buffered > 0)   // frames of an encoder-only pool call: only the active slots' rows are defined
        return fail(ctx, RNNT_ERR_STATE, "rnnt_greedy_decode: stream pool frames are decoded by rnnt_pool_chunk(greedy != 0)");
    hipStream_t s = (hipStream_t)stream;
    const int nf = ctx->frames_buffered;
    if (nf <= ctx->frames_decoded) return RNNT_OK;
    int rc;
    if (ctx->use_persistent) {
        if ((rc = decode_resident(ctx, s, nf))) return rc;
        ctx->frames_decoded = nf;
        return RNNT_OK;
    }
    const int first = nf - ctx->frames_decoded + 2;
    if ((rc = greedy_steps(ctx, s, first, nf))) return rc;
    if ((rc = greedy_drain(ctx, s, nf, first))) return rc;
    ctx->frames_decoded = nf;
    return RNNT_OK;
}

int rnnt_get_tokens(rnnt_ctx* ctx, int32_t* counts_host, int32_t* tokens_host, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (counts_host) HIPCHK(hipMemcpyAsync(counts_host, ctx->count, ctx->n_streams * sizeof(int), hipMemcpyDeviceToHost, s));
    if (tokens_host)
        HIPCHK(hipMemcpyAsync(tokens_host, ctx->tokens, (size_t)ctx->n_streams * ctx->cfg.max_tokens * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_frames_consume(rnnt_ctx* ctx, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (ctx->frames_decoded != ctx->frames_buffered) return fail(ctx, RNNT_ERR_STATE, "undecoded frames in the buffer");
    hipStream_t s = (hipStream_t)stream;
    ctx->frames_buffered = 0;
    ctx->frames_decoded = 0;
    HIPCHK(hipMemsetAsync(ctx->fidx, 0, ctx->cfg.max_streams * sizeof(int), s));
    return RNNT_OK;
}
