// C ABI: diagnostics, state read-back in the reference's layouts, launch-site profiling, counters.  Included by rnnt_api.hip inside extern "C".

// diagnostic only (not in the header): n_bytes streamed src -> dst `iters` times with the given cache policy
int rnnt_debug_stream_copy(rnnt_ctx* ctx, const float* src_dev, float* dst_dev, int64_t n_bytes, int32_t mode, int32_t iters, void* stream) {
    if (!ctx || !src_dev || !dst_dev) return RNNT_ERR_ARG;
    for (int i = 0; i < iters; ++i)
        hipLaunchKernelGGL(debug_stream_copy, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, src_dev, dst_dev, (long long)(n_bytes / 16), mode);
    LAUNCHCHK("debug_stream_copy");
    return RNNT_OK;
}

int rnnt_get_att_cache(rnnt_ctx* ctx, int32_t b, float* dst_host, int32_t* len_out, void* stream) {
    if (!ctx || b < 0 || b >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_get_att_cache: bad stream index");
    hipStream_t s = (hipStream_t)stream;
    // stream pool: the slot's own cache window
    const SlotPos& p = ctx->pool_mode ? ctx->slot[b].pos : ctx->pos;
    const int cache_len = p.cache_len, kv_start = p.kv_start;
    if (len_out) *len_out = cache_len;
    if (!dst_host || cache_len == 0) return RNNT_OK;
    const long long n = (long long)L * RNNT_H * cache_len * 128;
    hipLaunchKernelGGL(gather_att_cache, dim3(grid_for(n)), dim3(256), 0, s, ctx->kcache, ctx->vcache, ctx->scratch, b, ctx->cfg.max_streams,
                       (long long)ctx->tcap, kv_start, cache_len);
    LAUNCHCHK("gather_att_cache");
    HIPCHK(hipMemcpyAsync(dst_host, ctx->scratch, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_get_cnn_cache(rnnt_ctx* ctx, int32_t b, float* dst_host, void* stream) {
    if (!ctx || !dst_host || b < 0 || b >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_get_cnn_cache: bad argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gather_cnn_cache, dim3(L * RNNT_LORDER), dim3(64), 0, s, ctx->xring, ctx->ln_conv_g_all, ctx->ln_conv_b_all, ctx->scratch, b,
                       ctx->cfg.max_streams, ctx->cap, (ctx->pool_mode ? ctx->slot[b].pos : ctx->pos).conv_pos);
    LAUNCHCHK("gather_cnn_cache");
    HIPCHK(hipMemcpyAsync(dst_host, ctx->scratch, (size_t)L * D * RNNT_LORDER * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_get_predictor_state(rnnt_ctx* ctx, int32_t b, float* h_host, float* c_host, int32_t* last_token, void* stream) {
    if (!ctx || b < 0 || b >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_get_predictor_state: bad stream index");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(ctx->pinned + 4, ctx->sel + b, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const size_t bo = (size_t)(ctx->pinned[4] & 1) * ctx->cfg.max_streams * D;   // committed buffer of this stream
    if (h_host) HIPCHK(hipMemcpyAsync(h_host, ctx->h + bo + (size_t)b * D, D * sizeof(float), hipMemcpyDeviceToHost, s));
    if (c_host) HIPCHK(hipMemcpyAsync(c_host, ctx->c + bo + (size_t)b * D, D * sizeof(float), hipMemcpyDeviceToHost, s));
    if (last_token) HIPCHK(hipMemcpyAsync(last_token, ctx->tok + b, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_get_enc_frames(rnnt_ctx* ctx, float* dst_host, int32_t* frames_out, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nf = ctx->frames_buffered;
    if (frames_out) *frames_out = nf;
    if (!dst_host || nf == 0) return RNNT_OK;
    HIPCHK(hipMemcpy2DAsync(dst_host, (size_t)nf * D * sizeof(float), ctx->encbuf, (size_t)ctx->fstride * D * sizeof(float),
                            (size_t)nf * D * sizeof(float), ctx->n_streams, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

const float* rnnt_enc_frames_dev(rnnt_ctx* ctx, int32_t* frames_out, int32_t* stride_frames) {
    if (!ctx) return nullptr;
    if (frames_out) *frames_out = ctx->frames_buffered;
    if (stride_frames) *stride_frames = ctx->fstride;
    return ctx->encbuf;
}

int rnnt_profile_begin(rnnt_ctx* ctx, int32_t tag) {
    if (!ctx) return RNNT_ERR_ARG;
    ctx->prof_tag = tag;
    ctx->prof_used = 0;
    return RNNT_OK;
}

int rnnt_profile_end(rnnt_ctx* ctx, double* total_ms, int64_t* n_launches) {
    if (!ctx) return RNNT_ERR_ARG;
    double tot = 0;
    for (size_t i = 0; i + 1 < ctx->prof_used; i += 2) {
        HIPCHK(hipEventSynchronize(ctx->prof_ev[i + 1]));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ctx->prof_ev[i], ctx->prof_ev[i + 1]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (n_launches) *n_launches = (int64_t)(ctx->prof_used / 2);
    ctx->prof_tag = -1;
    ctx->prof_used = 0;
    return RNNT_OK;
}

int rnnt_form_log_begin(rnnt_ctx* ctx) {
    if (!ctx) return RNNT_ERR_ARG;
    ctx->form_log.clear();
    ctx->form_log_on = true;
    return RNNT_OK;
}

int rnnt_form_log_end(rnnt_ctx* ctx, char* buf, int64_t cap, int64_t* needed) {
    if (!ctx) return RNNT_ERR_ARG;
    ctx->form_log_on = false;
    std::string text;
    for (const auto& kv : ctx->form_log) text += kv.first + "\t" + std::to_string(kv.second) + "\n";
    if (needed) *needed = (int64_t)text.size() + 1;
    if (buf && cap > 0) {
        const size_t n = std::min(text.size(), (size_t)cap - 1);
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return RNNT_OK;
}

int rnnt_get_counters(rnnt_ctx* ctx, int64_t* launches, int64_t* greedy_steps) {
    if (!ctx) return RNNT_ERR_ARG;
    if (launches) *launches = ctx->launches;
    if (greedy_steps) *greedy_steps = ctx->greedy_steps;
    return RNNT_OK;
}
