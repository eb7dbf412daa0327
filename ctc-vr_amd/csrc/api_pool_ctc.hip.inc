// C ABI: WeNet's CTC prefix beam search with contextual biasing per slot of the stream pool, carried across calls
// (rnnt_stream_ctc_prefix_reset, rnnt_pool_ctc_prefix_logprobs, rnnt_stream_get_ctc_prefix; rnnt_pool_chunk_ctc_prefix is in
// api_pool.hip.inc with the other encoder forms).  Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_ctc_prefix.hip.h.
//
// The search is a per-frame recursion whose whole state at a frame boundary is the <= 16 hypothesis records and the two append-only
// arenas.  ctc_prefix_search_pool loads a slot's record, walks the call's frames with the frame step of the one-launch search
// (cp_frame, the same code) and stores the record back, so a search fed in pieces is bit for bit the one-launch search over the same
// rows, whatever the split.  Device state per slot: CpSlotState (2120 bytes) and [max_cache_frames * CP_MAX_BEAM + 1] int2 of either
// arena (1.28 MB each at max_cache_frames = 5000), allocated on the first use.  Host state per slot (PoolSlot::ctc, a SearchSlot): the
// frames walked, and the beam, use_context, graph generation, use_ngram and model generation of the search in progress.
//
// Rules: a slot's search is fresh after a reset; its first advancing call fixes beam_size, use_context and use_ngram until the next
// reset (another value: RNNT_ERR_ARG).  A reset record holds the n-gram start MARKER (NG_START), which the first step resolves under
// the model of that first call; rnnt_ngram_set starts a new model generation, with the graph's rule for the searches that use it.  rnnt_context_set starts a new graph generation: a search biased under an older one holds node ids
// of a graph that no longer exists and is refused (RNNT_ERR_STATE) until its slot is reset; unbiased searches go on.  Every refusal
// is decided before the first launch and changes nothing.  Frames, and the times reported, count from the slot's reset.

namespace {

size_t pool_ctc_astride(const rnnt_ctx* ctx) { return (size_t)ctx->cfg.max_cache_frames * CP_MAX_BEAM + 1; }

// the device state, on the first use: every slot starts from the start hypothesis
int pool_ctc_alloc(rnnt_ctx* ctx, hipStream_t s) {
    if (ctx->pc_state) return RNNT_OK;
    const size_t B = (size_t)ctx->cfg.max_streams;
    int rc;
    if ((rc = reserve(ctx, ctx->pc_parena, B * pool_ctc_astride(ctx)))) return rc;
    if ((rc = reserve(ctx, ctx->pc_tarena, B * pool_ctc_astride(ctx)))) return rc;
    if ((rc = calltab_alloc(ctx, ctx->pc_tab, 2 * B))) return rc;
    if ((rc = reserve(ctx, ctx->pc_state, B))) return rc;   // last: its presence says the state exists (pool_ctc_reset)
    hipLaunchKernelGGL(ctc_prefix_slot_reset, dim3((unsigned)B), dim3(64), 0, s, ctx->pc_state.p, 0);   // host records stay: a reset slot is fresh there already
    LAUNCHCHK("ctc_prefix_slot_reset");
    return RNNT_OK;
}

// Everything that can refuse an advance of the listed slots by t frames, slot range and duplicates aside; changes nothing.
int pool_ctc_check(rnnt_ctx* ctx, const char* fn, int n, const int* slots, int t, int beam_size, int use_context, int use_ngram) {
    const int V = ctx->cfg.vocab_size;
    if (t < 1) return fail(ctx, RNNT_ERR_ARG, "%s: %d frames", fn, t);
    if (V < 1 || V > 512) return fail(ctx, RNNT_ERR_ARG, "%s: vocab %d outside [1, 512]", fn, V);
    if (beam_size < 1 || beam_size > CP_MAX_BEAM || beam_size > V)
        return fail(ctx, RNNT_ERR_ARG, "%s: beam_size %d outside [1, min(%d, vocab %d)]", fn, beam_size, CP_MAX_BEAM, V);
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "%s: use_context without a context graph (rnnt_context_set)", fn);
    if (use_ngram && !ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "%s: use_ngram without an n-gram model (rnnt_ngram_set)", fn);
    for (int i = 0; i < n; ++i) {
        const SearchSlot& q = ctx->slot[slots[i]].ctc;
        if (q.beam != 0 && (q.use_ngram != 0) != (use_ngram != 0))
            return fail(ctx, RNNT_ERR_ARG, "%s: slot %d: use_ngram %d differs from the search in progress (%d); reset the slot first", fn, slots[i], use_ngram != 0,
                        q.use_ngram);
        if (q.beam != 0 && q.use_ngram && q.ngen != ctx->ng_gen)
            return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the n-gram model changed since its search began; reset the slot first", fn, slots[i]);
    }
    return search_slot_check(ctx, fn, &PoolSlot::ctc, n, slots, t, beam_size, 0.f, 0.f, use_context, false);
}

// the launch: pool_ctc_check has passed and the state exists.  One async copy of the call's table, ONE kernel, host bookkeeping.
int pool_ctc_launch(rnnt_ctx* ctx, hipStream_t s, int n, const int* slots, const float* lp_dev, int t, int beam_size, int use_context, int use_ngram) {
    int rc, *tab;
    if ((rc = calltab_fill(ctx, ctx->pc_tab, tab))) return rc;
    for (int i = 0; i < n; ++i) { tab[i] = slots[i]; tab[n + i] = ctx->slot[slots[i]].ctc.frames_done; }
    if ((rc = calltab_send(ctx, ctx->pc_tab, 2 * (size_t)n, s))) return rc;
    CtcPrefixPoolP p;
    memset(&p, 0, sizeof(p));
    p.lp = lp_dev; p.slots = ctx->pc_tab; p.t0 = ctx->pc_tab + n; p.t = t; p.V = ctx->cfg.vocab_size; p.blank = ctx->cfg.blank_id; p.beam = beam_size;
    if (use_context) p.g = ctx_graph_dev(ctx);
    if (use_ngram) p.ng = ngram_dev(ctx);
    p.parena = ctx->pc_parena; p.tarena = ctx->pc_tarena; p.astride = pool_ctc_astride(ctx); p.state = ctx->pc_state;
    {
        ProfScope prof(ctx, s, TAG_CTC_PREFIX_POOL);
        if (use_ngram) hipLaunchKernelGGL(ctc_prefix_search_pool<true>, dim3(n), dim3(CP_NT), 0, s, p);
        else hipLaunchKernelGGL(ctc_prefix_search_pool<false>, dim3(n), dim3(CP_NT), 0, s, p);
        LAUNCHCHK("ctc_prefix_search_pool");
    }
    search_slot_commit(ctx, &PoolSlot::ctc, n, slots, t, beam_size, 0.f, 0.f, use_context);
    for (int i = 0; i < n; ++i) { ctx->slot[slots[i]].ctc.use_ngram = use_ngram != 0; ctx->slot[slots[i]].ctc.ngen = ctx->ng_gen; }
    return RNNT_OK;
}

}  // namespace

int rnnt_stream_ctc_prefix_reset(rnnt_ctx* ctx, int32_t slot, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    const int B = ctx->cfg.max_streams;
    if (slot < -1 || slot >= B) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_ctc_prefix_reset: slot %d outside [-1, %d)", slot, B);
    return pool_ctc_reset(ctx, (hipStream_t)stream, slot < 0 ? 0 : slot, slot < 0 ? B : 1);
}

int rnnt_pool_ctc_prefix_logprobs(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* lp_dev, int32_t t, int32_t beam_size,
                                  int32_t use_context, void* stream) {
    return rnnt_pool_ctc_prefix_logprobs_ngram(ctx, n_active, slots_host, lp_dev, t, beam_size, use_context, 0, stream);
}

int rnnt_pool_ctc_prefix_logprobs_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* lp_dev, int32_t t, int32_t beam_size,
                                        int32_t use_context, int32_t use_ngram, void* stream) {
    const char* fn = "rnnt_pool_ctc_prefix_logprobs";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !lp_dev) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    int rc;
    if ((rc = pool_slots_check(ctx, fn, n_active, slots_host, ctx->cfg.max_streams))) return rc;
    if ((rc = pool_ctc_check(ctx, fn, n_active, slots_host, t, beam_size, use_context, use_ngram))) return rc;
    if ((size_t)n_active * t * ctx->cfg.vocab_size >= ((size_t)1 << 40)) return fail(ctx, RNNT_ERR_SHAPE, "%s: n_active=%d t=%d too large for one call", fn, n_active, t);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pool_ctc_alloc(ctx, s))) return rc;
    return pool_ctc_launch(ctx, s, n_active, slots_host, lp_dev, t, beam_size, use_context, use_ngram);
}

int rnnt_stream_get_ctc_prefix(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                               int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host, int32_t* frames_out, void* stream) {
    return rnnt_stream_get_ctc_prefix_ngram(ctx, slot, final, cap_hyps, cap_tokens, n_hyp, lens_host, tokens_host, times_host, scores_host, ctx_scores_host,
                                            nullptr, frames_out, stream);
}

// A slot whose search fuses the model reads with its n-gram scores in the totals whichever getter is called; ngram_scores_host
// [cap_hyps] (may be NULL) receives them: the running ones, or with final != 0 those with the end term.
int rnnt_stream_get_ctc_prefix_ngram(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp,
                                     int32_t* lens_host, int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host,
                                     double* ngram_scores_host, int32_t* frames_out, void* stream) {
    const char* fn = "rnnt_stream_get_ctc_prefix";
    if (!ctx) return RNNT_ERR_ARG;
    const bool query = !lens_host && !tokens_host && !times_host && !scores_host;   // the sizes a read needs: host only
    if (!n_hyp || (!query && (!lens_host || !tokens_host || !times_host || !scores_host))) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (slot < 0 || slot >= ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->cfg.max_streams);
    const SearchSlot q = ctx->slot[slot].ctc;
    const int beam = q.beam > 0 ? q.beam : 1;                        // a fresh slot holds the start hypothesis alone
    if (query) {
        *n_hyp = beam;
        if (frames_out) *frames_out = q.frames_done;
        return RNNT_OK;
    }
    if (cap_hyps < beam) return fail(ctx, RNNT_ERR_ARG, "%s: beam %d, room for %d hypotheses", fn, beam, cap_hyps);
    if (cap_tokens < q.frames_done || cap_tokens < 0) return fail(ctx, RNNT_ERR_ARG, "%s: cap_tokens %d < %d frames", fn, cap_tokens, q.frames_done);
    SearchRead rd;
    int rc;
    if ((rc = search_slot_read(ctx, fn, slot, q, final, rd))) return rc;
    const bool ngram = q.beam > 0 && q.use_ngram;
    if (ngram && final && (!ctx->ng_on || q.ngen != ctx->ng_gen))
        return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the n-gram model changed since its search began (final = 0 still reads it)", fn, slot);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pool_ctc_alloc(ctx, s))) return rc;
    // the packed block: scores [beam] | context scores [beam] | with a model its scores [beam] as doubles, then the ints of cp_out with B = 1
    const size_t R = (size_t)beam, lcap = (size_t)std::max(q.frames_done, 1), nd = ngram ? 3 : 2;
    Carve<int> oc;
    const size_t n_dbl = nd * R + (cp_out(oc, 1, R, lcap).total + 1) / 2;
    if ((rc = reserve(ctx, ctx->pc_out, n_dbl))) return rc;
    oc = {reinterpret_cast<int*>(ctx->pc_out + nd * R)};
    const CpOut o = cp_out(oc, 1, R, lcap);
    CtcPrefixPackP p;
    memset(&p, 0, sizeof(p));
    p.state = ctx->pc_state + slot;
    p.pa = ctx->pc_parena + (size_t)slot * pool_ctc_astride(ctx); p.ta = ctx->pc_tarena + (size_t)slot * pool_ctc_astride(ctx);
    p.fin_nscore = rd.fin ? ctx_graph_dev(ctx).nscore : nullptr;
    p.beam = beam; p.lcap = (int)lcap; p.final = final != 0;
    if (ngram && final) p.ng = ngram_dev(ctx);
    p.o.sc = ctx->pc_out; p.o.cs = ctx->pc_out + R;
    if (ngram) p.o.ls = ctx->pc_out + 2 * R;
    p.o.nh = o.nh; p.o.len = o.len; p.o.tok = o.tok; p.o.time = o.time;
    {
        ProfScope prof(ctx, s, TAG_CTC_PREFIX_PACK);
        if (ngram) hipLaunchKernelGGL(ctc_prefix_pack<true>, dim3(1), dim3(CP_NT), 0, s, p);
        else hipLaunchKernelGGL(ctc_prefix_pack<false>, dim3(1), dim3(CP_NT), 0, s, p);
        LAUNCHCHK("ctc_prefix_pack");
    }
    std::vector<double> od(n_dbl);
    HIPCHK(hipMemcpyAsync(od.data(), ctx->pc_out, n_dbl * sizeof(double), hipMemcpyDeviceToHost, s));     // the download
    HIPCHK(hipStreamSynchronize(s));
    Carve<int> hc{reinterpret_cast<int*>(od.data() + nd * R)};
    const CpOut h = cp_out(hc, 1, R, lcap);
    cp_out_copy(h, od.data(), 1, R, lcap, (size_t)cap_hyps, (size_t)cap_tokens, n_hyp, lens_host, tokens_host, times_host, scores_host, ctx_scores_host,
                ngram ? ngram_scores_host : nullptr);
    if (!ngram && ngram_scores_host) std::fill(ngram_scores_host, ngram_scores_host + cap_hyps, 0.0);
    if (frames_out) *frames_out = q.frames_done;
    return RNNT_OK;
}
