// C ABI: WeNet's CTC prefix beam search with contextual biasing per slot of the stream pool, carried across calls
// (rnnt_stream_ctc_prefix_reset, rnnt_pool_ctc_prefix_logprobs, rnnt_stream_get_ctc_prefix; rnnt_pool_chunk_ctc_prefix is in
// api_pool.hip.inc with the other encoder forms).  Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_ctc_prefix.hip.h.
//
// The search is a per-frame recursion whose whole state at a frame boundary is the <= 16 hypothesis records and the two append-only
// arenas.  ctc_prefix_search_pool loads a slot's record, walks the call's frames with the frame step of the one-launch search
// (cp_frame, the same code) and stores the record back, so a search fed in pieces is bit for bit the one-launch search over the same
// rows, whatever the split.  Device state per slot: CpSlotState (1928 bytes) and [max_cache_frames * CP_MAX_BEAM + 1] int2 of either
// arena (1.28 MB each at max_cache_frames = 5000), allocated on the first use.  Host state per slot (rnnt_ctx::PcSlot): the frames
// walked, and the beam, use_context and graph generation of the search in progress.
//
// Rules: a slot's search is fresh after a reset; its first advancing call fixes beam_size and use_context until the next reset
// (another value: RNNT_ERR_ARG).  rnnt_context_set starts a new graph generation: a search biased under an older one holds node ids
// of a graph that no longer exists and is refused (RNNT_ERR_STATE) until its slot is reset; unbiased searches go on.  Every refusal
// is decided before the first launch and changes nothing.  Frames, and the times reported, count from the slot's reset.

namespace {

std::vector<rnnt_ctx::PcSlot>& pool_ctc_slots(rnnt_ctx* ctx) {
    if (ctx->pc_slot.empty()) ctx->pc_slot.assign((size_t)ctx->cfg.max_streams, rnnt_ctx::PcSlot{0, 0, 0, 0});
    return ctx->pc_slot;
}

size_t pool_ctc_astride(const rnnt_ctx* ctx) { return (size_t)ctx->cfg.max_cache_frames * CP_MAX_BEAM + 1; }

// the device state, on the first use: every slot starts from the start hypothesis
int pool_ctc_alloc(rnnt_ctx* ctx, hipStream_t s) {
    if (ctx->pc_state) return RNNT_OK;
    const size_t B = (size_t)ctx->cfg.max_streams;
    int rc;
    if ((rc = reserve(ctx, ctx->pc_parena, B * pool_ctc_astride(ctx)))) return rc;
    if ((rc = reserve(ctx, ctx->pc_tarena, B * pool_ctc_astride(ctx)))) return rc;
    if ((rc = reserve(ctx, ctx->pc_tab, 2 * B))) return rc;
    if ((rc = reserve(ctx, ctx->pc_tab_host, 2 * B))) return rc;
    if (!ctx->pc_ev) HIPCHK(hipEventCreateWithFlags(&ctx->pc_ev, hipEventDisableTiming));
    if ((rc = reserve(ctx, ctx->pc_state, B))) return rc;   // last: its presence says the state exists (pool_ctc_reset)
    hipLaunchKernelGGL(ctc_prefix_slot_reset, dim3((unsigned)B), dim3(64), 0, s, ctx->pc_state.p, 0);   // host records stay: a reset slot is fresh there already
    LAUNCHCHK("ctc_prefix_slot_reset");
    return RNNT_OK;
}

// Everything that can refuse an advance of the listed slots by t frames, slot range and duplicates aside; changes nothing.
int pool_ctc_check(rnnt_ctx* ctx, const char* fn, int n, const int* slots, int t, int beam_size, int use_context) {
    const int V = ctx->cfg.vocab_size;
    if (t < 1) return fail(ctx, RNNT_ERR_ARG, "%s: %d frames", fn, t);
    if (V < 1 || V > 512) return fail(ctx, RNNT_ERR_ARG, "%s: vocab %d outside [1, 512]", fn, V);
    if (beam_size < 1 || beam_size > CP_MAX_BEAM || beam_size > V)
        return fail(ctx, RNNT_ERR_ARG, "%s: beam_size %d outside [1, min(%d, vocab %d)]", fn, beam_size, CP_MAX_BEAM, V);
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "%s: use_context without a context graph (rnnt_context_set)", fn);
    const std::vector<rnnt_ctx::PcSlot>& ps = pool_ctc_slots(ctx);
    for (int i = 0; i < n; ++i) {
        const rnnt_ctx::PcSlot& q = ps[slots[i]];
        if (q.beam != 0) {   // a search in progress
            if (q.beam != beam_size || (q.use_context != 0) != (use_context != 0))
                return fail(ctx, RNNT_ERR_ARG, "%s: slot %d: beam_size %d / use_context %d differ from the search in progress (%d / %d); reset the slot first", fn,
                            slots[i], beam_size, use_context != 0, q.beam, q.use_context);
            if (q.use_context && q.gen != ctx->cg_gen)
                return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the context graph changed since its search began; reset the slot first", fn, slots[i]);
        }
        if ((long long)q.frames_done + t > ctx->cfg.max_cache_frames)
            return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: %d + %d frames exceed max_cache_frames %d", fn, slots[i], q.frames_done, t, ctx->cfg.max_cache_frames);
    }
    return RNNT_OK;
}

// the launch: pool_ctc_check has passed and the state exists.  One async copy of the call's table, ONE kernel, host bookkeeping.
int pool_ctc_launch(rnnt_ctx* ctx, hipStream_t s, int n, const int* slots, const float* lp_dev, int t, int beam_size, int use_context) {
    std::vector<rnnt_ctx::PcSlot>& ps = pool_ctc_slots(ctx);
    HIPCHK(hipEventSynchronize(ctx->pc_ev));               // the previous call's copy has left the pinned buffer
    for (int i = 0; i < n; ++i) { ctx->pc_tab_host[i] = slots[i]; ctx->pc_tab_host[n + i] = ps[slots[i]].frames_done; }
    HIPCHK(hipMemcpyAsync(ctx->pc_tab, ctx->pc_tab_host, 2 * (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->pc_ev, s));
    CtcPrefixPoolP p;
    memset(&p, 0, sizeof(p));
    p.lp = lp_dev; p.slots = ctx->pc_tab; p.t0 = ctx->pc_tab + n; p.t = t; p.V = ctx->cfg.vocab_size; p.blank = ctx->cfg.blank_id; p.beam = beam_size;
    if (use_context) p.g = ctx_graph_dev(ctx);
    p.parena = ctx->pc_parena; p.tarena = ctx->pc_tarena; p.astride = pool_ctc_astride(ctx); p.state = ctx->pc_state;
    {
        ProfScope prof(ctx, s, TAG_CTC_PREFIX_POOL);
        hipLaunchKernelGGL(ctc_prefix_search_pool, dim3(n), dim3(CP_NT), 0, s, p);
        LAUNCHCHK("ctc_prefix_search_pool");
    }
    for (int i = 0; i < n; ++i) {
        rnnt_ctx::PcSlot& q = ps[slots[i]];
        q.frames_done += t;
        q.beam = beam_size; q.use_context = use_context != 0; q.gen = ctx->cg_gen;   // fixed by the first call; later ones passed the check with the same values
    }
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
    const char* fn = "rnnt_pool_ctc_prefix_logprobs";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !lp_dev) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    const int B = ctx->cfg.max_streams;
    if (n_active < 1 || n_active > B) return fail(ctx, RNNT_ERR_ARG, "%s: %d active slots of %d", fn, n_active, B);
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n_active; ++i) {
        const int slot = slots_host[i];
        if (slot < 0 || slot >= B) return fail(ctx, RNNT_ERR_ARG, "%s: row %d: slot %d outside [0, %d)", fn, i, slot, B);
        if (seen[slot]) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d listed twice", fn, slot);
        seen[slot] = 1;
    }
    int rc;
    if ((rc = pool_ctc_check(ctx, fn, n_active, slots_host, t, beam_size, use_context))) return rc;
    if ((size_t)n_active * t * ctx->cfg.vocab_size >= ((size_t)1 << 40)) return fail(ctx, RNNT_ERR_SHAPE, "%s: n_active=%d t=%d too large for one call", fn, n_active, t);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pool_ctc_alloc(ctx, s))) return rc;
    return pool_ctc_launch(ctx, s, n_active, slots_host, lp_dev, t, beam_size, use_context);
}

int rnnt_stream_get_ctc_prefix(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                               int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host, int32_t* frames_out, void* stream) {
    const char* fn = "rnnt_stream_get_ctc_prefix";
    if (!ctx) return RNNT_ERR_ARG;
    const bool query = !lens_host && !tokens_host && !times_host && !scores_host;   // the sizes a read needs: host only
    if (!n_hyp || (!query && (!lens_host || !tokens_host || !times_host || !scores_host))) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (slot < 0 || slot >= ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->cfg.max_streams);
    const rnnt_ctx::PcSlot q = pool_ctc_slots(ctx)[slot];
    const int beam = q.beam > 0 ? q.beam : 1;                        // a fresh slot holds the start hypothesis alone
    if (query) {
        *n_hyp = beam;
        if (frames_out) *frames_out = q.frames_done;
        return RNNT_OK;
    }
    if (cap_hyps < beam) return fail(ctx, RNNT_ERR_ARG, "%s: beam %d, room for %d hypotheses", fn, beam, cap_hyps);
    if (cap_tokens < q.frames_done || cap_tokens < 0) return fail(ctx, RNNT_ERR_ARG, "%s: cap_tokens %d < %d frames", fn, cap_tokens, q.frames_done);
    // finalize needs the graph the search ran under; a fresh slot has fixed none and finalizes its root under the graph that is set, if any
    const bool fin = final != 0 && (q.beam > 0 ? q.use_context != 0 : ctx->cg_on);
    if (fin && q.beam > 0 && (!ctx->cg_on || q.gen != ctx->cg_gen))
        return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the context graph changed since its search began (final = 0 still reads it)", fn, slot);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = pool_ctc_alloc(ctx, s))) return rc;
    // the packed block: scores [beam] | context scores [beam] as doubles, then the ints n_hyp | lens [beam] | tokens [beam][lcap] | times likewise
    const size_t R = (size_t)beam, lcap = (size_t)std::max(q.frames_done, 1), n_int = 1 + R + 2 * R * lcap, n_dbl = 2 * R + (n_int + 1) / 2;
    if ((rc = reserve(ctx, ctx->pc_out, n_dbl))) return rc;
    int* oi = reinterpret_cast<int*>(ctx->pc_out + 2 * R);
    CtcPrefixPackP p;
    memset(&p, 0, sizeof(p));
    p.state = ctx->pc_state + slot;
    p.pa = ctx->pc_parena + (size_t)slot * pool_ctc_astride(ctx); p.ta = ctx->pc_tarena + (size_t)slot * pool_ctc_astride(ctx);
    p.fin_nscore = fin ? ctx_graph_dev(ctx).nscore : nullptr;
    p.beam = beam; p.lcap = (int)lcap;
    p.o.sc = ctx->pc_out; p.o.cs = ctx->pc_out + R;
    p.o.nh = oi; p.o.len = oi + 1; p.o.tok = oi + 1 + R; p.o.time = oi + 1 + R + R * lcap;
    {
        ProfScope prof(ctx, s, TAG_CTC_PREFIX_PACK);
        hipLaunchKernelGGL(ctc_prefix_pack, dim3(1), dim3(CP_NT), 0, s, p);
        LAUNCHCHK("ctc_prefix_pack");
    }
    std::vector<double> od(n_dbl);
    HIPCHK(hipMemcpyAsync(od.data(), ctx->pc_out, n_dbl * sizeof(double), hipMemcpyDeviceToHost, s));     // the download
    HIPCHK(hipStreamSynchronize(s));
    const int* hi = reinterpret_cast<const int*>(od.data() + 2 * R);
    const size_t H = (size_t)cap_hyps;
    *n_hyp = hi[0];
    std::fill(lens_host, lens_host + H, 0);
    std::fill(scores_host, scores_host + H, 0.0);
    if (ctx_scores_host) std::fill(ctx_scores_host, ctx_scores_host + H, 0.0);
    std::fill(tokens_host, tokens_host + H * cap_tokens, 0);
    std::fill(times_host, times_host + H * cap_tokens, 0);
    memcpy(lens_host, hi + 1, R * sizeof(int));
    memcpy(scores_host, od.data(), R * sizeof(double));
    if (ctx_scores_host) memcpy(ctx_scores_host, od.data() + R, R * sizeof(double));
    const size_t ncopy = std::min<size_t>(lcap, (size_t)cap_tokens);
    for (size_t r = 0; r < R; ++r) {
        memcpy(tokens_host + r * cap_tokens, hi + 1 + R + r * lcap, ncopy * sizeof(int));
        memcpy(times_host + r * cap_tokens, hi + 1 + R + R * lcap + r * lcap, ncopy * sizeof(int));
    }
    if (frames_out) *frames_out = q.frames_done;
    return RNNT_OK;
}
