// C ABI: WeNet's CTC-fused transducer prefix beam search (wenet/transducer/search/prefix_beam_search.py:42-148) per slot of the stream
// pool, carried across calls (rnnt_stream_prefix_reset, rnnt_pool_prefix_frames, rnnt_stream_get_prefix; rnnt_pool_chunk_prefix is in
// api_pool.hip.inc with the other encoder forms; the _ctx forms add hot-word biasing by the graph of rnnt_context_set, the _ngram forms shallow fusion
// with the model of rnnt_ngram_set).  Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_prefix.hip.h.
//
// The search emits at most one symbol per frame and is frame-synchronous: its whole state at a frame boundary is the <= 16 hypotheses
// of the slot (token list, f64 score, hash, context state and score, n-gram state and score, two LSTM states each).  The pool kernels run the frame step of rnnt_prefix_beam_decode
// (prefix_step_rows / prefix_merge_rows, the same code) on rows that stay in HBM between calls, so a search fed in pieces is bit for
// bit the one-call search over the same frames, whatever the split.  Device state: rnnt_ctx::pp_*, rows slot * PB_MAX_BEAM + i of two
// buffer sets, allocated on the first use.  Host state per slot: the current set (PoolSlot::prefix_cur), and the frames walked, the beam
// and the two weights, use_context and graph generation, use_ngram and model generation of the search in progress (PoolSlot::prefix, a
// SearchSlot).
//
// Rules: a slot's search is fresh after a reset; its first advancing call fixes beam_size, ctc_weight, transducer_weight,
// use_context and use_ngram until the next reset (other values: RNNT_ERR_ARG).  A reset row holds the n-gram start MARKER (NG_START),
// which the first step resolves under the model of that first call; rnnt_ngram_set starts a new model generation, with the graph's
// rule for the searches that fuse it (the context keeps ONE model for this search and the CTC one, as it keeps one graph).  rnnt_context_set starts a new graph generation: a search biased
// under an older one holds node ids of a graph that no longer exists and is refused (RNNT_ERR_STATE) until its slot is reset;
// unbiased searches go on (the rule of api_pool_ctc.hip.inc).  Every refusal is decided before the first launch and changes nothing.

namespace {

// the device state, on the first use: every slot starts from [blank]; and room for a call's `frames` projected frames (and their
// CTC log-probabilities)
int pool_prefix_alloc(rnnt_ctx* ctx, hipStream_t s, size_t frames, bool with_ctc) {
    int rc;
    if ((rc = reserve(ctx, ctx->pp_encp, frames * D))) return rc;
    if (with_ctc && (rc = reserve(ctx, ctx->pp_ctc, frames * (size_t)ctx->cfg.vocab_size))) return rc;
    if (ctx->pp_nh) return RNNT_OK;
    const size_t B = (size_t)ctx->cfg.max_streams, R = B * PB_MAX_BEAM, lcap = (size_t)ctx->cfg.max_cache_frames + 1;
    for (int t = 0; t < 2; ++t) {
        if ((rc = reserve(ctx, ctx->pp_pool[t], R * 1024))) return rc;
        if ((rc = reserve(ctx, ctx->pp_tk[t], R * lcap))) return rc;
        if ((rc = reserve(ctx, ctx->pp_len[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_sc[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_hs[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_cst[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_cs[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_nst[t], R))) return rc;
        if ((rc = reserve(ctx, ctx->pp_ns[t], R))) return rc;
    }
    if ((rc = reserve(ctx, ctx->pp_toplp, R * PB_MAX_BEAM))) return rc;
    if ((rc = reserve(ctx, ctx->pp_toptok, R * PB_MAX_BEAM))) return rc;
    if ((rc = calltab_alloc(ctx, ctx->pp_tab, 2 * B))) return rc;
    if ((rc = reserve(ctx, ctx->pp_nh, B))) return rc;   // last: its presence says the state exists (pool_prefix_reset)
    hipLaunchKernelGGL(prefix_init_pool, dim3((unsigned)B), dim3(256), 0, s, pool_prefix_params(ctx), 0, (int)lcap, ctx->cfg.blank_id);   // host records stay: a reset slot is fresh there already
    LAUNCHCHK("prefix_init_pool");
    return RNNT_OK;
}

// Everything that can refuse an advance of the listed slots by t frames, slot range and duplicates aside (rnnt_prefix_beam_decode's
// range, then the slots' own); changes nothing.
int pool_prefix_check(rnnt_ctx* ctx, const char* fn, int n, const int* slots, int t, int beam_size, float cw, float tw, int use_context, int use_ngram) {
    const int V = ctx->cfg.vocab_size;
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "%s: weights not finalized", fn);
    if (t < 1) return fail(ctx, RNNT_ERR_ARG, "%s: %d frames", fn, t);
    if (V > 512) return fail(ctx, RNNT_ERR_ARG, "%s: vocab %d > 512", fn, V);
    if (beam_size < 1 || beam_size > PB_MAX_BEAM || beam_size > V)
        return fail(ctx, RNNT_ERR_ARG, "%s: beam_size %d outside [1, min(%d, vocab %d)]", fn, beam_size, PB_MAX_BEAM, V);
    if (!(cw >= 0.f) || !(tw >= 0.f) || (cw == 0.f && tw == 0.f)) return fail(ctx, RNNT_ERR_ARG, "%s: weights %g / %g (negative, or both zero)", fn, cw, tw);
    if (cw > 0.f && !ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "%s: ctc_weight > 0 and ctc_head.ctc_lo.* not loaded", fn);
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "%s: use_context without a context graph (rnnt_context_set)", fn);
    if (use_ngram && !ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "%s: use_ngram without an n-gram model (rnnt_ngram_set)", fn);
    for (int i = 0; i < n; ++i) {
        const SearchSlot& q = ctx->slot[slots[i]].prefix;
        if (q.beam != 0 && (q.use_ngram != 0) != (use_ngram != 0))
            return fail(ctx, RNNT_ERR_ARG, "%s: slot %d: use_ngram %d differs from the search in progress (%d); reset the slot first", fn, slots[i], use_ngram != 0,
                        q.use_ngram);
        if (q.beam != 0 && q.use_ngram && q.ngen != ctx->ng_gen)
            return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the n-gram model changed since its search began; reset the slot first", fn, slots[i]);
    }
    return search_slot_check(ctx, fn, &PoolSlot::prefix, n, slots, t, beam_size, cw, tw, use_context, true);
}

// the frame loop: pool_prefix_check has passed, the state exists, pp_encp (and pp_ctc when cw > 0) hold the call's n * t compact rows
// and slots_dev / cur0_dev [n] are on their way to the device.  Launches only, 2 per frame; then the host bookkeeping.
int pool_prefix_launch(rnnt_ctx* ctx, hipStream_t s, int n, const int* slots, const int* slots_dev, const int* cur0_dev, int t, int beam_size, float cw,
                       float tw, int use_context, int use_ngram) {
    PrefixStepP p;
    memset(&p, 0, sizeof(p));
    dec_weights(ctx, p); p.encp = ctx->pp_encp; p.ctc = cw > 0.f ? ctx->pp_ctc.p : nullptr;
    p.top_lp = ctx->pp_toplp; p.top_tok = ctx->pp_toptok; p.vocab = ctx->cfg.vocab_size; p.k = beam_size; p.beam = beam_size; p.T = t;
    p.lcap = ctx->cfg.max_cache_frames + 1; p.tw = tw; p.cw = cw;
    PrefixMergeP m;
    memset(&m, 0, sizeof(m));
    m.top_lp = ctx->pp_toplp; m.top_tok = ctx->pp_toptok; m.lcap = p.lcap; m.k = beam_size; m.beam = beam_size; m.blank = ctx->cfg.blank_id;
    CpGraph graph;
    memset(&graph, 0, sizeof(graph));
    if (use_context) graph = ctx_graph_dev(ctx);
    NgTables ng;
    memset(&ng, 0, sizeof(ng));
    if (use_ngram) ng = ngram_dev(ctx);
    PrefixPoolP q = pool_prefix_params(ctx);
    q.slots = slots_dev; q.cur0 = cur0_dev;
    // One hypothesis per workgroup finishes a frame sooner while every workgroup gets a CU of its own; PB_GROUP hypotheses per
    // workgroup read the weights a quarter as often and win once the launch would run in rounds (DESIGN.md section 7: the measured
    // crossover lies near 1.5 workgroups per CU).  The results are the same bits either way.  RNNT_PREFIX_GROUP=1 / 4 forces one.
    const bool grouped = ctx->prefix_group == PB_GROUP || (ctx->prefix_group != 1 && 2 * (long long)n * beam_size > 3 * (long long)ctx->n_cus);
    const int groups = grouped ? (beam_size + PB_GROUP - 1) / PB_GROUP : beam_size;
    for (int f = 0; f < t; ++f) {
        p.f = f; m.f = f;
        {
            ProfScope prof(ctx, s, TAG_PREFIX_STEP_POOL);
            if (grouped) hipLaunchKernelGGL(prefix_step_pool<PB_GROUP>, dim3((unsigned)(n * groups)), dim3(512), 0, s, p, q, groups);
            else hipLaunchKernelGGL(prefix_step_pool<1>, dim3((unsigned)(n * groups)), dim3(512), 0, s, p, q, groups);
            LAUNCHCHK("prefix_step_pool");
        }
        {
            ProfScope prof(ctx, s, TAG_PREFIX_MERGE_POOL);
            if (use_context && use_ngram) hipLaunchKernelGGL(prefix_merge_pool_ctx_ngram, dim3(n), dim3(PB_NT), 0, s, m, q, graph, ng);
            else if (use_ngram) hipLaunchKernelGGL(prefix_merge_pool_ngram, dim3(n), dim3(PB_NT), 0, s, m, q, ng);
            else if (use_context) hipLaunchKernelGGL(prefix_merge_pool_ctx, dim3(n), dim3(PB_NT), 0, s, m, q, graph);
            else hipLaunchKernelGGL(prefix_merge_pool, dim3(n), dim3(PB_NT), 0, s, m, q);
            LAUNCHCHK("prefix_merge_pool");
        }
    }
    search_slot_commit(ctx, &PoolSlot::prefix, n, slots, t, beam_size, cw, tw, use_context);
    for (int i = 0; i < n; ++i) {
        ctx->slot[slots[i]].prefix_cur ^= t & 1;
        ctx->slot[slots[i]].prefix.use_ngram = use_ngram != 0;
        ctx->slot[slots[i]].prefix.ngen = ctx->ng_gen;
    }
    return RNNT_OK;
}

}  // namespace

int rnnt_stream_prefix_reset(rnnt_ctx* ctx, int32_t slot, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    const int B = ctx->cfg.max_streams;
    if (slot < -1 || slot >= B) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_prefix_reset: slot %d outside [-1, %d)", slot, B);
    return pool_prefix_reset(ctx, (hipStream_t)stream, slot < 0 ? 0 : slot, slot < 0 ? B : 1);
}

int rnnt_pool_prefix_frames(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, int32_t beam_size,
                            float ctc_weight, float transducer_weight, void* stream) {
    return rnnt_pool_prefix_frames_ctx(ctx, n_active, slots_host, enc_dev, t, beam_size, ctc_weight, transducer_weight, 0, stream);
}

int rnnt_pool_prefix_frames_ctx(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, int32_t beam_size,
                                float ctc_weight, float transducer_weight, int32_t use_context, void* stream) {
    return rnnt_pool_prefix_frames_ngram(ctx, n_active, slots_host, enc_dev, t, beam_size, ctc_weight, transducer_weight, use_context, 0, stream);
}

int rnnt_pool_prefix_frames_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, int32_t beam_size,
                                  float ctc_weight, float transducer_weight, int32_t use_context, int32_t use_ngram, void* stream) {
    const char* fn = "rnnt_pool_prefix_frames";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !enc_dev) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    int rc;
    if ((rc = pool_slots_check(ctx, fn, n_active, slots_host, ctx->cfg.max_streams))) return rc;
    if ((rc = pool_prefix_check(ctx, fn, n_active, slots_host, t, beam_size, ctc_weight, transducer_weight, use_context, use_ngram))) return rc;
    const size_t frames = (size_t)n_active * t;
    if (frames * 512 >= ((size_t)1 << 31)) return fail(ctx, RNNT_ERR_SHAPE, "%s: n_active=%d t=%d too large for one call", fn, n_active, t);
    hipStream_t s = (hipStream_t)stream;
    const bool with_ctc = ctc_weight > 0.f;
    if ((rc = pool_prefix_alloc(ctx, s, frames, with_ctc))) return rc;
    const int n = n_active;
    int* tab;
    if ((rc = calltab_fill(ctx, ctx->pp_tab, tab))) return rc;
    for (int i = 0; i < n; ++i) { tab[i] = slots_host[i]; tab[n + i] = ctx->slot[slots_host[i]].prefix_cur; }
    if ((rc = calltab_send(ctx, ctx->pp_tab, 2 * (size_t)n, s))) return rc;   // the call's table
    {   // joint.enc_ffn and log_softmax(ctc_lo(.)) over the call's rows with the kernel / tile choices of a small call, as
        // rnnt_prefix_beam_decode forms them: a frame's sums do not depend on the call it arrives in
        GemmCapScope cap(ctx);
        GemmP g = plain_gemm(enc_dev, D, ctx->wenc, D, ctx->benc, ctx->pp_encp, D, (int)frames, D, D);
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_ENC_PROJ))) return rc;
        if (with_ctc && (rc = rnnt_ctc_logprobs(ctx, enc_dev, (int)frames, ctx->pp_ctc, stream))) return rc;
    }
    return pool_prefix_launch(ctx, s, n, slots_host, ctx->pp_tab, ctx->pp_tab + n, t, beam_size, ctc_weight, transducer_weight, use_context, use_ngram);
}

int rnnt_stream_get_prefix(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host, int32_t* tokens_host,
                           double* scores_host, float* h_host, float* c_host, void* stream) {
    return rnnt_stream_get_prefix_ctx(ctx, slot, 0, cap_hyps, cap_tokens, n_hyp, lens_host, tokens_host, scores_host, nullptr, h_host, c_host, stream);
}

// The same for a biased search: scores_host are the totals (score + context score), ctx_scores_host [cap_hyps] (may be NULL) the
// context part -- the running one, or with final != 0 finalize's, i.e. what rnnt_prefix_beam_decode_ctx would return had the utterance
// ended here (no re-sort).  Reading changes nothing.  final != 0 on a search biased under an older graph generation: RNNT_ERR_STATE.
// An unbiased slot reads as rnnt_stream_get_prefix does, with context scores 0; a fresh slot too, but with final != 0 and a graph set
// it finalizes its root, as the one-call search over no frames does.
int rnnt_stream_get_prefix_ctx(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                               int32_t* tokens_host, double* scores_host, double* ctx_scores_host, float* h_host, float* c_host, void* stream) {
    return rnnt_stream_get_prefix_ngram(ctx, slot, final, cap_hyps, cap_tokens, n_hyp, lens_host, tokens_host, scores_host, ctx_scores_host, nullptr, h_host,
                                        c_host, stream);
}

// A slot whose search fuses the model reads with its n-gram scores in the totals whichever getter is called; ngram_scores_host
// [cap_hyps] (may be NULL) receives them: the running ones, or with final != 0 those with the end term (context finalize first, then
// the end term: total = score + finalized context score + (n-gram score + eos)).  final != 0 on a search fused under an older model
// generation: RNNT_ERR_STATE.  A slot that fuses no model -- a fresh one too -- reads n-gram scores 0.
int rnnt_stream_get_prefix_ngram(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                                 int32_t* tokens_host, double* scores_host, double* ctx_scores_host, double* ngram_scores_host, float* h_host, float* c_host,
                                 void* stream) {
    const char* fn = "rnnt_stream_get_prefix";
    if (!ctx) return RNNT_ERR_ARG;
    const bool query = !lens_host && !tokens_host && !scores_host && !h_host && !c_host;   // the sizes a read needs: host only
    if (!n_hyp || (!query && (!lens_host || !tokens_host || !scores_host || (!h_host != !c_host)))) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (slot < 0 || slot >= ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->cfg.max_streams);
    const SearchSlot q = ctx->slot[slot].prefix;
    const int beam = q.beam > 0 ? q.beam : 1;                        // a fresh slot holds [blank] alone
    if (query) {
        n_hyp[0] = beam; n_hyp[1] = q.frames_done; n_hyp[2] = 1 + q.frames_done;   // one symbol per frame at most, after the leading blank
        return RNNT_OK;
    }
    if (cap_hyps < beam) return fail(ctx, RNNT_ERR_ARG, "%s: beam %d, room for %d hypotheses", fn, beam, cap_hyps);
    if (cap_tokens < 1 + q.frames_done) return fail(ctx, RNNT_ERR_ARG, "%s: cap_tokens %d < 1 + %d frames", fn, cap_tokens, q.frames_done);
    SearchRead rd;
    int rc;
    if ((rc = search_slot_read(ctx, fn, slot, q, final, rd))) return rc;
    const bool fused = q.beam > 0 && q.use_ngram;
    if (fused && final && (!ctx->ng_on || q.ngen != ctx->ng_gen))
        return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: the n-gram model changed since its search began (final = 0 still reads it)", fn, slot);
    NgTables ng;
    memset(&ng, 0, sizeof(ng));
    if (fused && final) ng = ngram_dev(ctx);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pool_prefix_alloc(ctx, s, 0, false))) return rc;
    const size_t R = (size_t)beam, ocap = (size_t)q.frames_done + 1, with_states = h_host ? 1 : 0;
    const size_t out_bytes = prefix_out(nullptr, 1, R, ocap, with_states).bytes, out_doubles = (out_bytes + sizeof(double) - 1) / sizeof(double);
    if ((rc = reserve(ctx, ctx->pp_out, out_doubles))) return rc;
    hipLaunchKernelGGL(prefix_pack_pool, dim3((unsigned)R), dim3(256), 0, s, pool_prefix_params(ctx), slot, ctx->slot[slot].prefix_cur, beam,
                       ctx->cfg.max_cache_frames + 1, (int)ocap, (int)with_states, rd.biased ? 1 : 0, rd.fin ? ctx_graph_dev(ctx).nscore : nullptr, fused ? 1 : 0,
                       fused && final ? 1 : 0, ng, ctx->pp_out.p);
    LAUNCHCHK("prefix_pack_pool");
    std::vector<double> out(out_doubles);
    HIPCHK(hipMemcpyAsync(out.data(), ctx->pp_out, out_bytes, hipMemcpyDeviceToHost, s));                 // the download
    HIPCHK(hipStreamSynchronize(s));
    const PrefixOut o = prefix_out(out.data(), 1, R, ocap, with_states);
    const size_t H = (size_t)cap_hyps;
    *n_hyp = o.nh[0];
    std::fill(lens_host, lens_host + H, 0);
    std::fill(scores_host, scores_host + H, 0.0);
    std::fill(tokens_host, tokens_host + H * cap_tokens, 0);
    if (ctx_scores_host) std::fill(ctx_scores_host, ctx_scores_host + H, 0.0);
    if (ngram_scores_host) std::fill(ngram_scores_host, ngram_scores_host + H, 0.0);
    if (with_states) { std::fill(h_host, h_host + H * D, 0.f); std::fill(c_host, c_host + H * D, 0.f); }
    prefix_out_copy(o, R, ocap, (size_t)cap_tokens, lens_host, tokens_host, scores_host, ctx_scores_host, ngram_scores_host, h_host, c_host);
    return RNNT_OK;
}
