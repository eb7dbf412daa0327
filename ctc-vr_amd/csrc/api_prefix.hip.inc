// C ABI: WeNet's CTC-fused prefix beam search (wenet/transducer/search/prefix_beam_search.py:42-148) for a padded batch, the whole
// frame loop on the device.  Included by rnnt_api.hip inside extern "C".  Kernels: rnnt_prefix.hip.h.

// The merge of one frame for ONE utterance as a pure function (no context, no GPU; CPU tests), the C++ statement of
// prefix_beam_search.py:105-145: candidates per hypothesis j, per rank t with f64((f32)score_j + top_lp[j][t]); a blank candidate
// keeps the tokens of j and state slot 0, any other token appends and takes slot 1; sequential prefix fusion in candidate order
// (log_add of the list [survivor, candidate] in double, the first one's tokens and state stay); stable descending sort;
// truncation.  Hypotheses are passed flat: hyp_len[n_hyp], hyp_tokens (concatenated), hyp_score[n_hyp]; top_lp / top_tok
// [n_hyp][k]; outputs likewise (out_tokens needs room for beam_size * (longest input + 1) ints).  Returns the number of survivors.
//
// With a context graph g (rnnt_prefix_merge_ctx_host; search.py:95-104,169-171,214-235 carried over to this frame step): hypothesis j
// also holds a context state hyp_cst[j] and score hyp_cs[j]; a blank candidate copies them, any other token takes one
// forward_one_step from the state and adds its score; fusion keeps the first candidate's (both are functions of the token sequence);
// the sort key is score + context score.  out_score stays the fused score; out_cst / out_cs are the survivors' context state / score.
//
// With an n-gram model ng (rnnt_prefix_merge_ngram_host; the CTC search's rule carried over to this frame step): hypothesis j also
// holds an n-gram state hyp_nst[j] (NG_START before its first token) and score hyp_ns[j]; a blank candidate copies them, any other
// token takes one ng_step and adds its score; fusion keeps the first candidate's; the sort key is score + context score + n-gram
// score, left to right, a term whose feature is off left out.
namespace {
int ctx_graph_build(int n_phrases, const int32_t* lens, const int32_t* tokens, double context_score, int vocab, int blank, CtxGraph& g,
                    std::string& err);   // api_ctc_prefix.hip.inc

int prefix_merge_host_impl(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score, const float* top_lp,
                           const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t* out_len, int32_t* out_tokens,
                           double* out_score, int32_t* out_src_row, int32_t* out_src_slot, const CtxGraph* g, const int32_t* hyp_cst,
                           const double* hyp_cs, int32_t* out_cst, double* out_cs, const NgTables* ng = nullptr, const int32_t* hyp_nst = nullptr,
                           const double* hyp_ns = nullptr, int32_t* out_nst = nullptr, double* out_ns = nullptr) {
    if (n_hyp < 1 || k < 1 || beam_size < 1 || !hyp_len || !hyp_score || !top_lp || !top_tok || !out_len || !out_tokens || !out_score) return RNNT_ERR_ARG;
    struct Cand { std::vector<int> tokens; double score; int row, slot; int cst; double cs; int nst; double ns; };
    std::vector<Cand> fused;
    size_t off = 0;
    for (int j = 0; j < n_hyp; ++j) {
        if (hyp_len[j] < 0 || (hyp_len[j] > 0 && !hyp_tokens)) return RNNT_ERR_ARG;
        const float s32 = (float)hyp_score[j];                                      // torch.tensor([s.score])
        for (int t = 0; t < k; ++t) {
            const float sum = s32 + top_lp[(size_t)j * k + t];                      // :105, f32
            const int tok = top_tok[(size_t)j * k + t];
            Cand c{std::vector<int>(hyp_tokens + off, hyp_tokens + off + hyp_len[j]), (double)sum, j, tok == blank ? 0 : 1, 0, 0.0, NG_START, 0.0};
            if (tok != blank) c.tokens.push_back(tok);
            if (g) {                                                                // copy_context / update_context
                c.cst = hyp_cst[j];
                c.cs = hyp_cs[j];
                if (tok != blank)
                    c.cs += cg_step(g->fail.data(), g->off.data(), g->ctok.data(), g->cid.data(), g->tscore.data(), g->nscore.data(), g->oscore.data(),
                                    hyp_cst[j], tok, &c.cst);
            }
            if (ng) {
                c.nst = hyp_nst[j];
                c.ns = hyp_ns[j];
                if (tok != blank) c.ns += ng_step(*ng, hyp_nst[j], tok, &c.nst);
            }
            bool merged = false;
            for (Cand& f : fused)
                if (f.tokens == c.tokens) {
                    f.score = prefix_log_add(f.score, c.score);                     // :136-138
                    merged = true;
                    break;
                }
            if (!merged) fused.push_back(std::move(c));
        }
        off += hyp_len[j];
    }
    if (g && ng) std::stable_sort(fused.begin(), fused.end(), [](const Cand& a, const Cand& b) { return a.score + a.cs + a.ns > b.score + b.cs + b.ns; });
    else if (ng) std::stable_sort(fused.begin(), fused.end(), [](const Cand& a, const Cand& b) { return a.score + a.ns > b.score + b.ns; });
    else if (g) std::stable_sort(fused.begin(), fused.end(), [](const Cand& a, const Cand& b) { return a.score + a.cs > b.score + b.cs; });
    else std::stable_sort(fused.begin(), fused.end(), [](const Cand& a, const Cand& b) { return a.score > b.score; });
    if ((int)fused.size() > beam_size) fused.resize(beam_size);
    off = 0;
    for (size_t a = 0; a < fused.size(); ++a) {
        out_len[a] = (int)fused[a].tokens.size();
        for (int t : fused[a].tokens) out_tokens[off++] = t;
        out_score[a] = fused[a].score;
        if (out_src_row) out_src_row[a] = fused[a].row;
        if (out_src_slot) out_src_slot[a] = fused[a].slot;
        if (out_cst) out_cst[a] = fused[a].cst;
        if (out_cs) out_cs[a] = fused[a].cs;
        if (out_nst) out_nst[a] = fused[a].nst;
        if (out_ns) out_ns[a] = fused[a].ns;
    }
    return (int)fused.size();
}
}  // namespace

int rnnt_prefix_merge_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score, const float* top_lp,
                           const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t* out_len, int32_t* out_tokens,
                           double* out_score, int32_t* out_src_row, int32_t* out_src_slot) {
    return prefix_merge_host_impl(n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score, out_src_row,
                                  out_src_slot, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// The same with the graph over n_phrases token lists (as rnnt_ctc_prefix_beam_host takes them; tokens only need to be >= 0 here) and
// the hypotheses' context states (node ids of that graph) and scores.  Returns the number of survivors.
int rnnt_prefix_merge_ctx_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score, const int32_t* hyp_ctx_state,
                               const double* hyp_ctx_score, const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size,
                               int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score, int32_t* out_len,
                               int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot, int32_t* out_ctx_state,
                               double* out_ctx_score) {
    if (n_phrases < 1 || n_hyp < 1 || !hyp_ctx_state || !hyp_ctx_score || !out_ctx_state || !out_ctx_score) return RNNT_ERR_ARG;
    CtxGraph g;
    std::string err;
    const int rc = ctx_graph_build(n_phrases, phrase_lens, phrase_tokens, context_score, -1, -1, g, err);
    if (rc) return rc;
    for (int j = 0; j < n_hyp; ++j)
        if (hyp_ctx_state[j] < 0 || hyp_ctx_state[j] >= (int)g.token.size()) return RNNT_ERR_ARG;
    return prefix_merge_host_impl(n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score, out_src_row,
                                  out_src_slot, &g, hyp_ctx_state, hyp_ctx_score, out_ctx_state, out_ctx_score);
}

// The same with the n-gram model, passed as the list rnnt_ngram_walk_host takes (n_ngrams == 0: none) over the given vocabulary, and
// the hypotheses' n-gram states (node ids of that model, or -1 = the start marker) and scores; n_phrases == 0: no graph (the context
// arguments may then be NULL, out_ctx_state / out_ctx_score receive 0).  Returns the number of survivors.
int rnnt_prefix_merge_ngram_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score, const int32_t* hyp_ctx_state,
                                 const double* hyp_ctx_score, const int32_t* hyp_ng_state, const double* hyp_ng_score, const float* top_lp,
                                 const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens,
                                 const int32_t* phrase_tokens, double context_score, int32_t n_ngrams, const int32_t* ngram_lens, const int32_t* ngram_tokens,
                                 const double* logp, const double* bow, double lm_weight, double length_bonus, double unk_logp, int32_t vocab,
                                 int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot,
                                 int32_t* out_ctx_state, double* out_ctx_score, int32_t* out_ng_state, double* out_ng_score) {
    if (n_phrases < 0 || n_ngrams < 0 || n_hyp < 1 || !top_tok || k < 1) return RNNT_ERR_ARG;
    if (n_phrases > 0 && (!hyp_ctx_state || !hyp_ctx_score || !out_ctx_state || !out_ctx_score)) return RNNT_ERR_ARG;
    if (n_ngrams > 0 && (!hyp_ng_state || !hyp_ng_score || !out_ng_state || !out_ng_score)) return RNNT_ERR_ARG;
    CtxGraph g;
    NgModel m;
    std::string err;
    int rc;
    if (n_phrases > 0) {
        if ((rc = ctx_graph_build(n_phrases, phrase_lens, phrase_tokens, context_score, -1, -1, g, err))) return rc;
        for (int j = 0; j < n_hyp; ++j)
            if (hyp_ctx_state[j] < 0 || hyp_ctx_state[j] >= (int)g.token.size()) return RNNT_ERR_ARG;
    }
    NgTables t{};
    if (n_ngrams > 0) {
        if ((rc = ngram_build(n_ngrams, ngram_lens, ngram_tokens, logp, bow, lm_weight, length_bonus, unk_logp, vocab, blank, m, err))) return rc;
        for (int j = 0; j < n_hyp; ++j)
            if (hyp_ng_state[j] < NG_START || hyp_ng_state[j] >= (int)m.fail.size()) return RNNT_ERR_ARG;
        for (int q = 0; q < n_hyp * k; ++q)                          // the root's row has vocab + 2 entries
            if (top_tok[q] != blank && !ngram_token_ok(top_tok[q], vocab, blank)) return RNNT_ERR_ARG;
        t = m.tables();
    }
    const int n = prefix_merge_host_impl(n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score,
                                         out_src_row, out_src_slot, n_phrases > 0 ? &g : nullptr, hyp_ctx_state, hyp_ctx_score,
                                         n_phrases > 0 ? out_ctx_state : nullptr, n_phrases > 0 ? out_ctx_score : nullptr, n_ngrams > 0 ? &t : nullptr,
                                         hyp_ng_state, hyp_ng_score, n_ngrams > 0 ? out_ng_state : nullptr, n_ngrams > 0 ? out_ng_score : nullptr);
    for (int a = 0; a < n; ++a) {
        if (n_phrases == 0 && out_ctx_state) out_ctx_state[a] = 0;
        if (n_phrases == 0 && out_ctx_score) out_ctx_score[a] = 0.0;
        if (n_ngrams == 0 && out_ng_state) out_ng_state[a] = NG_START;
        if (n_ngrams == 0 && out_ng_score) out_ng_score[a] = 0.0;
    }
    return n;
}

namespace {
// The call's own buffers: rows = B * beam fixed rows, token lists of lcap ints, `frames` = B * T projected frames.
struct PrefixBuf {
    float *encp, *ctc, *pool[2], *top_lp;
    int *tk[2], *len[2], *nh, *lens, *top_tok, *src_row, *src_slot, *cst[2], *nst[2];
    double *sc[2], *cs[2], *ns[2];
    unsigned long long* hs[2];
};
int prefix_buffers(rnnt_ctx* ctx, size_t B, size_t rows, size_t lcap, size_t frames, bool with_ctc, int k, PrefixBuf& o) {
    const size_t V = ctx->cfg.vocab_size;
    Carve<float> f;
    Carve<int> i;
    Carve<double> d;
    auto lay = [&] {
        o.encp = f.take(frames * D);
        o.ctc = with_ctc ? f.take(frames * V) : nullptr;
        for (float*& q : o.pool) q = f.take(rows * 1024);
        o.top_lp = f.take(rows * k);
        for (int*& q : o.tk) q = i.take(rows * lcap);
        for (int*& q : o.len) q = i.take(rows);
        o.nh = i.take(B);
        o.lens = i.take(B);
        o.top_tok = i.take(rows * k);
        o.src_row = i.take(rows);
        o.src_slot = i.take(rows);
        for (int*& q : o.cst) q = i.take(rows);
        for (int*& q : o.nst) q = i.take(rows);
        for (double*& q : o.sc) q = d.take(rows);
        for (double*& q : o.cs) q = d.take(rows);
        for (double*& q : o.ns) q = d.take(rows);
        for (unsigned long long*& q : o.hs) q = reinterpret_cast<unsigned long long*>(d.take(rows));
    };
    lay();   // sizes
    int rc;
    if ((rc = reserve(ctx, ctx->pb_f, f.off))) return rc;
    if ((rc = reserve(ctx, ctx->pb_i, i.off))) return rc;
    if ((rc = reserve(ctx, ctx->pb_d, d.off))) return rc;
    f = {ctx->pb_f}; i = {ctx->pb_i}; d = {ctx->pb_d};
    lay();   // pointers
    return RNNT_OK;
}

PrefixMergeP prefix_merge_params(const PrefixBuf& u, int t, bool states, int lcap, int k, int beam, int blank, int f) {
    PrefixMergeP m;
    memset(&m, 0, sizeof(m));
    if (states) { m.pool_in = u.pool[t]; m.pool_out = u.pool[t ^ 1]; }
    m.tk_in = u.tk[t]; m.tk_out = u.tk[t ^ 1];
    m.len_in = u.len[t]; m.len_out = u.len[t ^ 1];
    m.sc_in = u.sc[t]; m.sc_out = u.sc[t ^ 1];
    m.hs_in = u.hs[t]; m.hs_out = u.hs[t ^ 1];
    m.nh = u.nh; m.lens = u.lens; m.top_lp = u.top_lp; m.top_tok = u.top_tok; m.src_row = u.src_row; m.src_slot = u.src_slot;
    m.lcap = lcap; m.k = k; m.beam = beam; m.blank = blank; m.f = f;
    return m;
}

// the graph and set t's context rows; one prefix_merge launch, biased when g.fail != nullptr
PrefixCtxP prefix_ctx_params(const PrefixBuf& u, int t, const CpGraph& g) {
    PrefixCtxP x;
    memset(&x, 0, sizeof(x));
    x.g = g; x.cst_in = u.cst[t]; x.cst_out = u.cst[t ^ 1]; x.cs_in = u.cs[t]; x.cs_out = u.cs[t ^ 1];
    return x;
}
// the model and set t's n-gram rows
PrefixNgP prefix_ng_params(const PrefixBuf& u, int t, const NgTables& ng) {
    PrefixNgP n;
    memset(&n, 0, sizeof(n));
    n.g = ng; n.nst_in = u.nst[t]; n.nst_out = u.nst[t ^ 1]; n.ns_in = u.ns[t]; n.ns_out = u.ns[t ^ 1];
    return n;
}
// one prefix_merge launch: biased when g.fail != nullptr, fused with the model when ng.fail != nullptr -- four kernels, so that a
// search pays for what it uses only
int launch_prefix_merge(rnnt_ctx* ctx, hipStream_t s, int B, const PrefixMergeP& m, const PrefixBuf& u, int t, const CpGraph& g, const NgTables& ng) {
    ProfScope prof(ctx, s, TAG_PREFIX_MERGE);
    if (g.fail && ng.fail) hipLaunchKernelGGL(prefix_merge_ctx_ngram, dim3(B), dim3(PB_NT), 0, s, m, prefix_ctx_params(u, t, g), prefix_ng_params(u, t, ng));
    else if (ng.fail) hipLaunchKernelGGL(prefix_merge_ngram, dim3(B), dim3(PB_NT), 0, s, m, prefix_ng_params(u, t, ng));
    else if (g.fail) hipLaunchKernelGGL(prefix_merge_ctx, dim3(B), dim3(PB_NT), 0, s, m, prefix_ctx_params(u, t, g));
    else hipLaunchKernelGGL(prefix_merge, dim3(B), dim3(PB_NT), 0, s, m);
    LAUNCHCHK("prefix_merge");
    return RNNT_OK;
}
}  // namespace

// Prefix beam search of a padded batch in one call: joint.enc_ffn and the CTC log-probabilities of the B*T frames once, then per
// frame one prefix_step launch (one workgroup per live hypothesis) and one prefix_merge launch (one workgroup per utterance) over
// fixed rows b * beam + i with ping-pong buffers; one upload (the lengths), one download (prefix_pack's block), one
// synchronisation.  Touches nothing but its own buffers: streaming, pool and lock-step beam state stay as they are.
int rnnt_prefix_beam_decode(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                            float ctc_weight, float transducer_weight, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                            int32_t* tokens_host, double* scores_host, float* h_host, float* c_host, void* stream) {
    return rnnt_prefix_beam_decode_ctx(ctx, enc_dev, enc_lens_host, B, T, beam_size, ctc_weight, transducer_weight, 0, cap_tokens, n_hyp_host, lens_host,
                                       tokens_host, scores_host, nullptr, h_host, c_host, stream);
}

// The same with hot-word biasing by the graph of rnnt_context_set when use_context != 0 (none set: RNNT_ERR_STATE, before the first
// launch): prefix_merge keeps a context state and score per hypothesis and orders by the total; at the end finalize replaces the
// context scores (no re-sort, so the totals need not descend).  scores_host are the totals, ctx_scores_host [B, beam_size] (may be
// NULL) their context part.  use_context == 0: the unbiased search, bit for bit, context scores 0.
int rnnt_prefix_beam_decode_ctx(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                float ctc_weight, float transducer_weight, int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host,
                                int32_t* lens_host, int32_t* tokens_host, double* scores_host, double* ctx_scores_host, float* h_host, float* c_host,
                                void* stream) {
    return rnnt_prefix_beam_decode_ngram(ctx, enc_dev, enc_lens_host, B, T, beam_size, ctc_weight, transducer_weight, use_context, 0, cap_tokens, n_hyp_host,
                                         lens_host, tokens_host, scores_host, ctx_scores_host, nullptr, h_host, c_host, stream);
}

// The same with the model of rnnt_ngram_set fused when use_ngram != 0 (none set: RNNT_ERR_STATE, before the first launch):
// prefix_merge also keeps an n-gram state and score per hypothesis and orders by score + context score + n-gram score; at the end
// every survivor's n-gram score gains the end term of its state (no re-sort).  scores_host are the totals, ngram_scores_host
// [B, beam_size] (may be NULL) their n-gram part.  use_ngram == 0: rnnt_prefix_beam_decode_ctx, bit for bit, n-gram scores 0.
int rnnt_prefix_beam_decode_ngram(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                  float ctc_weight, float transducer_weight, int32_t use_context, int32_t use_ngram, int32_t cap_tokens,
                                  int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host, double* scores_host, double* ctx_scores_host,
                                  double* ngram_scores_host, float* h_host, float* c_host, void* stream) {
    if (!ctx || !enc_dev || !enc_lens_host || !n_hyp_host || !lens_host || !tokens_host || !scores_host || (!h_host != !c_host))
        return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: null argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    const int V = ctx->cfg.vocab_size, blank = ctx->cfg.blank_id;
    if (B < 1 || T < 0) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: B=%d T=%d", B, T);
    if (V > 512) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: vocab %d > 512", V);
    if (beam_size < 1 || beam_size > PB_MAX_BEAM || beam_size > V)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: beam_size %d outside [1, min(%d, vocab %d)]", beam_size, PB_MAX_BEAM, V);
    if (!(ctc_weight >= 0.f) || !(transducer_weight >= 0.f) || (ctc_weight == 0.f && transducer_weight == 0.f))
        return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: weights %g / %g (negative, or both zero)", ctc_weight, transducer_weight);
    int fmax = 0;
    for (int b = 0; b < B; ++b) {
        if (enc_lens_host[b] < 0 || enc_lens_host[b] > T)
            return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: utterance %d has %d frames, outside [0, %d]", b, enc_lens_host[b], T);
        fmax = std::max(fmax, enc_lens_host[b]);
    }
    if (cap_tokens < 1 + fmax) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_beam_decode: cap_tokens %d < 1 + %d frames", cap_tokens, fmax);
    const bool with_ctc = ctc_weight > 0.f;
    if (with_ctc && !ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_prefix_beam_decode: ctc_weight > 0 and ctc_head.ctc_lo.* not loaded");
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_prefix_beam_decode: use_context without a context graph (rnnt_context_set)");
    if (use_ngram && !ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_prefix_beam_decode: use_ngram without an n-gram model (rnnt_ngram_set)");
    const size_t frames = (size_t)B * T, R = (size_t)B * beam_size, lcap = (size_t)fmax + 1;
    if (frames * 512 >= ((size_t)1 << 31) || R * lcap >= ((size_t)1 << 31))
        return fail(ctx, RNNT_ERR_SHAPE, "rnnt_prefix_beam_decode: B=%d T=%d beam=%d too large for one call", B, T, beam_size);
    hipStream_t s = (hipStream_t)stream;
    const int k = beam_size, with_states = h_host ? 1 : 0;
    int rc;
    PrefixBuf u;
    if ((rc = prefix_buffers(ctx, B, R, lcap, frames, with_ctc, k, u))) return rc;
    const size_t out_bytes = prefix_out(nullptr, B, R, lcap, with_states).bytes, out_doubles = (out_bytes + sizeof(double) - 1) / sizeof(double);
    if ((rc = reserve(ctx, ctx->pb_out, out_doubles))) return rc;
    CpGraph graph;
    memset(&graph, 0, sizeof(graph));
    if (use_context) graph = ctx_graph_dev(ctx);
    NgTables ng;
    memset(&ng, 0, sizeof(ng));
    if (use_ngram) ng = ngram_dev(ctx);
    HIPCHK(hipMemcpyAsync(u.lens, enc_lens_host, B * sizeof(int), hipMemcpyHostToDevice, s));            // the upload
    hipLaunchKernelGGL(prefix_init, dim3(B), dim3(256), 0, s, u.pool[0], u.tk[0], u.len[0], u.sc[0], u.hs[0], u.cst[0], u.cs[0], u.nst[0], u.ns[0], u.nh,
                       beam_size, (int)lcap, blank);
    LAUNCHCHK("prefix_init");
    if (fmax > 0) {   // once per call: joint.enc_ffn and log_softmax(ctc_lo(.)) over the B*T frames, with the kernel / tile choices of a
                      // small call whatever B is, so that an utterance's sums do not depend on the batch it is in
        GemmCapScope cap(ctx);
        GemmP g = plain_gemm(enc_dev, D, ctx->wenc, D, ctx->benc, u.encp, D, (int)frames, D, D);
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_ENC_PROJ))) return rc;
        if (with_ctc && (rc = rnnt_ctc_logprobs(ctx, enc_dev, (int)frames, u.ctc, stream))) return rc;
    }
    PrefixStepP p;
    memset(&p, 0, sizeof(p));
    dec_weights(ctx, p); p.encp = u.encp; p.ctc = u.ctc; p.nh = u.nh; p.lens = u.lens;
    p.top_lp = u.top_lp; p.top_tok = u.top_tok; p.vocab = V; p.k = k; p.beam = beam_size; p.T = T; p.lcap = (int)lcap;
    p.tw = transducer_weight; p.cw = ctc_weight;
    int t = 0;
    for (int f = 0; f < fmax; ++f) {   // launches only
        p.pool = u.pool[t]; p.tk = u.tk[t]; p.len = u.len[t]; p.f = f;
        {
            ProfScope prof(ctx, s, TAG_PREFIX_STEP);
            hipLaunchKernelGGL(prefix_step, dim3((unsigned)R), dim3(512), 0, s, p);
            LAUNCHCHK("prefix_step");
        }
        if ((rc = launch_prefix_merge(ctx, s, B, prefix_merge_params(u, t, true, (int)lcap, k, beam_size, blank, f), u, t, graph, ng))) return rc;
        t ^= 1;
    }
    hipLaunchKernelGGL(prefix_pack, dim3((unsigned)R), dim3(256), 0, s, u.pool[t], u.tk[t], u.len[t], u.sc[t], use_context ? u.cst[t] : nullptr, u.cs[t],
                       graph.nscore, use_ngram ? u.nst[t] : nullptr, u.ns[t], ng, u.nh, B, beam_size, (int)lcap, with_states, ctx->pb_out.p);
    LAUNCHCHK("prefix_pack");
    std::vector<double> out(out_doubles);
    HIPCHK(hipMemcpyAsync(out.data(), ctx->pb_out, out_bytes, hipMemcpyDeviceToHost, s));                // the download
    HIPCHK(hipStreamSynchronize(s));
    const PrefixOut o = prefix_out(out.data(), B, R, lcap, with_states);
    memcpy(n_hyp_host, o.nh, B * sizeof(int));
    prefix_out_copy(o, R, lcap, (size_t)cap_tokens, lens_host, tokens_host, scores_host, ctx_scores_host, ngram_scores_host, h_host, c_host);
    return RNNT_OK;
}

// One prefix_merge launch on flat host inputs for ONE utterance (test seam against rnnt_prefix_merge_host): same arguments and
// results.  Uses the prefix search's own buffers only; no LSTM state is gathered.  Synchronises.
namespace {
int prefix_merge_device_impl(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                             const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t* out_len,
                             int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot, void* stream, bool biased,
                             const int32_t* hyp_cst, const double* hyp_cs, int32_t* out_cst, double* out_cs, bool fused = false,
                             const int32_t* hyp_nst = nullptr, const double* hyp_ns = nullptr, int32_t* out_nst = nullptr, double* out_ns = nullptr) {
    if (!ctx) return RNNT_ERR_ARG;
    if (fused) {
        if (!hyp_nst || !hyp_ns || !out_nst || !out_ns || !top_tok) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_ngram_device: null argument");
        if (!ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_prefix_merge_ngram_device: no n-gram model (rnnt_ngram_set)");
        for (int i = 0; i < n_hyp && i < PB_MAX_BEAM; ++i)
            if (hyp_nst[i] < NG_START || hyp_nst[i] >= (int)ctx->ng.fail.size())
                return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_ngram_device: hypothesis %d: n-gram state %d outside the model's %d nodes", i, hyp_nst[i],
                            (int)ctx->ng.fail.size());
        if (n_hyp >= 1 && n_hyp <= PB_MAX_BEAM && k >= 1 && k <= PB_MAX_BEAM)
            for (int q = 0; q < n_hyp * k; ++q)                      // the root's row has vocab_size + 2 entries
                if (top_tok[q] != blank && !ngram_token_ok(top_tok[q], ctx->cfg.vocab_size, ctx->cfg.blank_id))
                    return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_ngram_device: candidate token %d outside the vocabulary or the model's blank", top_tok[q]);
    }
    if (biased) {
        if (!hyp_cst || !hyp_cs || !out_cst || !out_cs) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_ctx_device: null argument");
        if (!ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_prefix_merge_ctx_device: no context graph (rnnt_context_set)");
        for (int i = 0; i < n_hyp && i < PB_MAX_BEAM; ++i)
            if (hyp_cst[i] < 0 || hyp_cst[i] >= (int)ctx->cg.token.size())
                return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_ctx_device: hypothesis %d: context state %d outside the graph's %d nodes", i, hyp_cst[i],
                            (int)ctx->cg.token.size());
    }
    if (!hyp_len || !hyp_score || !top_lp || !top_tok || !out_len || !out_tokens || !out_score)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_device: null argument");
    if (n_hyp < 1 || n_hyp > PB_MAX_BEAM || k < 1 || k > PB_MAX_BEAM || beam_size < 1 || beam_size > PB_MAX_BEAM)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_device: n_hyp %d, k %d, beam %d outside [1, %d]", n_hyp, k, beam_size, PB_MAX_BEAM);
    size_t lmax = 0, ntok = 0;
    for (int i = 0; i < n_hyp; ++i) {
        if (hyp_len[i] < 0) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_device: bad hypothesis %d", i);
        lmax = std::max(lmax, (size_t)hyp_len[i]);
        ntok += hyp_len[i];
    }
    if (ntok && !hyp_tokens) return fail(ctx, RNNT_ERR_ARG, "rnnt_prefix_merge_device: null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t lcap = lmax + 1, width = std::max(n_hyp, beam_size);
    int rc;
    PrefixBuf u;
    if ((rc = prefix_buffers(ctx, 1, width, lcap, 0, false, k, u))) return rc;
    std::vector<int> toks(width * lcap, 0), len(width, 0), nh(1, n_hyp);
    std::vector<double> sc(width, 0.0);
    std::vector<unsigned long long> hs(width, BEAM_HASH0);
    for (int i = 0, off = 0; i < n_hyp; off += hyp_len[i], ++i) {
        std::copy(hyp_tokens + off, hyp_tokens + off + hyp_len[i], toks.begin() + (size_t)i * lcap);
        len[i] = hyp_len[i];
        sc[i] = hyp_score[i];
        hs[i] = beam_hash(hyp_tokens + off, hyp_len[i]);
    }
    HIPCHK(hipMemcpyAsync(u.tk[0], toks.data(), toks.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.len[0], len.data(), width * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.sc[0], sc.data(), width * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.hs[0], hs.data(), width * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.nh, nh.data(), sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.top_lp, top_lp, (size_t)n_hyp * k * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(u.top_tok, top_tok, (size_t)n_hyp * k * sizeof(int), hipMemcpyHostToDevice, s));
    CpGraph graph;
    memset(&graph, 0, sizeof(graph));
    std::vector<int> cst(width, 0);
    std::vector<double> cs(width, 0.0);
    if (biased) {
        graph = ctx_graph_dev(ctx);
        std::copy(hyp_cst, hyp_cst + n_hyp, cst.begin());
        std::copy(hyp_cs, hyp_cs + n_hyp, cs.begin());
        HIPCHK(hipMemcpyAsync(u.cst[0], cst.data(), width * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(u.cs[0], cs.data(), width * sizeof(double), hipMemcpyHostToDevice, s));
    }
    NgTables ng;
    memset(&ng, 0, sizeof(ng));
    std::vector<int> nst(width, NG_START), onst(width, NG_START);
    std::vector<double> ns(width, 0.0), ons(width, 0.0);
    if (fused) {
        ng = ngram_dev(ctx);
        std::copy(hyp_nst, hyp_nst + n_hyp, nst.begin());
        std::copy(hyp_ns, hyp_ns + n_hyp, ns.begin());
        HIPCHK(hipMemcpyAsync(u.nst[0], nst.data(), width * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(u.ns[0], ns.data(), width * sizeof(double), hipMemcpyHostToDevice, s));
    }
    PrefixMergeP m = prefix_merge_params(u, 0, false, (int)lcap, k, beam_size, blank, 0);
    m.lens = nullptr;                                                // the utterance has this frame
    if ((rc = launch_prefix_merge(ctx, s, 1, m, u, 0, graph, ng))) return rc;
    std::vector<int> srow(width), sslot(width), ocst(width, 0);
    std::vector<double> ocs(width, 0.0);
    if (fused) {
        HIPCHK(hipMemcpyAsync(onst.data(), u.nst[1], width * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ons.data(), u.ns[1], width * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    if (biased) {
        HIPCHK(hipMemcpyAsync(ocst.data(), u.cst[1], width * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ocs.data(), u.cs[1], width * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(nh.data(), u.nh, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), u.len[1], width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sc.data(), u.sc[1], width * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(toks.data(), u.tk[1], toks.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(srow.data(), u.src_row, width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sslot.data(), u.src_slot, width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    size_t off = 0;
    for (int a = 0; a < nh[0]; ++a) {
        out_len[a] = len[a];
        for (int q = 0; q < len[a]; ++q) out_tokens[off++] = toks[(size_t)a * lcap + q];
        out_score[a] = sc[a];
        if (out_src_row) out_src_row[a] = srow[a];
        if (out_src_slot) out_src_slot[a] = sslot[a];
        if (biased) { out_cst[a] = ocst[a]; out_cs[a] = ocs[a]; }
        if (fused) { out_nst[a] = onst[a]; out_ns[a] = ons[a]; }
    }
    return nh[0];
}
}  // namespace

int rnnt_prefix_merge_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                             const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t* out_len,
                             int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot, void* stream) {
    return prefix_merge_device_impl(ctx, n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score,
                                    out_src_row, out_src_slot, stream, false, nullptr, nullptr, nullptr, nullptr);
}

// One prefix_merge launch with the graph that is set on the context (none: RNNT_ERR_STATE): rnnt_prefix_merge_device's arguments plus
// the hypotheses' context states and scores; the survivors' come back in out_ctx_state / out_ctx_score, out_score stays the fused score.
int rnnt_prefix_merge_ctx_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                                 const int32_t* hyp_ctx_state, const double* hyp_ctx_score, const float* top_lp, const int32_t* top_tok, int32_t k,
                                 int32_t blank, int32_t beam_size, int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row,
                                 int32_t* out_src_slot, int32_t* out_ctx_state, double* out_ctx_score, void* stream) {
    return prefix_merge_device_impl(ctx, n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score,
                                    out_src_row, out_src_slot, stream, true, hyp_ctx_state, hyp_ctx_score, out_ctx_state, out_ctx_score);
}

// One prefix_merge launch with the model that is set on the context (none: RNNT_ERR_STATE) and, when use_context != 0, its graph:
// rnnt_prefix_merge_ctx_device's arguments plus the hypotheses' n-gram states (node ids, or -1 = the start marker) and scores; the
// survivors' come back in out_ng_state / out_ng_score.  use_context == 0: the context arguments may be NULL (outputs, if given, 0).
int rnnt_prefix_merge_ngram_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                                   const int32_t* hyp_ctx_state, const double* hyp_ctx_score, const int32_t* hyp_ng_state, const double* hyp_ng_score,
                                   const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size, int32_t use_context,
                                   int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot,
                                   int32_t* out_ctx_state, double* out_ctx_score, int32_t* out_ng_state, double* out_ng_score, void* stream) {
    const int n = prefix_merge_device_impl(ctx, n_hyp, hyp_len, hyp_tokens, hyp_score, top_lp, top_tok, k, blank, beam_size, out_len, out_tokens, out_score,
                                           out_src_row, out_src_slot, stream, use_context != 0, hyp_ctx_state, hyp_ctx_score, out_ctx_state, out_ctx_score,
                                           true, hyp_ng_state, hyp_ng_score, out_ng_state, out_ng_score);
    if (!use_context)
        for (int a = 0; a < n; ++a) {
            if (out_ctx_state) out_ctx_state[a] = 0;
            if (out_ctx_score) out_ctx_score[a] = 0.0;
        }
    return n;
}
