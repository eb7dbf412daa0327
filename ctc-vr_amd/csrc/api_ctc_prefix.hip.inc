// C ABI: WeNet's CTC prefix beam search (wenet/transformer/search.py:125-247) with contextual biasing by its Aho-Corasick
// ContextGraph (wenet/utils/context_graph.py), for a padded batch in ONE launch.  Included by rnnt_api.hip inside extern "C".
// Kernel: rnnt_ctc_prefix.hip.h.  The graph and the host statement of the search are pure C++ (no context, no GPU).

namespace {
// context_graph.py:144-210 on flat tables.  Node ids follow creation order (root = 0); `kids` keeps a node's children in insertion
// order (the order the reference's dicts iterate in), the CSR (off / ctok / cid) holds them sorted by token for the device.
int ctx_graph_build(int n_phrases, const int32_t* lens, const int32_t* tokens, double context_score, int vocab, int blank, CtxGraph& g,
                    std::string& err) {
    g = CtxGraph();
    if (n_phrases < 0 || (n_phrases > 0 && (!lens || !tokens))) { err = "null phrase list"; return RNNT_ERR_ARG; }
    std::vector<std::vector<std::pair<int, int>>> kids(1);
    auto child = [&](int node, int tok) {
        for (auto& kv : kids[node])
            if (kv.first == tok) return kv.second;
        return -1;
    };
    g.token = {-1}; g.tscore = {0.0}; g.nscore = {0.0}; g.oscore = {0.0}; g.is_end = {0};
    size_t at = 0;
    for (int ph = 0; ph < n_phrases; ++ph) {
        if (lens[ph] < 1) { err = "phrase " + std::to_string(ph) + " is empty"; return RNNT_ERR_ARG; }
        int node = 0;
        for (int i = 0; i < lens[ph]; ++i) {
            const int tok = tokens[at + i];
            if (tok < 0 || (vocab >= 0 && tok >= vocab)) { err = "phrase " + std::to_string(ph) + ": token " + std::to_string(tok) + " outside the vocabulary"; return RNNT_ERR_ARG; }
            if (vocab >= 0 && tok == blank) { err = "phrase " + std::to_string(ph) + " holds the blank"; return RNNT_ERR_ARG; }
            int c = child(node, tok);
            if (c < 0) {                                                             // :161-172: is_end is decided at creation only
                c = (int)g.token.size();
                if (c >= CP_MAX_NODES) { err = "more than " + std::to_string(CP_MAX_NODES) + " nodes"; return RNNT_ERR_ARG; }
                const bool end = i == lens[ph] - 1;
                const double ns = g.nscore[node] + context_score;
                g.token.push_back(tok); g.tscore.push_back(context_score); g.nscore.push_back(ns);
                g.oscore.push_back(end ? ns : 0.0); g.is_end.push_back(end ? 1 : 0);
                kids.emplace_back();
                kids[node].push_back({tok, c});
            }
            node = c;
        }
        at += lens[ph];
    }
    const int n = (int)g.token.size();
    g.fail.assign(n, 0); g.output.assign(n, -1);
    std::vector<int> queue;
    for (auto& kv : kids[0]) { g.fail[kv.second] = 0; queue.push_back(kv.second); }
    for (size_t qh = 0; qh < queue.size(); ++qh) {                                   // :186-210
        const int cur = queue[qh];
        for (auto& kv : kids[cur]) {
            const int tok = kv.first, node = kv.second;
            int f = g.fail[cur];
            if (child(f, tok) >= 0) f = child(f, tok);
            else {
                f = g.fail[f];
                while (child(f, tok) < 0) {
                    f = g.fail[f];
                    if (g.token[f] == -1) break;                                     // breaks AFTER stepping to the root
                }
                if (child(f, tok) >= 0) f = child(f, tok);
            }
            g.fail[node] = f;
            int out = f;
            while (!g.is_end[out]) {
                out = g.fail[out];
                if (g.token[out] == -1) { out = -1; break; }
            }
            g.output[node] = out;
            g.oscore[node] += out < 0 ? 0.0 : g.oscore[out];                         // accumulates along the output arc
            queue.push_back(node);
        }
    }
    g.off.assign(n + 1, 0);
    for (int v = 0; v < n; ++v) {
        std::sort(kids[v].begin(), kids[v].end());
        g.off[v + 1] = g.off[v] + (int)kids[v].size();
        for (auto& kv : kids[v]) { g.ctok.push_back(kv.first); g.cid.push_back(kv.second); }
    }
    return RNNT_OK;
}

double ctx_graph_step(const CtxGraph& g, int state, int tok, int* next) {
    return cg_step(g.fail.data(), g.off.data(), g.ctok.data(), g.cid.data(), g.tscore.data(), g.nscore.data(), g.oscore.data(), state, tok, next);
}

// One hypothesis of search.py's PrefixScore, plus its prefix.
struct CpHyp {
    std::vector<int> prefix, times_s, times_ns;
    double s = -INFINITY, ns = -INFINITY, v_s = -INFINITY, v_ns = -INFINITY, cur_token_prob = -INFINITY, context_score = 0.0;
    int context_state = 0;
    double ngram_score = 0.0;                                                        // with an n-gram model: its score and state
    int ngram_state = 0;
    bool has_context = false;
    double score() const { return prefix_log_add(s, ns); }
    double viterbi_score() const { return v_s > v_ns ? v_s : v_ns; }
    const std::vector<int>& times() const { return v_s > v_ns ? times_s : times_ns; }
    double total_score() const { return score() + context_score + ngram_score; }
};

// search.py:139-236 for one utterance: lp [len][V]; graph may be null.  The dictionary of a frame is a vector in first-insertion order.
// ng (may be null): an n-gram model fused under the same first-touch rule as the graph; its end term is added at the end.
void ctc_prefix_search_host(const float* lp, int len, int V, int blank, int beam, const CtxGraph* g, const NgModel* ng, std::vector<CpHyp>& cur) {
    const NgTables nt = ng ? ng->tables() : NgTables{};
    cur.assign(1, CpHyp());
    cur[0].s = 0.0; cur[0].v_s = 0.0; cur[0].v_ns = 0.0;
    if (ng) cur[0].ngram_state = nt.start;
    for (int t = 0; t < len; ++t) {
        const float* row = lp + (size_t)t * V;
        std::vector<unsigned long long> keys(V);
        for (int v = 0; v < V; ++v) keys[v] = cp_key(row[v], v);
        std::partial_sort(keys.begin(), keys.begin() + beam, keys.end(), std::greater<unsigned long long>());
        std::vector<CpHyp> next;
        auto entry = [&](const std::vector<int>& prefix) -> size_t {
            for (size_t e = 0; e < next.size(); ++e)
                if (next[e].prefix == prefix) return e;
            next.emplace_back();
            next.back().prefix = prefix;
            return next.size() - 1;
        };
        auto copy_context = [&](CpHyp& n, const CpHyp& h) {
            if ((!g && !ng) || n.has_context) return;
            n.context_score = h.context_score; n.context_state = h.context_state; n.has_context = true;
            n.ngram_score = h.ngram_score; n.ngram_state = h.ngram_state;
        };
        auto update_context = [&](CpHyp& n, const CpHyp& h, int u) {
            if ((!g && !ng) || n.has_context) return;
            int nx;
            if (g) {
                const double sc = ctx_graph_step(*g, h.context_state, u, &nx);
                n.context_score = h.context_score; n.context_score += sc; n.context_state = nx;
            }
            if (ng) {
                n.ngram_score = h.ngram_score + ng_step(nt, h.ngram_state, u, &nx);
                n.ngram_state = nx;
            }
            n.has_context = true;
        };
        for (int r = 0; r < beam; ++r) {
            const int u = cp_key_index(keys[r]);
            const double prob = (double)cp_key_value(keys[r]);
            for (size_t hi = 0; hi < cur.size(); ++hi) {
                const CpHyp h = cur[hi];                                             // by value: `next` never aliases `cur`, this is for clarity
                const int last = h.prefix.empty() ? -1 : h.prefix.back();
                if (u == blank) {
                    CpHyp& n = next[entry(h.prefix)];
                    n.s = prefix_log_add(n.s, h.score() + prob);
                    n.v_s = h.viterbi_score() + prob;
                    n.times_s = h.times();
                    copy_context(n, h);
                } else if (u == last) {
                    {
                        CpHyp& n1 = next[entry(h.prefix)];
                        n1.ns = prefix_log_add(n1.ns, h.ns + prob);
                        if (n1.v_ns < h.v_ns + prob) {
                            n1.v_ns = h.v_ns + prob;
                            if (n1.cur_token_prob < prob) {
                                n1.cur_token_prob = prob;
                                if (!h.times_ns.empty()) { n1.times_ns = h.times_ns; n1.times_ns.back() = t; }
                            }
                        }
                        copy_context(n1, h);
                    }
                    std::vector<int> np = h.prefix;
                    np.push_back(u);
                    CpHyp& n2 = next[entry(np)];
                    n2.ns = prefix_log_add(n2.ns, h.s + prob);
                    if (n2.v_ns < h.v_s + prob) {
                        n2.v_ns = h.v_s + prob; n2.cur_token_prob = prob;
                        n2.times_ns = h.times_s; n2.times_ns.push_back(t);
                    }
                    update_context(n2, h, u);
                } else {
                    std::vector<int> np = h.prefix;
                    np.push_back(u);
                    CpHyp& n = next[entry(np)];
                    n.ns = prefix_log_add(n.ns, h.score() + prob);
                    if (n.v_ns < h.viterbi_score() + prob) {
                        n.v_ns = h.viterbi_score() + prob; n.cur_token_prob = prob;
                        n.times_ns = h.times(); n.times_ns.push_back(t);
                    }
                    update_context(n, h, u);
                }
            }
        }
        std::stable_sort(next.begin(), next.end(), [](const CpHyp& a, const CpHyp& b) { return a.total_score() > b.total_score(); });
        if ((int)next.size() > beam) next.resize(beam);
        cur.swap(next);
    }
    if (g)
        for (CpHyp& h : cur) { h.context_score = -g->nscore[h.context_state]; h.context_state = 0; }   // :227-232, not re-sorted
    if (ng)
        for (CpHyp& h : cur) h.ngram_score += ng_eos(nt, h.ngram_state);                               // likewise
}

int ctc_prefix_check(rnnt_ctx* ctx, const char* who, const void* in, const int32_t* enc_lens, int B, int T, int V, int beam_size, int cap_tokens,
                     const void* n_hyp, const void* lens, const void* tokens, const void* times, const void* scores, int* fmax_out) {
    if (!in || !enc_lens || !n_hyp || !lens || !tokens || !times || !scores) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", who);
    if (B < 1 || T < 0) return fail(ctx, RNNT_ERR_ARG, "%s: B=%d T=%d", who, B, T);
    if (V < 1 || V > 512) return fail(ctx, RNNT_ERR_ARG, "%s: vocab %d outside [1, 512]", who, V);
    if (beam_size < 1 || beam_size > CP_MAX_BEAM || beam_size > V)
        return fail(ctx, RNNT_ERR_ARG, "%s: beam_size %d outside [1, min(%d, vocab %d)]", who, beam_size, CP_MAX_BEAM, V);
    int fmax = 0;
    for (int b = 0; b < B; ++b) {
        if (enc_lens[b] < 0 || enc_lens[b] > T) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d frames, outside [0, %d]", who, b, enc_lens[b], T);
        fmax = std::max(fmax, enc_lens[b]);
    }
    if (cap_tokens < fmax) return fail(ctx, RNNT_ERR_ARG, "%s: cap_tokens %d < %d frames", who, cap_tokens, fmax);
    *fmax_out = fmax;
    return RNNT_OK;
}
}  // namespace

// The automaton of context_graph.py:144-210 over n_phrases token lists (phrase_tokens_host concatenated), uploaded for the searches
// below; n_phrases == 0 clears it.  Refuses an empty phrase, a token outside [0, vocab), the blank, more than 4096 nodes.
int rnnt_context_set(rnnt_ctx* ctx, int32_t n_phrases, const int32_t* phrase_lens_host, const int32_t* phrase_tokens_host, double context_score) {
    if (!ctx) return RNNT_ERR_ARG;
    if (n_phrases == 0) {
        ctx->cg_on = false;
        ctx->cg = CtxGraph();
        ++ctx->cg_gen;
        return RNNT_OK;
    }
    CtxGraph g;
    std::string err;
    int rc = ctx_graph_build(n_phrases, phrase_lens_host, phrase_tokens_host, context_score, ctx->cfg.vocab_size, ctx->cfg.blank_id, g, err);
    if (rc) return fail(ctx, rc, "rnnt_context_set: %s", err.c_str());
    const size_t n = g.token.size(), m = g.ctok.size();
    if ((rc = reserve(ctx, ctx->cg_i, 2 * n + 1 + 2 * m))) return rc;
    if ((rc = reserve(ctx, ctx->cg_d, 3 * n))) return rc;
    HIPCHK(hipDeviceSynchronize());                                  // a search still reading the previous tables
    std::vector<int> hi;
    hi.insert(hi.end(), g.fail.begin(), g.fail.end());
    hi.insert(hi.end(), g.off.begin(), g.off.end());
    hi.insert(hi.end(), g.ctok.begin(), g.ctok.end());
    hi.insert(hi.end(), g.cid.begin(), g.cid.end());
    std::vector<double> hd;
    hd.insert(hd.end(), g.tscore.begin(), g.tscore.end());
    hd.insert(hd.end(), g.nscore.begin(), g.nscore.end());
    hd.insert(hd.end(), g.oscore.begin(), g.oscore.end());
    HIPCHK(hipMemcpy(ctx->cg_i, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->cg_d, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->cg = std::move(g);
    ctx->cg_on = true;
    ++ctx->cg_gen;                                                   // a pool search biased by the previous graph holds its node ids (api_pool_ctc.hip.inc)
    return RNNT_OK;
}

// Test seam (no context, no GPU): builds the graph, returns its node tables (each out-pointer may be NULL; *n_nodes_out nodes, room for
// 1 + the total phrase length), feeds `tokens` through forward_one_step from the root (step_score_out / state_out [n_tokens]) and
// reports finalize's score of the last state.  Tokens are only required to be >= 0 here: there is no vocabulary.
int rnnt_context_walk_host(int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score, int32_t n_tokens,
                           const int32_t* tokens, double* step_score_out, int32_t* state_out, double* finalize_out) {
    CtxGraph g;
    std::string err;
    const int rc = ctx_graph_build(n_phrases, phrase_lens, phrase_tokens, context_score, -1, -1, g, err);
    if (rc) return rc;
    if (n_tokens < 0 || (n_tokens > 0 && !tokens)) return RNNT_ERR_ARG;
    int state = 0;
    for (int i = 0; i < n_tokens; ++i) {
        int nx;
        const double sc = ctx_graph_step(g, state, tokens[i], &nx);
        if (step_score_out) step_score_out[i] = sc;
        if (state_out) state_out[i] = nx;
        state = nx;
    }
    if (finalize_out) *finalize_out = -g.nscore[state];
    return RNNT_OK;
}

int rnnt_context_dump_host(int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score, int32_t* n_nodes_out,
                           int32_t* token_out, double* node_score_out, double* output_score_out, int32_t* is_end_out, int32_t* fail_out,
                           int32_t* output_out) {
    CtxGraph g;
    std::string err;
    const int rc = ctx_graph_build(n_phrases, phrase_lens, phrase_tokens, context_score, -1, -1, g, err);
    if (rc) return rc;
    if (!n_nodes_out) return RNNT_ERR_ARG;
    const size_t n = g.token.size();
    *n_nodes_out = (int)n;
    if (token_out) std::copy(g.token.begin(), g.token.end(), token_out);
    if (node_score_out) std::copy(g.nscore.begin(), g.nscore.end(), node_score_out);
    if (output_score_out) std::copy(g.oscore.begin(), g.oscore.end(), output_score_out);
    if (is_end_out) std::copy(g.is_end.begin(), g.is_end.end(), is_end_out);
    if (fail_out) std::copy(g.fail.begin(), g.fail.end(), fail_out);
    if (output_out) std::copy(g.output.begin(), g.output.end(), output_out);
    return RNNT_OK;
}

// The search as a pure C++ function (no context, no GPU): lp_host [B, T, vocab]; the graph as phrases (n_phrases == 0: none).  Same
// results and layout as rnnt_ctc_prefix_beam_logprobs; the device path is compared against it.
int rnnt_ctc_prefix_beam_host(const float* lp_host, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t vocab, int32_t blank,
                              int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score,
                              int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host, int32_t* times_host,
                              double* scores_host, double* ctx_scores_host) {
    return rnnt_ctc_prefix_beam_ngram_host(lp_host, enc_lens_host, B, T, vocab, blank, beam_size, n_phrases, phrase_lens, phrase_tokens, context_score, 0,
                                           nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, 0.0, cap_tokens, n_hyp_host, lens_host, tokens_host, times_host,
                                           scores_host, ctx_scores_host, nullptr);
}

// The same with an n-gram model fused (the list as rnnt_ngram_set takes it; n_ngrams == 0: none) and its scores ngram_scores_host
// [B, beam_size] (may be NULL).
int rnnt_ctc_prefix_beam_ngram_host(const float* lp_host, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t vocab, int32_t blank,
                                    int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score,
                                    int32_t n_ngrams, const int32_t* ngram_lens, const int32_t* ngram_tokens, const double* logp, const double* bow,
                                    double lm_weight, double length_bonus, double unk_logp, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                    int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host, double* ngram_scores_host) {
    int fmax, rc;
    if ((rc = ctc_prefix_check(nullptr, "rnnt_ctc_prefix_beam_host", lp_host, enc_lens_host, B, T, vocab, beam_size, cap_tokens, n_hyp_host, lens_host,
                               tokens_host, times_host, scores_host, &fmax)))
        return rc;
    CtxGraph g;
    std::string err;
    if (n_phrases && (rc = ctx_graph_build(n_phrases, phrase_lens, phrase_tokens, context_score, vocab, blank, g, err))) return rc;
    NgModel ng;
    if (n_ngrams && (rc = ngram_build(n_ngrams, ngram_lens, ngram_tokens, logp, bow, lm_weight, length_bonus, unk_logp, vocab, blank, ng, err))) return rc;
    const size_t R = (size_t)B * beam_size;
    std::fill(lens_host, lens_host + R, 0);
    std::fill(tokens_host, tokens_host + R * cap_tokens, 0);
    std::fill(times_host, times_host + R * cap_tokens, 0);
    std::fill(scores_host, scores_host + R, 0.0);
    if (ctx_scores_host) std::fill(ctx_scores_host, ctx_scores_host + R, 0.0);
    if (ngram_scores_host) std::fill(ngram_scores_host, ngram_scores_host + R, 0.0);
    for (int b = 0; b < B; ++b) {
        std::vector<CpHyp> hyps;
        ctc_prefix_search_host(lp_host + (size_t)b * T * vocab, enc_lens_host[b], vocab, blank, beam_size, n_phrases ? &g : nullptr, n_ngrams ? &ng : nullptr,
                               hyps);
        n_hyp_host[b] = (int)hyps.size();
        for (size_t a = 0; a < hyps.size(); ++a) {
            const size_t r = (size_t)b * beam_size + a;
            lens_host[r] = (int)hyps[a].prefix.size();
            std::copy(hyps[a].prefix.begin(), hyps[a].prefix.end(), tokens_host + r * cap_tokens);
            const std::vector<int>& tm = hyps[a].times();
            std::copy(tm.begin(), tm.end(), times_host + r * cap_tokens);
            scores_host[r] = hyps[a].total_score();
            if (ctx_scores_host) ctx_scores_host[r] = hyps[a].context_score;
            if (ngram_scores_host) ngram_scores_host[r] = hyps[a].ngram_score;
        }
    }
    return RNNT_OK;
}

// ctc_prefix_beam_search over log-probabilities lp_dev [B, T, vocab] already on the device: one upload (the lengths), ONE launch of
// ctc_prefix_search (one workgroup per utterance, frame loop inside, results packed by its epilogue), one download, one
// synchronisation.  Any context; weights are not needed.  Touches only its own buffers.
int rnnt_ctc_prefix_beam_logprobs(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                  int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host,
                                  int32_t* times_host, double* scores_host, double* ctx_scores_host, void* stream) {
    return rnnt_ctc_prefix_beam_logprobs_ngram(ctx, lp_dev, enc_lens_host, B, T, beam_size, use_context, 0, cap_tokens, n_hyp_host, lens_host, tokens_host,
                                               times_host, scores_host, ctx_scores_host, nullptr, stream);
}

// The same with the model of rnnt_ngram_set fused when use_ngram (ctc_prefix_search<true>); ngram_scores_host [B, beam_size] or NULL.
int rnnt_ctc_prefix_beam_logprobs_ngram(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                        int32_t use_context, int32_t use_ngram, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                        int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host,
                                        double* ngram_scores_host, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    const int V = ctx->cfg.vocab_size;
    int fmax, rc;
    if ((rc = ctc_prefix_check(ctx, "rnnt_ctc_prefix_beam_logprobs", lp_dev, enc_lens_host, B, T, V, beam_size, cap_tokens, n_hyp_host, lens_host,
                               tokens_host, times_host, scores_host, &fmax)))
        return rc;
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_prefix_beam_logprobs: use_context without a context graph (rnnt_context_set)");
    if (use_ngram && !ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_prefix_beam_logprobs: use_ngram without an n-gram model (rnnt_ngram_set)");
    const size_t nd = use_ngram ? 3 : 2;                              // scores | context scores | n-gram scores
    const size_t R = (size_t)B * beam_size, lcap = std::max(fmax, 1), astride = (size_t)T * beam_size + 1;
    if ((size_t)B * T * V >= ((size_t)1 << 40) || (size_t)B * astride >= ((size_t)1 << 30) || R * lcap >= ((size_t)1 << 30))
        return fail(ctx, RNNT_ERR_SHAPE, "rnnt_ctc_prefix_beam_logprobs: B=%d T=%d beam=%d too large for one call", B, T, beam_size);
    hipStream_t s = (hipStream_t)stream;
    // ints: lengths [B] | prefix arena [B][astride] int2 | time arena likewise | the downloaded block (cp_out)
    CtcPrefixP p;
    memset(&p, 0, sizeof(p));
    int* d_lens;
    CpOut o;
    Carve<int> i;
    auto lay = [&] {
        d_lens = i.take((size_t)B + (B & 1));                         // keeps the int2 arenas 8-byte aligned
        p.parena = reinterpret_cast<int2*>(i.take(2 * (size_t)B * astride));
        p.tarena = reinterpret_cast<int2*>(i.take(2 * (size_t)B * astride));
        o = cp_out(i, B, R, lcap);
    };
    lay();   // sizes
    if ((rc = reserve(ctx, ctx->cp_i, i.off))) return rc;
    if ((rc = reserve(ctx, ctx->cp_d, nd * R))) return rc;
    i = {ctx->cp_i};
    lay();   // pointers
    p.o.nh = o.nh; p.o.len = o.len; p.o.tok = o.tok; p.o.time = o.time;
    p.o.sc = ctx->cp_d; p.o.cs = ctx->cp_d + R;
    p.lp = lp_dev; p.lens = d_lens; p.T = T; p.V = V; p.blank = ctx->cfg.blank_id; p.beam = beam_size; p.lcap = (int)lcap;
    if (use_context) p.g = ctx_graph_dev(ctx);
    if (use_ngram) { p.ng = ngram_dev(ctx); p.o.ls = ctx->cp_d + 2 * R; }
    HIPCHK(hipMemcpyAsync(d_lens, enc_lens_host, B * sizeof(int), hipMemcpyHostToDevice, s));            // the upload
    {
        ProfScope prof(ctx, s, TAG_CTC_PREFIX);
        if (use_ngram) hipLaunchKernelGGL(ctc_prefix_search<true>, dim3(B), dim3(CP_NT), 0, s, p);
        else hipLaunchKernelGGL(ctc_prefix_search<false>, dim3(B), dim3(CP_NT), 0, s, p);
        LAUNCHCHK("ctc_prefix_search");
    }
    std::vector<int> oi(o.total);
    std::vector<double> od(nd * R);
    HIPCHK(hipMemcpyAsync(oi.data(), o.nh, o.total * sizeof(int), hipMemcpyDeviceToHost, s));            // the download (two blocks)
    HIPCHK(hipMemcpyAsync(od.data(), ctx->cp_d, nd * R * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    Carve<int> hc{oi.data()};
    const CpOut h = cp_out(hc, B, R, lcap);
    cp_out_copy(h, od.data(), B, R, lcap, R, (size_t)cap_tokens, n_hyp_host, lens_host, tokens_host, times_host, scores_host, ctx_scores_host,
                use_ngram ? ngram_scores_host : nullptr);
    if (!use_ngram && ngram_scores_host) std::fill(ngram_scores_host, ngram_scores_host + R, 0.0);
    return RNNT_OK;
}

// rnnt_ctc_logprobs over the B*T frames of enc_dev [B, T, 256], then the search above.
int rnnt_ctc_prefix_beam_decode(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host,
                                int32_t* times_host, double* scores_host, double* ctx_scores_host, void* stream) {
    return rnnt_ctc_prefix_beam_decode_ngram(ctx, enc_dev, enc_lens_host, B, T, beam_size, use_context, 0, cap_tokens, n_hyp_host, lens_host, tokens_host,
                                             times_host, scores_host, ctx_scores_host, nullptr, stream);
}

int rnnt_ctc_prefix_beam_decode_ngram(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                      int32_t use_context, int32_t use_ngram, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                      int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host,
                                      double* ngram_scores_host, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    int fmax, rc;
    if ((rc = ctc_prefix_check(ctx, "rnnt_ctc_prefix_beam_decode", enc_dev, enc_lens_host, B, T, ctx->cfg.vocab_size, beam_size, cap_tokens, n_hyp_host,
                               lens_host, tokens_host, times_host, scores_host, &fmax)))
        return rc;
    if (use_context && !ctx->cg_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_prefix_beam_decode: use_context without a context graph (rnnt_context_set)");
    if (use_ngram && !ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_prefix_beam_decode: use_ngram without an n-gram model (rnnt_ngram_set)");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_prefix_beam_decode: ctc_head.ctc_lo.* not loaded");
    if ((long long)B * T >= 0x7fffffffLL / 512) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_ctc_prefix_beam_decode: B=%d T=%d frames in one call", B, T);
    if ((rc = reserve(ctx, ctx->cp_lp, std::max<size_t>((size_t)B * T * ctx->cfg.vocab_size, 1)))) return rc;
    if (fmax > 0) {   // the kernel and tile choices of a small call whatever B is: an utterance's sums do not depend on its batch
        GemmCapScope cap(ctx);
        if ((rc = rnnt_ctc_logprobs(ctx, enc_dev, B * T, ctx->cp_lp, stream))) return rc;
    }
    return rnnt_ctc_prefix_beam_logprobs_ngram(ctx, ctx->cp_lp, enc_lens_host, B, T, beam_size, use_context, use_ngram, cap_tokens, n_hyp_host, lens_host,
                                               tokens_host, times_host, scores_host, ctx_scores_host, ngram_scores_host, stream);
}
