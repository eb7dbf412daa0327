// C ABI: the back-off n-gram model the CTC and the transducer prefix beam search fuse (rnnt_ngram_set, rnnt_ngram_walk_host, rnnt_ngram_score).
// Included by rnnt_api.hip inside extern "C".  Tables, step and the scoring kernel: rnnt_ngram.hip.h.  The builder and the walk are
// pure C++ (no context, no GPU).
//
// The model is a list of n-grams (tokens[1..k], logp, bow), k <= 8, natural logs in f64.  Tokens are model ids in [0, vocab) other
// than the blank, BOS = vocab (first position only) and EOS = vocab + 1 (last position only).  Every n-gram's prefix (all but its last
// token) is listed before it, so the list IS a trie in insertion order: n-gram i is node i + 1, the root is node 0.

namespace {
constexpr int NG_MAX_ORDER = 8, NG_MAX_NODES = 1 << 22;

// The tables of the list.  Values are prescaled here, once: each is ONE f64 multiplication followed by ONE f64 addition (never an
// FMA), so the restatement's `lm_weight * logp + length_bonus` gives the same bits.
int ngram_build(int n, const int32_t* lens, const int32_t* tokens, const double* logp, const double* bow, double lm_weight, double length_bonus,
                double unk_logp, int vocab, int blank, NgModel& m, std::string& err) {
#pragma clang fp contract(off)
    m = NgModel();
    if (n < 1 || !lens || !tokens || !logp || !bow) { err = "null or empty n-gram list"; return RNNT_ERR_ARG; }
    if (vocab < 1) { err = "vocabulary " + std::to_string(vocab); return RNNT_ERR_ARG; }
    if (!std::isfinite(lm_weight) || lm_weight < 0.0) { err = "lm_weight is negative or not finite"; return RNNT_ERR_ARG; }
    if (!std::isfinite(length_bonus) || !std::isfinite(unk_logp)) { err = "length_bonus or unk_logp is not finite"; return RNNT_ERR_ARG; }
    if ((long long)n + 1 > NG_MAX_NODES) { err = "more than " + std::to_string(NG_MAX_NODES) + " nodes"; return RNNT_ERR_ARG; }
    const int BOS = vocab, EOS = vocab + 1, N = n + 1;
    std::unordered_map<unsigned long long, int> kids;                // (node, token) -> child
    kids.reserve((size_t)n * 2);
    auto key = [&](int node, int tok) { return (unsigned long long)node * (unsigned)(vocab + 2) + (unsigned)tok; };
    auto child = [&](int node, int tok) {
        const auto it = kids.find(key(node, tok));
        return it == kids.end() ? -1 : it->second;
    };
    std::vector<int> parent(N, 0), last(N, -1), depth(N, 0);
    m.W.assign(N, 0.0); m.B.assign(N, 0.0);
    size_t at = 0;
    for (int g = 0; g < n; ++g) {
        const int k = lens[g], c = g + 1;
        const std::string who = "n-gram " + std::to_string(g);
        if (k < 1 || k > NG_MAX_ORDER) { err = who + ": " + std::to_string(k) + " tokens, outside [1, " + std::to_string(NG_MAX_ORDER) + "]"; return RNNT_ERR_ARG; }
        const int32_t* tk = tokens + at;
        for (int i = 0; i < k; ++i) {
            if (tk[i] < 0 || tk[i] >= vocab + 2) { err = who + ": token " + std::to_string(tk[i]) + " outside the vocabulary"; return RNNT_ERR_ARG; }
            if (tk[i] == blank) { err = who + " holds the blank"; return RNNT_ERR_ARG; }
            if (tk[i] == BOS && i != 0) { err = who + ": BOS is not first"; return RNNT_ERR_ARG; }
            if (tk[i] == EOS && i != k - 1) { err = who + ": EOS is not last"; return RNNT_ERR_ARG; }
        }
        if (!std::isfinite(logp[g]) || !std::isfinite(bow[g])) { err = who + ": value not finite"; return RNNT_ERR_ARG; }
        int node = 0;
        for (int i = 0; i + 1 < k && node >= 0; ++i) node = child(node, tk[i]);
        if (node < 0) { err = who + ": its prefix is not listed earlier"; return RNNT_ERR_ARG; }
        if (child(node, tk[k - 1]) >= 0) { err = who + " is listed twice"; return RNNT_ERR_ARG; }
        kids[key(node, tk[k - 1])] = c;
        parent[c] = node; last[c] = tk[k - 1]; depth[c] = k;
        const double w = lm_weight * logp[g];
        m.W[c] = tk[k - 1] == EOS ? w : w + length_bonus;
        m.B[c] = lm_weight * bow[g];
        if (tk[k - 1] == EOS) m.eos = EOS;
        at += (size_t)k;
    }
    const double u = lm_weight * unk_logp;
    m.U = u + length_bonus;
    // fail arcs: the longest proper suffix of the node's n-gram that is a node
    m.fail.assign(N, 0);
    for (int c = 1; c < N; ++c) {
        int s[NG_MAX_ORDER];
        const int k = depth[c];
        for (int v = c, i = k - 1; i >= 0; --i) { s[i] = last[v]; v = parent[v]; }
        for (int i = 1; i < k; ++i) {
            int node = 0;
            for (int q = i; q < k && node >= 0; ++q) node = child(node, s[q]);
            if (node >= 0) { m.fail[c] = node; break; }
        }
    }
    // children as a CSR sorted by token per node, and the root's dense row
    std::vector<int> cnt(N + 1, 0);
    for (int c = 1; c < N; ++c) ++cnt[parent[c] + 1];
    m.off.assign(N + 1, 0);
    for (int v = 0; v < N; ++v) m.off[v + 1] = m.off[v] + cnt[v + 1];
    m.ctok.assign(n, 0); m.cid.assign(n, 0);
    std::vector<int> fill(m.off.begin(), m.off.end() - 1);
    std::vector<std::pair<int, int>> row;
    for (int c = 1; c < N; ++c) { const int q = fill[parent[c]]++; m.ctok[q] = last[c]; m.cid[q] = c; }
    for (int v = 0; v < N; ++v) {
        row.clear();
        for (int q = m.off[v]; q < m.off[v + 1]; ++q) row.push_back({m.ctok[q], m.cid[q]});
        std::sort(row.begin(), row.end());
        for (int q = m.off[v]; q < m.off[v + 1]; ++q) { m.ctok[q] = row[q - m.off[v]].first; m.cid[q] = row[q - m.off[v]].second; }
    }
    m.root.assign(vocab + 2, -1);
    for (int q = m.off[0]; q < m.off[1]; ++q) m.root[m.ctok[q]] = m.cid[q];
    m.start = m.root[BOS] >= 0 ? m.root[BOS] : 0;
    return RNNT_OK;
}

// a token the walk and the scoring kernel may step over: a model id other than the blank (the root row has vocab + 2 entries)
bool ngram_token_ok(int tok, int vocab, int blank) { return tok >= 0 && tok < vocab && tok != blank; }
}  // namespace

// The model for the searches with use_ngram and for rnnt_ngram_score; n_ngrams == 0 clears it.  Starts a new model generation.
int rnnt_ngram_set(rnnt_ctx* ctx, int32_t n_ngrams, const int32_t* lens_host, const int32_t* tokens_host, const double* logp_host, const double* bow_host,
                   double lm_weight, double length_bonus, double unk_logp) {
    if (!ctx) return RNNT_ERR_ARG;
    if (n_ngrams == 0) {
        ctx->ng_on = false;
        ctx->ng = NgModel();
        ++ctx->ng_gen;
        return RNNT_OK;
    }
    NgModel m;
    std::string err;
    int rc = ngram_build(n_ngrams, lens_host, tokens_host, logp_host, bow_host, lm_weight, length_bonus, unk_logp, ctx->cfg.vocab_size, ctx->cfg.blank_id, m, err);
    if (rc) return fail(ctx, rc, "rnnt_ngram_set: %s", err.c_str());
    const size_t n = m.fail.size(), k = m.ctok.size();
    if ((rc = reserve(ctx, ctx->ng_i, 2 * n + 1 + 2 * k + m.root.size()))) return rc;
    if ((rc = reserve(ctx, ctx->ng_d, 2 * n))) return rc;
    HIPCHK(hipDeviceSynchronize());                                  // a search still reading the previous tables
    std::vector<int> hi;
    hi.insert(hi.end(), m.fail.begin(), m.fail.end());
    hi.insert(hi.end(), m.off.begin(), m.off.end());
    hi.insert(hi.end(), m.ctok.begin(), m.ctok.end());
    hi.insert(hi.end(), m.cid.begin(), m.cid.end());
    hi.insert(hi.end(), m.root.begin(), m.root.end());
    std::vector<double> hd;
    hd.insert(hd.end(), m.W.begin(), m.W.end());
    hd.insert(hd.end(), m.B.begin(), m.B.end());
    HIPCHK(hipMemcpy(ctx->ng_i, hi.data(), hi.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->ng_d, hd.data(), hd.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->ng = std::move(m);
    ctx->ng_on = true;
    ++ctx->ng_gen;                                                   // a pool search fused with the previous model holds its node ids (api_pool_ctc.hip.inc, api_pool_prefix.hip.inc)
    return RNNT_OK;
}

// Test seam (no context, no GPU): builds the model and feeds `tokens` through the step from the start state.  step_score_out /
// state_out [n_tokens] (each may be NULL), *eos_out the end term of the last state, *n_nodes_out the nodes (root included).
int rnnt_ngram_walk_host(int32_t n_ngrams, const int32_t* lens, const int32_t* ngram_tokens, const double* logp, const double* bow, double lm_weight,
                         double length_bonus, double unk_logp, int32_t vocab, int32_t blank, int32_t n_tokens, const int32_t* tokens,
                         double* step_score_out, int32_t* state_out, double* eos_out, int32_t* n_nodes_out) {
    NgModel m;
    std::string err;
    const int rc = ngram_build(n_ngrams, lens, ngram_tokens, logp, bow, lm_weight, length_bonus, unk_logp, vocab, blank, m, err);
    if (rc) return rc;
    if (n_tokens < 0 || (n_tokens > 0 && !tokens)) return RNNT_ERR_ARG;
    for (int i = 0; i < n_tokens; ++i)
        if (!ngram_token_ok(tokens[i], vocab, blank)) return RNNT_ERR_ARG;
    const NgTables g = m.tables();
    int state = g.start;
    for (int i = 0; i < n_tokens; ++i) {
        int nx;
        const double sc = ng_step(g, state, tokens[i], &nx);
        if (step_score_out) step_score_out[i] = sc;
        if (state_out) state_out[i] = nx;
        state = nx;
    }
    if (eos_out) *eos_out = ng_eos(g, state);
    if (n_nodes_out) *n_nodes_out = (int)m.fail.size();
    return RNNT_OK;
}

// n token sequences (tokens_host [n, cap], lens_host [n] in [0, cap]) scored by the model that is set, each from the start state:
// one upload, ONE launch of ngram_score_rows (one sequence per thread), one download, one synchronisation.  step_scores_host
// [n, cap] (may be NULL; zero beyond a length), totals_host [n] the sum in walk order, plus the end term when with_eos.
int rnnt_ngram_score(rnnt_ctx* ctx, int32_t n, const int32_t* lens_host, const int32_t* tokens_host, int32_t cap, int32_t with_eos,
                     double* step_scores_host, double* totals_host, void* stream) {
    const char* fn = "rnnt_ngram_score";
    if (!ctx) return RNNT_ERR_ARG;
    if (!lens_host || !tokens_host || !totals_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (n < 1 || cap < 1 || (size_t)n * cap >= ((size_t)1 << 30)) return fail(ctx, RNNT_ERR_ARG, "%s: n=%d cap=%d", fn, n, cap);
    if (!ctx->ng_on) return fail(ctx, RNNT_ERR_STATE, "%s: no n-gram model (rnnt_ngram_set)", fn);
    for (int i = 0; i < n; ++i) {
        if (lens_host[i] < 0 || lens_host[i] > cap) return fail(ctx, RNNT_ERR_ARG, "%s: sequence %d has %d tokens, outside [0, %d]", fn, i, lens_host[i], cap);
        for (int q = 0; q < lens_host[i]; ++q)
            if (!ngram_token_ok(tokens_host[(size_t)i * cap + q], ctx->cfg.vocab_size, ctx->cfg.blank_id))
                return fail(ctx, RNNT_ERR_ARG, "%s: sequence %d: token %d outside the vocabulary or the blank", fn, i, tokens_host[(size_t)i * cap + q]);
    }
    const size_t nt = (size_t)n * cap;
    int rc;
    if ((rc = reserve(ctx, ctx->ngs_i, n + nt))) return rc;
    if ((rc = reserve(ctx, ctx->ngs_d, nt + n))) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(ctx->ngs_i, lens_host, n * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->ngs_i + n, tokens_host, nt * sizeof(int), hipMemcpyHostToDevice, s));
    NgScoreP p;
    memset(&p, 0, sizeof(p));
    p.g = ngram_dev(ctx);
    p.lens = ctx->ngs_i; p.tokens = ctx->ngs_i + n; p.step = ctx->ngs_d; p.total = ctx->ngs_d + nt; p.n = n; p.cap = cap; p.with_eos = with_eos != 0;
    hipLaunchKernelGGL(ngram_score_rows, dim3((n + 63) / 64), dim3(64), 0, s, p);
    LAUNCHCHK("ngram_score_rows");
    std::vector<double> od(nt + n);
    HIPCHK(hipMemcpyAsync(od.data(), ctx->ngs_d, (nt + n) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (step_scores_host) memcpy(step_scores_host, od.data(), nt * sizeof(double));
    memcpy(totals_host, od.data() + nt, n * sizeof(double));
    return RNNT_OK;
}
