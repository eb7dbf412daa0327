// C ABI: beam search (device extension chains, C++ merge, library-side hypotheses).  Included by rnnt_api.hip inside extern "C".

int rnnt_beam_frame(rnnt_ctx* ctx, int32_t frame_idx, int32_t n_rows, const int32_t* row_stream_host, const int32_t* row_tok_host,
                    int32_t beam_k, int32_t* steps_host, float* blank_lp_host, float* top_lp_host, int32_t* top_tok_host, void* stream) {
    if (!ctx || !row_stream_host || !row_tok_host || !steps_host || !blank_lp_host || !top_lp_host || !top_tok_host)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_frame: null argument");
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_frame: no weights / no streams");
    if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_frame: context created with max_beam = 0");
    if (n_rows < 1 || n_rows > ctx->max_rows || beam_k < 1 || beam_k > ctx->cfg.max_beam || beam_k > ctx->cfg.vocab_size - 1)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_frame: n_rows=%d beam_k=%d out of range", n_rows, beam_k);
    if (frame_idx < 0 || frame_idx >= ctx->frames_buffered) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_frame: frame %d not buffered", frame_idx);
    hipStream_t s = (hipStream_t)stream;
    const int V = ctx->cfg.vocab_size, NS = ctx->cfg.n_steps, slots = NS + 1, R = n_rows;
    std::vector<int> fr(R);
    for (int r = 0; r < R; ++r) {
        if (row_stream_host[r] < 0 || row_stream_host[r] >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_frame: bad stream index");
        fr[r] = row_stream_host[r] * ctx->fstride + frame_idx;   // row of the projected-encoder-frame table
    }
    HIPCHK(hipMemcpyAsync(ctx->b_frame, fr.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_tok, row_tok_host, R * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(256), 0, s, ctx->b_active, 1, (long long)R);
    LAUNCHCHK("fill_i32");
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(64), 0, s, ctx->n_active + 1, R, 1LL);
    LAUNCHCHK("fill_i32");
    HIPCHK(hipMemsetAsync(ctx->b_steps, 0, R * sizeof(int), s));
    float* pool = ctx->pool[ctx->pool_cur];
    BeamOut bo{ctx->b_active, ctx->b_tok, ctx->b_steps, ctx->b_blank, ctx->b_toplp, ctx->b_toptok, ctx->n_active + 1};
    int rc;
    if (ctx->use_beam_chain && V <= 512) {   // one resident workgroup per row runs its whole extension chain
        BeamChainP c;
        memset(&c, 0, sizeof(c));
        dec_weights(ctx, c); c.encp = ctx->encp; c.pool = pool; c.frame = ctx->b_frame; c.tok_in = ctx->b_tok;
        c.steps = ctx->b_steps; c.blank_lp = ctx->b_blank; c.top_lp = ctx->b_toplp; c.top_tok = ctx->b_toptok;
        c.vocab = V; c.blank = ctx->cfg.blank_id; c.k = beam_k; c.n_steps = NS; c.slots = slots;
        hipLaunchKernelGGL(beam_chain, dim3(R), dim3(512), 0, s, c);
        LAUNCHCHK("beam_chain");
        ctx->launches += 1;
    } else
    for (int st = 0; st < NS; ++st) {
        float* sin = pool + (size_t)st * 512;
        float* sout = pool + (size_t)(st + 1) * 512;
        GemmP g1 = plain_gemm(sin, slots * 512, ctx->whh_il, D, nullptr, sout, D, R, 4 * D, D, EPI_LSTM);
        g1.X = ctx->egate; g1.I = ctx->b_tok; g1.X2 = sin + D; g1.Y2 = sout + D; g1.lstm_ld = slots * 512;
        if ((rc = launch_gemm(ctx, s, &g1, 1, TAG_LSTM))) return rc;
        GemmP g2 = plain_gemm(sout, slots * 512, ctx->wpr, D, ctx->bpr, ctx->bpred, D, R, D, D);
        if ((rc = launch_gemm(ctx, s, &g2, 1, TAG_PRED_PROJ))) return rc;
        GemmP g3 = plain_gemm(ctx->bpred, D, ctx->wpf, D, ctx->bpf, ctx->bz, D, R, D, D, EPI_TANH_ADD);
        g3.X = ctx->encp; g3.I = ctx->b_frame; g3.x_n = 1; g3.x_s0 = 0; g3.x_s1 = D;
        if ((rc = launch_gemm(ctx, s, &g3, 1, TAG_JOINT_TANH))) return rc;
        GemmP g4 = plain_gemm(ctx->bz, D, ctx->wout, D, ctx->bout, ctx->blogits, ctx->vpad, R, V, D);
        if ((rc = launch_gemm(ctx, s, &g4, 1, TAG_JOINT_OUT))) return rc;
        hipLaunchKernelGGL(beam_reduce, dim3(R), dim3(64), 0, s, ctx->blogits, ctx->vpad, V, ctx->cfg.blank_id, beam_k, st, NS, bo);
        LAUNCHCHK("beam_reduce");
        HIPCHK(hipMemcpyAsync(ctx->pinned + 1, ctx->n_active + 1, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (ctx->pinned[1] <= 0) break;
    }
    HIPCHK(hipMemcpyAsync(steps_host, ctx->b_steps, R * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(blank_lp_host, ctx->b_blank, (size_t)R * NS * sizeof(float), hipMemcpyDeviceToHost, s));
    // device layout of the top-k arrays is [R][NS][beam_k] with THIS call's beam_k
    HIPCHK(hipMemcpyAsync(top_lp_host, ctx->b_toplp, (size_t)R * NS * beam_k * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(top_tok_host, ctx->b_toptok, (size_t)R * NS * beam_k * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_beam_select(rnnt_ctx* ctx, int32_t n_new, const int32_t* src_row_host, const int32_t* src_step_host, void* stream) {
    if (!ctx || !src_row_host || !src_step_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_select: null argument");
    if (ctx->max_rows == 0 || n_new < 1 || n_new > ctx->max_rows) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_select: n_new out of range");
    hipStream_t s = (hipStream_t)stream;
    const int slots = ctx->cfg.n_steps + 1;
    for (int r = 0; r < n_new; ++r)
        if (src_row_host[r] < 0 || src_row_host[r] >= ctx->max_rows || src_step_host[r] < 0 || src_step_host[r] >= slots)
            return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_select: bad source slot");
    HIPCHK(hipMemcpyAsync(ctx->b_srcrow, src_row_host, n_new * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_srcstep, src_step_host, n_new * sizeof(int), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(beam_gather, dim3(n_new), dim3(128), 0, s, ctx->pool[ctx->pool_cur], ctx->pool[ctx->pool_cur ^ 1], ctx->b_srcrow, ctx->b_srcstep,
                       n_new, slots);
    LAUNCHCHK("beam_gather");
    HIPCHK(hipStreamSynchronize(s));   // the host arrays may be reused by the caller
    ctx->pool_cur ^= 1;
    return RNNT_OK;
}

// Host half of one encoder frame of _decode_chunk_beam_search (model/online_rnnt_model.py:419-518) for ONE stream, pure
// host code (also exported for CPU tests): candidates in the reference's order (per hypothesis, per evaluation: the blank
// candidate keeping the old state, then the top-k non-blank), scores accumulated in double exactly as Python floats
// (float32 log-prob widened, then added), stable descending sort (:506), first-wins de-duplication on the token
// sequence (:508-516), truncation to the beam.  src_row / src_step name the pooled LSTM state each survivor keeps.
namespace {
struct BeamCand { std::vector<int> tokens; double score; int row, step; };
void beam_merge_stream(const std::vector<rnnt_ctx::Hyp>& beam, int row0, const int* steps, const float* blank_lp, const float* top_lp,
                       const int* top_tok, int n_steps, int k, int beam_size, std::vector<rnnt_ctx::Hyp>& out, std::vector<int>& src_row,
                       std::vector<int>& src_step) {
    std::vector<BeamCand> cands;
    int r = row0;
    for (const rnnt_ctx::Hyp& h : beam) {
        std::vector<int> toks = h.tokens;
        double lp = h.log_prob;
        const int n = steps[r];
        for (int st = 0; st < n; ++st) {
            cands.push_back({toks, lp + (double)blank_lp[(size_t)r * n_steps + st], r, st});
            for (int j = 0; j < k; ++j) {
                BeamCand c{toks, lp + (double)top_lp[((size_t)r * n_steps + st) * k + j], r, st + 1};
                c.tokens.push_back(top_tok[((size_t)r * n_steps + st) * k + j]);
                cands.push_back(std::move(c));
            }
            if (st < n - 1) {   // chain continued with the best non-blank (:489-499)
                toks.push_back(top_tok[((size_t)r * n_steps + st) * k]);
                lp += (double)top_lp[((size_t)r * n_steps + st) * k];
            }
        }
        ++r;
    }
    std::stable_sort(cands.begin(), cands.end(), [](const BeamCand& a, const BeamCand& b) { return a.score > b.score; });
    out.clear();
    for (BeamCand& c : cands) {
        bool dup = false;
        for (const rnnt_ctx::Hyp& u : out)
            if (u.tokens == c.tokens) { dup = true; break; }
        if (dup) continue;
        out.push_back(rnnt_ctx::Hyp{std::move(c.tokens), c.score});
        src_row.push_back(c.row);
        src_step.push_back(c.step);
        if ((int)out.size() >= beam_size) break;
    }
}
}  // namespace

// Pure-host export of beam_merge_stream for one stream (CPU tests; no context, no GPU).  Hypotheses are passed flat:
// hyp_len[n_hyp], hyp_tokens (concatenated), hyp_score[n_hyp]; outputs likewise (out_tokens needs room for
// beam_size * (longest input + n_steps) ints).  Returns the number of surviving hypotheses.
int rnnt_beam_merge_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score, const int32_t* steps,
                         const float* blank_lp, const float* top_lp, const int32_t* top_tok, int32_t n_steps, int32_t k, int32_t beam_size,
                         int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_step) {
    if (n_hyp < 1 || !hyp_len || !hyp_score || !steps || !blank_lp || !top_lp || !top_tok || !out_len || !out_tokens || !out_score) return RNNT_ERR_ARG;
    std::vector<rnnt_ctx::Hyp> beam(n_hyp), out;
    size_t off = 0;
    for (int i = 0; i < n_hyp; ++i) {
        beam[i].tokens.assign(hyp_tokens + off, hyp_tokens + off + hyp_len[i]);
        beam[i].log_prob = hyp_score[i];
        off += hyp_len[i];
    }
    std::vector<int> sr, ss;
    beam_merge_stream(beam, 0, steps, blank_lp, top_lp, top_tok, n_steps, k, beam_size, out, sr, ss);
    off = 0;
    for (size_t i = 0; i < out.size(); ++i) {
        out_len[i] = (int)out[i].tokens.size();
        for (int t : out[i].tokens) out_tokens[off++] = t;
        out_score[i] = out[i].log_prob;
        if (out_src_row) out_src_row[i] = sr[i];
        if (out_src_step) out_src_step[i] = ss[i];
    }
    return (int)out.size();
}

// Beam search over the buffered encoder frames [frame_begin, frame_end) of every stream with the bookkeeping inside the
// library (the reference's per-frame loop, online_rnnt_model.py:419-518, for all streams at once): per frame one
// beam_chain launch, one copy of the candidates to the host, the merge above, one state-pool gather.
int rnnt_beam_advance(rnnt_ctx* ctx, int32_t frame_begin, int32_t frame_end, int32_t beam_size, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_advance: no weights / no streams");
    if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_advance: context created with max_beam = 0");
    if (beam_size < 1 || beam_size > ctx->cfg.max_beam) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_advance: beam_size %d outside [1, max_beam %d]", beam_size, ctx->cfg.max_beam);
    if (frame_begin < 0 || frame_end > ctx->frames_buffered || frame_begin > frame_end) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_advance: frames [%d, %d) not buffered", frame_begin, frame_end);
    if ((int)ctx->beams.size() != ctx->n_streams) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_advance: call rnnt_streams_reset first");
    const int NS = ctx->cfg.n_steps, B = ctx->n_streams;
    const int k = beam_size < ctx->cfg.vocab_size - 1 ? beam_size : ctx->cfg.vocab_size - 1;          // :467
    std::vector<int> row_stream, row_tok, steps, top_tok, src_row, src_step;
    std::vector<float> blank_lp, top_lp;
    std::vector<rnnt_ctx::Hyp> next;
    int rc;
    for (int f = frame_begin; f < frame_end; ++f) {
        row_stream.clear(); row_tok.clear();
        for (int b = 0; b < B; ++b)
            for (const rnnt_ctx::Hyp& h : ctx->beams[b]) {
                row_stream.push_back(b);
                row_tok.push_back(h.tokens.empty() ? ctx->cfg.blank_id : h.tokens.back());              // :429
            }
        const int R = (int)row_stream.size();
        steps.resize(R); blank_lp.resize((size_t)R * NS); top_lp.resize((size_t)R * NS * k); top_tok.resize((size_t)R * NS * k);
        if ((rc = rnnt_beam_frame(ctx, f, R, row_stream.data(), row_tok.data(), k, steps.data(), blank_lp.data(), top_lp.data(), top_tok.data(), stream)))
            return rc;
        src_row.clear(); src_step.clear();
        int row0 = 0;
        for (int b = 0; b < B; ++b) {
            const int nh = (int)ctx->beams[b].size();
            beam_merge_stream(ctx->beams[b], row0, steps.data(), blank_lp.data(), top_lp.data(), top_tok.data(), NS, k, beam_size, next, src_row, src_step);
            row0 += nh;
            ctx->beams[b].swap(next);
        }
        if ((rc = rnnt_beam_select(ctx, (int)src_row.size(), src_row.data(), src_step.data(), stream))) return rc;
    }
    return RNNT_OK;
}

// hypotheses of one stream after rnnt_beam_advance: count, then tokens / score of hypothesis i (device row = rows of the
// earlier streams + i, the index rnnt_beam_get_states uses)
int rnnt_beam_hyp_count(rnnt_ctx* ctx, int32_t stream_idx, int32_t* n_out) {
    if (!ctx || !n_out || stream_idx < 0 || stream_idx >= (int)ctx->beams.size()) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_hyp_count: bad argument");
    *n_out = (int)ctx->beams[stream_idx].size();
    return RNNT_OK;
}
int rnnt_beam_get_hyp(rnnt_ctx* ctx, int32_t stream_idx, int32_t hyp_idx, int32_t cap, int32_t* tokens_host, int32_t* n_tokens, double* log_prob) {
    if (!ctx || stream_idx < 0 || stream_idx >= (int)ctx->beams.size() || hyp_idx < 0 || hyp_idx >= (int)ctx->beams[stream_idx].size())
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_get_hyp: bad index");
    const rnnt_ctx::Hyp& h = ctx->beams[stream_idx][hyp_idx];
    if (n_tokens) *n_tokens = (int)h.tokens.size();
    if (log_prob) *log_prob = h.log_prob;
    if (tokens_host) {
        if (cap < (int)h.tokens.size()) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_get_hyp: %d tokens, room for %d", (int)h.tokens.size(), cap);
        for (size_t i = 0; i < h.tokens.size(); ++i) tokens_host[i] = h.tokens[i];
    }
    return RNNT_OK;
}

int rnnt_beam_get_states(rnnt_ctx* ctx, int32_t n_rows, float* h_host, float* c_host, void* stream) {
    if (!ctx || !h_host || !c_host || n_rows < 1 || n_rows > ctx->max_rows) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_get_states: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t pitch = (size_t)(ctx->cfg.n_steps + 1) * 512 * sizeof(float);
    const float* pool = ctx->pool[ctx->pool_cur];
    HIPCHK(hipMemcpy2DAsync(h_host, D * sizeof(float), pool, pitch, D * sizeof(float), n_rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpy2DAsync(c_host, D * sizeof(float), pool + D, pitch, D * sizeof(float), n_rows, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_frames_discard(rnnt_ctx* ctx, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    ctx->frames_buffered = 0;
    ctx->frames_decoded = 0;
    HIPCHK(hipMemsetAsync(ctx->fidx, 0, ctx->cfg.max_streams * sizeof(int), s));
    return RNNT_OK;
}

// ---- device-resident beam search (rnnt_beam_decode) ----------------------------------------------------------------------------
namespace {
// per-row lengths / scores / hashes [2][max_rows] and per-stream counts (allocated once), token lists [2][max_rows][lcap] (grown)
int beam_dev_buffers(rnnt_ctx* ctx, size_t lcap) {
    const size_t R = ctx->max_rows, Bm = ctx->cfg.max_streams;
    int rc;
    if ((rc = reserve(ctx, ctx->bd_len, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->bd_sc, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->bd_hs, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->bd_nh, Bm))) return rc;
    if ((rc = reserve(ctx, ctx->bd_fend, Bm))) return rc;
    return reserve(ctx, ctx->bd_tok, 2 * R * lcap);
}

unsigned long long beam_hash(const int* t, size_t n) {
    unsigned long long h = BEAM_HASH0;
    for (size_t i = 0; i < n; ++i) h = beam_hash_step(h, t[i]);
    return h;
}

BeamMergeP beam_merge_params(rnnt_ctx* ctx, int t, size_t lcap, int n_steps, int k, int beam, int width, int f) {
    const size_t R = ctx->max_rows;
    BeamMergeP m;
    memset(&m, 0, sizeof(m));
    m.tk_in = ctx->bd_tok + t * R * lcap; m.tk_out = ctx->bd_tok + (t ^ 1) * R * lcap;
    m.len_in = ctx->bd_len + t * R; m.len_out = ctx->bd_len + (t ^ 1) * R;
    m.sc_in = ctx->bd_sc + t * R; m.sc_out = ctx->bd_sc + (t ^ 1) * R;
    m.hs_in = ctx->bd_hs + t * R; m.hs_out = ctx->bd_hs + (t ^ 1) * R;
    m.nh = ctx->bd_nh; m.fend = ctx->bd_fend;
    m.steps = ctx->b_steps; m.blank_lp = ctx->b_blank; m.top_lp = ctx->b_toplp; m.top_tok = ctx->b_toptok;
    m.tok_next = ctx->b_tok; m.frame_next = ctx->b_frame; m.live = ctx->b_active; m.src_row = ctx->b_srcrow; m.src_step = ctx->b_srcstep;
    m.slots = ctx->cfg.n_steps + 1; m.lcap = (int)lcap; m.n_steps = n_steps; m.k = k; m.beam = beam; m.width = width;
    m.blank = ctx->cfg.blank_id; m.f = f; m.fstride = ctx->fstride;
    return m;
}
}  // namespace

// rnnt_beam_advance with the whole frame loop on the device: per frame one beam_chain launch (fixed-slot rows, dead rows exit at
// once) and one beam_merge_dev launch (candidates, stable order, de-duplication, truncation, state gather, next frame's inputs);
// no host copy and no synchronisation between frames.  Stream b covers frames [frame_begin, frame_end_host[b]).  Supported:
// beam_size <= 16, vocab <= 512, n_steps <= 10, the chain kernel enabled; otherwise RNNT_ERR_ARG / RNNT_ERR_STATE and the caller
// uses rnnt_beam_advance.
int rnnt_beam_decode(rnnt_ctx* ctx, int32_t frame_begin, const int32_t* frame_end_host, int32_t beam_size, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_decode: no weights / no streams");
    if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_decode: context created with max_beam = 0");
    if (!ctx->use_beam_chain) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_decode: RNNT_BEAM_CHAIN=0 (the device merge follows beam_chain only); use rnnt_beam_advance");
    const int V = ctx->cfg.vocab_size, NS = ctx->cfg.n_steps, B = ctx->n_streams;
    if (beam_size < 1 || beam_size > ctx->cfg.max_beam || beam_size > BM_MAX_BEAM)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_decode: beam_size %d outside [1, min(max_beam %d, %d)]", beam_size, ctx->cfg.max_beam, BM_MAX_BEAM);
    if (V > 512 || NS > BM_MAX_STEPS) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_decode: vocab %d > 512 or n_steps %d > %d; use rnnt_beam_advance", V, NS, BM_MAX_STEPS);
    if ((int)ctx->beams.size() != B) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_decode: call rnnt_streams_reset first");
    std::vector<int> fend(B), nh(B);
    int fmax = frame_begin, width = beam_size;
    size_t lmax = 0;
    for (int b = 0; b < B; ++b) {
        fend[b] = frame_end_host ? frame_end_host[b] : ctx->frames_buffered;
        if (frame_begin < 0 || fend[b] < frame_begin || fend[b] > ctx->frames_buffered)
            return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_decode: stream %d: frames [%d, %d) not buffered", b, frame_begin, fend[b]);
        fmax = std::max(fmax, fend[b]);
        nh[b] = (int)ctx->beams[b].size();
        width = std::max(width, nh[b]);
        for (const rnnt_ctx::Hyp& h : ctx->beams[b]) lmax = std::max(lmax, h.tokens.size());
    }
    if (width > BM_MAX_BEAM || (size_t)B * width > (size_t)ctx->max_rows)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_decode: %d hypotheses per stream; use rnnt_beam_advance", width);
    if (fmax == frame_begin) return RNNT_OK;
    hipStream_t s = (hipStream_t)stream;
    const int R = B * width, F = fmax - frame_begin, slots = NS + 1;
    const int k = beam_size < V - 1 ? beam_size : V - 1;                                                // :467
    const size_t lcap = lmax + (size_t)F * NS;   // a hypothesis grows by at most n_steps tokens per frame: no overflow
    if (lcap > (size_t)INT_MAX / 2 || (size_t)R * lcap > ((size_t)1 << 31)) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_beam_decode: token pool too large");
    int rc;
    if ((rc = beam_dev_buffers(ctx, lcap))) return rc;
    // ---- upload: hypotheses into fixed slots (row b * width + i), next-frame inputs, compacted pool rows -> fixed-slot rows -----
    std::vector<int> tok(R, ctx->cfg.blank_id), frame(R, 0), live(R, 0), len(R, 0), srow(R, 0), sstep(R, 0);
    std::vector<double> sc(R, 0.0);
    std::vector<unsigned long long> hs(R, BEAM_HASH0);
    std::vector<int> toks((size_t)R * std::max<size_t>(lmax, 1), 0);
    for (int b = 0, crow = 0; b < B; ++b)
        for (int i = 0; i < nh[b]; ++i, ++crow) {
            const rnnt_ctx::Hyp& h = ctx->beams[b][i];
            const int r = b * width + i;
            tok[r] = h.tokens.empty() ? ctx->cfg.blank_id : h.tokens.back();                                 // :429
            frame[r] = b * ctx->fstride + frame_begin;
            live[r] = frame_begin < fend[b] ? 1 : 0;
            len[r] = (int)h.tokens.size();
            sc[r] = h.log_prob;
            hs[r] = beam_hash(h.tokens.data(), h.tokens.size());
            srow[r] = crow;
            std::copy(h.tokens.begin(), h.tokens.end(), toks.begin() + (size_t)r * lmax);
        }
    const size_t Rm = ctx->max_rows;
    int* tk0 = ctx->bd_tok;
    HIPCHK(hipMemcpyAsync(ctx->b_tok, tok.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_frame, frame.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_active, live.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_srcrow, srow.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_srcstep, sstep.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_len, len.data(), R * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_sc, sc.data(), R * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_hs, hs.data(), R * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_nh, nh.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_fend, fend.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
    if (lmax > 0)
        HIPCHK(hipMemcpy2DAsync(tk0, lcap * sizeof(int), toks.data(), lmax * sizeof(int), lmax * sizeof(int), R, hipMemcpyHostToDevice, s));
    int cur = ctx->pool_cur, t = 0;
    hipLaunchKernelGGL(beam_gather, dim3(R), dim3(128), 0, s, ctx->pool[cur], ctx->pool[cur ^ 1], ctx->b_srcrow, ctx->b_srcstep, R, slots);
    LAUNCHCHK("beam_gather");
    cur ^= 1;
    // ---- frame loop: launches only ----------------------------------------------------------------------------------------------
    BeamChainP c;
    memset(&c, 0, sizeof(c));
    dec_weights(ctx, c); c.encp = ctx->encp; c.frame = ctx->b_frame; c.tok_in = ctx->b_tok; c.live = ctx->b_active;
    c.steps = ctx->b_steps; c.blank_lp = ctx->b_blank; c.top_lp = ctx->b_toplp; c.top_tok = ctx->b_toptok;
    c.vocab = V; c.blank = ctx->cfg.blank_id; c.k = k; c.n_steps = NS; c.slots = slots;
    for (int f = frame_begin; f < fmax; ++f) {
        c.pool = ctx->pool[cur];
        hipLaunchKernelGGL(beam_chain, dim3(R), dim3(512), 0, s, c);
        LAUNCHCHK("beam_chain");
        BeamMergeP m = beam_merge_params(ctx, t, lcap, NS, k, beam_size, width, f);
        m.pool_in = ctx->pool[cur]; m.pool_out = ctx->pool[cur ^ 1];
        hipLaunchKernelGGL(beam_merge_dev, dim3(B), dim3(BM_NT), 0, s, m);
        LAUNCHCHK("beam_merge_dev");
        cur ^= 1; t ^= 1;
    }
    // ---- compaction (rows of stream b after those of streams < b, as rnnt_beam_advance leaves them), one download, one sync -----
    hipLaunchKernelGGL(beam_compact, dim3(R), dim3(128), 0, s, ctx->pool[cur], ctx->pool[cur ^ 1], slots, ctx->bd_tok + t * Rm * lcap,
                       ctx->bd_tok + (t ^ 1) * Rm * lcap, (int)lcap, ctx->bd_len + t * Rm, ctx->bd_len + (t ^ 1) * Rm, ctx->bd_sc + t * Rm,
                       ctx->bd_sc + (t ^ 1) * Rm, ctx->bd_nh, width);
    LAUNCHCHK("beam_compact");
    cur ^= 1; t ^= 1;
    std::vector<int> out_tok((size_t)R * lcap);
    HIPCHK(hipMemcpyAsync(nh.data(), ctx->bd_nh, B * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), ctx->bd_len + t * Rm, R * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sc.data(), ctx->bd_sc + t * Rm, R * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_tok.data(), ctx->bd_tok + t * Rm * lcap, (size_t)R * lcap * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->pool_cur = cur;
    for (int b = 0, crow = 0; b < B; ++b) {
        ctx->beams[b].resize(nh[b]);
        for (int i = 0; i < nh[b]; ++i, ++crow) {
            const int* p = out_tok.data() + (size_t)crow * lcap;
            ctx->beams[b][i].tokens.assign(p, p + len[crow]);
            ctx->beams[b][i].log_prob = sc[crow];
        }
    }
    return RNNT_OK;
}

// One beam_merge_dev launch on flat host inputs for ONE stream (test seam against rnnt_beam_merge_host on adversarial inputs):
// same arguments and results as rnnt_beam_merge_host (src_row = the hypothesis index).  Uses the context's beam scratch only:
// the state pools and the hypotheses of rnnt_beam_advance / rnnt_beam_decode are left alone.  Synchronises.
int rnnt_beam_merge_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                           const int32_t* steps, const float* blank_lp, const float* top_lp, const int32_t* top_tok, int32_t n_steps,
                           int32_t k, int32_t beam_size, int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row,
                           int32_t* out_src_step, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!hyp_len || !hyp_score || !steps || !blank_lp || !top_lp || !top_tok || !out_len || !out_tokens || !out_score)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_merge_device: null argument");
    if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "rnnt_beam_merge_device: context created with max_beam = 0");
    const int width = std::max(n_hyp, beam_size);
    if (n_hyp < 1 || beam_size < 1 || width > BM_MAX_BEAM || width > ctx->max_rows || k < 1 || k > BM_MAX_BEAM || k > ctx->cfg.max_beam ||
        n_steps < 1 || n_steps > BM_MAX_STEPS || n_steps > ctx->cfg.n_steps)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_merge_device: n_hyp %d, beam %d, k %d, n_steps %d outside the supported range", n_hyp, beam_size, k, n_steps);
    size_t lmax = 0, ntok = 0;
    for (int i = 0; i < n_hyp; ++i) {
        if (hyp_len[i] < 0 || steps[i] < 0 || steps[i] > n_steps) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_merge_device: bad hypothesis %d", i);
        lmax = std::max(lmax, (size_t)hyp_len[i]);
        ntok += hyp_len[i];
    }
    if (ntok && !hyp_tokens) return fail(ctx, RNNT_ERR_ARG, "rnnt_beam_merge_device: null argument");
    hipStream_t s = (hipStream_t)stream;
    const size_t lcap = lmax + n_steps, Rm = ctx->max_rows;
    int rc;
    if ((rc = beam_dev_buffers(ctx, lcap))) return rc;
    std::vector<int> toks((size_t)width * lcap, 0), len(width, 0), nh(1, n_hyp), fend(1, 1);
    std::vector<double> sc(width, 0.0);
    std::vector<unsigned long long> hs(width, BEAM_HASH0);
    for (int i = 0, off = 0; i < n_hyp; off += hyp_len[i], ++i) {
        std::copy(hyp_tokens + off, hyp_tokens + off + hyp_len[i], toks.begin() + (size_t)i * lcap);
        len[i] = hyp_len[i];
        sc[i] = hyp_score[i];
        hs[i] = beam_hash(hyp_tokens + off, hyp_len[i]);
    }
    HIPCHK(hipMemcpyAsync(ctx->bd_tok, toks.data(), toks.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_len, len.data(), width * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_sc, sc.data(), width * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_hs, hs.data(), width * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_nh, nh.data(), sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->bd_fend, fend.data(), sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_steps, steps, n_hyp * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_blank, blank_lp, (size_t)n_hyp * n_steps * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_toplp, top_lp, (size_t)n_hyp * n_steps * k * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->b_toptok, top_tok, (size_t)n_hyp * n_steps * k * sizeof(int), hipMemcpyHostToDevice, s));
    BeamMergeP m = beam_merge_params(ctx, 0, lcap, n_steps, k, beam_size, width, 0);   // pool_in == nullptr: no state gather
    hipLaunchKernelGGL(beam_merge_dev, dim3(1), dim3(BM_NT), 0, s, m);
    LAUNCHCHK("beam_merge_dev");
    std::vector<int> srow(width), sstep(width);
    HIPCHK(hipMemcpyAsync(nh.data(), ctx->bd_nh, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), ctx->bd_len + Rm, width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sc.data(), ctx->bd_sc + Rm, width * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(toks.data(), ctx->bd_tok + Rm * lcap, toks.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(srow.data(), ctx->b_srcrow, width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sstep.data(), ctx->b_srcstep, width * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    size_t off = 0;
    for (int a = 0; a < nh[0]; ++a) {
        out_len[a] = len[a];
        for (int q = 0; q < len[a]; ++q) out_tokens[off++] = toks[(size_t)a * lcap + q];
        out_score[a] = sc[a];
        if (out_src_row) out_src_row[a] = srow[a];
        if (out_src_step) out_src_step[a] = sstep[a];
    }
    return nh[0];
}
