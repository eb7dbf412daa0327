// C ABI: teacher-forced scoring -- the transducer and CTC negative log-likelihoods of given transcripts (forward only) -- and
// forced alignment: the best path of a given transcript and the frame of each of its tokens.
// Below them two-pass decoding: the transducer likelihood of N hypotheses per utterance over frames projected once
// (rnnt_transducer_nll_nbest; rnnt_pool_rescore in api_pool_hist.hip.inc runs the same pipeline over kept frames) and the choice.
// Included by rnnt_api.hip inside extern "C".  Kernels: joint_lattice_rows<.., PICK> (rnnt_joint.hip.h), rnnt_score.hip.h.

// lengths and labels of a scoring call, checked on the host before anything is launched (what: the entry point's name)
static int score_check(rnnt_ctx* ctx, const char* what, const float* enc_dev, const int32_t* enc_lens, const int32_t* targets, const int32_t* target_lens,
                       int32_t B, int32_t T, int32_t Umax, double* nll_host, bool labels = true) {
    if (!ctx || !enc_dev || !enc_lens || !target_lens || !nll_host || (labels && Umax > 0 && !targets)) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", what);
    if (B < 1 || T < 1 || Umax < 0) return fail(ctx, RNNT_ERR_ARG, "%s: B=%d T=%d Umax=%d", what, B, T, Umax);
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (Umax > SCORE_UMAX) return fail(ctx, RNNT_ERR_SHAPE, "%s: Umax=%d exceeds %d labels", what, Umax, SCORE_UMAX);
    const int V = ctx->cfg.vocab_size, blank = ctx->cfg.blank_id;
    for (int b = 0; b < B; ++b) {
        if (enc_lens[b] < 1 || enc_lens[b] > T) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d frames, outside [1, %d]", what, b, enc_lens[b], T);
        if (target_lens[b] < 0 || target_lens[b] > Umax) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d labels, outside [0, %d]", what, b, target_lens[b], Umax);
        for (int u = 0; labels && u < target_lens[b]; ++u) {
            const int y = targets[(size_t)b * Umax + u];
            if (y < 0 || y >= V) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of utterance %d is %d, outside [0, %d)", what, u, b, y, V);
            if (y == blank) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of utterance %d is the blank (%d)", what, u, b, blank);
        }
    }
    return RNNT_OK;
}

// The int work buffer of a scoring call, uploaded in ONE copy: targets [B][ts] (entries beyond a row's length replaced by the
// blank: they are neither validated nor used, and the padded cells they reach stay defined) | lens [2][B] | tok [U1][B] (the
// predictor's input of step u: blank, then y_1 .. y_U; transducer only).  ts = max(Umax, 1).  targets may be null when the
// caller brings its own lattice: the rows then stay blank.
struct ScoreInts { int *tg, *lens, *tok; size_t total; };
static ScoreInts score_ints(Carve<int> c, size_t B, size_t ts, size_t tok_rows) {
    ScoreInts o;
    o.tg = c.take(B * ts);
    o.lens = c.take(2 * B);
    o.tok = c.take(tok_rows * B);
    o.total = c.off;
    return o;
}
static int score_upload(rnnt_ctx* ctx, hipStream_t s, const int32_t* enc_lens, const int32_t* targets, const int32_t* target_lens, int B,
                        int Umax, bool with_tok, std::vector<int>& host, int** tg_dev, int** lens_dev, int** tok_dev) {
    const int ts = Umax > 0 ? Umax : 1, blank = ctx->cfg.blank_id;
    const size_t tok_rows = with_tok ? Umax + 1 : 0;
    const size_t total = score_ints({}, B, ts, tok_rows).total;
    host.assign(total, blank);
    const ScoreInts h = score_ints({host.data()}, B, ts, tok_rows);
    for (int b = 0; b < B; ++b) {
        h.lens[b] = enc_lens[b];
        h.lens[B + b] = target_lens[b];
        for (int u = 0; targets && u < target_lens[b]; ++u) {
            h.tg[(size_t)b * ts + u] = targets[(size_t)b * Umax + u];
            if (with_tok) h.tok[(size_t)(u + 1) * B + b] = targets[(size_t)b * Umax + u];
        }
    }
    int rc;
    if ((rc = reserve(ctx, ctx->sc_i, total))) return rc;
    if ((rc = reserve(ctx, ctx->sc_nll, (size_t)B))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->sc_i, host.data(), total * sizeof(int), hipMemcpyHostToDevice, s));
    const ScoreInts d = score_ints({ctx->sc_i}, B, ts, tok_rows);
    *tg_dev = d.tg; *lens_dev = d.lens; *tok_dev = d.tok;
    return RNNT_OK;
}

// The picked lattice behind rnnt_transducer_nll, rnnt_transducer_align (N = 1) and rnnt_transducer_nll_nbest: joint.enc_ffn over the
// B*T frames, the predictor over [blank, y_1 .. y_Umax] from the zero state (add_blank + predictor(ys_in_pad),
// model/component/transducer.py:8-19) as Umax + 1 steps of rnnt_predictor_step's two GEMMs over B*N rows, joint.pred_ffn, then the
// pick kernel or its fallback over B x T x (N * U1) cells: the N transcripts of an utterance lie side by side along U, so they share
// its projected frames.  score_lattice_reserve: the shape refusals and the float buffers, before anything is uploaded.
static int score_lattice_reserve(rnnt_ctx* ctx, const char* what, int32_t B, int32_t T, int32_t N, int32_t Umax, const float* pick_dev) {
    int rc;
    const int V = ctx->cfg.vocab_size, U = N * (Umax + 1);
    const long long Mrows = (long long)B * T * U;
    const size_t needf = (size_t)B * T * D + (size_t)B * U * D;   // rnnt_joint's own check: e and p live in the context scratch
    if (needf > ctx->scratch.cap || Mrows >= 0x7fffffffLL - JR_ROWS)
        return fail(ctx, RNNT_ERR_SHAPE, "%s: lattice B=%d T=%d U=%d exceeds the context scratch", what, B, T, U);
    const bool rows_kernel = ctx->numerics != RNNT_NUM_F32 && ctx->joint_wfrag && V <= JR_NT * 16 && V % 4 == 0;
    // work floats: pred [B][U][256] | h, c ping-pong [2][2][B*N][256] | pick [B][T][U][2] when the caller keeps none
    const size_t n_pred = (size_t)B * U * D, n_state = (size_t)B * N * D;
    if ((rc = reserve(ctx, ctx->sc_f, n_pred + 4 * n_state + (pick_dev ? 0 : (size_t)Mrows * 2)))) return rc;
    if (!rows_kernel && (rc = reserve(ctx, ctx->sc_lat, (size_t)Mrows * V))) return rc;
    return RNNT_OK;
}

// tg [B][ts]: the target column of cell u (null: the blank everywhere); tok [U1][B*N]: the predictor's input of step u.  Both on the
// device, uploaded by the caller on the same stream.  *pick_out is pick_dev, or the internal lattice when that is null.
static int score_lattice(rnnt_ctx* ctx, const float* enc_dev, int32_t B, int32_t T, int32_t N, int32_t Umax, const int* tg, int ts, const int* tok,
                         float* pick_dev, void* stream, float** pick_out) {
    int rc;
    hipStream_t s = (hipStream_t)stream;
    const int V = ctx->cfg.vocab_size, U1 = Umax + 1, U = N * U1, R = B * N;
    const long long Mrows = (long long)B * T * U;
    const bool rows_kernel = ctx->numerics != RNNT_NUM_F32 && ctx->joint_wfrag && V <= JR_NT * 16 && V % 4 == 0;
    const size_t n_pred = (size_t)B * U * D, n_state = (size_t)R * D;
    float* pred = ctx->sc_f;
    float* hc = pred + n_pred;
    float* pick = pick_dev ? pick_dev : hc + 4 * n_state;
    HIPCHK(hipMemsetAsync(hc, 0, 4 * n_state * sizeof(float), s));   // zero state (predictor.py:165-183); set 1 is overwritten before it is read
    for (int u = 0; u < U1; ++u) {
        const float *h_in = hc + (size_t)(u & 1) * 2 * n_state, *c_in = h_in + n_state;
        float *h_out = hc + (size_t)((u + 1) & 1) * 2 * n_state, *c_out = h_out + n_state;
        GemmP g1 = plain_gemm(h_in, D, ctx->whh_il, D, nullptr, h_out, D, R, 4 * D, D, EPI_LSTM);
        g1.X = ctx->egate; g1.I = tok + (size_t)u * R; g1.X2 = c_in; g1.Y2 = c_out;
        if ((rc = launch_gemm(ctx, s, &g1, 1, TAG_LSTM))) return rc;
        GemmP g2 = plain_gemm(h_out, D, ctx->wpr, D, ctx->bpr, pred + (size_t)u * D, U1 * D, R, D, D);   // row (b, n) of step u -> pred[b][n * U1 + u]
        if ((rc = launch_gemm(ctx, s, &g2, 1, TAG_PRED_PROJ))) return rc;
    }
    if (rows_kernel) {
        float* e = ctx->scratch;
        float* pp = e + (size_t)B * T * D;
        GemmP ge = plain_gemm(enc_dev, D, ctx->wenc, D, ctx->benc, e, D, B * T, D, D, EPI_SCALE, JR_PRESCALE);
        if ((rc = launch_gemm_f32(ctx, s, &ge, 1, TAG_ENC_PROJ))) return rc;   // as rnnt_joint: the pick stays bitwise its lattice
        GemmP gp = plain_gemm(pred, D, ctx->wpf, D, ctx->bpf, pp, D, B * U, D, D, EPI_SCALE, JR_PRESCALE);
        if ((rc = launch_gemm_f32(ctx, s, &gp, 1, TAG_JOINT_TANH))) return rc;
        ProfScope prof(ctx, s, TAG_SCORE_PICK);
        JointRP jp;
        memset(&jp, 0, sizeof(jp));
        jp.e = e; jp.p = pp; jp.wfrag = ctx->joint_wfrag; jp.bias = ctx->bout; jp.M = Mrows; jp.T = T; jp.U = U; jp.V = V;
        jp.ntiles = (int)((Mrows + JR_ROWS - 1) / JR_ROWS);
        jp.counter = ctx->joint_counter;
        jp.stagger = JR_STAGGER;
        jp.targets = tg; jp.pick = pick; jp.tstride = ts; jp.blank = ctx->cfg.blank_id;
        const dim3 grid((unsigned)std::min(jp.ntiles, JR_WGS_PER_CU * ctx->n_cus));
        HIPCHK(hipMemsetAsync(ctx->joint_counter, 0, 16, s));
#define JR_PICK(NS_, F16_)                                                                                                                    \
        {                                                                                                                                     \
            if ((rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&joint_lattice_rows<NS_, F16_, true, true>), JR_LDS_ALLOC))) return rc;   \
            hipLaunchKernelGGL((joint_lattice_rows<NS_, F16_, true, true>), grid, dim3(256), JR_LDS_ALLOC, s, jp);                            \
        }
        if (ctx->numerics == RNNT_NUM_BF16) JR_PICK(1, false)
        else if (ctx->numerics == RNNT_NUM_F16X3) JR_PICK(2, true)
        else JR_PICK(2, false)
#undef JR_PICK
        LAUNCHCHK("joint_lattice_rows(pick)");
    } else {
        // exact-f32 mode, or a vocabulary rnnt_joint itself takes through the GEMM path: the whole log-softmax lattice through that
        // path, then the two columns.  Same values, V / 2 times the bytes: slow by design.
        ProfScope prof(ctx, s, TAG_SCORE_PICK);
        if ((rc = rnnt_joint(ctx, enc_dev, pred, B, T, U, 1, ctx->sc_lat, stream))) return rc;
        hipLaunchKernelGGL(pick_gather, dim3(grid_for(Mrows)), dim3(256), 0, s, ctx->sc_lat, tg, pick, Mrows, T, U, V, ts, ctx->cfg.blank_id);
        LAUNCHCHK("pick_gather");
    }
    *pick_out = pick;
    return RNNT_OK;
}

// One transcript per row (N = 1).  Uploads the int work buffer from `host`, which the caller keeps until it has synchronised.
static int score_pick(rnnt_ctx* ctx, const char* what, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                      const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, float* pick_dev, void* stream, std::vector<int>& host,
                      float** pick_out, int** lens_out) {
    int rc;
    if ((rc = score_lattice_reserve(ctx, what, B, T, 1, Umax, pick_dev))) return rc;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, (hipStream_t)stream, enc_lens_host, targets_host, target_lens_host, B, Umax, true, host, &tg, &lens, &tok))) return rc;
    *lens_out = lens;
    return score_lattice(ctx, enc_dev, B, T, 1, Umax, Umax > 0 ? tg : nullptr, Umax > 0 ? Umax : 1, tok, pick_dev, stream, pick_out);
}

// Transducer negative log-likelihood of B (frames, transcript) rows: -log of the sum over all monotonic alignments
// (torchaudio.functional.rnnt_loss, reduction "none"; online_rnnt_model.py:241-255): the picked lattice (two values per cell
// instead of the vocabulary), transducer_alpha, one copy of B doubles, one synchronisation.
int rnnt_transducer_nll(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                        int32_t B, int32_t T, int32_t Umax, double* nll_host, float* pick_dev, void* stream) {
    int rc;
    if ((rc = score_check(ctx, "rnnt_transducer_nll", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, nll_host))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> host;
    float* pick;
    int* lens;
    if ((rc = score_pick(ctx, "rnnt_transducer_nll", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, pick_dev, stream, host, &pick,
                         &lens)))
        return rc;
    {
        ProfScope prof(ctx, s, TAG_SCORE_ALPHA);
        hipLaunchKernelGGL(transducer_alpha, dim3(B), dim3(256), 0, s, pick, lens, B, T, Umax + 1, ctx->sc_nll);
        LAUNCHCHK("transducer_alpha");
    }
    HIPCHK(hipMemcpyAsync(nll_host, ctx->sc_nll, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

// CTC negative log-likelihood of B (frames, transcript) rows: nn.CTCLoss(blank, reduction="none") on
// log_softmax(ctc_lo(enc)) (OnlineCTC.forward, online_rnnt_model.py:22-32): rnnt_ctc_logprobs' projection and log-softmax over the
// B*T frames, then ctc_alpha.  +inf for a transcript its frames cannot hold.  Needs ctc_head.ctc_lo.*.
int rnnt_ctc_nll(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                 int32_t B, int32_t T, int32_t Umax, double* nll_host, void* stream) {
    int rc;
    if ((rc = score_check(ctx, "rnnt_ctc_nll", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, nll_host))) return rc;
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_nll: ctc_head.ctc_lo.* not loaded");
    const int V = ctx->cfg.vocab_size;
    if ((long long)B * T >= 0x7fffffffLL) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_ctc_nll: B=%d T=%d frames in one call", B, T);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = reserve(ctx, ctx->sc_lat, (size_t)B * T * V))) return rc;
    std::vector<int> host;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, s, enc_lens_host, targets_host, target_lens_host, B, Umax, false, host, &tg, &lens, &tok))) return rc;
    if ((rc = rnnt_ctc_logprobs(ctx, enc_dev, B * T, ctx->sc_lat, stream))) return rc;
    {
        ProfScope prof(ctx, s, TAG_SCORE_ALPHA);
        hipLaunchKernelGGL(ctc_alpha, dim3(B), dim3(512), 0, s, ctx->sc_lat, tg, lens, B, T, V, Umax > 0 ? Umax : 1, ctx->cfg.blank_id, ctx->sc_nll);
        LAUNCHCHK("ctc_alpha");
    }
    HIPCHK(hipMemcpyAsync(nll_host, ctx->sc_nll, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

// ---- forced alignment ------------------------------------------------------------------------------------------------------------------
// Device outputs of an alignment call, downloaded in ONE copy: best [B] f64 | nll [B] f64 | path [B][n] int32.
struct AlignOut { double *best, *nll; int* path; size_t total; };
static AlignOut align_out(Carve<double> c, size_t B, size_t n) {
    AlignOut o;
    o.best = c.take(B);
    o.nll = c.take(B);
    o.path = reinterpret_cast<int*>(c.take((B * n + 1) / 2));
    o.total = c.off;
    return o;
}

static int align_check(rnnt_ctx* ctx, const char* what, const float* dev, const int32_t* enc_lens, const int32_t* targets, const int32_t* target_lens,
                       int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* path_host, bool labels) {
    if (ctx && !path_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", what);
    return score_check(ctx, what, dev, enc_lens, targets, target_lens, B, T, Umax, best_host, labels);
}

// back-pointer words and outputs of one call (n path entries per row)
static int align_buffers(rnnt_ctx* ctx, size_t bp_words, int B, size_t n) {
    int rc;
    if ((rc = reserve(ctx, ctx->al_bp, bp_words))) return rc;
    return reserve(ctx, ctx->al_out, align_out({}, B, n).total);
}

static int align_download(rnnt_ctx* ctx, hipStream_t s, int B, size_t n, double* best_host, double* nll_host, int32_t* path_host) {
    const size_t total = align_out({}, B, n).total;
    std::vector<double> host(total);
    HIPCHK(hipMemcpyAsync(host.data(), ctx->al_out, total * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const AlignOut h = align_out({host.data()}, B, n);
    memcpy(best_host, h.best, (size_t)B * sizeof(double));
    if (nll_host) memcpy(nll_host, h.nll, (size_t)B * sizeof(double));
    memcpy(path_host, h.path, (size_t)B * n * sizeof(int32_t));
    return RNNT_OK;
}

static int transducer_viterbi_run(rnnt_ctx* ctx, hipStream_t s, const float* pick, const int* lens, int B, int T, int Umax, double* best_host,
                                  double* nll_host, int32_t* emit_host) {
    const int ts = Umax > 0 ? Umax : 1;
    {
        ProfScope prof(ctx, s, TAG_SCORE_VITERBI);
        const AlignOut o = align_out({ctx->al_out}, B, ts);
        hipLaunchKernelGGL(transducer_viterbi, dim3(B), dim3(256), 0, s, pick, lens, B, T, Umax + 1, ts, ctx->al_bp, o.best, o.path);
        LAUNCHCHK("transducer_viterbi");
    }
    return align_download(ctx, s, B, ts, best_host, nll_host, emit_host);
}

// The best alignment over a caller's picked lattice: only lengths go up, transducer_viterbi, one download.
int rnnt_transducer_align_pick(rnnt_ctx* ctx, const float* pick_dev, const int32_t* enc_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T,
                               int32_t Umax, double* best_host, int32_t* emit_host, void* stream) {
    int rc;
    if ((rc = align_check(ctx, "rnnt_transducer_align_pick", pick_dev, enc_lens_host, nullptr, target_lens_host, B, T, Umax, best_host, emit_host, false)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = align_buffers(ctx, (size_t)B * (Umax + 1) * ((T + 31) / 32), B, Umax > 0 ? Umax : 1))) return rc;
    std::vector<int> host;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, s, enc_lens_host, nullptr, target_lens_host, B, Umax, false, host, &tg, &lens, &tok))) return rc;
    return transducer_viterbi_run(ctx, s, pick_dev, lens, B, T, Umax, best_host, nullptr, emit_host);
}

// rnnt_transducer_nll's pipeline with transducer_viterbi behind the picked lattice; with nll_host, transducer_alpha over the same
// lattice first, so one call gives the total likelihood and the best path.
int rnnt_transducer_align(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                          int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* emit_host, double* nll_host, float* pick_dev, void* stream) {
    int rc;
    if ((rc = align_check(ctx, "rnnt_transducer_align", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, best_host, emit_host, true)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = align_buffers(ctx, (size_t)B * (Umax + 1) * ((T + 31) / 32), B, Umax > 0 ? Umax : 1))) return rc;
    std::vector<int> host;
    float* pick;
    int* lens;
    if ((rc = score_pick(ctx, "rnnt_transducer_align", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, pick_dev, stream, host, &pick,
                         &lens)))
        return rc;
    if (nll_host) {
        ProfScope prof(ctx, s, TAG_SCORE_ALPHA);
        hipLaunchKernelGGL(transducer_alpha, dim3(B), dim3(256), 0, s, pick, lens, B, T, Umax + 1, align_out({ctx->al_out}, B, 0).nll);   // (nll sits in front of the path: its place does not depend on n)
        LAUNCHCHK("transducer_alpha");
    }
    return transducer_viterbi_run(ctx, s, pick, lens, B, T, Umax, best_host, nll_host, emit_host);
}

static int ctc_viterbi_run(rnnt_ctx* ctx, hipStream_t s, const float* lp, const int32_t* enc_lens_host, const int32_t* targets_host,
                           const int32_t* target_lens_host, int B, int T, int Umax, double* best_host, int32_t* align_host) {
    int rc;
    const int ts = Umax > 0 ? Umax : 1;
    if ((rc = align_buffers(ctx, (size_t)B * (2 * ts + 1) * ((T + 15) / 16), B, T))) return rc;
    std::vector<int> host;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, s, enc_lens_host, targets_host, target_lens_host, B, Umax, false, host, &tg, &lens, &tok))) return rc;
    {
        ProfScope prof(ctx, s, TAG_SCORE_VITERBI);
        const AlignOut o = align_out({ctx->al_out}, B, T);
        hipLaunchKernelGGL(ctc_viterbi, dim3(B), dim3(512), 0, s, lp, tg, lens, B, T, ctx->cfg.vocab_size, ts, ctx->cfg.blank_id, ctx->al_bp, o.best,
                           o.path);
        LAUNCHCHK("ctc_viterbi");
    }
    return align_download(ctx, s, B, T, best_host, nullptr, align_host);
}

// The best CTC path over a caller's log-probabilities [B][T][vocab]: ctc_viterbi alone.  Needs no CTC head.
int rnnt_ctc_align_logprobs(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                            int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* align_host, void* stream) {
    int rc;
    if ((rc = align_check(ctx, "rnnt_ctc_align_logprobs", lp_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, best_host, align_host, true)))
        return rc;
    return ctc_viterbi_run(ctx, (hipStream_t)stream, lp_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, best_host, align_host);
}

// rnnt_ctc_logprobs over the B*T frames, then ctc_viterbi: the per-frame alignment torchaudio's forced_align returns.
int rnnt_ctc_align(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                   int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* align_host, void* stream) {
    int rc;
    if ((rc = align_check(ctx, "rnnt_ctc_align", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, best_host, align_host, true)))
        return rc;
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_align: ctc_head.ctc_lo.* not loaded");
    if ((long long)B * T >= 0x7fffffffLL) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_ctc_align: B=%d T=%d frames in one call", B, T);
    if ((rc = reserve(ctx, ctx->sc_lat, (size_t)B * T * ctx->cfg.vocab_size))) return rc;
    if ((rc = rnnt_ctc_logprobs(ctx, enc_dev, B * T, ctx->sc_lat, stream))) return rc;
    return ctc_viterbi_run(ctx, (hipStream_t)stream, ctx->sc_lat, enc_lens_host, targets_host, target_lens_host, B, T, Umax, best_host, align_host);
}

// ---- two-pass decoding: the transducer likelihood of an utterance's n-best ------------------------------------------------------------
// The int work buffer of an n-best call, uploaded in ONE copy: targets [B][N * U1] (entry n * U1 + u = y_{n,u+1} for u < len, else
// the blank) | frames [B] | labels [B][N] (0 for n >= n_hyp) | n_hyp [B] | tok [U1][B * N] (blank, then y_1 .. y_U; rows of missing
// hypotheses run on blanks) | slots [n_slots] (rnnt_pool_rescore: the histories to stage).
struct NbestInts { int *tg, *tl, *ul, *nh, *tok, *slots; size_t total; };
static NbestInts nbest_ints(Carve<int> c, size_t B, size_t N, size_t U1, size_t n_slots) {
    NbestInts o;
    o.tg = c.take(B * N * U1);
    o.tl = c.take(B);
    o.ul = c.take(B * N);
    o.nh = c.take(B);
    o.tok = c.take(U1 * B * N);
    o.slots = c.take(n_slots);
    o.total = c.off;
    return o;
}

// lengths and labels of an n-best call, checked on the host before anything is launched; rows n >= n_hyp are not looked at
static int nbest_check(rnnt_ctx* ctx, const char* what, const int32_t* enc_lens, const int32_t* n_hyp, const int32_t* hyp_lens, const int32_t* hyp_tokens,
                       int32_t B, int32_t T, int32_t N, int32_t Umax, double* nll_host, const float* pick_dev) {
    if (!enc_lens || !n_hyp || !hyp_lens || !nll_host || (Umax > 0 && !hyp_tokens)) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", what);
    if (B < 1 || T < 1 || Umax < 0 || N < 1 || N > 16) return fail(ctx, RNNT_ERR_ARG, "%s: B=%d T=%d N=%d (1..16) Umax=%d", what, B, T, N, Umax);
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (Umax > SCORE_UMAX) return fail(ctx, RNNT_ERR_SHAPE, "%s: Umax=%d exceeds %d labels", what, Umax, SCORE_UMAX);
    const int V = ctx->cfg.vocab_size, blank = ctx->cfg.blank_id;
    for (int b = 0; b < B; ++b) {
        if (enc_lens[b] < 1 || enc_lens[b] > T) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d frames, outside [1, %d]", what, b, enc_lens[b], T);
        if (n_hyp[b] < 1 || n_hyp[b] > N) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d hypotheses, outside [1, %d]", what, b, n_hyp[b], N);
        for (int n = 0; n < n_hyp[b]; ++n) {
            const int len = hyp_lens[(size_t)b * N + n];
            if (len < 0 || len > Umax) return fail(ctx, RNNT_ERR_ARG, "%s: hypothesis %d of utterance %d has %d labels, outside [0, %d]", what, n, b, len, Umax);
            for (int u = 0; u < len; ++u) {
                const int y = hyp_tokens[((size_t)b * N + n) * Umax + u];
                if (y < 0 || y >= V) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of hypothesis %d of utterance %d is %d, outside [0, %d)", what, u, n, b, y, V);
                if (y == blank) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of hypothesis %d of utterance %d is the blank (%d)", what, u, n, b, blank);
            }
        }
    }
    return score_lattice_reserve(ctx, what, B, T, N, Umax, pick_dev);   // the shape refusals, and the float buffers
}

// The checked call (nbest_check has reserved the float buffers): upload, (pool: stage the listed slots' histories as the frames), the shared lattice, transducer_alpha_nbest, one
// download of B * N doubles, one synchronisation.
static int nbest_run(rnnt_ctx* ctx, const float* enc_dev, const int32_t* slots_host, const int32_t* enc_lens, const int32_t* n_hyp,
                     const int32_t* hyp_lens, const int32_t* hyp_tokens, int32_t B, int32_t T, int32_t N, int32_t Umax, double* nll_host, float* pick_dev,
                     void* stream) {
    int rc;
    hipStream_t s = (hipStream_t)stream;
    const int U1 = Umax + 1, R = B * N, blank = ctx->cfg.blank_id;
    const size_t n_slots = slots_host ? B : 0, total = nbest_ints({}, B, N, U1, n_slots).total;
    std::vector<int> host(total, blank);
    const NbestInts h = nbest_ints({host.data()}, B, N, U1, n_slots);
    for (int b = 0; b < B; ++b) {
        h.tl[b] = enc_lens[b];
        h.nh[b] = n_hyp[b];
        if (slots_host) h.slots[b] = slots_host[b];
        for (int n = 0; n < N; ++n) {
            const int r = b * N + n, len = n < n_hyp[b] ? hyp_lens[r] : 0;
            h.ul[r] = len;
            for (int u = 0; u < len; ++u) {
                const int y = hyp_tokens[(size_t)r * Umax + u];
                h.tg[(size_t)r * U1 + u] = y;
                h.tok[(size_t)(u + 1) * R + r] = y;
            }
        }
    }
    if ((rc = reserve(ctx, ctx->sc_i, total))) return rc;
    if ((rc = reserve(ctx, ctx->sc_nll, (size_t)R))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->sc_i, host.data(), total * sizeof(int), hipMemcpyHostToDevice, s));
    const NbestInts d = nbest_ints({ctx->sc_i.p}, B, N, U1, n_slots);
    if (slots_host) {
        hipLaunchKernelGGL(pool_hist_gather, dim3(grid_for((long long)B * T * (D / 4))), dim3(256), 0, s, ctx->hs_stage.p, d.slots, ctx->hs_ptr.p,
                           ctx->hs_len.p, B, T);
        LAUNCHCHK("pool_hist_gather");
        enc_dev = ctx->hs_stage;
    }
    float* pick;
    if ((rc = score_lattice(ctx, enc_dev, B, T, N, Umax, d.tg, N * U1, d.tok, pick_dev, stream, &pick))) return rc;
    {
        ProfScope prof(ctx, s, TAG_SCORE_ALPHA);
        hipLaunchKernelGGL(transducer_alpha_nbest, dim3(R), dim3(256), 0, s, pick, d.tl, d.ul, d.nh, T, N, U1, ctx->sc_nll.p);
        LAUNCHCHK("transducer_alpha_nbest");
    }
    HIPCHK(hipMemcpyAsync(nll_host, ctx->sc_nll, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

// Transducer negative log-likelihood of N hypotheses per utterance over the utterance's frames, projected once: what
// rnnt_transducer_nll gives for frames b and transcript (b, n), without repeating the frames N times.
int rnnt_transducer_nll_nbest(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* n_hyp_host, const int32_t* hyp_lens_host,
                              const int32_t* hyp_tokens_host, int32_t B, int32_t T, int32_t N, int32_t Umax, double* nll_host, float* pick_dev, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!enc_dev) return fail(ctx, RNNT_ERR_ARG, "rnnt_transducer_nll_nbest: null argument");
    int rc;
    if ((rc = nbest_check(ctx, "rnnt_transducer_nll_nbest", enc_lens_host, n_hyp_host, hyp_lens_host, hyp_tokens_host, B, T, N, Umax, nll_host, pick_dev)))
        return rc;
    return nbest_run(ctx, enc_dev, nullptr, enc_lens_host, n_hyp_host, hyp_lens_host, hyp_tokens_host, B, T, N, Umax, nll_host,
                     pick_dev, stream);
}

// The choice of transducer_attention_rescoring (wenet/transducer/transducer.py:372-393) without an attention decoder: pure C++.
// No contraction: a product and a sum round separately, as the Python statement does.
int rnnt_rescore_select_host(int32_t n_hyp, const double* first_scores, const double* nll, double first_weight, double transducer_weight,
                             double* total_out, int32_t* best_out) {
#pragma clang fp contract(off)
    if (n_hyp < 1 || !first_scores || !nll || !total_out || !best_out) return RNNT_ERR_ARG;
    double best_score = -INFINITY;
    int best = 0;
    for (int i = 0; i < n_hyp; ++i) {
        const double first = first_scores[i] * first_weight, td = -nll[i] * transducer_weight;
        const double total = first + td;
        total_out[i] = total;
        if (total > best_score) { best_score = total; best = i; }
    }
    *best_out = best;
    return RNNT_OK;
}
