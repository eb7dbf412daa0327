// C ABI: teacher-forced scoring -- the transducer and CTC negative log-likelihoods of given transcripts (forward only).
// Included by rnnt_api.hip inside extern "C".  Kernels: joint_lattice_rows<.., PICK> (rnnt_joint.hip.h), rnnt_score.hip.h.

// lengths and labels of a scoring call, checked on the host before anything is launched (what: the entry point's name)
static int score_check(rnnt_ctx* ctx, const char* what, const float* enc_dev, const int32_t* enc_lens, const int32_t* targets, const int32_t* target_lens,
                       int32_t B, int32_t T, int32_t Umax, double* nll_host) {
    if (!ctx || !enc_dev || !enc_lens || !target_lens || !nll_host || (Umax > 0 && !targets)) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", what);
    if (B < 1 || T < 1 || Umax < 0) return fail(ctx, RNNT_ERR_ARG, "%s: B=%d T=%d Umax=%d", what, B, T, Umax);
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (Umax > SCORE_UMAX) return fail(ctx, RNNT_ERR_SHAPE, "%s: Umax=%d exceeds %d labels", what, Umax, SCORE_UMAX);
    const int V = ctx->cfg.vocab_size, blank = ctx->cfg.blank_id;
    for (int b = 0; b < B; ++b) {
        if (enc_lens[b] < 1 || enc_lens[b] > T) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d frames, outside [1, %d]", what, b, enc_lens[b], T);
        if (target_lens[b] < 0 || target_lens[b] > Umax) return fail(ctx, RNNT_ERR_ARG, "%s: utterance %d has %d labels, outside [0, %d]", what, b, target_lens[b], Umax);
        for (int u = 0; u < target_lens[b]; ++u) {
            const int y = targets[(size_t)b * Umax + u];
            if (y < 0 || y >= V) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of utterance %d is %d, outside [0, %d)", what, u, b, y, V);
            if (y == blank) return fail(ctx, RNNT_ERR_ARG, "%s: label %d of utterance %d is the blank (%d)", what, u, b, blank);
        }
    }
    return RNNT_OK;
}

// The int work buffer of a scoring call, uploaded in ONE copy: targets [B][ts] (entries beyond a row's length replaced by the
// blank: they are neither validated nor used, and the padded cells they reach stay defined) | lens [2][B] | tok [U1][B] (the
// predictor's input of step u: blank, then y_1 .. y_U; transducer only).  ts = max(Umax, 1).
static int score_upload(rnnt_ctx* ctx, hipStream_t s, const int32_t* enc_lens, const int32_t* targets, const int32_t* target_lens, int B,
                        int Umax, bool with_tok, std::vector<int>& host, int** tg_dev, int** lens_dev, int** tok_dev) {
    const int ts = Umax > 0 ? Umax : 1, U1 = Umax + 1, blank = ctx->cfg.blank_id;
    host.assign((size_t)B * ts + 2 * (size_t)B + (with_tok ? (size_t)U1 * B : 0), blank);
    int* lens = host.data() + (size_t)B * ts;
    int* tok = lens + 2 * (size_t)B;
    for (int b = 0; b < B; ++b) {
        lens[b] = enc_lens[b];
        lens[B + b] = target_lens[b];
        for (int u = 0; u < target_lens[b]; ++u) {
            host[(size_t)b * ts + u] = targets[(size_t)b * Umax + u];
            if (with_tok) tok[(size_t)(u + 1) * B + b] = targets[(size_t)b * Umax + u];
        }
    }
    int rc;
    if ((rc = grow(ctx, &ctx->sc_i, &ctx->sc_i_cap, host.size()))) return rc;
    if ((rc = grow(ctx, &ctx->sc_nll, &ctx->sc_nll_cap, (size_t)B))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->sc_i, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s));
    *tg_dev = ctx->sc_i;
    *lens_dev = ctx->sc_i + (size_t)B * ts;
    *tok_dev = *lens_dev + 2 * (size_t)B;
    return RNNT_OK;
}

// Transducer negative log-likelihood of B (frames, transcript) rows: -log of the sum over all monotonic alignments
// (torchaudio.functional.rnnt_loss, reduction "none"; online_rnnt_model.py:241-255).  joint.enc_ffn over the B*T frames, the
// predictor over [blank, y_1 .. y_Umax] from the zero state (add_blank + predictor(ys_in_pad), model/component/transducer.py:8-19)
// as Umax + 1 steps of rnnt_predictor_step's two GEMMs over B rows, joint.pred_ffn, the picked lattice (two values per cell
// instead of the vocabulary), transducer_alpha, one copy of B doubles, one synchronisation.
int rnnt_transducer_nll(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host, const int32_t* target_lens_host,
                        int32_t B, int32_t T, int32_t Umax, double* nll_host, float* pick_dev, void* stream) {
    int rc;
    if ((rc = score_check(ctx, "rnnt_transducer_nll", enc_dev, enc_lens_host, targets_host, target_lens_host, B, T, Umax, nll_host))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int V = ctx->cfg.vocab_size, U1 = Umax + 1, ts = Umax > 0 ? Umax : 1;
    const long long Mrows = (long long)B * T * U1;
    const size_t needf = (size_t)B * T * D + (size_t)B * U1 * D;   // rnnt_joint's own check: e and p live in the context scratch
    if (needf > ctx->scratch_floats || Mrows >= 0x7fffffffLL - JR_ROWS)
        return fail(ctx, RNNT_ERR_SHAPE, "rnnt_transducer_nll: lattice B=%d T=%d U=%d exceeds the context scratch", B, T, U1);
    const bool rows_kernel = ctx->numerics != RNNT_NUM_F32 && ctx->joint_wfrag && V <= JR_NT * 16 && V % 4 == 0;
    // work floats: pred [B][U1][256] | h, c ping-pong [2][2][B][256] | pick [B][T][U1][2] when the caller keeps none
    const size_t n_pred = (size_t)B * U1 * D, n_state = (size_t)B * D;
    if ((rc = grow(ctx, &ctx->sc_f, &ctx->sc_f_cap, n_pred + 4 * n_state + (pick_dev ? 0 : (size_t)Mrows * 2)))) return rc;
    if (!rows_kernel && (rc = grow(ctx, &ctx->sc_lat, &ctx->sc_lat_cap, (size_t)Mrows * V))) return rc;
    std::vector<int> host;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, s, enc_lens_host, targets_host, target_lens_host, B, Umax, true, host, &tg, &lens, &tok))) return rc;
    float* pred = ctx->sc_f;
    float* hc = pred + n_pred;
    float* pick = pick_dev ? pick_dev : hc + 4 * n_state;
    HIPCHK(hipMemsetAsync(hc, 0, 4 * n_state * sizeof(float), s));   // zero state (predictor.py:165-183); set 1 is overwritten before it is read
    for (int u = 0; u < U1; ++u) {
        const float *h_in = hc + (size_t)(u & 1) * 2 * n_state, *c_in = h_in + n_state;
        float *h_out = hc + (size_t)((u + 1) & 1) * 2 * n_state, *c_out = h_out + n_state;
        GemmP g1 = plain_gemm(h_in, D, ctx->whh_il, D, nullptr, h_out, D, B, 4 * D, D, EPI_LSTM);
        g1.X = ctx->egate; g1.I = tok + (size_t)u * B; g1.X2 = c_in; g1.Y2 = c_out;
        if ((rc = launch_gemm(ctx, s, &g1, 1))) return rc;
        GemmP g2 = plain_gemm(h_out, D, ctx->wpr, D, ctx->bpr, pred + (size_t)u * D, U1 * D, B, D, D);   // row b of step u -> pred[b][u]
        if ((rc = launch_gemm(ctx, s, &g2, 1))) return rc;
    }
    if (rows_kernel) {
        float* e = ctx->scratch;
        float* pp = e + (size_t)B * T * D;
        GemmP ge = plain_gemm(enc_dev, D, ctx->wenc, D, ctx->benc, e, D, B * T, D, D, EPI_SCALE, JR_PRESCALE);
        if ((rc = launch_gemm(ctx, s, &ge, 1))) return rc;
        GemmP gp = plain_gemm(pred, D, ctx->wpf, D, ctx->bpf, pp, D, B * U1, D, D, EPI_SCALE, JR_PRESCALE);
        if ((rc = launch_gemm(ctx, s, &gp, 1))) return rc;
        ProfScope prof(ctx, s, TAG_SCORE_PICK);
        JointRP jp;
        memset(&jp, 0, sizeof(jp));
        jp.e = e; jp.p = pp; jp.wfrag = ctx->joint_wfrag; jp.bias = ctx->bout; jp.M = Mrows; jp.T = T; jp.U = U1; jp.V = V;
        jp.ntiles = (int)((Mrows + JR_ROWS - 1) / JR_ROWS);
        jp.counter = ctx->joint_counter;
        jp.stagger = JR_STAGGER;
        jp.targets = Umax > 0 ? tg : nullptr; jp.pick = pick; jp.tstride = ts; jp.blank = ctx->cfg.blank_id;
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
        if ((rc = rnnt_joint(ctx, enc_dev, pred, B, T, U1, 1, ctx->sc_lat, stream))) return rc;
        hipLaunchKernelGGL(pick_gather, dim3(grid_for(Mrows)), dim3(256), 0, s, ctx->sc_lat, Umax > 0 ? tg : nullptr, pick, Mrows, T, U1, V, ts,
                           ctx->cfg.blank_id);
        LAUNCHCHK("pick_gather");
    }
    {
        ProfScope prof(ctx, s, TAG_SCORE_ALPHA);
        hipLaunchKernelGGL(transducer_alpha, dim3(B), dim3(256), 0, s, pick, lens, B, T, U1, ctx->sc_nll);
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
    if ((rc = grow(ctx, &ctx->sc_lat, &ctx->sc_lat_cap, (size_t)B * T * V))) return rc;
    std::vector<int> host;
    int *tg, *lens, *tok;
    if ((rc = score_upload(ctx, s, enc_lens_host, targets_host, target_lens_host, B, Umax, false, host, &tg, &lens, &tok))) return rc;
    if ((rc = rnnt_ctc_logprobs(ctx, enc_dev, B * T, ctx->sc_lat, stream))) return rc;
    hipLaunchKernelGGL(ctc_alpha, dim3(B), dim3(512), 0, s, ctx->sc_lat, tg, lens, B, T, V, Umax > 0 ? Umax : 1, ctx->cfg.blank_id, ctx->sc_nll);
    LAUNCHCHK("ctc_alpha");
    HIPCHK(hipMemcpyAsync(nll_host, ctx->sc_nll, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}
