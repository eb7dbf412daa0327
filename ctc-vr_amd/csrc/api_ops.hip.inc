// C ABI: step API (predictor, joint), full-context encoder, CTC head, offline greedy search, feature front-end.
// Included by rnnt_api.hip inside extern "C".

int rnnt_predictor_step(rnnt_ctx* ctx, const int32_t* tokens_dev, const float* h_in, const float* c_in, int32_t rows, float* out_dev,
                        float* h_out, float* c_out, void* stream) {
    if (!ctx || !tokens_dev || !h_in || !c_in || !out_dev || !h_out || !c_out || rows < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_predictor_step: bad argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    GemmP g1 = plain_gemm(h_in, D, ctx->whh_il, D, nullptr, h_out, D, rows, 4 * D, D, EPI_LSTM);
    g1.X = ctx->egate; g1.I = tokens_dev; g1.X2 = c_in; g1.Y2 = c_out;
    if ((rc = launch_gemm(ctx, s, &g1, 1))) return rc;
    GemmP g2 = plain_gemm(h_out, D, ctx->wpr, D, ctx->bpr, out_dev, D, rows, D, D);
    return launch_gemm(ctx, s, &g2, 1);
}

int rnnt_joint(rnnt_ctx* ctx, const float* enc_dev, const float* pred_dev, int32_t B, int32_t T, int32_t U, int32_t mode, float* logits_dev,
               void* stream) {
    if (!ctx || !enc_dev || !pred_dev || !logits_dev || B < 1 || T < 1 || U < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_joint: bad argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    hipStream_t s = (hipStream_t)stream;
    const int V = ctx->cfg.vocab_size;
    const size_t needf = (size_t)B * T * D + (size_t)B * U * D;
    if (needf > ctx->scratch.cap) return fail(ctx, RNNT_ERR_SHAPE, "joint lattice B=%d T=%d U=%d exceeds the context scratch", B, T, U);
    float* e = ctx->scratch;
    float* pp = e + (size_t)B * T * D;
    int rc;
    const long long Mrows = (long long)B * T * U;
    const bool rows_kernel = ctx->numerics != RNNT_NUM_F32 && ctx->joint_wfrag && V <= JR_NT * 16 && V % 4 == 0 && Mrows < 0x7fffffffLL - JR_ROWS;
    // joint_lattice_rows takes e and p multiplied by 2 log2(e): tanh(e + p) = 1 - 2 / (exp2(e' + p') + 1) (rnnt_joint.hip.h)
    const float pre = rows_kernel ? JR_PRESCALE : 1.0f;
    GemmP ge = plain_gemm(enc_dev, D, ctx->wenc, D, ctx->benc, e, D, B * T, D, D, rows_kernel ? EPI_SCALE : EPI_BIAS, pre);
    if ((rc = launch_gemm_f32(ctx, s, &ge, 1))) return rc;   // exact f32 in every mode: the tanh argument (host_launch.hip.inc)
    GemmP gp = plain_gemm(pred_dev, D, ctx->wpf, D, ctx->bpf, pp, D, B * U, D, D, rows_kernel ? EPI_SCALE : EPI_BIAS, pre);
    if ((rc = launch_gemm_f32(ctx, s, &gp, 1))) return rc;
    if (rows_kernel) {
        // split-operand modes: ONE lattice kernel with the (log-)softmax on the accumulators (joint_lattice_rows, rnnt_joint.hip.h):
        // persistent 64-row workgroups, two per CU, over a dynamic row-tile queue
        ProfScope prof(ctx, s, TAG_JOINT_OUT);
        JointRP jp;
        jp.e = e; jp.p = pp; jp.wfrag = ctx->joint_wfrag; jp.bias = ctx->bout; jp.out = logits_dev; jp.M = Mrows; jp.T = T; jp.U = U; jp.V = V;
        jp.ntiles = (int)((Mrows + JR_ROWS - 1) / JR_ROWS);
        jp.counter = ctx->joint_counter;
        jp.stagger = JR_STAGGER;
        const dim3 grid((unsigned)std::min(jp.ntiles, JR_WGS_PER_CU * ctx->n_cus));
        HIPCHK(hipMemsetAsync(ctx->joint_counter, 0, 16, s));
#define JR_LAUNCH(NS_, F16_)                                                                                                                  \
        {                                                                                                                                     \
            if (mode == 1) {                                                                                                                  \
                if ((rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&joint_lattice_rows<NS_, F16_, true>), JR_LDS_ALLOC))) return rc;          \
                hipLaunchKernelGGL((joint_lattice_rows<NS_, F16_, true>), grid, dim3(256), JR_LDS_ALLOC, s, jp);                              \
            } else {                                                                                                                          \
                if ((rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&joint_lattice_rows<NS_, F16_, false>), JR_LDS_ALLOC))) return rc;         \
                hipLaunchKernelGGL((joint_lattice_rows<NS_, F16_, false>), grid, dim3(256), JR_LDS_ALLOC, s, jp);                             \
            }                                                                                                                                 \
        }
        if (ctx->numerics == RNNT_NUM_BF16) JR_LAUNCH(1, false)
        else if (ctx->numerics == RNNT_NUM_F16X3) JR_LAUNCH(2, true)
        else JR_LAUNCH(2, false)
#undef JR_LAUNCH
        LAUNCHCHK("joint_lattice_rows");
        return RNNT_OK;
    }
    // exact-f32 mode: logits[b,t,u,:] = tanh(e[b,t,:] + pp[b,u,:]) * W_out^T + b_out with the tanh of the broadcast sum formed while
    // the A tile is staged into LDS (no [B,T,U,256] intermediate in HBM), then the normalisation pass for mode 1 (exact-f32 MFMA
    // makes this shape compute-bound by 6.5x, so the second pass is not what limits it)
    {
        ProfScope prof(ctx, s, TAG_JOINT_OUT);
        GemmBatch gb;
        memset(&gb, 0, sizeof(gb));
        GemmP& g = gb.g[0];
        g = plain_gemm(pp, D, ctx->wout, D, ctx->bout, logits_dev, V, B * T * U, V, D);
        g.a_n1 = T * U; g.a_n2 = U; g.a_s0 = (long long)U * D; g.a_s1 = 0; g.a_s2 = D;   // A row = pp[b, u]
        g.a_tanh = 1; g.X = e; g.x_n = U; g.x_s0 = D;                                    // X row = e[(b,t)] = e[m / U]
        if ((rc = prepare_gemm(ctx, g))) return rc;
        launch_gemm_ns<2, 2, true>(ctx, s, gb, g.M, V, 1);
        if (prefetch_depth(ctx) == 1) LAUNCHCHK("gemm_ns(joint lattice;pd1)"); else LAUNCHCHK("gemm_ns(joint lattice)");
    }
    if (mode == 1) {
        const long long rows = (long long)B * T * U;
        hipLaunchKernelGGL(log_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits_dev, rows, V);
        LAUNCHCHK("log_softmax_rows");
    }
    return RNNT_OK;
}

int rnnt_encoder_full(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B, int32_t T, float* out_dev,
                      int32_t* frames_out, void* stream) {
    if (!ctx || !fbank_dev || !lens_host || !out_dev) return fail(ctx, RNNT_ERR_ARG, "rnnt_encoder_full: null argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (B < 1 || B > ctx->cfg.max_streams || T < 7 || T > ctx->cfg.max_chunk_frames)
        return fail(ctx, RNNT_ERR_SHAPE, "rnnt_encoder_full: B=%d T=%d outside the context limits", B, T);
    const int tq = sub_len(T);
    if (tq > ctx->tcap) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_encoder_full: %d frames exceed the K/V capacity %d", tq, ctx->tcap);
    hipStream_t s = (hipStream_t)stream;
    // padding mask after subsampling: masks[:, :, 2::2][:, :, 2::2] (subsampling.py:228)
    std::vector<int> kl(B);
    for (int b = 0; b < B; ++b) {
        const int len = lens_host[b] < T ? lens_host[b] : T;
        const int n1 = len > 2 ? (len - 1) / 2 : 0;
        kl[b] = n1 > 2 ? (n1 - 1) / 2 : 0;
        if (kl[b] < 1) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_encoder_full: utterance %d too short", b);
    }
    HIPCHK(hipMemcpyAsync(ctx->klen, kl.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
    int rc;
    // fresh left context for the causal conv (zero pad, convolution.py:122-124); streaming state is clobbered
    hipLaunchKernelGGL(conv_ring_init, dim3(grid_for((long long)L * ctx->cfg.max_streams * ctx->cap * D)), dim3(256), 0, s, ctx->gring, ctx->xring,
                       ctx->glu0, ctx->cfg.max_streams, ctx->cap);
    LAUNCHCHK("conv_ring_init");
    ctx->n_streams = 0;   // streaming state invalid after a full-context pass
    if (ctx->use_lm) {
        // The full-context pass IS the layer-major schedule with one chunk of T frames: every query sees all (valid) keys at
        // positional window 0, the causal conv starts from a fresh stream's left context.  Same kernels as the streaming call.
        std::vector<ChunkInfo> ci(1);
        ci[0] = ChunkInfo{T, tq, tq, 0, 0, 0, 0, 0};
        const int32_t start0 = 0;
        std::vector<int> lkey = {B, 1, T, -1, 0, 0, 0, ctx->tcap};   // never equal to a streaming call's key
        bool done = false;
        ctx->n_streams = B;
        rc = encoder_chunks_lm(ctx, s, fbank_dev, T, &start0, ci, lkey, 0, &done, out_dev, ctx->klen);
        ctx->n_streams = 0;
        if (rc) return rc;
        if (done) {
            if (frames_out) *frames_out = tq;
            return RNNT_OK;
        }
    }
    if ((rc = run_subsample(ctx, s, fbank_dev, B, T, T, nullptr, 1, ctx->y1, ctx->y2, ctx->x))) return rc;
    for (int l = 0; l < L; ++l)
        if ((rc = run_layer(ctx, s, l, B, tq, tq, 0, 0, 0, ctx->klen))) return rc;
    if ((rc = launch_ln(ctx, s, LnP{ctx->x, ctx->after_g, ctx->after_b, out_dev, B * tq, BIG, 0, 0LL, (long long)D}))) return rc;
    if (frames_out) *frames_out = tq;
    return RNNT_OK;
}

// OnlineCTC.argmax over the full-context encoder (model/online_rnnt_model.py:37-38,655-658): per-frame argmax of
// ctc_lo(encoder(x)) for B utterances; ids_host [B, T'] int32.  The collapse rule (:660-671) stays on the host.
int rnnt_ctc_argmax(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t* ids_host,
                    int32_t* frames_out, void* stream) {
    if (!ctx || !ids_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_ctc_argmax: null argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_argmax: ctc_head.ctc_lo.* not loaded");
    hipStream_t s = (hipStream_t)stream;
    const int tq = sub_len(T);
    const size_t rows = (size_t)B * tq;
    if (rows * D + rows * 3 > ctx->scratch.cap) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_ctc_argmax: B=%d T=%d exceeds the context scratch", B, T);
    float* enc = ctx->scratch;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ctx->scratch + ((rows * D + 1) / 2) * 2);
    int* ids = reinterpret_cast<int*>(keys + rows);
    int rc, fo = 0;
    if ((rc = rnnt_encoder_full(ctx, fbank_dev, lens_host, B, T, enc, &fo, stream))) return rc;
    HIPCHK(hipMemsetAsync(keys, 0, rows * sizeof(unsigned long long), s));
    GemmP g = plain_gemm(enc, D, ctx->wctc, D, ctx->bctc, nullptr, 0, (int)rows, ctx->cfg.vocab_size, D, EPI_ARGMAX);
    g.key = keys;
    if ((rc = launch_gemm(ctx, s, &g, 1))) return rc;   // EPI_ARGMAX always takes the gemm16 (split-K) kernel
    hipLaunchKernelGGL(unpack_keys, dim3(grid_for((long long)rows)), dim3(256), 0, s, keys, ids, (long long)rows);
    LAUNCHCHK("unpack_keys");
    HIPCHK(hipMemcpyAsync(ids_host, ids, rows * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (frames_out) *frames_out = tq;
    return RNNT_OK;
}

// OnlineCTC.log_softmax (model/online_rnnt_model.py:34-35) on given encoder frames: out_dev [rows, vocab] = log_softmax(ctc_lo(enc)).
// Used by the prefix beam search's CTC fusion (wenet/transducer/search/prefix_beam_search.py:66,99-101).
int rnnt_ctc_logprobs(rnnt_ctx* ctx, const float* enc_dev, int32_t rows, float* out_dev, void* stream) {
    if (!ctx || !enc_dev || !out_dev || rows < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_ctc_logprobs: bad argument");
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (!ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "rnnt_ctc_logprobs: ctc_head.ctc_lo.* not loaded");
    hipStream_t s = (hipStream_t)stream;
    const int V = ctx->cfg.vocab_size;
    int rc;
    GemmP g = plain_gemm(enc_dev, D, ctx->wctc, D, ctx->bctc, out_dev, V, rows, V, D);
    if ((rc = launch_gemm(ctx, s, &g, 1))) return rc;
    hipLaunchKernelGGL(log_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, out_dev, (long long)rows, V);
    LAUNCHCHK("log_softmax_rows");
    return RNNT_OK;
}

// Offline greedy search (SURVEY.md §8f rank 4): model/component/transducer.py:22-70 `basic_greedy_search` as reached from
// OnlineRNNTModel.forward (online_rnnt_model.py:234-235,268) for a non-streaming model: full-context encoder, then per
// utterance a greedy RNN-T loop over its own valid frames with at most n_steps symbols per frame (default 64 there), zero
// predictor state, first token = blank.  (The reference reads `model.blank`, an attribute OnlineRNNTModel does not have;
// the blank id of the context is used.)  Unlike the streaming loop there is no forced frame advance after n_steps symbols
// other than leaving the inner loop -- which is the same thing -- so the resident decoder is reused unchanged with
// per-stream frame counts.  counts_host [B], tokens_host [B][max_tokens].
int rnnt_greedy_search_full(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t n_steps,
                            int32_t* counts_host, int32_t* tokens_host, void* stream) {
    if (!ctx || !counts_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_greedy_search_full: null argument");
    if (n_steps < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_greedy_search_full: n_steps %d", n_steps);
    hipStream_t s = (hipStream_t)stream;
    const int tq = sub_len(T);
    const size_t rows = (size_t)B * tq;
    if (rows * D > ctx->scratch.cap) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_greedy_search_full: B=%d T=%d exceeds the context scratch", B, T);
    if (tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_greedy_search_full: %d encoder frames exceed max_enc_frames %d", tq, ctx->fcap);
    int rc, fo = 0;
    if ((rc = rnnt_streams_reset(ctx, B, stream))) return rc;                                   // zero predictor state, token = blank
    if ((rc = rnnt_encoder_full(ctx, fbank_dev, lens_host, B, T, ctx->scratch, &fo, stream))) return rc;   // also fills ctx->klen (valid frames)
    ctx->n_streams = B;
    {   // joint.enc_ffn of every frame, [B*tq, 256] -> enc_proj [B][fstride][256]
        GemmP g = plain_gemm(ctx->scratch, D, ctx->wenc, D, ctx->benc, ctx->encp, D, (int)rows, D, D);
        g.c_n = tq; g.c_s0 = (long long)ctx->fstride * D; g.c_r0 = 0; g.c_mod = BIG; g.c_s1 = D;
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_ENC_PROJ))) return rc;
    }
    if ((rc = decode_resident(ctx, s, tq, ctx->klen, nullptr, 0, n_steps))) return rc;
    ctx->n_streams = 0;                                                                        // streaming state is not meaningful afterwards
    HIPCHK(hipMemcpyAsync(counts_host, ctx->count, B * sizeof(int), hipMemcpyDeviceToHost, s));
    if (tokens_host) HIPCHK(hipMemcpyAsync(tokens_host, ctx->tokens, (size_t)B * ctx->cfg.max_tokens * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

namespace {
// The DFT rows (w cos, -w sin interleaved, periodic Hamming window) and the HTK mel filterbank of (sample_rate, n_fft), in double on
// the host and cached on the device until another pair is asked for.  rnnt_fbank and rnnt_pool_wave multiply by the same two matrices.
int fbank_matrices(rnnt_ctx* ctx, hipStream_t s, int sample_rate, int n_fft) {
    if (ctx->fb_rate == sample_rate && ctx->fb_nfft == n_fft) return RNNT_OK;
    const int n_mels = 80, nfreq = n_fft / 2 + 1, n2p = (2 * nfreq + 63) / 64 * 64, kp = (nfreq + 63) / 64 * 64;
    int rc;
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = reserve_exact(ctx, ctx->fb_dft, (size_t)n2p * n_fft))) return rc;
    if ((rc = reserve_exact(ctx, ctx->fb_mel, (size_t)n_mels * kp))) return rc;
    const double pi = 3.14159265358979323846;
    std::vector<float> dft((size_t)n2p * n_fft, 0.f), mel((size_t)n_mels * kp, 0.f);
    std::vector<double> win(n_fft);
    for (int n = 0; n < n_fft; ++n) win[n] = 0.54 - 0.46 * cos(2.0 * pi * n / n_fft);   // torch.hamming_window (periodic)
    for (int k = 0; k < nfreq; ++k)
        for (int n = 0; n < n_fft; ++n) {
            const long long kn = ((long long)k * n) % n_fft;                              // exact phase reduction
            const double ph = 2.0 * pi * (double)kn / n_fft;
            dft[(size_t)(2 * k) * n_fft + n] = (float)(win[n] * cos(ph));
            dft[(size_t)(2 * k + 1) * n_fft + n] = (float)(-win[n] * sin(ph));
        }
    // torchaudio.functional.melscale_fbanks(n_freqs, 0, rate/2, 80, rate, norm=None, mel_scale="htk")
    const double fmax = (double)(sample_rate / 2);   // all_freqs = linspace(0, sample_rate // 2, n_freqs)
    const double m_max = 2595.0 * log10(1.0 + fmax / 700.0);             // f_max = float(sample_rate // 2)
    std::vector<double> fpts(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) fpts[i] = 700.0 * (pow(10.0, (m_max * i / (n_mels + 1)) / 2595.0) - 1.0);
    for (int k = 0; k < nfreq; ++k) {
        const double f = fmax * k / (nfreq - 1);
        for (int m = 0; m < n_mels; ++m) {
            const double down = (f - fpts[m]) / (fpts[m + 1] - fpts[m]);
            const double up = (fpts[m + 2] - f) / (fpts[m + 2] - fpts[m + 1]);
            const double v = down < up ? down : up;
            mel[(size_t)m * kp + k] = (float)(v > 0.0 ? v : 0.0);
        }
    }
    HIPCHK(hipMemcpy(ctx->fb_dft, dft.data(), dft.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->fb_mel, mel.data(), mel.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->fb_rate = sample_rate;
    ctx->fb_nfft = n_fft;
    return RNNT_OK;
}
}  // namespace

// Feature front-end on the device (SURVEY.md §8f): the reference's extract_audio_features (data/dataloader.py:15-41) =
// torchaudio MelSpectrogram(sample_rate, n_fft, n_mels=80, hop_length=512, window_fn=hamming_window, power=2.0)
// [defaults: win_length = n_fft, center=True, pad_mode="reflect", onesided, HTK mel scale, norm=None, f_min=0,
// f_max=sample_rate/2] followed by AmplitudeToDB() [power: 10*log10(clamp(x, 1e-10)), ref 1.0, no top_db].
// wave_dev [B][n_samples] float32 mono -> out_dev [B][1 + n_samples/512][80].  No model weights are needed.
int rnnt_fbank(rnnt_ctx* ctx, const float* wave_dev, int32_t B, int32_t n_samples, int32_t sample_rate, int32_t n_fft, float* out_dev,
               int32_t* frames_out, void* stream) {
    if (!ctx || !wave_dev || !out_dev) return fail(ctx, RNNT_ERR_ARG, "rnnt_fbank: null argument");
    const int hop = 512, n_mels = 80;
    if (B < 1 || sample_rate < 2 || n_fft < 64 || n_fft > 4096 || n_fft % 64 != 0)
        return fail(ctx, RNNT_ERR_SHAPE, "rnnt_fbank: B=%d sample_rate=%d n_fft=%d (n_fft must be a multiple of 64 in [64, 4096])", B, sample_rate, n_fft);
    if (n_samples <= n_fft / 2) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_fbank: reflect padding needs more than n_fft/2 = %d samples (got %d)", n_fft / 2, n_samples);
    hipStream_t s = (hipStream_t)stream;
    const int nfreq = n_fft / 2 + 1;
    const int n2p = (2 * nfreq + 63) / 64 * 64;          // DFT output columns (re, im interleaved), padded
    const int kp = (nfreq + 63) / 64 * 64;               // K of the mel projection, padded with zero columns
    const int T = 1 + n_samples / hop;
    const long long pstride = ((long long)n_samples + n_fft + 3) / 4 * 4;   // padded signal per stream, 16-B aligned rows
    const long long M = (long long)B * T;
    if (M > 0x7fffffffLL / 8) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_fbank: %lld frames in one call", M);
    int rc;
    if ((rc = fbank_matrices(ctx, s, sample_rate, n_fft))) return rc;   // once per (rate, n_fft)
    if ((rc = reserve(ctx, ctx->fb_pad, (size_t)B * pstride))) return rc;
    if ((rc = reserve(ctx, ctx->fb_spec, (size_t)M * n2p))) return rc;
    if ((rc = reserve(ctx, ctx->fb_pow, (size_t)M * kp))) return rc;
    hipLaunchKernelGGL(reflect_pad, dim3(grid_for((long long)B * pstride)), dim3(256), 0, s, wave_dev, ctx->fb_pad, B, n_samples, n_fft / 2, pstride);
    LAUNCHCHK("reflect_pad");
    // windowed DFT: implicit frames (row t of stream b starts at b*pstride + t*hop), K = n_fft
    GemmP g1 = plain_gemm(ctx->fb_pad, hop, ctx->fb_dft, n_fft, nullptr, ctx->fb_spec, n2p, (int)M, n2p, n_fft);
    g1.a_n1 = T; g1.a_n2 = T; g1.a_s0 = pstride; g1.a_s1 = 0; g1.a_s2 = hop;
    if ((rc = launch_gemm(ctx, s, &g1, 1))) return rc;
    hipLaunchKernelGGL(power_spectrum, dim3(grid_for(M * kp)), dim3(256), 0, s, ctx->fb_spec, ctx->fb_pow, M, nfreq, kp, n2p);
    LAUNCHCHK("power_spectrum");
    GemmP g2 = plain_gemm(ctx->fb_pow, kp, ctx->fb_mel, kp, nullptr, out_dev, n_mels, (int)M, n_mels, kp, EPI_DB);
    if ((rc = launch_gemm(ctx, s, &g2, 1))) return rc;
    if (frames_out) *frames_out = T;
    return RNNT_OK;
}
