// C ABI: audio in for the stream pool -- the feature front-end of rnnt_fbank per slot, fed in packets (rnnt_pool_wave,
// rnnt_stream_wave_reset, rnnt_stream_get_wave_state, rnnt_wave_stage_host).  Included by rnnt_api.hip inside extern "C".
// Kernels and the index helper: rnnt_frontend.hip.h.
//
// AmplitudeToDB() runs without top_db, so no frame depends on the rest of the utterance: frame f is a function of
// x[f*512 - n_fft/2, f*512 + n_fft/2) of the reflect-padded signal alone.  A slot therefore keeps the samples a pending frame can still
// read (the carry, at most n_fft floats on the device) and two host integers; a push stages `carry | new samples` per active row so
// that the row's first new frame starts at a fixed aligned position, runs rnnt_fbank's two GEMMs and power_spectrum over
// n_active x (most frames of a row) implicit frames, and rolls every carry from the staged rows.  Five launches whatever n_active is
// (two when no row completes a frame).  The GEMMs run under the pool's GemmCapScope (always gemm16: 16-row tiles, fixed split-K
// order), so a frame's bits depend neither on the neighbours nor on how the samples were split into packets, and they are the bits of
// rnnt_fbank over the whole waveform whenever that call has fewer than 1024 frames (it takes gemm16 too).
//
// Host state per slot (PoolSlot::wave, a WvSlot): samples, frames, the (sample_rate, n_fft) of the utterance in progress, finished.  Frame
// counts are host arithmetic (wave_plan_row): the call does not synchronise.  Every refusal is decided before the first launch.

namespace {

static_assert(WAVE_CARRY_CAP >= WAVE_MAX_NFFT, "a carry holds up to n_fft samples");

int pool_wave_alloc(rnnt_ctx* ctx, hipStream_t s) {
    if (ctx->wv_carry) return RNNT_OK;
    const size_t B = (size_t)ctx->cfg.max_streams;
    int rc;
    if ((rc = calltab_alloc(ctx, ctx->wv_tab, WAVE_TAB_INTS * B))) return rc;
    if ((rc = reserve(ctx, ctx->wv_carry, B * WAVE_CARRY_CAP))) return rc;   // last: its presence says the state exists
    HIPCHK(hipMemsetAsync(ctx->wv_carry, 0, B * WAVE_CARRY_CAP * sizeof(float), s));
    return RNNT_OK;
}

bool wave_shape_ok(int sample_rate, int n_fft) { return sample_rate >= 2 && n_fft >= 64 && n_fft <= WAVE_MAX_NFFT && n_fft % 64 == 0; }

}  // namespace

int rnnt_stream_wave_reset(rnnt_ctx* ctx, int32_t slot, void* stream) {
    (void)stream;
    if (!ctx) return RNNT_ERR_ARG;
    const int B = ctx->cfg.max_streams;
    if (slot < -1 || slot >= B) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_wave_reset: slot %d outside [-1, %d)", slot, B);
    pool_wave_reset(ctx, slot < 0 ? 0 : slot, slot < 0 ? B : 1);
    return RNNT_OK;
}

int rnnt_pool_wave(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* wave_dev, int32_t n_samples, const int32_t* samples_host,
                   const int32_t* final_host, int32_t sample_rate, int32_t n_fft, float* out_dev, int32_t cap_frames, int32_t* frames_host, void* stream) {
    const char* fn = "rnnt_pool_wave";
    if (!ctx) return RNNT_ERR_ARG;
    if (!slots_host || !wave_dev || !samples_host || !final_host || !out_dev || !frames_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    const int n = n_active, n_mels = 80;
    // ---- every refusal before anything changes ----------------------------------------------------------------------------------------
    int rc = pool_slots_check(ctx, fn, n, slots_host, ctx->cfg.max_streams, "active slots", [&] {
        if (n_samples < 0 || cap_frames < 0) return fail(ctx, RNNT_ERR_ARG, "%s: n_samples %d / cap_frames %d negative", fn, n_samples, cap_frames);
        if (!wave_shape_ok(sample_rate, n_fft))
            return fail(ctx, RNNT_ERR_SHAPE, "%s: sample_rate=%d n_fft=%d (n_fft must be a multiple of 64 in [64, %d])", fn, sample_rate, n_fft, WAVE_MAX_NFFT);
        return (int)RNNT_OK;
    }, [&](int i, int) {
        if (samples_host[i] >= 0 && samples_host[i] <= n_samples) return (int)RNNT_OK;
        return fail(ctx, RNNT_ERR_ARG, "%s: row %d: %d samples outside [0, %d]", fn, i, samples_host[i], n_samples);
    });
    if (rc) return rc;
    std::vector<WaveRow> rows((size_t)n);
    int max_f = 0, max_len = WAVE_PRE;
    for (int i = 0; i < n; ++i) {
        const WvSlot& q = ctx->slot[slots_host[i]].wave;
        const int fin = final_host[i] != 0;
        if (q.finished) return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: its utterance has ended; open or reset the slot first", fn, slots_host[i]);
        if (q.nfft != 0 && (q.rate != sample_rate || q.nfft != n_fft))
            return fail(ctx, RNNT_ERR_ARG, "%s: slot %d: sample_rate %d / n_fft %d differ from the utterance in progress (%d / %d)", fn, slots_host[i],
                        sample_rate, n_fft, q.rate, q.nfft);
        if ((long long)q.samples + samples_host[i] > 0x7fffffffLL - 2 * WAVE_MAX_NFFT)
            return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: %d + %d samples in one utterance", fn, slots_host[i], q.samples, samples_host[i]);
        const WaveRow r = wave_plan_row(q.samples, samples_host[i], fin, n_fft);
        if (r.f0 != q.frames || r.cl_old > n_fft || r.cl_new > n_fft || r.cl_new > WAVE_CARRY_CAP)   // the carry bound of the index arithmetic
            return fail(ctx, RNNT_ERR_STATE, "%s: slot %d: carry bookkeeping out of step (frames %d / %d, carry %d -> %d of %d)", fn, slots_host[i], r.f0,
                        q.frames, r.cl_old, r.cl_new, n_fft);
        if (r.nf > cap_frames) return fail(ctx, RNNT_ERR_ARG, "%s: row %d: %d frames, room for %d", fn, i, r.nf, cap_frames);
        rows[i] = r;
        max_f = r.nf > max_f ? r.nf : max_f;
        max_len = r.len > max_len ? r.len : max_len;
    }
    const int nfreq = n_fft / 2 + 1;
    const int n2p = (2 * nfreq + 63) / 64 * 64, kp = (nfreq + 63) / 64 * 64;          // as rnnt_fbank
    const long long stride = ((long long)max_len + 3) / 4 * 4;                           // 16-byte aligned staged rows
    const long long M = (long long)n * max_f;
    if (M > 0x7fffffffLL / 8 || (long long)n * stride > 0x7fffffffLL) return fail(ctx, RNNT_ERR_SHAPE, "%s: %lld frames / %lld staged samples in one call", fn, M, (long long)n * stride);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = pool_wave_alloc(ctx, s))) return rc;
    if (max_f > 0 && (rc = fbank_matrices(ctx, s, sample_rate, n_fft))) return rc;
    if ((rc = reserve(ctx, ctx->wv_stage, (size_t)n * stride))) return rc;
    if ((rc = reserve(ctx, ctx->fb_spec, (size_t)M * n2p))) return rc;
    if ((rc = reserve(ctx, ctx->fb_pow, (size_t)M * kp))) return rc;
    // ---- the call's table: one async copy, no synchronisation before the launches ---------------------------------------------------
    int* tab;
    if ((rc = calltab_fill(ctx, ctx->wv_tab, tab))) return rc;
    for (int i = 0; i < n; ++i) {
        int* e = tab + (size_t)i * WAVE_TAB_INTS;
        e[0] = slots_host[i]; e[1] = rows[i].n_old; e[2] = rows[i].n_new; e[3] = rows[i].final;
    }
    if ((rc = calltab_send(ctx, ctx->wv_tab, (size_t)n * WAVE_TAB_INTS, s))) return rc;
    {
        ProfScope prof(ctx, s, TAG_WAVE_STAGE);
        hipLaunchKernelGGL(wave_stage, dim3(grid_for((long long)n * stride)), dim3(256), 0, s, wave_dev, ctx->wv_carry.p, ctx->wv_stage.p, ctx->wv_tab.dev.p, n,
                           n_samples, n_fft, stride);
        LAUNCHCHK("wave_stage");
    }
    if (max_f > 0) {
        GemmCapScope cap_scope(ctx);   // kernel and tile as for one stream's rows, however many rows share the call
        // windowed DFT: implicit frames (frame r of row i starts at i*stride + WAVE_PRE + r*hop), K = n_fft
        GemmP g1 = plain_gemm(ctx->wv_stage + WAVE_PRE, WAVE_HOP, ctx->fb_dft, n_fft, nullptr, ctx->fb_spec, n2p, (int)M, n2p, n_fft);
        g1.a_n1 = max_f; g1.a_n2 = max_f; g1.a_s0 = stride; g1.a_s1 = 0; g1.a_s2 = WAVE_HOP;
        if ((rc = launch_gemm(ctx, s, &g1, 1))) return rc;
        hipLaunchKernelGGL(power_spectrum, dim3(grid_for(M * kp)), dim3(256), 0, s, ctx->fb_spec, ctx->fb_pow, M, nfreq, kp, n2p);
        LAUNCHCHK("power_spectrum");
        // mel projection + dB: row i * max_f + r -> out_dev[i][r]
        GemmP g2 = plain_gemm(ctx->fb_pow, kp, ctx->fb_mel, kp, nullptr, out_dev, n_mels, (int)M, n_mels, kp, EPI_DB);
        g2.c_n = max_f; g2.c_s0 = (long long)cap_frames * n_mels; g2.c_r0 = 0; g2.c_mod = BIG; g2.c_s1 = n_mels;
        if ((rc = launch_gemm(ctx, s, &g2, 1))) return rc;
    }
    hipLaunchKernelGGL(wave_carry_roll, dim3(grid_for((long long)n * n_fft)), dim3(256), 0, s, ctx->wv_stage.p, ctx->wv_carry.p, ctx->wv_tab.dev.p, n, n_fft, stride);
    LAUNCHCHK("wave_carry_roll");
    for (int i = 0; i < n; ++i) {
        frames_host[i] = rows[i].nf;
        if (rows[i].n_new == 0 && !rows[i].final) continue;     // a no-op row fixes nothing
        WvSlot& q = ctx->slot[slots_host[i]].wave;
        q.samples = rows[i].n_tot; q.frames = rows[i].f0 + rows[i].nf; q.rate = sample_rate; q.nfft = n_fft; q.finished = rows[i].final;
    }
    return RNNT_OK;
}

int rnnt_stream_get_wave_state(rnnt_ctx* ctx, int32_t slot, int32_t* samples_out, int32_t* frames_out, int32_t* sample_rate_out, int32_t* n_fft_out,
                               int32_t* finished_out, int32_t* n_carry_out, float* carry_host, int32_t cap_carry, void* stream) {
    const char* fn = "rnnt_stream_get_wave_state";
    if (!ctx) return RNNT_ERR_ARG;
    if (slot < 0 || slot >= ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->cfg.max_streams);
    const WvSlot q = ctx->slot[slot].wave;
    const int n_carry = q.nfft && !q.finished ? wave_plan_row(q.samples, 0, 0, q.nfft).cl_old : 0;   // a finished utterance reads nothing more
    if (samples_out) *samples_out = q.samples;
    if (frames_out) *frames_out = q.frames;
    if (sample_rate_out) *sample_rate_out = q.rate;
    if (n_fft_out) *n_fft_out = q.nfft;
    if (finished_out) *finished_out = q.finished;
    if (n_carry_out) *n_carry_out = n_carry;
    if (!carry_host) return RNNT_OK;                        // the sizes a read needs: host only
    if (cap_carry < n_carry) return fail(ctx, RNNT_ERR_ARG, "%s: carry of %d samples, room for %d", fn, n_carry, cap_carry);
    hipStream_t s = (hipStream_t)stream;
    if (n_carry > 0 && ctx->wv_carry)
        HIPCHK(hipMemcpyAsync(carry_host, ctx->wv_carry + (size_t)slot * WAVE_CARRY_CAP, (size_t)n_carry * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

// One slot's push as a pure C++ function (no context, no GPU): the staging and the carry roll of the two kernels through the same
// index helper.  staged_out receives the row from its first new frame on (frame r of the push at r * 512), *staged_len_out samples.
int rnnt_wave_stage_host(const float* carry_in, int32_t n_carry_in, int32_t samples_so_far, const float* new_samples, int32_t n_new, int32_t final,
                         int32_t n_fft, float* staged_out, int32_t cap_staged, int32_t* staged_len_out, int32_t* first_frame_out,
                         int32_t* n_frames_out, float* carry_out, int32_t cap_carry, int32_t* n_carry_out) {
    if (!staged_len_out || !first_frame_out || !n_frames_out || !n_carry_out) return RNNT_ERR_ARG;
    if (samples_so_far < 0 || n_new < 0 || (n_new > 0 && !new_samples) || (long long)samples_so_far + n_new > 0x7fffffffLL - 2 * WAVE_MAX_NFFT) return RNNT_ERR_ARG;
    if (!wave_shape_ok(2, n_fft)) return RNNT_ERR_SHAPE;
    const WaveRow r = wave_plan_row(samples_so_far, n_new, final != 0, n_fft);
    if (n_carry_in != r.cl_old || (r.cl_old > 0 && !carry_in)) return RNNT_ERR_ARG;
    if (r.cl_new > n_fft) return RNNT_ERR_STATE;
    *staged_len_out = r.len - WAVE_PRE; *first_frame_out = r.f0; *n_frames_out = r.nf; *n_carry_out = r.cl_new;
    if (cap_staged < r.len - WAVE_PRE || cap_carry < r.cl_new || (r.len > WAVE_PRE && !staged_out) || (r.cl_new > 0 && !carry_out)) return RNNT_ERR_ARG;
    std::vector<float> row((size_t)r.len);
    for (int p = 0; p < r.len; ++p) row[p] = wave_sample(r, carry_in, new_samples, p);
    for (int p = WAVE_PRE; p < r.len; ++p) staged_out[p - WAVE_PRE] = row[p];
    for (int k = 0; k < r.cl_new; ++k) carry_out[k] = row[(size_t)(r.cs_new + k - r.j0 + WAVE_PRE)];
    return RNNT_OK;
}
