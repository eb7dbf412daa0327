// Host side of the greedy decoder (kernels: rnnt_decode.hip.h): the launched step path (eager or hipGraph batches) and its drain,
// the resident decoders' parameter block, selection and launchers, the control block and the stream-overlap probe.
// Included by rnnt_api.hip.

namespace {

// `n` lock-step greedy evaluations for all streams over the buffered frames (n_frames in device memory)
// (_decode_chunk_streaming_logic inner loop, online_rnnt_model.py:196-220), 4 launches per evaluation:
//   greedy_decide   apply the previous argmax to every stream's state machine (token / frame / state-buffer select)
//   LSTM cell       gates = E[tok] + h * W_hh^T, candidate (h', c') into the non-committed buffer (predictor.py:200-204)
//   joint tanh      z = tanh(enc_ffn(enc)[t_b] + (pred_ffn o projection)(h')) (joint.py:54-66, folded Linear pair)
//   joint out       logits = z * W_out^T + b, argmax fused into the epilogue (packed atomicMax; online_rnnt_model.py:212)
// Streams without frames idle.
GreedyState greedy_state(rnnt_ctx* ctx) {
    return GreedyState{ctx->tok, ctx->fidx, ctx->nsym, ctx->count, ctx->tokens, ctx->sel, ctx->key, ctx->n_active, ctx->pinned + 8};
}

int greedy_steps_raw(rnnt_ctx* ctx, hipStream_t s, int n) {
    const int B = ctx->n_streams, V = ctx->cfg.vocab_size;
    const long long bs = (long long)ctx->cfg.max_streams * D;   // floats between the two state buffers
    GreedyState st = greedy_state(ctx);
    int rc;
    for (int it = 0; it < n; ++it) {
        hipLaunchKernelGGL(greedy_decide, dim3(1), dim3(64), 0, s, B, ctx->cfg.blank_id, ctx->cfg.n_steps, ctx->cfg.max_tokens, 0, st);
        LAUNCHCHK("greedy_decide");
        GemmP g1 = plain_gemm(ctx->h, D, ctx->whh_il, D, nullptr, ctx->h, D, B, 4 * D, D, EPI_LSTM);
        g1.X = ctx->egate; g1.I = ctx->tok; g1.X2 = ctx->c; g1.Y2 = ctx->c;
        g1.Asel = ctx->sel; g1.asel_stride = bs; g1.asel_invert = 0;
        g1.act_idx = ctx->fidx; g1.act_lim = ctx->n_active + 2;
        if ((rc = launch_gemm(ctx, s, &g1, 1, TAG_LSTM))) return rc;
        GemmP g3 = plain_gemm(ctx->h, D, ctx->wjc, D, ctx->bjc, ctx->z, D, B, D, D, EPI_TANH_ADD);
        g3.Asel = ctx->sel; g3.asel_stride = bs; g3.asel_invert = 1;   // candidate h' lives in the other buffer
        g3.X = ctx->encp; g3.I = ctx->fidx; g3.x_n = 1; g3.x_s0 = (long long)ctx->fstride * D; g3.x_s1 = D;
        g3.act_idx = ctx->fidx; g3.act_lim = ctx->n_active + 2;
        if ((rc = launch_gemm(ctx, s, &g3, 1, TAG_JOINT_TANH))) return rc;
        GemmP g4 = plain_gemm(ctx->z, D, ctx->wout, D, ctx->bout, ctx->logits, ctx->vpad, B, V, D, EPI_ARGMAX);
        g4.key = ctx->key; g4.I = ctx->fidx; g4.nframes = ctx->n_active + 2;
        g4.act_idx = ctx->fidx; g4.act_lim = ctx->n_active + 2;
        if ((rc = launch_gemm(ctx, s, &g4, 1, TAG_JOINT_OUT))) return rc;
    }
    return RNNT_OK;
}

// n greedy steps over the first n_frames buffered frames; the step sequence has static arguments, so it is captured
// once per (n_streams, n) into a hipGraph and replayed with ONE host call (the path is launch-bound: 5 kernels/step).
int greedy_steps(rnnt_ctx* ctx, hipStream_t s, int n, int n_frames) {
    int rc;
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(64), 0, s, ctx->n_active + 2, n_frames, 1LL);
    LAUNCHCHK("fill_i32");
    ctx->greedy_steps += n;
    if (!ctx->use_graphs || ctx->prof_tag >= 20) return greedy_steps_raw(ctx, s, n);   // decode sites being timed: eager
    for (auto& g : ctx->dec_graphs)
        if (g.n_streams == ctx->n_streams && g.k == n) {
            HIPCHK(hipGraphLaunch(g.exec, s));
            ctx->launches += 4 * n;
            return RNNT_OK;
        }
    if (!ctx->cap_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    const int64_t l0 = ctx->launches;
    HIPCHK(hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    rc = greedy_steps_raw(ctx, ctx->cap_stream, n);
    ctx->capturing = false;
    hipError_t e = hipStreamEndCapture(ctx->cap_stream, &graph);
    ctx->launches = l0;
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess) return fail(ctx, RNNT_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(ctx, RNNT_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    ctx->dec_graphs.push_back({ctx->n_streams, n, exec});
    HIPCHK(hipGraphLaunch(exec, s));
    ctx->launches += 4 * n;
    return RNNT_OK;
}

// run step batches until every stream has consumed all n_frames frames (host checks a device counter)
int greedy_drain(rnnt_ctx* ctx, hipStream_t s, int n_frames, int done_steps) {
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(64), 0, s, ctx->n_active + 2, n_frames, 1LL);
    LAUNCHCHK("fill_i32");
    const int max_steps = (n_frames - ctx->frames_decoded) * (ctx->cfg.n_steps + 1) + 8;
    int rc;
    while (true) {
        // apply the last evaluation and count the streams that still have frames
        hipLaunchKernelGGL(greedy_decide, dim3(1), dim3(64), 0, s, ctx->n_streams, ctx->cfg.blank_id, ctx->cfg.n_steps, ctx->cfg.max_tokens, 1,
                           greedy_state(ctx));
        LAUNCHCHK("greedy_decide");
        HIPCHK(hipMemcpyAsync(ctx->pinned, ctx->n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (ctx->pinned[0] <= 0) break;
        if (done_steps > max_steps) return fail(ctx, RNNT_ERR_STATE, "greedy decode did not terminate");
        const int dstep = ctx->drain_steps;
        if ((rc = greedy_steps(ctx, s, dstep, n_frames))) return rc;
        done_steps += dstep;
    }
    return RNNT_OK;
}

// ---- resident decoders (greedy_multi / greedy_stream): ONE kernel decodes every frame up to n_total, waiting on dec_ctrl[0]
// (frames_ready).  The control block must have been initialised on a stream the launch is ordered after. --------------------------

// The parameter block both kernels share.  slots != null (stream pool): n_rows workgroups / stream groups, row i decoding stream
// slots[i] (device array) over its frames [0, n_total).
DecP dec_params(const rnnt_ctx* ctx, int n_total, int n_steps_override, const int* nlim, const int* slots, int n_rows) {
    DecP d{};
    d.whh = ctx->whh_il; d.egate = ctx->egate; d.wjc = ctx->wjc; d.bjc = ctx->bjc; d.wout = ctx->wout; d.bout = ctx->bout;
    d.encp = ctx->encp; d.h = ctx->h; d.c = ctx->c; d.sel = ctx->sel; d.tok = ctx->tok; d.fidx = ctx->fidx; d.nsym = ctx->nsym;
    d.count = ctx->count; d.tokens = ctx->tokens; d.ctrl = ctx->dec_ctrl;
    d.fstride_f = (long long)ctx->fstride * D; d.bstride = (long long)ctx->cfg.max_streams * D;
    d.B = slots ? n_rows : ctx->n_streams; d.vocab = ctx->cfg.vocab_size; d.blank = ctx->cfg.blank_id;
    d.n_steps = n_steps_override > 0 ? n_steps_override : ctx->cfg.n_steps;
    d.max_tokens = ctx->cfg.max_tokens; d.n_total = n_total; d.nlim = nlim; d.slots = slots;
    d.timeout_ticks = 500000000ll;   // 5 s of the 100 MHz real-time counter: every wait in the kernels is bounded
    return d;
}

// Can greedy_multi decode `rows` streams at once?  Its grid must be resident as a whole, and a part's vocabulary rows must fit in LDS.
// greedy_multi is a resident grid of 4 workgroups per stream that spin on each other's mailboxes; it is launched normally, not
// cooperatively, and this only checks THIS context's 4 * rows <= n_cus.  Two contexts of one process on one device (the
// two-batches-in-flight mode of bench.py / INTEGRATION.md) put 2 x 256 such workgroups on 256 CUs.  That is safe, not lucky:
// (1) a workgroup only ever waits for the three other workgroups of ITS OWN stream, never for another stream or another
// context, so the first grid always drains; (2) every workgroup of the second grid becomes resident as soon as a CU is free, and
// 4 * B <= n_cus means all of them are resident once the first grid has drained -- until then its early workgroups spin on
// partners that are not resident yet, which costs time (at most the first grid's remaining decode, ~4 ms), not progress;
// (3) the give-up bound of a wait is 5 s.  A host mutex around launch..finish (tried in round 3) serialises the two contexts'
// whole steps, because the decoder is ENQUEUED right behind its encoder: two batches in flight fell from 6.95 to 9.2 ms per batch.
// tests/test_gpu_parity.py::test_two_contexts_in_flight[64] runs this configuration.
bool multi_decoder_ok(const rnnt_ctx* ctx, int rows) {
    return ctx->use_multi && GM_PARTS * rows <= ctx->n_cus && (ctx->cfg.vocab_size + GM_PARTS - 1) / GM_PARTS <= 128;
}

int launch_multi_decoder(rnnt_ctx* ctx, hipStream_t s, const DecP& common) {
    static const bool gdbg = getenv("RNNT_GM_DBG") != nullptr;
    const int B = common.B, rows_per = (common.vocab + GM_PARTS - 1) / GM_PARTS;
    const DecMP d{common, ctx->gm_x1, ctx->gm_xa, rows_per, gdbg ? ctx->gm_dbg : nullptr};
    // (The grid on a high- or low-priority side stream, ordered by events, was tried for the two-batches-in-flight mode: 6.79 and
    // 6.33 ms per batch against 6.10-6.19 on the caller's stream.)
    // tags restart at 1 every launch: no word of an earlier launch may survive
    HIPCHK(hipMemsetAsync(ctx->gm_x1, 0, (size_t)2 * B * GM_PARTS * GM_X1 * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(ctx->gm_xa, 0, (size_t)2 * B * GM_PARTS * 2 * GREEDY_KF * sizeof(unsigned long long), s));
    const size_t lds = ((size_t)rows_per * GM_WLD + 4 * D + GREEDY_KF * D + 16 * GREEDY_KF + GM_PARTS * 2 * GREEDY_KF + 8 + GREEDY_KF * 4 * 128) * sizeof(float)
                       + GM_DBG_W * sizeof(long long);
    ctx->gm_dbg_rows = gdbg ? B : 0;
    { const int rc_attr = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&greedy_multi<GREEDY_KF>), 160 * 1024); if (rc_attr) return rc_attr; }
    hipLaunchKernelGGL(greedy_multi<GREEDY_KF>, dim3((unsigned)((B + 7) / 8 * 8 * GM_PARTS)), dim3(512), lds, s, d);
    LAUNCHCHK("greedy_multi");
    return RNNT_OK;
}

// greedy_multi (4 CUs per stream, weights stationary) if the grid of this launch can be resident, else greedy_stream (one CU per
// stream).  Stream pool: the caller launches at most n_cus / GM_PARTS rows at a time, so a slot gets the decoder that a context
// holding only that stream would run.
int launch_persistent_decoder(rnnt_ctx* ctx, hipStream_t s, int n_total, int n_steps_override = 0, const int* nlim = nullptr,
                              const int* slots = nullptr, int n_rows = 0) {
    const DecP d = dec_params(ctx, n_total, n_steps_override, nlim, slots, n_rows);
    if (multi_decoder_ok(ctx, d.B)) return launch_multi_decoder(ctx, s, d);
    hipLaunchKernelGGL(greedy_stream<GREEDY_KF>, dim3(d.B), dim3(512), 0, s, d);
    LAUNCHCHK("greedy_stream");
    return RNNT_OK;
}

int init_decoder_ctrl(rnnt_ctx* ctx, hipStream_t s, int frames_ready) {
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(64), 0, s, ctx->dec_ctrl, 0, 32LL);
    LAUNCHCHK("fill_i32");
    hipLaunchKernelGGL(publish_frames, dim3(1), dim3(1), 0, s, ctx->dec_ctrl, frames_ready);
    LAUNCHCHK("publish_frames");
    return RNNT_OK;
}

// One-time check that a kernel on `s2` can stay resident while kernels on `s` run (what the pipelined resident decoder
// relies on).  Bounded to 20 ms; on failure the pipelined path falls back to graph-launched evaluation batches.
int probe_overlap(rnnt_ctx* ctx, hipStream_t s, hipStream_t s2) {
    hipLaunchKernelGGL(fill_i32, dim3(1), dim3(64), 0, s, ctx->dec_ctrl, 0, 32LL);
    LAUNCHCHK("fill_i32");
    HIPCHK(hipStreamSynchronize(s));
    hipLaunchKernelGGL(probe_overlap_wait, dim3(1), dim3(1), 0, s2, ctx->dec_ctrl, 2000000LL);
    LAUNCHCHK("probe_overlap_wait");
    hipLaunchKernelGGL(publish_frames, dim3(1), dim3(1), 0, s, ctx->dec_ctrl, 1);
    LAUNCHCHK("publish_frames");
    HIPCHK(hipStreamSynchronize(s2));
    HIPCHK(hipStreamSynchronize(s));
    int r[2] = {0, 0};
    HIPCHK(hipMemcpy(r, ctx->dec_ctrl, sizeof(r), hipMemcpyDeviceToHost));
    ctx->overlap_ok = r[1] ? 1 : 0;
    if (!ctx->overlap_ok)
        fprintf(stderr, "[rnnt] kernels of two HIP streams do not overlap here (serialising profiler or shared hardware queue): "
                        "the resident decoder is replaced by launched evaluation batches\n");
    return RNNT_OK;
}

// wait for the decoder and check its error word; updates the evaluation counter
int finish_persistent_decoder(rnnt_ctx* ctx, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(ctx->pinned + 12, ctx->dec_ctrl, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->greedy_steps += ctx->pinned[14];
    if (ctx->gm_dbg_rows > 0) {
        // RNNT_GM_DBG: the stamps of one stream group of the launch -- the one with the largest token count (the slowest chain of the
        // batch), or row RNNT_GM_DBG_STREAM -- as microseconds per pass, dirty (predictor) and non-dirty passes apart
        const int rows = ctx->gm_dbg_rows;
        ctx->gm_dbg_rows = 0;
        std::vector<long long> t((size_t)rows * GM_DBG_W);
        (void)hipMemcpy(t.data(), ctx->gm_dbg, t.size() * sizeof(long long), hipMemcpyDeviceToHost);
        int row = 0;
        const char* want = getenv("RNNT_GM_DBG_STREAM");
        if (want && atoi(want) >= 0 && atoi(want) < rows) row = atoi(want);
        else for (int i = 1; i < rows; ++i) if (t[(size_t)i * GM_DBG_W + 24] > t[(size_t)row * GM_DBG_W + 24]) row = i;
        const long long* r = t.data() + (size_t)row * GM_DBG_W;
        static const char* const name[10] = {"frames", "W_hh", "cell+W_c", "wait X1", "tanh", "quarter sums", "finish+argmax", "XA store", "wait XA", "tail"};
        fprintf(stderr, "[greedy_multi] row %d (stream %lld, %lld tokens): %lld dirty + %lld non-dirty passes; us per pass, dirty / non-dirty:", row, r[25], r[24],
                r[22], r[10]);
        double sum[2] = {0.0, 0.0};
        for (int k = 0; k < 10; ++k) {
            const double d = r[12 + k] / 100.0 / (double)(r[22] > 0 ? r[22] : 1), n = r[k] / 100.0 / (double)(r[10] > 0 ? r[10] : 1);
            sum[0] += d; sum[1] += n;
            fprintf(stderr, " %s %.2f / %.2f,", name[k], d, n);
        }
        // The early W_hh product is off the chain: wave 0 forms its share behind its XA stores (inside what used to be its XA wait, so
        // the dirty total includes it), waves 1-7 from the quarter-sum barrier on (wave 7's time: the product under full LDS contention).
        const double e0 = r[23] / 100.0 / (double)(r[22] > 0 ? r[22] : 1), e7 = r[26] / 100.0 / (double)(r[22] > 0 ? r[22] : 1);
        // Marks inside two phases of a dirty pass: the cell alone (the rest of "cell+W_c" is a barrier and the W_c partials) and the
        // arrival of the X1 words (the rest of "wait X1" is the pp sum, the frame's tanh and the barrier).
        const double mc = r[27] / 100.0 / (double)(r[22] > 0 ? r[22] : 1), mx = r[28] / 100.0 / (double)(r[22] > 0 ? r[22] : 1);
        fprintf(stderr, " total %.2f / %.2f; hidden early W_hh per dirty pass: wave 0 %.2f (after its XA store), wave 7 %.2f (from the quarter-sum barrier);"
                        " of cell+W_c the cell %.2f, of wait X1 the arrival %.2f\n",
                sum[0] + e0, sum[1], e0, e7, mc, mx);
    }
    if (ctx->pinned[13] != 0) return fail(ctx, RNNT_ERR_STATE, "persistent decoder gave up (code %d: 1 = frame wait, 2 = greedy_multi exchange wait)", ctx->pinned[13]);
    return RNNT_OK;
}

// the resident decoder over buffered frames that are all there: control block, launch, wait (synchronises s)
int decode_resident(rnnt_ctx* ctx, hipStream_t s, int n_total, const int* nlim = nullptr, const int* slots = nullptr, int n_rows = 0, int n_steps = 0) {
    int rc;
    if ((rc = init_decoder_ctrl(ctx, s, n_total))) return rc;
    if ((rc = launch_persistent_decoder(ctx, s, n_total, n_steps, nlim, slots, n_rows))) return rc;
    return finish_persistent_decoder(ctx, s);
}

}  // namespace
