// C ABI: the stream pool -- slots of one context that open, advance and close independently (rnnt_stream_open, rnnt_pool_chunk,
// rnnt_pool_chunk_beam, rnnt_stream_get_tokens, rnnt_stream_get_beam, rnnt_stream_get_beam_states).  Included by rnnt_api.hip inside extern "C".
//
// Every stream's state already lives per stream on the device (K/V cache, the two conv rings, LSTM h/c, last token, token buffer);
// the lock-step entry points only share its POSITION (SlotPos: cache_len, kv_start, conv_pos).  Here the position is per slot: plain
// host integers in ctx->slot[b].pos, planned and advanced by the same SlotPos methods as ctx->pos, and mirrored for each call into one
// small device table (PoolRow per active row + the slot list of the decoder), written by ONE async copy from pinned memory.  The
// rows of a call are compact -- row i * t' + f is frame f of active row i -- and every access to per-stream storage goes through
// slots[i]: the K/V and ring appends through GemmP::c_tab, attention / depthwise conv / decoder through their pool forms.  Idle
// slots are neither read nor written, and no launch is sized by them.
//
// Contract: what a slot computes is what a context holding only that stream computes through rnnt_encoder_chunk +
// rnnt_greedy_decode + rnnt_frames_consume, bit for bit.  Two things make that hold: every per-slot loop bound comes from the
// slot's own position (never from the launch's maximum), and kernel / tile choices that depend on the row count are made as for
// one stream's rows (ctx->gemm_m_cap; the resident decoder is the one a single stream gets).

namespace {

int pool_alloc(rnnt_ctx* ctx) {
    return calltab_alloc(ctx, ctx->pool_tab, (size_t)ctx->cfg.max_streams * (POOL_ROW_INTS + 2));   // + the slot list + the beam buffer index per active row
}

// the per-slot beam state (rnnt_ctx::ps_*), on the first beam call of a context with max_beam > 0: every slot starts with one
// empty hypothesis (no beam call has run in any of them yet)
int pool_beam_alloc(rnnt_ctx* ctx, hipStream_t s) {
    if (ctx->ps_nh) return RNNT_OK;
    const size_t R = ctx->max_rows, B = ctx->cfg.max_streams, state = R * (ctx->cfg.n_steps + 1) * 512;
    int rc;
    if ((rc = reserve(ctx, ctx->ps_pool[0], state))) return rc;
    if ((rc = reserve(ctx, ctx->ps_pool[1], state))) return rc;
    if ((rc = reserve(ctx, ctx->ps_tok, 2 * R * (size_t)ctx->cfg.max_tokens))) return rc;
    if ((rc = reserve(ctx, ctx->ps_len, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->ps_sc, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->ps_hs, 2 * R))) return rc;
    if ((rc = reserve(ctx, ctx->ps_nh, B))) return rc;   // last: its presence says the state exists (pool_beam_reset)
    return pool_beam_reset(ctx, s, 0, (int)B);
}

// from here on every slot has its own position (the lock-step entry points refuse until rnnt_streams_reset)
void pool_enter(rnnt_ctx* ctx) {
    if (ctx->pool_mode) return;
    for (PoolSlot& q : ctx->slot) { q.pos = ctx->pos; q.seg.frames = ctx->pos.conv_pos; }   // lock step: conv_pos counts the frames since the reset
    ctx->pool_mode = true;
}

// attention of one layer for the n active rows.  The kernel is chosen PER ROW exactly as launch_attn chooses it for that row's
// T2 (attn_stream_ok): the streaming kernel for <= 4 new frames and <= 4096 keys, the LDS-tiled one otherwise; a launch whose
// grid holds rows of the other kind lets their workgroups exit.  LDS of the streaming kernel: sized for the deepest row it serves.
int launch_attn_pool(rnnt_ctx* ctx, hipStream_t s, const AttnP& a, const PoolRow* rows_dev, const PoolRow* rows_host, int n) {
    ProfScope prof(ctx, s, TAG_ATTN);
    int n_stream = 0, max_t2 = 1;
    for (int i = 0; i < n; ++i)
        if (attn_stream_ok(ctx, a.tq, rows_host[i].T2)) { ++n_stream; max_t2 = rows_host[i].T2 > max_t2 ? rows_host[i].T2 : max_t2; }
    if (n_stream > 0) {
        const int cap = attn_t2cap(max_t2);
        const size_t lds = attn_stream_lds(cap);
        if (lds > 48 * 1024) { const int rc = ensure_dyn_lds(ctx, reinterpret_cast<const void*>(&rel_attention_stream_pool), lds); if (rc) return rc; }
        hipLaunchKernelGGL(rel_attention_stream_pool, dim3(n * RNNT_H), dim3(256), lds, s, a, rows_dev, cap);
        LAUNCHCHK("rel_attention_stream_pool");
    }
    if (n_stream < n) {
        const int sel = n_stream == 0 ? 2 : 0;   // all rows, or only those beyond the streaming kernel's range
        LAUNCH_ATTN_TILED(rel_attention_pool, s, n * RNNT_H, a.tq, 1, a, rows_dev, sel);
    }
    return RNNT_OK;
}

// run_layer for the n active rows of a pool call: the same 11 launches, per-slot positions from the table
int run_layer_pool(rnnt_ctx* ctx, hipStream_t s, int l, int n, int tq, const PoolRow* rows_dev, const PoolRow* rows_host) {
    LayerDescs d;
    LayerBufs bf{ctx->x, ctx->hbuf, ctx->qbuf, ctx->abuf, ctx->dbuf};
    int rc = build_layer(ctx, l, n, tq, tq, 0, 0, 0, nullptr, bf, d);   // positions of the descriptors are placeholders: the table has them
    if (rc) return rc;
    const int* tab = reinterpret_cast<const int*>(rows_dev);
    for (int i = 1; i < 3; ++i) { d.qkv[i].c_tab = tab; d.qkv[i].c_tab_col = POOL_COL_KV_W0; d.qkv[i].c_r0 = 0; }
    d.pw1.c_tab = tab; d.pw1.c_tab_col = POOL_COL_RING_W0; d.pw1.c_r0 = 0;
    if ((rc = launch_gemm(ctx, s, &d.ffn1m, 1, TAG_FFN1))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn2m, 1, TAG_FFN2))) return rc;
    if ((rc = launch_gemm(ctx, s, d.qkv, 3, TAG_QKV))) return rc;
    if ((rc = launch_attn_pool(ctx, s, d.attn, rows_dev, rows_host, n))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.out, 1, TAG_ATTN_OUT))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.pw1, 1, TAG_PW1))) return rc;
    {
        ProfScope prof(ctx, s, TAG_DWCONV);
        hipLaunchKernelGGL(dwconv_bn_silu_pool, dim3(grid_for((long long)n * tq * D)), dim3(256), 0, s, d.dw, rows_dev);
        LAUNCHCHK("dwconv_bn_silu_pool");
    }
    if ((rc = launch_gemm(ctx, s, &d.pw2, 1, TAG_PW2))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn1, 1, TAG_FFN1))) return rc;
    if ((rc = launch_gemm(ctx, s, &d.ffn2, 1, TAG_FFN2))) return rc;
    return launch_ln(ctx, s, d.lnf);
}

}  // namespace

int rnnt_stream_open(rnnt_ctx* ctx, int32_t slot, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "rnnt_stream_open: no weights / no streams");
    if (slot < 0 || slot >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_open: slot %d outside [0, %d)", slot, ctx->n_streams);
    if (ctx->frames_buffered != 0) return fail(ctx, RNNT_ERR_STATE, "rnnt_stream_open: %d buffered frames (consume or discard them first)", ctx->frames_buffered);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = pool_alloc(ctx))) return rc;
    hipLaunchKernelGGL(stream_slot_reset, dim3(grid_for((long long)L * ctx->cap * D)), dim3(256), 0, s, ctx->gring, ctx->xring, ctx->glu0,
                       ctx->cfg.max_streams, ctx->cap, slot, ctx->h, ctx->c, ctx->sel, ctx->key, ctx->fidx, ctx->nsym, ctx->count, ctx->tok,
                       ctx->cfg.blank_id);
    LAUNCHCHK("stream_slot_reset");
    if ((rc = pool_slot_reset(ctx, s, slot, 1))) return rc;
    pool_enter(ctx);
    ctx->slot[slot].pos = SlotPos{0, 0, 0};
    ctx->slot[slot].seg = SegSlot{};
    return RNNT_OK;
}

namespace {
enum { POOL_ENCODE = 0, POOL_GREEDY = 1, POOL_BEAM = 2, POOL_CTC_PREFIX = 3, POOL_PREFIX = 4 };

// rnnt_pool_chunk (mode POOL_ENCODE / POOL_GREEDY), rnnt_pool_chunk_beam (POOL_BEAM), rnnt_pool_chunk_ctc_prefix (POOL_CTC_PREFIX) and
// rnnt_pool_chunk_prefix (POOL_PREFIX): validation, the call's table, the encoder launches and the position bookkeeping are one code
// path; only what follows the encoder differs.  use_context: POOL_CTC_PREFIX and POOL_PREFIX; ctc_weight / transducer_weight: POOL_PREFIX only;
// use_ngram: POOL_CTC_PREFIX and POOL_PREFIX.
int pool_chunk_run(rnnt_ctx* ctx, const char* fn, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T,
                   const int32_t* offsets_host, const int32_t* required_host, int mode, int32_t beam_size, int32_t* frames_out, void* stream,
                   int32_t use_context = 0, float ctc_weight = 0.f, float transducer_weight = 0.f, int32_t use_ngram = 0) {
    if (!ctx || !slots_host || !fbank_dev || !offsets_host || !required_host) return fail(ctx, RNNT_ERR_ARG, "%s: null argument", fn);
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "%s: no weights / no streams", fn);
    if (mode == POOL_GREEDY && !ctx->use_persistent) return fail(ctx, RNNT_ERR_STATE, "%s: the greedy decode of a pool call needs the resident decoder", fn);
    if (mode == POOL_CTC_PREFIX && !ctx->wctc) return fail(ctx, RNNT_ERR_STATE, "%s: ctc_head.ctc_lo.* not loaded", fn);
    const int V = ctx->cfg.vocab_size, NS = ctx->cfg.n_steps, W = ctx->cfg.max_beam;
    if (mode == POOL_BEAM) {   // rnnt_beam_decode's range
        if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "%s: context created with max_beam = 0", fn);
        if (!ctx->use_beam_chain) return fail(ctx, RNNT_ERR_STATE, "%s: RNNT_BEAM_CHAIN=0 (the device merge follows the chain kernel only)", fn);
        if (beam_size < 1 || beam_size > W || beam_size > BM_MAX_BEAM)
            return fail(ctx, RNNT_ERR_ARG, "%s: beam_size %d outside [1, min(max_beam %d, %d)]", fn, beam_size, W, BM_MAX_BEAM);
        if (V > 512 || NS > BM_MAX_STEPS) return fail(ctx, RNNT_ERR_ARG, "%s: vocab %d > 512 or n_steps %d > %d", fn, V, NS, BM_MAX_STEPS);
    }
    if (ctx->frames_buffered != 0)
        return fail(ctx, RNNT_ERR_STATE, "%s: %d buffered frames of an earlier call (rnnt_frames_discard / rnnt_frames_consume first)", fn, ctx->frames_buffered);
    const int n = n_active;
    int tq = 0;
    // ---- validate every listed slot before anything changes: a wrong slot is a write into another caller's cache --------------------
    std::string err;
    std::vector<PoolRow> rows;
    hipStream_t s = (hipStream_t)stream;
    int rc = pool_slots_check(ctx, fn, n, slots_host, ctx->n_streams, "active slots", [&] {
        if (T < 7 || T > ctx->cfg.max_chunk_frames) return fail(ctx, RNNT_ERR_SHAPE, "chunk of %d frames outside [7, %d]", T, ctx->cfg.max_chunk_frames);
        tq = sub_len(T);
        if (tq > ctx->fcap) return fail(ctx, RNNT_ERR_SHAPE, "encoder-frame buffer capacity %d exceeded", ctx->fcap);
        rows.resize((size_t)n);
        return (int)RNNT_OK;
    }, [&](int i, int slot) {
        ChunkInfo k;
        if (!(ctx->pool_mode ? ctx->slot[slot].pos : ctx->pos).plan(tq, offsets_host[i], ctx->tcap, k, err)) return fail(ctx, RNNT_ERR_SHAPE, "slot %d: %s", slot, err.c_str());
        PoolRow& r = rows[i];
        r.slot = slot; r.T2 = k.T2; r.kv_row0 = k.kv_row0; r.pos_start = k.pos_start; r.ring_pos = k.ring_pos;
        r.kv_w0 = k.kv_w0(); r.ring_w0 = k.ring_pos % ctx->cap; r.zero = 0;
        return pool_hist_check(ctx, fn, slot, tq);
    });
    if (rc) return rc;
    if (mode == POOL_BEAM) {
        // token capacity: a hypothesis grows by at most n_steps tokens per frame.  beam_lbound is a conservative bound of the slot's
        // longest one; only when it would pass max_tokens is it refreshed from the device's lengths (one small synchronising copy, rare)
        const int grow_by = tq * NS;
        for (int i = 0; i < n; ++i) {
            const int slot = rows[i].slot;
            PoolSlot& q = ctx->slot[slot];
            if (!ctx->ps_nh) {
                if (grow_by > ctx->cfg.max_tokens) return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: %d new tokens possible, max_tokens %d", fn, slot, grow_by, ctx->cfg.max_tokens);
                continue;
            }
            if (q.beam_lbound + grow_by <= ctx->cfg.max_tokens) continue;
            std::vector<int> len((size_t)W + 1);
            HIPCHK(hipMemcpyAsync(len.data(), ctx->ps_len + (size_t)q.beam_cur * ctx->max_rows + (size_t)slot * W, W * sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(len.data() + W, ctx->ps_nh + slot, sizeof(int), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            int longest = 0;
            for (int h = 0; h < len[W] && h < W; ++h) longest = std::max(longest, len[h]);
            q.beam_lbound = longest;
            if (longest + grow_by > ctx->cfg.max_tokens)
                return fail(ctx, RNNT_ERR_SHAPE, "%s: slot %d: longest hypothesis %d + %d new tokens possible exceeds max_tokens %d", fn, slot, longest, grow_by, ctx->cfg.max_tokens);
        }
    }
    if (mode == POOL_CTC_PREFIX) {   // the search's own refusals, before anything is launched or moved; then its buffers
        if ((rc = pool_ctc_check(ctx, fn, n, slots_host, tq, beam_size, use_context, use_ngram))) return rc;
        if ((rc = reserve(ctx, ctx->cp_lp, (size_t)n * tq * V))) return rc;
        if ((rc = pool_ctc_alloc(ctx, s))) return rc;
    }
    if (mode == POOL_PREFIX) {       // likewise for the transducer prefix search
        if ((rc = pool_prefix_check(ctx, fn, n, slots_host, tq, beam_size, ctc_weight, transducer_weight, use_context, use_ngram))) return rc;
        if ((rc = pool_prefix_alloc(ctx, s, (size_t)n * tq, ctc_weight > 0.f))) return rc;
    }
    if ((rc = pool_alloc(ctx))) return rc;
    if (mode == POOL_BEAM && (rc = pool_beam_alloc(ctx, s))) return rc;
    // ---- the call's table: one async copy, no synchronisation before the launches ---------------------------------------------------
    int* tab;
    if ((rc = calltab_fill(ctx, ctx->pool_tab, tab))) return rc;
    memcpy(tab, rows.data(), (size_t)n * sizeof(PoolRow));
    for (int i = 0; i < n; ++i) tab[(size_t)n * POOL_ROW_INTS + i] = rows[i].slot;
    const bool with_cur = mode == POOL_BEAM || mode == POOL_PREFIX;   // the searches with two buffer sets: the slot's current one
    if (with_cur)
        for (int i = 0; i < n; ++i) tab[(size_t)n * (POOL_ROW_INTS + 1) + i] = mode == POOL_BEAM ? ctx->slot[rows[i].slot].beam_cur : ctx->slot[rows[i].slot].prefix_cur;
    if ((rc = calltab_send(ctx, ctx->pool_tab, (size_t)n * (POOL_ROW_INTS + (with_cur ? 2 : 1)), s))) return rc;
    const PoolRow* rows_dev = reinterpret_cast<const PoolRow*>(ctx->pool_tab.dev.p);
    const int* slots_dev = ctx->pool_tab + (size_t)n * POOL_ROW_INTS;
    pool_enter(ctx);
    {
        GemmCapScope cap_scope(ctx);
        if ((rc = run_subsample(ctx, s, fbank_dev, n, T, T, nullptr, 1, ctx->y1, ctx->y2, ctx->x))) return rc;
        for (int l = 0; l < L; ++l)
            if ((rc = run_layer_pool(ctx, s, l, n, tq, rows_dev, rows.data()))) return rc;
        // after_norm in place over the compact rows, then the joint's encoder projection into frames [0, t') of every active slot
        if ((rc = launch_ln(ctx, s, LnP{ctx->x, ctx->after_g, ctx->after_b, ctx->x, n * tq, BIG, 0, 0LL, (long long)D}))) return rc;
        if ((rc = pool_hist_append_rows(ctx, s, n, slots_host, slots_dev, tq))) return rc;   // slots that keep their frames (rnnt_stream_keep_frames)
        if ((rc = pool_endpoint_rows(ctx, s, n, slots_host, slots_dev, ctx->x, tq))) return rc;   // slots that detect their endpoint (rnnt_stream_endpoint)
        // (the transducer prefix search reads the call's frames compact, row i * t' + f, from its own buffer)
        GemmP g = plain_gemm(ctx->x, D, ctx->wenc, D, ctx->benc, mode == POOL_PREFIX ? ctx->pp_encp.p : ctx->encp.p, D, n * tq, D, D);
        if (mode != POOL_PREFIX) {
            g.c_n = tq; g.c_s0 = (long long)ctx->fstride * D; g.c_r0 = 0; g.c_mod = BIG; g.c_s1 = D;
            g.c_tab = ctx->pool_tab; g.c_tab_col = POOL_COL_ZERO;
        }
        if ((rc = launch_gemm(ctx, s, &g, 1, TAG_ENC_PROJ))) return rc;
    }
    for (int i = 0; i < n; ++i) {
        ctx->slot[rows[i].slot].pos.advance(rows[i].T2, tq, required_host[i]);
        ctx->slot[rows[i].slot].seg.frames += tq;
    }
    if (frames_out) *frames_out = tq;
    if (mode == POOL_BEAM) {
        // ---- the per-frame loop of _decode_chunk_beam_search over frames [0, t') of exactly the active slots: launches only -------------
        BeamChainP c;
        memset(&c, 0, sizeof(c));
        dec_weights(ctx, c); c.encp = ctx->encp;
        c.steps = ctx->b_steps; c.blank_lp = ctx->b_blank; c.top_lp = ctx->b_toplp; c.top_tok = ctx->b_toptok;
        c.vocab = V; c.blank = ctx->cfg.blank_id; c.k = beam_size < V - 1 ? beam_size : V - 1; c.n_steps = NS; c.slots = NS + 1;   // :467
        BeamMergeP m;
        memset(&m, 0, sizeof(m));
        m.steps = ctx->b_steps; m.blank_lp = ctx->b_blank; m.top_lp = ctx->b_toplp; m.top_tok = ctx->b_toptok;
        m.slots = NS + 1; m.lcap = ctx->cfg.max_tokens; m.n_steps = NS; m.k = c.k; m.beam = beam_size; m.width = W;
        m.blank = ctx->cfg.blank_id; m.fstride = ctx->fstride;
        BeamPoolP q = pool_beam_params(ctx);
        q.slots = slots_dev; q.cur0 = ctx->pool_tab + (size_t)n * (POOL_ROW_INTS + 1);
        for (int f = 0; f < tq; ++f) {
            q.f = f; m.f = f;
            hipLaunchKernelGGL(beam_chain_pool, dim3(n * W), dim3(512), 0, s, c, q);
            LAUNCHCHK("beam_chain_pool");
            hipLaunchKernelGGL(beam_merge_pool, dim3(n), dim3(BM_NT), 0, s, m, q);
            LAUNCHCHK("beam_merge_pool");
        }
        for (int i = 0; i < n; ++i) {
            ctx->slot[rows[i].slot].beam_cur ^= tq & 1;
            ctx->slot[rows[i].slot].beam_lbound += tq * NS;
        }
        return RNNT_OK;   // the frames are consumed: frames_buffered stays 0
    }
    if (mode == POOL_CTC_PREFIX) {
        // ---- log_softmax(ctc_lo(.)) of the compact after_norm rows (kernel choices as for one stream's rows), then the slots' searches ----
        {
            GemmCapScope cap_scope(ctx);
            if ((rc = rnnt_ctc_logprobs(ctx, ctx->x, n * tq, ctx->cp_lp, stream))) return rc;
        }
        return pool_ctc_launch(ctx, s, n, slots_host, ctx->cp_lp, tq, beam_size, use_context, use_ngram);   // the frames are consumed: frames_buffered stays 0
    }
    if (mode == POOL_PREFIX) {
        // ---- the CTC log-probabilities of the compact after_norm rows when the search fuses them, then the slots' searches ----
        if (ctc_weight > 0.f) {
            GemmCapScope cap_scope(ctx);
            if ((rc = rnnt_ctc_logprobs(ctx, ctx->x, n * tq, ctx->pp_ctc, stream))) return rc;
        }
        return pool_prefix_launch(ctx, s, n, slots_host, slots_dev, ctx->pool_tab + (size_t)n * (POOL_ROW_INTS + 1), tq, beam_size, ctc_weight,
                                  transducer_weight, use_context, use_ngram);   // the frames are consumed: frames_buffered stays 0
    }
    if (mode == POOL_ENCODE) {   // frames [0, t') of the active slots stay buffered for rnnt_get_enc_frames until rnnt_frames_discard
        hipLaunchKernelGGL(pool_scatter_frames, dim3(grid_for((long long)n * tq * (D / 4))), dim3(256), 0, s, ctx->x, ctx->encbuf, rows_dev, n, tq,
                           (long long)ctx->fstride * D);
        LAUNCHCHK("pool_scatter_frames");
        ctx->frames_buffered = tq;
        ctx->frames_decoded = 0;
        return RNNT_OK;
    }
    // ---- greedy decode of the new frames of exactly the active slots; grids sized by the rows of the call ----------------------------
    const int per = multi_decoder_ok(ctx, 1) ? (ctx->n_cus / GM_PARTS > 0 ? ctx->n_cus / GM_PARTS : 1) : n;   // greedy_multi: the whole grid resident
    for (int i0 = 0; i0 < n; i0 += per) {
        const int cnt = n - i0 < per ? n - i0 : per;
        if ((rc = decode_resident(ctx, s, tq, nullptr, slots_dev + i0, cnt))) return rc;   // synchronises
    }
    return RNNT_OK;
}
}  // namespace

int rnnt_pool_chunk(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                    const int32_t* required_host, int32_t greedy, int32_t* frames_out, void* stream) {
    return pool_chunk_run(ctx, "rnnt_pool_chunk", n_active, slots_host, fbank_dev, T, offsets_host, required_host, greedy ? POOL_GREEDY : POOL_ENCODE, 0,
                          frames_out, stream);
}

int rnnt_pool_chunk_beam(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                         const int32_t* required_host, int32_t beam_size, int32_t* frames_out, void* stream) {
    return pool_chunk_run(ctx, "rnnt_pool_chunk_beam", n_active, slots_host, fbank_dev, T, offsets_host, required_host, POOL_BEAM, beam_size, frames_out,
                          stream);
}

int rnnt_pool_chunk_ctc_prefix(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                               const int32_t* required_host, int32_t beam_size, int32_t use_context, int32_t* frames_out, void* stream) {
    return pool_chunk_run(ctx, "rnnt_pool_chunk_ctc_prefix", n_active, slots_host, fbank_dev, T, offsets_host, required_host, POOL_CTC_PREFIX, beam_size,
                          frames_out, stream, use_context);
}

int rnnt_pool_chunk_ctc_prefix_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                                     const int32_t* required_host, int32_t beam_size, int32_t use_context, int32_t use_ngram, int32_t* frames_out,
                                     void* stream) {
    return pool_chunk_run(ctx, "rnnt_pool_chunk_ctc_prefix", n_active, slots_host, fbank_dev, T, offsets_host, required_host, POOL_CTC_PREFIX, beam_size,
                          frames_out, stream, use_context, 0.f, 0.f, use_ngram);
}

int rnnt_pool_chunk_prefix(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                           const int32_t* required_host, int32_t beam_size, float ctc_weight, float transducer_weight, int32_t* frames_out, void* stream) {
    return rnnt_pool_chunk_prefix_ctx(ctx, n_active, slots_host, fbank_dev, T, offsets_host, required_host, beam_size, ctc_weight, transducer_weight, 0,
                                      frames_out, stream);
}

int rnnt_pool_chunk_prefix_ctx(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                               const int32_t* required_host, int32_t beam_size, float ctc_weight, float transducer_weight, int32_t use_context,
                               int32_t* frames_out, void* stream) {
    return rnnt_pool_chunk_prefix_ngram(ctx, n_active, slots_host, fbank_dev, T, offsets_host, required_host, beam_size, ctc_weight, transducer_weight,
                                        use_context, 0, frames_out, stream);
}

int rnnt_pool_chunk_prefix_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t T, const int32_t* offsets_host,
                                 const int32_t* required_host, int32_t beam_size, float ctc_weight, float transducer_weight, int32_t use_context,
                                 int32_t use_ngram, int32_t* frames_out, void* stream) {
    return pool_chunk_run(ctx, "rnnt_pool_chunk_prefix", n_active, slots_host, fbank_dev, T, offsets_host, required_host, POOL_PREFIX, beam_size,
                          frames_out, stream, use_context, ctc_weight, transducer_weight, use_ngram);
}

namespace {
// the slot's hypothesis count and lengths from its current buffer set (synchronises); allocates the beam state if this is its first use
int pool_beam_peek(rnnt_ctx* ctx, const char* fn, int slot, hipStream_t s, std::vector<int>& len, int& nh) {
    if (!ctx->finalized || ctx->n_streams < 1) return fail(ctx, RNNT_ERR_STATE, "%s: no weights / no streams", fn);
    if (ctx->max_rows == 0) return fail(ctx, RNNT_ERR_STATE, "%s: context created with max_beam = 0", fn);
    if (slot < 0 || slot >= ctx->n_streams) return fail(ctx, RNNT_ERR_ARG, "%s: slot %d outside [0, %d)", fn, slot, ctx->n_streams);
    int rc;
    if ((rc = pool_beam_alloc(ctx, s))) return rc;
    const int W = ctx->cfg.max_beam;
    len.assign((size_t)W + 1, 0);
    HIPCHK(hipMemcpyAsync(len.data(), ctx->ps_len + (size_t)ctx->slot[slot].beam_cur * ctx->max_rows + (size_t)slot * W, W * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data() + W, ctx->ps_nh + slot, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    nh = len[W];
    return RNNT_OK;
}
}  // namespace

int rnnt_stream_get_beam(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host, int32_t* tokens_host,
                         double* scores_host, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> len;
    int nh = 0, rc;
    if ((rc = pool_beam_peek(ctx, "rnnt_stream_get_beam", slot, s, len, nh))) return rc;
    if (n_hyp) *n_hyp = nh;
    if (!lens_host && !tokens_host && !scores_host) return RNNT_OK;
    if (cap_hyps < nh) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_beam: %d hypotheses, room for %d", nh, cap_hyps);
    const size_t row0 = (size_t)ctx->slot[slot].beam_cur * ctx->max_rows + (size_t)slot * ctx->cfg.max_beam, lcap = (size_t)ctx->cfg.max_tokens;
    for (int i = 0; i < nh; ++i) {
        if (lens_host) lens_host[i] = len[i];
        if (!tokens_host || len[i] == 0) continue;
        if (cap_tokens < len[i]) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_beam: hypothesis %d has %d tokens, room for %d", i, len[i], cap_tokens);
        HIPCHK(hipMemcpyAsync(tokens_host + (size_t)i * cap_tokens, ctx->ps_tok + (row0 + i) * lcap, (size_t)len[i] * sizeof(int), hipMemcpyDeviceToHost, s));
    }
    if (scores_host && nh > 0) HIPCHK(hipMemcpyAsync(scores_host, ctx->ps_sc + row0, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_stream_get_beam_states(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, float* h_host, float* c_host, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!h_host || !c_host) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_beam_states: null argument");
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> len;
    int nh = 0, rc;
    if ((rc = pool_beam_peek(ctx, "rnnt_stream_get_beam_states", slot, s, len, nh))) return rc;
    if (cap_hyps < nh) return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_beam_states: %d hypotheses, room for %d", nh, cap_hyps);
    if (nh == 0) return RNNT_OK;
    const size_t pitch = (size_t)(ctx->cfg.n_steps + 1) * 512 * sizeof(float);
    const float* pool = ctx->ps_pool[ctx->slot[slot].beam_cur] + (size_t)slot * ctx->cfg.max_beam * (ctx->cfg.n_steps + 1) * 512;
    HIPCHK(hipMemcpy2DAsync(h_host, D * sizeof(float), pool, pitch, D * sizeof(float), nh, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpy2DAsync(c_host, D * sizeof(float), pool + D, pitch, D * sizeof(float), nh, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return RNNT_OK;
}

int rnnt_stream_get_tokens(rnnt_ctx* ctx, int32_t slot, int32_t from, int32_t cap, int32_t* tokens_host, int32_t* n_out, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (slot < 0 || slot >= ctx->n_streams || from < 0 || cap < 0 || (cap > 0 && !tokens_host))
        return fail(ctx, RNNT_ERR_ARG, "rnnt_stream_get_tokens: bad argument");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(ctx->pinned + 5, ctx->count + slot, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int count = ctx->pinned[5];
    if (count > ctx->cfg.max_tokens) count = ctx->cfg.max_tokens;   // the counter runs on when the buffer is full
    const int avail = count > from ? count - from : 0;
    if (n_out) *n_out = avail;
    const int ncopy = avail < cap ? avail : cap;
    if (ncopy > 0) {
        HIPCHK(hipMemcpyAsync(tokens_host, ctx->tokens + (size_t)slot * ctx->cfg.max_tokens + from, (size_t)ncopy * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return RNNT_OK;
}
