// C ABI: context life cycle, weight ingest / packing (rnnt_finalize_weights), stream reset.  Included by rnnt_api.hip inside extern "C".

int rnnt_abi_version(void) { return 3; }

const char* rnnt_last_error(const rnnt_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rnnt_create(const rnnt_config* cfg, rnnt_ctx** out) {
    if (!cfg || !out) return RNNT_ERR_ARG;
    *out = nullptr;
    rnnt_ctx* ctx = new rnnt_ctx();
    ctx->cfg = *cfg;
    *out = ctx;   // returned even on failure so the caller can read rnnt_last_error, then destroy
    if (cfg->max_streams < 1 || cfg->max_chunk_frames < 7 || cfg->max_cache_frames < 1 || cfg->max_cache_frames > RNNT_PE_LEN ||
        cfg->max_enc_frames < 1 || cfg->max_tokens < 1 || cfg->vocab_size < 2 || cfg->blank_id < 0 || cfg->blank_id >= cfg->vocab_size ||
        cfg->n_steps < 1 || cfg->max_beam < 0 || cfg->max_beam > 64)
        return fail(ctx, RNNT_ERR_ARG, "rnnt_create: bad config");
    HIPCHK(hipSetDevice(cfg->device));
    if (const char* ng = getenv("RNNT_NO_GRAPH")) ctx->use_graphs = (ng[0] == '1') ? 0 : 1;
    if (const char* pe = getenv("RNNT_PERSISTENT")) ctx->use_persistent = (pe[0] == '0') ? 0 : 1;
    if (const char* me = getenv("RNNT_DEC_MULTI")) ctx->use_multi = (me[0] == '0') ? 0 : 1;
    HIPCHK(hipDeviceGetAttribute(&ctx->n_cus, hipDeviceAttributeMultiprocessorCount, cfg->device));
    if (const char* ae = getenv("RNNT_ATTN_STREAM")) ctx->attn_stream = (ae[0] == '0') ? 0 : 1;
    if (const char* be = getenv("RNNT_BEAM_CHAIN")) ctx->use_beam_chain = (be[0] == '0') ? 0 : 1;
    if (const char* pg = getenv("RNNT_PREFIX_GROUP")) ctx->prefix_group = pg[0] == '1' ? 1 : (pg[0] == '4' ? 4 : 0);
    if (const char* fu = getenv("RNNT_FUSED")) ctx->use_fused = atoi(fu);   // 0 off, 1 split-operand modes (default), 2 every mode
    if (const char* fe = getenv("RNNT_FUSE_AFTER_NORM")) ctx->fuse_after_norm = (fe[0] == '0') ? 0 : 1;
    if (const char* me = getenv("RNNT_WF_MERGE")) { const int m = atoi(me); ctx->wf_merge = m < 1 ? 1 : (m > WF_MERGE_MAX ? WF_MERGE_MAX : m); }
    if (const char* le = getenv("RNNT_LM")) ctx->use_lm = (le[0] == '0') ? 0 : 1;
    if (const char* ae2 = getenv("RNNT_AS")) ctx->use_as = (ae2[0] == '0') ? 0 : 1;
    if (const char* e_ = getenv("RNNT_LM_PW2_HEAD")) ctx->lm_pw2_head = atoi(e_);
    if (const char* e_ = getenv("RNNT_LM_FFN_MERGE")) ctx->lm_ffn_merge = atoi(e_);
    if (const char* e_ = getenv("RNNT_LM_SIDE")) ctx->lm_side = atoi(e_);
    if (const char* e_ = getenv("RNNT_LM_QKV_TAIL")) ctx->lm_qkv_tail = atoi(e_);
    if (const char* e_ = getenv("RNNT_LM_OUT_CHAIN")) ctx->lm_out_chain = atoi(e_);
    if (const char* e_ = getenv("RNNT_ATTN_BF")) ctx->attn_bf = atoi(e_);
    if (const char* e_ = getenv("RNNT_ATTN_RESIDENT")) ctx->attn_resident = atoi(e_);
    if (const char* e_ = getenv("RNNT_CONV1_FUSE")) ctx->conv1_fuse = atoi(e_);
    if (const char* se = getenv("RNNT_WF_SUB_ASYNC")) ctx->wf_sub_async = (se[0] == '0') ? 0 : 1;
    if (const char* e_ = getenv("RNNT_FFN_NW")) ctx->ffn_nw = atoi(e_);
    if (const char* e_ = getenv("RNNT_GEMM_PD")) ctx->gemm_pd = atoi(e_);
    if (const char* e_ = getenv("RNNT_CONV2_BW")) ctx->conv2_bw = atoi(e_);
    if (const char* e_ = getenv("RNNT_CONV1_ROWS")) ctx->conv1_rows = atoi(e_);
    if (const char* e_ = getenv("RNNT_CONV2_LDS")) ctx->conv2_lds = atoi(e_);
    if (const char* e_ = getenv("RNNT_BW_NW")) ctx->bw_nw = atoi(e_);
    if (const char* e_ = getenv("RNNT_GEMM_NS")) ctx->gemm_ns = atoi(e_);
    if (const char* e_ = getenv("RNNT_NS_MIN_GROUPS")) ctx->ns_min_groups = atoi(e_);
    if (const char* e_ = getenv("RNNT_XCD_X")) ctx->xcd_x = atoi(e_);
    if (const char* e_ = getenv("RNNT_FUSE_MERGE")) ctx->fuse_merge = atoi(e_);
    if (const char* e_ = getenv("RNNT_FUSE_FRAMES")) ctx->fuse_frames = atoi(e_);
    if (const char* e_ = getenv("RNNT_ATTN_PAIR_MAJOR")) ctx->attn_pair_major = atoi(e_);
    if (const char* e_ = getenv("RNNT_DEC_SLACK")) ctx->dec_slack = atoi(e_);
    if (const char* e_ = getenv("RNNT_DRAIN_STEPS")) ctx->drain_steps = atoi(e_);
    const int B = cfg->max_streams;
    ctx->slot = std::vector<PoolSlot>((size_t)B);   // max_streams is fixed here, so the pool's per-slot host state is too
    ctx->hs_buf = std::vector<DevBuf<float>>((size_t)B);
    ctx->tmax = sub_len(cfg->max_chunk_frames);
    ctx->t1max = sub1_len(cfg->max_chunk_frames);
    ctx->cap = RNNT_LORDER + WF_MERGE_MAX * ctx->tmax;   // several chunks of one layer may be in flight in one wavefront stage
    ctx->tcap = cfg->max_cache_frames;
    ctx->fcap = cfg->max_enc_frames;
    ctx->fstride = ctx->fcap + 1;   // +1 row: finished streams read one frame past the end
    ctx->vpad = (cfg->vocab_size + 31) / 32 * 32;
    const size_t M = (size_t)B * ctx->tmax;
    int rc;
#define ALLOC(p, n) if ((rc = reserve(ctx, ctx->p, (size_t)(n)))) return rc
    ALLOC(y1, (size_t)B * ctx->t1max * RNNT_F1 * D);
    ALLOC(y2, M * RNNT_FSUB * D);
    ALLOC(x, M * D);
    ALLOC(hbuf, M * FF);
    ALLOC(qbuf, M * D);
    ALLOC(abuf, M * D);
    ALLOC(dbuf, M * D);
    ALLOC(kcache, (size_t)L * B * ctx->tcap * D);
    ALLOC(vcache, (size_t)L * B * ctx->tcap * D);
    ALLOC(gring, (size_t)L * B * ctx->cap * D);
    ALLOC(xring, (size_t)L * B * ctx->cap * D);
    ALLOC(encbuf, (size_t)B * ctx->fstride * D);
    ALLOC(encp, (size_t)B * ctx->fstride * D);
    ALLOC(h, (size_t)2 * B * D); ALLOC(c, (size_t)2 * B * D); ALLOC(sel, B); ALLOC(key, B);
    ALLOC(pred, (size_t)B * D); ALLOC(z, (size_t)B * D); ALLOC(logits, (size_t)B * ctx->vpad);
    ALLOC(tok, B); ALLOC(fidx, B); ALLOC(nsym, B); ALLOC(count, B); ALLOC(tokens, (size_t)B * cfg->max_tokens);
    ALLOC(n_active, 4); ALLOC(klen, B); ALLOC(dec_ctrl, 32);
    ALLOC(gm_dbg, (size_t)B * GM_DBG_W);
    ALLOC(gm_x1, (size_t)2 * B * GM_PARTS * GM_X1);
    ALLOC(gm_xa, (size_t)2 * B * GM_PARTS * 2 * GREEDY_KF);
    if (cfg->max_beam > 0) {
        ctx->max_rows = B * cfg->max_beam;
        const size_t R = ctx->max_rows, NS = cfg->n_steps, KB = cfg->max_beam;
        ALLOC(pool[0], R * (NS + 1) * 512); ALLOC(pool[1], R * (NS + 1) * 512);
        ALLOC(bpred, R * D); ALLOC(bz, R * D); ALLOC(blogits, R * ctx->vpad);
        ALLOC(b_blank, R * NS); ALLOC(b_toplp, R * NS * KB); ALLOC(b_toptok, R * NS * KB);
        ALLOC(b_tok, R); ALLOC(b_frame, R); ALLOC(b_active, R); ALLOC(b_steps, R); ALLOC(b_srcrow, R); ALLOC(b_srcstep, R);
    }
    ALLOC(scratch, std::max((size_t)L * RNNT_H * ctx->tcap * 128, (size_t)B * ctx->fstride * D));
    ALLOC(pinned, 16);
#undef ALLOC
    HIPCHK(hipMemset(ctx->encbuf, 0, (size_t)B * ctx->fstride * D * sizeof(float)));
    HIPCHK(hipMemset(ctx->encp, 0, (size_t)B * ctx->fstride * D * sizeof(float)));
    return RNNT_OK;
}

void rnnt_destroy(rnnt_ctx* ctx) {
    if (ctx) delete ctx;
}

int64_t rnnt_live_device_bytes(void) { return live_device_bytes.load(); }

int rnnt_load_tensor(rnnt_ctx* ctx, const char* name, const float* host_data, int32_t ndim, const int64_t* dims) {
    if (!ctx || !name || ndim < 0 || ndim > 8) return fail(ctx, RNNT_ERR_ARG, "rnnt_load_tensor: bad argument");
    std::string n(name);
    if (n.find("num_batches_tracked") != std::string::npos) return RNNT_OK;   // int64 counter, unused in eval
    if (!host_data) return fail(ctx, RNNT_ERR_ARG, "rnnt_load_tensor(%s): null data", name);
    HostTensor t;
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        if (dims[i] < 0) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_load_tensor(%s): negative dim", name);
        t.dims.push_back(dims[i]);
        cnt *= (size_t)dims[i];
    }
    t.data.assign(host_data, host_data + cnt);
    ctx->host[n] = std::move(t);
    ctx->finalized = false;
    return RNNT_OK;
}

int rnnt_load_packed(rnnt_ctx* ctx, const float* blob, int64_t n_floats, int32_t on_device, int32_t n_tensors, const char* const* names,
                     const int32_t* ndims, const int64_t* dims_flat) {
    if (!ctx || !blob || !names || !ndims || !dims_flat || n_floats < 0 || n_tensors < 1) return fail(ctx, RNNT_ERR_ARG, "rnnt_load_packed: bad argument");
    std::vector<float> host;
    const float* src = blob;
    if (on_device) {
        HIPCHK(hipSetDevice(ctx->cfg.device));
        host.resize((size_t)n_floats);
        HIPCHK(hipMemcpy(host.data(), blob, (size_t)n_floats * sizeof(float), hipMemcpyDeviceToHost));
        src = host.data();
    }
    int64_t off = 0, d = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (!names[i] || ndims[i] < 0 || ndims[i] > 8) return fail(ctx, RNNT_ERR_ARG, "rnnt_load_packed: tensor %d malformed", i);
        int64_t cnt = 1;
        for (int k = 0; k < ndims[i]; ++k) {
            if (dims_flat[d + k] < 0) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_load_packed(%s): negative dim", names[i]);
            cnt *= dims_flat[d + k];
        }
        if (off + cnt > n_floats) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_load_packed: the table needs more than the %lld floats given (at %s)", (long long)n_floats, names[i]);
        const int rc = rnnt_load_tensor(ctx, names[i], src + off, ndims[i], dims_flat + d);
        if (rc) return rc;
        off += cnt;
        d += ndims[i];
    }
    if (off != n_floats) return fail(ctx, RNNT_ERR_SHAPE, "rnnt_load_packed: the table covers %lld of %lld floats", (long long)off, (long long)n_floats);
    return RNNT_OK;
}

// f32 -> nearest f16 value (ties to even) as f32: the rounding of pack2_16<true>, on the host
static inline float round_f16_host(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    const uint32_t sign = u & 0x80000000u;
    uint32_t a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return x;                      // inf / nan
    if (a >= 0x477ff000u) a = 0x7f800000u;               // >= 65520 rounds to inf
    else if (a < 0x38800000u) {                          // below 2^-14: f16 subnormal, quantum 2^-24 = the ulp of f32 in [0.5, 1)
        float f;
        memcpy(&f, &a, 4);
        f = (f + 0.5f) - 0.5f;
        memcpy(&a, &f, 4);
    } else {
        a += 0xfffu + ((a >> 13) & 1u);
        a &= ~0x1fffu;
    }
    a |= sign;
    float r;
    memcpy(&r, &a, 4);
    return r;
}

// The operand range of the f16x3 mode (include/rnnt_hip.h): every GEMM weight the mode carries as two f16 planes must survive the
// split.  |w| > 65504 overflows the hi plane; the lo plane of any |w| < 2^-3 is an f16 subnormal, its error absolute (up to 2^-25)
// instead of relative, so a tensor of small weights loses precision with every halving.  A tensor whose planes miss it by more than
// RNNT_F16X3_SPLIT_LIMIT of its r.m.s. magnitude is refused by name: the mode never returns frames off the parity bar silently.
// linear_pos, weight_ih and predictor.embed only feed tables that finalize derives in exact f32; conv.0 and the depthwise conv run in f32.
static int f16x3_refusal(rnnt_ctx* ctx) {
    static const char* const skip[] = {"depthwise_conv", "linear_pos", "pos_enc", "pos_bias", "embed.conv.0", "predictor.embed", "weight_ih"};
    for (const auto& kv : ctx->host) {
        const HostTensor& t = kv.second;
        if (t.dims.size() < 2) continue;
        bool skipped = false;
        for (const char* s : skip) skipped = skipped || kv.first.find(s) != std::string::npos;
        if (skipped) continue;
        double err2 = 0.0, mag2 = 0.0;
        float amax = 0.f;
        for (const float x : t.data) {
            const float hi = round_f16_host(x);
            const float lo = round_f16_host(x - hi);
            const double e = (double)x - ((double)hi + (double)lo);
            err2 += e * e;
            mag2 += (double)x * (double)x;
            amax = fmaxf(amax, fabsf(x));
        }
        if (!(amax <= 65504.f))
            return fail(ctx, RNNT_ERR_ARG, "rnnt_finalize_weights: f16x3 cannot carry %s: largest |w| %.4g is above 65504; use bf16x3 or fp32", kv.first.c_str(), (double)amax);
        if (mag2 > 0.0 && sqrt(err2) > RNNT_F16X3_SPLIT_LIMIT * sqrt(mag2))
            return fail(ctx, RNNT_ERR_ARG, "rnnt_finalize_weights: f16x3 cannot carry %s: its two f16 planes miss it by %.3g of its r.m.s. magnitude "
                        "(largest |w| %.3g), above RNNT_F16X3_SPLIT_LIMIT %.3g; use bf16x3 or fp32", kv.first.c_str(), sqrt(err2 / mag2), (double)amax,
                        (double)RNNT_F16X3_SPLIT_LIMIT);
    }
    return RNNT_OK;
}

int rnnt_finalize_weights(rnnt_ctx* ctx, int32_t numerics_mode, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (numerics_mode != RNNT_NUMERICS_FP32 && numerics_mode != RNNT_NUMERICS_BF16X3 && numerics_mode != RNNT_NUMERICS_BF16 &&
        numerics_mode != RNNT_NUMERICS_F16X3)
        return fail(ctx, RNNT_ERR_ARG, "unsupported numerics mode %d", numerics_mode);
    if (numerics_mode == RNNT_NUMERICS_F16X3) {
        const int rc = f16x3_refusal(ctx);               // before anything of the context changes: a refused call leaves it as it was
        if (rc) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->cfg.device));
    // everything that caches pointers into the weight blob dies here: wavefront descriptor tables and the captured decode
    // graphs (their kernel arguments hold blob addresses)
    ctx->wf_key.clear(); ctx->lm_key.clear();
    for (auto& g : ctx->dec_graphs) (void)hipGraphExecDestroy(g.exec);
    ctx->dec_graphs.clear();
    const int V = ctx->cfg.vocab_size;
    std::vector<float> blob;
    std::vector<std::pair<const float**, size_t>> fix;   // pointer slots to patch with blob offsets
    auto need = [&](const std::string& name, std::initializer_list<int64_t> dims) -> const HostTensor* {
        const HostTensor* t = find(ctx, name);
        if (!t) { fail(ctx, RNNT_ERR_STATE, "missing tensor %s", name.c_str()); return nullptr; }
        if (t->dims != std::vector<int64_t>(dims)) { fail(ctx, RNNT_ERR_SHAPE, "tensor %s has the wrong shape", name.c_str()); return nullptr; }
        return t;
    };
    auto put = [&](const float** slot, const float* data, size_t n) {
        while (blob.size() % 8) blob.push_back(0.f);   // 32-byte alignment of every tensor (16 bytes in the 16-bit planes)
        fix.push_back({slot, blob.size()});
        blob.insert(blob.end(), data, data + n);
    };
    auto putv = [&](const float** slot, const std::vector<float>& v) { put(slot, v.data(), v.size()); };
#define NEED(var, name, ...) const HostTensor* var = need(name, {__VA_ARGS__}); if (!var) return ctx->err.find("missing") != std::string::npos ? RNNT_ERR_STATE : RNNT_ERR_SHAPE

    // --- subsampling -------------------------------------------------------------------------
    NEED(c1w, "encoder.embed.conv.0.weight", D, 1, 3, 3);
    NEED(c1b, "encoder.embed.conv.0.bias", D);
    NEED(c2w, "encoder.embed.conv.2.weight", D, D, 3, 3);
    NEED(c2b, "encoder.embed.conv.2.bias", D);
    NEED(eow, "encoder.embed.out.0.weight", D, D * RNNT_FSUB);
    NEED(eob, "encoder.embed.out.0.bias", D);
    NEED(pe, "encoder.embed.pos_enc.pe", 1, RNNT_PE_LEN, D);
    NEED(ang, "encoder.after_norm.weight", D);
    NEED(anb, "encoder.after_norm.bias", D);
    {
        std::vector<float> w1t(9 * D);   // [kh*3+kw][c]
        for (int c = 0; c < D; ++c)
            for (int k = 0; k < 9; ++k) w1t[k * D + c] = c1w->data[c * 9 + k];
        putv(&ctx->conv1_wt, w1t);
        put(&ctx->conv1_b, c1b->data.data(), D);
        std::vector<float> w2((size_t)D * 2304);   // [co][kh][kw][ci]
        for (int co = 0; co < D; ++co)
            for (int ci = 0; ci < D; ++ci)
                for (int k = 0; k < 9; ++k) w2[(size_t)co * 2304 + k * D + ci] = c2w->data[((size_t)co * D + ci) * 9 + k];
        putv(&ctx->conv2_w, w2);
        put(&ctx->conv2_b, c2b->data.data(), D);
        std::vector<float> ew((size_t)D * RNNT_FSUB * D);   // column c*19+f -> f*256+c
        for (int n = 0; n < D; ++n)
            for (int c = 0; c < D; ++c)
                for (int f = 0; f < RNNT_FSUB; ++f) ew[(size_t)n * RNNT_FSUB * D + f * D + c] = eow->data[(size_t)n * RNNT_FSUB * D + c * RNNT_FSUB + f];
        putv(&ctx->emb_w, ew);
        put(&ctx->emb_b, eob->data.data(), D);
        put(&ctx->pe, pe->data.data(), (size_t)RNNT_PE_LEN * D);
        put(&ctx->after_g, ang->data.data(), D);
        put(&ctx->after_b, anb->data.data(), D);
    }
    // --- encoder layers ----------------------------------------------------------------------
    std::vector<float> lncg((size_t)L * D), lncb((size_t)L * D), glu0((size_t)L * D);
    for (int l = 0; l < L; ++l) {
        LayerW& w = ctx->lw[l];
        const std::string p = "encoder.encoders." + std::to_string(l) + ".";
        auto vec = [&](const float** slot, const std::string& nm, std::initializer_list<int64_t> dims) -> int {
            const HostTensor* t = need(p + nm, dims);
            if (!t) return -1;
            put(slot, t->data.data(), t->data.size());
            return 0;
        };
#define VEC(slot, nm, ...) if (vec(&w.slot, nm, {__VA_ARGS__})) return RNNT_ERR_STATE
        VEC(ln_ffm_g, "norm_ff_macaron.weight", D); VEC(ln_ffm_b, "norm_ff_macaron.bias", D);
        VEC(w1m, "feed_forward_macaron.w_1.weight", FF, D); VEC(b1m, "feed_forward_macaron.w_1.bias", FF);
        VEC(w2m, "feed_forward_macaron.w_2.weight", D, FF); VEC(b2m, "feed_forward_macaron.w_2.bias", D);
        VEC(ln_mha_g, "norm_mha.weight", D); VEC(ln_mha_b, "norm_mha.bias", D);
        VEC(wq, "self_attn.linear_q.weight", D, D); VEC(bq, "self_attn.linear_q.bias", D);
        VEC(wk, "self_attn.linear_k.weight", D, D); VEC(bk, "self_attn.linear_k.bias", D);
        VEC(wv, "self_attn.linear_v.weight", D, D); VEC(bv, "self_attn.linear_v.bias", D);
        VEC(wo, "self_attn.linear_out.weight", D, D); VEC(bo, "self_attn.linear_out.bias", D);
        VEC(pu, "self_attn.pos_bias_u", RNNT_H, DK); VEC(pv, "self_attn.pos_bias_v", RNNT_H, DK);
        VEC(wpos, "self_attn.linear_pos.weight", D, D);
        VEC(ln_conv_g, "norm_conv.weight", D); VEC(ln_conv_b, "norm_conv.bias", D);
        VEC(pw2, "conv_module.pointwise_conv2.weight", D, D, 1); VEC(bpw2, "conv_module.pointwise_conv2.bias", D);
        VEC(bdw, "conv_module.depthwise_conv.bias", D);
        VEC(ln_ff_g, "norm_ff.weight", D); VEC(ln_ff_b, "norm_ff.bias", D);
        VEC(w1, "feed_forward.w_1.weight", FF, D); VEC(b1, "feed_forward.w_1.bias", FF);
        VEC(w2, "feed_forward.w_2.weight", D, FF); VEC(b2, "feed_forward.w_2.bias", D);
        VEC(ln_fin_g, "norm_final.weight", D); VEC(ln_fin_b, "norm_final.bias", D);
#undef VEC
        NEED(p1w, p + "conv_module.pointwise_conv1.weight", 2 * D, D, 1);
        NEED(p1b, p + "conv_module.pointwise_conv1.bias", 2 * D);
        NEED(dww, p + "conv_module.depthwise_conv.weight", D, 1, RNNT_KDW);
        NEED(bng, p + "conv_module.norm.weight", D);
        NEED(bnb, p + "conv_module.norm.bias", D);
        NEED(bnm, p + "conv_module.norm.running_mean", D);
        NEED(bnv, p + "conv_module.norm.running_var", D);
        // GLU pairs interleaved: row 2j = value row j, row 2j+1 = gate row 256+j (F.glu dim=1, convolution.py:139)
        std::vector<float> p1((size_t)2 * D * D), p1bi(2 * D);
        for (int j = 0; j < D; ++j) {
            memcpy(&p1[(size_t)(2 * j) * D], &p1w->data[(size_t)j * D], D * sizeof(float));
            memcpy(&p1[(size_t)(2 * j + 1) * D], &p1w->data[(size_t)(D + j) * D], D * sizeof(float));
            p1bi[2 * j] = p1b->data[j];
            p1bi[2 * j + 1] = p1b->data[D + j];
            glu0[(size_t)l * D + j] = p1b->data[j] * (1.0f / (1.0f + expf(-p1b->data[D + j])));
        }
        putv(&w.pw1, p1);
        putv(&w.bpw1, p1bi);
        std::vector<float> dwt((size_t)RNNT_KDW * D), bs(D), bt(D);
        for (int c = 0; c < D; ++c) {
            for (int k = 0; k < RNNT_KDW; ++k) dwt[(size_t)k * D + c] = dww->data[(size_t)c * RNNT_KDW + k];
            // BatchNorm1d eval: y = (x - mean) / sqrt(var + eps) * gamma + beta  ->  x*s + t
            const float inv = 1.0f / sqrtf(bnv->data[c] + 1e-5f);
            bs[c] = bng->data[c] * inv;
            bt[c] = bnb->data[c] - bnm->data[c] * bs[c];
        }
        putv(&w.wdw_t, dwt);
        putv(&w.bn_s, bs);
        putv(&w.bn_t, bt);
        const HostTensor* g = find(ctx, p + "norm_conv.weight");
        const HostTensor* b = find(ctx, p + "norm_conv.bias");
        memcpy(&lncg[(size_t)l * D], g->data.data(), D * sizeof(float));
        memcpy(&lncb[(size_t)l * D], b->data.data(), D * sizeof(float));
    }
    putv(&ctx->ln_conv_g_all, lncg);
    putv(&ctx->ln_conv_b_all, lncb);
    putv(&ctx->glu0, glu0);
    // --- predictor / joint ---------------------------------------------------------------------
    NEED(emb, "predictor.embed.weight", V, D);
    NEED(wih, "predictor.rnn.weight_ih_l0", 4 * D, D);
    NEED(whh, "predictor.rnn.weight_hh_l0", 4 * D, D);
    NEED(bih, "predictor.rnn.bias_ih_l0", 4 * D);
    NEED(bhh, "predictor.rnn.bias_hh_l0", 4 * D);
    NEED(wpr, "predictor.projection.weight", D, D);
    NEED(bpr, "predictor.projection.bias", D);
    NEED(wen, "joint.enc_ffn.weight", D, D);
    NEED(ben, "joint.enc_ffn.bias", D);
    NEED(wpf, "joint.pred_ffn.weight", D, D);
    NEED(bpf, "joint.pred_ffn.bias", D);
    NEED(wou, "joint.ffn_out.weight", V, D);
    NEED(bou, "joint.ffn_out.bias", V);
    {
        // gate rows interleaved: row 4j+g = torch row g*256+j (gate order i,f,g,o)
        std::vector<float> hh((size_t)4 * D * D), ih((size_t)4 * D * D), bb(4 * D);
        for (int j = 0; j < D; ++j)
            for (int g = 0; g < 4; ++g) {
                memcpy(&hh[(size_t)(4 * j + g) * D], &whh->data[(size_t)(g * D + j) * D], D * sizeof(float));
                memcpy(&ih[(size_t)(4 * j + g) * D], &wih->data[(size_t)(g * D + j) * D], D * sizeof(float));
                bb[4 * j + g] = bih->data[g * D + j] + bhh->data[g * D + j];
            }
        putv(&ctx->whh_il, hh);
        putv(&ctx->wih_il, ih);
        putv(&ctx->b_lstm_il, bb);
        put(&ctx->pred_embed, emb->data.data(), emb->data.size());
        put(&ctx->wpr, wpr->data.data(), wpr->data.size()); put(&ctx->bpr, bpr->data.data(), D);
        put(&ctx->wenc, wen->data.data(), wen->data.size()); put(&ctx->benc, ben->data.data(), D);
        put(&ctx->wpf, wpf->data.data(), wpf->data.size()); put(&ctx->bpf, bpf->data.data(), D);
        put(&ctx->wout, wou->data.data(), wou->data.size()); put(&ctx->bout, bou->data.data(), V);
        // greedy decode only needs pred_ffn(projection(h)): fold the two Linears (joint.py:54, predictor.py:205) into
        // W_c = W_pf * W_pr, b_c = W_pf * b_pr + b_pf (accumulated in double, stored in float32)
        std::vector<float> wc((size_t)D * D), bc(D);
        for (int n = 0; n < D; ++n) {
            for (int k = 0; k < D; ++k) {
                double acc = 0.0;
                for (int j = 0; j < D; ++j) acc += (double)wpf->data[(size_t)n * D + j] * (double)wpr->data[(size_t)j * D + k];
                wc[(size_t)n * D + k] = (float)acc;
            }
            double acc = bpf->data[n];
            for (int j = 0; j < D; ++j) acc += (double)wpf->data[(size_t)n * D + j] * (double)bpr->data[j];
            bc[n] = (float)acc;
        }
        putv(&ctx->wjc, wc);
        putv(&ctx->bjc, bc);
        const HostTensor* cw = find(ctx, "ctc_head.ctc_lo.weight");
        const HostTensor* cb = find(ctx, "ctc_head.ctc_lo.bias");
        ctx->wctc = ctx->bctc = nullptr;
        if (cw && cb && cw->dims == std::vector<int64_t>{V, D} && cb->dims == std::vector<int64_t>{V}) {
            put(&ctx->wctc, cw->data.data(), cw->data.size());
            put(&ctx->bctc, cb->data.data(), V);
        }
    }
#undef NEED
    // upload (the allocation is kept when the size is unchanged: a reload of the same architecture re-copies in place)
    while (blob.size() % 8) blob.push_back(0.f);
    int rc;
    if (ctx->blob.cap != blob.size()) {
        HIPCHK(hipStreamSynchronize(s));
        ctx->blob_hi.release();   // the planes have the blob's size; allocated below when the mode reads them
        ctx->blob_lo.release();
        if ((rc = reserve_exact(ctx, ctx->blob, blob.size()))) return rc;
    }
    HIPCHK(hipMemcpyAsync(ctx->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice, s));
    for (auto& f : fix) *f.first = ctx->blob + f.second;
    ctx->numerics = RNNT_NUM_F32;   // the derived tables below are always exact f32
    if (numerics_mode != RNNT_NUMERICS_FP32) {
        // hi / lo 16-bit planes of every weight, same element index as the blob (gemm_bf reads them through GemmP::Wh / Wl)
        if ((rc = reserve(ctx, ctx->blob_hi, blob.size()))) return rc;
        if ((rc = reserve(ctx, ctx->blob_lo, blob.size()))) return rc;
        const long long n8 = (long long)(blob.size() / 8);
        if (numerics_mode == RNNT_NUMERICS_F16X3) hipLaunchKernelGGL(split_planes<true>, dim3(grid_for(n8)), dim3(256), 0, s, ctx->blob, ctx->blob_hi, ctx->blob_lo, n8);
        else hipLaunchKernelGGL(split_planes<false>, dim3(grid_for(n8)), dim3(256), 0, s, ctx->blob, ctx->blob_hi, ctx->blob_lo, n8);
        LAUNCHCHK("split_planes");
    }
    // fragment-major packed layer weights for the fused block kernels, in the requested mode (rnnt_fused.hip.h)
    {
        const int nm = numerics_mode;
        const size_t per_w = nm == RNNT_NUMERICS_BF16 ? 8 : 4;              // weights per 16-byte vector
        const size_t layer_w = (size_t)4 * FF * D + 5 * D * D + 2 * D * D;   // w1m w2m w1 w2 | wq wk wv wo pw2 | pw1
        const size_t vecs = ((size_t)L * layer_w + (size_t)D * 2304) / per_w;          // + conv2 [256][2304] for gemm_bw
        if (ctx->fuse_w.cap != vecs) {
            HIPCHK(hipStreamSynchronize(s));
            if ((rc = reserve_exact(ctx, ctx->fuse_w, vecs))) return rc;
        }
        if ((rc = reserve(ctx, ctx->layers_dev, (size_t)L))) return rc;
        std::vector<LayerDev> ld(L);
        uint4* cur = ctx->fuse_w;
        auto pack = [&](const float* W, int N, int K) -> const uint4* {
            const uint4* out = cur;
            const long long total = (long long)((N + 15) / 16) * (K / 32) * 64;
            const dim3 g(grid_for(total)), b(256);
            switch (nm) {
                case RNNT_NUMERICS_BF16X3: hipLaunchKernelGGL(pack_frag<RNNT_NUM_BF16X3>, g, b, 0, s, W, N, K, K, cur); break;
                case RNNT_NUMERICS_BF16: hipLaunchKernelGGL(pack_frag<RNNT_NUM_BF16>, g, b, 0, s, W, N, K, K, cur); break;
                case RNNT_NUMERICS_F16X3: hipLaunchKernelGGL(pack_frag<RNNT_NUM_F16X3>, g, b, 0, s, W, N, K, K, cur); break;
                default: hipLaunchKernelGGL(pack_frag<RNNT_NUM_F32>, g, b, 0, s, W, N, K, K, cur); break;
            }
            cur += (size_t)N * K / per_w;
            return out;
        };
        for (int l = 0; l < L; ++l) {
            const LayerW& w = ctx->lw[l];
            LayerDev& d = ld[l];
            d.w1m = pack(w.w1m, FF, D); d.w2m = pack(w.w2m, D, FF); d.wq = pack(w.wq, D, D); d.wk = pack(w.wk, D, D); d.wv = pack(w.wv, D, D);
            d.wo = pack(w.wo, D, D); d.pw1 = pack(w.pw1, 2 * D, D); d.pw2 = pack(w.pw2, D, D); d.w1 = pack(w.w1, FF, D); d.w2 = pack(w.w2, D, FF);
            d.b1m = w.b1m; d.b2m = w.b2m; d.bq = w.bq; d.bk = w.bk; d.bv = w.bv; d.bo = w.bo; d.bpw1 = w.bpw1; d.bpw2 = w.bpw2; d.b1 = w.b1; d.b2 = w.b2;
            d.ln_ffm_g = w.ln_ffm_g; d.ln_ffm_b = w.ln_ffm_b; d.ln_mha_g = w.ln_mha_g; d.ln_mha_b = w.ln_mha_b; d.ln_conv_g = w.ln_conv_g;
            d.ln_conv_b = w.ln_conv_b; d.ln_ff_g = w.ln_ff_g; d.ln_ff_b = w.ln_ff_b; d.ln_fin_g = w.ln_fin_g; d.ln_fin_b = w.ln_fin_b;
            d.wdw_t = w.wdw_t; d.bdw = w.bdw; d.bn_s = w.bn_s; d.bn_t = w.bn_t;
            d.kc = ctx->kcache + (size_t)l * ctx->cfg.max_streams * ctx->tcap * D;
            d.vc = ctx->vcache + (size_t)l * ctx->cfg.max_streams * ctx->tcap * D;
            d.gr = ctx->gring + (size_t)l * ctx->cfg.max_streams * ctx->cap * D;
            d.xr = ctx->xring + (size_t)l * ctx->cfg.max_streams * ctx->cap * D;
        }
        ctx->conv2_wp = pack(ctx->conv2_w, D, 2304);
        LAUNCHCHK("pack_frag");
        HIPCHK(hipMemcpyAsync(ctx->layers_dev, ld.data(), L * sizeof(LayerDev), hipMemcpyHostToDevice, s));
        ctx->layers_host = ld;
        HIPCHK(hipStreamSynchronize(s));   // ld dies at scope end
    }
    // joint.ffn_out in the lattice kernel's ring order (rnnt_joint.hip.h): one 1-KiB piece per MFMA operand
    if (numerics_mode != RNNT_NUMERICS_FP32 && V <= JR_NT * 16 && V % 4 == 0) {
        const bool lo = numerics_mode != RNNT_NUMERICS_BF16;
        const size_t bytes = (size_t)(lo ? 16 : 8) * JR_SLOT;
        if (ctx->joint_wfrag.cap != bytes) {
            HIPCHK(hipStreamSynchronize(s));
            if ((rc = reserve_exact(ctx, ctx->joint_wfrag, bytes))) return rc;
        }
        if ((rc = reserve(ctx, ctx->joint_counter, (size_t)4))) return rc;
        const dim3 g((unsigned)(bytes / 16 + 255) / 256), b(256);
        if (numerics_mode == RNNT_NUMERICS_F16X3) hipLaunchKernelGGL((pack_joint_w<true, true>), g, b, 0, s, ctx->wout, (int)V, ctx->joint_wfrag);
        else if (lo) hipLaunchKernelGGL((pack_joint_w<false, true>), g, b, 0, s, ctx->wout, (int)V, ctx->joint_wfrag);
        else hipLaunchKernelGGL((pack_joint_w<false, false>), g, b, 0, s, ctx->wout, (int)V, ctx->joint_wfrag);
        LAUNCHCHK("pack_joint_w");
    }
    // derived tables on the device: P_l = pe * W_pos^T (attention.py:396, batch-invariant), input-gate
    // table E = embed * W_ih^T + b_ih + b_hh (predictor.py:200,204)
    for (int l = 0; l < L; ++l) {
        if ((rc = reserve(ctx, ctx->ptab[l], (size_t)RNNT_PE_LEN * D))) return rc;
        ctx->lw[l].ptab = ctx->ptab[l];
        GemmP g = plain_gemm(ctx->pe, D, ctx->lw[l].wpos, D, nullptr, ctx->lw[l].ptab, D, RNNT_PE_LEN, D, D);
        if ((rc = launch_gemm(ctx, s, &g, 1))) return rc;
    }
    if ((rc = reserve(ctx, ctx->egate, (size_t)V * 4 * D))) return rc;
    {
        GemmP g = plain_gemm(ctx->pred_embed, D, ctx->wih_il, D, ctx->b_lstm_il, ctx->egate, 4 * D, V, 4 * D, D);
        if ((rc = launch_gemm(ctx, s, &g, 1))) return rc;
    }
    HIPCHK(hipStreamSynchronize(s));
    ctx->numerics = numerics_mode;
    ctx->finalized = true;
    return RNNT_OK;
}

int rnnt_streams_reset(rnnt_ctx* ctx, int32_t n_streams, void* stream) {
    if (!ctx) return RNNT_ERR_ARG;
    if (!ctx->finalized) return fail(ctx, RNNT_ERR_STATE, "weights not finalized");
    if (n_streams < 1 || n_streams > ctx->cfg.max_streams) return fail(ctx, RNNT_ERR_ARG, "n_streams %d out of range", n_streams);
    hipStream_t s = (hipStream_t)stream;
    const int B = ctx->cfg.max_streams;
    ctx->n_streams = n_streams;
    ctx->pos = SlotPos{0, 0, 0};
    ctx->frames_buffered = 0; ctx->frames_decoded = 0;
    ctx->launches = 0; ctx->greedy_steps = 0;
    ctx->pool_mode = false;                      // all slots share one position again
    for (PoolSlot& q : ctx->slot) q.pos = SlotPos{0, 0, 0};
    hipLaunchKernelGGL(conv_ring_init, dim3(grid_for((long long)L * B * ctx->cap * D)), dim3(256), 0, s, ctx->gring, ctx->xring, ctx->glu0, B, ctx->cap);
    LAUNCHCHK("conv_ring_init");
    hipLaunchKernelGGL(decode_state_reset, dim3(grid_for((long long)2 * B * D)), dim3(256), 0, s, ctx->h, ctx->c, ctx->sel, ctx->key, ctx->fidx, ctx->nsym,
                       ctx->count, ctx->n_active, ctx->tok, ctx->cfg.blank_id, B);
    LAUNCHCHK("decode_state_reset");
    if (ctx->max_rows > 0) {   // one empty hypothesis per stream with the zero LSTM state (online_rnnt_model.py:407-415)
        ctx->beams.assign(n_streams, std::vector<rnnt_ctx::Hyp>(1, rnnt_ctx::Hyp{{}, 0.0}));
        ctx->pool_cur = 0;
        HIPCHK(hipMemsetAsync(ctx->pool[0], 0, (size_t)ctx->max_rows * (ctx->cfg.n_steps + 1) * 512 * sizeof(float), s));
    }
    return pool_slot_reset(ctx, s, 0, B);   // the per-slot states of the stream pool
}
