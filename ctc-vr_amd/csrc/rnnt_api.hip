// librnnt_hip.so — host side: context, weight ingest/packing, per-chunk launch sequences, C ABI.
// See include/rnnt_hip.h for the contract and DESIGN.md for the data layout in HBM.
#include "rnnt_kernels.hip.h"
#include "../../include/rnnt_hip.h"

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <algorithm>
#include <array>
#include <atomic>
#include <vector>

namespace {

constexpr int D = RNNT_D, FF = RNNT_FF, L = RNNT_L, DK = RNNT_DK;
constexpr int BIG = INT_MAX;

struct LayerW {
    const float *ln_ffm_g, *ln_ffm_b, *w1m, *b1m, *w2m, *b2m;
    const float *ln_mha_g, *ln_mha_b, *wq, *bq, *wk, *bk, *wv, *bv, *wo, *bo, *pu, *pv;
    float* ptab;   // [5000][256] = pe * W_pos^T (view of rnnt_ctx::ptab)
    const float *wpos;
    const float *ln_conv_g, *ln_conv_b, *pw1, *bpw1, *wdw_t, *bdw, *bn_s, *bn_t, *pw2, *bpw2;
    const float *ln_ff_g, *ln_ff_b, *w1, *b1, *w2, *b2, *ln_fin_g, *ln_fin_b;
};

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> dims;
};

// One chunk of a call: fbank frames, t' new encoder frames, key window [kv_row0, kv_row0 + T2), first positional row, ring frame count,
// and where its frames go (fpos: frame buffer, xoff: x rows).
struct ChunkInfo {
    int len, tq, T2, kv_row0, pos_start, ring_pos, fpos; size_t xoff;
    int kv_w0() const { return kv_row0 + T2 - tq; }   // the row its new K/V rows are appended at
};

// A stream's position in the reference's chunk loop (encoder.py:254-264,288).  The lock-step entry points share one (rnnt_ctx::pos),
// every slot of the stream pool has its own; every entry point plans a chunk and moves on through these two methods.
struct SlotPos {
    int cache_len, kv_start, conv_pos;
    // the windows of a chunk of tq new frames at `offset`; false (err: the bound it breaks) when they leave the positional table or the K/V buffer
    bool plan(int tq, int offset, int tcap, ChunkInfo& out, std::string& err) const {
        out.tq = tq;
        out.T2 = cache_len + tq;               // attention_key_size (encoder.py:256)
        out.pos_start = offset - cache_len;    // encoder.py:257
        out.kv_row0 = kv_start;
        out.ring_pos = conv_pos;
        const bool in_table = out.pos_start >= 0 && out.pos_start + out.T2 <= RNNT_PE_LEN, in_cache = kv_start + out.T2 <= tcap;
        if (!in_table) err = "positional window [" + std::to_string(out.pos_start) + ", " + std::to_string(out.pos_start + out.T2) + ") outside the 5000-entry table";
        else if (!in_cache) err = "K/V cache capacity " + std::to_string(tcap) + " exceeded";
        return in_table && in_cache;
    }
    // the cache truncation after a chunk with T2 keys (encoder.py:259-264); an empty cache re-bases its window at row 0
    void advance(int T2, int tq, int required) {
        const int next_start = required < 0 ? 0 : (required == 0 ? T2 : (T2 - required > 0 ? T2 - required : 0));
        kv_start += next_start;
        cache_len = T2 - next_start;
        if (cache_len == 0) kv_start = 0;
        conv_pos += tq;
    }
};

// the launches of a wavefront stage (rnnt_ctx::WfLaunch): the eight GEMM shape classes first (they index wf_run_stage's shape table)
// ContextGraph of the CTC prefix beam search (api_ctc_prefix.hip.inc) as flat tables: node ids in creation order, root = 0
struct CtxGraph {
    std::vector<int> token, is_end, fail, output, off, ctok, cid;
    std::vector<double> tscore, nscore, oscore;
};

// Back-off n-gram model of the CTC prefix beam search (api_ngram.hip.inc) as flat tables, prescaled: node ids in list order, root = 0
struct NgModel {
    std::vector<int> fail, off, ctok, cid, root;
    std::vector<double> W, B;
    double U = 0.0;
    int start = 0, eos = -1;
    NgTables tables() const {
        NgTables g;
        g.fail = fail.data(); g.off = off.data(); g.ctok = ctok.data(); g.cid = cid.data(); g.root = root.data(); g.W = W.data(); g.B = B.data();
        g.U = U; g.start = start; g.eos = eos;
        return g;
    }
};

// Device bytes currently held through DevBuf owners, process-wide (rnnt_live_device_bytes).
std::atomic<int64_t> live_device_bytes{0};

// Owner of one allocation -- device memory, or pinned host memory when HOST: a pointer and its capacity in elements, freed by the
// destructor.  It converts to T*, so launches, copies and pointer arithmetic read as with a raw pointer.  Allocation goes through
// reserve / reserve_exact (host_launch.hip.inc); release() is the only place memory is given back.
template <typename T, bool HOST = false>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && HOST) (void)hipHostFree(p);
        else if (p) { (void)hipFree(p); live_device_bytes -= (int64_t)(cap * sizeof(T)); }
        p = nullptr;
        cap = 0;
    }
    operator T*() const { return p; }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

// Per slot of the stream pool, on the host.  SearchSlot, a prefix search carried across calls: the frames walked, and what its first
// advancing call fixed until the next reset -- beam (0: fresh), the two weights (0 for the CTC search), use_context, the graph
// generation (rnnt_ctx::cg_gen); either search also use_ngram and the model generation (rnnt_ctx::ng_gen).  WvSlot, the front-end: samples received and frames emitted since the reset, the (sample_rate,
// n_fft) its first push fixed (n_fft == 0: fresh), whether its utterance has ended.  HsSlot, the frame history: flag and length.
// ep: endpoint detection is on (the config and the counters live on the device, api_pool_endpoint.hip.inc).  SegSlot, the segment
// record (api_pool_segment.hip.inc): segments started since the slot was opened, the encoder frames it had encoded when the current
// one began, and those encoded since it was opened (the encoder position does not say: a fresh segment restarts it).
struct SearchSlot { int frames_done, beam; float cw, tw; int use_context; int64_t gen; int use_ngram; int64_t ngen; };
struct WvSlot { int samples, frames, rate, nfft, finished; };
struct HsSlot { int keep, len; };
struct SegSlot { int index, start, frames; };
// One record per slot (rnnt_ctx::slot, sized to max_streams by rnnt_create; pool_slot_reset makes slots fresh): the position, the
// current buffer set of the beam and of the transducer prefix search, a host upper bound of the beam's longest hypothesis.
struct PoolSlot {
    SlotPos pos{0, 0, 0};
    int beam_cur = 0, beam_lbound = 0, prefix_cur = 0;
    SearchSlot ctc{}, prefix{};
    WvSlot wave{};
    HsSlot hist{};
    int ep = 0;
    SegSlot seg{};
};
// The table of one pool call: ints filled in pinned memory and sent by ONE async copy; the event says the copy has left the pinned
// buffer, so the next call may fill it again (calltab_alloc / calltab_fill / calltab_send, host_launch.hip.inc).
struct CallTab {
    DevBuf<int> dev;
    PinnedBuf<int> host;
    hipEvent_t ev = nullptr;
    ~CallTab() { if (ev) (void)hipEventDestroy(ev); }
    operator int*() const { return dev.p; }
};

enum WfType { WF_FFN1M, WF_FFN2M, WF_QKV, WF_OUT, WF_PW1, WF_PW2, WF_FFN1, WF_FFN2, WF_ATTN, WF_DW, WF_LN, WF_BLOCK_FRONT, WF_BLOCK_BACK };

}  // namespace

struct rnnt_ctx {
    rnnt_config cfg;
    std::string err;
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    int numerics = 0;

    // packed weights (one device blob)
    DevBuf<float> blob;
    DevBuf<unsigned short> blob_hi, blob_lo;                 // 16-bit hi / lo planes of the blob (split-operand numerics modes)
    // fused Conformer-block kernels (rnnt_fused.hip.h): fragment-major packed layer weights of the current numerics mode and
    // the per-layer pointer table in device memory
    DevBuf<uint4> fuse_w;
    DevBuf<LayerDev> layers_dev;
    const uint4* conv2_wp = nullptr;          // fragment-major packed conv2 weights of the current numerics mode (gemm_bw)
    DevBuf<unsigned char> joint_wfrag;        // joint.ffn_out as the LDS-DMA ring's stage stream (pack_joint_w), split modes and bf16
    DevBuf<int> joint_counter;                // joint_lattice_rows' dynamic row-tile queue (zeroed before every launch)
    std::map<const void*, int> dyn_lds;       // kernels whose dynamic-LDS limit was raised for THIS context's device (ensure_dyn_lds)
    std::vector<LayerDev> layers_host;        // host copy (packed-weight pointers for gemm_as / ffn_as launches)
    int use_as = 1;                            // RNNT_AS=0: LDS-tiled gemm_bf for every layer contraction of the layer-major schedule
    int use_fused = 1;                         // RNNT_FUSED=0: the unfused wavefront (11 launches per stage)
    DevBuf<FuseItem> wf_ftab;
    int wf_fused_plan = 0;                     // the cached plan (wf_key) was built for the fused schedule
    LayerW lw[L];
    DevBuf<float> ptab[L];                     // LayerW::ptab
    const float *conv1_wt, *conv1_b, *conv2_w, *conv2_b, *emb_w, *emb_b, *pe, *after_g, *after_b;
    const float *ln_conv_g_all, *ln_conv_b_all, *glu0;
    const float *whh_il, *wih_il, *b_lstm_il, *pred_embed, *wpr, *bpr, *wenc, *benc, *wpf, *bpf, *wout, *bout;
    DevBuf<float> egate;      // [vocab][1024] interleaved input-gate table

    // geometry
    int tmax = 0, t1max = 0, cap = 0, tcap = 0, fcap = 0, fstride = 0, vpad = 0;
    // activations
    DevBuf<float> y1, y2, x, hbuf, qbuf, abuf, dbuf;
    DevBuf<float> kcache, vcache, gring, xring;
    DevBuf<float> encbuf, encp;
    // decode state
    // LSTM state: two buffers [2][B][256] per h and c; sel[b] says which one is committed, the other receives the candidate
    DevBuf<float> h, c, pred, z, logits;
    DevBuf<int> tok, fidx, nsym, count, tokens, n_active, klen, sel;
    DevBuf<unsigned long long> key;
    DevBuf<int> dec_ctrl;      // persistent decoder control block: [0] frames_ready, [1] error, [2] evaluations, [4] abort word of greedy_multi
    int use_persistent = 1;
    int attn_stream = 1;       // RNNT_ATTN_STREAM=0: LDS-tiled attention kernel for every chunk
    int fuse_after_norm = 1;   // RNNT_FUSE_AFTER_NORM=0: keep after_norm as its own launch in the pipelined greedy path
    int overlap_ok = -1;       // -1 not probed; 1: kernels of the decode stream run concurrently with the caller's stream
    int use_multi = 1;         // RNNT_DEC_MULTI=0: one CU per stream (greedy_stream) instead of greedy_multi (4 CUs per stream)
    int n_cus = 0;
    DevBuf<unsigned long long> gm_x1, gm_xa;  // greedy_multi mailboxes
    DevBuf<long long> gm_dbg;                 // [max_streams][GM_DBG_W] greedy_multi phase timers (RNNT_GM_DBG=1)
    int gm_dbg_rows = 0;                      // stream groups of the last greedy_multi launch that wrote them
    const float *wjc = nullptr, *bjc = nullptr;   // folded joint.pred_ffn o predictor.projection
    const float *wctc = nullptr, *bctc = nullptr; // ctc_head.ctc_lo (optional)
    // beam search: state pools [rows][n_steps+1][512] (ping-pong), per-row buffers
    int max_rows = 0;
    DevBuf<float> pool[2], bpred, bz, blogits, b_blank, b_toplp;
    DevBuf<int> b_tok, b_frame, b_active, b_steps, b_toptok, b_srcrow, b_srcstep;
    int pool_cur = 0;
    PinnedBuf<int> pinned;   // host-pinned scratch (n_active read-back)
    DevBuf<float> scratch;   // device scratch for getters / step API

    // stream state (all streams lock step)
    int n_streams = 0;
    SlotPos pos{0, 0, 0};
    int frames_buffered = 0, frames_decoded = 0;
    int64_t launches = 0, greedy_steps = 0;
    // stream pool (api_pool.hip.inc): once rnnt_stream_open or rnnt_pool_chunk has run, every slot has its own position (slot[b].pos)
    // and `pos` above is dead until the next rnnt_streams_reset.  Positions are host integers advanced by the reference's bookkeeping
    // (encoder.py:254-264) and mirrored per call into ONE device table: n PoolRow entries, the n slot indices the decoder reads and
    // the current buffer set per active row of a search that has two ([max_streams] (POOL_ROW_INTS + 2) ints).
    std::vector<PoolSlot> slot;
    bool pool_mode = false;
    CallTab pool_tab;
    int gemm_m_cap = 0;                        // > 0 during a pool call: GEMM kernels / tiles are chosen as for at most this many rows
    // wavefront (whole-utterance) path: per-chunk x rows, per-layer scratch, subsampling slabs, descriptor tables
    DevBuf<float> wf_x, wf_h, wf_q, wf_a, wf_d, wf_y1, wf_y2;
    int wf_slab = 0;
    DevBuf<int> wf_starts;
    DevBuf<GemmP> wf_gtab; DevBuf<AttnP> wf_atab; DevBuf<DwP> wf_dtab; DevBuf<LnP> wf_ltab;
    hipStream_t dec_stream = nullptr;          // decode runs here while the encoder wavefront runs on the caller's stream
    hipStream_t sub_stream = nullptr;          // subsampling slabs
    int wf_sub_async = 1;                      // RNNT_WF_SUB_ASYNC=0: the wavefront's subsampling slabs on the caller's stream
    int wf_merge = 2;                          // RNNT_WF_MERGE (1..WF_MERGE_MAX): chunks of one layer per wavefront stage
    // descriptor tables of the last rnnt_encoder_chunks call, reused when the next call has the same plan and entry state
    struct WfLaunch { WfType type; int off, n, maxM, maxT2; };
    std::vector<WfLaunch> wf_seq;
    std::vector<std::array<int, 13>> wf_lstart;
    std::vector<int> wf_sc_first, wf_key;
    std::vector<hipEvent_t> ev_pool;           // events of a wavefront call (wf_buffers)
    // layer-major schedule (host_lm.hip.inc): activations over all B*F rows of a call, per-layer linear post-GLU rows, one
    // subsampling slab, attention block table (reused while the plan and the entry state stay the same)
    int use_lm = 1;                            // RNNT_LM=0: wavefront schedule for every whole-utterance call
    int lm_pw2_head = 2;                       // RNNT_LM_PW2_HEAD: 2 depthwise conv + pointwise_conv2 inside the FFN launch, 1 only pointwise_conv2, 0 three launches
    int lm_ffn_merge = 0;                      // RNNT_LM_FFN_MERGE=1: one launch per layer boundary (better alone, worse with two batches in flight)
    int lm_qkv_tail = 1, lm_out_chain = 1;     // RNNT_LM_QKV_TAIL=0 / RNNT_LM_OUT_CHAIN=0: q/k/v and pointwise_conv1 as launches of their own
    int lm_side = 1;                           // RNNT_LM_SIDE=0: the tail chunk class's subsampling in line instead of on the side stream
    int attn_bf = 1;                           // RNNT_ATTN_BF=0: exact-f32 MFMA attention (rel_attention_lm_mfma) in every mode
    int attn_resident = 1;                     // RNNT_ATTN_RESIDENT=0: always the tiled rel_attention_lm_bf, never rel_attention_lm_res
    int conv1_fuse = 1;                        // RNNT_CONV1_FUSE=0: conv1_relu_rows + gemm_bw over the y1 slab, never gemm_bw_c1
    // launch-form knobs, read at rnnt_create like the ones above (a process can hold contexts of every value side by side)
    int ffn_nw = 8;                            // RNNT_FFN_NW: waves per ffn_as workgroup, 4 / 8 / 16 (anything else: 8)
    int gemm_pd = 2;                           // RNNT_GEMM_PD=1: one K block in flight per gemm_ns / gemm_ns_tab workgroup instead of two
    int conv2_bw = 1;                          // RNNT_CONV2_BW=0: conv2 never on gemm_bw / gemm_bw_c1 (launch_gemm's tiles at every M)
    int conv1_rows = 1;                        // RNNT_CONV1_ROWS=0: conv1_relu at every shape, never conv1_relu_rows
    int conv2_lds = 1;                         // RNNT_CONV2_LDS: exact-f32 conv2 of >= 2048 rows: 0 launch_gemm, 1 gemm_ns<2,2>, 2 non-temporal A (nc > 1)
    int bw_nw = 8;                             // RNNT_BW_NW=4: gemm_bw / gemm_bw_c1 with 4 waves (anything but 8 selects 4)
    int gemm_ns = 1;                           // RNNT_GEMM_NS=0: exact-f32 stage GEMMs on gemm16_tab whatever the number of descriptors
    int ns_min_groups = 2;                     // RNNT_NS_MIN_GROUPS: fewest descriptors of a stage GEMM that go to gemm_ns_tab
    int xcd_x = 0;                             // RNNT_XCD_X = 1 / 2 / 4 / 8: XCDs per descriptor of the table GEMMs' 1-D grids (else chosen per launch)
    int fuse_merge = FUSE_MAXC;                // RNNT_FUSE_MERGE: chunks of one layer per fused wavefront stage, clamped to 1..FUSE_MAXC
    int fuse_frames = 12;                      // RNNT_FUSE_FRAMES: frames per stream of one fused tile (at most FUSE_MAXF)
    int attn_pair_major = 1;                   // RNNT_ATTN_PAIR_MAJOR=0: rel_attention_stream_tab's workgroups head-major instead of pair-major
    int dec_slack = 8;                         // RNNT_DEC_SLACK: graph decoder steps per wavefront stage beyond the stage's new frames
    int drain_steps = 4;                       // RNNT_DRAIN_STEPS: graph decoder steps per round of greedy_drain
    DevBuf<float> lm_x, lm_h, lm_q, lm_a, lm_d, lm_g, lm_y1, lm_y2;
    DevBuf<float> lm_y1b, lm_y2b;                  // slabs of the tail chunk class (subsampled on sub_stream beside the main class)
    hipEvent_t sub_ev[2] = {nullptr, nullptr};     // fork / join of the tail class on sub_stream
    // ragged batches (rnnt_decode_ragged): gathered tail frames, their subsampled rows, gather / scatter entries
    DevBuf<float> rg_fb, rg_xt;
    DevBuf<int2> rg_ent;
    DevBuf<LmBlock> lm_blocks;
    std::vector<LmBlock> lm_blocks_host;
    std::vector<int> lm_key;
    // rel_attention_lm_res tables (host_lm.hip.inc: lm_res_plan), rebuilt with the block table
    DevBuf<LmResHdr> lm_rhdr;
    DevBuf<LmRow> lm_rrows;
    std::vector<LmResHdr> lm_rhdr_host;
    std::vector<LmRow> lm_rrows_host;
    int lm_res_ok = 0, lm_res_stride = 0;
    // native beam bookkeeping (rnnt_beam_advance): per stream, hypotheses in device-row order
    struct Hyp { std::vector<int> tokens; double log_prob; };
    std::vector<std::vector<Hyp>> beams;
    int use_beam_chain = 1;    // RNNT_BEAM_CHAIN=0: launched extension steps (5 kernels + one host sync per step)
    // device-resident bookkeeping (rnnt_beam_decode): token lists [2][max_rows][bd_lcap] (ping-pong, grown on demand), per-row
    // lengths / scores / hashes [2][max_rows], hypotheses per stream and per-stream end frames [max_streams]
    DevBuf<int> bd_tok, bd_len, bd_nh, bd_fend;
    DevBuf<double> bd_sc;
    DevBuf<unsigned long long> bd_hs;
    // per-slot beam state of the stream pool (rnnt_pool_chunk_beam), separate from the lock-step state above and allocated on the
    // first beam call: hypothesis i of slot b is row b * max_beam + i of two buffer sets -- state pools, token lists
    // [2][max_rows][max_tokens], lengths / scores / hashes [2][max_rows] -- plus the hypotheses per slot.  Slots advance
    // independently, so the current set is per slot (PoolSlot::beam_cur, with beam_lbound).
    DevBuf<float> ps_pool[2];
    DevBuf<int> ps_tok, ps_len, ps_nh;
    DevBuf<double> ps_sc;
    DevBuf<unsigned long long> ps_hs;
    // feature front-end (rnnt_fbank): DFT / mel matrices for (fb_rate, fb_nfft) and work buffers
    DevBuf<float> fb_dft, fb_mel, fb_pad, fb_spec, fb_pow;
    int fb_rate = 0, fb_nfft = 0;
    // teacher-forced scoring (api_score.hip.inc): predictor outputs / LSTM ping-pong / internal pick lattice (sc_f), step tokens /
    // targets / lengths (sc_i), per-utterance results (sc_nll), and the materialised log-softmax lattice of the fallback path or
    // the CTC log-probabilities (sc_lat)
    DevBuf<float> sc_f, sc_lat;
    DevBuf<int> sc_i;
    DevBuf<double> sc_nll;
    // forced alignment (api_score.hip.inc): back-pointer words and the outputs of one call (best | nll | path)
    DevBuf<unsigned> al_bp;
    DevBuf<double> al_out;
    // prefix beam search (api_prefix.hip.inc), sized by B * beam rows and T + 1 tokens -- projected frames / CTC log-probabilities /
    // state pools / top-k values (pb_f), token lists / lengths / counts / top-k tokens (pb_i), scores and hashes (pb_d), and the
    // packed block of one call's results (pb_out)
    DevBuf<float> pb_f;
    DevBuf<int> pb_i;
    DevBuf<double> pb_d, pb_out;
    // CTC prefix beam search (api_ctc_prefix.hip.inc): the context graph of rnnt_context_set (host tables, device ints / doubles) and
    // the call's own buffers -- lengths, prefix and time arenas, packed results (cp_i), scores (cp_d), log-probabilities of
    // rnnt_ctc_prefix_beam_decode (cp_lp)
    CtxGraph cg;
    bool cg_on = false;
    DevBuf<int> cg_i, cp_i;
    DevBuf<double> cg_d, cp_d;
    DevBuf<float> cp_lp;
    // CTC prefix search per slot of the stream pool (api_pool_ctc.hip.inc), allocated on its first use: the hypothesis record of every
    // slot, the two arenas [max_streams][max_cache_frames * CP_MAX_BEAM + 1], the call's table (slot and frames walked per active
    // row, [max_streams] 2 ints), one read's packed block.  Host per slot: PoolSlot::ctc.  cg_gen counts rnnt_context_set calls.
    int64_t cg_gen = 0;
    DevBuf<CpSlotState> pc_state;
    DevBuf<int2> pc_parena, pc_tarena;
    CallTab pc_tab;
    DevBuf<double> pc_out;
    // n-gram model of rnnt_ngram_set (api_ngram.hip.inc): host tables, device ints (fail | off | ctok | cid | root) and doubles (W | B);
    // ng_gen counts rnnt_ngram_set calls.  rnnt_ngram_score's own buffers: lengths | tokens (ngs_i), step scores | totals (ngs_d).
    NgModel ng;
    bool ng_on = false;
    int64_t ng_gen = 0;
    DevBuf<int> ng_i, ngs_i;
    DevBuf<double> ng_d, ngs_d;
    // transducer prefix beam search per slot of the stream pool (api_pool_prefix.hip.inc), allocated on its first use: hypothesis i of
    // slot b is row b * PB_MAX_BEAM + i of two buffer sets -- states [rows][2][512], token lists [rows][max_cache_frames + 1],
    // lengths / scores / hashes [rows] -- plus the hypotheses per slot, the step's top-k [rows][PB_MAX_BEAM], the frames of one call
    // (projected, CTC log-probabilities; grow-only), the seam form's table (slot and current set per active row, [max_streams] 2 ints)
    // and one read's packed block.  Host per slot: PoolSlot::prefix and prefix_cur (slots advance independently).  A biased search
    // also keeps a context state and score per row (pp_cst / pp_cs), a search that fuses the n-gram model an n-gram state and score
    // (pp_nst / pp_ns).
    int prefix_group = 0;                      // RNNT_PREFIX_GROUP: 0 by the size of the launch, 1 / 4 hypotheses per prefix_step_pool workgroup always
    DevBuf<float> pp_pool[2], pp_toplp, pp_encp, pp_ctc;
    DevBuf<int> pp_tk[2], pp_len[2], pp_cst[2], pp_nst[2], pp_nh, pp_toptok;
    DevBuf<double> pp_sc[2], pp_cs[2], pp_ns[2], pp_out;
    DevBuf<unsigned long long> pp_hs[2];
    CallTab pp_tab;
    // streaming feature front-end per slot of the stream pool (api_pool_wave.hip.inc), allocated on its first use: the carry of every
    // slot [max_streams][WAVE_CARRY_CAP], the staged rows of one call (grow-only), the call's table (slot, samples so far, new samples,
    // final per active row, [max_streams] WAVE_TAB_INTS ints).  Host per slot: PoolSlot::wave.
    DevBuf<float> wv_carry, wv_stage;
    CallTab wv_tab;
    // encoder-frame history per slot of the stream pool (api_pool_hist.hip.inc), allocated on a slot's first rnnt_stream_keep_frames:
    // hs_buf[slot] [max_cache_frames][256], the device tables hs_ptr / hs_len [max_streams] the append and gather kernels index by
    // slot, the dense staging of rnnt_pool_rescore (grow-only).  Host per slot: PoolSlot::hist.
    std::vector<DevBuf<float>> hs_buf;
    DevBuf<float*> hs_ptr;
    DevBuf<int> hs_len;
    DevBuf<float> hs_stage;
    // endpoint detection per slot of the stream pool (api_pool_endpoint.hip.inc), allocated on the first rnnt_stream_endpoint: config
    // (with the on flag) and the five counters per slot [max_streams], the call table of the seam form (the slot list), the pinned
    // block one rnnt_pool_get_endpoints read lands in.  Host per slot: PoolSlot::ep (the on flag only).
    DevBuf<EpCfg> ep_cfg;
    DevBuf<int> ep_state;
    CallTab ep_tab;
    PinnedBuf<int> ep_host;
    CallTab seg_tab;                           // the slot list of one rnnt_pool_segment call, [max_streams]
    hipStream_t cap_stream = nullptr;          // stream-capture scratch stream
    struct DecGraph { int n_streams, k; hipGraphExec_t exec; };
    std::vector<DecGraph> dec_graphs;          // K greedy steps captured once per (n_streams, K)
    bool capturing = false;
    int use_graphs = 1;
    // optional per-kernel-site timing with HIP events on the launch stream (bench.py roofline leg)
    int prof_tag = -1;
    std::vector<hipEvent_t> prof_ev;
    size_t prof_used = 0;
    // optional launch-form log (rnnt_form_log_begin / _end): the name LAUNCHCHK is given at every launch site, counted on the host
    bool form_log_on = false;
    std::map<std::string, int64_t> form_log;

    // The only free list: streams, events and graphs here, every buffer and call table through its owner's destructor.  No user-provided
    // constructor -- rnnt_create's `new rnnt_ctx()` value-initialises lw[] and the raw weight views to null.
    ~rnnt_ctx() {
        for (auto& g : dec_graphs) (void)hipGraphExecDestroy(g.exec);
        for (hipEvent_t e : {sub_ev[0], sub_ev[1]}) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : prof_ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
        for (hipStream_t st : {dec_stream, cap_stream, sub_stream}) if (st) (void)hipStreamDestroy(st);
    }
};

#include "host_launch.hip.inc"
#include "host_decode.hip.inc"
#include "host_lm.hip.inc"

extern "C" {
#include "api_lifecycle.hip.inc"
#include "api_encoder.hip.inc"
#include "api_decode.hip.inc"
#include "api_beam.hip.inc"
#include "api_ops.hip.inc"
#include "api_score.hip.inc"
#include "api_loss.hip.inc"
#include "api_ctc_loss.hip.inc"
#include "api_joint.hip.inc"
#include "api_joint_loss.hip.inc"
#include "api_lstm.hip.inc"
#include "api_attn.hip.inc"
#include "api_state.hip.inc"
#include "api_ngram.hip.inc"
#include "api_pool_ctc.hip.inc"
#include "api_pool_prefix.hip.inc"
#include "api_pool.hip.inc"
#include "api_pool_hist.hip.inc"
#include "api_pool_endpoint.hip.inc"
#include "api_pool_segment.hip.inc"
#include "api_pool_wave.hip.inc"
#include "api_prefix.hip.inc"
#include "api_ctc_prefix.hip.inc"
}  // extern "C"
