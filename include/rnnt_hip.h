/*
 * rnnt_hip.h — C ABI of librnnt_hip.so: the MI355X (gfx950) streaming RNN-Transducer
 * inference path (chunked Conformer encoder + LSTM predictor + joint + greedy/beam step kernels).
 *
 * The reference (CentaureaHO/CTC-VR) has no FFI/plugin layer: its boundary for this path is the
 * Python class OnlineRNNTModel (model/online_rnnt_model.py:58) and, one level below, WeNet's
 * step API forward_encoder_chunk / forward_predictor_step / forward_joint_step
 * (wenet/transducer/transducer.py:444-472).  Each entry point below names the reference
 * function it replaces.  The Python facade in ctc-vr_amd/online_rnnt_model.py binds these
 * symbols with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns 0 on success or a
 * negative rnnt_status; rnnt_last_error(ctx) returns a static/ctx-owned message; no exceptions
 * cross the ABI.  The caller owns every buffer it passes; the library owns what it allocates
 * inside a context.  "dev" pointers are HIP device pointers on the context's device; "host"
 * pointers are ordinary host memory.  A context is confined to one host thread at a time; all
 * work of one call is enqueued on the hipStream_t passed as `stream` (void*; NULL = default
 * stream).  Calls that return data to the host synchronise that stream.
 * All streams of one context advance in lock step (same chunk length per call) through rnnt_encoder_chunk / rnnt_encoder_chunks /
 * rnnt_decode_ragged; the stream pool (rnnt_stream_open, rnnt_pool_chunk) gives every slot a position of its own instead.
 */
#ifndef RNNT_HIP_H
#define RNNT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rnnt_ctx rnnt_ctx;

typedef enum {
    RNNT_OK = 0,
    RNNT_ERR_ARG = -1,      /* bad argument / unknown tensor name                         */
    RNNT_ERR_SHAPE = -2,    /* tensor shape or capacity mismatch                          */
    RNNT_ERR_OOM = -3,      /* hipMalloc failed                                           */
    RNNT_ERR_HIP = -4,      /* a HIP runtime call or kernel launch failed                 */
    RNNT_ERR_STATE = -5     /* call sequence error (weights not finalized, no streams...) */
} rnnt_status;

/* numerics modes for rnnt_finalize_weights: how the dense contractions of the encoder and of the joint lattice
 * (positionwise_feed_forward.py:50-58, attention.py:109-131, subsampling.py:188-193, convolution.py:138-148,
 * model/component/joint.py:62-69) are evaluated.  Storage is fp32 in every mode; LayerNorm, softmax, depthwise conv,
 * the LSTM predictor and the greedy/beam decode arithmetic are fp32 in every mode. */
#define RNNT_NUMERICS_FP32   0 /* exact-f32 MFMA (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain): default parity mode     */
#define RNNT_NUMERICS_BF16X3 1 /* split bf16: x = hi + lo, hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16, fp32        */
                               /* accumulate; ~1e-5 relative per product; parity-gated (tokens exact, logits <= 1e-3)      */
#define RNNT_NUMERICS_BF16   2 /* plain bf16 operands, fp32 accumulate: perf mode, token-match rate reported, no parity   */
#define RNNT_NUMERICS_F16X3  3 /* split f16 (11-bit planes): ~5e-7 relative per product, same cost as bf16x3; operand      */
                               /* range below                                                                               */
/* Operand range of each mode (operands: the weights and the activations a contraction reads; the planes carry no scale).
 *   FP32, BF16X3, BF16: the f32 exponent range.  A bf16 plane has the f32 exponent, so the relative error of hi + lo (2^-17) does
 *           not depend on the magnitude: a power-of-two rescale of an operand pair changes nothing (measured: DESIGN.md).
 *   F16X3:  upper limit 65504 (the largest f16; above it the hi plane is inf).  Lower limit 2^-3 for full precision: the lo plane
 *           of any |x| < 2^-3 lies below 2^-14, an f16 subnormal, and its error is absolute (up to 2^-25) instead of relative, so
 *           the planes of a tensor of magnitude m miss it by about 2^-25 / m: 3e-7 at m = 1/16 (seeded weights), 1.8e-5 at 2^-10,
 *           1.4e-4 at 2^-13; below 2^-25 nothing is left of the operand.  Activations of the encoder (LayerNorm outputs, O(1)) sit
 *           inside the range.  Weights are checked: rnnt_finalize_weights(F16X3) returns RNNT_ERR_ARG, naming the tensor, for a GEMM
 *           weight above 65504 or whose two planes miss it by more than RNNT_F16X3_SPLIT_LIMIT of its r.m.s. magnitude (a tensor
 *           at the limit moves the encoder frames by about 4e-4 of the 1e-3 parity bar; measured: DESIGN.md).  Nothing is
 *           launched or changed on the device by a refused call; BF16X3 or FP32 take the same loaded tensors. */
#define RNNT_F16X3_SPLIT_LIMIT 1e-4

typedef struct {
    int32_t max_streams;       /* B: streams (lock-stepped, or stream-pool slots) held by the context */
    int32_t max_chunk_frames;  /* largest fbank chunk (input frames) passed to rnnt_encoder_chunk  */
    int32_t max_cache_frames;  /* K/V cache capacity per stream, in encoder frames (<= 5000)       */
    int32_t max_enc_frames;    /* encoder-output frame buffer per stream (frames awaiting decode)  */
    int32_t max_tokens;        /* token buffer per stream                                          */
    int32_t vocab_size;        /* 412 for the reference tokenizer (tokenizer/tokenizer.py:53-60)   */
    int32_t blank_id;          /* 5                                                                */
    int32_t n_steps;           /* max symbols per encoder frame (online_rnnt_model.py:174) = 10    */
    int32_t device;            /* HIP device ordinal                                               */
    int32_t max_beam;          /* largest beam size for rnnt_beam_frame (0 = beam search unused)   */
} rnnt_config;

/* -- lifetime ------------------------------------------------------------------------------ */
/* replaces OnlineRNNTModel.__init__ (model/online_rnnt_model.py:58-143): fixed architecture
 * (12 Conformer blocks, D=256, H=4, FFN=1024, conv2d/4, rel_pos, causal dw k=31 + BatchNorm,
 * Embedding+LSTM(256) predictor, add/tanh joint). */
int rnnt_create(const rnnt_config* cfg, rnnt_ctx** out);
void rnnt_destroy(rnnt_ctx* ctx);
const char* rnnt_last_error(const rnnt_ctx* ctx);
int rnnt_abi_version(void);
/* Device bytes that the contexts of this process hold at this moment: the sum of the sizes requested from hipMalloc for every
 * buffer of every live context (create-time buffers, weights, and the work buffers that entry points allocate on their first call
 * or grow), not the allocator's rounding.  rnnt_destroy gives all of a context's bytes back; a failed rnnt_create followed by
 * rnnt_destroy leaves the count where it was.  For sizing a deployment: read it after one call of each entry point in use. */
int64_t rnnt_live_device_bytes(void);

/* -- weights --------------------------------------------------------------------------------- */
/* replaces load_state_dict(checkpoint['model']) (online_rnnt_decode.py:49-50): one call per
 * entry of the reference's 504-key state dict (names as in SURVEY.md §8b), float32 host data
 * (num_batches_tracked entries are accepted and ignored). */
int rnnt_load_tensor(rnnt_ctx* ctx, const char* name, const float* host_data, int32_t ndim,
                     const int64_t* dims);
/* The whole state dict in ONE call from a flat float32 blob (the packed blob of the multi-GPU weight broadcast, SURVEY.md §8e:
 * rank 0 broadcasts it over RCCL, every rank hands its device copy to its context).  blob: n_floats floats, on the context's
 * device (on_device != 0) or on the host; tensor i is `names[i]` with `ndims[i]` dimensions taken in order from dims_flat and
 * starts where tensor i-1 ends.  Equivalent to n_tensors calls of rnnt_load_tensor (one device-to-host copy instead of none:
 * the packing below needs the values on the host).  Fails with RNNT_ERR_SHAPE if the table does not cover exactly n_floats. */
int rnnt_load_packed(rnnt_ctx* ctx, const float* blob, int64_t n_floats, int32_t on_device, int32_t n_tensors,
                     const char* const* names, const int32_t* ndims, const int64_t* dims_flat);
/* packs weights for the kernels (BatchNorm fold, linear_pos table pe*W_pos^T, LSTM input table,
 * GLU/LSTM row interleave, conv2 channels-last) and uploads them.  Fails with RNNT_ERR_STATE if
 * any required tensor is missing. */
int rnnt_finalize_weights(rnnt_ctx* ctx, int32_t numerics_mode, void* stream);

/* -- stream state ------------------------------------------------------------------------------ */
/* replaces OnlineRNNTModel.reset_streaming_cache (model/online_rnnt_model.py:145-164) for
 * n_streams lock-stepped streams: empty K/V cache, zero conv left-context, zero LSTM state,
 * last token = blank, no beam, frame buffer empty. */
int rnnt_streams_reset(rnnt_ctx* ctx, int32_t n_streams, void* stream);

/* replaces encoder.forward_chunk(xs, offset, required_cache_size, att_cache, cnn_cache)
 * (wenet/transformer/encoder.py:203-299) as called from _decode_chunk_streaming_logic
 * (model/online_rnnt_model.py:175-181), for all streams at once.
 *   fbank_dev  [n_streams, chunk_frames, 80] float32, device
 *   offset, required_cache_size: the reference's arguments (estimated encoder offset; see
 *       model/online_rnnt_model.py:364-370).  required_cache_size < 0 keeps every key, 0 keeps none,
 *       R > 0 keeps the last R (encoder.py:259-264).  R bounds the attention window only: the K/V rows
 *       of a stream are appended to a linear buffer of max_cache_frames rows through which the window
 *       slides, so max_cache_frames bounds the encoder frames of the utterance (since the last reset,
 *       or since the cache last became empty), not the window.  Refused with RNNT_ERR_SHAPE, with no
 *       change of frames, caches or tokens (also by rnnt_encoder_chunks and rnnt_pool_chunk): a chunk
 *       whose key window would end beyond row max_cache_frames, and offset < the present cache length.
 * K/V and conv caches live in the context.  The t' = ((T-3)/2+1-3)/2+1 output frames of every
 * stream are appended to the context's encoder-frame buffer; *frames_out receives t'. */
int rnnt_encoder_chunk(rnnt_ctx* ctx, const float* fbank_dev, int32_t chunk_frames, int32_t offset,
                       int32_t required_cache_size, int32_t* frames_out, void* stream);

/* replaces the whole chunk loop around forward_chunk (online_rnnt_decode.py:87-117, or streaming_inference,
 * model/online_rnnt_model.py:311-342) for utterances that are fully available: chunk c of every stream covers fbank
 * frames [chunk_start[c], chunk_start[c]+chunk_len[c]) and is encoded with (offsets[c], required[c]) exactly as
 * n_chunks calls of rnnt_encoder_chunk would (same float32 arithmetic up to summation order).  Schedule: layer-major -- each
 * of the 12 blocks runs over all chunks at once (one GEMM over streams x frames rows per contraction; every query keeps its
 * own chunk's key window and positional window); plans with a cache reset in the middle of the call take the wavefront over
 * (chunk, layer) instead.  fbank_dev [n_streams, total_frames, 80]; host int arrays.
 * greedy != 0: the greedy decode of rnnt_greedy_decode follows on the same stream; the call returns with all frames
 * decoded (synchronises).  Two contexts driven by two host threads overlap one call's decode with the other's encoder. */
int rnnt_encoder_chunks(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, int32_t n_chunks,
                        const int32_t* chunk_start, const int32_t* chunk_len, const int32_t* offsets,
                        const int32_t* required, int32_t greedy, int32_t* frames_out, void* stream);

/* replaces the greedy loops of _decode_chunk_streaming_logic (model/online_rnnt_model.py:183-222)
 * over every buffered encoder frame not yet decoded, all streams in parallel, state carried in
 * the context (LSTM [h,c], last token).  Appends to the per-stream token buffers.  Synchronises. */
int rnnt_greedy_decode(rnnt_ctx* ctx, void* stream);

/* token buffers: counts_host[n_streams] total tokens so far; tokens_host [n_streams, max_tokens]
 * (row-major, int32).  Either pointer may be NULL.  Synchronises. */
int rnnt_get_tokens(rnnt_ctx* ctx, int32_t* counts_host, int32_t* tokens_host, void* stream);

/* drop decoded frames from the encoder-frame buffer (keeps undecoded ones). */
int rnnt_frames_consume(rnnt_ctx* ctx, void* stream);

/* -- stream pool: slots that open, advance and close independently ------------------------------ */
/* The n_streams slots of a context, each with its own life: a slot is opened (reset on its own), fed chunks whenever its caller
 * has one, and simply re-opened for the next caller, while its neighbours are anywhere in their own utterances or idle.
 * Contract: the tokens, encoder frames and cached state of an utterance that runs in a slot are those of the same utterance run
 * alone (n_streams = 1) through rnnt_encoder_chunk + rnnt_greedy_decode + rnnt_frames_consume, bit for bit, whatever the other
 * slots do.  Once rnnt_stream_open or rnnt_pool_chunk has run, the slots' positions may differ: rnnt_encoder_chunk,
 * rnnt_encoder_chunks, rnnt_decode_ragged and rnnt_encode_ragged refuse with RNNT_ERR_STATE until the next rnnt_streams_reset, and
 * the read-back getters return each slot's own state.  Pool calls leave the context's beam-search state alone: the lock-step
 * hypotheses and state pools of rnnt_beam_advance / rnnt_beam_decode / rnnt_beam_select.  The pool's own beam search
 * (rnnt_pool_chunk_beam) keeps a beam PER SLOT, resident on the device between calls and separate from that state: hypothesis i of
 * slot b is the fixed row b * max_beam + i (token list of capacity max_tokens, length, f64 score, 64-bit sequence hash, LSTM state),
 * allocated on the first beam call of a context created with max_beam > 0.  rnnt_stream_open also resets its slot's beam to the one
 * empty hypothesis with score 0 and the zero LSTM state (online_rnnt_model.py:407-415), rnnt_streams_reset those of all slots.  A
 * slot's greedy state and its beam are independent: greedy and beam calls may be mixed freely across the slots of a context.
 *
 * rnnt_stream_open: reset_streaming_cache (model/online_rnnt_model.py:145-164) for ONE slot in [0, n_streams) -- empty K/V cache,
 * conv left context of a fresh stream, zero LSTM state, last token = blank, token count 0, position 0.  Touches no other slot.
 * Valid after rnnt_streams_reset(ctx, n), which opens all n slots at once. */
int rnnt_stream_open(rnnt_ctx* ctx, int32_t slot, void* stream);
/* forward_chunk (wenet/transformer/encoder.py:203-299) for the n_active listed slots (distinct, in [0, n_streams)): row i of
 * fbank_dev [n_active, chunk_frames, 80] belongs to slot slots_host[i] and is encoded with offsets_host[i] / required_host[i] at
 * that slot's own cache length, K/V row, positional window and conv-ring position, exactly as rnnt_encoder_chunk would for a
 * context holding only that stream.  One chunk length per call; *frames_out receives t'.
 *   greedy != 0: the greedy decode of the new frames of the active slots follows and the frames are consumed (one call = encode +
 *     decode + consume; synchronises like rnnt_greedy_decode).  Read tokens with rnnt_stream_get_tokens / rnnt_get_tokens.
 *   greedy == 0: encoder only.  The new frames stay buffered as frames [0, t') of the active slots' rows, readable with
 *     rnnt_get_enc_frames (rows of idle slots are undefined), and must be dropped with rnnt_frames_discard before the next pool
 *     call, which otherwise refuses with RNNT_ERR_STATE.  Does not synchronise.
 * Slots not listed are neither read nor written: K/V rows, both rings, h, c, last token, token buffer and count stay bitwise as
 * they were.  Refusals (duplicated or out-of-range slot: RNNT_ERR_ARG; chunk outside [7, max_chunk_frames], a positional window
 * outside the 5000-entry table or a full K/V cache of ANY listed slot: RNNT_ERR_SHAPE; frames still buffered: RNNT_ERR_STATE) are
 * decided on the host before the first launch and change no slot's state. */
int rnnt_pool_chunk(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t chunk_frames,
                    const int32_t* offsets_host, const int32_t* required_host, int32_t greedy, int32_t* frames_out, void* stream);
/* rnnt_pool_chunk for the listed slots (same arguments, validation, encoder launches and position bookkeeping), followed by the
 * per-frame loop of _decode_chunk_beam_search (model/online_rnnt_model.py:419-518) over the new frames [0, t') of exactly those
 * slots, each on its own resident beam: per frame one extension-chain launch over the active slots' rows and one merge launch with
 * one workgroup per active slot (rnnt_beam_decode's kernels' arithmetic; no upload of hypotheses, no gather / compaction, no
 * download).  The frames are consumed: one call = encode + beam + consume.  Does not synchronise; the getters below do.
 * Contract: a slot's hypotheses, their order, f64 scores and LSTM states are those of a one-stream context run chunk by chunk
 * through rnnt_encoder_chunk + rnnt_beam_decode + rnnt_frames_discard, bit for bit, whatever the other slots do.
 * beam_size applies to every row of the call and may change from call to call.  Range: that of rnnt_beam_decode (beam_size <=
 * min(max_beam, 16), vocab_size <= 512, n_steps <= 10, the chain kernel enabled).  Refusals, all decided on the host before the first
 * launch and changing no slot's state or position: every refusal of rnnt_pool_chunk; beam_size outside the range, vocab_size > 512:
 * RNNT_ERR_ARG; max_beam = 0 or RNNT_BEAM_CHAIN=0: RNNT_ERR_STATE; a listed slot whose longest hypothesis + t' * n_steps would pass
 * max_tokens: RNNT_ERR_SHAPE (the library keeps a conservative host bound per slot and reads the slot's true lengths back, with one
 * small synchronising copy, only when that bound is reached). */
int rnnt_pool_chunk_beam(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t chunk_frames,
                         const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size, int32_t* frames_out, void* stream);
/* the slot's hypotheses in beam order: *n_hyp of them, lens_host [cap_hyps], tokens_host [cap_hyps][cap_tokens] (row i holds
 * lens_host[i] tokens), scores_host [cap_hyps] (f64).  Any output pointer may be NULL (all NULL: query *n_hyp only; tokens_host NULL:
 * query the lengths).  RNNT_ERR_ARG when cap_hyps or cap_tokens is too small for a requested output.  Synchronises. */
int rnnt_stream_get_beam(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                         int32_t* tokens_host, double* scores_host, void* stream);
/* LSTM state of the slot's hypotheses, in beam order: h_host, c_host [n_hyp][256] (cap_hyps >= n_hyp).  Synchronises. */
int rnnt_stream_get_beam_states(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, float* h_host, float* c_host, void* stream);
/* tokens [from, count) of one slot, at most cap of them into tokens_host; *n_out = count - from (0 if from >= count), so a caller
 * polls only its own increments.  Synchronises. */
int rnnt_stream_get_tokens(rnnt_ctx* ctx, int32_t slot, int32_t from, int32_t cap, int32_t* tokens_host, int32_t* n_out, void* stream);

/* Greedy decode of a padded batch of whole utterances of DIFFERENT lengths in one call (utils/utils.py:29-50 pads a batch,
 * online_rnnt_eval.py:86-94 decodes every utterance with its own audio_lens): stream b runs the decode script's chunk loop
 * (online_rnnt_decode.py:81-117) over its own lens_host[b] frames of fbank_dev [n_streams, total_frames, 80]; tokens / counts are
 * read with the usual getters and equal a B = 1 run of that utterance.  Needs freshly reset streams (rnnt_streams_reset) and leaves
 * them finished (reset before the next call).  Utterances of fewer than 7 frames give no tokens; an utterance that is a single
 * chunk (at least 7 but fewer than chunk_frames + max(16, chunk_frames) frames) is refused with RNNT_ERR_SHAPE -- run those through
 * rnnt_encoder_chunks.  frames_out [n_streams] (optional, host): encoder frames per stream. */
int rnnt_decode_ragged(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                       int32_t* frames_out, void* stream);

/* The encoder half of rnnt_decode_ragged (same chunk plans, launches and refusals) without the greedy decoder: stream b's
 * frames_out[b] encoder frames stay in the frame buffer for rnnt_beam_decode(ctx, 0, frames_out, ...).  Needs freshly reset
 * streams.  Does not synchronise. */
int rnnt_encode_ragged(rnnt_ctx* ctx, const float* fbank_dev, int32_t total_frames, const int32_t* lens_host, int32_t chunk_frames,
                       int32_t* frames_out, void* stream);

/* -- beam search: device half of _decode_chunk_beam_search (model/online_rnnt_model.py:419-503) -- */
/* One encoder frame, all live hypotheses ("rows") of all streams at once.  For every row the library runs the
 * reference's greedy extension chain (<= n_steps evaluations: predictor step, joint, log_softmax, blank
 * log-prob, top-beam_k non-blank, stop when blank >= max - 1e-6, else extend with the best non-blank) and
 * keeps every intermediate LSTM state in a pool.  The caller (host) owns the hypothesis bookkeeping — token
 * lists, Python-double scores, stable sort, first-wins de-dup (:505-518) — and then tells the library which
 * pooled state each surviving hypothesis keeps.
 *   frame_idx            index into the buffered encoder frames
 *   row_stream_host[n]   stream of each row;  row_tok_host[n] predictor input token (last token or blank)
 *   steps_host[n]        evaluations done per row
 *   blank_lp_host [n][n_steps], top_lp_host / top_tok_host [n][n_steps][beam_k]
 * Row r's state before evaluation s is pool slot (r, s); the state after consuming the input token of
 * evaluation s is slot (r, s+1).  Synchronises. */
int rnnt_beam_frame(rnnt_ctx* ctx, int32_t frame_idx, int32_t n_rows, const int32_t* row_stream_host,
                    const int32_t* row_tok_host, int32_t beam_k, int32_t* steps_host, float* blank_lp_host,
                    float* top_lp_host, int32_t* top_tok_host, void* stream);
/* new row r takes pool slot (src_row_host[r], src_step_host[r]); rows are renumbered 0..n_new-1. */
int rnnt_beam_select(rnnt_ctx* ctx, int32_t n_new, const int32_t* src_row_host, const int32_t* src_step_host, void* stream);
/* current [h,c] of rows 0..n_rows-1: h_host, c_host [n_rows,256].  Synchronises. */
int rnnt_beam_get_states(rnnt_ctx* ctx, int32_t n_rows, float* h_host, float* c_host, void* stream);

/* Beam search with the bookkeeping inside the library: the per-frame loop of _decode_chunk_beam_search
 * (model/online_rnnt_model.py:419-518) over the buffered frames [frame_begin, frame_end) of every stream -- extension
 * chains on the device (one resident workgroup per hypothesis), candidate order / double-precision scores / stable
 * sort / first-wins de-duplication on the host in C++, state pool gather.  rnnt_streams_reset starts every stream with
 * one empty hypothesis (:407-415).  Results: rnnt_beam_hyp_count / rnnt_beam_get_hyp (tokens_host may be NULL to query
 * the length); hypothesis i of stream b is device row (hypotheses of streams < b) + i for rnnt_beam_get_states. */
int rnnt_beam_advance(rnnt_ctx* ctx, int32_t frame_begin, int32_t frame_end, int32_t beam_size, void* stream);
int rnnt_beam_hyp_count(rnnt_ctx* ctx, int32_t stream_idx, int32_t* n_out);
int rnnt_beam_get_hyp(rnnt_ctx* ctx, int32_t stream_idx, int32_t hyp_idx, int32_t cap, int32_t* tokens_host, int32_t* n_tokens,
                      double* log_prob);
/* The host half of one frame for one stream as a pure function (no context, no GPU; CPU tests): flat hypotheses in,
 * flat survivors out, returns their number.  Same code rnnt_beam_advance runs. */
int rnnt_beam_merge_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                         const int32_t* steps, const float* blank_lp, const float* top_lp, const int32_t* top_tok,
                         int32_t n_steps, int32_t k, int32_t beam_size, int32_t* out_len, int32_t* out_tokens,
                         double* out_score, int32_t* out_src_row, int32_t* out_src_step);
/* Device-resident beam search: the same recursion as rnnt_beam_advance with the whole frame loop on the device -- per frame
 * one extension-chain launch and one merge launch (candidate order, double-precision scores with the host's additions in the
 * host's order, stable descending order, first-wins de-duplication on the full token sequence, truncation, state gather), no
 * host copy and no synchronisation inside the loop; one synchronisation at the end.  Stream b covers the buffered frames
 * [frame_begin, frame_end_host[b]) (frame_end_host NULL: frames_buffered for every stream), so a padded batch of utterances of
 * different lengths is beam-decoded in one call.  Afterwards rnnt_beam_hyp_count / rnnt_beam_get_hyp / rnnt_beam_get_states
 * read exactly what rnnt_beam_advance leaves (bitwise the same hypotheses, scores and states): the two calls can be mixed chunk
 * by chunk.  Supported: beam_size <= 16 (and <= max_beam), vocab_size <= 512, n_steps <= 10; otherwise RNNT_ERR_ARG, and with
 * RNNT_BEAM_CHAIN=0 RNNT_ERR_STATE: use rnnt_beam_advance then. */
int rnnt_beam_decode(rnnt_ctx* ctx, int32_t frame_begin, const int32_t* frame_end_host, int32_t beam_size, void* stream);
/* The merge of rnnt_beam_decode run once on the device for one stream, on flat host inputs: same arguments and results as
 * rnnt_beam_merge_host (test seam; needs a context created with max_beam >= k; n_hyp, beam_size, k <= 16, n_steps <= 10).
 * Leaves the context's hypotheses and state pools alone.  Synchronises. */
int rnnt_beam_merge_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                           const int32_t* steps, const float* blank_lp, const float* top_lp, const int32_t* top_tok,
                           int32_t n_steps, int32_t k, int32_t beam_size, int32_t* out_len, int32_t* out_tokens,
                           double* out_score, int32_t* out_src_row, int32_t* out_src_step, void* stream);
/* drop all buffered encoder frames (beam path; the greedy path uses rnnt_frames_consume). */
int rnnt_frames_discard(rnnt_ctx* ctx, void* stream);

/* -- step API (WeNet export precedent, wenet/transducer/transducer.py:444-472) ---------------- */
/* forward_predictor_step (wenet/transducer/predictor.py:185-210): tokens_dev int32 [rows],
 * h/c in/out float32 [rows,256] device; out_dev [rows,256]. */
int rnnt_predictor_step(rnnt_ctx* ctx, const int32_t* tokens_dev, const float* h_in_dev,
                        const float* c_in_dev, int32_t rows, float* out_dev, float* h_out_dev,
                        float* c_out_dev, void* stream);
/* TransducerJoint.forward (model/component/joint.py:48-69), lattice form:
 * enc_dev [B,T,256], pred_dev [B,U,256] -> logits_dev [B,T,U,vocab]; mode 0 = raw logits,
 * 1 = log_softmax over the vocabulary (online_rnnt_model.py:446-447). */
int rnnt_joint(rnnt_ctx* ctx, const float* enc_dev, const float* pred_dev, int32_t B, int32_t T,
               int32_t U, int32_t mode, float* logits_dev, void* stream);

/* replaces BaseEncoder.forward(xs, lens, decoding_chunk_size=-1) (full context,
 * wenet/transformer/encoder.py:121-180).  fbank_dev [B,T,80], lens_host[B];
 * out_dev [B,T',256]; *frames_out = T'.  Runs as the layer-major schedule with ONE chunk of T frames (all valid keys at
 * positional window 0, per-stream padding mask); invalidates the streaming state. */
int rnnt_encoder_full(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B,
                      int32_t T, float* out_dev, int32_t* frames_out, void* stream);

/* CTC head on the same encoder: per-frame argmax of OnlineCTC.ctc_lo over the full-context encoder
 * output (model/online_rnnt_model.py:37-38,655-658).  ids_host [B, T'] int32; the repeat/blank collapse (:660-671)
 * is host code.  Needs ctc_head.ctc_lo.{weight,bias} among the loaded tensors. */
int rnnt_ctc_argmax(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B, int32_t T,
                    int32_t* ids_host, int32_t* frames_out, void* stream);

/* OnlineCTC.log_softmax (model/online_rnnt_model.py:34-35) on encoder frames already on the device: out_dev [rows, vocab] =
 * log_softmax(ctc_lo(enc_dev [rows, 256])).  The CTC term of the WeNet prefix beam search (wenet/transducer/search/
 * prefix_beam_search.py:66,99-101), whose frame loop runs in the facade over rnnt_encoder_full / rnnt_predictor_step / rnnt_joint
 * (OnlineRNNTModel.prefix_beam_search), or entirely on the device in rnnt_prefix_beam_decode below. */
int rnnt_ctc_logprobs(rnnt_ctx* ctx, const float* enc_dev, int32_t rows, float* out_dev, void* stream);

/* -- prefix beam search: WeNet's CTC-fused search (wenet/transducer/search/prefix_beam_search.py:42-148), batched and ragged ---- */
/* One symbol at most per encoder frame, CTC shallow fusion, prefix merging with log-add, for a padded batch of utterances of
 * different lengths in one call: row b walks frames [0, enc_lens_host[b]) of enc_dev [B, T, 256] (the output of rnnt_encoder_full,
 * device).  The reference walks every frame of its (batch-1) encoder output, padded ones included (:64,76): pass T for every row
 * to do the same, or the valid frame counts to stop each row at its own end.  Once per call: joint.enc_ffn and
 * log_softmax(ctc_lo(.)) (rnnt_ctc_logprobs) over the B*T frames.  Per frame two launches over the fixed rows b * beam_size + i,
 * no host copy and no synchronisation:
 *   prefix_step   one workgroup per live hypothesis: the LSTM cell on its last token, projection, joint, log-softmax (one
 *                 evaluation of rnnt_beam_decode's chain arithmetic); fusion log(tw * exp(lp) + cw * exp(ctc[t])) in f32 (:99-101);
 *                 top-beam_size over the WHOLE vocabulary, blank included (:104), value descending and, on equal values, the lower
 *                 index first (torch.topk leaves the order of equal values unspecified; this is the order the library defines)
 *   prefix_merge  one workgroup per utterance: candidates per hypothesis, per rank; score = f64((f32)running score + top value)
 *                 (:105); a blank keeps tokens and state, a token extends both (:110-126); a candidate whose token sequence
 *                 equals an earlier survivor's is log-added into it in f64 (the list form log_add([a, b]): -inf if both are, else
 *                 max + log(sum exp)) and the first one's tokens and state stay (:130-142); stable descending sort, truncation
 * Results, hypotheses best first: n_hyp_host [B]; lens_host [B, beam_size]; tokens_host [B, beam_size, cap_tokens] (row (b, i)
 * holds lens_host[b][i] tokens INCLUDING the leading blank, as the reference's hyp does; the rest of a row is not written);
 * scores_host [B, beam_size] f64; h_host / c_host: both NULL, or [B, beam_size, 256] receiving the hypotheses' LSTM states.
 * Entries of hypotheses i >= n_hyp_host[b] are zero.  A row of length 0 returns the one start hypothesis [blank] with score 0 and
 * the zero state.  With ctc_weight == 0 the CTC head is not needed and the CTC term is the literal 0.f.
 * One upload, one download, one synchronisation at the end.  The call leaves streaming, pool and lock-step beam state alone and
 * works on a context created with max_beam = 0: its buffers are its own, grow-only, sized by B * beam_size rows and T + 1 tokens.
 * Refusals, all decided on the host before the first launch: null pointer (h_host / c_host: one without the other), B < 1, a
 * length outside [0, T], beam_size outside [1, min(16, vocab_size)], vocab_size > 512, a negative weight or both weights zero,
 * cap_tokens < 1 + the longest length: RNNT_ERR_ARG; weights not finalized, ctc_weight > 0 without ctc_head.ctc_lo.*:
 * RNNT_ERR_STATE. */
int rnnt_prefix_beam_decode(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                            float ctc_weight, float transducer_weight, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                            int32_t* tokens_host, double* scores_host, float* h_host, float* c_host, void* stream);
/* prefix_merge's step for ONE utterance as a pure function (no context, no GPU; CPU tests): hyp_len [n_hyp], hyp_tokens
 * (concatenated), hyp_score [n_hyp] f64, top_lp / top_tok [n_hyp][k] in; survivors best first out -- out_len, out_tokens
 * (concatenated; room for beam_size * (longest input + 1) ints), out_score, and where each survivor's LSTM state comes from:
 * out_src_row = the hypothesis index, out_src_slot = 0 (its state, blank candidate) or 1 (the state after its last token).
 * Returns the number of survivors, or RNNT_ERR_ARG. */
int rnnt_prefix_merge_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                           const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size,
                           int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot);
/* The same through ONE prefix_merge launch (test seam; n_hyp, k, beam_size <= 16; any context, weights not needed).  Uses the
 * prefix search's own buffers only.  Synchronises. */
int rnnt_prefix_merge_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                             const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank, int32_t beam_size,
                             int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot,
                             void* stream);
/* -- hot-word biasing in the prefix beam search (the graph of rnnt_context_set, below) -------------------------------------------
 * The reference's transducer search has no context graph; the semantics are those of wenet/transformer/search.py:95-104,169-171,
 * 214-235 carried over to this frame step.  Every hypothesis holds a context state (graph node; [blank] holds the root, the leading
 * blank is never fed to the graph) and an f64 context score beside its running score.  prefix_step is untouched: the first prune
 * does not see the graph (search.py:156).  In prefix_merge a blank candidate copies its parent's state and score, any other token
 * takes one forward_one_step from the parent's state and adds its score; prefix fusion keeps the first candidate's (both are
 * functions of the token sequence); the second prune orders by total = fused score + context score, equal totals to the lower
 * candidate index.  At the end of the utterance finalize REPLACES the context score of every survivor; there is no re-sort, so the
 * returned totals need not descend.  A graph whose context_score is 0 gives the unbiased tokens and scores exactly.
 *
 * rnnt_prefix_beam_decode plus use_context and ctx_scores_host [B, beam_size] (may be NULL): scores_host are the totals,
 * ctx_scores_host their context part (unbiased score = score - context score).  use_context == 0 is rnnt_prefix_beam_decode, bit
 * for bit, with context scores 0.  Also RNNT_ERR_STATE: use_context without a graph set, decided before the first launch. */
int rnnt_prefix_beam_decode_ctx(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t beam_size,
                                float ctc_weight, float transducer_weight, int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host,
                                int32_t* lens_host, int32_t* tokens_host, double* scores_host, double* ctx_scores_host, float* h_host,
                                float* c_host, void* stream);
/* rnnt_prefix_merge_host with a graph, passed as phrases as rnnt_ctc_prefix_beam_host takes them (n_phrases >= 1; tokens only need
 * to be >= 0): plus hyp_ctx_state / hyp_ctx_score [n_hyp] in (node ids of that graph, creation order, root = 0) and the survivors'
 * out_ctx_state / out_ctx_score out.  out_score stays the fused score; the order is by out_score + out_ctx_score. */
int rnnt_prefix_merge_ctx_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                               const int32_t* hyp_ctx_state, const double* hyp_ctx_score, const float* top_lp, const int32_t* top_tok,
                               int32_t k, int32_t blank, int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens,
                               const int32_t* phrase_tokens, double context_score, int32_t* out_len, int32_t* out_tokens, double* out_score,
                               int32_t* out_src_row, int32_t* out_src_slot, int32_t* out_ctx_state, double* out_ctx_score);
/* The same through ONE prefix_merge launch with the graph that is set on the context (none: RNNT_ERR_STATE; a context state outside
 * the graph: RNNT_ERR_ARG).  Synchronises. */
int rnnt_prefix_merge_ctx_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                                 const int32_t* hyp_ctx_state, const double* hyp_ctx_score, const float* top_lp, const int32_t* top_tok,
                                 int32_t k, int32_t blank, int32_t beam_size, int32_t* out_len, int32_t* out_tokens, double* out_score,
                                 int32_t* out_src_row, int32_t* out_src_slot, int32_t* out_ctx_state, double* out_ctx_score, void* stream);

/* -- CTC prefix beam search with contextual biasing: WeNet's ctc_prefix_beam_search (wenet/transformer/search.py:125-247) --------- */
/* The context graph ("hot words") of wenet/utils/context_graph.py:144-210 over n_phrases token lists (phrase_tokens_host holds them
 * concatenated, phrase_lens_host their lengths), built on the host and uploaded; n_phrases == 0 clears it.  Trie in phrase order,
 * node ids in creation order (root = 0); every node carries token_score, node_score (depth x context_score by repeated addition),
 * output_score and is_end (decided when the node is created); fail and output arcs from the reference's breadth-first fill, its
 * quirks included.  All scores f64.  Device form: flat node arrays and a CSR of (token, child) sorted by token per node.
 * Refusals, RNNT_ERR_ARG: an empty phrase, a token outside [0, vocab_size), the blank inside a phrase, more than 4096 nodes. */
int rnnt_context_set(rnnt_ctx* ctx, int32_t n_phrases, const int32_t* phrase_lens_host, const int32_t* phrase_tokens_host,
                     double context_score);
/* Test seams of the graph (no context, no GPU; tokens need only be >= 0).  walk: feeds tokens [n_tokens] through forward_one_step
 * (:212-247) from the root; step_score_out / state_out [n_tokens] receive every step's score and the node it lands in,
 * *finalize_out what finalize (:249-265) returns for the last state.  dump: the node tables in node-id order (each pointer may be
 * NULL; room for 1 + the total phrase length): token (-1 at the root), node_score, output_score, is_end, fail id, output id (-1: none). */
int rnnt_context_walk_host(int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score,
                           int32_t n_tokens, const int32_t* tokens, double* step_score_out, int32_t* state_out, double* finalize_out);
int rnnt_context_dump_host(int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens, double context_score,
                           int32_t* n_nodes_out, int32_t* token_out, double* node_score_out, double* output_score_out,
                           int32_t* is_end_out, int32_t* fail_out, int32_t* output_out);
/* The search over log-probabilities lp_dev [B, T, vocab] f32 already on the device (any context; weights are not needed), row b over
 * frames [0, enc_lens_host[b]), in ONE launch: ctc_prefix_search, one workgroup per utterance with the frame loop inside.  Per row
 * the semantics of search.py:139-236:
 *   start       the empty prefix with s = 0, ns = -inf, v_s = 0, v_ns = 0 (sic), context state root, context score 0
 *   first prune top-beam_size of the frame over the whole vocabulary, blank included: value descending and, on equal values, the
 *               lower index first (torch.topk leaves that order open; this is the order the library defines)
 *   expansion   outer loop over those tokens, inner over the hypotheses in their order, the value widened to f64; blank, repeat of
 *               the last token and other as written: v_s and times_s are ASSIGNED by a blank, the Viterbi updates use strict <, the
 *               repeat's times_ns[-1] = t happens only when cur_token_prob < prob as well; log_add is the two-argument form in f64
 *               (-inf if both are, else max + log(sum exp)); an entry takes its context from the first contribution that touches it
 *   second prune sort by score() + context score descending, stable over first insertion, truncate to beam_size
 *   end         with a graph every survivor's context score is REPLACED by finalize's -node_score (sic) and the list is NOT
 *               re-sorted; score = log_add(s, ns) + that; times = times_s if v_s > v_ns else times_ns
 * use_context == 0 (or no graph): context scores are 0.  Results in that order: n_hyp_host [B]; lens_host [B, beam_size];
 * tokens_host / times_host [B, beam_size, cap_tokens] (no leading blank: the reference's prefixes have none); scores_host
 * [B, beam_size] f64; ctx_scores_host [B, beam_size] f64 or NULL.  Entries of hypotheses i >= n_hyp_host[b] and of a row beyond its
 * length are zero (a times list shorter than its tokens, possible only with -inf values, is zero-filled).  A row of length 0
 * returns the one empty hypothesis with score 0.  Touches only its own grow-only buffers.
 * Refusals, decided on the host before the launch: null pointer, B < 1, a length outside [0, T], beam_size outside
 * [1, min(16, vocab_size)], vocab_size > 512, cap_tokens below the longest length: RNNT_ERR_ARG; use_context with no graph set:
 * RNNT_ERR_STATE. */
int rnnt_ctc_prefix_beam_logprobs(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, int32_t B, int32_t T,
                                  int32_t beam_size, int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                  int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host, void* stream);
/* The same over encoder frames enc_dev [B, T, 256]: rnnt_ctc_logprobs over the B*T frames first.  RNNT_ERR_STATE without
 * ctc_head.ctc_lo.* or before rnnt_finalize_weights. */
int rnnt_ctc_prefix_beam_decode(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T,
                                int32_t beam_size, int32_t use_context, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host, void* stream);

/* -- the same search per slot of the stream pool, carried across calls ---------------------------- */
/* The search is a per-frame recursion whose state at a frame boundary is its <= 16 hypothesis records and two append-only arenas, so
 * a search that stops at the end of a call and resumes at the next is, bit for bit, the one-launch search over the same rows,
 * whatever the split.  Per slot the device keeps one record (2120 bytes) and [max_cache_frames * 16 + 1] (parent, value) pairs of
 * either arena -- 1.28 MB per slot per arena at max_cache_frames = 5000 -- allocated on the first use.  Frames, and the times
 * returned, are absolute encoder-frame indices since the slot's reset; a slot holds at most max_cache_frames of them.
 * A slot's search is fresh after a reset; its first advancing call fixes beam_size and use_context until the next reset.
 * rnnt_context_set starts a new graph generation: a search biased (use_context != 0) under an older generation is refused with
 * RNNT_ERR_STATE until its slot is reset (its context states are node ids of a graph that no longer exists); unbiased searches go
 * on.  Every refusal is decided before the first launch and changes no slot's state, position or frame count.  A slot's greedy
 * state, its RNN-T beam and its CTC prefix search are independent of one another; a library call holds slots of one kind.
 *
 * start state (empty prefix, s = 0, ns = -inf, v_s = v_ns = 0, context root) for one slot, or all slots with slot = -1; any context,
 * weights not needed.  rnnt_stream_open does this for its slot, rnnt_streams_reset for all (once the state exists). */
int rnnt_stream_ctc_prefix_reset(rnnt_ctx* ctx, int32_t slot, void* stream);
/* advance the searches of the listed slots (distinct, in [0, max_streams)) by t >= 1 frames of log-probabilities the caller holds:
 * lp_dev [n_active, t, vocab] f32 device, row i belongs to slot slots_host[i].  ONE launch (ctc_prefix_search_pool: one workgroup per
 * active row), no copy back, no synchronisation.  Any context (weights not needed).
 * RNNT_ERR_ARG: null pointer, duplicated or out-of-range slot, t < 1, beam_size outside [1, min(16, vocab)], vocabulary > 512,
 * beam_size or use_context differing from the search in progress.  RNNT_ERR_SHAPE: a slot's frames so far + t > max_cache_frames.
 * RNNT_ERR_STATE: use_context with no graph set, or a stale graph generation. */
int rnnt_pool_ctc_prefix_logprobs(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* lp_dev, int32_t t,
                                  int32_t beam_size, int32_t use_context, void* stream);
/* rnnt_pool_chunk for the listed slots (same arguments, validation, encoder launches, position bookkeeping and refusals), then
 * log_softmax(ctc_lo(.)) of the n_active * t' new encoder frames (rnnt_ctc_logprobs' arithmetic, kernel choices as for one stream's
 * rows) and the launch above.  Frames are consumed: one call = encode + CTC + search.  Does not synchronise.  Also RNNT_ERR_STATE
 * when the weights are not finalized, ctc_head.ctc_lo.* is not loaded, or frames are still buffered. */
int rnnt_pool_chunk_ctc_prefix(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t chunk_frames,
                               const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size, int32_t use_context,
                               int32_t* frames_out, void* stream);
/* the slot's hypotheses now, in the search's order; layout and zero fill as rnnt_ctc_prefix_beam_logprobs for B = 1: lens / scores /
 * ctx_scores (optional) [cap_hyps], tokens / times [cap_hyps][cap_tokens], with cap_hyps >= the slot's beam (1 for a fresh slot) and
 * cap_tokens >= the frames walked.  final != 0: what the one-launch search returns had the utterance ended here (with a graph the
 * context score is REPLACED by finalize's, no re-sort).  final == 0: context scores are the running ones and score = log_add(s, ns) +
 * running.  A fresh slot has fixed no use_context: final != 0 finalizes its root under the graph that is set, if any (context score
 * -0.0, as the one-launch search with use_context over no frames; +0.0 with no graph set or final == 0).  Reading changes nothing:
 * the search goes on afterwards.  *frames_out (optional) = frames walked so far.  One pack launch (ctc_prefix_pack), one download,
 * synchronises.  RNNT_ERR_STATE for final != 0 on a biased search of a stale graph generation.
 * Size query: with lens_host, tokens_host, times_host and scores_host all NULL nothing is launched or copied; *n_hyp receives the
 * cap_hyps the slot needs (its beam, 1 for a fresh slot) and *frames_out the cap_tokens it needs (cap_hyps / cap_tokens are ignored). */
int rnnt_stream_get_ctc_prefix(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp,
                               int32_t* lens_host, int32_t* tokens_host, int32_t* times_host, double* scores_host,
                               double* ctx_scores_host, int32_t* frames_out, void* stream);

/* -- the transducer prefix beam search (rnnt_prefix_beam_decode) per slot of the stream pool, carried across calls ------------- */
/* The search emits at most one symbol per frame and is frame-synchronous: its state at a frame boundary is the slot's <= 16
 * hypotheses (token list, f64 score, hash, two LSTM states each).  The pool kernels run the frame step of rnnt_prefix_beam_decode
 * (the same device functions) on rows that stay on the device between calls, so a search fed in pieces is, bit for bit, the B = 1
 * one-call search over the same frames, whatever the split.  Per slot the device keeps 16 fixed rows of two buffer sets -- token lists
 * of max_cache_frames + 1 ints, lengths, scores, hashes, states [2][512] f32 -- allocated on the first use (about 8 KB * 16 * 2 of
 * states and 8 * 16 * (max_cache_frames + 1) bytes of tokens per slot), counted by rnnt_live_device_bytes.  A slot holds at most
 * max_cache_frames frames.  A slot's search is fresh after a reset; its first advancing call fixes beam_size and the two weights
 * until the next reset.  Every refusal is decided before the first launch and changes no slot's state, position or frame count.  A
 * slot's greedy state, its RNN-T beam, its CTC prefix search and this search are independent of one another, and
 * rnnt_prefix_beam_decode's own buffers are not touched; a library call holds slots of one kind.
 *
 * the start hypothesis [blank] (score 0, zero LSTM state) for one slot, or all slots with slot = -1.  rnnt_stream_open does this for
 * its slot, rnnt_streams_reset for all (once the state exists). */
int rnnt_stream_prefix_reset(rnnt_ctx* ctx, int32_t slot, void* stream);
/* advance the searches of the listed slots (distinct, in [0, max_streams)) by t >= 1 encoder frames the caller holds: enc_dev
 * [n_active, t, 256] f32 device (after_norm rows, as rnnt_prefix_beam_decode takes them), row i belongs to slot slots_host[i].
 * joint.enc_ffn and, when ctc_weight > 0, rnnt_ctc_logprobs over the n_active * t rows (kernel choices of a small call), then per
 * frame one prefix_step_pool launch (one hypothesis per workgroup, or -- once n_active * beam_size exceeds 1.5 workgroups per CU --
 * up to 4 hypotheses of one slot per workgroup, one pass over the predictor and joint weights for all of them: the same bits either
 * way; RNNT_PREFIX_GROUP=1 / 4 at rnnt_create forces one) and one prefix_merge_pool launch (one workgroup per active slot).  One async copy of the call's table, launches
 * only, no synchronisation.
 * RNNT_ERR_ARG: null pointer, duplicated or out-of-range slot, n_active outside [1, max_streams], t < 1, beam_size outside
 * [1, min(16, vocab)], vocabulary > 512, a negative weight or both zero, beam_size or a weight differing from the search in progress.
 * RNNT_ERR_SHAPE: a slot's frames so far + t > max_cache_frames.  RNNT_ERR_STATE: weights not finalized, or ctc_weight > 0 without
 * ctc_head.ctc_lo.*. */
int rnnt_pool_prefix_frames(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, int32_t beam_size,
                            float ctc_weight, float transducer_weight, void* stream);
/* rnnt_pool_chunk for the listed slots (same arguments, validation, encoder launches, rnnt_stream_keep_frames history, position
 * bookkeeping and refusals), then the search above over the n_active * t' new encoder frames (2 launches per frame).  Frames are
 * consumed: one call = encode + (CTC) + search.  Does not synchronise.  Also RNNT_ERR_STATE when frames are still buffered. */
int rnnt_pool_chunk_prefix(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t chunk_frames,
                           const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size, float ctc_weight,
                           float transducer_weight, int32_t* frames_out, void* stream);
/* the slot's hypotheses now, best first, layout and zero fill as rnnt_prefix_beam_decode for B = 1: lens / scores [cap_hyps], tokens
 * [cap_hyps][cap_tokens] INCLUDING the leading blank, h / c [cap_hyps][256] (both or neither), *n_hyp the hypotheses held; cap_hyps >=
 * the slot's beam (1 for a fresh slot), cap_tokens >= 1 + the frames walked.  Reading changes nothing: the search goes on afterwards.
 * One pack launch (prefix_pack_pool), one download, synchronises.
 * Size query: with lens_host, tokens_host, scores_host, h_host and c_host all NULL nothing is launched or copied and n_hyp receives
 * THREE ints: the cap_hyps the slot needs (its beam, 1 for a fresh slot), the frames walked, and the cap_tokens it needs (a bound on
 * the longest list: 1 + the frames walked).  cap_hyps / cap_tokens are ignored. */
int rnnt_stream_get_prefix(rnnt_ctx* ctx, int32_t slot, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp, int32_t* lens_host,
                           int32_t* tokens_host, double* scores_host, float* h_host, float* c_host, void* stream);
/* The pool calls with hot-word biasing (semantics: rnnt_prefix_beam_decode_ctx): the calls above plus use_context; the rows also keep
 * a context state (int) and score (f64) per hypothesis in both buffer sets, counted by rnnt_live_device_bytes.  A slot's first
 * advancing call fixes use_context together with the beam and the two weights until its reset; a differing value: RNNT_ERR_ARG.
 * The graph-generation rule of the CTC pool search applies: after rnnt_context_set a search biased under an older generation is
 * refused with RNNT_ERR_STATE until its slot is reset, unbiased searches go on; use_context without a graph: RNNT_ERR_STATE.  Every
 * refusal is decided before the first launch and moves no slot.  A call lists slots of one use_context. */
int rnnt_pool_prefix_frames_ctx(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t,
                                int32_t beam_size, float ctc_weight, float transducer_weight, int32_t use_context, void* stream);
int rnnt_pool_chunk_prefix_ctx(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev, int32_t chunk_frames,
                               const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size, float ctc_weight,
                               float transducer_weight, int32_t use_context, int32_t* frames_out, void* stream);
/* rnnt_stream_get_prefix plus final and ctx_scores_host [cap_hyps] (may be NULL): scores_host are the totals, ctx_scores_host their
 * context part -- the running one, or with final != 0 finalize's: what rnnt_prefix_beam_decode_ctx would return had the utterance
 * ended here (no re-sort).  Reading changes nothing.  final != 0 on a search biased under an older graph generation: RNNT_ERR_STATE.
 * An unbiased slot reads as rnnt_stream_get_prefix does, with context scores 0; so does a fresh slot, except that with final != 0 and
 * a graph set it finalizes its root, as the one-call search over no frames does. */
int rnnt_stream_get_prefix_ctx(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp,
                               int32_t* lens_host, int32_t* tokens_host, double* scores_host, double* ctx_scores_host, float* h_host,
                               float* c_host, void* stream);

/* The same search as a pure C++ function (no context, no GPU): lp_host [B, T, vocab], the graph passed as phrases (n_phrases == 0:
 * none).  The CPU seam the device path is compared against: tokens, times and order exact. */
int rnnt_ctc_prefix_beam_host(const float* lp_host, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t vocab, int32_t blank,
                              int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens,
                              double context_score, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host,
                              int32_t* times_host, double* scores_host, double* ctx_scores_host);

/* -- n-gram language model, shallow fusion in the CTC prefix beam search -------------------------------------------------------- */
/* The model is a list of n_ngrams n-grams (tokens_host concatenated, lens_host their lengths, 1 <= k <= 8; logp_host / bow_host
 * natural-log probability and back-off weight, f64, finite).  Tokens are model ids in [0, vocab_size) other than the blank, plus
 * BOS = vocab_size (first position only) and EOS = vocab_size + 1 (last position only).  Every n-gram's prefix (all but its last
 * token) must be listed before it, so the list is a trie in insertion order: n-gram i is node i + 1, the root node 0.  fail[c] is the
 * node of the longest proper suffix of c's n-gram that is listed (the root if none); the list need not be suffix-closed.
 * Values are prescaled once on the host, each ONE f64 multiplication then ONE f64 addition (no FMA):
 *   W[c] = lm_weight * logp[c] + length_bonus   (an n-gram that ends in EOS: lm_weight * logp[c], no bonus)
 *   B[c] = lm_weight * bow[c]                   U = lm_weight * unk_logp + length_bonus
 * step(state, tok) -> (score, next): acc = 0, node = state; loop { c = child(node, tok); if c: return (acc + W[c], c); if node is
 * the root: return (acc + U, root); acc += B[node]; node = fail[node] }.  Additions only, in this order: host, device and an f64
 * restatement give the same bits.  The start state is child(root, BOS), the root when [BOS] is not listed; eos(state) is
 * step(state, EOS).score, 0 when no n-gram ends in EOS.
 * In the search every hypothesis carries an n-gram score (f64, from 0) and state beside its context score and state: copied where the
 * context is copied, advanced by step where the context is advanced, under the same first-touch rule.  The second prune sorts by
 * score() + context score + n-gram score; the first prune stays acoustic; at the end eos(state) is added and the list is NOT
 * re-sorted.  use_context and use_ngram are independent.
 *
 * rnnt_ngram_set builds and uploads the model (n_ngrams == 0 clears it) and starts a new model generation.  Device form: flat node
 * arrays, a CSR of (token, child) sorted by token per node, and the root's children as a dense row [vocab_size + 2].
 * Refusals, RNNT_ERR_ARG: an empty n-gram or one longer than 8; a token outside [0, vocab_size + 2) or the blank; BOS not first or
 * EOS not last; a prefix not listed earlier; an n-gram listed twice; a value that is not finite; lm_weight < 0; more than 1 << 22
 * nodes. */
int rnnt_ngram_set(rnnt_ctx* ctx, int32_t n_ngrams, const int32_t* lens_host, const int32_t* tokens_host, const double* logp_host,
                   const double* bow_host, double lm_weight, double length_bonus, double unk_logp);
/* Test seam (no context, no GPU): builds the model over the given vocabulary and blank and feeds tokens [n_tokens] (ids in
 * [0, vocab) other than the blank) through step from the start state; step_score_out / state_out [n_tokens] and *eos_out (the end
 * term of the last state) and *n_nodes_out (root included) may each be NULL. */
int rnnt_ngram_walk_host(int32_t n_ngrams, const int32_t* lens, const int32_t* ngram_tokens, const double* logp, const double* bow,
                         double lm_weight, double length_bonus, double unk_logp, int32_t vocab, int32_t blank, int32_t n_tokens,
                         const int32_t* tokens, double* step_score_out, int32_t* state_out, double* eos_out, int32_t* n_nodes_out);
/* n >= 1 token sequences scored by the model that is set, each from the start state, in ONE launch (ngram_score_rows, one sequence
 * per thread): tokens_host [n, cap], lens_host [n] in [0, cap]; step_scores_host [n, cap] (may be NULL; zero beyond a length) the
 * per-token step scores, totals_host [n] their sum in walk order, plus eos(last state) when with_eos.  One upload, one download,
 * one synchronisation.  RNNT_ERR_STATE when no model is set; RNNT_ERR_ARG for a token outside [0, vocab_size) or the blank. */
int rnnt_ngram_score(rnnt_ctx* ctx, int32_t n, const int32_t* lens_host, const int32_t* tokens_host, int32_t cap, int32_t with_eos,
                     double* step_scores_host, double* totals_host, void* stream);
/* rnnt_ctc_prefix_beam_logprobs / _decode plus use_ngram (the model of rnnt_ngram_set is fused) and ngram_scores_host
 * [B, beam_size] f64 or NULL (the n-gram part of scores_host, end term included; zero without use_ngram).  With use_ngram == 0 the
 * result is, bit for bit, that of the calls without the suffix, which are these calls.  use_ngram with no model set: RNNT_ERR_STATE. */
int rnnt_ctc_prefix_beam_logprobs_ngram(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, int32_t B, int32_t T,
                                        int32_t beam_size, int32_t use_context, int32_t use_ngram, int32_t cap_tokens,
                                        int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host, int32_t* times_host,
                                        double* scores_host, double* ctx_scores_host, double* ngram_scores_host, void* stream);
int rnnt_ctc_prefix_beam_decode_ngram(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T,
                                      int32_t beam_size, int32_t use_context, int32_t use_ngram, int32_t cap_tokens,
                                      int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host, int32_t* times_host,
                                      double* scores_host, double* ctx_scores_host, double* ngram_scores_host, void* stream);
/* rnnt_ctc_prefix_beam_host plus the model, passed as the list rnnt_ngram_set takes (n_ngrams == 0: none), and ngram_scores_host. */
int rnnt_ctc_prefix_beam_ngram_host(const float* lp_host, const int32_t* enc_lens_host, int32_t B, int32_t T, int32_t vocab,
                                    int32_t blank, int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens,
                                    const int32_t* phrase_tokens, double context_score, int32_t n_ngrams, const int32_t* ngram_lens,
                                    const int32_t* ngram_tokens, const double* logp, const double* bow, double lm_weight,
                                    double length_bonus, double unk_logp, int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host,
                                    int32_t* tokens_host, int32_t* times_host, double* scores_host, double* ctx_scores_host,
                                    double* ngram_scores_host);
/* The pool calls of the CTC prefix search plus use_ngram (the two advancing calls) or ngram_scores_host [cap_hyps] (the read; may be
 * NULL).  A slot's first advancing call fixes use_ngram together with beam_size and use_context until its reset; a differing value:
 * RNNT_ERR_ARG.  The slot record (2120 bytes) holds an n-gram score and state per hypothesis; a reset record (rnnt_stream_ctc_prefix_reset,
 * rnnt_stream_open, rnnt_streams_reset, rnnt_pool_segment) holds a start marker that the first step resolves to the start state of the
 * model set at that first call.  After rnnt_ngram_set a search that uses the model under an older generation is refused with
 * RNNT_ERR_STATE (advance, and read with final != 0) until its slot is reset; searches that do not use it go on.  final != 0 adds
 * the end term, final == 0 returns the running n-gram score; either way scores_host holds the totals.  A call lists slots of one
 * use_ngram. */
int rnnt_pool_ctc_prefix_logprobs_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* lp_dev, int32_t t,
                                        int32_t beam_size, int32_t use_context, int32_t use_ngram, void* stream);
int rnnt_pool_chunk_ctc_prefix_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev,
                                     int32_t chunk_frames, const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size,
                                     int32_t use_context, int32_t use_ngram, int32_t* frames_out, void* stream);
int rnnt_stream_get_ctc_prefix_ngram(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp,
                                     int32_t* lens_host, int32_t* tokens_host, int32_t* times_host, double* scores_host,
                                     double* ctx_scores_host, double* ngram_scores_host, int32_t* frames_out, void* stream);

/* -- n-gram shallow fusion in the transducer prefix beam search (the model of rnnt_ngram_set, above) ------------------------------
 * The rule of the CTC search carried over to the transducer frame step, as the hot words were.  THE DEFINITION:
 *   - Every hypothesis carries (ngram_state, ngram_score) beside (context_state, context_score); neither is ever folded into the
 *     running score.  [blank] holds the start MARKER (-1) and 0.0: the leading blank is never fed to the model, and the marker
 *     resolves to the model's start state at the first step, so every reset path (the start of a call, rnnt_stream_prefix_reset,
 *     rnnt_stream_open, rnnt_streams_reset, rnnt_pool_segment) is model-agnostic.
 *   - First prune: untouched.  prefix_step does not see the model.
 *   - Candidates: a blank copies its parent's state and score; any other token takes step(parent state, token) and adds the step's
 *     score to the parent's.
 *   - Prefix fusion: unchanged; the first candidate's state and score stay (both are functions of the token sequence alone).
 *   - Second prune: the key is fused score + context score + n-gram score, evaluated left to right; a term whose feature is off is
 *     left out, not added as 0.0.  Equal totals go to the lower candidate index; truncation to beam_size.
 *   - End of the utterance: each survivor's n-gram score gains eos(state) (the marker resolves to the start state).  No re-sort.  The
 *     returned total includes the end term; context finalize replaces the context score first, then the end term is added:
 *     total = score + finalized context score + (n-gram score + eos).  A non-final read of a pool slot returns the running score.
 *   - With use_ngram == 0, or a model with lm_weight = 0 and length_bonus = 0, tokens and scores are bit for bit those without the
 *     model, and all n-gram scores are 0.
 *
 * rnnt_prefix_beam_decode_ctx plus use_ngram and ngram_scores_host [B, beam_size] (may be NULL): scores_host are the totals,
 * ngram_scores_host their n-gram part, end term included.  use_ngram == 0 is rnnt_prefix_beam_decode_ctx, bit for bit, which is this
 * call.  Also RNNT_ERR_STATE: use_ngram without a model set, decided before the first launch. */
int rnnt_prefix_beam_decode_ngram(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, int32_t B, int32_t T,
                                  int32_t beam_size, float ctc_weight, float transducer_weight, int32_t use_context, int32_t use_ngram,
                                  int32_t cap_tokens, int32_t* n_hyp_host, int32_t* lens_host, int32_t* tokens_host, double* scores_host,
                                  double* ctx_scores_host, double* ngram_scores_host, float* h_host, float* c_host, void* stream);
/* rnnt_prefix_merge_ctx_host plus the model, passed as rnnt_ngram_walk_host takes it (the list, the three scalars, the vocabulary;
 * the blank is the call's; n_ngrams == 0: none), and hyp_ng_state / hyp_ng_score [n_hyp] in (node ids of that model, or -1 = the
 * start marker), the survivors' out_ng_state / out_ng_score out.  n_phrases == 0 means no graph: the context arguments may be NULL
 * and the context outputs, if given, receive 0.  out_score stays the fused score; the order is by out_score (+ out_ctx_score)
 * (+ out_ng_score).  With a model every candidate token other than the blank must be in [0, vocab). */
int rnnt_prefix_merge_ngram_host(int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens, const double* hyp_score,
                                 const int32_t* hyp_ctx_state, const double* hyp_ctx_score, const int32_t* hyp_ng_state,
                                 const double* hyp_ng_score, const float* top_lp, const int32_t* top_tok, int32_t k, int32_t blank,
                                 int32_t beam_size, int32_t n_phrases, const int32_t* phrase_lens, const int32_t* phrase_tokens,
                                 double context_score, int32_t n_ngrams, const int32_t* ngram_lens, const int32_t* ngram_tokens,
                                 const double* logp, const double* bow, double lm_weight, double length_bonus, double unk_logp,
                                 int32_t vocab, int32_t* out_len, int32_t* out_tokens, double* out_score, int32_t* out_src_row,
                                 int32_t* out_src_slot, int32_t* out_ctx_state, double* out_ctx_score, int32_t* out_ng_state,
                                 double* out_ng_score);
/* The same through ONE prefix_merge launch with the model that is set on the context (none: RNNT_ERR_STATE) and, when use_context
 * != 0, its graph (none: RNNT_ERR_STATE); an n-gram state outside [-1, nodes) or a candidate token outside the model's vocabulary:
 * RNNT_ERR_ARG.  Synchronises. */
int rnnt_prefix_merge_ngram_device(rnnt_ctx* ctx, int32_t n_hyp, const int32_t* hyp_len, const int32_t* hyp_tokens,
                                   const double* hyp_score, const int32_t* hyp_ctx_state, const double* hyp_ctx_score,
                                   const int32_t* hyp_ng_state, const double* hyp_ng_score, const float* top_lp, const int32_t* top_tok,
                                   int32_t k, int32_t blank, int32_t beam_size, int32_t use_context, int32_t* out_len,
                                   int32_t* out_tokens, double* out_score, int32_t* out_src_row, int32_t* out_src_slot,
                                   int32_t* out_ctx_state, double* out_ctx_score, int32_t* out_ng_state, double* out_ng_score,
                                   void* stream);
/* The pool calls of the transducer prefix search plus use_ngram (the two advancing calls) or ngram_scores_host [cap_hyps] (the read;
 * may be NULL).  The rows also keep an n-gram state (int) and score (f64) per hypothesis in both buffer sets, allocated with the
 * rest, counted by rnnt_live_device_bytes, released by rnnt_destroy.  A slot's first advancing call fixes use_ngram together with
 * the beam, the two weights and use_context until its reset; a differing value: RNNT_ERR_ARG.  use_ngram without a model:
 * RNNT_ERR_STATE.  rnnt_ngram_set starts a model generation: a search fused under an older one is refused with RNNT_ERR_STATE
 * (advance, and read with final != 0) until its slot is reset; unfused searches go on.  The context keeps ONE model for this search
 * and the CTC prefix search, as it keeps one graph.  Every refusal is decided before the first launch and changes nothing.  final
 * != 0 adds the end term (after context finalize), final == 0 returns the running n-gram score; either way scores_host holds the
 * totals.  A slot that fuses no model reads n-gram scores 0.  A call lists slots of one use_ngram.  The calls without the suffix
 * are these calls with use_ngram = 0. */
int rnnt_pool_prefix_frames_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t,
                                  int32_t beam_size, float ctc_weight, float transducer_weight, int32_t use_context, int32_t use_ngram,
                                  void* stream);
int rnnt_pool_chunk_prefix_ngram(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* fbank_dev,
                                 int32_t chunk_frames, const int32_t* offsets_host, const int32_t* required_host, int32_t beam_size,
                                 float ctc_weight, float transducer_weight, int32_t use_context, int32_t use_ngram, int32_t* frames_out,
                                 void* stream);
int rnnt_stream_get_prefix_ngram(rnnt_ctx* ctx, int32_t slot, int32_t final, int32_t cap_hyps, int32_t cap_tokens, int32_t* n_hyp,
                                 int32_t* lens_host, int32_t* tokens_host, double* scores_host, double* ctx_scores_host,
                                 double* ngram_scores_host, float* h_host, float* c_host, void* stream);

/* -- teacher-forced scoring: how likely is a GIVEN transcript (forward only; rnnt_transducer_loss below has gradients) ----------------------------------- */
/* Transducer negative log-likelihood: the RNN-T term of the reference's forward with texts (model/online_rnnt_model.py:240-255),
 * torchaudio.functional.rnnt_loss(reduction="none") -- minus the log of the sum over all monotonic alignments; its `clamp` only
 * touches gradients.  Per row b: joint.enc_ffn of its frames, the predictor over [blank, y_1 .. y_Umax] from the zero state
 * (add_blank + predictor(ys_in_pad), model/component/transducer.py:8-19; Umax + 1 steps of rnnt_predictor_step's GEMMs),
 * joint.pred_ffn, then ONE lattice kernel that keeps the log-softmax in its accumulators and writes only the two values the
 * recursion reads per cell -- pick[b][t][u][0] = log P(blank | t, u), pick[b][t][u][1] = log P(y_{u+1} | t, u) -- and the
 * alpha recursion in f64 (anti-diagonal wavefront, one workgroup per row).  One copy of B doubles, one synchronisation.
 *   enc_dev [B, T, 256] device; enc_lens_host [B] (T_b in [1, T]); targets_host [B, Umax] int32; target_lens_host [B] (U_b in
 *   [0, Umax]); nll_host [B] double; pick_dev: NULL, or device float [B, T, Umax + 1, 2] that receives the picked lattice
 *   (for every cell t < T_b, u <= U_b, label slot u < U_b: bitwise rnnt_joint(mode 1) at those two columns; other cells undefined).
 * Rows need not be distinct utterances: the same frames with B transcripts is hypothesis rescoring (rnnt_transducer_nll_nbest
 * does that without repeating the frames).  Entries of targets_host
 * beyond a row's length, and frames beyond T_b, are never read into a result.  Like rnnt_joint the call leaves streaming, pool
 * and beam state alone.  Exact-f32 mode and vocabularies outside the lattice kernel's range (> 416 or not a multiple of 4)
 * materialise the whole log-softmax lattice in a grow-only buffer and gather the two columns: same values, slow by design.
 * Refusals, all decided on the host before the first launch: null pointer, B < 1, T_b outside [1, T], U_b outside [0, Umax], a
 * label outside [0, vocab) or equal to blank_id inside a row's length: RNNT_ERR_ARG; Umax > 255 or a lattice beyond the context
 * scratch (rnnt_joint's check): RNNT_ERR_SHAPE; weights not finalized: RNNT_ERR_STATE. */
int rnnt_transducer_nll(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                        const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, double* nll_host, float* pick_dev,
                        void* stream);
/* CTC negative log-likelihood: OnlineCTC.forward's nn.CTCLoss (model/online_rnnt_model.py:22-32) with reduction="none" on
 * log_softmax(ctc_lo(enc)) -- rnnt_ctc_logprobs over the B*T frames, then the forward recursion over the 2 L_b + 1 extended
 * states in f64 (one workgroup per row).  Same arguments, ranges and refusals as rnnt_transducer_nll (L_b <= Umax <= 255); a
 * transcript its frames cannot hold (fewer frames than labels plus adjacent repeats) gives +inf.  RNNT_ERR_STATE without
 * ctc_head.ctc_lo.{weight,bias}.  Synchronises. */
int rnnt_ctc_nll(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                 const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, double* nll_host, void* stream);

/* -- training: the transducer loss WITH its gradient over a caller's joint lattice (torchaudio.functional.rnnt_loss) -------------- */
/* The three entry points take no context: a loss needs no weights and no model, so a refusal is its status code alone.
 * Per row b the loss is rnnt_transducer_nll's likelihood -- minus the log of the sum over all monotonic alignments -- computed from
 * logits [B, T, Umax + 1, V] float32 (what rnnt_joint(mode 0) and the reference's joint write), and grad is d nll_b / d logits:
 *   loss_pick: one pass over the valid cells (t < T_b, u <= U_b): the max-subtracted log-sum-exp over V in a fixed order (no
 *     atomics: two calls agree bit for bit), lse [B, T, U1] and pick [B, T, U1, 2] = (logit_blank - lse, logit_{y_{u+1}} - lse) in
 *     rnnt_transducer_nll's layout (label slot for u < U_b only);
 *   transducer_alpha_beta: rnnt_transducer_nll's forward recursion and its mirror image, beta[T_b-1,U_b] = pick_blank, beta[t,u] =
 *     logaddexp(beta[t+1,u] + pick_blank[t,u], beta[t,u+1] + pick_label[t,u]), both f64 and both stored; nll_b = -beta[0,0];
 *   loss_coef, loss_grad: with p_k = exp(logit_k - lse) and logZ = beta[0,0], g_k = p_k exp(alpha + beta - logZ), minus
 *     exp(alpha + pick_blank + beta[t+1,u] - logZ) at k = blank (at t = T_b - 1 only for u = U_b, with beta[T_b,U_b] := 0), minus
 *     exp(alpha + pick_label + beta[t,u+1] - logZ) at k = y_{u+1} (u < U_b); clamp > 0 clamps every g_k to [-clamp, clamp].
 * float32 lse, picks, p_k and the three per-cell factors; f64 recursions and exponents.  The lattice is read twice and written once.
 *   logits_dev [B, T, Umax + 1, V] device, 16-byte aligned; targets_host [B, Umax] int32 (may be NULL when Umax = 0);
 *   logit_lens_host [B] (T_b in [1, T]); target_lens_host [B] (U_b in [0, Umax]); V >= 2 is any size; blank in [0, V);
 *   fused_log_softmax = 0: the input holds log-probabilities already (lse taken as 0, no p_k term: the gradient with respect to them);
 *   nll_dev [B] double, device; grad_dev: NULL (value only: the same nll bit for bit), or device float [B, T, Umax + 1, V], 16-byte
 *   aligned, EVERY element written: exactly 0 outside the valid cells; workspace_dev: device, 16-byte aligned, at least the bytes
 *   rnnt_transducer_loss_workspace(B, T, Umax + 1) reports.  It begins with [B] doubles that receive -(alpha[T_b-1,U_b] +
 *   pick_blank), the same likelihood from the forward recursion; the rest (alpha, beta, factors, pick, lse, lengths, targets) is scratch.
 * Cells outside the valid region, and targets beyond a row's length, are never read: they may hold anything, NaN included.
 * One upload of lengths and targets (an asynchronous copy from pageable host memory, which the runtime may complete before it
 * returns), then four launches (two without grad_dev) on `stream`; no stream or device synchronisation, the stream orders
 * the outputs.  Refusals, all decided on the host before the first launch, changing nothing: a null pointer, a misaligned device
 * pointer, B < 1, T_b outside [1, T], U_b outside [0, Umax], V < 2, blank outside [0, V), a label outside [0, V) or equal to blank
 * inside a row's length: RNNT_ERR_ARG; Umax > 255, B * T * (Umax + 1) >= 2^31 - 1, a workspace that is too small: RNNT_ERR_SHAPE. */
int rnnt_transducer_loss_workspace(int32_t B, int32_t T, int32_t U1, int64_t* bytes_out);
int rnnt_transducer_loss(const float* logits_dev, const int32_t* targets_host, const int32_t* logit_lens_host,
                         const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank,
                         int32_t fused_log_softmax, float clamp, double* nll_dev, float* grad_dev, void* workspace_dev,
                         int64_t workspace_bytes, void* stream);
/* rnnt_transducer_loss over a lattice of 16-bit elements, read and written as such: elem names the type of logits_dev AND grad_dev
 * (RNNT_LOSS_F32 float, RNNT_LOSS_BF16 bfloat16, RNNT_LOSS_F16 IEEE half), every other argument is rnnt_transducer_loss's.  Each
 * element is widened to float32 exactly on load; lse, picks, p_k, g_k and the clamp are the float32 arithmetic above, the
 * recursions f64; g_k is rounded ONCE, to nearest even, to the element type at the store (zeros outside the valid cells).  nll_dev
 * stays double [B]; the workspace and rnnt_transducer_loss_workspace do not depend on elem.  A 16-bit row is single elements up to
 * the first 16-byte boundary, vectors of 8, single elements (at most 7 either side), so logits_dev and grad_dev are 16-byte aligned
 * as before.  elem = RNNT_LOSS_F32 IS rnnt_transducer_loss (which forwards here): the same launches, the same bits.  Refusals as
 * rnnt_transducer_loss, plus an elem that is none of the three: RNNT_ERR_ARG, decided first, before any pointer is followed. */
#define RNNT_LOSS_F32 0
#define RNNT_LOSS_BF16 1
#define RNNT_LOSS_F16 2
int rnnt_transducer_loss_elem(const void* logits_dev, const int32_t* targets_host, const int32_t* logit_lens_host,
                              const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank,
                              int32_t elem, int32_t fused_log_softmax, float clamp, double* nll_dev, void* grad_dev,
                              void* workspace_dev, int64_t workspace_bytes, void* stream);
/* The same loss as a pure C++ function (no context, no GPU), f64 throughout over the float32 logits: logits_host as logits_dev,
 * nll_host [B] double, grad_host NULL or double [B, T, Umax + 1, V] (0 outside the valid cells).  Same ranges and refusals, without
 * the alignment and workspace ones; a refused call writes nothing. */
int rnnt_transducer_loss_host(const float* logits_host, const int32_t* targets_host, const int32_t* logit_lens_host,
                              const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V, int32_t blank,
                              int32_t fused_log_softmax, float clamp, double* nll_host, double* grad_host);

/* -- training: the CTC loss WITH its gradient (torch.nn.functional.ctc_loss; the reference's OnlineCTC.forward after ctc_lo,
 * model/online_rnnt_model.py:22-32) ------------------------------------------------------------------------------------------- */
/* Context-free like rnnt_transducer_loss: the caller's buffers and a stream, no allocation, no synchronisation, a refusal is its
 * status code alone.  Per row b the loss is rnnt_ctc_nll's likelihood -- minus the log of the sum over all paths of T_b frames that
 * collapse to the row's L_b labels -- over the S = 2 L_b + 1 extended states (blank, y_1, blank, .., y_L, blank), and grad is
 * d nll_b / d input:
 *   ctc_loss_pick: one pass over the valid frames (t < T_b): the max-subtracted float32 log-sum-exp over V (fused_log_softmax) and
 *     pick [B, T, Lmax + 1] = (lp_blank, lp_{y_1}, .., lp_{y_L}), lp = input - lse;
 *   ctc_alpha_beta: rnnt_ctc_nll's forward recursion and its mirror image from the last frame, both f64, both stored, each holding
 *     its own frame's lp (torch's convention); nll_b = -logaddexp(alpha[T_b-1][S-1], alpha[T_b-1][S-2]); +inf for a transcript its
 *     frames cannot hold (T_b < L_b + adjacent repeats);
 *   ctc_loss_occ: occ[t, k] = sum over the states s on column k of exp(alpha_t[s] + beta_t[s] - lp[t, k] + nll_b), one thread per
 *     (frame, distinct column) adding its states in ascending order (f64) -- a repeated label and the blank put several states on
 *     one column; the table of columns and states is built on the host from the host targets.  No floating-point atomics;
 *   ctc_loss_grad: g[t, k] = p_k - occ[t, k] with p_k = exp(input_k - lse) (fused), or -occ[t, k] (the input holds log-probabilities),
 *     every element of [B, T, V] written exactly once; EXACTLY 0 for frames t >= T_b and for every frame of a row whose nll is +inf
 *     (a deliberate departure: torch writes NaN into such a row unless zero_infinity is set).
 * Which lane sums which columns depends on V alone, not on the strides, the alignment or the element type: two calls agree bit for
 * bit, the three layouts below agree bit for bit, and a 16-bit input gives the nll bits of the float32 call on the widened input and
 * that call's gradient rounded once, to nearest even.
 *   logits_dev: device, 16-byte aligned; frame (b, t) is the V elements from element b stride_b + t stride_t (unit stride over V; the
 *   rows themselves may start on any element).  stride_b, stride_t >= V, and stride_b >= T stride_t (a contiguous [B, T, V]) or
 *   stride_t >= B stride_b (a contiguous [T, B, V], or the transposed view the reference passes): all run without a copy; the gradient
 *   is written with the same strides.  elem: RNNT_LOSS_F32 / _BF16 / _F16, the type of logits_dev AND grad_dev, widened exactly on load.
 *   targets_host [B, Lmax] int32 (may be NULL when Lmax = 0; entries beyond a row's length are never read); logit_lens_host [B] (T_b in
 *   [1, T]); target_lens_host [B] (L_b in [0, Lmax]); V >= 2; blank in [0, V); nll_dev [B] double, device; grad_dev: NULL (value only:
 *   the same nll bit for bit, B workgroups of the forward recursion alone, two launches) or device, 16-byte aligned; workspace_dev:
 *   device, 16-byte aligned, at least the bytes rnnt_ctc_loss_workspace reports.  With grad_dev it begins with [B] doubles that receive
 *   -logaddexp(beta[0][0], beta[0][1]), the same likelihood from the backward recursion (in the convention where beta leaves its own
 *   frame out: -logaddexp(beta[0][0] + lp[0][blank], beta[0][1] + lp[0][y_1])); the rest is scratch.
 * One upload of lengths, targets and the column tables (an asynchronous copy from pageable host memory), then four launches (two
 * without grad_dev) on `stream`, whatever the data.  Profile tags 51 - 54 name the four launches; without a context
 * rnnt_profile_begin cannot select them.  Refusals, all decided on the host before the first launch, changing nothing: an elem that is
 * none of the three (decided first), a null or misaligned pointer, B < 1, T_b outside [1, T], L_b outside [0, Lmax], V < 2, blank
 * outside [0, V), a label outside [0, V) or equal to blank inside a row's length, a stride < V, overlapping rows: RNNT_ERR_ARG;
 * Lmax > 255, B * T * (2 Lmax + 1) >= 2^31 - 1, a workspace that is too small: RNNT_ERR_SHAPE. */
int rnnt_ctc_loss_workspace(int32_t B, int32_t T, int32_t Lmax, int64_t* bytes_out);
int rnnt_ctc_loss_elem(const void* logits_dev, int64_t stride_b, int64_t stride_t, const int32_t* targets_host,
                       const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V,
                       int32_t blank, int32_t elem, int32_t fused_log_softmax, double* nll_dev, void* grad_dev, void* workspace_dev,
                       int64_t workspace_bytes, void* stream);
/* elem = RNNT_LOSS_F32: the same launches, the same bits. */
int rnnt_ctc_loss(const float* logits_dev, int64_t stride_b, int64_t stride_t, const int32_t* targets_host,
                  const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V,
                  int32_t blank, int32_t fused_log_softmax, double* nll_dev, float* grad_dev, void* workspace_dev,
                  int64_t workspace_bytes, void* stream);
/* The same loss as a pure C++ function (no context, no GPU), f64 throughout over the float32 input with the same strides: nll_host [B]
 * double (+inf for an infeasible row), grad_host NULL or double with the input's strides (only the V elements of each frame are
 * written; 0 in padding frames and infeasible rows).  Same ranges and refusals, without the alignment and workspace ones; a refused
 * call writes nothing. */
int rnnt_ctc_loss_host(const float* logits_host, int64_t stride_b, int64_t stride_t, const int32_t* targets_host,
                       const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Lmax, int32_t V,
                       int32_t blank, int32_t fused_log_softmax, double* nll_host, double* grad_host);

/* -- the joint lattice with gradients, for training (TransducerJoint.forward, model/component/joint.py:48-69, prejoin linear / add /
 * tanh): the step in front of rnnt_transducer_loss.  No context, no finalized weights: the weights are the trainer's own float32
 * tensors and change every step.  With e = joint.enc_ffn(enc) [B, T, 256], p = joint.pred_ffn(pred) [B, U1, 256], W = joint.ffn_out.weight
 * [V, 256], b = joint.ffn_out.bias [V], M = B T U1 cells (u fastest):
 *   forward   logits[b,t,u,:] = tanh(e[b,t,:] + p[b,u,:]) W^T + b   [B, T, U1, V] float32: pack_joint_w packs W into the workspace,
 *             joint_prescale forms JR_PRESCALE e and JR_PRESCALE p there, and the unchanged joint_lattice_rows<2, false, false> (bf16x3,
 *             raw logits) writes the lattice: tanh(e + p) exists in registers only.
 *   backward  for g = d loss / d logits [B, T, U1, V] float32:  h = tanh(e + p) recomputed as the forward formed it, dh = g W,
 *             dz = dh (1 - h^2), d_e[b,t,:] = sum_u dz, d_p[b,u,:] = sum_t dz, dW[v,k] = sum_m g[m,v] h[m,k], db[v] = sum_m g[m,v],
 *             all float32, every element written.  Both contractions are bf16x3 MFMAs (two bf16 planes per operand, three products,
 *             float32 accumulation: bf16 planes keep the exponent range a gradient scaled by 1 / B needs); tanh, 1 - h^2 and the
 *             sums over u, t and cells are float32.  No atomics: sums that cross workgroups go through partial slabs in the workspace
 *             and are added in a fixed order, so two calls on the same inputs agree bit for bit.  Nothing of M x 256 or M x V
 *             elements is written.  logit_lens_host [B] (T_b in [1, T]) and target_lens_host [B] (U_b in [0, U1 - 1]) may each be NULL
 *             (every frame / every u counts); cells with t >= T_b or u > U_b are never read in g and contribute exact zeros.
 * Ranges (joint_lattice_rows'): the joint width is 256; 4 <= V <= 416 with V % 4 == 0; M < 2^31 - 64.  Every device pointer is 16-byte
 * aligned.  The workspace serves either direction (the backward does not need the forward's contents):
 *   bytes = 425984 + 4 max(256 B (T + U1) + 4,  4 ceil(B / 2) + 256 (NUB B T + NC B U1 + NS V) + NS V)   with
 *   NUB = ceil(U1 / 16), TC = 4 ceil(ceil(T / max(1, floor(512 / (B NUB)))) / 4), NC = ceil(T / TC),
 *   CS = 32 ceil(ceil(M / 32) / max(1, floor(512 / ceil(V / 64)))), NS = ceil(M / CS)
 * (NS V 1 KiB <= 32 MiB + V KiB whatever M).  A call allocates nothing and synchronises nothing: launches (and the backward's one
 * upload of the lengths, from pageable memory) on `stream`.  Refusals, decided on the host before the first launch, changing nothing:
 * a null or misaligned pointer, B, T or U1 < 1, a length outside its range: RNNT_ERR_ARG; V outside its range, M too large, a
 * workspace too small: RNNT_ERR_SHAPE. */
int rnnt_joint_lattice_workspace(int32_t B, int32_t T, int32_t U1, int32_t V, int64_t* bytes_out);
int rnnt_joint_lattice_forward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, int32_t B, int32_t T,
                               int32_t U1, int32_t V, float* logits_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);
int rnnt_joint_lattice_backward(const float* e_dev, const float* p_dev, const float* w_dev, const float* g_dev,
                                const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t U1,
                                int32_t V, float* de_dev, float* dp_dev, float* dw_dev, float* db_dev, void* workspace_dev,
                                int64_t workspace_bytes, void* stream);
/* The backward as a pure C++ function (no context, no GPU): f64 throughout over the float32 inputs, outputs double [B, T, 256],
 * [B, U1, 256], [V, 256], [V].  Same ranges and refusals, without the alignment and workspace ones; a refused call writes nothing. */
int rnnt_joint_lattice_backward_host(const float* e_host, const float* p_host, const float* w_host, const float* g_host,
                                     const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t U1,
                                     int32_t V, double* de_host, double* dp_host, double* dw_host, double* db_host);

/* -- the fused transducer joint and loss: train without the [B, T, U1, V] lattice ------------------------------------------------ */
/* nll_b = the transducer loss (rnnt_transducer_loss, fused log-softmax) of logits[b,t,u,:] = tanh(e[b,t,:] + p[b,u,:]) W^T + bias
 * (rnnt_joint_lattice_forward), and in a second call its gradients, with neither the lattice nor its gradient ever stored: the
 * lattice is recomputed in registers three times (forward, d_e / d_p, dW / db).  Context-free, the caller's buffers, a stream; no
 * allocation, no synchronisation.  U1 = Umax + 1, M = B T U1 cells.
 *   forward   pack_joint_w, joint_prescale, the pick form of joint_lattice_rows (bf16x3) storing per cell the two picked
 *             log-probabilities and lse, transducer_alpha_beta (f64), loss_coef.  nll_dev [B] f64 = -beta[0,0]; the cross-check
 *             -(alpha[T_b-1,U_b] + pick) lies at the head of the workspace ([B] f64).  `state` receives what the backward needs:
 *             coef [M][4] floats (lse, occupancy, blank term, label term) and the device copy of lengths and targets.
 *   backward  g = clamp(d nll_b / d logits) row_scale[b] (clamp <= 0: none; the order of rnnt_transducer_loss followed by a scaling)
 *             is formed in registers from the recomputed logits and `state`, and contracted as in rnnt_joint_lattice_backward:
 *             de [B, T, 256], dp [B, U1, 256], dw [V, 256], db [V] float32, every element written.  row_scale_dev [B] float32 is
 *             d loss / d nll_b on the device (dW and db sum over batch rows, so it cannot be applied afterwards).  No host arrays,
 *             no upload.  No atomics: two calls on the same inputs agree bit for bit.  Cells with t >= T_b or u > U_b contribute
 *             exact zeros and neither e, p nor state of such a cell is read.
 * Ranges (the intersection of the two families): the joint width is 256; 4 <= V <= 416 with V % 4 == 0; Umax <= 255; M < 2^31 - 64;
 * blank in [0, V); labels in [0, V) and never the blank; T_b in [1, T], U_b in [0, Umax].  Every device pointer is 16-byte aligned.
 *   state_bytes = 16 M + 16 ceil((2 B + B max(Umax, 1)) / 4)
 *   work_bytes  = max(8 (B + B % 2) + 16 M + 425984 + 4 (256 B (T + U1) + 4 + 2 M + 4 ceil(M / 4)),
 *                     65536 ceil(V / 32) + 4 (256 (NUB B T + NC B U1 + NS V) + NS V))       (NUB, NC, NS of rnnt_joint_lattice_workspace)
 * Neither holds a term in M V.  Refusals, decided on the host before the first launch, changing nothing: a null or misaligned
 * pointer, B or T < 1, Umax < 0, a blank, length or label outside its range: RNNT_ERR_ARG; V outside its range, Umax > 255, M too
 * large, state_bytes or work_bytes too small: RNNT_ERR_SHAPE. */
int rnnt_joint_loss_workspace(int32_t B, int32_t T, int32_t U1, int32_t V, int64_t* work_bytes, int64_t* state_bytes);
int rnnt_joint_loss_forward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, const int32_t* targets_host,
                            const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax,
                            int32_t V, int32_t blank, double* nll_dev, void* state_dev, int64_t state_bytes, void* work_dev,
                            int64_t work_bytes, void* stream);
int rnnt_joint_loss_backward(const float* e_dev, const float* p_dev, const float* w_dev, const float* b_dev, const void* state_dev,
                             int64_t state_bytes, const float* row_scale_dev, float clamp, int32_t B, int32_t T, int32_t Umax,
                             int32_t V, int32_t blank, float* de_dev, float* dp_dev, float* dw_dev, float* db_dev, void* work_dev,
                             int64_t work_bytes, void* stream);
/* The same function in plain C++ (no context, no GPU): float64 throughout over the float32 inputs -- the host sides of the lattice,
 * of rnnt_transducer_loss_host and of rnnt_joint_lattice_backward_host composed with nothing rounded between them (on the host the
 * lattice and its gradient exist, in f64).  row_scale_host [B] f64, or NULL: nll_host [B] only, the four outputs untouched.  Outputs
 * double [B, T, 256], [B, U1, 256], [V, 256], [V].  Same ranges and refusals, without the alignment, state and workspace ones; a
 * refused call writes nothing. */
int rnnt_joint_loss_host(const float* e_host, const float* p_host, const float* w_host, const float* b_host, const int32_t* targets_host,
                         const int32_t* logit_lens_host, const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, int32_t V,
                         int32_t blank, float clamp, const double* row_scale_host, double* nll_host, double* de_host, double* dp_host,
                         double* dw_host, double* db_host);

/* -- the predictor's LSTM layer over a whole label sequence, with gradients -------------------------------------------------------- */
/* torch.nn.LSTM(256, 256, one layer, batch_first) in torch's layout: x [B, U1, 256], w_ih and w_hh [1024, 256], b_ih and b_hh [1024],
 * gate order i, f, g, o; h0, c0 [B, 256] or NULL (zeros); out [B, U1, 256]; hn, cn [B, 256] or NULL.  float32 throughout, with the
 * activations of the inference predictor, so the sequence forward and the step call differ in summation order only.  Context-free,
 * the caller's buffers, a stream; no allocation, no synchronisation; the launch count does not depend on U1.
 *   forward   lstm_pack_whh, lstm_gemm (xg = x W_ih^T + b_ih + b_hh for all B U1 rows, exact-f32 MFMA), then ONE recurrence launch
 *             lstm_seq_fwd that walks u = 0 .. U1-1: one workgroup per 4 batch rows, none waits on another.  With state_dev it saves
 *             per row and step the activated i, f, g, o and c ([B, U1, 5, 256] floats) for the backward; NULL: forward only.
 *   backward  ONE recurrence launch lstm_seq_bwd walking u = U1-1 .. 0 (dG [B U1, 1024] into the workspace, dh0 and dc0 [B, 256] or
 *             NULL), then dx = dG W_ih, dW_ih = dG^T x, dW_hh = dG^T h_prev (out shifted by one step behind h0) as slabs of 256 rows
 *             summed in slab order, db = sum dG (it is both db_ih and db_hh).  No atomics: two calls agree bit for bit.  c0_dev must
 *             be the forward's (the forget gate's gradient at step 0 needs it).
 * lens_host [B] or NULL: row b runs lens[b] steps (1..U1).  Beyond them x and dout are never read, out and dx are exactly 0, and
 * hn / cn / dh0 / dc0 belong to the row's own first and last valid steps.
 *   state_bytes = 5120 B U1
 *   work_bytes  = 4 (4 ceil(B / 4) + 262144 + 1024 B U1 + 525312 ceil(B U1 / 256))
 * Refusals, decided on the host before the first launch, changing nothing: a null required pointer, a pointer that is not 16-byte
 * aligned, B < 1, U1 < 1, a length outside [1, U1]: RNNT_ERR_ARG; U1 > 256, 1280 B U1 >= 2^31 - 1, work_bytes or state_bytes too
 * small: RNNT_ERR_SHAPE. */
int rnnt_lstm_workspace(int32_t B, int32_t U1, int64_t* work_bytes, int64_t* state_bytes);
int rnnt_lstm_forward(const float* x_dev, const float* w_ih_dev, const float* w_hh_dev, const float* b_ih_dev, const float* b_hh_dev,
                      const float* h0_dev, const float* c0_dev, const int32_t* lens_host, int32_t B, int32_t U1, float* out_dev,
                      float* hn_dev, float* cn_dev, void* state_dev, int64_t state_bytes, void* work_dev, int64_t work_bytes,
                      void* stream);
int rnnt_lstm_backward(const float* x_dev, const float* w_ih_dev, const float* w_hh_dev, const float* h0_dev, const float* c0_dev,
                       const float* out_dev, const void* state_dev, int64_t state_bytes, const float* dout_dev,
                       const int32_t* lens_host, int32_t B, int32_t U1, float* dx_dev, float* dw_ih_dev, float* dw_hh_dev,
                       float* db_dev, float* dh0_dev, float* dc0_dev, void* work_dev, int64_t work_bytes, void* stream);
/* Both directions in plain C++ (no context, no GPU): float64 throughout over the float32 inputs.  out_host [B, U1, 256], hn_host and
 * cn_host [B, 256] or NULL.  dout_host NULL: forward only, the six gradient outputs untouched; else dx_host [B, U1, 256], dw_ih_host
 * and dw_hh_host [1024, 256], db_host [1024] are required and dh0_host, dc0_host [B, 256] may be NULL.  Same ranges and refusals,
 * without the alignment, state and workspace ones; a refused call writes nothing. */
int rnnt_lstm_host(const float* x_host, const float* w_ih_host, const float* w_hh_host, const float* b_ih_host, const float* b_hh_host,
                   const float* h0_host, const float* c0_host, const int32_t* lens_host, int32_t B, int32_t U1, const float* dout_host,
                   double* out_host, double* hn_host, double* cn_host, double* dx_host, double* dw_ih_host, double* dw_hh_host,
                   double* db_host, double* dh0_host, double* dc0_host);

/* -- the attention core of an encoder layer (relative positions, chunk mask), with gradients ----------------------------------------- */
/* The reference's RelPositionMultiHeadedAttention between its Linears (wenet/transformer/attention.py:364-420, rel_shift commented
 * out there, so the positional term is indexed by the key's absolute position), H = 4 heads of 64:
 *   s[b,h,i,j] = ((q[b,i,h,:] + u[h,:]) . k[b,j,h,:] + (q[b,i,h,:] + vb[h,:]) . p[j,h,:]) / 8
 *   visible(b,i,j) = j < len_b and (chunk_size <= 0 or j < min(T, (i / chunk_size + 1) chunk_size))
 *                    and (chunk_size <= 0 or num_left_chunks < 0 or j >= (i / chunk_size - num_left_chunks) chunk_size)
 *   a = softmax of s over the visible j (0 at hidden j; all 0 for a row with no visible key);  out[b,i,h,:] = sum_j a[b,h,i,j] v[b,j,h,:]
 * q, k, v, out, dout, dq, dk, dv [B, T, 256] with head h at columns 64 h .. 64 h + 63 (as linear_q writes and linear_out reads);
 * p, dp [T, 256] (linear_pos(pos_emb[0])); u, vb, du, dvb [4, 64] (pos_bias_u, pos_bias_v).  All float32, contiguous, 16-byte
 * aligned.  Only keys are masked: every query row i < T is live, padded ones included.  Keys and values at j >= len_b are never
 * read.  Context-free, the caller's buffers, a stream; no allocation, no synchronisation; nothing of T x T size reaches memory.
 *   forward   ONE launch attn_fwd: a wave per (b, h, 16 queries) walks the 16-key tiles inside the tile's window and len_b, online
 *             softmax.  With state_dev it saves one float32 log-sum-exp per (b, h, i) ([B, 4, T]; +inf marks a row with no visible
 *             key); NULL: forward only.
 *   backward  attn_delta (dout . out), attn_bwd_k (key-owned: dk, dv, the row's dp partial), attn_bwd_q (query-owned: dq, the tile's
 *             du and dvb partials), then dp summed over rows and du / dvb over (row, query tile) in index order.  The probabilities
 *             are recomputed from q, k, p and the saved log-sum-exp in both passes.  No atomics: two calls agree bit for bit.
 * Arithmetic: every contraction on v_mfma_f32_16x16x4_f32 (exact float32 products, float32 accumulation); max, exp, sums, delta,
 * ds in float32.  A probability is never formed from a hidden key (a select, not exp(-inf)).
 * lens_host [B] or NULL (every row T keys).  T is capped at 4096.  The lengths are copied from a host array of the call's own; with
 * more than 16384 rows the call waits for that copy (the stream) before it returns, the one case in which it synchronises.
 *   state_bytes = 16 B T
 *   work_bytes  = 4 (4 ceil(B / 4) + 260 B T + 512 B ceil(T / 16))
 * Refusals, decided on the host before the first launch, changing nothing: a null required pointer, a pointer that is not 16-byte
 * aligned, B < 1, T < 1, a length outside [1, T], num_left_chunks >= 0 with chunk_size <= 0: RNNT_ERR_ARG; T > 4096,
 * 256 B T >= 2^31 - 1, work_bytes or state_bytes too small: RNNT_ERR_SHAPE. */
int rnnt_rel_attention_workspace(int32_t B, int32_t T, int64_t* work_bytes, int64_t* state_bytes);
int rnnt_rel_attention_forward(const float* q_dev, const float* k_dev, const float* v_dev, const float* p_dev, const float* u_dev,
                               const float* vb_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size,
                               int32_t num_left_chunks, float* out_dev, void* state_dev, int64_t state_bytes, void* work_dev,
                               int64_t work_bytes, void* stream);
int rnnt_rel_attention_backward(const float* q_dev, const float* k_dev, const float* v_dev, const float* p_dev, const float* u_dev,
                                const float* vb_dev, const float* out_dev, const void* state_dev, int64_t state_bytes,
                                const float* dout_dev, const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size,
                                int32_t num_left_chunks, float* dq_dev, float* dk_dev, float* dv_dev, float* dp_dev, float* du_dev,
                                float* dvb_dev, void* work_dev, int64_t work_bytes, void* stream);
/* Both directions in plain C++ (no context, no GPU): float64 throughout over the float32 inputs; it holds one [T] row of scores.
 * out_host [B, T, 256].  dout_host NULL: forward only, the six gradient outputs untouched; else dq_host, dk_host, dv_host
 * [B, T, 256], dp_host [T, 256], du_host, dvb_host [4, 64] are required.  Same ranges and refusals, without the alignment, state
 * and workspace ones; a refused call writes nothing. */
int rnnt_rel_attention_host(const float* q_host, const float* k_host, const float* v_host, const float* p_host, const float* u_host,
                            const float* vb_host, const int32_t* lens_host, int32_t B, int32_t T, int32_t chunk_size,
                            int32_t num_left_chunks, const float* dout_host, double* out_host, double* dq_host, double* dk_host,
                            double* dv_host, double* dp_host, double* du_host, double* dvb_host);

/* -- two-pass decoding: a cheap first pass yields n-best, the transducer likelihood re-scores it (the reference's WeNet layer:
 * Transducer.transducer_attention_rescoring with _cal_transducer_score, wenet/transducer/transducer.py:160-185, 261-395) ------- */
/* rnnt_transducer_nll for N hypotheses per utterance WITHOUT repeating the utterance's frames N times: nll_host[b][n] is what
 * rnnt_transducer_nll defines for frames b and transcript (b, n), n < n_hyp_host[b]; entries n >= n_hyp_host[b] are 0.  The
 * hypotheses of an utterance lie side by side along U of one lattice -- pred [B][N * (Umax + 1)][256] -- so joint.enc_ffn runs over
 * the B*T frames once and the context scratch holds B*T + B*N*(Umax+1) rows instead of B*N*(T + Umax + 1).  The predictor runs
 * Umax + 1 steps over B*N rows (rows of missing hypotheses on blanks), the unchanged lattice kernel writes the picked lattice with
 * U = N * (Umax + 1), and transducer_alpha_nbest (one workgroup per (b, n), rnnt_transducer_nll's recursion in f64) reads cell
 * (t, u) of hypothesis n at ((b T + t) N (Umax+1) + n (Umax+1) + u) * 2.  One upload, one download of B*N doubles, one synchronisation.
 *   enc_dev [B, T, 256] device; enc_lens_host [B] (T_b in [1, T]); n_hyp_host [B] (in [1, N]); hyp_lens_host [B, N] (in [0, Umax];
 *   an empty hypothesis is valid); hyp_tokens_host [B, N, Umax] int32; nll_host [B, N] double; pick_dev: NULL, or device float
 *   [B, T, N * (Umax + 1), 2] that receives the picked lattice (valid cells as for rnnt_transducer_nll, per hypothesis: bitwise
 *   rnnt_joint(mode 1) over pred [B, N * (Umax + 1), 256] at those two columns).
 * Frames beyond T_b, tokens beyond a hypothesis' length, and lengths and tokens of rows n >= n_hyp_host[b] are never read into a
 * result.  Exact-f32 mode and vocabularies outside the lattice kernel's range take rnnt_transducer_nll's fallback with the same U.
 * Like rnnt_joint the call leaves streaming, pool, beam and CTC-prefix state alone.  Profile tags: 20 / 21 the predictor steps,
 * 13 / 22 the two projections, 40 the pick, 41 the recursion.
 * Refusals, all decided on the host before the first launch, changing nothing: null pointer, B < 1, N outside [1, 16], n_hyp outside
 * [1, N], T_b outside [1, T], a length outside [0, Umax], a label outside [0, vocab) or equal to blank_id inside a length:
 * RNNT_ERR_ARG; Umax > 255, B*T*256 + B*N*(Umax+1)*256 floats beyond the context scratch, or B*T*N*(Umax+1) >= 2^31 - 64:
 * RNNT_ERR_SHAPE; weights not finalized: RNNT_ERR_STATE. */
int rnnt_transducer_nll_nbest(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* n_hyp_host,
                              const int32_t* hyp_lens_host, const int32_t* hyp_tokens_host, int32_t B, int32_t T, int32_t N,
                              int32_t Umax, double* nll_host, float* pick_dev, void* stream);
/* The choice among one utterance's re-scored hypotheses as a pure C++ function (no context, no GPU): transducer.py:372-393 with
 * attn_weight = 0.  total_out[i] = first_scores[i] * first_weight + (-nll[i]) * transducer_weight, each product and the sum rounded
 * separately in f64; *best_out starts at 0 with -inf and moves on strict > only, so the first of equal totals wins and a NaN total
 * (-inf * 0.0, as in Python) is never chosen; if none compares greater *best_out is 0.  RNNT_ERR_ARG: null pointer or n_hyp < 1. */
int rnnt_rescore_select_host(int32_t n_hyp, const double* first_scores, const double* nll, double first_weight,
                             double transducer_weight, double* total_out, int32_t* best_out);

/* -- frames that outlive their chunk: the per-slot encoder-frame history of the stream pool ------------------------------------------ */
/* keep != 0: from now on every pool call that encodes `slot` (rnnt_pool_chunk in either mode, rnnt_pool_chunk_beam,
 * rnnt_pool_chunk_ctc_prefix) appends the slot's t' new encoder outputs -- the after_norm rows rnnt_get_enc_frames returns, before
 * the joint projection -- to a history [max_cache_frames][256] f32 of the slot (ONE extra launch per pool call, pool_hist_append,
 * and only when a listed slot keeps frames).  Valid on a slot that has not advanced since it was opened or reset (RNNT_ERR_STATE
 * otherwise: its first frames are gone); the context enters pool mode.  The history is an owning device buffer per slot,
 * max_cache_frames KB: allocated on the slot's first keep, reused by its later utterances, counted by rnnt_live_device_bytes, freed
 * by rnnt_destroy.  rnnt_stream_open clears its slot's flag and length, rnnt_streams_reset all: a slot keeps nothing unless asked
 * again.  A pool call that would take a kept slot past max_cache_frames is refused with RNNT_ERR_SHAPE before its first launch and
 * moves no slot.  keep == 0: the flag and the length are cleared (any time).  Does not synchronise. */
int rnnt_stream_keep_frames(rnnt_ctx* ctx, int32_t slot, int32_t keep, void* stream);
/* frames [from, len) of the slot's history, at most cap_frames, device to device into dst_dev [cap_frames, 256] on `stream`;
 * *n_out (optional) = len - from (0 when from >= len).  dst_dev may be NULL with cap_frames = 0 to query.  The length is the host's:
 * no synchronisation.  RNNT_ERR_STATE on a slot that keeps no frames. */
int rnnt_stream_get_frames(rnnt_ctx* ctx, int32_t slot, int32_t from, int32_t cap_frames, float* dst_dev, int32_t* n_out, void* stream);
/* The second pass of a streaming server: rnnt_transducer_nll_nbest over the kept frames of the n listed slots (distinct, each
 * keeping >= 1 frame).  pool_hist_gather stages their histories into a dense grow-only [n][Tmax][256] buffer (Tmax = the longest
 * history of the call; rows beyond a slot's length are never read), then that pipeline runs with B = n, T = Tmax, T_b = the
 * history lengths: n_hyp_host [n], hyp_lens_host [n, N], hyp_tokens_host [n, N, Umax], nll_host [n, N] as there.  The call only
 * reads slot state: searches and streams go on afterwards, so partial results may be re-scored mid-utterance.  Refusals as
 * rnnt_transducer_nll_nbest, plus RNNT_ERR_ARG for a duplicated or out-of-range slot and RNNT_ERR_STATE for a listed slot that
 * keeps no frames or has none yet; all before the first launch.  Synchronises. */
int rnnt_pool_rescore(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, const int32_t* n_hyp_host, const int32_t* hyp_lens_host,
                      const int32_t* hyp_tokens_host, int32_t N, int32_t Umax, double* nll_host, void* stream);

/* -- when is the caller done: endpoint detection per slot of the stream pool ------------------------------------------------------------ */
/* The rule has the shape of WeNet's runtime endpointer, on the CTC head's blank posterior per encoder frame.  Per-slot state, five
 * int32: frames, trailing, speech, rule, at -- all 0 after open / reset.  For every new encoder frame, in order, with lp = that
 * frame's blank log-posterior log_softmax(ctc_lo(enc))[blank_id] (f32 in every numerics mode) and
 * log_thr = (float)log((double)blank_threshold), computed once where the config is accepted:
 *     frames += 1
 *     if (lp > log_thr) trailing += 1; else { trailing = 0; speech += 1; }          -- a NaN counts as speech
 *     if (rule == 0) {
 *         r = (R1 > 0 && speech <  S && trailing >= R1) ? 1
 *           : (R2 > 0 && speech >= S && trailing >= R2) ? 2
 *           : (R3 > 0 && frames >= R3)                  ? 3 : 0;
 *         if (r) { rule = r; at = frames; }
 *     }
 * Rules are evaluated per frame, not per call; the first to fire is sticky and the counters run on, so a slot's state depends only on
 * its frames, never on how they were split into calls.  With all three rules off the slot only counts.  "Something was said" is the
 * CTC speech count, not "the decoder has tokens": one rule for every slot kind, and the device needs nothing from the decoders.  A
 * caller who wants the decoder-based form applies it on the host from the returned frames / trailing and its own tokens. */
typedef struct {
    float   blank_threshold;    /* in (0, 1): a frame is blank iff its CTC blank posterior exceeds it */
    int32_t min_speech_frames;  /* S >= 0: "something was said" once speech >= S                       */
    int32_t rule1_trailing;     /* R1: nothing said yet and trailing >= R1; 0 = rule off               */
    int32_t rule2_trailing;     /* R2: something said and trailing >= R2;   0 = rule off               */
    int32_t rule3_frames;       /* R3: frames >= R3;                        0 = rule off               */
} rnnt_endpoint_config;         /* 20 bytes */
/* cfg != NULL: from now on every pool call that encodes `slot` (rnnt_pool_chunk in either mode, rnnt_pool_chunk_beam,
 * rnnt_pool_chunk_ctc_prefix, rnnt_pool_chunk_prefix[_ctx]) advances the slot's state by its t' new frames: ONE extra launch per
 * pool call (pool_endpoint, after the history append), and only when a listed slot has endpointing on.  Valid on a slot that has not
 * advanced since it was opened or reset (RNNT_ERR_STATE otherwise); the state starts at zero and the context enters pool mode.
 * RNNT_ERR_STATE without finalized weights or without ctc_head.ctc_lo.*; RNNT_ERR_ARG for a threshold outside (0, 1), a negative
 * count or a slot out of range.  The config and state tables [max_streams] are reserved on the first use and counted by
 * rnnt_live_device_bytes.  rnnt_stream_open clears its slot's flag, rnnt_streams_reset all: a slot detects nothing unless asked
 * again.  cfg == NULL: endpointing off for the slot (any time).  Does not synchronise. */
int rnnt_stream_endpoint(rnnt_ctx* ctx, int32_t slot, const rnnt_endpoint_config* cfg, void* stream);
/* The seam: the states of the n_active listed slots (distinct, endpointing on) advance by t >= 1 caller-held encoder frames
 * enc_dev [n_active][t][256] (16-byte aligned), row i belonging to slots_host[i].  One launch, no synchronisation.  RNNT_ERR_ARG:
 * null pointer, n_active outside [1, max_streams], t < 1, a duplicated or out-of-range slot; RNNT_ERR_STATE: a listed slot with
 * endpointing off.  Every refusal happens before the launch and changes nothing. */
int rnnt_pool_endpoint_frames(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* enc_dev, int32_t t, void* stream);
/* state_host [n][5] = frames, trailing, speech, rule, at of each listed slot (distinct, endpointing on: RNNT_ERR_STATE otherwise).
 * ONE device-to-host copy of the state table for the whole call; the rows are picked on the host.  Synchronises. */
int rnnt_pool_get_endpoints(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, int32_t* state_host, void* stream);
/* out_dev [rows] = log_softmax(ctc_lo(enc))[blank_id] for enc_dev [rows, 256] (16-byte aligned): the stateless kernel under the
 * above.  f32 FMA arithmetic in every numerics mode, online (max, sum) over the vocabulary, nothing of size rows x vocab written.
 * Preconditions as rnnt_ctc_logprobs.  Does not synchronise. */
int rnnt_ctc_blank_logprob(rnnt_ctx* ctx, const float* enc_dev, int32_t rows, float* out_dev, void* stream);
/* The rule as a pure C++ function (no context, no GPU), the very function the kernel runs: state [5] advances by the t >= 0
 * log-posteriors blank_lp [t].  RNNT_ERR_ARG on a null pointer (blank_lp may be NULL when t = 0), t < 0 or a config
 * rnnt_stream_endpoint refuses. */
int rnnt_endpoint_scan_host(const float* blank_lp, int32_t t, const rnnt_endpoint_config* cfg, int32_t* state);

/* -- segments: the next utterance in a slot that stays open ------------------------------------------------------------------------------ */
/* What follows an endpoint.  A segment boundary ends one utterance in each of the n listed slots (distinct, in [0, n_streams)) and
 * starts the next without rnnt_stream_open: the slot, its configuration and its audio stream stay.  Per listed slot, in both flavours:
 *   greedy state      as rnnt_stream_open leaves it: both LSTM buffers 0, last token = blank, token count 0;
 *   beam              the one empty hypothesis with score 0 and zero state;
 *   prefix searches   the start state of rnnt_stream_ctc_prefix_reset / rnnt_stream_prefix_reset; the next advancing call may fix
 *                     another beam size, other weights, another use_context, and a biased one binds the graph current at that call;
 *   endpoint          the five counters 0; the config and the on flag stay;
 *   frame history     length 0; the keep flag and the buffer stay;
 *   segment record    index + 1, start_frame = the encoder frames the slot had encoded since it was opened (see below).
 * A state kind the context has never allocated costs nothing.
 * keep_encoder != 0 (continuous decoding): nothing of the encoder or the audio front-end of any slot is read or written -- K/V rows,
 * position (cache length, window start, ring position), both conv rings, the wave state.  The caller's offsets run on.
 * keep_encoder == 0: also the encoder state of rnnt_stream_open for the listed slots -- the conv rings of all layers as for a fresh
 * stream, an empty cache at position 0; the next chunk's offset is 0.  The wave front-end (carry, samples, frames, sample rate /
 * n_fft), the endpoint config and the keep flag survive.  This is how a slot outlives max_cache_frames and the positional table.
 * Cost: ONE async copy of the slot list and ONE launch whatever n and whatever state kinds exist; no synchronisation, no download;
 * enqueued on `stream` in order.  The context enters pool mode; slots not listed are untouched.
 * Refusals, all before the launch and changing nothing: RNNT_ERR_ARG for a null list, n outside [1, n_streams], a slot out of range
 * or listed twice; RNNT_ERR_STATE without weights / streams or with frames still buffered. */
int rnnt_pool_segment(rnnt_ctx* ctx, int32_t n, const int32_t* slots_host, int32_t keep_encoder, void* stream);
/* Host only: index_out = segments started in `slot` since rnnt_stream_open / rnnt_streams_reset (0: none), start_frame_out = the
 * encoder frames the slot had encoded, since then, when its current segment began.  The frame indices the getters return -- CTC
 * times, alignment emit frames, the endpoint's `at` -- are relative to the segment; add start_frame_out for the session's.  Either
 * pointer may be NULL.  RNNT_ERR_ARG for a slot outside [0, max_streams). */
int rnnt_stream_get_segment(rnnt_ctx* ctx, int32_t slot, int32_t* index_out, int32_t* start_frame_out);

/* -- forced alignment: WHERE in the frames each token of a given transcript lies (the reference's WeNet layer: force_align,
 * gen_ctc_peak_time, gen_timestamps_from_peak, DecodeResult.times; wenet/utils/ctc_utils.py) ------------------------------------ */
/* The best monotonic alignment of each row's transcript: the max-plus (Viterbi) twin of rnnt_transducer_nll's recursion in f64,
 * over the same picked lattice -- v[0,0] = 0, v[t,u] = max(v[t-1,u] + pick[t-1,u][0], v[t,u-1] + pick[t,u-1][1]),
 * best = v[T_b-1,U_b] + pick[T_b-1,U_b][0] -- with one-bit back-pointers and the back-trace in the same launch.  Where both moves
 * reach a cell with equal values the blank move (from (t-1,u)) wins; additions and comparisons only, so the result is bitwise its
 * float64 restatement (ctc_vr_amd.testing.transducer_align_ref), ties included.
 *   best_host [B] double: log-probability of the best path; emit_host [B, max(Umax, 1)] int32: emit[b][u] = the frame at which
 *   label u is emitted (non-decreasing in u), -1 for u >= U_b; nll_host: NULL, or [B] double that receives what
 *   rnnt_transducer_nll returns for the same arguments (transducer_alpha over the same lattice); pick_dev as there.
 * Other arguments, ranges and refusals as rnnt_transducer_nll; best_host and emit_host must not be NULL.  One upload, one
 * download, one synchronisation; streaming, pool and beam state are left alone. */
int rnnt_transducer_align(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                          const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, double* best_host,
                          int32_t* emit_host, double* nll_host, float* pick_dev, void* stream);
/* The same recursion over a lattice the caller already holds: pick_dev [B, T, Umax + 1, 2] device floats in
 * rnnt_transducer_nll's layout; only cells t < T_b, u <= U_b (label slot u < U_b) are read.  No labels, hence no label checks;
 * the other refusals as above (without the scratch limit: nothing is projected). */
int rnnt_transducer_align_pick(rnnt_ctx* ctx, const float* pick_dev, const int32_t* enc_lens_host, const int32_t* target_lens_host,
                               int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* emit_host, void* stream);
/* CTC forced alignment: rnnt_ctc_logprobs over the B*T frames, then the Viterbi twin of rnnt_ctc_nll's recursion in f64 over the
 * 2 L_b + 1 extended states: v_t[s] = max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2] if the labels differ) + lp[t][ext s]; among
 * equal values staying beats s-1, which beats s-2; the path ends in the last state if v[S-1] >= v[S-2], else in the last label.
 *   best_host [B] double; align_host [B, T] int32: the label of the state occupied at frame t, blank_id included (the per-frame
 *   form torchaudio's forced_align returns), -1 for t >= T_b.
 * A transcript its frames cannot hold gives best = -inf and a row of -1; it is no error (the mirror of rnnt_ctc_nll's +inf).
 * Arguments, ranges and refusals as rnnt_ctc_nll. */
int rnnt_ctc_align(rnnt_ctx* ctx, const float* enc_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                   const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, double* best_host, int32_t* align_host,
                   void* stream);
/* The same over log-probabilities the caller already holds: lp_dev [B, T, vocab] device floats (they need not normalise: the
 * recursion only adds).  Needs no CTC head; the other refusals as rnnt_ctc_align. */
int rnnt_ctc_align_logprobs(rnnt_ctx* ctx, const float* lp_dev, const int32_t* enc_lens_host, const int32_t* targets_host,
                            const int32_t* target_lens_host, int32_t B, int32_t T, int32_t Umax, double* best_host,
                            int32_t* align_host, void* stream);

/* Offline greedy search: basic_greedy_search (model/component/transducer.py:22-70) behind
 * OnlineRNNTModel.forward(audios, audio_lens) of a non-streaming model (model/online_rnnt_model.py:234-235,268):
 * full-context encoder + per-utterance greedy loop over its valid frames, <= n_steps symbols per frame (reference
 * default 64).  counts_host [B]; tokens_host [B, max_tokens] (may be NULL).  Streaming state is clobbered. */
int rnnt_greedy_search_full(rnnt_ctx* ctx, const float* fbank_dev, const int32_t* lens_host, int32_t B, int32_t T,
                            int32_t n_steps, int32_t* counts_host, int32_t* tokens_host, void* stream);

/* Feature front-end on the device: replaces extract_audio_features (data/dataloader.py:15-41) =
 * torchaudio MelSpectrogram(sample_rate, n_fft, n_mels=80, hop_length=512, hamming window, power 2, centred reflect
 * padding, HTK mel scale) + AmplitudeToDB().  wave_dev [B, n_samples] mono float32 on the device ->
 * out_dev [B, 1 + n_samples/512, 80] (the layout rnnt_encoder_chunk takes).  Independent of the model weights. */
int rnnt_fbank(rnnt_ctx* ctx, const float* wave_dev, int32_t B, int32_t n_samples, int32_t sample_rate, int32_t n_fft,
               float* out_dev, int32_t* frames_out, void* stream);

/* -- audio in for the stream pool: rnnt_fbank per slot, fed in packets -------------------------------------------------------------- */
/* AmplitudeToDB() has no top_db, so frame f depends on x[f*512 - n_fft/2, f*512 + n_fft/2) of the reflect-padded signal alone and the
 * features are computable frame by frame.  Per slot, the frames emitted since its reset are the rows of rnnt_fbank over the slot's
 * whole waveform, concatenated in order, nothing twice: hop 512, 80 mels, periodic Hamming window, power 2, centred, reflect
 * padding, dB with the 1e-10 clamp.  With N samples received and the utterance not final, the frames with f*512 + n_fft/2 <= N are
 * out, and none before N >= n_fft/2 + 1 (frame 0's left reflection reads sample n_fft/2).  At final the remaining frames up to
 * 1 + N/512 follow with the right reflection j -> 2(N-1) - j.  A final slot with N <= n_fft/2 emits nothing and is no error.
 *   wave_dev [n_active, n_samples] f32 device: row i holds samples_host[i] in [0, n_samples] new samples of slot slots_host[i];
 *   final_host[i] != 0: that slot's utterance ends with them (0 new samples: flush the tail);  a row with 0 samples and final == 0
 *   is a no-op;  out_dev [n_active, cap_frames, 80] f32 device, frames_host[i] rows of row i are written (the rest unspecified).
 * State per slot, allocated on the first call through the context's owning buffers: on the device the carry -- the samples a pending
 * frame or the final reflection can still read, x[max(0, f*512 - n_fft/2 - 1), N) for the next frame f, at most n_fft floats (the
 * final frame centred on N = k*512 reflects one sample before its own span) -- and on the host samples, frames, finished and the
 * (sample_rate, n_fft) the slot's first push fixed until its next reset.  rnnt_stream_open resets its slot, rnnt_streams_reset and
 * rnnt_stream_wave_reset(-1) all.  Any context works (weights are not needed).
 * Launches, whatever n_active: wave_stage (carry | new samples | reflections into 16-byte aligned zero-filled rows, a row's first new
 * frame at a fixed position), rnnt_fbank's DFT GEMM / power_spectrum / mel GEMM over n_active x max-frames implicit frames with the
 * same cached matrices and kernel choices as for one stream's rows (gemm16: a frame's bits depend on neither neighbours nor packet
 * split, and equal rnnt_fbank's whenever that call has under 1024 frames), wave_carry_roll (new carry read from the staged rows).
 * Frame counts are host arithmetic: no synchronisation.  Every refusal is decided before the first launch and changes nothing:
 * RNNT_ERR_ARG null pointer, duplicated or out-of-range slot, samples_host[i] outside [0, n_samples], (sample_rate, n_fft) differing
 * from the slot's utterance in progress, cap_frames below a row's frame count; RNNT_ERR_SHAPE n_fft or sample_rate outside rnnt_fbank's
 * range; RNNT_ERR_STATE a push to a slot already final and not reset. */
int rnnt_pool_wave(rnnt_ctx* ctx, int32_t n_active, const int32_t* slots_host, const float* wave_dev, int32_t n_samples,
                   const int32_t* samples_host, const int32_t* final_host, int32_t sample_rate, int32_t n_fft, float* out_dev,
                   int32_t cap_frames, int32_t* frames_host, void* stream);
/* a fresh utterance (no samples, no frames, no fixed sample_rate / n_fft) for one slot, or all with slot = -1.  Host only. */
int rnnt_stream_wave_reset(rnnt_ctx* ctx, int32_t slot, void* stream);
/* one slot's front-end state; every output is optional.  carry_host == NULL: host only.  Otherwise the *n_carry_out carried samples
 * are copied into carry_host [cap_carry] and the stream is synchronised.  A fresh or finished slot carries nothing. */
int rnnt_stream_get_wave_state(rnnt_ctx* ctx, int32_t slot, int32_t* samples_out, int32_t* frames_out, int32_t* sample_rate_out,
                               int32_t* n_fft_out, int32_t* finished_out, int32_t* n_carry_out, float* carry_host, int32_t cap_carry,
                               void* stream);
/* One slot's push as a pure C++ function (no context, no GPU) through the index helper the two kernels use: carry_in [n_carry_in] and
 * samples_so_far before, new_samples [n_new], final -> staged_out: the staged row from the push's first new frame on (frame r of the
 * push starts at r * 512; *staged_len_out samples), *first_frame_out, *n_frames_out, and the carry after it.  n_carry_in must be the
 * carry length the arithmetic gives for samples_so_far (RNNT_ERR_ARG). */
int rnnt_wave_stage_host(const float* carry_in, int32_t n_carry_in, int32_t samples_so_far, const float* new_samples, int32_t n_new,
                         int32_t final, int32_t n_fft, float* staged_out, int32_t cap_staged, int32_t* staged_len_out,
                         int32_t* first_frame_out, int32_t* n_frames_out, float* carry_out, int32_t cap_carry, int32_t* n_carry_out);

/* -- state read-back in the reference's layouts (parity tests, facade attributes) -------------- */
/* streaming_att_cache of one stream: [12, 4, len, 128] (K = [...,:64], V = [...,64:],
 * wenet/transformer/encoder.py:284); *len_out = cached frames.  dst_host may be NULL to query len. */
int rnnt_get_att_cache(rnnt_ctx* ctx, int32_t stream_idx, float* dst_host, int32_t* len_out, void* stream);
/* streaming_cnn_cache of one stream: [12, 1, 256, 30] (wenet/transformer/convolution.py:130). */
int rnnt_get_cnn_cache(rnnt_ctx* ctx, int32_t stream_idx, float* dst_host, void* stream);
/* predictor state [h,c] each [256] and last token of one stream. */
int rnnt_get_predictor_state(rnnt_ctx* ctx, int32_t stream_idx, float* h_host, float* c_host,
                             int32_t* last_token, void* stream);
/* buffered encoder frames [n_streams, frames, 256] starting at the oldest buffered frame. */
int rnnt_get_enc_frames(rnnt_ctx* ctx, float* dst_host, int32_t* frames_out, void* stream);
/* device pointer of the encoder-frame buffer [n_streams, max_enc_frames, 256] (borrowed). */
const float* rnnt_enc_frames_dev(rnnt_ctx* ctx, int32_t* frames_out, int32_t* stride_frames);

/* per-launch-site timing with HIP events recorded on the launch stream (bench.py roofline leg).
 * tag selects ONE launch site: 1 conv1, 2 conv2 (implicit GEMM), 3 embed linear, 4 FFN w_1, 5 FFN w_2, 6 QKV,
 * 7 attention, 8 attention out-proj, 9 pointwise_conv1+GLU, 10 depthwise conv, 11 pointwise_conv2, 13 joint enc
 * projection, 20 LSTM cell, 21 predictor projection, 22 joint pred_ffn+tanh, 23 joint ffn_out (13 and 20 - 22 also tag the
 * teacher-forced predictor steps and the two projections of the scoring and alignment calls), 40 the picked lattice of
 * rnnt_transducer_nll, 41 its alpha recursion (and rnnt_ctc_nll's), 42 the Viterbi launch of the rnnt_*_align calls, 43 prefix_step
 * and 44 prefix_merge of rnnt_prefix_beam_decode (one launch each per frame), 45 ctc_prefix_search of the rnnt_ctc_prefix_beam_*
 * calls (one launch per call), 46 ctc_prefix_search_pool of rnnt_pool_ctc_prefix_logprobs / rnnt_pool_chunk_ctc_prefix (the resumable
 * search launch), 47 ctc_prefix_pack of rnnt_stream_get_ctc_prefix (the pack launch), 48 wave_stage of rnnt_pool_wave (the staging launch),
 * 49 prefix_step_pool and 50 prefix_merge_pool of rnnt_pool_prefix_frames / rnnt_pool_chunk_prefix (one launch each per frame).
 * (51 ctc_loss_pick, 52 ctc_alpha_beta, 53 ctc_loss_occ and 54 ctc_loss_grad name the launches of the context-free rnnt_ctc_loss;
 * a context cannot select them.)
 * rnnt_profile_end synchronises the recorded events and returns the summed kernel time and launch count. */
int rnnt_profile_begin(rnnt_ctx* ctx, int32_t tag);
int rnnt_profile_end(rnnt_ctx* ctx, double* total_ms, int64_t* n_launches);

/* launch-form log (tests): between begin and end every kernel launch of the context is counted on the host under the form name
 * of its launch site -- the kernel with every choice the host made for it, e.g. "gemm_bf<2,2>", "gemm16<8,1>", "ffn_as<8>",
 * "conv1_relu_rows", "rel_attention<4>".  Off (the default) it costs one branch per launch; on or off there is no device work and
 * no synchronisation.  Launches replayed from a captured graph are not seen (the encoder calls launch eagerly).  end stops the log
 * and writes "name\tcount\n" per distinct name, sorted by name and NUL-terminated, into buf[cap] (cut at cap - 1 characters);
 * *needed is the size of the whole text with its NUL, and the counts are kept until the next begin, so a short buffer can be
 * followed by a second end. */
int rnnt_form_log_begin(rnnt_ctx* ctx);
int rnnt_form_log_end(rnnt_ctx* ctx, char* buf, int64_t cap, int64_t* needed);

/* counters for bench/roofline: number of kernel launches and greedy steps since the last reset. */
int rnnt_get_counters(rnnt_ctx* ctx, int64_t* launches, int64_t* greedy_steps);

#ifdef __cplusplus
}
#endif
#endif /* RNNT_HIP_H */
