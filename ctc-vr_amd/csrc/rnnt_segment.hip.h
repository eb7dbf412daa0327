// Segments of the stream pool (rnnt_pool_segment; api_pool_segment.hip.inc): a new utterance in the listed slots without closing them.
// ONE launch whatever the number of slots and of state kinds: blockIdx.y is the listed row, and workgroup x = 0 of a row writes the
// start state of every decoder the context holds -- by the device functions the range-form resets are made of (greedy_slot_start,
// beam_slot_start, prefix_slot_start, ctc_prefix_slot_start), so a segment's start and an opened slot's are the same stores.  The encoder is touched
// only when p.fresh: then all workgroups of the row share stream_slot_reset's ring fill (ring_slot_fill) for that slot.
#pragma once
#include "rnnt_common.hip.h"
#include "rnnt_encoder.hip.h"
#include "rnnt_endpoint.hip.h"
#include "rnnt_beam.hip.h"
#include "rnnt_prefix.hip.h"
#include "rnnt_ctc_prefix.hip.h"

struct SegmentP {
    const int* slots;            // [gridDim.y] the listed slots, distinct
    // greedy decoder: both LSTM buffers [2][B][256], committed buffer, argmax key, frame index, symbol count, token count, last token
    float *h, *c;
    int* sel; unsigned long long* key; int *fidx, *nsym, *count, *tok;
    int B, blank;
    // the searches; a kind the context never allocated has a null nh / ctc and costs nothing
    BeamPoolP beam; int beam_state_slots;
    PrefixPoolP prefix; int prefix_lcap;
    CpSlotState* ctc;
    int* ep_state;               // [B][EP_STATE_INTS] or null: the counters only, the config stays
    int* hs_len;                 // [B] or null: the length only, the pointer (the keep flag) stays
    // fresh != 0: the conv rings [L][B][cap][256] of the slot as rnnt_stream_open leaves them
    float *gring, *xring; const float* glu0;
    int cap, fresh;
};

__global__ __launch_bounds__(256) void pool_segment_reset(SegmentP p) {
    __shared__ CpSlotState z;
    const int slot = ldgi(p.slots + blockIdx.y), tid = threadIdx.x;
    if (p.fresh) ring_slot_fill(p.gring, p.xring, p.glu0, p.B, p.cap, slot, (long long)blockIdx.x * 256 + tid, (long long)gridDim.x * 256);
    if (blockIdx.x != 0) return;                                   // uniform over the workgroup, before any barrier
    greedy_slot_start(p.h, p.c, p.sel, p.key, p.fidx, p.nsym, p.count, p.tok, p.B, slot, p.blank, tid, 256);
    if (p.beam.nh) beam_slot_start(p.beam, slot, p.beam_state_slots);
    if (p.prefix.nh) prefix_slot_start(p.prefix, slot, p.prefix_lcap, p.blank);
    if (p.ep_state && tid < EP_STATE_INTS) p.ep_state[slot * EP_STATE_INTS + tid] = 0;
    if (p.hs_len && tid == 0) p.hs_len[slot] = 0;
    if (p.ctc) ctc_prefix_slot_start(p.ctc + slot, z);             // last: it holds the barriers
}
