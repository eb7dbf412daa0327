"""Shapes, float64 references and the coverage table shared by test_kernel_forms_cpu.py and test_kernel_forms.py: the encoder's host
code chooses a kernel form by shape (host_launch.hip.inc: launch_gemm, run_subsample, launch_gemm_tab; host_lm.hip.inc: the
layer-major schedule), and every shape here sits just above or just below one of its thresholds.  rnnt_encoder_full is the call that
reaches them with a float64 oracle (oracle.rnnt_oracle.encoder_full).  No GPU is touched here."""
import os
import re

import numpy as np

import ctc_vr_amd.testing as T
import window_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_FILES = [os.path.join(ROOT, "ctc-vr_amd", "csrc", f) for f in ("host_launch.hip.inc", "host_lm.hip.inc")]

FSUB = 19                                               # frequency bins after the two stride-2 convolutions (RNNT_FSUB)
MODES = ["fp32", "bf16x3", "f16x3"]
SPLIT = ["bf16x3", "f16x3"]

# pair -> streams, frames above / below the threshold, ragged lengths (of T): stream 0 and the last stream are full length and
# carry the same audio, one stream is T - 1 (the other side of the subsampled mask's rounding), at least one is much shorter
PAIRS = {
    "layer-1024": {"B": 4, "above": 1031, "below": 1023, "lens": lambda t: [t, t - 1, 519, t], "seed": 8101},
    "conv2-32768": {"B": 7, "above": 991, "below": 987, "lens": lambda t: [t, t - 1, 700, 519, 300, t - 2, t], "seed": 8102},
    "conv2-2048": {"B": 4, "above": 111, "below": 107, "lens": lambda t: [t, t - 1, 60, t], "seed": 8103},
}
SIDES = ("above", "below")
# per-context knobs of a variant, set as test_encoder_window._env sets its own (a context reads them at rnnt_create)
VARIANTS = {
    "default": {},
    "noas": {"RNNT_AS": "0"},                           # LDS-tiled gemm_bf for every layer contraction
    "nolm": {"RNNT_LM": "0"},                           # eager run_subsample + run_layer, tiled rel_attention<4> under klen
    "nofuse": {"RNNT_CONV1_FUSE": "0"},                 # conv2-32768 only: conv1_relu_rows + gemm_bw instead of gemm_bw_c1
    "unchained": {"RNNT_LM_QKV_TAIL": "0", "RNNT_LM_OUT_CHAIN": "0", "RNNT_LM_PW2_HEAD": "0"},   # layer-1024, split modes: gemm_as, dwconv_lm
}
KNOBS = sorted({k for v in VARIANTS.values() for k in v})


def variants_of(pair, mode):
    v = ["default", "noas", "nolm"]
    if pair == "conv2-32768":
        v.append("nofuse")
    if pair == "layer-1024" and mode != "fp32":
        v.append("unchained")
    return v


def case_id(pair, side, mode, variant):
    return f"{pair}-{side}-{mode}-{variant}"


CASES = [(p, s, m, v) for p in PAIRS for s in SIDES for m in MODES for v in variants_of(p, m)]

# the wavefront case (fp32, RNNT_LM=0, rnnt_encoder_chunks): 64 streams, two chunks of 67 frames (t' 16, M = 1024 per descriptor).
# required_cache_size = 0 restarts the K/V cache after every chunk, so the two chunks cannot share a stage (wf_build_tables:
# `behind`) and the first and the last stage hold ONE descriptor per GEMM class -- the stages launch_gemm_tab gives gemm16_tab.
WF = {"B": 64, "len": 67, "chunks": 2, "policy": "zero", "seed": 8104, "streams": (0, 63)}
WF_ID = "wavefront-fp32-nolm"


def sub_len(t):
    return W.sub_len(t)


def klen(n):
    """valid encoder frames of an utterance of n fbank frames: the library's formula (rnnt_encoder_full)"""
    n1 = (n - 1) // 2 if n > 2 else 0
    return (n1 - 1) // 2 if n1 > 2 else 0


def shape(pair, side):
    """-> B, T, t', lens, layer rows M, conv2 rows M2"""
    p = PAIRS[pair]
    t = p[side]
    tq = sub_len(t)
    return p["B"], t, tq, p["lens"](t), p["B"] * tq, p["B"] * tq * FSUB


def tail_frames(pair, side):
    """frames of the LAST stream that lie in the last partial tile of a large form: the 64-row tiles of gemm_bf<2,*> / gemm_ns<2,*>
    over the B * t' layer rows, and the 128-row tiles of gemm_bw / gemm_bw_c1 over the B * t' * 19 conv2 rows"""
    _, _, tq, _, m, m2 = shape(pair, side)
    rows = m % 64 or 64
    rows2 = -(-(m2 % 128 or 128) // FSUB)
    return min(tq, max(rows, rows2))


_CACHE = {}


def state_dict():
    return W.state_dict()


def case_input(pair, side):
    """[B, T, 80] float32, zero beyond each stream's length; stream B - 1 is stream 0 again"""
    key = ("x", pair, side)
    if key not in _CACHE:
        b, t, _, lens, _, _ = shape(pair, side)
        x = T.synth_fbank(b, t, seed=PAIRS[pair]["seed"])
        x[b - 1] = x[0]
        for i in range(b):
            x[i, lens[i]:] = 0
        x.setflags(write=False)
        _CACHE[key] = x
    return _CACHE[key]


def full_ref(x, lens, dtype=None):
    """oracle.rnnt_oracle.encoder_full on the state dict cast to dtype (default float64) -> frames [B, t', 256] (numpy), valid [B]"""
    import torch
    from oracle import rnnt_oracle as O
    dtype = dtype or torch.float64
    with torch.no_grad():
        y, mask = O.encoder_full(T.ref_state_dict(state_dict(), dtype), torch.tensor(np.asarray(x), dtype=dtype), torch.tensor(lens))
    return y.numpy(), mask[:, 0].sum(1).tolist()


def case_ref(pair, side, dtype=None):
    """the reference of one shape, computed once per session and read-only"""
    key = ("ref", pair, side, dtype)
    if key not in _CACHE:
        y, valid = full_ref(case_input(pair, side), shape(pair, side)[3], dtype)
        y.setflags(write=False)
        _CACHE[key] = (y, valid)
    return _CACHE[key]


def valid_diff(got, want, valid, lo=0, hi=None):
    """max |difference| over the valid frames [lo, hi) of every stream (frames counted per stream)"""
    d = 0.0
    for b, n in enumerate(valid):
        a, e = min(lo, n), n if hi is None else min(hi, n)
        if e > a:
            d = max(d, W.maxdiff(got[b, a:e], want[b, a:e]))
    return d


def wf_plan():
    return W.make_plan(WF["len"], WF["policy"], WF["chunks"])


def wf_input():
    if "wfx" not in _CACHE:
        x = T.synth_fbank(WF["B"], WF["len"] * WF["chunks"], seed=WF["seed"])
        x[WF["B"] - 1] = x[0]
        x.setflags(write=False)
        _CACHE["wfx"] = x
    return _CACHE["wfx"]


def wf_ref(stream):
    key = ("wfref", stream)
    if key not in _CACHE:
        _CACHE[key] = np.concatenate([r["frames"] for r in T.encoder_stream_ref(state_dict(), wf_input()[stream].copy(), wf_plan())], 0)
    return _CACHE[key]


# ---- form names of the two host files ------------------------------------------------------------------------------------------------
def source_forms():
    """Every form name a launch site of the two host files can log: the literals given to LAUNCHCHK, and the names the tiled
    attention's launch macro builds from its kernel argument (LAUNCH_ATTN_TILED: KERNEL<NQ>, NQ = 1, 2, 4)."""
    out = set()
    for path in HOST_FILES:
        src = open(path, encoding="utf-8").read()
        out |= set(re.findall(r'LAUNCHCHK\("([^"]+)"\)', src))
        for k in re.findall(r"^\s*LAUNCH_ATTN_TILED\((\w+),", src, flags=re.M):
            out |= {f"{k}<{nq}>" for nq in (1, 2, 4)}
    return out


def _ids(pairs=None, sides=SIDES, modes=MODES, variants=None):
    return [case_id(p, s, m, v) for p in (pairs or PAIRS) for s in sides for m in modes for v in variants_of(p, m) if variants is None or v in variants]


# three small cases beside the pairs, for forms that no other float64 test dispatches
RAGGED = {"lens": [96, 71, 52], "chunk": 16, "seed": 8105}      # rnnt_encode_ragged: tail chunks of 16, 23 and 20 frames, one class each
TILED = (19, "one")                                      # window_cases plan of t' = 4 chunks through rnnt_encoder_chunk under RNNT_ATTN_STREAM=0
FUSED_WF = {"B": 3, "len": 67, "chunks": 2, "policy": "all", "seed": 8106}   # three streams of 16 frames fill a 48-row fused half-block tile
RAGGED_IDS = [f"ragged-{m}" for m in MODES]
TILED_IDS = [f"attn-tiled-{m}" for m in MODES]
FUSED_WF_IDS = [f"wavefront-fused-{m}" for m in SPLIT]
EXTRA_IDS = [WF_ID] + RAGGED_IDS + TILED_IDS + FUSED_WF_IDS


def ragged_plan(n, chunk):
    """one stream's chunks in a ragged call (ragged_encode: the decode script's slicing rule, offset = required = c * (chunk / 4))
    -> [(start, length, offset, required)]"""
    minc, plan, off = max(chunk, 16), [], 0
    while off < n:
        end = min(off + chunk, n)
        if n - end < minc and end < n:
            end = n
        plan.append((off, end - off, len(plan) * (chunk // 4), len(plan) * (chunk // 4)))
        off = end
    return plan


def ragged_input():
    if "rgx" not in _CACHE:
        lens = RAGGED["lens"]
        x = T.synth_fbank(len(lens), max(lens), seed=RAGGED["seed"])
        for b, n in enumerate(lens):
            x[b, n:] = 0
        x.setflags(write=False)
        _CACHE["rgx"] = x
    return _CACHE["rgx"]


def ragged_ref(b):
    key = ("rgref", b)
    if key not in _CACHE:
        n = RAGGED["lens"][b]
        _CACHE[key] = np.concatenate([r["frames"] for r in T.encoder_stream_ref(state_dict(), ragged_input()[b, :n].copy(), ragged_plan(n, RAGGED["chunk"]))], 0)
    return _CACHE[key]


def fused_wf_plan():
    return W.make_plan(FUSED_WF["len"], FUSED_WF["policy"], FUSED_WF["chunks"])


def fused_wf_input():
    if "fwx" not in _CACHE:
        x = T.synth_fbank(FUSED_WF["B"], FUSED_WF["len"] * FUSED_WF["chunks"], seed=FUSED_WF["seed"])
        x.setflags(write=False)
        _CACHE["fwx"] = x
    return _CACHE["fwx"]


def fused_wf_ref(b):
    key = ("fwref", b)
    if key not in _CACHE:
        _CACHE[key] = np.concatenate([r["frames"] for r in T.encoder_stream_ref(state_dict(), fused_wf_input()[b].copy(), fused_wf_plan())], 0)
    return _CACHE[key]


KNOB = "needs a process-static knob"
SHAPE = "needs a shape beyond a few-second test"
POOL = "stream-pool only"
NONE = "no encoder call reaches it"
WINDOW = "test_encoder_window.py::test_per_chunk_api_vs_float64"
WHOLE = "test_encoder_window.py::test_whole_utterance_call_vs_float64"
EXISTING = (WINDOW, WHOLE)
BIG2 = ("layer-1024", "conv2-32768")
LM = ("default", "noas", "nofuse", "unchained")          # the variants that keep the layer-major schedule

# form name -> the ids of the tests that must log it (case ids of test_kernel_forms.py, or an existing float64 test whose driver
# was run under the log), or the one-line reason it is not reached.  Every row was read off the form logs of an MI355X run; where
# the dispatch code reads differently from the issue's expectation the log decided (DESIGN §3 carries the table).
COVERAGE = {
    # subsampling
    "conv1_relu": _ids(["conv2-2048"]) + [WINDOW, WHOLE],
    "conv1_relu_rows": (_ids(["layer-1024"]) + _ids(["conv2-32768"], modes=["fp32"]) + _ids(["conv2-32768"], ["below"], SPLIT)
                        + _ids(["conv2-32768"], ["above"], SPLIT, ["nolm", "nofuse"]) + [WF_ID]),
    "gemm_bw_c1<8>": _ids(["conv2-32768"], ["above"], SPLIT, ["default", "noas"]),
    "gemm_bw<8>": _ids(["conv2-32768"], ["above"], SPLIT, ["nolm", "nofuse"]),
    "gemm_bw_c1<4>": KNOB + " (RNNT_BW_NW=4)",
    "gemm_bw<4>": KNOB + " (RNNT_BW_NW=4)",
    # launch_gemm, split-operand modes: conv2 below 32768 rows and the embed GEMM everywhere; every layer contraction under
    # RNNT_AS=0, RNNT_LM=0 and (attention out-projection, pointwise_conv2) unchained
    "gemm_bf<2,2>": _ids(modes=SPLIT),
    "gemm_bf<1,2>": _ids(["layer-1024"], ["below"], SPLIT, ["noas", "nolm"]) + _ids(["conv2-2048"], modes=SPLIT, variants=["noas", "nolm"]) + [WINDOW],
    "gemm_bf<1,1>": _ids(["layer-1024"], ["below"], SPLIT) + _ids(["conv2-2048"], modes=SPLIT) + [WINDOW, WHOLE],
    "gemm_bf<2,2,tanh>": NONE + ": the joint's tanh operand (rnnt_joint and the scoring calls; the decoder side is held by its own tests)",
    # launch_gemm, exact f32
    "gemm_ns<2,2>": _ids(BIG2, modes=["fp32"]) + _ids(["conv2-2048"], ["above"], ["fp32"]) + [WF_ID],
    "gemm_ns<1,2>": _ids(["layer-1024"], ["above"], ["fp32"]) + _ids(["conv2-32768"], modes=["fp32"]) + _ids(["conv2-2048"], ["below"], ["fp32"]) + [WF_ID],
    "gemm_ns<2,2,tanh>": NONE + ": the joint's tanh operand (rnnt_joint and the scoring calls; the decoder side is held by its own tests)",
    "gemm_ns<2,2,nt>": KNOB + " (RNNT_CONV2_LDS=2)",
    "gemm16<4,1>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<4,2>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<8,1>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<8,2>": NONE + ": no encoder contraction has K >= 1024 with N >= 512 (front-end and decoder shapes)",
    # layer-major schedule
    "lm_ctx_in": _ids(variants=LM),
    "ffn_as<8>": _ids(modes=SPLIT, variants=["default", "nofuse", "unchained"]) + [WHOLE],
    "ffn_as<4>": KNOB + " (RNNT_FFN_NW=4)",
    "ffn_as<16>": KNOB + " (RNNT_FFN_NW=16)",
    "gemm_as": _ids(modes=SPLIT, variants=["unchained"]),
    "rel_attention_lm_res": _ids(["conv2-2048"], modes=SPLIT, variants=LM) + [WHOLE],
    "rel_attention_lm_bf": _ids(BIG2, modes=SPLIT, variants=LM) + [WHOLE],          # t' >= 246 keys do not fit the resident plan
    "rel_attention_lm_mfma": _ids(modes=["fp32"], variants=LM) + [WHOLE],
    "dwconv_lm": _ids(modes=["fp32"], variants=LM) + _ids(modes=SPLIT, variants=["noas", "unchained"]) + [WHOLE],
    "lm_gather_tails": RAGGED_IDS,
    "lm_scatter_rows": RAGGED_IDS,
    # eager path (rnnt_encoder_chunk; rnnt_encoder_full under RNNT_LM=0)
    "rel_attention_stream": [WINDOW],
    "rel_attention<1>": TILED_IDS,
    "rel_attention<2>": [WINDOW],
    "rel_attention<4>": _ids(variants=["nolm"]) + [WINDOW],
    "dwconv_bn_silu": _ids(variants=["nolm"]) + [WINDOW],
    "layer_norm": _ids() + [WF_ID, WINDOW, WHOLE],
    # wavefront schedule
    "block_front<1>": [WHOLE], "block_front<2>": [WHOLE], "block_front<3>": FUSED_WF_IDS,
    "block_back<1>": [WHOLE], "block_back<2>": [WHOLE], "block_back<3>": FUSED_WF_IDS,
    "gemm_bf_tab<1,1>": [WHOLE], "gemm_bf_tab<1,2>": [WHOLE],
    "gemm_ns_tab<1,1,32>": [WF_ID, WHOLE], "gemm_ns_tab<1,1,64>": [WF_ID, WHOLE], "gemm_ns_tab<1,2,32>": [WF_ID, WHOLE],
    "gemm16_tab<4,1,1>": [WF_ID, WHOLE], "gemm16_tab<8,1,1>": [WF_ID, WHOLE], "gemm16_tab<4,1,2>": [WHOLE],
    "gemm16_tab<4,2,4>": [WF_ID],                        # ffn w_1 and pointwise_conv1 of the single-descriptor stages: 1024 rows x N >= 512
    # the two larger tiles need one descriptor of >= 2048 rows (two or more descriptors go to gemm_ns_tab): the log of the 64 x 16
    # row case shows <4,2,4> and the 16-row tiles only, and the shape is not grown
    "gemm16_tab<4,4,4>": SHAPE + ": a single descriptor of >= 2048 rows x 1024 columns (128 streams x 16 frames), or RNNT_GEMM_NS=0",
    "gemm16_tab<8,2,4>": SHAPE + ": a single K = 1024 descriptor of >= 2048 rows (128 streams x 16 frames), or RNNT_GEMM_NS=0",
    "gemm16_tab<8,1,2>": NONE + ": no stage GEMM class has K = 1024 with N >= 512",
    # helpers of the stream pool that live in host_launch.hip.inc
    "beam_slot_reset": POOL, "ctc_prefix_slot_reset": POOL, "prefix_init_pool": POOL, "pool_hist_set": POOL, "pool_hist_append": POOL,
    "pool_endpoint_set": POOL, "pool_endpoint": POOL,
}


def expected_forms(cid):
    return {f for f, v in COVERAGE.items() if not isinstance(v, str) and cid in v}


def design_rows():
    """the rows of DESIGN §3's "Launch forms and where each is held to float64" table, one per form, from COVERAGE"""
    known = {case_id(*c): c for c in CASES}
    rows = []
    for form in sorted(COVERAGE):
        v = COVERAGE[form]
        if isinstance(v, str):
            rows.append(f"| `{form}` | not reached: {v} |")
            continue
        count, parts = {}, []
        for i in v:
            if i in known:
                pair, side = known[i][:2]
                count.setdefault(pair, {}).setdefault(side, 0)
                count[pair][side] += 1
        for pair, c in count.items():
            parts.append(f"{pair} ×{sum(c.values())}" if len(c) == 2 else f"{pair} {next(iter(c))} ×{sum(c.values())}")
        parts += [i.replace("test_encoder_window.py::", "") if i in EXISTING else i for i in v if i not in known]
        rows.append(f"| `{form}` | {', '.join(parts)} |")
    return rows
