"""Shapes, float64 references and the coverage table shared by test_kernel_forms_cpu.py and test_kernel_forms.py: the encoder's host
code chooses a kernel form by shape (host_launch.hip.inc: launch_gemm, run_subsample, launch_gemm_tab; host_lm.hip.inc: the
layer-major schedule), and every shape here sits just above or just below one of its thresholds.  rnnt_encoder_full is the call that
reaches them with a float64 oracle (oracle.rnnt_oracle.encoder_full).  The forms, tile maps and stage plans that a knob selects
(read per context at rnnt_create) have cases of their own on the same shapes: KNOB_FULL, KNOB_WF, KNOB_CASES.  No GPU is touched here."""
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
    # ---- the launch-form knobs of KNOB_FULL / KNOB_WF below (per context like the ones above; no case of CASES sets them) ----
    "bw4": {"RNNT_BW_NW": "4"},                         # gemm_bw_c1<4>
    "bw4-nofuse": {"RNNT_BW_NW": "4", "RNNT_CONV1_FUSE": "0"},   # gemm_bw<4>
    "ffn4": {"RNNT_FFN_NW": "4"}, "ffn16": {"RNNT_FFN_NW": "16"},
    "nobw": {"RNNT_CONV2_BW": "0"},                     # conv2 of 32851 rows on gemm_bf<2,2>
    "norows": {"RNNT_CONV1_ROWS": "0"},                 # conv1_relu where conv1_relu_rows would run
    "pd1": {"RNNT_GEMM_PD": "1"},                       # gemm_ns with one K block in flight
    "attnf32": {"RNNT_ATTN_BF": "0"},                   # exact-f32 attention in a split mode
    # wavefront contexts (RNNT_LM=0)
    "nolm-lds2": {"RNNT_LM": "0", "RNNT_CONV2_LDS": "2"}, "nolm-lds0": {"RNNT_LM": "0", "RNNT_CONV2_LDS": "0"},
    "nolm-lds2-pd1": {"RNNT_LM": "0", "RNNT_CONV2_LDS": "2", "RNNT_GEMM_PD": "1"},
    "nolm-ns0": {"RNNT_LM": "0", "RNNT_GEMM_NS": "0"}, "nolm-nsmin1": {"RNNT_LM": "0", "RNNT_NS_MIN_GROUPS": "1"},
    "nolm-pd1": {"RNNT_LM": "0", "RNNT_GEMM_PD": "1"},
    **{f"nolm-x{x}": {"RNNT_LM": "0", "RNNT_XCD_X": str(x)} for x in (1, 2, 4, 8)},
    "nolm-apm0": {"RNNT_LM": "0", "RNNT_ATTN_PAIR_MAJOR": "0"},
    "nolm-subsync": {"RNNT_LM": "0", "RNNT_WF_SUB_ASYNC": "0"},   # the wavefront's subsampling on the caller's stream
    "nolm-unfused": {"RNNT_LM": "0", "RNNT_FUSED": "0"},
    **{f"nolm-unfused-x{x}": {"RNNT_LM": "0", "RNNT_FUSED": "0", "RNNT_XCD_X": str(x)} for x in (1, 2, 4, 8)},
    "nolm-unfused-merge1": {"RNNT_LM": "0", "RNNT_FUSED": "0", "RNNT_WF_MERGE": "1"},
    "nolm-fmerge1": {"RNNT_LM": "0", "RNNT_FUSE_MERGE": "1"}, "nolm-fmerge2": {"RNNT_LM": "0", "RNNT_FUSE_MERGE": "2"},
    "nolm-fframes8": {"RNNT_LM": "0", "RNNT_FUSE_FRAMES": "8"}, "nolm-fframes16": {"RNNT_LM": "0", "RNNT_FUSE_FRAMES": "16"},
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


def wf_cfg(kind):
    return {"wf": WF, "fwf": FUSED_WF, "fknob": FUSE_KNOB}[kind]


def wf_kind_plan(kind):
    c = wf_cfg(kind)
    return W.make_plan(c["len"], c["policy"], c["chunks"])


def wf_kind_input(kind):
    """[B, chunks * len, 80] float32 of a wavefront shape (read-only; "wf": stream B - 1 is stream 0 again)"""
    if kind == "wf":
        return wf_input()
    if kind == "fwf":
        return fused_wf_input()
    if "fkx" not in _CACHE:
        c = FUSE_KNOB
        x = T.synth_fbank(c["B"], c["len"] * c["chunks"], seed=c["seed"])
        x.setflags(write=False)
        _CACHE["fkx"] = x
    return _CACHE["fkx"]


def wf_kind_ref(kind, stream):
    """float64 frames of one stream of a wavefront shape (encoder_stream_ref over its chunk plan), computed once per session"""
    if kind == "wf":
        return wf_ref(stream)
    if kind == "fwf":
        return fused_wf_ref(stream)
    key = ("fkref", stream)
    if key not in _CACHE:
        _CACHE[key] = np.concatenate([r["frames"] for r in T.encoder_stream_ref(state_dict(), wf_kind_input(kind)[stream].copy(), wf_kind_plan(kind))], 0)
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


# ---- the knobs that were process-static: one context per value, in the same process ------------------------------------------------
# rnnt_encoder_full cases beside CASES: (pair, side, mode, variant) -> the default-knob case of the same shape and mode whose frames
# the code claims (or this table records) to be bit-identical, or None where only the float64 bar is asserted
KNOB_FULL = {}
for _m in SPLIT:
    KNOB_FULL[("conv2-32768", "above", _m, "bw4")] = "default"             # "RNNT_BW_NW=4, same results" (host_launch.hip.inc)
    KNOB_FULL[("conv2-32768", "above", _m, "bw4-nofuse")] = "nofuse"
    KNOB_FULL[("conv2-32768", "above", _m, "nobw")] = None                 # other tiles (64 rows, k order of gemm_bf): float64 bar only
    for _p in ("layer-1024", "conv2-2048"):
        KNOB_FULL[(_p, "above", _m, "ffn4")] = "default"                   # "bitwise the same results as 4" (host_lm.hip.inc)
        KNOB_FULL[(_p, "above", _m, "ffn16")] = "default"                  # "the same bits too" (host_lm.hip.inc): a column's sums do not depend on its wave
    KNOB_FULL[("conv2-2048", "above", _m, "attnf32")] = None
KNOB_FULL[("layer-1024", "above", "fp32", "norows")] = "default"           # conv1_relu and conv1_relu_rows: the same nine fmaf per output
KNOB_FULL[("layer-1024", "above", "bf16x3", "norows")] = "default"
KNOB_FULL[("layer-1024", "above", "fp32", "pd1")] = None                   # the prefetch depth reorders loads, not sums: recorded
KNOB_FULL_IDS = {c: case_id(*c) for c in KNOB_FULL}

# wavefront cases: id -> (shape kind, mode, variant, the variant it is compared with bit by bit or None, whether equality is asserted)
# "wf": 64 streams x 2 chunks (fp32; conv2 M = 19456 >= 2048 with nc = 2); "fwf": FUSED_WF's three streams, fused or (RNNT_FUSED=0)
# on gemm_bf_tab; "fknob": three streams x 8 chunks of 19 frames (t' = 4), the shape on which the fuse knobs move the stage plan
FUSE_KNOB = {"B": 3, "len": 19, "chunks": 8, "policy": "all", "seed": 8107}
KNOB_WF = {
    "wavefront-fp32-nolm-lds2": ("wf", "fp32", "nolm-lds2", "nolm", True),          # a non-temporal load changes no arithmetic
    "wavefront-fp32-nolm-lds0": ("wf", "fp32", "nolm-lds0", "nolm", False),
    "wavefront-fp32-nolm-lds2-pd1": ("wf", "fp32", "nolm-lds2-pd1", "nolm", False),
    "wavefront-fp32-nolm-ns0": ("wf", "fp32", "nolm-ns0", "nolm", False),
    "wavefront-fp32-nolm-nsmin1": ("wf", "fp32", "nolm-nsmin1", "nolm", False),
    "wavefront-fp32-nolm-pd1": ("wf", "fp32", "nolm-pd1", "nolm", False),
    **{f"wavefront-fp32-nolm-x{x}": ("wf", "fp32", f"nolm-x{x}", "nolm", True) for x in (1, 2, 4, 8)},   # X only deals tiles to workgroups
    "wavefront-fp32-nolm-apm0": ("wf", "fp32", "nolm-apm0", "nolm", True),             # t' = 16: no direct-stream attention, the knob is not read
    "wavefront-fp32-nolm-subsync": ("wf", "fp32", "nolm-subsync", "nolm", True),       # the same launches on the same arguments, on one stream
    "wavefront-t4-fp32-nolm": ("fknob", "fp32", "nolm", None, False),
    "wavefront-t4-fp32-nolm-apm0": ("fknob", "fp32", "nolm-apm0", "nolm", False),
    **{f"wavefront-unfused-{m}": ("fwf", m, "nolm-unfused", None, False) for m in SPLIT},
    **{f"wavefront-unfused-{m}-x{x}": ("fwf", m, f"nolm-unfused-x{x}", "nolm-unfused", True) for m in SPLIT for x in (1, 2, 4, 8)},
    **{f"wavefront-unfused-{m}-merge1": ("fwf", m, "nolm-unfused-merge1", "nolm-unfused", False) for m in SPLIT},
    **{f"fuse-knobs-{m}": ("fknob", m, "nolm", None, False) for m in SPLIT},
    **{f"fuse-knobs-{m}-{k}": ("fknob", m, f"nolm-{k}", "nolm", False) for m in SPLIT for k in ("fmerge1", "fmerge2", "fframes8", "fframes16")},
}
KNOB_IDS = list(KNOB_FULL_IDS.values()) + list(KNOB_WF)
# streams of the 64-stream shape that a knob case holds to float64.  Rows are stream-major, 16 per stream, so a 64-row tile
# (gemm16_tab<4,4,4>) holds streams 4k .. 4k + 3 in its four 16-row subtiles and a 32-row tile two: streams 0, 1, 2 and 63 sit in
# subtiles 0, 1, 2 and 3.  (Every stream is also held to the default context's frames, which WF["streams"] hold to float64.)
WF_KNOB_STREAMS = (0, 1, 2, 63)

# stage plans of the fused wavefront on FUSE_KNOB (8 chunks of t' = 4, R = -1): chunks per super-chunk = min(RNNT_FUSE_MERGE,
# floor(min(RNNT_FUSE_FRAMES, 16) / 4)); stages = super-chunks + 11, one block_front and one block_back launch per stage.  Three streams
# x (chunks x 4) frames per tile -> the half-block's row tiles MT = ceil(3 * frames / 16).
FUSE_PLANS = {"nolm": (3, 3), "nolm-fmerge1": (1, 1), "nolm-fmerge2": (2, 2), "nolm-fframes8": (2, 2), "nolm-fframes16": (4, 3)}   # variant -> (chunks per stage, MT)


def fuse_launches(variant):
    """-> (stages = block_front launches = block_back launches, MT of the full stages) of a FUSE_KNOB case"""
    per, mt = FUSE_PLANS[variant]
    return -(-FUSE_KNOB["chunks"] // per) + 11, mt


DECODE = "test_decode_edges.py::test_graph_decoder_step_budget"
# knob -> the ids of the cases that create a context under it (KNOB_CASES), or, for the knobs other test files hold, file::test
KNOB_CASES = {
    "RNNT_BW_NW": [i for c, i in KNOB_FULL_IDS.items() if c[3] in ("bw4", "bw4-nofuse")],
    "RNNT_FFN_NW": [i for c, i in KNOB_FULL_IDS.items() if c[3].startswith("ffn")],
    "RNNT_CONV2_BW": [i for c, i in KNOB_FULL_IDS.items() if c[3] == "nobw"],
    "RNNT_CONV1_ROWS": [i for c, i in KNOB_FULL_IDS.items() if c[3] == "norows"],
    "RNNT_ATTN_BF": [i for c, i in KNOB_FULL_IDS.items() if c[3] == "attnf32"],
    "RNNT_GEMM_PD": [i for c, i in KNOB_FULL_IDS.items() if c[3] == "pd1"] + ["wavefront-fp32-nolm-pd1", "wavefront-fp32-nolm-lds2-pd1"],
    "RNNT_CONV2_LDS": ["wavefront-fp32-nolm-lds2", "wavefront-fp32-nolm-lds0", "wavefront-fp32-nolm-lds2-pd1"],
    "RNNT_GEMM_NS": ["wavefront-fp32-nolm-ns0"],
    "RNNT_NS_MIN_GROUPS": ["wavefront-fp32-nolm-nsmin1"],
    "RNNT_XCD_X": [i for i in KNOB_WF if i[-3:-1] == "-x"],
    "RNNT_ATTN_PAIR_MAJOR": ["wavefront-fp32-nolm-apm0", "wavefront-t4-fp32-nolm-apm0"],
    "RNNT_FUSE_MERGE": [i for i in KNOB_WF if "-fmerge" in i],
    "RNNT_FUSE_FRAMES": [i for i in KNOB_WF if "-fframes" in i],
    "RNNT_WF_MERGE": [i for i in KNOB_WF if i.endswith("-merge1")],
    "RNNT_FUSED": [i for i in KNOB_WF if i.startswith("wavefront-unfused")],
    "RNNT_DEC_SLACK": [DECODE], "RNNT_DRAIN_STEPS": [DECODE], "RNNT_NO_GRAPH": [DECODE],
    "RNNT_WF_SUB_ASYNC": ["wavefront-fp32-nolm-subsync"],
    "RNNT_LM": _ids(variants=["nolm"]) + [WF_ID], "RNNT_AS": _ids(variants=["noas"]), "RNNT_CONV1_FUSE": _ids(variants=["nofuse"]),
    "RNNT_LM_QKV_TAIL": _ids(variants=["unchained"]), "RNNT_LM_OUT_CHAIN": _ids(variants=["unchained"]), "RNNT_LM_PW2_HEAD": _ids(variants=["unchained"]),
    "RNNT_ATTN_STREAM": TILED_IDS,
    "RNNT_LM_FFN_MERGE": ["test_gpu_parity.py"], "RNNT_LM_SIDE": ["test_gpu_parity.py"],
    "RNNT_ATTN_RESIDENT": ["test_attention_resident.py"], "RNNT_PERSISTENT": ["test_decode_edges.py"], "RNNT_DEC_MULTI": ["test_decode_edges.py"],
    "RNNT_BEAM_CHAIN": ["test_beam_device.py"], "RNNT_PREFIX_GROUP": ["test_stream_pool_prefix.py"],
}
# knobs of DESIGN §10 that change no device work (diagnostics, and names §10 lists as removed), each with its reason
KNOBS_WITHOUT_DEVICE_EFFECT = {
    "RNNT_LM_DEBUG": "diagnostic: host-side checksums printed after every launch of the layer-major schedule",
    "RNNT_GM_DBG": "diagnostic: greedy_multi writes phase stamps into a buffer of their own",
    "RNNT_GM_DBG_STREAM": "diagnostic: which row's stamps the host prints",
    "RNNT_TIMING": "diagnostic: host timers printed to stderr",
    "RNNT_BF_TILE": "removed with the 128-row tiles (named in §10 as gone)",
    "RNNT_COOP": "removed with the cooperative decoder (named in §10 as gone)",
    "RNNT_DEC_KF": "removed with the greedy_stream instantiations nothing used (named in §10 as gone)",
}


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
    "gemm_bw_c1<4>": [i for i in KNOB_CASES["RNNT_BW_NW"] if i.endswith("-bw4")],
    "gemm_bw<4>": [i for i in KNOB_CASES["RNNT_BW_NW"] if i.endswith("-bw4-nofuse")],
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
    "gemm_ns<2,2,nt>": ["wavefront-fp32-nolm-lds2"],
    # one K block in flight (RNNT_GEMM_PD=1): names of their own
    "gemm_ns<2,2;pd1>": ["layer-1024-above-fp32-pd1", "wavefront-fp32-nolm-pd1"],
    "gemm_ns<1,2;pd1>": ["layer-1024-above-fp32-pd1", "wavefront-fp32-nolm-pd1"],
    "gemm_ns<2,2,nt;pd1>": ["wavefront-fp32-nolm-lds2-pd1"],
    "gemm_ns<2,2,tanh;pd1>": NONE + ": the joint's tanh operand (rnnt_joint and the scoring calls; the decoder side is held by its own tests)",
    "gemm16<4,1>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<4,2>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<8,1>": _ids(["layer-1024"], ["below"], ["fp32"]) + _ids(["conv2-2048"], modes=["fp32"]) + [WINDOW, WHOLE],
    "gemm16<8,2>": NONE + ": no encoder contraction has K >= 1024 with N >= 512 (front-end and decoder shapes)",
    # layer-major schedule
    "lm_ctx_in": _ids(variants=LM),
    "ffn_as<8>": _ids(modes=SPLIT, variants=["default", "nofuse", "unchained"]) + [WHOLE],
    "ffn_as<4>": [i for i in KNOB_CASES["RNNT_FFN_NW"] if i.endswith("ffn4")],
    "ffn_as<16>": [i for i in KNOB_CASES["RNNT_FFN_NW"] if i.endswith("ffn16")],
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
    "gemm_bf_tab<1,1>": [WHOLE] + [f"wavefront-unfused-{m}" for m in SPLIT], "gemm_bf_tab<1,2>": [WHOLE] + [f"wavefront-unfused-{m}" for m in SPLIT],
    "gemm_ns_tab<1,1,32>": [WF_ID, WHOLE], "gemm_ns_tab<1,1,64>": [WF_ID, WHOLE], "gemm_ns_tab<1,2,32>": [WF_ID, WHOLE],
    "gemm_ns_tab<1,1,32;pd1>": ["wavefront-fp32-nolm-pd1"], "gemm_ns_tab<1,1,64;pd1>": ["wavefront-fp32-nolm-pd1"], "gemm_ns_tab<1,2,32;pd1>": ["wavefront-fp32-nolm-pd1"],
    "gemm16_tab<4,1,1>": [WF_ID, WHOLE], "gemm16_tab<8,1,1>": [WF_ID, WHOLE], "gemm16_tab<4,1,2>": [WHOLE],
    "gemm16_tab<4,2,4>": [WF_ID],                        # ffn w_1 and pointwise_conv1 of the single-descriptor stages: 1024 rows x N >= 512
    # the two larger tiles need n * maxM * N >= 2 097 152 (K < 1024) / >= 524 288 (K = 1024): in a default context one descriptor of
    # >= 2048 rows (two or more go to gemm_ns_tab); under RNNT_GEMM_NS=0 the two-descriptor stages of the 64 x 16 row case reach both
    "gemm16_tab<4,4,4>": ["wavefront-fp32-nolm-ns0"],
    "gemm16_tab<8,2,4>": ["wavefront-fp32-nolm-ns0"],
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
