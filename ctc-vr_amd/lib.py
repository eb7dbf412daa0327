"""ctypes binding of librnnt_hip.so (include/rnnt_hip.h).  Fails loudly when the HIP library is
missing or a call returns an error: there is no CPU fallback in the product path."""
import ctypes
import os

import numpy as np

from . import build as _build

c_i32, c_i64, c_f32p, c_i32p, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p


class RnntConfig(ctypes.Structure):
    _fields_ = [("max_streams", c_i32), ("max_chunk_frames", c_i32), ("max_cache_frames", c_i32),
                ("max_enc_frames", c_i32), ("max_tokens", c_i32), ("vocab_size", c_i32), ("blank_id", c_i32),
                ("n_steps", c_i32), ("device", c_i32), ("max_beam", c_i32)]


class RnntEndpointConfig(ctypes.Structure):
    """rnnt_endpoint_config: blank threshold in (0, 1), S, and the three rules in encoder frames (0: rule off)."""
    _fields_ = [("blank_threshold", ctypes.c_float), ("min_speech_frames", c_i32), ("rule1_trailing", c_i32), ("rule2_trailing", c_i32),
                ("rule3_frames", c_i32)]


# symbol -> (restype, argtypes); exactly the entry points declared in include/rnnt_hip.h
SIGNATURES = {
    "rnnt_create": (c_i32, [ctypes.POINTER(RnntConfig), ctypes.POINTER(c_vp)]),
    "rnnt_destroy": (None, [c_vp]),
    "rnnt_last_error": (ctypes.c_char_p, [c_vp]),
    "rnnt_abi_version": (c_i32, []),
    "rnnt_live_device_bytes": (c_i64, []),
    "rnnt_load_tensor": (c_i32, [c_vp, ctypes.c_char_p, c_vp, c_i32, ctypes.POINTER(c_i64)]),
    "rnnt_decode_ragged": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "rnnt_load_packed": (c_i32, [c_vp, c_vp, c_i64, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_i32), ctypes.POINTER(c_i64)]),
    "rnnt_finalize_weights": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_streams_reset": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_encoder_chunk": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32p, c_vp]),
    "rnnt_encoder_chunks": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32p, c_vp]),
    "rnnt_greedy_decode": (c_i32, [c_vp, c_vp]),
    "rnnt_get_tokens": (c_i32, [c_vp, c_vp, c_vp, c_vp]),
    "rnnt_frames_consume": (c_i32, [c_vp, c_vp]),
    "rnnt_beam_frame": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_beam_select": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_beam_get_states": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_beam_advance": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp]),
    "rnnt_beam_hyp_count": (c_i32, [c_vp, c_i32, c_i32p]),
    "rnnt_beam_get_hyp": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32p, ctypes.POINTER(ctypes.c_double)]),
    "rnnt_beam_merge_host": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_beam_decode": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp]),
    "rnnt_beam_merge_device": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_encode_ragged": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "rnnt_frames_discard": (c_i32, [c_vp, c_vp]),
    "rnnt_stream_open": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_pool_chunk": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_tokens": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_pool_chunk_beam": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_beam": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32p, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_stream_get_beam_states": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_predictor_step": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_joint": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "rnnt_encoder_full": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_ctc_argmax": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_ctc_logprobs": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp]),
    "rnnt_prefix_beam_decode": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_merge_host": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_merge_device": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_beam_decode_ctx": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp,
                                            c_vp, c_vp, c_vp]),
    "rnnt_prefix_merge_ctx_host": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, ctypes.c_double, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_merge_ctx_device": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                             c_vp, c_vp]),
    "rnnt_context_set": (c_i32, [c_vp, c_i32, c_vp, c_vp, ctypes.c_double]),
    "rnnt_context_walk_host": (c_i32, [c_i32, c_vp, c_vp, ctypes.c_double, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_context_dump_host": (c_i32, [c_i32, c_vp, c_vp, ctypes.c_double, c_i32p, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_host": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, ctypes.c_double, c_i32, c_vp, c_vp, c_vp,
                                          c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_logprobs": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_decode": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_stream_ctc_prefix_reset": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_pool_ctc_prefix_logprobs": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    "rnnt_pool_chunk_ctc_prefix": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_ctc_prefix": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32p, c_vp]),
    "rnnt_ngram_set": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "rnnt_ngram_walk_host": (c_i32, [c_i32, c_vp, c_vp, c_vp, c_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp,
                                     ctypes.POINTER(ctypes.c_double), c_i32p]),
    "rnnt_ngram_score": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_logprobs_ngram": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_decode_ngram": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_ctc_prefix_beam_ngram_host": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, ctypes.c_double, c_i32, c_vp, c_vp, c_vp, c_vp,
                                                ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_pool_ctc_prefix_logprobs_ngram": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp]),
    "rnnt_pool_chunk_ctc_prefix_ngram": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_ctc_prefix_ngram": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32p, c_vp]),
    "rnnt_stream_prefix_reset": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_pool_prefix_frames": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_vp]),
    "rnnt_pool_chunk_prefix": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, ctypes.c_float, ctypes.c_float, c_i32p, c_vp]),
    "rnnt_stream_get_prefix": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_pool_prefix_frames_ctx": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_vp]),
    "rnnt_pool_chunk_prefix_ctx": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_prefix_ctx": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_beam_decode_ngram": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp,
                                              c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_prefix_merge_ngram_host": (c_i32, [c_i32] + [c_vp] * 9 + [c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, ctypes.c_double, c_i32, c_vp, c_vp, c_vp, c_vp,
                                                                  ctypes.c_double, ctypes.c_double, ctypes.c_double, c_i32] + [c_vp] * 9),
    "rnnt_prefix_merge_ngram_device": (c_i32, [c_vp, c_i32] + [c_vp] * 9 + [c_i32, c_i32, c_i32, c_i32] + [c_vp] * 10),
    "rnnt_pool_prefix_frames_ngram": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_i32, c_vp]),
    "rnnt_pool_chunk_prefix_ngram": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, ctypes.c_float, ctypes.c_float, c_i32, c_i32, c_i32p, c_vp]),
    "rnnt_stream_get_prefix_ngram": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_transducer_nll": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_ctc_nll": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "rnnt_transducer_nll_nbest": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_transducer_loss_workspace": (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "rnnt_transducer_loss": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "rnnt_transducer_loss_elem": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_vp, c_vp, c_vp, c_i64,
                                          c_vp]),
    "rnnt_transducer_loss_host": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_vp, c_vp]),
    "rnnt_ctc_loss_workspace": (c_i32, [c_i32, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "rnnt_ctc_loss": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "rnnt_ctc_loss_elem": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "rnnt_ctc_loss_host": (c_i32, [c_vp, c_i64, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "rnnt_joint_lattice_workspace": (c_i32, [c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i64)]),
    "rnnt_joint_lattice_forward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    "rnnt_joint_lattice_backward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    "rnnt_joint_lattice_backward_host": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_joint_loss_workspace": (c_i32, [c_i32, c_i32, c_i32, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "rnnt_joint_loss_forward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "rnnt_joint_loss_host": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_vp, c_vp, c_vp, c_vp,
                                     c_vp, c_vp]),
    "rnnt_joint_loss_backward": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, ctypes.c_float, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp,
                                         c_vp, c_i64, c_vp]),
    "rnnt_lstm_workspace": (c_i32, [c_i32, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "rnnt_lstm_forward": (c_i32, [c_vp] * 8 + [c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "rnnt_lstm_backward": (c_i32, [c_vp] * 7 + [c_i64, c_vp, c_vp, c_i32, c_i32] + [c_vp] * 7 + [c_i64, c_vp]),
    "rnnt_lstm_host": (c_i32, [c_vp] * 8 + [c_i32, c_i32] + [c_vp] * 10),
    "rnnt_rel_attention_workspace": (c_i32, [c_i32, c_i32, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "rnnt_rel_attention_forward": (c_i32, [c_vp] * 7 + [c_i32] * 4 + [c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    "rnnt_rel_attention_backward": (c_i32, [c_vp] * 8 + [c_i64, c_vp, c_vp] + [c_i32] * 4 + [c_vp] * 7 + [c_i64, c_vp]),
    "rnnt_rel_attention_host": (c_i32, [c_vp] * 7 + [c_i32] * 4 + [c_vp] * 8),
    "rnnt_rescore_select_host": (c_i32, [c_i32, c_vp, c_vp, ctypes.c_double, ctypes.c_double, c_vp, c_i32p]),
    "rnnt_stream_keep_frames": (c_i32, [c_vp, c_i32, c_i32, c_vp]),
    "rnnt_stream_get_frames": (c_i32, [c_vp, c_i32, c_i32, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_pool_rescore": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "rnnt_stream_endpoint": (c_i32, [c_vp, c_i32, ctypes.POINTER(RnntEndpointConfig), c_vp]),
    "rnnt_pool_endpoint_frames": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp]),
    "rnnt_pool_get_endpoints": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_ctc_blank_logprob": (c_i32, [c_vp, c_vp, c_i32, c_vp, c_vp]),
    "rnnt_endpoint_scan_host": (c_i32, [c_vp, c_i32, ctypes.POINTER(RnntEndpointConfig), c_vp]),
    "rnnt_pool_segment": (c_i32, [c_vp, c_i32, c_vp, c_i32, c_vp]),
    "rnnt_stream_get_segment": (c_i32, [c_vp, c_i32, c_i32p, c_i32p]),
    "rnnt_transducer_align": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "rnnt_transducer_align_pick": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_ctc_align": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_ctc_align_logprobs": (c_i32, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_fbank": (c_i32, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_pool_wave": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp]),
    "rnnt_stream_wave_reset": (c_i32, [c_vp, c_i32, c_vp]),
    "rnnt_stream_get_wave_state": (c_i32, [c_vp, c_i32, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, c_vp, c_i32, c_vp]),
    "rnnt_wave_stage_host": (c_i32, [c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32p, c_i32p, c_i32p, c_vp, c_i32, c_i32p]),
    "rnnt_greedy_search_full": (c_i32, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "rnnt_get_att_cache": (c_i32, [c_vp, c_i32, c_vp, c_i32p, c_vp]),
    "rnnt_get_cnn_cache": (c_i32, [c_vp, c_i32, c_vp, c_vp]),
    "rnnt_get_predictor_state": (c_i32, [c_vp, c_i32, c_vp, c_vp, c_i32p, c_vp]),
    "rnnt_get_enc_frames": (c_i32, [c_vp, c_vp, c_i32p, c_vp]),
    "rnnt_enc_frames_dev": (c_vp, [c_vp, c_i32p, c_i32p]),
    "rnnt_profile_begin": (c_i32, [c_vp, c_i32]),
    "rnnt_profile_end": (c_i32, [c_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_i64)]),
    "rnnt_form_log_begin": (c_i32, [c_vp]),
    "rnnt_form_log_end": (c_i32, [c_vp, ctypes.c_char_p, c_i64, ctypes.POINTER(c_i64)]),
    "rnnt_get_counters": (c_i32, [c_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
}

_LIB = None

# numerics modes of rnnt_finalize_weights (include/rnnt_hip.h RNNT_NUMERICS_*)
NUMERICS = {"fp32": 0, "bf16x3": 1, "bf16": 2, "f16x3": 3}


def numerics_id(mode=None):
    """None -> $RNNT_NUMERICS or "fp32" (the exact-f32 parity mode); accepts the names above or their integer ids."""
    if mode is None:
        mode = os.environ.get("RNNT_NUMERICS", "fp32")
    if isinstance(mode, str):
        if mode not in NUMERICS:
            raise ValueError(f"unknown numerics mode {mode!r}: one of {sorted(NUMERICS)}")
        return NUMERICS[mode]
    return int(mode)


class RnntError(RuntimeError):
    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status      # the call's rnnt_status (None: not from a library call)


# rnnt_status values of a refusal (call outside its supported range / sequence), as opposed to a HIP failure
ERR_ARG, ERR_STATE = -1, -5
ERR_SHAPE = -2
ERR_OOM = -3          # a device allocation was refused


def load(build_if_needed=True):
    """Load (building in-tree with hipcc when sources are newer) librnnt_hip.so."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (soname libamdhip64.so.7).
    # Importing torch FIRST makes the loader resolve our NEEDED libamdhip64.so.7 to that already-loaded
    # runtime; loading ours first would pull in /opt/rocm's copy and the second runtime finds no device.
    import torch  # noqa: F401
    tlib = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(tlib):
        ctypes.CDLL(tlib, mode=ctypes.RTLD_GLOBAL)
    path = _build.lib_path()
    if build_if_needed and _build.needs_build() and os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        _build.build()
    if not os.path.exists(path):
        raise RnntError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    _LIB = lib
    return lib


def live_device_bytes():
    """rnnt_live_device_bytes: device bytes the contexts of this process hold at this moment."""
    return int(load().rnnt_live_device_bytes())


def _np_ptr(a):
    return a.ctypes.data_as(c_vp)


def _prefix_merge_call(fn, head, hyps, top_lp, top_tok, blank, beam_size, tail=(), graph=None):
    """Flat arguments of rnnt_prefix_merge_host / rnnt_prefix_merge_device -> the call's return value and
    [(tokens, score, src_row, src_slot)] of the survivors.  graph not None: the _ctx forms -- hyps [(tokens, score, context state,
    context score)], graph the host form's phrase arguments (() for the device form), survivors with (context state, context
    score) appended."""
    n = len(hyps)
    hl = np.array([len(h[0]) for h in hyps], np.int32)
    ht = np.array([x for h in hyps for x in h[0]] or [0], np.int32)
    hs = np.array([h[1] for h in hyps], np.float64)
    tl = np.ascontiguousarray(top_lp, np.float32).reshape(n, -1)
    tt = np.ascontiguousarray(top_tok, np.int32).reshape(n, -1)
    k = tl.shape[1]
    assert tt.shape == tl.shape
    cap = max(beam_size, 1)
    out_len, out_tok = np.zeros(cap, np.int32), np.zeros(cap * (int(hl.max(initial=0)) + 1) + 1, np.int32)
    out_sc, out_row, out_slot = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    hyp_ctx = out_ctx = ()
    if graph is not None:
        hst, hcs = np.array([h[2] for h in hyps], np.int32), np.array([h[3] for h in hyps], np.float64)
        out_st, out_cs = np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        hyp_ctx, out_ctx = (_np_ptr(hst), _np_ptr(hcs)), (_np_ptr(out_st), _np_ptr(out_cs))
    m = fn(*head, n, _np_ptr(hl), _np_ptr(ht), _np_ptr(hs), *hyp_ctx, _np_ptr(tl), _np_ptr(tt), k, blank, beam_size, *(graph or ()),
           _np_ptr(out_len), _np_ptr(out_tok), _np_ptr(out_sc), _np_ptr(out_row), _np_ptr(out_slot), *out_ctx, *tail)
    out, o = [], 0
    for a in range(max(m, 0)):
        ctx_part = (int(out_st[a]), float(out_cs[a])) if graph is not None else ()
        out.append((out_tok[o:o + out_len[a]].tolist(), float(out_sc[a]), int(out_row[a]), int(out_slot[a])) + ctx_part)
        o += out_len[a]
    return m, out


def prefix_merge_host(hyps, top_lp, top_tok, blank, beam_size):
    """rnnt_prefix_merge_host (no context, no GPU): one frame's merge of the prefix beam search for one utterance.  hyps
    [(tokens, score)], top_lp / top_tok [n][k] -> [(tokens, score, src_row, src_slot)] of the survivors, best first."""
    m, out = _prefix_merge_call(load().rnnt_prefix_merge_host, (), hyps, top_lp, top_tok, blank, beam_size)
    if m < 0:
        raise RnntError(f"rnnt_prefix_merge_host: bad argument (status {m})", m)
    return out


def prefix_merge_ctx_host(hyps, top_lp, top_tok, blank, beam_size, phrases, context_score):
    """rnnt_prefix_merge_ctx_host (no context, no GPU): prefix_merge_host with the context graph over `phrases`.  hyps [(tokens,
    score, context state, context score)] -> [(tokens, fused score, src_row, src_slot, context state, context score)] of the
    survivors, ordered by fused score + context score."""
    n, pl, pt = _phrase_args(phrases)
    m, out = _prefix_merge_call(load().rnnt_prefix_merge_ctx_host, (), hyps, top_lp, top_tok, blank, beam_size,
                                graph=(n, _np_ptr(pl), _np_ptr(pt), float(context_score)))
    if m < 0:
        raise RnntError(f"rnnt_prefix_merge_ctx_host: bad argument (status {m})", m)
    return out


def _prefix_merge_ngram_call(fn, head, hyps, top_lp, top_tok, blank, beam_size, mid, tail=()):
    """Flat arguments of rnnt_prefix_merge_ngram_host / _device: hyps [(tokens, score, context state, context score, n-gram state,
    n-gram score)], `mid` what the form passes between beam_size and the outputs -> the call's return value and [(tokens, fused
    score, src_row, src_slot, context state, context score, n-gram state, n-gram score)] of the survivors."""
    n = len(hyps)
    hl = np.array([len(h[0]) for h in hyps], np.int32)
    ht = np.array([x for h in hyps for x in h[0]] or [0], np.int32)
    hs, hcs, hns = (np.array([h[i] for h in hyps], np.float64) for i in (1, 3, 5))
    hst, hnst = (np.array([h[i] for h in hyps], np.int32) for i in (2, 4))
    tl = np.ascontiguousarray(top_lp, np.float32).reshape(n, -1)
    tt = np.ascontiguousarray(top_tok, np.int32).reshape(n, -1)
    assert tt.shape == tl.shape
    cap = max(beam_size, 1)
    out_len, out_tok = np.zeros(cap, np.int32), np.zeros(cap * (int(hl.max(initial=0)) + 1) + 1, np.int32)
    out_sc, out_cs, out_ns = (np.zeros(cap, np.float64) for _ in range(3))
    out_row, out_slot, out_st, out_nst = (np.zeros(cap, np.int32) for _ in range(4))
    m = fn(*head, n, _np_ptr(hl), _np_ptr(ht), _np_ptr(hs), _np_ptr(hst), _np_ptr(hcs), _np_ptr(hnst), _np_ptr(hns), _np_ptr(tl), _np_ptr(tt),
           tl.shape[1], blank, beam_size, *mid, _np_ptr(out_len), _np_ptr(out_tok), _np_ptr(out_sc), _np_ptr(out_row), _np_ptr(out_slot),
           _np_ptr(out_st), _np_ptr(out_cs), _np_ptr(out_nst), _np_ptr(out_ns), *tail)
    out, o = [], 0
    for a in range(max(m, 0)):
        out.append((out_tok[o:o + out_len[a]].tolist(), float(out_sc[a]), int(out_row[a]), int(out_slot[a]), int(out_st[a]), float(out_cs[a]),
                    int(out_nst[a]), float(out_ns[a])))
        o += out_len[a]
    return m, out


def prefix_merge_ngram_host(hyps, top_lp, top_tok, blank, beam_size, phrases, context_score, ngram, vocab):
    """rnnt_prefix_merge_ngram_host (no context, no GPU): prefix_merge_ctx_host with the NgramLM `ngram` over a vocabulary of `vocab`
    ids (None: no model; phrases None or empty: no graph).  hyps [(tokens, score, context state, context score, n-gram state, n-gram
    score)], the n-gram state a node id or -1 (the start marker) -> [(tokens, fused score, src_row, src_slot, context state, context
    score, n-gram state, n-gram score)] of the survivors, ordered by fused score (+ context score) (+ n-gram score)."""
    n, pl, pt = _phrase_args(phrases)
    a = _ngram_args(ngram)
    m, out = _prefix_merge_ngram_call(load().rnnt_prefix_merge_ngram_host, (), hyps, top_lp, top_tok, blank, beam_size,
                                      (n, _np_ptr(pl), _np_ptr(pt), float(context_score)) + _ngram_call_args(a) + (int(vocab),))
    if m < 0:
        raise RnntError(f"rnnt_prefix_merge_ngram_host: bad argument (status {m})", m)
    return out


def rescore_select(first_scores, nll, first_weight, transducer_weight):
    """rnnt_rescore_select_host (no context, no GPU): the choice of transducer_attention_rescoring among one utterance's
    hypotheses -> (best index, totals float64 [n]); total = first * first_weight + (-nll) * transducer_weight, the first of equal
    totals wins, a NaN total is never chosen."""
    fs, nl = np.ascontiguousarray(first_scores, np.float64), np.ascontiguousarray(nll, np.float64)
    assert fs.ndim == 1 and fs.shape == nl.shape
    total, best = np.zeros(max(fs.size, 1), np.float64), c_i32(0)
    rc = load().rnnt_rescore_select_host(fs.size, _np_ptr(fs), _np_ptr(nl), float(first_weight), float(transducer_weight), _np_ptr(total),
                                         ctypes.byref(best))
    if rc != 0:
        raise RnntError(f"rnnt_rescore_select_host: bad argument (status {rc})", rc)
    return best.value, total[:fs.size]


def pack_nbest(hyps, N=None, umax=None):
    """[[tokens, ...] per utterance] -> (n_hyp int32 [B], lens int32 [B, N], tokens int32 [B, N, umax]) of the n-best scoring calls;
    N / umax default to the largest count / length present (N at least 1).  Unused entries are 0 (never read)."""
    B = len(hyps)
    N = max([len(h) for h in hyps] + [1]) if N is None else N
    umax = max([len(t) for h in hyps for t in h] + [0]) if umax is None else umax
    nh = np.array([len(h) for h in hyps], np.int32)
    lens, toks = np.zeros((B, N), np.int32), np.zeros((B, N, umax), np.int32)
    for b, h in enumerate(hyps):
        for n, t in enumerate(h):
            lens[b, n] = len(t)
            toks[b, n, :len(t)] = t
    return nh, lens, toks


def _phrase_args(phrases):
    """[[token, ...], ...] -> (n, lens int32, concatenated tokens int32) of the context-graph entry points."""
    phrases = [list(map(int, ph)) for ph in (phrases or [])]
    lens = np.array([len(ph) for ph in phrases] or [0], np.int32)
    toks = np.array([t for ph in phrases for t in ph] or [0], np.int32)
    return len(phrases), lens, toks


def context_walk_host(phrases, context_score, tokens):
    """rnnt_context_walk_host (no context, no GPU): feed `tokens` through ContextGraph.forward_one_step from the root of the graph
    over `phrases` -> (step scores float64 [n], node ids int32 [n], finalize's score of the last state)."""
    n, pl, pt = _phrase_args(phrases)
    tk = np.array(list(tokens) or [0], np.int32)
    m = len(tokens)
    sc, st, fin = np.zeros(max(m, 1), np.float64), np.zeros(max(m, 1), np.int32), ctypes.c_double(0.0)
    rc = load().rnnt_context_walk_host(n, _np_ptr(pl), _np_ptr(pt), float(context_score), m, _np_ptr(tk), _np_ptr(sc), _np_ptr(st), ctypes.byref(fin))
    if rc != 0:
        raise RnntError(f"rnnt_context_walk_host: bad argument (status {rc})", rc)
    return sc[:m], st[:m], fin.value


def context_dump_host(phrases, context_score):
    """rnnt_context_dump_host: the node tables of the graph over `phrases` in node-id (creation) order -> dict of token, node_score,
    output_score, is_end, fail, output (-1: none)."""
    n, pl, pt = _phrase_args(phrases)
    cap = 1 + int(pl.sum())
    nn = c_i32(0)
    tok, end, fl, out = (np.zeros(cap, np.int32) for _ in range(4))
    ns, os_ = np.zeros(cap, np.float64), np.zeros(cap, np.float64)
    rc = load().rnnt_context_dump_host(n, _np_ptr(pl), _np_ptr(pt), float(context_score), ctypes.byref(nn), _np_ptr(tok), _np_ptr(ns), _np_ptr(os_),
                                       _np_ptr(end), _np_ptr(fl), _np_ptr(out))
    if rc != 0:
        raise RnntError(f"rnnt_context_dump_host: bad argument (status {rc})", rc)
    k = nn.value
    return {"token": tok[:k], "node_score": ns[:k], "output_score": os_[:k], "is_end": end[:k], "fail": fl[:k], "output": out[:k]}


def _ctc_prefix_out(B, beam, cap):
    w = max(beam, 1)
    return (np.zeros(B, np.int32), np.zeros((B, w), np.int32), np.zeros((B, w, cap), np.int32), np.zeros((B, w, cap), np.int32),
            np.zeros((B, w), np.float64), np.zeros((B, w), np.float64))


def _ctc_prefix_hyps(out):
    """The raw result arrays -> per utterance [(tokens, score, times, context score)] in the order the search returns."""
    nh, lens, toks, times, sc, cs = out
    return [[(toks[b, i, :lens[b, i]].tolist(), float(sc[b, i]), times[b, i, :lens[b, i]].tolist(), float(cs[b, i])) for i in range(nh[b])]
            for b in range(len(nh))]


def ctc_prefix_beam_host(lp, enc_lens, blank, beam_size, phrases=None, context_score=0.0, raw=False):
    """rnnt_ctc_prefix_beam_host (no context, no GPU): WeNet's ctc_prefix_beam_search over lp [B, T, vocab] float32, row b over its
    first enc_lens[b] frames, biased by the graph over `phrases` when given.  Per utterance [(tokens, score, times, context score)];
    raw: also the result arrays (n_hyp, lens, tokens, times, scores, context scores) as the C call filled them."""
    lp = np.ascontiguousarray(lp, np.float32)
    B, T, V = lp.shape
    el = np.ascontiguousarray(enc_lens, np.int32)
    assert el.size == B
    n, pl, pt = _phrase_args(phrases)
    cap = max(int(el.max(initial=0)), 1)
    out = _ctc_prefix_out(B, beam_size, cap)
    rc = load().rnnt_ctc_prefix_beam_host(_np_ptr(lp), _np_ptr(el), B, T, V, blank, beam_size, n, _np_ptr(pl), _np_ptr(pt), float(context_score), cap,
                                          *[_np_ptr(a) for a in out])
    if rc != 0:
        raise RnntError(f"rnnt_ctc_prefix_beam_host: bad argument (status {rc})", rc)
    return (_ctc_prefix_hyps(out), out) if raw else _ctc_prefix_hyps(out)


def _ngram_args(ngram):
    """An NgramLM (or None) -> the model arguments of the n-gram entry points: (n, lens int32, tokens int32, logp f64, bow f64,
    lm_weight, length_bonus, unk_logp), with the arrays kept alive by the tuple."""
    grams = list(ngram.ngrams) if ngram is not None else []
    lens = np.array([len(g[0]) for g in grams] or [0], np.int32)
    toks = np.array([int(t) for g in grams for t in g[0]] or [0], np.int32)
    logp = np.array([float(g[1]) for g in grams] or [0.0], np.float64)
    bow = np.array([float(g[2]) for g in grams] or [0.0], np.float64)
    w, lb, unk = (ngram.lm_weight, ngram.length_bonus, ngram.unk_logp) if ngram is not None else (0.0, 0.0, 0.0)
    return len(grams), lens, toks, logp, bow, float(w), float(lb), float(unk)


def _ngram_call_args(a):
    return (a[0], _np_ptr(a[1]), _np_ptr(a[2]), _np_ptr(a[3]), _np_ptr(a[4]), a[5], a[6], a[7])


def ngram_walk_host(ngram, vocab, blank, tokens):
    """rnnt_ngram_walk_host (no context, no GPU): feed `tokens` through the model's step from its start state -> (step scores float64
    [n], node ids int32 [n], the end term of the last state, the model's node count)."""
    a = _ngram_args(ngram)
    tk = np.array(list(tokens) or [0], np.int32)
    m = len(tokens)
    sc, st, eos, nn = np.zeros(max(m, 1), np.float64), np.zeros(max(m, 1), np.int32), ctypes.c_double(0.0), c_i32(0)
    rc = load().rnnt_ngram_walk_host(*_ngram_call_args(a), vocab, blank, m, _np_ptr(tk), _np_ptr(sc), _np_ptr(st), ctypes.byref(eos), ctypes.byref(nn))
    if rc != 0:
        raise RnntError(f"rnnt_ngram_walk_host: bad argument (status {rc})", rc)
    return sc[:m], st[:m], eos.value, nn.value


def ctc_prefix_beam_ngram_host(lp, enc_lens, blank, beam_size, phrases=None, context_score=0.0, ngram=None, raw=False):
    """rnnt_ctc_prefix_beam_ngram_host (no context, no GPU): ctc_prefix_beam_host with the NgramLM `ngram` fused.  Per utterance
    [(tokens, score, times, context score, n-gram score)]; raw: also the result arrays, the n-gram scores last."""
    lp = np.ascontiguousarray(lp, np.float32)
    B, T, V = lp.shape
    el = np.ascontiguousarray(enc_lens, np.int32)
    assert el.size == B
    n, pl, pt = _phrase_args(phrases)
    a = _ngram_args(ngram)
    cap = max(int(el.max(initial=0)), 1)
    out = _ctc_prefix_out(B, beam_size, cap)
    ls = np.zeros_like(out[4])
    rc = load().rnnt_ctc_prefix_beam_ngram_host(_np_ptr(lp), _np_ptr(el), B, T, V, blank, beam_size, n, _np_ptr(pl), _np_ptr(pt), float(context_score),
                                                *_ngram_call_args(a), cap, *[_np_ptr(x) for x in out], _np_ptr(ls))
    if rc != 0:
        raise RnntError(f"rnnt_ctc_prefix_beam_ngram_host: bad argument (status {rc})", rc)
    hyps = _ctc_prefix_ngram_hyps(out, ls)
    return (hyps, out + (ls,)) if raw else hyps


def _ctc_prefix_ngram_hyps(out, ls):
    """_ctc_prefix_hyps with the n-gram score as a fifth element."""
    nh = out[0]
    return [[h + (float(ls[b, i]),) for i, h in enumerate(row)] for b, row in zip(range(len(nh)), _ctc_prefix_hyps(out))]


def _endpoint_config(cfg):
    """RnntEndpointConfig from one, from a 5-tuple (blank_threshold, min_speech_frames, rule1, rule2, rule3) or from an object with
    those attributes (the facade's EndpointConfig)."""
    if isinstance(cfg, RnntEndpointConfig):
        return cfg
    if isinstance(cfg, (tuple, list)):
        thr, s, r1, r2, r3 = cfg
    else:
        thr, s, r1, r2, r3 = cfg.blank_threshold, cfg.min_speech_frames, cfg.rule1_trailing, cfg.rule2_trailing, cfg.rule3_frames
    return RnntEndpointConfig(float(thr), int(s), int(r1), int(r2), int(r3))


def endpoint_scan_host(blank_lp, cfg, state=None):
    """rnnt_endpoint_scan_host (no context, no GPU): the endpoint state [frames, trailing, speech, rule, at] after the float32
    log-posteriors blank_lp, starting from `state` (None: a fresh slot's zeros).  Returns a new int32 array [5]."""
    lp = np.ascontiguousarray(blank_lp, np.float32).reshape(-1)
    st = np.zeros(5, np.int32) if state is None else np.ascontiguousarray(state, np.int32).copy()
    assert st.shape == (5,)
    c = _endpoint_config(cfg)
    rc = load().rnnt_endpoint_scan_host(_np_ptr(lp) if lp.size else None, lp.size, ctypes.byref(c), _np_ptr(st))
    if rc != 0:
        raise RnntError(f"rnnt_endpoint_scan_host: bad config or argument (status {rc})", rc)
    return st


def _loss_args(targets, logit_lens, target_lens, B, umax):
    tg = np.ascontiguousarray(targets, np.int32).reshape(B, umax)
    ll, tl = np.ascontiguousarray(logit_lens, np.int32), np.ascontiguousarray(target_lens, np.int32)
    if ll.shape != (B,) or tl.shape != (B,):
        raise RnntError(f"rnnt_transducer_loss: {B} rows, but lengths of shapes {ll.shape} and {tl.shape}", ERR_ARG)
    return tg, ll, tl


LOSS_F32, LOSS_BF16, LOSS_F16 = 0, 1, 2          # RNNT_LOSS_*: the lattice element of rnnt_transducer_loss_elem

_LOSS_REFUSALS = {ERR_ARG: "a length, label, blank, element code or pointer outside its range",
                  ERR_SHAPE: "Umax > 255, too many cells or a workspace too small"}


def _loss_chk(rc, what, B, T, umax, V, blank):
    if rc != 0:
        raise RnntError(f"{what}: {_LOSS_REFUSALS.get(rc, 'HIP failure')} (B={B} T={T} Umax={umax} V={V} blank={blank}; status {rc})", rc)


def transducer_loss_workspace(B, T, U1):
    """rnnt_transducer_loss_workspace: bytes of the device workspace one rnnt_transducer_loss call of this shape needs."""
    n = c_i64(0)
    _loss_chk(load().rnnt_transducer_loss_workspace(B, T, U1, ctypes.byref(n)), "rnnt_transducer_loss_workspace", B, T, U1 - 1, "-", "-")
    return int(n.value)


def transducer_loss_host(logits, targets, logit_lens, target_lens, blank, fused_log_softmax=True, clamp=-1.0, want_grad=True):
    """rnnt_transducer_loss_host (no context, no GPU): logits [B, T, Umax + 1, V] float32 -> (nll [B] float64, grad float64 of the
    logits' shape or None).  Raises RnntError on a refusal."""
    x = np.ascontiguousarray(logits, np.float32)
    B, T, U1, V = x.shape
    tg, ll, tl = _loss_args(targets, logit_lens, target_lens, B, U1 - 1)
    nll = np.zeros(B, np.float64)
    grad = np.zeros(x.shape, np.float64) if want_grad else None
    rc = load().rnnt_transducer_loss_host(_np_ptr(x), _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, U1 - 1, V, blank,
                                          int(bool(fused_log_softmax)), float(clamp), _np_ptr(nll), _np_ptr(grad) if want_grad else None)
    _loss_chk(rc, "rnnt_transducer_loss_host", B, T, U1 - 1, V, blank)
    return nll, grad


def transducer_loss_device(logits_ptr, shape, targets, logit_lens, target_lens, blank, fused_log_softmax, clamp, nll_ptr, grad_ptr, work_ptr,
                           work_bytes, stream=None, elem=None):
    """rnnt_transducer_loss over device pointers: logits float32 of `shape` = (B, T, Umax + 1, V), nll [B] float64, grad float32 of
    `shape` or None, the workspace of transducer_loss_workspace(B, T, Umax + 1).  Launches on `stream` and returns: no synchronisation.
    elem (LOSS_F32, LOSS_BF16 or LOSS_F16) calls rnnt_transducer_loss_elem instead: logits and grad hold elements of that type."""
    B, T, U1, V = shape
    tg, ll, tl = _loss_args(targets, logit_lens, target_lens, B, U1 - 1)
    head = (logits_ptr, _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, U1 - 1, V, blank)
    tail = (int(bool(fused_log_softmax)), float(clamp), nll_ptr, grad_ptr, work_ptr, work_bytes, stream)
    if elem is None:
        _loss_chk(load().rnnt_transducer_loss(*head, *tail), "rnnt_transducer_loss", B, T, U1 - 1, V, blank)
    else:
        _loss_chk(load().rnnt_transducer_loss_elem(*head, int(elem), *tail), f"rnnt_transducer_loss_elem(elem={elem})", B, T, U1 - 1, V, blank)


_CTC_LOSS_REFUSALS = {ERR_ARG: "a length, label, blank, stride, element code or pointer outside its range",
                      ERR_SHAPE: "Lmax > 255, too many states or a workspace too small"}


def _ctc_loss_chk(rc, what, B, T, lmax, V, blank):
    if rc != 0:
        raise RnntError(f"{what}: {_CTC_LOSS_REFUSALS.get(rc, 'HIP failure')} (B={B} T={T} Lmax={lmax} V={V} blank={blank}; status {rc})", rc)


def _ctc_loss_args(targets, logit_lens, target_lens, B):
    tg = np.ascontiguousarray(targets, np.int32)
    ll, tl = np.ascontiguousarray(logit_lens, np.int32), np.ascontiguousarray(target_lens, np.int32)
    if tg.ndim != 2 or tg.shape[0] != B or ll.shape != (B,) or tl.shape != (B,):
        raise RnntError(f"rnnt_ctc_loss: {B} rows, but targets of shape {tg.shape} and lengths of shapes {ll.shape} and {tl.shape}", ERR_ARG)
    return tg, ll, tl


def ctc_loss_workspace(B, T, lmax):
    """rnnt_ctc_loss_workspace: bytes of the device workspace one rnnt_ctc_loss call of this shape needs."""
    n = c_i64(0)
    _ctc_loss_chk(load().rnnt_ctc_loss_workspace(B, T, lmax, ctypes.byref(n)), "rnnt_ctc_loss_workspace", B, T, lmax, "-", "-")
    return int(n.value)


def ctc_loss_host(logits, targets, logit_lens, target_lens, blank, fused_log_softmax=True, want_grad=True):
    """rnnt_ctc_loss_host (no context, no GPU): logits float32, indexed [b, t, v] -- a contiguous [B, T, V] array or the transposed view
    of a contiguous [T, B, V] one runs as it lies, anything else is copied -- targets [B, Lmax] -> (nll [B] float64, +inf for an
    infeasible row; grad float64 indexed and laid out like the logits, or None).  Raises RnntError on a refusal."""
    x = np.asarray(logits, np.float32)
    B, T, V = x.shape
    if not (x.transpose(1, 0, 2).flags.c_contiguous and B > 1 and T > 1):
        x = np.ascontiguousarray(x)
    tg, ll, tl = _ctc_loss_args(targets, logit_lens, target_lens, B)
    sb, st = (T * V, V) if x.flags.c_contiguous else (V, B * V)
    nll = np.zeros(B, np.float64)
    grad = None
    if want_grad:
        grad = np.zeros((B, T, V), np.float64) if x.flags.c_contiguous else np.zeros((T, B, V), np.float64).transpose(1, 0, 2)
    rc = load().rnnt_ctc_loss_host(_np_ptr(x), sb, st, _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, tg.shape[1], V, blank,
                                   int(bool(fused_log_softmax)), _np_ptr(nll), _np_ptr(grad) if want_grad else None)
    _ctc_loss_chk(rc, "rnnt_ctc_loss_host", B, T, tg.shape[1], V, blank)
    return nll, grad


def ctc_loss_device(logits_ptr, shape, strides, targets, logit_lens, target_lens, blank, fused_log_softmax, nll_ptr, grad_ptr, work_ptr,
                    work_bytes, stream=None, elem=None):
    """rnnt_ctc_loss over device pointers: frame (b, t) of `shape` = (B, T, V) starts at element b * strides[0] + t * strides[1];
    targets [B, Lmax]; nll [B] float64; grad with the logits' type and strides, or None (value only); the workspace of
    ctc_loss_workspace(B, T, Lmax).  Launches on `stream` and returns: no synchronisation.  elem (LOSS_F32, LOSS_BF16 or LOSS_F16)
    calls rnnt_ctc_loss_elem instead: logits and grad hold elements of that type."""
    B, T, V = shape
    tg, ll, tl = _ctc_loss_args(targets, logit_lens, target_lens, B)
    lmax = tg.shape[1]
    head = (logits_ptr, int(strides[0]), int(strides[1]), _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, lmax, V, blank)
    tail = (int(bool(fused_log_softmax)), nll_ptr, grad_ptr, work_ptr, work_bytes, stream)
    if elem is None:
        _ctc_loss_chk(load().rnnt_ctc_loss(*head, *tail), "rnnt_ctc_loss", B, T, lmax, V, blank)
    else:
        _ctc_loss_chk(load().rnnt_ctc_loss_elem(*head, int(elem), *tail), f"rnnt_ctc_loss_elem(elem={elem})", B, T, lmax, V, blank)


_JOINT_REFUSALS = {ERR_ARG: "a null or misaligned pointer, B, T or U1 < 1, or a length outside its range",
                   ERR_SHAPE: "V outside 4..416 or not a multiple of 4, too many cells, or a workspace too small"}
JOINT_D = 256                                    # the joint width the lattice kernels are built for


def _joint_chk(rc, what, B, T, U1, V):
    if rc != 0:
        raise RnntError(f"{what}: {_JOINT_REFUSALS.get(rc, 'HIP failure')} (B={B} T={T} U1={U1} V={V}; status {rc})", rc)


def _joint_lens(lens, B, what):
    if lens is None:
        return None
    a = np.ascontiguousarray(lens, np.int32)
    if a.shape != (B,):
        raise RnntError(f"{what}: {B} rows, but lengths of shape {a.shape}", ERR_ARG)
    return a


def joint_lattice_workspace(B, T, U1, V):
    """rnnt_joint_lattice_workspace: bytes of the device workspace one forward or backward call of this shape needs."""
    n = c_i64(0)
    _joint_chk(load().rnnt_joint_lattice_workspace(B, T, U1, V, ctypes.byref(n)), "rnnt_joint_lattice_workspace", B, T, U1, V)
    return int(n.value)


def joint_lattice_forward_device(e_ptr, p_ptr, w_ptr, b_ptr, shape, logits_ptr, work_ptr, work_bytes, stream=None):
    """rnnt_joint_lattice_forward over device pointers; shape = (B, T, U1, V).  Launches on `stream` and returns."""
    B, T, U1, V = shape
    _joint_chk(load().rnnt_joint_lattice_forward(e_ptr, p_ptr, w_ptr, b_ptr, B, T, U1, V, logits_ptr, work_ptr, work_bytes, stream),
               "rnnt_joint_lattice_forward", B, T, U1, V)


def joint_lattice_backward_device(e_ptr, p_ptr, w_ptr, g_ptr, logit_lens, target_lens, shape, de_ptr, dp_ptr, dw_ptr, db_ptr, work_ptr, work_bytes,
                                  stream=None):
    """rnnt_joint_lattice_backward over device pointers; shape = (B, T, U1, V), logit_lens / target_lens host arrays or None."""
    B, T, U1, V = shape
    ll, tl = _joint_lens(logit_lens, B, "rnnt_joint_lattice_backward"), _joint_lens(target_lens, B, "rnnt_joint_lattice_backward")
    rc = load().rnnt_joint_lattice_backward(e_ptr, p_ptr, w_ptr, g_ptr, None if ll is None else _np_ptr(ll), None if tl is None else _np_ptr(tl), B, T, U1, V,
                                            de_ptr, dp_ptr, dw_ptr, db_ptr, work_ptr, work_bytes, stream)
    _joint_chk(rc, "rnnt_joint_lattice_backward", B, T, U1, V)


def joint_lattice_backward_host(e, p, w, g, logit_lens=None, target_lens=None, out=None):
    """rnnt_joint_lattice_backward_host (no context, no GPU): e [B, T, 256], p [B, U1, 256], w [V, 256], g [B, T, U1, V] float32 ->
    (de, dp, dw, db) float64.  out: four float64 arrays to write into (a refused call leaves them alone).  Raises RnntError on a refusal."""
    e, p, w, g = (np.ascontiguousarray(a, np.float32) for a in (e, p, w, g))
    B, T, U1, V = g.shape
    if e.shape != (B, T, JOINT_D) or p.shape != (B, U1, JOINT_D) or w.shape != (V, JOINT_D):
        raise RnntError(f"rnnt_joint_lattice_backward_host: g {g.shape} wants e {(B, T, JOINT_D)}, p {(B, U1, JOINT_D)}, w {(V, JOINT_D)}; "
                        f"got {e.shape}, {p.shape}, {w.shape}", ERR_ARG)
    ll, tl = _joint_lens(logit_lens, B, "rnnt_joint_lattice_backward_host"), _joint_lens(target_lens, B, "rnnt_joint_lattice_backward_host")
    de, dp, dw, db = out if out is not None else (np.zeros(e.shape), np.zeros(p.shape), np.zeros(w.shape), np.zeros(V))
    rc = load().rnnt_joint_lattice_backward_host(_np_ptr(e), _np_ptr(p), _np_ptr(w), _np_ptr(g), None if ll is None else _np_ptr(ll),
                                                 None if tl is None else _np_ptr(tl), B, T, U1, V, _np_ptr(de), _np_ptr(dp), _np_ptr(dw), _np_ptr(db))
    _joint_chk(rc, "rnnt_joint_lattice_backward_host", B, T, U1, V)
    return de, dp, dw, db


_JOINT_LOSS_REFUSALS = {ERR_ARG: "a null or misaligned pointer, B or T < 1, or a blank, length or label outside its range",
                        ERR_SHAPE: "V outside 4..416 or not a multiple of 4, Umax > 255, too many cells, or a workspace or state too small"}


def _joint_loss_chk(rc, what, B, T, U1, V, blank):
    if rc != 0:
        raise RnntError(f"{what}: {_JOINT_LOSS_REFUSALS.get(rc, 'HIP failure')} (B={B} T={T} U1={U1} V={V} blank={blank}; status {rc})", rc)


def joint_loss_workspace(B, T, U1, V):
    """rnnt_joint_loss_workspace: (work_bytes, state_bytes) of the device buffers a fused joint-and-loss call of this shape needs."""
    wb, sb = c_i64(0), c_i64(0)
    _joint_loss_chk(load().rnnt_joint_loss_workspace(B, T, U1, V, ctypes.byref(wb), ctypes.byref(sb)), "rnnt_joint_loss_workspace", B, T, U1, V, "-")
    return int(wb.value), int(sb.value)


def joint_loss_forward_device(e_ptr, p_ptr, w_ptr, b_ptr, targets, logit_lens, target_lens, shape, blank, nll_ptr, state_ptr, state_bytes, work_ptr,
                              work_bytes, stream=None):
    """rnnt_joint_loss_forward over device pointers; shape = (B, T, Umax + 1, V), targets [B, Umax], logit_lens and target_lens [B] host
    arrays; nll [B] float64.  Launches on `stream` and returns: no synchronisation."""
    B, T, U1, V = shape
    tg, ll, tl = _loss_args(targets, logit_lens, target_lens, B, U1 - 1)
    rc = load().rnnt_joint_loss_forward(e_ptr, p_ptr, w_ptr, b_ptr, _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, U1 - 1, V, blank,
                                        nll_ptr, state_ptr, state_bytes, work_ptr, work_bytes, stream)
    _joint_loss_chk(rc, "rnnt_joint_loss_forward", B, T, U1, V, blank)


def joint_loss_backward_device(e_ptr, p_ptr, w_ptr, b_ptr, state_ptr, state_bytes, row_scale_ptr, clamp, shape, blank, de_ptr, dp_ptr, dw_ptr, db_ptr,
                               work_ptr, work_bytes, stream=None):
    """rnnt_joint_loss_backward over device pointers; shape = (B, T, Umax + 1, V), the state a forward of the same arguments left,
    row_scale [B] float32 on the device.  Launches on `stream` and returns: no host arrays, no upload, no synchronisation."""
    B, T, U1, V = shape
    rc = load().rnnt_joint_loss_backward(e_ptr, p_ptr, w_ptr, b_ptr, state_ptr, state_bytes, row_scale_ptr, float(clamp), B, T, U1 - 1, V, blank,
                                         de_ptr, dp_ptr, dw_ptr, db_ptr, work_ptr, work_bytes, stream)
    _joint_loss_chk(rc, "rnnt_joint_loss_backward", B, T, U1, V, blank)


def joint_loss_host(e, p, w, b, targets, logit_lens, target_lens, blank, clamp=-1.0, row_scale=None):
    """rnnt_joint_loss_host (no context, no GPU): e [B, T, 256], p [B, Umax + 1, 256], w [V, 256], b [V] float32 -> nll [B] float64, and
    with row_scale [B] also (de, dp, dw, db) float64 of sum_b row_scale[b] nll_b.  Float64 throughout; the lattice exists on the host."""
    e, p, w, b = (np.ascontiguousarray(a, np.float32) for a in (e, p, w, b))
    B, T, U1, V = e.shape[0], e.shape[1], p.shape[1], w.shape[0]
    if e.shape != (B, T, JOINT_D) or p.shape != (B, U1, JOINT_D) or w.shape != (V, JOINT_D) or b.shape != (V,):
        raise RnntError(f"rnnt_joint_loss_host: want e [B, T, {JOINT_D}], p [B, U1, {JOINT_D}], w [V, {JOINT_D}], b [V]; got {e.shape}, {p.shape}, "
                        f"{w.shape}, {b.shape}", ERR_ARG)
    tg, ll, tl = _loss_args(targets, logit_lens, target_lens, B, U1 - 1)
    nll = np.zeros(B, np.float64)
    rs = None if row_scale is None else np.ascontiguousarray(row_scale, np.float64).reshape(B)
    outs = None if rs is None else (np.zeros(e.shape), np.zeros(p.shape), np.zeros(w.shape), np.zeros(V))
    rc = load().rnnt_joint_loss_host(_np_ptr(e), _np_ptr(p), _np_ptr(w), _np_ptr(b), _np_ptr(tg) if tg.size else None, _np_ptr(ll), _np_ptr(tl), B, T, U1 - 1,
                                     V, blank, float(clamp), None if rs is None else _np_ptr(rs), _np_ptr(nll),
                                     *((None,) * 4 if outs is None else (_np_ptr(a) for a in outs)))
    _joint_loss_chk(rc, "rnnt_joint_loss_host", B, T, U1, V, blank)
    return nll, outs


_LSTM_REFUSALS = {ERR_ARG: "a null or misaligned pointer, B or U1 < 1, or a length outside 1..U1",
                  ERR_SHAPE: "U1 > 256, too many rows, or a workspace or state too small"}
LSTM_D = 256                                     # input and hidden width the LSTM kernels are built for


def _lstm_chk(rc, what, B, U1):
    if rc != 0:
        raise RnntError(f"{what}: {_LSTM_REFUSALS.get(rc, 'HIP failure')} (B={B} U1={U1}; status {rc})", rc)


def lstm_workspace(B, U1):
    """rnnt_lstm_workspace: (work_bytes, state_bytes) of the device buffers an LSTM forward or backward call of this shape needs."""
    wb, sb = c_i64(0), c_i64(0)
    _lstm_chk(load().rnnt_lstm_workspace(B, U1, ctypes.byref(wb), ctypes.byref(sb)), "rnnt_lstm_workspace", B, U1)
    return int(wb.value), int(sb.value)


def lstm_forward_device(x_ptr, w_ih_ptr, w_hh_ptr, b_ih_ptr, b_hh_ptr, h0_ptr, c0_ptr, lens, shape, out_ptr, hn_ptr, cn_ptr, state_ptr, state_bytes,
                        work_ptr, work_bytes, stream=None):
    """rnnt_lstm_forward over device pointers; shape = (B, U1), lens a host array [B] or None; h0 / c0 / hn / cn / state may be None.
    Launches on `stream` and returns."""
    B, U1 = shape
    ln = _joint_lens(lens, B, "rnnt_lstm_forward")
    rc = load().rnnt_lstm_forward(x_ptr, w_ih_ptr, w_hh_ptr, b_ih_ptr, b_hh_ptr, h0_ptr, c0_ptr, None if ln is None else _np_ptr(ln), B, U1, out_ptr, hn_ptr,
                                  cn_ptr, state_ptr, state_bytes, work_ptr, work_bytes, stream)
    _lstm_chk(rc, "rnnt_lstm_forward", B, U1)


def lstm_backward_device(x_ptr, w_ih_ptr, w_hh_ptr, h0_ptr, c0_ptr, out_ptr, state_ptr, state_bytes, dout_ptr, lens, shape, dx_ptr, dw_ih_ptr, dw_hh_ptr,
                         db_ptr, dh0_ptr, dc0_ptr, work_ptr, work_bytes, stream=None):
    """rnnt_lstm_backward over device pointers; shape = (B, U1), the out and state a forward of the same arguments left."""
    B, U1 = shape
    ln = _joint_lens(lens, B, "rnnt_lstm_backward")
    rc = load().rnnt_lstm_backward(x_ptr, w_ih_ptr, w_hh_ptr, h0_ptr, c0_ptr, out_ptr, state_ptr, state_bytes, dout_ptr, None if ln is None else _np_ptr(ln),
                                   B, U1, dx_ptr, dw_ih_ptr, dw_hh_ptr, db_ptr, dh0_ptr, dc0_ptr, work_ptr, work_bytes, stream)
    _lstm_chk(rc, "rnnt_lstm_backward", B, U1)


def lstm_host(x, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None, lens=None, dout=None, out=None):
    """rnnt_lstm_host (no context, no GPU): x [B, U1, 256], w_ih / w_hh [1024, 256], b_ih / b_hh [1024], h0 / c0 [B, 256] or None float32 ->
    (out, hn, cn) float64, and with dout [B, U1, 256] also (dx, dw_ih, dw_hh, db, dh0, dc0) float64.  out: the arrays to write into, in
    that order (a refused call leaves them alone).  Raises RnntError on a refusal."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    x, w_ih, w_hh, b_ih, b_hh, h0, c0, dout = (f(a) for a in (x, w_ih, w_hh, b_ih, b_hh, h0, c0, dout))
    D, G = LSTM_D, 4 * LSTM_D
    if x.ndim != 3 or x.shape[2] != D or w_ih.shape != (G, D) or w_hh.shape != (G, D) or b_ih.shape != (G,) or b_hh.shape != (G,) or \
            any(a is not None and a.shape != (x.shape[0], D) for a in (h0, c0)) or (dout is not None and dout.shape != x.shape):
        raise RnntError(f"rnnt_lstm_host: want x [B, U1, {D}], weights [{G}, {D}], biases [{G}], h0 / c0 [B, {D}], dout like x; got x {x.shape}", ERR_ARG)
    B, U1 = x.shape[:2]
    ln = _joint_lens(lens, B, "rnnt_lstm_host")
    n_out = 3 if dout is None else 9
    if out is None:
        out = [np.zeros(s) for s in ((B, U1, D), (B, D), (B, D), (B, U1, D), (G, D), (G, D), (G,), (B, D), (B, D))[:n_out]]
    p = lambda a: None if a is None else _np_ptr(a)
    rc = load().rnnt_lstm_host(p(x), p(w_ih), p(w_hh), p(b_ih), p(b_hh), p(h0), p(c0), p(ln), B, U1, p(dout), *(p(a) for a in out), *((None,) * (9 - len(out))))
    _lstm_chk(rc, "rnnt_lstm_host", B, U1)
    return tuple(out)


ATTN_H, ATTN_DK, ATTN_D = 4, 64, 256             # heads, width of a head, model width the attention kernels are built for
ATTN_TMAX = 4096                                 # the library's cap on T (include/rnnt_hip.h)
_ATTN_REFUSALS = {ERR_ARG: "a null or misaligned pointer, B or T < 1, a length outside 1..T, or num_left_chunks >= 0 without a chunk_size",
                  ERR_SHAPE: f"T > {ATTN_TMAX}, too many rows, or a workspace or state too small"}


def _attn_chk(rc, what, B, T, chunk, left):
    if rc != 0:
        raise RnntError(f"{what}: {_ATTN_REFUSALS.get(rc, 'HIP failure')} (B={B} T={T} chunk_size={chunk} num_left_chunks={left}; status {rc})", rc)


def rel_attention_workspace(B, T):
    """rnnt_rel_attention_workspace: (work_bytes, state_bytes) of the device buffers an attention forward or backward call of this shape needs."""
    wb, sb = c_i64(0), c_i64(0)
    _attn_chk(load().rnnt_rel_attention_workspace(B, T, ctypes.byref(wb), ctypes.byref(sb)), "rnnt_rel_attention_workspace", B, T, 0, -1)
    return int(wb.value), int(sb.value)


def rel_attention_forward_device(q_ptr, k_ptr, v_ptr, p_ptr, u_ptr, vb_ptr, lens, shape, chunk_size, num_left_chunks, out_ptr, state_ptr, state_bytes,
                                 work_ptr, work_bytes, stream=None):
    """rnnt_rel_attention_forward over device pointers; shape = (B, T), lens a host array [B] or None; state may be None (forward only).
    Launches on `stream` and returns."""
    B, T = shape
    ln = _joint_lens(lens, B, "rnnt_rel_attention_forward")
    rc = load().rnnt_rel_attention_forward(q_ptr, k_ptr, v_ptr, p_ptr, u_ptr, vb_ptr, None if ln is None else _np_ptr(ln), B, T, chunk_size, num_left_chunks,
                                           out_ptr, state_ptr, state_bytes, work_ptr, work_bytes, stream)
    _attn_chk(rc, "rnnt_rel_attention_forward", B, T, chunk_size, num_left_chunks)


def rel_attention_backward_device(q_ptr, k_ptr, v_ptr, p_ptr, u_ptr, vb_ptr, out_ptr, state_ptr, state_bytes, dout_ptr, lens, shape, chunk_size,
                                  num_left_chunks, dq_ptr, dk_ptr, dv_ptr, dp_ptr, du_ptr, dvb_ptr, work_ptr, work_bytes, stream=None):
    """rnnt_rel_attention_backward over device pointers; shape = (B, T), the out and state a forward of the same arguments left."""
    B, T = shape
    ln = _joint_lens(lens, B, "rnnt_rel_attention_backward")
    rc = load().rnnt_rel_attention_backward(q_ptr, k_ptr, v_ptr, p_ptr, u_ptr, vb_ptr, out_ptr, state_ptr, state_bytes, dout_ptr,
                                            None if ln is None else _np_ptr(ln), B, T, chunk_size, num_left_chunks, dq_ptr, dk_ptr, dv_ptr, dp_ptr, du_ptr,
                                            dvb_ptr, work_ptr, work_bytes, stream)
    _attn_chk(rc, "rnnt_rel_attention_backward", B, T, chunk_size, num_left_chunks)


def rel_attention_host(q, k, v, p, u, vb, lens=None, chunk_size=0, num_left_chunks=-1, dout=None):
    """rnnt_rel_attention_host (no context, no GPU): q, k, v [B, T, 256], p [T, 256], u, vb [4, 64] float32 -> (out,) float64, and with
    dout [B, T, 256] (out, dq, dk, dv, dp, du, dvb) float64.  Raises RnntError on a refusal."""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    q, k, v, p, u, vb, dout = (f(a) for a in (q, k, v, p, u, vb, dout))
    D = ATTN_D
    if q.ndim != 3 or q.shape[2] != D or k.shape != q.shape or v.shape != q.shape or p.shape != (q.shape[1], D) or u.shape != (ATTN_H, ATTN_DK) or \
            vb.shape != (ATTN_H, ATTN_DK) or (dout is not None and dout.shape != q.shape):
        raise RnntError(f"rnnt_rel_attention_host: want q, k, v, dout [B, T, {D}], p [T, {D}], u and vb [{ATTN_H}, {ATTN_DK}]; got q {q.shape}, k {k.shape}, "
                        f"v {v.shape}, p {p.shape}, u {u.shape}, vb {vb.shape}", ERR_ARG)
    B, T = q.shape[:2]
    ln = _joint_lens(lens, B, "rnnt_rel_attention_host")
    out = [np.zeros(s) for s in ((B, T, D),) + (() if dout is None else ((B, T, D), (B, T, D), (B, T, D), (T, D), (ATTN_H, ATTN_DK), (ATTN_H, ATTN_DK)))]
    ptr = lambda a: None if a is None else _np_ptr(a)
    rc = load().rnnt_rel_attention_host(ptr(q), ptr(k), ptr(v), ptr(p), ptr(u), ptr(vb), ptr(ln), B, T, int(chunk_size), int(num_left_chunks), ptr(dout),
                                        *(ptr(a) for a in out), *((None,) * (7 - len(out))))
    _attn_chk(rc, "rnnt_rel_attention_host", B, T, chunk_size, num_left_chunks)
    return tuple(out)


def wave_stage_host(carry, samples_so_far, new, final, n_fft=1024):
    """rnnt_wave_stage_host (no context, no GPU): one slot's push of the streaming front-end -- carry (float32 [n]) and the samples
    received before, `new` samples, final -> (staged row from the push's first new frame on: frame r at r * 512, first frame index,
    frames emitted, carry after the push)."""
    carry, new = np.ascontiguousarray(carry, np.float32), np.ascontiguousarray(new, np.float32)
    staged, out = np.zeros(new.size + 3 * n_fft + 1024, np.float32), np.zeros(n_fft, np.float32)
    sl, f0, nf, nc = c_i32(0), c_i32(0), c_i32(0), c_i32(0)
    rc = load().rnnt_wave_stage_host(_np_ptr(carry), carry.size, int(samples_so_far), _np_ptr(new), new.size, 1 if final else 0, n_fft, _np_ptr(staged),
                                     staged.size, ctypes.byref(sl), ctypes.byref(f0), ctypes.byref(nf), _np_ptr(out), out.size, ctypes.byref(nc))
    if rc != 0:
        raise RnntError(f"rnnt_wave_stage_host: bad argument (status {rc})", rc)
    return staged[:sl.value].copy(), f0.value, nf.value, out[:nc.value].copy()


class RnntEngine:
    """One context = one GPU = up to `max_streams` streams: lock-stepped (encoder_chunk / encoder_chunks / decode_ragged), or the
    slots of a stream pool that open, advance and close independently (stream_open / pool_chunk / stream_tokens, and per-slot beam
    search through pool_chunk_beam / stream_beam / stream_beam_states, per-slot CTC prefix beam search with hot words through
    pool_chunk_ctc_prefix / pool_ctc_prefix_logprobs / stream_ctc_prefix / stream_ctc_prefix_reset, the transducer prefix beam search per
    slot through pool_chunk_prefix / pool_prefix_frames / stream_prefix / stream_prefix_reset (with hot words: the _ctx forms), audio in per slot through
    pool_wave / wave_state / stream_wave_reset)."""

    def __init__(self, max_streams=1, max_chunk_frames=64, max_cache_frames=1024, max_enc_frames=1024, max_tokens=4096,
                 vocab_size=412, blank_id=5, n_steps=10, device=0, max_beam=0):
        self.lib = load()
        self.cfg = RnntConfig(max_streams, max_chunk_frames, max_cache_frames, max_enc_frames, max_tokens, vocab_size,
                              blank_id, n_steps, device, max_beam)
        self.ctx = c_vp()
        rc = self.lib.rnnt_create(ctypes.byref(self.cfg), ctypes.byref(self.ctx))
        if rc != 0:
            msg = self.lib.rnnt_last_error(self.ctx).decode() if self.ctx else "rnnt_create failed"
            if self.ctx:
                self.lib.rnnt_destroy(self.ctx)
                self.ctx = c_vp()
            raise RnntError(f"rnnt_create: {msg} (status {rc})", rc)
        self.n_streams = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rnnt_destroy(self.ctx)
            self.ctx = c_vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RnntError(f"{what}: {self.lib.rnnt_last_error(self.ctx).decode()} (status {rc})", rc)

    # ---- weights ----------------------------------------------------------------------------
    def load_state_dict(self, sd, stream=None, numerics=None):
        """sd: name -> float32 numpy array or torch tensor (the reference's 504-key layout); numerics: see numerics_id."""
        for name, v in sd.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            if "num_batches_tracked" in name:
                continue
            a = np.ascontiguousarray(v, dtype=np.float32)
            dims = (c_i64 * max(a.ndim, 1))(*a.shape)
            self._chk(self.lib.rnnt_load_tensor(self.ctx, name.encode(), _np_ptr(a), a.ndim, dims), f"rnnt_load_tensor({name})")
        self.numerics = numerics_id(numerics)
        self._chk(self.lib.rnnt_finalize_weights(self.ctx, self.numerics, stream), "rnnt_finalize_weights")

    def load_packed(self, blob, vocab, stream=None, numerics=None):
        """The whole state dict from ONE flat float32 blob in layout.state_dict_spec(vocab) order (num_batches_tracked slots are
        one float each and ignored): a torch tensor on this context's device (the blob dist.broadcast_packed leaves there) or a
        numpy array on the host.  One C-ABI call (rnnt_load_packed), then rnnt_finalize_weights."""
        from .layout import state_dict_spec
        spec = state_dict_spec(vocab)
        names = (ctypes.c_char_p * len(spec))(*[n.encode() for n, _, _ in spec])
        ndims = (c_i32 * len(spec))(*[len(s) for _, s, _ in spec])
        flat = [d for _, s, _ in spec for d in s]
        dims = (c_i64 * max(len(flat), 1))(*flat)
        if hasattr(blob, "data_ptr"):
            assert blob.dtype.is_floating_point and blob.element_size() == 4 and blob.is_contiguous()
            ptr, n, on_dev = blob.data_ptr(), blob.numel(), 1 if blob.is_cuda else 0
        else:
            blob = np.ascontiguousarray(blob, np.float32)
            ptr, n, on_dev = _np_ptr(blob), blob.size, 0
        self._chk(self.lib.rnnt_load_packed(self.ctx, ptr, n, on_dev, len(spec), names, ndims, dims), "rnnt_load_packed")
        self.numerics = numerics_id(numerics)
        self._chk(self.lib.rnnt_finalize_weights(self.ctx, self.numerics, stream), "rnnt_finalize_weights")

    # ---- streaming --------------------------------------------------------------------------
    def reset(self, n_streams, stream=None):
        self._chk(self.lib.rnnt_streams_reset(self.ctx, n_streams, stream), "rnnt_streams_reset")
        self.n_streams = n_streams

    def encoder_chunk(self, fbank_ptr, chunk_frames, offset, required_cache_size, stream=None):
        t = c_i32(0)
        self._chk(self.lib.rnnt_encoder_chunk(self.ctx, fbank_ptr, chunk_frames, offset, required_cache_size, ctypes.byref(t), stream),
                  "rnnt_encoder_chunk")
        return t.value

    # ---- stream pool ------------------------------------------------------------------------
    def stream_open(self, slot, stream=None):
        """rnnt_stream_open: reset ONE slot (fresh caches, zero predictor state, no tokens); no other slot is touched."""
        self._chk(self.lib.rnnt_stream_open(self.ctx, slot, stream), "rnnt_stream_open")

    def pool_chunk(self, slots, fbank_ptr, chunk_frames, offsets, required, greedy=True, stream=None):
        """rnnt_pool_chunk: one chunk of `chunk_frames` frames for every listed slot, row i of the device tensor at fbank_ptr
        ([len(slots), chunk_frames, 80]) belonging to slots[i] and encoded with (offsets[i], required[i]) at that slot's own
        position; greedy: decode + consume the new frames of exactly those slots.  Returns t', the new encoder frames per slot."""
        return self._pool_chunk("rnnt_pool_chunk", slots, fbank_ptr, chunk_frames, offsets, required, (1 if greedy else 0,), stream)

    def _pool_chunk(self, name, slots, fbank_ptr, chunk_frames, offsets, required, extra, stream):
        """What the rnnt_pool_chunk* entry points share: (slots, offsets, required) as int32 arrays of one length, the entry point's
        own arguments (extra) after them, t' back."""
        a, o, r = (np.ascontiguousarray(v, np.int32) for v in (slots, offsets, required))
        assert a.ndim == 1 and a.size == o.size == r.size
        t = c_i32(0)
        self._chk(getattr(self.lib, name)(self.ctx, a.size, _np_ptr(a), fbank_ptr, chunk_frames, _np_ptr(o), _np_ptr(r), *extra, ctypes.byref(t), stream), name)
        return t.value

    def stream_tokens(self, slot, start=0, stream=None):
        """rnnt_stream_get_tokens: tokens [start, count) of one slot."""
        n = c_i32(0)
        self._chk(self.lib.rnnt_stream_get_tokens(self.ctx, slot, start, 0, None, ctypes.byref(n), stream), "rnnt_stream_get_tokens")
        if n.value == 0:
            return []
        out = np.zeros(n.value, np.int32)
        self._chk(self.lib.rnnt_stream_get_tokens(self.ctx, slot, start, out.size, _np_ptr(out), ctypes.byref(n), stream), "rnnt_stream_get_tokens")
        return out[:min(n.value, out.size)].tolist()

    def pool_chunk_beam(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=4, stream=None):
        """rnnt_pool_chunk_beam: pool_chunk's encoder for the listed slots, then the beam recursion over the new frames of exactly
        those slots, each on its own device-resident beam; the frames are consumed.  Does not synchronise (stream_beam does).
        Returns t'.  Raises RnntError when the call refuses (max_beam = 0, beam_size > min(max_beam, 16), vocab > 512, ...)."""
        return self._pool_chunk("rnnt_pool_chunk_beam", slots, fbank_ptr, chunk_frames, offsets, required, (beam_size,), stream)

    def stream_beam(self, slot, stream=None):
        """rnnt_stream_get_beam: [(tokens, log_prob), ...] of one slot in beam order."""
        n = c_i32(0)
        self._chk(self.lib.rnnt_stream_get_beam(self.ctx, slot, 0, 0, ctypes.byref(n), None, None, None, stream), "rnnt_stream_get_beam")
        if n.value == 0:
            return []
        lens = np.zeros(n.value, np.int32)
        self._chk(self.lib.rnnt_stream_get_beam(self.ctx, slot, n.value, 0, ctypes.byref(n), _np_ptr(lens), None, None, stream), "rnnt_stream_get_beam")
        cap = max(int(lens.max()), 1)
        toks, sc = np.zeros((n.value, cap), np.int32), np.zeros(n.value, np.float64)
        self._chk(self.lib.rnnt_stream_get_beam(self.ctx, slot, n.value, cap, ctypes.byref(n), _np_ptr(lens), _np_ptr(toks), _np_ptr(sc), stream),
                  "rnnt_stream_get_beam")
        return [(toks[i, :lens[i]].tolist(), float(sc[i])) for i in range(n.value)]

    def stream_beam_states(self, slot, stream=None):
        """rnnt_stream_get_beam_states: (h, c), each [n_hyp, 256], of one slot's hypotheses in beam order."""
        n = c_i32(0)
        self._chk(self.lib.rnnt_stream_get_beam(self.ctx, slot, 0, 0, ctypes.byref(n), None, None, None, stream), "rnnt_stream_get_beam")
        h, c = np.zeros((n.value, 256), np.float32), np.zeros((n.value, 256), np.float32)
        if n.value:
            self._chk(self.lib.rnnt_stream_get_beam_states(self.ctx, slot, n.value, _np_ptr(h), _np_ptr(c), stream), "rnnt_stream_get_beam_states")
        return h, c

    def decode_ragged(self, fbank_ptr, total_frames, lens, chunk_frames, stream=None):
        """rnnt_decode_ragged: every stream over its own lens[b] frames (decode-script chunk loop), one call; returns encoder frames per stream."""
        a = np.ascontiguousarray(lens, np.int32)
        assert a.size == self.n_streams
        fo = np.zeros(self.n_streams, np.int32)
        self._chk(self.lib.rnnt_decode_ragged(self.ctx, fbank_ptr, total_frames, _np_ptr(a), chunk_frames, _np_ptr(fo), stream), "rnnt_decode_ragged")
        return fo

    def encoder_chunks(self, fbank_ptr, total_frames, starts, lens, offsets, required, stream=None, greedy=False):
        a, b, c, d = (np.ascontiguousarray(v, np.int32) for v in (starts, lens, offsets, required))
        t = c_i32(0)
        self._chk(self.lib.rnnt_encoder_chunks(self.ctx, fbank_ptr, total_frames, len(a), _np_ptr(a), _np_ptr(b), _np_ptr(c), _np_ptr(d),
                                               1 if greedy else 0, ctypes.byref(t), stream), "rnnt_encoder_chunks")
        return t.value

    def greedy_decode(self, stream=None):
        self._chk(self.lib.rnnt_greedy_decode(self.ctx, stream), "rnnt_greedy_decode")

    def frames_consume(self, stream=None):
        self._chk(self.lib.rnnt_frames_consume(self.ctx, stream), "rnnt_frames_consume")

    def token_counts(self, stream=None):
        counts = np.zeros(self.n_streams, np.int32)
        self._chk(self.lib.rnnt_get_tokens(self.ctx, _np_ptr(counts), None, stream), "rnnt_get_tokens")
        return counts

    def tokens(self, stream=None):
        counts = np.zeros(self.n_streams, np.int32)
        toks = np.zeros((self.n_streams, self.cfg.max_tokens), np.int32)
        self._chk(self.lib.rnnt_get_tokens(self.ctx, _np_ptr(counts), _np_ptr(toks), stream), "rnnt_get_tokens")
        if counts.max(initial=0) > self.cfg.max_tokens:
            raise RnntError("token buffer overflow: raise max_tokens")
        return [toks[b, :counts[b]].tolist() for b in range(self.n_streams)]

    # ---- beam search (device half) ------------------------------------------------------------
    def beam_frame(self, frame_idx, row_stream, row_tok, beam_k, stream=None):
        n, ns = len(row_stream), self.cfg.n_steps
        rs = np.ascontiguousarray(row_stream, np.int32)
        rt = np.ascontiguousarray(row_tok, np.int32)
        steps = np.zeros(n, np.int32)
        blank = np.zeros((n, ns), np.float32)
        top_lp = np.zeros((n, ns, beam_k), np.float32)
        top_tok = np.zeros((n, ns, beam_k), np.int32)
        self._chk(self.lib.rnnt_beam_frame(self.ctx, frame_idx, n, _np_ptr(rs), _np_ptr(rt), beam_k, _np_ptr(steps), _np_ptr(blank),
                                           _np_ptr(top_lp), _np_ptr(top_tok), stream), "rnnt_beam_frame")
        return steps, blank, top_lp, top_tok

    def beam_select(self, src_row, src_step, stream=None):
        a = np.ascontiguousarray(src_row, np.int32)
        b = np.ascontiguousarray(src_step, np.int32)
        self._chk(self.lib.rnnt_beam_select(self.ctx, len(a), _np_ptr(a), _np_ptr(b), stream), "rnnt_beam_select")

    def beam_advance(self, frame_begin, frame_end, beam_size, stream=None):
        """Native beam search over buffered frames [frame_begin, frame_end) of every stream (bookkeeping in the library)."""
        self._chk(self.lib.rnnt_beam_advance(self.ctx, frame_begin, frame_end, beam_size, stream), "rnnt_beam_advance")

    def beam_decode(self, frame_begin, frame_ends=None, beam_size=4, stream=None):
        """rnnt_beam_decode: the beam recursion over buffered frames [frame_begin, frame_ends[b]) of every stream, the whole frame
        loop on the device (frame_ends None: every buffered frame).  Raises RnntError when the call refuses (beam_size > 16,
        vocab > 512, RNNT_BEAM_CHAIN=0): rnnt_beam_advance is the path for those."""
        fe = None
        if frame_ends is not None:
            fe = np.ascontiguousarray(frame_ends, np.int32)
            assert fe.size == self.n_streams
        self._chk(self.lib.rnnt_beam_decode(self.ctx, frame_begin, None if fe is None else _np_ptr(fe), beam_size, stream), "rnnt_beam_decode")

    def encode_ragged(self, fbank_ptr, total_frames, lens, chunk_frames, stream=None):
        """rnnt_encode_ragged: the encoder half of decode_ragged (no greedy decode); returns encoder frames per stream, which stay
        buffered for beam_decode(0, frames)."""
        a = np.ascontiguousarray(lens, np.int32)
        assert a.size == self.n_streams
        fo = np.zeros(self.n_streams, np.int32)
        self._chk(self.lib.rnnt_encode_ragged(self.ctx, fbank_ptr, total_frames, _np_ptr(a), chunk_frames, _np_ptr(fo), stream), "rnnt_encode_ragged")
        return fo

    def beam_merge_device(self, hyps, steps, blank_lp, top_lp, top_tok, beam_size, stream=None):
        """rnnt_beam_merge_device for one stream: hyps [(tokens, score)], steps [n], blank_lp [n][n_steps], top_lp / top_tok
        [n][n_steps][k] -> [(tokens, score, src_row, src_step)] of the survivors (the shape of rnnt_beam_merge_host's results)."""
        n = len(hyps)
        hl = np.array([len(t) for t, _ in hyps], np.int32)
        ht = np.array([x for t, _ in hyps for x in t] or [0], np.int32)
        hs = np.array([sc for _, sc in hyps], np.float64)
        st = np.ascontiguousarray(steps, np.int32)
        bl = np.ascontiguousarray(blank_lp, np.float32)
        tl = np.ascontiguousarray(top_lp, np.float32)
        tt = np.ascontiguousarray(top_tok, np.int32)
        n_steps, k = tl.shape[1], tl.shape[2]
        cap = max(n, beam_size)
        out_len = np.zeros(cap, np.int32)
        out_tok = np.zeros(cap * (int(hl.max(initial=0)) + n_steps) + 1, np.int32)
        out_sc, out_row, out_step = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        m = self.lib.rnnt_beam_merge_device(self.ctx, n, _np_ptr(hl), _np_ptr(ht), _np_ptr(hs), _np_ptr(st), _np_ptr(bl), _np_ptr(tl), _np_ptr(tt),
                                            n_steps, k, beam_size, _np_ptr(out_len), _np_ptr(out_tok), _np_ptr(out_sc), _np_ptr(out_row),
                                            _np_ptr(out_step), stream)
        if m < 0:
            self._chk(m, "rnnt_beam_merge_device")
        out, o = [], 0
        for a in range(m):
            out.append((out_tok[o:o + out_len[a]].tolist(), float(out_sc[a]), int(out_row[a]), int(out_step[a])))
            o += out_len[a]
        return out

    def beam_hyps(self, b):
        """[(tokens, log_prob), ...] of stream b in device-row order."""
        n = c_i32(0)
        self._chk(self.lib.rnnt_beam_hyp_count(self.ctx, b, ctypes.byref(n)), "rnnt_beam_hyp_count")
        out = []
        for i in range(n.value):
            nt, lp = c_i32(0), ctypes.c_double(0.0)
            self._chk(self.lib.rnnt_beam_get_hyp(self.ctx, b, i, 0, None, ctypes.byref(nt), ctypes.byref(lp)), "rnnt_beam_get_hyp")
            toks = np.zeros(max(nt.value, 1), np.int32)
            self._chk(self.lib.rnnt_beam_get_hyp(self.ctx, b, i, toks.size, _np_ptr(toks), ctypes.byref(nt), ctypes.byref(lp)), "rnnt_beam_get_hyp")
            out.append((toks[:nt.value].tolist(), lp.value))
        return out

    def beam_states(self, n_rows, stream=None):
        h, c = np.zeros((n_rows, 256), np.float32), np.zeros((n_rows, 256), np.float32)
        self._chk(self.lib.rnnt_beam_get_states(self.ctx, n_rows, _np_ptr(h), _np_ptr(c), stream), "rnnt_beam_get_states")
        return h, c

    def frames_discard(self, stream=None):
        self._chk(self.lib.rnnt_frames_discard(self.ctx, stream), "rnnt_frames_discard")

    # ---- step API ---------------------------------------------------------------------------
    def predictor_step(self, tok_ptr, h_ptr, c_ptr, rows, out_ptr, h_out_ptr, c_out_ptr, stream=None):
        self._chk(self.lib.rnnt_predictor_step(self.ctx, tok_ptr, h_ptr, c_ptr, rows, out_ptr, h_out_ptr, c_out_ptr, stream), "rnnt_predictor_step")

    def joint(self, enc_ptr, pred_ptr, B, T, U, mode, out_ptr, stream=None):
        self._chk(self.lib.rnnt_joint(self.ctx, enc_ptr, pred_ptr, B, T, U, mode, out_ptr, stream), "rnnt_joint")

    def encoder_full(self, fbank_ptr, lens, B, T, out_ptr, stream=None):
        lens = np.ascontiguousarray(lens, np.int32)
        t = c_i32(0)
        self._chk(self.lib.rnnt_encoder_full(self.ctx, fbank_ptr, _np_ptr(lens), B, T, out_ptr, ctypes.byref(t), stream), "rnnt_encoder_full")
        self.n_streams = 0
        return t.value

    def ctc_argmax(self, fbank_ptr, lens, B, T, stream=None):
        lens = np.ascontiguousarray(lens, np.int32)
        tq = ((T - 3) // 2 + 1 - 3) // 2 + 1
        ids = np.zeros((B, tq), np.int32)
        t = c_i32(0)
        self._chk(self.lib.rnnt_ctc_argmax(self.ctx, fbank_ptr, _np_ptr(lens), B, T, _np_ptr(ids), ctypes.byref(t), stream), "rnnt_ctc_argmax")
        self.n_streams = 0
        return ids

    def ctc_logprobs(self, enc_ptr, rows, out_ptr, stream=None):
        self._chk(self.lib.rnnt_ctc_logprobs(self.ctx, enc_ptr, rows, out_ptr, stream), "rnnt_ctc_logprobs")

    # ---- prefix beam search ------------------------------------------------------------------
    def prefix_beam_decode(self, enc_ptr, enc_lens, B, T, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, want_states=False, stream=None):
        """rnnt_prefix_beam_decode: WeNet's CTC-fused prefix beam search over encoder frames enc [B, T, 256] on the device, row b
        over its first enc_lens[b] frames, the whole frame loop on the device.  Returns per utterance [(tokens incl. the leading
        blank, score)], best first; with want_states also (h, c), each [B, beam_size, 256] (rows beyond an utterance's hypotheses
        are zero)."""
        return self._prefix_decode(enc_ptr, enc_lens, B, T, beam_size, ctc_weight, transducer_weight, None, want_states, stream)

    def _prefix_decode(self, enc_ptr, enc_lens, B, T, beam_size, ctc_weight, transducer_weight, use_context, want_states, stream):
        """rnnt_prefix_beam_decode (use_context None) or rnnt_prefix_beam_decode_ctx (which also has a context score per hypothesis)."""
        biased = use_context is not None
        el = np.ascontiguousarray(enc_lens, np.int32)
        assert el.size == B
        w = max(beam_size, 1)
        cap = int(el.max(initial=0)) + 1
        nh, lens = np.zeros(B, np.int32), np.zeros((B, w), np.int32)
        toks, sc, cs = np.zeros((B, w, cap), np.int32), np.zeros((B, w), np.float64), np.zeros((B, w), np.float64)
        h = np.zeros((B, w, 256), np.float32) if want_states else None
        c = np.zeros((B, w, 256), np.float32) if want_states else None
        name = "rnnt_prefix_beam_decode_ctx" if biased else "rnnt_prefix_beam_decode"
        self._chk(getattr(self.lib, name)(self.ctx, enc_ptr, _np_ptr(el), B, T, beam_size, ctc_weight, transducer_weight,
                                          *((1 if use_context else 0,) if biased else ()), cap, _np_ptr(nh), _np_ptr(lens), _np_ptr(toks), _np_ptr(sc),
                                          *((_np_ptr(cs),) if biased else ()), _np_ptr(h) if want_states else None, _np_ptr(c) if want_states else None,
                                          stream), name)
        hyps = [[(toks[b, i, :lens[b, i]].tolist(), float(sc[b, i])) + ((float(cs[b, i]),) if biased else ()) for i in range(nh[b])] for b in range(B)]
        return (hyps, h, c) if want_states else hyps

    def prefix_beam_decode_ctx(self, enc_ptr, enc_lens, B, T, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=True, want_states=False,
                               stream=None):
        """rnnt_prefix_beam_decode_ctx: prefix_beam_decode biased by the graph of context_set when use_context.  Returns per
        utterance [(tokens incl. the leading blank, total score, context score)] in the search's order (finalize replaces the
        context scores at the end without a re-sort, so the totals need not descend); with want_states also (h, c)."""
        return self._prefix_decode(enc_ptr, enc_lens, B, T, beam_size, ctc_weight, transducer_weight, bool(use_context), want_states, stream)

    def prefix_beam_decode_ngram(self, enc_ptr, enc_lens, B, T, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=False, use_ngram=True,
                                 want_states=False, stream=None):
        """rnnt_prefix_beam_decode_ngram: prefix_beam_decode_ctx with the model of ngram_set fused when use_ngram.  Returns per
        utterance [(tokens incl. the leading blank, total score, context score, n-gram score)] in the search's order (the end term
        is added without a re-sort, so the totals need not descend); with want_states also (h, c)."""
        el = np.ascontiguousarray(enc_lens, np.int32)
        assert el.size == B
        w = max(beam_size, 1)
        cap = int(el.max(initial=0)) + 1
        nh, lens, toks = np.zeros(B, np.int32), np.zeros((B, w), np.int32), np.zeros((B, w, cap), np.int32)
        sc, cs, ns = (np.zeros((B, w), np.float64) for _ in range(3))
        h = np.zeros((B, w, 256), np.float32) if want_states else None
        c = np.zeros((B, w, 256), np.float32) if want_states else None
        self._chk(self.lib.rnnt_prefix_beam_decode_ngram(self.ctx, enc_ptr, _np_ptr(el), B, T, beam_size, ctc_weight, transducer_weight,
                                                         1 if use_context else 0, 1 if use_ngram else 0, cap, _np_ptr(nh), _np_ptr(lens), _np_ptr(toks),
                                                         _np_ptr(sc), _np_ptr(cs), _np_ptr(ns), _np_ptr(h) if want_states else None,
                                                         _np_ptr(c) if want_states else None, stream), "rnnt_prefix_beam_decode_ngram")
        hyps = [[(toks[b, i, :lens[b, i]].tolist(), float(sc[b, i]), float(cs[b, i]), float(ns[b, i])) for i in range(nh[b])] for b in range(B)]
        return (hyps, h, c) if want_states else hyps

    # ---- CTC prefix beam search with contextual biasing ------------------------------------------
    def context_set(self, phrases, context_score=6.0):
        """rnnt_context_set: build and upload the context graph over phrases [[token, ...], ...]; an empty list clears it."""
        n, pl, pt = _phrase_args(phrases)
        self._chk(self.lib.rnnt_context_set(self.ctx, n, _np_ptr(pl), _np_ptr(pt), float(context_score)), "rnnt_context_set")

    def _ctc_prefix(self, fn, name, dev_ptr, enc_lens, B, T, beam_size, use_context, raw, stream):
        el = np.ascontiguousarray(enc_lens, np.int32)
        assert el.size == B
        out = _ctc_prefix_out(B, beam_size, max(int(el.max(initial=0)), 1))
        self._chk(fn(self.ctx, dev_ptr, _np_ptr(el), B, T, beam_size, 1 if use_context else 0, out[2].shape[2], *[_np_ptr(a) for a in out], stream), name)
        return (_ctc_prefix_hyps(out), out) if raw else _ctc_prefix_hyps(out)

    def ctc_prefix_beam_logprobs(self, lp_ptr, enc_lens, B, T, beam_size=10, use_context=False, raw=False, stream=None):
        """rnnt_ctc_prefix_beam_logprobs: ctc_prefix_beam_search over log-probabilities [B, T, vocab] on the device, one launch.  Per
        utterance [(tokens, score, times, context score)] in the reference's order; raw as in ctc_prefix_beam_host."""
        return self._ctc_prefix(self.lib.rnnt_ctc_prefix_beam_logprobs, "rnnt_ctc_prefix_beam_logprobs", lp_ptr, enc_lens, B, T, beam_size, use_context,
                                raw, stream)

    def ctc_prefix_beam_decode(self, enc_ptr, enc_lens, B, T, beam_size=10, use_context=False, raw=False, stream=None):
        """rnnt_ctc_prefix_beam_decode: the same over encoder frames [B, T, 256] (rnnt_ctc_logprobs first)."""
        return self._ctc_prefix(self.lib.rnnt_ctc_prefix_beam_decode, "rnnt_ctc_prefix_beam_decode", enc_ptr, enc_lens, B, T, beam_size, use_context,
                                raw, stream)

    # ---- n-gram shallow fusion in the CTC prefix beam search -----------------------------------------------
    def ngram_set(self, ngram):
        """rnnt_ngram_set: build and upload the NgramLM `ngram`; None clears it."""
        a = _ngram_args(ngram)
        self._chk(self.lib.rnnt_ngram_set(self.ctx, *_ngram_call_args(a)), "rnnt_ngram_set")

    def ngram_score(self, seqs, with_eos=True, stream=None):
        """rnnt_ngram_score: the token sequences `seqs` scored by the model that is set, one launch -> (step scores float64
        [n, cap], totals float64 [n]); cap is the longest length (at least 1)."""
        n, cap = len(seqs), max([len(q) for q in seqs] + [1])
        lens, toks = np.array([len(q) for q in seqs] or [0], np.int32), np.zeros((max(n, 1), cap), np.int32)
        for i, q in enumerate(seqs):
            toks[i, :len(q)] = q
        step, tot = np.zeros((max(n, 1), cap), np.float64), np.zeros(max(n, 1), np.float64)
        self._chk(self.lib.rnnt_ngram_score(self.ctx, n, _np_ptr(lens), _np_ptr(toks), cap, 1 if with_eos else 0, _np_ptr(step), _np_ptr(tot), stream),
                  "rnnt_ngram_score")
        return step[:n], tot[:n]

    def _ctc_prefix_ngram(self, fn, name, dev_ptr, enc_lens, B, T, beam_size, use_context, use_ngram, raw, stream):
        el = np.ascontiguousarray(enc_lens, np.int32)
        assert el.size == B
        out = _ctc_prefix_out(B, beam_size, max(int(el.max(initial=0)), 1))
        ls = np.zeros_like(out[4])
        self._chk(fn(self.ctx, dev_ptr, _np_ptr(el), B, T, beam_size, 1 if use_context else 0, 1 if use_ngram else 0, out[2].shape[2],
                     *[_np_ptr(a) for a in out], _np_ptr(ls), stream), name)
        hyps = _ctc_prefix_ngram_hyps(out, ls)
        return (hyps, out + (ls,)) if raw else hyps

    def ctc_prefix_beam_logprobs_ngram(self, lp_ptr, enc_lens, B, T, beam_size=10, use_context=False, use_ngram=True, raw=False, stream=None):
        """rnnt_ctc_prefix_beam_logprobs_ngram: ctc_prefix_beam_logprobs with the model of ngram_set fused when use_ngram.  Per
        utterance [(tokens, score, times, context score, n-gram score)] in the search's order (not re-sorted after the end term)."""
        return self._ctc_prefix_ngram(self.lib.rnnt_ctc_prefix_beam_logprobs_ngram, "rnnt_ctc_prefix_beam_logprobs_ngram", lp_ptr, enc_lens, B, T, beam_size,
                                      use_context, use_ngram, raw, stream)

    def ctc_prefix_beam_decode_ngram(self, enc_ptr, enc_lens, B, T, beam_size=10, use_context=False, use_ngram=True, raw=False, stream=None):
        """rnnt_ctc_prefix_beam_decode_ngram: the same over encoder frames [B, T, 256] (rnnt_ctc_logprobs first)."""
        return self._ctc_prefix_ngram(self.lib.rnnt_ctc_prefix_beam_decode_ngram, "rnnt_ctc_prefix_beam_decode_ngram", enc_ptr, enc_lens, B, T, beam_size,
                                      use_context, use_ngram, raw, stream)

    def pool_ctc_prefix_logprobs_ngram(self, slots, lp_ptr, t, beam_size=10, use_context=False, use_ngram=True, stream=None):
        """rnnt_pool_ctc_prefix_logprobs_ngram: pool_ctc_prefix_logprobs for searches that fuse the model of ngram_set (use_ngram)."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_ctc_prefix_logprobs_ngram(self.ctx, a.size, _np_ptr(a), lp_ptr, t, beam_size, 1 if use_context else 0,
                                                               1 if use_ngram else 0, stream), "rnnt_pool_ctc_prefix_logprobs_ngram")

    def pool_chunk_ctc_prefix_ngram(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=10, use_context=False, use_ngram=True, stream=None):
        """rnnt_pool_chunk_ctc_prefix_ngram: pool_chunk_ctc_prefix for searches that fuse the model of ngram_set.  Returns t'."""
        return self._pool_chunk("rnnt_pool_chunk_ctc_prefix_ngram", slots, fbank_ptr, chunk_frames, offsets, required,
                                (beam_size, 1 if use_context else 0, 1 if use_ngram else 0), stream)

    def stream_ctc_prefix_ngram(self, slot, final=False, raw=False, stream=None):
        """rnnt_stream_get_ctc_prefix_ngram: stream_ctc_prefix with the n-gram score as a fifth element of every hypothesis (the
        running one, or with final the one with the end term; zero for a slot that fuses no model)."""
        frames, need = c_i32(0), c_i32(0)
        self._chk(self.lib.rnnt_stream_get_ctc_prefix_ngram(self.ctx, slot, 0, 0, 0, ctypes.byref(need), None, None, None, None, None, None,
                                                            ctypes.byref(frames), stream), "rnnt_stream_get_ctc_prefix_ngram")
        out = _ctc_prefix_out(1, need.value, max(frames.value, 1))
        ls = np.zeros_like(out[4])
        self._chk(self.lib.rnnt_stream_get_ctc_prefix_ngram(self.ctx, slot, 1 if final else 0, need.value, out[2].shape[2], *[_np_ptr(a) for a in out],
                                                            _np_ptr(ls), ctypes.byref(frames), stream), "rnnt_stream_get_ctc_prefix_ngram")
        hyps = _ctc_prefix_ngram_hyps(out, ls)[0]
        return (hyps, out + (ls,), frames.value) if raw else hyps

    # ---- the same search per slot of the stream pool ----------------------------------------------------
    def stream_ctc_prefix_reset(self, slot=-1, stream=None):
        """rnnt_stream_ctc_prefix_reset: the start hypothesis for one slot's CTC prefix search (-1: all slots)."""
        self._chk(self.lib.rnnt_stream_ctc_prefix_reset(self.ctx, slot, stream), "rnnt_stream_ctc_prefix_reset")

    def pool_ctc_prefix_logprobs(self, slots, lp_ptr, t, beam_size=10, use_context=False, stream=None):
        """rnnt_pool_ctc_prefix_logprobs: advance the searches of the listed slots by t frames of log-probabilities [len(slots), t, vocab]
        on the device; one launch, no synchronisation."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_ctc_prefix_logprobs(self.ctx, a.size, _np_ptr(a), lp_ptr, t, beam_size, 1 if use_context else 0, stream),
                  "rnnt_pool_ctc_prefix_logprobs")

    def pool_chunk_ctc_prefix(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=10, use_context=False, stream=None):
        """rnnt_pool_chunk_ctc_prefix: pool_chunk's encoder for the listed slots, the CTC log-probabilities of their new frames, and
        their searches advanced by those frames; the frames are consumed.  Does not synchronise (stream_ctc_prefix does).  Returns t'."""
        return self._pool_chunk("rnnt_pool_chunk_ctc_prefix", slots, fbank_ptr, chunk_frames, offsets, required, (beam_size, 1 if use_context else 0), stream)

    def stream_ctc_prefix(self, slot, final=False, raw=False, cap_hyps=None, cap_tokens=None, stream=None):
        """rnnt_stream_get_ctc_prefix: [(tokens, score, times, context score)] of one slot in the search's order, as they stand
        (final: as the one-launch search returns them had the utterance ended here).  raw: also the result arrays of a B = 1 call
        (n_hyp, lens, tokens, times, scores, context scores) and the frames walked.  cap_hyps / cap_tokens None: what the slot needs
        (its beam and the frames it has walked, asked of the library first: a host-only call), so a read costs what it returns."""
        frames = c_i32(0)
        if cap_hyps is None or cap_tokens is None:
            need = c_i32(0)
            self._chk(self.lib.rnnt_stream_get_ctc_prefix(self.ctx, slot, 0, 0, 0, ctypes.byref(need), None, None, None, None, None,
                                                          ctypes.byref(frames), stream), "rnnt_stream_get_ctc_prefix")
            cap_hyps = need.value if cap_hyps is None else cap_hyps
            cap_tokens = frames.value if cap_tokens is None else cap_tokens
        out = _ctc_prefix_out(1, cap_hyps, max(cap_tokens, 1))
        self._chk(self.lib.rnnt_stream_get_ctc_prefix(self.ctx, slot, 1 if final else 0, cap_hyps, out[2].shape[2], *[_np_ptr(a) for a in out],
                                                      ctypes.byref(frames), stream), "rnnt_stream_get_ctc_prefix")
        hyps = _ctc_prefix_hyps(out)[0]
        return (hyps, out, frames.value) if raw else hyps

    # ---- the transducer prefix beam search per slot of the stream pool ----------------------------------
    def stream_prefix_reset(self, slot=-1, stream=None):
        """rnnt_stream_prefix_reset: the start hypothesis [blank] for one slot's transducer prefix search (-1: all slots)."""
        self._chk(self.lib.rnnt_stream_prefix_reset(self.ctx, slot, stream), "rnnt_stream_prefix_reset")

    def pool_prefix_frames(self, slots, enc_ptr, t, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, stream=None):
        """rnnt_pool_prefix_frames: advance the prefix beam searches of the listed slots by t encoder frames [len(slots), t, 256] on
        the device; two launches per frame, no synchronisation."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_prefix_frames(self.ctx, a.size, _np_ptr(a), enc_ptr, t, beam_size, ctc_weight, transducer_weight, stream),
                  "rnnt_pool_prefix_frames")

    def pool_chunk_prefix(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, stream=None):
        """rnnt_pool_chunk_prefix: pool_chunk's encoder for the listed slots and their prefix beam searches advanced by the new frames;
        the frames are consumed.  Does not synchronise (stream_prefix does).  Returns t'."""
        return self._pool_chunk("rnnt_pool_chunk_prefix", slots, fbank_ptr, chunk_frames, offsets, required, (beam_size, ctc_weight, transducer_weight), stream)

    def pool_prefix_frames_ctx(self, slots, enc_ptr, t, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=True, stream=None):
        """rnnt_pool_prefix_frames_ctx: pool_prefix_frames for searches biased by the graph of context_set (use_context)."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_prefix_frames_ctx(self.ctx, a.size, _np_ptr(a), enc_ptr, t, beam_size, ctc_weight, transducer_weight,
                                                       1 if use_context else 0, stream), "rnnt_pool_prefix_frames_ctx")

    def pool_chunk_prefix_ctx(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=True,
                              stream=None):
        """rnnt_pool_chunk_prefix_ctx: pool_chunk_prefix for searches biased by the graph of context_set (use_context).  Returns t'."""
        return self._pool_chunk("rnnt_pool_chunk_prefix_ctx", slots, fbank_ptr, chunk_frames, offsets, required,
                                (beam_size, ctc_weight, transducer_weight, 1 if use_context else 0), stream)

    def pool_prefix_frames_ngram(self, slots, enc_ptr, t, beam_size=5, ctc_weight=0.3, transducer_weight=0.7, use_context=False, use_ngram=True, stream=None):
        """rnnt_pool_prefix_frames_ngram: pool_prefix_frames_ctx for searches that fuse the model of ngram_set (use_ngram)."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_prefix_frames_ngram(self.ctx, a.size, _np_ptr(a), enc_ptr, t, beam_size, ctc_weight, transducer_weight,
                                                         1 if use_context else 0, 1 if use_ngram else 0, stream), "rnnt_pool_prefix_frames_ngram")

    def pool_chunk_prefix_ngram(self, slots, fbank_ptr, chunk_frames, offsets, required, beam_size=5, ctc_weight=0.3, transducer_weight=0.7,
                                use_context=False, use_ngram=True, stream=None):
        """rnnt_pool_chunk_prefix_ngram: pool_chunk_prefix_ctx for searches that fuse the model of ngram_set.  Returns t'."""
        return self._pool_chunk("rnnt_pool_chunk_prefix_ngram", slots, fbank_ptr, chunk_frames, offsets, required,
                                (beam_size, ctc_weight, transducer_weight, 1 if use_context else 0, 1 if use_ngram else 0), stream)

    def stream_prefix_ngram(self, slot, final=False, states=False, stream=None):
        """rnnt_stream_get_prefix_ngram: [(tokens incl. the leading blank, total score, context score, n-gram score)] of one slot in
        the search's order, as they stand (final: finalize's context scores and the n-gram scores with the end term, what the
        one-call search returns had the utterance ended here; zero n-gram scores for a slot that fuses no model); with states also
        (h, c), each [n_hyp, 256].  Reading changes nothing."""
        w, _, cap = self.stream_prefix_size(slot)
        nh, lens, toks = np.zeros(1, np.int32), np.zeros(w, np.int32), np.zeros((w, cap), np.int32)
        sc, cs, ns = (np.zeros(w, np.float64) for _ in range(3))
        h = np.zeros((w, 256), np.float32) if states else None
        c = np.zeros((w, 256), np.float32) if states else None
        self._chk(self.lib.rnnt_stream_get_prefix_ngram(self.ctx, slot, 1 if final else 0, w, cap, _np_ptr(nh), _np_ptr(lens), _np_ptr(toks), _np_ptr(sc),
                                                        _np_ptr(cs), _np_ptr(ns), _np_ptr(h) if states else None, _np_ptr(c) if states else None, stream),
                  "rnnt_stream_get_prefix_ngram")
        n = int(nh[0])
        hyps = [(toks[i, :lens[i]].tolist(), float(sc[i]), float(cs[i]), float(ns[i])) for i in range(n)]
        return (hyps, h[:n], c[:n]) if states else hyps

    def stream_prefix_ctx(self, slot, final=False, states=False, stream=None):
        """rnnt_stream_get_prefix_ctx: [(tokens incl. the leading blank, total score, context score)] of one slot in the search's
        order, as they stand (final: finalize's context scores, what the one-call search returns had the utterance ended here);
        with states also (h, c), each [n_hyp, 256].  Reading changes nothing."""
        return self._stream_prefix(slot, bool(final), states, stream)

    def _stream_prefix(self, slot, final, states, stream):
        """rnnt_stream_get_prefix (final None) or rnnt_stream_get_prefix_ctx (which also has a context score per hypothesis).  Sized
        by the library's size query first (a host-only call), so a read costs what it returns."""
        biased = final is not None
        w, _, cap = self.stream_prefix_size(slot)
        nh, lens = np.zeros(1, np.int32), np.zeros(w, np.int32)
        toks, sc, cs = np.zeros((w, cap), np.int32), np.zeros(w, np.float64), np.zeros(w, np.float64)
        h = np.zeros((w, 256), np.float32) if states else None
        c = np.zeros((w, 256), np.float32) if states else None
        name = "rnnt_stream_get_prefix_ctx" if biased else "rnnt_stream_get_prefix"
        self._chk(getattr(self.lib, name)(self.ctx, slot, *((1 if final else 0,) if biased else ()), w, cap, _np_ptr(nh), _np_ptr(lens), _np_ptr(toks),
                                          _np_ptr(sc), *((_np_ptr(cs),) if biased else ()), _np_ptr(h) if states else None,
                                          _np_ptr(c) if states else None, stream), name)
        n = int(nh[0])
        hyps = [(toks[i, :lens[i]].tolist(), float(sc[i])) + ((float(cs[i]),) if biased else ()) for i in range(n)]
        return (hyps, h[:n], c[:n]) if states else hyps

    def stream_prefix_size(self, slot):
        """rnnt_stream_get_prefix's size query (host only): (beam, frames walked, bound on the longest token list) of one slot."""
        need = np.zeros(3, np.int32)
        self._chk(self.lib.rnnt_stream_get_prefix(self.ctx, slot, 0, 0, _np_ptr(need), None, None, None, None, None, None), "rnnt_stream_get_prefix")
        return int(need[0]), int(need[1]), int(need[2])

    def stream_prefix(self, slot, states=False, stream=None):
        """rnnt_stream_get_prefix: [(tokens incl. the leading blank, score)] of one slot, best first, as they stand; with states also
        (h, c), each [n_hyp, 256].  Sized by the library's size query first (a host-only call), so a read costs what it returns."""
        return self._stream_prefix(slot, None, states, stream)

    def pool_wave(self, slots, wave_ptr, n_samples, samples, final, out_ptr, cap_frames, sample_rate=16000, n_fft=1024, stream=None):
        """rnnt_pool_wave: the streaming feature front-end for the listed slots -- row i of the device tensor at wave_ptr
        ([len(slots), n_samples] float32) holds samples[i] new samples of slots[i], final[i]: its utterance ends with them; the new
        frames of row i go to row i of the device tensor at out_ptr ([len(slots), cap_frames, 80]).  Returns the frames written per
        row (int32 [len(slots)]).  Does not synchronise."""
        a, n, f = (np.ascontiguousarray(v, np.int32) for v in (slots, samples, [1 if x else 0 for x in final]))
        assert a.ndim == 1 and a.size == n.size == f.size
        frames = np.zeros(a.size, np.int32)
        self._chk(self.lib.rnnt_pool_wave(self.ctx, a.size, _np_ptr(a), wave_ptr, n_samples, _np_ptr(n), _np_ptr(f), sample_rate, n_fft, out_ptr,
                                          cap_frames, _np_ptr(frames), stream), "rnnt_pool_wave")
        return frames

    def stream_wave_reset(self, slot, stream=None):
        """rnnt_stream_wave_reset: a fresh utterance for one slot's front-end (-1: all slots)."""
        self._chk(self.lib.rnnt_stream_wave_reset(self.ctx, slot, stream), "rnnt_stream_wave_reset")

    def wave_state(self, slot, stream=None):
        """rnnt_stream_get_wave_state: dict of samples, frames, sample_rate, n_fft, finished and carry (float32 array) of one slot;
        synchronises."""
        v = [c_i32(0) for _ in range(6)]
        self._chk(self.lib.rnnt_stream_get_wave_state(self.ctx, slot, *[ctypes.byref(x) for x in v], None, 0, stream), "rnnt_stream_get_wave_state")
        carry = np.zeros(max(v[5].value, 1), np.float32)
        self._chk(self.lib.rnnt_stream_get_wave_state(self.ctx, slot, *[ctypes.byref(x) for x in v], _np_ptr(carry), carry.size, stream),
                  "rnnt_stream_get_wave_state")
        return {"samples": v[0].value, "frames": v[1].value, "sample_rate": v[2].value, "n_fft": v[3].value, "finished": bool(v[4].value),
                "carry": carry[:v[5].value]}

    wave_stage_host = staticmethod(wave_stage_host)

    def prefix_merge_device(self, hyps, top_lp, top_tok, blank, beam_size, stream=None):
        """rnnt_prefix_merge_device: prefix_merge_host's arguments and results through one prefix_merge launch."""
        m, out = _prefix_merge_call(self.lib.rnnt_prefix_merge_device, (self.ctx,), hyps, top_lp, top_tok, blank, beam_size, (stream,))
        if m < 0:
            self._chk(m, "rnnt_prefix_merge_device")
        return out

    def prefix_merge_ngram_device(self, hyps, top_lp, top_tok, blank, beam_size, use_context=False, stream=None):
        """rnnt_prefix_merge_ngram_device: prefix_merge_ngram_host's hypotheses and results through one prefix_merge launch with the
        model of ngram_set and, when use_context, the graph of context_set."""
        m, out = _prefix_merge_ngram_call(self.lib.rnnt_prefix_merge_ngram_device, (self.ctx,), hyps, top_lp, top_tok, blank, beam_size,
                                          (1 if use_context else 0,), (stream,))
        if m < 0:
            self._chk(m, "rnnt_prefix_merge_ngram_device")
        return out

    def prefix_merge_ctx_device(self, hyps, top_lp, top_tok, blank, beam_size, stream=None):
        """rnnt_prefix_merge_ctx_device: prefix_merge_ctx_host's hypotheses and results through one prefix_merge launch with the
        graph of context_set."""
        m, out = _prefix_merge_call(self.lib.rnnt_prefix_merge_ctx_device, (self.ctx,), hyps, top_lp, top_tok, blank, beam_size, (stream,), graph=())
        if m < 0:
            self._chk(m, "rnnt_prefix_merge_ctx_device")
        return out

    def _score_args(self, enc_lens, targets, target_lens, B):
        el, tl = np.ascontiguousarray(enc_lens, np.int32), np.ascontiguousarray(target_lens, np.int32)
        tg = np.ascontiguousarray(targets, np.int32)
        tg = tg.reshape(B, tg.size // B)
        assert el.size == B and tl.size == B
        return el, tg, tl, tg.shape[1]

    def transducer_nll(self, enc_ptr, enc_lens, targets, target_lens, B, T, pick_ptr=None, stream=None):
        """rnnt_transducer_nll: per-row transducer negative log-likelihood (float64 [B]) of targets [B, Umax] given encoder frames
        enc [B, T, 256] on the device; pick_ptr: optional device float [B, T, Umax + 1, 2] receiving the picked lattice."""
        el, tg, tl, umax = self._score_args(enc_lens, targets, target_lens, B)
        nll = np.zeros(B, np.float64)
        self._chk(self.lib.rnnt_transducer_nll(self.ctx, enc_ptr, _np_ptr(el), _np_ptr(tg), _np_ptr(tl), B, T, umax, _np_ptr(nll), pick_ptr, stream),
                  "rnnt_transducer_nll")
        return nll

    # ---- two-pass decoding -----------------------------------------------------------------------
    @staticmethod
    def _nbest_args(n_hyp, hyp_lens, hyp_tokens, B):
        nh, hl = np.ascontiguousarray(n_hyp, np.int32), np.ascontiguousarray(hyp_lens, np.int32)
        assert nh.size == B and hl.ndim == 2 and hl.shape[0] == B
        N = hl.shape[1]
        ht = np.ascontiguousarray(hyp_tokens, np.int32)
        ht = ht.reshape(B, N, ht.size // (B * N))
        return nh, hl, ht, N, ht.shape[2]

    def transducer_nll_nbest(self, enc_ptr, enc_lens, n_hyp, hyp_lens, hyp_tokens, B, T, pick_ptr=None, stream=None):
        """rnnt_transducer_nll_nbest: transducer negative log-likelihood (float64 [B, N]) of N hypotheses per utterance -- n_hyp [B],
        hyp_lens [B, N], hyp_tokens [B, N, Umax] (pack_nbest) -- over encoder frames enc [B, T, 256] on the device, projected once;
        0 where n >= n_hyp[b].  pick_ptr: optional device float [B, T, N * (Umax + 1), 2] receiving the picked lattice."""
        el = np.ascontiguousarray(enc_lens, np.int32)
        nh, hl, ht, N, umax = self._nbest_args(n_hyp, hyp_lens, hyp_tokens, B)
        assert el.size == B
        nll = np.zeros((B, N), np.float64)
        self._chk(self.lib.rnnt_transducer_nll_nbest(self.ctx, enc_ptr, _np_ptr(el), _np_ptr(nh), _np_ptr(hl), _np_ptr(ht), B, T, N, umax, _np_ptr(nll),
                                                     pick_ptr, stream), "rnnt_transducer_nll_nbest")
        return nll

    rescore_select = staticmethod(rescore_select)

    def stream_keep_frames(self, slot, keep=True, stream=None):
        """rnnt_stream_keep_frames: from now on the pool calls that encode `slot` append its encoder outputs to the slot's history
        (valid on a slot that has not advanced since it was opened); keep=False clears the flag and the length."""
        self._chk(self.lib.rnnt_stream_keep_frames(self.ctx, slot, 1 if keep else 0, stream), "rnnt_stream_keep_frames")

    # ---- endpoint detection per slot of the stream pool --------------------------------------------------
    def stream_endpoint(self, slot, cfg, stream=None):
        """rnnt_stream_endpoint: from now on the pool calls that encode `slot` advance its endpoint state (valid on a slot that has
        not advanced since it was opened); cfg: see _endpoint_config, None turns it off."""
        c = None if cfg is None else ctypes.byref(_endpoint_config(cfg))
        self._chk(self.lib.rnnt_stream_endpoint(self.ctx, slot, c, stream), "rnnt_stream_endpoint")

    def pool_endpoint_frames(self, slots, enc_ptr, t, stream=None):
        """rnnt_pool_endpoint_frames: advance the endpoint states of the listed slots by t encoder frames [len(slots), t, 256] on the
        device; one launch, no synchronisation."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_endpoint_frames(self.ctx, a.size, _np_ptr(a), enc_ptr, t, stream), "rnnt_pool_endpoint_frames")

    def pool_endpoints(self, slots, stream=None):
        """rnnt_pool_get_endpoints: int32 [len(slots), 5] = frames, trailing, speech, rule, at of the listed slots; one download."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        out = np.zeros((a.size, 5), np.int32)
        self._chk(self.lib.rnnt_pool_get_endpoints(self.ctx, a.size, _np_ptr(a), _np_ptr(out), stream), "rnnt_pool_get_endpoints")
        return out

    def ctc_blank_logprob(self, enc_ptr, rows, out_ptr, stream=None):
        """rnnt_ctc_blank_logprob: out [rows] = log_softmax(ctc_lo(enc))[blank] for enc [rows, 256] on the device."""
        self._chk(self.lib.rnnt_ctc_blank_logprob(self.ctx, enc_ptr, rows, out_ptr, stream), "rnnt_ctc_blank_logprob")

    endpoint_scan_host = staticmethod(endpoint_scan_host)

    # ---- segments: the next utterance in a slot that stays open -------------------------------------------
    def pool_segment(self, slots, keep_encoder=True, stream=None):
        """rnnt_pool_segment: a new segment in the listed slots -- their decoders, endpoint counters and history length start over;
        keep_encoder=False restarts their encoder too (the next chunk's offset is 0).  One copy, one launch, no synchronisation."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        self._chk(self.lib.rnnt_pool_segment(self.ctx, a.size, _np_ptr(a), 1 if keep_encoder else 0, stream), "rnnt_pool_segment")

    def stream_segment(self, slot):
        """rnnt_stream_get_segment: (index, start_frame) of the slot's current segment (host only)."""
        index, start = c_i32(0), c_i32(0)
        self._chk(self.lib.rnnt_stream_get_segment(self.ctx, slot, ctypes.byref(index), ctypes.byref(start)), "rnnt_stream_get_segment")
        return index.value, start.value

    def stream_frames_len(self, slot):
        """frames in the slot's history (host only); RnntError(ERR_STATE) on a slot that keeps none"""
        n = c_i32(0)
        self._chk(self.lib.rnnt_stream_get_frames(self.ctx, slot, 0, 0, None, ctypes.byref(n), None), "rnnt_stream_get_frames")
        return n.value

    def stream_frames(self, slot, start=0, stream=None):
        """rnnt_stream_get_frames: frames [start, len) of the slot's history as a device tensor [len - start, 256] (a copy, made on
        `stream`: torch's current stream when None)."""
        import torch
        n = max(self.stream_frames_len(slot) - start, 0)
        out = torch.empty(n, 256, device=torch.device("cuda", self.cfg.device), dtype=torch.float32)
        if n:
            s = torch.cuda.current_stream(out.device).cuda_stream if stream is None else stream
            self._chk(self.lib.rnnt_stream_get_frames(self.ctx, slot, start, n, out.data_ptr(), None, s), "rnnt_stream_get_frames")
        return out

    def pool_rescore(self, slots, n_hyp, hyp_lens, hyp_tokens, stream=None):
        """rnnt_pool_rescore: transducer_nll_nbest over the kept frames of the listed slots, one call -> float64 [len(slots), N]."""
        a = np.ascontiguousarray(slots, np.int32)
        assert a.ndim == 1
        nh, hl, ht, N, umax = self._nbest_args(n_hyp, hyp_lens, hyp_tokens, a.size)
        nll = np.zeros((a.size, N), np.float64)
        self._chk(self.lib.rnnt_pool_rescore(self.ctx, a.size, _np_ptr(a), _np_ptr(nh), _np_ptr(hl), _np_ptr(ht), N, umax, _np_ptr(nll), stream),
                  "rnnt_pool_rescore")
        return nll

    def ctc_nll(self, enc_ptr, enc_lens, targets, target_lens, B, T, stream=None):
        """rnnt_ctc_nll: per-row CTC negative log-likelihood (float64 [B], +inf where the frames cannot hold the transcript)."""
        el, tg, tl, umax = self._score_args(enc_lens, targets, target_lens, B)
        nll = np.zeros(B, np.float64)
        self._chk(self.lib.rnnt_ctc_nll(self.ctx, enc_ptr, _np_ptr(el), _np_ptr(tg), _np_ptr(tl), B, T, umax, _np_ptr(nll), stream), "rnnt_ctc_nll")
        return nll

    def transducer_align(self, enc_ptr, enc_lens, targets, target_lens, B, T, want_nll=False, pick_ptr=None, stream=None):
        """rnnt_transducer_align: the best alignment of targets [B, Umax] over encoder frames enc [B, T, 256] on the device ->
        (best float64 [B], emit int32 [B, max(Umax, 1)]: the frame of each label, -1 beyond a row's length), plus nll float64 [B]
        (what transducer_nll returns) when want_nll; pick_ptr as in transducer_nll."""
        el, tg, tl, umax = self._score_args(enc_lens, targets, target_lens, B)
        best, emit = np.zeros(B, np.float64), np.zeros((B, max(umax, 1)), np.int32)
        nll = np.zeros(B, np.float64) if want_nll else None
        self._chk(self.lib.rnnt_transducer_align(self.ctx, enc_ptr, _np_ptr(el), _np_ptr(tg), _np_ptr(tl), B, T, umax, _np_ptr(best), _np_ptr(emit),
                                                 _np_ptr(nll) if want_nll else None, pick_ptr, stream), "rnnt_transducer_align")
        return (best, emit, nll) if want_nll else (best, emit)

    def transducer_align_pick(self, pick_ptr, enc_lens, target_lens, B, T, umax, stream=None):
        """rnnt_transducer_align_pick: the same over a picked lattice [B, T, umax + 1, 2] already on the device -> (best, emit)."""
        el, tl = np.ascontiguousarray(enc_lens, np.int32), np.ascontiguousarray(target_lens, np.int32)
        assert el.size == B and tl.size == B
        best, emit = np.zeros(B, np.float64), np.zeros((B, max(umax, 1)), np.int32)
        self._chk(self.lib.rnnt_transducer_align_pick(self.ctx, pick_ptr, _np_ptr(el), _np_ptr(tl), B, T, umax, _np_ptr(best), _np_ptr(emit), stream),
                  "rnnt_transducer_align_pick")
        return best, emit

    def ctc_align(self, enc_ptr, enc_lens, targets, target_lens, B, T, stream=None):
        """rnnt_ctc_align: CTC forced alignment -> (best float64 [B], -inf where the frames cannot hold the transcript; align int32
        [B, T]: the label (blank included) of each frame, -1 beyond a row's frames and on an infeasible row)."""
        return self._ctc_align(self.lib.rnnt_ctc_align, "rnnt_ctc_align", enc_ptr, enc_lens, targets, target_lens, B, T, stream)

    def ctc_align_logprobs(self, lp_ptr, enc_lens, targets, target_lens, B, T, stream=None):
        """rnnt_ctc_align_logprobs: the same over log-probabilities [B, T, vocab] already on the device."""
        return self._ctc_align(self.lib.rnnt_ctc_align_logprobs, "rnnt_ctc_align_logprobs", lp_ptr, enc_lens, targets, target_lens, B, T, stream)

    def _ctc_align(self, fn, name, dev_ptr, enc_lens, targets, target_lens, B, T, stream):
        el, tg, tl, umax = self._score_args(enc_lens, targets, target_lens, B)
        best, align = np.zeros(B, np.float64), np.zeros((B, T), np.int32)
        self._chk(fn(self.ctx, dev_ptr, _np_ptr(el), _np_ptr(tg), _np_ptr(tl), B, T, umax, _np_ptr(best), _np_ptr(align), stream), name)
        return best, align

    def greedy_search_full(self, fbank_ptr, lens, B, T, n_steps=64, stream=None):
        """Offline greedy search over the full-context encoder (model/component/transducer.py:22-70) -> list of token lists."""
        lens = np.ascontiguousarray(lens, np.int32)
        counts = np.zeros(B, np.int32)
        toks = np.zeros((B, self.cfg.max_tokens), np.int32)
        self._chk(self.lib.rnnt_greedy_search_full(self.ctx, fbank_ptr, _np_ptr(lens), B, T, n_steps, _np_ptr(counts), _np_ptr(toks), stream),
                  "rnnt_greedy_search_full")
        self.n_streams = 0
        if counts.max(initial=0) > self.cfg.max_tokens:
            raise RnntError("token buffer overflow: raise max_tokens")
        return [toks[b, :counts[b]].tolist() for b in range(B)]

    def fbank(self, wave_ptr, B, n_samples, sample_rate, out_ptr, n_fft=1024, stream=None):
        """Device feature front-end (data/dataloader.py:15-41): wave [B, n_samples] -> out [B, 1 + n_samples // 512, 80]."""
        t = c_i32(0)
        self._chk(self.lib.rnnt_fbank(self.ctx, wave_ptr, B, n_samples, sample_rate, n_fft, out_ptr, ctypes.byref(t), stream), "rnnt_fbank")
        return t.value

    # ---- state read-back ----------------------------------------------------------------------
    def att_cache(self, b=0, stream=None):
        n = c_i32(0)
        self._chk(self.lib.rnnt_get_att_cache(self.ctx, b, None, ctypes.byref(n), stream), "rnnt_get_att_cache")
        out = np.zeros((12, 4, n.value, 128), np.float32)
        if n.value:
            self._chk(self.lib.rnnt_get_att_cache(self.ctx, b, _np_ptr(out), ctypes.byref(n), stream), "rnnt_get_att_cache")
        return out

    def cnn_cache(self, b=0, stream=None):
        out = np.zeros((12, 1, 256, 30), np.float32)
        self._chk(self.lib.rnnt_get_cnn_cache(self.ctx, b, _np_ptr(out), stream), "rnnt_get_cnn_cache")
        return out

    def predictor_state(self, b=0, stream=None):
        h, c, tok = np.zeros(256, np.float32), np.zeros(256, np.float32), c_i32(0)
        self._chk(self.lib.rnnt_get_predictor_state(self.ctx, b, _np_ptr(h), _np_ptr(c), ctypes.byref(tok), stream), "rnnt_get_predictor_state")
        return h, c, tok.value

    def enc_frames(self, stream=None):
        n = c_i32(0)
        self._chk(self.lib.rnnt_get_enc_frames(self.ctx, None, ctypes.byref(n), stream), "rnnt_get_enc_frames")
        out = np.zeros((self.n_streams, n.value, 256), np.float32)
        if n.value:
            self._chk(self.lib.rnnt_get_enc_frames(self.ctx, _np_ptr(out), ctypes.byref(n), stream), "rnnt_get_enc_frames")
        return out

    def profile_begin(self, tag):
        self._chk(self.lib.rnnt_profile_begin(self.ctx, tag), "rnnt_profile_begin")

    def profile_end(self):
        ms, n = ctypes.c_double(0), c_i64(0)
        self._chk(self.lib.rnnt_profile_end(self.ctx, ctypes.byref(ms), ctypes.byref(n)), "rnnt_profile_end")
        return ms.value, n.value

    def form_log_begin(self):
        """Start counting every launch of this context under the form name of its launch site (rnnt_form_log_begin)."""
        self._chk(self.lib.rnnt_form_log_begin(self.ctx), "rnnt_form_log_begin")

    def form_log_end(self):
        """Stop the log -> {form name: launches}, e.g. {"gemm_bf<2,2>": 1, "ffn_as<8>": 36, ...}."""
        need = c_i64(0)
        self._chk(self.lib.rnnt_form_log_end(self.ctx, None, 0, ctypes.byref(need)), "rnnt_form_log_end")
        buf = ctypes.create_string_buffer(need.value)
        self._chk(self.lib.rnnt_form_log_end(self.ctx, buf, need.value, ctypes.byref(need)), "rnnt_form_log_end")
        return {name: int(n) for name, n in (line.split("\t") for line in buf.value.decode().splitlines())}

    def counters(self):
        a, b = c_i64(0), c_i64(0)
        self._chk(self.lib.rnnt_get_counters(self.ctx, ctypes.byref(a), ctypes.byref(b)), "rnnt_get_counters")
        return a.value, b.value
