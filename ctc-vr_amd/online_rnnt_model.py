"""Host-side mirror of the reference's OnlineRNNTModel (model/online_rnnt_model.py:58-671) over the
HIP library.  Same constructor keywords, method names, argument meaning, return shapes and error
behaviour for the streaming inference path; the arithmetic runs in librnnt_hip.so (gfx950 kernels),
never on the CPU.  PyTorch is used only for device memory and streams.

Additions over the reference (which is batch-1 only, :277-278,348-349): `StreamingBatch`, B lock-stepped
independent streams in one context, and `StreamPool`, slots of one context that open, advance and close
independently (callers that connect and hang up whenever they like); each stream's result equals the
reference's B=1 result.
"""
from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .lib import ERR_ARG, ERR_SHAPE, ERR_STATE, RnntEngine, RnntError, pack_nbest, rescore_select
from .ngram import NgramLM


def _stream_ptr():
    return torch.cuda.current_stream().cuda_stream


class BeamHypothesis:
    """model/online_rnnt_model.py:41-55."""

    def __init__(self, tokens: List[int], log_prob: float, predictor_states=None):
        self.tokens = tokens
        self.log_prob = log_prob
        self.predictor_states = predictor_states

    def __lt__(self, other):
        return self.log_prob < other.log_prob

    def copy(self):
        return BeamHypothesis(tokens=self.tokens.copy(), log_prob=self.log_prob, predictor_states=self.predictor_states)


def beam_advance_frame(engine, frame_idx, beams, blank_id, beam_size, stream=None):
    """Host half of one encoder frame of _decode_chunk_beam_search (model/online_rnnt_model.py:419-518) for a
    list of per-stream beams (each a list of BeamHypothesis whose device rows are numbered in list order,
    streams concatenated).  The device evaluates every hypothesis' extension chain (rnnt_beam_frame); here the
    candidates are rebuilt in the reference's order (per hypothesis, per step: blank candidate, then the top-k
    non-blank), scored in Python floats (double), sorted stably in descending order (:506), de-duplicated
    first-wins on the token tuple (:508-516) and truncated to the beam."""
    row_stream, row_tok = [], []
    for b, beam in enumerate(beams):
        for h in beam:
            row_stream.append(b)
            row_tok.append(h.tokens[-1] if h.tokens else blank_id)          # :429
    k = min(beam_size, engine.cfg.vocab_size - 1)                            # :467
    steps, blank_lp, top_lp, top_tok = engine.beam_frame(frame_idx, row_stream, row_tok, k, stream)
    new_beams, src_row, src_step = [], [], []
    r = 0
    for b, beam in enumerate(beams):
        cands = []
        for h in beam:
            toks, lp = list(h.tokens), h.log_prob
            n = int(steps[r])
            for st in range(n):
                cands.append((toks.copy(), lp + float(blank_lp[r, st]), r, st))                 # blank: old state
                for j in range(k):
                    cands.append((toks + [int(top_tok[r, st, j])], lp + float(top_lp[r, st, j]), r, st + 1))
                if st < n - 1:                                                                   # chain continued (:489-499)
                    toks.append(int(top_tok[r, st, 0]))
                    lp += float(top_lp[r, st, 0])
            r += 1
        cands.sort(key=lambda c: c[1], reverse=True)
        uniq, seen = [], set()
        for c in cands:
            t = tuple(c[0])
            if t not in seen:
                uniq.append(c)
                seen.add(t)
                if len(uniq) >= beam_size:
                    break
        uniq = uniq[:beam_size]
        new_beams.append([BeamHypothesis(c[0], c[1]) for c in uniq])
        src_row.extend(c[2] for c in uniq)
        src_step.extend(c[3] for c in uniq)
    engine.beam_select(src_row, src_step, stream)
    return new_beams


def compose_losses(nll_rnnt, nll_ctc, text_lens, ctc_weight):
    """The loss composition of the reference's forward with texts (model/online_rnnt_model.py:247-263) from per-utterance
    negative log-likelihoods, in float64 on the host: loss_rnnt = mean(nll_rnnt) (rnnt_loss reduction="mean"); total =
    (1 - ctc_weight) * loss_rnnt; with nll_ctc given (the caller passes it only when ctc_weight > 0 and the head is loaded),
    loss_ctc = mean over the batch of nll_b / max(L_b, 1) with infinite terms zeroed (nn.CTCLoss(reduction="mean",
    zero_infinity=True), :22-23) and total += ctc_weight * loss_ctc.  Returns (total, loss_dict) with the reference's keys."""
    nll_rnnt = np.asarray(nll_rnnt, np.float64)
    loss_rnnt = float(nll_rnnt.mean())
    loss_dict = {"loss_rnnt": loss_rnnt}
    total = (1.0 - ctc_weight) * loss_rnnt
    if nll_ctc is not None:
        per = np.asarray(nll_ctc, np.float64).copy()
        per[~np.isfinite(per)] = 0.0
        loss_ctc = float((per / np.maximum(np.asarray(text_lens, np.float64), 1.0)).mean())
        loss_dict["loss_ctc"] = loss_ctc
        total = total + ctc_weight * loss_ctc
    return total, loss_dict


def peaks_from_ctc_alignment(align, blank_id=0):
    """The peak frame of each token of a per-frame CTC alignment (blank included), the semantics of WeNet's gen_ctc_peak_time
    (wenet/utils/ctc_utils.py): the first frame of every run of equal non-blank labels."""
    peaks, t, n = [], 0, len(align)
    while t < n:
        if align[t] != blank_id:
            peaks.append(t)
        first = t
        while t < n and align[t] == align[first]:
            t += 1
    return peaks


def timestamps_from_peaks(peaks, max_duration, frame_rate=0.04, max_token_duration=1.0):
    """[(start_s, end_s)] per token from its peak frame, the semantics of WeNet's gen_timestamps_from_peak: a token reaches half
    way to its neighbours' peaks but at most max_token_duration / 2 from its own, the first one not before 0 and the last one
    not beyond max_duration.  Same operations in the same order, so the floats are equal."""
    half = max_token_duration / 2
    last = len(peaks) - 1
    times = []
    for i, pk in enumerate(peaks):
        start = max(0, pk * frame_rate - half) if i == 0 else max((peaks[i - 1] + pk) / 2 * frame_rate, pk * frame_rate - half)
        end = min(max_duration, pk * frame_rate + half) if i == last else min((pk + peaks[i + 1]) / 2 * frame_rate, pk * frame_rate + half)
        times.append((start, end))
    return times


def check_rescoring_args(attn_weight=0.0, reverse_weight=0.0, decoding_chunk_size=-1, beam_search_type="transducer"):
    """What transducer_attention_rescoring cannot do here, said before anything runs (ValueError)."""
    if attn_weight != 0:
        raise ValueError(f"attn_weight={attn_weight}: this model has no attention decoder, so there is no attention score to weigh (pass 0)")
    if reverse_weight != 0:
        raise ValueError(f"reverse_weight={reverse_weight}: this model has no (right-to-left) attention decoder (pass 0)")
    if decoding_chunk_size != -1:
        raise ValueError(f"decoding_chunk_size={decoding_chunk_size}: rescoring runs on the full-context encoder, like the other offline "
                         "searches (pass -1); chunked two-pass decoding is StreamPool.rescore")
    if beam_search_type not in ("transducer", "ctc"):
        raise ValueError(f"beam_search_type={beam_search_type!r}: 'transducer' or 'ctc'")


def select_rescored(hyps, first_scores, nll, first_weight, transducer_weight):
    """One utterance's (best_index, [(tokens, first_score, td_score, total)]) in the first pass's order: td_score = -nll and the
    choice of rnnt_rescore_select_host (wenet/transducer/transducer.py:372-393 with attn_weight = 0).  nll None: no valid frame to
    score against -- td_score = nan, best_index = 0."""
    if nll is None:
        return 0, [(list(t), float(f), float("nan"), float("nan")) for t, f in zip(hyps, first_scores)]
    best, total = rescore_select(first_scores, nll, first_weight, transducer_weight)
    return best, [(list(t), float(f), -float(x), float(tt)) for t, f, x, tt in zip(hyps, first_scores, nll, total)]


class ContextBias:
    """Hot words for OnlineRNNTModel.ctc_prefix_beam_search: phrases as lists of token ids (no blank, no empty phrase) and the bonus
    per matched token, as the reference's ContextGraph(context_score=6.0) takes them after tokenisation."""

    def __init__(self, phrases: List[List[int]], context_score: float = 6.0):
        self.phrases = [[int(t) for t in ph] for ph in phrases]
        self.context_score = float(context_score)


class _EncoderView:
    """Attribute surface the reference's callers read: encoder.static_chunk_size and
    encoder.embed.subsampling_rate (model/online_rnnt_model.py:283-287)."""

    class _Embed:
        subsampling_rate = 4
        right_context = 6

    def __init__(self, static_chunk_size):
        self.static_chunk_size = static_chunk_size
        self.embed = self._Embed()


class OnlineRNNTModel:
    """Drop-in for the streaming-inference surface of the reference class of the same name."""

    def __init__(self, input_dim: int = 80, hidden_dim: int = 256, vocab_size: int = 4336, blank_id: int = 0,
                 streaming: bool = True, static_chunk_size: int = 32, use_dynamic_chunk: bool = True,
                 ctc_weight: float = 0.3, predictor_layers: int = 1, predictor_dropout: float = 0.1,
                 ctc_dropout_rate: float = 0.1, rnnt_loss_clamp: float = -1.0, ignore_id: int = -1,
                 # engine sizing (not in the reference)
                 max_streams: int = 1, max_chunk_frames: int = 256, max_cache_frames: int = 1024,
                 max_enc_frames: int = 1024, max_tokens: int = 8192, device: int = 0, max_beam: int = 8, numerics=None):
        if input_dim != 80 or hidden_dim != 256 or predictor_layers != 1:
            raise ValueError("the HIP path implements the reference's configured architecture: input_dim=80, hidden_dim=256, predictor_layers=1")
        self.blank_id = blank_id
        self.vocab_size = vocab_size
        self.streaming = streaming
        self.ctc_weight = ctc_weight
        self.ignore_id = ignore_id
        self.rnnt_loss_clamp = rnnt_loss_clamp
        self.encoder_output_size = hidden_dim
        self.encoder = _EncoderView(static_chunk_size if streaming else 0)
        self.device = torch.device("cuda", device)
        self._engine = RnntEngine(max_streams=max_streams, max_chunk_frames=max_chunk_frames, max_cache_frames=max_cache_frames,
                                  max_enc_frames=max_enc_frames, max_tokens=max_tokens, vocab_size=vocab_size, blank_id=blank_id,
                                  n_steps=10, device=device, max_beam=max_beam)
        self.numerics = numerics          # None -> $RNNT_NUMERICS or "fp32" (lib.numerics_id)
        self._loaded = False
        self._context_bias = None         # the ContextBias whose graph the context holds (ctc_prefix_beam_search, prefix_beam_search_batch)
        self._ngram_lm = None             # the NgramLM whose model the context holds (ctc_prefix_beam_search, prefix_beam_search_batch, rescoring_batch)
        self._chunks_done = None          # None = reset_streaming_cache not called yet (attributes are None, :138-143)
        self._tok_count = 0
        self.streaming_beam_hypotheses = None
        self._global_encoder_offset = 0

    # ---- nn.Module-like plumbing ------------------------------------------------------------------
    def eval(self):
        return self

    def to(self, device):
        return self

    def load_state_dict(self, state_dict, strict: bool = True):
        self._engine.load_state_dict(state_dict, numerics=self.numerics)
        self._loaded = True
        self._ctc_loaded = "ctc_head.ctc_lo.weight" in state_dict and "ctc_head.ctc_lo.bias" in state_dict

    # ---- streaming state (model/online_rnnt_model.py:138-164) ----------------------------------------
    def extract_audio_features(self, waveform, sample_rate, n_fft=1024):
        """Device version of data/dataloader.py:extract_audio_features: waveform [n] or [B, n] -> [.., 1 + n // 512, 80] dB
        mel features on this model's GPU (ctc_vr_amd.features)."""
        from .features import extract_audio_features
        return extract_audio_features(self._engine, waveform, sample_rate, n_fft=n_fft)

    def reset_streaming_cache(self, device=None):
        self._require_loaded()
        self._engine.reset(1, _stream_ptr())
        self._chunks_done = 0
        self._tok_count = 0
        self.streaming_beam_hypotheses = None
        self._global_encoder_offset = 0

    @property
    def streaming_att_cache(self) -> Optional[torch.Tensor]:
        if self._chunks_done is None:
            return None
        if self._chunks_done == 0:
            return torch.zeros((0, 0, 0, 0), device=self.device)
        return torch.from_numpy(self._engine.att_cache(0, _stream_ptr())).to(self.device)

    @property
    def streaming_cnn_cache(self) -> Optional[torch.Tensor]:
        if self._chunks_done is None:
            return None
        if self._chunks_done == 0:
            return torch.zeros((0, 0, 0, 0), device=self.device)
        return torch.from_numpy(self._engine.cnn_cache(0, _stream_ptr())).to(self.device)

    @property
    def streaming_predictor_states(self) -> Optional[List[torch.Tensor]]:
        if not self._chunks_done:
            return None
        h, c, _ = self._engine.predictor_state(0, _stream_ptr())
        return [torch.from_numpy(h).view(1, 1, 256).to(self.device), torch.from_numpy(c).view(1, 1, 256).to(self.device)]

    @property
    def streaming_last_emitted_token(self) -> int:
        if not self._chunks_done:
            return self.blank_id
        return self._engine.predictor_state(0, _stream_ptr())[2]

    def _require_loaded(self):
        if not self._loaded:
            raise RnntError("load_state_dict() must be called before streaming")

    # ---- one chunk, greedy (model/online_rnnt_model.py:166-222, 346-387) -----------------------------
    def _decode_chunk_streaming_logic(self, chunk_xs: torch.Tensor, offset: int, required_cache_size: int) -> List[int]:
        x = chunk_xs.to(self.device, torch.float32).contiguous()
        s = _stream_ptr()
        self._engine.encoder_chunk(x.data_ptr(), x.size(1), offset, required_cache_size, s)
        self._engine.greedy_decode(s)
        toks = self._engine.tokens(s)[0]
        new = toks[self._tok_count:]
        self._tok_count = len(toks)
        self._engine.frames_consume(s)
        self._chunks_done += 1
        return new

    def process_single_chunk(self, chunk_audio: torch.Tensor, chunk_len: torch.Tensor) -> Tuple[List[int], None, None]:
        assert self.streaming, "Model is not in streaming mode for process_single_chunk."
        assert chunk_audio.size(0) == 1, "Single chunk processing currently supports batch size 1 only."
        if self._chunks_done is None:
            self.reset_streaming_cache()
        if chunk_audio.size(1) < 7:
            print(f"Warning: Chunk too small ({chunk_audio.size(1)} frames), skipping")
            return [], None, None
        subsampling_rate = self.encoder.embed.subsampling_rate
        off = self._global_encoder_offset
        hyp = self._decode_chunk_streaming_logic(chunk_audio, off, off)
        self._global_encoder_offset += chunk_audio.size(1) // subsampling_rate
        return hyp, None, None

    # ---- whole utterance, greedy (model/online_rnnt_model.py:274-344) --------------------------------
    def _utterance_chunks(self, n_frames: int, chunk_size_ms: Optional[int]):
        sr = self.encoder.embed.subsampling_rate
        frames = (self.encoder.static_chunk_size if self.encoder.static_chunk_size > 0 else 16) * sr
        if chunk_size_ms is not None:
            frames = int(chunk_size_ms / 10)
        min_frames = max(16, sr * 4)
        if frames < min_frames:
            if n_frames >= min_frames:
                frames = min_frames
            else:
                if n_frames < 7:
                    return None
                frames = n_frames
        plan = []
        cur = 0
        while cur < n_frames:
            end = min(cur + frames, n_frames)
            if end - cur == 0:
                break
            if end - cur >= 7:
                plan.append((cur, end, cur // sr))
            cur = end
        return plan

    def streaming_inference(self, audios: torch.Tensor, audio_lens: torch.Tensor,
                            chunk_size_ms: Optional[int] = None) -> Tuple[List[List[int]], None, None]:
        assert self.streaming, "Model is not in streaming mode for streaming_inference."
        assert audios.size(0) == 1, "Streaming inference currently supports batch size 1 only."
        self.reset_streaming_cache()
        n = int(audio_lens.item())
        plan = self._utterance_chunks(n, chunk_size_ms)
        if plan is None:
            print(f"Error: Input audio too short ({n} frames) for conv layers. Skipping.")
            return [[] for _ in range(audios.size(0))], None, None
        full = []
        for s, e, off in plan:
            full.extend(self._decode_chunk_streaming_logic(audios[:, s:e, :], off, off))
        return [full], None, None

    # ---- beam search (model/online_rnnt_model.py:389-645) -------------------------------------------
    def _decode_chunk_beam_search(self, chunk_xs: torch.Tensor, offset: int, required_cache_size: int,
                                  beam_hypotheses_in: Optional[List[BeamHypothesis]], beam_size: int = 4) -> List[BeamHypothesis]:
        x = chunk_xs.to(self.device, torch.float32).contiguous()
        s = _stream_ptr()
        tq = self._engine.encoder_chunk(x.data_ptr(), x.size(1), offset, required_cache_size, s)
        # The hypotheses live in the library (one empty hypothesis with the zero LSTM state after a reset, :407-415); the
        # list handed back mirrors them, and `beam_hypotheses_in` is expected to be that list (as in the reference's callers).
        self._engine.beam_advance(0, tq, beam_size, s)
        beam = [BeamHypothesis(tokens=t, log_prob=lp) for t, lp in self._engine.beam_hyps(0)]
        h, c = self._engine.beam_states(len(beam), s)
        for i, hyp in enumerate(beam):
            hyp.predictor_states = [torch.from_numpy(h[i]).view(1, 1, 256).to(self.device),
                                    torch.from_numpy(c[i]).view(1, 1, 256).to(self.device)]
        self._engine.frames_discard(s)
        self._chunks_done += 1
        return beam

    def process_single_chunk_beam_search(self, chunk_audio: torch.Tensor, chunk_len: torch.Tensor,
                                         beam_size: int = 4) -> Tuple[List[BeamHypothesis], None, None]:
        assert self.streaming, "Model is not in streaming mode for process_single_chunk_beam_search."
        assert chunk_audio.size(0) == 1, "Single chunk beam search currently supports batch size 1 only."
        if self._chunks_done is None:
            self.reset_streaming_cache()
        if chunk_audio.size(1) < 7:
            print(f"Warning: Chunk too small ({chunk_audio.size(1)} frames), skipping")
            return self.streaming_beam_hypotheses or [], None, None
        off = self._global_encoder_offset
        self.streaming_beam_hypotheses = self._decode_chunk_beam_search(chunk_audio, off, off, self.streaming_beam_hypotheses, beam_size)
        self._global_encoder_offset += chunk_audio.size(1) // self.encoder.embed.subsampling_rate
        return self.streaming_beam_hypotheses, None, None

    def streaming_beam_search(self, audios: torch.Tensor, audio_lens: torch.Tensor, beam_size: int = 4,
                              chunk_size_ms: Optional[int] = None) -> Tuple[List[List[int]], None, None]:
        assert self.streaming, "Model is not in streaming mode for streaming_beam_search."
        assert audios.size(0) == 1, "Streaming beam search currently supports batch size 1 only."
        self.reset_streaming_cache()
        n = int(audio_lens.item())
        plan = self._utterance_chunks(n, chunk_size_ms)
        if plan is None:
            print(f"Error: Input audio too short ({n} frames) for conv layers. Skipping.")
            return [[] for _ in range(audios.size(0))], None, None
        for s, e, off in plan:
            self.streaming_beam_hypotheses = self._decode_chunk_beam_search(audios[:, s:e, :], off, off, self.streaming_beam_hypotheses, beam_size)
        if self.streaming_beam_hypotheses:
            return [max(self.streaming_beam_hypotheses, key=lambda h: h.log_prob).tokens], None, None     # :598-601
        return [[]], None, None

    # ---- CTC head (model/online_rnnt_model.py:647-671) ---------------------------------------------------
    def ctc_greedy_search(self, audios: torch.Tensor, audio_lens: torch.Tensor) -> List[List[int]]:
        """Greedy CTC decode on the same encoder.  Deviation, on purpose: the reference calls `self.encoder(x, lens)`,
        which in eval mode with use_dynamic_chunk draws a RANDOM chunk mask (wenet/utils/mask.py:170-183; SURVEY.md
        §0.8: two identical calls differ by 0.61); this uses the deterministic full-context encoder
        (decoding_chunk_size=-1).  Collapse rule as in :660-671: drop blanks and repeats over the valid frames.
        Invalidates the streaming state of this object (the full-context pass reuses the conv rings)."""
        if self.ctc_weight <= 0.0:
            return [[] for _ in range(audios.size(0))]
        self._require_loaded()
        B, T = audios.size(0), audios.size(1)
        x = audios.to(self.device, torch.float32).contiguous()
        lens = audio_lens.detach().cpu().numpy().astype(np.int32)
        ids = self._engine.ctc_argmax(x.data_ptr(), lens, B, T, _stream_ptr())
        self._chunks_done = None
        hyps = []
        for b in range(B):
            n1 = max(0, (min(int(lens[b]), T) - 1) // 2)          # valid frames after masks[:, :, 2::2][:, :, 2::2]
            n = max(0, (n1 - 1) // 2)
            hyp, prev = [], -1
            for t in range(n):
                tok = int(ids[b, t])
                if tok != self.blank_id and tok != prev:
                    hyp.append(tok)
                prev = tok
            hyps.append(hyp)
        return hyps

    # ---- teacher-forced scoring (model/online_rnnt_model.py:224-266 under torch.no_grad()) ----------------------------
    def _encode_for_scoring(self, audios, audio_lens, texts, text_lens):
        """Full-context encoder of a padded batch + the host arrays of a scoring call: (enc [B, T', 256] on the device, valid
        encoder frames [B], targets [B, Umax] int32, target lengths [B]).  Invalidates the streaming state."""
        self._require_loaded()
        B, T = audios.size(0), audios.size(1)
        x = audios.to(self.device, torch.float32).contiguous()
        lens = audio_lens.detach().cpu().numpy().astype(np.int32).reshape(B)
        tq = ((T - 3) // 2 + 1 - 3) // 2 + 1
        enc = torch.empty(B, tq, 256, device=self.device)
        self._engine.encoder_full(x.data_ptr(), lens, B, T, enc.data_ptr(), _stream_ptr())
        self._chunks_done = None
        n1 = np.maximum(0, (np.minimum(lens, T) - 1) // 2)         # valid frames after masks[:, :, 2::2][:, :, 2::2]
        enc_lens = np.maximum(0, (n1 - 1) // 2).astype(np.int32)
        tg = np.ascontiguousarray(texts.detach().cpu().numpy().astype(np.int32).reshape(B, -1) if texts.numel() else np.zeros((B, 0), np.int32))
        tl = text_lens.detach().cpu().numpy().astype(np.int32).reshape(B)
        return enc, enc_lens, tg, tl

    def transducer_nll(self, audios: torch.Tensor, audio_lens: torch.Tensor, texts: torch.Tensor, text_lens: torch.Tensor) -> torch.Tensor:
        """Per-utterance transducer negative log-likelihood, float64 [B]: torchaudio.functional.rnnt_loss(reduction="none") of
        the reference's lattice (:241-255), i.e. minus the log of the sum over all monotonic alignments, computed on the device
        (rnnt_transducer_nll) without materialising the [B, T, U+1, V] lattice.  texts [B, Umax] (entries beyond text_lens are
        ignored, the reference pads with ignore_id).  Deviation, on purpose: the reference's `self.encoder(x, lens)` draws a
        RANDOM chunk mask even in eval mode, so its loss is not reproducible; this runs the deterministic
        full-context encoder (rnnt_encoder_full, decoding_chunk_size=-1).  Invalidates the streaming state, as
        greedy_search_full does."""
        enc, enc_lens, tg, tl = self._encode_for_scoring(audios, audio_lens, texts, text_lens)
        nll = self._engine.transducer_nll(enc.data_ptr(), enc_lens, tg, tl, enc.size(0), enc.size(1), None, _stream_ptr())
        return torch.from_numpy(nll)

    def ctc_nll(self, audios: torch.Tensor, audio_lens: torch.Tensor, texts: torch.Tensor, text_lens: torch.Tensor) -> torch.Tensor:
        """Per-utterance CTC negative log-likelihood, float64 [B]: nn.CTCLoss(blank, reduction="none") on the CTC head's
        log-softmax (:22-32) over the same deterministic full-context encoder as transducer_nll (rnnt_ctc_nll); +inf where the
        frames cannot hold the transcript.  Invalidates the streaming state."""
        enc, enc_lens, tg, tl = self._encode_for_scoring(audios, audio_lens, texts, text_lens)
        nll = self._engine.ctc_nll(enc.data_ptr(), enc_lens, tg, tl, enc.size(0), enc.size(1), _stream_ptr())
        return torch.from_numpy(nll)

    FRAME_SECONDS = 0.04     # one encoder frame: 4x subsampling of 10 ms features, WeNet's frame_rate default

    def align(self, audios: torch.Tensor, audio_lens: torch.Tensor, texts: torch.Tensor, text_lens: torch.Tensor, method: str = "rnnt"):
        """Forced alignment of given transcripts over the deterministic full-context encoder (see transducer_nll): per utterance
        {"tokens", "frames", "times": [(start_s, end_s)], "log_prob"}.  method "rnnt": the best transducer path
        (rnnt_transducer_align), frames = the frame at which each token is emitted; "ctc": the best CTC path (rnnt_ctc_align, what
        WeNet's force_align asks of torchaudio), frames = its peaks (peaks_from_ctc_alignment).  times = timestamps_from_peaks
        with max_duration = the utterance's encoder frames * 0.04 s; log_prob is the best path's.  A transcript the CTC frames
        cannot hold has log_prob -inf and no frames.  Invalidates the streaming state."""
        assert method in ("rnnt", "ctc"), method
        enc, enc_lens, tg, tl = self._encode_for_scoring(audios, audio_lens, texts, text_lens)
        B, tq, s = enc.size(0), enc.size(1), _stream_ptr()
        if method == "rnnt":
            best, emit = self._engine.transducer_align(enc.data_ptr(), enc_lens, tg, tl, B, tq, stream=s)
        else:
            best, ali = self._engine.ctc_align(enc.data_ptr(), enc_lens, tg, tl, B, tq, s)
        out = []
        for b in range(B):
            if method == "rnnt":
                frames = emit[b, :tl[b]].tolist()
            else:
                frames = peaks_from_ctc_alignment(ali[b, :enc_lens[b]].tolist(), self.blank_id) if np.isfinite(best[b]) else []
            times = timestamps_from_peaks(frames, int(enc_lens[b]) * self.FRAME_SECONDS, self.FRAME_SECONDS)
            out.append({"tokens": tg[b, :tl[b]].tolist(), "frames": frames, "times": times, "log_prob": float(best[b])})
        return out

    def _has_ctc_head(self) -> bool:
        return bool(getattr(self, "_ctc_loaded", False))

    def forward(self, audios, audio_lens, texts=None, text_lens=None):
        """The reference's forward (model/online_rnnt_model.py:224-272).  Without texts: a streaming model goes to
        streaming_inference (:271-272); a non-streaming model runs the full-context encoder and basic_greedy_search
        (:234-235,268; model/component/transducer.py:22-70, n_steps=64) for the whole batch.
        With texts (the validation loop's call under torch.no_grad(), online_rnnt_train.py:184-200): returns
        (None, total_loss, loss_dict) with loss_rnnt = mean over the batch of transducer_nll (rnnt_loss reduction="mean"),
        total = (1 - ctc_weight) * loss_rnnt, and, when ctc_weight > 0 and the CTC head is loaded, loss_ctc =
        nn.CTCLoss(reduction="mean", zero_infinity=True) of ctc_nll and total += ctc_weight * loss_ctc (compose_losses).
        total_loss is a float64 tensor without a graph: this is scoring, not training.  The first element is None where the
        reference returns joint_out: the [B, T, U+1, V] lattice is never materialised (rnnt_joint gives it to whoever wants
        it).  The encoder is the deterministic full-context one (see transducer_nll)."""
        if texts is not None:
            enc, enc_lens, tg, tl = self._encode_for_scoring(audios, audio_lens, texts, text_lens)
            B, tq, s = enc.size(0), enc.size(1), _stream_ptr()
            nll_rnnt = self._engine.transducer_nll(enc.data_ptr(), enc_lens, tg, tl, B, tq, None, s)
            nll_ctc = None
            if self.ctc_weight > 0.0 and self._has_ctc_head():
                nll_ctc = self._engine.ctc_nll(enc.data_ptr(), enc_lens, tg, tl, B, tq, s)
            total, loss_dict = compose_losses(nll_rnnt, nll_ctc, tl, self.ctc_weight)
            return None, torch.tensor(total, dtype=torch.float64), loss_dict
        if self.streaming:
            return self.streaming_inference(audios, audio_lens)
        return self.greedy_search_full(audios, audio_lens), None, None

    def prefix_beam_search(self, audios: torch.Tensor, audio_lens: torch.Tensor, beam_size: int = 5, ctc_weight: float = 0.3,
                           transducer_weight: float = 0.7, context: Optional["ContextBias"] = None, ngram: Optional["NgramLM"] = None):
        """WeNet prefix beam search (wenet/transducer/search/prefix_beam_search.py:42-148) on the full-context encoder
        (decoding_chunk_size=-1), B = 1: at most one symbol per frame, CTC shallow fusion, prefix merging with log_add.
        Device: encoder (rnnt_encoder_full), CTC posteriors (rnnt_ctc_logprobs), one predictor step and one joint + log_softmax
        per frame for all hypotheses (rnnt_predictor_step, rnnt_joint).  Host: the fusion / top-k (float32, torch CPU ops as
        in the reference), candidate order, log_add merge (Python double, the LIST form the reference's call site was written
        for: its vendored log_add(*args) raises TypeError on a merge), stable sort, truncation.
        context: hot words, with the semantics of wenet/transformer/search.py:95-104,169-171,214-235 carried over (the reference's
        transducer search has none), in Python doubles on testing.context_graph_ref: every hypothesis holds a graph state and a
        context score beside its score ([blank]: root, 0); a blank candidate copies them, any other token takes one step and adds
        its score; merged candidates keep the first one's; the sort is by score + context score; after the last frame finalize
        replaces the context scores, without a re-sort.  The first prune (top-k) does not see the graph.
        Returns [(tokens incl. the leading blank, score)], best first; with a context the scores are the totals and
        self._prefix_context_scores holds [(running, finalized)] context scores per hypothesis.
        ngram: an NgramLM fused into the search (semantics: include/rnnt_hip.h, rnnt_prefix_beam_decode_ngram), in Python doubles on
        testing.ngram_ref: every hypothesis also holds an n-gram state and score ([blank]: the start marker, 0), copied and stepped
        where the context is; the sort is by score + context score + n-gram score, left to right, a term whose feature is off left
        out; after the last frame context finalize comes first, then every survivor's n-gram score gains the end term of its state,
        without a re-sort.  self._prefix_ngram_scores then holds [(running, final)] n-gram scores per hypothesis, and
        self._prefix_min_gap the smallest difference between adjacent totals at any frame's second prune, the pair across the beam
        boundary included (inf when no frame had two candidates)."""
        import math
        self._require_loaded()
        assert audios.size(0) == 1, "prefix_beam_search is batch-1 in the reference (:58)"
        eng, dev, V = self._engine, self.device, self.vocab_size
        x = audios.to(dev, torch.float32).contiguous()
        T = x.size(1)
        tq = ((T - 3) // 2 + 1 - 3) // 2 + 1
        s = _stream_ptr()
        enc = torch.empty(1, tq, 256, device=dev)
        eng.encoder_full(x.data_ptr(), np.asarray([int(audio_lens[0])], np.int32), 1, T, enc.data_ptr(), s)
        ctc_dev = torch.empty(tq, V, device=dev)
        eng.ctc_logprobs(enc.data_ptr(), tq, ctc_dev.data_ptr(), s)
        ctc = ctc_dev.cpu()
        hyps, scores = [[self.blank_id]], [0.0]
        graph = None
        if context is not None:
            from .testing import context_graph_ref
            graph = context_graph_ref(context.phrases, context.context_score)
        lm = None
        if ngram is not None:
            from .testing import ngram_ref
            lm = ngram_ref(ngram.ngrams, V, self.blank_id, ngram.lm_weight, ngram.length_bonus, ngram.unk_logp)
        from .testing import NG_START, ngram_eos_ref, ngram_step_ref, prefix_total_ref
        cstate, cscore = [0], [0.0]
        nstate, nscore = [NG_START], [0.0]
        min_gap = math.inf
        h = torch.zeros(1, 256, device=dev)
        c = torch.zeros(1, 256, device=dev)

        def log_add(args):
            if all(a == -float("inf") for a in args):
                return -float("inf")
            a_max = max(args)
            return a_max + math.log(sum(math.exp(a - a_max) for a in args))
        for i in range(tq):                                      # every encoder frame, padded ones included (maxlen = encoder_out.size(1), :64,76)
            n = len(hyps)
            tok = torch.tensor([hy[-1] for hy in hyps], dtype=torch.int32, device=dev)
            pred, h2, c2 = torch.empty(n, 256, device=dev), torch.empty(n, 256, device=dev), torch.empty(n, 256, device=dev)
            eng.predictor_step(tok.data_ptr(), h.data_ptr(), c.data_ptr(), n, pred.data_ptr(), h2.data_ptr(), c2.data_ptr(), s)
            lp_dev = torch.empty(1, 1, n, V, device=dev)
            eng.joint(enc[:, i:i + 1].contiguous().data_ptr(), pred.data_ptr(), 1, 1, n, 1, lp_dev.data_ptr(), s)
            logp = lp_dev.view(n, V).cpu()
            logp = torch.log(torch.add(transducer_weight * torch.exp(logp), ctc_weight * torch.exp(ctc[i].unsqueeze(0))))   # :99-101
            top_lp, top_ix = logp.topk(beam_size)                                                                            # :104
            sc = torch.add(torch.tensor(scores).unsqueeze(1), top_lp)                                                        # :105 (float32)
            cand = []                # [tokens, score, state row in cat(h, h2), context state, context score, n-gram state, n-gram score]
            for j in range(n):
                for t in range(beam_size):
                    if int(top_ix[j, t]) == self.blank_id:
                        cand.append([list(hyps[j]), sc[j, t].item(), j, cstate[j], cscore[j], nstate[j], nscore[j]])
                    else:
                        step, nxt = graph.step(cstate[j], int(top_ix[j, t])) if graph is not None else (0.0, 0)
                        lstep, lnxt = ngram_step_ref(lm, nstate[j], int(top_ix[j, t])) if lm is not None else (0.0, NG_START)
                        cand.append([list(hyps[j]) + [int(top_ix[j, t])], sc[j, t].item(), n + j, nxt, cscore[j] + step, lnxt, nscore[j] + lstep])
            fused = [cand[0]]
            for cnd in cand[1:]:
                for f in fused:
                    if cnd[0] == f[0]:
                        f[1] = log_add([f[1], cnd[1]])
                        break
                else:
                    fused.append(cnd)
            if lm is not None:
                fused.sort(key=lambda v: prefix_total_ref(v[1], v[4] if graph is not None else None, v[6]), reverse=True)
                tot = [prefix_total_ref(v[1], v[4] if graph is not None else None, v[6]) for v in fused[:beam_size + 1]]
                min_gap = min([min_gap] + [a - b for a, b in zip(tot, tot[1:])])
            elif graph is not None:
                fused.sort(key=lambda v: v[1] + v[4], reverse=True)
            else:
                fused.sort(key=lambda v: v[1], reverse=True)
            fused = fused[:beam_size]
            cstate, cscore = [f[3] for f in fused], [f[4] for f in fused]
            nstate, nscore = [f[5] for f in fused], [f[6] for f in fused]
            rows = torch.tensor([f[2] for f in fused], device=dev)
            h = torch.cat([h, h2], 0).index_select(0, rows).contiguous()
            c = torch.cat([c, c2], 0).index_select(0, rows).contiguous()
            hyps, scores = [f[0] for f in fused], [f[1] for f in fused]
        self._prefix_states = (h, c)
        if graph is not None:
            fin = [graph.finalize(st) for st in cstate]
            self._prefix_context_scores = list(zip(cscore, fin))
            scores = [sc + f for sc, f in zip(scores, fin)]
        if lm is not None:
            fin = [ns + ngram_eos_ref(lm, st) for st, ns in zip(nstate, nscore)]
            self._prefix_ngram_scores = list(zip(nscore, fin))
            self._prefix_min_gap = min_gap
            scores = [sc + f for sc, f in zip(scores, fin)]
        return list(zip(hyps, scores))

    def prefix_beam_search_batch(self, audios: torch.Tensor, audio_lens: torch.Tensor, beam_size: int = 5, ctc_weight: float = 0.3,
                                 transducer_weight: float = 0.7, walk_padding: bool = True, context: Optional["ContextBias"] = None,
                                 with_context_scores: bool = False, ngram: Optional["NgramLM"] = None, with_ngram_scores: bool = False):
        """prefix_beam_search for a padded batch audios [B, T, 80] of utterances of different lengths, with the frame loop on the
        device: one rnnt_encoder_full call and one rnnt_prefix_beam_decode call (two launches per encoder frame, one
        synchronisation at the end).  walk_padding: every utterance walks all T' encoder frames, the padded ones included, as the
        reference does (:64,76) and prefix_beam_search above; False: each stops after its own valid frames.  Equal values in the
        top-k are taken lower index first (torch.topk leaves that order open).
        context: a ContextBias whose phrases boost the hypotheses that match them (rnnt_prefix_beam_decode_ctx; semantics as in
        prefix_beam_search): the scores are then the totals, which carry finalize's correction and need not descend;
        with_context_scores: every hypothesis is (tokens, score, context score), so score - context score is the unbiased score.
        ngram: an NgramLM fused into the search (rnnt_prefix_beam_decode_ngram; semantics as in prefix_beam_search): the scores are
        the totals, end term included, and need not descend; with_ngram_scores: every hypothesis ends with its n-gram score.
        Returns one [(tokens incl. the leading blank, score)] per utterance, best first; the hypotheses' final LSTM states stay in
        self._prefix_states_batch, one (h, c) pair of host tensors [n_hyp, 256] per utterance.  Invalidates the streaming state."""
        self._require_loaded()
        B, T = audios.size(0), audios.size(1)
        x = audios.to(self.device, torch.float32).contiguous()
        lens = audio_lens.detach().cpu().numpy().astype(np.int32).reshape(B)
        tq = ((T - 3) // 2 + 1 - 3) // 2 + 1
        s = _stream_ptr()
        enc = torch.empty(B, tq, 256, device=self.device)
        self._engine.encoder_full(x.data_ptr(), lens, B, T, enc.data_ptr(), s)
        self._chunks_done = None
        if walk_padding:
            enc_lens = np.full(B, tq, np.int32)
        else:
            n1 = np.maximum(0, (np.minimum(lens, T) - 1) // 2)     # valid frames after masks[:, :, 2::2][:, :, 2::2]
            enc_lens = np.maximum(0, (n1 - 1) // 2).astype(np.int32)
        if ngram is not None or with_ngram_scores:
            if context is not None:
                self._set_context(context)
            if ngram is not None:
                self._set_ngram(ngram)
            hyps, h, c = self._engine.prefix_beam_decode_ngram(enc.data_ptr(), enc_lens, B, tq, beam_size, ctc_weight, transducer_weight, context is not None,
                                                               ngram is not None, True, s)
            hyps = [[(tok, score) + ((cs,) if with_context_scores else ()) + ((ns,) if with_ngram_scores else ()) for tok, score, cs, ns in row]
                    for row in hyps]
        elif context is None and not with_context_scores:
            hyps, h, c = self._engine.prefix_beam_decode(enc.data_ptr(), enc_lens, B, tq, beam_size, ctc_weight, transducer_weight, True, s)
        else:
            if context is not None:
                self._set_context(context)
            hyps, h, c = self._engine.prefix_beam_decode_ctx(enc.data_ptr(), enc_lens, B, tq, beam_size, ctc_weight, transducer_weight, context is not None,
                                                             True, s)
            if not with_context_scores:
                hyps = [[(tok, score) for tok, score, _ in row] for row in hyps]
        self._prefix_states_batch = [(torch.from_numpy(h[b, :len(hyps[b])].copy()), torch.from_numpy(c[b, :len(hyps[b])].copy())) for b in range(B)]
        return hyps

    def _set_context(self, context: Optional["ContextBias"]):
        if context is not self._context_bias:                       # the graph lives in the context until another one replaces it
            self._engine.context_set(context.phrases if context is not None else [], context.context_score if context is not None else 0.0)
            self._context_bias = context

    def _set_ngram(self, ngram: "NgramLM"):
        if ngram is not self._ngram_lm:                             # the model lives in the context until another one replaces it
            self._engine.ngram_set(ngram)
            self._ngram_lm = ngram

    def ctc_prefix_beam_search(self, audios: torch.Tensor, audio_lens: torch.Tensor, beam_size: int = 10, context: Optional["ContextBias"] = None,
                               ngram: Optional["NgramLM"] = None):
        """WeNet's ctc_prefix_beam_search (wenet/transformer/search.py:125-247) on the CTC head over the deterministic full-context
        encoder, for a padded batch audios [B, T, 80]: one rnnt_encoder_full call and one rnnt_ctc_prefix_beam_decode call (the CTC
        log-probabilities, then ONE launch that walks every utterance's own valid frames).  context: a ContextBias whose phrases
        boost the hypotheses that match them (wenet/utils/context_graph.py); None: no biasing.  Equal values of a frame are taken
        lower index first (torch.topk leaves that order open).
        Returns per utterance [(tokens, score, times)] in the reference's order (nbest, nbest_scores, nbest_times): best first by
        score + running context score; with a context the returned scores carry finalize's correction and need not descend.
        ngram: an NgramLM fused into the search (rnnt_ctc_prefix_beam_decode_ngram): the second prune sees score + context score +
        n-gram score, the end term is added after the last frame, and the rows come back stably sorted by that final score,
        descending.  Invalidates the streaming state."""
        self._require_loaded()
        B, T = audios.size(0), audios.size(1)
        x = audios.to(self.device, torch.float32).contiguous()
        lens = audio_lens.detach().cpu().numpy().astype(np.int32).reshape(B)
        tq = ((T - 3) // 2 + 1 - 3) // 2 + 1
        s = _stream_ptr()
        enc = torch.empty(B, tq, 256, device=self.device)
        self._engine.encoder_full(x.data_ptr(), lens, B, T, enc.data_ptr(), s)
        self._chunks_done = None
        n1 = np.maximum(0, (np.minimum(lens, T) - 1) // 2)         # valid frames after masks[:, :, 2::2][:, :, 2::2]
        enc_lens = np.maximum(0, (n1 - 1) // 2).astype(np.int32)
        self._set_context(context)
        if ngram is not None:
            self._set_ngram(ngram)
            hyps = self._engine.ctc_prefix_beam_decode_ngram(enc.data_ptr(), enc_lens, B, tq, beam_size, context is not None, True, False, s)
            return [sorted(((h[0], h[1], h[2]) for h in row), key=lambda h: h[1], reverse=True) for row in hyps]
        hyps = self._engine.ctc_prefix_beam_decode(enc.data_ptr(), enc_lens, B, tq, beam_size, context is not None, False, s)
        return [[(tok, score, times) for tok, score, times, _ in row] for row in hyps]

    # ---- two-pass decoding (wenet/transducer/transducer.py:261-395) -------------------------------------------------
    def rescoring_batch(self, audios: torch.Tensor, audio_lens: torch.Tensor, beam_size: int = 10, ctc_weight: float = 0.3,
                        transducer_weight: float = 0.7, beam_search_type: str = "ctc", context: Optional["ContextBias"] = None,
                        search_ctc_weight: float = 1.0, search_transducer_weight: float = 0.0, ngram: Optional["NgramLM"] = None):
        """Transducer rescoring of n-best for a padded batch audios [B, T, 80]: one full-context encoder call, one search call
        (beam_search_type "ctc": rnnt_ctc_prefix_beam_decode, biased by `context` when given; "transducer":
        rnnt_prefix_beam_decode with the two search weights over each utterance's valid frames, the leading blank dropped, :327;
        with `context` rnnt_prefix_beam_decode_ctx, whose totals are the first-pass scores, as for "ctc"),
        one rnnt_transducer_nll_nbest call over the same frames and, per utterance, the choice of rnnt_rescore_select_host:
        total = first_score * ctc_weight + td_score * transducer_weight (:388-390 with attn_weight = 0; the defaults are the
        fusion weights of the reference's beam_search, :223-224).  beam_size <= 16.
        Returns per utterance (best_index, [(tokens, first_score, td_score, total)]) in the first pass's order; an utterance with
        no valid encoder frame comes back with td_score = nan and best_index = 0.  Invalidates the streaming state.
        ngram (beam_search_type "ctc" only): the first pass fuses that NgramLM; its totals are the first-pass scores."""
        check_rescoring_args(beam_search_type=beam_search_type)
        if ngram is not None and beam_search_type != "ctc":
            raise ValueError(f"ngram fuses into the CTC prefix search only, not beam_search_type={beam_search_type!r}")
        enc, enc_lens, _, _ = self._encode_for_scoring(audios, audio_lens, torch.zeros(audios.size(0), 0), torch.zeros(audios.size(0)))
        B, tq, s = enc.size(0), enc.size(1), _stream_ptr()
        if beam_search_type == "ctc" and ngram is not None:
            self._set_context(context)
            self._set_ngram(ngram)
            first = [[(h[0], h[1]) for h in row]
                     for row in self._engine.ctc_prefix_beam_decode_ngram(enc.data_ptr(), enc_lens, B, tq, beam_size, context is not None, True, False, s)]
        elif beam_search_type == "ctc":
            self._set_context(context)
            first = [[(tok, score) for tok, score, _, _ in row]
                     for row in self._engine.ctc_prefix_beam_decode(enc.data_ptr(), enc_lens, B, tq, beam_size, context is not None, False, s)]
        elif context is not None:
            self._set_context(context)
            rows = self._engine.prefix_beam_decode_ctx(enc.data_ptr(), enc_lens, B, tq, beam_size, search_ctc_weight, search_transducer_weight, True, False, s)
            first = [[(tok[1:], score) for tok, score, _ in row] for row in rows]
        else:
            rows = self._engine.prefix_beam_decode(enc.data_ptr(), enc_lens, B, tq, beam_size, search_ctc_weight, search_transducer_weight, False, s)
            first = [[(tok[1:], score) for tok, score in row] for row in rows]
        valid = [b for b in range(enc.size(0)) if enc_lens[b] >= 1 and first[b]]
        nll = {}
        if valid:
            sub = enc if len(valid) == enc.size(0) else enc.index_select(0, torch.tensor(valid, device=enc.device)).contiguous()
            nh, hl, ht = pack_nbest([[t for t, _ in first[b]] for b in valid])
            out = self._engine.transducer_nll_nbest(sub.data_ptr(), enc_lens[valid], nh, hl, ht, len(valid), sub.size(1), None, _stream_ptr())
            nll = {b: out[i, :nh[i]] for i, b in enumerate(valid)}
        return [select_rescored([t for t, _ in row], [f for _, f in row], nll.get(b), ctc_weight, transducer_weight) for b, row in enumerate(first)]

    def transducer_attention_rescoring(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int, decoding_chunk_size: int = -1,
                                       num_decoding_left_chunks: int = -1, simulate_streaming: bool = False, reverse_weight: float = 0.0,
                                       ctc_weight: float = 0.0, attn_weight: float = 0.0, transducer_weight: float = 0.0,
                                       search_ctc_weight: float = 1.0, search_transducer_weight: float = 0.0,
                                       beam_search_type: str = "transducer"):
        """Transducer.transducer_attention_rescoring (wenet/transducer/transducer.py:261-395), B = 1, same signature and return value
        (tokens, score): n-best from the first pass -- "transducer": the prefix beam search with the two search weights, "ctc": the
        CTC prefix beam search -- every hypothesis re-scored with the full transducer likelihood over the same frames, the best of
        first_score * ctc_weight + td_score * transducer_weight.  This model has no attention decoder: attn_weight and
        reverse_weight must be 0; the encoder is the full-context one (decoding_chunk_size -1), num_decoding_left_chunks and
        simulate_streaming have nothing to act on.  The reference's `assert len(hyps) == beam_size` is not kept: a short
        utterance may yield fewer.  score is -inf when no total compares greater (:372), e.g. no valid frame."""
        check_rescoring_args(attn_weight, reverse_weight, decoding_chunk_size, beam_search_type)
        assert speech.shape[0] == speech_lengths.shape[0] == 1, "transducer_attention_rescoring is batch-1 in the reference (:313)"
        best, rows = self.rescoring_batch(speech, speech_lengths, beam_size, ctc_weight, transducer_weight, beam_search_type, None,
                                          search_ctc_weight, search_transducer_weight)[0]
        total = rows[best][3]
        return rows[best][0], (total if total > -float("inf") else -float("inf"))

    def greedy_search_full(self, audios, audio_lens, n_steps: int = 64):
        """basic_greedy_search over the deterministic full-context encoder; audios [B,T,80] with B <= max_streams,
        T <= max_chunk_frames, ((T-3)//2+1-3)//2+1 <= max_enc_frames.  Invalidates the streaming state."""
        self._require_loaded()
        B, T = audios.size(0), audios.size(1)
        x = audios.to(self.device, torch.float32).contiguous()
        lens = audio_lens.detach().cpu().numpy().astype(np.int32)
        hyps = self._engine.greedy_search_full(x.data_ptr(), lens, B, T, n_steps, _stream_ptr())
        self._chunks_done = None
        return hyps

    __call__ = forward


class StreamingBatch:
    """B independent streams advanced in lock step through one context (not in the reference, which
    is B=1): the chunk loop of online_rnnt_decode.py:81-117 / streaming_inference for a whole batch."""

    def __init__(self, state_dict, n_streams: int, vocab_size: int = 412, blank_id: int = 5, max_chunk_frames: int = 64,
                 max_cache_frames: int = 512, max_enc_frames: int = 512, max_tokens: int = 4096, device: int = 0, max_beam: int = 0,
                 numerics=None, packed=None):
        """state_dict: the reference's 504-key dict (numpy / torch values), or None with packed=(blob, vocab): the flat float32
        blob dist.broadcast_packed left on this rank's device, handed to the context in one call (RnntEngine.load_packed)."""
        self.device = torch.device("cuda", device)
        self.n = n_streams
        self.blank_id = blank_id
        self.engine = RnntEngine(max_streams=n_streams, max_chunk_frames=max_chunk_frames, max_cache_frames=max_cache_frames,
                                 max_enc_frames=max_enc_frames, max_tokens=max_tokens, vocab_size=vocab_size, blank_id=blank_id,
                                 n_steps=10, device=device, max_beam=max_beam)
        self.beams = None
        self.python_beam = False      # True: host half of the beam search in Python (beam_advance_frame), for tests
        if packed is not None:
            assert state_dict is None and int(packed[1]) == vocab_size, "packed=(blob, vocab): vocab must equal vocab_size"
            self.engine.load_packed(packed[0], int(packed[1]), numerics=numerics)
        else:
            self.engine.load_state_dict(state_dict, numerics=numerics)
        self.offset = 0

    def reset(self):
        self.engine.reset(self.n, _stream_ptr())
        self.offset = 0
        self.beams = None

    def _beam_frames(self, frames, beam_size, s, device_merge):
        """The beam recursion over buffered frames [0, frames) of every stream (frames: int, or one end per stream).
        device_merge: rnnt_beam_decode (frame loop on the device); a refusal (outside its supported range) falls back to
        rnnt_beam_advance when every stream has the same frames and returns False otherwise.  Returns True when done."""
        uniform = isinstance(frames, int)
        if device_merge:
            try:
                self.engine.beam_decode(0, None if uniform else [int(f) for f in frames], beam_size, s)
                return True
            except RnntError as e:
                if e.status not in (ERR_ARG, ERR_STATE):
                    raise
        if not uniform:
            return False
        self.engine.beam_advance(0, frames, beam_size, s)
        return True

    def process_chunk_beam(self, chunks: torch.Tensor, beam_size: int = 4, device_merge: bool = False):
        """process_single_chunk_beam_search semantics for every stream (online_rnnt_model.py:605-645)."""
        assert chunks.size(0) == self.n and chunks.is_cuda and chunks.dtype == torch.float32 and chunks.is_contiguous()
        if chunks.size(1) < 7:
            return self.beams
        s = _stream_ptr()
        tq = self.engine.encoder_chunk(chunks.data_ptr(), chunks.size(1), self.offset, self.offset, s)
        self.offset += chunks.size(1) // 4
        if self.python_beam:                                   # reference implementation of the host half (tests)
            if self.beams is None:
                self.beams = [[BeamHypothesis([], 0.0)] for _ in range(self.n)]
            for t in range(tq):
                self.beams = beam_advance_frame(self.engine, t, self.beams, self.blank_id, beam_size, s)
        else:                                                  # bookkeeping inside the library (rnnt_beam_advance / rnnt_beam_decode)
            self._beam_frames(tq, beam_size, s, device_merge)
            self.beams = self._native_beams()
        self.engine.frames_discard(s)
        return self.beams

    def _native_beams(self):
        return [[BeamHypothesis(t, lp) for t, lp in self.engine.beam_hyps(b)] for b in range(self.n)]

    def beam_script(self, audios: torch.Tensor, chunk_frames: int, beam_size: int = 4, pipelined: bool = False,
                    device_merge: bool = False):
        """Beam loop of online_rnnt_decode.py:123-178 over [B,T,80]; returns the final beams per stream.
        pipelined=True: the whole utterance's encoder in one rnnt_encoder_chunks call, then ONE rnnt_beam_advance over
        all frames (same hypotheses: the beam recursion only consumes encoder frames in order); needs
        max_enc_frames >= the utterance's encoder frames.
        device_merge=True: rnnt_beam_decode instead of rnnt_beam_advance (the frame loop on the device; bitwise the same
        hypotheses), rnnt_beam_advance where it refuses."""
        from .layout import chunk_plan
        self.reset()
        if pipelined and not self.python_beam:
            assert audios.is_cuda and audios.dtype == torch.float32 and audios.is_contiguous()
            plan = [(a, b) for a, b in chunk_plan(audios.size(1), chunk_frames) if b - a >= 7]
            offs, o = [], 0
            for a, b in plan:
                offs.append(o)
                o += (b - a) // 4
            s = _stream_ptr()
            frames = self.engine.encoder_chunks(audios.data_ptr(), audios.size(1), [a for a, _ in plan], [b - a for a, b in plan], offs, offs, s, greedy=False)
            self.offset = o
            self._beam_frames(frames, beam_size, s, device_merge)
            self.beams = self._native_beams()
            self.engine.frames_discard(s)
            return self.beams
        for (a, b) in chunk_plan(audios.size(1), chunk_frames):
            self.process_chunk_beam(audios[:, a:b, :].contiguous(), beam_size, device_merge)
        return self.beams

    def beam_script_ragged(self, audios: torch.Tensor, audio_lens, chunk_frames: int, beam_size: int = 4) -> List[List[BeamHypothesis]]:
        """Beam loop of online_rnnt_decode.py:123-178 for a PADDED batch of utterances of different lengths (utils/utils.py:29-50;
        online_rnnt_eval.py:86-94): stream b is beam-decoded over its own audio_lens[b] frames with its own chunk plan (tail-merge
        rule, < 7-frame skip), so its final beam equals a B = 1 beam_script(pipelined=True) run of that utterance.  Utterances of at
        least two chunks go through ONE rnnt_encode_ragged call and ONE rnnt_beam_decode call (per-stream frame ends); single-chunk
        utterances, and everything when the ragged call refuses, run as LENGTH CLASSES (one beam_script(pipelined=True,
        device_merge=True) per length).  An utterance shorter than 7 frames gives an empty beam (online_rnnt_model.py:615-618)."""
        assert audios.is_cuda and audios.dtype == torch.float32 and audios.size(0) == self.n
        lens = [int(v) for v in (audio_lens.tolist() if hasattr(audio_lens, "tolist") else audio_lens)]
        assert len(lens) == self.n and max(lens) <= audios.size(1) and min(lens) >= 0
        out: List[Optional[List[BeamHypothesis]]] = [None] * self.n
        two_chunks = chunk_frames + max(16, chunk_frames)
        done = set()
        if audios.is_contiguous() and not self.python_beam:
            ragged = [b for b in range(self.n) if lens[b] >= two_chunks or lens[b] < 7]
            big = [lens[b] for b in ragged if lens[b] >= two_chunks]
            if big and max(big) >= 2 * chunk_frames + max(16, chunk_frames):    # the longest one has at least three chunks
                self.reset()
                rset = set(ragged)
                call_lens = [lens[b] if b in rset else 0 for b in range(self.n)]
                s = _stream_ptr()
                frames = self.engine.encode_ragged(audios.data_ptr(), audios.size(1), call_lens, chunk_frames, s)
                if self._beam_frames(frames.tolist(), beam_size, s, True):
                    beams = self._native_beams()
                    for b in ragged:
                        out[b] = beams[b] if lens[b] >= 7 else []
                    done = rset
                self.engine.frames_discard(s)
                self.beams = None
        n_all = self.n
        try:
            for T_ in sorted({lens[b] for b in range(n_all) if b not in done}, reverse=True):
                idx = [b for b in range(n_all) if lens[b] == T_ and b not in done]
                if T_ < 7:                                   # shorter than the conv front-end's receptive field: skipped (:615-618)
                    for b in idx:
                        out[b] = []
                    continue
                sub = audios[torch.tensor(idx, device=audios.device), :T_, :].contiguous()
                self.n = len(idx)
                beams = self.beam_script(sub, chunk_frames, beam_size, pipelined=True, device_merge=True)
                for b, bm in zip(idx, beams):
                    out[b] = bm
        finally:
            self.n = n_all
        return out

    def process_chunk(self, chunks: torch.Tensor, decode: bool = True):
        """chunks [B,T,80] on the device; process_single_chunk semantics for every stream."""
        assert chunks.size(0) == self.n and chunks.is_cuda and chunks.dtype == torch.float32 and chunks.is_contiguous()
        if chunks.size(1) < 7:
            return None
        s = _stream_ptr()
        self.engine.encoder_chunk(chunks.data_ptr(), chunks.size(1), self.offset, self.offset, s)
        self.offset += chunks.size(1) // 4
        if decode:
            self.engine.greedy_decode(s)
            self.engine.frames_consume(s)

    def decode_script_ragged(self, audios: torch.Tensor, audio_lens, chunk_frames: int, pipelined: bool = True) -> List[List[int]]:
        """Greedy loop of online_rnnt_decode.py:81-117 for a PADDED batch of utterances of different lengths (utils/utils.py:29-50
        pads them; online_rnnt_eval.py:86-94 decodes each with its own audio_lens): stream b is decoded over its own
        audio_lens[b] frames with its own chunk plan (tail-merge rule, < 7-frame skip), so its tokens equal its B = 1 result.
        pipelined=True: ONE library call (rnnt_decode_ragged: per-stream chunk plans inside the layer-major launches) for every
        utterance of at least two chunks; utterances that are a single chunk (< chunk_frames + max(16, chunk_frames) frames) and the
        per-chunk form (pipelined=False) run as LENGTH CLASSES: streams of equal length share one whole-utterance call."""
        assert audios.is_cuda and audios.dtype == torch.float32 and audios.size(0) == self.n
        lens = [int(v) for v in (audio_lens.tolist() if hasattr(audio_lens, "tolist") else audio_lens)]
        assert len(lens) == self.n and max(lens) <= audios.size(1) and min(lens) >= 0
        out: List[Optional[List[int]]] = [None] * self.n
        two_chunks = chunk_frames + max(16, chunk_frames)
        done = set()
        if pipelined and audios.is_contiguous():
            ragged = [b for b in range(self.n) if lens[b] >= two_chunks or lens[b] < 7]
            big = [lens[b] for b in ragged if lens[b] >= two_chunks]
            if big and max(big) >= 2 * chunk_frames + max(16, chunk_frames):    # the longest one has at least three chunks
                self.reset()
                call_lens = [lens[b] if b in set(ragged) else 0 for b in range(self.n)]
                s = _stream_ptr()
                self.engine.decode_ragged(audios.data_ptr(), audios.size(1), call_lens, chunk_frames, s)
                toks = self.engine.tokens(s)
                for b in ragged:
                    out[b] = toks[b]
                done = set(ragged)
        n_all = self.n
        try:
            for T_ in sorted({lens[b] for b in range(n_all) if b not in done}, reverse=True):
                idx = [b for b in range(n_all) if lens[b] == T_ and b not in done]
                if T_ < 7:                                   # shorter than the conv front-end's receptive field: skipped (:356-359)
                    for b in idx:
                        out[b] = []
                    continue
                sub = audios[torch.tensor(idx, device=audios.device), :T_, :].contiguous()
                self.n = len(idx)
                toks = self.decode_script(sub, chunk_frames, per_chunk_decode=not pipelined, pipelined=pipelined)
                for b, t in zip(idx, toks):
                    out[b] = t
        finally:
            self.n = n_all
        return out

    def decode_script(self, audios: torch.Tensor, chunk_frames: int, per_chunk_decode: bool = True, pipelined: bool = False) -> List[List[int]]:
        """Greedy loop of online_rnnt_decode.py:81-117 over [B,T,80] equal-length utterances.
        per_chunk_decode=False runs the encoder over all chunks first and decodes once at the end
        (identical tokens: the greedy state machine is causal in the frame index).
        pipelined=True hands the whole chunk plan to rnnt_encoder_chunks (wavefront over chunk x layer,
        bit-identical encoder output) and decodes once."""
        from .layout import chunk_plan
        self.reset()
        T = audios.size(1)
        if pipelined:
            assert audios.is_cuda and audios.dtype == torch.float32 and audios.is_contiguous()
            plan = chunk_plan(T, chunk_frames)
            starts = [a for a, b in plan if b - a >= 7]
            lens = [b - a for a, b in plan if b - a >= 7]
            offs, o = [], 0
            for a, b in plan:                      # process_single_chunk: offset += frames // 4 (online_rnnt_model.py:384-385)
                if b - a >= 7:
                    offs.append(o)
                    o += (b - a) // 4
            s = _stream_ptr()
            self.engine.encoder_chunks(audios.data_ptr(), T, starts, lens, offs, offs, s, greedy=True)
            self.offset = o
            self.engine.frames_consume(s)
            return self.engine.tokens(s)
        for (a, b) in chunk_plan(T, chunk_frames):
            self.process_chunk(audios[:, a:b, :].contiguous(), decode=per_chunk_decode)
        if not per_chunk_decode:
            s = _stream_ptr()
            self.engine.greedy_decode(s)
            self.engine.frames_consume(s)
        return self.engine.tokens(_stream_ptr())


_PLAN_ORDER = ("greedy", "beam", "ctc_prefix", "prefix", "ctc_prefix_ngram", "prefix_ngram")   # the classes of a round run in this order of kinds


class Decoder(namedtuple("Decoder", ["kind", "beam", "use_context", "weights", "use_ngram"])):
    """The decoder a pool slot was opened with, fixed for its utterance: kind ("greedy", "beam", "ctc_prefix" or "prefix", a row of
    _KINDS), beam size (0 for greedy), hot-word biasing, the (ctc_weight, transducer_weight) of a "prefix" slot (None otherwise) and
    n-gram fusion (a "ctc_prefix" or "prefix" slot's).  Slots with equal decoders may share a library call."""
    __slots__ = ()

    @property
    def plan_kind(self):
        """the kind as pool_plan names it: the CTC prefix and transducer prefix slots that fuse a model are kinds of their own, ordered last"""
        return self.kind + "_ngram" if self.use_ngram else self.kind

    @property
    def plan_key(self):
        return (_PLAN_ORDER.index(self.plan_kind), self.beam, int(self.use_context)) + (self.weights or (0.0, 0.0))


GREEDY = Decoder("greedy", 0, False, None, False)

# one library call of a step: one chunk length, one decoder, every slot at most once
Call = namedtuple("Call", ["length", "slots", "offsets", "decoder"])


def plan_calls(queue, offsets, decoders):
    """The library calls of one StreamPool.step as a pure function (no GPU, no tensors): pool_plan's rounds, < 7-frame skip, offset
    bookkeeping and index, with decoders = {slot: Decoder} (an absent slot is greedy) in place of its four tables.  Returns (calls,
    new_offsets, index), every call one Call; inside a round the classes run in ascending (length, Decoder.plan_key)."""
    offs = dict(offsets)
    rounds: List[Dict[Tuple[int, Decoder], List[Tuple[int, int]]]] = []   # round -> (length, decoder) -> [(slot, queue index)]
    depth: Dict[int, int] = {}
    index: List[Optional[Tuple[int, int]]] = [None] * len(queue)
    for k, (slot, length) in enumerate(queue):
        if length < 7:
            continue
        r = depth.get(slot, 0)
        depth[slot] = r + 1
        while len(rounds) <= r:
            rounds.append({})
        rounds[r].setdefault((int(length), decoders.get(slot, GREEDY)), []).append((slot, k))
    calls = []
    for rnd in rounds:
        for length, decoder in sorted(rnd, key=lambda c: (c[0], c[1].plan_key)):
            slots, call_offs = [], []
            for slot, k in rnd[(length, decoder)]:
                index[k] = (len(calls), len(slots))
                slots.append(slot)
                call_offs.append(offs.get(slot, 0))
                offs[slot] = offs.get(slot, 0) + length // 4
            calls.append(Call(length, slots, call_offs, decoder))
    return calls, offs, index


def pool_plan(queue, offsets, beams=None, ctc_prefix=None, prefix=None, ngram=None):
    """The library calls of one StreamPool.step as a pure function (no GPU, no tensors).

    queue: [(slot, length)] in feed order, several entries per slot allowed; offsets: {slot: encoder offset so far}.
    Returns (calls, new_offsets, index): calls = [(length, [slot, ...], [offset, ...])], one rnnt_pool_chunk each, and index[k] =
    (call, row) of queue entry k (None for a skipped one).  A call holds ONE chunk length and every slot at most once; a slot's
    chunks keep their feed order across calls (its r-th queued chunk goes into round r, rounds run one after the other, and
    inside a round the length classes run in ascending length).  Per slot the bookkeeping is process_single_chunk's
    (model/online_rnnt_model.py:356-359,364-370,384-385): a chunk shorter than 7 frames is skipped without touching the offset, a
    chunk is encoded with offset = required_cache_size = the slot's offset so far, and the offset then grows by length // 4.

    beams: {slot: beam size} (0 or absent = greedy), None = all greedy and the result above.  With it every call is
    (length, slots, offsets, beam_size): one chunk length AND one beam size per call -- beam_size 0 is an rnnt_pool_chunk call,
    beam_size > 0 an rnnt_pool_chunk_beam call -- so greedy and beam slots never share a call; inside a round the classes run in
    ascending (length, beam size).  Feed order per slot and the round structure are the same.

    ctc_prefix: {slot: (beam size, use_context)} of the slots whose utterance runs the CTC prefix beam search, None = no such slot and
    the results above.  With it (an empty dict included) every call is (length, slots, offsets, beam_size, kind, use_context), kind
    one of "greedy" / "beam" / "ctc_prefix" -- an rnnt_pool_chunk, rnnt_pool_chunk_beam or rnnt_pool_chunk_ctc_prefix call -- with one
    (length, kind, beam size, use_context) class per call; inside a round the classes run in ascending (length, kind in that order,
    beam size, use_context).  A slot listed in ctc_prefix is not looked up in beams.

    prefix: {slot: (beam size, ctc_weight, transducer_weight)} of the slots whose utterance runs the transducer prefix beam search, None
    = no such slot and the results above.  With it (an empty dict included) every call is (length, slots, offsets, beam_size, kind,
    use_context, weights): kind "prefix" is an rnnt_pool_chunk_prefix call with weights = (ctc_weight, transducer_weight), every other
    kind is as above with weights None.  One (length, kind, beam size, use_context, weights) class per call -- slots with different
    weights never share one -- in ascending order inside a round.  A slot listed in prefix is looked up in neither ctc_prefix nor beams.
    A fourth element of a prefix entry is its use_context (hot-word biasing, an rnnt_pool_chunk_prefix_ctx call): biased and unbiased
    prefix slots of one length go in two calls.  A fifth element is its use_ngram (n-gram fusion, an rnnt_pool_chunk_prefix_ngram
    call): such calls have kind "prefix_ngram", ordered after "ctc_prefix_ngram", and never share a call with the other prefix slots.

    ngram: the slots among ctc_prefix whose search fuses the n-gram model (None or empty: none, and the results above).  Their calls
    have kind "ctc_prefix_ngram" (an rnnt_pool_chunk_ctc_prefix_ngram call), ordered after "prefix": such slots never share a call
    with the other CTC prefix slots."""
    decoders = {}
    for slot in {slot for slot, _ in queue}:
        if prefix is not None and slot in prefix:
            p = prefix[slot]
            decoders[slot] = Decoder("prefix", int(p[0]), bool(p[3]) if len(p) > 3 else False, (float(p[1]), float(p[2])),
                                     bool(p[4]) if len(p) > 4 else False)
        elif ctc_prefix is not None and slot in ctc_prefix:
            decoders[slot] = Decoder("ctc_prefix", int(ctc_prefix[slot][0]), bool(ctc_prefix[slot][1]), None, bool(ngram) and slot in ngram)
        elif beams and slot in beams:
            decoders[slot] = Decoder("beam" if int(beams[slot]) > 0 else "greedy", int(beams[slot]), False, None, False)
    calls, offs, index = plan_calls(queue, offsets, decoders)
    width = 7 if prefix is not None else 6 if ctc_prefix is not None else 4 if beams is not None else 3     # the only code that knows them
    return [(c.length, c.slots, c.offsets, c.decoder.beam, c.decoder.plan_kind, c.decoder.use_context, c.decoder.weights)[:width]
            for c in calls], offs, index


def wave_frames(n: int, n_fft: int, final: bool) -> int:
    """Frames of the streaming front-end emittable from n samples (rnnt_pool_wave's host arithmetic): frame f covers samples
    [f*512 - n_fft/2, f*512 + n_fft/2); before the end of the utterance every frame whose span ends by n, and none until frame 0's
    left reflection exists (n >= n_fft/2 + 1); at the end all 1 + n // 512, or none for n <= n_fft/2."""
    half = n_fft // 2
    if final:
        return 1 + n // 512 if n > half else 0
    return (n - half) // 512 + 1 if n >= half + 1 else 0


def wave_plan(queue, samples, fifo, chunk_frames, n_fft=1024):
    """The audio side of one StreamPool.step as a pure function (no GPU, no tensors): ONE rnnt_pool_wave call whatever the number of
    slots and packets, then the chunks that leave the per-slot frame FIFOs.

    queue: [(slot, n_samples, final)] in feed order, several packets per slot allowed (they are concatenated; the utterance is final
    when any of them says so); samples: {slot: samples received before}; fifo: {slot: frames waiting from earlier steps}.
    Returns (call, chunks, new_samples, new_fifo): call = (slots, counts, finals, frames) -- the rows of the call in order of each
    slot's first packet, the new samples, final flag and frames emitted per row -- or None for an empty queue; chunks = [(slot, start,
    length)] in row order: slices of the slot's FIFO (old frames, then the new ones) that go to the chunk queue, every full
    chunk_frames and, at final, the remainder as the slot's last chunk (feed() skips it under 7 frames, as process_single_chunk
    does); new_fifo = frames left waiting."""
    new_samples, new_fifo = dict(samples), dict(fifo)
    if not queue:
        return None, [], new_samples, new_fifo
    slots, counts, finals = [], {}, {}
    for slot, n, final in queue:
        if slot not in counts:
            slots.append(slot)
            counts[slot], finals[slot] = 0, False
        assert not finals[slot], f"slot {slot}: a packet after the final one"
        counts[slot] += int(n)
        finals[slot] = bool(final)
    frames, chunks = [], []
    for slot in slots:
        before = samples.get(slot, 0)
        nf = wave_frames(before + counts[slot], n_fft, finals[slot]) - wave_frames(before, n_fft, False)
        frames.append(nf)
        new_samples[slot] = before + counts[slot]
        have, at = fifo.get(slot, 0) + nf, 0
        while have - at >= chunk_frames:
            chunks.append((slot, at, chunk_frames))
            at += chunk_frames
        if finals[slot] and have > at:
            chunks.append((slot, at, have - at))
            at = have
        new_fifo[slot] = have - at
    return (slots, [counts[s] for s in slots], [finals[s] for s in slots], frames), chunks, new_samples, new_fifo


FRAME_MS = 40    # one encoder frame of the pool (OnlineRNNTModel.FRAME_SECONDS), in the integer milliseconds EndpointConfig divides by

# what StreamPool.endpoints() returns per slot: the rule that fired (0: none yet; it is sticky) and the frame count at which it did,
# then the running counters -- encoder frames so far, the trailing blank run, the non-blank frames
Endpoint = namedtuple("Endpoint", ["rule", "at_frame", "frames", "trailing", "speech"])


# One finished utterance of a slot that stays open (StreamPool.next_segment / segments): its number in the slot's session, the encoder
# frames the slot had encoded before it and in it, what close() would have returned for it, and the endpoint state it ended with
# (None on a slot without an EndpointConfig).  Frame indices inside result / endpoint are relative to the segment: add start_frame.
Segment = namedtuple("Segment", ["index", "start_frame", "frames", "result", "endpoint"])


class EndpointConfig:
    """When is the caller done: the rule of rnnt_stream_endpoint (include/rnnt_hip.h) in milliseconds, WeNet's runtime endpointer's
    shape and defaults.  A frame is blank when the CTC head's blank posterior exceeds blank_threshold; rule 1 fires after rule1_ms of
    trailing blank with nothing said yet, rule 2 after rule2_ms of trailing blank once min_speech_frames non-blank frames were seen,
    rule 3 at rule3_ms of audio; 0 switches a rule off.  Milliseconds become encoder frames of 40 ms by floor division: 125, 25 and
    500 frames by default."""

    def __init__(self, blank_threshold: float = 0.8, rule1_ms: int = 5000, rule2_ms: int = 1000, rule3_ms: int = 20000, min_speech_frames: int = 1):
        assert OnlineRNNTModel.FRAME_SECONDS * 1000 == FRAME_MS
        self.blank_threshold = float(blank_threshold)
        self.min_speech_frames = int(min_speech_frames)
        self.rule1_trailing, self.rule2_trailing, self.rule3_frames = (int(ms) // FRAME_MS for ms in (rule1_ms, rule2_ms, rule3_ms))

    def as_tuple(self):
        return (self.blank_threshold, self.min_speech_frames, self.rule1_trailing, self.rule2_trailing, self.rule3_frames)


# ---- the slot kinds of the pool: the only place that knows what a kind is opened with, advanced by and read through ------------------
# what: the kind's name in a refusal.  collects_tokens: step() hands out its new tokens.  advance(decoder) -> the engine method of its
# chunk call and that call's arguments between (slots, ptr, length, offsets, offsets) and the stream.  read(engine, decoder, slot, final,
# stream) -> its hypotheses, which is also what close() and a Segment return.  first_pass(hyps) -> [(tokens, score)] for rescore(), None:
# the kind is no first pass.  Engine methods are looked up when they are called: an engine needs only those of the kinds it serves.
_Kind = namedtuple("_Kind", ["what", "collects_tokens", "advance", "read", "first_pass"])


def _read_ctc_prefix(engine, d, slot, final, stream):
    if d.use_ngram:                                     # the totals carry the n-gram score (final: with the end term)
        return [(h[0], h[1], h[2]) for h in engine.stream_ctc_prefix_ngram(slot, final, stream=stream)]
    return [(tok, score, times) for tok, score, times, _ in engine.stream_ctc_prefix(slot, final, stream=stream)]


def _read_prefix(engine, d, slot, final, stream, with_context_scores=False, with_ngram_scores=False):
    if d.use_ngram or with_ngram_scores:                # the totals carry the n-gram score (final: with the end term)
        return [(tok, score) + ((cs,) if with_context_scores else ()) + ((ns,) if with_ngram_scores else ())
                for tok, score, cs, ns in engine.stream_prefix_ngram(slot, final, stream=stream)]
    if not d.use_context and not with_context_scores:
        return engine.stream_prefix(slot, stream=stream)            # no context score to finalize: final reads the same
    hyps = engine.stream_prefix_ctx(slot, final, stream=stream)
    return hyps if with_context_scores else [(tok, score) for tok, score, _ in hyps]


_KINDS = {
    "greedy": _Kind("greedy", True, lambda d: ("pool_chunk", (True,)),
                    lambda engine, d, slot, final, stream: engine.stream_tokens(slot, 0, stream), None),
    "beam": _Kind("beam", False, lambda d: ("pool_chunk_beam", (d.beam,)),
                  lambda engine, d, slot, final, stream: [BeamHypothesis(t, lp) for t, lp in engine.stream_beam(slot, stream)], None),
    "ctc_prefix": _Kind("CTC prefix", False,
                        lambda d: ("pool_chunk_ctc_prefix_ngram", (d.beam, d.use_context, True)) if d.use_ngram else
                                  ("pool_chunk_ctc_prefix", (d.beam, d.use_context)),
                        _read_ctc_prefix, lambda hyps: [(tok, score) for tok, score, _ in hyps]),
    "prefix": _Kind("transducer prefix", False,
                    lambda d: ("pool_chunk_prefix_ngram", (d.beam,) + d.weights + (d.use_context, True)) if d.use_ngram else
                              ("pool_chunk_prefix_ctx", (d.beam,) + d.weights + (True,)) if d.use_context else
                              ("pool_chunk_prefix", (d.beam,) + d.weights),
                    _read_prefix, lambda hyps: [(tok[1:], score) for tok, score in hyps]),      # the first pass drops the leading blank
}


def _decoder_of_open(pool, beam_size, ctc_prefix_beam, context, prefix_beam, ctc_weight, transducer_weight, prefix_context, endpoint,
                     on_endpoint, ngram, prefix_ngram=None) -> Decoder:
    """The Decoder that open()'s keywords select, or the RnntError of the first rule they break.  The order of the checks is part of the
    facade's behaviour: an open() with several faults reports the first one here."""
    if ngram is not None:
        if not ctc_prefix_beam:
            raise RnntError("stream pool: ngram needs ctc_prefix_beam")
        if ngram is not pool._ngram and any(r.ngram is not None for r in pool._slots.values()):
            raise RnntError("stream pool: another n-gram model is in use by an open slot (one model per pool at a time)")
    if prefix_ngram is not None:
        if not prefix_beam:
            raise RnntError("stream pool: prefix_ngram needs prefix_beam")
        if prefix_ngram is not pool._ngram and any(r.ngram is not None for r in pool._slots.values()):
            raise RnntError("stream pool: another n-gram model is in use by an open slot (one model per pool at a time)")
    if on_endpoint not in (None, "keep", "fresh"):
        raise RnntError(f"stream pool: on_endpoint {on_endpoint!r} is not None, 'keep' or 'fresh'")
    if on_endpoint is not None and endpoint is None:
        raise RnntError("stream pool: on_endpoint needs endpoint (an EndpointConfig)")
    biased_open = any(r.context is not None for r in pool._slots.values())
    if prefix_context is not None:
        if not prefix_beam:
            raise RnntError("stream pool: prefix_context needs prefix_beam")
        if prefix_context is not pool._context and biased_open:
            raise RnntError("stream pool: another context graph is in use by an open slot (one graph per pool at a time)")
    if prefix_beam:
        if beam_size or ctc_prefix_beam:
            raise RnntError("stream pool: prefix_beam, beam_size and ctc_prefix_beam are mutually exclusive")
        if context is not None:
            raise RnntError("stream pool: context biases the CTC prefix search only (ctc_prefix_beam)")
        if prefix_beam < 1 or prefix_beam > min(16, pool.vocab_size) or pool.vocab_size > 512:
            raise RnntError(f"stream pool: prefix_beam {prefix_beam} outside [1, min(16, vocabulary {pool.vocab_size})] or vocabulary > 512")
        if not ctc_weight >= 0 or not transducer_weight >= 0 or (ctc_weight == 0 and transducer_weight == 0):
            raise RnntError(f"stream pool: weights {ctc_weight} / {transducer_weight} (negative, or both zero)")
    if ctc_prefix_beam:
        if beam_size:
            raise RnntError("stream pool: beam_size and ctc_prefix_beam are mutually exclusive")
        if ctc_prefix_beam < 1 or ctc_prefix_beam > min(16, pool.vocab_size) or pool.vocab_size > 512:
            raise RnntError(f"stream pool: ctc_prefix_beam {ctc_prefix_beam} outside [1, min(16, vocabulary {pool.vocab_size})] or vocabulary > 512")
        if context is not None and context is not pool._context and biased_open:
            raise RnntError("stream pool: another context graph is in use by an open slot (one graph per pool at a time)")
    elif context is not None:
        raise RnntError("stream pool: context needs ctc_prefix_beam")
    if beam_size < 0 or beam_size > 0 and (beam_size > min(pool.max_beam, 16) or pool.vocab_size > 512):
        raise RnntError(f"stream pool: beam_size {beam_size} outside [0, min(max_beam {pool.max_beam}, 16)] or vocabulary "
                        f"{pool.vocab_size} > 512")
    if prefix_beam:
        return Decoder("prefix", int(prefix_beam), prefix_context is not None, (float(ctc_weight), float(transducer_weight)), prefix_ngram is not None)
    if ctc_prefix_beam:
        return Decoder("ctc_prefix", int(ctc_prefix_beam), context is not None, None, ngram is not None)
    return Decoder("beam", int(beam_size), False, None, False) if beam_size else GREEDY


class _Slot:
    """What the pool keeps of one open slot; "open" is "has a record", and close() drops it whole."""

    def __init__(self, decoder: Decoder, context: Optional[ContextBias], ngram: Optional[NgramLM], keep_frames: bool,
                 endpoint: Optional[EndpointConfig], on_endpoint: Optional[str]):
        self.decoder, self.context, self.ngram = decoder, context, ngram    # with the graph and the model it was opened with
        self.keep_frames = keep_frames
        self.endpoint = endpoint                        # the slot detects its endpoint under this config
        self.on_endpoint = on_endpoint                  # "keep" / "fresh": step() segments the slot when its rule has fired
        self.offset = 0                                 # encoder offset so far
        self.ntok = 0                                   # tokens already handed out by step()
        self.segment = (0, 0)                           # (index, start_frame) of the current segment
        self.fed: Optional[str] = None                  # "feed" / "wave": how the slot is fed (fixed by its first chunk or packet)
        self.wave_samples = 0                           # a wave slot: samples received,
        self.wave_fifo: Optional[torch.Tensor] = None   # [k, 80] frames waiting for a full chunk,
        self.wave_final = False                         # and whether the final packet has been queued


class StreamPool:
    """A context's slots, each with its own life (not in the reference, which is B=1): open() a slot when a caller connects, feed()
    it a chunk whenever the caller has one, step() to advance whatever subset of slots has chunks queued -- each at its own cache
    length, positional window and encoder offset, through rnnt_pool_chunk -- and close() it when the caller hangs up.  The tokens of
    an utterance are those of process_single_chunk on a model that holds only that stream, whatever the other slots do.
    Beam search per slot (max_beam > 0): open(beam_size=k) gives the slot a beam of its own, resident on the device, advanced by
    rnnt_pool_chunk_beam; beams(slot) returns what process_single_chunk_beam_search returns after each chunk, and close(slot) the
    final hypotheses.  Greedy and beam slots live side by side in one pool; a library call holds slots of one kind.
    CTC prefix beam search with hot words per slot: open(ctc_prefix_beam=k, context=None | ContextBias) gives the slot WeNet's
    ctc_prefix_beam_search on the CTC head, carried across chunks on the device by rnnt_pool_chunk_ctc_prefix (one call = encode +
    CTC + search of the new frames); ctc_hyps(slot) reads the hypotheses as they stand and close(slot) returns the final ones, those
    of the one-launch search over the utterance's frames.  The pool holds one context graph at a time.
    Audio in: feed_wave(slot, samples, final) queues PCM packets instead of feature chunks; step() first turns the packets of all
    slots into fbank frames with ONE rnnt_pool_wave call (the streaming form of rnnt_fbank: per slot the frames of the whole
    waveform, whatever the packet split), collects them in a per-slot device FIFO and moves every full chunk_frames, and at final
    the remainder, to the chunk queue.  A slot is fed either way, never both.
    Two-pass decoding: open(..., keep_frames=True) makes the slot keep its encoder frames on the device; rescore(slots, ctc_weight,
    transducer_weight) re-scores the n-best of CTC prefix slots with the transducer likelihood over their own frames in one library
    call (WeNet's transducer_attention_rescoring, per slot and mid-utterance if wanted), frames(slot) reads the frames and
    token_times(slot) aligns a greedy slot's tokens over them.
    Transducer prefix beam search per slot: open(prefix_beam=k, ctc_weight=, transducer_weight=) gives the slot WeNet's CTC-fused
    prefix beam search (rnnt_prefix_beam_decode's), carried across chunks on the device by rnnt_pool_chunk_prefix (with
    prefix_context=ContextBias: biased by hot words, rnnt_pool_chunk_prefix_ctx; the pool's one graph serves both searches); prefix_hyps(slot)
    reads the hypotheses as they stand, close(slot) returns the final ones -- those of the one-call search over the utterance's
    frames -- and rescore() takes such a slot as the first pass of the reference's own two-pass recipe.
    When is the caller done: open(..., endpoint=EndpointConfig(...)) makes the library watch the slot's CTC blank posterior inside the
    pool calls that encode it (any slot kind, one extra launch per call); endpoints() reads rule and counters of all such slots with
    one download.
    Segments: next_segment(slot, keep_encoder=True) ends the slot's utterance and starts the next one in the same slot -- its result is
    returned as a Segment, its decoders start over (rnnt_pool_segment), its audio stream and its configuration stay.  keep_encoder=True
    is WeNet's continuous decoding (the encoder's caches run on), False restarts the encoder too, which is how a session outlives
    max_cache_frames.  open(..., endpoint=, on_endpoint="keep" | "fresh") lets step() do it whenever the slot's rule has fired;
    segments(slot) hands out what it finished."""

    def __init__(self, state_dict, n_slots: int, vocab_size: int = 412, blank_id: int = 5, max_chunk_frames: int = 64,
                 max_cache_frames: int = 512, max_tokens: int = 4096, device: int = 0, numerics=None, packed=None, engine=None,
                 max_beam: int = 0, sample_rate: int = 16000, n_fft: int = 1024, chunk_frames: int = 16):
        """state_dict / packed: as StreamingBatch.  engine: an object with reset / stream_open / pool_chunk / stream_tokens (and
        pool_chunk_beam / stream_beam for beam slots, pool_chunk_ctc_prefix / stream_ctc_prefix / context_set for CTC prefix slots,
        pool_chunk_prefix / stream_prefix for transducer prefix slots,
        stream_keep_frames / stream_frames / pool_rescore / transducer_align for slots that keep their frames,
        stream_endpoint / pool_endpoints for slots opened with an EndpointConfig,
        pool_segment / stream_segment for next_segment and on_endpoint)
        to drive instead of a new RnntEngine (a recording fake in the CPU tests).
        max_beam: the largest beam_size open() may be given (0: greedy only).
        sample_rate / n_fft / chunk_frames: the front-end of feed_wave and the chunk length its frames are fed in (the engine also
        needs pool_wave then)."""
        self.n = n_slots
        self.sample_rate, self.n_fft, self.chunk_frames = int(sample_rate), int(n_fft), int(chunk_frames)
        self._wave_device = torch.device("cuda", device) if engine is None else None   # an injected engine: where the packets are
        self.blank_id = blank_id
        self.max_beam = max_beam
        self.vocab_size = vocab_size
        if engine is None:
            engine = RnntEngine(max_streams=n_slots, max_chunk_frames=max_chunk_frames, max_cache_frames=max_cache_frames,
                                max_enc_frames=max(16, (max_chunk_frames + 3) // 4), max_tokens=max_tokens, vocab_size=vocab_size,
                                blank_id=blank_id, n_steps=10, device=device, max_beam=max_beam)
            if packed is not None:
                assert state_dict is None and int(packed[1]) == vocab_size, "packed=(blob, vocab): vocab must equal vocab_size"
                engine.load_packed(packed[0], int(packed[1]), numerics=numerics)
            else:
                engine.load_state_dict(state_dict, numerics=numerics)
        self.engine = engine
        self._context: Optional[ContextBias] = None     # the ContextBias whose graph the context holds (it outlives reset())
        self._ngram: Optional[NgramLM] = None           # likewise the NgramLM whose model the context holds
        self.reset()

    def reset(self):
        """All slots free; the context freshly reset (the lock-step entry points work again until the first open)."""
        self.engine.reset(self.n, self._stream(None))
        self._free = list(range(self.n))
        self._slots: Dict[int, _Slot] = {}              # the open slots
        # the one thing kept per slot outside its record: what step() finished for an on_endpoint slot, until segments(slot) takes it.
        # segments() hands these out after close() too, so they outlive the record; the slot's next open() discards them
        self._segments: Dict[int, List[Segment]] = {}
        self._queue: List[Tuple[int, torch.Tensor]] = []
        self._carry: Dict[int, List[int]] = {}          # increments of other slots produced by the step inside a close()
        self._wave_queue: List[Tuple[int, torch.Tensor, bool]] = []   # PCM packets (slot, samples, final) in feed order

    @staticmethod
    def _stream(t):
        return _stream_ptr() if (t is None and torch.cuda.is_available()) or (t is not None and t.is_cuda) else None

    def _open_slot(self, slot: int) -> _Slot:
        if slot not in self._slots:
            raise RnntError(f"slot {slot} is not open")
        return self._slots[slot]

    def _slot_of_kind(self, slot: int, kind: str) -> _Slot:
        rec = self._slots.get(slot)
        if rec is None or rec.decoder.kind != kind:
            raise RnntError(f"slot {slot} is not an open {_KINDS[kind].what} slot")
        return rec

    def _queued(self, slot: int) -> bool:
        return any(s == slot for s, _ in self._queue) or any(s == slot for s, _, _ in self._wave_queue)

    def open(self, beam_size: int = 0, ctc_prefix_beam: int = 0, context: Optional[ContextBias] = None, keep_frames: bool = False,
             prefix_beam: int = 0, ctc_weight: float = 0.3, transducer_weight: float = 0.7, prefix_context: Optional[ContextBias] = None,
             endpoint: Optional[EndpointConfig] = None, on_endpoint: Optional[str] = None, ngram: Optional[NgramLM] = None,
             prefix_ngram: Optional[NgramLM] = None) -> int:
        """The lowest free slot, reset for a new utterance (reset_streaming_cache for that slot alone).  beam_size > 0: the slot's
        utterance is beam-searched with that beam (its hypotheses start as the one empty hypothesis); raises RnntError at once
        when this pool cannot do it.  ctc_prefix_beam > 0 (not together with beam_size): the slot's utterance runs the CTC prefix beam
        search with that beam, biased by `context` when given.  The pool holds one graph at a time: a context other than the current
        one is uploaded (context_set) unless another biased slot is still open, which raises RnntError.  A refused open() -- a
        graph the library rejects included (an empty phrase, the blank, a token outside the vocabulary) -- takes no slot.
        keep_frames: the slot keeps the encoder frames of its utterance on the device (rnnt_stream_keep_frames, max_cache_frames KB),
        what frames(), rescore() and token_times() read.
        prefix_beam > 0 (not together with beam_size or ctc_prefix_beam, and without context): the slot's utterance runs the
        transducer prefix beam search with that beam and the fusion weights ctc_weight / transducer_weight (>= 0, not both 0), biased
        by prefix_context when given (`context` belongs to ctc_prefix_beam).  The one graph of the pool serves both kinds: a graph other
        than the current one is refused while any biased slot of either kind is open.
        endpoint: the slot (of any kind) detects its endpoint under that config (rnnt_stream_endpoint); endpoints() reads the result.
        A config the library refuses takes no slot.
        on_endpoint: "keep" / "fresh" (needs endpoint): after its chunk calls step() reads the endpoints once and, for every such slot
        whose rule has fired, does what next_segment(slot, keep_encoder = on_endpoint == "keep") does; segments(slot) returns the
        finished Segments.  None: the slot's utterance ends with close() or next_segment() only.
        ngram (needs ctc_prefix_beam): the slot's search fuses that NgramLM (rnnt_pool_chunk_ctc_prefix_ngram calls of their own).  The
        pool holds one model at a time, with the graph's rule: a model other than the current one is uploaded (ngram_set) unless
        another slot that fuses one is still open, which raises RnntError and takes no slot.
        prefix_ngram (needs prefix_beam): the slot's transducer prefix search fuses that NgramLM (rnnt_pool_chunk_prefix_ngram calls of
        their own; `ngram` belongs to ctc_prefix_beam).  The one model of the pool serves both kinds, as the one graph does."""
        decoder = _decoder_of_open(self, beam_size, ctc_prefix_beam, context, prefix_beam, ctc_weight, transducer_weight, prefix_context,
                                   endpoint, on_endpoint, ngram, prefix_ngram)
        ngram = ngram if ngram is not None else prefix_ngram
        if not self._free:
            raise RnntError(f"stream pool full: all {self.n} slots are open")
        graph = context if context is not None else prefix_context
        if graph is not None and graph is not self._context:       # before a slot is taken: the library may refuse the graph
            self.engine.context_set(graph.phrases, graph.context_score)
            self._context = graph
        if ngram is not None and ngram is not self._ngram:         # likewise
            self.engine.ngram_set(ngram)
            self._ngram = ngram
        slot = self._free[0]
        self.engine.stream_open(slot, self._stream(None))
        if keep_frames:
            self.engine.stream_keep_frames(slot, True, self._stream(None))
        if endpoint is not None:
            self.engine.stream_endpoint(slot, endpoint.as_tuple(), self._stream(None))
        self._free.pop(0)
        self._slots[slot] = _Slot(decoder, graph, ngram, bool(keep_frames), endpoint, on_endpoint)
        self._segments.pop(slot, None)
        if on_endpoint is not None:
            self._segments[slot] = []
        return slot

    def feed(self, slot: int, chunk: torch.Tensor) -> bool:
        """Queue one chunk [T, 80] (float32, on the device) for an open slot; the next step() encodes and decodes it.  A chunk of
        fewer than 7 frames is skipped as in process_single_chunk (:356-359): returns False and the slot's offset stays.  Raises
        RnntError on a slot fed through feed_wave."""
        rec = self._open_slot(slot)
        rec.fed = rec.fed or "feed"
        if rec.fed != "feed":
            raise RnntError(f"slot {slot} is fed audio (feed_wave): feature chunks cannot be mixed in")
        return self._feed_chunk(slot, chunk)

    def _feed_chunk(self, slot: int, chunk: torch.Tensor) -> bool:
        assert chunk.dim() == 2 and chunk.size(1) == 80 and chunk.dtype == torch.float32
        if chunk.size(0) < 7:
            print(f"Warning: Chunk too small ({chunk.size(0)} frames), skipping")
            return False
        self._queue.append((slot, chunk))
        return True

    def feed_wave(self, slot: int, samples: torch.Tensor, final: bool = False):
        """Queue one PCM packet (1-D float32, on the host or the device; it may be empty) for an open slot; final: the utterance ends
        with it.  The next step() turns the queued packets of all slots into frames with one rnnt_pool_wave call and feeds every
        full chunk_frames of them, at final also the remainder.  Raises RnntError on a slot fed through feed(), or after its final
        packet."""
        rec = self._open_slot(slot)
        rec.fed = rec.fed or "wave"
        if rec.fed != "wave":
            raise RnntError(f"slot {slot} is fed feature chunks (feed): audio cannot be mixed in")
        if rec.wave_final:
            raise RnntError(f"slot {slot}: its utterance has ended (final packet already queued)")
        assert samples.dim() == 1 and samples.dtype == torch.float32
        rec.wave_final = bool(final)
        self._wave_queue.append((slot, samples, bool(final)))

    def _wave_step(self):
        """The queued packets of all slots through ONE rnnt_pool_wave call (wave_plan); full chunks leave the FIFOs for the chunk queue."""
        queue, self._wave_queue = self._wave_queue, []
        recs = {slot: self._slots[slot] for slot, _, _ in queue}
        call, chunks, samples, _ = wave_plan([(slot, p.numel(), fin) for slot, p, fin in queue], {slot: r.wave_samples for slot, r in recs.items()},
                                             {slot: r.wave_fifo.size(0) for slot, r in recs.items() if r.wave_fifo is not None},
                                             self.chunk_frames, self.n_fft)
        for slot, n in samples.items():
            recs[slot].wave_samples = n
        slots, counts, finals, frames = call
        dev = self._wave_device if self._wave_device is not None else queue[0][1].device
        parts: Dict[int, List[torch.Tensor]] = {slot: [] for slot in slots}
        for slot, p, _ in queue:
            parts[slot].append(p)
        rows = [parts[s][0] if len(parts[s]) == 1 else torch.cat(parts[s]) for s in slots]      # a slot's packets side by side in its row
        if any(r.device != rows[0].device for r in rows):
            rows = [r.to(dev) for r in rows]
        if max(counts) == 0:
            wave = torch.zeros(len(slots), 1, dtype=torch.float32, device=dev)
        elif min(counts) == max(counts):
            wave = torch.stack(rows, 0).to(dev)
        else:
            wave = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True).to(dev)                # rows padded to the longest
        n_max, cap = wave.size(1), max(max(frames), 1)
        out = torch.empty(len(slots), cap, 80, dtype=torch.float32, device=dev)
        got = self.engine.pool_wave(slots, wave.data_ptr(), n_max, counts, finals, out.data_ptr(), cap, self.sample_rate, self.n_fft, self._stream(wave))
        assert [int(g) for g in got] == frames, f"rnnt_pool_wave wrote {list(got)} frames, the plan says {frames}"
        for i, slot in enumerate(slots):
            if frames[i]:
                old = recs[slot].wave_fifo
                recs[slot].wave_fifo = out[i, :frames[i]] if old is None or old.size(0) == 0 else torch.cat([old, out[i, :frames[i]]], 0)
        taken: Dict[int, int] = {}
        for slot, start, length in chunks:
            self._feed_chunk(slot, recs[slot].wave_fifo[start:start + length].contiguous())
            taken[slot] = start + length
        for slot, k in taken.items():
            recs[slot].wave_fifo = recs[slot].wave_fifo[k:]

    def step(self) -> Dict[int, List[int]]:
        """Advance every slot that has chunks queued: one rnnt_pool_chunk call per chunk length of the greedy slots and one
        rnnt_pool_chunk_beam call per (chunk length, beam size) of the beam slots (plan_calls), the rows of a call gathered into one
        contiguous device tensor; CTC prefix slots likewise through one rnnt_pool_chunk_ctc_prefix call per (chunk length, beam size,
        use_context), transducer prefix slots through one rnnt_pool_chunk_prefix call per (chunk length, beam size, weights) -- the biased
        ones among them through rnnt_pool_chunk_prefix_ctx calls of their own.  Returns
        {slot: tokens emitted by this step} for the GREEDY slots that advanced; a beam slot's hypotheses are read with beams(slot), a
        CTC prefix slot's with ctc_hyps(slot), a transducer prefix slot's with prefix_hyps(slot)."""
        out, self._carry = self._carry, {}
        if self._wave_queue:
            self._wave_step()
        if not self._queue:
            return out
        recs = {slot: self._slots[slot] for slot, _ in self._queue}
        calls, offs, index = plan_calls([(slot, c.size(0)) for slot, c in self._queue], {slot: r.offset for slot, r in recs.items()},
                                        {slot: r.decoder for slot, r in recs.items()})
        rows: List[List[Optional[torch.Tensor]]] = [[None] * len(call.slots) for call in calls]
        for (slot, c), at in zip(self._queue, index):
            rows[at[0]][at[1]] = c
        touched = []
        for call, chunks in zip(calls, rows):
            x = torch.stack(chunks, 0).contiguous()
            kind = _KINDS[call.decoder.kind]
            method, args = kind.advance(call.decoder)
            getattr(self.engine, method)(call.slots, x.data_ptr(), call.length, call.offsets, call.offsets, *args, self._stream(x))
            if kind.collects_tokens:
                touched.extend(s for s in call.slots if s not in touched)
        for slot, offset in offs.items():
            recs[slot].offset = offset
        self._queue = []
        stream = self._stream(None)
        for slot in touched:
            new = self.engine.stream_tokens(slot, recs[slot].ntok, stream)
            recs[slot].ntok += len(new)
            out[slot] = out.get(slot, []) + new
        auto = [slot for slot, r in self._slots.items() if r.on_endpoint is not None]
        if auto:
            self._segment_fired(sorted(auto))
        return out

    def _read(self, slot: int, rec: _Slot, final: bool, *how):
        """The slot's hypotheses as its kind reads them; final=True: what close() returns for the utterance as it stands."""
        return _KINDS[rec.decoder.kind].read(self.engine, rec.decoder, slot, final, self._stream(None), *how)

    def _finish(self, slots: List[int], keep_encoder: bool, eps: Dict[int, Endpoint]) -> List[Segment]:
        """The results of the listed slots, then ONE rnnt_pool_segment call for all of them, then the facade's own records."""
        recs, stream = [self._slots[slot] for slot in slots], self._stream(None)
        results = [_KINDS[r.decoder.kind].read(self.engine, r.decoder, slot, True, stream) for slot, r in zip(slots, recs)]
        self.engine.pool_segment(slots, keep_encoder, stream)
        segs = []
        for slot, rec, res in zip(slots, recs, results):
            index, start = rec.segment
            rec.segment = tuple(int(v) for v in self.engine.stream_segment(slot))
            rec.ntok = 0
            if not keep_encoder:
                rec.offset = 0                          # the encoder starts over; with it kept the estimated offset runs on, as the cache does
            segs.append(Segment(index, start, rec.segment[1] - start, res, eps.get(slot)))
        return segs

    def _segment_fired(self, auto: List[int]):
        """step() with on_endpoint slots: ONE endpoints() read, then the slots whose rule has fired, one _finish per flavour."""
        eps = self.endpoints(auto)
        for flavour in ("keep", "fresh"):
            fired = [slot for slot, e in eps.items() if e.rule != 0 and self._slots[slot].on_endpoint == flavour]
            if fired:
                for seg, slot in zip(self._finish(fired, flavour == "keep", eps), fired):
                    self._segments[slot].append(seg)

    def next_segment(self, slot: int, keep_encoder: bool = True) -> Segment:
        """End the slot's utterance and start the next one in the same slot (queued chunks and packets are processed first, as in
        close()): returns its Segment -- result: what close() would have returned -- and leaves the slot open with its decoders, its
        endpoint counters and its kept frames started over.  The audio stream (feed_wave) goes on across the boundary: nothing is
        flushed, frames waiting for a full chunk belong to the next segment.  keep_encoder=True: the encoder's caches and the offset
        run on (continuous decoding); False: the encoder starts over too, the next chunk's offset is 0.  hot words, keep_frames and
        the endpoint config stay as open() set them."""
        rec = self._open_slot(slot)
        if self._queued(slot):
            self._carry = self.step()                   # the other slots' increments are handed out by the next step()
        self._carry.pop(slot, None)
        eps = self.endpoints([slot]) if rec.endpoint is not None else {}
        return self._finish([slot], bool(keep_encoder), eps)[0]

    def segments(self, slot: int) -> List[Segment]:
        """The Segments step() has finished for a slot opened with on_endpoint since the last call, oldest first (they survive close())."""
        done = self._segments.get(slot, [])
        if slot in self._segments:
            self._segments[slot] = []
        return done

    def beams(self, slot: int) -> List[BeamHypothesis]:
        """The current hypotheses of a beam slot, in beam order: what process_single_chunk_beam_search returns after each chunk
        (:605-645), also after a skipped < 7-frame chunk (:616-619).  Chunks still queued are not in them: step() first."""
        return self._read(slot, self._slot_of_kind(slot, "beam"), False)

    def ctc_hyps(self, slot: int, final: bool = False):
        """[(tokens, score, times)] of a CTC prefix slot in the search's order, as they stand after the chunks stepped so far (times:
        encoder-frame indices since the slot was opened, or since its current segment began).  final: what the one-launch search returns had the utterance ended here
        (finalize's context score instead of the running one).  Reading changes nothing."""
        return self._read(slot, self._slot_of_kind(slot, "ctc_prefix"), final)

    def prefix_hyps(self, slot: int, final: bool = False, with_context_scores: bool = False, with_ngram_scores: bool = False):
        """[(tokens including the leading blank, score)] of a transducer prefix slot, best first, as they stand after the chunks
        stepped so far.  A biased slot's scores are the totals (score + context score); final: with finalize's context scores, what
        the one-call search returns had the utterance ended here (no re-sort); with_context_scores: (tokens, score, context score).
        A slot that fuses a model (prefix_ngram) has its n-gram score in the totals too -- the running one, or with final the one
        with the end term; with_ngram_scores: every hypothesis ends with it.  Reading changes nothing."""
        return self._read(slot, self._slot_of_kind(slot, "prefix"), final, with_context_scores, with_ngram_scores)

    def endpoints(self, slots: Optional[List[int]] = None) -> Dict[int, Endpoint]:
        """{slot: Endpoint(rule, at_frame, frames, trailing, speech)} of the open slots that detect their endpoint, or of the listed
        ones (each must be such a slot), after the chunks stepped so far: ONE engine call (one download) for all of them, none when
        there is nothing to read.  Chunks still queued are not in it: step() first.  Reading changes nothing."""
        if slots is None:
            slots = sorted(slot for slot, r in self._slots.items() if r.endpoint is not None)
        slots = [int(x) for x in slots]
        for slot in slots:
            if slot not in self._slots or self._slots[slot].endpoint is None:
                raise RnntError(f"slot {slot} is not an open slot that detects its endpoint (open(endpoint=EndpointConfig(...)))", ERR_STATE)
        if not slots:
            return {}
        st = self.engine.pool_endpoints(slots, self._stream(None))
        return {slot: Endpoint(int(r[3]), int(r[4]), int(r[0]), int(r[1]), int(r[2])) for slot, r in zip(slots, st)}

    def _require_kept(self, slot: int) -> _Slot:
        if slot not in self._slots or not self._slots[slot].keep_frames:
            raise RnntError(f"slot {slot} is not an open slot that keeps its frames (open(keep_frames=True))", ERR_STATE)
        return self._slots[slot]

    def frames(self, slot: int) -> torch.Tensor:
        """The encoder frames [t, 256] of the slot's utterance so far (a device tensor, a copy): what the chunks stepped so far gave,
        the rows rnnt_get_enc_frames returns per chunk, concatenated."""
        self._require_kept(slot)
        return self.engine.stream_frames(slot, 0, self._stream(None))

    def rescore(self, slots: List[int], ctc_weight: float, transducer_weight: float):
        """The second pass for CTC prefix and transducer prefix slots opened with keep_frames=True: per slot ctc_hyps(final=True) --
        or prefix_hyps (the final totals of a biased slot or one that fuses a model) with the leading blank dropped and the search's score as the first score, the reference's default first pass
        (beam_search_type="transducer", wenet/transducer/transducer.py:327) --, then ONE
        rnnt_pool_rescore call for all listed slots -- every hypothesis re-scored with the transducer likelihood over the slot's kept
        frames -- then the choice of rnnt_rescore_select_host with total = ctc_score * ctc_weight + td_score * transducer_weight.
        Returns {slot: (best_index, [(tokens, ctc_score, td_score, total)])} in the search's order.  Only reads the slots: their
        searches go on, so partial results may be re-scored mid-utterance (queued chunks are not in them: step() first)."""
        slots = [int(x) for x in slots]
        for slot in slots:
            if slot not in self._slots or _KINDS[self._slots[slot].decoder.kind].first_pass is None:
                raise RnntError(f"slot {slot} is not an open CTC prefix or transducer prefix slot")
            self._require_kept(slot)
        first = [_KINDS[self._slots[slot].decoder.kind].first_pass(self._read(slot, self._slots[slot], True)) for slot in slots]
        nh, hl, ht = pack_nbest([[tok for tok, _ in row] for row in first])
        nll = self.engine.pool_rescore(slots, nh, hl, ht, self._stream(None))
        return {slot: select_rescored([tok for tok, _ in row], [sc for _, sc in row], nll[i, :nh[i]], ctc_weight, transducer_weight)
                for i, (slot, row) in enumerate(zip(slots, first))}

    def token_times(self, slot: int, frame_rate: float = 0.04):
        """[(start_s, end_s)] per token emitted so far by a GREEDY slot that keeps its frames: the best transducer alignment
        (rnnt_transducer_align) of its tokens over its kept frames, then timestamps_from_peaks of the emit frames with max_duration
        = the frames so far.  Raises RnntError beyond 255 tokens (the alignment's range)."""
        if self._require_kept(slot).decoder.kind != "greedy":
            raise RnntError(f"slot {slot} is not a greedy slot")
        s = self._stream(None)
        tokens = self.engine.stream_tokens(slot, 0, s)
        if len(tokens) > 255:
            raise RnntError(f"slot {slot}: {len(tokens)} tokens, the alignment holds at most 255", ERR_SHAPE)
        enc = self.engine.stream_frames(slot, 0, s)
        t = enc.size(0)
        if t == 0 or not tokens:
            return []
        _, emit = self.engine.transducer_align(enc.data_ptr(), [t], np.asarray(tokens, np.int32).reshape(1, -1), [len(tokens)], 1, t, stream=s)
        return timestamps_from_peaks(emit[0, :len(tokens)].tolist(), t * frame_rate, frame_rate)

    def close(self, slot: int):
        """Finish the slot's utterance (queued chunks are processed first) and free the slot; returns all its tokens (greedy slot),
        its final hypotheses (beam slot), ctc_hyps(slot, final=True) (CTC prefix slot) or prefix_hyps(slot, final=True) (transducer prefix slot)."""
        rec = self._open_slot(slot)
        if rec.fed == "wave" and not rec.wave_final:
            self.feed_wave(slot, torch.zeros(0, dtype=torch.float32), final=True)   # the caller hung up: flush the tail
        if self._queued(slot):
            self._carry = self.step()                   # the other slots' increments are handed out by the next step()
        self._carry.pop(slot, None)
        res = self._read(slot, rec, True)
        del self._slots[slot]                           # nothing else to forget; the library clears its flags when the slot is opened again
        self._free.append(slot)
        self._free.sort()
        return res
