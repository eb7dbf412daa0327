"""StreamPool as a whole, without a GPU: every slot kind side by side in one pool over a complete recording engine -- the ordered log
of what the library is asked and every value the facade returns -- and every open() the facade refuses, with its message.  The expected
values are literals recorded from the facade as it stood before the slot record and the kinds table replaced its per-feature dicts."""
import numpy as np
import pytest
import torch

from ctc_vr_amd.lib import ERR_ARG, RnntError
from ctc_vr_amd.ngram import NgramLM
from ctc_vr_amd.online_rnnt_model import BeamHypothesis, ContextBias, Endpoint, EndpointConfig, Segment, StreamPool

CFG = EndpointConfig(0.5, 0, 0, 6 * 40, 1)
GRAMS = [((1,), -1.0, -0.5), ((2,), -2.0, -0.25), ((1, 2), -0.5, 0.0)]


class Engine:
    """Every engine method StreamPool drives except pool_wave, with the positional arguments the facade passes; one ordered log (data
    pointers and streams left out).  A slot's tokens are one per chunk call since its segment began; pool_endpoints reports rule 3 for the
    slots in `fire` once they have had two chunk calls in the segment.  `refuse`: the method that raises instead."""

    def __init__(self, fire=(), refuse=None):
        self.log, self.fire, self.refuse = [], set(fire), refuse
        self.n, self.frames, self.seg = {}, {}, {}          # slot -> chunk calls in the segment, encoder frames since open, (index, start)

    def _say(self, *entry):
        self.log.append(entry)
        if entry[0] == self.refuse:
            raise RnntError(f"rnnt_{entry[0]}: refused (status -1)", ERR_ARG)

    def reset(self, n, stream):
        self._say("reset", n)

    def context_set(self, phrases, context_score):
        self._say("context_set", [list(p) for p in phrases], context_score)

    def ngram_set(self, ngram):
        self._say("ngram_set", ngram.lm_weight)

    def stream_open(self, slot, stream):
        self._say("stream_open", slot)
        self.n[slot], self.frames[slot], self.seg[slot] = 0, 0, (0, 0)

    def stream_keep_frames(self, slot, keep, stream):
        self._say("stream_keep_frames", slot, keep)

    def stream_endpoint(self, slot, cfg, stream):
        self._say("stream_endpoint", slot, tuple(cfg))

    def _advance(self, name, slots, ptr, length, offsets, required, *rest):
        assert ptr != 0
        self._say(name, list(slots), length, list(offsets), list(required), *rest)
        for s in slots:
            self.n[s] += 1
            self.frames[s] += length // 4

    def pool_chunk(self, slots, ptr, length, offsets, required, greedy, stream):
        self._advance("pool_chunk", slots, ptr, length, offsets, required, greedy)

    def pool_chunk_beam(self, slots, ptr, length, offsets, required, beam_size, stream):
        self._advance("pool_chunk_beam", slots, ptr, length, offsets, required, beam_size)

    def pool_chunk_ctc_prefix(self, slots, ptr, length, offsets, required, beam_size, use_context, stream):
        self._advance("pool_chunk_ctc_prefix", slots, ptr, length, offsets, required, beam_size, use_context)

    def pool_chunk_ctc_prefix_ngram(self, slots, ptr, length, offsets, required, beam_size, use_context, use_ngram, stream):
        self._advance("pool_chunk_ctc_prefix_ngram", slots, ptr, length, offsets, required, beam_size, use_context, use_ngram)

    def pool_chunk_prefix(self, slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, stream):
        self._advance("pool_chunk_prefix", slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight)

    def pool_chunk_prefix_ctx(self, slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context, stream):
        self._advance("pool_chunk_prefix_ctx", slots, ptr, length, offsets, required, beam_size, ctc_weight, transducer_weight, use_context)

    def _tokens(self, slot, base):
        return [base * slot + k for k in range(self.n[slot])]

    def stream_tokens(self, slot, start, stream):
        self._say("stream_tokens", slot, start)
        return self._tokens(slot, 100)[start:]

    def stream_beam(self, slot, stream):
        self._say("stream_beam", slot)
        return [(self._tokens(slot, 1000), -0.5 * self.n[slot])]

    def stream_ctc_prefix(self, slot, final, *, stream):
        self._say("stream_ctc_prefix", slot, final)
        t = self._tokens(slot, 10)
        return [(t, 1.0 if final else 0.0, list(range(len(t))), 0.5)]

    def stream_ctc_prefix_ngram(self, slot, final, *, stream):
        self._say("stream_ctc_prefix_ngram", slot, final)
        t = self._tokens(slot, 10)
        return [(t, 2.0 if final else -1.0, list(range(len(t))), 0.5, -0.25)]

    def stream_prefix(self, slot, *, stream):
        self._say("stream_prefix", slot)
        t = [5] + self._tokens(slot, 10)
        return [(t, -1.5), (t + [7], -2.5)]

    def stream_prefix_ctx(self, slot, final, *, stream):
        self._say("stream_prefix_ctx", slot, final)
        t, c = [5] + self._tokens(slot, 10), 9.0 if final else 6.0
        return [(t, -1.5 + c, c), (t + [7], -2.5, 0.0)]

    def pool_endpoints(self, slots, stream):
        self._say("pool_endpoints", list(slots))
        fired = [s in self.fire and self.n[s] >= 2 for s in slots]
        return np.asarray([[4 * self.n[s], 1, 4 * self.n[s] - 1, 3 if f else 0, 8 if f else 0] for s, f in zip(slots, fired)], np.int32)

    def pool_segment(self, slots, keep_encoder, stream):
        self._say("pool_segment", list(slots), keep_encoder)
        for s in slots:
            self.seg[s], self.n[s] = (self.seg[s][0] + 1, self.frames[s]), 0

    def stream_segment(self, slot):
        self._say("stream_segment", slot)
        return self.seg[slot]

    def stream_frames(self, slot, start, stream):
        self._say("stream_frames", slot, start)
        return torch.zeros(self.frames[slot] - self.seg[slot][1], 256)

    def pool_rescore(self, slots, n_hyp, hyp_lens, hyp_tokens, stream):
        self._say("pool_rescore", list(slots), np.asarray(n_hyp).tolist(), np.asarray(hyp_lens).tolist(), np.asarray(hyp_tokens).tolist())
        nll = np.full((len(slots), int(max(n_hyp))), 1.0, np.float64)
        nll[:, 0] = 9.0
        return nll

    def transducer_align(self, enc_ptr, enc_lens, tokens, token_lens, n, t_max, *, stream):
        self._say("transducer_align", list(enc_lens), np.asarray(tokens).tolist(), list(token_lens), n, t_max)
        return None, np.arange(np.asarray(tokens).shape[1], dtype=np.int32).reshape(1, -1)


def plain(v):
    """A returned value as literals: BeamHypothesis and tensors have no equality of their own."""
    if isinstance(v, BeamHypothesis):
        return ("BeamHypothesis", v.tokens, v.log_prob)
    if isinstance(v, torch.Tensor):
        return ("tensor", tuple(v.shape))
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(*(plain(x) for x in v)) if hasattr(v, "_fields") else type(v)(plain(x) for x in v)
    return v


def refused(call, *args, **kw):
    with pytest.raises(RnntError) as e:
        call(*args, **kw)
    return ("RnntError", str(e.value), e.value.status)


def every_kind_script():
    fake = Engine(fire=(2, 6))
    pool = StreamPool(None, 8, engine=fake, max_beam=4)
    graph, lm = ContextBias([[1, 2], [3]], 3.0), NgramLM(GRAMS, lm_weight=0.25)
    got = []

    def chunk(n):
        return torch.zeros(n, 80)

    def say(label, value):
        got.append((label, len(fake.log), plain(value)))     # with the log's length: where in the engine's log the value was returned
    opens = [dict(), dict(beam_size=4), dict(ctc_prefix_beam=4, endpoint=CFG, on_endpoint="keep"), dict(ctc_prefix_beam=4, context=graph),
             dict(ctc_prefix_beam=4, ngram=lm), dict(ctc_prefix_beam=4, ngram=lm, context=graph),
             dict(prefix_beam=5, endpoint=CFG, on_endpoint="fresh"), dict(prefix_beam=5, prefix_context=graph, keep_frames=True)]
    say("open", [pool.open(**kw) for kw in opens])
    say("open full", refused(pool.open))
    # 1-4: 16 frames to all, a second chunk to 0, 3 and 7, a skipped one to 1, step
    say("feed", [pool.feed(s, chunk(16)) for s in range(8)] + [pool.feed(s, chunk(24)) for s in (0, 3, 7)] + [pool.feed(1, chunk(6))])
    say("step", pool.step())
    # 5: every getter, on its kind and on a wrong one
    say("beams", pool.beams(1))
    say("beams of greedy", refused(pool.beams, 0))
    say("beams of ctc", refused(pool.beams, 2))
    for s in (2, 3, 4, 5):
        say(f"ctc_hyps {s}", [pool.ctc_hyps(s), pool.ctc_hyps(s, final=True)])
    say("ctc_hyps of prefix", refused(pool.ctc_hyps, 6))
    say("ctc_hyps of greedy", refused(pool.ctc_hyps, 0))
    for s in (6, 7):
        say(f"prefix_hyps {s}", [pool.prefix_hyps(s), pool.prefix_hyps(s, final=True), pool.prefix_hyps(s, with_context_scores=True),
                                 pool.prefix_hyps(s, final=True, with_context_scores=True)])
    say("prefix_hyps of ctc", refused(pool.prefix_hyps, 3))
    say("prefix_hyps of beam", refused(pool.prefix_hyps, 1))
    say("endpoints", [pool.endpoints(), pool.endpoints([6]), pool.endpoints([])])
    say("endpoints of a slot without", refused(pool.endpoints, [2, 3]))
    say("frames", pool.frames(7))
    say("frames not kept", refused(pool.frames, 2))
    say("rescore", pool.rescore([7], 0.5, 0.5))
    say("rescore not kept", refused(pool.rescore, [7, 3], 0.5, 0.5))
    say("rescore of greedy", refused(pool.rescore, [0], 0.5, 0.5))
    say("token_times of prefix", refused(pool.token_times, 7))
    say("token_times not kept", refused(pool.token_times, 0))
    say("segments before any", [pool.segments(s) for s in range(8)])
    # 6-7: the second step fires slots 2 (keep) and 6 (fresh)
    say("feed", [pool.feed(s, chunk(16)) for s in range(8)])
    say("step", pool.step())
    say("segments", [pool.segments(s) for s in range(8)])
    say("segments drained", [pool.segments(2), pool.segments(6)])
    # 8: a segment by hand, the encoder restarted
    say("next_segment", pool.next_segment(4, keep_encoder=False))
    say("next_segment with endpoint", pool.next_segment(2))
    # 9: close() steps the queue; slot 0's increment waits for the next step()
    say("feed", [pool.feed(s, chunk(16)) for s in (0, 3, 4, 6)])
    say("close 3", pool.close(3))
    say("closed", [refused(pool.feed, 3, chunk(16)), refused(pool.ctc_hyps, 3), refused(pool.close, 3), refused(pool.next_segment, 3)])
    say("step hands out the carry", pool.step())
    say("step with nothing queued", pool.step())
    # 10: close everything (slot 6 with another fired segment behind it), then its segments
    say("feed", [pool.feed(6, chunk(16))])
    say("close", [pool.close(s) for s in (7, 6, 5, 4, 2, 1, 0)])
    say("segments after close", [pool.segments(6), pool.segments(2)])
    # 11: reopen as another kind
    say("reopen", pool.open(keep_frames=True))
    say("segments of the reopened", pool.segments(0))
    say("feed", [pool.feed(0, chunk(16)), pool.feed(0, chunk(32))])
    say("step", pool.step())
    say("token_times", pool.token_times(0))
    say("frames", pool.frames(0))
    say("open after a close", [pool.open(prefix_beam=5, prefix_context=ContextBias([[4]], 2.0)), pool.open(ctc_prefix_beam=4, ngram=NgramLM(GRAMS, lm_weight=0.75))])
    say("close", [pool.close(0), pool.close(1), pool.close(2)])
    return got, fake.log


RETURNED = [('open', 14, [0, 1, 2, 3, 4, 5, 6, 7]),
 ('open full', 14, ('RnntError', 'stream pool full: all 8 slots are open', None)),
 ('feed', 14, [True, True, True, True, True, True, True, True, True, True, True, False]),
 ('step', 27, {0: [0, 1]}),
 ('beams', 28, [('BeamHypothesis', [1000], -0.5)]),
 ('beams of greedy', 28, ('RnntError', 'slot 0 is not an open beam slot', None)),
 ('beams of ctc', 28, ('RnntError', 'slot 2 is not an open beam slot', None)),
 ('ctc_hyps 2', 30, [[([20], 0.0, [0])], [([20], 1.0, [0])]]),
 ('ctc_hyps 3', 32, [[([30, 31], 0.0, [0, 1])], [([30, 31], 1.0, [0, 1])]]),
 ('ctc_hyps 4', 34, [[([40], -1.0, [0])], [([40], 2.0, [0])]]),
 ('ctc_hyps 5', 36, [[([50], -1.0, [0])], [([50], 2.0, [0])]]),
 ('ctc_hyps of prefix', 36, ('RnntError', 'slot 6 is not an open CTC prefix slot', None)),
 ('ctc_hyps of greedy', 36, ('RnntError', 'slot 0 is not an open CTC prefix slot', None)),
 ('prefix_hyps 6',
  40,
  [[([5, 60], -1.5), ([5, 60, 7], -2.5)],
   [([5, 60], -1.5), ([5, 60, 7], -2.5)],
   [([5, 60], 4.5, 6.0), ([5, 60, 7], -2.5, 0.0)],
   [([5, 60], 7.5, 9.0), ([5, 60, 7], -2.5, 0.0)]]),
 ('prefix_hyps 7',
  44,
  [[([5, 70, 71], 4.5), ([5, 70, 71, 7], -2.5)],
   [([5, 70, 71], 7.5), ([5, 70, 71, 7], -2.5)],
   [([5, 70, 71], 4.5, 6.0), ([5, 70, 71, 7], -2.5, 0.0)],
   [([5, 70, 71], 7.5, 9.0), ([5, 70, 71, 7], -2.5, 0.0)]]),
 ('prefix_hyps of ctc', 44, ('RnntError', 'slot 3 is not an open transducer prefix slot', None)),
 ('prefix_hyps of beam', 44, ('RnntError', 'slot 1 is not an open transducer prefix slot', None)),
 ('endpoints',
  46,
  [{2: Endpoint(rule=0, at_frame=0, frames=4, trailing=1, speech=3), 6: Endpoint(rule=0, at_frame=0, frames=4, trailing=1, speech=3)},
   {6: Endpoint(rule=0, at_frame=0, frames=4, trailing=1, speech=3)},
   {}]),
 ('endpoints of a slot without', 46, ('RnntError', 'slot 3 is not an open slot that detects its endpoint (open(endpoint=EndpointConfig(...)))', -5)),
 ('frames', 47, ('tensor', (10, 256))),
 ('frames not kept', 47, ('RnntError', 'slot 2 is not an open slot that keeps its frames (open(keep_frames=True))', -5)),
 ('rescore', 49, {7: (0, [([70, 71], 7.5, -9.0, -0.75), ([70, 71, 7], -2.5, -1.0, -1.75)])}),
 ('rescore not kept', 49, ('RnntError', 'slot 3 is not an open slot that keeps its frames (open(keep_frames=True))', -5)),
 ('rescore of greedy', 49, ('RnntError', 'slot 0 is not an open CTC prefix or transducer prefix slot', None)),
 ('token_times of prefix', 49, ('RnntError', 'slot 7 is not a greedy slot', None)),
 ('token_times not kept', 49, ('RnntError', 'slot 0 is not an open slot that keeps its frames (open(keep_frames=True))', -5)),
 ('segments before any', 49, [[], [], [], [], [], [], [], []]),
 ('feed', 49, [True, True, True, True, True, True, True, True]),
 ('step', 65, {0: [2]}),
 ('segments',
  65,
  [[],
   [],
   [Segment(index=0, start_frame=0, frames=8, result=[([20, 21], 1.0, [0, 1])], endpoint=Endpoint(rule=3, at_frame=8, frames=8, trailing=1, speech=7))],
   [],
   [],
   [],
   [Segment(index=0, start_frame=0, frames=8, result=[([5, 60, 61], -1.5), ([5, 60, 61, 7], -2.5)], endpoint=Endpoint(rule=3, at_frame=8, frames=8, trailing=1, speech=7))],
   []]),
 ('segments drained', 65, [[], []]),
 ('next_segment', 68, Segment(index=0, start_frame=0, frames=8, result=[([40, 41], 2.0, [0, 1])], endpoint=None)),
 ('next_segment with endpoint',
  72,
  Segment(index=1, start_frame=8, frames=0, result=[([], 1.0, [])], endpoint=Endpoint(rule=0, at_frame=0, frames=0, trailing=1, speech=-1))),
 ('feed', 72, [True, True, True, True]),
 ('close 3', 79, [([30, 31, 32, 33], 1.0, [0, 1, 2, 3])]),
 ('closed',
  79,
  [('RnntError', 'slot 3 is not open', None),
   ('RnntError', 'slot 3 is not an open CTC prefix slot', None),
   ('RnntError', 'slot 3 is not open', None),
   ('RnntError', 'slot 3 is not open', None)]),
 ('step hands out the carry', 79, {0: [3]}),
 ('step with nothing queued', 79, {}),
 ('feed', 79, [True]),
 ('close',
  91,
  [[([5, 70, 71, 72], 7.5), ([5, 70, 71, 72, 7], -2.5)],
   [([5], -1.5), ([5, 7], -2.5)],
   [([50, 51], 2.0, [0, 1])],
   [([40], 2.0, [0])],
   [([], 1.0, [])],
   [('BeamHypothesis', [1000, 1001], -1.0)],
   [0, 1, 2, 3]]),
 ('segments after close',
  91,
  [[Segment(index=1, start_frame=8, frames=8, result=[([5, 60, 61], -1.5), ([5, 60, 61, 7], -2.5)], endpoint=Endpoint(rule=3, at_frame=8, frames=8, trailing=1, speech=7))],
   []]),
 ('reopen', 93, 0),
 ('segments of the reopened', 93, []),
 ('feed', 93, [True, True]),
 ('step', 96, {0: [0, 1]}),
 ('token_times', 99, [(0, 0.02), (0.02, 0.48)]),
 ('frames', 100, ('tensor', (12, 256))),
 ('open after a close', 104, [1, 2]),
 ('close', 107, [[0, 1], [([5], 7.5), ([5, 7], -2.5)], [([], 2.0, [])]])]

LOG = [('reset', 8),
 ('stream_open', 0),
 ('stream_open', 1),
 ('stream_open', 2),
 ('stream_endpoint', 2, (0.5, 1, 0, 0, 6)),
 ('context_set', [[1, 2], [3]], 3.0),
 ('stream_open', 3),
 ('ngram_set', 0.25),
 ('stream_open', 4),
 ('stream_open', 5),
 ('stream_open', 6),
 ('stream_endpoint', 6, (0.5, 1, 0, 0, 6)),
 ('stream_open', 7),
 ('stream_keep_frames', 7, True),
 ('pool_chunk', [0], 16, [0], [0], True),
 ('pool_chunk_beam', [1], 16, [0], [0], 4),
 ('pool_chunk_ctc_prefix', [2], 16, [0], [0], 4, False),
 ('pool_chunk_ctc_prefix', [3], 16, [0], [0], 4, True),
 ('pool_chunk_prefix', [6], 16, [0], [0], 5, 0.3, 0.7),
 ('pool_chunk_prefix_ctx', [7], 16, [0], [0], 5, 0.3, 0.7, True),
 ('pool_chunk_ctc_prefix_ngram', [4], 16, [0], [0], 4, False, True),
 ('pool_chunk_ctc_prefix_ngram', [5], 16, [0], [0], 4, True, True),
 ('pool_chunk', [0], 24, [4], [4], True),
 ('pool_chunk_ctc_prefix', [3], 24, [4], [4], 4, True),
 ('pool_chunk_prefix_ctx', [7], 24, [4], [4], 5, 0.3, 0.7, True),
 ('stream_tokens', 0, 0),
 ('pool_endpoints', [2, 6]),
 ('stream_beam', 1),
 ('stream_ctc_prefix', 2, False),
 ('stream_ctc_prefix', 2, True),
 ('stream_ctc_prefix', 3, False),
 ('stream_ctc_prefix', 3, True),
 ('stream_ctc_prefix_ngram', 4, False),
 ('stream_ctc_prefix_ngram', 4, True),
 ('stream_ctc_prefix_ngram', 5, False),
 ('stream_ctc_prefix_ngram', 5, True),
 ('stream_prefix', 6),
 ('stream_prefix', 6),
 ('stream_prefix_ctx', 6, False),
 ('stream_prefix_ctx', 6, True),
 ('stream_prefix_ctx', 7, False),
 ('stream_prefix_ctx', 7, True),
 ('stream_prefix_ctx', 7, False),
 ('stream_prefix_ctx', 7, True),
 ('pool_endpoints', [2, 6]),
 ('pool_endpoints', [6]),
 ('stream_frames', 7, 0),
 ('stream_prefix_ctx', 7, True),
 ('pool_rescore', [7], [2], [[2, 3]], [[[70, 71, 0], [70, 71, 7]]]),
 ('pool_chunk', [0], 16, [10], [10], True),
 ('pool_chunk_beam', [1], 16, [4], [4], 4),
 ('pool_chunk_ctc_prefix', [2], 16, [4], [4], 4, False),
 ('pool_chunk_ctc_prefix', [3], 16, [10], [10], 4, True),
 ('pool_chunk_prefix', [6], 16, [4], [4], 5, 0.3, 0.7),
 ('pool_chunk_prefix_ctx', [7], 16, [10], [10], 5, 0.3, 0.7, True),
 ('pool_chunk_ctc_prefix_ngram', [4], 16, [4], [4], 4, False, True),
 ('pool_chunk_ctc_prefix_ngram', [5], 16, [4], [4], 4, True, True),
 ('stream_tokens', 0, 2),
 ('pool_endpoints', [2, 6]),
 ('stream_ctc_prefix', 2, True),
 ('pool_segment', [2], True),
 ('stream_segment', 2),
 ('stream_prefix', 6),
 ('pool_segment', [6], False),
 ('stream_segment', 6),
 ('stream_ctc_prefix_ngram', 4, True),
 ('pool_segment', [4], False),
 ('stream_segment', 4),
 ('pool_endpoints', [2]),
 ('stream_ctc_prefix', 2, True),
 ('pool_segment', [2], True),
 ('stream_segment', 2),
 ('pool_chunk', [0], 16, [14], [14], True),
 ('pool_chunk_ctc_prefix', [3], 16, [14], [14], 4, True),
 ('pool_chunk_prefix', [6], 16, [0], [0], 5, 0.3, 0.7),
 ('pool_chunk_ctc_prefix_ngram', [4], 16, [0], [0], 4, False, True),
 ('stream_tokens', 0, 3),
 ('pool_endpoints', [2, 6]),
 ('stream_ctc_prefix', 3, True),
 ('stream_prefix_ctx', 7, True),
 ('pool_chunk_prefix', [6], 16, [4], [4], 5, 0.3, 0.7),
 ('pool_endpoints', [2, 6]),
 ('stream_prefix', 6),
 ('pool_segment', [6], False),
 ('stream_segment', 6),
 ('stream_prefix', 6),
 ('stream_ctc_prefix_ngram', 5, True),
 ('stream_ctc_prefix_ngram', 4, True),
 ('stream_ctc_prefix', 2, True),
 ('stream_beam', 1),
 ('stream_tokens', 0, 0),
 ('stream_open', 0),
 ('stream_keep_frames', 0, True),
 ('pool_chunk', [0], 16, [0], [0], True),
 ('pool_chunk', [0], 32, [4], [4], True),
 ('stream_tokens', 0, 0),
 ('stream_tokens', 0, 0),
 ('stream_frames', 0, 0),
 ('transducer_align', [12], [[0, 1]], [2], 1, 12),
 ('stream_frames', 0, 0),
 ('context_set', [[4]], 2.0),
 ('stream_open', 1),
 ('ngram_set', 0.75),
 ('stream_open', 2),
 ('stream_tokens', 0, 0),
 ('stream_prefix_ctx', 1, True),
 ('stream_ctc_prefix_ngram', 2, True)]


def test_every_kind_in_one_pool():
    got, log = every_kind_script()
    for have, want in zip(got, RETURNED):
        assert have == want
    assert len(got) == len(RETURNED)
    for k, (have, want) in enumerate(zip(log, LOG)):
        assert have == want, f"engine call {k}"
    assert len(log) == len(LOG)


# ---- open() refusals ---------------------------------------------------------------------------------------------------------------
G1, G2 = ContextBias([[1, 2]], 2.0), ContextBias([[3]], 4.0)
LM1, LM2 = NgramLM(GRAMS, lm_weight=0.25), NgramLM(GRAMS[:2], lm_weight=0.75)
NAN = float("nan")

# (pool keywords, open() calls that succeed first, the refused open(), its message)
REFUSALS = [
    (dict(max_beam=4), [], dict(prefix_beam=4, beam_size=2),
     'stream pool: prefix_beam, beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ctc_prefix_beam=4),
     'stream pool: prefix_beam, beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [], dict(prefix_beam=4, context=G1),
     'stream pool: context biases the CTC prefix search only (ctc_prefix_beam)'),
    (dict(max_beam=4), [], dict(prefix_beam=17),
     'stream pool: prefix_beam 17 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(prefix_beam=-1),
     'stream pool: prefix_beam -1 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ctc_weight=-0.1),
     'stream pool: weights -0.1 / 0.7 (negative, or both zero)'),
    (dict(max_beam=4), [], dict(prefix_beam=4, transducer_weight=-1.0),
     'stream pool: weights 0.3 / -1.0 (negative, or both zero)'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ctc_weight=0.0, transducer_weight=0.0),
     'stream pool: weights 0.0 / 0.0 (negative, or both zero)'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ctc_weight=NAN),
     'stream pool: weights nan / 0.7 (negative, or both zero)'),
    (dict(vocab_size=600), [], dict(prefix_beam=4),
     'stream pool: prefix_beam 4 outside [1, min(16, vocabulary 600)] or vocabulary > 512'),
    (dict(vocab_size=8), [], dict(prefix_beam=9),
     'stream pool: prefix_beam 9 outside [1, min(16, vocabulary 8)] or vocabulary > 512'),
    (dict(), [], dict(beam_size=4),
     'stream pool: beam_size 4 outside [0, min(max_beam 0, 16)] or vocabulary 412 > 512'),
    (dict(max_beam=8), [], dict(beam_size=9),
     'stream pool: beam_size 9 outside [0, min(max_beam 8, 16)] or vocabulary 412 > 512'),
    (dict(max_beam=32), [], dict(beam_size=17),
     'stream pool: beam_size 17 outside [0, min(max_beam 32, 16)] or vocabulary 412 > 512'),
    (dict(max_beam=4, vocab_size=600), [], dict(beam_size=4),
     'stream pool: beam_size 4 outside [0, min(max_beam 4, 16)] or vocabulary 600 > 512'),
    (dict(max_beam=4), [], dict(beam_size=-1),
     'stream pool: beam_size -1 outside [0, min(max_beam 4, 16)] or vocabulary 412 > 512'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=4, beam_size=2),
     'stream pool: beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=17),
     'stream pool: ctc_prefix_beam 17 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=-1),
     'stream pool: ctc_prefix_beam -1 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(context=G1),
     'stream pool: context needs ctc_prefix_beam'),
    (dict(vocab_size=600), [], dict(ctc_prefix_beam=4),
     'stream pool: ctc_prefix_beam 4 outside [1, min(16, vocabulary 600)] or vocabulary > 512'),
    (dict(vocab_size=8), [], dict(ctc_prefix_beam=9),
     'stream pool: ctc_prefix_beam 9 outside [1, min(16, vocabulary 8)] or vocabulary > 512'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, context=G1)], dict(ctc_prefix_beam=4, context=G2),
     'stream pool: another context graph is in use by an open slot (one graph per pool at a time)'),
    (dict(max_beam=4), [], dict(on_endpoint='keep'),
     'stream pool: on_endpoint needs endpoint (an EndpointConfig)'),
    (dict(max_beam=4), [], dict(endpoint=CFG, on_endpoint='both'),
     "stream pool: on_endpoint 'both' is not None, 'keep' or 'fresh'"),
    (dict(max_beam=4), [], dict(ngram=LM1),
     'stream pool: ngram needs ctc_prefix_beam'),
    (dict(max_beam=4), [], dict(beam_size=2, ngram=LM1),
     'stream pool: ngram needs ctc_prefix_beam'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ngram=LM1),
     'stream pool: ngram needs ctc_prefix_beam'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, ngram=LM1)], dict(ctc_prefix_beam=4, ngram=LM2),
     'stream pool: another n-gram model is in use by an open slot (one model per pool at a time)'),
    (dict(max_beam=4), [], dict(prefix_context=G2),
     'stream pool: prefix_context needs prefix_beam'),
    (dict(max_beam=4), [], dict(beam_size=2, prefix_context=G2),
     'stream pool: prefix_context needs prefix_beam'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=4, prefix_context=G2),
     'stream pool: prefix_context needs prefix_beam'),
    (dict(max_beam=4), [dict(prefix_beam=4, prefix_context=G1)], dict(prefix_beam=4, prefix_context=G2),
     'stream pool: another context graph is in use by an open slot (one graph per pool at a time)'),
    (dict(max_beam=4), [dict(prefix_beam=4, prefix_context=G1)], dict(ctc_prefix_beam=4, context=G2),
     'stream pool: another context graph is in use by an open slot (one graph per pool at a time)'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, context=G1)], dict(prefix_beam=4, prefix_context=G2),
     'stream pool: another context graph is in use by an open slot (one graph per pool at a time)'),
    (dict(max_beam=4), [dict(), dict(beam_size=2)], dict(),
     'stream pool full: all 2 slots are open'),
    (dict(max_beam=4), [dict(), dict()], dict(ctc_prefix_beam=4, context=G1, ngram=LM1),
     'stream pool full: all 2 slots are open'),
    (dict(max_beam=4), [], dict(ngram=LM1, on_endpoint='both'),
     'stream pool: ngram needs ctc_prefix_beam'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, ngram=LM1)], dict(ctc_prefix_beam=4, ngram=LM2, on_endpoint='keep'),
     'stream pool: another n-gram model is in use by an open slot (one model per pool at a time)'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, ngram=LM1)], dict(ctc_prefix_beam=17, ngram=LM2),
     'stream pool: another n-gram model is in use by an open slot (one model per pool at a time)'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, ngram=LM1)], dict(ngram=LM2, prefix_context=G1),
     'stream pool: ngram needs ctc_prefix_beam'),
    (dict(max_beam=4), [], dict(on_endpoint='both'),
     "stream pool: on_endpoint 'both' is not None, 'keep' or 'fresh'"),
    (dict(max_beam=4), [], dict(on_endpoint='keep', prefix_context=G1),
     'stream pool: on_endpoint needs endpoint (an EndpointConfig)'),
    (dict(max_beam=4), [], dict(prefix_context=G1, context=G2),
     'stream pool: prefix_context needs prefix_beam'),
    (dict(max_beam=4), [dict(prefix_beam=4, prefix_context=G1)], dict(prefix_beam=17, prefix_context=G2),
     'stream pool: another context graph is in use by an open slot (one graph per pool at a time)'),
    (dict(max_beam=4), [], dict(prefix_beam=4, beam_size=2, context=G1),
     'stream pool: prefix_beam, beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [], dict(prefix_beam=17, context=G1),
     'stream pool: context biases the CTC prefix search only (ctc_prefix_beam)'),
    (dict(max_beam=4), [], dict(prefix_beam=17, ctc_weight=-1.0),
     'stream pool: prefix_beam 17 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(prefix_beam=4, ctc_prefix_beam=17, beam_size=2),
     'stream pool: prefix_beam, beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=17, beam_size=2),
     'stream pool: beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [dict(ctc_prefix_beam=4, context=G1)], dict(ctc_prefix_beam=17, context=G2),
     'stream pool: ctc_prefix_beam 17 outside [1, min(16, vocabulary 412)] or vocabulary > 512'),
    (dict(max_beam=4), [], dict(context=G1, beam_size=-1),
     'stream pool: context needs ctc_prefix_beam'),
    (dict(max_beam=4), [], dict(ctc_prefix_beam=4, beam_size=9),
     'stream pool: beam_size and ctc_prefix_beam are mutually exclusive'),
    (dict(max_beam=4), [dict(), dict()], dict(beam_size=9),
     'stream pool: beam_size 9 outside [0, min(max_beam 4, 16)] or vocabulary 412 > 512'),
    (dict(max_beam=4), [dict(), dict()], dict(prefix_beam=4, ctc_weight=-1.0),
     'stream pool: weights -1.0 / 0.7 (negative, or both zero)'),
    (dict(max_beam=4), [dict(), dict()], dict(endpoint=CFG, on_endpoint='both'),
     "stream pool: on_endpoint 'both' is not None, 'keep' or 'fresh'"),
]


def open_slots(pool):
    """the slots feed() takes (a 6-frame chunk is skipped: nothing is queued)"""
    out = []
    for s in range(pool.n):
        try:
            assert pool.feed(s, torch.zeros(6, 80)) is False
            out.append(s)
        except RnntError as e:
            assert str(e) == f"slot {s} is not open"
    return out


@pytest.mark.parametrize("pool_kw,before,bad,message", REFUSALS)
def test_open_refusal(pool_kw, before, bad, message):
    fake = Engine()
    pool = StreamPool(None, 2, engine=fake, **pool_kw)
    for kw in before:
        pool.open(**kw)
    free, asked, graph, model = list(pool._free), list(fake.log), pool._context, pool._ngram
    with pytest.raises(RnntError) as e:
        pool.open(**bad)
    assert str(e.value) == message and e.value.status is None
    assert pool._free == free and open_slots(pool) == [s for s in range(2) if s not in free], "no slot was taken"
    assert fake.log == asked and pool._context is graph and pool._ngram is model, "nothing was asked of the engine"


# the library refuses: (the method that raises, the open(), what the engine is asked by three attempts in a row, whether the graph and
# the model accepted before the refusal stay the pool's)
LIBRARY_REFUSALS = [
    ('context_set', dict(ctc_prefix_beam=4, context=G1),
     [[('context_set', [[1, 2]], 2.0)], [('context_set', [[1, 2]], 2.0)], [('context_set', [[1, 2]], 2.0)]], (False, False)),
    ('context_set', dict(prefix_beam=4, prefix_context=G1),
     [[('context_set', [[1, 2]], 2.0)], [('context_set', [[1, 2]], 2.0)], [('context_set', [[1, 2]], 2.0)]], (False, False)),
    ('ngram_set', dict(ctc_prefix_beam=4, context=G1, ngram=LM1),
     [[('context_set', [[1, 2]], 2.0), ('ngram_set', 0.25)], [('ngram_set', 0.25)], [('ngram_set', 0.25)]], (True, False)),
    ('stream_open', dict(ctc_prefix_beam=4, context=G1, ngram=LM1),
     [[('context_set', [[1, 2]], 2.0), ('ngram_set', 0.25), ('stream_open', 0)], [('stream_open', 0)], [('stream_open', 0)]], (True, True)),
    ('stream_open', dict(),
     [[('stream_open', 0)], [('stream_open', 0)], [('stream_open', 0)]], (False, False)),
    ('stream_keep_frames', dict(beam_size=4, keep_frames=True),
     [[('stream_open', 0), ('stream_keep_frames', 0, True)], [('stream_open', 0), ('stream_keep_frames', 0, True)], [('stream_open', 0), ('stream_keep_frames', 0, True)]], (False, False)),
    ('stream_endpoint', dict(prefix_beam=4, prefix_context=G1, keep_frames=True, endpoint=CFG, on_endpoint='keep'),
     [[('context_set', [[1, 2]], 2.0), ('stream_open', 0), ('stream_keep_frames', 0, True), ('stream_endpoint', 0, (0.5, 1, 0, 0, 6))], [('stream_open', 0), ('stream_keep_frames', 0, True), ('stream_endpoint', 0, (0.5, 1, 0, 0, 6))], [('stream_open', 0), ('stream_keep_frames', 0, True), ('stream_endpoint', 0, (0.5, 1, 0, 0, 6))]], (True, False)),
]


@pytest.mark.parametrize("method,bad,asked,kept", LIBRARY_REFUSALS)
def test_open_refused_by_the_library(method, bad, asked, kept):
    fake = Engine(refuse=method)
    pool = StreamPool(None, 2, engine=fake, max_beam=4)
    logs = []
    for _ in range(3):                                        # more refusals than the pool has slots
        del fake.log[:]
        with pytest.raises(RnntError) as e:
            pool.open(**bad)
        assert str(e.value) == f"rnnt_{method}: refused (status -1)" and e.value.status == ERR_ARG
        assert pool._free == [0, 1] and open_slots(pool) == [], "no slot was taken"
        logs.append(list(fake.log))
    assert logs == asked
    assert (pool._context is not None, pool._ngram is not None) == kept
    fake.refuse = None
    assert pool.open(**bad) == 0 and pool.open() == 1
