"""N-gram shallow fusion in the CTC prefix beam search, host side (no GPU): the new C-ABI symbols, the model builder and walker
(rnnt_ngram_walk_host) against the f64 restatement testing.ngram_ref with exact equality, every refusal of the builder,
NgramLM.from_arpa, the pure C++ search rnnt_ctc_prefix_beam_ngram_host against testing.ctc_prefix_beam_ngram_ref, and StreamPool over
a recording fake engine.  Tolerances and the gap condition: ngram_cases.py."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_vr_amd.lib as rlib
import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, RnntError, ctc_prefix_beam_host, ctc_prefix_beam_ngram_host, ngram_walk_host
from ctc_vr_amd.ngram import NgramLM
from ctc_vr_amd.online_rnnt_model import ContextBias, StreamPool, pool_plan
import ngram_cases as N
from test_stream_pool_ctc_prefix_cpu import FakeEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnnt_ngram_set", "rnnt_ngram_walk_host", "rnnt_ngram_score", "rnnt_ctc_prefix_beam_logprobs_ngram", "rnnt_ctc_prefix_beam_decode_ngram",
       "rnnt_ctc_prefix_beam_ngram_host", "rnnt_pool_ctc_prefix_logprobs_ngram", "rnnt_pool_chunk_ctc_prefix_ngram", "rnnt_stream_get_ctc_prefix_ngram")
CASES = N.search_cases()


def test_new_symbols_in_header_signatures_and_library():
    src = open(os.path.join(ROOT, "include", "rnnt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = rlib.load()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, f"{name} is not declared in include/rnnt_hip.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in rlib.SIGNATURES, f"{name} is missing from lib.SIGNATURES"
        res, args = rlib.SIGNATURES[name]
        assert res is rlib.c_i32 and len(args) == n_args, f"{name}: header has {n_args} arguments, SIGNATURES {len(args)}"
        assert hasattr(lib, name), f"librnnt_hip.so does not export {name}"
    assert lib.rnnt_abi_version() == 3


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _strings(name, vocab, blank):
    tk = N.real_tokens(vocab, blank)
    if name == "deep":
        r = np.random.default_rng(5)
        return [r.choice(tk, 12).tolist() for _ in range(40)] + [[tk[0], tk[1], tk[2], tk[3], tk[0], tk[4], tk[3]]]
    return [list(q) for n in range(5) for q in itertools.product(tk, repeat=n)]


@pytest.mark.parametrize("name", sorted(N.MODELS))
def test_walk_equals_the_restatement(name):
    vocab, blank = 6, 0
    model = N.MODELS[name](vocab, blank)
    ref = N.ref_model(model, vocab, blank)
    backoffs = unk = 0
    for toks in _strings(name, vocab, blank):
        sc, st, eos, nodes = ngram_walk_host(model, vocab, blank, toks)
        rs, rt, re_ = ref.walk(toks)
        assert sc.tolist() == rs and st.tolist() == rt and eos == re_, toks
        assert nodes == len(model.ngrams) + 1
        unk += any(s == 0 for s in rt)
        backoffs += any(ref.fail[a] != 0 for a in rt)
    assert ref.start == (0 if name in ("uni", "tri_pruned", "deep") else ref.next[0][vocab])
    if name == "uni":
        assert unk > 0, "no walk met a token without a unigram"
    if name in ("tri_pruned", "deep"):
        assert backoffs > 0


def test_models_are_what_they_claim():
    ref = N.ref_model(N.tri_pruned(6, 0), 6, 0)
    assert ref.fail[ref.node[(1, 2, 3)]] == ref.node[(3,)] and (2, 3) not in ref.node        # the fail arc skips the bigram level
    ref = N.ref_model(N.deep(6, 0), 6, 0)
    node, chain = ref.node[(1, 2, 3, 4, 1)], []
    while node:
        chain.append(node)
        node = ref.fail[node]
    assert len(chain) == 5, "four back-offs before the root's own miss"
    ref = N.ref_model(N.bi(6, 0), 6, 0)
    assert ref.has_eos and ref.start != 0 and ref.W[ref.node[(7,)]] == 0.5 * N.bi(6, 0).ngrams[6][1]
    assert N.ref_model(N.uni(6, 0), 6, 0).eos(0) == 0.0
    z = N.ref_model(N.weight0(6, 0), 6, 0)
    assert not any(z.W) and not any(z.B) and z.U == 0.0


GOOD = [((1,), -1.0, -0.5), ((2,), -2.0, -0.25), ((1, 2), -0.5, 0.0)]


@pytest.mark.parametrize("what,grams,kw", [
    ("empty n-gram", GOOD + [((), -1.0, 0.0)], {}),
    ("nine tokens", [((1,), -1.0, 0.0)] + [((1,) * k, -1.0, 0.0) for k in range(2, 10)], {}),
    ("token outside", GOOD + [((8,), -1.0, 0.0)], {}),
    ("negative token", GOOD + [((-1,), -1.0, 0.0)], {}),
    ("the blank", GOOD + [((0,), -1.0, 0.0)], {}),
    ("BOS not first", GOOD + [((1, 6), -1.0, 0.0)], {}),
    ("EOS not last", GOOD + [((7,), -1.0, 0.0), ((7, 1), -1.0, 0.0)], {}),
    ("prefix not listed", GOOD + [((3, 1), -1.0, 0.0)], {}),
    ("prefix listed later", [((1, 2), -1.0, 0.0), ((1,), -1.0, 0.0)], {}),
    ("duplicate", GOOD + [((2,), -1.0, 0.0)], {}),
    ("infinite logp", GOOD + [((3,), -math.inf, 0.0)], {}),
    ("nan bow", GOOD + [((3,), -1.0, math.nan)], {}),
    ("negative weight", GOOD, dict(lm_weight=-0.5)),
    ("infinite unk", GOOD, dict(unk_logp=-math.inf)),
    ("nan bonus", GOOD, dict(length_bonus=math.nan)),
])
def test_model_refusals(what, grams, kw):
    ngram_walk_host(NgramLM(GOOD), 6, 0, [1, 2])
    with pytest.raises(RnntError) as e:
        ngram_walk_host(NgramLM(grams, **kw), 6, 0, [1, 2])
    assert e.value.status == ERR_ARG, what
    with pytest.raises(RnntError):
        ctc_prefix_beam_ngram_host(np.zeros((1, 2, 6), np.float32), [2], 0, 2, ngram=NgramLM(grams, **kw))


def test_model_node_limit_and_allowed_forms():
    lib, n = rlib.load(), (1 << 22)
    z = np.zeros(n, np.int32)
    d = np.zeros(n, np.float64)
    p = lambda a: a.ctypes.data_as(rlib.c_vp)
    assert lib.rnnt_ngram_walk_host(n, p(z), p(z), p(d), p(d), 1.0, 0.0, -1.0, 6, 0, 0, None, None, None, None, None) == ERR_ARG
    # [BOS] alone and [BOS, EOS] are allowed; a walk over the blank or a pseudo-token is not
    sc, st, eos, nodes = ngram_walk_host(NgramLM([((6,), -1.0, -0.5), ((6, 7), -2.0, 0.0)], lm_weight=1.0), 6, 0, [])
    assert nodes == 3 and eos == -2.0
    for bad in ([0], [6], [7], [-1]):
        with pytest.raises(RnntError):
            ngram_walk_host(NgramLM(GOOD), 6, 0, bad)


ARPA = """
\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99 <s> -0.5
-1.0 a -0.25
-0.75 b
-2.0 zzz -0.1
-1.5 </s>

\\2-grams:
-0.5 <s> a -0.125
-0.25 a b
-0.3 a zzz
-0.6 b </s>

\\3-grams:
-0.1 <s> a b
-0.2 a zzz b

\\end\\
"""


def test_from_arpa():
    ln10 = math.log(10.0)
    lm = NgramLM.from_arpa(ARPA, {"a": 1, "b": 2, "<s>": 6, "</s>": 7}, lm_weight=0.25)
    assert lm.lm_weight == 0.25 and lm.length_bonus == 0.0 and lm.unk_logp == math.log(1e-10)
    assert lm.ngrams == [((6,), -99 * ln10, -0.5 * ln10), ((1,), -1.0 * ln10, -0.25 * ln10), ((2,), -0.75 * ln10, 0.0), ((7,), -1.5 * ln10, 0.0),
                         ((6, 1), -0.5 * ln10, -0.125 * ln10), ((1, 2), -0.25 * ln10, 0.0), ((2, 7), -0.6 * ln10, 0.0),
                         ((6, 1, 2), -0.1 * ln10, 0.0)], "orders ascending; zzz and what holds it dropped; a missing back-off is 0"
    sc, st, eos, nodes = ngram_walk_host(lm, 6, 0, [1, 2])
    assert nodes == 9 and st.tolist() == [5, 8] and eos == 0.25 * (-0.6 * ln10)      # (<s>, a, b) backs off to (b), then (b, </s>)
    # another word list: whatever holds an unknown word goes
    lm = NgramLM.from_arpa(ARPA, {"b": 2, "zzz": 3, "<s>": 6, "</s>": 7})
    assert [g[0] for g in lm.ngrams] == [(6,), (2,), (3,), (7,), (2, 7)]


# ---- the search ------------------------------------------------------------------------------------------------------------------
def host(case, raw=False):
    lp, lens, blank, beam, phrases, score, model = case
    return ctc_prefix_beam_ngram_host(lp, lens, blank, beam, phrases, score, model, raw=raw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_search_equals_the_restatement(name):
    got, raw = host(CASES[name], raw=True)
    N.assert_same(got, N.reference_of(CASES[name]), name)
    N.assert_zero_fill(raw)


def test_cases_are_what_they_claim():
    st = {name: {} for name in CASES}
    res = {name: N.reference_of(case, st[name]) for name, case in CASES.items()}
    for name in CASES:
        assert N.gap_ok(st[name]), (name, st[name])
    assert len(res["beam_sixteen"][0]) == 16
    m = N.ref_model(CASES["ragged_length_zero"][6], 7, 0)
    assert res["ragged_length_zero"][1] == [([], m.eos(m.start), [], 0.0, m.eos(m.start))] and m.eos(m.start) != 0.0
    assert any(h[3] != 0.0 for r in res["graph_and_model"] for h in r) and any(h[4] != 0.0 for r in res["graph_and_model"] for h in r)
    assert all(len(r) == 1 for r in res["uni_beam_one"])
    # the end term is added without a re-sort, so a list need not descend; the running scores do
    run = N.reference_of(CASES["bi_beam_three"], finalize=False)
    assert [h[1] for h in run[0]] == sorted((h[1] for h in run[0]), reverse=True)
    for (tok, sc, _, _, ls), (_, fsc, _, _, fls) in zip(run[0], res["bi_beam_three"][0]):
        ref = N.ref_model(CASES["bi_beam_three"][6], 7, 0)
        steps, states, eos = ref.walk(tok)
        want = 0.0
        for x in steps:
            want += x
        assert ls == want and fls == want + eos


def test_model_changes_the_result():
    """a model that is silently ignored would pass every comparison without it"""
    case = CASES["model_changes_the_best"]
    with_lm, plain = host(case), ctc_prefix_beam_host(*case[:6])
    assert with_lm[0][0][0] != plain[0][0][0]
    assert max(with_lm[0], key=lambda h: h[1])[0] != max(plain[0], key=lambda h: h[1])[0]
    assert any(h[4] != 0.0 for h in with_lm[0])


def test_weight_zero_equals_the_plain_search():
    case = CASES["weight0"]
    (got, raw), (plain, praw) = host(case, raw=True), ctc_prefix_beam_host(*case[:6], raw=True)
    assert [h[:4] for r in got for h in r] == [h for r in plain for h in r]
    for a, b in zip(raw[:6], praw):
        assert (a == b).all()
    assert not raw[6].any()
    # and no model at all through the new entry point is the old entry point
    none = ctc_prefix_beam_ngram_host(*case[:6], None, raw=True)[1]
    assert all((a == b).all() for a, b in zip(none[:6], praw)) and not none[6].any()


# ---- pool_plan and StreamPool over a recording fake engine -----------------------------------------------------------------------
def test_plan_gives_model_slots_calls_of_their_own():
    ctc = {1: (10, False), 2: (10, False), 3: (10, True), 4: (4, False)}
    prefix = {5: (5, 0.3, 0.7)}
    queue, offs = [(s, 16) for s in range(6)], {s: 8 * s for s in range(6)}
    calls, _, index = pool_plan(queue, offs, {0: 0}, ctc, prefix, {2, 3})
    assert calls == [(16, [0], [0], 0, "greedy", False, None), (16, [4], [32], 4, "ctc_prefix", False, None), (16, [1], [8], 10, "ctc_prefix", False, None),
                     (16, [5], [40], 5, "prefix", False, (0.3, 0.7)), (16, [2], [16], 10, "ctc_prefix_ngram", False, None),
                     (16, [3], [24], 10, "ctc_prefix_ngram", True, None)]
    assert index == [(0, 0), (2, 0), (4, 0), (5, 0), (1, 0), (3, 0)]
    for ngram in (None, set(), {7}):
        assert pool_plan(queue, offs, {0: 0}, ctc, prefix, ngram) == pool_plan(queue, offs, {0: 0}, ctc, prefix)
    assert pool_plan(queue, offs, {0: 0}, ctc, None, {2})[0][-1] == (16, [2], [16], 10, "ctc_prefix_ngram", False)


class NgramFake(FakeEngine):
    def __init__(self):
        super().__init__()
        self.models, self.ngram_reads = [], []

    def ngram_set(self, ngram):
        self.models.append(ngram)

    def pool_chunk_ctc_prefix_ngram(self, slots, ptr, length, offsets, required, beam_size=10, use_context=False, use_ngram=True, stream=None):
        assert ptr != 0 and beam_size > 0 and use_ngram
        self.calls.append(("ctc_prefix_ngram", list(slots), int(length), list(offsets), list(required), int(beam_size), bool(use_context)))
        for s in slots:
            self.ctc[s].append(10 * s + len(self.ctc[s]))
        return ((length - 3) // 2 + 1 - 3) // 2 + 1

    def stream_ctc_prefix_ngram(self, slot, final=False, raw=False, stream=None):
        self.ngram_reads.append((slot, bool(final)))
        t = list(self.ctc[slot])
        return [(t, 2.0 if final else -1.0, list(range(len(t))), 0.5, -0.25)]


def test_stream_pool_routes_model_slots():
    fake = NgramFake()
    pool = StreamPool(None, 4, engine=fake)
    a, b = NgramLM(GOOD), NgramLM(GOOD[:2])
    bias = ContextBias([[1, 2]], 2.0)
    s0 = pool.open(ctc_prefix_beam=4, ngram=a)
    with pytest.raises(RnntError):
        pool.open(ctc_prefix_beam=4, ngram=b)                  # a second model while a slot that fuses one is open
    assert fake.opened == [0] and fake.models == [a], "a refused open() takes no slot and uploads nothing"
    s1 = pool.open(ctc_prefix_beam=4)
    s2 = pool.open(ctc_prefix_beam=4, ngram=a, context=bias)
    s3 = pool.open(ctc_prefix_beam=4, context=bias)
    assert (s0, s1, s2, s3) == (0, 1, 2, 3) and fake.models == [a] and len(fake.graphs) == 1
    for s in range(4):
        assert pool.feed(s, torch.zeros(16, 80))
    assert pool.step() == {}
    assert fake.calls == [("ctc_prefix", [1], 16, [0], [0], 4, False), ("ctc_prefix", [3], 16, [0], [0], 4, True),
                          ("ctc_prefix_ngram", [0], 16, [0], [0], 4, False), ("ctc_prefix_ngram", [2], 16, [0], [0], 4, True)]
    assert pool.ctc_hyps(s0) == [([0], -1.0, [0])] and pool.ctc_hyps(s1) == [([10], 0.0, [0])]
    assert pool.close(s2) == [([20], 2.0, [0])] and pool.close(s0) == [([0], 2.0, [0])]
    assert fake.ngram_reads == [(0, False), (2, True), (0, True)] and fake.reads == [(1, False)]
    assert pool.open(ctc_prefix_beam=4, ngram=b) == 0 and fake.models == [a, b]      # no such slot left: the model is replaced
    for bad in (dict(ngram=a), dict(beam_size=2, ngram=a), dict(prefix_beam=4, ngram=a)):
        with pytest.raises(RnntError):
            pool.open(**bad)


def test_stream_pool_without_model_slots_calls_what_it_called():
    """the same script through a pool whose engine knows nothing of the model: every recorded call is today's"""
    def script(fake):
        pool = StreamPool(None, 4, engine=fake, max_beam=4)
        bias = ContextBias([[7, 8]], 3.0)
        slots = [pool.open(), pool.open(beam_size=4), pool.open(ctc_prefix_beam=10, context=bias), pool.open(ctc_prefix_beam=10)]
        for s in slots:
            pool.feed(s, torch.zeros(16, 80))
        pool.feed(slots[2], torch.zeros(24, 80))
        out = [pool.step(), pool.ctc_hyps(slots[2]), pool.close(slots[3]), pool.close(slots[2])]
        return out, fake.calls, fake.reads, fake.graphs, fake.opened
    out, calls, reads, graphs, opened = script(FakeEngine())
    assert script(NgramFake())[:5] == (out, calls, reads, graphs, opened)
    assert calls == [("greedy", [0], 16, [0], [0], 0, False), ("beam", [1], 16, [0], [0], 4, False), ("ctc_prefix", [3], 16, [0], [0], 10, False),
                     ("ctc_prefix", [2], 16, [0], [0], 10, True), ("ctc_prefix", [2], 24, [4], [4], 10, True)]
    assert reads == [(2, False), (3, True), (2, True)]
