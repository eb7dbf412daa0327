"""Cases of the n-gram shallow-fusion tests (test_ngram_cpu.py, test_ngram.py, test_stream_pool_ngram.py): small back-off models
and search cases whose expected result is the library's own definition, ctc_vr_amd.testing.ctc_prefix_beam_ngram_ref.

A model is built for a vocabulary and a blank (BOS = vocab, EOS = vocab + 1).  A search case is (lp [B, T, V] float32, lens, blank,
beam, phrases or None, context_score, model).

SCORE_TOL and MIN_GAP are those of ctc_prefix_cases.py: the n-gram term adds only exact additions that every side does in the same
order, so the bound on the totals is the bound on the log-adds.  Every seeded case is chosen on the CPU by the restatement alone: no
finite tie and no non-zero gap below MIN_GAP among the top values and among the totals INCLUDING the n-gram term."""
import itertools
import math

import numpy as np

import ctc_vr_amd.testing as T
from ctc_vr_amd.ngram import NgramLM
import ctc_prefix_cases as C

SCORE_TOL, MIN_GAP = C.SCORE_TOL, C.MIN_GAP


def _values(seed, n):
    r = np.random.default_rng(seed)
    return (-r.uniform(0.1, 5.0, n)).tolist(), (-r.uniform(0.0, 2.0, n)).tolist()


def _lm(strings, seed, **kw):
    logp, bow = _values(seed, len(strings))
    return NgramLM([(s, p, b) for s, p, b in zip(strings, logp, bow)], **kw)


def real_tokens(vocab, blank):
    return [t for t in range(vocab) if t != blank]


def uni(vocab, blank, **kw):
    """order 1, no BOS or EOS; the last real token has no unigram (the unk path)"""
    return _lm([(t,) for t in real_tokens(vocab, blank)[:-1]], 11, **{"lm_weight": 0.7, "length_bonus": 0.25, **kw})


def bi(vocab, blank, **kw):
    """order 2 with BOS and EOS; every second bigram over the first four real tokens"""
    bos, eos, tk = vocab, vocab + 1, real_tokens(vocab, blank)
    s = [(bos,)] + [(t,) for t in tk] + [(eos,)]
    s += [(bos, t) for t in tk[:2]] + [(bos, eos)]
    s += [p for i, p in enumerate(itertools.product(tk[:4], repeat=2)) if i % 2 == 0] + [(t, eos) for t in tk[1:3]]
    return _lm(s, 12, **{"lm_weight": 0.5, "length_bonus": 0.0, **kw})


def tri_pruned(vocab, blank, **kw):
    """order 3, not suffix-closed: (a, b, c) is listed, its suffix (b, c) is not, so fail[(a, b, c)] = (c): the arc skips a level"""
    a, b, c, d = real_tokens(vocab, blank)[:4]
    s = [(a,), (b,), (c,), (d,), (a, b), (b, a), (c, a), (a, b, c), (a, b, a), (b, a, b), (c, a, b)]
    return _lm(s, 13, **{"lm_weight": 0.6, "length_bonus": 0.1, **kw})


def deep(vocab, blank, **kw):
    """order 5 over four tokens: every suffix of (a, b, c, d, a) is listed, so a miss there backs off four times"""
    tk = real_tokens(vocab, blank)[:4]
    a, b, c, d = tk
    forced = {(a, b, c, d, a)[i:j] for i in range(5) for j in range(i + 1, 6)}
    r = np.random.default_rng(14)
    s, have = [], {()}
    for order in range(1, 6):
        for q in itertools.product(tk, repeat=order):
            if q[:-1] in have and (order <= 2 or q in forced or r.random() < 0.35):
                have.add(q)
                s.append(q)
    return _lm(s, 14, **{"lm_weight": 0.5, "length_bonus": 0.05, **kw})


def weight0(vocab, blank):
    return bi(vocab, blank, lm_weight=0.0, length_bonus=0.0)


def order3(tokens, vocab, seed, **kw):
    """an order-3 model with BOS and EOS over the given tokens: every unigram, a seeded third of the bigrams, a tenth of their extensions"""
    r = np.random.default_rng(seed)
    tokens = list(tokens)
    s = [(vocab,)] + [(t,) for t in tokens] + [(vocab + 1,)]
    pairs = [(a, b) for a in tokens for b in tokens if r.random() < 0.3]
    s += [(vocab, t) for t in tokens[:3]] + pairs + [(t, vocab + 1) for t in tokens[:3]]
    s += [(a, b, c) for a, b in pairs for c in tokens if r.random() < 0.1]
    return _lm(s, seed, **{"lm_weight": 0.6, "length_bonus": 0.5, **kw})


MODELS = {"uni": uni, "bi": bi, "tri_pruned": tri_pruned, "deep": deep, "weight0": weight0}


def ref_model(model, vocab, blank):
    return T.ngram_ref(model.ngrams, vocab, blank, model.lm_weight, model.length_bonus, model.unk_logp)


def reference_of(case, stats=None, finalize=True):
    """the restatement per utterance: [(tokens, score, times, context score, n-gram score)]"""
    lp, lens, blank, beam, phrases, score, model = case
    g = T.context_graph_ref(phrases, score) if phrases else None
    m = ref_model(model, lp.shape[2], blank) if model is not None else None
    return [T.ctc_prefix_beam_ngram_ref(lp[b], lens[b], blank, beam, g, m, stats, finalize)[0] for b in range(len(lens))]


def gap_ok(st):
    return st.get("nonzero_gap", math.inf) >= MIN_GAP and not st.get("top_ties") and not st.get("prune_ties")


def _seeded(B, T_, V, lens, blank, beam, phrases, score, model, also=None):
    """log-softmax rows of the first seed whose case meets the gap condition (and `also`), judged by the restatement alone"""
    for seed in range(1000):
        case, st = (C._rows(seed, B, T_, V), lens, blank, beam, phrases, score, model), {}
        res = reference_of(case, st)
        if gap_ok(st) and (also is None or also(case, res)):
            return case
    raise AssertionError("no seed satisfies the gap condition")


def _flips(case, res):
    """the best hypothesis with the model is another token string than the best without it"""
    plain = reference_of(case[:6] + (None,))
    return max(res[0], key=lambda h: h[1])[0] != max(plain[0], key=lambda h: h[1])[0] and res[0][0][0] != plain[0][0][0]


def search_cases():
    c = {}
    c["uni_beam_one"] = _seeded(1, 7, 6, [7], 2, 1, None, 0.0, uni(6, 2))
    c["bi_beam_three"] = _seeded(1, 9, 7, [9], 0, 3, None, 0.0, bi(7, 0))
    c["tri_pruned_beam_five"] = _seeded(1, 9, 8, [9], 0, 5, None, 0.0, tri_pruned(8, 0))
    c["deep_beam_five"] = _seeded(1, 9, 6, [9], 0, 5, None, 0.0, deep(6, 0))
    c["beam_sixteen"] = _seeded(2, 6, 40, [6, 5], 39, 16, [[3, 4], [4]], 0.75, bi(40, 39))
    c["ragged_length_zero"] = _seeded(3, 9, 7, [9, 0, 6], 0, 5, None, 0.0, bi(7, 0))
    c["graph_and_model"] = _seeded(3, 9, 7, [9, 4, 6], 0, 5, [[1, 2], [2, 3, 1], [2], [1, 2]], 1.0, tri_pruned(7, 0))
    c["rebuilt_parent_a"] = (C._rows(1745, 1, 8, 4), [8], 0, 2, None, 0.0, uni(4, 0, lm_weight=0.3))
    c["rebuilt_parent_b"] = (C._rows(29300, 1, 8, 4), [8], 0, 2, None, 0.0, uni(4, 0, lm_weight=0.3))
    c["weight0"] = c["bi_beam_three"][:6] + (weight0(7, 0),)
    c["model_changes_the_best"] = _seeded(1, 6, 6, [6], 0, 3, None, 0.0, uni(6, 0, lm_weight=1.5), also=_flips)
    return c


def assert_same(got, want, what=""):
    """got / want [(tokens, score, times, context score, n-gram score)] per utterance: tokens, times, order, context score and
    n-gram score exact, totals within SCORE_TOL"""
    C.assert_same(got, want, what)
    for b, (g, w) in enumerate(zip(got, want)):
        for i, (x, y) in enumerate(zip(g, w)):
            assert x[4] == y[4], f"{what} row {b} hyp {i}: n-gram score {x[4]!r} != {y[4]!r}"


def assert_zero_fill(raw):
    C.assert_zero_fill(raw[:6])
    nh, ls = raw[0], raw[6]
    for b in range(len(nh)):
        assert not ls[b, nh[b]:].any()
