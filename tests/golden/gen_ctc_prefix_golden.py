"""Generates tests/golden/ctc_prefix_*.npz: inputs and outputs of the reference's ctc_prefix_beam_search
(wenet/transformer/search.py:125-247) and ContextGraph (wenet/utils/context_graph.py) on seeded cases.  Run where the read-only
reference is present (the build container), on the CPU; never imported by tests, bench or the product.  Only data goes into the
fixtures.

The graph is built by the reference from a phrase file and a symbol table: a temporary file with one code point per token id.

A seed is kept only if ctc_vr_amd.testing.ctc_prefix_beam_ref, alone, gives every prune gap and every top-(beam + 1) gap >= MIN_GAP
(a condition on the inputs, as MIN_GAP in tests/prefix_cases.py), and the restatement must then reproduce the reference's tokens and
times exactly.

Search fixtures (ragged lists padded with zeros, hypothesis i of row b valid for i < n_hyp[b]):
  lp [B, T, V] f32, lens [B], blank, beam, phrase_lens / phrase_tokens (concatenated), context_score
  for tag in ("plain", "ctx"): {tag}_n_hyp [B], {tag}_len [B, beam], {tag}_tok / {tag}_times [B, beam, T], {tag}_score [B, beam] f64
Graph fixture: phrase_lens / phrase_tokens, context_score, node tables in node-id order (token, node_score, output_score, is_end,
  fail, output with -1 for none), and walks: walk_tok / walk_off (case i = [off[i], off[i + 1])) -> walk_score f64, walk_state,
  walk_final [n_walks] f64.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
MIN_GAP = 1e-6
BASE = 0x4E00     # token id v <-> code point BASE + v


def reference():
    from _ref_loader import load_reference
    load_reference()
    from wenet.transformer.search import ctc_prefix_beam_search
    from wenet.utils.context_graph import ContextGraph
    return ctc_prefix_beam_search, ContextGraph


def ref_graph(ContextGraph, phrases, vocab, score):
    table = {chr(BASE + v): v for v in range(vocab)}
    with tempfile.NamedTemporaryFile("w", suffix=".txt", encoding="utf-8", delete=False) as f:
        for ph in phrases:
            f.write("".join(chr(BASE + v) for v in ph) + "\n")
    try:
        g = ContextGraph(f.name, table, None, score)
    finally:
        os.unlink(f.name)
    assert g.context_list == [list(ph) for ph in phrases]
    return g


def node_tables(g):
    nodes, queue = {0: g.root}, [g.root]
    while queue:
        n = queue.pop(0)
        for c in n.next.values():
            nodes[c.id] = c
            queue.append(c)
    order = [nodes[i] for i in range(g.num_nodes + 1)]
    return {"token": np.array([n.token for n in order], np.int32), "node_score": np.array([n.node_score for n in order], np.float64),
            "output_score": np.array([n.output_score for n in order], np.float64), "is_end": np.array([n.is_end for n in order], np.int32),
            "fail": np.array([n.fail.id for n in order], np.int32),
            "output": np.array([-1 if n.output is None else n.output.id for n in order], np.int32)}


def make_lp(seed, B, T, V, hot, boost):
    import torch
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    x[..., hot] += np.float32(boost)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def pack(results, B, beam, T):
    n_hyp, ln = np.zeros(B, np.int32), np.zeros((B, beam), np.int32)
    tok, tim, sc = np.zeros((B, beam, T), np.int32), np.zeros((B, beam, T), np.int32), np.zeros((B, beam), np.float64)
    for b, r in enumerate(results):
        n_hyp[b] = len(r.nbest)
        for i, (p, s, t) in enumerate(zip(r.nbest, r.nbest_scores, r.nbest_times)):
            assert len(p) == len(t)
            ln[b, i], sc[b, i] = len(p), s
            tok[b, i, :len(p)], tim[b, i, :len(t)] = list(p), list(t)
    return {"n_hyp": n_hyp, "len": ln, "tok": tok, "times": tim, "score": sc}


def search_case(name, B, T, V, lens, blank, beam, hot, phrases, score, boost=4.0):
    import torch
    import ctc_vr_amd.testing as TT
    search, ContextGraph = reference()
    gref = TT.context_graph_ref(phrases, score)
    for seed in range(1000):
        lp = make_lp(seed, B, T, V, hot, boost)
        mine = {tag: [TT.ctc_prefix_beam_ref(lp[b], lens[b], blank, beam, g) for b in range(B)] for tag, g in (("plain", None), ("ctx", gref))}
        if min(min(pg, tg) for rows in mine.values() for _, pg, tg in rows) >= MIN_GAP:
            break
    else:
        raise SystemExit(f"{name}: no seed satisfies the gap condition")
    out = {"lp": lp, "lens": np.array(lens, np.int32), "blank": np.int32(blank), "beam": np.int32(beam), "seed": np.int32(seed),
           "phrase_lens": np.array([len(p) for p in phrases], np.int32), "phrase_tokens": np.array([t for p in phrases for t in p], np.int32),
           "context_score": np.float64(score)}
    for tag in ("plain", "ctx"):
        g = ref_graph(ContextGraph, phrases, V, score) if tag == "ctx" else None
        res = search(torch.from_numpy(lp), torch.tensor(lens), beam, g, blank)
        for b in range(B):
            hyps = mine[tag][b][0]
            assert [h[0] for h in hyps] == [list(p) for p in res[b].nbest], (name, tag, b)
            assert [h[2] for h in hyps] == [list(t) for t in res[b].nbest_times], (name, tag, b)
            assert np.allclose([h[1] for h in hyps], res[b].nbest_scores, rtol=0, atol=1e-9)
        out.update({f"{tag}_{k}": v for k, v in pack(res, B, beam, T).items()})
    path = os.path.join(HERE, f"ctc_prefix_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "seed", seed, os.path.getsize(path), "bytes;",
          "ctx differs from plain:", not np.array_equal(out["plain_tok"], out["ctx_tok"]))


def graph_case():
    _, ContextGraph = reference()
    long_phrase = [20 + (i * 7) % 23 for i in range(30)]
    phrases = [[1, 2, 3, 4], [2, 3, 4, 5], [3, 4], [2, 3], [1, 2, 3, 4], [4], [6, 1, 2], [1, 2], long_phrase, long_phrase[10:14], [3, 4]]
    score = 2.5
    g = ref_graph(ContextGraph, phrases, 64, score)
    walks = [[1, 2, 3, 4, 5], [6, 1, 2, 3, 9], [1, 2, 3, 5], [2, 3, 4], [6, 1, 2, 3, 4, 5, 4, 4], long_phrase, long_phrase[:17] + [1, 2, 3],
             long_phrase[8:15], [9, 9, 9], [4], [6, 1], [1, 2, 3], []]
    sc, st, fin = [], [], []
    for w in walks:
        state = g.root
        for tok in w:
            s, state = g.forward_one_step(state, tok)
            sc.append(s); st.append(state.id)
        fin.append(g.finalize(state)[0])
    out = node_tables(g)
    out.update({"phrase_lens": np.array([len(p) for p in phrases], np.int32), "phrase_tokens": np.array([t for p in phrases for t in p], np.int32),
                "context_score": np.float64(score), "walk_tok": np.array([t for w in walks for t in w], np.int32),
                "walk_off": np.cumsum([0] + [len(w) for w in walks]).astype(np.int64), "walk_score": np.array(sc, np.float64),
                "walk_state": np.array(st, np.int32), "walk_final": np.array(fin, np.float64)})
    path = os.path.join(HERE, "ctc_prefix_graph.npz")
    np.savez_compressed(path, **out)
    print("graph", len(out["token"]), "nodes", os.path.getsize(path), "bytes")


def main():
    phrases = [[7, 8, 9], [8, 9, 10, 11], [9], [7, 8]]
    search_case("v412_blank5_beam4", 2, 24, 412, [24, 17], 5, 4, [5, 7, 8, 9, 10, 11], phrases, 3.0)
    search_case("v412_blank0_beam1", 2, 24, 412, [24, 17], 0, 1, [0, 7, 8, 9, 10, 11], phrases, 3.0)
    search_case("v8_beam8", 1, 12, 8, [12], 0, 8, [0], [[1, 2], [2, 3, 4], [5]], 3.0, boost=1.0)
    graph_case()


if __name__ == "__main__":
    main()
