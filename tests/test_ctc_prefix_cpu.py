"""CTC prefix beam search with a context graph, host side (no GPU): the graph builder and walker (rnnt_context_walk_host /
rnnt_context_dump_host) against node tables and forward_one_step traces recorded from the reference's ContextGraph, and the pure C++
search rnnt_ctc_prefix_beam_host against the reference's recorded n-best lists and against the library's own definition
ctc_vr_amd.testing.ctc_prefix_beam_ref on crafted cases with exact ties.  Tolerances and the gap condition: ctc_prefix_cases.py."""
import math

import numpy as np
import pytest

import ctc_vr_amd.testing as T
from ctc_vr_amd.lib import ERR_ARG, RnntError, context_dump_host, context_walk_host, ctc_prefix_beam_host
import ctc_prefix_cases as C

GOLD = C.golden_cases()
CRAFTED = C.crafted_cases()
TABLES = ("token", "node_score", "output_score", "is_end", "fail", "output")


def host(case, raw=False):
    lp, lens, blank, beam, phrases, score = case
    return ctc_prefix_beam_host(lp, lens, blank, beam, phrases, score, raw=raw)


# ---- graph ------------------------------------------------------------------------------------------------------------------------
def test_graph_tables_equal_the_reference():
    """every score is a small multiple of 2.5: equality is exact"""
    z = C.load("graph")
    got = context_dump_host(C.phrases_of(z), float(z["context_score"]))
    ref = T.context_graph_ref(C.phrases_of(z), float(z["context_score"]))
    mine = {"token": ref.token, "node_score": ref.node_score, "output_score": ref.output_score, "is_end": ref.is_end, "fail": ref.fail,
            "output": ref.output}
    for k in TABLES:
        assert got[k].tolist() == z[k].tolist(), k
        assert [float(v) for v in mine[k]] == [float(v) for v in z[k]], f"restatement: {k}"
    # what the fixture is for: duplicates share nodes, a phrase ending on an existing node does not mark it, output scores accumulate
    assert len(z["token"]) < 1 + int(z["phrase_lens"].sum())
    assert (z["output_score"] > z["node_score"]).any() and (z["output"] >= 0).any() and (z["fail"] > 0).any()


def test_graph_walks_equal_the_reference():
    z = C.load("graph")
    phrases, score = C.phrases_of(z), float(z["context_score"])
    ref = T.context_graph_ref(phrases, score)
    off = z["walk_off"]
    assert (z["walk_score"] < 0).any(), "a walk leaves a partial match through a fail arc"
    assert (z["walk_final"] < 0).any(), "a walk ends inside a match"
    for i, (a, b) in enumerate(zip(off, off[1:])):
        toks = z["walk_tok"][a:b].tolist()
        sc, st, fin = context_walk_host(phrases, score, toks)
        assert sc.tolist() == z["walk_score"][a:b].tolist() and st.tolist() == z["walk_state"][a:b].tolist() and fin == z["walk_final"][i], i
        rs, rt, rf = ref.walk(toks)
        assert rs == sc.tolist() and rt == st.tolist() and rf == fin, f"restatement: walk {i}"


def test_graph_of_the_search_fixture():
    """prefix of another phrase, one-token phrase, repeated node: the graph the biased search cases use"""
    z = C.load("v412_blank5_beam4")
    got = context_dump_host(C.phrases_of(z), 3.0)
    assert got["token"].tolist() == [-1, 7, 8, 9, 8, 9, 10, 11, 9]
    assert got["is_end"].tolist() == [0, 0, 0, 1, 0, 0, 0, 1, 1]          # [7, 8] ends on a node [7, 8, 9] created: not an end
    assert got["output_score"].tolist() == [0, 0, 0, 12, 0, 3, 0, 12, 3]
    assert got["fail"].tolist() == [0, 0, 4, 5, 0, 8, 0, 0, 0] and got["output"].tolist() == [-1, -1, -1, 8, -1, 8, -1, -1, -1]


@pytest.mark.parametrize("phrases", [[[]], [[1, 2], []], [[-1]], [[1] * 5000]])
def test_graph_refusals(phrases):
    with pytest.raises(RnntError) as e:
        context_dump_host(phrases, 1.0)
    assert e.value.status == ERR_ARG
    with pytest.raises(RnntError):
        context_walk_host(phrases, 1.0, [1])


def test_graph_node_limit():
    chain = lambda n: [[1 + (i % 7) for i in range(n)]]
    assert len(context_dump_host(chain(4095), 1.0)["token"]) == 4096
    with pytest.raises(RnntError):
        context_dump_host(chain(4096), 1.0)


def test_search_refuses_phrases_outside_the_vocabulary():
    lp = np.zeros((1, 2, 6), np.float32)
    for phrases in ([[6]], [[0]], [[]]):                                  # beyond the vocabulary, the blank, empty
        with pytest.raises(RnntError):
            ctc_prefix_beam_host(lp, [2], 0, 2, phrases, 1.0)


# ---- search -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLD))
def test_host_search_equals_the_reference(name):
    case, want = GOLD[name]
    got, raw = host(case, raw=True)
    C.assert_same(got, want, name)
    C.assert_zero_fill(raw)
    C.assert_same(C.reference_of(case), want, f"restatement: {name}")


@pytest.mark.parametrize("name", sorted(CRAFTED))
def test_host_search_equals_python_restatement(name):
    got, raw = host(CRAFTED[name], raw=True)
    C.assert_same(got, C.reference_of(CRAFTED[name]), name)
    C.assert_zero_fill(raw)


def test_cases_are_what_they_claim():
    st = {name: {} for name in list(CRAFTED) + list(GOLD)}
    res = {name: C.reference_of(case, st[name]) for name, case in CRAFTED.items()}
    for name, (case, _) in GOLD.items():
        C.reference_of(case, st[name])
        assert st[name].get("nonzero_gap", math.inf) >= C.MIN_GAP and not st[name].get("top_ties") and not st[name].get("prune_ties"), name
    for name in CRAFTED:
        assert st[name].get("nonzero_gap", math.inf) >= C.MIN_GAP, name
    frames = sum(GOLD["v412_blank5_beam4_plain"][0][1])
    assert st["v412_blank5_beam4_plain"]["both_live"] > frames // 2         # "P and P + u both live" in most frames
    assert st["equal_frame_values"]["top_ties"] >= 3 and st["equal_frame_values"]["prune_ties"] >= 3
    first = C.reference_of((CRAFTED["equal_frame_values"][0], [1], 0, 3, None, 0.0))[0]
    assert [(h[0], h[1]) for h in first] == [([], -1.5), ([1], -1.5), ([2], -1.5)]   # the lowest indices, in insertion order
    assert st["ties_at_the_cut"]["cut_ties"] >= 2 and st["ties_at_the_cut"]["prune_ties"] >= 1
    first = C.reference_of((CRAFTED["ties_at_the_cut"][0], [1], 0, 2, None, 0.0))[0]
    assert [h[0] for h in first] == [[1], [2]] and first[0][1] == first[1][1]       # token 3 is cut from the top list at a tie
    assert any(h[1] == -math.inf for h in res["minus_inf"][0]) and any(len(h[2]) < len(h[0]) for r in res["minus_inf"] for h in r)
    assert [(h[0], h[1], h[2]) for h in res["length_zero"][0]] == [([], 0.0, [])] and res["length_zero_ctx"][0][0][1] == 0.0
    assert all(len(r) == 1 for r in res["beam_one"])
    assert st["stale_times"]["stale_times"] == 1 and res["stale_times"][0][0][0] == [1, 3, 1] and res["stale_times"][0][0][2] == [1, 3, 4]
    assert len(res["beam_sixteen"][0]) == 16
    assert st["rebuilt_parent_a"]["rebuilt_parent"] >= 1 and st["rebuilt_parent_b"]["rebuilt_parent"] >= 1


@pytest.mark.parametrize("name", ["v412_blank5_beam4", "v8_beam8"])
def test_context_changes_the_result(name):
    """a graph that is silently ignored would pass every comparison without it"""
    plain, ctx = host(GOLD[f"{name}_plain"][0]), host(GOLD[f"{name}_ctx"][0])
    assert [h[0] for h in plain[0]] != [h[0] for h in ctx[0]]
    assert all(h[3] == 0.0 for r in plain for h in r) and any(h[3] != 0.0 for r in ctx for h in r)


def test_host_search_refusals():
    lp, ok = np.zeros((2, 3, 6), np.float32), dict(enc_lens=[3, 2], blank=0, beam_size=2)
    ctc_prefix_beam_host(lp, **ok)
    for bad in (dict(enc_lens=[4, 2]), dict(enc_lens=[-1, 2]), dict(beam_size=0), dict(beam_size=7), dict(beam_size=17)):
        with pytest.raises(RnntError) as e:
            ctc_prefix_beam_host(lp, **{**ok, **bad})
        assert e.value.status == ERR_ARG
    with pytest.raises(RnntError):
        ctc_prefix_beam_host(np.zeros((1, 1, 513), np.float32), [1], 0, 2)
