"""Taxon placement support without a device: the two host references against each other and against the per-taxon
reference, ``regraft`` against the cluster definition, the C declaration against the binding, the argument checks
and the views of ``SupertreeScore`` on hand-filled counts."""

import re
from pathlib import Path

import numpy as np
import placement_reference as pr
import pytest
import score_reference as sr
import taxon_triplet_reference as xr

from spectralclustersupertree_amd import SupertreeScore, _native, score_supertree
from spectralclustersupertree_amd.tree import make_tree

KEYS = ("pl_trees", "pl_total", "pl_source", "pl_super", "pl_shared", "placement_distance")


def _tips(sup) -> list[str]:
    return [v.name for v in sr._preorder(sup) if v.is_tip()]


@pytest.fixture(scope="module")
def cases():
    rs = np.random.RandomState(43)
    out = []
    for _ in range(300):
        sup, trees = sr.random_case(rs)
        out.append((sup, trees, pr.brute_force(sup, trees, _tips(sup))))
    return out


def test_by_hand():
    # S = ((a,b),c), T = ((a,c),b), x = a: the one triple is ac|b in T; S says ab|c where a is (nodes 1, 2, 3: a's
    # parent, a, its sibling b), ac|b on the edge above c, and bc|a on the edge above the root
    ref = pr.brute_force(make_tree("((a,b),c);"), [make_tree("((a,c),b);")], ["a"])
    assert ref["pl_trees"].tolist() == [1] and ref["pl_total"].tolist() == [1] and ref["pl_source"].tolist() == [1]
    assert ref["pl_super"].tolist() == [[1, 1, 1, 1, 1]]
    assert ref["pl_shared"].tolist() == [[0, 0, 0, 0, 1]]
    assert ref["placement_distance"].tolist() == [[2, 2, 2, 2, 0]]


def test_the_references_agree_on_random_cases(cases):
    seen = 0
    for i, (sup, trees, brute) in enumerate(cases):
        rec = pr.recurrence(sup, trees, _tips(sup))
        for k in KEYS:
            assert rec[k].dtype == np.int64 and np.array_equal(brute[k], rec[k]), (i, k)
        seen += int(brute["pl_shared"].max(initial=0) > 0)
    assert seen > 100  # (the cases are not all trivial)


def test_a_subset_of_the_queries_gives_its_rows(cases):
    for i, (sup, trees, brute) in enumerate(cases[:60]):
        tips = _tips(sup)
        rows = list(range(len(tips)))[::2][::-1]
        rec = pr.recurrence(sup, trees, [tips[r] for r in rows])
        for k in KEYS:
            assert np.array_equal(rec[k], brute[k][rows]), (i, k)


def test_the_own_node_holds_the_per_taxon_counts(cases):
    for i, (sup, trees, brute) in enumerate(cases):
        tx = xr.brute_force(sup, trees)
        nodes = sr._preorder(sup)
        own = [k for k, v in enumerate(nodes) if v.is_tip()]
        index = {id(v): k for k, v in enumerate(nodes)}
        q = np.arange(len(own))
        assert np.array_equal(brute["pl_shared"][q, own], tx["tx_shared"]), i
        assert np.array_equal(brute["pl_super"][q, own], tx["tx_super"]), i
        for k in ("trees", "total", "source"):
            assert np.array_equal(brute[f"pl_{k}"], tx[f"tx_{k}"]), (i, k)
        for x, v in enumerate(own):  # the sibling and a parent with two children hold them too
            parent = nodes[v].parent
            if parent is not None and len(parent.children) == 2:
                for u in (index[id(parent)], *(index[id(c)] for c in parent.children)):
                    assert brute["pl_shared"][x, u] == tx["tx_shared"][x], (i, x, u)
                    assert brute["pl_super"][x, u] == tx["tx_super"][x], (i, x, u)


def _score(sup, **extra):
    n = len(sr._preorder(sup))
    one = np.ones(2, dtype=np.int64)
    z = np.zeros(n, dtype=np.int64)
    return SupertreeScore(sup, np.array([5, 4]), one, one, one, z, z.copy(), {}, **extra)


def test_regraft_gives_the_clusters_of_the_definition(cases):
    moved = 0
    for i, (sup, _, _) in enumerate(cases[:120]):
        res = _score(sup)
        tips = _tips(sup)
        nodes = sr._preorder(sup)
        for x in tips:
            for v in range(len(nodes)):
                got = res.regraft(x, v)
                got_nodes = sr._preorder(got)
                # (the definition drops x's own singleton unless v is x; a tree always has it)
                want = pr.regrafted_clusters(sup, x, v) | {frozenset([x])}
                assert set(sr._leaf_sets(got_nodes).values()) == want, (i, x, v)
                assert got_nodes[0].parent is None and all(c.parent is w for w in got_nodes for c in w.children)
                # (the node the tip left is suppressed: no more unary nodes than before)
                assert sum(len(w.children) == 1 for w in got_nodes) <= sum(len(w.children) == 1 for w in nodes)
                moved += set(sr._leaf_sets(got_nodes).values()) != set(sr._leaf_sets(nodes).values())
        assert _tips(sup) == tips  # (the supertree itself is left alone)
    assert moved > 1000
    res = _score(make_tree("(((a,b),c),(d,e));"))
    assert res.regraft("a", 7).get_newick() == "((b,c),((d,a),e));"
    assert res.regraft("a", 6).get_newick() == "((b,c),((d,e),a));"
    assert res.regraft(0, 2).get_newick() == "(((b,a),c),(d,e));"     # node 2 = (a,b): above its remaining child
    assert res.regraft("a", 3).get_newick() == "(((a,b),c),(d,e));"   # its own node: unchanged
    assert res.regraft("a", 0).get_newick() == "(((b,c),(d,e)),a);"
    for bad in (lambda: res.regraft("zz", 1), lambda: res.regraft(5, 1), lambda: res.regraft("a", 9)):
        with pytest.raises(ValueError):
            bad()


def test_the_header_declares_the_symbol_and_the_binding_holds_it():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int scs_score_placements\(([^;]*)\);", header)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = _native.SIGNATURES["scs_score_placements"]
    assert restype is _native.C.c_int and len(params) == len(argtypes) == 14
    ctype = {"scs_ctx *": _native.C.c_void_p, "const scs_tables *": _native.C.c_void_p,
             "int32_t ": _native.C.c_int32, "const int32_t *": _native.C.c_void_p, "int64_t *": _native.C.c_void_p}
    names = []
    for p, arg in zip(params, argtypes):
        name = re.search(r"(\w+)$", p).group(1)
        assert ctype[p[: -len(name)]] is arg, p
        names.append(name)
    assert names == ["ctx", "sources", "n_nodes", "parent", "taxon", "max_batch_trees", "max_lds_bytes", "n_queries",
                     "queries", "pl_trees", "pl_total", "pl_source", "pl_super", "pl_shared"]
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header


def test_bad_placements_are_refused_before_any_device_work():
    sup = make_tree("(((a,b),c),(d,e));")
    trees = [make_tree("((a,c),b);")]
    for bad, text in ((["a", "zz"], "'zz' is not in the supertree"), (["a", "b", "a"], "more than once"),
                      (-1, "negative"), ("a", "list of taxon names or a count"), (True, "list of taxon names")):
        with pytest.raises(ValueError, match=text):
            score_supertree(sup, trees, placements=bad, device=object())


SUP = "(((a,b),c),(d,e));"


def _counts() -> dict:
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    # nodes: 0 root, 1 ((a,b),c), 2 (a,b), 3 a, 4 b, 5 c, 6 (d,e), 7 d, 8 e; queries b and d
    return {"taxa": ["a", "b", "c", "d", "e"], "pl_taxa": i64(1, 3), "pl_trees": i64(2, 1), "pl_total": i64(9, 6),
            "pl_source": i64(6, 4),
            "pl_super": np.array([[9, 8, 6, 6, 6, 7, 5, 4, 4], [6, 5, 4, 3, 3, 3, 4, 4, 4]], dtype=np.int64),
            "pl_shared": np.array([[1, 2, 3, 3, 3, 6, 2, 1, 1], [2, 1, 1, 0, 0, 0, 3, 3, 3]], dtype=np.int64)}


def test_views_refuse_without_the_counts():
    plain = _score(make_tree(SUP))
    assert plain.pl_shared is None and plain.pl_taxa is None
    for call in (lambda: plain.placement_distance, plain.best_placements, plain.placement_table):
        with pytest.raises(ValueError, match=r"score_supertree\(\.\.\., placements=\.\.\.\)"):
            call()


def test_views_of_the_counts():
    res = _score(make_tree(SUP), **_counts())
    assert res.placement_distance.tolist() == [[13, 10, 6, 6, 6, 1, 7, 8, 8], [6, 7, 6, 7, 7, 7, 2, 2, 2]]
    best = res.best_placements()
    assert best[0] == {"taxon": 1, "name": "b", "trees": 2, "node": 4, "distance": 6, "best_node": 5,
                       "best_distance": 1, "improvement": 5}
    # d: nodes 6, 7 and 8 tie at the minimum, and its own node 7 is among them
    assert best[1] == {"taxon": 3, "name": "d", "trees": 1, "node": 7, "distance": 2, "best_node": 7,
                       "best_distance": 2, "improvement": 0}
    assert res.placement_table() == ("taxon\tname\ttrees\tnode\tdistance\tbest_node\tbest_distance\timprovement\n"
                                     "1\tb\t2\t4\t6\t5\t1\t5\n"
                                     "3\td\t1\t7\t2\t7\t2\t0\n")
    # without the own node among the minima the lowest preorder index wins
    counts = _counts()
    counts["pl_shared"][1, 7] = 2
    assert _score(make_tree(SUP), **counts).best_placements()[1]["best_node"] == 6


def test_the_other_tables_do_not_change():
    plain, full = _score(make_tree(SUP)), _score(make_tree(SUP), **_counts())
    assert plain.table() == full.table()
