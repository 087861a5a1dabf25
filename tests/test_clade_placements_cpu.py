"""The two host forms of the clade placement support (``tests/clade_placement_reference.py``) against each other,
against the taxon placement reference and closed forms; the clade selection rule and ``regraft_clade`` (no GPU)."""

import re
from pathlib import Path

import clade_placement_reference as cr
import numpy as np
import placement_reference as pr
import pytest
import score_reference as sr

from spectralclustersupertree_amd import _native
from spectralclustersupertree_amd.score import SupertreeScore, _check_clade_placements, select_clades, supertree_arrays
from spectralclustersupertree_amd.tree import make_tree

N_CASES = 200


@pytest.fixture(scope="module")
def cases():
    """200 random cases (polytomies, unary nodes, partial coverage, extra taxa), every non-root node queried, with
    the brute force of each."""
    rs = np.random.RandomState(23)
    out = []
    while len(out) < N_CASES:
        sup, trees = sr.random_case(rs, n_taxa=int(rs.randint(2, 10)))
        nodes = sr._preorder(sup)
        queries = list(range(1, len(nodes)))
        out.append((sup, trees, queries, cr.brute_force(sup, trees, queries)))
    return out


def _differences(ref, queries):
    own = np.arange(len(queries))
    return (ref["cp_super"] - ref["cp_super"][own, queries][:, None],
            ref["cp_shared"] - ref["cp_shared"][own, queries][:, None])


def _agree(sup, trees, queries, ref) -> bool:
    """Identity 2: what the brute force says a move changes is what rescoring the edited tree says; and the values at
    the clade's own place are what the sources cut in two at the clade leave of the supertree's triplet terms."""
    edit = cr.edit_and_rescore(sup, trees, queries)
    d_super, d_shared = _differences(ref, queries)
    own = np.arange(len(queries))
    return (np.array_equal(d_super, edit["d_super"]) and np.array_equal(d_shared, edit["d_shared"])
            and np.array_equal(ref["cp_super"][own, queries], edit["own_super"])
            and np.array_equal(ref["cp_shared"][own, queries], edit["own_shared"])
            and np.array_equal(ref["cp_source"], edit["own_source"]))


def test_the_two_forms_agree_on_every_entry(cases):
    crossed = moved = 0
    for n, (sup, trees, queries, ref) in enumerate(cases):
        assert _agree(sup, trees, queries, ref), n
        crossed += int((ref["cp_trees"] > 0).sum())
        d_super, d_shared = _differences(ref, queries)
        moved += int(np.count_nonzero(d_super) + np.count_nonzero(d_shared))
    assert crossed > 1000 and moved > 10000  # (the cases are not trivial)


def test_the_composed_form_agrees_with_the_brute_force(cases):
    for n, (sup, trees, queries, ref) in enumerate(cases):
        got = cr.composed(sup, trees, queries)
        for k in cr.KEYS:
            assert np.array_equal(got[k], ref[k]), (n, k)


def test_a_tip_query_is_a_taxon_placement(cases):
    seen = 0
    for n, (sup, trees, queries, ref) in enumerate(cases):
        nodes = sr._preorder(sup)
        tips = [q for q in queries if nodes[q].is_tip()]
        if not tips:
            continue
        want = pr.brute_force(sup, trees, [nodes[q].name for q in tips])
        rows = [queries.index(q) for q in tips]
        for k in cr.KEYS:
            assert np.array_equal(ref[k][rows], want[k.replace("clade_placement", "placement").replace("cp_", "pl_")]), \
                (n, k)
        seen += len(tips)
    assert seen > 500


def test_entries_that_are_no_move_hold_the_own_value(cases):
    for n, (sup, trees, queries, ref) in enumerate(cases):
        nodes = sr._preorder(sup)
        parent = pr._parents(nodes)
        sets = sr._leaf_sets(nodes)
        for i, q in enumerate(queries):
            same = set(cr.subtree(parent, q))
            up = parent[q]
            if len(nodes[up].children) == 2:  # the parent and the sibling
                same |= {up, *(k for k in range(len(nodes)) if parent[k] == up)}
            while up >= 0 and sets[id(nodes[up])] == sets[id(nodes[q])]:  # unary ancestors
                same.add(up)
                up = parent[up]
            for v in same:
                assert ref["cp_super"][i, v] == ref["cp_super"][i, q], (n, q, v)
                assert ref["cp_shared"][i, v] == ref["cp_shared"][i, q], (n, q, v)


def test_total_is_the_closed_form(cases):
    for n, (sup, trees, queries, ref) in enumerate(cases):
        n_trees, total = cr.total_closed_form(sup, trees, queries)
        assert ref["cp_trees"].tolist() == n_trees and ref["cp_total"].tolist() == total, n
        assert (ref["cp_source"] <= ref["cp_total"]).all() and (ref["cp_super"] <= ref["cp_total"][:, None]).all()
        assert (ref["cp_shared"] <= np.minimum(ref["cp_super"], ref["cp_source"][:, None])).all()


@pytest.mark.parametrize("defect", ["ancestors", "two_in_clade"])
def test_a_planted_defect_is_caught(cases, defect):
    """The comparison of the two forms bites: a brute force that forgets to take the clade out of the clusters above
    its old place, or that leaves out the triples with two taxa in the clade, no longer agrees with rescoring."""
    caught = 0
    for sup, trees, queries, _ in cases[:40]:
        caught += not _agree(sup, trees, queries, cr.brute_force(sup, trees, queries, defect=defect))
    assert caught >= 10, caught


def test_clade_selection_rule():
    #  0 root; 1 (a,b); 4 ((c,d),e); 5 (c,d); 9 ((f,g),(h,i)); 10 (f,g); 13 (h,i); 16 j
    sup = make_tree("((a,b),((c,d),e),((f,g),(h,i)),j);")
    parent, _, tips = supertree_arrays(sup)
    assert tips == list("abcdefghij")
    inst = np.array([0.5, 0.5, 0.9, 0.1, 0.5, 0.8, 0.2, 0.5, 0.5, 1.0])
    held = np.ones(10, dtype=np.int64)
    # means: (a,b) .5, (c,d) .5, ((c,d),e) .5, (f,g) .5, (h,i) .5, ((f,g),(h,i)) .5: the larger clade first, then the
    # lower index; nested and containing nodes are skipped
    assert select_clades(10, parent, inst, held, 64).tolist() == [9, 4, 1]
    assert select_clades(2, parent, inst, held, 64).tolist() == [9, 4]
    assert select_clades(10, parent, inst, held, 3).tolist() == [4, 1, 10, 13]
    assert select_clades(10, parent, inst, held, 2).tolist() == [1, 5, 10, 13]
    # a higher mean wins over size; tips no source holds and undefined instabilities are left out of the mean
    inst2 = inst.copy()
    inst2[7] = 0.9          # (h,i) .7 > ((f,g),(h,i)) .6
    assert select_clades(2, parent, inst2, held, 64).tolist() == [13, 4]
    held2 = held.copy()
    held2[3] = 0            # (c,d): c alone, .9
    assert select_clades(1, parent, inst, held2, 64).tolist() == [5]
    inst3 = inst.copy()
    inst3[[0, 1]] = np.nan  # (a,b) is no candidate
    assert 1 not in select_clades(10, parent, inst3, held, 64).tolist()
    assert select_clades(0, parent, inst, held, 64).tolist() == []


def test_clades_by_name_or_node():
    sup = make_tree("((a,b),(((c,d)),e),f);")
    parent, _, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    got = _check_clade_placements([["b", "a"], 2, ("c", "d"), "f"], parent, index, 64)
    assert got.tolist() == [1, 2, 5, 10]  # ((c,d)) has two nodes: the upper one
    for bad in ([["a", "c"]], [["a", "b", "c"]], [0], [11], [["a", "zz"]], [1, ["a", "b"]], [list("abcdef")], [[]]):
        with pytest.raises(ValueError):
            _check_clade_placements(bad, parent, index, 64)
    assert _check_clade_placements(3, parent, index, 64) == 3 and _check_clade_placements(None, parent, index, 64) is None
    with pytest.raises(ValueError):
        _check_clade_placements(-1, parent, index, 64)


def test_regraft_clade_moves_errors_and_no_moves():
    sup = make_tree("((a,b),(((c,d)),e),f);")
    view = SupertreeScore(sup, None, None, None, None, None, None)
    clusters = lambda t: set(sr._leaf_sets(sr._preorder(t)).values())  # noqa: E731
    # nodes: 0 root, 1 (a,b), 2 a, 3 b, 4 (((c,d)),e), 5 ((c,d)), 6 (c,d), 7 c, 8 d, 9 e, 10 f
    for node, target in [(0, 1), (11, 1), (-1, 1), (1, 11), (1, 2), (1, 1), (6, 8), (5, 6)]:
        with pytest.raises(ValueError):
            view.regraft_clade(node, target)
    for node, target in [(6, 5), (6, 9), (6, 4), (5, 9), (2, 3), (2, 1)]:  # unary ancestor, sibling, two-child parent
        assert clusters(view.regraft_clade(node, target)) == clusters(sup), (node, target)
    for node in range(1, 11):
        inside = cr.subtree(pr._parents(sr._preorder(sup)), node)
        for target in range(11):
            if target not in inside:
                moved = view.regraft_clade(node, target)
                assert clusters(moved) == cr.regrafted_clusters(sup, node, target), (node, target)
                assert sorted(moved.get_tip_names()) == list("abcdef")
    assert clusters(sup) == clusters(make_tree("((a,b),(((c,d)),e),f);"))  # (the supertree itself is not edited)
    moved = view.regraft_clade(1, 6)
    assert frozenset("abcd") in clusters(moved) and frozenset("abcde") in clusters(moved)


def test_methods_need_the_counts():
    view = SupertreeScore(make_tree("((a,b),c);"), None, None, None, None, None, None)
    for call in (lambda: view.clade_placement_distance, view.best_clade_placements, view.clade_placement_table):
        with pytest.raises(ValueError, match="clade_placements"):
            call()


def test_the_header_declares_the_symbol_and_the_binding_holds_it():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int scs_score_clade_placements\(([^;]*)\);", header)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = _native.SIGNATURES["scs_score_clade_placements"]
    assert restype is _native.C.c_int and len(params) == len(argtypes) == 14
    assert argtypes == _native.SIGNATURES["scs_score_placements"][1]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "sources", "n_nodes", "parent", "taxon", "max_batch_trees", "max_lds_bytes", "n_queries",
                     "query_nodes", "cp_trees", "cp_total", "cp_source", "cp_super", "cp_shared"]
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header
