"""The rule of ``refine_supertree`` on the host (no GPU): the reference loop of ``tests/refine_reference.py`` holds the
two identities of DESIGN.md section 24 -- moves with disjoint footprints add up, an interchange's gain is in the branch
triplet counts -- on random cases, a weakened footprint rule is caught, a misplaced tip is put back, and
``apply_moves``, the top-K rule and the boundary of the new export are checked."""

import re
from pathlib import Path

import branch_triplet_reference as btr
import numpy as np
import pytest
import refine_reference as rr
import score_reference as sr
import triplet_reference as tr
from concordance_reference import quartet_branches

from spectralclustersupertree_amd import _native
from spectralclustersupertree_amd.refine import (apply_moves, footprint_node, nni_candidates, select_moves,
                                                 subtree_ends, top_k_targets, tree_arrays_with_ids)
from spectralclustersupertree_amd.score import SupertreeScore, supertree_arrays
from spectralclustersupertree_amd.tree import make_tree

@pytest.fixture(scope="module")
def cases():
    return rr.additivity_cases(40)


def test_moves_with_disjoint_footprints_add_up(cases):
    """Every round's prediction is the rescored total (``reference_refine`` asserts it), the total falls strictly, and
    at least a tenth of the rounds with a move apply more than one."""
    with_move = multi = 0
    golden = rr.golden_runs()
    assert len(golden) == len(cases) == 40
    for n, (sup, trees) in enumerate(cases):
        out = rr.reference_refine(sup, trees, clade_max_tips=4)
        assert not out["mismatches"] and not out["interfered"]
        assert rr.run_record(out) == golden[n], n  # (the recorded runs the GPU tests read are the reference loop's)
        dist = [r["distance"] for r in out["rounds"]] + [out["final"]]
        assert out["initial"] == dist[0] and dist[-1] == rr.total_distance(out["tree"], trees), n
        for r, rnd in enumerate(out["rounds"]):
            if rnd["moves"]:
                assert dist[r + 1] == dist[r] - sum(m[3] for m in rnd["moves"]) < dist[r], (n, r)
                with_move += 1
                multi += len(rnd["moves"]) > 1
            else:
                assert r == len(out["rounds"]) - 1 and dist[r + 1] == dist[r]
        assert sorted(out["tree"].get_tip_names()) == sorted(sup.get_tip_names())
    print(f"rounds with a move {with_move}, with more than one {multi}")
    assert with_move >= 300 and 10 * multi >= with_move, (with_move, multi)


def test_a_weakened_footprint_rule_is_caught(cases):
    """The planted defect: with "the moved clades are disjoint" in place of disjoint footprints the gains of a round
    no longer add up to what rescoring says, on the same cases."""
    wrong = 0
    for sup, trees in cases:
        out = rr.reference_refine(sup, trees, clade_max_tips=4, footprint="clade", check=False)
        wrong += len(out["mismatches"])
    print(f"rounds whose prediction was wrong {wrong}")
    assert wrong >= 1


def test_an_interchange_gain_is_in_the_branch_triplet_counts():
    rs = np.random.RandomState(18)
    pairs = n_cases = 0
    while n_cases < 60:
        sup, trees = sr.random_case(rs, n_taxa=int(rs.randint(4, 13)))
        branches = quartet_branches(sup)
        if not branches:
            continue
        n_cases += 1
        nodes = sr._preorder(sup)
        index = {id(v): i for i, v in enumerate(nodes)}
        parent = sup.to_flat()[0]
        view = SupertreeScore(sup, None, None, None, None, None, None)
        base = tr.quadratic(sup, trees)
        bt = btr.node_sum(sup, trees)
        for c, a, b, _ in branches:
            for node, alt in ((b, "bt_alt1"), (a, "bt_alt2")):
                got = tr.quadratic(view.regraft_clade(index[id(node)], parent[c]), trees)
                assert int(got["t_super"].sum()) == int(base["t_super"].sum())
                assert (int(base["triplet_distance"].sum()) - int(got["triplet_distance"].sum())
                        == 2 * int(bt[alt][c] - bt["bt_concordant"][c])), (n_cases, c, alt)
                pairs += 1
        # the package's candidate list is the positive part of the same numbers
        want = sorted((index[id(node)], parent[c], 2 * int(bt[alt][c] - bt["bt_concordant"][c]), "nni")
                      for c, a, b, _ in branches for node, alt in ((b, "bt_alt1"), (a, "bt_alt2"))
                      if bt[alt][c] > bt["bt_concordant"][c])
        assert sorted(nni_candidates(parent, bt["bt_concordant"], bt["bt_alt1"], bt["bt_alt2"])) == want
    assert pairs >= 300, pairs


def test_a_misplaced_tip_is_put_back():
    rs = np.random.RandomState(7)
    kept = 0
    while kept < 30:
        case = rr.misplaced_tip_case(rs)
        if case is None:
            continue
        kept += 1
        start, trees = case
        out = rr.reference_refine(start, trees, taxa_per_round=len(start.get_tip_names()))
        assert out["initial"] > 0 and out["final"] == 0, kept
        assert sum(bool(r["moves"]) for r in out["rounds"]) == 1, (kept, out["rounds"])


def _clusters(tree):
    return set(sr._leaf_sets(sr._preorder(tree)).values())


def test_apply_moves_one_move_is_regraft_clade():
    sup = make_tree("((a,b),(((c,d)),e),f);")
    view = SupertreeScore(sup, None, None, None, None, None, None)
    before = sup.get_newick()
    n = len(sr._preorder(sup))
    ends = subtree_ends(sup.to_flat()[0])
    for node in range(1, n):
        for target in range(n):
            if node <= target < ends[node]:
                with pytest.raises(ValueError, match="inside"):
                    apply_moves(sup, [(node, target)])
            else:
                assert apply_moves(sup, [(node, target)]).get_newick() == view.regraft_clade(node, target).get_newick()
    assert sup.get_newick() == before and apply_moves(sup, []).get_newick() == before
    for bad in ([(0, 1)], [(n, 1)], [(-1, 1)], [(1, n)], [(1, -1)], [(1, 4), (6, 8)]):
        with pytest.raises(ValueError):
            apply_moves(sup, bad)


def test_apply_moves_disjoint_moves_do_not_depend_on_their_order():
    rs = np.random.RandomState(12)
    seen = 0
    for _ in range(200):
        sup = sr.random_tree(rs, [f"t{i}" for i in range(int(rs.randint(8, 25)))], polytomy=0.3, unary=0.1)
        parent = sup.to_flat()[0]
        n = len(parent)
        ends = subtree_ends(parent)
        cands = []
        for _ in range(40):
            q = int(rs.randint(1, n))
            v = int(rs.randint(0, n))
            if not q <= v < ends[q]:
                cands.append((q, v, int(rs.randint(1, 100)), "spr"))
        taken = select_moves(cands, parent)
        if len(taken) < 2:
            continue
        seen += 1
        moves = [(q, v) for q, v, _, _ in taken]
        one = apply_moves(sup, moves)
        assert apply_moves(sup, moves[::-1]).get_newick() == one.get_newick()
        for q, v in moves:  # what each move makes alone is in the tree that got them all
            alone = SupertreeScore(sup, None, None, None, None, None, None).regraft_clade(q, v)
            want = _clusters(alone) - _clusters(sup)
            assert want <= _clusters(one), (q, v)
        assert sorted(one.get_tip_names()) == sorted(sup.get_tip_names())
    assert seen >= 40, seen


def test_the_footprint_is_the_lca_or_the_ancestor_target():
    #  0 root; 1 (a,b); 2 a; 3 b; 4 (((c,d)),e); 5 ((c,d)); 6 (c,d); 7 c; 8 d; 9 e; 10 f
    sup = make_tree("((a,b),(((c,d)),e),f);")
    parent = sup.to_flat()[0]
    end = subtree_ends(parent)
    assert end.tolist() == [11, 4, 3, 4, 10, 9, 9, 8, 9, 10, 11]
    assert footprint_node(parent, end, 7, 8) == 6 and footprint_node(parent, end, 7, 9) == 4
    assert footprint_node(parent, end, 7, 4) == 4 and footprint_node(parent, end, 7, 5) == 5
    assert footprint_node(parent, end, 2, 7) == 0 and footprint_node(parent, end, 2, 0) == 0
    # (2 -> 3) stays inside (a,b), (7 -> 9) inside (((c,d)),e): both are taken; (10 -> 1) spans the root
    taken = select_moves([(2, 3, 5, "spr"), (7, 9, 9, "spr"), (10, 1, 7, "spr"), (7, 9, 4, "nni")], parent)
    assert taken == [(7, 9, 9, "spr"), (2, 3, 5, "spr")]
    assert select_moves([(10, 1, 9, "spr"), (2, 3, 5, "spr")], parent) == [(10, 1, 9, "spr")]
    # the weakened rule takes all three: their clades are disjoint
    assert len(select_moves([(2, 3, 5, "spr"), (7, 9, 9, "spr"), (10, 1, 7, "spr")], parent, footprint="clade")) == 3


def test_tree_arrays_with_ids_keeps_the_given_ids():
    sup = make_tree("((a,b),(c,d));")
    _, _, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    moved = apply_moves(sup, [(5, 2)])  # c onto the edge above a
    parent, taxon = tree_arrays_with_ids(moved, index)
    assert parent.dtype == np.int32 and taxon.dtype == np.int32 and parent.tolist() == moved.to_flat()[0]
    names = moved.to_flat()[1]
    assert [tips[t] for t in taxon if t >= 0] == [x for x in names if x in index]
    assert sorted(taxon[taxon >= 0].tolist()) == [0, 1, 2, 3] and taxon[taxon >= 0].tolist() != [0, 1, 2, 3]
    with pytest.raises(ValueError, match="taxon id"):
        tree_arrays_with_ids(make_tree("((a,b),(c,zz));"), index)


@pytest.mark.parametrize("pick", [top_k_targets, lambda d, q, e, k: rr.top_k(d, q, e, k).tolist()])
def test_top_k_rule_on_hand_made_rows(pick):
    row = [5, 3, 3, -7, 3, 9, -7, 0]
    assert pick(row, 3, 4, 3) == [6, 7, 1]              # the query's own -7 is left out; ties go to the lower index
    assert pick(row, 1, 3, 4) == [3, 6, 7, 4]           # the subtree [1, 3) is left out: 4 is the first 3
    assert pick(row, 6, 8, 2) == [3, 1]                 # the last range of the row
    assert pick(row, 1, 8, 3) == [0, -1, -1]            # a child of the root that holds the rest: the root alone
    assert pick(row, 2, 7, 8) == [7, 1, 0, -1, -1, -1, -1, -1]
    assert pick([0] * 7, 3, 5, 8) == [0, 1, 2, 5, 6, -1, -1, -1]  # all equal: preorder
    big = [-(1 << 61), 1 << 61, -(1 << 61) - 1, 0]
    assert pick(big, 3, 4, 3) == [2, 0, 1]              # signed 64-bit keys


def test_the_header_declares_the_symbol_and_the_binding_holds_it():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int scs_score_clade_moves\(([^;]*)\);", header)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = _native.SIGNATURES["scs_score_clade_moves"]
    assert restype is _native.C.c_int and len(params) == len(argtypes) == 18
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "sources", "n_nodes", "parent", "taxon", "max_batch_trees", "max_lds_bytes", "n_queries",
                     "query_nodes", "top_k", "cp_trees", "cp_total", "cp_source", "mv_own_super", "mv_own_shared",
                     "mv_node", "mv_super", "mv_shared"]
    placed = _native.SIGNATURES["scs_score_clade_placements"][1]
    assert argtypes[:9] == placed[:9] and argtypes[9] is _native._I32 and argtypes[10:13] == placed[9:12]
    for p, t in zip(params, argtypes):
        want = (_native._IP if "int32_t *" in p else _native._LP if "int64_t *" in p
                else _native._I32 if p.startswith("int32_t ") else _native._P)
        assert t is want, p
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header
