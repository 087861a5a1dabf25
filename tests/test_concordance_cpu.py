"""Branch concordance counts without a device: the host reference on hand-made cases and against the identities that
tie it to the RF and conflict references; the ``SupertreeScore`` views of the counts and ``--concordance`` refuse what
they cannot do."""

import numpy as np
import pytest
import concordance_reference as qr
import conflict_reference as cr
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import SupertreeScore
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.score import quartet_branches
from spectralclustersupertree_amd.tree import make_tree

# preorder of (((a,b),c),d): root, ((a,b),c), (a,b), a, b, c, d
SUP4 = "(((a,b),c),d);"


def _at(res, node):
    return [int(res[k][node]) for k in qr.PER_NODE]


def test_four_taxon_trees_give_concordant_alt1_alt2_in_that_order():
    sup = make_tree(SUP4)
    assert qr.brute_force(sup, [])["quartet_branch"].tolist() == [False, True, True, False, False, False, False]
    # at (a,b): A = a, B = b, D = c, so alt1 = (a,c) and alt2 = (b,c)
    for newick, want in (("(((a,b),c),d);", [1, 1, 0, 0]), ("(((a,c),b),d);", [1, 0, 1, 0]),
                         ("(((b,c),a),d);", [1, 0, 0, 1])):
        res = qr.brute_force(sup, [make_tree(newick)])
        assert _at(res, 2) == want, newick
        # at ((a,b),c): A = (a,b), B = c, D = d; every one of the three sources has the cluster {a,b,c}
        assert _at(res, 1) == [1, 1, 0, 0], newick
        assert res["n_decisive"].tolist() == [2]
        assert res["n_concordant"].tolist() == [1 + want[1]] and res["n_alternative"].tolist() == [want[2] + want[3]]
    both = qr.brute_force(sup, [make_tree("(((a,c),b),d);"), make_tree("((a,b),(c,d));"), make_tree("(a,b,c,d);")])
    assert _at(both, 2) == [3, 1, 1, 0]  # (a,b,c,d) is decisive and displays none of the three: `other`
    assert _at(both, 1) == [3, 1, 0, 1]  # ((a,b),(c,d)) has (c,d) = B ∪ D: alt2
    assert both["n_decisive"].tolist() == [2, 2, 2] and both["n_alternative"].tolist() == [1, 1, 0]


def test_alt2_of_the_upper_branch():
    # at ((a,b),c): alt2 = B ∪ D = (c,d)
    res = qr.brute_force(make_tree(SUP4), [make_tree("((a,b),(c,d));")])
    assert _at(res, 1) == [1, 0, 0, 1] and _at(res, 2) == [1, 1, 0, 0]


def test_a_source_without_the_sibling_is_informative_but_not_decisive():
    sup = make_tree(SUP4)
    trees = [make_tree("((a,b),d);")]
    res = qr.brute_force(sup, trees)
    rf = sr.brute_force(sup, trees)
    assert rf["informative"][2] == 1 and rf["supported"][2] == 1
    assert _at(res, 2) == [0, 0, 0, 0]
    assert _at(res, 1) == [0, 0, 0, 0]  # B = c misses the tree
    assert res["n_decisive"].tolist() == [0]
    small = qr.brute_force(sup, [make_tree("(a,b);"), make_tree("a;")])
    assert not any(small[k].any() for k in qr.PER_TREE + qr.PER_NODE)


def test_polytomies_and_unary_nodes_are_no_quartet_branches():
    full = [make_tree("((((a,b),c),d),(e,f));"), make_tree("(((a,c),b),(d,(e,f)));")]
    for newick in ("((a,b,c),d);",            # a polytomy
                   "(((a,b),c),d,e);",        # children of a polytomy (the root) and below it
                   "((((a,b)),c),d);",        # (a,b) under a unary node; the unary node has one child
                   "(((a,b),c));"):           # a unary root: its child has no sibling
        sup = make_tree(newick)
        res = qr.brute_force(sup, full)
        nodes = sr._preorder(sup)
        mask = res["quartet_branch"]
        assert np.array_equal(mask, quartet_branches(np.asarray(sup.to_flat()[0])))
        for i, v in enumerate(nodes):
            par = v.parent
            want = par is not None and len(v.children) == 2 and len(par.children) == 2
            assert mask[i] == want, (newick, i)
            if not want:
                assert _at(res, i) == [0, 0, 0, 0], (newick, i)
    assert not qr.brute_force(make_tree("((a,b,c),d);"), full)["quartet_branch"].any()
    assert qr.brute_force(make_tree("(((a,b),c),d,e);"), full)["quartet_branch"].tolist() == \
        [False, False, True, False, False, False, False, False]
    assert not qr.brute_force(make_tree("((((a,b)),c),d);"), full)["quartet_branch"][2:].any()


def test_identities_on_random_small_cases():
    rs = np.random.RandomState(17)
    seen = np.zeros(4, dtype=np.int64)
    for _ in range(150):
        sup, trees = sr.random_case(rs)
        res = qr.brute_force(sup, trees)
        rf = sr.brute_force(sup, trees)
        conf = cr.brute_force(sup, trees)
        assert (res["decisive"] <= rf["informative"]).all()
        assert (res["concordant"] <= rf["supported"]).all()
        assert (res["alt1"] + res["alt2"] <= conf["conflicting"]).all()
        assert (res["concordant"] + res["alt1"] + res["alt2"] <= res["decisive"]).all()
        assert not res["decisive"][~res["quartet_branch"]].any()
        assert np.array_equal(res["quartet_branch"], quartet_branches(np.asarray(sup.to_flat()[0])))
        assert int(res["decisive"].sum()) == int(res["n_decisive"].sum())
        assert int(res["concordant"].sum()) == int(res["n_concordant"].sum())
        assert int((res["alt1"] + res["alt2"]).sum()) == int(res["n_alternative"].sum())
        # a decisive source is concordant with a branch exactly when it supports the clade: one tree at a time
        for tree in trees:
            one, rf1 = qr.brute_force(sup, [tree]), sr.brute_force(sup, [tree])
            dec = one["decisive"] == 1
            assert np.array_equal(one["concordant"][dec], rf1["supported"][dec])
        seen += [int(res[k].sum()) for k in qr.PER_NODE]
    assert (seen > 0).all(), seen


def test_planted_sources_fill_every_category():
    rs = np.random.RandomState(211)
    names = [f"p{i}" for i in range(120)]
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    trees = [qr.planted(rs, sup, names, 0.5, 4, 0.2) for _ in range(20)]
    assert all(sorted(t.get_tip_names()) == sorted(set(t.get_tip_names())) and len(t.get_tip_names()) == 60
               for t in trees)
    res = qr.brute_force(sup, trees)
    other = res["decisive"] - res["concordant"] - res["alt1"] - res["alt2"]
    assert min(int(res["concordant"].sum()), int(res["alt1"].sum()), int(res["alt2"].sum()), int(other.sum())) > 0
    assert (res["concordant"].sum() > res["alt1"].sum() + res["alt2"].sum())  # (a few moves: mostly the supertree)
    exact = qr.brute_force(sup, [qr.planted(rs, sup, names, 1.0, 0, 0.0)])
    assert np.array_equal(exact["decisive"], exact["quartet_branch"].astype(np.int64))
    assert np.array_equal(exact["concordant"], exact["decisive"])


def _score(**extra):
    # preorder of (((a,b),c),d): root, ((a,b),c), (a,b), a, b, c, d
    one = np.ones(2, dtype=np.int64)
    z = np.zeros(7, dtype=np.int64)
    inf, sup = z.copy(), z.copy()
    inf[[1, 2]] = [9, 8]
    sup[[1, 2]] = [7, 2]
    return SupertreeScore(make_tree(SUP4), np.array([4, 4]), one, one * 0, one, inf, sup, {}, **extra)


def _counts():
    z = np.zeros(7, dtype=np.int64)
    dec, con, a1, a2 = z.copy(), z.copy(), z.copy(), z.copy()
    dec[[1, 2]] = [8, 8]
    con[[1, 2]] = [6, 2]
    a1[[1, 2]] = [1, 1]
    a2[[1, 2]] = [0, 4]
    return {"n_decisive": np.array([2, 1]), "n_concordant": np.array([1, 0]), "n_alternative": np.array([0, 1]),
            "decisive": dec, "concordant": con, "alt1": a1, "alt2": a2}


def test_views_refuse_without_the_counts():
    plain = _score()
    assert plain.decisive is None and plain.n_decisive is None and "n_decisive" not in plain.table()
    assert plain.quartet_branch.tolist() == [False, True, True, False, False, False, False]
    for call in (plain.annotate_concordance, plain.nni_candidates, plain.branch_table, lambda: plain.other,
                 lambda: plain.gcf, lambda: plain.gdf1, lambda: plain.gdf2, lambda: plain.gdfp):
        with pytest.raises(ValueError, match="concordance=True"):
            call()


def test_views_of_the_counts():
    res = _score(**_counts())
    assert res.other.tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert np.allclose(res.gcf[[1, 2]], [75.0, 25.0]) and np.allclose(res.gdf1[[1, 2]], [12.5, 12.5])
    assert np.allclose(res.gdf2[[1, 2]], [0.0, 50.0]) and np.allclose(res.gdfp[[1, 2]], [12.5, 12.5])
    assert np.isnan(res.gcf[[0, 3, 4, 5, 6]]).all() and np.isnan(res.gdfp[0])
    assert res.annotate_concordance().get_newick(with_node_names=True) == "(((a,b)2/1/4/8,c)6/1/0/8,d);"
    assert res.supertree.get_newick(with_node_names=True) == SUP4  # (the supertree itself keeps no names)
    assert res.nni_candidates() == [{"node": 2, "alternative": "alt2", "decisive": 8, "concordant": 2, "alt1": 1,
                                     "alt2": 4, "margin": 2}]
    lines = res.table().splitlines()
    assert lines[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf\tn_decisive\tn_concordant\tn_alternative"
    assert lines[1] == "0\t4\t1\t0\t1\t-1\t2\t1\t0" and lines[2].endswith("\t1\t0\t1")
    rows = [line.split("\t") for line in res.branch_table().splitlines()]
    assert rows[0] == ["node", "clade_size", "informative", "supported", "decisive", "concordant", "alt1", "alt2",
                       "other"]
    assert rows[1:] == [["1", "3", "9", "7", "8", "6", "1", "0", "1"], ["2", "2", "8", "2", "8", "2", "1", "4", "1"]]


def test_nni_candidates_are_sorted_by_margin():
    counts = _counts()
    counts["alt1"][1] = 8  # margin 2 at node 1 as well: the tie goes to the earlier node
    counts["alt2"][2] = 7  # margin 5 at node 2
    got = _score(**counts).nni_candidates()
    assert [(r["node"], r["alternative"], r["margin"]) for r in got] == [(2, "alt2", 5), (1, "alt1", 2)]


def test_cli_concordance_needs_scores_out(tmp_path):
    res = CliRunner().invoke(scs, ["-i", str(DATA_DIR / "dcm_iq_source.tre"), "-o", str(tmp_path / "out.tre"),
                                   "--concordance"])
    assert res.exit_code == 2 and "--concordance needs --scores-out" in res.output
    assert not (tmp_path / "out.tre").exists()
