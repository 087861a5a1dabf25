"""Per-branch triplet support without a device: the two host references against each other and against the relations
that tie the counts to the concordance and the rooted triplet references; the header and the binding; the
``SupertreeScore`` views of the counts."""

import re
from pathlib import Path

import numpy as np
import pytest
import branch_triplet_reference as br
import concordance_reference as qr
import conflict_reference as cr
import score_reference as sr
import triplet_reference as tr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import SupertreeScore, _native
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.tree import make_tree

KEYS = (*br.PER_TREE, *br.PER_NODE)
# preorder of (((a,b),c),d): root, ((a,b),c), (a,b), a, b, c, d
SUP4 = "(((a,b),c),d);"


def _same(a, b, what=""):
    for k in KEYS:
        assert a[k].dtype == np.int64 and np.array_equal(a[k], b[k]), (what, k)


def _at(res, node):
    return [int(res[k][node]) for k in br.PER_NODE]


def test_four_taxon_trees_by_hand():
    sup = make_tree(SUP4)
    # at (a,b): A = a, B = b, D = c: one triple; at ((a,b),c): A = (a,b), B = c, D = d: two triples (a,c,d), (b,c,d)
    for newick, low, high in (("(((a,b),c),d);", [1, 1, 0, 0], [2, 2, 0, 0]),
                              ("(((a,c),b),d);", [1, 0, 1, 0], [2, 2, 0, 0]),
                              ("(((b,c),a),d);", [1, 0, 0, 1], [2, 2, 0, 0]),
                              ("(a,b,c,d);", [1, 0, 0, 0], [2, 0, 0, 0]),
                              ("((a,b),(c,d));", [1, 1, 0, 0], [2, 0, 0, 2]),      # cd|a and cd|b: bd|a with b = c
                              ("(((a,d),c),b);", [1, 0, 1, 0], [2, 0, 1, 1])):     # ad|c is alt1, cd|b is alt2
        for ref in (br.brute_force, br.node_sum):
            res = ref(sup, [make_tree(newick)])
            assert _at(res, 2) == low and _at(res, 1) == high, (newick, ref.__name__)
            assert res["n_bt_total"].tolist() == [3]
            assert res["n_bt_concordant"].tolist() == [low[1] + high[1]]
            assert res["n_bt_alternative"].tolist() == [low[2] + low[3] + high[2] + high[3]]
    small = br.node_sum(sup, [make_tree("(a,b);"), make_tree("((a,b),d);"), make_tree("a;")])
    assert not any(small[k].any() for k in KEYS)  # (no source holds a taxon of all three sets of a branch)


def test_the_references_agree_on_random_cases():
    rs = np.random.RandomState(41)
    seen = np.zeros(4, dtype=np.int64)
    for i in range(60):
        sup, trees = sr.random_case(rs)
        ref = br.brute_force(sup, trees)
        _same(br.node_sum(sup, trees), ref, i)
        seen += [int(ref[k].sum()) for k in br.PER_NODE]
    assert (seen > 0).all(), seen


def _planted(seed: int, n_taxa: int, n_trees: int, frac: float, moves: int, share: float):
    rs = np.random.RandomState(seed)
    names = [f"p{i}" for i in range(n_taxa)]
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    return sup, [qr.planted(rs, sup, names, frac, moves, share) for _ in range(n_trees)]


def test_the_references_agree_on_a_planted_forest():
    sup, trees = _planted(97, 40, 12, 0.5, 3, 0.2)
    ref = br.brute_force(sup, trees)
    _same(br.node_sum(sup, trees), ref, "planted")
    fan = ref["bt_total"] - ref["bt_concordant"] - ref["bt_alt1"] - ref["bt_alt2"]
    sums = [int(ref[k].sum()) for k in br.PER_NODE[1:]] + [int(fan.sum())]
    assert min(sums) > 0, sums  # (every category occurs)
    assert sums[0] > sums[1] + sums[2]  # (a few moves: mostly the supertree's arrangement)


def _relations(sup, trees, ref):
    conc = qr.brute_force(sup, trees)
    assert (ref["bt_concordant"] + ref["bt_alt1"] + ref["bt_alt2"] <= ref["bt_total"]).all()
    assert np.array_equal(ref["bt_total"] > 0, conc["decisive"] > 0)
    assert not ref["bt_total"][~conc["quartet_branch"]].any()
    assert int(ref["bt_total"].sum()) == int(ref["n_bt_total"].sum())
    assert int(ref["bt_concordant"].sum()) == int(ref["n_bt_concordant"].sum())
    assert int((ref["bt_alt1"] + ref["bt_alt2"]).sum()) == int(ref["n_bt_alternative"].sum())
    trip = tr.quadratic(sup, trees)
    assert (ref["n_bt_total"] <= trip["t_super"]).all() and (ref["n_bt_concordant"] <= trip["t_shared"]).all()
    # a source that displays an arrangement at a branch gives all of its triples there to it: one tree at a time
    hits = np.zeros(3, dtype=np.int64)
    for tree in trees:
        one, c1 = br.node_sum(sup, [tree]), qr.brute_force(sup, [tree])
        for j, (whole, part) in enumerate((("concordant", "bt_concordant"), ("alt1", "bt_alt1"), ("alt2", "bt_alt2"))):
            at = c1[whole] == 1
            assert np.array_equal(one[part][at], one["bt_total"][at]), whole
            hits[j] += int(at.sum())
    return hits


def test_relations_on_random_and_planted_cases():
    rs = np.random.RandomState(43)
    hits = np.zeros(3, dtype=np.int64)
    for _ in range(60):
        sup, trees = sr.random_case(rs)
        hits += _relations(sup, trees, br.node_sum(sup, trees))
    sup, trees = _planted(98, 60, 10, 0.6, 3, 0.2)
    hits += _relations(sup, trees, br.node_sum(sup, trees))
    assert (hits > 0).all(), hits


def test_the_header_declares_the_symbol_and_the_binding_holds_it():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int scs_score_branch_triplets\(([^;]*)\);", header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).split(",")]
    restype, argtypes = _native.SIGNATURES["scs_score_branch_triplets"]
    assert len(params) == len(argtypes) == 13 and restype is _native.C.c_int
    assert argtypes == _native.SIGNATURES["scs_score_concordance"][1]
    assert [p.split("*")[-1].split()[-1] for p in params[6:]] == [*br.PER_TREE, *br.PER_NODE]
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header


def _score(**extra):
    one = np.ones(2, dtype=np.int64)
    z = np.zeros(7, dtype=np.int64)
    inf, sup = z.copy(), z.copy()
    inf[[1, 2]] = [9, 8]
    sup[[1, 2]] = [7, 2]
    return SupertreeScore(make_tree(SUP4), np.array([4, 4]), one, one * 0, one, inf, sup, {}, **extra)


def _counts() -> dict:
    sup = make_tree(SUP4)
    trees = [make_tree(x) for x in ("(((a,b),c),d);", "(((a,c),b),d);", "((a,c),(b,d));", "(a,b,c,d);",
                                    "(((a,c),b),d);")]
    return br.node_sum(sup, trees)


def test_views_refuse_without_the_counts():
    plain = _score()
    assert plain.bt_total is None and plain.n_bt_total is None and "n_bt_total" not in plain.table()
    for call in (plain.annotate_branch_triplets, lambda: plain.nni_candidates(by="triplets"), lambda: plain.bt_fan,
                 lambda: plain.tcf, lambda: plain.tdf1, lambda: plain.tdf2, lambda: plain.tdfu):
        with pytest.raises(ValueError, match="branch_triplets=True"):
            call()
    with pytest.raises(ValueError, match="'sources' or 'triplets'"):
        _score(**_counts()).nni_candidates(by="quartets")


def test_views_of_the_counts():
    counts = _counts()
    # node 2, (a,b) with D = c: one triple per source: ab|c, ac|b, ac|b, fan, ac|b
    # node 1, ((a,b),c) with D = d: the triples (a,c,d) and (b,c,d) per source: both concordant in sources 0, 1 and 4;
    # ac|d (concordant) and bd|c (alt1: a taxon of A with d) in source 2; two fans in source 3
    assert counts["bt_total"].tolist() == [0, 10, 5, 0, 0, 0, 0]
    assert [int(counts[k][1]) for k in br.PER_NODE] == [10, 7, 1, 0]
    assert counts["bt_concordant"][2] == 1 and counts["bt_alt1"][2] == 3 and counts["bt_alt2"][2] == 0
    res = _score(**counts)
    assert res.bt_fan.tolist() == (counts["bt_total"] - counts["bt_concordant"] - counts["bt_alt1"]
                                   - counts["bt_alt2"]).tolist()
    assert res.bt_fan[2] == 1 and (res.bt_fan >= 0).all()
    assert np.allclose(res.tcf[2], 20.0) and np.allclose(res.tdf1[2], 60.0) and np.allclose(res.tdf2[2], 0.0)
    assert np.allclose(res.tdfu[2], 20.0)
    for view in (res.tcf, res.tdf1, res.tdf2, res.tdfu):
        assert np.isnan(view[[0, 3, 4, 5, 6]]).all() and not np.isnan(view[[1, 2]]).any()
    assert np.allclose((res.tcf + res.tdf1 + res.tdf2 + res.tdfu)[[1, 2]], 100.0)
    c1 = [int(counts[k][1]) for k in ("bt_concordant", "bt_alt1", "bt_alt2", "bt_total")]
    assert res.annotate_branch_triplets().get_newick(with_node_names=True) == \
        f"(((a,b)1/3/0/5,c){c1[0]}/{c1[1]}/{c1[2]}/{c1[3]},d);"
    assert res.supertree.get_newick(with_node_names=True) == SUP4  # (the supertree itself keeps no names)
    assert res.nni_candidates(by="triplets") == [{"node": 2, "alternative": "alt1", "decisive": 5, "concordant": 1,
                                                  "alt1": 3, "alt2": 0, "margin": 2}]
    with pytest.raises(ValueError, match="concordance=True"):
        res.nni_candidates()  # (the default still counts sources)
    lines = res.table().splitlines()
    assert lines[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf\tn_bt_total\tn_bt_concordant\tn_bt_alternative"
    assert lines[1] == "0\t4\t1\t0\t1\t-1\t3\t3\t0" and lines[2] == "1\t4\t1\t0\t1\t-1\t3\t2\t1"


def test_a_branch_without_triples_gets_no_name():
    counts = {k: v.copy() for k, v in _counts().items()}
    for k in br.PER_NODE:
        counts[k][1] = 0
    assert _score(**counts).annotate_branch_triplets().get_newick(with_node_names=True) == "(((a,b)1/3/0/5,c),d);"


def test_tables_append_the_columns_only_when_present():
    conc = qr.brute_force(make_tree(SUP4), [make_tree("(((a,c),b),d);"), make_tree(SUP4)])
    conc.pop("quartet_branch")
    before = _score(**conc)
    both = _score(**conc, **_counts())
    assert before.branch_table().splitlines()[0].endswith("\talt2\tother")
    rows = [line.split("\t") for line in both.branch_table().splitlines()]
    assert rows[0][9:] == ["bt_total", "bt_concordant", "bt_alt1", "bt_alt2"]
    assert [r[:9] for r in rows] == [line.split("\t") for line in before.branch_table().splitlines()]
    assert [r[9:] for r in rows[1:]] == [[str(int(both.bt_total[i])), str(int(both.bt_concordant[i])),
                                          str(int(both.bt_alt1[i])), str(int(both.bt_alt2[i]))] for i in (1, 2)]
    assert both.table().splitlines()[0].endswith("\tn_alternative\tn_bt_total\tn_bt_concordant\tn_bt_alternative")
    assert before.table() == "\n".join(x.rsplit("\t", 3)[0] for x in both.table().splitlines()) + "\n"


def test_nni_candidates_by_triplets_are_sorted_by_margin():
    counts = {k: v.copy() for k, v in _counts().items()}
    counts["bt_concordant"][1], counts["bt_alt1"][1], counts["bt_alt2"][1] = 2, 1, 6
    got = _score(**counts).nni_candidates(by="triplets")
    assert [(r["node"], r["alternative"], r["margin"], r["decisive"]) for r in got] == [(1, "alt2", 4, 10),
                                                                                       (2, "alt1", 2, 5)]


def test_cli_branch_triplets_needs_a_table(tmp_path):
    res = CliRunner().invoke(scs, ["-i", str(DATA_DIR / "dcm_iq_source.tre"), "-o", str(tmp_path / "out.tre"),
                                   "--branch-triplets"])
    assert res.exit_code == 2 and "--branch-triplets needs --scores-out or --branches-out" in res.output
    assert not (tmp_path / "out.tre").exists()
