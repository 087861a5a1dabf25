"""Rooted triplet terms without a device: the two host references agree with each other and with closed forms, the
API refuses bad input before it touches a device, and ``table()`` gains its columns only on request."""

from math import comb

import numpy as np
import pytest
import score_reference as sr
import triplet_reference as tr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import SupertreeScore, score_supertree
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.tree import NotCompleted, TreeNode, make_tree

KEYS = ("t_super", "t_source", "t_shared", "triplet_distance")


def _agree(sup, trees):
    a, b = tr.brute_force(sup, trees), tr.quadratic(sup, trees)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (k, sup.get_newick(), [t.get_newick() for t in trees], a[k], b[k])
    return a


def _caterpillar(names):
    node = TreeNode(names[0])
    for name in names[1:]:
        node = TreeNode(None, [node, TreeNode(name)])
    return node


def test_references_agree_on_random_small_cases():
    rs = np.random.RandomState(7)
    sizes = set()
    for _ in range(300):
        sup, trees = sr.random_case(rs)
        _agree(sup, trees)
        sizes.update(len(t.get_tip_names()) for t in trees)
    assert {1, 2} <= sizes and max(sizes) >= 10


def test_references_on_hand_made_cases():
    sup = make_tree("((a,b),(c,(d,e)));")
    res = _agree(sup, [make_tree("((a,b),(c,(d,e)));")])
    assert res["t_super"].tolist() == [10] and res["triplet_distance"].tolist() == [0]
    # b moved next to c: the triples of b change, the others stay
    res = _agree(sup, [make_tree("(a,((b,c),(d,e)));")])
    assert res["t_shared"].tolist() == [5] and res["triplet_distance"].tolist() == [10]
    # a fan in the source against a resolved triple in the supertree
    res = _agree(sup, [make_tree("(a,b,c);")])
    assert res["t_source"].tolist() == [0] and res["t_super"].tolist() == [1]
    assert res["triplet_distance"].tolist() == [1]
    # trees of 1 and 2 leaves give zeros; unary nodes change nothing
    res = _agree(make_tree("(((a,b)),c,d);"), [make_tree("(a);"), make_tree("(a,b);"), make_tree("(((a,c)),b);")])
    assert res["t_super"].tolist() == [0, 0, 1] and res["t_shared"].tolist() == [0, 0, 0]


def test_identities():
    rs = np.random.RandomState(19)
    for _ in range(40):
        names = [f"x{i}" for i in range(int(rs.randint(3, 30)))]
        m = len(names)
        t = sr.random_tree(rs, names)
        own = tr.quadratic(t, [t])
        assert own["t_shared"][0] == own["t_source"][0] == own["t_super"][0]
        b1, b2 = sr.random_tree(rs, names, binary=True), sr.random_tree(rs, names, binary=True)
        res = tr.quadratic(b1, [b2])
        assert res["t_source"][0] == res["t_super"][0] == comb(m, 3)
        star = TreeNode(None, [TreeNode(n) for n in names])
        res = tr.quadratic(star, [b1, t])
        assert not res["t_super"].any() and not res["t_shared"].any()
        assert res["t_source"][0] == comb(m, 3)
        cat = _caterpillar(names)
        res = tr.quadratic(cat, [_caterpillar(names[::-1])])
        assert res["t_shared"][0] == 0 and res["t_super"][0] == res["t_source"][0] == comb(m, 3)
        s1, s2 = sr.random_tree(rs, names), sr.random_tree(rs, names)
        assert tr.quadratic(s1, [s2])["t_shared"][0] == tr.quadratic(s2, [s1])["t_shared"][0]


def test_rf_zero_means_triplet_distance_zero():
    rs = np.random.RandomState(4)
    hits = 0
    for _ in range(200):
        sup, trees = sr.random_case(rs, n_trees=3)
        rf = sr.brute_force(sup, trees)["rf"]
        td = tr.quadratic(sup, trees)["triplet_distance"]
        assert not td[rf == 0].any()
        hits += int((rf == 0).sum())
    assert hits > 50


def test_triplet_errors_come_before_any_device_call(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(score_mod, "_default_device", no_device)
    sup = make_tree("((a,b),(c,d));")
    with pytest.raises(ValueError, match="not in the supertree"):
        score_supertree(sup, [make_tree("((a,b),e);")], triplets=True)
    with pytest.raises(ValueError, match="more than once"):
        score_supertree(make_tree("((a,b),(a,d));"), [make_tree("(a,b);")], triplets=True)
    with pytest.raises(ValueError, match="at least one tree"):
        score_supertree(sup, [NotCompleted("FAIL", "load", "bad line")], triplets=True)


def _score(**triplets):
    one = np.ones(2, dtype=np.int64)
    return SupertreeScore(make_tree("((a,b),c);"), np.array([3, 2]), one, one * 0, one, np.zeros(5, dtype=np.int64),
                          np.zeros(5, dtype=np.int64), {}, **triplets)


def test_table_gains_columns_only_with_triplets():
    plain = _score()
    assert plain.table() == "index\tn_leaves\tn_super\tn_source\tshared\trf\n0\t3\t1\t0\t1\t-1\n1\t2\t1\t0\t1\t-1\n"
    assert plain.t_super is None
    with pytest.raises(ValueError, match="triplets=True"):
        _ = plain.triplet_fit
    trip = _score(t_super=np.array([1, 0]), t_source=np.array([1, 0]), t_shared=np.array([0, 0]))
    lines = trip.table().splitlines()
    assert lines[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf\tt_super\tt_source\tt_shared\ttriplet_distance"
    assert lines[1] == "0\t3\t1\t0\t1\t-1\t1\t1\t0\t2" and lines[2].endswith("\t0\t0\t0\t0")
    assert trip.triplet_distance.tolist() == [2, 0] and trip.total_triplet_distance == 2 and trip.triplet_fit == 0.0
    none = _score(t_super=np.zeros(2), t_source=np.zeros(2), t_shared=np.zeros(2))
    assert np.isnan(none.triplet_fit)


def test_cli_triplets_needs_scores_out(tmp_path):
    res = CliRunner().invoke(scs, ["-i", str(DATA_DIR / "dcm_iq_source.tre"), "-o", str(tmp_path / "out.tre"),
                                   "--triplets"])
    assert res.exit_code == 2 and "--triplets needs --scores-out" in res.output
    assert not (tmp_path / "out.tre").exists()
