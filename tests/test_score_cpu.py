"""``score_supertree`` without a device: the two host references agree with each other, and the API refuses bad
input before it touches a device."""

import numpy as np
import pytest
import score_reference as sr

from spectralclustersupertree_amd import score_supertree
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.tree import NotCompleted, TreeNode, make_tree

KEYS = ("n_super", "n_source", "shared", "rf", "informative", "supported")


def _agree(sup, trees):
    a, b = sr.brute_force(sup, trees), sr.linear(sup, trees)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (k, sup.get_newick(), [t.get_newick() for t in trees], a[k], b[k])
    return a


def test_references_agree_on_random_small_cases():
    rs = np.random.RandomState(12)
    for _ in range(400):
        sup, trees = sr.random_case(rs)
        _agree(sup, trees)


def test_references_on_hand_made_cases():
    sup = make_tree("((a,b),(c,(d,e)));")
    # identical tree: rf 0, every nontrivial clade supported
    res = _agree(sup, [make_tree("((a,b),(c,(d,e)));")])
    assert res["rf"].tolist() == [0] and res["n_super"].tolist() == [3]
    assert np.array_equal(res["informative"], res["supported"])
    # one conflicting clade: (a,c) against (a,b) / (c,d,e)
    res = _agree(sup, [make_tree("((a,c),(b,(d,e)));")])
    assert res["shared"].tolist() == [1] and res["rf"].tolist() == [4]
    # star source: nothing nontrivial on its side
    res = _agree(sup, [make_tree("(a,b,c,d);")])
    assert res["n_source"].tolist() == [0] and res["n_super"].tolist() == [2]
    # trees of 1 and 2 leaves give zeros
    res = _agree(sup, [make_tree("(a);"), make_tree("(a,b);")])
    assert res["rf"].tolist() == [0, 0] and not res["informative"].any()
    # unary nodes in S: every node on the path carries the count
    res = _agree(make_tree("(((a,b)),c,d);"), [make_tree("((a,b),c);")])
    assert res["informative"].tolist() == [0, 1, 1, 0, 0, 0, 0] and res["supported"].tolist() == [0, 1, 1, 0, 0, 0, 0]


def test_star_supertree_and_extra_taxa():
    rs = np.random.RandomState(3)
    names = [f"x{i}" for i in range(9)]
    star = TreeNode(None, [TreeNode(n) for n in names])
    trees = [sr.random_tree(rs, list(rs.choice(names[:6], size=5, replace=False))) for _ in range(6)]
    res = _agree(star, trees)
    assert not res["n_super"].any() and not res["informative"].any()


def test_api_errors_come_before_any_device_call(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(score_mod, "_default_device", no_device)
    sup = make_tree("((a,b),(c,d));")
    with pytest.raises(ValueError, match="not in the supertree"):
        score_supertree(sup, [make_tree("((a,b),e);")])
    with pytest.raises(ValueError, match="more than once"):
        score_supertree(make_tree("((a,b),(a,d));"), [make_tree("(a,b);")])
    with pytest.raises(ValueError, match="at least one tree"):
        score_supertree(sup, [])
    with pytest.raises(ValueError, match="at least one tree"):
        score_supertree(sup, [NotCompleted("FAIL", "load", "bad line")])
