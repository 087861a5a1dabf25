"""The polytomy tensors and the resolution built on them, on the host alone: the two references
of ``tests/polytomy_reference.py`` against each other, the merge identity against edit-and-rescore, and the package's
host half (``resolve.merge_gain``, ``agglomerate``, ``resolve_from_tensors``, the pass of ``score_supertree``) against
the plain-Python reference."""

import numpy as np
import polytomy_reference as pr
import pytest
from score_reference import _preorder

from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd import score_supertree
from spectralclustersupertree_amd.resolve import agglomerate, merge_gain, resolve_from_tensors
from spectralclustersupertree_amd.tree import TreeNode, make_tree


@pytest.fixture(scope="module")
def cases():
    out = []
    for sup, trees, model in pr.polytomy_cases(40):
        out.append((sup, trees, model, pr.node_sum(sup, trees)))
    return out


def test_the_case_set_covers_the_ground(cases):
    degrees, nested, unary, fans = set(), 0, 0, 0
    for sup, trees, _, ref in cases:
        assert ref["nodes"][0] == 0  # a polytomy at the root
        degrees |= set(ref["degree"].tolist())
        poly = {id(v) for v in _preorder(sup) if len(v.children) >= 3}
        nested += any(id(v.parent) in poly for v in _preorder(sup) if v.parent is not None and id(v) in poly)
        unary += any(len(v.children) == 1 for t in trees for v in _preorder(t))
        fans += any(len(v.children) >= 3 for t in trees for v in _preorder(t))
        assert 8 <= len(sup.get_tip_names()) <= 30 and 3 <= len(trees) <= 8
    assert min(degrees) == 3 and max(degrees) == 9 and len(degrees) >= 6, degrees
    assert nested >= 10 and unary >= 10 and fans >= 10, (nested, unary, fans)


def test_the_two_references_agree(cases):
    seen = {"total": 0, "joint": 0, "fans": 0, "idle": 0}
    for sup, trees, _, ref in cases:
        sets = pr.brute_force(sup, trees)
        assert np.array_equal(sets["nodes"], ref["nodes"]) and np.array_equal(sets["trees"], ref["trees"])
        for q in range(len(ref["nodes"])):
            assert np.array_equal(sets["total"][q], ref["total"][q]), q
            assert np.array_equal(sets["joint"][q], ref["joint"][q]), q
            k = len(ref["total"][q])
            for i in range(k):  # filled for i < j and l not in {i, j} only
                assert not ref["total"][q][i, :i + 1].any() and not ref["total"][q][i, :, i].any()
                assert not ref["total"][q][:, i, i].any()
            seen["total"] += int(ref["total"][q].sum())
            seen["joint"] += int(ref["joint"][q].sum())
            seen["idle"] += int(ref["trees"][q] < len(trees))
        seen["fans"] += int(sum((r["total"][q] > r["joint"][q] + r["joint"][q].transpose(0, 2, 1)).any()
                                for r in (ref,) for q in range(len(r["nodes"]))))
    print("cases", seen)
    assert min(seen.values()) > 0, seen


def test_the_gain_of_a_merge_is_what_rescoring_says(cases):
    pairs = later = 0
    for sup, trees, _, ref in cases[:24]:
        for q, node in enumerate(ref["nodes"]):
            total, joint = ref["total"][q], ref["joint"][q]
            k = len(total)
            groups = list(range(k))
            base = pr.distance(sup, trees)
            for i in range(k):
                for j in range(i + 1, k):
                    want = base - pr.distance(pr.merged_tree(sup, int(node), [g for g in groups if g not in (i, j)]
                                                             + [(i, j)]), trees)
                    assert pr.gain(total, joint, [i], [j]) == want == merge_gain(total, joint, [i], [j]), (node, i, j)
                    pairs += 1
            # merges of merged groups: a random agglomeration down to two groups, every step on the edited tree
            rs = np.random.RandomState(int(node) + k)
            while len(groups) >= 3:
                g, h = sorted(rs.choice(len(groups), size=2, replace=False).tolist())
                G, H = pr._flat(groups[g]), pr._flat(groups[h])
                want = pr.rescored_gain(sup, trees, int(node), groups, g, h)
                assert pr.gain(total, joint, G, H) == want == merge_gain(total, joint, G, H), (node, G, H)
                groups = [x for i, x in enumerate(groups) if i not in (g, h)] + [(groups[g], groups[h])]
                later += len(G) + len(H) > 2
    print("pairs", pairs, "merges of merged groups", later)
    assert pairs > 200 and later > 50


def test_the_gains_add_up_over_a_whole_resolution(cases):
    merged = several = 0
    for sup, trees, _, ref in cases:
        out = pr.reference_resolve(sup, trees)
        assert pr.distance(out["tree"], trees) == out["predicted"] <= out["initial"]
        assert sorted(out["tree"].get_tip_names()) == sorted(sup.get_tip_names())
        merged += len(out["merges"])
        several += len({m[0] for m in out["merges"]}) > 1
        # the package's host half on the reference's tensors: the same merges, the same tree
        got = resolve_from_tensors(sup, ref["nodes"], ref["total"], ref["joint"], [], out["initial"])
        assert [(m["node"], *m["groups"], m["gain"]) for m in got.merges] == out["merges"]
        assert got.supertree.get_newick() == out["tree"].get_newick()
        assert (got.initial_distance, got.predicted_distance) == (out["initial"], out["predicted"])
        assert got.table().count("\n") == len(out["merges"]) + 1
    print("merges", merged, "cases with several polytomies resolved", several)
    assert merged > 100 and several > 10


def test_one_collapsed_edge_is_restored():
    rs = np.random.RandomState(3)
    for _ in range(30):
        sup, trees, model = pr.collapsed_edge_case(rs)
        out = pr.reference_resolve(sup, trees)
        assert len(out["merges"]) == 1 and out["predicted"] == 0 < out["initial"]
        assert out["tree"].same_shape(model)
        ref = pr.node_sum(sup, trees)
        got = resolve_from_tensors(sup, ref["nodes"], ref["total"], ref["joint"], [], out["initial"])
        assert got.supertree.same_shape(model) and got.predicted_distance == 0


def test_a_larger_collapse_need_not_come_back():
    # two collapsed edges, sizes that let the right pair win: the model comes back
    model = make_tree("(((a,b),c),(d1,d2,d3,d4));")
    sup = make_tree("(a,b,c,(d1,d2,d3,d4));")
    out = pr.reference_resolve(sup, [model])
    assert pr.distance(out["tree"], [model]) == out["predicted"] == 0 and out["tree"].same_shape(model)
    # DESIGN.md section 25's counter-example: the model is (((a,b),C),D) with |C| = 3, |D| = 4 and the root of the
    # supertree holds a, b, C, D.  ({a}, {b}) gains 1 * 1 * (3 + 4) = 7; ({a}, C) loses the 3 triples with b and gains
    # the 12 with D: 9.  The greedy choice takes (a, C), which the model does not hold
    model = make_tree("(((a,b),(c1,c2,c3)),(d1,d2,d3,d4));")
    sup = make_tree("(a,b,(c1,c2,c3),(d1,d2,d3,d4));")
    ref = pr.node_sum(sup, [model])
    assert pr.gain(ref["total"][0], ref["joint"][0], [0], [1]) == 7
    assert pr.gain(ref["total"][0], ref["joint"][0], [0], [2]) == 9
    out = pr.reference_resolve(sup, [model])
    assert out["merges"][0] == (0, [0], [2], 9)
    assert pr.distance(out["tree"], [model]) == out["predicted"] > 0 and not out["tree"].same_shape(model)


def test_min_gain_is_honoured(cases):
    for sup, trees, _, ref in cases[:10]:
        loose = pr.reference_resolve(sup, trees, min_gain=1)
        gains = sorted(m[3] for m in loose["merges"])
        if len(gains) < 2 or gains[0] == gains[-1]:
            continue
        bar = gains[len(gains) // 2]
        for q in range(len(ref["nodes"])):
            got = agglomerate(ref["total"][q], ref["joint"][q], bar)
            assert got == pr.agglomerate(ref["total"][q], ref["joint"][q], bar)
            assert all(g >= bar for _, _, g in got)
            assert agglomerate(ref["total"][q], ref["joint"][q], 10 ** 15) == []


def test_a_polytomy_without_a_decisive_source_stays():
    sup = make_tree("((a,b,c,d),(e,f,g),h);")
    trees = [make_tree("((a,b),e);"), make_tree("((e,f),(a,h));"), make_tree("(c,d);")]
    ref = pr.node_sum(sup, trees)
    # the root (children abcd, efg, h) has one decisive source; (a,b,c,d) and (e,f,g) have none
    assert ref["nodes"].tolist() == [0, 1, 6] and ref["trees"].tolist() == [1, 0, 0]
    assert not ref["total"][1].any() and not ref["total"][2].any()
    got = resolve_from_tensors(sup, ref["nodes"], ref["total"], ref["joint"], [], None)
    assert {m["node"] for m in got.merges} <= {0} and got.predicted_distance is None
    assert got.supertree.get_newick() == pr.reference_resolve(sup, trees)["tree"].get_newick()
    kids = {len(v.children) for v in _preorder(got.supertree)}
    assert 4 in kids and 3 in kids


def test_ties_go_to_the_lowest_child_positions():
    zero = np.zeros((5, 5, 5), dtype=np.int64)
    want = [([0], [1], 0), ([0, 1], [2], 0), ([0, 1, 2], [3], 0)]
    assert agglomerate(zero, zero, 0) == want == pr.agglomerate(zero, zero, 0)
    assert agglomerate(zero, zero, 1) == [] == pr.agglomerate(zero, zero, 1)
    # equal positive gains: a star of four with the sources ((a,b),c) and ((c,d),a) -- (a,b) and (c,d) tie
    sup = make_tree("(a,b,c,d);")
    ref = pr.node_sum(sup, [make_tree("((a,b),c);"), make_tree("((c,d),a);")])
    got = agglomerate(ref["total"][0], ref["joint"][0])
    assert got == pr.agglomerate(ref["total"][0], ref["joint"][0]) and got[0][:2] == ([0], [1])
    assert got == agglomerate(ref["total"][0].copy(), ref["joint"][0].copy())


def test_merge_gain_refuses_what_is_no_merge():
    zero = np.zeros((4, 4, 4), dtype=np.int64)
    for G, H in (([], [1]), ([0], [0]), ([0, 1], [2, 3]), ([0], [4]), ([0, 0], [1])):
        with pytest.raises(ValueError):
            merge_gain(zero, zero, G, H)


# ------------------------------------------------------------------ the pass of score_supertree, on a fake device
class _Tables:
    def __init__(self, n_trees):
        self.n_trees = n_trees

    def free(self):
        pass


class _Device:
    """``upload``, ``score`` and ``score_polytomies`` from the numpy reference."""

    def __init__(self, sup, trees):
        self.sup, self.trees, self.calls = sup, trees, []

    def upload(self, tables):
        return _Tables(tables.n_trees)

    def score(self, tabs, parent, taxon, **kw):
        zeros = {k: np.zeros(tabs.n_trees, dtype=np.int64) for k in ("n_super", "n_source", "shared")}
        zeros.update({k: np.zeros(len(parent), dtype=np.int64) for k in ("informative", "supported")})
        return zeros

    def score_polytomies(self, tabs, parent, taxon, query_nodes, **kw):
        self.calls.append((list(map(int, query_nodes)), kw))
        ref = pr.node_sum(self.sup, self.trees, only=list(map(int, query_nodes)))
        order = [ref["nodes"].tolist().index(int(q)) for q in query_nodes]
        return {"py_degree": ref["degree"][order].astype(np.int32), "py_trees": ref["trees"][order],
                "py_total": [ref["total"][i] for i in order], "py_joint": [ref["joint"][i] for i in order]}


def test_score_supertree_sends_the_polytomies_it_can(monkeypatch):
    sup = make_tree("((a,b,c,d),(e,f,g),h,(i,j));")
    trees = [make_tree("(((a,b),c),(e,h));"), make_tree("((e,f),(g,a),i);")]
    dev = _Device(sup, trees)
    plain = score_supertree(sup, trees, device=dev)
    assert plain.py_nodes is None and plain.py_skipped is None and dev.calls == []
    with pytest.raises(ValueError, match="polytomy counts were not computed"):
        plain.polytomy_table()
    res = score_supertree(sup, trees, polytomies=True, polytomy_max_degree=3, device=dev)
    assert dev.calls == [([6], {"batch_trees": 0, "lds_bytes": 0})] and "polytomies" in res.timings
    assert res.py_nodes.tolist() == [6] and res.py_nodes.dtype == np.int64
    assert [(s["node"], s["degree"]) for s in res.py_skipped] == [(0, 4), (1, 4)]
    assert all("more than 3 children" in s["reason"] for s in res.py_skipped)
    res = score_supertree(sup, trees, polytomies=[["a", "b", "c", "d"], 0], device=dev)
    assert dev.calls[-1][0] == [1, 0] and res.py_degree.tolist() == [4, 4] and res.py_skipped == []
    ref = pr.node_sum(sup, trees)
    assert res.polytomy_merge_gain(1, [0], [1]) == pr.gain(ref["total"][0], ref["joint"][0], [0], [1])
    rows = res.polytomy_table().splitlines()
    assert rows[0] == "node\ti\tj\ttips\ttotal\tjoint\tgain" and len(rows) == 1 + 6 + 6
    assert rows[1].split("\t")[:4] == ["1", "0", "1", "2"]
    done = res.resolve_polytomies()
    assert done.initial_distance is None and done.supertree.get_newick() != sup.get_newick()
    assert sup.get_newick() == "((a,b,c,d),(e,f,g),h,(i,j));"  # (the input is untouched)
    # rows that do not fit the LDS cap are skipped on the host, with the reason
    monkeypatch.setattr(score_mod, "POLYTOMY_LDS_BYTES", 24)
    res = score_supertree(sup, trees, polytomies=True, device=dev)
    assert dev.calls[-1] == ([6], {"batch_trees": 0, "lds_bytes": 24})
    assert [s["node"] for s in res.py_skipped] == [0, 1] and "LDS" in res.py_skipped[0]["reason"]
    for bad in ([5], [99], [0, 0], [["a", "b"]], "a", 3):
        with pytest.raises(ValueError):
            score_supertree(sup, trees, polytomies=bad, device=dev)
    with pytest.raises(ValueError, match="polytomy_max_degree"):
        score_supertree(sup, trees, polytomies=True, polytomy_max_degree=65, device=dev)
