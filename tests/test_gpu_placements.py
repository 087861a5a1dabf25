"""Taxon placement support on the device (``scs_score_placements``), held to the host references of
``tests/placement_reference.py``, to the per-taxon kernels on regrafted trees and to closed forms, by exact equality."""

from math import comb

import numpy as np
import placement_reference as pr
import pytest
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import _native, load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree

pytestmark = pytest.mark.gpu

KEYS = ("pl_trees", "pl_total", "pl_source", "pl_super", "pl_shared", "placement_distance")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64 and got.shape == ref[k].shape, (what, k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (what, k, np.argwhere(got != ref[k])[:10])


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _tips(sup: TreeNode) -> list[str]:
    return supertree_arrays(sup)[2]


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for x in names[1:]:
        node = TreeNode(None, [node, TreeNode(x)])
    return node


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(31)
    for i in range(150):
        sup, trees = sr.random_case(rs)
        tips = _tips(sup)
        res = score_supertree(sup, trees, placements=tips, device=dev)
        assert res.pl_taxa.tolist() == list(range(len(tips))) and res.taxa == tips, i
        _same(res, pr.brute_force(sup, trees, tips), i)


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    tips = _tips(sup)
    queries = [tips[i] for i in np.random.RandomState(3).permutation(len(tips))[:12]]
    ref = pr.recurrence(sup, trees, queries)
    _same(score_supertree(sup, trees, placements=queries, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), placements=queries, device=dev), ref, sup_file)


@pytest.mark.parametrize("m", [3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_word_and_wave_edges(dev, m):
    rs = np.random.RandomState(m)
    names = _names(m)
    trees = [sr.random_tree(rs, names, binary=True), sr.random_tree(rs, names, polytomy=0.5, unary=0.0)]
    sup = sr.random_tree(rs, names, polytomy=0.4)
    queries = [names[i] for i in sorted({0, m // 2, m - 1, *rs.choice(m, size=min(m, 6), replace=False).tolist()})]
    _same(score_supertree(sup, trees, placements=queries, device=dev), pr.recurrence(sup, trees, queries), m)


def test_partial_coverage_extra_taxa_and_a_taxon_no_tree_holds(dev):
    rs = np.random.RandomState(2000)
    n_taxa, extra = 2000, 500
    names = _names(n_taxa + extra)
    trees = []
    for t in range(100):  # every second one non-binary
        subset = [names[i] for i in rs.choice(n_taxa, size=100, replace=False)]
        trees.append(sr.random_tree(rs, subset, binary=t % 2 == 0))
    sup = sr.random_tree(np.random.RandomState(2001), names, binary=True)
    held = sorted({name for tree in trees for name in tree.get_tip_names()})
    queries = [held[i] for i in rs.choice(len(held), size=20, replace=False)] + [names[n_taxa + 7]]
    res = score_supertree(sup, trees, placements=queries, device=dev)
    _same(res, pr.recurrence(sup, trees, queries), "partial coverage")
    assert res.pl_trees[:-1].min() >= 1 and "placements" in res.timings
    assert res.pl_trees[-1] == 0 and res.pl_total[-1] == 0 and res.pl_source[-1] == 0
    assert not res.pl_super[-1].any() and not res.pl_shared[-1].any()


@pytest.fixture(scope="module")
def deep():
    """1 500 taxa in a random order, and the caterpillar on them."""
    names = _names(1500)
    order = [names[i] for i in np.random.RandomState(77).permutation(1500)]
    return order, _caterpillar(order)


def test_caterpillar_source_queried_at_its_deepest_tip(dev, deep):
    # the longest group list: 1 499 entries for one query, more than a workgroup takes in one pass
    order, source = deep
    sup = sr.random_tree(np.random.RandomState(79), list(order), polytomy=0.2, unary=0.0)
    queries = [order[0], order[1], order[750], order[-1]]
    _same(score_supertree(sup, [source], placements=queries, device=dev), pr.recurrence(sup, [source], queries),
          "caterpillar source")


def test_caterpillar_supertree(dev, deep):
    order, sup = deep
    tree = sr.random_tree(np.random.RandomState(78), list(order), binary=True)
    queries = [order[0], order[3], order[700], order[-1]]
    _same(score_supertree(sup, [tree], placements=queries, device=dev), pr.recurrence(sup, [tree], queries),
          "caterpillar supertree")


@pytest.fixture(scope="module")
def forest():
    """300 taxa x 20 trees of 120 leaves, its supertree, one query per tip and the host reference."""
    trees = synthetic.tree_objects(6, 300, 20, leaves_per_tree=120)
    sup = sr.random_tree(np.random.RandomState(10), _names(300), binary=True)
    queries = _tips(sup)
    return sup, trees, queries, pr.recurrence(sup, trees, queries)


def test_more_queries_than_one_pass(dev, forest):
    sup, trees, queries, ref = forest
    _same(score_supertree(sup, trees, placements=queries, device=dev), ref, "300 queries")
    some = [queries[i] for i in (5, 299, 64, 63, 130)]
    rows = [queries.index(x) for x in some]
    part = score_supertree(sup, trees, placements=some, device=dev)
    _same(part, {k: ref[k][rows] for k in KEYS}, "5 queries")
    assert part.pl_taxa.tolist() == rows


def test_more_trees_than_one_batch(dev, forest, monkeypatch):
    sup, trees, queries, ref = forest
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    _same(score_supertree(sup, trees, placements=queries[:70], device=dev), {k: ref[k][:70] for k in KEYS},
          "batches of 7")


@pytest.mark.parametrize("lds_bytes", [4096, 64, 3488])
def test_less_lds_than_the_sums_need(dev, forest, monkeypatch, lds_bytes):
    # a row pair takes 64 bytes here, the sums of one node and 64 queries 1 056: 4 096 bytes leave room for three
    # nodes per workgroup, 64 for the rows alone, and every node pair then sends its own marks
    sup, trees, queries, ref = forest
    monkeypatch.setattr(score_mod, "PLACEMENT_LDS_BYTES", lds_bytes)
    if lds_bytes == 3488:
        # two batches of one call with different plans: rows of one word (trees of up to 31 leaves) leave room for
        # three nodes (272 + 3 (16 + 1 056) = 3 488), rows of three words (64 to 95 leaves) for two
        # (zb = 3 and 2, W = 1 and 3, the sums in LDS in both: the host plan worked out off the device for these six
        # sizes, by the loop this test was written against and by the library's; the results here do not show it)
        rs = np.random.RandomState(3488)
        names = _names(100)
        trees = [sr.random_tree(rs, [names[i] for i in rs.choice(100, size=n, replace=False)])
                 for n in (20, 31, 29, 64, 95, 70)]
        sup = sr.random_tree(rs, names, polytomy=0.3)
        queries = _tips(sup)
        ref = pr.recurrence(sup, trees, queries[:70])
        monkeypatch.setattr(score_mod, "BATCH_TREES", 3)
    _same(score_supertree(sup, trees, placements=queries[:70], device=dev), {k: ref[k][:70] for k in KEYS}, lds_bytes)


@pytest.mark.parametrize("lds_bytes", [None, 80])
def test_full_coverage_over_several_passes(dev, monkeypatch, lds_bytes):
    # every tree holds every query, so the super marks of a pass go to its common rows: three passes (64, 64 and 2
    # queries), with the sums in LDS and with room for the rows alone (80 bytes: five words of 32 leaves)
    rs = np.random.RandomState(130)
    names = _names(130)
    trees = [sr.random_tree(rs, names, binary=True), sr.random_tree(rs, names, polytomy=0.5, unary=0.0),
             sr.random_tree(rs, names[:90])]
    sup = sr.random_tree(rs, names, polytomy=0.3)
    queries = _tips(sup)
    if lds_bytes:
        monkeypatch.setattr(score_mod, "PLACEMENT_LDS_BYTES", lds_bytes)
    _same(score_supertree(sup, trees, placements=queries, device=dev), pr.recurrence(sup, trees, queries), lds_bytes)


def test_own_node_sibling_and_two_child_parent_hold_the_current_scores(dev, forest):
    sup, trees, queries, _ = forest
    res = score_supertree(sup, trees, taxon_triplets=True, placements=queries, device=dev)
    nodes = sr._preorder(sup)
    index = {id(v): i for i, v in enumerate(nodes)}
    own = [i for i, v in enumerate(nodes) if v.is_tip()]
    seen = 0
    for i, x in enumerate(res.pl_taxa):
        at = [own[x]]
        parent = nodes[own[x]].parent
        if len(parent.children) == 2:
            at += [index[id(parent)], *(index[id(c)] for c in parent.children)]
            seen += 1
        for v in at:
            assert res.pl_shared[i, v] == res.tx_shared[x] and res.pl_super[i, v] == res.tx_super[x], (i, v)
        assert res.pl_source[i] == res.tx_source[x] and res.pl_trees[i] == res.tx_trees[x]
        assert res.pl_total[i] == res.tx_total[x]
    assert seen == len(queries)  # (a binary supertree)
    best = res.best_placements()
    assert [r["taxon"] for r in best] == res.pl_taxa.tolist()
    dist = res.placement_distance
    for i, r in enumerate(best):
        assert r["distance"] == res.taxon_triplet_distance[r["taxon"]] and r["best_distance"] == dist[i].min()
        assert r["improvement"] == r["distance"] - r["best_distance"] >= 0
        assert dist[i, r["best_node"]] == r["best_distance"]


def test_the_least_stable_taxa_are_placed_on_request(dev, forest):
    sup, trees, _, ref = forest
    res = score_supertree(sup, trees, placements=9, device=dev)
    assert res.tx_shared is not None and "taxon_triplets" in res.timings
    want = [r["taxon"] for r in res.rogue_taxa(9)]
    assert res.pl_taxa.tolist() == want and len(want) == 9
    _same(res, {k: ref[k][want] for k in KEYS}, "9 least stable")
    arrays = synthetic.tree_arrays(6, 300, 20, leaves_per_tree=120)
    res = score_supertree(sup, arrays, placements=9, device=dev)
    assert res.pl_taxa.tolist() == want
    _same(res, {k: ref[k][want] for k in KEYS}, "9 least stable, tree arrays")


def test_regrafted_trees_score_what_the_placement_says(dev):
    rs = np.random.RandomState(55)
    names = _names(90)
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(90, size=60, replace=False)]) for _ in range(12)]
    sup = sr.random_tree(rs, names, polytomy=0.2)
    nodes = sr._preorder(sup)
    tips = _tips(sup)
    queries = [tips[0], tips[41], tips[89]]
    res = score_supertree(sup, trees, placements=queries, device=dev)
    dist = res.placement_distance
    for i, x in enumerate(queries):
        tip = next(k for k, v in enumerate(nodes) if v.name == x)
        ancestors = []
        u = nodes[tip].parent
        while u is not None:
            ancestors.append(next(k for k, v in enumerate(nodes) if v is u))
            u = u.parent
        far = [k for k in range(len(nodes)) if k not in ancestors and k != tip]
        for v in [ancestors[0], ancestors[-2], 0, far[0], far[len(far) // 2], far[-1], int(np.argmin(dist[i]))]:
            moved = res.regraft(x, v)
            again = score_supertree(moved, trees, taxon_triplets=True, device=dev)
            assert again.taxon_triplet_distance[again.taxa.index(x)] == dist[i, v], (x, v)


def test_identical_source_and_supertree_of_12_000_leaves(dev):
    n = 12_000
    rs = np.random.RandomState(12)
    parts = [TreeNode(synthetic.taxon_name(int(i))) for i in rs.permutation(n)]
    while len(parts) > 1:
        i = int(rs.randint(len(parts)))
        parts[i], parts[-1] = parts[-1], parts[i]
        a = parts.pop()
        j = int(rs.randint(len(parts)))
        parts[j], parts[-1] = parts[-1], parts[j]
        parts.append(TreeNode(None, [a, parts.pop()]))
    sup = parts[0]
    tips = _tips(sup)
    queries = [tips[0], tips[n // 3], tips[n - 1], synthetic.taxon_name(0)]
    res = score_supertree(sup, [sup.copy()], placements=queries, device=dev)
    dist = res.placement_distance
    own = [i for i, v in enumerate(sr._preorder(sup)) if v.is_tip()]
    assert (res.pl_source == comb(n - 1, 2)).all() and (res.pl_total == comb(n - 1, 2)).all()
    for i, x in enumerate(res.pl_taxa):
        assert dist[i, own[x]] == 0 and dist[i].min() == 0
        assert res.pl_shared[i, own[x]] == comb(n - 1, 2)
    for r in res.best_placements():
        assert r["improvement"] == 0 and r["best_node"] == r["node"] and r["distance"] == 0


def test_star_supertree_root_entry(dev):
    rs = np.random.RandomState(8)
    names = _names(400)
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(400, size=250, replace=False)]) for _ in range(6)]
    star = TreeNode(None, [TreeNode(x) for x in names])
    queries = names[:5]
    res = score_supertree(star, trees, placements=queries, device=dev)
    for i, x in enumerate(queries):
        want = 0
        for tree in trees:
            tip = next((t for t in tree.iter_tips() if t.name == x), None)
            if tip is None:
                continue
            u = tip
            while u.parent is not None:  # the groups of x: the other children of its ancestors
                want += sum(comb(len(c.get_tip_names()), 2) for c in u.parent.children if c is not u)
                u = u.parent
        assert res.pl_shared[i, 0] == want, x
        assert res.pl_super[i, 0] == sum(comb(249, 2) for t in trees if x in t.get_tip_names())
        assert res.pl_super[i, 1 + names.index(x)] == 0  # (where it is, x resolves nothing)


def test_other_outputs_do_not_change_with_placements(dev):
    arrays = synthetic.tree_arrays(12, 800, 60, leaves_per_tree=200)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = sr.random_tree(np.random.RandomState(5), _names(800), binary=True)
    queries = _tips(sup)[10:20]
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, triplets=True, taxon_triplets=True, device=dev)
        both = score_supertree(sup, trees, triplets=True, taxon_triplets=True, placements=queries, device=dev)
        assert plain.pl_shared is None and plain.pl_taxa is None and "placements" not in plain.timings
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super", "t_source",
                  "t_shared", "tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared"):
            assert np.array_equal(getattr(plain, k), getattr(both, k)), k
        assert plain.table() == both.table() and plain.taxon_table() == both.taxon_table()


def test_device_refuses_bad_queries(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),c);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="not a tip"):
        dev.score_placements(tables, parent, taxon, [4])
    with pytest.raises(ValueError, match="twice"):
        dev.score_placements(tables, parent, taxon, [1, 2, 1])
    with pytest.raises(ValueError, match="no query"):
        dev.score_placements(tables, parent, taxon, [])
    out = dev.score_placements(tables, parent, taxon, [3, 0])
    assert out["pl_trees"].tolist() == [0, 1] and out["pl_shared"].shape == (2, 7)


def test_the_library_exports_the_symbol(dev):
    assert hasattr(dev._lib, "scs_score_placements") and "scs_score_placements" in _native.SIGNATURES
    assert dev._lib.scs_version() == 109


def test_cli_placements_out(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    files = {i: {k: tmp_path / f"{k}.{i}" for k in ("out", "scores", "support", "taxa")} for i in (0, 1)}
    table = tmp_path / "placements.tsv"
    for i in (0, 1):
        args = ["-i", str(src), "-o", str(files[i]["out"]), "--scores-out", str(files[i]["scores"]), "--triplets",
                "--support-out", str(files[i]["support"]), "--taxa-out", str(files[i]["taxa"])]
        res = CliRunner().invoke(scs, args + (["--placements-out", str(table), "--place-taxa", "4"] if i else []))
        assert res.exit_code == 0, res.output
    for k in files[0]:
        assert files[0][k].read_bytes() == files[1][k].read_bytes(), k
    api = score_supertree(load_tree(files[1]["out"]), load_trees(src), placements=4)
    assert table.read_text() == api.placement_table()
    rows = [line.split("\t") for line in table.read_text().splitlines()]
    assert rows[0] == ["taxon", "name", "trees", "node", "distance", "best_node", "best_distance", "improvement"]
    assert [int(r[0]) for r in rows[1:]] == [r["taxon"] for r in api.rogue_taxa(4)]
