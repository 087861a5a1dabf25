"""Clade conflict counts on the device (``scs_score_conflicts``), held to the host references of
``tests/conflict_reference.py`` and to closed forms by exact equality."""

import numpy as np
import pytest
import conflict_reference as cr
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import construct_supertree, load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

KEYS = ("n_super_conflict", "n_source_conflict", "conflicting")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64, (what, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _arrays(trees, n_taxa: int) -> TreeArrays:
    return TreeArrays.from_trees(trees, [1.0] * len(trees), _names(n_taxa))


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(29)
    for i in range(150):
        sup, trees = sr.random_case(rs)
        _same(score_supertree(sup, trees, conflicts=True, device=dev), cr.brute_force(sup, trees), i)


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = cr.quadratic(sup, trees)
    _same(score_supertree(sup, trees, conflicts=True, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), conflicts=True, device=dev), ref, sup_file)


@pytest.mark.parametrize(("n_taxa", "n_trees", "per_tree", "extra"), [
    (200, 300, None, 0),     # full coverage
    (2000, 100, 100, 0),     # partial coverage
    (5000, 3, None, 1500),   # trees of 5 000 leaves, supertree with extra taxa
])
def test_contracted_synthetic_forests_match_quadratic_reference(dev, n_taxa, n_trees, per_tree, extra):
    # (binary trees alone would let n_super - shared pass for n_super_conflict: contract ~30 % of the inner edges)
    rs = np.random.RandomState(n_taxa + 7)
    trees = [cr.contract(t, rs, 0.3) for t in synthetic.tree_objects(17, n_taxa, n_trees, leaves_per_tree=per_tree)]
    sup = cr.contract(sr.random_tree(rs, _names(n_taxa + extra), binary=True), rs, 0.3)
    res = score_supertree(sup, trees, conflicts=True, device=dev)
    ref = cr.quadratic(sup, trees)
    _same(res, ref, (n_taxa, n_trees))
    assert "conflicts" in res.timings
    assert ref["n_super_conflict"].any() and (ref["n_super_conflict"] < res.n_super - res.shared).any()


def test_more_trees_than_one_batch(dev, monkeypatch):
    rs = np.random.RandomState(8)
    trees = [cr.contract(t, rs, 0.3) for t in synthetic.tree_objects(6, 300, 50, leaves_per_tree=120)]
    sup = cr.contract(sr.random_tree(rs, _names(300), binary=True), rs, 0.3)
    whole = score_supertree(sup, trees, conflicts=True, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, conflicts=True, device=dev)
    ref = cr.quadratic(sup, trees)
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")


def test_tree_arrays_and_tree_objects_score_alike(dev):
    rs = np.random.RandomState(10)
    objects = [cr.contract(t, rs, 0.3) for t in synthetic.tree_objects(9, 500, 40, leaves_per_tree=120)]
    arrays = _arrays(objects, 500)
    sup = cr.contract(sr.random_tree(rs, _names(500), binary=True), rs, 0.3)
    a = score_supertree(sup, arrays, conflicts=True, device=dev)
    b = score_supertree(sup, objects, conflicts=True, device=dev)
    for k in (*KEYS, "n_leaves", "rf", "supported", "informative"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.conflicting.any()


def test_other_terms_do_not_change_with_conflicts(dev):
    rs = np.random.RandomState(12)
    objects = [cr.contract(t, rs, 0.3) for t in synthetic.tree_objects(12, 800, 60, leaves_per_tree=200)]
    arrays = _arrays(objects, 800)
    sup = sr.random_tree(rs, _names(800), binary=True)
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, triplets=True, device=dev)
        both = score_supertree(sup, trees, triplets=True, conflicts=True, device=dev)
        assert plain.conflicting is None and "conflicts" not in plain.timings
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super",
                  "t_source", "t_shared"):
            assert np.array_equal(getattr(plain, k), getattr(both, k)), k
        assert plain.table() == "\n".join(line.rsplit("\t", 2)[0] for line in both.table().splitlines()) + "\n"
        assert (both.supported + both.conflicting <= both.informative).all()


def _twin_trees(seed: int, n: int) -> tuple[TreeNode, TreeNode]:
    """A random binary tree on n taxa (O(n) merges) and the same topology with child order shuffled."""
    rs = np.random.RandomState(seed)
    parts = [(TreeNode(x), TreeNode(x)) for x in (synthetic.taxon_name(int(i)) for i in rs.permutation(n))]
    while len(parts) > 1:
        i = int(rs.randint(len(parts)))
        parts[i], parts[-1] = parts[-1], parts[i]
        a = parts.pop()
        j = int(rs.randint(len(parts)))
        parts[j], parts[-1] = parts[-1], parts[j]
        b = parts.pop()
        twin = [a[1], b[1]] if rs.rand() < 0.5 else [b[1], a[1]]
        parts.append((TreeNode(None, [a[0], b[0]]), TreeNode(None, twin)))
    return parts[0]


def _every_other_edge_contracted(tree: TreeNode) -> TreeNode:
    """A copy of ``tree`` without the inner nodes at odd depth (their children hang from their parents)."""
    depth = {id(tree): 0}
    for node in sr._preorder(tree):
        for c in node.children:
            depth[id(c)] = depth[id(node)] + 1
    new: dict[int, TreeNode] = {}
    for node in reversed(sr._preorder(tree)):
        if node.is_tip():
            new[id(node)] = TreeNode(node.name)
            continue
        kids = []
        for c in node.children:
            nc = new.pop(id(c))
            kids.extend(list(nc.children) if not c.is_tip() and depth[id(c)] % 2 else [nc])
        new[id(node)] = TreeNode(None, kids)
    return new[id(tree)]


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for name in names[1:]:
        node = TreeNode(None, [node, TreeNode(name)])
    return node


@pytest.mark.parametrize("n", [12_000, 30_000, 100_000])
def test_large_trees_against_closed_forms(dev, n):
    sup, twin = _twin_trees(n, n)
    coarse = _every_other_edge_contracted(sup)
    res = score_supertree(sup, _arrays([twin, coarse], n), conflicts=True, device=dev)
    assert res.n_super_conflict.tolist() == res.n_source_conflict.tolist() == [0, 0]
    assert not res.conflicting.any() and res.rf[0] == 0 and res.rf[1] > 0
    names = _names(n)
    cat = _caterpillar(names)
    res = score_supertree(cat, _arrays([_caterpillar(names[::-1])], n), conflicts=True, device=dev)
    assert res.n_super_conflict.tolist() == res.n_source_conflict.tolist() == [n - 2]
    assert np.array_equal(res.conflicting, res.informative) and res.informative.sum() == n - 2
    other, _ = _twin_trees(n + 1, n)
    res = score_supertree(sup, _arrays([other], n), conflicts=True, device=dev)
    assert np.array_equal(res.n_super_conflict, res.n_super - res.shared)
    assert np.array_equal(res.n_source_conflict, res.n_source - res.shared)
    assert np.array_equal(res.conflicting, res.informative - res.supported) and res.conflicting.any()


def test_compatible_sources_score_zero(dev):
    rs = np.random.RandomState(21)
    for _ in range(3):
        names = [f"s{i}" for i in range(int(rs.randint(20, 60)))]
        model = sr.random_tree(rs, names, binary=True)
        trees = [model.get_sub_tree(list(rs.choice(names, size=int(rs.randint(4, len(names))), replace=False)))
                 for _ in range(int(rs.randint(3, 9)))]
        sup = construct_supertree(trees)
        res = score_supertree(sup, trees, conflicts=True, device=dev)
        assert not res.n_super_conflict.any() and not res.n_source_conflict.any() and not res.conflicting.any()


def test_cli_conflict_columns_and_counts(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    out, tsv, counts = tmp_path / "out.tre", tmp_path / "scores.tsv", tmp_path / "counts.tre"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(tsv), "--conflicts",
                                   "--conflict-out", str(counts)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src), conflicts=True)
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0][6:] == ["n_super_conflict", "n_source_conflict"]
    got = np.array([[int(x) for x in r[6:]] for r in rows[1:]], dtype=np.int64)
    assert np.array_equal(got, np.stack([api.n_super_conflict, api.n_source_conflict], axis=1))
    assert counts.read_text().strip() == api.annotate_counts().get_newick(with_node_names=True)
    named = [v.name for v in sr._preorder(load_tree(counts)) if not v.is_tip() and v.name]
    assert named and all(len(x.split("/")) == 3 for x in named)


def test_device_refuses_a_source_taxon_twice(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),a);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="twice"):
        dev.score_conflicts(tables, parent, taxon)
