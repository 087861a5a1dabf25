"""Rooted triplet terms on the device (``scs_score_triplets``), held to the host references of
``tests/triplet_reference.py`` and to closed forms by exact equality."""

from math import comb

import numpy as np
import pytest
import score_reference as sr
import triplet_reference as tr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree

pytestmark = pytest.mark.gpu

KEYS = ("t_super", "t_source", "t_shared", "triplet_distance")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64, (what, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])


def _binary_supertree(seed: int, n_taxa: int):
    rs = np.random.RandomState(seed)
    return sr.random_tree(rs, [synthetic.taxon_name(i) for i in range(n_taxa)], binary=True)


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(23)
    for i in range(150):
        sup, trees = sr.random_case(rs)
        _same(score_supertree(sup, trees, triplets=True, device=dev), tr.brute_force(sup, trees), i)


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = tr.quadratic(sup, trees)
    _same(score_supertree(sup, trees, triplets=True, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), triplets=True, device=dev), ref, sup_file)


@pytest.mark.parametrize(("n_taxa", "n_trees", "per_tree", "extra"), [
    (200, 300, None, 0),     # full coverage
    (2000, 100, 100, 0),     # partial coverage
    (5000, 3, None, 1500),   # trees of 5 000 leaves (C(m, 3) > 2^32), supertree with extra taxa
])
def test_synthetic_forests_match_quadratic_reference(dev, n_taxa, n_trees, per_tree, extra):
    trees = synthetic.tree_objects(13, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = _binary_supertree(n_taxa + 1, n_taxa + extra)
    res = score_supertree(sup, trees, triplets=True, device=dev)
    _same(res, tr.quadratic(sup, trees), (n_taxa, n_trees))
    assert "triplets" in res.timings


def test_more_trees_than_one_batch(dev, monkeypatch):
    trees = synthetic.tree_objects(6, 300, 50, leaves_per_tree=120)
    sup = _binary_supertree(10, 300)
    whole = score_supertree(sup, trees, triplets=True, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, triplets=True, device=dev)
    ref = tr.quadratic(sup, trees)
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")


def test_tree_arrays_and_tree_objects_score_alike(dev):
    arrays = synthetic.tree_arrays(9, 500, 40, leaves_per_tree=120)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = _binary_supertree(3, 500)
    a = score_supertree(sup, arrays, triplets=True, device=dev)
    b = score_supertree(sup, objects, triplets=True, device=dev)
    for k in (*KEYS, "n_leaves", "rf", "supported"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.triplet_fit == b.triplet_fit and 0 < a.triplet_fit < 1


def _twin_trees(seed: int, n: int) -> tuple[TreeNode, str]:
    """A random binary tree on n taxa (O(n) merges) and the Newick of the same topology with child order shuffled."""
    rs = np.random.RandomState(seed)
    names = [synthetic.taxon_name(int(i)) for i in rs.permutation(n)]
    parts = [(TreeNode(x), x) for x in names]
    while len(parts) > 1:
        i = int(rs.randint(len(parts)))
        parts[i], parts[-1] = parts[-1], parts[i]
        a = parts.pop()
        j = int(rs.randint(len(parts)))
        parts[j], parts[-1] = parts[-1], parts[j]
        b = parts.pop()
        nwk = f"({a[1]},{b[1]})" if rs.rand() < 0.5 else f"({b[1]},{a[1]})"
        parts.append((TreeNode(None, [a[0], b[0]]), nwk))
    return parts[0][0], parts[0][1] + ";"


@pytest.mark.parametrize("n", [12_000, 30_000, 100_000])  # 6, 2 and 1 S' nodes per workgroup
def test_large_trees_against_closed_forms(dev, tmp_path, n):
    sup, newick = _twin_trees(n, n)
    path = tmp_path / "source.tre"
    path.write_text(newick + "\n(t0000000,t0000001,t0000002);\n")
    arrays = load_tree_arrays(path)
    full = comb(n, 3)
    res = score_supertree(sup, arrays, triplets=True, device=dev)  # (+ a fan of three against a resolved triple)
    assert res.t_super.tolist() == [full, 1] and res.t_source.tolist() == [full, 0]
    assert res.t_shared.tolist() == [full, 0] and res.triplet_distance.tolist() == [0, 1]
    assert res.rf.tolist() == [0, 1]
    star = TreeNode(None, [TreeNode(synthetic.taxon_name(i)) for i in range(n)])
    res = score_supertree(star, arrays, triplets=True, device=dev)
    assert res.t_super.tolist() == res.t_shared.tolist() == [0, 0] and res.t_source.tolist() == [full, 0]
    assert res.triplet_distance.tolist() == [full, 0]


def test_device_refuses_a_source_taxon_twice(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),a);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="twice"):
        dev.score_triplets(tables, parent, taxon)


def test_cli_triplet_columns(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    out, tsv = tmp_path / "out.tre", tmp_path / "scores.tsv"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(tsv), "--triplets"])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src), triplets=True)
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0][6:] == ["t_super", "t_source", "t_shared", "triplet_distance"]
    got = np.array([[int(x) for x in r[6:]] for r in rows[1:]], dtype=np.int64)
    want = np.stack([api.t_super, api.t_source, api.t_shared, api.triplet_distance], axis=1)
    assert np.array_equal(got, want)


def test_rf_and_support_do_not_change_with_triplets(dev):
    arrays = synthetic.tree_arrays(12, 800, 60, leaves_per_tree=200)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = _binary_supertree(5, 800)
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, device=dev)
        both = score_supertree(sup, trees, triplets=True, device=dev)
        assert plain.t_super is None and "triplets" not in plain.timings
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported"):
            assert np.array_equal(getattr(plain, k), getattr(both, k)), k
        assert plain.table() == "\n".join(line.rsplit("\t", 4)[0] for line in both.table().splitlines()) + "\n"
