"""Per-taxon triplet support on the device (``scs_score_taxon_triplets``), held to the host references of
``tests/taxon_triplet_reference.py`` and to closed forms by exact equality."""

from math import comb

import numpy as np
import pytest
import score_reference as sr
import taxon_triplet_reference as xr
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

KEYS = (*xr.KEYS, "taxon_triplet_distance")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    assert res.taxa == supertree_arrays(res.supertree)[2], what
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64 and got.shape == ref[k].shape, (what, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _binary_supertree(seed: int, n_taxa: int) -> TreeNode:
    return sr.random_tree(np.random.RandomState(seed), _names(n_taxa), binary=True)


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for x in names[1:]:
        node = TreeNode(None, [node, TreeNode(x)])
    return node


def _sums_are_three_times_the_per_tree_sums(res):
    assert res.tx_shared.sum() == 3 * res.t_shared.sum()
    assert res.tx_super.sum() == 3 * res.t_super.sum()
    assert res.tx_source.sum() == 3 * res.t_source.sum()
    assert res.tx_total.sum() == 3 * sum(comb(int(m), 3) for m in res.n_leaves)


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(29)
    for i in range(150):
        sup, trees = sr.random_case(rs)
        _same(score_supertree(sup, trees, taxon_triplets=True, device=dev), xr.brute_force(sup, trees), i)


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = xr.quadratic(sup, trees)
    _same(score_supertree(sup, trees, taxon_triplets=True, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), taxon_triplets=True, device=dev), ref, sup_file)


@pytest.mark.parametrize("m", [3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_word_and_wave_edges(dev, m):
    rs = np.random.RandomState(m)
    names = _names(m)
    trees = [sr.random_tree(rs, names, binary=True), sr.random_tree(rs, names, polytomy=0.5, unary=0.0)]
    sup = sr.random_tree(rs, names, polytomy=0.4)
    _same(score_supertree(sup, trees, taxon_triplets=True, device=dev), xr.quadratic(sup, trees), m)


@pytest.mark.parametrize(("n_taxa", "n_trees", "per_tree", "extra"), [
    (200, 300, None, 0),     # full coverage
    (2000, 100, 100, 0),     # partial coverage
    (3000, 3, None, 500),    # trees of 3 000 leaves, supertree with extra taxa
])
def test_synthetic_forests_match_quadratic_reference(dev, n_taxa, n_trees, per_tree, extra):
    rs = np.random.RandomState(n_taxa)
    names = _names(n_taxa)
    trees = []
    for t in range(n_trees):  # every second one non-binary
        subset = names if per_tree is None else [names[i] for i in rs.choice(n_taxa, size=per_tree, replace=False)]
        trees.append(sr.random_tree(rs, list(subset), binary=t % 2 == 0))
    sup = _binary_supertree(n_taxa + 1, n_taxa + extra)
    res = score_supertree(sup, trees, triplets=True, taxon_triplets=True, device=dev)
    _same(res, xr.quadratic(sup, trees), (n_taxa, n_trees))
    _sums_are_three_times_the_per_tree_sums(res)
    assert "taxon_triplets" in res.timings
    if extra:
        assert (res.tx_trees == 0).sum() == extra and (res.tx_total[res.tx_trees == 0] == 0).all()


@pytest.fixture(scope="module")
def deep():
    """A caterpillar supertree on 1 500 taxa: the deepest tree, the longest per-node arrays and leaf passes."""
    names = _names(1500)
    order = [names[i] for i in np.random.RandomState(77).permutation(1500)]
    return order, _caterpillar(order)


@pytest.mark.parametrize("source", ["same", "reversed", "random"])
def test_caterpillar_supertree(dev, deep, source):
    order, sup = deep
    tree = {"same": lambda: _caterpillar(order), "reversed": lambda: _caterpillar(order[::-1]),
            "random": lambda: sr.random_tree(np.random.RandomState(78), list(order), binary=True)}[source]()
    res = score_supertree(sup, [tree], triplets=True, taxon_triplets=True, device=dev)
    _same(res, xr.quadratic(sup, [tree]), source)
    _sums_are_three_times_the_per_tree_sums(res)
    if source == "same":
        assert (res.taxon_triplet_distance == 0).all() and (res.tx_shared == comb(1499, 2)).all()


@pytest.fixture(scope="module")
def forest():
    """300 taxa x 50 trees of 120 leaves, its supertree and the host reference."""
    trees = synthetic.tree_objects(6, 300, 50, leaves_per_tree=120)
    sup = _binary_supertree(10, 300)
    return sup, trees, xr.quadratic(sup, trees)


def test_more_trees_than_one_batch(dev, forest, monkeypatch):
    sup, trees, ref = forest
    whole = score_supertree(sup, trees, taxon_triplets=True, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, taxon_triplets=True, device=dev)
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")


@pytest.mark.parametrize("lds_bytes", [1024, 600, 100])
def test_nodes_whose_arrays_do_not_fit_lds_go_through_global_memory(dev, forest, monkeypatch, lds_bytes):
    # the rows of a node take 64 bytes here.  1 024 bytes leave bins of 7, 52 and 112 entries, so every node with
    # |z| + |pz| > 110 goes to the slab; 600 leave smaller ones; 100 leave none, and every node goes to the slab
    sup, trees, ref = forest
    default = score_supertree(sup, trees, taxon_triplets=True, device=dev)
    monkeypatch.setattr(score_mod, "TAXON_LDS_BYTES", lds_bytes)
    small = score_supertree(sup, trees, taxon_triplets=True, device=dev)
    _same(default, ref, "default")
    _same(small, ref, lds_bytes)


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


@pytest.mark.parametrize("n", [12_000, 30_000])  # (the nodes under the root of the larger one fit no LDS bin)
def test_large_trees_against_closed_forms(dev, tmp_path, n):
    sup, newick = _twin_trees(n, n)
    path = tmp_path / "source.tre"
    path.write_text(newick + "\n")
    arrays = load_tree_arrays(path)
    each = comb(n - 1, 2)
    res = score_supertree(sup, arrays, taxon_triplets=True, device=dev)
    assert res.tx_trees.tolist() == [1] * n
    for k in ("tx_total", "tx_super", "tx_source", "tx_shared"):
        assert (getattr(res, k) == each).all(), k
    star = TreeNode(None, [TreeNode(synthetic.taxon_name(i)) for i in range(n)])
    res = score_supertree(star, arrays, taxon_triplets=True, device=dev)
    assert not res.tx_super.any() and not res.tx_shared.any()
    assert (res.tx_source == each).all() and (res.tx_total == each).all()


def test_large_tree_through_global_memory(dev, tmp_path, monkeypatch):
    """12 000 leaves with less than a third of the LDS: every node with |z| + |pz| above 5 382 takes the slab path,
    with arrays of up to 24 000 entries."""
    n = 12_000
    sup, newick = _twin_trees(n, n)
    path = tmp_path / "source.tre"
    path.write_text(newick + "\n")
    monkeypatch.setattr(score_mod, "TAXON_LDS_BYTES", 48 << 10)
    res = score_supertree(sup, load_tree_arrays(path), taxon_triplets=True, device=dev)
    for k in ("tx_total", "tx_super", "tx_source", "tx_shared"):
        assert (getattr(res, k) == comb(n - 1, 2)).all(), k


def test_tree_arrays_and_tree_objects_score_alike(dev):
    arrays = synthetic.tree_arrays(9, 500, 40, leaves_per_tree=120)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = _binary_supertree(3, 500)
    a = score_supertree(sup, arrays, taxon_triplets=True, device=dev)
    b = score_supertree(sup, objects, taxon_triplets=True, device=dev)
    assert a.taxa == b.taxa
    for k in (*KEYS, "n_leaves", "rf", "supported"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    inst = a.taxon_instability
    assert np.nanmin(inst) >= 0 and np.nanmax(inst) <= 1 and a.rogue_taxa(3)[0]["instability"] == np.nanmax(inst)


def test_other_outputs_do_not_change_with_taxon_triplets(dev):
    arrays = synthetic.tree_arrays(12, 800, 60, leaves_per_tree=200)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = _binary_supertree(5, 800)
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, triplets=True, device=dev)
        both = score_supertree(sup, trees, triplets=True, taxon_triplets=True, device=dev)
        assert plain.tx_shared is None and plain.taxa is None and "taxon_triplets" not in plain.timings
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super", "t_source",
                  "t_shared"):
            assert np.array_equal(getattr(plain, k), getattr(both, k)), k
        assert plain.table() == both.table()


def test_device_refuses_a_source_taxon_twice(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),a);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="twice"):
        dev.score_taxon_triplets(tables, parent, taxon)


def test_cli_taxa_out(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    files = {i: {k: tmp_path / f"{k}.{i}" for k in ("out", "scores", "support")} for i in (0, 1)}
    taxa = tmp_path / "taxa.tsv"
    for i in (0, 1):
        args = ["-i", str(src), "-o", str(files[i]["out"]), "--scores-out", str(files[i]["scores"]), "--triplets",
                "--support-out", str(files[i]["support"])]
        res = CliRunner().invoke(scs, args + (["--taxa-out", str(taxa), "--taxon-triplets"] if i else []))
        assert res.exit_code == 0, res.output
    for k in files[0]:
        assert files[0][k].read_bytes() == files[1][k].read_bytes(), k
    api = score_supertree(load_tree(files[1]["out"]), load_trees(src), taxon_triplets=True)
    rows = [line.split("\t") for line in taxa.read_text().splitlines()]
    assert rows[0] == ["taxon", "name", "tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared",
                       "triplet_distance"]
    assert [r[1] for r in rows[1:]] == api.taxa and [int(r[0]) for r in rows[1:]] == list(range(len(api.taxa)))
    got = np.array([[int(x) for x in r[2:]] for r in rows[1:]], dtype=np.int64)
    want = np.stack([api.tx_trees, api.tx_total, api.tx_super, api.tx_source, api.tx_shared,
                     api.taxon_triplet_distance], axis=1)
    assert np.array_equal(got, want)


def test_the_library_exports_the_symbol(dev):
    assert hasattr(dev._lib, "scs_score_taxon_triplets") and "scs_score_taxon_triplets" in _native.SIGNATURES
    assert dev._lib.scs_version() == 109


def test_sums_at_the_benchmark_shape(dev):
    """10 000 taxa, full trees: bin 0 holds five nodes per workgroup and every bin is used by every tree, a shape the
    host reference is too slow for; the sums are held to three times the per-tree sums of the same call."""
    n = 10_000
    arrays = synthetic.tree_arrays(1, n, 40)
    sup, _ = _twin_trees(2, n)
    res = score_supertree(sup, arrays, triplets=True, taxon_triplets=True, device=dev)
    _sums_are_three_times_the_per_tree_sums(res)
    assert (res.tx_trees == 40).all() and (res.tx_total == 40 * comb(n - 1, 2)).all()
    assert (res.tx_shared <= np.minimum(res.tx_super, res.tx_source)).all()
    assert (res.tx_source == 40 * comb(n - 1, 2)).all()  # (binary sources resolve every triple)
