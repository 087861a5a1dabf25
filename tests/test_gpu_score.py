"""``score_supertree`` on the device (``scs_score_supertree``), held to the host references of
``tests/score_reference.py`` by exact equality."""

import numpy as np
import pytest
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import construct_supertree, load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

KEYS = ("n_super", "n_source", "shared", "rf", "informative", "supported")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(5)
    for i in range(150):
        sup, trees = sr.random_case(rs)
        _same(score_supertree(sup, trees, device=dev), sr.brute_force(sup, trees), i)


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = sr.brute_force(sup, trees)
    _same(score_supertree(sup, trees, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), device=dev), ref, sup_file)


def _binary_supertree(seed: int, n_taxa: int):
    rs = np.random.RandomState(seed)
    return sr.random_tree(rs, [synthetic.taxon_name(i) for i in range(n_taxa)], binary=True)


@pytest.mark.parametrize(("n_taxa", "n_trees", "per_tree", "extra"), [
    (200, 1500, None, 0),    # full coverage
    (2000, 300, 100, 0),     # partial coverage
    (5000, 3, None, 1500),   # trees of 5 000 leaves (hundreds of workgroups each), supertree with extra taxa
])
def test_synthetic_forests_match_linear_reference(dev, n_taxa, n_trees, per_tree, extra):
    trees = synthetic.tree_objects(11, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = _binary_supertree(n_taxa, n_taxa + extra)
    _same(score_supertree(sup, trees, device=dev), sr.linear(sup, trees), (n_taxa, n_trees))


def test_more_trees_than_one_batch(dev, monkeypatch):
    trees = synthetic.tree_objects(4, 300, 50, leaves_per_tree=120)
    sup = _binary_supertree(9, 300)
    whole = score_supertree(sup, trees, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, device=dev)
    ref = sr.linear(sup, trees)
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")


def test_tree_arrays_and_tree_objects_score_alike(dev):
    arrays = synthetic.tree_arrays(8, 500, 40, leaves_per_tree=120)
    objects = [arrays.to_tree(t) for t in range(arrays.n_trees)]
    sup = _binary_supertree(2, 500)
    a = score_supertree(sup, arrays, device=dev)
    b = score_supertree(sup, objects, device=dev)
    for k in (*KEYS, "n_leaves"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_tree_arrays_without_a_tree_of_two_leaves_score_zero(dev):
    """No source tree has two leaves, so no tables exist: every requested output is there, zero-filled, and the
    counted queries (the least stable taxa and clades of all-zero counts) are none."""
    sup = make_tree("((a,b),(c,d));")
    names = ["a", "b", "c", "d"]
    arrays = TreeArrays.from_trees([make_tree("(a);"), TreeNode("c"), make_tree("((d));")], [1.0] * 3, names)
    res = score_supertree(sup, arrays, triplets=True, conflicts=True, concordance=True, branch_triplets=True,
                          taxon_triplets=True, placements=2, clade_placements=1, device=dev)
    zero = lambda *shape: np.zeros(shape, dtype=np.int64)  # noqa: E731
    want = {"n_leaves": np.ones(3, dtype=np.int64), "pl_taxa": zero(0), "cp_nodes": zero(0)}
    want.update({k: zero(3) for k in (
        "n_super", "n_source", "shared", "t_super", "t_source", "t_shared", "n_super_conflict", "n_source_conflict",
        "n_decisive", "n_concordant", "n_alternative", "n_bt_total", "n_bt_concordant", "n_bt_alternative")})
    want.update({k: zero(7) for k in ("informative", "supported", "conflicting", "decisive", "concordant", "alt1",
                                      "alt2", "bt_total", "bt_concordant", "bt_alt1", "bt_alt2")})
    want.update({k: zero(4) for k in ("tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared")})
    want.update({k: zero(0) for k in ("pl_trees", "pl_total", "pl_source", "cp_trees", "cp_total", "cp_source")})
    want.update({k: zero(0, 7) for k in ("pl_super", "pl_shared", "cp_super", "cp_shared")})
    for k, v in want.items():
        got = getattr(res, k)
        assert got.dtype == np.int64 and got.shape == v.shape and np.array_equal(got, v), (k, got)
    assert res.taxa == names
    assert set(res.timings) == {"prepare", "tables", "score", "triplets", "conflicts", "concordance",
                                "branch_triplets", "taxon_triplets", "placements", "clade_placements"}
    assert res.total_rf == 0 and res.total_triplet_distance == 0
    assert res.best_placements() == [] and res.best_clade_placements() == []


def test_compatible_sources_score_zero(dev):
    rs = np.random.RandomState(21)
    for _ in range(3):
        names = [f"s{i}" for i in range(int(rs.randint(20, 60)))]
        model = sr.random_tree(rs, names, binary=True)
        trees = [model.get_sub_tree(list(rs.choice(names, size=int(rs.randint(4, len(names))), replace=False)))
                 for _ in range(int(rs.randint(3, 9)))]
        sup = construct_supertree(trees)
        res = score_supertree(sup, trees, device=dev)
        assert not res.rf.any() and res.total_rf == 0
        assert np.array_equal(res.supported, res.informative)


def test_supertree_against_itself_and_another(dev):
    rs = np.random.RandomState(33)
    names = [f"z{i}" for i in range(80)]
    s1 = sr.random_tree(rs, names)
    s2 = sr.random_tree(rs, names)
    assert score_supertree(s1, [s1], device=dev).rf.tolist() == [0]
    res = score_supertree(s1, [s2], device=dev)
    _same(res, sr.brute_force(s1, [s2]))
    assert res.total_rf == int(sr.brute_force(s1, [s2])["rf"][0])


def test_device_refuses_a_source_taxon_twice(dev):
    with pytest.raises(ValueError, match="twice"):
        score_supertree(make_tree("((a,b),(c,d));"), [make_tree("((a,b),a);")], device=dev)


def test_cli_scores_and_support(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    out, tsv, sup_out = tmp_path / "out.tre", tmp_path / "scores.tsv", tmp_path / "support.tre"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(tsv),
                                   "--support-out", str(sup_out)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src))
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0] == ["index", "n_leaves", "n_super", "n_source", "shared", "rf"]
    got = np.array([[int(x) for x in r] for r in rows[1:]], dtype=np.int64)
    want = np.stack([np.arange(len(api.rf)), api.n_leaves, api.n_super, api.n_source, api.shared, api.rf], axis=1)
    assert np.array_equal(got, want)
    assert sup_out.read_text().strip() == api.annotate().get_newick(with_node_names=True)
