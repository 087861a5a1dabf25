"""Per-branch triplet support on the device (``scs_score_branch_triplets``), held to the host references of
``tests/branch_triplet_reference.py`` and to closed forms by exact equality."""

import ctypes

import numpy as np
import pytest
import branch_triplet_reference as br
import concordance_reference as qr
import conflict_reference as cr
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import _native, load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import TreeTables
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

KEYS = (*br.PER_TREE, *br.PER_NODE)
# the largest source tree: three bitset rows of int2 per 32 leaves within 160 KiB of LDS
LDS_CAP = (160 << 10) // 24 * 32 - 1


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64, (what, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])


def _sums(ref) -> dict:
    out = {k: int(ref[k].sum()) for k in br.PER_NODE}
    out["bt_fan"] = out["bt_total"] - out["bt_concordant"] - out["bt_alt1"] - out["bt_alt2"]
    return out


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _arrays(trees, n_taxa: int) -> TreeArrays:
    return TreeArrays.from_trees(trees, [1.0] * len(trees), _names(n_taxa))


def _sizes(tree: TreeNode) -> np.ndarray:
    """Leaves below every node, preorder."""
    nodes = sr._preorder(tree)
    parent = tree.to_flat()[0]
    size = np.array([1 if v.is_tip() else 0 for v in nodes], dtype=np.int64)
    for i in range(len(nodes) - 1, 0, -1):
        size[parent[i]] += size[i]
    return size


def _triples_around(tree: TreeNode) -> np.ndarray:
    """|A| |B| |D| at every quartet branch of ``tree`` (preorder; 0 elsewhere)."""
    nodes = sr._preorder(tree)
    size = _sizes(tree)
    index = {id(v): i for i, v in enumerate(nodes)}
    out = np.zeros(len(nodes), dtype=np.int64)
    for i, a, b, d in qr.quartet_branches(tree):
        out[i] = size[index[id(a)]] * size[index[id(b)]] * size[index[id(d)]]
    return out


def test_random_small_cases_match_the_set_reference(dev):
    rs = np.random.RandomState(29)
    total = {k: 0 for k in (*br.PER_NODE, "bt_fan")}
    for i in range(150):
        sup, trees = sr.random_case(rs)
        ref = br.brute_force(sup, trees)
        _same(score_supertree(sup, trees, branch_triplets=True, device=dev), ref, i)
        for k, v in _sums(ref).items():
            total[k] += v
    print("random cases", total)
    assert min(total.values()) > 0, total


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = br.node_sum(sup, trees)
    sums = _sums(ref)
    print(sup_file, sums)
    if sums["bt_total"] < 100_000:  # (the dcm pairs: small enough to go triple by triple as well)
        sets = br.brute_force(sup, trees)
        assert all(np.array_equal(sets[k], ref[k]) for k in KEYS)
        assert sums["bt_total"] == sums["bt_concordant"] > 0  # every decisive source is concordant there
    else:  # (binary sources: every triple is resolved, a good share of them another way)
        assert min(sums["bt_concordant"], sums["bt_alt1"], sums["bt_alt2"]) > 0 and sums["bt_fan"] == 0, sums
    _same(score_supertree(sup, trees, branch_triplets=True, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), branch_triplets=True, device=dev), ref, sup_file)


@pytest.mark.parametrize(("n_taxa", "n_trees", "frac", "moves", "share", "extra"), [
    (200, 60, 1.0, 6, 0.2, 0),      # full coverage
    (2000, 40, 0.05, 4, 0.2, 0),    # partial coverage: many informative sources are not decisive
    (3000, 3, 1.0, 60, 0.2, 0),     # large trees
    (400, 30, 0.5, 5, 0.2, 150),    # a supertree with taxa no source has
])
def test_planted_forests_match_the_node_sum(dev, n_taxa, n_trees, frac, moves, share, extra):
    rs = np.random.RandomState(n_taxa + 11)
    names = _names(n_taxa)
    sup = cr.contract(sr.random_tree(rs, _names(n_taxa + extra), binary=True), rs, 0.1)
    shown = sup.get_sub_tree(names) if extra else sup
    trees = [qr.planted(rs, shown, names, frac, moves, share) for _ in range(n_trees)]
    ref = br.node_sum(sup, trees)
    sums = _sums(ref)
    print("planted", n_taxa, n_trees, sums)
    # (not a measurement: a kernel that returns zeros must not pass)
    assert min(sums["bt_concordant"], sums["bt_alt1"], sums["bt_alt2"], sums["bt_fan"]) > 0, sums
    res = score_supertree(sup, trees, branch_triplets=True, concordance=True, device=dev)
    _same(res, ref, (n_taxa, n_trees))
    assert "branch_triplets" in res.timings
    assert np.array_equal(res.bt_total > 0, res.decisive > 0) and (res.bt_fan >= 0).all()
    _same(score_supertree(sup, _arrays(trees, n_taxa + extra), branch_triplets=True, device=dev), ref, "arrays")


def test_copies_of_a_binary_supertree_are_concordant_everywhere(dev):
    rs = np.random.RandomState(5)
    sup = sr.random_tree(rs, _names(300), binary=True)
    res = score_supertree(sup, [sup.copy() for _ in range(5)], branch_triplets=True, device=dev)
    around = _triples_around(sup)
    inner = np.array([i > 0 and not v.is_tip() for i, v in enumerate(sr._preorder(sup))])
    assert np.array_equal(around > 0, inner)
    assert np.array_equal(res.bt_total, 5 * around) and np.array_equal(res.bt_concordant, res.bt_total)
    assert not res.bt_alt1.any() and not res.bt_alt2.any() and not res.bt_fan.any()
    assert res.n_bt_total.tolist() == res.n_bt_concordant.tolist() == [int(around.sum())] * 5
    assert res.n_bt_alternative.tolist() == [0] * 5 and res.nni_candidates(by="triplets") == []
    assert np.array_equal(res.tcf[inner], np.full(int(inner.sum()), 100.0)) and np.isnan(res.tcf[~inner]).all()


@pytest.mark.parametrize("which", ["alt1", "alt2"])
def test_one_interchange_moves_the_triples_of_its_branch(dev, which):
    rs = np.random.RandomState(6)
    sup = sr.random_tree(rs, _names(200), binary=True)
    nodes = sr._preorder(sup)
    around = _triples_around(sup)
    branches = [i for i, v in enumerate(nodes) if i > 0 and not v.is_tip()]
    at = max(branches, key=lambda i: (around[i] > 1, -abs(i - len(nodes) // 2)))  # a branch of several triples
    assert around[at] > 1
    moved = sup.copy()
    c = sr._preorder(moved)[at]
    par = c.parent
    j = 1 - par.children.index(c)
    i = 1 if which == "alt1" else 0  # alt1 = ad|b: B changes places with D; alt2 = bd|a: A does
    c.children[i], par.children[j] = par.children[j], c.children[i]
    c.children[i].parent, par.children[j].parent = c, par
    res = score_supertree(sup, [moved, sup.copy()], branch_triplets=True, device=dev)
    _same(res, br.node_sum(sup, [moved, sup.copy()]), which)
    want = np.zeros(len(nodes), dtype=np.int64)
    want[at] = around[at]
    assert np.array_equal(getattr(res, "bt_" + which), want)
    assert not getattr(res, "bt_alt2" if which == "alt1" else "bt_alt1").any() and not res.bt_fan.any()
    assert np.array_equal(res.bt_total, 2 * around) and np.array_equal(res.bt_concordant, res.bt_total - want)
    assert res.n_bt_alternative.tolist() == [int(around[at]), 0]
    assert res.n_bt_total.tolist() == [int(around.sum())] * 2
    assert res.nni_candidates(by="triplets") == []  # (one source each way: no alternative is ahead)
    res = score_supertree(sup, [moved, moved.copy(), sup.copy()], branch_triplets=True, device=dev)
    n = int(around[at])
    assert res.nni_candidates(by="triplets") == [{"node": at, "alternative": which, "decisive": 3 * n,
                                                  "concordant": n, "alt1": 2 * n * (which == "alt1"),
                                                  "alt2": 2 * n * (which == "alt2"), "margin": n}]
    named = [v.name for v in sr._preorder(res.annotate_branch_triplets()) if not v.is_tip()]
    assert named[0] is None
    assert named[branches.index(at) + 1] == (f"{n}/{2 * n}/0/{3 * n}" if which == "alt1" else f"{n}/0/{2 * n}/{3 * n}")


def test_star_sources_are_all_fans(dev):
    rs = np.random.RandomState(7)
    names = _names(150)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.2)
    stars = [TreeNode(None, [TreeNode(x) for x in rs.permutation(names)]) for _ in range(4)]
    res = score_supertree(sup, stars, branch_triplets=True, device=dev)
    around = _triples_around(sup)
    assert around.any() and np.array_equal(res.bt_total, 4 * around) and np.array_equal(res.bt_fan, res.bt_total)
    assert not res.bt_concordant.any() and not res.bt_alt1.any() and not res.bt_alt2.any()
    assert res.n_bt_total.tolist() == [int(around.sum())] * 4 and not res.n_bt_concordant.any()
    assert np.array_equal(res.tdfu[around > 0], np.full(int((around > 0).sum()), 100.0))


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for name in names[1:]:
        node = TreeNode(None, [node, TreeNode(name)])
    return node


def test_deep_caterpillar(dev):
    n = 20_000
    names = _names(n)
    cat = _caterpillar(names)
    res = score_supertree(cat, _arrays([_caterpillar(names[::-1]), _caterpillar(names)], n), branch_triplets=True,
                          device=dev)
    # preorder: the inner nodes first (node i holds x0 .. x(n-1-i)), every one but the root a quartet branch with
    # A = x0 .. x(n-2-i), B = x(n-1-i), D = x(n-i): n - 1 - i triples per source.  The forward copy resolves all of
    # them ab|d; the reversed caterpillar's clusters are the sets x(j) .. x(n-1), so it resolves every one bd|a
    per = np.zeros(2 * n - 1, dtype=np.int64)
    per[1:n - 1] = n - 1 - np.arange(1, n - 1)
    assert np.array_equal(res.bt_total, 2 * per) and np.array_equal(res.bt_concordant, per)
    assert np.array_equal(res.bt_alt2, per) and not res.bt_alt1.any() and not res.bt_fan.any()
    assert res.n_bt_total.tolist() == [int(per.sum())] * 2
    assert res.n_bt_concordant.tolist() == [0, int(per.sum())]
    assert res.n_bt_alternative.tolist() == [int(per.sum()), 0]


def test_more_trees_than_one_batch(dev, monkeypatch):
    rs = np.random.RandomState(8)
    names = _names(300)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    trees = [qr.planted(rs, sup, names, 0.4, 5, 0.2) for _ in range(50)]
    whole = score_supertree(sup, trees, branch_triplets=True, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, branch_triplets=True, device=dev)
    arrays = score_supertree(sup, _arrays(trees, 300), branch_triplets=True, device=dev)
    ref = br.node_sum(sup, trees)
    assert ref["bt_alt1"].any() and ref["bt_alt2"].any()
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")
    _same(arrays, ref, "arrays, batches of 7")


def test_a_tree_above_the_lds_cap_is_refused(dev):
    # a star of one leaf more than three bitset rows hold, against a star supertree: refused by the size check at the
    # head of the call, before any kernel
    assert LDS_CAP == 218_431
    n = LDS_CAP + 1
    tables = TreeTables(n_taxa=n, tree_off=np.array([0, n], dtype=np.int64),
                        leaf_taxon=np.arange(n, dtype=np.int32), adj_depth=np.zeros(n, dtype=np.int32),
                        adj_val=np.zeros(n, dtype=np.float64), tree_w=np.ones(1, dtype=np.float64))
    parent = np.concatenate([[-1], np.zeros(n, dtype=np.int32)]).astype(np.int32)
    taxon = np.concatenate([[-1], np.arange(n, dtype=np.int32)]).astype(np.int32)
    tabs = dev.upload(tables)
    try:
        with pytest.raises(ValueError, match=rf"{n} leaves is more than the {LDS_CAP} the pair kernel holds in LDS"):
            dev.score_branch_triplets(tabs, parent, taxon)
        assert dev.score(tabs, parent, taxon)["n_super"].tolist() == [0]  # (the RF call has no such cap)
    finally:
        tabs.free()
    one_less = TreeTables(n_taxa=n, tree_off=np.array([0, n - 1], dtype=np.int64),
                          leaf_taxon=np.arange(n - 1, dtype=np.int32), adj_depth=np.zeros(n - 1, dtype=np.int32),
                          adj_val=np.zeros(n - 1, dtype=np.float64), tree_w=np.ones(1, dtype=np.float64))
    res = dev.score_branch_triplets(one_less, parent, taxon)  # (a star supertree has no quartet branch)
    assert not any(v.any() for v in res.values())


def test_other_terms_do_not_change_with_branch_triplets(dev):
    rs = np.random.RandomState(12)
    names = _names(500)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    objects = [qr.planted(rs, sup, names, 0.3, 6, 0.2) for _ in range(40)]
    arrays = _arrays(objects, 500)
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, triplets=True, conflicts=True, concordance=True, device=dev)
        full = score_supertree(sup, trees, triplets=True, conflicts=True, concordance=True, branch_triplets=True,
                               device=dev)
        assert plain.bt_total is None and plain.n_bt_total is None and "branch_triplets" not in plain.timings
        assert sorted(full.timings) == sorted([*plain.timings, "branch_triplets"])
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super",
                  "t_source", "t_shared", "n_super_conflict", "n_source_conflict", "conflicting", "n_decisive",
                  "n_concordant", "n_alternative", "decisive", "concordant", "alt1", "alt2"):
            assert np.array_equal(getattr(plain, k), getattr(full, k)), k
        assert plain.table() == "\n".join(line.rsplit("\t", 3)[0] for line in full.table().splitlines()) + "\n"
        assert full.table().splitlines()[0].endswith("\tn_bt_total\tn_bt_concordant\tn_bt_alternative")
        assert plain.branch_table() == "\n".join(x.rsplit("\t", 4)[0] for x in full.branch_table().splitlines()) + "\n"
        assert plain.nni_candidates() == full.nni_candidates()
        # the relations that tie the counts to the other terms, elementwise
        assert (full.bt_concordant + full.bt_alt1 + full.bt_alt2 <= full.bt_total).all()
        assert np.array_equal(full.bt_total > 0, full.decisive > 0)
        assert (full.n_bt_total <= full.t_super).all() and (full.n_bt_concordant <= full.t_shared).all()
        assert (full.bt_alt1 + full.bt_alt2).any() and full.bt_fan.any()
        only = score_supertree(sup, trees, branch_triplets=True, device=dev)
        for k in KEYS:
            assert np.array_equal(getattr(only, k), getattr(full, k)), k
        assert only.decisive is None and only.conflicting is None and only.t_shared is None


def test_cli_columns_and_files(tmp_path):
    src = DATA_DIR / "supertriplets_source.tre"
    out, tsv, plain_tsv = tmp_path / "out.tre", tmp_path / "scores.tsv", tmp_path / "plain.tsv"
    branches, named = tmp_path / "branches.tsv", tmp_path / "branch_triplets.tre"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(tsv), "--concordance",
                                   "--branch-triplets", "--branch-triplets-out", str(named), "--branches-out",
                                   str(branches)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src), concordance=True, branch_triplets=True)
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0][6:] == ["n_decisive", "n_concordant", "n_alternative", "n_bt_total", "n_bt_concordant",
                           "n_bt_alternative"]
    got = np.array([[int(x) for x in r[9:]] for r in rows[1:]], dtype=np.int64)
    assert np.array_equal(got, np.stack([api.n_bt_total, api.n_bt_concordant, api.n_bt_alternative], axis=1))
    assert tsv.read_text() == api.table()
    rows = [line.split("\t") for line in branches.read_text().splitlines()]
    assert rows[0][9:] == ["bt_total", "bt_concordant", "bt_alt1", "bt_alt2"]
    got = np.array([[int(x) for x in r] for r in rows[1:]], dtype=np.int64)
    at = np.flatnonzero(api.quartet_branch)
    assert np.array_equal(got[:, 0], at)
    assert np.array_equal(got[:, 9:], np.stack([api.bt_total[at], api.bt_concordant[at], api.bt_alt1[at],
                                                api.bt_alt2[at]], axis=1)) and api.bt_alt1.any()
    assert named.read_text().strip() == api.annotate_branch_triplets().get_newick(with_node_names=True)
    names = [v.name for v in sr._preorder(load_tree(named)) if not v.is_tip() and v.name]
    assert len(names) == int((api.bt_total > 0).sum()) > 0 and all(len(x.split("/")) == 4 for x in names)
    # without --branch-triplets the tables keep the columns of before, also when only the named tree is asked for
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(plain_tsv), "--branches-out",
                                   str(branches), "--branch-triplets-out", str(named)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src), concordance=True, branch_triplets=True)
    assert plain_tsv.read_text().splitlines()[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf"
    assert branches.read_text().splitlines()[0].endswith("\talt2\tother")
    assert named.read_text().strip() == api.annotate_branch_triplets().get_newick(with_node_names=True)


def test_symbol_and_abi_version():
    lib = _native.load_library()
    assert lib.scs_version() == 109 == _native.ABI_VERSION
    assert isinstance(lib.scs_score_branch_triplets, ctypes._CFuncPtr)
    assert "scs_score_branch_triplets" in _native.SIGNATURES
