"""Branch concordance counts on the device (``scs_score_concordance``), held to the host reference of
``tests/concordance_reference.py`` and to closed forms by exact equality."""

import ctypes

import numpy as np
import pytest
import concordance_reference as qr
import conflict_reference as cr
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
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

KEYS = (*qr.PER_TREE, *qr.PER_NODE)


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64, (what, k)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:10])
    assert np.array_equal(res.quartet_branch, ref["quartet_branch"]), what


def _sums(ref) -> dict:
    out = {k: int(ref[k].sum()) for k in qr.PER_NODE}
    out["other"] = out["decisive"] - out["concordant"] - out["alt1"] - out["alt2"]
    return out


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _arrays(trees, n_taxa: int) -> TreeArrays:
    return TreeArrays.from_trees(trees, [1.0] * len(trees), _names(n_taxa))


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(29)
    total = {"decisive": 0, "concordant": 0, "alt1": 0, "alt2": 0, "other": 0}
    for i in range(150):
        sup, trees = sr.random_case(rs)
        ref = qr.brute_force(sup, trees)
        _same(score_supertree(sup, trees, concordance=True, device=dev), ref, i)
        for k, v in _sums(ref).items():
            total[k] += v
    assert (total["decisive"], total["concordant"], total["alt1"], total["alt2"]) == (195, 11, 12, 11), total


@pytest.mark.parametrize(("sup_file", "src_file", "want"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre", None),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre", None),
    ("supertriplets_expected.tre", "supertriplets_source.tre",
     {"decisive": 3464, "concordant": 2596, "alt1": 157, "alt2": 193, "other": 518}),
])
def test_reference_fixtures(dev, sup_file, src_file, want):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    ref = qr.brute_force(sup, trees)
    if want is None:  # the dcm pairs: every decisive source is concordant; some informative ones are not decisive
        assert np.array_equal(ref["decisive"], ref["concordant"]) and ref["decisive"].sum() == 1100
        assert int((ref["decisive"] < sr.linear(sup, trees)["informative"]).sum()) == 4
    else:
        assert _sums(ref) == want
    _same(score_supertree(sup, trees, concordance=True, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), concordance=True, device=dev), ref, sup_file)


@pytest.mark.parametrize(("n_taxa", "n_trees", "frac", "moves", "share", "extra"), [
    (200, 60, 1.0, 6, 0.2, 0),      # full coverage
    (2000, 40, 0.05, 4, 0.2, 0),    # partial coverage: many informative sources are not decisive
    (3000, 3, 1.0, 60, 0.2, 0),     # large trees
    (400, 30, 0.5, 5, 0.2, 150),    # a supertree with taxa no source has
])
def test_planted_forests_match_brute_force(dev, n_taxa, n_trees, frac, moves, share, extra):
    rs = np.random.RandomState(n_taxa + 11)
    names = _names(n_taxa)
    sup = cr.contract(sr.random_tree(rs, _names(n_taxa + extra), binary=True), rs, 0.1)
    shown = sup.get_sub_tree(names) if extra else sup
    trees = [qr.planted(rs, shown, names, frac, moves, share) for _ in range(n_trees)]
    ref = qr.brute_force(sup, trees)
    sums = _sums(ref)
    print("planted", n_taxa, n_trees, sums)
    # (not a measurement: a classifier that returns zeros must not pass)
    assert min(sums["concordant"], sums["alt1"], sums["alt2"], sums["other"]) > 0, sums
    res = score_supertree(sup, trees, concordance=True, conflicts=True, device=dev)
    _same(res, ref, (n_taxa, n_trees))
    assert "concordance" in res.timings
    assert (res.decisive <= res.informative).all() and (res.concordant <= res.supported).all()
    assert (res.alt1 + res.alt2 <= res.conflicting).all() and (res.other >= 0).all()
    if frac < 1.0:
        assert (res.decisive < res.informative).any()
    _same(score_supertree(sup, _arrays(trees, n_taxa + extra), concordance=True, device=dev), ref, "arrays")


def test_copies_of_a_binary_supertree_are_concordant_everywhere(dev):
    rs = np.random.RandomState(5)
    sup = sr.random_tree(rs, _names(300), binary=True)
    res = score_supertree(sup, [sup.copy() for _ in range(5)], concordance=True, device=dev)
    inner = np.array([i > 0 and not v.is_tip() for i, v in enumerate(sr._preorder(sup))])
    assert np.array_equal(res.quartet_branch, inner)
    assert np.array_equal(res.decisive, 5 * inner) and np.array_equal(res.concordant, res.decisive)
    assert not res.alt1.any() and not res.alt2.any() and not res.other.any()
    assert res.n_decisive.tolist() == res.n_concordant.tolist() == [int(inner.sum())] * 5
    assert res.n_alternative.tolist() == [0] * 5 and res.nni_candidates() == []
    assert np.array_equal(res.gcf[inner], np.full(int(inner.sum()), 100.0)) and np.isnan(res.gcf[~inner]).all()


@pytest.mark.parametrize("which", ["alt1", "alt2"])
def test_one_interchange_is_one_alternative_at_its_branch(dev, which):
    rs = np.random.RandomState(6)
    sup = sr.random_tree(rs, _names(200), binary=True)
    nodes = sr._preorder(sup)
    branches = [i for i, v in enumerate(nodes) if i > 0 and not v.is_tip()]
    at = branches[len(branches) // 2]
    moved = sup.copy()
    c = sr._preorder(moved)[at]
    par = c.parent
    j = 1 - par.children.index(c)
    i = 1 if which == "alt1" else 0  # alt1 = (A ∪ D): B changes places with D; alt2 = (B ∪ D): A does
    c.children[i], par.children[j] = par.children[j], c.children[i]
    c.children[i].parent, par.children[j].parent = c, par
    res = score_supertree(sup, [moved, sup.copy()], concordance=True, device=dev)
    _same(res, qr.brute_force(sup, [moved, sup.copy()]), which)
    want = np.zeros(len(nodes), dtype=np.int64)
    want[at] = 1
    assert np.array_equal(getattr(res, which), want)
    assert not getattr(res, "alt2" if which == "alt1" else "alt1").any() and not res.other.any()
    assert np.array_equal(res.concordant, res.decisive - want) and res.decisive[at] == 2
    assert res.n_alternative.tolist() == [1, 0]
    assert res.nni_candidates() == []  # (one source each way: no alternative is ahead)
    res = score_supertree(sup, [moved, moved.copy(), sup.copy()], concordance=True, device=dev)
    assert res.nni_candidates() == [{"node": at, "alternative": which, "decisive": 3, "concordant": 1,
                                     "alt1": 2 * (which == "alt1"), "alt2": 2 * (which == "alt2"), "margin": 1}]
    named = [v.name for v in sr._preorder(res.annotate_concordance()) if not v.is_tip()]
    assert named[0] is None and named[branches.index(at) + 1] == ("1/2/0/3" if which == "alt1" else "1/0/2/3")


def test_star_sources_are_decisive_everywhere_and_display_nothing(dev):
    rs = np.random.RandomState(7)
    names = _names(150)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.2)
    stars = [TreeNode(None, [TreeNode(x) for x in rs.permutation(names)]) for _ in range(4)]
    res = score_supertree(sup, stars, concordance=True, device=dev)
    assert res.quartet_branch.any() and not res.quartet_branch.all()
    assert np.array_equal(res.decisive, 4 * res.quartet_branch) and np.array_equal(res.other, res.decisive)
    assert not res.concordant.any() and not res.alt1.any() and not res.alt2.any()
    assert res.n_decisive.tolist() == [int(res.quartet_branch.sum())] * 4
    assert np.array_equal(res.gdfp[res.quartet_branch], np.full(int(res.quartet_branch.sum()), 100.0))


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for name in names[1:]:
        node = TreeNode(None, [node, TreeNode(name)])
    return node


def test_deep_caterpillar(dev):
    n = 20_000
    names = _names(n)
    cat = _caterpillar(names)
    res = score_supertree(cat, _arrays([_caterpillar(names[::-1]), _caterpillar(names)], n), concordance=True,
                          device=dev)
    # preorder: the inner nodes first (node i holds x0 .. x(n-1-i)), every one but the root a quartet branch with
    # A = x0 .. x(n-2-i), B = x(n-1-i), D = x(n-i).  The reversed caterpillar's clusters are the sets
    # x(j) .. x(n-1): it displays only B ∪ D of node 1, and nothing at any other branch
    mask = np.zeros(2 * n - 1, dtype=bool)
    mask[1:n - 1] = True
    assert np.array_equal(res.quartet_branch, mask)
    assert np.array_equal(res.decisive, 2 * mask) and np.array_equal(res.concordant, 1 * mask)
    assert not res.alt1.any() and np.flatnonzero(res.alt2).tolist() == [1] and res.alt2[1] == 1
    assert res.n_decisive.tolist() == [n - 2, n - 2] and res.n_concordant.tolist() == [0, n - 2]
    assert res.n_alternative.tolist() == [1, 0] and res.other.sum() == n - 3


def test_more_trees_than_one_batch(dev, monkeypatch):
    rs = np.random.RandomState(8)
    names = _names(300)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    trees = [qr.planted(rs, sup, names, 0.4, 5, 0.2) for _ in range(50)]
    whole = score_supertree(sup, trees, concordance=True, device=dev)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    batched = score_supertree(sup, trees, concordance=True, device=dev)
    arrays = score_supertree(sup, _arrays(trees, 300), concordance=True, device=dev)
    ref = qr.brute_force(sup, trees)
    assert ref["alt1"].any() and ref["alt2"].any()
    _same(whole, ref, "one batch")
    _same(batched, ref, "batches of 7")
    _same(arrays, ref, "arrays, batches of 7")


def test_other_terms_do_not_change_with_concordance(dev):
    rs = np.random.RandomState(12)
    names = _names(500)
    sup = cr.contract(sr.random_tree(rs, names, binary=True), rs, 0.1)
    objects = [qr.planted(rs, sup, names, 0.3, 6, 0.2) for _ in range(40)]
    arrays = _arrays(objects, 500)
    for trees in (arrays, objects):
        plain = score_supertree(sup, trees, triplets=True, conflicts=True, device=dev)
        full = score_supertree(sup, trees, triplets=True, conflicts=True, concordance=True, device=dev)
        assert plain.decisive is None and plain.n_decisive is None and "concordance" not in plain.timings
        assert sorted(full.timings) == sorted([*plain.timings, "concordance"])
        for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super",
                  "t_source", "t_shared", "n_super_conflict", "n_source_conflict", "conflicting"):
            assert np.array_equal(getattr(plain, k), getattr(full, k)), k
        assert plain.table() == "\n".join(line.rsplit("\t", 3)[0] for line in full.table().splitlines()) + "\n"
        assert full.table().splitlines()[0].endswith("\tn_decisive\tn_concordant\tn_alternative")
        assert (full.alt1 + full.alt2 <= full.conflicting).all() and (full.alt1 + full.alt2).any()
        assert (full.decisive <= full.informative).all() and (full.concordant <= full.supported).all()
        only = score_supertree(sup, trees, concordance=True, device=dev)
        for k in KEYS:
            assert np.array_equal(getattr(only, k), getattr(full, k)), k
        assert only.conflicting is None and only.t_shared is None


def test_a_source_taxon_missing_from_the_supertree_raises(dev):
    sup = make_tree("((a,b),(c,d));")
    with pytest.raises(ValueError, match="not in the supertree"):
        score_supertree(sup, [make_tree("((a,b),e);")], concordance=True, device=dev)
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),a);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="twice"):
        dev.score_concordance(tables, parent, taxon)
    # taxon ids the supertree's tips do not cover (five taxa, four tips): the device refuses as for scs_score_supertree
    tables = flatten_trees([make_tree("((a,b),e);")], [1.0], "one", taxa=[*tips, "e"])
    with pytest.raises(ValueError, match="supertree lacks"):
        dev.score_concordance(tables, parent, taxon)
    with pytest.raises(ValueError, match="supertree lacks"):
        dev.score(tables, parent, taxon)


def test_cli_branch_table_and_columns(tmp_path):
    src = DATA_DIR / "supertriplets_source.tre"
    out, tsv, plain_tsv = tmp_path / "out.tre", tmp_path / "scores.tsv", tmp_path / "plain.tsv"
    branches, named = tmp_path / "branches.tsv", tmp_path / "concordance.tre"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(tsv), "--concordance",
                                   "--concordance-out", str(named), "--branches-out", str(branches)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_trees(src), concordance=True)
    rows = [line.split("\t") for line in tsv.read_text().splitlines()]
    assert rows[0][6:] == ["n_decisive", "n_concordant", "n_alternative"]
    got = np.array([[int(x) for x in r[6:]] for r in rows[1:]], dtype=np.int64)
    assert np.array_equal(got, np.stack([api.n_decisive, api.n_concordant, api.n_alternative], axis=1))
    rows = [line.split("\t") for line in branches.read_text().splitlines()]
    assert rows[0] == ["node", "clade_size", "informative", "supported", "decisive", "concordant", "alt1", "alt2",
                       "other"]
    got = np.array([[int(x) for x in r] for r in rows[1:]], dtype=np.int64)
    at = np.flatnonzero(api.quartet_branch)
    sizes = np.array([len(v.get_tip_names()) for v in sr._preorder(load_tree(out))], dtype=np.int64)
    want = np.stack([at, sizes[at], api.informative[at], api.supported[at], api.decisive[at], api.concordant[at],
                     api.alt1[at], api.alt2[at], api.other[at]], axis=1)
    assert len(at) > 0 and np.array_equal(got, want) and api.decisive.any()
    assert named.read_text().strip() == api.annotate_concordance().get_newick(with_node_names=True)
    names = [v.name for v in sr._preorder(load_tree(named)) if not v.is_tip() and v.name]
    assert len(names) == len(at) and all(len(x.split("/")) == 4 for x in names)
    # without the new flags: the six columns of before, also when only the branch table is asked for (every run is
    # held to the tree it wrote: the order of a node's children may differ from run to run)
    for extra in ([], ["--branches-out", str(tmp_path / "b2.tsv")]):
        res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(plain_tsv), *extra])
        assert res.exit_code == 0, res.output
        api = score_supertree(load_tree(out), load_trees(src), concordance=True)
        rows = [line.split("\t") for line in plain_tsv.read_text().splitlines()]
        assert rows[0] == ["index", "n_leaves", "n_super", "n_source", "shared", "rf"]
        got = np.array([[int(x) for x in r] for r in rows[1:]], dtype=np.int64)
        want = np.stack([np.arange(len(api.rf)), api.n_leaves, api.n_super, api.n_source, api.shared, api.rf],
                        axis=1)
        assert np.array_equal(got, want)
        if extra:
            assert (tmp_path / "b2.tsv").read_text() == api.branch_table()


def test_abi_version_and_symbol():
    lib = _native.load_library()
    assert lib.scs_version() == 109 == _native.ABI_VERSION
    assert isinstance(lib.scs_score_concordance, ctypes._CFuncPtr)
    assert "scs_score_concordance" in _native.SIGNATURES
