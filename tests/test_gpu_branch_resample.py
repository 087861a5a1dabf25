"""Resampled and weighted branch triplet support on the device (``scs_score_branch_resample``), held entry for entry
to the host reference of ``tests/resample_reference.py`` and to ``scs_score_branch_triplets`` on duplicated trees."""

import numpy as np
import pytest
import branch_triplet_reference as br
import resample_reference as rr
import score_reference as sr
from clade_placement_reference import _restricted
from click.testing import CliRunner
from conflict_reference import contract
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import load_trees, score_supertree
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import TreeTables, flatten_trees
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

LDS_CAP = (160 << 10) // 24 * 32 - 1  # leaves of the largest source tree
BUDGET = 3 << 29                      # bytes of accumulators a call may hold


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


@pytest.fixture(scope="module")
def cases():
    return rr.resample_cases()


@pytest.fixture(scope="module")
def counts(cases):
    return [rr.per_tree(sup, trees) for sup, trees in cases]


def _tables(sup: TreeNode, trees: list) -> tuple:
    parent, taxon, tips = supertree_arrays(sup)
    return flatten_trees(trees, [1.0] * len(trees), "one", taxa=tips), parent, taxon


def _call(dev, sup, trees, weights, rows=True, batch_trees=0) -> dict:
    tables, parent, taxon = _tables(sup, trees)
    tabs = dev.upload(tables)
    try:
        return dev.score_branch_resample(tabs, parent, taxon, weights, rows=rows, batch_trees=batch_trees)
    finally:
        tabs.free()


def _same(got: dict, all_rows: np.ndarray, what="") -> None:
    """``got`` of the device against the reference rows [4][R][nodes] (Python ints), entry for entry."""
    assert got["rs_point"].dtype == np.int64 and got["rs_wins"].dtype == np.int32, what
    assert np.array_equal(got["rs_point"], all_rows[:, 0, :].astype(np.int64)), (what, "rs_point")
    assert np.array_equal(got["rs_wins"], rr.wins(all_rows)), (what, "rs_wins")
    if got["rs_rows"] is not None:
        assert got["rs_rows"].dtype == np.int64
        assert np.array_equal(got["rs_rows"], all_rows.astype(np.int64)), (what, "rs_rows")


def _model_case(rs, n_taxa: int, sizes, share: float = 0.0):
    """A binary supertree on ``n_taxa`` taxa (``share`` of its edges collapsed) and one source per entry of ``sizes``:
    the restriction of another binary tree, half of them of the supertree itself, to that many taxa."""
    names = [f"t{i}" for i in range(n_taxa)]
    model = sr.random_tree(rs, names, binary=True)
    other = sr.random_tree(rs, names, binary=True)
    sup = contract(model, rs, share) if share else model
    trees = [contract(_restricted(model if i % 2 else other, set(rs.choice(names, size=k, replace=False).tolist())),
                      rs, 0.1) for i, k in enumerate(sizes)]
    return sup, trees


# ------------------------------------------------------------------ the reference cases
def test_the_cases_match_the_reference_entry_for_entry(dev, cases, counts):
    rs = np.random.RandomState(7)
    seen = np.zeros(4, dtype=np.int64)
    for i, ((sup, trees), c) in enumerate(zip(cases, counts)):
        w = rr.case_weights(rs, len(trees), 1 + int(rs.randint(1, 12)))
        ref = rr.rows(w, c)
        got = _call(dev, sup, trees, w)
        _same(got, ref, i)
        seen += got["rs_wins"].sum(axis=1)
    print("wins over the cases", seen.tolist())
    assert seen.min() > 0, seen  # (every outcome occurs: a kernel that counts nothing must not pass)


def test_a_row_of_ones_is_the_branch_triplet_call(dev, cases):
    for i, (sup, trees) in enumerate(cases):
        tables, parent, taxon = _tables(sup, trees)
        tabs = dev.upload(tables)
        try:
            bt = dev.score_branch_triplets(tabs, parent, taxon)
            got = dev.score_branch_resample(tabs, parent, taxon, np.ones((1, len(trees)), dtype=np.int64), rows=True)
        finally:
            tabs.free()
        assert np.array_equal(got["rs_point"], np.stack([bt[k] for k in br.PER_NODE])), i
        assert np.array_equal(got["rs_rows"][:, 0, :], got["rs_point"]) and not got["rs_wins"].any(), i


def test_an_integer_weight_is_that_many_uploaded_copies(dev, cases):
    rs = np.random.RandomState(8)
    for i, (sup, trees) in enumerate(cases[:20]):
        w = rs.randint(0, 4, size=len(trees))
        w[int(rs.randint(len(trees)))] = 0
        w[int(rs.randint(len(trees)))] = 3
        tables, parent, taxon = _tables(sup, rr.repeated(trees, w))
        bt = dev.score_branch_triplets(tables, parent, taxon)
        got = _call(dev, sup, trees, np.stack([np.ones_like(w), w]))
        assert np.array_equal(got["rs_rows"][:, 1, :], np.stack([bt[k] for k in br.PER_NODE])), i


# ------------------------------------------------------------------ the edges of the layouts
def test_sources_at_the_bitset_word_edges(dev):
    rs = np.random.RandomState(31)
    sizes = [31, 32, 33, 63, 64, 65, 257]
    sup, trees = _model_case(rs, 300, sizes, share=0.05)
    assert [len(t.get_tip_names()) for t in trees] == sizes
    w = rr.case_weights(rs, len(trees), 4)
    ref = rr.rows(w, rr.per_tree(sup, trees))
    assert min(int(ref[x][0].sum()) for x in range(4)) > 0
    _same(_call(dev, sup, trees, w), ref)
    _same(_call(dev, sup, trees, w, batch_trees=3), ref, "batches of 3")


@pytest.mark.parametrize("n_nodes", [3, 63, 64, 65, 255, 256, 257, 1025])
def test_supertrees_at_the_node_tile_edges(dev, n_nodes):
    rs = np.random.RandomState(n_nodes)
    n_taxa = (n_nodes + 1) // 2 if n_nodes % 2 else n_nodes // 2
    sup, trees = _model_case(rs, n_taxa, [min(n_taxa, k) for k in (2, 12, 40, 90, n_taxa)])
    if n_nodes % 2 == 0:  # (a binary tree has an odd number of nodes: a unary root makes it even)
        sup = TreeNode(None, [sup])
    assert len(sup.to_flat()[0]) == n_nodes
    w = rr.case_weights(rs, len(trees), 10)
    ref = rr.rows(w, rr.per_tree(sup, trees))
    assert (int(ref[0][0].sum()) > 0) == (n_nodes > 3)
    _same(_call(dev, sup, trees, w), ref, n_nodes)


@pytest.fixture(scope="module")
def tile_case():
    rs = np.random.RandomState(17)
    sup, trees = _model_case(rs, 24, [24, 20, 16, 12, 9, 6])
    return sup, trees, rr.per_tree(sup, trees)


@pytest.mark.parametrize("n_rep", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_replicate_counts_around_the_tile(dev, tile_case, n_rep):
    sup, trees, c = tile_case
    w = np.random.RandomState(n_rep).randint(0, 5, size=(n_rep, len(trees)))
    ref = rr.rows(w, c)
    got = _call(dev, sup, trees, w)
    assert got["rs_rows"].shape == (4, n_rep, len(sup.to_flat()[0]))
    _same(got, ref, n_rep)
    assert got["rs_point"].any() == bool(w[0].any()) and (n_rep > 1) >= bool(got["rs_wins"].any())


@pytest.mark.parametrize("batch_trees", [1, 2, 7])
def test_the_accumulators_carry_across_batches(dev, batch_trees):
    rs = np.random.RandomState(40 + batch_trees)
    sup, trees = _model_case(rs, 40, [40, 35, 30, 25, 20, 15, 10, 8, 6], share=0.05)
    w = rr.case_weights(rs, len(trees), 11)
    ref = rr.rows(w, rr.per_tree(sup, trees))
    assert int(ref[0][0].sum()) > 0
    _same(_call(dev, sup, trees, w, batch_trees=batch_trees), ref, batch_trees)


def test_sources_that_decide_nothing_or_weigh_nothing(dev):
    rs = np.random.RandomState(23)
    sup, trees = _model_case(rs, 30, [30, 2, 18, 2, 25])
    cherry = sup
    while not all(k.is_tip() for k in cherry.children):
        cherry = next(k for k in cherry.children if not k.is_tip())
    trees.append(TreeNode(None, [TreeNode(k.name) for k in cherry.children]))  # (inside one child: never decisive)
    c = rr.per_tree(sup, trees)
    assert not c[1].any() and not c[3].any() and not c[5].any() and c[0].any() and c[2].any()
    w = rs.randint(1, 4, size=(6, len(trees)))
    w[:, 2] = 0  # (a decisive source that no row counts)
    w[3, :] = 0  # (a replicate that drew nothing: uninformative everywhere)
    ref = rr.rows(w, c)
    got = _call(dev, sup, trees, w)
    _same(got, ref)
    assert not got["rs_rows"][:, 3, :].any() and got["rs_wins"].sum(axis=0).max() == 4
    # only such sources: zeros
    got = _call(dev, sup, [trees[1], trees[3], trees[5]], np.full((3, 3), 2))
    assert not got["rs_point"].any() and not got["rs_wins"].any() and not got["rs_rows"].any()


def test_a_star_supertree_has_no_branch(dev):
    rs = np.random.RandomState(2)
    names = [f"t{i}" for i in range(70)]
    sup = TreeNode(None, [TreeNode(n) for n in names])
    trees = [sr.random_tree(rs, names[:k], binary=True) for k in (70, 33, 5)]
    got = _call(dev, sup, trees, np.full((9, 3), 3))
    assert got["rs_point"].shape == (4, 71) and got["rs_wins"].shape == (4, 71) and got["rs_rows"].shape == (4, 9, 71)
    assert not got["rs_point"].any() and not got["rs_wins"].any() and not got["rs_rows"].any()


def test_the_rows_stay_on_the_device_unless_asked_for(dev, tile_case):
    sup, trees, c = tile_case
    w = np.random.RandomState(4).randint(0, 5, size=(13, len(trees)))
    got = _call(dev, sup, trees, w, rows=False)
    assert list(got) == ["rs_point", "rs_wins", "rs_rows"] and got["rs_rows"] is None
    _same(got, rr.rows(w, c))


# ------------------------------------------------------------------ what the library refuses
def _star_tables(n: int) -> tuple:
    """One star source of ``n`` leaves and a star supertree on them."""
    tables = TreeTables(n_taxa=n, tree_off=np.array([0, n], dtype=np.int64), leaf_taxon=np.arange(n, dtype=np.int32),
                        adj_depth=np.zeros(n, dtype=np.int32), adj_val=np.zeros(n, dtype=np.float64),
                        tree_w=np.ones(1, dtype=np.float64))
    parent = np.concatenate([[-1], np.zeros(n, dtype=np.int32)]).astype(np.int32)
    taxon = np.concatenate([[-1], np.arange(n, dtype=np.int32)]).astype(np.int32)
    return tables, parent, taxon


def test_the_library_names_the_limit_it_refuses(dev, tile_case):
    sup, trees, _ = tile_case
    tables, parent, taxon = _tables(sup, trees)
    tabs = dev.upload(tables)
    m = len(trees)
    try:
        with pytest.raises(ValueError, match=r"scs_score_branch_resample: n_rep = 0: at least row 0"):
            dev.score_branch_resample(tabs, parent, taxon, np.zeros((0, m), dtype=np.int64))
        w = np.ones((3, m), dtype=np.int64)
        w[2, 4] = -1
        with pytest.raises(ValueError, match=r"scs_score_branch_resample: weights\[2\]\[4\] = -1 is negative"):
            dev.score_branch_resample(tabs, parent, taxon, w)
        with pytest.raises(ValueError, match="a tree weight does not fit int32"):
            dev.score_branch_resample(tabs, parent, taxon, np.full((1, m), 2**31))
        with pytest.raises(ValueError, match="weights one row per replicate with one entry per source tree"):
            dev.score_branch_resample(tabs, parent, taxon, np.ones((2, m + 1), dtype=np.int64))
        # the accumulators: 32 bytes per row and node, within the 1.5 GB of the call's workspace
        n_nodes = len(parent)
        most = BUDGET // (32 * n_nodes)
        with pytest.raises(ValueError, match=rf"the accumulators of {most + 1} rows x {n_nodes} nodes need "
                                             rf"{32 * (most + 1) * n_nodes} bytes, more than the {BUDGET}"):
            dev.score_branch_resample(tabs, parent, taxon, np.zeros((most + 1, m), dtype=np.int32))
    finally:
        tabs.free()


def test_a_tree_above_the_lds_cap_is_refused(dev):
    assert LDS_CAP == 218_431
    tables, parent, taxon = _star_tables(LDS_CAP + 1)
    with pytest.raises(ValueError, match=rf"scs_score_branch_resample: a source tree of {LDS_CAP + 1} leaves is more "
                                         rf"than the {LDS_CAP} the pair kernel holds in LDS"):
        dev.score_branch_resample(tables, parent, taxon, np.ones((1, 1), dtype=np.int64))


def test_a_row_whose_weighted_counts_may_pass_int64_is_refused(dev):
    # one small tree and a weight near 2^31: weight x floor(leaves^3 / 27) must stay within int64
    n = 5000
    cube = n ** 3 // 27
    most = (2 ** 63 - 1) // cube
    assert most < 2 ** 31 - 1
    tables, parent, taxon = _star_tables(n)
    tabs = dev.upload(tables)
    try:
        got = dev.score_branch_resample(tabs, parent, taxon, np.array([[1], [most]]))
        assert not got["rs_point"].any()  # (a star supertree)
        with pytest.raises(ValueError, match=r"scs_score_branch_resample: the weighted triple counts of row 1 may not "
                                             r"fit 64 bits"):
            dev.score_branch_resample(tabs, parent, taxon, np.array([[1], [most + 1]]))
        with pytest.raises(ValueError, match="of row 0 may not fit 64 bits"):
            dev.score_branch_resample(tabs, parent, taxon, np.array([[2 ** 31 - 1], [0]]))
    finally:
        tabs.free()


# ------------------------------------------------------------------ the public interface
@pytest.mark.parametrize("kind", ["bootstrap", "jackknife"])
def test_score_supertree_draws_and_counts_on_both_input_paths(dev, cases, counts, kind):
    for i, ((sup, trees), c) in enumerate(zip(cases[:8], counts)):
        m = len(trees)
        tw = [1 + (t * 7 + i) % 3 for t in range(m)]
        w = rr.draws(m, 30, tw, kind, seed=i)
        ref = rr.rows(w, c)
        res = score_supertree(sup, trees, branch_resample=30, tree_weights=tw, resample=kind, resample_seed=i,
                              resample_rows=True, device=dev)
        assert np.array_equal(res.rs_weights, w) and "branch_resample" in res.timings
        got = {"rs_point": np.stack([res.rs_total, res.rs_concordant, res.rs_alt1, res.rs_alt2]),
               "rs_rows": np.stack([res.rs_total_rows, res.rs_concordant_rows, res.rs_alt1_rows, res.rs_alt2_rows]),
               "rs_wins": np.stack([res.rs_wins[k] for k in rr.WIN_KEYS])}
        _same(got, ref, (kind, i))
        # a TreeArrays input with a one-leaf tree among the sources: its column goes, the others keep their trees
        at = 1 + i % (m - 1)
        given = [*trees[:at], TreeNode(sup.get_tip_names()[0]), *trees[at:]]
        tw2 = [*tw[:at], 5, *tw[at:]]
        w2 = rr.draws(m + 1, 30, tw2, kind, seed=i)
        arrays = TreeArrays.from_trees(given, [1.0] * (m + 1), sup.get_tip_names())
        res = score_supertree(sup, arrays, branch_resample=30, tree_weights=tw2, resample=kind, resample_seed=i,
                              device=dev)
        ref2 = rr.rows(np.delete(w2, at, axis=1), c)
        assert np.array_equal(res.rs_weights, w2) and res.rs_total_rows is None
        got = {"rs_point": np.stack([res.rs_total, res.rs_concordant, res.rs_alt1, res.rs_alt2]), "rs_rows": None,
               "rs_wins": np.stack([res.rs_wins[k] for k in rr.WIN_KEYS])}
        _same(got, ref2, (kind, i, "arrays"))


def test_unweighted_counts_do_not_change_and_ones_agree_with_them(dev, cases):
    sup, trees = cases[0]
    plain = score_supertree(sup, trees, concordance=True, branch_triplets=True, device=dev)
    full = score_supertree(sup, trees, concordance=True, branch_triplets=True, branch_resample=12,
                           tree_weights=[3] * len(trees), device=dev)
    for k in ("n_super", "shared", "informative", "decisive", "concordant", "n_bt_total", *br.PER_NODE):
        assert np.array_equal(getattr(plain, k), getattr(full, k)), k
    assert np.array_equal(full.rs_total, 3 * full.bt_total) and np.array_equal(full.rs_alt1, 3 * full.bt_alt1)
    assert plain.rs_total is None and "branch_resample" not in plain.timings


def test_cli_columns_and_files(tmp_path, dev):
    src = DATA_DIR / "dcm_iq_source.tre"
    out, branches, named = tmp_path / "out.tre", tmp_path / "branches.tsv", tmp_path / "support.tre"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--branches-out", str(branches),
                                   "--branch-resample", "25", "--resample-seed", "3", "--branch-support-out",
                                   str(named)])
    assert res.exit_code == 0, res.output
    api = score_supertree(load_tree(out), load_tree_arrays(src), concordance=True, branch_resample=25,
                          resample_seed=3, device=dev)
    assert np.array_equal(api.rs_weights, rr.draws(len(load_trees(src)), 25, None, "bootstrap", 3))
    rows = [line.split("\t") for line in branches.read_text().splitlines()]
    assert rows[0][9:] == ["win_concordant", "win_alt1", "win_alt2", "win_tie", "support"]
    at = np.flatnonzero(api.quartet_branch)
    assert [int(r[0]) for r in rows[1:]] == at.tolist() and len(at) > 0
    got = np.array([[int(x) for x in r[9:13]] for r in rows[1:]], dtype=np.int64)
    assert np.array_equal(got, np.stack([api.rs_wins[k][at] for k in rr.WIN_KEYS], axis=1)) and got.any()
    assert branches.read_text() == api.branch_table()
    assert named.read_text().strip() == api.annotate_branch_support().get_newick(with_node_names=True)
    # the jackknife draws other replicates; without --branch-resample the table keeps its columns of before
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--branches-out", str(branches),
                                   "--branch-resample", "25", "--resample-seed", "3", "--jackknife"])
    assert res.exit_code == 0, res.output
    jack = score_supertree(load_tree(out), load_tree_arrays(src), concordance=True, branch_resample=25,
                           resample_seed=3, resample="jackknife", device=dev)
    assert branches.read_text() == jack.branch_table() and set(np.unique(jack.rs_weights)) == {0, 1}
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--branches-out", str(branches)])
    assert res.exit_code == 0, res.output
    assert branches.read_text().splitlines()[0].endswith("\talt2\tother")
    for args in (["--branch-resample", "5"], ["--branches-out", str(branches), "--jackknife"],
                 ["--branch-support-out", str(named)]):
        res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), *args])
        assert res.exit_code == 2 and "need" in res.output, res.output
