"""Pairwise source-tree distances on the device (``scs_score_source_pairs``) held exactly to the
references of ``tests/source_pairs_reference.py``: few and no common taxa, trees of one and two leaves, chains that
collapse onto one set, stars and caterpillars, overlaps around the wave, the workgroup scan and the block tables,
the same through the slab, a pair past LDS and the two entry widths, batches on both axes, chosen rows, null outputs,
a grid past 65 535, the counts ``scs_score_supertree`` shares with it, the refusals, and the way through
``source_distances`` and the command line."""

import random
from functools import lru_cache
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest
import source_pairs_reference as sp

from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, load_trees, source_distances
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.load import load_tree_arrays

pytestmark = pytest.mark.gpu

DATA = Path(__file__).parent / "golden" / "reference_data"
SLAB = 256  # max_lds_bytes that leaves room for pairs of a few leaves only: the others take the slab


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what) -> None:
    for k in sp.KEYS:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape, (what, k)
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (what, k, bad[:6].tolist(), got[k][got[k] != ref[k]][:6], ref[k][got[k] != ref[k]][:6])


def _n_source(dev, tabs, n_taxa: int) -> np.ndarray:
    parent, taxon = pr.preorder_arrays(list(range(n_taxa)) if n_taxa > 1 else 0)
    return dev.score(tabs, parent, taxon)["n_source"]


def _check(dev, trees, n_taxa, ref=None, rows=None, batches=(0,), lds=(0, SLAB), what="", tables=None) -> dict:
    """Every setting against the reference; the full matrix also against the invariants."""
    tables = pr.tables(trees, n_taxa) if tables is None else tables
    if ref is None:
        ref = sp.by_sets(trees, rows) if tables.tree_off[-1] <= 400 else sp.linear(tables, rows)
    tabs = dev.upload(tables)
    try:
        for bt in batches:
            for cap in lds:
                got = dev.score_source_pairs(tabs, rows, batch_trees=bt, lds_bytes=cap)
                _same(got, ref, (what, bt, cap))
                if rows is None:
                    sp.check_invariants(got, _n_source(dev, tabs, n_taxa))
    finally:
        tabs.free()
    return ref


# ------------------------------------------------------------------------------------------------ few common taxa
def test_zero_to_three_common_taxa_and_trees_of_one_and_two_leaves(dev):
    trees = [[[0, 1], [2, [3, 4]]],      # 0
             [[5, 6], [7, 8]],           # 1: disjoint from 0
             [[0, 5], [9, 10]],          # 2: one taxon of 0, one of 1
             [[0, 1], [6, 7]],           # 3: two of 0, two of 1
             [[0, [1, 2]], [5, 11]],     # 4: three of 0
             [[1, 2], 0],                # 5: three of 0, another shape
             3,                          # 6: one leaf
             [3, 4],                     # 7: two leaves
             [[0, 1], [2, [3, 4]]],      # 8: identical to 0
             [[0, 1], 2]]                # 9: a subset of 0 (A ⊂ B)
    ref = _check(dev, trees, 12, batches=(0, 1, 3))
    assert ref["common"][0].tolist() == [5, 0, 1, 2, 3, 3, 1, 2, 5, 3]
    assert ref["shared"][0, 8] == ref["clusters"][0, 0] == 3 and ref["shared"][0, 9] == 1 and ref["clusters"][0, 9] == 1
    assert ref["shared"][0, 4] == 0 and ref["clusters"][0, 4] == 1 and ref["clusters_other"][0, 4] == 1
    assert ref["shared"][4, 5] == 1 and not ref["clusters"][6].any() and not ref["clusters"][:, 7].any()


def test_a_restriction_collapses_a_chain_of_nodes_onto_one_set(dev):
    # {a,b} sits on three nodes of tree 0 restricted to {a,b,c,d}; unary chains above the root and inside
    trees = [[[[[[0, 9], 1], 8], 7], [2, 3]], [[0, 1], [2, 3]], [[[[[0, 1]]], [[2, 3]]]], [[0, 2], [1, 3]],
             [[[[0, 9], 8], 7], 1, 2]]
    ref = _check(dev, trees, 10, batches=(0, 2))
    assert ref["clusters"][0, 1] == 2 and ref["shared"][0, 1] == 2 and ref["clusters"][2, 1] == 2
    assert ref["shared"][2, 1] == 2 and ref["shared"][0, 3] == 0 and ref["clusters"][4, 1] == 0


def test_depths_past_16_bits_in_a_small_tree(dev):
    # a chain of unary nodes above a clade is as deep as it likes: the lists hold positions, never depths
    rng = random.Random(4)
    trees = [pr.rand_tree(rng.sample(range(90), 70), 3, rng) for _ in range(4)]
    tables = pr.tables(trees, 90)
    off = tables.tree_off
    tables.adj_depth[off[1]:off[2]] += 1 << 20
    deep = tables.adj_depth[off[2]:off[3]]
    deep[deep >= 2] += 70000
    _check(dev, trees, 90, ref=sp.by_sets(trees), tables=tables, what="deep")


# ------------------------------------------------------------------------------------------------ shapes
def test_stars_caterpillars_and_polytomies(dev):
    rng = random.Random(7)
    n = 150
    order = list(range(n))
    rng.shuffle(order)
    trees = [list(range(n)), pr.caterpillar(range(n), True), pr.caterpillar(range(n), False),
             pr.caterpillar(order, True), pr.caterpillar(order[:97], False), pr.rand_tree(range(n), 9, rng),
             pr.rand_tree(order[20:], 5, rng), pr.rand_tree(range(0, n, 2), 2, rng), list(range(40, 110))]
    ref = _check(dev, trees, n, ref=sp.linear(pr.tables(trees, n)), batches=(0, 4))
    assert ref["shared"][1, 2] == 0 and ref["clusters"][1, 2] == n - 2 and not ref["clusters"][0].any()
    assert ref["shared"][5, 5] == ref["clusters"][5, 5] > 0 and ref["common"][4, 8] > 0


def _overlap_pair(c: int, seed: int):
    """Two trees with exactly c common taxa (and a few of their own) that share some clades and not others: the second
    is the first restricted to the common taxa, a tenth of them swapped among themselves, beside taxa of its own."""
    rng = random.Random(seed)
    extra = max(3, c // 10)
    a = pr.rand_tree(range(c + extra), 4, rng)
    moved = rng.sample(range(c), max(2, c // 10))
    to = dict(zip(moved, moved[1:] + moved[:1]))

    def swapped(tree):
        return [swapped(x) for x in tree] if isinstance(tree, list) else to.get(tree, tree)

    b = [swapped(pr.restrict(a, set(range(c)))), pr.rand_tree(range(c + extra, c + 2 * extra), 3, rng)]
    return [a, b], c + 2 * extra


@lru_cache(maxsize=None)
def _overlap_case(c: int):
    trees, n = _overlap_pair(c, 500 + c)
    tables = pr.tables(trees, n)
    ref = sp.linear(tables)
    assert ref["common"][0, 1] == c and 0 < ref["shared"][0, 1] < min(ref["clusters"][0, 1], ref["clusters_other"][0, 1])
    return trees, n, tables, ref


@pytest.mark.parametrize("c", [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097])
def test_overlaps_around_the_wave_the_scan_and_the_block_tables_in_lds_and_through_the_slab(dev, c):
    trees, n, tables, ref = _overlap_case(c)
    _check(dev, trees, n, ref=ref, tables=tables, lds=(0, SLAB, 8192), what=c)
    plan = backend.debug_source_pairs_plan(tables.tree_off, n, lds_bytes=SLAB)
    assert plan["slab"][0, 0] == 1 and plan["slab_stride"] > SLAB and plan["width"][0, 0] == 2


def test_caterpillars_of_4097_leaves_against_each_other(dev):
    # the longest stretches and the clusters that span every block of the min / max tables
    n = 4097
    rng = random.Random(41)
    order = list(range(n))
    rng.shuffle(order)
    near = list(range(n))
    for i in range(0, n - 1, 97):
        near[i], near[i + 1] = near[i + 1], near[i]
    trees = [pr.caterpillar(range(n), True), pr.caterpillar(near, True), pr.caterpillar(range(n), False),
             pr.caterpillar(order, True)]
    ref = _check(dev, trees, n, what="caterpillars")
    assert ref["shared"][0, 1] > n // 2 and ref["shared"][0, 2] == 0 and ref["clusters"][0, 3] == n - 2


# ------------------------------------------------------------------------------------------------ past LDS, entry widths
def test_a_pair_past_lds_runs_from_the_slab(dev):
    trees, n = _overlap_pair(69000, 9)
    tables = pr.tables(trees, n)
    assert min(np.diff(tables.tree_off)) >= 70000
    plan = backend.debug_source_pairs_plan(tables.tree_off, n)
    assert plan["width"][0, 0] == 4 and plan["slab"][0, 0] == 1 and plan["need"][0, 0] > sp.TP_LDS_MAX
    ref = _check(dev, trees, n, tables=tables, lds=(0,), what="70 000 leaves")
    assert ref["common"][0, 1] == 69000 and 0 < ref["shared"][0, 1] < ref["clusters"][0, 1]


def test_the_entry_width_changes_at_65536_leaves(dev):
    rng = random.Random(65536)
    n = 65536
    base = pr.rand_tree(range(n), 3, rng)
    trees = [pr.restrict(base, set(range(n - 1))), pr.rand_tree(range(1, n), 2, rng), base]
    tables = pr.tables(trees, n)
    assert np.diff(tables.tree_off).tolist() == [65535, 65535, 65536]
    plan = backend.debug_source_pairs_plan(tables.tree_off, n, batch_trees=1)
    assert plan["width"].tolist() == [[2, 2, 4], [2, 2, 4], [4, 4, 4]] and plan["slab"].all()
    ref = sp.linear(tables, rows=[0, 2])
    assert ref["shared"][0, 2] == ref["clusters"][0, 2] == ref["clusters"][0, 0] > 30000  # (a restriction of `base`)
    tabs = dev.upload(tables)
    try:
        for bt in (0, 1):  # one batch: every pair 32-bit; a tree a batch: the pairs of trees 0 and 1 16-bit
            got = dev.score_source_pairs(tabs, batch_trees=bt)
            sp.check_invariants(got)
            _same({k: got[k][[0, 2]] for k in sp.KEYS}, ref, ("width", bt))
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ batches, rows, outputs
@lru_cache(maxsize=None)
def _mixed_case():
    rng = random.Random(77)
    n = 700
    sizes = [700, 3, 130, 1, 515, 64, 2]
    trees = [pr.rand_tree(rng.sample(range(n), s), rng.choice([2, 3, 6]), rng) for s in sizes]
    trees = [t[0] if len(t) == 1 else t for t in trees]
    tables = pr.tables(trees, n)
    return trees, n, tables, sp.linear(tables)


def test_batches_of_one_two_and_all_trees_on_both_axes(dev):
    trees, n, tables, ref = _mixed_case()
    _check(dev, trees, n, ref=ref, tables=tables, batches=(1, 2, 0, 7, 100), lds=(0, SLAB, 4096), what="mixed")
    plan = backend.debug_source_pairs_plan(tables.tree_off, n, batch_trees=2)
    assert plan["bstart"].tolist() == [0, 2, 4, 6, 7] and plan["lds"].shape == (4, 4)


def test_every_workgroup_size_gives_the_same_counts(dev, monkeypatch):
    # by default the size follows the tile's LDS (256 here, 1 024 for the caterpillars of 4 097 leaves); the probe
    # switch sets it for every tile
    trees, n, tables, ref = _mixed_case()
    assert backend.debug_source_pairs_plan(tables.tree_off, n)["threads"].tolist() == [[256]]
    for threads in (256, 512, 1024):
        monkeypatch.setenv("SCS_SP_THREADS", str(threads))
        assert backend.debug_source_pairs_plan(tables.tree_off, n)["threads"].tolist() == [[threads]]
        _check(dev, trees, n, ref=ref, tables=tables, batches=(0, 2), lds=(0, SLAB), what=threads)


def test_rows_as_a_subset_reordered_and_repeated(dev):
    trees, n, tables, ref = _mixed_case()
    for rows in ([4], [6, 0, 3], [2, 2, 5, 0, 2], list(range(7)), list(range(6, -1, -1))):
        want = {k: ref[k][rows] for k in sp.KEYS}
        _check(dev, trees, n, ref=want, rows=rows, tables=tables, batches=(0, 2, 3), what=rows)
    tabs = dev.upload(tables)
    try:
        assert dev.score_source_pairs(tabs, rows=[])["common"].shape == (0, 7)
    finally:
        tabs.free()


def test_null_outputs_are_left_out(dev):
    trees, n, tables, ref = _mixed_case()
    tabs = dev.upload(tables)
    try:
        for given in ((), ("shared",), ("common", "clusters_other"), ("clusters",), sp.KEYS):
            for rows in (None, [5, 0]):
                got = dev.score_source_pairs(tabs, rows, batch_trees=3, outputs=given)
                for k in sp.KEYS:
                    if k in given:
                        assert np.array_equal(got[k], ref[k] if rows is None else ref[k][rows]), (given, rows, k)
                    else:
                        assert got[k] is None
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ many pairs
def test_300_small_trees_a_grid_past_65535(dev):
    rng = random.Random(300)
    kinds = [pr.rand_tree(rng.sample(range(14), rng.randint(1, 14)), 3, rng) for _ in range(30)]
    kinds = [t[0] if len(t) == 1 else t for t in kinds]
    small = sp.by_sets(kinds)
    pick = [rng.randrange(30) for _ in range(300)]
    ref = {k: small[k][np.ix_(pick, pick)] for k in sp.KEYS}
    trees = [kinds[i] for i in pick]
    _check(dev, trees, 14, ref=ref, batches=(0, 128), lds=(0, 128), what="300 trees")
    rows = list(range(299, -1, -1))  # (chosen rows: every one of the 90 000 cells from its own workgroup)
    _check(dev, trees, 14, ref={k: ref[k][rows] for k in sp.KEYS}, rows=rows, lds=(0,), what="300 rows")


def test_more_cells_than_one_launch_holds(dev, monkeypatch):
    # 2 100 trees in workgroups of 1 024 threads: 4.41 million cells, past the 4 194 303 workgroups whose work-items a
    # dispatch can count, so the tile takes several launches, with the mirror and with a workgroup per cell
    monkeypatch.setenv("SCS_SP_THREADS", "1024")
    rng = random.Random(2100)
    kinds = [pr.rand_tree(rng.sample(range(9), rng.randint(1, 9)), 3, rng) for _ in range(25)]
    kinds = [t[0] if len(t) == 1 else t for t in kinds]
    small = sp.by_sets(kinds)
    pick = [rng.randrange(25) for _ in range(2100)]
    trees = [kinds[i] for i in pick]
    tables = pr.tables(trees, 9)
    plan = backend.debug_source_pairs_plan(tables.tree_off, 9)
    assert plan["threads"].tolist() == [[1024]] and plan["rows_per_launch"][0, 0] < 2100 and len(plan["bstart"]) == 2
    tabs = dev.upload(tables)
    try:
        got = dev.score_source_pairs(tabs)
        _same(got, {k: small[k][np.ix_(pick, pick)] for k in sp.KEYS}, "2 100 trees")
        rows = list(range(2099, -1, -1))
        got = dev.score_source_pairs(tabs, rows=rows, outputs=("shared", "common"))
        assert got["clusters"] is None and np.array_equal(got["shared"], small["shared"][np.ix_(pick[::-1], pick)])
        assert np.array_equal(got["common"], small["common"][np.ix_(pick[::-1], pick)])
    finally:
        tabs.free()


def test_300_taxa_and_40_partial_trees(dev):
    rng = random.Random(40)
    base = pr.rand_tree(range(300), 3, rng)
    trees = []
    for i in range(40):
        held = set(rng.sample(range(300), rng.randint(3, 300)))
        trees.append(pr.restrict(base, held) if i % 2 else pr.rand_tree(sorted(held), 4, rng))
    ref = _check(dev, trees, 300, ref=sp.linear(pr.tables(trees, 300)), batches=(0, 7), what="partial")
    odd = np.arange(1, 40, 2)
    sub = ref["shared"][np.ix_(odd, odd)]  # restrictions of one tree agree wherever they overlap
    assert np.array_equal(sub, ref["clusters"][np.ix_(odd, odd)]) and sub.max() > 50


def test_a_tree_over_all_taxa_scores_like_the_supertree_export(dev):
    rng = random.Random(14)
    n = 400
    sup = pr.rand_tree(range(n), 4, rng)
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(1, n)), 3, rng) for _ in range(25)]
    trees = [t[0] if len(t) == 1 else t for t in trees]
    parent, taxon = pr.preorder_arrays(sup)
    tabs = dev.upload(pr.tables([*trees, sup], n))
    try:
        got = dev.score_source_pairs(tabs, rows=[25], batch_trees=6)
    finally:
        tabs.free()
    tabs = dev.upload(pr.tables(trees, n))
    try:
        want = dev.score(tabs, parent, taxon)
    finally:
        tabs.free()
    assert np.array_equal(got["clusters"][0, :25], want["n_super"])
    assert np.array_equal(got["clusters_other"][0, :25], want["n_source"])
    assert np.array_equal(got["shared"][0, :25], want["shared"]) and want["shared"].sum() > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_messages(dev):
    tabs = dev.upload(pr.tables([[[0, 1], 2], [[1, 2], 3], [0, 3]], 4))
    twice = dev.upload(pr.tables([[[0, 1], 2], [[0, 1], 0]], 4))
    try:
        for rows, said in (([3], r"rows\[0\] = 3 is not a tree of the tables \(3 trees\)"),
                           ([0, -1], r"rows\[1\] = -1 is not a tree")):
            with pytest.raises(ValueError, match="scs_score_source_pairs: " + said):
                dev.score_source_pairs(tabs, rows=rows)
        with pytest.raises(ValueError, match="scs_score_source_pairs: max_lds_bytes = -1 is negative"):
            dev.score_source_pairs(tabs, lds_bytes=-1)
        lib, buf = dev._lib, np.zeros(9, dtype=np.int32)
        rows = np.zeros(3, dtype=np.int32)
        for n_rows, row_ptr, said in ((-1, rows.ctypes.data, b"n_rows = -1 is negative"),
                                      (2, None, b"rows is null and n_rows = 2 is not the 3 trees of the tables")):
            assert lib.scs_score_source_pairs(dev._ctx, tabs._h, n_rows, row_ptr, 0, 0, buf.ctypes.data, None, None,
                                              None) == nv.EINVAL
            assert lib.scs_last_error() == b"scs_score_source_pairs: " + said
        assert lib.scs_score_source_pairs(dev._ctx, None, 0, None, 0, 0, None, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_source_pairs: null argument"
        # a taxon twice in a tree: found on the device before a pair is counted, whichever rows are asked for
        for rows in (None, [0]):
            with pytest.raises(ValueError, match="^scs_score_source_pairs: a source tree has a taxon twice$"):
                dev.score_source_pairs(twice, rows=rows)
        # a taxon out of range never gets as far: the upload refuses it with the words the exports use
        with pytest.raises(ValueError, match=r"a leaf_taxon entry is out of range \[0, n_taxa\)"):
            dev.upload(pr.tables([[[0, 1], 4]], 4))
        # and a good call still works afterwards
        _same(dev.score_source_pairs(tabs), sp.by_sets([[[0, 1], 2], [[1, 2], 3], [0, 3]]), "after")
    finally:
        tabs.free()
        twice.free()


# ------------------------------------------------------------------------------------------------ API and CLI
def _dcm_reference(path):
    trees = load_trees(str(path))
    names: dict = {}
    for t in trees:
        for name in t.get_tip_names():
            names.setdefault(name, len(names))
    nested = [pr.from_treenode(t, names) for t in trees]
    return trees, sp.linear(pr.tables(nested, len(names)))


def test_source_distances_on_the_dcm_sources_as_trees_and_as_arrays(dev):
    path = DATA / "dcm_source_trees.tre"
    trees, ref = _dcm_reference(path)
    res = source_distances(trees, device=dev)
    _same({k: getattr(res, k) for k in sp.KEYS}, ref, "dcm trees")
    sp.check_invariants({k: getattr(res, k) for k in sp.KEYS})
    assert np.array_equal(res.rf, ref["clusters"].astype(np.int64) + ref["clusters_other"] - 2 * ref["shared"])
    # (the DCM sources are restrictions of one model tree: they agree wherever they overlap)
    assert res.shared.any() and not res.rf.any() and (res.common >= 4).sum() > len(trees) and "pairs" in res.timings
    arrays = source_distances(load_tree_arrays(str(path)), device=dev)
    _same({k: getattr(arrays, k) for k in sp.KEYS}, ref, "dcm arrays")
    rows = [7, 0, 30]
    part = source_distances(load_tree_arrays(str(path)), rows=rows, device=dev)
    _same({k: getattr(part, k) for k in sp.KEYS}, {k: ref[k][rows] for k in sp.KEYS}, "dcm rows")
    mean, comparable = res.mean_distance()
    worst = res.outlier_sources(3)
    assert len(worst) == 3 and worst[0]["mean_distance"] == np.nanmax(mean) and comparable.max() > 0
    assert res.table() == arrays.table() and len(res.table().splitlines()) == 1 + int((np.triu(res.common, 1) >= 3).sum())


def test_the_command_line_writes_the_pair_table(tmp_path):
    src = DATA / "supertriplets_source.tre"
    out, pairs, close, other = (tmp_path / x for x in ("out.tre", "pairs.tsv", "close.tsv", "other.tre"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--source-distances-out", str(pairs)])
    assert res.exit_code == 0, res.output
    api = source_distances(load_trees(str(src)))
    assert pairs.read_text() == api.table() and len(pairs.read_text().splitlines()) > 1
    assert pairs.read_text().splitlines()[0].split("\t") == ["tree_a", "tree_b", "common", "clusters_a", "clusters_b",
                                                             "shared", "rf", "normalized_rf"]
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--source-distances-out", str(close),
                                   "--min-common", "5"])
    assert res.exit_code == 0, res.output
    assert close.read_text() == api.table(5)
    # without the flag: the files of before and no other
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(other)])
    assert res.exit_code == 0 and sorted(p.name for p in tmp_path.iterdir()) == ["close.tsv", "other.tre", "out.tre",
                                                                                 "pairs.tsv"]
