"""The references and builders of ``tests/forest_reference.py`` (CPU): the plain analysis reference against the host
routines of the product, and every forest of ``tests/test_gpu_forest_edges.py`` against the numbers it is there for --
tree counts, node totals, nodes per workgroup, root-path lengths, universes and leaf counts on either side of a
constant of ``csrc/scs_forest.hip``.  A builder that drifts fails here, not silently on the GPU.
"""

from __future__ import annotations

import numpy as np
import pytest

from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.backend import debug_split_plan
from spectralclustersupertree_amd.treearrays import TreeArrays
from tests import forest_reference as fr
from tests.test_treearrays import random_forest


# ------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("seed", range(6))
def test_analysis_reference_agrees_with_the_host_components(seed):
    # partial coverage by few trees: several components, taxa no tree holds; multifurcations and unary nodes
    taxa, trees, weights = random_forest(seed, 90, 3 + seed)
    arrays = TreeArrays.from_trees(trees, weights, taxa)
    tables = arrays.flatten("depth")
    root, side_sets = fr.analysis_reference(tables)
    # labels 0 .. k - 1 by smallest member <-> the smallest member itself: the same partition, the same roots
    for labels in (fl.pcg_components(tables), fl.pcg_components_numpy(tables)):
        first = np.full(int(labels.max()) + 1, tables.n_taxa, dtype=np.int64)
        np.minimum.at(first, labels, np.arange(tables.n_taxa))
        assert np.array_equal(first[labels], root)
        assert np.array_equal(np.unique(root, return_inverse=True)[1], labels)
    occ = fl.taxa_occurrences(tables)
    assert [len(s) for s in side_sets] == occ.tolist()  # (a taxon occurs once per tree: one side per occurrence)
    absent = np.flatnonzero(occ == 0)
    assert np.array_equal(root[absent], absent)


@pytest.mark.parametrize("seed", range(6))
def test_equal_side_sets_are_the_contraction_groups(seed):
    """``contraction_groups_numpy`` refines by (tree, side) one tree at a time: its classes are the classes of equal
    side sets -- for ALL taxa, the absent ones included (they share the empty set and form one group there).  The
    two definitions part ways in one respect only: the device's signatures, which ``check_signatures`` holds to the
    side sets, say nothing about absent ids beyond ``(0, 0)``; the recursion never asks about them."""
    taxa, trees, weights = random_forest(50 + seed, 70, 2 + seed % 4)
    arrays = TreeArrays.from_trees(trees, weights, taxa)
    tables = arrays.flatten("one")
    _, side_sets = fr.analysis_reference(tables)
    for groups in (fl.contraction_groups_numpy(tables), fl.contraction_groups(tables)):
        assert fr.same_partition(side_sets, groups.tolist())
    equal, distinct = fr.pair_kinds(side_sets)
    assert distinct and (equal or seed % 4 > 1)  # few trees: twins by chance


def test_scan_reference():
    rows = np.asarray([[1, 0, 1, 1], [0, 0, 0, 1]], dtype=np.int32)
    assert fr.scan_reference(0, rows).tolist() == [[0, 1, 1, 2, 3], [0, 0, 0, 0, 1]]
    rows = np.asarray([[-1, 1, -1, 3], [-1, -1, -1, -1]], dtype=np.int32)
    assert fr.scan_reference(1, rows).tolist() == [[-1, -1, 1, 1, 3], [-1, -1, -1, -1, -1]]
    assert fr.scan_reference(0, np.zeros((2, 0), dtype=np.int32)).tolist() == [[0], [0]]
    assert fr.scan_reference(0, rows).dtype == np.int32


def test_same_partition_is_two_sided():
    assert fr.same_partition([1, 1, 2], ["a", "a", "b"])
    assert not fr.same_partition([1, 1, 2], ["a", "b", "b"])  # one class split
    assert not fr.same_partition([1, 2, 3], ["a", "a", "b"])  # two classes merged
    sets = [frozenset({1}), frozenset({1}), frozenset({2}), frozenset()]
    good = np.asarray([[5, 6], [5, 6], [7, 6], [0, 0]], dtype=np.uint64)
    fr.check_signatures(good, sets)
    for bad in ([[5, 6], [5, 7], [7, 6], [0, 0]], [[5, 6], [5, 6], [5, 6], [0, 0]], [[5, 6], [5, 6], [7, 6], [1, 0]],
                [[0, 0], [0, 0], [0, 0], [0, 0]]):  # all zero: what the one-sided assertion let through
        with pytest.raises(AssertionError):
            fr.check_signatures(np.asarray(bad, dtype=np.uint64), sets)


# --------------------------------------------------------------------------------------------- the builders
def test_tree_shapes_hit_their_node_counts():
    rng = np.random.RandomState(0)
    for k in (2, 3, 4, 19, 150):
        assert len(fr.tree_shape(rng, k)[0]) == 2 * k - 1
        assert len(fr.tree_shape(rng, k, "unary")[0]) == 2 * k
        if k >= 3:
            par, leaf = fr.tree_shape(rng, k, "tri")
            assert len(par) == 2 * k - 2 and np.count_nonzero(par == 0) == 3
    arrays = fr.build_forest(1, 60, [2, 3, 7, 30, 30, 5], extras={1: "tri", 3: "unary"}, combs=[4], neg_len=0.3,
                             nan_len=0.3)
    fr.well_formed(arrays)
    assert np.diff(arrays.node_off).tolist() == [3, 4, 13, 60, 59, 9]
    assert arrays.leaf_counts().tolist() == [2, 3, 7, 30, 30, 5]
    assert fr.max_inner_depth(arrays, 4) == 28
    inner = arrays.taxon < 0
    assert np.any(arrays.length[inner] < 0) and np.any(np.isnan(arrays.length[inner][1:]))  # the monotone flag matters


@pytest.mark.parametrize("n_trees", fr.OFFSET_TREES)
def test_offset_cases(n_trees):
    # k_split_scan: ceil(M / 1024) trees per thread -- 1, 1, 2, 5, 32; above 32 768 trees the multi-block scans
    per = (n_trees + fr.SPLIT_SCAN_THREADS - 1) // fr.SPLIT_SCAN_THREADS
    assert (per, n_trees > fr.SPLIT_SCAN_MAX_TREES) == {1023: (1, False), 1024: (1, False), 1025: (2, False),
                                                        5000: (5, False), 32768: (32, False), 32769: (33, True),
                                                        70000: (69, True)}[n_trees]
    assert fr.scan_blocks(32769) == 9 and fr.scan_blocks(70000) == 18
    for n_parts in (2, 3, 8):
        arrays, parts = fr.offsets_case(n_trees, n_parts)
        assert arrays.n_trees == n_trees and arrays.n_taxa == fr.TINY_UNIVERSE
        counts = arrays.leaf_counts()
        assert counts.min() == 3 and counts.max() == 6 and np.array_equal(np.diff(arrays.node_off), 2 * counts - 1)
        assert len(parts) == n_parts and sum(len(p) for p in parts) < arrays.n_taxa  # some taxa in no part
        assert len(np.unique(np.concatenate(parts))) == sum(len(p) for p in parts)
        if n_trees <= 5000:
            if n_trees == 1025:
                fr.well_formed(arrays)
            kids = arrays.split(parts)
            kept = np.asarray([c.n_trees for c in kids])
            assert np.all(kept[: n_parts - 1] > 0) and np.all(kept < n_trees * 0.97)  # many trees dropped
            if n_parts > 2:
                assert len(parts[-1]) == 1 and kept[-1] == 0  # a part that keeps no tree at all
            if n_parts == 8:
                assert np.all(kept < n_trees // 4)


@pytest.mark.parametrize("n_trees", (1025, 32769))
def test_level_cases(n_trees):
    for n_parts in (2, 3, 8):
        level, t_end, part_of, new_id, child_taxa, order, sets, bases = fr.level_case(n_trees, n_parts)
        assert level.n_trees == n_trees and t_end[-1] == n_trees and len(t_end) == fr.LEVEL_NODES
        assert np.all(np.diff(t_end) > 0) and np.diff(t_end).min() < n_trees // 50  # several nodes, one of them tiny
        # a node's trees hold the node's ids only
        tree_of = np.repeat(np.arange(n_trees), np.diff(level.node_off))
        node_of = np.searchsorted(t_end, tree_of, side="right")
        leaf = level.taxon >= 0
        assert np.array_equal(level.taxon[leaf] // fr.TINY_UNIVERSE, node_of[leaf])
        assert child_taxa == sum(len(s) for s in sets) < level.n_taxa and np.count_nonzero(part_of < 0) > 0
        assert len(order) == len(set(order)) and order == sorted(order)
        for (b, k), ids, base in zip(order, sets, bases):
            assert np.all(part_of[ids] == b) and np.all(ids // fr.TINY_UNIVERSE == k)
            assert np.array_equal(new_id[ids], base + np.arange(len(ids)))
        assert {b for b, _ in order} == set(range(n_parts))
        if n_parts > 2:
            assert (n_parts - 1, 3) not in order and len(sets[order.index((n_parts - 1, 1))]) == 1
        if n_trees == 1025:
            kids = level.split(sets)
            assert sum(c.n_trees == 0 for c in kids) >= (n_parts > 2) and sum(c.n_trees > 0 for c in kids) >= 10


@pytest.mark.parametrize("tpb", sorted(fr.STAGING))
def test_staging_cases(tpb):
    arrays = fr.staging_case(tpb)
    fr.well_formed(arrays)
    got, nodes = fr.workgroup_nodes(arrays)
    assert got == tpb and arrays.n_trees == fr.STAGING[tpb][3] and arrays.n_trees % tpb != 0
    assert nodes[1] == fr.SPLIT_CAP and nodes[2] == fr.SPLIT_CAP + 1  # the last staged size, the first in-place one
    # ... by the library's own rule and predicate, not only by their restatement in forest_reference.py
    lib_tpb, staged = debug_split_plan(arrays.node_off)
    assert lib_tpb == tpb and staged.tolist() == [True, True, False] + [True] * (len(nodes) - 3)
    assert np.all(np.delete(nodes, 2) <= fr.SPLIT_CAP) and len(nodes) == (arrays.n_trees + tpb - 1) // tpb
    start = np.repeat(arrays.node_off[:-1], np.diff(arrays.node_off))
    kids = np.bincount((start + arrays.parent)[arrays.parent >= 0], minlength=len(arrays.parent))[arrays.taxon < 0]
    how = fr.STAGING[tpb][1]  # the one node that makes 2 305: a trifurcation or a unary node, nothing else unusual
    assert np.count_nonzero(kids == 3) == (how == "tri") and np.count_nonzero(kids == 1) == (how == "unary")
    assert np.count_nonzero(kids == 2) == len(kids) - 1
    inner = arrays.taxon < 0
    assert np.any(arrays.length[inner] < 0) and np.any(np.isnan(arrays.length[inner]))


def test_mixed_staging_case():
    arrays = fr.mixed_staging_case()
    tpb, nodes = fr.workgroup_nodes(arrays)
    assert tpb == 64 and arrays.n_trees == 621 and arrays.n_trees % 64 != 0
    assert np.count_nonzero(nodes > fr.SPLIT_CAP) == 1 and np.count_nonzero(nodes <= fr.SPLIT_CAP) == len(nodes) - 1
    assert 0 < int(np.argmax(nodes)) < len(nodes) - 1  # in the middle of the launch
    lib_tpb, staged = debug_split_plan(arrays.node_off)
    assert lib_tpb == 64 and np.array_equal(staged, nodes <= fr.SPLIT_CAP)
    assert arrays.leaf_counts().max() == 150


@pytest.mark.parametrize("n_nodes", fr.NODE_TOTALS)
def test_exact_node_totals(n_nodes):
    arrays = fr.exact_nodes_case(n_nodes)
    fr.well_formed(arrays)
    assert int(arrays.node_off[-1]) == n_nodes == len(arrays.parent)
    # the scans run over N items and write N + 1 entries: the total alone in a block of its own at N = 4096 / 8192
    assert fr.scan_blocks(n_nodes) == {4095: 1, 4096: 2, 4097: 2, 8191: 2, 8192: 3}[n_nodes]
    assert n_nodes / arrays.n_trees > 32  # (the per-node family also by the launcher's own choice)


def test_combs_straddle_the_path_buffer():
    depths = [fr.max_inner_depth(fr.comb_forest(k, k, k + 10), 0) for k in fr.COMB_LEAVES]
    assert depths == [k - 2 for k in fr.COMB_LEAVES] == list(range(188, 195))
    assert [d > fr.PAR_PATH for d in depths] == [False] * 5 + [True] * 2  # 195 and 196 leaves: the fallback
    arrays = fr.comb_among_balanced_case()
    fr.well_formed(arrays)
    deep = [fr.max_inner_depth(arrays, t) for t in range(arrays.n_trees)]
    assert arrays.n_trees == 31 and deep[15] == 194 and sorted(deep)[-2] < 40


@pytest.mark.parametrize("name", sorted(fr.ANALYSIS))
def test_analysis_cases(name):
    arrays = fr.analysis_case(name)
    u, m, _, blocks = fr.ANALYSIS[name]
    assert arrays.n_taxa == u and arrays.n_trees == m and arrays.leaf_counts().min() >= 2
    tables = arrays.flatten("depth")
    leaves = tables.n_leaves
    want = {"lds_2047_partial": (False, 3, 0), "lds_2048_full": (False, 3, 0), "tiled_2049_full": (True, 1, 0),
            "tiled_16383_three_full": (True, 1, 0), "tiled_16384_partial20": (True, 1, 1),
            "tiled_16385_full70": (True, 2, 2), "tiled_20000_blocks": (True, 2, 0), "leaves_65536": (True, 1, 0),
            "leaves_65537": (True, 1, 1)}[name]
    tiled = u > fr.ANALYZE_LDS_TAXA
    groups = (u + fr.SIG_TILE - 1) // fr.SIG_TILE if tiled else (leaves + fr.ANALYZE_LEAVES_PER_BLOCK - 1) // fr.ANALYZE_LEAVES_PER_BLOCK
    passes = int(leaves > fr.SAMPLE_MIN_LEAVES) + int(leaves > 16 * fr.SAMPLE_MIN_LEAVES)
    assert (tiled, groups, passes) == want
    if name.startswith("leaves_"):
        assert leaves == int(name.split("_")[1])
    if name == "tiled_20000_blocks":
        assert u % fr.SIG_TILE == 3616
    root, side_sets = fr.analysis_reference(tables)
    assert fr.pair_kinds(side_sets) == (True, True)
    occ = fl.taxa_occurrences(tables)
    assert occ[0] > 0 and occ[-1] > 0 and 5 <= np.count_nonzero(occ == 0)  # ids no tree holds; the edges are held
    assert len(np.unique(root[occ > 0])) >= blocks
    classes = len({s for s in side_sets if s})
    if name == "tiled_16383_three_full":
        assert classes <= 8 + 2  # three full trees: 2^3 classes, and the rare taxa's two
    if name in ("tiled_16384_partial20", "tiled_16385_full70"):
        assert classes > 0.6 * np.count_nonzero(occ > 0)  # nearly all sets distinct
    if name == "tiled_20000_blocks":
        assert len(np.unique(root[occ > 0])) >= 3


@pytest.mark.parametrize("child_taxa", sorted(fr.ANALYSIS_LEVEL))
def test_analysis_level_cases(child_taxa):
    arrays, part_of, new_id, parts = fr.analysis_level_case(child_taxa)
    assert sum(len(p) for p in parts) == child_taxa == np.count_nonzero(part_of >= 0) < arrays.n_taxa
    assert part_of[0] >= 0 and part_of[-1] >= 0
    kids = arrays.split(parts)
    for c in kids:
        assert c.n_trees == arrays.n_trees
    tables = fr.union_tables(kids, [0, len(parts[0])], "depth", child_taxa)
    capacity = int(arrays.leaf_counts().sum())
    assert tables.n_leaves < 0.85 * capacity  # the device's leaf count is well below what its launches are sized by
    assert capacity > fr.SAMPLE_MIN_LEAVES or child_taxa < 16384
    root, side_sets = fr.analysis_reference(tables)
    assert fr.pair_kinds(side_sets) == (True, True)
    assert len(side_sets[0]) > 0 and len(side_sets[-1]) > 0


def test_the_librarys_split_plan_is_the_restated_one():
    forests = [fr.offsets_case(1025, 3)[0], fr.exact_nodes_case(8192), fr.comb_among_balanced_case(),
               fr.build_forest(3, 300, [100] * 9), fr.build_forest(4, 300, [31] * 70 + [2])]
    for arrays in forests:
        tpb, nodes = fr.workgroup_nodes(arrays)
        lib_tpb, staged = debug_split_plan(arrays.node_off)
        assert lib_tpb == tpb and np.array_equal(staged, nodes <= fr.SPLIT_CAP)
    assert {fr.workgroup_nodes(a)[0] for a in forests} == {64, 32, 16, 8}
