"""The forest split, its scans and the level analysis (``csrc/scs_forest.hip``) at the edges of their constants,
against exact host references -- everything here is integer or bit-for-bit work, so every comparison is
``np.array_equal`` (doubles through their bits).  DESIGN.md section 27 lists the edges and the test that pins each.

* the multi-block exclusive scan (``scs_debug_scan``: the product's own ``scan_exclusive``) against
  ``forest_reference.scan_reference``;
* ``scs_forest_split`` and ``scs_forest_split_level`` against the host sweep (``TreeArrays.split`` + ``flatten``, which
  ``tests/test_treearrays.py`` holds against the tree-object path; reference: src/sc_supertree/scs.py:139-171,
  :411-455) over many tiny trees, at the staging capacity of the thread-per-tree kernels, at the block edges and the
  path buffer of the per-node kernels;
* the analysis (components, contraction signatures; reference: scs.py:122, :302-316) against
  ``forest_reference.analysis_reference`` on every route.

The forests come from ``tests/forest_reference.py``; ``tests/test_forest_reference_cpu.py`` asserts that each of them has
the tree count, node totals, path lengths, universe and leaf count its case is named for.
"""

from __future__ import annotations

import numpy as np
import pytest

from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.treearrays import _STRATEGY_CODE, ResidentArrays
from tests import forest_reference as fr
from tests.test_gpu_forest import compare_split
from tests.test_treearrays import tables_equal

pytestmark = pytest.mark.gpu

FAMILIES = {"thread per tree": "1000000000", "per node": "0"}


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(autouse=True)
def device_split_of_any_size(monkeypatch):
    monkeypatch.setenv("SCS_DEVICE_SPLIT_MIN_NODES", "0")


def _force(monkeypatch, family: str) -> None:
    monkeypatch.setenv("SCS_FOREST_PARALLEL_MIN_TREE_NODES", FAMILIES[family])


@pytest.fixture(params=list(FAMILIES))
def family(request, monkeypatch):
    """Both families of kernels, forced as ``tests/test_gpu_forest.py`` forces them."""
    _force(monkeypatch, request.param)
    return request.param


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------------- scans
def scan_rows(op: int, n_parts: int, n: int, seed: int) -> np.ndarray:
    """The callers' inputs: for the sum 0/1 flags, for the maximum mostly -1 with the index itself at random places
    (increasing values); in both, runs of two whole blocks with nothing in them.  Every part draws its own row."""
    rng = np.random.RandomState(seed)
    rows = np.full((n_parts, n), 0 if op == 0 else -1, dtype=np.int32)
    for part in range(n_parts):
        if n == 0:
            break
        pos = rng.randint(0, n, size=max(1, n // 3 if n < 100000 else n // 40))
        rows[part, pos] = 1 if op == 0 else pos
        blocks = n // fr.SCAN_BLOCK
        for b in rng.randint(0, max(blocks - 1, 1), size=min(blocks // 2, 40)):
            rows[part, b * fr.SCAN_BLOCK:(b + 2) * fr.SCAN_BLOCK] = 0 if op == 0 else -1
    return rows


def check_scan(dev, op: int, n_parts: int, n: int) -> None:
    rows = scan_rows(op, n_parts, n, 1000 * n_parts + op + n % 997)
    if n_parts > 1 and n > 8:
        assert not np.array_equal(rows[0], rows[1])  # a wrong row stride would show
    got = dev.debug_scan(op, rows)
    want = fr.scan_reference(op, rows)
    assert got.shape == (n_parts, n + 1) and got.dtype == np.int32
    if not np.array_equal(got, want):
        part, at = np.argwhere(got != want)[0]
        msg = f"op {op}, {n_parts} part(s), n {n}: first difference in part {part} at {at} (block {at // fr.SCAN_BLOCK}): {got[part, at]} != {want[part, at]}"
        raise AssertionError(msg)
    if n > 1:
        assert want[:, -1].max() > 0  # (the totals are not trivial)


@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
@pytest.mark.parametrize("n_parts", [1, 8])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 4094, 4095, 4096, 4097, 8191])
def test_scan_at_the_thread_and_block_edges(dev, n, n_parts, op):
    """16 items per thread, 4 096 per workgroup, and entry n -- the total -- alone in a second block at n = 4 096."""
    check_scan(dev, op, n_parts, n)


@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
@pytest.mark.parametrize("blocks, n_parts", [(2, 8), (8192, 1), (8193, 1), (8193, 2), (9216, 1), (9216, 2), (9217, 1), (9217, 2)])
def test_scan_at_the_switch_to_scanned_block_sums(dev, blocks, n_parts, op):
    """Up to 8 192 workgroups every workgroup reduces the raw sums in front of it (``k_scan_add_raw``); above,
    ``k_scan_blocks`` scans them in rounds of 1 024 with a carry -- a partial round (8 193 = 8 x 1 024 + 1), a whole
    number of rounds (9 216) and one block past it (9 217).  ``n = (blocks - 1) x 4 096``: the total is alone in the
    last block."""
    n = (blocks - 1) * fr.SCAN_BLOCK
    assert fr.scan_blocks(n) == blocks and fr.scan_blocks(n - 1) == blocks - 1
    assert fr.SCAN_RAW_MAX_BLOCKS == 8192 and 9216 % fr.SCAN_BLOCKS_ROUND == 0 and 8193 % fr.SCAN_BLOCKS_ROUND == 1
    check_scan(dev, op, n_parts, n)


# ---------------------------------------------------------------------------------- offsets over many trees
@pytest.mark.parametrize("n_parts", [2, 3, 8])
@pytest.mark.parametrize("n_trees", fr.OFFSET_TREES)
def test_split_offsets_over_many_trees(dev, family, n_trees, n_parts):
    """``k_split_scan`` with 1, 2, 5 and 32 trees per thread; above 32 768 trees the multi-block scans and
    ``k_split_finalize``.  Tiny trees: most parts drop most trees, the last of three or eight keeps none."""
    arrays, parts = fr.offsets_case(n_trees, n_parts)
    compare_split(dev, arrays, parts, "branch", levels=1)


def compare_level_split(dev, case, n_parts: int, strategy: str):
    """``scs_forest_split_level`` on a case of ``forest_reference.level_case`` against the host: trees and leaves per
    child, the union's node arrays and tables child by child (``download`` / ``tables_range``), the present taxa, the
    monotone flag, and the analysis of the union."""
    level, t_end, part_of, new_id, child_taxa, order, sets, bases = case
    forest = ResidentArrays.from_host(level, dev).forest
    union, child_trees, child_leaves, present, comp_root, sig = forest.split_level(
        part_of, new_id, n_parts, child_taxa, _STRATEGY_CODE[strategy], t_end)
    want = level.split(sets)  # the host's child of every (part, node): other nodes' trees hold none of its ids
    where = {bk: c for c, bk in enumerate(order)}
    want_present = np.zeros(child_taxa, dtype=np.uint8)
    monotone = True
    kept, kept_bases = [], []
    t_at = 0
    for b in range(n_parts):
        for k in range(len(t_end)):
            m = int(child_trees[b, k])
            if (b, k) not in where:  # a node with fewer parts
                assert m == 0 and child_leaves[b, k] == 0
                continue
            w, base = want[where[(b, k)]], bases[where[(b, k)]]
            assert m == w.n_trees and int(child_leaves[b, k]) == int(w.leaf_counts().sum())
            if m == 0:
                continue
            node_off, parent, taxon, length, support, weights = union.download(t_at, t_at + m)
            assert np.array_equal(node_off, w.node_off) and np.array_equal(parent, w.parent)
            assert np.array_equal(np.where(taxon >= 0, taxon - base, -1), w.taxon)
            assert np.array_equal(_bits(length), _bits(w.length)) and np.array_equal(_bits(support), _bits(w.support))
            assert np.array_equal(_bits(weights), _bits(w.weights))
            tree_off, leaf_taxon, adj_depth, adj_val, tree_w = union.tables_range(t_at, t_at + m)
            tab = w.flatten(strategy)
            got = fl.TreeTables(n_taxa=w.n_taxa, tree_off=tree_off, leaf_taxon=(leaf_taxon - base).astype(np.int32),
                                adj_depth=adj_depth, adj_val=adj_val, tree_w=tree_w, monotone=tab.monotone)
            tables_equal(got, tab)
            monotone = monotone and tab.monotone
            want_present[base + w.present_taxa()] = 1
            kept.append(w)
            kept_bases.append(base)
            t_at += m
    assert t_at == union.n_trees
    assert np.array_equal(present, want_present)
    if strategy != "bootstrap":
        assert bool(union.monotone_flag) == monotone
    root, side_sets = fr.analysis_reference(fr.union_tables(kept, kept_bases, strategy, child_taxa))
    assert np.array_equal(comp_root, root)
    fr.check_signatures(sig, side_sets)
    return union


@pytest.mark.parametrize("n_parts", [2, 3, 8])
@pytest.mark.parametrize("n_trees", fr.OFFSET_TREES)
def test_level_split_offsets_over_many_trees(dev, family, n_trees, n_parts):
    """The same tree counts through ``scs_forest_split_level``: five nodes (one of them a hundredth of the level), odd
    nodes with two parts only, taxa in no part, a single-taxon part."""
    union = compare_level_split(dev, fr.level_case(n_trees, n_parts), n_parts, "branch")
    assert union.n_trees > n_trees // 10


# ---------------------------------------------------------------------------------- thread-per-tree staging
@pytest.mark.parametrize("strategy", ["branch", "depth", "one"])
@pytest.mark.parametrize("tpb", sorted(fr.STAGING))
def test_workgroups_at_the_staging_capacity(dev, monkeypatch, tpb, strategy):
    """One workgroup of exactly 2 304 nodes (the last that is copied to LDS) and the next of exactly 2 305 (walked in
    place), at every number of trees per workgroup the launcher chooses; negative and missing lengths."""
    _force(monkeypatch, "thread per tree")
    arrays = fr.staging_case(tpb)
    for n_parts in (2, 3):
        compare_split(dev, arrays, fr.parts_of(tpb + n_parts, np.arange(arrays.n_taxa), n_parts), strategy, levels=1)


@pytest.mark.parametrize("strategy", ["branch", "depth", "one", "bootstrap"])
def test_staged_and_in_place_workgroups_in_one_launch(dev, monkeypatch, strategy):
    _force(monkeypatch, "thread per tree")
    arrays = fr.mixed_staging_case()
    for n_parts in (2, 8):
        compare_split(dev, arrays, fr.parts_of(9 + n_parts, np.arange(arrays.n_taxa), n_parts), strategy, levels=1)
    if strategy == "bootstrap":
        compare_split(dev, fr.staging_case(64), fr.parts_of(1, np.arange(400), 2), strategy, levels=1)


# -------------------------------------------------------------------------------------- the per-node family
@pytest.mark.parametrize("n_parts", [2, 8])
@pytest.mark.parametrize("n_nodes", fr.NODE_TOTALS)
def test_per_node_split_at_the_scan_block_edges(dev, monkeypatch, n_nodes, n_parts):
    """Forests of exactly N nodes: the scans over the nodes write N + 1 entries -- 4 096 fills one block, 4 097 puts
    the total alone in a second one."""
    _force(monkeypatch, "per node")
    arrays = fr.exact_nodes_case(n_nodes)
    for strategy in ("branch", "depth"):
        compare_split(dev, arrays, fr.parts_of(n_nodes + n_parts, np.arange(arrays.n_taxa), n_parts), strategy, levels=1)


@pytest.mark.parametrize("n_leaves", fr.COMB_LEAVES)
def test_combs_around_the_path_buffer(dev, family, n_leaves):
    """Root paths of 188 ... 194 inner nodes around ``PAR_PATH`` = 192: the per-node family answers up to 192 and hands
    the call to the other family above -- whichever answers, the children are the host's.  Kept whole by one part
    (the other holds ids of no tree), and split between two."""
    arrays = fr.comb_forest(n_leaves, n_leaves, n_leaves + 10)
    held = arrays.present_taxa()
    other = np.setdiff1d(np.arange(arrays.n_taxa, dtype=np.int32), held)
    assert len(held) == n_leaves and len(other) == 10
    for strategy in ("branch", "depth"):
        compare_split(dev, arrays, [held, other], strategy, levels=1)
        compare_split(dev, arrays, [held[::2], held[1::2]], strategy, levels=1)
        compare_split(dev, arrays, [held[: n_leaves // 3], held[n_leaves // 3:]], strategy, levels=1)


def test_one_comb_among_balanced_trees(dev, family):
    """The fallback takes the whole call: thirty balanced trees are restricted by the thread-per-tree kernels too."""
    arrays = fr.comb_among_balanced_case()
    comb = np.sort(arrays.taxon[arrays.node_off[15]:arrays.node_off[16]])
    comb = comb[comb >= 0].astype(np.int32)
    rest = np.setdiff1d(np.arange(arrays.n_taxa, dtype=np.int32), comb)
    for strategy in ("branch", "one"):
        compare_split(dev, arrays, [comb, rest], strategy, levels=1)
        compare_split(dev, arrays, fr.parts_of(3, np.arange(arrays.n_taxa), 3), strategy, levels=1)


# ------------------------------------------------------------------------------------------------ analysis
MODES = {"default": None, "global signatures": "SCS_ANALYZE_GLOBAL_SIG", "no sampled pass": "SCS_ANALYZE_SAMPLE"}


def _in_every_mode(monkeypatch, run):
    """``run()`` under the default, with the signatures added by global atomics, and without the sampled union-find
    passes: ``{mode: (comp_root, sig)}``."""
    out = {}
    for mode, var in MODES.items():
        if var:
            monkeypatch.setenv(var, "1")
        out[mode] = run()
        if var:
            monkeypatch.delenv(var)
    return out


def check_analysis(got: dict, root: np.ndarray, side_sets) -> None:
    comp_root, sig = got["default"]
    assert np.array_equal(comp_root, root)
    fr.check_signatures(sig, side_sets)
    for mode in got:  # sums mod 2^64 and unions do not depend on the order: bit-identical on every route
        assert np.array_equal(got[mode][0], comp_root), mode
        assert np.array_equal(got[mode][1], sig), mode


@pytest.mark.parametrize("name", sorted(fr.ANALYSIS))
def test_analysis_of_an_identity_child(dev, monkeypatch, name):
    """``scs_forest_analyze`` on the child of a split that keeps everything: its tables are the forest's own, the
    leaf count is exact.  The LDS route with three workgroups, one and two tiles of signatures (a last tile of one
    taxon, a short one), leaf counts on both sides of each sampled pass's threshold; few classes of side sets and
    nearly as many as taxa; several components; ids no tree holds."""
    arrays = fr.analysis_case(name)
    tables = arrays.flatten("depth")
    root, side_sets = fr.analysis_reference(tables)
    n = arrays.n_taxa
    kid = ResidentArrays.from_host(arrays, dev).forest.split(
        np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), [n], _STRATEGY_CODE["depth"])[0]
    tree_off, leaf_taxon, adj_depth = kid.tables()[:3]
    assert np.array_equal(tree_off, tables.tree_off) and np.array_equal(leaf_taxon, tables.leaf_taxon)
    assert np.array_equal(adj_depth, tables.adj_depth)
    check_analysis(_in_every_mode(monkeypatch, kid.analyze), root, side_sets)


@pytest.mark.parametrize("child_taxa", sorted(fr.ANALYSIS_LEVEL))
def test_analysis_through_a_level_split_that_drops_taxa(dev, monkeypatch, child_taxa):
    """``scs_forest_split_level`` of one node into two parts with a fifth of the taxa in neither: the launches of the
    analysis are sized by the parent's leaf count, the leaves that exist are a device-side number well below it."""
    arrays, part_of, new_id, parts = fr.analysis_level_case(child_taxa)
    kids = arrays.split(parts)
    tables = fr.union_tables(kids, [0, len(parts[0])], "depth", child_taxa)
    root, side_sets = fr.analysis_reference(tables)
    forest = ResidentArrays.from_host(arrays, dev).forest
    t_end = np.asarray([arrays.n_trees], dtype=np.int32)

    def run():
        union, child_trees, child_leaves, present, comp_root, sig = forest.split_level(
            part_of, new_id, 2, child_taxa, _STRATEGY_CODE["depth"], t_end)
        assert child_trees.ravel().tolist() == [k.n_trees for k in kids]
        assert int(child_leaves.sum()) == tables.n_leaves
        tree_off, leaf_taxon, adj_depth, _, _ = union.tables_range(0, union.n_trees)
        assert np.array_equal(tree_off, tables.tree_off) and np.array_equal(leaf_taxon, tables.leaf_taxon)
        assert np.array_equal(adj_depth, tables.adj_depth)
        assert np.array_equal(present.astype(bool), np.asarray([len(s) > 0 for s in side_sets]))
        return comp_root, sig

    check_analysis(_in_every_mode(monkeypatch, run), root, side_sets)
