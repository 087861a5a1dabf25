"""The pairwise source-tree distances without a device: the two references of ``tests/source_pairs_reference.py`` held
to one another and to ``tests/score_reference.py``, the plan entry against its restatement, the bindings against the
header, and the host layer -- what ``Device.score_source_pairs`` hands to the export, how ``source_distances`` brings
the answers back to the trees as given, the derived values and the table on hand-made counts."""

import ctypes as C
import math
import random
import re
import types
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest
import score_reference as sr
import source_pairs_reference as sp

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, source_distances
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import SourceDistances
from spectralclustersupertree_amd.tree import TreeNode, make_tree

ROOT = Path(__file__).resolve().parent.parent


def random_tree(rng: random.Random, n_taxa: int, lo: int = 1):
    """A nested-list tree on a random subset of the taxa: polytomies, now and then a chain of unary nodes above the
    root or a clade, a caterpillar or a star."""
    tree = pr.rand_tree(rng.sample(range(n_taxa), rng.randint(min(lo, n_taxa), n_taxa)), rng.choice([2, 3, 6]), rng)
    kind = rng.random()
    if kind < 0.15:
        tree = pr.caterpillar(pr.leaves_of(tree), rng.random() < 0.5)
    elif kind < 0.2:
        tree = pr.leaves_of(tree)
    if isinstance(tree, list) and rng.random() < 0.3:
        if isinstance(tree[0], list):
            tree[0] = [[tree[0]]]
        tree = [[tree]]
    if isinstance(tree, list) and len(tree) == 1 and not isinstance(tree[0], list):
        tree = tree[0]  # (a tree of one leaf is the leaf)
    return tree


# ------------------------------------------------------------------------------------------------ the references
def test_the_two_references_agree_on_random_pairs():
    rng = random.Random(33)
    pairs = overlap = empty = 0
    for _ in range(150):
        n = rng.randint(1, 40)
        trees = [random_tree(rng, n) for _ in range(3)]
        tabs = pr.tables(trees, n)
        a, b = sp.by_sets(trees), sp.linear(tabs)
        for k in sp.KEYS:
            assert a[k].dtype == np.int32 and np.array_equal(a[k], b[k]), (trees, k, a[k], b[k])
        sp.check_invariants(a)
        pairs += 9
        overlap += int((a["shared"] < np.minimum(a["clusters"], a["clusters_other"])).sum())
        empty += int((a["common"] == 0).sum())
    assert pairs > 1000 and overlap > 100 and empty > 0
    rows = [2, 0, 2]
    assert np.array_equal(sp.linear(tabs, rows)["clusters"], b["clusters"][rows])


def test_the_definitions_on_hand_made_pairs():
    # ((a,b),(c,d)) against ((a,c),(b,d)): nothing shared; against itself: both clusters
    assert sp.pair_by_sets([[0, 1], [2, 3]], [[0, 2], [1, 3]]) == (4, 2, 2, 0)
    assert sp.pair_by_sets([[0, 1], [2, 3]], [[0, 1], [2, 3]]) == (4, 2, 2, 2)
    # a chain of nodes collapses onto one set: (((a,x),y),b,c) restricted to {a,b,c} has no cluster
    assert sp.pair_by_sets([[[0, 7], 8], 1, 2], [[0, 1], 2]) == (3, 0, 1, 0)
    # ... and ((((a,x),b),y),c) carries {a,b} on two nodes, once
    assert sp.pair_by_sets([[[[0, 7], 1], 8], 2], [[0, 1], 2]) == (3, 1, 1, 1)
    # fewer than three common taxa: zeros beside the count; trees of one and two leaves are legal
    assert sp.pair_by_sets([[0, 1], 2], [[0, 1], 5]) == (2, 0, 0, 0)
    assert sp.pair_by_sets(4, [[4, 1], 5]) == (1, 0, 0, 0) and sp.pair_by_sets([0, 1], [2, 3]) == (0, 0, 0, 0)


def _treenode(tree, names) -> TreeNode:
    return TreeNode(None, [_treenode(c, names) for c in tree]) if isinstance(tree, list) else TreeNode(names[tree])


def test_a_tree_over_all_taxa_scores_like_a_supertree():
    rng = random.Random(12)
    for _ in range(20):
        n = rng.randint(3, 30)
        names = [f"t{i}" for i in range(n)]
        sup = pr.rand_tree(range(n), rng.choice([2, 3, 5]), rng)
        trees = [random_tree(rng, n) for _ in range(5)]
        want = sr.brute_force(_treenode(sup, names), [_treenode(t, names) for t in trees])
        got = sp.linear(pr.tables([*trees, sup], n), rows=[5])
        sizes = np.array([len(pr.leaves_of(t)) for t in trees])
        assert np.array_equal(got["common"][0, :5], sizes)
        assert np.array_equal(got["clusters"][0, :5], want["n_super"])
        assert np.array_equal(got["clusters_other"][0, :5], want["n_source"])
        assert np.array_equal(got["shared"][0, :5], want["shared"])


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("sizes", [[1, 2, 3, 4, 66, 67, 130, 4099, 9000], [10] * 40, [70000, 70000, 5],
                                   [65535, 65536, 3], [1]])
def test_the_plan_entry_equals_its_restatement(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for n_taxa in (1, 500, 80000):
        for batch_trees, lds_bytes, n_rows in ((0, 0, None), (1, 0, 3), (2, 4096, 0), (3, 1 << 20, None), (0, 600, 1), (0, 8, None)):
            got = backend.debug_source_pairs_plan(off, n_taxa, n_rows, batch_trees, lds_bytes)
            want = sp.plan(off, n_taxa, len(sizes) if n_rows is None else n_rows, batch_trees, lds_bytes)
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (sizes, n_taxa, batch_trees, lds_bytes, k, got[k], want[k])
    one = backend.debug_source_pairs_plan(off, 500, None, 1)  # one tree a batch: a tile is a pair
    assert len(one["bstart"]) == len(sizes) + 1
    for i, a in enumerate(sizes):
        for j, b in enumerate(sizes):
            width = 2 if max(a, b) < 65536 else 4
            assert one["width"][i, j] == width and one["need"][i, j] == sp.pair_bytes(a, b, width) + sp.SP_SCRATCH
            assert one["slab"][i, j] == (one["need"][i, j] > sp.TP_LDS_MAX)
    if max(sizes) == 9000:
        # two pair workgroups of the largest trees fit a CU's 160 KiB
        assert 2 * one["need"].max() <= sp.TP_LDS_MAX and one["slab_stride"] == 0 and one["slab_wgs"] == 0
        assert one["threads"][8, 8] == 1024 and one["threads"][0, 0] == 256 and one["threads"][7, 7] == 512
    if max(sizes) == 70000:
        assert one["slab"][0, 1] == 1 and one["slab"][2, 2] == 0 and one["width"][0, 2] == 4
        assert one["slab_stride"] >= one["need"][0, 0] - sp.SP_SCRATCH and 1 <= one["slab_wgs"] <= 256


def test_a_launch_stays_under_the_work_items_a_dispatch_can_count(monkeypatch):
    # 5 000 trees of 500 leaves fit one batch: 25 million cells, more than one launch of 256-thread workgroups holds
    off = np.arange(5001, dtype=np.int64) * 500
    plan = backend.debug_source_pairs_plan(off, 20000)
    want = sp.plan(off, 20000, 5000)
    assert plan["bstart"].tolist() == [0, 5000] and plan["threads"].tolist() == [[256]]
    assert plan["grid_limit"].tolist() == [[(2**32 - 1) // 256]] == want["grid_limit"].tolist()
    assert plan["rows_per_launch"].tolist() == [[16777215 // 5000]] == want["rows_per_launch"].tolist()
    for threads in (256, 512, 1024):
        monkeypatch.setenv("SCS_SP_THREADS", str(threads))
        for sizes, batch in (([500] * 5000, 0), ([3] * 2100, 0), ([9000] * 5, 2), ([10] * 70000, 0)):
            tree_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            plan = backend.debug_source_pairs_plan(tree_off, 20000, batch_trees=batch)
            assert (plan["threads"] == threads).all()
            nb = np.diff(plan["bstart"])
            grid = np.minimum(plan["rows_per_launch"] * nb[None, :], plan["grid_limit"])
            assert (grid * plan["threads"] <= 2**32 - 1).all() and (grid <= 2**30).all() and (grid >= 1).all()
            assert (plan["rows_per_launch"] >= 1).all()
    # 2 100 trees at 1 024 threads: 4.4 million cells, more than the 4 194 303 workgroups of one launch
    assert plan["rows_per_launch"].max() < 70000 and 2100 * 2100 > (2**32 - 1) // 1024


def test_the_plan_entry_refuses_what_it_cannot_plan():
    off = np.array([0, 5, 3], dtype=np.int64)
    with pytest.raises(nv.ScsError, match="scs_debug_source_pairs_plan: tree_off decreases at tree 1"):
        backend.debug_source_pairs_plan(off, 10)
    with pytest.raises(nv.ScsError, match="scs_debug_source_pairs_plan: negative argument"):
        backend.debug_source_pairs_plan(np.array([0, 5], dtype=np.int64), 10, lds_bytes=-1)
    lib = nv.load_library()
    assert lib.scs_debug_source_pairs_plan(None, 1, None, 1, 1, 0, 0, None, None, None, None) == nv.EINVAL
    assert lib.scs_last_error() == b"scs_debug_source_pairs_plan: null argument"


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("symbol,count", [("scs_score_source_pairs", 10), ("scs_debug_source_pairs_plan", 11)])
def test_the_exports_are_declared_bound_and_exported(symbol, count):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(rf"int {symbol}\(([^)]*)\)", text)
    assert m, f"include/scs_hip.h does not declare {symbol}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES[symbol]
    assert restype is C.c_int and len(argtypes) == len(params) == count
    for p, a in zip(params, argtypes):
        assert (a is nv._I32) == (p.startswith("int32_t ") and "*" not in p), (symbol, p)
    lib = nv.load_library()
    assert hasattr(lib, symbol) and lib.scs_version() == nv.ABI_VERSION == 109
    if symbol == "scs_score_source_pairs":
        assert params == ["scs_ctx *ctx", "const scs_tables *sources", "int32_t n_rows", "const int32_t *rows",
                          "int32_t max_batch_trees", "int32_t max_lds_bytes", "int32_t *common", "int32_t *clusters",
                          "int32_t *clusters_other", "int32_t *shared"]
        assert lib.scs_score_source_pairs(None, None, 0, None, 0, 0, None, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_source_pairs: null argument"


# ------------------------------------------------------------------------------------------------ the host layer
def _at(address: int, dtype, count: int) -> np.ndarray:
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


class FakeLib:
    """``scs_score_source_pairs`` records its arguments and answers cell [i][j] = 100 x + 10 tree + j for output x."""

    def __init__(self, m):
        self.m, self.calls, self.rc = m, [], 0

    def scs_last_error(self):
        return b"scs_score_source_pairs: rows[0] = 9 is not a tree of the tables (3 trees)"

    def scs_score_source_pairs(self, ctx, tabs, n_rows, rows, batch, lds, *outs):
        ids = list(range(self.m)) if rows is None else _at(rows, np.int32, n_rows).tolist()
        self.calls.append((n_rows, None if rows is None else ids, batch, lds, [o is not None for o in outs]))
        for x, o in enumerate(outs):
            if o is not None:
                _at(o, np.int32, n_rows * self.m)[:] = [100 * x + 10 * t + j for t in ids for j in range(self.m)]
        return self.rc


def test_device_method_marshals_the_export():
    lib = FakeLib(3)
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3)
    got = dev.score_source_pairs(tabs)
    assert lib.calls == [(3, None, 0, 0, [True] * 4)] and list(got) == list(sp.KEYS)
    assert got["common"].dtype == np.int32 and got["common"].tolist() == [[0, 1, 2], [10, 11, 12], [20, 21, 22]]
    assert got["shared"][2].tolist() == [320, 321, 322]
    got = dev.score_source_pairs(tabs, rows=[2, 0, 2], batch_trees=5, lds_bytes=4096, outputs=("clusters",))
    assert lib.calls[-1] == (3, [2, 0, 2], 5, 4096, [False, True, False, False])
    assert got["common"] is None and got["clusters"][:, 0].tolist() == [120, 100, 120]
    assert dev.score_source_pairs(tabs, rows=[])["common"].shape == (0, 3)
    with pytest.raises(ValueError, match="rows must be a list of tree ids"):
        dev.score_source_pairs(tabs, rows=[[0, 1]])
    lib.rc = nv.EINVAL
    with pytest.raises(ValueError, match=r"rows\[0\] = 9 is not a tree of the tables"):
        dev.score_source_pairs(tabs, rows=[9])


class FakeTables:
    def __init__(self, n_trees):
        self.n_trees, self.freed = n_trees, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload`` and ``score_source_pairs``: cell [i][j] = 100 x + 10 tree + j, logged."""

    def __init__(self):
        self.log, self.tabs = [], None

    def upload(self, tables):
        self.names = None
        self.tabs = FakeTables(tables.n_trees)
        self.tables = tables
        return self.tabs

    def score_source_pairs(self, tabs, rows=None, batch_trees=0, lds_bytes=0):
        m = tabs.n_trees
        self.log.append(None if rows is None else np.asarray(rows).tolist())
        ids = list(range(m)) if rows is None else [int(r) for r in rows]
        return {k: np.array([[100 * x + 10 * t + j for j in range(m)] for t in ids], dtype=np.int32).reshape(len(ids), m)
                for x, k in enumerate(sp.KEYS)}


def test_source_distances_numbers_the_union_of_the_names_and_frees_the_tables():
    dev = FakeDevice()
    trees = [make_tree("((a,b),c);"), make_tree("(d,(b,e));"), make_tree("(a,e);")]
    res = source_distances(trees, device=dev)
    assert dev.log == [None] and dev.tabs.freed == 1 and dev.tables.n_taxa == 5
    assert dev.tables.leaf_taxon.tolist() == [0, 1, 2, 3, 1, 4, 0, 4]  # ids by first appearance: a b c d e
    assert isinstance(res, SourceDistances) and res.rows.tolist() == [0, 1, 2] and res.n_leaves.tolist() == [3, 3, 2]
    assert res.common.tolist() == [[0, 1, 2], [10, 11, 12], [20, 21, 22]] and res.shared[1, 2] == 312
    assert set(res.timings) == {"prepare", "tables", "pairs"}
    res = source_distances(trees, rows=[2, 0], device=dev)
    assert dev.log[-1] == [2, 0] and res.rows.tolist() == [2, 0] and res.clusters.tolist() == [[120, 121, 122], [100, 101, 102]]
    for rows in ([3], [-1], [[0]]):
        with pytest.raises(ValueError, match="rows must be indices of the 3 source trees"):
            source_distances(trees, rows=rows, device=dev)
    with pytest.raises(ValueError, match="at least one tree"):
        source_distances([], device=dev)


def test_the_counts_go_back_to_the_trees_as_given_on_both_axes(monkeypatch):
    # tables that hold the given trees 3, 0 and 4 (in that order) of five: trees 1 and 2 have no tables
    dev = FakeDevice()
    seen = {}

    class Resident:
        def __init__(self, device, trees, tips, index):
            seen["tips"], seen["index"] = tips, index

        def __enter__(self):
            return types.SimpleNamespace(dev=dev, tabs=FakeTables(3), n_leaves=np.array([5, 1, 1, 5, 3]), seconds=0.0,
                                         tree_index=lambda: np.array([3, 0, 4], dtype=np.int64))

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    monkeypatch.setattr(score_mod, "_source_names", lambda trees: ["x", "y"])
    res = source_distances(object(), device=dev)
    assert seen == {"tips": ["x", "y"], "index": {"x": 0, "y": 1}}
    assert dev.log == [[1, 0, 2]]  # the rows of the given trees 0, 3, 4 in the tables' numbering
    assert res.common.shape == (5, 5) and not res.common[[1, 2]].any() and not res.common[:, [1, 2]].any()
    # given tree 3 is tree 0 of the tables, given 0 is 1, given 4 is 2
    assert res.common[3, [3, 0, 4]].tolist() == [0, 1, 2] and res.common[0, [3, 0, 4]].tolist() == [10, 11, 12]
    assert res.shared[4, [3, 0, 4]].tolist() == [320, 321, 322]
    res = source_distances(object(), rows=[4, 1, 3], device=dev)
    assert dev.log[-1] == [2, 0] and res.rows.tolist() == [4, 1, 3]
    assert res.common[:, [3, 0, 4]].tolist() == [[20, 21, 22], [0, 0, 0], [0, 1, 2]]
    res = source_distances(object(), rows=[3, 0, 4], device=dev)
    assert dev.log[-1] is None  # every tree of the tables in their order: the call that mirrors


def test_without_tables_every_count_is_zero(monkeypatch):
    class Resident:
        def __init__(self, *a):
            pass

        def __enter__(self):
            return types.SimpleNamespace(dev=None, tabs=None, n_leaves=np.array([1, 1]), seconds=0.0,
                                         tree_index=lambda: None)

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    monkeypatch.setattr(score_mod, "_source_names", lambda trees: ["x"])
    res = source_distances(object())
    assert res.common.shape == (2, 2) and not res.common.any() and res.rf.tolist() == [[0, 0], [0, 0]]
    assert res.table() == "tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf\n"
    assert res.outlier_sources() == [] and np.isnan(res.mean_distance()[0]).all()


def _hand_made(rows=None) -> SourceDistances:
    common = np.array([[6, 5, 3, 2], [5, 7, 4, 0], [3, 4, 4, 4], [2, 0, 4, 9]], dtype=np.int32)
    clusters = np.array([[4, 3, 1, 0], [2, 5, 0, 0], [1, 2, 2, 2], [0, 0, 1, 6]], dtype=np.int32)
    shared = np.array([[4, 1, 1, 0], [1, 5, 0, 0], [1, 0, 2, 1], [0, 0, 1, 6]], dtype=np.int32)
    rows = np.arange(4) if rows is None else np.asarray(rows)
    return SourceDistances(common=common[rows], clusters=clusters[rows], clusters_other=clusters.T[rows],
                           shared=shared[rows], rows=rows, n_leaves=np.array([6, 7, 4, 9]))


def test_the_derived_values_on_hand_made_counts():
    res = _hand_made()
    assert res.rf.dtype == np.int64 and res.rf.tolist() == [[0, 3, 0, 0], [3, 0, 2, 0], [0, 2, 0, 1], [0, 0, 1, 0]]
    nrf = res.normalized_rf
    assert nrf[0, 1] == pytest.approx(3 / 5) and nrf[1, 2] == 1.0 and nrf[2, 3] == pytest.approx(1 / 3)
    assert nrf[0, 0] == 0.0 and math.isnan(nrf[0, 3]) and math.isnan(nrf[1, 3])
    mean, comparable = res.mean_distance()  # at least 4 common taxa, itself left out
    assert comparable.tolist() == [1, 2, 2, 1]
    assert mean.tolist() == pytest.approx([3 / 5, (3 / 5 + 1.0) / 2, (1.0 + 1 / 3) / 2, 1 / 3])
    mean, comparable = res.mean_distance(min_common=3)
    assert comparable.tolist() == [2, 2, 3, 1] and mean[0] == pytest.approx(3 / 10)
    mean, comparable = res.mean_distance(min_common=6)
    assert comparable.tolist() == [0, 0, 0, 0] and np.isnan(mean).all()
    worst = res.outlier_sources(2)
    assert [w["tree"] for w in worst] == [1, 2] and worst[0] == {"tree": 1, "mean_distance": pytest.approx(0.8),
                                                                 "comparable": 2}
    assert [w["tree"] for w in res.outlier_sources()] == [1, 2, 0, 3] and res.outlier_sources(0) == []


def test_the_table_lists_every_unordered_pair_once():
    head = "tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf"
    full = [head, "0\t1\t5\t3\t2\t1\t3\t0.6000", "0\t2\t3\t1\t1\t1\t0\t0.0000", "1\t2\t4\t0\t2\t0\t2\t1.0000",
            "2\t3\t4\t2\t1\t1\t1\t0.3333"]
    assert _hand_made().table().splitlines() == full
    assert _hand_made().table(min_common=4).splitlines() == [full[0], full[1], full[3], full[4]]
    # rows 2 and 0, and 2 again: the pair (0, 2) once, the pairs of 2 with trees that have no row from its side
    assert _hand_made([2, 0, 2]).table().splitlines() == full
    assert _hand_made([3]).table().splitlines() == [head, full[4]]
    assert _hand_made([1]).table().splitlines() == [head, full[1], full[3]]
