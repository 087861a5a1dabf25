"""The pairwise rooted-triplet terms of the sources without a device: the two references of
``tests/source_triplets_reference.py`` held to one another, to counts written out by hand and to
``tests/triplet_reference.py``, the plan entry against its restatement, the bindings against the header, and the host
layer -- what ``Device.score_source_pair_triplets`` hands to the export, how ``source_distances(triplets=True)`` brings
the answers back to the trees as given, the derived values and the table on hand-made counts."""

import ctypes as C
import math
import random
import re
import types
from math import comb
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest
import source_triplets_reference as st
import triplet_reference as tr

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, source_distances
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import SourceDistances
from spectralclustersupertree_amd.tree import make_tree

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
    rng = random.Random(38)
    cells = partial = empty = graded = 0
    for _ in range(120):
        n = rng.randint(1, 22)
        trees = [random_tree(rng, n) for _ in range(3)]
        a, b = st.by_sets(trees), st.quadratic(trees)
        for k in st.KEYS:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (trees, k, a[k], b[k])
        st.check_invariants(a)
        c = a["common"].astype(np.int64)
        assert (a["triplets"] <= c * (c - 1) * (c - 2) // 6).all()
        assert (a["triplets_shared"] <= np.minimum(a["triplets"], a["triplets_other"])).all()
        cells += 9
        sizes = np.array([len(pr.leaves_of(t)) for t in trees])
        partial += int(((c > 0) & (c < np.minimum.outer(sizes, sizes))).sum())
        empty += int((c == 0).sum())
        graded += int(((a["triplets_shared"] > 0) & (a["triplets_shared"] < np.minimum(a["triplets"],
                                                                                      a["triplets_other"]))).sum())
    assert cells == 1080 and partial > 100 and empty > 10 and graded > 100


def test_hand_made_pairs():
    # ((a,b),(c,d)) resolves all four triples, the caterpillar (((a,b),c),d) too; they agree on ab|c and ab|d only.
    # ((a,c),(b,d)) shares nothing with the first and ac|d with the second; ((a,b,c),d) leaves abc a fan
    trees = [[[0, 1], [2, 3]], [[[0, 1], 2], 3], [[0, 2], [1, 3]], [[0, 1, 2], 3]]
    for ref in (st.by_sets(trees), st.quadratic(trees)):
        assert ref["triplets"].tolist() == [[4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 4, 4], [3, 3, 3, 3]]
        assert ref["triplets_shared"].tolist() == [[4, 2, 0, 1], [2, 4, 1, 3], [0, 1, 4, 1], [1, 3, 1, 3]]
    # one rogue leaf: 9 moved from one end of a caterpillar of 10 to the other breaks every cluster (RF at its
    # ceiling) but only the C(9, 2) triples it is in
    a, b = pr.caterpillar(range(10)), pr.caterpillar([9, *range(9)])
    for pair in (st.pair_by_sets, st.pair_quadratic):
        assert pair(a, b) == (10, comb(10, 3), comb(10, 3), comb(9, 3))
        # a chain of nodes over one restricted set counts once; a polytomy the restriction makes binary resolves
        assert pair([[[[[0, 9], 1], 8], 7], [2, 3]], [[0, 1], [2, 3]]) == (4, 4, 4, 4)
        assert pair([[0, 1], [2, 3], [8, 9]], [[0, 1], [2, 3]]) == (4, 4, 4, 4)
        assert pair([[[[0, 9], 8], 7], 1, 2], [[0, 1], 2]) == (3, 0, 1, 0)
        assert pair([[0, 1], 2], [3, 4]) == (0, 0, 0, 0) and pair([0, 1, 2], [[0, 1], [2, 5]]) == (3, 0, 1, 0)


def _newick(tree) -> str:
    return "(" + ",".join(_newick(x) for x in tree) + ")" if isinstance(tree, list) else f"t{tree}"


def test_the_row_of_a_tree_over_all_taxa_is_the_supertree_score():
    rng = random.Random(15)
    n = 40
    sup = pr.rand_tree(range(n), 4, rng)
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(2, n)), 3, rng) for _ in range(12)]
    want = tr.quadratic(make_tree(_newick(sup) + ";"), [make_tree(_newick(t) + ";") for t in trees])
    got = st.quadratic([*trees, sup], rows=[12])
    assert np.array_equal(got["triplets"][0, :12], want["t_super"])
    assert np.array_equal(got["triplets_other"][0, :12], want["t_source"])
    assert np.array_equal(got["triplets_shared"][0, :12], want["t_shared"]) and want["t_shared"].sum() > 0


# ------------------------------------------------------------------------------------------------ the plan
def _forests():
    rng = random.Random(9)
    yield [700, 3, 130, 1, 515, 64, 2]
    yield [500] * 40
    yield [65, 64, 66, 63, 1, 2]
    yield [rng.randint(1, 300) for _ in range(60)]
    yield [70000, 100, 65536]
    yield [1]
    yield [327679, 5, 327679]


@pytest.mark.parametrize("knobs", [{}, {"batch_trees": 2}, {"chunk_pairs": 3}, {"batch_trees": 16, "chunk_pairs": 7},
                                   {"lds_bytes": 163840}, {"lds_bytes": 40000, "chunk_pairs": 1},
                                   {"rows": [0]}, {"rows": "some", "batch_trees": 3, "chunk_pairs": 5}])
def test_the_plan_entry_against_its_restatement(knobs):
    rng = random.Random(len(str(knobs)))
    for sizes in _forests():
        kw = dict(knobs)
        if kw.get("rows") == "some":
            kw["rows"] = [rng.randrange(len(sizes)) for _ in range(rng.randint(1, 2 * len(sizes)))]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        try:
            ref = st.plan(off, 1000, **kw)
        except ValueError as refusal:  # (a cap that does not hold the rows of the largest pair)
            with pytest.raises(ValueError, match=re.escape(str(refusal))):
                backend.debug_source_pair_triplets_plan(off, 1000, **kw)
            assert "lds_bytes" in kw and max(sizes) > 80000
            continue
        got = backend.debug_source_pair_triplets_plan(off, 1000, **kw)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), (sizes[:4], kw, k, got[k], ref[k])
        # every launch under the work-item limit; the chunks cover every pair of every tile once, in order
        ch = got["chunks"]
        assert (ch[:, 3] * 256 < 1 << 32).all() and (ch[:, 6] * 256 < 1 << 32).all() and (ch[:, 3] >= 1).all()
        assert ch[:, 3].sum() == got["pairs"].sum() and (ch[:, 4] + ch[:, 5] <= ch[:, 3]).all()
        for i, j in np.argwhere(got["tile_rows"] > 0):
            mine = ch[(ch[:, 0] == i) & (ch[:, 1] == j)]
            assert len(mine) == got["n_chunks"][i, j] and mine[0, 2] == 0 and (mine[:, 3] <= got["chunk_cap"][i, j]).all()
            assert np.array_equal(mine[1:, 2], np.cumsum(mine[:-1, 3]))
            assert got["lds_pairs"][i, j] <= got["lds_cap"] and got["zb"][i, j] * 16 * got["words"][i, j] <= got["lds_cap"]
        assert got["region_bytes"] >= (got["chunk_cap"] * got["pair_bytes"]).max()


def test_large_tiles_are_cut_into_chunks_under_the_byte_budget_and_the_launch_limit():
    # 400 trees of 100 000 leaves, 8 rows: 3 200 pairs of 99 998 sweep workgroups each, 320 million in all.  The
    # regions of a chunk stay under 512 MiB, which here keeps every launch under the 16 777 215 workgroups too
    off = np.arange(401, dtype=np.int64) * 100000
    got = backend.debug_source_pair_triplets_plan(off, 100000, rows=list(range(8)))
    ref = st.plan(off, 100000, rows=list(range(8)))
    assert np.array_equal(got["chunks"], ref["chunks"]) and len(got["chunks"]) > 20 and len(got["bstart"]) > 2
    assert got["chunks"][:, 6].max() <= got["grid_limit"] == 16777215 < got["chunks"][:, 6].sum() == 3200 * 99998
    assert got["region_bytes"] <= 512 << 20 and (got["zb"][0] == 1).all()


def test_the_plan_refuses_what_the_export_refuses():
    off = np.array([0, 327680, 2 * 327680, 2 * 327680 + 5], dtype=np.int64)
    for plan in (backend.debug_source_pair_triplets_plan, st.plan):
        with pytest.raises(ValueError, match="trees of 327680 and 327680 leaves may share more than the 327679 taxa a "
                                             "bitset row holds in LDS"):
            plan(off, 10)
        assert plan(off, 10, rows=[2])["max_common"][0, 0] == 5  # (the rows decide: no pair of the call is that large)
        with pytest.raises(ValueError, match="max_lds_bytes = 64 does not hold the bitset rows of trees of 400 and 500"):
            plan(np.array([0, 500, 900], dtype=np.int64), 600, rows=[1], batch_trees=1, lds_bytes=64)
    with pytest.raises(ValueError, match="scs_debug_source_pair_triplets_plan: negative argument"):
        backend.debug_source_pair_triplets_plan(np.array([0, 5], dtype=np.int64), 10, chunk_pairs=-1)
    with pytest.raises(ValueError, match="scs_debug_source_pair_triplets_plan: tree_off decreases at tree 1"):
        backend.debug_source_pair_triplets_plan(np.array([0, 5, 3], dtype=np.int64), 10)
    with pytest.raises(ValueError, match=r"rows\[1\] = 2 is not one of the 2 trees"):
        backend.debug_source_pair_triplets_plan(np.array([0, 5, 8], dtype=np.int64), 10, rows=[0, 2])
    lib = nv.load_library()
    assert lib.scs_debug_source_pair_triplets_plan(None, 1, None, 1, 1, None, 0, 0, 0, None, None, None, None,
                                                   None) == nv.EINVAL
    assert lib.scs_last_error() == b"scs_debug_source_pair_triplets_plan: null argument"


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("symbol,count", [("scs_score_source_pair_triplets", 11),
                                          ("scs_debug_source_pair_triplets_plan", 14)])
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
    if symbol == "scs_score_source_pair_triplets":
        assert params == ["scs_ctx *ctx", "const scs_tables *sources", "int32_t n_rows", "const int32_t *rows",
                          "int32_t max_batch_trees", "int32_t max_lds_bytes", "int32_t max_chunk_pairs",
                          "int32_t *common", "int64_t *triplets", "int64_t *triplets_other", "int64_t *triplets_shared"]
        assert lib.scs_score_source_pair_triplets(None, None, 0, None, 0, 0, 0, None, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_source_pair_triplets: null argument"


# ------------------------------------------------------------------------------------------------ the host layer
def _at(address: int, dtype, count: int) -> np.ndarray:
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


def _cell(x: int, t: int, j: int) -> int:
    return (x << 33) + 10 * t + j if x else 10 * t + j  # (the int64 outputs past 32 bits)


class FakeLib:
    """``scs_score_source_pair_triplets`` records its arguments and answers cell [i][j] = ``_cell(x, tree, j)`` for
    output x."""

    def __init__(self, m):
        self.m, self.calls, self.rc = m, [], 0

    def scs_last_error(self):
        return b"scs_score_source_pair_triplets: rows[0] = 9 is not a tree of the tables (3 trees)"

    def scs_score_source_pair_triplets(self, ctx, tabs, n_rows, rows, batch, lds, chunk, *outs):
        ids = list(range(self.m)) if rows is None else _at(rows, np.int32, n_rows).tolist()
        self.calls.append((n_rows, None if rows is None else ids, batch, lds, chunk, [o is not None for o in outs]))
        for x, o in enumerate(outs):
            if o is not None:
                _at(o, np.int64 if x else np.int32, n_rows * self.m)[:] = [_cell(x, t, j) for t in ids
                                                                          for j in range(self.m)]
        return self.rc


def test_device_method_marshals_the_export():
    lib = FakeLib(3)
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3)
    got = dev.score_source_pair_triplets(tabs)
    assert lib.calls == [(3, None, 0, 0, 0, [True] * 4)] and list(got) == list(st.KEYS)
    assert got["common"].dtype == np.int32 and got["common"].tolist() == [[0, 1, 2], [10, 11, 12], [20, 21, 22]]
    assert got["triplets_shared"].dtype == np.int64 and got["triplets_shared"][2].tolist() == [_cell(3, 2, j) for j in range(3)]
    got = dev.score_source_pair_triplets(tabs, rows=[2, 0, 2], batch_trees=5, lds_bytes=4096, chunk_pairs=9,
                                         outputs=("triplets",))
    assert lib.calls[-1] == (3, [2, 0, 2], 5, 4096, 9, [False, True, False, False])
    assert got["common"] is None and got["triplets"][:, 0].tolist() == [_cell(1, 2, 0), _cell(1, 0, 0), _cell(1, 2, 0)]
    assert dev.score_source_pair_triplets(tabs, rows=[])["triplets"].shape == (0, 3)
    with pytest.raises(ValueError, match="rows must be a list of tree ids"):
        dev.score_source_pair_triplets(tabs, rows=[[0, 1]])
    lib.rc = nv.EINVAL
    with pytest.raises(ValueError, match=r"rows\[0\] = 9 is not a tree of the tables"):
        dev.score_source_pair_triplets(tabs, rows=[9])


class FakeTables:
    def __init__(self, n_trees):
        self.n_trees, self.freed = n_trees, 0

    def free(self):
        self.freed += 1


RF_KEYS = ("common", "clusters", "clusters_other", "shared")


class FakeDevice:
    """``upload``, ``score_source_pairs`` (cell [i][j] = 100 x + 10 tree + j) and ``score_source_pair_triplets``
    (``_cell``), logged."""

    def __init__(self):
        self.log, self.tabs = [], None

    def upload(self, tables):
        self.tabs = FakeTables(tables.n_trees)
        self.tables = tables
        return self.tabs

    def score_source_pairs(self, tabs, rows=None, batch_trees=0, lds_bytes=0):
        m = tabs.n_trees
        self.log.append(("rf", None if rows is None else np.asarray(rows).tolist()))
        ids = list(range(m)) if rows is None else [int(r) for r in rows]
        return {k: np.array([[100 * x + 10 * t + j for j in range(m)] for t in ids], dtype=np.int32).reshape(len(ids), m)
                for x, k in enumerate(RF_KEYS)}

    def score_source_pair_triplets(self, tabs, rows=None, batch_trees=0, lds_bytes=0, chunk_pairs=0,
                                   outputs=st.KEYS):
        m = tabs.n_trees
        self.log.append(("triplets", None if rows is None else np.asarray(rows).tolist(), tuple(outputs)))
        ids = list(range(m)) if rows is None else [int(r) for r in rows]
        return {k: np.array([[_cell(x, t, j) for j in range(m)] for t in ids], dtype=np.int64).reshape(len(ids), m)
                if k in outputs else None for x, k in enumerate(st.KEYS)}


def test_source_distances_asks_for_the_triplets_only_when_told_to():
    dev = FakeDevice()
    trees = [make_tree("((a,b),c);"), make_tree("(d,(b,e));"), make_tree("(a,e);")]
    res = source_distances(trees, device=dev)
    assert dev.log == [("rf", None)] and res.triplets is None and res.triplets_other is None and res.triplets_shared is None
    assert set(res.timings) == {"prepare", "tables", "pairs"}
    assert res.table().splitlines()[0] == "tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf"
    res = source_distances(trees, device=dev, triplets=True)
    assert dev.log[1:] == [("rf", None), ("triplets", None, st.KEYS[1:])] and dev.tabs.freed == 1
    assert set(res.timings) == {"prepare", "tables", "pairs", "triplets"}
    assert res.common.tolist() == [[0, 1, 2], [10, 11, 12], [20, 21, 22]] and res.shared[1, 2] == 312
    assert res.triplets.dtype == np.int64 and res.triplets[1].tolist() == [_cell(1, 1, j) for j in range(3)]
    assert res.triplets_shared[2, 0] == _cell(3, 2, 0) and res.triplets_other[0, 2] == _cell(2, 0, 2)
    res = source_distances(trees, rows=[2, 0], device=dev, triplets=True)
    assert dev.log[-1] == ("triplets", [2, 0], st.KEYS[1:]) and res.rows.tolist() == [2, 0]
    assert res.triplets[:, 1].tolist() == [_cell(1, 2, 1), _cell(1, 0, 1)]


def test_the_triplet_counts_go_back_to_the_trees_as_given_on_both_axes(monkeypatch):
    # tables that hold the given trees 3, 0 and 4 (in that order) of five: trees 1 and 2 have no tables
    dev = FakeDevice()

    class Resident:
        def __init__(self, device, trees, tips, index):
            pass

        def __enter__(self):
            return types.SimpleNamespace(dev=dev, tabs=FakeTables(3), n_leaves=np.array([5, 1, 1, 5, 3]), seconds=0.0,
                                         tree_index=lambda: np.array([3, 0, 4], dtype=np.int64))

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    monkeypatch.setattr(score_mod, "_source_names", lambda trees: ["x", "y"])
    res = source_distances(object(), device=dev, triplets=True)
    assert dev.log == [("rf", [1, 0, 2]), ("triplets", [1, 0, 2], st.KEYS[1:])]
    assert res.triplets.shape == (5, 5) and not res.triplets[[1, 2]].any() and not res.triplets_shared[:, [1, 2]].any()
    # given tree 3 is tree 0 of the tables, given 0 is 1, given 4 is 2
    assert res.triplets[3, [3, 0, 4]].tolist() == [_cell(1, 0, j) for j in range(3)]
    assert res.triplets_other[0, [3, 0, 4]].tolist() == [_cell(2, 1, j) for j in range(3)]
    assert res.triplets_shared[4, [3, 0, 4]].tolist() == [_cell(3, 2, j) for j in range(3)]
    res = source_distances(object(), rows=[4, 1, 3], device=dev, triplets=True)
    assert dev.log[-1] == ("triplets", [2, 0], st.KEYS[1:]) and res.rows.tolist() == [4, 1, 3]
    assert res.triplets[:, [3, 0, 4]].tolist() == [[_cell(1, 2, j) for j in range(3)], [0, 0, 0],
                                                   [_cell(1, 0, j) for j in range(3)]]
    res = source_distances(object(), rows=[3, 0, 4], device=dev, triplets=True)
    assert dev.log[-1] == ("triplets", None, st.KEYS[1:])  # every tree of the tables in their order: the mirror


def test_without_tables_every_triplet_count_is_zero(monkeypatch):
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
    res = source_distances(object(), triplets=True)
    assert res.triplets.shape == (2, 2) and res.triplets.dtype == np.int64 and not res.triplets_shared.any()
    assert res.triplet_distance.tolist() == [[0, 0], [0, 0]] and np.isnan(res.normalized_triplet_distance).all()
    assert res.table() == ("tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf\ttriplets_a\t"
                           "triplets_b\ttriplets_shared\ttriplet_distance\tnormalized_triplet_distance\n")
    assert res.outlier_sources(by="triplets") == [] and np.isnan(res.mean_distance(by="triplets")[0]).all()


def _hand_made(rows=None, triplets=True) -> SourceDistances:
    common = np.array([[6, 5, 3, 2], [5, 7, 4, 0], [3, 4, 4, 4], [2, 0, 4, 9]], dtype=np.int32)
    clusters = np.array([[4, 3, 1, 0], [2, 5, 0, 0], [1, 2, 2, 2], [0, 0, 1, 6]], dtype=np.int32)
    shared = np.array([[4, 1, 1, 0], [1, 5, 0, 0], [1, 0, 2, 1], [0, 0, 1, 6]], dtype=np.int32)
    trip = np.array([[20, 10, 1, 0], [8, 30, 0, 0], [1, 4, 4, 3], [0, 0, 2, 80]], dtype=np.int64)
    both = np.array([[20, 6, 1, 0], [6, 30, 0, 0], [1, 0, 4, 1], [0, 0, 1, 80]], dtype=np.int64)
    rows = np.arange(4) if rows is None else np.asarray(rows)
    more = {"triplets": trip[rows], "triplets_other": trip.T[rows], "triplets_shared": both[rows]} if triplets else {}
    return SourceDistances(common=common[rows], clusters=clusters[rows], clusters_other=clusters.T[rows],
                           shared=shared[rows], rows=rows, n_leaves=np.array([6, 7, 4, 9]), **more)


def test_the_derived_triplet_values_on_hand_made_counts():
    res = _hand_made()
    assert res.triples_total.dtype == np.int64 and res.triples_total[0].tolist() == [20, 10, 1, 0]
    td = res.triplet_distance
    assert td.dtype == np.int64 and td.tolist() == [[0, 6, 0, 0], [6, 0, 4, 0], [0, 4, 0, 3], [0, 0, 3, 0]]
    ntd = res.normalized_triplet_distance
    assert ntd[0, 1] == pytest.approx(6 / 18) and ntd[1, 2] == 1.0 and ntd[2, 3] == pytest.approx(3 / 5)
    assert ntd[0, 0] == 0.0 and math.isnan(ntd[0, 3]) and math.isnan(ntd[1, 3]) and ntd[0, 2] == 0.0
    mean, comparable = res.mean_distance(by="triplets")  # at least 4 common taxa, itself left out
    assert comparable.tolist() == [1, 2, 2, 1]
    assert mean.tolist() == pytest.approx([1 / 3, (1 / 3 + 1.0) / 2, (1.0 + 3 / 5) / 2, 3 / 5])
    mean, comparable = res.mean_distance(min_common=3, by="triplets")
    assert comparable.tolist() == [2, 2, 3, 1] and mean[0] == pytest.approx(1 / 6)
    worst = res.outlier_sources(2, by="triplets")
    assert [w["tree"] for w in worst] == [2, 1] and worst[0] == {"tree": 2, "mean_distance": pytest.approx(0.8),
                                                                 "comparable": 2}
    assert [w["tree"] for w in res.outlier_sources(by="triplets")] == [2, 1, 3, 0]
    # by="rf" is the default and is what it was
    assert [w["tree"] for w in res.outlier_sources()] == [w["tree"] for w in res.outlier_sources(by="rf")] == [1, 2, 0, 3]
    assert res.mean_distance()[0].tolist() == pytest.approx([3 / 5, (3 / 5 + 1.0) / 2, (1.0 + 1 / 3) / 2, 1 / 3])


def test_by_triplets_needs_the_matrices():
    plain = _hand_made(triplets=False)
    for ask in (lambda: plain.mean_distance(by="triplets"), lambda: plain.outlier_sources(by="triplets"),
                lambda: plain.triplet_distance, lambda: plain.normalized_triplet_distance):
        with pytest.raises(ValueError, match="the triplet matrices are not there"):
            ask()
    with pytest.raises(ValueError, match="by must be 'rf' or 'triplets'"):
        plain.mean_distance(by="quartets")
    assert plain.triples_total[1].tolist() == [10, 35, 4, 0] and plain.outlier_sources()[0]["tree"] == 1


def test_the_table_appends_the_triplet_columns_only_with_the_matrices():
    head = "tree_a\ttree_b\tcommon\tclusters_a\tclusters_b\tshared\trf\tnormalized_rf"
    more = "\ttriplets_a\ttriplets_b\ttriplets_shared\ttriplet_distance\tnormalized_triplet_distance"
    plain = [head, "0\t1\t5\t3\t2\t1\t3\t0.6000", "0\t2\t3\t1\t1\t1\t0\t0.0000", "1\t2\t4\t0\t2\t0\t2\t1.0000",
             "2\t3\t4\t2\t1\t1\t1\t0.3333"]
    full = [plain[0] + more, plain[1] + "\t10\t8\t6\t6\t0.3333", plain[2] + "\t1\t1\t1\t0\t0.0000",
            plain[3] + "\t0\t4\t0\t4\t1.0000", plain[4] + "\t3\t2\t1\t3\t0.6000"]
    assert _hand_made(triplets=False).table().splitlines() == plain
    assert _hand_made().table().splitlines() == full
    assert _hand_made().table(min_common=4).splitlines() == [full[0], full[1], full[3], full[4]]
    # rows 2 and 0, and 2 again: the pair (0, 2) once, the pairs of 2 with trees that have no row from its side
    assert _hand_made([2, 0, 2]).table().splitlines() == full
    assert _hand_made([3]).table().splitlines() == [full[0], full[4]]
    assert _hand_made([1]).table().splitlines() == [full[0], full[1], full[3]]
