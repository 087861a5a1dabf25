"""The summed internode distances of the sources without a device: the two references of
``tests/internode_reference.py`` held to one another and to the four-point condition, the plan entry against its
restatement, the overflow bound at its edge, the bindings against the header, and the host layer -- what
``Device.score_internode`` hands to the export, how ``source_internode_distances`` names its rows and carries its
weights, the mean, the PHYLIP writer and the command-line options over a stub device."""

import ctypes as C
import random
import re
import types
from pathlib import Path

import internode_reference as ir
import numpy as np
import parsimony_reference as pr
import pytest
from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, source_internode_distances
from spectralclustersupertree_amd import cli as cli_mod
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import InternodeDistances
from spectralclustersupertree_amd.tree import make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the references
def _random_trees(rng, n) -> list:
    trees = []
    for _ in range(rng.randint(1, 6)):
        k = rng.randint(1, n)
        leaves = rng.sample(range(n), k)
        tree = pr.rand_tree(leaves, rng.choice([2, 3, 6]), rng) if k > 1 else leaves[0]
        trees.append([tree] if rng.random() < 0.3 else tree)  # (a unary root now and then)
    return trees


def test_the_two_references_agree_on_random_inputs():
    rng = random.Random(41)
    pairs = 0
    for _ in range(150):
        n = rng.randint(1, 16)
        trees = _random_trees(rng, n)
        w = None if rng.random() < 0.4 else [rng.randint(0, 4) for _ in trees]
        rows = None if rng.random() < 0.5 else [rng.randrange(n) for _ in range(rng.randint(0, 5))]
        specs = ir.specs_of(trees)
        a, b = ir.by_paths(trees, n, w, rows), ir.by_tables(specs, n, w, rows)
        c = ir.by_paths([ir.nested_of(*s) for s in specs], n, w, rows)  # (the raw arrays read back as trees)
        for key in ir.KEYS:
            assert a[key].dtype == b[key].dtype and np.array_equal(a[key], b[key]), (trees, w, rows, key)
            assert np.array_equal(a[key], c[key]), (trees, w, rows, key)
        ir.check_invariants(a, n, rows)
        pairs += int(a["taxon_partners"].sum())
    assert pairs > 2000


def test_the_definitions_on_hand_made_trees():
    assert ir.by_paths([[0, 1]], 2)["dist_sum"].tolist() == [[0, 2], [2, 0]]
    assert ir.by_paths([[[0, 1], 2]], 3)["dist_sum"].tolist() == [[0, 2, 3], [2, 0, 3], [3, 3, 0]]
    star = ir.by_tables(ir.specs_of([[0, 1, 2, 3]]), 4)
    assert (star["dist_sum"] + 2 * np.eye(4, dtype=np.int64) == 2).all() and star["taxon_sq"].tolist() == [12] * 4
    # raw depths 0, 3, 3, 5 are (0,(1,2,(3,4))), wherever the depths start; unary nodes are not counted
    for shift in (0, 4):
        r, dep, h = ir.gap_depths([shift + x for x in (0, 3, 3, 5)])
        assert r.tolist() == [0, 1, 1, 2] and dep.tolist() == [1, 2, 2, 3, 3] and h == 3
    assert ir.nested_of([0, 1, 2, 3, 4], [0, 3, 3, 5]) == [0, [1, 2, [3, 4]]]
    plain, unary = [[0, 1], 2, [3, 4, 5]], [[[[0, [1]]], [2], [[3, 4, 5]]]]
    assert ir.specs_of([plain]) != ir.specs_of([unary])
    for key in ir.KEYS:
        assert np.array_equal(ir.by_tables(ir.specs_of([plain]), 6)[key], ir.by_tables(ir.specs_of([unary]), 6)[key])
    # equal depths with a shallower gap between them are two nodes: ((0,1),(2,3)) is not a star
    assert ir.gap_depths([2, 1, 2])[0].tolist() == [1, 0, 1] and ir.gap_depths([2, 2, 2])[0].tolist() == [0, 0, 0]
    # a weight counts like copies, weight 0 like absence; a one-leaf tree changes nothing
    trees = [[[0, 1], [2, 3]], [0, [1, 2]], 3]
    a = ir.by_paths(trees, 4, [2, 0, 5])
    b = ir.by_paths([trees[0], trees[0]], 4)
    for key in ir.KEYS:
        assert np.array_equal(a[key], b[key])
    # d is taken in the tree itself, not in its restriction to the pair's common taxa
    assert ir.by_paths([[[0, [1, 4]], 2]], 5)["dist_sum"][0, 2] == 3 and ir.by_paths([[[0, 1], 2]], 5)["dist_sum"][0, 2] == 3
    assert ir.by_paths([[[[0, 4], 1], 2]], 5)["dist_sum"][0, 2] == 4


def test_single_tree_matrices_keep_the_four_point_condition():
    rng = random.Random(4)
    for _ in range(25):
        n = rng.randint(4, 11)
        tree = pr.rand_tree(list(range(n)), rng.choice([2, 3, 5]), rng)
        d = ir.by_tables(ir.specs_of([tree]), n)["dist_sum"]
        assert ir.four_point(d) and (d + 2 * np.eye(n, dtype=np.int64) >= 2).all()
    assert not ir.four_point(np.array([[0, 2, 2, 2], [2, 0, 2, 3], [2, 2, 0, 2], [2, 3, 2, 0]]))


def test_the_depths_of_a_deep_and_a_wide_tree():
    n = 70000
    ref = ir.depths_by_tables([(list(range(n)), list(range(n - 2, -1, -1))), (list(range(n)), [3] * (n - 1))])
    assert ref["tree_height"].tolist() == [n - 1, 1] and ref["gap_r"][0] == n - 2 and ref["gap_r"][n - 2] == 0
    assert ref["leaf_depth"][:3].tolist() == [n - 1, n - 1, n - 2] and ref["leaf_depth"][n:].max() == 1
    assert len(ref["gap_r"]) == 2 * n and ref["gap_r"][n - 1] == 0


# ------------------------------------------------------------------------------------------------ the plan
def _offsets(rng, n_trees, top):
    return np.concatenate([[0], np.cumsum([rng.randint(1, top) for _ in range(n_trees)])]).astype(np.int64)


@pytest.mark.parametrize("n_trees", [1, 31, 32, 33, 129, 1024, 1025, 5000])
def test_the_plan_entry_equals_its_restatement(n_trees):
    rng = random.Random(n_trees)
    for n_taxa in (1, 63, 64, 65, 256, 257, 3000, 10000):
        off = _offsets(rng, n_trees, rng.choice([2, 50, 600]))
        for n_rows, rb, tb, mats in ((None, 0, 0, 0), (None, 0, 0, 3), (5, 3, 0, 1), (0, 1, 4, 2), (None, 7, 1, 2),
                                     (None, 7, 33, 0), (70, 0, 1000, 3)):
            got = backend.debug_internode_plan(off, n_taxa, n_rows, rb, tb, mats)
            want = ir.plan(off, n_taxa, n_rows, rb, tb, mats)
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(got[key], want[key]), (n_trees, n_taxa, n_rows, rb, tb, mats, key)


def test_the_batches_their_bytes_and_their_grids():
    n, m = 10000, 500
    off = np.arange(m + 1, dtype=np.int64) * 500
    none, two, three = (backend.debug_internode_plan(off, n, matrices=k) for k in (0, 2, 3))
    assert none["row_bytes"] == 0 and two["row_bytes"] == 16 * n and none["levels"] == 9 and none["width"] == 4
    # without matrices nothing of rows x taxa: the dense rows of 500 trees (40 MB) and the tables are all there is
    assert none["fixed_bytes"] == two["fixed_bytes"] == none["bytes"] < 64 << 20
    assert none["mirror"] == 1 and none["n_row_batches"] == 1 and none["n_tree_batches"] == 1 and none["words"] == 16
    # two matrices of 10 000 x 10 000 int64 are 1.6 GB, twice the half of the block (768 MiB) the cells may take:
    # 5 033 rows of 160 000 bytes fit it, and 3 355 rows of three matrices
    assert two["n_row_batches"] == 2 and two["mirror"] == 0 and two["rows"].tolist() == [5033, 4967]
    assert two["bytes"] - two["fixed_bytes"] <= ir.BUDGET // 2 and three["rows"].tolist() == [3355, 3355, 3290]
    assert backend.debug_internode_plan(off, 5000, matrices=3)["mirror"] == 1  # 600 MB: every row at once
    # a work item is a row and several tiles while the rows alone give the device its items
    assert none["tiles"] == 40 and none["tiles_per_item"] == 40 and none["items_per_row"] == 1
    few = backend.debug_internode_plan(off, n, n_rows=3)
    assert few["tiles_per_item"] == 1 and few["items_per_row"] == 40 and few["grid"].tolist() == [120]
    # 2 000 trees over 20 000 taxa: dense rows of 320 MB, one tree batch; the knob splits them
    big = np.arange(2001, dtype=np.int64) * 500
    assert backend.debug_internode_plan(big, 20000)["n_tree_batches"] == 1
    cut = backend.debug_internode_plan(big, 20000, batch_trees=600)
    assert cut["trees"].tolist() == [600, 600, 600, 200] and cut["leaves"].tolist() == [300000] * 3 + [100000]
    # trees too many for half the block go in batches by bytes
    many = backend.debug_internode_plan(np.arange(10001, dtype=np.int64) * 20, 20000)
    # (a dense row of 20 032 x 8 bytes and 800 bytes of leaves a tree: 5 000 of them fill 768 MiB)
    assert many["trees"].tolist() == [5000, 5000] and many["trees"].sum() == 10000 and many["fixed_bytes"] <= ir.BUDGET // 2 + (64 << 20)
    # a launch stays under the work-items a dispatch counts
    wide = backend.debug_internode_plan(off[:9], 300000, n_rows=1 << 20)
    assert wide["grid_limit"] == (2**32 - 1) // 256 and wide["grid"][0] * 256 <= 2**32 - 1


def test_the_overflow_bound_at_the_limit_and_one_past_it():
    # one tree of 3 leaves and height 2: B1 = w 2 4, B2 = w 2 16; a second tree of 2 leaves adds w 2 / w 4
    off = np.array([0, 3, 5], dtype=np.int64)
    h = [2, 1]
    plan = lambda w, squares: backend.debug_internode_plan(off, 5, tree_weights=w, heights=h, squares=squares)  # noqa: E731
    w1 = ir.LIMIT // 8
    rest = ir.LIMIT - 8 * w1  # 7: three units of the second tree's 2 fit, four do not
    assert ir.bounds([3, 2], h, [w1, rest // 2])[0] == ir.LIMIT - 1
    plan([w1, rest // 2], False)
    with pytest.raises(ValueError, match=r"scs_debug_internode_plan: the bound B1 .* on dist_sum passes 2\^63 - 1 at tree 1"):
        plan([w1, rest // 2 + 1], False)
    with pytest.raises(ValueError, match="the bound B1 .* at tree 0"):
        plan([w1 + 1, 0], False)
    # (every term of B1 holds the factor 2 and 2^63 - 1 is odd: 2^63 - 2 above is the largest sum that passes, 2^63 the
    # smallest that does not)
    assert ir.bounds([3, 2], h, [w1, rest // 2 + 1])[0] == ir.LIMIT + 1
    # B2 applies only when squares are asked for
    w2 = ir.LIMIT // 32
    plan([w2, 0], True)
    plan([w2 + 1, 0], False)
    with pytest.raises(ValueError, match=r"the bound B2 .* on sq_sum passes 2\^63 - 1 at tree 0"):
        plan([w2 + 1, 0], True)
    assert ir.bounds([3, 2], h, [w2, 0])[1] <= ir.LIMIT < ir.bounds([3, 2], h, [w2 + 1, 0])[1]
    # weights of 2^62 on large trees: the sums are taken in 128 bits, not wrapped
    with pytest.raises(ValueError, match="the bound B1 .* at tree 0"):
        backend.debug_internode_plan(np.array([0, 1 << 20], dtype=np.int64), 5, tree_weights=[1 << 62],
                                     heights=[(1 << 20) - 1], squares=True)
    # trees of one leaf and of weight 0 add nothing
    backend.debug_internode_plan(np.array([0, 1, 4], dtype=np.int64), 5, tree_weights=[ir.LIMIT, 0], heights=[0, 2],
                                 squares=True)


def test_the_plan_entry_refuses_what_it_cannot_plan():
    off = np.array([0, 3, 5], dtype=np.int64)
    with pytest.raises(nv.ScsError, match="scs_debug_internode_plan: negative argument"):
        backend.debug_internode_plan(off, 10, batch_trees=-1)
    with pytest.raises(nv.ScsError, match="matrices_wanted = 4 is not 0 ... 3"):
        backend.debug_internode_plan(off, 10, matrices=4)
    with pytest.raises(nv.ScsError, match=r"tree_w\[1\] = -2 is negative"):
        backend.debug_internode_plan(off, 10, tree_weights=[1, -2])
    with pytest.raises(nv.ScsError, match="tree_off decreases at tree 1"):
        backend.debug_internode_plan(np.array([0, 3, 2], dtype=np.int64), 10)
    lib = nv.load_library()
    assert lib.scs_debug_internode_plan(None, 1, None, 1, 1, 0, 0, 0, None, None, 0, None, None, None) == nv.EINVAL
    assert lib.scs_last_error() == b"scs_debug_internode_plan: null argument"


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("symbol,count", [("scs_score_internode", 14), ("scs_debug_internode_plan", 14),
                                          ("scs_debug_internode_depths", 6)])
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
    if symbol == "scs_score_internode":
        assert params == ["scs_ctx *ctx", "const scs_tables *sources", "int32_t n_rows", "const int32_t *rows",
                          "const int64_t *tree_w", "int32_t max_batch_rows", "int32_t max_batch_trees",
                          "int64_t *pair_weight", "int64_t *dist_sum", "int64_t *sq_sum", "int64_t *taxon_weight",
                          "int64_t *taxon_sum", "int64_t *taxon_sq", "int32_t *taxon_partners"]
        assert lib.scs_score_internode(None, None, 0, None, None, 0, 0, *[None] * 7) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_internode: null argument"
    elif symbol == "scs_debug_internode_depths":
        assert lib.scs_debug_internode_depths(None, None, 0, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_debug_internode_depths: null argument"


# ------------------------------------------------------------------------------------------------ the host layer
def _at(address: int, dtype, count: int) -> np.ndarray:
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


class FakeLib:
    """``scs_score_internode`` records its arguments and answers cell [i][b] = 100 m + 10 taxon + b for matrix m,
    sum s of row i = 1000 (s + 1) + taxon and partners = taxon."""

    def __init__(self, n):
        self.n, self.calls, self.rc = n, [], 0

    def scs_last_error(self):
        return b"scs_score_internode: rows[0] = 9 is not a taxon of the tables (4 taxa)"

    def scs_score_internode(self, ctx, tabs, n_rows, rows, w, rb, tb, *outs):
        ids = list(range(self.n)) if rows is None else _at(rows, np.int32, n_rows).tolist()
        self.calls.append((n_rows, None if rows is None else ids, None if w is None else _at(w, np.int64, 3).tolist(),
                           rb, tb, [o is not None for o in outs]))
        for m, o in enumerate(outs[:3]):
            if o is not None:
                _at(o, np.int64, n_rows * self.n)[:] = [100 * m + 10 * t + b for t in ids for b in range(self.n)]
        for s, o in enumerate(outs[3:6]):
            if o is not None:
                _at(o, np.int64, n_rows)[:] = [1000 * (s + 1) + t for t in ids]
        if outs[6] is not None:
            _at(outs[6], np.int32, n_rows)[:] = ids
        return self.rc


def test_device_method_marshals_the_export():
    lib = FakeLib(4)
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3, n_taxa=4)
    got = dev.score_internode(tabs)
    assert lib.calls == [(4, None, None, 0, 0, [True, True, False, True, True, False, True])]
    assert list(got) == list(ir.KEYS) and got["sq_sum"] is None and got["taxon_sq"] is None
    assert got["pair_weight"].dtype == np.int64 and got["pair_weight"][2].tolist() == [20, 21, 22, 23]
    assert got["dist_sum"][1].tolist() == [110, 111, 112, 113] and got["taxon_sum"].tolist() == [2000, 2001, 2002, 2003]
    assert got["taxon_partners"].dtype == np.int32 and got["taxon_partners"].tolist() == [0, 1, 2, 3]
    got = dev.score_internode(tabs, rows=[2, 0, 2], tree_weights=[1, 0, 7], matrices=False, squares=True, batch_rows=5,
                              batch_trees=2)
    assert lib.calls[-1] == (3, [2, 0, 2], [1, 0, 7], 5, 2, [False, False, False, True, True, True, True])
    assert got["pair_weight"] is None and got["taxon_sq"].tolist() == [3002, 3000, 3002]
    got = dev.score_internode(tabs, rows=[], outputs=["sq_sum"])
    assert lib.calls[-1][-1] == [False, False, True, False, False, False, False] and got["sq_sum"].shape == (0, 4)
    with pytest.raises(ValueError, match="rows must be a list of taxon ids"):
        dev.score_internode(tabs, rows=[[0, 1]])
    with pytest.raises(ValueError, match=r"one weight per tree \(3\)"):
        dev.score_internode(tabs, tree_weights=[1, 2])
    with pytest.raises(ValueError, match="unknown outputs"):
        dev.score_internode(tabs, outputs=["mean"])
    lib.rc = nv.EINVAL
    with pytest.raises(ValueError, match=r"rows\[0\] = 9 is not a taxon of the tables"):
        dev.score_internode(tabs, rows=[9])


class FakeTables:
    def __init__(self, n_trees, n_taxa):
        self.n_trees, self.n_taxa, self.freed = n_trees, n_taxa, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload`` and ``score_internode`` answered by ``by_tables`` on the tables' own arrays, logged."""

    def __init__(self):
        self.log, self.tabs = [], None

    def upload(self, tables):
        self.tables = tables
        self.tabs = FakeTables(tables.n_trees, tables.n_taxa)
        return self.tabs

    def score_internode(self, tabs, rows=None, tree_weights=None, matrices=True, squares=False, batch_rows=0,
                        batch_trees=0, outputs=None):
        self.log.append((None if rows is None else np.asarray(rows).tolist(),
                         None if tree_weights is None else np.asarray(tree_weights).tolist(), matrices, squares))
        out = ir.by_tables(ir.specs_of_tables(self.tables), self.tables.n_taxa, tree_weights, rows)
        for k in ir.KEYS:
            if (not matrices and k in ir.MATRICES) or (not squares and k in ("sq_sum", "taxon_sq")):
                out[k] = None
        return out


TREES = ["((a,b),c);", "(d,(b,(e,a)));", "(a,e);", "f;"]


def test_source_internode_distances_numbers_the_union_of_the_names_and_frees_the_tables():
    dev = FakeDevice()
    trees = [make_tree(t) for t in TREES]
    res = source_internode_distances(trees, device=dev)
    assert dev.log == [(None, None, True, False)] and dev.tabs.freed == 1 and dev.tables.n_taxa == 6
    assert isinstance(res, InternodeDistances) and res.taxa == ["a", "b", "c", "d", "e", "f"]
    assert res.rows.tolist() == [0, 1, 2, 3, 4, 5] and res.sq_sum is None and res.taxon_sq is None
    # a-b: 2 in the first tree, 3 in the second; a-e: 2 and 2; f is with nobody
    assert res.pair_weight[0].tolist() == [0, 2, 1, 1, 2, 0] and res.dist_sum[0].tolist() == [0, 5, 3, 4, 4, 0]
    assert res.mean[0, 1] == 2.5 and res.mean[0, 4] == 2.0 and np.isnan(res.mean[0, 5]) and res.mean[5, 5] == 0.0
    assert np.isnan(res.mean[2, 3]) and res.mean.dtype == np.float64 and not res.mean.diagonal().any()
    assert res.taxon_partners.tolist() == [4, 4, 2, 3, 3, 0] and res.missing_pairs == 15 - 8 and res.complete is False
    assert res.taxon_mean[0] == 16 / 6 and np.isnan(res.taxon_mean[5])
    assert set(res.timings) == {"prepare", "tables", "internode"}
    with pytest.raises(ValueError, match="variance needs the squares"):
        res.variance
    assert res.table().splitlines()[:2] == ["taxon\tpartners\tweight\tsum\tmean", "a\t4\t6\t16\t2.6667"]
    assert res.table().splitlines()[-1] == "f\t0\t0\t0\tnan"
    near = res.nearest("a")
    assert [x["name"] for x in near] == ["e", "b", "c", "d"] and near[1] == {"taxon": 1, "name": "b", "mean": 2.5,
                                                                           "weight": 2}
    assert res.nearest(0, 1) == near[:1] and res.nearest("f") == []


def test_rows_weights_squares_and_no_matrices():
    dev = FakeDevice()
    trees = [make_tree(t) for t in TREES]
    res = source_internode_distances(trees, rows=["e", 0, "e"], tree_weights=[1.0, 3, 0, 2], squares=True, device=dev)
    assert dev.log == [([4, 0, 4], [1, 3, 0, 2], True, True)] and res.rows.tolist() == [4, 0, 4]
    assert res.missing_pairs is None and res.complete is None
    assert res.pair_weight[1].tolist() == [0, 4, 1, 3, 3, 0] and res.dist_sum[1].tolist() == [0, 11, 3, 12, 6, 0]
    var = res.variance
    assert var[1, 1] == pytest.approx(31 / 4 - (11 / 4) ** 2) and var[1, 4] == 0.0 and np.isnan(var[1, 5])
    assert var[0, 4] == 0.0 and var[1, 0] == 0.0  # the diagonal, wherever the row's taxon stands
    with pytest.raises(ValueError, match="to_phylip needs every taxon as a row"):
        res.to_phylip("nowhere.phy")
    with pytest.raises(ValueError, match="is not a row of these distances"):
        res.nearest("b")
    lean = source_internode_distances(trees, matrices=False, device=dev)
    assert dev.log[-1] == (None, None, False, False) and lean.pair_weight is None and lean.missing_pairs == 7
    assert lean.taxon_sum.tolist() == res.taxon_sum.tolist()[:0] + lean.taxon_sum.tolist() and lean.table()
    with pytest.raises(ValueError, match="mean needs the matrices"):
        lean.mean
    for rows, bad in ((["x"], "'x'"), ([6], "6"), ([-1], "-1")):
        with pytest.raises(ValueError, match=f"rows must be names or ids of the 6 taxa of the sources, not {bad}"):
            source_internode_distances(trees, rows=rows, device=dev)
    for w, said in (([1, 2, 3], r"one entry per source tree \(4\)"), ([1, 1.5, 1, 1], "must be non-negative integers"),
                    ([1, -1, 1, 1], "must be non-negative integers"), ([True] * 4, "must be non-negative integers")):
        with pytest.raises(ValueError, match=said):
            source_internode_distances(trees, tree_weights=w, device=dev)
    with pytest.raises(ValueError, match="at least one tree"):
        source_internode_distances([], device=dev)
    # a supertree's own matrix: one tree, every pair there
    own = source_internode_distances([make_tree("((a,b),(c,(d,e)));")], device=dev)
    assert own.complete is True and own.dist_sum[0].tolist() == [0, 2, 4, 5, 5] and ir.four_point(own.dist_sum)


def test_the_weights_of_tree_arrays_follow_the_trees_that_have_tables(monkeypatch):
    # as TreeArrays the trees of fewer than two leaves have no tables: their weights are dropped with them
    dev = FakeDevice()
    trees = [make_tree(t) for t in ["f;", *TREES, "b;"]]
    names = sorted({n for t in trees for n in t.get_tip_names()})
    arrays = TreeArrays.from_trees(trees, [1.0] * len(trees), names)
    w = [9, 1, 3, 0, 2, 9]
    want = source_internode_distances(trees, tree_weights=w, squares=True, device=dev)

    class Resident:
        def __init__(self, device, given, tips, index):
            self.tips = tips

        def __enter__(self):
            from spectralclustersupertree_amd.flatten import flatten_trees

            kept = [t for t in trees if len(t.get_tip_names()) >= 2]
            dev.upload(flatten_trees(kept, [1.0] * len(kept), "one", taxa=self.tips))
            return types.SimpleNamespace(dev=dev, tabs=dev.tabs, n_leaves=arrays.leaf_counts(), seconds=0.0,
                                         tree_index=lambda: np.array([1, 2, 3]))

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    got = source_internode_distances(arrays, tree_weights=w, squares=True, device=dev)
    assert dev.log[-1][1] == [1, 3, 0] and got.taxa == names
    order = [want.taxa.index(n) for n in names]
    for key in ir.MATRICES:
        assert np.array_equal(getattr(got, key), getattr(want, key)[np.ix_(order, order)])
    assert np.array_equal(got.taxon_partners, want.taxon_partners[order])


def test_to_phylip_writes_the_mean_and_refuses_missing_pairs(tmp_path):
    dev = FakeDevice()
    res = source_internode_distances([make_tree(t) for t in TREES[:2]], device=dev)
    path = tmp_path / "matrix.phy"
    with pytest.raises(ValueError, match=r"2 pairs of taxa are in no tree together \(the first: 'c', 'd'\)"):
        res.to_phylip(path)
    assert not path.exists()
    res.to_phylip(path, missing=-1)
    lines = path.read_text().splitlines()
    assert lines[0] == "5" and [x.split()[0] for x in lines[1:]] == ["a", "b", "c", "d", "e"]
    assert lines[1].split()[1:] == ["0.000000", "2.500000", "3.000000", "4.000000", "2.000000"]
    assert lines[3].split()[1:] == ["3.000000", "3.000000", "0.000000", "-1.000000", "-1.000000"]
    whole = source_internode_distances([make_tree("((a,b),c);")], device=dev)
    whole.to_phylip(path)
    assert path.read_text() == "3\na 0.000000 2.000000 3.000000\nb 2.000000 0.000000 3.000000\nc 3.000000 3.000000 0.000000\n"


def test_the_command_line_writes_the_matrix_and_the_table(monkeypatch, tmp_path):
    calls = []
    dev = FakeDevice()
    real = score_mod.source_internode_distances

    def fake(trees, rows=None, tree_weights=None, squares=False, matrices=True, device=None):
        calls.append((type(trees).__name__, rows, matrices))
        return real([make_tree("((a,b),c);"), make_tree("(a,d);")], matrices=matrices, device=dev)

    import spectralclustersupertree_amd as pkg

    monkeypatch.setattr(score_mod, "source_internode_distances", fake)
    monkeypatch.setattr(pkg, "construct_supertree", lambda sources, **kw: make_tree("((a,b),c);"))
    src, out, phy, tsv = (tmp_path / x for x in ("in.tre", "out.tre", "matrix.phy", "taxa.tsv"))
    src.write_text("((a,b),c);\n(a,d);\n")
    base = ["-i", str(src), "-o", str(out)]
    res = CliRunner().invoke(cli_mod.scs, [*base, "--internode-taxa-out", str(tsv)])
    assert res.exit_code == 0, res.output
    assert calls == [("TreeArrays", None, False)] and not phy.exists()  # the table alone asks for no matrix
    assert tsv.read_text().splitlines() == ["taxon\tpartners\tweight\tsum\tmean", "a\t3\t3\t7\t2.3333",
                                            "b\t2\t2\t5\t2.5000", "c\t2\t2\t6\t3.0000", "d\t1\t1\t2\t2.0000"]
    res = CliRunner().invoke(cli_mod.scs, [*base, "--internode-out", str(phy)])
    assert res.exit_code != 0 and "in no tree together" in res.output and calls[-1] == ("TreeArrays", None, True)
    res = CliRunner().invoke(cli_mod.scs, [*base, "--internode-out", str(phy), "--internode-missing", "9.5"])
    assert res.exit_code == 0, res.output
    assert phy.read_text().splitlines()[4] == "d 2.000000 9.500000 9.500000 0.000000"
    res = CliRunner().invoke(cli_mod.scs, [*base, "--internode-missing", "1"])
    assert res.exit_code != 0 and "--internode-missing needs --internode-out" in res.output
    n = len(calls)
    res = CliRunner().invoke(cli_mod.scs, base)
    assert res.exit_code == 0 and len(calls) == n  # the options are the only way in
