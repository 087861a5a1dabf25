"""The triple coverage of the sources without a device: the two references of ``tests/coverage_reference.py`` held to
one another, the plan entry against its restatement, the bindings against the header, and the host layer -- what
``Device.score_coverage`` hands to the export, how ``source_coverage`` names its rows, adds the one-leaf trees of a
``TreeArrays`` and derives its totals, the table and the command-line option over a stub device."""

import ctypes as C
import math
import random
import re
import types
from pathlib import Path

import coverage_reference as cr
import numpy as np
import pytest
from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, source_coverage
from spectralclustersupertree_amd import cli as cli_mod
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import SourceCoverage
from spectralclustersupertree_amd.tree import make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the references
def test_the_two_references_agree_on_random_inputs():
    rng = random.Random(36)
    covered = uncovered = 0
    for _ in range(60):
        n = rng.randint(1, 24)
        sets = cr.random_sets(rng, n, rng.randint(1, 10), 1, rng.choice([3, 8, 24]))
        last = None
        for k in (1, 2, 3):
            a, b = cr.by_sets(sets, n, k), cr.by_matmul(sets, n, k)
            for key in (*cr.KEYS, "covered"):
                assert np.array_equal(a[key], b[key]), (sets, k, key)
            assert a["pair_trees"].dtype == b["pair_trees"].dtype == np.int32 and b["taxon_covered"].dtype == np.int64
            cr.check_invariants(a, n, k)
            if last is not None:
                cr.check_monotone(last, a)
            last = a
        covered += a["covered"]
        uncovered += n * (n - 1) * (n - 2) // 6 - a["covered"]
        rows = [n - 1, 0, n - 1]
        sub = cr.by_matmul(sets, n, 2, rows)
        cr.check_invariants(sub, n, 2, rows)
        assert np.array_equal(sub["pair_covered"], cr.by_sets(sets, n, 2)["pair_covered"][rows])
    assert covered > 100 and uncovered > 1000


def test_the_definitions_on_hand_made_sources():
    # {0,1,2} twice and {2,3}: one triple, covered by two trees; taxon 4 is in no tree
    sets = [[0, 1, 2], [2, 1, 0], [2, 3]]
    one, two, three = (cr.by_sets(sets, 5, k) for k in (1, 2, 3))
    assert one["occurs"].tolist() == [2, 2, 3, 1, 0] and one["covered"] == two["covered"] == 1 and three["covered"] == 0
    assert one["pair_trees"][2].tolist() == [2, 2, 3, 1, 0] and one["pair_covered"][0].tolist() == [0, 1, 1, 0, 0]
    assert one["taxon_covered"].tolist() == [1, 1, 1, 0, 0]
    # identical trees on all taxa: every triple; disjoint trees: none across them
    assert cr.by_matmul([range(6)] * 2, 6, 2)["covered"] == 20
    assert cr.by_matmul([[0, 1, 2], [3, 4, 5]], 6)["covered"] == 2


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("n_trees", [0, 1, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 100000])
def test_the_plan_entry_equals_its_restatement(n_trees):
    for n_taxa in (0, 1, 63, 64, 65, 300, 10000):
        for n_rows, k, batch, reg, mats in ((None, 1, 0, 0, 0), (None, 2, 0, 0, 2), (5, 1, 3, 0, 1), (0, 3, 1, 4, 2),
                                            (None, 1, 7, 16, 2), (None, 1, 7, 1, 0), (70, 2, 0, 64, 2)):
            got = backend.debug_coverage_plan(n_trees, n_taxa, n_rows, k, batch, reg, mats)
            want = cr.plan(n_trees, n_taxa, n_rows, k, batch, reg, mats)
            assert sorted(got) == sorted(want)
            for key in want:
                assert np.array_equal(got[key], want[key]), (n_trees, n_taxa, n_rows, batch, reg, mats, key)


def test_the_variant_at_the_cap_and_one_past_it():
    words = lambda trees, reg=0: backend.debug_coverage_plan(trees, 100, reg_words=reg)  # noqa: E731
    assert [words(t)["variant"] for t in (1, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == \
        [4, 4, 8, 8, 16, 16, 32, 32, 64, 64]
    past = words(2049)
    assert past["words"] == 65 and past["variant"] == 0 and past["bits_stride"] == 65
    assert words(2048)["words"] == 64 and words(2048)["bits_stride"] == 64
    # the knob lowers the cap: 200 trees are 7 words, held in 8
    assert [words(200, reg)["variant"] for reg in (1, 4, 7, 8, 16, 64, 1000)] == [0, 0, 0, 8, 8, 8, 8]
    assert words(100, 4)["variant"] == 4 and words(100, 3)["variant"] == 0 and words(100, 3)["bits_stride"] == 4


def test_the_batches_their_bytes_and_their_grids():
    n = 10000
    none, both = (backend.debug_coverage_plan(500, n, matrices=m) for m in (0, 2))
    assert none["row_bytes"] == 8 and both["row_bytes"] == 8 + 8 * n
    assert none["fixed_bytes"] == both["fixed_bytes"] == none["bytes"][0] < 4 << 20  # nothing of rows x taxa
    assert both["bytes"][0] == both["fixed_bytes"] + 8 * n * n and both["n_batches"] == 1 and both["mirror"] == 1
    assert both["tiles"] == 157 and both["grid"].tolist() == [n * 157]
    # 20 000 taxa with both matrices: 3.2 GB of cells, more than a batch's 1.5 GB -- batches, and no mirror
    big = backend.debug_coverage_plan(2000, 20000, matrices=2)
    assert big["n_batches"] == 2 and big["mirror"] == 0 and big["rows"].sum() == 20000
    assert big["bytes"].max() - big["fixed_bytes"] <= cr.BUDGET
    assert backend.debug_coverage_plan(2000, 20000, matrices=0)["mirror"] == 1
    # the smallest n whose rows take more than 65 535 workgroups in one launch
    assert backend.debug_coverage_plan(8, 2047)["grid"].tolist() == [2047 * 32]
    assert backend.debug_coverage_plan(8, 2048)["grid"].tolist() == [65536]
    # a launch stays under the work-items a dispatch counts: 300 000 taxa are 4 688 tiles a row
    wide = backend.debug_coverage_plan(8, 300000)
    assert wide["grid_limit"] == (2**32 - 1) // 256 and wide["rows_per_launch"] == wide["grid_limit"] // 4688
    assert wide["grid"][0] == wide["rows_per_launch"] * 4688 and wide["grid"][0] * 256 <= 2**32 - 1


def test_the_plan_entry_refuses_what_it_cannot_plan():
    with pytest.raises(nv.ScsError, match="scs_debug_coverage_plan: negative argument"):
        backend.debug_coverage_plan(5, 10, reg_words=-1)
    with pytest.raises(nv.ScsError, match="scs_debug_coverage_plan: min_trees = 0 is less than 1"):
        backend.debug_coverage_plan(5, 10, min_trees=0)
    with pytest.raises(nv.ScsError, match="matrices_wanted = 3 is not 0, 1 or 2"):
        backend.debug_coverage_plan(5, 10, matrices=3)
    lib = nv.load_library()
    assert lib.scs_debug_coverage_plan(None, 1, None, 1, 1, 1, 0, 0, 0, None, None) == nv.EINVAL
    assert lib.scs_last_error() == b"scs_debug_coverage_plan: null argument"


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("symbol,count", [("scs_score_coverage", 11), ("scs_debug_coverage_plan", 11)])
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
    if symbol == "scs_score_coverage":
        assert params == ["scs_ctx *ctx", "const scs_tables *sources", "int32_t n_rows", "const int32_t *rows",
                          "int32_t min_trees", "int32_t max_batch_rows", "int32_t max_reg_words", "int32_t *occurs",
                          "int32_t *pair_trees", "int32_t *pair_covered", "int64_t *taxon_covered"]
        assert lib.scs_score_coverage(None, None, 0, None, 1, 0, 0, None, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_coverage: null argument"
    else:
        assert params[:4] == ["const scs_tables *sources", "int32_t n_trees", "const int64_t *tree_off",
                              "int32_t n_taxa"]
        assert params[4:] == ["int32_t n_rows", "int32_t min_trees", "int32_t max_batch_rows", "int32_t max_reg_words",
                              "int32_t matrices_wanted", "int64_t *info_out", "int64_t *batches_out"]


# ------------------------------------------------------------------------------------------------ the host layer
def _at(address: int, dtype, count: int) -> np.ndarray:
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


class FakeLib:
    """``scs_score_coverage`` records its arguments and answers occurs[x] = x + 1, cell [i][b] = 100 m + 10 taxon + b
    for matrix m and taxon_covered[i] = 1000 + taxon."""

    def __init__(self, n):
        self.n, self.calls, self.rc = n, [], 0

    def scs_last_error(self):
        return b"scs_score_coverage: rows[0] = 9 is not a taxon of the tables (4 taxa)"

    def scs_score_coverage(self, ctx, tabs, n_rows, rows, k, batch, reg, occurs, pt, pc, tc):
        ids = list(range(self.n)) if rows is None else _at(rows, np.int32, n_rows).tolist()
        self.calls.append((n_rows, None if rows is None else ids, k, batch, reg,
                           [o is not None for o in (occurs, pt, pc, tc)]))
        if occurs is not None:
            _at(occurs, np.int32, self.n)[:] = np.arange(self.n) + 1
        for m, o in enumerate((pt, pc)):
            if o is not None:
                _at(o, np.int32, n_rows * self.n)[:] = [100 * m + 10 * t + b for t in ids for b in range(self.n)]
        if tc is not None:
            _at(tc, np.int64, n_rows)[:] = [1000 + t for t in ids]
        return self.rc


def test_device_method_marshals_the_export():
    lib = FakeLib(4)
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3, n_taxa=4)
    got = dev.score_coverage(tabs)
    assert lib.calls == [(4, None, 1, 0, 0, [True, False, False, True])] and list(got) == list(cr.KEYS)
    assert got["occurs"].dtype == np.int32 and got["occurs"].tolist() == [1, 2, 3, 4]
    assert got["taxon_covered"].dtype == np.int64 and got["taxon_covered"].tolist() == [1000, 1001, 1002, 1003]
    assert got["pair_trees"] is None and got["pair_covered"] is None
    got = dev.score_coverage(tabs, rows=[2, 0, 2], min_trees=3, pairs=True, batch_rows=5, reg_words=8)
    assert lib.calls[-1] == (3, [2, 0, 2], 3, 5, 8, [True] * 4)
    assert got["pair_trees"].dtype == np.int32 and got["pair_trees"][:, 1].tolist() == [21, 1, 21]
    assert got["pair_covered"].shape == (3, 4) and got["pair_covered"][1].tolist() == [100, 101, 102, 103]
    got = dev.score_coverage(tabs, rows=[], pairs=True, outputs=())
    assert lib.calls[-1][-1] == [False, True, True, False] and got["pair_trees"].shape == (0, 4)
    assert got["occurs"] is None and got["taxon_covered"] is None
    with pytest.raises(ValueError, match="rows must be a list of taxon ids"):
        dev.score_coverage(tabs, rows=[[0, 1]])
    lib.rc = nv.EINVAL
    with pytest.raises(ValueError, match=r"rows\[0\] = 9 is not a taxon of the tables"):
        dev.score_coverage(tabs, rows=[9])


class FakeTables:
    def __init__(self, n_trees, n_taxa):
        self.n_trees, self.n_taxa, self.freed = n_trees, n_taxa, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload`` and ``score_coverage`` answered by the reference on the tables' own taxon sets, logged."""

    def __init__(self):
        self.log, self.tabs = [], None

    def upload(self, tables):
        self.tables = tables
        self.tabs = FakeTables(tables.n_trees, tables.n_taxa)
        return self.tabs

    def score_coverage(self, tabs, rows=None, min_trees=1, pairs=False, batch_rows=0, reg_words=0):
        self.log.append((None if rows is None else np.asarray(rows).tolist(), min_trees, pairs))
        off, leaf = self.tables.tree_off, self.tables.leaf_taxon
        sets = [leaf[off[t]:off[t + 1]].tolist() for t in range(len(off) - 1)]
        out = cr.by_sets(sets, self.tables.n_taxa, min_trees, rows)
        out.pop("covered", None)
        if not pairs:
            out["pair_trees"] = out["pair_covered"] = None
        return out


TREES = ["((a,b),c);", "(d,(b,(e,a)));", "(a,e);", "f;"]


def test_source_coverage_numbers_the_union_of_the_names_and_frees_the_tables():
    dev = FakeDevice()
    trees = [make_tree(t) for t in TREES]
    res = source_coverage(trees, device=dev)
    assert dev.log == [(None, 1, False)] and dev.tabs.freed == 1 and dev.tables.n_taxa == 6
    assert isinstance(res, SourceCoverage) and res.taxa == ["a", "b", "c", "d", "e", "f"]
    assert res.rows.tolist() == [0, 1, 2, 3, 4, 5] and res.min_trees == 1
    assert res.occurs.tolist() == [3, 2, 1, 1, 2, 1]
    # abc from tree 0; of {d, b, e, a} the four triples of tree 1
    assert res.taxon_covered.tolist() == [4, 4, 1, 3, 3, 0] and res.taxon_triples == 10
    assert res.triples_total == 20 and res.triples_covered == 5 and res.coverage == pytest.approx(0.25)
    assert res.decisive is False and res.pair_trees is None and res.pair_covered is None
    assert res.taxon_coverage.tolist() == pytest.approx([0.4, 0.4, 0.1, 0.3, 0.3, 0.0])
    assert set(res.timings) == {"prepare", "tables", "coverage"}
    with pytest.raises(ValueError, match="never_together needs the pair matrices"):
        res.never_together()
    assert res.table().splitlines() == ["taxon\toccurs\tcovered\ttriples\tcoverage", "a\t3\t4\t10\t0.4000",
                                        "b\t2\t4\t10\t0.4000", "c\t1\t1\t10\t0.1000", "d\t1\t3\t10\t0.3000",
                                        "e\t2\t3\t10\t0.3000", "f\t1\t0\t10\t0.0000"]
    worst = res.least_covered_taxa(3)
    assert [w["name"] for w in worst] == ["f", "c", "d"] and worst[1] == {
        "taxon": 2, "name": "c", "occurs": 1, "covered": 1, "coverage": pytest.approx(0.1)}
    assert [w["taxon"] for w in res.least_covered_taxa(min_occurs=2)] == [4, 0, 1] and res.least_covered_taxa(0) == []


def test_rows_by_name_or_id_the_matrices_and_min_trees():
    dev = FakeDevice()
    trees = [make_tree(t) for t in TREES]
    res = source_coverage(trees, min_trees=2, rows=["e", 0, "e"], pairs=True, device=dev)
    assert dev.log == [([4, 0, 4], 2, True)] and res.rows.tolist() == [4, 0, 4] and res.min_trees == 2
    assert res.triples_total is None and res.triples_covered is None and res.coverage is None and res.decisive is None
    assert res.pair_trees.tolist() == [[2, 1, 0, 1, 2, 0], [3, 2, 1, 1, 2, 0], [2, 1, 0, 1, 2, 0]]
    assert not res.pair_covered.any() and res.taxon_covered.tolist() == [0, 0, 0]
    assert res.never_together() == [(0, 5), (2, 4), (4, 5)]
    assert [w["taxon"] for w in res.least_covered_taxa()] == [0, 4]
    assert len(res.table().splitlines()) == 4
    for rows, bad in ((["x"], "'x'"), ([6], "6"), ([-1], "-1")):
        with pytest.raises(ValueError, match=f"rows must be names or ids of the 6 taxa of the sources, not {bad}"):
            source_coverage(trees, rows=rows, device=dev)
    with pytest.raises(ValueError, match="min_trees = 0 is less than 1"):
        source_coverage(trees, min_trees=0, device=dev)
    with pytest.raises(ValueError, match="at least one tree"):
        source_coverage([], device=dev)
    full = source_coverage([make_tree("((a,b),(c,d));")] * 2, min_trees=2, device=dev)
    assert full.decisive is True and full.coverage == 1.0 and full.triples_covered == 4
    two = source_coverage([make_tree("(a,b);")], device=dev)
    assert two.taxon_triples == 0 and np.isnan(two.taxon_coverage).all() and math.isnan(two.coverage)
    assert two.decisive is True and two.table().splitlines()[1] == "a\t1\t0\t0\tnan"


def test_the_one_leaf_trees_of_tree_arrays_are_added_on_the_host(monkeypatch):
    # as TreeArrays the trees of fewer than two leaves have no tables: the answer must be the list's all the same
    dev = FakeDevice()
    trees = [make_tree(t) for t in [*TREES, "b;", "f;"]]
    names = sorted({n for t in trees for n in t.get_tip_names()})
    arrays = TreeArrays.from_trees(trees, [1.0] * len(trees), names)
    want = source_coverage(trees, pairs=True, device=dev)
    seen = {}

    class Resident:
        def __init__(self, device, given, tips, index):
            seen["tips"], seen["index"] = tips, index

        def __enter__(self):
            from spectralclustersupertree_amd.flatten import flatten_trees

            kept = [t for t in trees if len(t.get_tip_names()) >= 2]
            dev.upload(flatten_trees(kept, [1.0] * len(kept), "one", taxa=seen["tips"]))
            return types.SimpleNamespace(dev=dev, tabs=dev.tabs, n_leaves=arrays.leaf_counts(), seconds=0.0)

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    got = source_coverage(arrays, pairs=True, device=dev)
    assert got.taxa == names == seen["tips"] and dev.tables.n_trees == 3
    assert got.occurs.tolist() == [3, 3, 1, 1, 2, 2]  # f only in one-leaf trees, b in one of them
    at = {n: i for i, n in enumerate(want.taxa)}
    order = [at[n] for n in names]
    assert np.array_equal(got.occurs, want.occurs[order])
    assert np.array_equal(got.pair_trees, want.pair_trees[np.ix_(order, order)])
    assert np.array_equal(got.pair_covered, want.pair_covered[np.ix_(order, order)])
    assert np.array_equal(got.taxon_covered, want.taxon_covered[order]) and got.triples_covered == want.triples_covered
    # rows by name reach the diagonal too
    sub = source_coverage(arrays, rows=["f", "b"], pairs=True, device=dev)
    assert sub.pair_trees[0, 5] == 2 and sub.pair_trees[1, 1] == 3 and sub.pair_trees[1, 5] == 0


def test_without_tables_the_occurrences_are_the_one_leaf_trees(monkeypatch):
    trees = [make_tree("a;"), make_tree("b;"), make_tree("a;")]
    arrays = TreeArrays.from_trees(trees, [1.0] * 3, ["a", "b"])

    class Resident:
        def __init__(self, *a):
            pass

        def __enter__(self):
            return types.SimpleNamespace(dev=None, tabs=None, n_leaves=np.array([1, 1, 1]), seconds=0.0)

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(score_mod, "_resident_tables", Resident)
    res = source_coverage(arrays, pairs=True)
    assert res.occurs.tolist() == [2, 1] and res.pair_trees.tolist() == [[2, 0], [0, 1]] and not res.pair_covered.any()
    assert res.taxon_covered.tolist() == [0, 0] and res.triples_total == 0 and res.never_together() == [(0, 1)]


def test_the_command_line_writes_the_table(monkeypatch, tmp_path):
    calls = []

    def fake_coverage(trees, min_trees=1, rows=None, pairs=False, device=None):
        calls.append((type(trees).__name__, min_trees, rows, pairs))
        return SourceCoverage(taxa=["a", "b", "c"], rows=np.arange(3), min_trees=min_trees,
                              occurs=np.array([2, 1, 1], dtype=np.int32), taxon_covered=np.array([1, 1, 1]),
                              taxon_triples=1, triples_total=1, triples_covered=1)

    import spectralclustersupertree_amd as pkg

    monkeypatch.setattr(score_mod, "source_coverage", fake_coverage)
    monkeypatch.setattr(pkg, "construct_supertree", lambda sources, **kw: make_tree("((a,b),c);"))
    src, out, cov = tmp_path / "in.tre", tmp_path / "out.tre", tmp_path / "coverage.tsv"
    src.write_text("((a,b),c);\n(a,c);\n")
    res = CliRunner().invoke(cli_mod.scs, ["-i", str(src), "-o", str(out), "--coverage-out", str(cov)])
    assert res.exit_code == 0, res.output
    assert calls == [("TreeArrays", 1, None, False)]
    assert cov.read_text().splitlines() == ["taxon\toccurs\tcovered\ttriples\tcoverage", "a\t2\t1\t1\t1.0000",
                                            "b\t1\t1\t1\t1.0000", "c\t1\t1\t1\t1.0000"]
    res = CliRunner().invoke(cli_mod.scs, ["-i", str(src), "-o", str(out), "--coverage-out", str(cov),
                                           "--coverage-min-trees", "2"])
    assert res.exit_code == 0 and calls[-1][1] == 2
    res = CliRunner().invoke(cli_mod.scs, ["-i", str(src), "-o", str(out), "--coverage-out", str(cov),
                                           "--coverage-min-trees", "0"])
    assert res.exit_code != 0 and len(calls) == 2
    res = CliRunner().invoke(cli_mod.scs, ["-i", str(src), "-o", str(out)])
    assert res.exit_code == 0 and len(calls) == 2  # the option is the only way in
