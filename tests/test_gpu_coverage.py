"""The triple coverage of the sources on the device (``scs_score_coverage``) held exactly to the
references of ``tests/coverage_reference.py``, every case at ``min_trees`` 1, 2 and 3, with the matrices and without,
and with the outputs null in turn: tiny hand-made sources, taxa counts around a wave and a tile, tree counts around a
word, every register variant and the streaming kernel, chosen rows and row batches, sparse sources that skip most
pairs, a grid past 65 535 workgroups, the refusals, and the way through ``source_coverage`` and the command line."""

import random
from functools import lru_cache
from pathlib import Path

import coverage_reference as cr
import numpy as np
import pytest
from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, load_trees, source_coverage, synthetic
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.load import load_tree_arrays

pytestmark = pytest.mark.gpu

DATA = Path(__file__).parent / "golden" / "reference_data"
KS = (1, 2, 3)


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what) -> None:
    for k in cr.KEYS:
        if got[k] is None:
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (what, k, bad[:6].tolist(), got[k][got[k] != ref[k]][:6], ref[k][got[k] != ref[k]][:6])


def _reference(sets, n, k, rows=None) -> dict:
    return cr.by_sets(sets, n, k, rows) if n <= 24 else cr.by_matmul(sets, n, k, rows)


def _check(dev, sets, n, rows=None, ks=KS, batches=(0,), regs=(0,), what="") -> dict:
    """Every setting against the reference, per k: the matrices on and off, the outputs null in turn; the invariants
    and, from one k to the next, that the counts do not grow.  Returns the device's answer per k."""
    tabs = dev.upload(cr.tables(sets, n))
    out, last = {}, None
    try:
        for k in ks:
            ref = _reference(sets, n, k, rows)
            assert int(ref["occurs"].sum()) == sum(len(s) for s in sets)  # the tables' leaves
            for batch in batches:
                for reg in regs:
                    at = (what, k, batch, reg)
                    full = dev.score_coverage(tabs, rows, k, True, batch, reg)
                    _same(full, ref, at)
                    assert all(full[key] is not None for key in cr.KEYS)
                    cr.check_invariants(full, n, k, rows)
                    lean = dev.score_coverage(tabs, rows, k, False, batch, reg)
                    assert lean["pair_trees"] is None and lean["pair_covered"] is None
                    _same(lean, ref, (*at, "no matrices"))
            for names in ((), ("occurs",), ("taxon_covered",)):
                for pairs in (False, True):
                    part = dev.score_coverage(tabs, rows, k, pairs, outputs=names)
                    assert [key for key in cr.KEYS if part[key] is not None] == \
                        [key for key in cr.KEYS if key in names or (pairs and key.startswith("pair_"))]
                    _same(part, ref, (what, k, names, pairs))
            if last is not None:
                cr.check_monotone(last, full)
            out[k] = last = full
    finally:
        tabs.free()
    return out


# ------------------------------------------------------------------------------------------------ tiny cases by sets
def test_taxa_in_no_one_and_all_trees_and_trees_of_one_two_and_three_leaves(dev):
    # taxon 0 in every tree, 9 in one, 10 in none; trees of one, two and three leaves beside larger ones
    sets = [[0, 1, 2, 3, 4], [0], [0, 5], [0, 1, 6], [0, 2, 3, 7, 8, 9], [4, 0, 1, 2], [0, 3]]
    got = _check(dev, sets, 11, batches=(0, 1, 3))
    assert got[1]["occurs"].tolist() == [7, 3, 3, 3, 2, 1, 1, 1, 1, 1, 0]
    assert not got[1]["pair_trees"][10].any() and not got[1]["pair_covered"][:, 10].any()
    assert got[1]["pair_covered"][0, 9] == 4 and got[2]["pair_covered"][0, 9] == 0  # 2, 3, 7, 8 beside them, once
    # {0, 1, 2, 4} in two trees: 0 and 4 beside the pair (1, 2); {0, 2, 3} in two as well
    assert got[2]["pair_covered"][1, 2] == 2 and got[2]["taxon_covered"].tolist() == [4, 3, 4, 1, 3, 0, 0, 0, 0, 0, 0]
    assert got[3]["taxon_covered"].sum() == 0 and (got[3]["pair_trees"] >= 3).sum() > 1


def test_disjoint_trees_cover_nothing_across_them_and_identical_trees_everything(dev):
    got = _check(dev, [[0, 1, 2, 3], [4, 5, 6], [7, 8]], 9)
    assert got[1]["taxon_covered"].tolist() == [3, 3, 3, 3, 1, 1, 1, 0, 0] and not got[2]["taxon_covered"].any()
    assert not got[1]["pair_trees"][:4, 4:].any()
    got = _check(dev, [list(range(7))] * 3, 7)
    for k in KS:  # decisive: every one of the C(7, 3) triples, whichever k up to the three trees
        assert got[k]["taxon_covered"].tolist() == [15] * 7 and (got[k]["pair_covered"] + 5 * np.eye(7, dtype=int) == 5).all()
    # disjoint pairs of trees: coverage 0
    got = _check(dev, [[0, 1], [2, 3], [4, 5]], 6)
    assert not got[1]["pair_covered"].any() and got[1]["pair_trees"].sum() == 12


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_two_and_three_taxa(dev, n):
    got = _check(dev, [list(range(n))] * 2 + [[0]], n, batches=(0, 1))
    assert got[2]["taxon_covered"].tolist() == [int(n == 3)] * n and got[3]["taxon_covered"].sum() == 0
    assert got[1]["occurs"].tolist() == [3, 2, 2][:n]


# ------------------------------------------------------------------------------------------------ lanes and waves
@pytest.mark.parametrize("n", [63, 64, 65, 127, 129, 255, 257])
def test_taxa_counts_around_a_wave_and_a_tile(dev, n):
    rng = random.Random(n)
    sets = cr.random_sets(rng, n, 20, 3, n // 2)
    sets.append([n - 1, n - 2, 0])  # the last lanes of the last tile with the first
    got = _check(dev, sets, n)
    assert got[1]["pair_covered"][n - 1].any() and 0 < got[2]["taxon_covered"].sum() < got[1]["taxon_covered"].sum()


# ------------------------------------------------------------------------------------------------ words
@pytest.mark.parametrize("n_trees", [31, 32, 33, 63, 64, 65, 129])
@pytest.mark.parametrize("n", [40, 70])
def test_tree_counts_around_a_word(dev, n_trees, n):
    rng = random.Random(100 * n_trees + n)
    sets = cr.random_sets(rng, n - 3, n_trees, 2, 12)  # (the last three taxa are placed by hand)
    sets[-1] = sorted({*sets[-1], n - 1, 0, 1})        # taxon n - 1 only in the last tree
    if n_trees > 32:
        sets[31] = sorted({*sets[31], n - 2, 2, 3})    # n - 2 only in tree 31, the last bit of word 0
        sets[32] = sorted({*sets[32], n - 3, 2, 3})    # n - 3 only in tree 32, the first bit of word 1
    got = _check(dev, sets, n)
    assert got[1]["occurs"][n - 1] == 1 and got[1]["pair_covered"][n - 1, 0] >= 1
    if n_trees > 32:
        assert got[1]["occurs"][n - 2] == got[1]["occurs"][n - 3] == 1 and got[1]["pair_trees"][n - 2, n - 3] == 0
        assert got[1]["pair_covered"][n - 2, 2] >= 1 and got[1]["pair_covered"][n - 3, 3] >= 1


# ------------------------------------------------------------------------------------------------ variants
def test_every_cap_on_one_input_gives_the_same_arrays(dev):
    # 200 trees are 7 words: the streaming kernel under a cap of 1 and 4, eight registers from 8 on
    rng = random.Random(8)
    n, sets = 300, cr.random_sets(random.Random(8), 300, 200, 4, 40)
    plans = [backend.debug_coverage_plan(200, n, reg_words=reg)["variant"] for reg in (1, 4, 8, 16, 0)]
    assert plans == [0, 0, 8, 8, 8]
    _check(dev, sets, n, regs=(1, 4, 8, 16, 0))
    rows = rng.sample(range(n), 9)
    _check(dev, sets, n, rows=rows, ks=(2,), regs=(1, 0), batches=(0, 4))


@pytest.mark.parametrize("n_trees,variant", [(100, 4), (250, 8), (400, 16), (900, 32), (1500, 64), (2048, 64)])
def test_every_register_variant_and_the_same_input_streamed(dev, n_trees, variant):
    rng = random.Random(n_trees)
    n = 70
    sets = cr.random_sets(rng, n, n_trees, 2, 9)
    sets[-1] = sorted({*sets[-1], 0, 1, n - 1})
    assert backend.debug_coverage_plan(n_trees, n)["variant"] == variant
    assert backend.debug_coverage_plan(n_trees, n, reg_words=variant // 2)["variant"] == 0
    _check(dev, sets, n, regs=(0, variant // 2))
    _check(dev, sets, n, rows=[n - 1, 3, 3], ks=(1, 2), regs=(0, variant // 2))


def test_more_trees_than_the_registers_hold(dev):
    # 2 100 trees are 66 words, past the 64 a lane holds: the streaming kernel without the knob
    rng = random.Random(21)
    n, n_trees = 80, 2100
    sets = cr.random_sets(rng, n, n_trees, 2, 7)
    sets[-1] = sorted({*sets[-1], 0, 1, n - 1})
    plan = backend.debug_coverage_plan(n_trees, n)
    assert plan["words"] == 66 and plan["variant"] == 0
    got = _check(dev, sets, n, batches=(0, 7))
    assert got[3]["taxon_covered"].sum() > 0


# ------------------------------------------------------------------------------------------------ rows and batches
def test_chosen_repeated_and_no_rows_and_row_batches(dev):
    rng = random.Random(5)
    n = 150
    sets = cr.random_sets(rng, n, 45, 3, 50)
    full = _check(dev, sets, n, batches=(1, 3, 0), ks=(1, 2))  # rows None: the mirror path unless batched matrices
    explicit = _check(dev, sets, n, rows=list(range(n)), batches=(0, 64), ks=(1, 2))
    for k in (1, 2):
        _same(explicit[k], full[k], ("mirror against range(n)", k))
    _check(dev, sets, n, rows=[149, 0, 77, 0, 149, 149, 64, 63], batches=(0, 1, 3))
    empty = _check(dev, sets, n, rows=[], ks=(1,), batches=(0, 2))
    assert empty[1]["pair_trees"].shape == (0, n) and empty[1]["occurs"].sum() == sum(len(s) for s in sets)
    # what the plan says of the two ways to ask for every row
    assert backend.debug_coverage_plan(45, n, matrices=2)["mirror"] == 1
    assert backend.debug_coverage_plan(45, n, batch_rows=3, matrices=2)["mirror"] == 0
    assert backend.debug_coverage_plan(45, n, batch_rows=3, matrices=0)["mirror"] == 1
    assert backend.debug_coverage_plan(45, n, n_rows=n, matrices=2)["mirror"] == 0


# ------------------------------------------------------------------------------------------------ skips
def test_sparse_sources_skip_most_pairs_and_taxa(dev):
    # 40 trees of 12 leaves over 300 taxa: most pairs never co-occur, and at k = 3 most taxa are in too few trees
    rng = random.Random(40)
    n = 300
    core = rng.sample(range(n), 20)
    sets = [rng.sample(core, 6) + rng.sample([x for x in range(n) if x not in core], 6) for _ in range(40)]
    got = _check(dev, sets, n, batches=(0, 50))
    assert (got[1]["pair_trees"] == 0).mean() > 0.9 and (got[1]["occurs"] < 3).mean() > 0.5
    assert 0 < got[3]["taxon_covered"].sum() < got[2]["taxon_covered"].sum() < got[1]["taxon_covered"].sum()


# ------------------------------------------------------------------------------------------------ a large grid
@lru_cache(maxsize=None)
def _wide():
    rng = random.Random(65)
    n = 2048
    sets = [rng.sample(range(n), rng.randint(300, 900)) for _ in range(6)] + [[0, 1, n - 1], [n - 1, n - 2, 5]]
    rows = sorted({0, 1, 5, 63, 64, 1000, n - 2, n - 1, *rng.sample(range(n), 8)})
    return n, sets, rows, {k: cr.by_matmul(sets, n, k, rows) for k in KS}


def test_a_grid_past_65535_workgroups(dev):
    n, sets, rows, refs = _wide()
    # the smallest n whose rows are more than 65 535 workgroups of one launch
    assert backend.debug_coverage_plan(len(sets), n, matrices=2)["grid"].tolist() == [65536]
    assert backend.debug_coverage_plan(len(sets), n - 1, matrices=2)["grid"].tolist() == [(n - 1) * 32]
    tabs = dev.upload(cr.tables(sets, n))
    try:
        last = None
        for k in KS:
            full = dev.score_coverage(tabs, None, k, True)
            cr.check_invariants(full, n, k)
            _same({key: full[key] if key == "occurs" else full[key][rows] for key in cr.KEYS}, refs[k], ("wide", k))
            _same(dev.score_coverage(tabs, None, k, False), {**full, "pair_trees": None, "pair_covered": None}, k)
            _same(dev.score_coverage(tabs, rows, k, True), refs[k], ("wide rows", k))
            if last is not None:
                cr.check_monotone(last, full)
            last = full
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_messages(dev):
    sets = [[0, 1, 2], [1, 2, 3], [0, 3]]
    tabs = dev.upload(cr.tables(sets, 4))
    twice = dev.upload(cr.tables([[0, 1, 2], [0, 1, 0]], 4))
    who = "scs_score_coverage: "
    try:
        for rows, said in (([4], r"rows\[0\] = 4 is not a taxon of the tables \(4 taxa\)"),
                           ([0, -1], r"rows\[1\] = -1 is not a taxon")):
            with pytest.raises(ValueError, match=who + said):
                dev.score_coverage(tabs, rows=rows)
        for kwargs, said in (({"min_trees": 0}, "min_trees = 0 is less than 1"),
                             ({"min_trees": -2}, "min_trees = -2 is less than 1"),
                             ({"batch_rows": -1}, "max_batch_rows = -1 is negative"),
                             ({"reg_words": -1}, "max_reg_words = -1 is negative")):
            with pytest.raises(ValueError, match=who + said):
                dev.score_coverage(tabs, **kwargs)
        lib, buf = dev._lib, np.zeros(4, dtype=np.int32)
        rows = np.zeros(3, dtype=np.int32)
        for n_rows, row_ptr, said in ((-1, rows.ctypes.data, b"n_rows = -1 is negative"),
                                      (2, None, b"rows is null and n_rows = 2 is not the 4 taxa of the tables")):
            assert lib.scs_score_coverage(dev._ctx, tabs._h, n_rows, row_ptr, 1, 0, 0, buf.ctypes.data, None, None,
                                          None) == nv.EINVAL
            assert lib.scs_last_error() == who.encode() + said
        for ctx, handle in ((dev._ctx, None), (None, tabs._h)):
            assert lib.scs_score_coverage(ctx, handle, 0, None, 1, 0, 0, None, None, None, None) == nv.EINVAL
            assert lib.scs_last_error() == b"scs_score_coverage: null argument"
        # a taxon twice in a tree: found on the device before a triple is counted, whichever rows are asked for
        for rows in (None, [0], []):
            with pytest.raises(ValueError, match="^scs_score_coverage: a source tree has a taxon twice$"):
                dev.score_coverage(twice, rows=rows, pairs=True)
        # a taxon out of range: the upload refuses it with the words the exports use ...
        with pytest.raises(ValueError, match=r"a leaf_taxon entry is out of range \[0, n_taxa\)"):
            dev.upload(cr.tables([[0, 1, 4]], 4))
        # ... and the context is as usable as before: a good call gives the right numbers
        for k in KS:
            _same(dev.score_coverage(tabs, None, k, True), cr.by_sets(sets, 4, k), ("after", k))
    finally:
        tabs.free()
        twice.free()


def test_a_taxon_out_of_range_in_a_late_chunk_is_found_on_the_device(dev):
    # page-locked tables of this size return from the upload after their first 64 trees; the device's range check of
    # the rest is collected by the first export that reads them all -- before any sweep kernel runs
    n, m = 2100, 288
    bad = synthetic.make_tables(0, n, m, "one", pinned=True)
    bad.leaf_taxon[-5] = n + 3
    dtab = dev.upload(bad)
    try:
        with pytest.raises(ValueError, match=r"a leaf_taxon entry is out of range \[0, n_taxa\)"):
            dev.score_coverage(dtab, rows=[0])
    finally:
        dtab.free()
    sets = [[0, 1, 2], [1, 2, 3], [0, 3]]
    tabs = dev.upload(cr.tables(sets, 4))
    try:
        _same(dev.score_coverage(tabs, None, 1, True), cr.by_sets(sets, 4, 1), "after")
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ API and CLI
@lru_cache(maxsize=None)
def _dcm():
    trees = load_trees(str(DATA / "dcm_source_trees.tre"))
    names: dict = {}
    for t in trees:
        for name in t.get_tip_names():
            names.setdefault(name, len(names))
    sets = [[names[x] for x in t.get_tip_names()] for t in trees]
    return trees, list(names), sets


@pytest.mark.parametrize("k", [1, 2])
def test_source_coverage_on_the_dcm_sources_as_trees_and_as_arrays(dev, k):
    trees, names, sets = _dcm()
    n = len(names)
    ref = cr.by_matmul(sets, n, k)
    res = source_coverage(trees, min_trees=k, pairs=True, device=dev)
    assert res.taxa == names and res.rows.tolist() == list(range(n)) and "coverage" in res.timings
    _same({key: getattr(res, key) for key in cr.KEYS}, ref, "dcm trees")
    cr.check_invariants({key: getattr(res, key) for key in cr.KEYS}, n, k)
    assert res.triples_covered == ref["covered"] and res.triples_total == n * (n - 1) * (n - 2) // 6
    assert 0 < res.coverage < 1 and res.decisive is False and res.coverage == ref["covered"] / res.triples_total
    arrays = source_coverage(load_tree_arrays(str(DATA / "dcm_source_trees.tre")), min_trees=k, pairs=True, device=dev)
    # (a TreeArrays numbers its taxa by name, the list by first appearance: the same numbers under that renaming)
    assert sorted(arrays.taxa) == sorted(names) and arrays.taxa != names
    order = [arrays.taxa.index(x) for x in names]
    _same({"occurs": arrays.occurs[order], "pair_trees": arrays.pair_trees[np.ix_(order, order)],
           "pair_covered": arrays.pair_covered[np.ix_(order, order)], "taxon_covered": arrays.taxon_covered[order]},
          ref, "dcm arrays")
    assert arrays.triples_covered == res.triples_covered and sorted(arrays.table().splitlines()) == sorted(
        res.table().splitlines())
    lean = source_coverage(trees, min_trees=k, device=dev)
    assert lean.pair_trees is None and np.array_equal(lean.taxon_covered, ref["taxon_covered"])
    rows = [names[700], 3, names[0]]
    part = source_coverage(trees, min_trees=k, rows=rows, pairs=True, device=dev)
    ids = [700, 3, 0]
    _same({key: getattr(part, key) for key in cr.KEYS}, {key: ref[key] if key == "occurs" else ref[key][ids]
                                                          for key in cr.KEYS}, "dcm rows")
    worst = res.least_covered_taxa(5)
    assert [w["covered"] for w in worst] == sorted(ref["taxon_covered"].tolist())[:5]
    together = res.never_together()
    assert len(together) == int((ref["pair_trees"][np.triu_indices(n, 1)] == 0).sum()) > 0
    assert together[0][0] < together[0][1] and ref["pair_trees"][together[0]] == 0 == ref["pair_trees"][together[-1]]


def test_the_command_line_writes_the_coverage_table(tmp_path):
    src = DATA / "supertriplets_source.tre"
    out, cov, two, other = (tmp_path / x for x in ("out.tre", "coverage.tsv", "two.tsv", "other.tre"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--coverage-out", str(cov)])
    assert res.exit_code == 0, res.output
    api = source_coverage(load_tree_arrays(str(src)))
    assert cov.read_text() == api.table() and len(cov.read_text().splitlines()) == 1 + len(api.taxa)
    assert cov.read_text().splitlines()[0].split("\t") == ["taxon", "occurs", "covered", "triples", "coverage"]
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--coverage-out", str(two),
                                   "--coverage-min-trees", "40"])
    assert res.exit_code == 0, res.output
    assert two.read_text() == source_coverage(load_tree_arrays(str(src)), min_trees=40).table() != api.table()
    # without the option: the files of before and no other
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(other)])
    assert res.exit_code == 0 and sorted(p.name for p in tmp_path.iterdir()) == ["coverage.tsv", "other.tre", "out.tre",
                                                                                 "two.tsv"]
