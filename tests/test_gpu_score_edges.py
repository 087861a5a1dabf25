"""The four base scoring exports on the device -- ``scs_score_supertree``, ``scs_score_triplets``,
``scs_score_conflicts``, ``scs_score_concordance`` -- at the sizes where ``csrc/scs_score.hip`` changes path
(DESIGN.md section 29): tree boundaries inside waves, table levels around powers of two, the 1 024-wide steps of the
compaction and the prefix pass, the 256-wide steps of the conflict scan, the galloping searches, the ``zb``
transitions of the pair kernel, dynamic LDS above 64 KiB up to the advertised limit, the byte budget splitting a
batch, and the refusals in a later batch.  The cases and their references come from ``tests/score_edge_reference.py``
(``tests/test_score_edge_reference_cpu.py`` holds every case to the numbers it is named for); every comparison is
``np.array_equal`` on int64."""

from functools import lru_cache

import numpy as np
import pytest
import score_edge_reference as se

from spectralclustersupertree_amd import backend
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.flatten import TreeTables

pytestmark = pytest.mark.gpu

ALL = tuple(se.EXPORTS)
NO_CONCORDANCE = ("score", "score_triplets", "score_conflicts")
C_NAME = {"score": "scs_score_supertree", "score_triplets": "scs_score_triplets",
          "score_conflicts": "scs_score_conflicts", "score_concordance": "scs_score_concordance"}


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d
        d.trim(0)  # (the byte-budget cases took 1.6 GB of the arena)


def _same(res: dict, ref: dict, export: str, what) -> None:
    for k in se.EXPORTS[export]:
        got = res[k]
        assert got.dtype == np.int64 and got.shape == ref[k].shape, (what, export, k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (what, export, k, np.flatnonzero(got != ref[k])[:8],
                                             got[got != ref[k]][:8], ref[k][got != ref[k]][:8])


def _check(dev, parent, taxon, tables, ref, exports=ALL, batches=(0,), what="") -> None:
    tabs = dev.upload(tables) if isinstance(tables, TreeTables) else tables
    try:
        for bt in batches:
            for export in exports:
                _same(getattr(dev, export)(tabs, parent, taxon, bt), ref, export, (what, bt))
    finally:
        if tabs is not tables:
            tabs.free()


def _check_case(dev, case: se.Case, exports=ALL) -> None:
    ref = se.reference(case.parent, case.taxon, case.arrays, exports)
    _check(dev, case.parent, case.taxon, case.tables(), ref, exports, case.batches, case.name)


# ------------------------------------------------------------------------------------------------ waves
@pytest.mark.parametrize("end", se.WAVE_ENDS)
def test_tree_boundaries_inside_waves(dev, end):
    case = se.wave_case(end)
    m = case.arrays.n_trees
    tabs = dev.upload(case.tables())
    try:
        counts = [len(backend.debug_score_plan(tabs, case.s_leaves, bt)["bstart"]) - 1 for bt in case.batches]
        assert counts == [1, m, (m + 1) // 2, 2, 1, 1]
        ref = se.reference(case.parent, case.taxon, case.arrays)
        assert all(ref[k].any() for k in ("shared", "t_shared", "n_super_conflict", "informative", "conflicting"))
        _check(dev, case.parent, case.taxon, tabs, ref, ALL, case.batches, case.name)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("among", [False, True], ids=["alone", "among"])
@pytest.mark.parametrize("kind", se.LEVEL_SHAPES)
@pytest.mark.parametrize("size", se.LEVEL_SIZES)
def test_largest_tree_around_a_power_of_two(dev, size, kind, among):
    _check_case(dev, se.level_case(size, kind, among))


@pytest.mark.parametrize("kind", ["star", "caterpillar", "mixed"])
@pytest.mark.parametrize("gaps", se.S_GAPS)
def test_supertree_gaps_around_a_power_of_two(dev, gaps, kind):
    _check_case(dev, se.s_gap_case(gaps, kind))


# ------------------------------------------------------------------------------------------------ compaction, prefix
@pytest.mark.parametrize("what", ["leaves", "nodes"])
@pytest.mark.parametrize("count", se.CHUNK_COUNTS)
def test_supertree_leaves_and_nodes_around_the_1024_steps(dev, count, what):
    case = se.chunk_case(count, what)
    ref = se.reference(case.parent, case.taxon, case.arrays)
    if count > 1000:
        assert ref["informative"].any() and ref["supported"].any()
    _check(dev, case.parent, case.taxon, case.tables(), ref, ALL, (0, 1), case.name)


# ------------------------------------------------------------------------------------------------ conflicts
@pytest.mark.parametrize("size", se.SCAN_SIZES)
def test_trees_around_the_256_steps_of_the_conflict_scan(dev, size):
    case = se.scan_case(size)
    ref = se.reference(case.parent, case.taxon, case.arrays)
    assert ref["n_super_conflict"].all() and ref["n_source_conflict"].all()
    _check(dev, case.parent, case.taxon, case.tables(), ref, ALL, (0, 1), case.name)


@pytest.mark.parametrize("star_is", ["source", "super"])
@pytest.mark.parametrize("at", se.GALLOP_AT)
def test_galloping_searches_at_every_distance(dev, at, star_is):
    _check_case(dev, se.gallop_case(at, star_is))


# ------------------------------------------------------------------------------------------------ concordance
def test_concordance_situations(dev):
    case = se.concordance_case()
    ref = se.reference(case.parent, case.taxon, case.arrays)
    assert all(ref[k].any() for k in se.CONCORDANCE)
    _check(dev, case.parent, case.taxon, case.tables(), ref, ALL, case.batches, case.name)


# ------------------------------------------------------------------------------------------------ zb transitions
def _alone(case: se.Case, ref: dict, exports) -> tuple:
    """The case's large tree alone and its reference: its own per-tree entries, and per node what is left of the
    whole forest's counts without the small trees'."""
    at = case.note["large"]
    rest = [t for t in range(case.arrays.n_trees) if t != at]
    small = se.reference(case.parent, case.taxon, se.subset(case.arrays, rest), exports)
    one = {k: (ref[k] - small[k] if k in se.PER_NODE else ref[k][at:at + 1]) for e in exports for k in se.EXPORTS[e]}
    return se.subset(case.arrays, [at]).flatten("one"), one


@lru_cache(maxsize=None)
def _zb_quadratic(size: int):
    case = se.zb_quadratic_case(size)
    return case, se.reference(case.parent, case.taxon, case.arrays, NO_CONCORDANCE)


@pytest.mark.parametrize(("size", "zb"), list(zip(se.ZB_QUADRATIC, (8, 7))))
def test_zb_8_to_7_against_the_quadratic_references(dev, size, zb):
    case, ref = _zb_quadratic(size)
    assert 0 < ref["t_shared"][3] < ref["t_super"][3] < ref["t_source"][3]
    tabs = dev.upload(case.tables())
    try:
        plan = backend.debug_score_plan(tabs, case.s_leaves, 0, 32, 8)
        assert plan["zb"].tolist() == [zb] and plan["words"].tolist() == [(size >> 5) + 1]
        _check(dev, case.parent, case.taxon, tabs, ref, NO_CONCORDANCE, (0,), case.name)
    finally:
        tabs.free()
    tables, one = _alone(case, ref, NO_CONCORDANCE)
    _check(dev, case.parent, case.taxon, tables, one, NO_CONCORDANCE, (0,), case.name + " alone")


@pytest.mark.parametrize(("size", "zb"), list(zip(se.ZB_COMB, (2, 1))))
@pytest.mark.parametrize("with_small", [False, True], ids=["alone", "batch"])
def test_zb_2_to_1_against_the_closed_forms(dev, size, zb, with_small):
    case = se.comb_case(size, "random", with_small)
    ref = se.comb_case_reference(case)
    tabs = dev.upload(case.tables())
    try:
        plan = backend.debug_score_plan(tabs, case.s_leaves, 0, 32, 8)
        assert plan["zb"].tolist() == [zb] and plan["words"].tolist() == [(size >> 5) + 1]
        _check(dev, case.parent, case.taxon, tabs, ref, NO_CONCORDANCE, (0,), case.name)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ LDS above 64 KiB
@pytest.mark.parametrize(("size", "kind"), list(zip(se.LDS_COMB, ("interleave", "random", "blocks"))))
def test_dynamic_lds_up_to_the_limit(dev, size, kind):
    case = se.comb_case(size, kind)
    ref = se.comb_case_reference(case)
    assert 0 < ref["t_shared"][0] < ref["t_super"][0]
    tabs = dev.upload(case.tables())
    try:
        plan = backend.debug_score_plan(tabs, case.s_leaves, 0, 32, 8)
        assert plan["zb"].tolist() == [1] and plan["workgroups"].tolist() == [size - 2]
        assert (16 * int(plan["words"][0]) > 64 * 1024) == (size >= 131072)
        _check(dev, case.parent, case.taxon, tabs, ref, NO_CONCORDANCE, (0,), case.name)
    finally:
        tabs.free()


def test_a_tree_above_the_lds_limit_is_refused(dev):
    n = se.LDS_CAP + 1
    tables = TreeTables(n_taxa=n, tree_off=np.array([0, n], dtype=np.int64), leaf_taxon=np.arange(n, dtype=np.int32),
                        adj_depth=np.zeros(n, dtype=np.int32), adj_val=np.zeros(n, dtype=np.float64),
                        tree_w=np.ones(1, dtype=np.float64))
    parent = np.concatenate([[-1], np.zeros(n, dtype=np.int32)]).astype(np.int32)
    taxon = np.concatenate([[-1], np.arange(n, dtype=np.int32)]).astype(np.int32)
    tabs = dev.upload(tables)
    try:
        with pytest.raises(ValueError, match=rf"{n} leaves is more than the {se.LDS_CAP} the pair kernel holds in LDS"):
            dev.score_triplets(tabs, parent, taxon)
        assert dev.score(tabs, parent, taxon)["n_super"].tolist() == [0]  # (the RF call has no such limit)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the byte budget
@pytest.mark.parametrize("export", ALL)
def test_the_byte_budget_splits_a_batch(dev, export):
    first = se.budget_first_split(export)
    parent, taxon = se.supertree("caterpillar", np.arange(se.BUDGET_LEAVES))
    s_order = np.arange(se.BUDGET_LEAVES)
    for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
        trees = se.budget_trees(first + 1)[:m]
        ref = se.three_leaf_closed_form(s_order, trees, se.BUDGET_LEAVES)
        tabs = dev.upload(se.budget_tables(trees))
        try:
            plan = backend.debug_score_plan(tabs, se.BUDGET_LEAVES, 0, *se.export_extras(export, 2))
            assert len(plan["bstart"]) - 1 == batches and plan["bstart"][1] == first - 1, (export, m, plan["bstart"])
            _same(getattr(dev, export)(tabs, parent, taxon), ref, export, m)
        finally:
            tabs.free()


# ------------------------------------------------------------------------------------------------ refusals
@lru_cache(maxsize=None)
def _refusal_reference():
    parent, taxon, arrays, _, _ = se.refusal_tables("twice", 1)
    return se.reference(parent, taxon, arrays)


@pytest.mark.parametrize("bad_tree", [1, 7], ids=["first_batch", "third_batch"])
@pytest.mark.parametrize("kind", list(se.REFUSALS))
@pytest.mark.parametrize("export", ALL)
def test_refusals_in_the_first_and_in_a_later_batch(dev, export, kind, bad_tree):
    parent, taxon, _, good, bad = se.refusal_tables(kind, bad_tree)
    call = getattr(dev, export)
    if kind == "range":  # (the upload's own check comes first: the export never sees such tables)
        with pytest.raises(ValueError, match=r"scs_tables_upload: a leaf_taxon entry is out of range \[0, n_taxa\)"):
            call(bad, parent, taxon, se.REFUSAL_BATCH)
    else:
        tabs = dev.upload(bad)
        try:
            plan = backend.debug_score_plan(tabs, int((taxon >= 0).sum()), se.REFUSAL_BATCH)
            assert plan["bstart"].tolist() == [0, 3, 6, 9]
            used = dev.arena_stats()["used_bytes"]
            with pytest.raises(ValueError, match=f"^{C_NAME[export]}: {se.REFUSALS[kind]}$"):
                call(tabs, parent, taxon, se.REFUSAL_BATCH)
            assert dev.arena_stats()["used_bytes"] == used  # the call's block went back
        finally:
            tabs.free()
    ref = _refusal_reference()
    for bt in (se.REFUSAL_BATCH, 0):
        _same(call(good, parent, taxon, bt), ref, export, (kind, bad_tree, bt))
