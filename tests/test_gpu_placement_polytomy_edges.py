"""The exports built on ``k_pl_*``, ``k_cp_*`` and ``k_py_*`` on the device -- ``scs_score_placements``,
``scs_score_clade_placements`` / ``scs_score_clade_moves``, ``scs_score_polytomies`` -- at the sizes where their own
plans change path: tree boundaries inside waves, the last workgroup of a tree, 64 words a step of
the rows' scans, the ``zb`` steps, the sums beside the rows under a cap, the last pass and its pad, the common rows,
1 024 nodes a round of the prefix, caterpillar lists, the clade passes and masks, the polytomy rows' stride and sums,
the colours, more trees than a grid row, counts from 2^32 on, the byte budget and the refusals in a later batch.  The cases and their array references (``placement_arrays``, ``clade_arrays``, ``polytomy_arrays``) come from
``tests/placement_edge_reference.py`` (``tests/test_placement_edge_reference_cpu.py`` holds every case to the numbers it
is named for and the array references to the brute-force ones); the exports are called directly with ``batch_trees``
and ``lds_bytes``; every comparison is ``np.array_equal`` on int64."""

from functools import lru_cache

import clade_placement_reference as cr
import numpy as np
import placement_edge_reference as pe
import polytomy_reference as yr
import pytest
import refine_reference as rf
import score_edge_reference as se

from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d
        d.trim(0)


def _same(res: dict, ref: dict, keys, what) -> None:
    for k in keys:
        got, want = res[k], np.asarray(ref[k], dtype=np.int64)
        assert got.dtype == np.int64 and got.shape == want.shape, (what, k, got.shape, want.shape)
        assert np.array_equal(got, want), (what, k, np.argwhere(got != want)[:8], got[got != want][:8],
                                           want[got != want][:8])


def _placements(dev, tabs, case, ref, batches=(0,), lds=0, queries=None) -> None:
    q = case.note["queries"] if queries is None else queries
    for bt in batches:
        _same(dev.score_placements(tabs, case.parent, case.taxon, q, bt, lds), ref, pe.PLACEMENTS,
              (case.name, "placements", bt, lds))


def _clades(dev, tabs, case, ref, batches=(0,), lds=0) -> None:
    for bt in batches:
        _same(dev.score_clade_placements(tabs, case.parent, case.taxon, case.note["clades"], bt, lds), ref, pe.CLADES,
              (case.name, "clades", bt, lds))


def _polytomies(dev, tabs, case, ref, batches=(0,), lds=0) -> None:
    for bt in batches:
        res = dev.score_polytomies(tabs, case.parent, case.taxon, case.note["polytomies"], bt, lds)
        what = (case.name, "polytomies", bt, lds)
        assert res["py_degree"].dtype == np.int32 and np.array_equal(res["py_degree"], ref["py_degree"]), what
        _same(res, ref, ("py_trees",), what)
        for key in ("py_total", "py_joint"):
            assert len(res[key]) == len(ref[key]), (what, key)
            for i, (got, want) in enumerate(zip(res[key], ref[key])):
                assert got.dtype == np.int64 and got.shape == want.shape, (what, key, i)
                assert np.array_equal(got, want), (what, key, i, np.argwhere(got != want)[:8])


def _moves(dev, tabs, case, rows: dict, top_k: int = 8, bt: int = 0, lds: int = 0) -> None:
    """``score_clade_moves`` against ``refine_reference.top_k`` of the judged rows."""
    queries = case.note["clades"]
    res = dev.score_clade_moves(tabs, case.parent, case.taxon, queries, top_k, bt, lds)
    _same(res, rows, pe.CLADES[:3], (case.name, "moves"))
    _, _, end = pe.preorder_tables(case.parent, case.taxon)
    sup, shared = np.asarray(rows["cp_super"], dtype=np.int64), np.asarray(rows["cp_shared"], dtype=np.int64)
    d = sup - 2 * shared
    at = np.arange(len(queries))
    want = np.stack([rf.top_k(d[i], q, end[q], top_k) for i, q in enumerate(queries)])
    assert res["mv_node"].dtype == np.int32 and np.array_equal(res["mv_node"], want), (case.name, "moves")
    assert np.array_equal(res["mv_own_super"], sup[at, queries]) and np.array_equal(res["mv_own_shared"], shared[at, queries])
    there = np.maximum(want, 0)
    for key, row in (("mv_super", sup), ("mv_shared", shared)):
        assert np.array_equal(res[key], np.where(want >= 0, row[at[:, None], there], 0)), (case.name, "moves", key)


def _plan(dev, tabs, case, bt: int = 0, lds: int = 0) -> dict:
    note = case.note
    lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
    subs = int(sum(hi[q] - lo[q] for q in note.get("clades", ()))) or 1
    kids = np.bincount(np.asarray(case.parent)[1:], minlength=len(case.parent))
    return dev.debug_placement_plan(tabs, case.s_leaves, bt, lds, max(len(note.get("queries", ())), 1), subs,
                                    [int(kids[q]) for q in note.get("polytomies", ())])


def _arrays(case: se.Case, queries=None) -> dict:
    return pe.placement_arrays(case.parent, case.taxon, case.arrays, case.note["queries"] if queries is None else queries)


def _composed(case: se.Case) -> dict:
    return cr.composed(se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays), case.note["clades"])


def _clade_arrays(case: se.Case) -> dict:
    return pe.clade_arrays(case.parent, case.taxon, case.arrays, case.note["clades"])


def _py_arrays(case: se.Case) -> dict:
    return pe.polytomy_arrays(case.parent, case.taxon, case.arrays, case.note["polytomies"])


# ------------------------------------------------------------------------------------------------ waves
@pytest.mark.parametrize("end", se.WAVE_ENDS)
def test_tree_boundaries_inside_waves(dev, end):
    case = pe.wave_case(end)
    m = case.arrays.n_trees
    ref = _arrays(case)
    assert ref["pl_shared"].any() and (ref["pl_trees"] == 0).sum() == 2 and (ref["pl_trees"] > 0).sum() >= 6
    cref = _composed(case)
    assert (cref["cp_trees"] > 0).sum() >= 4 and (cref["cp_trees"] == 0).any() and cref["cp_shared"].any()
    yref = _py_arrays(case)
    tabs = dev.upload(case.tables())
    try:
        counts = [len(_plan(dev, tabs, case, bt)["pl_bstart"]) - 1 for bt in case.batches]
        assert counts == [1, m, (m + 1) // 2, 2, 1]
        _placements(dev, tabs, case, ref, case.batches)
        _clades(dev, tabs, case, cref, case.batches)
        _polytomies(dev, tabs, case, yref, case.batches)
    finally:
        tabs.free()


def test_the_last_workgroup_of_a_tree(dev):
    case = pe.last_workgroup_case()
    ref = _arrays(case)
    assert ref["pl_shared"].any() and (ref["pl_trees"] >= 5).all()
    cref = _composed(case)
    assert cref["cp_shared"].any()
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case)
        assert plan["pl_zb"].tolist() == [8] and plan["cp_zb"].tolist() == [8]
        _placements(dev, tabs, case, ref, case.batches)
        _clades(dev, tabs, case, cref, case.batches)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ words
@pytest.mark.parametrize("size", pe.WORD_SIZES)
def test_rows_of_64_words_a_scan_step(dev, size):
    case = pe.words_case(size)
    ref = _arrays(case)
    assert all(len(set(ref["pl_shared"][i].tolist())) > 50 for i in range(3))
    yref = _py_arrays(case)
    assert all(j.any() for j in yref["py_joint"])
    cref = _clade_arrays(case)
    assert cref["cp_trees"].tolist() == [1, 1, 1] and all(len(set(r.tolist())) > 50 for r in cref["cp_shared"])
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case)
        assert plan["pl_words"].tolist() == [(size >> 5) + 1] and plan["py_words"][0, 0] == (size + 31) >> 5
        assert plan["cp_words"].tolist() == [(size >> 5) + 1]
        _placements(dev, tabs, case, ref)
        _polytomies(dev, tabs, case, yref)
        _clades(dev, tabs, case, cref)
        _moves(dev, tabs, case, cref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ zb
@pytest.mark.parametrize(("size", "zb"), list(zip((*pe.ZB_87, *pe.ZB_21), (8, 7, 2, 1))))
@pytest.mark.parametrize("with_small", [False, True], ids=["alone", "batch"])
def test_zb_steps_against_the_array_reference(dev, size, zb, with_small):
    case = pe.zb_case(size, with_small)
    ref = _arrays(case)
    assert all(len(set(ref["pl_shared"][i].tolist())) > 100 for i in range(2))
    cref = _clade_arrays(case)
    assert (cref["cp_trees"] >= 1).all() and all(len(set(r.tolist())) > 100 for r in cref["cp_shared"])
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case)
        assert plan["pl_zb"].tolist() == [zb] and plan["pl_sums"].tolist() == [1]
        assert plan["pl_blk"][case.note["large"]] == (2 * size + zb - 1) // zb
        assert plan["cp_zb"].tolist() == [zb] and plan["cp_sums"].tolist() == [1]
        _placements(dev, tabs, case, ref)
        _clades(dev, tabs, case, cref)
        _moves(dev, tabs, case, cref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ large trees
@pytest.mark.parametrize(("size", "nq", "sums", "lds"), [(pe.LDS_64K[0], 1, 1, 65536), (pe.LDS_64K[1], 1, 1, 65552),
                                                         (pe.NO_SUMS_1[0], 1, 1, 163840), (pe.NO_SUMS_1[1], 1, 0, 163792),
                                                         (pe.PL_CAP, 2, 0, 163840)])
def test_dynamic_lds_the_no_sums_path_and_the_leaf_limit(dev, size, nq, sums, lds):
    """One node a workgroup.  The pair of 64 queries either side of 325 024 leaves gave equal results here in 0.11 s
    and 0.16 s on the device, but its host reference takes 7.3 s: the one-query pair stands for it."""
    case = pe.large_case(size, nq)
    ref = _arrays(case)
    assert int(ref["pl_shared"].max()) > (2 ** 32 if size > 200000 else 2 ** 31) and ref["pl_trees"].tolist() == [1] * nq
    cref = _clade_arrays(case)  # (one sub-query: the clade's plan is the plan of one query)
    assert cref["cp_trees"].tolist() == [1] and int(cref["cp_shared"].max()) > 2 ** 31
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case)
        assert (plan["pl_zb"][0], plan["pl_sums"][0], plan["pl_lds_full"][0]) == (1, sums, lds)
        assert (plan["cp_zb"][0], plan["cp_sums"][0]) == (1, 1 if nq == 2 and size < pe.NO_SUMS_1[1] else sums)
        _placements(dev, tabs, case, ref)
        _clades(dev, tabs, case, cref)
    finally:
        tabs.free()


def test_placement_counts_from_2_to_the_32_on(dev):
    case = pe.big_placement_case()
    ref = _arrays(case)
    own = (pe.BIG_TWIN - 1) * (pe.BIG_TWIN - 2) // 2
    assert int(ref["pl_shared"].max()) == own > 2 ** 32 and ref["pl_source"].tolist() == [own, own]
    cref = _clade_arrays(case)
    assert (cref["cp_shared"].max(axis=1) > 2 ** 33).all() and cref["cp_trees"].tolist() == [1, 1]
    tabs = dev.upload(case.tables())
    try:
        _placements(dev, tabs, case, ref)
        _clades(dev, tabs, case, cref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the cap
@pytest.mark.parametrize("lds", pe.CAP_BYTES)
def test_sums_beside_the_rows_under_a_cap(dev, lds):
    case = pe.cap_case()
    ref, cref = _cap_reference()
    want = {287: (1, 0), 288: (1, 1), 543: (1, 1), 544: (2, 1), 2079: (7, 1), 2080: (8, 1), 0: (8, 1)}[lds]
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, 0, lds)
        assert (plan["pl_zb"][0], plan["pl_sums"][0]) == want and (plan["cp_zb"][0], plan["cp_sums"][0]) == want
        _placements(dev, tabs, case, ref, (0,), lds)
        _clades(dev, tabs, case, cref, (0,), lds)
    finally:
        tabs.free()


@lru_cache(maxsize=None)
def _cap_reference():
    case = pe.cap_case()
    return _arrays(case), _composed(case)


# ------------------------------------------------------------------------------------------------ passes
@lru_cache(maxsize=None)
def _pass_reference():
    """The rows of all 129 queries and of the 129 one-tip clades; a case with fewer takes the first of them."""
    return _arrays(pe.pass_case()), _clade_arrays(pe.pass_case())


@pytest.mark.parametrize("nq", pe.LAST_PASS)
def test_the_last_pass_and_its_pad(dev, nq):
    case = pe.pass_case()
    ref, cref = ({k: v[:nq] for k, v in r.items()} for r in _pass_reference())
    assert ref["pl_shared"][nq - 1].any() and cref["cp_shared"][nq - 1].any()
    some = se.Case(case.name, case.parent, case.taxon, case.arrays, note={"clades": case.note["clades"][:nq]})
    tabs = dev.upload(case.tables())
    try:
        _placements(dev, tabs, case, ref, (0, 5), 0, case.note["queries"][:nq])
        _clades(dev, tabs, some, cref, (0, 5))
    finally:
        tabs.free()


def test_common_rows_of_a_pass(dev):
    case = pe.common_case()
    ref = _arrays(case)
    assert (ref["pl_trees"][:128] >= 2).all() and ref["pl_trees"][128] == 9
    tabs = dev.upload(case.tables())
    try:
        _placements(dev, tabs, case, ref, case.batches)
    finally:
        tabs.free()


@pytest.mark.parametrize("count", pe.NODE_COUNTS)
def test_supertrees_of_1024_nodes_a_round(dev, count):
    case = pe.nodes_case(count)
    ref = _arrays(case)
    assert all(len(set(ref["pl_super"][i].tolist())) > 20 for i in range(5))
    cref = _composed(case)
    tabs = dev.upload(case.tables())
    try:
        _placements(dev, tabs, case, ref)
        _clades(dev, tabs, case, cref)
    finally:
        tabs.free()


def test_caterpillar_lists_beside_short_ones(dev):
    case = pe.lists_case()
    ref = _arrays(case)
    assert (ref["pl_trees"] >= 1).all() and ref["pl_shared"].any()
    tabs = dev.upload(case.tables())
    try:
        _placements(dev, tabs, case, ref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ clades
@pytest.mark.parametrize("which", list(pe.CLADE_PASSES))
def test_clade_passes(dev, which):
    case = pe.clade_pass_case(which)
    ref = _composed(case)
    assert (ref["cp_trees"] > 0).all() and ref["cp_shared"].any()
    tabs = dev.upload(case.tables())
    try:
        _clades(dev, tabs, case, ref, case.batches)
        if which == "64_5":
            _moves(dev, tabs, case, ref)
    finally:
        tabs.free()


def test_clade_rows_past_64_words_and_the_moves_over_them(dev):
    """The Q' row of ``k_cp_clades`` (one wave, 64 words a step) on a crossed tree of 2 100 leaves, and ``k_cp_best``
    over rows of 4 000 nodes made here."""
    case = pe.clade_words_case()
    ref = _composed(case)
    assert ref["cp_trees"].tolist() == [1, 1, 1] and all(len(set(r.tolist())) > 50 for r in ref["cp_shared"])
    tabs = dev.upload(case.tables())
    try:
        assert _plan(dev, tabs, case)["cp_words"].tolist() == [(pe.CLADE_WORDS >> 5) + 1]
        _clades(dev, tabs, case, ref)
        _moves(dev, tabs, case, ref)
    finally:
        tabs.free()


@pytest.mark.parametrize("n", [*pe.MASK_SIZES, pe.MASK_LARGE])
def test_clade_masks_around_the_query_clade(dev, n):
    case = pe.mask_case(n)
    # (brute force over the regrafted trees' sets takes 7 s at 40 leaves: there ``composed``, which the CPU tests hold to it)
    judge = cr.brute_force if n <= 17 else cr.composed
    ref = (_clade_arrays(case) if n > 40 else
           judge(se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays), case.note["clades"]))
    assert ref["cp_trees"].any()
    tabs = dev.upload(case.tables())
    try:
        _clades(dev, tabs, case, ref, case.batches)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ polytomies
@pytest.mark.parametrize(("size", "k"), [*[(n, 64) for n in pe.PY_WIDE], *[(n, 3) for n in pe.PY_THREE]])
def test_polytomy_rows_stride_and_sums(dev, size, k):
    case = pe.py_case(size, k)
    ref = _py_arrays(case)
    assert ref["py_degree"][0] == k and ref["py_trees"][0] >= 1 and (ref["py_joint"][0] > 0).sum() >= k
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case)
        assert tuple(int(plan[f"py_{x}"][0, 0]) for x in ("words", "stride", "acc_lds", "lds")) == pe.py_plan(size, k)
        _polytomies(dev, tabs, case, ref)
    finally:
        tabs.free()


@pytest.mark.parametrize("k", pe.COLOUR_DEGREES)
def test_colours_that_are_empty_and_trees_that_are_not_decisive(dev, k):
    case = pe.colour_case(k)
    ref = _py_arrays(case)
    node = yr.node_sum(se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays), only=[0])
    assert np.array_equal(ref["py_joint"][0], node["joint"][0]) and np.array_equal(ref["py_total"][0], node["total"][0])
    assert 0 < ref["py_trees"][0] < case.arrays.n_trees
    tabs = dev.upload(case.tables())
    try:
        _polytomies(dev, tabs, case, ref, case.batches)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the grid row
@pytest.mark.parametrize("count", pe.GRID_COUNTS)
def test_more_trees_than_a_grid_row(dev, count):
    """One batch of three-leaf sources: from 65 536 trees on ``k_py_sweep`` is launched twice, the second time on
    pointers moved past the first 65 535 trees."""
    parent, taxon = pe.grid_supertree()
    orders, cat = pe.grid_sources()
    ref = pe.three_leaf_polytomies(parent, taxon, [0, 1], orders[:count], cat[:count])
    assert ref["py_degree"].tolist() == [3, 4] and (ref["py_trees"] > 5000).all()
    case = se.Case(f"py_grid_{count}", parent, taxon, None, note={"polytomies": [0, 1]})
    tabs = dev.upload(pe.grid_tables(count))
    try:
        plan = dev.debug_placement_plan(tabs, pe.GRID_TAXA, 0, 0, 1, 1, [3, 4])
        assert plan["py_bstart"].tolist() == [0, count]
        _polytomies(dev, tabs, case, ref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ 2^32
def test_polytomy_counts_from_2_to_the_32_on(dev):
    case = pe.big_polytomy_case()
    ref = _py_arrays(case)
    assert int(ref["py_joint"][0][0, 1, 2]) >= 2 ** 32 and int(ref["py_total"][0][0, 1, 2]) >= 2 ** 32
    tabs = dev.upload(case.tables())
    try:
        _polytomies(dev, tabs, case, ref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the byte budget
@pytest.mark.parametrize("export", pe.BUDGET_EXPORTS)
def test_the_byte_budget_splits_a_batch(dev, export):
    first = pe.budget_first_split(export)
    name = {"score_placements": "pl", "score_clade_placements": "cp", "score_polytomies": "py"}[export]
    for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
        case = pe.budget_case(export, m)
        tabs = dev.upload(case.note["tables"])
        try:
            plan = _plan(dev, tabs, case)
            starts = plan[f"{name}_bstart"]
            assert len(starts) - 1 == batches and starts[1] == first - 1, (export, m, starts)
            if export == "score_placements":
                ref = _arrays(case)
                assert ref["pl_trees"].tolist() == [1, int(m >= first), int(m > first)] and ref["pl_shared"].any()
                _placements(dev, tabs, case, ref)
            elif export == "score_clade_placements":
                ref = _clade_arrays(case)
                assert ref["cp_trees"].tolist() == [1, int(m >= first), int(m > first)]
                _clades(dev, tabs, case, ref)
                _moves(dev, tabs, case, ref)
            else:
                ref = _py_arrays(case)
                assert ref["py_trees"][0] > 800
                _polytomies(dev, tabs, case, ref)
        finally:
            tabs.free()


# ------------------------------------------------------------------------------------------------ refusals
@lru_cache(maxsize=None)
def _refusal_reference():
    parent, taxon, arrays, _, _ = se.refusal_tables("twice", 1)
    case = se.Case("refusal", parent, taxon, arrays, note=pe.refusal_queries(parent, taxon))
    return case, _arrays(case), _composed(case), _py_arrays(case)


@pytest.mark.parametrize("bad_tree", [1, 7], ids=["first_batch", "third_batch"])
@pytest.mark.parametrize("export", list(pe.C_NAME))
def test_a_taxon_twice_in_the_first_and_in_a_later_batch(dev, export, bad_tree):
    _, _, _, good, bad = se.refusal_tables("twice", bad_tree)
    case, ref, cref, yref = _refusal_reference()
    parent, taxon, note = case.parent, case.taxon, case.note
    args = {"score_placements": (note["queries"],), "score_clade_placements": (note["clades"],),
            "score_clade_moves": (note["clades"], 8), "score_polytomies": (note["polytomies"],)}[export]
    tabs = dev.upload(bad)
    try:
        plan = _plan(dev, tabs, case, se.REFUSAL_BATCH)
        assert all(plan[f"{x}_bstart"].tolist() == [0, 3, 6, 9] for x in ("pl", "cp", "py"))
        used = dev.arena_stats()["used_bytes"]
        with pytest.raises(ValueError, match=f"^{pe.C_NAME[export]}: a source tree has a taxon twice$"):
            getattr(dev, export)(tabs, parent, taxon, *args, batch_trees=se.REFUSAL_BATCH)
        assert dev.arena_stats()["used_bytes"] == used  # the call's block went back
    finally:
        tabs.free()
    tabs = dev.upload(good)
    try:
        for bt in (se.REFUSAL_BATCH, 0):
            if export == "score_placements":
                _placements(dev, tabs, case, ref, (bt,))
            elif export == "score_clade_placements":
                _clades(dev, tabs, case, cref, (bt,))
            elif export == "score_clade_moves":
                _moves(dev, tabs, case, cref, 8, bt)
            else:
                _polytomies(dev, tabs, case, yref, (bt,))
    finally:
        tabs.free()
