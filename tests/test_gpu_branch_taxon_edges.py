"""The three scoring exports built on ``k_bt_*``, ``k_tx_*`` and ``k_rs_*`` on the device --
``scs_score_branch_triplets``, ``scs_score_taxon_triplets``, ``scs_score_branch_resample`` -- at the sizes where their
own plans change path: tree boundaries inside waves, the last workgroup of a tree, 64 words a
step of the rows' scan, the ``zb`` steps of the branch rows and of bin 0, dynamic LDS above 64 KiB, the LDS bins and
the slab path where it begins, 1 024 entries a round of ``tx_scan``, more trees than a weight chunk, counts from 2^32
on, the byte budget and the refusals in a later batch.  The cases and their references come from
``tests/branch_edge_reference.py`` (``tests/test_branch_edge_reference_cpu.py`` holds every case to the numbers it is
named for); every comparison is ``np.array_equal`` on int64 (int32 for ``rs_wins``)."""

from functools import lru_cache

import branch_edge_reference as be
import branch_triplet_reference as btr
import numpy as np
import pytest
import resample_reference as rr
import score_edge_reference as se

from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d
        d.trim(0)  # (the byte-budget cases took 1.6 GB of the arena)


def _same(res: dict, ref: dict, keys, what) -> None:
    for k in keys:
        got = res[k]
        assert got.dtype == np.int64 and got.shape == ref[k].shape, (what, k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (what, k, np.flatnonzero(got != ref[k])[:8], got[got != ref[k]][:8],
                                             ref[k][got != ref[k]][:8])


def _branch(dev, tabs, case, ref, batches=(0,)) -> None:
    for bt in batches:
        _same(dev.score_branch_triplets(tabs, case.parent, case.taxon, bt), ref, be.BRANCH, (case.name, "branch", bt))


def _taxon(dev, tabs, case, ref, batches=(0,), lds=0) -> None:
    for bt in batches:
        _same(dev.score_taxon_triplets(tabs, case.parent, case.taxon, bt, lds), ref, be.TAXON, (case.name, "taxon", bt))


def _resample(dev, tabs, case, weights, rows, batches=(0,)) -> None:
    """``rows``: [4][R][nodes] of exact integers (int64 or Python ints), all below 2^63."""
    want = np.asarray(rows).astype(np.int64)
    wins = be.wins(np.asarray(rows))
    for bt in batches:
        res = dev.score_branch_resample(tabs, case.parent, case.taxon, weights, rows=True, batch_trees=bt)
        what = (case.name, "resample", bt)
        assert res["rs_rows"].dtype == np.int64 and res["rs_wins"].dtype == np.int32
        assert np.array_equal(res["rs_rows"], want), (what, np.argwhere(res["rs_rows"] != want)[:8])
        assert np.array_equal(res["rs_point"], want[:, 0, :]), what
        assert np.array_equal(res["rs_wins"], wins.astype(np.int32)), (what, np.argwhere(res["rs_wins"] != wins)[:8])


def _node_sum(case: se.Case) -> dict:
    return btr.node_sum(se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays))


def _plan(dev, tabs, case, export: str, bt: int = 0, lds: int = 0) -> dict:
    return dev.debug_branch_plan(tabs, case.s_leaves, bt, *be.export_extras(export, len(case.parent)), lds)


def _scaled(closed: dict, weights) -> np.ndarray:
    """The rows of one source tree under ``weights`` (R x 1) from its branch counts."""
    per_node = np.stack([closed[k] for k in be.BRANCH_NODE])
    return np.asarray(weights, dtype=np.int64).reshape(1, -1, 1) * per_node[:, None, :]


# ------------------------------------------------------------------------------------------------ waves
@pytest.mark.parametrize("end", se.WAVE_ENDS)
def test_tree_boundaries_inside_waves(dev, end):
    case = be.wave_case(end)
    m = case.arrays.n_trees
    ref = _node_sum(case)
    assert all(ref[k].any() for k in be.BRANCH) and (ref["n_bt_total"] > 0).sum() > 10
    tref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    assert tref["tx_shared"].any() and (tref["tx_trees"] == 0).sum() >= 11
    weights = rr.case_weights(np.random.RandomState(end), m, 9)
    rows = rr.rows(weights, be.branch_arrays(case.parent, case.taxon, case.arrays, per_tree=True))
    tabs = dev.upload(case.tables())
    try:
        counts = [len(_plan(dev, tabs, case, "score_branch_triplets", bt)["bstart"]) - 1 for bt in case.batches]
        assert counts == [1, m, (m + 1) // 2, 2, 1]
        _branch(dev, tabs, case, ref, case.batches)
        _taxon(dev, tabs, case, tref, case.batches)
        _resample(dev, tabs, case, weights, rows, case.batches)
    finally:
        tabs.free()


def test_the_last_workgroup_of_a_tree(dev):
    case = be.last_workgroup_case()
    ref = _node_sum(case)
    assert ref["bt_concordant"].any() and ref["bt_alt1"].any() and ref["bt_alt2"].any()
    weights = rr.case_weights(np.random.RandomState(3), case.arrays.n_trees, 5)
    rows = rr.rows(weights, be.branch_arrays(case.parent, case.taxon, case.arrays, per_tree=True))
    tabs = dev.upload(case.tables())
    try:
        assert _plan(dev, tabs, case, "score_branch_triplets")["bt_zb"].tolist() == [8]
        _branch(dev, tabs, case, ref, case.batches)
        _resample(dev, tabs, case, weights, rows, case.batches)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ words and rounds
@pytest.mark.parametrize("size", [*be.ROUND_SIZES, *be.WORD_SIZES])
def test_rows_of_64_words_and_scan_rounds_of_1024(dev, size):
    case = be.words_case(size)
    ref = _node_sum(case)
    assert ref["bt_concordant"].any() and ref["bt_alt1"].any() and ref["bt_alt2"].any()
    tref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    assert len(set(tref["tx_shared"].tolist())) > 100 and tref["tx_super"].any() and tref["tx_source"].any()
    tabs = dev.upload(case.tables())
    try:
        assert _plan(dev, tabs, case, "score_branch_triplets")["bt_words"].tolist() == [(size >> 5) + 1]
        _branch(dev, tabs, case, ref)
        _taxon(dev, tabs, case, tref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the branch zb
@pytest.mark.parametrize(("size", "zb"), list(zip((*be.BT_ZB_87, *be.BT_ZB_21), (8, 7, 2, 1))))
@pytest.mark.parametrize("with_small", [False, True], ids=["alone", "batch"])
def test_branch_zb_steps_against_the_closed_forms(dev, size, zb, with_small):
    case = be.comb_case(size, "random", with_small)
    ref = be.comb_case_reference(case, "branch")
    assert ref["bt_concordant"].any() and ref["bt_alt1"].any() and ref["bt_alt2"].any()
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_branch_triplets")
        assert plan["bt_zb"].tolist() == [zb] and plan["bt_words"].tolist() == [(size >> 5) + 1]
        _branch(dev, tabs, case, ref)
        if not with_small:
            assert _plan(dev, tabs, case, "score_branch_resample")["bt_zb"].tolist() == [zb]
            _resample(dev, tabs, case, [[1], [3]], _scaled(ref, [1, 3]))
    finally:
        tabs.free()


@pytest.mark.parametrize(("size", "zb"), list(zip(be.BT_ZB_87, (8, 7))))
def test_branch_zb_8_to_7_with_large_sets_against_the_array_reference(dev, size, zb):
    case = be.zb_blocks_case(size)
    ref = be.branch_arrays(case.parent, case.taxon, case.arrays)
    assert (ref["bt_total"] > 10 ** 6).sum() == 30 and ref["bt_concordant"].any() and ref["bt_alt2"].any()
    tabs = dev.upload(case.tables())
    try:
        assert _plan(dev, tabs, case, "score_branch_triplets")["bt_zb"].tolist() == [zb]
        _branch(dev, tabs, case, ref)
    finally:
        tabs.free()
    at = case.note["large"]
    alone = se.Case(case.name + "_alone", case.parent, case.taxon, se.subset(case.arrays, [at]))
    tabs = dev.upload(alone.tables())
    try:
        _branch(dev, tabs, alone, be.branch_arrays(alone.parent, alone.taxon, alone.arrays))
    finally:
        tabs.free()


@pytest.mark.parametrize(("size", "kind"), list(zip(be.BT_LDS, ("interleave", "random", "blocks"))))
def test_branch_dynamic_lds_up_to_the_limit(dev, size, kind):
    case = be.comb_case(size, kind)
    ref = be.comb_case_reference(case, "branch")
    assert 0 < ref["n_bt_concordant"][0] < ref["n_bt_total"][0] and ref["n_bt_alternative"][0] > 0
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_branch_triplets")
        assert plan["bt_zb"].tolist() == [1] and plan["bt_workgroups"].tolist() == [size - 2]
        assert (plan["bt_lds"][0] > 64 * 1024) == (size >= 87360)
        _branch(dev, tabs, case, ref)
        _resample(dev, tabs, case, [[1], [3]], _scaled(ref, [1, 3]))
    finally:
        tabs.free()


def test_concordance_situations_through_the_branch_export(dev):
    case = se.concordance_case()
    ref = btr.node_sum(case.note["sup"], case.note["trees"])
    assert all(ref[k].any() for k in be.BRANCH)
    tabs = dev.upload(case.tables())
    try:
        _branch(dev, tabs, case, ref, case.batches)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the taxon bins
@pytest.mark.parametrize("n", be.BIN_SIZES)
def test_needs_on_both_sides_of_every_used_bin(dev, n):
    case = be.bin_case(n)
    ref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    assert len(set(ref["tx_shared"].tolist())) > n // 2
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets")
        assert plan["tx_dcap"].tolist() == [be.tx_plan_of((n >> 5) + 1)["dcap"]] and not plan["need_slab"]
        _taxon(dev, tabs, case, ref, case.batches)
    finally:
        tabs.free()


@pytest.mark.parametrize(("size", "zb"), list(zip(be.TX_ZB_87, (8, 7))))
def test_bin0_zb_8_to_7_against_the_quadratic_reference(dev, size, zb):
    case = be.tx_zb_case(size)
    ref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    tabs = dev.upload(case.tables())
    try:
        assert _plan(dev, tabs, case, "score_taxon_triplets")["tx_zb"][0, 0] == zb
        _taxon(dev, tabs, case, ref)
    finally:
        tabs.free()


@pytest.mark.parametrize(("size", "zb"), list(zip(be.TX_ZB_21, (2, 1))))
def test_bin0_zb_2_to_1_against_the_closed_form(dev, size, zb):
    case = be.comb_case(size, "random")
    ref = be.comb_case_reference(case, "taxon")
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets")
        assert plan["tx_zb"][0, 0] == zb and plan["tx_slab_launch"].tolist() == [1]
        _taxon(dev, tabs, case, ref)
    finally:
        tabs.free()


@pytest.mark.parametrize("where", be.ROUND_WHERE)
def test_single_node_workgroups_around_the_scan_rounds(dev, where):
    """``slab`` and ``lds`` under a cap; ``bin2`` (2 047 .. 2 049 entries) and ``bin0`` (all six totals) without one."""
    case, lds = be.round_case(where)
    ref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    want = {"slab": ([8, 2, 1], [0, 0, 0]), "lds": ([1, 1, 1], [2061, 0, 0]), "bin2": ([2, 2, 1], [2046, 0, 19194]),
            "bin0": ([1, 1, 1], [4982, 0, 18806])}[where]
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets", 0, lds)
        assert plan["tx_slab_launch"].tolist() == [1] and (lds == 0) == (where in ("bin2", "bin0"))
        assert plan["tx_dcap"].tolist() == [want[1]] and (where == "slab" or plan["tx_zb"].tolist() == [want[0]])
        _taxon(dev, tabs, case, ref, (0,), lds)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the slab
@pytest.mark.parametrize(("size", "slab"), list(zip(be.TX_SLAB_BEGINS, (0, 1, 1))))
@pytest.mark.parametrize("second", [False, True], ids=["alone", "batch"])
def test_the_slab_path_where_it_begins(dev, size, slab, second):
    case = be.comb_case(size, "random", second=size - 1 if second else 0)
    ref = be.comb_case_reference(case, "taxon")
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets")
        assert plan["need_slab"] == slab and plan["slab_wgs"] == 256 * slab and plan["tx_slab_launch"].tolist() == [slab]
        _taxon(dev, tabs, case, ref)
    finally:
        tabs.free()


@pytest.mark.parametrize("which", list(be.ROBIN_NODES))
def test_the_slab_round_robin_below_at_and_above_its_workgroups(dev, which):
    case = be.robin_case(which)
    ref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets", 0, 100)
        assert plan["slab_wgs"] == 256 and plan["tx_slab_launch"].tolist() == [1]
        _taxon(dev, tabs, case, ref, (0, 2), 100)
    finally:
        tabs.free()


@pytest.mark.parametrize("size", be.TX_SLAB_LDS)
def test_the_slab_kernels_lds_past_64_kib(dev, size):
    """The twin trees of ``test_gpu_taxon_triplets.py`` at these sizes: the permuted caterpillars, whose values differ
    from leaf to leaf, took 3.5 s each here (every node of a caterpillar takes the slab), above the bound of a test."""
    case = be.twin_case(size)
    ref = be.twin_reference(size)
    tabs = dev.upload(case.tables())
    try:
        plan = _plan(dev, tabs, case, "score_taxon_triplets")
        assert plan["tx_slab_launch"].tolist() == [1]
        assert plan["tx_slab_lds"].tolist() == [65536 if size == 131071 else 65552]
        _taxon(dev, tabs, case, ref)
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the resample
@pytest.mark.parametrize("n_rep", be.RS_REPS)
@pytest.mark.parametrize("n_trees", be.RS_TREES)
def test_more_trees_than_a_weight_chunk(dev, n_trees, n_rep):
    parent, taxon, arrays, each = be.chunk_forest()
    case = se.Case(f"rs_chunk_{n_trees}", parent, taxon, se.subset(arrays, range(n_trees)))
    weights = be.chunk_weights(n_rep, n_trees)
    tabs = dev.upload(case.tables())
    try:
        assert len(_plan(dev, tabs, case, "score_branch_resample")["bstart"]) == 2  # one batch
        _resample(dev, tabs, case, weights, be.weighted_rows(weights, each[:n_trees]))
    finally:
        tabs.free()


def test_counts_from_2_to_the_32_on(dev):
    case = be.big_case()
    each = be.branch_arrays(case.parent, case.taxon, case.arrays, per_tree=True)
    assert all(int(each[0, x, 1]) >= 2 ** 32 for x in (0, 1))
    weights = [[w] for w in be.big_weights(int(case.sizes[0]))]
    rows = rr.rows(weights, each)  # Python integers
    assert max(int(v) for v in rows[0, :, 1]) > 2 ** 62
    tabs = dev.upload(case.tables())
    try:
        _resample(dev, tabs, case, weights, rows)
        _branch(dev, tabs, case, be.branch_arrays(case.parent, case.taxon, case.arrays))
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ the byte budget
@pytest.mark.parametrize("export", list(be.C_NAME))
def test_the_byte_budget_splits_a_batch(dev, export):
    first = be.budget_first_split(export)
    s_order = np.arange(se.BUDGET_LEAVES)
    parent, taxon = se.supertree("caterpillar", s_order)
    for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
        trees = se.budget_trees(first + 1)[:m]
        ref = be.three_leaf(s_order, trees, se.BUDGET_LEAVES)
        case = se.Case(f"budget_{export}_{m}", parent, taxon, None)
        tabs = dev.upload(se.budget_tables(trees))
        try:
            plan = dev.debug_branch_plan(tabs, se.BUDGET_LEAVES, 0, *be.export_extras(export, len(parent)))
            assert len(plan["bstart"]) - 1 == batches and plan["bstart"][1] == first - 1, (export, m, plan["bstart"])
            if export == "score_branch_triplets":
                _branch(dev, tabs, case, ref)
            elif export == "score_taxon_triplets":
                _taxon(dev, tabs, case, ref)
            else:
                weights = rr.case_weights(np.random.RandomState(m), m, 3)
                _resample(dev, tabs, case, weights, be.three_leaf_rows(ref, weights, len(parent)))
        finally:
            tabs.free()


# ------------------------------------------------------------------------------------------------ refusals
@lru_cache(maxsize=None)
def _refusal_reference():
    parent, taxon, arrays, _, _ = se.refusal_tables("twice", 1)
    weights = rr.case_weights(np.random.RandomState(9), arrays.n_trees, 4)
    return (be.branch_arrays(parent, taxon, arrays), be.taxon_reference(parent, taxon, arrays), weights,
            rr.rows(weights, be.branch_arrays(parent, taxon, arrays, per_tree=True)))


@pytest.mark.parametrize("bad_tree", [1, 7], ids=["first_batch", "third_batch"])
@pytest.mark.parametrize("export", list(be.C_NAME))
def test_a_taxon_twice_in_the_first_and_in_a_later_batch(dev, export, bad_tree):
    parent, taxon, _, good, bad = se.refusal_tables("twice", bad_tree)
    bref, tref, weights, rows = _refusal_reference()
    case = se.Case(f"refusal_{export}_{bad_tree}", parent, taxon, None)
    args = (weights,) if export == "score_branch_resample" else ()
    kw = {"batch_trees": se.REFUSAL_BATCH}
    tabs = dev.upload(bad)
    try:
        plan = dev.debug_branch_plan(tabs, case.s_leaves, se.REFUSAL_BATCH, *be.export_extras(export, len(parent)))
        assert plan["bstart"].tolist() == [0, 3, 6, 9]
        used = dev.arena_stats()["used_bytes"]
        with pytest.raises(ValueError, match=f"^{be.C_NAME[export]}: a source tree has a taxon twice$"):
            getattr(dev, export)(tabs, parent, taxon, *args, **kw)
        assert dev.arena_stats()["used_bytes"] == used  # the call's block went back
    finally:
        tabs.free()
    tabs = dev.upload(good)
    try:
        for bt in (se.REFUSAL_BATCH, 0):
            if export == "score_branch_triplets":
                _branch(dev, tabs, case, bref, (bt,))
            elif export == "score_taxon_triplets":
                _taxon(dev, tabs, case, tref, (bt,))
            else:
                _resample(dev, tabs, case, weights, rows, (bt,))
    finally:
        tabs.free()
