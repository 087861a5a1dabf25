"""No device: the closed forms and the array reference of ``tests/branch_edge_reference.py`` equal the project's
references where those can go, the plans of the branch and taxon kernels restated in Python equal the library's own
(``scs_debug_branch_plan``), every case of ``tests/test_gpu_branch_taxon_edges.py`` has the numbers it is named for
(DESIGN.md section 30), and the new entry is declared, bound and exported."""

import re
from pathlib import Path

import branch_edge_reference as be
import branch_triplet_reference as btr
import build_reference as br
import numpy as np
import pytest
import resample_reference as rr
import score_edge_reference as se

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend

ROOT = Path(__file__).resolve().parent.parent
KIB = 1024
EXPORTS = tuple(be.C_NAME)


def _starts(case: se.Case) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(case.sizes)])


def _same_plan(off, s_leaves, bt=0, epl=0, ept=0, lds=0) -> dict:
    want = be.branch_plan(off, s_leaves, bt, epl, ept, lds)
    got = backend.debug_branch_plan(np.asarray(off, dtype=np.int64), s_leaves, bt, epl, ept, lds)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, bt, lds, got[k], want[k])
    return got


def _tips(case: se.Case, t: int) -> np.ndarray:
    _, tax = be.tree_slice(case.arrays, t)
    return tax[tax >= 0]


# ------------------------------------------------------------------------------------------------ the plans
def test_branch_zb_steps_and_lds_sit_at_their_sizes():
    first = {}  # the first size at which zb takes each value
    prev = be.BT_ZMAX
    for n in range(32, be.BT_CAP + 2, 32):  # (words change at multiples of 32 only)
        zb = be.bt_words_zb(n)[1]
        if zb != prev:
            first[zb] = n
            prev = zb
    assert [first[z] for z in (7, 6, 5, 4, 3, 2, 1)] == list(be.BT_ZB_STEPS) == [6816, 7776, 9088, 10912, 13632,
                                                                                  18176, 27296]
    assert [be.bt_words_zb(n)[:2] for n in (6815, 6816, 27295, 27296)] == [(213, 8), (214, 7), (853, 2), (854, 1)]
    assert be.bt_words_zb(87359)[2] == 24 * 2730 <= 64 * KIB < be.bt_words_zb(87360)[2] == 24 * 2731 == 65544
    assert be.BT_CAP == 218431 and be.bt_words_zb(be.BT_CAP)[2] == 24 * 6826 <= se.TP_LDS_MAX
    assert be.BT_ROW_BYTES * ((be.BT_CAP + 1 >> 5) + 1) > se.TP_LDS_MAX  # one leaf more is refused
    # the 768 bytes of the wave sums exceed the rows below 96 leaves (zb = 8, three words at 64 .. 95 leaves)
    assert be.BT_WAVE_SUMS == 768
    assert [be.bt_words_zb(n)[2] for n in (31, 64, 95, 96, 127, 128)] == [768, 768, 768, 768, 768, 960]
    assert [8 * 24 * ((n >> 5) + 1) for n in (95, 96)] == [576, 768]


def test_taxon_bins_and_the_slab_begin_at_their_sizes():
    p = be.tx_plan_of((159 >> 5) + 1)
    assert p["dcap"] == [309, 320, 0] and p["zb"] == [8, 2, 1] and 2 * 159 + 1 == 319
    assert be.tx_plan_of(51)["dcap"][1:] == [3222, 3264]  # 1 600 .. 1 631 leaves
    assert be.tx_plan_of((1632 >> 5) + 1)["dcap"] == [215, 3220, 3328]
    zb0 = lambda n: be.tx_plan_of((n >> 5) + 1)["zb"][0]  # noqa: E731
    assert [zb0(n) for n in (3071, 3072, 26623, 26624)] == [8, 7, 2, 1]
    first = {}
    prev = 8
    for n in range(32, 40000, 32):
        if zb0(n) != prev:
            first[zb0(n)] = n
            prev = zb0(n)
    assert first[7] == 3072 and first[1] == 26624 and sorted(first) == [1, 2, 3, 4, 5, 6, 7]
    # a bin drops out when it cannot be larger than the one before: bin 1 from 17 728, bin 0 from 106 240, bin 2 from
    # 327 424 leaves (every node then takes the slab)
    used = lambda n: [c > 0 for c in be.tx_plan_of((n >> 5) + 1)["dcap"]]  # noqa: E731
    assert used(17727) == [True, True, True] and used(17728) == [True, False, True]
    assert used(106239) == [True, False, True] and used(106240) == [False, False, True]
    assert used(327423) == [False, False, True] and used(327424) == [False, False, False]
    # the slab: needed from 9 925 leaves on (W = 311); its own LDS, 16 W bytes, passes 64 KiB at 131 072
    assert [be.tx_call_of(n)["need_slab"] for n in be.TX_SLAB_BEGINS] == [0, 1, 1] and (9925 >> 5) + 1 == 311
    assert be.tx_plan_of(311)["dcap_max"] == 19850 == 2 * 9925
    assert 16 * ((131071 >> 5) + 1) == 64 * KIB and 16 * ((131072 >> 5) + 1) == 64 * KIB + 16
    assert be.tx_call_of(300)["slab_wgs"] == 0 and be.tx_call_of(300, 100)["slab_wgs"] == 256
    assert be.tx_call_of(131072)["slab_wgs"] == 63


def test_the_python_plans_equal_the_librarys_for_every_row_width():
    for lds in (0, 100, 4 * 16 * 345 - 1):
        for w in range(1, 10241):
            n = 32 * w - 1  # the largest tree of w words
            p = be.tx_plan_of(w, min(lds, se.TP_LDS_MAX) if lds else se.TP_LDS_MAX)
            got = backend.debug_branch_plan(np.asarray([0, n], dtype=np.int64), n, 0, 0, 0, lds)
            words, zb, bytes_ = be.bt_words_zb(n)
            assert (got["bt_words"][0], got["bt_zb"][0], got["bt_lds"][0]) == (words, zb, bytes_) and words == w
            assert got["bt_workgroups"][0] == -(-max(n - 2, 0) // zb)
            assert got["tx_zb"][0].tolist() == p["zb"] and got["tx_dcap"][0].tolist() == p["dcap"], (w, lds)
            assert got["tx_lds"][0].tolist() == p["lds"], (w, lds)
            call = be.tx_call_of(n, lds)
            assert (got["need_slab"], got["slab_wgs"], got["slab_stride"]) == (call["need_slab"], call["slab_wgs"],
                                                                               call["slab_stride"])


def _every_case():
    for end in se.WAVE_ENDS:
        yield be.wave_case(end), 0
    yield be.last_workgroup_case(), 0
    for size in (*be.ROUND_SIZES, *be.WORD_SIZES):
        yield be.words_case(size), 0
    for size in (*be.BT_ZB_87, *be.BT_ZB_21):
        yield be.comb_case(size, "random", with_small=True), 0
    for size in be.BT_ZB_87:
        yield be.zb_blocks_case(size), 0
    for size in be.BT_LDS:
        yield be.comb_case(size, "blocks"), 0
    for n in be.BIN_SIZES:
        yield be.bin_case(n), 0
    for size in be.TX_ZB_87:
        yield be.tx_zb_case(size), 0
    for size in be.TX_SLAB_BEGINS:
        yield be.comb_case(size, "random", second=size - 1), 0
    for size in be.TX_ZB_21:
        yield be.comb_case(size, "random"), 0
    for where in be.ROUND_WHERE:
        yield be.round_case(where)
    for size in be.TX_SLAB_LDS:
        yield be.twin_case(size), 0
    for which in be.ROBIN_NODES:
        yield be.robin_case(which), 100
    yield be.big_case(), 0
    parent, taxon, arrays, _ = be.chunk_forest()
    for n_trees in be.RS_TREES:
        yield se.Case(f"rs_chunk_{n_trees}", parent, taxon, se.subset(arrays, range(n_trees))), 0
    yield se.concordance_case(), 0
    parent, taxon, arrays, _, _ = se.refusal_tables("twice", 1)
    yield se.Case("refusal", parent, taxon, arrays, batches=(0, se.REFUSAL_BATCH)), 0


def test_the_python_plans_equal_the_librarys_on_every_case():
    n = 0
    for case, lds in _every_case():
        off = _starts(case)
        for export in EXPORTS:
            for bt in case.batches:
                _same_plan(off, case.s_leaves, bt, *be.export_extras(export, len(case.parent)), lds)
                n += 1
    assert n > 100
    off = np.concatenate([[0], np.cumsum([100_000, 3, 200_000, 1, 2, be.BT_CAP] * 40)])
    got = _same_plan(off, 300_000, 0, 40, 8)
    assert len(got["bstart"]) >= 5
    for export in EXPORTS:
        first = be.budget_first_split(export)
        for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
            got = _same_plan(3 * np.arange(m + 1), se.BUDGET_LEAVES, 0, *be.export_extras(export, 2 * se.BUDGET_LEAVES - 1))
            assert len(got["bstart"]) - 1 == batches and got["bstart"][1] == min(first - 1, m), (export, m)


def test_the_byte_budget_cases_split_where_they_say():
    firsts = {e: be.budget_first_split(e) for e in EXPORTS}
    assert firsts == {"score_branch_triplets": 4011, "score_taxon_triplets": 4010, "score_branch_resample": 237}
    nn = 2 * se.BUDGET_LEAVES - 1
    for e, first in firsts.items():
        need = se.per_tree(3, se.BUDGET_LEAVES, 2, *be.export_extras(e, nn))
        assert (first - 1) * need <= se.SC_BUDGET < first * need
    # the resample's 32 bytes a supertree node and tree decide its split, not the rows
    assert 32 * nn > 15 * 4 * se.BUDGET_LEAVES


# ------------------------------------------------------------------------------------------------ the references
def test_comb_closed_forms_equal_brute_force():
    rs = np.random.RandomState(1)
    for _ in range(300):
        m = int(rs.randint(3, 10))
        s_order, t_order = rs.permutation(m).astype(np.int32), rs.permutation(m).astype(np.int32)
        parent, taxon = se.supertree("caterpillar", s_order)
        arrays = br.forest(0, m, [("caterpillar", t_order)])
        sup, trees = se.to_node(parent, taxon), se.source_nodes(arrays)
        ref = btr.brute_force(sup, trees)
        got = be.comb_branches(s_order, t_order, m)
        for k in be.BRANCH:
            assert np.array_equal(got[k], ref[k]), (k, s_order, t_order)
        ref = be.taxon_reference(parent, taxon, arrays, brute=True)
        got = be.comb_taxa(s_order, t_order, m)
        for k in be.TAXON:
            assert np.array_equal(got[k], ref[k]), (k, s_order, t_order)


def test_weighted_after_is_the_weighted_dominance():
    rs = np.random.RandomState(0)
    for m in (1, 2, 3, 7, 64, 65, 100, 333):
        a, w = rs.permutation(m), rs.randint(0, 50, m)
        want = [int(w[i + 1:][a[i + 1:] > a[i]].sum()) for i in range(m)]
        assert be.weighted_after(a, w).tolist() == want


@pytest.mark.parametrize("kind", ["random", "blocks", "interleave"])
def test_closed_forms_and_the_array_reference_equal_node_sum_and_quadratic(kind):
    m = 301
    case = be.comb_case(m, kind, with_small=True, second=77)
    sup, trees = se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays)
    ref = btr.node_sum(sup, trees)
    got, arr = be.comb_case_reference(case, "branch"), be.branch_arrays(case.parent, case.taxon, case.arrays)
    for k in be.BRANCH:
        assert np.array_equal(got[k], ref[k]) and np.array_equal(arr[k], ref[k]), k
    assert ref["bt_concordant"].any() and ref["bt_alt1"].any() and ref["bt_alt2"].any()
    ref = be.taxon_reference(case.parent, case.taxon, case.arrays)
    got = be.comb_case_reference(case, "taxon")
    for k in be.TAXON:
        assert np.array_equal(got[k], ref[k]), k
    assert len(set(ref["tx_shared"].tolist())) > 50  # unlike the twin trees: the values differ from leaf to leaf
    # a mixed supertree with polytomies and unary nodes: the array reference is node_sum, per tree too
    mixed = be.words_case(257 + len(kind))
    sup, trees = se.to_node(mixed.parent, mixed.taxon), se.source_nodes(mixed.arrays)
    ref, arr = btr.node_sum(sup, trees), be.branch_arrays(mixed.parent, mixed.taxon, mixed.arrays)
    for k in be.BRANCH:
        assert np.array_equal(arr[k], ref[k]), k
    assert ref["bt_total"].any()
    each = be.branch_arrays(mixed.parent, mixed.taxon, mixed.arrays, per_tree=True)
    assert np.array_equal(each, rr.per_tree(sup, trees))


def test_three_leaf_closed_forms_equal_brute_force():
    rs = np.random.RandomState(2)
    seen = {k: 0 for k in (*be.BRANCH, "tx_shared")}
    for it in range(40):
        r = int(rs.randint(4, 12))
        s_order = rs.permutation(r).astype(np.int32)
        trees = se.budget_trees(25, r, seed=it)
        parent, taxon = se.supertree("caterpillar", s_order)
        arrays = br.forest(0, r, trees)
        sup, nodes = se.to_node(parent, taxon), se.source_nodes(arrays)
        got = be.three_leaf(s_order, trees, r)
        ref = btr.brute_force(sup, nodes)
        ref.update(be.taxon_reference(parent, taxon, arrays, brute=True))
        for k in (*be.BRANCH, *be.TAXON):
            assert np.array_equal(got[k], ref[k]), (k, it)
        for k in seen:
            seen[k] += int(ref[k].sum())
        w = rr.case_weights(rs, 25, 5)
        rows = rr.rows(w, rr.per_tree(sup, nodes))
        mine = be.three_leaf_rows(got, w, len(parent))
        assert np.array_equal(mine, rows.astype(np.int64))
        assert np.array_equal(be.wins(mine), rr.wins(rows)) and np.array_equal(be.wins(rows), rr.wins(rows))
    assert min(seen.values()) > 0, seen


# ------------------------------------------------------------------------------------------------ the cases
def test_wave_and_last_workgroup_cases():
    for end in se.WAVE_ENDS:
        case = be.wave_case(end)
        assert np.array_equal(case.sizes, se.wave_case(end).sizes) and _starts(case)[-1] % se.SC_THREADS == end
        sizes = case.sizes
        # trees under 96 leaves (the wave sums exceed their rows) beside trees of 256 and 257
        assert (sizes < 96).sum() >= 8 and sizes.max() == 257
        tips = case.taxon[case.taxon >= 0]
        assert sorted(tips.tolist()) == list(range(se.WAVE_TAXA + 11)) and case.arrays.taxon.max() < se.WAVE_TAXA
        qb = be.quartet_branches(case.parent)
        assert len(qb) > 150
        rec = be.record_counts(case.parent, case.taxon, case.arrays)
        assert (rec[sizes >= 61] > 0).all() and (rec[sizes <= 2] == 0).all()
        m = len(sizes)
        assert case.batches == (0, 1, 2, m - 1, m)
    case = be.last_workgroup_case()
    rec = be.record_counts(case.parent, case.taxon, case.arrays)
    assert rec.tolist() == list(be.LAST_RECORDS) == [1, 7, 8, 9, 15, 16, 17] and (case.sizes == rec + 2).all()
    assert be.bt_words_zb(int(case.sizes.max()))[1] == 8


def test_word_round_and_zb_cases_land_on_their_sides():
    assert be.WORD_SIZES == (2047, 2048, 2049, 4095, 4096, 4097) and be.ROUND_SIZES == (1023, 1024, 1025)
    assert [((n >> 5) + 1 - 1) // 64 for n in be.WORD_SIZES] == [0, 1, 1, 1, 2, 2]  # carries between 64-word steps
    for size in (*be.ROUND_SIZES, *be.WORD_SIZES):
        case = be.words_case(size)
        assert case.sizes.tolist() == [size, 3]
        assert be.record_counts(case.parent, case.taxon, case.arrays)[0] > 30
    for size, zb in zip((*be.BT_ZB_87, *be.BT_ZB_21), (8, 7, 2, 1)):
        case = be.comb_case(size, "random", with_small=True)
        assert case.sizes.tolist() == [2, 3, size, 33, 64] and case.note["large"][0][0] == 2
        p = be.branch_plan(_starts(case), size, 0, 40, 8)
        assert p["bt_zb"].tolist() == [zb] and p["bt_words"].tolist() == [(size >> 5) + 1]
        rec = be.record_counts(case.parent, case.taxon, case.arrays)
        assert rec[2] == size - 2  # every workgroup of the large tree is full but the last
        alone = be.branch_plan([0, size], size, 0, 40, 8)
        assert alone["bt_zb"].tolist() == [zb] and alone["bt_workgroups"].tolist() == [-(-(size - 2) // zb)]
    for size, zb in zip(be.BT_ZB_87, (8, 7)):
        case = be.zb_blocks_case(size)
        assert case.sizes.tolist() == [2, 3, size, 33, 64]
        assert be.branch_plan(_starts(case), size, 0, 40, 8)["bt_zb"].tolist() == [zb]
        qb = be.quartet_branches(case.parent)
        assert len(qb) == 30 and be.record_counts(case.parent, case.taxon, case.arrays)[2] == 30
        a, b, _ = be.restricted(case.parent, case.taxon, size, _tips(case, 2))
        assert (b - a)[qb[:, 1:]].min() > 150
    for size in be.BT_LDS:
        case = be.comb_case(size, "blocks")
        p = be.branch_plan([0, size], size, 0, 40, 8)
        assert case.sizes.tolist() == [size] and p["bt_zb"].tolist() == [1] and p["bt_workgroups"].tolist() == [size - 2]
        assert (p["bt_lds"][0] > 64 * KIB) == (size >= 87360)
    for size, zb in zip(be.TX_ZB_87, (8, 7)):
        case = be.tx_zb_case(size)
        assert be.branch_plan(_starts(case), size, 0, 72, 24)["tx_zb"][0, 0] == zb and case.sizes.tolist() == [size, 40]


def test_bin_cases_hold_needs_on_both_sides_of_every_used_bin():
    for n, dcaps in zip(be.BIN_SIZES, ([309, 320, 0], [215, 3220, 3328])):
        case = be.bin_case(n)
        plan = be.branch_plan(_starts(case), case.s_leaves, 0, 72, 24)
        assert plan["tx_dcap"].tolist() == [dcaps] and not plan["need_slab"]
        assert case.sizes.tolist() == [n, n, n]
        seen = set()
        for t in range(3):
            need = be.needs(case.parent, case.taxon, case.arrays.n_taxa, _tips(case, t))
            assert set(case.note["targets"][t]) <= set(need.tolist()), (n, t)
            assert need.max() == 2 * n + 1 and len(need) >= n - 4
            seen |= set(need.tolist())
            bins = {be.bin_of(int(x), dcaps) for x in need}
            assert bins == ({0, 1} if n == 159 else {0, 1, 2})
        for c in dcaps:
            if c and c + 1 <= 2 * n + 1:
                assert {c - 1, c, c + 1} <= seen, (n, c)
        assert n != 159 or {308, 309, 310, 319} <= seen


def test_round_slab_and_robin_cases():
    case, lds = be.round_case("slab")
    plan = be.branch_plan(_starts(case), case.s_leaves, 0, 72, 24, lds)
    need = np.concatenate([be.needs(case.parent, case.taxon, case.arrays.n_taxa, _tips(case, t)) for t in (0, 1)])
    assert lds == 100 and plan["tx_dcap"].tolist() == [[0, 0, 0]] and plan["tx_slab_launch"].tolist() == [1]
    assert set(be.ROUND_TOTALS) <= set(need.tolist())  # every node takes the slab, one at a time
    case, lds = be.round_case("lds")
    plan = be.branch_plan(_starts(case), case.s_leaves, 0, 72, 24, lds)
    need = be.needs(case.parent, case.taxon, case.arrays.n_taxa, _tips(case, 0))
    assert plan["tx_zb"][0, 0] == 1 and plan["tx_dcap"].tolist() == [[2061, 0, 0]] and plan["tx_slab_launch"][0] == 1
    assert set(be.ROUND_TOTALS) <= set(need[need <= 2061].tolist()) and (need > 2061).sum() == 2
    # without a cap: at 20 416 leaves bin 0 holds 2 046 entries with two nodes a workgroup and bin 1 is no larger, so
    # the totals 2 047 .. 2 049 are the first of bin 2 (one node a workgroup); 1 023 .. 1 025 cannot be there -- they
    # fit bin 0, which k_tx_single tries first -- and meet a workgroup of one node only where bin 0 itself has zb = 1,
    # from 26 624 leaves on
    assert be.ROUND_BIN2_LEAVES == 20416 == 32 * 638 and be.ROUND_BIN0_LEAVES == 26624 == be.TX_ZB_21[1]
    for where, zb, dcap, alone in (("bin2", [2, 2, 1], [2046, 0, 19194], be.ROUND_TOTALS[3:]),
                                   ("bin0", [1, 1, 1], [4982, 0, 18806], be.ROUND_TOTALS)):
        case, lds = be.round_case(where)
        plan = be.branch_plan(_starts(case), case.s_leaves, 0, 72, 24, lds)
        need = be.needs(case.parent, case.taxon, case.arrays.n_taxa, _tips(case, 0))
        assert lds == 0 and plan["tx_zb"].tolist() == [zb] and plan["tx_dcap"].tolist() == [dcap]
        assert plan["tx_slab_launch"].tolist() == [1] and (need > dcap[2]).sum() == 2
        one = [i for i in range(3) if zb[i] == 1 and dcap[i]]  # the bins of one node a workgroup
        assert set(be.ROUND_TOTALS) <= set(need.tolist())
        assert all(be.bin_of(x, dcap) == one[0] for x in alone)
        if where == "bin2":
            assert all(be.bin_of(x, dcap) == 0 for x in be.ROUND_TOTALS[:3])
            smaller = be.tx_plan_of((be.ROUND_BIN2_LEAVES - 1 >> 5) + 1)  # one word fewer: 2 047 and 2 048 still fit bin 0
            assert smaller["dcap"][0] == 2048 and smaller["zb"][0] == 2
    for size, slab_nodes in zip(be.TX_SLAB_BEGINS, (0, 1, 2)):
        case = be.comb_case(size, "random")
        plan = be.branch_plan([0, size], size, 0, 72, 24)
        need = be.needs(case.parent, case.taxon, size, _tips(case, 0))
        assert (need > plan["tx_dcap"][0].max()).sum() == slab_nodes
        assert plan["tx_slab_launch"].tolist() == [int(slab_nodes > 0)] and plan["slab_wgs"] == (256 if slab_nodes else 0)
        both = be.comb_case(size, "random", second=size - 1)
        assert both.sizes.tolist() == [size, size - 1]
    for which, total in zip(be.ROBIN_NODES, (255, 256, 257, 702)):
        case = be.robin_case(which)
        plan = be.branch_plan(_starts(case), case.s_leaves, 0, 72, 24, 100)
        assert plan["slab_wgs"] == 256 and plan["tx_dcap"].tolist() == [[0, 0, 0]]
        counts = [len(be.needs(case.parent, case.taxon, case.arrays.n_taxa, _tips(case, t)))
                  for t in range(case.arrays.n_trees)]
        assert sum(counts) == total and counts[1] == 0 and len(counts) >= 4


def test_twin_cases_are_uniform_and_reach_the_slab():
    case = be.twin_case(257)
    ref, want = be.taxon_reference(case.parent, case.taxon, case.arrays), be.twin_reference(257)
    assert all(np.array_equal(ref[k], want[k]) for k in be.TAXON)
    assert not np.array_equal(_tips(case, 0), case.taxon[case.taxon >= 0])  # the leaf orders differ
    for size in be.TX_SLAB_LDS:
        case = be.twin_case(size)
        plan = be.branch_plan([0, size], size, 0, 72, 24)
        need = be.needs(case.parent, case.taxon, size, _tips(case, 0))
        dcap = 12280 if size == 131071 else 12278  # bins 0 and 1 are out: bin 2 or the slab
        assert plan["tx_dcap"].tolist() == [[0, 0, dcap]] and plan["tx_slab_launch"].tolist() == [1]
        assert 2 <= (need > dcap).sum() < 1000 and len(need) == size - 2
        assert plan["tx_slab_lds"].tolist() == [65536 if size == 131071 else 65552]


def test_resample_cases():
    parent, taxon, arrays, each = be.chunk_forest()
    assert arrays.n_trees == 1025 and 3 <= arrays.leaf_counts().min() and arrays.leaf_counts().max() <= 12
    assert 200 < len(parent) < 400
    busy = each[:, 0, :].sum(axis=1) > 0
    assert busy[:511].any() and busy[512:].any() and busy[1024]  # the trees past the chunk count
    for n_trees in be.RS_TREES:
        for n_rep in be.RS_REPS:
            w = be.chunk_weights(n_rep, n_trees)
            assert w[:, :512].max() < 4 and (n_trees <= 512 or w[:, 512:].min() >= 1000)
            rows = be.weighted_rows(w, each[:n_trees])
            if n_trees == 513 and n_rep == 9:  # the numpy restatements the GPU cases use are the references' own
                ref = rr.rows(w, each[:n_trees].astype(object))
                assert np.array_equal(rows, ref.astype(np.int64)) and np.array_equal(be.wins(rows), rr.wins(ref))
                assert be.wins(rows)[:3].any() and be.wins(rows)[3].any()
        plan = be.branch_plan(3 * np.arange(n_trees + 1), be.RS_TAXA, 0, *be.export_extras(
            "score_branch_resample", len(parent)))
        assert len(plan["bstart"]) == 2  # one batch
    assert [n % be.RS_AHEAD for n in (511, 512, 513, 1025 - 512)] == [3, 0, 1, 1]
    case = be.big_case()
    each = be.branch_arrays(case.parent, case.taxon, case.arrays, per_tree=True)
    assert case.sizes.tolist() == [3 * be.BIG_BLOCK] and be.BIG_BLOCK >= 1626
    assert each[0, 0, 1] == be.BIG_BLOCK ** 3 >= 2 ** 32 and each[0, 1, 1] >= 2 ** 32
    assert each[0, 2, 1] > 0 and each[0, 3, 1] > 0 and np.count_nonzero(each) == 4
    w = be.big_weights(3 * be.BIG_BLOCK)
    cube = (3 * be.BIG_BLOCK) ** 3 // 27
    assert w[:3] == [0, 1, 2 ** 30 + 12345] and w[3] * cube <= 2 ** 63 - 1 < (w[3] + 1) * cube and w[3] < 2 ** 31


# ------------------------------------------------------------------------------------------------ the entry
def test_the_branch_plan_entry_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(r"int scs_debug_branch_plan\(([^)]*)\)", text)
    assert m, "include/scs_hip.h does not declare scs_debug_branch_plan"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES["scs_debug_branch_plan"]
    assert restype is nv.C.c_int and len(argtypes) == len(params) == 13
    assert params[0] == "const scs_tables *sources" and params[7] == "int32_t max_lds_bytes"
    lib = nv.load_library()
    assert hasattr(lib, "scs_debug_branch_plan") and lib.scs_version() == nv.ABI_VERSION == 109
    assert lib.scs_debug_branch_plan(None, 0, None, 1, 0, 0, 0, 0, None, None, None, None, None) == nv.EINVAL
