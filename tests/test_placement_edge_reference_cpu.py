"""No device: the array references of ``tests/placement_edge_reference.py`` equal the project's brute-force and set
references where those can go, the plans of the placement, clade and polytomy kernels restated in Python equal the
library's own (``scs_debug_placement_plan``), every case of ``tests/test_gpu_placement_polytomy_edges.py`` has the
numbers it is named for, and the new entry is declared, bound and exported."""

import re
from pathlib import Path

import build_reference as br
import clade_placement_reference as cr
import numpy as np
import placement_edge_reference as pe
import placement_reference as pr
import polytomy_reference as yr
import pytest
import score_edge_reference as se

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend
from spectralclustersupertree_amd.treearrays import TreeArrays

ROOT = Path(__file__).resolve().parent.parent
KIB = 1024


# ------------------------------------------------------------------------------------------------ the references
def _mixed_tree(rs, ids):
    par, leaf = se.mixed_shape(len(ids), rs, polytomy=0.4, unary=0.15)
    tax = np.full(len(par), -1, dtype=np.int32)
    tax[leaf] = ids
    return par, tax


def _random_case(rs, n: int, n_sources: int):
    """A mixed supertree on ``n`` taxa and sources on random subsets of 1 .. n of them, with polytomies and unary
    nodes on both sides; ``n_taxa`` names, so that the supertree's ids are all there."""
    nm = se.names(n)
    parent, taxon = _mixed_tree(rs, rs.permutation(n).astype(np.int32))
    trees = []
    for i in range(n_sources):
        k = n if i == 0 else int(rs.randint(1, n + 1))
        par, tax = _mixed_tree(rs, rs.permutation(n)[:k].astype(np.int32))
        flat = ([int(p) for p in par], [nm[x] if x >= 0 else None for x in tax], [None] * len(par), [None] * len(par))
        trees.append(se.TreeNode.from_flat(flat))
    sup = se.TreeNode.from_flat(([int(p) for p in parent], [nm[x] if x >= 0 else None for x in taxon],
                                 [None] * len(parent), [None] * len(parent)))
    return parent, taxon, sup, trees, TreeArrays.from_trees(trees, [1.0] * len(trees), nm)


def _polytomies_of(parent) -> list[int]:
    kids = np.bincount(np.asarray(parent)[1:], minlength=len(parent))
    return [int(v) for v in np.flatnonzero((kids >= 3) & (kids <= pe.PY_KMAX))]


def _check_placements(parent, taxon, sup, trees, arrays, queries, judge) -> dict:
    nm = se.names(arrays.n_taxa)
    ref = judge(sup, trees, [nm[x] for x in queries])
    got = pe.placement_arrays(parent, taxon, arrays, queries)
    for k in pe.PLACEMENTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    return got


def _check_polytomies(parent, taxon, sup, trees, arrays, judge) -> dict | None:
    nodes = _polytomies_of(parent)
    if not nodes:
        return None
    ref = judge(sup, trees, only=nodes)
    got = pe.polytomy_arrays(parent, taxon, arrays, nodes)
    assert got["py_degree"].tolist() == ref["degree"].tolist() and np.array_equal(got["py_trees"], ref["trees"])
    for a, b in zip(got["py_total"] + got["py_joint"], ref["total"] + ref["joint"]):
        assert a.dtype == np.int64 and np.array_equal(a, b)
    return got


def test_the_array_references_equal_brute_force_on_small_cases():
    rs = np.random.RandomState(31)
    held = absent = decisive = 0
    for it in range(300):
        n = int(rs.randint(3, 10))
        parent, taxon, sup, trees, arrays = _random_case(rs, n, int(rs.randint(1, 5)))
        tips = taxon[taxon >= 0]
        _, t_tax = arrays.parent[: arrays.node_off[1]], arrays.taxon[: arrays.node_off[1]]
        t_tips = t_tax[t_tax >= 0]
        # the tips at S position 0 and n - 1, the first and the last leaf of the first source, and some more
        queries = list(dict.fromkeys([int(tips[0]), int(tips[-1]), int(t_tips[0]), int(t_tips[-1]),
                                      *[int(x) for x in rs.permutation(n)[: it % 4]]]))
        got = _check_placements(parent, taxon, sup, trees, arrays, queries, pr.brute_force)
        held += int((got["pl_trees"] > 0).sum())
        absent += int((got["pl_trees"] < len(trees)).sum())
        py = _check_polytomies(parent, taxon, sup, trees, arrays, yr.brute_force)
        decisive += int(py["py_trees"].sum()) if py else 0
    assert held > 1000 and absent > 300 and decisive > 100


def _same_clades(got: dict, ref: dict) -> None:
    for k in pe.CLADES:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])


def test_clade_arrays_equal_brute_force_on_small_cases_and_composed_on_larger_ones():
    rs = np.random.RandomState(23)
    crossed = 0
    for _ in range(200):
        n = int(rs.randint(3, 10))
        parent, taxon, sup, trees, arrays = _random_case(rs, n, int(rs.randint(1, 4)))
        tip_node = np.flatnonzero(taxon >= 0)
        # the first and the last tip of S and three more nodes
        qs = list(dict.fromkeys([int(tip_node[0]), int(tip_node[-1]),
                                 *[int(v) for v in rs.permutation(np.arange(1, len(parent)))[:3]]]))
        ref = cr.brute_force(sup, trees, qs)
        _same_clades(pe.clade_arrays(parent, taxon, arrays, qs), ref)
        crossed += int(ref["cp_trees"].sum())
    assert crossed > 800
    for n in (77, 301):
        parent, taxon, sup, trees, arrays = _random_case(rs, n, 3)
        lo, hi, _ = pe.preorder_tables(parent, taxon)
        inner = np.flatnonzero((taxon < 0) & (np.arange(len(parent)) > 0) & (hi - lo <= 30))
        qs = [int(inner[0]), int(inner[len(inner) // 2]), int(inner[-1]), int(np.flatnonzero(taxon >= 0)[0])]
        _same_clades(pe.clade_arrays(parent, taxon, arrays, qs), cr.composed(sup, trees, qs))


def test_the_three_leaf_polytomy_form_equals_the_array_reference():
    parent, taxon = pe.grid_supertree()
    orders, cat = pe.grid_sources()
    which = [*range(400), pe.PY_GRID_Y - 1, pe.PY_GRID_Y, pe.PY_GRID_Y + 1]
    arrays = br.forest(1, pe.GRID_TAXA, pe.grid_trees(which))
    want = pe.polytomy_arrays(parent, taxon, arrays, [0, 1])
    got = pe.three_leaf_polytomies(parent, taxon, [0, 1], orders[which], cat[which])
    assert got["py_degree"].tolist() == [3, 4] and np.array_equal(got["py_trees"], want["py_trees"]) and want["py_trees"].min() > 20
    assert all(np.array_equal(a, b) for a, b in zip(got["py_total"] + got["py_joint"], want["py_total"] + want["py_joint"]))
    tabs, flat = pe.grid_tables(400), arrays.flatten("one")
    assert np.array_equal(tabs.leaf_taxon, flat.leaf_taxon[:1200]) and np.array_equal(tabs.adj_depth, flat.adj_depth[:1200])
    # tree counts around a grid row; the trees of the second launch have the other shape than the first ones
    assert pe.GRID_COUNTS == (65535, 65536, 65537) and len(cat) == 65537
    assert cat[65535] != cat[0] and cat[65536] != cat[1]
    last = pe.three_leaf_polytomies(parent, taxon, [0, 1], orders[65535:], cat[65535:])
    assert last["py_trees"].tolist() == [1, 1]  # tree 65 535 is decisive at the root, tree 65 536 at the polytomy
    for count in pe.GRID_COUNTS:  # one batch each
        got = _same_plan(3 * np.arange(count + 1), pe.GRID_TAXA, degrees=(3, 4))
        assert got["py_bstart"].tolist() == [0, count]


def test_a_query_that_no_tree_holds_and_trees_that_hold_no_query():
    rs = np.random.RandomState(5)
    nm = se.names(9)
    parent, taxon = _mixed_tree(rs, rs.permutation(9).astype(np.int32))
    sup = se.to_node(parent, taxon)
    trees = [se.to_node(*_mixed_tree(rs, np.asarray(ids, dtype=np.int32))) for ids in
             ([0, 1, 2, 3], [4, 5, 6], [0, 4], [7], [1, 2, 3, 4, 5, 6, 7])]
    arrays = TreeArrays.from_trees(trees, [1.0] * len(trees), nm)
    got = _check_placements(parent, taxon, sup, trees, arrays, [8, 0, 7], pr.brute_force)
    assert got["pl_trees"].tolist() == [0, 1, 1] and not got["pl_super"][0].any()


@pytest.mark.parametrize("n", [77, 301])
def test_the_array_references_equal_the_set_references_at_77_and_301_leaves(n):
    rs = np.random.RandomState(n)
    for _ in range(2):
        parent, taxon, sup, trees, arrays = _random_case(rs, n, 4)
        tips = taxon[taxon >= 0]
        queries = [int(tips[0]), int(tips[-1]), *[int(x) for x in rs.permutation(tips[1:-1])[:4]]]
        got = _check_placements(parent, taxon, sup, trees, arrays, queries, pr.recurrence)
        assert got["pl_shared"].any()
        assert _check_polytomies(parent, taxon, sup, trees, arrays, yr.node_sum) is not None


# ------------------------------------------------------------------------------------------------ the plans
def test_the_steps_of_the_pair_plan_sit_at_their_sizes():
    first = pe.first_leaves
    # zb: the rows of k_trip_pairs; the sums of even 64 queries stay far below the cap at these sizes
    assert first(lambda n: pe.pair_plan(n, 64)[1] <= 7) == 10240 and first(lambda n: pe.pair_plan(n, 64)[1] <= 1) == 40960
    assert [pe.pair_plan(n, q) for n in (10239, 10240, 40959, 40960) for q in (1, 64)] == [
        (320, 8, 1), (320, 8, 1), (321, 7, 1), (321, 7, 1), (1280, 2, 1), (1280, 2, 1), (1281, 1, 1), (1281, 1, 1)]
    assert pe.ZB_87 == (10239, 10240) and pe.ZB_21 == (40959, 40960)
    # the sums leave LDS by themselves where 16 W + node + pass bytes pass 160 KiB
    assert pe.node_bytes(64) == 1056 and pe.pass_bytes(64) == 272 and pe.node_bytes(1) == 48 and pe.pass_bytes(1) == 16
    assert first(lambda n: pe.pair_plan(n, 64)[2] == 0) == 325024 and first(lambda n: pe.pair_plan(n, 1)[2] == 0) == 327552
    assert pe.pair_plan(pe.PL_CAP, 1) == (10240, 1, 0) and pe.PL_CAP == 327679
    # the launch passes 64 KiB (one query, zb = 1) from 130 944 leaves on
    lds = lambda n: pe.pair_lds(*pe.pair_plan(n, 1), 1)  # noqa: E731
    assert lds(130943) == 64 * KIB and lds(130944) == 64 * KIB + 16 and first(lambda n: lds(n) > 64 * KIB, 40960) == 130944
    # the pad of pref: 4 ((qc + 4) & ~3) bytes for the last passes of 1 .. 5 queries and a full one
    assert [pe.pass_bytes(q) for q in (1, 2, 3, 4, 5, 64)] == [16, 16, 16, 32, 32, 272]
    # under a cap: CAP_LEAVES leaves, CAP_QUERIES queries
    assert (pe.CAP_LEAVES >> 5) + 1 == 10 and pe.node_bytes(pe.CAP_QUERIES) == 96 and pe.pass_bytes(pe.CAP_QUERIES) == 32
    assert [pe.pair_plan(pe.CAP_LEAVES, pe.CAP_QUERIES, pe.lds_cap(c))[1:] for c in pe.CAP_BYTES] == [
        (1, 0), (1, 1), (1, 1), (2, 1), (7, 1), (8, 1), (8, 1)]


def test_the_steps_of_the_polytomy_plan_sit_at_their_sizes():
    # (W, Ws, acc_lds, bytes).  k = 64: the launch passes 64 KiB at 2 016 | 2 017 leaves (not at 4 096 | 4 097, where
    # the rows alone do); the stride goes odd -> even at 8 160 | 8 161 with the sums still in LDS; the sums leave at
    # 8 192 | 8 193; 10 240 is the last size, 10 241 is refused
    assert [pe.py_plan(n, 64) for n in pe.PY_WIDE] == [
        (63, 63, 1, 65024), (64, 65, 1, 66048), (128, 129, 1, 98816), (129, 129, 1, 98816), (255, 255, 1, 163328), (256, 256, 1, 163840),
        (256, 256, 1, 163840), (257, 257, 0, 131584), (320, 320, 0, 163840), (320, 320, 0, 163840)]
    assert pe.py_plan(10241, 64)[3] == 164352 > se.TP_LDS_MAX
    assert [pe.py_plan(n, 3) for n in pe.PY_THREE] == [(64, 65, 1, 1632), (64, 65, 1, 1632), (65, 65, 1, 1632),
                                                       (2727, 2727, 1, 65520), (2728, 2729, 1, 65568),
                                                       (6826, 6826, 0, 163824)]
    assert pe.PY_LIMIT_3 == 218432 and pe.py_plan(pe.PY_LIMIT_3 + 1, 3)[3] > se.TP_LDS_MAX
    # rows of ceil(n / 32) words: 32 k - 1, 32 k and 32 k + 1 leaves are all there
    sizes = (*pe.PY_WIDE, *pe.PY_THREE)
    assert {n % 32 for n in sizes} >= {31, 0, 1}


def _same_plan(off, s_leaves, **kw) -> dict:
    want = pe.placement_plan(off, s_leaves, **kw)
    got = backend.debug_placement_plan(np.asarray(off, dtype=np.int64), s_leaves, **kw)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, kw, got[k], want[k])
    return got


def test_the_python_plans_equal_the_librarys_for_every_row_width():
    """One tree of every width from 1 to 10 240 words, a batch each (``batch_trees`` = 1)."""
    off = np.concatenate([[0], np.cumsum(32 * np.arange(1, 10241) - 1)])
    for lds in (0, 287, 544, 2080, 64 * KIB):
        for nq, ns in ((1, 5), (pe.CAP_QUERIES, 64), (129, 65)):
            got = _same_plan(off, 1000, batch_trees=1, lds_bytes=lds, n_queries=nq, n_sub_queries=ns, degrees=(3, 7, 64))
            assert got["pl_words"].tolist() == list(range(1, 10241)) and got["py_words"][:, 0].tolist() == list(range(1, 10241))
    # and the neighbours of a multiple of 32
    off = np.concatenate([[0], np.cumsum([n + d for n in (32, 2048, 8160, 8192, 10240) for d in (-1, 0, 1)])])
    _same_plan(off, 1000, batch_trees=1, n_queries=3, n_sub_queries=70, degrees=(64, 3))


def _counts(case: se.Case) -> dict:
    note = case.note
    lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
    kids = np.bincount(np.asarray(case.parent)[1:], minlength=len(case.parent))
    return {"n_queries": max(len(note.get("queries", ())), 1),
            "n_sub_queries": int(sum(hi[q] - lo[q] for q in note.get("clades", ()))) or 1,
            "degrees": [int(kids[q]) for q in note.get("polytomies", ())]}


def _every_case():
    for end in se.WAVE_ENDS:
        yield pe.wave_case(end)
    yield pe.last_workgroup_case()
    for size in pe.WORD_SIZES:
        yield pe.words_case(size)
    for size in (*pe.ZB_87, *pe.ZB_21):
        yield pe.zb_case(size, True)
    yield pe.cap_case()
    yield pe.pass_case()
    yield pe.common_case()
    yield pe.lists_case()
    for count in pe.NODE_COUNTS:
        yield pe.nodes_case(count)
    for which in pe.CLADE_PASSES:
        yield pe.clade_pass_case(which)
    for n in (*pe.MASK_SIZES, pe.MASK_LARGE):
        yield pe.mask_case(n)
    for k in pe.COLOUR_DEGREES:
        yield pe.colour_case(k)
    yield pe.clade_words_case()
    yield pe.py_case(8161, 64)
    yield pe.py_case(2049, 3)
    yield pe.big_polytomy_case()


def test_the_plans_agree_on_the_forest_of_every_case():
    n = 0
    for case in _every_case():
        off = np.concatenate([[0], np.cumsum(case.sizes)])
        for bt in case.batches:
            for lds in ((0, *pe.CAP_BYTES) if case.name == "pl_cap" else (0,)):
                _same_plan(off, case.s_leaves, batch_trees=bt, lds_bytes=lds, **_counts(case))
                n += 1
    assert n > 70


# ------------------------------------------------------------------------------------------------ the cases
def test_wave_cases_hold_queries_at_both_ends_and_clades_of_every_kind():
    for end in se.WAVE_ENDS:
        case = pe.wave_case(end)
        tips, q = pe.s_tips(case), case.note["queries"]
        assert case.s_leaves == se.WAVE_TAXA + 11 and len(case.note["absent"]) == 11
        assert q[0] == tips[0] and q[1] == tips[-1] and np.isin(q, case.note["absent"]).sum() == 2 and len(set(q)) == 9
        off = np.concatenate([[0], np.cumsum(case.sizes)])
        assert int(off[-1]) % 256 == end and (np.diff(off) < 3).sum() >= 7 and (off[:-1] % 32 != 0).sum() > 10
        lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
        sizes = sorted(int(hi[v] - lo[v]) for v in case.note["clades"])
        assert sizes[0] == 1 and sizes[-1] >= 40 and 0 not in case.note["clades"] and len(case.note["polytomies"]) == 3


def test_the_last_workgroup_case_has_its_node_counts():
    case = pe.last_workgroup_case()
    z = pe.zcounts(case.parent, case.taxon, case.arrays)
    assert z.tolist() == [6, *pe.LAST_NODES, 0, 18] and pe.LAST_NODES == (7, 8, 9, 15, 16, 17, 23, 24, 25)
    assert pe.pair_plan(int(case.sizes.max()), 4)[1] == 8
    wgs = [-(-2 * int(n) // 8) if n >= 3 else 0 for n in case.sizes]
    # nz = min(zb, zcnt - j0): the last workgroup that finds a node finds one, zb - 1 or zb; later ones find none
    last = {(int(c) - 1) % 8 + 1 for c, w in zip(z, wgs) if w}
    slack = [8 * w - int(c) for c, w in zip(z, wgs) if w]
    assert {1, 7, 8} <= last and max(slack) >= 8 and min(slack) < 8


def test_word_and_zb_cases_have_their_widths():
    for size in pe.WORD_SIZES:
        case = pe.words_case(size)
        assert case.sizes.tolist() == [size, 3] and len(case.note["queries"]) == 3
        lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
        assert max(int(hi[v] - lo[v]) for v in case.note["polytomies"]) > size // 4  # colours spread over all of T's words
    assert [(n >> 5) + 1 for n in pe.WORD_SIZES] == [64, 65, 65, 128, 129, 129]
    for size, zb in zip((*pe.ZB_87, *pe.ZB_21), (8, 7, 2, 1)):
        case = pe.zb_case(size, True)
        assert case.sizes.tolist() == [2, 3, size, 33, 64] and case.note["large"] == 2
        assert pe.pair_plan(size, len(case.note["queries"]))[1:] == (zb, 1)


def test_pass_cases_have_their_query_counts():
    assert pe.LAST_PASS == (64, 65, 66, 67, 68, 69, 128, 129)
    assert [q - (q - 1) // 64 * 64 for q in pe.LAST_PASS] == [64, 1, 2, 3, 4, 5, 64, 1]
    case = pe.pass_case()
    assert len(set(case.note["queries"].tolist())) == 129 and case.s_leaves == pe.PASS_TAXA
    case = pe.common_case()
    q = case.note["queries"]
    assert len(q) == pe.COMMON_QUERIES == 129 and q.tolist() == list(range(129))
    held = pe.queries_held(case.arrays, q)
    assert held.tolist() == [[64, 0, 1], [63, 0, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0], [0, 64, 1], [0, 63, 1], [0, 1, 1],
                             [0, 0, 1], [64, 64, 1]]


def test_node_count_and_list_cases():
    for count in pe.NODE_COUNTS:
        case = pe.nodes_case(count)
        assert len(case.parent) == count and len(case.note["clades"]) == 2
    case = pe.lists_case()
    assert case.sizes.tolist() == [pe.COMB_LEAVES, pe.COMB_LEAVES, 5]
    t_par, t_tax = case.arrays.parent[: case.arrays.node_off[1]], case.arrays.taxon[: case.arrays.node_off[1]]
    tips = t_tax[t_tax >= 0]
    depth = np.zeros(len(t_par), dtype=np.int64)
    for v in range(1, len(t_par)):
        depth[v] = depth[t_par[v]] + 1
    tip_depth = depth[t_tax >= 0]
    q = case.note["queries"]
    assert q[0] == tips[0] and tip_depth[0] == pe.COMB_LEAVES - 1  # the deepest tip: m - 1 groups of one leaf
    assert q[1] == tips[-1] and tip_depth[-1] == 1  # the shallowest: one group of m - 1 leaves


def test_clade_cases_have_their_passes():
    want = {"64_5": [(64, 1, 0), (5, 1, 0)], "63_2": [(64, 2, 0), (1, 1, 1)], "65": [(64, 1, 0), (1, 1, 1)],
            "128": [(64, 1, 0), (64, 1, 1)], "129": [(64, 1, 0), (64, 1, 1), (1, 1, 1)], "ones": [(64, 64, 0), (3, 1, 0)]}
    assert sorted(want) == sorted(pe.CLADE_PASSES)
    for which, passes in want.items():
        case = pe.clade_pass_case(which)
        assert pe.clade_passes(case.parent, case.taxon, case.note["clades"]) == passes, which
    # (qc, ncl, skip0): a pass with ncl == skip0 holds only the tail of a clade, and k_cp_nodes is not launched
    assert sum(ncl == skip for p in want.values() for _, ncl, skip in p) == 5
    for n in pe.MASK_SIZES:
        case = pe.mask_case(n)
        lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
        sizes = sorted({int(hi[v] - lo[v]) for v in case.note["clades"]})
        assert sizes[0] == 1 and sizes[-1] == n - 1 and 2 in sizes and case.sizes.tolist()[0] == n
    # the masks: |Q' ∩ L| = 0, 1, n - 1, n, Q' at the first and at the last leaves of S', z = Q', z inside Q', z ⊋ Q' by
    # one leaf -- all of them from 4 tips on and in the large case; with 3 tips every source holds all of S
    every = {"none", "one", "all_but_one", "all", "first", "last", "z_equal", "z_inside", "z_one_more"}
    assert pe.mask_relations(pe.mask_case(3)) == every - {"none", "all", "z_inside"}
    for n in (*pe.MASK_SIZES[1:], pe.MASK_LARGE):
        assert pe.mask_relations(pe.mask_case(n)) == every, n
    # ... and on a source of exactly three leaves (the fourth tree of [4]): |Q'| = 0, 1, 2, 3
    case = pe.mask_case(4)
    assert case.sizes[3] == 3
    t_tax = case.arrays.taxon[case.arrays.node_off[3]:case.arrays.node_off[4]]
    lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
    held = {int(np.isin(pe.s_tips(case)[lo[q]:hi[q]], t_tax).sum()) for q in case.note["clades"]}
    assert held == {0, 1, 2, 3}
    case = pe.mask_case(pe.MASK_LARGE)
    assert case.sizes.tolist() == [2100, 41, 40, 2060, 3, 39, 2099] and pe.MASK_TIPS == 40


def test_the_clade_case_past_64_words_has_tips_on_both_sides():
    case = pe.clade_words_case()
    assert case.sizes.tolist() == [pe.CLADE_WORDS, 3] and (pe.CLADE_WORDS >> 5) + 1 == 66
    lo, hi, _ = pe.preorder_tables(case.parent, case.taxon)
    t_tax = case.arrays.taxon[: case.arrays.node_off[1]]
    t_pos = np.full(case.arrays.n_taxa, -1, dtype=np.int64)
    t_pos[t_tax[t_tax >= 0]] = np.arange(pe.CLADE_WORDS)
    words = [sorted(set((t_pos[pe.s_tips(case)[lo[v]:hi[v]]] >> 5).tolist())) for v in case.note["clades"]]
    assert all(4 <= hi[v] - lo[v] <= 60 for v in case.note["clades"])
    assert sum(min(ws) < 64 <= max(ws) for ws in words) >= 2  # Q' on both sides of word 63 | 64


def test_polytomy_cases_have_their_colours():
    for k in pe.COLOUR_DEGREES:
        case = pe.colour_case(k)
        ref = pe.polytomy_arrays(case.parent, case.taxon, case.arrays, [0])
        assert ref["py_degree"].tolist() == [k] and 1 in case.sizes and 2 in case.sizes
        assert ref["py_trees"][0] == (5 if k == 3 else 8)
    case = pe.big_polytomy_case()
    ref = pe.polytomy_arrays(case.parent, case.taxon, case.arrays, [0])
    assert int(ref["py_total"][0][0, 1, 2]) == pe.BIG_BLOCK ** 3 == 4362708104 > 2 ** 32
    assert 2 ** 32 < int(ref["py_joint"][0][0, 1, 2]) < pe.BIG_BLOCK ** 3
    case = pe.py_case(8161, 64)
    assert case.sizes.tolist() == [8161, 5] and case.note["polytomies"][0] == 0


def test_large_cases_sit_on_both_sides_of_their_gates():
    assert pe.LDS_64K == (130943, 130944) and pe.NO_SUMS_1 == (327551, 327552) and pe.NO_SUMS_64 == (325023, 325024)
    assert [pe.pair_plan(n, 1) for n in (*pe.LDS_64K, *pe.NO_SUMS_1)] == [(4092, 1, 1), (4093, 1, 1), (10236, 1, 1),
                                                                            (10237, 1, 0)]
    assert [pe.pair_plan(n, 64)[1:] for n in pe.NO_SUMS_64] == [(1, 1), (1, 0)] and pe.pair_plan(pe.PL_CAP, 2) == (10240, 1, 0)
    case = pe.large_case(pe.LDS_64K[1], 1)
    off = np.concatenate([[0], np.cumsum(case.sizes)])
    got = _same_plan(off, case.s_leaves, **_counts(case))
    assert case.sizes.tolist() == [130944, 5] and got["pl_lds_full"].tolist() == [64 * KIB + 16]
    assert len(case.parent) == 130944 + 2047  # the rows of 64 queries fit the workspace: 3 x 2 x 64 x nodes x 8 bytes
    assert 3 * 2 * 64 * 8 * (pe.NO_SUMS_64[1] + 2048) < se.SC_BUDGET < 3 * 2 * 64 * 8 * 2 * pe.NO_SUMS_64[1]
    assert (pe.BIG_TWIN - 1) * (pe.BIG_TWIN - 2) // 2 == 5000150001 > 2 ** 32


def test_the_byte_budget_cases_split_where_each_export_says():
    assert [pe.budget_first_split(e) for e in pe.BUDGET_EXPORTS] == [4008, 4007, 4011]
    decisive = []
    for export, name in zip(pe.BUDGET_EXPORTS, ("pl", "cp", "py")):
        first = pe.budget_first_split(export)
        for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
            case = pe.budget_case(export, m)
            tabs, flat = case.note["tables"], case.arrays.flatten("one")
            assert np.array_equal(tabs.leaf_taxon, flat.leaf_taxon) and np.array_equal(tabs.adj_depth, flat.adj_depth)
            got = _same_plan(tabs.tree_off, se.BUDGET_LEAVES, **_counts(case))
            assert len(got[f"{name}_bstart"]) - 1 == batches and (batches == 1 or got[f"{name}_bstart"][1] == first - 1)
            if export == "score_polytomies":
                decisive.append(int(pe.polytomy_arrays(case.parent, case.taxon, case.arrays, [0])["py_trees"][0]))
    assert decisive[1] == decisive[0] + 1 and decisive[2] == decisive[1] + 1  # the trees of the second batch count


def test_refusal_case_has_queries_for_all_four_exports():
    parent, taxon, _, _, _ = se.refusal_tables("twice", 1)
    note = pe.refusal_queries(parent, taxon)
    assert len(note["queries"]) == 3 and len(note["clades"]) == 2 and len(note["polytomies"]) == 2


# ------------------------------------------------------------------------------------------------ the entry
def test_the_entry_is_declared_bound_and_exported():
    text = (ROOT / "include" / "scs_hip.h").read_text()
    m = re.search(r"int scs_debug_placement_plan\(([^)]*)\)", text)
    assert m, "include/scs_hip.h does not declare scs_debug_placement_plan"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    restype, argtypes = nv.SIGNATURES["scs_debug_placement_plan"]
    assert n_args == len(argtypes) == 16
    lib = nv.load_library()
    assert hasattr(lib, "scs_debug_placement_plan") and lib.scs_version() == nv.ABI_VERSION == 109
    assert lib.scs_debug_placement_plan(None, 0, None, 1, 0, 0, 1, 1, 0, None, None, None, None, None, None, None) == nv.EINVAL
    with pytest.raises(nv.ScsError, match="degree 2 is not in"):
        backend.debug_placement_plan(np.asarray([0, 5], dtype=np.int64), 5, degrees=[2])
