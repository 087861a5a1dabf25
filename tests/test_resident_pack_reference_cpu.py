"""``tests/resident_pack_reference.py`` held to the host path and to its own numbers (no device): the reference's
arrays for a node are what ``child.flatten(strategy, local_ids=present)`` + ``scs.prepare_node`` give for that node,
every case sits on the edge its name says, and a pack with one of four plausible errors differs from the reference --
the comparison of ``tests/test_gpu_resident_pack_edges.py`` can fail.  DESIGN.md section 37."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

from spectralclustersupertree_amd import _native, scs
from tests import resident_pack_reference as rp


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want) -> bool:
    """Five packed arrays, bit for bit."""
    return (all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got[:3], want[:3]))
            and np.array_equal(_bits(got[3]), _bits(want[3])) and np.array_equal(_bits(got[4]), _bits(want[4])))


# ------------------------------------------------------------------------------------- against the host path
@pytest.mark.parametrize("name", ["9 nodes", "mixed sizes", "7 nodes depth", "7 nodes one", "subset permuted",
                                  "a node's first offset in slot 256"])
def test_the_reference_equals_the_host_path_node_by_node(name):
    case = rp.level_case(name)
    inp = case.inputs()
    sets = [np.arange(lo, lo + sz, dtype=np.int32) for lo, sz in zip(case.u_lo, case.u_sz)]
    children = case.level.split(sets)
    contracted = 0
    for i, k in enumerate(case.batch):
        child = children[k]
        assert child.n_trees == int(case.t_hi[k] - case.t_lo[k])  # the node's trees and no other
        tables = child.flatten(case.strategy, local_ids=child.present_taxa())
        work, perm, group_start, n_groups = scs.prepare_node(tables, case.kinds[k] == "groups")
        got, gs = inp["host_nodes"][i]
        assert got.n_taxa == work.n_taxa == int(inp["n_taxa"][i]) and n_groups == int(inp["n_groups"][i])
        assert np.array_equal(got.tree_off, work.tree_off) and np.array_equal(got.leaf_taxon, work.leaf_taxon)
        assert np.array_equal(got.adj_depth, work.adj_depth)
        assert np.array_equal(_bits(got.adj_val), _bits(work.adj_val)) and np.array_equal(_bits(got.tree_w), _bits(work.tree_w))
        if group_start is None:
            assert gs is None or np.array_equal(gs, np.arange(work.n_taxa + 1))
        else:
            assert np.array_equal(gs, group_start)
            contracted += 1
        at = int(np.cumsum(inp["n_groups"] + 1)[i] - inp["n_groups"][i] - 1)
        want_gs = np.arange(work.n_taxa + 1) if group_start is None else group_start
        assert np.array_equal(inp["group_start"][at:at + n_groups + 1], want_gs)
    if "groups" in [case.kinds[k] for k in case.batch]:
        assert contracted >= 1  # (taxa really contract somewhere: the third kind of relabel is not the second)


def test_an_identity_split_of_a_level_keeps_it_and_its_tables():
    """The GPU file makes a level resident through a split that keeps everything: on the host that split changes
    nothing, so the level's own ``flatten`` is what the device must hold."""
    for name in ("9 nodes", "tie of 128 nodes", "mixed sizes"):
        case = rp.level_case(name)
        level = case.level
        kid = level.split([np.arange(level.n_taxa, dtype=np.int32)])[0]
        assert np.array_equal(kid.node_off, level.node_off) and np.array_equal(kid.parent, level.parent)
        assert np.array_equal(kid.taxon, level.taxon) and np.array_equal(_bits(kid.weights), _bits(level.weights))
        a, b = kid.flatten(case.strategy), case.tables
        assert np.array_equal(a.tree_off, b.tree_off) and np.array_equal(a.leaf_taxon, b.leaf_taxon)
        assert np.array_equal(a.adj_depth, b.adj_depth) and np.array_equal(_bits(a.adj_val), _bits(b.adj_val))


def test_single_forests_equal_the_host_path():
    for name in rp.NODE_CASE_NAMES:
        case = rp.node_case(name)
        inp = rp.node_inputs(case)
        present = case.arrays.present_taxa()
        assert np.array_equal(np.flatnonzero(inp["present"]), present)
        tables = case.arrays.flatten(case.strategy, local_ids=present)
        work, perm, group_start, n_groups = scs.prepare_node(tables, case.kind == "groups")
        want = rp.pack_node(work)
        assert _same(inp["want"], want), name
        assert n_groups == inp["n_groups"] and work.n_taxa == inp["n_taxa"]
        if case.kind == "groups":
            assert n_groups < work.n_taxa and np.array_equal(group_start, inp["group_start"])
        if case.kind == "null":
            assert inp["relabel"] is None and len(present) == case.arrays.n_taxa
        else:
            assert len(present) == case.arrays.n_taxa - 5


# ------------------------------------------------------------------------------------ every case on its edge
def test_every_case_is_listed_and_within_the_size_limits():
    names = [c.name for c in rp.level_cases()]
    assert names == rp.LEVEL_CASE_NAMES and len(set(names)) == len(names)
    for case in rp.level_cases():
        inp = case.inputs()
        assert inp["n_taxa"].min() >= 2 and inp["n_taxa"].max() <= 128  # the batched path's sizes
        assert inp["n_groups"].min() >= 2
        assert int(case.tables.n_leaves) <= 4000
        assert np.all(inp["n_leaves"] >= 2 * inp["n_trees"]) and np.all(inp["n_leaves"] <= inp["n_trees"].astype(np.int64) * inp["n_taxa"])
        if len(case.u_lo) > 1:
            assert np.all(case.u_lo[1:] > 0)  # u_base > 0 on every node but the first
        # any wrong value shows: all weights differ, and under `branch` the gaps below the root carry random lengths
        assert len(np.unique(case.level.weights)) == case.level.n_trees
        if case.strategy == "branch":
            av = case.tables.adj_val[case.tables.adj_depth > 0]
            assert len(np.unique(av)) == len(av)


def test_relabels_are_bijections_on_the_present_ids_and_wrong_but_in_range_elsewhere():
    kinds_seen = set()
    absent_total = 0
    for case in rp.level_cases():
        tab = case.tables
        for k in case.batch:
            rl, n, ng, gs, here = rp.node_numbering(tab, int(case.t_lo[k]), int(case.t_hi[k]), int(case.u_lo[k]),
                                                    int(case.u_sz[k]), case.kinds[k])
            kinds_seen.add(case.kinds[k])
            assert sorted(rl[here].tolist()) == list(range(n))  # a bijection onto 0 .. n_pres - 1
            assert np.all(rl >= 0) and np.all(rl < n)  # absent entries: in range, never -1
            absent_total += int((~here).sum())
            if case.kinds[k] == "identity":
                assert here.all() and np.array_equal(rl, np.arange(n))
            if case.kinds[k] == "compact" and not here.all():
                assert np.array_equal(rl[here], np.arange(n)) and not np.array_equal(rl, np.arange(len(rl)))
            if gs is not None:
                assert gs[0] == 0 and gs[-1] == n and np.all(np.diff(gs) >= 1) and len(gs) == ng + 1
    assert kinds_seen == set(rp.KINDS) and absent_total > 100


def test_which_ids_are_absent():
    case = rp.level_case("9 nodes")
    tab = case.tables
    absent = []
    for k in range(9):
        here = rp.node_numbering(tab, int(case.t_lo[k]), int(case.t_hi[k]), int(case.u_lo[k]), int(case.u_sz[k]),
                                 "compact")[4]
        absent.append(np.flatnonzero(~here).tolist())
    # every third id from the second on, as many as the spec leaves out
    assert absent == [[1, 4, 7], [1, 4], [], [1], [1, 4, 7, 10], [], [1, 4, 7], [1], []]


@pytest.mark.parametrize("k", rp.NODE_COUNTS)
def test_node_counts(k):
    inp = rp.level_case(f"{k} nodes").inputs()
    assert len(inp["t_begin"]) == k
    if k >= 256:
        assert inp["n_taxa"].max() == 3 and set(inp["n_trees"].tolist()) == {1, 2}
        assert inp["leaf_ptr"][-1] > 3 * rp.WORKGROUP  # several workgroups of leaf slots over 256 | 257 nodes


@pytest.mark.parametrize("total", rp.LEAF_TOTALS)
def test_leaf_totals(total):
    inp = rp.level_case(f"{total} leaves").inputs()
    assert int(inp["leaf_ptr"][-1]) == total and total > int(inp["tree_ptr"][-1]) + len(inp["t_begin"])  # the leaves size the grid


@pytest.mark.parametrize("slot", rp.EDGE_SLOTS)
def test_boundary_slots(slot):
    case = rp.level_case(f"a node's first leaf in slot {slot}")
    inp = case.inputs()
    assert int(inp["leaf_ptr"][case.mark]) == slot and 0 < case.mark < len(case.batch) - 1
    case = rp.level_case(f"a node's first offset in slot {slot}")
    inp = case.inputs()
    assert int(inp["tree_ptr"][case.mark]) + case.mark == slot and 0 < case.mark < len(case.batch) - 1
    # ... and the weights of that node are written from those threads: its first weight sits at tree_ptr[k]
    assert int(inp["n_trees"][case.mark]) == 3


@pytest.mark.parametrize("k", rp.TIE_NODES)
def test_the_tie(k):
    inp = rp.level_case(f"tie of {k} nodes").inputs()
    n_leaf, n_tree = int(inp["leaf_ptr"][-1]), int(inp["tree_ptr"][-1])
    assert n_leaf == n_tree + k == 2 * k and 2 * k in (256, 258)
    assert np.all(inp["n_taxa"] == 2) and np.all(inp["n_trees"] == 1)
    # two leaves under one root: no proper cluster, W = 0 -- the solve cannot show a wrong pack, the arrays can
    from tests import small_solve_reference as ssr

    tables, gs = inp["host_nodes"][0]
    assert not ssr.oracle_w(tables, gs).any()


def test_subsets_late_trees_and_the_mixed_batch():
    asc, perm, rep = (rp.level_case(n) for n in ("subset ascending", "subset permuted", "subset with a repeat"))
    assert np.all(np.diff(asc.batch) >= 1) and np.any(np.diff(asc.batch) > 1)
    assert sorted(perm.batch.tolist()) == asc.batch.tolist() and perm.batch.tolist() != asc.batch.tolist()
    assert len(set(rep.batch.tolist())) == len(rep.batch) - 1
    late = rp.level_case("late trees")
    inp = late.inputs()
    assert 0 not in late.batch and int(late.tables.tree_off[inp["t_begin"][0]]) == 3000
    assert int(inp["n_leaves"].max()) < 100  # offsets thirty times the node's own leaves
    mixed = rp.level_case("mixed sizes").inputs()
    assert tuple(mixed["n_taxa"][:7].tolist()) == rp.MIXED_TAXA and mixed["n_groups"][7] < mixed["n_taxa"][7]
    assert np.array_equal(mixed["n_groups"][:7], mixed["n_taxa"][:7])
    assert np.any(mixed["u_size"] > mixed["n_taxa"])


def test_single_forest_and_slice_cases_sit_on_their_numbers():
    for name in rp.NODE_CASE_NAMES:
        what, num, kind = name.split()
        tab = rp.node_inputs(rp.node_case(name))["tables"]
        assert (tab.n_leaves if what == "leaves" else tab.n_trees) == int(num)
        if what == "trees" and int(num) > 1:
            assert tab.n_leaves > tab.n_trees + 1  # (the leaves size the grid; thread n_trees writes the last offset)
    case = rp.slice_level()
    inp = case.inputs()
    assert (inp["n_trees"][1:4] + 1).tolist() == [255, 256, 257] and inp["n_leaves"][4:7].tolist() == [255, 256, 257]
    assert int(inp["n_trees"][7]) == 1 and int(case.t_hi[-1]) == case.level.n_trees and int(case.t_lo[0]) == 0
    assert np.any(inp["u_size"] > inp["n_taxa"]) and np.all(inp["u_base"][1:] > 0)
    assert 0 < inp["u_base"][1] < inp["u_size"][1]  # (an ignored u_base reads inside node 1's relabel)
    for k in range(len(case.batch)):  # max_leaves == n_taxa exactly in every node: its first tree holds every present id
        info = rp.slice_tables(case.tables, int(case.t_lo[k]), int(case.t_hi[k]), int(case.u_lo[k]), None, int(inp["n_taxa"][k]))[5]
        assert info["max_leaves"] == info["n_taxa"]
    for n in (40, 300):
        b = rp.build_level(n)
        assert int(b.inputs()["n_taxa"][b.mark]) == n and int(b.u_lo[b.mark]) > 0 and int(b.u_sz[b.mark]) == n + 9


# ------------------------------------------------------------------------------------- the comparison can fail
def _faulty_pack(case: rp.LevelCase, defect: str):
    """``k_small_pack_level`` restated with one error (plain loops over the slots; a node's slots by adding up)."""
    inp = case.inputs()
    tab = case.tables
    k_n = len(case.batch)
    leaf_ptr, tree_ptr = inp["leaf_ptr"], inp["tree_ptr"]
    rl_ptr = np.concatenate(([0], np.cumsum(inp["u_size"])))
    n_leaf, n_tree = int(leaf_ptr[-1]), int(tree_ptr[-1])
    to = np.zeros(n_tree + k_n, dtype=np.int32)
    lt = np.zeros(n_leaf, dtype=np.int32)
    ad = np.zeros(n_leaf, dtype=np.int32)
    av = np.zeros(n_leaf)
    tw = np.zeros(n_tree)
    for k in range(k_n):
        t0 = int(inp["t_begin"][k])
        for i in range(int(leaf_ptr[k]), int(leaf_ptr[k + 1])):
            node = k
            if defect == "boundary leaf to the previous node" and i == leaf_ptr[k] and k > 0:
                node = k - 1
            src = int(tab.tree_off[inp["t_begin"][node]]) + i - int(leaf_ptr[node])
            x = int(tab.leaf_taxon[src]) - (0 if defect == "u_base ignored" else int(inp["u_base"][node]))
            lt[i] = inp["relabel"][(int(rl_ptr[node]) + x) % len(inp["relabel"])]
            ad[i], av[i] = tab.adj_depth[src], tab.adj_val[src]
        for j in range(int(inp["n_trees"][k]) + 1):
            base = 0 if defect == "offsets not rebased" else int(tab.tree_off[t0])
            to[int(tree_ptr[k]) + k + j] = int(tab.tree_off[t0 + j]) - base
            if j < int(inp["n_trees"][k]):
                shift = 1 if defect == "weight shifted by one tree" else 0
                tw[int(tree_ptr[k]) + j] = tab.tree_w[(t0 + j + shift) % tab.n_trees]
    return to, lt, ad, av, tw


DEFECTS = ("boundary leaf to the previous node", "weight shifted by one tree", "offsets not rebased", "u_base ignored")


@pytest.mark.parametrize("name", ["subset permuted", "subset ascending", "subset with a repeat"])
def test_a_pack_with_an_error_differs_from_the_reference(name):
    case = rp.level_case(name)
    want = case.inputs()["want"]
    assert _same(_faulty_pack(case, "none"), want)  # the restatement itself is right
    for defect in DEFECTS:
        got = _faulty_pack(case, defect)
        assert not _same(got, want), defect
        which = [n for n, g, w in zip(("tree_off", "leaf_taxon", "adj_depth", "adj_val", "tree_w"), got, want)
                 if not np.array_equal(g, w)]
        print(f"PACK DEFECT {name:18s} {defect:36s} shows in {', '.join(which)}")


def test_on_a_whole_level_a_boundary_leaf_read_through_the_previous_node_is_the_same_leaf():
    """Why the subsets are there: where the batch IS the level, node k - 1's source offset and relabel run on into
    node k's, and a first leaf handed to the node before comes out right.  Only a batch with gaps shows that error."""
    for name in ("9 nodes", "late trees"):  # (consecutive nodes of the level, from its first or not)
        case = rp.level_case(name)
        assert _same(_faulty_pack(case, "boundary leaf to the previous node"), case.inputs()["want"])
        for defect in DEFECTS[1:]:
            assert not _same(_faulty_pack(case, defect), case.inputs()["want"]), defect


def test_a_wrong_slice_differs_from_the_reference():
    case = rp.slice_level()
    inp = case.inputs()
    tab = case.tables
    rl_ptr = np.concatenate(([0], np.cumsum(inp["u_size"])))
    for k in (1, 4, 8):
        rl = inp["relabel"][rl_ptr[k]:rl_ptr[k + 1]]
        t0, t1, lo = int(case.t_lo[k]), int(case.t_hi[k]), int(case.u_lo[k])
        want = rp.slice_tables(tab, t0, t1, lo, rl, int(inp["n_taxa"][k]))
        off = tab.tree_off[t0:t1 + 1]
        assert not np.array_equal(off.astype(np.int64), want[0])  # not rebased
    # u_base ignored wherever the id itself still names an entry of the node's relabel: node 1 starts below its size
    k = 1
    rl = inp["relabel"][rl_ptr[k]:rl_ptr[k + 1]]
    lo = int(case.u_lo[k])
    x = tab.leaf_taxon[tab.tree_off[case.t_lo[k]]:tab.tree_off[case.t_hi[k]]]
    wrong = rl[np.where(x < len(rl), x, x - lo)]
    assert not np.array_equal(wrong, rp.slice_tables(tab, int(case.t_lo[k]), int(case.t_hi[k]), lo, rl, int(inp["n_taxa"][k]))[1])


# ----------------------------------------------------------------------------------------------- the hooks
NEW_SYMBOLS = {"scs_debug_small_inputs": 7, "scs_debug_tables_download": 8}


def test_the_header_declares_the_hooks_and_the_binding_holds_them():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(rf"int {name}\(([^;]*)\);", header)
        assert decl is not None, name
        params = [p.strip() for p in decl.group(1).split(",")]
        restype, argtypes = _native.SIGNATURES[name]
        assert len(params) == len(argtypes) == n_args and restype is _native.C.c_int, name
        for p, t in zip(params, argtypes):  # pointers travel as addresses, scalars by their C type
            assert t is (_native.C.c_void_p if "*" in p else _native.C.c_int32), (name, p)
    assert _native.ABI_VERSION == 109  # new symbols only
