"""The kernels that carry a resident forest's tables into the small solve's input block or into a tables handle --
``k_small_pack_level`` (``scs_small_solve_begin_level``), ``k_small_pack`` (``scs_small_solve_begin_forest``),
``k_rebase_offsets`` / ``k_relabel_taxa_range`` (``scs_tables_from_forest_range``) and ``k_relabel_taxa``
(``scs_tables_from_forest``) -- against the plain indexing of ``tests/resident_pack_reference.py`` at their edges
(needs an MI355X).  DESIGN.md section 37.

What they write is read back where the next kernel reads it: ``scs_debug_small_inputs`` copies a begun batch's packed
arrays from its device block, ``scs_debug_tables_download`` the five arrays of a handle.  Every comparison is of bits;
there is no tolerance in this file.  Resident forests with tables come from a split, as in the product: a level is
made resident by a level split that keeps everything, and its tree ranges and leaf counts are the ones that split
reported (``child_trees`` / ``child_leaves``), as ``levels.Engine`` takes them.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.backend import Device, SmallTicket
from spectralclustersupertree_amd.treearrays import _STRATEGY_CODE, ResidentArrays
from tests import resident_pack_reference as rp
from tests import small_solve_reference as ssr

pytestmark = pytest.mark.gpu

NAMES = ("tree_off", "leaf_taxon", "adj_depth", "adj_val", "tree_w")


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(autouse=True)
def device_split_of_any_size(monkeypatch):
    monkeypatch.setenv("SCS_DEVICE_SPLIT_MIN_NODES", "0")


# (tests/test_gpu_small_solve_edges.py: a node that comes back non-finite is solved again by another solver -- here
# that would put its answer in the place of the packed batch's)
_RESCUED = []


@pytest.fixture(scope="module", autouse=True)
def _watch_the_general_path():
    general_path = SmallTicket._general_path

    def noted(self, i):
        _RESCUED.append(i)
        return general_path(self, i)

    SmallTicket._general_path = noted
    yield
    SmallTicket._general_path = general_path


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_arrays(got, want, what: str, slots=None) -> None:
    """Five arrays, bit for bit; the first difference by array, slot and -- ``slots`` = (leaf_ptr, tree_ptr) -- node."""
    for i, (name, g, w) in enumerate(zip(NAMES, got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        a, b = (_bits(g), _bits(w)) if g.dtype == np.float64 else (g, w)
        if np.array_equal(a, b):
            continue
        at = int(np.flatnonzero(a != b)[0])
        node = ""
        if slots is not None:
            ptr = slots[0] if i in (1, 2, 3) else slots[1] + (np.arange(len(slots[1])) if i == 0 else 0)
            node = f" (node {int(np.searchsorted(ptr, at, side='right')) - 1} of the batch)"
        msg = (f"{what}: {name} differs in {int(np.count_nonzero(a != b))} of {len(a)} entries, first at {at}{node}: "
               f"{g[at]!r} != {w[at]!r}")
        raise AssertionError(msg)


class _Resident:
    """A level case on the device: the union of a level split that keeps everything, and what the split reported."""

    def __init__(self, dev, case: rp.LevelCase) -> None:
        level = case.level
        n = level.n_taxa
        self.source = ResidentArrays.from_host(level, dev).forest
        self.forest, child_trees, child_leaves, present, _, _ = self.source.split_level(
            np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), 1, n, _STRATEGY_CODE[case.strategy],
            case.t_hi.astype(np.int32))
        counts = child_trees[0].astype(np.int64)
        self.t_hi = np.cumsum(counts)
        self.t_lo = self.t_hi - counts
        self.n_leaves = child_leaves[0].astype(np.int64)
        assert np.array_equal(self.t_lo, case.t_lo) and np.array_equal(self.t_hi, case.t_hi)
        assert np.array_equal(self.n_leaves, case.tables.tree_off[case.t_hi] - case.tables.tree_off[case.t_lo])
        assert self.forest.n_trees == level.n_trees and self.forest.n_leaves == case.tables.n_leaves

    def free(self) -> None:
        self.forest.free()
        self.source.free()


@pytest.fixture(scope="module")
def resident(dev):
    """``resident(case)``: the case's level on the device (made once per level, freed with the module)."""
    made = {}

    def get(case: rp.LevelCase) -> _Resident:
        key = (id(case.level), case.strategy)
        if key not in made:
            made[key] = _Resident(dev, case)
        return made[key]

    yield get
    for r in made.values():
        r.free()


def _begin_level(dev, res: _Resident, case: rp.LevelCase, want_w: bool = False, forest=None, t_begin=None):
    """The batch of ``case`` through ``scs_small_solve_begin_level``, tree ranges and leaf counts as the split reported
    them: ``(ticket, inputs)``."""
    inp = case.inputs()
    nodes = case.batch
    t0 = res.t_lo[nodes] if t_begin is None else t_begin
    n_trees, n_leaves = (res.t_hi - res.t_lo)[nodes], res.n_leaves[nodes]
    assert np.array_equal(n_trees, inp["n_trees"]) and np.array_equal(n_leaves, inp["n_leaves"])
    ticket = dev.small_solve_begin_level(res.forest if forest is None else forest, t0, n_trees, n_leaves, inp["u_base"],
                                         inp["u_size"], inp["relabel"], inp["n_taxa"], inp["n_groups"],
                                         inp["group_start"], want_w=want_w)
    return ticket, inp


def _packed(ticket, inp):
    k = len(inp["t_begin"])
    assert ticket._counts == (int(inp["tree_ptr"][-1]) + k, int(inp["leaf_ptr"][-1]), int(inp["tree_ptr"][-1]))
    return ticket.debug_inputs()


# ---------------------------------------------------------------------------------- A. the level pack, the arrays
@pytest.mark.parametrize("name", rp.LEVEL_CASE_NAMES)
def test_level_pack_arrays(dev, resident, name):
    case = rp.level_case(name)
    ticket, inp = _begin_level(dev, resident(case), case)
    try:
        got = _packed(ticket, inp)  # (on a ticket that is still begun)
    finally:
        ticket.raw()
    assert_same_arrays(got, inp["want"], name, (inp["leaf_ptr"], inp["tree_ptr"]))


@pytest.mark.parametrize("k", [0, 4, 8])
def test_level_pack_arrays_of_a_node_taken_from_a_slice_of_the_level(dev, resident, k):
    """What ``Engine.redo`` does: the node's trees as a forest of their own (``t_begin = 0``), ids still the level's."""
    base = rp.level_case("9 nodes")
    case = base.with_batch(f"node {k} of a slice", [k])
    res = resident(base)
    piece = res.forest.slice(int(res.t_lo[k]), int(res.t_hi[k]))
    try:
        ticket, inp = _begin_level(dev, res, case, forest=piece, t_begin=np.zeros(1, dtype=np.int32))
        try:
            got = _packed(ticket, inp)
        finally:
            ticket.raw()
    finally:
        piece.free()
    assert_same_arrays(got, inp["want"], case.name, (inp["leaf_ptr"], inp["tree_ptr"]))


def test_the_host_packed_batch_reads_back_as_it_was_passed(dev):
    """The hook's own control: a batch packed on the host holds exactly the arrays it was given."""
    inp = rp.level_case("mixed sizes").inputs()
    ticket = dev.small_solve_begin(inp["host_nodes"])
    try:
        got = _packed(ticket, inp)
    finally:
        ticket.result()
    assert_same_arrays(got, inp["want"], "host-packed", (inp["leaf_ptr"], inp["tree_ptr"]))


# ----------------------------------------------------------------------------------- B. the level pack, the solve
@pytest.mark.parametrize("name", ["mixed sizes", "9 nodes"])
def test_level_solve_equals_the_host_packed_solve_and_the_oracle(dev, resident, name):
    case = rp.level_case(name)
    before = len(_RESCUED)
    ticket, inp = _begin_level(dev, resident(case), case, want_w=True)
    got = ticket.result()
    want = dev.small_solve_begin(inp["host_nodes"], want_w=True).result()
    assert len(_RESCUED) == before, "a node came back non-finite and was solved again by the general path"
    assert len(got) == len(want) == len(case.batch)
    for i, (g, w, (tables, gs)) in enumerate(zip(got, want, inp["host_nodes"])):
        for what, a, b in zip(("maps", "lambda", "W"), g, w):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{name}: node {i}: {what} differs"
        assert np.all(np.isfinite(g[1]))
        w_ref = ssr.oracle_w(tables, gs)
        assert np.array_equal(_bits(g[2]), _bits(w_ref)), f"{name}: node {i}: W differs from the oracle's bits"


# ---------------------------------------------------------------------------------------- C. the single-node pack
def _identity_child(dev, arrays, strategy: str):
    n = arrays.n_taxa
    source = ResidentArrays.from_host(arrays, dev).forest
    kid = source.split(np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), [n], _STRATEGY_CODE[strategy])[0]
    return source, kid


@pytest.mark.parametrize("name", rp.NODE_CASE_NAMES)
def test_single_node_pack_arrays_and_solve(dev, monkeypatch, name):
    case = rp.node_case(name)
    inp = rp.node_inputs(case)
    tab = inp["tables"]
    source, kid = _identity_child(dev, case.arrays, case.strategy)
    calls = []
    entry = dev._lib.scs_small_solve_begin_forest

    def counted(*args):
        calls.append(1)
        return entry(*args)

    monkeypatch.setattr(dev._lib, "scs_small_solve_begin_forest", counted)
    try:
        assert kid.n_trees == tab.n_trees and kid.n_leaves == tab.n_leaves
        host = inp["host"]
        node = fl.TreeTables(n_taxa=host.n_taxa, tree_off=host.tree_off, leaf_taxon=host.leaf_taxon,
                             adj_depth=host.adj_depth, adj_val=host.adj_val, tree_w=host.tree_w, monotone=host.monotone,
                             resident=(kid, inp["relabel"]))
        before = len(_RESCUED)
        out = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("SCS_RESIDENT_SOLVE", mode)
            ticket = dev.small_solve_begin([(node, inp["group_start"])], want_w=True)
            try:
                assert ticket._counts == (tab.n_trees + 1, tab.n_leaves, tab.n_trees)
                got = ticket.debug_inputs()
            finally:
                out[mode] = ticket.result()[0]
            assert_same_arrays(got, inp["want"], f"{name} (SCS_RESIDENT_SOLVE={mode})")
            assert len(calls) == 1, "the resident entry is taken with SCS_RESIDENT_SOLVE=1 and only then"
        assert len(_RESCUED) == before
        for what, a, b in zip(("maps", "lambda", "W"), out["1"], out["0"]):
            assert np.array_equal(_bits(a), _bits(b)), f"{name}: {what} differs from the host-packed solve"
        assert np.array_equal(_bits(out["1"][2]), _bits(ssr.oracle_w(host, inp["group_start"])))
    finally:
        kid.free()
        source.free()


# ------------------------------------------------------------------------------------------- D. the table slices
def _slice_want(case: rp.LevelCase, inp: dict, k: int):
    rl_ptr = np.concatenate(([0], np.cumsum(inp["u_size"])))
    rl = inp["relabel"][rl_ptr[k]:rl_ptr[k + 1]]
    want = rp.slice_tables(case.tables, int(case.t_lo[k]), int(case.t_hi[k]), int(case.u_lo[k]), rl, int(inp["n_taxa"][k]))
    return rl, want


def _check_handle(dtab, want, what: str) -> None:
    got = dtab.debug_download()
    assert got[5] == want[5], f"{what}: the handle says {got[5]}, expected {want[5]}"
    assert_same_arrays(got[:5], want[:5], what)


@pytest.mark.parametrize("context", ["own", "second"])
def test_table_slices_of_every_node(dev, resident, context):
    """``scs_tables_from_forest_range`` for every node of ``slice_level``: ``t_begin = 0``, ``t_begin > 0``, ``t_end =
    n_trees``, one tree, 255 | 256 | 257 offset entries, 255 | 256 | 257 leaves, ``u_base > 0``, compacting relabels,
    ``max_leaves == n_taxa`` in every node -- on the forest's own context and on a second one of the same GPU."""
    case = rp.slice_level()
    inp = case.inputs()
    res = resident(case)
    d = dev if context == "own" else Device(0)
    try:
        for k in range(len(case.batch)):
            rl, want = _slice_want(case, inp, k)
            assert want[5]["max_leaves"] == want[5]["n_taxa"]
            dtab = d.upload_range(res.forest, int(res.t_lo[k]), int(res.t_hi[k]), int(case.u_lo[k]), int(case.u_sz[k]),
                                  rl, int(inp["n_taxa"][k]), True)
            try:
                _check_handle(dtab, want, f"node {k} ({context} context)")
            finally:
                dtab.free()
    finally:
        if d is not dev:
            d.close()


def test_table_slices_taken_from_a_slice_of_the_forest(dev, resident):
    """The same from ``scs_forest_slice`` pieces: a node's own piece (``t_begin = 0``, all its trees) and a piece of
    five nodes with the range inside it (``t_begin > 0``)."""
    case = rp.slice_level()
    inp = case.inputs()
    res = resident(case)
    for k, (a, b) in ((2, (2, 3)), (5, (5, 6)), (4, (1, 6)), (1, (1, 6)), (8, (7, 9))):
        piece = res.forest.slice(int(res.t_lo[a]), int(res.t_hi[b - 1]))
        try:
            rl, want = _slice_want(case, inp, k)
            shift = int(res.t_lo[a])
            dtab = dev.upload_range(piece, int(res.t_lo[k]) - shift, int(res.t_hi[k]) - shift, int(case.u_lo[k]),
                                    int(case.u_sz[k]), rl, int(inp["n_taxa"][k]), True)
            try:
                _check_handle(dtab, want, f"node {k} from the piece of nodes {a} .. {b - 1}")
            finally:
                dtab.free()
        finally:
            piece.free()


@pytest.mark.parametrize("name", rp.NODE_CASE_NAMES)
def test_tables_of_a_whole_child(dev, monkeypatch, name):
    """``scs_tables_from_forest`` (``Device.upload`` of tables that are resident) on the single forests of section C:
    relabel null and non-null, from the child's context and from a second one."""
    case = rp.node_case(name)
    inp = rp.node_inputs(case)
    tab, host = inp["tables"], inp["host"]
    source, kid = _identity_child(dev, case.arrays, case.strategy)
    other = Device(0)
    monkeypatch.setenv("SCS_RESIDENT_SOLVE", "1")
    calls = []
    entry = dev._lib.scs_tables_from_forest

    def counted(*args):
        calls.append(1)
        return entry(*args)

    monkeypatch.setattr(dev._lib, "scs_tables_from_forest", counted)
    try:
        node = fl.TreeTables(n_taxa=host.n_taxa, tree_off=host.tree_off, leaf_taxon=host.leaf_taxon,
                             adj_depth=host.adj_depth, adj_val=host.adj_val, tree_w=host.tree_w, monotone=host.monotone,
                             resident=(kid, inp["relabel"]))
        want = rp.slice_tables(tab, 0, tab.n_trees, 0, inp["relabel"], host.n_taxa)
        for d in (dev, other):
            dtab = d.upload(node)
            try:
                _check_handle(dtab, want, f"{name} ({'own' if d is dev else 'second'} context)")
            finally:
                dtab.free()
        assert len(calls) == 2  # (both handles came from the resident forest, none from the host arrays)
    finally:
        other.close()
        kid.free()
        source.free()


@pytest.mark.parametrize("n_taxa", [40, 300])
def test_build_from_a_slice_equals_the_build_from_uploaded_tables(dev, resident, n_taxa):
    case = rp.build_level(n_taxa)
    inp = case.inputs()
    res = resident(case)
    k = case.mark
    rl, want = _slice_want(case, inp, k)
    tables = inp["host_nodes"][k][0]
    mono = bool(case.tables.monotone)
    tables.monotone = mono
    got = {}
    for how in ("slice", "upload"):
        if how == "slice":
            dtab = dev.upload_range(res.forest, int(res.t_lo[k]), int(res.t_hi[k]), int(case.u_lo[k]), int(case.u_sz[k]),
                                    rl, n_taxa, mono)
            _check_handle(dtab, want, f"build {n_taxa}")
        else:
            dtab = dev.upload(tables)
        try:
            graph = dtab.build()
        finally:
            dtab.free()
        try:
            got[how] = graph.download()
        finally:
            graph.free()
    assert got["slice"].shape == (n_taxa, n_taxa)
    assert np.array_equal(_bits(got["slice"]), _bits(got["upload"]))
    assert np.array_equal(_bits(got["slice"]), _bits(to.pcg_dense(tables)[0]))


# ------------------------------------------------------------------------------------------------- E. refusals
def _refused(message: str, rc_call) -> None:
    with pytest.raises(nv.ScsError) as err:
        nv.check(rc_call())
    assert err.value.code == nv.EINVAL and message in str(err.value), str(err.value)


def test_refusals_by_message_and_a_good_call_afterwards(dev, resident):
    case = rp.level_case("9 nodes")
    res = resident(case)
    inp = case.inputs()
    lib, ctx = dev._lib, dev._ctx
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    good = {"t_begin": i32(res.t_lo), "n_trees": i32(res.t_hi - res.t_lo), "n_leaves": res.n_leaves.copy(),
            "u_base": inp["u_base"], "u_size": inp["u_size"], "relabel": inp["relabel"], "n_taxa": inp["n_taxa"],
            "n_groups": inp["n_groups"], "group_start": inp["group_start"]}
    order = ("t_begin", "n_trees", "n_leaves", "u_base", "u_size", "relabel", "n_taxa", "n_groups", "group_start")

    def level(forest=None, **change):
        a = dict(good)
        a.update(change)
        ticket = C.c_int32(-1)
        args = [None if a[key] is None else a[key].ctypes.data for key in order]
        rc = lib.scs_small_solve_begin_level(ctx, (res.forest if forest is None else forest)._h, len(good["t_begin"]),
                                             *args, 0, C.byref(ticket))
        assert rc != 0 and ticket.value == -1
        return rc

    def changed(key, node, value):
        a = good[key].copy()
        a[node] = value
        return {key: a}

    def round_trip():
        ticket, _ = _begin_level(dev, res, case)
        try:
            got = _packed(ticket, inp)
        finally:
            ticket.raw()
        assert_same_arrays(got, inp["want"], "a good call", (inp["leaf_ptr"], inp["tree_ptr"]))
        rl, want = _slice_want(case, inp, 4)
        dtab = dev.upload_range(res.forest, int(res.t_lo[4]), int(res.t_hi[4]), int(case.u_lo[4]), int(case.u_sz[4]), rl,
                                int(inp["n_taxa"][4]), True)
        _check_handle(dtab, want, "a good slice")
        dtab.free()

    round_trip()  # (the slot and the arena are warm: what follows must leave both as they are)
    dev.synchronize()
    used = dev.arena_stats()["used_bytes"]
    plain = resident(case).source  # a plain upload: no tables
    n_trees, n_taxa = res.forest.n_trees, res.forest.n_taxa
    m = good["n_trees"]
    # ---- scs_small_solve_begin_level
    for key in order:
        _refused("scs_small_solve_begin_level: null argument", lambda key=key: level(**{key: None}))
    _refused("scs_small_solve_begin_level: the forest carries no tables", lambda: level(forest=plain))
    for node, key, value in ((0, "t_begin", -1), (8, "t_begin", n_trees - int(m[8]) + 1), (3, "n_trees", 0),
                             (8, "n_trees", int(m[8]) + 1)):
        _refused(f"scs_small_solve_begin_level: node {node}: bad tree range", lambda: level(**changed(key, node, value)))
    for node, key, value in ((2, "u_base", -1), (8, "u_size", int(case.u_sz[8]) + 1), (5, "u_size", 0),
                             (8, "u_base", n_taxa)):
        _refused(f"scs_small_solve_begin_level: node {node}: bad taxon range", lambda: level(**changed(key, node, value)))
    _refused("scs_small_solve_begin_level: node 6: bad leaf count", lambda: level(**changed("n_leaves", 6, 2 * int(m[6]) - 1)))
    _refused("scs_small_solve_begin_level: node 6: bad leaf count",
             lambda: level(**changed("n_leaves", 6, int(m[6]) * int(inp["n_taxa"][6]) + 1)))
    # ---- scs_small_solve_begin_forest
    gs = np.arange(3, dtype=np.int32)
    ticket = C.c_int32(-1)
    _refused("scs_small_solve_begin_forest: null argument",
             lambda: lib.scs_small_solve_begin_forest(ctx, res.forest._h, None, 2, 2, None, 0, C.byref(ticket)))
    _refused("scs_small_solve_begin_forest: null argument",
             lambda: lib.scs_small_solve_begin_forest(ctx, None, None, 2, 2, gs.ctypes.data, 0, C.byref(ticket)))
    _refused("scs_small_solve_begin_forest: the forest carries no tables",
             lambda: lib.scs_small_solve_begin_forest(ctx, plain._h, None, 2, 2, gs.ctypes.data, 0, C.byref(ticket)))
    assert ticket.value == -1
    # ---- scs_tables_from_forest_range
    rl, want = _slice_want(case, inp, 4)
    t0, t1, lo, sz, n4 = int(res.t_lo[4]), int(res.t_hi[4]), int(case.u_lo[4]), int(case.u_sz[4]), int(inp["n_taxa"][4])
    handle = C.c_void_p()

    def table_range(forest, a, b, u0, us, relabel, n):
        rc = lib.scs_tables_from_forest_range(ctx, forest._h if forest is not None else None, a, b, u0, us,
                                              relabel.ctypes.data if relabel is not None else None, n, C.byref(handle))
        assert rc != 0 and not handle.value
        return rc

    _refused("scs_tables_from_forest_range: null argument", lambda: table_range(res.forest, t0, t1, lo, sz, None, n4))
    _refused("scs_tables_from_forest_range: null argument", lambda: table_range(None, t0, t1, lo, sz, rl, n4))
    _refused("scs_tables_from_forest_range: the forest carries no tables", lambda: table_range(plain, t0, t1, lo, sz, rl, n4))
    for a, b in ((-1, t1), (t0, t0), (t1, t0), (t0, n_trees + 1)):
        _refused("scs_tables_from_forest_range: bad tree range", lambda: table_range(res.forest, a, b, lo, sz, rl, n4))
    for u0, us, n in ((-1, sz, n4), (lo, 0, n4), (n_taxa - sz + 1, sz, n4), (lo, sz, 0)):
        _refused("scs_tables_from_forest_range: bad taxon range", lambda: table_range(res.forest, t0, t1, u0, us, rl, n))
    _refused("scs_tables_from_forest_range: a tree has more leaves (40) than the node has taxa (39)",
             lambda: table_range(res.forest, t0, t1, lo, sz, rl, n4 - 1))
    # ---- scs_tables_from_forest (a child of scs_forest_split; a slice of one keeps no host offsets: no tables)
    node = rp.node_case("trees 2 groups")
    source, kid = _identity_child(dev, node.arrays, "branch")
    piece = kid.slice(0, 1)
    try:
        def table_child(forest, n):
            rc = lib.scs_tables_from_forest(ctx, forest._h if forest is not None else None, None, n, C.byref(handle))
            assert rc != 0 and not handle.value
            return rc

        _refused("scs_tables_from_forest: null argument", lambda: table_child(None, 20))
        _refused("scs_tables_from_forest: the forest carries no tables", lambda: table_child(source, 20))
        _refused("scs_tables_from_forest: the forest carries no tables", lambda: table_child(piece, 20))
        _refused("scs_tables_from_forest: need >= 1 taxon and >= 1 tree", lambda: table_child(kid, 0))
        _refused("scs_tables_from_forest: a tree has more leaves (20) than the node has taxa (19)", lambda: table_child(kid, 19))
    finally:
        piece.free()
        kid.free()
        source.free()
    # ---- the hooks
    _refused("scs_debug_tables_download: null argument",
             lambda: lib.scs_debug_tables_download(ctx, None, None, None, None, None, None, None))
    ended, _ = _begin_level(dev, res, case)
    number = ended._ticket
    ended.raw()
    for t in (-1, number, 1 << 20):
        _refused(f"scs_small_solve_end: no such ticket ({t})", lambda: lib.scs_debug_small_inputs(ctx, t, None, None, None, None, None))
    _refused("scs_debug_small_inputs: null context", lambda: lib.scs_debug_small_inputs(None, 0, None, None, None, None, None))
    # ---- nothing was left behind, and the entries still work
    dev.synchronize()
    assert dev.arena_stats()["used_bytes"] == used
    round_trip()
    dev.synchronize()
    assert dev.arena_stats()["used_bytes"] == used
