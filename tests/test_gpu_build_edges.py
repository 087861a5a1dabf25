"""The build of W, the degrees, the single-precision image and the contraction at the sizes where their code changes
path: W bit for bit against the C oracle -- the padding columns included, read through
``scs_debug_graph_raw`` from a block of the arena that held something else before --, the degrees within the rounding
bound of a sum in any order, the image bit for bit against ``float32(W)`` where it is defined, the contraction bit for
bit against a double loop.  The forests are built by ``tests/build_reference.py``; ``tests/test_build_reference_cpu.py``
proves without a device that each has the numbers it is named for and that the degree budget has teeth."""

import threading

import build_reference as br
import numpy as np
import pytest

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


_CACHE: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _oracle(key, tb):
    """``pcg_dense`` of the tables of case ``key``, computed once and left unchanged."""
    w = _cached(("w", key), lambda: to.pcg_dense(tb)[0])
    w.flags.writeable = False
    return w


def _dirty(dev, rows, ld):
    """Build and free a graph of ``rows x ld`` doubles whose every column is data (``ld`` taxa, no padding, nearly
    every cell 1.0): the arena hands the next graph of that size a block that is not zero where its padding lies."""
    if rows < 1 or rows > ld:
        return
    tb = _cached(("dirty", ld), lambda: br.tables(br.forest(0, ld, [("caterpillar", np.arange(ld, dtype=np.int32))],
                                                            unit_weights=True), "one"))
    dtab = dev.upload(tb)
    g = dtab.build(0, rows)
    g.free()
    dtab.free()


def _first_cells(diff, got, want):
    return (f"{int(diff.sum())} cells differ; first at {np.argwhere(diff)[:5].tolist()}, got {got[diff][:5]}, "
            f"want {want[diff][:5]}")


def _check_raw(g, n, want, what=""):
    """``raw[:, :n]`` equals ``want`` bit for bit and ``raw[:, n:ld]`` is all zero bits."""
    raw, info = g.raw(0)
    assert info["ld"] == br.ld_of(n) and raw.shape == (want.shape[0], info["ld"]) and info["col0"] == 0, (what, info)
    diff = raw[:, :n] != want
    assert not diff.any(), f"{what}: " + _first_cells(diff, raw[:, :n], want)
    assert np.array_equal(np.signbit(raw[:, :n]), np.signbit(want)), f"{what}: a zero of the other sign"
    pad = raw[:, n:].view(np.uint64) != 0
    assert not pad.any(), (f"{what}: {int(pad.sum())} padding cells of W are not zero; first at "
                           f"{(np.argwhere(pad)[:5] + [0, n]).tolist()}: {raw[:, n:][pad][:5]}")
    return raw


def _build_check(dev, tb, w_ref, ranges=None, what="", expect=None):
    """Every row range of ``ranges`` (default: the whole matrix) built into a dirty block and compared, padding
    included; ``expect(build_stats)`` asserts the path.  Returns the last build's stats."""
    n = tb.n_taxa
    dtab = dev.upload(tb)
    stats = None
    try:
        for rb, re_ in ranges or [(0, n)]:
            _dirty(dev, re_ - rb, br.ld_of(n))
            g = dtab.build(rb, re_)
            try:
                stats = g.build_stats
                if expect is not None:
                    expect(stats)
                _check_raw(g, n, w_ref[rb:re_] if w_ref.shape[0] == n else w_ref, f"{what} rows [{rb}, {re_})")
                w = g.download()
                assert np.array_equal(w, w_ref[rb:re_] if w_ref.shape[0] == n else w_ref)
            finally:
                g.free()
    finally:
        dtab.free()
    return stats


# ---------------------------------------------------------------------------------------------------------------
# 64-row blocks, 256-column groups, 512 padding
# ---------------------------------------------------------------------------------------------------------------
def _size_case(n, name):
    def make():
        tb = br.tables(br.size_forest(n, name), br.weighting(name)[0])
        if name == "signed":
            tb.monotone = False  # (trees of one or two leaves have no inner length to be negative: the general kernel anyway)
        return tb

    tb = _cached(("size", n, name), make)
    return tb, _oracle(("size", n, name), tb)


@pytest.mark.parametrize("name", br.WEIGHTINGS)
@pytest.mark.parametrize("n", br.SIZES)
def test_whole_matrix_at_block_group_and_padding_sizes(dev, n, name):
    tb, w_ref = _size_case(n, name)
    assert tb.monotone == (name in ("one", "branch"))
    st = _build_check(dev, tb, w_ref, what=f"n={n} {name}")
    assert st["n_tiles"] == len(br.tiles(n)) and st["symmetric"] == 1


@pytest.mark.parametrize("name", ["branch", "signed"])
@pytest.mark.parametrize("n", [65, 129, 257, 320, 513, 1025])
def test_row_ranges_inside_and_on_block_edges(dev, n, name):
    tb, w_ref = _size_case(n, name)
    for rb, re_ in br.size_ranges(n):
        st = _build_check(dev, tb, w_ref, [(rb, re_)], what=f"n={n} {name}")
        assert st["n_tiles"] == len(br.tiles(n, rb, re_)) and st["symmetric"] == 0


PATHS = {
    "wide": ("SCS_WIDE", "1", lambda s: s["spec_batches"] == s["n_batches"] >= 1),
    "tree_parallel": ("SCS_TREE_PARALLEL", "1", lambda s: s["tree_parallel_batches"] == s["n_batches"] >= 1),
    "tile_lists": ("SCS_TILE_LISTS", "1", lambda s: s["listed_batches"] == s["n_batches"] >= 1),
    "two_batches": ("SCS_BATCH_TREES", "3", lambda s: s["n_batches"] == 2),
}


def _expect(pred):
    def check(stats):
        assert pred(stats), stats
    return check


# (the producer / consumer kernel and the tile lists are the monotone path's: the general kernel has no such variant)
PATH_CASES = [(path, name) for path in sorted(PATHS) for name in br.WEIGHTINGS
              if name in ("one", "branch") or path not in ("wide", "tile_lists")]


@pytest.mark.parametrize(("path", "name"), PATH_CASES, ids=[f"{p}-{w}" for p, w in PATH_CASES])
@pytest.mark.parametrize("n", br.PATH_SIZES)
def test_every_accumulate_path_at_the_same_sizes(dev, monkeypatch, n, path, name):
    tb, w_ref = _size_case(n, name)
    env, value, pred = PATHS[path]
    monkeypatch.setenv(env, value)
    _build_check(dev, tb, w_ref, what=f"n={n} {name} {path}", expect=_expect(pred))
    if path in ("wide", "two_batches", "tile_lists") and n > 64:  # (the same through a row range: no mirror image)
        _build_check(dev, tb, w_ref, [(1, n - 1)], what=f"n={n} {name} {path}", expect=_expect(pred))


# ---------------------------------------------------------------------------------------------------------------
# the per-(row block, tree) record
# ---------------------------------------------------------------------------------------------------------------
KERNELS = {"mono": ("branch", "positive", None, None), "wide": ("branch", "positive", None, ("SCS_WIDE", "1")),
           "gen": ("branch", "positive", False, None), "gen_signed": ("branch", "signed", None, None)}


def _kernel_tables(key, make_forest, kernel):
    strategy, lengths, mono, env = KERNELS[kernel]
    tb = _cached((key, lengths, strategy, mono), lambda: br.tables(make_forest(lengths), strategy, mono))
    assert tb.monotone == (kernel in ("mono", "wide"))
    return tb, env


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("kind", ["star", "caterpillar", "balanced", "random"])
def test_rows_present_in_a_block(dev, monkeypatch, kind, kernel):
    tb, env = _kernel_tables(("record", kind), lambda lengths: br.record_forest(kind, lengths), kernel)
    if env:
        monkeypatch.setenv(*env)
    w_ref = _oracle(("record", kind, kernel), tb)
    st = _build_check(dev, tb, w_ref, what=f"{kind} {kernel}")
    assert (st["spec_batches"] > 0) == (kernel == "wide")
    lo, hi = br.RECORD_BLOCK * br.TR, (br.RECORD_BLOCK + 1) * br.TR
    _build_check(dev, tb, w_ref, [(lo, hi), (lo - 1, hi + 1)], what=f"{kind} {kernel}")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_rows_of_a_block_one_per_64_positions(dev, monkeypatch, kernel):
    tb, env = _kernel_tables(("spread",), br.spread_forest, kernel)
    if env:
        monkeypatch.setenv(*env)
    lo, hi = br.SPREAD_BLOCK * br.TR, (br.SPREAD_BLOCK + 1) * br.TR
    rows = _cached(("spread-rows", kernel), lambda: to.pcg_rows(tb, np.arange(lo, hi, dtype=np.int32)))
    _build_check(dev, tb, rows, [(lo, hi)], what=f"spread {kernel}")


# ---------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plain", "wide", "general"])
@pytest.mark.parametrize(("strategy", "lengths"), [("one", "positive"), ("branch", "equal"), ("branch", "zero"),
                                                    ("depth", "positive")])
@pytest.mark.parametrize("n", [130, 257])
def test_ties_between_gap_values(dev, monkeypatch, n, strategy, lengths, path):
    tb = br.tables(br.tie_forest(n, lengths), strategy, False if path == "general" else None)
    if path == "wide":
        monkeypatch.setenv("SCS_WIDE", "1")
    w_ref = _oracle(("tie", n, strategy, lengths), br.tables(br.tie_forest(n, lengths), strategy))
    _build_check(dev, tb, w_ref, what=f"ties n={n} {strategy} {lengths} {path}")
    _build_check(dev, tb, w_ref, [(63, 129)], what=f"ties n={n} {strategy} {lengths} {path}")


# ---------------------------------------------------------------------------------------------------------------
# trees without gaps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["plain", "wide", "tree_parallel", "general"])
@pytest.mark.parametrize("which", ["ones", "twos", "first", "last", "mixed"])
def test_trees_of_one_and_two_leaves(dev, monkeypatch, which, path):
    tb = br.tables(br.gapless_forest(which), "branch", False if path == "general" else None)
    if path in PATHS:
        monkeypatch.setenv(*PATHS[path][:2])
    if path == "tree_parallel":  # (five one-leaf trees on 70 taxa cover less than 1 / 64: tile lists would win)
        monkeypatch.setenv("SCS_TILE_LISTS", "0")
    w_ref = _oracle(("gapless", which), tb)
    if which in ("ones", "twos"):
        assert not w_ref.any()  # (two leaves meet at the root: no proper cluster)
    _build_check(dev, tb, w_ref, what=f"{which} {path}", expect=_expect(PATHS[path][2]) if path in PATHS else None)
    _build_check(dev, tb, w_ref, [(5, 69)], what=f"{which} {path}")


# ---------------------------------------------------------------------------------------------------------------
# table levels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", ["positive", "signed"])
@pytest.mark.parametrize("gaps", br.LEVEL_GAPS)
def test_table_levels_around_powers_of_two(dev, gaps, lengths):
    tb = br.tables(br.level_forest(gaps, lengths), "branch")
    if gaps >= 1023:
        assert tb.monotone == (lengths == "positive")
    elif lengths == "signed":
        tb.monotone = False  # (a tree of a few nodes may have drawn no negative length: the general kernel all the same)
    _build_check(dev, tb, to.pcg_dense(tb)[0], what=f"m={gaps} {lengths}")  # (33 MB at 2 049 gaps: not kept)


@pytest.mark.parametrize("lengths", ["positive", "signed"])
@pytest.mark.parametrize("mixed", [False, True], ids=["alone", "mixed"])
@pytest.mark.parametrize("leaves", [br.SPARSE_FUSED_MAX_LEAVES, br.SPARSE_FUSED_MAX_LEAVES + 1])
def test_fused_and_per_level_tables(dev, leaves, mixed, lengths):
    tb = br.tables(br.big_forest(leaves, mixed, lengths), "branch")
    assert tb.monotone == (lengths == "positive")
    rb, re_ = br.BIG_ROWS
    rows = to.pcg_rows(tb, np.arange(rb, re_, dtype=np.int32))
    st = _build_check(dev, tb, rows, [(rb, re_)], what=f"{leaves} leaves mixed={mixed} {lengths}")
    assert st["n_batches"] == 1 and st["n_trees"] == (21 if mixed else 1)


# ---------------------------------------------------------------------------------------------------------------
# dispatch gates, no switch set
# ---------------------------------------------------------------------------------------------------------------
def _assert_plan(st, want, n_trees):
    assert st["n_tiles"] == want["n_tiles"], (st, want)
    assert st["n_batches"] == 1 and st["n_trees"] == n_trees, st
    assert st["tree_parallel_batches"] == int(want["tree_parallel"]), (st, want)
    assert st["spec_batches"] == int(want["wide"]), (st, want)
    assert st["listed_batches"] == int(want["listed"]), (st, want)


@pytest.mark.parametrize("case", sorted(br.GATE_CASES))
def test_dispatch_gates_take_the_side_the_plan_says(dev, monkeypatch, case):
    for env in ("SCS_WIDE", "SCS_TREE_PARALLEL", "SCS_TILE_LISTS", "SCS_BATCH_TREES", "SCS_TILE_ORDER", "SCS_NO_MONOTONE"):
        monkeypatch.delenv(env, raising=False)
    n, n_trees, leaves = br.GATE_CASES[case]
    tb = br.tables(br.gate_forest(n, n_trees, leaves), "branch")
    assert tb.monotone
    want = br.plan(n, tb.n_trees, tb.n_leaves, True)
    st = _build_check(dev, tb, _oracle(("gate", case), tb), what=case)
    _assert_plan(st, want, n_trees)


@pytest.mark.parametrize("case", sorted(br.GATE_ROW_CASES))
def test_row_ranges_on_both_sides_of_the_tile_gates(dev, monkeypatch, case):
    for env in ("SCS_WIDE", "SCS_TREE_PARALLEL", "SCS_TILE_LISTS", "SCS_BATCH_TREES", "SCS_TILE_ORDER", "SCS_NO_MONOTONE"):
        monkeypatch.delenv(env, raising=False)
    n, n_trees, leaves, (rb, re_) = br.GATE_ROW_CASES[case]
    tb = br.tables(br.gate_forest(n, n_trees, leaves), "branch")
    want = br.plan(n, tb.n_trees, tb.n_leaves, True, rb, re_)
    rows = to.pcg_rows(tb, np.arange(rb, re_, dtype=np.int32))
    st = _build_check(dev, tb, rows, [(rb, re_)], what=case)
    _assert_plan(st, want, n_trees)


# ---------------------------------------------------------------------------------------------------------------
# degrees
# ---------------------------------------------------------------------------------------------------------------
_RATIOS: list = []


def _degrees_within_budget(deg, w, what):
    ref, budget = br.degrees_reference(w)
    err = np.abs(deg.astype(br.LD) - ref)
    ratio = float(np.max(np.where(budget > 0, err / np.where(budget > 0, budget, 1), np.where(err > 0, np.inf, 0.0))))
    _RATIOS.append(ratio)
    print(f"[degrees] {what}: worst error / budget = {ratio:.4f} (all cases so far: {max(_RATIOS):.4f})")
    bad = err > budget
    assert not bad.any(), f"{what}: rows {np.flatnonzero(bad)[:5].tolist()} off by {err[bad][:5]} > {budget[bad][:5]}"


@pytest.mark.parametrize("n", br.DEGREE_SIZES)
def test_degrees_of_signed_rows(dev, n):
    arrays, lone = br.degree_forest(n)
    tb = br.tables(arrays, "branch")
    dtab = dev.upload(tb)
    try:
        for rb, re_ in br.degree_ranges(n):
            g = dtab.build(rb, re_)
            try:
                deg = g.degrees()
                w = g.download()  # the budget is taken against the matrix the kernel summed
            finally:
                g.free()
            assert deg.shape == (re_ - rb,)
            if n >= 127 and (rb, re_) == (0, n):
                assert (w < 0).any() and (w > 0).any()
            _degrees_within_budget(deg, w, f"n={n} rows [{rb}, {re_})")
            if rb <= lone < re_:
                assert not w[lone - rb].any()
                assert deg[lone - rb] == 0.0 and not np.signbit(deg[lone - rb])
    finally:
        dtab.free()


def _ranks(world, fn):
    """``fn(rank, device)`` on ``world`` in-process ranks of one GPU, a host thread each; returns their results."""
    lib = nv.load_library()
    group = nv.C.c_void_p()
    nv.check(lib.scs_local_group_create(world, nv.C.byref(group)))
    out, err = [None] * world, [None] * world

    def worker(rank):
        try:
            d = Device(0, rank, world, _local_group=group)
            try:
                out[rank] = fn(rank, d)
            finally:
                d.close()
        except BaseException as e:  # noqa: BLE001
            err[rank] = e

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    lib.scs_local_group_destroy(group)
    assert err == [None] * world, err
    return out


@pytest.mark.parametrize("splits", br.RANK_SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_degrees_over_ranks(dev, splits):
    n = br.RANK_N
    tb = br.tables(br.degree_forest(n)[0], "branch")
    w_ref = _oracle(("degree", n), tb)

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1])
        try:
            return g.download(), g.degrees_all(), g.degrees()
        finally:
            g.free()
            dtab.free()

    out = _ranks(len(splits) - 1, rank_fn)
    w = np.concatenate([o[0] for o in out])
    assert np.array_equal(w, w_ref)
    for rank, (_, deg_all, deg_own) in enumerate(out):
        assert np.array_equal(deg_all, out[0][1]), rank  # every rank holds the same vector
        assert np.array_equal(deg_own, deg_all[splits[rank]:splits[rank + 1]])
    _degrees_within_budget(out[0][1], w, f"ranks {splits}")


# ---------------------------------------------------------------------------------------------------------------
# the single-precision image
# ---------------------------------------------------------------------------------------------------------------
def _check_image(img, info, w, row_begin, full, what):
    want, defined = br.image_reference(w, info["ld"], row_begin, full)
    assert img.dtype == np.float32 and img.shape == want.shape
    first = np.zeros(len(w), dtype=np.int64) if full else (row_begin + np.arange(len(w))) // br.IMG_TILE * br.IMG_TILE
    assert np.array_equal(info["first_col"], first), what
    diff = (img.view(np.uint32) != want.view(np.uint32)) & defined
    assert not diff.any(), (f"{what}: {int(diff.sum())} image cells differ; first at {np.argwhere(diff)[:5].tolist()}, "
                            f"got {img[diff][:5]}, want {want[diff][:5]}")


@pytest.mark.parametrize("n", br.IMAGE_SIZES)
def test_image_is_float32_of_w_where_defined(dev, n):
    tb = br.tables(br.size_forest(n, "signed", seed=1), "branch")
    w_ref = _oracle(("image", n), tb)
    dtab = dev.upload(tb)
    try:
        plain = dtab.build()
        deg_plain = plain.degrees()  # k_degrees<false>
        plain.free()
        _dirty(dev, n, br.ld_of(n))
        g = dtab.build()
        try:
            img, info = g.raw(1)  # k_degrees<true>: the image and the degrees in one pass
            deg = g.degrees()
            _check_raw(g, n, w_ref, f"image n={n}")
            _check_image(img, info, w_ref, 0, False, f"n={n}")
            again, _ = g.raw(1)  # (the image is kept: a second call returns the same bits)
            assert np.array_equal(again.view(np.uint32), img.view(np.uint32))
        finally:
            g.free()
    finally:
        dtab.free()
    assert np.array_equal(deg, deg_plain)
    _degrees_within_budget(deg, w_ref, f"image pass n={n}")


def test_image_of_a_partitioned_rank_holds_whole_rows(dev):
    n, splits = 1025, [0, 513, 1025]
    tb = br.tables(br.size_forest(n, "signed", seed=1), "branch")
    w_ref = _oracle(("image", n), tb)

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1])
        try:
            img, info = g.raw(1)
            return img, info, g.download(), g.degrees_all()
        finally:
            g.free()
            dtab.free()

    out = _ranks(2, rank_fn)
    for rank, (img, info, w, deg) in enumerate(out):
        assert np.array_equal(w, w_ref[splits[rank]:splits[rank + 1]])
        _check_image(img, info, w, splits[rank], True, f"rank {rank}")
        assert np.array_equal(deg, out[0][3])
    _degrees_within_budget(out[0][3], w_ref, "image pass, two ranks")


def test_no_image_means_unsupported(dev):
    tb, _ = _size_case(513, "branch")
    dtab = dev.upload(tb)
    try:
        g = dtab.build(64, 200)  # a row block on one rank
        with pytest.raises(nv.ScsError) as exc:
            g.raw(1)
        assert exc.value.code == nv.EUNSUP
        _, info = g.raw(0)
        assert info["rows"] == 136 and info["ld"] == 1024
        g.free()
        mf = dtab.matrix_free_graph()
        for what in (0, 1):
            with pytest.raises(nv.ScsError) as exc:
                mf.raw(what)
            assert exc.value.code == nv.EUNSUP
        mf.free()
        whole = dtab.build()
        for what in (2, 3, -1):  # (mode 2 has another shape: `degrees_all`)
            with pytest.raises(ValueError, match="what must be 0"):
                whole.raw(what)
        info = np.zeros(4, dtype=np.int32)
        assert dev._lib.scs_debug_graph_raw(dev._ctx, whole._h, 3, None, nv.iptr(info)) == nv.EINVAL
        whole.free()
    finally:
        dtab.free()


# ---------------------------------------------------------------------------------------------------------------
# contraction
# ---------------------------------------------------------------------------------------------------------------
def _contract_case(n=br.CONTRACT_N):
    tb = _cached(("contract", n), lambda: br.tables(br.contract_forest(n), "branch"))
    return tb, _oracle(("contract", n), tb)


def _contract_ref(n, gs):
    return _cached(("contract-ref", n, tuple(int(x) for x in gs)), lambda: br.contract_reference(_contract_case(n)[1], gs))


def _group_starts():
    out = {f"groups_{k}": br.contract_groups(br.CONTRACT_N, k) for k in br.CONTRACT_GROUPS}
    out["half_and_singles"] = br.contract_half_and_singles(br.CONTRACT_N)
    out["singles"] = np.arange(br.CONTRACT_N + 1, dtype=np.int32)
    return out


@pytest.mark.parametrize("case", sorted(_group_starts()))
def test_contraction_keeps_negative_maxima(dev, case):
    gs = _group_starts()[case]
    tb, w_ref = _contract_case()
    ref = _contract_ref(br.CONTRACT_N, gs)
    ng = len(gs) - 1
    if ng > 2:
        assert (ref < 0).any()  # a block whose maximum is negative: a maximum started at 0 would lose it
    dtab = dev.upload(tb)
    try:
        g = dtab.build()
        _dirty(dev, ng, br.ld_of(ng))
        c = g.contract(gs)
        try:
            assert c.shape == (ng, 0, ng)
            _check_raw(c, ng, ref, f"contract {case}")
            assert np.array_equal(c.download(), ref)
        finally:
            c.free()
    finally:
        dtab.free()


def test_contraction_on_two_ranks_and_a_straddling_split(dev):
    n = br.CONTRACT_N
    tb, w_ref = _contract_case()
    gs = br.contract_groups(n, 257)
    ref = _contract_ref(n, gs)
    at = 100  # rank 1 starts at group 100 (g_begin > 0), on a group boundary
    splits = [0, int(gs[at]), n]
    bad_splits = [0, int(gs[at]) + 1, n] if gs[at + 1] - gs[at] > 1 else None
    if bad_splits is None:  # (group `at` has one member: take the next group of two or more)
        k = next(i for i in range(1, len(gs) - 1) if gs[i + 1] - gs[i] > 1)
        bad_splits = [0, int(gs[k]) + 1, n]

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        try:
            g = dtab.build(bad_splits[rank], bad_splits[rank + 1])
            with pytest.raises(nv.ScsError, match="straddles") as exc:
                g.contract(gs)
            assert exc.value.code == nv.EINVAL
            g.free()
            g = dtab.build(splits[rank], splits[rank + 1])
            c = g.contract(gs)
            try:
                raw, info = c.raw(0)
                return c.shape, raw, c.download()
            finally:
                c.free()
        finally:
            dtab.free()

    out = _ranks(2, rank_fn)
    bounds = [0, at, len(gs) - 1]
    for rank, (shape, raw, w) in enumerate(out):
        lo, hi = bounds[rank], bounds[rank + 1]
        assert shape == (len(gs) - 1, lo, hi)
        assert np.array_equal(w, ref[lo:hi]), rank
        assert np.array_equal(raw[:, :len(gs) - 1], ref[lo:hi]) and not raw[:, len(gs) - 1:].view(np.uint64).any(), rank


# ---------------------------------------------------------------------------------------------------------------
# refusals: argument checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------
def test_build_refusals(dev):
    tb, _ = _size_case(513, "branch")
    dtab = dev.upload(tb)
    try:
        with pytest.raises(nv.ScsError, match="multiple of 256") as exc:
            dtab.build(64, 513, upper=True)
        assert exc.value.code == nv.EINVAL
        handle, stats = nv.C.c_void_p(), nv.BuildStats()
        rc = dev._lib.scs_pcg_build(dev._ctx, dtab._h, 0, 513, nv.BUILD_MONOTONE | nv.BUILD_SHARED | nv.BUILD_UPPER,
                                    nv.C.byref(handle), nv.C.byref(stats))
        assert rc == nv.EINVAL and b"exclude each other" in dev._lib.scs_last_error() and not handle.value
        with pytest.raises(nv.ScsError, match="SCS_BUILD_SCATTER") as exc:
            dtab.build(0, 512, scatter=True)
        assert exc.value.code == nv.EUNSUP
    finally:
        dtab.free()


def test_upper_graphs_have_no_image_and_do_not_contract(dev):
    n, splits = 513, [0, 256, 513]
    tb, w_ref = _size_case(n, "branch")

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], upper=True)
        try:
            with pytest.raises(nv.ScsError) as exc:
                g.raw(1)
            assert exc.value.code == nv.EUNSUP
            with pytest.raises(nv.ScsError, match="SCS_BUILD_UPPER") as exc:
                g.contract(np.arange(n + 1, dtype=np.int32))
            assert exc.value.code == nv.EUNSUP
            raw, info = g.raw(0)
            return raw, info, g.download()
        finally:
            g.free()
            dtab.free()

    out = _ranks(2, rank_fn)
    for rank, (raw, info, w) in enumerate(out):
        rb, re_ = splits[rank], splits[rank + 1]
        assert info["col0"] == rb and info["ld"] == br.ld_of(n - rb)
        # defined: from the row's 256-column diagonal tile on; the padding behind column n is zero
        keep = np.arange(n)[None, :] >= (np.arange(rb, re_) // 256 * 256)[:, None]
        assert np.array_equal(w, np.where(keep, w_ref[rb:re_], 0.0))
        assert np.array_equal(raw[:, : n - rb][keep[:, rb:]], w_ref[rb:re_][keep])
        assert not raw[:, n - rb:].view(np.uint64).any()
