"""What a solve runs only when it has more than one rank, held per entry to the longdouble reference at the edges of
its two layouts: the row slices through ``k_symm``, the all-gather and ``k_unpack`` or
``k_gram_qaq<B, 2>`` -- a rank of one row, slices of unequal length whose chunks have a tail nobody may read, every
block width --, the upper-triangle job's partial products through ``k_symm_tri`` / ``k_symm_tri_finish`` with a rank's
own row blocks and ``k_sum_parts`` or ``k_gram_qaq<B, 3>``, and its degrees (``k_degrees_upper_rows`` / ``_cols``); then
whole solves at the same edges, with and without ``SCS_FOLD_PASS2=0``, for the fused loop's own copy of the assembly.
The ranks are threads on device 0 (``scs_local_group_create``); ``tests/team_reference.py`` has the model and the
cases, ``tests/test_team_reference_cpu.py`` proves both without a device.

A rank function makes the same collective calls on every rank and asserts nothing: a rank that left early would leave
the others waiting for it.  It returns what it got; everything is compared after all ranks have returned."""

import os
import threading

import build_reference as br
import numpy as np
import pytest
import solver_reference as sr
import team_reference as tr

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import synthetic
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.partition import row_splits_upper

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


_CACHE: dict = {}
_RATIOS: dict = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _note(family, ratio, what):
    if ratio >= _RATIOS.get(family, (-1.0, ""))[0]:
        _RATIOS[family] = (ratio, what)


def _ranks(world, fn):
    """``fn(rank, device)`` on ``world`` in-process ranks of device 0, a host thread each; returns their results."""
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

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is still inside a collective"
    lib.scs_local_group_destroy(group)
    assert err == [None] * world, err
    return out


def _graph(dev, key, make_tables):
    """``(tables, W)`` of a case: W downloaded once from the one-device build and left unchanged."""
    tb = _cached(("tables",) + key, make_tables)

    def download():
        dtab = dev.upload(tb)
        g = dtab.build()
        try:
            w = g.download()
        finally:
            g.free()
            dtab.free()
        w.flags.writeable = False
        return w

    return tb, _cached(("w",) + key, download)


def _apply_graph(dev, n, lone):
    return _graph(dev, ("apply", n, tuple(lone)), lambda: br.tables(tr.apply_forest(n, lone), "branch"))


def _apply_ref(key, w, x, image):
    return _cached(("ref",) + key, lambda: sr.apply_reference(w, x, w_op=sr.image_model(w) if image else None))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _team_apply(tb, splits, panels, paths, image=False, upper=False):
    """Every rank: the graph of its rows, then ``team_apply`` for each (name, path) -- the same calls in the same
    order on every rank; ``out[rank][(name, path)] = (y, qaq, part, info)``."""

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], shared=not upper, upper=upper)
        try:
            return {(name, path): g.team_apply(q, aq, path=path, image=image, reps=tr.REPS)
                    for name, (q, aq) in panels.items() for path in paths}
        finally:
            g.free()
            dtab.free()

    return _ranks(len(splits) - 1, rank_fn)


def _check_product(family, what, out, key, w, n, b, q, aq, lone, image=False):
    """What every case asserts of one (operand, path): the same bits on every rank and in every application, the
    product of application 0 per entry inside the apply budget, +0.0 in the rows of degree 0, and (path 1) Q^T AQ
    inside the Gram budget of the block that was returned."""
    y0, qaq0, _, _ = out[0][key]
    for rank, res in enumerate(out):
        assert _same_bits(res[key][0], y0), f"{what}: rank {rank} holds other bits than rank 0"
        if qaq0 is not None:
            assert _same_bits(res[key][1], qaq0), f"{what}: Q^T AQ of rank {rank} differs from rank 0's"
    for rep in range(1, tr.REPS):
        assert _same_bits(y0[rep], y0[0]), f"{what}: application {rep} differs from application 0"
        if qaq0 is not None:
            assert _same_bits(qaq0[rep], qaq0[0]), f"{what}: Q^T AQ of application {rep} differs"
    want, budget = _apply_ref((n, tuple(lone), b, key[0], image), w, q[:, 2 * b:], image)
    ratio, at = sr.worst(y0[0], want, budget)
    _note(family, ratio, what)
    print(f"[{family}] {what}: worst error / budget = {ratio:.4f} at {at}")
    assert ratio <= 1.0, f"{what}: entry {at} is {y0[0][at]!r}, reference {float(want[at])!r}: {ratio:.3g} budgets off"
    for v in lone:
        assert not y0[0][v].any() and not np.signbit(y0[0][v]).any(), f"{what}: row {v} has degree 0: {y0[0][v]}"
    if qaq0 is not None:
        ref, gb = tr.qaq_reference(q, aq, y0[0])
        ratio, at = sr.worst(qaq0[0], ref, gb)
        _note(family + " gram", ratio, what)
        print(f"[{family} gram] {what}: worst error / budget = {ratio:.4f} at {at}")
        assert ratio <= 1.0, f"{what}: (Q^T AQ){at} is {qaq0[0][at]!r}, reference {float(ref[at])!r}: {ratio:.3g} budgets off"


# ---------------------------------------------------------------------------------------------------------------
# row slices: k_symm on a rank's rows, the all-gather, k_unpack (path 0) or k_gram_qaq<B, 2> (path 1)
# ---------------------------------------------------------------------------------------------------------------
def _row_case(dev, case, b, image=False):
    n, splits = case
    world = len(splits) - 1
    lone = tr.lone_rows(splits)
    tb, w = _apply_graph(dev, n, lone)
    panels = {name: tr.panels(n, b, 7, graded) for name, graded in (("x", False), ("graded", True))}
    paths = (0, 1) if b in tr.FUSED_WIDTHS else (0,)
    out = _team_apply(tb, splits, panels, paths, image=image)
    for key in [(name, path) for name in panels for path in paths]:
        q, aq = panels[key[0]]
        what = f"V={n} splits={list(splits)} b={b} {key[0]} path {key[1]}" + (" image" if image else "")
        for rank, res in enumerate(out):
            info = res[key][3]
            assert info["partial"] == 0 and info["path"] == key[1] and info["world"] == world, (what, rank, info)
            assert info["chunk"] == tr.chunk_of(splits, b) and info["tiles"] == 0, (what, rank, info)
            assert info["n_apply32"] == (tr.REPS if image else 0) and info["n_allgather"] == tr.REPS, (what, rank, info)
            assert 1 <= info["segments"] <= 4 and res[key][2] is None, (what, rank, info)
        _check_product("rows image" if image else "rows", what, out, key, w, n, b, q, aq, lone, image)


@pytest.mark.parametrize("b", tr.WIDTHS)
@pytest.mark.parametrize("case", tr.ROW_CASES, ids=tr.case_id)
def test_row_slices_are_assembled_on_every_rank(dev, case, b):
    _row_case(dev, case, b)


@pytest.mark.parametrize("image", [False, True], ids=["w", "image"])
@pytest.mark.parametrize("case", tr.IMAGE_CASES, ids=tr.case_id)
def test_row_slices_where_the_image_is_streamed(dev, case, image):
    _row_case(dev, case, 4, image)


def test_no_image_is_refused_on_every_rank_alike(dev):
    n, splits = 700, (0, 333, 700)
    tb, _ = _apply_graph(dev, n, tr.lone_rows(splits))
    q, aq = tr.panels(n, 4, 7)

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], shared=True)
        try:
            g.team_apply(q, aq, path=0, image=True)
        except nv.ScsError as e:
            got = (e.code, str(e))
        else:
            got = None
        after = g.team_apply(q, aq, path=0)  # (all ranks left the refusal at the same place: the next collective meets)
        g.free()
        dtab.free()
        return got, after[0]

    out = _ranks(2, rank_fn)
    assert out[0][0] is not None and out[0][0][0] == nv.EUNSUP and "no image" in out[0][0][1], out[0][0]
    assert out[1][0] == out[0][0] and _same_bits(out[1][1], out[0][1]) and not np.isnan(out[0][1]).any()


# ---------------------------------------------------------------------------------------------------------------
# upper triangle: k_symm_tri on a rank's row blocks, k_symm_tri_finish with rb_lo / rb_hi, the all-gather of the
# partial products, k_sum_parts (path 0) or k_gram_qaq<B, 3> (path 1)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", tr.FUSED_WIDTHS)
@pytest.mark.parametrize("case", tr.UPPER_CASES, ids=tr.case_id)
def test_upper_partial_products_and_their_sum(dev, case, b):
    n, splits = case
    world = len(splits) - 1
    lone = tr.lone_rows(splits)
    tb, w = _apply_graph(dev, n, lone)
    panels = {name: tr.panels(n, b, 7, graded) for name, graded in (("x", False), ("graded", True))}
    out = _team_apply(tb, splits, panels, (0, 1), upper=True)
    dinv = _cached(("dinv", n, tuple(lone)), lambda: sr.scaling(w))
    for name, (q, aq) in panels.items():
        z = dinv[:, None] * q[:, 2 * b:].astype(tr.LD)
        for rank in range(world):
            ref, mag = _cached(("partial", case, b, name, rank), lambda r=rank: tr.upper_partial(w, splits, r, z))
            for path in (0, 1):
                what = f"V={n} splits={list(splits)} b={b} {name} path {path}"
                _, _, part, info = out[rank][(name, path)]
                assert info["partial"] == 1 and info["path"] == path and info["world"] == world, (what, rank, info)
                assert info["chunk"] == n * b and info["segments"] == world, (what, rank, info)
                assert info["tiles"] == tr.upper_tiles(n, splits, rank) and info["n_apply32"] == 0, (what, rank, info)
                assert info["n_allgather"] == tr.REPS, (what, rank, info)
                for rep in range(1, tr.REPS):  # (the tile list runs forwards, backwards, forwards)
                    assert _same_bits(part[rep], part[0]), f"{what}: rank {rank}'s partial product changes with the tile order"
                ratio, at = sr.worst(part[0], ref, sr.apply_budget(n, mag))
                _note("upper partial", ratio, f"{what} rank {rank}")
                assert ratio <= 1.0, (f"{what}: RANK {rank}'s partial product, entry {at}, is {part[0][at]!r}, "
                                      f"reference {float(ref[at])!r}: {ratio:.3g} budgets off")
        for path in (0, 1):
            _check_product("upper", f"V={n} splits={list(splits)} b={b} {name} path {path}", out, (name, path), w, n, b,
                           q, aq, lone)


def test_upper_job_refuses_width_12_on_every_rank_alike(dev):
    n, splits = 769, tuple(row_splits_upper(769, 3))
    tb, _ = _apply_graph(dev, n, tr.lone_rows(splits))
    q, aq = tr.panels(n, 12, 7)
    q4, aq4 = tr.panels(n, 4, 7)

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], upper=True)
        try:
            g.team_apply(q, aq, path=0)
        except nv.ScsError as e:
            got = (e.code, str(e))
        else:
            got = None
        after = g.team_apply(q4, aq4, path=0)
        g.free()
        dtab.free()
        return got, after[0]

    out = _ranks(3, rank_fn)
    assert out[0][0] is not None and out[0][0][0] == nv.EUNSUP, out[0][0]
    assert "SCS_BUILD_UPPER graph is solved with block width 4 or 8 (asked: 12)" in out[0][0][1]
    for got, after in out[1:]:
        assert got == out[0][0] and _same_bits(after, out[0][1])


# ---------------------------------------------------------------------------------------------------------------
# the degrees of upper graphs: k_degrees_upper_rows / k_degrees_upper_cols, the gather, k_combine_degrees
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.UPPER_CASES, ids=tr.case_id)
def test_upper_degrees_on_every_rank(dev, case):
    n, splits = case
    lone = tr.lone_rows(splits)
    tb, w = _graph(dev, ("degree", n, tuple(lone)), lambda: br.tables(tr.degree_forest(n, lone), "branch"))
    assert (w < 0).any() and (w > 0).any()

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], upper=True)
        try:
            return g.degrees_all(), g.degrees()
        finally:
            g.free()
            dtab.free()

    out = _ranks(len(splits) - 1, rank_fn)
    deg = out[0][0]
    for rank, (deg_all, deg_own) in enumerate(out):
        assert _same_bits(deg_all, deg), rank
        assert _same_bits(deg_own, deg[splits[rank]:splits[rank + 1]]), rank
    ref, budget = br.degrees_reference(w)
    err = np.abs(deg.astype(br.LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.max(np.where(err == 0, 0.0, err / budget).astype(np.float64)))
    _note("upper degrees", ratio, f"V={n} splits={list(splits)}")
    print(f"[upper degrees] V={n} splits={list(splits)}: worst error / budget = {ratio:.4f}")
    bad = np.flatnonzero(~(err <= budget))
    assert not len(bad), f"rows {bad[:5].tolist()} off by {err[bad][:5]} > {budget[bad][:5]}"
    for v in lone:  # (that their scale is 1 and not 1 / sqrt(0) is what keeps the products above free of NaN)
        assert not w[v].any() and deg[v] == 0.0 and not np.signbit(deg[v]), v


# ---------------------------------------------------------------------------------------------------------------
# whole solves at the same edges: panel_gram_tf_body<B, 2 | 3> by default, k_gram_qaq under SCS_FOLD_PASS2=0
# ---------------------------------------------------------------------------------------------------------------
SOLVES = {
    "upper-b8-2": ("upper", 1300, tuple(row_splits_upper(1300, 2)), 8, False),
    "upper-b8-3": ("upper", 1300, tuple(row_splits_upper(1300, 3)), 8, False),
    "rows-b8": ("rows", 700, (0, 100, 290, 700), 8, False),
    "rows-b12": ("rows", 700, (0, 100, 290, 700), 12, False),
    "rows-b16": ("rows", 700, (0, 100, 290, 700), 16, False),
    "rows-isolated": ("rows", 700, (0, 333, 700), 0, True),
    "upper-isolated": ("upper", 1300, tuple(row_splits_upper(1300, 3)), 0, True),
}


def _solve_lone(splits):
    """Two lone vertices next to a rank boundary, not on it: a row that is all zero would hide a slice read from the
    wrong place, and in a whole solve the tail of a chunk holds zeros, not NaN."""
    return [int(splits[1]) - 2, int(splits[1]) + 1]


def _solve_tables(n, splits, isolated):
    lone = _solve_lone(splits) if isolated else []
    arrays = synthetic.tree_arrays(31, n - len(lone), 18, leaves_per_tree=n - len(lone) - 57, random_weights=True)
    return br.tables(tr.with_lone(arrays, lone) if isolated else arrays, "branch")


@pytest.mark.parametrize("fold", ["default", "fold_pass2_off"])
@pytest.mark.parametrize("name", sorted(SOLVES))
def test_whole_solves_at_the_edges(dev, monkeypatch, name, fold):
    layout, n, splits, block, isolated = SOLVES[name]
    monkeypatch.delenv("SCS_FOLD_PASS2", raising=False)
    monkeypatch.delenv("SCS_LOWP", raising=False)
    tb = _cached(("solve-tables", n, splits, isolated), lambda: _solve_tables(n, splits, isolated))
    v0 = np.random.RandomState(0).uniform(-1, 1, n)

    def single():
        dtab = dev.upload(tb)
        g = dtab.build()
        try:
            maps, stats = g.fiedler(v0)
            return maps, stats, g.download()
        finally:
            g.free()
            dtab.free()

    maps_single, stats_single, w = _cached(("solve-single", n, splits, isolated), single)
    # the comparison is well posed: the one-device solve converged and the Fiedler value is separated
    assert stats_single["converged"] == 1
    assert stats_single["lambda"][1] - stats_single["lambda_next"] >= 1e-3, stats_single
    lone = _solve_lone(splits) if isolated else []
    assert [v for v in range(n) if not w[v].any()] == lone
    if fold == "fold_pass2_off":
        monkeypatch.setenv("SCS_FOLD_PASS2", "0")

    def rank_fn(rank, d):
        dtab = d.upload(tb)
        g = dtab.build(splits[rank], splits[rank + 1], shared=layout == "rows", upper=layout == "upper")
        try:
            return g.fiedler(v0, block=block)
        except nv.ConvergenceError as e:
            return e.maps, e.stats
        finally:
            g.free()
            dtab.free()

    out = _ranks(len(splits) - 1, rank_fn)
    _, dd = to.normalized_operator(w)
    for rank, (maps, stats) in enumerate(out):
        assert stats["converged"] == 1, (rank, stats)
        assert stats["block"] == (block or 4) and stats["used_constraint"] == (0 if isolated else 1), (rank, stats)
        assert _same_bits(maps, out[0][0]), rank
        err = float(np.max(np.abs(maps[:, 1] - maps_single[:, 1])))
        err_unit = float(np.max(np.abs((maps[:, 1] - maps_single[:, 1]) * dd)))
        _note("solve (Fiedler column / 1e-10)", max(err, err_unit) / tr.FIEDLER_TOL, f"{name} {fold}")
        print(f"[solve] {name} {fold} rank {rank}: {err:.3e} / {err_unit:.3e}, {stats['iterations']} iterations")
        assert err <= tr.FIEDLER_TOL and err_unit <= tr.FIEDLER_TOL, (rank, err, err_unit)


def test_zz_worst_ratios_of_this_run():
    """The worst error / budget of every family over the cases that ran (``SCS_TEAM_RATIOS=<file>`` keeps them:
    ``profiles/team_edges_error_ratios.txt``); informational, every case has asserted its own."""
    lines = [f"{family}: worst error / budget = {ratio:.4f}  ({what})" for family, (ratio, what) in sorted(_RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("SCS_TEAM_RATIOS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(ratio <= 1.0 for ratio, _ in _RATIOS.values()), _RATIOS
