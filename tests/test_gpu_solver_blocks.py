"""The kernels inside the LOBPCG loop, one at a time, against extended-precision host references with error budgets
derived from the arithmetic (``solver_reference``; needs an MI355X): the operator on the symmetric upper-tile
schedule (``k_symm_tri``, W and the single-precision image, tile list forwards and backwards) and on ``k_symm``, the
Gram kernels and ``k_update`` on the strided column blocks the solver passes, and the Rayleigh-Ritz Jacobi on the
matrices it meets.  Every comparison is elementwise; a failure names the worst error / budget ratio and its index.

``SCS_BLOCK_RATIOS=<file>`` writes the worst ratio per family at the end of the run (informational: a later kernel
rewrite can see whether it moved; nothing gates on it)."""

import os

import numpy as np
import pytest
import solver_reference as ref

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import synthetic
from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

RATIOS: dict = {}


def _note(family: str, ratio: float, case: str) -> None:
    if family not in RATIOS or ratio > RATIOS[family][0]:
        RATIOS[family] = (ratio, case)


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    _drop_graph()
    d.close()
    out = os.environ.get("SCS_BLOCK_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("# worst measured error / budget (Jacobi: error / bar) per family, and the case it came from\n")
            for family in sorted(RATIOS):
                f.write(f"{family}\t{RATIOS[family][0]:.3e}\t{RATIOS[family][1]}\n")


# one graph at a time stays resident (W of 8 191 vertices is half a gigabyte on the host)
_GRAPH: dict = {}


def _drop_graph() -> None:
    if _GRAPH:
        _GRAPH["g"].free()
        _GRAPH["dtab"].free()
        _GRAPH.clear()


def _graph(dev, kind: str, v: int):
    """(graph, downloaded W) of a synthetic set of 3 - 6 trees: ``full`` covers every taxon in every tree, ``partial``
    leaves taxa out (isolated vertices: zero degrees), ``contracted`` merges random consecutive index ranges of a
    partial one down to ``v // 5`` groups.  W's own bit-exactness is test_gpu_parity's job: it is taken as downloaded."""
    if _GRAPH.get("key") != (kind, v):
        _drop_graph()
        if kind == "full":
            tables = synthetic.make_tables(v, v, 4, "branch", random_weights=True)
        else:
            tables = synthetic.make_tables(v, v, 3, "branch", leaves_per_tree=int(0.6 * v))
        dtab = dev.upload(tables)
        g = dtab.build()
        if kind == "contracted":
            cuts = np.random.RandomState(v).choice(np.arange(1, v), v // 5 - 1, replace=False)
            g = g.contract(np.unique(np.concatenate([[0, v], cuts])).astype(np.int32))
        _GRAPH.update(key=(kind, v), g=g, dtab=dtab, w=g.download())
    return _GRAPH["g"], _GRAPH["w"]


def _check_products(ys, want, budget, family: str, case: str, where) -> None:
    for r in range(len(ys)):
        ratio, at = ref.worst(ys[r], want, budget)
        _note(family, ratio, case)
        assert ratio <= 1.0, f"{case}, application {r}: error / budget {ratio:.3e} at row {at[0]} column {at[1]} ({where(at[0])})"


# ---------------------------------------------------------------------------------------------------------------
# operator, symmetric schedule
# ---------------------------------------------------------------------------------------------------------------
def _tri_tiles(v: int, tw: int) -> int:
    """Tiles on and above the diagonal: 128-row blocks, ``tw``-column tiles from the one holding the diagonal on."""
    return sum(-(-v // tw) - i * 128 // tw for i in range(-(-v // 128)))


def _tri_case(dev, kind: str, v: int, mode: str, graded: bool = False):
    g, w = _graph(dev, kind, v)
    b, image = (8 if mode == "w_b8" else 4), mode == "image_b4"
    x = ref.apply_vectors(v, b, v + b, graded)
    ys, info = g.apply_ex(x, image=image, reps=3)
    tw = 512 if image else 256
    # what ran: the symmetric schedule, on the image where asked, over every tile, three times
    assert info == {"symmetric": 1, "image": int(image), "tiles": _tri_tiles(v, tw), "segments": 1, "tile_width": tw,
                    "n_apply32": 3 * int(image), "partial": 0, "matrix_free": 0}, info
    case = f"{kind} V={v} {mode}" + (" graded" if graded else "")
    want, budget = ref.apply_reference(w, x, w_op=ref.image_model(w) if image else None)
    _check_products(ys, want, budget, "apply_tri_image" if image else "apply_tri_w", case,
                    lambda r: f"row block {r // 128}, column tile {r // tw}, {v - r} rows from the end")
    # forwards, backwards, forwards: every tile writes its own slabs, so the order cannot touch a bit
    for r in (1, 2):
        diff = np.flatnonzero((ys[r] != ys[0]).any(axis=1))
        assert len(diff) == 0, f"{case}: application {r} differs from application 0 in {len(diff)} rows, first {diff[0]}"
    return w, want, ys


@pytest.mark.parametrize("mode", ["w_b4", "w_b8", "image_b4"])
@pytest.mark.parametrize("v", ref.TRI_SIZES)
def test_symmetric_schedule_matches_reference(dev, v, mode):
    # on, one past and one short of the 128-row tile, the 256- and 512-column tiles and the leading dimension's 512
    _tri_case(dev, "full", v, mode)


@pytest.mark.parametrize("mode", ["w_b4", "w_b8", "image_b4"])
def test_symmetric_schedule_with_isolated_vertices(dev, mode):
    # (built as test_symmetric_schedule_with_isolated_vertices_converges builds its graphs)
    w, want, ys = _tri_case(dev, "partial", 4501, mode)
    dead = np.flatnonzero(w.sum(axis=0) == 0)
    assert len(dead) > 100
    assert not ys[:, dead, :].any() and not want[dead].any()  # zero degree: scale 1, a zero row


@pytest.mark.parametrize("mode", ["w_b4", "w_b8", "image_b4"])
def test_symmetric_schedule_with_graded_columns(dev, mode):
    # columns of magnitude 1, 1e-8, 1e+8: the budget of an entry is that of ITS column
    _tri_case(dev, "full", 4607, mode, graded=True)


def _default_solve(g, monkeypatch, block: int) -> dict:
    for name in ("SCS_LOWP", "SCS_LOWP_MAX_BYTES", "SCS_SPLIT_SMALL", "SCS_FOLD_PASS2", "SCS_LEGACY_LOOP"):
        monkeypatch.delenv(name, raising=False)
    try:
        return g.fiedler(None, block=block)[1]
    except nv.ConvergenceError as e:
        return e.stats


def test_the_image_is_refused_where_the_solver_streams_none(dev, monkeypatch):
    g, _ = _graph(dev, "full", 513)
    with pytest.raises(RuntimeError, match="scs_debug_apply_ex"):
        g.apply_ex(ref.apply_vectors(513, 4, 1), image=True)
    with pytest.raises(RuntimeError, match="block width 4"):
        g.apply_ex(ref.apply_vectors(513, 8, 1), image=True)
    # one predicate (solver::image_layout) answers the export and scs_fiedler: held where it switches, by both
    g, _ = _graph(dev, "full", 4095)
    with pytest.raises(RuntimeError, match="no image"):
        g.apply_ex(ref.apply_vectors(4095, 4, 1), image=True)
    assert _default_solve(g, monkeypatch, 4)["n_apply32"] == 0
    g, _ = _graph(dev, "full", 4096)
    _, info = g.apply_ex(ref.apply_vectors(4096, 4, 1), image=True)
    assert info["image"] == 1, info
    assert _default_solve(g, monkeypatch, 4)["n_apply32"] > 0
    with pytest.raises(RuntimeError, match="block width 4"):
        g.apply_ex(ref.apply_vectors(4096, 8, 1), image=True)
    assert _default_solve(g, monkeypatch, 8)["n_apply32"] == 0


# ---------------------------------------------------------------------------------------------------------------
# operator, k_symm
# ---------------------------------------------------------------------------------------------------------------
def _symm_segments(n: int, b: int) -> int:
    """The column segments ``solver::launch_symm`` cuts a k_symm launch into (whole graph on one device): enough
    workgroups to fill the chip, at most four, at most one per macro chunk of the padded row.  This restates the
    launch heuristic, so the assertion on it says what ran (launches of one to four segments), it is no independent
    check: a change of the heuristic fails it for no numerical reason and is answered by restating the rule here."""
    rpw, sdepth = (2 if b == 16 else 4), (4 if b == 4 else 2)
    rowblocks = -(-n // (4 * rpw))
    n_macros = -(-n // 512) * 512 // (sdepth * 128)
    nseg = max(1, min(-(-1024 // rowblocks), 4, n_macros))
    if b == 8 and nseg < 2 and n_macros >= 2 and rowblocks < 2048:
        nseg = 2
    mps = -(-n_macros // nseg)
    return -(-n_macros // mps)


# the sizes below run launches of one, two, three and four segments
assert [_symm_segments(*c) for c in ((129, 4), (129, 8), (1023, 4), (1025, 12), (2500, 8), (4097, 16))] == [1, 2, 2, 3, 4, 2]


def _symm_case(dev, kind: str, v: int, b: int, graded: bool = False):
    g, w = _graph(dev, kind, v)
    n = w.shape[0]
    x = ref.apply_vectors(n, b, v + b, graded)
    ys, info = g.apply_ex(x, reps=2)
    assert info["symmetric"] == 0 and info["image"] == 0 and info["tiles"] == 0 and info["n_apply32"] == 0, info
    assert info["segments"] == _symm_segments(n, b) and info["partial"] == 0 and info["matrix_free"] == 0, info
    case = f"{kind} V={n} b={b} segments={info['segments']}"
    want, budget = ref.apply_reference(w, x)
    _check_products(ys, want, budget, "apply_symm", case, lambda r: f"{n - r} rows from the end")
    assert np.array_equal(ys[0], ys[1]), case


@pytest.mark.parametrize("b", ref.WIDTHS)
@pytest.mark.parametrize("v", ref.SYMM_SIZES)
def test_symm_matches_reference(dev, v, b):
    _symm_case(dev, "full", v, b)


@pytest.mark.parametrize("b", [12, 16])
def test_symm_keeps_the_wide_blocks_above_4096(dev, b):
    _symm_case(dev, "full", 4097, b)


@pytest.mark.parametrize("b", ref.WIDTHS)
def test_symm_on_a_contracted_graph(dev, b):
    # 1 500 vertices merged into 300 groups: the leading dimension is the contracted graph's own (512)
    _symm_case(dev, "contracted", 1500, b, graded=(b == 8))


# ---------------------------------------------------------------------------------------------------------------
# Gram products and panel updates
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.PANEL_ROWS)
@pytest.mark.parametrize("b", ref.WIDTHS)
@pytest.mark.parametrize("pattern", ref.GRAM_PATTERNS)
def test_gram_on_the_solvers_blocks(dev, pattern, b, n):
    a, a0, ka, bm, b0, kb = ref.gram_case(pattern, b, n)
    want, budget = ref.gram_reference(a[:, a0:a0 + ka], bm[:, b0:b0 + kb])
    for use_mfma in (False, True):
        for blocks in ref.GRAM_BLOCKS:
            got = dev.debug_gram_ex(a, a0, ka, bm, b0, kb, use_mfma, blocks)
            ratio, at = ref.worst(got, want, budget)
            _note("gram_mfma" if use_mfma else "gram_valu", ratio, f"{pattern} b={b} n={n} blocks={blocks}")
            assert ratio <= 1.0, (f"{pattern} b={b} n={n} {'mfma' if use_mfma else 'valu'} gram_blocks={blocks}: "
                                  f"error / budget {ratio:.3e} at entry {at} (got {got[at]!r}, want {float(want[at])!r})")


@pytest.mark.parametrize("n", ref.PANEL_ROWS)
@pytest.mark.parametrize("b", ref.WIDTHS)
@pytest.mark.parametrize("pattern", ref.UPDATE_PATTERNS)
def test_update_on_the_solvers_blocks(dev, pattern, b, n):
    for alpha in (0.0, 1.0):
        for sign in (1.0, -1.0):
            y, y0, kc, a, a0, ka, c = ref.update_case(pattern, b, n, alpha)
            before = y.copy()
            a_before = before if a is y else a.copy()
            want, budget = ref.update_reference(before[:, y0:y0 + kc], alpha, a_before[:, a0:a0 + ka], c, sign)
            dev.debug_update(y, y0, kc, alpha, a, a0, ka, c, sign)
            case = f"{pattern} b={b} n={n} alpha={alpha} sign={sign}"
            ratio, at = ref.worst(y[:, y0:y0 + kc], want, budget)
            _note("update", ratio, case)
            assert ratio <= 1.0, f"{case}: error / budget {ratio:.3e} at row {at[0]} column {at[1]}"
            # the columns beside the block (sentinels, or the other blocks of the panel): not a bit moved
            keep = np.ones(y.shape[1], dtype=bool)
            keep[y0:y0 + kc] = False
            assert np.array_equal(y[:, keep], before[:, keep]), case
            if a is not y:
                assert np.array_equal(a, a_before), case


# ---------------------------------------------------------------------------------------------------------------
# Jacobi
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ref.JACOBI_SIZES)
@pytest.mark.parametrize("family", ref.JACOBI_FAMILIES)
def test_jacobi_on_the_matrices_the_solver_meets(dev, family, n):
    a = ref.jacobi_case(family, n)
    w, v = dev.debug_jacobi(a)
    assert np.isfinite(w).all() and np.isfinite(v).all()
    assert np.all(np.diff(w) <= 0), f"{family} n={n}: eigenvalues not descending"
    # test_jacobi_matches_lapack's three bars, with scale = max(1, ||A||).  The two badly scaled families are
    # judged on A / ||A|| (eigenvalues divided likewise): the bars are absolute once the scale is 1, and an
    # absolute 1e-12 means nothing at 1e+150 and everything at 1e-150.
    dw, res, orth, scale = ref.jacobi_errors(a, w, v, normalise=family.startswith("gauss_1e"))
    for what, err, bar in (("eig", dw, 1e-12 * scale), ("res", res, 1e-11 * scale), ("orth", orth, 1e-12)):
        _note(f"jacobi_{what}", err / bar, f"{family} n={n}")
    assert dw <= 1e-12 * scale, f"{family} n={n}: eigenvalues off by {dw:.3e} (scale {scale:.3e})"
    assert res <= 1e-11 * scale, f"{family} n={n}: residual {res:.3e} (scale {scale:.3e})"
    assert orth <= 1e-12, f"{family} n={n}: V^T V - I {orth:.3e}"
