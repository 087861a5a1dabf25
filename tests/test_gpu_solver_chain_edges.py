"""Whole solves through the LOBPCG chain at the edges of its tall kernels' row groups (needs an MI355X).

The tall panel kernels (``k_panel_rr_solve``, ``k_panel_tf_solve``, ``k_panel_gram_tf_solve`` and the pass-1 role of
``k_symm_tri_tf``, ``csrc/scs_panel.h``) load the operands of a wave's first two groups of 16 rows BEFORE the small
solve they run in front of their rows, and the rotation that closes start-up and a confirmation sets its own masks
and turns X and S X in one launch.  The symmetric schedule and the image loop start at 4 096 vertices, so the shapes
are the smallest that run those kernels: 4 096 (every wave's last group full), 4 111 (the last group partial: rows
>= n load as 0.0 and are never stored) and 4 160 (a wave with two groups whose second is the last one).

Every solve is held to the extended-precision operator of ``solver_reference`` with its budget: the residual
``S x - lambda x`` of the returned pair, formed on the host from the downloaded W, must agree with the residual norm
the solver reports.  With x = maps / d^-1/2 scaled to unit length the two differ by at most

* the budget of one application, ``(2 V + 16) u (|S| |x|)`` entrywise (``apply_reference``), 2-norm;
* what recovering x from the embedding adds: every entry carries the device's d^-1/2 (relative error (V / 2 + 4) u,
  the same terms the apply budget counts) and one product, and ``||S - lambda|| <= 2``: ``(V + 8) u``;
* the residual norm itself, a Gram product over V rows: ``(V + 2) u`` relative;
* the rotation that closes start-up and confirmation (``X <- X T``, ``S X <- (S X) T``, sums of b + 1 terms, b <= 8,
  on both sides): ``4 (b + 3) u <= 44 u``.

The variants of one loop (``SCS_SPLIT_SMALL=1``, ``SCS_LOWP=0``) are held to the default within the tolerance of
``test_small_solves_in_front_of_the_tall_kernels_change_no_bit``."""

import numpy as np
import pytest
import solver_reference as ref

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import synthetic
from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

SIZES = (4096, 4111, 4160)
COUNTERS = ("iterations", "n_apply", "n_apply32", "lowp_renewals")


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    _drop_graph()
    d.close()


# one graph at a time stays resident, with its W and the extended-precision scaling
_GRAPH: dict = {}


def _drop_graph() -> None:
    if _GRAPH:
        _GRAPH["g"].free()
        _GRAPH["dtab"].free()
        _GRAPH.clear()


def _graph(dev, kind: str, v: int):
    if _GRAPH.get("key") != (kind, v):
        _drop_graph()
        if kind == "full":
            tables = synthetic.make_tables(v + 1, v, 12, "branch", random_weights=True)
        elif kind == "isolated":  # taxa that no tree holds: zero degrees, no constraint vector, two wanted columns
            tables = synthetic.make_tables(v, v, 3, "branch", leaves_per_tree=int(0.6 * v))
        elif kind == "planted":  # a model tree and a few SPR moves: a split that every tree supports
            tables = synthetic.make_tables(v + 7, v, 6, "branch", random_weights=True,
                                           planted_spr=int(np.ceil(0.02 * v)))
        else:
            raise ValueError(kind)
        dtab = dev.upload(tables)
        g = dtab.build()
        w = g.download()
        _GRAPH.update(key=(kind, v), g=g, dtab=dtab, w=w, dinv=ref.scaling(w))
    return _GRAPH["g"], _GRAPH["w"], _GRAPH["dinv"]


def _solve(g, monkeypatch, env=None, **kw):
    for name in ("SCS_SPLIT_SMALL", "SCS_LOWP", "SCS_FOLD_PASS2", "SCS_OVERLAP_PASS1", "SCS_LEGACY_LOOP"):
        monkeypatch.delenv(name, raising=False)
    for name, value in (env or {}).items():
        monkeypatch.setenv(name, value)
    try:
        maps, stats = g.fiedler(None, **kw)
    except nv.ConvergenceError as e:
        maps, stats = e.maps, e.stats
    finally:
        for name in env or {}:
            monkeypatch.delenv(name, raising=False)
    return maps, stats


_check_against_reference = ref.check_against_reference  # (host code, shared with tests/test_gpu_fiedler_edges.py)


def _same_pair(maps_a, stats_a, maps_b, stats_b, case: str):
    # (the tolerance of test_small_solves_in_front_of_the_tall_kernels_change_no_bit)
    assert stats_a["converged"] == 1 and stats_b["converged"] == 1, case
    assert abs(stats_a["iterations"] - stats_b["iterations"]) <= 3, (case, stats_a["iterations"], stats_b["iterations"])
    assert abs(stats_a["lambda"][1] - stats_b["lambda"][1]) <= 1e-13, case
    scale = float(np.max(np.abs(maps_a[:, 1])))
    assert float(np.max(np.abs(maps_a[:, 1] - maps_b[:, 1]))) <= 1e-10 * scale, case


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("v", SIZES)
def test_default_loop_at_the_group_edges(dev, monkeypatch, v, block):
    # width 4 streams the single-precision image, width 8 W itself; both run pass 1 inside the SYMM launch
    g, w, dinv = _graph(dev, "full", v)
    case = f"full V={v} b={block}"
    maps, stats = _solve(g, monkeypatch, block=block)
    assert stats["converged"] == 1 and stats["block"] == block and stats["used_constraint"] == 1, (case, stats)
    assert stats["iterations"] > 3 and (stats["n_apply32"] > 0) == (block == 4), (case, stats)
    _check_against_reference(w, dinv, maps, stats, case)
    # the same input again: the same bits, the same counters
    maps2, stats2 = _solve(g, monkeypatch, block=block)
    assert np.array_equal(maps, maps2), case
    assert stats["lambda"] == stats2["lambda"] and stats["resid"] == stats2["resid"], case
    for name in COUNTERS:
        assert stats[name] == stats2[name], (case, name)


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("v", SIZES)
def test_split_small_solves_against_the_default(dev, monkeypatch, v, block):
    # SCS_SPLIT_SMALL=1: k_panel_rr / k_panel_tf / k_gram_qaq with one-workgroup solves between them, through the
    # same load and compute parts; another sequence of roundings (no folded pass 2), the same pair
    g, w, dinv = _graph(dev, "full", v)
    case = f"full V={v} b={block} split"
    maps, stats = _solve(g, monkeypatch, block=block)
    maps_s, stats_s = _solve(g, monkeypatch, {"SCS_SPLIT_SMALL": "1"}, block=block)
    assert stats_s["n_apply32"] == 0, case  # (the image belongs to the fused loop)
    _check_against_reference(w, dinv, maps_s, stats_s, case)
    _same_pair(maps, stats, maps_s, stats_s, case)


@pytest.mark.parametrize("v", SIZES)
def test_all_double_loop_against_the_image_loop(dev, monkeypatch, v):
    g, w, dinv = _graph(dev, "full", v)
    case = f"full V={v} b=4 SCS_LOWP=0"
    maps, stats = _solve(g, monkeypatch, block=4)
    maps_d, stats_d = _solve(g, monkeypatch, {"SCS_LOWP": "0"}, block=4)
    assert stats["n_apply32"] > 0 and stats_d["n_apply32"] == 0, (case, stats, stats_d)
    assert stats_d["lowp_renewals"] == 0, (case, stats_d)
    _check_against_reference(w, dinv, maps_d, stats_d, case)
    assert stats_d["converged"] == 1, case
    assert abs(stats["lambda"][1] - stats_d["lambda"][1]) <= 1e-13, case
    scale = float(np.max(np.abs(maps[:, 1])))
    assert float(np.max(np.abs(maps[:, 1] - maps_d[:, 1]))) <= 1e-10 * scale, case


@pytest.mark.parametrize("lowp", ["image", "double"])
@pytest.mark.parametrize(("kind", "v"), [("isolated", 4111), ("planted", 4160)])
def test_isolated_vertices_and_a_planted_split(dev, monkeypatch, kind, v, lowp):
    g, w, dinv = _graph(dev, kind, v)
    case = f"{kind} V={v} {lowp}"
    dead = np.flatnonzero(w.sum(axis=0) == 0)
    assert (len(dead) > 100) == (kind == "isolated"), case
    maps, stats = _solve(g, monkeypatch, {"SCS_LOWP": "0"} if lowp == "double" else None)
    assert stats["converged"] == 1 and stats["block"] == 4, (case, stats)
    assert stats["used_constraint"] == (0 if kind == "isolated" else 1), (case, stats)
    assert (stats["n_apply32"] > 0) == (lowp == "image"), (case, stats)
    _check_against_reference(w, dinv, maps, stats, case)
    maps2, stats2 = _solve(g, monkeypatch, {"SCS_LOWP": "0"} if lowp == "double" else None)
    assert np.array_equal(maps, maps2), case
    for name in COUNTERS:
        assert stats[name] == stats2[name], (case, name)


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("how", ["max_iter_1", "loose_tol"])
def test_start_up_and_confirmation_alone(dev, monkeypatch, how, block):
    # one iteration (start-up, one trip round the chain, no confirmation), and a tolerance that the first
    # iterations meet (start-up, a few trips, the confirmation through W): on the shape with a partial last group
    g, w, dinv = _graph(dev, "full", 4111)
    case = f"full V=4111 b={block} {how}"
    # (the start block's residual is near 6e-3 and the default tolerance takes 16 - 20 iterations from there)
    kw = {"max_iter": 1} if how == "max_iter_1" else {"tol": 1e-5}
    maps, stats = _solve(g, monkeypatch, block=block, **kw)
    if how == "max_iter_1":
        assert stats["iterations"] == 1 and stats["converged"] == 0, (case, stats)
    else:
        assert stats["converged"] == 1 and stats["resid"][1] <= 1e-5, (case, stats)
        full = _solve(g, monkeypatch, block=block)[1]["iterations"]
        assert 1 <= stats["iterations"] < full, (case, stats["iterations"], full)
    # (one iteration of the image loop reports on the start-up product, which streams the image)
    _check_against_reference(w, dinv, maps, stats, case, image=how == "max_iter_1" and stats["n_apply32"] > 0)
    maps2, stats2 = _solve(g, monkeypatch, block=block, **kw)
    assert np.array_equal(maps, maps2), case
    for name in COUNTERS:
        assert stats[name] == stats2[name], (case, name)
