"""The host references and error budgets of ``solver_reference`` without a device: plain fp64 numpy sits inside every
budget (so a correct kernel can), the image model lies far outside the budget of W (so an image test cannot pass
on W, nor a W test on the image), LAPACK meets the Jacobi bars on every family, and the diagnostic entry points are
declared and bound."""

import re
from pathlib import Path

import numpy as np
import pytest
import solver_reference as ref

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native, synthetic


def test_extended_precision_is_there():
    ref.require_extended_precision()
    assert np.finfo(ref.LD).eps <= 2.0 ** -63


def _numpy_apply(w, x, w_op=None):
    deg = w.sum(axis=0)
    dinv = np.where(deg == 0, 1.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))
    return dinv[:, None] * ((w if w_op is None else w_op) @ (dinv[:, None] * x))


@pytest.fixture(scope="module")
def graphs():
    full = to.pcg_dense(synthetic.make_tables(5, 4225, 4, "branch", random_weights=True))[0]
    part = to.pcg_dense(synthetic.make_tables(11, 1500, 3, "branch", leaves_per_tree=900))[0]
    gs = np.unique(np.concatenate([[0, 1500], np.random.RandomState(3).choice(np.arange(1, 1500), 299, False)]))
    return {"full": full, "isolated": part, "contracted": to.contract_dense(part, gs.astype(np.int32))}


@pytest.mark.parametrize(("name", "b", "graded"), [("full", 4, False), ("full", 8, True), ("isolated", 12, False),
                                                   ("contracted", 16, True)])
def test_numpy_apply_is_inside_the_budget(graphs, name, b, graded):
    w = graphs[name]
    x = ref.apply_vectors(w.shape[0], b, 7, graded)
    want, budget = ref.apply_reference(w, x)
    ratio, at = ref.worst(_numpy_apply(w, x), want, budget)
    assert ratio <= 1.0, (ratio, at)
    if name == "isolated":
        dead = np.flatnonzero(w.sum(axis=0) == 0)
        assert len(dead) > 0 and not want[dead].any() and not budget[dead].any()  # zero rows, and nothing allowed
    if graded:  # the budget is per column: eight orders of magnitude apart
        col = np.asarray(budget.max(axis=0), dtype=np.float64)
        assert col[2] > 1e12 * col[1] > 0


def test_the_image_is_told_from_w(graphs):
    w = graphs["full"]
    w32 = ref.image_model(w)
    assert np.count_nonzero(w32 != w) > w.size // 4  # (branch lengths: hardly a weight is a float)
    x = ref.apply_vectors(w.shape[0], 4, 9)
    on_w, budget = ref.apply_reference(w, x)
    on_image, budget32 = ref.apply_reference(w, x, w_op=w32)
    got_w, got_image = _numpy_apply(w, x), _numpy_apply(w, x, w32)
    assert ref.worst(got_w, on_w, budget)[0] <= 1.0 and ref.worst(got_image, on_image, budget32)[0] <= 1.0
    # ... and each far outside the other's: the typical entry by two orders of magnitude, not one outlier
    for got, want, bud in ((got_image, on_w, budget), (got_w, on_image, budget32)):
        ratios = np.abs(got - want) / bud
        assert float(np.median(ratios)) > 100.0, float(np.median(ratios))


@pytest.mark.parametrize("n", [1, 5, 65, 4099, 100003])
@pytest.mark.parametrize("pattern", ref.GRAM_PATTERNS)
def test_numpy_gram_is_inside_the_budget(pattern, n):
    b = 4 if n > 5000 else 16
    a, a0, ka, bm, b0, kb = ref.gram_case(pattern, b, n)
    ab, bb = a[:, a0:a0 + ka], bm[:, b0:b0 + kb]
    assert np.abs(ab).max() < 100 and np.abs(bb).max() < 100  # (no sentinel inside the blocks)
    if pattern != "q_aq":
        assert (a == ref.SENTINEL).any() or (bm == ref.SENTINEL).any() or a is bm
    want, budget = ref.gram_reference(ab, bb)
    ratio, at = ref.worst(ab.T @ bb, want, budget)
    assert ratio <= 1.0, (ratio, at)
    wrong = ab.T @ bb
    wrong[-1, -1] -= ab[-1, -1] * bb[-1, -1]  # the last row dropped from one entry
    assert ref.worst(wrong, want, budget)[0] > 1.0


@pytest.mark.parametrize("n", [1, 5, 65, 4099])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("pattern", ref.UPDATE_PATTERNS)
def test_numpy_update_is_inside_the_budget(pattern, alpha, n):
    y, y0, kc, a, a0, ka, c = ref.update_case(pattern, 8, n, alpha)
    yb, ab = y[:, y0:y0 + kc], a[:, a0:a0 + ka]
    for sign in (1.0, -1.0):
        want, budget = ref.update_reference(yb, alpha, ab, c, sign)
        got = sign * (ab @ c) + (alpha * yb if alpha else 0.0)
        ratio, at = ref.worst(got, want, budget)
        assert ratio <= 1.0 and np.isfinite(np.asarray(want, dtype=np.float64)).all(), (ratio, at)


def test_worst_reports_nan_and_the_index():
    want = np.ones((3, 2), dtype=ref.LD)
    budget = np.full((3, 2), 1e-15, dtype=ref.LD)
    got = np.ones((3, 2))
    assert ref.worst(got, want, budget) == (0.0, (0, 0))
    got[2, 1] += 1e-14
    ratio, at = ref.worst(got, want, budget)
    assert at == (2, 1) and 9.0 < ratio < 11.0
    got[1, 0] = np.nan
    assert ref.worst(got, want, budget) == (float("inf"), (1, 0))
    budget[0, 1] = 0.0
    got[1, 0] = 1.0
    assert ref.worst(got, want, budget)[0] < 11.0  # (no error over a zero budget: fine)
    got[0, 1] = 1.0 + 1e-15
    assert ref.worst(got, want, budget) == (float("inf"), (0, 1))


@pytest.mark.parametrize("n", ref.JACOBI_SIZES)
@pytest.mark.parametrize("family", ref.JACOBI_FAMILIES)
def test_lapack_meets_the_jacobi_bars(family, n):
    a = ref.jacobi_case(family, n)
    assert np.array_equal(a, a.T)
    w, v = np.linalg.eigh(a)
    w, v = w[::-1], v[:, ::-1]
    dw, res, orth, scale = ref.jacobi_errors(a, w, v, family.startswith("gauss_1e"))
    assert dw <= 1e-12 * scale and res <= 1e-11 * scale and orth <= 1e-12
    if family == "cluster":
        assert 0.99 < w[-1] <= w[0] < 1.0 and w[0] - w[-1] <= 1.01e-13 * (n - 1) + 1e-15
    if family == "ritz":
        assert 0 < np.abs(a - np.diag(np.diag(a))).max() < 1e-8 and 0.89 < w[-1] <= w[0] < 1.01
        assert w[0] - w[1] < 1e-8  # (the two values 1e-12 apart, split further by the perturbation only)
    if family == "graded" and n > 3:
        assert w[0] > 0.9 and abs(w[-1]) < 1e-14
    if family == "rank_one":
        assert np.linalg.matrix_rank(a) == 1
    if family == "repeated" and n >= 12:
        assert np.sum(np.abs(w - 1.0) < 1e-14) >= n // 3
    if family == "ritz_separated":
        # no sweep at all -- the diagonal as eigenvalues, the identity as vectors -- misses the residual bar, and
        # only that one: this is the family on which the last Jacobi sweep shows
        d0, r0, o0, s0 = ref.jacobi_errors(a, np.diag(a).copy(), np.eye(n), False)
        assert r0 >= 10 * 1e-11 * s0 and d0 <= 1e-12 * s0 and o0 == 0.0, (d0, r0)
    if family.startswith("gauss_1e"):
        big = np.abs(a).max()
        assert big > 1e149 or big < 1e-149


NEW_SYMBOLS = {"scs_debug_apply_ex": 8, "scs_debug_gram_ex": 13, "scs_debug_update": 14}


def test_the_header_declares_the_hooks_and_the_binding_holds_them():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    for name, n_args in NEW_SYMBOLS.items():
        decl = re.search(rf"int {name}\(([^;]*)\);", header)
        assert decl is not None, name
        params = [p.strip() for p in decl.group(1).split(",")]
        restype, argtypes = _native.SIGNATURES[name]
        assert len(params) == len(argtypes) == n_args and restype is _native.C.c_int, name
        for p, t in zip(params, argtypes):  # pointers travel as addresses, scalars by their C type
            want = _native.C.c_void_p if "*" in p else (_native.C.c_double if p.startswith("double") else _native.C.c_int32)
            assert t is want, (name, p)
    # the earlier entry points keep their signatures
    assert len(_native.SIGNATURES["scs_debug_apply"][1]) == 5 and len(_native.SIGNATURES["scs_debug_gram"][1]) == 8
    assert re.search(r"int scs_debug_apply\(scs_ctx \*ctx, scs_graph \*graph, const double \*x, int32_t b, double \*y\);",
                     header)
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header
