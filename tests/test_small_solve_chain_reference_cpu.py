"""``small_solve_chain_reference`` without a device: the float64 host models meet every identity on every case, each
planted-defect model misses at least one, no keep / drop decision of any case sits near its threshold, plain fp64
numpy sits inside the tall kernels' budgets, and the header and ``_native.SIGNATURES`` agree on the four hooks."""

import re
from pathlib import Path

import numpy as np
import pytest
import small_solve_chain_reference as ref
import solver_reference as sref

from spectralclustersupertree_amd import _native

U = ref.U


def test_extended_precision_is_available():
    ref.require_extended_precision()


# ---------------------------------------------------------------------------------------------------------------
# SVQB
# ---------------------------------------------------------------------------------------------------------------
SVQB_CASES = [(f, k) for k in ref.SVQB_SIZES for f in ref.SVQB_FAMILIES if ref.svqb_applicable(f, k)]


@pytest.mark.parametrize("family,k", SVQB_CASES)
def test_svqb_model_meets_the_identities(family, k):
    y, g, rank = ref.svqb_case(family, k)
    t, mask, w = ref.svqb_model(g, ref.DROP_TOL)
    assert ref.threshold_distance_ok(w, ref.DROP_TOL), (family, k, w / max(w[0], 1e-300))
    assert mask.tolist() == [1] * rank + [0] * (k - rank)
    assert not t[:, mask == 0].any()
    err = ref.svqb_identity(g, t, mask)
    # the yardstick itself stays small, so 8 x it is still a tight bar.  near_1e-5 cannot stay below 1e-6: its
    # smallest scaled eigenvalue is eps^2 / 2 = 5e-11, and an eigenvalue known to k u is known to k u / 5e-11 = 2e-6 k
    assert err < (1e-4 if family == "near_1e-5" else 1e-6), (family, k, err)
    if family == "asymmetric":
        gs = 0.5 * (g + g.T)
        assert not np.array_equal(g, gs)
        t2, mask2, _ = ref.svqb_model(gs, ref.DROP_TOL)
        assert np.array_equal(t, t2) and np.array_equal(mask, mask2)
    elif y is not None:
        g2 = ref.svqb_second_gram(y, t)
        t2, mask2, _ = ref.svqb_model(g2, 0.0)
        assert np.array_equal(mask2, mask)
        assert ref.svqb_two_pass_error(y, t, t2, mask) <= 64 * k * U, (family, k)


def test_svqb_identity_notices_a_wrong_transform():
    _, g, _ = ref.svqb_case("duplicate", 8)
    t, mask, _ = ref.svqb_model(g, ref.DROP_TOL)
    base = ref.svqb_identity(g, t, mask)
    bad = t.copy()
    bad[3, 2] *= 1.0 + 1e-9  # one entry off in the ninth digit
    assert ref.svqb_identity(g, bad, mask) > ref.model_bound(base, 8)
    # a transform built from the lower triangle alone
    _, ga, _ = ref.svqb_case("asymmetric", 8)
    tl, ml, _ = ref.svqb_model(np.tril(ga) + np.tril(ga, -1).T, ref.DROP_TOL)
    ta, ma, _ = ref.svqb_model(ga, ref.DROP_TOL)
    assert ref.svqb_identity(ga, tl, ml) > ref.model_bound(ref.svqb_identity(ga, ta, ma), 8)


# ---------------------------------------------------------------------------------------------------------------
# Rayleigh-Ritz
# ---------------------------------------------------------------------------------------------------------------
def _rr_cases():
    for nq, b in ref.RR_SHAPES:
        for family in ref.RR_FAMILIES:
            for kind in (ref.RR_MASKS if nq == 3 * b else ("live",)):
                yield nq, b, family, kind


@pytest.mark.parametrize("nq,b,family,kind", list(_rr_cases()))
def test_rr_model_meets_the_identities(nq, b, family, kind):
    mask = ref.rr_mask(kind, nq, b)
    t = ref.rr_matrix(family, nq, b, mask=mask)
    assert np.abs(t).max() <= 1.5
    c, d, theta, mask_p, lw = ref.rr_model(t, b, mask, ref.DROP_TOL)
    ident = ref.rr_identities(t, b, mask, c, d, theta, mask_p)
    assert ref.rr_failures(ident, nq) == [], ident
    if d is not None:
        assert ref.threshold_distance_ok(lw, ref.DROP_TOL), lw
        assert mask_p.all()  # every direction of these cases is kept
    if family == "converged":
        assert np.abs(t[:b, :b] - np.diag(np.diag(t[:b, :b]))).max() < 1e-11
    if family == "repeated" and nq > b:
        assert abs(theta[b - 1] - theta[b]) < 1e-14


@pytest.mark.parametrize("nq,b", [s for s in ref.RR_SHAPES if s[0] == 3 * s[1]])
def test_rr_span_cases_are_well_conditioned(nq, b):
    # the span assertion is made on the generic family only: what is left of its directions after the projection
    for kind in ref.RR_MASKS:
        t, mask = ref.rr_matrix("generic", nq, b), ref.rr_mask(kind, nq, b)
        c, d, _, mask_p, _ = ref.rr_model(t, b, mask, ref.DROP_TOL)
        assert ref.direction_conditioning(c, b) >= 1e-3, (nq, b, kind)
        assert ref.projector_difference(d, ref.rr_direction_block(c, b)) <= 1e-10


@pytest.mark.parametrize("nq,b", [s for s in ref.RR_SHAPES if s[0] == 3 * s[1]])
def test_rr_vanishing_direction_is_dropped(nq, b):
    slot = 2 * b + 1
    t, mask = ref.rr_vanishing(nq, b, slot), np.ones(nq, dtype=np.int32)
    c, d, theta, mask_p, lw = ref.rr_model(t, b, mask, ref.DROP_TOL)
    assert theta[0] == 2.0 and mask_p.tolist() == [1] * (b - 1) + [0]
    assert ref.threshold_distance_ok(lw, ref.DROP_TOL)
    assert ref.rr_failures(ref.rr_identities(t, b, mask, c, d, theta, mask_p), nq) == []


@pytest.mark.parametrize("nq,b", [s for s in ref.RR_SHAPES if s[0] == 3 * s[1]])
def test_rr_nearly_vanishing_direction_is_kept(nq, b):
    t, mask = ref.rr_nearly_vanishing(nq, b, 2 * b + 1), np.ones(nq, dtype=np.int32)
    c, d, theta, mask_p, lw = ref.rr_model(t, b, mask, ref.DROP_TOL)
    assert 1e-7 < np.linalg.norm(c[:b, 0]) < 1e-5  # what the top Ritz vector keeps in the X block
    assert mask_p.all() and ref.threshold_distance_ok(lw, ref.DROP_TOL)
    ident = ref.rr_identities(t, b, mask, c, d, theta, mask_p)
    assert ref.rr_failures(ident, nq) == [] and ident["d_orth"] < 1e-6, ident
    # one projection only: C^T D misses its bar, and nothing else does
    c, d, theta, mask_p, _ = ref.rr_model(t, b, mask, ref.DROP_TOL, defect="one_projection")
    assert ref.rr_failures(ref.rr_identities(t, b, mask, c, d, theta, mask_p), nq) == ["cd"]


@pytest.mark.parametrize("defect", ["mask_late", "dropped_direction", "dead_row_leak"])
def test_rr_identities_notice_the_planted_defects(defect):
    nq, b = 24, 8
    if defect == "mask_late":
        t, mask = ref.rr_vanishing(nq, b, 2 * b + 1), np.ones(nq, dtype=np.int32)
    else:
        t, mask = ref.rr_matrix("generic", nq, b), ref.rr_mask("dead_both", nq, b)
    c, d, theta, mask_p, _ = ref.rr_model(t, b, mask, ref.DROP_TOL, defect=defect)
    assert ref.rr_failures(ref.rr_identities(t, b, mask, c, d, theta, mask_p), nq) != []


def test_exact_from_takes_the_entry_with_the_exact_product():
    nq, b = 12, 4
    rs = np.random.RandomState(5)
    t = ref.rr_matrix("generic", nq, b) + 1e-6 * np.triu(rs.standard_normal((nq, nq)), 1)
    mask = np.ones(nq, dtype=np.int32)
    a = ref.rr_assemble(t, mask, exact_from=b)
    assert np.array_equal(a, a.T)
    for i in range(nq):
        for j in range(i + 1, nq):
            want = t[j, i] if i < b else 0.5 * (t[i, j] + t[j, i])  # Q_j^T (S Q_i): row j, column i
            assert a[i, j] == want
    assert not np.array_equal(a, ref.rr_assemble(t, mask))
    # the other triangle is a different matrix, and a solve of it misses the residual bar against this one
    other = ref.rr_assemble(t.T.copy(), mask, exact_from=b)
    c, d, theta, mask_p, _ = ref.rr_model(t.T.copy(), b, mask, ref.DROP_TOL, exact_from=b)
    assert not np.array_equal(a, other)
    assert "c_res" in ref.rr_failures(ref.rr_identities(t, b, mask, c, d, theta, mask_p, exact_from=b), nq)


@pytest.mark.parametrize("nparts", ref.RR_NPARTS)
def test_dyadic_split_sums_back_exactly_in_any_order(nparts):
    t = ref.rr_matrix("generic", 24, 8)
    tq, parts = ref.dyadic_split(t, nparts, seed=nparts)
    assert np.abs(tq - t).max() <= 2.0 ** -31
    flat = parts.reshape(nparts, -1)
    assert np.array_equal(ref.sum_partials_model(flat), tq.ravel())
    assert np.array_equal(flat[::-1].sum(axis=0), tq.ravel())
    if nparts > 128:  # a sum that drops partial 128 is another matrix
        assert not np.array_equal(np.delete(flat, 128, axis=0).sum(axis=0), tq.ravel())
    plain = ref.plain_split(t, nparts, seed=nparts).reshape(nparts, -1)
    assert np.abs(ref.sum_partials_model(plain) - t.ravel()).max() <= (nparts + 2) * U * np.abs(plain).sum(axis=0).max()


# ---------------------------------------------------------------------------------------------------------------
# projected SVQB
# ---------------------------------------------------------------------------------------------------------------
def _orth_cases():
    for b in ref.ORTH_WIDTHS:
        for with_u in (True, False):
            for planted in ref.ORTH_PLANTED:
                yield b, with_u, planted, "full"
            for rank in ref.ORTH_RANKS[1:]:
                yield b, with_u, 1e-3, rank


@pytest.mark.parametrize("b,with_u,planted,rank", list(_orth_cases()))
def test_orth_model_meets_the_identities(b, with_u, planted, rank):
    u, x, p, r = ref.orth_case(b, planted, rank, with_u)
    basis = np.concatenate(([u[:, None]] if with_u else []) + [x, p], axis=1)
    assert ref.maxabs(ref.gram_ld(basis, basis) - np.eye(basis.shape[1])) < 1e-14
    g = ref.orth_gram(u, x, p, r)
    if not with_u:
        assert not g[3 * b * b:].any()
    coef, mask, w, ratio = ref.orth_model(g, b, ref.DROP_TOL)
    assert mask.tolist() == [1] * ref.orth_rank(rank, b) + [0] * (b - ref.orth_rank(rank, b))
    assert ref.threshold_distance_ok(w, ref.DROP_TOL), w
    # the cancellation guard: dgn / gm is well above 1e-13, or exactly 0 (a zero column), or the planted 1e-14 within
    # its rounding (orth_case): no rounding moves it across
    noise = (2 * b + 3) * U
    planted_low = (ratio >= 1e-14 - noise) & (ratio <= 1e-14 + noise)
    assert np.all((ratio >= 100 * 1e-13) | (ratio == 0.0) | planted_low), ratio
    assert np.sum(planted_low) == (2 if rank == "inside" else 0)
    orth, cross = ref.orth_errors(u, x, p, r, coef, mask)
    assert orth < 1e-6 and cross < 1e-6, (orth, cross)
    assert not coef[3 * b + 1:].any()
    # the second pass, as the solver makes it, finishes the job
    k = 3 * b + 1
    cl = coef.astype(ref.LD)
    r1 = (x.astype(ref.LD) @ cl[:b] + p.astype(ref.LD) @ cl[b:2 * b] + r.astype(ref.LD) @ cl[2 * b:3 * b]
          + (np.outer(u.astype(ref.LD), cl[3 * b]) if with_u else 0)).astype(np.float64)
    coef2, mask2, _, _ = ref.orth_model(ref.orth_gram(u, x, p, r1), b, 0.0)
    assert np.array_equal(mask2, mask)
    orth2, cross2 = ref.orth_errors(u, x, p, r1, coef2, mask2)
    assert orth2 <= 64 * k * U and cross2 <= 64 * k * U, (orth2, cross2)


@pytest.mark.parametrize("defect", ["no_guard", "no_u", "pad"])
def test_orth_identities_notice_the_planted_defects(defect):
    b = 8
    u, x, p, r = ref.orth_case(b, 1e-3, "inside" if defect == "no_guard" else "full", True)
    g = ref.orth_gram(u, x, p, r)
    good, gmask, _, _ = ref.orth_model(g, b, ref.DROP_TOL)
    bad, bmask, _, _ = ref.orth_model(g, b, ref.DROP_TOL, defect=defect)
    go, gc = ref.orth_errors(u, x, p, r, good, gmask)
    bo, bc = ref.orth_errors(u, x, p, r, bad, bmask)
    noticed = (not np.array_equal(gmask, bmask) or bo > ref.model_bound(go, 3 * b + 1)
               or bc > ref.model_bound(gc, 3 * b + 1) or bad[3 * b + 1:].any())
    assert noticed, (defect, go, gc, bo, bc)


# ---------------------------------------------------------------------------------------------------------------
# tall kernels: plain fp64 numpy sits inside every budget, a dropped row does not
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 17, 257, 4111])
@pytest.mark.parametrize("b", [4, 8])
def test_numpy_sits_inside_the_tall_budgets(n, b):
    q, aq, u, dinv = ref.tall_panels(n, b, 0)
    rs = np.random.RandomState(n + b)
    c, d, theta = rs.standard_normal((3 * b, b)), rs.standard_normal((3 * b, b)), rs.uniform(-1, 1, b)
    want = ref.panel_rr_reference(q, aq, c, d, theta, n, b)
    cd = np.concatenate([c, d], axis=1)
    xq, xa = q[:n] @ cd, aq[:n] @ cd
    assert sref.worst(xq, *want["q_xp"])[0] <= 1.0 and sref.worst(xa, *want["aq_xp"])[0] <= 1.0
    res = xa[:, :b] - xq[:, :b] * theta[None, :]
    assert sref.worst(res, *want["r"])[0] <= 1.0
    coef = rs.standard_normal((3 * b + 4, b))
    rt, mag = ref.panel_tf_reference(q, u, coef, n, b)
    got = np.concatenate([q[:n], u[:n, None]], axis=1) @ coef[:3 * b + 1]
    assert sref.worst(got, rt, ref.budget(3 * b + 4, mag))[0] <= 1.0
    # u multiplied by a pad row of the coefficients (zero) instead of its own: far outside
    assert sref.worst(q[:n] @ coef[:3 * b], rt, ref.budget(3 * b + 4, mag))[0] > 100.0
    qn = q.copy()
    qn[:n, 2 * b:] = got
    pref, pbud = ref.panel_partials_reference(qn[:n], u[:n], n, b)
    g = np.concatenate([(qn[:n, :2 * b].T @ got).ravel(), (got.T @ got).ravel(), (u[:n] @ got).ravel()])
    assert sref.worst(g, pref, pbud)[0] <= 1.0
    if n > 1:  # the last row dropped from the Gram products: far outside
        g1 = np.concatenate([(qn[:n - 1, :2 * b].T @ got[:-1]).ravel(), (got[:-1].T @ got[:-1]).ravel(),
                             (u[:n - 1] @ got[:-1]).ravel()])
        assert sref.worst(g1, pref, pbud)[0] > 100.0


# ---------------------------------------------------------------------------------------------------------------
# the hooks
# ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = {"scs_debug_small_svqb": 6, "scs_debug_small_rr": 14, "scs_debug_small_orth": 10, "scs_debug_panel": 18}


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
    assert int(re.search(r"#define SCS_DEBUG_PANEL_PAD (\d+)", header).group(1)) == ref.PAD
    assert _native.ABI_VERSION == 109  # new symbols only


def test_the_jacobi_sizes_cover_every_dispatch():
    # jacobi_eig: 4, 8, 12 on jacobi_eig_waves, the rest up to 24 on jacobi_eig_fast (odd sizes pad), above generic
    assert {4, 5, 7, 8, 12, 16, 23, 24, 36}.issubset(sref.JACOBI_SIZES) and {2, 3, 48, 64}.issubset(sref.JACOBI_SIZES)
