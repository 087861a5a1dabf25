"""The small solves and the tall panel kernels of the LOBPCG loop, one launch at a time (needs an MI355X): the SVQB,
the Rayleigh-Ritz solve on all three of its paths, the projected SVQB on both of its layouts, ``k_panel_rr``,
``k_panel_tf``, ``k_gram_qaq``, ``k_rr_update`` and ``k_residual``, through the ``scs_debug_small_*`` and
``scs_debug_panel`` hooks.  Solves are held to identities evaluated in longdouble on their own outputs and to the
float64 host model on the same input, products to budgets derived from the arithmetic
(``small_solve_chain_reference``); wherever two paths claim the same bits, the bits are compared.

``SCS_CHAIN_RATIOS=<file>`` writes the worst error / bound ratio per family at the end of the run (informational)."""

import os

import numpy as np
import pytest
import small_solve_chain_reference as ref

from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

RATIOS: dict = {}
LD, U, TOL = ref.LD, ref.U, ref.DROP_TOL


def _note(family: str, ratio: float, case: str) -> None:
    if family not in RATIOS or ratio > RATIOS[family][0]:
        RATIOS[family] = (ratio, case)


def _hold(family: str, err: float, bound: float, case: str) -> None:
    ratio = 0.0 if err == 0.0 else (float("inf") if not bound > 0.0 or not np.isfinite(err) else err / bound)
    _note(family, ratio, case)
    assert ratio <= 1.0, f"{case}: {family} {err:.3e} against {bound:.3e} (ratio {ratio:.3e})"


def _within(family: str, got, want, budget, case: str) -> None:
    ratio, at = ref.worst(np.asarray(got), want, budget)
    _note(family, ratio, case)
    assert ratio <= 1.0, f"{case}: {family} error / budget {ratio:.3e} at {at} (got {np.asarray(got)[at]!r})"


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()
    out = os.environ.get("SCS_CHAIN_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("# worst measured error / bound per family, and the case it came from\n")
            for family in sorted(RATIOS):
                f.write(f"{family}\t{RATIOS[family][0]:.3e}\t{RATIOS[family][1]}\n")


def _same(a, b) -> bool:
    """Bit for bit, NaN patterns included."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# SVQB
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,k", [(f, k) for k in ref.SVQB_SIZES for f in ref.SVQB_FAMILIES
                                      if ref.svqb_applicable(f, k)])
def test_svqb(dev, family, k):
    y, g, rank = ref.svqb_case(family, k)
    case = f"svqb {family} k={k}"
    t, mask = dev.debug_small_svqb(g, TOL)
    assert np.isfinite(t).all(), case
    assert mask.tolist() == [1] * rank + [0] * (k - rank), f"{case}: mask {mask.tolist()}"
    assert not t[:, mask == 0].any(), f"{case}: a dropped column of T is not zero"
    tm, mm, _ = ref.svqb_model(g, TOL)
    _hold("svqb_pass1", ref.svqb_identity(g, t, mask), ref.model_bound(ref.svqb_identity(g, tm, mm), k), case)
    if family == "asymmetric":
        ts, ms = dev.debug_small_svqb(np.ascontiguousarray(0.5 * (g + g.T)), TOL)
        assert _same(t, ts) and _same(mask, ms), f"{case}: the symmetrised input gives other bits"
    elif y is not None:
        t2, mask2 = dev.debug_small_svqb(ref.svqb_second_gram(y, t), 0.0)
        assert np.array_equal(mask2, mask), f"{case}: pass 2 mask {mask2.tolist()}"
        assert not t2[:, mask == 0].any(), case
        _hold("svqb_pass2", ref.svqb_two_pass_error(y, t, t2, mask), 64 * k * U, case)


# ---------------------------------------------------------------------------------------------------------------
# Rayleigh-Ritz
# ---------------------------------------------------------------------------------------------------------------
def _rr_hold(t, nq, b, mask, out, case, family, exact_from=-1):
    """Every identity of one Rayleigh-Ritz result, D's orthogonality against the host model's on the same matrix."""
    c, d, theta, mask_p = out
    assert np.isfinite(c).all() and np.isfinite(theta[:min(b + 1, nq)]).all(), case
    if nq == b:  # no directions: d and mask_p are not touched
        assert np.isnan(d).all() and (mask_p == -1).all() and np.isnan(theta[b]), f"{case}: d, mask_p, theta[b] touched"
        d = mask_p = None
    else:
        assert np.isfinite(d).all() and set(mask_p.tolist()) <= {0, 1}, case
    ident = ref.rr_identities(t, b, mask, c, d, theta, mask_p, exact_from)
    mc, md, mth, mmp, _ = ref.rr_model(t, b, mask, TOL, exact_from)
    model = ref.rr_identities(t, b, mask, mc, md, mth, mmp, exact_from)
    bars = ref.rr_bars(nq, model.get("d_orth", 0.0))
    assert ident["descending"], f"{case}: theta not descending"
    for key, bar in bars.items():
        if key in ident:
            _hold(f"rr_{family}_{key}", ident[key], bar, case)
    return ident


def _rr_cases():
    for nq, b in ref.RR_SHAPES:
        for family in ref.RR_FAMILIES:
            for kind in (ref.RR_MASKS if nq == 3 * b else ("live",)):
                yield nq, b, family, kind


@pytest.mark.parametrize("nq,b,family,kind", list(_rr_cases()))
def test_rayleigh_ritz(dev, nq, b, family, kind):
    mask = ref.rr_mask(kind, nq, b)
    t = ref.rr_matrix(family, nq, b, mask=mask)
    case = f"rr ({nq},{b}) {family} {kind}"
    c, d, theta, mask_p, mask48 = dev.debug_small_rr(t, nq, b, mask, TOL)
    assert mask48[:nq].tolist() == mask.tolist() and (mask48[nq:] == -1).all(), f"{case}: the basis mask was written"
    _rr_hold(t, nq, b, mask, (c, d, theta, mask_p), case, "wave" if (nq, b) in ref.RR_WAVE_SHAPES else "general")
    if nq == 3 * b:
        assert mask_p.all(), f"{case}: a direction was dropped, mask_p {mask_p.tolist()}"
        if family == "generic":  # (conditioning of the span asserted on the host model, CPU test)
            _hold("rr_span", ref.projector_difference(d, ref.rr_direction_block(c, b)), 1e-10, case)


@pytest.mark.parametrize("nq,b", [s for s in ref.RR_SHAPES if s[0] == 3 * s[1]])
def test_rayleigh_ritz_drops_exactly_the_vanishing_direction(dev, nq, b):
    slot = 2 * b + 1
    t, mask = ref.rr_vanishing(nq, b, slot), np.ones(nq, dtype=np.int32)
    unit = np.zeros(nq)
    unit[slot] = 1.0
    for start in ((0, 2) if (nq, b) in ref.RR_WAVE_SHAPES else (0,)):
        case = f"rr vanishing ({nq},{b}) start={start}"
        c, d, theta, mask_p, _ = dev.debug_small_rr(t, nq, b, mask, TOL, start=start)
        # a pair with a zero entry is never rotated: the decoupled slot is the top Ritz vector, exactly
        assert theta[0] == 2.0 and np.array_equal(np.abs(c[:, 0]), unit), case
        assert not c[slot, 1:].any(), case
        wave = start == 0 and (nq, b) in ref.RR_WAVE_SHAPES
        # (the one-wave path drops the column itself, the SVQB of the general path the last eigen-direction)
        want = [0] + [1] * (b - 1) if wave else [1] * (b - 1) + [0]
        assert mask_p.tolist() == want, f"{case}: mask_p {mask_p.tolist()}"
        _rr_hold(t, nq, b, mask, (c, d, theta, mask_p), case, "vanishing")


@pytest.mark.parametrize("nq,b", [s for s in ref.RR_SHAPES if s[0] == 3 * s[1]])
def test_rayleigh_ritz_keeps_a_nearly_vanishing_direction(dev, nq, b):
    # 1e-6 of the top direction is left after the projection: the case the SECOND (I - C C^T) pass is there for
    t, mask = ref.rr_nearly_vanishing(nq, b, 2 * b + 1), np.ones(nq, dtype=np.int32)
    for start in ((0, 2) if (nq, b) in ref.RR_WAVE_SHAPES else (0,)):
        case = f"rr nearly vanishing ({nq},{b}) start={start}"
        c, d, theta, mask_p, _ = dev.debug_small_rr(t, nq, b, mask, TOL, start=start)
        assert mask_p.all(), f"{case}: mask_p {mask_p.tolist()}"
        _rr_hold(t, nq, b, mask, (c, d, theta, mask_p), case, "nearly_vanishing")


@pytest.mark.parametrize("b", [4, 8, 12, 16])
def test_rayleigh_ritz_start(dev, b):
    t = ref.rr_matrix("generic", b, b)
    c0, d0, th0, mp0, _ = dev.debug_small_rr(t, b, b, np.ones(b, dtype=np.int32), TOL)
    c, d, theta, mask_p, mask48 = dev.debug_small_rr(t, b, b, None, TOL, start=1)
    assert mask48.tolist() == [1] * b + [0] * b + [1] * (48 - 2 * b), mask48.tolist()
    assert _same(c, c0) and _same(theta, th0), "k_small_rr_start solves another matrix than k_small_rr at nq = b"
    assert np.isnan(d).all() and np.isnan(theta[b])
    _rr_hold(t, b, b, np.ones(b, dtype=np.int32), (c, d, theta, np.full(b, -1, dtype=np.int32)), f"rr start b={b}",
             "start")


@pytest.mark.parametrize("nparts", ref.RR_NPARTS)
@pytest.mark.parametrize("nq,b", ref.RR_WAVE_SHAPES)
def test_rayleigh_ritz_sums_its_partials(dev, nq, b, nparts):
    mask = ref.rr_mask("dead_p", nq, b)
    t = ref.rr_matrix("generic", nq, b)
    case = f"rr partials ({nq},{b}) nparts={nparts}"
    tq, parts = ref.dyadic_split(t, nparts, seed=nq + nparts)
    one = dev.debug_small_rr(np.ascontiguousarray(tq), nq, b, mask, TOL)
    summed = dev.debug_small_rr(parts, nq, b, mask, TOL)
    for name, a, bb in zip(("c", "d", "theta", "mask_p"), one, summed):
        assert _same(a, bb), f"{case}: {name} differs from the solve of the summed matrix"
    # partials off any grid: the matrix the kernel solves is their sum in its own fixed order
    plain = ref.plain_split(t, nparts, seed=nq + nparts)
    tsum = ref.sum_partials_model(plain.reshape(nparts, -1)).reshape(nq, nq)
    out = dev.debug_small_rr(plain, nq, b, mask, TOL)
    _rr_hold(tsum, nq, b, mask, out[:4], case, "partials")


@pytest.mark.parametrize("nparts", [1, 9])
@pytest.mark.parametrize("nq,b", ref.RR_WAVE_SHAPES)
def test_rayleigh_ritz_exact_from(dev, nq, b, nparts):
    rs = np.random.RandomState(nq)
    skew = np.triu(rs.choice([-1.0, 1.0], size=(nq, nq)) * rs.uniform(1e-6, 2e-6, (nq, nq)), 1)
    tq, parts = ref.dyadic_split(ref.rr_matrix("generic", nq, b) + skew - skew.T, nparts, seed=3 * nq + nparts)
    assert np.all(np.abs(tq - tq.T)[np.triu_indices(nq, 1)] >= 1e-6)  # every pair carries the planted asymmetry
    mask = np.ones(nq, dtype=np.int32)
    case = f"rr exact_from ({nq},{b}) nparts={nparts}"
    got = dev.debug_small_rr(parts, nq, b, mask, TOL, exact_from=b)
    assembled = np.ascontiguousarray(ref.rr_assemble(tq, mask, exact_from=b))
    want = dev.debug_small_rr(assembled, nq, b, mask, TOL)
    for name, a, bb in zip(("c", "d", "theta", "mask_p"), got, want):
        assert _same(a, bb), f"{case}: {name} differs from the solve of the matrix assembled with the documented choice"
    plain = dev.debug_small_rr(parts, nq, b, mask, TOL)
    assert not _same(got[0], plain[0]) and not _same(got[2], plain[2]), f"{case}: exact_from changed nothing"
    _rr_hold(tq, nq, b, mask, got[:4], case, "exact_from", exact_from=b)


@pytest.mark.parametrize("kind", ref.RR_MASKS)
@pytest.mark.parametrize("nq,b", ref.RR_WAVE_SHAPES)
def test_wave_path_against_general_path(dev, nq, b, kind):
    mask = ref.rr_mask(kind, nq, b)
    t = ref.rr_matrix("generic", nq, b, mask=mask)
    case = f"rr wave/general ({nq},{b}) {kind}"
    wave = dev.debug_small_rr(t, nq, b, mask, TOL)
    general = dev.debug_small_rr(t, nq, b, mask, TOL, start=2)
    assert _same(wave[0], general[0]) and _same(wave[2], general[2]), f"{case}: C or theta differ before the branch"
    _rr_hold(t, nq, b, mask, general[:4], case, "general_at_wave_sizes")
    assert wave[3].all() and general[3].all(), case
    # Gram-Schmidt in Ritz order against SVQB: other vectors, one span
    _hold("rr_span_wave_general", ref.projector_difference(wave[1], general[1]), 1e-10, case)


def test_the_small_hooks_refuse_what_the_kernels_cannot_take(dev):
    t = np.zeros((36, 36))
    with pytest.raises(RuntimeError, match="nq <= 24"):
        dev.debug_small_rr(np.zeros((2, 36, 36)), 36, 12, np.ones(36, dtype=np.int32), TOL)
    with pytest.raises(RuntimeError, match="b <= nq <= 3b"):
        dev.debug_small_rr(t, 36, 8, np.ones(36, dtype=np.int32), TOL)
    for b in (12, 16):  # the projected SVQB's working set holds cxp[16][8]: the fused loop's widths only
        with pytest.raises(RuntimeError, match="block widths up to 8"):
            dev.debug_small_orth(np.zeros((1, 3 * b * b + b)), b, TOL, np.zeros(b + 1))
    with pytest.raises(RuntimeError, match="compact layout"):
        dev.debug_small_orth(np.zeros((1, 3 * 36 + 6)), 6, TOL, np.zeros(7), layout=1)
    with pytest.raises(RuntimeError, match="does not take block width"):
        dev.debug_panel(0, 12, 4, np.zeros((20, 36)), np.zeros((20, 36)), coef_a=np.zeros((36, 12)),
                        coef_b=np.zeros((36, 12)), theta=np.zeros(12))


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
def test_projected_svqb(dev, b, with_u, planted, rank):
    u, x, p, r = ref.orth_case(b, planted, rank, with_u)
    g = ref.orth_gram(u, x, p, r)
    theta = np.linspace(1.0, 0.5, b + 1)
    nkeep = ref.orth_rank(rank, b)
    k = 3 * b + 1
    for nparts in ref.ORTH_NPARTS:
        case = f"orth b={b} u={int(with_u)} planted={planted} {rank} nparts={nparts}"
        parts = ref.plain_split(g, nparts, seed=b + nparts)
        gsum = ref.sum_partials_model(parts)
        coef, mask, report = dev.debug_small_orth(parts, b, TOL, theta, layout=0)
        assert np.isfinite(coef).all(), case
        assert mask.tolist() == [1] * nkeep + [0] * (b - nkeep), f"{case}: mask {mask.tolist()}"
        assert not coef[3 * b + 1:].any(), f"{case}: a pad row of the coefficients is not zero"
        assert not coef[:, mask == 0].any(), f"{case}: a dropped column is not zero"
        if not with_u:
            assert not coef[3 * b].any(), case
        # the report: diag G as the kernel summed it, theta, the sequence number; nothing else
        gd = np.diag(gsum[2 * b * b:3 * b * b].reshape(b, b))
        assert _same(report[:b], gd), f"{case}: report[0:b] {report[:b]} against diag G {gd}"
        assert _same(report[16:16 + b + 1], theta) and report[40] == 7.0, case
        assert np.isnan(report[b:16]).all() and np.isnan(report[16 + b + 1:40]).all(), case
        mcoef, mmask, _, _ = ref.orth_model(gsum, b, TOL)
        mo, mc = ref.orth_errors(u, x, p, r, mcoef, mmask)
        orth, cross = ref.orth_errors(u, x, p, r, coef, mask)
        _hold("orth_rtr", orth, ref.model_bound(mo, k), case)
        _hold("orth_cross", cross, ref.model_bound(mc, k), case)
        coef1, mask1, report1 = dev.debug_small_orth(parts, b, TOL, theta, layout=1)
        assert _same(coef1, coef) and _same(mask1, mask) and _same(report1, report), \
            f"{case}: the compact layout gives other bits"


# ---------------------------------------------------------------------------------------------------------------
# tall kernels
# ---------------------------------------------------------------------------------------------------------------
def _rows_past_n(case, n, before, after):
    assert _same(after[n:], before[n:]), f"{case}: a row past n was written"


def _coefficients(n: int, b: int):
    rs = np.random.RandomState(17 * n + b)
    return rs.standard_normal((3 * b, b)), rs.standard_normal((3 * b, b)), np.sort(rs.uniform(-1, 1, b))[::-1].copy()


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("n", ref.TALL_ROWS)
def test_panel_rr(dev, n, b):
    q, aq, u, _ = ref.tall_panels(n, b, 0)
    c, d, theta = _coefficients(n, b)
    want = ref.panel_rr_reference(q, aq, c, d, theta, n, b)
    first = None
    for blocks in ref.TALL_BLOCKS:
        for uu in (u, None):
            case = f"panel_rr n={n} b={b} blocks={blocks} u={int(uu is not None)}"
            q2, aq2, part = dev.debug_panel(0, b, n, q, aq, u=uu, coef_a=c, coef_b=d, theta=theta, blocks=blocks)
            _within("panel_rr_xp", q2[:n, :2 * b], *want["q_xp"], case)
            _within("panel_rr_sxp", aq2[:n, :2 * b], *want["aq_xp"], case)
            _within("panel_rr_r", q2[:n, 2 * b:], *want["r"], case)
            assert _same(aq2[:n, 2 * b:], aq[:n, 2 * b:]), f"{case}: the R slot of SQ moved"
            _rows_past_n(case, n, q, q2)
            _rows_past_n(case, n, aq, aq2)
            # the rows do not depend on the grid or on u
            if first is None:
                first = (q2, aq2)
            assert _same(q2, first[0]) and _same(aq2, first[1]), f"{case}: the panels depend on the grid"
            assert np.isfinite(part).all(), f"{case}: a workgroup wrote no partial"
            pref, pbud = ref.panel_partials_reference(q2[:n], None if uu is None else uu[:n], n, b)
            _within("panel_rr_gram", part.astype(LD).sum(axis=0), pref, pbud, case)
            if uu is None:
                assert not part[:, 3 * b * b:].any(), f"{case}: u^T r without u"


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("n", ref.TALL_ROWS)
def test_panel_tf(dev, n, b):
    q, _, u, dinv = ref.tall_panels(n, b, 1)
    aq = np.full_like(q, ref.SENTINEL)  # not an operand
    rs = np.random.RandomState(23 * n + b)
    coef = np.zeros((3 * b + 4, b))
    coef[:3 * b + 1] = rs.standard_normal((3 * b + 1, b))
    for uu in (u, None):
        rt, mag = ref.panel_tf_reference(q, uu, coef, n, b)
        for blocks in ref.TALL_BLOCKS:
            case = f"panel_tf n={n} b={b} blocks={blocks} u={int(uu is not None)}"
            # with the Gram products
            q2, aq2, part = dev.debug_panel(1, b, n, q, aq, u=uu, coef_a=coef, blocks=blocks)
            _within("panel_tf_r", q2[:n, 2 * b:], rt, ref.budget(3 * b + 4, mag), case)
            assert _same(q2[:n, :2 * b], q[:n, :2 * b]) and _same(aq2, aq), f"{case}: a column beside R moved"
            _rows_past_n(case, n, q, q2)
            assert np.isfinite(part).all(), f"{case}: a workgroup wrote no partial"
            pref, pbud = ref.panel_partials_reference(q2[:n], None if uu is None else uu[:n], n, b)
            _within("panel_tf_gram", part.astype(LD).sum(axis=0), pref, pbud, case)
            # with Z = dinv (.) R', k-major, instead
            zt = np.full((b, n + ref.PAD), ref.SENTINEL)
            q3, aq3, _ = dev.debug_panel(2, b, n, q, aq, u=uu, coef_a=coef, dinv=dinv, blocks=blocks, zt=zt)
            assert _same(q3, q2) and _same(aq3, aq), f"{case}: the Z variant transforms other bits"
            dl = dinv[:n].astype(LD)[None, :]
            _within("panel_tf_z", zt[:, :n], dl * rt.T, ref.budget(3 * b + 5, dl * mag.T), case)
            assert (zt[:, n:] == ref.SENTINEL).all(), f"{case}: Z written past n"


@pytest.mark.parametrize("b", [4, 8])
@pytest.mark.parametrize("n", ref.TALL_ROWS)
def test_gram_qaq(dev, n, b):
    q, aq, _, dinv = ref.tall_panels(n, b, 2)
    rs = np.random.RandomState(29 * n + b)
    for nseg in (1, 2, 4):
        ypart = np.full((nseg * n + ref.PAD) * b, ref.SENTINEL)
        ypart[:nseg * n * b] = rs.standard_normal(nseg * n * b)
        aq_in = aq.copy()
        aq_in[:n, 2 * b:] = ref.SENTINEL  # FINISH 1 makes the R slot, it does not read it
        segs = ypart[:nseg * n * b].reshape(nseg, n, b).astype(LD)
        dl = dinv[:n].astype(LD)[:, None]
        ar, ar_bud = dl * segs.sum(axis=0), ref.budget(nseg, dl * np.abs(segs).sum(axis=0))
        for blocks in ref.TALL_BLOCKS:
            case = f"gram_qaq n={n} b={b} nseg={nseg} blocks={blocks}"
            q2, aq2, part = dev.debug_panel(4, b, n, q, aq_in, dinv=dinv, ypart=ypart, nseg=nseg, blocks=blocks)
            _within("gram_qaq_sr", aq2[:n, 2 * b:], ar, ar_bud, case)
            assert _same(q2, q) and _same(aq2[:n, :2 * b], aq[:n, :2 * b]), f"{case}: an operand moved"
            _rows_past_n(case, n, aq_in, aq2)
            assert np.isfinite(part).all(), f"{case}: a workgroup wrote no partial"
            tref, tbud = ref.gram_budget(q, aq2, n)
            _within("gram_qaq_t", part.astype(LD).sum(axis=0).reshape(3 * b, 3 * b), tref, tbud, case)
            # the finished panel through FINISH 0: the same products in the same order
            q3, aq3, part0 = dev.debug_panel(3, b, n, q, aq2, blocks=blocks)
            assert _same(part0, part), f"{case}: FINISH 0 on the finished panel gives other partials"
            assert _same(q3, q) and _same(aq3, aq2), f"{case}: FINISH 0 wrote a panel"


@pytest.mark.parametrize("b", ref.LEGACY_WIDTHS)
@pytest.mark.parametrize("n", ref.TALL_ROWS)
def test_legacy_update_and_residual(dev, n, b):
    q, aq, _, _ = ref.tall_panels(n, b, 3)
    c, d, theta = _coefficients(n, b)
    case = f"rr_update n={n} b={b}"
    sent = np.full_like(aq, ref.SENTINEL)
    q2, aq2, _ = dev.debug_panel(5, b, n, q, sent, coef_a=c, coef_b=d)
    xq, mq = ref.product_ld(q[:n], np.concatenate([c, d], axis=1))
    _within("rr_update", q2[:n, :2 * b], xq, ref.budget(3 * b, mq), case)
    assert _same(q2[:n, 2 * b:], q[:n, 2 * b:]) and _same(aq2, sent), f"{case}: a column beside X, P moved"
    _rows_past_n(case, n, q, q2)
    # k_residual reads the X blocks only: every other column holds a sentinel
    case = f"residual n={n} b={b}"
    qs, aqs = np.full_like(q, ref.SENTINEL), np.full_like(aq, ref.SENTINEL)
    qs[:n, :b], aqs[:n, :b] = q[:n, :b], aq[:n, :b]
    q3, aq3, part = dev.debug_panel(6, b, n, qs, aqs, theta=theta)
    th = theta.astype(LD)[None, :]
    xl, al = qs[:n, :b].astype(LD), aqs[:n, :b].astype(LD)
    _within("residual_r", q3[:n, 2 * b:], al - xl * th, ref.budget(2, np.abs(al) + np.abs(xl) * np.abs(th)), case)
    assert _same(q3[:, :2 * b], qs[:, :2 * b]) and _same(aq3, aqs), f"{case}: a column beside R moved"
    _rows_past_n(case, n, qs, q3)
    assert part.shape == ((n + 255) // 256, b)
    for w in range(part.shape[0]):  # the partial norms, workgroup by workgroup, of the rows the launch stored
        v = q3[256 * w:min(n, 256 * w + 256), 2 * b:].astype(LD)
        _within("residual_norms", part[w], (v * v).sum(axis=0), ref.budget(256, (v * v).sum(axis=0)), f"{case} wg={w}")
