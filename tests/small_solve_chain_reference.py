"""Host references for the small solves and the tall panel kernels of the LOBPCG loop (``csrc/scs_eig.hip``:
``k_small_svqb``, ``small_rr_body``, ``small_orth_core``; ``csrc/scs_panel.h``: ``k_panel_rr``, ``k_panel_tf``,
``k_gram_qaq``; the legacy loop's ``k_rr_update`` and ``k_residual``).  A helper module: pytest collects nothing here.

numpy has no extended-precision eigensolver, so a solve is judged by IDENTITIES evaluated in ``np.longdouble`` (64-bit
mantissa, asserted) on the solve's own outputs: the transform it returns must orthonormalise the matrix it was given,
the Ritz pairs must satisfy T C = C theta, the directions must be orthonormal and orthogonal to C.  A float64 host
model of each solve -- the kernel's formulas with ``numpy.linalg.eigh`` in the place of the Jacobi sweeps -- supplies
the yardstick where no bound can be derived (the single-pass orthogonality of an SVQB step scales with the
conditioning of the scaled Gram matrix): the device may be 8 times as far off as the model plus 64 k u.  The factor
8 allows for the rotation order of a parallel Jacobi against LAPACK's, the floor for a model error of zero.

Products and sums are held to Higham's bound (Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1):
K products summed in any order, fused or not, are within gamma_K sum |a_i b_i| of the exact sum and (K + 2) u covers
gamma_K plus the rounding of the reference.  K per output:

* X' = Q c, P' = Q d, S X', S P' (``k_panel_rr``, ``k_rr_update``): 3b products                          K = 3b
* R = S X' - X' theta inside ``k_panel_rr``: both 3b-term sums, the product with theta and the
  subtraction, against |SQ||c| + |theta||Q||c|                                                       K = 3b + 3
* R = S X - X theta from stored operands (``k_residual``): one product, one subtraction               K = 2
* R' = [x p r u 0 0 0] coef (``k_panel_tf``): 3b + 4 products                                        K = 3b + 4
* Z = dinv (.) R': one more rounding                                                                 K = 3b + 5
* a Gram entry over n rows, per-workgroup partials summed on the host in longdouble, against the
  Gram product of the rows the launch stored                                                         K = n
* S R = dinv (.) sum of nseg segments (``k_gram_qaq<B, 1>``): nseg - 1 additions and a product         K = nseg
* a squared residual norm of one workgroup of ``k_residual`` (256 rows): 256 squares                   K = 256
"""

from __future__ import annotations

import numpy as np
from solver_reference import LD, SENTINEL, U, require_extended_precision, worst  # noqa: F401

DROP_TOL = 1e-13  # the loop's drop_tol (csrc/scs_eig.hip, lobpcg::drop_tol)
PAD = 16  # SCS_DEBUG_PANEL_PAD

SVQB_SIZES = (1, 2, 4, 8, 12, 16, 24, 64)
SVQB_FAMILIES = ("graded", "duplicate", "zero_column", "near_1e-3", "near_1e-5", "near_1e-8", "zero", "asymmetric")
RR_SHAPES = ((4, 4), (8, 8), (12, 12), (16, 16), (12, 4), (24, 8), (36, 12), (48, 16))
RR_WAVE_SHAPES = ((12, 4), (24, 8))
RR_FAMILIES = ("generic", "converged", "repeated")
RR_MASKS = ("live", "dead_p", "all_p_dead", "dead_r", "dead_both")
RR_NPARTS = (1, 7, 8, 9, 127, 128, 129, 1024)
ORTH_WIDTHS = (4, 8)  # the projected SVQB's working set (orth_lds) holds no wider block
ORTH_PLANTED = (0.0, 1e-3, 1.0 - 1e-6)
ORTH_RANKS = ("full", "duplicate", "zero_column", "inside")
ORTH_NPARTS = (1, 8, 9, 128)
TALL_ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257, 2047, 2049, 4111, 4160)
TALL_BLOCKS = (1, 3, 128)
LEGACY_WIDTHS = (4, 8, 12, 16)


def _rotation(rs, n: int) -> np.ndarray:
    q, r = np.linalg.qr(rs.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def _orthonormal(rs, n: int, k: int) -> np.ndarray:
    q, _ = np.linalg.qr(rs.standard_normal((n, k)))
    return q


def maxabs(a) -> float:
    a = np.asarray(a)
    return float(np.max(np.abs(a))) if a.size else 0.0


def gram_ld(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A^T B in longdouble."""
    require_extended_precision()
    return a.astype(LD).T @ b.astype(LD)


# ---------------------------------------------------------------------------------------------------------------
# the fixed summation order of sum_partials (csrc/scs_eig.hip), restated: additions only, so float64 numpy gives the
# kernel's bits
# ---------------------------------------------------------------------------------------------------------------
def sum_partials_model(partial: np.ndarray) -> np.ndarray:
    """partial: nparts x nout.  Eight interleaved slices (slice s takes partials s, s + 8, ...) summed in ascending
    order from 0.0, then the slices combined in ascending order."""
    nparts, nout = partial.shape
    tmp = np.zeros((8, nout))
    for s in range(8):
        for p in range(s, nparts, 8):
            tmp[s] = tmp[s] + partial[p]
    v = tmp[0].copy()
    for s in range(1, 8):
        v = v + tmp[s]
    return v


# ---------------------------------------------------------------------------------------------------------------
# SVQB
# ---------------------------------------------------------------------------------------------------------------
def svqb_applicable(family: str, k: int) -> bool:
    # (a duplicate, a near-duplicate and an asymmetric pair need two columns)
    return k >= 2 or family in ("graded", "zero_column", "zero")


def svqb_case(family: str, k: int):
    """(Y or None, G, rank): G = Y^T Y formed in longdouble and rounded once (Y: 200 x k)."""
    require_extended_precision()
    rs = np.random.RandomState(7000 + 100 * k + SVQB_FAMILIES.index(family))
    if family == "zero":
        return None, np.zeros((k, k)), 0
    if family == "graded":
        y = _orthonormal(rs, 200, k) * 10.0 ** np.linspace(-140, 140, k)[None, :]
        rank = k
    else:
        y = rs.standard_normal((200, k))
        rank = k
        if family == "duplicate":
            y[:, k - 1] = y[:, 0]
            rank = k - 1
        elif family == "zero_column":
            y[:, k // 2] = 0.0
            rank = k - 1
        elif family.startswith("near_"):
            eps = float(family.split("_")[1])
            y[:, k - 1] = y[:, 0] + eps * np.linalg.norm(y[:, 0]) * _orthonormal(rs, 200, 1)[:, 0]
            rank = k - 1 if eps < 1e-6 else k
    g = gram_ld(y, y).astype(np.float64)
    if family == "asymmetric":  # the kernel symmetrises: only the mean of a pair may matter
        skew = np.triu(rs.standard_normal((k, k)), 1)
        g = g + skew - skew.T
    return y, g, rank


def svqb_model(g: np.ndarray, drop_tol: float):
    """k_small_svqb's formulas in float64 with LAPACK's eigensolver: (t, mask, eigenvalues of the scaled matrix)."""
    k = g.shape[0]
    d = np.diag(g)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsc = np.where(d > 1e-290, 1.0 / np.sqrt(np.where(d > 1e-290, d, 1.0)), 0.0)
    a = 0.5 * (g + g.T) * dsc[:, None] * dsc[None, :]
    a[dsc == 0.0, :] = 0.0
    a[:, dsc == 0.0] = 0.0
    w, e = np.linalg.eigh(a)
    w, e = w[::-1], e[:, ::-1]
    keep = (w[0] > 0.0) & (w > drop_tol * w[0])
    t = np.zeros((k, k))
    t[:, keep] = dsc[:, None] * e[:, keep] / np.sqrt(w[keep])[None, :]
    return t, keep.astype(np.int32), w


def svqb_identity(g: np.ndarray, t: np.ndarray, mask: np.ndarray) -> float:
    """|| T^T G T - I ||_max on the kept columns, in longdouble, G symmetrised as the kernel does."""
    require_extended_precision()
    keep = np.flatnonzero(mask)
    if len(keep) == 0:
        return 0.0
    gs = LD(0.5) * (g.astype(LD) + g.astype(LD).T)
    tk = t[:, keep].astype(LD)
    return maxabs(tk.T @ gs @ tk - np.eye(len(keep), dtype=LD))


def svqb_second_gram(y, t1: np.ndarray) -> np.ndarray:
    """(Y T1)^T (Y T1) with Y T1 formed in longdouble, rounded once: what the solver's second pass is handed."""
    y1 = y.astype(LD) @ t1.astype(LD)
    return (y1.T @ y1).astype(np.float64)


def svqb_two_pass_error(y, t1, t2, mask) -> float:
    keep = np.flatnonzero(mask)
    if len(keep) == 0:
        return 0.0
    y2 = (y.astype(LD) @ t1.astype(LD)) @ t2.astype(LD)
    return maxabs((y2.T @ y2)[np.ix_(keep, keep)] - np.eye(len(keep), dtype=LD))


def threshold_distance_ok(w: np.ndarray, drop_tol: float) -> bool:
    """Every eigenvalue ratio is >= 100 x or <= 0.01 x drop_tol: rounding cannot flip a keep / drop decision."""
    if w[0] <= 0.0:
        return True
    r = w / w[0]
    return bool(np.all((r >= 100 * drop_tol) | (r <= 0.01 * drop_tol)))


# ---------------------------------------------------------------------------------------------------------------
# Rayleigh-Ritz
# ---------------------------------------------------------------------------------------------------------------
def rr_mask(kind: str, nq: int, b: int) -> np.ndarray:
    """Basis slots [X | P | R] (the panel's layout); X is always live."""
    m = np.ones(nq, dtype=np.int32)
    if nq < 3 * b:
        assert kind == "live"
        return m
    if kind in ("dead_p", "dead_both"):
        m[b + 1] = 0
    if kind == "all_p_dead":
        m[b:2 * b] = 0
    if kind in ("dead_r", "dead_both"):
        m[2 * b + b - 1] = 0
    return m


def rr_matrix(family: str, nq: int, b: int, seed: int = 0, mask=None) -> np.ndarray:
    """T = Q^T S Q of order one: S symmetric with its spectrum in [-1, 1], Q orthonormal (60 x nq).  ``repeated`` puts
    its pair into the block of the live slots of ``mask``; the dead rows and columns then hold entries of order one
    that no result may depend on (as in the other families)."""
    rs = np.random.RandomState(9000 + 100 * nq + RR_FAMILIES.index(family) + 7 * seed)
    if family == "generic":
        m = max(60, nq + 12)
        v = _rotation(rs, m)
        s = (v * rs.uniform(-1, 1, m)) @ v.T
        q = _orthonormal(rs, m, nq)
        t = q.T @ (0.5 * (s + s.T)) @ q
    elif family == "converged":  # the X block diagonal to 1e-12, and decoupled from the rest to 1e-12
        t = np.zeros((nq, nq))
        t[:b, :b] = np.diag(np.linspace(0.95, 0.8, b))
        if nq > b:
            v = _rotation(rs, nq - b)
            t[b:, b:] = (v * rs.uniform(-0.5, 0.5, nq - b)) @ v.T
        p = 1e-12 * rs.standard_normal((nq, nq))
        p[b:, b:] = 0.0
        t = t + p
    elif family == "repeated":  # theta_b = theta_{b+1}: the pair sits across the cut (inside X when nq = b)
        live = np.arange(nq) if mask is None else np.flatnonzero(mask)
        m = len(live)
        lam = np.sort(rs.uniform(-1, 1, m))[::-1]
        cut = b - 1 if nq > b else b // 2
        lam[cut] = lam[cut + 1]
        v = _rotation(rs, m)
        t = rs.uniform(-1, 1, (nq, nq))
        t[np.ix_(live, live)] = (v * lam) @ v.T
    else:
        raise ValueError(family)
    return 0.5 * (t + t.T)


def rr_vanishing(nq: int, b: int, slot: int) -> np.ndarray:
    """A generic T whose basis slot ``slot`` (>= b) is itself the top Ritz vector: decoupled, with the largest value.
    Its pair is never rotated, so column 0 of C is e_slot exactly and its search direction vanishes exactly."""
    t = rr_matrix("generic", nq, b, seed=3)
    t[slot, :] = 0.0
    t[:, slot] = 0.0
    t[slot, slot] = 2.0
    return t


def rr_nearly_vanishing(nq: int, b: int, slot: int, eps: float = 1e-6) -> np.ndarray:
    """The same with the slot coupled to every other one at ``eps``: the top Ritz vector keeps eps of its norm in
    the X block, so eps of its search direction is left after (I - C C^T).  One projection leaves about nq u of
    the direction's ORIGINAL norm along C, which is nq u / eps = 1e-10 nq of what is left -- the second projection is
    what brings C^T D under 64 nq u here, and on no other family (their directions keep a third of their norm)."""
    t = rr_vanishing(nq, b, slot)
    sign = np.where(np.arange(nq) % 2 == 0, 1.0, -1.0)
    t[slot, :] = eps * sign
    t[:, slot] = eps * sign
    t[slot, slot] = 2.0
    return t


def rr_assemble(t: np.ndarray, mask: np.ndarray, exact_from: int = -1) -> np.ndarray:
    """The masked, symmetrised matrix small_rr_body solves.  exact_from >= 0: of a pair with an index below it the
    entry with the exact product is taken, T[max(i, j)][min(i, j)] = Q_j^T (S Q_i), i < j."""
    nq = t.shape[0]
    a = 0.5 * (t + t.T)
    if exact_from >= 0:
        low = np.tril(t, -1)
        one_sided = low + low.T
        i, j = np.indices((nq, nq))
        pick = (i != j) & ((i < exact_from) | (j < exact_from))
        a = np.where(pick, one_sided, a)
    live = (mask[:, None] != 0) & (mask[None, :] != 0)
    a = np.where(live, a, 0.0)
    a[np.arange(nq)[mask == 0], np.arange(nq)[mask == 0]] = -1e30
    return a


def eigh_deflated(a: np.ndarray):
    """Eigenpairs of the symmetric ``a`` in descending order, with every slot whose off-diagonal entries are all
    exactly zero taken as the pair (a_jj, e_j) -- the Jacobi never rotates a pair with a zero entry, so on the device a
    dead slot (-1e30) or a decoupled one stays an exact unit vector; LAPACK works relative to ||a|| and would smear
    1e30 u over the rest."""
    n = a.shape[0]
    off = a - np.diag(np.diag(a))
    iso = ~off.any(axis=0)
    rest = np.flatnonzero(~iso)
    w, e = np.empty(n), np.zeros((n, n))
    w[:len(rest)], sub = np.linalg.eigh(a[np.ix_(rest, rest)]) if len(rest) else (np.empty(0), np.empty((0, 0)))
    e[np.ix_(rest, np.arange(len(rest)))] = sub
    for k, j in enumerate(np.flatnonzero(iso)):
        w[len(rest) + k] = a[j, j]
        e[j, len(rest) + k] = 1.0
    order = np.argsort(-w, kind="stable")
    return w[order], e[:, order]


def rr_model(t: np.ndarray, b: int, mask: np.ndarray, drop_tol: float, exact_from: int = -1, defect: str = ""):
    """small_rr_body's general path in float64 with LAPACK: (c, d, theta, mask_p, eigenvalues of the directions' scaled
    Gram matrix or None).  ``defect`` plants one of the faults the identities must notice."""
    nq = t.shape[0]
    a = rr_assemble(t, mask, exact_from)
    w, e = eigh_deflated(a)
    c = e[:, :b].copy()
    theta = w[:min(b + 1, nq)].copy()
    if nq == b:
        return c, None, theta, None, None
    d = c.copy()
    d[:b] = 0.0
    for _ in range(1 if defect == "one_projection" else 2):
        d = d - c @ (c.T @ d)
    g = d.T @ d
    dg = np.diag(g)
    dsc = np.where(dg > 1e-290, 1.0 / np.sqrt(np.where(dg > 1e-290, dg, 1.0)), 0.0)
    sa = 0.5 * (g + g.T) * dsc[:, None] * dsc[None, :]
    lw, le = np.linalg.eigh(sa)
    lw, le = lw[::-1], le[:, ::-1]
    keep = (lw[0] > 0.0) & (lw > drop_tol * lw[0])
    tt = np.zeros((b, b))
    tt[:, keep] = dsc[:, None] * le[:, keep] / np.sqrt(lw[keep])[None, :]
    dout = d @ tt
    mask_p = keep.astype(np.int32)
    if defect == "mask_late":  # mask_p written one slot late
        mask_p = np.roll(mask_p, 1)
    if defect == "dropped_direction":  # a kept direction comes back as a zero column
        dout[:, 0] = 0.0
    if defect == "dead_row_leak":
        dead = np.flatnonzero(mask == 0)
        if len(dead):
            dout[dead[0], 0] += 1e-9
    return c, dout, theta, mask_p, lw


def rr_identities(t: np.ndarray, b: int, mask: np.ndarray, c, d, theta, mask_p, exact_from: int = -1) -> dict:
    """Every identity of the Rayleigh-Ritz outputs, in longdouble, against the masked matrix the kernel defines."""
    require_extended_precision()
    nq = t.shape[0]
    a = rr_assemble(t, mask, exact_from)
    al, cl = a.astype(LD), c.astype(LD)
    nth = min(b + 1, nq)
    out = {
        "c_orth": maxabs(cl.T @ cl - np.eye(b, dtype=LD)),
        # (dead rows of C must be exactly zero, so the -1e30 on the diagonal contributes nothing)
        "c_res": maxabs(np.where(mask[:, None] != 0, al, LD(0)) @ cl - cl * theta[:b].astype(LD)[None, :]),
        "theta": maxabs(theta[:nth] - eigh_deflated(a)[0][:nth]),  # LAPACK on the live, coupled block
        "descending": bool(np.all(np.diff(theta[:nth]) <= 0)),
        "dead_rows_c": maxabs(c[mask == 0]),
    }
    if d is not None:
        keep = np.flatnonzero(mask_p)
        dl = d.astype(LD)
        out["d_orth"] = maxabs((dl.T @ dl)[np.ix_(keep, keep)] - np.eye(len(keep), dtype=LD)) if len(keep) else 0.0
        out["d_dropped"] = maxabs(d[:, mask_p == 0])
        out["cd"] = maxabs(cl.T @ dl)
        out["dead_rows_d"] = maxabs(d[mask == 0])
    return out


def rr_bars(nq: int, model_d_orth: float = 1e-6 / 8) -> dict:
    """The project's Jacobi bars (scale 1) for C and theta, and the derived 64 nq u for C^T D: D comes out of two
    projections against C in nq-term sums, each leaving at most a few nq u of a unit column along C.  D^T D - I is
    the single-pass orthogonality of an SVQB step: it scales with the conditioning of the directions' scaled Gram
    matrix (3.7e-6 where all of P is dead on a converged block), so it is held to the host model's on the same
    input (``model_bound``); the model on its own must stay below 1e-6."""
    return {"c_orth": 1e-12, "c_res": 1e-11, "theta": 1e-12, "d_orth": model_bound(model_d_orth, nq),
            "cd": 64 * nq * U, "dead_rows_c": 0.0, "dead_rows_d": 0.0, "d_dropped": 0.0}


def rr_failures(ident: dict, nq: int, model_d_orth: float = 1e-6 / 8) -> list:
    bars = rr_bars(nq, model_d_orth)
    bad = [k for k, bar in bars.items() if k in ident and not ident[k] <= bar]
    if not ident["descending"]:
        bad.append("descending")
    return bad


def rr_direction_block(c: np.ndarray, b: int) -> np.ndarray:
    """(I - C C^T) applied to the [P R] rows of C, in longdouble, rounded."""
    cl = c.astype(LD)
    w = cl.copy()
    w[:b] = 0
    w = w - cl @ (cl.T @ w)
    return w.astype(np.float64)


def projector_difference(d: np.ndarray, w: np.ndarray) -> float:
    """|| P_D - P_W ||_max for the spans of the non-zero columns of D and of W."""
    d = d[:, np.abs(d).max(axis=0) > 0]
    qd, _ = np.linalg.qr(d)
    qw, _ = np.linalg.qr(w)
    if qd.shape[1] != qw.shape[1]:
        return float("inf")
    return maxabs(qd @ qd.T - qw @ qw.T)


def direction_conditioning(c: np.ndarray, b: int) -> float:
    """Smallest singular value of the projected direction block with unit columns: what is left of each direction,
    and of each combination of them, after the projection."""
    w = rr_direction_block(c, b)
    nrm = np.linalg.norm(w, axis=0)
    keep_norm = np.linalg.norm(c[b:], axis=0)
    if np.any(keep_norm == 0) or np.any(nrm / keep_norm < 1e-3):
        return 0.0
    return float(np.linalg.svd(w / nrm[None, :], compute_uv=False)[-1])


def dyadic_split(t: np.ndarray, nparts: int, seed: int, grid: int = 30):
    """(T rounded to multiples of 2^-grid, nparts x nq x nq partials on the same grid that sum to it exactly in any
    order: every partial sum is an integer multiple of the grid below 2^53 grids)."""
    rs = np.random.RandomState(seed)
    scale = 2.0 ** grid
    tq = np.round(t * scale)
    parts = rs.randint(-(1 << grid), (1 << grid) + 1, size=(nparts,) + t.shape).astype(np.float64)
    parts[-1] = tq - parts[:-1].sum(axis=0)
    assert np.array_equal(parts.sum(axis=0), tq) and np.abs(parts).max() < 2.0 ** 45
    return tq / scale, parts / scale


def plain_split(t: np.ndarray, nparts: int, seed: int) -> np.ndarray:
    """Partials that sum to T up to rounding (no grid): positive weights, the last partial takes the remainder."""
    rs = np.random.RandomState(seed)
    wts = rs.uniform(0.5, 1.5, nparts)
    wts /= wts.sum()
    parts = t[None] * wts.reshape((nparts,) + (1,) * t.ndim)
    parts[-1] = (t.astype(LD) - parts[:-1].astype(LD).sum(axis=0)).astype(np.float64)
    return np.ascontiguousarray(parts)


# ---------------------------------------------------------------------------------------------------------------
# projected SVQB
# ---------------------------------------------------------------------------------------------------------------
def orth_rank(rank: str, b: int) -> int:
    return {"full": b, "duplicate": b - 1, "zero_column": b - 1, "inside": b - 2}[rank]


def orth_case(b: int, planted: float, rank: str, with_u: bool, n: int = 300):
    """(u or None, X, P, R) with [u X P] orthonormal and R = planted x (a unit vector of span[u X P]) + sqrt(1 -
    planted^2) x (a unit vector orthogonal to it), column by column.  ``inside``: columns 1 and 2 of R lie in the span
    but for 1e-14 of their squared norm.  The projected norm^2 the kernel forms, dgn = G_cc - sum of 2b + 1 squares,
    carries at most (2b + 3) u G_cc = 2.1e-15 G_cc of cancellation noise at b = 8, so the computed ratio dgn / G_cc
    lies in 0.79e-14 ... 1.21e-14: positive, and a factor 8 under the guard's 1e-13 -- the guard declares the column
    dead whatever the rounding, and a kernel without the guard scales that noise up to a unit direction."""
    rs = np.random.RandomState(11000 + 100 * b + 10 * ORTH_RANKS.index(rank) + int(with_u) + int(planted * 7919) % 97)
    basis = _orthonormal(rs, n, 3 * b + 1)
    span, free = basis[:, :2 * b + 1], basis[:, 2 * b + 1:]
    if not with_u:
        span = span[:, 1:]
    inside = span @ _orthonormal(rs, span.shape[1], b)
    outside = free @ _rotation(rs, b)
    r = planted * inside + np.sqrt(1.0 - planted * planted) * outside
    r = r * rs.uniform(0.5, 2.0, b)[None, :]
    if rank == "duplicate":
        r[:, b - 1] = r[:, 0]
    elif rank == "zero_column":
        r[:, b // 2] = 0.0
    elif rank == "inside":
        r[:, 1] = inside[:, 1] + 1e-7 * outside[:, 1]
        r[:, 2] = 0.5 * (inside[:, 2] + 1e-7 * outside[:, 2])
    u = basis[:, 0].copy() if with_u else None
    x, p = basis[:, 1:b + 1].copy(), basis[:, b + 1:2 * b + 1].copy()
    return u, x, p, np.ascontiguousarray(r)


def orth_gram(u, x, p, r) -> np.ndarray:
    """The 3 b^2 + b outputs a tall kernel hands the projected SVQB -- [x p]^T r, r^T r, u^T r -- from longdouble."""
    b = r.shape[1]
    xp = np.concatenate([x, p], axis=1)
    out = np.zeros(3 * b * b + b)
    out[:2 * b * b] = gram_ld(xp, r).astype(np.float64).ravel()
    out[2 * b * b:3 * b * b] = gram_ld(r, r).astype(np.float64).ravel()
    if u is not None:
        out[3 * b * b:] = gram_ld(u[:, None], r).astype(np.float64).ravel()
    return out


def orth_model(gsum: np.ndarray, b: int, drop_tol: float, defect: str = ""):
    """small_orth_core's formulas in float64 with LAPACK on the summed outputs: (coef, mask, scaled eigenvalues,
    dgn / gm per column)."""
    cxp = gsum[:2 * b * b].reshape(2 * b, b)
    gm = gsum[2 * b * b:].reshape(b + 1, b)
    mm = 0.5 * (gm[:b] + gm[:b].T) - np.outer(gm[b], gm[b]) - cxp.T @ cxp
    dgn, gd = np.diag(mm), np.diag(gm[:b])
    guard = np.full(b, True) if defect == "no_guard" else dgn > 1e-13 * gd
    ok = (dgn > 1e-290) & guard
    dsc = np.where(ok, 1.0 / np.sqrt(np.where(ok, dgn, 1.0)), 0.0)
    w, e = np.linalg.eigh(0.5 * (mm + mm.T) * dsc[:, None] * dsc[None, :])
    w, e = w[::-1], e[:, ::-1]
    keep = (w[0] > 0.0) & (w > drop_tol * w[0])
    tt = np.zeros((b, b))
    tt[:, keep] = dsc[:, None] * e[:, keep] / np.sqrt(w[keep])[None, :]
    coef = np.zeros((3 * b + 4, b))
    coef[:2 * b] = -cxp @ tt
    coef[2 * b:3 * b] = tt
    coef[3 * b] = -gm[b] @ tt
    if defect == "no_u":
        coef[3 * b] = 0.0
    if defect == "pad":
        coef[3 * b + 1, 0] = 1e-3
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(gd > 0, dgn / np.where(gd > 0, gd, 1.0), 0.0)
    return coef, keep.astype(np.int32), w, ratio


def orth_errors(u, x, p, r, coef: np.ndarray, mask: np.ndarray):
    """(|| R'^T R' - I ||_max on the kept columns, || [u X P]^T R' ||_max) for R' = R T + [x p u] K in longdouble."""
    b = r.shape[1]
    cl = coef.astype(LD)
    rp = x.astype(LD) @ cl[:b] + p.astype(LD) @ cl[b:2 * b] + r.astype(LD) @ cl[2 * b:3 * b]
    if u is not None:
        rp = rp + np.outer(u.astype(LD), cl[3 * b])
    keep = np.flatnonzero(mask)
    orth = maxabs((rp.T @ rp)[np.ix_(keep, keep)] - np.eye(len(keep), dtype=LD)) if len(keep) else 0.0
    basis = np.concatenate(([u[:, None]] if u is not None else []) + [x, p], axis=1).astype(LD)
    return orth, maxabs(basis.T @ rp)


def model_bound(model_error: float, k: int) -> float:
    """What a device result may show where the model shows ``model_error``: 8 x that plus 64 k u."""
    return 8.0 * model_error + 64 * k * U


# ---------------------------------------------------------------------------------------------------------------
# tall kernels
# ---------------------------------------------------------------------------------------------------------------
def tall_panels(n: int, b: int, seed: int):
    """(q, aq, u, dinv): panels of n + PAD rows and 3b columns of order one; the rows past n hold SENTINEL."""
    rs = np.random.RandomState(13000 + 31 * n + b + 1000 * seed)
    rows = n + PAD
    q, aq = rs.standard_normal((rows, 3 * b)), rs.standard_normal((rows, 3 * b)) + 0.25
    u, dinv = rs.standard_normal(rows) + 0.5, rs.uniform(0.1, 2.0, rows)
    for m in (q, aq, u, dinv):
        m[n:] = SENTINEL
    return q, aq, u, dinv


def product_ld(a: np.ndarray, c: np.ndarray):
    """(A C, |A| |C|) in longdouble."""
    al, cl = a.astype(LD), c.astype(LD)
    return al @ cl, np.abs(al) @ np.abs(cl)


def budget(k: int, mag: np.ndarray) -> np.ndarray:
    return (k + 2) * LD(U) * mag


def panel_rr_reference(q, aq, c, d, theta, n: int, b: int):
    """k_panel_rr on rows [0, n): references and budgets of the new Q = [X' P' R] and SQ = [SX' SP' .]."""
    cd = np.concatenate([c, d], axis=1)
    xq, mq = product_ld(q[:n], cd)
    xa, ma = product_ld(aq[:n], cd)
    th = theta[:b].astype(LD)[None, :]
    res = xa[:, :b] - xq[:, :b] * th
    mres = ma[:, :b] + mq[:, :b] * np.abs(th)
    return {"q_xp": (xq, budget(3 * b, mq)), "aq_xp": (xa, budget(3 * b, ma)), "r": (res, budget(3 * b + 3, mres))}


def panel_tf_reference(q, u, coef, n: int, b: int):
    """R' = [x p r u] coef on rows [0, n) (u None: the row of coefficients multiplies nothing)."""
    ext = np.concatenate([q[:n], (u[:n, None] if u is not None else np.zeros((n, 1)))], axis=1)
    ref, mag = product_ld(ext, coef[:3 * b + 1])
    return ref, mag


def gram_budget(a: np.ndarray, bm: np.ndarray, n: int):
    al, bl = a[:n].astype(LD), bm[:n].astype(LD)
    return al.T @ bl, budget(n, np.abs(al).T @ np.abs(bl))


def panel_partials_reference(q_new, u, n: int, b: int):
    """The 3 b^2 + b Gram outputs of k_panel_rr / k_panel_tf from the rows the launch stored: [x p]^T r, r^T r, u^T r."""
    r = q_new[:, 2 * b:]
    a, ba = gram_budget(q_new[:, :2 * b], r, n)
    g, bg = gram_budget(r, r, n)
    if u is not None:
        cu, bu = gram_budget(u[:, None], r, n)
    else:
        cu, bu = np.zeros((1, b), dtype=LD), np.zeros((1, b), dtype=LD)
    return (np.concatenate([a.ravel(), g.ravel(), cu.ravel()]), np.concatenate([ba.ravel(), bg.ravel(), bu.ravel()]))
