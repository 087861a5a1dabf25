"""Host references and error budgets for the kernels inside the LOBPCG loop (``csrc/scs_eig.hip``): the operator
(``k_symm``, ``k_symm_tri``, the single-precision image), the Gram products (``k_gram``, ``k_gram_mfma``), the panel
update (``k_update``) and the Rayleigh-Ritz Jacobi (``k_small_eig``).  A helper module: pytest collects nothing here.

Reference values are computed in ``np.longdouble`` (x87 extended: 64-bit mantissa), chunked over rows.

The budgets are derived from the arithmetic, not tuned against the kernels.  With u = 2^-53 (round to nearest,
fp64) a sum of n products formed in ANY order, with or without fused multiply-adds, in any number of partial sums,
differs from the exact one by at most gamma_n sum |a_i b_i|, gamma_n = n u / (1 - n u) (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., section 3.1); (n + 2) u covers gamma_n for every n below 2^50 and leaves
room for the rounding of the reference itself (2^-64 a term).

* Gram:    |got - ref|_ij <= (n + 2) u (|A|^T |B|)_ij.
* update:  Y' = alpha Y + sign A C is a sum of ka + 1 terms (alpha and sign are 0 or +-1 in the solver: exact):
           |got - ref|_ij <= (ka + 3) u (|alpha| |Y| + |A| |C|)_ij.
* apply:   y = d^-1/2 W d^-1/2 x with the degrees d = W 1 computed on the device.  The product sum has V terms
           (V u); each of the two scalings carries the relative error of a V-term sum of non-negative numbers
           under a reciprocal square root (V u / 2 each) plus the rounding of the square root, the division and
           the two multiplications (a handful of u: 16 covers them with room to spare):
           |got - ref|_i <= (2 V + 16) u (|S| |x|)_i,   S = d^-1/2 W d^-1/2, scale 1 where the degree is 0.
* image:   the same budget against W32 = float64(float32(W)) with the degrees of W: the kernel computes in double
           precision on a round-to-nearest single-precision copy.
"""

from __future__ import annotations

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

# ---------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU test of this module and the GPU tests)
# ---------------------------------------------------------------------------------------------------------------
TRI_SIZES = (4096, 4097, 4223, 4224, 4225, 4351, 4352, 4607, 4608, 4609, 6000, 8191)
SYMM_SIZES = (129, 255, 256, 257, 511, 513, 1023, 1025, 2500, 4095)
WIDTHS = (4, 8, 12, 16)
PANEL_ROWS = (1, 3, 4, 5, 63, 64, 65, 255, 257, 4099, 100003)
SENTINEL = 1e300  # fills the columns of a panel that a kernel must neither read nor write
GRAM_PATTERNS = ("x_ax", "q_r", "q_aq", "u_y")
UPDATE_PATTERNS = ("u", "in_place", "q_r")
JACOBI_SIZES = (2, 3, 4, 5, 7, 8, 12, 16, 23, 24, 36, 48, 64)
JACOBI_FAMILIES = ("zero", "identity", "rank_one", "repeated", "cluster", "graded", "ritz", "gauss_1e+150",
                   "gauss_1e-150", "ritz_separated")
# scs_fiedler sets `gram_blocks = 256` for every n (csrc/scs_eig.hip, solver::bind: "gram_blocks = 256"): the product's value
# and the old hook's coincide.  The others: one partial, the panel kernels' cap, and what the partials buffer holds.
FIEDLER_GRAM_BLOCKS = 256
GRAM_BLOCKS = (FIEDLER_GRAM_BLOCKS, 1, 128, 1024)


def require_extended_precision() -> None:
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"


def _row_chunks(n: int, width: int, target: int = 1 << 21):
    step = max(1, target // max(1, width))
    for r0 in range(0, n, step):
        yield r0, min(n, r0 + step)


# ---------------------------------------------------------------------------------------------------------------
# operator
# ---------------------------------------------------------------------------------------------------------------
def scaling(w: np.ndarray) -> np.ndarray:
    """d^-1/2 in extended precision from the full symmetric W; 1 where the degree is 0."""
    require_extended_precision()
    deg = np.zeros(w.shape[1], dtype=LD)
    for r0, r1 in _row_chunks(w.shape[0], w.shape[1]):
        deg += w[r0:r1].astype(LD).sum(axis=0)  # (column sums of a symmetric matrix: its degrees)
    out = np.ones_like(deg)
    pos = deg != 0
    out[pos] = 1 / np.sqrt(deg[pos])
    return out


def image_model(w: np.ndarray) -> np.ndarray:
    """What the single-precision image holds, as doubles: every entry of W rounded to nearest float."""
    return w.astype(np.float32).astype(np.float64)


def apply_reference(w: np.ndarray, x: np.ndarray, w_op: np.ndarray | None = None, row_begin: int = 0):
    """(ref, budget) of rows [row_begin, row_begin + rows) of S x: ``w`` (rows x V, or V x V when the degrees are
    to come from it) gives the degrees, ``w_op`` (default: ``w``) the entries that are multiplied."""
    assert w.shape[0] == w.shape[1], "the degrees need the whole matrix"
    v = w.shape[0]
    dinv = scaling(w)
    m = w if w_op is None else w_op
    z = dinv[:, None] * x.astype(LD)
    both = np.concatenate([z, np.abs(z)], axis=1)
    nonneg = bool(m.min() >= 0)
    ref = np.empty(x.shape, dtype=LD)
    mag = np.empty(x.shape, dtype=LD)
    b = x.shape[1]
    for r0, r1 in _row_chunks(v, v):
        mc = m[r0:r1].astype(LD)
        if nonneg:  # |W| = W: one product gives both
            p = mc @ both
            ref[r0:r1], mag[r0:r1] = p[:, :b], p[:, b:]
        else:
            ref[r0:r1] = mc @ z
            mag[r0:r1] = np.abs(mc) @ both[:, b:]
    ref *= dinv[:, None]
    mag *= dinv[:, None]
    return ref[row_begin:], apply_budget(v, mag)[row_begin:]


def apply_budget(v: int, mag: np.ndarray) -> np.ndarray:
    return (2 * v + 16) * LD(U) * mag


def apply_vectors(v: int, b: int, seed: int, graded: bool = False) -> np.ndarray:
    x = np.random.RandomState(seed).standard_normal((v, b))
    if graded:  # columns of very different magnitude: the elementwise budget has to hold in each of them
        x *= np.array([1.0, 1e-8, 1e8, 1.0] * (b // 4))[None, :]
    return x


# ---------------------------------------------------------------------------------------------------------------
# Gram products and panel updates
# ---------------------------------------------------------------------------------------------------------------
def gram_reference(a: np.ndarray, b: np.ndarray):
    """(ref, budget) of A^T B for the (n x ka) and (n x kb) blocks given."""
    require_extended_precision()
    n = a.shape[0]
    ref = np.zeros((a.shape[1], b.shape[1]), dtype=LD)
    mag = np.zeros_like(ref)
    for r0, r1 in _row_chunks(n, max(a.shape[1], b.shape[1]), 1 << 18):
        al, bl = a[r0:r1].astype(LD), b[r0:r1].astype(LD)
        ref += al.T @ bl
        mag += np.abs(al).T @ np.abs(bl)
    return ref, (n + 2) * LD(U) * mag


def update_reference(y: np.ndarray, alpha: float, a: np.ndarray, c: np.ndarray, sign: float):
    """(ref, budget) of alpha Y + sign A C; Y is not looked at when alpha is 0 (it may hold anything)."""
    require_extended_precision()
    al, cl = a.astype(LD), c.astype(LD)
    ref = LD(sign) * (al @ cl)
    mag = np.abs(al) @ np.abs(cl)
    if alpha != 0.0:
        ref += LD(alpha) * y.astype(LD)
        mag += abs(alpha) * np.abs(y).astype(LD)
    return ref, (a.shape[1] + 3) * LD(U) * mag


def _panel(rs, n: int, width: int, col0: int, k: int, shift: float = 0.0) -> np.ndarray:
    p = np.full((n, width), SENTINEL)
    p[:, col0:col0 + k] = rs.standard_normal((n, k)) + shift
    return p


def gram_case(pattern: str, b: int, n: int):
    """The operands of one of the solver's four Gram calls as (a, a_col0, ka, bm, b_col0, kb): blocks of 3b-wide
    panels whose other columns hold SENTINEL.  ``bm is a`` where the solver passes two blocks of one panel."""
    rs = np.random.RandomState(1000 * b + n % 997 + 17 * GRAM_PATTERNS.index(pattern))
    q3 = 3 * b
    if pattern == "x_ax":  # gram(X, 3b, b, AX, 3b, b): equal blocks of two panels (here: P's and R's columns)
        return _panel(rs, n, q3, b, b), b, b, _panel(rs, n, q3, 2 * b, b, 0.25), 2 * b, b
    if pattern == "q_r":  # gram(Q, 3b, 2b, R, 3b, b): R is the last block of Q
        q = rs.standard_normal((n, q3))
        q[:, 2 * b:] += 0.25
        return q, 0, 2 * b, q, 2 * b, b
    if pattern == "q_aq":  # gram(Q, 3b, 3b, AQ, 3b, 3b): the whole panels
        return rs.standard_normal((n, q3)), 0, q3, rs.standard_normal((n, q3)) + 0.25, 0, q3
    if pattern == "u_y":  # gram(u, 1, 1, Y, 3b, b): leading dimension 1
        return rs.standard_normal((n, 1)) + 0.5, 0, 1, _panel(rs, n, q3, b, b), b, b
    raise ValueError(pattern)


def update_case(pattern: str, b: int, n: int, alpha: float):
    """One of the solver's three update calls as (y, y_col0, kc, a, a_col0, ka, c): ``a is y`` where it passes
    blocks of one panel.  alpha = 0 must not read Y (the BLAS convention, and the kernel's own comment): a Y block
    that is written without being an operand starts as NaN."""
    rs = np.random.RandomState(2000 * b + n % 991 + 13 * UPDATE_PATTERNS.index(pattern))
    q3 = 3 * b
    if pattern == "u":  # update(Y, 3b, b, 1, u, 1, 1, C, b, -1): Y -= u (u^T Y)
        y = _panel(rs, n, q3, 2 * b, b)
        if alpha == 0.0:
            y[:, 2 * b:] = np.nan
        return y, 2 * b, b, rs.standard_normal((n, 1)), 0, 1, rs.standard_normal((1, b))
    if pattern == "in_place":  # update(Y, 3b, b, 0, Y, 3b, b, T, b, 1): Y = Y T, reads before writes
        y = _panel(rs, n, q3, b, b)
        return y, b, b, y, b, b, rs.standard_normal((b, b))
    if pattern == "q_r":  # update(R, 3b, b, 1, Q, 3b, 2b, C, b, -1): R -= [X | P] C inside one panel
        y = rs.standard_normal((n, q3))
        if alpha == 0.0:
            y[:, 2 * b:] = np.nan
        return y, 2 * b, b, y, 0, 2 * b, rs.standard_normal((2 * b, b))
    raise ValueError(pattern)


def worst(got: np.ndarray, ref: np.ndarray, budget: np.ndarray):
    """(ratio, index) of the entry with the largest |got - ref| / budget; a NaN or an error over a zero budget
    counts as infinite."""
    err = np.abs(got.astype(LD) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, LD(0), err / budget)
    ratio = np.where(np.isnan(ratio), LD(np.inf), ratio).astype(np.float64)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


# ---------------------------------------------------------------------------------------------------------------
# Jacobi
# ---------------------------------------------------------------------------------------------------------------
def _rotation(rs, n: int) -> np.ndarray:
    q, r = np.linalg.qr(rs.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def jacobi_case(family: str, n: int) -> np.ndarray:
    rs = np.random.RandomState(100 * n + JACOBI_FAMILIES.index(family))
    if family == "zero":
        return np.zeros((n, n))
    if family == "identity":
        return np.eye(n)
    if family == "rank_one":
        v = rs.standard_normal(n)
        return np.outer(v, v)
    if family in ("repeated", "cluster", "graded"):
        if family == "repeated":  # exactly repeated eigenvalues (three values) under a random rotation
            lam = np.array([1.0, 0.5, -0.25])[np.arange(n) % 3]
        elif family == "cluster":  # spaced 1e-13 apart, just below 1
            lam = 1.0 - 1e-3 - 1e-13 * np.arange(n)
        else:
            lam = 10.0 ** np.linspace(0, -15, n)
        q = _rotation(rs, n)
        a = (q * lam) @ q.T
        return 0.5 * (a + a.T)
    if family == "ritz":  # a converged Rayleigh-Ritz matrix: nearly diagonal, two values 1e-12 apart
        th = np.sort(rs.uniform(0.9, 1.0, n))[::-1]
        th[1] = th[0] - 1e-12
        p = 1e-9 * rs.standard_normal((n, n))
        return np.diag(th) + 0.5 * (p + p.T)
    if family == "ritz_separated":
        # The family that separates the LAST sweep.  diag(theta), theta evenly spaced over [0.5, 1] (gaps >= 1/128),
        # plus symmetric off-diagonal entries of magnitude 1e-10 ... 2e-10 and random sign: unrotated, those entries
        # ARE the residual (ten times the 1e-11 bar), and one sweep takes them to second order, at most
        # eps^2 sum_k 1 / |theta_i - theta_k| < 4e-20 * 4 (n - 1) (1 + ln n) = 5e-17 an entry at n = 64, under the
        # kernel's own stopping rule (off-diagonal mass <= 1.1e-16 n ||diag||_F, i.e. 7e-16 an entry at n = 64; at
        # n = 2 the one rotation annihilates the one entry).  So the kernel needs exactly one sweep here, and a
        # kernel that stops one sweep early returns the input and misses the bar; the cluster and ritz families
        # cannot show that (one sweep before the end they are already within 1e-12).
        p = np.triu(1e-10 * (1.0 + rs.uniform(size=(n, n))) * rs.choice([-1.0, 1.0], size=(n, n)), 1)
        return np.diag(np.linspace(1.0, 0.5, n)) + p + p.T
    if family.startswith("gauss_"):
        a = rs.standard_normal((n, n))
        return (a + a.T) * float(family.split("_")[1])
    raise ValueError(family)


def jacobi_errors(a: np.ndarray, w: np.ndarray, v: np.ndarray, normalise: bool):
    """(eigenvalue error, residual, orthogonality error, scale) against LAPACK.  ``normalise``: the matrix and the
    eigenvalues are divided by ||A||_2 first (the two badly scaled families: the bars are absolute above scale 1)."""
    w_ref = np.linalg.eigvalsh(a)[::-1]
    if normalise:
        nrm = float(np.abs(w_ref).max())
        a, w, w_ref = a / nrm, w / nrm, w_ref / nrm
    scale = max(1.0, float(np.abs(w_ref).max()))
    return (float(np.max(np.abs(w - w_ref))), float(np.max(np.abs(a @ v - v * w))),
            float(np.max(np.abs(v.T @ v - np.eye(len(w))))), scale)


# ---------------------------------------------------------------------------------------------------------------
# a whole solve: the reported residual against the extended-precision operator
# ---------------------------------------------------------------------------------------------------------------
def check_against_reference(w, dinv, maps, stats, case: str, image: bool = False):
    """The residual norms ``scs_fiedler`` reports against S x - lambda x in extended precision, formed on the host
    from the downloaded W and the returned pair.  With x = maps / d^-1/2 scaled to unit length the two differ by at most

    * the budget of one application, ``(2 V + 16) u (|S| |x|)`` entrywise (``apply_reference``), 2-norm;
    * what recovering x from the embedding adds: every entry carries the device's d^-1/2 (relative error
      (V / 2 + 4) u, the same terms the apply budget counts) and one product, and ``||S - lambda|| <= 2``:
      ``(V + 8) u``;
    * the residual norm itself, a Gram product over V rows: ``(V + 2) u`` relative;
    * the rotation that closes start-up and confirmation (``X <- X T``, ``S X <- (S X) T``, sums of b + 1 terms,
      b <= 8, on both sides): ``4 (b + 3) u <= 44 u``.

    ``image``: the product the report rests on streamed the single-precision image (start-up of the image loop; a
    confirmed solve always reports through W), so the reference multiplies the image's entries, as ``apply_reference``
    provides."""
    v = w.shape[0]
    assert np.isfinite(maps).all() and np.isfinite(stats["lambda"]).all() and np.isfinite(stats["resid"]).all(), case
    cols = (1,) if stats["used_constraint"] else (0, 1)
    x = maps[:, cols].astype(LD) / dinv[:, None]
    norm = np.sqrt((x * x).sum(axis=0))
    assert (norm > 0).all(), case
    x64 = (x / norm).astype(np.float64)  # (what the reference is given; its own rounding, u, is inside 44 u)
    sx, budget = apply_reference(w, x64, w_op=image_model(w) if image else None)
    b = stats["block"]
    for k, col in enumerate(cols):
        lam = LD(stats["lambda"][col])
        r = sx[:, k] - lam * x64[:, k].astype(LD)
        want = float(np.sqrt((r * r).sum()))
        got = float(stats["resid"][col])
        slack = (float(np.sqrt((budget[:, k] ** 2).sum())) + (v + 8) * U + (v + 2) * U * max(got, want)
                 + 4 * (b + 3) * U)
        print(f"[chain] {case} column {col}: reported {got:.3e}, reference {want:.3e}, slack {slack:.3e}, "
              f"{stats['iterations']} iterations")
        assert abs(got - want) <= slack, (f"{case} column {col}: reported {got:.6e}, reference {want:.6e}, "
                                          f"slack {slack:.3e}")
    return cols
