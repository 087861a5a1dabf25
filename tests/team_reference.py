"""A host model of what exists only when a solve has more than one rank (``csrc/scs_eig.hip``, ``world > 1``): which
cells of W a rank of the upper-triangle job stores and how ``k_symm_tri`` / ``k_symm_tri_finish`` apply them, the
rank's share of the degrees (``k_degrees_upper_rows`` / ``_cols``), and the receive buffer of the row-partitioned job
(``world`` chunks of ``max_rows * b`` doubles, ``k_unpack`` and ``k_gram_qaq<B, 2>`` its readers).  Plain numpy, values in
``np.longdouble`` where they meet the device; the cases of ``tests/test_gpu_team_edges.py``,
held to their numbers by ``tests/test_team_reference_cpu.py``.  A helper module: pytest collects nothing here.

The operator's reference and every budget are ``solver_reference``'s (apply ``(2V + 16) u |S||x|``, Gram
``(n + 2) u |A|^T|B|``), the degree budget and the forests are ``build_reference``'s; nothing here restates them."""

from __future__ import annotations

import build_reference as br
import numpy as np
import solver_reference as sr

from spectralclustersupertree_amd.partition import row_splits, row_splits_upper
from spectralclustersupertree_amd.treearrays import TreeArrays

LD = sr.LD
TW = 256  # the upper-triangle job's tile width: a row is stored from the first column of its diagonal tile on
WIDTHS = sr.WIDTHS
FUSED_WIDTHS = (4, 8)  # the fused loop's, and the symmetric schedule's
REPS = 3  # forwards, backwards, forwards
FIEDLER_TOL = 1e-10

# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
# row-partitioned: (V, splits); a rank of one row first and last, slices of unequal length (a chunk's tail), splits off
# the 64-row grid, V one past a multiple of 128 / 256 / 1024 / 4096
ROW_CASES = (
    (129, (0, 64, 129)), (129, (0, 1, 129)), (129, (0, 128, 129)),
    (257, (0, 64, 192, 257)),
    (700, (0, 333, 700)), (700, (0, 100, 290, 700)), (700, (0, 64, 65, 640, 700)),
    (1025, tuple(row_splits(1025, 4))),
)
# ... and where a rank may stream the image of its rows (V >= 4096, b = 4): once on W, once on the image
IMAGE_CASES = ((4096, (0, 2048, 4096)), (4097, (0, 4096, 4097)), (4225, tuple(row_splits(4225, 3))))
# upper triangle: every split but the last a multiple of 256
UPPER_CASES = tuple((n, tuple(row_splits_upper(n, w))) for n, w in
                    ((513, 2), (769, 3), (1025, 4), (1300, 4), (2049, 2), (2049, 3), (4097, 2))) + (
    (1025, (0, 1024, 1025)), (1300, (0, 256, 1300)))


def case_id(case) -> str:
    return f"{case[0]}-" + "_".join(str(s) for s in case[1])


def check_splits(n: int, splits, upper: bool = False) -> None:
    s = np.asarray(splits, dtype=np.int64)
    assert s[0] == 0 and s[-1] == n and (np.diff(s) > 0).all(), splits
    if upper:
        assert (s[:-1] % TW == 0).all(), splits


# ---------------------------------------------------------------------------------------------------------------
# forests
# ---------------------------------------------------------------------------------------------------------------
def with_lone(arrays: TreeArrays, lone) -> TreeArrays:
    """``arrays`` on ``n_taxa + len(lone)`` taxa: the ids in ``lone`` are in no tree (degree exactly 0), the others
    keep their order."""
    lone = np.unique(np.asarray(lone, dtype=np.int64))
    n = arrays.n_taxa + len(lone)
    assert len(lone) and lone.min() >= 0 and lone.max() < n
    keep = np.setdiff1d(np.arange(n, dtype=np.int64), lone)
    taxon = np.where(arrays.taxon >= 0, keep[np.maximum(arrays.taxon, 0)], arrays.taxon).astype(np.int32)
    return TreeArrays(n_taxa=n, node_off=arrays.node_off, parent=arrays.parent, taxon=taxon, length=arrays.length,
                      support=arrays.support, weights=arrays.weights, taxa=br.taxon_names(n))


def lone_rows(splits) -> list[int]:
    """The last row of rank 0 and the first of rank 1: lone vertices on both sides of a rank boundary."""
    return [int(splits[1]) - 1, int(splits[1])]


def apply_forest(n: int, lone=()) -> TreeArrays:
    """``build_reference.size_forest`` with positive lengths (every degree of a taxon in a tree is positive: the
    operator's scaling is real), on ``n`` taxa of which ``lone`` are in no tree."""
    if not len(lone):
        return br.size_forest(n, "branch")
    return with_lone(br.size_forest(n - len(set(lone)), "branch"), lone)


def degree_forest(n: int, lone=()) -> TreeArrays:
    """``build_reference.degree_forest`` (signed rows, its own lone taxon) with ``lone`` on top."""
    if not len(lone):
        return br.degree_forest(n)[0]
    return with_lone(br.degree_forest(n - len(set(lone)))[0], lone)


# ---------------------------------------------------------------------------------------------------------------
# the upper-triangle job
# ---------------------------------------------------------------------------------------------------------------
def upper_cells(n: int, splits, rank: int):
    """``(stored, transposed)``, boolean (rows of the rank) x V: the cells of W the rank stores -- row i from column
    ``i // 256 * 256`` on -- every one of which it applies directly (y_i += w_ic z_c), and those right of the row's
    256-column diagonal tile, which it applies transposed as well (y_c += w_ic z_i)."""
    check_splits(n, splits, upper=True)
    rows = np.arange(splits[rank], splits[rank + 1], dtype=np.int64)[:, None]
    cols = np.arange(n, dtype=np.int64)[None, :]
    return cols >= rows // TW * TW, cols >= (rows // TW + 1) * TW


def upper_partial(w: np.ndarray, splits, rank: int, z: np.ndarray):
    """``(ref, mag)`` of the rank's unscaled partial product for all V rows: ``w`` the whole symmetric W, ``z`` the
    scaled operand (V x b, longdouble); ``mag`` the same sums over absolute values (for the budget)."""
    sr.require_extended_precision()
    n = w.shape[0]
    assert w.shape == (n, n) and z.shape[0] == n
    lo, hi = int(splits[rank]), int(splits[rank + 1])
    stored, transposed = upper_cells(n, splits, rank)
    z = z.astype(LD)
    both = np.concatenate([z, np.abs(z)], axis=1)
    b = z.shape[1]
    out = np.zeros((n, 2 * b), dtype=LD)
    block = w[lo:hi].astype(LD)
    assert (w[lo:hi] >= 0).all(), "mag is taken from one product: W must not be negative here"
    out[lo:hi] += np.where(stored, block, LD(0)) @ both
    out += (both[lo:hi].T @ np.where(transposed, block, LD(0))).T
    return out[:, :b], out[:, b:]


def upper_tiles(n: int, splits, rank: int) -> int:
    """Tiles (128 rows x 256 columns) the rank streams per application: for each of its 128-row blocks the tiles from
    the one that holds the block's diagonal to the last column tile."""
    n_ct = (n + TW - 1) // TW
    lo, hi = int(splits[rank]) // 128, (int(splits[rank + 1]) + 127) // 128
    return sum(n_ct - i * 128 // TW for i in range(lo, hi))


def upper_degree_part(w: np.ndarray, splits, rank: int) -> np.ndarray:
    """The rank's V-long contribution to the degrees: for its own rows the row sum from the diagonal tile on, plus for
    every column the sum over those of its rows that lie in earlier 256-row blocks (``k_degrees_upper_rows`` /
    ``k_degrees_upper_cols``).  In the dtype of ``w`` for integers (exact), else longdouble."""
    n = w.shape[0]
    lo, hi = int(splits[rank]), int(splits[rank + 1])
    stored, transposed = upper_cells(n, splits, rank)
    block = w[lo:hi] if np.issubdtype(w.dtype, np.integer) else w[lo:hi].astype(LD)
    zero = block.dtype.type(0)
    out = np.zeros(n, dtype=block.dtype)
    out[lo:hi] = np.where(stored, block, zero).sum(axis=1)
    out += np.where(transposed, block, zero).sum(axis=0)
    return out


# ---------------------------------------------------------------------------------------------------------------
# the row-partitioned job's receive buffer
# ---------------------------------------------------------------------------------------------------------------
def chunk_of(splits, b: int) -> int:
    return int(np.diff(np.asarray(splits)).max()) * b


def unpack_index(n: int, splits, b: int) -> np.ndarray:
    """For every entry (i, k) of the V x b block its place in the receive buffer: rank r's chunk starts at
    ``r * chunk`` and holds its rows from ``splits[r]`` on."""
    check_splits(n, splits)
    s = np.asarray(splits, dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    r = np.searchsorted(s, i, side="right") - 1
    return (r * chunk_of(splits, b) + (i - s[r]) * b)[:, None] + np.arange(b, dtype=np.int64)[None, :]


def slices(y_full: np.ndarray, splits, b: int, mark=np.nan) -> np.ndarray:
    """The receive buffer (world x chunk) that holds ``y_full`` (V x b): the tail of a short slice is ``mark``."""
    n = y_full.shape[0]
    assert y_full.shape == (n, b)
    world = len(splits) - 1
    buf = np.full(world * chunk_of(splits, b), mark, dtype=y_full.dtype)
    buf[unpack_index(n, splits, b)] = y_full
    return buf.reshape(world, -1)


def unpack(buf: np.ndarray, n: int, splits, b: int) -> np.ndarray:
    return buf.reshape(-1)[unpack_index(n, splits, b)]


# ---------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------
def panels(n: int, b: int, seed: int, graded: bool = False):
    """``(q, aq)``, V x 3b: the R block of ``q`` is ``solver_reference.apply_vectors``; the X and P blocks of both are
    random; the R slot of ``aq`` is NaN (the path under test writes it before anybody reads it)."""
    rs = np.random.RandomState(seed + 31 * b)
    q = rs.standard_normal((n, 3 * b))
    q[:, 2 * b:] = sr.apply_vectors(n, b, seed, graded)
    aq = rs.standard_normal((n, 3 * b)) + 0.25
    aq[:, 2 * b:] = np.nan
    return q, aq


def qaq_reference(q: np.ndarray, aq: np.ndarray, y: np.ndarray):
    """``(ref, budget)`` of Q^T AQ with the RETURNED R slot ``y`` in AQ: the Gram kernel is held to the block it
    assembled, the operator is not tested twice."""
    b = y.shape[1]
    full = aq.copy()
    full[:, 2 * b:] = y
    return sr.gram_reference(q, full)
