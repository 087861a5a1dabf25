"""The argmin tables beside a tree's range-minimum tables (``csrc/scs_build.hip``: ``k_sparse_level``,
``k_sparse_levels_fused``, ``rmq_min_at``) restated in numpy, and the brute-force answers they are held to.  CPU only.

For every level k >= 1 the device keeps ``off[k][p]``, the offset of the LEFTMOST minimum inside the window
``[p, p + 2^k)``:  ``off[k][p] = half + off[k-1][p + half]  if  val[k-1][p + half] < val[k-1][p]  else  off[k-1][p]``
with ``half = 2^(k-1)`` and ``off[0] = 0`` (not stored).  A query over ``[a, b)`` reads ``x = val[k][a]`` and
``y = val[k][b - 2^k]`` for ``k = floor(log2(b - a))`` and answers ``b - 2^k + off[k][b - 2^k]`` when ``y < x``,
else ``a + off[k][a]``.  Both comparisons are strict, so ties go left; -0.0 and 0.0 tie.
"""

from __future__ import annotations

import numpy as np

ARGMIN_MAX_LEVEL = 16  # offsets are 16-bit: levels above keep the halving search (``halving_position``)


def levels_for(m: int) -> int:
    lv = 0
    while (1 << lv) <= m:
        lv += 1
    return lv


def build_tables(values: np.ndarray) -> tuple[list[np.ndarray], list[np.ndarray]]:
    """``(val, off)``: level k of each holds m - 2^k + 1 entries.  The value is picked as ``pick_smaller_value``
    picks it (``a if a < b else b``: the right one on a tie), the offset by the strict rule above."""
    v0 = np.asarray(values, dtype=np.float64)
    m = len(v0)
    val, off = [v0], [np.zeros(m, dtype=np.int64)]
    for k in range(1, levels_for(m)):
        half, cnt = 1 << (k - 1), m - (1 << k) + 1
        left, right = val[k - 1][:cnt], val[k - 1][half:half + cnt]
        val.append(np.where(left < right, left, right))
        off.append(np.where(right < left, half + off[k - 1][half:half + cnt], off[k - 1][:cnt]))
    return val, off


def query(val: list[np.ndarray], off: list[np.ndarray], a: int, b: int) -> tuple[float, int]:
    """``(minimum, position)`` over gaps [a, b), 0 <= a < b <= m, by the device's rule."""
    k = (b - a).bit_length() - 1
    x, y = val[k][a], val[k][b - (1 << k)]
    g = x if x < y else y
    if y < x:
        q = b - (1 << k)
        return g, q + int(off[k][q])
    return g, a + int(off[k][a])


def halving_position(val: list[np.ndarray], a: int, b: int) -> int:
    """The search the records ran before the table existed and still run from level 17 on: halve the range, keeping
    a half whose minimum still equals the range's (the left one when both do)."""

    def rmq(lo: int, hi: int) -> float:
        k = (hi - lo).bit_length() - 1
        x, y = val[k][lo], val[k][hi - (1 << k)]
        return x if x < y else y

    g = rmq(a, b)
    lo, hi = a, b
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if rmq(lo, mid) == g:
            hi = mid
        else:
            lo = mid
    return lo


def brute(values: np.ndarray, a: int, b: int) -> tuple[float, int]:
    """``(minimum, leftmost position)`` over [a, b): ``np.argmin`` returns the first of equal minima, and -0.0
    equals 0.0."""
    seg = np.asarray(values[a:b], dtype=np.float64)
    i = int(np.argmin(seg))
    return float(seg[i]), a + i


def gap_arrays(tb, t: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(leaf taxa, gap depths, gap values)`` of tree t of flattened tables: gap p lies between leaves p and p + 1;
    its value is ``adj_val * tree_w``, one rounded multiply, and 0.0 at depth 0 (``k_positions_values``)."""
    lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1])
    depth = np.asarray(tb.adj_depth[lo:hi - 1], dtype=np.int64)
    value = np.where(depth != 0, np.asarray(tb.adj_val[lo:hi - 1]) * float(tb.tree_w[t]), 0.0)
    return np.asarray(tb.leaf_taxon[lo:hi]), depth, value


def record_reference(tb, t: int, row_lo: int, row_hi: int, by_depth: bool) -> dict:
    """The record of the rows [row_lo, row_hi) (one 64-row block, or its part inside the row range) in tree t by brute
    force: ``spos`` the sorted positions of the rows the tree holds, and for neighbours k, k + 1 the minimum over the
    gaps [spos[k], spos[k + 1]) -- of the values (monotone kernels), or of the depths (general kernel: ``gap`` is then
    the value AT that position) -- with ``argpos`` its LEFTMOST position."""
    taxa, depth, value = gap_arrays(tb, t)
    spos = np.flatnonzero((taxa >= row_lo) & (taxa < row_hi))
    key = depth if by_depth else value
    at = np.asarray([int(spos[k]) + int(np.argmin(key[spos[k]:spos[k + 1]])) for k in range(len(spos) - 1)],
                    dtype=np.int64)
    return {"spos": spos, "argpos": at, "gap": value[at], "depth": depth[at], "cnt": len(spos)}


# ---- value patterns of the CPU test
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000)


def pairs_for(m: int, rng: np.random.RandomState) -> list[tuple[int, int]]:
    """All (a, b) up to 65 gaps, 4 000 random pairs above."""
    if m <= 65:
        return [(a, b) for a in range(m) for b in range(a + 1, m + 1)]
    a = rng.randint(0, m, size=4000)
    b = np.minimum(m, a + 1 + rng.randint(0, m, size=4000))
    return list(zip(a.tolist(), b.tolist()))


def value_patterns(m: int, rng: np.random.RandomState) -> dict[str, np.ndarray]:
    out = {"random": rng.random_sample(m) + 0.5, "few_values": rng.randint(0, 3, size=m).astype(np.float64),
           "all_equal": np.full(m, 0.75), "signed_zeros": np.where(rng.randint(0, 2, size=m) == 1, 0.0, -0.0),
           "zeros_among": np.where(rng.randint(0, 3, size=m) == 0, rng.choice([0.0, -0.0], size=m), 1.0)}
    # two equal minima on both sides of every window boundary: positions c - 1 and c for every power of two c, and
    # for every c that ends a window starting at a power of two
    cuts = sorted({c for k in range(0, 11) for c in ((1 << k), m - (1 << k), (1 << k) + (1 << max(k - 1, 0)))
                   if 1 <= c < m})
    for i, c in enumerate(cuts):
        v = rng.random_sample(m) + 1.0
        v[c - 1] = v[c] = 0.25
        out[f"twin_minima_at_{c}"] = v
        if i % 2 == 0 and c + 1 < m:  # and one twin pair that straddles the cut by one more position
            w = v.copy()
            w[c] = 1.5
            w[c + 1] = 0.25
            out[f"twin_minima_around_{c}"] = w
    return out
