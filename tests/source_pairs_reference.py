"""Host references of the pairwise source-tree distances (helper module, not collected).

For a row tree A and a column tree B, with L = L(A) ∩ L(B), c = |L| and C(X|L) the distinct sets cl(v) ∩ L of
2 <= size < c over the nodes v of X: ``common`` = c, ``clusters`` = |C(A|L)|, ``clusters_other`` = |C(B|L)|,
``shared`` = |C(A|L) ∩ C(B|L)|; c < 3 gives zeros beside ``common``.

* ``by_sets``: the definitions over Python sets, on nested-list trees (``parsimony_reference`` builds them);
* ``linear``: per pair on the flattened tables -- the restricted depth tables of both trees (a segmented minimum of
  the adjacent-LCA depths), their nodes by one stack pass each, and Day's test: a cluster of A|L is one of B|L iff its
  leaves' ranks in B|L are consecutive (max - min = size - 1) and that interval is a node of B|L.  No dense rows, no
  stretches, no bitsets: another algorithm than the kernel's, and fast enough for one pair of 70 000 leaves;
* ``plan``: the export's plan restated (``scs_debug_source_pairs_plan``).
"""

from __future__ import annotations

import numpy as np
import parsimony_reference as pr
from score_reference import _clusters

KEYS = ("common", "clusters", "clusters_other", "shared")

SC_BUDGET = 3 << 29
TP_LDS_MAX = 160 << 10
SP_SLAB_WGS = 256
SP_SLAB_BYTES = 128 << 20
SP_SCRATCH = 128


# ------------------------------------------------------------------------------------------------ by sets
def _restricted_clusters(tree, common: frozenset) -> set:
    c = len(common)
    return {s for s in (cl & common for cl in pr.clusters(tree)) if 2 <= len(s) < c}


def pair_by_sets(tree_a, tree_b) -> tuple[int, int, int, int]:
    common = frozenset(pr.leaves_of(tree_a)) & frozenset(pr.leaves_of(tree_b))
    if len(common) < 3:
        return len(common), 0, 0, 0
    ca, cb = _restricted_clusters(tree_a, common), _restricted_clusters(tree_b, common)
    return len(common), len(ca), len(cb), len(ca & cb)


def _matrix(trees, rows, pair) -> dict:
    rows = list(range(len(trees))) if rows is None else [int(r) for r in rows]
    out = {k: np.zeros((len(rows), len(trees)), dtype=np.int32) for k in KEYS}
    for i, r in enumerate(rows):
        for j in range(len(trees)):
            for k, v in zip(KEYS, pair(r, j)):
                out[k][i, j] = v
    return out


def by_sets(trees, rows=None) -> dict:
    """The four matrices (rows x trees, int32) of nested-list trees, straight from the definitions."""
    return _matrix(trees, rows, lambda r, j: pair_by_sets(trees[r], trees[j]))


# ------------------------------------------------------------------------------------------------ linear
def _range_table(values: np.ndarray, op) -> list:
    levels = [values]
    while (1 << len(levels)) <= len(values):
        prev, h = levels[-1], 1 << (len(levels) - 1)
        cur = prev.copy()
        cur[: len(values) - h] = op(prev[: len(values) - h], prev[h:])
        levels.append(cur)
    return levels


def _range_query(levels: list, op, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    j = np.floor(np.log2(hi - lo + 1)).astype(np.int64)
    tab = np.stack(levels)
    return op(tab[j, lo], tab[j, hi - (1 << j) + 1])


def _restricted_depths(adj: np.ndarray, at: np.ndarray) -> np.ndarray:
    """Depth of the LCA of the leaves at positions ``at[k]`` and ``at[k + 1]`` (ascending) of a tree with the
    adjacent-LCA depths ``adj``: the minimum of adj over [at[k], at[k + 1])."""
    return np.minimum.reduceat(adj[: at[-1]], at[:-1])


def pair_linear(leaf_a, adj_a, leaf_b, adj_b, n_taxa: int) -> tuple[int, int, int, int]:
    pos_b = np.full(n_taxa, -1, dtype=np.int64)
    pos_b[leaf_b] = np.arange(len(leaf_b))
    in_b = pos_b[leaf_a]                      # B position of every A leaf, -1
    at_a = np.flatnonzero(in_b >= 0)          # A positions of the common leaves, A's order
    c = len(at_a)
    if c < 3:
        return c, 0, 0, 0
    bq = in_b[at_a]                           # their B positions
    at_b = np.sort(bq)                        # B positions, B's order
    rank_b = np.searchsorted(at_b, bq)        # rank in B|L of the k-th leaf of A|L
    nodes_a = [(lo, hi) for lo, hi, _ in _clusters(_restricted_depths(adj_a, at_a), c) if hi - lo + 1 < c]
    nodes_b = {(lo, hi) for lo, hi, _ in _clusters(_restricted_depths(adj_b, at_b), c) if hi - lo + 1 < c}
    shared = 0
    if nodes_a:
        lo = np.array([x[0] for x in nodes_a], dtype=np.int64)
        hi = np.array([x[1] for x in nodes_a], dtype=np.int64)
        mn = _range_query(_range_table(rank_b, np.minimum), np.minimum, lo, hi)
        mx = _range_query(_range_table(rank_b, np.maximum), np.maximum, lo, hi)
        for a, b, s in zip(mn.tolist(), mx.tolist(), (hi - lo).tolist()):
            shared += b - a == s and (a, b) in nodes_b
    return c, len(nodes_a), len(nodes_b), shared


def linear(tables, rows=None) -> dict:
    """The four matrices of flattened tables (``TreeTables``), one linear pass per pair."""
    off = np.asarray(tables.tree_off, dtype=np.int64)
    leaf = [np.asarray(tables.leaf_taxon[off[t]:off[t + 1]], dtype=np.int64) for t in range(len(off) - 1)]
    adj = [np.asarray(tables.adj_depth[off[t]:off[t + 1]], dtype=np.int64) for t in range(len(off) - 1)]
    return _matrix(leaf, rows, lambda r, j: pair_linear(leaf[r], adj[r], leaf[j], adj[j], int(tables.n_taxa)))


def check_invariants(got: dict, n_source=None) -> None:
    """What every full matrix (rows = all trees) satisfies: ``shared`` and ``common`` symmetric, ``clusters`` the
    transpose of ``clusters_other``, the diagonal a tree's own cluster count."""
    assert np.array_equal(got["shared"], got["shared"].T) and np.array_equal(got["common"], got["common"].T)
    assert np.array_equal(got["clusters"], got["clusters_other"].T)
    d = np.diagonal(got["clusters"])
    assert np.array_equal(d, np.diagonal(got["clusters_other"])) and np.array_equal(d, np.diagonal(got["shared"]))
    if n_source is not None:
        assert np.array_equal(d, np.asarray(n_source))


# ------------------------------------------------------------------------------------------------ the plan
def _levels(n: int) -> int:
    lev = 1
    while (1 << lev) <= n:
        lev += 1
    return lev


def pair_bytes(n_a: int, n_b: int, width: int) -> int:
    """Bytes of one pair's arrays: two bitsets with their prefixes, three lists of min(n_a, n_b) entries, and the min
    and max tables over blocks of 64 entries."""
    cm = min(n_a, n_b)
    nblk = (cm >> 6) + 1
    at = 8 * ((n_a >> 5) + 1) + 8 * ((n_b >> 5) + 1) + 3 * cm * width
    at = (at + 3) & ~3
    at += 2 * _levels(nblk) * nblk * width
    return (at + 15) & ~15


def plan(tree_off, n_taxa: int, n_rows: int, batch_trees: int = 0, lds_bytes: int = 0) -> dict:
    off = [int(x) for x in tree_off]
    m = len(off) - 1
    sizes = [off[t + 1] - off[t] for t in range(m)]
    largest = max(sizes, default=0)
    levels = _levels(max(largest, 1))
    row_stride = (max(n_taxa, 1) + 63) // 64 * 64
    cap = min(lds_bytes, TP_LDS_MAX) if lds_bytes > 0 else TP_LDS_MAX
    need = pair_bytes(largest, largest, 2 if largest < 65536 else 4)
    slab_stride = slab_wgs = 0
    if need + SP_SCRATCH > cap:
        slab_stride = (need + 255) // 256 * 256
        slab_wgs = min(SP_SLAB_WGS, max(1, SP_SLAB_BYTES // slab_stride))
    budget = max(SC_BUDGET - slab_stride * slab_wgs, 0)
    bstart, acc = [0], 0
    for t in range(m):
        nb = t - bstart[-1]
        per = row_stride * 4 + sizes[t] * 8 * (levels - 1)
        if nb > 0 and (acc + per > budget or (batch_trees > 0 and nb >= batch_trees)):
            bstart.append(t)
            acc = 0
        acc += per
    bstart.append(m)
    k = len(bstart) - 1
    big = [max(sizes[bstart[b]:bstart[b + 1]], default=0) for b in range(k)]
    max_lb = max(off[bstart[b + 1]] - off[bstart[b]] for b in range(k))
    max_nb = max(bstart[b + 1] - bstart[b] for b in range(k))
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    lev = max(levels - 1, 1)
    workspace = (up(4) + 2 * up(4 * n_rows) + up(16 * n_rows * m) + up(slab_stride * slab_wgs)
                 + up(4 * max_nb * row_stride) + 2 * up(4 * max_lb * lev))
    tiles = np.zeros((k, k, 7), dtype=np.int64)
    for i in range(k):
        for j in range(k):
            width = 2 if max(big[i], big[j]) < 65536 else 4
            need = pair_bytes(big[i], big[j], width) + SP_SCRATCH
            lds = max(min(need, cap), SP_SCRATCH)
            threads = 256  # more while the LDS leaves a CU room for fewer than 32 waves
            while threads < 1024 and (TP_LDS_MAX // lds) * (threads // 64) < 32:
                threads *= 2
            # a dispatch counts its work-items in 32 bits: that many workgroups a launch, 2^30 at most
            limit = min(1 << 30, ((1 << 32) - 1) // threads)
            tiles[i, j] = (width, lds, need > cap, need, threads, limit,
                           max(limit // max(bstart[j + 1] - bstart[j], 1), 1))
    return {"bstart": np.asarray(bstart, dtype=np.int64), "levels": levels, "row_stride": row_stride,
            "slab_stride": slab_stride, "slab_wgs": slab_wgs, "workspace": workspace, "lds_cap": cap,
            "width": tiles[:, :, 0].copy(), "lds": tiles[:, :, 1].copy(), "slab": tiles[:, :, 2].copy(),
            "need": tiles[:, :, 3].copy(), "threads": tiles[:, :, 4].copy(), "grid_limit": tiles[:, :, 5].copy(),
            "rows_per_launch": tiles[:, :, 6].copy()}
