"""Host references of the pairwise rooted-triplet terms of the sources (helper module, not collected).

For a row tree A and a column tree B, with L = L(A) ∩ L(B) and c = |L|, a triple {a, b, d} of L is resolved ab|d in a
tree when one of its clusters holds a and b but not d: ``common`` = c, ``triplets`` / ``triplets_other`` = the triples
A / B resolves, ``triplets_shared`` = those both resolve the same way; c < 3 gives zeros beside ``common``.

* ``pair_by_sets``: every triple of L, decided from the trees' clusters as Python sets (c up to about 25);
* ``pair_quadratic``: the node-pair formula of DESIGN.md section 15 on the restricted trees, whose clusters are taken
  as sets of sets -- the distinct cl(v) ∩ L, the parent of one the smallest other that holds it -- and whose
  intersection sizes are one matrix product.  No leaf order, no gap depths, no bitset rows: another construction than
  the kernel's;
* ``plan``: the export's plan restated (``scs_debug_source_pair_triplets_plan``).
"""

from __future__ import annotations

from itertools import combinations

import numpy as np
import parsimony_reference as pr
import source_pairs_reference as sp
from score_reference import _clusters

KEYS = ("common", "triplets", "triplets_other", "triplets_shared")

TP_LDS_MAX = 160 << 10
TP_LDS_BUDGET = 40 << 10
ST_ZMAX = 32
ST_SMALL_C = 64
ST_SCRATCH = 128 + 4 * ST_SMALL_C * 8 + 4 * ST_SMALL_C
ST_HEADER = 32
ST_CHUNK_BYTES = 512 << 20
ST_ROW_MAX = TP_LDS_MAX // 16 * 32 - 1
GRID_LIMIT = min(1 << 30, ((1 << 32) - 1) // 256)


# ------------------------------------------------------------------------------------------------ by sets
def _resolution(triple, clusters):
    """The pair of ``triple`` a cluster holds without the third, None for a fan."""
    for cl in clusters:
        inside = [x for x in triple if x in cl]
        if len(inside) == 2:
            return frozenset(inside)
    return None


def pair_by_sets(tree_a, tree_b) -> tuple[int, int, int, int]:
    common = sorted(set(pr.leaves_of(tree_a)) & set(pr.leaves_of(tree_b)))
    ca = [cl for cl in pr.clusters(tree_a) if len(cl) >= 2]
    cb = [cl for cl in pr.clusters(tree_b) if len(cl) >= 2]
    t_a = t_b = t_s = 0
    for triple in combinations(common, 3):
        ra, rb = _resolution(triple, ca), _resolution(triple, cb)
        t_a += ra is not None
        t_b += rb is not None
        t_s += ra is not None and ra == rb
    return len(common), t_a, t_b, t_s


# ------------------------------------------------------------------------------------------------ node pairs
def _restricted_family(clusters, index: dict) -> tuple[np.ndarray, np.ndarray]:
    """The distinct sets cl ∩ L of 2 <= size < |L| over a tree's ``clusters`` as 0/1 rows over L (``index``: taxon ->
    column) and, row for row, the smallest set of the family (L included) that strictly holds each."""
    c = len(index)
    full = frozenset(index)
    family = {s for s in (cl & full for cl in clusters) if len(s) >= 2}
    family.add(full)
    masks = sorted(((len(s), sum(1 << index[x] for x in s)) for s in family))
    own, parent = [], []
    for i, (size, m) in enumerate(masks):
        if size == c:
            continue
        up = next(pm for _, pm in masks[i + 1:] if pm & m == m and pm != m)
        own.append(m)
        parent.append(up)

    def rows(ms):
        out = np.zeros((len(ms), c), dtype=np.float32)
        for r, m in enumerate(ms):
            bits = np.frombuffer(m.to_bytes((c + 7) // 8, "little"), dtype=np.uint8)
            out[r] = np.unpackbits(bits, bitorder="little")[:c]
        return out

    return rows(own), rows(parent)


def pair_quadratic(tree_a, tree_b) -> tuple[int, int, int, int]:
    return _quadratic(pr.leaves_of(tree_a), pr.clusters(tree_a), pr.leaves_of(tree_b), pr.clusters(tree_b))


def pair_quadratic_tables(leaf_a, adj_a, leaf_b, adj_b) -> tuple[int, int, int, int]:
    """``pair_quadratic`` for two trees of flattened tables: the leaves in order and the adjacent-LCA depths."""
    def clusters(leaf, adj):
        return {frozenset(leaf[lo:hi + 1]) for lo, hi, _ in _clusters(adj, len(leaf))}

    leaf_a, leaf_b = [int(x) for x in leaf_a], [int(x) for x in leaf_b]
    return _quadratic(leaf_a, clusters(leaf_a, adj_a), leaf_b, clusters(leaf_b, adj_b))


def _quadratic(leaves_a, clusters_a, leaves_b, clusters_b, block: int = 1024) -> tuple[int, int, int, int]:
    common = sorted(set(leaves_a) & set(leaves_b))
    c = len(common)
    if c < 3:
        return c, 0, 0, 0
    assert c < (1 << 24)  # (the products below are sums of at most c ones: exact in float32)
    index = {x: i for i, x in enumerate(common)}
    y, py = _restricted_family(clusters_a, index)
    z, pz = _restricted_family(clusters_b, index)

    def resolved(own, parent):
        s, p = own.sum(axis=1).astype(np.int64), parent.sum(axis=1).astype(np.int64)
        return int((s * (s - 1) // 2 * (p - s)).sum())

    shared, nz = 0, len(z)
    both = np.concatenate([z, pz]).T
    for at in range(0, len(y) if nz else 0, block):  # (blocks of A's sets: the products of a large pair stay small)
        ny = len(y[at:at + block])
        inter = (np.concatenate([y[at:at + block], py[at:at + block]]) @ both).astype(np.int64)
        iyz, iypz, ipyz, ipp = inter[:ny, :nz], inter[:ny, nz:], inter[ny:, :nz], inter[ny:, nz:]
        shared += int((iyz * (iyz - 1) // 2 * (ipp - iypz - ipyz + iyz)).sum())
    return c, resolved(y, py), resolved(z, pz), shared


def _matrix(trees, rows, pair) -> dict:
    rows = list(range(len(trees))) if rows is None else [int(r) for r in rows]
    out = {k: np.zeros((len(rows), len(trees)), dtype=np.int32 if k == "common" else np.int64) for k in KEYS}
    memo: dict = {}
    for i, r in enumerate(rows):
        for j in range(len(trees)):
            if (j, r) in memo:  # (the cell (B, A) is the cell (A, B) with the two trees' counts swapped)
                c, a, b, s = memo[(j, r)]
                vals = (c, b, a, s)
            else:
                vals = memo[(r, j)] = pair(trees[r], trees[j])
            for k, v in zip(KEYS, vals):
                out[k][i, j] = v
    return out


def by_sets(trees, rows=None) -> dict:
    return _matrix(trees, rows, pair_by_sets)


def quadratic(trees, rows=None) -> dict:
    return _matrix(trees, rows, pair_quadratic)


def check_invariants(got: dict) -> None:
    """What every full matrix (rows = all trees) satisfies."""
    assert np.array_equal(got["triplets_shared"], got["triplets_shared"].T)
    assert np.array_equal(got["common"], got["common"].T)
    assert np.array_equal(got["triplets"], got["triplets_other"].T)
    d = np.diagonal(got["triplets"])
    assert np.array_equal(d, np.diagonal(got["triplets_other"]))
    assert np.array_equal(d, np.diagonal(got["triplets_shared"]))


# ------------------------------------------------------------------------------------------------ the plan
def _up(n: int, m: int = 256) -> int:
    return (n + m - 1) // m * m


def work_bytes(n_a: int, n_b: int) -> int:
    """The arrays of one pair's restriction: two bitsets with their prefix counts, two lists of positions."""
    return 8 * ((n_a >> 5) + 1 + (n_b >> 5) + 1) + 8 * min(n_a, n_b)


def region_bytes(n_a: int, n_b: int) -> int:
    """A pair's region for a tile whose row / column trees have at most n_a / n_b leaves: header, two node lists of 16
    bytes an entry, the B rank -> A rank list, the restriction's arrays."""
    cm = min(n_a, n_b)
    return _up(((ST_HEADER + 36 * cm + 15) & ~15) + work_bytes(n_a, n_b))


def pair_blocks(n_a: int, n_b: int, zb: int) -> int:
    cm = min(n_a, n_b)
    return 0 if cm <= ST_SMALL_C else (cm - 2 + zb - 1) // zb


def plan(tree_off, n_taxa: int, rows=None, batch_trees: int = 0, lds_bytes: int = 0, chunk_pairs: int = 0) -> dict:
    off = [int(x) for x in tree_off]
    m = len(off) - 1
    sizes = [off[t + 1] - off[t] for t in range(m)]
    mirror = rows is None
    rows = list(range(m)) if rows is None else [int(r) for r in rows]
    base = sp.plan(off, n_taxa, len(rows), batch_trees, 0)  # (section 33's batches, without an LDS cap)
    bstart = base["bstart"].tolist()
    k = len(bstart) - 1
    cap = min(lds_bytes, TP_LDS_MAX) if lds_bytes > 0 else TP_LDS_MAX
    batch_of = [b for b in range(k) for _ in range(bstart[b + 1] - bstart[b])]
    by_batch = [[r for r in rows if batch_of[r] == b] for b in range(k)]
    names = ("tile_rows", "max_common", "words", "zb", "lds_pairs", "lds_restrict", "slab", "need", "pair_bytes",
             "chunk_cap", "pairs", "n_chunks")
    tiles = np.zeros((k, k, 12), dtype=np.int64)
    chunks, max_chunk, region = [], 0, 0
    for i in range(k):
        if not by_batch[i]:
            continue
        na = max(sizes[r] for r in by_batch[i])
        for j in range(i if mirror else 0, k):
            cols = list(range(bstart[j], bstart[j + 1]))
            nb = max(sizes[t] for t in cols)
            cm = min(na, nb)
            words = (min(cm, ST_ROW_MAX) >> 5) + 1
            rowb = 16 * words
            if cm > ST_ROW_MAX:
                msg = (f"trees of {na} and {nb} leaves may share more than the {ST_ROW_MAX} taxa a bitset row holds "
                       "in LDS")
                raise ValueError(msg)
            if rowb > cap:
                msg = f"max_lds_bytes = {lds_bytes} does not hold the bitset rows of trees of {na} and {nb} leaves"
                raise ValueError(msg)
            zb = min(ST_ZMAX, max(1, min(TP_LDS_BUDGET, cap) // rowb))
            need = work_bytes(na, nb) + ST_SCRATCH
            stride = region_bytes(na, nb)
            pairs = len(by_batch[i]) * len(cols)
            chunk_cap = max(1, ST_CHUNK_BYTES // stride)
            if chunk_pairs > 0:
                chunk_cap = min(chunk_cap, chunk_pairs)
            chunk_cap = min(chunk_cap, pairs, GRID_LIMIT)
            max_chunk = max(max_chunk, chunk_cap)
            region = max(region, chunk_cap * stride)
            mine = 0
            cur = None
            for idx in range(pairs):
                a, b = by_batch[i][idx // len(cols)], cols[idx % len(cols)]
                skip = mirror and a > b
                blocks = 0 if skip else pair_blocks(sizes[a], sizes[b], zb)
                if cur is None or cur[3] == chunk_cap or cur[6] + blocks > GRID_LIMIT:
                    cur = [i, j, idx, 0, 0, 0, 0, 0]
                    chunks.append(cur)
                    mine += 1
                cur[3] += 1
                cur[4] += (not skip) and min(sizes[a], sizes[b]) <= ST_SMALL_C
                cur[5] += skip
                cur[6] += blocks
                cur[7] = idx // len(cols) - cur[2] // len(cols) + 1
            tiles[i, j] = (len(by_batch[i]), cm, words, zb, max(zb * rowb, 32), max(min(need, cap), ST_SCRATCH),
                           need > cap, need, stride, chunk_cap, pairs, mine)
    lev = max(base["levels"] - 1, 1)
    max_lb = max(off[bstart[b + 1]] - off[bstart[b]] for b in range(k))
    max_nb = max(bstart[b + 1] - bstart[b] for b in range(k))
    cells = len(rows) * m
    workspace = (_up(4) + 2 * _up(4 * len(rows)) + _up(4 * cells) + _up(24 * cells)
                 + _up(4 * max_nb * base["row_stride"]) + 2 * _up(4 * max_lb * lev) + _up(8 * (max_chunk + 1))
                 + _up(region))
    return {"bstart": np.asarray(bstart, dtype=np.int64), "levels": base["levels"], "row_stride": base["row_stride"],
            "lds_cap": cap, "small_common": ST_SMALL_C, "workspace": workspace, "region_bytes": region,
            "grid_limit": GRID_LIMIT, **{name: tiles[:, :, i].copy() for i, name in enumerate(names)},
            "chunks": np.asarray(chunks, dtype=np.int64).reshape(-1, 8)}
