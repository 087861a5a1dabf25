"""Builders and plain references for the edges of the cluster-graph build, the degrees, the single-precision image
and the contraction (``csrc/scs_build.hip`` with ``scs_mono.h``, ``scs_mono_wide.h``, ``scs_gen.h``; the cases of
``tests/test_gpu_build_edges.py``, held to their numbers by ``tests/test_build_reference_cpu.py``).  CPU only.

The reference for W itself stays ``oracle.tables_oracle.pcg_dense`` / ``pcg_rows``, the C restatement of the
reference's accumulation (src/sc_supertree/scs.py:495-663); nothing here restates it.  What is here:

* forests of a stated shape written as preorder node arrays -> ``TreeArrays`` -> ``flatten`` (no tree objects: a
  tree of 32 769 leaves takes a fraction of a second): random binary trees of exactly k leaves on chosen taxa,
  caterpillars, stars, balanced trees, one- and two-leaf trees, and leaf orders that put a 64-row block of W
  consecutively, one row per 64 positions, or with exactly c of its rows present;
* the host plan of ``scs_pcg_build`` restated where a case sits on it: tiles, padding, table levels, the gates;
* ``degrees_reference``: row sums in ``np.longdouble`` and the rounding budget that holds for ANY summation order;
* ``image_reference``: ``float32(W)``, zero padding, and the mask of the columns the image defines;
* ``contract_reference``: a double loop over member pairs, independent of ``oracle.tables_oracle.contract_dense``.
"""

from __future__ import annotations

from collections.abc import Sequence

import numpy as np

from spectralclustersupertree_amd.treearrays import TreeArrays

LD = np.longdouble

# ---- the constants of csrc/scs_build.hip and csrc/scs_internal.h the cases are placed by
TR = 64  # SCS_TR: rows of W per tile, one block record per (row block, tree)
TCW = 256  # SCS_TCW / MONO_TCW: columns per column group = threads per workgroup
NPAD = 512  # SCS_NPAD: the position tables' row length rounds up to this
LD_ALIGN = 512  # SCS_LD_ALIGN: leading dimension of W and of the image
IMG_TILE = 512  # the image of row r is defined from column (r / 512) * 512 on (one device)
SPARSE_FUSED_MAX_LEAVES = 32768  # a batch whose largest tree is larger takes one launch per table level
FUSED_THREADS = 1024  # k_sparse_levels_fused strides a level by this
TREE_PAR_MAX_TILES = 24  # tree-parallel build: up to this many tiles ...
TREE_PAR_MIN_TREES = 128  # ... from this many trees
WIDE_MIN_TILES = 13  # producer / consumer kernel: from this many tiles ...
WIDE_MIN_TREES = 96  # ... and this many trees in the batch
XCD_MIN_TILES = 9  # the per-XCD tile order: more than 8 tiles
LIST_COVERAGE = 1.0 / 64.0  # per-tile tree lists: leaves / (trees * taxa) below this
SMALL_N_ONE_BATCH = 2048  # up to here one batch holds up to 4096 trees


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def ld_of(n: int) -> int:
    return round_up(n, LD_ALIGN)


def npad_of(n: int) -> int:
    return round_up(round_up(n, TCW), NPAD)


def levels_for(m: int) -> int:
    """Levels k of a tree's range-minimum table with 2^k <= m (m gaps = leaves - 1); the table holds levels * m
    entries, level k the minima over [p, p + 2^k) for p <= m - 2^k."""
    lv = 0
    while (1 << lv) <= m:
        lv += 1
    return lv


def tiles(n: int, row_begin: int = 0, row_end: int | None = None, upper: bool | None = None) -> list[tuple[int, int]]:
    """The (row block, column group) tiles of a build of rows [row_begin, row_end), in row-major order: all of them
    for a row range, for the whole matrix on one rank only those that reach right of the block's first row."""
    row_end = n if row_end is None else row_end
    upper = (row_begin == 0 and row_end == n) if upper is None else upper
    gb0 = row_begin // TR
    n_blocks = (row_end - row_begin + TR - 1) // TR
    n_cg = (n + TCW - 1) // TCW
    return [(b, c) for b in range(n_blocks) for c in range(n_cg) if not (upper and (c + 1) * TCW <= (gb0 + b) * TR)]


def plan(n: int, n_trees: int, n_leaves: int, monotone: bool, row_begin: int = 0, row_end: int | None = None) -> dict:
    """What ``scs_pcg_build`` decides for one rank with no switch set and tables that fit one batch (n <= 2048 and at
    most 4096 trees, or at most 256 trees of small tables): ``n_tiles``, ``tree_parallel``, ``wide`` (the batch runs the
    producer / consumer kernel), ``listed``, ``xcd_reorder``."""
    row_end = n if row_end is None else row_end
    sym = row_begin == 0 and row_end == n
    nt = len(tiles(n, row_begin, row_end))
    listed = monotone and nt > 0 and n_trees > 0 and n_leaves / (n_trees * max(n, 1)) < LIST_COVERAGE
    tree_par = sym and 0 < nt <= TREE_PAR_MAX_TILES and n_trees >= TREE_PAR_MIN_TREES and not listed
    wide = monotone and not tree_par and not listed and nt >= WIDE_MIN_TILES and n_trees >= WIDE_MIN_TREES
    return {"n_tiles": nt, "tree_parallel": tree_par, "wide": wide, "listed": listed, "xcd_reorder": nt >= XCD_MIN_TILES}


# ------------------------------------------------------------------------------------------------ tree shapes
def shape(kind: str, k: int, rng: np.random.RandomState | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``(parent, is_leaf)`` in preorder of a tree of ``k`` leaves: ``random`` (binary, random splits), ``balanced``
    (binary, halves), ``caterpillar`` (binary, the inner nodes one path; the leaves come deepest first), ``star``
    (one polytomy of k - 1 leaves under the root beside one more leaf: every gap but the last has depth 1).  k = 1 is the lone node (root and leaf at once), k = 2 the root with two leaves."""
    assert k >= 1 and kind in ("random", "balanced", "caterpillar", "star")
    if k == 1:
        return np.asarray([-1], dtype=np.int32), np.asarray([True])
    if kind == "star" and k >= 3:
        # the root holds one polytomy of k - 1 leaves and one more leaf: every gap but the last has depth 1
        return (np.concatenate([[-1, 0], np.ones(k - 1, dtype=np.int32), [0]]).astype(np.int32),
                np.concatenate([[False, False], np.ones(k, dtype=bool)]))
    if kind == "caterpillar":
        # nodes: inner 0, 2, 4, ... (a path), then the two deepest leaves; leaf 2i + 1 hangs off inner 2i afterwards
        # in preorder the first child (the path) comes first: inner nodes 0 .. k - 2, then the leaves deepest first
        inner = np.arange(k - 1, dtype=np.int32)
        par_inner = inner - 1  # root: -1
        # leaves in preorder: two under the deepest inner node, then one under each inner node going up
        par_leaves = np.concatenate([[k - 2], np.arange(k - 2, -1, -1)]).astype(np.int32)
        parent = np.concatenate([par_inner, par_leaves]).astype(np.int32)
        return parent, np.concatenate([np.zeros(k - 1, dtype=bool), np.ones(k, dtype=bool)])
    if kind == "star":
        kind = "balanced"  # (two leaves: the root and its two children)
    parent = np.empty(2 * k - 1, dtype=np.int32)
    leaf = np.zeros(2 * k - 1, dtype=bool)
    at = 0
    stack = [(k, -1)]
    while stack:
        n, p = stack.pop()
        parent[at] = p
        if n == 1:
            leaf[at] = True
        else:
            a = n // 2 if kind == "balanced" else int(rng.randint(1, n))
            stack.append((n - a, at))
            stack.append((a, at))
        at += 1
    assert at == 2 * k - 1
    return parent, leaf


def taxon_names(n_taxa: int) -> list[str]:
    return [f"t{i:06d}" for i in range(n_taxa)]


def forest(seed: int, n_taxa: int, trees: Sequence[tuple[str, Sequence[int]]], lengths: str = "positive",
           unit_weights: bool = False) -> TreeArrays:
    """One ``TreeArrays`` over ``n_taxa`` ids from ``(kind, leaves in DFS order)`` per tree.

    ``lengths``: ``positive`` inner lengths (the ``branch`` value is monotone), ``signed`` (a third of the inner
    lengths negative: ``branch`` then takes the general kernel, and W has negative entries), ``equal`` (every length
    1.0), ``zero`` (every inner length 0.0: all ``branch`` values tie at 0).  Inner nodes carry integer supports;
    the root has no length; every tree its own weight unless ``unit_weights``."""
    assert lengths in ("positive", "signed", "equal", "zero")
    rng = np.random.RandomState(seed)
    parents, taxa = [], []
    for kind, order in trees:
        order = np.asarray(order, dtype=np.int32)
        assert len(np.unique(order)) == len(order) and len(order) >= 1
        assert order.min() >= 0 and order.max() < n_taxa
        # (a ``(parent, is_leaf)`` pair in place of a kind: a shape made elsewhere, tests/matrix_free_reference.py)
        par, leaf = kind if isinstance(kind, tuple) else shape(kind, len(order), rng)
        assert int(np.count_nonzero(leaf)) == len(order)
        tax = np.full(len(par), -1, dtype=np.int32)
        tax[leaf] = order
        parents.append(par)
        taxa.append(tax)
    node_off = np.zeros(len(trees) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in parents], out=node_off[1:])
    parent = np.concatenate(parents).astype(np.int32)
    taxon = np.concatenate(taxa).astype(np.int32)
    total = len(parent)
    inner = taxon < 0
    if lengths == "equal":
        length = np.ones(total)
    elif lengths == "zero":
        length = np.where(inner, 0.0, 1.0)
    else:
        length = rng.exponential(0.1, total) + 1e-3
        if lengths == "signed":
            flip = inner & (rng.random_sample(total) < 1.0 / 3.0)
            length[flip] = -3.0 * length[flip]
    length[node_off[:-1]] = np.nan
    support = np.where(inner, rng.randint(50, 101, total).astype(np.float64), np.nan)
    m = len(trees)
    weights = np.ones(m) if unit_weights else rng.choice([1.0, 2.0, 0.5, 0.75], size=m) + rng.randint(0, 2, m) * rng.random_sample(m)
    return TreeArrays(n_taxa=n_taxa, node_off=node_off, parent=parent, taxon=taxon, length=length, support=support,
                      weights=weights.astype(np.float64), taxa=taxon_names(n_taxa))


def tables(arrays: TreeArrays, strategy: str, monotone: bool | None = None):
    """``arrays.flatten(strategy)``; ``monotone=False`` sends tables that are monotone to the general kernel."""
    tb = arrays.flatten(strategy)
    if monotone is not None:
        assert monotone is False or tb.monotone
        tb.monotone = monotone
    return tb


# ------------------------------------------------------------------------------------------------ leaf orders
def block_rows(n: int, b: int) -> np.ndarray:
    return np.arange(b * TR, min(n, (b + 1) * TR), dtype=np.int32)


def order_random(rng: np.random.RandomState, pool: Sequence[int], k: int | None = None) -> np.ndarray:
    """``k`` distinct ids of ``pool`` (default: all) in random order."""
    pool = np.asarray(pool, dtype=np.int32)
    return pool[rng.permutation(len(pool))[: len(pool) if k is None else k]]


def order_block_consecutive(rng: np.random.RandomState, n: int, b: int, others: int | None = None) -> np.ndarray:
    """All rows of block ``b`` next to each other in DFS order (shuffled among themselves), ``others`` ids from
    outside the block around them (default: all)."""
    rows = block_rows(n, b)
    rest = order_random(rng, np.setdiff1d(np.arange(n, dtype=np.int32), rows), others)
    cut = int(rng.randint(0, len(rest) + 1))
    return np.concatenate([rest[:cut], rows[rng.permutation(len(rows))], rest[cut:]]).astype(np.int32)


def order_block_spread(rng: np.random.RandomState, n: int, b: int) -> np.ndarray:
    """Row i of block ``b`` (shuffled) at DFS position 64 i, ids from outside the block in between and behind: needs
    n >= 63 * 64 + 64."""
    rows = block_rows(n, b)
    rows = rows[rng.permutation(len(rows))]
    rest = order_random(rng, np.setdiff1d(np.arange(n, dtype=np.int32), rows))
    total = (len(rows) - 1) * TR + 1
    assert len(rest) >= total - len(rows)
    out = np.empty(len(rows) + len(rest), dtype=np.int32)
    at = np.arange(len(rows)) * TR
    mask = np.ones(len(out), dtype=bool)
    mask[at] = False
    out[at] = rows
    out[mask] = rest
    return out


def order_block_count(rng: np.random.RandomState, n: int, b: int, c: int, others: int | None = None) -> np.ndarray:
    """Exactly ``c`` rows of block ``b`` and ``others`` ids from outside it (default: all), in random order."""
    rows = block_rows(n, b)
    assert 0 <= c <= len(rows)
    rest = order_random(rng, np.setdiff1d(np.arange(n, dtype=np.int32), rows), others)
    return order_random(rng, np.concatenate([rows[rng.permutation(len(rows))[:c]], rest]))


def block_counts(tb) -> np.ndarray:
    """``cnt[b][t]``: the rows of 64-row block b that tree t holds -- the record's count."""
    n_blocks = (tb.n_taxa + TR - 1) // TR
    out = np.zeros((n_blocks, tb.n_trees), dtype=np.int64)
    for t in range(tb.n_trees):
        lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1])
        out[:, t] = np.bincount(tb.leaf_taxon[lo:hi] // TR, minlength=n_blocks)
    return out


def block_positions(tb, b: int, t: int) -> np.ndarray:
    """Sorted DFS positions in tree t of the rows of block b."""
    lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1])
    return np.flatnonzero(tb.leaf_taxon[lo:hi] // TR == b)


def coverage(tb) -> float:
    return tb.n_leaves / (tb.n_trees * max(tb.n_taxa, 1))


# ------------------------------------------------------------------------------------------------ references
def _need_extended() -> None:
    assert np.finfo(LD).nmant >= 63, "np.longdouble has no 64-bit mantissa on this platform"


def degrees_reference(w: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Row sums of ``w`` (rows x n) in ``np.longdouble`` and the per-row budget (n + 2) 2^-53 sum_j |w_ij|: the
    gamma_n bound on a sum of n doubles in ANY order (n - 1 rounded adds, plus the final rounding of the reference
    to double and slack of one), so that no correct kernel can fail it."""
    _need_extended()
    n = w.shape[1]
    ref = w.astype(LD).sum(axis=1)
    budget = (n + 2) * 2.0 ** -53 * np.abs(w).astype(LD).sum(axis=1)
    return ref, budget


def image_reference(w: np.ndarray, ld: int, row_begin: int = 0, full: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """``(image, defined)`` of rows [row_begin, row_begin + rows) of W: ``float32(w)`` with zeros in the padding
    columns [n, ld), and the mask of what the image defines -- column c of global row r from (r // 512) * 512 on,
    the padding included, or every column when ``full`` (a row-partitioned rank)."""
    rows, n = w.shape
    assert ld >= n and ld % LD_ALIGN == 0
    img = np.zeros((rows, ld), dtype=np.float32)
    img[:, :n] = w.astype(np.float32)
    first = np.zeros(rows, dtype=np.int64) if full else (row_begin + np.arange(rows)) // IMG_TILE * IMG_TILE
    defined = np.arange(ld)[None, :] >= first[:, None]
    return img, defined


def contract_reference(w: np.ndarray, group_start: Sequence[int]) -> np.ndarray:
    """W'[g][h] = max over the member pairs of groups g and h, diagonal 0 (reference: scs.py:336-387), by a plain
    double loop over the pairs."""
    gs = [int(x) for x in group_start]
    ng = len(gs) - 1
    out = np.zeros((ng, ng))
    for g in range(ng):
        for h in range(ng):
            if g == h:
                continue
            best = None
            for r in range(gs[g], gs[g + 1]):
                for c in range(gs[h], gs[h + 1]):
                    v = float(w[r, c])
                    if best is None or v > best:
                        best = v
            out[g, h] = best
    return out


def signed_matrix(seed: int, n: int) -> np.ndarray:
    """A symmetric matrix of signed doubles with zero diagonal: what a contraction case takes as W when the point
    is the kernel's maximum, not the build."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, n))
    a = np.triu(a, 1)
    return a + a.T


# ------------------------------------------------------------------------------------------------ the cases
# (shared by tests/test_gpu_build_edges.py, which runs them, and tests/test_build_reference_cpu.py, which holds
# every forest to the numbers it is named for)
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 511, 512, 513, 1023, 1024, 1025)
PATH_SIZES = (64, 65, 256, 257, 512, 513, 1025)
WEIGHTINGS = ("one", "branch", "bootstrap", "signed")  # signed: `branch` on negative lengths (the general kernel)
LEVEL_GAPS = (1, 2, 3, 4, 1023, 1024, 1025, 2047, 2048, 2049)
DEGREE_SIZES = (1, 2, 3, 127, 128, 129, 255, 257, 513)
IMAGE_SIZES = (511, 512, 513, 1023, 1024, 1025, 1537)
RECORD_COUNTS = (0, 1, 2, 63, 64)
RECORD_N, RECORD_BLOCK = 320, 2  # five row blocks, the middle one the block under test
SPREAD_N, SPREAD_BLOCK = 4160, 3  # 65 row blocks: room for one row per 64 positions
BIG_TAXA = 32800


def weighting(name: str) -> tuple[str, str]:
    """``(strategy, lengths)`` of a case's weighting name."""
    return ("branch", "signed") if name == "signed" else (name, "positive")


def size_forest(n: int, name: str = "branch", seed: int = 0) -> TreeArrays:
    """A handful of trees on ``n`` taxa, full and partial coverage, every shape: all taxa at random, half of them
    balanced, up to 37 as a caterpillar, all but one at random, up to 70 as a star."""
    rng = np.random.RandomState(1000 * seed + n)
    ids = np.arange(n, dtype=np.int32)
    trees = [("random", order_random(rng, ids)), ("balanced", order_random(rng, ids, max(1, n // 2))),
             ("caterpillar", order_random(rng, ids, min(n, 37))), ("random", order_random(rng, ids, max(1, n - 1))),
             ("star", order_random(rng, ids, min(n, 70)))]
    return forest(n + 7 * seed, n, trees, lengths=weighting(name)[1])


def size_ranges(n: int) -> list[tuple[int, int]]:
    """Row ranges that start and end inside a block and on a block edge."""
    want = [(0, 64), (64, n), (37, 101), (n - 1, n), (0, n - 1), (64, 128), (100, 257)]
    return [(a, b) for a, b in want if 0 <= a < b <= n]


def record_forest(kind: str, lengths: str = "positive", seed: int = 3) -> TreeArrays:
    """RECORD_N taxa; block RECORD_BLOCK holds 0, 1, 2, 63, 64 rows in trees 0 .. 4 (all other blocks full), all of
    them consecutive in DFS order in tree 5, all of them with few other taxa in tree 6."""
    rng = np.random.RandomState(seed)
    trees = [(kind, order_block_count(rng, RECORD_N, RECORD_BLOCK, c)) for c in RECORD_COUNTS]
    trees.append((kind, order_block_consecutive(rng, RECORD_N, RECORD_BLOCK)))
    trees.append((kind, order_block_consecutive(rng, RECORD_N, RECORD_BLOCK, others=40)))
    return forest(seed, RECORD_N, trees, lengths=lengths)


def spread_forest(lengths: str = "positive", seed: int = 4) -> TreeArrays:
    """SPREAD_N taxa; the rows of block SPREAD_BLOCK sit at DFS positions 0, 64, ..., 4032 of every tree: a random
    tree, a balanced tree and a caterpillar."""
    rng = np.random.RandomState(seed)
    trees = [(kind, order_block_spread(rng, SPREAD_N, SPREAD_BLOCK)) for kind in ("random", "balanced", "caterpillar")]
    return forest(seed, SPREAD_N, trees, lengths=lengths)


def tie_forest(n: int, lengths: str, seed: int = 5) -> TreeArrays:
    """Caterpillars and stars, whole and partial: with `one`, equal or zero lengths every gap of a star ties, and
    every gap of a caterpillar under `one`."""
    rng = np.random.RandomState(seed + n)
    ids = np.arange(n, dtype=np.int32)
    trees = [("caterpillar", order_random(rng, ids)), ("star", order_random(rng, ids)),
             ("caterpillar", order_random(rng, ids, n // 2)), ("star", order_random(rng, ids, n - 3)),
             ("balanced", order_random(rng, ids))]
    return forest(seed, n, trees, lengths=lengths)


GAPLESS_N = 70


def gapless_forest(which: str, seed: int = 6) -> TreeArrays:
    """GAPLESS_N taxa: ``ones`` five one-leaf trees, ``twos`` five two-leaf trees, ``first`` / ``last`` a one-leaf
    tree in front of / behind four ordinary trees, ``mixed`` one- and two-leaf trees between ordinary ones."""
    rng = np.random.RandomState(seed)
    ids = np.arange(GAPLESS_N, dtype=np.int32)
    one = lambda: ("random", order_random(rng, ids, 1))  # noqa: E731
    two = lambda: ("random", order_random(rng, ids, 2))  # noqa: E731
    full = lambda: ("random", order_random(rng, ids, int(rng.randint(20, GAPLESS_N + 1))))  # noqa: E731
    trees = {"ones": lambda: [one() for _ in range(5)], "twos": lambda: [two() for _ in range(5)],
             "first": lambda: [one()] + [full() for _ in range(4)], "last": lambda: [full() for _ in range(4)] + [one()],
             "mixed": lambda: [full(), one(), two(), full(), one(), full(), two()]}[which]()
    return forest(seed, GAPLESS_N, trees)


def level_forest(gaps: int, lengths: str = "positive") -> TreeArrays:
    """One tree of ``gaps + 1`` leaves.  From 1 023 gaps on: a random tree on a universe three taxa larger.  Up to 4
    gaps: a caterpillar with ONE leaf in each 64-row block of a universe of 64 k + 3 taxa.  Leaves that share a row block
    are each other's neighbours in the block's record and are joined through level 0 alone, whatever the tree; with
    one leaf a block every query runs from the block's row to a column any number of gaps away, and a caterpillar's
    gaps get shallower from left to right, so every entry of every level above 0 is the second of the two it is made
    of."""
    k = gaps + 1
    rng = np.random.RandomState(gaps)
    if gaps >= 1023:
        return forest(gaps, k + 3, [("random", order_random(rng, np.arange(k + 3, dtype=np.int32), k))], lengths=lengths)
    order = (TR * rng.permutation(k) + rng.randint(0, TR, size=k)).astype(np.int32)
    return forest(gaps, TR * k + 3, [("caterpillar", order)], lengths=lengths)


def big_forest(leaves: int, mixed: bool, lengths: str = "positive") -> TreeArrays:
    """One tree of ``leaves`` leaves on BIG_TAXA taxa, alone or as tree 7 of a batch with twenty trees of 3 to 50
    leaves."""
    rng = np.random.RandomState(leaves + mixed)
    ids = np.arange(BIG_TAXA, dtype=np.int32)
    small = [("random", order_random(rng, ids, int(k))) for k in rng.randint(3, 51, size=20)] if mixed else []
    trees = small[:7] + [("random", order_random(rng, ids, leaves))] + small[7:]
    return forest(leaves, BIG_TAXA, trees, lengths=lengths)


BIG_ROWS = (100, 230)  # 130 rows: starts and ends inside a block, three row blocks


def gate_forest(n: int, n_trees: int, leaves: int | Sequence[int], seed: int = 8) -> TreeArrays:
    """``n_trees`` random trees of ``leaves`` leaves each (or one count per tree) on ``n`` taxa."""
    rng = np.random.RandomState(seed + n + n_trees)
    counts = [leaves] * n_trees if np.isscalar(leaves) else list(leaves)
    assert len(counts) == n_trees
    ids = np.arange(n, dtype=np.int32)
    return forest(seed, n, [("random", order_random(rng, ids, int(k))) for k in counts])


# (n, trees, leaves per tree): whole-matrix builds on each side of a gate, no switch set.  Whole-matrix builds have
# 1, 2, 3, 4, 9, 10, 11, 12, 21, 22, 23, 24, 37, ... tiles (the CPU test derives it): 8, 13 and 25 do not occur, the
# cases sit on the neighbours that do.
GATE_CASES = {
    "tiles_4": (256, 8, 120), "tiles_9": (257, 8, 120),  # the per-XCD order starts above 8 tiles
    "tiles_12": (512, 100, 60), "tiles_21": (513, 100, 60),  # producer / consumer kernel from 13 tiles
    "tiles_24_trees_127": (768, 127, 60), "tiles_24_trees_128": (768, 128, 60),  # tree-parallel from 128 trees ...
    "tiles_37_trees_128": (769, 128, 60),  # ... up to 24 tiles
    "tiles_37_trees_95": (769, 95, 60), "tiles_37_trees_96": (769, 96, 60),  # producer / consumer from 96 trees
    "coverage_at": (1024, 8, 16),  # leaves / (trees * taxa) = 1 / 64 exactly: not below
    "coverage_below": (1024, 8, [16] * 7 + [15]),  # one leaf fewer: per-tile tree lists
}
# row ranges (all column groups of the rows' blocks) reach the counts a whole matrix skips: exactly 8 and 9 tiles,
# and -- the producer / consumer kernel's gate does not ask for the whole matrix -- 12 tiles (3 blocks x 4 groups) and
# 13 (1 block x 13 groups, which takes 3 073 taxa) with 96 trees, 13 with 95
GATE_ROW_CASES = {"rows_tiles_8": (1024, 20, 200, (0, 128)), "rows_tiles_9": (768, 20, 200, (0, 192)),
                  "rows_tiles_12_trees_96": (1024, 96, 200, (0, 192)), "rows_tiles_13_trees_96": (3073, 96, 200, (0, 64)),
                  "rows_tiles_13_trees_95": (3073, 95, 200, (0, 64))}


def degree_forest(n: int, seed: int = 9) -> tuple[TreeArrays, int]:
    """Signed lengths on ``n`` taxa; taxon ``n // 2`` is in no tree (its degree is exactly 0)."""
    rng = np.random.RandomState(seed + n)
    lone = n // 2
    ids = np.setdiff1d(np.arange(n, dtype=np.int32), [lone]) if n >= 3 else np.arange(1, dtype=np.int32)
    trees = [("random", order_random(rng, ids)), ("balanced", order_random(rng, ids, max(1, len(ids) // 2))),
             ("random", order_random(rng, ids, max(1, len(ids) - 1)))]
    return forest(seed, n, trees, lengths="signed"), (lone if n >= 3 else n - 1)


def degree_ranges(n: int) -> list[tuple[int, int]]:
    """The whole matrix and row ranges with rows % 4 in {0, 1, 2, 3}, starting inside the matrix."""
    want = [(0, n), (1, 5), (2, 7), (n // 2, n // 2 + 6), (n - 7, n), (3, n)]
    return sorted({(a, b) for a, b in want if 0 <= a < b <= n})


RANK_N = 513
RANK_SPLITS = ([0, 1, RANK_N], [0, 65, RANK_N], [0, 257, 300, RANK_N])
CONTRACT_N = 300
CONTRACT_GROUPS = (1, 2, 255, 256, 257)


def contract_groups(n: int, n_groups: int, seed: int = 10) -> np.ndarray:
    """``group_start`` of ``n_groups`` consecutive non-empty ranges of [0, n), cuts at random."""
    rng = np.random.RandomState(seed + n_groups)
    cuts = np.sort(rng.permutation(np.arange(1, n))[: n_groups - 1])
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


def contract_half_and_singles(n: int) -> np.ndarray:
    """One group of half the taxa, then groups of one taxon."""
    return np.concatenate([[0], np.arange(n // 2, n + 1)]).astype(np.int32)


def contract_forest(n: int = CONTRACT_N, seed: int = 11) -> TreeArrays:
    rng = np.random.RandomState(seed)
    ids = np.arange(n, dtype=np.int32)
    return forest(seed, n, [("random", order_random(rng, ids, k)) for k in (n, n - 40, n // 2, n)], lengths="signed")
