"""References and builders for the edge cases of ``scs_score_internode``, no device.

``by_edges`` is a third judge beside ``internode_reference.by_paths`` and ``by_tables``: linear in the leaves, no pair
loop and no range minimum, so it reaches the all-rows lean calls on thousands of taxa.  The closed forms give whole
matrices of single trees (caterpillars, balanced trees, stars), ``composed`` puts such trees under a top tree and
knows every cell of the result by construction.  Then the polytomy builders, ``shifted`` (raw tables with per-tree
depth offsets and a chosen entry at every tree's last leaf), ``chunks`` (the staging chunks of a tree batch, restated)
and one builder per device case of ``tests/test_gpu_internode_edges.py``."""

import random
from functools import lru_cache

import internode_reference as ir
import numpy as np
import parsimony_reference as pr

from spectralclustersupertree_amd.flatten import TreeTables

INT32_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ by edges
def node_spans(gaps) -> list:
    """``(lo, hi)`` leaf spans of the inner nodes of T* below the root, by one stack pass over ``adj_depth``: a gap
    closes the open nodes deeper than itself and joins the open node of its own depth, if that is on top."""
    spans, stack = [], []  # stack: (depth, first leaf) of the open nodes, deepest on top
    for k, d in enumerate(gaps):
        lo = k
        while stack and stack[-1][0] > d:
            _, lo = stack.pop()
            spans.append((lo, k))
        if not stack or stack[-1][0] < d:
            stack.append((d, lo))
    m = len(gaps) + 1
    while len(stack) > 1:
        spans.append((stack.pop()[1], m - 1))
    return spans  # (what is left on the stack is the root)


def tree_by_edges(gaps) -> tuple:
    """``(row_sums, total)`` of one tree of m = len(gaps) + 1 leaves: Σ_b d(a, b) per leaf position a, and
    Σ_{a<b} d(a, b).  An edge above a node v of s_v leaves lies on the paths from a to the m - s_v leaves outside v
    when a is below it and to the s_v leaves inside otherwise: Σ_v s_v + Σ_{v above a, or a} (m - 2 s_v)."""
    m = len(gaps) + 1
    if m < 2:
        return np.zeros(m, dtype=np.int64), 0
    spans = node_spans(gaps)
    lo = np.array([s[0] for s in spans], dtype=np.int64).reshape(-1)
    hi = np.array([s[1] for s in spans], dtype=np.int64).reshape(-1)
    s = hi - lo + 1
    diff = np.zeros(m + 1, dtype=np.int64)
    np.add.at(diff, lo, m - 2 * s)
    np.add.at(diff, hi + 1, -(m - 2 * s))
    rows = int(s.sum()) + m + np.cumsum(diff[:m]) + (m - 2)  # (the leaves: s = 1 each, m - 2 for a's own)
    total = int((s * (m - s)).sum()) + m * (m - 1)
    return rows, total


def by_edges(specs, n_taxa: int, weights=None) -> dict:
    """``taxon_weight`` and ``taxon_sum`` of every taxon, and ``tree_total`` = Σ_{a<b} d per tree (unweighted)."""
    tw, ts, totals = np.zeros(n_taxa, dtype=np.int64), np.zeros(n_taxa, dtype=np.int64), []
    for t, (taxa, gaps) in enumerate(specs):
        rows, total = tree_by_edges(gaps)
        totals.append(total)
        w = 1 if weights is None else int(weights[t])
        if w == 0 or len(taxa) < 2:
            continue
        taxa = np.asarray(taxa, dtype=np.int64)
        tw[taxa] += w * (len(taxa) - 1)
        ts[taxa] += w * rows
    return {"taxon_weight": tw, "taxon_sum": ts, "tree_total": np.array(totals, dtype=np.int64)}


# ------------------------------------------------------------------------------------------------ closed forms
def caterpillar(taxa, left: bool = True) -> tuple:
    """Raw arrays of ((((a,b),c),d),...) when ``left``, else (a,(b,(c,...)))."""
    g = list(range(len(taxa) - 1))
    return list(taxa), g[::-1] if left else g


def caterpillar_d(m: int, left: bool = True) -> np.ndarray:
    """d of positions p < q of a left caterpillar is q - max(p, 1) + 2; the right one is its mirror image."""
    p = np.arange(m, dtype=np.int64)
    lo, hi = np.minimum(p[:, None], p[None, :]), np.maximum(p[:, None], p[None, :])
    d = hi - np.maximum(lo, 1) + 2
    d[p, p] = 0
    return d if left else d[::-1, ::-1].copy()


def caterpillar_depth(m: int, left: bool = True) -> np.ndarray:
    """Edges from the root to every leaf: m - max(p, 1) in a left caterpillar."""
    dep = m - np.maximum(np.arange(m, dtype=np.int64), 1)
    return dep if left else dep[::-1].copy()


def balanced(taxa) -> tuple:
    """Raw arrays of the balanced binary tree on 2^k taxa: the gap after leaf i splits at depth
    k - bit_length(i ^ (i + 1))."""
    k = (len(taxa) - 1).bit_length()
    assert len(taxa) == 1 << k
    return list(taxa), [k - (i ^ (i + 1)).bit_length() for i in range(len(taxa) - 1)]


def balanced_d(k: int) -> np.ndarray:
    i = np.arange(1 << k, dtype=np.int64)
    x = i[:, None] ^ i[None, :]
    bits = np.zeros_like(x)
    while x.any():  # bit_length(i xor j): the levels up to the node that holds both
        bits += x > 0
        x >>= 1
    return 2 * bits


def star(taxa, depth: int = 0) -> tuple:
    return list(taxa), [depth] * (len(taxa) - 1)


def star_d(m: int) -> np.ndarray:
    return 2 * (1 - np.eye(m, dtype=np.int64))


# ------------------------------------------------------------------------------------------------ composed trees
class Piece:
    """A tree on positions 0 ... m - 1: its gaps, d between its leaves and every leaf's depth below its root."""

    def __init__(self, gaps, d, depth):
        self.gaps, self.d, self.depth = list(gaps), np.asarray(d, dtype=np.int64), np.asarray(depth, dtype=np.int64)
        self.m = len(self.gaps) + 1
        assert self.d.shape == (self.m, self.m) and self.depth.shape == (self.m,)


def piece_leaf() -> Piece:
    return Piece([], np.zeros((1, 1)), np.zeros(1))


def piece_caterpillar(m: int, left: bool = True) -> Piece:
    return Piece(caterpillar(range(m), left)[1], caterpillar_d(m, left), caterpillar_depth(m, left))


def piece_balanced(k: int) -> Piece:
    return Piece(balanced(range(1 << k))[1], balanced_d(k), np.full(1 << k, k))


def piece_star(m: int) -> Piece:
    return Piece([0] * (m - 1), star_d(m), np.ones(m))


def piece_of(gaps) -> Piece:
    """Any tree, by climbing parent pointers (``internode_reference.tree_paths``) with one leaf more beside its root:
    that leaf's distance to a leaf is the leaf's depth plus the two edges below the new root."""
    m = len(gaps) + 1
    if m == 1:
        return piece_leaf()
    _, d = ir.tree_paths([ir.nested_of(list(range(m)), list(gaps)), m])
    return Piece(gaps, d[:m, :m], d[:m, m] - 2)


class Composed:
    """A top tree with a tree of its own in every block (a block of one leaf is the top leaf itself)."""

    def __init__(self, top: Piece, blocks: list):
        assert top.m == len(blocks) >= 2
        self.top, self.blocks = top, blocks
        below = max(top.gaps) + 1  # every gap inside a block lies deeper than every gap of the top tree
        gaps = []
        for i, b in enumerate(blocks):
            gaps += [below + g for g in b.gaps]
            if i + 1 < len(blocks):
                gaps.append(top.gaps[i])
        self.gaps = gaps
        self.m = len(gaps) + 1
        self.block_of = np.repeat(np.arange(len(blocks)), [b.m for b in blocks])
        self.start = np.concatenate([[0], np.cumsum([b.m for b in blocks])])
        self.depth = np.concatenate([b.depth for b in blocks])

    def matrix(self) -> np.ndarray:
        """Every cell, as outer sums per block pair."""
        d = np.zeros((self.m, self.m), dtype=np.int64)
        for i, a in enumerate(self.blocks):
            for j, b in enumerate(self.blocks):
                at = (slice(self.start[i], self.start[i + 1]), slice(self.start[j], self.start[j + 1]))
                d[at] = a.d if i == j else a.depth[:, None] + b.depth[None, :] + self.top.d[i, j]
        return d

    def rows(self, positions) -> np.ndarray:
        """The rows of ``matrix`` at the leaf positions given."""
        out = np.zeros((len(positions), self.m), dtype=np.int64)
        for x, p in enumerate(positions):
            i = int(self.block_of[p])
            out[x] = self.depth[p] + self.depth + self.top.d[i][self.block_of]
            out[x, self.start[i]:self.start[i + 1]] = self.blocks[i].d[p - self.start[i]]
        return out


def composed(top: Piece, blocks: list) -> Composed:
    return Composed(top, blocks)


def sum_rows(trees, n_taxa: int, rows, weights=None) -> dict:
    """The three matrices' rows ``rows`` (taxon ids) of sources given as ``(taxa, Composed)``."""
    out = {k: np.zeros((len(rows), n_taxa), dtype=np.int64) for k in ir.MATRICES}
    for t, (taxa, c) in enumerate(trees):
        w = 1 if weights is None else int(weights[t])
        pos = {x: p for p, x in enumerate(taxa)}
        have = [(i, pos[a]) for i, a in enumerate(rows) if a in pos]
        if not have or w == 0:
            continue
        d = c.rows([p for _, p in have])
        at = np.asarray(taxa, dtype=np.int64)
        for (i, p), row in zip(have, d):
            seen = np.ones(c.m, dtype=np.int64)
            seen[p] = 0
            out["pair_weight"][i, at] += w * seen
            out["dist_sum"][i, at] += w * row
            out["sq_sum"][i, at] += w * row * row
    return out


# ------------------------------------------------------------------------------------------------ polytomies
RUN_PLACES = ("left", "right", "middle", "interrupted", "ended")


def polytomy_gaps(run: int, where: str, arm: int = 3) -> list:
    """The gaps of a tree with ``run`` equal gaps in a row: a polytomy of run + 1 children.  ``left`` / ``right``: the
    deepest node of a caterpillar of ``arm`` more leaves, at the tree's end; ``middle``: below two such arms, whose
    gaps of equal depth on both sides are one node each (a deeper clade between them); ``interrupted``: deeper clades
    hang between the run's gaps, still one node; ``ended``: a shallower gap cuts the run in two, two nodes."""
    if where == "left":
        return [arm] * run + list(range(arm - 1, -1, -1))
    if where == "right":
        return list(range(arm)) + [arm] * run
    if where == "middle":
        return list(range(arm)) + [arm] * run + list(range(arm - 1, -1, -1))
    if where == "interrupted":
        gaps = []
        for i in range(run):
            gaps.append(1)
            if i % 3 == 1 and i + 1 < run:
                gaps += [2 + i % 4] * (1 + i % 2) + ([5, 5] if i % 5 == 1 else [])
        return gaps + [0]
    assert where == "ended"
    return [2] * run + [1] + [2] * run + [0]


def polytomy_piece(run: int, where: str, arm: int = 3) -> Composed:
    """``left`` and ``right`` of ``polytomy_gaps`` as a star under a caterpillar, with every cell known."""
    assert where in ("left", "right")
    blocks = [piece_star(run + 1)] + [piece_leaf()] * arm
    return composed(piece_caterpillar(arm + 1, where == "left"), blocks if where == "left" else blocks[::-1])


RUNS = tuple(s for k in range(1, 11) for s in ((1 << k) - 1, 1 << k, (1 << k) + 1))


def run_specs(where: str, seed: int = 0) -> tuple:
    """``(specs, n_taxa)``: one tree per run length 2^k - 1, 2^k, 2^k + 1, k = 1 ... 10, on random taxa; ``star``:
    stars of that many leaves (a star of one leaf is a tree without a gap)."""
    rng = random.Random(f"runs {where} {seed}")
    all_gaps = [[7] * (r - 1) for r in RUNS] if where == "star" else [polytomy_gaps(r, where) for r in RUNS]
    n = max(len(g) for g in all_gaps) + 4
    return [(rng.sample(range(n), len(g) + 1), g) for g in all_gaps], n


# ------------------------------------------------------------------------------------------------ raw tables, chunks
def shifted(specs, offsets, last: int, n_taxa: int) -> TreeTables:
    """The tables of ``specs`` with tree t's ``adj_depth`` raised by ``offsets[t]`` and the entry at every tree's
    last leaf, which belongs to no gap, set to ``last``."""
    off, leaf_taxon, adj = [0], [], []
    for (taxa, gaps), o in zip(specs, offsets):
        leaf_taxon += list(taxa)
        adj += [g + o for g in gaps] + [last]
        off.append(len(leaf_taxon))
    assert max(adj, default=0) <= INT32_MAX and min(adj, default=0) >= 0
    return TreeTables(n_taxa=n_taxa, tree_off=np.asarray(off, dtype=np.int64),
                      leaf_taxon=np.asarray(leaf_taxon, dtype=np.int32), adj_depth=np.asarray(adj, dtype=np.int32),
                      adj_val=np.zeros(len(adj), dtype=np.float64), tree_w=np.ones(len(specs), dtype=np.float64))


def chunks(t0: int, t1: int) -> tuple:
    """``(n_chunks, words of every chunk)`` of the tree batch [t0, t1) as ``k_in_sweep`` stages it: the batch's words
    of 32 trees, 32 words at a time from the word of its first tree."""
    w_lo, w_hi = t0 >> 5, (t1 - 1) >> 5
    n = (w_hi - w_lo) // 32 + 1
    return n, [min(32, w_hi - (w_lo + 32 * c) + 1) for c in range(n)]


def batch_chunks(plan: dict) -> list:
    """``chunks`` of every tree batch of a plan."""
    return [chunks(int(a), int(a + b)) for a, b in zip(plan["first_tree"], plan["trees"])]


def rounds(largest: int) -> int:
    """The rounds of pointer doubling of a tree batch: the least L with 2^L above its largest tree."""
    return max(int(largest), 1).bit_length()


def off_of(specs) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([len(t) for t, _ in specs])]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the device cases
def random_specs(rng, n: int, n_trees: int, lo: int, hi: int, arity: int = 3) -> list:
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(min(lo, n), min(hi, n))), arity, rng)
             for _ in range(n_trees)]
    return ir.specs_of(trees)


def corners(n: int) -> tuple:
    """((n - 1, 0), (1, n - 2)): the last taxon with the first, placed by hand."""
    return ir.specs_of([[[n - 1, 0], [1, n - 2]]])[0]


TG_TAXA, TG_ABSENT, TG_ROWS = 600, 8, 5462


@lru_cache(maxsize=None)
def case_tg_rows() -> tuple:
    """``(specs, n, rows)``: 1 100 trees of 2 ... 9 leaves over 600 taxa, of which 592 ... 599 are in no tree but
    598 and 599 in the last and in tree 999, by hand; 5 462 rows with repeats, the taxa of no tree among them."""
    rng = random.Random(4201)
    n = TG_TAXA
    specs = random_specs(rng, n - TG_ABSENT, 1100, 2, 9)
    specs[-1] = corners(n)
    specs[999] = ir.specs_of([[[n - 1, 1], [n - 2, [0, 300]]]])[0]
    rows = [n - 1, 0, 255, 256, 511, 512, n - 3, n - 2, 1] + [rng.randrange(n) for _ in range(TG_ROWS - 10)] + [n - 5]
    return specs, n, rows


@lru_cache(maxsize=None)
def case_mirror(n: int) -> list:
    """400 trees of 2 ... 9 leaves over n taxa, one of 40, and the corners."""
    rng = random.Random(4300 + n)
    specs = random_specs(rng, n, 400, 2, 9) + random_specs(rng, n, 1, 40, 40, arity=5)
    return [*specs, corners(n)]


REAL_TAXA = 3000


@lru_cache(maxsize=None)
def case_real() -> tuple:
    """``(trees, specs, n, weights)``: ten composed trees of 2 000 ... 3 000 leaves over 3 000 taxa.  A top tree of
    about a hundred leaves (a random one, a caterpillar or a star) over blocks that are caterpillars of both hands,
    balanced trees, stars of 2^j - 1, 2^j, 2^j + 1 leaves, random trees and single leaves."""
    rng = random.Random(4400)
    n = REAL_TAXA
    trees, weights = [], []
    for t in range(10):
        want = rng.randint(2000, n)
        j = 2 + t % 6  # (polytomy runs of 2^j - 1, 2^j and 2^j + 1 equal gaps, j = 2 ... 7 over the trees)
        blocks = [piece_star(r + 1) for r in ((1 << j) - 1, 1 << j, (1 << j) + 1)]
        rng.shuffle(blocks)
        m = sum(b.m for b in blocks)
        while m < want:
            kind = rng.randrange(6)
            j = rng.randint(1, 7)
            size = rng.choice([(1 << j) - 1, 1 << j, (1 << j) + 1])
            if kind == 0 or size < 2:
                b = piece_leaf()
            elif kind == 1:
                b = piece_caterpillar(size + 30 * (j == 7), left=bool(rng.randrange(2)))
            elif kind == 2:
                b = piece_balanced(j)
            elif kind == 3:
                b = piece_star(size)
            else:
                b = piece_of(ir.specs_of([pr.rand_tree(list(range(min(size, 40))), rng.choice([2, 3, 5]), rng)])[0][1])
            if m + b.m > n:
                b = piece_leaf()
            blocks.append(b)
            m += b.m
        k = len(blocks)
        if t % 3 == 0:
            top = piece_caterpillar(k, left=bool(t & 1)) if k <= 400 else piece_star(k)
        elif t % 3 == 1:
            top = piece_star(k)
        else:
            top = piece_of(ir.specs_of([pr.rand_tree(list(range(k)), 4, rng)])[0][1]) if k <= 150 else piece_star(k)
        c = composed(top, blocks)
        trees.append((rng.sample(range(n), c.m), c))
        weights.append(rng.choice([1, 2, 3, 0]) if t else 2)
    # the corners and the last with the first in two trees by hand: positions swapped into place
    for t, (a, b) in ((0, (n - 1, 0)), (1, (0, n - 1))):
        taxa = trees[t][0]
        for want, at in ((a, 0), (b, len(taxa) - 1)):
            if want in taxa:
                i = taxa.index(want)
                taxa[i], taxa[at] = taxa[at], taxa[i]
            else:
                taxa[at] = want
        assert len(set(taxa)) == len(taxa)
    specs = [(taxa, c.gaps) for taxa, c in trees]
    return trees, specs, n, weights


def case_chunk_gate(n_trees: int) -> tuple:
    """``(specs, n)``: 70 taxa; taxon 69 only in tree 1 023, the last bit of chunk 0, taxon 68 only in tree 1 024,
    the first bit of chunk 1, taxon 67 in both and nowhere else (as far as the trees exist)."""
    rng = random.Random(4500 + n_trees)
    n = 70
    specs = random_specs(rng, n - 3, n_trees, 2, 9)
    if n_trees > 1023:
        specs[1023] = (specs[1023][0] + [n - 1, n - 3], specs[1023][1] + [0, 0])
    if n_trees > 1024:
        specs[1024] = ([n - 2, n - 3] + specs[1024][0], [1, 0] + specs[1024][1])
    return specs, n


def case_mid_word(n_trees: int) -> tuple:
    """``(specs, n)``: 70 taxa, taxon 69 only in the last tree, with a random tree beside it."""
    rng = random.Random(4600 + n_trees)
    n = 70
    specs = random_specs(rng, n - 1, n_trees, 2, 9)
    specs[-1] = ir.specs_of([[pr.rand_tree(specs[-1][0], 2, rng), n - 1]])[0]
    return specs, n


WAVE_SIZES = (64, 128, 1, 63, 65, 1, 64)


def case_waves(turn: str, seed: int = 0) -> tuple:
    """``(specs, n)``: trees of 64, 128, 1, 63, 65, 1 and 64 leaves: leaves 0 ... 63 and 64 ... 191 are whole waves
    of one tree, the waves from 192 on mix trees and one-leaf trees, the last ends at leaf 386, two lanes into its
    wave.  ``turn``: ``left`` caterpillars (the deepest leaves first: lane 0 of a tree on a wave boundary),
    ``right`` (last: lane 63), ``mixed`` (alternating) or ``random`` trees."""
    rng = random.Random(f"waves {turn} {seed}")
    n = 130
    specs = []
    for i, m in enumerate(WAVE_SIZES):
        taxa = rng.sample(range(n), m)
        if m == 1:
            specs.append((taxa, []))
        elif turn == "random":
            specs.append(ir.specs_of([pr.rand_tree(taxa, 3, rng)])[0])
        else:
            specs.append(caterpillar(taxa, left=turn == "left" or (turn == "mixed" and i % 2 == 0)))
    return specs, n


def case_rounds(which: str) -> tuple:
    """``deep_then_small``: a caterpillar of 300 leaves, then trees of 2, 3, 2 and 3 leaves; ``parities``:
    caterpillars of 3, 4, 5, 6 and 7 leaves (two rounds of pointer doubling for 3 leaves, three from 4 on: with a
    tree a batch the final buffer is the first and the second)."""
    rng = random.Random(f"rounds {which}")
    n = 310
    sizes = (300, 2, 3, 2, 3) if which == "deep_then_small" else (3, 4, 5, 6, 7)
    return [caterpillar(rng.sample(range(n), m), left=bool(i & 1)) for i, m in enumerate(sizes)], n


def case_leak() -> tuple:
    """``(specs, n)``: a mixed source for ``shifted``: random trees, stars, caterpillars and one-leaf trees."""
    rng = random.Random(4700)
    n = 90
    specs = random_specs(rng, n, 14, 2, 40, arity=4)
    specs[3] = (rng.sample(range(n), 1), [])
    specs[7] = star(rng.sample(range(n), 33))
    specs[8] = caterpillar(rng.sample(range(n), 65))
    specs[9] = (rng.sample(range(n), 1), [])
    specs[10] = caterpillar(rng.sample(range(n), 64), left=False)
    specs.append(corners(n))
    return specs, n
