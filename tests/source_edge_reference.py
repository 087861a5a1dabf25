"""References, builders and named numbers for the edge pass over the parsimony, source-pair, coverage and pair-triplet
exports (helper module, not collected).  No device: the plans come from the library's host
entries (``backend.debug_*_plan``).

The project's references stay the judges where they reach: ``parsimony_reference.reference`` / ``hartigan``,
``source_pairs_reference.linear`` / ``by_sets``, ``source_triplets_reference.quadratic`` / ``by_sets``,
``coverage_reference.by_matmul`` / ``by_sets``.  New here:

* ``Family``: a random binary tree on positions 0 .. n - 1 as numpy arrays of its inner nodes (made level by level, no
  Python loop over leaves), the *members* of a family -- the tree with some inner nodes contracted, restricted to some
  positions -- and their flattened tables;
* ``pair_contracted``: the four pair-triplet terms of two members of one family of which one keeps a subset of the
  other's nodes: every triple the coarser one resolves the finer one resolves alike, so ``triplets_shared`` is the
  coarser tree's own count, sum C(s, 2) (ps - s) over its nodes with s, ps counted on the common positions -- linear
  time, nothing of the kernel's bitset rows, node lists or node pairs;
* ``pair_composed``: the four terms of two trees that are each a top tree over the same k blocks with a tree of its
  own inside every block: the triples inside one block by ``source_triplets_reference.pair_quadratic`` on the block,
  those with two taxa in one block (resolved alike by both), and those over three blocks by the node-pair sum on the
  two top trees with the blocks' common sizes as weights;
* ``coverage_by_signatures``: coverage from the distinct membership signatures of the taxa (few trees): a table over
  all 2^M masks, no product over trees and no walk over taxa;
* the closed forms of parsimony on a star supertree and of the coverage of one tree over all taxa;
* the cases of ``tests/test_gpu_source_edges.py`` and, per case, the numbers it is named for.
"""

from __future__ import annotations

import random
from dataclasses import dataclass
from functools import lru_cache
from math import comb

import coverage_reference as cr
import numpy as np
import parsimony_reference as pr
import source_pairs_reference as sp
import source_triplets_reference as st
from score_reference import _clusters

from spectralclustersupertree_amd import backend
from spectralclustersupertree_amd.flatten import TreeTables

TP_LDS_MAX = st.TP_LDS_MAX
TP_LDS_BUDGET = st.TP_LDS_BUDGET
LDS_64K = 64 << 10


# ------------------------------------------------------------------------------------------------ tables and lists
def tables_of(trees, n_taxa: int) -> TreeTables:
    """Flattened tables of trees given as ``(leaf_taxon, gap depths)`` array pairs (m leaves: m - 1 gaps)."""
    off, leaf, adj = [0], [], []
    for taxa, gaps in trees:
        assert len(gaps) == max(len(taxa) - 1, 0)
        leaf.append(np.asarray(taxa, dtype=np.int32))
        adj.append(np.append(np.asarray(gaps, dtype=np.int32), np.int32(0)) if len(taxa) else np.zeros(0, np.int32))
        off.append(off[-1] + len(taxa))
    n = off[-1]
    return TreeTables(n_taxa=n_taxa, tree_off=np.asarray(off, dtype=np.int64), leaf_taxon=np.concatenate(leaf),
                      adj_depth=np.concatenate(adj), adj_val=np.zeros(n, dtype=np.float64),
                      tree_w=np.ones(len(trees), dtype=np.float64))


def arrays_of(tree) -> tuple[np.ndarray, np.ndarray]:
    """A nested-list tree as ``(leaf_taxon, gap depths)``."""
    leaves, gaps, _ = pr.layout(tree)
    return np.asarray(leaves, dtype=np.int32), np.asarray(gaps, dtype=np.int32)


def nested_of(taxa, gaps):
    """``(leaf_taxon, gap depths)`` as nested lists: the clusters of the depth sequence, each a list of its maximal
    sub-clusters and loose leaves (a unary chain of the tables leaves no trace: it holds no cluster of its own)."""
    n = len(taxa)
    if n == 1:
        return int(taxa[0])
    nodes = sorted({(lo, -hi) for lo, hi, _ in _clusters(np.asarray(gaps), n)} | {(0, -(n - 1))})
    root: list = []
    stack = [(0, n - 1, root, [0])]  # lo, hi, list, next leaf to place
    for lo, mhi in nodes[1:]:
        hi = -mhi
        while not (stack[-1][0] <= lo and hi <= stack[-1][1]):
            _close(stack.pop(), taxa)
        top = stack[-1]
        top[2].extend(int(taxa[p]) for p in range(top[3][0], lo))
        top[3][0] = hi + 1
        mine: list = []
        top[2].append(mine)
        stack.append((lo, hi, mine, [lo]))
    while stack:
        _close(stack.pop(), taxa)
    return root


def _close(frame, taxa) -> None:
    _, hi, into, nxt = frame
    into.extend(int(taxa[p]) for p in range(nxt[0], hi + 1))


def nested_of_tables(tables: TreeTables) -> list:
    off = tables.tree_off
    return [nested_of(tables.leaf_taxon[off[t]:off[t + 1]], tables.adj_depth[off[t]:off[t + 1] - 1])
            for t in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------------ families
@dataclass(frozen=True, eq=False)
class Family:
    """A binary tree on positions 0 .. n - 1: node v spans [lo[v], hi[v]) and splits it at cut[v]; node 0 is the root,
    parents come before children, depth[v] counts the proper ancestors."""
    n: int
    lo: np.ndarray
    hi: np.ndarray
    cut: np.ndarray
    parent: np.ndarray
    depth: np.ndarray
    taxa: np.ndarray  # taxon of every position

    @property
    def nodes(self) -> int:
        return len(self.lo)


def random_family(n: int, seed: int, taxa=None, spread: float = 1.0) -> Family:
    """Every node splits its span at a random place (``spread`` < 1 keeps the cut that near the middle), level by
    level; taxa: a random labelling of the positions by 0 .. n - 1 unless given."""
    assert n >= 2
    rs = np.random.RandomState(seed)
    los, his, cuts, pars, deps = [], [], [], [], []
    lo, hi, par = np.array([0], dtype=np.int64), np.array([n], dtype=np.int64), np.array([-1], dtype=np.int64)
    first, d = 0, 0
    while len(lo):
        size = hi - lo
        u = 0.5 + (rs.random_sample(len(lo)) - 0.5) * spread
        cut = lo + 1 + np.minimum((u * (size - 1)).astype(np.int64), size - 2)
        idx = first + np.arange(len(lo), dtype=np.int64)
        los.append(lo), his.append(hi), cuts.append(cut), pars.append(par), deps.append(np.full(len(lo), d))
        c_lo, c_hi, c_par = np.concatenate([lo, cut]), np.concatenate([cut, hi]), np.concatenate([idx, idx])
        big = c_hi - c_lo >= 2
        first += len(lo)
        lo, hi, par = c_lo[big], c_hi[big], c_par[big]
        d += 1
    taxa = rs.permutation(n) if taxa is None else np.asarray(taxa)
    cat = lambda parts: np.concatenate(parts).astype(np.int64)  # noqa: E731
    fam = Family(n, cat(los), cat(his), cat(cuts), cat(pars), cat(deps), taxa.astype(np.int64))
    assert fam.nodes == n - 1 and len(taxa) == n
    return fam


def contraction(fam: Family, seed: int, share: float = 1 / 3) -> np.ndarray:
    """``keep``: every inner node but a random ``share`` of the non-root ones."""
    keep = np.random.RandomState(seed).random_sample(fam.nodes) >= share
    keep[0] = True
    return keep


def _kept_above(fam: Family, keep: np.ndarray) -> np.ndarray:
    """The nearest kept proper ancestor of every node (the root: itself)."""
    up = fam.parent.copy()
    up[0] = 0
    while not keep[up].all():
        up = np.where(keep[up], up, fam.parent[up])
    return up


def member(fam: Family, keep=None, mask=None) -> tuple[np.ndarray, np.ndarray]:
    """``(leaf_taxon, gap depths)`` of the family's tree with the nodes outside ``keep`` contracted into their parents,
    restricted to the positions of ``mask``: a gap takes the depth -- counted in kept nodes -- of the kept node that
    holds its split, a restricted gap the least of the gaps it spans; the root's gaps are brought to 0."""
    keep = np.ones(fam.nodes, dtype=bool) if keep is None else keep
    up = _kept_above(fam, keep)
    kd = np.zeros(fam.nodes, dtype=np.int64)
    for d in range(1, int(fam.depth.max()) + 1):
        at = np.flatnonzero(fam.depth == d)
        kd[at] = kd[up[at]] + 1  # (of a contracted node: the depth it would have, never used)
    own = np.where(keep, np.arange(fam.nodes), up)
    gaps = np.zeros(fam.n - 1, dtype=np.int64)
    gaps[fam.cut - 1] = kd[own]
    if mask is None:
        return fam.taxa.astype(np.int32), gaps.astype(np.int32)
    pos = np.flatnonzero(mask)
    if len(pos) < 2:
        return fam.taxa[pos].astype(np.int32), np.zeros(0, dtype=np.int32)
    rg = np.minimum.reduceat(gaps[: pos[-1]], pos[:-1])
    return fam.taxa[pos].astype(np.int32), (rg - rg.min()).astype(np.int32)


def resolved(fam: Family, keep=None, mask=None) -> int:
    """The triples of the positions of ``mask`` that the kept nodes resolve: sum C(s, 2) (ps - s), s and ps the mask's
    positions below a kept node and below the kept node above it.  (A node whose restriction equals its parent's adds
    nothing, one of fewer than two positions neither: no set has to be told from another.)"""
    keep = np.ones(fam.nodes, dtype=bool) if keep is None else keep
    mask = np.ones(fam.n, dtype=bool) if mask is None else mask
    assert fam.n < 2_000_000  # (C(s, 2) (ps - s) <= n^3 / 2 and the sum <= C(n, 3): below 2^62)
    cnt = np.concatenate([[0], np.cumsum(mask, dtype=np.int64)])
    s = cnt[fam.hi] - cnt[fam.lo]
    ps = s[_kept_above(fam, keep)]
    term = s * (s - 1) // 2 * (ps - s)
    term[0] = 0
    return int(term[keep].sum())


def pair_contracted(fam: Family, keep_a, mask_a, keep_b, mask_b) -> tuple[int, int, int, int]:
    """``(common, triplets, triplets_other, triplets_shared)`` of two members of one family whose kept nodes are
    nested: the coarser tree's clusters on the common positions are clusters of the finer one's, so what it resolves
    the other resolves alike."""
    full = np.ones(fam.nodes, dtype=bool)
    keep_a, keep_b = (full if keep_a is None else keep_a), (full if keep_b is None else keep_b)
    everywhere = np.ones(fam.n, dtype=bool)
    both = (everywhere if mask_a is None else mask_a) & (everywhere if mask_b is None else mask_b)
    c = int(both.sum())
    if c < 3:
        return c, 0, 0, 0
    a_in_b, b_in_a = bool((keep_b | ~keep_a).all()), bool((keep_a | ~keep_b).all())
    assert a_in_b or b_in_a, "the kept nodes of the two members are not nested"
    ta, tb = resolved(fam, keep_a, both), resolved(fam, keep_b, both)
    return c, ta, tb, (tb if b_in_a else ta)


# ------------------------------------------------------------------------------------------------ composed trees
def compose(top, subtrees):
    """The top tree (nested lists over block ids) with block i replaced by ``subtrees[i]``."""
    if not isinstance(top, list):
        return subtrees[top]
    return [compose(x, subtrees) for x in top]


def _lists_with_parents(tree, up=None, out=None) -> list:
    """``(leaf set, parent's leaf set)`` of every non-root list of a nested-list tree."""
    out = [] if out is None else out
    if isinstance(tree, list):
        mine = frozenset(pr.leaves_of(tree))
        if up is not None:
            out.append((mine, up))
        for x in tree:
            _lists_with_parents(x, mine, out)
    return out


def _top_rows(top, k: int) -> tuple[np.ndarray, np.ndarray]:
    pairs = _lists_with_parents(top)
    own, par = np.zeros((len(pairs), k)), np.zeros((len(pairs), k))
    for r, (mine, up) in enumerate(pairs):
        own[r, list(mine)] = 1.0
        par[r, list(up)] = 1.0
    return own, par


def pair_composed(top_a, subs_a, top_b, subs_b, inside=st.pair_quadratic) -> tuple[int, int, int, int]:
    """The four terms of ``compose(top_a, subs_a)`` against ``compose(top_b, subs_b)``: both top trees hold every
    block id 0 .. k - 1 once and have at least two children at the root, block i of either tree lies on taxa no other
    block has.  With b_i the common taxa of block i and c their sum: the triples inside one block (``inside`` on the
    block's two subtrees), the C(b_i, 2) (c - b_i) with two taxa in block i -- a cluster of both trees, so both say
    xy|z --, and the triples over three blocks: for top nodes u of A and v of B the pairs from different blocks of
    u ∩ v, ((sum b)^2 - sum b^2) / 2, times the taxa of (pu - u) ∩ (pv - v), sum b."""
    k = len(subs_a)
    assert len(subs_b) == k and sorted(pr.leaves_of(top_a)) == sorted(pr.leaves_of(top_b)) == list(range(k))
    assert isinstance(top_a, list) and isinstance(top_b, list) and len(top_a) >= 2 and len(top_b) >= 2
    la = [set(pr.leaves_of(x)) for x in subs_a]
    lb = [set(pr.leaves_of(x)) for x in subs_b]
    all_a, all_b = set().union(*la), set().union(*lb)
    assert len(all_a) == sum(map(len, la)) and len(all_b) == sum(map(len, lb))
    b = np.array([len(la[i] & lb[i]) for i in range(k)], dtype=np.float64)
    c = int(b.sum())
    assert len(all_a & all_b) == c, "a taxon lies in different blocks of the two trees"
    if c < 3:
        return c, 0, 0, 0
    assert c ** 3 < 1 << 53  # (every product and partial sum below: an integer a float64 holds exactly)
    ta = tb = ts = 0
    for i in range(k):
        if b[i] >= 3:
            _, xa, xb, xs = inside(subs_a[i], subs_b[i])
            ta, tb, ts = ta + xa, tb + xb, ts + xs
    two = int(sum(comb(int(x), 2) * (c - int(x)) for x in b))
    y, py = _top_rows(top_a, k)
    z, pz = _top_rows(top_b, k)

    def over_three(own, par):
        s1, s2 = own @ b, own @ (b * b)
        return int(np.rint(((s1 * s1 - s2) / 2 * ((par - own) @ b)).sum()))

    s1, s2 = (y * b) @ z.T, (y * b * b) @ z.T
    out = ((py - y) * b) @ (pz - z).T
    shared3 = int(np.rint(((s1 * s1 - s2) / 2 * out).sum()))
    return c, ta + two + over_three(y, py), tb + two + over_three(z, pz), ts + two + shared3


# ------------------------------------------------------------------------------------------------ closed forms
def star_parsimony(tree) -> dict:
    """Every output of the parsimony export for one source ``tree`` (nested lists) on a star supertree that holds all
    its taxa: a character C of a tree of m leaves takes min(|C|, m - |C| + 1) changes -- one per taxon of C, or the
    outgroup's and one per taxon outside C --, so ``mrp_length`` is ``mrp_max``; with 2 <= |C| < m that is at least 2,
    a cherry's included: nothing is perfect on a star."""
    m = len(pr.leaves_of(tree))
    lo, hi = pr.characters(tree) if m >= 3 else (np.zeros(0, dtype=np.int64),) * 2
    width = hi - lo + 1
    length = np.minimum(width, m - width + 1)
    return {"mrp_chars": len(lo), "mrp_length": int(length.sum()), "mrp_perfect": int((length == 1).sum()),
            "mrp_max": int(length.sum()), "char_len": length.astype(np.int32), "char_lo": lo.astype(np.int32),
            "char_hi": hi.astype(np.int32)}


def caterpillar_star_length(m: int) -> int:
    """``mrp_length`` of a caterpillar of m leaves on a star: sum over s = 2 .. m - 1 of min(s, m - s + 1)."""
    return sum(min(s, m - s + 1) for s in range(2, m))


def one_tree_coverage(n: int) -> int:
    """``taxon_covered`` of every taxon when one tree holds all n taxa (k = 1): the pairs of the others."""
    return comb(n - 1, 2)


# ------------------------------------------------------------------------------------------------ coverage, few trees
def coverage_by_signatures(sets, n_taxa: int, k: int = 1, rows=None, matrices: bool = True) -> dict:
    """The outputs of the coverage export from the taxa's signatures (bit t: tree t holds the taxon), for at most 16
    trees: G[s] = the taxa whose signature shares at least k trees with the mask s, for every mask; then
    ``pair_covered[a][b]`` = G[sig a & sig b] less a and b themselves, which are among those taxa exactly when the pair
    shares k trees."""
    m = len(sets)
    assert m <= 16
    sig = np.zeros(n_taxa, dtype=np.int64)
    for t, s in enumerate(sets):
        assert len(set(s)) == len(s)
        sig[list(s)] |= 1 << t
    pop = np.array([bin(x).count("1") for x in range(1 << m)], dtype=np.int64)
    held = np.bincount(sig, minlength=1 << m)
    present = np.flatnonzero(held)
    masks = np.arange(1 << m, dtype=np.int64)
    g = np.zeros(1 << m, dtype=np.int64)
    for s in present:
        g += held[s] * (pop[masks & s] >= k)
    ids = np.arange(n_taxa) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    out = {"occurs": pop[sig].astype(np.int32)}
    meet = sig[ids][:, None] & sig[None, :]
    pc = np.where(pop[meet] >= k, g[meet] - 2, 0)
    pc[np.arange(len(ids)), ids] = 0
    out["taxon_covered"] = pc.sum(axis=1, dtype=np.int64) // 2
    out["pair_trees"] = pop[meet].astype(np.int32) if matrices else None
    out["pair_covered"] = pc.astype(np.int32) if matrices else None
    return out


# ------------------------------------------------------------------------------------------------ array trees
def join(trees) -> tuple[np.ndarray, np.ndarray]:
    """The ``(leaf_taxon, gap depths)`` trees under one new root."""
    taxa, gaps = [], []
    for i, (t, g) in enumerate(trees):
        if i:
            gaps.append(np.zeros(1, dtype=np.int32))
        taxa.append(np.asarray(t, dtype=np.int32))
        gaps.append(np.asarray(g, dtype=np.int32) + 1)
    return np.concatenate(taxa), np.concatenate(gaps)


def relabel(tree, to):
    return [relabel(x, to) for x in tree] if isinstance(tree, list) else int(to[tree])


def balanced(leaves):
    leaves = list(leaves)
    half = len(leaves) // 2
    return leaves[0] if len(leaves) == 1 else [balanced(leaves[:half]), balanced(leaves[half:])]


@dataclass(eq=False)
class Case:
    """One GPU case: the tables, the call's rows, the reference of every output, and what the builder knows of it."""
    tables: TreeTables
    ref: dict
    rows: list | None = None
    note: dict | None = None


def _cells(m: int, rows, cell, keys=st.KEYS, swap=(0, 2, 1, 3)) -> dict:
    """The matrices of ``cell(a, b)`` -> four numbers over ``rows`` x m trees (a mirrored cell is read swapped)."""
    rows = list(range(m)) if rows is None else list(rows)
    out = {k: np.zeros((len(rows), m), dtype=np.int32 if k == "common" else np.int64) for k in keys}
    memo: dict = {}
    for i, a in enumerate(rows):
        for b in range(m):
            if (b, a) in memo:
                vals = [memo[(b, a)][x] for x in swap]
            else:
                vals = memo[(a, b)] = cell(a, b)
            for k, v in zip(keys, vals):
                out[k][i, b] = v
    return out


# ------------------------------------------------------------------------------------------------ pair triplets
SMALL_NEIGHBOURS = (2, 3, 33, 64)


@lru_cache(maxsize=None)
def composed_pair(n: int, seed: int, kinds: int = 24, lo: int = 5, hi: int = 60) -> dict:
    """Two composed trees of exactly n leaves on the same n taxa: blocks of ``kinds`` shape pairs (two different random
    trees on the same lo .. hi labels, polytomies among them) in turn, a last block of what is left, two different
    random top trees.  ``cells``: the terms of (A, B), (A, A) and (B, B) by ``pair_composed``, the inside of a block
    judged once per shape pair by ``pair_quadratic``."""
    rng = random.Random(seed)

    def shape(s):
        if s == 1:
            return 1, 0, 0
        return s, *(pr.rand_tree(range(s), rng.choice([2, 3, 5]), rng) for _ in range(2))

    shapes = [shape(rng.randint(lo, hi)) for _ in range(kinds)]
    picks, left = [], n
    while left > 0:
        kind = len(picks) % kinds
        if shapes[kind][0] > left:
            shapes.append(shape(left))
            kind = len(shapes) - 1
        picks.append(kind)
        left -= shapes[kind][0]
    k = len(picks)
    assert k >= 3
    lab = list(range(n))
    rng.shuffle(lab)
    subs_a, subs_b, kind_of, at = [], [], {}, 0
    for kind in picks:
        s, a, b = shapes[kind]
        to = lab[at:at + s]
        at += s
        subs_a.append(relabel(a, to))
        subs_b.append(relabel(b, to))
        kind_of[id(subs_a[-1])] = (kind, 1)
        kind_of[id(subs_b[-1])] = (kind, 2)
    top_a, top_b = pr.rand_tree(range(k), 3, rng), pr.rand_tree(range(k), 4, rng)
    memo: dict = {}

    def inside(x, y):
        (kx, sx), (ky, sy) = kind_of[id(x)], kind_of[id(y)]
        assert kx == ky
        if (kx, sx, sy) not in memo:
            memo[(kx, sx, sy)] = st.pair_quadratic(shapes[kx][sx], shapes[kx][sy])
        return memo[(kx, sx, sy)]

    cells = {"ab": pair_composed(top_a, subs_a, top_b, subs_b, inside),
             "aa": pair_composed(top_a, subs_a, top_a, subs_a, inside),
             "bb": pair_composed(top_b, subs_b, top_b, subs_b, inside)}
    return {"trees": [compose(top_a, subs_a), compose(top_b, subs_b)], "n": n, "blocks": k, "cells": cells}


@lru_cache(maxsize=None)
def zb_step_case(n: int, batched: bool) -> Case:
    """A composed pair of n leaves each, alone or in a batch with trees of 2, 3, 33 and 64 leaves (restrictions of
    either large tree with a leaf pair swapped, so that they agree with it on some triples only)."""
    pair = composed_pair(n, 4000 + n)
    a, b = pair["trees"]
    c = pair["cells"]
    if not batched:
        trees, known = [a, b], {(0, 0): c["aa"], (0, 1): c["ab"], (1, 1): c["bb"]}
    else:
        rng = random.Random(n)
        small = []
        for i, s in enumerate(SMALL_NEIGHBOURS):
            taxa = rng.sample(range(n), s)
            t = pr.restrict((a, b)[i % 2], set(taxa))
            swap = dict(zip(taxa[:2], taxa[1::-1]))
            small.append(relabel(t, {x: swap.get(x, x) for x in taxa}))
        trees = [a, small[0], small[1], b, small[2], small[3]]
        known = {(0, 0): c["aa"], (0, 3): c["ab"], (3, 3): c["bb"]}
    leaves = [set(pr.leaves_of(t)) for t in trees]

    def cell(i, j):
        if (i, j) in known:
            return known[(i, j)]
        both = leaves[i] & leaves[j]
        if len(both) < 3:
            return len(both), 0, 0, 0
        return st.pair_quadratic(pr.restrict(trees[i], both), pr.restrict(trees[j], both))

    tables = tables_of([arrays_of(t) for t in trees], n)
    large = sorted({i for i, _ in known} | {j for _, j in known})
    return Case(tables, _cells(len(trees), None, cell), None, {"large": large})


@lru_cache(maxsize=None)
def contracted_case(n_common: int, extra: int = 40, small: int = 33, rows=(1,), seed: int = 0) -> Case:
    """Trees [A, B, s] of one family: A on ``n_common + extra`` positions, B = A with a third of its inner nodes
    contracted and restricted to ``n_common`` of them, s = A restricted to ``small`` positions of B.  Every cell of the
    rows by ``pair_contracted``."""
    seed = seed or n_common
    fam = random_family(n_common + extra, seed)
    rs = np.random.RandomState(seed + 2)
    mask_b = np.ones(fam.n, dtype=bool)
    mask_b[rs.choice(fam.n, extra, replace=False)] = False
    mask_s = np.zeros(fam.n, dtype=bool)
    mask_s[rs.choice(np.flatnonzero(mask_b), small, replace=False)] = True
    members = [(None, None), (contraction(fam, seed + 1), mask_b), (None, mask_s)]
    tables = tables_of([member(fam, *m) for m in members], fam.n)
    rows = None if rows is None else list(rows)
    ref = _cells(3, rows, lambda i, j: pair_contracted(fam, *members[i], *members[j]))
    return Case(tables, ref, rows, {"sizes": np.diff(tables.tree_off).tolist()})


def triplet_plan(case: Case, **kw) -> dict:
    return backend.debug_source_pair_triplets_plan(case.tables.tree_off, int(case.tables.n_taxa), case.rows, **kw)


def pair_side(n_a: int, n_b: int, lds_restrict: int) -> bool:
    """True: k_st_restrict keeps the pair's arrays in the launch's LDS; False: in the pair's region."""
    return st.work_bytes(n_a, n_b) + st.ST_SCRATCH <= lds_restrict


@lru_cache(maxsize=None)
def few_common_case() -> Case:
    """Trees of 300 leaves (so that sweep workgroups are counted for every pair) that share 0, 1, 2 and 65 taxa with
    the row tree, after two pairs that fill a region's lists: with one pair a chunk every pair reuses region 0."""
    rng = random.Random(65)
    n, m = 300, 300
    a = pr.rand_tree(range(m), 3, rng)
    full = pr.rand_tree(range(m), 2, rng)
    others = [pr.rand_tree([*rng.sample(range(m), share), *range(n + i * m, n + (i + 1) * m - share)], 3, rng)
              for i, share in enumerate((0, 1, 2, 65))]
    trees = [a, full, *others]
    return Case(pr.tables(trees, n + 4 * m), st.quadratic(trees, [0]), [0], {"trees": trees})


@lru_cache(maxsize=None)
def b_nodes_case(k: int) -> Case:
    """``test_b_node_counts_around_the_block_of_a_sweep_workgroup``'s pair: B has k nodes below its root."""
    c, n = 100, 110
    rng = random.Random(k)
    a = pr.rand_tree(range(n), 3, rng)
    order = rng.sample(range(c), c)
    b = [pr.caterpillar(order[: k + 1]), *order[k + 1:]]
    return Case(pr.tables([a, b], n), st.quadratic([a, b]), None, {"k": k})


# ------------------------------------------------------------------------------------------------ source pairs
@lru_cache(maxsize=None)
def overlap_case(n_a: int, c: int, own: int = 0, seed: int = 0) -> Case:
    """Trees [A, B, C]: A a random tree of n_a leaves; B = A contracted and restricted to c of its positions, beside
    ``own`` taxa of its own; C another random tree on those c taxa.  ``source_pairs_reference.linear`` judges."""
    seed = seed or 7 * n_a + c
    fam = random_family(n_a, seed)
    rs = np.random.RandomState(seed + 2)
    mask = np.zeros(n_a, dtype=bool)
    mask[rs.choice(n_a, c, replace=False)] = True
    b = member(fam, contraction(fam, seed + 1), mask)
    if own:
        b = join([b, member(random_family(own, seed + 3, taxa=np.arange(n_a, n_a + own)))])
    other = member(random_family(c, seed + 4, taxa=rs.permutation(fam.taxa[mask])))
    tables = tables_of([member(fam), b, other], n_a + own)
    return Case(tables, sp.linear(tables), None, {"sizes": np.diff(tables.tree_off).tolist()})


def pairs_plan(case: Case, **kw) -> dict:
    n_rows = None if case.rows is None else len(case.rows)
    return backend.debug_source_pairs_plan(case.tables.tree_off, int(case.tables.n_taxa), n_rows, **kw)


SLAB_CAP = 256


@lru_cache(maxsize=None)
def slab_reuse_case() -> Case:
    """18 trees of 200, 20 and 150 leaves in turn -- large, small, large --, every row asked for: 324 pairs, of which
    every one takes a slab under ``SLAB_CAP`` bytes of LDS."""
    rng = random.Random(18)
    n = 260
    bases = [pr.rand_tree(range(n), 3, rng), pr.rand_tree(range(n), 2, rng)]  # (restrictions of two trees in turn)
    trees = []
    for i in range(18):
        taxa = set(rng.sample(range(n), (200, 20, 150)[i % 3]))
        trees.append(pr.restrict(bases[i % 2], taxa))
    tables = pr.tables(trees, n)
    rows = list(range(18))
    return Case(tables, sp.linear(tables, rows), rows, {"trees": trees})


@lru_cache(maxsize=None)
def whole_blocks_case() -> Case:
    """Trees on the same 704 taxa: A's root has clusters on the ranks [0, 64), [64, 192), [192, 384), [384, 448),
    [448, 640) and the loose rest -- one, two and three whole blocks of 64 --, each resolved at random; B holds the
    same clusters with other trees inside and in another order, C is a random tree.  D holds them too, and its first
    leaf of [192, 384) and its last of [448, 640) are the taxa at A's ranks 262 and 518: the least and the largest B
    position of those clusters belong to a leaf of their *middle* block of 64 ranks, alone under the cluster's root,
    so that without the block tables' term the B node above the extremes is one leaf short."""
    rng = random.Random(64)
    n = 704
    cuts = [0, 64, 192, 384, 448, 640]
    parts = [list(range(lo, hi)) for lo, hi in zip(cuts, cuts[1:])]
    a = [*(pr.rand_tree(p, 3, rng) for p in parts), *range(640, n)]
    b = [*range(640, n), *(pr.rand_tree(p, 2, rng) for p in reversed(parts))]
    order = pr.leaves_of(a)
    first, last = order[262], order[518]
    d = [[first, pr.rand_tree([x for x in parts[2] if x != first], 2, rng)], pr.rand_tree(parts[0] + parts[1], 3, rng),
         [pr.rand_tree([x for x in parts[4] if x != last], 2, rng), last], *parts[3], *range(640, n)]
    trees = [a, b, pr.rand_tree(range(n), 3, rng), d]
    tables = pr.tables(trees, n)
    return Case(tables, sp.linear(tables), None, {"trees": trees, "cuts": cuts})


@lru_cache(maxsize=None)
def width_case() -> Case:
    """A tree of 3 000 leaves and one of 65 536, a batch each: the tile of the first with itself has 16-bit list
    entries, the two others 32-bit ones."""
    fam = random_family(65536, 16)
    mask = np.zeros(fam.n, dtype=bool)
    mask[np.random.RandomState(3).choice(fam.n, 3000, replace=False)] = True
    tables = tables_of([member(fam, contraction(fam, 5), mask), member(fam)], fam.n)
    return Case(tables, sp.linear(tables), None, None)


# ------------------------------------------------------------------------------------------------ parsimony
def star_arrays(m: int) -> tuple[np.ndarray, np.ndarray]:
    """``(parent, taxon)`` of the star on taxa 0 .. m - 1."""
    parent = np.zeros(m + 1, dtype=np.int32)
    parent[0] = -1
    return parent, np.concatenate([[-1], np.arange(m)]).astype(np.int32)


def caterpillar_arrays(taxa) -> tuple[np.ndarray, np.ndarray]:
    """The left caterpillar ((((a, b), c), d), ...) as ``(leaf_taxon, gap depths)``."""
    m = len(taxa)
    return np.asarray(taxa, dtype=np.int32), np.arange(m - 2, -1, -1, dtype=np.int32)


def caterpillar_star_reference(m: int, chars: bool) -> dict:
    """The outputs for one left caterpillar of m leaves on a star: its clusters are the first s leaves, s = 2 .. m - 1,
    in that order."""
    s = np.arange(2, m, dtype=np.int64)
    length = np.minimum(s, m - s + 1)
    one = lambda v: np.array([v], dtype=np.int64)  # noqa: E731
    out = {"mrp_chars": one(m - 2), "mrp_length": one(length.sum()), "mrp_perfect": one((length == 1).sum()),
           "mrp_max": one(length.sum())}
    if chars:
        out.update(char_off=np.array([0, m - 2], dtype=np.int64), char_len=length.astype(np.int32),
                   char_lo=np.zeros(m - 2, dtype=np.int32), char_hi=(s - 1).astype(np.int32))
    return out


def smallest_caterpillar_past_32_bits() -> int:
    """The least m whose caterpillar's star length passes 2^32: the sum is about m^2 / 4."""
    def total(m):
        s = np.arange(2, m, dtype=np.int64)
        return int(np.minimum(s, m - s + 1).sum())

    lo, hi = 3, 1 << 20
    while lo < hi:
        mid = (lo + hi) // 2
        if total(mid) > 1 << 32:
            hi = mid
        else:
            lo = mid + 1
    assert total(lo) > 1 << 32 >= total(lo - 1)
    return lo


FRAME_STAR = 16384


@lru_cache(maxsize=None)
def frames_case(deep: int):
    """S = [a star of 16 384 tips, a balanced subtree of ``deep`` tips]: 15 counter slices, and log2(deep) + 1 frames.
    Sources that mix tips of both parts, one on the whole balanced part, one caterpillar over some of everything."""
    rng = random.Random(deep)
    n = FRAME_STAR + deep
    parent, taxon = pr.preorder_arrays([list(range(FRAME_STAR)), balanced(range(FRAME_STAR, n))])
    trees = [pr.rand_tree(rng.sample(range(FRAME_STAR), 20) + rng.sample(range(FRAME_STAR, n), 40), 3, rng)
             for _ in range(3)]
    trees.append(pr.rand_tree(range(FRAME_STAR, n), 2, rng))
    trees.append(pr.caterpillar(rng.sample(range(FRAME_STAR), 90) + rng.sample(range(FRAME_STAR, n), deep // 2)))
    return parent, taxon, trees, n, pr.reference(parent, taxon, trees)


@lru_cache(maxsize=None)
def arity_case(arity: int):
    """``test_one_supertree_node_of_that_many_children``'s supertree: one node of ``arity`` children."""
    rng = random.Random(arity)
    n = 4 * arity + 6
    wide = [pr.rand_tree(range(4 * i, 4 * i + 4), 2, rng) for i in range(arity)]
    parent, taxon = pr.preorder_arrays([[wide, [n - 6, n - 5]], [[n - 4, n - 3], [n - 2, n - 1]]])
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(3, n)), 4, rng) for _ in range(8)]
    return parent, taxon, trees, n, pr.reference(parent, taxon, trees)


LIST_SIZES = (3, 1, 4, 2, 5, 257, 1, 258, 2, 513, 514)


@lru_cache(maxsize=None)
def list_rounds_case():
    """Sources of 3, 4, 5, 257, 258, 513 and 514 leaves -- the segments of k_mp_scan, rounds of 256 gaps of k_mp_list
    and one more -- with one- and two-leaf trees between, on a random supertree of 520 tips."""
    rng = random.Random(257)
    n = 520
    parent, taxon = pr.preorder_arrays(pr.rand_tree(range(n), 4, rng))
    trees = []
    for i, s in enumerate(LIST_SIZES):
        taxa = rng.sample(range(n), s)
        t = pr.caterpillar(taxa, i % 2 == 0) if s > 5 and i % 3 == 0 else pr.rand_tree(taxa, 2 if i % 2 else 3, rng)
        trees.append(t[0] if s == 1 else t)
    return parent, taxon, trees, n, pr.reference(parent, taxon, trees)


# ------------------------------------------------------------------------------------------------ coverage
CORE_TREES = 8


@lru_cache(maxsize=None)
def compact_case(nc: int, fillers: int = 0):
    """``CORE_TREES`` trees over n = nc + 40 taxa of which nc lie in two to four trees and 40 in one tree each (20 of
    them the first ids, 20 spread), so that at k = 2 the walk is over nc compact taxa whose index is not their id;
    the two last compact taxa share trees 0 and 1.  ``fillers`` one-leaf trees on the first compact taxon come first:
    they change its ``occurs`` and nothing else, and push the core trees' bits to the words past them.  Returns
    (sets, n, rows, {k: reference}) with the rows all taxa."""
    rng = random.Random(nc)
    n = nc + 40
    single = set(range(20)) | set(rng.sample(range(20, n - 2), 20))
    compact = [x for x in range(n) if x not in single]
    core = [[] for _ in range(CORE_TREES)]
    for x in range(n):
        held = [rng.randrange(CORE_TREES)] if x in single else rng.sample(range(CORE_TREES), rng.randint(2, 4))
        if x >= n - 2:
            held = sorted({0, 1, *held})
        for t in held:
            core[t].append(x)
    refs = {}
    for k in (1, 2):
        ref = coverage_by_signatures(core, n, k)
        ref["occurs"][compact[0]] += fillers
        ref["pair_trees"][compact[0], compact[0]] += fillers
        refs[k] = ref
    sets = [[compact[0]]] * fillers + core
    return sets, n, compact, refs


@lru_cache(maxsize=None)
def tree_count_case(n_trees: int):
    """``n_trees`` random trees of 2 .. 9 of the first 67 taxa; the last tree also holds the three taxa no other tree
    holds."""
    rng = random.Random(n_trees)
    n = 70
    sets = cr.random_sets(rng, n - 3, n_trees, 2, 9)
    sets[-1] = sorted({*sets[-1], n - 3, n - 2, n - 1})
    return sets, n


def smallest_taxa_past_32_bits() -> int:
    n = 3
    while comb(n - 1, 2) <= 1 << 32:
        n += max(1, int(((1 << 33) ** 0.5 - n) // 2))
    while comb(n - 2, 2) > 1 << 32:
        n -= 1
    assert comb(n - 1, 2) > 1 << 32 >= comb(n - 2, 2)
    return n
