"""Builders, closed forms and the host plan for the edges of the four base scoring exports (``csrc/scs_score.hip``:
``scs_score_supertree``, ``scs_score_triplets``, ``scs_score_conflicts``, ``scs_score_concordance``; the cases of
``tests/test_gpu_score_edges.py``, held to their numbers by ``tests/test_score_edge_reference_cpu.py``).  CPU only.

The references stay the project's own -- ``score_reference``, ``triplet_reference``, ``conflict_reference``,
``concordance_reference`` --, and the source forests come from ``build_reference.forest``.  What is here:

* the supertree as preorder ``parent`` / ``taxon`` arrays of a stated shape (``random``, ``balanced``, ``caterpillar``,
  ``star`` as in ``build_reference.shape``, and ``mixed``: binary in places, polytomies in places, unary nodes), with
  unary chains that set the node count independently of the leaf count, and the way back to ``TreeNode`` objects;
* ``reference``: all four exports' results from the existing references, brute force where the case is tiny;
* closed forms where the references cannot go: two caterpillars under a permutation (every triple resolved, the
  outgroup the taxon of largest rank: ``t_shared`` is a dominance count, the shared clusters are the common prefix
  sets), and three-leaf sources on a caterpillar supertree;
* the host plan of ``sc_begin`` and ``scs_score_triplets`` restated: ``levels``, ``row_stride``, ``per_tree``, the
  batch starts, and ``words`` / ``zb`` / workgroups per batch -- compared with ``scs_debug_score_plan``;
* the cases, each a function of its name.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache
from math import comb

import build_reference as br
import concordance_reference as qr
import conflict_reference as cr
import numpy as np
import score_reference as sr
import triplet_reference as tr

from spectralclustersupertree_amd.tree import TreeNode
from spectralclustersupertree_amd.treearrays import TreeArrays

# ---- the constants of csrc/scs_score.hip the cases are placed by
SC_THREADS = 256  # threads per workgroup: one thread per leaf of the batch
SC_ROW_ALIGN = 1024  # row stride, and the S positions one step of k_score_compact takes
SC_PREFIX_CHUNK = 1024  # S nodes one step of k_score_prefix takes
SC_BUDGET = 3 << 29  # workspace bytes per batch
TP_ZMAX = 8  # S' nodes per workgroup of k_trip_pairs at most
TP_LDS_BUDGET = 40 << 10  # LDS bytes a workgroup of k_trip_pairs aims at
TP_LDS_MAX = 160 << 10  # ... and may take for one S' node
LDS_CAP = TP_LDS_MAX // 16 * 32 - 1  # 327 679: the largest source tree scs_score_triplets takes

RF = ("n_super", "n_source", "shared", "informative", "supported")
TRIPLETS = ("t_super", "t_source", "t_shared")
CONFLICTS = ("n_super_conflict", "n_source_conflict", "conflicting")
CONCORDANCE = (*qr.PER_TREE, *qr.PER_NODE)
EXPORTS = {"score": RF, "score_triplets": TRIPLETS, "score_conflicts": CONFLICTS, "score_concordance": CONCORDANCE}
PER_NODE = ("informative", "supported", "conflicting", *qr.PER_NODE)


# ------------------------------------------------------------------------------------------------ the host plan
def levels_of(n: int) -> int:
    """``sc_levels_host``: 2^levels > n."""
    lv = 1
    while (1 << lv) <= n:
        lv += 1
    return lv


def export_extras(export: str, levels: int) -> tuple[int, int]:
    """``(extra_per_leaf, extra_per_tree)`` the export hands to ``sc_begin``."""
    return {"score": (0, 0), "score_concordance": (0, 0), "score_triplets": (32, 8),
            "score_conflicts": (8 * levels + 8, 0)}[export]


def per_tree(n: int, row_stride: int, levels: int, extra_per_leaf: int = 0, extra_per_tree: int = 0) -> int:
    return row_stride * 4 + n * (4 * 3 + 8 * levels + 4 * (levels - 1) + extra_per_leaf) + extra_per_tree


def words_zb(n_max: int) -> tuple[int, int]:
    words = (n_max >> 5) + 1
    return words, min(TP_ZMAX, max(1, TP_LDS_BUDGET // (16 * words)))


def plan(tree_off, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0, extra_per_tree: int = 0) -> dict:
    """What ``backend.debug_score_plan`` returns, restated."""
    off = [int(x) for x in tree_off]
    m = len(off) - 1
    sizes = [off[t + 1] - off[t] for t in range(m)]
    row_stride = br.round_up(max(super_leaves, 1), SC_ROW_ALIGN)
    levels = levels_of(max(max(sizes, default=0), 1))
    bstart, acc = [0], 0
    for t in range(m):
        need = per_tree(sizes[t], row_stride, levels, extra_per_leaf, extra_per_tree)
        nb = t - bstart[-1]
        if nb > 0 and (acc + need > SC_BUDGET or (batch_trees > 0 and nb >= batch_trees)):
            bstart.append(t)
            acc = 0
        acc += need
    bstart.append(m)
    words, zb, wg = [], [], []
    for b in range(len(bstart) - 1):
        mine = sizes[bstart[b]:bstart[b + 1]]
        w, z = words_zb(max(mine, default=0))
        words.append(w)
        zb.append(z)
        wg.append(sum((max(n - 2, 0) + z - 1) // z for n in mine))
    as64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    return {"bstart": as64(bstart), "levels": levels, "row_stride": row_stride, "words": as64(words), "zb": as64(zb),
            "workgroups": as64(wg)}


def export_plan(export: str, tree_off, super_leaves: int, batch_trees: int = 0) -> dict:
    sizes = np.diff(np.asarray(tree_off, dtype=np.int64))
    epl, ept = export_extras(export, levels_of(max(int(sizes.max(initial=0)), 1)))
    return plan(tree_off, super_leaves, batch_trees, epl, ept)


# ------------------------------------------------------------------------------------------------ supertrees
def mixed_shape(k: int, rng: np.random.RandomState, polytomy: float = 0.35, unary: float = 0.08):
    """``(parent, is_leaf)`` in preorder of a tree of ``k`` leaves with binary nodes, polytomies (a node takes one
    more child with probability ``polytomy``, again and again) and unary nodes (probability ``unary`` above a node)."""
    parent, leaf = [], []
    stack = [(k, -1, True)]
    while stack:
        n, p, may_unary = stack.pop()
        at = len(parent)
        parent.append(p)
        if n == 1:
            leaf.append(True)
            continue
        leaf.append(False)
        if may_unary and rng.rand() < unary:
            stack.append((n, at, False))
            continue
        c = 2
        while c < n and rng.rand() < polytomy:
            c += 1
        cuts = np.sort(rng.permutation(np.arange(1, n))[: c - 1])
        parts = np.diff(np.concatenate([[0], cuts, [n]]))
        for part in parts[::-1]:
            stack.append((int(part), at, True))
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def insert_unary(parent: np.ndarray, leaf: np.ndarray, at: int, count: int):
    """A chain of ``count`` unary nodes above preorder node ``at`` (which may be the root)."""
    if count == 0:
        return parent, leaf
    old = np.arange(len(parent))
    shifted = np.where(parent >= at, parent + count, parent)
    shifted[at] = at + count - 1
    chain = np.concatenate([[parent[at]], np.arange(at, at + count - 1)])
    new_parent = np.concatenate([shifted[old < at], chain, shifted[old >= at]]).astype(np.int32)
    new_leaf = np.concatenate([leaf[:at], np.zeros(count, dtype=bool), leaf[at:]])
    return new_parent, new_leaf


def supertree(kind: str, order, seed: int = 0, nodes: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """``(parent, taxon)`` of a supertree of shape ``kind`` whose tips in preorder carry the ids ``order``; with
    ``nodes`` unary chains -- a third of them above the root, the rest above a node in the middle -- bring the node
    count to exactly that."""
    order = np.asarray(order, dtype=np.int32)
    rng = np.random.RandomState(seed)
    par, leaf = mixed_shape(len(order), rng) if kind == "mixed" else br.shape(kind, len(order), rng)
    if nodes is not None:
        extra = nodes - len(par)
        assert extra >= 0, (kind, len(order), nodes, len(par))
        par, leaf = insert_unary(par, leaf, len(par) // 2, extra - extra // 3)
        par, leaf = insert_unary(par, leaf, 0, extra // 3)
        assert len(par) == nodes
    taxon = np.full(len(par), -1, dtype=np.int32)
    taxon[leaf] = order
    return par, taxon


def names(n: int) -> list[str]:
    return br.taxon_names(n)


def to_node(parent: np.ndarray, taxon: np.ndarray) -> TreeNode:
    """The supertree as ``TreeNode`` objects, nodes in the arrays' order (``TreeNode.to_flat`` gives it back)."""
    nm = names(int(taxon.max()) + 1)
    flat = ([int(p) for p in parent], [nm[x] if x >= 0 else None for x in taxon], [None] * len(parent),
            [None] * len(parent))
    return TreeNode.from_flat(flat)


def source_nodes(arrays: TreeArrays) -> list[TreeNode]:
    return [arrays.to_tree(t) for t in range(arrays.n_trees)]


def leaf_ranges(parent: np.ndarray, taxon: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """First and last S position below every node."""
    n = len(parent)
    lo, hi = np.full(n, n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    tip = taxon >= 0
    lo[tip] = hi[tip] = np.arange(int(tip.sum()))
    for v in range(n - 1, 0, -1):
        u = parent[v]
        lo[u], hi[u] = min(lo[u], lo[v]), max(hi[u], hi[v])
    return lo, hi


def s_positions(taxon: np.ndarray, n_taxa: int) -> np.ndarray:
    """S position of every taxon id below ``n_taxa`` (-1: not in S)."""
    tips = taxon[taxon >= 0]
    pos = np.full(n_taxa, -1, dtype=np.int64)
    keep = tips < n_taxa
    pos[tips[keep]] = np.flatnonzero(keep)
    return pos


# ------------------------------------------------------------------------------------------------ references
def reference(parent: np.ndarray, taxon: np.ndarray, arrays: TreeArrays, exports=tuple(EXPORTS)) -> dict:
    """The results of ``exports`` from the project's references: brute force over sets when the supertree and
    every source have at most 12 leaves, ``linear`` / ``quadratic`` otherwise (concordance has brute force only)."""
    sup, trees = to_node(parent, taxon), source_nodes(arrays)
    tiny = int((taxon >= 0).sum()) <= 12 and int(arrays.leaf_counts().max()) <= 12
    out: dict = {}
    if "score" in exports:
        out.update((sr.brute_force if tiny else sr.linear)(sup, trees))
    if "score_triplets" in exports:
        out.update((tr.brute_force if tiny else tr.quadratic)(sup, trees))
    if "score_conflicts" in exports:
        out.update((cr.brute_force if tiny else cr.quadratic)(sup, trees))
    if "score_concordance" in exports:
        out.update(qr.brute_force(sup, trees))
    return {k: np.asarray(out[k], dtype=np.int64) for e in exports for k in EXPORTS[e]}


def dominance(a: np.ndarray) -> np.ndarray:
    """``dom[i] = #{j < i : a[j] < a[i]}`` for distinct ``a``, by a bottom-up merge in numpy (O(m log^2 m))."""
    m = len(a)
    size = 1
    while size < m:
        size *= 2
    rank = np.empty(m, dtype=np.int64)
    rank[np.argsort(a, kind="stable")] = np.arange(m)
    val = np.concatenate([rank, np.arange(m, size)]).astype(np.int64)  # (the padding is larger than every value)
    idx = np.arange(size)
    dom = np.zeros(size, dtype=np.int64)
    w = 1
    while w < size:
        v, ix = val.reshape(-1, 2, w), idx.reshape(-1, 2, w)
        nb = v.shape[0]
        base = (np.arange(nb, dtype=np.int64) * size)[:, None]  # keeps the pairs of blocks apart in one sorted row
        left = (v[:, 0, :] + base).ravel()
        below = np.searchsorted(left, (v[:, 1, :] + base).ravel()).reshape(nb, w) - (np.arange(nb) * w)[:, None]
        dom[ix[:, 1, :].ravel()] += below.ravel()
        both, bi = v.reshape(nb, 2 * w), ix.reshape(nb, 2 * w)
        o = np.argsort(both, axis=1, kind="stable")
        val, idx = np.take_along_axis(both, o, 1).ravel(), np.take_along_axis(bi, o, 1).ravel()
        w *= 2
    return dom[:m]


def comb_pair(s_order, t_order, n_taxa: int) -> dict:
    """Closed forms for S = ``supertree("caterpillar", s_order)`` against the one source
    ``("caterpillar", t_order)`` on the same m >= 3 taxa.  A caterpillar's clusters are the prefixes of its leaf order
    (``build_reference.shape`` lists the leaves deepest first), so every triple is resolved and its outgroup is the
    taxon latest in the order.  With a[i] the T position of the taxon at S position i:

    * ``t_super = t_source = C(m, 3)``; a triple is shared iff one taxon c is last in both orders, so
      ``t_shared = sum_c C(dom(c), 2)``, dom(c) = #{x : x before c in S and in T};
    * ``n_super = n_source = m - 2`` (prefixes of 2 .. m - 1 leaves); the prefix of k leaves is shared iff
      max(a[:k]) = k - 1; a prefix set of one comb is compatible with the other's chain of prefix sets only if it
      is one of them, so both conflict counts are ``m - 2 - shared``;
    * S's inner node j (preorder: the path first) holds the first m - j leaves: informative once for 1 <= j <= m - 2,
      supported or conflicting by its prefix."""
    s_order, t_order = np.asarray(s_order, dtype=np.int64), np.asarray(t_order, dtype=np.int64)
    m = len(s_order)
    assert m >= 3 and len(t_order) == m
    t_pos = np.full(n_taxa, -1, dtype=np.int64)
    t_pos[t_order] = np.arange(m)
    a = t_pos[s_order]
    assert (a >= 0).all()
    dom = dominance(a)
    same = np.maximum.accumulate(a)[1:m - 1] == np.arange(1, m - 1)  # prefixes of k = 2 .. m - 1 leaves
    shared = int(same.sum())
    one = lambda x: np.asarray([x], dtype=np.int64)  # noqa: E731
    informative = np.zeros(2 * m - 1, dtype=np.int64)
    supported = np.zeros(2 * m - 1, dtype=np.int64)
    informative[1:m - 1] = 1
    supported[1:m - 1] = same[::-1]
    return {"t_super": one(comb(m, 3)), "t_source": one(comb(m, 3)), "t_shared": one(int((dom * (dom - 1) // 2).sum())),
            "n_super": one(m - 2), "n_source": one(m - 2), "shared": one(shared), "informative": informative,
            "supported": supported, "n_super_conflict": one(m - 2 - shared), "n_source_conflict": one(m - 2 - shared),
            "conflicting": informative - supported}


def permutation(kind: str, m: int, seed: int = 0) -> np.ndarray:
    """A leaf order of m taxa to hold against the identity: ``random``; ``blocks`` (consecutive blocks of 1 .. 96
    taxa, each reversed or shuffled: the prefixes agree at every block's end); ``interleave`` (the even positions,
    then the odd ones)."""
    rng = np.random.RandomState(seed)
    ids = np.arange(m, dtype=np.int32)
    if kind == "random":
        return ids[rng.permutation(m)]
    if kind == "interleave":
        return np.concatenate([ids[0::2], ids[1::2]])
    assert kind == "blocks"
    out, at = [], 0
    while at < m:
        w = min(int(rng.randint(1, 97)), m - at)
        blk = ids[at:at + w]
        out.append(blk[::-1] if rng.rand() < 0.5 else blk[rng.permutation(w)])
        at += w
    return np.concatenate(out)


def three_leaf_closed_form(s_order, trees, n_taxa: int) -> dict:
    """Closed forms for S = ``supertree("caterpillar", s_order)`` (m leaves) against three-leaf sources
    ``(kind, order)``, kind ``caterpillar`` ((a, b), c) or ``balanced`` (a, (b, c)).  With p0 < p1 < p2 the S positions
    of a source's taxa, S restricted to them is ((p0, p1), p2): one cluster and one triple each way, shared iff the
    source's cherry is {p0, p1}, in conflict otherwise.  S's inner node j holds the positions below k = m - j, so its
    restricted set is {p0, p1} for p1 < k <= p2.  Node j (1 <= j <= m - 2) is a quartet branch with A = the positions
    below k - 1, B = {k - 1}, D = {k}: the source is decisive for it iff p1 = k - 1 and p2 = k, and then concordant,
    alt1 (A and D together) or alt2 (B and D together) by its cherry."""
    s_order = np.asarray(s_order, dtype=np.int64)
    m, n_trees = len(s_order), len(trees)
    s_pos = np.full(n_taxa, -1, dtype=np.int64)
    s_pos[s_order] = np.arange(m)
    pos = np.asarray([s_pos[np.asarray(o, dtype=np.int64)] for _, o in trees], dtype=np.int64).reshape(n_trees, 3)
    assert (pos >= 0).all() and all(k in ("caterpillar", "balanced") for k, _ in trees)
    first = np.asarray([k == "caterpillar" for k, _ in trees])
    out_of = np.where(first, pos[:, 2], pos[:, 0])  # the source's outgroup
    p = np.sort(pos, axis=1)
    share = out_of == p[:, 2]
    ones = np.ones(n_trees, dtype=np.int64)
    res = {"n_super": ones, "n_source": ones, "shared": share.astype(np.int64), "t_super": ones, "t_source": ones,
           "t_shared": share.astype(np.int64), "n_super_conflict": (~share).astype(np.int64),
           "n_source_conflict": (~share).astype(np.int64)}
    n_nodes = 2 * m - 1

    def over_nodes(lo_k, hi_k, weight):  # += weight at the inner nodes j = m - k for lo_k <= k <= hi_k
        d = np.zeros(n_nodes + 1, dtype=np.int64)
        np.add.at(d, m - hi_k, weight)
        np.add.at(d, m - lo_k + 1, -weight)
        return np.cumsum(d)[:n_nodes]

    res["informative"] = over_nodes(p[:, 1] + 1, p[:, 2], ones)
    res["supported"] = over_nodes(p[:, 1] + 1, p[:, 2], share.astype(np.int64))
    res["conflicting"] = res["informative"] - res["supported"]
    dec = p[:, 2] == p[:, 1] + 1
    alt1, alt2 = dec & (out_of == p[:, 1]), dec & (out_of == p[:, 0])
    res["n_decisive"] = dec.astype(np.int64)
    res["n_concordant"] = (dec & share).astype(np.int64)
    res["n_alternative"] = (alt1 | alt2).astype(np.int64)
    for key, mask in (("decisive", dec), ("concordant", dec & share), ("alt1", alt1), ("alt2", alt2)):
        per = np.zeros(n_nodes, dtype=np.int64)
        np.add.at(per, (m - p[:, 2])[mask], 1)
        res[key] = per
    return res


# ------------------------------------------------------------------------------------------------ the cases
@dataclass
class Case:
    """One supertree and one forest; ``batches``: the ``batch_trees`` values the case runs with."""
    name: str
    parent: np.ndarray
    taxon: np.ndarray
    arrays: TreeArrays
    batches: tuple = (0,)
    note: dict = field(default_factory=dict)

    @property
    def s_leaves(self) -> int:
        return int((self.taxon >= 0).sum())

    @property
    def sizes(self) -> np.ndarray:
        return np.asarray(self.arrays.leaf_counts(), dtype=np.int64)

    def tables(self):
        return self.arrays.flatten("one")


def _ids(n: int) -> np.ndarray:
    return np.arange(n, dtype=np.int32)


def _tree(rng, kind: str, pool, k: int):
    return (kind, br.order_random(rng, pool, k))


# ---- tree boundaries in waves.  One thread per leaf of the batch: the first leaf of tree t sits at thread
# off[t] - off[first tree of the batch].  The sizes put boundaries on lane 0 (64, 128), lane 63 (127) and a workgroup's
# first thread (256, 512, ...), one- and two-leaf trees first, last and between large ones.
WAVE_TAXA = 300
WAVE_SIZES = (1, 2, 61, 63, 1, 128, 3, 64, 65, 124, 127, 129, 255, 1, 256, 2, 257, 2, 1)
WAVE_ENDS = (255, 0, 1)  # the batch's leaves mod 256


def wave_case(end: int) -> Case:
    """The trees of WAVE_SIZES and, before the last two, one more that brings the leaves of all of them to ``end``
    mod 256 (255, 0 or 1), against a mixed supertree with 11 taxa no source has; shapes in turn."""
    rng = np.random.RandomState(41)
    sizes = (*WAVE_SIZES[:-2], (end - sum(WAVE_SIZES)) % 256 or 256, *WAVE_SIZES[-2:])
    kinds = ("random", "caterpillar", "star", "balanced")
    trees = [_tree(rng, kinds[i % 4], _ids(WAVE_TAXA), k) for i, k in enumerate(sizes)]
    parent, taxon = supertree("mixed", rng.permutation(WAVE_TAXA + 11), seed=end + 1)
    m = len(sizes)
    return Case(f"wave_end_{end}", parent, taxon, br.forest(41, WAVE_TAXA, trees), batches=(0, 1, 2, m - 1, m, m + 1))


# ---- levels.  2^levels > the call's largest tree; the descents' widest step must cover any stretch.  A star or a
# caterpillar of n leaves has a stretch of n - 2 gaps: at 2^k and 2^k + 1 leaves the new top level (2^k) is built but no
# descent needs it yet, 2^k + 2 is the first size where one does.
LEVEL_SIZES = (3, 4, 5, 6, 63, 64, 65, 66, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050)
LEVEL_SHAPES = ("star", "caterpillar", "random")
LEVEL_SMALL = 24  # three-leaf trees around the large one


def level_case(size: int, kind: str, among: bool) -> Case:
    """One tree of ``size`` leaves, alone or in the middle of LEVEL_SMALL three-leaf trees, against a mixed supertree
    on ``size + 3`` taxa."""
    rng = np.random.RandomState(size * 7 + len(kind))
    n = size + 3
    small = [_tree(rng, "caterpillar" if i % 2 else "balanced", _ids(n), 3) for i in range(LEVEL_SMALL)] if among else []
    half = len(small) // 2
    trees = small[:half] + [_tree(rng, kind, _ids(n), size)] + small[half:]
    parent, taxon = supertree("mixed", rng.permutation(n), seed=size)
    return Case(f"level_{size}_{kind}_{'among' if among else 'alone'}", parent, taxon, br.forest(size, n, trees))


S_GAPS = (3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)


def s_gap_case(gaps: int, kind: str) -> Case:
    """A supertree of ``gaps + 1`` leaves, ``star`` (one stretch over every gap but the last), ``caterpillar`` or
    ``mixed``, against whole and partial sources of every shape."""
    rng = np.random.RandomState(gaps * 3 + len(kind))
    n = gaps + 1
    trees = [_tree(rng, "random", _ids(n), n), _tree(rng, "caterpillar", _ids(n), max(3, n // 2)),
             _tree(rng, "star", _ids(n), max(3, n - 1)), _tree(rng, "balanced", _ids(n), min(n, 40))]
    parent, taxon = supertree(kind, rng.permutation(n), seed=gaps)
    return Case(f"s_gaps_{gaps}_{kind}", parent, taxon, br.forest(gaps, n, trees))


# ---- compaction and prefix.  k_score_compact takes 1 024 S positions a step, k_score_prefix 1 024 S nodes.
CHUNK_COUNTS = (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049)
CHUNK_EXTRA = 5  # taxa of S no source has (ids below n_taxa) ...
CHUNK_FOREIGN = 3  # ... and ids from n_taxa on, which the sources' tables cannot name


def _chunk_sources(rng, taxon: np.ndarray, n_taxa: int, lone: np.ndarray):
    """Sources by S position: wholly below 1 024, wholly from 1 024 on, with taxa at 1 023 and 1 024, and all.  The
    caterpillars list their taxa in S's own order: their prefixes are clusters of S's leftmost path, so some clades
    are supported."""
    tips = taxon[taxon >= 0]
    ok = (tips < n_taxa) & ~np.isin(tips, lone)
    at = np.flatnonzero(ok)
    first, second = tips[at[at < SC_ROW_ALIGN]], tips[at[at >= SC_ROW_ALIGN]]
    trees = [_tree(rng, "random", first, len(first)), ("caterpillar", first)]
    if len(second) >= 1:
        trees += [_tree(rng, "random", second, len(second)), ("caterpillar", second)]
        edge = tips[[SC_ROW_ALIGN - 1, SC_ROW_ALIGN]]
        assert ok[[SC_ROW_ALIGN - 1, SC_ROW_ALIGN]].all()
        rest = np.setdiff1d(tips[at], edge)
        straddle = np.concatenate([edge, br.order_random(rng, rest, min(len(rest), 200))])
        trees.append(("random", straddle[rng.permutation(len(straddle))]))
        trees.append(_tree(rng, "balanced", tips[at], len(at)))
    return trees


def chunk_case(count: int, what: str) -> Case:
    """A mixed supertree with ``count`` leaves (``what`` = "leaves") or ``count`` nodes, reached through unary
    chains (``what`` = "nodes").  From 1 025 leaves on it has CHUNK_EXTRA taxa no source has and CHUNK_FOREIGN ids the
    sources' tables cannot name."""
    rng = np.random.RandomState(count * 2 + len(what))
    if what == "nodes":
        leaves = max(1, count // 3)
        order = rng.permutation(leaves)
        parent, taxon = supertree("mixed", order, seed=count, nodes=count)
        return Case(f"chunk_{count}_nodes", parent, taxon, br.forest(count, leaves, _chunk_sources(
            rng, taxon, leaves, np.empty(0, dtype=np.int32))))
    foreign = CHUNK_FOREIGN if count > SC_ROW_ALIGN else 0
    n_taxa = count - foreign
    order = [int(x) for x in rng.permutation(n_taxa)]
    for i, at in enumerate((3, 700, 1022)[:foreign]):  # (S positions 1 023 and 1 024 stay with the sources)
        order.insert(at, n_taxa + i)
    parent, taxon = supertree("mixed", order, seed=count)
    tips = taxon[taxon >= 0]
    pool = np.setdiff1d(_ids(n_taxa), tips[[SC_ROW_ALIGN - 1, SC_ROW_ALIGN]]) if foreign else _ids(n_taxa)
    lone = br.order_random(rng, pool, CHUNK_EXTRA) if foreign else np.empty(0, dtype=np.int32)
    return Case(f"chunk_{count}_leaves", parent, taxon, br.forest(count, n_taxa, _chunk_sources(rng, taxon, n_taxa, lone)),
                note={"lone": lone})


# ---- conflicts.  k_conf_scan: one workgroup per tree, 256 entries a step.
SCAN_SIZES = (255, 256, 257, 511, 512, 513)


def scan_case(size: int) -> Case:
    rng = np.random.RandomState(size)
    n = size + 2
    trees = [_tree(rng, "random", _ids(n), size), _tree(rng, "caterpillar", _ids(n), size),
             _tree(rng, "balanced", _ids(n), size)]
    parent, taxon = supertree("mixed", rng.permutation(n), seed=size)
    return Case(f"scan_{size}", parent, taxon, br.forest(size, n, trees))


# The galloping searches.  A "star" holds all leaves but its last in one polytomy K.  Against a caterpillar in the
# order that puts that one outside leaf at position `at`, every other leaf x is asked for the nearest leaf outside K
# on both sides: it lies |x - at| positions away on one side and is missing on the other -- every distance from 1 to
# max(at, n - 1 - at), the 2^j - 1, 2^j, 2^j + 1 among them up to the table's top level, at once.
GALLOP_N = 1030  # levels 11: the widest step is 1 024
GALLOP_AT = (0, 1, 515, GALLOP_N - 2, GALLOP_N - 1)


def gallop_case(at: int, star_is: str) -> Case:
    """``star_is`` "source": a star source against a caterpillar supertree; "super": the other way round.  The
    star's outside leaf is taxon 0; the caterpillar lists it at position ``at``."""
    n = GALLOP_N
    rng = np.random.RandomState(at + len(star_is))
    rest = 1 + rng.permutation(n - 1).astype(np.int32)
    comb_order = np.concatenate([rest[:at], [0], rest[at:]]).astype(np.int32)
    star_order = np.concatenate([1 + rng.permutation(n - 1), [0]]).astype(np.int32)  # (br.shape: the last leaf is outside)
    s_kind, s_order, t_kind, t_order = (("caterpillar", comb_order, "star", star_order) if star_is == "source"
                                        else ("star", star_order, "caterpillar", comb_order))
    parent, taxon = supertree(s_kind, s_order, seed=at)
    trees = [(t_kind, t_order), ("random", br.order_random(rng, _ids(n), 17))]
    return Case(f"gallop_{star_is}_{at}", parent, taxon, br.forest(at, n, trees))


# ---- concordance.  A binary supertree (every inner node but the root is a quartet branch, first and second
# children alike); sources planted on it so that every category occurs, with one- and two-leaf trees between them
# that move the sources' first threads through the lanes.
CONC_TAXA = 192
CONC_SEED = 5


@lru_cache(maxsize=None)
def concordance_case() -> Case:
    rs = np.random.RandomState(CONC_SEED)
    nm = names(CONC_TAXA)
    sup = sr.random_tree(rs, nm, binary=True)
    parents, node_names, _, _ = sup.to_flat()
    index = {x: i for i, x in enumerate(nm)}
    parent = np.asarray(parents, dtype=np.int32)
    taxon = np.asarray([index[x] if x else -1 for x in node_names], dtype=np.int32)
    tips = [x for x in node_names if x]
    trees: list[TreeNode] = []
    for i in range(20):
        frac = (1.0, 1.0, 0.7, 0.4)[i % 4]
        trees.append(qr.planted(rs, sup, nm, frac, int(rs.randint(0, 12)), 0.15 if i % 3 == 0 else 0.0))
        if i % 2 == 0:
            trees.append(_tiny(rs, tips, 1 + (i // 2) % 2))
    # a source that lacks the first and the last leaves of S, and one without a whole subtree D
    trees.append(sup.get_sub_tree(tips[7:-9]).copy())
    trees.append(sup.get_sub_tree(tips[:40] + tips[64:]).copy())
    # every category on lane 0 and on lane 63.  A source on all taxa runs branch c on the thread (its first leaf's
    # thread) + (S position of the last leaf of c's first child).  A copy of S is concordant and a star is "other"
    # on every lane; S with B or A exchanged for D at c is alt1 / alt2 there, behind a filler tree that moves c's
    # thread onto the lane
    trees.append(sup.copy())
    trees.append(TreeNode(None, [TreeNode(x) for x in tips]))
    _, hi = leaf_ranges(parent, taxon)
    first_kid = {}
    for v in range(len(parent) - 1, 0, -1):
        first_kid[int(parent[v])] = v
    inner = [v for v in range(1, len(parent)) if taxon[v] < 0]
    for n, (which, lane) in enumerate((w, ln) for w in ("alt1", "alt2") for ln in (0, 63)):
        c = inner[(len(inner) * (n + 1)) // 5]
        total = sum(len(list(t.iter_tips())) for t in trees)
        fill = (lane - total - int(hi[first_kid[c]])) % 64 or 64
        trees.append(TreeNode(None, [TreeNode(x) for x in tips[:fill]]) if fill > 1 else TreeNode(tips[0]))
        moved = sup.copy()
        node = sr._preorder(moved)[c]
        par = node.parent
        j, i = 1 - par.children.index(node), (1 if which == "alt1" else 0)
        node.children[i], par.children[j] = par.children[j], node.children[i]
        node.children[i].parent, par.children[j].parent = node, par
        trees.append(moved)
    arrays = TreeArrays.from_trees(trees, [1.0] * len(trees), nm)
    return Case("concordance", parent, taxon, arrays, batches=(0, 1, 5), note={"sup": sup, "trees": trees})


def _tiny(rs, tips, k: int) -> TreeNode:
    pick = [str(x) for x in rs.choice(tips, size=k, replace=False)]
    return TreeNode(pick[0]) if k == 1 else TreeNode(None, [TreeNode(x) for x in pick])


# ---- zb transitions of k_trip_pairs: W = (n >> 5) + 1 words, zb = min(8, 40 960 / (16 W)).
ZB_SMALL = (2, 3, 32, 33, 64)  # the other trees of the batch: their last leaf lies in word 0 or 1, n itself in 0, 1 or 2
ZB_QUADRATIC = (10239, 10240)  # zb 8 | 7, against triplet_reference.quadratic
ZB_COMB = (40959, 40960)  # zb 2 | 1, against the closed forms
LDS_COMB = (131071, 131072, LDS_CAP)  # dynamic LDS below and from 64 KiB on, and the advertised limit


def zb_small(rng, n_taxa: int):
    kinds = ("random", "caterpillar", "balanced", "star", "random")
    return [_tree(rng, kinds[i], _ids(n_taxa), k) for i, k in enumerate(ZB_SMALL)]


def zb_quadratic_case(size: int) -> Case:
    """A random tree of ``size`` leaves between the trees of ZB_SMALL against a mixed supertree rich in polytomies
    (about half as many inner nodes as a binary one: the reference's cost is nodes x leaves)."""
    rng = np.random.RandomState(size)
    small = zb_small(rng, size)
    trees = small[:3] + [_tree(rng, "random", _ids(size), size)] + small[3:]
    order = rng.permutation(size)
    par, leaf = mixed_shape(size, np.random.RandomState(size + 1), polytomy=0.6, unary=0.02)
    taxon = np.full(len(par), -1, dtype=np.int32)
    taxon[leaf] = order
    return Case(f"zb_{size}", par, taxon, br.forest(size, size, trees), note={"large": 3})


def comb_case(size: int, kind: str, with_small: bool = False) -> Case:
    """A caterpillar supertree in the identity order against a caterpillar source in the order
    ``permutation(kind, size)``, alone or between the trees of ZB_SMALL."""
    rng = np.random.RandomState(size)
    t_order = permutation(kind, size, seed=size)
    small = zb_small(rng, size) if with_small else []
    trees = small[:3] + [("caterpillar", t_order)] + small[3:]
    parent, taxon = supertree("caterpillar", _ids(size))
    return Case(f"comb_{size}_{kind}{'_batch' if with_small else ''}", parent, taxon,
                br.forest(size, size, trees, unit_weights=True), note={"large": len(small[:3]), "t_order": t_order})


def comb_case_reference(case: Case, exports=("score", "score_triplets", "score_conflicts")) -> dict:
    """The closed forms for the caterpillar, the project's references for the small trees around it."""
    at = case.note["large"]
    m = case.arrays.n_trees
    big = comb_pair(_ids(case.s_leaves), case.note["t_order"], case.arrays.n_taxa)
    keys = [k for e in exports for k in EXPORTS[e]]
    if m == 1:
        return {k: big[k] for k in keys}
    rest = [t for t in range(m) if t != at]
    small = reference(case.parent, case.taxon, subset(case.arrays, rest), exports)
    out = {}
    for k in keys:
        if k in PER_NODE:
            out[k] = big[k] + small[k]
        else:
            out[k] = np.insert(small[k], at, big[k][0])
    return out


def subset(arrays: TreeArrays, which) -> TreeArrays:
    """The trees ``which`` of ``arrays``, in that order."""
    lo, hi = arrays.node_off[:-1], arrays.node_off[1:]
    node_off = np.zeros(len(which) + 1, dtype=np.int64)
    np.cumsum([hi[t] - lo[t] for t in which], out=node_off[1:])
    cut = lambda a: np.concatenate([a[lo[t]:hi[t]] for t in which])  # noqa: E731
    return TreeArrays(n_taxa=arrays.n_taxa, node_off=node_off, parent=cut(arrays.parent), taxon=cut(arrays.taxon),
                      length=cut(arrays.length), support=cut(arrays.support),
                      weights=np.asarray(arrays.weights)[list(which)], taxa=arrays.taxa)


# ---- the byte budget: three-leaf sources on a caterpillar supertree of BUDGET_LEAVES leaves; the rows alone (4 bytes
# x row stride a tree) pass SC_BUDGET at about 4 011 trees.
BUDGET_LEAVES = 98 * 1024


def budget_first_split(export: str) -> int:
    """M*: the smallest count of three-leaf trees the plan splits in two batches."""
    row_stride = br.round_up(BUDGET_LEAVES, SC_ROW_ALIGN)
    epl, ept = export_extras(export, levels_of(3))
    return SC_BUDGET // per_tree(3, row_stride, levels_of(3), epl, ept) + 1


@lru_cache(maxsize=None)
def budget_trees(count: int, r: int = BUDGET_LEAVES, seed: int = 17):
    """``count`` three-leaf sources on ``r`` taxa (the first ``k`` of them are the first ``k`` of any larger count): a
    third with two taxa next to each other in the identity order, so that some are decisive."""
    rng = np.random.RandomState(seed)
    trees = []
    for i in range(count):
        if i % 3 == 0:
            p = int(rng.randint(1, r - 1))
            ids = [int(rng.randint(0, p)), p, p + 1]
        else:
            ids = [int(x) for x in rng.randint(0, r, size=3)]
            while len(set(ids)) < 3:
                ids = [int(x) for x in rng.randint(0, r, size=3)]
        order = np.asarray(ids, dtype=np.int32)[rng.permutation(3)]
        trees.append(("caterpillar" if rng.rand() < 0.5 else "balanced", order))
    return trees


def budget_tables(trees, r: int = BUDGET_LEAVES):
    """The flattened tables of three-leaf sources without the node arrays: ((a, b), c) has gap depths 1, 0 and
    (a, (b, c)) 0, 1 (the last entry of a tree is unused)."""
    from spectralclustersupertree_amd.flatten import TreeTables
    m = len(trees)
    leaf_taxon = np.concatenate([np.asarray(o, dtype=np.int32) for _, o in trees]) if m else np.empty(0, dtype=np.int32)
    adj = np.concatenate([[1, 0, 0] if k == "caterpillar" else [0, 1, 0] for k, _ in trees]).astype(np.int32)
    return TreeTables(n_taxa=r, tree_off=3 * np.arange(m + 1, dtype=np.int64), leaf_taxon=leaf_taxon, adj_depth=adj,
                      adj_val=np.ones(3 * m, dtype=np.float64), tree_w=np.ones(m, dtype=np.float64))


# ---- refusals
REFUSALS = {"range": "out of range", "missing": "a source tree has a taxon the supertree lacks",
            "twice": "a source tree has a taxon twice"}
REFUSAL_TREES, REFUSAL_BATCH = 9, 3  # three batches of three trees


def refusal_tables(kind: str, bad_tree: int):
    """Good tables of REFUSAL_TREES trees on 40 taxa (taxon 39 is not in the supertree and in no good tree) and the
    same with one leaf of tree ``bad_tree`` changed: to id 40 (``range``), to taxon 39 (``missing``) or to the
    tree's own first taxon (``twice``).  Returns ``(parent, taxon, good arrays, good tables, bad tables)``."""
    rng = np.random.RandomState(3)
    n = 40
    trees = [_tree(rng, ("random", "caterpillar", "star")[i % 3], _ids(n - 1), int(rng.randint(5, 30)))
             for i in range(REFUSAL_TREES)]
    arrays = br.forest(3, n, trees)
    parent, taxon = supertree("mixed", rng.permutation(n - 1), seed=3)
    good, bad = arrays.flatten("one"), arrays.flatten("one")
    at = int(bad.tree_off[bad_tree]) + 2
    bad.leaf_taxon[at] = {"range": n, "missing": n - 1, "twice": bad.leaf_taxon[int(bad.tree_off[bad_tree])]}[kind]
    return parent, taxon, arrays, good, bad
