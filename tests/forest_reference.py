"""Builders and plain references for the edges of the forest split, its scans and the level analysis
(``csrc/scs_forest.hip``; the cases of ``tests/test_gpu_forest_edges.py``, held to their numbers by
``tests/test_forest_reference_cpu.py``).  CPU only: numpy and plain Python.

The restriction itself has its reference already -- ``TreeArrays.split`` + ``flatten``, held against the tree-object
path by ``tests/test_treearrays.py`` (reference: src/sc_supertree/scs.py:411-455); nothing here restates it.  What is
here:

* forests of prescribed shape as preorder node arrays: exact tree counts ``M``, exact node totals ``N`` (a binary
  tree of k leaves has 2k - 1 nodes, one unary node makes 2k, one trifurcation 2k - 2), exact node totals per
  workgroup of the thread-per-tree kernels, combs of a given root-path length;
* ``scan_reference``: the exclusive scans by ``np.cumsum`` / ``np.maximum.accumulate`` in int64;
* ``analysis_reference``: components of "join consecutive leaves unless the gap is a root gap", labelled by smallest
  member (reference: scs.py:122 ``_get_graph_components``, :458-492), and per taxon the set of (tree, root side)
  it occurs in (reference: scs.py:302-316, the contraction relation);
* the constants of ``scs_forest.hip`` that the cases sit on, restated where a case depends on them.
"""

from __future__ import annotations

from collections.abc import Sequence

import numpy as np

from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.treearrays import TreeArrays

# ---- the constants of csrc/scs_forest.hip the cases are placed by
SCAN_BLOCK = 4096  # items per workgroup of k_scan_local; entry n of a row is the total
SCAN_RAW_MAX_BLOCKS = 8192  # up to here k_scan_add_raw, above k_scan_blocks + k_scan_add
SCAN_BLOCKS_ROUND = 1024  # block sums per round of k_scan_blocks (the carry goes from round to round)
SPLIT_SCAN_MAX_TREES = 32768  # up to here k_split_scan (one workgroup), above the multi-block scans + k_split_finalize
SPLIT_SCAN_THREADS = 1024  # k_split_scan: ceil(M / 1024) trees per thread
SPLIT_THREADS = 64  # trees per workgroup of the thread-per-tree kernels, halved down to 8 ...
SPLIT_CAP = 2304  # ... a workgroup of at most this many nodes works on a copy in LDS
PAR_PATH = 192  # longest root path (in the child) the per-node family takes; longer: the other family
ANALYZE_LDS_TAXA = 2048  # universes up to here: k_analyze_leaves_lds
ANALYZE_LEAVES_PER_BLOCK = 256 * 32  # leaves per workgroup of k_analyze_leaves_lds
SIG_TILE = 16384  # taxa per tile of k_analyze_sig_tiled
ANALYZE_SAMPLE = 256  # the union-find's sampled passes: one wave in 256, before it one in 4096 ...
SAMPLE_MIN_LEAVES = 64 * ANALYZE_SAMPLE * 4  # ... each only above this many leaves (65 536; 1 048 576 for the coarser one)


def scan_blocks(n: int) -> int:
    """Workgroups of ``scan_exclusive`` over ``n`` items (``n + 1`` outputs)."""
    return (n + 1 + SCAN_BLOCK - 1) // SCAN_BLOCK


def trees_per_workgroup(n_nodes: int, n_trees: int) -> int:
    """The launcher's choice (``forest_split``): 64 trees a workgroup, halved while the forest's AVERAGE tree makes
    a workgroup's nodes exceed 0.85 of the LDS copy, down to 8."""
    tpb = SPLIT_THREADS
    while tpb > 8 and n_nodes / n_trees * tpb > 0.85 * SPLIT_CAP:
        tpb >>= 1
    return tpb


def workgroup_nodes(arrays: TreeArrays) -> tuple[int, np.ndarray]:
    """``(tpb, nodes per workgroup)`` of the thread-per-tree kernels on ``arrays``; a workgroup is staged in LDS iff
    its entry is ``<= SPLIT_CAP``."""
    m = arrays.n_trees
    tpb = trees_per_workgroup(int(arrays.node_off[-1]), m)
    cuts = np.minimum(np.arange(0, m + tpb, tpb), m)
    cuts = cuts[: (m + tpb - 1) // tpb + 1]
    return tpb, np.diff(arrays.node_off[cuts])


def max_inner_depth(arrays: TreeArrays, t: int) -> int:
    """Depth (root = 0) of the deepest inner node of tree ``t``: the longest root path ``k_par_values`` collects when
    the whole tree is kept.  The call falls back to the thread-per-tree kernels iff it exceeds ``PAR_PATH``."""
    lo, hi = int(arrays.node_off[t]), int(arrays.node_off[t + 1])
    par, tax = arrays.parent[lo:hi], arrays.taxon[lo:hi]
    depth = np.zeros(hi - lo, dtype=np.int64)
    for i in range(1, hi - lo):
        depth[i] = depth[par[i]] + 1
    inner = tax < 0
    return int(depth[inner].max()) if inner.any() else 0


# ------------------------------------------------------------------------------------------------ builders
def taxon_names(n_taxa: int) -> list[str]:
    return [f"t{i:06d}" for i in range(n_taxa)]


def tree_shape(rng: np.random.RandomState, k: int, extra: str | None = None, comb: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """``(parent, is_leaf)`` of a rooted tree of ``k >= 2`` leaves in preorder: binary (2k - 1 nodes) with random
    splits, or -- ``comb`` -- a caterpillar whose inner nodes form one path (the deepest at depth k - 2).
    ``extra='unary'`` puts one node of a single child under the root (2k nodes), ``extra='tri'`` gives the root
    three children (2k - 2 nodes, ``k >= 3``)."""
    assert k >= 2 and extra in (None, "unary", "tri") and (extra != "tri" or k >= 3)
    parent: list[int] = []
    leaf: list[bool] = []
    stack = [(k, -1, "root")]
    while stack:
        n, p, role = stack.pop()
        me = len(parent)
        parent.append(p)
        if role == "unary":  # one child that holds all n leaves
            leaf.append(False)
            stack.append((n, me, ""))
            continue
        if n == 1:
            leaf.append(True)
            continue
        leaf.append(False)
        if role == "root" and extra == "tri":
            a = int(rng.randint(1, n - 1))
            b = int(rng.randint(1, n - a))
            stack.extend([(n - a - b, me, ""), (b, me, ""), (a, me, "")])
            continue
        a = n - 1 if comb else int(rng.randint(1, n))
        # (a comb: the first child carries the rest of the path, the second is a leaf)
        stack.extend([(n - a, me, ""), (a, me, "unary" if role == "root" and extra == "unary" else "")])
    want = 2 * k - 1 + (extra == "unary") - (extra == "tri")
    assert len(parent) == want and sum(leaf) == k
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def _sample_rows(rng: np.random.RandomState, count: int, pool: np.ndarray, k: int) -> np.ndarray:
    """``count`` rows of ``k`` distinct ids of ``pool``, in random order."""
    assert k <= len(pool)
    if k * k * 8 < len(pool):  # few of many: draw, and draw the rows with a repeat again
        rows = rng.randint(0, len(pool), size=(count, k))
        while True:
            s = np.sort(rows, axis=1)
            bad = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
            if len(bad) == 0:
                break
            rows[bad] = rng.randint(0, len(pool), size=(len(bad), k))
    else:
        rows = np.argsort(rng.random_sample((count, len(pool))), axis=1)[:, :k]
    return pool[rows]


def build_forest(seed: int, n_taxa: int, leaf_counts: Sequence[int], extras: dict | None = None,
                 pools: Sequence[np.ndarray] | None = None, pool_of: Sequence[int] | None = None,
                 combs: Sequence[int] = (), neg_len: float = 0.0, nan_len: float = 0.0,
                 shapes_per_class: int = 3) -> TreeArrays:
    """Trees of the prescribed leaf counts, in the prescribed order, as ONE ``TreeArrays`` over ``n_taxa`` ids.

    ``extras``: tree index -> ``'unary'`` / ``'tri'`` (``tree_shape``); ``combs``: tree indices that are caterpillars.
    ``pools`` / ``pool_of``: tree ``t`` draws its (distinct) taxa from ``pools[pool_of[t]]`` (default: all ids).
    Inner lengths are positive, negative with probability ``neg_len`` and missing (NaN) with ``nan_len`` (so the
    monotone flag and the host's order of additions matter); leaves carry lengths, inner nodes supports; the root
    has no length; every tree has its own weight."""
    rng = np.random.RandomState(seed)
    extras = extras or {}
    combs = set(combs)
    leaf_counts = np.asarray(leaf_counts, dtype=np.int64)
    m = len(leaf_counts)
    pools = [np.arange(n_taxa, dtype=np.int32)] if pools is None else [np.asarray(p, dtype=np.int32) for p in pools]
    pool_of = np.zeros(m, dtype=np.int64) if pool_of is None else np.asarray(pool_of, dtype=np.int64)
    special = np.zeros(m, dtype=np.int64)  # 0 plain, 1 unary, 2 tri, +4 comb
    for t, e in extras.items():
        special[t] = {"unary": 1, "tri": 2}[e]
    for t in combs:
        special[t] += 4
    nodes = 2 * leaf_counts - 1 + (special % 4 == 1) - (special % 4 == 2)
    node_off = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(nodes, out=node_off[1:])
    total = int(node_off[-1])
    parent = np.empty(total, dtype=np.int32)
    taxon = np.full(total, -1, dtype=np.int32)
    root = np.zeros(total, dtype=bool)
    root[node_off[:-1]] = True
    key = (leaf_counts * 8 + special) * len(pools) + pool_of
    for cls in np.unique(key):
        trees = np.flatnonzero(key == cls)
        k, sp, pool = int(leaf_counts[trees[0]]), int(special[trees[0]]), pools[int(pool_of[trees[0]])]
        extra = {0: None, 1: "unary", 2: "tri"}[sp % 4]
        which = rng.randint(0, shapes_per_class, size=len(trees))
        for s in range(shapes_per_class):
            mine = trees[which == s]
            if len(mine) == 0:
                continue
            par, leaf = tree_shape(rng, k, extra, comb=sp >= 4)
            at = node_off[mine][:, None] + np.arange(len(par))[None, :]
            parent[at] = par[None, :]
            taxon[at[:, leaf]] = _sample_rows(rng, len(mine), pool, k)
    inner = taxon < 0
    length = rng.exponential(0.1, total) + 1e-3
    flip = inner & (rng.random_sample(total) < neg_len)
    length[flip] = -length[flip]
    length[inner & (rng.random_sample(total) < nan_len)] = np.nan
    length[root] = np.nan
    support = np.where(inner, rng.randint(50, 101, total).astype(np.float64), np.nan)
    weights = rng.choice([1.0, 2.0, 0.5, 0.75], size=m) + rng.randint(0, 2, m) * rng.random_sample(m)
    return TreeArrays(n_taxa=n_taxa, node_off=node_off, parent=parent, taxon=taxon, length=length, support=support,
                      weights=weights, taxa=taxon_names(n_taxa))


def comb_forest(seed: int, n_leaves: int, n_taxa: int | None = None) -> TreeArrays:
    """One caterpillar of ``n_leaves`` leaves (its deepest inner node at depth ``n_leaves - 2``) over ``n_taxa`` ids."""
    n_taxa = n_leaves if n_taxa is None else n_taxa
    return build_forest(seed, n_taxa, [n_leaves], combs=[0], shapes_per_class=1)


def tiny_forest(seed: int, n_trees: int, n_taxa: int = 300, pools=None, pool_of=None, **kw) -> TreeArrays:
    """``n_trees`` trees of 3 to 6 leaves each over a universe of a few hundred ids, per-tree weights: the forests of
    a deep level in small (7 to 11 nodes a tree)."""
    rng = np.random.RandomState(seed + 7919)
    return build_forest(seed, n_taxa, rng.randint(3, 7, size=n_trees), pools=pools, pool_of=pool_of, **kw)


def concat_forests(forests: Sequence[TreeArrays]) -> TreeArrays:
    """The trees of ``forests`` (over the same ids), one after the other."""
    first = forests[0]
    assert all(f.n_taxa == first.n_taxa and f.ids is None for f in forests)
    off = [np.zeros(1, dtype=np.int64)]
    for f in forests:
        off.append(f.node_off[1:] + off[-1][-1])
    return TreeArrays(n_taxa=first.n_taxa, node_off=np.concatenate(off),
                      parent=np.concatenate([f.parent for f in forests]),
                      taxon=np.concatenate([f.taxon for f in forests]),
                      length=np.concatenate([f.length for f in forests]),
                      support=np.concatenate([f.support for f in forests]),
                      weights=np.concatenate([f.weights for f in forests]), taxa=first.taxa)


def parts_of(seed: int, ids: np.ndarray, n_parts: int, drop: float = 0.1, lone_last: bool = False) -> list[np.ndarray]:
    """Disjoint sorted id sets: ``drop`` of ``ids`` in no part, the rest dealt at random; ``lone_last``: the last part
    is ONE taxon -- no tree can keep two leaves of it, so that part keeps no tree at all."""
    rng = np.random.RandomState(seed)
    ids = np.asarray(ids, dtype=np.int32)
    ids = ids[rng.permutation(len(ids))][: max(2 * n_parts, int(round(len(ids) * (1.0 - drop))))]
    real = n_parts - 1 if lone_last else n_parts
    lone = ids[:1] if lone_last else ids[:0]
    rest = ids[len(lone):]
    label = rng.randint(0, real, size=len(rest))
    label[:real] = np.arange(real)  # no part empty
    out = [np.sort(rest[label == b]).astype(np.int32) for b in range(real)]
    if lone_last:
        out.append(lone.astype(np.int32))
    return out


def well_formed(arrays: TreeArrays) -> None:
    """Preorder parents, one root per tree, every inner node with a child, taxon ids in range and distinct per tree."""
    for t in range(arrays.n_trees):
        lo, hi = int(arrays.node_off[t]), int(arrays.node_off[t + 1])
        par, tax = arrays.parent[lo:hi], arrays.taxon[lo:hi]
        assert hi > lo and par[0] == -1
        assert np.all(par[1:] >= 0) and np.all(par[1:] < np.arange(1, hi - lo))
        assert np.all(tax >= -1) and np.all(tax < arrays.n_taxa)
        assert np.all(tax[par[1:]] == -1)  # parents are inner nodes
        kids = np.bincount(par[1:], minlength=hi - lo)
        assert np.all(kids[tax < 0] >= 1) and np.all(kids[tax >= 0] == 0)
        # preorder: a node's parent is on the root path of the node before it
        depth = np.zeros(hi - lo, dtype=np.int64)
        for i in range(1, hi - lo):
            depth[i] = depth[par[i]] + 1
            q = i - 1
            while q != par[i]:
                q = par[q]
                assert q >= 0
        leaves = tax[tax >= 0]
        assert len(np.unique(leaves)) == len(leaves)
    assert len(arrays.weights) == arrays.n_trees


# ---------------------------------------------------------------------------------------------- references
def scan_reference(op: int, rows: np.ndarray) -> np.ndarray:
    """``out[part][i]`` = sum (``op`` 0, identity 0) or maximum (``op`` 1, identity -1) of ``rows[part][:i]``,
    ``i`` in ``[0, n]``: accumulated in int64, cast back."""
    rows = np.asarray(rows)
    assert rows.ndim == 2 and op in (0, 1)
    out = np.empty((rows.shape[0], rows.shape[1] + 1), dtype=np.int64)
    out[:, 0] = 0 if op == 0 else -1
    if op == 0:
        np.cumsum(rows, axis=1, dtype=np.int64, out=out[:, 1:])
    else:
        np.maximum.accumulate(rows, axis=1, dtype=np.int64, out=out[:, 1:])
        np.maximum(out, -1, out=out)
    assert out.min(initial=0) >= -(1 << 31) and out.max(initial=0) < (1 << 31)
    return out.astype(np.int32)


def analysis_reference(tables: fl.TreeTables) -> tuple[np.ndarray, list]:
    """``(comp_root [n_taxa], side_sets [n_taxa])`` of host tables.

    ``comp_root[x]``: the smallest id of x's component under "join leaf p and p + 1 unless ``adj_depth[p] == 0``"
    (a root gap, or the padding slot behind a tree's last leaf) -- x itself for an id no tree holds.  Computed by
    propagating the smallest label along the distinct joins until nothing changes (no union-find: not the
    algorithm of the kernels or of ``flatten.pcg_components``).

    ``side_sets[x]``: the ``frozenset`` of ``flatten.leaf_side_ids`` taxon x occurs in (empty for an absent id).  Two
    taxa are contracted iff their sets are equal (``flatten.contraction_groups_numpy``)."""
    n = tables.n_taxa
    tax = tables.leaf_taxon.astype(np.int64)
    label = np.arange(n, dtype=np.int64)
    joined = np.flatnonzero(tables.adj_depth != 0)
    if len(joined):
        assert joined.max() + 1 < len(tax)
        pairs = np.unique(tax[joined] * n + tax[joined + 1])
        u, v = pairs // n, pairs % n
        while True:
            new = label.copy()
            np.minimum.at(new, u, label[v])
            np.minimum.at(new, v, label[u])
            new = new[new]  # (labels are ids of the same component: follow them)
            if np.array_equal(new, label):
                break
            label = new
    side = fl.leaf_side_ids(tables)
    order = np.argsort(tax, kind="stable")
    counts = np.bincount(tax, minlength=n)
    chunks = np.split(side[order], np.cumsum(counts)[:-1]) if n else []
    side_sets = [frozenset(c.tolist()) for c in chunks]
    return label.astype(np.int32), side_sets


def same_partition(keys_a: Sequence, keys_b: Sequence) -> bool:
    """Whether two labellings of the same items induce the same partition (both directions)."""
    assert len(keys_a) == len(keys_b)
    a_to_b: dict = {}
    b_to_a: dict = {}
    for a, b in zip(keys_a, keys_b):
        if a_to_b.setdefault(a, b) != b or b_to_a.setdefault(b, a) != a:
            return False
    return True


def check_signatures(sig: np.ndarray, side_sets: Sequence[frozenset]) -> None:
    """The device's signatures against the side sets: the partition of the PRESENT taxa by their
    ``(sig[x, 0], sig[x, 1])`` pair is the partition by side set, in both directions -- equal sets, equal pairs
    (necessary for a contraction to be found) and distinct sets, distinct pairs (a false collision has probability
    about T^2 / 2^65); an absent id carries ``(0, 0)``."""
    assert sig.shape == (len(side_sets), 2) and sig.dtype == np.uint64
    here = np.asarray([len(s) > 0 for s in side_sets], dtype=bool)
    assert not sig[~here].any(), "an id no tree holds carries a signature"
    pairs = [(int(a), int(b)) for a, b in sig[here]]
    sets = [s for s in side_sets if s]
    assert same_partition(pairs, sets), "signature classes differ from side-set classes"


def pair_kinds(side_sets: Sequence[frozenset]) -> tuple[bool, bool]:
    """``(some two present taxa have equal side sets, some two have distinct ones)``: an analysis case needs both."""
    present = [s for s in side_sets if s]
    distinct = len(set(present))
    return distinct < len(present), distinct > 1


def union_tables(children: Sequence[TreeArrays], bases: Sequence[int], strategy: str, n_taxa: int) -> fl.TreeTables:
    """The tables of the union forest a level split returns, from the HOST's children: their tables one after the
    other (the union's tree order), child ``c``'s taxa moved to ``bases[c] + id``."""
    tabs = [c.flatten(strategy) for c in children]
    off = [np.zeros(1, dtype=np.int64)]
    for t in tabs:
        off.append(t.tree_off[1:] + off[-1][-1])
    return fl.TreeTables(
        n_taxa=n_taxa, tree_off=np.concatenate(off),
        leaf_taxon=np.concatenate([t.leaf_taxon + np.int32(b) for t, b in zip(tabs, bases)]).astype(np.int32),
        adj_depth=np.concatenate([t.adj_depth for t in tabs]).astype(np.int32),
        adj_val=np.concatenate([t.adj_val for t in tabs]), tree_w=np.concatenate([t.tree_w for t in tabs]),
        monotone=all(t.monotone for t in tabs))


# --------------------------------------------------------------------------------------------------- cases
# The forests of tests/test_gpu_forest_edges.py.  tests/test_forest_reference_cpu.py asserts the numbers each of them
# is there for, so that a change to a builder cannot quietly move a case off its edge.
TINY_UNIVERSE = 300
OFFSET_TREES = (1023, 1024, 1025, 5000, 32768, 32769, 70000)


def offsets_case(n_trees: int, n_parts: int):
    """``(forest of n_trees tiny trees, parts)``: a tenth of the taxa in no part, trees of 3 to 6 leaves so that most
    parts drop most trees; with three and more parts the last one is a single taxon and keeps no tree at all."""
    arrays = tiny_forest(n_trees, n_trees, TINY_UNIVERSE, neg_len=0.05, nan_len=0.1)
    parts = parts_of(n_trees + n_parts, np.arange(TINY_UNIVERSE), n_parts, drop=0.1, lone_last=n_parts > 2)
    return arrays, parts


LEVEL_NODES = 5
LEVEL_CUTS = (0.10, 0.35, 0.36, 0.80, 1.0)  # the nodes' shares of the level's trees (one of them tiny)


def level_case(n_trees: int, n_parts: int):
    """A level forest of ``LEVEL_NODES`` nodes (node k owns the ids ``[k U, (k + 1) U)`` and a consecutive tree range)
    and its split: ``(level forest, node_tree_end, part_of, new_id, child_taxa, order, sets)`` -- ``order`` lists the
    children ``(part, node)`` in the union's tree order (part-major), ``sets[c]`` the level ids of child
    ``order[c]``, numbered ``new_id`` = ``base[c] + rank`` in the children's universe.  Odd nodes have two parts
    only; node 1 ends with a single-taxon part when it has more; a tenth of every node's taxa is in no part."""
    u = TINY_UNIVERSE
    t_end = np.asarray([max(k + 1, int(round(c * n_trees))) for k, c in enumerate(LEVEL_CUTS)], dtype=np.int32)
    t_end[-1] = n_trees
    pool_of = np.searchsorted(t_end, np.arange(n_trees), side="right")
    pools = [np.arange(k * u, (k + 1) * u, dtype=np.int32) for k in range(LEVEL_NODES)]
    level = tiny_forest(n_trees + 1, n_trees, LEVEL_NODES * u, pools=pools, pool_of=pool_of, neg_len=0.05, nan_len=0.1)
    node_parts = []
    for k in range(LEVEL_NODES):
        np_k = n_parts if k % 2 == 0 or k == 1 else 2
        node_parts.append(parts_of(1000 * n_parts + k, pools[k], np_k, drop=0.1, lone_last=(k == 1 and np_k > 2)))
    part_of = np.full(level.n_taxa, -1, dtype=np.int32)
    new_id = np.zeros(level.n_taxa, dtype=np.int32)
    order, sets, bases, at = [], [], [], 0
    for b in range(n_parts):
        for k in range(LEVEL_NODES):
            if b < len(node_parts[k]):
                ids = node_parts[k][b]
                part_of[ids] = b
                new_id[ids] = at + np.arange(len(ids), dtype=np.int32)
                order.append((b, k))
                sets.append(ids)
                bases.append(at)
                at += len(ids)
    return level, t_end, part_of, new_id, at, order, sets, bases


# trees per workgroup -> (leaves of the two heavy tree sizes, how the 2305th node is made, filler leaves, tree count)
STAGING = {64: (18, "tri", 3, 401), 32: (36, "unary", 16, 137), 16: (72, "tri", 40, 69), 8: (144, "unary", 100, 35)}


def staging_case(tpb: int) -> TreeArrays:
    """Workgroup 1 of ``tpb`` trees holds exactly ``SPLIT_CAP`` nodes (half of k leaves, half of k + 1: tpb (2k) nodes),
    workgroup 2 exactly ``SPLIT_CAP + 1`` (one tree less of k + 1 leaves, and one of k + 1 leaves with a unary node or
    of k + 2 leaves with a trifurcation: one node more); fillers around them keep the forest's average where the
    launcher chooses ``tpb``; the last workgroup is partial."""
    k, how, filler, m = STAGING[tpb]
    half = tpb // 2
    counts = [filler] * tpb + [k] * half + [k + 1] * half + [k] * half + [k + 1] * (half - 1)
    counts.append(k + 1 if how == "unary" else k + 2)
    extras = {len(counts) - 1: how}
    counts += [filler] * (m - len(counts))
    return build_forest(100 + tpb, 400, counts, extras=extras, neg_len=0.1, nan_len=0.1)


def mixed_staging_case() -> TreeArrays:
    """Small trees with a run of twenty 150-leaf trees in the middle: staged and in-place workgroups in one launch."""
    rng = np.random.RandomState(5)
    counts = rng.randint(3, 7, size=300).tolist() + [150] * 20 + rng.randint(3, 7, size=301).tolist()
    return build_forest(55, 400, counts, neg_len=0.1, nan_len=0.1)


NODE_TOTALS = (4095, 4096, 4097, 8191, 8192)


def exact_nodes_case(n_nodes: int, k: int = 40) -> TreeArrays:
    """A forest of exactly ``n_nodes`` nodes: binary trees of ``k`` leaves, and a last tree that takes the rest -- with
    a unary node where the rest is even (binary trees alone give odd totals)."""
    q = n_nodes // (2 * k - 1) - 1
    rest = n_nodes - q * (2 * k - 1)
    counts = [k] * q
    extras = {}
    if rest % 2:
        counts.append((rest + 1) // 2)
    else:
        counts.append(rest // 2)
        extras[q] = "unary"
    return build_forest(n_nodes, 200, counts, extras=extras, neg_len=0.05, nan_len=0.1)


COMB_LEAVES = tuple(range(190, 197))  # deepest inner node at 188 ... 194: PAR_PATH = 192 lies inside


def comb_among_balanced_case() -> TreeArrays:
    """Thirty balanced trees and, in their middle, one comb past ``PAR_PATH``: the fallback takes the whole call."""
    a = build_forest(71, 220, [40] * 15)
    c = comb_forest(72, 196, 220)
    b = build_forest(73, 220, [40] * 15)
    return concat_forests([a, c, b])


def analysis_forest(seed: int, n_taxa: int, leaf_counts: Sequence, blocks: int = 1, absent: int = 5, rare: int = 6) -> TreeArrays:
    """A forest for the analysis: ``absent`` ids no tree holds, ``rare`` ids only tree 0 holds (two root sides: some
    two of them have EQUAL side sets), the rest dealt into ``blocks`` interleaved pools -- tree t draws from pool
    t mod blocks, so the forest falls into at least ``blocks`` components.  A leaf count of ``None`` is full coverage
    of the tree's pool.  The first and the last id are always held (the last tile of the signatures is never empty)."""
    rng = np.random.RandomState(seed)
    inner = rng.permutation(np.arange(1, n_taxa - 1))
    gone, rare_ids = inner[:absent], inner[absent:absent + rare]
    ends = np.asarray([0, n_taxa - 1])
    common = np.setdiff1d(np.arange(1, n_taxa - 1), inner[:absent + rare])
    pools = [common[b::blocks] for b in range(blocks)]
    pools[0] = np.sort(np.concatenate([pools[0], ends]))
    pools.append(np.sort(np.concatenate([pools[0], rare_ids])))
    m = len(leaf_counts)
    pool_of = np.arange(m) % blocks
    pool_of[0] = blocks
    counts = [len(pools[pool_of[t]]) if c is None else int(c) for t, c in enumerate(leaf_counts)]
    arrays = build_forest(seed, n_taxa, counts, pools=pools, pool_of=pool_of, shapes_per_class=1)
    # tree 0 holds the two ends and every rare id, whatever it drew: they take the place of other leaves of it
    first = arrays.taxon[: int(arrays.node_off[1])]
    must = np.concatenate([ends, rare_ids])
    free = np.flatnonzero((first >= 0) & ~np.isin(first, must))
    missing = must[~np.isin(must, first)]
    first[free[: len(missing)]] = missing
    assert len(gone) == absent and np.all(np.isin(must, first))
    return arrays


# name -> (universe, trees, leaves per tree (None: full coverage), blocks)
ANALYSIS = {
    "lds_2047_partial": (2047, 12, 1500, 1),          # LDS route, 3 workgroups (18 000 leaves), nearly all sets distinct
    "lds_2048_full": (2048, 12, None, 1),             # the largest LDS universe, 3 workgroups
    "tiled_2049_full": (2049, 12, None, 1),           # the smallest tiled one: one tile, no sampled pass
    "tiled_16383_three_full": (16383, 3, None, 1),    # one tile; 8 side-set classes: huge groups of equal sets
    "tiled_16384_partial20": (16384, 20, 6500, 2),    # exactly one full tile; 130 000 leaves: one sampled pass
    "tiled_16385_full70": (16385, 70, None, 1),       # a last tile of ONE taxon; 1.15 M leaves: both sampled passes
    "tiled_20000_blocks": (20000, 6, 3000, 3),        # a short last tile; three pools: several components
    "leaves_65536": (4000, 32, 2048, 1),              # at the sampled pass's threshold: it does not run
    "leaves_65537": (4000, 32, 2048, 1),              # one leaf more: it runs
}


def analysis_case(name: str) -> TreeArrays:
    u, m, leaves, blocks = ANALYSIS[name]
    counts = [leaves] * m
    if name == "leaves_65537":
        counts[-1] += 1
    if name == "lds_2047_partial":
        counts[0] = None
    return analysis_forest(sum(map(ord, name)), u, counts, blocks=blocks)


# children's universe -> (trees, leaves per tree): the analysis reached through a level split that DROPS a fifth of
# the parent's taxa, so the device's leaf count is well below the capacity its launches are sized by
ANALYSIS_LEVEL = {2048: (12, 2200), 2049: (12, 2200), 16384: (8, 9000), 16385: (8, None)}


def analysis_level_case(child_taxa: int):
    """``(forest, part_of, new_id, parts)``: a forest over ``child_taxa * 5 // 4`` ids of which exactly ``child_taxa``
    (the first and the last among them) go to two parts; the children are numbered part after part."""
    m, leaves = ANALYSIS_LEVEL[child_taxa]
    n_taxa = child_taxa * 5 // 4
    arrays = analysis_forest(child_taxa, n_taxa, [leaves] * m, blocks=2 if child_taxa == 16384 else 1)
    rng = np.random.RandomState(child_taxa)
    kept = np.concatenate([[0, n_taxa - 1], 1 + rng.permutation(n_taxa - 2)[: child_taxa - 2]])
    label = rng.randint(0, 2, size=child_taxa)
    label[:2] = (0, 1)
    parts = [np.sort(kept[label == b]).astype(np.int32) for b in range(2)]
    part_of = np.full(n_taxa, -1, dtype=np.int32)
    new_id = np.zeros(n_taxa, dtype=np.int32)
    at = 0
    for b, ids in enumerate(parts):
        part_of[ids] = b
        new_id[ids] = at + np.arange(len(ids), dtype=np.int32)
        at += len(ids)
    assert at == child_taxa
    return arrays, part_of, new_id, parts
