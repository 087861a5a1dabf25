"""Plain references and case builders for the kernels that carry a resident forest's tables into the small solve's
input block or into a tables handle (``k_small_pack_level``, ``k_small_pack``, ``k_rebase_offsets``,
``k_relabel_taxa_range``, ``k_relabel_taxa``; the cases of ``tests/test_gpu_resident_pack_edges.py``, held to their
numbers by ``tests/test_resident_pack_reference_cpu.py``).  CPU only: numpy and the host library.  DESIGN.md
section 37.

A *level forest* is a ``TreeArrays`` whose node ``k`` owns the consecutive trees ``[t_lo[k], t_hi[k])`` and the taxon
ids ``[u_lo[k], u_lo[k] + u_sz[k])`` -- what ``scs_forest_split_level`` leaves on the device, built here as
``tests/test_gpu_levels.py::_level_of`` and ``forest_reference.level_case`` build theirs.  Everything the kernels must
produce is indexing into its host ``flatten(strategy)``:

* ``pack_level``: per node ``tree_off[t0 .. t0 + m] - tree_off[t0]`` as int32, the taxa through the node's relabel,
  ``adj_depth`` / ``adj_val`` as they are, the trees' weights -- node after node in the order of the batch;
* ``pack_node``: the same for one child forest, relabel optional;
* ``slice_tables``: what ``scs_tables_from_forest_range`` / ``scs_tables_from_forest`` leave in a handle.

None of them searches: a node's slots are found by adding up what came before, on the host, in Python.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.treearrays import TreeArrays
from tests import forest_reference as fr

WORKGROUP = 256  # threads per workgroup of every kernel held here; slots 255 | 256 | 257 straddle the first edge
EDGE_SLOTS = (255, 256, 257)
LEAF_TOTALS = (255, 256, 257, 511, 512, 513)
NODE_COUNTS = (1, 2, 3, 7, 8, 9, 256, 257)
TIE_NODES = (128, 129)  # 2K = 256, 258 leaves = trees + nodes
MIXED_TAXA = (2, 3, 24, 25, 64, 65, 128)  # k_small_finish<256> | <1024> at 24 | 25 groups, finish_big above 64 taxa
KINDS = ("compact", "groups", "identity")


# ------------------------------------------------------------------------------------------------- references
def pack_level(tab: fl.TreeTables, t_begin, n_trees, u_base, u_size, relabel):
    """``(tree_off int32, leaf_taxon, adj_depth, adj_val, tree_w)`` of a batch of nodes of the level tables ``tab``:
    node ``i`` of the batch owns the trees ``[t_begin[i], t_begin[i] + n_trees[i])`` and the ids ``[u_base[i],
    u_base[i] + u_size[i])``; ``relabel`` holds the nodes' maps one after the other, ``u_size[i]`` entries each."""
    to, lt, ad, av, tw = [], [], [], [], []
    rl_at = 0
    for t0, m, lo, sz in zip(t_begin, n_trees, u_base, u_size):
        t0, m, lo, sz = int(t0), int(m), int(lo), int(sz)
        off = tab.tree_off[t0:t0 + m + 1]
        a, b = int(off[0]), int(off[-1])
        rl = np.asarray(relabel[rl_at:rl_at + sz], dtype=np.int32)
        rl_at += sz
        local = tab.leaf_taxon[a:b] - lo
        assert np.all(local >= 0) and np.all(local < sz)  # the node's trees hold the node's ids only
        to.append((off - a).astype(np.int32))
        lt.append(rl[local])
        ad.append(tab.adj_depth[a:b])
        av.append(tab.adj_val[a:b])
        tw.append(tab.tree_w[t0:t0 + m])
    return (np.concatenate(to).astype(np.int32), np.concatenate(lt).astype(np.int32),
            np.concatenate(ad).astype(np.int32), np.concatenate(av).astype(np.float64),
            np.concatenate(tw).astype(np.float64))


def pack_node(tab: fl.TreeTables, relabel=None):
    """The same for ONE child forest's tables (``scs_small_solve_begin_forest``): offsets as they are, narrowed;
    ``relabel[x]`` the node's id of the forest's taxon ``x`` (None: identity)."""
    assert int(tab.tree_off[0]) == 0
    lt = tab.leaf_taxon if relabel is None else np.asarray(relabel, dtype=np.int32)[tab.leaf_taxon]
    return (tab.tree_off.astype(np.int32), lt.astype(np.int32), tab.adj_depth.astype(np.int32),
            tab.adj_val.astype(np.float64), tab.tree_w.astype(np.float64))


def slice_tables(tab: fl.TreeTables, t_begin: int, t_end: int, u_base: int, relabel, n_taxa: int):
    """What a tables handle holds after ``scs_tables_from_forest_range`` (``relabel[x - u_base]``) or -- ``t_begin``
    0, ``t_end`` all trees, ``u_base`` 0, ``relabel`` possibly None -- ``scs_tables_from_forest``:
    ``(tree_off int64, leaf_taxon, adj_depth, adj_val, tree_w, info)``."""
    off = tab.tree_off[t_begin:t_end + 1]
    a, b = int(off[0]), int(off[-1])
    x = tab.leaf_taxon[a:b] - u_base
    lt = x if relabel is None else np.asarray(relabel, dtype=np.int32)[x]
    info = {"n_taxa": int(n_taxa), "n_trees": int(t_end - t_begin), "n_leaves": b - a,
            "max_leaves": int(np.diff(off).max())}
    return ((off - a).astype(np.int64), lt.astype(np.int32), tab.adj_depth[a:b].astype(np.int32),
            tab.adj_val[a:b].astype(np.float64), tab.tree_w[t_begin:t_end].astype(np.float64), info)


def node_numbering(tab: fl.TreeTables, t_lo: int, t_hi: int, u_lo: int, u_sz: int, kind: str):
    """The renumbering ``levels.Engine`` hands the pack for one node, by the same host routines: ``(relabel [u_sz],
    n_pres, n_groups, group_start or None, present [u_sz] bool)``.  ``compact``: a present id goes to its rank among
    the present ones; ``groups``: further to the numbering that makes the contraction groups consecutive
    (``fl.contraction_groups`` on the node's own tables, ordered as ``scs.relabel_for_contraction`` orders them);
    ``identity``: every id is present and keeps its place.  An ABSENT id's entry holds an id of the node that is in
    range and belongs to another taxon -- no leaf may ever read it."""
    a, b = int(tab.tree_off[t_lo]), int(tab.tree_off[t_hi])
    local = tab.leaf_taxon[a:b] - u_lo
    here = np.zeros(u_sz, dtype=bool)
    here[local] = True
    n = int(here.sum())
    prank = np.cumsum(here) - 1
    new_of_old = np.arange(n, dtype=np.int32)
    group_start, n_groups = None, n
    if kind == "identity":
        assert n == u_sz, "an identity numbering needs every id of the range in some tree"
    elif kind == "groups":
        own = fl.TreeTables(n_taxa=n, tree_off=(tab.tree_off[t_lo:t_hi + 1] - a).astype(np.int64),
                            leaf_taxon=prank[local].astype(np.int32), adj_depth=tab.adj_depth[a:b],
                            adj_val=tab.adj_val[a:b], tree_w=tab.tree_w[t_lo:t_hi])
        groups = fl.contraction_groups(own)
        n_groups = int(groups.max()) + 1
        order = np.lexsort((np.arange(n), groups))  # by group, then id
        new_of_old = np.empty(n, dtype=np.int32)
        new_of_old[order] = np.arange(n, dtype=np.int32)
        group_start = np.zeros(n_groups + 1, dtype=np.int32)
        np.cumsum(np.bincount(groups, minlength=n_groups), out=group_start[1:])
    else:
        assert kind == "compact"
    relabel = ((np.arange(u_sz) * 7 + 3) % n).astype(np.int32)  # absent ids: in range, nobody's
    relabel[here] = new_of_old[prank[here]]
    return relabel, n, n_groups, group_start, here


# ------------------------------------------------------------------------------------------------------ cases
@dataclass
class LevelCase:
    """A level forest, the relabel kind of every node and the batch (node indices, in the order they are passed)."""

    name: str
    level: TreeArrays
    t_lo: np.ndarray
    t_hi: np.ndarray
    u_lo: np.ndarray
    u_sz: np.ndarray
    kinds: list
    batch: np.ndarray
    strategy: str = "branch"
    mark: int = -1  # the node (position in the batch) the case's name speaks of
    _tab: dict = field(default_factory=dict)

    @property
    def tables(self) -> fl.TreeTables:
        if "t" not in self._tab:
            self._tab["t"] = self.level.flatten(self.strategy)
        return self._tab["t"]

    def with_batch(self, name: str, batch) -> "LevelCase":
        return LevelCase(name, self.level, self.t_lo, self.t_hi, self.u_lo, self.u_sz, self.kinds,
                         np.asarray(batch, dtype=np.int64), self.strategy, -1, self._tab)

    def inputs(self) -> dict:
        """Every argument of ``scs_small_solve_begin_level`` for the batch, the slots its nodes start at, and the
        nodes' own host tables (the reference's pack cut node by node) with their group boundaries."""
        if "in" in self._tab and self._tab["in"][0] == tuple(self.batch.tolist()):
            return self._tab["in"][1]
        tab = self.tables
        nodes = self.batch
        rl, n_taxa, n_groups, gs, gs_of = [], [], [], [], []
        for k in nodes:
            r, n, ng, g, _ = node_numbering(tab, int(self.t_lo[k]), int(self.t_hi[k]), int(self.u_lo[k]),
                                            int(self.u_sz[k]), self.kinds[k])
            rl.append(r)
            n_taxa.append(n)
            n_groups.append(ng)
            gs_of.append(g)
            gs.append(np.arange(n + 1, dtype=np.int32) if g is None else g)
        out = {"t_begin": self.t_lo[nodes].astype(np.int32), "n_trees": (self.t_hi - self.t_lo)[nodes].astype(np.int32),
               "n_leaves": (tab.tree_off[self.t_hi[nodes]] - tab.tree_off[self.t_lo[nodes]]).astype(np.int64),
               "u_base": self.u_lo[nodes].astype(np.int32), "u_size": self.u_sz[nodes].astype(np.int32),
               "relabel": np.concatenate(rl).astype(np.int32), "n_taxa": np.asarray(n_taxa, dtype=np.int32),
               "n_groups": np.asarray(n_groups, dtype=np.int32), "group_start": np.concatenate(gs).astype(np.int32)}
        out["leaf_ptr"] = np.concatenate(([0], np.cumsum(out["n_leaves"])))
        out["tree_ptr"] = np.concatenate(([0], np.cumsum(out["n_trees"].astype(np.int64))))
        want = pack_level(tab, out["t_begin"], out["n_trees"], out["u_base"], out["u_size"], out["relabel"])
        out["want"] = want
        host = []
        for i in range(len(nodes)):
            a, b = int(out["leaf_ptr"][i]), int(out["leaf_ptr"][i + 1])
            t0, t1 = int(out["tree_ptr"][i]), int(out["tree_ptr"][i + 1])
            host.append((fl.TreeTables(n_taxa=int(n_taxa[i]), tree_off=want[0][t0 + i:t1 + i + 1].astype(np.int64),
                                       leaf_taxon=want[1][a:b], adj_depth=want[2][a:b], adj_val=want[3][a:b],
                                       tree_w=want[4][t0:t1], monotone=True), gs_of[i]))
        out["host_nodes"] = host
        self._tab["in"] = (tuple(self.batch.tolist()), out)
        return out


def _forest(seed: int, n_taxa: int, leaf_counts, pools, pool_of) -> TreeArrays:
    """``forest_reference.build_forest`` with weights that are all different (a weight taken from another tree must
    change the arrays) and non-dyadic; lengths are exponential draws, positive: the tables are monotone."""
    arrays = fr.build_forest(seed, n_taxa, leaf_counts, pools=pools, pool_of=pool_of)
    rng = np.random.RandomState(seed + 4241)
    arrays.weights = rng.uniform(0.5, 2.0, arrays.n_trees) + np.arange(arrays.n_trees) * 1e-7
    return arrays


def level_of(name: str, seed: int, specs, kinds=None, strategy: str = "branch", batch=None, mark: int = -1) -> LevelCase:
    """``specs[k] = (leaf counts of node k's trees, ids of its range, ids of the range in no tree)``: node after
    node, ranges consecutive.  The ids left out are spread over the range (every third, from the second on); a first
    tree as large as what is left covers every remaining id.  ``kinds``: per node, default cycling through ``KINDS``
    (``identity`` only where nothing is absent)."""
    counts, pools, pool_of, t_hi, u_sz = [], [], [], [], []
    u_at = 0
    for k, (leaves, ids, absent) in enumerate(specs):
        assert 0 <= absent and ids - absent >= max(leaves) and min(leaves) >= 2
        out = {int(i) for i in 1 + 3 * np.arange(absent) if i < ids}
        for i in range(ids - 1, -1, -1):  # (more than a third absent: the rest from the top)
            if len(out) == absent:
                break
            out.add(i)
        pools.append(np.asarray([u_at + i for i in range(ids) if i not in out], dtype=np.int32))
        counts.extend(leaves)
        pool_of.extend([k] * len(leaves))
        t_hi.append(len(counts))
        u_sz.append(ids)
        u_at += ids
    level = _forest(seed, u_at, counts, pools, pool_of)
    t_hi = np.asarray(t_hi, dtype=np.int64)
    u_sz = np.asarray(u_sz, dtype=np.int64)
    if kinds is None:
        kinds = []
        for k, (leaves, ids, absent) in enumerate(specs):
            kind = KINDS[k % 3]
            if kind == "identity" and (absent or leaves[0] != ids):
                kind = "compact"
            kinds.append(kind)
    return LevelCase(name, level, np.concatenate(([0], t_hi[:-1])), t_hi, np.cumsum(u_sz) - u_sz, u_sz, list(kinds),
                     np.arange(len(specs)) if batch is None else np.asarray(batch, dtype=np.int64), strategy, mark)


def tiny(trees: int):
    """A node of 3 taxa and one, two or three trees: 3, 5 or 7 leaves, ``trees + 1`` offset slots."""
    return ([3, 2, 2][:trees], 3, 0)


PLAIN = ([40, 11], 40, 0)  # 51 leaves
_VARIED = [([12, 5, 9], 15, 3), ([7, 7], 9, 2), ([30, 4, 17, 22], 30, 0), ([5], 6, 1), ([40, 13], 44, 4),
           ([9, 2, 3, 4, 5], 9, 0), ([17, 6], 20, 3), ([3, 3], 4, 1), ([26, 26, 8], 26, 0)]


def nodes_case(k: int, strategy: str = "branch") -> LevelCase:
    """``k`` nodes.  Up to nine: different sizes, one to five trees, all three relabel kinds, absent ids; 256 and 257:
    nodes of 3 taxa with one or two trees (the searches over 256 | 257 entries, several workgroups of leaf slots)."""
    if k <= len(_VARIED):
        return level_of(f"{k} nodes" + ("" if strategy == "branch" else f" {strategy}"), 100 + k, _VARIED[:k],
                        strategy=strategy)
    return level_of(f"{k} nodes", 100 + k, [tiny(1 + (i * 7 % 3 == 0)) for i in range(k)])


def _filled(total: int):
    """Nodes of 40 taxa and two trees, 51 leaves each -- the last one with what is left -- holding ``total`` leaves."""
    n = total // 51
    specs = [PLAIN] * n
    specs[-1] = ([40, 11 + total - 51 * n], 40, 0)
    return specs


def leaf_total_case(total: int) -> LevelCase:
    return level_of(f"{total} leaves", 200 + total, _filled(total))


def leaf_boundary_case(slot: int) -> LevelCase:
    """A node whose first leaf sits in slot ``slot`` of the batch, with nodes on both sides of it."""
    before = _filled(slot)
    return level_of(f"a node's first leaf in slot {slot}", 300 + slot, before + [([40, 11], 44, 4), ([40, 7], 40, 0)],
                    mark=len(before))


def offset_boundary_case(slot: int) -> LevelCase:
    """A node whose first OFFSET entry (``tree_ptr[k] + k``) sits in slot ``slot``: nodes of two trees (three
    entries) in front of it, ``slot % 3`` of them with a third tree."""
    four = slot % 3
    before = [tiny(3)] * four + [tiny(2)] * ((slot - 4 * four) // 3)
    assert sum(len(s[0]) + 1 for s in before) == slot
    return level_of(f"a node's first offset in slot {slot}", 400 + slot, before + [([9, 4, 6], 11, 2), tiny(2)],
                    mark=len(before))


def tie_case(k: int) -> LevelCase:
    """Every node ONE tree of two leaves: ``n_leaf == n_tree + K``, the smallest grid the launch can have."""
    return level_of(f"tie of {k} nodes", 500 + k, [([2], 2, 0)] * k, kinds=["identity"] * k)


def subset_cases():
    """Batches that are not the level: ascending with gaps (what ``Engine._solve_small`` passes), the same nodes in
    another order, one node twice."""
    base = nodes_case(9)
    return [base.with_batch("subset ascending", [1, 3, 4, 7]), base.with_batch("subset permuted", [7, 1, 4, 3]),
            base.with_batch("subset with a repeat", [3, 5, 3, 8])]


def late_case() -> LevelCase:
    """A first node of 3 000 leaves that is NOT in the batch: the offsets the batch's nodes are rebased against are
    far above their own leaf counts."""
    specs = [([100] * 30, 100, 0)] + _VARIED[:4]
    return level_of("late trees", 600, specs, batch=[1, 2, 3, 4])


def mixed_case() -> LevelCase:
    """Nodes of 2, 3, 24, 25, 64, 65 and 128 PRESENT taxa (both sides of every threshold of the finishing kernels)
    and one contracted node, absent ids in every other one."""
    specs, kinds = [], []
    for i, n in enumerate(MIXED_TAXA):
        absent = (i % 2) * (1 + n // 10)
        trees = [n] + [max(2, n // 2), max(2, n - 1), max(2, n // 3)][: 1 + i % 4]
        specs.append((trees, n + absent, absent))
        kinds.append("compact" if absent else "identity")
    specs.append(([40, 40], 43, 3))
    kinds.append("groups")
    return level_of("mixed sizes", 700, specs, kinds=kinds)


def level_cases() -> list:
    """Every case of section A of ``tests/test_gpu_resident_pack_edges.py``, by name."""
    out = [nodes_case(k) for k in NODE_COUNTS]
    out += [leaf_total_case(t) for t in LEAF_TOTALS]
    out += [leaf_boundary_case(s) for s in EDGE_SLOTS]
    out += [offset_boundary_case(s) for s in EDGE_SLOTS]
    out += [tie_case(k) for k in TIE_NODES]
    out += subset_cases()
    out += [late_case(), mixed_case(), nodes_case(7, "one"), nodes_case(7, "depth")]
    return out


_CASES = {}


def level_case(name: str) -> LevelCase:
    if not _CASES:
        _CASES.update({c.name: c for c in level_cases()})
    return _CASES[name]


LEVEL_CASE_NAMES = ([f"{k} nodes" for k in NODE_COUNTS] + [f"{t} leaves" for t in LEAF_TOTALS]
                    + [f"a node's first leaf in slot {s}" for s in EDGE_SLOTS]
                    + [f"a node's first offset in slot {s}" for s in EDGE_SLOTS] + [f"tie of {k} nodes" for k in TIE_NODES]
                    + ["subset ascending", "subset permuted", "subset with a repeat", "late trees", "mixed sizes",
                       "7 nodes one", "7 nodes depth"])


# ---- single forests (children of scs_forest_split): section C, and the slices of section D
@dataclass
class NodeCase:
    name: str
    arrays: TreeArrays
    kind: str  # "null" (no relabel: every id present), "compact" or "groups"
    strategy: str = "branch"


def node_case(name: str) -> NodeCase:
    """One child forest: ``leaves N`` (N leaves in seven trees of up to 40), ``trees M`` (M trees of two or three
    leaves over 20 ids, one of them over all 20), each with ``null`` / ``compact`` / ``groups`` behind the name."""
    what, num, kind = name.split()
    num = int(num)
    absent = 0 if kind == "null" else 5
    if what == "leaves":
        counts = [40] * 6 + [num - 240]
        ids = 40 + absent
    else:
        assert what == "trees"
        counts = [20] + [2 + (i % 2) for i in range(num - 1)]
        ids = 20 + absent
    case = level_of(name, 800 + num + len(kind), [(counts, ids, absent)])
    return NodeCase(name, case.level, kind)


NODE_CASE_NAMES = ([f"leaves {n} {k}" for n in EDGE_SLOTS for k in ("null", "compact")]
                   + [f"trees {m} {k}" for m in (1, 255, 256, 257) for k in ("null", "compact")]
                   + ["trees 1 groups", "trees 2 groups"])


def node_inputs(case: NodeCase) -> dict:
    """Relabel (None for ``null``), taxon count, groups and the expected pack of a ``NodeCase``."""
    tab = case.arrays.flatten(case.strategy)
    kind = {"null": "identity"}.get(case.kind, case.kind)
    rl, n, ng, gs, here = node_numbering(tab, 0, tab.n_trees, 0, case.arrays.n_taxa, kind)
    relabel = None if case.kind == "null" else rl
    want = pack_node(tab, relabel)
    host = fl.TreeTables(n_taxa=n, tree_off=tab.tree_off, leaf_taxon=want[1], adj_depth=tab.adj_depth,
                         adj_val=tab.adj_val, tree_w=tab.tree_w, monotone=tab.monotone)
    return {"tables": tab, "relabel": relabel, "n_taxa": n, "n_groups": ng, "group_start": gs, "present": here,
            "want": want, "host": host}


def slice_level() -> LevelCase:
    """The level of section D: a first node to slice from ``t_begin = 0``, nodes of 254 | 255 | 256 trees (``n_trees
    + 1`` entries at the workgroup's edge), of 255 | 256 | 257 leaves, a single tree, a last node (``t_end =
    n_trees``); absent ids in every other node, all ranges but the first above 0.  The first node is SMALL: node 1's
    ids start below its own ``u_size``, so an id that was not moved down by ``u_base`` still finds an entry of the
    node's relabel -- the wrong one, not one outside it."""
    specs = [([5, 3], 6, 1)]
    specs += [([20] + [2 + (i % 2) for i in range(m - 1)], 24 + (m % 2) * 3, 4 + (m % 2) * 3) for m in (254, 255, 256)]
    specs += [([40] * 6 + [n - 240], 40 + (n % 2) * 5, (n % 2) * 5) for n in EDGE_SLOTS]
    specs += [([17], 17, 0), ([50, 21], 57, 7)]
    kinds = ["compact" if s[2] else "identity" for s in specs]
    return level_of("slices", 900, specs, kinds=kinds)


def build_level(n_taxa: int) -> LevelCase:
    """A node of ``n_taxa`` present taxa between two others, for the graphs built from a slice (40: one tile; 300:
    the largest node of this file, more than one 256-row block)."""
    big = ([n_taxa] + [max(2, n_taxa * (3 + i) // 9) for i in range(5)], n_taxa + 9, 9)
    return level_of(f"build {n_taxa}", 950 + n_taxa, [PLAIN, big, PLAIN], kinds=["identity", "compact", "identity"], mark=1)
