"""Host references of the clade conflict counts of ``score_supertree(..., conflicts=True)`` (helper module, not
collected).

* ``brute_force``: every nontrivial restricted supertree cluster against every cluster of the source tree, over
  Python sets (small cases only);
* ``quadratic``: both trees' clusters as ranges of their leaf orders (polytomies and unary nodes allowed, as in
  ``triplet_reference``); for every cluster z of the restricted supertree one prefix-count vector over T's leaf order
  gives I(y, z) = |y ∩ z| for all of T's clusters y at once, and y, z conflict iff 0 < I(y, z) < min(|y|, |z|).  The
  flags reach the supertree's nodes through their restricted sets.

Both take the supertree (a ``TreeNode``) and a list of source ``TreeNode`` objects and return a dict of int64
arrays: ``n_super_conflict``, ``n_source_conflict`` per tree, ``conflicting`` per supertree node in
``TreeNode.to_flat`` order.  ``contract`` removes a random share of a tree's internal edges.
"""

from __future__ import annotations

import numpy as np
from score_reference import _leaf_sets, _nontrivial, _preorder
from triplet_reference import _hierarchy, _ranges

from spectralclustersupertree_amd.tree import TreeNode


def _result(n_super_conflict, n_source_conflict, conflicting) -> dict:
    return {
        "n_super_conflict": np.asarray(n_super_conflict, dtype=np.int64),
        "n_source_conflict": np.asarray(n_source_conflict, dtype=np.int64),
        "conflicting": np.asarray(conflicting, dtype=np.int64),
    }


def _conflict(a: frozenset, b: frozenset) -> bool:
    return bool(a & b) and not a <= b and not b <= a


def brute_force(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    s_nodes = _preorder(supertree)
    s_sets = _leaf_sets(s_nodes)
    s_list = [s_sets[id(v)] for v in s_nodes]
    n_super_conflict, n_source_conflict = [], []
    conflicting = np.zeros(len(s_nodes), dtype=np.int64)
    for tree in trees:
        t_sets = _leaf_sets(_preorder(tree))
        leaves = t_sets[id(tree)]
        n = len(leaves)
        restricted = [c & leaves for c in s_list]
        c_t = _nontrivial(t_sets.values(), n) if n >= 3 else set()
        c_st = _nontrivial(restricted, n) if n >= 3 else set()
        n_super_conflict.append(sum(any(_conflict(z, y) for y in c_t) for z in c_st))
        n_source_conflict.append(sum(any(_conflict(y, z) for z in c_st) for y in c_t))
        for i, c in enumerate(restricted):
            if c in c_st and any(_conflict(c, y) for y in c_t):
                conflicting[i] += 1
    return _result(n_super_conflict, n_source_conflict, conflicting)


def quadratic(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    s_nodes = _preorder(supertree)
    s_tips = [v.name for v in s_nodes if v.is_tip()]
    s_index = {name: i for i, name in enumerate(s_tips)}
    n_super_conflict, n_source_conflict = [], []
    conflicting = np.zeros(len(s_nodes), dtype=np.int64)
    for tree in trees:
        t_nodes = _preorder(tree)
        t_tips = [v.name for v in t_nodes if v.is_tip()]
        m = len(t_tips)
        if m < 3:
            n_super_conflict.append(0)
            n_source_conflict.append(0)
            continue
        t_pos = {name: i for i, name in enumerate(t_tips)}
        y, _ = _hierarchy(_ranges(t_nodes, t_pos), m)
        # S' in S order: the tree's leaves sorted by their supertree position; every S node's restricted range
        s_order = sorted(t_tips, key=s_index.__getitem__)
        s_ranges = _ranges(s_nodes, {name: k for k, name in enumerate(s_order)})
        z, _ = _hierarchy(s_ranges, m)
        tp = np.array([t_pos[name] for name in s_order], dtype=np.int64)  # T position of S' leaf k
        y_size = y[:, 1] - y[:, 0]
        y_flag = np.zeros(len(y), dtype=bool)
        z_flag = np.zeros(len(z), dtype=bool)
        for j, (zl, zh) in enumerate(z):
            ind = np.zeros(m + 1, dtype=np.int64)
            ind[tp[zl:zh] + 1] = 1
            cz = np.cumsum(ind)
            i_yz = cz[y[:, 1]] - cz[y[:, 0]]
            hit = (i_yz > 0) & (i_yz < np.minimum(y_size, zh - zl))
            z_flag[j] = hit.any()
            y_flag |= hit
        n_super_conflict.append(int(z_flag.sum()))
        n_source_conflict.append(int(y_flag.sum()))
        flagged = {(int(a), int(b)) for (a, b), f in zip(z, z_flag) if f}
        if flagged:
            hits = [(int(a), int(b)) in flagged for a, b in s_ranges]
            conflicting += np.asarray(hits, dtype=np.int64)
    return _result(n_super_conflict, n_source_conflict, conflicting)


def contract(tree: TreeNode, rs: np.random.RandomState, share: float) -> TreeNode:
    """A copy of ``tree`` in which each internal edge (below an inner node, above an inner node) is contracted with
    probability ``share``: the child's children hang from its parent instead."""
    new: dict[int, TreeNode] = {}
    for node in reversed(_preorder(tree)):
        if node.is_tip():
            new[id(node)] = TreeNode(node.name)
            continue
        kids: list[TreeNode] = []
        for c in node.children:
            nc = new.pop(id(c))
            if not c.is_tip() and rs.rand() < share:
                kids.extend(list(nc.children))
            else:
                kids.append(nc)
        new[id(node)] = TreeNode(None, kids)
    return new[id(tree)]
