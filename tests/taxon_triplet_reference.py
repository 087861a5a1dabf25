"""Host references of the per-taxon triplet support of ``score_supertree(..., taxon_triplets=True)`` (helper module,
not collected).

* ``brute_force``: every triple of every source tree against every cluster of both trees, over Python sets (small
  cases only), each resolved triple credited to its three taxa;
* ``quadratic``: the node-pair formula of ``score.py``'s docstring in numpy -- the clusters and prefix-count vectors
  of ``triplet_reference.quadratic``, and for every node z of the restricted supertree two difference arrays over T's
  leaf order (add at a range's start, subtract at its end, prefix-sum): (I - 1) J on the leaves of y, C(I, 2) on those
  of py ∖ y, read by the leaves of z and of pz ∖ z.  About 0.7 s for one tree of 3 000 leaves.

Both take the supertree (a ``TreeNode``) and a list of source ``TreeNode`` objects and return a dict of int64 arrays
per supertree tip, in the order of ``supertree_arrays``' ``tips``: ``tx_trees``, ``tx_total``, ``tx_super``,
``tx_source``, ``tx_shared``, ``taxon_triplet_distance``.
"""

from __future__ import annotations

from itertools import combinations

import numpy as np
from score_reference import _leaf_sets, _preorder
from triplet_reference import _hierarchy, _outgroup, _ranges

from spectralclustersupertree_amd.tree import TreeNode

KEYS = ("tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared")


def _tips(supertree: TreeNode) -> list[str]:
    return [v.name for v in _preorder(supertree) if v.is_tip()]


def _result(out: dict) -> dict:
    out = {k: np.asarray(out[k], dtype=np.int64) for k in KEYS}
    out["taxon_triplet_distance"] = out["tx_super"] + out["tx_source"] - 2 * out["tx_shared"]
    return out


def brute_force(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    tips = _tips(supertree)
    index = {name: i for i, name in enumerate(tips)}
    out = {k: np.zeros(len(tips), dtype=np.int64) for k in KEYS}
    s_sets = list(_leaf_sets(_preorder(supertree)).values())
    for tree in trees:
        t_sets = _leaf_sets(_preorder(tree))
        leaves = t_sets[id(tree)]
        m = len(leaves)
        if m < 3:
            continue
        c_t = set(t_sets.values())
        c_s = {c & leaves for c in s_sets}
        for x in leaves:
            out["tx_trees"][index[x]] += 1
            out["tx_total"][index[x]] += (m - 1) * (m - 2) // 2
        for triple in combinations(sorted(leaves), 3):
            a, b = _outgroup(triple, c_s), _outgroup(triple, c_t)
            ids = [index[x] for x in triple]
            if a is not None:
                out["tx_super"][ids] += 1
            if b is not None:
                out["tx_source"][ids] += 1
            if a is not None and a == b:
                out["tx_shared"][ids] += 1
    return _result(out)


def _bincount(index: np.ndarray, value: np.ndarray, n: int) -> np.ndarray:
    """``np.bincount`` with non-negative int64 weights, exact: the weights go in as two 26-bit halves, whose float64
    sums stay below 2^53."""
    low = np.bincount(index, weights=value & ((1 << 26) - 1), minlength=n).astype(np.int64)
    high = np.bincount(index, weights=value >> 26, minlength=n).astype(np.int64)
    return low + (high << 26)


def _stab(m: int, lo: np.ndarray, hi: np.ndarray, value: np.ndarray) -> np.ndarray:
    """Per position of [0, m): the sum of ``value`` (>= 0) over the ranges [lo, hi) that hold it."""
    return np.cumsum(_bincount(lo, value, m + 1) - _bincount(hi, value, m + 1))[:m]


def _single(nodes: np.ndarray, parents: np.ndarray, m: int) -> np.ndarray:
    """Per position of one tree's leaf order: the resolved triples that hold the leaf."""
    if len(nodes) == 0:
        return np.zeros(m, dtype=np.int64)
    size = nodes[:, 1] - nodes[:, 0]
    a = (size - 1) * (parents[:, 1] - parents[:, 0] - size)
    b = size * (size - 1) // 2
    return _stab(m, nodes[:, 0], nodes[:, 1], a) - _stab(m, nodes[:, 0], nodes[:, 1], b) + _stab(
        m, parents[:, 0], parents[:, 1], b)


def quadratic(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    s_nodes = _preorder(supertree)
    tips = [v.name for v in s_nodes if v.is_tip()]
    s_index = {name: i for i, name in enumerate(tips)}
    out = {k: np.zeros(len(tips), dtype=np.int64) for k in KEYS}
    for tree in trees:
        t_nodes = _preorder(tree)
        t_tips = [v.name for v in t_nodes if v.is_tip()]
        m = len(t_tips)
        if m < 3:
            continue
        t_pos = {name: i for i, name in enumerate(t_tips)}
        ids_t = np.array([s_index[name] for name in t_tips], dtype=np.int64)  # taxon of T position
        y, py = _hierarchy(_ranges(t_nodes, t_pos), m)
        s_order = sorted(t_tips, key=s_index.__getitem__)
        z, pz = _hierarchy(_ranges(s_nodes, {name: k for k, name in enumerate(s_order)}), m)
        tp = np.array([t_pos[name] for name in s_order], dtype=np.int64)  # T position of S' leaf k
        ids_s = ids_t[tp]
        out["tx_trees"][ids_t] += 1
        out["tx_total"][ids_t] += (m - 1) * (m - 2) // 2
        out["tx_source"][ids_t] += _single(y, py, m)
        out["tx_super"][ids_s] += _single(z, pz, m)
        if len(y) == 0:
            continue
        shared = np.zeros(m, dtype=np.int64)  # per T position
        for (zl, zh), (pl, ph) in zip(z, pz):
            ind_z = np.zeros(m, dtype=np.int64)
            ind_z[tp[zl:zh]] = 1
            ind_p = np.zeros(m, dtype=np.int64)
            ind_p[tp[pl:ph]] = 1
            cz = np.concatenate([[0], np.cumsum(ind_z)])
            cp = np.concatenate([[0], np.cumsum(ind_p)])
            i_yz = cz[y[:, 1]] - cz[y[:, 0]]
            i_pyz = cz[py[:, 1]] - cz[py[:, 0]]
            i_ypz = cp[y[:, 1]] - cp[y[:, 0]]
            i_pypz = cp[py[:, 1]] - cp[py[:, 0]]
            j = i_pypz - i_ypz - i_pyz + i_yz
            sel = np.flatnonzero((i_yz >= 2) & (j != 0))  # (the pairs with a triple to hand out)
            if len(sel) == 0:
                continue
            a = (i_yz[sel] - 1) * j[sel]
            b = i_yz[sel] * (i_yz[sel] - 1) // 2
            inner = _stab(m, y[sel, 0], y[sel, 1], a)                                       # x in y ...
            outer = _stab(m, py[sel, 0], py[sel, 1], b) - _stab(m, y[sel, 0], y[sel, 1], b)   # x in py ∖ y ...
            shared += inner * ind_z + outer * (ind_p - ind_z)                               # ... and in z / pz ∖ z
        out["tx_shared"][ids_t] += shared
    return _result(out)
