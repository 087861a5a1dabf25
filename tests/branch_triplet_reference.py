"""Host references of the per-branch triplet support of ``score_supertree(..., branch_triplets=True)`` (helper module,
not collected).

For a quartet branch C of the supertree (children A, first in preorder, and B; sibling D -- ``concordance_reference``)
and a source tree T on L with A' = A ∩ L, B' = B ∩ L, D' = D ∩ L all non-empty, every triple (a in A', b in B',
d in D') is resolved ab|d by T (concordant: some cluster of T holds a and b but not d), ad|b (alt1), bd|a (alt2), or
it is a fan.

* ``brute_force``: triple by triple over Python frozensets, straight from the definitions (small cases only);
* ``node_sum``: with y over T's non-root clusters of two or more leaves, py the smallest cluster strictly above y and
  I(y, X) = |cl(y) ∩ X|: concordant = Σ_y I(y,A') I(y,B') (I(py,D') - I(y,D')), alt1 with (A', D', B'), alt2 with
  (B', D', A') -- T's clusters as ranges of its leaf order and one prefix-count vector per set, in numpy.  Fast enough
  for trees of a few thousand leaves.

Both take the supertree (a ``TreeNode``) and a list of source ``TreeNode`` objects and return a dict of int64 arrays:
``n_bt_total``, ``n_bt_concordant``, ``n_bt_alternative`` per tree and ``bt_total``, ``bt_concordant``, ``bt_alt1``,
``bt_alt2`` per supertree node in ``TreeNode.to_flat`` order.
"""

from __future__ import annotations

import numpy as np
from concordance_reference import quartet_branches
from score_reference import _leaf_sets, _preorder
from triplet_reference import _hierarchy, _ranges

from spectralclustersupertree_amd.tree import TreeNode

PER_TREE = ("n_bt_total", "n_bt_concordant", "n_bt_alternative")
PER_NODE = ("bt_total", "bt_concordant", "bt_alt1", "bt_alt2")


def _empty(n_trees: int, n_nodes: int) -> dict:
    out = {k: np.zeros(n_trees, dtype=np.int64) for k in PER_TREE}
    out.update({k: np.zeros(n_nodes, dtype=np.int64) for k in PER_NODE})
    return out


def _branches(supertree: TreeNode):
    s_nodes = _preorder(supertree)
    s_sets = _leaf_sets(s_nodes)
    return len(s_nodes), [(i, s_sets[id(a)], s_sets[id(b)], s_sets[id(d)])
                          for i, a, b, d in quartet_branches(supertree)]


def _add(out: dict, t: int, i: int, total: int, con: int, alt1: int, alt2: int) -> None:
    out["bt_total"][i] += total
    out["bt_concordant"][i] += con
    out["bt_alt1"][i] += alt1
    out["bt_alt2"][i] += alt2
    out["n_bt_total"][t] += total
    out["n_bt_concordant"][t] += con
    out["n_bt_alternative"][t] += alt1 + alt2


def brute_force(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    n_nodes, branches = _branches(supertree)
    out = _empty(len(trees), n_nodes)
    for t, tree in enumerate(trees):
        t_sets = _leaf_sets(_preorder(tree))
        leaves = t_sets[id(tree)]
        clusters = set(t_sets.values())
        for i, a_set, b_set, d_set in branches:
            a_set, b_set, d_set = a_set & leaves, b_set & leaves, d_set & leaves
            if not (a_set and b_set and d_set):
                continue
            con = alt1 = alt2 = 0
            for a in a_set:
                for b in b_set:
                    for d in d_set:
                        con += any(a in c and b in c and d not in c for c in clusters)
                        alt1 += any(a in c and d in c and b not in c for c in clusters)
                        alt2 += any(b in c and d in c and a not in c for c in clusters)
            _add(out, t, i, len(a_set) * len(b_set) * len(d_set), con, alt1, alt2)
    return out


def node_sum(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    n_nodes, branches = _branches(supertree)
    out = _empty(len(trees), n_nodes)
    for t, tree in enumerate(trees):
        t_nodes = _preorder(tree)
        t_tips = [v.name for v in t_nodes if v.is_tip()]
        m = len(t_tips)
        if m < 3:
            continue
        t_pos = {name: k for k, name in enumerate(t_tips)}
        leaves = frozenset(t_tips)
        y, py = _hierarchy(_ranges(t_nodes, t_pos), m)

        def inside(names, t_pos=t_pos, m=m, y=y, py=py):
            """I(y, X) and I(py, X) - I(y, X) for every y, X = ``names``."""
            ind = np.zeros(m + 1, dtype=np.int64)
            ind[[t_pos[x] + 1 for x in names]] = 1
            c = np.cumsum(ind)
            own = c[y[:, 1]] - c[y[:, 0]]
            return own, c[py[:, 1]] - c[py[:, 0]] - own

        for i, a_set, b_set, d_set in branches:
            a_set, b_set, d_set = a_set & leaves, b_set & leaves, d_set & leaves
            if not (a_set and b_set and d_set):
                continue
            (ia, oa), (ib, ob), (id_, od) = inside(a_set), inside(b_set), inside(d_set)
            _add(out, t, i, len(a_set) * len(b_set) * len(d_set), int((ia * ib * od).sum()),
                 int((ia * id_ * ob).sum()), int((ib * id_ * oa).sum()))
    return out
