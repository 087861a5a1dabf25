"""Host reference of the branch concordance counts of ``score_supertree(..., concordance=True)`` (helper module, not
collected).

* ``brute_force``: the definitions over Python frozensets.  A node C of the supertree is a quartet branch when it is
  not the root, has exactly two children A (first in preorder) and B, and its parent has exactly two children, C and
  its sibling D.  A source tree T on L is decisive for C when A ∩ L, B ∩ L and D ∩ L are non-empty, and then
  concordant / alt1 / alt2 when (A ∪ B) ∩ L / (A ∪ D) ∩ L / (B ∪ D) ∩ L is a cluster of T.
* ``planted``: a source tree that agrees with the supertree up to a few nearest-neighbour interchanges and some
  contracted edges, so that every category occurs (independent random trees are almost never concordant or alt).

``brute_force`` takes the supertree (a ``TreeNode``) and a list of source ``TreeNode`` objects and returns a dict of
int64 arrays: ``n_decisive``, ``n_concordant``, ``n_alternative`` per tree, ``decisive``, ``concordant``, ``alt1``,
``alt2`` per supertree node in ``TreeNode.to_flat`` order, and the bool mask ``quartet_branch``.
"""

from __future__ import annotations

import numpy as np
from conflict_reference import contract
from score_reference import _leaf_sets, _preorder

from spectralclustersupertree_amd.tree import TreeNode

PER_TREE = ("n_decisive", "n_concordant", "n_alternative")
PER_NODE = ("decisive", "concordant", "alt1", "alt2")


def quartet_branches(supertree: TreeNode) -> list[tuple[int, TreeNode, TreeNode, TreeNode]]:
    """``(preorder index of C, A, B, D)`` for every quartet branch C."""
    nodes = _preorder(supertree)
    index = {id(v): i for i, v in enumerate(nodes)}
    out = []
    for par in nodes:
        if len(par.children) != 2:
            continue
        for c, d in (par.children, par.children[::-1]):
            if len(c.children) == 2:
                out.append((index[id(c)], c.children[0], c.children[1], d))
    return sorted(out, key=lambda r: r[0])


def brute_force(supertree: TreeNode, trees: list[TreeNode]) -> dict:
    s_nodes = _preorder(supertree)
    s_sets = _leaf_sets(s_nodes)
    branches = [(i, s_sets[id(a)], s_sets[id(b)], s_sets[id(d)]) for i, a, b, d in quartet_branches(supertree)]
    out = {k: np.zeros(len(trees), dtype=np.int64) for k in PER_TREE}
    out.update({k: np.zeros(len(s_nodes), dtype=np.int64) for k in PER_NODE})
    out["quartet_branch"] = np.zeros(len(s_nodes), dtype=bool)
    for i, _, _, _ in branches:
        out["quartet_branch"][i] = True
    for t, tree in enumerate(trees):
        t_sets = _leaf_sets(_preorder(tree))
        leaves = t_sets[id(tree)]
        clusters = set(t_sets.values())
        for i, a, b, d in branches:
            a, b, d = a & leaves, b & leaves, d & leaves
            if not (a and b and d):
                continue
            out["decisive"][i] += 1
            out["n_decisive"][t] += 1
            if a | b in clusters:
                out["concordant"][i] += 1
                out["n_concordant"][t] += 1
            if a | d in clusters:
                out["alt1"][i] += 1
                out["n_alternative"][t] += 1
            if b | d in clusters:
                out["alt2"][i] += 1
                out["n_alternative"][t] += 1
    return out


def nni(tree: TreeNode, rs: np.random.RandomState) -> bool:
    """One random rooted nearest-neighbour interchange in place: a child of an inner non-root node changes places
    with one of that node's siblings.  False when the tree has no such node."""
    spots = [(par, v) for par in _preorder(tree) for v in par.children if v.children and len(par.children) > 1]
    if not spots:
        return False
    par, v = spots[int(rs.randint(len(spots)))]
    sibs = [s for s in par.children if s is not v]
    s = sibs[int(rs.randint(len(sibs)))]
    i, j = int(rs.randint(len(v.children))), par.children.index(s)
    v.children[i], par.children[j] = par.children[j], v.children[i]
    v.children[i].parent, par.children[j].parent = v, par
    return True


def planted(rs: np.random.RandomState, supertree: TreeNode, names: list[str], frac: float, moves: int,
            share: float) -> TreeNode:
    """The supertree restricted to a random ``frac`` of ``names`` (at least 3), after ``moves`` random rooted NNIs
    and with a random ``share`` of its inner edges contracted."""
    k = min(len(names), max(3, int(round(frac * len(names)))))
    subset = names if k == len(names) else list(rs.choice(names, size=k, replace=False))
    tree = supertree.get_sub_tree(subset).copy()
    for _ in range(moves):
        nni(tree, rs)
    return contract(tree, rs, share)
