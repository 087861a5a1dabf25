"""Host references of the clade placement support of ``score_supertree(..., clade_placements=...)`` (helper module,
not collected).

* ``brute_force``: the cluster definition of ``score.py``'s docstring over Python sets -- for every query node q and
  every node v the clusters of "S with the subtree of q pruned and regrafted on the edge above v", restricted to every
  source the clade crosses, and every crossing triple of that source against them (small cases only);
* ``edit_and_rescore``: no clade arithmetic at all -- ``SupertreeScore.regraft_clade`` builds the moved tree and
  ``triplet_reference.brute_force`` scores it and the supertree over *all* triples; the differences of the summed
  ``t_super`` and ``t_shared`` are what the move changes, and the sources cut in two at the clade give the values at
  the clade's own place.

* ``composed``: the same numbers for larger cases, put together from the older references -- a source cut down to
  R ∪ {x} gives, through ``placement_reference.recurrence`` for x, the triples with x alone in the clade on every
  edge; the values at the clade's own place come from ``triplet_reference.quadratic`` on the source and its two
  sides, and fix the part that no edge changes.

``brute_force`` and ``composed`` take the supertree (a ``TreeNode``), a list of source ``TreeNode`` objects and the query
nodes (preorder indices, ``TreeNode.to_flat`` order) and return a dict of int64 arrays: ``cp_trees``, ``cp_total``,
``cp_source`` per query, ``cp_super``, ``cp_shared`` and ``clade_placement_distance`` per query and supertree node.
``edit_and_rescore`` returns ``d_super`` and ``d_shared`` per query and node: by identity 2 of DESIGN.md section 23
they equal ``cp_super[i, v] - cp_super[i, q_i]`` and ``cp_shared[i, v] - cp_shared[i, q_i]``; and ``own_super``,
``own_source``, ``own_shared`` per query, the values at the clade's own place: all triples less those of the sources
restricted to the clade and to its complement.
"""

from __future__ import annotations

from itertools import combinations
from math import comb

import numpy as np
import placement_reference as pr
import triplet_reference as tr
from placement_reference import _parents
from score_reference import _leaf_sets, _preorder
from triplet_reference import _outgroup

from spectralclustersupertree_amd.score import SupertreeScore
from spectralclustersupertree_amd.tree import TreeNode

KEYS = ("cp_trees", "cp_total", "cp_source", "cp_super", "cp_shared", "clade_placement_distance")


def _result(trees, total, source, sup, shared) -> dict:
    out = {
        "cp_trees": np.asarray(trees, dtype=np.int64),
        "cp_total": np.asarray(total, dtype=np.int64),
        "cp_source": np.asarray(source, dtype=np.int64),
        "cp_super": np.asarray(sup, dtype=np.int64).reshape(len(trees), -1),
        "cp_shared": np.asarray(shared, dtype=np.int64).reshape(len(trees), -1),
    }
    out["clade_placement_distance"] = out["cp_super"] + out["cp_source"][:, None] - 2 * out["cp_shared"]
    return out


def subtree(parent: list[int], q: int) -> set:
    """The preorder nodes of the subtree of ``q``, ``q`` included."""
    inside = {q}
    for i in range(q + 1, len(parent)):
        if parent[i] in inside:
            inside.add(i)
    return inside


def regrafted_clusters(supertree: TreeNode, q: int, v: int, defect: str | None = None) -> set:
    """The clusters of S_{q -> v}: S with the subtree of preorder node ``q`` pruned and regrafted on the edge above
    preorder node ``v``; S's own clusters when ``v`` lies in that subtree.  ``defect="ancestors"`` plants a mistake
    (tests): the clusters above the clade's old place keep the clade."""
    nodes = _preorder(supertree)
    sets = _leaf_sets(nodes)
    parent = _parents(nodes)
    inside = subtree(parent, q)
    if v in inside:
        return set(sets.values())
    clade = sets[id(nodes[q])]
    above = set()
    u = parent[v]
    while u >= 0:
        above.add(u)
        u = parent[u]
    out = set()
    for i, node in enumerate(nodes):
        if i in inside:
            out.add(sets[id(node)])
        elif i in above:
            out.add(sets[id(node)] | clade)
        elif defect == "ancestors":
            out.add(sets[id(node)])
        else:
            out.add(sets[id(node)] - clade)
    out.add(sets[id(nodes[v])] | clade)
    out.discard(frozenset())
    return out


def brute_force(supertree: TreeNode, trees: list[TreeNode], queries: list[int], defect: str | None = None) -> dict:
    """``defect`` plants a mistake (tests): ``"ancestors"`` (``regrafted_clusters``) or ``"two_in_clade"``, which
    leaves out the triples with two taxa in the clade."""
    nodes = _preorder(supertree)
    sets = _leaf_sets(nodes)
    n_nodes = len(nodes)
    nq = len(queries)
    n_trees, total, source = [0] * nq, [0] * nq, [0] * nq
    sup = np.zeros((nq, n_nodes), dtype=np.int64)
    shared = np.zeros((nq, n_nodes), dtype=np.int64)
    t_info = []
    for tree in trees:
        t_sets = _leaf_sets(_preorder(tree))
        t_info.append((t_sets[id(tree)], set(t_sets.values())))
    for i, q in enumerate(queries):
        clade = sets[id(nodes[q])]
        crossed = []
        for leaves, c_t in t_info:
            inside, rest = leaves & clade, leaves - clade
            if len(leaves) < 3 or not inside or not rest:
                continue
            n_trees[i] += 1
            triples = [t for t in combinations(sorted(leaves), 3) if 0 < sum(x in clade for x in t) < 3]
            total[i] += len(triples)
            if defect == "two_in_clade":
                triples = [t for t in triples if sum(x in clade for x in t) == 1]
            answers = [_outgroup(t, c_t) for t in triples]
            source[i] += sum(a is not None for a in answers)
            crossed.append((leaves, triples, answers))
        memo: dict = {}
        for v in range(n_nodes):
            clusters = regrafted_clusters(supertree, q, v, defect)
            for k, (leaves, triples, answers) in enumerate(crossed):
                c_s = frozenset(c & leaves for c in clusters if len(c & leaves) >= 2)
                if (k, c_s) not in memo:
                    got = [_outgroup(t, c_s) for t in triples]
                    memo[k, c_s] = (sum(g is not None for g in got),
                                    sum(g is not None and g == a for g, a in zip(got, answers)))
                sup[i, v] += memo[k, c_s][0]
                shared[i, v] += memo[k, c_s][1]
    return _result(n_trees, total, source, sup, shared)


def total_closed_form(supertree: TreeNode, trees: list[TreeNode], queries: list[int]) -> tuple[list, list]:
    """``cp_trees`` and ``cp_total`` from the sizes alone: C(m, 3) - C(|Q'|, 3) - C(|R|, 3) per crossed source."""
    nodes = _preorder(supertree)
    sets = _leaf_sets(nodes)
    n_trees, total = [], []
    for q in queries:
        clade = sets[id(nodes[q])]
        nt = tot = 0
        for tree in trees:
            leaves = set(tree.get_tip_names())
            a, m = len(leaves & clade), len(leaves)
            if m >= 3 and 0 < a < m:
                nt += 1
                tot += comb(m, 3) - comb(a, 3) - comb(m - a, 3)
        n_trees.append(nt)
        total.append(tot)
    return n_trees, total


def _restricted(tree: TreeNode, keep) -> TreeNode | None:
    """``tree`` without the tips outside ``keep`` and the nodes they leave empty; None when nothing is left (no
    recursion: a caterpillar is as deep as it has leaves)."""
    made: dict = {}
    for node in reversed(_preorder(tree)):
        if node.is_tip():
            made[id(node)] = TreeNode(node.name) if node.name in keep else None
        else:
            kids = [made[id(c)] for c in node.children if made[id(c)] is not None]
            made[id(node)] = TreeNode(None, kids) if kids else None
    return made[id(tree)]


def _own_terms(supertree: TreeNode, trees: list[TreeNode], clade: frozenset, base: dict) -> tuple[int, int, int]:
    """The crossing triples S resolves, T resolves and both resolve alike, summed over the sources: all triples less
    those inside the clade and those outside it, each scored on the source restricted to that side."""
    out = [int(base[k].sum()) for k in ("t_super", "t_source", "t_shared")]
    for tree in trees:
        leaves = set(tree.get_tip_names())
        for side in (leaves & clade, leaves - clade):
            part = _restricted(tree, side)
            if part is not None:
                got = tr.brute_force(supertree, [part])
                for j, k in enumerate(("t_super", "t_source", "t_shared")):
                    out[j] -= int(got[k][0])
    return out[0], out[1], out[2]


def edit_and_rescore(supertree: TreeNode, trees: list[TreeNode], queries: list[int]) -> dict:
    view = SupertreeScore(supertree, None, None, None, None, None, None)
    nodes = _preorder(supertree)
    parent = _parents(nodes)
    n_nodes = len(nodes)
    base = tr.brute_force(supertree, trees)
    base_super, base_shared = int(base["t_super"].sum()), int(base["t_shared"].sum())
    d_super = np.zeros((len(queries), n_nodes), dtype=np.int64)
    d_shared = np.zeros((len(queries), n_nodes), dtype=np.int64)
    memo: dict = {}
    sets = _leaf_sets(nodes)
    own = np.zeros((len(queries), 3), dtype=np.int64)
    for i, q in enumerate(queries):
        inside = subtree(parent, q)
        own[i] = _own_terms(supertree, trees, sets[id(nodes[q])], base)
        for v in range(n_nodes):
            if v in inside:  # (no move)
                continue
            moved = view.regraft_clade(q, v)
            key = frozenset(_leaf_sets(_preorder(moved)).values())
            if key not in memo:
                got = tr.brute_force(moved, trees)
                memo[key] = (int(got["t_super"].sum()), int(got["t_shared"].sum()),
                             got["t_source"].tolist() == base["t_source"].tolist())
            assert memo[key][2], "t_source moved"
            d_super[i, v] = memo[key][0] - base_super
            d_shared[i, v] = memo[key][1] - base_shared
    return {"d_super": d_super, "d_shared": d_shared, "own_super": own[:, 0], "own_source": own[:, 1],
            "own_shared": own[:, 2]}


def composed(supertree: TreeNode, trees: list[TreeNode], queries: list[int]) -> dict:
    nodes = _preorder(supertree)
    sets = _leaf_sets(nodes)
    n_nodes = len(nodes)
    nq = len(queries)
    n_trees, total = total_closed_form(supertree, trees, queries)
    source = [0] * nq
    sup = np.zeros((nq, n_nodes), dtype=np.int64)
    shared = np.zeros((nq, n_nodes), dtype=np.int64)
    whole = tr.quadratic(supertree, trees)
    for i, q in enumerate(queries):
        clade = sets[id(nodes[q])]
        own = dict.fromkeys(("t_super", "t_source", "t_shared"), 0)
        sides, singled = [], []
        for t, tree in enumerate(trees):
            leaves = set(tree.get_tip_names())
            inside, rest = leaves & clade, leaves - clade
            if len(leaves) < 3 or not inside or not rest:
                continue
            for k in own:
                own[k] += int(whole[k][t])
            sides += [_restricted(tree, inside), _restricted(tree, rest)]
            singled += [_restricted(tree, rest | {x}) for x in inside]  # (each holds one taxon of the clade)
        if not sides:
            continue
        got = tr.quadratic(supertree, sides)
        for k in own:
            own[k] -= int(got[k].sum())
        got = pr.recurrence(supertree, singled, sorted(clade))
        rows_super, rows_shared = got["pl_super"].sum(axis=0), got["pl_shared"].sum(axis=0)
        source[i] = own["t_source"]
        sup[i] = rows_super + (own["t_super"] - rows_super[q])
        shared[i] = rows_shared + (own["t_shared"] - rows_shared[q])
    return _result(n_trees, total, source, sup, shared)
