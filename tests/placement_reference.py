"""Host references of the taxon placement support of ``score_supertree(..., placements=...)`` (helper module, not
collected).

* ``brute_force``: the cluster definition of ``score.py``'s docstring over Python sets -- for every query taxon x and
  every node v the clusters of "S with x pruned and regrafted on the edge above v", restricted to every source that
  holds x, and every triple {x, a, b} of that source against them (small cases only);
* ``recurrence``: the node-local formula in numpy -- per (source, x) the groups of x in the source, their leaf counts
  inside every supertree node by prefix sums over the supertree's leaf order, and the root-path sums as a difference
  array over the preorder.

Both take the supertree (a ``TreeNode``), a list of source ``TreeNode`` objects and the query tip names, and return a
dict of int64 arrays: ``pl_trees``, ``pl_total``, ``pl_source`` per query, ``pl_super``, ``pl_shared`` and
``placement_distance`` per query and supertree node (preorder, ``TreeNode.to_flat`` order).
"""

from __future__ import annotations

from itertools import combinations

import numpy as np
from score_reference import _leaf_sets, _preorder
from triplet_reference import _outgroup

from spectralclustersupertree_amd.tree import TreeNode


def _result(trees, total, source, sup, shared) -> dict:
    out = {
        "pl_trees": np.asarray(trees, dtype=np.int64),
        "pl_total": np.asarray(total, dtype=np.int64),
        "pl_source": np.asarray(source, dtype=np.int64),
        "pl_super": np.asarray(sup, dtype=np.int64).reshape(len(trees), -1),
        "pl_shared": np.asarray(shared, dtype=np.int64).reshape(len(trees), -1),
    }
    out["placement_distance"] = out["pl_super"] + out["pl_source"][:, None] - 2 * out["pl_shared"]
    return out


def _parents(nodes: list[TreeNode]) -> list[int]:
    index = {id(v): i for i, v in enumerate(nodes)}
    parent = [-1] * len(nodes)
    for i, v in enumerate(nodes):
        for c in v.children:
            parent[index[id(c)]] = i
    return parent


def regrafted_clusters(supertree: TreeNode, x: str, v: int) -> set:
    """The clusters of S_{x -> v}: S with the tip ``x`` pruned and regrafted on the edge above preorder node ``v``."""
    nodes = _preorder(supertree)
    sets = _leaf_sets(nodes)
    parent = _parents(nodes)
    above = set()
    u = parent[v]
    while u >= 0:
        above.add(u)
        u = parent[u]
    out = set()
    for i, node in enumerate(nodes):
        c = sets[id(node)] - {x}
        out.add(c | {x} if i in above else c)
    out.add((sets[id(nodes[v])] - {x}) | {x})
    out.discard(frozenset())
    return out


def brute_force(supertree: TreeNode, trees: list[TreeNode], queries: list[str]) -> dict:
    n_nodes = len(_preorder(supertree))
    nq = len(queries)
    n_trees, total, source = [0] * nq, [0] * nq, [0] * nq
    sup = np.zeros((nq, n_nodes), dtype=np.int64)
    shared = np.zeros((nq, n_nodes), dtype=np.int64)
    t_info = []
    for tree in trees:
        t_sets = _leaf_sets(_preorder(tree))
        t_info.append((t_sets[id(tree)], set(t_sets.values())))
    for i, x in enumerate(queries):
        held = [(leaves, c_t) for leaves, c_t in t_info if x in leaves and len(leaves) >= 3]
        for leaves, c_t in held:
            m = len(leaves)
            n_trees[i] += 1
            total[i] += (m - 1) * (m - 2) // 2
        # T's own answer for every triple with x, once per source
        in_t = []
        for leaves, c_t in held:
            pairs = list(combinations(sorted(leaves - {x}), 2))
            answers = [_outgroup((x, a, b), c_t) for a, b in pairs]
            source[i] += sum(a is not None for a in answers)
            in_t.append((leaves, pairs, answers))
        for v in range(n_nodes):
            clusters = regrafted_clusters(supertree, x, v)
            for leaves, pairs, answers in in_t:
                c_s = {c & leaves for c in clusters}
                c_s = [c for c in c_s if len(c) >= 2]  # (a smaller set holds no two taxa of a triple)
                for (a, b), ans in zip(pairs, answers):
                    got = _outgroup((x, a, b), c_s)
                    sup[i, v] += got is not None
                    shared[i, v] += got is not None and got == ans
    return _result(n_trees, total, source, sup, shared)


def recurrence(supertree: TreeNode, trees: list[TreeNode], queries: list[str]) -> dict:
    s_nodes = _preorder(supertree)
    n_nodes = len(s_nodes)
    parent = np.array(_parents(s_nodes), dtype=np.int64)
    tips = [v.name for v in s_nodes if v.is_tip()]
    s_pos = {name: k for k, name in enumerate(tips)}
    n_tips = len(tips)
    lo = np.full(n_nodes, n_tips, dtype=np.int64)
    hi = np.full(n_nodes, -1, dtype=np.int64)
    end = np.arange(1, n_nodes + 1, dtype=np.int64)
    k = 0
    for i, v in enumerate(s_nodes):
        if v.is_tip():
            lo[i] = hi[i] = k
            k += 1
    for i in range(n_nodes - 1, 0, -1):
        p = parent[i]
        lo[p] = min(lo[p], lo[i])
        hi[p] = max(hi[p], hi[i])
        end[p] = max(end[p], end[i])
    nq = len(queries)
    n_trees, total, source = [0] * nq, [0] * nq, [0] * nq
    sup = np.zeros((nq, n_nodes), dtype=np.int64)
    shared = np.zeros((nq, n_nodes), dtype=np.int64)
    qi = {x: i for i, x in enumerate(queries)}

    def path_sums(root_value, strict, own):
        """value(v) = root_value + the sums of strict[q] over v's strict ancestors q and of own[u] over the path
        (root, v]: one mark per node on its preorder range, one prefix sum."""
        mark = own.copy()
        mark[1:] += strict[parent[1:]]
        mark[0] = root_value
        d = np.zeros(n_nodes + 1, dtype=np.int64)
        np.add.at(d, np.arange(n_nodes), mark)
        np.add.at(d, end, -mark)
        return np.cumsum(d)[:n_nodes]

    for tree in trees:
        t_nodes = _preorder(tree)
        t_tips = [v.name for v in t_nodes if v.is_tip()]
        m = len(t_tips)
        if m < 3:
            continue
        held = [x for x in t_tips if x in qi]
        if not held:
            continue
        t_parent = _parents(t_nodes)
        t_sets = _leaf_sets(t_nodes)
        tip_node = {v.name: i for i, v in enumerate(t_nodes) if v.is_tip()}
        kids = [[] for _ in t_nodes]
        for i in range(1, len(t_nodes)):
            kids[t_parent[i]].append(i)
        for x in held:
            i = qi[x]
            n_trees[i] += 1
            total[i] += (m - 1) * (m - 2) // 2
            # the groups of x: the subtrees hanging off its root path, with the level of their parent (0 = deepest);
            # unary nodes repeat a cluster and add no group
            gid = np.full(n_tips, -1, dtype=np.int64)
            level = []
            u, lev = tip_node[x], 0
            while t_parent[u] >= 0:
                p = t_parent[u]
                others = [c for c in kids[p] if c != u]
                for c in others:
                    for name in t_sets[id(t_nodes[c])]:
                        gid[s_pos[name]] = len(level)
                    level.append(lev)
                lev += bool(others)
                u = p
            g = len(level)
            level = np.array(level, dtype=np.int64)
            sizes = np.bincount(gid[gid >= 0], minlength=g)
            # pairs in different groups of one level are fans of T
            fans = 0
            for lv in range(int(level.max()) + 1 if g else 0):
                s = sizes[level == lv]
                fans += (int(s.sum()) ** 2 - int((s * s).sum())) // 2
            source[i] += (m - 1) * (m - 2) // 2 - fans
            # cnt[g][q] = leaves of group g inside supertree node q; below[g][q] = those of the groups inside py
            ind = np.zeros((g, n_tips + 1), dtype=np.int64)
            sel = np.flatnonzero(gid >= 0)
            ind[gid[sel], sel + 1] = 1
            pre = np.cumsum(ind, axis=1)
            cnt = pre[:, hi + 1] - pre[:, lo]                      # [g][node]
            per_level = np.zeros((int(level.max()) + 1 if g else 0, n_nodes), dtype=np.int64)
            np.add.at(per_level, level, cnt)
            below = np.cumsum(per_level, axis=0)[level]            # [g][node]: |q ∩ py| without x
            size = cnt.sum(axis=0)
            a_sh = (cnt * (cnt - 1) // 2).sum(axis=0)
            a_su = size * (size - 1) // 2
            kid_sh = np.zeros(n_nodes, dtype=np.int64)
            kid_su = np.zeros(n_nodes, dtype=np.int64)
            np.add.at(kid_sh, parent[1:], a_sh[1:])
            np.add.at(kid_su, parent[1:], a_su[1:])
            par = np.maximum(parent, 0)
            x_sh = (cnt * ((size[par] - below[:, par]) - (size - below))).sum(axis=0)
            x_su = size * (size[par] - size)
            shared[i] += path_sums(a_sh[0], kid_sh - a_sh, x_sh)
            sup[i] += path_sums(a_su[0], kid_su - a_su, x_su)
    return _result(n_trees, total, source, sup, shared)
