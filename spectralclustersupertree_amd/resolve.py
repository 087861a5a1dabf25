"""``resolve_polytomies``: the polytomies of a supertree resolved by what the source trees' rooted triples say about
their children.

For a polytomy p with children c_0 .. c_{k-1}, ``scs_score_polytomies`` returns two k x k x k tensors over the sources
that hold leaves of three or more children: ``py_total[i][j][l]`` (i < j, l not in {i, j}), the triples with a leaf
below c_i, one below c_j and one below c_l -- all fans in the supertree -- and ``py_joint[i][j][l]``, those of them the
source resolves with the first two together.  Putting two groups G and H of children under one new node (a third group
remaining) resolves exactly the triples (a below G, b below H, d below p and neither), so the summed triplet distance
falls by

    gain(G, H) = 2 M(G, H) - N(G, H),    M, N = the sums of py_joint, py_total over i in G, j in H, l in neither

(index pairs ordered so that i < j).  The gain is exact on the current partition and merges at different polytomies
touch different triples, so a whole agglomeration is a host computation on the tensors: no rescoring.

The agglomeration is greedy: while three or more groups remain, the pair of groups with the largest gain >= ``min_gain``
is merged; ties go to the smallest original child position of G, then of H (groups are kept in the order of their
smallest child position, G before H).  The merged group's node holds the two groups' nodes in that order.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from spectralclustersupertree_amd import score as _score
from spectralclustersupertree_amd.score import _leaf_ranges, _preorder, _resident_tables, supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode


def _pair_tensor(total, joint) -> np.ndarray:
    """A[i][j][l] = 2 joint - total of the unordered pair {i, j} and the third child l, filled for both orders."""
    a = 2 * np.asarray(joint, dtype=np.int64) - np.asarray(total, dtype=np.int64)
    return a + a.transpose(1, 0, 2)


def merge_gain(total, joint, G, H) -> int:
    """2 M(G, H) - N(G, H) on the tensors of one polytomy: ``G`` and ``H`` are disjoint non-empty lists of child
    positions that leave at least one child out (``ValueError`` otherwise)."""
    k = len(total)
    g, h = sorted({int(i) for i in G}), sorted({int(i) for i in H})
    if not g or not h or len(g) != len(list(G)) or len(h) != len(list(H)) or set(g) & set(h):
        msg = "G and H must be two disjoint, non-empty sets of child positions"
        raise ValueError(msg)
    if min(g + h) < 0 or max(g + h) >= k or len(g) + len(h) >= k:
        msg = f"G and H must lie in [0, {k}) and leave a child out"
        raise ValueError(msg)
    rest = [x for x in range(k) if x not in g and x not in h]
    return int(_pair_tensor(total, joint)[np.ix_(g, h, rest)].sum())


def agglomerate(total, joint, min_gain: int = 1) -> list[tuple]:
    """The greedy agglomeration of one polytomy (module docstring): ``[(G, H, gain)]`` in the order the merges are
    made, G and H sorted lists of original child positions."""
    b = _pair_tensor(total, joint)  # b[g][h][r]: the sum of A over the members of the groups g, h, r
    groups = [[i] for i in range(len(b))]
    merges = []
    while len(groups) >= 3:
        n = len(groups)
        gain = b.sum(axis=2) - b[np.arange(n)[:, None], np.arange(n)[None, :], np.arange(n)[:, None]] \
            - b[np.arange(n)[:, None], np.arange(n)[None, :], np.arange(n)[None, :]]
        best, at = None, None
        for g in range(n):
            for h in range(g + 1, n):
                if gain[g, h] >= min_gain and (best is None or gain[g, h] > best):
                    best, at = int(gain[g, h]), (g, h)
        if at is None:
            break
        g, h = at
        merges.append((list(groups[g]), list(groups[h]), best))
        groups[g] = sorted(groups[g] + groups[h])
        del groups[h]
        for axis in range(3):
            idx = [slice(None)] * 3
            src = list(idx)
            idx[axis], src[axis] = g, h
            b[tuple(idx)] += b[tuple(src)]
            b = np.delete(b, h, axis=axis)
    return merges


def apply_merges(tree: TreeNode, plan: dict) -> TreeNode:
    """A copy of ``tree`` with the merges ``plan[node] = [(G, H, gain)]`` (preorder index -> ``agglomerate``'s list)
    made at every polytomy: all indices refer to ``tree`` as given."""
    out = tree.copy()
    nodes = _preorder(out)
    for node, merges in plan.items():
        top = nodes[int(node)]
        group = {i: c for i, c in enumerate(top.children)}  # smallest child position -> the group's node
        for g, h, _ in merges:
            new = TreeNode(None)
            new.append(group[g[0]])
            new.append(group.pop(h[0]))
            group[g[0]] = new
        top.children = []
        for i in sorted(group):
            top.append(group[i])
    return out


@dataclass
class ResolveResult:
    """What ``resolve_polytomies`` did.  ``merges``: dicts with ``node`` (the polytomy, a preorder index in the input
    tree), ``groups`` (the two lists of child positions), ``gain`` and ``tips`` (of the new node), polytomy by
    polytomy in the order the merges were made.  ``skipped``: the polytomies that were not scored (``node``,
    ``degree``, ``reason``).  ``predicted_distance`` = ``initial_distance`` - the sum of the gains: the summed triplet
    distance of ``supertree``, known without scoring it."""

    supertree: TreeNode
    initial_distance: int | None
    predicted_distance: int | None
    merges: list = field(default_factory=list)
    skipped: list = field(default_factory=list)
    timings: dict = field(default_factory=dict)

    def table(self) -> str:
        """One TSV row per merge: node, group_a, group_b (child positions, comma-separated), tips, gain,
        distance_after (empty when the initial distance is not known)."""
        rows = ["node\tgroup_a\tgroup_b\ttips\tgain\tdistance_after"]
        left = self.initial_distance
        for m in self.merges:
            if left is not None:
                left -= m["gain"]
            a, b = (",".join(str(i) for i in g) for g in m["groups"])
            rows.append(f"{m['node']}\t{a}\t{b}\t{m['tips']}\t{m['gain']}\t{'' if left is None else left}")
        return "\n".join(rows) + "\n"


def resolve_from_tensors(supertree: TreeNode, py_nodes, py_total, py_joint, skipped, initial, min_gain: int = 1,
                         timings: dict | None = None) -> ResolveResult:
    """The agglomeration of every scored polytomy and the resolved tree, from the outputs of ``scs_score_polytomies``
    on ``supertree``."""
    parent = np.asarray(supertree.to_flat()[0], dtype=np.int64)
    lo, hi = _leaf_ranges(parent)
    plan, merges = {}, []
    for q, node in enumerate(py_nodes):
        done = agglomerate(py_total[q], py_joint[q], min_gain)
        if not done:
            continue
        plan[int(node)] = done
        kids = np.flatnonzero(parent == node)
        size = hi[kids] - lo[kids] + 1
        for g, h, gain in done:
            merges.append({"node": int(node), "groups": (g, h), "gain": gain, "tips": int(size[g + h].sum())})
    predicted = None if initial is None else int(initial) - sum(m["gain"] for m in merges)
    return ResolveResult(apply_merges(supertree, plan), None if initial is None else int(initial), predicted, merges,
                         list(skipped), timings or {})


def resolve_polytomies(supertree: TreeNode, trees, *, max_degree: int = 64, min_gain: int = 1,
                       device=None) -> ResolveResult:
    """Resolves the polytomies of ``supertree`` (every node with 3 to ``max_degree`` <= 64 children) by the greedy
    agglomeration of the module docstring, from one ``scs_score_polytomies`` call; ``scs_score_triplets`` gives
    ``initial_distance``.  ``trees`` as for ``score_supertree`` (either input path, the same ``ValueError``s, weights
    ignored).  Only merges that lower the summed triplet distance by ``min_gain`` or more are made, so with the default
    the distance never rises and a polytomy no source is decisive for stays.  The input tree is not modified."""
    import time

    if not 3 <= int(max_degree) <= _score.PY_MAX_DEGREE:
        msg = f"max_degree = {max_degree} is not in [3, {_score.PY_MAX_DEGREE}]"
        raise ValueError(msg)
    parent, taxon, tips = supertree_arrays(supertree)
    index = {name: i for i, name in enumerate(tips)}
    batch, lds = _score.BATCH_TREES or 0, _score.POLYTOMY_LDS_BYTES or 0
    timings = {}
    with _resident_tables(device, trees, tips, index) as src:
        timings["tables"] = src.seconds
        if src.tabs is None:  # (no source tree has two leaves: nothing to fit)
            return ResolveResult(supertree.copy(), 0, 0, [], [], timings)
        sent, skipped = _score.polytomy_queries(parent, True, int(max_degree), int(np.max(src.n_leaves)), lds)
        t = time.perf_counter()
        trip = src.dev.score_triplets(src.tabs, parent, taxon, batch_trees=batch)
        timings["triplets"] = time.perf_counter() - t
        initial = int((trip["t_super"] + trip["t_source"] - 2 * trip["t_shared"]).sum())
        if len(sent) == 0:
            return ResolveResult(supertree.copy(), initial, initial, [], skipped, timings)
        t = time.perf_counter()
        py = src.dev.score_polytomies(src.tabs, parent, taxon, sent, batch_trees=batch, lds_bytes=lds)
        timings["polytomies"] = time.perf_counter() - t
    return resolve_from_tensors(supertree, sent, py["py_total"], py["py_joint"], skipped, initial, min_gain, timings)
