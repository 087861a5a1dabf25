"""``refine_supertree``: a hill-climb on the summed rooted triplet distance of a supertree to its sources, by subtree
prune-and-regraft moves (of which nearest-neighbour interchanges are a special case); DESIGN.md section 24.

A move (q, v) prunes the subtree of preorder node q and regrafts it on the edge above node v (``regraft_clade``).  Its
*footprint* is the cluster of f = LCA(q, v) (f = v when v is an ancestor of q): only triples whose three taxa lie in
cl(f) can change their resolution, and every cluster outside the subtree of f, and cl(f) itself, stays.  So moves
whose footprints are pairwise disjoint tip ranges change the total by the sum of their single gains, and one round
can apply many moves scored on the same tree.

One round, on source tables that stay on the device from the first round to the last (the taxon ids are the tip
positions of the input supertree and do not move with the edits):

1. ``scs_score_taxon_triplets``: D = Σ (tx_super + tx_source - 2 tx_shared) / 3, which must equal what the round
   before predicted (``RuntimeError`` otherwise);
2. the queries: the tips of the ``taxa_per_round`` least stable taxa (``rogue_taxa``, instability > 0), then the clades
   ``select_clades(clades_per_round, ..., clade_max_tips)`` picks; one ``scs_score_clade_moves`` call returns each
   query's own entry and its ``top_k`` best targets; a candidate is (q, v, gain) with
   gain = (own_super - 2 own_shared) - (mv_super - 2 mv_shared) > 0;
3. with ``nni``: ``scs_score_branch_triplets``; for a quartet branch c with children A, B (in child order) and parent P
   the candidates (B, P) with gain 2 (bt_alt1 - bt_concordant) and (A, P) with gain 2 (bt_alt2 - bt_concordant),
   where positive;
4. a repeated (q, v) keeps its larger gain (the first entry on a tie; the regraft candidates are listed first); the
   candidates are sorted by (-gain, q, v) and taken greedily while their footprint is disjoint from those taken;
5. ``apply_moves``; the prediction is D - Σ gains.

The search stops when a round takes no move or after ``max_rounds``; the last tree is scored once more by step 1.

With ``resolve=True`` the polytomies of the start tree are resolved first (``resolve.agglomerate`` on one
``scs_score_polytomies`` call) and recorded as a round 0 whose moves have ``kind`` "resolve",
``node`` = ``target`` = the polytomy and ``groups``; round 1 then scores the resolved tree and holds the resolution to
its prediction like any other round.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from spectralclustersupertree_amd import score as _score
from spectralclustersupertree_amd.score import (SupertreeScore, _leaf_ranges, _move_clade, _preorder,
                                                _resident_tables, quartet_branches, select_clades, supertree_arrays)
from spectralclustersupertree_amd.tree import TreeNode


@dataclass
class RefineResult:
    """What ``refine_supertree`` did.  ``rounds``: one dict per scoring round with ``distance`` (the total triplet
    distance of the round's tree), ``moves`` (dicts with ``kind`` "spr" or "nni", ``node``, ``target`` (preorder
    indices in the round's tree), ``gain`` and ``tips``, in the order they were taken) and ``seconds``.  ``timings``:
    ``tables`` (seconds to build the resident source tables) and per round the lists ``taxon_triplets``,
    ``branch_triplets`` and ``clade_moves`` (seconds of the three device calls)."""

    supertree: TreeNode
    initial_distance: int
    final_distance: int
    rounds: list = field(default_factory=list)
    timings: dict = field(default_factory=dict)

    def table(self) -> str:
        """One TSV row per move: round, kind, node, target, tips, gain, distance_after (the round's distance less the
        gains of the round's moves up to this one)."""
        rows = ["round\tkind\tnode\ttarget\ttips\tgain\tdistance_after"]
        for r, rnd in enumerate(self.rounds):
            left = rnd["distance"]
            for m in rnd["moves"]:
                left -= m["gain"]
                rows.append(f"{r}\t{m['kind']}\t{m['node']}\t{m['target']}\t{m['tips']}\t{m['gain']}\t{left}")
        return "\n".join(rows) + "\n"


def tree_arrays_with_ids(tree: TreeNode, index: dict) -> tuple[np.ndarray, np.ndarray]:
    """``(parent, taxon)`` of ``tree`` in preorder (``TreeNode.to_flat`` order) with the taxon id of every tip taken
    from ``index`` (name -> id) and -1 at inner nodes: ``supertree_arrays`` for ids that are not the tips' positions.
    ``ValueError`` for a tip whose name ``index`` does not hold."""
    parents, names, _, _ = tree.to_flat()
    parent = np.asarray(parents, dtype=np.int32)
    has_child = np.zeros(len(parent), dtype=bool)
    has_child[parent[1:]] = True
    taxon = np.full(len(parent), -1, dtype=np.int32)
    for v in np.flatnonzero(~has_child):
        if names[v] not in index:
            msg = f"tip {names[v]!r} has no taxon id"
            raise ValueError(msg)
        taxon[v] = index[names[v]]
    return parent, taxon


def subtree_ends(parent) -> np.ndarray:
    """One past the last preorder index of every node's subtree."""
    parent = np.asarray(parent, dtype=np.int64)
    end = np.arange(1, len(parent) + 1, dtype=np.int64)
    for v in range(len(parent) - 1, 0, -1):
        end[parent[v]] = max(end[parent[v]], end[v])
    return end


def footprint_node(parent, end, q: int, v: int) -> int:
    """f = LCA(q, v), and v itself when v is an ancestor of q: the node whose cluster holds every triple the move
    (q, v) can change."""
    f = int(v)
    while not f <= q < end[f]:
        f = int(parent[f])
    return f


def top_k_targets(d_row, q: int, end_q: int, k: int) -> list[int]:
    """The rule of ``scs_score_clade_moves`` on one row of keys d (host form, for tests and documentation): the nodes
    outside [q, end_q) by (d, node) ascending, the first ``k``; -1 where fewer exist."""
    d_row = np.asarray(d_row, dtype=np.int64)
    nodes = [v for v in range(len(d_row)) if not q <= v < end_q]
    nodes.sort(key=lambda v: (int(d_row[v]), v))
    nodes = nodes[:k]
    return nodes + [-1] * (k - len(nodes))


def nni_candidates(parent, bt_concordant, bt_alt1, bt_alt2) -> list[tuple]:
    """(node, target, gain, "nni") for every quartet branch and alternative with a positive gain."""
    parent = np.asarray(parent, dtype=np.int64)
    kids: dict = {}
    for v in range(1, len(parent)):
        kids.setdefault(int(parent[v]), []).append(v)
    out = []
    for c in np.flatnonzero(quartet_branches(parent)):
        a, b = kids[int(c)]
        p = int(parent[c])
        for node, alt in ((b, bt_alt1), (a, bt_alt2)):
            gain = 2 * (int(alt[c]) - int(bt_concordant[c]))
            if gain > 0:
                out.append((node, p, gain, "nni"))
    return out


def select_moves(candidates, parent, *, footprint: str = "lca") -> list[tuple]:
    """Step 4 of a round: ``candidates`` are (node, target, gain, kind).  ``footprint="clade"`` weakens the rule to
    "the moved clades are disjoint" (tests plant it as a defect: such moves do not add up)."""
    best: dict = {}
    for q, v, gain, kind in candidates:
        if (q, v) not in best or gain > best[q, v][2]:
            best[q, v] = (q, v, gain, kind)
    ranked = sorted(best.values(), key=lambda m: (-m[2], m[0], m[1]))
    lo, hi = _leaf_ranges(np.asarray(parent, dtype=np.int64))
    end = subtree_ends(parent)
    taken, spans = [], []
    for q, v, gain, kind in ranked:
        f = footprint_node(parent, end, q, v) if footprint == "lca" else q
        if all(hi[f] < a or b < lo[f] for a, b in spans):
            taken.append((q, v, gain, kind))
            spans.append((int(lo[f]), int(hi[f])))
    return taken


def apply_moves(tree: TreeNode, moves) -> TreeNode:
    """A copy of ``tree`` with every (node, target) of ``moves`` applied: the subtree of ``node`` pruned and regrafted
    on the edge above ``target``, as ``SupertreeScore.regraft_clade`` does it.  All preorder indices refer to ``tree``
    as given and are resolved before the first edit; the edits then run in list order.  Moves with disjoint
    footprints (module docstring) do not see each other, and their order does not matter.  ``ValueError`` when a node
    is the root or out of range, a target is out of range or lies inside its node's subtree, or an earlier move of
    the list has put the target there."""
    out = tree.copy()
    nodes = _preorder(out)
    pairs = []
    for node, target in moves:
        if not 1 <= int(node) < len(nodes):
            msg = f"node {node} is the root or not in [1, {len(nodes)})"
            raise ValueError(msg)
        if not 0 <= int(target) < len(nodes):
            msg = f"target {target} is not in [0, {len(nodes)})"
            raise ValueError(msg)
        pairs.append((nodes[int(node)], nodes[int(target)], int(node), int(target)))
    for clade, goal, node, target in pairs:
        up = goal
        while up is not None:
            if up is clade:
                msg = f"target {target} lies inside the subtree of node {node}"
                raise ValueError(msg)
            up = up.parent
    replaced: dict = {}  # a suppressed node -> the child that took its place
    for clade, goal, node, target in pairs:
        while id(goal) in replaced:
            goal = replaced[id(goal)]
        up = goal
        while up is not None:
            if up is clade:
                msg = f"an earlier move put target {target} inside the subtree of node {node}"
                raise ValueError(msg)
            up = up.parent
        out = _move_clade(out, clade, goal, replaced)
    return out


def _round_queries(parent, taxon, tips, tx: dict, taxa_per_round: int, clades_per_round: int,
                   clade_max_tips: int) -> list[int]:
    """Step 2's query nodes: rogue tips first, then the picked clades, each node once, never the root."""
    view = SupertreeScore(None, None, None, None, None, None, None, taxa=list(tips), tx_trees=tx["tx_trees"],
                          tx_total=tx["tx_total"], tx_super=tx["tx_super"], tx_source=tx["tx_source"],
                          tx_shared=tx["tx_shared"])
    tip_nodes = np.flatnonzero(taxon >= 0)
    node_of = np.zeros(len(tips), dtype=np.int64)
    node_of[taxon[tip_nodes]] = tip_nodes
    queries = [int(node_of[r["taxon"]]) for r in view.rogue_taxa(max(int(taxa_per_round), 0))
               if r["instability"] > 0]
    if clades_per_round > 0:
        ids = taxon[tip_nodes]  # (the counts are per taxon id; select_clades wants them per tip position)
        queries += select_clades(int(clades_per_round), parent, view.taxon_instability[ids], tx["tx_trees"][ids],
                                 clade_max_tips).tolist()
    seen: set = set()
    return [q for q in queries if q != 0 and not (q in seen or seen.add(q))]


def refine_supertree(supertree: TreeNode, trees, *, max_rounds: int = 50, clades_per_round: int = 64,
                     taxa_per_round: int = 64, clade_max_tips: int = 64, top_k: int = 4, nni: bool = True,
                     resolve: bool = False, device=None) -> RefineResult:
    """Lowers the summed rooted triplet distance of ``supertree`` to ``trees`` by rounds of prune-and-regraft moves
    with disjoint footprints (module docstring) until a round finds none or ``max_rounds`` have run.  ``trees`` as for
    ``score_supertree`` (either input path, the same ``ValueError``s, weights ignored).  ``taxa_per_round`` tips and
    ``clades_per_round`` clades of up to ``clade_max_tips`` tips are queried per round, ``top_k`` (1 to 8) targets
    each; ``nni`` adds the nearest-neighbour interchanges of every quartet branch; ``resolve`` resolves the polytomies
    of the start tree before the first round (module docstring).  The input tree is not modified."""
    if max_rounds < 0 or clades_per_round < 0 or taxa_per_round < 0 or clade_max_tips < 2 or not 1 <= top_k <= 8:
        msg = (f"max_rounds = {max_rounds}, clades_per_round = {clades_per_round} or taxa_per_round = "
               f"{taxa_per_round} is negative, clade_max_tips = {clade_max_tips} is under 2 or top_k = {top_k} is "
               f"not in [1, 8]")
        raise ValueError(msg)
    _, _, tips = supertree_arrays(supertree)
    index = {name: i for i, name in enumerate(tips)}
    dev = device if device is not None else _score._default_device()
    batch = _score.BATCH_TREES or 0
    tree = supertree.copy()
    rounds: list = []
    timings = {"tables": 0.0, "taxon_triplets": [], "branch_triplets": [], "clade_moves": []}
    if resolve:
        timings["polytomies"] = []
    t0 = time.perf_counter()
    with _resident_tables(dev, trees, tips, index) as src:
        tabs = src.tabs
        timings["tables"] = time.perf_counter() - t0
        if tabs is None:  # (no source tree has two leaves: nothing to fit)
            return RefineResult(tree, 0, 0, rounds, timings)

        def distance(parent, taxon):
            t = time.perf_counter()
            tx = dev.score_taxon_triplets(tabs, parent, taxon, batch_trees=batch,
                                          lds_bytes=_score.TAXON_LDS_BYTES or 0)
            timings["taxon_triplets"].append(time.perf_counter() - t)
            total = int((tx["tx_super"] + tx["tx_source"] - 2 * tx["tx_shared"]).sum())
            assert total % 3 == 0, total
            return tx, total // 3

        predicted = None
        initial = final = None
        if resolve:
            from spectralclustersupertree_amd.resolve import resolve_from_tensors

            t_round = time.perf_counter()
            parent, taxon = tree_arrays_with_ids(tree, index)
            _, initial = distance(parent, taxon)
            sent, _ = _score.polytomy_queries(parent, True, _score.PY_MAX_DEGREE, int(np.max(src.n_leaves)),
                                              _score.POLYTOMY_LDS_BYTES or 0)
            moves = []
            if len(sent):
                t = time.perf_counter()
                py = dev.score_polytomies(tabs, parent, taxon, sent, batch_trees=batch,
                                          lds_bytes=_score.POLYTOMY_LDS_BYTES or 0)
                timings["polytomies"].append(time.perf_counter() - t)
                done = resolve_from_tensors(tree, sent, py["py_total"], py["py_joint"], [], initial)
                tree, predicted = done.supertree, done.predicted_distance
                moves = [{"kind": "resolve", "node": m["node"], "target": m["node"], "gain": m["gain"],
                          "tips": m["tips"], "groups": m["groups"]} for m in done.merges]
            rounds.append({"distance": initial, "moves": moves, "seconds": time.perf_counter() - t_round})
        for r in range(max_rounds + 1):
            t_round = time.perf_counter()
            parent, taxon = tree_arrays_with_ids(tree, index)
            tx, dist = distance(parent, taxon)
            if predicted is not None and dist != predicted:
                msg = (f"refine_supertree: round {r} scores {dist}, but the moves of round {r - 1} predicted "
                       f"{predicted}")
                raise RuntimeError(msg)
            if initial is None:
                initial = dist
            final = dist
            if r == max_rounds:  # (the confirmation of the last tree: no further round)
                break
            candidates = []
            queries = _round_queries(parent, taxon, tips, tx, taxa_per_round, clades_per_round, clade_max_tips)
            t = time.perf_counter()
            if queries:
                mv = dev.score_clade_moves(tabs, parent, taxon, queries, top_k=top_k, batch_trees=batch,
                                           lds_bytes=_score.CLADE_PLACEMENT_LDS_BYTES or 0)
                own = mv["mv_own_super"] - 2 * mv["mv_own_shared"]
                there = mv["mv_super"] - 2 * mv["mv_shared"]
                for i, q in enumerate(queries):
                    for j in range(top_k):
                        v = int(mv["mv_node"][i, j])
                        gain = int(own[i] - there[i, j])
                        if v >= 0 and gain > 0:
                            candidates.append((q, v, gain, "spr"))
            timings["clade_moves"].append(time.perf_counter() - t)
            t = time.perf_counter()
            if nni:
                bt = dev.score_branch_triplets(tabs, parent, taxon, batch_trees=batch)
                candidates += nni_candidates(parent, bt["bt_concordant"], bt["bt_alt1"], bt["bt_alt2"])
            timings["branch_triplets"].append(time.perf_counter() - t)
            taken = select_moves(candidates, parent)
            lo, hi = _leaf_ranges(parent.astype(np.int64))
            moves = [{"kind": kind, "node": q, "target": v, "gain": gain, "tips": int(hi[q] - lo[q] + 1)}
                     for q, v, gain, kind in taken]
            if taken:
                tree = apply_moves(tree, [(q, v) for q, v, _, _ in taken])
                predicted = dist - sum(m[2] for m in taken)
            rounds.append({"distance": dist, "moves": moves, "seconds": time.perf_counter() - t_round})
            if not taken:
                break
    return RefineResult(tree, initial, final, rounds, timings)
