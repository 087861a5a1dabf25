"""Times ``score_supertree`` (``scs_score_supertree``) on synthetic forests (``synthetic.tree_arrays``) against a
random binary supertree on all taxa: one JSON line per size with the host / device split.

    python tools/score_bench.py                      # the three sizes below
    python tools/score_bench.py --size 10000x500     # one size; NxM or NxMxK (K leaves per tree)
    python tools/score_bench.py --triplets           # also the rooted triplet terms
    python tools/score_bench.py --conflicts          # also the clade conflict counts
    python tools/score_bench.py --concordance        # also the branch concordance counts
    python tools/score_bench.py --branch-triplets    # also the per-branch triplet support
    python tools/score_bench.py --taxon-triplets     # also the per-taxon triplet support
    python tools/score_bench.py --placements 16      # also the placement support of 16 taxa
    python tools/score_bench.py --triplets --clade-placements 16 --placements-as-clade-tips
                                                     # also the placement support of 16 clades,
                                                     # beside as many taxon placements as the clades hold tips
    python tools/score_bench.py --large-clade        # the same for one clade: the first child of the root's first child
    python tools/score_bench.py --refine --size 10000x500   # refine_supertree on a model tree with 20 planted regrafts
                                                     # against restrictions of the model
    python tools/score_bench.py --polytomies --size 10000x500   # scs_score_polytomies on a supertree with collapsed
                                                     # edges (degrees 3, 8, 32; --collapse N nodes of each) beside one
                                                     # scs_score_triplets call
    python tools/score_bench.py --branch-resample 100 --size 10000x500   # scs_score_branch_resample with 100 weight
                                                     # rows (repeatable) beside one scs_score_branch_triplets call
                                                     # 
    python tools/score_bench.py --parsimony --size 10000x500   # scs_score_parsimony with and without the per-clade
                                                     # lengths beside one scs_score_triplets call
    python tools/score_bench.py --source-pairs --size 10000x500   # scs_score_source_pairs, every pair of sources,
                                                     # beside scs_score_supertree and scs_score_triplets on the same
                                                     # tables and the host reference on a sample of the pairs
                                                     # 
    python tools/score_bench.py --source-triplets    # scs_score_source_pair_triplets: one row and 16 rows of 10000x500,
                                                     # every pair of 20000x2000x500, beside scs_score_source_pairs and
                                                     # scs_score_triplets on the same tables and the host reference on
                                                     # sampled cells
    python tools/score_bench.py --coverage --size 10000x500   # scs_score_coverage for min_trees 1 and 2, with and
                                                     # without the two matrices, beside the numpy reference on a sample
                                                     # of rows and the word operations the sweep needs (DESIGN.md
                                                     # section 36)
    python tools/score_bench.py --internode          # scs_score_internode on 10000x500 and 20000x2000x500 with and
                                                     # without the matrices, beside the host reference on a sample of
                                                     # rows and the (pair, tree) evaluations per second (DESIGN.md
                                                     # section 41)
    python tools/score_bench.py --caterpillar        # supertree and sources caterpillars, sources reversed
    python tools/score_bench.py --caterpillar-supertree   # a caterpillar supertree against the synthetic sources
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

from spectralclustersupertree_amd import refine_supertree, score_supertree, synthetic  # noqa: E402
from spectralclustersupertree_amd import refine as refine_mod  # noqa: E402
from spectralclustersupertree_amd.backend import Device, debug_parsimony_plan  # noqa: E402
from spectralclustersupertree_amd.score import (_leaf_ranges, _resident_tables, resample_weights,  # noqa: E402
                                                select_clades, supertree_arrays)
from spectralclustersupertree_amd.tree import TreeNode  # noqa: E402
from spectralclustersupertree_amd.treearrays import TreeArrays  # noqa: E402

SIZES = ("10000x500", "100000x5000", "20000x2000x500")


def random_binary_tree(seed: int, n_taxa: int) -> TreeNode:
    """Random merges of two parts at a time, O(n)."""
    rs = np.random.RandomState(seed)
    parts = [TreeNode(synthetic.taxon_name(int(i))) for i in rs.permutation(n_taxa)]
    while len(parts) > 1:
        i = int(rs.randint(len(parts)))
        parts[i], parts[-1] = parts[-1], parts[i]
        a = parts.pop()
        j = int(rs.randint(len(parts)))
        parts[j], parts[-1] = parts[-1], parts[j]
        parts.append(TreeNode(None, [a, parts.pop()]))
    return parts[0]


def caterpillar(order) -> TreeNode:
    """(((x0, x1), x2), ...) over the taxon ids ``order``, O(n)."""
    node = TreeNode(synthetic.taxon_name(int(order[0])))
    for x in order[1:]:
        node = TreeNode(None, [node, TreeNode(synthetic.taxon_name(int(x)))])
    return node


def caterpillar_arrays(n_taxa: int, n_trees: int, per_tree: int | None) -> TreeArrays:
    """``n_trees`` caterpillars on the first ``per_tree`` taxa (all by default) in reverse taxon order, as preorder
    node arrays: the inner nodes root first, then the leaves (the first two hang from the deepest inner node)."""
    k = n_taxa if per_tree is None else per_tree
    order = np.arange(k - 1, -1, -1, dtype=np.int32)
    parent = np.concatenate([np.arange(-1, k - 2, dtype=np.int32), [k - 2, k - 2],
                             np.arange(k - 3, -1, -1, dtype=np.int32)])
    taxon = np.concatenate([np.full(k - 1, -1, dtype=np.int32), order])
    nn = 2 * k - 1
    return TreeArrays(n_taxa=n_taxa, node_off=np.arange(n_trees + 1, dtype=np.int64) * nn,
                      parent=np.tile(parent, n_trees), taxon=np.tile(taxon, n_trees),
                      length=np.full(n_trees * nn, np.nan), support=np.full(n_trees * nn, np.nan),
                      weights=np.ones(n_trees), taxa=[synthetic.taxon_name(i) for i in range(n_taxa)])


def run(dev: Device, size: str, repeats: int, triplets: bool = False, conflicts: bool = False,
        cat: bool = False, concordance: bool = False, branch_triplets: bool = False, taxon_triplets: bool = False,
        cat_sup: bool = False, placements: int = 0, clades: int = 0, clade_max_tips: int = 64,
        large_clade: bool = False, match_tips: bool = False) -> dict:
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    t0 = time.perf_counter()
    if cat:
        arrays = caterpillar_arrays(n_taxa, n_trees, per_tree)
        sup = caterpillar(np.arange(n_taxa))
    else:
        arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
        sup = caterpillar(np.random.RandomState(2).permutation(n_taxa)) if cat_sup else random_binary_tree(2, n_taxa)
    gen_s = time.perf_counter() - t0
    nodes = None
    if clades or large_clade:  # the query nodes, fixed before the timed calls
        parent = np.asarray(sup.to_flat()[0], dtype=np.int64)
        lo, hi = _leaf_ranges(parent)
        if large_clade:
            nodes = np.array([2], dtype=np.int32)  # (preorder: the root, its first child, that child's first child)
        else:
            first = score_supertree(sup, arrays, taxon_triplets=True, device=dev)
            nodes = select_clades(clades, parent, first.taxon_instability, first.tx_trees, clade_max_tips)
        clade_tips = int((hi[nodes] - lo[nodes] + 1).sum())
        if match_tips and clade_tips <= 1024:  # (more query taxa than that need more rows than a call may take)
            placements = clade_tips
    runs = []
    for i in range(repeats + (nodes is not None)):  # (with clades: a warm-up call at this size, not timed)
        t0 = time.perf_counter()
        res = score_supertree(sup, arrays, triplets=triplets, conflicts=conflicts, concordance=concordance,
                              branch_triplets=branch_triplets, taxon_triplets=taxon_triplets,
                              placements=_queries(sup, placements) if placements else None,
                              clade_placements=nodes, device=dev)
        if i or nodes is None:
            runs.append((time.perf_counter() - t0, res.timings))
    wall, tim = min(runs, key=lambda r: r[0])
    out = {
        "size": size, "input": "caterpillar" if cat else "caterpillar supertree" if cat_sup else "random", "n_taxa": n_taxa, "n_trees": n_trees, "leaves": int(arrays.leaf_counts().sum()),
        "supertree_nodes": len(res.informative), "repeats": repeats, "input_generation_s": round(gen_s, 3),
        "wall_s": round(wall, 4), "host_prepare_s": round(tim["prepare"], 4),
        "device_tables_s": round(tim["tables"], 4), "score_call_s": round(tim["score"], 4),
        "total_rf": res.total_rf, "mean_rf": float(res.rf.mean()),
    }
    if triplets:
        out.update({"triplets_call_s": round(tim["triplets"], 4), "total_triplet_distance": res.total_triplet_distance,
                    "triplet_fit": res.triplet_fit})
    if conflicts:
        leaves = int(arrays.leaf_counts().sum())
        out.update({"conflicts_call_s": round(tim["conflicts"], 4),
                    "conflicts_ns_per_leaf": round(tim["conflicts"] / max(leaves, 1) * 1e9, 3),
                    "total_n_super_conflict": int(res.n_super_conflict.sum()),
                    "total_n_source_conflict": int(res.n_source_conflict.sum()),
                    "total_conflicting": int(res.conflicting.sum()), "total_supported": int(res.supported.sum()),
                    "total_informative": int(res.informative.sum())})
    if concordance:
        leaves = int(arrays.leaf_counts().sum())
        out.update({"concordance_call_s": round(tim["concordance"], 5),
                    "concordance_call_s_min_median_max": [round(x, 5)
                                                          for x in _spread([r[1]["concordance"] for r in runs])],
                    "concordance_ns_per_leaf": round(tim["concordance"] / max(leaves, 1) * 1e9, 3),
                    "score_call_s_min_median_max": [round(x, 5) for x in _spread([r[1]["score"] for r in runs])],
                    "total_decisive": int(res.decisive.sum()), "total_concordant": int(res.concordant.sum()),
                    "total_alt1": int(res.alt1.sum()), "total_alt2": int(res.alt2.sum()),
                    "total_other": int(res.other.sum()), "quartet_branches": int(res.quartet_branch.sum())})
    if branch_triplets:
        out.update({"branch_triplets_call_s": round(tim["branch_triplets"], 5),
                    "branch_triplets_call_s_min_median_max":
                        [round(x, 5) for x in _spread([r[1]["branch_triplets"] for r in runs])],
                    "total_bt_total": int(res.bt_total.sum()), "total_bt_concordant": int(res.bt_concordant.sum()),
                    "total_bt_alt1": int(res.bt_alt1.sum()), "total_bt_alt2": int(res.bt_alt2.sum()),
                    "total_bt_fan": int(res.bt_fan.sum()), "branches_with_triples": int((res.bt_total > 0).sum())})
        if triplets:
            out["triplets_call_s_min_median_max"] = [round(x, 5) for x in _spread([r[1]["triplets"] for r in runs])]
            out["branch_triplets_over_triplets"] = round(tim["branch_triplets"] / tim["triplets"], 3)
    if taxon_triplets:
        # (y, z) pairs of the sweep: T's nontrivial clusters times those of the restricted supertree, per tree
        pairs = int((res.n_source * res.n_super).sum())
        med = _spread([r[1]["taxon_triplets"] for r in runs])[1]
        worst = res.rogue_taxa(1)
        out.update({"taxon_triplets_call_s": round(tim["taxon_triplets"], 5),
                    "taxon_triplets_call_s_min_median_max":
                        [round(x, 5) for x in _spread([r[1]["taxon_triplets"] for r in runs])],
                    "node_pairs": pairs, "taxon_triplets_pairs_per_s": round(pairs / max(med, 1e-9), 1),
                    "total_tx_shared": int(res.tx_shared.sum()), "total_tx_source": int(res.tx_source.sum()),
                    "total_tx_super": int(res.tx_super.sum()), "total_tx_total": int(res.tx_total.sum()),
                    "worst_instability": worst[0]["instability"] if worst else None})
        if triplets:
            tmed = _spread([r[1]["triplets"] for r in runs])[1]
            out["triplets_call_s_min_median_max"] = [round(x, 5) for x in _spread([r[1]["triplets"] for r in runs])]
            out["triplets_pairs_per_s"] = round(pairs / max(tmed, 1e-9), 1)
            out["taxon_triplets_over_triplets"] = round(med / max(tmed, 1e-9), 3)
            out["sums_are_three_times_the_per_tree_sums"] = bool(
                int(res.tx_shared.sum()) == 3 * int(res.t_shared.sum())
                and int(res.tx_source.sum()) == 3 * int(res.t_source.sum())
                and int(res.tx_super.sum()) == 3 * int(res.t_super.sum()))
    if placements:
        best = res.best_placements()
        out.update({"placements": placements, "placements_call_s": round(tim["placements"], 5),
                    "placements_call_s_min_median_max":
                        [round(x, 5) for x in _spread([r[1]["placements"] for r in runs])],
                    "placement_entries": int(res.pl_shared.size), "total_pl_trees": int(res.pl_trees.sum()),
                    "total_best_distance": int(sum(r["best_distance"] for r in best)),
                    "taxa_with_a_better_place": int(sum(r["improvement"] > 0 for r in best))})
    if nodes is not None:
        best = res.best_clade_placements()
        cmed = _spread([r[1]["clade_placements"] for r in runs])[1]
        out.update({"clade_placements": len(nodes), "clade_tips": clade_tips,
                    "clade_placements_call_s": round(tim["clade_placements"], 5),
                    "clade_placements_call_s_min_median_max":
                        [round(x, 5) for x in _spread([r[1]["clade_placements"] for r in runs])],
                    "clade_placement_entries": int(res.cp_shared.size), "total_cp_trees": int(res.cp_trees.sum()),
                    "total_best_clade_distance": int(sum(r["best_distance"] for r in best)),
                    "clades_with_a_better_place": int(sum(r["improvement"] > 0 for r in best))})
        if placements:
            pmed = _spread([r[1]["placements"] for r in runs])[1]
            out["clade_placements_over_placements"] = round(cmed / max(pmed, 1e-9), 3)
        if triplets:
            tmed = _spread([r[1]["triplets"] for r in runs])[1]
            out["triplets_call_s_min_median_max"] = [round(x, 5) for x in _spread([r[1]["triplets"] for r in runs])]
            out["clade_placements_over_triplets"] = round(cmed / max(tmed, 1e-9), 3)
    if placements:
        if taxon_triplets:
            xmed = _spread([r[1]["taxon_triplets"] for r in runs])[1]
            pmed = _spread([r[1]["placements"] for r in runs])[1]
            out["placements_over_taxon_triplets"] = round(pmed / max(xmed, 1e-9), 3)
    return out


def model_arrays(model: TreeNode, n_trees: int, per_tree: int | None, seed: int) -> TreeArrays:
    """``n_trees`` restrictions of ``model`` to ``per_tree`` random taxa each (copies of it when None)."""
    taxa = model.get_tip_names()
    one = TreeArrays.from_trees([model], [1.0], taxa)
    rs = np.random.RandomState(seed)
    parts = [one if per_tree is None or per_tree >= len(taxa)
             else one.restrict(np.sort(rs.choice(len(taxa), size=per_tree, replace=False)).astype(np.int32))
             for _ in range(n_trees)]
    off = np.concatenate([[0], np.cumsum([len(p.parent) for p in parts])]).astype(np.int64)
    return TreeArrays(n_taxa=len(taxa), node_off=off, parent=np.concatenate([p.parent for p in parts]),
                      taxon=np.concatenate([p.taxon for p in parts]), length=np.concatenate([p.length for p in parts]),
                      support=np.concatenate([p.support for p in parts]), weights=np.ones(n_trees), taxa=list(taxa))


def run_refine(dev: Device, size: str, planted: int = 20, repeats: int = 5) -> dict:
    """``refine_supertree`` on a random binary model tree with ``planted`` clades of up to 8 tips regrafted at random,
    against restrictions of the model: a warm-up and ``repeats`` timed runs; beside them the calls a hand-written loop
    makes per turn (one ``score_supertree`` with the three options), and ``scs_score_clade_moves`` against
    ``scs_score_clade_placements`` on resident tables for the same 64 clades and for 1 500 tip queries."""
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    model = random_binary_tree(2, n_taxa)
    arrays = model_arrays(model, n_trees, per_tree, 3)
    rs = np.random.RandomState(4)
    start = model
    for _ in range(planted):
        end = refine_mod.subtree_ends(start.to_flat()[0])
        at = np.arange(len(end))
        q = int(rs.choice(np.flatnonzero((end - at <= 15) & (at > 0))))
        v = int(rs.randint(len(end)))
        while q <= v < end[q]:
            v = int(rs.randint(len(end)))
        start = refine_mod.apply_moves(start, [(q, v)])
    runs = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        res = refine_supertree(start, arrays, device=dev)
        runs.append((time.perf_counter() - t0, res))
    runs = runs[1:]
    per_round = {k: [float(np.mean(r.timings[k])) for _, r in runs]
                 for k in ("taxon_triplets", "branch_triplets", "clade_moves")}
    res = runs[0][1]
    out = {"size": size, "refine": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "planted": planted, "rounds": len(res.rounds), "moves": [len(r["moves"]) for r in res.rounds],
           "initial_distance": res.initial_distance, "final_distance": res.final_distance,
           "refine_wall_s_min_median_max": [round(x, 4) for x in _spread([w for w, _ in runs])],
           "tables_s_min_median_max": [round(x, 4) for x in _spread([r.timings["tables"] for _, r in runs])],
           "round_s_min_median_max": [round(x, 4) for x in _spread(
               [float(np.mean([rnd["seconds"] for rnd in r.rounds])) for _, r in runs])]}
    for k, v in per_round.items():
        out[f"{k}_s_per_round_min_median_max"] = [round(x, 5) for x in _spread(v)]
    hand = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        sc = score_supertree(start, arrays, taxon_triplets=True, branch_triplets=True, clade_placements=64, device=dev)
        hand.append((time.perf_counter() - t0, sc.timings))
    hand = hand[1:]
    out["hand_turn_wall_s_min_median_max"] = [round(x, 4) for x in _spread([w for w, _ in hand])]
    for k in ("tables", "taxon_triplets", "branch_triplets", "clade_placements"):
        out[f"hand_turn_{k}_s_min_median_max"] = [round(x, 5) for x in _spread([t[k] for _, t in hand])]
    parent, _, tips = supertree_arrays(start)
    index = {x: i for i, x in enumerate(tips)}
    parent, taxon = refine_mod.tree_arrays_with_ids(start, index)
    tip_nodes = np.flatnonzero(taxon >= 0)
    sets = {"64_clades": sc.cp_nodes.astype(np.int32),
            "1500_tips": tip_nodes[np.linspace(0, len(tip_nodes) - 1, num=min(1500, len(tip_nodes)), dtype=np.int64)]}
    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        for name, nodes in sets.items():
            for what, call in (("placements", lambda n=nodes: dev.score_clade_placements(tabs, parent, taxon, n)),
                               ("moves", lambda n=nodes: dev.score_clade_moves(tabs, parent, taxon, n, top_k=4))):
                times = []
                for _ in range(repeats + 1):
                    t0 = time.perf_counter()
                    call()
                    times.append(time.perf_counter() - t0)
                out[f"{name}_{what}_s_min_median_max"] = [round(x, 5) for x in _spread(times[1:])]
    return out


def collapse_to_degrees(tree: TreeNode, degrees, per_degree: int, seed: int) -> TreeNode:
    """A copy of the binary ``tree`` in which, for every k of ``degrees``, ``per_degree`` disjoint inner nodes with at
    least 2 k tips below have the children of their largest inner children pulled up until they hold k children."""
    out = tree.copy()
    rs = np.random.RandomState(seed)
    nodes = [out]
    for v in nodes:  # (preorder without recursion)
        nodes.extend(v.children)
    tips = {id(v): 1 for v in nodes if not v.children}
    for v in reversed(nodes):
        if v.children:
            tips[id(v)] = sum(tips[id(c)] for c in v.children)
    taken: set = set()

    def free(v):
        while v is not None:
            if id(v) in taken:
                return False
            v = v.parent
        return True

    for k in sorted(degrees, reverse=True):
        room = [v for v in nodes if v.children and v.parent is not None and 2 * k <= tips[id(v)] <= 40 * k]
        rs.shuffle(room)
        made = 0
        for v in room:
            if made == per_degree:
                break
            below = [v]
            for u in below:
                below.extend(u.children)
            if not free(v) or any(id(u) in taken for u in below):
                continue
            while len(v.children) < k:
                c = max((c for c in v.children if c.children), key=lambda c: tips[id(c)])
                at = [x is c for x in v.children].index(True)
                kids = list(c.children)
                v.children[at:at + 1] = kids
                for x in kids:
                    x.parent = v
            taken.add(id(v))
            made += 1
    return out


def run_polytomies(dev: Device, size: str, per_degree: int = 4, repeats: int = 5, degrees=(3, 8, 32)) -> dict:
    """``scs_score_polytomies`` on resident tables, a warm-up and ``repeats`` timed calls: all collapsed nodes in one
    call, and per degree its nodes in one call and one node alone; beside them one ``scs_score_triplets`` call, the
    rescoring that resolving a polytomy pair by pair would make k (k - 1) / 2 times."""
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = collapse_to_degrees(random_binary_tree(2, n_taxa), degrees, per_degree, 5)
    parent, taxon, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    kids = np.bincount(parent[1:], minlength=len(parent))
    out = {"size": size, "polytomies": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "repeats": repeats,
           "collapsed": {int(k): int((kids == k).sum()) for k in degrees}}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        out["triplets_s_min_median_max"], trip = timed(lambda: dev.score_triplets(tabs, parent, taxon))
        every = np.flatnonzero(kids >= 3).astype(np.int32)
        out["all_nodes_s_min_median_max"], res = timed(lambda: dev.score_polytomies(tabs, parent, taxon, every))
        out["py_trees"] = res["py_trees"].tolist()
        out["joint_over_total"] = round(sum(int(j.sum()) for j in res["py_joint"])
                                        / max(sum(int(t.sum()) for t in res["py_total"]), 1), 4)
        for k in degrees:
            nodes = np.flatnonzero(kids == k).astype(np.int32)
            if len(nodes) == 0:
                continue
            out[f"degree_{k}_nodes_s_min_median_max"], _ = timed(
                lambda n=nodes: dev.score_polytomies(tabs, parent, taxon, n))
            one, _ = timed(lambda n=nodes[:1]: dev.score_polytomies(tabs, parent, taxon, n))
            out[f"degree_{k}_one_node_s_min_median_max"] = one
            out[f"degree_{k}_rescorings_s"] = round(k * (k - 1) // 2 * out["triplets_s_min_median_max"][1], 5)
            out[f"degree_{k}_one_node_over_rescorings"] = round(one[1] / max(out[f"degree_{k}_rescorings_s"], 1e-9), 4)
    return out


def run_resample(dev: Device, size: str, n_rows, repeats: int = 5) -> dict:
    """``scs_score_branch_resample`` on resident tables, a warm-up and ``repeats`` timed calls per row count R (row 0
    of ones and R - 1 bootstrap replicates, seed 0; the rows stay on the device); beside it one
    ``scs_score_branch_triplets`` call, which the same answer takes R of without the export."""
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = random_binary_tree(2, n_taxa)
    parent, taxon, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    out = {"size": size, "branch_resample": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "supertree_nodes": len(parent), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        out["branch_triplets_s_min_median_max"], bt = timed(lambda: dev.score_branch_triplets(tabs, parent, taxon))
        one = out["branch_triplets_s_min_median_max"][1]
        for rows in n_rows:
            w = resample_weights(tabs.n_trees, rows - 1, None, "bootstrap", 0)
            spread, res = timed(lambda w=w: dev.score_branch_resample(tabs, parent, taxon, w))
            same = all(np.array_equal(res["rs_point"][x], bt[k])
                       for x, k in enumerate(("bt_total", "bt_concordant", "bt_alt1", "bt_alt2")))
            wins = res["rs_wins"].sum(axis=1)
            out[f"rows_{rows}"] = {"s_min_median_max": spread, "over_one_branch_triplets_call": round(spread[1] / one, 3),
                                   "rows_times_one_call_s": round(rows * one, 4),
                                   "over_rows_times_one_call": round(spread[1] / (rows * one), 5),
                                   "row_0_equals_branch_triplets": bool(same), "wins": [int(x) for x in wins]}
    return out


def run_parsimony(dev: Device, size: str, repeats: int = 5) -> dict:
    """``scs_score_parsimony`` on resident tables, a warm-up and ``repeats`` timed calls without and with the
    per-character lengths; beside it one ``scs_score_triplets`` call, the other pass that is quadratic per tree, and
    the bytes of the membership tiles the fold reads (8 bytes per leaf and 64-character word of its tree) and all
    tile traffic (the clearing of every pass, the scan's two reads and one write, the fold's read)."""
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = random_binary_tree(2, n_taxa)
    parent, taxon, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    out = {"size": size, "parsimony": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "supertree_nodes": len(parent), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        out["triplets_s_min_median_max"], _ = timed(lambda: dev.score_triplets(tabs, parent, taxon))
        out["parsimony_s_min_median_max"], res = timed(lambda: dev.score_parsimony(tabs, parent, taxon))
        total = int(res["mrp_chars"].sum())
        out["parsimony_chars_s_min_median_max"], full = timed(
            lambda: dev.score_parsimony(tabs, parent, taxon, chars=True, n_chars=total))
        plan = debug_parsimony_plan(tabs, parent, chars=res["mrp_chars"])
    leaves = arrays.leaf_counts().astype(np.int64)
    leaves = leaves[leaves >= 2]  # (the tables hold the trees of two leaves and more, in order)
    words = (res["mrp_chars"] + 63) // 64
    fold = int((leaves * words).sum()) * 8
    cleared = sum(int(leaves[a:b].sum()) * int(p) for a, b, p in zip(plan["bstart"][:-1], plan["bstart"][1:],
                                                                     plan["passes"])) * 8 * plan["pass_words"]
    med = out["parsimony_s_min_median_max"][1]
    out.update({"characters": total, "mrp_length": int(res["mrp_length"].sum()),
                "same_per_tree_numbers": all(np.array_equal(res[k], full[k]) for k in res if res[k] is not None),
                "batches": len(plan["bstart"]) - 1, "passes": [int(x) for x in plan["passes"]],
                "frame_depth": plan["frame_depth"], "counter_bits": plan["counter_bits"],
                "fold_lds_bytes": plan["lds_bytes"], "tile_bytes_fold": fold, "tile_bytes_all": cleared + 4 * fold,
                "tile_gb_per_s_of_call": round((cleared + 4 * fold) / med / 1e9, 2),
                "over_triplets": round(med / out["triplets_s_min_median_max"][1], 3)})
    return out


def run_source_pairs(dev: Device, size: str, repeats: int = 7, sample: int = 40) -> dict:
    """``scs_score_source_pairs`` for every pair of sources on resident tables, a warm-up and ``repeats`` timed calls;
    for scale ``scs_score_supertree`` and ``scs_score_triplets`` on the same tables, and the host's linear reference
    (``tests/source_pairs_reference.py``) on ``sample`` of the pairs, which must give the device's numbers."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import source_pairs_reference as sp

    from spectralclustersupertree_amd.backend import debug_source_pairs_plan

    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = random_binary_tree(2, n_taxa)
    parent, taxon, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    out = {"size": size, "source_pairs": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        m = tabs.n_trees
        out["supertree_s_min_median_max"], rf = timed(lambda: dev.score(tabs, parent, taxon))
        out["triplets_s_min_median_max"], _ = timed(lambda: dev.score_triplets(tabs, parent, taxon))
        out["source_pairs_s_min_median_max"], res = timed(lambda: dev.score_source_pairs(tabs))
        out["one_row_s_min_median_max"], row = timed(lambda: dev.score_source_pairs(tabs, rows=[m // 2]))
        plan = debug_source_pairs_plan(tabs)
        off, leaf, adj = (np.array(x) for x in src.forest.tables()[:3])
    rs = np.random.RandomState(3)
    pairs = [(int(a), int(b)) for a, b in rs.randint(0, m, size=(sample, 2))]
    t0 = time.perf_counter()
    same = True
    for a, b in pairs:
        want = sp.pair_linear(leaf[off[a]:off[a + 1]].astype(np.int64), adj[off[a]:off[a + 1]].astype(np.int64),
                              leaf[off[b]:off[b + 1]].astype(np.int64), adj[off[b]:off[b + 1]].astype(np.int64), n_taxa)
        same = same and tuple(int(res[k][a, b]) for k in sp.KEYS) == tuple(int(x) for x in want)
    host = (time.perf_counter() - t0) / max(len(pairs), 1)
    med = out["source_pairs_s_min_median_max"][1]
    unordered = m * (m + 1) // 2
    common = res["common"].astype(np.int64)
    out.update({"tables_trees": m, "pairs_computed": unordered, "cells": m * m,
                "pairs_per_s": round(unordered / med), "us_per_pair": round(med / unordered * 1e6, 3),
                "common_leaves_mean": round(float(common.mean()), 1), "common_leaves_max": int(common.max()),
                "common_leaves_per_s": round(float(np.triu(common).sum()) / med),
                "pairs_with_3_common": int((np.triu(common, 1) >= 3).sum()),
                "mean_normalized_rf": round(float(np.nanmean(np.where(
                    res["clusters"] + res["clusters_other"] > 0,
                    (res["clusters"] + res["clusters_other"] - 2.0 * res["shared"])
                    / np.maximum(res["clusters"] + res["clusters_other"], 1), np.nan))), 4),
                "diagonal_equals_n_source": bool(np.array_equal(np.diagonal(res["shared"]), rf["n_source"])),
                "one_row_equals_its_row": all(np.array_equal(row[k][0], res[k][m // 2]) for k in sp.KEYS),
                "host_reference_sample": len(pairs), "host_reference_s_per_pair": round(host, 6),
                "host_reference_agrees": bool(same), "host_over_device_per_pair": round(host / (med / unordered), 1),
                "batches": len(plan["bstart"]) - 1, "entry_width": int(plan["width"].max()),
                "pair_lds_bytes": int(plan["lds"].max()), "slab_launch": bool(plan["slab"].any()),
                "workspace_bytes": plan["workspace"],
                "over_supertree": round(med / out["supertree_s_min_median_max"][1], 2),
                "over_triplets": round(med / out["triplets_s_min_median_max"][1], 2)})
    return out


def run_source_triplets(dev: Device, size: str, repeats: int = 5, sample: int = 40) -> dict:
    """``scs_score_source_pair_triplets`` on resident tables by the scheme of ``run_source_pairs``: a warm-up and
    ``repeats`` timed calls.  Trees of more than 2 000 leaves: rows = one tree and 16 rows (every pair would take as
    long as the node pairs of 125 250 such pairs do); smaller trees: every pair.  For scale ``scs_score_source_pairs``
    with the same rows and ``scs_score_triplets`` on the same tables; sampled cells (one, for the large trees) against
    the host's node-pair reference (``tests/source_triplets_reference.py``), which must give the device's numbers."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import source_triplets_reference as st

    from spectralclustersupertree_amd.backend import debug_source_pair_triplets_plan

    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = random_binary_tree(2, n_taxa)
    parent, taxon, tips = supertree_arrays(sup)
    index = {x: i for i, x in enumerate(tips)}
    large = int(arrays.leaf_counts().max()) > 2000
    out = {"size": size, "source_triplets": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    def node_pairs(common, mirror):
        c = np.maximum((np.triu(common) if mirror else common).astype(np.int64) - 2, 0)
        return int((c * c).sum())

    runs = {}
    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        m = tabs.n_trees
        out["triplets_s_min_median_max"], _ = timed(lambda: dev.score_triplets(tabs, parent, taxon))
        asks = {"one_row": [m // 2], "rows_16": list(range(0, m, max(m // 16, 1)))[:16]} if large else {"all_pairs": None}
        for name, rows in asks.items():
            out[f"{name}_rf_s_min_median_max"], _ = timed(lambda: dev.score_source_pairs(tabs, rows))
            out[f"{name}_s_min_median_max"], res = timed(lambda: dev.score_source_pair_triplets(tabs, rows))
            out[f"{name}_unshared_s_min_median_max"], part = timed(lambda: dev.score_source_pair_triplets(
                tabs, rows, outputs=("common", "triplets", "triplets_other")))
            plan = debug_source_pair_triplets_plan(tabs, rows=rows)
            med = out[f"{name}_s_min_median_max"][1]
            pairs = node_pairs(res["common"], rows is None)
            out.update({f"{name}_node_pairs": pairs, f"{name}_node_pairs_per_s": round(pairs / med),
                        f"{name}_chunks": len(plan["chunks"]), f"{name}_sweep_workgroups": int(plan["chunks"][:, 6].sum()),
                        f"{name}_restrict_workgroups": int(plan["chunks"][:, 3].sum()),
                        f"{name}_workspace_bytes": plan["workspace"], f"{name}_zb": int(plan["zb"].max()),
                        f"{name}_over_rf": round(med / out[f"{name}_rf_s_min_median_max"][1], 2),
                        f"{name}_unshared_same": all(np.array_equal(part[k], res[k]) for k in st.KEYS[:3])})
            runs[name] = (rows, res)
        off, leaf, adj = (np.array(x) for x in src.forest.tables()[:3])
    rows, res = next(iter(runs.values()))
    ids = list(range(m)) if rows is None else rows
    rs = np.random.RandomState(3)
    cells = [(int(i), int(b)) for i, b in zip(rs.randint(0, len(ids), size=sample), rs.randint(0, m, size=sample))]
    cells = cells[:1] if large else cells
    t0 = time.perf_counter()
    same = True
    for i, b in cells:
        a = ids[i]
        want = st.pair_quadratic_tables(leaf[off[a]:off[a + 1]], adj[off[a]:off[a + 1]], leaf[off[b]:off[b + 1]],
                                        adj[off[b]:off[b + 1]])
        same = same and tuple(int(res[k][i, b]) for k in st.KEYS) == tuple(int(x) for x in want)
    common = res["common"].astype(np.int64)
    total = res["triplets"] + res["triplets_other"]
    out.update({"tables_trees": m, "common_leaves_mean": round(float(common.mean()), 1),
                "common_leaves_max": int(common.max()),
                "mean_normalized_triplet_distance": round(float(np.nanmean(np.where(
                    total > 0, (total - 2.0 * res["triplets_shared"]) / np.maximum(total, 1), np.nan))), 4),
                "host_reference_sample": len(cells), "host_reference_agrees": bool(same),
                "host_reference_s_per_cell": round((time.perf_counter() - t0) / max(len(cells), 1), 3)})
    for name in runs:
        out[f"{name}_over_triplets"] = round(out[f"{name}_s_min_median_max"][1] / out["triplets_s_min_median_max"][1], 2)
    return out


# vector lanes of the device per second: 256 CUs x 4 SIMDs x 32 lanes at 2.4 GHz (one 32-bit operation each)
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def run_coverage(dev: Device, size: str, repeats: int = 5, sample: int = 64) -> dict:
    """``scs_score_coverage`` for every taxon on resident tables, min_trees 1 and 2, with and without the two
    matrices: a warm-up and ``repeats`` timed calls each.  Beside them the numpy reference
    (``tests/coverage_reference.py``, ``by_matmul``) on ``sample`` rows, which must give the device's numbers and whose
    time is scaled to all rows, and the word operations the sweep's lanes need at the device's rate."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import coverage_reference as cr

    from spectralclustersupertree_amd.backend import debug_coverage_plan

    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    tips = [arrays.name(i) for i in range(n_taxa)]
    index = {x: i for i, x in enumerate(tips)}
    out = {"size": size, "coverage": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    res = {}
    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        for k in (1, 2):
            out[f"k{k}_s_min_median_max"], res[k, False] = timed(lambda: dev.score_coverage(tabs, min_trees=k))
            out[f"k{k}_matrices_s_min_median_max"], res[k, True] = timed(
                lambda: dev.score_coverage(tabs, min_trees=k, pairs=True))
        plan = debug_coverage_plan(tabs, matrices=2)
        off, leaf = (np.array(x) for x in src.forest.tables()[:2])
    sets = [leaf[off[t]:off[t + 1]].tolist() for t in range(len(off) - 1)]
    rows = np.random.RandomState(3).choice(n_taxa, size=min(sample, n_taxa), replace=False)
    same = True
    for k in (1, 2):
        t0 = time.perf_counter()
        want = cr.by_matmul(sets, n_taxa, k, rows)
        out[f"k{k}_host_reference_s_all_rows"] = round((time.perf_counter() - t0) / len(rows) * n_taxa, 1)
        same = same and np.array_equal(want["occurs"], res[k, True]["occurs"])
        for key in ("pair_trees", "pair_covered", "taxon_covered"):
            same = same and np.array_equal(want[key], res[k, True][key][rows])
        same = same and np.array_equal(res[k, False]["taxon_covered"], res[k, True]["taxon_covered"])
        # the model: every pair a < b that takes part meets every taxon in k trees or more, `variant` words each (one
        # and-or a word, or an and and a popcount); a streamed row has its own words
        pt = res[k, True]["pair_trees"]
        pairs = (int((pt >= k).sum()) - int((np.diagonal(pt) >= k).sum())) // 2
        nc = int((res[k, True]["occurs"] >= k).sum())
        ops = pairs * nc * (plan["variant"] or plan["words"]) * (1 if k == 1 else 2)
        covered = int(res[k, True]["taxon_covered"].sum()) // 3
        med = out[f"k{k}_s_min_median_max"][1]
        out.update({f"k{k}_pairs_swept": pairs, f"k{k}_taxa_walked": nc, f"k{k}_lane_ops": ops,
                    f"k{k}_model_s": round(ops / LANE_OPS_PER_S, 4), f"k{k}_over_model": round(med * LANE_OPS_PER_S / ops, 2)
                    if ops else None, f"k{k}_triples_covered": covered,
                    f"k{k}_coverage": round(covered / (n_taxa * (n_taxa - 1) * (n_taxa - 2) / 6), 6),
                    f"k{k}_host_over_device": round(out[f"k{k}_host_reference_s_all_rows"] / med, 1)})
    out.update({"words": plan["words"], "variant": plan["variant"], "batches_with_matrices": plan["n_batches"],
                "mirror_with_matrices": plan["mirror"], "block_bytes_with_matrices": int(plan["bytes"].max()),
                "host_reference_rows": len(rows), "host_reference_agrees": bool(same)})
    return out


def run_internode(dev: Device, size: str, repeats: int = 3, sample: int = 16) -> dict:
    """``scs_score_internode`` for every taxon on resident tables, without the matrices and with ``pair_weight`` and
    ``dist_sum``: a warm-up and ``repeats`` timed calls each.  Beside them the host reference
    (``tests/internode_reference.py``, ``by_tables``) on ``sample`` rows, which must give the device's numbers and whose
    time is scaled to all rows, and the (pair, tree) evaluations a second: Σ m (m - 1) / 2 evaluations when only a < b
    is swept (``mirror``), twice that otherwise."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import internode_reference as ir

    from spectralclustersupertree_amd.backend import debug_internode_plan

    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    tips = [arrays.name(i) for i in range(n_taxa)]
    index = {x: i for i, x in enumerate(tips)}
    out = {"size": size, "internode": True, "n_taxa": n_taxa, "n_trees": n_trees,
           "leaves": int(arrays.leaf_counts().sum()), "repeats": repeats}

    def timed(call):
        times = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            res = call()
            times.append(time.perf_counter() - t0)
        return [round(x, 5) for x in _spread(times[1:])], res

    with _resident_tables(dev, arrays, tips, index) as src:
        tabs = src.tabs
        out["s_min_median_max"], lean = timed(lambda: dev.score_internode(tabs, matrices=False))
        out["matrices_s_min_median_max"], full = timed(lambda: dev.score_internode(tabs))
        plans = {m: debug_internode_plan(tabs, matrices=m) for m in (0, 2)}
        off, leaf, adj = (np.array(x) for x in src.forest.tables()[:3])
    specs = [(leaf[off[t]:off[t + 1]].tolist(), adj[off[t]:off[t + 1] - 1].tolist()) for t in range(len(off) - 1)]
    rows = np.random.RandomState(3).choice(n_taxa, size=min(sample, n_taxa), replace=False)
    t0 = time.perf_counter()
    want = ir.by_tables(specs, n_taxa, None, rows)
    out["host_reference_s_all_rows"] = round((time.perf_counter() - t0) / len(rows) * n_taxa, 1)
    same = all(np.array_equal(want[k], full[k][rows]) for k in ir.KEYS if full[k] is not None)
    same = same and all(np.array_equal(lean[k], full[k]) for k in ir.KEYS if lean[k] is not None)
    sizes = np.diff(off)
    pairs = int((sizes * (sizes - 1) // 2).sum())
    for name, key, m in (("", "s_min_median_max", 0), ("matrices_", "matrices_s_min_median_max", 2)):
        evals = pairs * (1 if plans[m]["mirror"] else 2)
        out.update({f"{name}evaluations": evals, f"{name}evaluations_per_s": round(evals / out[key][1]),
                    f"{name}mirror": plans[m]["mirror"], f"{name}row_batches": plans[m]["n_row_batches"],
                    f"{name}block_bytes": plans[m]["bytes"]})
    out.update({"tree_batches": plans[0]["n_tree_batches"], "levels": plans[0]["levels"], "words": plans[0]["words"],
                "tiles_per_item": plans[0]["tiles_per_item"], "pairs_in_trees": pairs,
                "missing_pairs": n_taxa * (n_taxa - 1) // 2 - int(lean["taxon_partners"].astype(np.int64).sum()) // 2,
                "host_over_device": round(out["host_reference_s_all_rows"] / out["s_min_median_max"][1], 1),
                "host_reference_rows": len(rows), "host_reference_agrees": bool(same)})
    return out


def _queries(sup: TreeNode, n: int) -> list[str]:
    """``n`` tip names of the supertree, evenly spread over its leaf order (the same for every run)."""
    tips = sup.get_tip_names()
    return [tips[i] for i in np.linspace(0, len(tips) - 1, num=min(n, len(tips)), dtype=np.int64)]


def _spread(values) -> tuple[float, float, float]:
    v = sorted(values)
    return v[0], v[len(v) // 2], v[-1]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--size", action="append", help="NxM or NxMxK; repeatable (default: the three sizes)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--triplets", action="store_true", help="also count the rooted triplet terms")
    ap.add_argument("--conflicts", action="store_true", help="also count the clade conflicts")
    ap.add_argument("--concordance", action="store_true", help="also count the branch concordance factors")
    ap.add_argument("--branch-triplets", action="store_true", help="also count the per-branch triplet support")
    ap.add_argument("--taxon-triplets", action="store_true", help="also count the per-taxon triplet support")
    ap.add_argument("--placements", type=int, default=0, metavar="N",
                    help="also the placement support of N taxa spread over the supertree's leaf order")
    ap.add_argument("--clade-placements", type=int, default=0, metavar="N",
                    help="also the placement support of N clades (the choice of score_supertree(clade_placements=N))")
    ap.add_argument("--clade-max-tips", type=int, default=64, help="the largest clade --clade-placements considers")
    ap.add_argument("--large-clade", action="store_true",
                    help="also the placement support of one clade: the first child of the root's first child")
    ap.add_argument("--placements-as-clade-tips", action="store_true",
                    help="--placements N with N = the number of tips the query clades hold in all")
    ap.add_argument("--refine", action="store_true",
                    help="time refine_supertree instead (a model tree with planted regrafts; --planted N)")
    ap.add_argument("--planted", type=int, default=20, help="how many clades --refine regrafts at random")
    ap.add_argument("--polytomies", action="store_true",
                    help="time scs_score_polytomies instead (a supertree with collapsed edges; --collapse N)")
    ap.add_argument("--collapse", type=int, default=4, help="how many nodes --polytomies collapses to each degree")
    ap.add_argument("--branch-resample", type=int, action="append", metavar="R",
                    help="time scs_score_branch_resample instead, with R weight rows (repeatable)")
    ap.add_argument("--parsimony", action="store_true",
                    help="time scs_score_parsimony instead, without and with the per-clade lengths")
    ap.add_argument("--source-pairs", action="store_true",
                    help="time scs_score_source_pairs instead: every pair of the synthetic sources")
    ap.add_argument("--source-triplets", action="store_true",
                    help="time scs_score_source_pair_triplets instead: one row and 16 rows of 10000x500, every pair of "
                         "20000x2000x500")
    ap.add_argument("--coverage", action="store_true",
                    help="time scs_score_coverage instead: the triple coverage of the synthetic sources")
    ap.add_argument("--coverage-sample", type=int, default=64, metavar="ROWS",
                    help="the rows --coverage checks against the numpy reference")
    ap.add_argument("--internode", action="store_true",
                    help="time scs_score_internode instead: the summed internode distances of the synthetic sources, "
                         "with and without the matrices")
    ap.add_argument("--caterpillar-supertree", action="store_true",
                    help="a caterpillar supertree on a random taxon order against the synthetic sources")
    ap.add_argument("--caterpillar", action="store_true",
                    help="a caterpillar supertree in taxon order against caterpillar sources in reverse order")
    args = ap.parse_args()
    if args.branch_resample:
        with Device(0) as dev:
            run_resample(dev, "200x6", [3], repeats=1)  # warm-up
            for size in args.size or SIZES[:1]:
                print(json.dumps(run_resample(dev, size, args.branch_resample)), flush=True)
        return
    if args.parsimony:
        with Device(0) as dev:
            run_parsimony(dev, "200x6", repeats=1)  # warm-up
            for size in args.size or SIZES[:1]:
                print(json.dumps(run_parsimony(dev, size, max(args.repeats, 5))), flush=True)
        return
    if args.source_pairs:
        with Device(0) as dev:
            run_source_pairs(dev, "200x6", repeats=1, sample=4)  # warm-up
            for size in args.size or SIZES[:1]:
                print(json.dumps(run_source_pairs(dev, size, args.repeats)), flush=True)
        return
    if args.source_triplets:
        with Device(0) as dev:
            run_source_triplets(dev, "200x6", repeats=1, sample=4)  # warm-up
            for size in args.size or ("10000x500", "20000x2000x500"):
                print(json.dumps(run_source_triplets(dev, size, max(args.repeats, 5))), flush=True)
        return
    if args.coverage:
        with Device(0) as dev:
            run_coverage(dev, "200x6", repeats=1, sample=4)  # warm-up
            for size in args.size or ("10000x500", "20000x2000x500"):
                print(json.dumps(run_coverage(dev, size, max(args.repeats, 3), args.coverage_sample)), flush=True)
        return
    if args.internode:
        with Device(0) as dev:
            run_internode(dev, "200x6", repeats=1, sample=4)  # warm-up
            for size in args.size or ("10000x500", "20000x2000x500"):
                print(json.dumps(run_internode(dev, size, max(args.repeats, 3))), flush=True)
        return
    if args.polytomies:
        with Device(0) as dev:
            run_polytomies(dev, "200x6", per_degree=1, repeats=1)  # warm-up
            for size in args.size or SIZES[:1]:
                print(json.dumps(run_polytomies(dev, size, args.collapse)), flush=True)
        return
    if args.refine:
        with Device(0) as dev:
            run_refine(dev, "60x6", planted=2, repeats=1)  # warm-up
            for size in args.size or SIZES[:1]:
                print(json.dumps(run_refine(dev, size, args.planted)), flush=True)
        return
    with Device(0) as dev:
        score_supertree(random_binary_tree(0, 50), synthetic.tree_arrays(0, 50, 4), triplets=args.triplets,
                        conflicts=args.conflicts, concordance=args.concordance, branch_triplets=args.branch_triplets,
                        taxon_triplets=args.taxon_triplets,
                        placements=2 if args.placements or args.placements_as_clade_tips else None,
                        clade_placements=2 if args.clade_placements or args.large_clade else None,
                        device=dev)  # warm-up
        for size in args.size or SIZES:
            reps = 1 if int(size.split("x")[0]) * int(size.split("x")[1]) > 10**8 else args.repeats
            print(json.dumps(run(dev, size, reps, args.triplets, args.conflicts, args.caterpillar,
                                 args.concordance, args.branch_triplets, args.taxon_triplets,
                                 args.caterpillar_supertree, args.placements, args.clade_placements,
                                 args.clade_max_tips, args.large_clade, args.placements_as_clade_tips)),
                  flush=True)


if __name__ == "__main__":
    main()
