"""Times ``score_supertree`` (``scs_score_supertree``) on synthetic forests (``synthetic.tree_arrays``) against a
random binary supertree on all taxa: one JSON line per size with the host / device split.

    python tools/score_bench.py                      # the three sizes below
    python tools/score_bench.py --size 10000x500     # one size; NxM or NxMxK (K leaves per tree)
    python tools/score_bench.py --triplets           # also the rooted triplet terms
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402

from spectralclustersupertree_amd import score_supertree, synthetic  # noqa: E402
from spectralclustersupertree_amd.backend import Device  # noqa: E402
from spectralclustersupertree_amd.tree import TreeNode  # noqa: E402

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


def run(dev: Device, size: str, repeats: int, triplets: bool = False) -> dict:
    dims = [int(x) for x in size.split("x")]
    n_taxa, n_trees = dims[0], dims[1]
    per_tree = dims[2] if len(dims) > 2 else None
    t0 = time.perf_counter()
    arrays = synthetic.tree_arrays(1, n_taxa, n_trees, leaves_per_tree=per_tree)
    sup = random_binary_tree(2, n_taxa)
    gen_s = time.perf_counter() - t0
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = score_supertree(sup, arrays, triplets=triplets, device=dev)
        runs.append((time.perf_counter() - t0, res.timings))
    wall, tim = min(runs, key=lambda r: r[0])
    out = {
        "size": size, "n_taxa": n_taxa, "n_trees": n_trees, "leaves": int(arrays.leaf_counts().sum()),
        "supertree_nodes": len(res.informative), "repeats": repeats, "input_generation_s": round(gen_s, 3),
        "wall_s": round(wall, 4), "host_prepare_s": round(tim["prepare"], 4),
        "device_tables_s": round(tim["tables"], 4), "score_call_s": round(tim["score"], 4),
        "total_rf": res.total_rf, "mean_rf": float(res.rf.mean()),
    }
    if triplets:
        out.update({"triplets_call_s": round(tim["triplets"], 4), "total_triplet_distance": res.total_triplet_distance,
                    "triplet_fit": res.triplet_fit})
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--size", action="append", help="NxM or NxMxK; repeatable (default: the three sizes)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--triplets", action="store_true", help="also count the rooted triplet terms")
    args = ap.parse_args()
    with Device(0) as dev:
        score_supertree(random_binary_tree(0, 50), synthetic.tree_arrays(0, 50, 4), triplets=args.triplets,
                        device=dev)  # warm-up
        for size in args.size or SIZES:
            reps = 1 if int(size.split("x")[0]) * int(size.split("x")[1]) > 10**8 else args.repeats
            print(json.dumps(run(dev, size, reps, args.triplets)), flush=True)


if __name__ == "__main__":
    main()
