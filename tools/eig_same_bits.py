#!/usr/bin/env python3
"""The bits of scs_fiedler over a fixed grid of solves, one JSON line per solve: the SHA-256 of ``maps`` and the
report's lambda, lambda_next, resid, iterations, n_apply, n_apply32, lowp_renewals, block, converged and
used_constraint.  Two builds of the library solve the same grid bit for bit iff their outputs are equal line for line
(the solves are deterministic: tests/test_gpu_solver_chain_edges.py and test_gpu_fiedler_edges.py assert bit-equal
repeats).  Written for host-side changes of csrc/scs_eig.hip, which must not move a bit.

    python tools/eig_same_bits.py --tree <checkout with its libraries built> --out <file>
    python tools/eig_same_bits.py --compare <file a> <file b> --out profiles/<name>.json

The package, tests/ and oracle/ are imported from ``--tree`` (default: this checkout); a fresh process per tree, with
SCS_DEBUG=1 so that the probe switches of the grid are read.  Every shape is one a test already uses: the cases of
tests/fiedler_reference.py; make_tables(v + 1, v, 12) at v = 4096, 4111, 4160 at widths 4 and 8 under each switch of
the loop; widths 12 and 16, the graph with isolated vertices, max_iter = 1 and tol = 1e-5 at 4111; a matrix-free
graph; the two- and three-rank solves of tests/test_gpu_team_edges.py through its in-process team.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

FIELDS = ("lambda", "lambda_next", "resid", "iterations", "n_apply", "n_apply32", "lowp_renewals", "block",
          "converged", "used_constraint")
SWITCHES = ("SCS_SPLIT_SMALL", "SCS_FOLD_PASS2", "SCS_OVERLAP_PASS1", "SCS_LEGACY_LOOP", "SCS_LOWP", "SCS_NO_MFMA")
GRID_ENV = ({}, {"SCS_SPLIT_SMALL": "1"}, {"SCS_FOLD_PASS2": "0"}, {"SCS_OVERLAP_PASS1": "0"},
            {"SCS_LEGACY_LOOP": "1"}, {"SCS_LOWP": "0"}, {"SCS_LOWP": "1"}, {"SCS_NO_MFMA": "1"})


def compare(a: str, b: str, out: str) -> int:
    la, lb = (Path(p).read_text().splitlines() for p in (a, b))
    differing = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    same = not differing and len(la) == len(lb)
    head = {"verdict": "same bits" if same else "DIFFERENT", "solves": len(lb), "solves_other": len(la),
            "differing_lines": differing, "columns": ["case", "sha256"] + list(FIELDS)}
    # one solve per line, its values in the order of `columns`
    rows = [json.dumps(list(json.loads(x).values()), separators=(",", ":")) for x in lb]
    Path(out).write_text(json.dumps(head)[:-1] + ', "lines": [\n' + ",\n".join(rows) + "\n]}\n")
    print(f"{head['verdict']}: {len(la)} / {len(lb)} solves, {len(differing)} differing lines")
    return 0 if same else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", required=True)
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare, args.out)

    tree, out_path = Path(args.tree).resolve(), Path(args.out).resolve()
    os.chdir(tree)
    sys.path[:0] = [str(tree), str(tree / "tests")]
    os.environ["SCS_DEBUG"] = "1"
    for name in SWITCHES:
        os.environ.pop(name, None)

    import fiedler_reference as fr
    import matrix_free_reference as mf
    import numpy as np
    import test_gpu_team_edges as team

    from spectralclustersupertree_amd import _native as nv
    from spectralclustersupertree_amd import synthetic
    from spectralclustersupertree_amd.backend import Device

    out = open(out_path, "w")

    def emit(case, maps, stats):
        rec = {"case": case, "sha256": hashlib.sha256(np.ascontiguousarray(maps).tobytes()).hexdigest()}
        for f in FIELDS:
            v = stats[f]
            rec[f] = [float(x).hex() for x in v] if isinstance(v, (list, tuple, np.ndarray)) else (
                float(v).hex() if isinstance(v, float) else int(v))
        out.write(json.dumps(rec) + "\n")
        out.flush()

    def solve(g, x0=None, env=None, **kw):
        os.environ.update(env or {})
        try:
            return g.fiedler(x0, **kw)
        except nv.ConvergenceError as e:
            return e.maps, e.stats
        finally:
            for name in env or {}:
                os.environ.pop(name, None)

    dev = Device(0)
    # ---- all three paths and their switches (64|65, 96|97, 128|129)
    for name in fr.GROUPS:
        for case in fr.group(name):
            label, tables, gs, _, block, _ = case
            dtab = dev.upload(tables)
            g = dtab.build()
            dtab.free()
            if gs is not None:
                g = g.contract(gs)
            emit(f"{name}/{label}", *solve(g, fr.x_init(case), block=block))
            g.free()
    # ---- the loop at the group edges, under each of its switches
    for v in (4096, 4111, 4160):
        dtab = dev.upload(synthetic.make_tables(v + 1, v, 12, "branch", random_weights=True))
        g = dtab.build()
        for env in GRID_ENV:
            for block in (4, 8):
                tag = ",".join(f"{k}={x}" for k, x in env.items()) or "default"
                emit(f"full-{v}/b{block}/{tag}", *solve(g, env=env, block=block))
        if v == 4111:
            for block in (12, 16):
                emit(f"full-{v}/b{block}/default", *solve(g, block=block))
            emit(f"full-{v}/max_iter=1", *solve(g, max_iter=1))
            emit(f"full-{v}/tol=1e-5", *solve(g, tol=1e-5))
        g.free()
        dtab.free()
    dtab = dev.upload(synthetic.make_tables(4111, 4111, 3, "branch", leaves_per_tree=int(0.6 * 4111)))
    g = dtab.build()
    emit("isolated-4111", *solve(g))
    g.free()
    dtab.free()
    # ---- matrix-free
    dtab = dev.upload(mf.tables_of("widths"))
    g = dtab.matrix_free_graph(max_block=8)
    emit("matrix-free/widths", *solve(g))
    g.free()
    dtab.free()
    dev.close()
    # ---- multi-rank solves, rows and upper
    for name in sorted(team.SOLVES):
        layout, n, splits, block, isolated = team.SOLVES[name]
        tb = team._solve_tables(n, splits, isolated)
        v0 = np.random.RandomState(0).uniform(-1, 1, n)

        def rank_fn(rank, d):
            dtab = d.upload(tb)
            g = dtab.build(splits[rank], splits[rank + 1], shared=layout == "rows", upper=layout == "upper")
            try:
                return solve(g, v0, block=block)
            finally:
                g.free()
                dtab.free()

        for rank, (maps, stats) in enumerate(team._ranks(len(splits) - 1, rank_fn)):
            emit(f"team/{name}/rank{rank}", maps, stats)
    out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
