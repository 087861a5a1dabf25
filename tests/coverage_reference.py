"""Host references for the triple coverage of the sources (``scs_score_coverage``).

The sources are given as the taxon sets of their trees (the coverage reads nothing else of a tree).  M[x] is the set
of trees that hold taxon x, cov(a, b, c) = |M[a] ∩ M[b] ∩ M[c]|, and a triple of three distinct taxa is covered when
cov >= k.  Two independent references -- ``by_sets`` walks ``itertools.combinations`` over Python sets (a few dozen
taxa), ``by_matmul`` takes cov(a, ., .) of a row taxon from one float64 product, exact because every entry is a small
integer -- the invariants any answer must keep, and a restatement of the library's plan."""

import itertools
import random

import numpy as np
import parsimony_reference as pr

KEYS = ("occurs", "pair_trees", "pair_covered", "taxon_covered")


def tables(sets, n_taxa: int):
    """Flattened tables whose tree t is a star on ``sets[t]`` (a one-leaf tree is the leaf)."""
    return pr.tables([list(s) if len(s) != 1 else list(s)[0] for s in sets], n_taxa)


def random_sets(rng: random.Random, n_taxa: int, n_trees: int, lo: int, hi: int) -> list:
    return [rng.sample(range(n_taxa), rng.randint(min(lo, n_taxa), min(hi, n_taxa))) for _ in range(n_trees)]


def membership(sets, n_taxa: int) -> np.ndarray:
    """B[x][t] = 1 when tree t holds taxon x (taxa x trees, float64)."""
    b = np.zeros((n_taxa, len(sets)), dtype=np.float64)
    for t, s in enumerate(sets):
        b[list(s), t] = 1.0
    return b


def by_sets(sets, n_taxa: int, k: int = 1, rows=None) -> dict:
    trees_of = [set() for _ in range(n_taxa)]
    for t, s in enumerate(sets):
        for x in s:
            trees_of[x].add(t)
    pair_trees = np.zeros((n_taxa, n_taxa), dtype=np.int32)
    pair_covered = np.zeros((n_taxa, n_taxa), dtype=np.int32)
    taxon_covered = np.zeros(n_taxa, dtype=np.int64)
    for a in range(n_taxa):
        for b in range(n_taxa):
            pair_trees[a, b] = len(trees_of[a] & trees_of[b])
    covered = 0
    for a, b, c in itertools.combinations(range(n_taxa), 3):
        if len(trees_of[a] & trees_of[b] & trees_of[c]) >= k:
            covered += 1
            for x, y in ((a, b), (a, c), (b, c)):
                pair_covered[x, y] += 1
                pair_covered[y, x] += 1
            taxon_covered[[a, b, c]] += 1
    ids = np.arange(n_taxa) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    out = {"occurs": np.array([len(s) for s in trees_of], dtype=np.int32).reshape(n_taxa),
           "pair_trees": pair_trees[ids], "pair_covered": pair_covered[ids], "taxon_covered": taxon_covered[ids]}
    if rows is None:
        out["covered"] = covered
    return out


def by_matmul(sets, n_taxa: int, k: int = 1, rows=None) -> dict:
    b = membership(sets, n_taxa)
    ids = np.arange(n_taxa) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    pair_trees = np.zeros((len(ids), n_taxa), dtype=np.int32)
    pair_covered = np.zeros((len(ids), n_taxa), dtype=np.int32)
    others = np.ones(n_taxa, dtype=bool)
    for i, a in enumerate(ids.tolist()):
        cov = (b * b[a]) @ b.T                       # cov[x][y] = cov(a, x, y); cov[x][x] = |M[a] ∩ M[x]|
        pair_trees[i] = np.rint(np.diag(cov)).astype(np.int32)
        hit = cov >= k
        hit[np.arange(n_taxa), np.arange(n_taxa)] = False   # c != b
        hit[:, a] = False                                   # c != a
        others[:] = True
        others[a] = False
        pair_covered[i] = np.where(others, hit.sum(axis=1), 0)
    out = {"occurs": np.rint(b.sum(axis=1)).astype(np.int32).reshape(n_taxa), "pair_trees": pair_trees,
           "pair_covered": pair_covered, "taxon_covered": pair_covered.sum(axis=1, dtype=np.int64) // 2}
    if rows is None:
        out["covered"] = int(out["taxon_covered"].sum()) // 3
    return out


def check_invariants(res: dict, n_taxa: int, k: int, rows=None) -> None:
    """What the four outputs of one call must keep, whatever the sources."""
    ids = np.arange(n_taxa) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    occurs, pt, pc, tc = (res[key] for key in KEYS)
    assert occurs.dtype == np.int32 and occurs.shape == (n_taxa,)
    assert pt.dtype == pc.dtype == np.int32 and pt.shape == pc.shape == (len(ids), n_taxa)
    assert tc.dtype == np.int64 and tc.shape == (len(ids),)
    at = np.arange(len(ids))
    assert np.array_equal(pt[at, ids], occurs[ids]) and not pc[at, ids].any()          # the diagonal rule
    assert np.array_equal(pt[:, ids], pt[:, ids].T) and np.array_equal(pc[:, ids], pc[:, ids].T)  # symmetric
    assert np.array_equal(pc.sum(axis=1, dtype=np.int64), 2 * tc)
    assert (pc >= 0).all() and (pc <= max(n_taxa - 2, 0)).all() and not pc[pt < k].any()
    assert (pt <= np.minimum(occurs[ids][:, None], occurs[None, :])).all()
    if rows is None:
        assert tc.sum() % 3 == 0
        if "covered" in res:
            assert tc.sum() == 3 * res["covered"]


def check_monotone(res_k: dict, res_k1: dict) -> None:
    """The counts at k + 1 against those at k: monotone non-increasing in k."""
    assert (res_k1["pair_covered"] <= res_k["pair_covered"]).all()
    assert (res_k1["taxon_covered"] <= res_k["taxon_covered"]).all()
    assert np.array_equal(res_k1["pair_trees"], res_k["pair_trees"])


# ------------------------------------------------------------------------------------------------ the plan
BUDGET = 3 << 29
REG_WORDS_MAX = 64
TILE, CHUNK, THREADS = 64, 256, 256
GRID_MAX, ITEMS_MAX = 1 << 30, (1 << 32) - 1


def _up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def plan(n_trees: int, n_taxa: int, n_rows=None, min_trees: int = 1, batch_rows: int = 0, reg_words: int = 0,
         matrices: int = 0) -> dict:
    """What ``backend.debug_coverage_plan`` must answer, worked out here."""
    n = n_taxa
    all_rows = n_rows is None
    nr = n if all_rows else n_rows
    words = max((n_trees + 31) // 32, 1)
    cap = min(reg_words, REG_WORDS_MAX) if reg_words > 0 else REG_WORDS_MAX
    v = 4
    while v < words and v < REG_WORDS_MAX:
        v *= 2
    variant = v if words <= v <= cap else 0
    wp = variant or words
    n_pad, ncs = _up(max(n, 1), 64), _up(max(n, 1), 2 * CHUNK)
    tiles = (n + TILE - 1) // TILE
    row_bytes = 8 + matrices * 4 * n
    per = max(1, BUDGET // row_bytes)
    if batch_rows > 0:
        per = min(per, batch_rows)
    first = list(range(0, nr, per))
    rows = [min(per, nr - r) for r in first]
    fixed = sum(_up(b, 256) for b in (4, 4 * nr, 4 * n, 4 * n, 8 * max(nr, n), 4 * max(n, 1) * wp, 4 * words * n_pad,
                                      4 * wp * ncs))
    grid_limit = min(GRID_MAX, ITEMS_MAX // THREADS)
    rows_per_launch = max(grid_limit // max(tiles, 1), 1)
    out_rows = min(per, nr)
    return {"words": words, "variant": variant, "bits_stride": wp, "taxa_stride": n_pad, "tiles": tiles,
            "row_bytes": row_bytes, "fixed_bytes": fixed, "n_batches": len(first), "grid_limit": grid_limit,
            "rows_per_launch": rows_per_launch, "mirror": int(all_rows and (matrices == 0 or len(first) <= 1)),
            "count": int(min_trees > 1), "first_row": np.array(first, dtype=np.int64),
            "rows": np.array(rows, dtype=np.int64),
            "bytes": np.array([fixed + _up(matrices * out_rows * n * 4, 256)] * len(first), dtype=np.int64),
            "grid": np.array([min(min(r, rows_per_launch) * tiles, grid_limit) for r in rows], dtype=np.int64)}
