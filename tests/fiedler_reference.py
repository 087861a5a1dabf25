"""Cases and path rules for the per-graph Fiedler solve (``scs_fiedler`` in ``csrc/scs_eig.hip``) at the edges of its
three code paths.  A helper module: pytest collects nothing here, and nothing here needs a device.  DESIGN.md
section 38.

The reference, the checks and the table builders are those of ``small_solve_reference`` (the same operation: the two
leading eigenpairs of S = d^-1/2 W d^-1/2 and scikit-learn's embedding conventions); this module adds the cases and
says which path a case runs on:

* V <= 64: ``k_dense_s`` -> ``k_small_eig`` (two-sided Jacobi; variants of its own at n = 4, 8, 12, n <= 24, above);
* 65 <= V <= 96 with ``block == 0``: ``k_dense_s`` -> ``k_dense_onesided`` (an odd V padded to V + 1);
* otherwise LOBPCG on ``k_symm`` (the fused loop at widths 4 and 8, the legacy loop at 12 and 16; degrees prepared
  synchronously up to 128 vertices).

A case is ``(label, tables, group_start | None, expects_vectors, block, x_init_seed | None)``.
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import small_solve_reference as ssr

JACOBI_MAX = 64  # csrc/scs_eig.hip MAXS: the two-sided Jacobi kernel's largest matrix
ONE_SIDED_MAX = 96  # ... dense_max: the one-sided dense solve up to here (block == 0, one rank)
SYNC_DEGREES_MAX = 128  # ... DENSE2_MAX: the degrees are prepared before anything else up to here
WIDTHS = (16, 12, 8, 4)  # the block widths of the iterative path, widest first
ITERATIVE_GAP = 1e-3  # both gaps of a GENERIC case that runs on LOBPCG (the Davis-Kahan bar of the GPU test)

NEW_GROUPS = ("generic", "widths", "contracted_above_128", "long_paths", "complete_graphs", "two_components_large",
              "isolated_large", "scaled_large")
GROUPS = ssr.FAMILIES + NEW_GROUPS


def path_of(v: int, block: int) -> str:
    """``two_sided``, ``one_sided`` or ``iterative``: the path ``scs_fiedler`` takes on one rank."""
    if v <= JACOBI_MAX:
        return "two_sided"
    if v <= ONE_SIDED_MAX and block == 0:
        return "one_sided"
    return "iterative"


def width_of(v: int, block: int) -> int:
    """The block width the iterative path reports below 4 096 vertices: 4 by default, else the widest allowed width
    that is at most what was asked for and leaves room for 3 b basis vectors and the constraint (3 b + 2 <= V)."""
    want = block or 4
    cap = (v - 2) // 3
    return next((a for a in WIDTHS if a <= want and a <= cap), 4)


def vertices(case) -> int:
    _, tables, gs, *_ = case
    return tables.n_taxa if gs is None else len(gs) - 1


def x_init(case):
    """The start vector of a case as the product draws it, or None."""
    seed = case[5]
    return None if seed is None else np.random.RandomState(seed).uniform(-1, 1, vertices(case))


def _generic(seed: int, n: int, strategy: str, group_start=None, block: int = 0, m: int = 12):
    """``small_solve_reference.generic_tables`` with the gaps the case's path needs, judged on the oracle's W."""
    v = n if group_start is None else len(group_start) - 1
    iterative = path_of(v, block) == "iterative"
    for s in range(seed, seed + 50):
        tables = ssr.mixed_tables(s, n, m, strategy)
        g1, g2 = ssr.gaps(ssr.oracle_w(tables, group_start))
        if min(g1, g2) > (ITERATIVE_GAP if iterative else 10 * ssr.GAP):
            return tables
    raise AssertionError(f"no generic node for {(seed, n, m, strategy, block)}")


class _Seeds:
    """Every second iterative case of a group gets a start vector."""

    def __init__(self, base: int) -> None:
        self.base, self.count = base, 0

    def next(self, v: int, block: int):
        if path_of(v, block) != "iterative":
            return None
        self.count += 1
        return self.base + self.count if self.count % 2 else None


GENERIC_SMALL = (5, 12, 13)  # the k_small_eig variants that the families of small_solve_reference miss
GENERIC_SIZES = (95, 96, 97, 129, 255, 256, 257, 1025)
FORCED_WIDTHS = ((65, 4), (65, 16), (96, 8), (96, 12), (97, 8), (257, 12), (257, 16))


@functools.lru_cache(maxsize=None)
def generic():
    out, seeds = [], _Seeds(5000)
    for i, n in enumerate(GENERIC_SMALL + GENERIC_SIZES):
        strategy = ssr.STRATEGIES[i % 4]
        tables = _generic(50000 + 50 * i, n, strategy)
        out.append((f"generic-n{n}-{strategy}", tables, None, True, 0, seeds.next(n, 0)))
    return out


@functools.lru_cache(maxsize=None)
def widths():
    out, seeds = [], _Seeds(5100)
    for i, (n, block) in enumerate(FORCED_WIDTHS):
        strategy = ssr.STRATEGIES[(i + 1) % 4]
        tables = _generic(51000 + 50 * i, n, strategy, block=block)
        out.append((f"widths-n{n}-b{block}-{strategy}", tables, None, True, block, seeds.next(n, block)))
    return out


CONTRACTED_ABOVE_128 = ((200, (2, 3, 24, 25, 64, 65, 95, 96)), (300, (97, 129)))


@functools.lru_cache(maxsize=None)
def contracted_above_128():
    """Why the dense per-graph paths exist in the product: a node of more than 128 taxa whose graph contracts to a
    handful of vertices."""
    out, seeds, i = [], _Seeds(5200), 0
    for n, groups in CONTRACTED_ABOVE_128:
        for v in groups:
            for tag, gs in (("cuts", ssr.random_cuts(np.random.RandomState(100 * n + v), n, v)),
                            ("big", ssr.one_big_group(n, v))):
                strategy = ssr.STRATEGIES[i % 4]
                tables = _generic(52000 + 50 * i, n, strategy, gs)
                out.append((f"contracted-n{n}-v{v}-{tag}-{strategy}", tables, gs, True, 0, seeds.next(v, 0)))
                i += 1
    return out


LONG_PATHS = (95, 96, 97, 129, 257)  # one-sided with the eigenvalue -1 (odd and even), then iterative


@functools.lru_cache(maxsize=None)
def long_paths():
    seeds = _Seeds(5300)
    return [(f"path-n{n}", ssr.path_tables(n), None, True, 0, seeds.next(n, 0)) for n in LONG_PATHS]


COMPLETE_GRAPHS = ((95, 0), (96, 0), (97, 0), (129, 0), (65, 4))


@functools.lru_cache(maxsize=None)
def complete_graphs():
    """K_V: on the iterative path the start block is an eigen-block already (S = -1 / (V - 1) on the complement of
    the trivial vector): the residual is 0 and R is the zero block."""
    seeds = _Seeds(5400)
    return [(f"complete-v{v}" + (f"-b{block}" if block else ""), ssr.star_tables(v, 1.0 + 0.25 * (v % 3)), None, False,
             block, seeds.next(v, block)) for v, block in COMPLETE_GRAPHS]


TWO_COMPONENTS_LARGE = (96, 98, 130, 258)


@functools.lru_cache(maxsize=None)
def two_components_large():
    seeds = _Seeds(5500)
    return [(f"two_components-n{n}", ssr.two_component_tables(n), None, False, 0, seeds.next(n, 0))
            for n in TWO_COMPONENTS_LARGE]


ISOLATED_LARGE = (95, 97, 129, 257)
ISOLATED_OWN_GROUP = (200, 100)  # taxa, vertices: the loner a group of its own


@functools.lru_cache(maxsize=None)
def isolated_large():
    out, seeds = [], _Seeds(5600)
    for n in ISOLATED_LARGE:
        out.append((f"isolated-n{n}", ssr._isolated_tables(n), None, True, 0, seeds.next(n, 0)))
    n, v = ISOLATED_OWN_GROUP
    gs = np.concatenate(([0], ssr.random_cuts(np.random.RandomState(n), n - 1, v - 1) + 1)).astype(np.int32)
    out.append((f"isolated-n{n}-own-group-v{v}", ssr._isolated_tables(n), gs, True, 0, seeds.next(v, 0)))
    return out


GRADED_LARGE = (100, 200)
SCALED_LARGE = 200


@functools.lru_cache(maxsize=None)
def scaled_large():
    """Labels as in ``small_solve_reference.scaled``: ``scale_of`` and ``twin_of`` apply."""
    out, seeds = [], _Seeds(5700)
    for n in GRADED_LARGE:
        graded = ssr._graded_tables(n)
        out.append((f"scaled-graded-lengths-n{n}", graded, None, ssr.vectors_defined(ssr.oracle_w(graded, None)), 0,
                    seeds.next(n, 0)))
    n = SCALED_LARGE
    base = _generic(57000, n, "branch", m=9)
    seed = seeds.next(n, 0)  # (a twin starts where its base starts)
    out.append((f"scaled-n{n}-base", base, None, True, 0, seed))
    for sc in ssr.SCALES:
        twin = dataclasses.replace(base, tree_w=base.tree_w * sc)
        out.append((f"scaled-n{n}-x{sc:g}", twin, None, True, 0, seed))
    return out


def unit_vector_error(w: np.ndarray, maps: np.ndarray) -> float:
    """``small_solve_reference.vector_error`` on the unit-norm scale: max |maps dd - reference dd| over both columns
    (the unit eigenvectors, which a scaling of W leaves alone), either sign where the sign rule ties."""
    if not np.all(np.isfinite(maps)):
        return float("inf")
    ref, _ = ssr.lapack_embedding(w)
    dd = ssr.reference(w)[1]
    want = (ref.astype(ssr.LD) * dd[:, None]).astype(np.float64)
    got = (np.asarray(maps, dtype=np.float64).astype(ssr.LD) * dd[:, None]).astype(np.float64)
    worst = 0.0
    for c in range(2):
        err = float(np.max(np.abs(got[:, c] - want[:, c])))
        mags = np.sort(np.abs(ref[:, c]))[::-1]
        if len(mags) > 1 and mags[0] - mags[1] <= ssr.TIE_REL * mags[0]:
            err = min(err, float(np.max(np.abs(got[:, c] + want[:, c]))))
        worst = max(worst, err)
    return worst


def embedding_bar(w: np.ndarray, scale: float = 1.0) -> float:
    """The bar of the iterative path on the embedding scale (``vector_error(w, maps, scale)``): ``FIEDLER_TOL`` on
    the unit vectors, carried through the division by dd of the unscaled matrix -- taken from the reference."""
    dd = ssr.reference(w)[1] / np.sqrt(ssr.LD(scale))
    return ssr.FIEDLER_TOL * max(1.0, float(np.max(1 / dd)))


def group(name: str):
    """The cases of a group: a family of ``small_solve_reference`` as it stands (``block`` 0, no start vector), or
    one of ``NEW_GROUPS``."""
    if name in ssr.FAMILIES:
        return [(label, tables, gs, expects, 0, None) for label, tables, gs, expects in ssr.family(name)]
    assert name in NEW_GROUPS, name
    return globals()[name]()
