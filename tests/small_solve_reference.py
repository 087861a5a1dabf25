"""Reference, checks and cases for the batched small-node solve (``scs_small_solve*``: ``k_small_addends`` ->
``k_small_sum`` -> ``k_small_finish<256|1024>`` / ``k_small_finish_big`` in ``csrc/scs_eig_small.h``).  A helper module:
pytest collects nothing here, and nothing here needs a device.  DESIGN.md section 21.

The reference of a node is built from its contracted W (fp64: the kernel's ``w_out``, bit for bit the oracle's) in
``np.longdouble``: degrees as column sums, dd = sqrt(d) with dd = 1 where d = 0, S = (W / dd) / dd^T symmetrised, zero
diagonal.  ``check_node`` holds ANY returned ``(maps, lambda)`` to it -- degenerate or not -- as an eigen-pair;
``compare_vectors`` compares with LAPACK's eigenvectors where those are defined (both gaps above 1e-6).

The bars are the project's own (DESIGN.md sections 6 and 19, on a matrix of norm 1 -- and ||S||_2 = 1): eigenvalues
1e-12, residual 1e-11, orthonormality 1e-12, embedding entries 1e-10 (``FIEDLER_TOL``), and the sign-tie rule of
``tests/test_gpu_parity.py`` (two largest magnitudes within 1e-9 relative: either sign).
"""

from __future__ import annotations

import dataclasses
import functools
import random

import numpy as np
from reference_cases import INLINE_CASES
from solver_reference import LD, require_extended_precision

from oracle import tables_oracle as to
from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd import synthetic
from spectralclustersupertree_amd.tree import TreeNode, make_tree

LAMBDA_BAR = 1e-12
RESIDUAL_BAR = 1e-11
ORTH_BAR = 1e-12
FIEDLER_TOL = 1e-10
TIE_REL = 1e-9
GAP = 1e-6  # below this distance of lambda_1, lambda_2, lambda_3 the eigenvectors are not compared entry by entry

SMALL_TR_MAX = 24  # csrc/scs_eig_small.h: the addend layout changes above this many TAXA (and k_small_finish<256> gives
#                    way to <1024> above as many VERTICES)
TWO_SIDED_MAX = 64  # ... and k_small_finish to k_small_finish_big above this many TAXA
STRATEGIES = ("one", "depth", "branch", "bootstrap")
FAMILIES = ("sizes", "contracted", "two_vertices", "complete", "two_squares", "path", "isolated", "two_components",
            "scaled")


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def reference(w: np.ndarray):
    """(S, dd) in extended precision from the contracted fp64 W."""
    require_extended_precision()
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    np.fill_diagonal(wl, 0)
    d = wl.sum(axis=0)
    dd = np.where(d == 0, LD(1), np.sqrt(np.where(d == 0, LD(1), d)))
    s = (wl / dd[None, :]) / dd[:, None]
    s = (s + s.T) / 2
    np.fill_diagonal(s, 0)
    return s, dd


def eigenvalues(w: np.ndarray) -> np.ndarray:
    """Eigenvalues of S, descending (LAPACK on the fp64 rounding of the extended-precision S)."""
    return np.linalg.eigvalsh(reference(w)[0].astype(np.float64))[::-1]


def gaps(w: np.ndarray):
    """(lambda_1 - lambda_2, lambda_2 - lambda_3); a matrix of two vertices has no third eigenvalue: inf."""
    ev = eigenvalues(w)
    return float(ev[0] - ev[1]), (float(ev[1] - ev[2]) if len(ev) > 2 else float("inf"))


def vectors_defined(w: np.ndarray) -> bool:
    g1, g2 = gaps(w)
    return g1 > GAP and g2 > GAP


def sign_tied(w: np.ndarray) -> bool:
    """True when the sign rule does not fix the SECOND column of the reference embedding: its two largest magnitudes
    tie."""
    ref, _ = lapack_embedding(w)
    # (the first column of a connected graph is the constant 1 / ||sqrt(d)||, tied at every node: only the second tells)
    mags = np.sort(np.abs(ref[:, 1]))[::-1]
    return bool(len(mags) > 1 and mags[0] - mags[1] <= TIE_REL * mags[0])


def _sign_ok(col: np.ndarray) -> bool:
    mags = np.abs(col)
    order = np.argsort(-mags, kind="stable")
    if col[order[0]] > 0:
        return True
    return len(col) > 1 and mags[order[0]] - mags[order[1]] <= TIE_REL * mags[order[0]]


def node_errors(w: np.ndarray, maps: np.ndarray, lam: np.ndarray, exact: int = 3) -> dict:
    """The figures ``check_node`` judges: finite, norm, orth, residual, lambda, tail, sign.  ``exact``: how many
    leading entries of ``lam`` are eigenvalues (3: the dense solves).  With 2 (the iterative per-graph solve,
    ``fiedler_reference``) ``lam[2]`` is an unconverged Ritz value of a block orthogonal to what has converged: by
    Cauchy interlacing at most lambda_3, and at most ``lam[1]`` (the Ritz values come in order); ``lambda_next`` is
    how far it exceeds either, and it has no lower bar."""
    assert exact in (2, 3), exact
    v = w.shape[0]
    maps = np.asarray(maps, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    assert maps.shape == (v, 2) and lam.shape == (3,), (maps.shape, lam.shape, v)
    out = {"finite": bool(np.all(np.isfinite(maps)) and np.all(np.isfinite(lam)))}
    if not out["finite"]:
        return out
    s, dd = reference(w)
    x = maps.astype(LD) * dd[:, None]
    out["norm"] = float(max(abs(np.sqrt((x[:, c] * x[:, c]).sum()) - 1) for c in range(2)))
    out["orth"] = float(abs((x[:, 0] * x[:, 1]).sum()))
    out["residual"] = float(max(np.max(np.abs(s @ x[:, c] - LD(lam[c]) * x[:, c])) for c in range(2)))
    ev = np.linalg.eigvalsh(s.astype(np.float64))[::-1]
    k = min(exact, v)
    out["lambda"] = float(np.max(np.abs(lam[:k] - ev[:k])))
    if exact == 2 and v > 2:
        out["lambda_next"] = float(max(lam[2] - ev[2], lam[2] - lam[1]))
    out["tail"] = bool(np.all(lam[v:] == 0))
    out["sign"] = bool(_sign_ok(maps[:, 0]) and _sign_ok(maps[:, 1]))
    return out


def check_node(w: np.ndarray, maps: np.ndarray, lam: np.ndarray, exact: int = 3) -> dict:
    """Holds one node's ``(maps, lambda)`` to the reference of its W, whatever its spectrum; returns the figures.
    ``exact``: see ``node_errors``."""
    e = node_errors(w, maps, lam, exact)
    assert e["finite"], f"non-finite output: maps {maps!r} lambda {lam!r}"
    assert e["norm"] <= ORTH_BAR, f"| ||x_c|| - 1 | = {e['norm']:.3e} > {ORTH_BAR}"
    assert e["orth"] <= ORTH_BAR, f"|x_0^T x_1| = {e['orth']:.3e} > {ORTH_BAR}"
    assert e["residual"] <= RESIDUAL_BAR, f"max|S x - lambda x| = {e['residual']:.3e} > {RESIDUAL_BAR}"
    assert e["lambda"] <= LAMBDA_BAR, f"|lambda - LAPACK| = {e['lambda']:.3e} > {LAMBDA_BAR} ({lam!r})"
    if "lambda_next" in e:
        # (against lambda_3 with the eigenvalue bar; against lam[1] exactly: both are the solver's own numbers)
        assert e["lambda_next"] <= LAMBDA_BAR and lam[2] <= lam[1], (
            f"lambda_next {lam[2]!r} above lambda_3 + {LAMBDA_BAR} or above lambda[1] {lam[1]!r}")
    assert e["tail"], f"lambda beyond the vertex count is not 0: {lam!r}"
    assert e["sign"], "the entry of largest magnitude of a column is negative (and no tie)"
    return e


def lapack_embedding(w: np.ndarray):
    """``(maps, lambda)`` as LAPACK and the embedding conventions give them from the fp64 S: the two leading unit
    eigenvectors divided by dd, the entry of largest magnitude of each column positive; lambda padded with zeros."""
    s, dd = reference(w)
    ev, vec = np.linalg.eigh(s.astype(np.float64))
    vec = vec[:, ::-1][:, :2] / dd.astype(np.float64)[:, None]
    lam = np.zeros(3)
    k = min(3, len(ev))
    lam[:k] = ev[::-1][:k]
    return to.sign_flip_columns(vec), lam


def vector_error(w: np.ndarray, maps: np.ndarray, scale: float = 1.0) -> float:
    """max |maps sqrt(scale) - reference| over both columns, either sign where the sign rule ties.  ``scale``: W is
    ``scale`` times a matrix of ordinary size, and the comparison is made on that matrix's embedding."""
    ref, _ = lapack_embedding(w)
    rt = float(np.sqrt(LD(scale)))
    ref, got = ref * rt, np.asarray(maps, dtype=np.float64) * rt
    worst = 0.0
    for c in range(2):
        err = float(np.max(np.abs(got[:, c] - ref[:, c])))
        mags = np.sort(np.abs(ref[:, c]))[::-1]
        if len(mags) > 1 and mags[0] - mags[1] <= TIE_REL * mags[0]:
            err = min(err, float(np.max(np.abs(got[:, c] + ref[:, c]))))
        worst = max(worst, err)
    return worst


def compare_vectors(w: np.ndarray, maps: np.ndarray, scale: float = 1.0) -> float:
    """Only where both gaps exceed 1e-6: the embedding against LAPACK's at ``FIEDLER_TOL``."""
    assert vectors_defined(w), f"compare_vectors on a degenerate node (gaps {gaps(w)})"
    err = vector_error(w, maps, scale)
    assert np.all(np.isfinite(maps)) and err <= FIEDLER_TOL, f"|maps - LAPACK| = {err:.3e} > {FIEDLER_TOL}"
    return err


def oracle_w(tables, group_start) -> np.ndarray:
    w, _ = to.pcg_dense(tables)
    if group_start is not None:
        w = to.contract_dense(w, group_start)
    return w


# ---------------------------------------------------------------------------------------------------------------
# building blocks of the cases
# ---------------------------------------------------------------------------------------------------------------
def merge_tables(parts, n_taxa: int):
    """The trees of several table sets over the same taxa, dealt round-robin into one set (part 0's first tree,
    part 1's first tree, ..., part 0's second tree, ...): neighbouring trees of different leaf counts."""
    trees = []
    for i in range(max(p.n_trees for p in parts)):
        trees.extend((p, i) for p in parts if i < p.n_trees)
    off = [0]
    lt, ad, av, tw = [], [], [], []
    for p, i in trees:
        a, b = int(p.tree_off[i]), int(p.tree_off[i + 1])
        lt.append(p.leaf_taxon[a:b])
        ad.append(p.adj_depth[a:b])
        av.append(p.adj_val[a:b])
        tw.append(p.tree_w[i])
        off.append(off[-1] + b - a)
    return fl.TreeTables(n_taxa, np.asarray(off, dtype=np.int64), np.ascontiguousarray(np.concatenate(lt), np.int32),
                         np.ascontiguousarray(np.concatenate(ad), np.int32),
                         np.ascontiguousarray(np.concatenate(av), np.float64), np.asarray(tw, dtype=np.float64),
                         parts[0].taxa, monotone=all(p.monotone for p in parts))


def mixed_tables(seed: int, n: int, m: int, strategy: str):
    """``m`` synthetic trees over ``n`` taxa: trees of n, n / 2 and 2 leaves in turn (a two-leaf tree is one gap at
    the root: its addends are all +0.0 -- it exercises the staging, not the weights)."""
    counts = [len(range(j, m, 3)) for j in range(3)]
    ks = [n, max(2, n // 2), 2]
    parts = [synthetic.make_tables(seed + 7919 * j, n, c, strategy, leaves_per_tree=k, random_weights=True)
             for j, (c, k) in enumerate(zip(counts, ks)) if c]
    return merge_tables(parts, n)


def generic_tables(seed: int, n: int, m: int, strategy: str, group_start=None):
    """``mixed_tables`` at the first seed (seed, seed + 1, ...) whose (contracted) S has both gaps above 1e-5, so
    that the eigenvectors are defined with room to spare; judged on the oracle's W, never on a kernel's."""
    for s in range(seed, seed + 50):
        tables = mixed_tables(s, n, m, strategy)
        g1, g2 = gaps(oracle_w(tables, group_start))
        if g1 > 10 * GAP and g2 > 10 * GAP:
            return tables
    raise AssertionError(f"no generic node for {(seed, n, m, strategy)}")


def _names(n: int):
    return [f"t{i:03d}" for i in range(n)]


def _leaf(name: str, length: float = 0.05):
    return TreeNode(name, None, length)


def _join(rng: random.Random, leaves, length=lambda: 0.1):
    """Random binary tree over the leaves (joined in random order), every internal node with a length."""
    nodes = list(leaves)
    rng.shuffle(nodes)
    while len(nodes) > 1:
        kids = [nodes.pop(rng.randrange(len(nodes))) for _ in range(2)]
        nodes.append(TreeNode("", kids, length(), 75.0))
    return nodes[0]


def _unary(tree):
    """The tree under a root with one child: no pair of its leaves is separated by the root."""
    return TreeNode("", [tree])


def star_tables(n: int, omega: float):
    """``((t0,...,tn-1));`` with tree weight omega under strategy ``one``: W = omega off the diagonal, exactly."""
    names = _names(n)
    tree = _unary(TreeNode("", [_leaf(x) for x in names], 1.0, 100.0))
    return fl.flatten_trees([tree], [omega], "one", names)


def equal_groups(n: int, v: int) -> np.ndarray:
    assert n % v == 0
    return np.arange(0, n + 1, n // v, dtype=np.int32)


def random_cuts(rs, n: int, v: int) -> np.ndarray:
    cuts = np.sort(rs.choice(np.arange(1, n), size=v - 1, replace=False))
    return np.concatenate(([0], cuts, [n])).astype(np.int32)


def one_big_group(n: int, v: int) -> np.ndarray:
    """v groups over n taxa: singletons but for one group of n - v + 1 taxa in the middle."""
    sizes = np.ones(v, dtype=np.int64)
    sizes[v // 2] = n - v + 1
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# the families: lists of (name, tables, group_start or None, expects_vectors)
# ---------------------------------------------------------------------------------------------------------------
SIZES_TAXA = (2, 3, 4, 23, 24, 25, 63, 64, 65, 66, 127, 128)
TREE_COUNTS = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192)


def sizes_plan():
    """[(n_taxa, tree count)]: every count of TREE_COUNTS at least once at 3 ... SMALL_TR_MAX taxa, once above, and
    once above 64 taxa.  Three counts a size cannot do that (four such sizes on either side against eighteen counts):
    those sizes take five counts each, the sizes in between and n = 2 (whose W is zero whatever the trees) three."""
    small = [n for n in SIZES_TAXA if 2 < n <= SMALL_TR_MAX]
    big = [n for n in SIZES_TAXA if n > TWO_SIDED_MAX]
    rest = [n for n in SIZES_TAXA if n not in small and n not in big]
    plan = []
    for group, shift in ((small, 0), (big, 7)):
        per = -(-len(TREE_COUNTS) // len(group))
        for i, n in enumerate(group):
            for j in range(per):
                plan.append((n, TREE_COUNTS[(i * per + j + shift) % len(TREE_COUNTS)]))
    for i, n in enumerate(rest):
        for j in range(3):
            plan.append((n, TREE_COUNTS[(5 * i + 6 * j + 2) % len(TREE_COUNTS)]))
    return plan


@functools.lru_cache(maxsize=None)
def sizes():
    out = []
    for i, (n, m) in enumerate(sizes_plan()):
        strategy = STRATEGIES[i % 4]
        name = f"sizes-n{n}-m{m}-{strategy}"
        if n == 2 or m == 1:
            # two taxa are separated by the root of every binary tree (W = 0), and a single binary tree joins no taxon
            # of one root side to the other (two components, unless one side is a single taxon): what the trees
            # give decides whether the eigenvectors are defined
            tables = mixed_tables(3000 + 50 * i, n, m, strategy)
            out.append((name, tables, None, vectors_defined(oracle_w(tables, None))))
        else:
            out.append((name, generic_tables(3000 + 50 * i, n, m, strategy), None, True))
    return out


CONTRACTED_TAXA = (24, 25, 40, 64, 65, 100, 128)
CONTRACTED_GROUPS = (2, 3, 4, 10, 24, 25, 63, 64)


@functools.lru_cache(maxsize=None)
def contracted():
    out = []
    i = 0
    for n in CONTRACTED_TAXA:
        # (v == n: every taxon a group of its own, passed as an explicit identity group_start)
        for v in sorted({g for g in CONTRACTED_GROUPS if g <= n} | {n - 1}):
            layouts = [("cuts", random_cuts(np.random.RandomState(100 * n + v), n, v))]
            if v < n - 1:
                layouts.append(("big", one_big_group(n, v)))
            for tag, gs in layouts:
                strategy = STRATEGIES[i % 4]
                tables = generic_tables(20000 + 50 * i, n, 12, strategy, gs)
                out.append((f"contracted-n{n}-v{v}-{tag}-{strategy}", tables, gs, True))
                i += 1
    return out


TWO_VERTEX_TAXA = (4, 64, 65, 128)
TWO_VERTEX_WEIGHTS = (1.0, 2.0, 3.0, 4.0, 0.3, 7.5, 9.0, 1e-9)


@functools.lru_cache(maxsize=None)
def two_vertices():
    # (the second column is (+-1, -+1) / sqrt(2 omega): its two magnitudes tie, so its sign is not defined)
    return [(f"two_vertices-n{n}-w{omega:g}", star_tables(n, omega),
             np.array([0, n // 3 + 1, n], dtype=np.int32), False)
            for n in TWO_VERTEX_TAXA for omega in TWO_VERTEX_WEIGHTS]


COMPLETE_VERTICES = (3, 5, 24, 25, 64, 65, 128)


@functools.lru_cache(maxsize=None)
def complete():
    """K_V: lambda = (1, -1 / (V - 1) repeated V - 1 times).  Uncontracted, and as equal groups of 2 taxa and of as
    many taxa as 128 allow (V = 65 and 128 have no contracted form within 128 taxa)."""
    out = []
    for v in COMPLETE_VERTICES:
        out.append((f"complete-v{v}", star_tables(v, 1.0 + 0.25 * (v % 3)), None, False))
        for g in sorted({2, 128 // v} - {1}):
            if v * g <= 128:
                out.append((f"complete-v{v}-groups-of-{g}", star_tables(v * g, 2.0), equal_groups(v * g, v), False))
    return out


@functools.lru_cache(maxsize=None)
def two_squares():
    case = next(c for c in INLINE_CASES if c.name == "two_squares")
    trees = [make_tree(s) for s in case.trees]
    names = sorted({x for t in trees for x in t.get_tip_names()})
    tables = fl.flatten_trees(trees, [1.0] * len(trees), case.pcg_weighting, names)
    groups = fl.contraction_groups(tables)
    assert int(groups.max()) + 1 == tables.n_taxa  # nothing contracts
    # (the issue lists this node as the repeated lambda_2 from real input.  It is not one: S of these tables has the gaps
    # 0.27 and 0.5 -- no inline case of the reference has a connected graph with a repeated lambda_2 in S -- so it is
    # a generic node, compared entry by entry, and `complete` is the only repeated-lambda_2 family)
    return [("two_squares", tables, None, vectors_defined(oracle_w(tables, None)))]


PATH_TAXA = (3, 8, 64, 65, 128)


def path_tables(n: int):
    """The path t0 - t1 - ... - t(n-1): one two-leaf tree an edge, weight 1 under strategy ``one``."""
    names = _names(n)
    trees = [_unary(TreeNode("", [_leaf(names[i]), _leaf(names[i + 1])], 1.0, 100.0)) for i in range(n - 1)]
    return fl.flatten_trees(trees, [1.0] * (n - 1), "one", names)


@functools.lru_cache(maxsize=None)
def path():
    return [(f"path-n{n}", path_tables(n), None, True) for n in PATH_TAXA]


ISOLATED_TAXA = (40, 64, 65, 128)


def _isolated_tables(n: int):
    """One taxon that never shares a root side with another (tests/test_gpu_parity.py,
    test_fiedler_with_isolated_vertices): it is the root's own child in every tree that holds it."""
    rng = random.Random(n)
    names = _names(n)
    loner, rest = names[0], names[1:]
    trees = []
    for i in range(12):
        members = rest if i % 2 else rng.sample(rest, 5)
        inner = _join(rng, [_leaf(x, rng.expovariate(10.0)) for x in members], lambda: rng.expovariate(10.0))
        trees.append(TreeNode("", [_leaf(loner), inner]))
    return fl.flatten_trees(trees, [1.0 + 0.1 * i for i in range(12)], "branch", names)


@functools.lru_cache(maxsize=None)
def isolated():
    out = []
    for n in ISOLATED_TAXA:
        tables = _isolated_tables(n)
        out.append((f"isolated-n{n}", tables, None, True))
        v = n // 2
        gs = np.concatenate(([0], random_cuts(np.random.RandomState(n), n - 1, v - 1) + 1)).astype(np.int32)
        out.append((f"isolated-n{n}-own-group-v{v}", tables, gs, True))
    return out


TWO_COMPONENT_TAXA = (10, 64, 90)


def two_component_tables(n: int):
    """Two groups of n / 2 - 1 and n / 2 + 1 taxa that no tree joins: two random trees over either."""
    rng = random.Random(7 * n)
    names = _names(n)
    half = n // 2 - 1
    trees = []
    for side in (names[:half], names[half:], names[:half], names[half:]):
        leaves = [_leaf(x, rng.expovariate(10.0)) for x in side]
        trees.append(_unary(_join(rng, leaves, lambda: rng.expovariate(10.0))))
    return fl.flatten_trees(trees, [1.0, 1.5, 0.75, 2.0], "branch", names)


@functools.lru_cache(maxsize=None)
def two_components():
    return [(f"two_components-n{n}", two_component_tables(n), None, False) for n in TWO_COMPONENT_TAXA]


SCALES = (1e150, 1e-150)


def _graded_tables(n: int):
    """Branch lengths 10^u, u uniform over -12 ... 12, under strategy ``branch``; every tree under a unary root."""
    rng = random.Random(4242)
    names = _names(n)
    grade = lambda: 10.0 ** rng.uniform(-12, 12)  # noqa: E731
    trees = [_unary(_join(rng, [_leaf(x, grade()) for x in names], grade)) for _ in range(6)]
    return fl.flatten_trees(trees, [1.0] * 6, "branch", names)


@functools.lru_cache(maxsize=None)
def scaled():
    """(name, tables, group_start, expects_vectors) as everywhere; ``scale_of(name)`` gives a twin's factor and
    ``twin_of(name)`` its unscaled node."""
    out = []
    for n in (30, 100):
        base = generic_tables(40000 + n, n, 9, "branch")
        out.append((f"scaled-n{n}-base", base, None, True))
        for sc in SCALES:
            twin = dataclasses.replace(base, tree_w=base.tree_w * sc)
            out.append((f"scaled-n{n}-x{sc:g}", twin, None, True))
    graded = _graded_tables(30)
    out.append(("scaled-graded-lengths-n30", graded, None, vectors_defined(oracle_w(graded, None))))
    return out


def scale_of(name: str) -> float:
    return float(name.rsplit("-x", 1)[1]) if "-x" in name else 1.0


def twin_of(name: str) -> str | None:
    return name.rsplit("-x", 1)[0] + "-base" if "-x" in name else None


def family(name: str):
    return globals()[name]()


# ---------------------------------------------------------------------------------------------------------------
# closed forms of the degenerate cases
# ---------------------------------------------------------------------------------------------------------------
def closed_form_error(name: str, w: np.ndarray, maps: np.ndarray, lam: np.ndarray) -> float:
    """What IS defined of a node whose eigenvectors are not, as the largest deviation (to be held to FIEDLER_TOL for
    vectors; eigenvalues are held to LAMBDA_BAR by ``check_node`` already and here once more in closed form)."""
    v = w.shape[0]
    if not (np.all(np.isfinite(maps)) and np.all(np.isfinite(lam))):
        return float("inf")
    s, dd = reference(w)
    dd64 = dd.astype(np.float64)
    x = np.asarray(maps, dtype=np.float64) * dd64[:, None]
    if name.startswith("two_vertices"):
        omega = float(w[0, 1])
        want = (1 / np.sqrt(2.0)) / np.sqrt(omega)
        err = max(abs(lam[0] - 1), abs(lam[1] + 1), abs(lam[2]), float(np.max(np.abs(maps[:, 0] - want)) / want),
                  float(np.max(np.abs(np.abs(maps[:, 1]) - want)) / want))
        return float("inf") if maps[0, 1] * maps[1, 1] >= 0 else float(err)
    if name.startswith("complete"):
        rep = -1.0 / (v - 1)
        return float(max(abs(lam[0] - 1), abs(lam[1] - rep), abs(lam[2] - rep),
                         np.max(np.abs(x[:, 0] - 1 / np.sqrt(v)))))
    if name.startswith("sizes") and not w.any():
        return float(np.max(np.abs(lam)))  # S = 0: every vector is an eigenvector, every eigenvalue 0
    if name.startswith(("two_components", "sizes")):
        # lambda_1 = lambda_2 = 1: the span of the two columns is the span of sqrt(d) restricted to the components
        comps = _components(w)
        big = sorted(set(comps), key=lambda c: -np.sum(comps == c))[:2]
        basis = np.stack([np.where(comps == c, dd64, 0.0) for c in big], axis=1)
        basis /= np.linalg.norm(basis, axis=0)
        return float(max(abs(lam[0] - 1), abs(lam[1] - 1), np.max(np.abs(x - basis @ (basis.T @ x)))))
    raise AssertionError(f"no closed form for {name}: the node is not one of the degenerate kinds")


def _components(w: np.ndarray) -> np.ndarray:
    v = w.shape[0]
    label = np.arange(v)
    for _ in range(v):
        new = label.copy()
        for i in range(v):
            nb = np.flatnonzero(w[i])
            if len(nb):
                new[i] = min(label[i], label[nb].min())
        if np.array_equal(new, label):
            break
        label = new
    return label
