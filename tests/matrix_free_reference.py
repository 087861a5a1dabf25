"""Host references, the error budget, a model of the walk and the cases for the matrix-free operator
(``csrc/scs_matfree.h``: ``k_mf_maxdepth``, ``k_mf_chunk``, ``k_mf_carry``, ``k_mf_reduce``; set up by
``scs_graph_matrix_free`` / ``scs_matfree_apply`` in ``csrc/scs_eig.hip``).  CPU only, numpy only; a helper module:
pytest collects nothing here.  The cases are run by ``tests/test_gpu_matrix_free_edges.py`` and held to the numbers
they are named for by ``tests/test_matrix_free_reference_cpu.py``.

* ``w_reference``: the dense W by the definition in the header of ``scs_matfree.h``, pair by pair.
* ``apply_reference``: ``dinv (.) W (dinv (.) x)`` in ``np.longdouble``.
* ``budget``: the rounding budget of the walk, PER TREE (derivation in its docstring).
* ``walk_profile`` / ``plan_reference``: what every (tree, direction, chunk) does, read off ``adj_depth`` alone.
* ``discrimination``: how far a single misplaced leaf moves the reference, in budgets.
* shapes the build's cases lack (root polytomies, the other caterpillar, a unary chain, a zigzag of spines whose
  stack entries come back from the global strip, mirror images) and the cases.
"""

from __future__ import annotations

import numpy as np

import build_reference as br
from solver_reference import LD, U, _row_chunks, apply_vectors, require_extended_precision

LDS_LEVELS = 32  # MF_LDS_LEVELS: entries below the top that live in LDS; the next one goes to the strip
MAX_CHUNKS = 16
CHUNK_LEAVES = 256
DENSE2_MAX = 128  # scs_graph_matrix_free wants more taxa than this


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def _tree(tables, t: int):
    lo, hi = int(tables.tree_off[t]), int(tables.tree_off[t + 1])
    return (tables.leaf_taxon[lo:hi], tables.adj_depth[lo:hi - 1] if hi > lo else tables.adj_depth[lo:lo],
            tables.adj_val[lo:hi - 1] if hi > lo else tables.adj_val[lo:lo], float(tables.tree_w[t]))


def w_reference(tables) -> np.ndarray:
    """W (n x n, ``np.longdouble``): for the leaves at DFS positions p < q of tree t, with the LEFTMOST shallowest
    separator of adj_depth[p .. q - 1] at depth d > 0, ``double(adj_val * tree_w)`` is added to W[a][b] and W[b][a]
    (one rounded multiply, as the library and the oracle form it; a separator of depth 0 is the root and adds
    nothing).  The sum over the trees is taken in extended precision: the oracle's differs by its double roundings."""
    require_extended_precision()
    n = tables.n_taxa
    w = np.zeros((n, n), dtype=LD)
    for t in range(tables.n_trees):
        tax, dep, val, wt = _tree(tables, t)
        nl = len(tax)
        at = np.arange(max(nl - 1, 0))
        for p in range(nl - 1):
            d = dep[p:]
            m = np.minimum.accumulate(d)
            first = np.ones(len(d), dtype=bool)
            first[1:] = m[1:] < m[:-1]  # a strictly shallower separator: the LCA moves up
            idx = np.maximum.accumulate(np.where(first, at[: len(d)], 0))
            v = np.where(m > 0, val[p:][idx] * wt, 0.0).astype(LD)
            w[tax[p], tax[p + 1:]] += v
            w[tax[p + 1:], tax[p]] += v
    return w


def dinv_of(deg: np.ndarray) -> np.ndarray:
    """d^-1/2 as the library defines it (``k_dinv``): 1 where the degree is 0.  In extended precision from the
    degrees given (the device's own, in the GPU test: the operator is then held apart from the degrees)."""
    deg = np.asarray(deg).astype(LD)
    out = np.ones_like(deg)
    pos = deg != 0
    out[pos] = 1 / np.sqrt(deg[pos])
    return out


def apply_reference(w: np.ndarray, x: np.ndarray, dinv: np.ndarray | None = None) -> np.ndarray:
    """``dinv (.) (W (dinv (.) x))`` in extended precision; ``dinv=None``: W x (the degrees, for x = 1)."""
    require_extended_precision()
    n = w.shape[0]
    z = x.astype(LD) if dinv is None else dinv[:, None] * x.astype(LD)
    ref = np.empty(z.shape, dtype=LD)
    for r0, r1 in _row_chunks(n, n):
        ref[r0:r1] = w[r0:r1] @ z
    return ref if dinv is None else ref * dinv[:, None]


def tree_scales(tables) -> np.ndarray:
    """Per tree ``w_t * max |adj_val| over its separators of depth > 0`` (0 for a tree without one)."""
    out = np.zeros(tables.n_trees, dtype=LD)
    for t in range(tables.n_trees):
        _, dep, val, wt = _tree(tables, t)
        inner = dep > 0
        if inner.any():
            out[t] = abs(LD(wt)) * LD(np.abs(val[inner]).max())
    return out


def budget(tables, x: np.ndarray, dinv: np.ndarray | None = None) -> np.ndarray:
    """The rounding budget of ``dinv (.) W (dinv (.) x)`` as the walk computes it, per entry (a, k):

        budget[a][k] = dinv_a * U * sum over the trees t that hold a of (4 L_t + 2 M + 16) * T_t[k],
        T_t[k] = w_t * max |adj_val over the separators of depth > 0 of t| * sum_{q in t} |z_q[k]|,  z = dinv (.) x,

    with L_t the tree's leaves, M the number of trees, U = 2^-53.  It is built per TREE, not per entry: a walk keeps
    one running ``total`` per thread and the rounding a large group leaves behind when it is taken off the stack
    stays in ``total`` for every later leaf of the tree, however small that leaf's own sum is.  |W||z| of the row is
    therefore no bound of this algorithm; the tree's largest magnitude T_t is (every value times every partial sum
    of z the walk forms is at most T_t in magnitude, and so is every value of ``total``, up to 1 + O(L U)).

    Derivation, for one tree, counting roundings of relative size U on quantities of magnitude at most T_t
    (Z = sum |z_q| over the tree, v the values; T_t = max |v| * Z):

    * The values: ``v = adj_val * tree_w`` is one rounded multiply in the kernel AND in the reference: no term.
    * A walk over n leaves (k_mf_chunk).  A group's sum s is a sum of z in some order: its error is at most
      (leaves of the group - 1) U Z_group, for ANY order (Higham, section 4.2).  ``total += v s`` at the push and
      ``total -= v ts`` at the pop use the same rounded s, so a group that has left the stack leaves no error of
      its sum behind, only the two roundings of the fused multiply-adds: at most 2 n U T_t after n leaves.  The
      groups still on the stack carry sum_g |v_g| (leaves of g) U Z_g <= n U T_t.  Together 3 n U T_t.
    * The stack S0 a chunk starts from (k_mf_carry, read by step C).  PS[j] is a sum of the z of at most n0 leaves
      in front of the chunk, by the walks' adds, the carry's ``extra`` adds and the prefix adds -- again some order of
      a sum: n0 U Z each, for PS_all and for PS[j]; their difference rounds once more; times the value: (2 n0 + 1) U
      T_t.  PA[j] = sum v_i s_i by fused multiply-adds: the sums' errors n0 U T_t, the roundings at most n0 U T_t.
      The output ``total + fma(vmin, PS_all - PS[j], PA[j])`` rounds twice more.  Together (4 n0 + 3) U T_t.
    * A leaf at position p: the walk from the left has n + n0 = p leaves behind it, the walk from the right
      L - 1 - p.  Both directions together: at most (4 (L - 1) + 6) U T_t <= (4 L + 2) U T_t.
    * k_mf_reduce adds the 2 M slabs of a taxon in order: 2 M roundings of partial sums bounded by the sum of the
      T_t of the trees that hold the taxon (a slab of a tree that does not hold it is 0 and adds exactly).
    * The scalings: the device forms dinv = 1 / sqrt(deg) (two correctly rounded operations; 3 U allowed), z = dinv x
      (U) and the final dinv * y (U) with its own 3 U: 8 U relative to (|W_t| |z|)_a <= T_t.  The reference is
      rounded in extended precision: below U / 1000 a term.
    * Second-order terms: a factor 1 + O(L U), far inside the remaining slack.

    Sum: (4 L_t + 2) + 2 M + 8 <= 4 L_t + 2 M + 16.  The constant is the issue's starting form; the re-derivation
    found no operation it misses (it has 6 U to spare).  It is changed by argument from the arithmetic only."""
    require_extended_precision()
    n, m = tables.n_taxa, tables.n_trees
    z = np.abs(x.astype(LD) if dinv is None else dinv[:, None] * x.astype(LD))
    scale = tree_scales(tables)
    out = np.zeros(z.shape, dtype=LD)
    for t in range(m):
        tax = _tree(tables, t)[0]
        tt = scale[t] * z[tax].sum(axis=0)
        out[tax] += (4 * len(tax) + 2 * m + 16) * tt[None, :]
    out *= LD(U)
    return out if dinv is None else out * dinv[:, None]


# ---------------------------------------------------------------------------------------------------------------
# the plan and the walk, from adj_depth alone
# ---------------------------------------------------------------------------------------------------------------
def plan_reference(tables) -> dict:
    """``chunks``, per tree the deepest separator (``maxd``; a tree's last slot holds none) and ``stack_total`` =
    sum (maxd + 1), as ``scs_graph_matrix_free`` plans them."""
    counts = np.diff(tables.tree_off)
    max_leaves = int(counts.max()) if len(counts) else 0
    maxd = np.zeros(tables.n_trees, dtype=np.int32)
    for t in range(tables.n_trees):
        dep = _tree(tables, t)[1]
        if len(dep):
            maxd[t] = max(0, int(dep.max()))
    return {"chunks": max(1, min(MAX_CHUNKS, max_leaves // CHUNK_LEAVES)), "maxd": maxd,
            "stack_total": int(maxd.astype(np.int64).sum() + tables.n_trees)}


def walk_profile(tables, chunks: int) -> dict:
    """What each (tree, direction, chunk) does, as arrays [n_trees][2][chunks] (direction 0 walks from the left):

    ``empty``    the chunk holds no leaf (the early return);
    ``leaves``   leaves of the chunk;
    ``entries``  most stack entries at once in step A, the top in registers included (entry 34 is the first one in
                 the global strip: 1 in registers + 32 in LDS before it);
    ``strip_reads`` pops of step A that bring an entry back from the global strip (34 or more entries before the pop);
    ``summary``  entries of the summary step A leaves;
    ``root``     step A met a root separator (depth 0);
    ``root_last`` the separator behind the chunk's last leaf is the root;
    ``s0``       entries of the stack S0 the carry hands to step C."""
    m = tables.n_trees
    shape = (m, 2, chunks)
    out = {k: np.zeros(shape, dtype=np.int64) for k in ("leaves", "entries", "strip_reads", "summary", "s0")}
    out.update({k: np.zeros(shape, dtype=bool) for k in ("empty", "root", "root_last")})
    for t in range(m):
        dep = _tree(tables, t)[1]
        nl = int(tables.tree_off[t + 1] - tables.tree_off[t])
        cl = (nl + chunks - 1) // chunks
        for direction in (0, 1):
            seps = dep if direction == 0 else dep[::-1]  # separator i sits behind leaf i of the walk
            running: list[int] = []  # the carry's stack, depths only
            for c in range(chunks):
                i0, i1 = c * cl, min(nl, c * cl + cl)
                if i0 >= nl:
                    out["empty"][t, direction, c] = True
                    out["s0"][t, direction, c] = 0  # (step C never reads it)
                    continue
                out["leaves"][t, direction, c] = i1 - i0
                stack: list[int] = []
                most, root, reads = 0, False, 0
                for i in range(i0, min(i1, nl - 1)):
                    d = int(seps[i])
                    while stack and stack[-1] >= d:
                        reads += len(stack) >= LDS_LEVELS + 2
                        stack.pop()
                    if d > 0:
                        stack.append(d)
                        most = max(most, len(stack))
                    else:
                        root = True
                out["entries"][t, direction, c] = most
                out["strip_reads"][t, direction, c] = reads
                out["summary"][t, direction, c] = len(stack)
                out["root"][t, direction, c] = root
                out["root_last"][t, direction, c] = i1 - 1 < nl - 1 and int(seps[i1 - 1]) == 0
                out["s0"][t, direction, c] = len(running)
                if root:
                    running = []
                if stack:
                    while running and running[-1] >= stack[0]:
                        running.pop()
                    running.extend(stack)
    return out


# ---------------------------------------------------------------------------------------------------------------
# discrimination: a single misplaced leaf against the budget
# ---------------------------------------------------------------------------------------------------------------
def discrimination(tables, x: np.ndarray, dinv: np.ndarray | None, bud: np.ndarray):
    """For every leaf p of every tree of weight != 0 and each of the moves

    * up: p leaves its parent for its grandparent -- the pairs (p, q), q in the parent's other leaves, take the
      value of the next shallower node (0 when that is the root or nothing is above);
    * down: p joins the child clade next to it under its parent -- the pairs (p, q), q in that clade, take the
      clade's value --

    the change of ``dinv (.) W (dinv (.) x)`` is measured in two of the entries it touches, row p and the row of the
    nearest leaf q of the range, as the largest ratio |change| / budget over the columns.  Returns ``(least ratio
    over all moves, moves, exempt)``; ``exempt`` counts the moves between two nodes of EQUAL value, which would change
    nothing (none in the cases: the zero-length node of `weights` has no leaf of its own)."""
    z = x.astype(LD) if dinv is None else dinv[:, None] * x.astype(LD)
    dl = np.ones(tables.n_taxa, dtype=LD) if dinv is None else dinv
    least, moves, exempt = np.inf, 0, 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(tables.n_trees):
            tax, dep, val, wt = _tree(tables, t)
            nl = len(tax)
            if wt == 0.0 or nl < 2:
                continue
            zt = z[tax]
            pre = np.concatenate([np.zeros((1, z.shape[1]), dtype=LD), np.cumsum(zt, axis=0)])
            bt, dt = bud[tax], dl[tax]

            def sep(i):  # depth of separator i, -1 outside the tree
                return int(dep[i]) if 0 <= i < nl - 1 else -1

            def effect(p, lo, hi, dv):  # the pairs (p, q), q in [lo, hi] \ {p}, change by dv
                nonlocal least, moves, exempt
                moves += 1
                if dv == 0.0:
                    exempt += 1
                    return
                others = pre[hi + 1] - pre[lo] - (zt[p] if lo <= p <= hi else 0)
                q = p + 1 if (p + 1 <= hi and p + 1 >= lo) else (p - 1 if lo <= p - 1 else (lo if lo > p else hi))
                r = max(float(np.max(np.abs(dt[p] * dv * others) / bt[p])),
                        float(np.max(np.abs(dt[q] * dv * zt[p]) / bt[q])))
                least = min(least, r)

            ns = nl - 1
            # per separator j: the nearest separator on each side that is shallower (lt_*) / no deeper (le_*)
            lt_l, lt_r = np.full(ns, -1), np.full(ns, ns)
            le_l, le_r = np.full(ns, -1), np.full(ns, ns)
            st: list[int] = []
            for j in range(ns):
                while st and dep[st[-1]] > dep[j]:
                    lt_r[st.pop()] = j
                st.append(j)
            st = []
            for j in range(ns):
                while st and dep[st[-1]] >= dep[j]:
                    le_r[st.pop()] = j
                st.append(j)
            st = []
            for j in range(ns - 1, -1, -1):
                while st and dep[st[-1]] > dep[j]:
                    lt_l[st.pop()] = j
                st.append(j)
            st = []
            for j in range(ns - 1, -1, -1):
                while st and dep[st[-1]] >= dep[j]:
                    le_l[st.pop()] = j
                st.append(j)
            for p in range(nl):
                a, b = sep(p - 1), sep(p)
                dp = max(a, b)
                j = p - 1 if a == dp else p  # the separator at the parent's depth next to p
                vp = 0.0 if dp <= 0 else float(val[j]) * wt
                if dp > 0:  # up: the leaves under p's parent are those between the shallower separators around j
                    jl, jr = int(lt_l[j]), int(lt_r[j])
                    da, db = sep(jl), sep(jr)
                    d2 = max(da, db)
                    v2 = 0.0 if d2 <= 0 else float(val[jl] if da == d2 else val[jr]) * wt
                    effect(p, jl + 1, jr, v2 - vp)
                for side in (-1, 1):  # down: the child clade of the parent on this side, if it is a clade
                    first = p - 1 if side < 0 else p  # the separator between p and that clade
                    if not 0 <= first < ns or int(dep[first]) != dp:
                        continue
                    e = int(le_l[first]) if side < 0 else int(le_r[first])  # where the clade ends
                    inner = dep[e + 1:first] if side < 0 else dep[first + 1:e]
                    if len(inner) == 0:
                        continue  # a single leaf next to p: nothing below to join
                    best = (e + 1 if side < 0 else first + 1) + int(np.argmin(inner))
                    clo, chi = (e + 1, p - 1) if side < 0 else (p + 1, e)
                    effect(p, clo, chi, float(val[best]) * wt - vp)
    return least, moves, exempt


# ---------------------------------------------------------------------------------------------------------------
# shapes (preorder ``(parent, is_leaf)``, as ``build_reference.shape`` returns them)
# ---------------------------------------------------------------------------------------------------------------
def caterpillar_shallow_first(k: int):
    """The other orientation of ``shape("caterpillar", k)``: the leaves come shallowest first, the separators read
    0, 1, ..., k - 2 -- a walk from the left stacks k - 2 entries, one from the right a single one."""
    assert k >= 2
    parent, leaf, at = [-1], [False], 0
    for _ in range(k - 2):
        parent += [at, at]
        leaf += [True, False]
        at = len(parent) - 1
    parent += [at, at]
    leaf += [True, True]
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def root_polytomy(parts):
    """The root with one child per part, in order: a ``(parent, is_leaf)`` subtree, or 1 for a single leaf.  Every
    separator between two parts is a root separator."""
    parent, leaf = [-1], [False]
    for part in parts:
        base = len(parent)
        if isinstance(part, int):
            assert part == 1
            parent.append(0)
            leaf.append(True)
            continue
        par, lf = part
        parent += [0 if q < 0 else int(q) + base for q in par]
        leaf += [bool(v) for v in lf]
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def unary_chain(length: int, clade):
    """The root with two children: a chain of ``length`` one-child nodes that ends in ``clade``, then one leaf.  The
    separators inside the clade lie ``length + 1`` levels deeper than the clade's own: depth far beyond the number
    of stack entries."""
    par, lf = clade
    chain = np.arange(length, dtype=np.int64)  # node i + 1 hangs off node i
    base = length + 1
    parent = np.concatenate([[-1], chain, np.where(par < 0, length, par + base), [0]])
    leaf = np.concatenate([np.zeros(length + 1, dtype=bool), lf, [True]])
    return parent.astype(np.int32), leaf


def zigzag(k: int, extras: dict):
    """``caterpillar_shallow_first(k)`` whose spine node of depth j has a third child ``extras[j]`` behind the spine:
    the separators read 0, 1, ..., k - 2 down the spine, then -- deepest j first -- j and the separators of
    ``extras[j]`` shifted by j + 1.  A walk from the left stacks k - 2 entries, takes the ones from j on OFF again
    (through the global strip when there are more than 33) and goes on: the popped values show in every later leaf."""
    assert k >= 3 and all(0 <= j <= k - 2 for j in extras)
    parent, leaf, spine = [-1], [False], [0]
    for _ in range(k - 2):
        parent += [spine[-1], spine[-1]]
        leaf += [True, False]
        spine.append(len(parent) - 1)
    parent += [spine[-1], spine[-1]]
    leaf += [True, True]
    for j in sorted(extras, reverse=True):
        par, lf = extras[j]
        base = len(parent)
        parent += [spine[j] if q < 0 else int(q) + base for q in par]
        leaf += [bool(v) for v in lf]
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def mirror(sh):
    """The same tree with the children of every node in reverse order: what a walk from the left meets in ``sh``, a
    walk from the right meets here."""
    par, lf = sh
    kids: list[list[int]] = [[] for _ in par]
    for i in range(1, len(par)):
        kids[par[i]].append(i)
    parent, leaf, todo = [], [], [(0, -1)]
    while todo:
        i, p = todo.pop()
        parent.append(p)
        leaf.append(bool(lf[i]))
        todo.extend((c, len(parent) - 1) for c in kids[i])  # (popped last first: the children come out reversed)
    return np.asarray(parent, dtype=np.int32), np.asarray(leaf, dtype=bool)


def leaves_of(sh) -> int:
    return int(np.count_nonzero(sh[1]))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
STACK_LEAVES = (33, 34, 35, 36, 40)  # caterpillars: 31, 32, 33 (LDS full), 34 (one in the strip) and 38 entries
CHUNK_SIZES = {511: 1, 512: 2, 513: 2, 767: 2, 768: 3, 4095: 15, 4096: 16, 4097: 16}
MIXED_SIZES = (1, 2, 3, 15, 16, 17, 241, 255, 256, 257)
CHAIN_DEPTH = 70000
WHOLE_MATRIX_MAX = 640  # up to here the unit vectors recover all of W


def _ids(rng, n, k, pool=None):
    return br.order_random(rng, np.arange(n, dtype=np.int32) if pool is None else pool, k)


def _rand(rng, k):
    return br.shape("random", k, rng)


def case(name: str):
    """``(TreeArrays, strategy)`` of a case.  Strategies ``branch`` (positive random lengths) and ``depth``, every
    tree its own weight: the values differ from node to node, which is what lets a misplaced leaf show."""
    kind, _, arg = name.partition("_")
    rng = np.random.RandomState(sum(map(ord, name)))
    if kind == "zigzag":  # entries that went to the strip come BACK and are used: one chunk (42) and two (300)
        k = int(arg)
        if k == 42:
            n = 200
            sh = zigzag(42, {20: caterpillar_shallow_first(30), 5: caterpillar_shallow_first(30), 1: _rand(rng, 10)})
        else:
            n = 640
            sh = zigzag(300, {150: caterpillar_shallow_first(200), 40: caterpillar_shallow_first(100)})
        trees = [(sh, _ids(rng, n, leaves_of(sh))), (mirror(sh), _ids(rng, n, leaves_of(sh))),
                 ("random", _ids(rng, n, n // 2))]
        return br.forest(k, n, trees), ("depth" if k == 42 else "branch")
    if kind == "stack":  # one chunk; both caterpillars of k leaves beside small random trees
        k, n = int(arg), 160
        trees = [("caterpillar", _ids(rng, n, k)), (caterpillar_shallow_first(k), _ids(rng, n, k)),
                 ("random", _ids(rng, n, 140)), ("random", _ids(rng, n, 50))]
        return br.forest(k, n, trees), ("branch" if k % 2 else "depth")
    if kind == "deep":  # summaries and S0 of hundreds of entries
        k = int(arg)
        if k == 600:
            n = 640
            trees = [("caterpillar", _ids(rng, n, 600)), (caterpillar_shallow_first(600), _ids(rng, n, 600)),
                     ("random", _ids(rng, n, 300))]
        else:
            n = k + 100
            trees = [("caterpillar", _ids(rng, n, k)), (caterpillar_shallow_first(2000), _ids(rng, n, 2000)),
                     ("random", _ids(rng, n, 1000)), ("random", _ids(rng, n, 17))]
        return br.forest(k, n, trees), "depth"
    if kind == "chunks":  # the largest tree decides the chunk count
        k = int(arg)
        n = k + 5
        trees = [("random", _ids(rng, n, k)), ("balanced", _ids(rng, n, k // 2)), ("random", _ids(rng, n, 100))]
        return br.forest(k, n, trees), "branch"
    if name == "mixed":  # 16 chunks over trees of 1 ... 257 leaves; taxon `lone` is in no tree
        n = 4300
        pool = np.setdiff1d(np.arange(n, dtype=np.int32), [MIXED_LONE])
        trees = [("random", _ids(rng, n, k, pool)) for k in MIXED_SIZES[:5]] + [("random", _ids(rng, n, 4096, pool))] + \
                [("random", _ids(rng, n, k, pool)) for k in MIXED_SIZES[5:]]
        return br.forest(7, n, trees), "branch"
    if name == "root_leaves":  # every separator of tree 0 is the root
        n = 150
        trees = [(root_polytomy([1] * 140), _ids(rng, n, 140)), ("random", _ids(rng, n, 150)), ("random", _ids(rng, n, 60))]
        return br.forest(11, n, trees), "branch"
    if name == "root_clades":  # root polytomies of subtrees, one chunk
        n = 200
        a = root_polytomy([_rand(rng, 40), 1, _rand(rng, 2), caterpillar_shallow_first(36), 1, 1, _rand(rng, 60)])
        b = root_polytomy([br.shape("caterpillar", 37), _rand(rng, 3), br.shape("caterpillar", 37)])
        trees = [(a, _ids(rng, n, leaves_of(a))), (b, _ids(rng, n, leaves_of(b))), ("random", _ids(rng, n, 190))]
        return br.forest(12, n, trees), "depth"
    if name == "root_edges":  # 1024 leaves, 4 chunks of 256: root separators at and around the chunk edges
        n = 1100
        a = root_polytomy([_rand(rng, k) for k in ROOT_EDGE_PARTS])
        b = root_polytomy([_rand(rng, 256)] + [1] * 256 + [_rand(rng, 512)])
        trees = [(a, _ids(rng, n, 1024)), (b, _ids(rng, n, 1024)), ("random", _ids(rng, n, 600))]
        return br.forest(13, n, trees), "branch"
    if name == "maxdepth":  # what k_mf_maxdepth's 64-slot pieces can meet
        n = 200
        trees = [("random", _ids(rng, n, 1)) for _ in range(200)]
        trees += [("random", _ids(rng, n, k)) for k in (63, 64, 65)]
        trees += [("caterpillar", _ids(rng, n, 30)), (caterpillar_shallow_first(30), _ids(rng, n, 30))]
        used = 200 + 63 + 64 + 65 + 60
        pad = (60 - used) % 64 or 64  # the next tree starts at slot 60 of a piece
        trees.append(("random", _ids(rng, n, pad)))
        before = root_polytomy([caterpillar_shallow_first(5), br.shape("balanced", 4)])  # deepest: slot 63
        after = root_polytomy([1] * 57 + [caterpillar_shallow_first(4)] + [1] * 3)  # deepest: slot 128 = 69 + 59
        trees += [(before, _ids(rng, n, 9)), (after, _ids(rng, n, 64))]
        chain = unary_chain(CHAIN_DEPTH, _rand(rng, 19))
        trees.append((chain, _ids(rng, n, 20)))
        return br.forest(14, n, trees), "depth"
    if name == "widths":  # partial coverage: most entries of a slab belong to taxa the tree does not hold
        n = 300
        trees = [("random", _ids(rng, n, k)) for k in (150, 40, 299, 7, 120)] + [("caterpillar", _ids(rng, n, 45))]
        return br.forest(15, n, trees), "branch"
    if name in ("weights", "weights_depth"):  # a tree of weight 0; a separator of value 0 at depth 1
        n = 180
        trees = [("random", _ids(rng, n, 170)), ("random", _ids(rng, n, 90)), ("balanced", _ids(rng, n, 64)),
                 ("caterpillar", _ids(rng, n, 50))]
        arrays = br.forest(16, n, trees)
        arrays.weights[1] = 0.0
        # tree 2 (balanced): its root's first child gets length 0 -- under `branch` its value is 0 at depth 1
        arrays.length[int(arrays.node_off[2]) + 1] = 0.0
        return arrays, ("depth" if name.endswith("depth") else "branch")
    raise ValueError(name)


MIXED_LONE = 2150
ROOT_EDGE_PARTS = (256, 255, 258, 255)  # root separators behind leaves 255 (a chunk's last), 510 and 768

CASES = tuple([f"stack_{k}" for k in STACK_LEAVES] + ["zigzag_42", "zigzag_300", "deep_600", "deep_4100"] + [f"chunks_{k}" for k in CHUNK_SIZES] +
              ["mixed", "root_leaves", "root_clades", "root_edges", "maxdepth", "widths", "weights", "weights_depth"])


def tables_of(name: str):
    arrays, strategy = case(name)
    return br.tables(arrays, strategy)


def probes(n: int, name: str) -> dict:
    """The dense probes of a case (``solver_reference.apply_vectors``): ``plain`` at width 8 and ``graded`` at width 4,
    and up to WHOLE_MATRIX_MAX taxa also ``graded`` at 8 and ``plain`` at 4 -- in this order the width changes with
    every application."""
    seed = sum(map(ord, name))
    out = {"plain8": apply_vectors(n, 8, seed), "graded4": apply_vectors(n, 4, seed + 1, graded=True)}
    if n <= WHOLE_MATRIX_MAX:
        out.update({"graded8": apply_vectors(n, 8, seed + 2, graded=True), "plain4": apply_vectors(n, 4, seed + 3)})
    return out


def unit_columns(tables, chunks: int) -> np.ndarray:
    """The columns of W the unit vectors recover: all of them up to WHOLE_MATRIX_MAX taxa, beyond that the taxa of
    every tree's first and last leaf, of the leaves either side of every chunk boundary and of every root separator,
    and of the leaves either side of every tree's deepest separator."""
    n = tables.n_taxa
    if n <= WHOLE_MATRIX_MAX:
        return np.arange(n, dtype=np.int32)
    pick: set[int] = set()
    for t in range(tables.n_trees):
        tax, dep, _, _ = _tree(tables, t)
        nl = len(tax)
        pos = {0, nl - 1}
        cl = (nl + chunks - 1) // chunks
        for c in range(1, chunks):
            for direction in (0, 1):
                for i in (c * cl - 1, c * cl):
                    if 0 <= i < nl:
                        pos.add(i if direction == 0 else nl - 1 - i)
        for i in np.flatnonzero(dep == 0)[:64]:
            pos.update((int(i), int(i) + 1))
        if len(dep):
            i = int(np.argmax(dep))
            pos.update((i, i + 1))
        pick.update(int(tax[i]) for i in pos)
    return np.asarray(sorted(pick), dtype=np.int32)
