"""``tests/matrix_free_reference.py`` held to itself, to the oracle and to the numbers its cases are named for; no
device.  What the GPU test (``tests/test_gpu_matrix_free_edges.py``) relies on is checked here:

* ``w_reference`` against ``oracle.tables_oracle.pcg_dense`` on every case, and against brute force over explicit
  leaf sets on small trees of every shape;
* every case reaches the path of ``csrc/scs_matfree.h`` it is named for (``walk_profile``, ``plan_reference``);
* the budget cannot hide a structural failure: a single leaf joined to the wrong node moves the reference by more
  than 100 budgets, in every case and under every probe."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import build_reference as br
import matrix_free_reference as mf
from oracle import tables_oracle as to
from solver_reference import LD, U, scaling

DISCRIMINATION = 100.0


@functools.lru_cache(maxsize=None)
def _tables(name):
    return mf.tables_of(name)


@functools.lru_cache(maxsize=None)
def _profile(name):
    tb = _tables(name)
    plan = mf.plan_reference(tb)
    return plan, mf.walk_profile(tb, plan["chunks"])


def _leaves(tb, t):
    return int(tb.tree_off[t + 1] - tb.tree_off[t])


# ---------------------------------------------------------------------------------------------------------------
# the two references
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mf.CASES)
def test_w_reference_agrees_with_the_oracle(name):
    """Both add the same doubles ``adj_val * tree_w`` per pair; the oracle adds them in double precision in tree
    order, the reference in extended precision.  So they agree to the rounding of the oracle's M - 1 double adds of
    non-negative terms -- (M - 1) U W elementwise -- and EXACTLY wherever a single tree reaches the pair."""
    tb = _tables(name)
    assert tb.n_taxa > mf.DENSE2_MAX
    assert float(tb.adj_val.min()) >= 0.0 and float(tb.tree_w.min()) >= 0.0
    w = mf.w_reference(tb)
    w_o, _ = to.pcg_dense(tb)
    assert np.array_equal(w, w.T)
    assert not np.diagonal(w).any()
    err = np.abs(w - w_o.astype(LD))
    assert bool(np.all(err <= (tb.n_trees - 1) * LD(U) * w))
    member = np.zeros((tb.n_trees, tb.n_taxa), dtype=np.int64)
    for t in range(tb.n_trees):
        member[t, mf._tree(tb, t)[0]] = 1
    single = member.T @ member <= 1  # pairs at most one tree holds together
    assert bool(np.all(err[single] == 0))
    # the degrees of both give the same scaling, to the same rounding
    assert np.allclose(np.asarray(scaling(w_o), dtype=np.float64), np.asarray(mf.dinv_of(w.sum(axis=1)), dtype=np.float64),
                       rtol=1e-13, atol=0)


def _brute_force(arrays, strategy):
    """W from explicit leaf sets: for every inner node but the root, every pair of leaves from two DIFFERENT
    children gets the node's value (its depth, or the sum of the lengths down to it) times the tree's weight."""
    n = arrays.n_taxa
    w = np.zeros((n, n), dtype=LD)
    for t in range(arrays.n_trees):
        lo, hi = int(arrays.node_off[t]), int(arrays.node_off[t + 1])
        par, tax, length = arrays.parent[lo:hi], arrays.taxon[lo:hi], arrays.length[lo:hi]
        k = hi - lo
        value = np.zeros(k)
        for i in range(1, k):
            value[i] = value[par[i]] + (1.0 if strategy == "depth" else float(length[i]))
        below = [set() for _ in range(k)]
        for i in range(k - 1, -1, -1):
            if tax[i] >= 0:
                below[i].add(int(tax[i]))
            if i:
                below[par[i]] |= below[i]
        for i in range(1, k):
            kids = [c for c in range(i + 1, k) if par[c] == i]
            for x in range(len(kids)):
                for y in range(x + 1, len(kids)):
                    for a in below[kids[x]]:
                        for b in below[kids[y]]:
                            v = LD(value[i] * float(arrays.weights[t]))
                            w[a, b] += v
                            w[b, a] += v
    return w


@pytest.mark.parametrize("strategy", ["depth", "branch"])
def test_w_reference_agrees_with_brute_force_over_leaf_sets(strategy):
    rng = np.random.RandomState(5)
    n = 14
    shapes = [br.shape("random", 12, rng), br.shape("caterpillar", 9), mf.caterpillar_shallow_first(9),
              mf.root_polytomy([1, 1, 1, 1, 1]), mf.root_polytomy([br.shape("random", 4, rng), 1, br.shape("balanced", 3), 1]),
              mf.unary_chain(7, br.shape("random", 5, rng)), br.shape("star", 8), br.shape("random", 1, rng), br.shape("random", 2, rng),
              mf.root_polytomy([mf.unary_chain(3, mf.caterpillar_shallow_first(3)), br.shape("caterpillar", 4)])]
    trees = [(sh, br.order_random(rng, np.arange(n, dtype=np.int32), mf.leaves_of(sh))) for sh in shapes]
    arrays = br.forest(3, n, trees)
    tb = br.tables(arrays, strategy)
    got, want = mf.w_reference(tb), _brute_force(arrays, strategy)
    # (the same doubles added in extended precision in another order: a few units of 2^-64)
    assert bool(np.all(np.abs(got - want) <= 2.0 ** -60 * np.abs(want)))
    assert float(np.abs(want).max()) > 0


def test_budget_is_per_tree_and_scales_with_the_operand():
    tb = _tables("widths")
    x = mf.probes(tb.n_taxa, "widths")["graded4"]
    dinv = mf.dinv_of(mf.w_reference(tb).sum(axis=1))
    b = mf.budget(tb, x, dinv)
    assert b.shape == x.shape and bool(np.all(b > 0))
    assert np.allclose(np.asarray(mf.budget(tb, 3.0 * x, dinv) / b, dtype=np.float64), 3.0)
    # by hand for one entry: taxon a, column 2
    a = int(mf._tree(tb, 3)[0][0])
    z = np.abs(dinv[:, None] * x.astype(LD))
    want = LD(0)
    for t in range(tb.n_trees):
        tax, dep, val, wt = mf._tree(tb, t)
        if a in tax:
            want += (4 * len(tax) + 2 * tb.n_trees + 16) * LD(wt) * LD(val[dep > 0].max()) * z[tax, 2].sum()
    assert abs(float(b[a, 2] / (dinv[a] * LD(U) * want)) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------------
# every case sits on the path it is named for
# ---------------------------------------------------------------------------------------------------------------
def test_plan_reference_by_hand():
    tb = _tables("stack_36")
    plan = mf.plan_reference(tb)
    assert plan["chunks"] == 1 and list(plan["maxd"][:2]) == [34, 34]
    assert plan["stack_total"] == int(plan["maxd"].sum()) + tb.n_trees
    for t in range(tb.n_trees):
        lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1])
        assert plan["maxd"][t] == max(int(d) for d in tb.adj_depth[lo:hi - 1])


@pytest.mark.parametrize("k", mf.STACK_LEAVES)
def test_stack_cases_sit_on_the_edge_of_the_lds_levels(k):
    """A caterpillar of k leaves stacks k - 2 entries in the walk that meets its separators shallowest first: 31 and
    32 (inside the LDS levels), 33 (the top and all 32 LDS levels: full, none in the strip), 34 (one in the strip),
    38 (five in the strip).  The opposite walk keeps a single entry."""
    plan, prof = _profile(f"stack_{k}")
    assert plan["chunks"] == 1
    ent = prof["entries"][:, :, 0]
    assert ent[0, 1] == k - 2 and ent[0, 0] == 1  # deepest leaves first: the walk from the right stacks
    assert ent[1, 0] == k - 2 and ent[1, 1] == 1  # shallowest first: the walk from the left
    in_strip = max(0, k - 2 - (mf.LDS_LEVELS + 1))
    assert in_strip == {33: 0, 34: 0, 35: 0, 36: 1, 40: 5}[k]
    assert prof["summary"][0, 1, 0] == k - 2  # the summary copies the strip's entries too (j >= 32)
    assert ent[2:].max() <= mf.LDS_LEVELS  # the random trees beside them stay in LDS
    assert not prof["strip_reads"].any()  # a caterpillar only stacks: what comes BACK from the strip is zigzag's to hold


def test_zigzag_cases_read_the_strip_back():
    """Down a spine (40 / 298 entries), back up to a node half way (the pops run through the strip: 7 / 265 of the
    entries taken off lie there), down the next spine, up again: what was read back is used by every later leaf."""
    plan, prof = _profile("zigzag_42")
    assert plan["chunks"] == 1
    # spine 1 .. 40; off down to 20, spine 21 .. 49; off down to 5, spine 6 .. 34; off down to 1
    assert prof["entries"][0, 0, 0] == 49 and prof["entries"][1, 1, 0] == 49
    assert prof["strip_reads"][0, 0, 0] == 7 + 16 + 1 == prof["strip_reads"][1, 1, 0]
    assert prof["entries"][0, 1, 0] <= 8 and not prof["strip_reads"][0, 1].any()  # the opposite walk stays shallow
    plan, prof = _profile("zigzag_300")
    assert plan["chunks"] == 2  # 600 leaves: chunk 0 is the spine of 300 and the separator (150) behind it
    assert list(prof["entries"][0, 0]) == [298, 199] and list(prof["summary"][0, 0]) == [150, 100]
    assert list(prof["strip_reads"][0, 0]) == [298 - 149, 166] and prof["s0"][0, 0, 1] == 150
    assert list(prof["strip_reads"][1, 1]) == list(prof["strip_reads"][0, 0])  # the mirror, from the right


def test_deep_cases_carry_hundreds_of_entries():
    plan, prof = _profile("deep_600")
    assert plan["chunks"] == 2
    # shallowest first, 600 leaves in 2 chunks of 300: the root separator, then depths 1 .. 299 | 300 .. 598
    assert list(prof["entries"][1, 0]) == [299, 299] and list(prof["summary"][1, 0]) == [299, 299]
    assert list(prof["s0"][1, 0]) == [0, 299] and list(prof["root"][1, 0]) == [True, False]
    assert list(prof["entries"][0, 1]) == [299, 299] and prof["s0"][0, 1, 1] == 299
    # deepest first from the left: every separator pops the one before it -- S0 is one entry, the summary too
    assert list(prof["entries"][0, 0]) == [1, 1] and prof["s0"][0, 0, 1] == 1
    plan, prof = _profile("deep_4100")
    tb = _tables("deep_4100")
    assert plan["chunks"] == 16 and _leaves(tb, 0) == 4100  # chunks of 257 leaves, the last of 245
    assert list(prof["leaves"][0, 1]) == [257] * 15 + [245]
    assert list(prof["entries"][0, 1]) == [256] + [257] * 14 + [244]
    assert list(prof["s0"][0, 1]) == [0] + [256 + 257 * c for c in range(15)]  # up to 3 854 entries
    assert list(prof["s0"][0, 0]) == [0] + [1] * 15
    assert _leaves(tb, 3) == 17  # 16 chunks of 2: eight full, one of one leaf, seven empty
    assert list(prof["leaves"][3, 0]) == [2] * 8 + [1] + [0] * 7 and list(prof["empty"][3, 1]) == [False] * 9 + [True] * 7


@pytest.mark.parametrize(("k", "chunks"), sorted(mf.CHUNK_SIZES.items()))
def test_chunk_cases_give_the_chunk_counts(k, chunks):
    tb = _tables(f"chunks_{k}")
    plan, prof = _profile(f"chunks_{k}")
    assert int(np.diff(tb.tree_off).max()) == k and plan["chunks"] == chunks
    assert prof["leaves"][0, 0].sum() == k and not prof["empty"][0].any()
    if chunks > 1:
        assert prof["s0"][0, :, 1:].min() >= 1  # the carry hands every later chunk of the largest tree something


def test_mixed_case_has_short_trees_empty_chunks_and_a_lone_taxon():
    tb = _tables("mixed")
    plan, prof = _profile("mixed")
    assert plan["chunks"] == 16
    sizes = [_leaves(tb, t) for t in range(tb.n_trees)]
    assert sizes == list(mf.MIXED_SIZES[:5]) + [4096] + list(mf.MIXED_SIZES[5:])
    by = {s: t for t, s in enumerate(sizes)}
    for direction in (0, 1):
        assert list(prof["empty"][by[1], direction]) == [False] + [True] * 15  # fewer leaves than chunks
        assert list(prof["leaves"][by[3], direction]) == [1, 1, 1] + [0] * 13
        assert list(prof["leaves"][by[15], direction]) == [1] * 15 + [0]
        assert list(prof["leaves"][by[17], direction]) == [2] * 8 + [1] + [0] * 7  # chunk 9 of the 17-leaf tree is empty
        assert bool(prof["empty"][by[17], direction, 9]) and not prof["empty"][by[17], direction, 8]
        assert list(prof["leaves"][by[241], direction]) == [16] * 15 + [1]  # a last chunk of one leaf
        assert list(prof["leaves"][by[255], direction]) == [16] * 15 + [15]
        assert list(prof["leaves"][by[256], direction]) == [16] * 16
        assert list(prof["leaves"][by[257], direction]) == [17] * 15 + [2]
        assert list(prof["leaves"][by[4096], direction]) == [256] * 16
    assert mf.MIXED_LONE not in set(tb.leaf_taxon.tolist())
    w = mf.w_reference(tb)
    assert not w[mf.MIXED_LONE].any() and not w[:, mf.MIXED_LONE].any()
    assert mf.dinv_of(w.sum(axis=1))[mf.MIXED_LONE] == 1


def test_root_cases_put_root_separators_where_they_are_named():
    tb = _tables("root_leaves")
    _, prof = _profile("root_leaves")
    assert _leaves(tb, 0) == 140 and not mf._tree(tb, 0)[1].any()  # every separator is the root
    assert prof["entries"][0].max() == 0 and prof["summary"][0].max() == 0 and prof["root"][0].all()

    tb = _tables("root_clades")
    plan, prof = _profile("root_clades")
    assert plan["chunks"] == 1
    assert int(np.count_nonzero(mf._tree(tb, 0)[1] == 0)) == 6 and int(np.count_nonzero(mf._tree(tb, 1)[1] == 0)) == 2
    # a caterpillar of 36 / 37 leaves under the root is one level deeper: 35 / 36 entries, two / three in the strip,
    # and the root separator behind it empties that stack (a pop run through the strip and all LDS levels)
    assert prof["entries"][0, 0, 0] == 35 and prof["entries"][1, 1, 0] == 36 and prof["entries"][1, 0, 0] <= 3

    tb = _tables("root_edges")
    plan, prof = _profile("root_edges")
    assert plan["chunks"] == 4 and _leaves(tb, 0) == 1024 and _leaves(tb, 1) == 1024  # chunks of 256 leaves
    dep = mf._tree(tb, 0)[1]
    assert list(np.flatnonzero(dep == 0)) == [255, 510, 768]
    # from the left: behind chunk 0's last leaf (255); one leaf before chunk 1's last (510: one separator follows it
    # in the chunk, so the summary has one entry); one after chunk 2's last (768: the first separator of chunk 3)
    assert list(prof["root_last"][0, 0]) == [True, False, False, False]
    assert list(prof["root"][0, 0]) == [True, True, False, True]
    assert prof["summary"][0, 0, 1] == 1 and prof["s0"][0, 0, 1] == 0 and prof["s0"][0, 0, 2] == 1
    assert prof["s0"][0, 0, 3] >= 1  # what chunk 3 starts from is dropped at its first separator
    # from the right the same separators sit at walk positions 1023 - 1 - q = 767 (chunk 2's last), 512, 254
    assert list(prof["root_last"][0, 1]) == [False, False, True, False]
    # tree 1: leaves 256 .. 511 hang off the root one by one -- a chunk made of root separators only
    dep = mf._tree(tb, 1)[1]
    assert not dep[255:512].any() and dep[:255].all() and dep[512:].all()
    for direction, c in ((0, 1), (1, 2)):
        assert prof["entries"][1, direction, c] == 0 and prof["summary"][1, direction, c] == 0
        assert prof["root"][1, direction, c] and prof["root_last"][1, direction, c]
        assert prof["s0"][1, direction, c + 1] == 0


def test_maxdepth_case_meets_what_a_64_slot_piece_can_meet():
    tb = _tables("maxdepth")
    plan = mf.plan_reference(tb)
    sizes = [_leaves(tb, t) for t in range(tb.n_trees)]
    assert sizes[:200] == [1] * 200 and not plan["maxd"][:200].any()  # a piece meets 64 tree boundaries
    assert sizes[200:203] == [63, 64, 65] and [int(tb.tree_off[t]) for t in (200, 201, 202)] == [200, 263, 327]
    cat, rev, before, after, chain = 203, 204, 206, 207, 208
    assert int(np.argmax(mf._tree(tb, cat)[1])) == 0  # the deepest separator is the tree's first ...
    assert int(np.argmax(mf._tree(tb, rev)[1])) == sizes[rev] - 2  # ... and its last
    for t, slot in ((before, 63), (after, 0)):  # the slot before a 64-slot boundary, and the one after
        dep = mf._tree(tb, t)[1]
        deepest = np.flatnonzero(dep == dep.max())
        assert len(deepest) == 1 and (int(tb.tree_off[t]) + int(deepest[0])) % 64 == slot
        assert int(tb.tree_off[t]) // 64 != (int(tb.tree_off[t + 1]) - 1) // 64  # the tree crosses the boundary
    assert sizes[chain] == 20 and plan["maxd"][chain] > mf.CHAIN_DEPTH
    prof = mf.walk_profile(tb, 1)
    assert prof["entries"][chain].max() <= 19  # depth 70 000, a stack of a few entries
    assert plan["stack_total"] == int(plan["maxd"].astype(np.int64).sum()) + tb.n_trees > mf.CHAIN_DEPTH


def test_widths_and_weights_cases():
    tb = _tables("widths")
    assert max(_leaves(tb, t) for t in range(tb.n_trees)) < tb.n_taxa  # partial coverage in every tree
    for name in ("weights", "weights_depth"):
        tb = _tables(name)
        assert tb.tree_w[1] == 0.0 and np.count_nonzero(tb.tree_w) == tb.n_trees - 1
    _, dep, val, _ = mf._tree(_tables("weights"), 2)
    assert bool(np.any((dep > 0) & (val == 0.0)))  # a separator of value 0 that is not the root
    _, dep, val, _ = mf._tree(_tables("weights_depth"), 2)
    assert bool(np.all(val[dep > 0] == dep[dep > 0]))  # `depth`: the value is the depth


# ---------------------------------------------------------------------------------------------------------------
# the budget cannot hide a misplaced leaf
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mf.CASES)
def test_a_misplaced_leaf_moves_the_reference_by_more_than_100_budgets(name):
    """Every leaf of every tree (of weight != 0), moved one level up or down: some entry of the product changes by
    more than 100 times its budget, under the vector of ones, under the unit vectors (of the leaf itself: the
    entries of W that change) and under each dense probe.  ``one`` would fail it by construction (every value ties);
    the cases use ``branch`` on positive random lengths and ``depth``, with a weight per tree."""
    tb = _tables(name)
    n = tb.n_taxa
    dinv = mf.dinv_of(mf.w_reference(tb).sum(axis=1))
    ones = np.ones((n, 1))
    least, moves, exempt = mf.discrimination(tb, ones, None, mf.budget(tb, ones, None))
    print(f"{name}: ones {least:.3g} ({moves} moves, {exempt} exempt)", end="")
    assert least > DISCRIMINATION and moves >= tb.n_leaves // 2
    assert exempt == 0
    for probe, x in mf.probes(n, name).items():
        least, _, _ = mf.discrimination(tb, x, dinv, mf.budget(tb, x, dinv))
        print(f", {probe} {least:.3g}", end="")
        assert least > DISCRIMINATION, probe
    # unit vectors: column q of the product is W[:, q] scaled; a move of leaf p changes W[p][q] for the q of the range,
    # by dv, against the budget of entry (p, q) -- which holds only the trees that hold q: at most all of them
    scale = mf.tree_scales(tb)
    worst_budget = LD(U) * sum((4 * _leaves(tb, t) + 2 * tb.n_trees + 16) * scale[t] for t in range(tb.n_trees))
    gaps = []
    for t in range(tb.n_trees):
        _, dep, val, wt = mf._tree(tb, t)
        if wt == 0.0:
            continue
        vals = np.unique(np.concatenate([[0.0], val[dep > 0] * wt]))
        if len(vals) > 1:
            gaps.append(float(np.diff(vals).min()))
    print(f", unit {min(gaps) / float(worst_budget):.3g}")
    assert min(gaps) / float(worst_budget) > DISCRIMINATION
