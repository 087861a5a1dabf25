"""The judges and builders of ``tests/internode_edge_reference.py`` without a device:
``by_edges`` held to ``by_tables`` and ``by_paths``, the closed forms and ``composed`` held to ``by_tables``, and every
named number of every case of ``tests/test_gpu_internode_edges.py`` proved from ``backend.debug_internode_plan`` (the
library's own arithmetic, on the host) and ``chunks``: each gate found by bisection and asserted as a literal."""

import random

import internode_edge_reference as er
import internode_reference as ir
import numpy as np
import parsimony_reference as pr
import pytest

from spectralclustersupertree_amd import backend


def _plan(specs_or_off, n, **kw) -> dict:
    off = er.off_of(specs_or_off) if isinstance(specs_or_off, list) else np.asarray(specs_or_off, dtype=np.int64)
    got = backend.debug_internode_plan(off, n, **kw)
    ref = ir.plan(off, n, **kw)
    for k, v in ref.items():  # (the restatement of section 41 agrees wherever this file reads the plan)
        assert np.array_equal(got[k], v), (k, got[k], v)
    return got


def _named(p: dict) -> tuple:
    return p["tiles_per_item"], p["items_per_row"], p["mirror"], p["n_row_batches"], p["n_tree_batches"], p["words"]


def _step(f, lo: int, hi: int) -> tuple:
    """``(x, x + 1)``: where f leaves f(lo) for good, by bisection (f takes two values on [lo, hi], lo's first)."""
    first = f(lo)
    assert f(hi) != first
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(mid) == first else (lo, mid)
    return lo, hi


# ------------------------------------------------------------------------------------------------ by_edges
def _random_source(rng, n) -> list:
    trees = []
    for _ in range(rng.randint(1, 7)):
        k = rng.randint(1, n)
        leaves = rng.sample(range(n), k)
        tree = pr.rand_tree(leaves, rng.choice([2, 3, 6, 9]), rng) if k > 1 else leaves[0]
        if rng.random() < 0.3 and isinstance(tree, list):
            i = rng.randrange(len(tree))
            tree = [*tree[:i], [tree[i]], *tree[i + 1:]]  # (a unary node above a child)
        trees.append([tree] if rng.random() < 0.3 else tree)  # (a unary root)
    return trees


def test_by_edges_agrees_with_by_tables_and_by_paths_on_random_sources():
    rng = random.Random(4242)
    one_leaf = zero = polytomies = 0
    for _ in range(300):
        n = rng.randint(1, 24)
        trees = _random_source(rng, n)
        w = None if rng.random() < 0.4 else [rng.randint(0, 4) for _ in trees]
        specs = ir.specs_of(trees)
        got, a, b = er.by_edges(specs, n, w), ir.by_tables(specs, n, w), ir.by_paths(trees, n, w)
        for k in ("taxon_weight", "taxon_sum"):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], a[k]), (trees, w)
            assert np.array_equal(got[k], b[k]), (trees, w)
        for t, spec in enumerate(specs):
            alone = ir.by_tables([spec], n)["dist_sum"]
            assert 2 * got["tree_total"][t] == alone.sum(), spec
            one_leaf += len(spec[0]) == 1
            polytomies += any(x == y for x, y in zip(spec[1], spec[1][1:]))
        zero += w is not None and 0 in w
    assert one_leaf > 20 and zero > 50 and polytomies > 200 and got["tree_total"].dtype == np.int64


def test_node_spans_of_hand_made_gaps():
    assert er.node_spans([]) == [] and er.node_spans([0]) == [] and er.node_spans([5, 5, 5]) == []
    assert er.node_spans([1, 0]) == [(0, 1)] and er.node_spans([0, 1]) == [(1, 2)]
    # ((0,1,2),(3,4,5),6): equal depths with a shallower gap between them are two nodes
    assert sorted(er.node_spans([2, 2, 1, 4, 4, 1])) == [(0, 2), (3, 5)]
    # depths 1, 3, 1: the two gaps of depth 1 around a deeper clade are one node
    assert sorted(er.node_spans([1, 3, 1, 0])) == [(0, 3), (1, 2)]
    rows, total = er.tree_by_edges([1, 0])  # ((a,b),c)
    assert rows.tolist() == [5, 5, 6] and total == 8


# ------------------------------------------------------------------------------------------------ closed forms
def _d_of(gaps) -> np.ndarray:
    m = len(gaps) + 1
    return ir.by_tables([(list(range(m)), list(gaps))], m)["dist_sum"]


@pytest.mark.parametrize("left", [True, False])
def test_the_caterpillar_form(left):
    for m in (*range(2, 20), 63, 64, 65, 257):
        gaps = er.caterpillar(range(m), left)[1]
        assert np.array_equal(er.caterpillar_d(m, left), _d_of(gaps)), m
        if m <= 65:
            p = er.piece_of(gaps)
            assert np.array_equal(p.depth, er.caterpillar_depth(m, left))
            assert np.array_equal(p.d, er.caterpillar_d(m, left))
    assert er.caterpillar_d(4).tolist() == [[0, 2, 3, 4], [2, 0, 3, 4], [3, 3, 0, 3], [4, 4, 3, 0]]
    assert er.caterpillar([7, 8, 9], left)[1] == ([1, 0] if left else [0, 1])


def test_the_balanced_and_the_star_form():
    for k in range(1, 9):
        gaps = er.balanced(range(1 << k))[1]
        assert np.array_equal(er.balanced_d(k), _d_of(gaps)), k
        if k <= 5:
            p = er.piece_of(gaps)
            assert p.depth.tolist() == [k] * (1 << k) and np.array_equal(p.d, er.balanced_d(k))
    assert er.balanced_d(2).tolist() == [[0, 2, 4, 4], [2, 0, 4, 4], [4, 4, 0, 2], [4, 4, 2, 0]]
    for m in (*range(2, 12), 64, 65, 300):
        assert np.array_equal(er.star_d(m), _d_of(er.star(range(m), depth=m % 3)[1])), m
    assert er.piece_of([4, 4, 4]).depth.tolist() == [1] * 4


# ------------------------------------------------------------------------------------------------ composed
def _random_piece(rng, m: int) -> er.Piece:
    if m == 1:
        return er.piece_leaf()
    kind = rng.randrange(4)
    if kind == 0:
        return er.piece_caterpillar(m, left=bool(rng.randrange(2)))
    if kind == 1:
        return er.piece_star(m)
    if kind == 2 and m & (m - 1) == 0:
        return er.piece_balanced(m.bit_length() - 1)
    tree = pr.rand_tree(list(range(m)), rng.choice([2, 3, 5]), rng)
    return er.piece_of(ir.specs_of([[tree] if rng.random() < 0.2 else tree])[0][1])


def test_composed_agrees_with_by_tables():
    rng = random.Random(4243)
    singles = cells = 0
    for _ in range(120):
        k = rng.randint(2, 9)
        blocks = [_random_piece(rng, rng.choice([1, 1, 2, 3, 4, 5, 8, 9])) for _ in range(k)]
        c = er.composed(_random_piece(rng, k), blocks)
        d = c.matrix()
        assert np.array_equal(d, _d_of(c.gaps)), c.gaps
        pos = [rng.randrange(c.m) for _ in range(4)]
        assert np.array_equal(c.rows(pos), d[pos])
        singles += sum(b.m == 1 for b in blocks)
        cells += c.m * c.m
    assert singles > 100 and cells > 40000


def test_sum_rows_agrees_with_by_tables_on_weighted_composed_sources():
    rng = random.Random(4244)
    n = 60
    trees = []
    for _ in range(7):
        k = rng.randint(2, 6)
        c = er.composed(_random_piece(rng, k), [_random_piece(rng, rng.randint(1, 8)) for _ in range(k)])
        trees.append((rng.sample(range(n), c.m), c))
    w = [2, 0, 1, 3, 1, 0, 5]
    rows = [0, 59, 0, 17, 30, 31]
    specs = [(taxa, c.gaps) for taxa, c in trees]
    got, ref = er.sum_rows(trees, n, rows, w), ir.by_tables(specs, n, w, rows)
    for k in ir.MATRICES:
        assert np.array_equal(got[k], ref[k]), k
    assert got["pair_weight"].any()


def test_the_composed_trees_of_the_device_case_at_their_size():
    trees, specs, n, w = er.case_real()
    sizes = [len(t) for t, _ in specs]
    assert n == 3000 and len(trees) == 10 and min(sizes) >= 2000 and max(sizes) <= 3000 and max(sizes) >= 2048
    assert all(len(set(t)) == len(t) for t, _ in specs) and 0 in w and w[0] == 2
    assert specs[0][0][0] == n - 1 and specs[0][0][-1] == 0 and specs[1][0][0] == 0 and specs[1][0][-1] == n - 1
    edges = er.by_edges(specs, n)
    for t in (0, 4):  # (every cell of two of them, 72 MB each: the linear judge against the outer sums)
        d = trees[t][1].matrix()
        assert 2 * edges["tree_total"][t] == d.sum() and np.array_equal(d, d.T) and not d.diagonal().any()
        rows, _ = er.tree_by_edges(specs[t][1])
        assert np.array_equal(rows, d.sum(axis=1))
    # polytomy runs and deep clades are there by construction
    kinds = {type(b.gaps) for _, c in trees for b in c.blocks}
    assert kinds == {list} and max(int(c.depth.max()) + len(c.blocks) for _, c in trees) > 100
    runs = {b.m - 1 for _, c in trees for b in c.blocks if b.m > 2 and len(set(b.gaps)) == 1}
    assert {r for j in range(2, 8) for r in ((1 << j) - 1, 1 << j, (1 << j) + 1)} <= runs, sorted(runs)


# ------------------------------------------------------------------------------------------------ polytomies
def test_polytomy_builders_make_the_nodes_they_name():
    for run in (1, 2, 3, 4, 5, 8, 17):
        for where in ("left", "right"):
            c = er.polytomy_piece(run, where)
            assert c.gaps == er.polytomy_gaps(run, where), (run, where)
            assert np.array_equal(c.matrix(), _d_of(c.gaps))
        g = er.polytomy_gaps(run, "middle")
        r = ir.depths_by_tables([(list(range(len(g) + 1)), g)])["gap_r"][:-1]
        assert r.tolist() == [0, 1, 2] + [3] * run + [2, 1, 0]  # (an arm's gap is the node of its twin across the run)
        g = er.polytomy_gaps(run, "interrupted")
        r = ir.depths_by_tables([(list(range(len(g) + 1)), g)])["gap_r"][:-1]
        assert g.count(1) == run and {x for x, d in zip(r.tolist(), g) if d == 1} == {1}
        spans = er.node_spans(g)
        assert sum(hi - lo + 1 == len(g) for lo, hi in spans) == 1  # (one node holds the whole run)
        assert run < 3 or max(g) > 1
        g = er.polytomy_gaps(run, "ended")
        spans = sorted(er.node_spans(g))
        assert spans == [(0, run), (0, 2 * run + 1), (run + 1, 2 * run + 1)]
    assert er.RUNS[:6] == (1, 2, 3, 3, 4, 5) and er.RUNS[-3:] == (1023, 1024, 1025) and len(er.RUNS) == 30


@pytest.mark.parametrize("where", ["star", *er.RUN_PLACES])
def test_the_run_sources_by_edges_and_by_tables(where):
    specs, n = er.run_specs(where)
    assert len(specs) == 30 and all(len(set(t)) == len(t) and max(t) < n for t, _ in specs)
    rows = list(range(0, n, max(n // 24, 1)))
    ref, edges = ir.by_tables(specs, n, None, rows), er.by_edges(specs, n)
    assert np.array_equal(ref["taxon_sum"], edges["taxon_sum"][rows]) and ref["pair_weight"].any()
    assert np.array_equal(ref["taxon_weight"], edges["taxon_weight"][rows])
    if where == "star":
        assert [len(t) for t, _ in specs] == list(er.RUNS) and specs[0][1] == []
        assert np.array_equal(ref["dist_sum"], 2 * ref["pair_weight"])
        assert edges["tree_total"].tolist() == [m * (m - 1) for m in er.RUNS]


# ------------------------------------------------------------------------------------------------ shifted, chunks
def test_shifted_and_chunks():
    specs = [([3, 1, 2], [4, 0]), ([0], []), ([2, 0], [9])]
    t = er.shifted(specs, [7, 0, 1000000], er.INT32_MAX, 4)
    assert t.adj_depth.tolist() == [11, 7, er.INT32_MAX, er.INT32_MAX, 1000009, er.INT32_MAX]
    assert t.adj_depth.dtype == np.int32 and t.tree_off.tolist() == [0, 3, 4, 6]
    assert t.leaf_taxon.tolist() == [3, 1, 2, 0, 2, 0]
    plain = ir.tables(specs, 4)
    assert np.array_equal(er.shifted(specs, [0, 0, 0], 0, 4).adj_depth, plain.adj_depth)
    assert er.chunks(0, 1) == (1, [1]) and er.chunks(0, 1024) == (1, [32]) and er.chunks(0, 1025) == (2, [32, 1])
    assert er.chunks(31, 33) == (1, [2]) and er.chunks(1000, 1100) == (1, [4]) and er.chunks(0, 1100) == (2, [32, 3])
    assert er.chunks(32, 1056) == (1, [32]) and er.chunks(32, 1057) == (2, [32, 1])
    assert er.chunks(0, 2049) == (3, [32, 32, 1])


# ------------------------------------------------------------------------------------------------ the gates
def _pairs(n_trees: int) -> np.ndarray:
    return 2 * np.arange(n_trees + 1, dtype=np.int64)  # (trees of two leaves)


def test_the_gates_of_the_plan_by_bisection():
    off = _pairs(10)
    # tiles of an item: rows x tiles // 8192
    assert _step(lambda r: _plan(off, 600, n_rows=r, matrices=2)["tiles_per_item"], 1, 8192) == (5461, 5462)
    assert _step(lambda n: _plan(off, n)["tiles_per_item"], 1, 4096) == (2047, 2048)
    assert _step(lambda n: _plan(off, n, matrices=1)["tiles_per_item"], 1, 4096) == (2047, 2048)
    # words and chunks of one batch
    assert _step(lambda m: _plan(_pairs(m), 70)["words"] > 32, 1, 4096) == (1024, 1025)
    assert _step(lambda m: er.chunks(0, m)[0], 1, 2048) == (1024, 1025)

    def second(b: int) -> tuple:
        p = _plan(_pairs(2 * b), 70, batch_trees=b)
        assert p["first_tree"].tolist() == [0, b] and p["trees"].tolist() == [b, b]
        return er.batch_chunks(p)[1]

    assert _step(lambda b: second(b)[0], 512, 1023) == (1008, 1009)
    assert second(1008) == (1, [32]) and second(1009) == (2, [32, 1]) and second(1023) == (2, [32, 1])
    # (a batch of exactly 1 024 trees from tree 1 024 on starts on a word: one chunk again)
    assert second(1024) == (1, [32])
    # mirror: all rows in one row batch
    for n in (150, 2049):
        assert _step(lambda r: _plan(off, n, batch_rows=r, matrices=3)["mirror"], 1, n) == (n - 1, n)
        assert _plan(off, n, batch_rows=n - 1, matrices=3)["n_row_batches"] == 2
        assert _plan(off, n, batch_rows=n - 1, matrices=0)["mirror"] == 1  # (no matrices: any number of row batches)
        assert _plan(off, n, n_rows=n, matrices=0)["mirror"] == 0  # (rows given, if all of them: no mirror)


# ------------------------------------------------------------------------------------------------ the cases
def test_the_numbers_of_the_chosen_rows_case():
    specs, n, rows = er.case_tg_rows()
    assert (n, len(specs), len(rows)) == (600, 1100, 5462) and max(len(t) for t, _ in specs) == 9
    present = {x for t, _ in specs for x in t}
    assert sorted(set(range(n)) - present) == [592, 593, 594, 595, 596, 597] and {595, 597} <= set(rows)
    assert len(set(rows)) == 600 and len(set(rows[:5461])) == 600  # (every taxon is a row, most of them many times)
    # tiles_per_item, items_per_row, mirror, row batches, tree batches, words
    assert _named(_plan(specs, n, n_rows=5461, matrices=2)) == (1, 3, 0, 1, 1, 35)
    assert _named(_plan(specs, n, n_rows=5462, matrices=2)) == (2, 2, 0, 1, 1, 35)
    p = _plan(specs, n, n_rows=5462, matrices=2)
    assert p["tiles"] == 3 and er.batch_chunks(p) == [(2, [32, 3])] and p["levels"] == 4
    assert p["row_bytes"] == 9600 and p["bytes"] - p["fixed_bytes"] == 2 * 5462 * 600 * 8
    p = _plan(specs, n, n_rows=5462, matrices=2, batch_trees=1000)
    assert _named(p) == (2, 2, 0, 1, 2, 35) and p["first_tree"].tolist() == [0, 1000]
    assert er.batch_chunks(p) == [(1, [32]), (1, [4])]
    p = _plan(specs, n, n_rows=5461, matrices=2, batch_trees=1000)
    assert _named(p) == (1, 3, 0, 1, 2, 35)
    # the first 1 000 trees: one chunk, staged once for both tiles of an item
    for r, named in ((5461, (1, 3, 0, 1, 1, 32)), (5462, (2, 2, 0, 1, 1, 32))):
        p = _plan(specs[:1000], n, n_rows=r, matrices=2)
        assert _named(p) == named and er.batch_chunks(p) == [(1, [32])]


def test_the_numbers_of_the_mirror_cases():
    for n, tiles, tg, ng in ((2047, 8, 1, 8), (2048, 8, 2, 4), (2049, 9, 2, 5)):
        specs = er.case_mirror(n)
        assert len(specs) == 402 and specs[-1][0] == [n - 1, 0, 1, n - 2]
        for mats in (0, 1):
            p = _plan(specs, n, matrices=mats)
            assert _named(p) == (tg, ng, 1, 1, 1, 13) and p["tiles"] == tiles and er.batch_chunks(p) == [(1, [13])]
    # 9 tiles in groups of 2: the last group is one tile
    assert 9 - 2 * (5 - 1) == 1
    trees, specs, n, _ = er.case_real()
    p = _plan(specs, n)
    assert _named(p) == (4, 3, 1, 1, 1, 1) and p["tiles"] == 12 and p["levels"] == 12
    p = _plan(specs, n, n_rows=8, matrices=3)
    assert _named(p) == (1, 12, 0, 1, 1, 1)


def test_the_numbers_of_the_chunk_and_word_cases():
    for m, words, ch in ((1023, 32, (1, [32])), (1024, 32, (1, [32])), (1025, 33, (2, [32, 1]))):
        specs, n = er.case_chunk_gate(m)
        p = _plan(specs, n)
        assert _named(p) == (1, 1, 1, 1, 1, words) and er.batch_chunks(p) == [ch] and n == 70
        where = [[t for t, (taxa, _) in enumerate(specs) if x in taxa] for x in (69, 68, 67)]
        assert where == [[1023][:m - 1023], [1024][:max(m - 1024, 0)], [1023, 1024][:max(m - 1023, 0)]]
    for m, b, second in ((2016, 1008, (1, [32])), (2018, 1009, (2, [32, 1]))):
        specs, n = er.case_mid_word(m)
        p = _plan(specs, n, batch_trees=b)
        assert _named(p) == (1, 1, 1, 1, 2, 63 + (m > 2016)) and p["first_tree"].tolist() == [0, b]
        assert er.batch_chunks(p) == [(1, [32]), second] and b & 31 in (16, 17)
        assert [t for t, (taxa, _) in enumerate(specs) if 69 in taxa] == [m - 1]
    # the last tree of the 2 018 lies in the second chunk's only word, with one tree beside it
    assert (2017 >> 5) - (1009 >> 5) == 32 and 2016 >> 5 == 2017 >> 5 == 63
    specs, n = er.case_mid_word(1100)
    p = _plan(specs, n, batch_trees=33)
    assert _named(p) == (1, 1, 1, 1, 34, 35) and p["trees"].tolist() == [33] * 33 + [11]
    assert {int(t) & 31 for t in p["first_tree"]} == set(range(32))
    assert [c for c in er.batch_chunks(p)] == [(1, [2])] * 33 + [(1, [1])]


def test_the_numbers_of_the_small_cases():
    rng = random.Random(5)
    off = er.off_of(er.random_specs(rng, 150, 45, 3, 60))
    assert _named(_plan(off, 150, batch_rows=150, matrices=3)) == (1, 1, 1, 1, 1, 2)
    assert _named(_plan(off, 150, batch_rows=149, matrices=3)) == (1, 1, 0, 2, 1, 2)
    p = _plan(off, 150, batch_rows=149, matrices=3, batch_trees=3)
    assert _named(p) == (1, 1, 0, 2, 15, 2) and p["rows"].tolist() == [149, 1]
    assert _named(_plan(off, 150, batch_rows=150, matrices=3, batch_trees=3)) == (1, 1, 1, 1, 15, 2)
    for turn in ("left", "right", "mixed", "random"):
        specs, n = er.case_waves(turn)
        off = er.off_of(specs)
        assert off.tolist() == [0, 64, 192, 193, 256, 321, 322, 386] and n == 130 and 386 % 64 == 2
        for b, first, leaves in ((0, [0], [386]), (1, list(range(7)), list(er.WAVE_SIZES)),
                                 (3, [0, 3, 6], [193, 129, 64])):
            p = _plan(specs, n, batch_trees=b)
            assert p["first_tree"].tolist() == first and p["leaves"].tolist() == leaves and p["levels"] == 8
    # the deepest leaves of a left caterpillar are its first two, of a right one its last two
    deep = ir.depths_by_tables([er.caterpillar(range(64)), er.caterpillar(range(64), left=False)])["leaf_depth"]
    assert deep[:2].tolist() == [63, 63] and deep[126:].tolist() == [63, 63] and deep.max() == 63
    specs, n = er.case_rounds("deep_then_small")
    p = _plan(specs, n, batch_trees=1)
    assert p["levels"] == 9 and p["leaves"].tolist() == [300, 2, 3, 2, 3] and _plan(specs, n)["n_tree_batches"] == 1
    specs, n = er.case_rounds("parities")
    p = _plan(specs, n, batch_trees=1)
    assert p["levels"] == 3 and p["leaves"].tolist() == [3, 4, 5, 6, 7]
    # rounds of pointer doubling: the levels of the batch's largest tree; an odd count ends in the second buffer
    assert [er.rounds(m) for m in (2, 3, 4, 7, 300)] == [2, 2, 3, 3, 9]
    specs, n = er.case_leak()
    assert n == 90 and [len(t) for t, _ in specs][7:11] == [33, 65, 1, 64] and len(specs) == 15
    for kind in ("star", *er.RUN_PLACES):
        specs, n = er.run_specs(kind)
        p = _plan(specs, n)
        assert _named(p)[2:5] == (1, 1, 1) and p["levels"] == (12 if kind == "ended" else 11)
