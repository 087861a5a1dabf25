"""The summed internode distances of the sources on the device (``scs_score_internode``) held
bitwise to the references of ``tests/internode_reference.py``: every case with the matrices and without, with squares,
and with each output null in turn.  Hand-made sources and raw ``adj_depth``, taxa counts around a wave and a tile, tree
counts around a word, tree sizes around every table level, the depth pass alone on deep and wide trees, cells past
2^32, weights, rows and batches, sparse sources, the refusals, and the way through ``source_internode_distances`` and
the command line."""

import random
from functools import lru_cache
from pathlib import Path

import internode_reference as ir
import numpy as np
import parsimony_reference as pr
import pytest
from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import (backend, load_trees, source_coverage, source_internode_distances,
                                          synthetic)
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.load import load_tree_arrays

pytestmark = pytest.mark.gpu

DATA = Path(__file__).parent / "golden" / "reference_data"
ALL = {"matrices": True, "squares": True}


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what) -> None:
    for k in ir.KEYS:
        if got[k] is None:
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (what, k, bad[:6].tolist(), got[k][got[k] != ref[k]][:6], ref[k][got[k] != ref[k]][:6])


def _check(dev, specs, n, rows=None, weights=None, row_batches=(0,), tree_batches=(0,), trees=None, nulls=True,
           what="") -> dict:
    """Every setting against ``by_tables`` (and ``by_paths`` when nested-list ``trees`` are given, or the input is
    small): the matrices on and off, squares on and off, each output null in turn; the invariants.  Returns the
    device's full answer."""
    ref = ir.by_tables(specs, n, weights, rows)
    if trees is not None or sum(len(t) for t, _ in specs) <= 400:
        nested = trees if trees is not None else [ir.nested_of(*s) for s in specs]
        _same(ir.by_paths(nested, n, weights, rows), ref, (what, "the references"))
    tabs = dev.upload(ir.tables(specs, n))
    try:
        full = None
        for rb in row_batches:
            for tb in tree_batches:
                at = (what, rb, tb)
                full = dev.score_internode(tabs, rows, weights, batch_rows=rb, batch_trees=tb, **ALL)
                assert all(full[k] is not None for k in ir.KEYS)
                _same(full, ref, at)
                ir.check_invariants(full, n, rows)
                lean = dev.score_internode(tabs, rows, weights, matrices=False, squares=True, batch_rows=rb,
                                           batch_trees=tb)
                assert all(lean[k] is None for k in ir.MATRICES) and all(lean[k] is not None for k in ir.SUMS)
                _same(lean, ref, (*at, "no matrices"))
        plain = dev.score_internode(tabs, rows, weights)
        assert [k for k in ir.KEYS if plain[k] is None] == ["sq_sum", "taxon_sq"]
        _same(plain, ref, (what, "no squares"))
        for k in ir.KEYS if nulls else ():
            part = dev.score_internode(tabs, rows, weights, outputs=[x for x in ir.KEYS if x != k])
            assert [x for x in ir.KEYS if part[x] is None] == [k]
            _same(part, ref, (what, "without", k))
            one = dev.score_internode(tabs, rows, weights, outputs=[k])
            assert [x for x in ir.KEYS if one[x] is not None] == [k]
            _same(one, ref, (what, "only", k))
    finally:
        tabs.free()
    return full


def _caterpillar(taxa, left: bool = True) -> tuple:
    """Raw arrays of ((((a,b),c),d),...) when ``left``, else (a,(b,(c,...)))."""
    g = list(range(len(taxa) - 1))
    return list(taxa), g[::-1] if left else g


# ------------------------------------------------------------------------------------------------ hand-made sources
def test_a_cherry_a_caterpillar_and_a_star(dev):
    got = _check(dev, ir.specs_of([[0, 1]]), 2, trees=[[0, 1]])
    assert got["dist_sum"].tolist() == [[0, 2], [2, 0]] and got["pair_weight"].tolist() == [[0, 1], [1, 0]]
    got = _check(dev, ir.specs_of([[[0, 1], 2]]), 3, trees=[[[0, 1], 2]])
    assert got["dist_sum"].tolist() == [[0, 2, 3], [2, 0, 3], [3, 3, 0]] and got["sq_sum"][0].tolist() == [0, 4, 9]
    got = _check(dev, ir.specs_of([[0, 1, 2, 3, 4]]), 5, trees=[[0, 1, 2, 3, 4]])
    assert (got["dist_sum"] + 2 * np.eye(5, dtype=np.int64) == 2).all() and got["taxon_partners"].tolist() == [4] * 5


def test_unary_nodes_and_depth_jumps_are_not_counted(dev):
    # a unary root, a unary node above a leaf and above a clade: the same distances as without them
    plain = [[0, 1], 2, [3, 4, 5]]
    unary = [[[[0, [1]]], [2], [[3, 4, 5]]]]
    a = _check(dev, ir.specs_of([plain]), 6, trees=[plain])
    b = _check(dev, ir.specs_of([unary]), 6, trees=[unary])
    _same(a, b, "unary nodes")
    assert ir.specs_of([plain]) != ir.specs_of([unary])
    # raw depths 0, 3, 3, 5 are (0,(1,2,(3,4))): the top node has r = 0 wherever its depth starts
    for shift in (0, 7):
        got = _check(dev, [([0, 1, 2, 3, 4], [shift + x for x in (0, 3, 3, 5)])], 5, trees=[[0, [1, 2, [3, 4]]]])
        assert got["dist_sum"][0].tolist() == [0, 3, 3, 4, 4] and got["dist_sum"][3].tolist() == [4, 3, 3, 0, 2]
    # a polytomy next to a deeper clade, and equal depths apart from one another: two nodes, not one
    got = _check(dev, [([0, 1, 2, 3, 4, 5, 6], [2, 2, 1, 4, 4, 1]), ([6, 5, 4, 3, 2, 1, 0], [3, 0, 3, 0, 5, 5])], 7)
    # ((0,1,2),(3,4,5),6) and ((6,5),(4,3),(2,1,0)): d(0,1) = 2 + 2, d(0,3) = 4 + 4, d(6,4) = 3 + 4
    assert got["dist_sum"][0, 1] == 4 and got["dist_sum"][0, 3] == 8 and got["dist_sum"][6, 4] == 7
    assert got["pair_weight"][0, 6] == 2


def test_taxa_in_no_one_and_all_trees_and_trees_of_one_two_and_three_leaves(dev):
    # taxon 0 in every tree, 9 in one, 10 in none; one-leaf trees have no pairs
    trees = [[[0, 1], [2, [3, 4]]], 0, [0, 5], [[0, 1], 6], [0, [2, 3, [7, 8]], 9], [[4, 0], [1, 2]], [3, 0]]
    got = _check(dev, ir.specs_of(trees), 11, trees=trees, row_batches=(0, 1, 3), tree_batches=(0, 1, 3))
    assert not got["pair_weight"][10].any() and not got["pair_weight"][:, 10].any() and got["taxon_partners"][10] == 0
    assert got["taxon_partners"].tolist()[:2] == [9, 5] and got["pair_weight"][0, 1] == 3
    assert got["taxon_partners"][9] == 5 and got["pair_weight"][9].sum() == 5


def test_disjoint_trees_leave_pairs_missing_and_identical_trees_add_up(dev):
    trees = [[[0, 1], [2, 3]], [4, [5, 6]], [7, 8]]
    got = _check(dev, ir.specs_of(trees), 9, trees=trees)
    assert not got["pair_weight"][:4, 4:].any() and got["taxon_partners"].tolist() == [3, 3, 3, 3, 2, 2, 2, 1, 1]
    tree = [[0, [1, 2]], [3, [4, [5, 6]]]]
    one = _check(dev, ir.specs_of([tree]), 7, trees=[tree])
    three = _check(dev, ir.specs_of([tree] * 3), 7, trees=[tree] * 3, tree_batches=(0, 2))
    for k in ir.KEYS[:-1]:
        assert np.array_equal(three[k], 3 * one[k])
    assert ir.four_point(one["dist_sum"])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_two_and_three_taxa(dev, n):
    trees = [list(range(n)) if n > 1 else 0] * 2 + [0]
    got = _check(dev, ir.specs_of(trees), n, trees=trees, row_batches=(0, 1), tree_batches=(0, 1))
    assert got["dist_sum"].sum() == 2 * 2 * n * (n - 1)
    empty = _check(dev, ir.specs_of(trees), n, rows=[], nulls=False)
    assert empty["dist_sum"].shape == (0, n) and empty["taxon_sum"].shape == (0,)


# ------------------------------------------------------------------------------------------------ lanes, words, levels
def _random_specs(rng, n, n_trees, lo, hi, arity=3) -> list:
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(min(lo, n), min(hi, n))), arity, rng) for _ in range(n_trees)]
    return ir.specs_of(trees)


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_taxa_counts_around_a_wave_and_a_tile(dev, n):
    rng = random.Random(n)
    specs = _random_specs(rng, n, 12, 3, n // 2)
    specs += ir.specs_of([[[n - 1, n - 2], 0], pr.rand_tree(list(range(n)), 4, rng)])  # the last lanes with the first
    got = _check(dev, specs, n, nulls=n in (65, 257), row_batches=(0, 64))
    assert got["pair_weight"][n - 1, 0] >= 2 and got["taxon_partners"].min() == n - 1


@pytest.mark.parametrize("n_trees", [31, 32, 33, 63, 64, 65, 129])
def test_tree_counts_around_a_word(dev, n_trees):
    rng = random.Random(n_trees)
    n = 70
    specs = _random_specs(rng, n - 3, n_trees, 2, 12)  # (the last three taxa are placed by hand)
    specs[-1] = ir.specs_of([[pr.rand_tree(specs[-1][0], 2, rng), n - 1]])[0]  # taxon n - 1 only in the last tree
    if n_trees > 32:
        specs[31] = (specs[31][0] + [n - 2], specs[31][1] + [0])  # n - 2 only in tree 31, the last bit of word 0
        specs[32] = ([n - 3] + specs[32][0], [0] + specs[32][1])  # n - 3 only in tree 32, the first bit of word 1
    got = _check(dev, specs, n, nulls=False, tree_batches=(0, 32, 33))
    assert got["taxon_weight"][n - 1] == len(specs[-1][0]) - 1 and got["taxon_partners"][n - 1] > 0
    if n_trees > 32:
        assert got["pair_weight"][n - 2, n - 3] == 0 and got["taxon_partners"][n - 2] == len(specs[31][0]) - 1
        assert got["taxon_partners"][n - 3] == len(specs[32][0]) - 1


@pytest.mark.parametrize("k", range(1, 10))
def test_tree_sizes_around_every_table_level(dev, k):
    # trees of 2^k - 1, 2^k and 2^k + 1 leaves: a balanced-ish random tree, and a caterpillar whose end pairs span
    # every gap of the tree (the top level of its table, both entries overlapping or not)
    rng = random.Random(k)
    sizes = [s for s in ((1 << k) - 1, 1 << k, (1 << k) + 1) if s >= 2]
    n = sizes[-1] + 3
    specs = []
    for s in sizes:
        specs += ir.specs_of([pr.rand_tree(rng.sample(range(n), s), 3, rng)])
        specs.append(_caterpillar(rng.sample(range(n), s), left=bool(s & 1)))
    rows = None if k <= 7 else sorted({0, 1, n - 1, *(specs[-1][0][i] for i in (0, 1, -2, -1))})
    got = _check(dev, specs, n, rows=rows, nulls=False, tree_batches=(0, 1))
    first, last = specs[-1][0][0], specs[-1][0][-1]
    i = first if rows is None else rows.index(first)
    assert got["dist_sum"][i, last] >= sizes[-1]  # (the two ends of the caterpillar: every node between them)


# ------------------------------------------------------------------------------------------------ the depth pass
def _depths(dev, specs, n, batches=(0,)) -> dict:
    ref = ir.depths_by_tables(specs)
    tabs = dev.upload(ir.tables(specs, n))
    try:
        for tb in batches:
            got = dev.debug_internode_depths(tabs, batch_trees=tb)
            for k in ("gap_r", "leaf_depth", "tree_height"):
                assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (k, tb)
    finally:
        tabs.free()
    return ref


def test_the_depth_pass_on_caterpillars_a_balanced_and_a_random_tree(dev):
    n = 5000
    rng = random.Random(50)
    balanced = list(range(512))
    while len(balanced) > 1:
        balanced = [balanced[i:i + 2] for i in range(0, len(balanced), 2)]
    specs = [_caterpillar(range(300)), _caterpillar(range(300), left=False), ir.specs_of(balanced)[0],
             ir.specs_of([pr.rand_tree(list(range(n)), 5, rng)])[0], ([7], []),
             (list(range(40)), [rng.choice([2, 2, 5, 9, 30]) for _ in range(39)])]
    ref = _depths(dev, specs, n, batches=(0, 1, 2))
    assert ref["tree_height"].tolist()[:3] == [299, 299, 9] and ref["tree_height"][4] == 0


@lru_cache(maxsize=None)
def _long():
    n = 70000
    spec = _caterpillar(range(n))
    rows = [0, n // 2, n - 1]
    return n, spec, rows, ir.depths_by_tables([spec]), ir.by_tables([spec], n, None, rows)


def test_a_caterpillar_of_70000_leaves_passes_the_depth_pass(dev):
    n, spec, _, ref, _ = _long()
    assert ref["tree_height"].tolist() == [n - 1] and ref["gap_r"][0] == n - 2
    tabs = dev.upload(ir.tables([spec], n))
    try:
        got = dev.debug_internode_depths(tabs)
        for k in ("gap_r", "leaf_depth", "tree_height"):
            assert np.array_equal(got[k], ref[k]), k
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ width and 2^32
def test_cells_past_32_bits_in_the_squares_of_a_70000_leaf_caterpillar(dev):
    n, spec, rows, _, ref = _long()
    assert ref["sq_sum"].max() > 1 << 32 and ref["dist_sum"].max() == n - 1 + 1
    tabs = dev.upload(ir.tables([spec], n))
    try:
        _same(dev.score_internode(tabs, rows, **ALL), ref, "70000")
        _same(dev.score_internode(tabs, rows, matrices=False, squares=True), ref, "70000 lean")
    finally:
        tabs.free()


def test_cells_past_32_bits_in_the_sums_of_a_heavy_3000_leaf_caterpillar(dev):
    n, w = 3000, [2_000_000]
    spec = _caterpillar(random.Random(3).sample(range(n), n), left=False)
    b1, b2 = ir.bounds([n], [n - 1], w)
    assert b1 < b2 <= ir.LIMIT
    rows = [spec[0][0], spec[0][n // 2], spec[0][-1], 5]
    ref = ir.by_tables([spec], n, w, rows)
    assert ref["dist_sum"].max() > 1 << 32
    tabs = dev.upload(ir.tables([spec], n))
    try:
        _same(dev.score_internode(tabs, rows, w, **ALL), ref, "heavy")
        lean = dev.score_internode(tabs, None, w, matrices=False, squares=True)
        _same(lean, ir.by_tables([spec], n, w), "heavy, every row")
        assert lean["taxon_sq"].max() <= b2 and lean["taxon_sum"].max() <= b1
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ weights
def test_weights_count_like_copies_and_weight_zero_like_absence(dev):
    rng = random.Random(9)
    n = 40
    specs = _random_specs(rng, n, 9, 2, 25, arity=4)
    w = [3, 0, 1, 2, 0, 5, 1, 1, 4]
    got = _check(dev, specs, n, weights=w, tree_batches=(0, 1, 4), nulls=False)
    copies = [s for s, k in zip(specs, w) for _ in range(k)]
    _same(_check(dev, copies, n, nulls=False), got, "copies")
    kept = [s for s, k in zip(specs, w) if k]
    _same(_check(dev, kept, n, weights=[k for k in w if k], nulls=False), got, "weight 0 removed")
    ones = _check(dev, specs, n, weights=[1] * 9, nulls=False)
    _same(_check(dev, specs, n, nulls=False), ones, "ones")
    # integral floats are integers to the array's eye; the library sees int64 either way
    tabs = dev.upload(ir.tables(specs, n))
    try:
        _same(dev.score_internode(tabs, None, np.asarray(w, dtype=np.int64), **ALL), got, "int64 array")
    finally:
        tabs.free()


def test_sums_past_63_bits_are_refused_by_name_before_anything_is_summed(dev):
    n = 300
    spec = _caterpillar(range(n))
    tabs = dev.upload(ir.tables([spec, ([0, 1], [0])], n))
    h = n - 1
    try:
        used = dev.arena_stats()["used_bytes"]
        # B2 alone passes: refused only when squares are asked for
        w2 = ir.LIMIT // ((n - 1) * (2 * h) ** 2) + 1
        assert ir.bounds([n, 2], [h, 1], [w2, 0])[1] > ir.LIMIT >= ir.bounds([n, 2], [h, 1], [w2, 0])[0]
        with pytest.raises(ValueError, match=r"^scs_score_internode: the bound B2 .* on sq_sum passes 2\^63 - 1 at tree 0$"):
            dev.score_internode(tabs, [0], [w2, 0], **ALL)
        with pytest.raises(ValueError, match="the bound B2"):
            dev.score_internode(tabs, [0], [w2, 0], outputs=["taxon_sq"])
        ok = dev.score_internode(tabs, [0, n - 1], [w2, 0])
        _same(ok, ir.by_tables([spec, ([0, 1], [0])], n, [w2, 0], [0, n - 1]), "B1 fits")
        # one below the B2 limit is taken
        ok = dev.score_internode(tabs, [0, n - 1], [w2 - 1, 0], **ALL)
        _same(ok, ir.by_tables([spec, ([0, 1], [0])], n, [w2 - 1, 0], [0, n - 1]), "B2 fits")
        w1 = ir.LIMIT // ((n - 1) * 2 * h) + 1
        with pytest.raises(ValueError, match=r"^scs_score_internode: the bound B1 .* on dist_sum passes 2\^63 - 1 at tree 0$"):
            dev.score_internode(tabs, [0], [w1, 0], matrices=False)
        # the second tree tips the sum over
        with pytest.raises(ValueError, match="the bound B1 .* at tree 1$"):
            dev.score_internode(tabs, [0], [w1 - 1, ir.LIMIT // 2], matrices=False)
        assert dev.arena_stats()["used_bytes"] == used
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ rows and batches
def test_chosen_repeated_and_no_rows_and_every_batch_size(dev):
    rng = random.Random(5)
    n = 150
    specs = _random_specs(rng, n, 45, 3, 60)
    full = _check(dev, specs, n, row_batches=(0, 1, 3, 64), tree_batches=(0, 1, 3), nulls=False)  # rows None: mirror
    explicit = _check(dev, specs, n, rows=list(range(n)), row_batches=(0, 64), tree_batches=(0, 3), nulls=False)
    _same(explicit, full, "mirror against range(n)")
    _check(dev, specs, n, rows=[149, 0, 77, 0, 149, 149, 64, 63], row_batches=(0, 1, 3), tree_batches=(0, 3))
    off = ir.tables(specs, n).tree_off
    assert backend.debug_internode_plan(off, n, matrices=3)["mirror"] == 1
    assert backend.debug_internode_plan(off, n, batch_rows=3, matrices=3)["mirror"] == 0
    assert backend.debug_internode_plan(off, n, batch_rows=3, matrices=0)["mirror"] == 1
    assert backend.debug_internode_plan(off, n, n_rows=n, matrices=3)["mirror"] == 0
    assert backend.debug_internode_plan(off, n, batch_trees=3)["n_tree_batches"] == 15
    # the unweighted pair weights are the pair counts of the coverage
    tabs = dev.upload(ir.tables(specs, n))
    try:
        cov = dev.score_coverage(tabs, None, 1, True)
        ir.check_invariants(full, n, None, cov["pair_trees"])
    finally:
        tabs.free()


def test_more_trees_than_one_staging_chunk_and_items_of_several_tiles(dev):
    # 1 100 trees are 35 words, past the 32 a workgroup stages at once; 600 taxa are 3 tiles
    rng = random.Random(11)
    n = 600
    specs = _random_specs(rng, n, 1100, 2, 9)
    specs[-1] = ir.specs_of([[[n - 1, 0], [1, n - 2]]])[0]
    rows = [n - 1, 0, 300, 255, 256, 1]
    got = _check(dev, specs, n, rows=rows, tree_batches=(0, 1000), nulls=False)
    assert got["pair_weight"][0, 0] >= 1
    tabs = dev.upload(ir.tables(specs, n))
    try:
        lean = dev.score_internode(tabs, None, matrices=False, squares=True)
        _same(lean, ir.by_tables(specs, n), "every row, no matrices")
    finally:
        tabs.free()


def test_sparse_sources(dev):
    # 40 trees of 12 leaves over 300 taxa: most pairs never co-occur
    rng = random.Random(40)
    n = 300
    specs = _random_specs(rng, n, 40, 12, 12)
    got = _check(dev, specs, n, row_batches=(0, 50), nulls=False)
    occurs = np.bincount([x for taxa, _ in specs for x in taxa], minlength=n)
    # (a taxon meets at most the 11 others of every tree that holds it)
    assert (got["pair_weight"] == 0).mean() > 0.9 and (got["taxon_partners"] <= 11 * occurs).all()
    assert np.array_equal(got["taxon_weight"], 11 * occurs) and (occurs == 0).any()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_messages(dev):
    trees = [[[0, 1], 2], [1, [2, 3]], [0, 3]]
    specs = ir.specs_of(trees)
    tabs = dev.upload(ir.tables(specs, 4))
    who = "scs_score_internode: "
    ref = ir.by_paths(trees, 4)
    try:
        used = dev.arena_stats()["used_bytes"]
        for rows, said in (([4], r"rows\[0\] = 4 is not a taxon of the tables \(4 taxa\)"),
                           ([0, -1], r"rows\[1\] = -1 is not a taxon")):
            with pytest.raises(ValueError, match=who + said):
                dev.score_internode(tabs, rows=rows)
        for kwargs, said in (({"batch_rows": -1}, "max_batch_rows = -1 is negative"),
                             ({"batch_trees": -1}, "max_batch_trees = -1 is negative"),
                             ({"tree_weights": [1, -1, 1]}, r"tree_w\[1\] = -1 is negative")):
            with pytest.raises(ValueError, match=who + said):
                dev.score_internode(tabs, **kwargs)
        with pytest.raises(ValueError, match="one weight per tree"):
            dev.score_internode(tabs, tree_weights=[1, 1])
        lib, buf = dev._lib, np.zeros(4, dtype=np.int64)
        rows = np.zeros(3, dtype=np.int32)
        for n_rows, row_ptr, said in ((-1, rows.ctypes.data, b"n_rows = -1 is negative"),
                                      (2, None, b"rows is null and n_rows = 2 is not the 4 taxa of the tables")):
            assert lib.scs_score_internode(dev._ctx, tabs._h, n_rows, row_ptr, None, 0, 0, None, None, None,
                                           buf.ctypes.data, None, None, None) == nv.EINVAL
            assert lib.scs_last_error() == who.encode() + said
        for ctx, handle in ((dev._ctx, None), (None, tabs._h)):
            assert lib.scs_score_internode(ctx, handle, 0, None, None, 0, 0, None, None, None, None, None, None,
                                           None) == nv.EINVAL
            assert lib.scs_last_error() == b"scs_score_internode: null argument"
        assert dev.arena_stats()["used_bytes"] == used
        # a taxon twice in a tree of the first batch or of a later one: found before a distance is summed
        for at in (0, 2):
            bad = list(specs)
            bad[at] = ([0, 1, 0], [1, 0])
            twice = dev.upload(ir.tables(bad, 4))
            used = dev.arena_stats()["used_bytes"]  # (with these tables' own block)
            try:
                for rows in (None, [0], []):
                    for tb in (0, 1):
                        with pytest.raises(ValueError, match="^scs_score_internode: a source tree has a taxon twice$"):
                            dev.score_internode(twice, rows=rows, batch_trees=tb)
                with pytest.raises(ValueError, match="^scs_debug_internode_depths: a source tree has a taxon twice$"):
                    dev.debug_internode_depths(twice)
                assert dev.arena_stats()["used_bytes"] == used
            finally:
                twice.free()
        # ... and the context is as usable as before
        _same(dev.score_internode(tabs, **ALL), ref, "after")
    finally:
        tabs.free()


def test_a_taxon_out_of_range_in_a_late_chunk_is_found_on_the_device(dev):
    # page-locked tables of this size return from the upload after their first 64 trees; the device's range check of
    # the rest is collected by the first export that reads them all -- before any sweep kernel runs
    n, m = 2100, 288
    bad = synthetic.make_tables(0, n, m, "one", pinned=True)
    bad.leaf_taxon[-5] = n + 3
    dtab = dev.upload(bad)
    try:
        used = dev.arena_stats()["used_bytes"]
        with pytest.raises(ValueError, match=r"a leaf_taxon entry is out of range \[0, n_taxa\)"):
            dev.score_internode(dtab, rows=[0])
        assert dev.arena_stats()["used_bytes"] == used
    finally:
        dtab.free()
    trees = [[[0, 1], 2], [1, [2, 3]], [0, 3]]
    tabs = dev.upload(ir.tables(ir.specs_of(trees), 4))
    try:
        _same(dev.score_internode(tabs, **ALL), ir.by_paths(trees, 4), "after")
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ API and CLI
@lru_cache(maxsize=None)
def _dcm():
    trees = load_trees(str(DATA / "dcm_source_trees.tre"))
    names: dict = {}
    for t in trees:
        for name in t.get_tip_names():
            names.setdefault(name, len(names))
    nested = [pr.from_treenode(t, names) for t in trees]
    return trees, list(names), ir.by_tables(ir.specs_of(nested), len(names))


def test_source_internode_distances_on_the_dcm_sources_as_trees_and_as_arrays(dev):
    trees, names, ref = _dcm()
    n = len(names)
    res = source_internode_distances(trees, squares=True, device=dev)
    assert res.taxa == names and res.rows.tolist() == list(range(n)) and "internode" in res.timings
    got = {k: getattr(res, k) for k in ir.KEYS}
    _same(got, ref, "dcm trees")
    ir.check_invariants(got, n, None, source_coverage(trees, pairs=True, device=dev).pair_trees)
    mean = res.mean
    seen = ref["pair_weight"] > 0
    assert np.array_equal(np.isnan(mean), ~seen & ~np.eye(n, dtype=bool)) and not mean.diagonal().any()
    assert np.array_equal(mean[seen], ref["dist_sum"][seen] / ref["pair_weight"][seen]) and mean[seen].min() >= 2
    assert res.missing_pairs == int((~seen).sum() - n) // 2 and res.complete is (res.missing_pairs == 0)
    var = res.variance
    assert (var[seen] >= 0).all() and np.isnan(var[~seen & ~np.eye(n, dtype=bool)]).all()
    arrays = source_internode_distances(load_tree_arrays(str(DATA / "dcm_source_trees.tre")), squares=True, device=dev)
    # (a TreeArrays numbers its taxa by name, the list by first appearance: the same numbers under that renaming)
    assert sorted(arrays.taxa) == sorted(names)
    order = [arrays.taxa.index(x) for x in names]
    _same({k: getattr(arrays, k)[np.ix_(order, order)] if k in ir.MATRICES else getattr(arrays, k)[order]
           for k in ir.KEYS}, ref, "dcm arrays")
    assert sorted(arrays.table().splitlines()) == sorted(res.table().splitlines())
    lean = source_internode_distances(trees, matrices=False, device=dev)
    assert lean.pair_weight is None and lean.taxon_sq is None and np.array_equal(lean.taxon_sum, ref["taxon_sum"])
    ids = [min(700, n - 1), 3, 0]
    part = source_internode_distances(trees, rows=[names[ids[0]], 3, names[0]], squares=True, device=dev)
    _same({k: getattr(part, k) for k in ir.KEYS}, {k: ref[k][ids] for k in ir.KEYS}, "dcm rows")
    assert part.missing_pairs is None and part.complete is None
    near = res.nearest(names[0], 5)
    assert [x["mean"] for x in near] == sorted(mean[0][seen[0]].tolist())[:5] and near[0]["weight"] >= 1
    doubled = source_internode_distances(trees, tree_weights=[2.0] * len(trees), device=dev)
    assert np.array_equal(doubled.dist_sum, 2 * ref["dist_sum"])
    # a supertree's own matrix: one tree, a tree metric on its taxa
    own = source_internode_distances([trees[0]], device=dev)
    assert own.complete and (own.pair_weight + np.eye(len(own.taxa), dtype=np.int64) == 1).all()


def test_the_command_line_writes_the_matrix_and_the_table(tmp_path):
    src = DATA / "supertriplets_source.tre"
    out, phy, tsv, other = (tmp_path / x for x in ("out.tre", "matrix.phy", "taxa.tsv", "other.tre"))
    api = source_internode_distances(load_tree_arrays(str(src)))
    args = ["-i", str(src), "-o", str(out), "--internode-out", str(phy), "--internode-taxa-out", str(tsv)]
    res = CliRunner().invoke(scs, args + ["--internode-missing", "-1"])
    assert res.exit_code == 0, res.output
    assert tsv.read_text() == api.table() and tsv.read_text().splitlines()[0].split("\t") == [
        "taxon", "partners", "weight", "sum", "mean"]
    lines = phy.read_text().splitlines()
    assert lines[0] == str(len(api.taxa)) and len(lines) == 1 + len(api.taxa)
    first = lines[1].split()
    assert first[0] == api.taxa[0] and len(first) == 1 + len(api.taxa) and float(first[1]) == 0.0
    mean = np.where(np.isnan(api.mean), -1.0, api.mean)
    assert np.allclose([float(x) for x in lines[2].split()[1:]], mean[1], atol=1e-6, rtol=0)
    if not api.complete:  # without a fill value a missing pair is an error that names one
        phy.unlink()
        res = CliRunner().invoke(scs, args)
        assert res.exit_code != 0 and "in no tree together" in (res.output + str(res.exception))
    # without the options: the files of before and no other
    before = sorted(p.name for p in tmp_path.iterdir())
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(other)])
    assert res.exit_code == 0 and sorted(p.name for p in tmp_path.iterdir()) == sorted([*before, "other.tre"])
