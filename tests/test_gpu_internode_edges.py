"""``scs_score_internode`` at the gates of its own plan: items of one and of two tiles with
chosen rows and matrices, with one staging chunk and with two, under mirror with a short last group, on real trees of
thousands of leaves; 1 023 | 1 024 | 1 025 trees and tree batches that start inside a word and need a second chunk;
the mirror gate on one input; polytomy runs of 2^k - 1, 2^k and 2^k + 1 at a tree's ends and middle; trees on wave
boundaries of the depth pass; rounds of pointer doubling per batch; depths of a neighbouring tree and the entry at a
tree's last leaf; a weight-0 tree that holds a taxon twice.  Every comparison is ``np.array_equal`` on every output
asked for, against ``internode_reference.by_tables`` and the judges of ``tests/internode_edge_reference.py``; the named
numbers of every case are proved in ``tests/test_internode_edge_reference_cpu.py``."""

import random
from functools import lru_cache

import internode_edge_reference as er
import internode_reference as ir
import numpy as np
import pytest

from spectralclustersupertree_amd import backend
from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

ALL = {"matrices": True, "squares": True}
DEPTHS = ("gap_r", "leaf_depth", "tree_height")


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what, asked=None) -> None:
    """Every output asked for (all that are not None when ``asked`` is not given) equals the reference's."""
    if asked is not None:
        assert [k for k in ir.KEYS if got[k] is not None] == [k for k in ir.KEYS if k in asked], what
    for k in ir.KEYS:
        if got[k] is None:
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:6].tolist(), got[k][got[k] != ref[k]][:6],
                               ref[k][got[k] != ref[k]][:6])


def _check(dev, specs, n, rows=None, weights=None, row_batches=(0,), tree_batches=(0,), what="") -> dict:
    """All seven outputs and the lean call against ``by_tables`` under every batch setting, the row sums against
    ``by_edges``, the invariants.  Returns the last full answer."""
    ref = ir.by_tables(specs, n, weights, rows)
    edges = er.by_edges(specs, n, weights)
    ids = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    assert ref["pair_weight"].any() and ref["dist_sum"].any(), what
    for k in ("taxon_weight", "taxon_sum"):
        assert np.array_equal(ref[k], edges[k][ids]), (what, k, "the references")
    tabs = dev.upload(ir.tables(specs, n))
    full = None
    try:
        for rb in row_batches:
            for tb in tree_batches:
                at = (what, rb, tb)
                full = dev.score_internode(tabs, rows, weights, batch_rows=rb, batch_trees=tb, **ALL)
                _same(full, ref, at, asked=ir.KEYS)
                ir.check_invariants(full, n, rows)
                lean = dev.score_internode(tabs, rows, weights, matrices=False, squares=True, batch_rows=rb,
                                           batch_trees=tb)
                _same(lean, ref, (*at, "no matrices"), asked=(*ir.SUMS, "taxon_partners"))
    finally:
        tabs.free()
    return full


def _depths(dev, specs, n, batches=(0,), tables=None) -> dict:
    ref = ir.depths_by_tables(specs)
    tabs = dev.upload(ir.tables(specs, n) if tables is None else tables)
    try:
        for tb in batches:
            got = dev.debug_internode_depths(tabs, batch_trees=tb)
            for k in DEPTHS:
                bad = np.flatnonzero(got[k] != ref[k])
                assert got[k].dtype == np.int32 and len(bad) == 0, (k, tb, bad[:8].tolist(), got[k][bad[:8]],
                                                                    ref[k][bad[:8]])
    finally:
        tabs.free()
    return ref


# ------------------------------------------------------------------------------------------------ tiles of an item
TWO = ("pair_weight", "dist_sum", "taxon_weight", "taxon_sum", "taxon_sq", "taxon_partners")


@lru_cache(maxsize=None)
def _tg_reference(n_trees: int) -> dict:
    specs, n, rows = er.case_tg_rows()
    return ir.by_tables(specs[:n_trees], n, None, rows)


@pytest.mark.parametrize("n_trees", [1100, 1000])
@pytest.mark.parametrize("n_rows", [5461, 5462])
def test_items_of_one_and_of_two_tiles_with_chosen_rows_and_matrices(dev, n_rows, n_trees):
    """600 taxa in 3 tiles: 5 461 rows give items of one tile (3 a row), 5 462 items of two (2 a row, the second a
    single tile).  1 100 trees are two staging chunks (32 + 3 words: every tile restages), in batches of 1 000 one
    chunk each (32 and 4 words, the second from the middle of word 31); the first 1 000 trees alone are one chunk,
    staged once for both tiles of an item.  Two matrices of 5 462 x 600 cells; every row and cell is judged."""
    specs, n, rows = er.case_tg_rows()
    specs, rows = specs[:n_trees], rows[:n_rows]
    ref = {k: v[:n_rows] for k, v in _tg_reference(n_trees).items()}
    p = backend.debug_internode_plan(er.off_of(specs), n, n_rows=n_rows, matrices=2)
    assert (p["tiles_per_item"], p["items_per_row"]) == ((1, 3) if n_rows == 5461 else (2, 2)) and p["mirror"] == 0
    assert er.batch_chunks(p)[0][0] == (2 if n_trees == 1100 else 1)
    lone = [i for i, a in enumerate(rows) if a in (592, 593, 594, 595, 596, 597)]
    assert len(lone) > 20 and ref["pair_weight"].any() and not ref["pair_weight"][lone].any()
    assert ref["pair_weight"][0, 0] >= 1 and ref["dist_sum"][1, n - 1] >= 2  # (rows 0 and 1 are taxa n - 1 and 0)
    tabs = dev.upload(ir.tables(specs, n))
    try:
        for tb in (0, 1000) if n_trees == 1100 else (0,):
            got = dev.score_internode(tabs, rows, outputs=TWO, batch_trees=tb)
            _same(got, ref, (n_rows, n_trees, tb), asked=TWO)
            for part in (slice(0, 600), slice(n_rows - 600, n_rows)):  # (the invariants need rows x rows cells)
                ir.check_invariants({k: None if v is None else v[part] for k, v in got.items()}, n, rows[part])
        lean = dev.score_internode(tabs, rows, matrices=False, squares=True)
        _same(lean, ref, (n_rows, n_trees, "no matrices"), asked=(*ir.SUMS, "taxon_partners"))
    finally:
        tabs.free()


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_mirror_with_items_of_one_and_of_two_tiles(dev, n):
    """Every row, so only the cells right of the row taxon are swept: 8 tiles in items of one at 2 047 taxa, in
    items of two at 2 048, 9 tiles in 5 items at 2 049 (the last one tile).  A row taxon from 255 on skips the first
    tile of its first item, so the second one stages; the last rows skip whole items."""
    specs = er.case_mirror(n)
    p = backend.debug_internode_plan(er.off_of(specs), n, matrices=1)
    assert (p["tiles"], p["tiles_per_item"], p["items_per_row"], p["mirror"]) == \
        {2047: (8, 1, 8, 1), 2048: (8, 2, 4, 1), 2049: (9, 2, 5, 1)}[n]
    ref, edges = ir.by_tables(specs, n), er.by_edges(specs, n)
    assert ref["dist_sum"][n - 1, 0] >= 2 and ref["dist_sum"][0, n - 1] >= 2 and ref["pair_weight"][n - 2, 1] >= 1
    assert (ref["taxon_partners"] > 0).mean() > 0.5
    tabs = dev.upload(ir.tables(specs, n))
    try:
        lean = dev.score_internode(tabs, None, matrices=False, squares=True)
        _same(lean, ref, (n, "lean"), asked=(*ir.SUMS, "taxon_partners"))
        ir.check_invariants(lean, n)
        for k in ("taxon_weight", "taxon_sum"):
            assert np.array_equal(lean[k], edges[k]), (n, k, "by edges")
        one = dev.score_internode(tabs, None, outputs=["dist_sum"])
        _same(one, ref, (n, "dist_sum"), asked=["dist_sum"])
        ir.check_invariants(one, n)
        assert one["dist_sum"][n - 1, 0] == ref["dist_sum"][0, n - 1] > 0
    finally:
        tabs.free()


def test_mirror_with_items_of_four_tiles_on_trees_of_thousands_of_leaves(dev):
    """Ten composed trees of 2 000 ... 3 000 leaves over 3 000 taxa, weights 0 ... 3: 12 tiles in 3 items a row.
    Every row without matrices: the sums by ``by_edges``, the partners from the trees' members.  Eight rows with all
    three matrices: every cell by ``composed``."""
    trees, specs, n, w = er.case_real()
    p = backend.debug_internode_plan(er.off_of(specs), n)
    assert (p["tiles"], p["tiles_per_item"], p["items_per_row"], p["mirror"], p["levels"]) == (12, 4, 3, 1, 12)
    edges = er.by_edges(specs, n, w)
    member = np.zeros((len(specs), n), dtype=np.int64)
    for t, (taxa, _) in enumerate(specs):
        member[t, taxa] = w[t] > 0
    partners = ((member.T @ member) > 0).sum(axis=1) - (member.sum(axis=0) > 0)
    assert edges["taxon_sum"].min() > 0 and partners.min() > 0
    rows = [n - 1, 0, 255, 256, 1500, 2047, 2048, 2999, 0]
    cells = er.sum_rows(trees, n, rows, w)
    assert cells["dist_sum"][0, 0] >= 4 and cells["pair_weight"][1, n - 1] >= 2  # (tree 0 of weight 2, by hand)
    tabs = dev.upload(ir.tables(specs, n))
    try:
        lean = dev.score_internode(tabs, None, w, matrices=False)
        assert [k for k in ir.KEYS if lean[k] is not None] == ["taxon_weight", "taxon_sum", "taxon_partners"]
        for k in ("taxon_weight", "taxon_sum"):
            assert lean[k].dtype == np.int64 and np.array_equal(lean[k], edges[k]), k
        assert lean["taxon_partners"].dtype == np.int32 and np.array_equal(lean["taxon_partners"], partners)
        got = dev.score_internode(tabs, rows, w, **ALL)
        ref = dict(cells)
        ref.update({s: cells[k].sum(axis=1, dtype=np.int64) for s, k in zip(ir.SUMS, ir.MATRICES)})
        ref["taxon_partners"] = (cells["pair_weight"] > 0).sum(axis=1).astype(np.int32)
        _same(got, ref, "composed", asked=ir.KEYS)
        ir.check_invariants(got, n, rows)
        for k in ("taxon_weight", "taxon_sum"):
            assert np.array_equal(got[k], lean[k][rows]), k
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ chunks and words
@pytest.mark.parametrize("n_trees", [1023, 1024, 1025])
def test_tree_counts_around_a_staging_chunk(dev, n_trees):
    """32 | 33 words: the 1 025th tree is the first bit of a second chunk of one word."""
    specs, n = er.case_chunk_gate(n_trees)
    assert er.chunks(0, n_trees) == ((1, [32]) if n_trees < 1025 else (2, [32, 1]))
    got = _check(dev, specs, n, what=n_trees)
    if n_trees > 1023:  # taxon 69 only in tree 1 023, with 67
        assert got["taxon_partners"][69] == len(specs[1023][0]) - 1 and got["pair_weight"][69, 67] == 1
        assert got["pair_weight"][69, 68] == 0
    if n_trees > 1024:  # taxon 68 only in tree 1 024, with 67, which is in both trees and in no other
        assert got["taxon_partners"][68] == len(specs[1024][0]) - 1 and got["pair_weight"][68, 67] == 1
        assert got["taxon_partners"][67] == len({*specs[1023][0], *specs[1024][0]}) - 1
    chosen = _check(dev, specs, n, rows=[69, 0, 68, 67, 67, 1], what=(n_trees, "rows"))
    assert (chosen["taxon_weight"][:4] > 0).tolist() == [n_trees > 1023, True, n_trees > 1024, n_trees > 1023]


@pytest.mark.parametrize("n_trees,batch", [(2016, 1008), (2018, 1009), (1100, 33)])
def test_tree_batches_that_start_inside_a_word(dev, n_trees, batch):
    """Trees 1 008 ... 2 015 are words 31 ... 62, one chunk; trees 1 009 ... 2 017 are words 31 ... 63, and the
    second chunk is word 63 alone with trees 2 016 and 2 017 in it.  Batches of 33 of 1 100 trees start at every bit."""
    specs, n = er.case_mid_word(n_trees)
    p = backend.debug_internode_plan(er.off_of(specs), n, batch_trees=batch)
    assert er.batch_chunks(p)[1] == {1008: (1, [32]), 1009: (2, [32, 1]), 33: (1, [2])}[batch]
    got = _check(dev, specs, n, tree_batches=(batch, 0), what=(n_trees, batch))
    assert got["taxon_weight"][69] == len(specs[-1][0]) - 1 > 0 and got["taxon_partners"][69] == len(specs[-1][0]) - 1
    _check(dev, specs, n, rows=[69, 3, 69, 0], tree_batches=(batch,), what=(n_trees, batch, "rows"))


def test_the_mirror_gate_on_one_input(dev):
    """150 rows in one row batch are swept with mirror, in batches of 149 and 1 without: the same answer."""
    specs = er.random_specs(random.Random(5), 150, 45, 3, 60)
    n = 150
    off = er.off_of(specs)
    assert backend.debug_internode_plan(off, n, batch_rows=150, matrices=3)["mirror"] == 1
    assert backend.debug_internode_plan(off, n, batch_rows=149, matrices=3)["mirror"] == 0
    ref = ir.by_tables(specs, n)
    tabs = dev.upload(ir.tables(specs, n))
    try:
        answers = [dev.score_internode(tabs, None, batch_rows=rb, batch_trees=tb, **ALL)
                   for rb in (150, 149) for tb in (0, 3)]
    finally:
        tabs.free()
    for i, got in enumerate(answers):
        _same(got, ref, ("gate", i), asked=ir.KEYS)
        _same(got, answers[0], ("gate, one another", i), asked=ir.KEYS)
        ir.check_invariants(got, n)
    assert (ref["taxon_partners"] > 0).all()


# ------------------------------------------------------------------------------------------------ polytomy runs
@pytest.mark.parametrize("where", ["star", *er.RUN_PLACES])
def test_polytomy_runs_around_every_power_of_two(dev, where):
    """Runs of 2^k - 1, 2^k and 2^k + 1 equal gaps, k = 1 ... 10 (as stars: that many leaves), where the binary
    descents of ``k_in_links`` take their widest steps: through the depth pass, and through the export on 60 rows
    with the matrices and on every row without."""
    specs, n = er.run_specs(where)
    ref_d = _depths(dev, specs, n, batches=(0, 1, 4))
    if where == "star":
        assert ref_d["tree_height"].tolist() == [int(m > 1) for m in er.RUNS] and not ref_d["gap_r"].any()
    else:
        assert ref_d["tree_height"].min() >= 2 and ref_d["gap_r"].max() >= 3 - (where != "middle")
    rows = sorted({x for taxa, _ in specs[::3] for x in (taxa[0], taxa[len(taxa) // 2], taxa[-1])} | {0, n - 1})
    got = _check(dev, specs, n, rows=rows, tree_batches=(0, 7), what=where)
    if where == "star":
        assert np.array_equal(got["dist_sum"], 2 * got["pair_weight"])
        assert np.array_equal(got["sq_sum"], 2 * got["dist_sum"])
    if where in ("left", "right"):
        known = er.sum_rows([(taxa, er.polytomy_piece(r, where)) for (taxa, _), r in zip(specs, er.RUNS)], n, rows)
        for k in ir.MATRICES:
            assert np.array_equal(got[k], known[k]), (where, k, "composed")
    edges = er.by_edges(specs, n)
    tabs = dev.upload(ir.tables(specs, n))
    try:
        lean = dev.score_internode(tabs, None, matrices=False)
    finally:
        tabs.free()
    for k in ("taxon_weight", "taxon_sum"):
        assert np.array_equal(lean[k], edges[k]), (where, k)
    assert edges["taxon_sum"].any() and np.array_equal(lean["taxon_partners"][rows], got["taxon_partners"])


# ------------------------------------------------------------------------------------------------ the depth pass
@pytest.mark.parametrize("turn", ["left", "right", "mixed", "random"])
def test_trees_on_the_wave_boundaries_of_the_depth_pass(dev, turn):
    """Trees of 64, 128, 1, 63, 65, 1 and 64 leaves: waves of one tree (a wave maximum and one atomic) and waves of
    several (an atomic per lane), one-leaf trees between them whose height stays 0, a last wave of two lanes.  The
    deepest leaves of a caterpillar are its first two (lane 0) or its last two (lane 63)."""
    specs, n = er.case_waves(turn)
    ref = _depths(dev, specs, n, batches=(0, 1, 3))
    if turn != "random":
        assert ref["tree_height"].tolist() == [63, 127, 0, 62, 64, 0, 63]
        first = ref["leaf_depth"][:64]
        assert (first[0] if turn != "right" else first[63]) == 63 and first.argmax() == (62 if turn == "right" else 0)
    assert ref["tree_height"][2] == ref["tree_height"][5] == 0
    _check(dev, specs, n, tree_batches=(0, 1, 3), what=turn)


@pytest.mark.parametrize("which", ["deep_then_small", "parities"])
def test_rounds_of_pointer_doubling_per_batch(dev, which):
    """The table's levels are the call's, the rounds the batch's: a batch of 2 or 3 leaves after one of 300 (9 rounds,
    then 2), and batches of 3 and of 4 ... 7 leaves (2 and 3 rounds: the answer lies in either buffer)."""
    specs, n = er.case_rounds(which)
    sizes = [len(t) for t, _ in specs]
    assert {er.rounds(m) & 1 for m in sizes} == {0, 1}
    ref = _depths(dev, specs, n, batches=(1, 0, 2))
    assert ref["tree_height"].tolist() == [m - 1 for m in sizes]
    _check(dev, specs, n, tree_batches=(1, 0, 2), what=which)


def test_depths_of_other_trees_and_the_entry_at_a_last_leaf_do_not_leak(dev):
    """The min table is built over a batch's whole leaf array.  Every tree's depths raised by 0, 7 or 10^6 in varying
    order, and the entry at every tree's last leaf, which belongs to no gap, 0 or 2^31 - 1 (the upload refuses only
    negative entries, so that is the largest it accepts): every output as from the plain tables."""
    specs, n = er.case_leak()
    base = _check(dev, specs, n, what="plain")
    plain_depths = ir.depths_by_tables(specs)
    for turn in range(3):
        offsets = [(0, 7, 1000000)[(t + turn + (t // 5)) % 3] for t in range(len(specs))]
        assert set(offsets) == {0, 7, 1000000}
        for last in (0, er.INT32_MAX):
            tables = er.shifted(specs, offsets, last, n)
            assert tables.adj_depth.max() == max(last, 1000000 + max(max(g, default=0) for (_, g), o in
                                                                    zip(specs, offsets) if o == 1000000))
            ref = _depths(dev, specs, n, batches=(0, 2), tables=tables)
            assert all(np.array_equal(ref[k], plain_depths[k]) for k in DEPTHS)
            tabs = dev.upload(tables)
            try:
                for tb in (0, 2):
                    _same(dev.score_internode(tabs, None, batch_trees=tb, **ALL), base, (turn, last, tb), asked=ir.KEYS)
                _same(dev.score_internode(tabs, [89, 0, 5], **ALL), {k: v[[89, 0, 5]] for k, v in base.items()},
                      (turn, last, "rows"), asked=ir.KEYS)
            finally:
                tabs.free()


# ------------------------------------------------------------------------------------------------ weight 0
def test_a_tree_of_weight_0_that_holds_a_taxon_twice_is_still_refused(dev):
    """What the library does today: ``k_in_scatter`` flags a taxon twice in one tree whatever the tree's weight (the
    weight only keeps the tree's bits clear), so the call is refused although the tree counts for nothing."""
    good = ir.specs_of([[[0, 1], 2], [1, [2, 3]], [0, 3]])
    bad = [good[0], ([0, 1, 0], [1, 0]), good[2]]
    ref = ir.by_tables(good, 4, [1, 0, 1])
    tabs = dev.upload(ir.tables(good, 4))
    try:
        _same(dev.score_internode(tabs, None, [1, 0, 1], **ALL), ref, "weight 0", asked=ir.KEYS)
    finally:
        tabs.free()
    twice = dev.upload(ir.tables(bad, 4))
    try:
        used = dev.arena_stats()["used_bytes"]
        for tb in (0, 1):
            for w in ([1, 0, 1], [0, 0, 0], None):
                with pytest.raises(ValueError, match="^scs_score_internode: a source tree has a taxon twice$"):
                    dev.score_internode(twice, None, w, batch_trees=tb)
        assert dev.arena_stats()["used_bytes"] == used
    finally:
        twice.free()
    tabs = dev.upload(ir.tables(good, 4))
    try:
        _same(dev.score_internode(tabs, None, [1, 0, 1], **ALL), ref, "after", asked=ir.KEYS)
    finally:
        tabs.free()
    assert ref["pair_weight"].tolist() == [[0, 1, 1, 1], [1, 0, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]]
    # a good tree of weight 0 counts for nothing, in one tree batch and in several: taxa 39 and 38 are only in such
    # trees
    rng = random.Random(4800)
    n, w = 40, [3, 0, 1, 2, 0, 5, 1, 1, 4]
    specs = er.random_specs(rng, n - 2, 9, 2, 20, arity=4)
    specs[1] = (specs[1][0] + [n - 1], specs[1][1] + [0])
    specs[4] = ([n - 2] + specs[4][0], [0] + specs[4][1])
    got = _check(dev, specs, n, weights=w, tree_batches=(0, 1, 4), what="weights")
    assert not got["taxon_partners"][n - 2:].any() and not got["pair_weight"][:, n - 2:].any()
    kept = [s for s, k in zip(specs, w) if k]
    _same(_check(dev, kept, n, weights=[k for k in w if k], tree_batches=(0, 2), what="weight 0 removed"), got, "kept")
    alone = ir.by_tables([specs[1], specs[4]], n)  # (what the two trees would add: partners the others do not give)
    assert ((alone["pair_weight"] > 0) & (got["pair_weight"] == 0)).any()
