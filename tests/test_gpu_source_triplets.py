"""Pairwise rooted-triplet terms of the sources on the device (``scs_score_source_pair_triplets``)
held exactly to the references of ``tests/source_triplets_reference.py``: few and no common taxa, the four states of a
triple, chains that collapse onto one set, polytomies that a restriction makes binary, overlaps around the word, the
wave, the workgroup and the pairs finished in the restrict kernel -- each with the default LDS and with the least that
holds one node's rows, which also sends the restriction through the pair's region --, node counts around the sweep's
block, sums past 2^32, 32-bit positions, chunks, batches, chosen rows, null outputs, the counts ``scs_score_triplets``
shares with it, the refusals, and the way through ``source_distances`` and the command line."""

import random
from functools import lru_cache
from math import comb
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest
import source_triplets_reference as st

from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, load_trees, source_distances
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.load import load_tree_arrays

pytestmark = pytest.mark.gpu

DATA = Path(__file__).parent / "golden" / "reference_data"


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what) -> None:
    for k in st.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        bad = got[k] != ref[k]
        assert not bad.any(), (what, k, np.argwhere(bad)[:6].tolist(), got[k][bad][:6], ref[k][bad][:6])


def _least_lds(tables, rows=None) -> int:
    """The max_lds_bytes that holds one node's two rows and no more: zb = 1, and no restriction fits the launch."""
    plan = backend.debug_source_pair_triplets_plan(tables.tree_off, int(tables.n_taxa), rows)
    tight = 16 * int(plan["words"].max())
    again = backend.debug_source_pair_triplets_plan(tables.tree_off, int(tables.n_taxa), rows, lds_bytes=tight)
    used = again["tile_rows"] > 0
    assert (again["zb"][used] == 1).all() and again["slab"][used].all()
    return tight


def _check(dev, trees, n_taxa, ref=None, rows=None, batches=(0,), lds=(0, None), chunks=(0,), what="",
           tables=None) -> dict:
    """Every setting against the reference; the full matrix also against the invariants.  An LDS of None stands for
    the least that the plan accepts."""
    tables = pr.tables(trees, n_taxa) if tables is None else tables
    if ref is None:
        ref = st.by_sets(trees, rows) if max(np.diff(tables.tree_off)) <= 12 else st.quadratic(trees, rows)
    tabs = dev.upload(tables)
    try:
        for bt in batches:
            for cap in lds:
                cap = _least_lds(tables, rows) if cap is None else cap
                for ch in chunks:
                    got = dev.score_source_pair_triplets(tabs, rows, batch_trees=bt, lds_bytes=cap, chunk_pairs=ch)
                    _same(got, ref, (what, bt, cap, ch))
                    if rows is None:
                        st.check_invariants(got)
    finally:
        tabs.free()
    return ref


# ------------------------------------------------------------------------------------------------ few common taxa
def test_zero_to_three_common_taxa_and_trees_of_one_and_two_leaves(dev):
    trees = [[[0, 1], [2, [3, 4]]],      # 0
             [[5, 6], [7, 8]],           # 1: disjoint from 0
             [[0, 5], [9, 10]],          # 2: one taxon of 0, one of 1
             [[0, 1], [6, 7]],           # 3: two of 0, two of 1
             [[0, [1, 2]], [5, 11]],     # 4: three of 0, resolved 12|0 where 0 has 01|2
             [[0, 1], 2],                # 5: three of 0, resolved alike (and A ⊂ B)
             3,                          # 6: one leaf
             [3, 4],                     # 7: two leaves
             [[0, 1], [2, [3, 4]]],      # 8: identical to 0
             [0, 1, 2],                  # 9: three of 0 as a fan
             [2, 1, 0, 11]]              # 10: a fan again
    ref = _check(dev, trees, 12, batches=(0, 1, 3), chunks=(0, 1))
    assert np.array_equal(ref["common"], st.quadratic(trees)["common"])
    assert ref["common"][0].tolist() == [5, 0, 1, 2, 3, 3, 1, 2, 5, 3, 3]
    cell = lambda a, b: tuple(int(ref[k][a, b]) for k in st.KEYS[1:])  # noqa: E731
    assert cell(0, 5) == (1, 1, 1)      # resolved alike
    assert cell(0, 4) == (1, 1, 0)      # resolved differently
    assert cell(0, 9) == (1, 0, 0)      # one side a fan
    assert cell(9, 10) == (0, 0, 0)     # both sides fans
    assert cell(0, 8) == cell(0, 0) == (10, 10, 10) and cell(1, 1) == (4, 4, 4)
    assert cell(0, 1) == cell(0, 3) == cell(6, 0) == cell(0, 7) == (0, 0, 0)


def test_hand_made_pairs(dev):
    # ((a,b),(c,d)) resolves all four triples, the caterpillar (((a,b),c),d) too; they agree on ab|c and ab|d only.
    # ((a,c),(b,d)) shares nothing with the first and ac|d with the second; ((a,b,c),d) leaves abc a fan
    trees = [[[0, 1], [2, 3]], [[[0, 1], 2], 3], [[0, 2], [1, 3]], [[0, 1, 2], 3]]
    tabs = dev.upload(pr.tables(trees, 4))
    try:
        got = dev.score_source_pair_triplets(tabs)
    finally:
        tabs.free()
    assert got["triplets"].tolist() == [[4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 4, 4], [3, 3, 3, 3]]
    assert got["triplets_shared"].tolist() == [[4, 2, 0, 1], [2, 4, 1, 3], [0, 1, 4, 1], [1, 3, 1, 3]]
    assert got["common"].tolist() == [[4] * 4] * 4 and np.array_equal(got["triplets"], got["triplets_other"].T)


# ------------------------------------------------------------------------------------------------ basic shapes
def test_identical_trees_stars_and_caterpillars(dev):
    rng = random.Random(7)
    n = 150
    order = list(range(n))
    rng.shuffle(order)
    binary = pr.rand_tree(range(n), 2, rng)
    half = n // 2

    def balanced(leaves):
        return leaves[0] if len(leaves) == 1 else [balanced(leaves[: len(leaves) // 2]),
                                                   balanced(leaves[len(leaves) // 2:])]

    trees = [binary, binary, list(range(n)), list(range(n - 1, -1, -1)), pr.caterpillar(range(n), True),
             pr.caterpillar(range(n), False), balanced(list(range(n))), pr.caterpillar(order[:97], True),
             pr.rand_tree(order[20:], 9, rng), [binary, [pr.caterpillar(range(n, n + half)), n + half]]]
    ref = _check(dev, trees, n + half + 1, batches=(0, 4))
    all_of = lambda a, b: {int(ref[k][a, b]) for k in st.KEYS[1:]}  # noqa: E731
    assert all_of(0, 1) == {comb(n, 3)} and all_of(0, 9) == {comb(n, 3)} and all_of(2, 3) == {0}
    assert ref["triplets"][4, 5] == ref["triplets_other"][4, 5] == comb(n, 3)
    # (the left and the right caterpillar agree on no triple; the balanced tree on some with either)
    assert ref["triplets_shared"][4, 5] == 0 and 0 < ref["triplets_shared"][4, 6] < comb(n, 3)
    assert ref["triplets"][2].max() == 0 and ref["triplets_other"][0, 2] == 0 and ref["triplets_shared"][:, 2].max() == 0


# ------------------------------------------------------------------------------------------------ distinctness
def test_a_restriction_collapses_chains_and_makes_polytomies_binary(dev):
    trees = [[[[[[0, 9], 1], 8], 7], [2, 3]],       # {0,1} sits on three nodes once 7, 8, 9 are gone
             [[0, 1], [2, 3]],
             [[[[[0, 1]]], [[2, 3]]]],              # unary chains above the root's children and inside
             [[0, 2], [1, 3]],
             [[[[0, 9], 8], 7], 1, 2],              # the common leaves of a node all sit in one child
             [[0, 1], [2, 3], [8, 9]],              # three children, two of them with common leaves: binary
             [[0, 1, 8], [2, 9, 3], 7],             # polytomies that lose a leaf each
             [[[0, 7], [1, 8]], [[2, 9], 3]]]       # every node keeps one leaf of two
    ref = _check(dev, trees, 10, batches=(0, 2), chunks=(0, 3))
    assert np.array_equal(ref["triplets"], st.quadratic(trees)["triplets"])
    assert ref["triplets"][0, 1] == 4 and ref["triplets_shared"][0, 1] == 4 and ref["triplets_shared"][2, 1] == 4
    assert ref["triplets"][4, 1] == 0 and ref["triplets"][5, 1] == 4 and ref["triplets_shared"][5, 1] == 4
    assert ref["triplets_shared"][0, 3] == 0 and ref["triplets_shared"][7, 1] == 4


def test_depths_past_16_bits_in_small_trees(dev):
    # a chain of unary nodes above a clade is as deep as it likes
    rng = random.Random(4)
    trees = [pr.rand_tree(rng.sample(range(90), 70), 3, rng) for _ in range(4)]
    tables = pr.tables(trees, 90)
    off = tables.tree_off
    tables.adj_depth[off[1]:off[2]] += 1 << 20
    deep = tables.adj_depth[off[2]:off[3]]
    deep[deep >= 2] += 70000
    ref = _check(dev, trees, 90, ref=st.quadratic(trees), tables=tables, what="deep")
    assert ref["triplets_shared"][1, 2] > 0 and 50 < ref["common"][1, 2] < 70


# ------------------------------------------------------------------------------------------------ words, waves, blocks
def _overlap_pair(c: int, seed: int, arity: int = 4):
    """Two trees with exactly c common taxa (and a few of their own) that agree on some triples and not on others: the
    second is the first restricted to the common taxa, a tenth of them swapped among themselves, beside taxa of its
    own."""
    rng = random.Random(seed)
    extra = max(3, c // 10)
    a = pr.rand_tree(range(c + extra), arity, rng)
    moved = rng.sample(range(c), max(2, c // 10))
    to = dict(zip(moved, moved[1:] + moved[:1]))

    def swapped(tree):
        return [swapped(x) for x in tree] if isinstance(tree, list) else to.get(tree, tree)

    b = [swapped(pr.restrict(a, set(range(c)))), pr.rand_tree(range(c + extra, c + 2 * extra), 3, rng)]
    return [a, b], c + 2 * extra


@pytest.mark.parametrize("c", [31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_overlaps_around_the_word_the_wave_the_workgroup_and_the_small_pairs(dev, c):
    # (63 and 64 common taxa are finished in the restrict kernel, by what the device finds: both trees are larger)
    trees, n = _overlap_pair(c, 500 + c)
    ref = _check(dev, trees, n, ref=st.quadratic(trees), what=c)
    assert ref["common"][0, 1] == c and 0 < ref["triplets_shared"][0, 1] < ref["triplets"][0, 1] < comb(c, 3)
    plan = backend.debug_source_pair_triplets_plan(pr.tables(trees, n).tree_off, n)
    assert plan["small_common"] == 64 and (plan["max_common"][0, 0] > 64) == (c > 60)


def test_pairs_the_host_knows_to_be_small(dev):
    rng = random.Random(64)
    base = pr.rand_tree(range(80), 3, rng)
    trees = [pr.restrict(base, set(range(64))), pr.rand_tree(range(64), 3, rng), pr.rand_tree(range(65), 4, rng),
             pr.restrict(base, set(range(3, 68))), pr.rand_tree(range(10, 74), 2, rng)]
    tables = pr.tables(trees, 80)
    assert np.diff(tables.tree_off).tolist() == [64, 64, 65, 65, 64]
    plan = backend.debug_source_pair_triplets_plan(tables.tree_off, 80)
    assert plan["chunks"][:, 3:7].tolist() == [[25, 12, 10, 6]]  # (three pairs of 65 leaves: 2 workgroups each)
    ref = _check(dev, trees, 80, ref=st.quadratic(trees), tables=tables, what="small")
    assert ref["common"][2, 3] == 62 and ref["common"][2, 2] == 65 and ref["triplets_shared"][0, 3] == ref["triplets"][0, 3]


@pytest.mark.parametrize("blocks,more", [(1, -1), (1, 0), (1, 1), (2, 1)], ids=["zb - 1", "zb", "zb + 1", "2 zb + 1"])
def test_b_node_counts_around_the_block_of_a_sweep_workgroup(dev, blocks, more):
    c, n = 100, 110
    rng = random.Random(10 * blocks + more)
    a = pr.rand_tree(range(n), 3, rng)
    zb = int(backend.debug_source_pair_triplets_plan(np.array([0, n, n + c], dtype=np.int64), n)["zb"][0, 0])
    k = blocks * zb + more
    assert zb == 32
    order = rng.sample(range(c), c)
    b = [pr.caterpillar(order[: k + 1]), *order[k + 1:]]  # k nodes below the root, the other leaves under the root
    ref = _check(dev, [a, b], n, ref=st.quadratic([a, b]), what=k)
    assert ref["triplets_other"][0, 1] == sum(comb(s, 2) * ((s + 1 if s <= k else c) - s) for s in range(2, k + 2))
    assert ref["triplets_shared"][0, 1] > 0


# ------------------------------------------------------------------------------------------------ past 2^32, mid size
def test_caterpillars_of_3000_leaves_count_past_32_bits(dev):
    n = 3000
    trees = [pr.caterpillar(range(n), True), pr.caterpillar(range(n), True), list(range(n))]
    total = comb(n, 3)
    assert total == 4_495_501_000 > 1 << 32
    ref = {k: np.zeros((3, 3), dtype=np.int64) for k in st.KEYS}
    ref["common"] = np.full((3, 3), n, dtype=np.int32)
    ref["triplets"][:2] = total
    ref["triplets_other"][:, :2] = total
    ref["triplets_shared"][:2, :2] = total
    _check(dev, trees, n, ref=ref, what="caterpillars")


@lru_cache(maxsize=None)
def _mid_case():
    trees, n = _overlap_pair(4097, 41)
    return trees, n, st.pair_quadratic(*trees)


def test_a_pair_of_4097_common_taxa(dev):
    trees, n, (c, ta, tb, ts) = _mid_case()
    assert c == 4097 and 0 < ts < min(ta, tb)
    tabs = dev.upload(pr.tables(trees, n))
    try:
        for cap in (0, 16 * ((4097 + 409 >> 5) + 1)):
            got = dev.score_source_pair_triplets(tabs, rows=[0, 1], lds_bytes=cap)
            assert [int(got[k][0, 1]) for k in st.KEYS] == [c, ta, tb, ts], cap
            assert [int(got[k][1, 0]) for k in st.KEYS] == [c, tb, ta, ts], cap
            assert got["triplets"][0, 0] == got["triplets_other"][0, 0] == got["triplets_shared"][0, 0] > ta
    finally:
        tabs.free()


def test_positions_past_16_bits(dev):
    # two trees of 65 536 leaves that share 100 taxa, and a tree of 4 097 leaves inside the first
    rng = random.Random(65536)
    n = 65536
    a = pr.rand_tree(range(n), 3, rng)
    shared = rng.sample(range(n), 100)
    b = pr.rand_tree([*shared, *range(n, 2 * n - 100)], 3, rng)
    inside = rng.sample(range(n), 4097)
    small = pr.rand_tree(inside, 3, rng)
    tables = pr.tables([a, b, small], 2 * n - 100)
    assert np.diff(tables.tree_off).tolist() == [n, n, 4097]
    want_b = st.pair_quadratic(pr.restrict(a, set(shared)), pr.restrict(b, set(shared)))
    want_s = st.pair_quadratic(pr.restrict(a, set(inside)), small)
    assert want_b[0] == 100 and want_s[0] == 4097 and want_b[3] > 0 and want_s[3] > 0
    tabs = dev.upload(tables)
    try:
        got = dev.score_source_pair_triplets(tabs, rows=[1, 2])
        assert [int(got[k][0, 0]) for k in st.KEYS] == [100, want_b[2], want_b[1], want_b[3]]
        assert [int(got[k][1, 0]) for k in st.KEYS] == [4097, want_s[2], want_s[1], want_s[3]]
        assert got["common"][:, :2].tolist() == [[100, n], [4097, len(set(inside) & set(shared))]]
        assert got["common"][1, 2] == 4097 and got["triplets"][0, 1] == got["triplets_shared"][0, 1] > want_b[2]
        got = dev.score_source_pair_triplets(tabs, rows=[0], batch_trees=1, outputs=("common", "triplets_other"))
        assert got["triplets"] is None and got["common"][0].tolist()[:2] == [n, 100]
        assert got["triplets_other"][0, 1:].tolist() == [want_b[2], want_s[2]]
    finally:
        tabs.free()


# ------------------------------------------------------------------------------------------------ chunks, batches, rows
@lru_cache(maxsize=None)
def _mixed_case():
    rng = random.Random(77)
    n = 700
    sizes = [700, 3, 130, 1, 515, 64, 2]
    trees = [pr.rand_tree(rng.sample(range(n), s), rng.choice([2, 3, 6]), rng) for s in sizes]
    trees = [t[0] if len(t) == 1 else t for t in trees]
    return trees, n, pr.tables(trees, n), st.quadratic(trees)


def test_chunks_and_batches_give_the_same_counts(dev):
    trees, n, tables, ref = _mixed_case()
    _check(dev, trees, n, ref=ref, tables=tables, batches=(1, 2, 0), chunks=(1, 2, 7, 0), lds=(0,), what="mixed")
    _check(dev, trees, n, ref=ref, tables=tables, batches=(2, 0), chunks=(2, 0), lds=(None, 4096), what="mixed lds")
    plan = backend.debug_source_pair_triplets_plan(tables.tree_off, n, batch_trees=2, chunk_pairs=2)
    assert plan["bstart"].tolist() == [0, 2, 4, 6, 7] and len(plan["chunks"]) == 7 + 5 + 3 + 1


def test_rows_as_a_subset_reordered_repeated_and_empty(dev):
    trees, n, tables, ref = _mixed_case()
    for rows in ([4], [6, 0, 3], [2, 2, 5, 0, 2], list(range(7)), list(range(6, -1, -1))):
        want = {k: ref[k][rows] for k in st.KEYS}
        _check(dev, trees, n, ref=want, rows=rows, tables=tables, batches=(0, 3), chunks=(0, 3), lds=(0,), what=rows)
    tabs = dev.upload(tables)
    try:
        got = dev.score_source_pair_triplets(tabs, rows=[])
        assert got["common"].shape == (0, 7) and got["triplets_shared"].shape == (0, 7)
    finally:
        tabs.free()


def test_null_outputs_are_left_out(dev):
    trees, n, tables, ref = _mixed_case()
    tabs = dev.upload(tables)
    try:
        for given in ((), ("triplets_shared",), ("common",), ("triplets",), ("triplets_other",),
                      ("common", "triplets", "triplets_other"), ("common", "triplets", "triplets_shared"),
                      ("common", "triplets_other", "triplets_shared"), ("triplets", "triplets_other", "triplets_shared"),
                      st.KEYS):
            for rows in (None, [5, 0]):
                got = dev.score_source_pair_triplets(tabs, rows, batch_trees=3, outputs=given)
                for k in st.KEYS:
                    if k in given:
                        assert np.array_equal(got[k], ref[k] if rows is None else ref[k][rows]), (given, rows, k)
                    else:
                        assert got[k] is None
    finally:
        tabs.free()


def test_300_small_trees_mirrored_and_with_chosen_rows(dev):
    rng = random.Random(300)
    kinds = [pr.rand_tree(rng.sample(range(14), rng.randint(1, 14)), 3, rng) for _ in range(30)]
    kinds = [t[0] if len(t) == 1 else t for t in kinds]
    small = st.quadratic(kinds)
    assert np.array_equal(small["triplets_shared"], st.by_sets(kinds)["triplets_shared"])
    pick = [rng.randrange(30) for _ in range(300)]
    ref = {k: small[k][np.ix_(pick, pick)] for k in st.KEYS}
    trees = [kinds[i] for i in pick]
    _check(dev, trees, 14, ref=ref, batches=(0, 128), chunks=(0, 1000), what="300 trees")
    rows = list(range(299, -1, -1))  # (chosen rows: every one of the 90 000 cells from its own workgroup)
    _check(dev, trees, 14, ref={k: ref[k][rows] for k in st.KEYS}, rows=rows, lds=(0,), what="300 rows")


def test_a_tree_over_all_taxa_scores_like_the_supertree_export(dev):
    rng = random.Random(14)
    n = 400
    sup = pr.rand_tree(range(n), 4, rng)
    trees = [pr.rand_tree(rng.sample(range(n), rng.randint(1, n)), 3, rng) for _ in range(25)]
    trees = [t[0] if len(t) == 1 else t for t in trees]
    parent, taxon = pr.preorder_arrays(sup)
    tabs = dev.upload(pr.tables([*trees, sup], n))
    try:
        got = dev.score_source_pair_triplets(tabs, rows=[25], batch_trees=6)
    finally:
        tabs.free()
    tabs = dev.upload(pr.tables(trees, n))
    try:
        want = dev.score_triplets(tabs, parent, taxon)
    finally:
        tabs.free()
    assert np.array_equal(got["triplets"][0, :25], want["t_super"])
    assert np.array_equal(got["triplets_other"][0, :25], want["t_source"])
    assert np.array_equal(got["triplets_shared"][0, :25], want["t_shared"]) and want["t_shared"].sum() > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_messages(dev):
    who = "scs_score_source_pair_triplets: "
    tabs = dev.upload(pr.tables([[[0, 1], 2], [[1, 2], 3], [0, 3]], 4))
    twice = dev.upload(pr.tables([[[0, 1], 2], [[0, 1], 0]], 4))
    try:
        for rows, said in (([3], r"rows\[0\] = 3 is not a tree of the tables \(3 trees\)"),
                           ([0, -1], r"rows\[1\] = -1 is not a tree")):
            with pytest.raises(ValueError, match=who + said):
                dev.score_source_pair_triplets(tabs, rows=rows)
        with pytest.raises(ValueError, match=who + "max_lds_bytes = -1 is negative"):
            dev.score_source_pair_triplets(tabs, lds_bytes=-1)
        with pytest.raises(ValueError, match=who + "max_chunk_pairs = -2 is negative"):
            dev.score_source_pair_triplets(tabs, chunk_pairs=-2)
        with pytest.raises(ValueError, match=who + "max_lds_bytes = 8 does not hold the bitset rows of trees of 3 and 3"):
            dev.score_source_pair_triplets(tabs, lds_bytes=8)
        lib, buf = dev._lib, np.zeros(9, dtype=np.int32)
        rows = np.zeros(3, dtype=np.int32)
        for n_rows, row_ptr, said in ((-1, rows.ctypes.data, b"n_rows = -1 is negative"),
                                      (2, None, b"rows is null and n_rows = 2 is not the 3 trees of the tables")):
            assert lib.scs_score_source_pair_triplets(dev._ctx, tabs._h, n_rows, row_ptr, 0, 0, 0, buf.ctypes.data,
                                                      None, None, None) == nv.EINVAL
            assert lib.scs_last_error() == who.encode() + said
        assert lib.scs_score_source_pair_triplets(dev._ctx, None, 0, None, 0, 0, 0, None, None, None, None) == nv.EINVAL
        assert lib.scs_last_error() == who.encode() + b"null argument"
        # a taxon twice in a tree: found on the device before a pair is counted, whichever rows are asked for
        for rows in (None, [0]):
            with pytest.raises(ValueError, match="^" + who + "a source tree has a taxon twice$"):
                dev.score_source_pair_triplets(twice, rows=rows)
        # the size refusal is the plan's, on the host: no tables of that size are made
        off = np.array([0, 327680, 2 * 327680, 2 * 327680 + 5], dtype=np.int64)
        with pytest.raises(ValueError, match="trees of 327680 and 327680 leaves may share more than the 327679 taxa"):
            backend.debug_source_pair_triplets_plan(off, 10)
        assert backend.debug_source_pair_triplets_plan(off - np.array([0, 1, 2, 2]), 10)["words"][0, 0] == 10240
        assert backend.debug_source_pair_triplets_plan(off, 10, rows=[2])["max_common"][0, 0] == 5
        # and a good call still works afterwards
        _same(dev.score_source_pair_triplets(tabs), st.by_sets([[[0, 1], 2], [[1, 2], 3], [0, 3]]), "after")
    finally:
        tabs.free()
        twice.free()


# ------------------------------------------------------------------------------------------------ API and CLI
def _dcm_reference(path):
    trees = load_trees(str(path))
    names: dict = {}
    for t in trees:
        for name in t.get_tip_names():
            names.setdefault(name, len(names))
    return trees, st.quadratic([pr.from_treenode(t, names) for t in trees])


def test_source_distances_with_triplets_on_the_dcm_sources_as_trees_and_as_arrays(dev):
    path = DATA / "dcm_source_trees.tre"
    trees, ref = _dcm_reference(path)
    res = source_distances(trees, device=dev, triplets=True)
    _same({k: getattr(res, k) for k in st.KEYS}, ref, "dcm trees")
    st.check_invariants({k: getattr(res, k) for k in st.KEYS})
    assert np.array_equal(res.triplet_distance, ref["triplets"] + ref["triplets_other"] - 2 * ref["triplets_shared"])
    # (the DCM sources are restrictions of one model tree: they agree wherever they overlap)
    assert res.triplets_shared.any() and not res.triplet_distance.any() and "triplets" in res.timings
    plain = source_distances(trees, device=dev)
    assert plain.triplets is None and np.array_equal(plain.shared, res.shared) and "triplets" not in plain.timings
    arrays = source_distances(load_tree_arrays(str(path)), device=dev, triplets=True)
    _same({k: getattr(arrays, k) for k in st.KEYS}, ref, "dcm arrays")
    rows = [7, 0, 30]
    part = source_distances(load_tree_arrays(str(path)), rows=rows, device=dev, triplets=True)
    _same({k: getattr(part, k) for k in st.KEYS}, {k: ref[k][rows] for k in st.KEYS}, "dcm rows")
    mean, comparable = res.mean_distance(by="triplets")
    assert comparable.max() > 0 and np.nanmax(mean) == 0.0 and res.table() == arrays.table()
    assert res.table().splitlines()[0].endswith("\ttriplet_distance\tnormalized_triplet_distance")
    assert [line.split("\t")[:8] for line in res.table().splitlines()] == [line.split("\t") for line in
                                                                          plain.table().splitlines()]


def test_the_command_line_adds_the_triplet_columns(tmp_path):
    src = DATA / "supertriplets_source.tre"
    out, pairs, plain = (tmp_path / x for x in ("out.tre", "pairs.tsv", "plain.tsv"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--source-distances-out", str(pairs),
                                   "--source-triplets"])
    assert res.exit_code == 0, res.output
    api = source_distances(load_trees(str(src)), triplets=True)
    assert pairs.read_text() == api.table() and len(pairs.read_text().splitlines()) > 1
    assert pairs.read_text().splitlines()[0].split("\t")[8:] == ["triplets_a", "triplets_b", "triplets_shared",
                                                                 "triplet_distance", "normalized_triplet_distance"]
    assert (api.triplet_distance > 0).any()
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--source-distances-out", str(plain)])
    assert res.exit_code == 0 and plain.read_text() == source_distances(load_trees(str(src))).table()
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--source-triplets"])
    assert res.exit_code != 0 and "--source-triplets needs --source-distances-out" in res.output
