"""The block records as the build's preparation leaves them (``scs_debug_block_records``): for every (64-row block,
tree) the sorted positions, and for every pair of neighbours the value of the shallowest gap between them and the
position the record names for it -- which must be the LEFTMOST position of the minimum, what the halving search gave
before the argmin tables (``csrc/scs_build.hip``) replaced it.  W cannot show a wrong position of an equal minimum;
this can.  All three record kernels, against brute force (``tests/prep_reference.py``)."""

import build_reference as br
import numpy as np
import prep_reference as pr
import pytest

from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

KINDS = ("mono", "wide", "general")
INT_MAX = 0x7FFFFFFF


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


def _check(dev, tb, kind, row_begin=0, row_end=None, what=""):
    """Every (block, tree) record of the rows [row_begin, row_end) equals the brute-force record."""
    row_end = tb.n_taxa if row_end is None else row_end
    dtab = dev.upload(tb)
    try:
        got = dtab.block_records(kind, 0, tb.n_trees, row_begin, row_end)
    finally:
        dtab.free()
    n_blocks = (row_end - row_begin + br.TR - 1) // br.TR
    assert got["cnt"].shape == (n_blocks, tb.n_trees)
    ties = 0
    for b in range(n_blocks):
        lo, hi = row_begin + b * br.TR, min(row_end, row_begin + (b + 1) * br.TR)
        for t in range(tb.n_trees):
            ref = pr.record_reference(tb, t, lo, hi, by_depth=(kind == "general"))
            c, tag = ref["cnt"], f"{what} {kind} block {b} tree {t}"
            assert got["cnt"][b, t] == c, tag
            assert np.array_equal(got["spos"][b, t, :c], ref["spos"]) and (got["spos"][b, t, c:] == INT_MAX).all(), tag
            g = max(c - 1, 0)
            assert np.array_equal(got["gap"][b, t, :g], ref["gap"]), tag
            assert not got["gap"][b, t, g:].any(), tag
            bad = got["argpos"][b, t, :g] != ref["argpos"]
            assert not bad.any(), (f"{tag}: gaps {np.flatnonzero(bad)[:5].tolist()} name positions "
                                   f"{got['argpos'][b, t, :g][bad][:5]}, leftmost minima at {ref['argpos'][bad][:5]}")
            if kind == "general":
                assert np.array_equal(got["depth"][b, t, :g], ref["depth"]), tag
            if g:  # (how many of the gaps had a second position with the same minimum: the cases that tell)
                taxa, depth, value = pr.gap_arrays(tb, t)
                key = depth if kind == "general" else value
                ties += sum(int(np.count_nonzero(key[ref["spos"][k]:ref["spos"][k + 1]] == key[ref["argpos"][k]]) > 1)
                            for k in range(g))
    return ties


def _tables(arrays, strategy, kind):
    tb = br.tables(arrays, strategy)
    if kind == "general":
        tb.monotone = False
    return tb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["star", "caterpillar", "balanced", "random"])
def test_records_with_0_to_64_rows_present(dev, shape, kind):
    _check(dev, _tables(br.record_forest(shape), "branch", kind), kind, what=f"record {shape}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize(("strategy", "lengths"), [("one", "positive"), ("branch", "equal"), ("branch", "zero")])
@pytest.mark.parametrize("n", [130, 257])
def test_ties_name_the_leftmost_position(dev, n, strategy, lengths, kind):
    ties = _check(dev, _tables(br.tie_forest(n, lengths), strategy, kind), kind, what=f"ties {n} {strategy} {lengths}")
    assert ties > 0
    _check(dev, _tables(br.tie_forest(n, lengths), strategy, kind), kind, 63, 129, what=f"ties {n} rows [63, 129)")


@pytest.mark.parametrize("kind", KINDS)
def test_signed_lengths_general_and_value_minima(dev, kind):
    # (negative lengths: the general kernel's case; the monotone kernels still take minima over the values)
    _check(dev, br.tables(br.record_forest("random", "signed"), "branch"), kind, what="signed")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gaps", br.LEVEL_GAPS)
def test_table_levels_around_powers_of_two(dev, gaps, kind):
    _check(dev, _tables(br.level_forest(gaps), "branch", kind), kind, what=f"m={gaps}")


_BIG: dict = {}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("leaves", [br.SPARSE_FUSED_MAX_LEAVES, br.SPARSE_FUSED_MAX_LEAVES + 1])
def test_fused_and_per_level_tables(dev, leaves, kind):
    # (32 768 leaves: one workgroup builds all levels; one more: a launch per level)
    arrays = _BIG.setdefault(leaves, br.big_forest(leaves, True))
    rb, re_ = br.BIG_ROWS
    _check(dev, _tables(arrays, "branch", kind), kind, rb, re_, what=f"{leaves} leaves")


@pytest.mark.parametrize("kind", KINDS)
def test_star_trees_where_every_gap_is_equal(dev, kind):
    n = 300
    rng = np.random.RandomState(12)
    ids = np.arange(n, dtype=np.int32)
    trees = [("star", br.order_random(rng, ids)), ("star", br.order_random(rng, ids, 200)),
             ("star", br.order_random(rng, ids, 65)), ("star", br.order_random(rng, ids, 3))]
    tb = _tables(br.forest(12, n, trees), "one", kind)
    taxa, depth, value = pr.gap_arrays(tb, 0)
    assert len(np.unique(value[:-1])) == 1 and depth[-1] == 0  # every gap but the root's last one ties
    assert _check(dev, tb, kind, what="stars") > 0


def _spaced_forest(n, head, far, seed):
    """One tree of ``n`` leaves on ``n`` taxa: the rows 0 .. 63 - len(far) of block 0 lie among its first ``head``
    leaves, the other rows of the block at the leaf positions ``far`` (ascending, the last one n - 1)."""
    rng = np.random.RandomState(seed)
    k = 64 - len(far)
    order = br.order_random(rng, np.arange(64, n, dtype=np.int32))
    at = np.concatenate([np.sort(rng.permutation(head)[:k]), np.asarray(far[:-1], dtype=np.int64)])
    order = np.insert(order, at - np.arange(63), rng.permutation(63).astype(np.int32))
    order = np.concatenate([order, [63]]).astype(np.int32)
    assert far[-1] == n - 1 and len(order) == n and len(np.unique(order)) == n
    return br.forest(seed, n, [("random", order)])


def _far_forest():
    """140 000 leaves; the rows 0 .. 62 lie among the first 8 000 leaves, row 63 is the last leaf: the gap between the
    two last rows of block 0 spans at least 2^17 positions -- a query of level 17, above the 16-bit argmin levels."""
    return _spaced_forest(140000, 8000, [139999], 17)


@pytest.mark.parametrize("kind", KINDS)
def test_a_gap_of_2_to_the_17_between_rows(dev, kind):
    arrays = _BIG.setdefault("far", _far_forest())
    tb = _tables(arrays, "branch", kind)
    ref = pr.record_reference(tb, 0, 0, 64, by_depth=(kind == "general"))
    assert ref["cnt"] == 64 and ref["spos"][63] - ref["spos"][62] >= 1 << 17
    _check(dev, tb, kind, 0, 64, what="far")


@pytest.mark.parametrize("kind", KINDS)
def test_the_highest_argmin_levels_and_offsets_above_32767(dev, kind):
    """120 000 leaves; rows 61, 62 and 63 of block 0 are 48 000 and 70 000 positions apart: queries of levels 15 and 16,
    the highest the argmin table holds, and -- level 16 -- an offset that needs all 16 bits of an entry."""
    arrays = _BIG.setdefault("high", _spaced_forest(120000, 2000, [50000, 119999], 23))
    tb = _tables(arrays, "branch", kind)
    ref = pr.record_reference(tb, 0, 0, 64, by_depth=(kind == "general"))
    gaps = np.diff(ref["spos"])[-2:]
    assert ref["cnt"] == 64 and 1 << 15 <= gaps[0] < 1 << 16 <= gaps[1] < 1 << 17
    # the level-16 window the device reads the position from: the left one unless the right one's minimum is smaller
    a, b, at = int(ref["spos"][62]), int(ref["spos"][63]), int(ref["argpos"][62])
    window = a if at < a + (1 << 16) else b - (1 << 16)
    assert at - window >= 1 << 15, (a, b, at)
    _check(dev, tb, kind, 0, 64, what="high levels")
