"""``tests/prep_reference.py`` -- the argmin table's build rule and query as the device runs them -- against brute
force: the query's position is the LEFTMOST position of the minimum, which is also what the halving search gives.
No GPU."""

from __future__ import annotations

import numpy as np
import pytest

import prep_reference as pr


@pytest.mark.parametrize("m", pr.SIZES)
def test_query_is_leftmost_argmin(m):
    rng = np.random.RandomState(m)
    pairs = pr.pairs_for(m, rng)
    patterns = pr.value_patterns(m, rng)
    assert {"random", "all_equal", "signed_zeros"} <= set(patterns)
    assert m < 3 or any(name.startswith("twin_minima_at_") for name in patterns)
    for name, values in patterns.items():
        val, off = pr.build_tables(values)
        assert len(val) == len(off) == pr.levels_for(m)
        for k in range(1, len(off)):
            assert off[k].min() >= 0 and off[k].max() < (1 << k), (name, k)
        for a, b in pairs:
            g, at = pr.query(val, off, a, b)
            g_ref, at_ref = pr.brute(values, a, b)
            assert g == g_ref and at == at_ref, (name, a, b, at, at_ref)
            assert values[at] == g


@pytest.mark.parametrize("m", [m for m in pr.SIZES if m <= 65])
def test_halving_search_gives_the_same_position(m):
    rng = np.random.RandomState(100 + m)
    for name, values in pr.value_patterns(m, rng).items():
        val, off = pr.build_tables(values)
        for a, b in pr.pairs_for(m, rng):
            assert pr.halving_position(val, a, b) == pr.query(val, off, a, b)[1], (name, a, b)


def test_level_values_are_the_window_minima():
    rng = np.random.RandomState(7)
    values = rng.random_sample(200)
    val, off = pr.build_tables(values)
    for k in range(len(val)):
        for p in range(len(val[k])):
            g, at = pr.brute(values, p, p + (1 << k))
            assert val[k][p] == g and p + off[k][p] == at


def test_signed_zero_ties_go_left():
    values = np.asarray([1.0, 0.0, -0.0, 0.0, 2.0, -0.0])
    val, off = pr.build_tables(values)
    assert pr.query(val, off, 0, 6)[1] == 1 and pr.query(val, off, 2, 6)[1] == 2
    assert pr.brute(values, 0, 6)[1] == 1 and pr.halving_position(val, 0, 6) == 1
