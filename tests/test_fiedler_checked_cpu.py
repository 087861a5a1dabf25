"""``scs._fiedler_checked``, the convergence ladder of the recursion, on a stub graph (no device): one call where the
first converges; the widest block and four times the iterations where it does not; the better of two stopped blocks
with a warning inside ``ACCEPT_RESIDUAL`` and ``ACCEPT_RESIDUAL_OVER_GAP``; ``RuntimeError`` outside either."""

import warnings

import numpy as np
import pytest

from spectralclustersupertree_amd import scs
from spectralclustersupertree_amd._native import ConvergenceError

TOL, MAX_ITER = 1e-13, 50


def _stats(resid, lam2=0.9, lam_next=0.8):
    return {"n_vertices": 300, "block": 4, "iterations": 7, "converged": 0, "lambda": [1.0, lam2],
            "lambda_next": lam_next, "resid": [0.0, resid]}


class _Graph:
    """``fiedler`` answers from a script: a stats dict converges with it, a float raises with that residual."""

    def __init__(self, script, upper=None):
        self.script, self.calls = list(script), []
        if upper is not None:
            self.upper = upper

    def fiedler(self, v0, tol, max_iter, block):
        self.calls.append((v0, tol, max_iter, block))
        step = self.script[len(self.calls) - 1]
        maps = np.full((3, 2), float(len(self.calls)))
        if isinstance(step, dict):
            return maps, step
        raise ConvergenceError("not converged", maps, _stats(*step) if isinstance(step, tuple) else _stats(step))


def test_the_first_call_converges():
    good = dict(_stats(1e-14), converged=1)
    g = _Graph([good])
    v0 = np.arange(3.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        maps, stats = scs._fiedler_checked(g, v0, TOL, MAX_ITER, 8)
    assert g.calls == [(v0, TOL, MAX_ITER, 8)] and stats is good and np.all(maps == 1.0)
    assert "accepted_residual" not in stats


@pytest.mark.parametrize(("upper", "widest"), [(None, 16), (False, 16), (True, 8)])
def test_the_second_call_is_the_widest_block_and_four_times_the_iterations(upper, widest):
    good = dict(_stats(1e-14), converged=1)
    g = _Graph([1e-9, good], upper)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        maps, stats = scs._fiedler_checked(g, None, TOL, MAX_ITER, 0)
    assert g.calls == [(None, TOL, MAX_ITER, 0), (None, TOL, 4 * MAX_ITER, widest)]
    assert stats is good and np.all(maps == 2.0) and "accepted_residual" not in stats


@pytest.mark.parametrize(("first", "second", "best"), [(5e-9, 2e-9, 2), (3e-10, 8e-9, 1)])
def test_a_stopped_block_inside_both_limits_is_used_with_a_warning(first, second, best):
    g = _Graph([first, second])
    with pytest.warns(RuntimeWarning, match="stopped at residual"):
        maps, stats = scs._fiedler_checked(g, None, TOL, MAX_ITER, 0)
    assert len(g.calls) == 2 and np.all(maps == float(best))
    assert stats["accepted_residual"] == min(first, second) == max(stats["resid"])
    assert stats["accepted_residual"] <= scs.ACCEPT_RESIDUAL
    assert stats["accepted_residual"] <= scs.ACCEPT_RESIDUAL_OVER_GAP * abs(stats["lambda"][1] - stats["lambda_next"])


@pytest.mark.parametrize(("first", "second"), [
    (1e-7, 2e-8),  # above ACCEPT_RESIDUAL with a wide gap
    ((5e-9, 0.9, 0.9 - 1e-5), (4e-9, 0.9, 0.9 - 1e-5)),  # inside it, but 4e-9 / 1e-5 is above ACCEPT_RESIDUAL_OVER_GAP
])
def test_a_stopped_block_outside_either_limit_raises(first, second):
    assert scs.ACCEPT_RESIDUAL == 1e-8 and scs.ACCEPT_RESIDUAL_OVER_GAP == 1e-4
    g = _Graph([first, second])
    with pytest.raises(RuntimeError, match="did not converge") as info:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            scs._fiedler_checked(g, None, TOL, MAX_ITER, 0)
    assert not isinstance(info.value, ConvergenceError) and isinstance(info.value.__cause__, ConvergenceError)
    assert len(g.calls) == 2


def test_the_limits_are_inclusive():
    gap = 0.1
    at = min(scs.ACCEPT_RESIDUAL, scs.ACCEPT_RESIDUAL_OVER_GAP * gap)
    g = _Graph([(at, 0.9, 0.9 - gap), (1.0, 0.9, 0.9 - gap)])
    with pytest.warns(RuntimeWarning):
        _, stats = scs._fiedler_checked(g, None, TOL, MAX_ITER, 0)
    assert stats["accepted_residual"] == at
