"""The batched small-node solve (``scs_small_solve*``) against the extended-precision reference of
``small_solve_reference`` at its edges: repeated eigenvalues, zero degrees, heavy contraction above 64 taxa, the
24 | 25 and 64 | 65 thresholds, every tree count at which a loop of ``k_small_addends`` / ``k_small_sum`` changes its
step (needs an MI355X).  DESIGN.md section 21.

Every family is ONE ``Device.small_solve`` call: a mixed batch of ``k_small_finish<256>``, ``<1024>`` and
``k_small_finish_big`` nodes.  Nothing is skipped: a node whose eigenvectors are not defined is held to
``check_node`` (which needs no gap) and to the closed form of what IS defined.

On the parent commit's library (profiles/small_solve_edges_error_ratios.txt) every
``two_vertices`` node of 65 and 128 taxa fails: where s = (w / sqrt(w)) / sqrt(w) is exactly 1 (w = 1, 4, 7.5, 9, 1e-9)
column 1 comes back NaN, and so does the end-to-end case; where s is one ulp off (w = 2, 3, 0.3) column 1 is rounding
noise that is not orthogonal to column 0 (|x_0^T x_1| = 0.17).
"""

import numpy as np
import pytest
import small_solve_reference as ref

from spectralclustersupertree_amd import flatten as fl
from spectralclustersupertree_amd.backend import Device, SmallTicket
from spectralclustersupertree_amd.tree import TreeNode

pytestmark = pytest.mark.gpu

BARS = {"norm": ref.ORTH_BAR, "orth": ref.ORTH_BAR, "residual": ref.RESIDUAL_BAR, "lambda": ref.LAMBDA_BAR,
        "vectors": ref.FIEDLER_TOL, "closed_form": ref.FIEDLER_TOL, "twin": ref.FIEDLER_TOL}


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


# Device.small_solve sends a node whose batched solve came back non-finite through the general per-node path
# (SmallTicket.result): right for a caller, but here it would put another solver's answer in the kernel's place.
# Every such call while this module runs is noted, and a node that needed one fails.
_RESCUED = []


@pytest.fixture(scope="module", autouse=True)
def _watch_the_general_path():
    general_path = SmallTicket._general_path

    def noted(self, i):
        _RESCUED.append(i)
        return general_path(self, i)

    SmallTicket._general_path = noted
    yield
    SmallTicket._general_path = general_path


_SOLVED = {}


def _solved(dev, name):
    """The family's nodes, the oracle's W of each and what ONE batched call returned for them (computed once)."""
    if name not in _SOLVED:
        cases = ref.family(name)
        before = len(_RESCUED)
        out = dev.small_solve([(tables, gs) for _, tables, gs, _ in cases], want_w=True)
        rescued = set(_RESCUED[before:])
        _SOLVED[name] = [(label, tables, gs, expects, ref.oracle_w(tables, gs), maps.copy(), lam.copy(), w.copy(),
                          i in rescued)
                         for i, ((label, tables, gs, expects), (maps, lam, w)) in enumerate(zip(cases, out))]
    return _SOLVED[name]


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_family_against_the_reference(dev, name):
    worst = {}
    failures = []

    def note(key, value):
        worst[key] = max(worst.get(key, 0.0), value)

    solved = _solved(dev, name)
    by_label = {s[0]: s for s in solved}
    for label, tables, gs, expects, w_ref, maps, lam, w, rescued in solved:
        try:
            assert not rescued, "the batched solve came back non-finite (the node was solved again by the general path)"
            assert np.array_equal(w, w_ref), "W differs from the oracle's bits"
            assert np.array_equal(w, w.T), "W is not symmetric"
            figures = ref.node_errors(w_ref, maps, lam)
            for key in ("norm", "orth", "residual", "lambda"):
                note(key, figures.get(key, np.inf))
            ref.check_node(w_ref, maps, lam)
            if expects:
                err = ref.vector_error(w_ref, maps, ref.scale_of(label))
                note("vectors", err)
                ref.compare_vectors(w_ref, maps, ref.scale_of(label))
            else:
                err = ref.closed_form_error(label, w_ref, maps, lam)
                note("closed_form", err)
                assert err <= ref.FIEDLER_TOL, f"closed form missed by {err:.3e}"
            twin = ref.twin_of(label)
            if twin is not None:
                # S does not change under a scaling of W: maps sqrt(scale) is the unscaled node's embedding
                rt = float(np.sqrt(ref.LD(ref.scale_of(label))))
                err = float(np.max(np.abs(maps * rt - by_label[twin][5])))
                note("twin", err)
                assert err <= ref.FIEDLER_TOL, f"differs from its unscaled twin by {err:.3e}"
                assert np.max(np.abs(lam - by_label[twin][6])) <= ref.LAMBDA_BAR
        except AssertionError as exc:
            failures.append(f"{label} (taxa {tables.n_taxa}, trees {tables.n_trees}, vertices {w_ref.shape[0]}): {exc}")
    for key, value in worst.items():
        print(f"SMALL EDGES {name:15s} nodes {len(solved):3d} {key:12s} worst {value:.3e} bar {BARS[key]:.0e}")
    assert not failures, f"{len(failures)} of {len(solved)} nodes of '{name}' fail:\n" + "\n".join(failures)


@pytest.mark.parametrize("name", ["contracted", "two_vertices"])
def test_a_node_alone_gives_the_bits_it_gives_inside_the_batch(dev, name):
    failures = []
    solved = _solved(dev, name)
    before = len(_RESCUED)
    for label, tables, gs, _, _, maps, lam, w, _ in solved:
        m1, l1, w1 = dev.small_solve([(tables, gs)], want_w=True)[0]
        if not (np.array_equal(m1, maps, equal_nan=True) and np.array_equal(l1, lam, equal_nan=True)
                and np.array_equal(w1, w)):
            failures.append(label)
    assert not failures, failures
    assert len(_RESCUED) == before, "a node alone came back non-finite and was solved again by the general path"


def test_a_node_twice_in_one_batch_gives_the_same_bits(dev):
    picks = []
    for name in ("sizes", "contracted", "two_vertices", "complete", "path", "isolated"):
        cases = ref.family(name)
        picks += [cases[i] for i in sorted({0, len(cases) // 3, len(cases) // 2, len(cases) - 1})]
    nodes = [(tables, gs) for _, tables, gs, _ in picks]
    before = len(_RESCUED)
    out = dev.small_solve(nodes + nodes[::-1], want_w=True)
    assert len(_RESCUED) == before, "a node came back non-finite and was solved again by the general path"
    k = len(nodes)
    for i, (label, *_) in enumerate(picks):
        a, b = out[i], out[2 * k - 1 - i]
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), label


def test_two_vertices_after_contraction_of_65_taxa(dev):
    # tests/test_gpu_parity.py test_two_vertices_after_contraction at 65 taxa: the one-sided kernel's size.  Two
    # trees over the same two clades, one of them under a unary root: the clades contract to one vertex each, joined
    # by the weight 1 of the first tree under strategy `one` -- s = 1 exactly
    from spectralclustersupertree_amd.scs import relabel_for_contraction, spectral_bipartition_device

    names = [f"t{i:03d}" for i in range(65)]

    def forest_tree(unary):
        sides = [TreeNode("", [TreeNode(x, None, 0.05) for x in part], 1.0, 100.0) for part in (names[:33], names[33:])]
        root = TreeNode("", sides, 1.0, 100.0)
        return TreeNode("", [root]) if unary else root

    tables = fl.flatten_trees([forest_tree(True), forest_tree(False)], [1.0, 1.0], "one", names)
    assert int(fl.pcg_components(tables).max()) == 0
    groups = fl.contraction_groups(tables)
    assert int(groups.max()) + 1 == 2
    work, perm, group_start = relabel_for_contraction(tables, groups)
    w2 = ref.oracle_w(work, group_start)
    assert np.array_equal(w2, [[0.0, 1.0], [1.0, 0.0]])
    # the batched kernel itself, as the library leaves it: finite, and the closed form
    maps, lam = dev.small_solve_begin([(work, group_start)]).raw()
    ref.check_node(w2, maps, lam[0])
    assert ref.closed_form_error("two_vertices", w2, maps, lam[0]) <= ref.FIEDLER_TOL
    report = {}
    before = len(_RESCUED)
    members, labels = spectral_bipartition_device(tables, np.random.RandomState(3), contract_edges=True, device=dev,
                                                  report=report)
    assert sorted(sorted(int(i) for i in mm) for mm in members) == [list(range(33)), list(range(33, 65))]
    assert labels[0] != labels[1]
    assert report["n_vertices"] == 2 and report["small_path"]
    assert len(_RESCUED) == before, "the node came back non-finite and was solved again by the general path"
