"""The checks and the case generator of ``small_solve_reference`` without a device: LAPACK passes every bar on every
case (so a correct kernel can), every case is what its flag and its family say it is (so the GPU test skips nothing
silently), and the checks fail on the defects they are there for."""

import numpy as np
import pytest
import small_solve_reference as ref


def _cases(name):
    return [(case[0], ref.oracle_w(case[1], case[2]), case) for case in ref.family(name)]


def test_every_tree_count_is_met_on_both_sides_of_every_threshold():
    plan = ref.sizes_plan()
    assert {n for n, _ in plan} == set(ref.SIZES_TAXA)
    for lo, hi in ((3, ref.SMALL_TR_MAX), (ref.SMALL_TR_MAX + 1, 128), (ref.TWO_SIDED_MAX + 1, 128)):
        assert {m for n, m in plan if lo <= n <= hi} == set(ref.TREE_COUNTS), (lo, hi)
    got = {(c[1].n_taxa, c[1].n_trees) for c in ref.sizes()}
    assert got == set(plan)
    # trees of n, n / 2 and 2 leaves in one node wherever it has three trees or more
    for _, tables, _, _ in ref.sizes():
        if tables.n_trees >= 3 and tables.n_taxa >= 8:
            assert set(np.diff(tables.tree_off)) == {tables.n_taxa, tables.n_taxa // 2, 2}


def test_the_contracted_family_crosses_kernel_choice_with_jacobi_size():
    seen = {(c[1].n_taxa, len(c[2]) - 1) for c in ref.contracted()}
    for n in ref.CONTRACTED_TAXA:
        for v in (*[g for g in ref.CONTRACTED_GROUPS if g <= n], n - 1):
            assert (n, v) in seen
    # the two 24 | 25 thresholds disagree, and the big kernel runs at a handful of vertices
    assert (24, 24) in seen and (25, 25) in seen and (64, 64) in seen  # identity group_start, given explicitly
    assert (40, 10) in seen and (25, 24) in seen and (100, 2) in seen and (100, 3) in seen and (128, 25) in seen
    for name, tables, gs, _ in ref.contracted():
        assert gs[0] == 0 and gs[-1] == tables.n_taxa and np.all(np.diff(gs) >= 1), name
        if "-big-" in name:
            assert np.diff(gs).max() == tables.n_taxa - (len(gs) - 1) + 1


@pytest.mark.parametrize("name", ref.FAMILIES)
def test_lapack_passes_every_bar_and_every_flag_is_true(name):
    cases = _cases(name)
    assert cases
    for label, w, (_, tables, gs, expects) in cases:
        assert np.array_equal(w, w.T) and not np.diag(w).any(), label
        maps, lam = ref.lapack_embedding(w)
        ref.check_node(w, maps, lam)
        if expects:
            g1, g2 = ref.gaps(w)
            assert g1 > ref.GAP and g2 > ref.GAP, (label, g1, g2)
            assert ref.compare_vectors(w, maps, ref.scale_of(label)) == 0.0
        else:
            assert not ref.vectors_defined(w) or ref.sign_tied(w), label
            assert ref.closed_form_error(label, w, maps, lam) <= ref.FIEDLER_TOL, label
    if name not in ("sizes", "two_vertices", "complete", "two_components"):
        assert all(c[2][3] for c in cases)  # no other family holds a degenerate node


def test_the_families_are_what_they_say():
    for label, w, (_, tables, gs, _) in _cases("two_vertices"):
        omega = float(label.rsplit("-w", 1)[1])
        assert w.shape == (2, 2) and w[0, 1] == omega and w[1, 0] == omega, label
    assert {float(c[0].rsplit("-w", 1)[1]) for c in ref.two_vertices()} == set(ref.TWO_VERTEX_WEIGHTS)
    for label, w, _ in _cases("path"):
        assert abs(ref.eigenvalues(w)[-1] + 1) <= 1e-12, label
    for label, w, (_, tables, gs, _) in _cases("isolated"):
        assert np.count_nonzero(w.sum(axis=0) == 0) == 1, label
        if gs is not None:
            assert gs[1] == 1 and w[0].sum() == 0  # the loner is a group of its own
    for label, w, _ in _cases("complete"):
        v = w.shape[0]
        ev = ref.eigenvalues(w)
        assert abs(ev[0] - 1) <= 1e-12 and np.max(np.abs(ev[1:] + 1 / (v - 1))) <= 1e-12, label
    for label, w, _ in _cases("two_components"):
        ev = ref.eigenvalues(w)
        assert abs(ev[0] - 1) <= 1e-12 and abs(ev[1] - 1) <= 1e-12 and ev[2] < 1 - 1e-3, label
    assert {c[2][1].n_taxa for c in _cases("complete")} >= set(ref.COMPLETE_VERTICES)


def test_scaled_twins_have_the_same_operator():
    cases = {label: w for label, w, _ in _cases("scaled")}
    for label, w in cases.items():
        twin = ref.twin_of(label)
        if twin is None:
            continue
        sc = ref.scale_of(label)
        assert sc in ref.SCALES
        assert np.max(np.abs(w / sc - cases[twin])) <= 1e-15 * cases[twin].max()
        a, _ = ref.lapack_embedding(w)
        b, _ = ref.lapack_embedding(cases[twin])
        assert np.max(np.abs(a * float(np.sqrt(ref.LD(sc))) - b)) <= ref.FIEDLER_TOL
    graded = next(c for c in ref.scaled() if "graded" in c[0])[1]
    inner = graded.adj_val[graded.adj_depth > 0]
    assert inner.max() > 1e12 * inner.min() > 0  # (the values are sums of lengths along a path: the small ones vanish)


def _generic():
    label, tables, gs, _ = next(c for c in ref.contracted() if c[0].startswith("contracted-n40-v10-cuts"))
    w = ref.oracle_w(tables, gs)
    maps, lam = ref.lapack_embedding(w)
    ref.check_node(w, maps, lam)
    return w, maps, lam


def test_a_nan_column_fails():
    w, maps, lam = _generic()
    bad = maps.copy()
    bad[:, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ref.check_node(w, bad, lam)
    with pytest.raises(AssertionError):
        ref.compare_vectors(w, bad)
    # the defect of the one-sided kernel at two vertices: finite eigenvalues, 0 / 0 in the second column
    w2 = ref.oracle_w(*ref.two_vertices()[0][1:3])
    m2, l2 = ref.lapack_embedding(w2)
    m2[:, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ref.check_node(w2, m2, l2)
    assert ref.closed_form_error("two_vertices", w2, m2, l2) > ref.FIEDLER_TOL


def test_an_unrotated_matrix_fails():
    w, maps, lam = _generic()
    _, dd = ref.reference(w)
    ident = np.eye(w.shape[0])[:, :2] / dd.astype(np.float64)[:, None]
    with pytest.raises(AssertionError, match="S x - lambda x"):
        ref.check_node(w, ident, lam)


def test_a_wrong_sign_fails():
    w, maps, lam = _generic()
    # (the first column of a connected graph is the constant 1 / ||sqrt(d)||: every magnitude ties and the rule leaves
    # its sign open, as it does in scikit-learn; the second column is where a sign can be wrong)
    mags = np.sort(np.abs(maps[:, 1]))[::-1]
    assert mags[0] - mags[1] > 1e-3 * mags[0]
    bad = maps.copy()
    bad[:, 1] = -bad[:, 1]
    with pytest.raises(AssertionError, match="largest magnitude"):
        ref.check_node(w, bad, lam)
    with pytest.raises(AssertionError):
        ref.compare_vectors(w, bad)


def test_an_eigenvector_of_w_instead_of_s_fails():
    w, maps, lam = _generic()
    _, dd = ref.reference(w)
    ev, vec = np.linalg.eigh(w)
    bad = ref.to.sign_flip_columns(vec[:, ::-1][:, :2] / dd.astype(np.float64)[:, None])
    with pytest.raises(AssertionError):
        ref.check_node(w, bad, lam)
    with pytest.raises(AssertionError):
        ref.compare_vectors(w, bad)


def test_a_sign_taken_on_the_unit_vector_fails_somewhere():
    # the sign rule is on x / dd, not on the unit eigenvector x: the generator holds nodes at which the two differ
    differ = 0
    for label, tables, gs, expects in ref.contracted() + ref.isolated():
        w = ref.oracle_w(tables, gs)
        maps, lam = ref.lapack_embedding(w)
        _, dd = ref.reference(w)
        x = maps * dd.astype(np.float64)[:, None]
        for c in range(2):
            if np.argmax(np.abs(x[:, c])) != np.argmax(np.abs(maps[:, c])) and x[np.argmax(np.abs(x[:, c])), c] < 0:
                differ += 1
    assert differ >= 3


def test_eigenvalues_off_by_more_than_the_bar_fail():
    w, maps, lam = _generic()
    for k in range(3):
        bad = lam.copy()
        bad[k] += 3e-12
        with pytest.raises(AssertionError):
            ref.check_node(w, maps, bad)
    w2 = ref.oracle_w(*ref.two_vertices()[0][1:3])
    m2, l2 = ref.lapack_embedding(w2)
    l2[2] = 1e-300
    with pytest.raises(AssertionError, match="beyond the vertex count"):
        ref.check_node(w2, m2, l2)


def test_a_non_finite_embedding_marks_its_own_node_only():
    from spectralclustersupertree_amd.backend import _refuse_nonfinite_maps

    n_groups = np.array([3, 2, 4], dtype=np.int32)
    maps, lam = np.ones((9, 2)), np.arange(9.0).reshape(3, 3)
    _refuse_nonfinite_maps(maps, lam, n_groups)
    assert np.array_equal(lam, np.arange(9.0).reshape(3, 3))  # all finite: untouched
    maps[4, 1] = np.nan  # second node, second column: the defect's shape
    _refuse_nonfinite_maps(maps, lam, n_groups)
    assert np.all(np.isnan(lam[1])) and np.array_equal(lam[[0, 2]], np.arange(9.0).reshape(3, 3)[[0, 2]])
    maps[8, 0] = np.inf
    _refuse_nonfinite_maps(maps, lam, n_groups)
    assert np.all(np.isnan(lam[1:])) and np.array_equal(lam[0], [0.0, 1.0, 2.0])
