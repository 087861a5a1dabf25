"""The cases and checks of ``fiedler_reference`` without a device: LAPACK passes every bar on every new case (so a
correct solver can), every case is what its flag, its group and its path say it is (so the GPU test skips nothing
silently), the path thresholds are the library's, and the checks fail on the defects they are there for."""

import re
from pathlib import Path

import fiedler_reference as fr
import numpy as np
import pytest
import small_solve_reference as ssr

SOURCE = Path(__file__).resolve().parent.parent / "spectralclustersupertree_amd" / "csrc" / "scs_eig.hip"


def _cases(name):
    return [(case, ssr.oracle_w(case[1], case[2])) for case in fr.group(name)]


def test_the_path_thresholds_are_the_librarys():
    text = SOURCE.read_text()

    def constant(pattern):
        found = re.findall(pattern, text)
        assert len(found) == 1, (pattern, found)
        return int(found[0])

    assert constant(r"constexpr int MAXS = (\d+);") == fr.JACOBI_MAX == 64
    assert constant(r"static const int dense_max = (\d+);") == fr.ONE_SIDED_MAX == 96
    assert constant(r"constexpr int DENSE2_MAX = (\d+);") == fr.SYNC_DEGREES_MAX == 128
    assert "if (n <= DENSE2_MAX) SCS_TRY(scs_graph_prepare_degrees(ctx, g));" in text
    assert "if (n > MAXS && n <= dense_max && block == 0 && ctx->comm.world == 1 && !g->upper)" in text
    assert tuple(int(x) for x in re.findall(r"const int allowed\[\] = \{(.*?)\};", text)[0].split(",")) == fr.WIDTHS
    for v, block, path in ((2, 0, "two_sided"), (64, 16, "two_sided"), (65, 0, "one_sided"), (65, 4, "iterative"),
                           (96, 0, "one_sided"), (96, 12, "iterative"), (97, 0, "iterative"), (4095, 0, "iterative")):
        assert fr.path_of(v, block) == path, (v, block)
    # 3 b + 2 <= V: 16 fits from 50 vertices on, 12 from 38
    assert [fr.width_of(v, b) for v, b in ((65, 16), (65, 0), (97, 8), (257, 12), (49, 16), (37, 12), (97, 5))] == [
        16, 4, 8, 12, 12, 8, 4]


def test_every_family_of_the_small_solve_is_a_group_unchanged():
    assert fr.GROUPS[:len(ssr.FAMILIES)] == ssr.FAMILIES
    seen = set()
    for name in ssr.FAMILIES:
        old, new = ssr.family(name), fr.group(name)
        assert len(old) == len(new)
        for (label, tables, gs, expects), case in zip(old, new):
            assert case[0] == label and case[1] is tables and case[2] is gs and case[3] == expects
            assert case[4] == 0 and case[5] is None
            seen.add(fr.path_of(fr.vertices(case), 0))
    assert seen == {"two_sided", "one_sided", "iterative"}
    # the base of 100 taxa and its twins now run on the iterative path
    assert {fr.path_of(fr.vertices(c), 0) for c in fr.group("scaled") if "-n100-" in c[0]} == {"iterative"}


def test_every_listed_size_and_width_is_present():
    def have(name):
        return {(fr.vertices(c), c[4]) for c in fr.group(name)}

    assert have("generic") == {(v, 0) for v in (5, 12, 13, 95, 96, 97, 129, 255, 256, 257, 1025)}
    assert have("widths") == {(65, 4), (65, 16), (96, 8), (96, 12), (97, 8), (257, 12), (257, 16)}
    assert all(fr.path_of(v, b) == "iterative" and fr.width_of(v, b) == b for v, b in have("widths"))
    got = {(c[1].n_taxa, fr.vertices(c), c[0].split("-")[3]) for c in fr.group("contracted_above_128")}
    want = {(200, v, t) for v in (2, 3, 24, 25, 64, 65, 95, 96) for t in ("cuts", "big")}
    want |= {(300, v, t) for v in (97, 129) for t in ("cuts", "big")}
    assert got == want
    for _, tables, gs, *_ in fr.group("contracted_above_128"):
        assert tables.n_taxa > fr.SYNC_DEGREES_MAX  # (beyond the batched small-node solve)
        assert gs[0] == 0 and gs[-1] == tables.n_taxa and np.all(np.diff(gs) >= 1)
    assert have("long_paths") == {(v, 0) for v in (95, 96, 97, 129, 257)}
    assert have("complete_graphs") == {(95, 0), (96, 0), (97, 0), (129, 0), (65, 4)}
    assert have("two_components_large") == {(v, 0) for v in (96, 98, 130, 258)}
    assert have("isolated_large") == {(v, 0) for v in (95, 97, 129, 257, 100)}
    own = next(c for c in fr.group("isolated_large") if "own-group" in c[0])
    assert own[1].n_taxa == 200 and own[2][1] == 1
    assert {c[1].n_taxa for c in fr.group("scaled_large") if "graded" in c[0]} == {100, 200}
    assert {c[0] for c in fr.group("scaled_large") if "graded" not in c[0]} == {
        "scaled-n200-base", "scaled-n200-x1e+150", "scaled-n200-x1e-150"}
    assert max(fr.vertices(c) for name in fr.GROUPS for c in fr.group(name)) == 1025


def test_half_of_the_iterative_cases_start_from_a_drawn_vector():
    with_seed = without = 0
    for name in fr.NEW_GROUPS:
        for case in fr.group(name):
            v = fr.vertices(case)
            if fr.path_of(v, case[4]) != "iterative":
                assert case[5] is None, case[0]
                continue
            x = fr.x_init(case)
            if case[5] is None:
                assert x is None
                without += 1
            else:
                assert np.array_equal(x, np.random.RandomState(case[5]).uniform(-1, 1, v)) and x.shape == (v,)
                with_seed += 1
    assert with_seed >= 15 and abs(with_seed - without) <= len(fr.NEW_GROUPS)


@pytest.mark.parametrize("name", fr.NEW_GROUPS)
def test_lapack_passes_every_bar_and_every_flag_is_true(name):
    cases = _cases(name)
    assert cases
    for (label, tables, gs, expects, block, _), w in cases:
        assert np.array_equal(w, w.T) and not np.diag(w).any(), label
        maps, lam = ssr.lapack_embedding(w)
        ssr.check_node(w, maps, lam)
        ssr.check_node(w, maps, lam, exact=2)
        g1, g2 = ssr.gaps(w)
        if expects:
            assert g1 > ssr.GAP and g2 > ssr.GAP, (label, g1, g2)
            assert ssr.compare_vectors(w, maps, ssr.scale_of(label)) == 0.0
            assert fr.unit_vector_error(w, maps) == 0.0
            assert fr.embedding_bar(w, ssr.scale_of(label)) >= ssr.FIEDLER_TOL
        else:
            assert not ssr.vectors_defined(w) or ssr.sign_tied(w), label
            assert ssr.closed_form_error(label, w, maps, lam) <= ssr.FIEDLER_TOL, label
        if name in ("generic", "widths", "contracted_above_128"):
            bar = fr.ITERATIVE_GAP if fr.path_of(w.shape[0], block) == "iterative" else 10 * ssr.GAP
            assert min(g1, g2) > bar, (label, g1, g2)
    if name not in ("complete_graphs", "two_components_large"):
        assert all(c[3] for c, _ in cases)  # no other group holds a degenerate node


def test_the_groups_are_what_they_say():
    for (label, *_), w in _cases("long_paths"):
        v = w.shape[0]
        ev = ssr.eigenvalues(w)
        # a path is bipartite: the eigenvalue -1 (a zero column of the one-sided sweeps), and cos(k pi / (V - 1))
        assert np.max(np.abs(ev - np.cos(np.arange(v) * np.pi / (v - 1)))) <= 1e-12, label
    for (label, *_), w in _cases("complete_graphs"):
        v = w.shape[0]
        ev = ssr.eigenvalues(w)
        assert abs(ev[0] - 1) <= 1e-12 and np.max(np.abs(ev[1:] + 1 / (v - 1))) <= 1e-12, label
        assert len(set(w[~np.eye(v, dtype=bool)])) == 1, label
    for (label, *_), w in _cases("two_components_large"):
        ev = ssr.eigenvalues(w)
        assert abs(ev[0] - 1) <= 1e-12 and abs(ev[1] - 1) <= 1e-12 and ev[2] < 1 - 1e-3, label
        assert len(set(ssr._components(w))) == 2 and not (w.sum(axis=0) == 0).any(), label
    for (label, tables, gs, *_), w in _cases("isolated_large"):
        assert np.count_nonzero(w.sum(axis=0) == 0) == 1 and w[0].sum() == 0, label
    for (label, tables, *_), w in _cases("scaled_large"):
        if "graded" in label:
            inner = tables.adj_val[tables.adj_depth > 0]
            assert inner.max() > 1e12 * inner.min() > 0, label
    cases = {c[0]: w for c, w in _cases("scaled_large")}
    for label, w in cases.items():
        twin = ssr.twin_of(label)
        if twin is not None:
            sc = ssr.scale_of(label)
            assert sc in ssr.SCALES and np.max(np.abs(w / sc - cases[twin])) <= 1e-15 * cases[twin].max()


def _generic():
    case = next(c for c in fr.group("generic") if c[0].startswith("generic-n97"))
    w = ssr.oracle_w(case[1], case[2])
    maps, lam = ssr.lapack_embedding(w)
    ssr.check_node(w, maps, lam, exact=2)
    return w, maps, lam


def test_planted_defects_fail():
    w, maps, lam = _generic()
    _, dd = ssr.reference(w)
    # a NaN column
    bad = maps.copy()
    bad[:, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        ssr.check_node(w, bad, lam, exact=2)
    assert not fr.unit_vector_error(w, bad) <= ssr.FIEDLER_TOL
    # a wrong sign of the second column
    mags = np.sort(np.abs(maps[:, 1]))[::-1]
    assert mags[0] - mags[1] > 1e-3 * mags[0]
    bad = maps.copy()
    bad[:, 1] = -bad[:, 1]
    with pytest.raises(AssertionError, match="largest magnitude"):
        ssr.check_node(w, bad, lam, exact=2)
    assert fr.unit_vector_error(w, bad) > ssr.FIEDLER_TOL
    # a second column that is not orthogonal to the first: 1e-9 of the trivial vector left in it
    x = maps * dd.astype(np.float64)[:, None]
    x[:, 1] = (x[:, 1] + 1e-9 * x[:, 0]) / np.sqrt(1 + 1e-18)
    bad = x / dd.astype(np.float64)[:, None]
    with pytest.raises(AssertionError, match=r"x_0\^T x_1"):
        ssr.check_node(w, bad, lam, exact=2)
    assert fr.unit_vector_error(w, bad) > ssr.FIEDLER_TOL
    # an eigenvalue off by 1e-9
    for k in range(2):
        bad = lam.copy()
        bad[k] += 1e-9
        with pytest.raises(AssertionError):
            ssr.check_node(w, maps, bad, exact=2)


def test_the_relaxed_rule_for_lambda_next():
    w, maps, lam = _generic()
    ev = ssr.eigenvalues(w)
    # an unconverged Ritz value: anywhere below lambda_3 passes with two exact eigenvalues, and fails with three
    for below in (1e-9, 1e-3, 0.5):
        ritz = lam.copy()
        ritz[2] = ev[2] - below
        e = ssr.check_node(w, maps, ritz, exact=2)
        assert e["lambda_next"] == pytest.approx(-below, rel=1e-6)
        with pytest.raises(AssertionError, match="lambda - LAPACK"):
            ssr.check_node(w, maps, ritz)
    # ... but not above lambda_3 + bar (Cauchy interlacing), nor above lambda[1]
    for above in (3e-12, 1e-9, 0.5 * (ev[1] - ev[2])):
        ritz = lam.copy()
        ritz[2] = ev[2] + above
        with pytest.raises(AssertionError, match="lambda_next"):
            ssr.check_node(w, maps, ritz, exact=2)
    ritz = lam.copy()
    ritz[2] = np.nextafter(lam[1], 2.0)
    with pytest.raises(AssertionError, match="lambda_next"):
        ssr.check_node(w, maps, ritz, exact=2)
    # the default keeps the three exact eigenvalues and reports no such figure
    assert "lambda_next" not in ssr.node_errors(w, maps, lam)
    # a complete graph: lambda_2 = lambda_3, and a Ritz value equal to lambda[1] passes
    case = fr.group("complete_graphs")[0]
    wk = ssr.oracle_w(case[1], case[2])
    mk, lk = ssr.lapack_embedding(wk)
    lk[2] = lk[1]
    ssr.check_node(wk, mk, lk, exact=2)
