"""``team_reference`` without a device: on integers the ranks' partial products of the upper-triangle job add up to
W z exactly and their degree parts to the row sums (every cell counted once), every stored cell is one the build
defines, the receive buffer's layout inverts and never reads a tail, plain fp64 numpy that assembles the product the
way the device does sits inside every budget the GPU tests use (and the defects DESIGN.md section 34 plants do not), and
the entry point is declared and bound."""

import re
from pathlib import Path

import numpy as np
import pytest
import solver_reference as sr
import team_reference as tr

from spectralclustersupertree_amd import _native as nv

ROOT = Path(__file__).resolve().parent.parent
ALL_UPPER = sorted({c for c in tr.UPPER_CASES if c[0] <= 1300})  # (the model's arithmetic does not change above)
ALL_ROWS = tr.ROW_CASES + tr.IMAGE_CASES


def _integer_w(n, seed=0, lone=()):
    rs = np.random.RandomState(seed + n)
    a = np.triu(rs.randint(0, 7, size=(n, n)), 1).astype(np.int64)
    w = a + a.T
    w[list(lone), :] = 0
    w[:, list(lone)] = 0
    return w


def test_the_cases_are_the_ones_named():
    for n, splits in ALL_ROWS:
        tr.check_splits(n, splits)
    for n, splits in tr.UPPER_CASES:
        tr.check_splits(n, splits, upper=True)
    assert [len(s) - 1 for _, s in tr.ROW_CASES] == [2, 2, 2, 3, 2, 3, 4, 4]
    one_row = [(n, s) for n, s in ALL_ROWS + tr.UPPER_CASES if 1 in np.diff(s)]
    assert {np.diff(s).tolist().index(1) == 0 for _, s in one_row} == {True, False}  # first and last
    assert (1025, (0, 1024, 1025)) in tr.UPPER_CASES and (1300, (0, 256, 1300)) in tr.UPPER_CASES
    # slices of unequal length: a chunk with a tail in every case but the even halves of 4096
    assert [len(set(np.diff(s))) > 1 for _, s in ALL_ROWS].count(False) == 1
    assert max(len(s) - 1 for _, s in ALL_ROWS + tr.UPPER_CASES) == 4
    assert {n for n, _ in tr.UPPER_CASES} == {513, 769, 1025, 1300, 2049, 4097}


@pytest.mark.parametrize("case", ALL_UPPER, ids=tr.case_id)
def test_upper_partials_add_up_to_the_product_exactly(case):
    n, splits = case
    w = _integer_w(n, lone=tr.lone_rows(splits))
    z = np.random.RandomState(1).randint(-5, 6, size=(n, 4)).astype(np.float64)
    total = np.zeros((n, 4), dtype=tr.LD)
    for rank in range(len(splits) - 1):
        part, mag = tr.upper_partial(w, splits, rank, z)
        assert (np.abs(part) <= mag).all()
        total += part
    assert np.array_equal(total.astype(np.int64), w @ z.astype(np.int64))


@pytest.mark.parametrize("case", ALL_UPPER, ids=tr.case_id)
def test_every_cell_is_counted_once_by_the_degree_parts(case):
    n, splits = case
    w = _integer_w(n, seed=3)
    world = len(splits) - 1
    parts = [tr.upper_degree_part(w, splits, r) for r in range(world)]
    assert parts[0].dtype == np.int64 and np.array_equal(sum(parts), w.sum(axis=1))
    # ... and counted ONCE: with every cell 1 (the diagonal included) the parts add up to V in every row
    ones = np.ones((n, n), dtype=np.int64)
    assert np.array_equal(sum(tr.upper_degree_part(ones, splits, r) for r in range(world)), np.full(n, n))
    # a rank contributes to its own rows and, transposed, only to columns right of its first 256-row block
    for r, p in enumerate(tr.upper_degree_part(ones, splits, r) for r in range(world)):
        assert not p[: splits[r]].any() and p[splits[r]:].all()


@pytest.mark.parametrize("case", ALL_UPPER, ids=tr.case_id)
def test_stored_cells_are_the_ones_the_build_defines(case):
    n, splits = case
    for rank in range(len(splits) - 1):
        stored, transposed = tr.upper_cells(n, splits, rank)
        rows = np.arange(splits[rank], splits[rank + 1])
        first_col = rows // 256 * 256  # section 28: "defined from the row's 256-column diagonal tile on"
        assert np.array_equal(stored, np.arange(n)[None, :] >= first_col[:, None])
        assert np.array_equal(np.argmax(stored, axis=1), first_col)
        assert first_col.min() >= splits[rank]  # (col0 of the rank's block: nothing left of it is stored)
        assert not (transposed & ~stored).any()
        # the diagonal tile is applied directly only, from both of its rows; everything right of it twice
        assert np.array_equal(stored & ~transposed, (np.arange(n)[None, :] // 256) == (rows // 256)[:, None])


@pytest.mark.parametrize("case", ALL_ROWS, ids=tr.case_id)
@pytest.mark.parametrize("b", tr.WIDTHS)
def test_unpack_inverts_slices_and_reads_no_tail(case, b):
    n, splits = case
    world, chunk = len(splits) - 1, tr.chunk_of(splits, b)
    y = np.random.RandomState(b).standard_normal((n, b))
    buf = tr.slices(y, splits, b)
    assert buf.shape == (world, chunk)
    assert np.array_equal(tr.unpack(buf, n, splits, b), y)  # (a NaN of a tail would not compare equal)
    idx = tr.unpack_index(n, splits, b)
    assert len(np.unique(idx)) == n * b
    for r in range(world):
        used = (splits[r + 1] - splits[r]) * b
        assert np.isnan(buf[r, used:]).all() and not np.isnan(buf[r, :used]).any()
        mine = idx[splits[r]:splits[r + 1]]
        assert mine.min() == r * chunk and mine.max() == r * chunk + used - 1
    assert int(np.isnan(buf).sum()) == world * chunk - n * b


# ---------------------------------------------------------------------------------------------------------------
# plain fp64, assembled the way the device assembles it, against the budgets of the GPU tests
# ---------------------------------------------------------------------------------------------------------------
def _float_w(n, lone=()):
    rs = np.random.RandomState(n)
    a = np.triu(rs.exponential(0.1, size=(n, n)) * (rs.random_sample((n, n)) < 0.3), 1)
    w = a + a.T
    w[list(lone), :] = 0.0
    w[:, list(lone)] = 0.0
    return w


def _dinv(w):
    deg = w.sum(axis=1)
    return np.where(deg == 0, 1.0, 1.0 / np.sqrt(np.where(deg == 0, 1.0, deg)))


@pytest.mark.parametrize("graded", [False, True])
@pytest.mark.parametrize("case", [c for c in ALL_UPPER if c[0] <= 1025], ids=tr.case_id)
def test_numpy_upper_job_is_inside_the_budgets(case, graded):
    n, splits = case
    lone = tr.lone_rows(splits)
    w = _float_w(n, lone)
    dinv = _dinv(w)
    x = sr.apply_vectors(n, 8, 5, graded)
    z = dinv[:, None] * x
    want, budget = sr.apply_reference(w, x)
    z_ref = sr.scaling(w)[:, None] * x.astype(tr.LD)
    parts = []
    for rank in range(len(splits) - 1):
        stored, transposed = tr.upper_cells(n, splits, rank)
        lo, hi = splits[rank], splits[rank + 1]
        p = np.zeros((n, 8))
        p[lo:hi] = np.where(stored, w[lo:hi], 0.0) @ z
        p += np.where(transposed, w[lo:hi], 0.0).T @ z[lo:hi]
        ref, mag = tr.upper_partial(w, splits, rank, z_ref)
        assert sr.worst(p, ref, sr.apply_budget(n, mag))[0] <= 1.0
        parts.append(p)
    got = dinv[:, None] * sum(parts)
    assert sr.worst(got, want, budget)[0] <= 1.0
    assert not got[lone].any() and not budget[lone].any()
    # the defects of section 34: the last rank left out, a rank's transposed slabs dropped.  (A last rank of one row
    # stores the diagonal cell alone, a zero: its partial product is zero and leaving it out shows nowhere -- the
    # hand-made split [0, 1024, 1025] is there for the tile lists, the other splits for this.)
    assert parts[-1].any() == (splits[-1] - splits[-2] > 1)
    if parts[-1].any():
        assert sr.worst(dinv[:, None] * sum(parts[:-1]), want, budget)[0] > 1e6
    direct_only = parts[0].copy()
    direct_only[splits[1]:] = 0.0
    ref0, mag0 = tr.upper_partial(w, splits, 0, z_ref)
    if ref0[splits[1]:].any():  # (not where the only row behind rank 0 is a lone vertex)
        assert sr.worst(direct_only, ref0, sr.apply_budget(n, mag0))[0] > 1e6
    # the degrees in fp64, part by part
    deg_ref, deg_budget = tr.br.degrees_reference(w)
    deg = sum(tr.upper_degree_part(w, splits, r).astype(np.float64) for r in range(len(splits) - 1))
    assert (np.abs(deg.astype(tr.LD) - deg_ref) <= deg_budget).all() and not deg[lone].any()


@pytest.mark.parametrize("case", [c for c in tr.ROW_CASES if c[0] <= 700], ids=tr.case_id)
def test_numpy_row_job_is_inside_the_budgets(case):
    n, splits = case
    b = 4
    lone = tr.lone_rows(splits)
    w = _float_w(n, lone)
    dinv = _dinv(w)
    q, aq = tr.panels(n, b, 11, graded=True)
    assert np.isnan(aq[:, 2 * b:]).all() and not np.isnan(aq[:, : 2 * b]).any()
    x = q[:, 2 * b:]
    want, budget = sr.apply_reference(w, x)
    y = dinv[:, None] * (w @ (dinv[:, None] * x))
    got = tr.unpack(tr.slices(y, splits, b), n, splits, b)
    assert sr.worst(got, want, budget)[0] <= 1.0
    ref, gb = tr.qaq_reference(q, aq, got)
    full = aq.copy()
    full[:, 2 * b:] = got
    assert sr.worst(q.T @ full, ref, gb)[0] <= 1.0
    # the defects of section 34: `>` for `>=` at a split reads the last row of the rank before, and a chunk indexed
    # with the rank's own row count instead of `chunk` reads another rank's rows or a tail
    idx = tr.unpack_index(n, splits, b)
    buf = tr.slices(y, splits, b).reshape(-1)
    off_by_one = idx.copy()
    for r in range(1, len(splits) - 1):
        s = splits[r]
        off_by_one[s] = (r - 1) * tr.chunk_of(splits, b) + (s - splits[r - 1]) * b + np.arange(b)
    rows = np.diff(splits)
    # (row splits[r] is then looked for at the END of rank r - 1's chunk: where that rank has the longest slice, the
    # end of its chunk is the start of the next one, the right row -- the defect shows only behind a shorter slice)
    assert (sr.worst(buf[off_by_one], want, budget)[0] > 1e6) == bool((rows[:-1] < rows.max()).any())
    rank = np.searchsorted(splits, np.arange(n), side="right") - 1
    own_count = (rank * rows[rank] * b + (np.arange(n) - np.asarray(splits)[rank]) * b)[:, None] + np.arange(b)[None, :]
    # (and this one only in front of a rank other than the first whose slice is shorter than the longest)
    assert (sr.worst(buf[own_count], want, budget)[0] > 1e6) == bool((rows[1:] < rows.max()).any())


def test_lone_forests_put_degree_zero_on_both_sides_of_a_boundary():
    from oracle import tables_oracle as to

    n, splits = 513, (0, 256, 513)
    lone = tr.lone_rows(splits)
    assert lone == [255, 256]
    for arrays in (tr.apply_forest(n, lone), tr.degree_forest(n, lone)):
        assert arrays.n_taxa == n
        w = to.pcg_dense(tr.br.tables(arrays, "branch"))[0]
        assert not w[lone].any() and not w[:, lone].any()
        assert (np.abs(w).sum(axis=1) > 0).sum() >= n - 3  # (degree_forest keeps a lone taxon of its own)
    w = to.pcg_dense(tr.br.tables(tr.apply_forest(n), "branch"))[0]
    assert (w >= 0).all() and (w.sum(axis=1) > 0).all()


def test_the_team_entry_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(r"int scs_debug_team_apply\(([^)]*)\)", text)
    assert m, "include/scs_hip.h does not declare scs_debug_team_apply"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES["scs_debug_team_apply"]
    assert restype is nv.C.c_int and len(argtypes) == len(params) == 12
    for i, (p, a) in enumerate(zip(params, argtypes)):
        assert (a is nv.C.c_int32) == p.startswith("int32_t "), (i, p)
        assert (a is nv.C.c_void_p) == ("*" in p), (i, p)
    assert params[4:8] == ["int32_t b", "int32_t path", "int32_t image", "int32_t reps"]
    assert params[-1] == "int64_t *info_out"
    lib = nv.load_library()
    assert hasattr(lib, "scs_debug_team_apply") and lib.scs_version() == nv.ABI_VERSION == 109
