"""The matrix-free operator (``csrc/scs_matfree.h``: ``k_mf_maxdepth``, ``k_mf_chunk``, ``k_mf_carry``,
``k_mf_reduce``, ``k_mf_operand``, ``k_mf_column0``; ``scs_graph_matrix_free`` / ``scs_matfree_apply``) against the host
reference of ``tests/matrix_free_reference.py`` at its edges: stacks that spill into the global strip and come back, deep
summaries and carried stacks, every chunk count, trees shorter than the chunk count, root separators at chunk edges,
what a 64-slot piece of ``k_mf_maxdepth`` can meet, both widths in turn on one graph, zero weights.

Every product is held elementwise to ``matrix_free_reference.budget`` (derived from the arithmetic, per tree); the
plan the library made (``DeviceGraph.matrix_free_plan``) equals ``plan_reference``; the CPU test
``tests/test_matrix_free_reference_cpu.py`` pins every case to its path and shows that a single misplaced leaf
exceeds the budget a hundredfold.  The scaling d^-1/2 of the reference is formed from the DEVICE's degrees, which are
themselves held to the reference (the vector of ones): operator and degrees are checked apart."""

from __future__ import annotations

import time

import numpy as np
import pytest

import build_reference as br
import matrix_free_reference as mf
from solver_reference import LD, apply_vectors, worst
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu

SCS_EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


def _check_plan(plan, want, b_cap, slabs_b, n_apply):
    assert plan["chunks"] == want["chunks"]
    assert np.array_equal(plan["maxd"], want["maxd"]), np.flatnonzero(plan["maxd"] != want["maxd"])[:8]
    assert plan["stack_total"] == want["stack_total"]
    assert (plan["b_cap"], plan["slabs_b"], plan["n_apply"]) == (b_cap, slabs_b, n_apply)


def _hold(what, got, ref, bud, figures):
    ratio, at = worst(got, ref, bud)
    figures[what] = ratio
    print(f"    {what}: worst |got - ref| / budget = {ratio:.3g} at {at}")
    assert ratio <= 1.0, (what, ratio, at)


def _unit_batches(cols, n):
    for i in range(0, len(cols), 8):
        x = np.zeros((n, 8))
        part = cols[i:i + 8]
        x[part, np.arange(len(part))] = 1.0
        yield part, x


@pytest.mark.parametrize("name", mf.CASES)
def test_matrix_free_operator_against_the_reference(dev, name):
    tb = mf.tables_of(name)
    n = tb.n_taxa
    want = mf.plan_reference(tb)
    w = mf.w_reference(tb)
    figures: dict = {}
    spent = 0.0
    dtab = dev.upload(tb)
    gm = dtab.matrix_free_graph(max_block=8)
    try:
        _check_plan(gm.matrix_free_plan(), want, 8, 0, 0)  # k_mf_maxdepth against the host, before anything runs
        if name.startswith("chunks_"):
            assert gm.matrix_free_plan()["chunks"] == mf.CHUNK_SIZES[int(name.split("_")[1])]
        # the vector of ones: the degrees
        t0 = time.perf_counter()
        deg = gm.degrees()
        spent += time.perf_counter() - t0
        ones = np.ones((n, 1))
        _hold("ones", deg[:, None], mf.apply_reference(w, ones), mf.budget(tb, ones), figures)
        _check_plan(gm.matrix_free_plan(), want, 8, 4, 1)
        zero = np.asarray(w.sum(axis=1) == 0)
        assert bool(np.all(deg[zero] == 0.0)) and bool(np.all(deg[~zero] > 0.0))
        if name == "mixed":  # (a taxon that shares no tree with another one has degree 0 as well)
            assert zero[mf.MIXED_LONE] and mf.MIXED_LONE not in set(tb.leaf_taxon.tolist())
        dinv = mf.dinv_of(deg)  # 1 where the degree is 0, as k_dinv has it
        # the dense probes: one reference product for all of them
        pr = mf.probes(n, name)
        ref_all = mf.apply_reference(w, np.concatenate(list(pr.values()), axis=1), dinv)
        at, applied = 0, 1
        for what, x in pr.items():
            b = x.shape[1]
            t0 = time.perf_counter()
            y, info = gm.apply_ex(x, reps=2)
            spent += time.perf_counter() - t0
            applied += 2
            assert info["matrix_free"] == 1 and info["image"] == 0
            _hold(what, y[0], ref_all[:, at:at + b], mf.budget(tb, x, dinv), figures)
            assert np.array_equal(y[0], y[1]), f"{what}: two applications of one vector differ"  # no atomics
            assert gm.matrix_free_plan()["slabs_b"] == b
            at += b
        # unit vectors: columns of W, eight per application
        cols = mf.unit_columns(tb, want["chunks"])
        assert len(cols) == n or n > mf.WHOLE_MATRIX_MAX
        s_ref = dinv[:, None] * w[:, cols] * dinv[cols][None, :]
        worst_unit = 0.0
        for i, (part, x) in enumerate(_unit_batches(cols, n)):
            t0 = time.perf_counter()
            y, _ = gm.apply_ex(x)
            spent += time.perf_counter() - t0
            applied += 1
            ref = np.zeros((n, 8), dtype=LD)
            ref[:, :len(part)] = s_ref[:, 8 * i:8 * i + len(part)]
            ratio, where = worst(y[0], ref, mf.budget(tb, x, dinv))
            worst_unit = max(worst_unit, ratio)
            assert ratio <= 1.0, ("unit", int(part[where[1]]) if where[1] < len(part) else -1, where, ratio)
        figures["unit"] = worst_unit
        print(f"    unit ({len(cols)} columns): worst ratio {worst_unit:.3g}")
        _check_plan(gm.matrix_free_plan(), want, 8, 8, applied)  # the plan is what it was; the count moved
    finally:
        gm.free()
        dtab.free()
    print(f"MF-EDGE | {name} | {n} | {tb.n_trees} | {want['chunks']} | "
          + " | ".join(f"{figures.get(k, float('nan')):.2g}" for k in ("ones", "plain8", "graded4", "graded8", "plain4", "unit"))
          + f" | {1e3 * spent:.0f} ms |")


def test_widths_in_turn_on_one_graph(dev):
    """b = 8, b = 4, b = 8 with different vectors on a graph of partial coverage: the slabs are laid out per width,
    and the entries of the taxa a tree does not hold must be zero again after every change."""
    tb = mf.tables_of("widths")
    n = tb.n_taxa
    w = mf.w_reference(tb)
    dtab = dev.upload(tb)
    gm = dtab.matrix_free_graph(max_block=8)
    try:
        dinv = mf.dinv_of(gm.degrees())
        assert gm.matrix_free_plan()["slabs_b"] == 4
        figures: dict = {}
        for step, (b, seed) in enumerate(((8, 101), (4, 102), (8, 103), (4, 104))):
            x = apply_vectors(n, b, seed, graded=bool(step % 2))
            y, _ = gm.apply_ex(x)
            _hold(f"step {step} (b = {b})", y[0], mf.apply_reference(w, x, dinv), mf.budget(tb, x, dinv), figures)
            assert gm.matrix_free_plan()["slabs_b"] == b
    finally:
        gm.free()
        dtab.free()


def test_refusals(dev):
    tb = mf.tables_of("widths")
    dtab = dev.upload(tb)
    try:
        g4 = dtab.matrix_free_graph(max_block=4)
        try:
            assert g4.matrix_free_plan()["b_cap"] == 4
            y, _ = g4.apply_ex(apply_vectors(tb.n_taxa, 4, 1))
            assert np.isfinite(y).all()
            with pytest.raises(nv.ScsError, match=r"block width 8 \(graph made for 4\)"):
                g4.apply_ex(apply_vectors(tb.n_taxa, 8, 1))
            assert g4.matrix_free_plan()["n_apply"] == 2  # the degrees and the one product: the refusal ran nothing
        finally:
            g4.free()
        for bad in (0, 2, 6, 12, 16):
            with pytest.raises(nv.ScsError, match="widest block 4 or 8"):
                dtab.matrix_free_graph(max_block=bad)
        g = dtab.build()
        try:
            with pytest.raises(nv.ScsError, match="the graph has a matrix") as err:
                g.matrix_free_plan()
            assert err.value.code == SCS_EINVAL
        finally:
            g.free()
    finally:
        dtab.free()
    small = br.tables(br.size_forest(mf.DENSE2_MAX), "branch")
    dtab = dev.upload(small)
    try:
        with pytest.raises(nv.ScsError, match=f"more than {mf.DENSE2_MAX} taxa"):
            dtab.matrix_free_graph(max_block=8)
    finally:
        dtab.free()
