"""No device: every forest of ``tests/build_reference.py`` has the numbers ``tests/test_gpu_build_edges.py`` runs it
for, the degree budget accepts plain double precision in any order and rejects what a broken
kernel would give, the image reference differs from W, the contraction cases hold blocks whose maximum is negative,
and the new diagnostic entry is declared, bound and exported."""

import re
from pathlib import Path

import build_reference as br
import forest_reference as fr
import numpy as np
import pytest

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native as nv

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the host plan
def test_padding_and_tile_counts_at_the_sizes():
    assert [br.ld_of(n) for n in (1, 511, 512, 513, 1024, 1025)] == [512, 512, 512, 1024, 1024, 1536]
    assert [br.npad_of(n) for n in (1, 256, 257, 512, 513, 769)] == [512, 512, 512, 512, 1024, 1024]
    for n in br.SIZES:
        t = br.tiles(n)
        n_blocks, n_cg = -(-n // br.TR), -(-n // br.TCW)
        assert len(br.tiles(n, upper=False)) == n_blocks * n_cg
        # a tile is kept iff it reaches right of its block's first row: every cell on or right of the diagonal is
        # in a kept tile, and a dropped tile lies wholly left of it
        kept = set(t)
        for b in range(n_blocks):
            for c in range(n_cg):
                assert ((b, c) in kept) == ((c + 1) * br.TCW > b * br.TR)
    # the sizes sit on, one short of and one past the three granularities
    assert {63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025} <= set(br.SIZES)


def test_whole_matrix_tile_counts_skip_8_13_and_25():
    counts = {n: len(br.tiles(n)) for n in range(1, 900)}
    seen = sorted(set(counts.values()))
    assert seen[:13] == [1, 2, 3, 4, 9, 10, 11, 12, 21, 22, 23, 24, 37]
    first = {c: min(n for n in counts if counts[n] == c) for c in seen}
    last = {c: max(n for n in counts if counts[n] == c) for c in seen}
    # the neighbours of the three gates that do occur, and the sizes where they change
    assert (last[4], first[9]) == (256, 257)  # per-XCD order: more than 8 tiles
    assert (last[12], first[21]) == (512, 513)  # producer / consumer kernel: from 13 tiles
    assert (last[24], first[37]) == (768, 769)  # tree-parallel build: up to 24 tiles
    # exactly 8 and 9 tiles exist as row ranges (every column group of the rows' blocks)
    # ... and 12 and 13: the producer / consumer gate, which does not ask for the whole matrix, on its two sides
    want_tiles = {"rows_tiles_8": 8, "rows_tiles_9": 9, "rows_tiles_12_trees_96": 12, "rows_tiles_13_trees_96": 13,
                  "rows_tiles_13_trees_95": 13}
    assert sorted(want_tiles) == sorted(br.GATE_ROW_CASES)
    plans = {}
    for case, want in want_tiles.items():
        n, n_trees, leaves, (rb, re_) = br.GATE_ROW_CASES[case]
        assert len(br.tiles(n, rb, re_)) == want and n_trees <= 256
        assert leaves / n > 2 * br.LIST_COVERAGE  # no tile lists
        plans[case] = br.plan(n, n_trees, n_trees * leaves, True, rb, re_)
        assert not plans[case]["tree_parallel"] and not plans[case]["listed"]
    assert {c for c in plans if plans[c]["wide"]} == {"rows_tiles_13_trees_96"}
    assert min(n for n in range(1, 4000) if len(br.tiles(n, 0, 64)) == 13) == 3073


def test_gate_cases_sit_on_both_sides_of_every_gate():
    plans = {}
    for case, (n, n_trees, leaves) in br.GATE_CASES.items():
        tb = br.tables(br.gate_forest(n, n_trees, leaves), "branch")
        assert tb.monotone and tb.n_trees == n_trees and n <= br.SMALL_N_ONE_BATCH and n_trees <= 4096
        plans[case] = br.plan(n, tb.n_trees, tb.n_leaves, True)
        plans[case]["coverage"] = br.coverage(tb)
    p = plans
    assert (p["tiles_4"]["n_tiles"], p["tiles_9"]["n_tiles"]) == (4, 9)
    assert not p["tiles_4"]["xcd_reorder"] and p["tiles_9"]["xcd_reorder"]
    assert (p["tiles_12"]["n_tiles"], p["tiles_21"]["n_tiles"]) == (12, 21)
    assert not p["tiles_12"]["wide"] and p["tiles_21"]["wide"]
    assert not p["tiles_12"]["tree_parallel"] and not p["tiles_21"]["tree_parallel"]  # 100 trees
    assert p["tiles_24_trees_127"]["n_tiles"] == p["tiles_24_trees_128"]["n_tiles"] == 24
    assert not p["tiles_24_trees_127"]["tree_parallel"] and p["tiles_24_trees_127"]["wide"]
    assert p["tiles_24_trees_128"]["tree_parallel"] and not p["tiles_24_trees_128"]["wide"]
    assert p["tiles_37_trees_128"]["n_tiles"] == 37
    assert not p["tiles_37_trees_128"]["tree_parallel"] and p["tiles_37_trees_128"]["wide"]
    assert not p["tiles_37_trees_95"]["wide"] and p["tiles_37_trees_96"]["wide"]
    assert p["coverage_at"]["coverage"] == br.LIST_COVERAGE and not p["coverage_at"]["listed"]
    assert p["coverage_below"]["coverage"] < br.LIST_COVERAGE and p["coverage_below"]["listed"]
    assert p["coverage_below"]["coverage"] > br.LIST_COVERAGE * 0.99  # just under
    for case in plans:
        if not case.startswith("coverage"):
            assert plans[case]["coverage"] > 2 * br.LIST_COVERAGE and not plans[case]["listed"]


def test_levels_for_changes_at_powers_of_two():
    assert [br.levels_for(m) for m in (0, 1, 2, 3, 4, 1023, 1024, 1025, 2047, 2048, 2049)] == [0, 1, 2, 2, 3, 10, 11, 11, 11, 12, 12]
    for m in br.LEVEL_GAPS:
        lv = br.levels_for(m)
        assert (1 << (lv - 1)) <= m < (1 << lv)
        top = m - (1 << (lv - 1)) + 1  # entries of the top level
        assert top == 1 if m & (m - 1) == 0 else top > 1
    # the fused kernel's stride: levels with more than, exactly and fewer than 1024 entries
    assert {1023, 1024, 1025} <= set(br.LEVEL_GAPS) and br.FUSED_THREADS == 1024
    assert br.levels_for(br.SPARSE_FUSED_MAX_LEAVES - 1) == 15 and br.levels_for(br.SPARSE_FUSED_MAX_LEAVES) == 16


# ------------------------------------------------------------------------------------------------ the forests
@pytest.mark.parametrize("kind", ["random", "balanced", "caterpillar", "star"])
def test_shapes_are_well_formed_and_have_their_depths(kind):
    rng = np.random.RandomState(1)
    for k in (1, 2, 3, 4, 5, 64, 65, 257):
        arrays = br.forest(k, 300, [(kind, br.order_random(rng, np.arange(300), k))])
        fr.well_formed(arrays)
        tb = br.tables(arrays, "depth")
        assert tb.n_leaves == k and tb.tree_off.tolist() == [0, k]
        gaps = tb.adj_depth[: k - 1]
        if k <= 2:
            assert not gaps.any()  # the only LCA is the root
        elif kind == "star":
            assert gaps[:-1].tolist() == [1] * (k - 2) and gaps[-1] == 0
        elif kind == "caterpillar":
            assert gaps.tolist() == list(range(k - 2, -1, -1))
        elif kind == "balanced":
            assert gaps.max() == int(np.ceil(np.log2(k))) - 1 and (gaps == 0).sum() == 1


def test_a_tree_of_32769_leaves_is_written_as_arrays():
    # no tree objects: one pass over 2 k - 1 nodes (a fraction of a second; no wall-clock bound is asserted here)
    arrays = br.big_forest(br.SPARSE_FUSED_MAX_LEAVES + 1, False)
    assert arrays.n_trees == 1 and arrays.node_off.tolist() == [0, 2 * 32769 - 1]
    assert int((arrays.taxon >= 0).sum()) == 32769 and arrays.parent[0] == -1
    tb = br.tables(arrays, "branch")
    assert tb.n_leaves == 32769 and tb.n_taxa == br.BIG_TAXA and tb.monotone


@pytest.mark.parametrize("n", br.SIZES)
def test_size_forests(n):
    for name in br.WEIGHTINGS:
        arrays = br.size_forest(n, name)
        fr.well_formed(arrays)
        tb = br.tables(arrays, br.weighting(name)[0])
        assert tb.n_taxa == n and tb.n_trees == 5
        assert np.diff(tb.tree_off).tolist() == [n, max(1, n // 2), min(n, 37), max(1, n - 1), min(n, 70)]
        assert tb.monotone == (name in ("one", "branch")) or n < 8
        assert br.coverage(tb) > br.LIST_COVERAGE
        cnt = br.block_counts(tb)
        assert cnt[:, 0].tolist() == [len(br.block_rows(n, b)) for b in range(len(cnt))]  # full coverage
        if n > 64:
            assert (cnt[:, 1] < cnt[:, 0]).any()  # partial coverage
        if name == "signed" and n >= 63:
            w = to.pcg_dense(tb)[0]
            assert (w < 0).any() and (w > 0).any()
    for rb, re_ in br.size_ranges(n):
        assert 0 <= rb < re_ <= n
    if n >= 257:
        r = br.size_ranges(n)
        assert any(a % 64 and b % 64 for a, b in r) and any(a % 64 == 0 and b % 64 == 0 for a, b in r)


@pytest.mark.parametrize("kind", ["star", "caterpillar", "balanced", "random"])
def test_record_forests_hold_the_counts_they_are_named_for(kind):
    arrays = br.record_forest(kind)
    fr.well_formed(arrays)
    tb = br.tables(arrays, "branch")
    assert tb.monotone and tb.n_taxa == br.RECORD_N and tb.n_trees == 7
    cnt = br.block_counts(tb)
    assert cnt.shape == (5, 7)
    assert cnt[br.RECORD_BLOCK].tolist() == [0, 1, 2, 63, 64, 64, 64]
    others = np.delete(cnt, br.RECORD_BLOCK, axis=0)
    assert (others[:, :6] == 64).all()  # the other blocks are full
    assert others[:, 6].sum() == 40
    for t in (5, 6):
        pos = br.block_positions(tb, br.RECORD_BLOCK, t)
        assert len(pos) == 64 and pos[-1] - pos[0] == 63  # consecutive in DFS order
    pos = br.block_positions(tb, br.RECORD_BLOCK, 4)
    assert pos[-1] - pos[0] > 63  # (tree 4 holds all 64 rows too, scattered)
    assert not br.tables(br.record_forest(kind, "signed"), "branch").monotone


def test_spread_forest_puts_one_row_per_64_positions():
    arrays = br.spread_forest()
    fr.well_formed(arrays)
    tb = br.tables(arrays, "branch")
    assert tb.n_taxa == br.SPREAD_N and tb.n_trees == 3 and tb.monotone
    for t in range(3):
        pos = br.block_positions(tb, br.SPREAD_BLOCK, t)
        assert pos.tolist() == list(range(0, 64 * 64, 64))
        # the search pivots (sorted ranks 7, 15, ..., 63) and the wave segments (ranks 0, 16, 32, 48) are distinct
        # positions far apart
        assert pos[7::8].tolist() == [64 * r for r in range(7, 64, 8)]
    assert len(br.tiles(br.SPREAD_N, br.SPREAD_BLOCK * 64, br.SPREAD_BLOCK * 64 + 64)) == -(-br.SPREAD_N // br.TCW)


@pytest.mark.parametrize(("strategy", "lengths"), [("one", "positive"), ("branch", "equal"), ("branch", "zero")])
def test_tie_forests_tie(strategy, lengths):
    for n in (130, 257):
        arrays = br.tie_forest(n, lengths)
        fr.well_formed(arrays)
        tb = br.tables(arrays, strategy)
        assert tb.monotone and tb.n_trees == 5
        for t in (1, 3):  # the stars: every gap of depth 1 carries the same value
            lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1]) - 1
            inner = tb.adj_depth[lo:hi] > 0
            assert inner.sum() == hi - lo - 1 and len(set(tb.adj_val[lo:hi][inner].tolist())) == 1
        if strategy == "one" or lengths == "zero":  # ... and every gap of every tree
            for t in range(5):
                lo, hi = int(tb.tree_off[t]), int(tb.tree_off[t + 1]) - 1
                inner = tb.adj_depth[lo:hi] > 0
                assert len(set(tb.adj_val[lo:hi][inner].tolist())) == 1
        if lengths == "zero":
            assert not to.pcg_dense(tb)[0].any()


def test_gapless_forests():
    want = {"ones": [1] * 5, "twos": [2] * 5}
    for which in ("ones", "twos", "first", "last", "mixed"):
        arrays = br.gapless_forest(which)
        fr.well_formed(arrays)
        tb = br.tables(arrays, "branch")
        leaves = np.diff(tb.tree_off).tolist()
        assert tb.monotone and tb.n_taxa == br.GAPLESS_N
        if which in want:
            assert leaves == want[which] and not to.pcg_dense(tb)[0].any()
            assert all(br.levels_for(k - 1) == k - 1 for k in leaves)  # m = 0: no level; m = 1: one
        if which == "first":
            assert leaves[0] == 1 and min(leaves[1:]) >= 20
        if which == "last":
            assert leaves[-1] == 1 and min(leaves[:-1]) >= 20
        if which == "mixed":
            assert sorted(leaves)[:4] == [1, 1, 2, 2]
    assert br.coverage(br.tables(br.gapless_forest("ones"), "branch")) < br.LIST_COVERAGE  # tile lists by default


def test_level_and_big_forests():
    for gaps in br.LEVEL_GAPS:
        tb = br.tables(br.level_forest(gaps), "branch")
        assert tb.n_trees == 1 and tb.n_leaves == gaps + 1 and tb.monotone
        if gaps >= 1023:
            assert tb.n_taxa == gaps + 4
        else:  # one leaf in each 64-row block, gaps shallower from left to right
            assert tb.n_taxa == 64 * (gaps + 1) + 3 and br.block_counts(tb)[: gaps + 1, 0].tolist() == [1] * (gaps + 1)
            assert tb.adj_depth[:gaps].tolist() == list(range(gaps - 1, -1, -1))
    for gaps in (1023, 2049):
        assert not br.tables(br.level_forest(gaps, "signed"), "branch").monotone
    for leaves in (br.SPARSE_FUSED_MAX_LEAVES, br.SPARSE_FUSED_MAX_LEAVES + 1):
        for mixed in (False, True):
            tb = br.tables(br.big_forest(leaves, mixed), "branch")
            sizes = np.diff(tb.tree_off)
            assert tb.n_taxa == br.BIG_TAXA and sizes.max() == leaves
            assert (sizes.max() <= br.SPARSE_FUSED_MAX_LEAVES) == (leaves == 32768)  # fused, or one launch per level
            if mixed:
                assert tb.n_trees == 21 and sizes[7] == leaves and np.delete(sizes, 7).max() <= 50 and np.delete(sizes, 7).min() >= 3
                # the small trees of the batch have fewer gaps than the large tree's upper levels are long
                assert br.levels_for(int(np.delete(sizes, 7).max()) - 1) < br.levels_for(leaves - 1)
            else:
                assert tb.n_trees == 1
    rb, re_ = br.BIG_ROWS
    assert re_ - rb <= 130 and rb % 64 and re_ % 64 and len({r // 64 for r in range(rb, re_)}) == 3


# ------------------------------------------------------------------------------------------------ degrees
def test_degree_budget_accepts_any_double_order_and_has_teeth():
    rng = np.random.RandomState(0)
    for n in br.DEGREE_SIZES + (1000,):
        arrays, lone = br.degree_forest(n)
        tb = br.tables(arrays, "branch")
        w = to.pcg_dense(tb)[0]
        assert not w[lone].any()  # the isolated taxon
        ref, budget = br.degrees_reference(w)
        assert ref.dtype == br.LD and budget[lone] == 0 and ref[lone] == 0
        for got in (w.sum(axis=1), w[:, ::-1].sum(axis=1), np.array([sum(row.tolist()) for row in w]),
                    w[:, rng.permutation(n)].cumsum(axis=1)[:, -1]):
            assert (np.abs(got.astype(br.LD) - ref) <= budget).all()
        if n < 127:
            continue
        assert (w < 0).any() and (w > 0).any()
        busy = np.flatnonzero(budget > 0)
        # a dropped last column (the scalar tail of an odd n), a dropped row, a single-precision accumulation
        last = w[:, : n - 1].sum(axis=1)
        hit = np.flatnonzero(w[:, n - 1] != 0)
        assert len(hit) and (np.abs(last.astype(br.LD) - ref)[hit] > budget[hit]).all()
        # (a dropped row: a workgroup that skips one of its four rows, or a `row_begin` off by one, leaves every later
        # degree in its neighbour's slot -- modelled by the correct sums shifted by one; rows whose neighbour happens to
        # have nearly the same sum may stay inside, so more than half is asked, not all)
        shifted = np.roll(w.sum(axis=1), 1)
        assert (np.abs(shifted.astype(br.LD) - ref) > budget).sum() > len(busy) // 2
        f32 = w.astype(np.float32).cumsum(axis=1)[:, -1].astype(np.float64)
        assert (np.abs(f32.astype(br.LD) - ref)[busy] > budget[busy]).sum() > len(busy) // 2
    for n in br.DEGREE_SIZES:
        rows = sorted({(b - a) % 4 for a, b in br.degree_ranges(n)})
        assert rows == [0, 1, 2, 3] or n < 8
    assert all(s[0] == 0 and s[-1] == br.RANK_N and (np.diff(s) > 0).all() for s in br.RANK_SPLITS)
    assert [s[1] for s in br.RANK_SPLITS] == [1, 65, 257]


# ------------------------------------------------------------------------------------------------ the image
def test_image_reference_rounds_and_masks():
    n = 513
    tb = br.tables(br.size_forest(n, "signed", seed=1), "branch")
    w = to.pcg_dense(tb)[0]
    img, defined = br.image_reference(w, br.ld_of(n))
    assert img.dtype == np.float32 and img.shape == (n, 1024) and not img[:, n:].any()
    off = w != 0
    assert (img[:, :n].astype(np.float64) != w)[off].mean() > 0.25 and (img[:, :n].astype(np.float64) != w).mean() > 0.25
    assert defined[:512].all() and not defined[512, :512].any() and defined[512, 512:].all()
    _, full = br.image_reference(w[100:300], br.ld_of(n), 100, True)
    assert full.all()
    _, part = br.image_reference(w[500:], br.ld_of(n), 500, False)
    assert part[:12].all() and not part[12, :512].any()
    assert all(n % 2 for n in (511, 513, 1023, 1025, 1537)) and {512, 1024} <= set(br.IMAGE_SIZES)


# ------------------------------------------------------------------------------------------------ contraction
def test_contract_reference_agrees_with_the_oracle_on_signed_matrices():
    for seed, n, ng in ((1, 40, 7), (2, 64, 64), (3, 65, 1), (4, 90, 2)):
        w = br.signed_matrix(seed, n)
        gs = br.contract_groups(n, ng, seed)
        ref = br.contract_reference(w, gs)
        assert np.array_equal(ref, to.contract_dense(w, gs))
        if ng > 2:
            assert (ref < 0).any()
            zero_start = np.maximum(ref, 0.0)  # what a maximum started at 0 would give
            assert not np.array_equal(zero_start, ref)


def test_contraction_cases_hold_negative_maxima():
    tb = br.tables(br.contract_forest(), "branch")
    assert not tb.monotone
    w = to.pcg_dense(tb)[0]
    assert np.array_equal(w, w.T)
    for k in br.CONTRACT_GROUPS:
        gs = br.contract_groups(br.CONTRACT_N, k)
        assert len(gs) == k + 1 and gs[0] == 0 and gs[-1] == br.CONTRACT_N and (np.diff(gs) > 0).all()
    assert {255, 256, 257} <= set(br.CONTRACT_GROUPS)  # around the 256 threads of a workgroup
    for gs in (br.contract_groups(br.CONTRACT_N, 257), br.contract_half_and_singles(br.CONTRACT_N)):
        ref = br.contract_reference(w, gs)
        assert np.array_equal(ref, to.contract_dense(w, gs))
        assert (ref < 0).any() and not np.array_equal(np.maximum(ref, 0.0), ref)
    half = br.contract_half_and_singles(br.CONTRACT_N)
    assert half[1] == br.CONTRACT_N // 2 and (np.diff(half)[1:] == 1).all()


# ------------------------------------------------------------------------------------------------ the entry
def test_the_raw_entry_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(r"int scs_debug_graph_raw\(([^)]*)\)", text)
    assert m, "include/scs_hip.h does not declare scs_debug_graph_raw"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES["scs_debug_graph_raw"]
    assert restype is nv.C.c_int and len(argtypes) == len(params) == 5
    assert "int32_t what" in params[2] and argtypes[2] is nv.C.c_int32
    lib = nv.load_library()
    assert hasattr(lib, "scs_debug_graph_raw") and lib.scs_version() == nv.ABI_VERSION == 109
