"""The parsimony, source-pair, coverage and pair-triplet exports at the gates of their own plans:
``scs_score_parsimony``, ``scs_score_source_pairs``, ``scs_score_coverage`` and ``scs_score_source_pair_triplets``
called through ``Device.score_*`` with the knobs they have, every output held with ``np.array_equal`` to a host
reference that shares nothing with the kernels' decomposition (``tests/source_edge_reference.py``).  The numbers a case
is named for -- ``zb``, words, launch bytes, ``slab``, ``threads``, ``slab_wgs``, ``nblk``, frame depth, counter bits,
``nc``, ``variant`` -- are asserted on the host in ``tests/test_source_edge_reference_cpu.py``."""

from math import comb

import coverage_reference as cr
import numpy as np
import parsimony_reference as pr
import pytest
import score_edge_reference as se
import source_edge_reference as sr
import source_pairs_reference as sp
import source_triplets_reference as st

from spectralclustersupertree_amd.backend import Device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, keys, what) -> None:
    for k in keys:
        assert got[k] is not None and got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        bad = got[k] != ref[k]
        at = np.argwhere(bad)[:6].tolist()
        assert np.array_equal(got[k], ref[k]), (what, k, at, got[k][bad][:6], ref[k][bad][:6])


def _triplets(dev, case, what, settings=({},)) -> None:
    tabs = dev.upload(case.tables)
    try:
        for kw in settings:
            got = dev.score_source_pair_triplets(tabs, case.rows, **kw)
            _same(got, case.ref, st.KEYS, (what, kw))
            if case.rows is None:
                st.check_invariants(got)
    finally:
        tabs.free()


def _pairs(dev, case, what, settings=({},)) -> None:
    tabs = dev.upload(case.tables)
    try:
        for kw in settings:
            got = dev.score_source_pairs(tabs, case.rows, **kw)
            _same(got, case.ref, sp.KEYS, (what, kw))
            if case.rows is None:
                sp.check_invariants(got)
    finally:
        tabs.free()


# ================================================================================================ pair triplets
@pytest.mark.parametrize("batched", [False, True], ids=["alone", "in_a_batch"])
@pytest.mark.parametrize("n", [2559, 2560, 40959, 40960])
def test_triplet_zb_steps_against_composed_trees(dev, n, batched):
    # zb 32 | 31 and 2 | 1: two composed trees of n leaves on the same taxa, other top trees, other trees in the blocks
    case = sr.zb_step_case(n, batched)
    ab = case.ref["triplets_shared"][0, case.note["large"][1]]
    assert 0 < ab < min(case.ref["triplets"][0, 0], case.ref["triplets_other"][0, case.note["large"][1]])
    _triplets(dev, case, (n, batched))


@pytest.mark.parametrize("k", [4, 5, 6, 11], ids=["zb - 1", "zb", "zb + 1", "2 zb + 1"])
def test_triplet_b_node_counts_around_a_block_of_five(dev, k):
    # 320 bytes hold five nodes' rows of four words: zb = 5
    case = sr.b_nodes_case(k)
    assert case.ref["triplets_shared"][0, 1] > 0
    _triplets(dev, case, k, ({"lds_bytes": 320}, {}))


@pytest.mark.parametrize("n", [81919, 81920, 131071, 131072, 327679])
def test_triplet_rows_past_the_budget_past_64_kib_and_at_the_leaf_limit(dev, n):
    # the row tree B (n leaves) against A (n + 40, B's taxa among them), itself and a tree of 33 leaves
    case = sr.contracted_case(n)
    assert case.ref["common"].tolist() == [[n, n, 33]] and case.ref["triplets_shared"][0, 0] > 1 << 32
    _triplets(dev, case, n)


@pytest.mark.parametrize("n", [18988, 18989], ids=["lds", "region"])
def test_triplet_restriction_in_lds_and_in_the_region_by_itself(dev, n):
    _triplets(dev, sr.contracted_case(n, 0, 33, None), n)


def test_triplet_one_tile_with_pairs_on_both_sides_of_the_restrict_gate(dev):
    # A of 19 100 leaves makes the tile launch both kernels; (B, B) of 18 000 each stays in LDS, (A, A) does not
    _triplets(dev, sr.contracted_case(18000, 1100, 33, None), "both sides")


def test_triplet_large_trees_with_few_common_taxa_reuse_a_filled_region(dev):
    case = sr.few_common_case()
    assert case.ref["common"].tolist() == [[300, 300, 0, 1, 2, 65]] and case.ref["triplets_shared"][0, 5] > 0
    _triplets(dev, case, "few common", ({"chunk_pairs": 1}, {}, {"chunk_pairs": 1, "lds_bytes": 4096}))


# ================================================================================================ source pairs
@pytest.mark.parametrize("n", [2956, 2957, 5885, 5886])
def test_pair_thread_steps_with_gap_loops_of_several_rounds(dev, n):
    # 256 | 512 and 512 | 1 024 threads by the LDS of the largest pair; more common taxa than threads
    case = sr.overlap_case(n, n - n // 5, n // 10)
    ref = case.ref
    assert ref["common"][0, 1] == n - n // 5 > 2 * 1024 and 0 < ref["shared"][0, 1] < ref["clusters"][0, 1]
    _pairs(dev, case, n)


@pytest.mark.parametrize("n", [23174, 23175], ids=["lds", "slab"])
def test_pair_arrays_in_lds_and_in_a_slab_by_themselves(dev, n):
    _pairs(dev, sr.overlap_case(n, 20000, 1000), n)


def test_pair_slabs_are_reused_by_smaller_pairs_after_larger_ones(dev):
    case = sr.slab_reuse_case()
    _pairs(dev, case, "slab reuse", ({"lds_bytes": sr.SLAB_CAP}, {}))


@pytest.mark.parametrize("c", [64, 65, 128, 129, 8192, 8193])
def test_pair_common_counts_around_the_block_tables(dev, c):
    case = sr.overlap_case(c + 30, c, 25)
    assert case.ref["common"][0].tolist() == [c + 30, c, c] and case.ref["shared"][0, 1] > 0
    _pairs(dev, case, c, ({}, {"lds_bytes": sr.SLAB_CAP}))


def test_pair_clusters_on_whole_blocks_of_64_ranks(dev):
    case = sr.whole_blocks_case()
    assert case.ref["shared"][0, 1] >= 5
    _pairs(dev, case, "whole blocks", ({}, {"lds_bytes": sr.SLAB_CAP}))


def test_pair_tiles_of_16_and_32_bit_entries_in_one_call(dev):
    _pairs(dev, sr.width_case(), "width", ({"batch_trees": 1},))


# ================================================================================================ parsimony
def _same_mp(got: dict, ref: dict, what) -> None:
    _same(got, ref, pr.PER_TREE, what)
    if got.get("char_off") is not None:
        _same(got, ref, ("char_off", *pr.PER_CHAR), what)


def _parsimony(dev, parent, taxon, tables, ref, what, batches=(0,), chars=(True, False)) -> None:
    tabs = dev.upload(tables)
    try:
        for bt in batches:
            for ch in chars:
                _same_mp(dev.score_parsimony(tabs, parent, taxon, chars=ch, batch_trees=bt), ref, (what, bt, ch))
    finally:
        tabs.free()


@pytest.mark.parametrize("deep", [64, 128, 256])
def test_parsimony_frames_below_at_and_past_64_kib_of_lds(dev, deep):
    # depth (bits + 1) = 112 | 128 | 144: 57 344 and 65 536 bytes of LDS beside the static 128, then the call's block
    parent, taxon, trees, n, ref = sr.frames_case(deep)
    assert ref["mrp_length"][3] > ref["mrp_chars"][3] == deep - 2
    _parsimony(dev, parent, taxon, pr.tables(trees, n), ref, deep, batches=(0, 2))


@pytest.mark.parametrize("arity", [31, 32, 63, 64, 127, 128, 255, 256])
def test_parsimony_arities_around_the_counter_slices(dev, arity):
    parent, taxon, trees, n, ref = sr.arity_case(arity)
    _parsimony(dev, parent, taxon, pr.tables(trees, n), ref, arity)


def test_parsimony_caterpillar_on_a_star_carries_through_the_length_adder(dev):
    # lengths 2 .. 2 500: twelve slices of the per-character adder
    m = 5000
    parent, taxon = sr.star_arrays(m + 3)
    taxa = np.random.RandomState(5).permutation(m + 3)[:m]
    ref = sr.caterpillar_star_reference(m, True)
    assert ref["char_len"].max() == 2500 and ref["mrp_perfect"][0] == 0
    _parsimony(dev, parent, taxon, sr.tables_of([sr.caterpillar_arrays(taxa)], m + 3), ref, "caterpillar")


def test_parsimony_sources_around_the_list_rounds_and_scan_segments(dev):
    parent, taxon, trees, n, ref = sr.list_rounds_case()
    assert ref["mrp_chars"].tolist() == [0, 0, 1, 0, 2, 255, 0, 256, 0, 511, 356]
    _parsimony(dev, parent, taxon, pr.tables(trees, n), ref, "lists", batches=(0, 1, 4))


def test_parsimony_sources_past_a_list_round_on_a_star_and_in_a_batch(dev):
    # caterpillars of 258 and 514 leaves beside a tree of three: the second and third rounds of k_mp_list against the
    # closed form (every length known without a fold on the host)
    sizes = (258, 3, 514)
    parent, taxon = sr.star_arrays(600)
    rs = np.random.RandomState(258)
    taxa = [rs.permutation(600)[:m] for m in sizes]
    parts = [sr.caterpillar_star_reference(m, True) for m in sizes]
    ref = {k: np.concatenate([p[k] for p in parts]) for k in (*pr.PER_TREE, *pr.PER_CHAR)}
    ref["char_off"] = np.concatenate([[0], np.cumsum(ref["mrp_chars"])]).astype(np.int64)
    tables = sr.tables_of([sr.caterpillar_arrays(t) for t in taxa], 600)
    _parsimony(dev, parent, taxon, tables, ref, "star batch", batches=(0, 1, 2))


# (lengths from 2^32 on -- a caterpillar of 131 072 leaves on a star, the least that reaches them -- take 5.2 s without
# and 10.9 s with the per-character lengths, mostly 32 passes of one wave over 131 072 leaves: past this file's bound
# per case, so they are no case here.  DESIGN.md section 40 has the measurement and what it showed.)


# ================================================================================================ coverage
def _coverage(dev, sets, n, refs, what, rows=None, reg=0, pairs=(True, False)) -> None:
    tabs = dev.upload(cr.tables(sets, n))
    try:
        for k, ref in refs.items():
            for with_pairs in pairs:
                got = dev.score_coverage(tabs, rows, k, with_pairs, 0, reg)
                _same(got, ref, cr.KEYS if with_pairs else ("occurs", "taxon_covered"), (what, k, with_pairs))
                if with_pairs:
                    cr.check_invariants(got, n, k, rows)
    finally:
        tabs.free()


@pytest.mark.parametrize("mode", ["two_per_lane", "words_64", "streamed"])
@pytest.mark.parametrize("nc", [255, 256, 257, 511, 512, 513, 1023, 1024, 1025])
def test_coverage_compact_taxa_on_the_steps_of_the_walk(dev, nc, mode):
    sets, n, compact, refs = sr.compact_case(nc, 1030 if mode == "words_64" else 0)
    assert len(compact) == nc and compact[-1] == n - 1 and refs[2]["pair_covered"][n - 1, n - 2] > 0
    _coverage(dev, sets, n, refs, (nc, mode), reg=1 if mode == "streamed" else 0)


@pytest.mark.parametrize("n_trees", [128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049])
def test_coverage_tree_counts_on_the_register_variants(dev, n_trees):
    sets, n = sr.tree_count_case(n_trees)
    refs = {k: cr.by_matmul(sets, n, k) for k in (1, 2)}
    assert refs[1]["occurs"][n - 3:].tolist() == [1, 1, 1] and refs[1]["pair_covered"][n - 1, n - 2] >= 3
    _coverage(dev, sets, n, refs, n_trees)


def test_coverage_with_k_above_every_occurs(dev):
    sets, n = sr.tree_count_case(129)
    ref = cr.by_matmul(sets, n, 1)
    k = int(ref["occurs"].max()) + 1
    refs = {k: cr.by_matmul(sets, n, k)}
    assert not refs[k]["pair_covered"].any() and refs[k]["pair_trees"].any()
    _coverage(dev, sets, n, refs, "k above")
    _coverage(dev, sets, n, {k: cr.by_matmul(sets, n, k, [n - 1, 0])}, "k above, rows", rows=[n - 1, 0], reg=1)


def test_coverage_counts_from_2_to_the_32_on(dev):
    n = sr.smallest_taxa_past_32_bits()
    assert n == 92684 and sr.one_tree_coverage(n) == comb(n - 1, 2) == 4295022903 > 1 << 32
    rows = [0, n // 2, n - 1]
    ref = {"occurs": np.ones(n, dtype=np.int32), "taxon_covered": np.full(3, comb(n - 1, 2), dtype=np.int64)}
    tabs = dev.upload(sr.tables_of([(np.random.RandomState(9).permutation(n), np.zeros(n - 1))], n))
    try:
        _same(dev.score_coverage(tabs, rows), ref, ("occurs", "taxon_covered"), "2^32")
    finally:
        tabs.free()


# ================================================================================================ refusals
def _refusal_calls(dev, parent, taxon):
    return {
        "scs_score_parsimony": lambda tabs, bt: dev.score_parsimony(tabs, parent, taxon, chars=True, batch_trees=bt),
        "scs_score_source_pairs": lambda tabs, bt: dev.score_source_pairs(tabs, batch_trees=bt),
        "scs_score_coverage": lambda tabs, bt: dev.score_coverage(tabs, None, 2, True),
        "scs_score_source_pair_triplets": lambda tabs, bt: dev.score_source_pair_triplets(tabs, batch_trees=bt),
    }


@pytest.mark.parametrize("bad_tree", [1, 7], ids=["first_batch", "third_batch"])
@pytest.mark.parametrize("export", ["scs_score_parsimony", "scs_score_source_pairs", "scs_score_coverage",
                                    "scs_score_source_pair_triplets"])
def test_a_taxon_twice_in_the_first_and_in_a_later_batch(dev, export, bad_tree):
    parent, taxon, _, good, bad = se.refusal_tables("twice", bad_tree)
    call = _refusal_calls(dev, parent, taxon)[export]
    tabs = dev.upload(bad)
    try:
        used = dev.arena_stats()["used_bytes"]
        with pytest.raises(ValueError, match=f"^{export}: a source tree has a taxon twice$"):
            call(tabs, se.REFUSAL_BATCH)
        assert dev.arena_stats()["used_bytes"] == used  # the call's block went back
    finally:
        tabs.free()
    trees = sr.nested_of_tables(good)
    n = int(good.n_taxa)
    ref, keys = {
        "scs_score_parsimony": lambda: (pr.reference(parent, taxon, trees), (*pr.PER_TREE, "char_off", *pr.PER_CHAR)),
        "scs_score_source_pairs": lambda: (sp.linear(good), sp.KEYS),
        "scs_score_coverage": lambda: (cr.by_matmul([pr.leaves_of(t) for t in trees], n, 2), cr.KEYS),
        "scs_score_source_pair_triplets": lambda: (st.quadratic(trees), st.KEYS),
    }[export]()
    tabs = dev.upload(good)
    try:
        for bt in (se.REFUSAL_BATCH, 0):
            _same(call(tabs, bt), ref, keys, (export, bt))
    finally:
        tabs.free()
