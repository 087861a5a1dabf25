"""``tests/source_edge_reference.py`` held to the project's references, and every case of
``tests/test_gpu_source_edges.py`` shown to have the numbers it is named for.  No device: the
plans are the library's own, through its host entries; the thresholds are found from them and asserted as literals."""

import random
from math import comb

import coverage_reference as cr
import numpy as np
import parsimony_reference as pr
import pytest
import source_edge_reference as sr
import source_pairs_reference as sp
import source_triplets_reference as st

from spectralclustersupertree_amd import backend


def _first(pred, lo: int, hi: int) -> int:
    """The least x of [lo, hi] with pred(x), pred being monotone."""
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
    return lo


# ------------------------------------------------------------------------------------------------ the references
def test_nested_lists_come_back_from_their_tables():
    rng = random.Random(1)
    for _ in range(300):
        n = rng.randint(1, 14)
        tree = pr.rand_tree(rng.sample(range(20), n), rng.choice([2, 3, 5]), rng)
        tree = tree[0] if n == 1 else [[tree]] if rng.random() < 0.2 else tree  # (unary nodes leave no trace)
        back = sr.nested_of(*sr.arrays_of(tree))
        assert pr.leaves_of(back) == pr.leaves_of(tree)
        assert pr.clusters(back) == pr.clusters(tree) or n == 1


def _random_composed(rng):
    k = rng.randint(3, 12)
    pools, at = [], 0
    for i in range(k):
        s = 1 if i == 1 else rng.randint(1, 9)  # (a block of one leaf in every case)
        pools.append(list(range(at, at + s)))
        at += s

    def sub(pool):
        mine = rng.sample(pool, max(1, rng.randint(len(pool) - 2, len(pool))))  # (partial overlap)
        tree = pr.rand_tree(mine, rng.choice([2, 3, 4]), rng)
        return tree[0] if len(mine) == 1 else [tree] if rng.random() < 0.25 else tree  # (unary nodes)

    def top():
        tree = pr.rand_tree(range(k), rng.choice([2, 3, 5]), rng)
        if rng.random() < 0.3 and isinstance(tree[0], list):
            tree[0] = [tree[0]]
        return tree

    return top(), [sub(p) for p in pools], top(), [sub(p) for p in pools]


def test_pair_composed_against_quadratic_and_by_sets():
    rng = random.Random(40)
    by_sets = polytomies = 0
    for _ in range(250):
        top_a, subs_a, top_b, subs_b = _random_composed(rng)
        a, b = sr.compose(top_a, subs_a), sr.compose(top_b, subs_b)
        got = tuple(sr.pair_composed(top_a, subs_a, top_b, subs_b))
        assert got == tuple(st.pair_quadratic(a, b))
        polytomies += got[1] < comb(got[0], 3)
        if got[0] <= 16:
            by_sets += 1
            assert got == tuple(st.pair_by_sets(a, b))
    assert by_sets > 20 and polytomies > 100


def test_pair_contracted_against_quadratic_and_by_sets():
    nested_both_ways = 0
    for seed in range(120):
        n = random.Random(seed).randint(3, 40)
        fam = sr.random_family(n, seed)
        rs = np.random.RandomState(seed)
        keep = sr.contraction(fam, seed)
        mask_a, mask_b = rs.random_sample(n) < 0.8, rs.random_sample(n) < 0.7
        if min(mask_a.sum(), mask_b.sum()) == 0:
            continue
        members = [(None, mask_a), (keep, mask_b)][:: 1 if seed % 2 else -1]  # (the coarser tree as row and as column)
        a, b = (sr.nested_of(*sr.member(fam, *m)) for m in members)
        got = sr.pair_contracted(fam, *members[0], *members[1])
        assert got == tuple(st.pair_quadratic(a, b)) and got[3] == min(got[1], got[2])
        if got[0] <= 16:
            assert got == tuple(st.pair_by_sets(a, b))
        nested_both_ways += 1
    assert nested_both_ways > 100
    with pytest.raises(AssertionError, match="not nested"):
        fam = sr.random_family(30, 1)
        sr.pair_contracted(fam, sr.contraction(fam, 1), None, sr.contraction(fam, 2), None)


def test_the_judges_at_the_sizes_quadratic_still_reaches():
    # quadratic takes 0.1 s at 1 024 common leaves, 0.8 s at 2 560, 2 s at 4 097 and 13 s at 8 192: above about 4 000
    # the composed and the contracted pairs are the judges
    fam = sr.random_family(1024, 7)
    keep = sr.contraction(fam, 8)
    a, b = sr.nested_of(*sr.member(fam)), sr.nested_of(*sr.member(fam, keep))
    assert sr.pair_contracted(fam, None, None, keep, None) == tuple(st.pair_quadratic(a, b))
    pair = sr.composed_pair(2559, 4000 + 2559)
    assert pair["blocks"] == 85 and pair["cells"]["ab"] == tuple(st.pair_quadratic(*pair["trees"]))
    assert pair["cells"]["ab"] == (2559, 2710447389, 2591012318, 775961902)


def test_star_closed_forms_against_sankoff_and_hartigan():
    rng = random.Random(9)
    for m in (3, 4, 5, 9, 30):
        star = list(range(m + 2))
        parent, taxon = sr.star_arrays(m + 2)
        assert all(np.array_equal(x, y) for x, y in zip((parent, taxon), pr.preorder_arrays(star)))
        for tree in (pr.caterpillar(rng.sample(range(m + 2), m)), pr.rand_tree(rng.sample(range(m + 2), m), 3, rng)):
            ref, mine = pr.reference(parent, taxon, [tree]), sr.star_parsimony(tree)
            for k in pr.PER_TREE:
                assert ref[k].tolist() == [mine[k]]
            for k in pr.PER_CHAR:
                assert np.array_equal(ref[k], mine[k])
            assert np.array_equal(pr.hartigan(star, tree), mine["char_len"]) and mine["mrp_perfect"] == 0
        cat = sr.caterpillar_star_reference(m, True)
        taxa = rng.sample(range(m + 2), m)
        assert np.array_equal(sr.arrays_of(pr.caterpillar(taxa))[1], sr.caterpillar_arrays(taxa)[1])
        ref = pr.reference(parent, taxon, [pr.caterpillar(taxa)])
        assert all(np.array_equal(ref[k], cat[k]) for k in (*pr.PER_TREE, *pr.PER_CHAR, "char_off"))
        assert cat["mrp_length"][0] == sr.caterpillar_star_length(m)
    # a cherry costs two changes on a star, not one: nothing of a star is perfect
    assert sr.star_parsimony([[0, 1], 2, 3])["char_len"].tolist() == [2]
    m = sr.smallest_caterpillar_past_32_bits()
    assert m == 131072 and sr.caterpillar_star_reference(m, False)["mrp_length"][0] == 4295032830 > 1 << 32
    assert sr.caterpillar_star_reference(m - 1, False)["mrp_length"][0] == (1 << 32) - 2


def test_coverage_closed_form_and_signatures_against_matmul_and_sets():
    for n in (3, 4, 17, 70):
        ref = cr.by_matmul([list(range(n))], n, 1)
        assert ref["taxon_covered"].tolist() == [sr.one_tree_coverage(n)] * n
    n = sr.smallest_taxa_past_32_bits()
    assert n == 92684 and comb(n - 1, 2) == 4295022903 > 1 << 32 > comb(n - 2, 2)
    for seed in range(40):
        rng = random.Random(seed)
        n, m = rng.randint(3, 60), rng.randint(1, 9)
        sets = cr.random_sets(rng, n, m, 1, n)
        for k in (1, 2, 3):
            rows = None if seed % 2 else [rng.randrange(n) for _ in range(5)]
            mine, ref = sr.coverage_by_signatures(sets, n, k, rows), cr.by_matmul(sets, n, k, rows)
            assert all(np.array_equal(mine[key], ref[key]) and mine[key].dtype == ref[key].dtype for key in cr.KEYS)
            if n <= 14:
                assert all(np.array_equal(mine[key], cr.by_sets(sets, n, k, rows)[key]) for key in cr.KEYS)


# ------------------------------------------------------------------------------------------------ pair triplets
def _tp(n: int, **kw) -> dict:
    return backend.debug_source_pair_triplets_plan(np.array([0, n, 2 * n], dtype=np.int64), 2 * n, **kw)


def _tile(plan: dict, *names, at=(0, 0)) -> tuple:
    return tuple(int(plan[x][at]) for x in names)


def test_triplet_gates_as_the_plan_has_them():
    assert _first(lambda n: _tp(n)["zb"][0, 0] <= 31, 100, 100000) == 2560
    assert _first(lambda n: _tp(n)["zb"][0, 0] <= 1, 100, 100000) == 40960
    assert _first(lambda n: _tp(n)["lds_pairs"][0, 0] > sr.TP_LDS_BUDGET, 100, 327679) == 81920
    assert _first(lambda n: _tp(n)["lds_pairs"][0, 0] > sr.LDS_64K, 100, 327679) == 131072
    assert _first(lambda n: _tp(n)["slab"][0, 0] == 1, 100, 100000) == 18989
    assert _tile(_tp(327679), "words", "zb", "lds_pairs") == (10240, 1, sr.TP_LDS_MAX)
    with pytest.raises(ValueError, match="may share more than the 327679 taxa"):
        _tp(327680)


ZB_STEPS = {2559: (32, 80, 40960), 2560: (31, 81, 40176), 40959: (2, 1280, 40960), 40960: (1, 1281, 20496)}


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("n", list(ZB_STEPS))
def test_triplet_zb_cases(n, batched):
    case = sr.zb_step_case(n, batched)
    sizes = np.diff(case.tables.tree_off).tolist()
    assert sizes == ([n, 2, 3, n, 33, 64] if batched else [n, n]) and case.rows is None
    plan = sr.triplet_plan(case)
    assert _tile(plan, "zb", "words", "lds_pairs", "max_common") == (*ZB_STEPS[n], n) and len(plan["bstart"]) == 2
    zb = ZB_STEPS[n][0]
    large = 3 * ((n - 2 + zb - 1) // zb)  # (A, A), (A, B), (B, B)
    # (in the batch 21 pairs run, 18 of them small enough for the restrict kernel to finish)
    assert plan["chunks"][:, 6].sum() == large and plan["chunks"][:, 4].sum() == (18 if batched else 0)
    # the composed judge's cells: both trees resolve most triples, and agree on a part of them
    big = case.note["large"]
    cell = {k: int(case.ref[k][big[0], big[1]]) for k in st.KEYS}
    assert cell["common"] == n and 0 < 3 * cell["triplets_shared"] < 2 * min(cell["triplets"], cell["triplets_other"])
    own = (big[0], big[0])
    assert cell["triplets"] < comb(n, 3) and case.ref["triplets_shared"][own] == case.ref["triplets"][own]
    if batched:
        assert case.ref["common"][0].tolist() == [n, 2, 3, n, 33, 64]
        assert case.ref["triplets_shared"][4, 0] not in (0, case.ref["triplets"][4, 0])  # (the swapped pair shows)


@pytest.mark.parametrize("k", [4, 5, 6, 11])
def test_triplet_b_node_cases(k):
    case = sr.b_nodes_case(k)
    plan = sr.triplet_plan(case, lds_bytes=320)
    assert _tile(plan, "zb", "words", "lds_pairs", "slab") == (5, 4, 320, 1)
    _, hi = pr.characters(sr.nested_of_tables(case.tables)[1])  # (B's nodes below its root: all its taxa are A's)
    assert len(hi) == k and case.ref["common"][0, 1] == 100


LDS_CASES = {81919: (2560, 40960), 81920: (2561, 40976), 131071: (4096, 65536), 131072: (4097, 65552),
             327679: (10240, 163840)}


@pytest.mark.parametrize("n", list(LDS_CASES))
def test_triplet_lds_cases(n):
    case = sr.contracted_case(n)
    assert case.note["sizes"] == [n + 40, n, 33] and case.rows == [1]
    plan = sr.triplet_plan(case)
    assert _tile(plan, "zb", "words", "lds_pairs", "max_common", "tile_rows") == (1, *LDS_CASES[n], n, 1)
    # two large pairs, (B, A) and (B, B), of n - 2 workgroups each; (B, s) is finished in the restrict kernel
    assert plan["chunks"][:, 3:7].tolist() == [[3, 1, 0, 2 * (n - 2)]]
    ref = case.ref
    assert ref["common"].tolist() == [[n, n, 33]]
    assert ref["triplets"][0, 0] == ref["triplets_shared"][0, 0] == ref["triplets"][0, 1]
    assert ref["triplets_other"][0, 0] > ref["triplets"][0, 0] > 1 << 32  # (A resolves what B's contractions do not)
    assert ref["triplets_other"][0, 0] == comb(n, 3)                        # (and, binary, every triple)
    assert 0 < ref["triplets_shared"][0, 2] < ref["triplets_other"][0, 2] == comb(33, 3)


def test_triplet_restrict_gate_cases():
    for n, slab, need in ((18988, 0, 163840), (18989, 1, 163848)):
        case = sr.contracted_case(n, 0, 33, None)
        assert case.note["sizes"] == [n, n, 33] and case.rows is None
        plan = sr.triplet_plan(case)
        assert _tile(plan, "slab", "need", "lds_restrict") == (slab, need, sr.TP_LDS_MAX)
        assert sr.pair_side(n, n, sr.TP_LDS_MAX) == (not slab) and sr.pair_side(n, 33, sr.TP_LDS_MAX)
        assert 0 < case.ref["triplets_shared"][0, 1] == case.ref["triplets"][1, 1] < case.ref["triplets"][0, 0]
    case = sr.contracted_case(18000, 1100, 33, None)
    assert case.note["sizes"] == [19100, 18000, 33]
    plan = sr.triplet_plan(case)
    assert _tile(plan, "slab", "need", "lds_restrict") == (1, 164784, sr.TP_LDS_MAX)
    sides = [sr.pair_side(a, b, sr.TP_LDS_MAX) for a, b in ((19100, 19100), (19100, 18000), (18000, 18000))]
    assert sides == [False, True, True]


def test_triplet_few_common_case():
    case = sr.few_common_case()
    assert np.diff(case.tables.tree_off).tolist() == [300] * 6 and case.rows == [0]
    plan = sr.triplet_plan(case, chunk_pairs=1)
    # one pair a chunk, ten sweep workgroups counted for each whatever it shares, one region for all
    assert plan["chunks"][:, 3].tolist() == [1] * 6 and plan["chunks"][:, 6].tolist() == [10] * 6
    assert plan["region_bytes"] == plan["pair_bytes"][0, 0] and _tile(plan, "zb", "words") == (32, 10)
    assert case.ref["common"].tolist() == [[300, 300, 0, 1, 2, 65]]


# ------------------------------------------------------------------------------------------------ source pairs
def _sp(n: int, **kw) -> dict:
    return backend.debug_source_pairs_plan(np.array([0, n, 2 * n], dtype=np.int64), 2 * n, **kw)


def test_pair_gates_as_the_plan_has_them():
    assert _first(lambda n: _sp(n)["threads"][0, 0] >= 512, 10, 100000) == 2957
    assert _first(lambda n: _sp(n)["threads"][0, 0] >= 1024, 10, 100000) == 5886
    assert _first(lambda n: _sp(n)["slab"][0, 0] == 1, 10, 100000) == 23175


THREAD_STEPS = {2956: (256, 20480), 2957: (512, 20496), 5885: (512, 40960), 5886: (1024, 40976)}


@pytest.mark.parametrize("n", list(THREAD_STEPS))
def test_pair_thread_cases(n):
    case = sr.overlap_case(n, n - n // 5, n // 10)
    assert case.note["sizes"] == [n, n - n // 5 + n // 10, n - n // 5]
    plan = sr.pairs_plan(case)
    assert _tile(plan, "threads", "lds", "slab", "width") == (*THREAD_STEPS[n], 0, 2)
    ref = case.ref
    assert ref["common"][0].tolist() == [n, n - n // 5, n - n // 5] and ref["common"][0, 1] > 2 * 1024
    # B's clusters on the common taxa are A's; the random C shares none with A
    assert 0 < ref["shared"][0, 1] == ref["clusters_other"][0, 1] < ref["clusters"][0, 1] and ref["shared"][0, 2] == 0


def test_pair_slab_cases():
    for n, slab, need, wgs, stride in ((23174, 0, 163840, 0, 0), (23175, 1, 163856, 256, 163840)):
        case = sr.overlap_case(n, 20000, 1000)
        plan = sr.pairs_plan(case)
        assert _tile(plan, "slab", "need", "threads", "lds") == (slab, need, 1024, sr.TP_LDS_MAX)
        assert (int(plan["slab_wgs"]), int(plan["slab_stride"])) == (wgs, stride)
    case = sr.slab_reuse_case()
    sizes = np.diff(case.tables.tree_off).tolist()
    assert sizes == [200, 20, 150] * 6 and case.rows == list(range(18))
    plan = sr.pairs_plan(case, lds_bytes=sr.SLAB_CAP)
    in_slab = [sp.pair_bytes(a, b, 2) + sp.SP_SCRATCH > sr.SLAB_CAP for a in sizes for b in sizes]
    assert (int(plan["slab_wgs"]), sum(in_slab), _tile(plan, "slab", "lds")) == (256, 324, (1, 256))
    # workgroup 0 takes the pairs 0 and 256: trees (0, 0) of 200 leaves each, then (14, 4) of 150 and 20
    assert (sizes[256 // 18], sizes[256 % 18]) == (150, 20)
    assert case.ref["shared"][0, 2] > 0 and case.ref["shared"][1, 3] > 0 and case.ref["shared"][14, 4] > 0


@pytest.mark.parametrize("c,nblk,levels",
                         [(64, 1, 1), (65, 2, 2), (128, 2, 2), (129, 3, 2), (8192, 128, 8), (8193, 129, 8)])
def test_pair_common_count_cases(c, nblk, levels):
    case = sr.overlap_case(c + 30, c, 25)
    assert case.note["sizes"] == [c + 30, c + 25, c] and case.ref["common"][0].tolist() == [c + 30, c, c]
    # the blocks of 64 list entries the kernel fills for c common taxa, and the table levels over them
    assert ((c - 1) >> 6) + 1 == nblk and sum((1 << j) <= nblk for j in range(20)) == levels
    plan = sr.pairs_plan(case)
    assert int(plan["need"][0, 0]) == sp.pair_bytes(c + 30, c + 30, 2) + sp.SP_SCRATCH
    assert int(sr.pairs_plan(case, lds_bytes=sr.SLAB_CAP)["slab"][0, 0]) == 1


def test_pair_whole_block_and_width_cases():
    case = sr.whole_blocks_case()
    a, b, _, d = case.note["trees"]
    # D's positions by A rank: the extremes of two clusters of three blocks lie in their middle block, and the node
    # of D above the other leaves misses exactly that one
    pos_d = {x: p for p, x in enumerate(pr.leaves_of(d))}
    by_rank = np.array([pos_d[x] for x in pr.leaves_of(a)])
    assert 192 + int(np.argmin(by_rank[192:384])) == 262 and 448 + int(np.argmax(by_rank[448:640])) == 518
    assert (262 >> 6, 518 >> 6) == ((192 >> 6) + 1, (448 >> 6) + 1)
    assert [len(pr.leaves_of(x)) for x in (d[0], d[0][1], d[2], d[2][0])] == [192, 191, 192, 191]
    assert case.ref["shared"][0, 3] == 2 and case.ref["shared"][3, 0] == 2
    spans = {(lo, hi - lo + 1) for _, lo, hi in pr.layout(a)[2]}
    # (every taxon is common to the three trees: a leaf's rank in A|L is its position in A)
    assert {(0, 64), (64, 128), (192, 192), (384, 64), (448, 192)} <= spans
    assert sorted(pr.leaves_of(a)) == list(range(704))
    assert case.ref["shared"][0, 1] >= 5 and case.ref["common"].min() == 704
    case = sr.width_case()
    assert np.diff(case.tables.tree_off).tolist() == [3000, 65536]
    plan = sr.pairs_plan(case, batch_trees=1)
    assert plan["width"].tolist() == [[2, 4], [4, 4]] and plan["bstart"].tolist() == [0, 1, 2]
    assert plan["slab"].tolist() == [[0, 0], [0, 1]]  # (only the large tree with itself leaves LDS)


# ------------------------------------------------------------------------------------------------ parsimony
@pytest.mark.parametrize("deep,depth,lds,in_block", [(64, 7, 57344, 0), (128, 8, 65536, 0), (256, 9, 0, 1)])
def test_parsimony_frame_cases(deep, depth, lds, in_block):
    parent, taxon, trees, n, ref = sr.frames_case(deep)
    plan = backend.debug_parsimony_plan(pr.tables(trees, n).tree_off, parent)
    got = tuple(int(plan[k]) for k in ("frame_depth", "counter_bits", "lds_bytes", "frames_in_block"))
    assert got == (depth, 15, lds, in_block) and depth * 16 == {64: 112, 128: 128, 256: 144}[deep]
    mine = pr.plan(pr.tables(trees, n).tree_off, parent)
    assert all(int(mine[k]) == int(plan[k]) for k in ("frame_depth", "counter_bits", "lds_bytes", "frames_in_block"))
    assert ref["mrp_chars"][3] == deep - 2 and (ref["mrp_length"] > ref["mrp_chars"]).all()


def test_parsimony_arity_and_list_cases():
    for arity, bits in zip((31, 32, 63, 64, 127, 128, 255, 256), (5, 6, 6, 7, 7, 8, 8, 9)):
        parent, taxon, trees, n, _ = sr.arity_case(arity)
        assert np.bincount(parent[1:]).max() == arity
        assert backend.debug_parsimony_plan(pr.tables(trees, n).tree_off, parent)["counter_bits"] == bits
    parent, taxon, trees, n, ref = sr.list_rounds_case()
    sizes = [len(pr.leaves_of(t)) for t in trees]
    assert tuple(sizes) == sr.LIST_SIZES and [s - 1 for s in sizes if s > 5] == [256, 257, 512, 513]
    assert ref["mrp_chars"].tolist() == [0, 0, 1, 0, 2, 255, 0, 256, 0, 511, 356]


# ------------------------------------------------------------------------------------------------ coverage
NCS = {255: 512, 256: 512, 257: 512, 511: 512, 512: 512, 513: 1024, 1023: 1024, 1024: 1024, 1025: 1536}


@pytest.mark.parametrize("nc", list(NCS))
def test_coverage_compact_cases(nc):
    sets, n, compact, refs = sr.compact_case(nc)
    occurs = refs[2]["occurs"]
    assert n == nc + 40 and int((occurs >= 2).sum()) == nc == len(compact) and int((occurs >= 1).sum()) == n
    assert int((occurs == 1).sum()) == 40 and compact[0] >= 20 and compact[-2:] == [n - 2, n - 1]
    assert (nc + 511) // 512 * 512 == NCS[nc]  # the stride of the walk: the compact taxa rounded up to two chunks
    plan = backend.debug_coverage_plan(len(sets), n, min_trees=2, matrices=2)
    assert (int(plan["words"]), int(plan["variant"]), int(plan["mirror"]), int(plan["count"])) == (1, 4, 1, 1)
    assert int(backend.debug_coverage_plan(len(sets), n, min_trees=2, reg_words=1)["variant"]) == 0
    # the last row taxon and its partner sit in the last chunk of the walk and are covered together
    assert refs[2]["pair_covered"][n - 1, n - 2] > 0 and refs[2]["pair_trees"][n - 1, n - 2] >= 2
    assert 0 < refs[2]["taxon_covered"].sum() < refs[1]["taxon_covered"].sum()
    sets, _, compact, with_fillers = sr.compact_case(nc, 1030)
    plan = backend.debug_coverage_plan(len(sets), n, min_trees=2, matrices=2)
    assert len(sets) == 1038 and (int(plan["words"]), int(plan["variant"])) == (33, 64)
    assert with_fillers[2]["occurs"][compact[0]] == occurs[compact[0]] + 1030
    assert np.array_equal(with_fillers[2]["pair_covered"], refs[2]["pair_covered"])


def test_coverage_tree_count_cases():
    variants = {128: 4, 129: 8, 256: 8, 257: 16, 512: 16, 513: 32, 1024: 32, 1025: 64, 2048: 64, 2049: 0}
    for n_trees, variant in variants.items():
        sets, n = sr.tree_count_case(n_trees)
        assert len(sets) == n_trees and int(backend.debug_coverage_plan(n_trees, n)["variant"]) == variant
        held = [t for t, s in enumerate(sets) if n - 1 in s]
        assert held == [n_trees - 1]
