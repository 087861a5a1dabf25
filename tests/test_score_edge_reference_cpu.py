"""No device: every forest and supertree of ``tests/score_edge_reference.py`` has the numbers
``tests/test_gpu_score_edges.py`` runs it for, the ``words`` / ``zb`` pairs sit on both sides of
every transition, the plan restated in Python equals the library's own (``scs_debug_score_plan``) on every case, the
closed forms equal the brute-force references on small inputs, and the new entry is declared, bound and exported."""

import re
from math import comb
from pathlib import Path

import build_reference as br
import concordance_reference as qr
import numpy as np
import pytest
import score_edge_reference as se
import triplet_reference as tr

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend

ROOT = Path(__file__).resolve().parent.parent
KIB = 1024


def _starts(case: se.Case) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(case.sizes)])


# ------------------------------------------------------------------------------------------------ the host plan
def test_words_and_zb_on_both_sides_of_every_transition():
    assert [se.words_zb(n) for n in (10239, 10240, 40959, 40960)] == [(320, 8), (321, 7), (1280, 2), (1281, 1)]
    # zb 8 -> 7 and 2 -> 1 happen nowhere else near: one leaf fewer or more changes nothing
    assert se.words_zb(10238)[1] == 8 and se.words_zb(10241)[1] == 7
    assert se.words_zb(40958)[1] == 2 and se.words_zb(40961)[1] == 1
    lds = lambda n: se.words_zb(n)[1] * 16 * se.words_zb(n)[0]  # noqa: E731
    assert lds(131071) == 64 * KIB and lds(131072) == 64 * KIB + 16  # the default limit of dynamic LDS and past it
    assert lds(se.LDS_CAP) == se.TP_LDS_MAX == 160 * KIB and se.LDS_CAP == 327679
    assert 16 * ((se.LDS_CAP + 1 >> 5) + 1) > se.TP_LDS_MAX  # one leaf more is refused
    assert all(lds(n) <= 40 * KIB for n in (12000, 30000)) and lds(100_000) < 64 * KIB  # what the older tests reach
    assert [se.levels_of(n) for n in (1, 2, 3, 4, 63, 64, 1023, 1024, 2047, 2048, 2049)] == [1, 2, 2, 3, 6, 7, 10, 11, 11,
                                                                                          12, 12]


def _every_case():
    for end in se.WAVE_ENDS:
        yield se.wave_case(end)
    for size in se.LEVEL_SIZES:
        for kind in se.LEVEL_SHAPES:
            yield se.level_case(size, kind, False)
            yield se.level_case(size, kind, True)
    for gaps in se.S_GAPS:
        for kind in ("star", "caterpillar", "mixed"):
            yield se.s_gap_case(gaps, kind)
    for count in se.CHUNK_COUNTS:
        yield se.chunk_case(count, "leaves")
        yield se.chunk_case(count, "nodes")
    for size in se.SCAN_SIZES:
        yield se.scan_case(size)
    for at in se.GALLOP_AT:
        yield se.gallop_case(at, "source")
        yield se.gallop_case(at, "super")
    yield se.concordance_case()
    for size in se.ZB_QUADRATIC:
        yield se.zb_quadratic_case(size)
    for size in se.ZB_COMB:
        yield se.comb_case(size, "random", with_small=True)
    for size in se.LDS_COMB:
        yield se.comb_case(size, "blocks")


def test_the_python_plan_equals_the_librarys_on_every_case():
    n = 0
    for case in _every_case():
        off = _starts(case)
        for export in se.EXPORTS:
            for bt in case.batches:
                want = se.export_plan(export, off, case.s_leaves, bt)
                epl, ept = se.export_extras(export, want["levels"])
                got = backend.debug_score_plan(off, case.s_leaves, bt, epl, ept)
                assert sorted(got) == sorted(want)
                for k in want:
                    assert np.array_equal(got[k], want[k]), (case.name, export, bt, k, got[k], want[k])
                n += 1
    assert n > 600
    # the byte budget, with trees large enough for a handful of batches, and at the three-leaf cases' own split
    off = np.concatenate([[0], np.cumsum([100_000, 3, 250_000, 1, 2, 327_679] * 40)])
    want = se.plan(off, 300_000, 0, 32, 8)
    got = backend.debug_score_plan(off, 300_000, 0, 32, 8)
    assert len(want["bstart"]) > 5 and all(np.array_equal(got[k], want[k]) for k in want)
    for export in se.EXPORTS:
        first = se.budget_first_split(export)
        for m, batches in ((first - 1, 1), (first, 2), (first + 1, 2)):
            off = 3 * np.arange(m + 1)
            want = se.export_plan(export, off, se.BUDGET_LEAVES)
            got = backend.debug_score_plan(off, se.BUDGET_LEAVES, 0, *se.export_extras(export, 2))
            assert len(want["bstart"]) - 1 == batches and want["bstart"][1] == min(first - 1, m), (export, m)
            assert all(np.array_equal(got[k], want[k]) for k in want), (export, m)


def test_the_byte_budget_cases_split_where_they_say():
    assert se.BUDGET_LEAVES % se.SC_ROW_ALIGN == 0
    rows = 4 * se.BUDGET_LEAVES
    firsts = {e: se.budget_first_split(e) for e in se.EXPORTS}
    assert firsts == {"score": 4012, "score_triplets": 4011, "score_conflicts": 4011, "score_concordance": 4012}
    for e, first in firsts.items():
        need = se.per_tree(3, se.BUDGET_LEAVES, 2, *se.export_extras(e, 2))
        assert (first - 1) * need <= se.SC_BUDGET < first * need and need - rows < 256  # the rows decide it
    # scs_score_triplets' 32 bytes a leaf move the boundary by one tree
    assert firsts["score_triplets"] == firsts["score"] - 1
    trees = se.budget_trees(60, 11, seed=2)
    assert [k for k, _ in trees] == [k for k, _ in se.budget_trees(80, 11, seed=2)[:60]]
    tb, fl = se.budget_tables(trees, 11), br.forest(0, 11, trees).flatten("one")
    gaps = np.arange(len(tb.adj_depth)) % 3 != 2
    assert np.array_equal(tb.leaf_taxon, fl.leaf_taxon) and np.array_equal(tb.tree_off, fl.tree_off)
    assert np.array_equal(tb.adj_depth[gaps], fl.adj_depth[gaps])
    assert {k for k, _ in trees} == {"caterpillar", "balanced"}


# ------------------------------------------------------------------------------------------------ the cases
def test_wave_cases_put_boundaries_on_the_lanes_they_are_named_for():
    for end in se.WAVE_ENDS:
        case = se.wave_case(end)
        sizes, starts = case.sizes, _starts(case)
        assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257} <= set(sizes.tolist())
        assert starts[-1] % se.SC_THREADS == end
        inner = starts[1:-1]
        assert (inner % 64 == 0).any() and (inner % 64 == 63).any() and (inner % se.SC_THREADS == 0).sum() >= 3
        # one- and two-leaf trees first, last and between large ones
        assert sizes[0] == 1 and sizes[1] == 2 and sizes[-1] == 1 and sizes[-2] == 2
        assert any(sizes[i] <= 2 and sizes[i - 1] >= 64 and sizes[i + 1] >= 64 for i in range(1, len(sizes) - 1))
        m = len(sizes)
        assert case.batches == (0, 1, 2, m - 1, m, m + 1)
        # the supertree: binary nodes, polytomies, unary nodes, taxa no source can name
        kids = np.bincount(case.parent[1:], minlength=len(case.parent))
        assert (kids == 1).any() and (kids == 2).any() and (kids >= 3).any()
        assert (case.taxon >= case.arrays.n_taxa).sum() == 11
        # batches of two start trees on other lanes than the whole forest does
        two = se.export_plan("score", starts, case.s_leaves, 2)["bstart"]
        assert len(two) - 1 == (m + 1) // 2


def test_level_cases_sit_around_the_powers_of_two():
    around = {2 ** k + d for k in (2, 6, 10, 11) for d in (-1, 0, 1)}
    assert around == set(se.S_GAPS) and around | {2 ** k + 2 for k in (2, 6, 10, 11)} == set(se.LEVEL_SIZES)
    # the longest stretch of a star or a caterpillar (n - 2 gaps) needs the top level of 2^levels > n from 2^k + 2 on
    assert all(n - 2 < 2 ** (se.levels_of(n) - 1) for n in (64, 65, 2048, 2049))
    assert all(n - 2 >= 2 ** (se.levels_of(n) - 1) for n in (63, 66, 1023, 1026, 2047, 2050))
    for size in se.LEVEL_SIZES:
        for kind in se.LEVEL_SHAPES:
            for among in (False, True):
                case = se.level_case(size, kind, among)
                sizes = case.sizes
                assert sizes.max() == size and ((sizes == size).sum() == 1 or size == 3)
                assert len(sizes) == (1 + se.LEVEL_SMALL if among else 1)
                assert not among or (np.delete(sizes, se.LEVEL_SMALL // 2) == 3).all()
                p = se.export_plan("score", _starts(case), case.s_leaves)
                assert p["levels"] == se.levels_of(size) and 2 ** (p["levels"] - 1) <= size < 2 ** p["levels"]
            if kind == "star":  # one stretch over every gap but the last
                tb = se.level_case(size, "star", False).tables()
                assert len(set(tb.adj_depth[: size - 2].tolist())) == 1 and tb.adj_depth[size - 2] < tb.adj_depth[0]
    for gaps in se.S_GAPS:
        for kind in ("star", "caterpillar", "mixed"):
            case = se.s_gap_case(gaps, kind)
            assert case.s_leaves - 1 == gaps and case.sizes.max() == gaps + 1
        par, _ = se.supertree("star", np.arange(gaps + 1))
        assert (par[2:-1] == 1).all() and par[-1] == 0


def test_chunk_cases_fill_the_chunks_they_are_named_for():
    assert {1023, 1024, 1025, 2047, 2048, 2049, 1, 2, 3} == set(se.CHUNK_COUNTS)
    for count in se.CHUNK_COUNTS:
        nodes = se.chunk_case(count, "nodes")
        assert len(nodes.parent) == count and nodes.s_leaves == max(1, count // 3)
        kids = np.bincount(nodes.parent[1:], minlength=count) if count > 1 else np.zeros(1)
        assert count < 1000 or (kids == 1).sum() > 100  # the count is reached through unary chains
        case = se.chunk_case(count, "leaves")
        assert case.s_leaves == count
        n_taxa = case.arrays.n_taxa
        pos = se.s_positions(case.taxon, n_taxa)
        tb = case.tables()
        where = [pos[tb.leaf_taxon[tb.tree_off[t]:tb.tree_off[t + 1]]] for t in range(tb.n_trees)]
        assert all((w >= 0).all() for w in where)
        assert max(w.max() for w in where[:2]) < se.SC_ROW_ALIGN
        if count > se.SC_ROW_ALIGN:
            assert tb.n_trees == 6
            assert min(w.min() for w in where[2:4]) >= se.SC_ROW_ALIGN  # the first chunk's total is 0
            assert {se.SC_ROW_ALIGN - 1, se.SC_ROW_ALIGN} <= set(where[4].tolist())
            assert (case.taxon >= n_taxa).sum() == se.CHUNK_FOREIGN and len(case.note["lone"]) == se.CHUNK_EXTRA
            assert (pos[case.note["lone"]] >= 0).all() and not np.isin(tb.leaf_taxon, case.note["lone"]).any()
        else:
            assert tb.n_trees == 2


def test_scan_and_gallop_cases():
    assert {255, 256, 257, 511, 512, 513} == set(se.SCAN_SIZES)
    for size in se.SCAN_SIZES:
        assert se.scan_case(size).sizes.tolist() == [size] * 3
    n = se.GALLOP_N
    top = se.levels_of(n) - 1
    assert 2 ** top + 1 <= n - 1  # a distance of 2^top + 1 fits
    want = {2 ** j + d for j in range(top + 1) for d in (-1, 0, 1)} - {0}
    for star_is in ("source", "super"):
        reached = {}
        for at in se.GALLOP_AT:
            case = se.gallop_case(at, star_is)
            tb = case.tables()
            assert tb.tree_off[1] == n and se.export_plan("score", _starts(case), n)["levels"] == top + 1
            s_order, t_order = case.taxon[case.taxon >= 0], tb.leaf_taxon[:n]
            star, chain = (t_order, s_order) if star_is == "source" else (s_order, t_order)
            assert star[-1] == 0 and chain[at] == 0  # the leaf outside the polytomy, and where the caterpillar has it
            reached[at] = (set(range(1, at + 1)), set(range(1, n - at)))  # distances to it from the right / left
        assert reached[0][0] == set() and reached[n - 1][1] == set()  # missing on one side
        assert want <= reached[0][1] and want <= reached[n - 1][0]
        assert all(len(a) and len(b) for k, (a, b) in reached.items() if 0 < k < n - 1)


def _concordance_events(case: se.Case):
    """``(tree, lane, category, first child?, lo == 0, hi == n - 1)`` of every decisive (tree, quartet branch), and
    the count of branches with A and B but no D, from S positions alone: the thread of a branch is the tree's first
    thread plus the S' index of the last leaf of its first child."""
    sup, trees = case.note["sup"], case.note["trees"]
    n_nodes = len(case.parent)
    kids = [[] for _ in range(n_nodes)]
    for v in range(1, n_nodes):
        kids[case.parent[v]].append(v)
    lo, hi = se.leaf_ranges(case.parent, case.taxon)
    pos = se.s_positions(case.taxon, case.arrays.n_taxa)
    tb = case.tables()
    events, no_d = [], 0
    for t, tree in enumerate(trees):
        ref = qr.brute_force(sup, [tree])
        mine = np.sort(pos[tb.leaf_taxon[tb.tree_off[t]:tb.tree_off[t + 1]]])
        inside = lambda v: (int(np.searchsorted(mine, lo[v])), int(np.searchsorted(mine, hi[v], side="right")) - 1)  # noqa: E731
        for c in range(1, n_nodes):
            u = case.parent[c]
            if len(kids[c]) != 2 or len(kids[u]) != 2:
                continue
            (a0, a1), (b0, b1) = inside(kids[c][0]), inside(kids[c][1])
            d0, d1 = inside(kids[u][1] if kids[u][0] == c else kids[u][0])
            if a1 < a0 or b1 < b0:
                continue
            if d1 < d0:
                no_d += 1
                assert ref["decisive"][c] == 0
                continue
            assert ref["decisive"][c] == 1
            cat = ("concordant" if ref["concordant"][c] else "alt1" if ref["alt1"][c] else "alt2" if ref["alt2"][c]
                   else "other")
            events.append((t, int(tb.tree_off[t] + a1) % 64, cat, kids[u][0] == c, a0 == 0, b1 == len(mine) - 1))
    return events, no_d


def test_the_concordance_case_holds_every_situation():
    case = se.concordance_case()
    kids = np.bincount(case.parent[1:], minlength=len(case.parent))
    assert set(kids.tolist()) == {0, 2} and case.s_leaves == se.CONC_TAXA
    assert {1, 2} <= set(case.sizes.tolist())
    events, no_d = _concordance_events(case)
    assert no_d > 0  # A and B but no D: not decisive
    for cat in ("concordant", "alt1", "alt2", "other"):
        mine = [e for e in events if e[2] == cat]
        assert {e[3] for e in mine} == {True, False}, cat  # first child (D after) and second child (D before)
    for lane in (0, 63):
        assert {e[2] for e in events if e[1] == lane} == {"concordant", "alt1", "alt2", "other"}, lane
    assert any(e[3] and e[4] for e in events) and any(not e[3] and e[5] for e in events)  # touching 0 and n - 1


def test_zb_and_lds_cases_land_on_their_sides():
    for size, zb in zip((*se.ZB_QUADRATIC, *se.ZB_COMB), (8, 7, 2, 1)):
        case = se.zb_quadratic_case(size) if size in se.ZB_QUADRATIC else se.comb_case(size, "random", with_small=True)
        sizes = case.sizes
        assert sizes.tolist() == [2, 3, 32, size, 33, 64] and case.note["large"] == 3
        p = se.export_plan("score_triplets", _starts(case), case.s_leaves)
        assert p["zb"].tolist() == [zb] and p["words"].tolist() == [(size >> 5) + 1]
        assert sorted({(int(n) - 1) >> 5 for n in sizes if n != size}) == [0, 1]  # the small trees' last words
        alone = se.export_plan("score_triplets", [0, size], size)
        assert alone["zb"].tolist() == [zb] and alone["workgroups"].tolist() == [-(-(size - 2) // zb)]
    kids = np.bincount(se.zb_quadratic_case(10239).parent[1:])
    assert (kids == 1).any() and (kids == 2).any() and (kids >= 3).any()
    for size in se.LDS_COMB:
        case = se.comb_case(size, "blocks")
        assert case.sizes.tolist() == [size] and case.s_leaves == size
        assert not np.array_equal(case.note["t_order"], np.arange(size))


def test_refusal_tables_differ_in_one_leaf():
    for kind in se.REFUSALS:
        for bad_tree in (1, 7):
            parent, taxon, arrays, good, bad = se.refusal_tables(kind, bad_tree)
            diff = np.flatnonzero(good.leaf_taxon != bad.leaf_taxon)
            assert len(diff) == 1 and good.tree_off[bad_tree] <= diff[0] < good.tree_off[bad_tree + 1]
            assert bad_tree // se.REFUSAL_BATCH == (0 if bad_tree == 1 else 2) and good.n_trees == se.REFUSAL_TREES
            x = int(bad.leaf_taxon[diff[0]])
            pos = se.s_positions(taxon, good.n_taxa + 1)
            mine = bad.leaf_taxon[bad.tree_off[bad_tree]:bad.tree_off[bad_tree + 1]]
            assert {"range": x == good.n_taxa, "missing": x < good.n_taxa and pos[x] < 0,
                    "twice": (mine == x).sum() == 2}[kind]
            assert (pos[good.leaf_taxon] >= 0).all()


# ------------------------------------------------------------------------------------------------ the closed forms
def test_dominance_and_permutations():
    rs = np.random.RandomState(0)
    for m in (1, 2, 3, 7, 64, 65, 100, 333):
        a = rs.permutation(m)
        assert se.dominance(a).tolist() == [int((a[:i] < a[i]).sum()) for i in range(m)]
    for kind in ("random", "blocks", "interleave"):
        p = se.permutation(kind, 500, seed=1)
        assert sorted(p.tolist()) == list(range(500)) and not np.array_equal(p, np.arange(500))


def test_comb_closed_forms_equal_brute_force():
    rs = np.random.RandomState(1)
    exports = ("score", "score_triplets", "score_conflicts")
    for _ in range(300):
        m = int(rs.randint(3, 10))
        s_order, t_order = rs.permutation(m).astype(np.int32), rs.permutation(m).astype(np.int32)
        parent, taxon = se.supertree("caterpillar", s_order)
        ref = se.reference(parent, taxon, br.forest(0, m, [("caterpillar", t_order)]), exports)
        got = se.comb_pair(s_order, t_order, m)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (k, s_order, t_order)


@pytest.mark.parametrize("kind", ["random", "blocks", "interleave"])
def test_comb_closed_forms_equal_the_quadratic_references(kind):
    m = 301
    t_order = se.permutation(kind, m, seed=4)
    case = se.comb_case(m, kind)
    assert np.array_equal(case.note["t_order"], se.permutation(kind, m, seed=m))
    parent, taxon = se.supertree("caterpillar", np.arange(m))
    arrays = br.forest(0, m, [("caterpillar", t_order)])
    ref = se.reference(parent, taxon, arrays, ("score", "score_triplets", "score_conflicts"))
    got = se.comb_pair(np.arange(m), t_order, m)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert got["t_super"][0] == comb(m, 3) and 0 < got["t_shared"][0] < comb(m, 3)
    # a planted error in one I(y, z) changes the sum: the terms are not all of one kind
    assert 0 <= got["shared"][0] < m - 2
    # the case with small trees around it: closed form and references put together equal the references alone
    both = se.comb_case(65, kind, with_small=True)
    ref = se.reference(both.parent, both.taxon, both.arrays, ("score", "score_triplets", "score_conflicts"))
    got = se.comb_case_reference(both)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_three_leaf_closed_forms_equal_brute_force():
    rs = np.random.RandomState(2)
    seen = {k: 0 for k in se.CONCORDANCE}
    for it in range(40):
        r = int(rs.randint(4, 12))
        s_order = rs.permutation(r).astype(np.int32)
        trees = se.budget_trees(25, r, seed=it)
        parent, taxon = se.supertree("caterpillar", s_order)
        ref = se.reference(parent, taxon, br.forest(0, r, trees))
        got = se.three_leaf_closed_form(s_order, trees, r)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (k, it)
        for k in seen:
            seen[k] += int(ref[k].sum())
    assert min(seen.values()) > 0, seen


def test_references_agree_where_both_apply():
    # `reference` takes brute force up to 12 leaves and linear / quadratic above: the same numbers at the seam
    case = se.s_gap_case(5, "mixed")
    tiny = se.reference(case.parent, case.taxon, case.arrays)
    sup, trees = se.to_node(case.parent, case.taxon), se.source_nodes(case.arrays)
    assert sup.to_flat()[0] == case.parent.tolist()
    quad = tr.quadratic(sup, trees)
    assert all(np.array_equal(tiny[k], quad[k]) for k in se.TRIPLETS)
    par, leaf = se.insert_unary(*br.shape("balanced", 5), 3, 4)
    assert len(par) == 13 and leaf.sum() == 5 and (par[1:] < np.arange(1, 13)).all() and par[3:8].tolist() == [1, 3, 4, 5, 6]


# ------------------------------------------------------------------------------------------------ the entry
def test_the_plan_entry_is_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(r"int scs_debug_score_plan\(([^)]*)\)", text)
    assert m, "include/scs_hip.h does not declare scs_debug_score_plan"
    params = [p.strip() for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES["scs_debug_score_plan"]
    assert restype is nv.C.c_int and len(argtypes) == len(params) == 13
    assert params[0] == "const scs_tables *sources" and "int64_t extra_per_leaf" in params[5]
    assert argtypes[5] is nv.C.c_int64 and argtypes[6] is nv.C.c_int64
    lib = nv.load_library()
    assert hasattr(lib, "scs_debug_score_plan") and lib.scs_version() == nv.ABI_VERSION == 109
    # neither tables nor offsets: refused, not read
    assert lib.scs_debug_score_plan(None, 0, None, 1, 0, 0, 0, None, None, None, None, None, None) == nv.EINVAL
