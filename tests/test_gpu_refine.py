"""``scs_score_clade_moves`` against numpy on the rows of ``scs_score_clade_placements`` of the same test, and
``refine_supertree`` against the host reference loop of ``tests/refine_reference.py`` move for move; exact equality."""

import numpy as np
import pytest
import refine_reference as rr
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import _native, load_trees, refine_supertree, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.refine import apply_moves, subtree_ends
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _check_moves(dev, sup, trees, queries, ks=(1, 2, 8), **kw):
    """The moves call against numpy on the rows the placements call returns for the same inputs; returns the rows and
    the last moves."""
    parent, taxon, tips = supertree_arrays(sup)
    tables = dev.upload(flatten_trees(trees, [1.0] * len(trees), "one", taxa=tips))
    try:
        rows = dev.score_clade_placements(tables, parent, taxon, queries, **kw)
        end = subtree_ends(parent)
        d = rows["cp_super"] - 2 * rows["cp_shared"]
        at = np.arange(len(queries))
        for k in ks:
            mv = dev.score_clade_moves(tables, parent, taxon, queries, top_k=k, **kw)
            assert mv["mv_node"].dtype == np.int32 and mv["mv_node"].shape == (len(queries), k)
            for key in ("cp_trees", "cp_total", "cp_source"):
                assert np.array_equal(mv[key], rows[key]), (k, key)
            assert np.array_equal(mv["mv_own_super"], rows["cp_super"][at, queries]), k
            assert np.array_equal(mv["mv_own_shared"], rows["cp_shared"][at, queries]), k
            want = np.stack([rr.top_k(d[i], q, end[q], k) for i, q in enumerate(queries)])
            assert np.array_equal(mv["mv_node"], want), (k, np.argwhere(mv["mv_node"] != want)[:5])
            there = np.maximum(want, 0)
            for key, row in (("mv_super", "cp_super"), ("mv_shared", "cp_shared")):
                assert np.array_equal(mv[key], np.where(want >= 0, rows[row][at[:, None], there], 0)), (k, key)
    finally:
        tables.free()
    return rows, mv


@pytest.mark.parametrize("n_nodes", [3, 63, 64, 65, 255, 256, 257, 1025])
def test_moves_are_the_top_k_of_the_rows(dev, n_nodes):
    # a binary tree on t taxa has 2 t - 1 nodes; an even count takes a unary root above it.  The root's children are
    # a clade of all taxa but one (node 1: the first range of a row; the root and the last tip are its only
    # candidates, fewer than K) and that taxon (the last node: a tip, the last range)
    rs = np.random.RandomState(n_nodes)
    t = (n_nodes + 1) // 2
    names = _names(t)
    body = TreeNode(None, [sr.random_tree(rs, names[:-1], binary=True), TreeNode(names[-1])]) if t > 2 else \
        TreeNode(None, [TreeNode(names[0]), TreeNode(names[1])])
    sup = TreeNode(None, [body]) if n_nodes % 2 == 0 else body
    parent, taxon, _ = supertree_arrays(sup)
    assert len(parent) == n_nodes
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(t, size=max(2, min(t, 3 * t // 4)), replace=False)])
             for _ in range(3)]
    end = subtree_ends(parent)
    size = end - np.arange(n_nodes)
    first = 1 + (n_nodes % 2 == 0)          # the clade of all taxa but one (below the unary root when there is one)
    inner = [int(v) for v in np.flatnonzero((size > 1) & (size < n_nodes // 2))]
    tip_nodes = [int(v) for v in np.flatnonzero(taxon >= 0)]
    queries = {1, first, n_nodes - 1, tip_nodes[0], tip_nodes[len(tip_nodes) // 2]}
    queries |= set(inner[:: max(1, len(inner) // 5)][:6])
    queries |= {int(v) for v in np.flatnonzero(end == n_nodes - 1)[:3]}   # subtrees that end where the last tip begins
    queries = sorted(queries - {0})
    rows, mv = _check_moves(dev, sup, trees, queries)
    i = queries.index(first)
    if n_nodes > 3:
        assert end[first] == n_nodes - 1 and mv["mv_node"][i].tolist()[:3] != [-1] * 3
        assert (mv["mv_node"][i][2 + (n_nodes % 2 == 0):] == -1).all()   # K = 8 is padded
    if n_nodes % 2 == 0:   # node 1 holds every taxon: the root is its only candidate
        assert mv["mv_node"][queries.index(1)].tolist() == [0] + [-1] * 7


def test_equal_rows_tie_across_lanes_waves_and_strides(dev):
    # the root holds AB = (A, B) and C; A has 35 tips (nodes [2, 71)), B 96 (nodes [71, 262)), and the sources hold
    # taxa of C only: the rows of A, B and AB are zero, and their winners are the lowest indices outside the subtree,
    # which begin at lane 7 of the second wave (A), run up to a gap (B) and start in the second stride of 256 (AB)
    rs = np.random.RandomState(5)
    names = _names(400)
    a = sr.random_tree(rs, names[:35], binary=True)
    b = sr.random_tree(rs, names[35:131], binary=True)
    c = sr.random_tree(rs, names[131:], polytomy=0.3, unary=0.0)
    sup = TreeNode(None, [TreeNode(None, [a, b]), c])
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(np.arange(131, 400), size=90, replace=False)])
             for _ in range(4)]
    parent, taxon, _ = supertree_arrays(sup)
    end = subtree_ends(parent)
    assert (end[1], end[2], end[71]) == (262, 71, 262)
    tip = int(np.flatnonzero(taxon >= 0)[10])
    size = end - np.arange(len(parent))
    in_c = int(np.flatnonzero((np.arange(len(parent)) > 262) & (size >= 40) & (size < 300))[0])
    queries = [2, 71, 1, tip, in_c]
    rows, mv = _check_moves(dev, sup, trees, queries)
    assert not rows["cp_super"][:4].any() and rows["cp_trees"][:4].tolist() == [0] * 4 and rows["cp_trees"][4] > 0
    assert mv["mv_node"][0].tolist() == [0, 1, 71, 72, 73, 74, 75, 76]
    assert mv["mv_node"][1].tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert mv["mv_node"][2].tolist() == [0, 262, 263, 264, 265, 266, 267, 268]
    assert not mv["mv_super"][:4].any() and not mv["mv_shared"][:4].any()
    # a star: every row is constant over the other tips
    star = TreeNode(None, [TreeNode(x) for x in names[:300]])
    few = [sr.random_tree(rs, [names[i] for i in rs.choice(299, size=40, replace=False)]) for _ in range(3)]
    rows, mv = _check_moves(dev, star, few, [1, 64, 65, 257, 300])
    assert mv["mv_node"][4].tolist() == [0, 1, 2, 3, 4, 5, 6, 7] and rows["cp_trees"][4] == 0   # no source holds it


@pytest.fixture(scope="module")
def passes():
    """A supertree on 400 taxa whose root holds clades of 1, 2, 63, 64, 65 and 130 tips and the 75 other taxa, five
    sources on 150 taxa each, and the six clades as queries: 325 sub-queries, so the clade of 130 spans passes."""
    rs = np.random.RandomState(64)
    names = _names(400)
    parts, at = [], 0
    for k in (1, 2, 63, 64, 65, 130):
        parts.append(sr.random_tree(rs, names[at:at + k], polytomy=0.2, unary=0.05) if k > 1 else TreeNode(names[at]))
        at += k
    sup = TreeNode(None, [*parts, sr.random_tree(rs, names[at:], binary=True)])
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(400, size=150, replace=False)]) for _ in range(5)]
    nodes = sr._preorder(sup)
    queries = [next(i for i, v in enumerate(nodes) if v is p) for p in parts]
    return sup, trees, queries


@pytest.mark.parametrize(("batch_trees", "lds_bytes"), [(0, 0), (2, 0), (7, 0), (0, 4096), (0, 80), (2, 80)])
def test_batches_lds_plans_and_clades_that_span_passes(dev, passes, batch_trees, lds_bytes):
    sup, trees, queries = passes
    more = trees + trees[:3] if batch_trees == 7 else trees   # (eight trees: a batch of seven and one more)
    _check_moves(dev, sup, more, queries, ks=(2,), batch_trees=batch_trees, lds_bytes=lds_bytes)


def test_device_refuses_bad_input(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),c);")], [1.0], "one", taxa=tips)
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match="top_k"):
            dev.score_clade_moves(tables, parent, taxon, [1], top_k=k)
    for bad in ([0], [7], [-1]):
        with pytest.raises(ValueError, match="root or out of range"):
            dev.score_clade_moves(tables, parent, taxon, bad)
    with pytest.raises(ValueError, match="twice"):
        dev.score_clade_moves(tables, parent, taxon, [1, 2, 1])
    with pytest.raises(ValueError, match="no query"):
        dev.score_clade_moves(tables, parent, taxon, [])
    with pytest.raises(ValueError, match="max_lds_bytes"):
        dev.score_clade_moves(tables, parent, taxon, [1], lds_bytes=8)
    out = dev.score_clade_moves(tables, parent, taxon, [4], top_k=8)   # (c,d): c against (a,b)
    assert out["mv_node"].tolist() == [[0, 1, 2, 3, -1, -1, -1, -1]]    # shared 1 at the root and (a,b), 0 on a and b
    assert out["mv_own_super"].tolist() == [1] and out["mv_own_shared"].tolist() == [1]
    assert out["mv_shared"].tolist() == [[1, 1, 0, 0, 0, 0, 0, 0]]
    assert out["mv_super"].tolist() == [[1, 1, 1, 1, 0, 0, 0, 0]]


def test_the_library_exports_the_symbol(dev):
    assert hasattr(dev._lib, "scs_score_clade_moves") and "scs_score_clade_moves" in _native.SIGNATURES
    assert dev._lib.scs_version() == 109


# ------------------------------------------------------------------ refine_supertree
def _moves(result) -> list:
    return [[(m["kind"], m["node"], m["target"], m["gain"], m["tips"]) for m in r["moves"]] for r in result.rounds]


def _as_arrays(trees) -> TreeArrays:
    taxa = sorted({x for t in trees for x in t.get_tip_names()}, reverse=True)   # (ids unlike the supertree's)
    return TreeArrays.from_trees(trees, [1.0] * len(trees), taxa)


def _same_run(got, ref, what):
    assert _moves(got) == [[tuple(m) for m in r["moves"]] for r in ref["rounds"]], what
    assert [r["distance"] for r in got.rounds] == [r["distance"] for r in ref["rounds"]], what
    assert got.supertree.get_newick() == (ref["newick"] if "newick" in ref else ref["tree"].get_newick()), what
    assert (got.initial_distance, got.final_distance) == (ref["initial"], ref["final"]), what


@pytest.fixture(scope="module")
def cases():
    return rr.additivity_cases(32)


def test_refinement_is_the_reference_loop_move_for_move(dev, cases):
    # the runs of the host reference loop on these cases are recorded (``refine_reference.GOLDEN``; the CPU tests hold
    # the record to the loop), so that this test pays for the device runs only
    moves = multi = 0
    golden = rr.golden_runs()
    for n, (sup, trees) in enumerate(cases):
        kw = {"clade_max_tips": 4}
        before = sup.get_newick()
        ref = golden[n]
        got = refine_supertree(sup, trees, device=dev, **kw)
        _same_run(got, ref, n)
        _same_run(refine_supertree(sup, _as_arrays(trees), device=dev, **kw), ref, (n, "arrays"))
        assert sup.get_newick() == before
        moves += sum(len(r) for r in _moves(got))
        multi += sum(len(r) > 1 for r in _moves(got))
    assert moves >= 300 and multi >= 20, (moves, multi)


@pytest.mark.parametrize("kw", [{"nni": False}, {"top_k": 1}, {"top_k": 8, "taxa_per_round": 3, "clades_per_round": 2},
                                {"clades_per_round": 0}, {"taxa_per_round": 0, "clade_max_tips": 6}])
def test_variants_are_the_reference_loop_too(dev, cases, kw):
    kw = {"clade_max_tips": 4, "max_rounds": 2, **kw}
    for n, (sup, trees) in enumerate(cases[:6]):
        _same_run(refine_supertree(sup, trees, device=dev, **kw), rr.reference_refine(sup, trees, **kw), (n, kw))


def test_a_misplaced_tip_is_put_back_in_one_round(dev):
    rs = np.random.RandomState(7)
    kept = 0
    while kept < 12:
        case = rr.misplaced_tip_case(rs)
        if case is None:
            continue
        kept += 1
        start, trees = case
        got = refine_supertree(start, trees, taxa_per_round=len(start.get_tip_names()), device=dev)
        assert got.initial_distance > 0 and got.final_distance == 0, kept
        assert sum(bool(r["moves"]) for r in got.rounds) == 1 and len(got.rounds) == 2, kept


@pytest.fixture(scope="module")
def planted():
    """A binary model tree on 300 taxa with ten clades of up to 12 tips regrafted at random, and 40 restrictions of
    the model to 120 taxa each."""
    rs = np.random.RandomState(300)
    names = _names(300)
    model = sr.random_tree(rs, names, binary=True)
    trees = [rr.cr._restricted(model, set(rs.choice(names, size=120, replace=False).tolist())) for _ in range(40)]
    start = model
    for _ in range(10):
        parent = start.to_flat()[0]
        end = subtree_ends(parent)
        small = np.flatnonzero((end - np.arange(len(parent)) <= 23) & (np.arange(len(parent)) > 0))
        q = int(rs.choice(small))
        v = int(rs.choice([u for u in range(len(parent)) if not q <= u < end[q]]))
        start = apply_moves(start, [(q, v)])
    return start, trees


@pytest.fixture(scope="module")
def planted_run(dev, planted):
    start, trees = planted
    return refine_supertree(start, trees, device=dev)   # (a wrong prediction raises RuntimeError)


def test_planted_regrafts_on_300_taxa(dev, planted, planted_run):
    start, trees = planted
    got = planted_run
    dist = [r["distance"] for r in got.rounds] + [got.final_distance]
    assert got.initial_distance == dist[0] > 0 and len(got.rounds) >= 2
    for r, rnd in enumerate(got.rounds):
        if rnd["moves"]:
            assert dist[r + 1] == dist[r] - sum(m["gain"] for m in rnd["moves"]) < dist[r], r
        else:
            assert r == len(got.rounds) - 1 and dist[r + 1] == dist[r]
    again = score_supertree(got.supertree, trees, triplets=True, device=dev)
    assert got.final_distance == again.total_triplet_distance
    assert score_supertree(start, trees, triplets=True, device=dev).total_triplet_distance == got.initial_distance
    assert sorted(got.supertree.get_tip_names()) == sorted(start.get_tip_names())
    assert set(got.timings) == {"tables", "taxon_triplets", "branch_triplets", "clade_moves"}
    assert len(got.timings["taxon_triplets"]) == len(got.rounds) + (len(got.rounds) == 50)
    assert len(got.timings["clade_moves"]) == len(got.timings["branch_triplets"]) == len(got.rounds)
    rows = [line.split("\t") for line in got.table().splitlines()]
    assert rows[0] == ["round", "kind", "node", "target", "tips", "gain", "distance_after"]
    assert len(rows) - 1 == sum(len(r["moves"]) for r in got.rounds)
    assert {r[1] for r in rows[1:]} <= {"spr", "nni"} and int(rows[-1][6]) == got.final_distance


def test_no_round_and_no_move(dev, planted, planted_run):
    start, trees = planted
    none = refine_supertree(start, trees, max_rounds=0, device=dev)
    assert none.rounds == [] and none.initial_distance == none.final_distance > 0
    assert none.supertree.get_newick() == start.get_newick() and none.supertree is not start
    assert len(none.timings["taxon_triplets"]) == 1 and none.timings["clade_moves"] == []
    one = refine_supertree(start, trees, max_rounds=1, device=dev)
    assert len(one.rounds) == 1 and one.rounds[0]["moves"] and len(one.timings["taxon_triplets"]) == 2
    assert one.final_distance < one.initial_distance
    done = planted_run.supertree
    still = refine_supertree(done, trees, device=dev)   # a local optimum: one scoring round, no move
    assert len(still.rounds) == 1 and still.rounds[0]["moves"] == []
    assert still.initial_distance == still.final_distance and still.supertree.get_newick() == done.get_newick()
    assert len(still.timings["taxon_triplets"]) == 1
    for bad in ({"top_k": 0}, {"top_k": 9}, {"max_rounds": -1}, {"clade_max_tips": 1}):
        with pytest.raises(ValueError):
            refine_supertree(start, trees, device=dev, **bad)
    with pytest.raises(ValueError, match="not in the supertree"):
        refine_supertree(make_tree("((a,b),c);"), [make_tree("((a,b),zz);")], device=dev)
    with pytest.raises(ValueError, match="at least one tree"):
        refine_supertree(make_tree("((a,b),c);"), [], device=dev)


def test_small_batches_and_lds_plans_do_not_change_the_run(dev, cases, monkeypatch):
    sup, trees = cases[0]
    ref = rr.reference_refine(sup, trees, clade_max_tips=4, max_rounds=3)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 2)
    monkeypatch.setattr(score_mod, "CLADE_PLACEMENT_LDS_BYTES", 16)
    _same_run(refine_supertree(sup, trees, clade_max_tips=4, max_rounds=3, device=dev), ref, "small")


def test_cli_refined_out(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    plain, out, refined, log = (tmp_path / n for n in ("plain.tre", "out.tre", "refined.tre", "moves.tsv"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(plain)])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--refined-out", str(refined),
                                   "--refine-rounds", "5", "--refine-log", str(log)])
    assert res.exit_code == 0, res.output
    assert out.read_bytes() == plain.read_bytes()
    api = refine_supertree(load_tree(out), load_trees(src), max_rounds=5)
    assert load_tree(refined).get_newick() == api.supertree.get_newick() and log.read_text() == api.table()
    assert log.read_text().splitlines()[0].split("\t")[0] == "round"
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--refine-log", str(log)])
    assert res.exit_code != 0 and "--refined-out" in res.output
