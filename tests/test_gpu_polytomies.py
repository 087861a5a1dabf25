"""Polytomy support on the device (``scs_score_polytomies``) held to the numpy node sum of
``tests/polytomy_reference.py`` entry for entry, and ``resolve_polytomies`` / ``refine_supertree(resolve=True)`` held to
the plain-Python agglomeration and to a fresh scoring of the resolved tree; exact equality throughout."""

import concordance_reference as qr
import numpy as np
import polytomy_reference as pr
import pytest
import refine_reference as rr
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import (_native, refine_supertree, resolve_polytomies, score_supertree, synthetic)
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.score import supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree
from spectralclustersupertree_amd.treearrays import TreeArrays

pytestmark = pytest.mark.gpu

LDS_ALL = 160 << 10


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


@pytest.fixture(scope="module")
def cases():
    return pr.polytomy_cases(40)


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _check(dev, sup, trees, only=None, ref=None, **kw) -> dict:
    """One ``scs_score_polytomies`` call on the polytomies ``only`` (default all, in preorder) against the node sum."""
    parent, taxon, tips = supertree_arrays(sup)
    ref = ref or pr.node_sum(sup, trees, only)
    queries = ref["nodes"] if only is None else np.asarray(only)
    order = [ref["nodes"].tolist().index(int(q)) for q in queries]
    got = dev.score_polytomies(flatten_trees(trees, [1.0] * len(trees), "one", taxa=tips), parent, taxon, queries, **kw)
    assert got["py_degree"].dtype == np.int32 and got["py_trees"].dtype == np.int64
    assert got["py_degree"].tolist() == ref["degree"][order].tolist(), kw
    assert got["py_trees"].tolist() == ref["trees"][order].tolist(), kw
    for i, q in enumerate(order):
        for key, name in (("total", "py_total"), ("joint", "py_joint")):
            have = got[name][i]
            assert have.dtype == np.int64 and have.shape == ref[key][q].shape
            assert np.array_equal(have, ref[key][q]), (kw, int(queries[i]), name, np.argwhere(have != ref[key][q])[:5])
    return ref


def test_the_library_exports_the_symbol(dev):
    assert hasattr(dev._lib, "scs_score_polytomies") and "scs_score_polytomies" in _native.SIGNATURES
    assert dev._lib.scs_version() == 109


def test_random_cases_match_the_node_sum(dev, cases):
    # polytomies of 3 to 9 children, at the root and below one another, sources with fans and unary nodes that miss
    # colours; every polytomy of a tree in one call, then a few in another order
    seen = {"joint": 0, "idle": 0, "queries": 0}
    for n, (sup, trees, _) in enumerate(cases):
        ref = _check(dev, sup, trees)
        seen["joint"] += sum(int(j.sum()) for j in ref["joint"])
        seen["idle"] += int((ref["trees"] < len(trees)).sum())
        seen["queries"] += len(ref["nodes"]) > 1
        if n % 4 == 0 and len(ref["nodes"]) > 1:
            _check(dev, sup, trees, only=ref["nodes"][::-1][:3].tolist())
    assert min(seen.values()) > 0, seen


def _plan(k: int, words: int, cap: int) -> tuple:
    """(sums in LDS, odd row stride): what the sweep does with ``cap`` bytes."""
    odd, acc = words | 1, 8 * k * k
    sums = 8 * k * words + acc <= cap
    return sums, (8 * k * odd + acc <= cap) if sums else (8 * k * odd <= cap)


def _wide_case(k: int, sizes, seed: int):
    """A root of ``k`` children (clades of several tips and single tips) on 300 taxa; one source per entry of
    ``sizes`` with fans and unary nodes, one on two children only and one of two leaves."""
    rs = np.random.RandomState(seed)
    names = _names(300)
    cuts = np.sort(rs.choice(np.arange(1, 300), size=k - 1, replace=False))
    parts = np.split(np.arange(300), cuts)
    kids = [sr.random_tree(rs, [names[i] for i in p], polytomy=0.2, unary=0.1) if len(p) > 1
            else TreeNode(names[p[0]]) for p in parts]
    sup = TreeNode(None, kids)
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(300, size=m, replace=False)], polytomy=0.3, unary=0.1)
             for m in sizes]
    trees.append(sr.random_tree(rs, [names[i] for p in parts[:2] for i in p][:40]))   # two colours: not decisive
    trees.append(make_tree(f"({names[0]},{names[299]});"))
    return sup, trees


SIZES = (31, 32, 33, 63, 64, 65, 257)


@pytest.mark.parametrize("k", [3, 4, 63, 64])
def test_degrees_and_row_boundaries(dev, k):
    # the sources' sizes sit on the word and wave boundaries of a row; with 300 taxa under 63 or 64 children most
    # sources miss many colours.  All sources in one batch (rows of 9 words), then one source per batch (1, 2, 3 and
    # 9 words), in every LDS plan the sizes allow
    sup, trees = _wide_case(k, SIZES, k)
    ref = _check(dev, sup, trees, only=[0])
    assert ref["trees"][0] >= len(SIZES) and (ref["total"][0] > 0).any() and (ref["joint"][0] > 0).any()
    plans = set()
    for batch, words in ((0, 9), (1, 2)):
        part = trees if batch == 0 else [trees[2], trees[4], trees[7]]   # 33, 64 and a few leaves: at most 2 words
        part_ref = ref if batch == 0 else pr.node_sum(sup, part, [0])
        rows, acc = 8 * k * words, 8 * k * k
        for cap in (0, rows + acc, 8 * k * (words | 1) + acc, 8 * k * (words | 1), rows):
            plans.add(_plan(k, words, cap or LDS_ALL))
            _check(dev, sup, part, only=[0], ref=part_ref, lds_bytes=cap, batch_trees=batch)
    assert plans == {(True, True), (True, False), (False, True), (False, False)}, plans
    _check(dev, sup, trees, only=[0], ref=ref, batch_trees=1)


@pytest.mark.parametrize("batch_trees", [2, 7])
def test_batches(dev, cases, batch_trees):
    for sup, trees, _ in cases[:6]:
        more = (trees * 3)[:8]   # (eight trees: batches of two, or seven and one)
        _check(dev, sup, more, batch_trees=batch_trees)


def test_sources_that_are_not_decisive_leave_zeros(dev):
    sup = make_tree("((a,b,c,d),(e,f,g),h,(i,j));")
    trees = [make_tree("((a,b),e);"), make_tree("((e,f),(a,h));"), make_tree("(c,d);"), make_tree("((a,e),(h,i),j);")]
    ref = _check(dev, sup, trees)
    assert ref["nodes"].tolist() == [0, 1, 6] and ref["trees"].tolist() == [2, 0, 0]
    res = score_supertree(sup, trees, polytomies=True, triplets=True, device=dev)
    assert res.py_trees.tolist() == [2, 0, 0] and not res.py_total[1].any() and not res.py_joint[2].any()
    done = res.resolve_polytomies()
    assert {m["node"] for m in done.merges} <= {0}
    assert done.predicted_distance == score_supertree(done.supertree, trees, triplets=True,
                                                      device=dev).total_triplet_distance


def test_device_refuses_bad_input(dev):
    star = TreeNode(None, [TreeNode(n) for n in _names(65)])
    sup = make_tree("((a,b,c),(d,e),f,g);")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),(d,f),g);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="more than the 64"):
        p65, t65, tips65 = supertree_arrays(star)
        dev.score_polytomies(flatten_trees([star.copy()], [1.0], "one", taxa=tips65), p65, t65, [0])
    with pytest.raises(ValueError, match="has 2 children"):
        dev.score_polytomies(tables, parent, taxon, [0, 5])
    with pytest.raises(ValueError, match="has 0 children"):
        dev.score_polytomies(tables, parent, taxon, [2])
    with pytest.raises(ValueError, match="given twice"):
        dev.score_polytomies(tables, parent, taxon, [0, 1, 0])
    for q in (-1, len(parent)):
        with pytest.raises(ValueError, match=r"is not in \[0, "):
            dev.score_polytomies(tables, parent, taxon, [0, q])
    with pytest.raises(ValueError, match="no query node"):
        dev.score_polytomies(tables, parent, taxon, [])
    # four rows of one word: 32 bytes
    with pytest.raises(ValueError, match=r"max_lds_bytes"):
        dev.score_polytomies(tables, parent, taxon, [0, 1], lds_bytes=31)
    dev.score_polytomies(tables, parent, taxon, [0, 1], lds_bytes=32)
    with pytest.raises(ValueError, match="negative"):
        dev.score_polytomies(tables, parent, taxon, [0], lds_bytes=-1)


def _arrays(trees) -> TreeArrays:
    taxa = sorted({x for t in trees for x in t.get_tip_names()}, reverse=True)   # (ids unlike the supertree's)
    return TreeArrays.from_trees(trees, [1.0] * len(trees), taxa)


def test_resolution_is_the_reference_agglomeration(dev, cases):
    merges = 0
    for n, (sup, trees, _) in enumerate(cases):
        ref = pr.reference_resolve(sup, trees)
        before = sup.get_newick()
        for what, src in (("trees", trees), ("arrays", _arrays(trees))):
            got = resolve_polytomies(sup, src, device=dev)
            assert [(m["node"], *m["groups"], m["gain"]) for m in got.merges] == ref["merges"], (n, what)
            assert got.supertree.get_newick() == ref["tree"].get_newick(), (n, what)
            assert (got.initial_distance, got.predicted_distance) == (ref["initial"], ref["predicted"]), (n, what)
            assert got.skipped == [] and sup.get_newick() == before
        merges += len(ref["merges"])
    assert merges > 100
    sup, trees, _ = cases[0]
    few = resolve_polytomies(sup, trees, max_degree=3, min_gain=2, device=dev)
    assert all(m["gain"] >= 2 for m in few.merges)
    assert sorted(s["node"] for s in few.skipped) == [i for i, c in pr.polytomies(sup) if len(c) > 3]


@pytest.fixture(scope="module")
def collapsed():
    """300 taxa x 40 sources: a binary model with a dozen inner edges collapsed, sources planted on the model."""
    rs = np.random.RandomState(41)
    names = _names(300)
    model = sr.random_tree(rs, names, binary=True)
    sup = model.copy()
    inner = [v for v in sr._preorder(sup) if v.children and v.parent is not None]
    for i in rs.choice(len(inner), size=12, replace=False):
        c = inner[int(i)]
        up = c.parent
        at = [x is c for x in up.children].index(True)
        kids = list(c.children)
        up.children[at:at + 1] = kids
        for x in kids:
            x.parent = up
    trees = [qr.planted(rs, model, names, 0.6, 4, 0.1) for _ in range(40)]
    return sup, trees, model


def test_the_prediction_is_what_a_fresh_scoring_says(dev, collapsed):
    sup, trees, model = collapsed
    got = resolve_polytomies(sup, trees, device=dev)
    assert len(got.merges) >= 12 and got.predicted_distance < got.initial_distance
    assert got.initial_distance == score_supertree(sup, trees, triplets=True, device=dev).total_triplet_distance
    fresh = score_supertree(got.supertree, trees, triplets=True, device=dev)
    assert fresh.total_triplet_distance == got.predicted_distance
    assert max(len(v.children) for v in sr._preorder(got.supertree)) == 2
    print("collapsed", got.initial_distance, got.predicted_distance, len(got.merges), got.timings)


def _moves(result) -> list:
    return [[(m["kind"], m["node"], m["target"], m["gain"], m["tips"]) for m in r["moves"]] for r in result.rounds]


def test_refine_resolves_first_and_keeps_its_prediction(dev, collapsed, cases):
    sup, trees, _ = collapsed
    got = refine_supertree(sup, trees, resolve=True, max_rounds=2, device=dev)   # (a wrong prediction raises)
    alone = resolve_polytomies(sup, trees, device=dev)
    first = got.rounds[0]
    assert first["distance"] == got.initial_distance == alone.initial_distance
    assert [(m["kind"], m["node"], m["gain"], m["groups"]) for m in first["moves"]] == \
        [("resolve", m["node"], m["gain"], m["groups"]) for m in alone.merges]
    assert got.rounds[1]["distance"] == alone.predicted_distance >= got.final_distance
    assert got.table().splitlines()[1].split("\t")[:2] == ["0", "resolve"] and "polytomies" in got.timings
    for sup, trees, _ in cases[:6]:
        run = refine_supertree(sup, trees, resolve=True, clade_max_tips=4, device=dev)
        assert run.final_distance <= run.rounds[0]["distance"] == run.initial_distance
        assert all(m["kind"] == "resolve" for m in run.rounds[0]["moves"])


def test_refine_without_resolve_is_the_recorded_run(dev):
    golden = rr.golden_runs()
    for n, (sup, trees) in enumerate(rr.additivity_cases(6)):
        got = refine_supertree(sup, trees, clade_max_tips=4, resolve=False, device=dev)
        ref = golden[n]
        assert _moves(got) == [[tuple(m) for m in r["moves"]] for r in ref["rounds"]], n
        assert got.supertree.get_newick() == ref["newick"], n
        assert (got.initial_distance, got.final_distance) == (ref["initial"], ref["final"]), n
        assert "polytomies" not in got.timings


def test_small_batches_and_lds_plans_do_not_change_the_resolution(dev, cases, monkeypatch):
    sup, trees, _ = cases[1]
    ref = pr.reference_resolve(sup, trees)
    monkeypatch.setattr(score_mod, "BATCH_TREES", 2)
    monkeypatch.setattr(score_mod, "POLYTOMY_LDS_BYTES", 8 * 9 * 1)   # nine rows of one word: no room for the sums
    got = resolve_polytomies(sup, trees, device=dev)
    assert got.supertree.get_newick() == ref["tree"].get_newick() and got.skipped == []
    monkeypatch.setattr(score_mod, "POLYTOMY_LDS_BYTES", 8 * 3)       # three rows: larger polytomies are skipped
    got = resolve_polytomies(sup, trees, device=dev)
    assert sorted(s["node"] for s in got.skipped) == [i for i, c in pr.polytomies(sup) if len(c) > 3]
    assert all("LDS" in s["reason"] for s in got.skipped)


def test_cli_options(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    plain, out, table, resolved, refined, log = (tmp_path / n for n in (
        "plain.tre", "out.tre", "poly.tsv", "resolved.tre", "refined.tre", "moves.tsv"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(plain)])
    assert res.exit_code == 0, res.output
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--polytomies-out", str(table), "--resolved-out",
                                   str(resolved), "--resolve-min-gain", "1", "--refined-out", str(refined),
                                   "--resolve-polytomies", "--refine-rounds", "3", "--refine-log", str(log)])
    assert res.exit_code == 0, res.output
    assert out.read_bytes() == plain.read_bytes()
    rows = table.read_text().splitlines()
    assert rows[0] == "node\ti\tj\ttips\ttotal\tjoint\tgain"
    sup = load_tree(out)
    pairs = sum(len(c) * (len(c) - 1) // 2 for _, c in pr.polytomies(sup))
    assert len(rows) == 1 + pairs
    done = load_tree(resolved)
    assert sorted(done.get_tip_names()) == sorted(sup.get_tip_names())
    assert sorted(load_tree(refined).get_tip_names()) == sorted(sup.get_tip_names())
    if pairs:
        assert all(r.split("\t")[1] == "resolve" for r in log.read_text().splitlines()[1:] if r.startswith("0\t"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--resolve-polytomies"])
    assert res.exit_code != 0 and "--refined-out" in res.output
