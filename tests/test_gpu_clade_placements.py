"""Clade placement support on the device (``scs_score_clade_placements``), held to the host references of
``tests/clade_placement_reference.py``, to ``scs_score_placements`` for tips and to ``scs_score_triplets`` on edited
trees, by exact equality."""

import clade_placement_reference as cr
import numpy as np
import pytest
import score_reference as sr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import _native, load_trees, score_supertree, synthetic
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.flatten import flatten_trees
from spectralclustersupertree_amd.load import load_tree_arrays
from spectralclustersupertree_amd.score import _leaf_ranges, supertree_arrays
from spectralclustersupertree_amd.tree import TreeNode, load_tree, make_tree

pytestmark = pytest.mark.gpu

KEYS = cr.KEYS


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(res, ref, what=""):
    for k in KEYS:
        got = getattr(res, k)
        assert got.dtype == np.int64 and got.shape == ref[k].shape, (what, k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (what, k, np.argwhere(got != ref[k])[:10])


def _names(n: int) -> list[str]:
    return [synthetic.taxon_name(i) for i in range(n)]


def _caterpillar(names) -> TreeNode:
    node = TreeNode(names[0])
    for x in names[1:]:
        node = TreeNode(None, [node, TreeNode(x)])
    return node


def _sizes(sup: TreeNode) -> np.ndarray:
    lo, hi = _leaf_ranges(np.asarray(sup.to_flat()[0], dtype=np.int64))
    return hi - lo + 1


def _node_of(sup: TreeNode, names) -> int:
    """The topmost preorder node whose cluster is ``names``."""
    want = frozenset(names)
    nodes = sr._preorder(sup)
    sets = sr._leaf_sets(nodes)
    return next(i for i, v in enumerate(nodes) if sets[id(v)] == want)


def test_random_small_cases_match_brute_force(dev):
    rs = np.random.RandomState(41)
    crossed = 0
    for i in range(150):
        sup, trees = sr.random_case(rs, n_taxa=int(rs.randint(2, 11)))
        queries = list(range(1, len(sr._preorder(sup))))
        res = score_supertree(sup, trees, clade_placements=queries, device=dev)
        assert res.cp_nodes.tolist() == queries, i
        _same(res, cr.brute_force(sup, trees, queries), i)
        crossed += int((res.cp_trees > 0).sum())
    assert crossed > 500, crossed


@pytest.mark.parametrize(("sup_file", "src_file"), [
    ("dcm_model_tree.tre", "dcm_source_trees.tre"),
    ("dcm_iq_expected.tre", "dcm_iq_source.tre"),
    ("supertriplets_expected.tre", "supertriplets_source.tre"),
])
def test_reference_fixtures(dev, sup_file, src_file):
    sup = load_tree(DATA_DIR / sup_file)
    trees = load_trees(DATA_DIR / src_file)
    size = _sizes(sup)
    inner = np.flatnonzero((size >= 2) & (size <= 12))  # (small ones: the host reference works tip by tip)
    queries = sorted(int(q) for q in np.random.RandomState(3).permutation(inner)[:12])
    ref = cr.composed(sup, trees, queries)
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, sup_file)
    _same(score_supertree(sup, load_tree_arrays(DATA_DIR / src_file), clade_placements=queries, device=dev), ref,
          sup_file)


@pytest.mark.parametrize("m", [3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257])
def test_word_and_wave_edges(dev, m):
    rs = np.random.RandomState(m)
    names = _names(m)
    trees = [sr.random_tree(rs, names, binary=True), sr.random_tree(rs, names, polytomy=0.5, unary=0.0)]
    sup = sr.random_tree(rs, names, polytomy=0.4)
    size = _sizes(sup)
    pick = [int(np.flatnonzero(size == s)[0]) for s in sorted(set(size[1:].tolist()))[:: max(1, m // 12)]]
    queries = sorted({1, len(size) - 1, int(np.argmax(size[1:])) + 1, *pick} - {0})
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), cr.composed(sup, trees, queries), m)


@pytest.fixture(scope="module")
def passes():
    """A supertree on 400 taxa whose root holds clades of 1, 2, 63, 64, 65 and 130 tips and the 75 other taxa, five
    sources on 150 taxa each, the six clades as queries and the host reference."""
    rs = np.random.RandomState(64)
    names = _names(400)
    parts, at = [], 0
    for k in (1, 2, 63, 64, 65, 130):
        parts.append(sr.random_tree(rs, names[at:at + k], polytomy=0.2, unary=0.05) if k > 1 else TreeNode(names[at]))
        at += k
    sup = TreeNode(None, [*parts, sr.random_tree(rs, names[at:], binary=True)])
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(400, size=150, replace=False)]) for _ in range(5)]
    queries = [_node_of(sup, p.get_tip_names()) for p in parts]
    return sup, trees, queries, cr.composed(sup, trees, queries)


def test_clades_of_one_pass_and_more(dev, passes):
    sup, trees, queries, ref = passes
    assert _sizes(sup)[queries].tolist() == [1, 2, 63, 64, 65, 130]
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, "all six")
    for i, q in enumerate(queries):  # alone, a clade starts its own first pass
        _same(score_supertree(sup, trees, clade_placements=[q], device=dev), {k: ref[k][[i]] for k in KEYS}, q)
    back = queries[::-1]
    _same(score_supertree(sup, trees, clade_placements=back, device=dev), {k: ref[k][::-1] for k in KEYS}, "reversed")


def test_more_trees_than_one_batch(dev, passes, monkeypatch):
    sup, trees, queries, ref = passes
    monkeypatch.setattr(score_mod, "BATCH_TREES", 2)
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, "batches of 2")


def test_batches_of_seven_trees(dev, monkeypatch):
    trees = synthetic.tree_objects(6, 300, 20, leaves_per_tree=120)
    sup = sr.random_tree(np.random.RandomState(10), _names(300), binary=True)
    size = _sizes(sup)
    queries = [int(q) for q in np.flatnonzero((size >= 2) & (size <= 12))[::9][:10]]
    ref = cr.composed(sup, trees, queries)
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, "one batch")
    monkeypatch.setattr(score_mod, "BATCH_TREES", 7)
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, "batches of 7")


@pytest.mark.parametrize("lds_bytes", [4096, 64, 3488])
def test_less_lds_than_the_sums_need(dev, passes, monkeypatch, lds_bytes):
    # a row pair takes 80 bytes here (150 leaves: five words), the sums of one node and 64 sub-queries 1 056: 4 096
    # bytes leave room for three nodes per workgroup; 64 bytes are less than one row pair and are refused
    sup, trees, queries, ref = passes
    monkeypatch.setattr(score_mod, "CLADE_PLACEMENT_LDS_BYTES", lds_bytes)
    if lds_bytes == 3488:
        # two batches of one call with different plans: rows of one word (trees of up to 31 leaves) leave room for
        # three nodes (272 + 3 (16 + 1 056) = 3 488), rows of three words (64 to 95 leaves) for two
        # (zb = 3 and 2, W = 1 and 3, the sums in LDS in both: the host plan worked out off the device for these six
        # sizes, by the loop this test was written against and by the library's; the results here do not show it)
        rs = np.random.RandomState(3488)
        names = _names(100)
        trees = [sr.random_tree(rs, [names[i] for i in rs.choice(100, size=n, replace=False)])
                 for n in (20, 31, 29, 64, 95, 70)]
        sup = sr.random_tree(rs, names, binary=True)
        size = _sizes(sup)
        queries = [int(q) for q in np.flatnonzero((size >= 2) & (size <= 12))[::2][:20]]
        assert size[queries].sum() >= 64  # (a full pass of sub-queries: the sums of a node take 1 056 bytes)
        ref = cr.composed(sup, trees, queries)
        monkeypatch.setattr(score_mod, "BATCH_TREES", 3)
    if lds_bytes < 80:
        with pytest.raises(ValueError, match="max_lds_bytes"):
            score_supertree(sup, trees, clade_placements=queries, device=dev)
        monkeypatch.setattr(score_mod, "CLADE_PLACEMENT_LDS_BYTES", 80)  # the rows alone: every pair sends its marks
    _same(score_supertree(sup, trees, clade_placements=queries, device=dev), ref, lds_bytes)


STRUCTURE = "((q1,q2,(q3,q4)),(((a,b),((c,(d,e)))),(f,g,(h,(i,j))),k),x1,x2);"


@pytest.mark.parametrize("lds_bytes", [None, 16])
def test_structural_edges(dev, monkeypatch, lds_bytes):
    sup = make_tree(STRUCTURE)
    trees = [make_tree(t) for t in (
        "((a,b),(c,d),(f,(g,h)));",                    # none of the clade (q1..q4)
        "((a,q3),(b,(c,f)),k);",                       # exactly one tip of it
        "((q1,q2),(q3,q4));",                          # all of it and nothing else
        "(((q1,a),(q2,(b,c))),((q3,d),(e,(q4,f))),(g,(h,(i,(j,k)))));",  # every taxon a source may hold
        "((q1,q4),(a,(q2,k)));",
        "(q1,a);",                                      # under three leaves
        "((d,e),(c,(i,j)),h);",
    )]
    nodes = sr._preorder(sup)
    # a child of the root (R small in the third tree), clades under a polytomy, one with a unary chain above it (and
    # the chain's own node), nested clades, tips, and (x1): a taxon no source holds
    queries = [_node_of(sup, s) for s in (["q1", "q2", "q3", "q4"], ["q3", "q4"], ["d", "e"], ["h", "i", "j"],
                                          ["i", "j"], ["f", "g", "h", "i", "j"], ["a", "b"], ["q1"], ["k"], ["x1"])]
    chain = _node_of(sup, ["c", "d", "e"])              # the unary node, and the clade below it
    assert len(nodes[chain].children) == 1
    queries += [chain, chain + 1]
    assert len(set(queries)) == len(queries)
    if lds_bytes:
        monkeypatch.setattr(score_mod, "CLADE_PLACEMENT_LDS_BYTES", lds_bytes)
    res = score_supertree(sup, trees, clade_placements=queries, device=dev)
    _same(res, cr.brute_force(sup, trees, queries), lds_bytes)
    assert res.cp_trees[0] == 3 and res.cp_trees[9] == 0
    for k in KEYS:
        assert not getattr(res, k)[9].any(), k  # a query no source crosses gives zero rows


@pytest.fixture(scope="module")
def deep():
    """1 500 taxa in a random order, and the caterpillar on them (the first two names its deepest cherry)."""
    names = _names(1500)
    order = [names[i] for i in np.random.RandomState(77).permutation(1500)]
    return order, _caterpillar(order)


def test_caterpillar_source(dev, deep):
    # the longest group lists: 1 498 entries for each tip of the source's deepest cherry, which is a clade of the
    # supertree; and a clade of three taxa from the middle of the source
    order, source = deep
    grown = {order[0]: order[:2], order[700]: order[700:703]}
    rest = [x for x in order if x in grown or not any(x in g for g in grown.values())]
    sup = sr.random_tree(np.random.RandomState(79), rest, polytomy=0.2, unary=0.0)
    for tip in list(sup.iter_tips()):
        if tip.name in grown:
            kids = [TreeNode(x) for x in grown[tip.name]]
            tip.name = None
            for k in kids:
                tip.append(k)
    queries = [_node_of(sup, order[:2]), _node_of(sup, order[700:703])]
    assert _sizes(sup)[queries].tolist() == [2, 3] and len(sup.get_tip_names()) == 1500
    _same(score_supertree(sup, [source], clade_placements=queries, device=dev), cr.composed(sup, [source], queries),
          "caterpillar source")


def test_caterpillar_supertree(dev, deep):
    order, sup = deep
    tree = sr.random_tree(np.random.RandomState(78), list(order), binary=True)
    deepest = _node_of(sup, order[:2])           # the deepest cherry
    higher = _node_of(sup, order[:12])           # 12 tips, 1 488 nodes above it
    queries = [deepest, higher, _node_of(sup, order[:3])]
    _same(score_supertree(sup, [tree], clade_placements=queries, device=dev), cr.composed(sup, [tree], queries),
          "caterpillar supertree")


def test_a_tip_query_is_the_taxon_placement_of_the_same_call(dev, passes):
    sup, trees, _, _ = passes
    parent, taxon, tips = supertree_arrays(sup)
    own = np.flatnonzero(taxon >= 0)
    pick = [int(i) for i in np.random.RandomState(5).choice(len(tips), size=70, replace=False)]
    res = score_supertree(sup, trees, placements=[tips[i] for i in pick], clade_placements=[int(own[i]) for i in pick],
                          device=dev)
    assert "clade_placements" in res.timings and "placements" in res.timings
    for k in KEYS:
        other = k.replace("clade_placement", "placement").replace("cp_", "pl_")
        assert np.array_equal(getattr(res, k), getattr(res, other)), k
    best, tip_best = res.best_clade_placements(), res.best_placements()
    for a, b in zip(best, tip_best):
        assert a["tips"] == 1 and all(a[k] == b[k] for k in ("node", "trees", "distance", "best_node",
                                                             "best_distance", "improvement"))


def test_edited_trees_score_what_the_placement_says(dev):
    # identity 2 through scs_score_triplets: the summed t_shared / t_super of the edited tree less those of the
    # supertree are the differences of the clade's row; t_source does not move
    rs = np.random.RandomState(56)
    names = _names(90)
    trees = [sr.random_tree(rs, [names[i] for i in rs.choice(90, size=60, replace=False)]) for _ in range(12)]
    sup = sr.random_tree(rs, names, polytomy=0.2)
    size = _sizes(sup)
    parent = np.asarray(sup.to_flat()[0], dtype=np.int64)
    queries = [int(np.flatnonzero(size == s)[0]) for s in (1, 2, 5)] + [int(np.flatnonzero(size >= 12)[-1])]
    res = score_supertree(sup, trees, triplets=True, clade_placements=queries, device=dev)
    dist = res.clade_placement_distance
    base = (int(res.t_super.sum()), int(res.t_source.sum()), int(res.t_shared.sum()))
    checked = 0
    for i, q in enumerate(queries):
        inside = cr.subtree(parent.tolist(), q)
        ancestors = []
        u = parent[q]
        while u >= 0:
            ancestors.append(int(u))
            u = parent[u]
        far = [k for k in range(len(parent)) if k not in ancestors and k not in inside]
        for v in {ancestors[0], ancestors[max(len(ancestors) - 2, 0)], 0, far[0], far[len(far) // 2], far[-1], int(np.argmin(dist[i]))}:
            if v in inside:
                continue
            again = score_supertree(res.regraft_clade(q, v), trees, triplets=True, device=dev)
            assert int(again.t_source.sum()) == base[1]
            assert int(again.t_super.sum()) - base[0] == res.cp_super[i, v] - res.cp_super[i, q], (q, v)
            assert int(again.t_shared.sum()) - base[2] == res.cp_shared[i, v] - res.cp_shared[i, q], (q, v)
            assert int(again.triplet_distance.sum()) - int(res.triplet_distance.sum()) == dist[i, v] - dist[i, q]
            checked += 1
        assert (res.cp_super[i, sorted(inside)] == res.cp_super[i, q]).all()
        assert (res.cp_shared[i, sorted(inside)] == res.cp_shared[i, q]).all()
    assert checked >= 20
    for r, q in zip(res.best_clade_placements(), queries):
        assert r["node"] == q and r["tips"] == size[q] and r["improvement"] == r["distance"] - r["best_distance"] >= 0


def test_clades_are_picked_on_request(dev, passes):
    sup, trees, _, _ = passes
    res = score_supertree(sup, trees, clade_placements=5, clade_max_tips=20, device=dev)
    assert res.tx_shared is not None and "taxon_triplets" in res.timings
    parent = np.asarray(sup.to_flat()[0], dtype=np.int64)
    want = score_mod.select_clades(5, parent, res.taxon_instability, res.tx_trees, 20)
    assert res.cp_nodes.tolist() == want.tolist() and len(want) == 5
    size = _sizes(sup)
    assert (size[want] >= 2).all() and (size[want] <= 20).all()
    _same(res, cr.composed(sup, trees, want.tolist()), "picked")
    listed = score_supertree(sup, [t.copy() for t in trees], clade_placements=want.tolist(), device=dev)
    _same(listed, {k: getattr(res, k) for k in KEYS}, "as a list")
    rows = [line.split("\t") for line in res.clade_placement_table().splitlines()]
    assert rows[0] == ["node", "tips", "trees", "distance", "best_node", "best_distance", "improvement"]
    assert [int(r[0]) for r in rows[1:]] == want.tolist()


def test_other_outputs_do_not_change_with_clade_placements(dev):
    arrays = synthetic.tree_arrays(12, 800, 60, leaves_per_tree=200)
    sup = sr.random_tree(np.random.RandomState(5), _names(800), binary=True)
    plain = score_supertree(sup, arrays, triplets=True, taxon_triplets=True, placements=3, device=dev)
    both = score_supertree(sup, arrays, triplets=True, taxon_triplets=True, placements=3, clade_placements=4,
                           device=dev)
    assert plain.cp_shared is None and plain.cp_nodes is None and "clade_placements" not in plain.timings
    for k in ("n_leaves", "n_super", "n_source", "shared", "rf", "informative", "supported", "t_super", "t_source",
              "t_shared", "tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared", "pl_taxa", "pl_super",
              "pl_shared", "pl_source"):
        assert np.array_equal(getattr(plain, k), getattr(both, k)), k
    assert both.cp_shared.shape == (4, len(both.informative))


def test_device_refuses_bad_queries(dev):
    sup = make_tree("((a,b),(c,d));")
    parent, taxon, tips = supertree_arrays(sup)
    tables = flatten_trees([make_tree("((a,b),c);")], [1.0], "one", taxa=tips)
    with pytest.raises(ValueError, match="root or out of range"):
        dev.score_clade_placements(tables, parent, taxon, [0])
    with pytest.raises(ValueError, match="root or out of range"):
        dev.score_clade_placements(tables, parent, taxon, [7])
    with pytest.raises(ValueError, match="root or out of range"):
        dev.score_clade_placements(tables, parent, taxon, [-1])
    with pytest.raises(ValueError, match="twice"):
        dev.score_clade_placements(tables, parent, taxon, [1, 2, 1])
    with pytest.raises(ValueError, match="no query"):
        dev.score_clade_placements(tables, parent, taxon, [])
    out = dev.score_clade_placements(tables, parent, taxon, [6, 1, 4])  # d: in no source; (a,b); (c,d)
    assert out["cp_trees"].tolist() == [0, 1, 1] and out["cp_shared"].shape == (3, 7)
    assert out["cp_total"].tolist() == [0, 1, 1] and out["cp_source"].tolist() == [0, 1, 1]
    # {a, b, c} has two taxa in (a,b): resolved, and as the source has it, wherever the clade goes
    assert out["cp_shared"][1].tolist() == [1] * 7 and out["cp_super"][1].tolist() == [1] * 7
    assert out["cp_super"][2].tolist() == [1, 1, 1, 1, 1, 1, 1] and out["cp_shared"][2].tolist() == [1, 1, 0, 0, 1, 1, 1]


def test_the_library_exports_the_symbol(dev):
    assert hasattr(dev._lib, "scs_score_clade_placements") and "scs_score_clade_placements" in _native.SIGNATURES
    assert dev._lib.scs_version() == 109


def test_cli_clade_placements_out(tmp_path):
    src = DATA_DIR / "dcm_iq_source.tre"
    files = {i: {k: tmp_path / f"{k}.{i}" for k in ("out", "scores", "taxa")} for i in (0, 1)}
    table = tmp_path / "clades.tsv"
    for i in (0, 1):
        args = ["-i", str(src), "-o", str(files[i]["out"]), "--scores-out", str(files[i]["scores"]), "--triplets",
                "--taxa-out", str(files[i]["taxa"])]
        more = ["--clade-placements-out", str(table), "--place-clades", "3", "--clade-max-tips", "8"]
        res = CliRunner().invoke(scs, args + (more if i else []))
        assert res.exit_code == 0, res.output
    for k in files[0]:
        assert files[0][k].read_bytes() == files[1][k].read_bytes(), k
    api = score_supertree(load_tree(files[1]["out"]), load_trees(src), clade_placements=3, clade_max_tips=8)
    assert table.read_text() == api.clade_placement_table()
    rows = [line.split("\t") for line in table.read_text().splitlines()]
    assert rows[0] == ["node", "tips", "trees", "distance", "best_node", "best_distance", "improvement"]
    assert len(rows) == 4 and all(2 <= int(r[1]) <= 8 for r in rows[1:])
