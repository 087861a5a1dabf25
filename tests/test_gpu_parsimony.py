"""MRP parsimony scores on the device (``scs_score_parsimony``) held exactly, per tree and per
character, to Sankoff's DP of ``tests/parsimony_reference.py``: the rooted coding, characters around the 64-bit word
and the 64-word wave, several passes, every width of the frames' counters, the stack on caterpillar supertrees, frames
in the call's block, partial coverage, batches, the counts ``scs_score_supertree`` shares with it, the refusals, and
the way through ``score_supertree`` and the command line."""

import math
import random
from functools import lru_cache
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest

from click.testing import CliRunner

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, load_trees, score_supertree
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.tree import load_tree, make_tree

pytestmark = pytest.mark.gpu

DATA = Path(__file__).parent / "golden" / "reference_data"


@pytest.fixture(scope="module")
def dev():
    with Device(0) as d:
        yield d


def _same(got: dict, ref: dict, what) -> None:
    for k in pr.PER_TREE:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    if got.get("char_off") is not None:
        assert np.array_equal(got["char_off"], ref["char_off"]), (what, "char_off")
        for k in pr.PER_CHAR:
            assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (
                what, k, np.flatnonzero(got[k] != ref[k])[:8], got[k][got[k] != ref[k]][:8],
                ref[k][got[k] != ref[k]][:8])


def _check(dev, parent, taxon, trees, n_taxa, ref=None, batches=(0,), passes=(0,), what="") -> dict:
    """Both kernel variants (with and without the per-character lengths) against the reference."""
    ref = pr.reference(parent, taxon, trees) if ref is None else ref
    tabs = dev.upload(pr.tables(trees, n_taxa))
    try:
        for bt in batches:
            for pw in passes:
                _same(dev.score_parsimony(tabs, parent, taxon, chars=True, batch_trees=bt, pass_words=pw), ref,
                      (what, bt, pw, "chars"))
                _same(dev.score_parsimony(tabs, parent, taxon, batch_trees=bt, pass_words=pw), ref, (what, bt, pw))
    finally:
        tabs.free()
    return ref


# ------------------------------------------------------------------------------------------------ the coding
def test_the_outgroup_makes_the_coding_rooted(dev):
    # S = (a,(b,(c,d))), T = ((a,b),c,d): {a,b} needs two origins under an all-zero outgroup, one without it
    parent, taxon = pr.preorder_arrays([0, [1, [2, 3]]])
    ref = _check(dev, parent, taxon, [[[0, 1], 2, 3]], 4)
    assert ref["char_len"].tolist() == [2] and ref["char_lo"].tolist() == [0] and ref["char_hi"].tolist() == [1]
    assert ref["mrp_max"].tolist() == [2] and ref["mrp_perfect"].tolist() == [0]


# ------------------------------------------------------------------------------------------------ words, waves, passes
@lru_cache(maxsize=None)
def _word_case(n_chars: int, kind: str):
    m = n_chars + 2  # a binary tree of m leaves has m - 2 nontrivial clusters
    rng = random.Random(1000 + n_chars)
    taxa = list(range(m))
    rng.shuffle(taxa)
    tree = pr.caterpillar(taxa) if kind == "caterpillar" else pr.rand_tree(taxa, 2, rng)
    parent, taxon = pr.preorder_arrays(pr.rand_tree(range(m), 3, rng))
    ref = pr.reference(parent, taxon, [tree])
    assert ref["mrp_chars"].tolist() == [n_chars]
    return parent, taxon, tree, m, ref


@pytest.mark.parametrize("kind", ["caterpillar", "random"])
@pytest.mark.parametrize("n_chars", [63, 64, 65, 4095, 4096, 4097])
def test_characters_around_a_word_and_a_wave_in_one_and_several_passes(dev, n_chars, kind):
    parent, taxon, tree, m, ref = _word_case(n_chars, kind)
    assert ref["mrp_length"][0] > ref["mrp_chars"][0]
    _check(dev, parent, taxon, [tree], m, ref, passes=(0, 1, 2, 63), what=(n_chars, kind))


# ------------------------------------------------------------------------------------------------ counter bits
def _sources(rng, n_taxa: int, count: int, lo: int, hi: int, arity: int = 3) -> list:
    return [pr.rand_tree(rng.sample(range(n_taxa), rng.randint(lo, hi)), arity, rng) for _ in range(count)]


@pytest.mark.parametrize("arity", [2, 3, 4, 7, 8, 15, 16])
def test_one_supertree_node_of_that_many_children(dev, arity):
    rng = random.Random(arity)
    n = 4 * arity + 6
    groups = [list(range(4 * i, 4 * i + 4)) for i in range(arity)]
    wide = [pr.rand_tree(g, 2, rng) for g in groups]
    parent, taxon = pr.preorder_arrays([[wide, [n - 6, n - 5]], [[n - 4, n - 3], [n - 2, n - 1]]])
    assert np.bincount(parent[1:]).max() == arity
    trees = _sources(rng, n, 12, 3, n, 4)
    _check(dev, parent, taxon, trees, n, what=arity)
    plan = backend.debug_parsimony_plan(pr.tables(trees, n).tree_off, parent)
    assert plan["counter_bits"] == arity.bit_length()


def test_a_star_supertree_and_a_star_under_a_resolved_root(dev):
    rng = random.Random(300)
    trees = _sources(rng, 300, 10, 3, 300, 5)
    parent, taxon = pr.preorder_arrays(list(range(300)))
    ref = _check(dev, parent, taxon, trees, 300, what="star")
    assert np.array_equal(ref["mrp_length"], ref["mrp_max"])  # the star length, by definition of gmax
    assert backend.debug_parsimony_plan(pr.tables(trees, 300).tree_off, parent)["counter_bits"] == 9
    parent, taxon = pr.preorder_arrays([list(range(150)), pr.rand_tree(range(150, 300), 3, rng)])
    _check(dev, parent, taxon, trees, 300, what="star under a root")


# ------------------------------------------------------------------------------------------------ the stack
@pytest.mark.parametrize("left", [True, False], ids=["left", "right"])
def test_caterpillar_supertrees_keep_the_stack_short(dev, left):
    rng = random.Random(7 + left)
    order = list(range(300))
    rng.shuffle(order)
    parent, taxon = pr.preorder_arrays(pr.caterpillar(order, left))
    trees = _sources(rng, 300, 8, 3, 300)
    plan = backend.debug_parsimony_plan(pr.tables(trees, 300).tree_off, parent)
    assert plan["frame_depth"] <= math.floor(math.log2(300)) + 1 and not plan["frames_in_block"]
    _check(dev, parent, taxon, trees, 300, what=("caterpillar", left))


def test_frames_that_do_not_fit_lds_go_to_the_block(dev):
    # a node of 2^15 children (16 counter slices) beside a balanced subtree that opens nine frames
    rng = random.Random(15)
    wide, deep = 1 << 15, 512

    def balanced(a, b):
        return a if b - a == 1 else [balanced(a, (a + b) // 2), balanced((a + b) // 2, b)]

    parent, taxon = pr.preorder_arrays([list(range(wide)), balanced(wide, wide + deep)])
    n = wide + deep
    trees = [pr.rand_tree(rng.sample(range(wide), 20) + rng.sample(range(wide, n), 40), 3, rng) for _ in range(4)]
    trees.append(pr.rand_tree(range(wide, n), 2, rng))
    plan = backend.debug_parsimony_plan(pr.tables(trees, n).tree_off, parent)
    assert plan["frames_in_block"] and plan["lds_bytes"] == 0 and plan["counter_bits"] == 16
    assert plan["frame_depth"] == 10 and plan["extra_per_tree"] == 4 + 10 * 17 * 512
    _check(dev, parent, taxon, trees, n, batches=(0, 2), what="block")


# ------------------------------------------------------------------------------------------------ coverage
def test_partial_coverage_small_trees_unheld_tips_and_unary_nodes(dev):
    rng = random.Random(60)
    inner = pr.rand_tree(range(60), 4, rng)
    # tips no source holds: 60 .. 64 (ids the tables have) and 70, 71 (ids past the tables' n_taxa); unary nodes
    # above a tip, inside and above the root
    parent, taxon = pr.preorder_arrays([[[[inner, [60], 61], [[62]], 70], 63, [64, 71]]])
    trees = [pr.rand_tree(rng.sample(range(60), 3), 2, rng), [5, 9], [7], [[4, 8], 15], [3, 11, 17]]
    trees += _sources(rng, 60, 6, 3, 60)
    ref = _check(dev, parent, taxon, trees, 65, what="coverage")
    assert ref["mrp_chars"][:5].tolist() == [1, 0, 0, 1, 0] and ref["mrp_length"][1:3].tolist() == [0, 0]


def test_the_supertree_itself_as_a_source_is_perfect(dev):
    rng = random.Random(11)
    tree = pr.rand_tree(range(200), 5, rng)
    parent, taxon = pr.preorder_arrays(tree)
    ref = _check(dev, parent, taxon, [tree, pr.restrict(tree, set(range(0, 200, 3)))], 200, what="S = T")
    assert np.array_equal(ref["mrp_length"], ref["mrp_chars"]) and np.array_equal(ref["mrp_perfect"], ref["mrp_chars"])


# ------------------------------------------------------------------------------------------------ batches, cross-checks
@lru_cache(maxsize=None)
def _mixed_case():
    rng = random.Random(77)
    parent, taxon = pr.preorder_arrays(pr.rand_tree(range(400), 6, rng))
    trees = [pr.rand_tree(rng.sample(range(400), k), 3, rng) for k in (3, 400, 2, 70, 131, 4, 260)]
    return parent, taxon, trees, pr.reference(parent, taxon, trees)


def test_batches_of_mixed_trees_agree(dev):
    parent, taxon, trees, ref = _mixed_case()
    _check(dev, parent, taxon, trees, 400, ref, batches=(1, 2, 0), passes=(0, 1), what="batches")


def test_counts_shared_with_the_rf_export_and_the_bounds(dev):
    parent, taxon, trees, _ = _mixed_case()
    tabs = dev.upload(pr.tables(trees, 400))
    try:
        rf = dev.score(tabs, parent, taxon)
        got = dev.score_parsimony(tabs, parent, taxon, chars=True, n_chars=int(rf["n_source"].sum()))
    finally:
        tabs.free()
    assert np.array_equal(got["mrp_chars"], rf["n_source"]) and np.array_equal(got["mrp_perfect"], rf["shared"])
    assert np.all(got["mrp_chars"] <= got["mrp_length"]) and np.all(got["mrp_length"] <= got["mrp_max"])
    assert np.array_equal(np.add.reduceat(np.append(got["char_len"], 0).astype(np.int64), got["char_off"][:-1])
                          * (got["mrp_chars"] > 0), got["mrp_length"])
    assert got["char_len"].min() >= 1


def test_many_partial_trees_on_a_polytomous_supertree(dev):
    rng = random.Random(40)
    parent, taxon = pr.preorder_arrays(pr.rand_tree(range(300), 9, rng))
    _check(dev, parent, taxon, _sources(rng, 300, 40, 20, 200, 4), 300, batches=(0, 16), what="300 x 40")


def test_the_dcm_sources_on_the_model_tree(dev):
    model = load_trees(str(DATA / "dcm_model_tree.tre"))[0]
    sources = load_trees(str(DATA / "dcm_source_trees.tre"))
    names = model.get_tip_names()
    index = {name: i for i, name in enumerate(names)}
    parent, taxon = pr.preorder_arrays(pr.from_treenode(model, index))
    trees = [pr.from_treenode(t, index) for t in sources]
    ref = _check(dev, parent, taxon, trees, len(names), what="dcm")
    assert ref["mrp_chars"].sum() > 0


# ------------------------------------------------------------------------------------------------ the C interface
def test_any_output_pointer_may_be_null(dev):
    parent, taxon, trees, ref = _mixed_case()
    tabs = dev.upload(pr.tables(trees, 400))
    lib, m, total = dev._lib, len(trees), int(ref["char_off"][-1])
    names = (*pr.PER_TREE, "char_off", *pr.PER_CHAR)
    try:
        for given in ((), ("mrp_length",), ("char_len",), ("char_lo", "char_hi"), ("mrp_perfect", "char_off"),
                      ("mrp_chars", "mrp_max", "char_hi"), names):
            bufs = {k: np.full(m + 1 if k == "char_off" else total if k in pr.PER_CHAR else m, -7,
                               dtype=np.int32 if k in pr.PER_CHAR else np.int64) for k in given}
            rc = lib.scs_score_parsimony(dev._ctx, tabs._h, len(parent), nv.iptr(parent), nv.iptr(taxon), 0, 0,
                                         *(bufs[k].ctypes.data if k in bufs else None for k in names))
            assert rc == 0, (given, lib.scs_last_error())
            for k in given:
                assert np.array_equal(bufs[k], ref[k]), (given, k)
    finally:
        tabs.free()


def test_refusals_are_those_of_the_rf_export(dev):
    tree = [[0, 1], [2, 3]]
    parent, taxon = pr.preorder_arrays(tree)
    tabs = dev.upload(pr.tables([[[0, 1], 2], [[1, 2], 3]], 4))
    twice = dev.upload(pr.tables([[[0, 1], 0]], 4))
    beyond = dev.upload(pr.tables([[[0, 1], 3]], 4))
    edit = lambda a, i, v: np.concatenate([a[:i], [v], a[i + 1:]]).astype(np.int32)  # noqa: E731
    cases = [(tabs, parent[:0], taxon[:0]), (tabs, edit(parent, 0, 0), taxon), (tabs, edit(parent, 2, 5), taxon),
             (tabs, edit(parent, 2, -1), taxon), (tabs, parent, edit(taxon, 2, -1)), (tabs, parent, edit(taxon, 3, 0)),
             (tabs, parent, edit(taxon, 1, 2)), (twice, parent, taxon), (beyond, *pr.preorder_arrays([[0, 1], 2]))]
    try:
        for tb, par, tax in cases:
            said = []
            for method in (dev.score, dev.score_parsimony):
                with pytest.raises(ValueError) as err:
                    method(tb, par, tax)
                said.append(str(err.value))
            assert said[1] == said[0].replace("scs_score_supertree", "scs_score_parsimony"), said
            assert said[1].startswith("scs_score_parsimony: ")
        # and a good call still works afterwards
        _same(dev.score_parsimony(tabs, parent, taxon), pr.reference(parent, taxon, [[[0, 1], 2], [[1, 2], 3]]), "after")
    finally:
        for tb in (tabs, twice, beyond):
            tb.free()
    null = dev._lib.scs_score_parsimony(dev._ctx, None, 1, None, None, 0, 0, *([None] * 8))
    assert null == nv.EINVAL and dev._lib.scs_last_error() == b"scs_score_parsimony: null argument"


# ------------------------------------------------------------------------------------------------ API and CLI
NEWICK_SUPER = "((a,b),((c,d),(e,(f,g))));"
NEWICK_SOURCES = ["((a,b),(c,(d,e)));", "((a,c),(b,d),e);", "(e,(f,g));", "((a,g),(b,f),(c,e),d);", "(a,b);"]


def _api_reference():
    sup = make_tree(NEWICK_SUPER)
    names = sup.get_tip_names()
    index = {name: i for i, name in enumerate(names)}
    parent, taxon = pr.preorder_arrays(pr.from_treenode(sup, index))
    trees = [pr.from_treenode(make_tree(t), index) for t in NEWICK_SOURCES]
    return names, trees, pr.reference(parent, taxon, trees)


def test_score_supertree_with_parsimony(dev):
    names, trees, ref = _api_reference()
    sources = [make_tree(t) for t in NEWICK_SOURCES]
    res = score_supertree(make_tree(NEWICK_SUPER), sources, parsimony=True, parsimony_chars=True, device=dev)
    for k in pr.PER_TREE:
        assert np.array_equal(getattr(res, k), ref[k]), k
    assert np.array_equal(res.mrp_chars, res.n_source) and np.array_equal(res.mrp_perfect, res.shared)
    assert np.array_equal(res.mrp_extra, ref["mrp_length"] - ref["mrp_chars"]) and "parsimony" in res.timings
    assert res.total_mrp_length == int(ref["mrp_length"].sum())
    assert res.consistency_index == pytest.approx(ref["mrp_chars"].sum() / ref["mrp_length"].sum())
    gap = ref["mrp_max"].sum() - ref["mrp_chars"].sum()
    assert res.retention_index == pytest.approx((ref["mrp_max"].sum() - ref["mrp_length"].sum()) / gap)
    off = ref["char_off"]
    for i in range(len(sources)):
        assert np.array_equal(res.mrp_char_length(i), ref["char_len"][off[i]:off[i + 1]])
        want = [sorted(names[x] for x in pr.leaves_of(trees[i])[lo:hi + 1])
                for lo, hi in zip(ref["char_lo"][off[i]:off[i + 1]], ref["char_hi"][off[i]:off[i + 1]])]
        assert [sorted(c) for c in res.mrp_char_clusters(i)] == want
    worst = res.worst_source_clades()
    assert len(worst) == off[-1] and [r["length"] for r in worst] == sorted(ref["char_len"].tolist(), reverse=True)
    assert worst[0]["length"] == ref["char_len"].max() and res.worst_source_clades(2) == worst[:2]
    assert all(r["size"] == len(r["tips"]) and 1 <= r["length"] <= r["gmax"] for r in worst)
    noted = res.annotate_source(3)
    named = sorted(int(v.name) for v in noted.iter_nontips() if v.name is not None)
    assert named == sorted(ref["char_len"][off[3]:off[4]].tolist())
    assert sorted(noted.get_tip_names()) == sorted(sources[3].get_tip_names())
    rows = res.parsimony_table().splitlines()
    assert rows[0].split("\t")[:5] == ["index", "n_leaves", "mrp_chars", "mrp_length", "mrp_perfect"]
    assert len(rows) == len(sources) + 1
    plain = score_supertree(make_tree(NEWICK_SUPER), sources, device=dev)
    assert plain.mrp_length is None and "parsimony" not in plain.timings
    with pytest.raises(ValueError, match="parsimony=True"):
        plain.total_mrp_length
    brief = score_supertree(make_tree(NEWICK_SUPER), sources, parsimony=True, device=dev)
    assert np.array_equal(brief.mrp_length, ref["mrp_length"])
    with pytest.raises(ValueError, match="parsimony_chars=True"):
        brief.worst_source_clades()


def test_the_command_line_writes_the_scores_and_the_clades(tmp_path):
    src = DATA / "supertriplets_source.tre"
    out, plain, full, clades = (tmp_path / x for x in ("out.tre", "plain.tsv", "full.tsv", "clades.tsv"))
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(full), "--parsimony",
                                   "--source-clades-out", str(clades)])
    assert res.exit_code == 0, res.output
    # (every run is held to the tree it wrote: the order of a node's children may differ from run to run)
    api = score_supertree(load_tree(out), load_trees(src), parsimony=True, parsimony_chars=True)
    rows = [line.split("\t") for line in full.read_text().splitlines()]
    assert rows[0] == ["index", "n_leaves", "n_super", "n_source", "shared", "rf", *pr.PER_TREE]
    got = np.array([[int(x) for x in r[6:]] for r in rows[1:]], dtype=np.int64)
    assert np.array_equal(got, np.stack([getattr(api, k) for k in pr.PER_TREE], axis=1)) and api.mrp_extra.any()
    # the command line reads the sources into flat arrays, the call above as tree objects: the same clades and names
    assert clades.read_text() == api.source_clade_table()
    assert clades.read_text().splitlines()[0].split("\t") == ["tree", "tips", "size", "length", "gmax"]
    assert len(clades.read_text().splitlines()) == int(api.mrp_chars.sum()) + 1
    # without --parsimony: the six columns of before, also when only the clade table is asked for
    for extra in ([], ["--source-clades-out", str(tmp_path / "c2.tsv")]):
        res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--scores-out", str(plain), *extra])
        assert res.exit_code == 0, res.output
        api = score_supertree(load_tree(out), load_trees(src))
        assert plain.read_text() == api.table()
        assert plain.read_text().splitlines()[0].split("\t") == ["index", "n_leaves", "n_super", "n_source", "shared",
                                                                  "rf"]
    res = CliRunner().invoke(scs, ["-i", str(src), "-o", str(out), "--parsimony"])
    assert res.exit_code != 0 and "--parsimony needs --scores-out" in res.output
