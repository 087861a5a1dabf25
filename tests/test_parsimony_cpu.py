"""The MRP parsimony scores without a device: the references of ``tests/parsimony_reference.py`` held to one another
and to the definitions (Sankoff's DP against every labelling, against a literal Hartigan pass, length 1 exactly for
the displayed clusters, the star length), the plan entry against its restatement, the bindings against the header,
and the host layer -- what ``Device.score_parsimony`` hands to the export, what ``score_supertree`` makes of its
answers, the derived indices on hand-made counts."""

import ctypes as C
import math
import random
import re
import types
from pathlib import Path

import numpy as np
import parsimony_reference as pr
import pytest

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import backend, score_supertree
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import SupertreeScore
from spectralclustersupertree_amd.tree import make_tree

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the references
def test_sankoff_equals_every_labelling_on_tiny_supertrees():
    rng = random.Random(8)
    seen = 0
    for _ in range(300):
        tips = rng.randint(3, 5)
        sup = pr.rand_tree(range(tips), 3, rng)
        parent, taxon = pr.preorder_arrays(sup)
        if len(parent) > 8:
            continue
        tree = pr.rand_tree(rng.sample(range(tips), rng.randint(3, tips)), 3, rng)
        got, want = pr.sankoff(parent, taxon, tree), pr.exhaustive(parent, taxon, tree)
        assert np.array_equal(got, want), (sup, tree, got, want)
        seen += len(got)
    assert seen > 200
    # the case of the issue: rooted coding, {a, b} takes two changes on (a,(b,(c,d)))
    parent, taxon = pr.preorder_arrays([0, [1, [2, 3]]])
    assert pr.exhaustive(parent, taxon, [[0, 1], 2, 3]).tolist() == [2] == pr.sankoff(parent, taxon, [[0, 1], 2, 3]).tolist()


def _random_case(rng, trial: int):
    n = rng.randint(3, 40)
    sup = pr.rand_tree(range(n), rng.choice([2, 3, 5, 9]), rng)
    if trial % 7 == 0:
        order = list(range(n))
        rng.shuffle(order)
        sup = pr.caterpillar(order, left=bool(trial % 14))
    held = rng.sample(range(n), rng.randint(3, n))
    return sup, pr.rand_tree(held, rng.choice([2, 3, 6]), rng)


def test_sankoff_equals_hartigan_and_length_one_means_displayed():
    rng = random.Random(5)
    chars = perfect = 0
    for trial in range(300):
        sup, tree = _random_case(rng, trial)
        parent, taxon = pr.preorder_arrays(sup)
        got = pr.sankoff(parent, taxon, tree)
        assert np.array_equal(got, pr.hartigan(sup, tree)), (sup, tree)
        leaves = pr.leaves_of(tree)
        lo, hi = pr.characters(tree)
        m = len(leaves)
        assert len(lo) == len({frozenset(c) for c in pr.clusters(tree) if 2 <= len(c) < m})
        restricted = pr.restrict(sup, set(leaves))
        shown = pr.clusters(restricted) if isinstance(restricted, list) else set()
        for a, b, length in zip(lo, hi, got):
            size = b - a + 1
            assert 1 <= length <= min(size, m - size + 1)
            assert (length == 1) == (frozenset(leaves[a:b + 1]) in shown)
        chars += len(got)
        perfect += int((got == 1).sum())
    assert chars > 2000 and 0 < perfect < chars


def test_the_length_on_a_star_is_gmax():
    rng = random.Random(3)
    parent, taxon = pr.preorder_arrays(list(range(30)))
    for _ in range(20):
        tree = pr.rand_tree(rng.sample(range(30), rng.randint(3, 30)), 4, rng)
        lo, hi = pr.characters(tree)
        size, m = hi - lo + 1, len(pr.leaves_of(tree))
        assert np.array_equal(pr.sankoff(parent, taxon, tree), np.minimum(size, m - size + 1))
    ref = pr.reference(parent, taxon, [[[0, 1], 2, [3, 4, 5]], [0, 1], [7]])
    assert ref["mrp_chars"].tolist() == [2, 0, 0] and ref["mrp_max"].tolist() == [5, 0, 0]
    assert ref["mrp_length"].tolist() == [5, 0, 0] and ref["char_off"].tolist() == [0, 2, 2, 2]
    assert ref["char_lo"].tolist() == [0, 3] and ref["char_hi"].tolist() == [1, 5]


def test_characters_come_in_the_order_of_their_first_gaps():
    # ((a,b),c,(d,(e,f)),g): first gaps after a ({a,b}), after d ({d,e,f}), after e ({e,f}); the root is no character
    lo, hi = pr.characters([[0, 1], 2, [3, [4, 5]], 6])
    assert lo.tolist() == [0, 3, 4] and hi.tolist() == [1, 5, 5]
    # a unary node repeats no cluster, and a cluster over every leaf is trivial
    lo, hi = pr.characters([[[[0, 1]], 2]])
    assert lo.tolist() == [0] and hi.tolist() == [1]


# ------------------------------------------------------------------------------------------------ the plan
def _balanced(a, b):
    return a if b - a == 1 else [_balanced(a, (a + b) // 2), _balanced((a + b) // 2, b)]


PLAN_SUPERTREES = {
    "binary": lambda rng: pr.rand_tree(range(500), 2, rng),
    "polytomous": lambda rng: pr.rand_tree(range(500), 17, rng),
    "left caterpillar": lambda rng: pr.caterpillar(range(300), True),
    "right caterpillar": lambda rng: pr.caterpillar(range(300), False),
    "star": lambda rng: list(range(300)),
    "unary chain": lambda rng: [[[pr.rand_tree(range(40), 3, rng)]]],
    "wide and deep": lambda rng: [list(range(1 << 15)), _balanced(1 << 15, (1 << 15) + 512)],
    "one tip": lambda rng: 0,
}


@pytest.mark.parametrize("shape", list(PLAN_SUPERTREES))
def test_the_plan_entry_equals_its_restatement(shape):
    rng = random.Random(len(shape))
    parent, _ = pr.preorder_arrays(PLAN_SUPERTREES[shape](rng))
    sizes = [rng.choice([1, 2, 3, 4, 66, 67, 130, 4099, 9000]) for _ in range(23)]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    chars = np.array([rng.randint(0, max(n - 2, 0)) for n in sizes], dtype=np.int64)
    for given in (None, chars):
        for batch_trees, pass_words in ((0, 0), (1, 1), (2, 63), (5, 64), (0, 200), (3, 2)):
            got = backend.debug_parsimony_plan(off, parent, given, batch_trees, pass_words)
            want = pr.plan(off, parent, given, batch_trees, pass_words)
            assert sorted(got) == sorted(want)
            for k in want:
                assert np.array_equal(got[k], want[k]), (shape, given is None, batch_trees, pass_words, k, got[k], want[k])
    tips = int(got["super_tips"])
    assert got["frame_depth"] <= max(int(math.floor(math.log2(max(tips, 1)))), 0) + 1
    assert got["frames_in_block"] == (shape == "wide and deep")
    if shape == "star":
        assert got["frame_depth"] == 1 and got["counter_bits"] == 9 and got["lds_bytes"] == 10 * 512
    if shape.endswith("caterpillar"):
        assert got["frame_depth"] == 1 and got["counter_bits"] == 2
    # (the last setting: 2 words a pass, the characters given)
    assert np.array_equal(got["passes"], -(-got["words"] // 2)) and got["words"].max() == (chars.max() + 63) // 64


def test_the_plan_entry_refuses_what_is_no_supertree():
    off = np.array([0, 5], dtype=np.int64)
    for parent in ([0, 0], [-1, 1], [-1, 0, 3], []):
        with pytest.raises(nv.ScsError, match="scs_debug_parsimony_plan"):
            backend.debug_parsimony_plan(off, np.array(parent, dtype=np.int32))
    with pytest.raises(ValueError, match="one entry per source tree"):
        backend.debug_parsimony_plan(off, np.array([-1, 0, 0], dtype=np.int32), chars=[1, 2])


# ------------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("symbol,count", [("scs_score_parsimony", 15), ("scs_debug_parsimony_plan", 12)])
def test_the_exports_are_declared_bound_and_exported(symbol, count):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "scs_hip.h").read_text(), flags=re.S)
    m = re.search(rf"int {symbol}\(([^)]*)\)", text)
    assert m, f"include/scs_hip.h does not declare {symbol}"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    restype, argtypes = nv.SIGNATURES[symbol]
    assert restype is C.c_int and len(argtypes) == len(params) == count
    for p, a in zip(params, argtypes):
        assert (a is nv._I32) == (p.startswith("int32_t ") and "*" not in p), (symbol, p)
    lib = nv.load_library()
    assert hasattr(lib, symbol) and lib.scs_version() == nv.ABI_VERSION
    if symbol == "scs_score_parsimony":
        assert params[:7] == ["scs_ctx *ctx", "const scs_tables *sources", "int32_t n_nodes", "const int32_t *parent",
                              "const int32_t *taxon", "int32_t max_batch_trees", "int32_t max_pass_words"]
        assert [p.split("*")[1] for p in params[7:]] == [*pr.PER_TREE, "char_off", *pr.PER_CHAR]
        # a null context is refused like scs_score_supertree refuses it, before any device call
        assert lib.scs_score_parsimony(None, None, 1, None, None, 0, 0, *([None] * 8)) == nv.EINVAL
        assert lib.scs_last_error() == b"scs_score_parsimony: null argument"
    header = (ROOT / "include" / "scs_hip.h").read_text()
    assert "sum of\n * mrp_chars entries" in header and "min(|C|, m - |C| + 1)" in header


# ------------------------------------------------------------------------------------------------ the host layer
PARENT = [-1, 0, 1, 1, 0, 4, 4]
TAXON = [-1, -1, 0, 1, -1, 2, 3]


def _at(address: int, dtype, count: int) -> np.ndarray:
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


class FakeLib:
    """``scs_score_parsimony`` records its arguments and answers three trees of 2, 0 and 1 characters."""

    def __init__(self):
        self.calls = []

    def scs_last_error(self):
        return b""

    def scs_score_parsimony(self, ctx, tabs, n, parent, taxon, batch, words, *outs):
        self.calls.append((batch, words, [o is not None for o in outs]))
        for o, row in zip(outs[:4], ([2, 0, 1], [5, 0, 1], [0, 0, 1], [6, 0, 2])):
            _at(o, np.int64, 3)[:] = row
        if outs[4] is not None:
            _at(outs[4], np.int64, 4)[:] = [0, 2, 2, 3]
        for o, row in zip(outs[5:], ([3, 2, 1], [0, 2, 1], [1, 3, 2])):
            if o is not None:
                _at(o, np.int32, 3)[:] = row
        return 0


def test_device_method_marshals_the_export_and_sizes_the_characters():
    lib = FakeLib()
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3)
    got = dev.score_parsimony(tabs, PARENT, TAXON, batch_trees=4, pass_words=2)
    assert lib.calls == [(4, 2, [True] * 4 + [False] * 4)]
    assert list(got) == [*pr.PER_TREE, "char_off", *pr.PER_CHAR] and got["char_off"] is None and got["char_len"] is None
    assert got["mrp_length"].tolist() == [5, 0, 1] and got["mrp_length"].dtype == np.int64
    lib.calls.clear()
    got = dev.score_parsimony(tabs, PARENT, TAXON, chars=True)  # a first call sizes the buffers
    assert lib.calls == [(0, 0, [True] * 5 + [False] * 3), (0, 0, [True] * 8)]
    assert got["char_len"].tolist() == [3, 2, 1] and got["char_len"].dtype == np.int32 and got["char_hi"].tolist() == [1, 3, 2]
    lib.calls.clear()
    got = dev.score_parsimony(tabs, PARENT, TAXON, chars=True, n_chars=3)  # or the caller does
    assert lib.calls == [(0, 0, [True] * 8)] and got["char_off"].tolist() == [0, 2, 2, 3]
    with pytest.raises(ValueError, match="one entry per supertree node"):
        dev.score_parsimony(tabs, PARENT, TAXON[:-1])


class FakeTables:
    def __init__(self, n_trees):
        self.n_trees, self.freed = n_trees, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload``, ``score`` and ``score_parsimony`` for the sources below, logged."""

    def __init__(self):
        self.log, self.tabs = [], None

    def upload(self, tables):
        self.tabs = FakeTables(tables.n_trees)
        return self.tabs

    def score(self, tabs, parent, taxon, batch_trees=0):
        self.log.append(("score", batch_trees))
        m = tabs.n_trees
        return {"n_super": np.ones(m, dtype=np.int64), "n_source": np.array([2, 0, 1], dtype=np.int64),
                "shared": np.array([0, 0, 1], dtype=np.int64), "informative": np.zeros(len(parent), dtype=np.int64),
                "supported": np.zeros(len(parent), dtype=np.int64)}

    def score_parsimony(self, tabs, parent, taxon, chars=False, batch_trees=0, pass_words=0, n_chars=None):
        self.log.append(("score_parsimony", chars, batch_trees, pass_words, n_chars))
        out = {"mrp_chars": [2, 0, 1], "mrp_length": [5, 0, 1], "mrp_perfect": [0, 0, 1], "mrp_max": [6, 0, 2]}
        out = {k: np.array(v, dtype=np.int64) for k, v in out.items()}
        if chars:
            out.update(char_off=np.array([0, 2, 2, 3], dtype=np.int64), char_len=np.array([3, 2, 1], dtype=np.int32),
                       char_lo=np.array([0, 2, 1], dtype=np.int32), char_hi=np.array([1, 3, 2], dtype=np.int32))
        return out


SOURCES = ["((a,b),(c,d),e);", "(a,c);", "(b,(c,d));"]


def test_score_supertree_runs_the_parsimony_pass_last_and_serves_the_clades(monkeypatch):
    monkeypatch.setattr(score_mod, "BATCH_TREES", 11)
    monkeypatch.setattr(score_mod, "PARSIMONY_PASS_WORDS", 3)
    sup, trees = make_tree("((a,b),((c,d),e));"), [make_tree(t) for t in SOURCES]
    dev = FakeDevice()
    res = score_supertree(sup, trees, parsimony_chars=True, device=dev)  # (implies parsimony=True)
    assert dev.log == [("score", 11), ("score_parsimony", True, 11, 3, 3)] and dev.tabs.freed == 1
    assert set(res.timings) == {"prepare", "tables", "score", "parsimony"}
    assert res.mrp_length.tolist() == [5, 0, 1] and res.mrp_extra.tolist() == [3, 0, 0] and res.total_mrp_length == 6
    assert res.mrp_char_length(0).tolist() == [3, 2] and res.mrp_char_length(1).tolist() == []
    assert res.mrp_char_clusters(0) == [["a", "b"], ["c", "d"]] and res.mrp_char_clusters(2) == [["c", "d"]]
    assert res.worst_source_clades() == [
        {"tree": 0, "tips": ["a", "b"], "size": 2, "length": 3, "gmax": 2},
        {"tree": 0, "tips": ["c", "d"], "size": 2, "length": 2, "gmax": 2},
        {"tree": 2, "tips": ["c", "d"], "size": 2, "length": 1, "gmax": 2}]
    assert res.worst_source_clades(1) == res.worst_source_clades()[:1]
    assert res.source_clade_table().splitlines() == ["tree\ttips\tsize\tlength\tgmax", "0\ta,b\t2\t3\t2",
                                                     "0\tc,d\t2\t2\t2", "2\tc,d\t2\t1\t2"]
    assert res.annotate_source(0).get_newick(with_node_names=True).rstrip(";") == "((a,b)3,(c,d)2,e)"
    assert trees[0].get_newick(with_node_names=True).rstrip(";") == "((a,b),(c,d),e)"  # (a copy was named)
    assert res.table().splitlines()[0].split("\t")[-4:] == list(pr.PER_TREE)
    assert res.table().splitlines()[1].split("\t")[-4:] == ["2", "5", "0", "6"]
    assert res.parsimony_table().splitlines()[1] == "0\t5\t2\t5\t0\t6\t3\t0.4000\t0.2500"
    # without the keyword: the passes, fields and table of before
    dev = FakeDevice()
    plain = score_supertree(sup, trees, device=dev)
    assert dev.log == [("score", 11)] and plain.mrp_length is None and plain.mrp_chars is None
    assert plain.table().splitlines()[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf"
    for call in (lambda: plain.total_mrp_length, lambda: plain.consistency_index, plain.parsimony_table):
        with pytest.raises(ValueError, match="parsimony=True"):
            call()
    dev = FakeDevice()
    brief = score_supertree(sup, trees, parsimony=True, device=dev)
    assert dev.log[1] == ("score_parsimony", False, 11, 3, None) and brief.total_mrp_length == 6
    for call in (brief.worst_source_clades, lambda: brief.mrp_char_length(0), lambda: brief.annotate_source(0)):
        with pytest.raises(ValueError, match="parsimony_chars=True"):
            call()


def test_the_characters_go_back_to_the_trees_as_given():
    # tables that hold the given trees 3, 0 and 4 (in that order) of five
    req = score_mod._Request(False, False, False, False, False, None, None, 64, ["a", "b", "c", "d"], parsimony=True,
                             parsimony_chars=True)
    src = types.SimpleNamespace(dev=FakeDevice(), tabs=FakeTables(3), n_leaves=np.array([5, 1, 1, 5, 3]),
                                tree_index=lambda: np.array([3, 0, 4], dtype=np.int64))
    res = score_mod._run_passes(src, np.array(PARENT, dtype=np.int32), np.array(TAXON, dtype=np.int32), req, {})
    assert res["mrp_length"].tolist() == [0, 0, 0, 5, 1] and res["mrp_chars"].tolist() == [0, 0, 0, 2, 1]
    assert [r["len"].tolist() for r in res["mrp_char_rows"]] == [[], [], [], [3, 2], [1]]
    assert [r["hi"].tolist() for r in res["mrp_char_rows"]] == [[], [], [], [1, 3], [2]]


def test_the_pass_without_tables_gives_zeros():
    req = score_mod._Request(False, False, False, False, False, None, None, 64, ["a", "b", "c", "d"], parsimony=True,
                             parsimony_chars=True)
    src = types.SimpleNamespace(dev=None, tabs=None, n_leaves=np.array([1, 1]), tree_index=lambda: None)
    timings: dict = {}
    res = score_mod._run_passes(src, np.array(PARENT, dtype=np.int32), np.array(TAXON, dtype=np.int32), req, timings)
    assert set(timings) == {"score", "parsimony"}
    for k in pr.PER_TREE:
        assert res[k].dtype == np.int64 and res[k].tolist() == [0, 0]
    out = score_mod._result(make_tree("((a,b),(c,d));"), src.n_leaves, res, timings, [make_tree("a;"), make_tree("b;")])
    assert out.total_mrp_length == 0 and math.isnan(out.consistency_index) and math.isnan(out.retention_index)
    assert out.worst_source_clades() == [] and out.mrp_char_length(1).tolist() == []
    assert out.parsimony_table().splitlines()[1] == "0\t1\t0\t0\t0\t0\t0\tnan\tnan"


def test_the_derived_indices_on_hand_made_counts():
    res = SupertreeScore(None, np.array([6, 5, 2, 4]), None, None, None, None, None)
    res._mrp = {"mrp_chars": np.array([4, 3, 0, 2]), "mrp_length": np.array([6, 3, 0, 4]),
                "mrp_perfect": np.array([2, 3, 0, 0]), "mrp_max": np.array([8, 5, 0, 4]), "chars": None, "source": None}
    assert res.mrp_extra.tolist() == [2, 0, 0, 2] and res.total_mrp_length == 13
    assert res.consistency_index == pytest.approx(9 / 13) and res.retention_index == pytest.approx((17 - 13) / (17 - 9))
    ci, ri = res.tree_consistency_index, res.tree_retention_index
    assert ci[:2].tolist() == pytest.approx([4 / 6, 1.0]) and math.isnan(ci[2]) and ci[3] == 0.5
    assert ri[:2].tolist() == pytest.approx([0.5, 1.0]) and math.isnan(ri[2]) and ri[3] == 0.0
    assert score_mod.retention(3, 3, 3) != score_mod.retention(3, 3, 3)  # NaN: no character can take a second change
    assert score_mod.consistency(0, 0) != score_mod.consistency(0, 0)
