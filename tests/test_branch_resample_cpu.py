"""Resampled and weighted branch triplet support without a device: the host reference against the section 18
reference, the wins rule, the replicate draws, the weight checks, how ``score_supertree`` runs the pass on a fake
device and what ``nni_candidates(min_support=...)`` keeps."""

import ctypes as C
import re
import types
from pathlib import Path

import numpy as np
import pytest
import branch_triplet_reference as br
import resample_reference as rr

from spectralclustersupertree_amd import _native
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd import score_supertree
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.score import SupertreeScore, resample_weights
from spectralclustersupertree_amd.tree import make_tree

EXPORT = "scs_score_branch_resample"


@pytest.fixture(scope="module")
def cases():
    return rr.resample_cases()


@pytest.fixture(scope="module")
def counts(cases):
    return [rr.per_tree(sup, trees) for sup, trees in cases]


# ------------------------------------------------------------------ the reference itself
def test_the_cases_have_branches_with_every_outcome(cases, counts):
    assert len(cases) == 40
    total = np.zeros(4, dtype=object)
    for (sup, trees), c in zip(cases, counts):
        assert 8 <= len(sup.get_tip_names()) <= 30 and 3 <= len(trees) <= 8
        total += c.sum(axis=(0, 2))
    # (a reference of zeros must not pass: concordant, both alternatives and fans all occur)
    assert min(total[1:]) > 0 and total[0] > total[1:].sum(), total


def test_ones_give_the_branch_triplet_counts_of_the_list(cases, counts):
    for (sup, trees), c in zip(cases, counts):
        ref = br.node_sum(sup, trees)
        got = rr.rows(np.ones((1, len(trees)), dtype=np.int64), c)
        for x, key in enumerate(br.PER_NODE):
            assert [int(v) for v in ref[key]] == list(got[x][0]), key


def test_an_integer_weight_is_that_many_copies_of_the_tree(cases, counts):
    rs = np.random.RandomState(3)
    for (sup, trees), c in zip(cases, counts):
        w = rs.randint(0, 4, size=len(trees))
        w[int(rs.randint(len(trees)))] = 0
        ref = br.node_sum(sup, rr.repeated(trees, w))
        got = rr.rows(w[None, :], c)
        for x, key in enumerate(br.PER_NODE):
            assert [int(v) for v in ref[key]] == list(got[x][0]), key


def test_the_wins_rule():
    # one column per situation, rows 1 .. 3 decided (row 0, the point estimate, never is)
    #            con wins  alt1 wins  alt2 wins  con=alt1 top  con=alt2 top  alt1=alt2 top  all fans  no branch
    con = [[9] * 8, [5, 1, 1, 4, 4, 1, 0, 0], [5, 1, 1, 4, 4, 1, 0, 0], [0] * 8]
    alt1 = [[9] * 8, [1, 5, 1, 4, 1, 4, 0, 0], [1, 5, 1, 4, 1, 4, 0, 0], [0] * 8]
    alt2 = [[9] * 8, [1, 1, 5, 1, 4, 4, 0, 0], [1, 1, 5, 1, 4, 4, 0, 0], [0] * 8]
    total = [[30] * 8, [9, 9, 9, 9, 9, 9, 7, 0], [9, 9, 9, 9, 9, 9, 7, 0], [0] * 8]  # (row 3: uninformative)
    got = rr.wins(np.array([total, con, alt1, alt2], dtype=object))
    assert got.tolist() == [[2, 0, 0, 0, 0, 0, 0, 0],
                            [0, 2, 0, 0, 0, 0, 0, 0],
                            [0, 0, 2, 0, 0, 0, 0, 0],
                            [0, 0, 0, 2, 2, 2, 2, 0]]


# ------------------------------------------------------------------ the draws and the weight checks
@pytest.mark.parametrize("kind", ["bootstrap", "jackknife"])
def test_the_draws_follow_the_seed_and_the_stated_recipe(kind):
    tw = [2, 0, 1, 3, 1, 1, 5]
    a = resample_weights(7, 25, tw, kind, 11)
    assert a.dtype == np.int64 and a.shape == (26, 7) and a[0].tolist() == tw
    assert np.array_equal(a, resample_weights(7, 25, tw, kind, 11))
    assert not np.array_equal(a, resample_weights(7, 25, tw, kind, 12))
    assert np.array_equal(a, rr.draws(7, 25, tw, kind, 11))
    assert np.array_equal(resample_weights(7, 25, None, kind, 11), rr.draws(7, 25, None, kind, 11))
    if kind == "jackknife":
        assert all(set(a[1:, t].tolist()) <= {0, tw[t]} for t in range(7))
        assert 0 < int((a[1:, 0] > 0).sum()) < 25
    else:
        flat = resample_weights(7, 25, [3] * 7, kind, 11)
        assert (flat[1:].sum(axis=1) == 7 * 3).all() and len({tuple(r) for r in flat[1:].tolist()}) > 1


def test_a_matrix_and_tree_weights_are_taken_as_given():
    assert resample_weights(3) is None
    assert resample_weights(3, None, [1.0, 0, 2]).tolist() == [[1, 0, 2]]
    got = resample_weights(3, [[0, 1, 2], [3.0, 0, 0]], [5, 5, 5])
    assert got.tolist() == [[5, 5, 5], [0, 1, 2], [3, 0, 0]] and got.dtype == np.int64
    assert resample_weights(3, 0).tolist() == [[1, 1, 1]]
    assert resample_weights(3, np.zeros((0, 3))).tolist() == [[1, 1, 1]]


@pytest.mark.parametrize(("kwargs", "message"), [
    ({"tree_weights": [1, 1.5, 1]}, "tree_weights must be non-negative integers: scoring is exact"),
    ({"tree_weights": [1, -1, 1]}, "tree_weights must be non-negative integers: scoring is exact"),
    ({"tree_weights": [1, float("nan"), 1]}, "tree_weights must be non-negative integers"),
    ({"tree_weights": ["a", "b", "c"]}, "tree_weights must be non-negative integers"),
    ({"tree_weights": [1, 1]}, r"one entry per source tree \(3\)"),
    ({"branch_resample": [[1, 1]]}, r"replicates x source trees \(3\)"),
    ({"branch_resample": [1, 1, 1]}, r"replicates x source trees \(3\)"),
    ({"branch_resample": [[1, 0.5, 1]]}, "branch_resample must be non-negative integers: scoring is exact"),
    ({"branch_resample": [[1, -2, 1]]}, "branch_resample must be non-negative integers"),
    ({"branch_resample": -1}, "branch_resample must be non-negative integers"),
    ({"branch_resample": 2.5}, "branch_resample must be non-negative integers"),
    ({"branch_resample": 2, "resample": "subsample"}, "resample must be 'bootstrap' or 'jackknife'"),
])
def test_weights_that_are_not_integers_of_the_right_shape_are_refused(kwargs, message):
    sup, trees = _sequence_case()
    dev = FakeDevice()
    with pytest.raises(ValueError, match=message):
        score_supertree(sup, trees, device=dev, **kwargs)
    assert dev.log == []  # (refused before the tables are made)


# ------------------------------------------------------------------ the pass on a fake device
class FakeTables:
    def __init__(self, n_trees):
        self.n_trees, self.freed = n_trees, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload`` and the three methods these tests reach: logged, answered with ramps of the right shapes."""

    def __init__(self):
        self.log, self.tabs, self.weights = [], None, None

    def upload(self, tables):
        self.tabs = FakeTables(tables.n_trees)
        return self.tabs

    def score(self, tabs, parent, taxon, batch_trees=0):
        self.log.append("score")
        zeros = {k: np.zeros(tabs.n_trees, dtype=np.int64) for k in ("n_super", "n_source", "shared")}
        return {**zeros, "informative": np.zeros(len(parent), dtype=np.int64),
                "supported": np.zeros(len(parent), dtype=np.int64)}

    def score_branch_triplets(self, tabs, parent, taxon, batch_trees=0):
        self.log.append("score_branch_triplets")
        out = {k: np.zeros(tabs.n_trees, dtype=np.int64) for k in br.PER_TREE}
        out.update({k: np.zeros(len(parent), dtype=np.int64) for k in br.PER_NODE})
        return out

    def score_branch_resample(self, tabs, parent, taxon, weights, rows=False, batch_trees=0):
        self.log.append(("score_branch_resample", rows, batch_trees))
        self.weights = np.array(weights)
        n, r = len(parent), len(weights)
        return {"rs_point": 100 + np.arange(4 * n, dtype=np.int64).reshape(4, n),
                "rs_wins": np.arange(4 * n, dtype=np.int32).reshape(4, n),
                "rs_rows": 1000 + np.arange(4 * r * n, dtype=np.int64).reshape(4, r, n) if rows else None}


class FakeLib:
    """``scs_score_branch_resample`` records its arguments and what the weight buffer held, and fills the outputs."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def scs_last_error(self):
        return b"the export said no"

    def scs_score_branch_resample(self, ctx, tabs, n, parent, taxon, batch, n_rep, weights, point, wins, rows):
        at = lambda addr, dtype, count: np.frombuffer(  # noqa: E731
            (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(addr), dtype=dtype, count=count)
        self.calls.append({"n": n, "batch": batch, "n_rep": n_rep, "rows": rows,
                           "weights": at(weights, np.int32, n_rep * 3).reshape(n_rep, 3).copy()})
        at(point, np.int64, 4 * n)[:] = np.arange(4 * n)
        at(wins, np.int32, 4 * n)[:] = 7
        if rows is not None:
            at(rows, np.int64, 4 * n_rep * n)[:] = 9
        return self.rc


@pytest.mark.parametrize("rows", [False, True])
def test_the_device_method_marshals_the_export(rows):
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = FakeLib(), C.c_void_p()
    tabs = types.SimpleNamespace(_h=object(), n_trees=3)
    parent, taxon = [-1, 0, 1, 1, 0, 4, 4], [-1, -1, 0, 1, -1, 2, 3]
    got = dev.score_branch_resample(tabs, parent, taxon, [[1, 2, 3], [0.0, 4, 0]], rows=rows, batch_trees=5)
    (seen,) = dev._lib.calls
    assert (seen["n"], seen["batch"], seen["n_rep"]) == (7, 5, 2) and (seen["rows"] is not None) == rows
    assert seen["weights"].tolist() == [[1, 2, 3], [0, 4, 0]]
    assert list(got) == ["rs_point", "rs_wins", "rs_rows"]
    assert got["rs_point"].dtype == np.int64 and got["rs_point"].tolist() == np.arange(28).reshape(4, 7).tolist()
    assert got["rs_wins"].dtype == np.int32 and got["rs_wins"].shape == (4, 7) and (got["rs_wins"] == 7).all()
    assert got["rs_rows"] is None if not rows else (got["rs_rows"].shape == (4, 2, 7) and (got["rs_rows"] == 9).all())
    with pytest.raises(ValueError, match="weights one row per replicate with one entry per source tree"):
        dev.score_branch_resample(tabs, parent, taxon, [[1, 2]])
    with pytest.raises(ValueError, match="does not fit int32"):
        dev.score_branch_resample(tabs, parent, taxon, [[1, 2, 2**31]])
    assert len(dev._lib.calls) == 1
    dev._lib.rc = _native.EINVAL
    with pytest.raises(ValueError, match="^the export said no$"):
        dev.score_branch_resample(tabs, parent, taxon, [[1, 2, 3]])


def _sequence_case():
    return make_tree("((a,b),(c,d));"), [make_tree("((a,b),c);"), make_tree("(a,(c,d));"), make_tree("(b,c,d);")]


def test_nothing_asked_for_runs_no_resample_pass():
    sup, trees = _sequence_case()
    dev = FakeDevice()
    res = score_supertree(sup, trees, branch_triplets=True, device=dev)
    assert dev.log == ["score", "score_branch_triplets"] and "branch_resample" not in res.timings
    for name in ("rs_weights", "rs_total", "rs_concordant", "rs_alt1", "rs_alt2", "rs_total_rows", "rs_alt2_rows",
                 "rs_wins", "branch_support"):
        assert getattr(res, name) is None, name
    with pytest.raises(ValueError, match="no replicates were scored"):
        res.annotate_branch_support()
    with pytest.raises(ValueError, match="min_support needs by='triplets' and replicates"):
        res.nni_candidates(by="triplets", min_support=0.5)


def test_the_pass_runs_last_with_the_drawn_weights(monkeypatch):
    monkeypatch.setattr(score_mod, "BATCH_TREES", 11)
    sup, trees = _sequence_case()
    dev = FakeDevice()
    res = score_supertree(sup, trees, branch_triplets=True, branch_resample=6, tree_weights=[1, 2, 3],
                          resample_seed=5, resample_rows=True, device=dev)
    assert dev.log == ["score", "score_branch_triplets", ("score_branch_resample", True, 11)]
    assert "branch_resample" in res.timings and dev.tabs.freed == 1
    want = rr.draws(3, 6, [1, 2, 3], "bootstrap", 5)
    assert np.array_equal(dev.weights, want) and np.array_equal(res.rs_weights, want)
    n = 7
    for x, name in enumerate(("rs_total", "rs_concordant", "rs_alt1", "rs_alt2")):
        assert getattr(res, name).tolist() == list(range(100 + x * n, 100 + (x + 1) * n))
        assert getattr(res, name + "_rows").shape == (7, n)
        assert getattr(res, name + "_rows")[0, 0] == 1000 + x * 7 * n
    assert list(res.rs_wins) == list(rr.WIN_KEYS)
    assert res.rs_wins["win_alt1"].tolist() == list(range(n, 2 * n))
    share = np.arange(n) / np.maximum(np.arange(4 * n).reshape(4, n).sum(axis=0), 1)
    assert np.allclose(res.branch_support, share)
    # the dataclass fields are what they were: the results hang beside them
    assert "rs_point" not in {f.name for f in score_mod.fields(SupertreeScore)}


def test_tree_weights_alone_give_row_0_and_no_wins():
    sup, trees = _sequence_case()
    dev = FakeDevice()
    res = score_supertree(sup, trees, tree_weights=[4, 0, 1], device=dev)
    assert dev.log == ["score", ("score_branch_resample", False, 0)]
    assert dev.weights.tolist() == [[4, 0, 1]] and res.rs_weights.tolist() == [[4, 0, 1]]
    assert res.rs_total.shape == (7,) and res.rs_total_rows is None
    assert res.rs_wins is None and res.branch_support is None


def test_jackknife_and_an_explicit_matrix_reach_the_device():
    sup, trees = _sequence_case()
    dev = FakeDevice()
    score_supertree(sup, trees, branch_resample=4, resample="jackknife", resample_seed=2, device=dev)
    assert np.array_equal(dev.weights, rr.draws(3, 4, None, "jackknife", 2))
    score_supertree(sup, trees, branch_resample=[[0, 0, 7], [1, 1, 1]], device=dev)
    assert dev.weights.tolist() == [[1, 1, 1], [0, 0, 7], [1, 1, 1]]


def test_weights_follow_their_trees_into_the_tables_order():
    # a TreeArrays input: the tables drop the trees of fewer than two leaves and name the given tree behind each of
    # theirs; the columns of the weights go with them, and the result keeps the matrix as given
    sup, _ = _sequence_case()
    parent, taxon, tips = score_mod.supertree_arrays(sup)
    forest = types.SimpleNamespace(tables=lambda: (None, None, None, None, [0, 2, 3]))
    dev = FakeDevice()
    dev.tabs = FakeTables(3)
    src = score_mod._Sources(dev, dev.tabs, np.array([3, 1, 3, 2]), 0.0, forest)
    given = resample_weights(4, [[5, 6, 7, 8], [0, 9, 0, 1]], [1, 2, 3, 4])
    req = score_mod._Request(False, False, False, False, False, None, None, 64, tips, resample=given)
    res = score_mod._run_passes(src, parent, taxon, req, {})
    assert dev.log == ["score", ("score_branch_resample", False, 0)]
    assert dev.weights.tolist() == [[1, 3, 4], [5, 7, 8], [0, 0, 1]]
    assert np.array_equal(res["rs_weights"], given)
    # no tree of two leaves: no tables, no call, zeros
    dev = FakeDevice()
    src = score_mod._Sources(dev, None, np.array([1, 1, 1, 0]), 0.0)
    res = score_mod._run_passes(src, parent, taxon, score_mod.replace(req, resample_rows=True), {})
    assert dev.log == [] and not res["rs_point"].any() and res["rs_point"].shape == (4, 7)
    assert res["rs_rows"].shape == (4, 3, 7) and not any(v.any() for v in res["rs_wins"].values())


# ------------------------------------------------------------------ what the replicates filter
def _scored(**rs):
    sup = make_tree("(((a,b),c),(d,(e,f)));")
    n = len(sup.to_flat()[0])
    zeros = np.zeros(n, dtype=np.int64)
    res = SupertreeScore(sup, None, None, None, None, zeros, zeros)
    res._rs = rs or None
    return res, n


def test_nni_candidates_keep_what_the_replicates_repeat():
    res, n = _scored()
    assert np.flatnonzero(res.quartet_branch).tolist() == [1, 2, 6, 8]
    bt = {"bt_total": [0, 0, 50, 0, 0, 0, 0, 0, 40, 0, 0], "bt_concordant": [0, 0, 10, 0, 0, 0, 0, 0, 10, 0, 0],
          "bt_alt1": [0, 0, 30, 0, 0, 0, 0, 0, 5, 0, 0], "bt_alt2": [0, 0, 5, 0, 0, 0, 0, 0, 20, 0, 0]}
    for k, v in bt.items():
        setattr(res, k, np.array(v, dtype=np.int64))
    plain = res.nni_candidates(by="triplets")
    assert [(r["node"], r["alternative"], r["margin"]) for r in plain] == [(2, "alt1", 20), (8, "alt2", 10)]
    wins = np.zeros((4, n), dtype=np.int32)
    wins[:, 2] = [1, 8, 0, 1]   # alt1 wins 8 of 10 informative replicates
    wins[:, 8] = [3, 0, 3, 0]   # alt2 wins 3 of 6
    point = np.array([bt["bt_total"], bt["bt_concordant"], bt["bt_alt1"], bt["bt_alt2"]], dtype=np.int64)
    res._rs = {"rs_weights": np.ones((11, 3), dtype=np.int64), "rs_point": point, "rs_rows": None,
               "rs_wins": dict(zip(rr.WIN_KEYS, wins))}
    assert res.nni_candidates(by="triplets") == plain  # (unchanged without min_support)
    kept = res.nni_candidates(by="triplets", min_support=0.75)
    assert [(r["node"], r["alternative"], r["replicate_share"]) for r in kept] == [(2, "alt1", 0.8)]
    assert [r["node"] for r in res.nni_candidates(by="triplets", min_support=0.5)] == [2, 8]
    assert res.nni_candidates(by="triplets", min_support=0.9) == []
    with pytest.raises(ValueError, match="min_support needs by='triplets'"):
        res.nni_candidates(by="sources", min_support=0.5)
    # the point estimates stand in where the unweighted counts were not computed
    for k in bt:
        setattr(res, k, None)
    assert [r["node"] for r in res.nni_candidates(by="triplets", min_support=0.75)] == [2]
    # support in percent as the branches' names; no name where no replicate is informative
    wins[:, 8] = 0
    named = res.annotate_branch_support().get_newick(with_node_names=True)
    assert named.count("10.0") == 1 and "nan" not in named, named
    assert np.isnan(res.branch_support[8]) and res.branch_support[2] == 0.1


# ------------------------------------------------------------------ the boundary
def test_the_header_declares_the_export_and_the_binding_requires_it(monkeypatch):
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int " + EXPORT + r"\(([^;]*)\);", header)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "sources", "n_nodes", "parent", "taxon", "max_batch_trees", "n_rep", "weights",
                     "rs_point", "rs_wins", "rs_rows"]
    restype, argtypes = _native.SIGNATURES[EXPORT]
    assert restype is _native.C.c_int and len(argtypes) == len(params)
    assert argtypes[:6] == _native.SIGNATURES["scs_score_branch_triplets"][1][:6]
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header
    assert hasattr(_native.load_library(), EXPORT)

    class Without:
        """A library that exports every symbol but this one."""

        def __getattr__(self, name):
            if name == EXPORT:
                raise AttributeError(name)
            return types.SimpleNamespace(restype=None, argtypes=None)

    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native.C, "CDLL", lambda path: Without())
    with pytest.raises(AttributeError, match=EXPORT):
        _native.load_library()
    assert _native._lib is None
