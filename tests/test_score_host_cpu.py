"""The host layer of the scoring passes without a device or the library: what ``Device.score*`` hand to the exports
and make of their answers, which passes ``score_supertree`` runs in which order with which knobs, and that the three
prune-and-regraft entry points (``regraft``, ``regraft_clade``, ``apply_moves``) build the same trees."""

import ctypes as C
import dataclasses
import types

import numpy as np
import pytest
import score_reference as sr

from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import score as score_mod
from spectralclustersupertree_amd import score_supertree
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.refine import apply_moves, subtree_ends
from spectralclustersupertree_amd.score import SupertreeScore
from spectralclustersupertree_amd.tree import make_tree

# ((a,b),(c,d)); in preorder: 7 nodes, 4 tips; 3 source trees, 2 queries, top_k = 3
PARENT = [-1, 0, 1, 1, 0, 4, 4]
TAXON = [-1, -1, 0, 1, -1, 2, 3]
N, M, TIPS, NQ, K = 7, 3, 4, 2, 3
QUERIES = [3, 1]
I64, I32 = np.int64, np.int32


def _spec(*groups):
    """[(name, dtype, shape, fill)] from (names, shape[, dtype, fill]) groups."""
    out = []
    for names, shape, *rest in groups:
        dtype, fill = rest if rest else (I64, 0)
        out += [(k, dtype, shape, fill) for k in names]
    return out


# method -> (export, keyword arguments, the scalar arguments after ``taxon`` ("Q": the query buffer), outputs)
CALLS = {
    "score": ("scs_score_supertree", {"batch_trees": 5}, (5,),
              _spec((("n_super", "n_source", "shared"), (M,)), (("informative", "supported"), (N,)))),
    "score_triplets": ("scs_score_triplets", {"batch_trees": 5}, (5,),
                       _spec((("t_super", "t_source", "t_shared"), (M,)))),
    "score_conflicts": ("scs_score_conflicts", {"batch_trees": 5}, (5,),
                        _spec((("n_super_conflict", "n_source_conflict"), (M,)), (("conflicting",), (N,)))),
    "score_concordance": ("scs_score_concordance", {"batch_trees": 5}, (5,),
                          _spec((("n_decisive", "n_concordant", "n_alternative"), (M,)),
                                (("decisive", "concordant", "alt1", "alt2"), (N,)))),
    "score_branch_triplets": ("scs_score_branch_triplets", {"batch_trees": 5}, (5,),
                              _spec((("n_bt_total", "n_bt_concordant", "n_bt_alternative"), (M,)),
                                    (("bt_total", "bt_concordant", "bt_alt1", "bt_alt2"), (N,)))),
    "score_taxon_triplets": ("scs_score_taxon_triplets", {"batch_trees": 5, "lds_bytes": 9}, (5, 9),
                             _spec((("tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared"), (TIPS,)))),
    "score_placements": ("scs_score_placements", {"queries": QUERIES, "batch_trees": 5, "lds_bytes": 9},
                         (5, 9, NQ, "Q"),
                         _spec((("pl_trees", "pl_total", "pl_source"), (NQ,)), (("pl_super", "pl_shared"), (NQ, N)))),
    "score_clade_placements": ("scs_score_clade_placements",
                               {"query_nodes": QUERIES, "batch_trees": 5, "lds_bytes": 9}, (5, 9, NQ, "Q"),
                               _spec((("cp_trees", "cp_total", "cp_source"), (NQ,)),
                                     (("cp_super", "cp_shared"), (NQ, N)))),
    "score_clade_moves": ("scs_score_clade_moves",
                          {"query_nodes": QUERIES, "top_k": K, "batch_trees": 5, "lds_bytes": 9},
                          (5, 9, NQ, "Q", K),
                          _spec((("cp_trees", "cp_total", "cp_source", "mv_own_super", "mv_own_shared"), (NQ,)),
                                (("mv_node",), (NQ, K), I32, -1), (("mv_super", "mv_shared"), (NQ, K)))),
}


def _at(address: int, dtype, count: int) -> np.ndarray:
    """The ``count`` items of ``dtype`` at a raw address, as a writable view."""
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(address), dtype=dt, count=count)


def _ramp(i: int, dtype, shape) -> np.ndarray:
    return (100 * (i + 1) + np.arange(int(np.prod(shape)))).astype(dtype).reshape(shape)


class FakeLib:
    """``scs_score_*`` record their arguments, what the buffers held, and write a ramp into every output."""

    def __init__(self, outputs, n_scalars, rc=0, message=b""):
        self.outputs, self.n_scalars, self.rc, self.message = outputs, n_scalars, rc, message
        self.calls = []

    def scs_last_error(self):
        return self.message

    def __getattr__(self, export):
        if not export.startswith("scs_score_"):
            raise AttributeError(export)

        def call(*args):
            head, outs = args[:5 + self.n_scalars], args[5 + self.n_scalars:]
            assert len(outs) == len(self.outputs)
            seen = {"export": export, "args": head, "parent": _at(head[3], I32, head[2]).copy(),
                    "taxon": _at(head[4], I32, head[2]).copy(), "before": []}
            for i, (addr, (_, dtype, shape, _)) in enumerate(zip(outs, self.outputs)):
                buf = _at(addr, dtype, int(np.prod(shape)))
                seen["before"].append(buf.copy())
                buf[:] = _ramp(i, dtype, shape).ravel()
            self.calls.append(seen)
            return self.rc

        return call


def _device(lib) -> Device:
    dev = Device.__new__(Device)
    dev._lib, dev._ctx = lib, C.c_void_p()  # (a null context: ``close`` has nothing to destroy)
    return dev


@pytest.mark.parametrize("method", list(CALLS))
def test_device_method_marshals_its_export(method):
    export, kwargs, scalars, outputs = CALLS[method]
    lib = FakeLib(outputs, len(scalars))
    dev = _device(lib)
    tabs = types.SimpleNamespace(_h=object(), n_trees=M)
    got = getattr(dev, method)(tabs, np.array(PARENT, dtype=I64), list(TAXON), **kwargs)
    (seen,) = lib.calls
    assert seen["export"] == export
    args = seen["args"]
    assert args[0] is dev._ctx and args[1] is tabs._h and args[2] == N
    assert seen["parent"].tolist() == PARENT and seen["taxon"].tolist() == TAXON
    for value, want in zip(args[5:], scalars):
        if want == "Q":
            assert _at(value, I32, NQ).tolist() == QUERIES
        else:
            assert type(value) is int and value == want
    assert list(got) == [name for name, *_ in outputs]
    for i, (name, dtype, shape, fill) in enumerate(outputs):
        assert got[name].dtype == dtype and got[name].shape == shape, name
        assert np.array_equal(got[name], _ramp(i, dtype, shape)), name
        assert seen["before"][i].dtype == dtype and (seen["before"][i] == fill).all(), name


@pytest.mark.parametrize("method", list(CALLS))
def test_device_method_maps_einval_and_checks_shapes_first(method):
    export, kwargs, scalars, outputs = CALLS[method]
    tabs = types.SimpleNamespace(_h=object(), n_trees=M)
    dev = _device(FakeLib(outputs, len(scalars), rc=nv.EINVAL, message=b"the export said no"))
    with pytest.raises(ValueError, match="^the export said no$"):
        getattr(dev, method)(tabs, PARENT, TAXON, **kwargs)
    for empty in (b"", None):
        dev = _device(FakeLib(outputs, len(scalars), rc=nv.EINVAL, message=empty))
        with pytest.raises(ValueError, match=f"^{export}: invalid input$"):
            getattr(dev, method)(tabs, PARENT, TAXON, **kwargs)
    lib = FakeLib(outputs, len(scalars))
    with pytest.raises(ValueError, match="^parent and taxon must have one entry per supertree node"):
        getattr(_device(lib), method)(tabs, PARENT, TAXON[:-1], **kwargs)
    assert lib.calls == []


# ------------------------------------------------------------------ the pass sequence, tree-object path
class FakeTables:
    def __init__(self, n_trees):
        self.n_trees, self.freed = n_trees, 0

    def free(self):
        self.freed += 1


class FakeDevice:
    """``upload`` and the nine methods: zeros of the right shapes (ones where ``ones`` names the key), logged."""

    def __init__(self, fail=None, ones=()):
        self.log, self.fail, self.ones, self.tabs = [], fail, ones, None

    def upload(self, tables):
        self.tabs = FakeTables(tables.n_trees)
        return self.tabs

    def __getattr__(self, method):
        if method not in CALLS:
            raise AttributeError(method)

        def call(tabs, parent, taxon, *queries, **kwargs):
            assert tabs is self.tabs and not tabs.freed
            self.log.append((method, kwargs))
            if method == self.fail:
                raise RuntimeError("the pass failed")
            sizes = {M: tabs.n_trees, N: len(parent), TIPS: int((np.asarray(taxon) >= 0).sum()),
                     NQ: len(queries[0]) if queries else 0}
            return {name: np.full(tuple(sizes[s] for s in shape), int(name in self.ones), dtype=dtype)
                    for name, dtype, shape, _ in CALLS[method][3]}

        return call


GROUPS = {
    "triplets": ("t_super", "t_source", "t_shared"),
    "conflicts": ("n_super_conflict", "n_source_conflict", "conflicting"),
    "concordance": ("n_decisive", "n_concordant", "n_alternative", "decisive", "concordant", "alt1", "alt2"),
    "branch_triplets": ("n_bt_total", "n_bt_concordant", "n_bt_alternative", "bt_total", "bt_concordant", "bt_alt1",
                        "bt_alt2"),
    "taxon_triplets": ("taxa", "tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared"),
    "placements": ("pl_taxa", "pl_trees", "pl_total", "pl_source", "pl_super", "pl_shared"),
    "clade_placements": ("cp_nodes", "cp_trees", "cp_total", "cp_source", "cp_super", "cp_shared"),
}
BATCH, LDS_TX, LDS_PL, LDS_CP = 11, 22, 33, 44
PLAIN, TAXA = {"batch_trees": BATCH}, {"batch_trees": BATCH, "lds_bytes": LDS_TX}


def _sequence_case():
    return make_tree("((a,b),(c,d));"), [make_tree("((a,b),c);"), make_tree("(a,(c,d));"), make_tree("(b,c,d);")]


@pytest.fixture
def knobs(monkeypatch):
    monkeypatch.setattr(score_mod, "BATCH_TREES", BATCH)
    monkeypatch.setattr(score_mod, "TAXON_LDS_BYTES", LDS_TX)
    monkeypatch.setattr(score_mod, "PLACEMENT_LDS_BYTES", LDS_PL)
    monkeypatch.setattr(score_mod, "CLADE_PLACEMENT_LDS_BYTES", LDS_CP)


def _none_fields(res) -> set:
    return {f.name for f in dataclasses.fields(res) if getattr(res, f.name) is None}


def _all_of(*groups) -> set:
    return {name for g in groups for name in GROUPS[g]}


def test_score_supertree_alone_runs_one_pass(knobs):
    sup, trees = _sequence_case()
    dev = FakeDevice()
    res = score_supertree(sup, trees, device=dev)
    assert dev.log == [("score", PLAIN)]
    assert set(res.timings) == {"prepare", "tables", "score"}
    assert _none_fields(res) == _all_of(*GROUPS)
    assert res.n_leaves.tolist() == [3, 3, 3] and res.n_super.shape == (3,) and res.informative.shape == (7,)
    assert dev.tabs.freed == 1


def test_score_supertree_with_everything_runs_the_passes_in_order(knobs):
    sup, trees = _sequence_case()
    dev = FakeDevice()
    res = score_supertree(sup, trees, triplets=True, conflicts=True, concordance=True, branch_triplets=True,
                          taxon_triplets=True, placements=["a"], clade_placements=[1], device=dev)
    assert dev.log == [("score", PLAIN), ("score_triplets", PLAIN), ("score_conflicts", PLAIN),
                       ("score_concordance", PLAIN), ("score_branch_triplets", PLAIN),
                       ("score_taxon_triplets", TAXA),
                       ("score_placements", {"batch_trees": BATCH, "lds_bytes": LDS_PL}),
                       ("score_clade_placements", {"batch_trees": BATCH, "lds_bytes": LDS_CP})]
    assert set(res.timings) == {"prepare", "tables", "score", *GROUPS}
    assert _none_fields(res) == set()
    assert res.taxa == ["a", "b", "c", "d"] and res.pl_taxa.tolist() == [0] and res.cp_nodes.tolist() == [1]
    assert res.pl_taxa.dtype == I64 and res.cp_nodes.dtype == I64
    assert res.pl_super.shape == (1, 7) and res.cp_shared.shape == (1, 7) and res.tx_trees.shape == (4,)
    assert dev.tabs.freed == 1


def test_a_placement_count_alone_implies_the_taxon_triplets(knobs):
    sup, trees = _sequence_case()
    # every taxon in a source and fully unstable: taxon 0 is the least stable one
    dev = FakeDevice(ones=("tx_trees", "tx_super", "tx_source"))
    res = score_supertree(sup, trees, placements=1, device=dev)
    assert dev.log == [("score", PLAIN), ("score_taxon_triplets", TAXA),
                       ("score_placements", {"batch_trees": BATCH, "lds_bytes": LDS_PL})]
    assert set(res.timings) == {"prepare", "tables", "score", "taxon_triplets", "placements"}
    assert _none_fields(res) == _all_of("triplets", "conflicts", "concordance", "branch_triplets", "clade_placements")
    assert res.pl_taxa.tolist() == [0] and res.taxa == ["a", "b", "c", "d"]
    # no taxon in a source: no query, and the placement pass is not sent to the device
    dev = FakeDevice()
    res = score_supertree(sup, trees, placements=1, device=dev)
    assert dev.log == [("score", PLAIN), ("score_taxon_triplets", TAXA)]
    assert set(res.timings) == {"prepare", "tables", "score", "taxon_triplets", "placements"}
    assert res.pl_taxa.shape == (0,) and res.pl_trees.shape == (0,) and res.pl_super.shape == (0, 7)
    assert dev.tabs.freed == 1


@pytest.mark.parametrize("fail", ["score", "score_conflicts", "score_clade_placements"])
def test_the_tables_are_freed_when_a_pass_raises(knobs, fail):
    sup, trees = _sequence_case()
    dev = FakeDevice(fail=fail)
    with pytest.raises(RuntimeError, match="the pass failed"):
        score_supertree(sup, trees, triplets=True, conflicts=True, concordance=True, branch_triplets=True,
                        taxon_triplets=True, placements=["a"], clade_placements=[1], device=dev)
    assert dev.log[-1][0] == fail and dev.tabs.freed == 1


# ------------------------------------------------------------------ one prune-and-regraft
@pytest.fixture(scope="module")
def regraft_trees():
    rs = np.random.RandomState(24)
    return [sr.random_tree(rs, [f"t{i}" for i in range(int(rs.randint(2, 10)))], polytomy=0.3, unary=0.15)
            for _ in range(240)]


def test_regraft_of_a_tip_is_regraft_clade_of_its_node(regraft_trees):
    same = own = 0
    for sup in regraft_trees:
        view = SupertreeScore(sup, None, None, None, None, None, None)
        before = sup.get_newick()
        nodes = sr._preorder(sup)
        tip_nodes = [i for i, v in enumerate(nodes) if v.is_tip()]
        for x, q in enumerate(tip_nodes):
            for v in range(len(nodes)):
                got = view.regraft(x, v).get_newick()
                assert got == view.regraft(nodes[q].name, v).get_newick()
                if v == q:
                    assert got == before
                    with pytest.raises(ValueError, match="inside"):
                        view.regraft_clade(q, v)
                    own += 1
                else:
                    assert got == view.regraft_clade(q, v).get_newick(), (before, x, v)
                    same += 1
        assert sup.get_newick() == before
    assert same > 5000 and own > 1000, (same, own)


def test_one_move_of_apply_moves_is_regraft_clade(regraft_trees):
    same = refused = 0
    for sup in regraft_trees:
        view = SupertreeScore(sup, None, None, None, None, None, None)
        n = len(sup.to_flat()[0])
        ends = subtree_ends(sup.to_flat()[0])
        for q in range(1, n):
            for v in range(n):
                if q <= v < ends[q]:
                    with pytest.raises(ValueError, match="inside"):
                        view.regraft_clade(q, v)
                    with pytest.raises(ValueError, match="inside"):
                        apply_moves(sup, [(q, v)])
                    refused += 1
                else:
                    assert apply_moves(sup, [(q, v)]).get_newick() == view.regraft_clade(q, v).get_newick(), (q, v)
                    same += 1
    assert same > 8000 and refused > 2000, (same, refused)
