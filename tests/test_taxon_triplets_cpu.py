"""Per-taxon triplet support without a device: the two host references against each other and against the per-tree
triplet sums, the C declaration against the binding, and the views of ``SupertreeScore`` on hand-filled counts."""

import re
from math import comb
from pathlib import Path

import numpy as np
import pytest
import score_reference as sr
import taxon_triplet_reference as xr
import triplet_reference as tr
from click.testing import CliRunner
from reference_cases import DATA_DIR

from spectralclustersupertree_amd import SupertreeScore, _native
from spectralclustersupertree_amd.cli import scs
from spectralclustersupertree_amd.tree import make_tree

KEYS = (*xr.KEYS, "taxon_triplet_distance")


@pytest.fixture(scope="module")
def cases():
    rs = np.random.RandomState(41)
    out = []
    for _ in range(160):
        sup, trees = sr.random_case(rs)
        out.append((sup, trees, xr.brute_force(sup, trees)))
    return out


def test_by_hand():
    # S = ((a,b),(c,d)), T = ((a,c),b): one triple, ac|b in T and ab|c in S'; d is in no source
    ref = xr.brute_force(make_tree("((a,b),(c,d));"), [make_tree("((a,c),b);"), make_tree("(a,b);")])
    assert ref["tx_trees"].tolist() == [1, 1, 1, 0] and ref["tx_total"].tolist() == [1, 1, 1, 0]
    assert ref["tx_super"].tolist() == ref["tx_source"].tolist() == [1, 1, 1, 0]
    assert ref["tx_shared"].tolist() == [0, 0, 0, 0] and ref["taxon_triplet_distance"].tolist() == [2, 2, 2, 0]
    # T = (((a,b),c),d) against itself: every triple resolved alike, C(3, 2) per taxon
    same = make_tree("(((a,b),c),d);")
    ref = xr.quadratic(same, [same])
    assert all(ref[k].tolist() == [3, 3, 3, 3] for k in ("tx_total", "tx_super", "tx_source", "tx_shared"))
    # d moved next to a: the triples without d stay, those with d are all resolved differently or lost
    ref = xr.quadratic(same, [make_tree("(((a,d),b),c);")])
    assert ref["tx_shared"].tolist() == [1, 1, 1, 0] and ref["taxon_triplet_distance"].tolist() == [4, 4, 4, 6]


def test_the_references_agree_on_random_cases(cases):
    for i, (sup, trees, brute) in enumerate(cases):
        quad = xr.quadratic(sup, trees)
        for k in KEYS:
            assert quad[k].dtype == np.int64 and np.array_equal(brute[k], quad[k]), (i, k)


def test_every_triple_has_three_taxa(cases):
    seen = 0
    for i, (sup, trees, brute) in enumerate(cases):
        per_tree = tr.quadratic(sup, trees)
        for k in ("shared", "super", "source"):
            assert brute[f"tx_{k}"].sum() == 3 * per_tree[f"t_{k}"].sum(), (i, k)
        sizes = [len(t.get_tip_names()) for t in trees]
        assert brute["tx_total"].sum() == 3 * sum(comb(m, 3) for m in sizes), i
        assert brute["tx_trees"].sum() == sum(m for m in sizes if m >= 3), i
        assert (brute["tx_shared"] <= np.minimum(brute["tx_super"], brute["tx_source"])).all(), i
        assert (np.maximum(brute["tx_super"], brute["tx_source"]) <= brute["tx_total"]).all(), i
        seen += int(brute["tx_shared"].sum() > 0)
    assert seen > 50  # (the cases are not all trivial)


def test_the_header_declares_the_symbol_and_the_binding_holds_it():
    header = (Path(__file__).resolve().parent.parent / "include" / "scs_hip.h").read_text()
    decl = re.search(r"int scs_score_taxon_triplets\(([^;]*)\);", header)
    assert decl is not None
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    restype, argtypes = _native.SIGNATURES["scs_score_taxon_triplets"]
    assert restype is _native.C.c_int and len(params) == len(argtypes) == 12
    ctype = {"scs_ctx *": _native.C.c_void_p, "const scs_tables *": _native.C.c_void_p,
             "int32_t ": _native.C.c_int32, "const int32_t *": _native.C.c_void_p, "int64_t *": _native.C.c_void_p}
    names = []
    for p, arg in zip(params, argtypes):
        name = re.search(r"(\w+)$", p).group(1)
        assert ctype[p[: -len(name)]] is arg, p
        names.append(name)
    assert names == ["ctx", "sources", "n_nodes", "parent", "taxon", "max_batch_trees", "max_lds_bytes", *xr.KEYS]
    assert _native.ABI_VERSION == 109 and "ABI version of this header: 109." in header


SUP = "(((a,b),c),(d,e));"


def _score(**extra):
    one = np.ones(2, dtype=np.int64)
    z = np.zeros(9, dtype=np.int64)
    return SupertreeScore(make_tree(SUP), np.array([5, 4]), one, one, one, z, z.copy(), {}, **extra)


def _counts() -> dict:
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    return {"taxa": ["a", "b", "c", "d", "e"], "tx_trees": i64(2, 2, 1, 2, 0), "tx_total": i64(9, 9, 6, 9, 0),
            "tx_super": i64(8, 8, 4, 0, 0), "tx_source": i64(8, 4, 4, 0, 0), "tx_shared": i64(8, 3, 0, 0, 0)}


def test_views_refuse_without_the_counts():
    plain = _score()
    assert plain.tx_shared is None and plain.taxa is None
    for call in (lambda: plain.taxon_triplet_distance, lambda: plain.taxon_fit, lambda: plain.taxon_instability,
                 plain.rogue_taxa, plain.taxon_table):
        with pytest.raises(ValueError, match=r"score_supertree\(\.\.\., taxon_triplets=True\)"):
            call()
    assert plain.table().splitlines()[0] == "index\tn_leaves\tn_super\tn_source\tshared\trf"


def test_views_of_the_counts():
    res = _score(**_counts())
    assert res.taxon_triplet_distance.tolist() == [0, 6, 8, 0, 0]
    fit, inst = res.taxon_fit, res.taxon_instability
    assert fit[:3].tolist() == [1.0, 0.75, 0.0] and np.isnan(fit[3:]).all()
    assert inst[:3].tolist() == [0.0, 0.5, 1.0] and np.isnan(inst[3:]).all()
    rogue = res.rogue_taxa()
    assert [r["name"] for r in rogue] == ["c", "b", "a"]  # (d and e have no defined instability)
    assert rogue[0] == {"taxon": 2, "name": "c", "trees": 1, "total": 6, "super": 4, "source": 4, "shared": 0,
                        "distance": 8, "instability": 1.0}
    assert [r["taxon"] for r in res.rogue_taxa(n=2)] == [2, 1]
    assert [r["taxon"] for r in res.rogue_taxa(min_trees=2)] == [1, 0]
    assert res.rogue_taxa(n=0) == [] and res.rogue_taxa(min_trees=3) == []


def test_rogue_taxa_break_ties_by_distance_then_id():
    counts = _counts()
    i64 = lambda *v: np.array(v, dtype=np.int64)  # noqa: E731
    counts.update(tx_super=i64(4, 8, 4, 2, 2), tx_source=i64(4, 8, 4, 2, 2), tx_shared=i64(2, 4, 2, 1, 1),
                  tx_trees=i64(1, 1, 1, 1, 1))
    # every instability is 1/2; distances 4, 8, 4, 2, 2
    assert [r["taxon"] for r in _score(**counts).rogue_taxa()] == [1, 0, 2, 3, 4]


def test_taxon_table_text():
    assert _score(**_counts()).taxon_table() == (
        "taxon\tname\ttx_trees\ttx_total\ttx_super\ttx_source\ttx_shared\ttriplet_distance\n"
        "0\ta\t2\t9\t8\t8\t8\t0\n"
        "1\tb\t2\t9\t8\t4\t3\t6\n"
        "2\tc\t1\t6\t4\t4\t0\t8\n"
        "3\td\t2\t9\t0\t0\t0\t0\n"
        "4\te\t0\t0\t0\t0\t0\t0\n")


def test_the_other_tables_do_not_change():
    plain, full = _score(), _score(**_counts())
    assert plain.table() == full.table()


def test_cli_taxon_triplets_needs_a_table(tmp_path):
    res = CliRunner().invoke(scs, ["-i", str(DATA_DIR / "dcm_iq_source.tre"), "-o", str(tmp_path / "out.tre"),
                                   "--taxon-triplets"])
    assert res.exit_code == 2 and "--taxon-triplets needs --taxa-out" in res.output
