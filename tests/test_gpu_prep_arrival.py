"""Prep by arrival (``scs_pcg_build``): tables uploaded from page-locked memory arrive in chunks behind the first 64
trees, and every tree batch is prepared piece by piece as the chunks land.  A forest large enough for three late
chunks -- 2 100 taxa, 700 trees of 1 050 to 2 100 leaves, about 17 MB of leaf arrays: chunks [64, 320), [320, 576),
[576, 700) -- with trees of unequal size, so that a piece that starts at the wrong tree-in-batch offset writes into
another tree's tables.  Whole W bit for bit against the C oracle on every path."""

import numpy as np
import pytest

from oracle import tables_oracle as to
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd import synthetic
from spectralclustersupertree_amd.backend import Device
from spectralclustersupertree_amd.flatten import TreeTables

pytestmark = pytest.mark.gpu

N_TAXA, N_TREES = 2100, 700
LATE_CHUNKS = ((64, 320), (320, 576), (576, 700))  # scs_tables_upload: 64 trees at once, then 256 a chunk


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


_CACHE: dict = {}


def _forest(strategy):
    """``(pageable tables, oracle W)`` of the forest under ``strategy``, made once and left unchanged."""
    if strategy not in _CACHE:
        rng = np.random.RandomState(2100)
        leaves = rng.randint(N_TAXA // 2, N_TAXA + 1, size=N_TREES)
        parts = [synthetic.make_tables(1000 + t, N_TAXA, 1, strategy, leaves_per_tree=int(k), random_weights=True)
                 for t, k in enumerate(leaves)]
        tree_off = np.zeros(N_TREES + 1, dtype=np.int64)
        np.cumsum(leaves, out=tree_off[1:])
        tb = TreeTables(N_TAXA, tree_off, np.concatenate([p.leaf_taxon for p in parts]),
                        np.concatenate([p.adj_depth for p in parts]), np.concatenate([p.adj_val for p in parts]),
                        np.concatenate([p.tree_w for p in parts]), None, monotone=strategy != "bootstrap")
        assert tb.n_leaves * 16 >= 8 << 20 and len(set(leaves.tolist())) > 100
        w = to.pcg_dense_mt(tb, 16)
        w.flags.writeable = False
        _CACHE[strategy] = (tb, w)
    return _CACHE[strategy]


def _pinned(tb):
    """The same tables in page-locked arrays: ``Device.upload`` then sends all but the first 64 trees in chunks."""
    def copy(a):
        out = nv.pinned_empty(a.shape, a.dtype)
        out[...] = a
        return out

    return TreeTables(tb.n_taxa, copy(tb.tree_off), copy(tb.leaf_taxon), copy(tb.adj_depth), copy(tb.adj_val),
                      copy(tb.tree_w), None, monotone=tb.monotone)


def _build(dev, tb):
    dtab = dev.upload(tb)
    try:
        g = dtab.build()
        try:
            return g.download(), g.build_stats
        finally:
            g.free()
    finally:
        dtab.free()


def _pieces(batch_starts, cut=True):
    """Prep pieces of the batches ``batch_starts`` (with the end): one per batch and one more per late-chunk start
    strictly inside a batch."""
    inside = sum(1 for a, b in zip(batch_starts[:-1], batch_starts[1:]) for c, _ in LATE_CHUNKS if a < c < b)
    return len(batch_starts) - 1 + (inside if cut else 0)


SWITCHES = ("SCS_WIDE", "SCS_BATCH_TREES", "SCS_PREP_BY_ARRIVAL", "SCS_TREE_PARALLEL", "SCS_TILE_LISTS", "SCS_NO_MONOTONE")


BATCHES_OF_100 = [0, 64, 164, 264, 364, 464, 564, 664, 700]  # [264, 364) holds the start of chunk 320, [564, 664) of 576
VARIANTS = {  # name: (strategy, switches)
    "default": ("branch", {}),
    "narrow": ("branch", {"SCS_WIDE": "0"}),
    "batches_of_100": ("branch", {"SCS_BATCH_TREES": "100"}),
    # the 4-wave and the general prep kernels with a piece that starts inside a batch (their own batches of 256 trees
    # end where the chunks do)
    "narrow_batches_of_100": ("branch", {"SCS_WIDE": "0", "SCS_BATCH_TREES": "100"}),
    "bootstrap": ("bootstrap", {}),
    "bootstrap_batches_of_100": ("bootstrap", {"SCS_BATCH_TREES": "100"}),
    "switch_off": ("branch", {"SCS_PREP_BY_ARRIVAL": "0"}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_pieces_by_arrival_give_the_oracles_w(dev, monkeypatch, variant):
    for env in SWITCHES:
        monkeypatch.delenv(env, raising=False)
    strategy, env = VARIANTS[variant]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    tb, w_ref = _forest(strategy)
    w, st = _build(dev, _pinned(tb))
    print(f"[arrival] {variant}: {st['n_batches']} batches, {st['prep_pieces']} pieces, prep {st['prep_ms']:.3f} ms")
    diff = w != w_ref
    assert not diff.any(), f"{variant}: {int(diff.sum())} cells differ, first at {np.argwhere(diff)[:5].tolist()}"
    assert st["n_batches"] >= 2
    if variant == "switch_off":
        assert st["prep_pieces"] == st["n_batches"] == 3
    elif variant in ("narrow", "bootstrap"):
        # the 4-wave and general kernels' batches of 256 trees end where the chunks do: a piece each, none cut
        assert st["n_batches"] == 4 and st["prep_pieces"] == _pieces([0, 64, 320, 576, 700]) == 4
    elif variant == "default":
        # 64 arrived trees, then the 636 others in two batches of 318: [64, 382) holds the start of chunk [320, 576),
        # [382, 700) that of [576, 700)
        assert st["n_batches"] == 3 and st["spec_batches"] == 2 and st["prep_pieces"] == _pieces([0, 64, 382, 700]) == 5
    else:  # two batches are cut inside: their second pieces start at tree-in-batch 56 and 12
        assert st["n_batches"] == len(BATCHES_OF_100) - 1 and st["prep_pieces"] == _pieces(BATCHES_OF_100) == 10
    if "narrow" in variant or "bootstrap" in variant:
        assert st["spec_batches"] == 0
    if variant == "batches_of_100":
        assert st["spec_batches"] == 6  # (the batches of 100 trees; the first 64 and the last 36 are the 4-wave kernel's)


def test_pageable_tables_are_one_piece_per_batch(dev, monkeypatch):
    for env in SWITCHES:
        monkeypatch.delenv(env, raising=False)
    tb, w_ref = _forest("branch")
    w, st = _build(dev, tb)
    assert np.array_equal(w, w_ref)
    assert st["prep_pieces"] == st["n_batches"] >= 1
