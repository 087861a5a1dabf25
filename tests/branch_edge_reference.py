"""Builders, closed forms, an array reference and the host plans for the edges of the three scoring exports built on
``k_bt_*``, ``k_tx_*`` and ``k_rs_*`` (``csrc/scs_score.hip``: ``scs_score_branch_triplets``,
``scs_score_taxon_triplets``, ``scs_score_branch_resample``; the cases of ``tests/test_gpu_branch_taxon_edges.py``,
held to their numbers by ``tests/test_branch_edge_reference_cpu.py``).  CPU only; beside ``score_edge_reference``, whose
builders it reuses.

The references stay the project's own where they can go -- ``branch_triplet_reference.brute_force`` / ``node_sum``,
``taxon_triplet_reference.brute_force`` / ``quadratic``, ``resample_reference.rows`` / ``wins``.  What is here:

* ``branch_arrays``: the sum of ``node_sum`` on integer arrays -- S ranges, T ranges, one prefix-count vector per set
  and decisive branch, no set per node -- for the sizes where ``node_sum``'s frozensets are too slow;
* closed forms for two caterpillars under a permutation (``comb_branches``, ``comb_taxa``) and for three-leaf sources on
  a caterpillar supertree (``three_leaf``), for all three exports;
* the plans of ``sc_bt_plan`` and ``sc_tx_plan_of`` / ``sc_tx_call_of`` / ``sc_tx_batches`` restated (``branch_plan``),
  compared with ``scs_debug_branch_plan``;
* ``needs``: |z| + |pz| + 2 of every node of the restricted supertree, which decides a node's bin;
* the cases, each a function of its name.
"""

from __future__ import annotations

from functools import lru_cache

import build_reference as br
import numpy as np
import score_edge_reference as se
import taxon_triplet_reference as xr

from spectralclustersupertree_amd.treearrays import TreeArrays

# ---- the constants of csrc/scs_score.hip the cases are placed by
BT_ZMAX = 8  # records per workgroup of k_bt_pairs / k_rs_pairs at most
BT_ROW_BYTES = 24  # LDS bytes per 32 T positions of one record
BT_WAVE_SUMS = (se.SC_THREADS // 64) * BT_ZMAX * 3 * 8  # 768 bytes: the least a launch takes
BT_CAP = se.TP_LDS_MAX // BT_ROW_BYTES * 32 - 1  # 218 431: the largest source tree of the branch exports
TX_BINS = 3
TX_SCRATCH = 64
TX_SLAB_PAD = 8
TX_SLAB_WGS = 256
TX_SLAB_BYTES = 128 << 20
TX_BIN_BUDGET = (20 << 10, 52 << 10, se.TP_LDS_MAX)
TX_BIN_ZMAX = (se.TP_ZMAX, 2, 1)
TX_SMALL = 192
TX_ROUND = 4 * se.SC_THREADS  # 1 024 entries a round of tx_scan
RS_TILE, RS_CHUNK, RS_AHEAD = 8, 512, 4

BRANCH = ("n_bt_total", "n_bt_concordant", "n_bt_alternative", "bt_total", "bt_concordant", "bt_alt1", "bt_alt2")
BRANCH_NODE = BRANCH[3:]
TAXON = xr.KEYS
C_NAME = {"score_branch_triplets": "scs_score_branch_triplets", "score_taxon_triplets": "scs_score_taxon_triplets",
          "score_branch_resample": "scs_score_branch_resample"}


# ------------------------------------------------------------------------------------------------ the host plans
def export_extras(export: str, n_nodes: int = 0) -> tuple[int, int]:
    """``(extra_per_leaf, extra_per_tree)`` the export hands to ``sc_begin``: an int4 and a 24-byte record a leaf and
    two counts a tree (branch); the same and the slab's 32 bytes a supertree node (resample); two int4, three sums and
    four bin entries a leaf, six counts a tree (taxon)."""
    return {"score_branch_triplets": (40, 8), "score_branch_resample": (40, 8 + 32 * n_nodes),
            "score_taxon_triplets": (72, 24)}[export]


def bt_words_zb(n_max: int) -> tuple[int, int, int]:
    """``(words, zb, launch bytes)`` of ``sc_bt_plan`` for a batch whose largest tree has ``n_max`` leaves."""
    words = (n_max >> 5) + 1
    zb = min(BT_ZMAX, max(1, se.TP_LDS_BUDGET // (BT_ROW_BYTES * words)))
    return words, zb, max(zb * BT_ROW_BYTES * words, BT_WAVE_SUMS)


def tx_plan_of(words: int, lds_cap: int = se.TP_LDS_MAX) -> dict:
    """``sc_tx_plan_of``: per bin ``zb``, ``dcap`` (0: not used) and launch bytes; ``dcap_max``."""
    rowb = 16 * words
    zbs, dcaps, ldss, dcap_max = [], [], [], 0
    for i in range(TX_BINS):
        base = (min(TX_BIN_BUDGET[1], max(TX_BIN_BUDGET[0], TX_SCRATCH + se.TP_ZMAX * (rowb + 8 * TX_SMALL)))
                if i == 0 else TX_BIN_BUDGET[i])
        budget = min(base, lds_cap)
        zb = min(TX_BIN_ZMAX[i], max(1, budget // (2 * rowb)))
        avail = budget - TX_SCRATCH - zb * rowb
        dcap = min(avail // (8 * zb), 64 * words) if avail > 0 else 0
        zbs.append(zb)
        dcaps.append(dcap if dcap >= 7 and dcap > dcap_max else 0)
        ldss.append(TX_SCRATCH + zb * (rowb + 8 * dcap))
        dcap_max = max(dcap_max, dcaps[-1])
    return {"zb": zbs, "dcap": dcaps, "lds": ldss, "dcap_max": dcap_max}


def tx_call_of(m_max: int, lds_bytes: int = 0) -> dict:
    """``sc_tx_call_of``: the LDS cap and the slab path of one call."""
    cap = min(lds_bytes, se.TP_LDS_MAX) if lds_bytes > 0 else se.TP_LDS_MAX
    stride = 2 * m_max + 2 + TX_SLAB_PAD
    need_slab = 2 * m_max + 1 > tx_plan_of((m_max >> 5) + 1, cap)["dcap_max"]
    wgs = min(TX_SLAB_WGS, max(1, TX_SLAB_BYTES // (stride * 8))) if need_slab else 0
    return {"lds_cap": cap, "need_slab": int(need_slab), "slab_wgs": wgs, "slab_stride": stride}


def bin_of(need: int, dcaps) -> int:
    """``k_tx_single``'s choice: the first bin that holds ``need`` entries, TX_BINS (the slab) when none does."""
    return next((i for i in range(TX_BINS) if need <= dcaps[i]), TX_BINS)


def branch_plan(tree_off, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0, extra_per_tree: int = 0,
                lds_bytes: int = 0) -> dict:
    """What ``backend.debug_branch_plan`` returns, restated."""
    off = [int(x) for x in tree_off]
    sizes = [off[t + 1] - off[t] for t in range(len(off) - 1)]
    bstart = se.plan(off, super_leaves, batch_trees, extra_per_leaf, extra_per_tree)["bstart"]
    call = tx_call_of(max(sizes, default=0), lds_bytes)
    rows = {k: [] for k in ("bt_words", "bt_zb", "bt_lds", "bt_workgroups", "tx_zb", "tx_dcap", "tx_lds",
                            "tx_workgroups", "tx_slab_launch", "tx_slab_lds")}
    wgs = lambda mine, z: sum((max(n - 2, 0) + z - 1) // z for n in mine)  # noqa: E731
    for b in range(len(bstart) - 1):
        mine = sizes[bstart[b]:bstart[b + 1]]
        w, z, lds = bt_words_zb(max(mine, default=0))
        p = tx_plan_of(w, call["lds_cap"])
        for k, v in (("bt_words", w), ("bt_zb", z), ("bt_lds", lds), ("bt_workgroups", wgs(mine, z)),
                     ("tx_zb", p["zb"]), ("tx_dcap", p["dcap"]), ("tx_lds", p["lds"]),
                     ("tx_workgroups", [wgs(mine, zi) for zi in p["zb"]]),
                     ("tx_slab_launch", int(call["slab_wgs"] > 0 and 64 * w > p["dcap_max"])), ("tx_slab_lds", 16 * w)):
            rows[k].append(v)
    out = {k: np.asarray(v, dtype=np.int64).reshape((len(bstart) - 1, TX_BINS) if k in (
        "tx_zb", "tx_dcap", "tx_lds", "tx_workgroups") else (len(bstart) - 1,)) for k, v in rows.items()}
    out.update(bstart=bstart, need_slab=call["need_slab"], slab_wgs=call["slab_wgs"], slab_stride=call["slab_stride"])
    return out


# ------------------------------------------------------------------------------------------------ trees as arrays
def tree_slice(arrays: TreeArrays, t: int) -> tuple[np.ndarray, np.ndarray]:
    lo, hi = int(arrays.node_off[t]), int(arrays.node_off[t + 1])
    return np.asarray(arrays.parent[lo:hi]), np.asarray(arrays.taxon[lo:hi])


def clusters(parent: np.ndarray, taxon: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A tree's distinct non-root clusters of two or more leaves as ranges of its leaf order: ``y`` and ``py``
    ([k, 2]: first position, last + 1; py the smallest cluster strictly above) and the tips' taxa in leaf order."""
    lo, hi = se.leaf_ranges(parent, taxon)
    v = np.arange(1, len(parent))
    u = parent[1:]
    keep = (hi[v] > lo[v]) & ((lo[v] != lo[u]) | (hi[v] != hi[u]))  # (a unary node's child repeats its set)
    v, u = v[keep], u[keep]
    return np.stack([lo[v], hi[v] + 1], 1), np.stack([lo[u], hi[u] + 1], 1), taxon[taxon >= 0]


def quartet_branches(parent: np.ndarray):
    """``(c, a, b, d)`` per quartet branch: an inner node with two children a (first in preorder), b whose parent has
    two children, c and d -- the library's ``q_parent`` rule."""
    n = len(parent)
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[parent[v]].append(v)
    out = []
    for c in range(1, n):
        u = parent[c]
        if len(kids[c]) == 2 and len(kids[u]) == 2:
            out.append((c, kids[c][0], kids[c][1], kids[u][1] if kids[u][0] == c else kids[u][0]))
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def restricted(parent: np.ndarray, taxon: np.ndarray, n_taxa: int, tips: np.ndarray):
    """For a source with the taxa ``tips``: ``(first, last + 1)`` S' index below every S node, and the S' order as
    indices into ``tips``."""
    lo, hi = se.leaf_ranges(parent, taxon)
    pos = se.s_positions(taxon, n_taxa)[tips]
    assert (pos >= 0).all()
    order = np.argsort(pos, kind="stable")
    mine = pos[order]
    return np.searchsorted(mine, lo), np.searchsorted(mine, hi, side="right"), order


def needs(parent: np.ndarray, taxon: np.ndarray, n_taxa: int, tips: np.ndarray) -> np.ndarray:
    """|z| + |pz| + 2 of every node z of S' (non-root clusters of two or more leaves of S restricted to ``tips``,
    each set once): the entries of its two difference arrays, by which ``k_tx_single`` picks its bin."""
    a, b, _ = restricted(parent, taxon, n_taxa, np.asarray(tips))
    size = np.maximum(b - a, 0)
    v = np.arange(1, len(parent))
    u = parent[1:]
    keep = (size[v] >= 2) & (size[v] != size[u])
    return np.sort(size[v[keep]] + size[u[keep]] + 2)


def branch_arrays(parent: np.ndarray, taxon: np.ndarray, arrays: TreeArrays, per_tree: bool = False):
    """``branch_triplet_reference.node_sum`` on arrays: the seven outputs as int64, or with ``per_tree`` the object
    array [trees][4][nodes] of ``resample_reference.per_tree``."""
    n_nodes, m_trees = len(parent), arrays.n_trees
    qb = quartet_branches(parent)
    out = {k: np.zeros(m_trees if k.startswith("n_") else n_nodes, dtype=np.int64) for k in BRANCH}
    each = np.zeros((m_trees, 4, n_nodes), dtype=object) if per_tree else None
    for t in range(m_trees):
        y, py, tips = clusters(*tree_slice(arrays, t))
        m = len(tips)
        if m < 3 or len(qb) == 0:  # (a tree without a cluster still counts its totals: every triple is a fan)
            continue
        a, b, order = restricted(parent, taxon, arrays.n_taxa, tips)
        size = b - a
        dec = np.flatnonzero((size[qb[:, 1]] > 0) & (size[qb[:, 2]] > 0) & (size[qb[:, 3]] > 0))

        def inside(v, a=a, b=b, order=order, m=m, y=y, py=py):
            ind = np.zeros(m + 1, dtype=np.int64)
            ind[order[a[v]:b[v]] + 1] = 1
            c = np.cumsum(ind)
            own = c[y[:, 1]] - c[y[:, 0]]
            return own, c[py[:, 1]] - c[py[:, 0]] - own

        for c_node, av, bv, dv in qb[dec]:
            (ia, oa), (ib, ob), (id_, od) = inside(av), inside(bv), inside(dv)
            vals = (int(size[av]) * int(size[bv]) * int(size[dv]), int((ia * ib * od).sum()),
                    int((ia * id_ * ob).sum()), int((ib * id_ * oa).sum()))
            for k, x in zip(BRANCH_NODE, vals):
                out[k][c_node] += x
            out["n_bt_total"][t] += vals[0]
            out["n_bt_concordant"][t] += vals[1]
            out["n_bt_alternative"][t] += vals[2] + vals[3]
            if per_tree:
                each[t, :, c_node] = vals
    return each if per_tree else out


def record_counts(parent: np.ndarray, taxon: np.ndarray, arrays: TreeArrays) -> np.ndarray:
    """The quartet branches every tree is decisive for: the records ``k_bt_records`` lists for it."""
    qb = quartet_branches(parent)
    out = np.zeros(arrays.n_trees, dtype=np.int64)
    for t in range(arrays.n_trees):
        _, tax = tree_slice(arrays, t)
        tips = tax[tax >= 0]
        if len(tips) >= 3 and len(qb):
            a, b, _ = restricted(parent, taxon, arrays.n_taxa, tips)
            size = b - a
            out[t] = int(((size[qb[:, 1]] > 0) & (size[qb[:, 2]] > 0) & (size[qb[:, 3]] > 0)).sum())
    return out


def taxon_reference(parent: np.ndarray, taxon: np.ndarray, arrays: TreeArrays, brute: bool = False) -> dict:
    """``taxon_triplet_reference`` on a case's arrays, indexed by taxon id (the supertree's tips must carry the ids
    0 .. tips - 1, as the export asks)."""
    res = (xr.brute_force if brute else xr.quadratic)(se.to_node(parent, taxon), se.source_nodes(arrays))
    tips = taxon[taxon >= 0]
    out = {}
    for k in TAXON:
        out[k] = np.zeros(len(tips), dtype=np.int64)
        out[k][tips] = res[k]
    return out


# ------------------------------------------------------------------------------------------------ closed forms
def weighted_after(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """``out[i] = sum of w[j] over j > i with a[j] > a[i]`` for distinct ``a``: the merge of ``se.dominance`` with
    weights, read from the left block's side (O(m log^2 m))."""
    m = len(a)
    size = 1
    while size < m:
        size *= 2
    rank = np.empty(m, dtype=np.int64)
    rank[np.argsort(a, kind="stable")] = np.arange(m)
    val = np.concatenate([rank, np.arange(m, size)]).astype(np.int64)
    wt = np.concatenate([np.asarray(w, dtype=np.int64), np.zeros(size - m, dtype=np.int64)])  # (the padding weighs 0)
    idx = np.arange(size)
    out = np.zeros(size, dtype=np.int64)
    w_ = 1
    while w_ < size:
        v, ix, ww = val.reshape(-1, 2, w_), idx.reshape(-1, 2, w_), wt.reshape(-1, 2, w_)
        nb = v.shape[0]
        base = (np.arange(nb, dtype=np.int64) * size)[:, None]
        right = (v[:, 1, :] + base).ravel()
        cw = np.concatenate([[0], np.cumsum(ww[:, 1, :].ravel())])
        below = np.searchsorted(right, (v[:, 0, :] + base).ravel())
        end = np.repeat((np.arange(nb) + 1) * w_, w_)
        out[ix[:, 0, :].ravel()] += cw[end] - cw[below]
        both = v.reshape(nb, 2 * w_)
        o = np.argsort(both, axis=1, kind="stable")
        val = np.take_along_axis(both, o, 1).ravel()
        idx = np.take_along_axis(ix.reshape(nb, 2 * w_), o, 1).ravel()
        wt = np.take_along_axis(ww.reshape(nb, 2 * w_), o, 1).ravel()
        w_ *= 2
    return out[:m]


def _t_positions(s_order, t_order, n_taxa: int) -> np.ndarray:
    s_order, t_order = np.asarray(s_order, dtype=np.int64), np.asarray(t_order, dtype=np.int64)
    t_pos = np.full(n_taxa, -1, dtype=np.int64)
    t_pos[t_order] = np.arange(len(t_order))
    a = t_pos[s_order]
    assert len(s_order) == len(t_order) >= 3 and (a >= 0).all()
    return a


def comb_branches(s_order, t_order, n_taxa: int) -> dict:
    """S = ``supertree("caterpillar", s_order)`` against the one source ``("caterpillar", t_order)`` on the same m
    taxa.  S's inner node i (1 <= i <= m - 2) is a quartet branch with A = the S positions below k = m - 1 - i,
    B = {k}, D = {k + 1}; T resolves every triple with the member latest in T as the outgroup.  With a[p] the T
    position of S position p and dom as in ``se.dominance``: D is last of (b, d) iff a[k + 1] > a[k], and then
    concordant = #{p < k : a[p] < a[k + 1]} = dom[k + 1] - 1 and alt1 = 0; else concordant = 0 and
    alt1 = #{p < k : a[p] < a[k]} = dom[k]; alt2 = the rest of the k triples (a is last)."""
    a = _t_positions(s_order, t_order, n_taxa)
    m = len(a)
    dom = se.dominance(a)
    k = np.arange(1, m - 1)
    d_last = a[k + 1] > a[k]
    con = np.where(d_last, dom[k + 1] - 1, 0)
    alt1 = np.where(d_last, 0, dom[k])
    alt2 = k - con - alt1
    out = {key: np.zeros(2 * m - 1, dtype=np.int64) for key in BRANCH_NODE}
    node = m - 1 - k
    out["bt_total"][node], out["bt_concordant"][node], out["bt_alt1"][node], out["bt_alt2"][node] = k, con, alt1, alt2
    one = lambda x: np.asarray([int(x)], dtype=np.int64)  # noqa: E731
    out.update(n_bt_total=one(k.sum()), n_bt_concordant=one(con.sum()), n_bt_alternative=one(alt1.sum() + alt2.sum()))
    return out


def comb_taxa(s_order, t_order, n_taxa: int) -> dict:
    """The same pair for the taxon export, per taxon id: every triple is resolved by both, so ``tx_super = tx_source =
    tx_total = C(m - 1, 2)``; a triple is shared iff one taxon c is last in both orders, which gives its outgroup
    C(dom(c), 2) and each x before c in both orders dom(c) - 1 (the choices of the third taxon)."""
    a = _t_positions(s_order, t_order, n_taxa)
    m = len(a)
    dom = se.dominance(a)
    shared = dom * (dom - 1) // 2 + weighted_after(a, dom - 1)
    out = {k: np.zeros(n_taxa, dtype=np.int64) for k in TAXON}
    ids = np.asarray(s_order, dtype=np.int64)
    out["tx_trees"][ids] = 1
    for k in ("tx_total", "tx_super", "tx_source"):
        out[k][ids] = (m - 1) * (m - 2) // 2
    out["tx_shared"][ids] = shared
    return out


def three_leaf(s_order, trees, n_taxa: int) -> dict:
    """``se.three_leaf_closed_form`` extended: a three-leaf source is decisive for at most one branch, with one triple
    (the concordance counts are the branch counts), and gives each of its taxa one tree, one triple, one resolved
    triple each way and one shared triple iff its cherry is S's."""
    base = se.three_leaf_closed_form(s_order, trees, n_taxa)
    out = {"n_bt_total": base["n_decisive"], "n_bt_concordant": base["n_concordant"],
           "n_bt_alternative": base["n_alternative"], "bt_total": base["decisive"],
           "bt_concordant": base["concordant"], "bt_alt1": base["alt1"], "bt_alt2": base["alt2"]}
    ids = np.asarray([o for _, o in trees], dtype=np.int64).reshape(len(trees), 3)
    ones = np.ones(ids.size, dtype=np.int64)
    for k in ("tx_trees", "tx_total", "tx_super", "tx_source"):
        out[k] = np.zeros(n_taxa, dtype=np.int64)
        np.add.at(out[k], ids.ravel(), ones)
    out["tx_shared"] = np.zeros(n_taxa, dtype=np.int64)
    np.add.at(out["tx_shared"], ids.ravel(), np.repeat(base["t_shared"], 3))
    # per tree: its one branch (-1: none) and the four counters it adds there (total, concordant, alt1, alt2)
    s_pos = np.full(n_taxa, -1, dtype=np.int64)
    s_pos[np.asarray(s_order, dtype=np.int64)] = np.arange(len(s_order))
    pos = s_pos[ids]
    out_of = np.where(np.asarray([k == "caterpillar" for k, _ in trees]), pos[:, 2], pos[:, 0])
    p = np.sort(pos, axis=1)
    dec = p[:, 2] == p[:, 1] + 1
    out["tree_node"] = np.where(dec, len(s_order) - p[:, 2], -1)
    out["tree_counts"] = np.stack([dec, dec & (out_of == p[:, 2]), dec & (out_of == p[:, 1]),
                                   dec & (out_of == p[:, 0])], 1).astype(np.int64)
    return out


def three_leaf_rows(closed: dict, weights, n_nodes: int) -> np.ndarray:
    """[4][R][nodes] int64: the rows of ``weights`` (R x trees, small) over three-leaf sources, from ``three_leaf``."""
    w = np.asarray(weights, dtype=np.int64)
    node, counts = closed["tree_node"], closed["tree_counts"]
    on = node >= 0
    out = np.zeros((4, len(w), n_nodes), dtype=np.int64)
    for x in range(4):
        for r in range(len(w)):
            np.add.at(out[x, r], node[on], w[r, on] * counts[on, x])
    return out


def weighted_rows(weights, each: np.ndarray) -> np.ndarray:
    """``resample_reference.rows`` in int64 for weights and counts whose products provably fit (asserted)."""
    w = np.asarray(weights, dtype=np.int64)
    c = np.asarray(each, dtype=np.int64)
    assert float(np.abs(w).sum(axis=1).max()) * float(c.max(initial=0)) < 2.0 ** 62
    return np.einsum("rt,txu->xru", w, c)


def wins(all_rows: np.ndarray) -> np.ndarray:
    """``resample_reference.wins`` in numpy, for integer arrays of any width (object arrays included)."""
    tot, con, a1, a2 = (all_rows[x][1:] for x in range(4))
    gt = lambda p, q: np.asarray(p > q, dtype=bool)  # noqa: E731 (object arrays compare to object arrays)
    live = gt(tot, 0)
    w0, w1, w2 = gt(con, a1) & gt(con, a2), gt(a1, con) & gt(a1, a2), gt(a2, con) & gt(a2, a1)
    tie = ~(w0 | w1 | w2)
    return np.stack([(live & x).sum(axis=0) for x in (w0, w1, w2, tie)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the cases
_ids = se._ids
_tree = se._tree


def rich_supertree(order, seed: int, polytomy: float = 0.08, unary: float = 0.04):
    """A ``mixed`` supertree that is binary nearly everywhere: most inner nodes are quartet branches."""
    par, leaf = se.mixed_shape(len(order), np.random.RandomState(seed), polytomy=polytomy, unary=unary)
    taxon = np.full(len(par), -1, dtype=np.int32)
    taxon[leaf] = np.asarray(order, dtype=np.int32)
    return par, taxon


def wave_case(end: int) -> se.Case:
    """The forest of ``se.wave_case`` against a binary-rich supertree whose tips carry 0 .. tips - 1 (the taxon
    export's rule): 11 of them are in no source."""
    base = se.wave_case(end)
    rng = np.random.RandomState(end + 5)
    parent, taxon = rich_supertree(rng.permutation(se.WAVE_TAXA + 11), seed=end + 7)
    m = base.arrays.n_trees
    arrays = TreeArrays(n_taxa=se.WAVE_TAXA + 11, node_off=base.arrays.node_off, parent=base.arrays.parent,
                        taxon=base.arrays.taxon, length=base.arrays.length, support=base.arrays.support,
                        weights=base.arrays.weights, taxa=se.names(se.WAVE_TAXA + 11))
    return se.Case(f"bt_wave_end_{end}", parent, taxon, arrays, batches=(0, 1, 2, m - 1, m))


# ---- the last workgroup of a tree: nz = min(zb, rcnt - j0).  A caterpillar source on the first n taxa of a
# caterpillar S is decisive for n - 2 branches (S positions k, k + 1 both present and one before them).
LAST_RECORDS = (1, 7, 8, 9, 15, 16, 17)


def last_workgroup_case() -> se.Case:
    rng = np.random.RandomState(12)
    n_taxa = max(LAST_RECORDS) + 2
    trees = [("caterpillar" if i % 2 else "random", _ids(r + 2)[rng.permutation(r + 2)])
             for i, r in enumerate(LAST_RECORDS)]
    parent, taxon = se.supertree("caterpillar", _ids(n_taxa))
    return se.Case("bt_last_workgroup", parent, taxon, br.forest(12, n_taxa, trees), batches=(0, 1, 3))


# ---- 64 words a step of the rows' scan (W > 64 from 2 048 leaves), 1 024 entries a round of tx_scan
WORD_SIZES = (2047, 2048, 2049, 4095, 4096, 4097)
ROUND_SIZES = (1023, 1024, 1025)


def words_case(size: int) -> se.Case:
    """One random binary tree of ``size`` leaves and a three-leaf tree against a mixed supertree on size + 2 taxa."""
    rng = np.random.RandomState(size + 30)
    n = size + 2
    trees = [_tree(rng, "random", _ids(n), size), _tree(rng, "balanced", _ids(n), 3)]
    parent, taxon = se.supertree("mixed", rng.permutation(n), seed=size + 30)
    return se.Case(f"bt_words_{size}", parent, taxon, br.forest(size, n, trees))


# ---- zb of k_bt_pairs: W = (n >> 5) + 1 words, zb = min(8, 40 960 / (24 W))
BT_ZB_STEPS = (6816, 7776, 9088, 10912, 13632, 18176, 27296)  # the first size with zb = 7, 6, ..., 1
BT_ZB_87 = (6815, 6816)
BT_ZB_21 = (27295, 27296)
BT_SMALL = (2, 3, 33, 64)
BT_LDS = (87359, 87360, BT_CAP)  # dynamic LDS below and from 64 KiB on, and the limit


def comb_case(size: int, kind: str, with_small: bool = False, second: int = 0) -> se.Case:
    """A caterpillar supertree in the identity order against a caterpillar source in the order
    ``se.permutation(kind, size)``: alone, between the trees of BT_SMALL, or before a second caterpillar of ``second``
    leaves (the first ``second`` taxa, permuted)."""
    rng = np.random.RandomState(size + 1)
    t_order = se.permutation(kind, size, seed=size)
    kinds = ("random", "caterpillar", "balanced", "star")
    small = [_tree(rng, kinds[i], _ids(size), k) for i, k in enumerate(BT_SMALL)] if with_small else []
    trees = small[:2] + [("caterpillar", t_order)] + small[2:]
    note = {"large": [(len(small[:2]), _ids(size), t_order)]}
    if second:
        o2 = se.permutation("random", second, seed=second + 3)
        trees.append(("caterpillar", o2))
        note["large"].append((len(trees) - 1, _ids(second), o2))
    parent, taxon = se.supertree("caterpillar", _ids(size))
    name = f"bt_comb_{size}_{kind}{'_batch' if with_small else ''}{f'_and_{second}' if second else ''}"
    return se.Case(name, parent, taxon, br.forest(size, size, trees, unit_weights=True), note=note)


def comb_case_reference(case: se.Case, which: str) -> dict:
    """Closed forms for the caterpillars of ``case`` (``which``: "branch" or "taxon"), the references for the small
    trees around them."""
    n_taxa, m = case.arrays.n_taxa, case.arrays.n_trees
    large = case.note["large"]
    at = [i for i, _, _ in large]
    rest = [t for t in range(m) if t not in at]
    if which == "taxon":
        out = {k: np.zeros(n_taxa, dtype=np.int64) for k in TAXON}
        for _, s_sub, t_order in large:
            # (a source on the first k taxa of the identity caterpillar: S restricted to it is the caterpillar on them)
            one = comb_taxa(s_sub, t_order, n_taxa)
            for k in TAXON:
                out[k] += one[k]
        if rest:
            small = taxon_reference(case.parent, case.taxon, se.subset(case.arrays, rest))
            for k in TAXON:
                out[k] += small[k]
        return out
    out = {k: np.zeros(m if k.startswith("n_") else len(case.parent), dtype=np.int64) for k in BRANCH}
    size = case.s_leaves
    for i, s_sub, t_order in large:
        one = comb_branches(s_sub, t_order, n_taxa)
        k = len(s_sub)
        for key in BRANCH_NODE:  # inner node j of the caterpillar on k leaves is node j + (size - k) of S
            out[key][size - k + 1:size - 1] += one[key][1:k - 1]
        for key in BRANCH[:3]:
            out[key][i] = one[key][0]
    if rest:
        small = branch_arrays(case.parent, case.taxon, se.subset(case.arrays, rest))
        for key in BRANCH_NODE:
            out[key] += small[key]
        for key in BRANCH[:3]:
            out[key][rest] = small[key]
    return out


def blocks_supertree(n: int, depth: int, seed: int):
    """A balanced binary top of ``depth`` levels whose 2^depth tips are polytomies of about n / 2^depth leaves each:
    binary at 2^depth - 2 places, each with large A, B and D."""
    rng = np.random.RandomState(seed)
    parent, taxon = [], []
    order = rng.permutation(n).astype(np.int32)
    stack = [(0, n, -1, depth)]
    while stack:
        lo, hi, p, d = stack.pop()
        at = len(parent)
        parent.append(p)
        taxon.append(-1)
        if d == 0:
            for x in order[lo:hi]:
                parent.append(at)
                taxon.append(int(x))
            continue
        mid = (lo + hi) // 2 + int(rng.randint(-3, 4))
        stack.append((mid, hi, at, d - 1))
        stack.append((lo, mid, at, d - 1))
    return np.asarray(parent, dtype=np.int32), np.asarray(taxon, dtype=np.int32)


def zb_blocks_case(size: int) -> se.Case:
    """A random binary tree of ``size`` leaves between the trees of BT_SMALL against ``blocks_supertree`` (30 quartet
    branches, A', B', D' of a few hundred leaves and more)."""
    rng = np.random.RandomState(size + 2)
    kinds = ("random", "caterpillar", "balanced", "star")
    small = [_tree(rng, kinds[i], _ids(size), k) for i, k in enumerate(BT_SMALL)]
    trees = small[:2] + [_tree(rng, "random", _ids(size), size)] + small[2:]
    parent, taxon = blocks_supertree(size, 5, size)
    return se.Case(f"bt_zb_blocks_{size}", parent, taxon, br.forest(size, size, trees), note={"large": 2})


# ---- bins of k_tx_pairs.  A chain supertree: the clusters are prefixes of the leaf order, of every size from 2 to n
# but the skipped ones -- a caterpillar with polytomy steps.  A node of s leaves below one of s + 1 needs 2 s + 3
# entries (odd), below one of s + 2 (size s + 1 skipped) 2 s + 4 (even).
def chain_supertree(blocks):
    """``blocks``: ``(taxa in leaf order, skipped sizes)`` each; one chain per block under a common root (the root is
    the chain's own when there is one block)."""
    parent, taxon = [], []
    if len(blocks) > 1:
        parent.append(-1)
        taxon.append(-1)
    for order, skips in blocks:
        n = len(order)
        sizes = [s for s in range(n, 1, -1) if s not in skips or s == n]
        at = len(parent)
        up = 0 if len(blocks) > 1 else -1
        tips = []  # (parent node, leaf position), deepest first
        for i, s in enumerate(sizes):
            parent.append(up)
            taxon.append(-1)
            nxt = sizes[i + 1] if i + 1 < len(sizes) else 0
            tips.append((at + i, range(nxt, s)))
            up = at + i
        for node, rng_ in reversed(tips):
            for p in rng_:
                parent.append(node)
                taxon.append(int(order[p]))
    return np.asarray(parent, dtype=np.int32), np.asarray(taxon, dtype=np.int32)


def skip_for(need: int) -> int | None:
    """The size to skip so that a chain holds a node that needs ``need`` entries (None: odd, a caterpillar step)."""
    return None if need % 2 else (need - 4) // 2 + 1


BIN_SIZES = (159, 1632)


def bin_case(n: int, extra_needs=()) -> se.Case:
    """Three random binary trees of ``n`` leaves on three disjoint blocks of taxa, against three chains whose nodes
    need dcap - 1, dcap and dcap + 1 entries (one chain each) for every bin the plan uses at n leaves; ``extra_needs``
    go to the middle chain."""
    plan = tx_plan_of((n >> 5) + 1)
    rng = np.random.RandomState(n)
    blocks, targets = [], []
    for j, d in enumerate((-1, 0, 1)):
        want = [c + d for c in plan["dcap"] if c and c + d <= 2 * n + 1] + (list(extra_needs) if d == 0 else [])
        skips = {skip_for(x) for x in want} - {None}
        blocks.append((_ids(3 * n)[j * n:(j + 1) * n][rng.permutation(n)], skips))
        targets.append(want)
    parent, taxon = chain_supertree(blocks)
    trees = [("random", order[rng.permutation(n)]) for order, _ in blocks]
    return se.Case(f"tx_bins_{n}", parent, taxon, br.forest(n, 3 * n, trees), batches=(0, 1), note={"targets": targets})


# ---- bin 0's zb: 8 S' nodes a workgroup while 2 x 8 rows fit the growing budget of bin 0
TX_ZB_87 = (3071, 3072)
TX_ZB_21 = (26623, 26624)
TX_SLAB_BEGINS = (9924, 9925, 9926)
TX_SLAB_LDS = (131071, 131072)


def tx_zb_case(size: int) -> se.Case:
    rng = np.random.RandomState(size + 4)
    trees = [_tree(rng, "random", _ids(size), size), _tree(rng, "caterpillar", _ids(size), 40)]
    par, leaf = se.mixed_shape(size, np.random.RandomState(size + 5), polytomy=0.6, unary=0.02)
    taxon = np.full(len(par), -1, dtype=np.int32)
    taxon[leaf] = rng.permutation(size)
    return se.Case(f"tx_zb_{size}", par, taxon, br.forest(size, size, trees))


def twin_case(n: int) -> se.Case:
    """A random binary supertree of ``n`` leaves against the same topology with the children of every node in the
    other order with probability 1/2 (the twin trees of ``test_gpu_taxon_triplets.py``, built as arrays): every triple
    is shared, so all four sums are C(n - 1, 2) at every leaf."""
    rng = np.random.RandomState(n)
    par, leaf = br.shape("random", n, rng)
    taxon = np.full(len(par), -1, dtype=np.int32)
    taxon[leaf] = rng.permutation(n)
    idx = np.arange(1, len(par))
    later = idx != par[1:] + 1  # (a binary node's first child follows it in preorder)
    second = np.zeros(len(par), dtype=np.int64)
    second[par[1:][later]] = idx[later]
    flip = rng.rand(len(par)) < 0.5
    t_par, t_tax, stack = [], [], [(0, -1)]
    while stack:
        v, p = stack.pop()
        at = len(t_par)
        t_par.append(p)
        t_tax.append(int(taxon[v]))
        if not leaf[v]:
            a, b = (int(second[v]), v + 1) if flip[v] else (v + 1, int(second[v]))
            stack.append((b, at))
            stack.append((a, at))
    t_tax = np.asarray(t_tax, dtype=np.int32)
    length = np.ones(len(par))
    length[0] = np.nan
    arrays = TreeArrays(n_taxa=n, node_off=np.asarray([0, len(par)], dtype=np.int64),
                        parent=np.asarray(t_par, dtype=np.int32), taxon=t_tax, length=length,
                        support=np.where(t_tax < 0, 100.0, np.nan), weights=np.ones(1), taxa=se.names(n))
    return se.Case(f"tx_twin_{n}", par, taxon, arrays)


def twin_reference(n: int) -> dict:
    each = (n - 1) * (n - 2) // 2
    return {k: np.full(n, 1 if k == "tx_trees" else each, dtype=np.int64) for k in TAXON}


# ---- single-node workgroups whose arrays total 1 023 ... 1 025 and 2 047 ... 2 049 entries
ROUND_TOTALS = (1023, 1024, 1025, 2047, 2048, 2049)
ROUND_CHAIN = 1030  # a chain of 1 030 leaves holds needs up to 2 061
ROUND_LDS_LEAVES = 11008  # W = 345: the smallest rows with which one node's 2 049 entries fit a capped bin of zb = 1
ROUND_BIN2_LEAVES = 20416  # W = 639: bin 0 holds 2 046 entries (zb = 2), bin 1 is out: 2 047 on go to bin 2 (zb = 1)
ROUND_BIN0_LEAVES = 26624  # W = 833: bin 0 itself has zb = 1 and holds 4 982 entries
ROUND_WHERE = ("slab", "lds", "bin2", "bin0")


def round_case(where: str) -> tuple[se.Case, int]:
    """``(case, lds_bytes)``.  Two chains of ROUND_CHAIN leaves: a caterpillar (every odd total) and one with the
    steps that give 1 024 and 2 048 (no chain holds three totals in a row: they are sums of neighbours in one
    increasing sequence).  ``slab``: one tree per chain, ``lds_bytes`` = 100 (no bin: every node takes the slab, one
    at a time).  The others: one tree against both chains under a root that holds the other leaves -- ``lds``:
    ROUND_LDS_LEAVES leaves with the cap that leaves bin 0 one node a workgroup and room for 2 049 entries; ``bin2``
    and ``bin0``: no cap, at the sizes where the plan by itself gives the totals from 2 047 on (bin 2) and all six
    (bin 0) a workgroup of one node."""
    skips = {skip_for(x) for x in ROUND_TOTALS} - {None}
    rng = np.random.RandomState(len(where))
    n = {"slab": 2 * ROUND_CHAIN, "lds": ROUND_LDS_LEAVES, "bin2": ROUND_BIN2_LEAVES, "bin0": ROUND_BIN0_LEAVES}[where]
    order = rng.permutation(n).astype(np.int32)
    blocks = [(order[:ROUND_CHAIN], set()), (order[ROUND_CHAIN:2 * ROUND_CHAIN], skips)]
    parent, taxon = chain_supertree(blocks)
    if where == "slab":
        trees = [("random", b[rng.permutation(ROUND_CHAIN)]) for b, _ in blocks]
        return se.Case("tx_round_slab", parent, taxon, br.forest(1, n, trees)), 100
    parent = np.concatenate([parent, np.zeros(n - 2 * ROUND_CHAIN, dtype=np.int32)]).astype(np.int32)
    taxon = np.concatenate([taxon, order[2 * ROUND_CHAIN:]]).astype(np.int32)
    rowb = 16 * ((n >> 5) + 1)
    return (se.Case(f"tx_round_{where}", parent, taxon, br.forest(2, n, [_tree(rng, "random", _ids(n), n)])),
            4 * rowb - 1 if where == "lds" else 0)


# ---- the slab's round robin: lds_bytes = 100 leaves no bin, every S' node takes the slab; a random tree of n leaves
# on a caterpillar S has n - 2 such nodes
ROBIN_NODES = {"below": (128, 88, 39), "at": (128, 88, 40), "above": (128, 88, 41), "thrice": (300, 2, 270, 130)}


def robin_case(which: str) -> se.Case:
    rng = np.random.RandomState(len(which))
    n_taxa = 320
    trees = [_tree(rng, "random", _ids(n_taxa), k + 2) for k in ROBIN_NODES[which]]
    trees.insert(1, _tree(rng, "balanced", _ids(n_taxa), 2))  # (a tree without a node between two with many)
    parent, taxon = se.supertree("caterpillar", rng.permutation(n_taxa))
    return se.Case(f"tx_robin_{which}", parent, taxon, br.forest(5, n_taxa, trees))


# ---- more trees than a weight chunk of k_rs_reduce
RS_TREES = (511, 512, 513, 1025)
RS_REPS = (9, 17)
RS_TAXA = 150


@lru_cache(maxsize=None)
def chunk_forest():
    """``(parent, taxon, arrays of 1 025 trees of 3 .. 12 leaves, C [trees][4][nodes] int64)``; a count of fewer
    trees takes the first of them."""
    rng = np.random.RandomState(26)
    kinds = ("random", "caterpillar", "balanced", "random")
    trees = [_tree(rng, kinds[i % 4], _ids(RS_TAXA), int(rng.randint(3, 13))) for i in range(max(RS_TREES))]
    parent, taxon = rich_supertree(rng.permutation(RS_TAXA), seed=26, polytomy=0.05, unary=0.03)
    arrays = br.forest(26, RS_TAXA, trees)
    each = branch_arrays(parent, taxon, arrays, per_tree=True).astype(np.int64)
    return parent, taxon, arrays, each


def chunk_weights(n_rep: int, n_trees: int) -> np.ndarray:
    """Small weights with zeros; from tree RS_CHUNK on every weight is 1 000 more than anything before it, so that a
    tree read with a weight of the first chunk changes the sums."""
    rng = np.random.RandomState(n_rep * 7 + n_trees)
    w = rng.randint(0, 4, size=(n_rep, n_trees)).astype(np.int64)
    w[0] = rng.randint(1, 4, size=n_trees)
    w[:, RS_CHUNK:] += 1000 + np.arange(n_rep)[:, None]
    return w


# ---- counts from 2^32 on: the high word of a slab entry
BIG_BLOCK = 1634


def big_case() -> se.Case:
    """A supertree ((A, B), D) of three polytomies of BIG_BLOCK leaves against one caterpillar source that lists A, B,
    D in turn with every block shuffled and a few taxa moved: |A||B||D| = 4.36 x 10^9 triples, nearly all
    concordant."""
    n = 3 * BIG_BLOCK
    rng = np.random.RandomState(32)
    parent = [-1, 0, 1] + [2] * BIG_BLOCK + [1] + [3 + BIG_BLOCK] * BIG_BLOCK + [0] + [4 + 2 * BIG_BLOCK] * BIG_BLOCK
    ids = rng.permutation(n).astype(np.int32)
    blocks = [ids[i * BIG_BLOCK:(i + 1) * BIG_BLOCK] for i in range(3)]
    taxon = np.concatenate([[-1, -1, -1], blocks[0], [-1], blocks[1], [-1], blocks[2]]).astype(np.int32)
    t_order = np.concatenate([b[rng.permutation(BIG_BLOCK)] for b in blocks])
    for _ in range(40):  # (a few alt1 and alt2 triples)
        i, j = rng.randint(0, n, size=2)
        t_order[i], t_order[j] = t_order[j], t_order[i]
    return se.Case("rs_big", np.asarray(parent, dtype=np.int32), taxon, br.forest(32, n, [("caterpillar", t_order)]))


def big_weights(n_leaves: int) -> list[int]:
    """0, 1, 2^30 + 12 345 and the largest weight the export's own check admits for one tree of ``n_leaves``
    (weight x floor(leaves^3 / 27) <= 2^63 - 1, and int32)."""
    return [0, 1, (1 << 30) + 12345, min((1 << 31) - 1, ((1 << 63) - 1) // (n_leaves ** 3 // 27))]


# ---- the byte budget
def budget_first_split(export: str) -> int:
    """M*: the smallest count of three-leaf trees the plan splits in two batches (S of ``se.BUDGET_LEAVES`` leaves)."""
    row_stride = br.round_up(se.BUDGET_LEAVES, se.SC_ROW_ALIGN)
    epl, ept = export_extras(export, 2 * se.BUDGET_LEAVES - 1)
    return se.SC_BUDGET // se.per_tree(3, row_stride, se.levels_of(3), epl, ept) + 1

