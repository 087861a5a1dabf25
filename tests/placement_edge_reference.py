"""Builders, array references and the host plans for the edges of the exports built on ``k_pl_*``, ``k_cp_*`` and
``k_py_*`` (``csrc/scs_score.hip``: ``scs_score_placements``, ``scs_score_clade_placements`` /
``scs_score_clade_moves``, ``scs_score_polytomies``; the cases of ``tests/test_gpu_placement_polytomy_edges.py``, held to
their numbers by ``tests/test_placement_edge_reference_cpu.py``).  CPU only; beside ``score_edge_reference`` and
``branch_edge_reference``, whose builders it reuses.

The references stay the project's own where they can go -- ``placement_reference.brute_force`` / ``recurrence``,
``clade_placement_reference.brute_force`` / ``composed``, ``polytomy_reference.brute_force`` / ``node_sum``,
``refine_reference.top_k``.  What is here:

* ``placement_arrays``: section 22's recurrence on integer arrays -- per (query, source) the groups of x off its root
  path in T as ranges of T's leaf order, one sorted vector of S positions per group, A and X for all nodes of S at
  once, the marks as a difference array over S's preorder -- for the sizes where the references' sets are too slow;
* ``polytomy_arrays``: ``polytomy_reference.node_sum`` with the colours as ranges of S's leaf order and one
  prefix-count vector over T's leaf order per colour;
* the plans of ``sc_plan_pairs`` under ``sc_pl_rule``, of ``sc_pl_lds`` and of ``sc_py_plan_of`` restated
  (``placement_plan``), compared with ``scs_debug_placement_plan``;
* the cases, each a function of its name.
"""

from __future__ import annotations

from functools import lru_cache

import branch_edge_reference as be
import build_reference as br
import numpy as np
import score_edge_reference as se

from spectralclustersupertree_amd.treearrays import TreeArrays

# ---- the constants of csrc/scs_score.hip the cases are placed by
PL_QMAX = 64  # query taxa per pass of scs_score_placements
CP_QMAX = 64  # sub-queries (tips of query clades) per pass of the clade exports
PY_KMAX = 64  # children of a polytomy at most: one lane each
PY_GRID_Y = 65535  # trees per launch of k_py_sweep
PL_CAP = se.LDS_CAP  # 327 679: the largest source tree of the placement and clade exports

PLACEMENTS = ("pl_trees", "pl_total", "pl_source", "pl_super", "pl_shared")
CLADES = ("cp_trees", "cp_total", "cp_source", "cp_super", "cp_shared")
POLYTOMIES = ("py_degree", "py_trees", "py_total", "py_joint")
C_NAME = {"score_placements": "scs_score_placements", "score_clade_placements": "scs_score_clade_placements",
          "score_clade_moves": "scs_score_clade_moves", "score_polytomies": "scs_score_polytomies"}


# ------------------------------------------------------------------------------------------------ the host plans
def lds_cap(lds_bytes: int = 0) -> int:
    """``sc_lds_cap``."""
    return min(lds_bytes, se.TP_LDS_MAX) if lds_bytes > 0 else se.TP_LDS_MAX


def node_bytes(qc: int) -> int:
    """``sc_pl_node_bytes``: the LDS sums of one S' node beside its rows."""
    return 16 * qc + 32


def pass_bytes(qc: int) -> int:
    """``sc_pl_pass_bytes``: ``pref`` and its pad."""
    return 4 * ((qc + 4) & ~3)


def pair_plan(n_max: int, qcap: int, cap: int = se.TP_LDS_MAX) -> tuple[int, int, int]:
    """``(words, zb, sums)`` of ``sc_plan_pairs`` under ``sc_pl_rule(qcap, cap)`` for a batch whose largest tree has
    ``n_max`` leaves."""
    words = (n_max >> 5) + 1
    rowb = 16 * words
    zb = min(se.TP_ZMAX, max(1, se.TP_LDS_BUDGET // rowb))
    while zb > 1 and zb * (rowb + node_bytes(qcap)) + pass_bytes(qcap) > cap:
        zb -= 1
    return words, zb, int(zb * (rowb + node_bytes(qcap)) + pass_bytes(qcap) <= cap)


def pair_lds(words: int, zb: int, sums: int, qc: int) -> int:
    """``sc_pl_lds``: the launch bytes of ``k_pl_pairs`` / ``k_cp_pairs`` for a pass of ``qc`` queries."""
    return zb * 16 * words + (zb * node_bytes(qc) + pass_bytes(qc) if sums else 0)


def py_plan(n_max: int, k: int, cap: int = se.TP_LDS_MAX) -> tuple[int, int, int, int]:
    """``(W, Ws, acc_lds, launch bytes)`` of ``sc_py_plan_of`` for a batch whose largest tree has ``n_max`` leaves."""
    w = max((n_max + 31) >> 5, 1)
    accb, odd = 8 * k * k, w | 1
    acc_odd, acc_even = k * odd * 8 + accb <= cap, k * w * 8 + accb <= cap
    acc = int(acc_odd or acc_even)
    ws = odd if (acc_odd if acc else k * odd * 8 <= cap) else w
    return w, ws, acc, k * ws * 8 + (accb if acc else 0)


def export_extras(export: str, count: int = 1, degrees=()) -> tuple[int, int]:
    """``(extra_per_leaf, extra_per_tree)`` the export hands to ``sc_begin``: ``count`` query taxa (placements) or
    tips of all query clades (clades); the polytomies' ``degrees``."""
    if export == "score_placements":
        qcap = min(max(count, 1), PL_QMAX)
        return 16 * qcap + 64, 12 * qcap + 8
    if export in ("score_clade_placements", "score_clade_moves"):
        qcap = min(max(count, 1), CP_QMAX)
        return 25 * qcap + 64, 36 * qcap + 8
    assert export == "score_polytomies"
    return 16, 4 + 4 * (sum(int(k) + 1 for k in degrees) + len(degrees))


def placement_plan(tree_off, super_leaves: int, batch_trees: int = 0, lds_bytes: int = 0, n_queries: int = 1,
                   n_sub_queries: int = 1, degrees=()) -> dict:
    """What ``backend.debug_placement_plan`` returns, restated."""
    off = [int(x) for x in tree_off]
    sizes = [off[t + 1] - off[t] for t in range(len(off) - 1)]
    cap = lds_cap(lds_bytes)
    as64 = lambda x: np.asarray(x, dtype=np.int64)  # noqa: E731
    out = {}
    for name, export, count, qmax in (("pl", "score_placements", n_queries, PL_QMAX),
                                      ("cp", "score_clade_placements", n_sub_queries, CP_QMAX)):
        qcap = min(count, qmax)
        q_last = count - (count - 1) // qcap * qcap
        bstart = se.plan(off, super_leaves, batch_trees, *export_extras(export, count))["bstart"]
        rows = {k: [] for k in ("words", "zb", "sums", "lds_full", "lds_last", "workgroups")}
        blk = []
        for b in range(len(bstart) - 1):
            mine = sizes[bstart[b]:bstart[b + 1]]
            w, zb, sums = pair_plan(max(mine, default=0), qcap, cap)
            wgs = [(2 * n + zb - 1) // zb if n >= 3 else 0 for n in mine]
            blk += wgs
            for k, v in (("words", w), ("zb", zb), ("sums", sums), ("lds_full", pair_lds(w, zb, sums, qcap)),
                         ("lds_last", pair_lds(w, zb, sums, q_last)), ("workgroups", sum(wgs))):
                rows[k].append(v)
        out[f"{name}_bstart"] = bstart
        out[f"{name}_blk"] = as64(blk)
        out.update({f"{name}_{k}": as64(v) for k, v in rows.items()})
    bstart = se.plan(off, super_leaves, batch_trees, *export_extras("score_polytomies", 0, degrees))["bstart"]
    py = [[py_plan(max(sizes[bstart[b]:bstart[b + 1]], default=0), int(k), cap) for k in degrees]
          for b in range(len(bstart) - 1)]
    py = as64(py).reshape(len(bstart) - 1, len(degrees), 4)
    out.update(py_bstart=bstart, py_words=py[:, :, 0], py_stride=py[:, :, 1], py_acc_lds=py[:, :, 2], py_lds=py[:, :, 3])
    return out


def first_leaves(pred, lo: int = 3, hi: int = PL_CAP + 1) -> int:
    """The smallest n in (lo, hi] with ``pred(n)``, for a predicate that is false at ``lo`` and monotone."""
    assert not pred(lo) and pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


# ------------------------------------------------------------------------------------------------ trees as arrays
def preorder_tables(parent, taxon) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(lo, hi, end)`` of every node of a tree in preorder: its leaves are the positions [lo, hi) of the leaf
    order, its subtree the nodes [v, end)."""
    par = np.asarray(parent).tolist()
    tip = np.asarray(taxon) >= 0
    n = len(par)
    leaves, nodes = tip.astype(np.int64).tolist(), [1] * n
    for v in range(n - 1, 0, -1):
        p = par[v]
        leaves[p] += leaves[v]
        nodes[p] += nodes[v]
    lo = np.cumsum(tip) - tip
    return lo.astype(np.int64), lo + np.asarray(leaves, dtype=np.int64), np.arange(n) + np.asarray(nodes, dtype=np.int64)


def children(parent) -> tuple[np.ndarray, np.ndarray]:
    """``(start, kid)``: the children of node v, in preorder, are ``kid[start[v]:start[v + 1]]``."""
    par = np.asarray(parent, dtype=np.int64)
    kid = np.argsort(par[1:], kind="stable") + 1
    return np.searchsorted(par[kid], np.arange(len(par) + 1)), kid


def _inside(sorted_pos: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """How many of ``sorted_pos`` lie in [lo, hi), for every node."""
    return np.searchsorted(sorted_pos, hi) - np.searchsorted(sorted_pos, lo)


class _Super:
    """S as arrays, once per call: leaf ranges, preorder ends, S position per taxon."""

    def __init__(self, parent, taxon, n_taxa: int) -> None:
        self.par = np.asarray(parent, dtype=np.int64)
        self.n_nodes = len(self.par)
        self.lo, self.hi, self.end = preorder_tables(parent, taxon)
        self.pos = se.s_positions(np.asarray(taxon), max(int(n_taxa), int(np.max(taxon)) + 1))
        self.up = np.maximum(self.par, 0)

    def path_sums(self, root_value, a, x):
        """value(root) = root_value, value(v) = value(q) + (sum of a over q's children - a[q]) + x[v]: every node's
        term on its preorder range of a difference array, then one cumulative sum."""
        kids = np.zeros(self.n_nodes, dtype=np.int64)
        np.add.at(kids, self.par[1:], a[1:])
        term = (kids - a)[self.up] + x
        term[0] = root_value
        d = np.zeros(self.n_nodes + 1, dtype=np.int64)
        d[:self.n_nodes] += term
        np.add.at(d, self.end, -term)
        return np.cumsum(d)[:self.n_nodes]


class _Source:
    """One source tree as arrays: leaf ranges of its nodes, children, the S position of the leaf at every T position."""

    def __init__(self, arrays: TreeArrays, t: int, sup: _Super) -> None:
        self.par, self.tax = be.tree_slice(arrays, t)
        self.tips = self.tax[self.tax >= 0]
        self.m = len(self.tips)
        if self.m >= 3:
            self.lo, self.hi, _ = preorder_tables(self.par, self.tax)
            self.start, self.kid = children(self.par)
            self.spos = sup.pos[self.tips]
            assert (self.spos >= 0).all()


def _one_placement(sup: _Super, src: _Source, x: int, keep=None):
    """``(fans, shared row, super row)`` of the taxon ``x`` of ``src`` over the nodes of S, on the ground set of the
    T positions ``keep`` (default all) and x itself."""
    u = int(np.flatnonzero(src.tax == x)[0])
    mask = np.ones(src.m, dtype=bool) if keep is None else keep.copy()
    mask[int(src.lo[u])] = False
    n_of = _inside(np.sort(src.spos[mask]), sup.lo, sup.hi)
    levels = []  # per branching ancestor of x, deepest first: the sorted S positions of every group there
    while src.par[u] >= 0:
        p = int(src.par[u])
        groups = [np.sort(src.spos[src.lo[c]:src.hi[c]][mask[src.lo[c]:src.hi[c]]])
                  for c in src.kid[src.start[p]:src.start[p + 1]] if c != u]
        groups = [g for g in groups if len(g)]
        if groups:
            levels.append(groups)
        u = p
    up = sup.up
    below = np.zeros(sup.n_nodes, dtype=np.int64)
    a_sh = np.zeros(sup.n_nodes, dtype=np.int64)
    x_sh = np.zeros(sup.n_nodes, dtype=np.int64)
    fans = 0
    for groups in levels:
        counts = [_inside(g, sup.lo, sup.hi) for g in groups]
        for c in counts:
            below += c
        outside = (n_of[up] - below[up]) - (n_of - below)
        for c in counts:
            a_sh += c * (c - 1) // 2
            x_sh += c * outside
        g_sizes = [len(g) for g in groups]
        fans += (sum(g_sizes) ** 2 - sum(s * s for s in g_sizes)) // 2
    assert np.array_equal(below, n_of)
    a_su = n_of * (n_of - 1) // 2
    return fans, sup.path_sums(a_sh[0], a_sh, x_sh), sup.path_sums(a_su[0], a_su, n_of * (n_of[up] - n_of))


def placement_arrays(parent, taxon, arrays: TreeArrays, queries) -> dict:
    """The five outputs of ``scs_score_placements`` (int64; rows queries x nodes) from the definition of section 22.
    For a source T that holds the query x, the groups of x are the subtrees hanging off its root path; with
    c_g(z) the leaves of group g below the S node z, n(z) their sum and b_g(z) the sum over the groups that hang no
    higher than g, ``A(z) = sum_g C(c_g(z), 2)`` and ``X(v, q) = sum_g c_g(v) ((n(q) - b_g(q)) - (n(v) - b_g(v)))`` for
    a child v of q; then ``shared(root) = A(root)`` and
    ``shared(v) = shared(q) + [sum of A over the children of q - A(q)] + X(v, q)``.  The triples S_{x->v} resolves
    follow the same with one group of everything: ``C(n(z), 2)`` and ``n(v) (n(q) - n(v))``.  Every count of one tree
    is below m^2, asserted to sum within int64."""
    sup = _Super(parent, taxon, arrays.n_taxa)
    nq = len(queries)
    slot = {int(x): i for i, x in enumerate(queries)}
    assert len(slot) == nq
    sizes = np.asarray(arrays.leaf_counts(), dtype=np.int64)
    assert float((sizes.astype(np.float64) ** 2).sum()) < 2.0 ** 62
    out = {k: np.zeros(nq if k in PLACEMENTS[:3] else (nq, sup.n_nodes), dtype=np.int64) for k in PLACEMENTS}
    for t in range(arrays.n_trees):
        src = _Source(arrays, t, sup)
        m = src.m
        held = [int(x) for x in src.tips if int(x) in slot] if m >= 3 else []
        for x in held:
            i = slot[x]
            fans, shared, super_ = _one_placement(sup, src, x)
            out["pl_trees"][i] += 1
            out["pl_total"][i] += (m - 1) * (m - 2) // 2
            out["pl_source"][i] += (m - 1) * (m - 2) // 2 - fans
            out["pl_shared"][i] += shared
            out["pl_super"][i] += super_
    return out


def _joined_pairs(src: _Source, mask: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Per node y of T: the pairs of leaves of ``mask`` (over T positions) whose smallest common cluster is y, and
    the leaves of ``mask`` below y."""
    pre = np.concatenate([[0], np.cumsum(mask.astype(np.int64))])
    u = pre[src.hi] - pre[src.lo]
    f = u * (u - 1) // 2
    kids = np.zeros(len(f), dtype=np.int64)
    np.add.at(kids, np.asarray(src.par, dtype=np.int64)[1:], f[1:])
    return np.where(src.hi - src.lo >= 2, f - kids, 0), u


def _resolved(src: _Source, mask: np.ndarray) -> int:
    """The triples of the leaves ``mask`` that T resolves: a pair joined at y and a third leaf outside y."""
    joined, u = _joined_pairs(src, mask)
    return int((joined * (int(mask.sum()) - u)).sum())


def clade_arrays(parent, taxon, arrays: TreeArrays, query_nodes) -> dict:
    """The five outputs of ``scs_score_clade_placements`` (int64; rows clades x nodes), section 23 from its
    definition.  For a source T on L crossed by the clade Q (Q' = Q ∩ L, R = L - Q', both non-empty), a crossing triple
    has one taxon in Q' or two.  One taxon x: the triple is {x, a, b} with a, b in R, and what S_{Q->v} and T say
    about it is what the placement of x alone says on the ground set R ∪ {x}: ``_one_placement`` with the T positions
    of R, summed over the tips of Q'.  Two taxa x, y in Q' and r in R: S_{Q->v} says xy|r on every edge, C(|Q'|, 2) |R|
    triples; T agrees where r lies outside the smallest cluster of T that holds x and y.  ``cp_source``: the triples T
    resolves, less those inside Q' and those inside R; ``cp_total`` = C(m, 3) - C(|Q'|, 3) - C(|R|, 3)."""
    sup = _Super(parent, taxon, arrays.n_taxa)
    nq = len(query_nodes)
    sizes = np.asarray(arrays.leaf_counts(), dtype=np.int64)
    assert float((sizes.astype(np.float64) ** 3).sum()) < 2.0 ** 62
    out = {k: np.zeros(nq if k in CLADES[:3] else (nq, sup.n_nodes), dtype=np.int64) for k in CLADES}
    c3 = lambda n: n * (n - 1) * (n - 2) // 6  # noqa: E731
    for t in range(arrays.n_trees):
        src = _Source(arrays, t, sup)
        m = src.m
        if m < 3:
            continue
        everyone = np.ones(m, dtype=bool)
        whole = None
        for i, q in enumerate(query_nodes):
            in_q = (src.spos >= sup.lo[q]) & (src.spos < sup.hi[q])
            a = int(in_q.sum())
            if a == 0 or a == m:
                continue
            whole = _resolved(src, everyone) if whole is None else whole
            out["cp_trees"][i] += 1
            out["cp_total"][i] += c3(m) - c3(a) - c3(m - a)
            out["cp_source"][i] += whole - _resolved(src, in_q) - _resolved(src, ~in_q)
            joined, _ = _joined_pairs(src, in_q)
            _, r_below = _joined_pairs(src, ~in_q)
            out["cp_shared"][i] += int((joined * ((m - a) - r_below)).sum())
            out["cp_super"][i] += a * (a - 1) // 2 * (m - a)
            for x in src.tips[in_q]:
                _, shared, super_ = _one_placement(sup, src, int(x), ~in_q)
                out["cp_shared"][i] += shared
                out["cp_super"][i] += super_
    return out


def t_clusters(t_par, t_tax) -> tuple[np.ndarray, np.ndarray]:
    """T's distinct non-root clusters of two or more leaves and the smallest cluster strictly above each, as ranges
    [first, last + 1) of T's leaf order ([k, 2] each)."""
    lo, hi, _ = preorder_tables(t_par, t_tax)
    v = np.arange(1, len(t_par))
    u = np.asarray(t_par, dtype=np.int64)[1:]
    keep = (hi[v] - lo[v] >= 2) & ((lo[v] != lo[u]) | (hi[v] != hi[u]))  # (a unary node's child repeats its set)
    v, u = v[keep], u[keep]
    return np.stack([lo[v], hi[v]], 1), np.stack([lo[u], hi[u]], 1)


def polytomy_arrays(parent, taxon, arrays: TreeArrays, query_nodes) -> dict:
    """The outputs of ``scs_score_polytomies`` from ``polytomy_reference.node_sum``'s formula on arrays: colour i of
    a query node is the stretch [lo(c_i), lo(c_{i+1})) of S's leaf order; per source one prefix-count vector per
    colour over T's leaf order gives I(y, C_i') and I(py, C_i') of every cluster y at once.  int64; above 8 children
    the triple products are summed in float64, where every partial sum is an integer below 2^53 (asserted), so the
    sums are exact."""
    par = np.asarray(parent, dtype=np.int64)
    s_lo, s_hi, _ = preorder_tables(parent, taxon)
    s_pos = se.s_positions(np.asarray(taxon), max(int(arrays.n_taxa), int(np.max(taxon)) + 1))
    start, kid = children(par)
    bounds, keeps = [], []
    for q in query_nodes:
        kids = kid[start[q]:start[q + 1]]
        k = len(kids)
        assert 3 <= k <= PY_KMAX
        bounds.append(np.concatenate([s_lo[kids], [s_hi[q]]]))
        keep = np.zeros((k, k, k), dtype=bool)
        for i in range(k):
            for j in range(i + 1, k):  # the entries [i][j][l] the export fills: i < j, l not in {i, j}
                keep[i, j, :] = True
                keep[i, j, [i, j]] = False
        keeps.append(keep)
    ks = [len(b) - 1 for b in bounds]
    out = {"py_degree": np.asarray(ks, dtype=np.int32), "py_trees": np.zeros(len(ks), dtype=np.int64),
           "py_total": [np.zeros((k, k, k), dtype=np.int64) for k in ks],
           "py_joint": [np.zeros((k, k, k), dtype=np.int64) for k in ks]}
    for t in range(arrays.n_trees):
        t_par, t_tax = be.tree_slice(arrays, t)
        tips = t_tax[t_tax >= 0]
        m = len(tips)
        if m < 3:
            continue
        t_spos = s_pos[tips]
        y = py = None
        for q, (bnd, keep, k) in enumerate(zip(bounds, keeps, ks)):
            col = np.searchsorted(bnd, t_spos, side="right") - 1  # (k: past the node's last leaf)
            inside = (col >= 0) & (col < k)
            size = np.bincount(col[inside], minlength=k).astype(np.int64)
            if (size > 0).sum() < 3:
                continue
            if y is None:
                y, py = t_clusters(t_par, t_tax)
            out["py_trees"][q] += 1
            ind = np.zeros((k, m + 1), dtype=np.int64)
            ind[col[inside], np.flatnonzero(inside) + 1] = 1
            pre = np.cumsum(ind, axis=1)
            h = pre[:, y[:, 1]] - pre[:, y[:, 0]]  # [colour][cluster]: I(y, C')
            d = pre[:, py[:, 1]] - pre[:, py[:, 0]] - h  # I(py, C') - I(y, C')
            two = (h > 0).sum(axis=0) >= 2  # (every term has two colours inside y)
            h, d = h[:, two], d[:, two]
            if k <= 8:
                joint = np.einsum("iy,jy,ly->ijl", h, h, d)
            else:
                assert float(h.max(initial=0)) ** 2 * float(np.abs(d).sum(axis=1).max(initial=0)) < 2.0 ** 53
                hf, df = h.astype(np.float64), d.astype(np.float64).T
                joint = np.stack([np.rint((hf[i] * hf) @ df) for i in range(k)]).astype(np.int64)
            out["py_joint"][q] += np.where(keep, joint, 0)
            out["py_total"][q] += np.where(keep, size[:, None, None] * size[None, :, None] * size[None, None, :], 0)
    return out


def zcounts(parent, taxon, arrays: TreeArrays) -> np.ndarray:
    """The S' nodes ``k_pl_znodes`` lists per tree: its leaves and the distinct sets of two or more of them among
    S's nodes (the root's among them); 0 for a tree of fewer than three leaves."""
    s_lo, s_hi, _ = preorder_tables(parent, taxon)
    s_pos = se.s_positions(np.asarray(taxon), max(int(arrays.n_taxa), int(np.max(taxon)) + 1))
    out = np.zeros(arrays.n_trees, dtype=np.int64)
    for t in range(arrays.n_trees):
        _, t_tax = be.tree_slice(arrays, t)
        mine = np.sort(s_pos[t_tax[t_tax >= 0]])
        if len(mine) >= 3:
            a, b = np.searchsorted(mine, s_lo), np.searchsorted(mine, s_hi)
            sets = {(int(x), int(y)) for x, y in zip(a, b) if y - x >= 2}
            out[t] = len(mine) + len(sets)
    return out


def queries_held(arrays: TreeArrays, queries) -> np.ndarray:
    """[trees][passes]: how many queries of every pass of PL_QMAX a tree of three or more leaves holds."""
    q = np.asarray(queries)
    n_pass = (len(q) + PL_QMAX - 1) // PL_QMAX
    out = np.zeros((arrays.n_trees, n_pass), dtype=np.int64)
    for t in range(arrays.n_trees):
        _, t_tax = be.tree_slice(arrays, t)
        tips = t_tax[t_tax >= 0]
        if len(tips) >= 3:
            for p in range(n_pass):
                out[t, p] = int(np.isin(q[p * PL_QMAX:(p + 1) * PL_QMAX], tips).sum())
    return out


def clade_passes(parent, taxon, query_nodes) -> list[tuple[int, int, int]]:
    """``(qc, ncl, skip0)`` of every pass of ``sc_clade_rows``: the sub-queries are the tips of the query clades,
    clade by clade, CP_QMAX a pass; ncl the clades a pass touches, skip0 whether its first clade began earlier."""
    lo, hi, _ = preorder_tables(parent, taxon)
    clade = np.concatenate([np.full(int(hi[q] - lo[q]), i) for i, q in enumerate(query_nodes)])
    out = []
    for i0 in range(0, len(clade), CP_QMAX):
        mine = clade[i0:i0 + CP_QMAX]
        out.append((len(mine), int(mine[-1] - mine[0] + 1), int(i0 > 0 and clade[i0 - 1] == mine[0])))
    return out


# ------------------------------------------------------------------------------------------------ the cases
_ids = se._ids
_tree = se._tree


def clades_around(case: se.Case, t: int, positions, least: int = 4, most: int = 60) -> list[int]:
    """The smallest clades of ``least`` .. ``most`` tips around the taxa at (or next to) the T ``positions`` of source
    ``t``."""
    lo, hi, _ = preorder_tables(case.parent, case.taxon)
    _, t_tax = be.tree_slice(case.arrays, t)
    t_tips = t_tax[t_tax >= 0]
    out = []
    for pos in positions:
        step = 1 if pos < len(t_tips) // 2 else -1
        while True:  # (the next T position where the tip's first clade of ``least`` tips is not a large polytomy)
            v = int(np.flatnonzero(case.taxon == t_tips[pos])[0])
            while hi[v] - lo[v] < least:
                v = int(case.parent[v])
            if v > 0 and hi[v] - lo[v] <= most and v not in out:
                break
            pos += step
        out.append(v)
    return out


def tip_nodes(case: se.Case, taxa) -> list[int]:
    """The supertree's tip nodes of ``taxa``."""
    return [int(np.flatnonzero(case.taxon == x)[0]) for x in taxa]


def s_tips(case: se.Case) -> np.ndarray:
    return case.taxon[case.taxon >= 0]


def polytomy_nodes(parent, taxon, count: int = 3) -> list[int]:
    """The ``count`` polytomies of 3 .. PY_KMAX children with the most leaves below them, in preorder."""
    lo, hi, _ = preorder_tables(parent, taxon)
    kids = np.bincount(np.asarray(parent)[1:], minlength=len(parent))
    cand = np.flatnonzero((kids >= 3) & (kids <= PY_KMAX))
    best = cand[np.argsort(-(hi - lo)[cand], kind="stable")[:count]]
    return sorted(int(v) for v in best)


def edge_queries(case: se.Case, count: int, seed: int = 0, absent=()) -> np.ndarray:
    """``count`` query taxa: the tips at S position 0 and at the last position, the first and the last leaf of the
    largest source, ``absent`` (taxa of S that no source holds) and random tips."""
    tips = s_tips(case)
    t = int(np.argmax(case.sizes))
    _, t_tax = be.tree_slice(case.arrays, t)
    t_tips = t_tax[t_tax >= 0]
    first = [int(tips[0]), int(tips[-1]), int(t_tips[0]), int(t_tips[-1]), *[int(x) for x in absent]]
    rest = np.random.RandomState(seed).permutation(tips)
    out = list(dict.fromkeys(first + [int(x) for x in rest]))
    return np.asarray(out[:count], dtype=np.int32)


# ---- tree boundaries inside waves: section 29's forest (WAVE_SIZES) against a mixed S; 11 taxa of S in no source
def wave_case(end: int) -> se.Case:
    case = se.wave_case(end)
    m = case.arrays.n_trees
    absent = np.setdiff1d(s_tips(case), np.unique(case.arrays.taxon[case.arrays.taxon >= 0]))
    lo, hi, _ = preorder_tables(case.parent, case.taxon)
    size = hi - lo
    inner = np.flatnonzero((case.taxon < 0) & (np.arange(len(case.parent)) > 0))
    # clades of about 70, 40, 9 and 2 tips, a tip every source lacks and the first tip
    picks = []
    for want in (70, 40, 9, 2):
        picks.append(int(inner[np.argmin(np.abs(size[inner] - want) + 1e-3 * np.arange(len(inner)))]))
    tip_node = np.flatnonzero(case.taxon >= 0)
    picks += [int(tip_node[np.flatnonzero(np.isin(s_tips(case), absent))[0]]), int(tip_node[0])]
    note = {"queries": edge_queries(case, 9, end, absent[:2]), "absent": absent,
            "clades": sorted(set(picks)), "polytomies": polytomy_nodes(case.parent, case.taxon)}
    return se.Case(f"pl_wave_end_{end}", case.parent, case.taxon, case.arrays, batches=(0, 1, 2, m - 1, m), note=note)


# ---- the last workgroup of a tree: nz = min(zb, zcnt - j0).  S is a star of LAST_TAXA tips under the root beside a
# chain: a source with a tips of the star and the first c >= 2 tips of a caterpillar part has a + c leaves and c - 1
# sets in the part, plus the root's: 2 c + a nodes.  zb = 8 at these sizes.
LAST_NODES = (7, 8, 9, 15, 16, 17, 23, 24, 25)
LAST_TAXA = 60


def last_workgroup_case() -> se.Case:
    """Sources whose S' node counts are LAST_NODES (zb - 1, zb, zb + 1, 2 zb -+ 1, 2 zb, 3 zb -+ 1, 3 zb), between a
    star source (n + 1 nodes) and a two-leaf one."""
    rng = np.random.RandomState(22)
    half = LAST_TAXA // 2
    star, comb = _ids(LAST_TAXA)[:half], _ids(LAST_TAXA)[half:]
    par, tax = se.supertree("caterpillar", comb)
    parent = np.concatenate([[-1], par + 1, np.zeros(half, dtype=np.int32)]).astype(np.int32)
    taxon = np.concatenate([[-1], tax, star]).astype(np.int32)
    comb_order = tax[tax >= 0]  # the caterpillar's tips, deepest first
    trees = [("star", star[:5])]
    for i, z in enumerate(LAST_NODES):
        c = 2 + i % 2 if z >= 2 * (2 + i % 2) + 1 else 2
        a = z - 2 * c
        assert a >= 1
        order = np.concatenate([comb_order[:c], star[:a]])
        trees.append(("random" if i % 2 else "caterpillar", order[rng.permutation(len(order))]))
    trees.append(("balanced", star[:2]))
    trees.append(("random", np.concatenate([comb_order[:6], star[:6]])))
    case = se.Case("pl_last_workgroup", parent, taxon, br.forest(22, LAST_TAXA, trees), batches=(0, 1, 4))
    case.note.update(queries=np.asarray([star[0], comb_order[0], comb_order[1], star[3]], dtype=np.int32),
                     clades=[2, int(np.flatnonzero(taxon == star[0])[0]), 1])
    return case


# ---- 64 words a step of the rows' scans (W > 64 from 2 048 leaves): section 30's pair of a random binary tree and a
# three-leaf tree against a mixed S
WORD_SIZES = be.WORD_SIZES


def words_case(size: int) -> se.Case:
    case = be.words_case(size)
    note = {"queries": edge_queries(case, 3, size), "polytomies": polytomy_nodes(case.parent, case.taxon, 3),
            "clades": clades_around(case, 0, (100, 2040, size - 10))}
    return se.Case(f"pl_words_{size}", case.parent, case.taxon, case.arrays, note=note)


# ---- zb of k_pl_pairs / k_cp_pairs: the rows of k_trip_pairs, W = (n >> 5) + 1 words, zb = min(8, 40 960 / (16 W)),
# and with the sums of a pass of up to 64 queries beside them still far below the cap of 160 KiB
ZB_87 = (10239, 10240)
ZB_21 = (40959, 40960)
ZB_SMALL = (2, 3, 33, 64)


def zb_case(size: int, with_small: bool) -> se.Case:
    """A random binary tree of ``size`` leaves, alone or between the trees of ZB_SMALL, against a mixed S."""
    rng = np.random.RandomState(size + 6)
    kinds = ("random", "caterpillar", "balanced", "star")
    small = [_tree(rng, kinds[i], _ids(size), k) for i, k in enumerate(ZB_SMALL)] if with_small else []
    trees = small[:2] + [_tree(rng, "random", _ids(size), size)] + small[2:]
    parent, taxon = se.supertree("mixed", rng.permutation(size), seed=size + 6)
    case = se.Case(f"pl_zb_{size}{'_batch' if with_small else ''}", parent, taxon, br.forest(size, size, trees))
    case.note.update(queries=edge_queries(case, 2, size), large=len(small[:2]))
    case.note.update(clades=clades_around(case, len(small[:2]), (5, size // 2, size - 3)))
    return case


# ---- the sums beside the rows, under a cap: one tree of CAP_LEAVES leaves (W = 10, 160 bytes a node's rows) and
# CAP_QUERIES queries: a node's sums take 96 bytes, the pass 32
CAP_LEAVES = 300
CAP_QUERIES = 4
CAP_BYTES = (287, 288, 543, 544, 2079, 2080, 0)  # sums 0 | 1 at zb = 1; zb 1 | 2; zb 7 | 8; no cap


def cap_case() -> se.Case:
    rng = np.random.RandomState(35)
    n = CAP_LEAVES + 20
    trees = [_tree(rng, "random", _ids(n), CAP_LEAVES), _tree(rng, "caterpillar", _ids(n), 90),
             _tree(rng, "star", _ids(n), 7)]
    parent, taxon = se.supertree("mixed", rng.permutation(n), seed=35)
    case = se.Case("pl_cap", parent, taxon, br.forest(35, n, trees))
    _, t_tax = be.tree_slice(case.arrays, 0)
    case.note.update(queries=np.asarray(t_tax[t_tax >= 0][[0, 7, 150, CAP_LEAVES - 1]], dtype=np.int32))
    lo, hi, _ = preorder_tables(parent, taxon)
    inner = np.flatnonzero((taxon < 0) & (np.arange(len(parent)) > 0) & (hi - lo == CAP_QUERIES))
    case.note.update(clades=[int(inner[0])])
    return case


# ---- the last pass: 4 ((qc + 4) & ~3) bytes of pref before the rows' sums
LAST_PASS = (64, 65, 66, 67, 68, 69, 128, 129)
PASS_TAXA = 150


@lru_cache(maxsize=None)
def pass_case() -> se.Case:
    """A mixed S of PASS_TAXA tips and 14 sources of 3 .. 70 leaves; the first q entries of ``note["queries"]`` are
    the queries of the case with q of them."""
    rng = np.random.RandomState(64)
    kinds = ("random", "caterpillar", "balanced", "star")
    trees = [_tree(rng, kinds[i % 4], _ids(PASS_TAXA), int(k)) for i, k in
             enumerate((3, 70, 4, 33, 64, 65, 9, 31, 32, 2, 50, 17, 1, 40))]
    parent, taxon = se.supertree("mixed", rng.permutation(PASS_TAXA), seed=64)
    case = se.Case("pl_pass", parent, taxon, br.forest(64, PASS_TAXA, trees))
    case.note.update(queries=edge_queries(case, max(LAST_PASS), 64))
    case.note.update(clades=tip_nodes(case, case.note["queries"]))  # one-tip clades: as many sub-queries as clades
    return case


# ---- the common rows: a tree that holds every query of a pass sends the super marks of the taxa outside pz once
COMMON_TAXA = 200
COMMON_QUERIES = 2 * PL_QMAX + 1


@lru_cache(maxsize=None)
def common_case() -> se.Case:
    """Queries: taxa 0 .. 63 (pass 0), 64 .. 127 (pass 1), 128 (pass 2, held by every tree of three leaves or more).
    Trees, with 130 .. 199 the taxa that are no query: all 64 of pass 0; 63 of them; one; none; then the same for
    pass 1; one with every query; a two-leaf tree between."""
    rng = np.random.RandomState(77)
    free = _ids(COMMON_TAXA)[130:]
    q0, q1, last = _ids(64), _ids(128)[64:], np.asarray([128], dtype=np.int32)
    cat = lambda *parts: np.concatenate(parts).astype(np.int32)  # noqa: E731
    sets = [cat(q0, last, free[:9]), cat(q0[:63], last, free[:5]), cat(q0[5:6], last, free[:30]), cat(last, free[:40]),
            cat(free[:2]),
            cat(q1, last), cat(q1[1:], last, free[3:20]), cat(q1[40:41], last, free[10:12]), cat(last, free[50:52]),
            cat(q0, q1, last, free)]
    kinds = ("random", "caterpillar", "balanced", "random")
    trees = [(kinds[i % 4] if len(s) > 2 else "balanced", s[rng.permutation(len(s))]) for i, s in enumerate(sets)]
    parent, taxon = se.supertree("mixed", rng.permutation(COMMON_TAXA), seed=77)
    case = se.Case("pl_common", parent, taxon, br.forest(77, COMMON_TAXA, trees), batches=(0, 3))
    case.note.update(queries=cat(q0, q1, last))
    return case


# ---- 1 024 nodes a round of k_pl_prefix and of the marks: section 29's supertrees with exactly that many nodes
NODE_COUNTS = (1023, 1024, 1025, 2047, 2048, 2049)


def nodes_case(count: int) -> se.Case:
    case = se.chunk_case(count, "nodes")
    assert len(case.parent) == count
    lo, hi, _ = preorder_tables(case.parent, case.taxon)
    inner = np.flatnonzero((case.taxon < 0) & (np.arange(count) > 0) & (hi - lo >= 3) & (hi - lo <= 12))
    note = {"queries": edge_queries(case, 5, count), "clades": [int(inner[0]), int(inner[-1])]}
    return se.Case(f"pl_nodes_{count}", case.parent, case.taxon, case.arrays, note=note)


# ---- caterpillar lists: a caterpillar source queried at its deepest tip (m - 1 groups), at its shallowest (one group
# of m - 1 leaves) and at tips of a balanced source (about log m groups) in one pass
COMB_LEAVES = 1000


def lists_case() -> se.Case:
    rng = np.random.RandomState(91)
    n = COMB_LEAVES + 30
    comb = br.order_random(rng, _ids(n), COMB_LEAVES)
    trees = [("caterpillar", comb), _tree(rng, "balanced", _ids(n), COMB_LEAVES), _tree(rng, "random", _ids(n), 5)]
    parent, taxon = se.supertree("mixed", rng.permutation(n), seed=91)
    case = se.Case("pl_lists", parent, taxon, br.forest(91, n, trees))
    case.note.update(queries=np.asarray([comb[0], comb[-1], comb[1], comb[COMB_LEAVES // 2], comb[-2]], dtype=np.int32))
    return case


# ---- polytomies.  S: the root with k children, child i a mixed subtree on a block of the taxa; T: one random binary
# tree on all of them, so that every colour is spread over all of T's leaf order
def block_supertree(blocks, seed: int):
    """The root with one mixed subtree per block of taxa (a single taxon: a tip)."""
    parent, taxon = [np.asarray([-1], dtype=np.int32)], [np.asarray([-1], dtype=np.int32)]
    at = 1
    for i, blk in enumerate(blocks):
        par, tax = se.supertree("mixed", blk, seed=seed + i)
        par = np.where(par < 0, 0, par + at).astype(np.int32)
        parent.append(par)
        taxon.append(tax)
        at += len(par)
    return np.concatenate(parent).astype(np.int32), np.concatenate(taxon).astype(np.int32)


# k = 64: the launch passes 64 KiB; the rows alone do; the stride goes odd | even; the sums leave LDS; the last sizes
PY_WIDE = (2016, 2017, 4096, 4097, 8160, 8161, 8192, 8193, 10239, 10240)
PY_LIMIT_3 = 218432  # the largest tree with k = 3
PY_THREE = (2047, 2048, 2049, 87264, 87265, PY_LIMIT_3)  # k = 3: 64 words a scan step; 64 KiB; the limit


def py_case(size: int, k: int) -> se.Case:
    """One random binary tree of ``size`` leaves and a five-leaf tree against the root polytomy of ``k`` blocks of
    unequal sizes; the query nodes are the root and the largest polytomy inside a block."""
    rng = np.random.RandomState(size + k)
    cuts = np.sort(rng.permutation(np.arange(1, size))[: k - 1])
    ids = rng.permutation(size).astype(np.int32)
    blocks = np.split(ids, cuts)
    parent, taxon = block_supertree(blocks, size)
    trees = [_tree(rng, "random", _ids(size), size), _tree(rng, "balanced", _ids(size), 5)]
    inner = [v for v in polytomy_nodes(parent, taxon, 2) if v != 0][:1]
    return se.Case(f"py_{size}_k{k}", parent, taxon, br.forest(size + k, size, trees), note={"polytomies": [0, *inner]})


# ---- colours: k = 3, 4, 63, 64 children of one or two tips each; sources that lack the first, the last or a middle
# colour, hold exactly two or three colours, a star, a two-leaf and a one-leaf tree between decisive ones
COLOUR_DEGREES = (3, 4, 63, 64)


def colour_case(k: int) -> se.Case:
    rng = np.random.RandomState(k)
    n = 2 * k
    blocks = [np.asarray([2 * i, 2 * i + 1], dtype=np.int32) for i in range(k)]
    parent, taxon = block_supertree(blocks, k)
    every = _ids(n)
    pick = lambda cols: np.concatenate([blocks[c] for c in cols]).astype(np.int32)  # noqa: E731
    mid = k // 2
    sets = [every, every[2:], pick([0, 1]), every[:-2], np.delete(every, [2 * mid, 2 * mid + 1]), every[:1],
            pick([0, mid, k - 1]), every[:2], pick([1, k - 1]), every[::2], pick([0, 1, 2])[1:], every]
    kinds = ("random", "caterpillar", "balanced", "random", "caterpillar", "balanced", "star", "balanced", "random",
             "star", "caterpillar", "star")
    trees = [(kind, s[rng.permutation(len(s))]) for kind, s in zip(kinds, sets)]
    return se.Case(f"py_colours_{k}", parent, taxon, br.forest(k, n, trees), batches=(0, 1, 5), note={"polytomies": [0]})


# ---- counts from 2^32 on
BIG_BLOCK = be.BIG_BLOCK


def big_polytomy_case() -> se.Case:
    """Three polytomies of BIG_BLOCK tips under the root against a caterpillar that lists the first two blocks, then
    the third, each part shuffled, with a few taxa moved: joint[0][1][2] is nearly |A||B||D| = 4.36 x 10^9."""
    n = 3 * BIG_BLOCK
    rng = np.random.RandomState(33)
    ids = rng.permutation(n).astype(np.int32)
    blocks = [ids[i * BIG_BLOCK:(i + 1) * BIG_BLOCK] for i in range(3)]
    parent = np.asarray([-1] + sum(([0] + [1 + i * (BIG_BLOCK + 1)] * BIG_BLOCK for i in range(3)), []), dtype=np.int32)
    taxon = np.concatenate(sum(([np.asarray([-1]), b] for b in blocks), [np.asarray([-1])])).astype(np.int32)
    ab = np.concatenate(blocks[:2])
    t_order = np.concatenate([ab[rng.permutation(len(ab))], blocks[2][rng.permutation(BIG_BLOCK)]])
    for _ in range(40):
        i, j = rng.randint(0, n, size=2)
        t_order[i], t_order[j] = t_order[j], t_order[i]
    return se.Case("py_big", parent, taxon, br.forest(33, n, [("caterpillar", t_order)]), note={"polytomies": [0]})


BIG_TWIN = 100003  # C(n - 1, 2) = 5.0 x 10^9 triples with x, all of them shared at x's own place


def big_placement_case() -> se.Case:
    """Section 30's twin trees: a random binary S and the same topology with children exchanged as its one source."""
    case = be.twin_case(BIG_TWIN)
    tips = s_tips(case)
    lo, hi, _ = preorder_tables(case.parent, case.taxon)
    cherry = np.flatnonzero((hi - lo == 2) & (case.taxon < 0))
    note = {"queries": tips[[0, BIG_TWIN // 3]].astype(np.int32), "clades": [int(cherry[0]), int(cherry[-1])]}
    return se.Case("pl_big", case.parent, case.taxon, case.arrays, note=note)


# ---- clade passes: the sub-queries are the tips of the query clades in turn, CP_QMAX a pass
CLADE_PASSES = {"64_5": (64, 5), "63_2": (63, 2), "65": (65,), "128": (128,), "129": (129,), "ones": (1,) * 64 + (3,)}


def clade_pass_case(which: str) -> se.Case:
    """S: the root over one mixed subtree per clade size of CLADE_PASSES[which] and a rest of 30 tips; the query
    nodes are those subtrees' roots in turn.  Nine sources of 3 .. 90 leaves."""
    sizes = CLADE_PASSES[which]
    rng = np.random.RandomState(len(which) + sum(sizes))
    n = sum(sizes) + 30
    ids = rng.permutation(n).astype(np.int32)
    blocks = np.split(ids, np.cumsum(sizes))
    parent, taxon = block_supertree(blocks, n)
    clades = [int(v) for v in np.flatnonzero(np.asarray(parent) == 0)[:len(sizes)]]
    kinds = ("random", "caterpillar", "balanced", "star")
    trees = [_tree(rng, kinds[i % 4], _ids(n), min(int(k), n)) for i, k in enumerate((90, 3, 40, 2, 64, 33, 12, 5, 70))]
    return se.Case(f"cp_pass_{which}", parent, taxon, br.forest(n, n, trees), batches=(0, 4), note={"clades": clades})


# ---- clade masks: Q' against the nodes z of S' around it
MASK_SIZES = (3, 4, 7, 17, 40)
MASK_LARGE = 2100
MASK_TIPS = 40  # the clade of the large case


def mask_case(n: int) -> se.Case:
    """A caterpillar S of ``n`` tips in the identity order (the tips deepest first: node j holds the first n - j).
    Up to 40 tips the query nodes are the clade of the first two tips, of all but one, of half, the first and the last
    tip, and the sources hold all taxa, all but the last, all but the first, the first three, the last three, two.
    At MASK_LARGE the large clade holds the first MASK_TIPS tips and the sources all taxa, those tips and one more
    (all but one leaf of L), those tips alone (all of L), the others (none), and all but the first."""
    rng = np.random.RandomState(n)
    parent, taxon = se.supertree("caterpillar", _ids(n))
    every = _ids(n)
    tip_node = np.flatnonzero(taxon >= 0)
    if n > 40:
        k = MASK_TIPS
        sets = [every, every[:k + 1], every[:k], every[k:], every[:3], every[:k - 1], every[1:]]
        clades = sorted({n - 2, n - k, int(tip_node[0]), int(tip_node[-1])})
    else:
        sets = [every, every[:max(3, n - 1)], every[1:] if n > 3 else every, every[:3], every[-3:], every[:2]]
        clades = sorted({n - 2, 1, max(1, (n - 1) // 2), int(tip_node[0]), int(tip_node[-1])})
    kinds = ("random", "caterpillar", "balanced", "random", "star", "caterpillar", "balanced")
    trees = [(kind, s[rng.permutation(len(s))]) for kind, s in zip(kinds, sets)]
    return se.Case(f"cp_mask_{n}", parent, taxon, br.forest(n, n, trees), batches=(0, 2), note={"clades": clades})


def mask_relations(case: se.Case) -> set:
    """What the sources of a mask case show, as a set of names: per (clade, tree of three leaves or more)
    ``none`` / ``one`` / ``all_but_one`` / ``all`` by |Q' ∩ L|, ``first`` / ``last`` when a crossing Q' begins or ends
    S', and for the nodes z of S' (sets of two or more leaves) ``z_equal``, ``z_inside`` (inside a larger Q') and
    ``z_one_more``."""
    sup = _Super(case.parent, case.taxon, case.arrays.n_taxa)
    out = set()
    for t in range(case.arrays.n_trees):
        src = _Source(case.arrays, t, sup)
        if src.m < 3:
            continue
        mine = np.sort(src.spos)
        a, b = np.searchsorted(mine, sup.lo), np.searchsorted(mine, sup.hi)  # S' range of every S node
        z = {(int(x), int(y)) for x, y in zip(a, b) if y - x >= 2}
        for q in case.note["clades"]:
            qa, qb = int(a[q]), int(b[q])
            size = qb - qa
            out |= {("none",) if size == 0 else ("all",) if size == src.m else ("one",) if size == 1 else ()}
            out |= {("all_but_one",)} if size == src.m - 1 else set()
            if 0 < size < src.m:
                out |= {("first",)} if qa == 0 else set()
                out |= {("last",)} if qb == src.m else set()
                out |= {("z_equal",)} if (qa, qb) in z else set()
                out |= {("z_inside",)} if any(qa <= x and y <= qb and y - x < size for x, y in z) else set()
                out |= {("z_one_more",)} if any(x <= qa and qb <= y and y - x == size + 1 for x, y in z) else set()
    return {x[0] for x in out if x}


# ---- more trees than a grid row of k_py_sweep (65 535): three-leaf sources on GRID_TAXA taxa.  S: the root with
# three children -- a polytomy of four stars of three tips (taxa 0 .. 11), a star of four (12 .. 15), a star of four
# (16 .. 19); the query nodes are the root (k = 3) and the polytomy (k = 4)
GRID_COUNTS = (PY_GRID_Y, PY_GRID_Y + 1, PY_GRID_Y + 2)
GRID_TAXA = 20


def grid_supertree():
    parent, taxon = [-1, 0], [-1, -1]
    for i in range(4):
        at = len(parent)
        parent += [1, at, at, at]
        taxon += [-1, 3 * i, 3 * i + 1, 3 * i + 2]
    for i in range(2):
        at = len(parent)
        parent += [0, at, at, at, at]
        taxon += [-1, *range(12 + 4 * i, 16 + 4 * i)]
    return np.asarray(parent, dtype=np.int32), np.asarray(taxon, dtype=np.int32)


@lru_cache(maxsize=None)
def grid_sources(count: int = GRID_COUNTS[-1]):
    """``(orders [count][3], caterpillar [count])``: tree i is ((a, b), c) where ``caterpillar[i]``, else (a, (b, c));
    the trees from 65 535 on have the other shape than the trees 65 535 before them and are decisive, so that a launch
    that read the first trees' nodes for them would count other triples."""
    rng = np.random.RandomState(65)
    orders = np.argsort(rng.rand(count, GRID_TAXA), axis=1)[:, :3].astype(np.int32)
    cat = rng.rand(count) < 0.5
    cat[PY_GRID_Y:] = ~cat[:count - PY_GRID_Y]
    # ... and are decisive: tree 65 535 at the root (one taxon of each child), tree 65 536 at the polytomy
    orders[PY_GRID_Y:] = np.asarray([[0, 13, 17], [1, 4, 7]], dtype=np.int32)[:count - PY_GRID_Y]
    return orders, cat


def grid_tables(count: int):
    """The flattened tables of the first ``count`` sources (``score_edge_reference.budget_tables``, vectorised)."""
    from spectralclustersupertree_amd.flatten import TreeTables
    orders, cat = grid_sources()
    orders, cat = orders[:count], cat[:count]
    adj = np.where(cat[:, None], [1, 0, 0], [0, 1, 0]).astype(np.int32)
    return TreeTables(n_taxa=GRID_TAXA, tree_off=3 * np.arange(count + 1, dtype=np.int64), leaf_taxon=orders.ravel().copy(),
                      adj_depth=adj.ravel().copy(), adj_val=np.ones(3 * count), tree_w=np.ones(count))


def grid_trees(which) -> list:
    """``(kind, order)`` of the sources ``which``, for ``build_reference.forest``."""
    orders, cat = grid_sources()
    return [("caterpillar" if cat[i] else "balanced", orders[i]) for i in which]


def three_leaf_polytomies(parent, taxon, query_nodes, orders, cat) -> dict:
    """The outputs of ``scs_score_polytomies`` for three-leaf sources: a source is decisive at a query node when its
    taxa have three different colours there; it then adds 1 to ``total`` at [i][j][l] for each of its colours as l
    (i < j the other two) and 1 to ``joint`` where l is the colour of its outgroup."""
    lo, hi, _ = preorder_tables(parent, taxon)
    start, kid = children(parent)
    s_pos = se.s_positions(np.asarray(taxon), int(np.max(taxon)) + 1)
    out_at = np.where(cat, 2, 0)  # ((a, b), c): c is the outgroup; (a, (b, c)): a
    res = {"py_degree": [], "py_trees": [], "py_total": [], "py_joint": []}
    for q in query_nodes:
        kids = kid[start[q]:start[q + 1]]
        k = len(kids)
        bnd = np.concatenate([lo[kids], [hi[q]]])
        col = np.searchsorted(bnd, s_pos[orders], side="right") - 1
        ok = ((col >= 0) & (col < k)).all(axis=1)
        c = np.sort(col, axis=1)
        dec = ok & (c[:, 0] < c[:, 1]) & (c[:, 1] < c[:, 2])
        total = np.zeros((k, k, k), dtype=np.int64)
        joint = np.zeros((k, k, k), dtype=np.int64)
        cd = c[dec]
        for i, j, l in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            np.add.at(total, (cd[:, i], cd[:, j], cd[:, l]), 1)
        og = col[dec, out_at[dec]]
        rest = np.sort(np.where(np.arange(3)[None, :] == out_at[dec][:, None], k, col[dec]), axis=1)[:, :2]
        np.add.at(joint, (rest[:, 0], rest[:, 1], og), 1)
        res["py_degree"].append(k)
        res["py_trees"].append(int(dec.sum()))
        res["py_total"].append(total)
        res["py_joint"].append(joint)
    res["py_degree"] = np.asarray(res["py_degree"], dtype=np.int32)
    res["py_trees"] = np.asarray(res["py_trees"], dtype=np.int64)
    return res


# ---- refusals: section 29's tables; the queries of all four exports on its supertree
def refusal_queries(parent, taxon) -> dict:
    tips = taxon[taxon >= 0]
    lo, hi, _ = preorder_tables(parent, taxon)
    inner = np.flatnonzero((taxon < 0) & (np.arange(len(parent)) > 0) & (hi - lo >= 2))
    return {"queries": tips[[0, 5, len(tips) - 1]].astype(np.int32), "clades": [int(inner[0]), int(inner[-1])],
            "polytomies": polytomy_nodes(parent, taxon, 2)}


# ---- dynamic LDS above 64 KiB, the no-sums path where it begins by itself and the leaf limit: one random binary tree
# of that many leaves and a five-leaf tree against section 30's blocks supertree (a balanced top over polytomies: the
# cluster sizes sum to O(n log n), and 2 x queries x nodes x 24 bytes of rows stay inside the call's workspace)
LDS_64K = (130943, 130944)  # one query, zb = 1: the launch takes 64 KiB | 16 bytes more
NO_SUMS_64 = (325023, 325024)  # 64 queries: sums 1 | 0
NO_SUMS_1 = (327551, 327552)  # one query: sums 1 | 0


def large_case(size: int, n_queries: int) -> se.Case:
    rng = np.random.RandomState(size % 1000 + n_queries)
    parent, taxon = be.blocks_supertree(size, 10, size)
    trees = [_tree(rng, "random", _ids(size), size), _tree(rng, "balanced", _ids(size), 5)]
    case = se.Case(f"pl_large_{size}_q{n_queries}", parent, taxon, br.forest(size % 1000, size, trees))
    case.note.update(queries=edge_queries(case, n_queries, size))
    case.note.update(clades=tip_nodes(case, case.note["queries"][:1]))  # (S's inner nodes hold 300 tips and more)
    return case


# ---- the Q' row of k_cp_clades past 64 words: a random binary tree of CLADE_WORDS leaves crossed by clades of a few
# tips, which lie all over T's leaf order
CLADE_WORDS = 2100


def clade_words_case(size: int = CLADE_WORDS) -> se.Case:
    """Section 30's pair at ``size`` leaves; the query clades are the smallest ones of four or more tips around the
    taxa at T positions 100, 2 050 and size - 10: two of them have tips in the words from 64 on."""
    case = be.words_case(size)
    lo, hi, _ = preorder_tables(case.parent, case.taxon)
    _, t_tax = be.tree_slice(case.arrays, 0)
    t_tips = t_tax[t_tax >= 0]
    clades = []
    for pos in (100, 2050, size - 10):
        v = int(np.flatnonzero(case.taxon == t_tips[pos])[0])
        while hi[v] - lo[v] < 4:
            v = int(case.parent[v])
        clades.append(v)
    assert len(set(clades)) == 3 and 0 not in clades
    return se.Case(f"cp_words_{size}", case.parent, case.taxon, case.arrays, note={"clades": clades})


# ---- the byte budget: section 29's three-leaf sources on BUDGET_LEAVES taxa (the rows alone, 4 bytes x row stride a
# tree, pass SC_BUDGET at about 4 000 trees) against three mixed blocks under the root; each export splits where its
# own bytes per leaf and per tree say
BUDGET_EXPORTS = ("score_placements", "score_clade_placements", "score_polytomies")
BUDGET_QUERIES = 3


def budget_first_split(export: str) -> int:
    """M*: the smallest count of three-leaf trees the export's plan splits in two batches."""
    row_stride = br.round_up(se.BUDGET_LEAVES, se.SC_ROW_ALIGN)
    epl, ept = export_extras(export, BUDGET_QUERIES, (3,))
    return se.SC_BUDGET // se.per_tree(3, row_stride, se.levels_of(3), epl, ept) + 1


@lru_cache(maxsize=None)
def budget_supertree():
    """Three mixed blocks under the root; the three polytomy sources around their split have a taxon in each."""
    first = budget_first_split("score_polytomies")
    trees = se.budget_trees(first + 1)
    blk = np.random.RandomState(98).randint(0, 3, size=se.BUDGET_LEAVES)
    for t in (first - 2, first - 1, first):
        blk[np.asarray(trees[t][1])] = [0, 1, 2]
    ids = np.argsort(blk, kind="stable").astype(np.int32)
    return block_supertree(np.split(ids, np.cumsum(np.bincount(blk, minlength=3))[:2]), 98)


def budget_case(export: str, count: int) -> se.Case:
    """The first ``count`` sources; the queries are taxa (tips, for the clades) of the trees around the split, the
    polytomy is the root."""
    first = budget_first_split(export)
    trees = se.budget_trees(first + 1)
    parent, taxon = budget_supertree()
    case = se.Case(f"budget_{export}_{count}", parent, taxon, br.forest(98, se.BUDGET_LEAVES, trees[:count]))
    taxa = np.asarray([trees[first - 2][1][0], trees[first - 1][1][1], trees[first][1][2]], dtype=np.int32)
    assert len(set(taxa.tolist())) == BUDGET_QUERIES
    case.note.update(queries=taxa, clades=tip_nodes(case, taxa), polytomies=[0], tables=se.budget_tables(trees[:count]))
    return case
