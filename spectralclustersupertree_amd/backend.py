"""Host-side handles on the device objects of libscs_hip.so.

``Device`` owns one context (one process <-> one MI355X); ``DeviceGraph`` is a
row block of the proper-cluster-graph weight matrix resident in HBM.  These are
thin: every number is produced by the HIP kernels behind include/scs_hip.h.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from spectralclustersupertree_amd import _env
from spectralclustersupertree_amd import _native as nv
from spectralclustersupertree_amd.flatten import TreeTables

DEFAULT_TOL = 1e-13
DEFAULT_MAX_ITER = 2000

# output dims of ``Device._score_call``: per source tree, per supertree node, per query, queries x nodes, queries x top_k
_M, _N, _Q, _QN, _QK = ("m",), ("n_nodes",), ("nq",), ("nq", "n_nodes"), ("nq", "top_k")


def _resident_solve() -> bool:
    """SCS_RESIDENT_SOLVE=0 (diagnostic): small nodes pack their tables on the host even when the
    tables are resident on the device."""
    return bool(int(_env.probe("SCS_RESIDENT_SOLVE", "1")))


class Device:
    """One libscs_hip context.  ``Device()`` = GPU 0, single rank."""

    def __init__(self, device: int = 0, rank: int = 0, world: int = 1, unique_id: bytes | None = None,
                 *, _local_group=None) -> None:
        self._lib = nv.load_library()
        self._ctx = C.c_void_p()
        self.rank, self.world = rank, world
        self.index = device  # the GPU this context lives on
        if _local_group is not None:
            nv.check(self._lib.scs_ctx_create_local(device, rank, _local_group, C.byref(self._ctx)))
        else:
            uid = None
            if unique_id is not None:
                if len(unique_id) != nv.UNIQUE_ID_BYTES:
                    msg = f"unique_id must be {nv.UNIQUE_ID_BYTES} bytes"
                    raise ValueError(msg)
                uid = C.create_string_buffer(bytes(unique_id), nv.UNIQUE_ID_BYTES)
            nv.check(self._lib.scs_ctx_create(device, rank, world, uid, C.byref(self._ctx)))

    @staticmethod
    def unique_id() -> bytes:
        """RCCL bootstrap id; rank 0 creates it and ships it to the other ranks."""
        lib = nv.load_library()
        buf = C.create_string_buffer(nv.UNIQUE_ID_BYTES)
        nv.check(lib.scs_comm_unique_id(buf))
        return buf.raw

    def close(self) -> None:
        if self._ctx:
            self._lib.scs_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self) -> "Device":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def synchronize(self) -> None:
        nv.check(self._lib.scs_ctx_synchronize(self._ctx))

    def trim(self, keep_bytes: int = 0) -> None:
        """``scs_ctx_trim``: hand whole free slabs of the device's arena back to the driver until at most
        ``keep_bytes`` of free arena memory remain (the arena is shared by every context of the process on this
        device and never shrinks by itself)."""
        nv.check(self._lib.scs_ctx_trim(self._ctx, int(keep_bytes)))

    def reserve(self, n_bytes: int) -> None:
        """``scs_ctx_reserve``: the device's arena holds ``n_bytes`` of free memory in one piece afterwards."""
        nv.check(self._lib.scs_ctx_reserve(self._ctx, int(n_bytes)))

    def arena_stats(self) -> dict:
        """``scs_debug_arena_stats`` of this context's device."""
        out = (C.c_int64 * 8)()
        nv.check(self._lib.scs_debug_arena_stats(int(self.index), out))
        keys = ("slab_bytes", "used_bytes", "slabs", "chunks", "pending_chunks", "driver_allocations",
                "driver_releases", "requests")
        return dict(zip(keys, (int(x) for x in out)))

    def comm_info(self) -> dict:
        """The communicator as it sees itself (``scs_ctx_comm_info``): kind, the world / rank it was
        created with and what ncclCommCount / ncclCommUserRank report (-1: not available)."""
        v = [C.c_int32(0) for _ in range(5)]
        nv.check(self._lib.scs_ctx_comm_info(self._ctx, *[C.byref(x) for x in v]))
        kind, world, rank, rep_world, rep_rank = (int(x.value) for x in v)
        return {"kind": {0: "none", 1: "rccl", 2: "in-process team"}.get(kind, str(kind)), "world": world,
                "rank": rank, "reported_world": rep_world, "reported_rank": rep_rank}

    # -- tables ------------------------------------------------------------
    def upload(self, tables: TreeTables) -> "DeviceTables":
        tables.validate(ranges=False)  # (ranges: checked by a kernel on the uploaded copy)
        handle = C.c_void_p()
        res = getattr(tables, "resident", None)
        if res is not None and _resident_solve() and res[0].dev.index == self.index and res[0]._h:
            # the tables are on this device already (a child of scs_forest_split): device-to-device
            forest, relabel = res
            rl = None if relabel is None else np.ascontiguousarray(relabel, dtype=np.int32)
            nv.check(self._lib.scs_tables_from_forest(self._ctx, forest._h, nv.iptr(rl) if rl is not None else None,
                                                      int(tables.n_taxa), C.byref(handle)))
            return DeviceTables(self, handle, tables.n_taxa, tables.n_trees, bool(tables.monotone))
        rc = self._lib.scs_tables_upload(
            self._ctx, tables.n_taxa, tables.n_trees, nv.lptr(tables.tree_off),
            nv.iptr(tables.leaf_taxon), nv.iptr(tables.adj_depth), nv.dptr(tables.adj_val),
            nv.dptr(tables.tree_w), C.byref(handle),
        )
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_tables_upload: invalid tables")
        nv.check(rc)
        out = DeviceTables(self, handle, tables.n_taxa, tables.n_trees, bool(tables.monotone))
        out._source = tables  # (page-locked arrays may still be read until the first build returns)
        return out

    # -- scoring a supertree ----------------------------------------------------
    def _score_call(self, export: str, sources, parent, taxon, ints, outputs, queries=None, noun: str = "",
                    top_k=None, sizes=None, weights=None) -> dict:
        """One ``scs_score_*`` export.  ``sources`` are uploaded when they are ``TreeTables``; ``parent`` / ``taxon``
        (and ``queries``, which ``noun`` names in the shape message) travel as int32.  The export takes the context,
        the tables, the supertree, ``ints``, then the query count and ``queries``, then ``top_k``, then one buffer per
        output.  ``outputs``: ``(names, dims[, dtype, fill])`` entries with ``dims`` out of ``m`` (source trees),
        ``n_nodes``, ``n_tips``, ``nq``, ``top_k`` and the keys of ``sizes``; int64 zeros unless said otherwise; ``dims``
        None: not asked for (a null pointer, and None in the result).  ``weights``: one more int32 input, rows x ``m``,
        sent after ``ints`` as its row count (``n_rep`` in ``dims``) and the array.
        Returns name -> array in that order; SCS_EINVAL becomes ``ValueError`` with the library's message."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        parent = np.ascontiguousarray(parent, dtype=np.int32)
        taxon = np.ascontiguousarray(taxon, dtype=np.int32)
        size = {"m": tabs.n_trees, "n_nodes": len(parent), **(sizes or {})}
        args = [int(x) for x in ints]
        ok, msg = taxon.shape == (len(parent),), "parent and taxon must have one entry per supertree node"
        if queries is not None:
            queries = np.ascontiguousarray(queries, dtype=np.int32)
            size["nq"] = len(queries)
            args += [size["nq"], nv.iptr(queries)]
            ok, msg = ok and queries.ndim == 1, f"{msg}, {noun}"
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.int32)
            ok = ok and weights.ndim == 2 and weights.shape[1] == size["m"]
            msg = f"{msg}, weights one row per replicate with one entry per source tree"
            size["n_rep"] = len(weights)
            args += [size["n_rep"], nv.iptr(weights)]
        if not ok:
            raise ValueError(msg)
        if top_k is not None:
            size["top_k"] = max(int(top_k), 0)
            args.append(int(top_k))
        if any(dims is not None and "n_tips" in dims for _, dims, *_ in outputs):
            size["n_tips"] = len(parent) - len(np.unique(parent[1:]))
        out = {}
        for names, dims, *rest in outputs:
            dtype, fill = rest or (np.int64, 0)
            shape = None if dims is None else tuple(size[d] for d in dims)
            for name in names:
                out[name] = (None if shape is None else np.zeros(shape, dtype=dtype) if fill == 0
                             else np.full(shape, fill, dtype=dtype))
        rc = getattr(self._lib, export)(self._ctx, tabs._h, len(parent), nv.iptr(parent), nv.iptr(taxon), *args,
                                        *(None if v is None else v.ctypes.data for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else f"{export}: invalid input")
        nv.check(rc)
        return out

    def score(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0) -> dict:
        """``scs_score_supertree``: RF terms per source tree and clade support per supertree node.

        ``sources`` are the flattened source trees (``TreeTables``, uploaded here, or ``DeviceTables``) over
        the supertree's taxon ids; ``parent`` / ``taxon`` the supertree in preorder (parent -1 at the root,
        taxon -1 at inner nodes).  ``batch_trees`` > 0 caps the trees of one device batch.  Returns int64
        arrays ``n_super``, ``n_source``, ``shared`` (per tree) and ``informative``, ``supported`` (per node).
        """
        return self._score_call("scs_score_supertree", sources, parent, taxon, (batch_trees,),
                                ((("n_super", "n_source", "shared"), _M), (("informative", "supported"), _N)))

    def score_triplets(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0) -> dict:
        """``scs_score_triplets``: rooted triplet terms per source tree, with the inputs of ``score``.  Returns int64
        arrays ``t_super``, ``t_source``, ``t_shared`` (per tree)."""
        return self._score_call("scs_score_triplets", sources, parent, taxon, (batch_trees,),
                                ((("t_super", "t_source", "t_shared"), _M),))

    def score_conflicts(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0) -> dict:
        """``scs_score_conflicts``: clade conflict counts, with the inputs of ``score``.  Returns int64 arrays
        ``n_super_conflict``, ``n_source_conflict`` (per tree) and ``conflicting`` (per node)."""
        return self._score_call("scs_score_conflicts", sources, parent, taxon, (batch_trees,),
                                ((("n_super_conflict", "n_source_conflict"), _M), (("conflicting",), _N)))

    def score_concordance(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0) -> dict:
        """``scs_score_concordance``: branch concordance counts, with the inputs of ``score``.  Returns int64 arrays
        ``n_decisive``, ``n_concordant``, ``n_alternative`` (per tree) and ``decisive``, ``concordant``, ``alt1``,
        ``alt2`` (per node)."""
        return self._score_call("scs_score_concordance", sources, parent, taxon, (batch_trees,),
                                ((("n_decisive", "n_concordant", "n_alternative"), _M),
                                 (("decisive", "concordant", "alt1", "alt2"), _N)))

    def score_branch_triplets(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0) -> dict:
        """``scs_score_branch_triplets``: per-branch triplet support, with the inputs of ``score``.  Returns int64
        arrays ``n_bt_total``, ``n_bt_concordant``, ``n_bt_alternative`` (per tree) and ``bt_total``,
        ``bt_concordant``, ``bt_alt1``, ``bt_alt2`` (per node)."""
        return self._score_call("scs_score_branch_triplets", sources, parent, taxon, (batch_trees,),
                                ((("n_bt_total", "n_bt_concordant", "n_bt_alternative"), _M),
                                 (("bt_total", "bt_concordant", "bt_alt1", "bt_alt2"), _N)))

    def score_branch_resample(self, sources, parent: np.ndarray, taxon: np.ndarray, weights, rows: bool = False,
                              batch_trees: int = 0) -> dict:
        """``scs_score_branch_resample``: the per-branch triplet counts under ``weights``, R rows of one non-negative
        integer weight per tree of the tables (row 0 the point estimate, the others replicates), with the inputs of
        ``score``.  Returns ``rs_point`` (int64, 4 x nodes: total, concordant, alt1, alt2 of row 0), ``rs_wins``
        (int32, 4 x nodes: the replicates won by concordant, alt1, alt2 and tied) and ``rs_rows`` (int64,
        4 x R x nodes with ``rows``, else None)."""
        w = np.asarray(weights)
        if w.size and (w.min() < np.iinfo(np.int32).min or w.max() > np.iinfo(np.int32).max):
            msg = "scs_score_branch_resample: a tree weight does not fit int32 (at most 2^31 - 1)"
            raise ValueError(msg)
        return self._score_call("scs_score_branch_resample", sources, parent, taxon, (batch_trees,),
                                ((("rs_point",), ("x4", "n_nodes")), (("rs_wins",), ("x4", "n_nodes"), np.int32, 0),
                                 (("rs_rows",), ("x4", "n_rep", "n_nodes") if rows else None)),
                                sizes={"x4": 4}, weights=w)

    def score_taxon_triplets(self, sources, parent: np.ndarray, taxon: np.ndarray, batch_trees: int = 0,
                             lds_bytes: int = 0) -> dict:
        """``scs_score_taxon_triplets``: per-taxon triplet support, with the inputs of ``score``.  Returns int64
        arrays ``tx_trees``, ``tx_total``, ``tx_super``, ``tx_source``, ``tx_shared`` with one entry per supertree tip,
        indexed by taxon id (the tips' ids must be 0 .. tips - 1, as ``supertree_arrays`` numbers them).
        ``lds_bytes`` > 0 caps the LDS one workgroup of the pair kernel takes (tests)."""
        return self._score_call("scs_score_taxon_triplets", sources, parent, taxon, (batch_trees, lds_bytes),
                                ((("tx_trees", "tx_total", "tx_super", "tx_source", "tx_shared"), ("n_tips",)),))

    def score_placements(self, sources, parent: np.ndarray, taxon: np.ndarray, queries, batch_trees: int = 0,
                         lds_bytes: int = 0) -> dict:
        """``scs_score_placements``: the triplet terms every query taxon would have on the edge above every supertree
        node, with the inputs of ``score`` and ``queries`` = taxon ids of supertree tips, each once.  Returns int64
        arrays ``pl_trees``, ``pl_total``, ``pl_source`` (one entry per query) and ``pl_super``, ``pl_shared``
        (queries x nodes).  ``lds_bytes`` > 0 caps the LDS one workgroup of the pair kernel takes (tests)."""
        return self._score_call("scs_score_placements", sources, parent, taxon, (batch_trees, lds_bytes),
                                ((("pl_trees", "pl_total", "pl_source"), _Q), (("pl_super", "pl_shared"), _QN)),
                                queries, "queries one per query taxon")

    def score_clade_placements(self, sources, parent: np.ndarray, taxon: np.ndarray, query_nodes,
                               batch_trees: int = 0, lds_bytes: int = 0) -> dict:
        """``scs_score_clade_placements``: the triplet terms the subtree of every query node would have on the edge
        above every supertree node, with the inputs of ``score`` and ``query_nodes`` = preorder indices of supertree
        nodes (not the root), each once.  Returns int64 arrays ``cp_trees``, ``cp_total``, ``cp_source`` (one entry
        per query) and ``cp_super``, ``cp_shared`` (queries x nodes).  ``lds_bytes`` as for ``score_placements``."""
        return self._score_call("scs_score_clade_placements", sources, parent, taxon, (batch_trees, lds_bytes),
                                ((("cp_trees", "cp_total", "cp_source"), _Q), (("cp_super", "cp_shared"), _QN)),
                                query_nodes, "query_nodes one per query clade")

    def score_clade_moves(self, sources, parent: np.ndarray, taxon: np.ndarray, query_nodes, top_k: int = 4,
                          batch_trees: int = 0, lds_bytes: int = 0) -> dict:
        """``scs_score_clade_moves``: the sweep of ``score_clade_placements`` with every row reduced on the device to
        the clade's own entry and its ``top_k`` (1 to 8) best regraft targets outside its subtree, by
        (``mv_super`` - 2 ``mv_shared``, node) ascending.  Returns int64 arrays ``cp_trees``, ``cp_total``,
        ``cp_source``, ``mv_own_super``, ``mv_own_shared`` (one entry per query), ``mv_node`` (int32) and ``mv_super``,
        ``mv_shared`` (queries x top_k; -1 and zeros where fewer candidates exist)."""
        return self._score_call("scs_score_clade_moves", sources, parent, taxon, (batch_trees, lds_bytes),
                                ((("cp_trees", "cp_total", "cp_source", "mv_own_super", "mv_own_shared"), _Q),
                                 (("mv_node",), _QK, np.int32, -1), (("mv_super", "mv_shared"), _QK)),
                                query_nodes, "query_nodes one per query clade", top_k)

    def score_polytomies(self, sources, parent: np.ndarray, taxon: np.ndarray, query_nodes, batch_trees: int = 0,
                         lds_bytes: int = 0) -> dict:
        """``scs_score_polytomies``: what the sources say about grouping the children of every query node, with the
        inputs of ``score`` and ``query_nodes`` = preorder indices of supertree nodes with 3 to 64 children, each once.
        Returns ``py_degree`` (int32) and ``py_trees`` (int64), one entry per query, and ``py_total``, ``py_joint``:
        lists with one int64 array k x k x k per query, entry [i][j][l] filled for i < j and l not in {i, j}.
        ``lds_bytes`` > 0 caps the LDS one workgroup of the sweep takes (tests)."""
        par = np.asarray(parent, dtype=np.int64)
        kids = np.bincount(par[1:], minlength=len(par)) if len(par) > 1 else np.zeros(len(par), dtype=np.int64)
        q = np.asarray(query_nodes, dtype=np.int64)
        ok = q.ndim == 1 and bool(np.all((q >= 0) & (q < len(par))))
        # (an out-of-range query has no size: one cell, and the library names the query in its message)
        cubes = kids[q] ** 3 if ok else np.ones(q.size, dtype=np.int64)
        out = self._score_call("scs_score_polytomies", sources, parent, taxon, (batch_trees, lds_bytes),
                               ((("py_degree",), _Q, np.int32, 0), (("py_trees",), _Q), (("py_total", "py_joint"), ("k3",))),
                               query_nodes, "query_nodes one per polytomy", sizes={"k3": int(cubes.sum())})
        ends = np.cumsum(cubes)
        for name in ("py_total", "py_joint"):
            out[name] = [out[name][e - c:e].reshape(int(k), int(k), int(k))
                         for e, c, k in zip(ends, cubes, out["py_degree"])]
        return out

    def score_parsimony(self, sources, parent: np.ndarray, taxon: np.ndarray, chars: bool = False,
                        batch_trees: int = 0, pass_words: int = 0, n_chars: int | None = None) -> dict:
        """``scs_score_parsimony``: the MRP parsimony scores, with the inputs of ``score``.  Returns int64 arrays
        ``mrp_chars``, ``mrp_length``, ``mrp_perfect``, ``mrp_max`` (per tree) and, with ``chars``, per character
        ``char_off`` (int64, trees + 1) and ``char_len``, ``char_lo``, ``char_hi`` (int32; None otherwise), sized by
        ``n_chars`` (the sum of ``n_source`` of ``score``) or, without it, by a first call.  ``pass_words`` > 0 lowers
        the 64-character words of a tree one pass covers (tests)."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        ints = (batch_trees, pass_words)
        per_tree = (("mrp_chars", "mrp_length", "mrp_perfect", "mrp_max"), _M)
        per_char = ("char_len", "char_lo", "char_hi")
        sizes = {"m1": tabs.n_trees + 1}
        if not chars or n_chars is None:
            out = self._score_call("scs_score_parsimony", tabs, parent, taxon, ints,
                                   (per_tree, (("char_off",), ("m1",) if chars else None), (per_char, None)), sizes=sizes)
            if not chars:
                return out
            n_chars = int(out["char_off"][-1])
        sizes["total"] = int(n_chars)
        return self._score_call("scs_score_parsimony", tabs, parent, taxon, ints,
                                (per_tree, (("char_off",), ("m1",)), (per_char, ("total",), np.int32, 0)), sizes=sizes)

    def score_source_pairs(self, sources, rows=None, batch_trees: int = 0, lds_bytes: int = 0,
                           outputs=("common", "clusters", "clusters_other", "shared")) -> dict:
        """``scs_score_source_pairs``: the Robinson-Foulds terms between every two source trees, each pair restricted
        to the taxa both hold.  ``sources`` as for ``score``; ``rows``: the tree ids of the rows wanted (any order,
        repeats allowed; None: every tree).  Returns int32 arrays ``common``, ``clusters``, ``clusters_other``,
        ``shared``, rows x trees (None for a name ``outputs`` leaves out).  ``batch_trees`` > 0 caps the trees of a row
        and of a column batch, ``lds_bytes`` > 0 the LDS of a pair workgroup (tests)."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        m = tabs.n_trees
        if rows is None:
            n_rows, row_ptr = m, None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.ndim != 1:
                msg = "rows must be a list of tree ids"
                raise ValueError(msg)
            n_rows, row_ptr = len(rows), nv.iptr(rows)
        names = ("common", "clusters", "clusters_other", "shared")
        out = {k: np.zeros((n_rows, m), dtype=np.int32) if k in outputs else None for k in names}
        rc = self._lib.scs_score_source_pairs(self._ctx, tabs._h, n_rows, row_ptr, int(batch_trees), int(lds_bytes),
                                              *(None if v is None else v.ctypes.data for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_score_source_pairs: invalid input")
        nv.check(rc)
        return out

    def score_source_pair_triplets(self, sources, rows=None, batch_trees: int = 0, lds_bytes: int = 0,
                                   chunk_pairs: int = 0,
                                   outputs=("common", "triplets", "triplets_other", "triplets_shared")) -> dict:
        """``scs_score_source_pair_triplets``: the rooted-triplet terms between every two source trees, each pair
        restricted to the taxa both hold.  ``sources`` and ``rows`` as for ``score_source_pairs``.  Returns ``common``
        (int32) and ``triplets``, ``triplets_other``, ``triplets_shared`` (int64), rows x trees (None for a name
        ``outputs`` leaves out).  ``batch_trees`` > 0 caps the trees of a row and of a column batch, ``lds_bytes`` > 0
        the LDS of a workgroup, ``chunk_pairs`` > 0 the pairs restricted at once (tests)."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        m = tabs.n_trees
        if rows is None:
            n_rows, row_ptr = m, None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.ndim != 1:
                msg = "rows must be a list of tree ids"
                raise ValueError(msg)
            n_rows, row_ptr = len(rows), nv.iptr(rows)
        names = ("common", "triplets", "triplets_other", "triplets_shared")
        out = {k: np.zeros((n_rows, m), dtype=np.int32 if k == "common" else np.int64) if k in outputs else None
               for k in names}
        rc = self._lib.scs_score_source_pair_triplets(self._ctx, tabs._h, n_rows, row_ptr, int(batch_trees),
                                                      int(lds_bytes), int(chunk_pairs),
                                                      *(None if v is None else v.ctypes.data for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_score_source_pair_triplets: invalid input")
        nv.check(rc)
        return out

    def score_coverage(self, sources, rows=None, min_trees: int = 1, pairs: bool = False, batch_rows: int = 0,
                       reg_words: int = 0, outputs=("occurs", "taxon_covered")) -> dict:
        """``scs_score_coverage``: the triple coverage of the sources.  ``sources`` as for ``score`` (only their trees'
        taxa are read); ``rows``: the taxon ids of the rows wanted (any order, repeats allowed; None: every taxon);
        a triple counts as covered when ``min_trees`` trees hold all three.  Returns ``occurs`` (int32, taxa),
        ``taxon_covered`` (int64, rows) and, with ``pairs``, ``pair_trees`` and ``pair_covered`` (int32, rows x taxa;
        None otherwise) -- ``outputs`` names the ones wanted beside the matrices, the others are None.
        ``batch_rows`` > 0 caps a row batch, ``reg_words`` > 0 the words of a membership row a lane holds in registers
        (tests).  The cost is O(rows x taxa^2 x ceil(trees / 32))."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        n = tabs.n_taxa
        if rows is None:
            n_rows, row_ptr = n, None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.ndim != 1:
                msg = "rows must be a list of taxon ids"
                raise ValueError(msg)
            n_rows, row_ptr = len(rows), nv.iptr(rows)
        want = set(outputs) | ({"pair_trees", "pair_covered"} if pairs else set())
        shapes = {"occurs": ((n,), np.int32), "pair_trees": ((n_rows, n), np.int32),
                  "pair_covered": ((n_rows, n), np.int32), "taxon_covered": ((n_rows,), np.int64)}
        out = {k: np.zeros(shape, dtype=dt) if k in want else None for k, (shape, dt) in shapes.items()}
        rc = self._lib.scs_score_coverage(self._ctx, tabs._h, n_rows, row_ptr, int(min_trees), int(batch_rows),
                                          int(reg_words), *(None if v is None else v.ctypes.data for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_score_coverage: invalid input")
        nv.check(rc)
        return out

    INTERNODE_OUTPUTS = ("pair_weight", "dist_sum", "sq_sum", "taxon_weight", "taxon_sum", "taxon_sq",
                         "taxon_partners")

    def score_internode(self, sources, rows=None, tree_weights=None, matrices: bool = True, squares: bool = False,
                        batch_rows: int = 0, batch_trees: int = 0, outputs=None) -> dict:
        """``scs_score_internode``: the internode distances of the sources, summed per pair of taxa.  ``sources`` as
        for ``score`` (only their trees' taxa and ``adj_depth`` are read); ``rows``: the taxon ids of the rows wanted
        (any order, repeats allowed; None: every taxon); ``tree_weights``: non-negative integers per tree (None: 1).
        Returns ``pair_weight``, ``dist_sum``, ``sq_sum`` (int64, rows x taxa), ``taxon_weight``, ``taxon_sum``,
        ``taxon_sq`` (int64, rows) and ``taxon_partners`` (int32, rows).  ``outputs`` names the ones wanted (the
        others are None); by default all but the matrices without ``matrices`` and the squared ones without
        ``squares``.  ``batch_rows`` / ``batch_trees`` > 0 cap a row / tree batch (tests)."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        n = tabs.n_taxa
        if rows is None:
            n_rows, row_ptr = n, None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.ndim != 1:
                msg = "rows must be a list of taxon ids"
                raise ValueError(msg)
            n_rows, row_ptr = len(rows), nv.iptr(rows)
        w_ptr = None
        if tree_weights is not None:
            tree_weights = np.ascontiguousarray(tree_weights, dtype=np.int64)
            if tree_weights.shape != (tabs.n_trees,):
                msg = f"tree_weights must hold one weight per tree ({tabs.n_trees}), not {tree_weights.shape}"
                raise ValueError(msg)
            w_ptr = nv.lptr(tree_weights)
        if outputs is None:
            outputs = [k for k in self.INTERNODE_OUTPUTS
                       if (matrices or k.startswith("taxon")) and (squares or k not in ("sq_sum", "taxon_sq"))]
        unknown = set(outputs) - set(self.INTERNODE_OUTPUTS)
        if unknown:
            msg = f"unknown outputs {sorted(unknown)}"
            raise ValueError(msg)
        out = {}
        for k in self.INTERNODE_OUTPUTS:
            shape = (n_rows,) if k.startswith("taxon") else (n_rows, n)
            out[k] = np.zeros(shape, dtype=np.int32 if k == "taxon_partners" else np.int64) if k in outputs else None
        rc = self._lib.scs_score_internode(self._ctx, tabs._h, n_rows, row_ptr, w_ptr, int(batch_rows),
                                           int(batch_trees),
                                           *(None if v is None else v.ctypes.data for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_score_internode: invalid input")
        nv.check(rc)
        return out

    def debug_internode_depths(self, sources, batch_trees: int = 0) -> dict:
        """``scs_debug_internode_depths``: the depth pass of ``score_internode`` alone -- ``gap_r`` (r of the gap
        after every leaf; 0 at a tree's last leaf), ``leaf_depth`` (both int32 by global leaf index) and
        ``tree_height`` (int32 per tree), downloaded from the arrays the sweep reads."""
        tabs = self.upload(sources) if isinstance(sources, TreeTables) else sources
        four = np.zeros(4, dtype=np.int64)  # (n_taxa, n_trees, n_leaves, max_leaves as the handle holds them)
        nv.check(self._lib.scs_debug_tables_download(self._ctx, tabs._h, None, None, None, None, None, nv.lptr(four)))
        leaves = int(four[2])
        out = {"gap_r": np.zeros(leaves, dtype=np.int32), "leaf_depth": np.zeros(leaves, dtype=np.int32),
               "tree_height": np.zeros(tabs.n_trees, dtype=np.int32)}
        rc = self._lib.scs_debug_internode_depths(self._ctx, tabs._h, int(batch_trees),
                                                  *(nv.iptr(v) if len(v) else None for v in out.values()))
        if rc == nv.EINVAL:
            msg = self._lib.scs_last_error()
            raise ValueError(msg.decode() if msg else "scs_debug_internode_depths: invalid input")
        nv.check(rc)
        return out

    # -- batched small nodes --------------------------------------------------
    # largest node of the batched path (SMALL_MAXS of libscs_hip: two-sided Jacobi in LDS up to 64
    # vertices, one-sided up to 128 -- SURVEY.md 8f rank 3).  SCS_SMALL_MAX_TAXA moves the limit down.
    SMALL_MAX_TAXA = max(2, min(128, int(_env.probe("SCS_SMALL_MAX_TAXA", "128"))))

    def small_solve(self, nodes, want_w: bool = False):
        """K small recursion nodes in one launch (``scs_small_solve``; reference: scs.py:110-134
        at depth).  ``nodes``: list of ``(tables, group_start or None)`` with at most
        ``SMALL_MAX_TAXA`` taxa each, taxa numbered so that contraction groups are consecutive
        ranges.  Returns one ``(maps, lambdas)`` -- or ``(maps, lambdas, W)`` -- per node."""
        if len(nodes) == 0:
            return []
        return self.small_solve_begin(nodes, want_w).result()

    def small_solve_begin(self, nodes, want_w: bool = False) -> "SmallTicket":
        """The same, not waited for (``scs_small_solve_begin``): the returned ticket's
        ``result()`` is the list ``small_solve`` returns.  At least one node."""
        k = len(nodes)
        if k == 1 and getattr(nodes[0][0], "resident", None) is not None and _resident_solve():
            forest, relabel = nodes[0][0].resident
            if forest.dev is self and forest._h:
                # the node's tables are on this device already (a child of scs_forest_split): only the
                # group boundaries and the renumbering travel (scs_small_solve_begin_forest)
                tables, group_start = nodes[0]
                gs = (np.arange(tables.n_taxa + 1, dtype=np.int32) if group_start is None
                      else np.ascontiguousarray(group_start, dtype=np.int32))
                rl = None if relabel is None else np.ascontiguousarray(relabel, dtype=np.int32)
                ticket = C.c_int32(-1)
                nv.check(self._lib.scs_small_solve_begin_forest(
                    self._ctx, forest._h, nv.iptr(rl) if rl is not None else None, int(tables.n_taxa), len(gs) - 1,
                    nv.iptr(gs), int(want_w), C.byref(ticket)))
                return SmallTicket(self, ticket.value, np.asarray([len(gs) - 1], dtype=np.int32), want_w, list(nodes),
                                   # (a slice does not know its leaf count here: no counts, no read-back)
                                   None if getattr(forest, "_base", None) is not None
                                   else (forest.n_trees + 1, forest.n_leaves, forest.n_trees))
        n_taxa = np.empty(k, dtype=np.int32)
        n_trees = np.empty(k, dtype=np.int32)
        n_groups = np.empty(k, dtype=np.int32)
        toff, gstart, lt, ad, av, tw = [], [], [], [], [], []
        for i, (tables, group_start) in enumerate(nodes):
            n_taxa[i], n_trees[i] = tables.n_taxa, tables.n_trees
            gs = (np.arange(tables.n_taxa + 1, dtype=np.int32) if group_start is None
                  else np.ascontiguousarray(group_start, dtype=np.int32))
            n_groups[i] = len(gs) - 1
            toff.append(np.asarray(tables.tree_off, dtype=np.int32))
            gstart.append(gs)
            lt.append(tables.leaf_taxon)
            ad.append(tables.adj_depth)
            av.append(tables.adj_val)
            tw.append(tables.tree_w)
        if k == 1:
            cat = lambda parts: parts[0]  # noqa: E731
        else:
            cat = np.concatenate
        toff_a = np.ascontiguousarray(cat(toff), dtype=np.int32)
        gs_a = np.ascontiguousarray(cat(gstart), dtype=np.int32)
        lt_a = np.ascontiguousarray(cat(lt), dtype=np.int32)
        ad_a = np.ascontiguousarray(cat(ad), dtype=np.int32)
        av_a = np.ascontiguousarray(cat(av), dtype=np.float64)
        tw_a = np.ascontiguousarray(cat(tw), dtype=np.float64)
        ticket = C.c_int32(-1)
        nv.check(self._lib.scs_small_solve_begin(
            self._ctx, k, nv.iptr(n_taxa), nv.iptr(n_trees), nv.iptr(n_groups), nv.iptr(toff_a),
            nv.iptr(lt_a), nv.iptr(ad_a), nv.dptr(av_a), nv.dptr(tw_a), nv.iptr(gs_a), int(want_w),
            C.byref(ticket)))
        return SmallTicket(self, ticket.value, n_groups, want_w, list(nodes), (len(toff_a), len(lt_a), len(tw_a)))

    def small_solve_begin_level(self, forest: "DeviceForest", t_begin, n_trees, n_leaves, u_base, u_size, relabel,
                                n_taxa, n_groups, group_start, want_w: bool = False) -> "SmallTicket":
        """``scs_small_solve_begin_level``: the K small nodes of one level of the recursion from the level
        forest's resident tables (``levels.Engine``; reference: scs.py:110-134 for every node of the level).
        All arguments are arrays over the K nodes (``relabel`` / ``group_start`` concatenated).  ``want_w``: the
        ticket's ``result()`` carries every node's contracted W as well."""
        k = len(t_begin)
        as32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        t_begin, n_trees, u_base, u_size = as32(t_begin), as32(n_trees), as32(u_base), as32(u_size)
        relabel, n_taxa, n_groups, group_start = as32(relabel), as32(n_taxa), as32(n_groups), as32(group_start)
        n_leaves = np.ascontiguousarray(n_leaves, dtype=np.int64)
        ticket = C.c_int32(-1)
        nv.check(self._lib.scs_small_solve_begin_level(
            self._ctx, forest._h, k, nv.iptr(t_begin), nv.iptr(n_trees), nv.lptr(n_leaves), nv.iptr(u_base),
            nv.iptr(u_size), nv.iptr(relabel), nv.iptr(n_taxa), nv.iptr(n_groups), nv.iptr(group_start), int(want_w),
            C.byref(ticket)))
        return SmallTicket(self, ticket.value, n_groups, bool(want_w), None,
                           (int(n_trees.sum()) + k, int(n_leaves.sum()), int(n_trees.sum())))

    def debug_small_inputs(self, ticket: int, n_toff: int, n_leaf: int, n_tree: int):
        """``scs_debug_small_inputs`` of the begun batch ``ticket`` (``SmallTicket.debug_inputs``, which knows the
        counts: the library copies what the batch holds, whatever the buffers here are sized for)."""
        tree_off = np.full(int(n_toff), -1, dtype=np.int32)
        leaf_taxon = np.full(int(n_leaf), -1, dtype=np.int32)
        adj_depth = np.full(int(n_leaf), -1, dtype=np.int32)
        adj_val = np.full(int(n_leaf), np.nan)
        tree_w = np.full(int(n_tree), np.nan)
        nv.check(self._lib.scs_debug_small_inputs(self._ctx, int(ticket), nv.iptr(tree_off), nv.iptr(leaf_taxon),
                                                  nv.iptr(adj_depth), nv.dptr(adj_val), nv.dptr(tree_w)))
        return tree_off, leaf_taxon, adj_depth, adj_val, tree_w

    def upload_range(self, forest: "DeviceForest", t_begin: int, t_end: int, u_base: int, u_size: int,
                     relabel: np.ndarray, n_taxa: int, monotone: bool) -> "DeviceTables":
        """``scs_tables_from_forest_range``: the tables of ONE node of a level forest as a handle for
        ``build`` (the nodes of a level that are too large for the batched small path)."""
        handle = C.c_void_p()
        rl = np.ascontiguousarray(relabel, dtype=np.int32)
        nv.check(self._lib.scs_tables_from_forest_range(self._ctx, forest._h, int(t_begin), int(t_end), int(u_base),
                                                        int(u_size), nv.iptr(rl), int(n_taxa), C.byref(handle)))
        return DeviceTables(self, handle, int(n_taxa), int(t_end - t_begin), bool(monotone))

    def copy_bandwidth(self, nbytes: int = 1 << 30, reps: int = 6) -> float:
        """Measured device-to-device copy rate of this GPU in GB/s (read + write bytes over
        time; ``scs_debug_copy_bandwidth``) -- the figure to hold beside the nominal HBM peak."""
        out = C.c_double(0.0)
        nv.check(self._lib.scs_debug_copy_bandwidth(self._ctx, int(nbytes), int(reps), C.byref(out)))
        return float(out.value)

    # -- building blocks exposed for the parity tests -----------------------
    def comm_selftest(self, x: np.ndarray) -> np.ndarray:
        """One grouped ncclSend/ncclRecv round to this rank itself plus an ncclAllGather,
        through the library's RCCL wrappers (``scs_debug_comm_selftest``); returns what came
        back.  The context must own an RCCL communicator (created with a unique id)."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.empty_like(x)
        nv.check(self._lib.scs_debug_comm_selftest(self._ctx, len(x), nv.dptr(x), nv.dptr(out)))
        return out


    def debug_jacobi(self, a: np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float64)
        n = a.shape[0]
        w = np.empty(n)
        v = np.empty((n, n))
        nv.check(self._lib.scs_debug_jacobi(self._ctx, nv.dptr(a), n, nv.dptr(w), nv.dptr(v)))
        return w, v

    def debug_gram(self, a: np.ndarray, b: np.ndarray, use_mfma: bool):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = np.empty((a.shape[1], b.shape[1]))
        nv.check(self._lib.scs_debug_gram(self._ctx, nv.dptr(a), nv.dptr(b), a.shape[0], a.shape[1],
                                          b.shape[1], int(use_mfma), nv.dptr(out)))
        return out

    def debug_gram_ex(self, a: np.ndarray, a_col0: int, ka: int, b: np.ndarray, b_col0: int, kb: int,
                      use_mfma: bool, gram_blocks: int = 256) -> np.ndarray:
        """``A^T B`` for column blocks of the row-major panels ``a`` and ``b`` (``scs_debug_gram_ex``);
        passing the same array twice makes it one device panel."""
        assert a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 2
        assert b.dtype == np.float64 and b.flags.c_contiguous and b.ndim == 2 and b.shape[0] == a.shape[0]
        out = np.empty((ka, kb))
        nv.check(self._lib.scs_debug_gram_ex(self._ctx, nv.dptr(a), a.shape[1], a_col0, ka, nv.dptr(b),
                                             b.shape[1], b_col0, kb, a.shape[0], int(use_mfma),
                                             int(gram_blocks), nv.dptr(out)))
        return out

    def debug_update(self, y: np.ndarray, y_col0: int, kc: int, alpha: float, a: np.ndarray, a_col0: int,
                     ka: int, c: np.ndarray, sign: float) -> None:
        """``y[:, y_col0:+kc] = alpha * y[:, y_col0:+kc] + sign * a[:, a_col0:+ka] @ c[:, :kc]`` in place on
        the host panel ``y`` through one launch of the update kernel (``scs_debug_update``); ``a is y``
        makes them one device panel."""
        for m in (y, a, c):
            assert m.dtype == np.float64 and m.flags.c_contiguous and m.ndim == 2
        assert a.shape[0] == y.shape[0] and c.shape[0] == ka
        nv.check(self._lib.scs_debug_update(self._ctx, nv.dptr(y), y.shape[1], y_col0, kc, float(alpha),
                                            nv.dptr(a), a.shape[1], a_col0, ka, nv.dptr(c), c.shape[1],
                                            float(sign), y.shape[0]))

    def debug_small_svqb(self, g: np.ndarray, drop_tol: float):
        """One ``k_small_svqb`` launch on ``g`` (k x k): ``(t, mask)`` (``scs_debug_small_svqb``)."""
        assert g.dtype == np.float64 and g.flags.c_contiguous and g.ndim == 2 and g.shape[0] == g.shape[1]
        k = g.shape[0]
        t = np.empty((k, k))
        mask = np.empty(k, dtype=np.int32)
        nv.check(self._lib.scs_debug_small_svqb(self._ctx, nv.dptr(g), k, float(drop_tol), nv.dptr(t), nv.iptr(mask)))
        return t, mask

    def debug_small_rr(self, tm: np.ndarray, nq: int, b: int, mask, drop_tol: float, exact_from: int = -1,
                       start: int = 0):
        """The Rayleigh-Ritz solve through the product kernels (``scs_debug_small_rr``): ``tm`` is nq x nq, or
        nparts x nq x nq partials that the kernel sums.  ``(c, d, theta, mask_p, mask48)``."""
        assert tm.dtype == np.float64 and tm.flags.c_contiguous and tm.shape[-2:] == (nq, nq)
        nparts = tm.shape[0] if tm.ndim == 3 else 0
        c, d = np.empty((nq, b)), np.empty((nq, b))
        theta = np.empty(b + 1)
        mask_p, mask48 = np.empty(b, dtype=np.int32), np.empty(48, dtype=np.int32)
        mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        assert mk is None or mk.shape == (nq,)
        nv.check(self._lib.scs_debug_small_rr(self._ctx, nv.dptr(tm), nparts, nq, b, None if mk is None else nv.iptr(mk),
                                              float(drop_tol), int(exact_from), int(start), nv.dptr(c), nv.dptr(d),
                                              nv.dptr(theta), nv.iptr(mask_p), nv.iptr(mask48)))
        return c, d, theta, mask_p, mask48

    def debug_small_orth(self, partial: np.ndarray, b: int, drop_tol: float, theta: np.ndarray, layout: int = 0):
        """The projected SVQB on ``partial`` (nparts x (3 b^2 + b)) (``scs_debug_small_orth``): ``(coef, mask,
        report)``; ``layout`` 1 runs it on the compact working set of one width."""
        assert partial.dtype == np.float64 and partial.flags.c_contiguous and partial.ndim == 2
        assert partial.shape[1] == 3 * b * b + b and theta.dtype == np.float64 and theta.shape == (b + 1,)
        coef = np.empty((3 * b + 4, b))
        mask = np.empty(b, dtype=np.int32)
        report = np.empty(41)
        nv.check(self._lib.scs_debug_small_orth(self._ctx, nv.dptr(partial), partial.shape[0], b, float(drop_tol),
                                                nv.dptr(theta), int(layout), nv.dptr(coef), nv.iptr(mask),
                                                nv.dptr(report)))
        return coef, mask, report

    PANEL_PAD = 16  # SCS_DEBUG_PANEL_PAD: rows the panels of debug_panel carry past n

    def debug_panel(self, which: int, b: int, n: int, q: np.ndarray, aq: np.ndarray, u=None, coef_a=None,
                    coef_b=None, theta=None, dinv=None, ypart=None, nseg: int = 0, blocks: int = 1, zt=None):
        """One launch of one tall kernel of the loop on the panels ``q``, ``aq`` ((n + PANEL_PAD) x 3b)
        (``scs_debug_panel``; ``which`` as the header lists them): ``(q_out, aq_out, partials)``; ``zt`` (kernel 2)
        is updated in place."""
        rows = n + self.PANEL_PAD
        for m in (q, aq):
            assert m.dtype == np.float64 and m.flags.c_contiguous and m.shape == (rows, 3 * b)
        for m in (u, dinv):
            assert m is None or (m.dtype == np.float64 and m.flags.c_contiguous and m.shape == (rows,))
        for m in (coef_a, coef_b):
            assert m is None or (m.dtype == np.float64 and m.flags.c_contiguous
                                 and m.shape == ((3 * b + 4 if which in (1, 2) else 3 * b), b))
        assert theta is None or (theta.dtype == np.float64 and theta.flags.c_contiguous and len(theta) >= b)
        assert ypart is None or (ypart.dtype == np.float64 and ypart.flags.c_contiguous
                                 and ypart.size == (nseg * n + self.PANEL_PAD) * b)
        assert zt is None or (zt.dtype == np.float64 and zt.flags.c_contiguous and zt.shape == (b, rows))
        nb = (n + 15) // 16 if which == 5 else ((n + 255) // 256 if which == 6 else blocks)
        nper = 3 * b * b + b if which <= 1 else (b if which == 6 else 9 * b * b)
        part = np.empty((nb, nper))
        q_out, aq_out = np.empty_like(q), np.empty_like(aq)
        ptr = lambda m: None if m is None else nv.dptr(m)  # noqa: E731
        nv.check(self._lib.scs_debug_panel(self._ctx, int(which), b, n, nv.dptr(q), nv.dptr(aq), ptr(u), ptr(coef_a),
                                           ptr(coef_b), ptr(theta), ptr(dinv), ptr(ypart), int(nseg), int(blocks),
                                           nv.dptr(q_out), nv.dptr(aq_out), nv.dptr(part), ptr(zt)))
        return q_out, aq_out, part

    def debug_scan(self, op: int, rows: np.ndarray) -> np.ndarray:
        """The exclusive scan of every row of ``rows`` (int32 ``[n_parts, n]``; ``op`` 0 sum, 1 max) through the
        multi-block scan of the forest split (``scs_debug_scan``): ``[n_parts, n + 1]``, the last entry the total."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        assert rows.ndim == 2
        out = np.empty((rows.shape[0], rows.shape[1] + 1), dtype=np.int32)
        nv.check(self._lib.scs_debug_scan(self._ctx, int(op), rows.shape[0], rows.shape[1], nv.iptr(rows), nv.iptr(out)))
        return out

    def debug_score_plan(self, sources, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0,
                         extra_per_tree: int = 0) -> dict:
        """``debug_score_plan`` (below) for tables on this device."""
        return debug_score_plan(sources, super_leaves, batch_trees, extra_per_leaf, extra_per_tree)

    def debug_branch_plan(self, sources, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0,
                          extra_per_tree: int = 0, lds_bytes: int = 0) -> dict:
        """``debug_branch_plan`` (below) for tables on this device."""
        return debug_branch_plan(sources, super_leaves, batch_trees, extra_per_leaf, extra_per_tree, lds_bytes)

    def debug_placement_plan(self, sources, super_leaves: int, batch_trees: int = 0, lds_bytes: int = 0,
                             n_queries: int = 1, n_sub_queries: int = 1, degrees=()) -> dict:
        """``debug_placement_plan`` (below) for tables on this device."""
        return debug_placement_plan(sources, super_leaves, batch_trees, lds_bytes, n_queries, n_sub_queries, degrees)


class DeviceForest:
    """A source forest resident in HBM (``scs_forest``): preorder node arrays, and -- for the
    children of ``split`` -- their flattened tables.  See ``treearrays.ResidentArrays``."""

    def __init__(self, dev: Device, handle, n_taxa: int, n_trees: int, n_nodes: int, n_leaves: int,
                 monotone_flag: bool = True) -> None:
        self.dev, self._h = dev, handle
        self.n_taxa, self.n_trees, self.n_nodes, self.n_leaves = n_taxa, n_trees, n_nodes, n_leaves
        self.monotone_flag = monotone_flag

    @classmethod
    def upload(cls, dev: Device, n_taxa, node_off, parent, taxon, length, support, weights, n_leaves) -> "DeviceForest":
        handle = C.c_void_p()
        nv.check(dev._lib.scs_forest_upload(dev._ctx, int(n_taxa), len(weights), nv.lptr(node_off), nv.iptr(parent),
                                            nv.iptr(taxon), nv.dptr(length), nv.dptr(support), nv.dptr(weights),
                                            int(n_leaves), C.byref(handle)))
        return cls(dev, handle, int(n_taxa), len(weights), int(node_off[-1]), int(n_leaves))

    def free(self) -> None:
        if self._h:
            self.dev._lib.scs_forest_free(self.dev._ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            if self.dev._ctx:
                self.free()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def split(self, part_of: np.ndarray, new_id: np.ndarray, part_taxa, strategy_code: int) -> list["DeviceForest"]:
        """``scs_forest_split``: one child per part, each with its tables (reference: scs.py:411-455)."""
        n_parts = len(part_taxa)
        handles = (C.c_void_p * n_parts)()
        info = (nv.ForestInfo * n_parts)()
        pt = np.ascontiguousarray(part_taxa, dtype=np.int32)
        rc = self.dev._lib.scs_forest_split(self.dev._ctx, self._h, nv.iptr(part_of), nv.iptr(new_id), n_parts,
                                            nv.iptr(pt), int(strategy_code), handles, info)
        if rc == nv.EUNSUP:
            # the reference fails in ``length * tree_weight`` with a missing support (scs.py:656)
            msg = "unsupported operand type(s) for *: 'NoneType' and 'float'"
            raise TypeError(msg)
        nv.check(rc)
        return [DeviceForest(self.dev, C.c_void_p(handles[c]), int(pt[c]), int(info[c].n_trees), int(info[c].n_nodes),
                             int(info[c].n_leaves), bool(info[c].monotone)) for c in range(n_parts)]

    def split_level(self, part_of: np.ndarray, new_id: np.ndarray, n_parts: int, child_taxa: int, strategy_code: int,
                    node_tree_end: np.ndarray):
        """``scs_forest_split_level``: every node of a level (consecutive tree ranges of this forest, ``node_tree_end``)
        restricted to every one of its parts in ONE call (reference: scs.py:411-455 for every node of the level).
        Returns ``(union forest, child_trees [n_parts, K], child_leaves [n_parts, K], present, comp_root, sig)``."""
        k = len(node_tree_end)
        handle = C.c_void_p()
        info = nv.ForestInfo()
        nte = np.ascontiguousarray(node_tree_end, dtype=np.int32)
        child_trees = np.zeros((n_parts, k), dtype=np.int32)
        child_leaves = np.zeros((n_parts, k), dtype=np.int64)
        present = np.zeros(child_taxa, dtype=np.uint8)
        comp_root = np.zeros(child_taxa, dtype=np.int32)
        sig = np.zeros((child_taxa, 2), dtype=np.uint64)
        rc = self.dev._lib.scs_forest_split_level(
            self.dev._ctx, self._h, nv.iptr(part_of), nv.iptr(new_id), int(n_parts), int(child_taxa),
            int(strategy_code), k, nv.iptr(nte), C.byref(handle), C.byref(info), nv.iptr(child_trees),
            nv.lptr(child_leaves), present.ctypes.data, nv.iptr(comp_root), sig.ctypes.data)
        if rc == nv.EUNSUP:
            # the reference fails in ``length * tree_weight`` with a missing support (scs.py:656)
            msg = "unsupported operand type(s) for *: 'NoneType' and 'float'"
            raise TypeError(msg)
        nv.check(rc)
        union = DeviceForest(self.dev, handle, int(child_taxa), int(info.n_trees), int(info.n_nodes),
                             int(info.n_leaves), bool(info.monotone))
        return union, child_trees, child_leaves, present, comp_root, sig

    def slice(self, t_begin: int, t_end: int) -> "DeviceForest":
        """``scs_forest_slice``: the trees [t_begin, t_end) as a forest of their own, nothing copied (taxon ids stay
        this forest's)."""
        handle = C.c_void_p()
        nv.check(self.dev._lib.scs_forest_slice(self.dev._ctx, self._h, int(t_begin), int(t_end), C.byref(handle)))
        out = DeviceForest(self.dev, handle, self.n_taxa, int(t_end - t_begin), 0, 0, self.monotone_flag)
        out._base = self  # (the slice points into this forest's arrays)
        return out

    def analyze(self):
        """``scs_forest_analyze``: ``(comp_root [n_taxa], sig [n_taxa, 2])`` of a forest that carries tables."""
        comp_root = np.zeros(max(self.n_taxa, 1), dtype=np.int32)
        sig = np.zeros((max(self.n_taxa, 1), 2), dtype=np.uint64)
        nv.check(self.dev._lib.scs_forest_analyze(self.dev._ctx, self._h, nv.iptr(comp_root), sig.ctypes.data))
        return comp_root, sig

    def tables_range(self, t_begin: int, t_end: int):
        """``(tree_off, leaf_taxon, adj_depth, adj_val, tree_w)`` of the trees [t_begin, t_end) (host copies)."""
        m = int(t_end - t_begin)
        tree_off = np.zeros(m + 1, dtype=np.int64)
        nv.check(self.dev._lib.scs_forest_tables_download_range(self.dev._ctx, self._h, int(t_begin), int(t_end),
                                                                nv.lptr(tree_off), None, None, None, None))
        l = int(tree_off[-1])
        leaf_taxon = np.empty(l, dtype=np.int32)
        adj_depth = np.empty(l, dtype=np.int32)
        adj_val = np.empty(l, dtype=np.float64)
        tree_w = np.empty(m, dtype=np.float64)
        nv.check(self.dev._lib.scs_forest_tables_download_range(
            self.dev._ctx, self._h, int(t_begin), int(t_end), nv.lptr(tree_off), nv.iptr(leaf_taxon) if l else None,
            nv.iptr(adj_depth) if l else None, nv.dptr(adj_val) if l else None, nv.dptr(tree_w) if m else None))
        return tree_off, leaf_taxon, adj_depth, adj_val, tree_w

    def tables(self):
        """``(tree_off, leaf_taxon, adj_depth, adj_val, tree_index, tree_w, present)`` of a child of
        ``split``: read-only views of the page-locked host copy the split left (no further copy; the
        views keep this forest -- and with it the block -- alive)."""
        m, l = self.n_trees, self.n_leaves
        ptrs = [C.c_void_p() for _ in range(7)]
        nv.check(self.dev._lib.scs_forest_tables_host(self.dev._ctx, self._h, *[C.byref(x) for x in ptrs]))

        def view(ptr, dtype, count):
            dt = np.dtype(dtype)
            if count == 0:
                return np.empty(0, dtype=dt)
            buf = (C.c_char * (count * dt.itemsize)).from_address(ptr.value)
            buf._scs_owner = self
            a = np.frombuffer(buf, dtype=dt, count=count)
            a.flags.writeable = False
            return a

        return (view(ptrs[0], np.int64, m + 1), view(ptrs[1], np.int32, l), view(ptrs[2], np.int32, l),
                view(ptrs[3], np.float64, l), view(ptrs[4], np.int32, m), view(ptrs[5], np.float64, m),
                view(ptrs[6], np.uint8, max(self.n_taxa, 0)))

    def download(self, t_begin: int = 0, t_end: int | None = None):
        """Node arrays of the trees ``[t_begin, t_end)``: ``(node_off, parent, taxon, length, support, weights)``."""
        t_end = self.n_trees if t_end is None else t_end
        m = t_end - t_begin
        node_off = np.zeros(m + 1, dtype=np.int64)
        # (sizes are known only after the offsets arrive: two calls)
        nv.check(self.dev._lib.scs_forest_download(self.dev._ctx, self._h, t_begin, t_end, nv.lptr(node_off),
                                                   None, None, None, None, None))
        n = int(node_off[-1])
        parent = np.empty(n, dtype=np.int32)
        taxon = np.empty(n, dtype=np.int32)
        length = np.empty(n, dtype=np.float64)
        support = np.empty(n, dtype=np.float64)
        weights = np.empty(m, dtype=np.float64)
        nv.check(self.dev._lib.scs_forest_download(self.dev._ctx, self._h, t_begin, t_end, nv.lptr(node_off),
                                                   nv.iptr(parent) if n else None, nv.iptr(taxon) if n else None,
                                                   nv.dptr(length) if n else None, nv.dptr(support) if n else None,
                                                   nv.dptr(weights) if m else None))
        return node_off, parent, taxon, length, support, weights


def debug_split_plan(node_off: np.ndarray):
    """``scs_debug_split_plan``: ``(trees per workgroup, staged [workgroups] bool)`` of the thread-per-tree split
    kernels for a forest's offsets -- the launcher's rule and the kernels' predicate, evaluated on the host."""
    node_off = np.ascontiguousarray(node_off, dtype=np.int64)
    m = len(node_off) - 1
    tpb, groups = C.c_int32(0), C.c_int32(0)
    staged = np.zeros((m + 7) // 8 + 1, dtype=np.uint8)
    nv.check(nv.load_library().scs_debug_split_plan(m, nv.lptr(node_off), C.byref(tpb), C.byref(groups), staged.ctypes.data))
    return int(tpb.value), staged[: groups.value].astype(bool)


def debug_score_plan(sources, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0,
                     extra_per_tree: int = 0) -> dict:
    """``scs_debug_score_plan``: the batches a ``scs_score_*`` export makes of ``sources`` (``DeviceTables``, or the
    ``tree_off`` array of tables that need not be on a device) for a supertree of ``super_leaves`` tips, and the pair
    kernel's plan per batch -- ``bstart`` (the first tree of every batch, then the tree count), ``levels``,
    ``row_stride``, and per batch ``words``, ``zb``, ``workgroups``.  The library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    nb = C.c_int32(0)
    bstart = np.zeros(m + 1, dtype=np.int32)
    info = np.zeros(2, dtype=np.int64)
    words, zb = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32)
    wg = np.zeros(max(m, 1), dtype=np.int64)
    nv.check(nv.load_library().scs_debug_score_plan(
        handle, m, None if off is None else nv.lptr(off), int(super_leaves), int(batch_trees), int(extra_per_leaf),
        int(extra_per_tree), C.byref(nb), nv.iptr(bstart), nv.lptr(info), nv.iptr(words), nv.iptr(zb), nv.lptr(wg)))
    k = int(nb.value)
    return {"bstart": bstart[: k + 1].astype(np.int64), "levels": int(info[0]), "row_stride": int(info[1]),
            "words": words[:k].astype(np.int64), "zb": zb[:k].astype(np.int64), "workgroups": wg[:k].copy()}


def debug_branch_plan(sources, super_leaves: int, batch_trees: int = 0, extra_per_leaf: int = 0,
                      extra_per_tree: int = 0, lds_bytes: int = 0) -> dict:
    """``scs_debug_branch_plan``: the plans of ``scs_score_branch_triplets`` / ``scs_score_branch_resample`` and of
    ``scs_score_taxon_triplets`` for ``sources`` (as for ``debug_score_plan``) -- ``bstart``; per batch ``bt_words``,
    ``bt_zb``, ``bt_lds``, ``bt_workgroups``; per batch and LDS bin ``tx_zb``, ``tx_dcap``, ``tx_lds``,
    ``tx_workgroups`` (batches x 3; ``tx_dcap`` 0: the bin is not launched); per batch ``tx_slab_launch`` and
    ``tx_slab_lds`` (the slab kernel's launch bytes); and once
    ``need_slab``, ``slab_wgs``, ``slab_stride``.  The library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    nb = C.c_int32(0)
    bstart = np.zeros(m + 1, dtype=np.int32)
    bt = np.zeros((max(m, 1), 4), dtype=np.int64)
    tx = np.zeros((max(m, 1), 14), dtype=np.int64)
    call = np.zeros(3, dtype=np.int64)
    nv.check(nv.load_library().scs_debug_branch_plan(
        handle, m, None if off is None else nv.lptr(off), int(super_leaves), int(batch_trees), int(extra_per_leaf),
        int(extra_per_tree), int(lds_bytes), C.byref(nb), nv.iptr(bstart), nv.lptr(bt), nv.lptr(tx), nv.lptr(call)))
    k = int(nb.value)
    bins = tx[:k, :12].reshape(k, 3, 4)
    return {"bstart": bstart[: k + 1].astype(np.int64), "bt_words": bt[:k, 0].copy(), "bt_zb": bt[:k, 1].copy(),
            "bt_lds": bt[:k, 2].copy(), "bt_workgroups": bt[:k, 3].copy(), "tx_zb": bins[:, :, 0].copy(),
            "tx_dcap": bins[:, :, 1].copy(), "tx_lds": bins[:, :, 2].copy(), "tx_workgroups": bins[:, :, 3].copy(),
            "tx_slab_launch": tx[:k, 12].copy(), "tx_slab_lds": tx[:k, 13].copy(), "need_slab": int(call[0]),
            "slab_wgs": int(call[1]),
            "slab_stride": int(call[2])}


def debug_placement_plan(sources, super_leaves: int, batch_trees: int = 0, lds_bytes: int = 0, n_queries: int = 1,
                         n_sub_queries: int = 1, degrees=()) -> dict:
    """``scs_debug_placement_plan``: the plans of ``scs_score_placements`` (``n_queries`` query taxa), of
    ``scs_score_clade_placements`` / ``scs_score_clade_moves`` (``n_sub_queries`` tips of all query clades) and of
    ``scs_score_polytomies`` (``degrees``: the children of every query node) for ``sources`` (as for
    ``debug_score_plan``) -- per export x in ``pl``, ``cp``, ``py`` the batches ``x_bstart`` under the export's own
    workspace bytes; for ``pl`` and ``cp`` per batch ``x_words``, ``x_zb``, ``x_sums``, ``x_lds_full``, ``x_lds_last``
    (the pair kernel's launch bytes for a full and for the last pass), ``x_workgroups``, and per tree ``x_blk`` (its
    workgroups); for ``py`` per batch and degree ``py_words``, ``py_stride``, ``py_acc_lds``, ``py_lds``.  The
    library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    deg = np.ascontiguousarray(degrees, dtype=np.int32)
    nb = np.zeros(3, dtype=np.int32)
    bstart = np.zeros((3, m + 1), dtype=np.int32)
    pair = np.zeros((2, max(m, 1), 6), dtype=np.int64)
    blk = np.zeros((2, m + 1), dtype=np.int64)
    py = np.zeros((max(m, 1), max(len(deg), 1), 4), dtype=np.int64)
    nv.check(nv.load_library().scs_debug_placement_plan(
        handle, m, None if off is None else nv.lptr(off), int(super_leaves), int(batch_trees), int(lds_bytes),
        int(n_queries), int(n_sub_queries), len(deg), nv.iptr(deg) if len(deg) else None, nv.iptr(nb),
        nv.iptr(bstart), nv.lptr(pair[0]), nv.lptr(pair[1]), nv.lptr(blk), nv.lptr(py)))
    out = {}
    for x, name in enumerate(("pl", "cp")):
        k = int(nb[x])
        out[f"{name}_bstart"] = bstart[x, : k + 1].astype(np.int64)
        for i, key in enumerate(("words", "zb", "sums", "lds_full", "lds_last", "workgroups")):
            out[f"{name}_{key}"] = pair[x, :k, i].copy()
        out[f"{name}_blk"] = np.diff(blk[x])
    k = int(nb[2])
    out["py_bstart"] = bstart[2, : k + 1].astype(np.int64)
    rows = py.reshape(-1)[: k * len(deg) * 4].reshape(k, len(deg), 4)
    for i, key in enumerate(("words", "stride", "acc_lds", "lds")):
        out[f"py_{key}"] = rows[:, :, i].copy()
    return out


def debug_parsimony_plan(sources, parent, chars=None, batch_trees: int = 0, pass_words: int = 0) -> dict:
    """``scs_debug_parsimony_plan``: the plan of ``scs_score_parsimony`` for ``sources`` (as for ``debug_score_plan``)
    whose trees have ``chars`` characters (None: leaves - 2 each) and the supertree ``parent`` -- ``bstart``; per batch
    ``passes`` and ``words``; once ``pass_words``, ``frame_depth``, ``counter_bits``, ``lds_bytes`` (of a fold
    workgroup; 0 with ``frames_in_block``), ``frames_in_block``, ``extra_per_leaf``, ``extra_per_tree``,
    ``super_tips``.  The library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    parent = np.ascontiguousarray(parent, dtype=np.int32)
    if chars is not None:
        chars = np.ascontiguousarray(chars, dtype=np.int64)
        if chars.shape != (m,):
            msg = f"chars must have one entry per source tree ({m}), not shape {chars.shape}"
            raise ValueError(msg)
    nb = C.c_int32(0)
    bstart = np.zeros(m + 1, dtype=np.int32)
    info = np.zeros(8, dtype=np.int64)
    rows = np.zeros((max(m, 1), 2), dtype=np.int64)
    nv.check(nv.load_library().scs_debug_parsimony_plan(
        handle, m, None if off is None else nv.lptr(off), None if chars is None else nv.lptr(chars), len(parent),
        nv.iptr(parent), int(batch_trees), int(pass_words), C.byref(nb), nv.iptr(bstart), nv.lptr(info),
        nv.lptr(rows)))
    k = int(nb.value)
    keys = ("pass_words", "frame_depth", "counter_bits", "lds_bytes", "frames_in_block", "extra_per_leaf",
            "extra_per_tree", "super_tips")
    return {"bstart": bstart[: k + 1].astype(np.int64), "passes": rows[:k, 0].copy(), "words": rows[:k, 1].copy(),
            **{key: int(info[i]) for i, key in enumerate(keys)}}


def debug_source_pairs_plan(sources, n_taxa: int = 0, n_rows: int | None = None, batch_trees: int = 0,
                            lds_bytes: int = 0) -> dict:
    """``scs_debug_source_pairs_plan``: the plan of ``scs_score_source_pairs`` for ``sources`` (as for
    ``debug_score_plan``; ``n_taxa`` is read with a ``tree_off`` array) and ``n_rows`` rows (None: every tree) --
    ``bstart`` (the batches, the same on both axes); per tile (row batch x column batch) ``width`` (bytes of a list
    entry), ``lds`` (dynamic LDS of the pair launch), ``slab`` (the tile also launches the slab kernel), ``need``
    (bytes of its largest pair), ``threads`` (of a pair workgroup), ``grid_limit`` (workgroups one launch may have)
    and ``rows_per_launch``; once ``levels``, ``row_stride``, ``slab_stride``, ``slab_wgs``, ``workspace`` (bytes of the
    call's block), ``lds_cap``.  The library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    lib = nv.load_library()
    nb = C.c_int32(0)
    bstart = np.zeros(m + 1, dtype=np.int32)
    info = np.zeros(6, dtype=np.int64)
    args = (handle, m, None if off is None else nv.lptr(off), int(n_taxa), m if n_rows is None else int(n_rows),
            int(batch_trees), int(lds_bytes), C.byref(nb), nv.iptr(bstart), nv.lptr(info))
    nv.check(lib.scs_debug_source_pairs_plan(*args, None))  # (the batches first: they size the tiles)
    k = int(nb.value)
    tiles = np.zeros((k, k, 7), dtype=np.int64)
    nv.check(lib.scs_debug_source_pairs_plan(*args, nv.lptr(tiles)))
    keys = ("levels", "row_stride", "slab_stride", "slab_wgs", "workspace", "lds_cap")
    return {"bstart": bstart[: k + 1].astype(np.int64), **{key: int(info[i]) for i, key in enumerate(keys)},
            "width": tiles[:, :, 0].copy(), "lds": tiles[:, :, 1].copy(), "slab": tiles[:, :, 2].copy(),
            "need": tiles[:, :, 3].copy(), "threads": tiles[:, :, 4].copy(), "grid_limit": tiles[:, :, 5].copy(),
            "rows_per_launch": tiles[:, :, 6].copy()}


def debug_source_pair_triplets_plan(sources, n_taxa: int = 0, rows=None, batch_trees: int = 0, lds_bytes: int = 0,
                                    chunk_pairs: int = 0) -> dict:
    """``scs_debug_source_pair_triplets_plan``: the plan of ``scs_score_source_pair_triplets`` for ``sources`` (as for
    ``debug_source_pairs_plan``) and ``rows`` (tree ids; None: every tree) -- ``bstart``; per tile (row batch x column
    batch; zeros: no launch) ``tile_rows``, ``max_common``, ``words``, ``zb``, ``lds_pairs``, ``lds_restrict``,
    ``slab``, ``need``, ``pair_bytes``, ``chunk_cap``, ``pairs``, ``n_chunks``; ``chunks``, one row per chunk in launch
    order: I, J, first pair, pairs, small pairs, mirrored pairs, sweep workgroups, rows; once ``levels``,
    ``row_stride``, ``lds_cap``, ``small_common``, ``workspace``, ``region_bytes``, ``grid_limit``.  The library's own
    arithmetic, on the host; ``ValueError`` for the sizes the export refuses."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
    lib = nv.load_library()
    nb = C.c_int32(0)
    bstart = np.zeros(m + 1, dtype=np.int32)
    info = np.zeros(8, dtype=np.int64)
    args = (handle, m, None if off is None else nv.lptr(off), int(n_taxa), m if rows is None else len(rows),
            None if rows is None else nv.iptr(rows), int(batch_trees), int(lds_bytes), int(chunk_pairs), C.byref(nb),
            nv.iptr(bstart), nv.lptr(info))
    rc = lib.scs_debug_source_pair_triplets_plan(*args, None, None)  # (the batches and the chunk count first)
    if rc == nv.EINVAL:
        raise ValueError(lib.scs_last_error().decode())
    nv.check(rc)
    k = int(nb.value)
    tiles = np.zeros((k, k, 12), dtype=np.int64)
    chunks = np.zeros((int(info[7]), 8), dtype=np.int64)
    nv.check(lib.scs_debug_source_pair_triplets_plan(*args, nv.lptr(tiles), nv.lptr(chunks)))
    keys = ("levels", "row_stride", "lds_cap", "small_common", "workspace", "region_bytes", "grid_limit")
    names = ("tile_rows", "max_common", "words", "zb", "lds_pairs", "lds_restrict", "slab", "need", "pair_bytes",
             "chunk_cap", "pairs", "n_chunks")
    return {"bstart": bstart[: k + 1].astype(np.int64), **{key: int(info[i]) for i, key in enumerate(keys)},
            **{name: tiles[:, :, i].copy() for i, name in enumerate(names)}, "chunks": chunks}


def debug_coverage_plan(sources, n_taxa: int = 0, n_rows: int | None = None, min_trees: int = 1, batch_rows: int = 0,
                        reg_words: int = 0, matrices: int = 0) -> dict:
    """``scs_debug_coverage_plan``: the plan of ``scs_score_coverage`` for ``sources`` (device tables, or the number
    of trees with ``n_taxa``), ``n_rows`` rows (None: rows None, every taxon) and ``matrices`` of the two matrices
    wanted -- once ``words`` (per taxon), ``variant`` (words a lane holds in registers; 0: the streaming kernel),
    ``bits_stride``, ``taxa_stride``, ``tiles`` (workgroups of a row), ``row_bytes``, ``fixed_bytes``, ``n_batches``,
    ``grid_limit``, ``rows_per_launch``, ``mirror``, ``count`` (``min_trees`` > 1); per batch ``first_row``, ``rows``,
    ``bytes`` (of the call's block) and ``grid`` (workgroups of its first launch).  The library's own arithmetic, on
    the host."""
    handle, m = (sources._h, sources.n_trees) if isinstance(sources, DeviceTables) else (None, int(sources))
    lib = nv.load_library()
    info = np.zeros(12, dtype=np.int64)
    args = (handle, m, None, int(n_taxa), -1 if n_rows is None else int(n_rows), int(min_trees), int(batch_rows),
            int(reg_words), int(matrices), nv.lptr(info))
    nv.check(lib.scs_debug_coverage_plan(*args, None))  # (the number of batches first)
    batches = np.zeros((int(info[7]), 4), dtype=np.int64)
    nv.check(lib.scs_debug_coverage_plan(*args, nv.lptr(batches) if len(batches) else None))
    keys = ("words", "variant", "bits_stride", "taxa_stride", "tiles", "row_bytes", "fixed_bytes", "n_batches",
            "grid_limit", "rows_per_launch", "mirror", "count")
    return {**{key: int(info[i]) for i, key in enumerate(keys)}, "first_row": batches[:, 0].copy(),
            "rows": batches[:, 1].copy(), "bytes": batches[:, 2].copy(), "grid": batches[:, 3].copy()}


def debug_internode_plan(sources, n_taxa: int = 0, n_rows: int | None = None, batch_rows: int = 0,
                         batch_trees: int = 0, matrices: int = 0, tree_weights=None, heights=None,
                         squares: bool = False) -> dict:
    """``scs_debug_internode_plan``: the plan of ``scs_score_internode`` for ``sources`` (device tables, or a
    ``tree_off`` array with ``n_taxa``), ``n_rows`` rows (None: rows None, every taxon) and ``matrices`` of the three
    matrices wanted -- once ``levels``, ``width`` (bytes of an entry of the depth table), ``words``, ``taxa_stride``,
    ``tiles``, ``tiles_per_item``, ``items_per_row``, ``row_bytes``, ``batch_rows``, ``fixed_bytes`` (the block without
    matrices), ``bytes`` (with them), ``n_row_batches``, ``n_tree_batches``, ``grid_limit``, ``rows_per_launch``,
    ``mirror``; per row batch ``first_row``, ``rows``, ``grid``; per tree batch ``first_tree``, ``trees``, ``leaves``.
    With ``heights`` (h_t per tree) the export's overflow rule is applied to them and ``tree_weights`` (None: 1),
    with B2 when ``squares``: ``ValueError`` with the library's message.  The library's own arithmetic, on the host."""
    handle, off = (sources._h, None) if isinstance(sources, DeviceTables) else (None, sources)
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    m = sources.n_trees if off is None else len(off) - 1
    if tree_weights is not None:
        tree_weights = np.ascontiguousarray(tree_weights, dtype=np.int64)
    if heights is not None:
        heights = np.ascontiguousarray(heights, dtype=np.int32)
    lib = nv.load_library()
    info = np.zeros(16, dtype=np.int64)
    args = (handle, m, None if off is None else nv.lptr(off), int(n_taxa), -1 if n_rows is None else int(n_rows),
            int(batch_rows), int(batch_trees), int(matrices), None if tree_weights is None else nv.lptr(tree_weights))
    nv.check(lib.scs_debug_internode_plan(*args, None, 0, nv.lptr(info), None, None))  # (the batch counts first)
    rows_b = np.zeros((int(info[11]), 3), dtype=np.int64)
    trees_b = np.zeros((int(info[12]), 3), dtype=np.int64)
    rc = lib.scs_debug_internode_plan(*args, None if heights is None else nv.iptr(heights), int(bool(squares)),
                                      nv.lptr(info), nv.lptr(rows_b) if len(rows_b) else None,
                                      nv.lptr(trees_b) if len(trees_b) else None)
    if rc == nv.EINVAL:
        raise ValueError(lib.scs_last_error().decode())
    nv.check(rc)
    keys = ("levels", "width", "words", "taxa_stride", "tiles", "tiles_per_item", "items_per_row", "row_bytes",
            "batch_rows", "fixed_bytes", "bytes", "n_row_batches", "n_tree_batches", "grid_limit", "rows_per_launch",
            "mirror")
    return {**{key: int(info[i]) for i, key in enumerate(keys)}, "first_row": rows_b[:, 0].copy(),
            "rows": rows_b[:, 1].copy(), "grid": rows_b[:, 2].copy(), "first_tree": trees_b[:, 0].copy(),
            "trees": trees_b[:, 1].copy(), "leaves": trees_b[:, 2].copy()}


# A module attribute only a test sets (never the environment: ADVICE r05): the batched path then reports the nodes of
# more than 64 vertices as unconverged, and the per-node general path below takes them.
_FAIL_SMALL_FOR_TESTS = False


def _refuse_nonfinite_maps(maps: np.ndarray, lam: np.ndarray, n_groups: np.ndarray) -> None:
    """A node whose embedding holds a NaN or an infinity is a failed node whatever its eigenvalues say: its
    ``lambda`` row becomes NaN, the one sign of failure every caller looks at.  No such embedding may reach k-means."""
    if np.isfinite(maps).all():
        return
    at = 0
    for i, v in enumerate(n_groups):
        if not np.isfinite(maps[at:at + int(v)]).all():
            lam[i] = np.nan
        at += int(v)


class SmallTicket:
    """An ``scs_small_solve_begin`` that has not been ended: ``result()`` waits and returns one
    ``(maps, lambdas[, W])`` per node (once; kept).  Dropped unasked-for, it releases its slot."""

    def __init__(self, dev: Device, ticket: int, n_groups: np.ndarray, want_w: bool, nodes=None, counts=None) -> None:
        self.dev, self._ticket, self._n_groups, self._want_w = dev, ticket, n_groups, want_w
        self._nodes = nodes
        self._counts = counts  # (offset entries, leaves, trees) of the batch's packed input arrays
        self._out = None

    def _general_path(self, i: int):
        """Node ``i`` once more through the general per-node path (upload, build, contract, LOBPCG
        with an explicit block width -- which keeps scs_fiedler off the dense one-sided solve that
        has just failed): ``(maps, lambdas, W or None)``.  Raises RuntimeError if that fails too."""
        tables, group_start = self._nodes[i]
        dtab = self.dev.upload(tables)
        try:
            graph = dtab.build()
        finally:
            dtab.free()
        try:
            if group_start is not None:
                graph = graph.contract(group_start)
            last = None
            # (a graph too small for an explicit block width -- a 65..128-taxon node may contract to a handful of
            # vertices -- takes the library's default path: ADVICE r05)
            widths = [(b, it) for b, it in ((4, DEFAULT_MAX_ITER), (8, 4 * DEFAULT_MAX_ITER)) if graph.shape[0] > 3 * b + 2]
            for block, iters in widths or [(0, 4 * DEFAULT_MAX_ITER)]:
                try:
                    maps, stats = graph.fiedler(None, block=block, max_iter=iters)
                    lam = np.array([stats["lambda"][0], stats["lambda"][1], stats["lambda_next"]])
                    return maps, lam, (graph.download() if self._want_w else None)
                except nv.ConvergenceError as exc:
                    last = exc
            msg = f"small-node eigen-solve did not converge, nor did the general path ({last})"
            raise RuntimeError(msg)
        finally:
            graph.free()

    def debug_inputs(self):
        """``scs_debug_small_inputs``: ``(tree_off, leaf_taxon, adj_depth, adj_val, tree_w)`` of this batch as its
        first kernel reads them from the device block -- trees + 1 over the nodes, leaves, leaves, leaves and trees
        entries, the counts the batch was begun with.  Waits for the batch; the ticket stays begun."""
        if self._counts is None:
            msg = "this batch's array sizes are not known here"
            raise ValueError(msg)
        return self.dev.debug_small_inputs(self._ticket, *self._counts)

    def raw(self):
        """Waits and returns ``(maps [sum n_groups, 2], lambdas [K, 3])``, nothing re-solved: a node whose one-sided
        Jacobi ran out of sweeps carries NaN eigenvalues from the library, and one whose embedding is not finite is
        given them here (``_refuse_nonfinite_maps``); the caller decides what to do with such a node."""
        n_groups = self._n_groups
        maps = np.empty((int(n_groups.sum()), 2))
        lam = np.empty((len(n_groups), 3))
        ticket, self._ticket = self._ticket, -1
        nv.check(self.dev._lib.scs_small_solve_end(self.dev._ctx, ticket, nv.dptr(maps), nv.dptr(lam), None))
        _refuse_nonfinite_maps(maps, lam, n_groups)
        return maps, lam

    def result(self):
        if self._out is None:
            n_groups, want_w = self._n_groups, self._want_w
            k = len(n_groups)
            maps = np.empty((int(n_groups.sum()), 2))
            lam = np.empty((k, 3))
            w = np.empty(int((n_groups.astype(np.int64) ** 2).sum())) if want_w else None
            ticket, self._ticket = self._ticket, -1
            nv.check(self.dev._lib.scs_small_solve_end(self.dev._ctx, ticket, nv.dptr(maps), nv.dptr(lam),
                                                       nv.dptr(w) if want_w else None))
            redo = {}
            _refuse_nonfinite_maps(maps, lam, n_groups)
            if _FAIL_SMALL_FOR_TESTS:  # (tests/test_gpu_parity.py monkeypatches it: the one-sided Jacobi "gave up")
                lam[n_groups > 64] = np.nan
            if not np.all(np.isfinite(lam)):
                # the one-sided Jacobi of a node of more than 64 vertices ran out of sweeps (NaN
                # eigenvalues, never a half-rotated basis), or its embedding is not finite
                # (_refuse_nonfinite_maps): only THAT node goes through the general path again; if
                # that fails too the call raises, as the reference's ARPACK call raises rather than
                # return a guess (scs.py:252)
                bad = [i for i in range(k) if not np.all(np.isfinite(lam[i]))]
                if self._nodes is None:
                    msg = f"small-node eigen-solve did not converge (nodes {bad} of a batch of {k})"
                    raise RuntimeError(msg)
                for i in bad:
                    redo[i] = self._general_path(i)
            out, at, wat = [], 0, 0
            for i in range(k):
                v = int(n_groups[i])
                if i in redo:
                    item = (redo[i][0], redo[i][1]) + ((redo[i][2],) if want_w else ())
                else:
                    item = (maps[at:at + v], lam[i])
                    if want_w:
                        item += (w[wat:wat + v * v].reshape(v, v),)
                if want_w:
                    wat += v * v
                out.append(item)
                at += v
            self._nodes = None
            self._out = out
        return self._out

    def __del__(self) -> None:
        try:
            if self._ticket >= 0 and self.dev._ctx:
                self.dev._lib.scs_small_solve_end(self.dev._ctx, self._ticket, None, None, None)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class DeviceTables:
    def __init__(self, dev: Device, handle, n_taxa: int, n_trees: int, monotone: bool = False) -> None:
        self.dev, self._h = dev, handle
        self.n_taxa, self.n_trees = n_taxa, n_trees
        self.monotone = monotone

    def free(self) -> None:
        if self._h:
            self.dev._lib.scs_tables_free(self.dev._ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass

    def debug_download(self):
        """``scs_debug_tables_download``: ``(tree_off, leaf_taxon, adj_depth, adj_val, tree_w, info)`` -- host copies
        of the handle's five device arrays, ``info`` = ``{n_taxa, n_trees, n_leaves, max_leaves}`` as the handle
        holds them."""
        four = np.zeros(4, dtype=np.int64)
        nv.check(self.dev._lib.scs_debug_tables_download(self.dev._ctx, self._h, None, None, None, None, None,
                                                         nv.lptr(four)))
        m, l = int(four[1]), int(four[2])
        tree_off = np.full(m + 1, -1, dtype=np.int64)
        leaf_taxon = np.full(l, -1, dtype=np.int32)
        adj_depth = np.full(l, -1, dtype=np.int32)
        adj_val = np.full(l, np.nan)
        tree_w = np.full(m, np.nan)
        nv.check(self.dev._lib.scs_debug_tables_download(self.dev._ctx, self._h, nv.lptr(tree_off), nv.iptr(leaf_taxon),
                                                         nv.iptr(adj_depth), nv.dptr(adj_val), nv.dptr(tree_w),
                                                         nv.lptr(four)))
        info = dict(zip(("n_taxa", "n_trees", "n_leaves", "max_leaves"), (int(x) for x in four)))
        return tree_off, leaf_taxon, adj_depth, adj_val, tree_w, info

    def build(self, row_begin: int = 0, row_end: int | None = None,
              shared: bool | None = None, upper: bool = False, scatter: bool = False) -> "DeviceGraph":
        """Rows [row_begin, row_end) of W (reference: scs.py:495-663).

        ``shared`` (default: on whenever the device belongs to a multi-rank job) makes the
        call collective: the ranks split the upper-triangle tiles, exchange them and keep
        their own rows, so no cell is evaluated twice across the job.

        ``upper`` (multi-rank jobs, instead of ``shared``): every rank keeps only the tiles on
        and right of the diagonal of its own rows -- no exchange, half the memory, and the
        solve streams half the bytes (``SCS_BUILD_UPPER``; ``row_begin`` a multiple of 256, see
        ``partition.row_splits_upper``).  Not for nodes that contract.
        """
        if row_end is None:
            row_end = self.n_taxa
        handle = C.c_void_p()
        stats = nv.BuildStats()
        flags = nv.BUILD_MONOTONE if self.monotone else 0
        if upper:
            flags |= nv.BUILD_UPPER
            shared = False
        if scatter:  # the atomic-scatter comparison variant (measurements only)
            flags |= nv.BUILD_SCATTER
            shared = False
        if shared is None:
            shared = self.dev.world > 1
        if shared:
            flags |= nv.BUILD_SHARED
        nv.check(self.dev._lib.scs_pcg_build(self.dev._ctx, self._h, row_begin, row_end, flags,
                                             C.byref(handle), C.byref(stats)))
        graph = DeviceGraph(self.dev, handle, stats.as_dict())
        graph.upper = bool(upper)
        return graph

    def block_records(self, kind: str, t_begin: int = 0, t_end: int | None = None, row_begin: int = 0,
                      row_end: int | None = None) -> dict:
        """``scs_debug_block_records``: what the build's preparation leaves per (64-row block, tree) for the trees
        [t_begin, t_end) and the blocks of rows [row_begin, row_end), through the record kernel ``kind`` (``mono``,
        ``wide`` or ``general``).  Arrays of shape (blocks, trees, 64): ``spos`` the sorted DFS positions of the
        block's rows, ``gap`` the value of the shallowest gap between neighbours, ``argpos`` the position named for
        it, ``depth`` its depth (``general`` only, else None); ``cnt`` (blocks, trees) the rows present."""
        t_end = self.n_trees if t_end is None else t_end
        row_end = self.n_taxa if row_end is None else row_end
        code = {"mono": 0, "wide": 1, "general": 2}[kind]
        nb, nt = (max(row_end - row_begin, 0) + 63) // 64, max(t_end - t_begin, 0)
        spos = np.empty((nb, nt, 64), dtype=np.int32)
        gap = np.empty((nb, nt, 64), dtype=np.float64)
        argpos = np.empty((nb, nt, 64), dtype=np.int32)
        depth = np.empty((nb, nt, 64), dtype=np.int32) if code == 2 else None
        cnt = np.empty((nb, nt), dtype=np.int32)
        nv.check(self.dev._lib.scs_debug_block_records(
            self.dev._ctx, self._h, int(t_begin), int(t_end), int(row_begin), int(row_end), code, nv.iptr(spos),
            nv.dptr(gap), nv.iptr(argpos), nv.iptr(depth) if depth is not None else None, nv.iptr(cnt)))
        return {"spos": spos, "gap": gap, "argpos": argpos, "depth": depth, "cnt": cnt}


    def matrix_free_graph(self, max_block: int = 8) -> "DeviceGraph":
        """A graph WITHOUT its matrix (``scs_graph_matrix_free``): ``fiedler`` on it applies W straight
        from these tables -- a measured comparison (``tools/matrix_free_compare.py``), not the product
        path; the tables must outlive the graph; no ``download`` / ``contract``."""
        handle = C.c_void_p()
        nv.check(self.dev._lib.scs_graph_matrix_free(self.dev._ctx, self._h, int(max_block), C.byref(handle)))
        return DeviceGraph(self.dev, handle, {})


class DeviceGraph:
    def __init__(self, dev: Device, handle, build_stats: dict | None = None) -> None:
        self.dev, self._h = dev, handle
        self.build_stats = build_stats or {}
        self.upper = False  # an upper-triangle job (SCS_BUILD_UPPER): block widths 4 and 8 only

    def free(self) -> None:
        if self._h:
            self.dev._lib.scs_graph_free(self.dev._ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self) -> None:
        try:
            self.free()
        except Exception:  # noqa: BLE001
            pass

    @property
    def shape(self) -> tuple[int, int, int]:
        """(V, row_begin, row_end)."""
        n, rb, re_ = C.c_int32(), C.c_int32(), C.c_int32()
        nv.check(self.dev._lib.scs_graph_shape(self._h, C.byref(n), C.byref(rb), C.byref(re_)))
        return n.value, rb.value, re_.value

    def contract(self, group_start: np.ndarray) -> "DeviceGraph":
        """Merge consecutive index ranges (reference: scs.py:336-387); consumes self."""
        gs = np.ascontiguousarray(group_start, dtype=np.int32)
        handle = C.c_void_p()
        nv.check(self.dev._lib.scs_graph_contract(self.dev._ctx, self._h, nv.iptr(gs), len(gs) - 1,
                                                  C.byref(handle)))
        self._h = C.c_void_p()
        return DeviceGraph(self.dev, handle, self.build_stats)

    def download(self) -> np.ndarray:
        n, rb, re_ = self.shape
        out = np.empty((re_ - rb, n))
        nv.check(self.dev._lib.scs_graph_download(self.dev._ctx, self._h, nv.dptr(out)))
        return out

    def download_rows(self, first: int, count: int) -> np.ndarray:
        out = np.empty((count, self.shape[0]))
        nv.check(self.dev._lib.scs_graph_download_rows(self.dev._ctx, self._h, first, count,
                                                       nv.dptr(out)))
        return out

    def degrees(self) -> np.ndarray:
        n, rb, re_ = self.shape
        out = np.empty(re_ - rb)
        nv.check(self.dev._lib.scs_graph_degrees(self.dev._ctx, self._h, nv.dptr(out)))
        return out

    def apply(self, x: np.ndarray) -> np.ndarray:
        """One SYMM launch: rows of S @ x for this rank's row block (x: V x b)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, rb, re_ = self.shape
        y = np.empty((re_ - rb, x.shape[1]))
        nv.check(self.dev._lib.scs_debug_apply(self.dev._ctx, self._h, nv.dptr(x), x.shape[1],
                                               nv.dptr(y)))
        return y

    APPLY_INFO = ("symmetric", "image", "tiles", "segments", "tile_width", "n_apply32", "partial", "matrix_free")

    def apply_ex(self, x: np.ndarray, image: bool = False, reps: int = 1):
        """``reps`` consecutive SYMM applications by one solver object (``scs_debug_apply_ex``): the
        products (reps x rows x b) and a dict of what ran (``APPLY_INFO``)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        n, rb, re_ = self.shape
        y = np.empty((reps, re_ - rb, x.shape[1]))
        info = np.zeros(8, dtype=np.int32)
        nv.check(self.dev._lib.scs_debug_apply_ex(self.dev._ctx, self._h, nv.dptr(x), x.shape[1], int(image),
                                                  int(reps), nv.dptr(y), nv.iptr(info)))
        return y, dict(zip(self.APPLY_INFO, (int(v) for v in info)))

    TEAM_INFO = ("partial", "path", "world", "chunk", "segments", "tiles", "n_apply32", "n_allgather")

    def team_apply(self, q: np.ndarray, aq: np.ndarray, path: int = 0, image: bool = False, reps: int = 1):
        """``scs_debug_team_apply`` (collective: every rank, the same arguments): S applied ``reps`` times to the
        R block of the panel ``q`` (V x 3b) as a multi-rank solve assembles it -- ``path`` 0 ``solver::apply``, 1 the
        fused loop's back half.  Returns ``(y, qaq, part, info)``: AQ's R slot after every application (reps x V x b,
        all V rows as this rank holds them), Q^T AQ (reps x 3b x 3b; path 1, else None), this rank's own partial
        product (reps x V x b; upper-triangle graphs, else None) and a dict of what ran (``TEAM_INFO``)."""
        q = np.ascontiguousarray(q, dtype=np.float64)
        aq = np.ascontiguousarray(aq, dtype=np.float64)
        n = self.shape[0]
        if q.ndim != 2 or q.shape[0] != n or q.shape[1] % 3 or aq.shape != q.shape:
            msg = f"team_apply: q and aq must both have shape ({n}, 3b)"
            raise ValueError(msg)
        b = q.shape[1] // 3
        y = np.empty((reps, n, b))
        qaq = np.empty((reps, 3 * b, 3 * b)) if path == 1 else None
        part = np.empty((reps, n, b)) if self.upper else None
        info = np.zeros(8, dtype=np.int64)
        nv.check(self.dev._lib.scs_debug_team_apply(
            self.dev._ctx, self._h, nv.dptr(q), nv.dptr(aq), b, int(path), int(image), int(reps), nv.dptr(y),
            nv.dptr(qaq) if qaq is not None else None, nv.dptr(part) if part is not None else None, nv.lptr(info)))
        return y, qaq, part, dict(zip(self.TEAM_INFO, (int(v) for v in info)))

    def raw(self, what: int = 0):
        """``scs_debug_graph_raw``: the stored block with all ``ld`` columns -- ``what`` 0 the rows of W (float64),
        1 the single-precision image (float32; made by the solver's degree pass if missing) -- and a dict with
        ``rows``, ``ld``, ``col0`` and ``first_col`` (the first defined column of every row; all zero for W and for
        a row-partitioned rank's image).  ``ScsError`` with code ``EUNSUP`` where the library makes no image.  Mode 2
        of the entry has another shape: ``degrees_all``."""
        if what not in (0, 1):
            msg = f"DeviceGraph.raw: what must be 0 (W) or 1 (image), not {what!r}"
            raise ValueError(msg)
        info = np.zeros(4, dtype=np.int32)
        nv.check(self.dev._lib.scs_debug_graph_raw(self.dev._ctx, self._h, int(what), None, nv.iptr(info)))
        rows, ld = int(info[0]), int(info[1])
        out = np.empty((rows, ld), dtype=np.float32 if what else np.float64)
        nv.check(self.dev._lib.scs_debug_graph_raw(self.dev._ctx, self._h, int(what), out.ctypes.data, nv.iptr(info)))
        rb = self.shape[1]
        first = (np.zeros(rows, dtype=np.int64) if (not what or info[3])
                 else (rb + np.arange(rows, dtype=np.int64)) // 512 * 512)
        return out, {"rows": rows, "ld": ld, "col0": int(info[2]), "first_col": first}

    def matrix_free_plan(self) -> dict:
        """``scs_debug_matrix_free_plan``: what ``scs_graph_matrix_free`` planned (``chunks``, ``stack_total``,
        ``b_cap``), where the graph stands (``slabs_b``, ``n_apply``) and ``maxd``, per tree the deepest separator
        the device found.  Host fields only: nothing is launched.  ``ScsError`` (``EINVAL``) on a graph with a matrix."""
        info = np.zeros(6, dtype=np.int64)
        nv.check(self.dev._lib.scs_debug_matrix_free_plan(self._h, nv.lptr(info), None))
        maxd = np.zeros(int(info[5]), dtype=np.int32)
        nv.check(self.dev._lib.scs_debug_matrix_free_plan(self._h, nv.lptr(info), nv.iptr(maxd)))
        return {"chunks": int(info[0]), "stack_total": int(info[1]), "b_cap": int(info[2]), "slabs_b": int(info[3]),
                "n_apply": int(info[4]), "maxd": maxd}

    def degrees_all(self) -> np.ndarray:
        """The degrees of ALL vertices as this rank holds them (``scs_debug_graph_raw``, mode 2)."""
        info = np.zeros(4, dtype=np.int32)
        out = np.empty(self.shape[0])
        nv.check(self.dev._lib.scs_debug_graph_raw(self.dev._ctx, self._h, 2, out.ctypes.data, nv.iptr(info)))
        return out

    def fiedler(self, x_init: np.ndarray | None = None, tol: float = DEFAULT_TOL,
                max_iter: int = DEFAULT_MAX_ITER, block: int = 0):
        """V x 2 spectral embedding + solver report (reference: scs.py:252).

        Raises ``_native.ConvergenceError`` (carrying the embedding and the report it
        reached) when the residual target was not met.
        """
        n = self.shape[0]
        maps = np.empty((n, 2))
        stats = nv.Stats()
        x0 = None
        if x_init is not None:
            x_init = np.ascontiguousarray(x_init, dtype=np.float64)
            if x_init.shape != (n,):
                msg = f"x_init must have shape ({n},)"
                raise ValueError(msg)
            x0 = nv.dptr(x_init)
        rc = self.dev._lib.scs_fiedler(self.dev._ctx, self._h, x0, tol, max_iter, block,
                                       nv.dptr(maps), C.byref(stats))
        if rc == nv.ENOCONV:
            msg = self.dev._lib.scs_last_error()
            raise nv.ConvergenceError(msg.decode() if msg else "not converged", maps, stats.as_dict())
        nv.check(rc)
        return maps, stats.as_dict()
