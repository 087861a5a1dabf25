/*
 * scs_hip.h -- C-ABI of libscs_hip.so, the MI355X (gfx950) spectral-clustering
 * core for Spectral Cluster Supertree.
 *
 * The reference (rmcar17/SpectralClusterSupertree) has no FFI seam on this
 * path: the hot path is private Python called in-process
 * (src/sc_supertree/scs.py:110-134) and its only delegate is scikit-learn's
 * estimator call at scs.py:235-252.  Each entry point below names the reference
 * code it replaces.  All pointers are plain host pointers unless stated, all
 * sizes are explicit, no C++ or torch types cross the boundary.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SCS_E* code on failure;
 *     scs_last_error() gives the message of the calling thread's last failure.
 *   - input arrays are caller-owned, read-only for the duration of the call.
 *   - handles are owned by the library; free them with the matching *_free.
 *   - one host thread per context at a time; different contexts are independent.
 *   - no entry point ever computes on the CPU: without a usable HIP device
 *     scs_ctx_create fails and nothing else can be called.
 */
#ifndef SCS_HIP_H
#define SCS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCS_OK 0
#define SCS_EINVAL (-1)   /* bad argument (shape, range, null pointer)          */
#define SCS_EHIP (-2)     /* a HIP runtime call failed                          */
#define SCS_ENOMEM (-3)   /* device or host allocation failed                   */
#define SCS_ECOMM (-4)    /* RCCL / communicator failure                        */
#define SCS_ENOCONV (-5)  /* scs_fiedler stopped above tol: maps_out and stats filled   */
#define SCS_EUNSUP (-6)   /* valid request the library does not support (yet)   */

#define SCS_UNIQUE_ID_BYTES 128

typedef struct scs_ctx scs_ctx;       /* device, stream, communicator, scratch        */
typedef struct scs_tables scs_tables; /* flattened source trees, resident in HBM      */
typedef struct scs_graph scs_graph;   /* this rank's row block of the PCG weight matrix */

/* Per-call report of scs_fiedler (all times in milliseconds, device-side
 * hipEvent measurements on the context's stream). */
typedef struct scs_stats {
    int32_t n_vertices;      /* V of the graph the solve ran on                      */
    int32_t block;           /* LOBPCG block width actually used (0: dense path)     */
    int32_t iterations;      /* LOBPCG iterations                                    */
    int32_t n_apply;         /* operator applications (launches of the SYMM kernel)  */
    int32_t converged;       /* 1 if the wanted pair(s) met tol                      */
    int32_t used_constraint; /* 1: trivial eigenvector deflated analytically         */
    double lambda[2];        /* two largest eigenvalues of S = D^-1/2 A D^-1/2       */
    double resid[2];         /* ||S x - lambda x||_2 of the returned unit vectors    */
    double lambda_next;      /* next Ritz value below lambda[1] (gap estimate)       */
    double apply_ms_total;   /* SYMM kernel time: HIP-event-timed launches (every 4th
                              * in the fused loop), scaled to all n_apply launches */
    double apply_ms_min;     /* fastest single SYMM launch                           */
    double solve_ms;         /* whole scs_fiedler call, device time                  */
    double apply_bytes;      /* algorithmic HBM bytes of ONE SYMM launch on this rank */
    double allgather_ms_total; /* multi-rank solves: device time of the per-iteration all-gathers
                                * (timed every 4th, scaled to all n_allgather)            */
    double allgather_bytes;  /* bytes ONE all-gather delivers to this rank (world x chunk x 8) */
    int32_t n_allgather;     /* all-gathers enqueued by the solve                      */
    int32_t n_apply32;       /* of n_apply: launches that streamed the single-precision image of W
                              * (mixed-precision loop; apply_ms_total covers the OTHER launches)   */
    double apply32_ms_total; /* SYMM kernel time of those launches (timed sample scaled to all)   */
    double apply32_bytes;    /* algorithmic HBM bytes of ONE such launch                          */
    int32_t lowp_renewals;   /* times S X and S P were renewed through W inside the loop          */
    int32_t reserved;
    double event_pair_ms;    /* an EMPTY event pair on the solve's stream: what the pair around a timed
                              * launch adds to apply_ms_* (a profiler's kernel time is about that much less) */
} scs_stats;

/* Per-call report of scs_pcg_build. */
typedef struct scs_build_stats {
    int32_t n_taxa;
    int32_t n_trees;
    int32_t row_begin, row_end; /* rows of W this rank owns                          */
    int32_t symmetric;          /* 1: upper tiles computed, lower mirrored; 2: shared */
    int32_t n_tiles;            /* workgroups of the accumulate kernel per batch     */
    int32_t n_batches;          /* tree batches (scratch bounded by ctx workspace)   */
    int32_t spec_batches;       /* of them walked by the producer / consumer tile kernel
                                   (k_accumulate_spec; the others by the 4-wave kernels)   */
    double cell_trees;          /* (matrix cell, tree) evaluations performed         */
    double prep_ms;             /* position fill, position / sparse-table / argmin / block-record kernels, and --
                                   tables still on their way, prepared piece by piece as their chunks arrive --
                                   whatever the stream waited for a chunk in between */
    double accumulate_ms;       /* the tile accumulate kernel(s)                     */
    double exchange_ms;         /* shared build: tile all-gather + unpack            */
    double total_ms;            /* whole call, device time                           */
    double bytes_w;             /* algorithmic bytes: W written once (8 * rows * V)  */
    double bytes_tables;        /* algorithmic bytes: tables read once               */
    double exchange_bytes;      /* shared build: bytes of packed tiles this rank received */
    int32_t tree_parallel_batches; /* batches of a small node built tree-parallel: a workgroup
                                      per (tile, tree), the trees' cells added up in order
                                      afterwards (k_sum_tree_tiles) -- same bits as the walk */
    int32_t spec_trees;            /* trees the spec_batches walked (the rest: 4-wave kernels)       */
    double spec_ms;                /* device time of the k_accumulate_spec launches (of accumulate_ms) */
    int32_t listed_batches;        /* batches walked through per-tile tree lists (partial-coverage forests) */
    int32_t prep_pieces;           /* pieces the batches were prepared in: a batch is cut where a late chunk of the
                                      table upload begins, one piece per batch when the tables are resident */
} scs_build_stats;

/* ABI version of this header: 109.  Still 109: scs_debug_matrix_free_plan added (a new symbol breaks no caller).  Still 109: scs_debug_block_records added, and scs_build_stats' `reserved` slot became prep_pieces.  (The rule for a reserved slot: the version changes when a struct's size or a field's offset or meaning changes for a caller that follows the older header of the same number.  A slot that header called `reserved` was written as 0 and promised nothing; naming it, with size and offsets as they were, leaves every such caller correct -- it reads a count it ignores -- so the number stays.  The earlier reuses, 100 -> 101 and 101 -> 102, also made their structs longer.)  scs_debug_apply_ex, scs_debug_gram_ex and scs_debug_update added; scs_score_branch_triplets, scs_score_taxon_triplets, scs_score_placements, scs_score_clade_placements and scs_score_clade_moves added (a new symbol breaks no caller).  108 -> 109: scs_score_concordance added.  107 -> 108: scs_score_conflicts added.  106 -> 107: scs_score_triplets added.  105 -> 106: scs_score_supertree added.  104 -> 105: scs_debug_arena_stats and scs_ctx_reserve added; scs_ctx_trim's keep_bytes counts the
 * free bytes of the device's arena.  103 -> 104: scs_forest_split_level, scs_forest_analyze,
 * scs_forest_tables_download_range, scs_tables_from_forest_range, scs_small_solve_begin_level added;
 * scs_forest_upload checks the arrays.  102 -> 103: scs_stats ends with event_pair_ms.  101 -> 102: scs_stats is
 * 24 bytes longer (n_apply32 in the old `reserved` slot, apply32_ms_total, apply32_bytes, lowp_renewals).  100 -> 101: scs_build_stats is 8 bytes longer
 * (tree_parallel_batches; the old `reserved` slot became spec_batches) and again by spec_trees /
 * spec_ms; scs_forest_* added.  Callers compare it with the value they were compiled against before passing
 * structs (the Python binding refuses a library of another version at load). */
int scs_version(void);
const char *scs_last_error(void);

/* Number of HIP devices visible (0 when none); never fails. */
int scs_device_count(void);

/* ---- context ----------------------------------------------------------- */

/* Rank 0 calls this and ships the 128 bytes to the other ranks by any host
 * channel before they all call scs_ctx_create (RCCL bootstrap). */
int scs_comm_unique_id(void *out128);

/* One context per process per GPU.  world == 1: single device, unique_id may be
 * NULL.  world > 1: row-partitioned solve, one RCCL rank per process
 * (SURVEY.md 8e); the only collective on the data path is the all-gather of
 * the Krylov block inside scs_fiedler. */
int scs_ctx_create(int device, int rank, int world, const void *unique_id128, scs_ctx **out);

/* In-process communicator for `world` contexts that live in ONE process and
 * are driven by `world` host threads (used to exercise the row-partitioned
 * code path on a single GPU; the collective is a thread barrier plus device
 * copies instead of RCCL).  `group` comes from scs_local_group_create. */
typedef struct scs_local_group scs_local_group;
int scs_local_group_create(int world, scs_local_group **out);
int scs_local_group_destroy(scs_local_group *group);
int scs_ctx_create_local(int device, int rank, scs_local_group *group, scs_ctx **out);

int scs_ctx_destroy(scs_ctx *ctx);
int scs_ctx_synchronize(scs_ctx *ctx);
/* Device memory: every block of the library is carved out of a per-device ARENA shared by all contexts of the
 * process (csrc/scs_arena.h) -- slabs taken from the driver stay with the process until they are handed back
 * here, or until the driver refuses a request (then whole free slabs go back and the request is tried again).
 * scs_ctx_trim hands back whole free slabs, largest first, until at most keep_bytes of free arena memory remain
 * on the context's device (0: everything that is free), and with keep_bytes == 0 the context's free
 * page-locked host blocks and the staging / scratch blocks of its small-solve slots that no ticket holds.
 * No reference counterpart. */
int scs_ctx_trim(scs_ctx *ctx, int64_t keep_bytes);
/* Make sure the arena of the context's device holds `bytes` of free memory in one piece, so that a request of
 * that size is served without the driver (on this pool hipMalloc of memory another process has used before costs
 * ~25 ms per GB: the driver clears it).  What a warm-up call leaves behind, without the call. */
int scs_ctx_reserve(scs_ctx *ctx, int64_t bytes);
/* The arena of a device, for tests and reports: out8 = {bytes of slabs held, bytes in use, slabs, chunks,
 * released chunks not yet safe for other contexts, driver allocations so far, driver releases so far,
 * requests served so far}. */
int scs_debug_arena_stats(int device, int64_t *out8);
/* The communicator as it sees itself: kind (0 none, 1 RCCL, 2 in-process team), the world / rank
 * it was created with, and what ncclCommCount / ncclCommUserRank report (-1: not available).
 * No reference counterpart (the reference has no parallelism, scs.py:239 n_jobs = 1). */
int scs_ctx_comm_info(scs_ctx *ctx, int32_t *kind, int32_t *world, int32_t *rank,
                      int32_t *reported_world, int32_t *reported_rank);

/* ---- source forests in HBM (round 5) ------------------------------------ */

/* The source trees as preorder node arrays, resident on the device: what the recursion restricts
 * at every node (reference: src/sc_supertree/scs.py:139-171 with :411-455 --
 * `_generate_induced_trees_with_weights`, cogent3's get_sub_tree per tree and part).
 * Arrays as spectralclustersupertree_amd/treearrays.py: tree t owns nodes [node_off[t],
 * node_off[t+1]) in preorder; parent relative to the tree's first node (-1 root); taxon -1 for
 * inner nodes; length / support NaN for None; n_leaves = nodes with taxon >= 0. */
typedef struct scs_forest scs_forest;
typedef struct scs_forest_info {
    int32_t n_trees;  /* trees that keep two or more leaves of the part       */
    int32_t monotone; /* `branch`: 1 unless a merged inner length is negative  */
    int64_t n_nodes;
    int64_t n_leaves;
} scs_forest_info;

int scs_forest_upload(scs_ctx *ctx, int32_t n_taxa, int32_t n_trees, const int64_t *node_off,
                      const int32_t *parent, const int32_t *taxon, const double *length,
                      const double *support, const double *weights, int64_t n_leaves, scs_forest **out);
int scs_forest_free(scs_ctx *ctx, scs_forest *forest);

/* The forests induced on up to 8 disjoint taxon sets, all from ONE sweep of `forest`, each with
 * its flattened tables (scs.py:411-455 + the strategy values of :555-564): part_of[x] = part of
 * taxon x or -1, new_id[x] = its id inside the part (children number their taxa 0 .. k-1),
 * part_taxa[c] = k of part c, strategy 0 one / 1 depth / 2 branch / 3 bootstrap.  Dropped
 * leaves, spliced unary nodes with merged lengths (folded bottom-up, the parent's length in
 * front), collapsed unary roots, trees left with fewer than two leaves of a part dropped --
 * bit for bit what libscs_host.so's scs_host_split_* + scs_host_flatten produce.
 * SCS_EUNSUP: bootstrap weighting met an inner node without support (the reference fails in
 * `length * tree_weight`, scs.py:656). */
int scs_forest_split(scs_ctx *ctx, const scs_forest *forest, const int32_t *part_of,
                     const int32_t *new_id, int32_t n_parts, const int32_t *part_taxa, int32_t strategy,
                     scs_forest **out_forests, scs_forest_info *info);

/* The tables of a child of scs_forest_split to the host (any pointer may be null): tree_off
 * [n_trees + 1], leaf_taxon / adj_depth / adj_val [n_leaves], tree_index [n_trees] (the tree's
 * index in the parent forest), tree_w [n_trees], present [n_taxa] (1: the taxon occurs). */
int scs_forest_tables_download(scs_ctx *ctx, const scs_forest *forest, int64_t *tree_off,
                               int32_t *leaf_taxon, int32_t *adj_depth, double *adj_val,
                               int32_t *tree_index, double *tree_w, uint8_t *present);

/* The same arrays WITHOUT a copy: scs_forest_split leaves the children's tables in page-locked
 * host memory of the context (one device-to-host copy for all parts); the pointers stay valid
 * until the forest is freed. */
int scs_forest_tables_host(scs_ctx *ctx, const scs_forest *forest, const int64_t **tree_off,
                           const int32_t **leaf_taxon, const int32_t **adj_depth, const double **adj_val,
                           const int32_t **tree_index, const double **tree_w, const uint8_t **present);

/* Node arrays of the trees [t_begin, t_end) to the host (node_off [t_end - t_begin + 1], made
 * relative to the first of them; the other pointers may be null). */
int scs_forest_download(scs_ctx *ctx, const scs_forest *forest, int32_t t_begin, int32_t t_end,
                        int64_t *node_off, int32_t *parent, int32_t *taxon, double *length,
                        double *support, double *weights);

/* The tables of a child of scs_forest_split as an scs_tables handle (what scs_tables_upload makes from
 * host arrays) WITHOUT leaving the device: relabel[x] (may be null: identity) = id of the forest's taxon
 * x in the node's numbering, n_taxa = the node's taxon count.  For scs_pcg_build of the recursion's
 * larger nodes; free with scs_tables_free.  `ctx` may be another context on the same GPU than the one
 * the forest was split on (the look-ahead worker's). */
int scs_tables_from_forest(scs_ctx *ctx, const scs_forest *forest, const int32_t *relabel, int32_t n_taxa,
                           scs_tables **out);

/* ---- a whole level of the recursion in one call (round 6) ---------------- */

/* The reference walks the recursion depth-first, one node at a time (scs.py:139-171).  The nodes of one
 * LEVEL below some node hold disjoint taxon sets, so their forests fit in ONE forest -- the trees of node
 * 0, then of node 1, ... -- over one numbering of the taxa (node k owns a consecutive id range), and one
 * call restricts all of them to all of their parts (scs.py:411-455 for every node of the level):
 *   node_tree_end[k]  exclusive end of node k's trees in `forest` (the last entry = its tree count)
 *   part_of[x]        part of taxon x INSIDE ITS NODE (0 .. n_parts - 1 <= 7), -1: in no child
 *   new_id[x]         its id in the children's numbering (unique over all children), < child_taxa
 * The children come back as ONE forest again -- part-major: the first parts of all nodes (node order),
 * then the second parts, ... -- with its tables resident, and of it the host receives only
 *   child_trees / child_leaves [n_parts][n_nodes]   trees (>= 2 leaves kept) and leaves of child (part, node)
 *   present   [child_taxa]      1: the taxon occurs in a kept tree
 *   comp_root [child_taxa]      smallest id of the taxon's connected component in the proper cluster
 *                               graph of its child (scs.py:458-492 `_get_graph_components`; edges = shared
 *                               root sides whatever the weight, :651-652)
 *   sig       [child_taxa][2]   a 128-bit function of the SET of (tree, root side) the taxon occurs in:
 *                               two taxa are contracted (scs.py:302-316) only if their sets -- hence these
 *                               values -- are equal; distinct values prove that nothing contracts, equal
 *                               ones send the node to the exact host routine.
 * info[0] describes the union (monotone: all parts).  Same restriction semantics and bits as
 * scs_forest_split. */
int scs_forest_split_level(scs_ctx *ctx, const scs_forest *forest, const int32_t *part_of,
                           const int32_t *new_id, int32_t n_parts, int32_t child_taxa, int32_t strategy,
                           int32_t n_nodes, const int32_t *node_tree_end, scs_forest **out_union,
                           scs_forest_info *info, int32_t *child_trees, int64_t *child_leaves,
                           uint8_t *present, int32_t *comp_root, uint64_t *sig);

/* The trees [t_begin, t_end) of a forest as a forest of its own WITHOUT copying a node (the slice points
 * into the arrays of `forest` and keeps them alive; taxon ids stay those of `forest`): one node of a level
 * forest whose subtree is taken up again from its own trees when the true draws did not confirm its
 * provisional partition (scs.py:139-171: the labels of record are the stream's).  Free with
 * scs_forest_free. */
int scs_forest_slice(scs_ctx *ctx, const scs_forest *forest, int32_t t_begin, int32_t t_end, scs_forest **out);

/* comp_root [n_taxa] and sig [n_taxa][2] (as above) of a forest that carries tables: the first forest of a
 * level-synchronous walk (a child of scs_forest_split). */
int scs_forest_analyze(scs_ctx *ctx, const scs_forest *forest, int32_t *comp_root, uint64_t *sig);

/* Tables of the trees [t_begin, t_end) of a forest that carries them to the host (tree_off
 * [t_end - t_begin + 1] made relative to the first of them; other pointers may be null): the exact host
 * routine for the contraction groups of a node whose signatures collide (scs.py:302-316). */
int scs_forest_tables_download_range(scs_ctx *ctx, const scs_forest *forest, int32_t t_begin, int32_t t_end,
                                     int64_t *tree_off, int32_t *leaf_taxon, int32_t *adj_depth,
                                     double *adj_val, double *tree_w);

/* scs_tables_from_forest for ONE node of a level forest: the trees [t_begin, t_end), whose taxon ids lie
 * in [u_base, u_base + u_size); relabel[x - u_base] = the node's own id of taxon x (present taxa only,
 * contraction groups consecutive), n_taxa = the node's taxon count. */
int scs_tables_from_forest_range(scs_ctx *ctx, const scs_forest *forest, int32_t t_begin, int32_t t_end,
                                 int32_t u_base, int32_t u_size, const int32_t *relabel, int32_t n_taxa,
                                 scs_tables **out);

/* ---- tables ------------------------------------------------------------ */

/* Page-locked host memory (hipHostMalloc) for callers that want scs_tables_upload to run at
 * the full PCIe rate: tables that live in such a block are copied by DMA straight from it, a
 * pageable source is staged by the runtime at a fraction of that.  Optional -- any host
 * pointer is accepted by scs_tables_upload.  Free with scs_host_free. */
int scs_host_alloc(size_t bytes, void **out);
int scs_host_free(void *p);

/* Host -> HBM copy of the flattened trees (layout: DESIGN.md "Tables").
 * Replaces the reference's in-memory cogent3 trees as the input of
 * _proper_cluster_graph_edges (scs.py:495-583); the weighting strategy
 * (scs.py:555-564) is already folded into adj_val by the host.
 *   tree_off   int64 [n_trees+1]   leaf offsets, tree_off[0] == 0
 *   leaf_taxon int32 [L]           taxon id of each leaf in DFS order
 *   adj_depth  int32 [L]           depth of LCA(leaf p, leaf p+1); last slot of a tree unused
 *   adj_val    fp64  [L]           strategy value at that LCA
 *   tree_w     fp64  [n_trees]     tree weights
 * Shapes are checked on the host, the ranges of leaf_taxon / adj_depth by a kernel on the
 * uploaded copy (SCS_EINVAL, nothing is kept).  The arrays share ONE device block taken from
 * the context's block cache.
 * Page-locked arrays (scs_host_alloc) of a forest that scs_pcg_build walks in several tree
 * batches (more than 2 048 taxa): the call returns once the first 64 trees have arrived and been
 * checked (scs_pcg_build makes them a first, short batch); the rest travels on a copy stream in chunks, and scs_pcg_build makes
 * its stream wait for the chunks each tree batch needs -- the copy overlaps the first batches.
 * The three leaf arrays must then stay valid and unchanged until the first scs_pcg_build on
 * these tables (or scs_tables_free) has returned, and a range error in a late chunk is reported
 * by that call (SCS_EINVAL) instead of this one.  Pageable arrays: copied whole, as before.  */
int scs_tables_upload(scs_ctx *ctx, int32_t n_taxa, int32_t n_trees, const int64_t *tree_off,
                      const int32_t *leaf_taxon, const int32_t *adj_depth, const double *adj_val,
                      const double *tree_w, scs_tables **out);
int scs_tables_free(scs_ctx *ctx, scs_tables *tables);

/* ---- scoring a supertree against its sources ------ */

/* Robinson-Foulds terms per source tree and clade support per supertree node -- neither the reference nor the
 * recursion computes them.  `sources` are flattened trees (scs_tables_upload / scs_tables_from_forest; adj_val and
 * tree_w are not read: every count is unweighted) over the taxon ids 0 .. n_taxa - 1; the supertree S comes as
 * preorder arrays of n_nodes: parent[v] < v (-1 for node 0, the root), taxon[v] = id of a tip (each id at most
 * once; ids >= the sources' n_taxa are taxa no source has), -1 for an inner node.  Clusters are leaf sets; a
 * cluster of a tree on leaf set L is nontrivial when 2 <= size < |L|; C(S|T) = the nontrivial sets C ∩ L(T) over
 * the clades C of S, C(T) = T's own nontrivial clusters.  Per source tree t (n_trees entries):
 *   n_super[t] = |C(S|T)|, n_source[t] = |C(T)|, shared[t] = |C(S|T) ∩ C(T)|  (RF = n_super + n_source - 2 shared)
 * Per node C of S (n_nodes entries, S's preorder, unary nodes included):
 *   informative[C] = #{T : 2 <= |C ∩ L(T)| < |L(T)|},  supported[C] = those T with C ∩ L(T) in C(T).
 * max_batch_trees > 0 caps the trees of one device batch (tests); 0: sized by workspace.  Output pointers may be
 * null.  SCS_EINVAL: malformed supertree arrays, or (checked on the device) a source taxon out of range, missing
 * from S or twice in one tree. */
int scs_score_supertree(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                        const int32_t *taxon, int32_t max_batch_trees, int64_t *n_super, int64_t *n_source,
                        int64_t *shared, int64_t *informative, int64_t *supported);

/* MRP parsimony scores per source tree and per source clade, same inputs and SCS_EINVAL cases,
 * in the same order, as scs_score_supertree.  For a source tree T on leaf set L with m = |L| >= 3 and S' = S|L:
 *   characters: T's nontrivial clusters C(T), 2 <= |C| < m, each once, in the order of the clusters' first gaps in
 *     T's DFS order (the gap between the first and second child in the flattened table).  Character C gives state 1
 *     to the taxa of C, 0 to L - C, and "missing" to every other tip of S (the Baum-Ragan matrix of the sources).
 *   len(C): the least number of state changes of that character on S with an all-zero outgroup attached above the
 *     root (rooted coding), polytomies taken as hard; it equals the length on S' with the outgroup.  len(C) >= 1;
 *     len(C) = 1 iff C is a cluster of S'; len(C) <= gmax(C) = min(|C|, m - |C| + 1), the length on a star.
 * Per source tree t (n_trees entries; trees of fewer than 3 leaves give zeros):
 *   mrp_chars[t] = |C(T)| (= n_source[t]), mrp_length[t] = sum of len, mrp_perfect[t] = #{len = 1} (= shared[t]),
 *   mrp_max[t] = sum of gmax.
 * Per character, in tree order and within a tree in character order: char_off[n_trees + 1] the first character of
 * every tree (and the total), char_len its length, char_lo / char_hi the first and last leaf position of its cluster
 * in T's DFS order, relative to the tree.  char_len, char_lo and char_hi are buffers the caller sizes: sum of
 * mrp_chars entries, which a first call with the three null returns (char_off[n_trees]), as does n_source of
 * scs_score_supertree.  Any output pointer may be null; the per-character lengths cost a second kernel variant that
 * runs only when char_len is given.  max_pass_words > 0 lowers the 64-character words of a tree one pass covers (at
 * most 64; tests); a tree of more characters takes several passes. */
int scs_score_parsimony(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                        const int32_t *taxon, int32_t max_batch_trees, int32_t max_pass_words, int64_t *mrp_chars,
                        int64_t *mrp_length, int64_t *mrp_perfect, int64_t *mrp_max, int64_t *char_off,
                        int32_t *char_len, int32_t *char_lo, int32_t *char_hi);

/* Pairwise source-tree distances on shared taxa: the Robinson-Foulds terms between every two
 * source trees, each pair restricted to the taxa both hold.  `sources` as for scs_score_supertree (adj_val and tree_w
 * are not read).  For a row tree A and a column tree B, with L = L(A) ∩ L(B), c = |L| and C(X|L) the set of DISTINCT
 * leaf sets {cl(v) ∩ L : v a node of X} with 2 <= size < c (a set counts once however many nodes carry it):
 *   common[A][B] = c, clusters[A][B] = |C(A|L)|, clusters_other[A][B] = |C(B|L)|, shared[A][B] = |C(A|L) ∩ C(B|L)|
 *   (RF = clusters + clusters_other - 2 shared).  c < 3: common = c, the other three 0.  A against itself: c = its
 *   leaves, all three counts its n_source.  Every count is exact and unweighted.
 * rows: n_rows tree ids, in any order, repeats allowed; NULL: every tree, and n_rows must be the tables' tree count.
 * Outputs: n_rows x n_trees int32, row-major (every count is below a tree's leaf count); any of them may be null.
 * max_batch_trees > 0 caps the trees of a row batch and of a column batch of the tiled pair matrix (tests); 0: sized
 * by workspace.  max_lds_bytes > 0 caps the LDS of a pair workgroup (tests): a pair whose arrays need more runs from
 * a slab in the call's block, as does every pair past the 160 KiB of a workgroup -- no tree size is refused.
 * SCS_EINVAL: a row id out of range, n_rows < 0, rows NULL with n_rows != n_trees, max_lds_bytes < 0, or (checked on
 * the device before any pair kernel runs) a source taxon out of range or twice in one tree. */
int scs_score_source_pairs(scs_ctx *ctx, const scs_tables *sources, int32_t n_rows, const int32_t *rows,
                           int32_t max_batch_trees, int32_t max_lds_bytes, int32_t *common, int32_t *clusters,
                           int32_t *clusters_other, int32_t *shared);

/* Pairwise rooted-triplet terms of the source trees on shared taxa: the two-sided restriction of
 * scs_score_source_pairs joined to the node-pair sum of scs_score_triplets.  `sources`, `rows`, `n_rows` and
 * max_batch_trees as for scs_score_source_pairs.  For a row tree A and a column tree B, with L = L(A) ∩ L(B) and
 * c = |L|, a triple {a, b, d} of L is resolved ab|d in a tree when one of its clusters holds a and b but not d:
 *   common[A][B] = c (int32),
 *   triplets[A][B] = the triples of L that A resolves, triplets_other[A][B] = those that B resolves,
 *   triplets_shared[A][B] = those both resolve the same way (int64; the total is C(c, 3)).
 *   c < 3: the three counts are 0.  A against itself: all three are equal.  Every count is exact and unweighted.
 * Outputs: n_rows x n_trees, row-major; any of them may be null (without triplets_shared no node pair is swept).
 * With rows NULL only the pairs A <= B are computed and the cell (B, A) gets the cell (A, B) with triplets and
 * triplets_other swapped.
 * max_lds_bytes > 0 caps the LDS of a workgroup (tests): the sweep takes fewer nodes of B a workgroup, down to one,
 * and a pair whose restriction needs more runs from its region of the call's block.  max_chunk_pairs > 0 caps the
 * pairs whose restricted trees lie in the workspace at once (tests); 0: sized by bytes.
 * SCS_EINVAL: the cases of scs_score_source_pairs, a negative knob, a pair of trees whose smaller one has more than
 * 327 679 leaves (the two bitset rows of one node of B must fit the 160 KiB of a workgroup) or, with max_lds_bytes,
 * more than its rows hold -- both decided on the host before any kernel runs. */
int scs_score_source_pair_triplets(scs_ctx *ctx, const scs_tables *sources, int32_t n_rows, const int32_t *rows,
                                   int32_t max_batch_trees, int32_t max_lds_bytes, int32_t max_chunk_pairs,
                                   int32_t *common, int64_t *triplets, int64_t *triplets_other,
                                   int64_t *triplets_shared);

/* Triple coverage of the sources: which taxa are ever seen together.
 * `sources` are tables as for scs_score_source_pairs.  Only `tree_off` and `leaf_taxon` are read.  n = the tables'
 * `n_taxa`.
 *   M[x] is the set of trees that hold taxon x.
 *   cov(a, b, c) = |M[a] ∩ M[b] ∩ M[c]|.
 *   A triple of three distinct taxa is *covered* when cov >= k, with k = `min_trees` >= 1.
 * For the row taxa r, given as `rows` (ids in any order, repeats allowed; NULL means every taxon, and then `n_rows`
 * must be n):
 *   `occurs[x]`, int32, n entries, always for all taxa: |M[x]|.
 *   `pair_trees[r][b]`, int32, n_rows x n, row-major: |M[a] ∩ M[b]|.  The diagonal is `occurs[a]`.
 *   `pair_covered[r][b]`, int32, n_rows x n: #{c ∉ {a, b} : cov(a, b, c) >= k}.  The diagonal is 0.
 *   `taxon_covered[r]`, int64, n_rows: the covered triples that contain a.  This equals Σ_b `pair_covered[r][b]` / 2.
 * Any output may be null.  With both matrices null no device buffer of n_rows x n entries is allocated: taxon_covered
 * comes from sums kept on the device.  The rows are batched by workspace; max_batch_rows > 0 caps a row batch (tests).
 * max_reg_words > 0 lowers the words of a taxon's membership row a lane holds in registers (64 at most: up to 2 048
 * trees; tests) -- a row of more words is streamed from memory instead, so no number of trees is refused.  No size is
 * refused: the cost is O(n_rows · n² · ⌈trees/32⌉) word operations, every count exact.
 * SCS_EINVAL: null ctx or tables, min_trees < 1, a row id out of range, n_rows < 0, rows NULL with n_rows != n, a
 * negative knob, or (checked on the device before any sweep kernel runs) a source taxon out of range or twice in one
 * tree. */
int scs_score_coverage(scs_ctx *ctx, const scs_tables *sources, int32_t n_rows, const int32_t *rows, int32_t min_trees,
                       int32_t max_batch_rows, int32_t max_reg_words, int32_t *occurs, int32_t *pair_trees,
                       int32_t *pair_covered, int64_t *taxon_covered);

/* Internode distances of the sources, summed per pair of taxa: the input of ASTRID / NJst and
 * of average-consensus supertrees.  `sources` are tables as for scs_score_source_pairs.  Only `tree_off`,
 * `leaf_taxon` and `adj_depth` are read.  n = the tables' `n_taxa`.
 *   T* is the tree of T's distinct clusters: gaps of equal adj_depth with no shallower gap between them are one node
 *   (a polytomy is one node); a node with one child is merged away (the tables cannot see it).
 *   r(gap) = the number of distinct nodes strictly above the gap's node.  The top node has r = 0 whatever its
 *   adj_depth; the parent of a node is the node of the deeper of the two nearest strictly shallower gaps, left and
 *   right.  A leaf's parent is the node of the deeper of its two neighbouring gaps (its only one at a tree's end), and
 *   depth(leaf) = that r + 1.
 *   d_T(a, b), a != b both in T, = depth(a) + depth(b) - 2 min r over the gaps between the two leaves: the number of
 *   edges between them in T*.  A cherry gives 2; in ((a,b),c) d(a,c) = 3; every pair of a star gives 2.  d_T is taken
 *   in T itself, not in a restriction (ASTRID's convention).
 *   `tree_w`: a non-negative int64 per tree, NULL = 1.  A tree of weight w counts exactly like w copies of it; weight 0
 *   counts as absent.
 * For the row taxa r, given as `rows` (ids in any order, repeats allowed; NULL means every taxon, and then `n_rows`
 * must be n), all int64 and exact, n_rows x n row-major with diagonal 0:
 *   `pair_weight[r][b]` = Σ w_t over the trees that hold both taxa,
 *   `dist_sum[r][b]` = Σ w_t d_t(a, b),   `sq_sum[r][b]` = Σ w_t d_t(a, b)²;
 *   `taxon_weight[r]`, `taxon_sum[r]`, `taxon_sq[r]`: the row sums of the three;
 *   `taxon_partners[r]`, int32: #{b : pair_weight > 0}.
 * Any output may be null.  With the three matrices null no device buffer of n_rows x n entries is allocated: the
 * per-taxon outputs come from sums kept on the device.  Rows and trees are batched by workspace; max_batch_rows /
 * max_batch_trees > 0 cap a row / tree batch (tests).  Results do not depend on the batches.  No size is refused.
 * Overflow: with h_t the largest leaf depth and m_t the leaves of tree t, B1 = Σ w_t (m_t - 1) 2h_t and, when sq_sum
 * or taxon_sq is asked for, B2 = Σ w_t (m_t - 1) (2h_t)² bound every cell and row sum; one above 2^63 - 1 is
 * SCS_EINVAL, decided after the depth pass and before any sweep kernel.
 * SCS_EINVAL as well: null ctx or tables, a row id out of range, n_rows < 0, rows NULL with n_rows != n, a negative
 * weight or knob, or (checked on the device before any sweep kernel runs) a source taxon out of range or twice in one
 * tree. */
int scs_score_internode(scs_ctx *ctx, const scs_tables *sources, int32_t n_rows, const int32_t *rows,
                        const int64_t *tree_w, int32_t max_batch_rows, int32_t max_batch_trees,
                        int64_t *pair_weight, int64_t *dist_sum, int64_t *sq_sum, int64_t *taxon_weight,
                        int64_t *taxon_sum, int64_t *taxon_sq, int32_t *taxon_partners);

/* Rooted triplet terms per source tree, same inputs and SCS_EINVAL cases as
 * scs_score_supertree.  For a source tree T on the leaf set L and S' = S|L, a triple {a, b, c} of L is resolved
 * ab|c in a tree when one of its clusters holds a and b but not c, and a fan when no cluster separates one pair:
 *   t_super[t]  = triples S' resolves,  t_source[t] = triples T resolves,
 *   t_shared[t] = triples resolved alike in both  (triplet distance = t_super + t_source - 2 t_shared).
 * Trees of fewer than 3 leaves give zeros; counts are unweighted.  The pair kernel holds two bitsets over a tree's
 * leaves in LDS: SCS_EINVAL as well for a source tree of more than 327 679 leaves. */
int scs_score_triplets(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                       const int32_t *taxon, int32_t max_batch_trees, int64_t *t_super, int64_t *t_source,
                       int64_t *t_shared);

/* Clade conflicts, same inputs and SCS_EINVAL cases as scs_score_supertree.  Two sets A and
 * B conflict when A ∩ B is not empty and neither holds the other; a set conflicts with a tree when it conflicts with
 * one of the tree's clusters (a cluster the tree displays never does).  For a source tree T on the leaf set L and
 * S' = S|L, with C(S|T) and C(T) as for scs_score_supertree:
 *   n_super_conflict[t]  = the clusters of C(S|T) that conflict with T,
 *   n_source_conflict[t] = the clusters of C(T) that conflict with S'.
 * Per node C of S (n_nodes entries, S's preorder):
 *   conflicting[C] = #{T : C ∩ L(T) is nontrivial and conflicts with T}  (supported + conflicting <= informative;
 *   the rest are the sources that are compatible with C without resolving it).
 * Trees of fewer than 3 leaves give zeros; counts are unweighted.  Output pointers may be null. */
int scs_score_conflicts(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                        const int32_t *taxon, int32_t max_batch_trees, int64_t *n_super_conflict,
                        int64_t *n_source_conflict, int64_t *conflicting);

/* Branch concordance, same inputs and SCS_EINVAL cases as scs_score_supertree.  A node C of S
 * is a quartet branch when it is not the root, has exactly two children A (the first in preorder) and B, and its
 * parent has exactly two children, C and its sibling D.  A source tree T on the leaf set L is decisive for C when
 * A ∩ L, B ∩ L and D ∩ L are all non-empty; a decisive T is concordant when (A ∪ B) ∩ L is a cluster of T, alt1 when
 * (A ∪ D) ∩ L is, alt2 when (B ∪ D) ∩ L is (at most one of the three holds) and `other` when none is.
 * Per source tree:
 *   n_decisive[t]    = the quartet branches t is decisive for,
 *   n_concordant[t]  = those it is concordant with,
 *   n_alternative[t] = those where it displays alt1 or alt2.
 * Per node C of S (n_nodes entries, S's preorder; zeros where C is not a quartet branch):
 *   decisive[C], concordant[C], alt1[C], alt2[C] = the sources of each kind
 *   (decisive <= informative, concordant <= supported, alt1 + alt2 <= conflicting,
 *   other = decisive - concordant - alt1 - alt2 >= 0).
 * Trees of fewer than 3 leaves give zeros; counts are unweighted.  Output pointers may be null. */
int scs_score_concordance(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                          const int32_t *taxon, int32_t max_batch_trees, int64_t *n_decisive, int64_t *n_concordant,
                          int64_t *n_alternative, int64_t *decisive, int64_t *concordant, int64_t *alt1,
                          int64_t *alt2);

/* Per-branch triplet support, same inputs and SCS_EINVAL cases as scs_score_supertree: the
 * graded form of scs_score_concordance.  For a quartet branch C of S (children A and B, sibling D) and a source tree T
 * on the leaf set L that is decisive for it (A' = A ∩ L, B' = B ∩ L, D' = D ∩ L all non-empty), each of the
 * |A'| |B'| |D'| triples (a in A', b in B', d in D') is resolved ab|d by T (some cluster of T holds a and b but not
 * d), ad|b, bd|a, or left a fan.
 * Per node C of S (n_nodes entries, S's preorder; zeros where C is not a quartet branch), summed over the sources:
 *   bt_total[C] = the triples, bt_concordant[C] / bt_alt1[C] / bt_alt2[C] = those resolved ab|d / ad|b / bd|a
 *   (bt_concordant + bt_alt1 + bt_alt2 <= bt_total, the rest are fans; bt_total[C] > 0 iff decisive[C] > 0).
 * Per source tree, the same sums over its branches:
 *   n_bt_total[t], n_bt_concordant[t], n_bt_alternative[t] (alt1 + alt2)
 *   (a triple belongs to at most one branch: n_bt_total <= t_super, n_bt_concordant <= t_shared).
 * Counts are unweighted and exact; output pointers may be null.  The pair kernel holds three bitsets over a tree's
 * leaves in LDS: SCS_EINVAL as well for a source tree of more than 218 431 leaves, and when the sum over the trees of
 * (leaves / 3)^3, the bound of a node's count, does not fit int64. */
int scs_score_branch_triplets(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                              const int32_t *taxon, int32_t max_batch_trees, int64_t *n_bt_total,
                              int64_t *n_bt_concordant, int64_t *n_bt_alternative, int64_t *bt_total,
                              int64_t *bt_concordant, int64_t *bt_alt1, int64_t *bt_alt2);

/* Per-taxon triplet support, same inputs and SCS_EINVAL cases as scs_score_supertree: the
 * triplet terms of scs_score_triplets attributed to the taxa of every triple, to name the misplaced ones.  Per
 * supertree tip x, summed over the source trees T on a leaf set L with x in L and m = |L| >= 3, S' = S|L:
 *   tx_trees[x]  = the number of such trees,      tx_total[x]  = sum of C(m - 1, 2), the triples of L that hold x,
 *   tx_super[x]  = those of them S' resolves,     tx_source[x] = those T resolves,
 *   tx_shared[x] = those resolved alike in both   (per-taxon triplet distance = tx_super + tx_source - 2 tx_shared).
 * Every triple has three taxa: sum_x tx_shared = 3 sum_t t_shared, likewise tx_super and tx_source, and
 * sum_x tx_total = 3 sum_t C(m, 3).  The outputs are indexed by taxon id and have one entry per supertree tip, so the
 * tips' ids must be below their number: SCS_EINVAL otherwise, and, as for scs_score_triplets, for a source tree of
 * more than 327 679 leaves.  Counts are unweighted and exact; taxa no source holds and trees of fewer than 3 leaves
 * give zeros; output pointers may be null.  max_lds_bytes > 0 caps the LDS a workgroup of the pair kernel takes beyond
 * one pair of bitset rows (tests: the nodes whose arrays do not fit are counted through global memory); 0: the
 * default, all a workgroup can take. */
int scs_score_taxon_triplets(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                             const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                             int64_t *tx_trees, int64_t *tx_total, int64_t *tx_super, int64_t *tx_source,
                             int64_t *tx_shared);

/* Taxon placement support, same inputs and SCS_EINVAL cases as scs_score_supertree: for each
 * of n_queries query taxa x (taxon ids of supertree tips, each once) and every node v of the supertree S, the triplet
 * terms x would have if it were pruned and regrafted on the edge above v.  S_{x->v} has, for every cluster C of S,
 * (C - x) + x when C belongs to a strict ancestor of v and C - x otherwise, and the new cluster (cl(v) - x) + x; empty
 * sets are dropped.  Summed over the source trees T on a leaf set L with x in L and m = |L| >= 3, over the C(m - 1, 2)
 * triples {x, a, b} of L:
 *   pl_trees[i], pl_total[i]         = tx_trees[x], tx_total[x] of scs_score_taxon_triplets,
 *   pl_source[i]                     = the triples T resolves (no v in it),
 *   pl_super[i * n_nodes + v]        = the triples S_{x->v}|L resolves,
 *   pl_shared[i * n_nodes + v]       = those T and S_{x->v}|L resolve alike,
 * for query i, so that pl_super + pl_source - 2 pl_shared is the triplet distance x would have there.  The entry at
 * x's own node (and at its sibling, and at a parent with two children) holds tx_super[x] and tx_shared[x].  Counts are
 * unweighted and exact; a query no source holds gives zero rows; output pointers may be null.  SCS_EINVAL as well for
 * a query that is no tip's taxon id or is given twice, for a source tree of more than 327 679 leaves (as for
 * scs_score_triplets), and when the rows do not fit the call's workspace: three rows of n_nodes + 1 int64 per query
 * and output and two of n_nodes per 64 queries, 48 n_queries (n_nodes + 1) + 16 ceil(n_queries / 64) n_nodes bytes,
 * may take at most 1.5 GB (64 queries on 480 000 nodes, 1 500 on 20 000).  Queries go through the batches 64 at a time.
 * max_lds_bytes > 0 caps the LDS a workgroup of the pair kernel takes (tests: when the sums per node and query do not
 * fit beside the bitset rows, every node pair sends its own marks); 0: the default, all a workgroup can take. */
int scs_score_placements(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                         const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes, int32_t n_queries,
                         const int32_t *queries, int64_t *pl_trees, int64_t *pl_total, int64_t *pl_source,
                         int64_t *pl_super, int64_t *pl_shared);

/* Clade placement support, same inputs and SCS_EINVAL cases as scs_score_placements: for each
 * of n_queries query nodes q of the supertree S (preorder indices; any node but the root, a tip included) with leaf
 * set Q, and every node v of S, the triplet terms the clade would have if the subtree of q were pruned and regrafted
 * on the edge above v.  For v outside the subtree of q, S_{q->v} has, for every cluster C of S not inside that subtree,
 * (C - Q) + Q when C belongs to a strict ancestor of v and C - Q otherwise, the clusters inside the subtree unchanged,
 * and the new cluster (cl(v) - Q) + Q; empty sets are dropped.  For v inside the subtree of q (q included) S_{q->v} = S:
 * those entries hold the value of the clade's own position.  Summed over the source trees T on a leaf set L with
 * Q' = Q & L and R = L - Q both non-empty and m = |L| >= 3, over the crossing triples of L (a taxon in Q', one in R):
 *   cp_trees[i]                      = the number of such sources,
 *   cp_total[i]                      = the crossing triples, C(m, 3) - C(|Q'|, 3) - C(|R|, 3) per source,
 *   cp_source[i]                     = those T resolves (no v in it),
 *   cp_super[i * n_nodes + v]        = those S_{q->v}|L resolves,
 *   cp_shared[i * n_nodes + v]       = those T and S_{q->v}|L resolve alike,
 * so that cp_super + cp_source - 2 cp_shared is the part of the triplet distance the move can change.  For a tip q
 * the outputs are those of scs_score_placements for its taxon.  Counts are unweighted and exact; a query no source
 * crosses gives zero rows; nested or overlapping query clades are independent; output pointers may be null.
 * SCS_EINVAL as well for a query node that is the root, out of range or given twice, for a source tree of more than
 * 327 679 leaves (as for scs_score_triplets), and when the rows do not fit the call's workspace: three rows of
 * n_nodes + 1 int64 per query and output, 48 n_queries (n_nodes + 1) bytes, may take at most 1.5 GB (64 clades on
 * 480 000 nodes, 1 500 on 20 000).  Every tip of a query clade is a sub-query of the sweep, and the sub-queries go
 * through the batches 64 at a time: the cost grows linearly with the tips of the query clades taken together.
 * max_lds_bytes as for scs_score_placements. */
int scs_score_clade_placements(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                               const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                               int32_t n_queries, const int32_t *query_nodes, int64_t *cp_trees, int64_t *cp_total,
                               int64_t *cp_source, int64_t *cp_super, int64_t *cp_shared);

/* The best regraft targets of every query clade: the sweep, the inputs, the SCS_EINVAL cases
 * and the workspace rule of scs_score_clade_placements, but the two rows per query (cp_super, cp_shared) stay on the
 * device and a kernel reduces each of them there; cp_trees, cp_total and cp_source are as there.  top_k is 1 to 8
 * (SCS_EINVAL otherwise).  Per query i with node q = query_nodes[i]:
 *   mv_own_super[i], mv_own_shared[i] = the row entries at q itself: the clade where it is;
 *   mv_node[i * top_k + j]            = the j-th best candidate node, int32,
 *   mv_super[i * top_k + j], mv_shared[i * top_k + j] = the row entries there.
 * The candidates are the nodes v outside the preorder range [q, end of the subtree of q): the whole subtree is left
 * out.  They are ordered by the key (d, v) ascending with d = cp_super[i][v] - 2 cp_shared[i][v] (signed; cp_source is
 * the same along a row, so this is the order of the clade placement distance) and ties go to the lower preorder index.
 * The root is always a candidate, so j = 0 always holds a node; where fewer than top_k candidates exist the further
 * entries hold mv_node = -1 and zeros.  Output pointers may be null. */
int scs_score_clade_moves(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                          const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes, int32_t n_queries,
                          const int32_t *query_nodes, int32_t top_k, int64_t *cp_trees, int64_t *cp_total,
                          int64_t *cp_source, int64_t *mv_own_super, int64_t *mv_own_shared, int32_t *mv_node,
                          int64_t *mv_super, int64_t *mv_shared);

/* Supertree polytomies, with the inputs and SCS_EINVAL cases of scs_score_branch_triplets:
 * what the sources say about grouping the children of an unresolved node.  query_nodes: n_queries preorder indices of
 * nodes of S with k = 3 to 64 children c_0 .. c_{k-1} (child order; the root may be one).  For a source tree T on the
 * leaf set L, colour i is C_i' = cl(c_i) & L; T is decisive when at least three colours are non-empty.  Per query q:
 *   py_degree[q] = k (int32),   py_trees[q] = the decisive sources,
 *   py_total / py_joint: one dense block of k^3 int64 per query, the blocks one after the other in query order (block
 *   q starts at the sum of the earlier queries' k^3); entry [(i k + j) k + l] is filled for i < j and l not in
 *   {i, j}, zero elsewhere.  Over the decisive sources:
 *   py_total[i][j][l] = sum |C_i'| |C_j'| |C_l'|: the triples (a in C_i, b in C_j, d in C_l), all fans in S,
 *   py_joint[i][j][l] = those of them T resolves ab|d.
 * Merging the groups G and H of a partition of the children under a new node (a third group remaining) lowers the
 * summed triplet distance by exactly 2 M(G, H) - N(G, H), M and N the sums of py_joint and py_total over i in G,
 * j in H (ordered so that i < j), l in neither.  Counts are unweighted and exact; output pointers may be null.
 * SCS_EINVAL, before any kernel runs, as well for: a query that is no node, has fewer than 3 or more than 64 children
 * or is given twice; the k rows of the largest source tree (m leaves) not fitting a workgroup's LDS,
 * 8 k ceil(m / 32) bytes > 160 KiB (218 432 leaves at k = 3, 10 240 at k = 64) or > max_lds_bytes when that is
 * positive; the tensors not fitting the call's workspace, 16 sum k^3 bytes > 1.5 GB; sum (m_t / 3)^3 not fitting
 * int64.  max_lds_bytes > 0 caps the LDS a workgroup of the sweep takes (tests: where the k^2 sums do not fit beside
 * the rows, the sweep adds straight onto the output); 0: the default, all a workgroup can take. */
int scs_score_polytomies(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                         const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes, int32_t n_queries,
                         const int32_t *query_nodes, int32_t *py_degree, int64_t *py_trees, int64_t *py_total,
                         int64_t *py_joint);

/* Resampled and weighted branch triplet support, with the inputs of
 * scs_score_branch_triplets.  weights: n_rep rows of n_trees non-negative int32 tree weights, in the tables' tree
 * order; a tree of weight w counts exactly like w copies of it.  With bt_x(T, u) what T alone contributes to bt_x[u]
 * (x = total, concordant, alt1, alt2 in this order; 0 where T is not decisive for u):
 *   rs_x[r][u] = sum_T weights[r][T] bt_x(T, u).
 * Row 0 is the point estimate (all ones: the outputs of scs_score_branch_triplets); rows 1 .. n_rep - 1 are
 * replicates.  A replicate with rs_total[r][u] > 0 is counted once at u: in win_concordant when concordant is strictly
 * greater than both alternatives, else in win_alt1 / win_alt2 when that alternative is strictly greatest, else in
 * win_tie.  Outputs:
 *   rs_point[4][n_nodes] (int64): row 0;   rs_wins[4][n_nodes] (int32): win_concordant, win_alt1, win_alt2, win_tie;
 *   rs_rows[4][n_rep][n_nodes] (int64): every row, or NULL (not downloaded).
 * Nodes that are no quartet branch hold zeros.  The section 18 sweep runs once per batch and keeps its per-tree terms
 * in a slab of 32 n_nodes bytes per tree, which bounds the trees of a batch.  SCS_EINVAL, before any kernel runs, as
 * well for: n_rep < 1; a negative weight; a source tree of more than 218 431 leaves; a row whose
 * sum_T weights[r][T] floor(m_T^3 / 27) does not fit int64; accumulators of 32 n_rep n_nodes bytes > 1.5 GB. */
int scs_score_branch_resample(scs_ctx *ctx, const scs_tables *sources, int32_t n_nodes, const int32_t *parent,
                              const int32_t *taxon, int32_t max_batch_trees, int32_t n_rep, const int32_t *weights,
                              int64_t *rs_point, int32_t *rs_wins, int64_t *rs_rows);

/* ---- proper cluster graph ---------------------------------------------- */

/* Build rows [row_begin, row_end) of the N x N fp64 weight matrix W on the
 * device: W[a][b] = sum over trees, in tree order, of value(LCA(a,b)) * w_t for
 * every tree in which a and b share a root side.  Bit-identical to the
 * reference's accumulation (scs.py:655-657): one rounded multiply, then rounded
 * adds in tree order.  Replaces _proper_cluster_graph_edges/_dfs_pcg_weights
 * (scs.py:495-663) and the dense fill loop (scs.py:246-250).
 * row_begin = 0, row_end = n_taxa with world == 1 uses the symmetric schedule.
 * flags: SCS_BUILD_MONOTONE promises that adj_val never decreases from an
 * ancestor to a descendant inside any tree (true for `one`, `depth`, and for
 * `branch` when no internal branch length is negative); it selects a cheaper
 * kernel that produces the same bits.  Pass 0 when unsure.
 * SCS_BUILD_SHARED (collective, world > 1, every rank passes it or none does):
 * instead of every rank evaluating all the cells of its own rows -- each
 * off-diagonal cell twice across the job -- the ranks split the upper-triangle
 * tiles of the whole matrix round-robin, all-gather the packed tiles and unpack
 * their own rows (direct cells and mirror images).  Same bits, half the
 * evaluations.  The exchange is point to point: a tile travels only to the ranks whose rows
 * it touches (one grouped round of RCCL send/recv, ~8 V^2 / world bytes received per rank;
 * SCS_EXCHANGE=allgather selects one all-gather of the whole packed triangle instead).  Falls
 * back to the plain row build when the packed triangle would exceed 96 GiB.  stats may be
 * NULL. */
#define SCS_BUILD_MONOTONE 1
#define SCS_BUILD_SHARED 2
/* SCS_BUILD_UPPER (world > 1, every rank passes it or none does; not together with
 * SCS_BUILD_SHARED): W is symmetric, so the job keeps only its upper triangle.  Rank r builds the
 * tiles on and right of the diagonal of ITS rows and nothing else -- every cell is evaluated
 * once across the job, there is NO exchange, and the rank stores (row_end - row_begin) x
 * (V - row_begin) doubles instead of (row_end - row_begin) x V.  row_begin must be a multiple
 * of 256 (the tile width); splits that balance the trapezoids' areas come from the host
 * (partition.row_splits_upper).  scs_fiedler applies the operator from these tiles twice
 * (directly and transposed), all-gathers the ranks' V x b partial products and adds them in
 * rank order -- half the streamed bytes of the row-partitioned solve at every world size, the
 * same bits on every rank.  Such a graph cannot be contracted (scs_graph_contract needs whole
 * rows: SCS_EUNSUP); scs_graph_download_rows returns zeros left of the rank's first column. */
#define SCS_BUILD_UPPER 4
/* SCS_BUILD_SCATTER (with SCS_BUILD_MONOTONE, one rank, the whole matrix): the input-stationary
 * COMPARISON variant -- one workgroup per 64 x 64 block of leaf pairs of a tree, fp64 atomicAdd
 * into W (both triangles).  Same sums up to the order of the additions (<= 1e-12 relative, not
 * bit-exact), two orders of magnitude slower than the ordered tile kernel on random 8-byte
 * read-modify-writes; kept so that the choice is a measured one (profiles/). */
#define SCS_BUILD_SCATTER 8
int scs_pcg_build(scs_ctx *ctx, const scs_tables *tables, int32_t row_begin, int32_t row_end,
                  int32_t flags, scs_graph **out, scs_build_stats *stats);

/* Contract consecutive index ranges into single vertices: vertex g of the new
 * graph is rows/columns [group_start[g], group_start[g+1]) of the old one,
 * W'[g][h] = max over member pairs, diagonal 0 (reference: scs.py:336-387; the
 * host has already relabelled taxa so that every contraction group is a
 * consecutive range that does not straddle a rank's row block).
 * group_start: int32 [n_groups+1], group_start[0] == 0, last == old V.
 * The input graph is consumed (freed) and *out receives the contracted one. */
int scs_graph_contract(scs_ctx *ctx, scs_graph *graph, const int32_t *group_start,
                       int32_t n_groups, scs_graph **out);

/* Shape of this rank's block. */
int scs_graph_shape(const scs_graph *graph, int32_t *n_vertices, int32_t *row_begin,
                    int32_t *row_end);

/* Dense copy of this rank's rows to the host: out is (row_end-row_begin) x V,
 * row-major, caller-owned.  For tests and golden vectors. */
int scs_graph_download(scs_ctx *ctx, const scs_graph *graph, double *out);

/* Rows [first, first+count) of the graph (global row indices, inside this
 * rank's block) to the host: out is count x V row-major. */
int scs_graph_download_rows(scs_ctx *ctx, const scs_graph *graph, int32_t first, int32_t count,
                            double *out);

/* Row sums of this rank's rows (the degree vector d of scipy's normalized
 * Laplacian, scipy/sparse/csgraph/_laplacian.py:550): out has row_end-row_begin
 * entries. */
int scs_graph_degrees(scs_ctx *ctx, scs_graph *graph, double *out);

int scs_graph_free(scs_ctx *ctx, scs_graph *graph);

/* ---- Fiedler solve ----------------------------------------------------- */

/* The V x 2 spectral embedding scikit-learn's SpectralClustering clusters
 * (replaces sklearn/manifold/_spectral_embedding.py:299-467 as reached from
 * scs.py:252): column 0 <-> eigenvalue 1 of S = D^-1/2 A D^-1/2, column 1 the
 * Fiedler vector; unit-norm eigenvectors divided elementwise by sqrt(degree)
 * (1 where the degree is 0), each column sign-flipped so its entry of largest
 * magnitude is positive.
 *   x_init   fp64 [V] or NULL   start vector for the first block column (the
 *                               reference's ARPACK v0 draw, sklearn/utils/_arpack.py:31-33)
 *   tol      residual target: ||S x - lambda x||_2 <= tol (unit x)
 *   max_iter LOBPCG iteration cap
 *   block    LOBPCG block width (<= 16); 0 picks the default
 *   maps_out fp64 [V*2] row-major, caller-owned; every rank receives all V rows
 * Collective over the context's communicator when world > 1.
 * Returns SCS_ENOCONV when the wanted pair(s) stopped above tol (iteration cap, or the
 * residual stopped improving): maps_out and stats then hold the block that was reached
 * and the caller decides (the host retries wider, then warns or raises). */
int scs_fiedler(scs_ctx *ctx, scs_graph *graph, const double *x_init, double tol,
                int32_t max_iter, int32_t block, double *maps_out, scs_stats *stats);

/* A MEASURED COMPARISON, not the product path: a graph WITHOUT its matrix.  scs_fiedler on
 * it applies W straight from the flattened tables (per tree one sweep from the left and one from the right
 * over the leaves, a stack of (depth, value, sum) per sweep; trees added in order) -- scs_pcg_build is not run
 * at all.  One device, more than 128 taxa, block widths 4 and 8 (max_block: the widest the graph's buffers are
 * made for); the tables must outlive the graph; no contraction, no download.  Results agree with the dense
 * path to rounding, not bit for bit.  Free with scs_graph_free. */
int scs_graph_matrix_free(scs_ctx *ctx, const scs_tables *tables, int32_t max_block, scs_graph **out);

/* What scs_graph_matrix_free planned for a matrix-free graph and where the graph stands, from host fields alone: no
 * launch, nothing on the device changes (tests/test_gpu_matrix_free_edges.py).  info_out[6]: [0] chunks a tree's
 * leaves are cut into per direction, [1] stack_total, the entries of all strips of one (direction, column, chunk) --
 * the sum over the trees of (deepest separator + 1), [2] the widest block the buffers are made for, [3] the block
 * width the slabs were last written with (0: never), [4] operator applications so far (the degrees count as one),
 * [5] the number of trees.  maxd_out (n_trees x int32, may be NULL): per tree the deepest separator the device found
 * at creation, which sizes that tree's strips.  SCS_EINVAL for a graph that has a matrix. */
int scs_debug_matrix_free_plan(const scs_graph *graph, int64_t *info_out, int32_t *maxd_out);

/* ---- batched small nodes ----------------------------------------------- */

/* Deep recursion levels (reference: scs.py:110-134 at depth): K
 * independent nodes of at most 128 taxa each (round 4; 64 before), the batch spread over the
 * chip in three launches.  Every node goes from its flattened tables to the V x 2 embedding: proper-cluster-graph weights
 * (bit-identical to scs_pcg_build's W), contraction of consecutive id ranges (max over member
 * pairs, scs.py:336-387), scipy's degree scaling, full Jacobi eigen-decomposition in LDS
 * (two-sided up to 64 vertices, one-sided up to 128),
 * scikit-learn's embedding conventions (as scs_fiedler).  Replaces, per node,
 * scs_tables_upload + scs_pcg_build + scs_graph_contract + scs_fiedler.
 *   n_taxa, n_trees, n_groups  int32 [K]   (2 <= n_groups <= n_taxa <= 128)
 *   tree_off    int32, per node n_trees+1 leaf offsets starting at 0, nodes concatenated
 *   leaf_taxon / adj_depth / adj_val       the nodes' tables, concatenated (taxon ids 0..n_taxa-1,
 *                                          numbered so that every contraction group is a
 *                                          consecutive range)
 *   tree_w      fp64, n_trees per node, concatenated
 *   group_start int32, per node n_groups+1 entries 0 .. n_taxa, concatenated
 *   maps_out    fp64 [sum n_groups][2]     lambda_out fp64 [K][3] (three largest eigenvalues of S)
 *   w_out       fp64, per node n_groups^2 (row-major), concatenated, or NULL */
int scs_small_solve(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa, const int32_t *n_trees,
                    const int32_t *n_groups, const int32_t *tree_off, const int32_t *leaf_taxon,
                    const int32_t *adj_depth, const double *adj_val, const double *tree_w,
                    const int32_t *group_start, double *maps_out, double *lambda_out,
                    double *w_out);

/* The same in two halves.  _begin copies the inputs into a page-locked block of the context,
 * enqueues the upload, the three launches and the download of the results and returns a ticket
 * without waiting; _end waits for that ticket's results and copies them out (NULL outputs: the
 * results are dropped).  Several tickets may be outstanding on a context; they complete in the
 * order they were begun.  The recursion begins a child's solve as soon as its tables are
 * flattened: the next child is flattened on the host meanwhile, and a right sibling's embedding is
 * long there when the walk arrives (reference order of the walk: scs.py:139-171).
 * want_w != 0: the contracted weight matrices are kept for _end's w_out.  The input arrays may be
 * reused as soon as _begin returns. */
int scs_small_solve_begin(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa,
                          const int32_t *n_trees, const int32_t *n_groups, const int32_t *tree_off,
                          const int32_t *leaf_taxon, const int32_t *adj_depth, const double *adj_val,
                          const double *tree_w, const int32_t *group_start, int32_t want_w,
                          int32_t *ticket_out);
/* scs_small_solve_begin for ONE node whose tables are resident -- a child of scs_forest_split
 * (declared above): its leaf arrays are packed on the device, only the group boundaries and the
 * renumbering travel.  relabel[x] (may be null: identity) = id of the forest's taxon x in the node's
 * numbering (present taxa only, contraction groups consecutive); n_taxa = the node's taxon count. */
int scs_small_solve_begin_forest(scs_ctx *ctx, const scs_forest *forest, const int32_t *relabel,
                                 int32_t n_taxa, int32_t n_groups, const int32_t *group_start,
                                 int32_t want_w, int32_t *ticket_out);
/* scs_small_solve_begin for the K small nodes of ONE LEVEL of the recursion, straight from the level
 * forest's resident tables (scs_forest_split_level; reference: scs.py:110-134 for every node of the
 * level): node k owns the trees [t_begin[k], t_begin[k] + n_trees[k]) with n_leaves[k] leaves in all and
 * the taxon ids [u_base[k], u_base[k] + u_size[k]); relabel (all nodes' maps concatenated, u_size[k]
 * entries each) sends id x to relabel[.. + x - u_base[k]], the node's own numbering (present taxa only,
 * contraction groups consecutive); n_taxa / n_groups / group_start as scs_small_solve_begin. */
int scs_small_solve_begin_level(scs_ctx *ctx, const scs_forest *forest, int32_t n_nodes,
                                const int32_t *t_begin, const int32_t *n_trees, const int64_t *n_leaves,
                                const int32_t *u_base, const int32_t *u_size, const int32_t *relabel,
                                const int32_t *n_taxa, const int32_t *n_groups, const int32_t *group_start,
                                int32_t want_w, int32_t *ticket_out);
int scs_small_solve_end(scs_ctx *ctx, int32_t ticket, double *maps_out, double *lambda_out,
                        double *w_out);

/* ---- diagnostics used by the parity tests ------------------------------ */

/* The packed input arrays of a begun batch (a ticket of any of the three _begin entries that has not been
 * ended; it stays begun), copied from the batch's DEVICE block exactly as the solve's first kernel reads
 * them: tree_off [sum (n_trees[k] + 1)] (every node's offsets start at 0), leaf_taxon / adj_depth / adj_val
 * [sum of the nodes' leaves], tree_w [sum n_trees[k]].  Any pointer may be null.  Waits for the batch.  What
 * scs_small_solve_begin_forest and _level pack on the device is held against the host's packing with it. */
int scs_debug_small_inputs(scs_ctx *ctx, int32_t ticket, int32_t *tree_off, int32_t *leaf_taxon,
                           int32_t *adj_depth, double *adj_val, double *tree_w);

/* The five device arrays of a tables handle to the host -- tree_off [n_trees + 1], leaf_taxon / adj_depth /
 * adj_val [n_leaves], tree_w [n_trees]; any pointer may be null -- and info = {n_taxa, n_trees, n_leaves,
 * max_leaves} (may be null; a first call with null arrays gives the sizes).  Waits for an upload that is
 * still on its way.  What scs_tables_from_forest and _from_forest_range leave in a handle is read with it. */
int scs_debug_tables_download(scs_ctx *ctx, const scs_tables *tables, int64_t *tree_off, int32_t *leaf_taxon,
                              int32_t *adj_depth, double *adj_val, double *tree_w, int64_t *info);

/* The stop / renew / confirm rules of scs_fiedler's loop (csrc/scs_policy.h; what stands in for ARPACK's
 * tol = 0 behind scs.py:252) on a scripted sequence of residuals, no device involved: actions_out[i] = 0 go
 * on, 1 stop for the confirmation (the next residual of the script is the one measured through W), 2 renew
 * S X / S P through W, 3 / 4 the loop ended converged / not converged, -1 behind the end.  image != 0: the
 * loop starts on the single-precision image of W. */
int scs_debug_loop_policy(double tol, int32_t lowp_mode, double lowp_tol, double lowp_tol2, int32_t image,
                          int32_t n, const double *residuals, int32_t *actions_out);

/* Eigen-decomposition of a dense symmetric n x n matrix (n <= 64) by the
 * device Jacobi kernel that serves the Rayleigh-Ritz step: eigenvalues
 * descending in w[n], eigenvectors in the columns of v (n x n row-major). */
int scs_debug_jacobi(scs_ctx *ctx, const double *a, int32_t n, double *w, double *v);

/* out (ka x kb, row-major) = A^T B for host matrices A (n x ka), B (n x kb),
 * row-major, through the device Gram kernel; use_mfma selects the
 * v_mfma_f64_16x16x4_f64 variant. */
int scs_debug_gram(scs_ctx *ctx, const double *a, const double *b, int32_t n, int32_t ka,
                   int32_t kb, int32_t use_mfma, double *out);

/* y (rows x b) = S[row block] * x for a host x (V x b): one launch of the
 * SYMM kernel with the graph's degree scaling. */
int scs_debug_apply(scs_ctx *ctx, scs_graph *graph, const double *x, int32_t b, double *y);

/* scs_debug_apply through ONE solver object for `reps` consecutive applications, so that the symmetric
 * schedule's tile list runs forwards, backwards, forwards, ... as it does in scs_fiedler's loop: y_out
 * (reps x rows x b) receives every application's product.  image != 0: the single-precision image of W is
 * made if the graph has none and the products come from it (b = 4 only); a graph whose shape keeps
 * scs_fiedler from streaming an image (matrix-free, SCS_BUILD_UPPER, fewer than 4096 vertices, no memory) is
 * refused with an error, never served from W (the loop's own switches, SCS_LOWP and the legacy loop, are
 * not looked at).  info_out[8] reports what ran: [0] symmetric schedule
 * (k_symm_tri) or not (k_symm), [1] image, [2] tiles per application (0 for k_symm), [3] column
 * segments, [4] tile width in columns (0 for k_symm), [5] applications that streamed the image,
 * [6] SCS_BUILD_UPPER partial products, [7] matrix-free.  The partial-sum buffers are filled with NaN
 * patterns before every application: a partial sum no tile wrote shows in the product. */
int scs_debug_apply_ex(scs_ctx *ctx, scs_graph *graph, const double *x, int32_t b, int32_t image,
                       int32_t reps, double *y_out, int32_t *info_out);

/* The operator as a multi-rank solve assembles it.  COLLECTIVE: every rank of the job calls it with the same
 * arguments.  A solver is set up exactly as scs_fiedler sets it up for this graph (row splits gathered, chunk =
 * the longest slice x b, receive buffer, the SCS_BUILD_UPPER rank's tile lists) and S is applied `reps` times
 * on that one object to the R block (columns 2b ... 3b-1) of the host panel q (V x 3b, row-major; aq likewise)
 * by path 0, solver::apply (scale, SYMM, all-gather, unpack -- SCS_BUILD_UPPER: sum of the ranks' partial
 * products --, store into AQ's R slot; b = 4, 8, 12, 16, SCS_BUILD_UPPER graphs 4 and 8), or path 1, the
 * fused loop's back half with the second pass in front (SYMM, all-gather, the Gram kernel that assembles AQ's
 * R slot on its way, the reduction of its partials; b = 4, 8).  y_out (reps x V x b): AQ's R slot after every
 * application, ALL V rows as this rank holds them.  qaq_out (reps x 3b x 3b; path 1, else may be null): Q^T AQ.
 * part_out (reps x V x b; SCS_BUILD_UPPER graphs, else may be null): this rank's own unscaled partial product.
 * image != 0: the ranks stream the single-precision image of their rows -- only where scs_fiedler does
 * (more than one rank, not SCS_BUILD_UPPER, V >= 4096, b = 4); refused with SCS_EUNSUP otherwise, on every
 * rank alike and behind the same collectives, never served from W.  info_out[8]: [0] layout (0 row slices,
 * 1 partial products), [1] path, [2] ranks, [3] chunk in doubles, [4] column segments (partial products:
 * ranks) of the last SYMM, [5] tiles per application (0 for k_symm), [6] applications that streamed the
 * image, [7] all-gathers made.  Every buffer an application adds up or unpacks, and AQ's R slot, is filled
 * with NaN patterns before it: what no rank wrote shows in the product. */
int scs_debug_team_apply(scs_ctx *ctx, scs_graph *graph, const double *q, const double *aq, int32_t b,
                         int32_t path, int32_t image, int32_t reps, double *y_out, double *qaq_out,
                         double *part_out, int64_t *info_out);

/* scs_debug_gram on column blocks of wider panels, as the solver calls it: out (ka x kb) = A^T B with
 * A = columns [a_col0, a_col0 + ka) of the host panel a (n x lda, row-major), B likewise; a == b with
 * lda == ldb is ONE device panel (two blocks of Q).  gram_blocks (1 ... 1024) caps the number of
 * per-workgroup partials, scs_fiedler's `gram_blocks`. */
int scs_debug_gram_ex(scs_ctx *ctx, const double *a, int32_t lda, int32_t a_col0, int32_t ka,
                      const double *b, int32_t ldb, int32_t b_col0, int32_t kb, int32_t n,
                      int32_t use_mfma, int32_t gram_blocks, double *out);

/* One launch of the panel update kernel on host operands: Y = alpha * Y + sign * A C with Y = columns
 * [y_col0, y_col0 + kc) of the panel y (n x ldy), A = columns [a_col0, a_col0 + ka) of a (n x lda), C
 * (ka x kc, leading dimension ldc); kc <= 16, ka <= 48.  The whole panel y comes back, so that the
 * columns beside the block can be checked.  a == y with lda == ldy is ONE device panel (in place, or two
 * blocks of Q). */
int scs_debug_update(scs_ctx *ctx, double *y, int32_t ldy, int32_t y_col0, int32_t kc, double alpha,
                     const double *a, int32_t lda, int32_t a_col0, int32_t ka, const double *c,
                     int32_t ldc, double sign, int32_t n);

/* The small solves and tall panel kernels of the LOBPCG loop, ONE launch of the product code each on host
 * arrays.  Every output and scratch buffer is filled with 0xFF bytes before the launch:
 * an entry nobody wrote comes back as NaN (doubles) or -1 (ints).
 *
 * scs_debug_small_svqb: one k_small_svqb launch on g (k x k, row-major), 1 <= k <= 64: t_out (k x k), mask_out (k). */
int scs_debug_small_svqb(scs_ctx *ctx, const double *g, int32_t k, double drop_tol, double *t_out,
                         int32_t *mask_out);

/* The Rayleigh-Ritz solve (small_rr_body) through the product kernels.  tm: nq x nq, or with nparts > 0 (nq <= 24
 * only) nparts partials of it that the kernel sums; mask: nq ints (live basis slots); 1 <= b <= 16, b <= nq <= 3b.
 * start = 0: k_small_rr, with exact_from handed through (-1: none).  start = 1: k_small_rr_start (nq = b, nparts = 0;
 * mask is not read).  start = 2: the same body with the one-wave direction path of nq = 3b, b = 4 or 8 switched off,
 * so that these sizes run the general path too (a debug kernel; the product never takes this switch).
 * c_out, d_out: nq x b; theta_out: b + 1; mask_p_out: b; mask_out: the 48 mask slots as the launch left them. */
int scs_debug_small_rr(scs_ctx *ctx, const double *tm, int32_t nparts, int32_t nq, int32_t b, const int32_t *mask,
                       double drop_tol, int32_t exact_from, int32_t start, double *c_out, double *d_out,
                       double *theta_out, int32_t *mask_p_out, int32_t *mask_out);

/* The projected SVQB (small_orth_core) on nparts (1 ... 1024) partials of 3 b^2 + b doubles each ([x p]^T r, r^T r,
 * u^T r).  layout 0: k_small_orth (b <= 8: its working set holds no wider block); layout 1 (b = 4 or 8): a debug
 * kernel that declares the compact orth_small_lds<b> and calls small_orth_core on it as k_symm_tri_tf does.
 * theta: b + 1 values for the report.  coef_out: (3b + 4) x b; mask_out: b; report_out: 41 doubles of ordinary
 * device memory, written with a sequence number of 7 (slots [0, b), [16, 16 + b] and [40]). */
int scs_debug_small_orth(scs_ctx *ctx, const double *partial, int32_t nparts, int32_t b, double drop_tol,
                         const double *theta, int32_t layout, double *coef_out, int32_t *mask_out,
                         double *report_out);

/* One launch of one tall kernel on the panels q, aq ((n + SCS_DEBUG_PANEL_PAD) x 3b, row-major; the rows past n
 * are the caller's sentinels and travel both ways, as do the columns the kernel leaves alone).  which:
 *   0 k_panel_rr<b>: coef_a = c, coef_b = d (3b x b each), theta (b); partial_out: blocks x (3 b^2 + b);
 *   1 k_panel_tf<b, Gram>: coef_a ((3b + 4) x b); partial_out as 0;
 *   2 k_panel_tf<b, writes Z>: coef_a, dinv; zt_out (b x (n + pad), k-major, leading dimension n + pad) goes in
 *     with the caller's sentinels and comes back with the launch's stores;
 *   3 k_gram_qaq<b, 0>: partial_out: blocks x (3b x 3b);
 *   4 k_gram_qaq<b, 1>: ypart ((nseg x n + pad) x b, nseg in 1 ... 4), dinv; aq_out gets AR; partial_out as 3;
 *   5 k_rr_update on q with nq = 3b: coef_a = c, coef_b = d; its own grid ((n + 15) / 16 workgroups);
 *   6 k_residual: theta (b); partial_out: (n + 255) / 256 x b squared norms, one row per workgroup.
 * 0 ... 4 take b = 4, 8 and blocks in 1 ... 128 (the grid); 5 and 6 take b = 4, 8, 12, 16.  u, dinv: n + pad
 * entries; u may be null (unconstrained).  The per-workgroup partials come back unsummed.  q_out, aq_out (may be
 * null): the panels after the launch. */
#define SCS_DEBUG_PANEL_PAD 16
int scs_debug_panel(scs_ctx *ctx, int32_t which, int32_t b, int32_t n, const double *q, const double *aq,
                    const double *u, const double *coef_a, const double *coef_b, const double *theta,
                    const double *dinv, const double *ypart, int32_t nseg, int32_t blocks, double *q_out,
                    double *aq_out, double *partial_out, double *zt_out);

/* One grouped round of ncclSend + ncclRecv from this rank to itself through the wrapper the
 * shared build's tile exchange uses (ncclGroupStart ... ncclGroupEnd, ncclFloat64, the
 * context's stream): host_out receives host_in (count doubles).  Needs a context created
 * with an RCCL communicator (scs_ctx_create with world >= 1 and a unique id). */
int scs_debug_comm_selftest(scs_ctx *ctx, int32_t count, const double *host_in, double *host_out);

/* The box's own copy rate, to quote beside the nominal 8 TB/s (SURVEY.md 8d "Peak to quote"):
 * `reps` device-to-device copies of `bytes` bytes on the context's stream, timed with HIP
 * events after one untimed copy; *gbs_out = 2 * bytes * reps / time in GB/s (a copy reads
 * and writes every byte once). */
int scs_debug_copy_bandwidth(scs_ctx *ctx, int64_t bytes, int32_t reps, double *gbs_out);

/* The multi-block exclusive scan that carries the node-parallel forest split, the offsets of a level's
 * trees and the analysis (csrc/scs_forest.hip, 4096 items per workgroup; the same code the product runs) on
 * host rows: out[part][i] = op over in[part][j], j < i, for i in [0, n] -- entry n is the row's total.  op 0:
 * sum (identity 0), op 1: maximum (identity -1).  in is n_parts x n, out n_parts x (n + 1), row-major;
 * 1 <= n_parts <= 8. */
int scs_debug_scan(scs_ctx *ctx, int32_t op, int32_t n_parts, int64_t n, const int32_t *in, int32_t *out);

/* The stored block of a graph as it lies in device memory, padding columns included: what = 0 the rows of W
 * (rows x ld doubles), what = 1 the single-precision image (rows x ld floats), made if the graph has none by the
 * degree pass the solver runs, what = 2 the degrees of ALL V vertices as this rank holds them (V doubles; what the
 * solver scales by).  Modes 1 and 2 are collective over the communicator when world > 1 and the degrees are not
 * known yet; nothing else is run.  info_out[4]: [0] rows, [1] ld (elements), [2] the first stored column (SCS_BUILD_UPPER
 * graphs store columns [col0, V)), [3] image only: 1 when whole rows are defined (a row-partitioned rank), 0 when
 * row r (global) is defined from column (r / 512) * 512 on.  out may be NULL: info_out alone is filled (no image is
 * made).  SCS_EUNSUP, never something else, where the library makes no image: a matrix-free graph (what = 0 as
 * well: it has no matrix), an SCS_BUILD_UPPER graph, a row block on one rank, no memory. */
int scs_debug_graph_raw(scs_ctx *ctx, scs_graph *graph, int32_t what, void *out, int32_t *info_out);

/* The block records of the trees [t_begin, t_end) for the 64-row blocks of rows [row_begin, row_end), made by the
 * build's own preparation (positions, range-minimum and argmin tables, one record kernel) as ONE batch in one piece
 * (tests/test_gpu_prep_records.py).  kind: 0 k_block_records_mono, 1 k_block_records_wide, 2 k_block_records_gen
 * (pair tables); 0 and 1 take the tables as monotone, whatever they are.  With B = ceil((row_end - row_begin) / 64)
 * blocks and T trees, per (block b, tree t) at index b * T + t: spos_out 64 x int32, the sorted DFS positions of the
 * block's rows (INT32_MAX beyond the count); gap_out 64 x double, entry k the value of the shallowest gap in
 * [spos[k], spos[k + 1]) (0 beyond count - 1); argpos_out 64 x int32, the position the record names for that gap --
 * the LEFTMOST one that attains the minimum (W cannot show which: every position of the minimum gives the same
 * cells); depth_out 64 x int32, kind 2 only (else untouched, may be NULL): the gap's depth; cnt_out one int32, the
 * rows of the block the tree holds. */
int scs_debug_block_records(scs_ctx *ctx, const scs_tables *tables, int32_t t_begin, int32_t t_end, int32_t row_begin,
                            int32_t row_end, int32_t kind, int32_t *spos_out, double *gap_out, int32_t *argpos_out,
                            int32_t *depth_out, int32_t *cnt_out);

/* The plan of the thread-per-tree split kernels for a forest's offsets (node_off[n_trees + 1]), by the launcher's
 * rule and the kernels' predicate, on the host (no device): *tpb_out trees per workgroup (64 ... 8),
 * *n_groups_out workgroups, staged_out[g] = 1 where workgroup g copies its trees to LDS (at most SPLIT_CAP nodes),
 * 0 where it walks them in place.  staged_out holds (n_trees + 7) / 8 bytes at least. */
int scs_debug_split_plan(int32_t n_trees, const int64_t *node_off, int32_t *tpb_out, int32_t *n_groups_out,
                         uint8_t *staged_out);

/* The plan of one scs_score_* call on the host (no device work, no device memory): the batches sc_begin makes of the
 * source trees and what scs_score_triplets decides per batch, by the functions the exports call.  The trees are
 * those of `sources`, or, when `sources` is NULL, tree_off[n_trees + 1] (with `sources`, n_trees must be its tree
 * count and tree_off is not read).  super_leaves: the supertree's tips; max_batch_trees as for the exports;
 * extra_per_leaf / extra_per_tree: the export's own workspace bytes per leaf and per tree of a batch (0 / 0 for
 * scs_score_supertree and scs_score_concordance, 32 / 8 for scs_score_triplets, 8 * levels + 8 / 0 for
 * scs_score_conflicts).  *n_batches_out batches; bstart_out[n_batches + 1] (room for n_trees + 1) the first tree of
 * every batch and n_trees; info_out[2] = {levels of the per-tree tables, row stride in entries}; per batch (room for
 * max(n_trees, 1)): words_out the 32-bit words of a bitset row of the pair kernel, zb_out its S' nodes per workgroup,
 * wg_out its workgroups. */
int scs_debug_score_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t super_leaves,
                         int32_t max_batch_trees, int64_t extra_per_leaf, int64_t extra_per_tree,
                         int32_t *n_batches_out, int32_t *bstart_out, int64_t *info_out, int32_t *words_out,
                         int32_t *zb_out, int64_t *wg_out);

/* The same for scs_score_branch_triplets / scs_score_branch_resample (one plan: both call sc_plan_pairs) and for
 * scs_score_taxon_triplets, on the host, by the functions those exports call.  Inputs as for scs_debug_score_plan
 * (extra_per_leaf / extra_per_tree: 40 / 8 for the branch export, 40 / 8 + 32 x supertree nodes for the resample,
 * 72 / 24 for the taxon export) and max_lds_bytes as for scs_score_taxon_triplets (0: no cap).  *n_batches_out and
 * bstart_out as there.  bt_out[4 x batch] = {words, zb, dynamic LDS bytes of the launch, workgroups} of k_bt_pairs /
 * k_rs_pairs.  tx_out[14 x batch]: for each of the three LDS bins {zb, dcap (0: the bin is not used and not
 * launched), dynamic LDS bytes, workgroups} of k_tx_pairs<false>, then 1 when the batch launches the slab kernel, and
 * the dynamic LDS bytes of that launch.
 * call_out[3] = {need_slab, slab_wgs, slab_stride} of the call.  Room for max(n_trees, 1) batches in bt_out and
 * tx_out. */
int scs_debug_branch_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t super_leaves,
                          int32_t max_batch_trees, int64_t extra_per_leaf, int64_t extra_per_tree,
                          int32_t max_lds_bytes, int32_t *n_batches_out, int32_t *bstart_out, int64_t *bt_out,
                          int64_t *tx_out, int64_t *call_out);

/* The same for scs_score_placements, scs_score_clade_placements / scs_score_clade_moves (one plan) and
 * scs_score_polytomies, on the host, by the functions those exports call.  Trees, super_leaves, max_batch_trees and
 * max_lds_bytes as for scs_debug_branch_plan; the workspace bytes per leaf and per tree are the exports' own, from
 * n_queries (query taxa of the placements), n_sub_queries (tips of all query clades) and degrees[n_degrees] (the
 * children, 3 to 64, of every query node of the polytomies; n_degrees may be 0).  Export x = 0 placements, 1 clades,
 * 2 polytomies: n_batches_out[x] batches, bstart_out[x * (n_trees + 1) ...] the first tree of every batch and n_trees.
 * pl_out / cp_out[6 x batch] = {words, zb, 1 when the sums of a pass lie in LDS beside the rows, dynamic LDS bytes of
 * k_pl_pairs / k_cp_pairs for a full pass, the same for the last pass, workgroups of one launch};
 * blk_out[x * (n_trees + 1) + t], x = 0, 1: the first pair workgroup of tree t (and the total at n_trees).
 * py_out[4 x (batch * n_degrees + i)] = {W words per row, Ws the rows' stride in LDS, 1 when the k^2 sums lie in LDS,
 * dynamic LDS bytes of k_py_sweep} for degrees[i] (whether they fit the cap is scs_score_polytomies' own refusal).
 * Room for max(n_trees, 1) batches in pl_out, cp_out and py_out. */
int scs_debug_placement_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t super_leaves,
                             int32_t max_batch_trees, int32_t max_lds_bytes, int32_t n_queries,
                             int32_t n_sub_queries, int32_t n_degrees, const int32_t *degrees, int32_t *n_batches_out,
                             int32_t *bstart_out, int64_t *pl_out, int64_t *cp_out, int64_t *blk_out, int64_t *py_out);

/* The plan of one scs_score_parsimony call on the host, by the functions the export calls.  Trees and
 * max_batch_trees as for scs_debug_score_plan; chars[n_trees]: the characters of every tree (NULL: leaves - 2, the
 * most a tree can have); parent[n_nodes]: the supertree (root -1, every other parent an earlier node; SCS_EINVAL
 * otherwise); max_pass_words as for the export.  *n_batches_out and bstart_out as there.  info_out[8] = {words of a
 * tree one pass covers, frames a fold may open on the supertree laid out largest child first, slices of a frame's
 * counter, dynamic LDS bytes of a fold workgroup (0 when the frames lie in the call's block), 1 when they do,
 * workspace bytes per leaf, per tree, the supertree's tips}; batch_out[2 x batch] = {passes, words of the batch's
 * largest character set}.  Room for max(n_trees, 1) batches in batch_out. */
int scs_debug_parsimony_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, const int64_t *chars,
                             int32_t n_nodes, const int32_t *parent, int32_t max_batch_trees, int32_t max_pass_words,
                             int32_t *n_batches_out, int32_t *bstart_out, int64_t *info_out, int64_t *batch_out);

/* The plan of one scs_score_source_pairs call on the host, by the functions the export calls.  Trees as for
 * scs_debug_score_plan (n_taxa is read when `sources` is NULL); n_rows, max_batch_trees and max_lds_bytes as for the
 * export.  *n_batches_out batches, the same on both axes of the pair matrix; bstart_out[n_batches + 1] (room for
 * n_trees + 1).
 * info_out[6] = {levels of the per-tree min tables, stride of a dense position row in entries, bytes of one slab (0:
 * no pair of the call needs one), persistent workgroups of a slab launch, workspace bytes of the call with all four
 * outputs asked for, the LDS bytes a pair workgroup may take}.
 * tile_out (may be NULL; room for n_batches x n_batches x 7), per row batch I and column batch J:
 *   {entry width in bytes (2: both batches' trees have fewer than 65 536 leaves, else 4),
 *    dynamic LDS bytes of the pair launch,
 *    1 when the tile also launches the slab kernel,
 *    the bytes the tile's largest pair needs,
 *    threads of a pair workgroup (256, or more while the LDS leaves a CU room for fewer than 32 waves),
 *    the workgroups one launch may have (2^30, and no more work-items than a dispatch counts in 32 bits),
 *    the rows of the tile one launch takes under that limit (at least 1: a longer row is strided over)}.
 * A pair goes to the slab when its own bytes exceed the launch's; the fourth entry of a tile of one tree by one tree
 * is a pair's bytes. */
int scs_debug_source_pairs_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t n_taxa,
                                int32_t n_rows, int32_t max_batch_trees, int32_t max_lds_bytes, int32_t *n_batches_out,
                                int32_t *bstart_out, int64_t *info_out, int64_t *tile_out);

/* The plan of one scs_score_source_pair_triplets call on the host, by the functions the export calls.  Trees as for
 * scs_debug_source_pairs_plan; n_rows, rows and the three knobs as for the export (the chunks depend on which trees
 * the rows are).  Batches as scs_debug_source_pairs_plan reports them without an LDS cap.
 * info_out[8] = {levels of the per-tree min tables, stride of a dense position row in entries, the LDS bytes a
 * workgroup may take, the common taxa up to which a pair is finished in the restrict kernel (64), workspace bytes of
 * the call with all four outputs asked for, of which the regions of a chunk, the workgroups one launch may have, the
 * chunks of the call}.
 * tile_out (may be NULL; room for n_batches x n_batches x 12), per row batch I and column batch J (zeros: no launch):
 *   {rows of the tile, the common taxa a pair of it may have (the smaller of its largest row and column tree),
 *    words of a bitset row, nodes of B a sweep workgroup takes (zb), dynamic LDS bytes of the sweep launch,
 *    dynamic LDS bytes of the restrict launch, 1 when the tile also launches the restrict kernel over the regions,
 *    the LDS bytes its largest pair's restriction needs, bytes of a pair's region, pairs of a chunk at most,
 *    pairs of the tile (rows x column trees), chunks of the tile}.
 * chunk_out (may be NULL; room for 8 x the chunks, which a first call returns in info_out[7]), in launch order:
 *   {I, J, first pair of the tile (row-major), pairs (= workgroups of the restrict launch), of which pairs the host
 *    knows to finish in the restrict kernel (the smaller tree has at most 64 leaves), of which pairs the mirror
 *    leaves out, workgroups of the sweep launch, rows of the tile the chunk touches}.
 * SCS_EINVAL also for the sizes the export refuses, with its message. */
int scs_debug_source_pair_triplets_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off,
                                        int32_t n_taxa, int32_t n_rows, const int32_t *rows, int32_t max_batch_trees,
                                        int32_t max_lds_bytes, int32_t max_chunk_pairs, int32_t *n_batches_out,
                                        int32_t *bstart_out, int64_t *info_out, int64_t *tile_out, int64_t *chunk_out);

/* The plan of one scs_score_coverage call on the host, by the functions the export calls.  `sources` or, when it is
 * NULL, n_trees and n_taxa (tree_off is not read: the plan depends on the tree count alone).  n_rows < 0 stands for
 * rows NULL (every taxon); min_trees, max_batch_rows and max_reg_words as for the export; matrices_wanted: how many
 * of pair_trees / pair_covered are asked for (0, 1 or 2).
 * info_out[12] = {words per taxon (⌈trees/32⌉, at least 1),
 *   the sweep variant: words a lane holds in registers (4, 8, 16, 32 or 64), or 0 for the streaming kernel,
 *   stride of a taxon-major membership row in words, stride of a word-major row in taxa (n rounded up to 64),
 *   tiles of 64 column taxa per row (one workgroup each),
 *   bytes a row adds to the call's block (8 and its cells of the matrices wanted),
 *   bytes of the block without the matrices,
 *   row batches,
 *   the workgroups one launch may have (2^30, and no more work-items than a dispatch counts in 32 bits),
 *   the rows one launch takes under that limit (at least 1: a longer row is strided over),
 *   1 when only pairs a < b are swept and both cells written (rows NULL, and the matrices, if wanted, hold every row
 *   at once), 1 when the lanes count trees (min_trees > 1) instead of testing for one}.
 * batches_out (may be NULL; room for 4 x the batches, which a first call with NULL returns in info_out[7]):
 *   {first row, rows, bytes of the call's block, workgroups of the batch's first launch}. */
int scs_debug_coverage_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t n_taxa,
                            int32_t n_rows, int32_t min_trees, int32_t max_batch_rows, int32_t max_reg_words,
                            int32_t matrices_wanted, int64_t *info_out, int64_t *batches_out);

/* The plan of one scs_score_internode call on the host, by the functions the export calls.  `sources` or, when it is
 * NULL, n_trees, tree_off[n_trees + 1] and n_taxa.  n_rows < 0 stands for rows NULL (every taxon); the two knobs as
 * for the export; matrices_wanted: how many of pair_weight / dist_sum / sq_sum are asked for (0 ... 3).
 * With `heights` (h_t per tree; `tree_w` per tree or NULL = 1; `squares` != 0 when a squared output is asked for) the
 * export's overflow rule is applied too, and its SCS_EINVAL returned after the plan is written.
 * info_out[16] = {levels of the min tables (2^levels > the largest tree), bytes of an entry of the table of r (4: the
 *   one width there is), words per taxon (⌈trees/32⌉, at least 1), stride of a dense row in taxa (n rounded up to 64),
 *   tiles of 256 column taxa per row, tiles of one work item, work items (workgroups) per row,
 *   bytes of a row's cells in the matrices wanted, rows of a row batch at most,
 *   bytes of the block without the matrices, bytes of the block with them,
 *   row batches, tree batches,
 *   the workgroups one launch may have (2^30, and no more work-items than a dispatch counts in 32 bits),
 *   the rows one launch takes under that limit (at least 1: a longer row is strided over),
 *   1 when only pairs a < b are swept and both cells written (rows NULL, and the matrices, if wanted, hold every row
 *   at once)}.
 * rows_out (may be NULL; 3 x the row batches): {first row, rows, workgroups of the batch's first launch}.
 * trees_out (may be NULL; 3 x the tree batches): {first tree, trees, leaves}.  A first call with both NULL returns
 * the two counts in info_out[11] and info_out[12]. */
int scs_debug_internode_plan(const scs_tables *sources, int32_t n_trees, const int64_t *tree_off, int32_t n_taxa,
                             int32_t n_rows, int32_t max_batch_rows, int32_t max_batch_trees, int32_t matrices_wanted,
                             const int64_t *tree_w, const int32_t *heights, int32_t squares, int64_t *info_out,
                             int64_t *rows_out, int64_t *trees_out);

/* The depth pass of scs_score_internode alone, downloaded from the arrays its sweep reads: gap_r[leaves] (r of the gap
 * after every leaf, by global leaf index; 0 at a tree's last leaf, which has no gap), leaf_depth[leaves] and
 * tree_height[n_trees] (h_t, the largest leaf depth; 0 for a tree of one leaf).  Any output may be null.
 * max_batch_trees as for the export.  SCS_EINVAL as the export's device check. */
int scs_debug_internode_depths(scs_ctx *ctx, const scs_tables *sources, int32_t max_batch_trees, int32_t *gap_r,
                               int32_t *leaf_depth, int32_t *tree_height);

#ifdef __cplusplus
}
#endif
#endif /* SCS_HIP_H */
