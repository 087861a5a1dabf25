// scs_score_supertree: how well a supertree S fits its source trees.
//
// Per source tree T (leaf set L(T), n = |L(T)|), with C(S|T) the nontrivial clusters {C ∩ L(T)} of S's clades and
// C(T) T's own: n_super = |C(S|T)|, n_source = |C(T)|, shared = |C(S|T) ∩ C(T)|.  Per node C of S: informative =
// #{T : 2 <= |C ∩ L(T)| < n}, supported = those of them whose C ∩ L(T) is a cluster of T.
//
// Everything works on T's flattened table (leaf_taxon, adj_depth in DFS order) and on S's leaf order:
//   1. k_score_scatter / k_score_compact: T's leaves sorted by their position in S -- a dense row per tree
//      (row[S position] = T position), compacted in order: sp[k] (S position), tp[k] (T position).
//   2. k_score_restrict: D[k] / U[k] = depth / node of LCA_S(sp[k], sp[k+1]), one range-minimum query on S's gap
//      table (packed depth << 32 | gap, so the minimum names the gap too).  D is the depth table of S|L(T).
//   3. k_score_nodes, per gap k: its restricted node u = U[k] covers the T leaves whose S position lies in u's leaf
//      range [sl(u), sr(u)]: [lo, hi] by two binary searches in sp.  k is the node's first gap iff k == lo or
//      LCA_S(sp[lo], sp[k]) lies below u.  T's own first gaps: the nearest gap to the left with depth <= adj[k]
//      is missing or strictly shallower (a binary descent on T's min table).
//   4. The restricted node (not the root) is a cluster of T iff its T positions a = min, b = max of tp[lo..hi]
//      span exactly hi - lo + 1 leaves and the LCA of leaves a..b (depth dT = min adj[a..b-1]) has no further
//      leaf on either side: a == 0 or adj[a-1] < dT, b == n-1 or adj[b] < dT.
//   5. The S nodes whose C ∩ L(T) equals the node's set are the path [u, w), w = the S node of its restricted
//      parent (the deeper of the bounding gaps lo-1 and hi): +1 at u, -1 at w; k_score_subtree sums the marks over
//      S's subtrees.  Integer atomics: exact and order-free.
// Trees go in batches (rows and per-tree sparse tables in one arena block); the W-build kernels are not involved.
#include <algorithm>
#include <cmath>
#include <vector>

#include "scs_internal.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_ROW_ALIGN = 1024;  // row stride: 256 threads x 4 entries of the compaction
constexpr uint64_t SC_BUDGET = (uint64_t)3 << 29;  // workspace bytes per batch (1.5 GB)

// tree of global leaf index p among the batch's trees [0, nb): off[t] <= p < off[t + 1]
__device__ __forceinline__ int sc_tree_of(const int64_t *__restrict__ off, int nb, int64_t p) {
    int a = 0, b = nb;  // off[a] <= p < off[b]
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (off[m] <= p) a = m; else b = m;
    }
    return a;
}

__device__ __forceinline__ int sc_log2(int64_t len) { return 63 - __clzll((unsigned long long)len); }

// range minimum over [l, r] of a sparse table with `stride` entries per level
template <typename T>
__device__ __forceinline__ T sc_rmq_min(const T *__restrict__ tab, int64_t stride, int64_t l, int64_t r) {
    const int j = sc_log2(r - l + 1);
    const T a = tab[j * stride + l], b = tab[j * stride + r - ((int64_t)1 << j) + 1];
    return a < b ? a : b;
}

__device__ __forceinline__ int2 sc_rmq_minmax(const int2 *__restrict__ tab, int64_t stride, int64_t l, int64_t r) {
    const int j = sc_log2(r - l + 1);
    const int2 a = tab[j * stride + l], b = tab[j * stride + r - ((int64_t)1 << j) + 1];
    return make_int2(min(a.x, b.x), max(a.y, b.y));
}

// per-tree counters: wave-aggregated when the whole wave works on one tree (the common case)
__device__ __forceinline__ void sc_count(unsigned long long *__restrict__ ctr, int t, bool hit) {
    const int t0 = __shfl(t, 0, 64);
    if (__all(t == t0)) {
        const unsigned long long n = __popcll(__ballot(hit));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(ctr + t0, n);
    } else if (hit) {
        atomicAdd(ctr + t, 1ull);
    }
}

// level j of a packed (uint64) or int32 min table / an int2 min-max table from level j - 1 (entries that would
// reach past the array keep level j - 1: no query of a tree reads them)
__global__ void k_score_level_u64(const uint64_t *__restrict__ prev, uint64_t *__restrict__ cur, int64_t n,
                                  int64_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t a = prev[i];
    cur[i] = (i + half < n) ? min(a, prev[i + half]) : a;
}

__global__ void k_score_level_tree(const int32_t *__restrict__ dprev, int32_t *__restrict__ dcur,
                                   const int2 *__restrict__ mprev, int2 *__restrict__ mcur, int64_t n, int64_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t d = dprev[i];
    const int2 m = mprev[i];
    if (i + half < n) {
        const int2 m2 = mprev[i + half];
        dcur[i] = min(d, dprev[i + half]);
        mcur[i] = make_int2(min(m.x, m2.x), max(m.y, m2.y));
    } else {
        dcur[i] = d;
        mcur[i] = m;
    }
}

// step 1a: row[t][S position of leaf p's taxon] = p - off[t]; flags: 1 taxon out of range, 2 taxon not in S,
// 4 a taxon twice in one tree
__global__ void k_score_scatter(const int64_t *__restrict__ off, int nb, const int32_t *__restrict__ leaf_taxon,
                                int32_t n_taxa, const int32_t *__restrict__ s_pos, int32_t *__restrict__ rows,
                                int64_t row_stride, unsigned *__restrict__ flags) {
    const int64_t p = off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    const int32_t x = leaf_taxon[p];
    if (x < 0 || x >= n_taxa) {
        atomicOr(flags, 1u);
        return;
    }
    const int32_t s = s_pos[x];
    if (s < 0) {
        atomicOr(flags, 2u);
        return;
    }
    if (atomicCAS(rows + (int64_t)t * row_stride + s, -1, (int32_t)(p - off[t])) != -1) atomicOr(flags, 4u);
}

// step 1b: one workgroup per tree compacts its row in S order: sp[k], tp[k] (as level 0 of the min-max table)
__global__ void __launch_bounds__(SC_THREADS) k_score_compact(const int64_t *__restrict__ off,
                                                              const int32_t *__restrict__ rows, int64_t row_stride,
                                                              int32_t *__restrict__ sp, int2 *__restrict__ mm0) {
    __shared__ int wave_sum[SC_THREADS / 64];
    const int t = blockIdx.x;
    const int64_t base = off[t] - off[0];
    const int4 *row = reinterpret_cast<const int4 *>(rows + (int64_t)t * row_stride);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t done = 0;
    for (int64_t c = 0; c < row_stride / 4; c += SC_THREADS) {
        const int4 v = row[c + threadIdx.x];
        const int cnt = (v.x >= 0) + (v.y >= 0) + (v.z >= 0) + (v.w >= 0);
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < SC_THREADS / 64; ++w) {
            before += (w < wave) ? wave_sum[w] : 0;
            total += wave_sum[w];
        }
        int64_t k = base + done + before + incl - cnt;
        const int32_t s0 = (int32_t)(4 * (c + threadIdx.x));
        const int32_t e[4] = {v.x, v.y, v.z, v.w};
        for (int i = 0; i < 4; ++i)
            if (e[i] >= 0) {
                sp[k] = s0 + i;
                mm0[k] = make_int2(e[i], e[i]);
                ++k;
            }
        done += total;
        __syncthreads();
    }
}

// step 2: depth and S node of LCA_S(sp[k], sp[k+1]) for every gap of every tree in the batch
__global__ void k_score_restrict(const int64_t *__restrict__ off, int nb, const int32_t *__restrict__ sp,
                                 const uint64_t *__restrict__ s_tab, int64_t s_stride,
                                 const int32_t *__restrict__ s_gap_node, int32_t *__restrict__ dep,
                                 int32_t *__restrict__ node) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // batch-relative leaf index
    const int64_t p = off[0] + q;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    if (p + 1 >= off[t + 1]) return;  // the last leaf of a tree has no gap
    const uint64_t m = sc_rmq_min(s_tab, s_stride, (int64_t)sp[q], (int64_t)sp[q + 1] - 1);
    dep[q] = (int32_t)(m >> 32);
    node[q] = s_gap_node[(uint32_t)m];
}

struct sc_nodes_args {
    const int64_t *off;          // tree_off + t0 (global leaf offsets of the batch's trees)
    int nb;                      // trees in the batch
    const int32_t *sp;           // [Lb] S positions in S order
    const int32_t *dep, *node;   // [Lb] D and U of the restricted tree
    const int2 *mm;              // min-max table of tp: level j at mm[j * Lb]
    const int32_t *adj;          // T's adj_depth of the batch (level 0 of the min table)
    const int32_t *amin;         // levels >= 1 of the min table of adj: level j at amin[(j - 1) * Lb]
    int levels;                  // levels of the batch's tables (2^levels > largest tree)
    int64_t Lb;
    const uint64_t *s_tab;       // S's packed gap table
    int64_t s_stride;
    const int32_t *s_lo, *s_hi;  // leaf range of every S node
    int32_t *mark_inf, *mark_sup;                   // [S nodes]
    unsigned long long *c_super, *c_source, *c_shared;  // [nb] of the batch
};

// min of adj over the batch-relative range [l, r] (r >= l)
__device__ __forceinline__ int32_t sc_adj_min(const sc_nodes_args &a, int64_t l, int64_t r) {
    const int j = sc_log2(r - l + 1);
    const int32_t *lev = j == 0 ? a.adj : a.amin + (int64_t)(j - 1) * a.Lb;
    return min(lev[l], lev[r - ((int64_t)1 << j) + 1]);
}

// steps 3 - 5, one thread per gap
__global__ void __launch_bounds__(SC_THREADS) k_score_nodes(sc_nodes_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];  // batch-relative first leaf of the tree
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    const bool gap = in && k + 1 < n;
    bool t_first = false, s_first = false, shared = false;
    if (gap) {
        // T's own first gap: nearest gap to the left with depth <= adj[k] is missing or shallower
        const int32_t d = a.adj[q];
        int64_t pos = k;  // exclusive end of the stretch of deeper gaps
        for (int j = a.levels - 1; j >= 0; --j) {
            const int64_t w = (int64_t)1 << j;
            if (pos >= w) {
                const int32_t *lev = j == 0 ? a.adj : a.amin + (int64_t)(j - 1) * a.Lb;
                if (lev[base + pos - w] > d) pos -= w;
            }
        }
        t_first = pos == 0 || a.adj[base + pos - 1] < d;

        const int32_t u = a.node[q], du = a.dep[q];
        const int32_t sl = a.s_lo[u], sr = a.s_hi[u];
        const int32_t *sp = a.sp + base;
        // lo: first k' with sp[k'] >= sl (<= k), hi: last with sp[k'] <= sr (>= k + 1)
        int64_t l0 = 0, l1 = k;
        while (l0 < l1) {
            const int64_t m = (l0 + l1) >> 1;
            if (sp[m] >= sl) l1 = m; else l0 = m + 1;
        }
        const int64_t lo = l0;
        int64_t h0 = k + 1, h1 = n - 1;
        while (h0 < h1) {
            const int64_t m = (h0 + h1 + 1) >> 1;
            if (sp[m] <= sr) h0 = m; else h1 = m - 1;
        }
        const int64_t hi = h0;
        s_first = lo == k || (int32_t)(sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[lo], (int64_t)sp[k] - 1) >> 32) > du;
        if (s_first && (lo > 0 || hi < n - 1)) {
            // restricted parent: the deeper of the bounding gaps
            int64_t g;
            if (lo == 0) g = hi;
            else if (hi == n - 1) g = lo - 1;
            else g = a.dep[base + lo - 1] >= a.dep[base + hi] ? lo - 1 : hi;
            const int32_t w = a.node[base + g];
            const int2 ab = sc_rmq_minmax(a.mm, a.Lb, base + lo, base + hi);
            if (ab.y - ab.x == hi - lo) {
                const int32_t dT = sc_adj_min(a, base + ab.x, base + ab.y - 1);
                shared = (ab.x == 0 || a.adj[base + ab.x - 1] < dT) && (ab.y == n - 1 || a.adj[base + ab.y] < dT);
            }
            atomicAdd(a.mark_inf + u, 1);
            atomicAdd(a.mark_inf + w, -1);
            if (shared) {
                atomicAdd(a.mark_sup + u, 1);
                atomicAdd(a.mark_sup + w, -1);
            }
        } else {
            s_first = false;  // (the restricted root: not a nontrivial cluster)
        }
    }
    sc_count(a.c_source, t, t_first);
    sc_count(a.c_super, t, s_first);
    sc_count(a.c_shared, t, shared);
}

// inclusive prefix sums of the two mark arrays, one workgroup (S has at most a few hundred thousand nodes)
__global__ void __launch_bounds__(1024) k_score_prefix(const int32_t *__restrict__ m0, const int32_t *__restrict__ m1,
                                                       int64_t n, int64_t *__restrict__ p0, int64_t *__restrict__ p1) {
    __shared__ int64_t ws[2][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t run0 = 0, run1 = 0;
    for (int64_t c = 0; c < n; c += 1024) {
        const int64_t i = c + threadIdx.x;
        int64_t x0 = i < n ? m0[i] : 0, x1 = i < n ? m1[i] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t y0 = __shfl_up(x0, d, 64), y1 = __shfl_up(x1, d, 64);
            if (lane >= d) {
                x0 += y0;
                x1 += y1;
            }
        }
        if (lane == 63) {
            ws[0][wave] = x0;
            ws[1][wave] = x1;
        }
        __syncthreads();
        int64_t b0 = run0, b1 = run1, t0 = 0, t1 = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) {
                b0 += ws[0][w];
                b1 += ws[1][w];
            }
            t0 += ws[0][w];
            t1 += ws[1][w];
        }
        if (i < n) {
            p0[i + 1] = b0 + x0;
            p1[i + 1] = b1 + x1;
        }
        run0 += t0;
        run1 += t1;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        p0[0] = 0;
        p1[0] = 0;
    }
}

// step 5: count of S node x = the marks of its subtree, preorder [x, end[x])
__global__ void k_score_subtree(const int64_t *__restrict__ p0, const int64_t *__restrict__ p1,
                                const int32_t *__restrict__ end, int64_t n, int64_t *__restrict__ inf,
                                int64_t *__restrict__ sup) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const int32_t e = end[x];
    inf[x] = p0[e] - p0[x];
    sup[x] = p1[e] - p1[x];
}

// levels of a sparse table over n entries: 2^levels > n (the binary descent's widest step covers any stretch)
int sc_levels_host(int64_t n) {
    int l = 1;
    while (((int64_t)1 << l) <= n) ++l;
    return l;
}

int grid_of(int64_t n) { return (int)std::max<int64_t>((n + SC_THREADS - 1) / SC_THREADS, 1); }

}  // namespace

extern "C" int scs_score_supertree(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                   const int32_t *taxon, int32_t max_batch_trees, int64_t *n_super,
                                   int64_t *n_source, int64_t *shared, int64_t *informative, int64_t *supported) {
    SCS_REQUIRE(ctx && src && parent && taxon, "scs_score_supertree: null argument");
    SCS_REQUIRE(n_nodes >= 1, "scs_score_supertree: the supertree has no node");
    SCS_REQUIRE(parent[0] == -1, "scs_score_supertree: node 0 must be the root (parent -1)");
    const int32_t n_taxa = src->n_taxa;
    // ---- the supertree's preorder arrays on the host: leaf ranges, subtree ends, gap table (O(nodes)) ----
    std::vector<int32_t> s_lo(n_nodes), s_hi(n_nodes), sub_end(n_nodes), depth(n_nodes), n_kids(n_nodes, 0);
    for (int32_t v = 1; v < n_nodes; ++v) {
        SCS_REQUIRE(parent[v] >= 0 && parent[v] < v, "scs_score_supertree: parent[%d] = %d is not an earlier node", v,
                    parent[v]);
        n_kids[parent[v]]++;
    }
    std::vector<int32_t> s_pos(std::max(n_taxa, 1), -1);
    int32_t n_leaves = 0;
    depth[0] = 0;
    for (int32_t v = 0; v < n_nodes; ++v) {
        if (v) depth[v] = depth[parent[v]] + 1;
        if (n_kids[v] == 0) {
            const int32_t x = taxon[v];
            SCS_REQUIRE(x >= 0, "scs_score_supertree: tip %d has no taxon", v);
            if (x < n_taxa) {
                SCS_REQUIRE(s_pos[x] < 0, "scs_score_supertree: taxon %d occurs twice in the supertree", x);
                s_pos[x] = n_leaves;
            }
            s_lo[v] = n_leaves;
            s_hi[v] = n_leaves;
            ++n_leaves;
        } else {
            SCS_REQUIRE(taxon[v] < 0, "scs_score_supertree: inner node %d carries a taxon", v);
            s_lo[v] = INT32_MAX;
            s_hi[v] = -1;
        }
        sub_end[v] = v + 1;
    }
    for (int32_t v = n_nodes - 1; v >= 1; --v) {  // (preorder: children after parents)
        const int32_t u = parent[v];
        s_lo[u] = std::min(s_lo[u], s_lo[v]);
        s_hi[u] = std::max(s_hi[u], s_hi[v]);
        sub_end[u] = std::max(sub_end[u], sub_end[v]);
    }
    // gap g (between S leaves g and g + 1) belongs to the node whose consecutive children it separates
    const int64_t n_gaps = std::max<int64_t>(n_leaves - 1, 1);
    std::vector<uint64_t> s_gap(n_gaps, 0);
    std::vector<int32_t> s_gap_node(n_gaps, 0);
    for (int32_t v = 1; v < n_nodes; ++v) {
        const int32_t u = parent[v];
        if (s_hi[v] < s_hi[u]) {  // v is not u's last child
            const int32_t g = s_hi[v];
            s_gap[g] = ((uint64_t)depth[u] << 32) | (uint32_t)g;
            s_gap_node[g] = u;
        }
    }
    const int32_t M = src->n_trees;
    const std::vector<int64_t> &off = src->h_tree_off;
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    hipStream_t s = ctx->stream;

    // ---- batches: rows (V per tree) + per-leaf arrays and tables (levels of the batch's largest tree) ----
    const int64_t row_stride = scs_round_up(std::max<int64_t>(n_leaves, 1), SC_ROW_ALIGN);
    const int levels = sc_levels_host(std::max<int64_t>(src->max_leaves, 1));
    const auto per_tree = [&](int32_t t) {
        const int64_t n = off[t + 1] - off[t];
        return (uint64_t)row_stride * 4 + (uint64_t)n * (4 * 3 + 8 * levels + 4 * (levels - 1));
    };
    std::vector<int32_t> bstart{0};
    {
        uint64_t acc = 0;
        for (int32_t t = 0; t < M; ++t) {
            const int32_t nb = t - bstart.back();
            if (nb > 0 && (acc + per_tree(t) > SC_BUDGET || (max_batch_trees > 0 && nb >= max_batch_trees))) {
                bstart.push_back(t);
                acc = 0;
            }
            acc += per_tree(t);
        }
        bstart.push_back(M);
    }
    int64_t max_rows = 0, max_lb = 0;
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        max_rows = std::max<int64_t>(max_rows, bstart[b + 1] - bstart[b]);
        max_lb = std::max<int64_t>(max_lb, off[bstart[b + 1]] - off[bstart[b]]);
    }
    auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
    const int s_levels = sc_levels_host(n_gaps);
    // persistent part: S arrays, marks, prefix sums, counters, flags
    size_t o = 0;
    const size_t o_spos = o; o += up256((size_t)std::max(n_taxa, 1) * 4);
    const size_t o_gnode = o; o += up256((size_t)n_gaps * 4);
    const size_t o_stab = o; o += up256((size_t)n_gaps * 8 * s_levels);
    const size_t o_slo = o; o += up256((size_t)n_nodes * 4);
    const size_t o_shi = o; o += up256((size_t)n_nodes * 4);
    const size_t o_end = o; o += up256((size_t)n_nodes * 4);
    const size_t o_mark = o; o += up256((size_t)n_nodes * 8);
    const size_t o_pref = o; o += up256(((size_t)n_nodes + 1) * 16);
    const size_t o_out = o; o += up256((size_t)n_nodes * 16);
    const size_t o_cnt = o; o += up256((size_t)M * 24);
    const size_t o_flag = o; o += 256;
    // batch part
    const size_t o_rows = o; o += up256((size_t)max_rows * row_stride * 4);
    const size_t o_sp = o; o += up256((size_t)max_lb * 4);
    const size_t o_dep = o; o += up256((size_t)max_lb * 4);
    const size_t o_node = o; o += up256((size_t)max_lb * 4);
    const size_t o_mm = o; o += up256((size_t)max_lb * 8 * levels);
    const size_t o_amin = o; o += up256((size_t)max_lb * 4 * std::max(levels - 1, 1));
    void *block = nullptr;
    SCS_TRY(scs_block_alloc(ctx, o, &block));
    char *bp = (char *)block;
    auto *d_spos = (int32_t *)(bp + o_spos);
    auto *d_gnode = (int32_t *)(bp + o_gnode);
    auto *d_stab = (uint64_t *)(bp + o_stab);
    auto *d_slo = (int32_t *)(bp + o_slo);
    auto *d_shi = (int32_t *)(bp + o_shi);
    auto *d_end = (int32_t *)(bp + o_end);
    auto *d_mark = (int32_t *)(bp + o_mark);
    auto *d_pref = (int64_t *)(bp + o_pref);
    auto *d_out = (int64_t *)(bp + o_out);
    auto *d_cnt = (unsigned long long *)(bp + o_cnt);
    auto *d_flag = (unsigned *)(bp + o_flag);
    auto *d_rows = (int32_t *)(bp + o_rows);
    auto *d_sp = (int32_t *)(bp + o_sp);
    auto *d_dep = (int32_t *)(bp + o_dep);
    auto *d_node = (int32_t *)(bp + o_node);
    auto *d_mm = (int2 *)(bp + o_mm);
    auto *d_amin = (int32_t *)(bp + o_amin);

    hipError_t e = hipSuccess;
    unsigned bad = 0;
    auto launch_ok = [&]() {
        if (e == hipSuccess) e = hipGetLastError();
        return e == hipSuccess;
    };
    e = hipMemcpyAsync(d_spos, s_pos.data(), (size_t)std::max(n_taxa, 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_gnode, s_gap_node.data(), (size_t)n_gaps * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_stab, s_gap.data(), (size_t)n_gaps * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slo, s_lo.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_shi, s_hi.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_end, sub_end.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_mark, 0, (size_t)n_nodes * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 24, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, 4, s);
    for (int j = 1; j < s_levels && e == hipSuccess; ++j) {
        k_score_level_u64<<<grid_of(n_gaps), SC_THREADS, 0, s>>>(d_stab + (j - 1) * n_gaps, d_stab + j * n_gaps, n_gaps,
                                                                 (int64_t)1 << (j - 1));
        launch_ok();
    }
    for (size_t b = 0; b + 1 < bstart.size() && e == hipSuccess; ++b) {
        const int32_t t0 = bstart[b], nb = bstart[b + 1] - t0;
        const int64_t *d_off = src->d_tree_off + t0;
        const int64_t L0 = off[t0], Lb = off[t0 + nb] - L0;
        e = hipMemsetAsync(d_rows, 0xff, (size_t)nb * row_stride * 4, s);
        if (e != hipSuccess) break;
        k_score_scatter<<<grid_of(Lb), SC_THREADS, 0, s>>>(d_off, nb, src->d_leaf_taxon, n_taxa, d_spos, d_rows,
                                                           row_stride, d_flag);
        if (!launch_ok()) break;
        // (a bad taxon leaves a row short: nothing below may read the arrays it did not fill -- stop here)
        e = hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess || bad) break;
        k_score_compact<<<nb, SC_THREADS, 0, s>>>(d_off, d_rows, row_stride, d_sp, d_mm);
        if (!launch_ok()) break;
        const int32_t *adj = src->d_adj_depth + L0;
        for (int j = 1; j < levels && e == hipSuccess; ++j) {
            k_score_level_tree<<<grid_of(Lb), SC_THREADS, 0, s>>>(j == 1 ? adj : d_amin + (int64_t)(j - 2) * Lb,
                                                                   d_amin + (int64_t)(j - 1) * Lb, d_mm + (j - 1) * Lb,
                                                                   d_mm + j * Lb, Lb, (int64_t)1 << (j - 1));
            launch_ok();
        }
        if (e != hipSuccess) break;
        k_score_restrict<<<grid_of(Lb), SC_THREADS, 0, s>>>(d_off, nb, d_sp, d_stab, n_gaps, d_gnode, d_dep, d_node);
        if (!launch_ok()) break;
        sc_nodes_args a;
        a.off = d_off;
        a.nb = nb;
        a.sp = d_sp;
        a.dep = d_dep;
        a.node = d_node;
        a.mm = d_mm;
        a.adj = adj;
        a.amin = d_amin;
        a.levels = levels;
        a.Lb = Lb;
        a.s_tab = d_stab;
        a.s_stride = n_gaps;
        a.s_lo = d_slo;
        a.s_hi = d_shi;
        a.mark_inf = d_mark;
        a.mark_sup = d_mark + n_nodes;
        a.c_super = d_cnt + t0;
        a.c_source = d_cnt + M + t0;
        a.c_shared = d_cnt + 2 * (int64_t)M + t0;
        k_score_nodes<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
        if (!launch_ok()) break;
    }
    if (e == hipSuccess && !bad) {
        k_score_prefix<<<1, 1024, 0, s>>>(d_mark, d_mark + n_nodes, n_nodes, d_pref, d_pref + n_nodes + 1);
        launch_ok();
    }
    if (e == hipSuccess && !bad) {
        k_score_subtree<<<grid_of(n_nodes), SC_THREADS, 0, s>>>(d_pref, d_pref + n_nodes + 1, d_end, n_nodes, d_out,
                                                                d_out + n_nodes);
        launch_ok();
    }
    std::vector<unsigned long long> cnt((size_t)M * 3);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)M * 24, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && informative)
        e = hipMemcpyAsync(informative, d_out, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && supported)
        e = hipMemcpyAsync(supported, d_out + n_nodes, (size_t)n_nodes * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipStreamSynchronize(s);  // (nothing may still write into the block)
    scs_block_release(ctx, block);
    if (e != hipSuccess) {
        scs_set_error("scs_score_supertree: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCS_ENOMEM : SCS_EHIP;
    }
    if (bad) {
        scs_set_error("scs_score_supertree: %s", (bad & 1u)   ? "a leaf_taxon entry is out of range [0, n_taxa)"
                                                 : (bad & 2u) ? "a source tree has a taxon the supertree lacks"
                                                              : "a source tree has a taxon twice");
        return SCS_EINVAL;
    }
    for (int32_t t = 0; t < M; ++t) {
        const int64_t n = off[t + 1] - off[t];
        const int64_t ns = (int64_t)cnt[t], nt = n >= 2 ? (int64_t)cnt[M + t] - 1 : 0, sh = (int64_t)cnt[2 * M + t];
        if (n_super) n_super[t] = ns;
        if (n_source) n_source[t] = nt;
        if (shared) shared[t] = sh;
    }
    return SCS_OK;
}
