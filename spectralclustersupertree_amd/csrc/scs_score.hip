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

// first index in [l, r) with sp[i] >= v, r if none (sp ascending)
__device__ __forceinline__ int64_t sc_first_ge(const int32_t *__restrict__ sp, int64_t l, int64_t r, int32_t v) {
    while (l < r) {
        const int64_t m = (l + r) >> 1;
        if (sp[m] >= v) r = m; else l = m + 1;
    }
    return l;
}

// last index in [l, r] with sp[i] <= v (sp ascending, sp[l] <= v)
__device__ __forceinline__ int64_t sc_last_le(const int32_t *__restrict__ sp, int64_t l, int64_t r, int32_t v) {
    while (l < r) {
        const int64_t m = (l + r + 1) >> 1;
        if (sp[m] <= v) l = m; else r = m - 1;
    }
    return l;
}

// binary descents on T's min table of adj (level 0 = adj, level j >= 1 at amin[(j - 1) * Lb]), gaps of the tree at
// batch-relative base: the start of the stretch [p, pos) of gaps whose depth is > d (>= d when `ge`) ...
__device__ __forceinline__ int64_t sc_stretch_left(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin,
                                                   int64_t Lb, int levels, int64_t base, int64_t pos, int32_t d,
                                                   bool ge) {
    for (int j = levels - 1; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos >= w) {
            const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
            const int32_t x = lev[base + pos - w];
            if (ge ? x >= d : x > d) pos -= w;
        }
    }
    return pos;
}

// ... and the end of the stretch [pos, p) of gaps whose depth is >= d, p <= last
__device__ __forceinline__ int64_t sc_stretch_right(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin,
                                                    int64_t Lb, int levels, int64_t base, int64_t pos, int64_t last,
                                                    int32_t d) {
    for (int j = levels - 1; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos + w <= last) {
            const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
            if (lev[base + pos] >= d) pos += w;
        }
    }
    return pos;
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

// one prepared batch as the kernels see it (sc_batch_of fills it on the host): every kernel argument struct below
// derives from it and adds its own members, so a kernel may be handed a few pointers it does not read
struct sc_batch {
    const int64_t *off;          // tree_off + t0 (global leaf offsets of the batch's trees)
    int nb;                      // trees in the batch
    const int32_t *sp;           // [Lb] S positions in S order
    const int32_t *dep, *node;   // [Lb] D and U of the restricted tree S'
    const int2 *mm;              // min-max table of tp (.x of level 0 is tp itself): level j at mm[j * Lb]
    const int32_t *adj;          // T's adj_depth of the batch (level 0 of the min table)
    const int32_t *amin;         // levels >= 1 of the min table of adj: level j at amin[(j - 1) * Lb]
    int levels;                  // levels of the batch's tables (2^levels > largest tree)
    int64_t Lb;                  // leaves of the batch
    const uint64_t *s_tab;       // S's packed gap table
    int64_t s_stride;            // entries per level of it (S's gaps)
    int s_levels;                // its levels (2^s_levels > S's gaps)
    const int32_t *s_lo, *s_hi;  // leaf range of every S node
};

struct sc_nodes_args : sc_batch {
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
        const int64_t pos = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
        t_first = pos == 0 || a.adj[base + pos - 1] < d;

        const int32_t u = a.node[q], du = a.dep[q];
        const int32_t sl = a.s_lo[u], sr = a.s_hi[u];
        const int32_t *sp = a.sp + base;
        // lo: first k' with sp[k'] >= sl (<= k), hi: last with sp[k'] <= sr (>= k + 1)
        const int64_t lo = sc_first_ge(sp, 0, k, sl);
        const int64_t hi = sc_last_le(sp, k + 1, n - 1, sr);
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

// ---- rooted triplets (scs_score_triplets) ----
//
// A tree on the leaf set L is given as its leaves in some order and the depths of the n - 1 adjacent LCAs (its
// gaps): T as adj_depth in T order, S' = S|L(T) as D in S order.  Gap k starts an internal node when it is the
// node's first gap; the node's leaves lie between the nearest strictly shallower gaps on either side, and its
// parent is the node of the deeper of those two gaps.  With y over T's non-root internal nodes, z over S''s,
// py / pz their parents and I(y, z) = |cl(y) ∩ cl(z)|:
//   t_source = sum_y C(|y|, 2) (|py| - |y|),  t_super likewise over S',
//   t_shared = sum_y sum_z C(I(y,z), 2) (I(py,pz) - I(y,pz) - I(py,z) + I(y,z))
// (a triple ab|c resolved alike in both is counted once: at the children y, z of the two LCAs that hold a and b).
//   k_trip_nodes: one thread per gap lists both trees' nodes as int4 {lo, hi + 1, parent lo, parent hi + 1} --
//     T ranges in T positions, S' ranges in S order -- and sums t_source / t_super.
//   k_trip_pairs: one workgroup per (tree, block of up to TP_ZMAX S' nodes z).  cl(z) and cl(pz) become bitsets
//     over T positions in LDS, each 32-bit word paired with the count of set bits before it, so a count over a
//     range of T positions is two ds_read_b64; the workgroup then sweeps T's node list once for all its z.

constexpr int TP_ZMAX = 8;                // S' nodes per workgroup
constexpr int TP_LDS_BUDGET = 40 << 10;   // LDS bytes a workgroup aims at (4 workgroups per CU) ...
constexpr int TP_LDS_MAX = 160 << 10;     // ... and may take for one S' node: trees of up to 327 679 leaves

struct sc_trip_args : sc_batch {
    int4 *ylist, *zlist;                   // [Lb]: the nodes of a tree from its first leaf on
    int32_t *ycnt, *zcnt;                   // [nb] list lengths
    unsigned long long *c_super, *c_source; // [nb] of the batch
};

// slot of a `hit` lane in tree t's list (wave-aggregated when the wave works on one tree), -1 for the others
__device__ __forceinline__ int sc_append(int32_t *__restrict__ cnt, int t, bool hit) {
    const int t0 = __shfl(t, 0, 64);
    if (__all(t == t0)) {
        const unsigned long long mask = __ballot(hit);
        int first = 0;
        if ((threadIdx.x & 63) == 0 && mask) first = atomicAdd(cnt + t0, (int)__popcll(mask));
        first = __shfl(first, 0, 64);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        return hit ? first + below : -1;
    }
    return hit ? atomicAdd(cnt + t, 1) : -1;
}

// per-tree 64-bit sums, wave-aggregated as in sc_count
__device__ __forceinline__ void sc_add64(unsigned long long *__restrict__ ctr, int t, unsigned long long v) {
    const int t0 = __shfl(t, 0, 64);
    if (__all(t == t0)) {
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctr + t0, v);
    } else if (v) {
        atomicAdd(ctr + t, v);
    }
}

__device__ __forceinline__ unsigned long long sc_pairs_out(int64_t lo, int64_t hi, int64_t plo, int64_t phi) {
    const int64_t s = hi - lo + 1;
    return (unsigned long long)(s * (s - 1) / 2 * (phi - plo + 1 - s));
}

// one thread per gap: T's and S''s non-root internal nodes into their lists, t_source / t_super
__global__ void __launch_bounds__(SC_THREADS) k_trip_nodes(sc_trip_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    int4 ny = make_int4(0, 0, 0, 0), nz = ny;
    bool t_node = false, s_node = false;
    unsigned long long vt = 0, vs = 0;
    if (in && k + 1 < n) {
        // T: the first gap of its node (the nearest gap to the left with depth <= d is missing or shallower)
        const int32_t d = a.adj[q];
        const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
        if (lo == 0 || a.adj[base + lo - 1] < d) {
            const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
            if (lo > 0 || hi < n - 1) {  // (not the root)
                const int64_t g = lo == 0 ? hi
                                  : hi == n - 1 ? lo - 1
                                  : (a.adj[base + lo - 1] >= a.adj[base + hi] ? lo - 1 : hi);
                const int32_t dg = a.adj[base + g];
                const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
                const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
                t_node = true;
                ny = make_int4((int)lo, (int)hi + 1, (int)plo, (int)phi + 1);
                vt = sc_pairs_out(lo, hi, plo, phi);
            }
        }
        // S': the node u = U[k] restricted, first gap and parent as in k_score_nodes
        const int32_t u = a.node[q], du = a.dep[q];
        const int32_t *sp = a.sp + base;
        const int64_t lo_s = sc_first_ge(sp, 0, k, a.s_lo[u]);
        const int64_t hi_s = sc_last_le(sp, k + 1, n - 1, a.s_hi[u]);
        const bool first = lo_s == k ||
                           (int32_t)(sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[lo_s], (int64_t)sp[k] - 1) >> 32) > du;
        if (first && (lo_s > 0 || hi_s < n - 1)) {
            const int64_t g = lo_s == 0 ? hi_s
                              : hi_s == n - 1 ? lo_s - 1
                              : (a.dep[base + lo_s - 1] >= a.dep[base + hi_s] ? lo_s - 1 : hi_s);
            const int32_t w = a.node[base + g];
            const int64_t plo = sc_first_ge(sp, 0, lo_s, a.s_lo[w]);
            const int64_t phi = sc_last_le(sp, hi_s, n - 1, a.s_hi[w]);
            s_node = true;
            nz = make_int4((int)lo_s, (int)hi_s + 1, (int)plo, (int)phi + 1);
            vs = sc_pairs_out(lo_s, hi_s, plo, phi);
        }
    }
    const int iy = sc_append(a.ycnt, t, t_node);
    if (iy >= 0) a.ylist[base + iy] = ny;
    const int iz = sc_append(a.zcnt, t, s_node);
    if (iz >= 0) a.zlist[base + iz] = nz;
    sc_add64(a.c_source, t, vt);
    sc_add64(a.c_super, t, vs);
}

// set bits of a bitset row below T position x: (word x / 32, mask of the bits below x % 32)
__device__ __forceinline__ int tp_count(const int2 *row, int w, unsigned m) {
    const int2 r = row[w];
    return r.y + __popc((unsigned)r.x & m);
}

// the hot path: one workgroup per (tree t, block of zb of t's S' nodes); blk[i] = first workgroup of the batch's
// tree i (cumulative over the trees, blk[0] = the batch's own start); W = words of a row (> largest n / 32)
__global__ void __launch_bounds__(SC_THREADS) k_trip_pairs(const int64_t *__restrict__ blk, int nb,
                                                           const int64_t *__restrict__ off,
                                                           const int4 *__restrict__ ylist,
                                                           const int4 *__restrict__ zlist,
                                                           const int32_t *__restrict__ ycnt,
                                                           const int32_t *__restrict__ zcnt,
                                                           const int2 *__restrict__ tp, int zb, int W,
                                                           unsigned long long *__restrict__ t_shared) {
    extern __shared__ __attribute__((aligned(16))) int2 rows[];  // [2 zb][W]: rows 2j / 2j + 1 = cl(z_j) / cl(pz_j)
    const int64_t g = blk[0] + blockIdx.x;
    const int t = sc_tree_of(blk, nb, g);
    const int j0 = (int)(g - blk[t]) * zb;
    const int nz = min(zb, zcnt[t] - j0);
    if (nz <= 0) return;  // (the grid counts n - 2 nodes per tree: an upper bound)
    const int64_t base = off[t] - off[0];
    const int nrow = 2 * nz;
    for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);  // (word i of the image: .x of entry i / 2)
    for (int j = 0; j < nz; ++j) {
        const int4 z = zlist[base + j0 + j];
        for (int k = z.x + threadIdx.x; k < z.y; k += SC_THREADS) {
            const int x = tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j) * W + (x >> 5)), 1u << (x & 31));
        }
        for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
            const int x = tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j + 1) * W + (x >> 5)), 1u << (x & 31));
        }
    }
    __syncthreads();
    // every word's .y = set bits in the words before it: one wave per row, wave64 scans of 64 words
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrow; r += SC_THREADS / 64) {
        int2 *row = rows + r * W;
        int run = 0;
        for (int c = 0; c < W; c += 64) {
            const int i = c + lane;
            const int v = i < W ? __popc((unsigned)row[i].x) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    unsigned long long acc = 0;
    const int ny = ycnt[t];
    for (int i = threadIdx.x; i < ny; i += SC_THREADS) {
        const int4 y = ylist[base + i];  // T positions [y.x, y.y) of y, [y.z, y.w) of py
        const int wa = y.x >> 5, wb = y.y >> 5, wc = y.z >> 5, wd = y.w >> 5;
        const unsigned ma = (1u << (y.x & 31)) - 1u, mb = (1u << (y.y & 31)) - 1u;
        const unsigned mc = (1u << (y.z & 31)) - 1u, md = (1u << (y.w & 31)) - 1u;
        for (int j = 0; j < nz; ++j) {
            const int2 *rz = rows + 2 * j * W, *rp = rz + W;
            const int iyz = tp_count(rz, wb, mb) - tp_count(rz, wa, ma);
            if (iyz < 2) continue;
            const int ipyz = tp_count(rz, wd, md) - tp_count(rz, wc, mc);
            const int iypz = tp_count(rp, wb, mb) - tp_count(rp, wa, ma);
            const int ipp = tp_count(rp, wd, md) - tp_count(rp, wc, mc);
            acc += (unsigned long long)((int64_t)iyz * (iyz - 1) / 2 * (int64_t)(ipp - iypz - ipyz + iyz));
        }
    }
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    __syncthreads();  // (the rows are read no more: their first 32 bytes take the wave sums)
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(rows);
    if (lane == 0) ws[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < SC_THREADS / 64; ++w) tot += ws[w];
        if (tot) atomicAdd(t_shared + t, tot);
    }
}

// ---- clade conflicts (scs_score_conflicts) ----
//
// Two sets conflict when they overlap and neither holds the other.  A cluster z of one tree (S' or T) conflicts with
// the other tree iff some gap p of the other tree's leaf order has exactly one of its leaves in z and lies strictly
// below lca(z) there.  Fix a gap p, x one of its two leaves, x' the other and K the leaves of lca(x, x'): the clusters
// it flags through x are the ancestors of x that miss x' and are not inside K -- a path from z*, the lowest ancestor
// of x with a leaf outside K (the deeper LCA of x with the nearest leaf outside K on either side of x, in z's own leaf
// order), up to A = lca(x, x'), A excluded.  +1 at a gap of z*, -1 at a gap of A: the marks on a node's gaps (its
// subtree) sum to the paths through it, and it conflicts iff the sum is positive.
//   k_conf_ip / k_conf_level: ip[T position] = S' index (the inverse of tp) and its min-max table.
//   k_conf_marks, one thread per gap, for both trees: T's gap marks S''s gaps (descents on tp's table, LCAs on S's
//     gap table), S''s gap marks T's gaps (descents on ip's table, LCAs on T's min table of adj).
//   k_conf_scan: one workgroup per tree, inclusive prefix sums of both mark rows.
//   k_conf_nodes, one thread per gap: every non-root node at its first gap reads its sum; a flagged S' node marks the
//     S path [u, w) of its cluster for `conflicting`, as k_score_nodes does for `supported`.

struct sc_conf_args : sc_batch {
    const int2 *im;              // min-max table of ip (T order): level j at im[j * Lb]
    int32_t *mark_s, *mark_t;    // [Lb] marks on S''s / T's gaps, then their per-tree inclusive prefix sums
    int32_t *mark_node;          // [S nodes]
    unsigned long long *c_super, *c_source;  // [nb] of the batch
};

// The searches of k_conf_marks gallop: blocks of 1, 2, 4, ... entries while the condition holds, then the binary
// descent from the last level that failed -- O(log of the distance found), as most answers lie a few leaves away.

// nearest index left of x / right of x (tree-relative, the tree at base, n leaves) whose entry in a min-max table lies
// outside [lo, hi]: -1 / n when there is none
__device__ __forceinline__ int64_t sc_outside_left(const int2 *__restrict__ tab, int64_t Lb, int levels, int64_t base,
                                                   int64_t x, int32_t lo, int32_t hi) {
    int64_t pos = x;
    int j = 0;
    for (; j < levels; ++j) {
        const int64_t w = (int64_t)1 << j;
        if (pos < w) break;
        const int2 v = tab[j * Lb + base + pos - w];
        if (v.x < lo || v.y > hi) break;
        pos -= w;
    }
    for (--j; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos >= w) {
            const int2 v = tab[j * Lb + base + pos - w];
            if (v.x >= lo && v.y <= hi) pos -= w;
        }
    }
    return pos - 1;
}

__device__ __forceinline__ int64_t sc_outside_right(const int2 *__restrict__ tab, int64_t Lb, int levels, int64_t base,
                                                    int64_t x, int64_t n, int32_t lo, int32_t hi) {
    int64_t pos = x + 1;
    int j = 0;
    for (; j < levels; ++j) {
        const int64_t w = (int64_t)1 << j;
        if (pos + w > n) break;
        const int2 v = tab[j * Lb + base + pos];
        if (v.x < lo || v.y > hi) break;
        pos += w;
    }
    for (--j; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos + w <= n) {
            const int2 v = tab[j * Lb + base + pos];
            if (v.x >= lo && v.y <= hi) pos += w;
        }
    }
    return pos;
}

// sc_stretch_left (ge) / sc_stretch_right, galloping: the start of the stretch [p, pos) of T gaps with depth >= d ...
__device__ __forceinline__ int64_t sc_gallop_left(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin,
                                                  int64_t Lb, int levels, int64_t base, int64_t pos, int32_t d) {
    int j = 0;
    for (; j < levels; ++j) {
        const int64_t w = (int64_t)1 << j;
        if (pos < w) break;
        const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
        if (lev[base + pos - w] < d) break;
        pos -= w;
    }
    for (--j; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos >= w) {
            const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
            if (lev[base + pos - w] >= d) pos -= w;
        }
    }
    return pos;
}

// ... and the end of the stretch [pos, p) of gaps with depth >= d, p <= last
__device__ __forceinline__ int64_t sc_gallop_right(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin,
                                                   int64_t Lb, int levels, int64_t base, int64_t pos, int64_t last,
                                                   int32_t d) {
    int j = 0;
    for (; j < levels; ++j) {
        const int64_t w = (int64_t)1 << j;
        if (pos + w > last) break;
        const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
        if (lev[base + pos] < d) break;
        pos += w;
    }
    for (--j; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos + w <= last) {
            const int32_t *lev = j == 0 ? adj : amin + (int64_t)(j - 1) * Lb;
            if (lev[base + pos] >= d) pos += w;
        }
    }
    return pos;
}

// sc_first_ge over [0, k] given sp[k] >= v, and sc_last_le over [k, last] given sp[k] <= v, galloping from k
__device__ __forceinline__ int64_t sc_gallop_first_ge(const int32_t *__restrict__ sp, int64_t k, int32_t v) {
    int64_t w = 1;
    while (k - w >= 0 && sp[k - w] >= v) {
        k -= w;
        w <<= 1;
    }
    return sc_first_ge(sp, std::max<int64_t>(k - w + 1, 0), k, v);
}

__device__ __forceinline__ int64_t sc_gallop_last_le(const int32_t *__restrict__ sp, int64_t k, int64_t last,
                                                     int32_t v) {
    int64_t w = 1;
    while (k + w <= last && sp[k + w] <= v) {
        k += w;
        w <<= 1;
    }
    return sc_last_le(sp, k, std::min<int64_t>(k + w - 1, last), v);
}

// min of adj over the batch-relative range [l, r] (r >= l)
__device__ __forceinline__ int32_t sc_conf_adj_min(const sc_conf_args &a, int64_t l, int64_t r) {
    const int j = sc_log2(r - l + 1);
    const int32_t *lev = j == 0 ? a.adj : a.amin + (int64_t)(j - 1) * a.Lb;
    return min(lev[l], lev[r - ((int64_t)1 << j) + 1]);
}

// level 0 of ip's min-max table: im[T position] = (k, k) for the tree's S' index k
__global__ void k_conf_ip(const int64_t *__restrict__ off, int nb, const int2 *__restrict__ mm0,
                          int2 *__restrict__ im0) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = off[0] + q;
    if (p >= off[nb]) return;
    const int64_t base = off[sc_tree_of(off, nb, p)] - off[0];
    const int32_t k = (int32_t)(q - base);
    im0[base + mm0[q].x] = make_int2(k, k);
}

__global__ void k_conf_level(const int2 *__restrict__ prev, int2 *__restrict__ cur, int64_t n, int64_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int2 m = prev[i];
    if (i + half < n) {
        const int2 m2 = prev[i + half];
        cur[i] = make_int2(min(m.x, m2.x), max(m.y, m2.y));
    } else {
        cur[i] = m;
    }
}

// one thread per gap k of a tree: as T's gap it marks the paths of S' nodes it flags, as S''s gap those of T's nodes
__global__ void __launch_bounds__(SC_THREADS) k_conf_marks(sc_conf_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    if (p >= a.off[a.nb]) return;
    const int t = sc_tree_of(a.off, a.nb, p);
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    if (k + 1 >= n) return;
    const int32_t *sp = a.sp + base;
    {
        // T's gap k: K = the T positions [klo, khi] of lca_T(k, k + 1); x, x' = their S' indices
        const int32_t d = a.adj[q];
        const int32_t klo = (int32_t)sc_gallop_left(a.adj, a.amin, a.Lb, a.levels, base, k, d);
        const int32_t khi = (int32_t)sc_gallop_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
        if (klo > 0 || khi < n - 1) {  // (K = L leaves nothing outside)
            const int32_t i0 = a.im[q].x, i1 = a.im[q + 1].x;
            const int64_t lo = min(i0, i1), hi = max(i0, i1);
            const uint64_t pa = sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[lo], (int64_t)sp[hi] - 1);
            const int32_t da = (int32_t)(pa >> 32);
            int64_t ga = -1;
            for (int s = 0; s < 2; ++s) {
                const int64_t x = s ? hi : lo;
                const int64_t l = sc_outside_left(a.mm, a.Lb, a.levels, base, x, klo, khi);
                const int64_t r = sc_outside_right(a.mm, a.Lb, a.levels, base, x, n, klo, khi);
                const uint64_t pl = l >= 0 ? sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[l], (int64_t)sp[x] - 1) : 0;
                const uint64_t pr = r < n ? sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[x], (int64_t)sp[r] - 1) : 0;
                const int32_t dl = l >= 0 ? (int32_t)(pl >> 32) : -1, dr = r < n ? (int32_t)(pr >> 32) : -1;
                if (max(dl, dr) <= da) continue;  // (z* is A or above it: no path)
                const int64_t gz = dl >= dr ? sc_last_le(sp, l, x - 1, (int32_t)(uint32_t)pl)
                                            : sc_last_le(sp, x, r - 1, (int32_t)(uint32_t)pr);
                if (ga < 0) ga = sc_last_le(sp, lo, hi - 1, (int32_t)(uint32_t)pa);
                atomicAdd(a.mark_s + base + gz, 1);
                atomicAdd(a.mark_s + base + ga, -1);
            }
        }
    }
    {
        // S''s gap k: K' = the S' indices [klo, khi] of its node U[k]; x, x' = the T positions of S' leaves k, k + 1
        const int32_t u = a.node[q];
        const int32_t klo = (int32_t)sc_gallop_first_ge(sp, k, a.s_lo[u]);
        const int32_t khi = (int32_t)sc_gallop_last_le(sp, k + 1, n - 1, a.s_hi[u]);
        if (klo > 0 || khi < n - 1) {
            const int32_t i0 = a.mm[q].x, i1 = a.mm[q + 1].x;
            const int64_t lo = min(i0, i1), hi = max(i0, i1);
            const int32_t da = sc_conf_adj_min(a, base + lo, base + hi - 1);
            int64_t ga = -1;
            for (int s = 0; s < 2; ++s) {
                const int64_t x = s ? hi : lo;
                const int64_t l = sc_outside_left(a.im, a.Lb, a.levels, base, x, klo, khi);
                const int64_t r = sc_outside_right(a.im, a.Lb, a.levels, base, x, n, klo, khi);
                const int32_t dl = l >= 0 ? sc_conf_adj_min(a, base + l, base + x - 1) : -1;
                const int32_t dr = r < n ? sc_conf_adj_min(a, base + x, base + r - 1) : -1;
                if (max(dl, dr) <= da) continue;
                // a gap of the LCA: the first gap of the range no deeper than its minimum
                const int64_t gz = dl >= dr ? sc_gallop_right(a.adj, a.amin, a.Lb, a.levels, base, l, x - 1, dl + 1)
                                            : sc_gallop_right(a.adj, a.amin, a.Lb, a.levels, base, x, r - 1, dr + 1);
                if (ga < 0) ga = sc_gallop_right(a.adj, a.amin, a.Lb, a.levels, base, lo, hi - 1, da + 1);
                atomicAdd(a.mark_t + base + gz, 1);
                atomicAdd(a.mark_t + base + ga, -1);
            }
        }
    }
}

// inclusive prefix sums of both mark rows over every tree's own entries, one workgroup per tree
__global__ void __launch_bounds__(SC_THREADS) k_conf_scan(const int64_t *__restrict__ off, int32_t *__restrict__ m0,
                                                          int32_t *__restrict__ m1) {
    __shared__ int ws[2][SC_THREADS / 64];
    const int t = blockIdx.x;
    const int64_t base = off[t] - off[0], n = off[t + 1] - off[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int run0 = 0, run1 = 0;
    for (int64_t c = 0; c < n; c += SC_THREADS) {
        const int64_t i = c + threadIdx.x;
        int x0 = i < n ? m0[base + i] : 0, x1 = i < n ? m1[base + i] : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int y0 = __shfl_up(x0, d, 64), y1 = __shfl_up(x1, d, 64);
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
        int b0 = run0, b1 = run1;
        for (int w = 0; w < SC_THREADS / 64; ++w) {
            if (w < wave) {
                b0 += ws[0][w];
                b1 += ws[1][w];
            }
            run0 += ws[0][w];
            run1 += ws[1][w];
        }
        if (i < n) {
            m0[base + i] = b0 + x0;
            m1[base + i] = b1 + x1;
        }
        __syncthreads();
    }
}

// marks on the gaps [lo, hi) of the tree at base, from the inclusive prefix sums
__device__ __forceinline__ int32_t sc_conf_sum(const int32_t *__restrict__ pre, int64_t base, int64_t lo, int64_t hi) {
    return pre[base + hi - 1] - (lo > 0 ? pre[base + lo - 1] : 0);
}

// one thread per gap: the non-root nodes of both trees at their first gaps read their sums
__global__ void __launch_bounds__(SC_THREADS) k_conf_nodes(sc_conf_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    bool t_hit = false, s_hit = false;
    if (in && k + 1 < n) {
        // T: the first gap of its node, the node's leaves [lo, hi]
        const int32_t d = a.adj[q];
        const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
        if (lo == 0 || a.adj[base + lo - 1] < d) {
            const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
            if (lo > 0 || hi < n - 1) t_hit = sc_conf_sum(a.mark_t, base, lo, hi) > 0;
        }
        // S': the restricted node u = U[k], first gap and parent as in k_score_nodes
        const int32_t u = a.node[q], du = a.dep[q];
        const int32_t *sp = a.sp + base;
        const int64_t lo_s = sc_first_ge(sp, 0, k, a.s_lo[u]);
        const int64_t hi_s = sc_last_le(sp, k + 1, n - 1, a.s_hi[u]);
        const bool first = lo_s == k ||
                           (int32_t)(sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[lo_s], (int64_t)sp[k] - 1) >> 32) > du;
        if (first && (lo_s > 0 || hi_s < n - 1) && sc_conf_sum(a.mark_s, base, lo_s, hi_s) > 0) {
            s_hit = true;
            const int64_t g = lo_s == 0 ? hi_s
                              : hi_s == n - 1 ? lo_s - 1
                              : (a.dep[base + lo_s - 1] >= a.dep[base + hi_s] ? lo_s - 1 : hi_s);
            atomicAdd(a.mark_node + u, 1);
            atomicAdd(a.mark_node + a.node[base + g], -1);
        }
    }
    sc_count(a.c_source, t, t_hit);
    sc_count(a.c_super, t, s_hit);
}

// ---- branch concordance (scs_score_concordance) ----
//
// A node C of S is a quartet branch when it is not the root, has exactly two children A (first in preorder) and B, and
// its parent has exactly two children, C and its sibling D.  A source tree T on L is decisive for C when A ∩ L, B ∩ L
// and D ∩ L are all non-empty; it is then concordant when (A ∪ B) ∩ L is a cluster of T, alt1 when (A ∪ D) ∩ L is,
// alt2 when (B ∪ D) ∩ L is (the three conflict pairwise: at most one holds), and `other` when none is.
// With A ∩ L and B ∩ L non-empty, C is the S node of LCA_S(C ∩ L): U[k] at the gap k between the last leaf of A ∩ L and
// the first of B ∩ L in S order, and as C has two children no other gap of the tree has U = C.  So one thread per gap
// finds every decisive (C, T) once: [lo, hi] = C ∩ L by two searches in sp, A ∩ L = [lo, k], B ∩ L = [k + 1, hi], and
// D ∩ L is the stretch of sp inside the parent's leaf range on the other side of [lo, hi].  A union of two of the
// three ranges is a cluster of T iff the T positions of its leaves (min / max over each range from tp's table) span
// exactly its size and the LCA of that span has no further leaf (step 4 of section 14).  Every result belongs to C
// alone: the counts go straight onto per-node counters, no path marks and no prefix pass.

// (not over sc_batch: with the view's unread members between its own, k_conc_branches fetches its arguments in four
// pieces where it fetched them in one, and scs_score_concordance, which is this one launch a batch, came out 0.06 ms
// behind in two of four comparisons; alone, the struct leaves the kernel as it was, instruction for instruction)
struct sc_conc_args {
    const int64_t *off;          // tree_off + t0
    int nb;
    const int32_t *sp, *node;    // [Lb] S positions in S order, U of S'
    const int2 *mm;              // min-max table of tp: level j at mm[j * Lb]
    const int32_t *adj, *amin;   // T's min table of adj_depth (as in sc_batch)
    int64_t Lb;
    const int32_t *s_lo, *s_hi;  // leaf range of every S node
    const int32_t *q_parent;     // [S nodes] the parent of a quartet branch, -1 for every other node
    unsigned long long *n_dec, *n_con, *n_alt1, *n_alt2;  // [S nodes]
    unsigned long long *c_dec, *c_con, *c_alt;            // [nb] of the batch
};

// are the `size` (>= 2) leaves of the tree at base (n leaves) whose T positions span [ab.x, ab.y] a cluster of T
__device__ __forceinline__ bool sc_conc_cluster(const sc_conc_args &a, int64_t base, int64_t n, int2 ab,
                                                int64_t size) {
    if (ab.y - ab.x + 1 != size) return false;
    const int64_t l = base + ab.x, r = base + ab.y - 1;
    const int j = sc_log2(r - l + 1);
    const int32_t *lev = j == 0 ? a.adj : a.amin + (int64_t)(j - 1) * a.Lb;
    const int32_t dT = min(lev[l], lev[r - ((int64_t)1 << j) + 1]);
    return (ab.x == 0 || a.adj[l - 1] < dT) && (ab.y == n - 1 || a.adj[r + 1] < dT);
}

__device__ __forceinline__ int2 sc_join(int2 x, int2 y) { return make_int2(min(x.x, y.x), max(x.y, y.y)); }

// one thread per gap: the quartet branch u = U[k] the tree is decisive for, classified
__global__ void __launch_bounds__(SC_THREADS) k_conc_branches(sc_conc_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    bool dec = false, con = false, alt = false;
    if (in && k + 1 < n) {
        const int32_t u = a.node[q];
        const int32_t pu = a.q_parent[u];
        if (pu >= 0) {
            const int32_t *sp = a.sp + base;
            const int32_t sl = a.s_lo[u], pl = a.s_lo[pu];
            const int64_t lo = sc_gallop_first_ge(sp, k, sl);
            const int64_t hi = sc_gallop_last_le(sp, k + 1, n - 1, a.s_hi[u]);
            // D ∩ L = [dlo, dhi]: after [lo, hi] when u is the parent's first child, before it otherwise
            int64_t dlo = 0, dhi = -1;
            if (pl == sl) {
                const int32_t pr = a.s_hi[pu];
                if (hi + 1 < n && sp[hi + 1] <= pr) {
                    dlo = hi + 1;
                    dhi = sc_gallop_last_le(sp, hi + 1, n - 1, pr);
                }
            } else if (lo > 0 && sp[lo - 1] >= pl) {
                dhi = lo - 1;
                dlo = sc_gallop_first_ge(sp, lo - 1, pl);
            }
            if (dhi >= dlo) {
                dec = true;
                const int2 ma = sc_rmq_minmax(a.mm, a.Lb, base + lo, base + k);
                const int2 mb = sc_rmq_minmax(a.mm, a.Lb, base + k + 1, base + hi);
                const int2 md = sc_rmq_minmax(a.mm, a.Lb, base + dlo, base + dhi);
                const int64_t za = k - lo + 1, zb = hi - k, zd = dhi - dlo + 1;
                con = sc_conc_cluster(a, base, n, sc_join(ma, mb), za + zb);
                bool alt1 = false, alt2 = false;
                if (!con) alt1 = sc_conc_cluster(a, base, n, sc_join(ma, md), za + zd);
                if (!con && !alt1) alt2 = sc_conc_cluster(a, base, n, sc_join(mb, md), zb + zd);
                alt = alt1 || alt2;
                atomicAdd(a.n_dec + u, 1ull);
                if (con) atomicAdd(a.n_con + u, 1ull);
                if (alt1) atomicAdd(a.n_alt1 + u, 1ull);
                if (alt2) atomicAdd(a.n_alt2 + u, 1ull);
            }
        }
    }
    sc_count(a.c_dec, t, dec);
    sc_count(a.c_con, t, con);
    sc_count(a.c_alt, t, alt);
}

// ---- per-branch triplet support (scs_score_branch_triplets) ----
//
// The graded form of the branch concordance: for a quartet branch C of S (children A and B, sibling D) and a source T
// on L that is decisive for it (A' = A ∩ L, B' = B ∩ L, D' = D ∩ L all non-empty), the |A'||B'||D'| triples (a, b, d)
// with a in A', b in B', d in D' are resolved ab|d (concordant), ad|b (alt1), bd|a (alt2) or left a fan by T.  With y
// over T's non-root nodes, py the parent and I(y, X) = |cl(y) ∩ X|, a triple resolved ab|d has exactly one y with
// a, b in y and d in py \ y:
//   bt_concordant = sum_y I(y,A') I(y,B') (I(py,D') - I(y,D')),  alt1 with (A', D', B'),  alt2 with (B', D', A').
//   k_bt_records: one thread per gap lists T's nodes (as k_trip_nodes does) and, by steps 1 - 3 of k_conc_branches,
//     the decisive branch of the gap as a record {u, lo, k, hi, dlo, dhi} (S' indices); bt_total on the way.
//   k_bt_pairs: one workgroup per (tree, block of zb records).  A', A' ∪ B' and A' ∪ B' ∪ D' become bitset rows over T
//     positions in LDS in the {bits, prefix} layout of k_trip_pairs (the B' and D' counts are differences of two
//     rows); the workgroup sweeps T's node list once for all its records.

constexpr int BT_ZMAX = 8;       // records per workgroup
constexpr int BT_ROW_BYTES = 24; // LDS bytes per 32 T positions of one record: three rows of int2

struct sc_bt_rec {
    int32_t u;             // the quartet branch (S node)
    int32_t lo, k, hi;     // A' = S' indices [lo, k], B' = [k + 1, hi]
    int32_t dlo, dhi;      // D' = [dlo, dhi]
};

struct sc_bt_args : sc_batch {
    const int32_t *q_parent;    // [S nodes] the parent of a quartet branch, -1 for every other node
    int4 *ylist;                 // [Lb] T's nodes of a tree from its first leaf on
    sc_bt_rec *recs;             // [Lb] the tree's records likewise
    int32_t *ycnt, *rcnt;        // [nb] list lengths
    unsigned long long *n_tot;   // [S nodes] bt_total
    unsigned long long *c_tot;   // [nb] n_bt_total of the batch
    int64_t nn;                  // S nodes (the resample sweep: n_tot is the batch's slab [nb][4][nn], no c_tot)
};

// one thread per gap: T's non-root internal node that starts here, and the quartet branch the tree is decisive for.
// SLAB (scs_score_branch_resample, section 26): the tree's own total is stored, not added over the trees -- a tree has
// one record per branch (a quartet branch has two children: one gap of S' lies between them), so the entry has one owner
template <bool SLAB>
__device__ __forceinline__ void bt_records(const sc_bt_args &a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    int4 ny = make_int4(0, 0, 0, 0);
    sc_bt_rec r = {0, 0, 0, 0, 0, 0};
    bool t_node = false, dec = false;
    unsigned long long vt = 0;
    if (in && k + 1 < n) {
        // T: the first gap of its node, the node's and its parent's leaves (as k_trip_nodes)
        const int32_t d = a.adj[q];
        const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
        if (lo == 0 || a.adj[base + lo - 1] < d) {
            const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
            if (lo > 0 || hi < n - 1) {  // (not the root)
                const int64_t g = lo == 0 ? hi
                                  : hi == n - 1 ? lo - 1
                                  : (a.adj[base + lo - 1] >= a.adj[base + hi] ? lo - 1 : hi);
                const int32_t dg = a.adj[base + g];
                const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
                const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
                t_node = true;
                ny = make_int4((int)lo, (int)hi + 1, (int)plo, (int)phi + 1);
            }
        }
        // S: u = U[k] a quartet branch, [lo, hi] and the D' stretch (steps 1 - 3 of k_conc_branches)
        const int32_t u = a.node[q];
        const int32_t pu = a.q_parent[u];
        if (pu >= 0) {
            const int32_t *sp = a.sp + base;
            const int32_t sl = a.s_lo[u], pl = a.s_lo[pu];
            const int64_t lo_s = sc_gallop_first_ge(sp, k, sl);
            const int64_t hi_s = sc_gallop_last_le(sp, k + 1, n - 1, a.s_hi[u]);
            int64_t dlo = 0, dhi = -1;
            if (pl == sl) {
                const int32_t pr = a.s_hi[pu];
                if (hi_s + 1 < n && sp[hi_s + 1] <= pr) {
                    dlo = hi_s + 1;
                    dhi = sc_gallop_last_le(sp, hi_s + 1, n - 1, pr);
                }
            } else if (lo_s > 0 && sp[lo_s - 1] >= pl) {
                dhi = lo_s - 1;
                dlo = sc_gallop_first_ge(sp, lo_s - 1, pl);
            }
            if (dhi >= dlo) {
                dec = true;
                r = {u, (int32_t)lo_s, (int32_t)k, (int32_t)hi_s, (int32_t)dlo, (int32_t)dhi};
                vt = (unsigned long long)((k - lo_s + 1) * (hi_s - k) * (dhi - dlo + 1));
                if (SLAB)
                    a.n_tot[(int64_t)t * 4 * a.nn + u] = vt;
                else
                    atomicAdd(a.n_tot + u, vt);
            }
        }
    }
    const int iy = sc_append(a.ycnt, t, t_node);
    if (iy >= 0) a.ylist[base + iy] = ny;
    const int ir = sc_append(a.rcnt, t, dec);
    if (ir >= 0) a.recs[base + ir] = r;
    if (!SLAB) sc_add64(a.c_tot, t, vt);
}

__global__ void __launch_bounds__(SC_THREADS) k_bt_records(sc_bt_args a) { bt_records<false>(a); }

__global__ void __launch_bounds__(SC_THREADS) k_rs_records(sc_bt_args a) { bt_records<true>(a); }

// the hot path: one workgroup per (tree t, block of zb of t's records); blk and W as in k_trip_pairs.  node_ctr holds
// bt_concordant, bt_alt1, bt_alt2 as three arrays of nn entries; c_con / c_alt are the batch's per-tree counters.
// SLAB: node_ctr is the batch's slab [nb][4][nn] and lane 3 j + c stores counter c of record j into rows 1 - 3 of its
// tree (one owner per entry, as in bt_records<true>); no per-tree counters
template <bool SLAB>
__device__ __forceinline__ void bt_pairs(const int64_t *__restrict__ blk, int nb, const int64_t *__restrict__ off,
                                         const int4 *__restrict__ ylist, const sc_bt_rec *__restrict__ recs,
                                         const int32_t *__restrict__ ycnt, const int32_t *__restrict__ rcnt,
                                         const int2 *__restrict__ tp, int zb, int W,
                                         unsigned long long *__restrict__ node_ctr, int64_t nn,
                                         unsigned long long *__restrict__ c_con,
                                         unsigned long long *__restrict__ c_alt) {
    // [3 zb][W]: rows 3j, 3j + 1, 3j + 2 = A', A' ∪ B', A' ∪ B' ∪ D' of record j
    extern __shared__ __attribute__((aligned(16))) int2 rows[];
    const int64_t g = blk[0] + blockIdx.x;
    const int t = sc_tree_of(blk, nb, g);
    const int j0 = (int)(g - blk[t]) * zb;
    const int nz = min(zb, rcnt[t] - j0);
    if (nz <= 0) return;  // (the grid counts n - 2 records per tree: an upper bound)
    const int64_t base = off[t] - off[0];
    const int nrow = 3 * nz;
    for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);  // (word i of the image: .x of entry i / 2)
    for (int j = 0; j < nz; ++j) {
        const sc_bt_rec r = recs[base + j0 + j];
        for (int k = r.lo + threadIdx.x; k <= r.hi; k += SC_THREADS) {
            const int x = tp[base + k].x;
            const unsigned bit = 1u << (x & 31);
            if (k <= r.k) atomicOr(bits + 2 * ((3 * j) * W + (x >> 5)), bit);
            atomicOr(bits + 2 * ((3 * j + 1) * W + (x >> 5)), bit);
            atomicOr(bits + 2 * ((3 * j + 2) * W + (x >> 5)), bit);
        }
        for (int k = r.dlo + threadIdx.x; k <= r.dhi; k += SC_THREADS) {
            const int x = tp[base + k].x;
            atomicOr(bits + 2 * ((3 * j + 2) * W + (x >> 5)), 1u << (x & 31));
        }
    }
    __syncthreads();
    // every word's .y = set bits in the words before it: one wave per row, wave64 scans of 64 words
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrow; r += SC_THREADS / 64) {
        int2 *row = rows + r * W;
        int run = 0;
        for (int c = 0; c < W; c += 64) {
            const int i = c + lane;
            const int v = i < W ? __popc((unsigned)row[i].x) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    unsigned long long acc[BT_ZMAX][3];
#pragma unroll
    for (int j = 0; j < BT_ZMAX; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0;
    const int ny = ycnt[t];
    for (int i = threadIdx.x; i < ny; i += SC_THREADS) {
        const int4 y = ylist[base + i];  // T positions [y.x, y.y) of y, [y.z, y.w) of py
        const int wa = y.x >> 5, wb = y.y >> 5, wc = y.z >> 5, wd = y.w >> 5;
        const unsigned ma = (1u << (y.x & 31)) - 1u, mb = (1u << (y.y & 31)) - 1u;
        const unsigned mc = (1u << (y.z & 31)) - 1u, md = (1u << (y.w & 31)) - 1u;
#pragma unroll
        for (int j = 0; j < BT_ZMAX; ++j) {
            if (j >= nz) break;
            const int2 *ra = rows + 3 * j * W, *rab = ra + W, *rabd = rab + W;
            const int yab = tp_count(rab, wb, mb) - tp_count(rab, wa, ma);
            if (yab == 0) continue;  // (every term has a factor I(y, A') or I(y, B'))
            const int ya = tp_count(ra, wb, mb) - tp_count(ra, wa, ma);
            const int yabd = tp_count(rabd, wb, mb) - tp_count(rabd, wa, ma);
            const int pa = tp_count(ra, wd, md) - tp_count(ra, wc, mc);
            const int pab = tp_count(rab, wd, md) - tp_count(rab, wc, mc);
            const int pabd = tp_count(rabd, wd, md) - tp_count(rabd, wc, mc);
            const int64_t ia = ya, ib = yab - ya, id = yabd - yab;         // I(y, A'), I(y, B'), I(y, D')
            const int64_t oa = pa - ya, ob = (pab - pa) - ib, od = (pabd - pab) - id;  // the same of py \ y
            acc[j][0] += (unsigned long long)(ia * ib * od);
            acc[j][1] += (unsigned long long)(ia * id * ob);
            acc[j][2] += (unsigned long long)(ib * id * oa);
        }
    }
    __syncthreads();  // (the rows are read no more: their first 768 bytes take the wave sums)
    unsigned long long *ws = reinterpret_cast<unsigned long long *>(rows);  // [waves][BT_ZMAX][3]
#pragma unroll
    for (int j = 0; j < BT_ZMAX; ++j) {
        if (j >= nz) break;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned long long v = acc[j][c];
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
            if (lane == 0) ws[(wave * BT_ZMAX + j) * 3 + c] = v;
        }
    }
    __syncthreads();
    if (wave == 0) {
        // lane 3 j + c: counter c of record j over the waves, one atomic where it is not zero; then the tree's two sums
        unsigned long long tot = 0;
        if (lane < 3 * nz)
            for (int w = 0; w < SC_THREADS / 64; ++w) tot += ws[w * BT_ZMAX * 3 + lane];
        const int c = lane % 3;
        if (SLAB) {
            if (tot) node_ctr[((int64_t)t * 4 + 1 + c) * nn + recs[base + j0 + lane / 3].u] = tot;
            return;
        }
        if (tot) atomicAdd(node_ctr + c * nn + recs[base + j0 + lane / 3].u, tot);
        unsigned long long con = c == 0 ? tot : 0, alt = c == 0 ? 0 : tot;
        for (int d = 32; d >= 1; d >>= 1) {
            con += __shfl_xor(con, d, 64);
            alt += __shfl_xor(alt, d, 64);
        }
        if (lane == 0 && con) atomicAdd(c_con + t, con);
        if (lane == 0 && alt) atomicAdd(c_alt + t, alt);
    }
}

__global__ void __launch_bounds__(SC_THREADS) k_bt_pairs(const int64_t *__restrict__ blk, int nb,
                                                         const int64_t *__restrict__ off,
                                                         const int4 *__restrict__ ylist,
                                                         const sc_bt_rec *__restrict__ recs,
                                                         const int32_t *__restrict__ ycnt,
                                                         const int32_t *__restrict__ rcnt,
                                                         const int2 *__restrict__ tp, int zb, int W,
                                                         unsigned long long *__restrict__ node_ctr, int64_t nn,
                                                         unsigned long long *__restrict__ c_con,
                                                         unsigned long long *__restrict__ c_alt) {
    bt_pairs<false>(blk, nb, off, ylist, recs, ycnt, rcnt, tp, zb, W, node_ctr, nn, c_con, c_alt);
}

__global__ void __launch_bounds__(SC_THREADS) k_rs_pairs(const int64_t *__restrict__ blk, int nb,
                                                         const int64_t *__restrict__ off,
                                                         const int4 *__restrict__ ylist,
                                                         const sc_bt_rec *__restrict__ recs,
                                                         const int32_t *__restrict__ ycnt,
                                                         const int32_t *__restrict__ rcnt,
                                                         const int2 *__restrict__ tp, int zb, int W,
                                                         unsigned long long *__restrict__ node_ctr, int64_t nn,
                                                         unsigned long long *__restrict__ c_con,
                                                         unsigned long long *__restrict__ c_alt) {
    bt_pairs<true>(blk, nb, off, ylist, recs, ycnt, rcnt, tp, zb, W, node_ctr, nn, c_con, c_alt);
}

// ---- per-taxon triplet support (scs_score_taxon_triplets) ----
//
// The per-tree sums of section 15 handed to the leaves of every triple.  A shared triple ab|c is counted at one pair
// (y, z): with I = I(y, z) and J = I(py,pz) - I(y,pz) - I(py,z) + I(y,z), every leaf of cl(y) ∩ cl(z) is a or b in
// (I - 1) J of the pair's triples and every leaf of (cl(py) ∖ cl(y)) ∩ (cl(pz) ∖ cl(z)) is c in C(I, 2) of them.  T's
// clusters are ranges of T positions, so for a fixed z both are interval-stabbing sums: difference arrays over the
// *rank* of a T position among the set bits of cl(z) / cl(pz) -- the tp_count values the sweep reads anyway -- then a
// prefix sum, and every leaf of z (of pz ∖ z) reads the entry of its own rank.
//   k_trip_nodes (unchanged) lists the nodes; k_tx_single, one thread per listed node: the single-tree terms
//     (tx_source over T positions, tx_super over S' positions) as difference rows, and every z into the list of the
//     bin that holds its two difference arrays (|z| + 1 and |pz| + 1 entries);
//   k_tx_pairs<false>: the k_trip_pairs grid once per LDS bin, bitset rows and difference arrays in LDS;
//   k_tx_pairs<true>: the nodes whose arrays fit no bin, one at a time by a bounded grid of persistent workgroups, the
//     arrays in a slab of the workspace per workgroup (global 64-bit atomics, loads and stores past the L1);
//   k_tx_scan: per-tree prefix sums of the two single-tree rows; k_tx_fold: the batch's per-leaf sums into the
//     per-taxon outputs (64-bit atomics: integers, so order-free).
// Every intermediate is a count of triples of one tree: below m^3 < 2^63 for the m <= 327 679 the rows allow.

constexpr int TX_BINS = 3;           // LDS bins; list TX_BINS is the slab's
constexpr int TX_SCRATCH = 64;       // bytes ahead of the rows: the wave sums of the workgroup scan
constexpr int TX_SLAB_PAD = 8;       // entries behind a slab's arrays: the same wave sums
constexpr int TX_SLAB_WGS = 256;     // persistent workgroups of the slab path, at most
constexpr uint64_t TX_SLAB_BYTES = (uint64_t)128 << 20;  // all slabs together (fewer workgroups for larger trees)
// LDS a workgroup of each bin aims at: 8, 3 and 1 workgroups per CU (the last is all a workgroup can take)
constexpr int TX_BIN_BUDGET[TX_BINS] = {20 << 10, 52 << 10, TP_LDS_MAX};
// ... and the S' nodes a workgroup takes at most: the last bin gives all of its LDS to one node's arrays
constexpr int TX_BIN_ZMAX[TX_BINS] = {TP_ZMAX, 2, 1};
constexpr int TX_SMALL = 192;        // entries a node of bin 0 keeps when the rows grow

struct sc_tx_bins {
    int dcap[TX_BINS];  // entries (both arrays) a node of the bin may take; 0: the bin is not used
};

__device__ __forceinline__ void tx_mark(unsigned long long *__restrict__ row, int n, int i, unsigned long long v) {
    if (i < n && v) atomicAdd(row + i, v);  // (entry n is read by no leaf)
}

// a node {lo, hi, parent lo, parent hi} of one tree alone: its leaves take (s - 1)(ps - s) each, the parent's other
// leaves C(s, 2) each
__device__ __forceinline__ void tx_single(unsigned long long *__restrict__ row, int n, const int4 v) {
    const int64_t s = v.y - v.x, ps = v.w - v.z;
    const unsigned long long a = (unsigned long long)((s - 1) * (ps - s)), b = (unsigned long long)(s * (s - 1) / 2);
    tx_mark(row, n, v.x, a - b);
    tx_mark(row, n, v.y, b - a);
    tx_mark(row, n, v.z, b);
    tx_mark(row, n, v.w, 0ull - b);
}

// one thread per leaf slot i of a tree: node i of T's list and node i of S''s list
__global__ void __launch_bounds__(SC_THREADS) k_tx_single(const int64_t *__restrict__ off, int nb,
                                                          const int4 *__restrict__ ylist,
                                                          const int4 *__restrict__ zlist,
                                                          const int32_t *__restrict__ ycnt,
                                                          const int32_t *__restrict__ zcnt, sc_tx_bins bins, int64_t Lb,
                                                          int32_t *__restrict__ zbin, int32_t *__restrict__ zbcnt,
                                                          unsigned long long *__restrict__ d_src,
                                                          unsigned long long *__restrict__ d_sup, int has_slab,
                                                          unsigned *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = off[0] + q;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    const int64_t base = off[t] - off[0];
    const int n = (int)(off[t + 1] - off[t]);
    const int i = (int)(q - base);
    if (i < ycnt[t]) tx_single(d_src + base, n, ylist[base + i]);
    if (i < zcnt[t]) {
        const int4 z = zlist[base + i];
        tx_single(d_sup + base, n, z);
        const int need = (z.y - z.x) + (z.w - z.z) + 2;
        int bin = TX_BINS;
        for (int c = TX_BINS - 1; c >= 0; --c)
            if (need <= bins.dcap[c]) bin = c;
        // (the host launches the slab path by its own reading of the same plan: a node it does not expect must not
        // vanish)
        if (bin == TX_BINS && !has_slab) atomicOr(flags, 8u);
        const int slot = atomicAdd(zbcnt + (int64_t)bin * nb + t, 1);
        zbin[bin * Lb + base + slot] = i;
    }
}

// the difference arrays live in LDS or, for the slab path, in global memory that other workgroups' lines may share
// a cache with: those loads and stores go past the L1, as the atomics do
template <bool SLAB>
__device__ __forceinline__ unsigned long long tx_ld(const unsigned long long *p) {
    if constexpr (SLAB) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

template <bool SLAB>
__device__ __forceinline__ void tx_st(unsigned long long *p, unsigned long long v) {
    if constexpr (SLAB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

template <bool SLAB>
__device__ __forceinline__ void tx_sync() {
    if constexpr (SLAB) __threadfence();
    __syncthreads();
}

// inclusive prefix sums of d[0, total) by the workgroup, four entries per thread and round; ws: SC_THREADS / 64 sums
template <bool SLAB>
__device__ __forceinline__ void tx_scan(unsigned long long *d, int total, unsigned long long *ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (int c = 0; c < total; c += 4 * SC_THREADS) {
        const int i0 = c + 4 * threadIdx.x;
        unsigned long long v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i0 + e < total ? tx_ld<SLAB>(d + i0 + e) : 0ull;
        v[1] += v[0];
        v[2] += v[1];
        v[3] += v[2];
        unsigned long long incl = v[3];
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long y = __shfl_up(incl, s, 64);
            if (lane >= s) incl += y;
        }
        if (lane == 63) tx_st<SLAB>(ws + wave, incl);
        tx_sync<SLAB>();
        unsigned long long before = carry + incl - v[3];
        for (int w = 0; w < SC_THREADS / 64; ++w) {
            const unsigned long long s = tx_ld<SLAB>(ws + w);
            if (w < wave) before += s;
            carry += s;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < total) tx_st<SLAB>(d + i0 + e, v[e] + before);
        tx_sync<SLAB>();
    }
}

// nz S' nodes of the tree at base (entries zi[0, nz) of its list) against all of T's nodes: rows [2 nz][W] in LDS,
// diff: node j's `in` array (|z| + 1 entries) and `out` array (|pz| + 1) one after the other.  Every array sums to
// zero, so one scan over all of them gives each its own prefix sums.
template <bool SLAB, int ZMAX>
__device__ __forceinline__ void tx_block(int2 *rows, unsigned long long *diff, unsigned long long *ws, int64_t base,
                                         const int4 *__restrict__ zlist, const int32_t *__restrict__ zi, int nz,
                                         const int4 *__restrict__ ylist, int ny, const int2 *__restrict__ tp, int W,
                                         unsigned long long *__restrict__ acc) {
    const int nrow = 2 * nz;
    int oin[ZMAX], oout[ZMAX], total = 0;
#pragma unroll
    for (int j = 0; j < ZMAX; ++j) {
        oin[j] = oout[j] = 0;
        if (j >= nz) continue;
        const int4 z = zlist[base + zi[j]];
        oin[j] = total;
        oout[j] = total + (z.y - z.x) + 1;
        total = oout[j] + (z.w - z.z) + 1;
    }
    for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
    for (int i = threadIdx.x; i < total; i += SC_THREADS) tx_st<SLAB>(diff + i, 0ull);
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);  // (word i of the image: .x of entry i / 2)
    for (int j = 0; j < nz; ++j) {
        const int4 z = zlist[base + zi[j]];
        for (int k = z.x + threadIdx.x; k < z.y; k += SC_THREADS) {
            const int x = tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j) * W + (x >> 5)), 1u << (x & 31));
        }
        for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
            const int x = tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j + 1) * W + (x >> 5)), 1u << (x & 31));
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrow; r += SC_THREADS / 64) {
        int2 *row = rows + r * W;
        int run = 0;
        for (int c = 0; c < W; c += 64) {
            const int i = c + lane;
            const int v = i < W ? __popc((unsigned)row[i].x) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    tx_sync<SLAB>();  // (and the zeroed arrays are in place before the first atomic)
    // the sweep: the eight counts of k_trip_pairs are the ranks the difference arrays are indexed by
    for (int i = threadIdx.x; i < ny; i += SC_THREADS) {
        const int4 y = ylist[base + i];  // T positions [y.x, y.y) of y, [y.z, y.w) of py
        const int wa = y.x >> 5, wb = y.y >> 5, wc = y.z >> 5, wd = y.w >> 5;
        const unsigned ma = (1u << (y.x & 31)) - 1u, mb = (1u << (y.y & 31)) - 1u;
        const unsigned mc = (1u << (y.z & 31)) - 1u, md = (1u << (y.w & 31)) - 1u;
#pragma unroll
        for (int j = 0; j < ZMAX; ++j) {
            if (j >= nz) break;
            const int2 *rz = rows + 2 * j * W, *rp = rz + W;
            const int cza = tp_count(rz, wa, ma), czb = tp_count(rz, wb, mb);
            const int iyz = czb - cza;
            if (iyz < 2) continue;
            const int czc = tp_count(rz, wc, mc), czd = tp_count(rz, wd, md);
            const int cpa = tp_count(rp, wa, ma), cpb = tp_count(rp, wb, mb);
            const int cpc = tp_count(rp, wc, mc), cpd = tp_count(rp, wd, md);
            const int64_t jj = (int64_t)(cpd - cpc) - (cpb - cpa) - (czd - czc) + iyz;
            if (jj == 0) continue;  // (no leaf takes the third place: nothing to hand out)
            const unsigned long long a = (unsigned long long)((int64_t)(iyz - 1) * jj);
            const unsigned long long b = (unsigned long long)((int64_t)iyz * (iyz - 1) / 2);
            unsigned long long *in = diff + oin[j], *out = diff + oout[j];
            atomicAdd(in + cza, a);
            atomicAdd(in + czb, 0ull - a);
            // py ∖ y = [py.lo, y.lo) ∪ [y.hi, py.hi): an empty side (y the first or last child) adds nothing
            if (y.x != y.z) {
                atomicAdd(out + cpc, b);
                atomicAdd(out + cpa, 0ull - b);
            }
            if (y.y != y.w) {
                atomicAdd(out + cpb, b);
                atomicAdd(out + cpd, 0ull - b);
            }
        }
    }
    tx_sync<SLAB>();
    tx_scan<SLAB>(diff, total, ws);
    // the leaf pass: S' position k of pz holds T position x; inside z it reads `in` at its rank in cl(z), else `out`
    // at its rank in cl(pz)
#pragma unroll
    for (int j = 0; j < ZMAX; ++j) {
        if (j >= nz) break;
        const int4 z = zlist[base + zi[j]];
        const int2 *rz = rows + 2 * j * W, *rp = rz + W;
        for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
            const int x = tp[base + k].x;
            const unsigned m = (1u << (x & 31)) - 1u;
            const bool inner = k >= z.x && k < z.y;
            const int r = inner ? oin[j] + tp_count(rz, x >> 5, m) : oout[j] + tp_count(rp, x >> 5, m);
            const unsigned long long v = tx_ld<SLAB>(diff + r);
            if (v) atomicAdd(acc + base + x, v);
        }
    }
}

// SLAB false: one workgroup per (tree t, block of zb of the bin's S' nodes of t), blk and W as in k_trip_pairs, dynamic
// LDS = TX_SCRATCH + zb (16 W + 8 dcap) bytes.  SLAB true (zb = 1, dynamic LDS = 16 W bytes): the workgroups share
// the batch's slab-list nodes round robin, each with its own slab of slab_stride entries.
// zbin / zbcnt: the bin's own list (indices into zlist) and lengths
template <bool SLAB>
__global__ void __launch_bounds__(SC_THREADS) k_tx_pairs(const int64_t *__restrict__ blk, int nb,
                                                         const int64_t *__restrict__ off,
                                                         const int4 *__restrict__ ylist,
                                                         const int4 *__restrict__ zlist,
                                                         const int32_t *__restrict__ ycnt,
                                                         const int32_t *__restrict__ zbin,
                                                         const int32_t *__restrict__ zbcnt,
                                                         const int2 *__restrict__ tp, int zb, int W,
                                                         unsigned long long *__restrict__ slab, int64_t slab_stride,
                                                         unsigned long long *__restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tx_lds[];
    if constexpr (SLAB) {
        int2 *rows = reinterpret_cast<int2 *>(tx_lds);
        unsigned long long *diff = slab + (int64_t)blockIdx.x * slab_stride;
        unsigned long long *ws = diff + slab_stride - TX_SLAB_PAD;
        int64_t first = 0;  // index of the tree's first slab node among the batch's
        for (int t = 0; t < nb; ++t) {
            const int cnt = zbcnt[t];
            const int64_t base = off[t] - off[0];
            int j = (int)(((int64_t)blockIdx.x - first % gridDim.x + gridDim.x) % gridDim.x);
            for (; j < cnt; j += gridDim.x) {
                tx_block<true, 1>(rows, diff, ws, base, zlist, zbin + base + j, 1, ylist, ycnt[t], tp, W, acc);
                tx_sync<true>();  // (the rows and the slab are reused)
            }
            first += cnt;
        }
    } else {
        unsigned long long *ws = reinterpret_cast<unsigned long long *>(tx_lds);
        int2 *rows = reinterpret_cast<int2 *>(tx_lds + TX_SCRATCH);
        const int64_t g = blk[0] + blockIdx.x;
        const int t = sc_tree_of(blk, nb, g);
        const int j0 = (int)(g - blk[t]) * zb;
        const int nz = min(zb, zbcnt[t] - j0);
        if (nz <= 0) return;  // (the grid counts n - 2 nodes per tree and bin: an upper bound)
        const int64_t base = off[t] - off[0];
        unsigned long long *diff = reinterpret_cast<unsigned long long *>(rows + (int64_t)2 * zb * W);
        tx_block<false, TP_ZMAX>(rows, diff, ws, base, zlist, zbin + base + j0, nz, ylist, ycnt[t], tp, W, acc);
    }
}

// inclusive prefix sums of both single-tree rows over every tree's own entries, one workgroup per tree
__global__ void __launch_bounds__(SC_THREADS) k_tx_scan(const int64_t *__restrict__ off,
                                                        unsigned long long *__restrict__ d_src,
                                                        unsigned long long *__restrict__ d_sup) {
    __shared__ unsigned long long ws[SC_THREADS / 64];
    const int t = blockIdx.x;
    const int64_t base = off[t] - off[0];
    const int n = (int)(off[t + 1] - off[t]);
    tx_scan<false>(d_src + base, n, ws);
    tx_scan<false>(d_sup + base, n, ws);
}

// one thread per leaf of the batch: T position q - base gives its taxon the shared and source sums, S' position
// q - base gives the taxon of its leaf the super sum; tx: five arrays of n_out entries (trees, total, super, source,
// shared)
__global__ void __launch_bounds__(SC_THREADS) k_tx_fold(const int64_t *__restrict__ off, int nb,
                                                        const int32_t *__restrict__ leaf_taxon,
                                                        const int2 *__restrict__ tp,
                                                        const unsigned long long *__restrict__ acc,
                                                        const unsigned long long *__restrict__ d_src,
                                                        const unsigned long long *__restrict__ d_sup,
                                                        unsigned long long *__restrict__ tx, int64_t n_out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = off[0] + q;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    const int64_t n = off[t + 1] - off[t];
    if (n < 3) return;
    const int32_t x = leaf_taxon[p];
    atomicAdd(tx + x, 1ull);
    atomicAdd(tx + n_out + x, (unsigned long long)((n - 1) * (n - 2) / 2));
    if (d_src[q]) atomicAdd(tx + 3 * n_out + x, d_src[q]);
    if (acc[q]) atomicAdd(tx + 4 * n_out + x, acc[q]);
    const int32_t xs = leaf_taxon[off[t] + tp[q].x];
    if (d_sup[q]) atomicAdd(tx + 2 * n_out + xs, d_sup[q]);
}

// ---- taxon placement support (scs_score_placements) ----
//
// For a query taxon x and a node v of S, S_{x->v} is S with x pruned and regrafted on the edge above v.  Fix a source T
// on L with x in L; every set below is restricted to L.  The groups of x in T are the clusters y with x not in y and
// x in py (the subtrees hanging off x's root path, leaves included); they partition L - {x}.  Of the pairs {a, b} of
// L - {x}, T says ab|x when a and b share a group and xa|b when a is in y and b outside py.  With
//   A(z) = sum_y C(|y ∩ z|, 2)   and   X(z) = sum_y |y ∩ z| (|pz - py| - |z - py|)       (z a node of S' = S|L)
// the triples {x, a, b} that T and S_{x->v} resolve alike are a root-path sum: A(root of S') for every v, and for every
// node z of S' with parent pz, + A(z) strictly below the S node of pz, - A(z) strictly below z's own S node, and
// + X(z) on the subtree of the highest S node whose restricted set is z's.  The triples S_{x->v} resolves follow the
// same sums with A1 = C(|z - x|, 2) and X1 = |z - x| (|pz - x| - |z - x|).  x lies in no group but in every py, so no
// count over a group needs a correction for it.
//   k_pl_queries: per (tree, query): x's T position and S' index (-1 when the tree lacks x or has under 3 leaves);
//     per tree the number of queries it holds.
//   k_pl_znodes, one thread per leaf: every node of S', leaves and root included, as int4 {lo, hi + 1, parent lo,
//     parent hi + 1} in S order and int4 {own S node (-1: a leaf), parent's S node (-1: the root), top S node, 0}.
//   k_pl_groups, one thread per leaf: T's leaf k and the node whose first gap is k go, with their parent's range, into
//     the list of every query of the tree that the parent holds and the node does not; pl_source on the way.
//   k_pl_pairs: the grid and rows of k_trip_pairs; the workgroup sweeps the group lists of its tree's queries, adds
//     A and X per (z, query) in LDS, and issues the non-zero marks as 64-bit atomics on two rows per query: `sub`
//     (counts for the node's subtree) and `strict` (for its strict descendants).  The super marks of a taxon outside
//     pz do not depend on the taxon: a tree that holds every query of the pass sends them once, to rows common to the
//     pass, and a query adds only what its own place in z or pz changes.
//   k_pl_marks / k_pl_prefix: mark(u) = sub[u] + strict[parent u] on the preorder range [u, end u) of a difference
//     row, and its prefix sums: the value of every node.

constexpr int PL_QMAX = 64;  // query taxa per pass over a batch (a group list entry per leaf and query: 1 KB a leaf)

// the highest S node below the node of depth d whose leaves hold S position p: its first leaf lies after the nearest
// gap to the left that is no deeper than d, and the path from a node to its first leaf takes first children only,
// which follow their parents at once in preorder
__device__ __forceinline__ int32_t pl_top(const uint64_t *__restrict__ s_tab, int64_t stride, int s_levels,
                                          const int32_t *__restrict__ tip_node, const int32_t *__restrict__ tip_depth,
                                          int32_t p, int32_t d) {
    int64_t pos = p;
    for (int j = s_levels - 1; j >= 0; --j) {
        const int64_t w = (int64_t)1 << j;
        if (pos >= w && (int32_t)(s_tab[j * stride + pos - w] >> 32) > d) pos -= w;
    }
    return tip_node[pos] - (tip_depth[pos] - (d + 1));
}

__global__ void __launch_bounds__(SC_THREADS) k_pl_queries(const int64_t *__restrict__ off, int nb,
                                                           const int32_t *__restrict__ q_spos, int qc,
                                                           const int32_t *__restrict__ rows, int64_t row_stride,
                                                           const int32_t *__restrict__ sp, int2 *__restrict__ qinfo,
                                                           int32_t *__restrict__ gcnt, int32_t *__restrict__ qheld,
                                                           unsigned long long *__restrict__ q_trees,
                                                           unsigned long long *__restrict__ q_total) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)nb * qc) return;
    const int t = (int)(idx / qc), i = (int)(idx % qc);
    const int64_t base = off[t] - off[0], n = off[t + 1] - off[t];
    const int32_t s = q_spos[i];
    int32_t px = -1, kx = -1;
    if (n >= 3 && s >= 0) {
        px = rows[(int64_t)t * row_stride + s];
        if (px >= 0) {
            kx = (int32_t)sc_first_ge(sp + base, 0, n, s);
            atomicAdd(qheld + t, 1);
            atomicAdd(q_trees + i, 1ull);
            atomicAdd(q_total + i, (unsigned long long)((n - 1) * (n - 2) / 2));
        }
    }
    qinfo[idx] = make_int2(px, kx);
    gcnt[idx] = 0;
}

struct sc_pl_args : sc_batch {
    const int32_t *tip_node, *tip_depth;    // [S leaves] preorder index and depth of the tip at an S position
    int4 *zlist, *zmeta;                    // [2 Lb]: the nodes of a tree from twice its first leaf on
    int32_t *zcnt;                          // [nb]
    const int2 *qinfo;                      // [nb][qc]
    int qc;
    int4 *glist;                            // [Lb qc]: tree t, query i from base qc + i n on
    int32_t *gcnt;                          // [nb][qc]
    unsigned long long *q_source;           // [qc]
};

// one thread per leaf k of a tree of 3 or more leaves: S' leaf k, and the S' node whose first gap is k
__global__ void __launch_bounds__(SC_THREADS) k_pl_znodes(sc_pl_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    const bool leaf = in && n >= 3;
    bool inner = false;
    int4 zl = make_int4(0, 0, 0, 0), ml = zl, zi = zl, mi = zl;
    if (leaf) {
        const int32_t *sp = a.sp + base;
        {
            const int64_t g = k == 0 ? 0 : k == n - 1 ? n - 2 : (a.dep[base + k - 1] >= a.dep[base + k] ? k - 1 : k);
            const int32_t w = a.node[base + g];
            const int64_t plo = sc_first_ge(sp, 0, k, a.s_lo[w]);
            const int64_t phi = sc_last_le(sp, k, n - 1, a.s_hi[w]);
            zl = make_int4((int)k, (int)k + 1, (int)plo, (int)phi + 1);
            ml = make_int4(-1, w, pl_top(a.s_tab, a.s_stride, a.s_levels, a.tip_node, a.tip_depth, sp[k],
                                         a.dep[base + g]), 0);
        }
        if (k + 1 < n) {
            const int32_t u = a.node[q], du = a.dep[q];
            const int64_t lo_s = sc_first_ge(sp, 0, k, a.s_lo[u]);
            const int64_t hi_s = sc_last_le(sp, k + 1, n - 1, a.s_hi[u]);
            inner = lo_s == k ||
                    (int32_t)(sc_rmq_min(a.s_tab, a.s_stride, (int64_t)sp[lo_s], (int64_t)sp[k] - 1) >> 32) > du;
            if (inner && lo_s == 0 && hi_s == n - 1) {  // the root: its own parent, and above it every node of S
                zi = make_int4(0, (int)n, 0, (int)n);
                mi = make_int4(u, -1, 0, 0);
            } else if (inner) {
                const int64_t g = lo_s == 0 ? hi_s
                                  : hi_s == n - 1 ? lo_s - 1
                                  : (a.dep[base + lo_s - 1] >= a.dep[base + hi_s] ? lo_s - 1 : hi_s);
                const int32_t w = a.node[base + g];
                const int64_t plo = sc_first_ge(sp, 0, lo_s, a.s_lo[w]);
                const int64_t phi = sc_last_le(sp, hi_s, n - 1, a.s_hi[w]);
                zi = make_int4((int)lo_s, (int)hi_s + 1, (int)plo, (int)phi + 1);
                mi = make_int4(u, w, pl_top(a.s_tab, a.s_stride, a.s_levels, a.tip_node, a.tip_depth, sp[lo_s],
                                            a.dep[base + g]), 0);
            }
        }
    }
    const int il = sc_append(a.zcnt, t, leaf);
    if (il >= 0) {
        a.zlist[2 * base + il] = zl;
        a.zmeta[2 * base + il] = ml;
    }
    const int ii = sc_append(a.zcnt, t, inner);
    if (ii >= 0) {
        a.zlist[2 * base + ii] = zi;
        a.zmeta[2 * base + ii] = mi;
    }
}

// node [lo, hi) of T with parent [plo, phi) into the list of every query of tree t that the parent holds and the node
// does not; the pairs {a, b} it gives T a resolved triple {x, a, b} for: both inside it, or a inside and b outside py
__device__ __forceinline__ void pl_group(const sc_pl_args &a, int t, int64_t base, int64_t n, int4 e) {
    const int64_t s = e.y - e.x;
    const unsigned long long v = (unsigned long long)(s * (s - 1) / 2 + s * (n - (e.w - e.z)));
    for (int i = 0; i < a.qc; ++i) {
        const int32_t px = a.qinfo[(int64_t)t * a.qc + i].x;
        if (px < e.z || px >= e.w || (px >= e.x && px < e.y)) continue;
        const int slot = atomicAdd(a.gcnt + (int64_t)t * a.qc + i, 1);
        a.glist[base * a.qc + (int64_t)i * n + slot] = e;
        atomicAdd(a.q_source + i, v);
    }
}

// one thread per leaf k of a tree: T's leaf k, and T's node whose first gap is k (as in k_trip_nodes)
__global__ void __launch_bounds__(SC_THREADS) k_pl_groups(sc_pl_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    if (p >= a.off[a.nb]) return;
    const int t = sc_tree_of(a.off, a.nb, p);
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    if (n < 3) return;
    {
        const int64_t g = k == 0 ? 0 : k == n - 1 ? n - 2 : (a.adj[base + k - 1] >= a.adj[base + k] ? k - 1 : k);
        const int32_t dg = a.adj[base + g];
        const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
        const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
        pl_group(a, t, base, n, make_int4((int)k, (int)k + 1, (int)plo, (int)phi + 1));
    }
    if (k + 1 >= n) return;
    const int32_t d = a.adj[q];
    const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
    if (lo != 0 && a.adj[base + lo - 1] >= d) return;  // (not the node's first gap)
    const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
    if (lo == 0 && hi == n - 1) return;  // (the root)
    const int64_t g = lo == 0 ? hi : hi == n - 1 ? lo - 1 : (a.adj[base + lo - 1] >= a.adj[base + hi] ? lo - 1 : hi);
    const int32_t dg = a.adj[base + g];
    const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
    const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
    pl_group(a, t, base, n, make_int4((int)lo, (int)hi + 1, (int)plo, (int)phi + 1));
}

// the marks of one (z, query) on the query's two rows: av for the strict descendants of pz's S node (every node when
// z is the root) and not for those of z's own, xv for the subtree of z's top node
__device__ __forceinline__ void pl_emit(unsigned long long *__restrict__ sub, unsigned long long *__restrict__ strict,
                                        int4 meta, unsigned long long av, unsigned long long xv) {
    if (av) {
        atomicAdd(meta.y < 0 ? sub : strict + meta.y, av);
        if (meta.x >= 0) atomicAdd(strict + meta.x, 0ull - av);
    }
    if (xv) atomicAdd(sub + meta.z, xv);
}

struct sc_pl_pair_args {
    const int64_t *blk;       // first workgroup of the batch's tree i (cumulative, blk[0] = the batch's own start)
    int nb;
    const int64_t *off;
    const int4 *glist;
    const int32_t *gcnt;
    const int2 *qinfo;
    const int32_t *qheld;     // [nb] queries of the pass the tree holds
    int qc;
    const int4 *zlist, *zmeta;
    const int32_t *zcnt;
    const int2 *tp;
    int zb, W;
    int lds_sums;             // A and X summed per (z, query) in LDS; else every (z, y) sends its own marks
    unsigned long long *sub, *strict;  // rows [2][n_queries][n_nodes] (shared, super), at the pass's first query
    int64_t row_stride;       // n_nodes
    int64_t super_off;        // n_queries * n_nodes
    unsigned long long *csub, *cstrict;  // [n_nodes] each: marks of the super rows of every query of the pass
};

// the hot path: one workgroup per (tree t, block of zb of t's S' nodes).  LDS: with lds_sums the sums [zb][qc]{A, X},
// the nodes [zb]{range, meta} and the list offsets [qc + 1]; then the rows [2 zb][W] of k_trip_pairs
__global__ void __launch_bounds__(SC_THREADS) k_pl_pairs(sc_pl_pair_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pl_lds[];
    const int64_t g = a.blk[0] + blockIdx.x;
    const int t = sc_tree_of(a.blk, a.nb, g);
    const int j0 = (int)(g - a.blk[t]) * a.zb;
    const int nz = min(a.zb, a.zcnt[t] - j0);
    if (nz <= 0) return;
    const int qc = a.qc, W = a.W;
    const int2 *qinfo = a.qinfo + (int64_t)t * qc;
    if (a.qheld[t] == 0) return;  // (the tree holds no query of this pass)
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int4 *zlist = a.zlist + 2 * base + j0, *zmeta = a.zmeta + 2 * base + j0;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(pl_lds);
    int4 *zs = reinterpret_cast<int4 *>(sums + (a.lds_sums ? 2 * a.zb * qc : 0));
    int *pref = reinterpret_cast<int *>(zs + (a.lds_sums ? 2 * a.zb : 0));
    int2 *rows = reinterpret_cast<int2 *>(pl_lds + (a.lds_sums ? 16 * a.zb * qc + 32 * a.zb + 4 * ((qc + 4) & ~3) : 0));
    const int nrow = 2 * nz;
    for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
    if (a.lds_sums) {
        for (int i = threadIdx.x; i < 2 * nz * qc; i += SC_THREADS) sums[i] = 0;
        for (int i = threadIdx.x; i < nz; i += SC_THREADS) {
            zs[2 * i] = zlist[i];
            zs[2 * i + 1] = zmeta[i];
        }
        if (threadIdx.x == 0) {
            int run = 0;
            for (int i = 0; i < qc; ++i) {
                pref[i] = run;
                run += a.gcnt[(int64_t)t * qc + i];
            }
            pref[qc] = run;
        }
    }
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);
    for (int j = 0; j < nz; ++j) {
        const int4 z = zlist[j];
        for (int k = z.x + threadIdx.x; k < z.y; k += SC_THREADS) {
            const int x = a.tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j) * W + (x >> 5)), 1u << (x & 31));
        }
        for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
            const int x = a.tp[base + k].x;
            atomicOr(bits + 2 * ((2 * j + 1) * W + (x >> 5)), 1u << (x & 31));
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < nrow; r += SC_THREADS / 64) {
        int2 *row = rows + r * W;
        int run = 0;
        for (int c = 0; c < W; c += 64) {
            const int i = c + lane;
            const int v = i < W ? __popc((unsigned)row[i].x) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    // A and X of one (z, y): y's T positions [y.x, y.y), py's [y.z, y.w)
    const auto pair = [&](const int4 y, int j, int4 z, unsigned long long &av, unsigned long long &xv) {
        const int2 *rz = rows + 2 * j * W, *rp = rz + W;
        const int wa = y.x >> 5, wb = y.y >> 5;
        const unsigned ma = (1u << (y.x & 31)) - 1u, mb = (1u << (y.y & 31)) - 1u;
        const int iyz = tp_count(rz, wb, mb) - tp_count(rz, wa, ma);
        if (iyz == 0) return false;
        const int wc = y.z >> 5, wd = y.w >> 5;
        const unsigned mc = (1u << (y.z & 31)) - 1u, md = (1u << (y.w & 31)) - 1u;
        const int ipyz = tp_count(rz, wd, md) - tp_count(rz, wc, mc);
        const int ipp = tp_count(rp, wd, md) - tp_count(rp, wc, mc);
        av = (unsigned long long)((int64_t)iyz * (iyz - 1) / 2);
        xv = (unsigned long long)((int64_t)iyz * (((z.w - z.z) - ipp) - ((z.y - z.x) - ipyz)));
        return true;
    };
    if (a.lds_sums) {
        const int total = pref[qc];
        for (int e = threadIdx.x; e < total; e += SC_THREADS) {
            int i = 0, hi = qc;  // pref[i] <= e < pref[hi]
            while (hi - i > 1) {
                const int m = (i + hi) >> 1;
                if (pref[m] <= e) i = m; else hi = m;
            }
            const int4 y = a.glist[base * qc + (int64_t)i * n + (e - pref[i])];
            for (int j = 0; j < nz; ++j) {
                unsigned long long av, xv;
                if (!pair(y, j, zs[2 * j], av, xv)) continue;
                if (av) atomicAdd(sums + 2 * (j * qc + i), av);
                if (xv) atomicAdd(sums + 2 * (j * qc + i) + 1, xv);
            }
        }
        __syncthreads();
    } else {
        for (int i = 0; i < qc; ++i) {
            const int cnt = a.gcnt[(int64_t)t * qc + i];
            for (int e = threadIdx.x; e < cnt; e += SC_THREADS) {
                const int4 y = a.glist[base * qc + (int64_t)i * n + e];
                for (int j = 0; j < nz; ++j) {
                    unsigned long long av, xv;
                    if (!pair(y, j, zlist[j], av, xv)) continue;
                    pl_emit(a.sub + i * a.row_stride, a.strict + i * a.row_stride, zmeta[j], av, xv);
                }
            }
        }
    }
    // a tree that holds every query of the pass sends the super marks of a taxon outside pz once, to the pass's common
    // rows; a query then adds what its own place in z or pz changes (nothing for most z)
    const bool common = a.qheld[t] == qc;
    if (common)
        for (int j = threadIdx.x; j < nz; j += SC_THREADS) {
            const int4 z = a.lds_sums ? zs[2 * j] : zlist[j];
            const int64_t sz = z.y - z.x, spz = z.w - z.z;
            pl_emit(a.csub, a.cstrict, a.lds_sums ? zs[2 * j + 1] : zmeta[j], (unsigned long long)(sz * (sz - 1) / 2),
                    (unsigned long long)(sz * (spz - sz)));
        }
    // per (z, query the tree holds): the summed marks of the shared row, the closed-form marks of the super row
    for (int it = threadIdx.x; it < nz * qc; it += SC_THREADS) {
        const int j = it / qc, i = it % qc;
        const int kx = qinfo[i].y;
        if (kx < 0) continue;
        const int4 z = a.lds_sums ? zs[2 * j] : zlist[j], meta = a.lds_sums ? zs[2 * j + 1] : zmeta[j];
        if (a.lds_sums)
            pl_emit(a.sub + i * a.row_stride, a.strict + i * a.row_stride, meta, sums[2 * it], sums[2 * it + 1]);
        const int64_t sz = (z.y - z.x) - (kx >= z.x && kx < z.y), spz = (z.w - z.z) - (kx >= z.z && kx < z.w);
        unsigned long long av = (unsigned long long)(sz * (sz - 1) / 2), xv = (unsigned long long)(sz * (spz - sz));
        if (common) {
            const int64_t s0 = z.y - z.x, p0 = z.w - z.z;
            av -= (unsigned long long)(s0 * (s0 - 1) / 2);
            xv -= (unsigned long long)(s0 * (p0 - s0));
        }
        pl_emit(a.sub + a.super_off + i * a.row_stride, a.strict + a.super_off + i * a.row_stride, meta, av, xv);
    }
}

// mark(u) = sub[u] + strict[parent u] on [u, end u) of the row's difference array (zeroed; n + 1 entries); the rows
// [n_rows / 2, n_rows) are the super rows of the queries, pass by pass of qcap queries: they take their pass's common
// rows [pass][n] as well
__global__ void __launch_bounds__(SC_THREADS) k_pl_marks(const unsigned long long *__restrict__ sub,
                                                         const unsigned long long *__restrict__ strict,
                                                         const unsigned long long *__restrict__ csub,
                                                         const unsigned long long *__restrict__ cstrict, int qcap,
                                                         const int32_t *__restrict__ parent,
                                                         const int32_t *__restrict__ end, int64_t n, int64_t n_rows,
                                                         unsigned long long *__restrict__ diff) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n_rows) return;
    const int64_t r = idx / n, u = idx % n;
    unsigned long long m = sub[idx] + (u ? strict[r * n + parent[u]] : 0ull);
    if (2 * r >= n_rows) {
        const int64_t pass = (r - n_rows / 2) / qcap;
        m += csub[pass * n + u] + (u ? cstrict[pass * n + parent[u]] : 0ull);
    }
    if (!m) return;
    atomicAdd(diff + r * (n + 1) + u, m);
    atomicAdd(diff + r * (n + 1) + end[u], 0ull - m);
}

// inclusive prefix sums of every row's difference array: the values of the row's nodes, one workgroup per row
__global__ void __launch_bounds__(1024) k_pl_prefix(const unsigned long long *__restrict__ diff, int64_t n,
                                                    unsigned long long *__restrict__ out) {
    __shared__ unsigned long long ws[16];
    const unsigned long long *d = diff + (int64_t)blockIdx.x * (n + 1);
    unsigned long long *o = out + (int64_t)blockIdx.x * n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long run = 0;
    for (int64_t c = 0; c < n; c += 1024) {
        const int64_t i = c + threadIdx.x;
        unsigned long long x = i < n ? d[i] : 0;
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long y = __shfl_up(x, s, 64);
            if (lane >= s) x += y;
        }
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        unsigned long long before = run, total = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += ws[w];
            total += ws[w];
        }
        if (i < n) o[i] = before + x;
        run += total;
        __syncthreads();
    }
}

// ---- scs_score_clade_placements: the triplet terms a whole clade of the supertree would have on the edge above every
// node.  Q is the clade's leaf set, Q' = Q ∩ L (a range of S' leaves), R = L ∖ Q.  The triples
// with two taxa in Q' do not depend on the edge: node sums over T (k_cp_nodes) and a closed form (k_cp_clades).  Those
// with one taxon x in Q' follow the recurrence of scs_score_placements on the ground set R ∪ {x}: every tip of Q' is a
// sub-query whose group list is swept against the rows as there, every count is intersected with R (an S' node inside
// Q' has no taxon of R and sends nothing, one that holds Q' loses |· ∩ Q'|, which a group brings along from a bitset
// row of Q' over T positions), and the marks of all the tips of a clade go to the clade's own pair of rows.
//   k_cp_clades, a workgroup per (tree, clade of the pass): Q' as a range of S' leaves, its bitset row over T positions
//     (global memory, the word format of k_trip_pairs), cp_trees, cp_total and the closed form C(|Q'|, 2) |R|.
//   k_cp_queries, per (tree, sub-query): the tip's T position, -1 unless the tree crosses the clade.
//   k_cp_nodes, one thread per leaf: T's node whose first gap it is, against the Q' row of every clade that begins in
//     this pass: cp_source and the shared triples with two taxa in Q'.
//   k_cp_groups: k_pl_groups with |y ∩ Q'| and |py ∩ Q'| beside every list entry.
//   k_cp_pairs, the hot kernel: k_pl_pairs with the masked counts, sums per (z, clade) and the closed-form super marks
//     once per (z, clade), times |Q'|.
//   k_cp_marks, then k_pl_prefix: the rows' values.

constexpr int CP_QMAX = 64;  // sub-queries (tips of query clades) per pass over a batch

struct sc_cp_args : sc_batch {    // (mm: .x of its level 0 is the T position of every S' leaf)
    const int32_t *rows;            // [nb][row_stride] T position by S position
    int64_t row_stride;
    const int32_t *c_lo, *c_hi;     // [ncl] S leaf range of the pass's clades
    const int32_t *q_spos, *q_slot; // [qc] S position and clade (slot in the pass) of the pass's sub-queries
    int ncl, qc;
    int skip0;                      // the pass's first clade began in an earlier pass: its own sums are done
    int2 *qrow;                     // [ncl][rstride] Q' rows, tree t from (base >> 5) + t on
    int64_t rstride;
    int4 *cinfo;                    // [nb][ncl] {first S' leaf of Q', end, crossing, 0}
    int2 *qinfo;                    // [nb][qc] {T position of the tip or -1, slot}
    int32_t *gcnt;                  // [nb][qc]
    int32_t *qheld;                 // [nb]
    int4 *glist;                    // [Lb qc]: tree t, sub-query i from base qc + i n on
    int2 *gq;                       // beside glist: {|y ∩ Q'|, |py ∩ Q'|}
    unsigned long long *c_trees, *c_total, *c_source;  // [ncl] at the pass's first clade
    unsigned long long *sub;        // rows [2][n_clades][n_nodes] (shared, super), at the pass's first clade
    int64_t node_stride, super_off;
};

__global__ void __launch_bounds__(SC_THREADS) k_cp_clades(sc_cp_args a) {
    const int t = blockIdx.x / a.ncl, c = blockIdx.x % a.ncl;
    const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
    const int32_t *sp = a.sp + base;
    const int64_t ka = sc_first_ge(sp, 0, n, a.c_lo[c]);
    const int64_t kb = sc_first_ge(sp, ka, n, a.c_hi[c] + 1);
    const int64_t nq = kb - ka;
    const bool cross = n >= 3 && nq > 0 && nq < n;
    if (threadIdx.x == 0) a.cinfo[(int64_t)t * a.ncl + c] = make_int4((int)ka, (int)kb, cross ? 1 : 0, 0);
    if (!cross) return;
    int2 *row = a.qrow + (int64_t)c * a.rstride + (base >> 5) + t;
    const int W = (int)(n >> 5) + 1;
    unsigned *bits = reinterpret_cast<unsigned *>(row);  // (zeroed by the host before the launch)
    for (int64_t k = ka + threadIdx.x; k < kb; k += SC_THREADS) {
        const int x = a.mm[base + k].x;
        atomicOr(bits + 2 * (x >> 5), 1u << (x & 31));
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        int run = 0;
        for (int w0 = 0; w0 < W; w0 += 64) {
            const int i = w0 + lane;
            // (the bits were set by atomics of other waves: read them where the atomics ran)
            const int v = i < W ? __popc(__hip_atomic_load(bits + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    if (threadIdx.x == 0 && !(c == 0 && a.skip0)) {
        const int64_t r = n - nq;
        atomicAdd(a.c_trees + c, 1ull);
        atomicAdd(a.c_total + c, (unsigned long long)(n * (n - 1) * (n - 2) / 6 - nq * (nq - 1) * (nq - 2) / 6 -
                                                      r * (r - 1) * (r - 2) / 6));
        // two taxa in Q', one in R: S says xx'|b on every edge
        if (nq >= 2) atomicAdd(a.sub + a.super_off + c * a.node_stride, (unsigned long long)(nq * (nq - 1) / 2 * r));
    }
}

__global__ void __launch_bounds__(SC_THREADS) k_cp_queries(sc_cp_args a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)a.nb * a.qc) return;
    const int t = (int)(idx / a.qc), i = (int)(idx % a.qc);
    const int c = a.q_slot[i];
    int32_t px = -1;
    if (a.cinfo[(int64_t)t * a.ncl + c].z) {
        px = a.rows[(int64_t)t * a.row_stride + a.q_spos[i]];
        if (px >= 0) atomicAdd(a.qheld + t, 1);
    }
    a.qinfo[idx] = make_int2(px, c);
    a.gcnt[idx] = 0;
}

// |[lo, hi) ∩ Q'| over T positions, from a Q' row
__device__ __forceinline__ int cp_range(const int2 *__restrict__ row, int lo, int hi) {
    return tp_count(row, hi >> 5, (1u << (hi & 31)) - 1u) - tp_count(row, lo >> 5, (1u << (lo & 31)) - 1u);
}

// T's node [lo, hi] whose first gap is k, with its parent [plo, phi]; false for a leaf's thread without one, the root
__device__ __forceinline__ bool cp_tnode(const sc_cp_args &a, int64_t base, int64_t n, int64_t k, int4 &e) {
    if (k + 1 >= n) return false;
    const int32_t d = a.adj[base + k];
    const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
    if (lo != 0 && a.adj[base + lo - 1] >= d) return false;  // (not the node's first gap)
    const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
    if (lo == 0 && hi == n - 1) return false;  // (the root)
    const int64_t g = lo == 0 ? hi : hi == n - 1 ? lo - 1 : (a.adj[base + lo - 1] >= a.adj[base + hi] ? lo - 1 : hi);
    const int32_t dg = a.adj[base + g];
    const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
    const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
    e = make_int4((int)lo, (int)hi + 1, (int)plo, (int)phi + 1);
    return true;
}

// the node sums of the clades that begin in this pass: cp_source and the shared triples with two taxa in Q'
__global__ void __launch_bounds__(SC_THREADS) k_cp_nodes(sc_cp_args a) {
    __shared__ unsigned long long acc[2 * CP_QMAX];
    for (int i = threadIdx.x; i < 2 * a.ncl; i += SC_THREADS) acc[i] = 0;
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    if (p < a.off[a.nb]) {
        const int t = sc_tree_of(a.off, a.nb, p);
        const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
        int4 e;
        if (n >= 3 && cp_tnode(a, base, n, q - base, e)) {
            const int64_t s = e.y - e.x, out = (e.w - e.z) - s;
            for (int c = a.skip0 ? 1 : 0; c < a.ncl; ++c) {
                if (!a.cinfo[(int64_t)t * a.ncl + c].z) continue;
                const int2 *row = a.qrow + (int64_t)c * a.rstride + (base >> 5) + t;
                const int64_t pq = cp_range(row, e.z, e.w);
                if (pq == 0) continue;  // (py lies in R: nothing crosses)
                const int64_t yq = cp_range(row, e.x, e.y), yr = s - yq, oq = pq - yq, orr = out - oq;
                const int64_t both = yq * (yq - 1) / 2 * orr;
                const int64_t src = s * (s - 1) / 2 * out - yq * (yq - 1) / 2 * oq - yr * (yr - 1) / 2 * orr;
                if (src) atomicAdd(acc + 2 * c, (unsigned long long)src);
                if (both) atomicAdd(acc + 2 * c + 1, (unsigned long long)both);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * a.ncl; i += SC_THREADS) {
        if (!acc[i]) continue;
        const int c = i >> 1;
        atomicAdd((i & 1) ? a.sub + c * a.node_stride : a.c_source + c, acc[i]);
    }
}

__device__ __forceinline__ void cp_group(const sc_cp_args &a, int t, int64_t base, int64_t n, int4 e) {
    for (int i = 0; i < a.qc; ++i) {
        const int2 qi = a.qinfo[(int64_t)t * a.qc + i];
        const int32_t px = qi.x;
        if (px < e.z || px >= e.w || (px >= e.x && px < e.y)) continue;
        const int2 *row = a.qrow + (int64_t)qi.y * a.rstride + (base >> 5) + t;
        const int slot = atomicAdd(a.gcnt + (int64_t)t * a.qc + i, 1);
        const int64_t at = base * a.qc + (int64_t)i * n + slot;
        a.glist[at] = e;
        a.gq[at] = make_int2(cp_range(row, e.x, e.y), cp_range(row, e.z, e.w));
    }
}

// one thread per leaf k of a tree: T's leaf k, and T's node whose first gap is k, into the sub-queries' group lists
__global__ void __launch_bounds__(SC_THREADS) k_cp_groups(sc_cp_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    if (p >= a.off[a.nb]) return;
    const int t = sc_tree_of(a.off, a.nb, p);
    if (a.qheld[t] == 0) return;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    if (n < 3) return;
    {
        const int64_t g = k == 0 ? 0 : k == n - 1 ? n - 2 : (a.adj[base + k - 1] >= a.adj[base + k] ? k - 1 : k);
        const int32_t dg = a.adj[base + g];
        const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
        const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
        cp_group(a, t, base, n, make_int4((int)k, (int)k + 1, (int)plo, (int)phi + 1));
    }
    int4 e;
    if (cp_tnode(a, base, n, k, e)) cp_group(a, t, base, n, e);
}

struct sc_cp_pair_args {
    const int64_t *blk;       // first workgroup of the batch's tree i (cumulative, blk[0] = the batch's own start)
    int nb;
    const int64_t *off;
    const int4 *glist;
    const int2 *gq;
    const int32_t *gcnt;
    const int2 *qinfo;
    const int4 *cinfo;
    const int32_t *qheld;
    int qc, ncl, skip0;
    const int4 *zlist, *zmeta;
    const int32_t *zcnt;
    const int2 *tp;
    int zb, W;
    int lds_sums;             // A and X summed per (z, clade) in LDS; else every (z, y) sends its own marks
    unsigned long long *sub, *strict;  // rows [2][n_clades][n_nodes] (shared, super), at the pass's first clade
    int64_t row_stride;       // n_nodes
    int64_t super_off;        // n_clades * n_nodes
};

// z's and pz's sizes without Q' = [ka, kb) of S' (nq leaves): false when z lies inside Q' and holds no taxon of R
__device__ __forceinline__ bool cp_masked(int4 z, int ka, int kb, int &cz, int &cp) {
    if (z.x >= ka && z.y <= kb) return false;
    cz = z.x <= ka && kb <= z.y;
    cp = z.z <= ka && kb <= z.w;
    return true;
}

// the hot path: one workgroup per (tree t, block of zb of t's S' nodes).  LDS: with lds_sums the sums [zb][qc]{A, X},
// the nodes [zb]{range, meta} and the list offsets [qc + 1]; then the rows [2 zb][W] of k_trip_pairs
__global__ void __launch_bounds__(SC_THREADS) k_cp_pairs(sc_cp_pair_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cp_lds[];
    const int64_t g = a.blk[0] + blockIdx.x;
    const int t = sc_tree_of(a.blk, a.nb, g);
    const int j0 = (int)(g - a.blk[t]) * a.zb;
    const int nz = min(a.zb, a.zcnt[t] - j0);
    if (nz <= 0) return;
    const int qc = a.qc, W = a.W, ncl = a.ncl;
    const int2 *qinfo = a.qinfo + (int64_t)t * qc;
    const int4 *cinfo = a.cinfo + (int64_t)t * ncl;
    const bool any_first = [&] {
        for (int c = a.skip0 ? 1 : 0; c < ncl; ++c)
            if (cinfo[c].z) return true;
        return false;
    }();
    if (a.qheld[t] == 0 && !any_first) return;  // (the tree crosses no clade of this pass)
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int4 *zlist = a.zlist + 2 * base + j0, *zmeta = a.zmeta + 2 * base + j0;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(cp_lds);
    int4 *zs = reinterpret_cast<int4 *>(sums + (a.lds_sums ? 2 * a.zb * qc : 0));
    int *pref = reinterpret_cast<int *>(zs + (a.lds_sums ? 2 * a.zb : 0));
    int2 *rows = reinterpret_cast<int2 *>(cp_lds + (a.lds_sums ? 16 * a.zb * qc + 32 * a.zb + 4 * ((qc + 4) & ~3) : 0));
    const int nrow = 2 * nz;
    if (a.lds_sums) {
        for (int i = threadIdx.x; i < 2 * nz * qc; i += SC_THREADS) sums[i] = 0;
        for (int i = threadIdx.x; i < nz; i += SC_THREADS) {
            zs[2 * i] = zlist[i];
            zs[2 * i + 1] = zmeta[i];
        }
        if (threadIdx.x == 0) {
            int run = 0;
            for (int i = 0; i < qc; ++i) {
                pref[i] = run;
                run += a.gcnt[(int64_t)t * qc + i];
            }
            pref[qc] = run;
        }
    }
    if (a.qheld[t] != 0) {  // (uniform over the workgroup: the rows serve the sweep only)
        for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
        __syncthreads();
        unsigned *bits = reinterpret_cast<unsigned *>(rows);
        for (int j = 0; j < nz; ++j) {
            const int4 z = zlist[j];
            for (int k = z.x + threadIdx.x; k < z.y; k += SC_THREADS) {
                const int x = a.tp[base + k].x;
                atomicOr(bits + 2 * ((2 * j) * W + (x >> 5)), 1u << (x & 31));
            }
            for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
                const int x = a.tp[base + k].x;
                atomicOr(bits + 2 * ((2 * j + 1) * W + (x >> 5)), 1u << (x & 31));
            }
        }
        __syncthreads();
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int r = wave; r < nrow; r += SC_THREADS / 64) {
            int2 *row = rows + r * W;
            int run = 0;
            for (int c = 0; c < W; c += 64) {
                const int i = c + lane;
                const int v = i < W ? __popc((unsigned)row[i].x) : 0;
                int incl = v;
                for (int d = 1; d < 64; d <<= 1) {
                    const int y = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += y;
                }
                if (i < W) row[i].y = run + incl - v;
                run += __shfl(incl, 63, 64);
            }
        }
    }
    __syncthreads();
    // A and X of one (z, y) on the ground set R: y's T positions [y.x, y.y), py's [y.z, y.w), yq = {|y ∩ Q'|, |py ∩ Q'|}
    const auto pair = [&](const int4 y, const int2 yq, int j, int4 z, int4 ci, unsigned long long &av,
                          unsigned long long &xv) {
        int cz, cp;
        if (!cp_masked(z, ci.x, ci.y, cz, cp)) return false;
        const int2 *rz = rows + 2 * j * W, *rp = rz + W;
        const int wa = y.x >> 5, wb = y.y >> 5;
        const unsigned ma = (1u << (y.x & 31)) - 1u, mb = (1u << (y.y & 31)) - 1u;
        const int iyz = tp_count(rz, wb, mb) - tp_count(rz, wa, ma) - (cz ? yq.x : 0);
        if (iyz == 0) return false;
        const int wc = y.z >> 5, wd = y.w >> 5;
        const unsigned mc = (1u << (y.z & 31)) - 1u, md = (1u << (y.w & 31)) - 1u;
        const int ipyz = tp_count(rz, wd, md) - tp_count(rz, wc, mc) - (cz ? yq.y : 0);
        const int ipp = tp_count(rp, wd, md) - tp_count(rp, wc, mc) - (cp ? yq.y : 0);
        const int nq = ci.y - ci.x;
        const int zr = (z.y - z.x) - (cz ? nq : 0), pr = (z.w - z.z) - (cp ? nq : 0);
        av = (unsigned long long)((int64_t)iyz * (iyz - 1) / 2);
        xv = (unsigned long long)((int64_t)iyz * ((pr - ipp) - (zr - ipyz)));
        return true;
    };
    if (a.lds_sums) {
        const int total = pref[qc];
        for (int e = threadIdx.x; e < total; e += SC_THREADS) {
            int i = 0, hi = qc;  // pref[i] <= e < pref[hi]
            while (hi - i > 1) {
                const int m = (i + hi) >> 1;
                if (pref[m] <= e) i = m; else hi = m;
            }
            const int64_t at = base * qc + (int64_t)i * n + (e - pref[i]);
            const int4 y = a.glist[at];
            const int2 yq = a.gq[at];
            const int c = qinfo[i].y;
            const int4 ci = cinfo[c];
            for (int j = 0; j < nz; ++j) {
                unsigned long long av, xv;
                if (!pair(y, yq, j, zs[2 * j], ci, av, xv)) continue;
                if (av) atomicAdd(sums + 2 * (j * qc + c), av);
                if (xv) atomicAdd(sums + 2 * (j * qc + c) + 1, xv);
            }
        }
        __syncthreads();
    } else {
        for (int i = 0; i < qc; ++i) {
            const int cnt = a.gcnt[(int64_t)t * qc + i];
            const int c = qinfo[i].y;
            const int4 ci = cinfo[c];
            for (int e = threadIdx.x; e < cnt; e += SC_THREADS) {
                const int64_t at = base * qc + (int64_t)i * n + e;
                const int4 y = a.glist[at];
                const int2 yq = a.gq[at];
                for (int j = 0; j < nz; ++j) {
                    unsigned long long av, xv;
                    if (!pair(y, yq, j, zlist[j], ci, av, xv)) continue;
                    pl_emit(a.sub + c * a.row_stride, a.strict + c * a.row_stride, zmeta[j], av, xv);
                }
            }
        }
    }
    // per (z, clade the tree crosses): the summed marks of the shared row; for a clade that begins in this pass the
    // closed-form marks of the super row, the same for every tip of Q': once, times |Q'|
    for (int it = threadIdx.x; it < nz * ncl; it += SC_THREADS) {
        const int j = it / ncl, c = it % ncl;
        const int4 ci = cinfo[c];
        if (!ci.z) continue;
        const int4 z = a.lds_sums ? zs[2 * j] : zlist[j], meta = a.lds_sums ? zs[2 * j + 1] : zmeta[j];
        if (a.lds_sums)
            pl_emit(a.sub + c * a.row_stride, a.strict + c * a.row_stride, meta, sums[2 * (j * qc + c)],
                    sums[2 * (j * qc + c) + 1]);
        if (c == 0 && a.skip0) continue;
        int cz, cp;
        if (!cp_masked(z, ci.x, ci.y, cz, cp)) continue;
        const int64_t nq = ci.y - ci.x;
        const int64_t sz = (z.y - z.x) - (cz ? nq : 0), spz = (z.w - z.z) - (cp ? nq : 0);
        pl_emit(a.sub + a.super_off + c * a.row_stride, a.strict + a.super_off + c * a.row_stride, meta,
                (unsigned long long)(nq * (sz * (sz - 1) / 2)), (unsigned long long)(nq * sz * (spz - sz)));
    }
}

// mark(u) = sub[u] + strict[parent u] on [u, end u) of the row's difference array (zeroed; n + 1 entries)
__global__ void __launch_bounds__(SC_THREADS) k_cp_marks(const unsigned long long *__restrict__ sub,
                                                         const unsigned long long *__restrict__ strict,
                                                         const int32_t *__restrict__ parent,
                                                         const int32_t *__restrict__ end, int64_t n, int64_t n_rows,
                                                         unsigned long long *__restrict__ diff) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n_rows) return;
    const int64_t r = idx / n, u = idx % n;
    const unsigned long long m = sub[idx] + (u ? strict[r * n + parent[u]] : 0ull);
    if (!m) return;
    atomicAdd(diff + r * (n + 1) + u, m);
    atomicAdd(diff + r * (n + 1) + end[u], 0ull - m);
}

// ---- scs_score_clade_moves: the rows of scs_score_clade_placements stay on the device and every
// row is reduced to the clade's own entry and its top_k best regraft targets.  One workgroup per query.  A candidate is
// a node v outside the preorder range [q, end q); its key is (d, v) with d = super[v] - 2 shared[v], signed.  Keys are
// unique, so pass j takes the smallest key above the winner of pass j - 1: a strided scan per thread, a wave-64 shuffle
// reduction of the pair and one LDS step across the waves.  The sentinel (INT64_MAX, INT32_MAX) is above every real
// key and marks "no candidate left".  The row is 16 bytes a node and is read top_k times (L2).
constexpr int MV_KMAX = 8;

__device__ __forceinline__ bool mv_less(long long d0, int v0, long long d1, int v1) {
    return d0 < d1 || (d0 == d1 && v0 < v1);
}

__global__ void __launch_bounds__(SC_THREADS) k_cp_best(const long long *__restrict__ shared,
                                                        const long long *__restrict__ super, int64_t n,
                                                        const int32_t *__restrict__ qnode,
                                                        const int32_t *__restrict__ end, int top_k,
                                                        int32_t *__restrict__ mv_node, long long *__restrict__ mv_super,
                                                        long long *__restrict__ mv_shared,
                                                        long long *__restrict__ own_super,
                                                        long long *__restrict__ own_shared) {
    __shared__ long long wd[SC_THREADS / 64];
    __shared__ int wv[SC_THREADS / 64];
    __shared__ long long bd;
    __shared__ int bv;
    const int64_t i = blockIdx.x;
    const long long *sh = shared + i * n, *su = super + i * n;
    const int q = qnode[i], qe = end[q];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        own_super[i] = su[q];
        own_shared[i] = sh[q];
    }
    long long pd = INT64_MIN;  // the winner of the pass before: below every key at first
    int pv = -1;
    for (int j = 0; j < top_k; ++j) {
        long long d = INT64_MAX;
        int v = INT32_MAX;
        for (int64_t u = threadIdx.x; u < n; u += SC_THREADS) {
            if (u >= q && u < qe) continue;
            const long long k = su[u] - 2 * sh[u];
            if (mv_less(pd, pv, k, (int)u) && mv_less(k, (int)u, d, v)) {
                d = k;
                v = (int)u;
            }
        }
        for (int s = 32; s >= 1; s >>= 1) {
            const long long od = __shfl_xor(d, s, 64);
            const int ov = __shfl_xor(v, s, 64);
            if (mv_less(od, ov, d, v)) {
                d = od;
                v = ov;
            }
        }
        if (lane == 0) {
            wd[wave] = d;
            wv[wave] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < SC_THREADS / 64; ++w)
                if (mv_less(wd[w], wv[w], d, v)) {
                    d = wd[w];
                    v = wv[w];
                }
            bd = d;
            bv = v;
            const bool found = v != INT32_MAX;
            mv_node[i * top_k + j] = found ? v : -1;
            mv_super[i * top_k + j] = found ? su[v] : 0;
            mv_shared[i * top_k + j] = found ? sh[v] : 0;
        }
        __syncthreads();
        pd = bd;
        pv = bv;
    }
}

// levels of a sparse table over n entries: 2^levels > n (the binary descent's widest step covers any stretch)
int sc_levels_host(int64_t n) {
    int l = 1;
    while (((int64_t)1 << l) <= n) ++l;
    return l;
}

int grid_of(int64_t n) { return (int)std::max<int64_t>((n + SC_THREADS - 1) / SC_THREADS, 1); }

size_t sc_up256(size_t b) { return (b + 255) / 256 * 256; }

bool sc_launched(hipError_t &e) {
    if (e == hipSuccess) e = hipGetLastError();
    return e == hipSuccess;
}

// what both exports share: the supertree's host layout, the batches and the device block with S's arrays, the rows and
// the per-batch tables of steps 1 - 2.  The caller's own arrays: extra_bytes once (d_extra) and extra_per_leaf /
// extra_per_tree bytes per leaf / tree of the largest batch (d_extra_batch: max_lb leaves, max_rows trees), both
// counted in the batch budget.
struct sc_call {
    const char *who = nullptr;
    int32_t n_taxa = 0, n_leaves = 0, M = 0;
    int64_t n_gaps = 0, row_stride = 0, max_lb = 0, max_rows = 0;
    size_t extra_bytes = 0, extra_batch_bytes = 0;
    int levels = 0;
    std::vector<int32_t> s_lo, s_hi, sub_end, s_pos, s_gap_node, bstart;
    std::vector<uint64_t> s_gap;
    void *block = nullptr;
    int32_t *d_spos = nullptr, *d_gnode = nullptr, *d_slo = nullptr, *d_shi = nullptr, *d_end = nullptr;
    int32_t *d_rows = nullptr, *d_sp = nullptr, *d_dep = nullptr, *d_node = nullptr, *d_amin = nullptr;
    uint64_t *d_stab = nullptr;
    int2 *d_mm = nullptr;
    unsigned *d_flag = nullptr;
    char *d_extra = nullptr, *d_extra_batch = nullptr;
};

// the batches of one call, for sc_begin and scs_debug_score_plan alike: rows (V per tree) + per-leaf arrays and tables
// (levels of the call's largest tree) + the caller's bytes per leaf and per tree; a batch ends before the tree that
// would take it past SC_BUDGET, or at max_batch_trees trees (> 0).  off[M + 1]; bstart gets the first tree of every
// batch and M
void sc_plan_batches(const int64_t *off, int32_t M, int64_t max_leaves, int64_t s_leaves, int32_t max_batch_trees,
                     uint64_t extra_per_leaf, uint64_t extra_per_tree, int &levels_out, int64_t &row_stride_out,
                     std::vector<int32_t> &bstart) {
    const int64_t row_stride = row_stride_out = scs_round_up(std::max<int64_t>(s_leaves, 1), SC_ROW_ALIGN);
    const int levels = levels_out = sc_levels_host(std::max<int64_t>(max_leaves, 1));
    const auto per_tree = [&](int32_t t) {
        const int64_t n = off[t + 1] - off[t];
        return (uint64_t)row_stride * 4 + (uint64_t)n * (4 * 3 + 8 * levels + 4 * (levels - 1) + extra_per_leaf) +
               extra_per_tree;
    };
    bstart.assign(1, 0);
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

// the largest tree among [t0, t1), and the words W of a bitset row over its T positions (one word per 32, one more
// than the last position needs: the pair kernels' rows)
int64_t sc_largest_tree(const int64_t *off, int32_t t0, int32_t t1) {
    int64_t nmax = 0;
    for (int32_t t = t0; t < t1; ++t) nmax = std::max(nmax, off[t + 1] - off[t]);
    return nmax;
}

int sc_row_words(const int64_t *off, int32_t t0, int32_t t1) { return (int)(sc_largest_tree(off, t0, t1) >> 5) + 1; }

// what differs between the pair kernels' plans
struct sc_pair_rule {
    int word_bytes;          // LDS bytes of one node's (record's) rows per word of a row
    int zmax;                // nodes per workgroup at most
    int aux_node, aux_pass;  // LDS bytes beside the rows, per node and per launch (0, 0: the kernel keeps none) ...
    int lds_cap;             // ... and what the rows and those bytes may take together
    size_t lds_floor;        // the least dynamic LDS of a launch
    bool leaves_too;         // a tree's workgroups: ceil(2 n / zb) for n >= 3 (S' has n leaves and at most n - 1 other
                             // nodes), else ceil((n - 2) / zb) (n - 2 bounds the non-root internal nodes)
};

// k_trip_pairs: two rows (cl(z), cl(pz)) of int2 a node; a launch asks for 32 bytes at least
const sc_pair_rule SC_TRIP_RULE = {16, TP_ZMAX, 0, 0, 0, 32, false};
// k_bt_pairs / k_rs_pairs: three rows a record; at least the 768 bytes of the workgroup's wave sums
const sc_pair_rule SC_BT_RULE = {BT_ROW_BYTES, BT_ZMAX, 0, 0, 0, (size_t)(SC_THREADS / 64) * BT_ZMAX * 3 * 8, false};

// k_pl_pairs / k_cp_pairs with qc queries in a pass keep sums in LDS beside the rows, where they fit: these bytes a
// node, and these a pass
constexpr int sc_pl_node_bytes(int qc) { return 16 * qc + 32; }
constexpr int sc_pl_pass_bytes(int qc) { return 4 * ((qc + 4) & ~3); }

// their plan with up to qcap queries in a pass: the rows of k_trip_pairs and those sums, under the caller's cap
sc_pair_rule sc_pl_rule(int qcap, int lds_cap) {
    return {16, TP_ZMAX, sc_pl_node_bytes(qcap), sc_pl_pass_bytes(qcap), lds_cap, 0, true};
}

// the plan per batch, for the exports and the debug entries alike: W words per bitset row (largest tree of the
// batch), zb nodes per workgroup -- as many as TP_LDS_BUDGET holds rows of, fewer while the bytes beside the rows
// take them past the cap; sums: those bytes fit (with zb = 1 they may not: the kernel then adds straight to memory);
// lds: the rows' bytes of a launch, at least the floor; blk: the first pair workgroup of every tree
struct sc_pair_plan {
    std::vector<int> words, zbs, sums;
    std::vector<size_t> lds;
    std::vector<int64_t> blk;
};

sc_pair_plan sc_plan_pairs(const int64_t *off, const std::vector<int32_t> &bstart, const sc_pair_rule &r) {
    const size_t n_batches = bstart.size() - 1;
    sc_pair_plan p;
    p.words.assign(n_batches, 0);
    p.zbs.assign(n_batches, 0);
    p.sums.assign(n_batches, 0);
    p.lds.assign(n_batches, 0);
    p.blk.assign((size_t)bstart.back() + 1, 0);
    for (size_t b = 0; b < n_batches; ++b) {
        p.words[b] = sc_row_words(off, bstart[b], bstart[b + 1]);
        const int rowb = r.word_bytes * p.words[b];
        int zb = (int)std::min<int64_t>(r.zmax, std::max<int64_t>(1, TP_LDS_BUDGET / rowb));
        if (r.aux_node) {
            while (zb > 1 && zb * (rowb + r.aux_node) + r.aux_pass > r.lds_cap) --zb;
            p.sums[b] = zb * (rowb + r.aux_node) + r.aux_pass <= r.lds_cap;
        }
        p.zbs[b] = zb;
        p.lds[b] = std::max<size_t>((size_t)zb * rowb, r.lds_floor);
        for (int32_t t = bstart[b]; t < bstart[b + 1]; ++t) {
            const int64_t n = off[t + 1] - off[t];
            const int64_t nodes = r.leaves_too ? (n >= 3 ? 2 * n : 0) : std::max<int64_t>(n - 2, 0);
            p.blk[t + 1] = p.blk[t] + (nodes + zb - 1) / zb;
        }
    }
    return p;
}

// the dynamic LDS of a k_pl_pairs / k_cp_pairs launch of batch b with qc queries in the pass
size_t sc_pl_lds(const sc_pair_plan &p, size_t b, int qc) {
    return p.lds[b] + (p.sums[b] ? (size_t)p.zbs[b] * sc_pl_node_bytes(qc) + sc_pl_pass_bytes(qc) : 0);
}

// the workspace bytes per leaf and per tree of a batch that scs_score_placements, the clade exports and
// scs_score_polytomies give sc_begin (they decide the batch split), for the exports and scs_debug_placement_plan
// alike: qcap queries (sub-queries) in a pass; totb boundaries of nq polytomies
struct sc_extras {
    uint64_t per_leaf, per_tree;
};
sc_extras sc_pl_extras(int qcap) { return {16 * (uint64_t)qcap + 64, 12 * (uint64_t)qcap + 8}; }
sc_extras sc_cp_extras(int qcap) { return {25 * (uint64_t)qcap + 64, 36 * (uint64_t)qcap + 8}; }
sc_extras sc_py_extras(size_t totb, size_t nq) { return {16, 4 + 4 * ((uint64_t)totb + nq)}; }

// A bump allocator over one block of a call's workspace: typed pointers, `step` bytes apart at least.  An export
// declares its d_extra arrays once, as a function of the carver, and runs it twice: over nothing for the size it asks
// sc_begin for, then over the block for the pointers.  d_extra_batch is carved with step 1 for max_lb leaves and
// max_rows trees: its arrays are packed, because the per-leaf and per-tree byte counts an export gives sc_begin are
// the contract -- they decide the batch split -- and the carver checks the export against them.  An array that does
// not fit gets the block's start, never an address past it, and sets `over`: the export then ends the call with an
// internal error (SC_BAD_LAYOUT) before it launches anything of its own.  That check is the one over d_extra_batch:
// over d_extra the second run is bounded by the size the first run gave, so it cannot fail while both runs are the
// same code, and the exports test it only because the pass is the same function
struct sc_carver {
    char *base = nullptr;
    size_t cap = SIZE_MAX, step = 256, at = 0;
    bool over = false;
    template <typename T>
    T *take(size_t n) {
        const size_t bytes = (n * sizeof(T) + step - 1) / step * step;
        over = over || bytes > cap - at;
        if (over) return (T *)base;
        at += bytes;
        return base ? (T *)(base + at - bytes) : nullptr;
    }
};

// batch b as the kernels see it, and for the host its first tree and its first leaf
struct sc_bview : sc_batch {
    int32_t t0;
    int64_t L0;
};

sc_bview sc_batch_of(const scs_tables *src, const sc_call &c, size_t b) {
    sc_bview v;
    v.t0 = c.bstart[b];
    v.nb = c.bstart[b + 1] - v.t0;
    v.L0 = src->h_tree_off[v.t0];
    v.Lb = src->h_tree_off[v.t0 + v.nb] - v.L0;
    v.off = src->d_tree_off + v.t0;
    v.sp = c.d_sp;
    v.dep = c.d_dep;
    v.node = c.d_node;
    v.mm = c.d_mm;
    v.adj = src->d_adj_depth + v.L0;
    v.amin = c.d_amin;
    v.levels = c.levels;
    v.s_tab = c.d_stab;
    v.s_stride = c.n_gaps;
    v.s_levels = sc_levels_host(c.n_gaps);
    v.s_lo = c.d_slo;
    v.s_hi = c.d_shi;
    return v;
}

// a kernel's argument struct over a batch view; its own members start as zero
template <typename A>
A sc_args(const sc_batch &v) {
    A a{};
    static_cast<sc_batch &>(a) = v;
    return a;
}

// checks, host layout, block, uploads (their errors in e); SCS_OK or the code of a failure before the block exists
int sc_begin(scs_ctx *ctx, const scs_tables *src, const char *who, int32_t n_nodes, const int32_t *parent,
             const int32_t *taxon, int32_t max_batch_trees, size_t extra_bytes, uint64_t extra_per_leaf,
             uint64_t extra_per_tree, sc_call &c, hipError_t &e) {
    c.who = who;
    SCS_REQUIRE(ctx && src && parent && taxon, "%s: null argument", who);
    SCS_REQUIRE(n_nodes >= 1, "%s: the supertree has no node", who);
    SCS_REQUIRE(parent[0] == -1, "%s: node 0 must be the root (parent -1)", who);
    const int32_t n_taxa = c.n_taxa = src->n_taxa;
    // ---- the supertree's preorder arrays on the host: leaf ranges, subtree ends, gap table (O(nodes)) ----
    std::vector<int32_t> &s_lo = c.s_lo, &s_hi = c.s_hi, &sub_end = c.sub_end;
    s_lo.resize(n_nodes);
    s_hi.resize(n_nodes);
    sub_end.resize(n_nodes);
    std::vector<int32_t> depth(n_nodes), n_kids(n_nodes, 0);
    for (int32_t v = 1; v < n_nodes; ++v) {
        SCS_REQUIRE(parent[v] >= 0 && parent[v] < v, "%s: parent[%d] = %d is not an earlier node", who, v, parent[v]);
        n_kids[parent[v]]++;
    }
    std::vector<int32_t> &s_pos = c.s_pos;
    s_pos.assign(std::max(n_taxa, 1), -1);
    int32_t n_leaves = 0;
    depth[0] = 0;
    for (int32_t v = 0; v < n_nodes; ++v) {
        if (v) depth[v] = depth[parent[v]] + 1;
        if (n_kids[v] == 0) {
            const int32_t x = taxon[v];
            SCS_REQUIRE(x >= 0, "%s: tip %d has no taxon", who, v);
            if (x < n_taxa) {
                SCS_REQUIRE(s_pos[x] < 0, "%s: taxon %d occurs twice in the supertree", who, x);
                s_pos[x] = n_leaves;
            }
            s_lo[v] = n_leaves;
            s_hi[v] = n_leaves;
            ++n_leaves;
        } else {
            SCS_REQUIRE(taxon[v] < 0, "%s: inner node %d carries a taxon", who, v);
            s_lo[v] = INT32_MAX;
            s_hi[v] = -1;
        }
        sub_end[v] = v + 1;
    }
    c.n_leaves = n_leaves;
    for (int32_t v = n_nodes - 1; v >= 1; --v) {  // (preorder: children after parents)
        const int32_t u = parent[v];
        s_lo[u] = std::min(s_lo[u], s_lo[v]);
        s_hi[u] = std::max(s_hi[u], s_hi[v]);
        sub_end[u] = std::max(sub_end[u], sub_end[v]);
    }
    // gap g (between S leaves g and g + 1) belongs to the node whose consecutive children it separates
    const int64_t n_gaps = c.n_gaps = std::max<int64_t>(n_leaves - 1, 1);
    c.s_gap.assign(n_gaps, 0);
    c.s_gap_node.assign(n_gaps, 0);
    for (int32_t v = 1; v < n_nodes; ++v) {
        const int32_t u = parent[v];
        if (s_hi[v] < s_hi[u]) {  // v is not u's last child
            const int32_t g = s_hi[v];
            c.s_gap[g] = ((uint64_t)depth[u] << 32) | (uint32_t)g;
            c.s_gap_node[g] = u;
        }
    }
    const int32_t M = c.M = src->n_trees;
    const std::vector<int64_t> &off = src->h_tree_off;
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    hipStream_t s = ctx->stream;

    // ---- batches: rows (V per tree) + per-leaf arrays and tables (levels of the batch's largest tree) ----
    std::vector<int32_t> &bstart = c.bstart;
    sc_plan_batches(off.data(), M, src->max_leaves, n_leaves, max_batch_trees, extra_per_leaf, extra_per_tree, c.levels,
                    c.row_stride, bstart);
    const int64_t row_stride = c.row_stride;
    const int levels = c.levels;
    int64_t max_rows = 0, max_lb = 0;
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        max_rows = std::max<int64_t>(max_rows, bstart[b + 1] - bstart[b]);
        max_lb = std::max<int64_t>(max_lb, off[bstart[b + 1]] - off[bstart[b]]);
    }
    c.max_lb = max_lb;
    c.max_rows = max_rows;
    c.extra_bytes = extra_bytes;
    c.extra_batch_bytes = (size_t)(max_lb * extra_per_leaf + max_rows * extra_per_tree);
    const int s_levels = sc_levels_host(n_gaps);
    const auto layout = [&](sc_carver w) {
        // persistent part: S arrays, flags, the caller's arrays
        c.d_spos = w.take<int32_t>((size_t)std::max(n_taxa, 1));
        c.d_gnode = w.take<int32_t>((size_t)n_gaps);
        c.d_stab = w.take<uint64_t>((size_t)n_gaps * s_levels);
        c.d_slo = w.take<int32_t>((size_t)n_nodes);
        c.d_shi = w.take<int32_t>((size_t)n_nodes);
        c.d_end = w.take<int32_t>((size_t)n_nodes);
        c.d_flag = w.take<unsigned>(1);
        c.d_extra = w.take<char>(extra_bytes);
        // batch part
        c.d_rows = w.take<int32_t>((size_t)max_rows * row_stride);
        c.d_sp = w.take<int32_t>((size_t)max_lb);
        c.d_dep = w.take<int32_t>((size_t)max_lb);
        c.d_node = w.take<int32_t>((size_t)max_lb);
        c.d_mm = w.take<int2>((size_t)max_lb * levels);
        c.d_amin = w.take<int32_t>((size_t)max_lb * std::max(levels - 1, 1));
        c.d_extra_batch = w.take<char>(c.extra_batch_bytes);
        return w.at;
    };
    const size_t bytes = layout(sc_carver());
    SCS_TRY(scs_block_alloc(ctx, bytes, &c.block));
    layout(sc_carver{(char *)c.block, bytes});

    e = hipMemcpyAsync(c.d_spos, s_pos.data(), (size_t)std::max(n_taxa, 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(c.d_gnode, c.s_gap_node.data(), (size_t)n_gaps * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(c.d_stab, c.s_gap.data(), (size_t)n_gaps * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(c.d_slo, s_lo.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(c.d_shi, s_hi.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(c.d_end, sub_end.data(), (size_t)n_nodes * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(c.d_flag, 0, 4, s);
    for (int j = 1; j < s_levels && e == hipSuccess; ++j) {
        k_score_level_u64<<<grid_of(n_gaps), SC_THREADS, 0, s>>>(c.d_stab + (j - 1) * n_gaps, c.d_stab + j * n_gaps,
                                                                 n_gaps, (int64_t)1 << (j - 1));
        sc_launched(e);
    }
    return SCS_OK;
}

// steps 1 - 2 for batch b: sp, the tp min-max table, T's min table of adj, D and U.  False (stop) on an error or on a
// bad source taxon (`bad`): a row left short must not be read
bool sc_prepare_batch(const scs_tables *src, hipStream_t s, sc_call &c, size_t b, hipError_t &e, unsigned &bad) {
    const sc_bview v = sc_batch_of(src, c, b);
    const int64_t *d_off = v.off, Lb = v.Lb;
    const int32_t nb = v.nb;
    e = hipMemsetAsync(c.d_rows, 0xff, (size_t)nb * c.row_stride * 4, s);
    if (e != hipSuccess) return false;
    k_score_scatter<<<grid_of(Lb), SC_THREADS, 0, s>>>(d_off, nb, src->d_leaf_taxon, c.n_taxa, c.d_spos, c.d_rows,
                                                       c.row_stride, c.d_flag);
    if (!sc_launched(e)) return false;
    e = hipMemcpyAsync(&bad, c.d_flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || bad) return false;
    k_score_compact<<<nb, SC_THREADS, 0, s>>>(d_off, c.d_rows, c.row_stride, c.d_sp, c.d_mm);
    if (!sc_launched(e)) return false;
    for (int j = 1; j < c.levels && e == hipSuccess; ++j) {
        k_score_level_tree<<<grid_of(Lb), SC_THREADS, 0, s>>>(j == 1 ? v.adj : c.d_amin + (int64_t)(j - 2) * Lb,
                                                               c.d_amin + (int64_t)(j - 1) * Lb, c.d_mm + (j - 1) * Lb,
                                                               c.d_mm + j * Lb, Lb, (int64_t)1 << (j - 1));
        sc_launched(e);
    }
    if (e != hipSuccess) return false;
    k_score_restrict<<<grid_of(Lb), SC_THREADS, 0, s>>>(d_off, nb, c.d_sp, c.d_stab, c.n_gaps, c.d_gnode, c.d_dep,
                                                        c.d_node);
    return sc_launched(e);
}

constexpr unsigned SC_BAD_LAYOUT = 16u;  // host only: an export carved more than it budgeted (the device flag has 1 - 8
                                         // and 32, SC_BAD_FRAMES of scs_score_parsimony.h)

// the call's sc_carver over d_extra (the bytes the export asked sc_begin for) ...
sc_carver sc_carve_extra(const sc_call &c) { return sc_carver{c.d_extra, c.extra_bytes}; }

// ... and over d_extra_batch: packed, for max_lb leaves and max_rows trees
sc_carver sc_carve_batch(const sc_call &c) { return sc_carver{c.d_extra_batch, c.extra_batch_bytes, 1}; }

// reads the device flag (it only gathers bits: `bad` is an earlier reading of it, or SC_BAD_LAYOUT), waits for the
// stream (after the caller's copies), releases the block, reports
int sc_end(scs_ctx *ctx, sc_call &c, hipError_t e, unsigned bad) {
    hipStream_t s = ctx->stream;
    unsigned flag = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, c.d_flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipStreamSynchronize(s);  // (nothing may still write into the block)
    scs_block_release(ctx, c.block);
    if (e != hipSuccess) {
        scs_set_error("%s: %s", c.who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCS_ENOMEM : SCS_EHIP;
    }
    bad |= flag;
    if (bad) {
        scs_set_error("%s: %s", c.who,
                      (bad & SC_BAD_LAYOUT) ? "internal: the export's arrays do not fit the bytes it budgeted for them"
                      : (bad & 32u)         ? "internal: a parsimony fold opened more frames than were planned"
                      : (bad & 8u)          ? "internal: a node was listed for a slab launch that is not made"
                      : (bad & 1u)          ? "a leaf_taxon entry is out of range [0, n_taxa)"
                      : (bad & 2u)          ? "a source tree has a taxon the supertree lacks"
                                            : "a source tree has a taxon twice");
        return SCS_EINVAL;
    }
    return SCS_OK;
}

// the tail of an export with k counters per tree (d_cnt [k][M]): they come down, sc_end, and row i goes to outs[i]
// where that is not null
int sc_end_counted(scs_ctx *ctx, sc_call &c, hipError_t e, unsigned bad, const unsigned long long *d_cnt, int k,
                   int64_t *const *outs) {
    const size_t M = (size_t)c.M;
    std::vector<unsigned long long> cnt(M * k);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, M * k * 8, hipMemcpyDeviceToHost, ctx->stream);
    SCS_TRY(sc_end(ctx, c, e, bad));
    for (int i = 0; i < k; ++i)
        for (size_t t = 0; t < M && outs[i]; ++t) outs[i][t] = (int64_t)cnt[i * M + t];
    return SCS_OK;
}

// k rows of n 64-bit entries each, from d on, come down into the outputs that are not null
void sc_fetch_rows(hipStream_t s, const void *d, size_t n, int k, int64_t *const *outs, hipError_t &e) {
    for (int i = 0; i < k && e == hipSuccess; ++i)
        if (outs[i] && n) e = hipMemcpyAsync(outs[i], (const char *)d + i * n * 8, n * 8, hipMemcpyDeviceToHost, s);
}

// the marks of the S nodes (two rows) become every node's sum over its subtree: d_pref two rows of n_nodes + 1 prefix
// sums, d_out the two rows of results
void sc_subtree_sums(hipStream_t s, const sc_call &c, int32_t n_nodes, const int32_t *d_mark, int64_t *d_pref,
                     int64_t *d_out, hipError_t &e, unsigned bad) {
    if (e == hipSuccess && !bad) {
        k_score_prefix<<<1, 1024, 0, s>>>(d_mark, d_mark + n_nodes, n_nodes, d_pref, d_pref + n_nodes + 1);
        sc_launched(e);
    }
    if (e == hipSuccess && !bad) {
        k_score_subtree<<<grid_of(n_nodes), SC_THREADS, 0, s>>>(d_pref, d_pref + n_nodes + 1, c.d_end, n_nodes, d_out,
                                                                d_out + n_nodes);
        sc_launched(e);
    }
}

int64_t sc_max_leaves(const scs_tables *src) { return src ? std::max<int64_t>(src->max_leaves, 0) : 0; }

// the LDS a workgroup may take: the caller's max_lds_bytes (0: no wish), TP_LDS_MAX at most
int sc_lds_cap(int32_t max_lds_bytes) {
    return max_lds_bytes > 0 ? std::min<int>(max_lds_bytes, TP_LDS_MAX) : TP_LDS_MAX;
}

// the rows of one node (row_bytes per word) of the largest tree must fit one workgroup's LDS -- and, where the caller
// names its wish, under that
int sc_rows_fit(const char *who, const scs_tables *src, int row_bytes, int32_t max_lds_bytes = 0) {
    const int64_t m_max = sc_max_leaves(src), need = row_bytes * ((m_max >> 5) + 1);
    if (max_lds_bytes > 0) {
        SCS_REQUIRE(need <= sc_lds_cap(max_lds_bytes),
                    "%s: max_lds_bytes = %d does not hold the rows of a source tree of %lld leaves", who,
                    max_lds_bytes, (long long)m_max);
        return SCS_OK;
    }
    SCS_REQUIRE(need <= TP_LDS_MAX,
                "%s: a source tree of %lld leaves is more than the %d the pair kernel holds in LDS", who,
                (long long)m_max, TP_LDS_MAX / row_bytes * 32 - 1);
    return SCS_OK;
}

// a sum over nodes of triples is at most sum_t (m_t / 3)^3: it must fit int64
int sc_cubes_fit(const char *who, const scs_tables *src) {
    if (!src) return SCS_OK;
    unsigned __int128 cubes = 0;
    for (int32_t t = 0; t < src->n_trees; ++t) {
        const unsigned __int128 m = (unsigned __int128)(src->h_tree_off[t + 1] - src->h_tree_off[t]);
        cubes += m * m * m;
    }
    SCS_REQUIRE(cubes / 27 <= (unsigned __int128)INT64_MAX,
                "%s: the triple counts of %d source trees may not fit 64 bits", who, src->n_trees);
    return SCS_OK;
}

// quartet branches: two children, below a parent of two children -- their parent, -1 for every other node (sc_begin
// has checked `parent`)
std::vector<int32_t> sc_quartet_parents(int32_t n_nodes, const int32_t *parent) {
    const size_t nn = (size_t)std::max(n_nodes, 0);
    std::vector<int32_t> n_kids(nn, 0), q_parent(nn, -1);
    for (int32_t v = 1; v < n_nodes; ++v) n_kids[parent[v]]++;
    for (int32_t v = 1; v < n_nodes; ++v)
        if (n_kids[v] == 2 && n_kids[parent[v]] == 2) q_parent[v] = parent[v];
    return q_parent;
}

// The supertree as an export needs it for its own refusals, before sc_begin has checked it: every node's children,
// depth and -- with `ranges` -- leaf range (tips counted in preorder), the tips' nodes and depths by leaf position.  A
// parent entry that is not an earlier node is passed over, not refused: sc_begin refuses it afterwards, and the
// export's own refusals come first
struct sc_walk {
    std::vector<int32_t> n_kids, depth, lo, hi, tip_node, tip_depth;
};

sc_walk sc_walk_super(int32_t n_nodes, const int32_t *parent, bool ranges) {
    sc_walk w;
    w.n_kids.assign((size_t)n_nodes, 0);
    w.depth.assign((size_t)n_nodes, 0);
    if (ranges) {
        w.lo.assign((size_t)n_nodes, INT32_MAX);
        w.hi.assign((size_t)n_nodes, -1);
    }
    const auto linked = [&](int32_t v) { return parent[v] >= 0 && parent[v] < v; };
    for (int32_t v = 1; v < n_nodes; ++v)
        if (linked(v)) {
            w.n_kids[parent[v]]++;
            w.depth[v] = w.depth[parent[v]] + 1;
        }
    for (int32_t v = 0; v < n_nodes; ++v)
        if (!w.n_kids[v]) {
            if (ranges) w.lo[v] = w.hi[v] = (int32_t)w.tip_node.size();
            w.tip_node.push_back(v);
            w.tip_depth.push_back(w.depth[v]);
        }
    for (int32_t v = n_nodes - 1; v >= 1 && ranges; --v)
        if (linked(v)) {
            w.lo[parent[v]] = std::min(w.lo[parent[v]], w.lo[v]);
            w.hi[parent[v]] = std::max(w.hi[parent[v]], w.hi[v]);
        }
    return w;
}

// what the two debug plan entries share: off (the tables' or the caller's) with its largest tree, and the batches by
// sc_plan_batches
struct sc_debug_plan {
    const int64_t *off = nullptr;
    int64_t max_leaves = 0, row_stride = 0;
    int levels = 0;
    std::vector<int32_t> bstart;
};

// ... after their checks (outs_given: the entry's own outputs are there); the batches are written out as well
int sc_debug_batches(const char *who, const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                     int32_t super_leaves, int32_t max_batch_trees, int64_t extra_per_leaf, int64_t extra_per_tree,
                     int32_t max_lds_bytes, bool outs_given, int32_t *n_batches_out, int32_t *bstart_out,
                     sc_debug_plan &d) {
    SCS_REQUIRE((src || tree_off) && n_batches_out && bstart_out && outs_given, "%s: null argument", who);
    SCS_REQUIRE(!src || n_trees == src->n_trees, "%s: the tables hold %d trees, not %d", who, src ? src->n_trees : 0,
                n_trees);
    SCS_REQUIRE(n_trees >= 0 && super_leaves >= 0 && extra_per_leaf >= 0 && extra_per_tree >= 0 && max_lds_bytes >= 0,
                "%s: negative argument", who);
    d.off = src ? src->h_tree_off.data() : tree_off;
    d.max_leaves = src ? src->max_leaves : 0;
    if (!src)
        for (int32_t t = 0; t < n_trees; ++t) {
            SCS_REQUIRE(d.off[t + 1] >= d.off[t], "%s: tree_off decreases at tree %d", who, t);
            d.max_leaves = std::max(d.max_leaves, d.off[t + 1] - d.off[t]);
        }
    sc_plan_batches(d.off, n_trees, d.max_leaves, super_leaves, max_batch_trees, (uint64_t)extra_per_leaf,
                    (uint64_t)extra_per_tree, d.levels, d.row_stride, d.bstart);
    *n_batches_out = (int32_t)d.bstart.size() - 1;
    std::copy(d.bstart.begin(), d.bstart.end(), bstart_out);
    return SCS_OK;
}

}  // namespace

extern "C" int scs_score_supertree(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                   const int32_t *taxon, int32_t max_batch_trees, int64_t *n_super,
                                   int64_t *n_source, int64_t *shared, int64_t *informative, int64_t *supported) {
    // own arrays: marks, prefix sums, outputs per S node (two rows each); three counters per tree
    const size_t nn = (size_t)std::max(n_nodes, 0), mt = src ? (size_t)src->n_trees : 0;
    int32_t *d_mark;
    int64_t *d_pref, *d_out;
    unsigned long long *d_cnt;
    const auto own = [&](sc_carver w) {
        d_mark = w.take<int32_t>(2 * nn);
        d_pref = w.take<int64_t>(2 * (nn + 1));
        d_out = w.take<int64_t>(2 * nn);
        d_cnt = w.take<unsigned long long>(3 * mt);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_supertree", n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at, 0,
                     0, c, e));
    if (own(sc_carve_extra(c)).over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_mark, 0, nn * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 24, s);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        auto a = sc_args<sc_nodes_args>(v);
        a.mark_inf = d_mark;
        a.mark_sup = d_mark + n_nodes;
        a.c_super = d_cnt + v.t0;
        a.c_source = d_cnt + M + v.t0;
        a.c_shared = d_cnt + 2 * (int64_t)M + v.t0;
        k_score_nodes<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
    }
    sc_subtree_sums(s, c, n_nodes, d_mark, d_pref, d_out, e, bad);
    int64_t *const node_outs[2] = {informative, supported};
    sc_fetch_rows(s, d_out, nn, 2, node_outs, e);
    int64_t *const outs[3] = {n_super, n_source, shared};
    SCS_TRY(sc_end_counted(ctx, c, e, bad, d_cnt, 3, outs));
    // n_source is the kernel's count less one for a tree of two leaves or more, 0 for the others
    const std::vector<int64_t> &off = src->h_tree_off;
    for (int32_t t = 0; t < M && n_source; ++t) n_source[t] = off[t + 1] - off[t] >= 2 ? n_source[t] - 1 : 0;
    return SCS_OK;
}

extern "C" int scs_score_triplets(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                  const int32_t *taxon, int32_t max_batch_trees, int64_t *t_super, int64_t *t_source,
                                  int64_t *t_shared) {
    // a row pair (cl(z), cl(pz)) of the largest tree must fit one workgroup's LDS
    SCS_TRY(sc_rows_fit("scs_score_triplets", src, 16));
    // own arrays: three counters and the first pair workgroup per tree (+ 1); per batch two node lists (int4 per
    // leaf) and their two lengths per tree
    const size_t mt = src ? (size_t)src->n_trees : 0;
    unsigned long long *d_cnt;
    int64_t *d_blk;
    const auto own = [&](sc_carver w) {
        d_cnt = w.take<unsigned long long>(3 * mt);
        d_blk = w.take<int64_t>(mt + 1);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_triplets", n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at, 32,
                     8, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_ylist = wb.take<int4>(c.max_lb);
    auto *d_zlist = wb.take<int4>(c.max_lb);
    auto *d_ycnt = wb.take<int32_t>(2 * c.max_rows);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    // per batch: W words per bitset row, zb S' nodes per workgroup; blk: the first pair workgroup of every tree
    const sc_pair_plan pl = sc_plan_pairs(src->h_tree_off.data(), c.bstart, SC_TRIP_RULE);
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 24, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk, pl.blk.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_trip_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        e = hipMemsetAsync(d_ycnt, 0, (size_t)nb * 8, s);
        if (e != hipSuccess) break;
        auto a = sc_args<sc_trip_args>(v);
        a.ylist = d_ylist;
        a.zlist = d_zlist;
        a.ycnt = d_ycnt;
        a.zcnt = d_ycnt + nb;
        a.c_super = d_cnt + t0;
        a.c_source = d_cnt + M + t0;
        k_trip_nodes<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        const int64_t n_wg = pl.blk[t0 + nb] - pl.blk[t0];
        if (n_wg == 0) continue;
        k_trip_pairs<<<(unsigned)n_wg, SC_THREADS, pl.lds[b], s>>>(d_blk + t0, nb, a.off, d_ylist, d_zlist, a.ycnt,
                                                                   a.zcnt, c.d_mm, pl.zbs[b], pl.words[b],
                                                                   d_cnt + 2 * (int64_t)M + t0);
        if (!sc_launched(e)) break;
    }
    int64_t *const outs[3] = {t_super, t_source, t_shared};
    return sc_end_counted(ctx, c, e, bad, d_cnt, 3, outs);
}

// the plan of one scoring call on the host: what sc_begin and scs_score_triplets decide, by their own functions
extern "C" int scs_debug_score_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                    int32_t super_leaves, int32_t max_batch_trees, int64_t extra_per_leaf,
                                    int64_t extra_per_tree, int32_t *n_batches_out, int32_t *bstart_out,
                                    int64_t *info_out, int32_t *words_out, int32_t *zb_out, int64_t *wg_out) {
    sc_debug_plan d;
    SCS_TRY(sc_debug_batches("scs_debug_score_plan", src, n_trees, tree_off, super_leaves, max_batch_trees,
                             extra_per_leaf, extra_per_tree, 0, info_out && words_out && zb_out && wg_out,
                             n_batches_out, bstart_out, d));
    const std::vector<int32_t> &bstart = d.bstart;
    const sc_pair_plan pl = sc_plan_pairs(d.off, bstart, SC_TRIP_RULE);
    info_out[0] = d.levels;
    info_out[1] = d.row_stride;
    for (size_t b = 0; b + 1 < bstart.size(); ++b) {
        words_out[b] = pl.words[b];
        zb_out[b] = pl.zbs[b];
        wg_out[b] = pl.blk[bstart[b + 1]] - pl.blk[bstart[b]];
    }
    return SCS_OK;
}

extern "C" int scs_score_conflicts(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                   const int32_t *taxon, int32_t max_batch_trees, int64_t *n_super_conflict,
                                   int64_t *n_source_conflict, int64_t *conflicting) {
    // own arrays: marks (two rows: k_score_prefix sums two; the second stays 0), prefix sums and outputs per S node,
    // two counters per tree; per batch leaf ip's min-max table (the levels sc_begin gives the batch) and two mark rows
    const size_t nn = (size_t)std::max(n_nodes, 0), mt = src ? (size_t)src->n_trees : 0;
    const int levels = sc_levels_host(std::max<int64_t>(src ? src->max_leaves : 1, 1));
    int32_t *d_mark;
    int64_t *d_pref, *d_out;
    unsigned long long *d_cnt;
    const auto own = [&](sc_carver w) {
        d_mark = w.take<int32_t>(2 * nn);
        d_pref = w.take<int64_t>(2 * (nn + 1));
        d_out = w.take<int64_t>(2 * nn);
        d_cnt = w.take<unsigned long long>(2 * mt);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_conflicts", n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     8 * (uint64_t)levels + 8, 0, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_im = wb.take<int2>((size_t)c.levels * c.max_lb);
    auto *d_ms = wb.take<int32_t>(2 * c.max_lb);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_mark, 0, nn * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 16, s);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int64_t Lb = v.Lb;
        int32_t *d_mt = d_ms + Lb;
        e = hipMemsetAsync(d_ms, 0, (size_t)Lb * 8, s);
        if (e != hipSuccess) break;
        k_conf_ip<<<grid_of(Lb), SC_THREADS, 0, s>>>(v.off, v.nb, c.d_mm, d_im);
        if (!sc_launched(e)) break;
        for (int j = 1; j < c.levels && e == hipSuccess; ++j) {
            k_conf_level<<<grid_of(Lb), SC_THREADS, 0, s>>>(d_im + (j - 1) * Lb, d_im + j * Lb, Lb,
                                                            (int64_t)1 << (j - 1));
            sc_launched(e);
        }
        if (e != hipSuccess) break;
        auto a = sc_args<sc_conf_args>(v);
        a.im = d_im;
        a.mark_s = d_ms;
        a.mark_t = d_mt;
        a.mark_node = d_mark;
        a.c_super = d_cnt + v.t0;
        a.c_source = d_cnt + M + v.t0;
        k_conf_marks<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        k_conf_scan<<<v.nb, SC_THREADS, 0, s>>>(v.off, d_ms, d_mt);
        if (!sc_launched(e)) break;
        k_conf_nodes<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
    }
    sc_subtree_sums(s, c, n_nodes, d_mark, d_pref, d_out, e, bad);
    sc_fetch_rows(s, d_out, nn, 1, &conflicting, e);
    int64_t *const outs[2] = {n_super_conflict, n_source_conflict};
    return sc_end_counted(ctx, c, e, bad, d_cnt, 2, outs);
}

extern "C" int scs_score_concordance(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                     const int32_t *taxon, int32_t max_batch_trees, int64_t *n_decisive,
                                     int64_t *n_concordant, int64_t *n_alternative, int64_t *decisive,
                                     int64_t *concordant, int64_t *alt1, int64_t *alt2) {
    // own arrays: four counters and the quartet-branch record per S node, three counters per tree; nothing per leaf
    const size_t nn = (size_t)std::max(n_nodes, 0), mt = src ? (size_t)src->n_trees : 0;
    unsigned long long *d_node, *d_cnt;
    int32_t *d_qp;
    const auto own = [&](sc_carver w) {
        d_node = w.take<unsigned long long>(4 * nn);
        d_qp = w.take<int32_t>(nn);
        d_cnt = w.take<unsigned long long>(3 * mt);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_concordance", n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     0, 0, c, e));
    if (own(sc_carve_extra(c)).over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    const std::vector<int32_t> q_parent = sc_quartet_parents(n_nodes, parent);
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(d_qp, q_parent.data(), nn * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_node, 0, nn * 32, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 24, s);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        sc_conc_args a;
        a.off = v.off;
        a.nb = v.nb;
        a.sp = v.sp;
        a.node = v.node;
        a.mm = v.mm;
        a.adj = v.adj;
        a.amin = v.amin;
        a.Lb = v.Lb;
        a.s_lo = v.s_lo;
        a.s_hi = v.s_hi;
        a.q_parent = d_qp;
        a.n_dec = d_node;
        a.n_con = d_node + nn;
        a.n_alt1 = d_node + 2 * nn;
        a.n_alt2 = d_node + 3 * nn;
        a.c_dec = d_cnt + v.t0;
        a.c_con = d_cnt + M + v.t0;
        a.c_alt = d_cnt + 2 * (int64_t)M + v.t0;
        k_conc_branches<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
    }
    int64_t *const node_outs[4] = {decisive, concordant, alt1, alt2};
    sc_fetch_rows(s, d_node, nn, 4, node_outs, e);
    int64_t *const outs[3] = {n_decisive, n_concordant, n_alternative};
    return sc_end_counted(ctx, c, e, bad, d_cnt, 3, outs);
}

extern "C" int scs_score_branch_triplets(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                         const int32_t *taxon, int32_t max_batch_trees, int64_t *n_bt_total,
                                         int64_t *n_bt_concordant, int64_t *n_bt_alternative, int64_t *bt_total,
                                         int64_t *bt_concordant, int64_t *bt_alt1, int64_t *bt_alt2) {
    // the three rows of one record of the largest tree must fit one workgroup's LDS, and a node's sum int64
    SCS_TRY(sc_rows_fit("scs_score_branch_triplets", src, BT_ROW_BYTES));
    SCS_TRY(sc_cubes_fit("scs_score_branch_triplets", src));
    // own arrays: four counters and the quartet-branch record per S node, three counters and the first pair workgroup
    // per tree (+ 1); per batch T's node list (int4) and the record list per leaf, their two lengths per tree
    const size_t nn = (size_t)std::max(n_nodes, 0), mt = src ? (size_t)src->n_trees : 0;
    unsigned long long *d_node, *d_cnt;
    int32_t *d_qp;
    int64_t *d_blk;
    const auto own = [&](sc_carver w) {
        d_node = w.take<unsigned long long>(4 * nn);
        d_qp = w.take<int32_t>(nn);
        d_cnt = w.take<unsigned long long>(3 * mt);
        d_blk = w.take<int64_t>(mt + 1);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_branch_triplets", n_nodes, parent, taxon, max_batch_trees,
                     own(sc_carver()).at, 16 + sizeof(sc_bt_rec), 8, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_ylist = wb.take<int4>(c.max_lb);
    auto *d_recs = wb.take<sc_bt_rec>(c.max_lb);
    auto *d_ycnt = wb.take<int32_t>(2 * c.max_rows);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    const std::vector<int32_t> q_parent = sc_quartet_parents(n_nodes, parent);
    // per batch: W words per bitset row, zb records per workgroup and the launch's LDS; blk: the first pair workgroup
    // of every tree
    const sc_pair_plan pl = sc_plan_pairs(src->h_tree_off.data(), c.bstart, SC_BT_RULE);
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(d_qp, q_parent.data(), nn * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_node, 0, nn * 32, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 24, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk, pl.blk.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_bt_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        e = hipMemsetAsync(d_ycnt, 0, (size_t)nb * 8, s);
        if (e != hipSuccess) break;
        auto a = sc_args<sc_bt_args>(v);
        a.q_parent = d_qp;
        a.ylist = d_ylist;
        a.recs = d_recs;
        a.ycnt = d_ycnt;
        a.rcnt = d_ycnt + nb;
        a.n_tot = d_node;
        a.c_tot = d_cnt + t0;
        a.nn = (int64_t)nn;
        k_bt_records<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        const int64_t n_wg = pl.blk[t0 + nb] - pl.blk[t0];
        if (n_wg == 0) continue;
        k_bt_pairs<<<(unsigned)n_wg, SC_THREADS, pl.lds[b], s>>>(d_blk + t0, nb, a.off, d_ylist, d_recs, a.ycnt,
                                                                 a.rcnt, c.d_mm, pl.zbs[b], pl.words[b], d_node + nn,
                                                                 (int64_t)nn, d_cnt + M + t0,
                                                                 d_cnt + 2 * (int64_t)M + t0);
        if (!sc_launched(e)) break;
    }
    int64_t *const node_outs[4] = {bt_total, bt_concordant, bt_alt1, bt_alt2};
    sc_fetch_rows(s, d_node, nn, 4, node_outs, e);
    int64_t *const outs[3] = {n_bt_total, n_bt_concordant, n_bt_alternative};
    return sc_end_counted(ctx, c, e, bad, d_cnt, 3, outs);
}

namespace {

// the LDS bins of a batch whose rows have W words: nodes per workgroup, entries per node and launch bytes of each
struct sc_tx_plan {
    int zb[TX_BINS], lds[TX_BINS];
    sc_tx_bins bins;
    int dcap_max;
};

sc_tx_plan sc_tx_plan_of(int W, int lds_cap) {
    sc_tx_plan p;
    p.dcap_max = 0;
    const int rowb = 16 * W;  // cl(z) and cl(pz)
    for (int i = 0; i < TX_BINS; ++i) {
        // (bin 0 grows with the rows, so that eight nodes keep TX_SMALL entries each, up to the budget of bin 1)
        const int base = i == 0 ? std::min(TX_BIN_BUDGET[1], std::max(TX_BIN_BUDGET[0],
                                                                      TX_SCRATCH + TP_ZMAX * (rowb + 8 * TX_SMALL)))
                                : TX_BIN_BUDGET[i];
        const int budget = std::min(base, lds_cap);
        // at most half of the budget for rows, the rest for the arrays: no more than the 2 n + 1 entries a node of
        // the batch can need, at least the 7 of the smallest node
        const int zb = std::min(TX_BIN_ZMAX[i], std::max(1, budget / (2 * rowb)));
        const int avail = budget - TX_SCRATCH - zb * rowb;
        const int dcap = avail > 0 ? std::min(avail / (8 * zb), 64 * W) : 0;
        p.zb[i] = zb;
        p.bins.dcap[i] = dcap >= 7 && dcap > p.dcap_max ? dcap : 0;  // (no larger than an earlier bin: never chosen)
        p.lds[i] = TX_SCRATCH + zb * (rowb + 8 * dcap);
        p.dcap_max = std::max(p.dcap_max, p.bins.dcap[i]);
    }
    return p;
}

// what a call decides once, for scs_score_taxon_triplets and scs_debug_branch_plan alike: the LDS cap, and the slab
// path -- needed when a node's arrays (at most 2 m + 1 entries) may exceed the largest bin of the largest tree
struct sc_tx_call {
    int lds_cap = 0, slab_wgs = 0;
    int64_t slab_stride = 0;
    bool need_slab = false;
};

sc_tx_call sc_tx_call_of(int64_t m_max, int32_t max_lds_bytes) {
    sc_tx_call tc;
    tc.lds_cap = sc_lds_cap(max_lds_bytes);
    tc.slab_stride = 2 * m_max + 2 + TX_SLAB_PAD;
    tc.need_slab = 2 * m_max + 1 > sc_tx_plan_of((int)(m_max >> 5) + 1, tc.lds_cap).dcap_max;
    tc.slab_wgs = !tc.need_slab ? 0
                                : (int)std::min<uint64_t>(TX_SLAB_WGS,
                                                          std::max<uint64_t>(1, TX_SLAB_BYTES / (tc.slab_stride * 8)));
    return tc;
}

// the slab kernel's dynamic LDS: the two rows of its one node
size_t sc_tx_slab_lds(int W) { return (size_t)16 * W; }

// ... and per batch: W words per bitset row (largest tree of the batch), the plan of its bins and whether the slab
// kernel is launched; blk[TX_BINS][M + 1]: per bin the first pair workgroup of every tree, ceil((n - 2) / zb) of them
// (n - 2 bounds the nodes of any list)
void sc_tx_batches(const int64_t *off, const std::vector<int32_t> &bstart, const sc_tx_call &tc,
                   std::vector<int> &words, std::vector<sc_tx_plan> &plans, std::vector<char> &slab_launch,
                   std::vector<int64_t> &blk) {
    const size_t n_batches = bstart.size() - 1;
    const int32_t M = bstart.back();
    words.assign(n_batches, 0);
    plans.resize(n_batches);
    slab_launch.assign(n_batches, 0);
    blk.assign(((size_t)M + 1) * TX_BINS, 0);
    for (size_t b = 0; b < n_batches; ++b) {
        words[b] = sc_row_words(off, bstart[b], bstart[b + 1]);
        plans[b] = sc_tx_plan_of(words[b], tc.lds_cap);
        slab_launch[b] = tc.slab_wgs > 0 && 2 * ((int64_t)words[b] * 32) > plans[b].dcap_max;
        for (int i = 0; i < TX_BINS; ++i) {
            int64_t *bl = blk.data() + (size_t)i * (M + 1);
            for (int32_t t = bstart[b]; t < bstart[b + 1]; ++t)
                bl[t + 1] = bl[t] + (std::max<int64_t>(off[t + 1] - off[t] - 2, 0) + plans[b].zb[i] - 1) / plans[b].zb[i];
        }
    }
}

}  // namespace

extern "C" int scs_score_taxon_triplets(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                        const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                                        int64_t *tx_trees, int64_t *tx_total, int64_t *tx_super, int64_t *tx_source,
                                        int64_t *tx_shared) {
    // a row pair (cl(z), cl(pz)) of the largest tree must fit one workgroup's LDS, as for scs_score_triplets; every
    // count of one tree is then below m^3 < 2^63
    SCS_TRY(sc_rows_fit("scs_score_taxon_triplets", src, 16));
    SCS_REQUIRE(max_lds_bytes >= 0, "scs_score_taxon_triplets: max_lds_bytes = %d is negative", max_lds_bytes);
    // the outputs have one entry per supertree tip: the tips' taxon ids must be below their number.  (Not
    // sc_walk_super: this export has always taken any parent entry in range for a link here, and what it refuses for
    // an array sc_begin would refuse later follows from that)
    int64_t n_out = 0;
    if (parent && taxon && n_nodes >= 1) {
        std::vector<char> has_kid((size_t)n_nodes, 0);
        for (int32_t v = 1; v < n_nodes; ++v)
            if (parent[v] >= 0 && parent[v] < n_nodes) has_kid[parent[v]] = 1;
        for (int32_t v = 0; v < n_nodes; ++v) n_out += !has_kid[v];
        for (int32_t v = 0; v < n_nodes; ++v)
            SCS_REQUIRE(has_kid[v] || taxon[v] < n_out,
                        "scs_score_taxon_triplets: tip %d has taxon %d, not below the %lld tips of the supertree", v,
                        taxon[v], (long long)n_out);
    }
    // the LDS cap and the slab path
    const sc_tx_call tc = sc_tx_call_of(sc_max_leaves(src), max_lds_bytes);
    const int64_t slab_stride = tc.slab_stride;
    const int slab_wgs = tc.slab_wgs;
    // own arrays: the five outputs per taxon, the first pair workgroup per tree (+ 1) and bin, the slabs; per batch
    // the two node lists (int4), three sums (shared and source in T order, super in S' order) and the TX_BINS + 1
    // bin lists per leaf, and per tree the lengths of all those lists
    const size_t mt = src ? (size_t)src->n_trees : 0;
    unsigned long long *d_tx, *d_slab;
    int64_t *d_blk;
    const auto own = [&](sc_carver w) {
        d_tx = w.take<unsigned long long>(5 * (size_t)n_out);
        d_blk = w.take<int64_t>((mt + 1) * TX_BINS);
        d_slab = w.take<unsigned long long>((size_t)slab_wgs * slab_stride);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, "scs_score_taxon_triplets", n_nodes, parent, taxon, max_batch_trees,
                     own(sc_carver()).at, 32 + 24 + 4 * (TX_BINS + 1), 8 + 4 * (TX_BINS + 1), c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_ylist = wb.take<int4>(c.max_lb);
    auto *d_zlist = wb.take<int4>(c.max_lb);
    auto *d_acc = wb.take<unsigned long long>(c.max_lb);
    auto *d_dsrc = wb.take<unsigned long long>(c.max_lb);
    auto *d_dsup = wb.take<unsigned long long>(c.max_lb);
    auto *d_zbin = wb.take<int32_t>((TX_BINS + 1) * c.max_lb);
    auto *d_ycnt = wb.take<int32_t>((2 + TX_BINS + 1) * c.max_rows);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    // per batch: W words per bitset row, the plan of its bins and whether the slab kernel runs; blk: per bin the first
    // pair workgroup of every tree
    std::vector<int> words;
    std::vector<sc_tx_plan> plans;
    std::vector<char> slab_launches;
    std::vector<int64_t> blk;
    sc_tx_batches(src->h_tree_off.data(), c.bstart, tc, words, plans, slab_launches, blk);
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_tx, 0, (size_t)n_out * 40, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_blk, blk.data(), blk.size() * 8, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_tx_pairs<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                TP_LDS_MAX);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_tx_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        const int64_t Lb = v.Lb;
        e = hipMemsetAsync(d_ycnt, 0, (size_t)nb * (8 + 4 * (TX_BINS + 1)), s);
        if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, (size_t)c.max_lb * 8, s);
        if (e != hipSuccess) break;
        auto a = sc_args<sc_trip_args>(v);
        a.ylist = d_ylist;
        a.zlist = d_zlist;
        a.ycnt = d_ycnt;
        a.zcnt = d_ycnt + nb;
        // k_trip_nodes' own per-tree sums are not wanted here.  They are added at [t], t < nb, of the two rows given
        // below; a tree has a leaf, so nb <= Lb <= max_lb and the entries lie inside the rows, and the memset after
        // the launch clears both rows (they are adjacent) before k_tx_single writes its marks
        a.c_super = d_dsrc;
        a.c_source = d_dsup;
        k_trip_nodes<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        e = hipMemsetAsync(d_dsrc, 0, (size_t)c.max_lb * 16, s);
        if (e != hipSuccess) break;
        int32_t *d_zbcnt = d_ycnt + 2 * nb;
        const sc_tx_plan &pl = plans[b];
        const bool slab_launch = slab_launches[b] != 0;
        k_tx_single<<<grid_of(Lb), SC_THREADS, 0, s>>>(a.off, nb, d_ylist, d_zlist, a.ycnt, a.zcnt, pl.bins, Lb, d_zbin,
                                                       d_zbcnt, d_dsrc, d_dsup, slab_launch, c.d_flag);
        if (!sc_launched(e)) break;
        for (int i = 0; i < TX_BINS; ++i) {
            const int64_t *bl = blk.data() + (size_t)i * (M + 1);
            const int64_t n_wg = bl[t0 + nb] - bl[t0];
            if (pl.bins.dcap[i] == 0 || n_wg == 0) continue;
            k_tx_pairs<false><<<(unsigned)n_wg, SC_THREADS, (size_t)pl.lds[i], s>>>(
                d_blk + (size_t)i * (M + 1) + t0, nb, a.off, d_ylist, d_zlist, a.ycnt, d_zbin + (int64_t)i * Lb,
                d_zbcnt + (int64_t)i * nb, c.d_mm, pl.zb[i], words[b], nullptr, 0, d_acc);
            if (!sc_launched(e)) break;
        }
        if (e != hipSuccess) break;
        // k_tx_single lists a node for the slab iff its |z| + |pz| + 2 > pl.dcap_max.  That is at most 2 n + 1 < 64 W,
        // and dcap_max only grows when W shrinks (bin 2 holds one node: (cap - 64 - 16 W) / 8, capped by 64 W), so a
        // batch lists such a node only if need_slab held for m_max, that is only if the slabs exist
        if (slab_launch) {
            k_tx_pairs<true><<<(unsigned)slab_wgs, SC_THREADS, sc_tx_slab_lds(words[b]), s>>>(
                nullptr, nb, a.off, d_ylist, d_zlist, a.ycnt, d_zbin + (int64_t)TX_BINS * Lb,
                d_zbcnt + (int64_t)TX_BINS * nb, c.d_mm, 1, words[b], d_slab, slab_stride, d_acc);
            if (!sc_launched(e)) break;
        }
        k_tx_scan<<<nb, SC_THREADS, 0, s>>>(a.off, d_dsrc, d_dsup);
        if (!sc_launched(e)) break;
        k_tx_fold<<<grid_of(Lb), SC_THREADS, 0, s>>>(a.off, nb, src->d_leaf_taxon, c.d_mm, d_acc, d_dsrc, d_dsup, d_tx,
                                                     n_out);
        if (!sc_launched(e)) break;
    }
    int64_t *const outs[5] = {tx_trees, tx_total, tx_super, tx_source, tx_shared};
    sc_fetch_rows(s, d_tx, (size_t)n_out, 5, outs, e);
    return sc_end(ctx, c, e, bad);
}

// the plans of scs_score_branch_triplets / scs_score_branch_resample and of scs_score_taxon_triplets on the host, by
// the functions those exports call
extern "C" int scs_debug_branch_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                     int32_t super_leaves, int32_t max_batch_trees, int64_t extra_per_leaf,
                                     int64_t extra_per_tree, int32_t max_lds_bytes, int32_t *n_batches_out,
                                     int32_t *bstart_out, int64_t *bt_out, int64_t *tx_out, int64_t *call_out) {
    sc_debug_plan d;
    SCS_TRY(sc_debug_batches("scs_debug_branch_plan", src, n_trees, tree_off, super_leaves, max_batch_trees,
                             extra_per_leaf, extra_per_tree, max_lds_bytes, bt_out && tx_out && call_out,
                             n_batches_out, bstart_out, d));
    const int64_t *off = d.off;
    const std::vector<int32_t> &bstart = d.bstart;
    const size_t n_batches = bstart.size() - 1;
    const sc_pair_plan bt = sc_plan_pairs(off, bstart, SC_BT_RULE);
    for (size_t b = 0; b < n_batches; ++b) {
        int64_t *o = bt_out + 4 * b;
        o[0] = bt.words[b];
        o[1] = bt.zbs[b];
        o[2] = (int64_t)bt.lds[b];
        o[3] = bt.blk[bstart[b + 1]] - bt.blk[bstart[b]];
    }
    const sc_tx_call tc = sc_tx_call_of(std::max<int64_t>(d.max_leaves, 0), max_lds_bytes);
    std::vector<int> words;
    std::vector<sc_tx_plan> plans;
    std::vector<char> slab_launches;
    std::vector<int64_t> blk;
    sc_tx_batches(off, bstart, tc, words, plans, slab_launches, blk);
    for (size_t b = 0; b < n_batches; ++b) {
        int64_t *o = tx_out + (4 * TX_BINS + 2) * b;
        for (int i = 0; i < TX_BINS; ++i) {
            const int64_t *bl = blk.data() + (size_t)i * (n_trees + 1);
            o[4 * i] = plans[b].zb[i];
            o[4 * i + 1] = plans[b].bins.dcap[i];
            o[4 * i + 2] = plans[b].lds[i];
            o[4 * i + 3] = bl[bstart[b + 1]] - bl[bstart[b]];
        }
        o[4 * TX_BINS] = slab_launches[b];
        o[4 * TX_BINS + 1] = (int64_t)sc_tx_slab_lds(words[b]);
    }
    call_out[0] = tc.need_slab;
    call_out[1] = tc.slab_wgs;
    call_out[2] = tc.slab_stride;
    return SCS_OK;
}

extern "C" int scs_score_placements(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                    const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                                    int32_t n_queries, const int32_t *queries, int64_t *pl_trees, int64_t *pl_total,
                                    int64_t *pl_source, int64_t *pl_super, int64_t *pl_shared) {
    const char *const who = "scs_score_placements";
    // a row pair (cl(z), cl(pz)) of the largest tree must fit one workgroup's LDS, as for scs_score_triplets; every
    // count of one tree is then below m^2 < 2^63
    SCS_TRY(sc_rows_fit(who, src, 16));
    SCS_REQUIRE(max_lds_bytes >= 0, "%s: max_lds_bytes = %d is negative", who, max_lds_bytes);
    SCS_REQUIRE(n_queries >= 1 && queries, "%s: no query taxon", who);
    SCS_TRY(sc_rows_fit(who, src, 16, max_lds_bytes));
    // the queries are tips of the supertree, each once; the tips' preorder index and depth by leaf position
    sc_walk sw;
    if (parent && taxon && n_nodes >= 1) {
        sw = sc_walk_super(n_nodes, parent, false);
        std::vector<int32_t> tips;
        for (const int32_t v : sw.tip_node) tips.push_back(taxon[v]);
        std::sort(tips.begin(), tips.end());
        std::vector<int32_t> qs(queries, queries + n_queries);
        std::sort(qs.begin(), qs.end());
        for (int32_t i = 0; i < n_queries; ++i) {
            SCS_REQUIRE(std::binary_search(tips.begin(), tips.end(), qs[i]),
                        "%s: query taxon %d is not a tip of the supertree", who, qs[i]);
            SCS_REQUIRE(i == 0 || qs[i] != qs[i - 1], "%s: query taxon %d is given twice", who, qs[i]);
        }
    }
    // own arrays: three rows of n_nodes + 1 sums per query and output (`sub`, later the values; `strict`; the
    // difference row), the two common rows per pass, three sums per query, the queries' S positions, S's parents and
    // tips, the first pair workgroup per tree (+ 1).  Per batch: a group list entry per leaf and query of a pass, two
    // node lists of two entries per leaf; per tree and query the query's positions and its list's length, per tree
    // the node list's length and the number of queries it holds
    const size_t nn = (size_t)std::max(n_nodes, 0), nq = (size_t)n_queries, mt = src ? (size_t)src->n_trees : 0;
    const size_t row_bytes = sc_up256(2 * nq * (nn + 1) * 8);
    const int qcap = std::min<int>(std::max(n_queries, 1), PL_QMAX);
    const size_t n_pass = (nq + qcap - 1) / qcap, common_bytes = sc_up256(2 * n_pass * nn * 8);
    SCS_REQUIRE(3 * (uint64_t)row_bytes + common_bytes <= SC_BUDGET,
                "%s: %d query taxa x %d supertree nodes need %llu bytes of rows, more than the %llu of the call's "
                "workspace", who, n_queries, n_nodes, (unsigned long long)(3 * (uint64_t)row_bytes + common_bytes),
                (unsigned long long)SC_BUDGET);
    unsigned long long *d_sub, *d_strict, *d_diff, *d_common, *d_qs;
    int32_t *d_qpos, *d_par, *d_tipn, *d_tipd;
    int64_t *d_blk;
    const auto own = [&](sc_carver w) {
        d_sub = w.take<unsigned long long>(2 * nq * (nn + 1));  // (row_bytes each; zeroed up to d_qpos in one go)
        d_strict = w.take<unsigned long long>(2 * nq * (nn + 1));
        d_diff = w.take<unsigned long long>(2 * nq * (nn + 1));
        d_common = w.take<unsigned long long>(2 * n_pass * nn);
        d_qs = w.take<unsigned long long>(3 * nq);
        d_qpos = w.take<int32_t>(nq);
        d_par = w.take<int32_t>(nn);
        d_tipn = w.take<int32_t>(nn);
        d_tipd = w.take<int32_t>(nn);
        d_blk = w.take<int64_t>(mt + 1);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, who, n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     sc_pl_extras(qcap).per_leaf, sc_pl_extras(qcap).per_tree, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_glist = wb.take<int4>(c.max_lb * qcap);
    auto *d_zlist = wb.take<int4>(2 * c.max_lb);
    auto *d_zmeta = wb.take<int4>(2 * c.max_lb);
    auto *d_qinfo = wb.take<int2>(c.max_rows * qcap);
    auto *d_gcnt = wb.take<int32_t>(c.max_rows * qcap);
    auto *d_zcnt = wb.take<int32_t>(c.max_rows);
    auto *d_qheld = wb.take<int32_t>(c.max_rows);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    hipStream_t s = ctx->stream;
    std::vector<int32_t> q_spos(nq);
    for (size_t i = 0; i < nq; ++i) q_spos[i] = queries[i] < c.n_taxa ? c.s_pos[queries[i]] : -1;
    // per batch: W words per bitset row, zb S' nodes per workgroup and whether the sums of a pass fit beside the rows;
    // blk: the first pair workgroup of every tree
    const sc_pair_plan pl = sc_plan_pairs(src->h_tree_off.data(), c.bstart, sc_pl_rule(qcap, sc_lds_cap(max_lds_bytes)));
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_sub, 0, (size_t)((char *)d_qpos - (char *)d_sub), s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qpos, q_spos.data(), nq * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_par, parent, nn * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_tipn, sw.tip_node.data(), sw.tip_node.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_tipd, sw.tip_depth.data(), sw.tip_depth.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk, pl.blk.data(), (mt + 1) * 8, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_pl_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        e = hipMemsetAsync(d_zcnt, 0, (size_t)nb * 4, s);
        if (e != hipSuccess) break;
        auto a = sc_args<sc_pl_args>(v);
        a.tip_node = d_tipn;
        a.tip_depth = d_tipd;
        a.zlist = d_zlist;
        a.zmeta = d_zmeta;
        a.zcnt = d_zcnt;
        a.qinfo = d_qinfo;
        a.glist = d_glist;
        a.gcnt = d_gcnt;
        k_pl_znodes<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        const int64_t n_wg = pl.blk[t0 + nb] - pl.blk[t0];
        for (int32_t q0 = 0; q0 < n_queries && n_wg > 0; q0 += qcap) {
            const int qc = std::min<int>(qcap, n_queries - q0);
            a.qc = qc;
            a.q_source = d_qs + 2 * nq + q0;
            e = hipMemsetAsync(d_qheld, 0, (size_t)nb * 4, s);
            if (e != hipSuccess) break;
            k_pl_queries<<<grid_of((int64_t)nb * qc), SC_THREADS, 0, s>>>(a.off, nb, d_qpos + q0, qc, c.d_rows,
                                                                          c.row_stride, c.d_sp, d_qinfo, d_gcnt,
                                                                          d_qheld, d_qs + q0, d_qs + nq + q0);
            if (!sc_launched(e)) break;
            k_pl_groups<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            sc_pl_pair_args pa;
            pa.blk = d_blk + t0;
            pa.nb = nb;
            pa.off = a.off;
            pa.glist = d_glist;
            pa.gcnt = d_gcnt;
            pa.qinfo = d_qinfo;
            pa.qheld = d_qheld;
            pa.qc = qc;
            pa.zlist = d_zlist;
            pa.zmeta = d_zmeta;
            pa.zcnt = d_zcnt;
            pa.tp = c.d_mm;
            pa.zb = pl.zbs[b];
            pa.W = pl.words[b];
            pa.lds_sums = pl.sums[b];
            pa.sub = d_sub + (size_t)q0 * nn;
            pa.strict = d_strict + (size_t)q0 * nn;
            pa.row_stride = (int64_t)nn;
            pa.super_off = (int64_t)(nq * nn);
            pa.csub = d_common + (size_t)(q0 / qcap) * nn;
            pa.cstrict = d_common + (n_pass + (size_t)(q0 / qcap)) * nn;
            k_pl_pairs<<<(unsigned)n_wg, SC_THREADS, sc_pl_lds(pl, b, qc), s>>>(pa);
            if (!sc_launched(e)) break;
        }
    }
    if (e == hipSuccess && !bad) {
        k_pl_marks<<<grid_of((int64_t)(2 * nq * nn)), SC_THREADS, 0, s>>>(d_sub, d_strict, d_common,
                                                                        d_common + n_pass * nn, qcap, d_par, c.d_end,
                                                                        (int64_t)nn, (int64_t)(2 * nq), d_diff);
        sc_launched(e);
    }
    if (e == hipSuccess && !bad) {
        k_pl_prefix<<<(unsigned)(2 * nq), 1024, 0, s>>>(d_diff, (int64_t)nn, d_sub);
        sc_launched(e);
    }
    int64_t *const scal[3] = {pl_trees, pl_total, pl_source}, *const rows[2] = {pl_shared, pl_super};
    sc_fetch_rows(s, d_qs, nq, 3, scal, e);
    sc_fetch_rows(s, d_sub, nq * nn, 2, rows, e);
    return sc_end(ctx, c, e, bad);
}

// what scs_score_clade_placements and scs_score_clade_moves share: the checks, the sweep and the rows in the call's
// workspace.  top_k = 0: the rows are copied out (cp_super, cp_shared); top_k >= 1: k_cp_best reduces them where they
// are and only its outputs come down
static int sc_clade_rows(const char *const who, scs_ctx *ctx, const scs_tables *src, int32_t n_nodes,
                         const int32_t *parent, const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                         int32_t n_queries, const int32_t *query_nodes, int32_t top_k, int64_t *cp_trees,
                         int64_t *cp_total, int64_t *cp_source, int64_t *cp_super, int64_t *cp_shared,
                         int64_t *mv_own_super, int64_t *mv_own_shared, int32_t *mv_node, int64_t *mv_super,
                         int64_t *mv_shared) {
    SCS_TRY(sc_rows_fit(who, src, 16));
    SCS_REQUIRE(max_lds_bytes >= 0, "%s: max_lds_bytes = %d is negative", who, max_lds_bytes);
    SCS_REQUIRE(n_queries >= 1 && query_nodes, "%s: no query node", who);
    SCS_TRY(sc_rows_fit(who, src, 16, max_lds_bytes));
    // the query nodes: not the root, in range, each once; their leaf ranges; the tips' preorder index and depth by
    // leaf position; the sub-queries (the S positions of every clade's tips, clade by clade)
    sc_walk sw;
    std::vector<int32_t> c_lo, c_hi, q_spos, q_clade;
    if (parent && taxon && n_nodes >= 1) {
        sw = sc_walk_super(n_nodes, parent, true);
        std::vector<char> seen((size_t)n_nodes, 0);
        for (int32_t i = 0; i < n_queries; ++i) {
            const int32_t q = query_nodes[i];
            SCS_REQUIRE(q >= 1 && q < n_nodes, "%s: query node %d is the root or out of range [1, %d)", who, q, n_nodes);
            SCS_REQUIRE(!seen[q], "%s: query node %d is given twice", who, q);
            seen[q] = 1;
            c_lo.push_back(sw.lo[q]);
            c_hi.push_back(sw.hi[q]);
            for (int32_t p = sw.lo[q]; p <= sw.hi[q]; ++p) {
                q_spos.push_back(p);
                q_clade.push_back(i);
            }
        }
    }
    // own arrays: three rows of n_nodes + 1 sums per clade and output (`sub`, later the values; `strict`; the
    // difference row), three sums per clade, the clades' leaf ranges, the sub-queries, S's parents and tips, the first
    // pair workgroup per tree (+ 1).  Per batch: a group list entry (24 bytes) per leaf and sub-query of a pass, a
    // word of a Q' row per 32 leaves and clade of a pass, two node lists of two entries per leaf; per tree and
    // sub-query the clade's range, the tip's position and its list's length
    const size_t nn = (size_t)std::max(n_nodes, 0), nq = (size_t)n_queries, ns = q_spos.size(),
                 mt = src ? (size_t)src->n_trees : 0;
    const size_t row_bytes = sc_up256(2 * nq * (nn + 1) * 8);
    SCS_REQUIRE(3 * (uint64_t)row_bytes <= SC_BUDGET,
                "%s: %d query clades x %d supertree nodes need %llu bytes of rows, more than the %llu of the call's "
                "workspace", who, n_queries, n_nodes, (unsigned long long)(3 * (uint64_t)row_bytes),
                (unsigned long long)SC_BUDGET);
    const int qcap = (int)std::min<size_t>(std::max<size_t>(ns, 1), CP_QMAX);
    // (after the sweep's arrays the reduced rows, top_k >= 1: the query nodes, then per query top_k (node, super,
    // shared) and its own pair)
    const size_t kk = (size_t)top_k;
    unsigned long long *d_sub, *d_strict, *d_diff, *d_cs;
    int32_t *d_clo, *d_chi, *d_qpos, *d_qslot, *d_par, *d_tipn, *d_tipd, *d_qnode = nullptr, *d_mvn;
    int64_t *d_blk;
    long long *d_mvs, *d_mvh, *d_own = nullptr;
    const auto own = [&](sc_carver w) {
        d_sub = w.take<unsigned long long>(2 * nq * (nn + 1));  // (row_bytes each; zeroed up to d_clo in one go)
        d_strict = w.take<unsigned long long>(2 * nq * (nn + 1));
        d_diff = w.take<unsigned long long>(2 * nq * (nn + 1));
        d_cs = w.take<unsigned long long>(3 * nq);
        d_clo = w.take<int32_t>(nq);
        d_chi = w.take<int32_t>(nq);
        d_qpos = w.take<int32_t>(ns);
        d_qslot = w.take<int32_t>(ns);
        d_par = w.take<int32_t>(nn);
        d_tipn = w.take<int32_t>(nn);
        d_tipd = w.take<int32_t>(nn);
        d_blk = w.take<int64_t>(mt + 1);
        if (kk) d_qnode = w.take<int32_t>(nq);
        d_mvn = w.take<int32_t>(nq * kk);
        d_mvs = w.take<long long>(nq * kk);
        d_mvh = w.take<long long>(nq * kk);
        if (kk) d_own = w.take<long long>(2 * nq);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, who, n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     sc_cp_extras(qcap).per_leaf, sc_cp_extras(qcap).per_tree, c, e));
    const int64_t max_rstride = (c.max_lb >> 5) + c.max_rows;
    sc_carver wb = sc_carve_batch(c);
    auto *d_glist = wb.take<int4>(c.max_lb * qcap);
    auto *d_zlist = wb.take<int4>(2 * c.max_lb);
    auto *d_zmeta = wb.take<int4>(2 * c.max_lb);
    auto *d_cinfo = wb.take<int4>(c.max_rows * qcap);
    auto *d_gq = wb.take<int2>(c.max_lb * qcap);
    auto *d_qrow = wb.take<int2>(max_rstride * qcap);
    auto *d_qinfo = wb.take<int2>(c.max_rows * qcap);
    auto *d_gcnt = wb.take<int32_t>(c.max_rows * qcap);
    auto *d_zcnt = wb.take<int32_t>(c.max_rows);
    auto *d_qheld = wb.take<int32_t>(c.max_rows);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    hipStream_t s = ctx->stream;
    // the sub-queries' slots: the clade's index less the first clade of the sub-query's pass
    std::vector<int32_t> q_slot(ns);
    for (size_t i = 0; i < ns; ++i) q_slot[i] = q_clade[i] - q_clade[i / qcap * qcap];
    // per batch W, zb and whether the sums fit, and blk, as in scs_score_placements
    const sc_pair_plan pl = sc_plan_pairs(src->h_tree_off.data(), c.bstart, sc_pl_rule(qcap, sc_lds_cap(max_lds_bytes)));
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_sub, 0, (size_t)((char *)d_clo - (char *)d_sub), s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_clo, c_lo.data(), nq * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_chi, c_hi.data(), nq * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qpos, q_spos.data(), ns * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qslot, q_slot.data(), ns * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_par, parent, nn * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_tipn, sw.tip_node.data(), sw.tip_node.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(d_tipd, sw.tip_depth.data(), sw.tip_depth.size() * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk, pl.blk.data(), (mt + 1) * 8, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_cp_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        const int64_t Lb = v.Lb;
        e = hipMemsetAsync(d_zcnt, 0, (size_t)nb * 4, s);
        if (e != hipSuccess) break;
        // k_pl_znodes, the one kernel launched with these arguments here, reads nothing of a query: those members of
        // sc_pl_args stay null (the clades' own lists go through sc_cp_args below)
        auto za = sc_args<sc_pl_args>(v);
        za.tip_node = d_tipn;
        za.tip_depth = d_tipd;
        za.zlist = d_zlist;
        za.zmeta = d_zmeta;
        za.zcnt = d_zcnt;
        za.qinfo = nullptr;
        za.qc = 0;
        za.glist = nullptr;
        za.gcnt = nullptr;
        za.q_source = nullptr;
        k_pl_znodes<<<grid_of(Lb), SC_THREADS, 0, s>>>(za);
        if (!sc_launched(e)) break;
        const int64_t n_wg = pl.blk[t0 + nb] - pl.blk[t0];
        const int64_t rstride = (Lb >> 5) + nb;
        for (size_t i0 = 0; i0 < ns && n_wg > 0; i0 += qcap) {
            const int qc = (int)std::min<size_t>(qcap, ns - i0);
            const int32_t c0 = q_clade[i0], c1 = q_clade[i0 + qc - 1];
            auto a = sc_args<sc_cp_args>(v);
            a.rows = c.d_rows;
            a.row_stride = c.row_stride;
            a.c_lo = d_clo + c0;
            a.c_hi = d_chi + c0;
            a.q_spos = d_qpos + i0;
            a.q_slot = d_qslot + i0;
            a.ncl = c1 - c0 + 1;
            a.qc = qc;
            a.skip0 = i0 > 0 && q_clade[i0 - 1] == c0;
            a.qrow = d_qrow;
            a.rstride = rstride;
            a.cinfo = d_cinfo;
            a.qinfo = d_qinfo;
            a.gcnt = d_gcnt;
            a.qheld = d_qheld;
            a.glist = d_glist;
            a.gq = d_gq;
            a.c_trees = d_cs + c0;
            a.c_total = d_cs + nq + c0;
            a.c_source = d_cs + 2 * nq + c0;
            a.sub = d_sub + (size_t)c0 * nn;
            a.node_stride = (int64_t)nn;
            a.super_off = (int64_t)(nq * nn);
            e = hipMemsetAsync(d_qheld, 0, (size_t)nb * 4, s);
            if (e == hipSuccess) e = hipMemsetAsync(d_qrow, 0, (size_t)a.ncl * rstride * 8, s);
            if (e != hipSuccess) break;
            k_cp_clades<<<(unsigned)((int64_t)nb * a.ncl), SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            k_cp_queries<<<grid_of((int64_t)nb * qc), SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            if (a.ncl > a.skip0) {
                k_cp_nodes<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
                if (!sc_launched(e)) break;
            }
            k_cp_groups<<<grid_of(Lb), SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            sc_cp_pair_args pa;
            pa.blk = d_blk + t0;
            pa.nb = nb;
            pa.off = a.off;
            pa.glist = d_glist;
            pa.gq = d_gq;
            pa.gcnt = d_gcnt;
            pa.qinfo = d_qinfo;
            pa.cinfo = d_cinfo;
            pa.qheld = d_qheld;
            pa.qc = qc;
            pa.ncl = a.ncl;
            pa.skip0 = a.skip0;
            pa.zlist = d_zlist;
            pa.zmeta = d_zmeta;
            pa.zcnt = d_zcnt;
            pa.tp = c.d_mm;
            pa.zb = pl.zbs[b];
            pa.W = pl.words[b];
            pa.lds_sums = pl.sums[b];
            pa.sub = a.sub;
            pa.strict = d_strict + (size_t)c0 * nn;
            pa.row_stride = (int64_t)nn;
            pa.super_off = a.super_off;
            k_cp_pairs<<<(unsigned)n_wg, SC_THREADS, sc_pl_lds(pl, b, qc), s>>>(pa);
            if (!sc_launched(e)) break;
        }
    }
    if (e == hipSuccess && !bad) {
        k_cp_marks<<<grid_of((int64_t)(2 * nq * nn)), SC_THREADS, 0, s>>>(d_sub, d_strict, d_par, c.d_end, (int64_t)nn,
                                                                        (int64_t)(2 * nq), d_diff);
        sc_launched(e);
    }
    if (e == hipSuccess && !bad) {
        k_pl_prefix<<<(unsigned)(2 * nq), 1024, 0, s>>>(d_diff, (int64_t)nn, d_sub);
        sc_launched(e);
    }
    int64_t *const scal[3] = {cp_trees, cp_total, cp_source}, *const rows[2] = {cp_shared, cp_super};
    sc_fetch_rows(s, d_cs, nq, 3, scal, e);
    sc_fetch_rows(s, d_sub, nq * nn, 2, rows, e);
    if (top_k > 0 && e == hipSuccess && !bad) {
        e = hipMemcpyAsync(d_qnode, query_nodes, nq * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) {
            k_cp_best<<<(unsigned)nq, SC_THREADS, 0, s>>>((const long long *)d_sub, (const long long *)(d_sub + nq * nn),
                                                         (int64_t)nn, d_qnode, c.d_end, top_k, d_mvn, d_mvs, d_mvh,
                                                         d_own, d_own + nq);
            sc_launched(e);
        }
        if (e == hipSuccess && mv_node) e = hipMemcpyAsync(mv_node, d_mvn, nq * kk * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && mv_super) e = hipMemcpyAsync(mv_super, d_mvs, nq * kk * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && mv_shared) e = hipMemcpyAsync(mv_shared, d_mvh, nq * kk * 8, hipMemcpyDeviceToHost, s);
        int64_t *const owns[2] = {mv_own_super, mv_own_shared};
        sc_fetch_rows(s, d_own, nq, 2, owns, e);
    }
    return sc_end(ctx, c, e, bad);
}

extern "C" int scs_score_clade_placements(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                          const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                                          int32_t n_queries, const int32_t *query_nodes, int64_t *cp_trees,
                                          int64_t *cp_total, int64_t *cp_source, int64_t *cp_super,
                                          int64_t *cp_shared) {
    return sc_clade_rows("scs_score_clade_placements", ctx, src, n_nodes, parent, taxon, max_batch_trees,
                         max_lds_bytes, n_queries, query_nodes, 0, cp_trees, cp_total, cp_source, cp_super, cp_shared,
                         nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int scs_score_clade_moves(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                     const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                                     int32_t n_queries, const int32_t *query_nodes, int32_t top_k, int64_t *cp_trees,
                                     int64_t *cp_total, int64_t *cp_source, int64_t *mv_own_super,
                                     int64_t *mv_own_shared, int32_t *mv_node, int64_t *mv_super, int64_t *mv_shared) {
    SCS_REQUIRE(top_k >= 1 && top_k <= MV_KMAX, "scs_score_clade_moves: top_k = %d is not in [1, %d]", top_k, MV_KMAX);
    return sc_clade_rows("scs_score_clade_moves", ctx, src, n_nodes, parent, taxon, max_batch_trees, max_lds_bytes,
                         n_queries, query_nodes, top_k, cp_trees, cp_total, cp_source, nullptr, nullptr, mv_own_super,
                         mv_own_shared, mv_node, mv_super, mv_shared);
}

// ---- supertree polytomies (scs_score_polytomies) ----
//
// A polytomy p of S with children c_0 .. c_{k-1} (k >= 3) colours the leaves of a source tree T: colour i is
// C_i' = cl(c_i) ∩ L(T), a stretch of S' indices (the children of p are contiguous in S's leaf order).  T is decisive
// when three colours or more are not empty.  For i < j and l not in {i, j}, over the decisive trees:
//   py_total[i][j][l] = sum_T |C_i'| |C_j'| |C_l'|
//   py_joint[i][j][l] = sum_T sum_y I(y,C_i') I(y,C_j') (I(py,C_l') - I(y,C_l'))     (the node sum of section 18)
//   k_py_records: one thread per gap lists T's non-root nodes {lo, hi + 1, parent lo, parent hi + 1} (k_bt_records'
//     T half); k_py_colours: one thread per (tree, query) finds the k + 1 colour boundaries in S' order, says whether
//     the tree is decisive and counts it in py_trees; k_py_total: one thread per output entry sums the batch's sizes.
//   k_py_sweep, the hot path: one workgroup per (tree, query, colour i).  The k colours become bitset rows over T
//     positions in LDS ({bits, prefix}, as k_bt_pairs); a wave takes a node y with lane = colour: lane c holds
//     h[c] = I(y,C_c') and d[c] = I(py,C_c') - h[c] from four reads of its own row, a ballot names the colours j > i
//     present in y, and for each of them lane l adds h[i] h[j] d[l] onto accumulator [j][l] -- 64-bit atomics, in LDS
//     where k^2 sums fit beside the rows (one flush of the non-zero ones at the end), else straight onto the output.

namespace {

constexpr int PY_KMAX = 64;  // children of a query node: one lane each

struct sc_py_rec_args : sc_batch {
    int4 *ylist;               // [Lb] T's nodes of a tree from its first leaf on
    int32_t *ycnt;              // [nb] list lengths
};

// one thread per gap: T's non-root internal node that starts here (as k_bt_records lists it)
__global__ void __launch_bounds__(SC_THREADS) k_py_records(sc_py_rec_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = a.off[0] + q;
    const bool in = p < a.off[a.nb];
    const int t = in ? sc_tree_of(a.off, a.nb, p) : a.nb - 1;
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int64_t k = q - base;
    int4 ny = make_int4(0, 0, 0, 0);
    bool t_node = false;
    if (in && k + 1 < n) {
        const int32_t d = a.adj[q];
        const int64_t lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
        if (lo == 0 || a.adj[base + lo - 1] < d) {
            const int64_t hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
            if (lo > 0 || hi < n - 1) {  // (not the root)
                const int64_t g = lo == 0 ? hi
                                  : hi == n - 1 ? lo - 1
                                  : (a.adj[base + lo - 1] >= a.adj[base + hi] ? lo - 1 : hi);
                const int32_t dg = a.adj[base + g];
                const int64_t plo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, g, dg, true);
                const int64_t phi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, g + 1, n - 1, dg);
                t_node = true;
                ny = make_int4((int)lo, (int)hi + 1, (int)plo, (int)phi + 1);
            }
        }
    }
    const int iy = sc_append(a.ycnt, t, t_node);
    if (iy >= 0) a.ylist[base + iy] = ny;
}

// what the colour, total and sweep kernels share: query q has k = coff[q + 1] - coff[q] - 1 children, its k + 1
// boundaries (S positions: the first leaf of every child, then one past the node's last) at bnd[coff[q] ...], the same
// slots in a tree's row of cidx (S' indices), and its k^3 output entries at ooff[q]
struct sc_py_args : sc_batch {
    int nq, totb;             // queries, boundaries of all queries
    const int32_t *coff;     // [nq + 1]
    const int64_t *ooff;      // [nq + 1]
    const int32_t *bnd;       // [totb]
    int32_t *cidx;            // [nb][totb]
    int32_t *dec;             // [nb][nq] 1: the tree is decisive at the query
    unsigned long long *trees, *total, *joint;  // py_trees [nq], py_total / py_joint [ooff[nq]]
    // the sweep alone: the queries of one degree k, T's node lists, the words of a row and its stride in LDS (and of
    // the batch view off and mm, moved to the launch's first tree)
    const int32_t *gq;
    int ngq, k, W, Ws, acc_lds;
    const int4 *ylist;
    const int32_t *ycnt;
};

// one thread per (tree, query): the colour boundaries in the tree's S' order; decisive trees counted
__global__ void __launch_bounds__(SC_THREADS) k_py_colours(sc_py_args a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)a.nb * a.nq) return;
    const int t = (int)(idx / a.nq), q = (int)(idx % a.nq);
    const int64_t base = a.off[t] - a.off[0];
    const int64_t n = a.off[t + 1] - a.off[t];
    const int32_t c0 = a.coff[q], k = a.coff[q + 1] - c0 - 1;
    int32_t *cx = a.cidx + (int64_t)t * a.totb + c0;
    int32_t prev = 0, present = 0;
    for (int i = 0; i <= k; ++i) {
        const int32_t c = (int32_t)sc_first_ge(a.sp + base, 0, n, a.bnd[c0 + i]);
        cx[i] = c;
        if (i > 0 && c > prev) ++present;
        prev = c;
    }
    const int32_t dec = present >= 3;
    a.dec[idx] = dec;
    if (dec) atomicAdd(a.trees + q, 1ull);
}

// one thread per output entry [i][j][l] with i < j, l not in {i, j}: the batch's decisive trees' |C_i'| |C_j'| |C_l'|
// (one thread owns the entry and the batches follow each other on the stream: a plain add)
__global__ void __launch_bounds__(SC_THREADS) k_py_total(sc_py_args a) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.ooff[a.nq]) return;
    const int q = sc_tree_of(a.ooff, a.nq, e);
    const int32_t c0 = a.coff[q], k = a.coff[q + 1] - c0 - 1;
    const int64_t r = e - a.ooff[q];
    const int l = (int)(r % k), j = (int)(r / k % k), i = (int)(r / ((int64_t)k * k));
    if (!(i < j && l != i && l != j)) return;
    unsigned long long sum = 0;
    for (int t = 0; t < a.nb; ++t) {
        if (!a.dec[(int64_t)t * a.nq + q]) continue;
        const int32_t *cx = a.cidx + (int64_t)t * a.totb + c0;
        sum += (unsigned long long)((int64_t)(cx[i + 1] - cx[i]) * (cx[j + 1] - cx[j]) * (cx[l + 1] - cx[l]));
    }
    if (sum) a.total[e] += sum;
}

// set bits of a bitset row at the T positions below x: the word of position x - 1 and the bits up to it (a row of
// ceil(n / 32) words answers every x <= n)
__device__ __forceinline__ int py_count(const int2 *row, int x) {
    if (x == 0) return 0;
    const int2 r = row[(x - 1) >> 5];
    return r.y + __popc((unsigned)r.x & (0xffffffffu >> (31 - ((x - 1) & 31))));
}

// the hot path: workgroup (x, y) = (query of the degree and colour i, tree of the chunk at a.off)
__global__ void __launch_bounds__(SC_THREADS) k_py_sweep(sc_py_args a) {
    extern __shared__ __attribute__((aligned(16))) int2 rows[];  // [k][Ws], then k^2 sums when acc_lds
    const int k = a.k, Ws = a.Ws;
    const int t = blockIdx.y;
    const int q = a.gq[blockIdx.x / (k - 1)], ci = (int)(blockIdx.x % (k - 1));
    if (!a.dec[(int64_t)t * a.nq + q]) return;
    const int32_t *cx = a.cidx + (int64_t)t * a.totb + a.coff[q];
    // every term has the factors I(y, C_i') and I(y, C_j') of a j > i
    if (cx[ci + 1] == cx[ci] || cx[k] == cx[ci + 1]) return;
    const int64_t base = a.off[t] - a.off[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(rows + k * Ws);
    for (int i = threadIdx.x; i < k * Ws; i += SC_THREADS) rows[i] = make_int2(0, 0);
    if (a.acc_lds)
        for (int i = threadIdx.x; i < k * k; i += SC_THREADS) acc[i] = 0;
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);  // (word i of the image: .x of entry i / 2)
    for (int c = wave; c < k; c += SC_THREADS / 64)
        for (int s = cx[c] + lane; s < cx[c + 1]; s += 64) {
            const int x = a.mm[base + s].x;
            atomicOr(bits + 2 * (c * Ws + (x >> 5)), 1u << (x & 31));
        }
    __syncthreads();
    // every word's .y = set bits in the words before it: one wave per row, wave64 scans of 64 words
    for (int r = wave; r < k; r += SC_THREADS / 64) {
        int2 *row = rows + r * Ws;
        int run = 0;
        for (int c = 0; c < a.W; c += 64) {
            const int i = c + lane;
            const int v = i < a.W ? __popc((unsigned)row[i].x) : 0;
            int incl = v;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(incl, d, 64);
                if (lane >= d) incl += y;
            }
            if (i < a.W) row[i].y = run + incl - v;
            run += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    unsigned long long *out = a.joint + a.ooff[q] + (int64_t)ci * k * k;  // entries [ci][j][l] at j * k + l
    const bool mine = lane < k;
    const int2 *row = rows + (mine ? lane : 0) * Ws, *row_i = rows + ci * Ws;
    const int ny = a.ycnt[t];
    for (int iy = wave; iy < ny; iy += SC_THREADS / 64) {
        const int4 y = a.ylist[base + iy];  // T positions [y.x, y.y) of y, [y.z, y.w) of py
        const int hi = py_count(row_i, y.y) - py_count(row_i, y.x);  // (the same for every lane)
        if (hi == 0) continue;
        int h = 0, d = 0;
        if (mine) {
            h = py_count(row, y.y) - py_count(row, y.x);
            d = py_count(row, y.w) - py_count(row, y.z) - h;
        }
        unsigned long long mj = __ballot(h > 0) & ~((2ull << ci) - 1ull);
        const bool third = d != 0 && lane != ci;
        if (mj == 0 || !__any(third)) continue;
        while (mj) {
            const int j = __ffsll((long long)mj) - 1;
            mj &= mj - 1;
            const int hj = __shfl(h, j, 64);
            if (third && lane != j) {
                const unsigned long long v = (unsigned long long)((int64_t)hi * hj * d);
                if (a.acc_lds) atomicAdd(acc + j * k + lane, v);
                else atomicAdd(out + j * k + lane, v);
            }
        }
    }
    if (!a.acc_lds) return;
    __syncthreads();
    for (int i = threadIdx.x; i < k * k; i += SC_THREADS) {
        const unsigned long long v = acc[i];
        if (v) atomicAdd(out + i, v);
    }
}

// the sweep's plan for one batch and degree k, for scs_score_polytomies and scs_debug_placement_plan alike: W words per
// row (largest tree of the batch, ceil(n / 32)); the rows' stride Ws is odd where that fits (lane = row: an even stride
// puts the lanes' reads on few banks); the k^2 sums in LDS where they fit beside the rows; lds: the launch's bytes
struct sc_py_plan {
    int W, Ws, acc_lds;
    size_t lds;
};

int sc_py_words(int64_t n_max) { return (int)std::max<int64_t>((n_max + 31) >> 5, 1); }

sc_py_plan sc_py_plan_of(int W, int k, int lds_cap) {
    sc_py_plan p;
    const int64_t accb = (int64_t)k * k * 8, odd = W | 1;
    const bool acc_odd = k * odd * 8 + accb <= lds_cap, acc_even = (int64_t)k * W * 8 + accb <= lds_cap;
    p.W = W;
    p.acc_lds = acc_odd || acc_even;
    p.Ws = (p.acc_lds ? acc_odd : k * odd * 8 <= lds_cap) ? (int)odd : W;
    p.lds = (size_t)k * p.Ws * 8 + (p.acc_lds ? (size_t)accb : 0);
    return p;
}

}  // namespace

extern "C" int scs_score_polytomies(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                    const int32_t *taxon, int32_t max_batch_trees, int32_t max_lds_bytes,
                                    int32_t n_queries, const int32_t *query_nodes, int32_t *py_degree,
                                    int64_t *py_trees, int64_t *py_total, int64_t *py_joint) {
    const char *const who = "scs_score_polytomies";
    const int64_t m_max = sc_max_leaves(src);
    SCS_REQUIRE(max_lds_bytes >= 0, "%s: max_lds_bytes = %d is negative", who, max_lds_bytes);
    SCS_REQUIRE(n_queries >= 1 && query_nodes, "%s: no query node", who);
    const int lds_cap = sc_lds_cap(max_lds_bytes);
    // the query nodes: nodes, each once, 3 to PY_KMAX children; their children in child order
    const size_t nq = (size_t)n_queries;
    std::vector<int32_t> coff(nq + 1, 0), kid_of;  // kid_of: the children of query i at coff[i] - i ...
    std::vector<int64_t> ooff(nq + 1, 0);
    int k_max = 0;
    if (parent && taxon && n_nodes >= 1) {
        const std::vector<int32_t> n_kids = sc_walk_super(n_nodes, parent, false).n_kids;
        std::vector<int32_t> slot((size_t)n_nodes, -1);
        for (size_t i = 0; i < nq; ++i) {
            const int32_t q = query_nodes[i];
            SCS_REQUIRE(q >= 0 && q < n_nodes, "%s: query node %d is not in [0, %d)", who, q, n_nodes);
            SCS_REQUIRE(slot[q] < 0, "%s: query node %d is given twice", who, q);
            const int32_t k = n_kids[q];
            SCS_REQUIRE(k >= 3, "%s: query node %d has %d children, fewer than the 3 of a polytomy", who, q, k);
            SCS_REQUIRE(k <= PY_KMAX, "%s: query node %d has %d children, more than the %d the sweep has lanes for",
                        who, q, k, PY_KMAX);
            slot[q] = (int32_t)i;
            coff[i + 1] = coff[i] + k + 1;
            ooff[i + 1] = ooff[i] + (int64_t)k * k * k;
            k_max = std::max(k_max, (int)k);
        }
        kid_of.assign((size_t)coff[nq], -1);
        std::vector<int32_t> fill(nq, 0);
        for (int32_t v = 1; v < n_nodes; ++v)
            if (parent[v] >= 0 && parent[v] < v && slot[parent[v]] >= 0) {
                const int32_t i = slot[parent[v]];
                kid_of[coff[i] + fill[i]++] = v;
            }
    }
    const int64_t w_max = sc_py_words(m_max);
    SCS_REQUIRE((int64_t)k_max * w_max * 8 <= lds_cap,
                "%s: the %d rows of a source tree of %lld leaves take %lld bytes, more than the %d of a workgroup's "
                "LDS%s", who, k_max, (long long)m_max, (long long)k_max * w_max * 8, lds_cap,
                max_lds_bytes > 0 ? " (max_lds_bytes)" : "");
    SCS_REQUIRE((uint64_t)ooff[nq] * 16 <= SC_BUDGET,
                "%s: the tensors of %d query nodes need %llu bytes, more than the %llu of the call's workspace", who,
                n_queries, (unsigned long long)ooff[nq] * 16, (unsigned long long)SC_BUDGET);
    // an entry is at most sum_t (m_t / 3)^3: it must fit int64
    SCS_TRY(sc_cubes_fit(who, src));
    // own arrays: the two tensors, py_trees, the offsets, the boundaries and the queries by degree; per batch T's node
    // list (int4) per leaf, its length per tree, and per tree the boundaries in S' order and the decisive flags
    const size_t totb = (size_t)coff[nq], n_out = (size_t)ooff[nq];
    unsigned long long *d_total, *d_joint, *d_trees;
    int32_t *d_coff, *d_bnd, *d_gq;
    int64_t *d_ooff;
    const auto own = [&](sc_carver w) {
        d_total = w.take<unsigned long long>(n_out);  // (both tensors and py_trees are zeroed in one go)
        d_joint = w.take<unsigned long long>(n_out);
        d_trees = w.take<unsigned long long>(nq);
        d_coff = w.take<int32_t>(nq + 1);
        d_ooff = w.take<int64_t>(nq + 1);
        d_bnd = w.take<int32_t>(totb);
        d_gq = w.take<int32_t>(nq);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, who, n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     sc_py_extras(totb, nq).per_leaf, sc_py_extras(totb, nq).per_tree, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_ylist = wb.take<int4>(c.max_lb);
    auto *d_ycnt = wb.take<int32_t>(c.max_rows);
    auto *d_cidx = wb.take<int32_t>(c.max_rows * totb);
    auto *d_dec = wb.take<int32_t>(c.max_rows * nq);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const std::vector<int64_t> &off = src->h_tree_off;
    hipStream_t s = ctx->stream;
    // the boundaries (S positions, sc_begin's leaf ranges) and the queries grouped by degree
    std::vector<int32_t> bnd(totb), gq(nq), g_first(PY_KMAX + 2, 0);
    for (size_t i = 0; i < nq; ++i) {
        const int32_t k = coff[i + 1] - coff[i] - 1;
        for (int32_t j = 0; j < k; ++j) bnd[coff[i] + j] = c.s_lo[kid_of[coff[i] + j]];
        bnd[coff[i] + k] = c.s_hi[query_nodes[i]] + 1;
        if (py_degree) py_degree[i] = k;
        g_first[k + 1]++;
    }
    for (int k = 0; k <= PY_KMAX; ++k) g_first[k + 1] += g_first[k];
    {
        std::vector<int32_t> at(g_first.begin(), g_first.end() - 1);
        for (size_t i = 0; i < nq; ++i) gq[at[coff[i + 1] - coff[i] - 1]++] = (int32_t)i;
    }
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_total, 0, (size_t)((char *)d_coff - (char *)d_total), s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_coff, coff.data(), (nq + 1) * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ooff, ooff.data(), (nq + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_bnd, bnd.data(), totb * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_gq, gq.data(), nq * 4, hipMemcpyHostToDevice, s);
    // (the attribute is per function and device: set on every call)
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_py_sweep, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        e = hipMemsetAsync(d_ycnt, 0, (size_t)nb * 4, s);
        if (e != hipSuccess) break;
        auto r = sc_args<sc_py_rec_args>(v);
        r.ylist = d_ylist;
        r.ycnt = d_ycnt;
        k_py_records<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(r);
        if (!sc_launched(e)) break;
        auto a = sc_args<sc_py_args>(v);  // (the sweep's own members: zero until its launches)
        a.nq = n_queries;
        a.totb = (int)totb;
        a.coff = d_coff;
        a.ooff = d_ooff;
        a.bnd = d_bnd;
        a.cidx = d_cidx;
        a.dec = d_dec;
        a.trees = d_trees;
        a.total = d_total;
        a.joint = d_joint;
        a.gq = d_gq;
        a.ylist = d_ylist;
        a.ycnt = d_ycnt;
        k_py_colours<<<grid_of((int64_t)nb * n_queries), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        k_py_total<<<grid_of((int64_t)n_out), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        // the sweep, one launch per degree (and chunk of 65535 trees), by sc_py_plan_of
        a.W = sc_py_words(sc_largest_tree(off.data(), t0, t0 + nb));
        for (int k = 3; k <= PY_KMAX && e == hipSuccess; ++k) {
            const int ng = g_first[k + 1] - g_first[k];
            if (ng == 0) continue;
            const sc_py_plan pp = sc_py_plan_of(a.W, k, lds_cap);
            a.acc_lds = pp.acc_lds;
            a.Ws = pp.Ws;
            a.k = k;
            a.gq = d_gq + g_first[k];
            a.ngq = ng;
            const size_t lds = pp.lds;
            for (int32_t ty = 0; ty < nb && e == hipSuccess; ty += 65535) {
                sc_py_args ac = a;
                ac.off = a.off + ty;
                ac.cidx = d_cidx + (int64_t)ty * (int64_t)totb;
                ac.dec = d_dec + (int64_t)ty * n_queries;
                ac.ycnt = d_ycnt + ty;
                // (lists and tp are indexed from the batch's first leaf: off[t] - off[0] of the chunk's own off)
                const int64_t shift = off[t0 + ty] - v.L0;
                ac.ylist = d_ylist + shift;
                ac.mm = c.d_mm + shift;
                k_py_sweep<<<dim3((unsigned)(ng * (k - 1)), (unsigned)std::min<int32_t>(nb - ty, 65535)), SC_THREADS,
                             lds, s>>>(ac);
                sc_launched(e);
            }
        }
    }
    if (e == hipSuccess && py_trees) e = hipMemcpyAsync(py_trees, d_trees, nq * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && py_total) e = hipMemcpyAsync(py_total, d_total, n_out * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && py_joint) e = hipMemcpyAsync(py_joint, d_joint, n_out * 8, hipMemcpyDeviceToHost, s);
    return sc_end(ctx, c, e, bad);
}

// the plans of scs_score_placements, scs_score_clade_placements / scs_score_clade_moves and scs_score_polytomies on the
// host, by the functions those exports call
extern "C" int scs_debug_placement_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                        int32_t super_leaves, int32_t max_batch_trees, int32_t max_lds_bytes,
                                        int32_t n_queries, int32_t n_sub_queries, int32_t n_degrees,
                                        const int32_t *degrees, int32_t *n_batches_out, int32_t *bstart_out,
                                        int64_t *pl_out, int64_t *cp_out, int64_t *blk_out, int64_t *py_out) {
    const char *const who = "scs_debug_placement_plan";
    SCS_REQUIRE(n_queries >= 1 && n_sub_queries >= 1 && n_degrees >= 0 && (n_degrees == 0 || degrees),
                "%s: no query, no sub-query or no degrees", who);
    size_t totb = 0;
    for (int32_t i = 0; i < n_degrees; ++i) {
        SCS_REQUIRE(degrees[i] >= 3 && degrees[i] <= PY_KMAX, "%s: degree %d is not in [3, %d]", who, degrees[i],
                    PY_KMAX);
        totb += (size_t)degrees[i] + 1;
    }
    const bool outs = pl_out && cp_out && blk_out && (py_out || n_degrees == 0);
    const size_t m1 = (size_t)std::max(n_trees, 0) + 1;
    const int lds_cap = sc_lds_cap(max_lds_bytes);
    const int counts[2] = {n_queries, n_sub_queries}, qmax[2] = {PL_QMAX, CP_QMAX};
    int64_t *const pair_out[2] = {pl_out, cp_out};
    for (int x = 0; x < 2; ++x) {
        const int qcap = std::min(counts[x], qmax[x]), q_last = counts[x] - (counts[x] - 1) / qcap * qcap;
        const sc_extras ex = x == 0 ? sc_pl_extras(qcap) : sc_cp_extras(qcap);
        sc_debug_plan d;
        SCS_TRY(sc_debug_batches(who, src, n_trees, tree_off, super_leaves, max_batch_trees, (int64_t)ex.per_leaf,
                                 (int64_t)ex.per_tree, max_lds_bytes, outs, n_batches_out ? n_batches_out + x : nullptr,
                                 bstart_out ? bstart_out + x * m1 : nullptr, d));
        const sc_pair_plan pl = sc_plan_pairs(d.off, d.bstart, sc_pl_rule(qcap, lds_cap));
        for (size_t b = 0; b + 1 < d.bstart.size(); ++b) {
            int64_t *o = pair_out[x] + 6 * b;
            o[0] = pl.words[b];
            o[1] = pl.zbs[b];
            o[2] = pl.sums[b];
            o[3] = (int64_t)sc_pl_lds(pl, b, qcap);
            o[4] = (int64_t)sc_pl_lds(pl, b, q_last);
            o[5] = pl.blk[d.bstart[b + 1]] - pl.blk[d.bstart[b]];
        }
        std::copy(pl.blk.begin(), pl.blk.end(), blk_out + x * m1);
    }
    const sc_extras ex = sc_py_extras(totb, (size_t)n_degrees);
    sc_debug_plan d;
    SCS_TRY(sc_debug_batches(who, src, n_trees, tree_off, super_leaves, max_batch_trees, (int64_t)ex.per_leaf,
                             (int64_t)ex.per_tree, max_lds_bytes, outs, n_batches_out ? n_batches_out + 2 : nullptr,
                             bstart_out ? bstart_out + 2 * m1 : nullptr, d));
    for (size_t b = 0; b + 1 < d.bstart.size(); ++b) {
        const int W = sc_py_words(sc_largest_tree(d.off, d.bstart[b], d.bstart[b + 1]));
        for (int32_t i = 0; i < n_degrees; ++i) {
            const sc_py_plan pp = sc_py_plan_of(W, degrees[i], lds_cap);
            int64_t *o = py_out + 4 * (b * (size_t)n_degrees + i);
            o[0] = pp.W;
            o[1] = pp.Ws;
            o[2] = pp.acc_lds;
            o[3] = (int64_t)pp.lds;
        }
    }
    return SCS_OK;
}

// ---- resampled and weighted branch triplet support (scs_score_branch_resample) ----
//
// rs_x[r][u] = sum_T w[r][T] bt_x(T, u) for the four counters x of section 18 and R rows of non-negative integer tree
// weights: row 0 the point estimate, rows 1 .. R - 1 replicates (a bootstrap or jackknife draw of the sources).  The
// sweep of section 18 runs once per batch and keeps its per-(tree, branch) terms:
//   k_rs_records / k_rs_pairs: bt_records<true> / bt_pairs<true>, plain stores into the batch's slab [tree][x][u];
//   k_rs_reduce: acc[x][r][u] += sum_t w[r][t] slab[t][x][u], one thread per (x, u) and tile of RS_TILE replicates in
//     registers, the slab read coalesced over u, a tree whose 64 entries are zero skipped by the wave, the tile's
//     weights in LDS (every lane reads the same address: a broadcast);
//   k_rs_wins: one thread per node decides every replicate and counts the four outcomes.

namespace {

constexpr int RS_TILE = 8;     // replicates a thread of k_rs_reduce accumulates
constexpr int RS_CHUNK = 512;  // trees whose weights a workgroup holds in LDS at a time (16 KiB)
constexpr int RS_AHEAD = 4;    // slab loads in flight per thread

// acc += w * v for 0 <= w < 2^31: a 32 x 32 -> 64 multiply-add on v's low word, a 32-bit one on its high word
__device__ __forceinline__ void rs_mad(unsigned long long &acc, uint32_t w, uint32_t lo, uint32_t hi) {
    acc += (unsigned long long)w * lo + ((unsigned long long)(w * hi) << 32);
}

// grid (node blocks x replicate tiles, 4): slab [nb][4][nn] of the batch, w = weights + t0 with row stride M
__global__ void __launch_bounds__(SC_THREADS) k_rs_reduce(const unsigned long long *__restrict__ slab, int nb,
                                                          int64_t nn, int n_ub, const int32_t *__restrict__ w,
                                                          int64_t M, int R, unsigned long long *__restrict__ acc) {
    __shared__ __attribute__((aligned(16))) uint32_t ws[RS_CHUNK][RS_TILE];
    const int64_t u = (int64_t)(blockIdx.x % n_ub) * SC_THREADS + threadIdx.x;
    const int r0 = (int)(blockIdx.x / n_ub) * RS_TILE, x = blockIdx.y;
    const bool in = u < nn;
    unsigned long long a[RS_TILE];
#pragma unroll
    for (int j = 0; j < RS_TILE; ++j) a[j] = 0;
    for (int c0 = 0; c0 < nb; c0 += RS_CHUNK) {
        const int nc = min(RS_CHUNK, nb - c0);
        __syncthreads();  // (the chunk before is read)
        for (int i = threadIdx.x; i < nc * RS_TILE; i += SC_THREADS) {
            const int j = i / nc, tt = i - j * nc;
            ws[tt][j] = r0 + j < R ? (uint32_t)w[(int64_t)(r0 + j) * M + c0 + tt] : 0u;
        }
        __syncthreads();
        const unsigned long long *p = slab + ((int64_t)c0 * 4 + x) * nn + (in ? u : 0);
        for (int tt = 0; tt < nc; tt += RS_AHEAD, p += RS_AHEAD * 4 * nn) {
            unsigned long long v[RS_AHEAD];
#pragma unroll
            for (int k = 0; k < RS_AHEAD; ++k) v[k] = in && tt + k < nc ? p[(int64_t)k * 4 * nn] : 0ull;
#pragma unroll
            for (int k = 0; k < RS_AHEAD; ++k) {
                if (__ballot(v[k] != 0) == 0) continue;  // (sparse sources: most (tree, 64 nodes) are empty)
                const uint32_t lo = (uint32_t)v[k], hi = (uint32_t)(v[k] >> 32);
                const uint32_t *wt = ws[min(tt + k, nc - 1)];
#pragma unroll
                for (int j = 0; j < RS_TILE; ++j) rs_mad(a[j], wt[j], lo, hi);
            }
        }
    }
    if (!in) return;
#pragma unroll
    for (int j = 0; j < RS_TILE; ++j)
        if (r0 + j < R) acc[((int64_t)x * R + r0 + j) * nn + u] += a[j];  // (one owner per entry, batches in order)
}

// one thread per node: every replicate r >= 1 with rs_total > 0 counts once, for the arrangement that is strictly
// greatest or as a tie; wins [4][nn] = concordant, alt1, alt2, tie
__global__ void __launch_bounds__(SC_THREADS) k_rs_wins(const unsigned long long *__restrict__ acc, int64_t nn, int R,
                                                        int32_t *__restrict__ wins) {
    const int64_t u = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (u >= nn) return;
    const int64_t row = (int64_t)R * nn;
    int32_t n_con = 0, n_a1 = 0, n_a2 = 0, n_tie = 0;
    for (int r = 1; r < R; ++r) {
        const unsigned long long *p = acc + (int64_t)r * nn + u;
        if (p[0] == 0) continue;
        const unsigned long long con = p[row], a1 = p[2 * row], a2 = p[3 * row];
        if (con > a1 && con > a2) ++n_con;
        else if (a1 > con && a1 > a2) ++n_a1;
        else if (a2 > con && a2 > a1) ++n_a2;
        else ++n_tie;
    }
    wins[u] = n_con;
    wins[nn + u] = n_a1;
    wins[2 * nn + u] = n_a2;
    wins[3 * nn + u] = n_tie;
}

}  // namespace

extern "C" int scs_score_branch_resample(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                         const int32_t *taxon, int32_t max_batch_trees, int32_t n_rep,
                                         const int32_t *weights, int64_t *rs_point, int32_t *rs_wins,
                                         int64_t *rs_rows) {
    const char *const who = "scs_score_branch_resample";
    SCS_REQUIRE(ctx && src && parent && taxon && weights && rs_point && rs_wins, "%s: null argument", who);
    SCS_REQUIRE(n_rep >= 1, "%s: n_rep = %d: at least row 0, the point estimate, is needed", who, n_rep);
    const int32_t M = src->n_trees;
    const std::vector<int64_t> &off = src->h_tree_off;
    // the three rows of one record of the largest tree must fit one workgroup's LDS (section 18)
    SCS_TRY(sc_rows_fit(who, src, BT_ROW_BYTES));
    // a row's entry is at most sum_t w[r][t] floor(m_t^3 / 27): it must fit int64 (the bound of sc_cubes_fit tree by
    // tree, each floored before its weight: not that sum)
    {
        std::vector<unsigned __int128> cube((size_t)M);
        for (int32_t t = 0; t < M; ++t) {
            const unsigned __int128 m = (unsigned __int128)(off[t + 1] - off[t]);
            cube[t] = m * m * m / 27;
        }
        for (int32_t r = 0; r < n_rep; ++r) {
            unsigned __int128 sum = 0;
            for (int32_t t = 0; t < M; ++t) {
                const int32_t wt = weights[(size_t)r * M + t];
                SCS_REQUIRE(wt >= 0, "%s: weights[%d][%d] = %d is negative", who, r, t, wt);
                sum += (unsigned __int128)wt * cube[t];
            }
            SCS_REQUIRE(sum <= (unsigned __int128)INT64_MAX,
                        "%s: the weighted triple counts of row %d may not fit 64 bits (the sum of weight x "
                        "leaves^3 / 27 over the %d source trees exceeds 2^63 - 1)", who, r, M);
        }
    }
    const size_t nn = (size_t)std::max(n_nodes, 0), mt = (size_t)M, R = (size_t)n_rep;
    SCS_REQUIRE((unsigned __int128)32 * R * nn <= SC_BUDGET,
                "%s: the accumulators of %d rows x %d nodes need %llu bytes, more than the %llu of the call's "
                "workspace", who, n_rep, n_nodes, (unsigned long long)(32 * R * nn), (unsigned long long)SC_BUDGET);
    // own arrays: the accumulators [4][R][nn], the wins [4][nn], the weights, the quartet-branch record per S node and
    // the first pair workgroup per tree (+ 1); per batch the lists of section 18 and the slab [tree][4][nn]
    unsigned long long *d_acc;
    int32_t *d_wins, *d_w, *d_qp;
    int64_t *d_blk;
    const auto own = [&](sc_carver w) {
        d_acc = w.take<unsigned long long>(4 * R * nn);
        d_wins = w.take<int32_t>(4 * nn);
        d_w = w.take<int32_t>(R * mt);
        d_qp = w.take<int32_t>(nn);
        d_blk = w.take<int64_t>(mt + 1);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, who, n_nodes, parent, taxon, max_batch_trees, own(sc_carver()).at,
                     16 + sizeof(sc_bt_rec), 8 + 32 * (uint64_t)nn, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_ylist = wb.take<int4>(c.max_lb);
    auto *d_recs = wb.take<sc_bt_rec>(c.max_lb);
    auto *d_ycnt = wb.take<int32_t>(2 * c.max_rows);
    auto *d_slab = wb.take<unsigned long long>(c.max_rows * 4 * nn);
    if (own(sc_carve_extra(c)).over || wb.over) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    hipStream_t s = ctx->stream;
    const std::vector<int32_t> q_parent = sc_quartet_parents(n_nodes, parent);
    // W, zb, the launch's LDS and blk per batch as in scs_score_branch_triplets
    const sc_pair_plan pl = sc_plan_pairs(off.data(), c.bstart, SC_BT_RULE);
    const int n_ub = grid_of((int64_t)nn), n_tiles = (n_rep + RS_TILE - 1) / RS_TILE;
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(d_qp, q_parent.data(), nn * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, weights, R * mt * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, 32 * R * nn, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk, pl.blk.data(), ((size_t)M + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_rs_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        e = hipMemsetAsync(d_ycnt, 0, (size_t)nb * 8, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_slab, 0, (size_t)nb * 32 * nn, s);
        if (e != hipSuccess) break;
        auto a = sc_args<sc_bt_args>(v);
        a.q_parent = d_qp;
        a.ylist = d_ylist;
        a.recs = d_recs;
        a.ycnt = d_ycnt;
        a.rcnt = d_ycnt + nb;
        a.n_tot = d_slab;
        a.c_tot = nullptr;
        a.nn = (int64_t)nn;
        k_rs_records<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        const int64_t n_wg = pl.blk[t0 + nb] - pl.blk[t0];
        if (n_wg > 0) {
            k_rs_pairs<<<(unsigned)n_wg, SC_THREADS, pl.lds[b], s>>>(d_blk + t0, nb, a.off, d_ylist, d_recs, a.ycnt,
                                                                     a.rcnt, c.d_mm, pl.zbs[b], pl.words[b], d_slab,
                                                                     (int64_t)nn, nullptr, nullptr);
            if (!sc_launched(e)) break;
        }
        k_rs_reduce<<<dim3((unsigned)n_ub * (unsigned)n_tiles, 4), SC_THREADS, 0, s>>>(d_slab, nb, (int64_t)nn, n_ub,
                                                                                      d_w + t0, (int64_t)M, n_rep,
                                                                                      d_acc);
        if (!sc_launched(e)) break;
    }
    if (e == hipSuccess && !bad) {
        k_rs_wins<<<n_ub, SC_THREADS, 0, s>>>(d_acc, (int64_t)nn, n_rep, d_wins);
        sc_launched(e);
    }
    for (size_t x = 0; x < 4 && e == hipSuccess; ++x)  // (row 0 of every counter)
        e = hipMemcpyAsync(rs_point + x * nn, d_acc + x * R * nn, nn * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(rs_wins, d_wins, nn * 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rs_rows) e = hipMemcpyAsync(rs_rows, d_acc, 32 * R * nn, hipMemcpyDeviceToHost, s);
    return sc_end(ctx, c, e, bad);
}

#include "scs_score_parsimony.h"
#include "scs_score_pairs.h"
#include "scs_score_pair_triplets.h"
#include "scs_score_coverage.h"
#include "scs_score_internode.h"
