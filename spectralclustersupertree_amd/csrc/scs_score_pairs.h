// scs_score_source_pairs: the Robinson-Foulds terms between every two source trees, each pair restricted to the taxa
// both trees hold.  Included by scs_score.hip after its shared host layer.  The export has no
// supertree, so it does not go through sc_begin: it plans its own tiles of the pair matrix and carves its own block.
//
// Per pair (A, B) -- A a row tree, B a column tree -- with L = L(A) ∩ L(B), c = |L|: common = c, clusters = |C(A|L)|,
// clusters_other = |C(B|L)|, shared = |C(A|L) ∩ C(B|L)|, C(X|L) the distinct sets cl(v) ∩ L of 2 <= size < c.
//   k_sp_scatter: dense position rows of a batch of trees, rowpos[A][taxon] = position in A or -1 (atomicCAS: a taxon
//                 twice in one tree is flagged, as in k_score_scatter).
//   k_sp_level:   levels >= 1 of a batch's min table of adj (level 0 is adj itself), for the two stretches and the
//                 range minima on either tree.
//   k_sp_pairs:   one workgroup per pair.  (1) every leaf q of B looks its taxon up in A's row: membership bitsets of
//                 A's and of B's positions, then the set bits before each word (rank = prefix + popc(bits & mask)).
//                 (2) the compact lists a[k] / bq[k] (A / B position of the k-th common leaf in A's order) and b[k]
//                 (B position of the k-th in B's order).  (3) from B's side one thread per restricted gap: its node is
//                 the run of gaps >= D around it; a first gap of a node with 2 <= size < c is a cluster of B|L.
//                 (4) min / max tables of bq over blocks of 64.  (5) the same from A's side, and the cluster [lo, hi]
//                 (ranks) is shared iff the B node above the B positions min .. max of bq[lo .. hi] holds exactly
//                 hi - lo + 1 common leaves.
// The lists hold POSITIONS, not depths: a position of a tree of fewer than 65 536 leaves fits 16 bits, a depth need
// not (a chain of unary nodes is as deep as it likes), so the B-LCA of a cluster is taken from its extreme B
// positions and one query on B's min table rather than from a range minimum over LCA depths.
// The arrays of a pair lie in LDS, or -- where they exceed the launch's bytes -- in a slab of the call's block that a
// persistent workgroup owns (template SLAB).

namespace {

constexpr int SP_SLAB_WGS = 256;                          // persistent workgroups of the slab launch, at most
constexpr uint64_t SP_SLAB_BYTES = (uint64_t)128 << 20;   // all slabs together (fewer workgroups for larger trees)
constexpr int64_t SP_GRID_MAX = (int64_t)1 << 30;         // workgroups of one launch at most, and ...
constexpr int64_t SP_ITEMS_MAX = ((int64_t)1 << 32) - 1;  // ... its work-items: the dispatch packet counts them in 32 bits
constexpr int SP_SCRATCH = 128;                           // LDS bytes ahead of a pair's arrays: wave sums, counters
constexpr int SP_THREADS_MAX = 1024;                      // threads of a pair workgroup at most (SC_THREADS at least)
constexpr int SP_WAVES_WANTED = 32;                       // waves a CU should hold: larger workgroups while the pairs'
                                                          // LDS leaves room for fewer

// where the arrays of one pair lie in its LDS block or slab (bytes from its start), for kernel and plan alike
struct sp_layout {
    uint32_t w_a, w_b;      // words of A's and of B's bitset (one more than the last position needs)
    uint32_t nblk, blev;    // blocks of 64 list entries at most, levels of the block tables (2^blev > nblk)
    uint64_t o_bits_a, o_pre_a, o_bits_b, o_pre_b, o_a, o_bq, o_b, o_tmin, o_tmax, bytes;
};

__host__ __device__ inline sp_layout sp_layout_of(int64_t n_a, int64_t n_b, int width) {
    sp_layout l;
    l.w_a = (uint32_t)(n_a >> 5) + 1;
    l.w_b = (uint32_t)(n_b >> 5) + 1;
    const uint64_t cm = (uint64_t)(n_a < n_b ? n_a : n_b);
    l.nblk = (uint32_t)(cm >> 6) + 1;
    l.blev = 1;
    while (((uint64_t)1 << l.blev) <= l.nblk) ++l.blev;
    uint64_t at = 0;
    l.o_bits_a = at, at += 4ull * l.w_a;
    l.o_pre_a = at, at += 4ull * l.w_a;
    l.o_bits_b = at, at += 4ull * l.w_b;
    l.o_pre_b = at, at += 4ull * l.w_b;
    l.o_a = at, at += cm * width;
    l.o_bq = at, at += cm * width;
    l.o_b = at, at += cm * width;
    at = (at + 3) & ~3ull;
    l.o_tmin = at, at += (uint64_t)l.blev * l.nblk * width;
    l.o_tmax = at, at += (uint64_t)l.blev * l.nblk * width;
    l.bytes = (at + 15) & ~15ull;
    return l;
}

struct sp_args {
    const int64_t *off;                  // tree_off of the tables (all trees)
    const int32_t *leaf_taxon, *adj;     // the tables' arrays (global leaf index)
    const int32_t *amin_r, *amin_c;      // levels >= 1 of the row / column batch's min table: level j at [(j - 1) * Lb]
    int64_t l0_r, lb_r, l0_c, lb_c;      // first leaf and leaves of the two batches
    int levels;
    const int32_t *rowpos;               // dense rows of the row batch
    int64_t row_stride;
    int32_t t0_r, t0_c, nb_c;            // first tree of the row batch; the column batch
    const int32_t *rl_row, *rl_tree;     // the rows of this launch: output row and tree
    int64_t n_pairs;                     // rows of the launch x nb_c
    int32_t M;
    int mirror;                          // rows = every tree in order: pairs A > B are skipped, A < B writes both cells
    uint32_t lds_bytes;                  // the LDS launch's bytes (SP_SCRATCH and a pair's arrays); a pair that
                                         // needs more is the slab launch's
    char *slab;
    int64_t slab_stride;
    int32_t *common, *clusters, *other, *shared;
};

template <bool SLAB, typename T>
__device__ __forceinline__ T sp_ld(const T *p) {
    if constexpr (SLAB) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

template <bool SLAB, typename T>
__device__ __forceinline__ void sp_st(T *p, T v) {
    if constexpr (SLAB) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

template <bool SLAB>
__device__ __forceinline__ void sp_sync() {
    if constexpr (SLAB) __threadfence();
    __syncthreads();
}

// set bits of the row below position pos (pos may be one past the last leaf: the row has a word for it)
template <bool SLAB>
__device__ __forceinline__ int sp_rank(const uint32_t *bits, const uint32_t *pre, int64_t pos) {
    const int64_t w = pos >> 5;
    return (int)(sp_ld<SLAB>(pre + w) + __popc(sp_ld<SLAB>(bits + w) & ((1u << (pos & 31)) - 1u)));
}

// pre[w] = set bits of the words before w; returns their total.  ws: one int of LDS per wave of the workgroup
template <bool SLAB>
__device__ __forceinline__ int sp_scan_bits(const uint32_t *bits, uint32_t *pre, int words, int *ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    const int nw = blockDim.x >> 6;
    for (int c0 = 0; c0 < words; c0 += blockDim.x) {
        const int w = c0 + threadIdx.x;
        const int cnt = w < words ? __popc(sp_ld<SLAB>(bits + w)) : 0;
        int incl = cnt;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        int before = carry, total = 0;
        for (int v = 0; v < nw; ++v) {
            before += v < wave ? ws[v] : 0;
            total += ws[v];
        }
        if (w < words) sp_st<SLAB>(pre + w, (uint32_t)(before + incl - cnt));
        carry += total;
        __syncthreads();
    }
    return carry;
}

// min of adj over the batch-relative gaps [l, r] (r >= l) of a batch's min table
__device__ __forceinline__ int32_t sp_adj_min(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin,
                                              int64_t Lb, int64_t l, int64_t r) {
    const int j = sc_log2(r - l + 1);
    // (level j of this table starts at amin + (j - 1) * Lb: sc_rmq_min is handed that level with stride 0, finds the
    // same j from r - l + 1 and reads tab[j * 0 + l] and tab[j * 0 + r - 2^j + 1] of it)
    return j == 0 ? adj[l] : sc_rmq_min(amin + (int64_t)(j - 1) * Lb, 0, l, r);
}

// the node of depth d above leaf pos of the tree at `base` (n leaves): its first and last leaf
__device__ __forceinline__ void sp_node(const int32_t *__restrict__ adj, const int32_t *__restrict__ amin, int64_t Lb,
                                        int levels, int64_t base, int64_t n, int64_t pos, int32_t d, int64_t &first,
                                        int64_t &last) {
    first = sc_stretch_left(adj, amin, Lb, levels, base, pos, d, true);
    last = sc_stretch_right(adj, amin, Lb, levels, base, pos, n - 1, d);
}

template <bool SLAB, typename E>
__device__ __forceinline__ void sp_pair(const sp_args &a, char *mem, const sp_layout &l, int r, int A, int B,
                                        int64_t n_a, int64_t n_b, int *ws) {
    uint32_t *bits_a = (uint32_t *)(mem + l.o_bits_a), *pre_a = (uint32_t *)(mem + l.o_pre_a);
    uint32_t *bits_b = (uint32_t *)(mem + l.o_bits_b), *pre_b = (uint32_t *)(mem + l.o_pre_b);
    E *la = (E *)(mem + l.o_a), *lbq = (E *)(mem + l.o_bq), *lb = (E *)(mem + l.o_b);
    E *tmin = (E *)(mem + l.o_tmin), *tmax = (E *)(mem + l.o_tmax);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p_a = a.off[A], p_b = a.off[B];
    const int32_t *row = a.rowpos + (int64_t)(A - a.t0_r) * a.row_stride;
    const int32_t *tax_b = a.leaf_taxon + p_b;
    // the two trees in their batches' tables
    const int32_t *adj_a = a.adj + a.l0_r, *adj_b = a.adj + a.l0_c;
    const int64_t base_a = p_a - a.l0_r, base_b = p_b - a.l0_c;
    const int threads = blockDim.x;
    int *cnt = ws + SP_THREADS_MAX / 64;  // clusters, clusters_other, shared

    // (1) membership
    for (uint32_t w = threadIdx.x; w < l.w_a; w += threads) sp_st<SLAB>(bits_a + w, 0u);
    for (uint32_t w = threadIdx.x; w < l.w_b; w += threads) sp_st<SLAB>(bits_b + w, 0u);
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    sp_sync<SLAB>();
    for (int64_t q = threadIdx.x; q < n_b; q += threads) {
        const int32_t pa = row[tax_b[q]];
        if (pa >= 0) {
            atomicOr(bits_b + (q >> 5), 1u << (q & 31));
            atomicOr(bits_a + (pa >> 5), 1u << (pa & 31));
        }
    }
    sp_sync<SLAB>();
    const int c = sp_scan_bits<SLAB>(bits_a, pre_a, (int)l.w_a, ws);
    sp_scan_bits<SLAB>(bits_b, pre_b, (int)l.w_b, ws);
    const int64_t cell = (int64_t)r * a.M + B, mirror = (int64_t)B * a.M + A;
    const bool both = a.mirror && A != B;
    if (c < 3) {  // (the three counts stay 0, as the call's memset left them)
        if (threadIdx.x == 0) {
            if (a.common) {
                a.common[cell] = c;
                if (both) a.common[mirror] = c;
            }
        }
        return;
    }
    sp_sync<SLAB>();
    // (2) the compact lists
    for (int64_t q = threadIdx.x; q < n_b; q += threads) {
        const int32_t pa = row[tax_b[q]];
        if (pa >= 0) {
            const int k = sp_rank<SLAB>(bits_a, pre_a, pa);
            sp_st<SLAB>(la + k, (E)pa);
            sp_st<SLAB>(lbq + k, (E)q);
            sp_st<SLAB>(lb + sp_rank<SLAB>(bits_b, pre_b, q), (E)q);
        }
    }
    sp_sync<SLAB>();
    // (3) the clusters of B|L: one thread per restricted gap
    int n_other = 0;
    for (int k0 = 0; k0 < c - 1; k0 += threads) {
        const int k = k0 + threadIdx.x;
        bool is = false;
        if (k < c - 1) {
            const int64_t p0 = sp_ld<SLAB>(lb + k), p1 = sp_ld<SLAB>(lb + k + 1);
            const int32_t d = sp_adj_min(adj_b, a.amin_c, a.lb_c, base_b + p0, base_b + p1 - 1);
            int64_t first, last;
            sp_node(adj_b, a.amin_c, a.lb_c, a.levels, base_b, n_b, p0, d, first, last);
            const int lo = sp_rank<SLAB>(bits_b, pre_b, first), hi = sp_rank<SLAB>(bits_b, pre_b, last + 1) - 1;
            if (hi - lo + 1 < c) {
                const int64_t pl = sp_ld<SLAB>(lb + lo);
                is = k == lo || sp_adj_min(adj_b, a.amin_c, a.lb_c, base_b + pl, base_b + p0 - 1) > d;
            }
        }
        n_other += __popcll(__ballot(is));
    }
    // (4) min and max of bq over blocks of 64 entries, one wave per block, and the levels above
    const int nblk = ((c - 1) >> 6) + 1;
    for (int b = wave; b < nblk; b += threads >> 6) {
        const int k = 64 * b + lane;
        uint32_t mn = k < c ? (uint32_t)sp_ld<SLAB>(lbq + k) : 0xffffffffu, mx = k < c ? (uint32_t)sp_ld<SLAB>(lbq + k) : 0u;
        for (int d = 32; d >= 1; d >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        }
        if (lane == 0) {
            sp_st<SLAB>(tmin + b, (E)mn);
            sp_st<SLAB>(tmax + b, (E)mx);
        }
    }
    sp_sync<SLAB>();
    for (int j = 1; (1 << j) <= nblk; ++j) {
        const int half = 1 << (j - 1);
        const E *pmin = tmin + (size_t)(j - 1) * l.nblk, *pmax = tmax + (size_t)(j - 1) * l.nblk;
        for (int b = threadIdx.x; b < nblk; b += threads) {
            E mn = sp_ld<SLAB>(pmin + b), mx = sp_ld<SLAB>(pmax + b);
            if (b + half < nblk) {
                mn = min(mn, sp_ld<SLAB>(pmin + b + half));
                mx = max(mx, sp_ld<SLAB>(pmax + b + half));
            }
            sp_st<SLAB>(tmin + (size_t)j * l.nblk + b, mn);
            sp_st<SLAB>(tmax + (size_t)j * l.nblk + b, mx);
        }
        sp_sync<SLAB>();
    }
    // (5) the clusters of A|L, and which of them B|L has
    int n_clusters = 0, n_shared = 0;
    for (int k0 = 0; k0 < c - 1; k0 += threads) {
        const int k = k0 + threadIdx.x;
        bool is = false, sh = false;
        if (k < c - 1) {
            const int64_t p0 = sp_ld<SLAB>(la + k), p1 = sp_ld<SLAB>(la + k + 1);
            const int32_t d = sp_adj_min(adj_a, a.amin_r, a.lb_r, base_a + p0, base_a + p1 - 1);
            int64_t first, last;
            sp_node(adj_a, a.amin_r, a.lb_r, a.levels, base_a, n_a, p0, d, first, last);
            const int lo = sp_rank<SLAB>(bits_a, pre_a, first), hi = sp_rank<SLAB>(bits_a, pre_a, last + 1) - 1;
            const int s = hi - lo + 1;
            if (s < c) {
                const int64_t pl = sp_ld<SLAB>(la + lo);
                is = k == lo || sp_adj_min(adj_a, a.amin_r, a.lb_r, base_a + pl, base_a + p0 - 1) > d;
            }
            if (is) {
                // the extreme B positions of the cluster's leaves
                uint32_t mn = 0xffffffffu, mx = 0;
                const int bl = lo >> 6, bh = hi >> 6;
                const int e0 = bl == bh ? hi : 64 * bl + 63;
                for (int i = lo; i <= e0; ++i) {
                    const uint32_t v = sp_ld<SLAB>(lbq + i);
                    mn = min(mn, v);
                    mx = max(mx, v);
                }
                if (bh > bl) {
                    for (int i = 64 * bh; i <= hi; ++i) {
                        const uint32_t v = sp_ld<SLAB>(lbq + i);
                        mn = min(mn, v);
                        mx = max(mx, v);
                    }
                    if (bh - bl > 1) {
                        const int x = bl + 1, y = bh - 1, j = sc_log2(y - x + 1);
                        const E *pmin = tmin + (size_t)j * l.nblk, *pmax = tmax + (size_t)j * l.nblk;
                        mn = min(mn, (uint32_t)min(sp_ld<SLAB>(pmin + x), sp_ld<SLAB>(pmin + y - (1 << j) + 1)));
                        mx = max(mx, (uint32_t)max(sp_ld<SLAB>(pmax + x), sp_ld<SLAB>(pmax + y - (1 << j) + 1)));
                    }
                }
                // the B node above them holds the cluster and nothing else of L
                const int32_t dx = sp_adj_min(adj_b, a.amin_c, a.lb_c, base_b + mn, base_b + (int64_t)mx - 1);
                sp_node(adj_b, a.amin_c, a.lb_c, a.levels, base_b, n_b, (int64_t)mn, dx, first, last);
                sh = sp_rank<SLAB>(bits_b, pre_b, last + 1) - sp_rank<SLAB>(bits_b, pre_b, first) == s;
            }
        }
        n_clusters += __popcll(__ballot(is));
        n_shared += __popcll(__ballot(sh));
    }
    if (lane == 0) {
        atomicAdd(cnt + 0, n_clusters);
        atomicAdd(cnt + 1, n_other);
        atomicAdd(cnt + 2, n_shared);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t v[4] = {c, cnt[0], cnt[1], cnt[2]};
        int32_t *const outs[4] = {a.common, a.clusters, a.other, a.shared};
        for (int i = 0; i < 4; ++i) {
            if (!outs[i]) continue;
            outs[i][cell] = v[i];
            if (both) outs[i][mirror] = v[i == 1 ? 2 : i == 2 ? 1 : i];
        }
    }
}

// SLAB false: one workgroup per pair, the pairs that fit a.lds_bytes; true: persistent workgroups, each with its own
// slab, over the pairs that do not
template <bool SLAB, typename E>
__global__ void __launch_bounds__(SP_THREADS_MAX) k_sp_pairs(sp_args a) {
    extern __shared__ __align__(16) char sp_lds[];
    int *ws = (int *)sp_lds;  // SP_SCRATCH bytes
    for (int64_t idx = blockIdx.x; idx < a.n_pairs; idx += gridDim.x) {
        const int i = (int)(idx / a.nb_c), j = (int)(idx % a.nb_c);
        const int r = a.rl_row[i], A = a.rl_tree[i], B = a.t0_c + j;
        if (a.mirror && A > B) continue;
        const int64_t n_a = a.off[A + 1] - a.off[A], n_b = a.off[B + 1] - a.off[B];
        const sp_layout l = sp_layout_of(n_a, n_b, (int)sizeof(E));
        if ((l.bytes + SP_SCRATCH <= a.lds_bytes) == SLAB) continue;
        __syncthreads();  // (the last pair's counters have been read)
        if constexpr (SLAB) sp_pair<true, E>(a, a.slab + (int64_t)blockIdx.x * a.slab_stride, l, r, A, B, n_a, n_b, ws);
        else sp_pair<false, E>(a, sp_lds + SP_SCRATCH, l, r, A, B, n_a, n_b, ws);
    }
}

// dense position rows of the trees [t0, t0 + nb): flags 1 a taxon out of range, 4 a taxon twice in one tree
__global__ void k_sp_scatter(const int64_t *__restrict__ off, int nb, const int32_t *__restrict__ leaf_taxon,
                             int32_t n_taxa, int32_t *__restrict__ rows, int64_t row_stride,
                             unsigned *__restrict__ flags) {
    const int64_t p = off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    const int32_t x = leaf_taxon[p];
    if (x < 0 || x >= n_taxa) {
        atomicOr(flags, 1u);
        return;
    }
    if (atomicCAS(rows + (int64_t)t * row_stride + x, -1, (int32_t)(p - off[t])) != -1) atomicOr(flags, 4u);
}

// level j of an int32 min table from level j - 1 (k_score_level_tree without the min-max table this export has no
// use for: 8 bytes a leaf and level)
__global__ void k_sp_level(const int32_t *__restrict__ prev, int32_t *__restrict__ cur, int64_t n, int64_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t d = prev[i];
    cur[i] = (i + half < n) ? min(d, prev[i + half]) : d;
}

// The plan of a call: the tree batches (both axes of the pair matrix are tiled by them), the slabs, the bytes.
struct sp_plan {
    int levels = 1;
    int64_t row_stride = 0, max_lb = 0, max_nb = 0;
    int lds_cap = 0;
    int threads = 0;          // probe switch SCS_SP_THREADS: every pair workgroup that size (0: by the tile's LDS)
    int64_t slab_stride = 0;  // 0: no pair needs a slab
    int slab_wgs = 0;
    std::vector<int32_t> bstart;
    std::vector<int64_t> largest;  // per batch
};

// the workgroups a launch of that workgroup size may have
int64_t sp_grid_limit(int threads) { return std::min<int64_t>(SP_GRID_MAX, SP_ITEMS_MAX / threads); }

// a tile (row batch I, column batch J): entry width, the bytes its largest pair needs (SP_SCRATCH and the arrays), the
// LDS bytes of the launch, whether the slab launch is made
struct sp_tile {
    int width, threads;
    uint64_t need, lds;
    bool slab;
};

sp_tile sp_tile_of(const sp_plan &p, size_t I, size_t J) {
    sp_tile t;
    t.width = std::max(p.largest[I], p.largest[J]) < 65536 ? 2 : 4;
    t.need = sp_layout_of(p.largest[I], p.largest[J], t.width).bytes + SP_SCRATCH;
    t.slab = t.need > (uint64_t)p.lds_cap;
    t.lds = std::max<uint64_t>(std::min<uint64_t>(t.need, (uint64_t)p.lds_cap), SP_SCRATCH);  // (a cap below the scratch)
    // the pairs are bound by the latency of the descents on the min tables: where their LDS leaves a CU room for few
    // workgroups, each brings more waves
    t.threads = p.threads ? p.threads : SC_THREADS;
    while (!p.threads && t.threads < SP_THREADS_MAX && (TP_LDS_MAX / t.lds) * (t.threads / 64) < SP_WAVES_WANTED)
        t.threads *= 2;
    return t;
}

// batches by bytes against SC_BUDGET less the slabs: per tree its dense row and twice its min-table levels (it serves
// as a row and as a column tree); a batch ends before the tree that would take it past that, or at max_batch_trees
sp_plan sp_plan_of(const int64_t *off, int32_t M, int64_t max_leaves, int32_t n_taxa, int32_t max_batch_trees,
                   int32_t max_lds_bytes) {
    sp_plan p;
    p.levels = sc_levels_host(std::max<int64_t>(max_leaves, 1));
    p.row_stride = scs_round_up(std::max<int64_t>(n_taxa, 1), 64);
    p.lds_cap = sc_lds_cap(max_lds_bytes);
    if (const char *e = scs_dbg("SCS_SP_THREADS")) {
        const int t = atoi(e);
        if (t == 256 || t == 512 || t == 1024) p.threads = t;
    }
    const int width = max_leaves < 65536 ? 2 : 4;
    const uint64_t need = sp_layout_of(max_leaves, max_leaves, width).bytes;
    if (need + SP_SCRATCH > (uint64_t)p.lds_cap) {
        p.slab_stride = (int64_t)sc_up256(need);
        p.slab_wgs = (int)std::min<uint64_t>(SP_SLAB_WGS, std::max<uint64_t>(1, SP_SLAB_BYTES / p.slab_stride));
    }
    const uint64_t slabs = (uint64_t)p.slab_stride * p.slab_wgs;
    const uint64_t budget = SC_BUDGET > slabs ? SC_BUDGET - slabs : 0;
    const auto per_tree = [&](int32_t t) {
        return (uint64_t)p.row_stride * 4 + (uint64_t)(off[t + 1] - off[t]) * 8 * (p.levels - 1);
    };
    p.bstart.assign(1, 0);
    uint64_t acc = 0;
    for (int32_t t = 0; t < M; ++t) {
        const int32_t nb = t - p.bstart.back();
        if (nb > 0 && (acc + per_tree(t) > budget || (max_batch_trees > 0 && nb >= max_batch_trees))) {
            p.bstart.push_back(t);
            acc = 0;
        }
        acc += per_tree(t);
    }
    p.bstart.push_back(M);
    for (size_t b = 0; b + 1 < p.bstart.size(); ++b) {
        p.largest.push_back(sc_largest_tree(off, p.bstart[b], p.bstart[b + 1]));
        p.max_lb = std::max(p.max_lb, off[p.bstart[b + 1]] - off[p.bstart[b]]);
        p.max_nb = std::max<int64_t>(p.max_nb, p.bstart[b + 1] - p.bstart[b]);
    }
    return p;
}

// the block of a call: flag, row lists, outputs, slabs, the dense rows and the two batches' table levels
struct sp_block {
    unsigned *flag;
    int32_t *rl_row, *rl_tree, *out, *rowpos, *amin_r, *amin_c;
    char *slab;
};

// (n_out: the output matrices the caller asked for; the others get no room)
size_t sp_carve(sc_carver &w, const sp_plan &p, size_t n_rows, size_t M, size_t n_out, sp_block &k) {
    const size_t lev = (size_t)std::max(p.levels - 1, 1);
    k.flag = w.take<unsigned>(1);
    k.rl_row = w.take<int32_t>(n_rows);
    k.rl_tree = w.take<int32_t>(n_rows);
    k.out = w.take<int32_t>(n_out * n_rows * M);
    k.slab = w.take<char>((size_t)p.slab_stride * p.slab_wgs);
    k.rowpos = w.take<int32_t>((size_t)p.max_nb * p.row_stride);
    k.amin_r = w.take<int32_t>((size_t)p.max_lb * lev);
    k.amin_c = w.take<int32_t>((size_t)p.max_lb * lev);
    return w.at;
}

template <bool SLAB>
void sp_launch(const sp_args &a, int width, unsigned grid, int threads, size_t lds, hipStream_t s) {
    if (width == 2) k_sp_pairs<SLAB, uint16_t><<<grid, threads, lds, s>>>(a);
    else k_sp_pairs<SLAB, uint32_t><<<grid, threads, lds, s>>>(a);
}

}  // namespace

extern "C" int scs_score_source_pairs(scs_ctx *ctx, const scs_tables *src, int32_t n_rows, const int32_t *rows,
                                      int32_t max_batch_trees, int32_t max_lds_bytes, int32_t *common,
                                      int32_t *clusters, int32_t *clusters_other, int32_t *shared) {
    const char *const who = "scs_score_source_pairs";
    SCS_REQUIRE(ctx && src, "%s: null argument", who);
    const int32_t M = src->n_trees;
    SCS_REQUIRE(n_rows >= 0, "%s: n_rows = %d is negative", who, n_rows);
    SCS_REQUIRE(rows || n_rows == M, "%s: rows is null and n_rows = %d is not the %d trees of the tables", who, n_rows,
                M);
    SCS_REQUIRE(max_lds_bytes >= 0, "%s: max_lds_bytes = %d is negative", who, max_lds_bytes);
    for (int32_t r = 0; r < n_rows && rows; ++r)
        SCS_REQUIRE(rows[r] >= 0 && rows[r] < M, "%s: rows[%d] = %d is not a tree of the tables (%d trees)", who, r,
                    rows[r], M);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    if (n_rows == 0 || M == 0) return SCS_OK;
    const std::vector<int64_t> &off = src->h_tree_off;
    const sp_plan p = sp_plan_of(off.data(), M, src->max_leaves, src->n_taxa, max_batch_trees, max_lds_bytes);
    const size_t n_batches = p.bstart.size() - 1;
    // the rows by the batch of their tree (a batch's rows are one run of the lists)
    std::vector<int32_t> batch_of((size_t)M), rl_row, rl_tree;
    std::vector<size_t> rl_start(n_batches + 1, 0);
    for (size_t b = 0; b < n_batches; ++b)
        for (int32_t t = p.bstart[b]; t < p.bstart[b + 1]; ++t) batch_of[t] = (int32_t)b;
    for (int32_t r = 0; r < n_rows; ++r) rl_start[batch_of[rows ? rows[r] : r] + 1]++;
    for (size_t b = 0; b < n_batches; ++b) rl_start[b + 1] += rl_start[b];
    rl_row.resize((size_t)n_rows);
    rl_tree.resize((size_t)n_rows);
    {
        std::vector<size_t> at(rl_start.begin(), rl_start.end() - 1);
        for (int32_t r = 0; r < n_rows; ++r) {
            const int32_t t = rows ? rows[r] : r;
            rl_row[at[batch_of[t]]] = r;
            rl_tree[at[batch_of[t]]++] = t;
        }
    }
    sp_block k;
    sc_carver sizing;
    int32_t *const outs[4] = {common, clusters, clusters_other, shared};
    size_t n_out = 0;
    for (int i = 0; i < 4; ++i) n_out += outs[i] != nullptr;
    const size_t bytes = sp_carve(sizing, p, (size_t)n_rows, (size_t)M, n_out, k);
    void *block = nullptr;
    SCS_TRY(scs_block_alloc(ctx, bytes, &block));
    sc_carver carve{(char *)block, bytes};
    sp_carve(carve, p, (size_t)n_rows, (size_t)M, n_out, k);
    // the matrices asked for lie one after the other
    int32_t *d_outs[4];
    for (size_t i = 0, at = 0; i < 4; ++i) d_outs[i] = outs[i] ? k.out + at++ * (size_t)n_rows * M : nullptr;
    hipStream_t s = ctx->stream;
    const size_t cells = (size_t)n_rows * M;
    unsigned bad = 0;
    hipError_t e = hipMemsetAsync(k.flag, 0, 4, s);
    if (e == hipSuccess && n_out) e = hipMemsetAsync(k.out, 0, n_out * cells * 4, s);
    if (e == hipSuccess) e = hipMemcpyAsync(k.rl_row, rl_row.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(k.rl_tree, rl_tree.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    // the dense rows of batch b; its table levels into `amin`
    const auto scatter = [&](size_t b) {
        const int32_t t0 = p.bstart[b], nb = p.bstart[b + 1] - t0;
        e = hipMemsetAsync(k.rowpos, 0xff, (size_t)nb * p.row_stride * 4, s);
        if (e != hipSuccess) return;
        k_sp_scatter<<<grid_of(off[t0 + nb] - off[t0]), SC_THREADS, 0, s>>>(src->d_tree_off + t0, nb, src->d_leaf_taxon,
                                                                          src->n_taxa, k.rowpos, p.row_stride, k.flag);
        sc_launched(e);
    };
    const auto levels_of = [&](size_t b, int32_t *amin) {
        const int64_t l0 = off[p.bstart[b]], lb = off[p.bstart[b + 1]] - l0;
        for (int j = 1; j < p.levels && e == hipSuccess; ++j) {
            k_sp_level<<<grid_of(lb), SC_THREADS, 0, s>>>(j == 1 ? src->d_adj_depth + l0 : amin + (int64_t)(j - 2) * lb,
                                                          amin + (int64_t)(j - 1) * lb, lb, (int64_t)1 << (j - 1));
            sc_launched(e);
        }
    };
    // every tree's taxa are checked before a pair kernel reads a row by them: one scatter of every batch
    for (size_t b = 0; b < n_batches && e == hipSuccess; ++b) scatter(b);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, k.flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const bool mirror = rows == nullptr;
    // (the attribute is per function and device: set on every call)
    const void *const fns[4] = {(const void *)k_sp_pairs<false, uint16_t>, (const void *)k_sp_pairs<false, uint32_t>,
                                (const void *)k_sp_pairs<true, uint16_t>, (const void *)k_sp_pairs<true, uint32_t>};
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
        e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    for (size_t I = 0; I < n_batches && e == hipSuccess && !bad; ++I) {
        const size_t n_rl = rl_start[I + 1] - rl_start[I];
        if (n_rl == 0) continue;
        if (n_batches > 1) scatter(I);  // (one batch: the rows of the check are this batch's)
        levels_of(I, k.amin_r);
        for (size_t J = mirror ? I : 0; J < n_batches && e == hipSuccess; ++J) {
            if (J != I) levels_of(J, k.amin_c);
            if (e != hipSuccess) break;
            const sp_tile tile = sp_tile_of(p, I, J);
            sp_args a{};
            a.off = src->d_tree_off;
            a.leaf_taxon = src->d_leaf_taxon;
            a.adj = src->d_adj_depth;
            a.amin_r = k.amin_r;
            a.amin_c = J == I ? k.amin_r : k.amin_c;
            a.l0_r = off[p.bstart[I]];
            a.lb_r = off[p.bstart[I + 1]] - a.l0_r;
            a.l0_c = off[p.bstart[J]];
            a.lb_c = off[p.bstart[J + 1]] - a.l0_c;
            a.levels = p.levels;
            a.rowpos = k.rowpos;
            a.row_stride = p.row_stride;
            a.t0_r = p.bstart[I];
            a.t0_c = p.bstart[J];
            a.nb_c = p.bstart[J + 1] - p.bstart[J];
            a.M = M;
            a.mirror = mirror;
            a.lds_bytes = (uint32_t)tile.lds;
            a.slab = k.slab;
            a.slab_stride = p.slab_stride;
            a.common = d_outs[0];
            a.clusters = d_outs[1];
            a.other = d_outs[2];
            a.shared = d_outs[3];
            // a launch holds as many rows of the tile as keep its grid under the limit of its workgroup size; the
            // kernel strides over its grid, so a single row of more cells than that is capped, not refused
            const int64_t limit = sp_grid_limit(tile.threads);
            const size_t per = (size_t)std::max<int64_t>(limit / a.nb_c, 1);
            for (size_t r0 = 0; r0 < n_rl && e == hipSuccess; r0 += per) {
                const size_t nr = std::min(per, n_rl - r0);
                a.rl_row = k.rl_row + rl_start[I] + r0;
                a.rl_tree = k.rl_tree + rl_start[I] + r0;
                a.n_pairs = (int64_t)nr * a.nb_c;
                sp_launch<false>(a, tile.width, (unsigned)std::min(a.n_pairs, limit), tile.threads, (size_t)tile.lds, s);
                if (!sc_launched(e)) break;
                if (tile.slab) {
                    // (a slab pair is a large one, and a CU holds one persistent workgroup: the most waves)
                    sp_launch<true>(a, tile.width, (unsigned)std::min<int64_t>(p.slab_wgs, a.n_pairs),
                                    p.threads ? p.threads : SP_THREADS_MAX, SP_SCRATCH, s);
                    sc_launched(e);
                }
            }
        }
    }
    for (int i = 0; i < 4 && e == hipSuccess && !bad; ++i)
        if (outs[i]) e = hipMemcpyAsync(outs[i], d_outs[i], cells * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipStreamSynchronize(s);  // (nothing may still write into the block)
    scs_block_release(ctx, block);
    if (e != hipSuccess) {
        scs_set_error("%s: %s", who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCS_ENOMEM : SCS_EHIP;
    }
    SCS_REQUIRE(!bad, "%s: %s", who,
                (bad & 1u) ? "a leaf_taxon entry is out of range [0, n_taxa)" : "a source tree has a taxon twice");
    return SCS_OK;
}

// the plan of one scs_score_source_pairs call on the host, by the functions the export calls
extern "C" int scs_debug_source_pairs_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                           int32_t n_taxa, int32_t n_rows, int32_t max_batch_trees,
                                           int32_t max_lds_bytes, int32_t *n_batches_out, int32_t *bstart_out,
                                           int64_t *info_out, int64_t *tile_out) {
    const char *const who = "scs_debug_source_pairs_plan";
    SCS_REQUIRE((src || tree_off) && n_batches_out && bstart_out && info_out, "%s: null argument", who);
    SCS_REQUIRE(!src || n_trees == src->n_trees, "%s: the tables hold %d trees, not %d", who, src ? src->n_trees : 0,
                n_trees);
    SCS_REQUIRE(n_trees >= 0 && n_taxa >= 0 && n_rows >= 0 && max_lds_bytes >= 0, "%s: negative argument", who);
    const int64_t *off = src ? src->h_tree_off.data() : tree_off;
    int64_t max_leaves = src ? src->max_leaves : 0;
    if (!src)
        for (int32_t t = 0; t < n_trees; ++t) {
            SCS_REQUIRE(off[t + 1] >= off[t], "%s: tree_off decreases at tree %d", who, t);
            max_leaves = std::max(max_leaves, off[t + 1] - off[t]);
        }
    const sp_plan p = sp_plan_of(off, n_trees, max_leaves, src ? src->n_taxa : n_taxa, max_batch_trees, max_lds_bytes);
    const size_t nb = p.bstart.size() - 1;
    *n_batches_out = (int32_t)nb;
    std::copy(p.bstart.begin(), p.bstart.end(), bstart_out);
    sp_block k;
    sc_carver sizing;
    const int64_t info[6] = {p.levels, p.row_stride, p.slab_stride, p.slab_wgs,
                             (int64_t)sp_carve(sizing, p, (size_t)n_rows, (size_t)n_trees, 4, k), p.lds_cap};
    std::copy(info, info + 6, info_out);
    for (size_t I = 0; I < nb && tile_out; ++I)
        for (size_t J = 0; J < nb; ++J) {
            const sp_tile t = sp_tile_of(p, I, J);
            const int64_t limit = sp_grid_limit(t.threads), nb_c = p.bstart[J + 1] - p.bstart[J];
            const int64_t row[7] = {t.width, (int64_t)t.lds, t.slab, (int64_t)t.need, t.threads, limit,
                                    std::max<int64_t>(limit / std::max<int64_t>(nb_c, 1), 1)};
            std::copy(row, row + 7, tile_out + 7 * (I * nb + J));
        }
    return SCS_OK;
}
