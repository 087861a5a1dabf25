// scs_score_internode: the internode distances of the sources, summed per pair of taxa.
// Included by scs_score.hip after its shared host layer.  Like scs_score_source_pairs and scs_score_coverage the
// export has no supertree, so it does not go through sc_begin: it plans its own batches and carves its own block.
//
// `sources` are tables as for scs_score_source_pairs.  Only `tree_off`, `leaf_taxon` and `adj_depth` are read.
// n = the tables' `n_taxa`.
//   T* is the tree of T's distinct clusters: gaps of equal adj_depth with no shallower gap between them are one node
//   (so a polytomy is one node), and a node with one child is no node (the tables cannot see it).
//   r(gap) = the number of distinct nodes strictly above the gap's node: 0 at the top node, whatever its adj_depth;
//   the parent of a node is the node of the deeper of the two nearest strictly shallower gaps, left and right.
//   depth(leaf) = 1 + r of the deeper of its two neighbouring gaps (its only one at a tree's end).
//   d_T(a, b), a != b both in T, = depth(a) + depth(b) - 2 min r over the gaps between them: the edges between the
//   two leaves in T*.  A cherry gives 2, ((a,b),c) gives d(a,c) = 3, a star gives 2 everywhere.  d_T is taken in T
//   itself, not in a restriction.
//   `tree_w`: non-negative int64 per tree, NULL = 1; a tree of weight w counts like w copies, weight 0 as absent.
// For the row taxa r, given as `rows` (ids in any order, repeats allowed; NULL means every taxon, and then `n_rows`
// must be n), all int64 and exact, n_rows x n row-major with diagonal 0:
//   `pair_weight[r][b]` = Σ w_t over the trees that hold both,  `dist_sum[r][b]` = Σ w_t d_t(a, b),
//   `sq_sum[r][b]` = Σ w_t d_t(a, b)²;  `taxon_weight[r]`, `taxon_sum[r]`, `taxon_sq[r]` their row sums and
//   `taxon_partners[r]` (int32) = #{b : pair_weight > 0}.  Any output may be null.
// Overflow is decided on the host after the depth pass, before any sweep, from the largest leaf depth h_t per tree
// (m_t leaves): B1 = Σ w_t (m_t - 1) 2h_t and, when a squared output is asked for, B2 = Σ w_t (m_t - 1) (2h_t)²
// bound every cell and every row sum; one above 2^63 - 1 is SCS_EINVAL.
//
//   k_in_links:   one thread per gap: its parent gap, by the binary descents of k_trip_nodes on the batch's min table
//                 of adj_depth (the first gap of its node to the left, the end of the node to the right, the deeper of
//                 the two gaps that bound it), packed (parent << 32 | 1); the top node's gaps are (DONE | 0).
//   k_in_jump:    one round of pointer doubling over the links, from one buffer into the other; after
//                 ceil(log2 height) rounds every entry is (DONE | r).
//   k_in_depths:  r per gap into level 0 of the batch's table, the leaf depths, and h_t (wave max, one atomic each).
//   k_sp_level:   the levels above, as in section 33.
//   k_in_scatter: dense rows per tree of the batch, rowpd[t][taxon] = (position | depth << 32) or all ones
//                 (atomicCAS: a taxon twice in one tree is flagged, as k_sp_scatter does), and the membership bits
//                 word-major `bitsT[tree / 32][taxon]` of the trees of weight > 0 (as k_cv_scatter does).
//   k_in_sweep:   one workgroup per (row taxon a, group of tiles of 256 taxa b); a lane owns one b.  Per chunk of
//                 1024 trees the positions, depths, table bases and weights of a are staged in LDS (a tree's row is
//                 read only where a's bit is set); the lane walks the set bits of M[a] & M[b] and makes one gather of
//                 rowpd[t][b] and two of t's table at level 31 - clz(gaps).  Sums in int64 registers, cells written
//                 only when matrices are wanted (both cells with `mirror`), the row totals by a wave reduction and one
//                 atomic per wave and item.
//   k_in_partners: taxon_partners over all trees' bits, where the trees go in more than one batch (with one batch the
//                 sweep counts them).

namespace {

constexpr int IN_TILE = SC_THREADS;   // taxa b of one pass of a workgroup: one per thread
constexpr int IN_CHUNK_WORDS = 32;    // words of trees whose data of taxon a a workgroup stages at a time
constexpr int IN_CHUNK = 32 * IN_CHUNK_WORDS;
constexpr int64_t IN_ITEMS_WANTED = 8192;  // work items of a call the tile groups aim at
constexpr uint32_t IN_DONE = 0xffffffffu;
constexpr unsigned long long IN_EMPTY = ~0ull;

struct in_args {
    const int32_t *rows;   // row taxa of the call (null: row r is taxon r)
    int64_t r0;            // first row of the launch
    int64_t n_items;       // rows of the launch x ng
    int32_t n, nt, tg, ng; // taxa; tiles of a row; tiles of a group; groups of a row
    int64_t n_pad;         // stride of a row of rowpd and of bitsT
    int32_t t0, t1;        // the trees of the batch
    const int64_t *off;    // tree_off of the tables (all trees)
    int64_t l0, Lb;        // first leaf and leaves of the batch
    const unsigned long long *rowpd;
    const uint32_t *bitsT;
    const int32_t *tab;    // level j of the batch's min table of r at [j * Lb]
    const int32_t *ldep;
    const int64_t *w;      // per tree of the tables, or null
    int mirror, count_partners;
    int64_t out_r0;        // first row the matrices of this batch hold
    unsigned long long *c_w, *c_d, *c_q;  // the batch's rows x n, or null
    unsigned long long *s_w, *s_d, *s_q;  // per row of the call
    int32_t *partners;
};

__device__ __forceinline__ unsigned long long in_wave_sum(unsigned long long v) {
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned long long)__shfl_xor((long long)v, d, 64);
    return v;
}

__global__ void __launch_bounds__(SC_THREADS) k_in_sweep(in_args a) {
    __shared__ int32_t s_pa[IN_CHUNK], s_da[IN_CHUNK], s_base[IN_CHUNK];
    __shared__ long long s_wt[IN_CHUNK];
    __shared__ uint32_t s_ma[IN_CHUNK_WORDS];
    const int lane = threadIdx.x & 63;
    const int32_t w_lo = a.t0 >> 5, w_hi = (a.t1 - 1) >> 5;  // the batch's words of bitsT (t1 > t0)
    const int n_chunks = (w_hi - w_lo) / IN_CHUNK_WORDS + 1;
    for (int64_t idx = blockIdx.x; idx < a.n_items; idx += gridDim.x) {
        const int64_t ri = a.r0 + idx / a.ng;
        const int32_t tile0 = (int32_t)(idx % a.ng) * a.tg;
        const int32_t ta = a.rows ? a.rows[ri] : (int32_t)ri;
        unsigned long long tw = 0, td = 0, tq = 0;
        int tp = 0;
        bool staged = false;
        for (int32_t tile = tile0; tile < min(tile0 + a.tg, a.nt); ++tile) {
            const int32_t b0 = tile * IN_TILE;
            if (a.mirror && b0 + IN_TILE - 1 <= ta) continue;  // (left to the rows of the tile's taxa)
            const int32_t b = b0 + (int32_t)threadIdx.x;
            const bool act = b < a.n && b != ta && (!a.mirror || b > ta);
            unsigned long long sw = 0, sd = 0, sq = 0;
            for (int c = 0; c < n_chunks; ++c) {
                const int32_t cw0 = w_lo + c * IN_CHUNK_WORDS, cw = min(IN_CHUNK_WORDS, w_hi - cw0 + 1);
                if (n_chunks > 1 || !staged) {
                    __syncthreads();  // (the last chunk's reads are over)
                    for (int i = threadIdx.x; i < 32 * cw; i += SC_THREADS) {
                        const int32_t t = 32 * cw0 + i;
                        int32_t pa = -1;
                        if (t >= a.t0 && t < a.t1 && ((a.bitsT[(int64_t)(cw0 + (i >> 5)) * a.n_pad + ta] >> (i & 31)) & 1u)) {
                            const unsigned long long e = a.rowpd[(int64_t)(t - a.t0) * a.n_pad + ta];
                            pa = (int32_t)(uint32_t)e;
                            s_da[i] = (int32_t)(e >> 32);
                            s_base[i] = (int32_t)(a.off[t] - a.l0);
                            s_wt[i] = a.w ? a.w[t] : 1;
                        }
                        s_pa[i] = pa;
                        // (i runs in steps of the workgroup: a wave holds 64 trees in a row, two words)
                        const unsigned long long m = __ballot(pa >= 0);
                        if (lane == 0) {
                            s_ma[i >> 5] = (uint32_t)m;
                            s_ma[(i >> 5) + 1] = (uint32_t)(m >> 32);
                        }
                    }
                    __syncthreads();
                    staged = true;
                }
                if (!act) continue;
                for (int w = 0; w < cw; ++w) {
                    uint32_t m = s_ma[w];
                    if (!m) continue;
                    m &= a.bitsT[(int64_t)(cw0 + w) * a.n_pad + b];
                    for (; m; m &= m - 1) {
                        const int i = 32 * w + __builtin_ctz(m);
                        const unsigned long long e = a.rowpd[(int64_t)(32 * cw0 + i - a.t0) * a.n_pad + b];
                        const int32_t pb = (int32_t)(uint32_t)e, pa = s_pa[i];
                        const int32_t l = min(pa, pb), len = max(pa, pb) - l;  // gaps l .. l + len - 1
                        const int j = 31 - __clz(len);
                        const int32_t *lev = a.tab + (int64_t)j * a.Lb + s_base[i] + l;
                        const int32_t rm = min(lev[0], lev[len - (1 << j)]);
                        const unsigned long long d = (unsigned long long)(s_da[i] + (int32_t)(e >> 32) - 2 * rm);
                        const unsigned long long wt = (unsigned long long)s_wt[i], wd = wt * d;
                        sw += wt;
                        sd += wd;
                        sq += wd * d;
                    }
                }
            }
            if (act) {
                if (a.c_w || a.c_d || a.c_q) {
                    const int64_t cell = (ri - a.out_r0) * a.n + b, mir = (int64_t)b * a.n + ta;
                    unsigned long long *const cs[3] = {a.c_w, a.c_d, a.c_q};
                    const unsigned long long v[3] = {sw, sd, sq};
                    for (int x = 0; x < 3; ++x) {
                        if (!cs[x] || !v[x]) continue;  // (cells accumulate over the tree batches, from zeros)
                        cs[x][cell] += v[x];
                        if (a.mirror) cs[x][mir] += v[x];
                    }
                }
                if (a.mirror && sw) {
                    atomicAdd(a.s_w + b, sw);
                    atomicAdd(a.s_d + b, sd);
                    atomicAdd(a.s_q + b, sq);
                    if (a.count_partners) atomicAdd(a.partners + b, 1);
                }
                tw += sw;
                td += sd;
                tq += sq;
                tp += sw != 0;
            }
        }
        tw = in_wave_sum(tw);
        td = in_wave_sum(td);
        tq = in_wave_sum(tq);
        tp = (int)in_wave_sum((unsigned long long)tp);
        if (lane == 0 && tw) {
            atomicAdd(a.s_w + ri, tw);
            atomicAdd(a.s_d + ri, td);
            atomicAdd(a.s_q + ri, tq);
            if (a.count_partners) atomicAdd(a.partners + ri, tp);
        }
    }
}

// taxon_partners from the bits of all trees: one workgroup per (row, tile), a lane owns one b
__global__ void __launch_bounds__(SC_THREADS) k_in_partners(const int32_t *__restrict__ rows, int64_t r0,
                                                            int64_t n_items, int32_t n, int32_t nt, int64_t n_pad,
                                                            int W, const uint32_t *__restrict__ bitsT,
                                                            int32_t *__restrict__ partners) {
    for (int64_t idx = blockIdx.x; idx < n_items; idx += gridDim.x) {
        const int64_t ri = r0 + idx / nt;
        const int32_t b = (int32_t)(idx % nt) * IN_TILE + (int32_t)threadIdx.x;
        const int32_t ta = rows ? rows[ri] : (int32_t)ri;
        uint32_t any = 0;
        if (b < n && b != ta)
            for (int w = 0; w < W; ++w) any |= bitsT[(int64_t)w * n_pad + ta] & bitsT[(int64_t)w * n_pad + b];
        const int cnt = __popcll(__ballot(any != 0));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(partners + ri, cnt);
    }
}

// one thread per leaf of the batch's trees [0, nb) (off points at the batch's first tree): the link of its gap
__global__ void __launch_bounds__(SC_THREADS) k_in_links(const int64_t *__restrict__ off, int nb,
                                                         const int32_t *__restrict__ adj,
                                                         const int32_t *__restrict__ amin, int64_t Lb, int levels,
                                                         unsigned long long *__restrict__ link) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Lb) return;
    const int t = sc_tree_of(off, nb, off[0] + q);
    const int64_t base = off[t] - off[0], n = off[t + 1] - off[t], k = q - base;
    unsigned long long e = (unsigned long long)IN_DONE << 32;
    if (k + 1 < n) {
        const int32_t d = adj[q];
        // the gaps [lo, hi) around k are at depth d or deeper: k's node and what hangs below it
        const int64_t lo = sc_stretch_left(adj, amin, Lb, levels, base, k, d, true);
        const int64_t hi = sc_stretch_right(adj, amin, Lb, levels, base, k + 1, n - 1, d);
        if (lo > 0 || hi < n - 1) {
            const int64_t g = lo == 0 ? hi : hi == n - 1 ? lo - 1 : (adj[base + lo - 1] >= adj[base + hi] ? lo - 1 : hi);
            e = (unsigned long long)(base + g) << 32 | 1ull;
        }
    }
    link[q] = e;
}

__global__ void k_in_jump(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst,
                          int64_t Lb) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Lb) return;
    unsigned long long e = src[q];
    const uint32_t p = (uint32_t)(e >> 32);
    if (p != IN_DONE) {
        const unsigned long long f = src[p];
        e = (f & 0xffffffff00000000ull) | (uint32_t)((uint32_t)e + (uint32_t)f);
    }
    dst[q] = e;
}

// r per gap (0 at a tree's last leaf, which has no gap), the leaf depths and the largest per tree
__global__ void __launch_bounds__(SC_THREADS) k_in_depths(const int64_t *__restrict__ off, int nb,
                                                          const unsigned long long *__restrict__ link, int64_t Lb,
                                                          int32_t *__restrict__ r_out, int32_t *__restrict__ ldep,
                                                          int32_t *__restrict__ ht) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = q < Lb;
    const int t = in ? sc_tree_of(off, nb, off[0] + q) : nb - 1;
    int32_t dep = 0;
    if (in) {
        const int64_t base = off[t] - off[0], n = off[t + 1] - off[t], k = q - base;
        const int32_t r = k + 1 < n ? (int32_t)(uint32_t)link[q] : 0;
        r_out[q] = r;
        if (n > 1) dep = 1 + max(k + 1 < n ? r : -1, k > 0 ? (int32_t)(uint32_t)link[q - 1] : -1);
        ldep[q] = dep;
    }
    const int t0 = __shfl(t, 0, 64);
    if (__all(t == t0)) {
        for (int d = 32; d >= 1; d >>= 1) dep = max(dep, __shfl_xor(dep, d, 64));
        if ((threadIdx.x & 63) == 0 && dep > 0) atomicMax(ht + t0, dep);
    } else if (in && dep > 0) {
        atomicMax(ht + t, dep);
    }
}

// dense rows of the batch's trees [0, nb) (off points at the batch's first tree, tree t0 of the tables) and their
// bits: flags 1 a taxon out of range, 4 a taxon twice in one tree
__global__ void k_in_scatter(const int64_t *__restrict__ off, int nb, int32_t t0,
                             const int32_t *__restrict__ leaf_taxon, int32_t n_taxa,
                             const int32_t *__restrict__ ldep, const int64_t *__restrict__ w,
                             unsigned long long *__restrict__ rowpd, uint32_t *__restrict__ bitsT, int64_t n_pad,
                             unsigned *__restrict__ flags) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = off[0] + q;
    if (p >= off[nb]) return;
    const int t = sc_tree_of(off, nb, p);
    const int32_t x = leaf_taxon[p];
    if (x < 0 || x >= n_taxa) {
        atomicOr(flags, 1u);
        return;
    }
    const unsigned long long e = (unsigned long long)(uint32_t)ldep[q] << 32 | (uint32_t)(p - off[t]);
    if (atomicCAS(rowpd + (int64_t)t * n_pad + x, IN_EMPTY, e) != IN_EMPTY) atomicOr(flags, 4u);
    if (!w || w[t0 + t] != 0) atomicOr(bitsT + (int64_t)((t0 + t) >> 5) * n_pad + x, 1u << ((t0 + t) & 31));
}

// The plan of a call: the row batches (outer loop) and the tree batches (inner loop), each within half of SC_BUDGET
struct in_plan {
    int levels = 1;         // of the min tables: 2^levels > the largest tree
    int width = 4;          // bytes of an entry of the table of r
    int32_t W = 1;          // words of a taxon over all trees
    int64_t n_pad = 0;      // stride of the dense rows and of bitsT: n rounded up to 64
    int32_t nt = 0, tg = 1, ng = 0;  // tiles of a row, tiles of a work item, items of a row
    int64_t per_row = 0;    // bytes of a row's cells in the matrices wanted
    int64_t batch_rows = 0, out_rows = 0;  // rows of a batch at most; rows the matrices hold
    int64_t max_lb = 0, max_nb = 0;
    int64_t fixed = 0;      // bytes of the block without the matrices
    int mirror = 0;
    int64_t grid_limit = 0, rows_per_launch = 0;
    std::vector<int64_t> rstart;  // first row of every row batch, and n_rows
    std::vector<int32_t> bstart;  // first tree of every tree batch, and M
};

struct in_block {
    unsigned *flag;
    int32_t *rows, *ht, *partners, *tab, *ldep;
    int64_t *w;
    unsigned long long *sums, *rowpd, *link0, *link1, *out;
    uint32_t *bitsT;
};

size_t in_carve(sc_carver &c, const in_plan &p, size_t n, size_t n_rows, size_t M, size_t n_mat, in_block &k) {
    const size_t nr = std::max(n_rows, n);  // (mirror adds to the totals by taxon)
    k.flag = c.take<unsigned>(1);
    k.rows = c.take<int32_t>(n_rows);
    k.w = c.take<int64_t>(M);
    k.ht = c.take<int32_t>(M);
    k.sums = c.take<unsigned long long>(3 * nr);
    k.partners = c.take<int32_t>(nr);
    k.bitsT = c.take<uint32_t>((size_t)p.W * p.n_pad);
    k.rowpd = c.take<unsigned long long>((size_t)p.max_nb * p.n_pad);
    k.link0 = c.take<unsigned long long>((size_t)p.max_lb);
    k.link1 = c.take<unsigned long long>((size_t)p.max_lb);
    k.ldep = c.take<int32_t>((size_t)p.max_lb);
    k.tab = c.take<int32_t>((size_t)p.max_lb * std::max(p.levels, 2));
    k.out = c.take<unsigned long long>(n_mat * (size_t)p.out_rows * n);
    return c.at;
}

// Tree batches by bytes against half of SC_BUDGET: per tree its dense row (8 bytes a taxon) and per leaf the two link
// buffers, the depth and the table's levels; a batch ends before the tree that would take it past that, or at
// max_batch_trees.  Row batches by the cells of the matrices wanted against the other half, or max_batch_rows.
// `mirror` (only a < b is swept, both cells written) when the rows are all taxa and the matrices, if wanted, hold
// every row at once.  A work item is a row and `tg` tiles of it: fewer stagings of the row taxon's data where the rows
// alone give the device enough items.
in_plan in_plan_of(const int64_t *off, int32_t M, int64_t max_leaves, int32_t n, int64_t n_rows, bool all_rows,
                   int32_t max_batch_rows, int32_t max_batch_trees, int n_mat) {
    in_plan p;
    p.levels = sc_levels_host(std::max<int64_t>(max_leaves, 1));
    p.W = std::max<int32_t>((int32_t)(((int64_t)M + 31) / 32), 1);
    p.n_pad = scs_round_up(std::max<int64_t>(n, 1), 64);
    p.nt = (int32_t)(((int64_t)n + IN_TILE - 1) / IN_TILE);
    const uint64_t half = SC_BUDGET / 2;
    const auto per_tree = [&](int32_t t) {
        return (uint64_t)p.n_pad * 8 + (uint64_t)(off[t + 1] - off[t]) * (16 + 4 + 4 * std::max(p.levels, 2));
    };
    p.bstart.assign(1, 0);
    uint64_t acc = 0;
    for (int32_t t = 0; t < M; ++t) {
        const int32_t nb = t - p.bstart.back();
        if (nb > 0 && (acc + per_tree(t) > half || (max_batch_trees > 0 && nb >= max_batch_trees))) {
            p.bstart.push_back(t);
            acc = 0;
        }
        acc += per_tree(t);
    }
    p.bstart.push_back(M);
    for (size_t b = 0; b + 1 < p.bstart.size(); ++b) {
        p.max_lb = std::max(p.max_lb, off[p.bstart[b + 1]] - off[p.bstart[b]]);
        p.max_nb = std::max<int64_t>(p.max_nb, p.bstart[b + 1] - p.bstart[b]);
    }
    p.per_row = (int64_t)n_mat * 8 * n;
    p.batch_rows = p.per_row ? std::max<int64_t>(1, (int64_t)(half / (uint64_t)p.per_row)) : std::max<int64_t>(n_rows, 1);
    if (max_batch_rows > 0) p.batch_rows = std::min<int64_t>(p.batch_rows, max_batch_rows);
    for (int64_t r = 0; r < n_rows; r += p.batch_rows) p.rstart.push_back(r);
    p.rstart.push_back(n_rows);
    if (n_rows == 0) p.rstart.assign(1, 0);
    p.out_rows = std::min<int64_t>(p.batch_rows, n_rows);
    p.mirror = all_rows && (n_mat == 0 || p.rstart.size() <= 2);
    const int64_t per_item = std::max<int64_t>(n_rows, 1) * std::max<int32_t>(p.nt, 1) / IN_ITEMS_WANTED;
    p.tg = (int32_t)std::min<int64_t>(std::max<int64_t>(per_item, 1), std::max<int32_t>(p.nt, 1));
    p.ng = p.nt ? (p.nt + p.tg - 1) / p.tg : 0;
    p.grid_limit = sp_grid_limit(SC_THREADS);
    p.rows_per_launch = std::max<int64_t>(p.grid_limit / std::max<int32_t>(p.ng, 1), 1);
    in_block k;
    sc_carver sizing;
    p.fixed = (int64_t)in_carve(sizing, p, (size_t)n, (size_t)n_rows, (size_t)M, 0, k);
    return p;
}

// the workgroups of the first launch of a row batch of nr rows
int64_t in_grid(const in_plan &p, int64_t nr) {
    return std::min<int64_t>(std::min(nr, p.rows_per_launch) * p.ng, p.grid_limit);
}

// B1 = Σ w (m - 1) 2h and, with `squares`, B2 = Σ w (m - 1) (2h)² against 2^63 - 1
int in_check_bounds(const char *who, const int64_t *off, int32_t M, const int64_t *w, const int32_t *h, bool squares) {
    const unsigned __int128 lim = (unsigned __int128)INT64_MAX;
    unsigned __int128 b1 = 0, b2 = 0;
    for (int32_t t = 0; t < M; ++t) {
        const int64_t m = off[t + 1] - off[t];
        if (m < 2) continue;
        const unsigned __int128 x = (unsigned __int128)(uint64_t)(w ? w[t] : 1) * (uint64_t)(m - 1), d = 2 * (uint64_t)h[t];
        // (a term alone is below 2^64 x 2^31 x 2^64: no wrap before the compare)
        b1 += x * d;
        SCS_REQUIRE(b1 <= lim, "%s: the bound B1 = sum of w (m - 1) 2h on dist_sum passes 2^63 - 1 at tree %d", who, t);
        if (!squares) continue;
        SCS_REQUIRE(x <= lim, "%s: the bound B2 = sum of w (m - 1) (2h)^2 on sq_sum passes 2^63 - 1 at tree %d", who, t);
        b2 += x * d * d;
        SCS_REQUIRE(b2 <= lim, "%s: the bound B2 = sum of w (m - 1) (2h)^2 on sq_sum passes 2^63 - 1 at tree %d", who, t);
    }
    return SCS_OK;
}

// the depth pass and the scatter of tree batch b into the block: tab, ldep, ht, rowpd, bitsT, flag
void in_prepare(const scs_tables *src, const in_plan &p, const in_block &k, size_t b, bool weighted, hipStream_t s,
                hipError_t &e) {
    const std::vector<int64_t> &off = src->h_tree_off;
    const int32_t t0 = p.bstart[b], nb = p.bstart[b + 1] - t0;
    const int64_t l0 = off[t0], lb = off[t0 + nb] - l0;
    if (lb == 0 || e != hipSuccess) return;
    const int64_t *d_off = src->d_tree_off + t0;
    const int32_t *adj = src->d_adj_depth + l0;
    // the min table of adj_depth lies in the levels the table of r takes afterwards
    int32_t *amin = k.tab + lb;
    for (int j = 1; j < p.levels && e == hipSuccess; ++j) {
        k_sp_level<<<grid_of(lb), SC_THREADS, 0, s>>>(j == 1 ? adj : amin + (int64_t)(j - 2) * lb,
                                                      amin + (int64_t)(j - 1) * lb, lb, (int64_t)1 << (j - 1));
        sc_launched(e);
    }
    if (e != hipSuccess) return;
    k_in_links<<<grid_of(lb), SC_THREADS, 0, s>>>(d_off, nb, adj, amin, lb, p.levels, k.link0);
    if (!sc_launched(e)) return;
    // a chain of links is shorter than the batch's largest tree
    const int rounds = sc_levels_host(std::max<int64_t>(sc_largest_tree(off.data(), t0, t0 + nb), 1));
    unsigned long long *from = k.link0, *to = k.link1;
    for (int r = 0; r < rounds; ++r) {
        k_in_jump<<<grid_of(lb), SC_THREADS, 0, s>>>(from, to, lb);
        if (!sc_launched(e)) return;
        std::swap(from, to);
    }
    k_in_depths<<<grid_of(lb), SC_THREADS, 0, s>>>(d_off, nb, from, lb, k.tab, k.ldep, k.ht + t0);
    if (!sc_launched(e)) return;
    for (int j = 1; j < p.levels && e == hipSuccess; ++j) {
        k_sp_level<<<grid_of(lb), SC_THREADS, 0, s>>>(k.tab + (int64_t)(j - 1) * lb, k.tab + (int64_t)j * lb, lb,
                                                      (int64_t)1 << (j - 1));
        sc_launched(e);
    }
    if (e == hipSuccess) e = hipMemsetAsync(k.rowpd, 0xff, (size_t)nb * p.n_pad * 8, s);
    if (e != hipSuccess) return;
    k_in_scatter<<<grid_of(lb), SC_THREADS, 0, s>>>(d_off, nb, t0, src->d_leaf_taxon, src->n_taxa, k.ldep,
                                                   weighted ? k.w : nullptr, k.rowpd, k.bitsT, p.n_pad, k.flag);
    sc_launched(e);
}

// the common head of the export and of scs_debug_internode_depths: the block, zeros, rows and weights up, the depth
// pass and the scatter of every tree batch, the flag and h_t down.  On SCS_OK the block is held and, with one tree
// batch, prepared; the caller releases it.
struct in_call {
    in_plan p;
    in_block k;
    void *block = nullptr;
    unsigned bad = 0;
    std::vector<int32_t> h;
};

int in_begin(const char *who, scs_ctx *ctx, const scs_tables *src, const in_plan &p, int32_t n_rows,
             const int32_t *rows, const int64_t *tree_w, int n_mat, in_call &c, hipError_t &e,
             int32_t *r_out = nullptr, int32_t *ldep_out = nullptr) {
    (void)who;
    const int32_t M = src->n_trees, n = src->n_taxa;
    const std::vector<int64_t> &off = src->h_tree_off;
    c.p = p;
    sc_carver sizing;
    const size_t bytes = in_carve(sizing, p, (size_t)n, (size_t)n_rows, (size_t)M, (size_t)n_mat, c.k);
    SCS_TRY(scs_block_alloc(ctx, bytes, &c.block));
    sc_carver carve{(char *)c.block, bytes};
    in_carve(carve, p, (size_t)n, (size_t)n_rows, (size_t)M, (size_t)n_mat, c.k);
    const in_block &k = c.k;
    hipStream_t s = ctx->stream;
    c.h.assign((size_t)M, 0);
    // flag, rows, weights, h_t, totals, partners and the bits are zeros to begin with (they lie ahead of rowpd)
    e = hipMemsetAsync(c.block, 0, (size_t)((char *)k.rowpd - (char *)c.block), s);
    if (e == hipSuccess && rows && n_rows) e = hipMemcpyAsync(k.rows, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && tree_w && M) e = hipMemcpyAsync(k.w, tree_w, (size_t)M * 8, hipMemcpyHostToDevice, s);
    for (size_t b = 0; b + 1 < p.bstart.size() && e == hipSuccess; ++b) {
        in_prepare(src, p, k, b, tree_w != nullptr, s, e);
        const int64_t l0 = off[p.bstart[b]], lb = off[p.bstart[b + 1]] - l0;
        if (e == hipSuccess && r_out && lb) e = hipMemcpyAsync(r_out + l0, k.tab, (size_t)lb * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && ldep_out && lb)
            e = hipMemcpyAsync(ldep_out + l0, k.ldep, (size_t)lb * 4, hipMemcpyDeviceToHost, s);
    }
    // every tree's taxa are checked, and every h_t known, before a sweep kernel runs
    if (e == hipSuccess) e = hipMemcpyAsync(&c.bad, k.flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && M) e = hipMemcpyAsync(c.h.data(), k.ht, (size_t)M * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return SCS_OK;
}

int in_end(const char *who, scs_ctx *ctx, in_call &c, hipError_t e) {
    if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);  // (nothing may still write into the block)
    scs_block_release(ctx, c.block);
    if (e != hipSuccess) {
        scs_set_error("%s: %s", who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCS_ENOMEM : SCS_EHIP;
    }
    SCS_REQUIRE(!c.bad, "%s: %s", who,
                (c.bad & 1u) ? "a leaf_taxon entry is out of range [0, n_taxa)" : "a source tree has a taxon twice");
    return SCS_OK;
}

}  // namespace

extern "C" int scs_score_internode(scs_ctx *ctx, const scs_tables *src, int32_t n_rows, const int32_t *rows,
                                   const int64_t *tree_w, int32_t max_batch_rows, int32_t max_batch_trees,
                                   int64_t *pair_weight, int64_t *dist_sum, int64_t *sq_sum, int64_t *taxon_weight,
                                   int64_t *taxon_sum, int64_t *taxon_sq, int32_t *taxon_partners) {
    const char *const who = "scs_score_internode";
    SCS_REQUIRE(ctx && src, "%s: null argument", who);
    const int32_t M = src->n_trees, n = src->n_taxa;
    SCS_REQUIRE(n_rows >= 0, "%s: n_rows = %d is negative", who, n_rows);
    SCS_REQUIRE(rows || n_rows == n, "%s: rows is null and n_rows = %d is not the %d taxa of the tables", who, n_rows,
                n);
    SCS_REQUIRE(max_batch_rows >= 0, "%s: max_batch_rows = %d is negative", who, max_batch_rows);
    SCS_REQUIRE(max_batch_trees >= 0, "%s: max_batch_trees = %d is negative", who, max_batch_trees);
    for (int32_t r = 0; r < n_rows && rows; ++r)
        SCS_REQUIRE(rows[r] >= 0 && rows[r] < n, "%s: rows[%d] = %d is not a taxon of the tables (%d taxa)", who, r,
                    rows[r], n);
    for (int32_t t = 0; t < M && tree_w; ++t)
        SCS_REQUIRE(tree_w[t] >= 0, "%s: tree_w[%d] = %lld is negative", who, t, (long long)tree_w[t]);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    if (n == 0) return SCS_OK;
    const std::vector<int64_t> &off = src->h_tree_off;
    int64_t *const mats[3] = {pair_weight, dist_sum, sq_sum};
    int n_mat = 0;
    for (int i = 0; i < 3; ++i) n_mat += mats[i] != nullptr;
    const in_plan p = in_plan_of(off.data(), M, src->max_leaves, n, n_rows, rows == nullptr, max_batch_rows,
                                 max_batch_trees, n_mat);
    in_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(in_begin(who, ctx, src, p, n_rows, rows, tree_w, n_mat, c, e));
    const in_block &k = c.k;
    hipStream_t s = ctx->stream;
    if (e != hipSuccess || c.bad) return in_end(who, ctx, c, e);
    if (const int rc = in_check_bounds(who, off.data(), M, tree_w, c.h.data(), sq_sum || taxon_sq)) {
        scs_block_release(ctx, c.block);
        return rc;
    }
    const size_t n_tb = p.bstart.size() - 1, nr_tot = std::max<size_t>((size_t)n_rows, (size_t)n);
    const size_t cells = (size_t)p.out_rows * n;
    unsigned long long *d_mats[3];
    for (size_t i = 0, at = 0; i < 3; ++i) d_mats[i] = mats[i] ? k.out + at++ * cells : nullptr;
    in_args a{};
    a.rows = rows ? k.rows : nullptr;
    a.n = n;
    a.nt = p.nt;
    a.tg = p.tg;
    a.ng = p.ng;
    a.n_pad = p.n_pad;
    a.off = src->d_tree_off;
    a.rowpd = k.rowpd;
    a.bitsT = k.bitsT;
    a.tab = k.tab;
    a.ldep = k.ldep;
    a.w = tree_w ? k.w : nullptr;
    a.mirror = p.mirror;
    a.count_partners = n_tb == 1;
    a.c_w = d_mats[0];
    a.c_d = d_mats[1];
    a.c_q = d_mats[2];
    a.s_w = k.sums;
    a.s_d = k.sums + nr_tot;
    a.s_q = k.sums + 2 * nr_tot;
    a.partners = k.partners;
    for (size_t rb = 0; rb + 1 < p.rstart.size() && e == hipSuccess && M > 0; ++rb) {
        const int64_t r0 = p.rstart[rb], nr = p.rstart[rb + 1] - r0;
        a.out_r0 = r0;
        if (n_mat) e = hipMemsetAsync(k.out, 0, (size_t)n_mat * cells * 8, s);
        for (size_t b = 0; b < n_tb && e == hipSuccess; ++b) {
            if (n_tb > 1) in_prepare(src, p, k, b, tree_w != nullptr, s, e);  // (one batch: in_begin left it prepared)
            a.t0 = p.bstart[b];
            a.t1 = p.bstart[b + 1];
            a.l0 = off[a.t0];
            a.Lb = off[a.t1] - a.l0;
            if (a.Lb == 0) continue;
            for (int64_t q0 = 0; q0 < nr && e == hipSuccess; q0 += p.rows_per_launch) {
                a.r0 = r0 + q0;
                a.n_items = std::min(p.rows_per_launch, nr - q0) * p.ng;
                k_in_sweep<<<(unsigned)std::min(a.n_items, p.grid_limit), SC_THREADS, 0, s>>>(a);
                sc_launched(e);
            }
        }
        for (int i = 0; i < 3 && e == hipSuccess; ++i)
            if (mats[i])
                e = hipMemcpyAsync(mats[i] + (size_t)r0 * n, d_mats[i], (size_t)nr * n * 8, hipMemcpyDeviceToHost, s);
        // (the next batch's memset follows the copies on the stream)
    }
    if (n_tb > 1 && taxon_partners)
        for (int64_t q0 = 0; q0 < n_rows && e == hipSuccess; q0 += p.rows_per_launch) {
            const int64_t items = std::min<int64_t>(p.rows_per_launch, n_rows - q0) * p.nt;
            k_in_partners<<<(unsigned)std::min(items, p.grid_limit), SC_THREADS, 0, s>>>(a.rows, q0, items, n, p.nt, p.n_pad,
                                                                                       p.W, k.bitsT, k.partners);
            sc_launched(e);
        }
    int64_t *const sums[3] = {taxon_weight, taxon_sum, taxon_sq};
    for (int i = 0; i < 3 && e == hipSuccess; ++i)
        if (sums[i] && n_rows)
            e = hipMemcpyAsync(sums[i], k.sums + (size_t)i * nr_tot, (size_t)n_rows * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && taxon_partners && n_rows)
        e = hipMemcpyAsync(taxon_partners, k.partners, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return in_end(who, ctx, c, e);
}

// the depth pass alone: r per gap (0 at every tree's last leaf), the leaf depths, both by global leaf index, and h_t
// per tree, downloaded from the arrays the sweep reads
extern "C" int scs_debug_internode_depths(scs_ctx *ctx, const scs_tables *src, int32_t max_batch_trees,
                                          int32_t *gap_r, int32_t *leaf_depth, int32_t *tree_height) {
    const char *const who = "scs_debug_internode_depths";
    SCS_REQUIRE(ctx && src, "%s: null argument", who);
    SCS_REQUIRE(max_batch_trees >= 0, "%s: max_batch_trees = %d is negative", who, max_batch_trees);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));
    if (src->n_taxa == 0) return SCS_OK;
    const in_plan p = in_plan_of(src->h_tree_off.data(), src->n_trees, src->max_leaves, src->n_taxa, 0, false, 0,
                                 max_batch_trees, 0);
    in_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(in_begin(who, ctx, src, p, 0, nullptr, nullptr, 0, c, e, gap_r, leaf_depth));
    const int rc = in_end(who, ctx, c, e);
    if (rc == SCS_OK && tree_height) std::copy(c.h.begin(), c.h.end(), tree_height);
    return rc;
}

// the plan of one scs_score_internode call on the host, by the functions the export calls.  n_rows < 0 stands for
// rows NULL.  With `heights` (h_t per tree; `tree_w` may be null) the overflow rule is applied as well, and its
// SCS_EINVAL returned.  info_out[16]: levels, entry width of the table of r, words, n_pad, tiles of a row, tiles of an
// item, items of a row, bytes of a row's cells, rows of a batch, fixed bytes (the block without matrices), the block's
// bytes with them, row batches, tree batches, grid limit, rows per launch, mirror.  rows_out[3 x row batches]: first
// row, rows, grid of the first launch.  trees_out[3 x tree batches]: first tree, trees, leaves.
extern "C" int scs_debug_internode_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                        int32_t n_taxa, int32_t n_rows, int32_t max_batch_rows,
                                        int32_t max_batch_trees, int32_t matrices_wanted, const int64_t *tree_w,
                                        const int32_t *heights, int32_t squares, int64_t *info_out, int64_t *rows_out,
                                        int64_t *trees_out) {
    const char *const who = "scs_debug_internode_plan";
    SCS_REQUIRE((src || tree_off) && info_out, "%s: null argument", who);
    SCS_REQUIRE(!src || n_trees == src->n_trees, "%s: the tables hold %d trees, not %d", who, src ? src->n_trees : 0,
                n_trees);
    SCS_REQUIRE(n_trees >= 0 && n_taxa >= 0 && max_batch_rows >= 0 && max_batch_trees >= 0, "%s: negative argument",
                who);
    SCS_REQUIRE(matrices_wanted >= 0 && matrices_wanted <= 3, "%s: matrices_wanted = %d is not 0 ... 3", who,
                matrices_wanted);
    const int64_t *off = src ? src->h_tree_off.data() : tree_off;
    int64_t max_leaves = src ? src->max_leaves : 0;
    if (!src)
        for (int32_t t = 0; t < n_trees; ++t) {
            SCS_REQUIRE(off[t + 1] >= off[t], "%s: tree_off decreases at tree %d", who, t);
            max_leaves = std::max(max_leaves, off[t + 1] - off[t]);
        }
    for (int32_t t = 0; t < n_trees && tree_w; ++t)
        SCS_REQUIRE(tree_w[t] >= 0, "%s: tree_w[%d] = %lld is negative", who, t, (long long)tree_w[t]);
    const int32_t n = src ? src->n_taxa : n_taxa;
    const bool all_rows = n_rows < 0;
    const int64_t nr = all_rows ? n : n_rows;
    const in_plan p = in_plan_of(off, n_trees, max_leaves, n, nr, all_rows, max_batch_rows, max_batch_trees,
                                 matrices_wanted);
    const int64_t n_rb = (int64_t)p.rstart.size() - 1, n_tb = (int64_t)p.bstart.size() - 1;
    const int64_t info[16] = {p.levels, p.width, p.W, p.n_pad, p.nt, p.tg, p.ng, p.per_row, p.batch_rows, p.fixed,
                              p.fixed + (int64_t)sc_up256((size_t)matrices_wanted * p.out_rows * n * 8), n_rb, n_tb,
                              p.grid_limit, p.rows_per_launch, p.mirror};
    std::copy(info, info + 16, info_out);
    for (int64_t b = 0; b < n_rb && rows_out; ++b) {
        const int64_t row[3] = {p.rstart[b], p.rstart[b + 1] - p.rstart[b], in_grid(p, p.rstart[b + 1] - p.rstart[b])};
        std::copy(row, row + 3, rows_out + 3 * b);
    }
    for (int64_t b = 0; b < n_tb && trees_out; ++b) {
        const int64_t row[3] = {p.bstart[b], p.bstart[b + 1] - p.bstart[b], off[p.bstart[b + 1]] - off[p.bstart[b]]};
        std::copy(row, row + 3, trees_out + 3 * b);
    }
    if (heights) SCS_TRY(in_check_bounds(who, off, n_trees, tree_w, heights, squares != 0));
    return SCS_OK;
}
