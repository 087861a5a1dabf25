// scs_score_source_pair_triplets: the rooted-triplet terms between every two source trees, each pair restricted to the
// taxa both trees hold.  Included by scs_score.hip after scs_score_pairs.h, whose batches, dense
// rows, min tables and sp_* helpers it uses as they are: the two-sided restriction of section 33 joined to the
// node-pair sum of section 15.
//
// Per pair (A, B) -- A a row tree, B a column tree -- with L = L(A) ∩ L(B), c = |L|, y over the distinct non-root
// clusters of A|L, z over those of B|L, py / pz their parents and I(y, z) = |cl(y) ∩ cl(z)|:
//   triplets = sum_y C(|y|, 2) (|py| - |y|), triplets_other likewise over z,
//   triplets_shared = sum_y sum_z C(I(y,z), 2) (I(py,pz) - I(y,pz) - I(py,z) + I(y,z)).
// The pairs of a tile (row batch x column batch) go in CHUNKS; a pair of the chunk owns one region of the call's block:
// a header, A's node list (A ranks), B's node list (B ranks), the list B rank -> A rank, and the arrays of the
// restriction where they do not fit the launch's LDS.
//   k_st_restrict: one workgroup per pair.  Steps 1 - 2 of k_sp_pairs (membership bitsets with ranks, the compact
//     position lists), then one thread per restricted gap of either tree: the gap's node in the whole tree (two
//     descents on the tree's min table) has the ranks [lo, hi]; the gap is the first of its depth among the node's
//     restricted gaps iff it starts a distinct restricted cluster; the parent is the node of the deeper of the two
//     bounding restricted gaps (k_trip_nodes' rule on the restricted depth sequence, whose entries are range minima
//     of adj).  The same pass sums triplets / triplets_other.  A pair of c <= ST_SMALL_C is finished here: a cluster
//     is one 64-bit mask over A ranks and I a popcount.
//   k_st_pairs: the hot path, k_trip_pairs over a chunk: one workgroup per (pair, block of zb B nodes), cl(z) and
//     cl(pz) as bitsets over A ranks in LDS, each word paired with its prefix count; A's node list is swept once for
//     all zb nodes; one 64-bit atomic per workgroup and cell.  The grid counts min(n_A, n_B) - 2 nodes a pair.

namespace {

constexpr int ST_SMALL_C = 64;                            // c at most: the pair is finished in k_st_restrict
constexpr int ST_ZMAX = 32;                               // nodes of B a sweep workgroup takes at most (the grid counts
                                                          // min(n_A, n_B) - 2 nodes a pair: fewer idle workgroups)
constexpr int ST_HEAD = 128;                              // LDS bytes ahead: wave sums, node counters, 64-bit sums ...
constexpr int ST_SCRATCH = ST_HEAD + 4 * ST_SMALL_C * 8 + ST_SMALL_C * 4;  // ... and of a small pair the masks y, py,
                                                          // z, pz and its B rank -> A rank list
constexpr int ST_HEADER = 32;                             // a region's header: {c, ny, nz, both; cell; mirror cell}
constexpr uint64_t ST_CHUNK_BYTES = (uint64_t)512 << 20;  // regions of a chunk, together
constexpr uint64_t ST_HOLD_BYTES = (uint64_t)64 << 20;    // host offsets of chunks in flight, at most
constexpr int64_t ST_ROW_MAX = (int64_t)TP_LDS_MAX / 16 * 32 - 1;  // common taxa one node's two rows hold in LDS

// where the lists of a pair lie in its region, for a tile whose row trees have at most n_a leaves and whose column
// trees at most n_b; `work`: the restriction's arrays of the tile's largest pair, `stride`: bytes from pair to pair
struct st_layout {
    uint64_t o_z, o_map, o_work, work, stride;
};

// the restriction's arrays of one pair: both bitsets with their prefix counts, then the positions of the common
// leaves in A's and in B's order
__host__ __device__ inline uint64_t st_work_bytes(int64_t n_a, int64_t n_b) {
    const uint64_t cm = (uint64_t)(n_a < n_b ? n_a : n_b);
    return 8ull * ((uint64_t)(n_a >> 5) + 1 + (uint64_t)(n_b >> 5) + 1) + 8ull * cm;
}

st_layout st_layout_of(int64_t n_a, int64_t n_b) {
    st_layout l;
    const uint64_t cm = (uint64_t)std::min(n_a, n_b);
    l.o_z = ST_HEADER + 16 * cm;
    l.o_map = l.o_z + 16 * cm;
    l.o_work = (l.o_map + 4 * cm + 15) & ~15ull;
    l.work = st_work_bytes(n_a, n_b);
    l.stride = sc_up256(l.o_work + l.work);
    return l;
}

struct st_args {
    const int64_t *off;
    const int32_t *leaf_taxon, *adj;
    const int32_t *amin_r, *amin_c;      // as sp_args: the row / column batch's min table
    int64_t l0_r, lb_r, l0_c, lb_c;
    int levels;
    const int32_t *rowpos;
    int64_t row_stride;
    int32_t t0_r, t0_c, nb_c;
    const int32_t *rl_row, *rl_tree;     // the rows of the tile
    int64_t idx0, n_pairs;               // the chunk: pairs idx0 .. idx0 + n_pairs - 1 of the tile, row-major
    int32_t M;
    int mirror;
    int finish;                          // triplets_shared is wanted: lists for k_st_pairs, small pairs finished
    uint32_t lds_bytes;                  // of the LDS launch: ST_SCRATCH and a pair's arrays
    char *region;
    uint64_t o_z, o_map, o_work, stride;
    int32_t *common;
    unsigned long long *trip, *other, *shared;
};

// the bits [lo, hi) of a 64-bit mask
__device__ __forceinline__ unsigned long long st_range_mask(int lo, int hi) {
    const unsigned long long below_hi = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    return below_hi & ~((1ull << lo) - 1ull);
}

// One thread per restricted gap of the tree at `base` (n leaves; lp[k] = position of its k-th common leaf, c of them):
// the distinct non-root clusters {lo, hi + 1, parent lo, parent hi + 1} in the tree's own ranks into `list` (when
// given), their count into *cnt, and the thread's share of sum C(s, 2) (ps - s).  With m_own (a small pair) every
// cluster and its parent also as masks over A ranks, through `map` (B rank -> A rank, in LDS; null: the ranks are A's)
template <bool SLAB>
__device__ __forceinline__ unsigned long long st_nodes(const int32_t *__restrict__ adj,
                                                       const int32_t *__restrict__ amin, int64_t Lb, int levels,
                                                       int64_t base, int64_t n, const uint32_t *bits,
                                                       const uint32_t *pre, const uint32_t *lp, int c, int4 *list,
                                                       int *cnt, unsigned long long *m_own, unsigned long long *m_par,
                                                       const int32_t *map) {
    unsigned long long v = 0;
    const int threads = blockDim.x;
    for (int k0 = 0; k0 < c - 1; k0 += threads) {
        const int k = k0 + threadIdx.x;
        bool is = false;
        int4 nd = make_int4(0, 0, 0, 0);
        if (k < c - 1) {
            const int64_t p0 = sp_ld<SLAB>(lp + k), p1 = sp_ld<SLAB>(lp + k + 1);
            const int32_t d = sp_adj_min(adj, amin, Lb, base + p0, base + p1 - 1);
            int64_t first, last;
            sp_node(adj, amin, Lb, levels, base, n, p0, d, first, last);
            const int lo = sp_rank<SLAB>(bits, pre, first), hi = sp_rank<SLAB>(bits, pre, last + 1) - 1;
            if (hi - lo + 1 < c) {
                const int64_t pl = sp_ld<SLAB>(lp + lo);
                is = k == lo || sp_adj_min(adj, amin, Lb, base + pl, base + p0 - 1) > d;
            }
            if (is) {
                // the parent: the node of the deeper of the restricted gaps lo - 1 and hi
                const int g = lo == 0 ? hi : lo - 1;
                int64_t q0 = sp_ld<SLAB>(lp + g);
                int32_t dg = sp_adj_min(adj, amin, Lb, base + q0, base + (int64_t)sp_ld<SLAB>(lp + g + 1) - 1);
                if (lo > 0 && hi < c - 1) {
                    const int64_t r0 = sp_ld<SLAB>(lp + hi), r1 = sp_ld<SLAB>(lp + hi + 1);
                    const int32_t dh = sp_adj_min(adj, amin, Lb, base + r0, base + r1 - 1);
                    if (dh > dg) q0 = r0, dg = dh;
                }
                sp_node(adj, amin, Lb, levels, base, n, q0, dg, first, last);
                const int plo = sp_rank<SLAB>(bits, pre, first), phi = sp_rank<SLAB>(bits, pre, last + 1) - 1;
                nd = make_int4(lo, hi + 1, plo, phi + 1);
                v += sc_pairs_out(lo, hi, plo, phi);
            }
        }
        const unsigned long long hits = __ballot(is);
        int slot = 0;
        if ((threadIdx.x & 63) == 0 && hits) slot = atomicAdd(cnt, (int)__popcll(hits));
        slot = __shfl(slot, 0, 64) + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hits >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((unsigned)hits, 0u));
        if (is) {
            if (list) list[slot] = nd;
            if (m_own) {  // (c <= 64: at most 62 clusters)
                unsigned long long mo = 0, mp = 0;
                if (map) {
                    for (int i = nd.z; i < nd.w; ++i) {
                        const unsigned long long bit = 1ull << map[i];
                        mp |= bit;
                        if (i >= nd.x && i < nd.y) mo |= bit;
                    }
                } else {
                    mo = st_range_mask(nd.x, nd.y);
                    mp = st_range_mask(nd.z, nd.w);
                }
                m_own[slot] = mo;
                m_par[slot] = mp;
            }
        }
    }
    return v;
}

// adds the threads' v into the LDS sum *to
__device__ __forceinline__ void st_sum(unsigned long long v, unsigned long long *to) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(to, v);
}

template <bool SLAB>
__device__ __forceinline__ void st_pair(const st_args &a, char *reg, char *work, int r, int A, int B, int64_t n_a,
                                        int64_t n_b, char *head) {
    const uint32_t w_a = (uint32_t)(n_a >> 5) + 1, w_b = (uint32_t)(n_b >> 5) + 1;
    const int64_t cm = n_a < n_b ? n_a : n_b;
    uint32_t *bits_a = (uint32_t *)work, *pre_a = bits_a + w_a, *bits_b = pre_a + w_a, *pre_b = bits_b + w_b;
    uint32_t *la = pre_b + w_b, *lb = la + cm;
    int4 *ylist = (int4 *)(reg + ST_HEADER), *zlist = (int4 *)(reg + a.o_z);
    int32_t *map = (int32_t *)(reg + a.o_map);
    int *ws = (int *)head;                                                // [16] wave sums of sp_scan_bits
    int *cnt = ws + SP_THREADS_MAX / 64;                                  // ny, nz
    unsigned long long *sums = (unsigned long long *)(head + 80);        // triplets, triplets_other, shared
    unsigned long long *masks = (unsigned long long *)(head + ST_HEAD);  // [4][ST_SMALL_C]
    int32_t *smap = (int32_t *)(masks + 4 * ST_SMALL_C);                 // map's first ST_SMALL_C entries
    const int64_t p_a = a.off[A], p_b = a.off[B];
    const int32_t *row = a.rowpos + (int64_t)(A - a.t0_r) * a.row_stride;
    const int32_t *tax_b = a.leaf_taxon + p_b;
    const int32_t *adj_a = a.adj + a.l0_r, *adj_b = a.adj + a.l0_c;
    const int64_t base_a = p_a - a.l0_r, base_b = p_b - a.l0_c;
    const int threads = blockDim.x;

    // (1) membership, as k_sp_pairs
    for (uint32_t w = threadIdx.x; w < w_a; w += threads) sp_st<SLAB>(bits_a + w, 0u);
    for (uint32_t w = threadIdx.x; w < w_b; w += threads) sp_st<SLAB>(bits_b + w, 0u);
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    if (threadIdx.x < 3) sums[threadIdx.x] = 0;
    sp_sync<SLAB>();
    for (int64_t q = threadIdx.x; q < n_b; q += threads) {
        const int32_t pa = row[tax_b[q]];
        if (pa >= 0) {
            atomicOr(bits_b + (q >> 5), 1u << (q & 31));
            atomicOr(bits_a + (pa >> 5), 1u << (pa & 31));
        }
    }
    sp_sync<SLAB>();
    const int c = sp_scan_bits<SLAB>(bits_a, pre_a, (int)w_a, ws);
    sp_scan_bits<SLAB>(bits_b, pre_b, (int)w_b, ws);
    const int64_t cell = (int64_t)r * a.M + B, mirror = (int64_t)B * a.M + A;
    const bool both = a.mirror && A != B;
    int *hdr = (int *)reg;
    if (c < 3) {  // (the three counts stay 0, as the call's memset left them)
        if (threadIdx.x == 0) {
            hdr[0] = c, hdr[1] = 0, hdr[2] = 0, hdr[3] = 0;
            if (a.common) {
                a.common[cell] = c;
                if (both) a.common[mirror] = c;
            }
        }
        return;
    }
    sp_sync<SLAB>();
    // (2) the compact lists, and B rank -> A rank
    for (int64_t q = threadIdx.x; q < n_b; q += threads) {
        const int32_t pa = row[tax_b[q]];
        if (pa >= 0) {
            const int ka = sp_rank<SLAB>(bits_a, pre_a, pa), kb = sp_rank<SLAB>(bits_b, pre_b, q);
            sp_st<SLAB>(la + ka, (uint32_t)pa);
            sp_st<SLAB>(lb + kb, (uint32_t)q);
            map[kb] = ka;
            if (kb < ST_SMALL_C) smap[kb] = ka;
        }
    }
    __threadfence();
    __syncthreads();
    // (3) the distinct clusters of both restricted trees
    const bool small = c <= ST_SMALL_C, finish = a.finish != 0;
    const bool lists = finish && !small, mask = finish && small;
    const unsigned long long vt =
        st_nodes<SLAB>(adj_a, a.amin_r, a.lb_r, a.levels, base_a, n_a, bits_a, pre_a, la, c, lists ? ylist : nullptr,
                       cnt + 0, mask ? masks : nullptr, masks + ST_SMALL_C, nullptr);
    const unsigned long long vs =
        st_nodes<SLAB>(adj_b, a.amin_c, a.lb_c, a.levels, base_b, n_b, bits_b, pre_b, lb, c, lists ? zlist : nullptr,
                       cnt + 1, mask ? masks + 2 * ST_SMALL_C : nullptr, masks + 3 * ST_SMALL_C, smap);
    st_sum(vt, sums + 0);
    st_sum(vs, sums + 1);
    __syncthreads();
    const int ny = cnt[0], nz = cnt[1];
    if (mask) {
        // (4) a small pair: every node pair from the masks
        const unsigned long long *ym = masks, *pym = ym + ST_SMALL_C, *zm = pym + ST_SMALL_C, *pzm = zm + ST_SMALL_C;
        unsigned long long acc = 0;
        for (int i = threadIdx.x; i < ny * nz; i += threads) {
            const int y = i / nz, z = i - y * nz;
            const int iyz = __popcll(ym[y] & zm[z]);
            if (iyz < 2) continue;
            const int ipyz = __popcll(pym[y] & zm[z]), iypz = __popcll(ym[y] & pzm[z]);
            const int ipp = __popcll(pym[y] & pzm[z]);
            acc += (unsigned long long)((int64_t)iyz * (iyz - 1) / 2 * (int64_t)(ipp - iypz - ipyz + iyz));
        }
        st_sum(acc, sums + 2);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hdr[0] = c, hdr[1] = ny, hdr[2] = lists ? nz : 0, hdr[3] = both;
        ((int64_t *)reg)[2] = cell;
        ((int64_t *)reg)[3] = mirror;
        if (a.common) {
            a.common[cell] = c;
            if (both) a.common[mirror] = c;
        }
        if (a.trip) {
            a.trip[cell] = sums[0];
            if (both) a.trip[mirror] = sums[1];
        }
        if (a.other) {
            a.other[cell] = sums[1];
            if (both) a.other[mirror] = sums[0];
        }
        if (mask) {  // (a larger pair's cells take the sums of k_st_pairs)
            a.shared[cell] = sums[2];
            if (both) a.shared[mirror] = sums[2];
        }
    }
}

// SLAB false: the pairs of the chunk whose arrays fit a.lds_bytes; true: the others, their arrays in their regions
template <bool SLAB>
__global__ void __launch_bounds__(SC_THREADS) k_st_restrict(st_args a) {
    extern __shared__ __align__(16) char st_lds[];
    const int64_t p = blockIdx.x;
    if (p >= a.n_pairs) return;
    const int64_t idx = a.idx0 + p;
    const int i = (int)(idx / a.nb_c), j = (int)(idx % a.nb_c);
    const int r = a.rl_row[i], A = a.rl_tree[i], B = a.t0_c + j;
    if (a.mirror && A > B) return;
    const int64_t n_a = a.off[A + 1] - a.off[A], n_b = a.off[B + 1] - a.off[B];
    if ((st_work_bytes(n_a, n_b) + ST_SCRATCH <= a.lds_bytes) == SLAB) return;
    char *reg = a.region + p * a.stride;
    st_pair<SLAB>(a, reg, SLAB ? reg + a.o_work : st_lds + ST_SCRATCH, r, A, B, n_a, n_b, st_lds);
}

// the hot path: workgroup g of the chunk is block g - blk[p] of zb B nodes of pair p (blk[0] = 0, blk[n] = the grid)
__global__ void __launch_bounds__(SC_THREADS) k_st_pairs(const int64_t *__restrict__ blk, int n, const char *region,
                                                         uint64_t stride, uint64_t o_z, uint64_t o_map, int zb,
                                                         unsigned long long *__restrict__ shared) {
    extern __shared__ __attribute__((aligned(16))) int2 st_rows[];  // [2 zb][W]: rows 2j / 2j + 1 = cl(z_j) / cl(pz_j)
    int2 *rows = st_rows;
    const int64_t g = blockIdx.x;
    const int p = sc_tree_of(blk, n, g);
    const char *reg = region + (uint64_t)p * stride;
    const int4 hdr = *(const int4 *)reg;  // {c, ny, nz, both}
    const int j0 = (int)(g - blk[p]) * zb;
    const int nz = min(zb, hdr.z - j0);
    if (nz <= 0) return;  // (the grid counts min(n_A, n_B) - 2 nodes per pair: an upper bound)
    const int W = (hdr.x >> 5) + 1;
    const int4 *ylist = (const int4 *)(reg + ST_HEADER), *zlist = (const int4 *)(reg + o_z);
    const int32_t *map = (const int32_t *)(reg + o_map);
    const int nrow = 2 * nz;
    for (int i = threadIdx.x; i < nrow * W; i += SC_THREADS) rows[i] = make_int2(0, 0);
    __syncthreads();
    unsigned *bits = reinterpret_cast<unsigned *>(rows);  // (word i of the image: .x of entry i / 2)
    for (int j = 0; j < nz; ++j) {
        const int4 z = zlist[j0 + j];
        for (int k = z.x + threadIdx.x; k < z.y; k += SC_THREADS) {
            const int x = map[k];
            atomicOr(bits + 2 * ((2 * j) * W + (x >> 5)), 1u << (x & 31));
        }
        for (int k = z.z + threadIdx.x; k < z.w; k += SC_THREADS) {
            const int x = map[k];
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
    unsigned long long acc = 0;
    const int ny = hdr.y;
    for (int i = threadIdx.x; i < ny; i += SC_THREADS) {
        const int4 y = ylist[i];  // A ranks [y.x, y.y) of y, [y.z, y.w) of py
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
        if (tot) {
            const int64_t *cells = (const int64_t *)reg;
            atomicAdd(shared + cells[2], tot);
            if (hdr.w) atomicAdd(shared + cells[3], tot);
        }
    }
}

// ---- the plan ----

// a tile (row batch I, column batch J) with rows: its largest row tree, its largest column tree, the common taxa a
// pair may have, the words and nodes of a k_st_pairs workgroup and its LDS, the LDS of the k_st_restrict launch and
// whether the region launch is made too, the regions, the pairs of a chunk at most
struct st_tile {
    int64_t n_rl = 0, na = 0, nb = 0, cm = 0, chunk_cap = 0, pairs = 0;
    int W = 0, zb = 0;
    uint64_t lds_pairs = 0, lds_restrict = 0, need = 0;
    bool slab = false;
    st_layout lay{};
};

struct st_chunk {
    int64_t idx0 = 0, n = 0, small = 0, skipped = 0, blocks = 0;
};

struct st_plan {
    sp_plan sp;  // the batches, the levels, the dense rows: section 33's
    int lds_cap = 0;
    bool mirror = false;
    std::vector<int32_t> rl_row, rl_tree;  // the rows by the batch of their tree
    std::vector<size_t> rl_start;
    std::vector<st_tile> tiles;            // [I * batches + J]; n_rl = 0: no launch
    int64_t max_chunk = 0;                 // pairs of the call's largest chunk
    uint64_t region_bytes = 0;
};

// the k_st_pairs workgroups of a pair: none for the pair the mirror leaves out and for one that k_st_restrict surely
// finishes
int64_t st_pair_blocks(int64_t n_a, int64_t n_b, int zb) {
    const int64_t cm = std::min(n_a, n_b);
    return cm <= ST_SMALL_C ? 0 : (cm - 2 + zb - 1) / zb;
}

// the next chunk of a tile from pair idx0 on: it ends at the tile's chunk_cap pairs, or before the pair whose
// workgroups would take the k_st_pairs grid past the launch limit; blk gets its n + 1 offsets
st_chunk st_next_chunk(const int64_t *off, const st_plan &p, size_t I, size_t J, int64_t idx0,
                       std::vector<int64_t> *blk) {
    const st_tile &t = p.tiles[I * (p.sp.bstart.size() - 1) + J];
    const int32_t t0_c = p.sp.bstart[J], nb_c = p.sp.bstart[J + 1] - t0_c;
    const int64_t limit = sp_grid_limit(SC_THREADS);
    st_chunk ch;
    ch.idx0 = idx0;
    if (blk) blk->assign(1, 0);
    for (int64_t idx = idx0; idx < t.pairs && ch.n < t.chunk_cap; ++idx) {
        const int32_t A = p.rl_tree[p.rl_start[I] + (size_t)(idx / nb_c)], B = t0_c + (int32_t)(idx % nb_c);
        const int64_t n_a = off[A + 1] - off[A], n_b = off[B + 1] - off[B];
        const bool skip = p.mirror && A > B;
        const int64_t nblk = skip ? 0 : st_pair_blocks(n_a, n_b, t.zb);
        if (ch.n > 0 && ch.blocks + nblk > limit) break;
        ch.blocks += nblk;
        ch.skipped += skip;
        ch.small += !skip && std::min(n_a, n_b) <= ST_SMALL_C;
        ++ch.n;
        if (blk) blk->push_back(ch.blocks);
    }
    return ch;
}

// what a plan refuses: a pair that may share more taxa than a bitset row holds in LDS at all, or under the caller's cap
enum st_refusal { ST_FITS = 0, ST_TOO_LARGE, ST_CAP_TOO_SMALL };

// The plan of a call, and whether (and for which tree sizes) it is refused
st_refusal st_plan_of(st_plan &p, const int64_t *off, int32_t M, int64_t max_leaves, int32_t n_taxa, int32_t n_rows,
                       const int32_t *rows, int32_t max_batch_trees, int32_t max_lds_bytes, int32_t max_chunk_pairs,
                       int64_t &refused_a, int64_t &refused_b) {
    p.sp = sp_plan_of(off, M, max_leaves, n_taxa, max_batch_trees, 0);
    p.lds_cap = sc_lds_cap(max_lds_bytes);
    p.mirror = rows == nullptr;
    const size_t n_batches = p.sp.bstart.size() - 1;
    std::vector<int32_t> batch_of((size_t)M);
    p.rl_start.assign(n_batches + 1, 0);
    for (size_t b = 0; b < n_batches; ++b)
        for (int32_t t = p.sp.bstart[b]; t < p.sp.bstart[b + 1]; ++t) batch_of[t] = (int32_t)b;
    for (int32_t r = 0; r < n_rows; ++r) p.rl_start[batch_of[rows ? rows[r] : r] + 1]++;
    for (size_t b = 0; b < n_batches; ++b) p.rl_start[b + 1] += p.rl_start[b];
    p.rl_row.resize((size_t)n_rows);
    p.rl_tree.resize((size_t)n_rows);
    std::vector<size_t> at(p.rl_start.begin(), p.rl_start.end() - 1);
    for (int32_t r = 0; r < n_rows; ++r) {
        const int32_t t = rows ? rows[r] : r;
        p.rl_row[at[batch_of[t]]] = r;
        p.rl_tree[at[batch_of[t]]++] = t;
    }
    p.tiles.assign(n_batches * n_batches, st_tile{});
    st_refusal refused = ST_FITS;
    for (size_t I = 0; I < n_batches; ++I) {
        const size_t n_rl = p.rl_start[I + 1] - p.rl_start[I];
        if (n_rl == 0) continue;
        int64_t na = 0;
        for (size_t i = p.rl_start[I]; i < p.rl_start[I + 1]; ++i)
            na = std::max(na, off[p.rl_tree[i] + 1] - off[p.rl_tree[i]]);
        for (size_t J = p.mirror ? I : 0; J < n_batches; ++J) {
            st_tile &t = p.tiles[I * n_batches + J];
            t.n_rl = (int64_t)n_rl;
            t.na = na;
            t.nb = p.sp.largest[J];
            t.cm = std::min(t.na, t.nb);
            t.pairs = t.n_rl * (p.sp.bstart[J + 1] - p.sp.bstart[J]);
            t.W = (int)(std::min<int64_t>(t.cm, ST_ROW_MAX) >> 5) + 1;
            const int64_t rowb = 16 * (int64_t)t.W;
            if ((t.cm > ST_ROW_MAX || rowb > p.lds_cap) && refused == ST_FITS) {
                refused = t.cm > ST_ROW_MAX ? ST_TOO_LARGE : ST_CAP_TOO_SMALL;
                refused_a = t.na, refused_b = t.nb;
            }
            t.zb = (int)std::min<int64_t>(ST_ZMAX, std::max<int64_t>(1, std::min(TP_LDS_BUDGET, p.lds_cap) / rowb));
            t.lds_pairs = std::max<uint64_t>((uint64_t)t.zb * rowb, 32);
            t.lay = st_layout_of(t.na, t.nb);
            t.need = t.lay.work + ST_SCRATCH;
            t.slab = t.need > (uint64_t)p.lds_cap;
            t.lds_restrict = std::max<uint64_t>(std::min<uint64_t>(t.need, (uint64_t)p.lds_cap), ST_SCRATCH);
            t.chunk_cap = std::max<int64_t>(1, (int64_t)(ST_CHUNK_BYTES / t.lay.stride));
            if (max_chunk_pairs > 0) t.chunk_cap = std::min<int64_t>(t.chunk_cap, max_chunk_pairs);
            t.chunk_cap = std::min(std::min(t.chunk_cap, t.pairs), sp_grid_limit(SC_THREADS));
            p.max_chunk = std::max(p.max_chunk, t.chunk_cap);
            p.region_bytes = std::max(p.region_bytes, (uint64_t)t.chunk_cap * t.lay.stride);
        }
    }
    return refused;
}

// the block of a call: flag, row lists, outputs, the dense rows, the two batches' table levels, a chunk's offsets
// and regions
struct st_block {
    unsigned *flag;
    int32_t *rl_row, *rl_tree, *common, *rowpos, *amin_r, *amin_c;
    unsigned long long *out;
    int64_t *blk;
    char *region;
};

// (has_common, n_out: the matrices the caller asked for; the others get no room)
size_t st_carve(sc_carver &w, const st_plan &p, size_t n_rows, size_t M, bool has_common, size_t n_out, st_block &k) {
    const size_t lev = (size_t)std::max(p.sp.levels - 1, 1);
    k.flag = w.take<unsigned>(1);
    k.rl_row = w.take<int32_t>(n_rows);
    k.rl_tree = w.take<int32_t>(n_rows);
    k.common = w.take<int32_t>(has_common ? n_rows * M : 0);
    k.out = w.take<unsigned long long>(n_out * n_rows * M);
    k.rowpos = w.take<int32_t>((size_t)p.sp.max_nb * p.sp.row_stride);
    k.amin_r = w.take<int32_t>((size_t)p.sp.max_lb * lev);
    k.amin_c = w.take<int32_t>((size_t)p.sp.max_lb * lev);
    k.blk = w.take<int64_t>((size_t)p.max_chunk + 1);
    k.region = w.take<char>((size_t)p.region_bytes);
    return w.at;
}

int st_refuse(const char *who, st_refusal refused, int32_t max_lds_bytes, int64_t na, int64_t nb) {
    SCS_REQUIRE(refused != ST_TOO_LARGE,
                "%s: trees of %lld and %lld leaves may share more than the %lld taxa a bitset row holds in LDS", who,
                (long long)na, (long long)nb, (long long)ST_ROW_MAX);
    SCS_REQUIRE(refused != ST_CAP_TOO_SMALL,
                "%s: max_lds_bytes = %d does not hold the bitset rows of trees of %lld and %lld leaves", who,
                max_lds_bytes, (long long)na, (long long)nb);
    return SCS_OK;
}

}  // namespace

extern "C" int scs_score_source_pair_triplets(scs_ctx *ctx, const scs_tables *src, int32_t n_rows, const int32_t *rows,
                                              int32_t max_batch_trees, int32_t max_lds_bytes, int32_t max_chunk_pairs,
                                              int32_t *common, int64_t *triplets, int64_t *triplets_other,
                                              int64_t *triplets_shared) {
    const char *const who = "scs_score_source_pair_triplets";
    SCS_REQUIRE(ctx && src, "%s: null argument", who);
    const int32_t M = src->n_trees;
    SCS_REQUIRE(n_rows >= 0, "%s: n_rows = %d is negative", who, n_rows);
    SCS_REQUIRE(rows || n_rows == M, "%s: rows is null and n_rows = %d is not the %d trees of the tables", who, n_rows,
                M);
    SCS_REQUIRE(max_lds_bytes >= 0, "%s: max_lds_bytes = %d is negative", who, max_lds_bytes);
    SCS_REQUIRE(max_chunk_pairs >= 0, "%s: max_chunk_pairs = %d is negative", who, max_chunk_pairs);
    for (int32_t r = 0; r < n_rows && rows; ++r)
        SCS_REQUIRE(rows[r] >= 0 && rows[r] < M, "%s: rows[%d] = %d is not a tree of the tables (%d trees)", who, r,
                    rows[r], M);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    if (n_rows == 0 || M == 0) return SCS_OK;
    const std::vector<int64_t> &off = src->h_tree_off;
    st_plan p;
    int64_t ref_a = 0, ref_b = 0;
    const st_refusal refused = st_plan_of(p, off.data(), M, src->max_leaves, src->n_taxa, n_rows, rows, max_batch_trees,
                                     max_lds_bytes, max_chunk_pairs, ref_a, ref_b);
    SCS_TRY(st_refuse(who, refused, max_lds_bytes, ref_a, ref_b));
    const size_t n_batches = p.sp.bstart.size() - 1;
    int64_t *const outs[3] = {triplets, triplets_other, triplets_shared};
    size_t n_out = 0;
    for (int i = 0; i < 3; ++i) n_out += outs[i] != nullptr;
    st_block k;
    sc_carver sizing;
    const size_t bytes = st_carve(sizing, p, (size_t)n_rows, (size_t)M, common != nullptr, n_out, k);
    void *block = nullptr;
    SCS_TRY(scs_block_alloc(ctx, bytes, &block));
    sc_carver carve{(char *)block, bytes};
    st_carve(carve, p, (size_t)n_rows, (size_t)M, common != nullptr, n_out, k);
    const size_t cells = (size_t)n_rows * M;
    unsigned long long *d_outs[3];
    for (size_t i = 0, at = 0; i < 3; ++i) d_outs[i] = outs[i] ? k.out + at++ * cells : nullptr;
    hipStream_t s = ctx->stream;
    unsigned bad = 0;
    hipError_t e = hipMemsetAsync(k.flag, 0, 4, s);
    if (e == hipSuccess && common) e = hipMemsetAsync(k.common, 0, cells * 4, s);
    if (e == hipSuccess && n_out) e = hipMemsetAsync(k.out, 0, n_out * cells * 8, s);
    if (e == hipSuccess) e = hipMemcpyAsync(k.rl_row, p.rl_row.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(k.rl_tree, p.rl_tree.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    // the dense rows of batch b; its table levels into `amin` (as scs_score_source_pairs)
    const auto scatter = [&](size_t b) {
        const int32_t t0 = p.sp.bstart[b], nb = p.sp.bstart[b + 1] - t0;
        e = hipMemsetAsync(k.rowpos, 0xff, (size_t)nb * p.sp.row_stride * 4, s);
        if (e != hipSuccess) return;
        k_sp_scatter<<<grid_of(off[t0 + nb] - off[t0]), SC_THREADS, 0, s>>>(src->d_tree_off + t0, nb, src->d_leaf_taxon,
                                                                          src->n_taxa, k.rowpos, p.sp.row_stride,
                                                                          k.flag);
        sc_launched(e);
    };
    const auto levels_of = [&](size_t b, int32_t *amin) {
        const int64_t l0 = off[p.sp.bstart[b]], lb = off[p.sp.bstart[b + 1]] - l0;
        for (int j = 1; j < p.sp.levels && e == hipSuccess; ++j) {
            k_sp_level<<<grid_of(lb), SC_THREADS, 0, s>>>(j == 1 ? src->d_adj_depth + l0 : amin + (int64_t)(j - 2) * lb,
                                                          amin + (int64_t)(j - 1) * lb, lb, (int64_t)1 << (j - 1));
            sc_launched(e);
        }
    };
    // every tree's taxa are checked before a pair kernel reads a row by them: one scatter of every batch
    for (size_t b = 0; b < n_batches && e == hipSuccess; ++b) scatter(b);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, k.flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    // (the attribute is per function and device: set on every call)
    const void *const fns[3] = {(const void *)k_st_restrict<false>, (const void *)k_st_restrict<true>,
                                (const void *)k_st_pairs};
    for (int i = 0; i < 3 && e == hipSuccess; ++i)
        e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, TP_LDS_MAX);
    // the offsets of the chunks in flight: the copies read them after the call that queued them has returned
    std::vector<std::vector<int64_t>> held;
    uint64_t held_bytes = 0;
    for (size_t I = 0; I < n_batches && e == hipSuccess && !bad; ++I) {
        if (p.rl_start[I + 1] == p.rl_start[I]) continue;
        if (n_batches > 1) scatter(I);  // (one batch: the rows of the check are this batch's)
        levels_of(I, k.amin_r);
        for (size_t J = p.mirror ? I : 0; J < n_batches && e == hipSuccess; ++J) {
            if (J != I) levels_of(J, k.amin_c);
            if (e != hipSuccess) break;
            const st_tile &tile = p.tiles[I * n_batches + J];
            st_args a{};
            a.off = src->d_tree_off;
            a.leaf_taxon = src->d_leaf_taxon;
            a.adj = src->d_adj_depth;
            a.amin_r = k.amin_r;
            a.amin_c = J == I ? k.amin_r : k.amin_c;
            a.l0_r = off[p.sp.bstart[I]];
            a.lb_r = off[p.sp.bstart[I + 1]] - a.l0_r;
            a.l0_c = off[p.sp.bstart[J]];
            a.lb_c = off[p.sp.bstart[J + 1]] - a.l0_c;
            a.levels = p.sp.levels;
            a.rowpos = k.rowpos;
            a.row_stride = p.sp.row_stride;
            a.t0_r = p.sp.bstart[I];
            a.t0_c = p.sp.bstart[J];
            a.nb_c = p.sp.bstart[J + 1] - p.sp.bstart[J];
            a.rl_row = k.rl_row + p.rl_start[I];
            a.rl_tree = k.rl_tree + p.rl_start[I];
            a.M = M;
            a.mirror = p.mirror;
            a.finish = triplets_shared != nullptr;
            a.lds_bytes = (uint32_t)tile.lds_restrict;
            a.region = k.region;
            a.o_z = tile.lay.o_z;
            a.o_map = tile.lay.o_map;
            a.o_work = tile.lay.o_work;
            a.stride = tile.lay.stride;
            a.common = common ? k.common : nullptr;
            a.trip = d_outs[0];
            a.other = d_outs[1];
            a.shared = d_outs[2];
            for (int64_t idx0 = 0; idx0 < tile.pairs && e == hipSuccess;) {
                std::vector<int64_t> offsets;
                const st_chunk ch = st_next_chunk(off.data(), p, I, J, idx0, &offsets);
                a.idx0 = ch.idx0;
                a.n_pairs = ch.n;
                idx0 += ch.n;
                if (ch.skipped == ch.n) continue;  // (the mirror leaves the whole chunk out)
                k_st_restrict<false><<<(unsigned)ch.n, SC_THREADS, (size_t)tile.lds_restrict, s>>>(a);
                if (!sc_launched(e)) break;
                if (tile.slab) {
                    k_st_restrict<true><<<(unsigned)ch.n, SC_THREADS, ST_SCRATCH, s>>>(a);
                    if (!sc_launched(e)) break;
                }
                if (!a.finish || ch.blocks == 0) continue;
                held.push_back(std::move(offsets));
                const std::vector<int64_t> &blk = held.back();
                e = hipMemcpyAsync(k.blk, blk.data(), blk.size() * 8, hipMemcpyHostToDevice, s);
                if (e != hipSuccess) break;
                k_st_pairs<<<(unsigned)ch.blocks, SC_THREADS, (size_t)tile.lds_pairs, s>>>(
                    k.blk, (int)ch.n, k.region, tile.lay.stride, tile.lay.o_z, tile.lay.o_map, tile.zb, d_outs[2]);
                if (!sc_launched(e)) break;
                held_bytes += blk.size() * 8;
                if (held_bytes > ST_HOLD_BYTES) {
                    e = hipStreamSynchronize(s);
                    held.clear();
                    held_bytes = 0;
                }
            }
        }
    }
    if (e == hipSuccess && !bad && common) e = hipMemcpyAsync(common, k.common, cells * 4, hipMemcpyDeviceToHost, s);
    for (int i = 0; i < 3 && e == hipSuccess && !bad; ++i)
        if (outs[i]) e = hipMemcpyAsync(outs[i], d_outs[i], cells * 8, hipMemcpyDeviceToHost, s);
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

// the plan of one scs_score_source_pair_triplets call on the host, by the functions the export calls
extern "C" int scs_debug_source_pair_triplets_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                                   int32_t n_taxa, int32_t n_rows, const int32_t *rows,
                                                   int32_t max_batch_trees, int32_t max_lds_bytes,
                                                   int32_t max_chunk_pairs, int32_t *n_batches_out,
                                                   int32_t *bstart_out, int64_t *info_out, int64_t *tile_out,
                                                   int64_t *chunk_out) {
    const char *const who = "scs_debug_source_pair_triplets_plan";
    SCS_REQUIRE((src || tree_off) && n_batches_out && bstart_out && info_out, "%s: null argument", who);
    SCS_REQUIRE(!src || n_trees == src->n_trees, "%s: the tables hold %d trees, not %d", who, src ? src->n_trees : 0,
                n_trees);
    SCS_REQUIRE(n_trees >= 0 && n_taxa >= 0 && n_rows >= 0 && max_lds_bytes >= 0 && max_chunk_pairs >= 0,
                "%s: negative argument", who);
    SCS_REQUIRE(rows || n_rows == n_trees, "%s: rows is null and n_rows = %d is not the %d trees", who, n_rows,
                n_trees);
    for (int32_t r = 0; r < n_rows && rows; ++r)
        SCS_REQUIRE(rows[r] >= 0 && rows[r] < n_trees, "%s: rows[%d] = %d is not one of the %d trees", who, r, rows[r],
                    n_trees);
    const int64_t *off = src ? src->h_tree_off.data() : tree_off;
    int64_t max_leaves = src ? src->max_leaves : 0;
    if (!src)
        for (int32_t t = 0; t < n_trees; ++t) {
            SCS_REQUIRE(off[t + 1] >= off[t], "%s: tree_off decreases at tree %d", who, t);
            max_leaves = std::max(max_leaves, off[t + 1] - off[t]);
        }
    st_plan p;
    int64_t ref_a = 0, ref_b = 0;
    const st_refusal refused = st_plan_of(p, off, n_trees, max_leaves, src ? src->n_taxa : n_taxa, n_rows, rows,
                                     max_batch_trees, max_lds_bytes, max_chunk_pairs, ref_a, ref_b);
    SCS_TRY(st_refuse(who, refused, max_lds_bytes, ref_a, ref_b));
    const size_t nb = p.sp.bstart.size() - 1;
    *n_batches_out = (int32_t)nb;
    std::copy(p.sp.bstart.begin(), p.sp.bstart.end(), bstart_out);
    int64_t n_chunks = 0;
    for (size_t I = 0; I < nb; ++I)
        for (size_t J = 0; J < nb; ++J) {
            const st_tile &t = p.tiles[I * nb + J];
            int64_t mine = 0;
            for (int64_t idx0 = 0; idx0 < t.pairs; ++mine) {
                const st_chunk ch = st_next_chunk(off, p, I, J, idx0, nullptr);
                idx0 += ch.n;
                if (chunk_out) {
                    const int32_t nb_c = p.sp.bstart[J + 1] - p.sp.bstart[J];
                    const int64_t row[8] = {(int64_t)I, (int64_t)J, ch.idx0, ch.n, ch.small, ch.skipped, ch.blocks,
                                            (ch.idx0 + ch.n - 1) / nb_c - ch.idx0 / nb_c + 1};
                    std::copy(row, row + 8, chunk_out + 8 * (n_chunks + mine));
                }
            }
            if (tile_out) {
                const int64_t row[12] = {t.n_rl, t.cm, t.W, t.zb, (int64_t)t.lds_pairs, (int64_t)t.lds_restrict,
                                         t.slab, (int64_t)t.need, (int64_t)t.lay.stride, t.chunk_cap, t.pairs, mine};
                std::copy(row, row + 12, tile_out + 12 * (I * nb + J));
            }
            n_chunks += mine;
        }
    st_block k;
    sc_carver sizing;
    const int64_t info[8] = {p.sp.levels, p.sp.row_stride, p.lds_cap, ST_SMALL_C,
                             (int64_t)st_carve(sizing, p, (size_t)n_rows, (size_t)n_trees, true, 3, k),
                             (int64_t)p.region_bytes, sp_grid_limit(SC_THREADS), n_chunks};
    std::copy(info, info + 8, info_out);
    return SCS_OK;
}
