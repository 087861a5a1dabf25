// scs_score_coverage: the triple coverage of the sources -- which taxa are ever seen together.
// Included by scs_score.hip after its shared host layer.  Like scs_score_source_pairs the export has no supertree, so
// it does not go through sc_begin: it plans its own row batches and carves its own block.
//
// `sources` are tables as for scs_score_source_pairs.  Only `tree_off` and `leaf_taxon` are read.  n = the tables'
// `n_taxa`.
//   M[x] is the set of trees that hold taxon x.
//   cov(a, b, c) = |M[a] ∩ M[b] ∩ M[c]|.
//   A triple of three distinct taxa is *covered* when cov >= k, with k = `min_trees` >= 1.
// For the row taxa r, given as `rows` (ids in any order, repeats allowed; NULL means every taxon, and then `n_rows`
// must be n):
//   `occurs[x]`, int32, n entries, always for all taxa: |M[x]|.
//   `pair_trees[r][b]`, int32, n_rows x n, row-major: |M[a] ∩ M[b]|.  The diagonal is `occurs[a]`.
//   `pair_covered[r][b]`, int32, n_rows x n: #{c ∉ {a, b} : cov(a, b, c) >= k}.  The diagonal is 0.
//   `taxon_covered[r]`, int64, n_rows: the covered triples that contain a.  This equals Σ_b `pair_covered[r][b]` / 2.
//
//   k_cv_scatter: the membership bit matrix, one bit per (taxon, tree) in 32-bit words, built with atomicOr in both
//                 orders: taxon-major `bits[taxon][w]` for the pair side, word-major `bitsT[w][taxon]` for the lanes.  A
//                 bit already set in the returned old value is a taxon twice in one tree (flag 4, as k_sp_scatter).
//   k_cv_occurs:  occurs[x] = the set bits of row x.
//   k_cv_compact: the taxa with occurs >= k (the others cover nothing) as columns of `bitsC[w][i]`, word-major.
//   k_cv_sweep<WORDS, COUNT> / k_cv_stream<COUNT>: one workgroup per (row taxon a, tile of 64 taxa b).  Every wave
//                 first counts |M[a] ∩ M[b]| for its lane's b (that is pair_trees) and ballots the pairs that take
//                 part: pair_trees >= k, b != a and, when the rows are all taxa (`mirror`), b > a.  Then the
//                 workgroup walks the compact taxa c in chunks of 256, a lane owning one c of a chunk (of two
//                 chunks at once up to 32 words): it holds Q = M[c] & M[a] in WORDS registers (k_cv_stream reads it word by word from bitsC instead, for any
//                 number of trees), and for every pair of the ballot M[b] is wave-uniform -- one LDS address for the
//                 whole wave in k_cv_sweep, which stages the tile's rows there once; scalar loads in k_cv_stream --
//                 so the lane's test is one and-or per word and a compare (COUNT false, k = 1) or a popcount sum
//                 (k > 1).
//                 The covered lanes are counted with __ballot / __popcll and added to the register of the lane that
//                 stands for b: one add per (pair, 64 taxa), no atomics.  a and b themselves are lanes of the walk
//                 and are always covered in a pair that takes part (cov(a, b, a) = pair_trees), so 2 comes off at
//                 the end.  The four waves' sums meet in LDS; the tile's cells are written (both cells with `mirror`)
//                 and its sum is added to the row's 64-bit total, from which taxon_covered is halved on the host.
// Without the two matrices nothing of n_rows x n is allocated: the tile sums go straight to the row totals.

namespace {

constexpr int CV_REG_WORDS_MAX = 64;  // words of M[c] a lane holds at most; more trees than 32 x that stream
constexpr int CV_TILE = 64;           // taxa b of a workgroup: one per lane of a wave
constexpr int CV_CHUNK = SC_THREADS;  // taxa c of one pass of a workgroup: one per thread

struct cv_args {
    const int32_t *rows;   // row taxa of the call (null: row r is taxon r)
    int64_t r0;            // first row of the launch
    int64_t n_items;       // rows of the launch x nt
    int32_t n, nt;         // taxa; tiles of a row
    int32_t W;             // words of a taxon that hold trees
    int64_t wp;            // stride of a row of `bits` in words (WORDS of the register variant, else W)
    int64_t ncs;           // stride of a row of `bitsC`: the compact taxa rounded up to 2 CV_CHUNK (the rest zeros)
    int32_t k;
    int mirror;
    int64_t out_r0;        // first row the matrices of this batch hold (mirror: 0, and they hold all rows)
    int32_t *pair_trees, *pair_covered;  // the batch's rows x n, or null
    unsigned long long *rowsum;          // per row of the call
};

// |M[a] ∩ M[b]| over the W words of two rows of `bits`
__device__ __forceinline__ int cv_pair_trees(const uint32_t *__restrict__ ma, const uint32_t *__restrict__ mb, int W) {
    int pt = 0;
    for (int w = 0; w < W; ++w) pt += __popc(ma[w] & mb[w]);
    return pt;
}

// what both sweeps do before the walk: pair_trees of the lane's b, its cells, and the ballot of the pairs taking part
__device__ __forceinline__ unsigned long long cv_prologue(const cv_args &a, const uint32_t *__restrict__ bits,
                                                          int64_t ri, int32_t ta, int32_t b0) {
    const int lane = threadIdx.x & 63;
    const int32_t b = b0 + lane;
    const bool in = b < a.n;
    const int pt = in ? cv_pair_trees(bits + (int64_t)ta * a.wp, bits + (int64_t)b * a.wp, a.W) : 0;
    if (a.pair_trees && threadIdx.x < 64 && in && (!a.mirror || b >= ta)) {
        a.pair_trees[(ri - a.out_r0) * a.n + b] = pt;
        if (a.mirror && b > ta) a.pair_trees[(int64_t)b * a.n + ta] = pt;
    }
    return __ballot(in && pt >= a.k && b != ta && (!a.mirror || b > ta));
}

// ... and after it: the waves' sums of the tile, its cells and the row totals.  acc: the lane's count for b0 + lane
// over the c's of its wave, a and b among them
__device__ __forceinline__ void cv_epilogue(const cv_args &a, int (*red)[CV_TILE], int acc, unsigned long long act,
                                            int64_t ri, int32_t ta, int32_t b0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    red[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int32_t b = b0 + lane;
        int tot = 0;
        if ((act >> lane) & 1) tot = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane] - 2;
        if (a.pair_covered && b < a.n && (!a.mirror || b >= ta)) {
            a.pair_covered[(ri - a.out_r0) * a.n + b] = tot;
            if (a.mirror && b > ta) a.pair_covered[(int64_t)b * a.n + ta] = tot;
        }
        if (a.mirror && tot > 0) atomicAdd(a.rowsum + b, (unsigned long long)tot);
        long long s = tot;
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0 && s > 0) atomicAdd(a.rowsum + ri, (unsigned long long)s);
    }
    __syncthreads();  // (the next tile writes red again)
}

// row and tile of a work item; false: `mirror` leaves the whole tile to the rows of its taxa
__device__ __forceinline__ bool cv_item(const cv_args &a, int64_t idx, int64_t &ri, int32_t &ta, int32_t &b0) {
    ri = a.r0 + idx / a.nt;
    b0 = (int32_t)(idx % a.nt) * CV_TILE;
    ta = a.rows ? a.rows[ri] : (int32_t)ri;
    return !(a.mirror && b0 + CV_TILE - 1 < ta);
}

// WORDS: the stride of `bits` and the rows of `bitsC` (words past W are zeros).  COUNT: k > 1.  The tile's 64 rows
// M[b] are staged in LDS once and read from there by every chunk of the walk, one address for the whole wave (a
// broadcast).  Up to 32 words a lane owns two taxa c, CV_CHUNK apart, so one read of M[b] serves 128 taxa of a wave
template <int WORDS, bool COUNT>
__global__ void __launch_bounds__(SC_THREADS) k_cv_sweep(cv_args a, const uint32_t *__restrict__ bits,
                                                         const uint32_t *__restrict__ bitsC) {
    constexpr int CPL = WORDS <= 32 ? 2 : 1;
    __shared__ int red[SC_THREADS / 64][CV_TILE];
    __shared__ uint4 mbs[CV_TILE][WORDS / 4];
    const int lane = threadIdx.x & 63;
    for (int64_t idx = blockIdx.x; idx < a.n_items; idx += gridDim.x) {
        int64_t ri;
        int32_t ta, b0;
        if (!cv_item(a, idx, ri, ta, b0)) continue;
        const unsigned long long act = cv_prologue(a, bits, ri, ta, b0);
        int acc = 0;
        if (act) {
            // (rows past the last taxon are not read: they are no pair of the ballot)
            const uint4 *__restrict__ tile = (const uint4 *)(bits + (int64_t)b0 * WORDS);
            const int rows_in = min(CV_TILE, a.n - b0);
            for (int i = threadIdx.x; i < rows_in * (WORDS / 4); i += SC_THREADS) (&mbs[0][0])[i] = tile[i];
            __syncthreads();
            const uint32_t *__restrict__ ma = bits + (int64_t)ta * WORDS;
            for (int64_t cb = 0; cb < a.ncs; cb += CPL * CV_CHUNK) {
                uint32_t q[CPL][WORDS];
#pragma unroll
                for (int j = 0; j < CPL; ++j)
#pragma unroll
                    for (int w = 0; w < WORDS; ++w)
                        q[j][w] = bitsC[(int64_t)w * a.ncs + cb + j * CV_CHUNK + threadIdx.x] & ma[w];
                for (unsigned long long m = act; m; m &= m - 1) {
                    const int bi = __builtin_ctzll(m);
                    uint32_t t[CPL] = {};
#pragma unroll
                    for (int w4 = 0; w4 < WORDS / 4; ++w4) {
                        const uint4 v = mbs[bi][w4];
                        const uint32_t mb[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int j = 0; j < CPL; ++j)
#pragma unroll
                            for (int x = 0; x < 4; ++x) {
                                if constexpr (COUNT) t[j] += __popc(q[j][4 * w4 + x] & mb[x]);
                                else t[j] |= q[j][4 * w4 + x] & mb[x];
                            }
                    }
                    int cnt = 0;
#pragma unroll
                    for (int j = 0; j < CPL; ++j) cnt += __popcll(__ballot(COUNT ? t[j] >= (uint32_t)a.k : t[j] != 0));
                    acc += lane == bi ? cnt : 0;
                }
            }
        }
        cv_epilogue(a, red, acc, act, ri, ta, b0);
    }
}

// the same walk with M[c] read word by word from bitsC: any number of trees
template <bool COUNT>
__global__ void __launch_bounds__(SC_THREADS) k_cv_stream(cv_args a, const uint32_t *__restrict__ bits,
                                                          const uint32_t *__restrict__ bitsC) {
    __shared__ int red[SC_THREADS / 64][CV_TILE];
    const int lane = threadIdx.x & 63;
    for (int64_t idx = blockIdx.x; idx < a.n_items; idx += gridDim.x) {
        int64_t ri;
        int32_t ta, b0;
        if (!cv_item(a, idx, ri, ta, b0)) continue;
        const unsigned long long act = cv_prologue(a, bits, ri, ta, b0);
        int acc = 0;
        if (act) {
            const uint32_t *__restrict__ ma = bits + (int64_t)ta * a.wp;
            for (int64_t cb = 0; cb < a.ncs; cb += CV_CHUNK) {
                const uint32_t *__restrict__ mc = bitsC + cb + threadIdx.x;
                for (unsigned long long m = act; m; m &= m - 1) {
                    const int bi = __builtin_ctzll(m);
                    const uint32_t *__restrict__ mb = bits + (int64_t)(b0 + bi) * a.wp;
                    uint32_t t = 0;
                    for (int w = 0; w < a.W; ++w) {
                        const uint32_t x = mc[(int64_t)w * a.ncs] & ma[w] & mb[w];
                        if constexpr (COUNT) t += __popc(x);
                        else t |= x;
                    }
                    const int cnt = __popcll(__ballot(COUNT ? t >= (uint32_t)a.k : t != 0));
                    acc += lane == bi ? cnt : 0;
                }
            }
        }
        cv_epilogue(a, red, acc, act, ri, ta, b0);
    }
}

// one thread per leaf of the tables: flags 1 a taxon out of range, 4 a taxon twice in one tree
__global__ void k_cv_scatter(const int64_t *__restrict__ off, int M, const int32_t *__restrict__ leaf_taxon,
                             int32_t n_taxa, uint32_t *__restrict__ bits, int64_t wp, uint32_t *__restrict__ bitsT,
                             int64_t n_pad, unsigned *__restrict__ flags) {
    const int64_t p = off[0] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= off[M]) return;
    const int t = sc_tree_of(off, M, p);
    const int32_t x = leaf_taxon[p];
    if (x < 0 || x >= n_taxa) {
        atomicOr(flags, 1u);
        return;
    }
    const uint32_t bit = 1u << (t & 31);
    if (atomicOr(bits + (int64_t)x * wp + (t >> 5), bit) & bit) atomicOr(flags, 4u);
    atomicOr(bitsT + (int64_t)(t >> 5) * n_pad + x, bit);
}

__global__ void k_cv_occurs(const uint32_t *__restrict__ bitsT, int64_t n_pad, int W, int32_t n,
                            int32_t *__restrict__ occurs) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    int c = 0;
    for (int w = 0; w < W; ++w) c += __popc(bitsT[(int64_t)w * n_pad + x]);
    occurs[x] = c;
}

// bitsC[w][i] = bitsT[w][clist[i]] for the nc compact taxa (the block's memset left the rest of a row zeros)
__global__ void k_cv_compact(const uint32_t *__restrict__ bitsT, int64_t n_pad, int W, const int32_t *__restrict__ clist,
                             int64_t nc, uint32_t *__restrict__ bitsC, int64_t ncs) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const int32_t x = clist[i];
    for (int w = 0; w < W; ++w) bitsC[(int64_t)w * ncs + i] = bitsT[(int64_t)w * n_pad + x];
}

// The plan of a call: the words, the sweep variant, the row batches
struct cv_plan {
    int32_t W = 1;          // words of a taxon: ceil(trees / 32), at least 1
    int variant = 0;        // WORDS of k_cv_sweep (4 / 8 / 16 / 32 / 64); 0: k_cv_stream
    int64_t wp = 1;         // stride of a row of bits, and the rows of bitsC
    int64_t n_pad = 0;      // stride of a row of bitsT: n rounded up to 64
    int64_t ncs_max = 0;    // stride of a row of bitsC at most: n rounded up to 2 CV_CHUNK
    int32_t nt = 0;         // tiles of a row
    int64_t per_row = 0;    // bytes a row adds to the block: its total and its cells of the matrices wanted
    int64_t fixed = 0;      // bytes of the block without the rows' matrices
    int64_t batch_rows = 0; // rows of a batch at most
    int mirror = 0;
    int64_t grid_limit = 0, rows_per_launch = 0;
    std::vector<int64_t> bstart;  // first row of every batch, and n_rows
};

struct cv_block {
    unsigned *flag;
    int32_t *rows, *occurs, *clist, *out;
    unsigned long long *rowsum;
    uint32_t *bits, *bitsT, *bitsC;
};

// (out_rows: the rows the matrices hold at once)
size_t cv_carve(sc_carver &w, const cv_plan &p, size_t n, size_t n_rows, size_t n_mat, size_t out_rows, cv_block &k) {
    k.flag = w.take<unsigned>(1);
    k.rows = w.take<int32_t>(n_rows);
    k.occurs = w.take<int32_t>(n);
    k.clist = w.take<int32_t>(n);
    k.rowsum = w.take<unsigned long long>(std::max(n_rows, n));
    k.bits = w.take<uint32_t>((size_t)std::max<int64_t>(n, 1) * p.wp);
    k.bitsT = w.take<uint32_t>((size_t)p.W * p.n_pad);
    k.bitsC = w.take<uint32_t>((size_t)p.wp * p.ncs_max);
    k.out = w.take<int32_t>(n_mat * out_rows * n);
    return w.at;
}

// variant: the smallest of 4 / 8 / 16 / 32 / 64 words that holds W, unless that is past the cap (CV_REG_WORDS_MAX,
// or max_reg_words below it).  Row batches by bytes against SC_BUDGET, or max_batch_rows.  `mirror` (only a < b is
// swept, both cells written) when the rows are all taxa and the matrices, if wanted, hold every row at once.
cv_plan cv_plan_of(int32_t M, int32_t n, int64_t n_rows, bool all_rows, int32_t max_batch_rows, int32_t max_reg_words,
                   int n_mat) {
    cv_plan p;
    p.W = std::max<int32_t>((int32_t)(((int64_t)M + 31) / 32), 1);
    const int cap = max_reg_words > 0 ? std::min(max_reg_words, CV_REG_WORDS_MAX) : CV_REG_WORDS_MAX;
    int v = 4;
    while (v < p.W && v < CV_REG_WORDS_MAX) v *= 2;
    p.variant = (v >= p.W && v <= cap) ? v : 0;
    p.wp = p.variant ? p.variant : p.W;
    p.n_pad = scs_round_up(std::max<int64_t>(n, 1), 64);
    p.ncs_max = scs_round_up(std::max<int64_t>(n, 1), 2 * CV_CHUNK);
    p.nt = (int32_t)(((int64_t)n + CV_TILE - 1) / CV_TILE);
    p.per_row = 8 + (int64_t)n_mat * 4 * n;
    p.batch_rows = std::max<int64_t>(1, (int64_t)(SC_BUDGET / (uint64_t)p.per_row));
    if (max_batch_rows > 0) p.batch_rows = std::min<int64_t>(p.batch_rows, max_batch_rows);
    for (int64_t r = 0; r < n_rows; r += p.batch_rows) p.bstart.push_back(r);
    p.bstart.push_back(n_rows);
    if (n_rows == 0) p.bstart.assign(1, 0);
    p.mirror = all_rows && (n_mat == 0 || p.bstart.size() <= 2);
    p.grid_limit = sp_grid_limit(SC_THREADS);
    p.rows_per_launch = std::max<int64_t>(p.grid_limit / std::max<int32_t>(p.nt, 1), 1);
    cv_block k;
    sc_carver sizing;
    p.fixed = (int64_t)cv_carve(sizing, p, (size_t)n, (size_t)n_rows, 0, 0, k);
    return p;
}

// rows the matrices hold at once, and the workgroups of the first launch of a batch of nr rows
int64_t cv_out_rows(const cv_plan &p, int64_t n_rows) { return std::min<int64_t>(p.batch_rows, n_rows); }
int64_t cv_grid(const cv_plan &p, int64_t nr) {
    return std::min<int64_t>(std::min(nr, p.rows_per_launch) * p.nt, p.grid_limit);
}

template <bool COUNT>
void cv_launch(const cv_plan &p, const cv_args &a, unsigned grid, const uint32_t *bits, const uint32_t *bitsC,
               hipStream_t s) {
    switch (p.variant) {
    case 4: k_cv_sweep<4, COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    case 8: k_cv_sweep<8, COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    case 16: k_cv_sweep<16, COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    case 32: k_cv_sweep<32, COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    case 64: k_cv_sweep<64, COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    default: k_cv_stream<COUNT><<<grid, SC_THREADS, 0, s>>>(a, bits, bitsC); break;
    }
}

}  // namespace

extern "C" int scs_score_coverage(scs_ctx *ctx, const scs_tables *src, int32_t n_rows, const int32_t *rows,
                                  int32_t min_trees, int32_t max_batch_rows, int32_t max_reg_words, int32_t *occurs,
                                  int32_t *pair_trees, int32_t *pair_covered, int64_t *taxon_covered) {
    const char *const who = "scs_score_coverage";
    SCS_REQUIRE(ctx && src, "%s: null argument", who);
    const int32_t M = src->n_trees, n = src->n_taxa;
    SCS_REQUIRE(min_trees >= 1, "%s: min_trees = %d is less than 1", who, min_trees);
    SCS_REQUIRE(n_rows >= 0, "%s: n_rows = %d is negative", who, n_rows);
    SCS_REQUIRE(rows || n_rows == n, "%s: rows is null and n_rows = %d is not the %d taxa of the tables", who, n_rows,
                n);
    SCS_REQUIRE(max_batch_rows >= 0, "%s: max_batch_rows = %d is negative", who, max_batch_rows);
    SCS_REQUIRE(max_reg_words >= 0, "%s: max_reg_words = %d is negative", who, max_reg_words);
    for (int32_t r = 0; r < n_rows && rows; ++r)
        SCS_REQUIRE(rows[r] >= 0 && rows[r] < n, "%s: rows[%d] = %d is not a taxon of the tables (%d taxa)", who, r,
                    rows[r], n);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, src));  // (late chunks of a page-locked upload: all of them are read)
    if (n == 0) return SCS_OK;
    const std::vector<int64_t> &off = src->h_tree_off;
    const int n_mat = (pair_trees != nullptr) + (pair_covered != nullptr);
    const cv_plan p = cv_plan_of(M, n, n_rows, rows == nullptr, max_batch_rows, max_reg_words, n_mat);
    const size_t out_rows = (size_t)cv_out_rows(p, n_rows);
    cv_block k;
    sc_carver sizing;
    const size_t bytes = cv_carve(sizing, p, (size_t)n, (size_t)n_rows, (size_t)n_mat, out_rows, k);
    void *block = nullptr;
    SCS_TRY(scs_block_alloc(ctx, bytes, &block));
    sc_carver carve{(char *)block, bytes};
    cv_carve(carve, p, (size_t)n, (size_t)n_rows, (size_t)n_mat, out_rows, k);
    int32_t *const d_pt = pair_trees ? k.out : nullptr;
    int32_t *const d_pc = pair_covered ? k.out + (pair_trees ? out_rows * (size_t)n : 0) : nullptr;
    hipStream_t s = ctx->stream;
    unsigned bad = 0;
    std::vector<int32_t> h_occurs((size_t)n), clist;
    std::vector<unsigned long long> h_sum((size_t)n_rows);
    // flag, rows, occurs, clist, totals and the three bit matrices are zeros to begin with
    hipError_t e = hipMemsetAsync(block, 0, (size_t)p.fixed, s);
    if (e == hipSuccess && rows && n_rows)
        e = hipMemcpyAsync(k.rows, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, s);
    const int64_t leaves = M > 0 ? off[M] - off[0] : 0;
    if (e == hipSuccess && leaves > 0) {
        k_cv_scatter<<<grid_of(leaves), SC_THREADS, 0, s>>>(src->d_tree_off, M, src->d_leaf_taxon, n, k.bits, p.wp,
                                                           k.bitsT, p.n_pad, k.flag);
        sc_launched(e);
    }
    if (e == hipSuccess) {
        k_cv_occurs<<<grid_of(n), SC_THREADS, 0, s>>>(k.bitsT, p.n_pad, p.W, n, k.occurs);
        sc_launched(e);
    }
    // every tree's taxa are checked before a sweep kernel reads a row by them
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, k.flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h_occurs.data(), k.occurs, (size_t)n * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess && !bad && n_rows > 0) {
        // a taxon c in fewer than k trees covers nothing: the walk is over the others
        for (int32_t x = 0; x < n; ++x)
            if (h_occurs[x] >= min_trees) clist.push_back(x);
        const int64_t nc = (int64_t)clist.size(), ncs = scs_round_up(nc, 2 * CV_CHUNK);
        if (nc > 0) {
            e = hipMemcpyAsync(k.clist, clist.data(), (size_t)nc * 4, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) {
                k_cv_compact<<<grid_of(nc), SC_THREADS, 0, s>>>(k.bitsT, p.n_pad, p.W, k.clist, nc, k.bitsC, ncs);
                sc_launched(e);
            }
        }
        cv_args a{};
        a.rows = rows ? k.rows : nullptr;
        a.n = n;
        a.nt = p.nt;
        a.W = p.W;
        a.wp = p.wp;
        a.ncs = ncs;
        a.k = min_trees;
        a.mirror = p.mirror;
        a.pair_trees = d_pt;
        a.pair_covered = d_pc;
        a.rowsum = k.rowsum;
        for (size_t b = 0; b + 1 < p.bstart.size() && e == hipSuccess; ++b) {
            const int64_t r0 = p.bstart[b], nr = p.bstart[b + 1] - r0;
            a.out_r0 = r0;
            if (n_mat) e = hipMemsetAsync(k.out, 0, (size_t)n_mat * out_rows * n * 4, s);
            for (int64_t l0 = 0; l0 < nr && e == hipSuccess; l0 += p.rows_per_launch) {
                const int64_t lr = std::min(p.rows_per_launch, nr - l0);
                a.r0 = r0 + l0;
                a.n_items = lr * p.nt;
                const unsigned grid = (unsigned)std::min(a.n_items, p.grid_limit);
                if (min_trees > 1) cv_launch<true>(p, a, grid, k.bits, k.bitsC, s);
                else cv_launch<false>(p, a, grid, k.bits, k.bitsC, s);
                sc_launched(e);
            }
            if (e == hipSuccess && pair_trees)
                e = hipMemcpyAsync(pair_trees + (size_t)r0 * n, d_pt, (size_t)nr * n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && pair_covered)
                e = hipMemcpyAsync(pair_covered + (size_t)r0 * n, d_pc, (size_t)nr * n * 4, hipMemcpyDeviceToHost, s);
            // (the next batch's memset follows the copies on the stream)
        }
        if (e == hipSuccess && taxon_covered)
            e = hipMemcpyAsync(h_sum.data(), k.rowsum, (size_t)n_rows * 8, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) (void)hipStreamSynchronize(s);  // (nothing may still write into the block)
    scs_block_release(ctx, block);
    if (e != hipSuccess) {
        scs_set_error("%s: %s", who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCS_ENOMEM : SCS_EHIP;
    }
    SCS_REQUIRE(!bad, "%s: %s", who,
                (bad & 1u) ? "a leaf_taxon entry is out of range [0, n_taxa)" : "a source tree has a taxon twice");
    if (occurs) std::copy(h_occurs.begin(), h_occurs.end(), occurs);
    for (int32_t r = 0; r < n_rows && taxon_covered; ++r) taxon_covered[r] = (int64_t)(h_sum[r] / 2);
    return SCS_OK;
}

// the plan of one scs_score_coverage call on the host, by the functions the export calls
extern "C" int scs_debug_coverage_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off, int32_t n_taxa,
                                       int32_t n_rows, int32_t min_trees, int32_t max_batch_rows,
                                       int32_t max_reg_words, int32_t matrices_wanted, int64_t *info_out,
                                       int64_t *batches_out) {
    const char *const who = "scs_debug_coverage_plan";
    SCS_REQUIRE(info_out, "%s: null argument", who);
    (void)tree_off;  // (the plan reads the tree count only)
    SCS_REQUIRE(!src || n_trees == src->n_trees, "%s: the tables hold %d trees, not %d", who, src ? src->n_trees : 0,
                n_trees);
    SCS_REQUIRE(n_trees >= 0 && n_taxa >= 0 && max_batch_rows >= 0 && max_reg_words >= 0, "%s: negative argument", who);
    SCS_REQUIRE(min_trees >= 1, "%s: min_trees = %d is less than 1", who, min_trees);
    SCS_REQUIRE(matrices_wanted >= 0 && matrices_wanted <= 2, "%s: matrices_wanted = %d is not 0, 1 or 2", who,
                matrices_wanted);
    const int32_t n = src ? src->n_taxa : n_taxa;
    const bool all_rows = n_rows < 0;  // (n_rows < 0 stands for rows NULL: every taxon)
    const int64_t nr = all_rows ? n : n_rows;
    const cv_plan p = cv_plan_of(n_trees, n, nr, all_rows, max_batch_rows, max_reg_words, matrices_wanted);
    const int64_t nb = (int64_t)p.bstart.size() - 1;
    const int64_t info[12] = {p.W, p.variant, p.wp, p.n_pad, p.nt, p.per_row, p.fixed, nb, p.grid_limit,
                              p.rows_per_launch, p.mirror, min_trees > 1};
    std::copy(info, info + 12, info_out);
    for (int64_t b = 0; b < nb && batches_out; ++b) {
        const int64_t rows_b = p.bstart[b + 1] - p.bstart[b];
        const int64_t row[4] = {p.bstart[b], rows_b,
                                p.fixed + (int64_t)sc_up256((size_t)matrices_wanted * cv_out_rows(p, nr) * n * 4),
                                cv_grid(p, rows_b)};
        std::copy(row, row + 4, batches_out + 4 * b);
    }
    return SCS_OK;
}
