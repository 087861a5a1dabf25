// The batched small-node solve of the recursion's deep levels: small_batch, the k_small_* and pack kernels,
// small_solve_begin_impl and the begin / end entries.  Included by scs_eig.hip behind scs_fiedler (one translation
// unit: the Jacobi device routines and dbuf are the ones defined there).

// ---------------------------------------------------------------------------
// batched small nodes: tables -> W -> contraction -> S -> Jacobi -> maps
// ---------------------------------------------------------------------------
// Deep levels of the recursion are thousands of nodes of a few to a few dozen taxa
// (reference: scs.py:110-134 at depth; 47 spectral calls with V <= 100 in the reference's
// supertriplets fixture), each with up to thousands of trees, and at any moment the recursion
// knows only a handful of them (the children of the node it has just split).  A launch per
// node with one workgroup walking the node's trees one after the other left the other 255
// CUs idle for milliseconds (round 2: 3.2 us per tree, 16 ms for a 60-taxon node of 5 000
// trees).  Round 3 spreads ONE node over the chip without giving up the tree-ordered sums:
//   k_small_addends  the trees of a node are dealt to workgroups in runs; a workgroup stages
//                    four trees at a time (one per wave: sparse table over the gaps' depths by
//                    wave shuffles) and every thread writes, for its cells (x, y) and each
//                    tree, the ADDEND value(LCA) * weight -- rounded on its own, 0 when the
//                    tree does not join the two taxa -- to addends[tree][cell];
//   k_small_sum      one thread per cell adds its addends in tree order: the reference's sum
//                    (scs.py:644-658; x + 0.0 == x, so the zeros change nothing), bit-identical
//                    to scs_pcg_build's W; the dependent chain is one fp64 add per tree;
//   k_small_finish   one workgroup per node, in LDS: contraction max-reduce over consecutive id
//                    ranges, scipy's degree scaling, the full Jacobi eigen-decomposition and
//                    scikit-learn's embedding conventions.
// K nodes = three launches, one upload, one download.
struct small_batch {
    const int32_t *n_taxa;      // [K] taxa of the node (<= MAXS)
    const int32_t *n_trees;     // [K]
    const int32_t *n_groups;    // [K] vertices after contraction (>= 2)
    const int32_t *tree_ptr;    // [K+1] first tree of node k in tree_w; its tree_off starts at tree_ptr[k] + k
    const int64_t *leaf_ptr;    // [K+1] first leaf slot of node k
    const int32_t *vertex_ptr;  // [K+1] first vertex of node k in maps; its group_start at vertex_ptr[k] + k
    const int32_t *tree_off;    // per node: n_trees + 1 leaf offsets relative to the node's first slot
    const int32_t *leaf_taxon;
    const int32_t *adj_depth;
    const double *adj_val;
    const double *tree_w;
    const int32_t *group_start;  // per node: n_groups + 1 entries, 0 .. n_taxa
    double *maps;                // [total vertices][2]
    double *lambda;              // [K][3]
    double *w_out;               // per node n_groups^2 doubles at w_ptr[k], or null
    const int64_t *w_ptr;
    // work items of k_small_addends: (node, first tree, end tree); of k_small_sum: (node, first cell)
    const int32_t *item_node, *item_t0, *item_t1;
    const int32_t *sum_node, *sum_e0;
    // [K] first addend of node k.  Nodes of at most SMALL_TR_MAX taxa: addends[add_ptr[k] + (x * v0 + y) * ms +
    // tree], ms = trees rounded up to even -- a cell's addends lie in tree order in ONE piece, which the one
    // thread of that cell streams with 16-byte loads (a node of 8 taxa has 28 cells: with the trees outermost
    // its few threads fetched a line per tree).  Larger nodes: addends[add_ptr[k] + tree * v0^2 + x * v0 + y]
    // -- hundreds of cells, neighbouring threads read neighbouring addresses (measured both ways:
    // tools/small_solve_bench.py).  The space reserved is v0^2 * ms either way.
    const int64_t *add_ptr;
    double *addends;
    const int64_t *w0_ptr;   // [K] the node's v0 x v0 uncontracted weights in w0
    double *w0;
};

constexpr int SMALL_Q = MAXS * MAXS / 256;  // cells of a thread at the largest node of the one-wave form
constexpr int SMALL_MAXS = 128;             // largest node of the batched path (round 4: was MAXS)
constexpr int SMALL_TR_MAX = 24;            // up to here a cell's addends are stored contiguously (small_batch::add_ptr)

// A node of 65 .. 128 taxa (round 4; SURVEY.md 8f rank 3 asks for V <= 128): the same three
// launches.  A tree restricted to such a node has up to 128 leaves -- two per lane while a wave
// stages it, the sparse table built level by level in LDS (seven levels, keys (depth << 7 | gap));
// a thread owns the cells of one column y and every other row x < y.
__device__ void small_addends_big(const small_batch &p, int k, int t0, int t1, unsigned (*s_sp)[7][SMALL_MAXS],
                                  double (*s_val)[SMALL_MAXS], int (*s_pos)[SMALL_MAXS]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int v0 = p.n_taxa[k];
    const int ncell = v0 * v0;
    const int32_t *toff = p.tree_off + p.tree_ptr[k] + k;
    const int64_t lbase = p.leaf_ptr[k];
    double *out = p.addends + p.add_ptr[k];
    const bool tr = v0 <= SMALL_TR_MAX;  // (never here: the big path starts above 64 taxa; kept for symmetry)
    const int64_t cs = tr ? (p.n_trees[k] + 1) & ~1 : 1;  // stride between two cells of a tree (small_batch::add_ptr)
    const int y = tid & 127, x0 = tid >> 7;
    for (int g = t0; g < t1; g += 4) {
        __syncthreads();  // the cells of the previous four trees are done with the buffers
        const int ts = g + wave;
        if (ts < t1) {
            const int off = toff[ts], n = toff[ts + 1] - off;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = lane + 64 * h;
                int f_dep = 0;
                double f_val = 0.0;
                if (i < n) {
                    f_dep = p.adj_depth[lbase + off + i];
                    f_val = p.adj_val[lbase + off + i];
                }
                // gap i = the LCA of leaves i and i + 1 (adj_* of leaf i), i < n - 1
                s_sp[wave][0][i] = i + 1 < n ? ((unsigned)f_dep << 7) | (unsigned)i : 0xFFFFFFFFu;
                s_val[wave][i] = f_val;
                s_pos[wave][i] = -1;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (one wave: its LDS operations are performed in order)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int i = lane + 64 * h;
                if (i < n) s_pos[wave][p.leaf_taxon[lbase + off + i]] = i;
            }
            for (int j = 1; j < 7; ++j) {
                if ((1 << j) >= n) break;  // (uniform) no pair of this tree is 2^j gaps apart
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                unsigned nk[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int i = lane + 64 * h, i2 = i + (1 << (j - 1));
                    const unsigned a = s_sp[wave][j - 1][i];
                    const unsigned b = i2 < SMALL_MAXS ? s_sp[wave][j - 1][i2] : 0xFFFFFFFFu;
                    nk[h] = b < a ? b : a;
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) s_sp[wave][j][lane + 64 * h] = nk[h];
            }
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) {
            const int t = g + j;
            if (t >= t1) break;
            const double wt = p.tree_w[p.tree_ptr[k] + t];
            double *row = tr ? out + t : out + (int64_t)t * ncell;
            const int py = y < v0 ? s_pos[j][y] : -1;
            for (int x = x0; x < y && y < v0; x += 2) {
                const int px = s_pos[j][x];
                const bool live = px >= 0 && py >= 0;
                const int lo = live ? (px < py ? px : py) : 0, hi = live ? (px < py ? py : px) : 1;
                const int lv = 31 - __clz(hi - lo);
                const unsigned ka = s_sp[j][lv][lo], kb = s_sp[j][lv][hi - (1 << lv)];
                // (leftmost on ties, as a left-to-right sweep finds it)
                const unsigned key = kb < ka ? kb : ka;
                const double mv = s_val[j][key & 127u];
                double add = 0.0;
                // the root (depth 0) separates the two: nothing to add
                if (live && (key >> 7) != 0) {
#pragma clang fp contract(off)
                    add = mv * wt;  // rounded on its own, never fused into the sum
                }
                row[(int64_t)(x * v0 + y) * cs] = add;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_small_addends(small_batch p) {
    // per wave one staged tree: sparse table over the gaps' (depth << 6 | gap) keys, the gaps'
    // values, the position of every taxon (-1: absent)
    __shared__ unsigned s_sp[4][7][SMALL_MAXS];
    __shared__ double s_val[4][SMALL_MAXS];
    __shared__ int s_pos[4][SMALL_MAXS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = p.item_node[blockIdx.x];
    const int t0 = p.item_t0[blockIdx.x], t1 = p.item_t1[blockIdx.x];
    const int v0 = p.n_taxa[k];
    if (v0 > MAXS) {
        small_addends_big(p, k, t0, t1, s_sp, s_val, s_pos);
        return;
    }
    const int ncell = v0 * v0;
    const int32_t *toff = p.tree_off + p.tree_ptr[k] + k;
    const int64_t lbase = p.leaf_ptr[k];
    double *out = p.addends + p.add_ptr[k];
    const bool tr = v0 <= SMALL_TR_MAX;
    const int64_t cs = tr ? (p.n_trees[k] + 1) & ~1 : 1;
    const int nq = (ncell + 255) / 256;
    int cx[SMALL_Q], cy[SMALL_Q];
#pragma unroll
    for (int q = 0; q < SMALL_Q; ++q) {
        const int e = tid + 256 * q;
        cx[q] = e / v0;
        cy[q] = e - cx[q] * v0;
        if (e >= ncell || cx[q] >= cy[q]) cx[q] = -1;  // not a cell of the upper triangle
    }
    for (int g = t0; g < t1; g += 4) {
        __syncthreads();  // the cells of the previous four trees are done with the buffers
        const int ts = g + wave;
        if (ts < t1) {
            const int off = toff[ts], n = toff[ts + 1] - off;
            int f_tax = 0, f_dep = 0;
            double f_val = 0.0;
            if (lane < n) {
                f_tax = p.leaf_taxon[lbase + off + lane];
                f_dep = p.adj_depth[lbase + off + lane];
                f_val = p.adj_val[lbase + off + lane];
            }
            // gap i = the LCA of leaves i and i + 1 (adj_* of leaf i), i < n - 1
            unsigned key = lane + 1 < n ? ((unsigned)f_dep << 6) | (unsigned)lane : 0xFFFFFFFFu;
            s_sp[wave][0][lane] = key;
#pragma unroll
            for (int j = 1; j < 6; ++j) {
                if ((1 << j) >= n) break;  // (uniform) no pair of this tree is 2^j gaps apart
                const unsigned other = __shfl_down(key, 1 << (j - 1), 64);
                if (lane + (1 << (j - 1)) < 64) key = other < key ? other : key;
                s_sp[wave][j][lane] = key;
            }
            s_val[wave][lane] = f_val;
            s_pos[wave][lane] = -1;
            if (lane < n) s_pos[wave][f_tax] = lane;  // (same wave: after the clearing store)
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = g + j;
            if (t >= t1) break;
            const double wt = p.tree_w[p.tree_ptr[k] + t];
            double *row = tr ? out + t : out + (int64_t)t * ncell;
#pragma unroll
            for (int q = 0; q < SMALL_Q; ++q) {
                if (q >= nq) break;  // (uniform) most nodes are tiny
                if (cx[q] < 0) continue;
                const int px = s_pos[j][cx[q]], py = s_pos[j][cy[q]];
                const bool live = px >= 0 && py >= 0;
                const int lo = live ? (px < py ? px : py) : 0, hi = live ? (px < py ? py : px) : 1;
                const int lv = 31 - __clz(hi - lo);
                const unsigned ka = s_sp[j][lv][lo], kb = s_sp[j][lv][hi - (1 << lv)];
                // (leftmost on ties, as a left-to-right sweep finds it)
                const unsigned key = kb < ka ? kb : ka;
                const double mv = s_val[j][key & 63u];
                double add = 0.0;
                // the root (depth 0) separates the two: nothing to add
                if (live && (key >> 6) != 0) {
#pragma clang fp contract(off)
                    add = mv * wt;  // rounded on its own, never fused into the sum
                }
                row[(int64_t)(tid + 256 * q) * cs] = add;
            }
        }
    }
}

// thread = one cell (x < y) of one node: its addends in tree order (reference: scs.py:655-657)
__global__ __launch_bounds__(256) void k_small_sum(small_batch p) {
    const int k = p.sum_node[blockIdx.x];
    const int e = p.sum_e0[blockIdx.x] + threadIdx.x;
    const int v0 = p.n_taxa[k], m = p.n_trees[k];
    const int ncell = v0 * v0;
    if (e >= ncell) return;
    const int x = e / v0, y = e - x * v0;
    double *w0 = p.w0 + p.w0_ptr[k];
    if (x == y) w0[e] = 0.0;
    if (x >= y) return;
    double acc = 0.0;
    int t = 0;
    // (the adds are one chain in tree order -- the reference's order, scs.py:656 -- but the LOADS need not wait
    // for it.  With 8 loads in flight the kernel took 190 us for 5 000 trees whatever the node's size, 625 round
    // trips, and a recursion runs it tens of thousands of times; tools/small_solve_bench.py)
    if (v0 <= SMALL_TR_MAX) {
        const int64_t ms = (m + 1) & ~1;
        const double *in = p.addends + p.add_ptr[k] + (int64_t)e * ms;  // 16-byte aligned: add_ptr and ms are even
        // two batches of 64 addends in flight: the next one's loads are issued before this one's adds
        if (t + 64 <= m) {
            double2 a[32], b[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) a[j] = *(const double2 *)(in + t + 2 * j);
            for (; t + 128 <= m; t += 64) {
#pragma unroll
                for (int j = 0; j < 32; ++j) b[j] = *(const double2 *)(in + t + 64 + 2 * j);
#pragma unroll
                for (int j = 0; j < 32; ++j) {
                    acc = acc + a[j].x;
                    acc = acc + a[j].y;
                }
#pragma unroll
                for (int j = 0; j < 32; ++j) a[j] = b[j];
            }
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                acc = acc + a[j].x;
                acc = acc + a[j].y;
            }
            t += 64;
        }
        for (; t + 8 <= m; t += 8) {
            double2 a[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = *(const double2 *)(in + t + 2 * j);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = acc + a[j].x;
                acc = acc + a[j].y;
            }
        }
        for (; t < m; ++t) acc = acc + in[t];
    } else {
        const double *in = p.addends + p.add_ptr[k] + e;
        for (; t + 32 <= m; t += 32) {
            double a[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) a[j] = in[(int64_t)(t + j) * ncell];
#pragma unroll
            for (int j = 0; j < 32; ++j) acc = acc + a[j];
        }
        for (; t < m; ++t) acc = acc + in[(int64_t)t * ncell];
    }
    w0[e] = acc;
    w0[y * v0 + x] = acc;
}

// NT = 256: the nodes of up to 24 vertices (the Jacobi variants written for 256 threads).  NT = 1 024 (round 5, late):
// the nodes of 25 .. 64 vertices -- everything up to the eigen-solve is done by the first 256 threads as it
// always was, the Jacobi sweeps spread their independent work items over all 1 024 (jacobi_eig_generic): the same
// bits, a solve of 64 vertices 1.5 -> 0.7 ms.  The host launches the instance(s) a batch needs.
template <int NT>
__global__ __launch_bounds__(NT) void k_small_finish(small_batch p) {
    __shared__ jacobi_lds s;
    __shared__ double s_dd[MAXS];
    __shared__ int s_gs[MAXS + 1];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const int v = p.n_groups[k], v0 = p.n_taxa[k];
    if (v0 > MAXS) return;  // k_small_finish_big's
    if ((v > 24) != (NT > 256)) return;  // the other instance's
    const bool first = tid < 256;  // the threads of the 256-thread form: every strided loop below is theirs
    double(*w0)[SLD] = s.e;  // the uncontracted weights live where Jacobi later keeps its vectors
    if (first && tid <= v) s_gs[tid] = p.group_start[p.vertex_ptr[k] + k + tid];
    {
        const double *src = p.w0 + p.w0_ptr[k];
        for (int e = tid; e < v0 * v0 && first; e += 256) w0[e / v0][e % v0] = src[e];
    }
    __syncthreads();
    // ---- contraction: vertex g = taxa [gs[g], gs[g+1]); weight = max over member pairs
    // (reference: scs.py:336-387), diagonal 0
    for (int e = tid; e < v * v && first; e += 256) {
        const int g = e / v, h = e - g * v;
        double best = 0.0;
        if (g != h) {
            best = w0[s_gs[g]][s_gs[h]];
            for (int r = s_gs[g]; r < s_gs[g + 1]; ++r)
                for (int c = s_gs[h]; c < s_gs[h + 1]; ++c) best = w0[r][c] > best ? w0[r][c] : best;
        }
        s.a[g][h] = best;
    }
    __syncthreads();
    if (p.w_out)
        for (int e = tid; e < v * v && first; e += 256) p.w_out[p.w_ptr[k] + e] = s.a[e / v][e % v];
    // ---- degrees as scipy takes them (column sums, rows in order; isolated -> 1)
    if (tid < v) {
        double d = 0.0;
        for (int i = 0; i < v; ++i) d = d + s.a[i][tid];
        s_dd[tid] = d == 0.0 ? 1.0 : sqrt(d);
    }
    __syncthreads();
    // S = (W / dd) / dd^T: two successive divisions (scipy/sparse/csgraph/_laplacian.py:552-557),
    // then the symmetric part (the two orders of division may differ in the last bit)
    double keep[(MAXS * MAXS + 255) / 256];
    {
        int q = 0;
        for (int e = tid; e < v * v && first; e += 256, ++q) {
            const int g = e / v, h = e - g * v;
            const double x = (s.a[g][h] / s_dd[h]) / s_dd[g];
            const double y = (s.a[h][g] / s_dd[g]) / s_dd[h];
            keep[q] = g == h ? 0.0 : 0.5 * (x + y);
        }
        __syncthreads();
        q = 0;
        for (int e = tid; e < v * v && first; e += 256, ++q) s.a[e / v][e % v] = keep[q];
    }
    __syncthreads();
    if (NT > 256) jacobi_eig_generic<NT>(s, v);
    else jacobi_eig(s, v);
    // ---- embedding: unit eigenvectors / dd, largest |entry| of each column positive, column 0
    // <-> the largest eigenvalue (sklearn/manifold/_spectral_embedding.py:373-376, 463)
    if (tid < 2) {
        const int col = s.perm[tid];
        int arg = 0;
        double best = -1.0;
        for (int i = 0; i < v; ++i) {
            const double x = fabs(s.e[i][col] / s_dd[i]);
            if (x > best) {
                best = x;
                arg = i;
            }
        }
        const double sg = s.e[arg][col] < 0.0 ? -1.0 : 1.0;
        double *out = p.maps + (int64_t)p.vertex_ptr[k] * 2 + tid;
        for (int i = 0; i < v; ++i) out[2 * i] = sg * (s.e[i][col] / s_dd[i]);
    }
    if (tid < 3) p.lambda[k * 3 + tid] = tid < v ? s.w[tid] : 0.0;
}

// The nodes of 65 .. 128 taxa of a batch, one workgroup each: contraction straight from the
// uncontracted weights in device memory into the one LDS array the one-sided Jacobi works in
// (dense path of scs_fiedler: (V + 1) x V doubles, 132 KB at 128), scipy's degree scaling in
// place (the contracted matrix is symmetric bit for bit, so every cell's two orders of division
// need only the cell itself), A = S + I, the sweeps, scikit-learn's embedding conventions.  A
// batch's workgroups of this kind run side by side on as many CUs: what the recursion's walk
// used to solve one node after the other with ~35 latency-bound LOBPCG iterations each.
__global__ __launch_bounds__(256) void k_small_finish_big(small_batch p) {
    extern __shared__ double dyn_lds[];
    double(*a)[DENSE2_LD] = (double(*)[DENSE2_LD])dyn_lds;
    __shared__ double s_dd[SMALL_MAXS], s_norm[SMALL_MAXS];
    __shared__ int s_gs[SMALL_MAXS + 1];
    __shared__ int s_rot, s_top[3];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    const int v = p.n_groups[k], v0 = p.n_taxa[k];
    if (v0 <= MAXS) return;  // k_small_finish's
    const int m = v + (v & 1);
    if (tid <= v) s_gs[tid] = p.group_start[p.vertex_ptr[k] + k + tid];
    __syncthreads();
    // ---- contraction: vertex g = taxa [gs[g], gs[g+1]); weight = max over member pairs
    // (reference: scs.py:336-387), diagonal 0; the padding row / column of an odd V is zero
    const double *w0 = p.w0 + p.w0_ptr[k];
    for (int e = tid; e < m * m; e += 256) {
        const int g = e / m, h = e - g * m;
        double best = 0.0;
        if (g != h && g < v && h < v) {
            best = w0[s_gs[g] * v0 + s_gs[h]];
            for (int r = s_gs[g]; r < s_gs[g + 1]; ++r)
                for (int c = s_gs[h]; c < s_gs[h + 1]; ++c) {
                    const double x = w0[r * v0 + c];
                    best = x > best ? x : best;
                }
        }
        a[g][h] = best;
    }
    __syncthreads();
    if (p.w_out)
        for (int e = tid; e < v * v; e += 256) p.w_out[p.w_ptr[k] + e] = a[e / v][e % v];
    // ---- degrees as scipy takes them (column sums, rows in order; isolated -> 1)
    if (tid < v) {
        double d = 0.0;
        for (int i = 0; i < v; ++i) d = d + a[i][tid];
        s_dd[tid] = d == 0.0 ? 1.0 : sqrt(d);
    }
    __syncthreads();
    // S = (W / dd) / dd^T: two successive divisions (scipy/sparse/csgraph/_laplacian.py:552-557),
    // then the symmetric part (the two orders of division may differ in the last bit); + I
    for (int e = tid; e < v * v; e += 256) {
        const int g = e / v, h = e - g * v;
        const double w = a[g][h];  // == a[h][g]
        const double x = (w / s_dd[h]) / s_dd[g];
        const double y = (w / s_dd[g]) / s_dd[h];
        a[g][h] = g == h ? 1.0 : 0.5 * (x + y);
    }
    __syncthreads();
    // Two vertices that share an edge: S = [[0, s], [s, 0]] with s = 1 up to its last bit, lambda = (s, -s), and
    // the second eigenvalue is the null direction of A = S + I -- a WANTED column whose norm is 0 (s == 1 exactly:
    // contracted weights 1, 4, 9, ...) or rounding noise, and the division by that norm below is 0 / 0.  Every other
    // wanted column is safe: with three vertices or more the trace of S is 0 and lambda_2 >= -1 / (V - 1), a norm
    // of at least 1 / 2; without an edge A = I.  So this one case is written down in closed form -- eigenvectors
    // (1, 1) / sqrt(2) and (1, -1) / sqrt(2) -- with the conventions of the general case below.
    // (the branch is uniform; a NaN weight takes it too and comes back as NaN eigenvalues, which the host refuses)
    if (v == 2 && a[0][1] != 0.0) {
        if (tid == 0) {
            const double s01 = a[0][1], r = 0.70710678118654752440;
            const double x0 = r / s_dd[0], x1 = r / s_dd[1];
            // the largest |entry| of a column positive, the first one on a tie
            const double sg = x1 > x0 ? -1.0 : 1.0;
            double *out = p.maps + (int64_t)p.vertex_ptr[k] * 2;
            out[0] = x0;
            out[2] = x1;
            out[1] = sg * x0;
            out[3] = -sg * x1;
            p.lambda[k * 3 + 0] = s01;
            p.lambda[k * 3 + 1] = -s01;
            p.lambda[k * 3 + 2] = 0.0;
        }
        return;
    }
    const bool ok = onesided_sweeps(a, m, &s_rot);
    // eigenvalues of S: column norms - 1 (the padding column of an odd V has norm 0: last)
    if (tid < v) {
        double s2 = 0.0;
        for (int r = 0; r < v; ++r) s2 = fma(a[r][tid], a[r][tid], s2);
        s_norm[tid] = sqrt(s2);
    }
    __syncthreads();
    if (tid < v) {
        const double mine = s_norm[tid];
        int rank = 0;
        for (int j = 0; j < v; ++j) {
            const double o = s_norm[j];
            if (o > mine || (o == mine && j < tid)) ++rank;
        }
        if (rank < 3) s_top[rank] = tid;
    }
    __syncthreads();
    // ---- embedding: unit eigenvectors / dd, largest |entry| of each column positive, column 0
    // <-> the largest eigenvalue (sklearn/manifold/_spectral_embedding.py:373-376, 463)
    if (tid < 2) {
        const int col = s_top[tid];
        const double nrm = s_norm[col];
        int arg = 0;
        double best = -1.0;
        for (int i = 0; i < v; ++i) {
            const double x = fabs((a[i][col] / nrm) / s_dd[i]);
            if (x > best) {
                best = x;
                arg = i;
            }
        }
        const double sg = a[arg][col] < 0.0 ? -1.0 : 1.0;
        double *out = p.maps + (int64_t)p.vertex_ptr[k] * 2 + tid;
        for (int i = 0; i < v; ++i) out[2 * i] = sg * ((a[i][col] / nrm) / s_dd[i]);
    }
    // (sweeps that did not converge: NaN eigenvalues -- the host refuses the node)
    if (tid < 3) p.lambda[k * 3 + tid] = !ok ? __longlong_as_double(0x7FF8000000000000ll)
                                             : (tid < v ? s_norm[s_top[tid]] - 1.0 : 0.0);
}

// leaf arrays of ONE node straight from a forest's device tables into the batch's device block
// (taxa renumbered through `relabel` when the node numbers them differently -- present taxa only,
// contraction groups made consecutive), offsets narrowed to 32 bits
__global__ void k_small_pack(const int64_t *__restrict__ tree_off64, const int32_t *__restrict__ leaf_taxon,
                             const int32_t *__restrict__ adj_depth, const double *__restrict__ adj_val,
                             const double *__restrict__ tree_w, const int32_t *__restrict__ relabel,
                             int32_t n_trees, int64_t n_leaves, int32_t *__restrict__ to, int32_t *__restrict__ lt,
                             int32_t *__restrict__ ad, double *__restrict__ av, double *__restrict__ tw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_leaves) {
        const int32_t x = leaf_taxon[i];
        lt[i] = relabel ? relabel[x] : x;
        ad[i] = adj_depth[i];
        av[i] = adj_val[i];
    }
    if (i <= n_trees) to[i] = (int32_t)tree_off64[i];
    if (i < n_trees) tw[i] = tree_w[i];
}

// the same for the K nodes of a level (scs_small_solve_begin_level): node k owns the trees [t_begin[k],
// t_begin[k] + n_trees[k]) of the level forest and the taxon ids [u_base[k], u_base[k] + u_size[k]) of its
// universe; relabel (all nodes' maps, concatenated: rl_ptr[k] is node k's first entry) sends an id of that
// range to the node's own numbering
struct level_pack {
    const int32_t *t_begin, *u_base, *rl_ptr;  // device [K]
    const int32_t *relabel;                    // device, concatenated
    const int32_t *tree_ptr;                   // device [K + 1] first tree of node k in the batch
    const int64_t *leaf_ptr;                   // device [K + 1] first leaf slot of node k in the batch
};

__global__ void k_small_pack_level(const int64_t *__restrict__ tree_off64, const int32_t *__restrict__ leaf_taxon,
                                   const int32_t *__restrict__ adj_depth, const double *__restrict__ adj_val,
                                   const double *__restrict__ tree_w, level_pack lp, int32_t n_nodes, int64_t n_leaves,
                                   int32_t n_trees, int32_t *__restrict__ to, int32_t *__restrict__ lt,
                                   int32_t *__restrict__ ad, double *__restrict__ av, double *__restrict__ tw) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_leaves) {
        int32_t lo = 0, hi = n_nodes - 1;  // last k with leaf_ptr[k] <= i
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (lp.leaf_ptr[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const int64_t src = tree_off64[lp.t_begin[lo]] + (i - lp.leaf_ptr[lo]);
        lt[i] = lp.relabel[lp.rl_ptr[lo] + (leaf_taxon[src] - lp.u_base[lo])];
        ad[i] = adj_depth[src];
        av[i] = adj_val[src];
    }
    if (i < n_trees + n_nodes) {
        // node k's offsets sit at tree_ptr[k] + k .. tree_ptr[k + 1] + k (its trees + 1 entries)
        int32_t lo = 0, hi = n_nodes - 1;  // last k with tree_ptr[k] + k <= i
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (lp.tree_ptr[mid] + mid <= i) lo = mid;
            else hi = mid - 1;
        }
        const int32_t j = (int32_t)i - (lp.tree_ptr[lo] + lo);  // 0 .. trees of the node
        const int32_t t0 = lp.t_begin[lo];
        to[i] = (int32_t)(tree_off64[t0 + j] - tree_off64[t0]);
        if (j < lp.tree_ptr[lo + 1] - lp.tree_ptr[lo]) tw[lp.tree_ptr[lo] + j] = tree_w[t0 + j];
    }
}

struct level_src {
    const scs_forest *forest;
    const int32_t *t_begin, *u_base, *u_size;  // host [K]
    const int64_t *n_leaves;                   // host [K]
    const int32_t *relabel;                    // host, concatenated (sum of u_size entries)
};

static int small_solve_begin_impl(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa,
                                  const int32_t *n_trees, const int32_t *n_groups,
                                  const int32_t *tree_off, const int32_t *leaf_taxon,
                                  const int32_t *adj_depth, const double *adj_val,
                                  const double *tree_w, const int32_t *group_start, int32_t want_w,
                                  int32_t *ticket_out, const scs_forest *src, const int32_t *relabel,
                                  const level_src *lvl = nullptr);

// The K small nodes of one level of the recursion straight from the level forest's resident tables
// (scs_forest_split_level): nothing but the renumbering and the group boundaries travels.
extern "C" int scs_small_solve_begin_level(scs_ctx *ctx, const scs_forest *forest, int32_t n_nodes,
                                           const int32_t *t_begin, const int32_t *n_trees, const int64_t *n_leaves,
                                           const int32_t *u_base, const int32_t *u_size, const int32_t *relabel,
                                           const int32_t *n_taxa, const int32_t *n_groups,
                                           const int32_t *group_start, int32_t want_w, int32_t *ticket_out) {
    SCS_REQUIRE(ctx && forest && t_begin && n_trees && n_leaves && u_base && u_size && relabel && n_taxa && n_groups &&
                    group_start && ticket_out,
                "scs_small_solve_begin_level: null argument");
    SCS_REQUIRE(forest->has_tables, "scs_small_solve_begin_level: the forest carries no tables");
    for (int32_t k = 0; k < n_nodes; ++k) {
        SCS_REQUIRE(t_begin[k] >= 0 && n_trees[k] >= 1 && (int64_t)t_begin[k] + n_trees[k] <= forest->n_trees,
                    "scs_small_solve_begin_level: node %d: bad tree range", k);
        SCS_REQUIRE(u_base[k] >= 0 && u_size[k] >= 1 && (int64_t)u_base[k] + u_size[k] <= forest->n_taxa,
                    "scs_small_solve_begin_level: node %d: bad taxon range", k);
        SCS_REQUIRE(n_leaves[k] >= 2 * (int64_t)n_trees[k] && n_leaves[k] <= (int64_t)n_trees[k] * n_taxa[k],
                    "scs_small_solve_begin_level: node %d: bad leaf count", k);
    }
    level_src lvl{forest, t_begin, u_base, u_size, n_leaves, relabel};
    return small_solve_begin_impl(ctx, n_nodes, n_taxa, n_trees, n_groups, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  group_start, want_w, ticket_out, nullptr, nullptr, &lvl);
}

extern "C" int scs_small_solve_begin(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa,
                                     const int32_t *n_trees, const int32_t *n_groups,
                                     const int32_t *tree_off, const int32_t *leaf_taxon,
                                     const int32_t *adj_depth, const double *adj_val,
                                     const double *tree_w, const int32_t *group_start, int32_t want_w,
                                     int32_t *ticket_out) {
    SCS_REQUIRE(ctx && n_taxa && n_trees && n_groups && tree_off && leaf_taxon && adj_depth &&
                    adj_val && tree_w && group_start && ticket_out,
                "scs_small_solve: null argument");
    return small_solve_begin_impl(ctx, n_nodes, n_taxa, n_trees, n_groups, tree_off, leaf_taxon, adj_depth, adj_val,
                                  tree_w, group_start, want_w, ticket_out, nullptr, nullptr);
}

// ONE node whose tables are resident (a child of scs_forest_split): nothing but the group boundaries
// and the renumbering travels; the leaf arrays are packed on the device (k_small_pack)
extern "C" int scs_small_solve_begin_forest(scs_ctx *ctx, const scs_forest *forest, const int32_t *relabel,
                                            int32_t n_taxa, int32_t n_groups, const int32_t *group_start,
                                            int32_t want_w, int32_t *ticket_out) {
    SCS_REQUIRE(ctx && forest && group_start && ticket_out, "scs_small_solve_begin_forest: null argument");
    SCS_REQUIRE(forest->has_tables, "scs_small_solve_begin_forest: the forest carries no tables (not a child of scs_forest_split)");
    SCS_REQUIRE(forest->n_leaves <= INT32_MAX, "scs_small_solve_begin_forest: too many leaves");
    const int32_t n_trees = forest->n_trees;
    return small_solve_begin_impl(ctx, 1, &n_taxa, &n_trees, &n_groups, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  group_start, want_w, ticket_out, forest, relabel);
}

static int small_solve_begin_impl(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa,
                                  const int32_t *n_trees, const int32_t *n_groups,
                                  const int32_t *tree_off, const int32_t *leaf_taxon,
                                  const int32_t *adj_depth, const double *adj_val,
                                  const double *tree_w, const int32_t *group_start, int32_t want_w,
                                  int32_t *ticket_out, const scs_forest *src, const int32_t *relabel,
                                  const level_src *lvl) {
    const bool w_out = want_w != 0;
    SCS_REQUIRE(n_nodes >= 1, "scs_small_solve: need at least one node");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    // (a stream of its own: scs_internal.h)
    const bool own_stream = true;
    if (own_stream && !ctx->small_stream)
        SCS_HIP_CHECK(hipStreamCreateWithFlags(&ctx->small_stream, hipStreamNonBlocking));
    hipStream_t s = own_stream ? ctx->small_stream : ctx->stream;
    const int K = n_nodes;
    // ---- layout of the one staging block: [pointers | tree_off | group_start | leaf arrays |
    // tree_w], 8-byte aligned pieces
    std::vector<int32_t> tree_ptr(K + 1, 0), vertex_ptr(K + 1, 0);
    std::vector<int64_t> leaf_ptr(K + 1, 0), w_ptr(K + 1, 0);
    int64_t toff_at = 0;
    bool any_big = false;  // nodes of more than MAXS taxa: k_small_finish_big
    for (int k = 0; k < K; ++k) {
        SCS_REQUIRE(n_taxa[k] >= 2 && n_taxa[k] <= SMALL_MAXS, "scs_small_solve: node %d has %d taxa (2..%d)",
                    k, n_taxa[k], SMALL_MAXS);
        any_big = any_big || n_taxa[k] > MAXS;
        SCS_REQUIRE(n_groups[k] >= 2 && n_groups[k] <= n_taxa[k], "scs_small_solve: node %d: bad group count %d",
                    k, n_groups[k]);
        SCS_REQUIRE(n_trees[k] >= 1, "scs_small_solve: node %d has no tree", k);
        const int32_t *to = (src || lvl) ? nullptr : tree_off + toff_at;
        if (!src && !lvl) {
            SCS_REQUIRE(to[0] == 0, "scs_small_solve: node %d: tree_off must start at 0", k);
            for (int t = 0; t < n_trees[k]; ++t)
                SCS_REQUIRE(to[t + 1] >= to[t] && to[t + 1] - to[t] <= n_taxa[k],
                            "scs_small_solve: node %d tree %d: bad leaf range", k, t);
        }
        const int32_t *gs = group_start + vertex_ptr[k] + k;
        SCS_REQUIRE(gs[0] == 0 && gs[n_groups[k]] == n_taxa[k], "scs_small_solve: node %d: group_start must span the taxa", k);
        for (int g = 0; g < n_groups[k]; ++g)
            SCS_REQUIRE(gs[g] < gs[g + 1], "scs_small_solve: node %d: empty group %d", k, g);
        tree_ptr[k + 1] = tree_ptr[k] + n_trees[k];
        leaf_ptr[k + 1] = leaf_ptr[k] + (lvl ? lvl->n_leaves[k] : src ? src->n_leaves : (int64_t)to[n_trees[k]]);
        vertex_ptr[k + 1] = vertex_ptr[k] + n_groups[k];
        w_ptr[k + 1] = w_ptr[k] + (int64_t)n_groups[k] * n_groups[k];
        toff_at += n_trees[k] + 1;
    }
    const int64_t n_toff = toff_at, n_gs = vertex_ptr[K] + K, n_leaf = leaf_ptr[K], n_tree = tree_ptr[K];
    // ---- work items: runs of trees for k_small_addends (enough runs to fill the chip, at
    // least 16 trees each, whole groups of four), 256-cell pieces for k_small_sum
    int per_item = (int)std::max<int64_t>(16, (n_tree + 1023) / 1024);
    per_item = (per_item + 3) / 4 * 4;
    std::vector<int32_t> item_node, item_t0, item_t1, sum_node, sum_e0;
    std::vector<int64_t> add_ptr(K + 1, 0), w0_ptr(K + 1, 0);
    for (int k = 0; k < K; ++k) {
        const int64_t ncell = (int64_t)n_taxa[k] * n_taxa[k];
        add_ptr[k + 1] = add_ptr[k] + ncell * (((int64_t)n_trees[k] + 1) & ~(int64_t)1);
        w0_ptr[k + 1] = w0_ptr[k] + ncell;
        for (int t = 0; t < n_trees[k]; t += per_item) {
            item_node.push_back(k);
            item_t0.push_back(t);
            item_t1.push_back(std::min(n_trees[k], t + per_item));
        }
        for (int e = 0; e < ncell; e += 256) {
            sum_node.push_back(k);
            sum_e0.push_back(e);
        }
    }
    const size_t n_items = item_node.size(), n_sums = sum_node.size();
    SCS_REQUIRE((uint64_t)add_ptr[K] * 8 <= ((uint64_t)48 << 30),
                "scs_small_solve: batch too large (%lld addends): pass fewer nodes per call",
                (long long)add_ptr[K]);
    auto up8 = [](size_t x) { return (x + 7) & ~(size_t)7; };
    size_t at = 0;
    const size_t o_nt = at; at += up8((size_t)K * 4);
    const size_t o_nm = at; at += up8((size_t)K * 4);
    const size_t o_ng = at; at += up8((size_t)K * 4);
    const size_t o_tp = at; at += up8((size_t)(K + 1) * 4);
    const size_t o_vp = at; at += up8((size_t)(K + 1) * 4);
    const size_t o_lp = at; at += (size_t)(K + 1) * 8;
    const size_t o_wp = at; at += (size_t)(K + 1) * 8;
    const size_t o_ap = at; at += (size_t)(K + 1) * 8;
    const size_t o_w0p = at; at += (size_t)(K + 1) * 8;
    const size_t o_in = at; at += up8(n_items * 4);
    const size_t o_i0 = at; at += up8(n_items * 4);
    const size_t o_i1 = at; at += up8(n_items * 4);
    const size_t o_sn = at; at += up8(n_sums * 4);
    const size_t o_s0 = at; at += up8(n_sums * 4);
    const size_t o_to = at; at += up8((size_t)n_toff * 4);
    const size_t o_gs = at; at += up8((size_t)n_gs * 4);
    const size_t o_lt = at; at += up8((size_t)n_leaf * 4);
    const size_t o_ad = at; at += up8((size_t)n_leaf * 4);
    const size_t o_av = at; at += (size_t)n_leaf * 8;
    const size_t o_tw = at; at += (size_t)n_tree * 8;
    // (a resident node: the leaf arrays above are filled on the device; only the header travels --
    // up to o_to -- and the renumbering behind it)
    const size_t o_rl = at; if (src && relabel) at += up8((size_t)src->n_taxa * 4);
    // a level: t_begin | u_base | rl_ptr [K] each, then the concatenated renumbering
    std::vector<int32_t> rl_ptr(lvl ? K + 1 : 0, 0);
    for (int k = 0; lvl && k < K; ++k) rl_ptr[k + 1] = rl_ptr[k] + lvl->u_size[k];
    const size_t o_ltb = at; if (lvl) at += up8((size_t)K * 4);
    const size_t o_lub = at; if (lvl) at += up8((size_t)K * 4);
    const size_t o_lrp = at; if (lvl) at += up8((size_t)K * 4);
    const size_t o_lrl = at; if (lvl) at += up8((size_t)rl_ptr[K] * 4);
    const size_t in_bytes = at;
    const size_t o_maps = at; at += (size_t)vertex_ptr[K] * 16;
    const size_t o_lam = at; at += (size_t)K * 24;
    const size_t o_w = at; if (w_out) at += (size_t)w_ptr[K] * 8;
    const size_t total = at;
    // a free slot that is large enough (the smallest such), else the largest free one (grown), else
    // a new one
    int pick = -1;
    for (size_t i = 0; i < ctx->small_slots.size(); ++i) {
        const auto &c = ctx->small_slots[i];
        if (c.busy) continue;
        if (pick < 0) {
            pick = (int)i;
            continue;
        }
        const auto &p = ctx->small_slots[pick];
        const bool c_fits = c.cap >= total, p_fits = p.cap >= total;
        if ((c_fits && (!p_fits || c.cap < p.cap)) || (!c_fits && !p_fits && c.cap > p.cap)) pick = (int)i;
    }
    if (pick < 0) {
        ctx->small_slots.emplace_back();
        pick = (int)ctx->small_slots.size() - 1;
    }
    scs_ctx::small_slot &slot = ctx->small_slots[pick];
    if (slot.cap < total) {
        if (slot.dev) scs_dev_free(slot.dev);
        if (slot.host) hipHostFree(slot.host);
        slot.dev = nullptr;
        slot.host = nullptr;
        slot.cap = 0;
        const size_t cap = std::max<size_t>(total * 2, (size_t)1 << 20);
        SCS_HIP_CHECK(scs_dev_malloc(ctx, (void **)&slot.dev, cap));
        SCS_HIP_CHECK(hipHostMalloc((void **)&slot.host, cap, hipHostMallocDefault));
        slot.cap = cap;
    }
    if (!slot.done) SCS_HIP_CHECK(hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    // device scratch: the addends (trees x cells per node) and the uncontracted weights
    t_ctx = ctx;
    const size_t add_bytes = ((size_t)std::max<int64_t>(add_ptr[K], 1) * 8 + 255) / 256 * 256;
    const size_t w0_bytes = (size_t)std::max<int64_t>(w0_ptr[K], 1) * 8;
    if (slot.scratch_cap < add_bytes + w0_bytes) {
        if (slot.scratch) scs_dev_free(slot.scratch);
        slot.scratch = nullptr;
        slot.scratch_cap = 0;
        const size_t cap = std::max<size_t>((add_bytes + w0_bytes) * 3 / 2, (size_t)1 << 20);
        SCS_HIP_CHECK(scs_dev_malloc(ctx, (void **)&slot.scratch, cap));
        slot.scratch_cap = cap;
    }
    unsigned char *h = slot.host, *d = slot.dev;
    memcpy(h + o_nt, n_taxa, (size_t)K * 4);
    memcpy(h + o_nm, n_trees, (size_t)K * 4);
    memcpy(h + o_ng, n_groups, (size_t)K * 4);
    memcpy(h + o_tp, tree_ptr.data(), (size_t)(K + 1) * 4);
    memcpy(h + o_vp, vertex_ptr.data(), (size_t)(K + 1) * 4);
    memcpy(h + o_lp, leaf_ptr.data(), (size_t)(K + 1) * 8);
    memcpy(h + o_wp, w_ptr.data(), (size_t)(K + 1) * 8);
    memcpy(h + o_ap, add_ptr.data(), (size_t)(K + 1) * 8);
    memcpy(h + o_w0p, w0_ptr.data(), (size_t)(K + 1) * 8);
    memcpy(h + o_in, item_node.data(), n_items * 4);
    memcpy(h + o_i0, item_t0.data(), n_items * 4);
    memcpy(h + o_i1, item_t1.data(), n_items * 4);
    memcpy(h + o_sn, sum_node.data(), n_sums * 4);
    memcpy(h + o_s0, sum_e0.data(), n_sums * 4);
    memcpy(h + o_gs, group_start, (size_t)n_gs * 4);
    if (lvl) {
        // header and group boundaries, the level's per-node ranges and renumbering; the leaf arrays are
        // packed on the device from the level forest's tables
        memcpy(h + o_ltb, lvl->t_begin, (size_t)K * 4);
        memcpy(h + o_lub, lvl->u_base, (size_t)K * 4);
        memcpy(h + o_lrp, rl_ptr.data(), (size_t)K * 4);
        memcpy(h + o_lrl, lvl->relabel, (size_t)rl_ptr[K] * 4);
        SCS_HIP_CHECK(hipMemcpyAsync(d, h, o_to, hipMemcpyHostToDevice, s));
        SCS_HIP_CHECK(hipMemcpyAsync(d + o_gs, h + o_gs, up8((size_t)n_gs * 4), hipMemcpyHostToDevice, s));
        SCS_HIP_CHECK(hipMemcpyAsync(d + o_ltb, h + o_ltb, in_bytes - o_ltb, hipMemcpyHostToDevice, s));
        level_pack lp;
        lp.t_begin = (const int32_t *)(d + o_ltb);
        lp.u_base = (const int32_t *)(d + o_lub);
        lp.rl_ptr = (const int32_t *)(d + o_lrp);
        lp.relabel = (const int32_t *)(d + o_lrl);
        lp.tree_ptr = (const int32_t *)(d + o_tp);
        lp.leaf_ptr = (const int64_t *)(d + o_lp);
        const scs_forest *lf = lvl->forest;
        const int64_t work = std::max<int64_t>(n_leaf, n_tree + K);
        k_small_pack_level<<<(unsigned)((work + 255) / 256), 256, 0, s>>>(
            lf->tree_off, lf->leaf_taxon, lf->adj_depth, lf->adj_val, lf->weights, lp, K, n_leaf, (int32_t)n_tree,
            (int32_t *)(d + o_to), (int32_t *)(d + o_lt), (int32_t *)(d + o_ad), (double *)(d + o_av),
            (double *)(d + o_tw));
    } else if (!src) {
        memcpy(h + o_to, tree_off, (size_t)n_toff * 4);
        memcpy(h + o_lt, leaf_taxon, (size_t)n_leaf * 4);
        memcpy(h + o_ad, adj_depth, (size_t)n_leaf * 4);
        memcpy(h + o_av, adj_val, (size_t)n_leaf * 8);
        memcpy(h + o_tw, tree_w, (size_t)n_tree * 8);
        SCS_HIP_CHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    } else {
        // header and group boundaries (two small pieces around the leaf arrays), the renumbering
        SCS_HIP_CHECK(hipMemcpyAsync(d, h, o_to, hipMemcpyHostToDevice, s));
        SCS_HIP_CHECK(hipMemcpyAsync(d + o_gs, h + o_gs, up8((size_t)n_gs * 4), hipMemcpyHostToDevice, s));
        const int32_t *d_rl = nullptr;
        if (relabel) {
            memcpy(h + o_rl, relabel, (size_t)src->n_taxa * 4);
            SCS_HIP_CHECK(hipMemcpyAsync(d + o_rl, h + o_rl, (size_t)src->n_taxa * 4, hipMemcpyHostToDevice, s));
            d_rl = (const int32_t *)(d + o_rl);
        }
        const int64_t work = std::max<int64_t>(n_leaf, n_tree + 1);
        k_small_pack<<<(unsigned)((work + 255) / 256), 256, 0, s>>>(
            src->tree_off, src->leaf_taxon, src->adj_depth, src->adj_val, src->weights, d_rl, (int32_t)n_tree, n_leaf,
            (int32_t *)(d + o_to), (int32_t *)(d + o_lt), (int32_t *)(d + o_ad), (double *)(d + o_av),
            (double *)(d + o_tw));
    }
    small_batch sb;
    sb.n_taxa = (const int32_t *)(d + o_nt);
    sb.n_trees = (const int32_t *)(d + o_nm);
    sb.n_groups = (const int32_t *)(d + o_ng);
    sb.tree_ptr = (const int32_t *)(d + o_tp);
    sb.vertex_ptr = (const int32_t *)(d + o_vp);
    sb.leaf_ptr = (const int64_t *)(d + o_lp);
    sb.w_ptr = (const int64_t *)(d + o_wp);
    sb.add_ptr = (const int64_t *)(d + o_ap);
    sb.w0_ptr = (const int64_t *)(d + o_w0p);
    sb.item_node = (const int32_t *)(d + o_in);
    sb.item_t0 = (const int32_t *)(d + o_i0);
    sb.item_t1 = (const int32_t *)(d + o_i1);
    sb.sum_node = (const int32_t *)(d + o_sn);
    sb.sum_e0 = (const int32_t *)(d + o_s0);
    sb.tree_off = (const int32_t *)(d + o_to);
    sb.group_start = (const int32_t *)(d + o_gs);
    sb.leaf_taxon = (const int32_t *)(d + o_lt);
    sb.adj_depth = (const int32_t *)(d + o_ad);
    sb.adj_val = (const double *)(d + o_av);
    sb.tree_w = (const double *)(d + o_tw);
    sb.maps = (double *)(d + o_maps);
    sb.lambda = (double *)(d + o_lam);
    sb.w_out = w_out ? (double *)(d + o_w) : nullptr;
    sb.addends = (double *)slot.scratch;
    sb.w0 = (double *)(slot.scratch + add_bytes);
    k_small_addends<<<(unsigned)n_items, 256, 0, s>>>(sb);
    k_small_sum<<<(unsigned)n_sums, 256, 0, s>>>(sb);
    {
        bool any_small = false, any_mid = false;
        for (int k = 0; k < K; ++k) {
            if (n_taxa[k] > MAXS) continue;
            if (n_groups[k] > 24) any_mid = true;
            else any_small = true;
        }
        if (any_small) k_small_finish<256><<<K, 256, 0, s>>>(sb);
        if (any_mid) k_small_finish<1024><<<K, 1024, 0, s>>>(sb);
    }
    if (any_big) {
        // (every node gets a workgroup of either kind; the one that is not its own returns at once)
        SCS_HIP_CHECK(hipFuncSetAttribute((const void *)k_small_finish_big, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          DENSE2_MAX * DENSE2_LD * (int)sizeof(double)));
        k_small_finish_big<<<K, 256, (size_t)DENSE2_MAX * DENSE2_LD * sizeof(double), s>>>(sb);
    }
    SCS_HIP_CHECK(hipGetLastError());
    SCS_HIP_CHECK(hipMemcpyAsync(h + o_maps, d + o_maps, total - o_maps, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipEventRecord(slot.done, s));
    slot.busy = true;
    slot.o_maps = o_maps;
    slot.maps_bytes = (size_t)vertex_ptr[K] * 16;
    slot.o_lam = o_lam;
    slot.lam_bytes = (size_t)K * 24;
    slot.o_w = o_w;
    slot.w_bytes = w_out ? (size_t)w_ptr[K] * 8 : 0;
    slot.o_to = o_to;
    slot.o_lt = o_lt;
    slot.o_ad = o_ad;
    slot.o_av = o_av;
    slot.o_tw = o_tw;
    slot.n_toff = n_toff;
    slot.n_leaf = n_leaf;
    slot.n_tree = n_tree;
    *ticket_out = pick;
    return SCS_OK;
}

// The packed input arrays of a begun batch, copied from the slot's DEVICE block as k_small_addends reads them
// (n_toff, n_leaf, n_leaf, n_leaf and n_tree entries; any pointer may be null) -- whichever entry began the
// batch: packed on the host, by k_small_pack or by k_small_pack_level.  The ticket stays begun.
extern "C" int scs_debug_small_inputs(scs_ctx *ctx, int32_t ticket, int32_t *tree_off, int32_t *leaf_taxon,
                                      int32_t *adj_depth, double *adj_val, double *tree_w) {
    SCS_REQUIRE(ctx != nullptr, "scs_debug_small_inputs: null context");
    SCS_REQUIRE(ticket >= 0 && (size_t)ticket < ctx->small_slots.size() && ctx->small_slots[ticket].busy,
                "scs_small_solve_end: no such ticket (%d)", ticket);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    const scs_ctx::small_slot &slot = ctx->small_slots[ticket];
    // (the batch's kernels and its copy back have run: nothing of the slot's is in flight behind the event)
    SCS_HIP_CHECK(hipEventSynchronize(slot.done));
    const unsigned char *d = slot.dev;
    const size_t nl = (size_t)slot.n_leaf;
    if (tree_off && slot.n_toff) SCS_HIP_CHECK(hipMemcpy(tree_off, d + slot.o_to, (size_t)slot.n_toff * 4, hipMemcpyDeviceToHost));
    if (leaf_taxon && nl) SCS_HIP_CHECK(hipMemcpy(leaf_taxon, d + slot.o_lt, nl * 4, hipMemcpyDeviceToHost));
    if (adj_depth && nl) SCS_HIP_CHECK(hipMemcpy(adj_depth, d + slot.o_ad, nl * 4, hipMemcpyDeviceToHost));
    if (adj_val && nl) SCS_HIP_CHECK(hipMemcpy(adj_val, d + slot.o_av, nl * 8, hipMemcpyDeviceToHost));
    if (tree_w && slot.n_tree) SCS_HIP_CHECK(hipMemcpy(tree_w, d + slot.o_tw, (size_t)slot.n_tree * 8, hipMemcpyDeviceToHost));
    return SCS_OK;
}

extern "C" int scs_small_solve_end(scs_ctx *ctx, int32_t ticket, double *maps_out, double *lambda_out,
                                   double *w_out) {
    SCS_REQUIRE(ctx != nullptr, "scs_small_solve_end: null context");
    SCS_REQUIRE(ticket >= 0 && (size_t)ticket < ctx->small_slots.size() && ctx->small_slots[ticket].busy,
                "scs_small_solve_end: no such ticket (%d)", ticket);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    scs_ctx::small_slot &slot = ctx->small_slots[ticket];
    const hipError_t e = hipEventSynchronize(slot.done);
    slot.busy = false;  // (whatever happened: the slot is the caller's no longer)
    if (e != hipSuccess) {
        scs_set_error("scs_small_solve: %s", hipGetErrorString(e));
        return SCS_EHIP;
    }
    if (maps_out) memcpy(maps_out, slot.host + slot.o_maps, slot.maps_bytes);
    if (lambda_out) memcpy(lambda_out, slot.host + slot.o_lam, slot.lam_bytes);
    if (w_out && slot.w_bytes) memcpy(w_out, slot.host + slot.o_w, slot.w_bytes);
    return SCS_OK;
}

extern "C" int scs_small_solve(scs_ctx *ctx, int32_t n_nodes, const int32_t *n_taxa,
                               const int32_t *n_trees, const int32_t *n_groups,
                               const int32_t *tree_off, const int32_t *leaf_taxon,
                               const int32_t *adj_depth, const double *adj_val,
                               const double *tree_w, const int32_t *group_start, double *maps_out,
                               double *lambda_out, double *w_out) {
    SCS_REQUIRE(maps_out && lambda_out, "scs_small_solve: null output");
    int32_t ticket = -1;
    SCS_TRY(scs_small_solve_begin(ctx, n_nodes, n_taxa, n_trees, n_groups, tree_off, leaf_taxon, adj_depth,
                                  adj_val, tree_w, group_start, w_out != nullptr, &ticket));
    return scs_small_solve_end(ctx, ticket, maps_out, lambda_out, w_out);
}
