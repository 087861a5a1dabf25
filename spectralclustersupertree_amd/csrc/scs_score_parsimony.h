// scs_score_parsimony: the parsimony length of the supertree S on the Baum-Ragan (MRP) matrix of its sources
// (DESIGN.md section 32).  Included by scs_score.hip after its shared host layer: the kernels read the prepared batch
// view (sc_batch) and nothing of the other exports.
//
// Per source tree T on leaf set L, m = |L| >= 3: one binary character per nontrivial cluster C of T (state 1 on C,
// 0 on L - C, missing elsewhere), in the order of the clusters' first gaps in T's DFS order.  len(C) = the least
// number of changes on S with an all-zero outgroup above the root = the same on S' = S|L.
//   k_mp_list:   one workgroup per tree lists T's characters -- [lo, hi] in T positions, in first-gap order -- and
//                counts them and their star lengths gmax = min(|C|, m - |C| + 1).
//   k_mp_toggle / k_mp_scan: the membership tile of one pass, M[T position][word] (bit j of word w: the leaf lies in
//                character 64 w + j): every character toggles its bit at lo and at hi + 1, a prefix XOR along the
//                positions fills the interval.  8 wc bytes per leaf; a tree of more than 64 wc characters takes
//                several passes over the same tile.
//   k_mp_fold:   Hartigan's first pass, bit-parallel: one wave per tree, lane l holds word w0 + l of the pass.  The
//                wave walks the leaves of S' left to right (tp[k], dep[k]); a stack of open nodes (frames) folds the
//                children in postorder.  With m0 / m1 the children of a node whose state set lacks 0 / lacks 1, the
//                node costs min(m0, m1) and its set lacks 0 iff m0 > m1, lacks 1 iff m1 > m0.  A frame keeps only the
//                excess |m0 - m1| (bit-sliced, `bits` slices) and its direction: a child on the minority side lowers
//                the excess and costs one change at once, so every merge yields a 64-character cost mask.  The root
//                costs one more where its set lacks 0 (the outgroup).
// S is laid out for this export with every node's children sorted by tip count, largest first: the open frames are
// then the ancestors in which the next leaf lies in a child that is not the first, at most floor(log2(tips)) of them.
// The host counts them for the layout it made (`depth`), so the frames' size is exact, not an estimate.

namespace {

constexpr int MP_WAVE_WORDS = 64;      // words of one tree a pass covers at most: one lane each
constexpr int MP_LEN_BITS = 32;        // slices of the per-character length adder (a length is under 2^31)
constexpr int MP_LDS_MAX = 64 << 10;   // LDS the frames of a wave may take; more goes to the call's block
constexpr int MP_MAX_DEPTH = 32;       // frames of any supertree of int32 tips
constexpr unsigned SC_BAD_FRAMES = 32u;  // device flag: a fold opened more frames than the host planned

struct sc_mp_args : sc_batch {
    int32_t *clo, *chi;                  // [Lb] a tree's characters from its first leaf's slot on: T positions
    int32_t *clen;                       // [Lb] their lengths (the variant with per-character output)
    int32_t *ccnt;                       // [nb] characters per tree
    unsigned long long *tile;            // [Lb][wc] membership words of the pass
    int wc, w0;                          // words per leaf of the tile, first word of the pass
    int depth, bits;                     // frames a wave may open, slices of a frame's excess
    unsigned long long *frames;          // [nb][depth][bits + 1][64] where the frames do not fit LDS
    unsigned long long *c_chars, *c_len, *c_perfect, *c_max;  // [nb] of the batch
    unsigned *flags;
};

// T's characters: the first gaps of its non-root inner nodes, in order
__global__ void __launch_bounds__(SC_THREADS) k_mp_list(sc_mp_args a) {
    __shared__ int wave_sum[SC_THREADS / 64];
    __shared__ unsigned long long wave_max[SC_THREADS / 64];
    const int t = blockIdx.x;
    const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t done = 0;
    unsigned long long gmax = 0;
    for (int64_t c = 0; n >= 3 && c < n - 1; c += SC_THREADS) {
        const int64_t k = c + threadIdx.x;
        bool is = false;
        int64_t lo = 0, hi = 0;
        if (k + 1 < n) {
            const int32_t d = a.adj[base + k];
            lo = sc_stretch_left(a.adj, a.amin, a.Lb, a.levels, base, k, d, false);
            if (lo == 0 || a.adj[base + lo - 1] < d) {
                hi = sc_stretch_right(a.adj, a.amin, a.Lb, a.levels, base, k + 1, n - 1, d);
                is = lo > 0 || hi < n - 1;  // (not the root)
            }
        }
        const unsigned long long mask = __ballot(is);
        if (lane == 0) wave_sum[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < SC_THREADS / 64; ++w) {
            before += (w < wave) ? wave_sum[w] : 0;
            total += wave_sum[w];
        }
        if (is) {
            const int64_t idx = base + done + before + __popcll(mask & (((unsigned long long)1 << lane) - 1));
            a.clo[idx] = (int32_t)lo;
            a.chi[idx] = (int32_t)hi;
            const int64_t size = hi - lo + 1;
            gmax += (unsigned long long)min(size, n - size + 1);
        }
        done += total;
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) gmax += __shfl_down(gmax, d, 64);
    if (lane == 0) wave_max[wave] = gmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long g = 0;
        for (int w = 0; w < SC_THREADS / 64; ++w) g += wave_max[w];
        a.ccnt[t] = (int32_t)done;
        a.c_chars[t] = (unsigned long long)done;
        a.c_max[t] = g;
    }
}

// the pass's characters toggle their bit at the first position of their interval and after its last
__global__ void __launch_bounds__(SC_THREADS) k_mp_toggle(sc_mp_args a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // batch-relative slot of a character
    const int64_t p = a.off[0] + q;
    if (p >= a.off[a.nb]) return;
    const int t = sc_tree_of(a.off, a.nb, p);
    const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
    const int64_t j = q - base;
    if (j >= a.ccnt[t]) return;
    const int64_t w = (j >> 6) - a.w0;
    if (w < 0 || w >= a.wc) return;
    const unsigned long long bit = (unsigned long long)1 << (j & 63);
    const int64_t lo = a.clo[q], hi = a.chi[q];
    atomicXor(a.tile + (base + lo) * a.wc + w, bit);
    if (hi + 1 < n) atomicXor(a.tile + (base + hi + 1) * a.wc + w, bit);
}

// prefix XOR of every word column of a tree's tile along the T positions: one workgroup per tree, lane = word, the
// positions in one segment per wave (XOR of the segment, then the scan from the segments before it)
__global__ void __launch_bounds__(SC_THREADS) k_mp_scan(sc_mp_args a) {
    __shared__ unsigned long long seg[SC_THREADS / 64][64];
    const int t = blockIdx.x;
    const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
    const int act = min(a.wc, ((a.ccnt[t] + 63) >> 6) - a.w0);  // words of this tree in the pass
    if (act <= 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = lane < act;
    const int64_t per = (n + SC_THREADS / 64 - 1) / (SC_THREADS / 64);
    const int64_t i0 = min(n, wave * per), i1 = min(n, i0 + per);
    unsigned long long *col = a.tile + base * a.wc + lane;
    unsigned long long x = 0;
    if (on)
        for (int64_t i = i0; i < i1; ++i) x ^= col[i * a.wc];
    seg[wave][lane] = x;
    __syncthreads();
    unsigned long long pre = 0;
    for (int w = 0; w < wave; ++w) pre ^= seg[w][lane];
    if (on)
        for (int64_t i = i0; i < i1; ++i) {
            pre ^= col[i * a.wc];
            col[i * a.wc] = pre;
        }
}

// One child (state sets cur0 / cur1: bit set = the set holds 0 / 1) joins frame f of this lane: returns the cost
// mask, and the frame's new excess (any slice set) and direction for the caller that closes it.  fr: the wave's
// frames, slice i of frame f at fr[(f * (bits + 1) + i) * 64 + lane], the direction after the slices.
__device__ __forceinline__ unsigned long long mp_merge(unsigned long long *fr, int bits, int f, int lane,
                                                       unsigned long long cur0, unsigned long long cur1,
                                                       unsigned long long &nz_out, unsigned long long &dir_out) {
    unsigned long long *slot = fr + (int64_t)f * (bits + 1) * 64 + lane;
    const unsigned long long la = ~cur0, lb = ~cur1;  // the child lacks 0 / lacks 1 (never both)
    unsigned long long nz = 0;
    for (int i = 0; i < bits; ++i) nz |= slot[i * 64];
    const unsigned long long dir = slot[bits * 64];  // 1: more children lack 0 than lack 1
    const unsigned long long dec = nz & ((la & ~dir) | (lb & dir));
    unsigned long long carry = (la | lb) & ~dec, borrow = dec, nz2 = 0;
    for (int i = 0; i < bits; ++i) {
        const unsigned long long x = slot[i * 64], y = x ^ carry ^ borrow;
        slot[i * 64] = y;
        nz2 |= y;
        carry &= x;
        borrow &= ~x;
    }
    const unsigned long long dir2 = (dir & nz) | (la & ~nz);
    slot[bits * 64] = dir2;
    nz_out = nz2;
    dir_out = dir2;
    return dec;
}

template <bool CHARS, bool BLOCK>
__global__ void __launch_bounds__(64) k_mp_fold(sc_mp_args a) {
    extern __shared__ __align__(16) unsigned long long mp_lds[];
    __shared__ int fdep[MP_MAX_DEPTH];
    const int t = blockIdx.x;
    const int64_t base = a.off[t] - a.off[0], n = a.off[t + 1] - a.off[t];
    const int nch = a.ccnt[t];
    const int act = min(a.wc, ((nch + 63) >> 6) - a.w0);
    if (act <= 0) return;
    const int lane = threadIdx.x;
    const bool on = lane < act;
    const int bits = a.bits, depth = min(a.depth, MP_MAX_DEPTH);
    unsigned long long *fr = BLOCK ? a.frames + (int64_t)t * a.depth * (bits + 1) * 64 : mp_lds;
    const unsigned long long *col = a.tile + base * a.wc + (on ? lane : 0);
    const int2 *mm = a.mm + base;
    const int32_t *dep = a.dep + base;

    unsigned long long two = 0, once = 0;  // characters with a length of 2 and more / 1 and more so far
    unsigned long long acc[MP_LEN_BITS];
    if (CHARS) {
#pragma unroll
        for (int i = 0; i < MP_LEN_BITS; ++i) acc[i] = 0;
    }
    unsigned long long length = 0;
    const auto cost = [&](unsigned long long dec) {
        length += __popcll(dec);
        two |= once & dec;
        once |= dec;
        if (CHARS) {
            unsigned long long carry = dec;
#pragma unroll
            for (int i = 0; i < MP_LEN_BITS; ++i) {
                if (!__any(carry != 0)) break;
                const unsigned long long x = acc[i];
                acc[i] = x ^ carry;
                carry &= x;
            }
        }
    };

    int top = 0;
    unsigned long long cur0 = 0, cur1 = 0, nz, dir;
    // the next leaf's word is loaded while this one folds, its T position one leaf earlier still
    int32_t tp2 = n > 1 ? mm[1].x : 0;
    unsigned long long word1 = on ? col[(int64_t)mm[0].x * a.wc] : 0;
    int32_t g1 = n > 1 ? dep[0] : -1;
    for (int64_t k = 0; k < n; ++k) {
        const unsigned long long word = word1;
        const int g = __builtin_amdgcn_readfirstlane(g1);
        if (k + 1 < n) {
            word1 = on ? col[(int64_t)tp2 * a.wc] : 0;
            g1 = k + 2 < n ? dep[k + 1] : -1;
            tp2 = k + 2 < n ? mm[k + 2].x : 0;
        }
        cur1 = word;
        cur0 = ~word;
        while (top > 0 && __builtin_amdgcn_readfirstlane(fdep[top - 1]) > g) {  // the leaf ends these nodes
            cost(mp_merge(fr, bits, top - 1, lane, cur0, cur1, nz, dir));
            cur0 = ~(nz & dir);
            cur1 = ~(nz & ~dir);
            --top;
        }
        if (g < 0) break;
        if (top > 0 && __builtin_amdgcn_readfirstlane(fdep[top - 1]) == g) {
            cost(mp_merge(fr, bits, top - 1, lane, cur0, cur1, nz, dir));
        } else {
            if (top >= depth) {  // (never, by the host's count: refused, not written)
                if (lane == 0) atomicOr(a.flags, SC_BAD_FRAMES);
                return;
            }
            unsigned long long *slot = fr + (int64_t)top * (bits + 1) * 64 + lane;
            const unsigned long long la = ~cur0, lb = ~cur1;
            slot[0] = la | lb;
            for (int i = 1; i < bits; ++i) slot[i * 64] = 0;
            slot[bits * 64] = la;
            fdep[top] = g;
            ++top;
        }
    }
    cost(~cur0);  // the outgroup: one more change where the root's set lacks 0
    // (bits past the tree's characters are 0 at every leaf: they never cost, and `valid` keeps them out of perfect)
    const int first = 64 * (a.w0 + lane);
    const int left = on ? nch - first : 0;
    const unsigned long long valid = left >= 64 ? ~0ull : left > 0 ? (((unsigned long long)1 << left) - 1) : 0;
    unsigned long long perfect = __popcll(valid & ~two);
    for (int d = 32; d >= 1; d >>= 1) {
        length += __shfl_down(length, d, 64);
        perfect += __shfl_down(perfect, d, 64);
    }
    if (lane == 0) {
        atomicAdd(a.c_len + t, length);
        atomicAdd(a.c_perfect + t, perfect);
    }
    if (CHARS) {
        for (int j = 0; j < 64 && j < left; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < MP_LEN_BITS; ++i) v |= (uint32_t)((acc[i] >> j) & 1) << i;
            a.clen[base + first + j] = (int32_t)v;
        }
    }
}

// S for this export: the preorder arrays with every node's children sorted by tip count, largest first (stable), the
// most frames a fold can open on it (the ancestors in which a tip lies in a child that is not the first) and the
// largest number of children.  ok: the arrays passed every check sc_begin makes of them, in which case sc_begin gets
// the new layout; otherwise it gets the caller's arrays and refuses them with its own message.
struct sc_mp_super {
    bool ok = false;
    std::vector<int32_t> parent, taxon;
    int32_t tips = 0, depth = 1, arity = 0;
};

sc_mp_super sc_mp_layout(int32_t n_nodes, const int32_t *parent, const int32_t *taxon, int32_t n_taxa) {
    sc_mp_super s;
    if (!parent || n_nodes < 1 || parent[0] != -1) return s;
    for (int32_t v = 1; v < n_nodes; ++v)
        if (parent[v] < 0 || parent[v] >= v) return s;
    const sc_walk w = sc_walk_super(n_nodes, parent, true);
    if (taxon) {
        std::vector<char> seen((size_t)std::max(n_taxa, 0), 0);
        for (int32_t v = 0; v < n_nodes; ++v) {
            if (w.n_kids[v]) {
                if (taxon[v] >= 0) return s;
            } else {
                if (taxon[v] < 0) return s;
                if (taxon[v] < n_taxa) {
                    if (seen[taxon[v]]) return s;
                    seen[taxon[v]] = 1;
                }
            }
        }
    }
    // children of every node in the caller's order, then sorted by tips
    std::vector<int32_t> first((size_t)n_nodes + 1, 0), kids((size_t)std::max(n_nodes - 1, 0));
    for (int32_t v = 1; v < n_nodes; ++v) first[parent[v] + 1]++;
    for (int32_t v = 0; v < n_nodes; ++v) first[v + 1] += first[v];
    {
        std::vector<int32_t> at(first.begin(), first.end() - 1);
        for (int32_t v = 1; v < n_nodes; ++v) kids[at[parent[v]]++] = v;
    }
    const auto tips_of = [&](int32_t v) { return w.hi[v] - w.lo[v] + 1; };
    for (int32_t v = 0; v < n_nodes; ++v)
        std::stable_sort(kids.begin() + first[v], kids.begin() + first[v + 1],
                         [&](int32_t x, int32_t y) { return tips_of(x) > tips_of(y); });
    s.parent.resize(n_nodes);
    s.taxon.assign(n_nodes, -1);
    std::vector<int32_t> light((size_t)n_nodes, 0);  // by new index
    std::vector<std::pair<int32_t, int32_t>> stack;  // (old node, new parent)
    stack.emplace_back(0, -1);
    int32_t next = 0;
    while (!stack.empty()) {
        const auto [v, up] = stack.back();
        stack.pop_back();
        const int32_t x = next++;
        s.parent[x] = up;
        if (taxon) s.taxon[x] = taxon[v];
        if (up >= 0) light[x] = light[up] + (v != kids[first[parent[v]]] ? 1 : 0);
        const int32_t k = first[v + 1] - first[v];
        s.arity = std::max(s.arity, k);
        if (k == 0) {
            s.tips++;
            s.depth = std::max(s.depth, light[x]);
        }
        for (int32_t i = first[v + 1] - 1; i >= first[v]; --i) stack.emplace_back(kids[i], x);
    }
    s.ok = true;
    return s;
}

// the fold's plan for a supertree of that frame depth and arity: wc words a pass, `bits` slices of a frame's excess
// (2^bits > arity), the frames' bytes per wave, in LDS or (in_block) in the call's block, and the workspace bytes
// per leaf and per tree of a batch that follow
struct sc_mp_plan {
    int wc, depth, bits;
    size_t frame_bytes;
    bool in_block;
    sc_extras ex;
};

sc_mp_plan sc_mp_plan_of(int32_t depth, int32_t arity, int32_t max_pass_words) {
    sc_mp_plan p;
    p.wc = max_pass_words > 0 ? std::min<int>(max_pass_words, MP_WAVE_WORDS) : MP_WAVE_WORDS;
    p.depth = std::max(depth, 1);
    p.bits = sc_levels_host(std::max(arity, 1));
    p.frame_bytes = (size_t)p.depth * (p.bits + 1) * 64 * 8;
    p.in_block = p.frame_bytes > (size_t)MP_LDS_MAX;
    // per leaf: the tile's words, clo, chi, clen; per tree: the character count, and the frames that left LDS
    p.ex = {8 * (uint64_t)p.wc + 12, 4 + (p.in_block ? (uint64_t)p.frame_bytes : 0)};
    return p;
}

template <bool CHARS>
void sc_mp_launch_fold(const sc_mp_args &a, const sc_mp_plan &p, hipStream_t s) {
    if (p.in_block)
        k_mp_fold<CHARS, true><<<a.nb, 64, 0, s>>>(a);
    else
        k_mp_fold<CHARS, false><<<a.nb, 64, p.frame_bytes, s>>>(a);
}

}  // namespace

extern "C" int scs_score_parsimony(scs_ctx *ctx, const scs_tables *src, int32_t n_nodes, const int32_t *parent,
                                   const int32_t *taxon, int32_t max_batch_trees, int32_t max_pass_words,
                                   int64_t *mrp_chars, int64_t *mrp_length, int64_t *mrp_perfect, int64_t *mrp_max,
                                   int64_t *char_off, int32_t *char_len, int32_t *char_lo, int32_t *char_hi) {
    const char *const who = "scs_score_parsimony";
    // (a null or malformed argument is sc_begin's to refuse: the layout is only made of arrays it will accept)
    const sc_mp_super sup = (ctx && src && parent && taxon) ? sc_mp_layout(n_nodes, parent, taxon, src->n_taxa)
                                                            : sc_mp_super();
    const sc_mp_plan plan = sc_mp_plan_of(sup.depth, sup.arity, max_pass_words);
    // own arrays: four counters per tree (chars, length, perfect, max); per batch the tile, the frames that left LDS,
    // the characters' lo, hi and length per leaf slot and their count per tree
    const size_t mt = src ? (size_t)src->n_trees : 0;
    unsigned long long *d_cnt;
    const auto own = [&](sc_carver w) {
        d_cnt = w.take<unsigned long long>(4 * mt);
        return w;
    };
    sc_call c;
    hipError_t e = hipSuccess;
    SCS_TRY(sc_begin(ctx, src, who, n_nodes, sup.ok ? sup.parent.data() : parent, sup.ok ? sup.taxon.data() : taxon,
                     max_batch_trees, own(sc_carver()).at, plan.ex.per_leaf, plan.ex.per_tree, c, e));
    sc_carver wb = sc_carve_batch(c);
    auto *d_tile = wb.take<unsigned long long>((size_t)c.max_lb * plan.wc);
    auto *d_frames = wb.take<unsigned long long>(plan.in_block ? (size_t)c.max_rows * plan.frame_bytes / 8 : 0);
    auto *d_clo = wb.take<int32_t>(c.max_lb);
    auto *d_chi = wb.take<int32_t>(c.max_lb);
    auto *d_clen = wb.take<int32_t>(c.max_lb);
    auto *d_ccnt = wb.take<int32_t>(c.max_rows);
    // (sc_begin accepted arrays the layout refused: the frames were not planned for them)
    if (own(sc_carve_extra(c)).over || wb.over || !sup.ok) return sc_end(ctx, c, e, SC_BAD_LAYOUT);
    const int32_t M = c.M;
    hipStream_t s = ctx->stream;
    const std::vector<int64_t> &off = src->h_tree_off;
    const bool want_chars = char_len || char_lo || char_hi;
    std::vector<int64_t> coff((size_t)M + 1, 0);
    std::vector<int32_t> ccnt, stage;
    unsigned bad = 0;
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, (size_t)M * 32, s);
    // the frames in LDS take up to MP_LDS_MAX beside the static fdep (the attribute is per function and device: set
    // on every call; the two variants with the frames in the block take no dynamic LDS)
    if (!plan.in_block) {
        const void *const fns[2] = {(const void *)k_mp_fold<false, false>, (const void *)k_mp_fold<true, false>};
        for (int i = 0; i < 2 && e == hipSuccess; ++i)
            e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, MP_LDS_MAX);
    }
    for (size_t b = 0; b + 1 < c.bstart.size() && e == hipSuccess; ++b) {
        if (!sc_prepare_batch(src, s, c, b, e, bad)) break;
        const sc_bview v = sc_batch_of(src, c, b);
        const int32_t t0 = v.t0, nb = v.nb;
        auto a = sc_args<sc_mp_args>(v);
        a.clo = d_clo;
        a.chi = d_chi;
        a.clen = d_clen;
        a.ccnt = d_ccnt;
        a.tile = d_tile;
        a.wc = plan.wc;
        a.depth = plan.depth;
        a.bits = plan.bits;
        a.frames = d_frames;
        a.c_chars = d_cnt + t0;
        a.c_len = d_cnt + M + t0;
        a.c_perfect = d_cnt + 2 * (int64_t)M + t0;
        a.c_max = d_cnt + 3 * (int64_t)M + t0;
        a.flags = c.d_flag;
        k_mp_list<<<nb, SC_THREADS, 0, s>>>(a);
        if (!sc_launched(e)) break;
        ccnt.resize(nb);
        e = hipMemcpyAsync(ccnt.data(), d_ccnt, (size_t)nb * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) break;
        int64_t words = 0;
        for (int32_t i = 0; i < nb; ++i) {
            coff[t0 + i + 1] = coff[t0 + i] + ccnt[i];
            words = std::max<int64_t>(words, ((int64_t)ccnt[i] + 63) >> 6);
        }
        for (int64_t w0 = 0; w0 < words && e == hipSuccess; w0 += plan.wc) {
            a.w0 = (int)w0;
            e = hipMemsetAsync(d_tile, 0, (size_t)v.Lb * plan.wc * 8, s);
            if (e != hipSuccess) break;
            k_mp_toggle<<<grid_of(v.Lb), SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            k_mp_scan<<<nb, SC_THREADS, 0, s>>>(a);
            if (!sc_launched(e)) break;
            if (char_len) sc_mp_launch_fold<true>(a, plan, s);
            else sc_mp_launch_fold<false>(a, plan, s);
            if (!sc_launched(e)) break;
        }
        if (e != hipSuccess || !want_chars || coff[t0 + nb] == coff[t0]) continue;
        // the characters of the batch come down by leaf slot and are packed by tree
        int32_t *const outs[3] = {char_lo, char_hi, char_len};
        const int32_t *const from[3] = {d_clo, d_chi, d_clen};
        stage.resize((size_t)v.Lb);
        for (int x = 0; x < 3 && e == hipSuccess; ++x) {
            if (!outs[x]) continue;
            e = hipMemcpyAsync(stage.data(), from[x], (size_t)v.Lb * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            for (int32_t i = 0; i < nb && e == hipSuccess; ++i)
                std::copy_n(stage.begin() + (off[t0 + i] - v.L0), ccnt[i], outs[x] + coff[t0 + i]);
        }
    }
    int64_t *const outs[4] = {mrp_chars, mrp_length, mrp_perfect, mrp_max};
    SCS_TRY(sc_end_counted(ctx, c, e, bad, d_cnt, 4, outs));
    if (char_off) std::copy(coff.begin(), coff.end(), char_off);
    return SCS_OK;
}

// the plan of one scs_score_parsimony call on the host, by the functions the export calls
extern "C" int scs_debug_parsimony_plan(const scs_tables *src, int32_t n_trees, const int64_t *tree_off,
                                        const int64_t *chars, int32_t n_nodes, const int32_t *parent,
                                        int32_t max_batch_trees, int32_t max_pass_words, int32_t *n_batches_out,
                                        int32_t *bstart_out, int64_t *info_out, int64_t *batch_out) {
    const char *const who = "scs_debug_parsimony_plan";
    SCS_REQUIRE(parent && info_out && batch_out, "%s: null argument", who);
    const sc_mp_super sup = sc_mp_layout(n_nodes, parent, nullptr, 0);
    SCS_REQUIRE(sup.ok, "%s: parent is not a preorder array (root -1, every other parent an earlier node)", who);
    const sc_mp_plan plan = sc_mp_plan_of(sup.depth, sup.arity, max_pass_words);
    sc_debug_plan d;
    SCS_TRY(sc_debug_batches(who, src, n_trees, tree_off, sup.tips, max_batch_trees, (int64_t)plan.ex.per_leaf,
                             (int64_t)plan.ex.per_tree, 0, true, n_batches_out, bstart_out, d));
    const int64_t info[8] = {plan.wc, plan.depth, plan.bits, plan.in_block ? 0 : (int64_t)plan.frame_bytes,
                             plan.in_block, (int64_t)plan.ex.per_leaf, (int64_t)plan.ex.per_tree, sup.tips};
    std::copy(info, info + 8, info_out);
    for (size_t b = 0; b + 1 < d.bstart.size(); ++b) {
        int64_t words = 0;
        for (int32_t t = d.bstart[b]; t < d.bstart[b + 1]; ++t) {
            const int64_t n = d.off[t + 1] - d.off[t];
            const int64_t ch = n < 3 ? 0 : chars ? std::min(std::max<int64_t>(chars[t], 0), n - 2) : n - 2;
            words = std::max(words, (ch + 63) >> 6);
        }
        batch_out[2 * b] = (words + plan.wc - 1) / plan.wc;
        batch_out[2 * b + 1] = words;
    }
    return SCS_OK;
}
