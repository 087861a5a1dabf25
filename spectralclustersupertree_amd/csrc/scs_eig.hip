// Fiedler solve on gfx950: LOBPCG on S = D^-1/2 A D^-1/2 (A = this rank's row
// block of W, zero diagonal), replacing scikit-learn's shift-invert ARPACK path
// (reference call site: src/sc_supertree/scs.py:235-252; arithmetic replaced:
// sklearn/manifold/_spectral_embedding.py:332-376, scipy _laplacian.py:547-558).
//
// The only kernel that touches the N x N matrix is k_symm (HBM-bound: 8 N^2
// bytes per launch, b/4 flop per byte): one wave streams four rows with 16-byte
// loads, multiplies against the scaled block Z = D^-1/2 X and reduces across
// the 64 lanes with wave shuffles.  Everything else works on N x 3b panels.
// The Rayleigh-Ritz Gram product runs on v_mfma_f64_16x16x4_f64; the 3b x 3b
// eigenproblem is solved on the device by a one-workgroup parallel Jacobi, so
// an iteration needs one small device->host read (the residual norms).

#include <algorithm>
#include <chrono>
#include <cmath>

#include "scs_internal.h"
#include "scs_policy.h"
#include "scs_symm.h"
#include "scs_matfree.h"
#include "scs_symm_tri.h"

#include <sched.h>
#include "scs_panel.h"

constexpr int MAXB = 16;      // widest LOBPCG block
constexpr int MAXS = 64;      // largest matrix the Jacobi kernel takes
constexpr int SLD = MAXS + 1; // LDS leading dimension (breaks the power-of-two stride)

typedef double v4d __attribute__((ext_vector_type(4)));

// zt[k][i] = dinv[i] * x[i*ldx + c0 + k]   (k-major, leading dimension ldz; columns >= n stay 0)
__global__ void k_scale_rows(const double *__restrict__ x, int ldx, int c0, int b, int n,
                             const double *__restrict__ dinv, double *__restrict__ zt,
                             int64_t ldz) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * b) return;
    const int k = idx / n, i = idx - k * n;
    zt[(int64_t)k * ldz + i] = dinv[i] * x[(int64_t)i * ldx + c0 + k];
}

// dst[i*ldd + c0 + k] = src[i*b + k]
__global__ void k_store_cols(const double *__restrict__ src, int b, int n, double *__restrict__ dst,
                             int ldd, int c0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * b) return;
    const int i = idx / b, k = idx - i * b;
    dst[(int64_t)i * ldd + c0 + k] = src[idx];
}

// gathered chunks [world][chunk_rows*b] -> y_full rows by row_splits
__global__ void k_unpack(const double *__restrict__ recv, int64_t chunk, int b,
                         const int32_t *__restrict__ splits, int world, int n,
                         double *__restrict__ y) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * b) return;
    const int i = idx / b, k = idx - i * b;
    int r = 0;
    while (r + 1 < world && i >= splits[r + 1]) ++r;
    y[idx] = recv[(int64_t)r * chunk + (int64_t)(i - splits[r]) * b + k];
}

// ---------------------------------------------------------------------------
// Gram products on tall panels: out (ka x kb) = A^T B, A: n x ka (lda), B: n x kb (ldb)
// Deterministic: per-workgroup partials, then a fixed-order reduction.
// ---------------------------------------------------------------------------
constexpr int GRAM_CH = 64;

__global__ __launch_bounds__(256) void k_gram(const double *__restrict__ a, int lda, int ka,
                                               const double *__restrict__ b, int ldb, int kb,
                                               int n, double *__restrict__ partial) {
    __shared__ double sa[GRAM_CH][3 * MAXB + 1];
    __shared__ double sb[GRAM_CH][3 * MAXB + 1];
    const int tid = threadIdx.x;
    const int nout = ka * kb;
    constexpr int MAXO = (3 * MAXB * 3 * MAXB + 255) / 256;  // outputs per thread
    double acc[MAXO];
#pragma unroll
    for (int o = 0; o < MAXO; ++o) acc[o] = 0.0;
    for (int base = blockIdx.x * GRAM_CH; base < n; base += gridDim.x * GRAM_CH) {
        const int rows = min(GRAM_CH, n - base);
        for (int e = tid; e < rows * ka; e += 256) {
            const int r = e / ka, c = e - r * ka;
            sa[r][c] = a[(int64_t)(base + r) * lda + c];
        }
        for (int e = tid; e < rows * kb; e += 256) {
            const int r = e / kb, c = e - r * kb;
            sb[r][c] = b[(int64_t)(base + r) * ldb + c];
        }
        __syncthreads();
#pragma unroll
        for (int o = 0; o < MAXO; ++o) {
            const int e = tid + o * 256;
            if (e < nout) {
                const int ia = e / kb, jb = e - ia * kb;
                double s = acc[o];
                for (int r = 0; r < rows; ++r) s += sa[r][ia] * sb[r][jb];
                acc[o] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
        const int e = tid + o * 256;
        if (e < nout) partial[(int64_t)blockIdx.x * nout + e] = acc[o];
    }
}

// fp64 MFMA variant: one wave per workgroup slab, tiles of 16 x 16 outputs.
// A operand lane l: A^T[i = l&15][k = l>>4] = a[row k][col i]; B operand lane l:
// B[k = l>>4][j = l&15]; accumulator reg r of lane l: row (l>>4) + 4r, col l&15.
template <int TA, int TB>
__global__ __launch_bounds__(64) void k_gram_mfma(const double *__restrict__ a, int lda, int ka,
                                                  const double *__restrict__ b, int ldb, int kb,
                                                  int n, double *__restrict__ partial) {
    const int lane = threadIdx.x;
    const int kk = lane >> 4, cc = lane & 15;
    v4d acc[TA][TB];
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int base = blockIdx.x * 4; base < n; base += gridDim.x * 4) {
        const int r = base + kk;
        double fa[TA], fb[TB];
#pragma unroll
        for (int i = 0; i < TA; ++i) {
            const int c = i * 16 + cc;
            fa[i] = (r < n && c < ka) ? a[(int64_t)r * lda + c] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < TB; ++j) {
            const int c = j * 16 + cc;
            fb[j] = (r < n && c < kb) ? b[(int64_t)r * ldb + c] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < TA; ++i)
#pragma unroll
            for (int j = 0; j < TB; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    const int nout = ka * kb;
#pragma unroll
    for (int i = 0; i < TA; ++i)
#pragma unroll
        for (int j = 0; j < TB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i * 16 + kk + 4 * r;
                const int col = j * 16 + cc;
                if (row < ka && col < kb)
                    partial[(int64_t)blockIdx.x * nout + row * kb + col] = acc[i][j][r];
            }
}

// one wave per output element: lanes read the partials (fixed assignment), then a
// fixed-order shuffle tree -> deterministic result
__global__ __launch_bounds__(256) void k_reduce_partials(const double *__restrict__ partial,
                                                          int nparts, int nout,
                                                          double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= nout) return;
    double s = 0.0;
    for (int p = lane; p < nparts; p += 64) s += partial[(int64_t)p * nout + e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[e] = s;
}

// ---------------------------------------------------------------------------
// panel updates (row-local, safe in place)
// ---------------------------------------------------------------------------
// y[:, 0:kc] = alpha_y * y[:, 0:kc] + sign * a[:, 0:ka] * c   (c: ka x kc, row-major, ldc)
// y and a may alias (in-place y = y*c): every thread of a row reads the row's inputs
// before any thread of that row writes, because a row lives inside one workgroup
// and a barrier separates the two phases.
// (y2, a2: a second pair of panels that takes the same transform in the same launch -- X and S X under
// one rotation; the workgroups with blockIdx.y == 1 work on it, every element as in a launch of its own)
__global__ __launch_bounds__(256) void k_update(double *y, int ldy, int kc, double alpha_y,
                                                 const double *a, int lda, int ka,
                                                 const double *__restrict__ c, int ldc,
                                                 double sign, int n, double *y2 = nullptr,
                                                 const double *a2 = nullptr) {
    __shared__ double sc[3 * MAXB][MAXB];
    if (blockIdx.y) {
        y = y2;
        a = a2;
    }
    for (int e = threadIdx.x; e < ka * kc; e += 256) {
        const int i = e / kc, j = e - i * kc;
        sc[i][j] = c[i * ldc + j];
    }
    __syncthreads();
    // 256 / 16 = 16 rows per workgroup, 16 column slots per row
    const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int j = threadIdx.x & 15;
    double acc = 0.0, yold = 0.0;
    const bool live = r < n && j < kc;
    if (live) {
        const double *ar = a + (int64_t)r * lda;
        for (int i = 0; i < ka; ++i) acc += ar[i] * sc[i][j];
        if (alpha_y != 0.0) yold = y[(int64_t)r * ldy + j];
    }
    __syncthreads();
    if (live) y[(int64_t)r * ldy + j] = (alpha_y == 0.0 ? 0.0 : alpha_y * yold) + sign * acc;
}

// Rayleigh-Ritz update of a panel q = [X | R | P] (n x 3b, ld 3b): with coefficient
// matrices c, d (nq x b each, nq = 2b or 3b)   X' = q[:, :nq] c,   P' = q[:, :nq] d,
// written in place (a row lives inside one workgroup; a barrier separates reads from writes).
__global__ __launch_bounds__(256) void k_rr_update(double *q, int b, int nq,
                                                    const double *__restrict__ c,
                                                    const double *__restrict__ d, int n) {
    __shared__ double sc[3 * MAXB][MAXB];
    __shared__ double sd[3 * MAXB][MAXB];
    for (int e = threadIdx.x; e < nq * b; e += 256) {
        const int i = e / b, j = e - i * b;
        sc[i][j] = c[e];
        sd[i][j] = d[e];
    }
    __syncthreads();
    const int r = blockIdx.x * 16 + (threadIdx.x >> 4);
    const int j = threadIdx.x & 15;
    const bool live = r < n && j < b;
    double xa = 0.0, pa = 0.0;
    double *qr = q + (int64_t)(live ? r : 0) * (3 * b);
    if (live) {
        for (int i = 0; i < nq; ++i) {
            const double v = qr[i];
            xa += v * sc[i][j];
            pa += v * sd[i][j];
        }
    }
    __syncthreads();
    if (live) {
        qr[j] = xa;
        qr[b + j] = pa;
    }
}

// R = AX - X diag(theta) into q[:, 2b:3b]; per-workgroup partial squared norms
__global__ __launch_bounds__(256) void k_residual(double *__restrict__ q,
                                                   const double *__restrict__ aq, int b,
                                                   const double *__restrict__ theta, int n,
                                                   double *__restrict__ partial) {
    __shared__ double red[4][MAXB];
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sq[MAXB];
#pragma unroll
    for (int j = 0; j < MAXB; ++j) sq[j] = 0.0;
    if (r < n) {
        double *qr = q + (int64_t)r * (3 * b);
        const double *ar = aq + (int64_t)r * (3 * b);
#pragma unroll
        for (int j = 0; j < MAXB; ++j)
            if (j < b) {
                const double v = ar[j] - qr[j] * theta[j];
                qr[2 * b + j] = v;
                sq[j] = v * v;
            }
    }
#pragma unroll
    for (int j = 0; j < MAXB; ++j) {
        double s = sq[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) red[wave][j] = s;
    }
    __syncthreads();
    if (threadIdx.x < b)
        partial[(int64_t)blockIdx.x * b + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] +
                                                         red[2][threadIdx.x] + red[3][threadIdx.x];
}

__device__ __forceinline__ double hash_uniform(unsigned long long i, unsigned long long j) {
    unsigned long long x = i * 0x9E3779B97F4A7C15ull + j * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// q[:, 0:b] = [x_init | hashed uniform(-1,1)]
__global__ void k_init_block(double *__restrict__ q, int b, int n, const double *__restrict__ x0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * b) return;
    const int i = idx / b, k = idx - i * b;
    double v = hash_uniform((unsigned long long)i, (unsigned long long)k + 1);
    if (k == 0 && x0) v = x0[i];
    q[(int64_t)i * (3 * b) + k] = v;
}

// u[i] = sqrt(deg[i]) / ||sqrt(deg)||   (trivial eigenvector of S when no row is isolated)
__global__ void k_trivial(const double *__restrict__ deg, double inv_norm, int n,
                          double *__restrict__ u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = sqrt(deg[i]) * inv_norm;
}

// The two columns the caller gets, taken from the panel on the device: the trivial eigenvector
// (constant 1 / ||sqrt d|| when it was deflated analytically, else X's first column / sqrt d) and
// the Fiedler column / sqrt d (sklearn/manifold/_spectral_embedding.py:463).  16 V bytes travel
// instead of the 8 V 3b of the whole panel.
__global__ void k_extract_maps(const double *__restrict__ q, int ldq, int n,
                               const double *__restrict__ dinv, double inv_norm, int constrained,
                               double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double di = dinv[i];
    if (constrained) {
        out[2 * i] = inv_norm;  // (sqrt(d_i) / ||sqrt d||) / sqrt(d_i)
        out[2 * i + 1] = q[(int64_t)i * ldq] * di;
    } else {
        out[2 * i] = q[(int64_t)i * ldq] * di;
        out[2 * i + 1] = q[(int64_t)i * ldq + 1] * di;
    }
}

// SCS_BUILD_UPPER jobs: y = dinv (.) (sum over ranks, in rank order, of the gathered partial
// products); parts is world x (n * b)
__global__ void k_sum_parts(const double *__restrict__ parts, int world, int n, int b,
                            const double *__restrict__ dinv, double *__restrict__ y) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * b) return;
    double s = 0.0;
    for (int r = 0; r < world; ++r) s += parts[(int64_t)r * n * b + idx];
    y[idx] = dinv[idx / b] * s;
}

// ---------------------------------------------------------------------------
// one-workgroup parallel Jacobi eigensolver (n <= 64), LDS resident
// ---------------------------------------------------------------------------
struct jacobi_lds {
    alignas(16) double a[MAXS][SLD];
    alignas(16) double e[MAXS][SLD];
    alignas(16) double cs[MAXS / 2][2];
    int pq[MAXS / 2][2];
    double red[256];
    double w[MAXS];
    int perm[MAXS];
    __device__ double *rot_log() { return &e[16][0]; }  // jacobi_eig_waves' log of a sweep's rotations
};

// The same for ONE size M in {4, 8}: 2 KB instead of 80 -- a kernel whose LDS also holds another role's
// tiles (k_symm_tri_tf) runs its small solve on this one (jacobi_eig_waves is written against either)
template <int M>
struct jacobi_small_lds {
    alignas(16) double a[M][M];
    alignas(16) double e[M][M];
    alignas(16) double cs[M / 2][2];
    alignas(16) double rlog[2 * (M - 1) * (M / 2) * 2];
    double w[M];
    int pq[1][2];
    int perm[M];
    __device__ double *rot_log() { return rlog; }
};

// On entry s.a holds the symmetric matrix (n x n).  On exit s.w holds the
// eigenvalues in DESCENDING order and s.perm[k] the column of s.e holding the
// k-th eigenvector.  All 256 threads of the workgroup must call.
//
// Parallel-ordered two-sided Jacobi.  A step rotates m/2 disjoint index pairs at
// once: A <- J^T A J splits into independent 2x2 blocks (row pair x column pair),
// each updated by one thread, so a step costs two barriers.
// ---- fast variant for n <= 24 (the sizes the fused LOBPCG loop solves every iteration)
// A lone wave issues about one instruction per 8 clocks, so a Jacobi step is bound by the
// instruction count on its critical path, not by arithmetic.  This variant therefore
//   * keeps the rotated pairs at FIXED positions (2k, 2k+1) and moves the data instead: every
//     work item -- a 2 x 2 block of A or a column pair of one row of E -- reads from one copy
//     of the matrices and writes its results to precomputed, round-robin-permuted addresses
//     in the other copy, so a step needs no index arithmetic;
//   * computes each pair's rotation once (m / 2 lanes, from the pair's diagonal block, with
//     hardware rsq/rcp seeds refined by Newton steps instead of IEEE division and square
//     root) and hands it to the items through LDS: a second barrier per step, but the long
//     rotation chain is off the path of the threads that own two items.
// At most two items per thread (256 threads).  Interface as jacobi_eig.
// 1 / sqrt(x) to full precision: the hardware seed (2^-23) and ONE third-order step
// y (1 + h / 2 + 3 h^2 / 8), h = 1 - x y^2 -- four dependent operations
__device__ __forceinline__ double rsq_full(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    const double xy = x * y;
    const double h = fma(-xy, y, 1.0);
    const double p = fma(0.375, h, 0.5);
    return fma(y * h, p, y);
}

// The rotation (c, s) that annihilates a_pq, |angle| <= pi / 4:  tan 2t = a_pq / dl with
// dl = (a_qq - a_pp) / 2, taken through cos 2t = |dl| / hypot(dl, a_pq):
//   c^2 = (1 + cos 2t) / 2,   s = sin 2t / (2 c).
// A Jacobi step of a lone wave is bound by the LENGTH of this dependent chain (about ten clocks
// an operation), so it is written for depth: two reciprocal square roots, no division, 17
// operations deep (the textbook t = sign / (|theta| + sqrt(theta^2 + 1)) form with refined
// rsq / rcp seeds was 31).  Straight-line (selects, no branch).
__device__ __forceinline__ void jacobi_rot(double app, double apq, double aqq, double &c,
                                           double &sn) {
    const double dl = 0.5 * (aqq - app);
    const double x = fma(dl, dl, apq * apq);
    const double y = rsq_full(x);                   // 1 / hypot(dl, apq)
    const double c2 = fma(0.5 * fabs(dl), y, 0.5);  // in [0.5, 1]
    const double z = rsq_full(c2);
    const double hs = (0.5 * apq) * y;
    const double cc = c2 * z;
    double ss = hs * z;
    ss = dl >= 0.0 ? ss : -ss;
    // nothing to rotate, or hypot^2 outside the range the seed handles (never seen: the
    // matrices are O(1) and dead directions carry -1e30): identity
    const bool rot = apq != 0.0 && x >= 1e-290 && x <= 1e290;
    c = rot ? cc : 1.0;
    sn = rot ? ss : 0.0;
}

__device__ void jacobi_eig_fast(jacobi_lds &s, int n) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int m = n + (n & 1), half = m / 2;
    const int nblk = half * half, ne = m * half;
    double *fa = &s.a[0][0];  // [2][nblk][4]: 2 x 2 blocks, row-major inside a block
    double *fe = &s.e[0][0];  // [2][ne][2]:   E[r][2 kc], E[r][2 kc + 1]
    // position after one round-robin move: 0 stays, the rest cycles 1 -> 3 -> ... -> m-1 ->
    // m-2 -> ... -> 4 -> 2 -> 1
    auto next_pos = [&](int i) {
        if (i == 0 || m == 2) return i;
        if (i & 1) return i == m - 1 ? m - 2 : i + 2;
        return i == 2 ? 1 : i - 2;
    };
    int kind[2], ia[2], ib[2], dst[2][4];
    double v[2][4];
    // blocks take whole waves (a wave that mixes blocks and E items would run both code
    // paths one after the other), E items follow
    const int nblk_pad = (nblk + 63) & ~63;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const int e = tid + 256 * w;
        kind[w] = 0;
        ia[w] = ib[w] = 0;
        if (e < nblk) {
            kind[w] = 1;
            const int kr = e / half, kc = e - kr * half;
            ia[w] = kr;
            ib[w] = kc;
#pragma unroll
            for (int al = 0; al < 2; ++al)
#pragma unroll
                for (int be = 0; be < 2; ++be) {
                    const int i = 2 * kr + al, j = 2 * kc + be;
                    v[w][al * 2 + be] = (i < n && j < n) ? s.a[i][j] : 0.0;
                    const int pi = next_pos(i), pj = next_pos(j);
                    dst[w][al * 2 + be] = ((pi >> 1) * half + (pj >> 1)) * 4 + (pi & 1) * 2 + (pj & 1);
                }
        } else if (e >= nblk_pad && e < nblk_pad + ne) {
            kind[w] = 2;
            const int r = (e - nblk_pad) / half, kc = (e - nblk_pad) - r * half;
            ia[w] = r;
            ib[w] = kc;
#pragma unroll
            for (int be = 0; be < 2; ++be) {
                const int j = 2 * kc + be;
                v[w][be] = r == j ? 1.0 : 0.0;
                const int pj = next_pos(j);
                dst[w][be] = (r * half + (pj >> 1)) * 2 + (pj & 1);
            }
        }
    }
    __syncthreads();  // everyone has read its part of the input matrix
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        if (kind[w] == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) fa[(ia[w] * half + ib[w]) * 4 + k] = v[w][k];
        } else if (kind[w] == 2) {
            fe[(ia[w] * half + ib[w]) * 2 + 0] = v[w][0];
            fe[(ia[w] * half + ib[w]) * 2 + 1] = v[w][1];
        }
    }
    __syncthreads();
    int cur = 0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double *ac = fa + cur * nblk * 4;
        // convergence: off-diagonal mass against the diagonal (dead directions carry -1e30 on
        // the diagonal, k_small_rr: not part of the scale)
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int w = 0; w < 2; ++w)
            if (kind[w] == 1) {
                const double *bp = ac + (ia[w] * half + ib[w]) * 4;
                const double b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
                if (ia[w] == ib[w]) {
                    dia += (b0 > -1e29 ? b0 * b0 : 0.0) + (b3 > -1e29 ? b3 * b3 : 0.0);
                    off += b1 * b1 + b2 * b2;
                } else {
                    off += (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
                }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            off += __shfl_xor(off, o, 64);
            dia += __shfl_xor(dia, o, 64);
        }
        if (lane == 0) {
            s.red[wave] = off;
            s.red[4 + wave] = dia;
        }
        __syncthreads();
        off = s.red[0] + s.red[1] + s.red[2] + s.red[3];
        dia = s.red[4] + s.red[5] + s.red[6] + s.red[7];
        __syncthreads();
        if (off <= 1.25e-32 * (double)(n * n) * dia || off == 0.0) break;

        for (int step = 0; step < m - 1; ++step) {
            const double *a0 = fa + cur * nblk * 4;
            const double *e0 = fe + cur * ne * 2;
            double *a1 = fa + (cur ^ 1) * nblk * 4;
            double *e1 = fe + (cur ^ 1) * ne * 2;
            // the rotation of pair k, once, from its diagonal block
            if (tid < half) {
                const double *dc = a0 + (tid * half + tid) * 4;
                double c, sn;
                jacobi_rot(dc[0], dc[1], dc[3], c, sn);
                s.cs[tid][0] = c;
                s.cs[tid][1] = sn;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (kind[w] == 0) continue;
                const double c2 = s.cs[ib[w]][0], s2 = s.cs[ib[w]][1];
                if (kind[w] == 1) {
                    const double c1 = s.cs[ia[w]][0], s1 = s.cs[ia[w]][1];
                    const double *bp = a0 + (ia[w] * half + ib[w]) * 4;
                    const double a00 = bp[0], a01 = bp[1], a10 = bp[2], a11 = bp[3];
                    const double t00 = c2 * a00 - s2 * a01, t01 = s2 * a00 + c2 * a01;
                    const double t10 = c2 * a10 - s2 * a11, t11 = s2 * a10 + c2 * a11;
                    a1[dst[w][0]] = c1 * t00 - s1 * t10;
                    a1[dst[w][1]] = c1 * t01 - s1 * t11;
                    a1[dst[w][2]] = s1 * t00 + c1 * t10;
                    a1[dst[w][3]] = s1 * t01 + c1 * t11;
                } else {
                    const double *ep = e0 + (ia[w] * half + ib[w]) * 2;
                    const double x = ep[0], y = ep[1];
                    e1[dst[w][0]] = c2 * x - s2 * y;
                    e1[dst[w][1]] = s2 * x + c2 * y;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    // back to the caller's layout: eigenvector of position j in column j of s.e, positions
    // ranked by eigenvalue (descending); an odd n leaves out the padded coordinate, whose
    // column is the only one with a non-zero in row n
    const double *ac = fa + cur * nblk * 4;
    const double *ec = fe + cur * ne * 2;
#pragma unroll
    for (int w = 0; w < 2; ++w)
        if (kind[w] == 2) {
            v[w][0] = ec[(ia[w] * half + ib[w]) * 2 + 0];
            v[w][1] = ec[(ia[w] * half + ib[w]) * 2 + 1];
        }
    double wi = 0.0;
    int rank = -1;
    if (tid < m) {
        auto diag_at = [&](int i) { return ac[((i >> 1) * half + (i >> 1)) * 4 + (i & 1) * 3]; };
        auto is_pad = [&](int i) { return m != n && ec[(n * half + (i >> 1)) * 2 + (i & 1)] != 0.0; };
        if (!is_pad(tid)) {
            wi = diag_at(tid);
            rank = 0;
            for (int j = 0; j < m; ++j) {
                if (is_pad(j)) continue;
                const double wj = diag_at(j);
                if (wj > wi || (wj == wi && j < tid)) ++rank;
            }
        }
    }
    __syncthreads();  // all reads of the flat copies are done: s.e may be overwritten
#pragma unroll
    for (int w = 0; w < 2; ++w)
        if (kind[w] == 2 && ia[w] < n) {
            s.e[ia[w]][2 * ib[w] + 0] = v[w][0];
            s.e[ia[w]][2 * ib[w] + 1] = v[w][1];
        }
    if (rank >= 0) {
        s.w[rank] = wi;
        s.perm[rank] = tid;
    }
    __syncthreads();
}

// (Round 4: a ONE-wave variant of the above for n <= 12 -- two items per lane, no workgroup
// barrier inside the sweeps, bitwise the same results -- was built and measured slower:
// k_small_rr 50.6 us against 43.5, k_small_orth unchanged at 13.1: four waves with one item per
// thread and two cheap barriers beat one wave that serialises two items and both item kinds;
// profiles/r04_jacobi_wave.txt.  What did work is to split the two item KINDS over two waves:
// jacobi_eig_waves below.)
// The same sum when only the first 16 (ROWS = 1) or 32 (ROWS = 2) lanes carry non-zero terms and
// only they need the result: four DPP steps inside a row of 16 lanes (quad swaps, then the two
// mirrors) instead of six trips through the LDS crossbar; every lane of the rows that count
// ends with bitwise the same total.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int ROWS>
__device__ __forceinline__ double row_sum(double v) {
    v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);  // row_half_mirror
    v += dpp_f64<0x140>(v);  // row_mirror
    if (ROWS == 2) v += __shfl_xor(v, 16, 64);
    return v;
}

// ---- wave-specialised variant for n = 4, 8, 12 (the sizes the fused b = 4 loop solves in
// every iteration: the 12 x 12 Rayleigh-Ritz problem and the 4 x 4 SVQB ones)
// The variant above spends 1 200 clocks on a step at n = 12 -- two workgroup barriers, three
// dependent LDS round trips, the rotation chain -- for 36 + 72 work items.  Here wave 0 alone
// iterates on A: its lanes own the (n/2)^2 2 x 2 blocks in registers, every lane computes the
// rotation of its own block (only the diagonal blocks' ones mean anything: they are published,
// 16 bytes each), applies the two it needs and writes its four results to their round-robin
// positions, in place -- a wave's LDS operations execute in order, so the step needs no barrier
// at all.  The rotations of a sweep are also logged; wave 1, one lane per ROW of the eigenvector
// matrix with the row in registers (the round-robin moves are compile-time renamings over the
// unrolled sweep), replays the log one sweep behind wave 0, concurrently: one workgroup barrier
// per sweep.  Same rotations, same arithmetic, same order as the variant above.
typedef double jw_d2 __attribute__((ext_vector_type(2)));
constexpr int jw_next_pos(int i, int m) {
    if (i == 0 || m == 2) return i;
    if (i & 1) return i == m - 1 ? m - 2 : i + 2;
    return i == 2 ? 1 : i - 2;
}

template <int M, typename L>
__device__ void jacobi_eig_waves(L &s) {
    constexpr int H = M / 2, NB = H * H, SPS = M - 1;
    static_assert(M % 2 == 0 && NB <= 64 && M <= 16, "one wave holds the blocks");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    double *fa = &s.a[0][0];                 // [NB][4]: 2 x 2 blocks, row-major inside a block
    double *rlog = s.rot_log();              // [2][SPS][H][2]: (c, s) of a sweep's rotations
    volatile int *flag = &s.pq[0][0];        // [2]: wave 0's verdict before sweep k, at k & 1
    const int kr = lane / H, kc = lane - kr * H;
    const bool blk = wave == 0 && lane < NB;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    int d00 = 0, d01 = 0, d10 = 0, d11 = 0;
    if (blk) {
        a00 = s.a[2 * kr][2 * kc];
        a01 = s.a[2 * kr][2 * kc + 1];
        a10 = s.a[2 * kr + 1][2 * kc];
        a11 = s.a[2 * kr + 1][2 * kc + 1];
        const int r0 = jw_next_pos(2 * kr, M), r1 = jw_next_pos(2 * kr + 1, M);
        const int c0 = jw_next_pos(2 * kc, M), c1 = jw_next_pos(2 * kc + 1, M);
        auto at = [&](int pi, int pj) { return ((pi >> 1) * H + (pj >> 1)) * 4 + (pi & 1) * 2 + (pj & 1); };
        d00 = at(r0, c0);
        d01 = at(r0, c1);
        d10 = at(r1, c0);
        d11 = at(r1, c1);
    }
    // row `lane` of E (wave 1), by position
    double e[M];
#pragma unroll
    for (int i = 0; i < M; ++i) e[i] = i == lane ? 1.0 : 0.0;
    __syncthreads();  // the input matrix has been read: its memory now holds the flat blocks
    if (blk) {
        double *bp = fa + lane * 4;
        bp[0] = a00;
        bp[1] = a01;
        bp[2] = a10;
        bp[3] = a11;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        if (wave == 0) {
            // convergence: off-diagonal mass against the diagonal (dead directions carry -1e30 on
            // the diagonal, k_small_rr: not part of the scale)
            double off = 0.0, dia = 0.0;
            if (blk) {
                if (kr == kc) {
                    dia = (a00 > -1e29 ? a00 * a00 : 0.0) + (a11 > -1e29 ? a11 * a11 : 0.0);
                    off = a01 * a01 + a10 * a10;
                } else {
                    off = (a00 * a00 + a01 * a01) + (a10 * a10 + a11 * a11);
                }
            }
            off = row_sum<1>(off);
            dia = row_sum<1>(dia);
            if (NB > 16) {
                off += __shfl_xor(off, 16, 64);
                dia += __shfl_xor(dia, 16, 64);
            }
            if (NB > 32) {
                off += __shfl_xor(off, 32, 64);
                dia += __shfl_xor(dia, 32, 64);
            }
            const bool done = off <= 1.25e-32 * (double)(M * M) * dia || off == 0.0;
            if (lane == 0) flag[sweep & 1] = done ? 1 : 0;
            if (!done) {
                double *lg = rlog + (sweep & 1) * SPS * H * 2;
                for (int step = 0; step < SPS; ++step) {
                    double c, sn;
                    jacobi_rot(a00, a01, a11, c, sn);
                    if (blk && kr == kc) {
                        const jw_d2 v = {c, sn};
                        *(jw_d2 *)&s.cs[kr][0] = v;
                        *(jw_d2 *)&lg[(step * H + kr) * 2] = v;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (blk) {
                        const jw_d2 r1 = *(const jw_d2 *)&s.cs[kr][0], r2 = *(const jw_d2 *)&s.cs[kc][0];
                        const double c1 = r1.x, s1 = r1.y;
                        const double c2 = r2.x, s2 = r2.y;
                        const double t00 = c2 * a00 - s2 * a01, t01 = s2 * a00 + c2 * a01;
                        const double t10 = c2 * a10 - s2 * a11, t11 = s2 * a10 + c2 * a11;
                        fa[d00] = c1 * t00 - s1 * t10;
                        fa[d01] = c1 * t01 - s1 * t11;
                        fa[d10] = s1 * t00 + c1 * t10;
                        fa[d11] = s1 * t01 + c1 * t11;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (blk) {
                        const jw_d2 *bp = (const jw_d2 *)(fa + lane * 4);
                        const jw_d2 lo = bp[0], hi = bp[1];
                        a00 = lo.x;
                        a01 = lo.y;
                        a10 = hi.x;
                        a11 = hi.y;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
            }
        }
        __syncthreads();
        if (flag[sweep & 1]) break;
        if (wave == 1 && lane < M) {
            const double *lg = rlog + (sweep & 1) * SPS * H * 2;
#pragma unroll
            for (int step = 0; step < SPS; ++step) {
                double t[M];
#pragma unroll
                for (int k = 0; k < H; ++k) {
                    const jw_d2 r = *(const jw_d2 *)&lg[(step * H + k) * 2];
                    const double c2 = r.x, s2 = r.y;
                    const double x = e[2 * k], y = e[2 * k + 1];
                    t[jw_next_pos(2 * k, M)] = c2 * x - s2 * y;
                    t[jw_next_pos(2 * k + 1, M)] = s2 * x + c2 * y;
                }
#pragma unroll
                for (int i = 0; i < M; ++i) e[i] = t[i];
            }
        }
    }
    // back to the caller's layout: eigenvector of position j in column j of s.e, positions
    // ranked by eigenvalue (descending)
    if (wave == 1 && lane < M) {
#pragma unroll
        for (int i = 0; i < M; ++i) s.e[lane][i] = e[i];
    }
    double wi = 0.0;
    int rank = -1;
    if (tid < M) {
        auto diag_at = [&](int i) { return fa[((i >> 1) * H + (i >> 1)) * 4 + (i & 1) * 3]; };
        wi = diag_at(tid);
        rank = 0;
        for (int j = 0; j < M; ++j) {
            const double wj = diag_at(j);
            if (wj > wi || (wj == wi && j < tid)) ++rank;
        }
    }
    __syncthreads();
    if (rank >= 0) {
        s.w[rank] = wi;
        s.perm[rank] = tid;
    }
    __syncthreads();
}

// The general form, for a workgroup of NT threads (256, or 1 024: k_small_finish<1024>, round 5).  With 1 024
// threads only the independent work items of a step are spread wider -- three per thread instead of twelve at
// n = 64; everything whose ORDER matters (the convergence sums: per-thread partials over e = tid mod 256, wave
// shuffles, four wave totals) is done by the first 256 threads exactly as before: the same bits.
template <int NT>
__device__ void jacobi_eig_generic(jacobi_lds &s, int n) {
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int m = n + (n & 1);  // even; a padded index has zero row/column
    for (int e = tid; e < m * m; e += NT) {
        const int i = e / m, j = e - i * m;
        s.e[i][j] = i == j ? 1.0 : 0.0;
        if (i >= n || j >= n) s.a[i][j] = 0.0;
    }
    __syncthreads();
    const int half = m / 2;
    for (int sweep = 0; sweep < 30; ++sweep) {
        // convergence: off-diagonal mass against the diagonal
        double off = 0.0, dia = 0.0;
        for (int e = tid; e < n * n && tid < 256; e += 256) {
            const int i = e / n, j = e - i * n;
            const double v = s.a[i][j];
            // dead directions carry -1e30 on the diagonal (k_small_rr): not part of the scale
            if (i == j) dia += v > -1e29 ? v * v : 0.0;
            else off += v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            off += __shfl_xor(off, o, 64);
            dia += __shfl_xor(dia, o, 64);
        }
        if (lane == 0 && wave < 4) {
            s.red[wave] = off;
            s.red[4 + wave] = dia;
        }
        __syncthreads();
        off = s.red[0] + s.red[1] + s.red[2] + s.red[3];
        dia = s.red[4] + s.red[5] + s.red[6] + s.red[7];
        __syncthreads();
        // off-diagonal mass at the rounding floor of an n x n matrix: (n * eps)^2 * ||diag||^2
        if (off <= 1.25e-32 * (double)(n * n) * dia || off == 0.0) break;

        for (int step = 0; step < m - 1; ++step) {
            if (tid < half) {
                // round-robin tournament: index m-1 stays, the others rotate
                int p, q;
                if (tid == 0) {
                    p = m - 1;
                    q = step;
                } else {
                    p = (step + tid) % (m - 1);
                    q = (step - tid + (m - 1)) % (m - 1);
                }
                if (p > q) {
                    const int t = p;
                    p = q;
                    q = t;
                }
                const double apq = s.a[p][q];
                double c = 1.0, sn = 0.0;
                if (apq != 0.0) {
                    const double th = (s.a[q][q] - s.a[p][p]) / (2.0 * apq);
                    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    sn = t * c;
                }
                s.cs[tid][0] = c;
                s.cs[tid][1] = sn;
                s.pq[tid][0] = p;
                s.pq[tid][1] = q;
            }
            __syncthreads();
            // work items: half*half 2x2 blocks of A, then m*half column pairs of E
            const int nblk = half * half;
            for (int e = tid; e < nblk + m * half; e += NT) {
                if (e < nblk) {
                    const int kr = e / half, kc = e - kr * half;
                    const int p = s.pq[kr][0], q = s.pq[kr][1];
                    const int pc = s.pq[kc][0], qc = s.pq[kc][1];
                    const double c1 = s.cs[kr][0], s1 = s.cs[kr][1];
                    const double c2 = s.cs[kc][0], s2 = s.cs[kc][1];
                    const double a00 = s.a[p][pc], a01 = s.a[p][qc];
                    const double a10 = s.a[q][pc], a11 = s.a[q][qc];
                    // right: columns (pc, qc) <- (c2*x - s2*y, s2*x + c2*y)
                    const double t00 = c2 * a00 - s2 * a01, t01 = s2 * a00 + c2 * a01;
                    const double t10 = c2 * a10 - s2 * a11, t11 = s2 * a10 + c2 * a11;
                    // left: rows (p, q) <- (c1*rp - s1*rq, s1*rp + c1*rq)
                    double n00 = c1 * t00 - s1 * t10, n01 = c1 * t01 - s1 * t11;
                    double n10 = s1 * t00 + c1 * t10, n11 = s1 * t01 + c1 * t11;
                    if (kr == kc) {  // the rotated pair itself: annihilated exactly
                        n01 = 0.0;
                        n10 = 0.0;
                    }
                    s.a[p][pc] = n00;
                    s.a[p][qc] = n01;
                    s.a[q][pc] = n10;
                    s.a[q][qc] = n11;
                } else {
                    const int f = e - nblk;
                    const int r = f / half, kc = f - r * half;
                    const int pc = s.pq[kc][0], qc = s.pq[kc][1];
                    const double c2 = s.cs[kc][0], s2 = s.cs[kc][1];
                    const double ep = s.e[r][pc], eq = s.e[r][qc];
                    s.e[r][pc] = c2 * ep - s2 * eq;
                    s.e[r][qc] = s2 * ep + c2 * eq;
                }
            }
            __syncthreads();
        }
    }
    // sort descending (rank by counting)
    if (tid < n) {
        const double wi = s.a[tid][tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double wj = s.a[j][j];
            if (wj > wi || (wj == wi && j < tid)) ++rank;
        }
        s.w[rank] = wi;
        s.perm[rank] = tid;
    }
    __syncthreads();
}

__device__ void jacobi_eig(jacobi_lds &s, int n) {
    if (n == 12) return jacobi_eig_waves<12>(s);
    if (n == 8) return jacobi_eig_waves<8>(s);
    if (n == 4) return jacobi_eig_waves<4>(s);
    if (n <= 24) {
        jacobi_eig_fast(s, n);
        return;
    }
    jacobi_eig_generic<256>(s, n);
}

// Sum `nparts` per-workgroup partials of `nout` outputs (partial[p * nout + e]) in a fixed
// order with all 256 threads of the workgroup: eight interleaved slices of the partials are
// summed with the loads of a slice in flight together, then the slices are combined.
// out(e, value) is called by one thread per output; ends with a workgroup barrier.
template <int TL, typename F>
__device__ __forceinline__ void sum_partials(const double *__restrict__ partial, int nparts,
                                             int nout, double (*tmp)[TL], F out) {
    // tmp: [8][>= nout] doubles of LDS
    // (up to five outputs per thread at a time, sixteen loads of each in flight before the first
    // add: the kernel is one workgroup, nothing else hides the latency of a load, and the
    // partials come from the other XCDs' workgroups, i.e. from memory -- the 12 x 12 Rayleigh-Ritz
    // matrix, 1 152 slice sums, is then ONE round trip instead of ten)
    constexpr int IT = 5;
    const int total = nout * 8;
    for (int f0 = threadIdx.x; f0 < total; f0 += 256 * IT) {
        int sl[IT], el[IT];
        bool on[IT];
        double v[IT];
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int f = f0 + 256 * j;
            on[j] = f < total;
            sl[j] = on[j] ? f / nout : 0;
            el[j] = on[j] ? f - sl[j] * nout : 0;
            v[j] = 0.0;
        }
        for (int base = 0; base < nparts; base += 128) {
            double x[IT][16];
#pragma unroll
            for (int j = 0; j < IT; ++j)
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const int p = base + sl[j] + 8 * k;
                    x[j][k] = (on[j] && p < nparts) ? partial[(int64_t)p * nout + el[j]] : 0.0;
                }
#pragma unroll
            for (int k = 0; k < 16; ++k)
#pragma unroll
                for (int j = 0; j < IT; ++j) v[j] += x[j][k];
        }
#pragma unroll
        for (int j = 0; j < IT; ++j)
            if (on[j]) tmp[sl[j]][el[j]] = v[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nout; e += 256) {
        double v = tmp[0][e];
#pragma unroll
        for (int k = 1; k < 8; ++k) v += tmp[k][e];
        out(e, v);
    }
    __syncthreads();
}

// plain eigen-decomposition of a global n x n matrix (debug entry point, dense path)
__global__ __launch_bounds__(256) void k_small_eig(const double *__restrict__ a, int n,
                                                    double *__restrict__ w, double *__restrict__ v) {
    __shared__ jacobi_lds s;
    // The sweeps are written for matrices of order one (the solver's: S and its Rayleigh-Ritz projections):
    // jacobi_rot leaves a pair alone when dl^2 + a_pq^2 is outside 1e-290 ... 1e290, the convergence test squares the entries, and
    // -1e30 on the diagonal marks a dead direction.  A matrix far from that range is solved as a power of
    // two times one of order one -- exact up to the underflow of entries that are negligible beside the
    // largest; one within 2^-256 ... 2^256 is not touched at all.
    double big = 0.0;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        big = fmax(big, fabs(0.5 * a[i * n + j] + 0.5 * a[j * n + i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) big = fmax(big, __shfl_xor(big, o, 64));
    if ((threadIdx.x & 63) == 0) s.red[threadIdx.x >> 6] = big;
    __syncthreads();
    big = fmax(fmax(s.red[0], s.red[1]), fmax(s.red[2], s.red[3]));
    const int ex = (big > 0.0 && big < INFINITY) ? ilogb(big) : 0;
    const int sh = (ex >= 256 || ex <= -256) ? -ex : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        const double x = 0.5 * (a[i * n + j] + a[j * n + i]);
        // (halved before they are added where the sum itself would overflow)
        s.a[i][j] = sh ? ldexp(0.5 * a[i * n + j], sh) + ldexp(0.5 * a[j * n + i], sh) : x;
    }
    __syncthreads();
    jacobi_eig(s, n);
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, k = e - i * n;
        v[i * n + k] = s.e[i][s.perm[k]];
    }
    if (threadIdx.x < n) w[threadIdx.x] = sh ? ldexp(s.w[threadIdx.x], -sh) : s.w[threadIdx.x];
}

// ---------------------------------------------------------------------------
// dense path for 65 .. 128 vertices: one-sided (Hestenes) Jacobi in LDS
// ---------------------------------------------------------------------------
// The two-sided Jacobi above keeps the matrix AND the accumulated rotations in LDS: two
// (n + 1) x n arrays, 64 vertices at most.  Up to 128 vertices one array still fits the 160 KB,
// and the one-sided method needs no second one: rotating the COLUMNS of A = S + I (symmetric
// positive semi-definite: the eigenvalues of S lie in [-1, 1]) until they are mutually
// orthogonal turns column j into lambda_j v_j -- its norm is the eigenvalue (of S, plus 1), its
// direction the eigenvector.  A step orthogonalises m / 2 disjoint column pairs (round-robin
// tournament), four threads per pair: three dot products over the rows (partial sums by
// shuffles), one rotation, the two columns rewritten.  Recursion nodes of 65 .. 128 taxa are
// then ~1 ms of one workgroup instead of ~35 latency-bound LOBPCG iterations.
constexpr int DENSE2_MAX = 128;
constexpr int DENSE2_LD = DENSE2_MAX + 1;

// The sweeps: columns of a (m x m, m even) rotated pairwise until mutually orthogonal.  All 256
// threads of the workgroup call; returns false when 40 sweeps did not get there (never seen: the
// method converges quadratically; a caller reports it rather than hand back a half-rotated basis).
__device__ bool onesided_sweeps(double (*a)[DENSE2_LD], int m, int *s_rot) {
    const int tid = threadIdx.x;
    const int half = m / 2;
    const int pair = tid >> 2, part = tid & 3;
    bool done = false;
    for (int sweep = 0; sweep < 40 && !done; ++sweep) {
        if (tid == 0) *s_rot = 0;
        __syncthreads();
        for (int step = 0; step < m - 1; ++step) {
            int rotated = 0;
            if (pair < half) {
                // round-robin tournament: index m - 1 stays, the others rotate
                int p, q;
                if (pair == 0) {
                    p = m - 1;
                    q = step;
                } else {
                    p = (step + pair) % (m - 1);
                    q = (step - pair + (m - 1)) % (m - 1);
                }
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = part; r < m; r += 4) {
                    const double x = a[r][p], y = a[r][q];
                    al = fma(x, x, al);
                    be = fma(y, y, be);
                    ga = fma(x, y, ga);
                }
                al += __shfl_xor(al, 1, 64);
                be += __shfl_xor(be, 1, 64);
                ga += __shfl_xor(ga, 1, 64);
                al += __shfl_xor(al, 2, 64);
                be += __shfl_xor(be, 2, 64);
                ga += __shfl_xor(ga, 2, 64);
                // (the four threads of a pair hold the same sums: the same decision); columns
                // whose cosine is at the rounding floor of a 128-term dot product (~ n eps = 3e-14)
                // are orthogonal: rotating them again would never end
                // -- and a column whose squared norm is below 1e-24 IS zero: an eigenvalue -1 of S
                // (a bipartite component) is a null direction of A = S + I, its column shrinks to
                // rounding noise whose "cosine" with the other columns is anything, and the pair
                // would be rotated for ever (seen: a 2-tree bootstrap forest in the recursion sweep).
                // The wanted columns have norms near 2; what a 1e-12 column still overlaps with them
                // moves their eigenvalues by 1e-24.
                if (ga * ga > 1e-27 * al * be && al > 1e-24 && be > 1e-24) {
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
                    const double c = 1.0 / sqrt(fma(t, t, 1.0)), sn = c * t;
                    for (int r = part; r < m; r += 4) {
                        const double x = a[r][p], y = a[r][q];
                        a[r][p] = c * x - sn * y;
                        a[r][q] = sn * x + c * y;
                    }
                    rotated = 1;
                }
            }
            if (rotated) *s_rot = 1;  // (benign race: every writer stores 1)
            __syncthreads();
        }
        done = *s_rot == 0;
        __syncthreads();
    }
    return done;
}

// w3: the three largest eigenvalues of S and, in w3[3], 1.0 when the sweeps converged (0.0: they did not)
__global__ __launch_bounds__(256) void k_dense_onesided(const double *__restrict__ sd, int n,
                                                         double *__restrict__ w3,
                                                         double *__restrict__ v2) {
    extern __shared__ double dyn_lds[];
    double(*a)[DENSE2_LD] = (double(*)[DENSE2_LD])dyn_lds;  // a[row][col]
    __shared__ double s_norm[DENSE2_MAX];
    __shared__ int s_rot, s_top[3];
    const int tid = threadIdx.x;
    const int m = n + (n & 1);  // an odd n gets a zero column / row of padding
    for (int e = tid; e < m * m; e += 256) {
        const int i = e / m, j = e - i * m;
        double v = 0.0;
        if (i < n && j < n) v = i == j ? 1.0 : 0.5 * (sd[i * n + j] + sd[j * n + i]);
        a[i][j] = v;
    }
    __syncthreads();
    const bool ok = onesided_sweeps(a, m, &s_rot);
    // eigenvalues of S: column norms - 1; the three largest, the two leading unit columns
    if (tid < n) {
        double s2 = 0.0;
        for (int r = 0; r < n; ++r) s2 = fma(a[r][tid], a[r][tid], s2);
        s_norm[tid] = sqrt(s2);
    }
    __syncthreads();
    if (tid < n) {
        const double mine = s_norm[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double o = s_norm[j];
            if (o > mine || (o == mine && j < tid)) ++rank;
        }
        if (rank < 3) s_top[rank] = tid;
    }
    __syncthreads();
    if (tid < 3) w3[tid] = tid < n ? s_norm[s_top[tid]] - 1.0 : 0.0;
    if (tid == 3) w3[3] = ok ? 1.0 : 0.0;
    for (int e = tid; e < 2 * n; e += 256) {
        const int k = e / n, r = e - k * n;
        const int col = s_top[k];
        v2[r * 2 + k] = a[r][col] / s_norm[col];
    }
}

// SVQB (Stathopoulos & Wu): from G = Y^T Y (k x k) build T (k x k) with
// (Y T)^T (Y T) = I on the kept directions; directions whose scaled eigenvalue is
// below drop_tol * largest are dropped (zero column of T, mask 0).
__global__ __launch_bounds__(256) void k_small_svqb(const double *__restrict__ g, int k,
                                                     double drop_tol, double *__restrict__ t,
                                                     int *__restrict__ mask) {
    __shared__ jacobi_lds s;
    __shared__ double dsc[MAXS];
    const int tid = threadIdx.x;
    if (tid < k) {
        const double d = g[tid * k + tid];
        dsc[tid] = d > 1e-290 ? 1.0 / sqrt(d) : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        double v = 0.5 * (g[i * k + j] + g[j * k + i]) * dsc[i] * dsc[j];
        if (dsc[i] == 0.0 || dsc[j] == 0.0) v = 0.0;  // dead column: decoupled, eigenvalue 0
        s.a[i][j] = v;
    }
    __syncthreads();
    jacobi_eig(s, k);
    const double wmax = s.w[0];
    for (int e = tid; e < k * k; e += 256) {
        const int i = e / k, c = e - i * k;
        const double lam = s.w[c];
        const bool keep = wmax > 0.0 && lam > drop_tol * wmax;
        t[i * k + c] = keep ? dsc[i] * s.e[i][s.perm[c]] / sqrt(lam) : 0.0;
    }
    if (tid < k) mask[tid] = (wmax > 0.0 && s.w[tid] > drop_tol * wmax) ? 1 : 0;
}

// Search-direction coefficients of the fused loop (b = 4, 8), one wave, registers and
// wave shuffles only: lane i holds row i of C (the top-b eigenvectors) and of D.
//   D <- the [P R] rows of C;  D <- (I - C C^T) D twice;  then classical Gram-Schmidt with
//   re-orthogonalisation over the columns in Ritz order, a column being dropped (zero,
//   mask 0) when less than drop_tol of its squared norm is left.
// Same role as the SVQB step of the general path below; cheaper because nothing iterates.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int B>
__device__ void rr_directions_wave(const jacobi_lds &s, int nq, double drop_tol,
                                   double *__restrict__ d_out, int *__restrict__ mask_p) {
    const int i = threadIdx.x;  // lane of wave 0
    const bool row = i < nq;
    double c[B], d[B];
#pragma unroll
    for (int k = 0; k < B; ++k) {
        const double v = row ? s.e[i][s.perm[k]] : 0.0;
        c[k] = v;
        d[k] = i >= B ? v : 0.0;
    }
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        double g[B][B];
#pragma unroll
        for (int a = 0; a < B; ++a)
#pragma unroll
            for (int k = 0; k < B; ++k) g[a][k] = row_sum<(3 * B + 15) / 16>(c[a] * d[k]);
#pragma unroll
        for (int k = 0; k < B; ++k)
#pragma unroll
            for (int a = 0; a < B; ++a) d[k] -= c[a] * g[a][k];
    }
    double n0[B];
#pragma unroll
    for (int k = 0; k < B; ++k) n0[k] = row_sum<(3 * B + 15) / 16>(d[k] * d[k]);
    int keep_mask = 0;
#pragma unroll
    for (int k = 0; k < B; ++k) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            double r[B];
#pragma unroll
            for (int j = 0; j < k; ++j) r[j] = row_sum<(3 * B + 15) / 16>(d[j] * d[k]);
#pragma unroll
            for (int j = 0; j < k; ++j) d[k] -= r[j] * d[j];
        }
        const double n1 = row_sum<(3 * B + 15) / 16>(d[k] * d[k]);
        const bool keep = n0[k] > 1e-290 && n1 > drop_tol * n0[k];
        const double sc = keep ? 1.0 / sqrt(n1) : 0.0;
        d[k] *= sc;
        keep_mask |= keep ? (1 << k) : 0;
    }
#pragma unroll
    for (int k = 0; k < B; ++k) {
        if (row) d_out[i * B + k] = d[k];
        if (i == k) mask_p[k] = (keep_mask >> k) & 1;
    }
}

// Rayleigh-Ritz: T (nq x nq) = Q^T A Q on an orthonormal basis Q = [X R P]; mask marks
// live basis columns.  Outputs
//   c (nq x b): top-b eigenvectors  -> X' = Q c,   theta[0..b) their values, theta[b] the next;
//   d (nq x b): coefficients of the next search directions P' = Q d, orthonormal and
//     orthogonal to X' *in coefficient space* (Q is orthonormal, so no tall Gram product is
//     needed): start from the [R P] part of c (the LOBPCG direction), project out c twice,
//     SVQB-orthonormalise with rank-revealing drop; mask_p[k] = 0 marks a dropped direction.
//   nparts > 0: tm holds nparts per-workgroup partials of T (k_gram_qaq), summed here in
//   fixed order.
// (mask, c, d, theta, mask_p may live in LDS: k_panel_rr_solve runs this in front of its panel pass)
// exact_from >= 0 (mixed-precision loop): only the products S Q_i of the columns i < exact_from (the X
// block) are exact -- S R came through the single-precision image of W, and S P is a combination that
// contains it.  Of the two entries of a pair (i < exact_from <= j) only the one with the exact product,
// Q_j^T (S Q_i), is used: the other carries the image's rounding as an ABSOLUTE error, on an entry (the
// coupling of X to a search direction) that is as small as the residual itself.  Inside the X block the
// entry with the product of the LOWER column is used likewise: the columns behind the wanted one take
// long steps along image products, their S X drifts by more, and the mean would rotate that drift into
// the wanted column (measured: a floor of 1.4e-13 ... 3e-13 under the residual of column 0).  Pairs of
// two search directions keep the mean: their entries are O(||S||).
__device__ __forceinline__ void small_rr_body(const double *__restrict__ tm, int nparts, int nq, int b,
                              const int *mask, double *c, double *d, double *theta, int *mask_p,
                              double drop_tol, int exact_from = -1, bool wave_path = true) {
    __shared__ jacobi_lds s;
    __shared__ double cc[3 * MAXB][MAXB];
    __shared__ double dd[3 * MAXB][MAXB];
    __shared__ double gg[MAXB][MAXB];
    __shared__ double dsc[MAXB];
    const int tid = threadIdx.x;
    if (nparts > 0) {
        __shared__ double tmp[8][3 * MAXB * 3 * MAXB / 4];  // fused path: nq <= 24
        // parked in the eigenvector array until symmetrised
        sum_partials(tm, nparts, nq * nq, tmp, [&](int e, double v) { s.e[e / nq][e % nq] = v; });
    }
    for (int e = tid; e < nq * nq; e += 256) {
        const int i = e / nq, j = e - i * nq;
        double v = nparts > 0 ? 0.5 * (s.e[i][j] + s.e[j][i])
                              : 0.5 * (tm[i * nq + j] + tm[j * nq + i]);
        if (exact_from >= 0 && nparts > 0 && i != j && (i < exact_from || j < exact_from))
            v = i < j ? s.e[j][i] : s.e[i][j];
        const bool live = mask[i] && mask[j];
        if (!live) v = (i == j) ? -1e30 : 0.0;  // dead directions can never be selected
        s.a[i][j] = v;
    }
    __syncthreads();
    jacobi_eig(s, nq);
    for (int e = tid; e < nq * b; e += 256) {
        const int i = e / b, k = e - i * b;
        const double v = s.e[i][s.perm[k]];
        cc[i][k] = v;
        dd[i][k] = i >= b ? v : 0.0;
        c[e] = v;
    }
    if (tid <= b && tid < nq) theta[tid] = s.w[tid];
    __syncthreads();
    if (nq == b) return;  // plain rotation of X (start-up / refresh): no search directions
    // (wave_path = false: the debug hook's general path at these sizes, DESIGN.md section 35 -- a constant
    // in every kernel, so the product kernels compile as before)
    if (wave_path && nq == 3 * b && (b == 4 || b == 8)) {
        if (tid < 64) {
            if (b == 4) rr_directions_wave<4>(s, nq, drop_tol, d, mask_p);
            else rr_directions_wave<8>(s, nq, drop_tol, d, mask_p);
        }
        return;
    }
    // D <- (I - C C^T) D, twice
    for (int pass = 0; pass < 2; ++pass) {
        for (int e = tid; e < b * b; e += 256) {
            const int a = e / b, k = e - a * b;
            double g = 0.0;
            for (int i = 0; i < nq; ++i) g += cc[i][a] * dd[i][k];
            gg[a][k] = g;
        }
        __syncthreads();
        for (int e = tid; e < nq * b; e += 256) {
            const int i = e / b, k = e - i * b;
            double v = dd[i][k];
            for (int a = 0; a < b; ++a) v -= cc[i][a] * gg[a][k];
            dd[i][k] = v;
        }
        __syncthreads();
    }
    // SVQB on D (b columns in an nq-dimensional coefficient space)
    for (int e = tid; e < b * b; e += 256) {
        const int a = e / b, k = e - a * b;
        double g = 0.0;
        for (int i = 0; i < nq; ++i) g += dd[i][a] * dd[i][k];
        gg[a][k] = g;
    }
    __syncthreads();
    if (tid < b) dsc[tid] = gg[tid][tid] > 1e-290 ? 1.0 / sqrt(gg[tid][tid]) : 0.0;
    __syncthreads();
    for (int e = tid; e < b * b; e += 256) {
        const int a = e / b, k = e - a * b;
        s.a[a][k] = 0.5 * (gg[a][k] + gg[k][a]) * dsc[a] * dsc[k];
    }
    __syncthreads();
    jacobi_eig(s, b);
    const double wmax = s.w[0];
    // transform T = diag(dsc) U Lambda^-1/2 (dropped columns zero), D_hat = D T
    for (int e = tid; e < b * b; e += 256) {
        const int a = e / b, k = e - a * b;
        const double lam = s.w[k];
        const bool keep = wmax > 0.0 && lam > drop_tol * wmax;
        gg[a][k] = keep ? dsc[a] * s.e[a][s.perm[k]] / sqrt(lam) : 0.0;
    }
    if (tid < b) mask_p[tid] = (wmax > 0.0 && s.w[tid] > drop_tol * wmax) ? 1 : 0;
    __syncthreads();
    for (int e = tid; e < nq * b; e += 256) {
        const int i = e / b, k = e - i * b;
        double v = 0.0;
        for (int a = 0; a < b; ++a) v += dd[i][a] * gg[a][k];
        d[e] = v;
    }
}

__global__ __launch_bounds__(256) void k_small_rr(const double *__restrict__ tm, int nparts,
                                                   int nq, int b, const int *__restrict__ mask,
                                                   double *__restrict__ c, double *__restrict__ d,
                                                   double *__restrict__ theta,
                                                   int *__restrict__ mask_p, double drop_tol,
                                                   int exact_from = -1) {
    small_rr_body(tm, nparts, nq, b, mask, c, d, theta, mask_p, drop_tol, exact_from);
}

// The b x b rotation of X that closes start-up and a confirmation, with the masks it needs and leaves set
// here instead of by two launches of their own: all 48 slots live going in, P's slots dead coming out
// (no search directions yet).  mask: the 48 ints; the solve itself is k_small_rr's with nq = b.
__global__ __launch_bounds__(256) void k_small_rr_start(const double *__restrict__ tm, int b, int *mask,
                                                         double *__restrict__ c, double *__restrict__ d,
                                                         double *__restrict__ theta, double drop_tol) {
    if (threadIdx.x < 48) mask[threadIdx.x] = 1;
    __syncthreads();
    small_rr_body(tm, 0, b, b, mask, c, d, theta, mask + b, drop_tol);
    __syncthreads();
    if ((int)threadIdx.x < b) mask[b + threadIdx.x] = 0;
}

// Projected SVQB (fused path, b <= 8).  Input: per-workgroup partials of
//   Cxp = [x p]^T r (2b x b),  G = r^T r (b x b),  cu = u^T r (1 x b)
// for an orthonormal [u x p].  With M = G - Cxp^T Cxp - cu^T cu (the Gram matrix of r
// after projecting [u x p] out) and M = D^-1 V L V^T D^-1 its scaled eigen-decomposition,
// T = D V L^-1/2 and K = -C T make   r T + [x p u] K   orthonormal and orthogonal to
// [u x p] up to the cancellation in M -- a second pass of the same step removes that.
// Output coef: rows [x (b) | p (b) | r (b) | u | 3 zero rows] x b, the operand of
// k_panel_tf; mask[c] = 0 marks a dropped direction (zero column).
// report (mapped host memory, may be null): [0, b) squared residual norms diag(G),
// [16, 16 + b] the current Ritz values, [40] the caller's sequence number, written last.
// (coef may live in LDS, mask may be null: k_panel_tf_solve runs this in front of its panel pass)
// (the working set is a template parameter: the general one below, or the compact one of a single block
// width -- same arithmetic, same bits)
struct orth_lds {
    jacobi_lds s;
    double cxp[16][8], gm[9][8], mm[8][8], tt[8][8], dsc[8];
    double tmp[8][3 * MAXB * 3 * MAXB / 4];
    __device__ void eig(int b) { jacobi_eig(s, b); }
};
template <int B>
struct orth_small_lds {
    jacobi_small_lds<B> s;
    double cxp[2 * B][B], gm[B + 1][B], mm[B][B], tt[B][B], dsc[B];
    double tmp[8][3 * B * B + B];
    double coef[PANEL_COEF_ROWS<B> * B];
    panel_red_t red;
    __device__ void eig(int) { jacobi_eig_waves<B>(s); }
};

template <typename ST>
__device__ __forceinline__ void small_orth_core(ST &L, const double *__restrict__ partial, int nparts, int b,
                                                double drop_tol, double *coef, int *mask,
                                                const double *__restrict__ theta, double *report, double seq) {
    auto &s = L.s;
    auto &cxp = L.cxp;
    auto &gm = L.gm;
    auto &mm = L.mm;
    auto &tt = L.tt;
    auto &dsc = L.dsc;
    const int tid = threadIdx.x;
    const int nxp = 2 * b * b, nout = 3 * b * b + b;
    sum_partials(partial, nparts, nout, L.tmp, [&](int e, double v) {
        if (e < nxp) cxp[e / b][e % b] = v;
        else gm[(e - nxp) / b][(e - nxp) % b] = v;
    });
    if (report) {
        // hand the norms to the host through mapped memory: data, system-scope fence, then the
        // sequence number the host is polling for (no stream event: recording one costs the
        // device a ~6 us bubble).  seq < 0: the caller sends the sequence number itself, later
        // (report_sequence): the fence then finds the stores long done instead of waiting a PCIe
        // round trip for them in front of the workgroup's rows.
        if (tid < b) report[tid] = gm[tid][tid];
        if (tid <= b) report[16 + tid] = theta[tid];
        if (seq >= 0.0) {
            __threadfence_system();
            __syncthreads();
            if (tid == 0) {
                ((volatile double *)report)[40] = seq;
                __threadfence_system();
            }
        }
    }
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, j = e - i * b;
        double v = 0.5 * (gm[i][j] + gm[j][i]) - gm[b][i] * gm[b][j];
        for (int k = 0; k < 2 * b; ++k) v -= cxp[k][i] * cxp[k][j];
        mm[i][j] = v;
    }
    __syncthreads();
    if (tid < b) {
        // a column whose projected norm^2 is at the cancellation floor of G carries no
        // direction of its own: dead
        const double dgn = mm[tid][tid];
        dsc[tid] = (dgn > 1e-290 && dgn > 1e-13 * gm[tid][tid]) ? 1.0 / sqrt(dgn) : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, j = e - i * b;
        s.a[i][j] = 0.5 * (mm[i][j] + mm[j][i]) * dsc[i] * dsc[j];
    }
    __syncthreads();
    L.eig(b);
    const double wmax = s.w[0];
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, c = e - i * b;
        const double lam = s.w[c];
        const bool keep = wmax > 0.0 && lam > drop_tol * wmax;
        tt[i][c] = keep ? dsc[i] * s.e[i][s.perm[c]] / sqrt(lam) : 0.0;
    }
    if (mask && tid < b) mask[tid] = (wmax > 0.0 && s.w[tid] > drop_tol * wmax) ? 1 : 0;
    __syncthreads();
    for (int e = tid; e < (3 * b + 4) * b; e += 256) {
        const int k = e / b, c = e - k * b;
        double v = 0.0;
        if (k < 2 * b) {
            for (int i = 0; i < b; ++i) v -= cxp[k][i] * tt[i][c];
        } else if (k < 3 * b) {
            v = tt[k - 2 * b][c];
        } else if (k == 3 * b) {
            for (int i = 0; i < b; ++i) v -= gm[b][i] * tt[i][c];
        }
        coef[e] = v;
    }
}

__device__ __forceinline__ void small_orth_body(const double *__restrict__ partial, int nparts, int b,
                                                double drop_tol, double *coef, int *mask,
                                                const double *__restrict__ theta, double *report, double seq) {
    __shared__ orth_lds L;
    small_orth_core(L, partial, nparts, b, drop_tol, coef, mask, theta, report, seq);
}

__global__ __launch_bounds__(256) void k_small_orth(const double *__restrict__ partial,
                                                     int nparts, int b, double drop_tol,
                                                     double *__restrict__ coef,
                                                     int *__restrict__ mask,
                                                     const double *__restrict__ theta,
                                                     double *report, double seq) {
    small_orth_body(partial, nparts, b, drop_tol, coef, mask, theta, report, seq);
}

// ---- the small solves in FRONT of the tall kernels that consume them
// A one-workgroup kernel between two tall ones costs its launch and the drain of the one before
// (~5 us a time, three times an iteration).  The tall kernel's workgroups can each run the small
// solve themselves, redundantly -- same partials, same code, same bits in every workgroup --
// and go straight on to their rows with the coefficients in LDS; workgroup 0 also publishes what
// later kernels and the host read (Ritz values, masks, the residual report).  Nothing is shared
// between the workgroups inside the kernel, so there is no release / acquire across XCDs (the
// variant that ran the solve in the TAIL of the producing kernel paid for exactly that,
// scs_panel.h).  Partials alternate between two buffers: a workgroup still summing the incoming
// ones must not see another one's outgoing ones; the search-direction mask alternates likewise.
template <int B>
__global__ __launch_bounds__(256) void k_panel_rr_solve(double *q, double *aq,
                                                         const double *__restrict__ u,
                                                         const double *__restrict__ tm, int nparts_in,
                                                         int solve, double *theta_g,
                                                         const int *__restrict__ maskp_in,
                                                         const int *__restrict__ mask_r,
                                                         int *maskp_out, double drop_tol, int n,
                                                         double *__restrict__ partial,
                                                         const double *__restrict__ dinv = nullptr,
                                                         double *__restrict__ zt = nullptr, int64_t ldz = 0,
                                                         int exact_from = -1) {
    __shared__ double c_s[3 * B * B], d_s[3 * B * B], th_s[B + 4];
    __shared__ int live_s[3 * B], mp_s[B];
    const int tid = threadIdx.x;
    // the rows' operands are on their way while the solve runs (scs_panel.h: load part / compute part)
    panel_rr_ops<B> pre[PANEL_PRE];
    panel_rr_prefetch<B>(pre, q, aq, u, dinv, zt != nullptr, n);
    if (solve) {
        if (tid < 3 * B) live_s[tid] = tid < B ? 1 : (tid < 2 * B ? maskp_in[tid - B] : mask_r[tid - 2 * B]);
        __syncthreads();
        small_rr_body(tm, nparts_in, 3 * B, B, live_s, c_s, d_s, th_s, mp_s, drop_tol, exact_from);
    } else {
        // first iteration, and after a refresh: X stays, no search directions
        for (int e = tid; e < 3 * B * B; e += 256) {
            c_s[e] = (e / B == e % B) ? 1.0 : 0.0;
            d_s[e] = 0.0;
        }
        if (tid <= B) th_s[tid] = theta_g[tid];
        if (tid < B) mp_s[tid] = 0;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (solve && tid <= B) theta_g[tid] = th_s[tid];
        if (tid < B) maskp_out[tid] = mp_s[tid];
    }
    panel_rr_run<B>(pre, q, aq, u, c_s, d_s, th_s, n, partial, dinv, zt, ldz);
}

template <int B, bool GRAM, bool WRITE_Z>
__global__ __launch_bounds__(256) void k_panel_tf_solve(double *q, const double *__restrict__ u,
                                                         const double *__restrict__ part_in,
                                                         int nparts_in, double drop_tol, int *mask_r,
                                                         const double *__restrict__ theta_g,
                                                         double *report, double seq, int n,
                                                         double *__restrict__ partial,
                                                         const double *__restrict__ dinv,
                                                         double *__restrict__ zt, int64_t ldz) {
    __shared__ double coef_s[PANEL_COEF_ROWS<B> * B];
    const bool lead = blockIdx.x == 0;
    panel_tf_ops<B> pre[PANEL_PRE];
    panel_tf_prefetch<B, GRAM, WRITE_Z>(pre, q, u, dinv, n);
    small_orth_body(part_in, nparts_in, B, drop_tol, coef_s, lead ? mask_r : nullptr, theta_g,
                    lead ? report : nullptr, -1.0);
    __syncthreads();
    panel_tf_run<B, GRAM, WRITE_Z>(pre, q, u, coef_s, n, partial, dinv, zt, ldz);
    if (lead && report) {
        // the report's sequence number, after the rows (the end of the kernel makes it visible)
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) ((volatile double *)report)[40] = seq;
    }
}

// Pass 2 of the orthonormalisation of R folded into the Gram kernel (scs_panel.h, round 5): the
// small solve on pass 1's Gram partials in front, then R and S R transformed on the way to Q^T S Q.
template <int B, int FINISH>
__global__ __launch_bounds__(256) void k_panel_gram_tf_solve(double *q, double *aq, const double *__restrict__ u,
                                                              const double *__restrict__ part_in, int nparts_in,
                                                              int *mask_r, const double *__restrict__ theta_g, int n,
                                                              const double *__restrict__ ypart, int nseg,
                                                              const double *__restrict__ dinv,
                                                              double *__restrict__ partial, int64_t chunk = 0,
                                                              const int32_t *__restrict__ splits = nullptr,
                                                              const double *__restrict__ coef1 = nullptr) {
    constexpr int NC = PANEL_COEF_ROWS<B> * B;
    __shared__ double coef_s[NC], coefa_s[NC];
    const bool lead = blockIdx.x == 0;
    panel_gram_tf_ops<B> pre[PANEL_PRE];
    panel_gram_tf_prefetch<B, FINISH>(pre, q, aq, u, n, ypart, nseg, dinv, chunk, splits);
    small_orth_body(part_in, nparts_in, B, 0.0, coef_s, lead ? mask_r : nullptr, theta_g, nullptr, -1.0);
    __syncthreads();
    // coef1 (overlapped loop, k_symm_tri_tf): the operator was applied to the RAW residual block R~, and
    // pass 1 made R1 = R~ T1 + [x p u] K1 beside it.  With pass 2's R2 = R1 T2 + [x p u] K2:
    //   S R2 = (S R~) T1 T2 + S [x p u] (K1 T2 + K2)
    for (int e = threadIdx.x; e < NC; e += 256) {
        const int k = e / B, c = e - k * B;
        double v = coef_s[e];
        if (coef1) {
            if (k >= 2 * B && k < 3 * B) v = 0.0;
            for (int i = 0; i < B; ++i) v += coef1[k * B + i] * coef_s[(2 * B + i) * B + c];
        }
        coefa_s[e] = v;
    }
    __syncthreads();
    panel_gram_tf_body<B, FINISH>(pre, q, aq, u, coef_s, coefa_s, n, ypart, nseg, dinv, partial, chunk, splits);
}

// Pass 1 of that orthonormalisation INSIDE the SYMM launch (round 5): the first n_tf workgroups run it
// (small solve on the compact LDS layout, then their share of the rows) while the others stream W against
// the raw residual block.  The two roles share the workgroup's LDS; nothing passes between them inside
// the launch.  Workgroup 0 publishes pass 1's coefficients for the Gram kernel (above).
template <int B, int CT, int RPW, int D, typename WT = double>
__global__ __launch_bounds__(256, 2) void k_symm_tri_tf(const WT *__restrict__ w, int64_t ld, int n,
                                                        const double *__restrict__ zt, int64_t ldz,
                                                        const int2 *__restrict__ tiles,
                                                        double *__restrict__ pdir, double *__restrict__ ptr_,
                                                        int n_tf, double *q, const double *__restrict__ u,
                                                        const double *__restrict__ part_in, int nparts_in,
                                                        double drop_tol, int *mask_r,
                                                        const double *__restrict__ theta_g, double *report,
                                                        double seq, double *__restrict__ partial,
                                                        double *__restrict__ coef_out) {
    union lds_t {
        symm_tri_lds<B, CT, WT> symm;
        orth_small_lds<B> tf;
    };
    __shared__ lds_t lds;
    const int bid = blockIdx.x;
    if (bid >= n_tf) {
        symm_tri_body<B, CT, RPW, D, WT>(w, ld, n, zt, ldz, tiles[bid - n_tf], pdir, ptr_, 0, lds.symm);
        return;
    }
    const bool lead = bid == 0;
    // the rows' operands ahead of the solve (scs_panel.h) at width 4 only: at width 8 the solve's
    // registers and two groups of operands do not fit the 256 VGPRs that two workgroups per CU leave
    // (measured on the code object: 44 registers spilled to scratch), so there the loads follow it
    constexpr bool AHEAD = B == 4;
    panel_tf_ops<B> pre[PANEL_PRE];
    if (AHEAD) panel_tf_prefetch<B, true, false>(pre, q, u, nullptr, n, bid, n_tf);
    small_orth_core(lds.tf, part_in, nparts_in, B, drop_tol, lds.tf.coef, lead ? mask_r : nullptr, theta_g,
                    lead ? report : nullptr, -1.0);
    __syncthreads();
    if (!AHEAD) panel_tf_prefetch<B, true, false>(pre, q, u, nullptr, n, bid, n_tf);
    if (lead)
        for (int e = threadIdx.x; e < PANEL_COEF_ROWS<B> * B; e += 256) coef_out[e] = lds.tf.coef[e];
    panel_tf_run<B, true, false>(pre, q, u, lds.tf.coef, n, partial, nullptr, nullptr, 0, bid, n_tf, &lds.tf.red);
    if (lead && report) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) ((volatile double *)report)[40] = seq;
    }
}

// c = first b columns of the 3b x 3b identity, d = 0: the Rayleigh-Ritz coefficients that
// leave X alone and clear the search directions (first iteration, and after a refresh)
__global__ void k_unit_coeffs(double *__restrict__ c, double *__restrict__ d, int b) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3 * b * b) return;
    c[e] = (e / b == e % b) ? 1.0 : 0.0;
    d[e] = 0.0;
}

// dense S for the small-V path: s[i][j] = dinv[i] * w[i][j] * dinv[j], zero diagonal
__global__ void k_dense_s(const double *__restrict__ w, int64_t ld, int n,
                          const double *__restrict__ dinv, double *__restrict__ s) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int i = idx / n, j = idx - i * n;
    s[idx] = i == j ? 0.0 : dinv[i] * w[(int64_t)i * ld + j] * dinv[j];
}

// ---------------------------------------------------------------------------
// matrix-free graphs (scs_matfree.h): creation, the operator, release
// ---------------------------------------------------------------------------
void scs_matfree_release(scs_graph *g) {
    mf_data *m = g->mf;
    if (!m) return;
    scs_dev_free(m->d_stack_off);
    scs_dev_free(m->st_val);
    scs_dev_free(m->st_sum);
    scs_dev_free(m->st_dep);
    scs_dev_free(m->sm_val);
    scs_dev_free(m->sm_sum);
    scs_dev_free(m->sm_dep);
    scs_dev_free(m->cy_pa);
    scs_dev_free(m->cy_ps);
    scs_dev_free(m->cy_dep);
    scs_dev_free(m->sm_cnt);
    scs_dev_free(m->sm_root);
    scs_dev_free(m->cy_cnt);
    scs_dev_free(m->x);
    scs_dev_free(m->y);
    scs_dev_free(m->slabs);
    delete m;
    g->mf = nullptr;
}

extern "C" int scs_graph_matrix_free(scs_ctx *ctx, const scs_tables *tb, int32_t max_block, scs_graph **out) {
    SCS_REQUIRE(ctx && tb && out, "scs_graph_matrix_free: null argument");
    SCS_REQUIRE(max_block == 4 || max_block == 8, "scs_graph_matrix_free: widest block 4 or 8 (asked: %d)", max_block);
    SCS_REQUIRE(ctx->comm.world == 1, "scs_graph_matrix_free: one device only (a measured comparison, DESIGN.md)");
    SCS_REQUIRE(tb->n_taxa > DENSE2_MAX, "scs_graph_matrix_free: more than %d taxa (the dense small paths need W)", DENSE2_MAX);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    SCS_TRY(scs_tables_finish(ctx, tb));
    hipStream_t s = ctx->stream;
    const int n = tb->n_taxa, M = tb->n_trees;
    auto *g = new scs_graph();
    g->n = n;
    g->row_begin = 0;
    g->row_end = n;
    g->ld = scs_round_up(n, SCS_LD_ALIGN);
    g->mf = new mf_data();
    mf_data *m = g->mf;
    m->tb = tb;
    m->b_cap = max_block;
    auto fail = [&](int rc) {
        scs_matfree_release(g);
        delete g;
        return rc;
    };
    // strips: a tree's stack never holds more entries than its deepest separator
    int32_t *d_maxd = nullptr;
    if (scs_dev_malloc((scs_ctx *)nullptr, (void **)&d_maxd, (size_t)M * 4) != hipSuccess) return fail(SCS_ENOMEM);
    hipMemsetAsync(d_maxd, 0, (size_t)M * 4, s);
    k_mf_maxdepth<<<(unsigned)(((tb->n_leaves + 63) / 64 + 255) / 256), 256, 0, s>>>(tb->d_tree_off, M, tb->d_adj_depth,
                                                                                     tb->n_leaves, d_maxd);
    std::vector<int32_t> &maxd = m->maxd;  // kept: scs_debug_matrix_free_plan reports it
    maxd.assign((size_t)M, 0);
    hipError_t e = hipMemcpyAsync(maxd.data(), d_maxd, (size_t)M * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    scs_dev_free(d_maxd);
    if (e != hipSuccess) {
        scs_set_error("scs_graph_matrix_free: %s", hipGetErrorString(e));
        return fail(SCS_EHIP);
    }
    std::vector<int64_t> soff((size_t)M + 1, 0);
    for (int t = 0; t < M; ++t) soff[t + 1] = soff[t] + maxd[t] + 1;
    m->stack_total = soff[M];
    // chunks per direction: pieces of a few hundred leaves, at most 16
    m->chunks = std::max(1, std::min(16, tb->max_leaves / 256));
    const size_t strips = (size_t)2 * max_block * (size_t)m->chunks * (size_t)m->stack_total;
    const size_t slots = (size_t)2 * max_block * (size_t)m->chunks * (size_t)M;
    const size_t slab_bytes = (size_t)2 * M * (size_t)n * max_block * 8;
    // (every request by name and size: the message of a failure quotes the bytes that were asked for)
    const size_t strip_n = std::max<size_t>(strips, 1);
    const struct {
        void **p;
        size_t bytes;
        const char *what;
    } want[] = {{(void **)&m->d_stack_off, (size_t)(M + 1) * 8, "strip offsets"},
                {(void **)&m->st_val, strip_n * 8, "stack strips (values)"},
                {(void **)&m->st_sum, strip_n * 8, "stack strips (sums)"},
                {(void **)&m->st_dep, strip_n * 4, "stack strips (depths)"},
                {(void **)&m->sm_val, strip_n * 8, "summary strips (values)"},
                {(void **)&m->sm_sum, strip_n * 8, "summary strips (sums)"},
                {(void **)&m->sm_dep, strip_n * 4, "summary strips (depths)"},
                {(void **)&m->cy_pa, strip_n * 8, "carry strips (value prefix sums)"},
                {(void **)&m->cy_ps, strip_n * 8, "carry strips (prefix sums)"},
                {(void **)&m->cy_dep, strip_n * 4, "carry strips (depths)"},
                {(void **)&m->sm_cnt, slots * 4, "summary counts"},
                {(void **)&m->sm_root, slots * 4, "root flags"},
                {(void **)&m->cy_cnt, slots * 4, "carry counts"},
                {(void **)&m->x, (size_t)n * max_block * 8, "operand"},
                {(void **)&m->y, (size_t)n * max_block * 8, "result"},
                {(void **)&m->slabs, slab_bytes, "slabs"}};
    size_t asked = 0;
    for (const auto &w : want) {
        asked += w.bytes;
        if (scs_dev_malloc((scs_ctx *)nullptr, w.p, w.bytes) != hipSuccess) {
            (void)hipGetLastError();
            scs_set_error("scs_graph_matrix_free: cannot allocate %.3f GB of %s (%.3f GB asked for so far; the nine "
                          "strip arrays take %.3f GB, the slabs %.3f GB)",
                          w.bytes / 1073741824.0, w.what, asked / 1073741824.0,
                          (6.0 * 8 + 3.0 * 4) * strip_n / 1073741824.0, slab_bytes / 1073741824.0);
            return fail(SCS_ENOMEM);
        }
    }
    e = hipMemcpyAsync(m->d_stack_off, soff.data(), (size_t)(M + 1) * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(m->slabs, 0, slab_bytes, s);  // taxa a tree does not hold stay zero
    if (e == hipSuccess) e = hipStreamSynchronize(s);                      // (`soff` goes out of scope)
    if (e != hipSuccess) {
        scs_set_error("scs_graph_matrix_free: %s", hipGetErrorString(e));
        return fail(SCS_EHIP);
    }
    *out = g;
    return SCS_OK;
}

// zt == null: the vector of ones (the degrees: column 0 of the result goes to g->d_deg)
int scs_matfree_apply(scs_ctx *ctx, scs_graph *g, const double *zt, int64_t ldz, int b, double *y_out,
                      hipStream_t s) {
    mf_data *m = g->mf;
    SCS_REQUIRE(m && (b == 4 || b == 8) && b <= m->b_cap, "matrix-free apply: block width %d (graph made for %d)", b,
                m ? m->b_cap : 0);
    const scs_tables *tb = m->tb;
    const int n = g->n, M = tb->n_trees;
    const int64_t nb = (int64_t)n * b;
    if (m->slabs_b != b) {
        // another width lays the slabs out differently: entries of taxa a tree does not hold must be zero
        SCS_HIP_CHECK(hipMemsetAsync(m->slabs, 0, (size_t)2 * M * (size_t)n * b * 8, s));
        m->slabs_b = b;
    }
    if (zt) {
        if (b == 4) k_mf_operand<4><<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(zt, ldz, n, m->x);
        else k_mf_operand<8><<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(zt, ldz, n, m->x);
    } else {
        k_mf_fill<<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(m->x, nb, 1.0);
    }
    mf_params a;
    a.tree_off = tb->d_tree_off;
    a.leaf_taxon = tb->d_leaf_taxon;
    a.adj_depth = tb->d_adj_depth;
    a.adj_val = tb->d_adj_val;
    a.tree_w = tb->d_tree_w;
    a.stack_off = m->d_stack_off;
    a.n_trees = M;
    a.n_taxa = n;
    a.stack_total = m->stack_total;
    a.st_val = m->st_val;
    a.st_sum = m->st_sum;
    a.st_dep = m->st_dep;
    a.x = m->x;
    a.y_slabs = m->slabs;
    a.chunks = m->chunks;
    a.sm_dep = m->sm_dep;
    a.sm_val = m->sm_val;
    a.sm_sum = m->sm_sum;
    a.cy_dep = m->cy_dep;
    a.cy_pa = m->cy_pa;
    a.cy_ps = m->cy_ps;
    a.sm_cnt = m->sm_cnt;
    a.sm_root = m->sm_root;
    a.cy_cnt = m->cy_cnt;
    const int64_t units = (int64_t)M * 2 * b;
    const int64_t threads = units * m->chunks;
    double *y = y_out ? y_out : m->y;
    // (strips are laid out for the graph's widest block; a narrower one uses a prefix of the units)
    if (b == 4) {
        k_mf_chunk<4, false><<<(unsigned)((threads + 63) / 64), 64, 0, s>>>(a);
        k_mf_carry<4><<<(unsigned)((units + 63) / 64), 64, 0, s>>>(a);
        k_mf_chunk<4, true><<<(unsigned)((threads + 63) / 64), 64, 0, s>>>(a);
        k_mf_reduce<4><<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(m->slabs, M, n, y);
    } else {
        k_mf_chunk<8, false><<<(unsigned)((threads + 63) / 64), 64, 0, s>>>(a);
        k_mf_carry<8><<<(unsigned)((units + 63) / 64), 64, 0, s>>>(a);
        k_mf_chunk<8, true><<<(unsigned)((threads + 63) / 64), 64, 0, s>>>(a);
        k_mf_reduce<8><<<(unsigned)((nb + 255) / 256), 256, 0, s>>>(m->slabs, M, n, y);
    }
    if (!zt) k_mf_column0<<<(n + 255) / 256, 256, 0, s>>>(y, n, b, g->d_deg);
    SCS_HIP_CHECK(hipGetLastError());
    ++m->n_apply;
    return SCS_OK;
}

// what scs_graph_matrix_free planned and where the graph stands: host fields only, no launch
extern "C" int scs_debug_matrix_free_plan(const scs_graph *g, int64_t *info_out, int32_t *maxd_out) {
    SCS_REQUIRE(g && info_out, "scs_debug_matrix_free_plan: null argument");
    SCS_REQUIRE(g->mf, "scs_debug_matrix_free_plan: the graph has a matrix (only scs_graph_matrix_free plans a walk)");
    const mf_data *m = g->mf;
    info_out[0] = m->chunks;
    info_out[1] = m->stack_total;
    info_out[2] = m->b_cap;
    info_out[3] = m->slabs_b;
    info_out[4] = m->n_apply;
    info_out[5] = (int64_t)m->maxd.size();
    if (maxd_out && !m->maxd.empty()) memcpy(maxd_out, m->maxd.data(), m->maxd.size() * sizeof(int32_t));
    return SCS_OK;
}

// ---------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------
namespace {

// a device block from the calling context's cache (scs_block_alloc): the entry points below
// name their context in t_ctx before the first allocation
thread_local scs_ctx *t_ctx = nullptr;

struct dbuf {
    void *p = nullptr;
    scs_ctx *owner = nullptr;
    ~dbuf() {
        if (p && owner) scs_block_release(owner, p);
        else if (p) scs_dev_free(p);
    }
    int alloc(size_t bytes) {
        if (t_ctx) {
            owner = t_ctx;
            return scs_block_alloc(t_ctx, bytes, &p);
        }
        SCS_HIP_CHECK(scs_dev_malloc((scs_ctx *)nullptr, &p, bytes ? bytes : 16));
        return SCS_OK;
    }
    double *d() const { return (double *)p; }
};

struct solver {
    scs_ctx *ctx = nullptr;
    scs_graph *g = nullptr;
    hipStream_t s = nullptr;
    int n = 0, b = 0, rows = 0, world = 1;
    bool use_mfma = true;
    dbuf q, aq, z, ypart, yloc, yfull, recv, u, part, part2, part3, small, splits_d;
    // round 5: the second orthonormalisation pass of R rides the Gram kernel behind the SYMM stream
    // (k_panel_gram_tf_solve; SCS_FOLD_PASS2=0 keeps it as a launch of its own in front of the stream)
    bool fold_pass2 = false;
    // ... and the first pass rides the SYMM launch itself (k_symm_tri_tf: one device, symmetric schedule;
    // SCS_OVERLAP_PASS1=0 keeps it in front)
    bool overlap_pass1 = false;
    struct {
        bool armed = false;
        double drop_tol = 0.0, seq = 0.0;
        double *report = nullptr;
    } tf1;
    dbuf coef1;
    // round 5, mixed precision: while use32 is set the symmetric SYMM streams the single-precision image
    // of W (g->d_w32, half the bytes; products and sums stay in double precision) -- the operator applied
    // to SEARCH DIRECTIONS only; S X and S P are renewed through W itself (scs_fiedler)
    bool use32 = false;
    bool gram_from32 = false;  // the Gram partials waiting for the next Rayleigh-Ritz solve hold image products
    int n_apply32 = 0;
    std::vector<char> ev32;  // per timed launch in `ev`: streamed the image
    const double *fold_u = nullptr;
    int *fold_mask_r = nullptr;
    const double *fold_theta = nullptr;
    size_t ypart_cap = 0;
    int64_t chunk = 0;
    int gram_blocks = 0;
    std::vector<int32_t> splits;
    // timing of SYMM launches
    std::vector<hipEvent_t> ev;
    std::vector<hipEvent_t> ev_ag;  // pairs around the timed all-gathers (multi-rank solves)
    hipEvent_t ev_cal[2] = {nullptr, nullptr};  // an empty pair (calibration)
    bool time_ag = false;           // set by fused_back for the launches it times
    int n_allgather = 0;
    int n_apply = 0;

    ~solver() {
        if (ctx) {
            ctx->event_pool.insert(ctx->event_pool.end(), ev.begin(), ev.end());
            ctx->event_pool.insert(ctx->event_pool.end(), ev_ag.begin(), ev_ag.end());
            for (auto e : ev_cal)
                if (e) ctx->event_pool.push_back(e);
        } else {
            for (auto e : ev_cal)
                if (e) hipEventDestroy(e);
            for (auto e : ev) hipEventDestroy(e);
            for (auto e : ev_ag) hipEventDestroy(e);
        }
    }
    int new_event(hipEvent_t *e) {
        if (ctx && !ctx->event_pool.empty()) {
            *e = ctx->event_pool.back();
            ctx->event_pool.pop_back();
            return SCS_OK;
        }
        SCS_HIP_CHECK(hipEventCreate(e));
        return SCS_OK;
    }

    double *small_at(int off) const { return small.d() + off; }

    // ---- set-up.  The local part is `bind` and then alloc_symm_buffers; the team part is team_splits
    // (COLLECTIVE: scs_fiedler and scs_debug_team_apply only) and then team_buffers.  The callers allocate
    // their own panels and yloc in between, each in the order it always had.
    // (`g` stays null for the exports that only reach gram / update)
    void bind(scs_ctx *c, int n_, int b_ = 0, scs_graph *g_ = nullptr) {
        ctx = c;
        g = g_;
        s = c->stream;
        n = n_;
        b = b_;
        rows = g ? g->row_end - g->row_begin : 0;
        world = c->comm.world;
        gram_blocks = 256;
    }
    int team_splits() {
        SCS_TRY(scs_gather_row_splits(ctx, g->row_begin, g->row_end, g->n, splits));
        int max_rows = 0;
        for (int r = 0; r < world; ++r) max_rows = std::max(max_rows, splits[r + 1] - splits[r]);
        chunk = g->upper ? (int64_t)n * b : (int64_t)max_rows * b;  // (upper: whole partial products travel)
        return SCS_OK;
    }
    // (after alloc_symm_buffers, which decides part_mode)
    int team_buffers() {
        if (world == 1 || part_mode) return SCS_OK;
        SCS_TRY(yfull.alloc((size_t)n * b * 8));
        SCS_TRY(recv.alloc((size_t)chunk * world * 8));
        SCS_TRY(splits_d.alloc((size_t)(world + 1) * 4));
        SCS_HIP_CHECK(hipMemcpyAsync(splits_d.p, splits.data(), (size_t)(world + 1) * 4, hipMemcpyHostToDevice, s));
        return SCS_OK;
    }

    // Where the loop may stream the single-precision image, as far as the graph's layout and the width say:
    // whole rows of W at width 4, either all of them on one rank (alloc_symm_buffers then picks the symmetric
    // schedule, whose 256-column tiles -- tri_ct == 2, the only width it sets -- the image's own tile list
    // sits behind) or a row-partitioned rank's (k_symm).  Asked before the solver is set up (the width choice
    // and the degree pass depend on it), so it reads the graph and not the solver.  scs_fiedler adds its
    // switches and the byte cap; the debug exports add nothing.
    static bool image_layout(const scs_ctx *ctx, const scs_graph *g, int b) {
        const int world = ctx->comm.world;
        const bool one = world == 1 && !g->upper && g->row_begin == 0 && g->row_end == g->n;
        const bool row_ranks = world > 1 && !g->upper;  // (part_mode is g->upper)
        return !g->mf && g->n >= 4096 && b == 4 && (one || row_ranks);
    }

    // the all-gather of an iteration, timed with its own event pair when fused_back times the launch
    int gather(const double *send, double *recvb, size_t count) {
        hipEvent_t a = nullptr, b = nullptr;
        if (time_ag) {
            SCS_TRY(new_event(&a));
            SCS_TRY(new_event(&b));
            ev_ag.push_back(a);
            ev_ag.push_back(b);
            SCS_HIP_CHECK(hipEventRecord(a, s));
        }
        SCS_TRY(scs_comm_allgather_f64(&ctx->comm, send, recvb, count, s));
        if (time_ag) SCS_HIP_CHECK(hipEventRecord(b, s));
        ++n_allgather;
        return SCS_OK;
    }

    int last_nseg = 1;  // column segments of the most recent k_symm launch

    // symmetric schedule (k_symm_tri): the whole matrix on this device, streamed by upper tiles;
    // or (SCS_BUILD_UPPER graphs, `part`) this rank's tiles of the job's upper triangle: its
    // product is then PARTIAL -- all V rows, to be added to the other ranks' in rank order
    bool tri = false, part_mode = false;
    int tri_ct = 2, tri_nct = 0, tri_ntiles = 0;
    int tri_rb_lo = 0, tri_rb_hi = 0x7FFFFFFF;  // this rank's row blocks (of TRI_TH rows)
    // The tile list is stored twice, forwards and backwards, and consecutive applications
    // alternate: the tiles an application streamed last are the ones the next one starts with,
    // so whatever part of W the 256 MiB Infinity Cache still holds is read there and not from
    // HBM (a cyclic sweep of more than the cache's size would find nothing).  Every tile writes
    // its own slabs of the partial sums: the order of the tiles does not touch the result.
    bool tri_backwards = false;
    dbuf tri_tiles, tri_pdir, tri_ptr, ysend;
    std::vector<int2> tiles_host;  // source of the asynchronous upload of the tile lists: lives as long as the solve
    // the image is streamed in 128 x 512 tiles (2 KB pieces of a row, as W's 256 doubles): its own tile list,
    // stored behind W's in tri_tiles; the partial-sum slabs are W's (fewer column tiles: a prefix)
    int tri32_nct = 0, tri32_ntiles = 0;
    double w32_bytes_per_apply = 0.0;
    int64_t ldz = 0;                 // leading dimension of the k-major operand z
    double w_bytes_per_apply = 0.0;  // bytes of W one application streams

    int launch_symm_tri(const double *zin, double *yout) {
        const int tw = tri_ct * 128;
        // global indices address the stored block: an SCS_BUILD_UPPER rank keeps rows from
        // row_begin and columns from col0 on; its transposed partials only need the slabs of
        // its own row blocks
        const double *w_eff = g->d_w - (int64_t)g->row_begin * g->ld - g->col0;
        double *ptr_eff = tri_ptr.d() - (int64_t)tri_rb_lo * n * b;
        // (tf1.armed: pass 1 of R's orthonormalisation in the first workgroups of the launch)
        const int n_tf = panel_blocks16();
        const int ntiles = use32 ? tri32_ntiles : tri_ntiles;
#define TRI_T(B_, CT_, RPW_, D_, WT_, W_)                                                            \
    if (tf1.armed)                                                                                   \
        k_symm_tri_tf<B_, CT_, RPW_, D_, WT_><<<ntiles + n_tf, 256, 0, s>>>(                         \
            W_, g->ld, n, zin, ldz, tile_list, tri_pdir.d(), ptr_eff, n_tf, q.d(), fold_u,           \
            part.d(), n_tf, tf1.drop_tol, fold_mask_r, fold_theta, tf1.report, tf1.seq, part2.d(),   \
            coef1.d());                                                                              \
    else                                                                                             \
        k_symm_tri<B_, CT_, RPW_, D_, WT_><<<ntiles, 256, 0, s>>>(W_, g->ld, n, zin, ldz,            \
                                                                      tile_list, tri_pdir.d(), ptr_eff)
#define TRI(B_, CT_, RPW_, D_) TRI_T(B_, CT_, RPW_, D_, double, w_eff)
        const int2 *tile_list = (const int2 *)tri_tiles.p + (use32 ? 2 * tri_ntiles : 0) + (tri_backwards ? ntiles : 0);
        tri_backwards = !tri_backwards;
        if (use32) {
            // (b = 4, 128 x 512 tiles: 8 % faster than 256-column ones, tools/symm_tri_bench.hip)
            TRI_T(4, 2, 2, 3, float, g->d_w32);
            ++n_apply32;
        } else if (b == 4) {
            if (tri_ct == 4) TRI(4, 4, 2, 3);
            else if (tri_ct == 1) TRI(4, 1, 4, 4);
            else TRI(4, 2, 4, 3);
        } else {
            if (tri_ct == 1) TRI(8, 1, 2, 6);
            else TRI(8, 2, 2, 4);
        }
#undef TRI
#undef TRI_T
        SCS_HIP_CHECK(hipGetLastError());
        tf1.armed = false;
        const bool img_tiles = use32;
        if (part_mode) {
            // this rank's partial product, unscaled, all V rows: gathered and added by the caller
            k_symm_tri_finish<<<(4 * n * b + 255) / 256, 256, 0, s>>>(tri_pdir.d(), ptr_eff, n, b, tw, tri_nct,
                                                                  nullptr, ysend.d(), tri_rb_lo, tri_rb_hi);
            SCS_HIP_CHECK(hipGetLastError());
            SCS_TRY(gather(ysend.d(), recv.d(), (size_t)n * b));
            if (yout) {
                k_sum_parts<<<(n * b + 255) / 256, 256, 0, s>>>(recv.d(), world, n, b, g->d_dinv, yout);
                SCS_HIP_CHECK(hipGetLastError());
            }
            last_nseg = world;
            return SCS_OK;
        }
        // one segment: scaled into yout, or unscaled into ypart for k_gram_qaq to fold in
        k_symm_tri_finish<<<(4 * n * b + 255) / 256, 256, 0, s>>>(tri_pdir.d(), tri_ptr.d(), n, b, img_tiles ? 512 : tw,
                                                              img_tiles ? tri32_nct : tri_nct,
                                                              yout ? g->d_dinv : nullptr,
                                                              yout ? yout : ypart.d());
        SCS_HIP_CHECK(hipGetLastError());
        last_nseg = 1;
        return SCS_OK;
    }

    // yout (rows x b) = dinv (.) (W_local * Z), Z given k-major in zin (b x ld);
    // yout == null leaves the column segments in ypart for the caller to combine
    int launch_symm(const double *zin, double *yout) {
        if (g->mf) {
            // matrix-free graph: one unscaled segment into ypart, as k_symm leaves its column segments
            SCS_TRY(scs_matfree_apply(ctx, g, zin, ldz, b, ypart.d(), s));
            last_nseg = 1;
            if (yout)
                k_symm_finish<<<(rows * b + 255) / 256, 256, 0, s>>>(ypart.d(), 1, rows, b, g->d_dinv,
                                                                     g->row_begin, yout);
            SCS_HIP_CHECK(hipGetLastError());
            return SCS_OK;
        }
        if (tri) return launch_symm_tri(zin, yout);
        const int64_t ld = g->ld;
        int rpw = 4, sdepth = 2;
        if (b == 16) rpw = 2;
        if (b == 4) sdepth = 4;
        const int rowblocks = (rows + 4 * rpw - 1) / (4 * rpw);
        const int n_macros = (int)(ld / (sdepth * SYMM_SUB));
        int nseg = (1024 + rowblocks - 1) / rowblocks;
        nseg = std::max(1, std::min(std::min(nseg, 4), n_macros));
        if (b == 8 && nseg < 2 && n_macros >= 2 && rowblocks < 2048) nseg = 2;
        const int mps = (n_macros + nseg - 1) / nseg;
        nseg = (n_macros + mps - 1) / mps;
        if (ypart_cap < (size_t)nseg * rows * b) {
            scs_set_error("internal: ypart buffer too small");
            return SCS_EINVAL;
        }
        dim3 grid((unsigned)rowblocks, (unsigned)nseg);
        switch (b) {
            case 4:
                if (use32) {
                    ++n_apply32;
                    k_symm<4, 4, 4, 3, float><<<grid, 256, 0, s>>>(g->d_w32, ld, rows, zin, ypart.d(), mps);
                } else {
                    k_symm<4, 4, 4, 3><<<grid, 256, 0, s>>>(g->d_w, ld, rows, zin, ypart.d(), mps);
                }
                break;
            case 8:
                k_symm<8, 4, 2, 2><<<grid, 256, 0, s>>>(g->d_w, ld, rows, zin, ypart.d(), mps);
                break;
            case 12:
                k_symm<12, 4, 2, 1><<<grid, 256, 0, s>>>(g->d_w, ld, rows, zin, ypart.d(), mps);
                break;
            case 16:
                k_symm<16, 2, 2, 2><<<grid, 256, 0, s>>>(g->d_w, ld, rows, zin, ypart.d(), mps);
                break;
            default:
                scs_set_error("unsupported block width %d (need 4, 8, 12 or 16)", b);
                return SCS_EUNSUP;
        }
        SCS_HIP_CHECK(hipGetLastError());
        last_nseg = nseg;
        if (yout)
            k_symm_finish<<<(rows * b + 255) / 256, 256, 0, s>>>(ypart.d(), nseg, rows, b,
                                                                 g->d_dinv, g->row_begin, yout);
        return SCS_OK;
    }

    int alloc_symm_buffers() {
        ypart_cap = (size_t)4 * rows * b;
        SCS_TRY(ypart.alloc(ypart_cap * 8));
        ldz = g->upper ? scs_round_up(n, SCS_LD_ALIGN) : g->ld;
        SCS_TRY(z.alloc((size_t)b * ldz * 8));
        SCS_HIP_CHECK(hipMemsetAsync(z.p, 0, (size_t)b * ldz * 8, s));
        w_bytes_per_apply = 8.0 * rows * (double)n;
        w32_bytes_per_apply = 4.0 * rows * (double)n;  // (k_symm on the image of a rank's rows; the symmetric schedule sets its own)
        if (g->mf)  // both sweeps read the leaf arrays (16 bytes a leaf); the slabs are written and read once
            w_bytes_per_apply = 2.0 * 16.0 * (double)g->mf->tb->n_leaves +
                                2.0 * 2.0 * 8.0 * (double)g->mf->tb->n_trees * (double)n * b;
        if (g->upper) {
            // the job's upper triangle, this rank's row blocks: TW = 256 (the diagonal tile of a
            // row block then starts where the build's stored cells of those rows start)
            if (b != 4 && b != 8) {
                scs_set_error("an SCS_BUILD_UPPER graph is solved with block width 4 or 8 (asked: %d)", b);
                return SCS_EUNSUP;
            }
            tri = true;
            part_mode = true;
            tri_ct = 2;
            const int tw = 256;
            tri_nct = (n + tw - 1) / tw;
            tri_rb_lo = g->row_begin / TRI_TH;
            tri_rb_hi = (g->row_end + TRI_TH - 1) / TRI_TH;
            std::vector<int2> tiles;
            for (int i = tri_rb_lo; i < tri_rb_hi; ++i)
                for (int j = i * TRI_TH / tw; j < tri_nct; ++j) tiles.push_back(make_int2(i, j));
            tri_ntiles = (int)tiles.size();
            tiles.insert(tiles.end(), tiles.rbegin(), tiles.rend());  // and backwards
            SCS_TRY(tri_tiles.alloc(std::max<size_t>(tiles.size(), 1) * sizeof(int2)));
            SCS_HIP_CHECK(hipMemcpyAsync(tri_tiles.p, tiles.data(), tiles.size() * sizeof(int2),
                                         hipMemcpyHostToDevice, s));
            SCS_HIP_CHECK(hipStreamSynchronize(s));  // `tiles` goes out of scope
            SCS_TRY(tri_pdir.alloc((size_t)tri_nct * n * b * 8));
            SCS_TRY(tri_ptr.alloc((size_t)(tri_rb_hi - tri_rb_lo) * n * b * 8));
            SCS_TRY(ysend.alloc((size_t)n * b * 8));
            if (!recv.p) SCS_TRY(recv.alloc((size_t)n * b * world * 8));
            w_bytes_per_apply = 8.0 * (double)tri_ntiles * TRI_TH * tw;
            return SCS_OK;
        }
        // W is symmetric: with all of it on this device only the tiles on and above the
        // diagonal need streaming (small matrices keep k_symm, whose column segments fill the
        // chip better).
        tri = !g->mf && world == 1 && rows == n && g->row_begin == 0 && n >= 4096 && (b == 4 || b == 8);
        if (tri) {
            const int tw = tri_ct * 128;
            const int n_rb = (n + TRI_TH - 1) / TRI_TH;
            tri_nct = (n + tw - 1) / tw;
            std::vector<int2> &tiles = tiles_host;
            tiles.clear();
            for (int i = 0; i < n_rb; ++i)
                for (int j = i * TRI_TH / tw; j < tri_nct; ++j) tiles.push_back(make_int2(i, j));
            tri_ntiles = (int)tiles.size();
            tiles.insert(tiles.end(), tiles.rbegin(), tiles.rend());  // and backwards
            {
                // the image's 128 x 512 tiles, behind W's list
                std::vector<int2> t32;
                tri32_nct = (n + 511) / 512;
                for (int i = 0; i < n_rb; ++i)
                    for (int j = i * TRI_TH / 512; j < tri32_nct; ++j) t32.push_back(make_int2(i, j));
                tri32_ntiles = (int)t32.size();
                tiles.insert(tiles.end(), t32.begin(), t32.end());
                tiles.insert(tiles.end(), t32.rbegin(), t32.rend());
                w32_bytes_per_apply = 4.0 * (double)tri32_ntiles * TRI_TH * 512;
            }
            SCS_TRY(tri_tiles.alloc(tiles.size() * sizeof(int2)));
            // (no wait here: the degree pass is still streaming W, and the list's source outlives the solve)
            SCS_HIP_CHECK(hipMemcpyAsync(tri_tiles.p, tiles.data(), tiles.size() * sizeof(int2),
                                         hipMemcpyHostToDevice, s));
            SCS_TRY(tri_pdir.alloc((size_t)std::max(tri_nct, tri32_nct) * n * b * 8));
            SCS_TRY(tri_ptr.alloc((size_t)n_rb * n * b * 8));
            w_bytes_per_apply = 8.0 * (double)tri_ntiles * TRI_TH * tw;
        }
        return SCS_OK;
    }

    // one application, counted; `timed`: between an event pair of its own (kept in `ev`, read by the statistics)
    int timed_symm(bool timed, const double *zin, double *yout) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timed) {
            SCS_TRY(new_event(&e0));
            SCS_TRY(new_event(&e1));
            ev.push_back(e0);
            ev.push_back(e1);
            ev32.push_back(use32 ? 1 : 0);
            SCS_HIP_CHECK(hipEventRecord(e0, s));
        }
        SCS_TRY(launch_symm(zin, yout));
        if (timed) SCS_HIP_CHECK(hipEventRecord(e1, s));
        ++n_apply;
        return SCS_OK;
    }

    // dst_panel[:, c0:c0+b] = S * src_panel[:, c0s:c0s+b]   (panels have ld 3b)
    int apply(const double *src, int c0s, double *dst, int c0d) {
        const int nb = n * b;
        k_scale_rows<<<(nb + 255) / 256, 256, 0, s>>>(src, 3 * b, c0s, b, n, g->d_dinv, z.d(),
                                                      ldz);
        SCS_TRY(timed_symm(true, z.d(), yloc.d()));
        const double *yf = yloc.d();
        if (part_mode) {
            // (launch_symm_tri gathered the ranks' partial products and yloc holds their scaled
            // sum for all V rows)
        } else if (world > 1) {
            SCS_TRY(gather(yloc.d(), recv.d(), (size_t)chunk));
            k_unpack<<<(nb + 255) / 256, 256, 0, s>>>(recv.d(), chunk, b,
                                                      (const int32_t *)splits_d.p, world, n,
                                                      yfull.d());
            yf = yfull.d();
        }
        k_store_cols<<<(nb + 255) / 256, 256, 0, s>>>(yf, b, n, dst, 3 * b, c0d);
        return SCS_OK;
    }

    // out (ka x kb, device) = A^T B
    int gram(const double *a, int lda, int ka, const double *bm, int ldb, int kb, double *out,
             bool mfma) {
        const int nout = ka * kb;
        int nparts;
        if (mfma && ka <= 48 && kb <= 48) {
            nparts = std::min(gram_blocks, std::max(1, (n + 3) / 4));
            const int ta = (ka + 15) / 16, tb = (kb + 15) / 16;
#define GM(TA, TB)                                                                               \
    if (ta == TA && tb == TB)                                                                    \
        k_gram_mfma<TA, TB><<<nparts, 64, 0, s>>>(a, lda, ka, bm, ldb, kb, n, part.d());
            GM(1, 1) GM(1, 2) GM(1, 3) GM(2, 1) GM(2, 2) GM(2, 3) GM(3, 1) GM(3, 2) GM(3, 3)
#undef GM
        } else {
            nparts = std::min(gram_blocks, std::max(1, (n + GRAM_CH - 1) / GRAM_CH));
            k_gram<<<nparts, 256, 0, s>>>(a, lda, ka, bm, ldb, kb, n, part.d());
        }
        k_reduce_partials<<<(nout + 3) / 4, 256, 0, s>>>(part.d(), nparts, nout, out);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    int update(double *y, int ldy, int kc, double alpha, const double *a, int lda, int ka,
               const double *c, int ldc, double sign) {
        k_update<<<(n + 15) / 16, 256, 0, s>>>(y, ldy, kc, alpha, a, lda, ka, c, ldc, sign, n);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    // Y <- Y C and Y2 <- Y2 C (both n x kc blocks of panels with leading dimension ld) in one launch
    int rotate2(double *y, double *y2, int ld, int kc, const double *c, int ldc) {
        k_update<<<dim3((n + 15) / 16, 2), 256, 0, s>>>(y, ld, kc, 0.0, y, ld, kc, c, ldc, 1.0, n, y2, y2);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    // ---- fused iteration (scs_panel.h), block widths 4 and 8 ----
    static int panel_cap() {
        static const int cap = PANEL_BLOCKS_MAX;
        return cap;
    }
    int panel_blocks16() const { return std::max(1, std::min(panel_cap(), ((n + 15) / 16 + 3) / 4)); }
    int panel_blocks4() const { return std::max(1, std::min(panel_cap(), ((n + 3) / 4 + 3) / 4)); }

    template <int B>
    int fused_front(const double *uvec, const double *c, const double *d, const double *theta,
                    double *coef, int *mask_r, double drop_tol, double *report, double seq) {
        const int nb = panel_blocks16();
        k_panel_rr<B><<<nb, 256, 0, s>>>(q.d(), aq.d(), uvec, c, d, theta, n, part.d());
        k_small_orth<<<1, 256, 0, s>>>(part.d(), nb, B, drop_tol, coef, mask_r, theta, report, seq);
        k_panel_tf<B, true, false><<<nb, 256, 0, s>>>(q.d(), uvec, coef, n, part.d(), nullptr,
                                                      nullptr, 0);
        k_small_orth<<<1, 256, 0, s>>>(part.d(), nb, B, 0.0, coef, mask_r, theta, nullptr, 0.0);
        k_panel_tf<B, false, true><<<nb, 256, 0, s>>>(q.d(), uvec, coef, n, nullptr, g->d_dinv,
                                                      z.d(), ldz);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    // The same front with the small solves inside the tall kernels (k_panel_rr_solve,
    // k_panel_tf_solve): three launches instead of five, and the Rayleigh-Ritz kernel that used
    // to close the iteration is the head of the next one's first launch.  `solve` = 0: X stays
    // and the search directions are cleared (first iteration, after a refresh).
    template <int B>
    int fused_front_solve(const double *uvec, int nparts_in, int solve, double *theta,
                          const int *maskp_in, int *mask_r, int *maskp_out, double drop_tol,
                          double *report, double seq) {
        const int nb = panel_blocks16();
        if (overlap_pass1) {
            // the Rayleigh-Ritz kernel hands the SYMM the scaled RAW residual block; pass 1 is armed for
            // the SYMM launch of fused_back.  (One-sided Gram entries, exact_from = B, in this loop always:
            // S R is composed from S applied to the raw block and the products of what pass 1 projects out,
            // a difference of terms up to 1e6 times its size when a column's residual lies almost inside
            // [X P] -- its rounding is then what the image's is, small_rr_body.  Found by
            // tools/fuzz_mixed_precision.py: with the mean of both entries the all-double loop left a
            // converged column's noise grow until the block blew up, graphs with isolated vertices.)
            k_panel_rr_solve<B><<<nb, 256, 0, s>>>(q.d(), aq.d(), uvec, part3.d(), nparts_in, solve, theta,
                                                   maskp_in, mask_r, maskp_out, drop_tol, n, part.d(),
                                                   g->d_dinv, z.d(), ldz, B);
            SCS_HIP_CHECK(hipGetLastError());
            tf1.armed = true;
            tf1.drop_tol = drop_tol;
            tf1.report = report;
            tf1.seq = seq;
            return SCS_OK;
        }
        if (fold_pass2) {
            // round 5: pass 1 writes Z; pass 2 rides the Gram kernel behind the SYMM stream (fused_back)
            k_panel_rr_solve<B><<<nb, 256, 0, s>>>(q.d(), aq.d(), uvec, part3.d(), nparts_in, solve, theta,
                                                   maskp_in, mask_r, maskp_out, drop_tol, n, part.d(), nullptr,
                                                   nullptr, 0, gram_from32 ? B : -1);
            k_panel_tf_solve<B, true, true><<<nb, 256, 0, s>>>(q.d(), uvec, part.d(), nb, drop_tol, mask_r,
                                                               theta, report, seq, n, part2.d(), g->d_dinv,
                                                               z.d(), ldz);
            SCS_HIP_CHECK(hipGetLastError());
            return SCS_OK;
        }
        k_panel_rr_solve<B><<<nb, 256, 0, s>>>(q.d(), aq.d(), uvec, part2.d(), nparts_in, solve, theta,
                                               maskp_in, mask_r, maskp_out, drop_tol, n, part.d(), nullptr,
                                               nullptr, 0, gram_from32 ? B : -1);
        k_panel_tf_solve<B, true, false><<<nb, 256, 0, s>>>(q.d(), uvec, part.d(), nb, drop_tol, mask_r,
                                                            theta, report, seq, n, part2.d(), nullptr,
                                                            nullptr, 0);
        k_panel_tf_solve<B, false, true><<<nb, 256, 0, s>>>(q.d(), uvec, part2.d(), nb, 0.0, mask_r, theta,
                                                            nullptr, 0.0, n, nullptr, g->d_dinv, z.d(),
                                                            ldz);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    // AR = S R (R's scaled transpose already sits in z) into AQ's R slot, then the
    // partials of Q^T AQ (into pout); returns their count.
    // (Folding k_symm_tri_finish into k_gram_qaq -- every lane of the Gram kernel sums the ~60
    // tile partials of one AR entry, same order, same bits, 32 loads in flight -- was measured:
    // 25.1 us against 7.7 + 7.8 for the two launches: 128 workgroups cannot hide the latency of
    // that many dependent rounds of loads; the finish kernel spreads them over 625.)
    template <int B>
    int fused_back(int *nparts, double *pout) {
        // k_symm is timed with HIP events on every fourth launch only: recording an event costs
        // the device a ~6 us bubble
        const bool timed = (n_apply & 3) == 0;
        time_ag = timed && world > 1;
        gram_from32 = use32;
        const int nb = fold_pass2 ? panel_blocks16() : panel_blocks4();
        const int nb16 = panel_blocks16();  // partials of pass 1's Gram products (k_panel_tf_solve)
        *nparts = nb;
        // What the Gram kernel sums into AQ's R slot (its FINISH), scaling as it goes:
        //   3  the ranks' gathered partial products (world x V x b), added in rank order (launch_symm_tri gathers);
        //   1  this device's column segments, left unscaled in ypart;
        //   2  the ranks' gathered slices, scaled by launch_symm, placed by `chunk` and the row splits.
        const int finish = part_mode ? 3 : (world == 1 ? 1 : 2);
        SCS_TRY(timed_symm(timed, z.d(), finish == 2 ? yloc.d() : nullptr));
        if (finish == 2) SCS_TRY(gather(yloc.d(), recv.d(), (size_t)chunk));
        const double *seg = finish == 1 ? ypart.d() : recv.d();
        const int nseg = finish == 1 ? last_nseg : world;
        const int64_t ch = finish == 2 ? chunk : 0;
        const int32_t *sp = finish == 2 ? (const int32_t *)splits_d.p : nullptr;
        // (overlap_pass1 is a one-device loop: FINISH 1)
#define GRAM_BACK(F_)                                                                                             \
    if (fold_pass2)                                                                                               \
        k_panel_gram_tf_solve<B, F_><<<nb, 256, 0, s>>>(q.d(), aq.d(), fold_u, part2.d(), nb16, fold_mask_r,      \
                                                        fold_theta, n, seg, nseg, g->d_dinv, pout, ch, sp,        \
                                                        overlap_pass1 ? coef1.d() : nullptr);                     \
    else                                                                                                          \
        k_gram_qaq<B, F_><<<nb, 256, 0, s>>>(q.d(), aq.d(), n, seg, nseg, g->d_dinv, pout, ch, sp)
        if (finish == 3) {
            GRAM_BACK(3);
        } else if (finish == 1) {
            GRAM_BACK(1);
        } else {
            GRAM_BACK(2);
        }
#undef GRAM_BACK
        time_ag = false;
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }
};

// layout of the small-matrix scratch (doubles)
constexpr int SM_G = 0;                         // up to 48 x 48
constexpr int SM_T = SM_G + 48 * 48;            // svqb transform (<= 16 x 16) / rr coeffs (48 x 16)
constexpr int SM_C = SM_T + 48 * 16;            // projection coefficients (<= 32 x 16)
constexpr int SM_D = SM_C + 48 * 16;            // search-direction coefficients (48 x 16)
constexpr int SM_THETA = SM_D + 48 * 16;        // theta[0..b], padded
constexpr int SM_RN = SM_THETA + 32;            // residual norms^2 [b]
constexpr int SM_MASK = SM_RN + 32;             // int mask[48] (as 24 doubles)
constexpr int SM_TOTAL = SM_MASK + 32;

void sign_flip_and_store(const std::vector<double> &col0, const std::vector<double> &col1, int n,
                         double *maps) {
    // reference: sklearn/utils/extmath.py _deterministic_vector_sign_flip
    for (int c = 0; c < 2; ++c) {
        const std::vector<double> &v = c == 0 ? col0 : col1;
        int arg = 0;
        double best = -1.0;
        for (int i = 0; i < n; ++i)
            if (std::fabs(v[i]) > best) {
                best = std::fabs(v[i]);
                arg = i;
            }
        const double sg = v[arg] < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) maps[(size_t)i * 2 + c] = sg * v[i];
    }
}

// the two readings of a probe switch (scs_dbg: unset unless SCS_DEBUG=1 at load)
bool dbg_on(const char *name) {  // off unless set to non-zero
    const char *e = scs_dbg(name);
    return e && atoi(e);
}
bool dbg_not_off(const char *name) {  // on unless set to 0
    const char *e = scs_dbg(name);
    return !(e && !atoi(e));
}

// Every switch of a solve, read once (scs_fiedler makes one plan per call), and what follows from them.  The image decision
// (made before the width is chosen) and the loop (set up after it) ask the same plan: a loop that was not built
// for the image cannot be handed it.
struct loop_plan {
    // ---- mixed precision (round 5; SCS_LOWP=0 off, 1, 2 = default).  The loop applies the operator to
    // its SEARCH DIRECTIONS only (S X and S P are carried by linear updates), and a search direction does
    // not need S to sixteen digits: with the symmetric schedule at width 4 the SYMM streams a single-
    // precision image of W -- half the bytes, products and sums still in double precision -- that the
    // degree pass writes on its way through W.  What the image's rounding leaves in S X and S P is removed
    // by renewing both through W itself (two applications) when the residual passes 1e-8, and
    // once more should it stop halving; mode 1 goes on in double precision after the first renewal, mode 2
    // stays with the image.  The confirmation at the end always applies W, and a solve it sends back into the loop
    // continues without the image.
    const int lowp_mode = getenv("SCS_LOWP") ? atoi(getenv("SCS_LOWP")) : 2;
    // (an image above SCS_LOWP_MAX_BYTES, default 16 GiB -- about 65 000 vertices -- is not made: what it
    // saves a solve of that size, some 80 ms, is less than what an allocation of tens of GB can cost)
    const double lowp_max_bytes = getenv("SCS_LOWP_MAX_BYTES") ? atof(getenv("SCS_LOWP_MAX_BYTES")) : 16.0 * (1u << 30);
    // SCS_LEGACY_LOOP=1: the one-kernel-per-step formulation at widths 4 and 8 too
    const bool legacy_loop = dbg_on("SCS_LEGACY_LOOP");
    // SCS_SPLIT_SMALL=1: the small solves as one-workgroup kernels of their own (the round-3 loop)
    const bool split_small = dbg_on("SCS_SPLIT_SMALL");
    const bool fold_pass2_on = dbg_not_off("SCS_FOLD_PASS2"), overlap_pass1_on = dbg_not_off("SCS_OVERLAP_PASS1");
    const bool use_mfma = !dbg_on("SCS_NO_MFMA");

    // Fused iteration (scs_panel.h) for the default block widths; the unfused loop is the only one for widths 12 and 16.
    bool fused(int b) const { return (b == 4 || b == 8) && !legacy_loop; }
    // round 5: the second orthonormalisation pass of R rides the Gram kernel behind the SYMM stream.
    // (Only this, the default loop, hands its Rayleigh-Ritz solve the one-sided entries -- small_rr_body -- so
    // only it is given the image.)
    bool fold_pass2(int b) const { return fused(b) && !split_small && fold_pass2_on; }
    // ... and the first pass rides the SYMM launch itself (k_symm_tri_tf: one device, symmetric schedule)
    bool overlap_pass1(int b, bool tri, bool part_mode, int world) const {
        return fold_pass2(b) && tri && !part_mode && world == 1 && overlap_pass1_on;
    }
};

// The block width of a solve, and (want32) whether its loop will stream the image: the degree pass, begun
// right after, then writes it.
int choose_width(const scs_ctx *ctx, const scs_graph *g, int block, const loop_plan &plan, bool *want32) {
    const int n = g->n;
    // (round 6: a row-partitioned job -- whole rows on every rank, k_symm -- keeps the image of each rank's rows:
    // the first real multi-GPU run streams per rank what the one-GPU run streams, not twice that)
    const bool image_ok = solver::image_layout(ctx, g, 4) && plan.lowp_mode > 0 && plan.fold_pass2(4) &&
                          (g->have_w32 ||
                           4.0 * (double)(g->row_end - g->row_begin) * (double)g->ld <= plan.lowp_max_bytes);
    // default width: 4 while the panel kernels and the 3b x 3b Rayleigh-Ritz solve weigh
    // against the SYMM stream, 8 once streaming W dominates (measured crossover ~ 16k) -- unless the
    // loop can stream the single-precision image, which exists at width 4: half the bytes an
    // application outweigh the iterations width 8 saves (configs[3], 50 000 vertices: 48 iterations and
    // 78 ms against 35 and 101)
    int b = block ? block : ((n >= 16384 && !image_ok) ? 8 : 4);
    if (g->upper && b > 8) b = 8;  // the symmetric SYMM kernel comes in widths 4 and 8
    if (g->mf) b = std::min(b <= 4 ? 4 : 8, g->mf->b_cap);  // (the sweep kernel likewise)
    {
        const int allowed[] = {16, 12, 8, 4};
        const int cap = (n - 2) / 3;  // 3b basis vectors + the constraint must fit in V
        int pick = 4;
        for (int a : allowed)
            if (a <= b && a <= cap) {
                pick = a;
                break;
            }
        b = pick;  // (>= 4: more than the one or two pairs wanted)
    }
    *want32 = image_ok && b == 4;
    return b;
}

// One LOBPCG solve: the solver's buffers and launches, the loop's pointers into them and what the host keeps
// between iterations.  scs_fiedler drives it step by step; every step only enqueues, unless it says that it waits.
struct lobpcg {
    scs_ctx *const ctx;
    scs_graph *const g;
    const hipStream_t s;
    const int n, b, q3;
    const loop_plan &plan;
    const bool fused;
    solver sv;
    scs_loop_policy policy;  // the stop / renew / confirm rules (scs_policy.h)
    static constexpr double drop_tol = 1e-13;
    // panel layout [X | P | R]: the blocks R is projected against are contiguous
    double *Q = nullptr, *AQ = nullptr, *X = nullptr, *R = nullptr, *AX = nullptr;
    double *G = nullptr, *T = nullptr, *C = nullptr, *D = nullptr, *TH = nullptr, *RN = nullptr;
    int *MASK = nullptr;
    bool constrained = false;
    int want = 0;
    const double *uvec = nullptr;
    dbuf x0d, res_part;
    int res_blocks = 0;
    std::vector<double> h_rn, h_th;  // the residual norms^2 and Ritz values of the block the host last saw
    double final_res[2] = {0.0, 0.0};
    // fused loop: where the Gram partials go, and what the next iteration's opening Rayleigh-Ritz solve is told
    double *qaq_out = nullptr;
    int rr_solve = 0, rr_parts = 0, mpar = 0;
    int *maskp[2] = {nullptr, nullptr};

    lobpcg(scs_ctx *ctx_, scs_graph *g_, int b_, const loop_plan &plan_)
        : ctx(ctx_), g(g_), s(ctx_->stream), n(g_->n), b(b_), q3(3 * b_), plan(plan_), fused(plan_.fused(b_)) {}

    // the solver and every buffer of the loop but three small ones of `start`; ends by WAITING for the degrees
    int setup(double tol, bool want32) {
        sv.bind(ctx, n, b, g);
        sv.use_mfma = plan.use_mfma;
        SCS_TRY(sv.team_splits());
        SCS_TRY(sv.q.alloc((size_t)n * q3 * 8));
        SCS_TRY(sv.aq.alloc((size_t)n * q3 * 8));
        SCS_TRY(sv.alloc_symm_buffers());
        SCS_TRY(sv.yloc.alloc((size_t)sv.chunk * 8));
        SCS_TRY(sv.u.alloc((size_t)n * 8));
        SCS_TRY(sv.part.alloc((size_t)1024 * q3 * q3 * 8));
        SCS_TRY(sv.part2.alloc((size_t)1024 * q3 * q3 * 8));
        SCS_TRY(sv.part3.alloc((size_t)1024 * q3 * q3 * 8));
        SCS_TRY(sv.small.alloc((size_t)SM_TOTAL * 8));
        SCS_TRY(sv.team_buffers());
        SCS_HIP_CHECK(hipMemsetAsync(sv.q.p, 0, (size_t)n * q3 * 8, s));
        SCS_HIP_CHECK(hipMemsetAsync(sv.aq.p, 0, (size_t)n * q3 * 8, s));
        SCS_HIP_CHECK(hipMemsetAsync(sv.yloc.p, 0, (size_t)sv.chunk * 8, s));
        SCS_HIP_CHECK(hipMemsetAsync(sv.small.p, 0, (size_t)SM_TOTAL * 8, s));
        sv.fold_pass2 = plan.fold_pass2(b);
        sv.overlap_pass1 = plan.overlap_pass1(b, sv.tri, sv.part_mode, sv.world);

        Q = sv.q.d(), AQ = sv.aq.d();
        X = Q, R = Q + 2 * b;
        AX = AQ;
        G = sv.small_at(SM_G), T = sv.small_at(SM_T), C = sv.small_at(SM_C);
        D = sv.small_at(SM_D);
        TH = sv.small_at(SM_THETA), RN = sv.small_at(SM_RN);
        MASK = (int *)sv.small_at(SM_MASK);
        h_rn.resize(b);
        h_th.resize(b + 1);

        SCS_TRY(scs_graph_prepare_degrees(ctx, g));  // (begun by the caller: the degrees are needed from here on)
        sv.use32 = want32 && g->have_w32;
        policy.tol = tol;
        policy.lowp_mode = plan.lowp_mode;
        policy.lowp_tol = 1e-8;
        policy.lowp_tol2 = 0.0;
        policy.lowp_state = sv.use32 ? 1 : 0;  // image in use: 1 + the renewals of S X / S P made so far; 0: off
        constrained = g->n_isolated == 0;
        want = constrained ? 1 : 2;
        return SCS_OK;
    }

    // project the constraint out of a panel block (`passes` times)
    int project_u(double *Y, int passes) {
        if (!constrained) return SCS_OK;
        for (int pass = 0; pass < passes; ++pass) {
            SCS_TRY(sv.gram(sv.u.d(), 1, 1, Y, q3, b, C, false));
            SCS_TRY(sv.update(Y, q3, b, 1.0, sv.u.d(), 1, 1, C, b, -1.0));
        }
        return SCS_OK;
    }
    // SVQB-orthonormalise a panel block; the companion AY (may be null) receives the same column transform.
    // mask handling: pass 2 would overwrite mask with all-live for surviving columns and 0
    // for dead ones (their Gram diagonal is 0 -> dsc 0 -> eigenvalue 0 -> dropped since
    // 0 > 0 is false), so the mask of the second pass is the final one.
    int svqb(double *Y, double *AY, int *mask_out) {
        for (int pass = 0; pass < 2; ++pass) {
            SCS_TRY(sv.gram(Y, q3, b, Y, q3, b, G, sv.use_mfma));
            k_small_svqb<<<1, 256, 0, s>>>(G, b, pass == 0 ? drop_tol : 0.0, T, mask_out);
            // second pass: every surviving direction is kept (dead columns stay dead: dsc = 0)
            SCS_TRY(sv.update(Y, q3, b, 0.0, Y, q3, b, T, b, 1.0));
            if (AY) SCS_TRY(sv.update(AY, q3, b, 0.0, AY, q3, b, T, b, 1.0));
        }
        return SCS_OK;
    }
    // rotate X so that X^T A X is diagonal
    // (masks: all live going in, no search directions coming out -- set by the kernel itself, which leaves the
    // P slots dead; X and S X rotated in one launch)
    int rotate_x() {
        SCS_TRY(sv.gram(X, q3, b, AX, q3, b, G, sv.use_mfma));
        k_small_rr_start<<<1, 256, 0, s>>>(G, b, MASK, T, D, TH, drop_tol);
        return sv.rotate2(X, AX, q3, b, T, b);
    }

    // the start block: constraint vector, init, projection, SVQB, first application, the rotating Rayleigh-Ritz
    int start(const double *x_init) {
        if (x_init) {
            SCS_TRY(x0d.alloc((size_t)n * 8));
            SCS_HIP_CHECK(hipMemcpyAsync(x0d.p, x_init, (size_t)n * 8, hipMemcpyHostToDevice, s));
        }
        if (constrained)
            k_trivial<<<(n + 255) / 256, 256, 0, s>>>(g->d_deg, 1.0 / g->dd_norm, n, sv.u.d());
        k_init_block<<<(n * b + 255) / 256, 256, 0, s>>>(Q, b, n, x_init ? x0d.d() : nullptr);
        SCS_TRY(project_u(X, 2));
        SCS_TRY(svqb(X, nullptr, MASK));
        SCS_TRY(sv.apply(Q, 0, AQ, 0));
        SCS_TRY(rotate_x());

        res_blocks = (n + 255) / 256;
        SCS_TRY(res_part.alloc((size_t)res_blocks * b * 8));
        if (fused) {
            if (!ctx->h_report) {
                SCS_HIP_CHECK(hipHostMalloc((void **)&ctx->h_report, 64 * sizeof(double),
                                            hipHostMallocMapped | hipHostMallocCoherent));
                SCS_HIP_CHECK(hipHostGetDevicePointer((void **)&ctx->d_report, ctx->h_report, 0));
                memset(ctx->h_report, 0, 64 * sizeof(double));
            }
            k_unit_coeffs<<<(3 * b * b + 255) / 256, 256, 0, s>>>(T, D, b);
        }
        uvec = constrained ? sv.u.d() : nullptr;
        if (sv.overlap_pass1) SCS_TRY(sv.coef1.alloc((size_t)(3 * 8 + 4) * 8 * 8));
        sv.fold_u = uvec;
        sv.fold_mask_r = MASK + 2 * b;
        sv.fold_theta = TH;
        qaq_out = sv.fold_pass2 ? sv.part3.d() : sv.part2.d();
        maskp[0] = MASK + b;
        maskp[1] = MASK + 32;
        return SCS_OK;
    }

    template <int B>
    int enqueue_fused_b(double seq) {
        int nparts = 0;
        if (!plan.split_small) {
            // (the Rayleigh-Ritz solve on the previous iteration's Gram partials opens the
            // first launch)
            SCS_TRY(sv.fused_front_solve<B>(uvec, rr_parts, rr_solve, TH, maskp[mpar], MASK + 2 * b, maskp[mpar ^ 1],
                                            drop_tol, ctx->d_report, seq));
            SCS_TRY(sv.fused_back<B>(&nparts, qaq_out));
            rr_parts = nparts;
            rr_solve = 1;
            mpar ^= 1;
        } else {
            SCS_TRY(sv.fused_front<B>(uvec, T, D, TH, C, MASK + 2 * b, drop_tol, ctx->d_report, seq));
            SCS_TRY(sv.fused_back<B>(&nparts, sv.part.d()));
            k_small_rr<<<1, 256, 0, s>>>(sv.part.d(), nparts, q3, b, MASK, T, D, TH, MASK + b, drop_tol);
        }
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }
    // One fused iteration, all of it enqueued before the host looks at the residual norms the
    // first small kernel reports under `seq`: the device never waits for the host.  Nothing
    // after that kernel touches X, so on a stop X is the block the norms belong to.
    int enqueue_fused(double *seq) {
        *seq = (double)(++ctx->report_seq);
        return b == 4 ? enqueue_fused_b<4>(*seq) : enqueue_fused_b<8>(*seq);
    }

    // WAITS for the report of the iteration enqueued under `seq` (the device is already working on the rest
    // of the iteration) and takes its norms and Ritz values; gives up if the stream died
    int await_report(double seq, int iter) {
        volatile double *hr = (volatile double *)ctx->h_report;
        const auto t_wait = std::chrono::steady_clock::now();
        unsigned spins = 0;
        while (hr[40] != seq) {
            __builtin_ia32_pause();
            // (a report normally arrives within a few microseconds; a host thread that has
            // waited much longer lets others run -- eight ranks may share the cores)
            if (spins > (1u << 18) && (spins & 0x3FF) == 0) sched_yield();
            if ((++spins & 0xFFFF) == 0) {
                const hipError_t qe = hipStreamQuery(s);
                if (qe != hipSuccess && qe != hipErrorNotReady) {
                    scs_set_error("scs_fiedler: stream failed: %s", hipGetErrorString(qe));
                    return SCS_EHIP;
                }
                if (qe == hipSuccess && hr[40] != seq) {
                    // everything ran and the report never arrived
                    if (std::chrono::steady_clock::now() - t_wait > std::chrono::seconds(5)) {
                        scs_set_error("scs_fiedler: residual report lost at iteration %d", iter);
                        return SCS_EHIP;
                    }
                }
            }
        }
        for (int j = 0; j < b; ++j) h_rn[j] = hr[j];
        for (int j = 0; j <= b; ++j) h_th[j] = hr[16 + j];
        return SCS_OK;
    }

    // the residual block of X and its norms, read back (WAITS): an unfused iteration's front, and the confirmation's measurement
    int read_residual() {
        k_residual<<<res_blocks, 256, 0, s>>>(Q, AQ, b, TH, n, res_part.d());
        k_reduce_partials<<<(b + 3) / 4, 256, 0, s>>>(res_part.d(), res_blocks, b, RN);
        SCS_HIP_CHECK(hipMemcpyAsync(h_rn.data(), RN, (size_t)b * 8, hipMemcpyDeviceToHost, s));
        SCS_HIP_CHECK(hipMemcpyAsync(h_th.data(), TH, (size_t)(b + 1) * 8, hipMemcpyDeviceToHost, s));
        SCS_HIP_CHECK(hipStreamSynchronize(s));
        return SCS_OK;
    }
    // the worst residual of the wanted columns in h_rn; they are what the solve reports should it end here
    double worst_residual() {
        double worst = 0.0;
        for (int j = 0; j < want; ++j) worst = std::max(worst, std::sqrt(h_rn[j]));
        for (int j = 0; j < want; ++j) final_res[constrained ? 1 : j] = std::sqrt(h_rn[j]);
        return worst;
    }

    // the back of an unfused iteration: projection, SVQB, application, Rayleigh-Ritz
    int unfused_back() {
        // R <- orthonormal complement of [u, X, P] within span(R); P is orthonormal and
        // orthogonal to X by construction (k_small_rr), dead P columns are zero vectors
        // S u = u exactly, so R = S X - X theta inherits X's orthogonality to u; one
        // pass keeps rounding drift from accumulating
        SCS_TRY(project_u(R, 1));
        for (int pass = 0; pass < 2; ++pass) {
            SCS_TRY(sv.gram(Q, q3, 2 * b, R, q3, b, C, sv.use_mfma));
            SCS_TRY(sv.update(R, q3, b, 1.0, Q, q3, 2 * b, C, b, -1.0));
        }
        SCS_TRY(svqb(R, nullptr, MASK + 2 * b));
        SCS_TRY(sv.apply(Q, 2 * b, AQ, 2 * b));

        // Rayleigh-Ritz on the orthonormal basis [X P R]; new X and new P in one pass each
        SCS_TRY(sv.gram(Q, q3, q3, AQ, q3, q3, G, sv.use_mfma));
        k_small_rr<<<1, 256, 0, s>>>(G, 0, q3, b, MASK, T, D, TH, MASK + b, drop_tol);
        k_rr_update<<<(n + 15) / 16, 256, 0, s>>>(Q, b, q3, T, D, n);
        k_rr_update<<<(n + 15) / 16, 256, 0, s>>>(AQ, b, q3, T, D, n);
        SCS_HIP_CHECK(hipGetLastError());
        return SCS_OK;
    }

    // S X and S P anew through W itself, behind the iteration already enqueued (its Gram matrix,
    // formed with the old products, steers one more Rayleigh-Ritz step: coefficients only).
    // What the image adds to S X afterwards is its rounding (~1e-10 ||S||) times the steps still
    // to be taken, which are of the size of the residual over the spectral gap: one renewal clears
    // what the long early steps left (measured: without it 15 more iterations); a second one is
    // made when the residual stops halving (four iterations) (a second threshold on the residual itself exists and is off).
    // After the FIRST renewal a loop that has not halved its residual in eight iterations stops for the
    // confirmation (the image's rounding has become the floor); before it LOBPCG has plateaus of its own
    // -- ten iterations at 4e-5 on the `bootstrap` workload -- five orders above the image's rounding.
    int renew() {
        sv.use32 = false;
        SCS_TRY(sv.apply(Q, 0, AQ, 0));
        SCS_TRY(sv.apply(Q, b, AQ, b));
        sv.use32 = policy.image_in_use();
        return SCS_OK;
    }

    // The confirmation: the residual of X against a freshly applied operator (AX drifts by linear updates),
    // into *w2 (WAITS).  The search directions are dead afterwards: a loop that goes on calls restart_directions.
    int confirm(double tol, double *w2) {
        sv.use32 = false;  // the confirmation, and whatever follows it, through W
        SCS_TRY(sv.apply(Q, 0, AQ, 0));
        SCS_TRY(rotate_x());
        SCS_TRY(read_residual());
        *w2 = worst_residual();
        if (!(*w2 <= tol)) {
            // X is carried by linear updates and never normalised again: after hundreds of iterations
            // ||x||^2 = 1 + 2 eps, the Ritz value x^T S x is off by 2 eps lambda, and no residual
            // S x - theta x can fall below that error however good x is (the path on 257 vertices:
            // theta off by 2.4e-13 / 1.8e-13 / 7.3e-13 at widths 4 / 8 / 16, the residuals flat at
            // exactly those values).  So a confirmation that misses the target
            // orthonormalises X, takes the fresh S X through the same transform (no further
            // application) and measures once more.
            SCS_TRY(svqb(X, AX, MASK));
            SCS_TRY(rotate_x());
            SCS_TRY(read_residual());
            *w2 = worst_residual();
        }
        return SCS_OK;
    }
    int restart_directions() {
        if (fused) k_unit_coeffs<<<(3 * b * b + 255) / 256, 256, 0, s>>>(T, D, b);
        rr_solve = 0;
        return SCS_OK;
    }

    // the two wanted columns, scaled, from the device (not the whole panel), sign-fixed into maps_out, and the
    // Ritz values into st; records ev_b behind the solve's last copy and WAITS
    int extract(hipEvent_t ev_b, double *maps_out, scs_stats *st) {
        // what an event pair around a launch adds to the launch's own time on this stream (the pair's two records
        // back to back, the stream busy with the solve's last kernels): reported beside the timed launches
        hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;
        if (sv.new_event(&ev_c0) == SCS_OK && sv.new_event(&ev_c1) == SCS_OK) {
            sv.ev_cal[0] = ev_c0;
            sv.ev_cal[1] = ev_c1;
            hipEventRecord(ev_c0, s);
            hipEventRecord(ev_c1, s);
        }
        dbuf maps_d;
        SCS_TRY(maps_d.alloc((size_t)n * 2 * 8));
        k_extract_maps<<<(n + 255) / 256, 256, 0, s>>>(Q, q3, n, g->d_dinv, 1.0 / g->dd_norm, constrained ? 1 : 0,
                                                      maps_d.d());
        // (page-locked staging: a pageable destination goes through the runtime's own bounce buffers)
        struct pinned_buf {
            scs_ctx *ctx;
            void *p = nullptr;
            ~pinned_buf() {
                if (p) scs_pinned_release(ctx, p);
            }
        } cols_h{ctx};
        SCS_TRY(scs_pinned_get(ctx, (size_t)n * 2 * 8, &cols_h.p));
        const double *cols = (const double *)cols_h.p;
        SCS_HIP_CHECK(hipMemcpyAsync(cols_h.p, maps_d.p, (size_t)n * 2 * 8, hipMemcpyDeviceToHost, s));
        // (fused loop: TH already holds the next iteration's Ritz values; h_th has X's)
        if (!fused)
            SCS_HIP_CHECK(hipMemcpyAsync(h_th.data(), TH, (size_t)(b + 1) * 8, hipMemcpyDeviceToHost, s));
        SCS_HIP_CHECK(hipEventRecord(ev_b, s));
        SCS_HIP_CHECK(hipStreamSynchronize(s));
        std::vector<double> c0(n), c1(n);
        for (int i = 0; i < n; ++i) {
            c0[i] = cols[(size_t)i * 2];
            c1[i] = cols[(size_t)i * 2 + 1];
        }
        if (constrained) {
            st->lambda[0] = 1.0;
            st->lambda[1] = h_th[0];
            st->lambda_next = b > 1 ? h_th[1] : 0.0;
        } else {
            st->lambda[0] = h_th[0];
            st->lambda[1] = h_th[1];
            st->lambda_next = b > 2 ? h_th[2] : 0.0;
        }
        sign_flip_and_store(c0, c1, n, maps_out);
        return SCS_OK;
    }

    // the counts and the event arithmetic (after `extract`: every event has been reached)
    void fill_stats(scs_stats *st) const {
        st->block = b;
        st->n_apply = sv.n_apply;
        st->n_apply32 = sv.n_apply32;
        st->used_constraint = constrained ? 1 : 0;
        st->resid[0] = final_res[0];
        st->resid[1] = final_res[1];
        double tot = 0.0, mn = 1e300, tot32 = 0.0;
        int n_timed = 0, n_timed32 = 0;
        for (size_t i = 0; i + 1 < sv.ev.size(); i += 2) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, sv.ev[i], sv.ev[i + 1]) == hipSuccess) {
                if (i / 2 < sv.ev32.size() && sv.ev32[i / 2]) {
                    tot32 += t;
                    ++n_timed32;
                    continue;
                }
                tot += t;
                mn = std::min(mn, (double)t);
                ++n_timed;
            }
        }
        // the fused loop times every fourth launch: scale the sample to all launches (of its kind: the
        // launches that streamed the single-precision image are reported on their own)
        if (n_timed > 0) tot *= (double)(sv.n_apply - sv.n_apply32) / n_timed;
        if (n_timed32 > 0) tot32 *= (double)sv.n_apply32 / n_timed32;
        st->apply_ms_total = tot;
        st->apply32_ms_total = tot32;
        st->apply32_bytes = sv.n_apply32 ? sv.w32_bytes_per_apply + 8.0 * (double)n * b + 8.0 * (double)sv.rows * b : 0.0;
        st->apply_ms_min = n_timed ? mn : 0.0;
        {
            float t = 0.f;
            st->event_pair_ms = (sv.ev_cal[1] && hipEventElapsedTime(&t, sv.ev_cal[0], sv.ev_cal[1]) == hipSuccess) ? t : 0.0;
        }
        // W bytes one application streams (all of this rank's rows, or the upper tiles of the
        // symmetric schedule) + the block in and out
        st->apply_bytes = sv.w_bytes_per_apply + 8.0 * (double)n * b + 8.0 * (double)sv.rows * b;
        {
            // the timed all-gathers (every fourth iteration of the fused loop), scaled to all of them
            double ag = 0.0;
            int n_ag = 0;
            for (size_t i = 0; i + 1 < sv.ev_ag.size(); i += 2) {
                float t = 0.f;
                if (hipEventElapsedTime(&t, sv.ev_ag[i], sv.ev_ag[i + 1]) == hipSuccess) {
                    ag += t;
                    ++n_ag;
                }
            }
            st->n_allgather = sv.n_allgather;
            st->allgather_ms_total = n_ag ? ag * (double)sv.n_allgather / n_ag : 0.0;
            // bytes one all-gather delivers to this rank: `world` chunks of `chunk` doubles
            st->allgather_bytes = sv.world > 1 ? 8.0 * (double)sv.chunk * sv.world : 0.0;
        }
    }
};

}  // namespace

// small-V path: dense S on the device, full Jacobi, top two eigenvectors
// 65 .. 128 vertices: dense S on the device, one-sided Jacobi in LDS (k_dense_onesided)
static int fiedler_dense_onesided(scs_ctx *ctx, scs_graph *g, double *maps, scs_stats *st) {
    const int n = g->n;
    hipStream_t s = ctx->stream;
    SCS_REQUIRE(ctx->comm.world == 1 && !g->upper, "dense path needs the whole matrix on one rank (V = %d)", n);
    dbuf sd, wv, vv;
    SCS_TRY(sd.alloc((size_t)n * n * 8));
    SCS_TRY(wv.alloc(4 * 8));
    SCS_TRY(vv.alloc((size_t)n * 2 * 8));
    k_dense_s<<<(n * n + 255) / 256, 256, 0, s>>>(g->d_w, g->ld, n, g->d_dinv, sd.d());
    const size_t lds = (size_t)(n + (n & 1)) * DENSE2_LD * sizeof(double);
    // (the attribute is per function AND device: set on every call -- a process may drive several
    // devices and threads, and a flag set once would cover only the first)
    SCS_HIP_CHECK(hipFuncSetAttribute((const void *)k_dense_onesided, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      DENSE2_MAX * DENSE2_LD * (int)sizeof(double)));
    k_dense_onesided<<<1, 256, lds, s>>>(sd.d(), n, wv.d(), vv.d());
    SCS_HIP_CHECK(hipGetLastError());
    std::vector<double> w(4), v((size_t)n * 2), dinv(n);
    SCS_HIP_CHECK(hipMemcpyAsync(w.data(), wv.p, 4 * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipMemcpyAsync(v.data(), vv.p, (size_t)n * 2 * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipMemcpyAsync(dinv.data(), g->d_dinv, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<double> c0(n), c1(n);
    for (int i = 0; i < n; ++i) {
        c0[i] = v[(size_t)i * 2 + 0] * dinv[i];
        c1[i] = v[(size_t)i * 2 + 1] * dinv[i];
    }
    sign_flip_and_store(c0, c1, n, maps);
    if (st) {
        st->block = 0;
        st->converged = w[3] != 0.0 ? 1 : 0;
        st->lambda[0] = w[0];
        st->lambda[1] = w[1];
        st->lambda_next = w[2];
    }
    if (w[3] == 0.0) {
        scs_set_error("scs_fiedler: the dense one-sided Jacobi did not converge in 40 sweeps (V = %d)", n);
        return SCS_ENOCONV;
    }
    return SCS_OK;
}

static int fiedler_dense(scs_ctx *ctx, scs_graph *g, double *maps, scs_stats *st) {
    const int n = g->n;
    hipStream_t s = ctx->stream;
    SCS_REQUIRE(ctx->comm.world == 1, "dense small-V path needs world == 1 (V = %d)", n);
    dbuf sd, wv, vv;
    SCS_TRY(sd.alloc((size_t)n * n * 8));
    SCS_TRY(wv.alloc((size_t)n * 8));
    SCS_TRY(vv.alloc((size_t)n * n * 8));
    k_dense_s<<<(n * n + 255) / 256, 256, 0, s>>>(g->d_w, g->ld, n, g->d_dinv, sd.d());
    k_small_eig<<<1, 256, 0, s>>>(sd.d(), n, wv.d(), vv.d());
    std::vector<double> w(n), v((size_t)n * n), dinv(n);
    SCS_HIP_CHECK(hipMemcpyAsync(w.data(), wv.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipMemcpyAsync(v.data(), vv.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipMemcpyAsync(dinv.data(), g->d_dinv, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<double> c0(n), c1(n);
    for (int i = 0; i < n; ++i) {
        c0[i] = v[(size_t)i * n + 0] * dinv[i];
        c1[i] = (n > 1 ? v[(size_t)i * n + 1] : 0.0) * dinv[i];
    }
    sign_flip_and_store(c0, c1, n, maps);
    if (st) {
        st->block = 0;
        st->converged = 1;
        st->lambda[0] = w[0];
        st->lambda[1] = n > 1 ? w[1] : 0.0;
        st->lambda_next = n > 2 ? w[2] : 0.0;
    }
    return SCS_OK;
}

extern "C" int scs_fiedler(scs_ctx *ctx, scs_graph *g, const double *x_init, double tol,
                           int32_t max_iter, int32_t block, double *maps_out, scs_stats *stats) {
    SCS_REQUIRE(ctx && g && maps_out, "scs_fiedler: null argument");
    SCS_REQUIRE(g->n >= 2, "scs_fiedler: need at least 2 vertices (have %d)", g->n);
    SCS_REQUIRE(!g->upper || g->n > MAXS, "scs_fiedler: an SCS_BUILD_UPPER graph needs more than %d vertices", MAXS);
    SCS_REQUIRE(block >= 0 && block <= MAXB, "scs_fiedler: block must be in [0, %d]", MAXB);
    SCS_REQUIRE(tol > 0.0 && max_iter >= 1, "scs_fiedler: tol must be > 0 and max_iter >= 1");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    const int n = g->n;
    scs_stats st_local;
    scs_stats *st = stats ? stats : &st_local;
    memset(st, 0, sizeof(*st));
    st->n_vertices = n;

    // timing events live in the context (created once: this call is made thousands of times
    // per recursion)
    for (auto &e : ctx->solve_events)
        if (!e) SCS_HIP_CHECK(hipEventCreate(&e));
    hipEvent_t ev_a = ctx->solve_events[0], ev_b = ctx->solve_events[1];
    SCS_HIP_CHECK(hipEventRecord(ev_a, s));
    const auto t_entry = std::chrono::steady_clock::now();

    if (n <= DENSE2_MAX) SCS_TRY(scs_graph_prepare_degrees(ctx, g));

    // 65 .. 96 vertices on one rank: the one-sided dense solve.  Its time grows with n^2 (n - 1
    // steps per sweep, each rewriting two columns per pair): measured 1.9 ms at 80 vertices
    // against 3.0 ms for LOBPCG, 4.5 against 3.5 ms at 120 -- the crossover is near 100.
    // An asked-for block width keeps the iterative path.
    static const int dense_max = 96;
    int (*dense)(scs_ctx *, scs_graph *, double *, scs_stats *) = nullptr;
    if (n > MAXS && n <= dense_max && block == 0 && ctx->comm.world == 1 && !g->upper) dense = fiedler_dense_onesided;
    if (n <= MAXS) dense = fiedler_dense;
    if (dense) {
        SCS_TRY(dense(ctx, g, maps_out, st));
        SCS_HIP_CHECK(hipEventRecord(ev_b, s));
        SCS_HIP_CHECK(hipEventSynchronize(ev_b));
        float ms = 0.f;
        hipEventElapsedTime(&ms, ev_a, ev_b);
        st->solve_ms = ms;
        return SCS_OK;
    }

    const loop_plan plan{};
    bool want32 = false;
    const int b = choose_width(ctx, g, block, plan, &want32);
    // (the iterative path allocates and clears its buffers while k_degrees streams W, and only then waits
    // for the degrees)
    SCS_TRY(scs_graph_prepare_degrees_begin(ctx, g, want32));
    lobpcg L(ctx, g, b, plan);
    SCS_TRY(L.setup(tol, want32));
    SCS_TRY(L.start(x_init));

    int iter = 0;
    bool converged = false;
    for (iter = 0; iter < max_iter; ++iter) {
        if (L.fused) {
            double seq = 0.0;
            SCS_TRY(L.enqueue_fused(&seq));
            SCS_TRY(L.await_report(seq, iter));
        } else {
            SCS_TRY(L.read_residual());
        }
        const double worst = L.worst_residual();
        static const bool trace_res = dbg_on("SCS_TRACE_RESIDUAL");
        if (trace_res) fprintf(stderr, "[lobpcg] it %3d  residual %.3e  theta %.12g %.12g\n", iter, worst, L.h_th[0], L.h_th[1]);
        if (!(worst == worst)) {
            scs_set_error("scs_fiedler: NaN residual at iteration %d", iter);
            return SCS_EHIP;
        }
        const int action = L.policy.step(worst);
        if (action == scs_loop_policy::RENEW) {
            SCS_TRY(L.renew());
            ++st->lowp_renewals;
        }
        if (action == scs_loop_policy::STOP) {
            if (!L.policy.begin_confirmation()) {
                converged = worst <= tol;
                break;
            }
            double w2 = 0.0;
            SCS_TRY(L.confirm(tol, &w2));
            bool conv = false;
            if (L.policy.confirm(w2, &conv)) {
                converged = conv;
                break;
            }
            SCS_TRY(L.restart_directions());
        }
        if (!L.fused) SCS_TRY(L.unfused_back());
    }

    SCS_TRY(L.extract(ev_b, maps_out, st));
    float ms = 0.f;
    hipEventElapsedTime(&ms, ev_a, ev_b);
    st->solve_ms = ms;
    st->iterations = iter;
    st->converged = converged ? 1 : 0;
    L.fill_stats(st);
    const double res = std::max(L.final_res[0], L.final_res[1]);
    if (n >= 4096 && dbg_on("SCS_TRACE_SOLVES"))
        fprintf(stderr, "[solve] V %d block %d iterations %d applies %d image %d renewals %d refreshes %d solve_ms %.3f "
                        "wall_ms %.3f residual %.3e gap %.3e\n", n, b, iter, st->n_apply, st->n_apply32, st->lowp_renewals,
                L.policy.confirmations, st->solve_ms,
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_entry).count(),
                res, st->lambda[1] - st->lambda_next);
    if (!converged) {
        // maps_out and stats are filled: the caller decides whether the block is usable
        scs_set_error("scs_fiedler: residual %.3e above tol %.3e after %d iterations (V = %d, block %d)", res, tol,
                      iter, n, b);
        return SCS_ENOCONV;
    }
    return SCS_OK;
}

#include "scs_eig_small.h"
#include "scs_eig_debug.h"
