// The eigen-solver's debug exports (parity tests of the building blocks).  Included by scs_eig.hip at its end (one
// translation unit: they reach the kernels, `solver` and the loop policy defined there).

// ---------------------------------------------------------------------------
// debug entry points (parity tests of the building blocks)
// ---------------------------------------------------------------------------
extern "C" int scs_debug_jacobi(scs_ctx *ctx, const double *a, int32_t n, double *w, double *v) {
    SCS_REQUIRE(ctx && a && w && v, "scs_debug_jacobi: null argument");
    SCS_REQUIRE(n >= 1 && n <= MAXS, "scs_debug_jacobi: n must be in [1, %d]", MAXS);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    dbuf da, dw, dv;
    SCS_TRY(da.alloc((size_t)n * n * 8));
    SCS_TRY(dw.alloc((size_t)n * 8));
    SCS_TRY(dv.alloc((size_t)n * n * 8));
    SCS_HIP_CHECK(hipMemcpyAsync(da.p, a, (size_t)n * n * 8, hipMemcpyHostToDevice, ctx->stream));
    k_small_eig<<<1, 256, 0, ctx->stream>>>(da.d(), n, dw.d(), dv.d());
    SCS_HIP_CHECK(hipMemcpyAsync(w, dw.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SCS_HIP_CHECK(hipMemcpyAsync(v, dv.p, (size_t)n * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SCS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SCS_OK;
}

// whole panels, the loop's own count of partials: scs_debug_gram_ex says the rest
extern "C" int scs_debug_gram(scs_ctx *ctx, const double *a, const double *b, int32_t n,
                              int32_t ka, int32_t kb, int32_t use_mfma, double *out) {
    return scs_debug_gram_ex(ctx, a, ka, 0, ka, b, kb, 0, kb, n, use_mfma, 256, out);
}

// one application through W: scs_debug_apply_ex says the rest
extern "C" int scs_debug_apply(scs_ctx *ctx, scs_graph *g, const double *x, int32_t b, double *y) {
    int32_t info[8];
    return scs_debug_apply_ex(ctx, g, x, b, 0, 1, y, info);
}

// scs_debug_apply with ONE solver object for `reps` applications (the tile lists alternate as in the loop),
// optionally on the single-precision image, and a report of what ran
extern "C" int scs_debug_apply_ex(scs_ctx *ctx, scs_graph *g, const double *x, int32_t b, int32_t image,
                                  int32_t reps, double *y_out, int32_t *info_out) {
    SCS_REQUIRE(ctx && g && x && y_out && info_out, "scs_debug_apply_ex: null argument");
    SCS_REQUIRE(b == 4 || b == 8 || b == 12 || b == 16, "scs_debug_apply_ex: b must be 4, 8, 12 or 16");
    SCS_REQUIRE(reps >= 1 && reps <= 64, "scs_debug_apply_ex: reps must be in [1, 64]");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    if (image) {
        SCS_REQUIRE(!g->mf, "scs_debug_apply_ex: a matrix-free graph has no image");
        SCS_REQUIRE(b == 4, "scs_debug_apply_ex: the image is streamed at block width 4 (asked: %d)", b);
        SCS_TRY(scs_graph_prepare_degrees_begin(ctx, g, true));
    }
    SCS_TRY(scs_graph_prepare_degrees(ctx, g));
    const int n = g->n;
    solver sv;
    sv.bind(ctx, n, b, g);
    dbuf dx;
    SCS_TRY(dx.alloc((size_t)n * b * 8));
    SCS_TRY(sv.alloc_symm_buffers());
    if (image) {
        // (where scs_fiedler streams none, nothing else is ever run on it)
        if (!g->have_w32 || !solver::image_layout(ctx, g, b)) {
            scs_set_error("scs_debug_apply_ex: no image for this graph (%s)",
                          !g->have_w32 ? "it could not be made" : "the solver does not stream one at this size");
            return SCS_EUNSUP;
        }
        sv.use32 = true;
    }
    // (an SCS_BUILD_UPPER graph: collective, the product comes back for all V rows and this
    // rank's slice of it is returned)
    const size_t out_rows = (size_t)(g->upper ? n : sv.rows);
    SCS_TRY(sv.yloc.alloc(out_rows * b * 8));
    SCS_HIP_CHECK(hipMemcpyAsync(dx.p, x, (size_t)n * b * 8, hipMemcpyHostToDevice, ctx->stream));
    k_scale_rows<<<(n * b + 255) / 256, 256, 0, ctx->stream>>>(dx.d(), b, 0, b, n, g->d_dinv, sv.z.d(), sv.ldz);
    int tiles = 0;
    for (int r = 0; r < reps; ++r) {
        // every application has to write every partial sum it adds up: what an earlier one left must not
        // stand in for a tile that was dropped
        if (sv.tri) {  // (the sizes alloc_symm_buffers gave them)
            const size_t slab = (size_t)n * b * 8;
            const size_t n_rb = g->upper ? (size_t)(sv.tri_rb_hi - sv.tri_rb_lo) : (size_t)((n + TRI_TH - 1) / TRI_TH);
            SCS_HIP_CHECK(hipMemsetAsync(sv.tri_pdir.p, 0xFF, (size_t)std::max(sv.tri_nct, sv.tri32_nct) * slab,
                                         ctx->stream));
            SCS_HIP_CHECK(hipMemsetAsync(sv.tri_ptr.p, 0xFF, n_rb * slab, ctx->stream));
        }
        if (!g->mf) SCS_HIP_CHECK(hipMemsetAsync(sv.ypart.p, 0xFF, sv.ypart_cap * 8, ctx->stream));
        SCS_HIP_CHECK(hipMemsetAsync(sv.yloc.p, 0xFF, out_rows * b * 8, ctx->stream));
        SCS_TRY(sv.launch_symm(sv.z.d(), sv.yloc.d()));
        SCS_HIP_CHECK(hipMemcpyAsync(y_out + (size_t)r * sv.rows * b,
                                     sv.yloc.d() + (g->upper ? (size_t)g->row_begin * b : 0),
                                     (size_t)sv.rows * b * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    SCS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (sv.tri) tiles = sv.use32 ? sv.tri32_ntiles : sv.tri_ntiles;
    info_out[0] = sv.tri ? 1 : 0;
    info_out[1] = sv.use32 ? 1 : 0;
    info_out[2] = tiles;
    info_out[3] = sv.last_nseg;
    info_out[4] = sv.tri ? (sv.use32 ? 512 : sv.tri_ct * 128) : 0;
    info_out[5] = sv.n_apply32;
    info_out[6] = sv.part_mode ? 1 : 0;
    info_out[7] = g->mf ? 1 : 0;
    return SCS_OK;
}

// The operator as a multi-rank solve assembles it (collective): the solver is set up as scs_fiedler sets it up,
// S is applied to the R block of the host panel q by solver::apply (path 0) or solver::fused_back with
// fold_pass2 off (path 1), `reps` times on one solver object, and every application returns the R slot of AQ
// -- all V rows, as THIS rank holds them after the gather
extern "C" int scs_debug_team_apply(scs_ctx *ctx, scs_graph *g, const double *q, const double *aq, int32_t b,
                                    int32_t path, int32_t image, int32_t reps, double *y_out, double *qaq_out,
                                    double *part_out, int64_t *info_out) {
    // (argument checks: the same verdict on every rank, before the first collective)
    SCS_REQUIRE(ctx && g && q && aq && y_out && info_out, "scs_debug_team_apply: null argument");
    SCS_REQUIRE(!g->mf, "scs_debug_team_apply: a matrix-free graph is solved on one rank");
    SCS_REQUIRE(path == 0 || path == 1, "scs_debug_team_apply: path must be 0 (apply) or 1 (fused_back)");
    SCS_REQUIRE(b == 4 || b == 8 || b == 12 || b == 16, "scs_debug_team_apply: b must be 4, 8, 12 or 16");
    SCS_REQUIRE(path == 0 || b == 4 || b == 8, "scs_debug_team_apply: the fused loop takes block widths 4 and 8 (asked: %d)", b);
    SCS_REQUIRE(path == 0 || qaq_out, "scs_debug_team_apply: path 1 returns Q^T AQ");
    SCS_REQUIRE(!g->upper || part_out, "scs_debug_team_apply: an SCS_BUILD_UPPER graph returns its partial product");
    SCS_REQUIRE(reps >= 1 && reps <= 64, "scs_debug_team_apply: reps must be in [1, 64]");
    SCS_REQUIRE(!image || b == 4, "scs_debug_team_apply: the image is streamed at block width 4 (asked: %d)", b);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    const int n = g->n, q3 = 3 * b;
    // (this export streams the image as a row-partitioned rank does: of its rows)
    const bool image_rows = ctx->comm.world > 1 && solver::image_layout(ctx, g, b);
    SCS_TRY(scs_graph_prepare_degrees_begin(ctx, g, image && image_rows));
    SCS_TRY(scs_graph_prepare_degrees(ctx, g));

    solver sv;
    sv.bind(ctx, n, b, g);
    SCS_TRY(sv.team_splits());
    // (from here on every refusal is the same on all ranks and no collective lies behind it)
    SCS_TRY(sv.alloc_symm_buffers());
    if (image) {
        if (!image_rows || !g->have_w32) {
            scs_set_error("scs_debug_team_apply: no image for this graph (%s)",
                          image_rows ? "it could not be made" : "the solver does not stream one in this layout or at this size");
            return SCS_EUNSUP;
        }
        sv.use32 = true;
    }
    SCS_TRY(sv.q.alloc((size_t)n * q3 * 8));
    SCS_TRY(sv.aq.alloc((size_t)n * q3 * 8));
    SCS_TRY(sv.yloc.alloc((size_t)sv.chunk * 8));
    SCS_TRY(sv.part2.alloc((size_t)1024 * q3 * q3 * 8));
    SCS_TRY(sv.small.alloc((size_t)SM_TOTAL * 8));
    SCS_TRY(sv.team_buffers());
    SCS_HIP_CHECK(hipMemcpyAsync(sv.q.p, q, (size_t)n * q3 * 8, hipMemcpyHostToDevice, s));
    SCS_HIP_CHECK(hipMemcpyAsync(sv.aq.p, aq, (size_t)n * q3 * 8, hipMemcpyHostToDevice, s));
    double *G = sv.small_at(SM_G);
    const size_t slab = (size_t)n * b * 8;
    for (int r = 0; r < reps; ++r) {
        // whatever an application adds up or unpacks it has to have written itself: a tail of a chunk, a slab or
        // a row that nobody wrote is NaN in the product, not what the application before left there
        if (sv.tri) {  // (the sizes alloc_symm_buffers gave them)
            const size_t n_rb = sv.part_mode ? (size_t)(sv.tri_rb_hi - sv.tri_rb_lo) : (size_t)((n + TRI_TH - 1) / TRI_TH);
            SCS_HIP_CHECK(hipMemsetAsync(sv.tri_pdir.p, 0xFF, (size_t)std::max(sv.tri_nct, sv.tri32_nct) * slab, s));
            SCS_HIP_CHECK(hipMemsetAsync(sv.tri_ptr.p, 0xFF, n_rb * slab, s));
        }
        if (sv.ysend.p) SCS_HIP_CHECK(hipMemsetAsync(sv.ysend.p, 0xFF, slab, s));
        if (sv.recv.p) SCS_HIP_CHECK(hipMemsetAsync(sv.recv.p, 0xFF, (size_t)sv.chunk * sv.world * 8, s));
        if (sv.yfull.p) SCS_HIP_CHECK(hipMemsetAsync(sv.yfull.p, 0xFF, slab, s));
        SCS_HIP_CHECK(hipMemsetAsync(sv.ypart.p, 0xFF, sv.ypart_cap * 8, s));
        SCS_HIP_CHECK(hipMemsetAsync(sv.yloc.p, 0xFF, (size_t)sv.chunk * 8, s));
        SCS_HIP_CHECK(hipMemset2DAsync(sv.aq.d() + 2 * b, (size_t)q3 * 8, 0xFF, (size_t)b * 8, (size_t)n, s));
        if (path == 0) {
            SCS_TRY(sv.apply(sv.q.d(), 2 * b, sv.aq.d(), 2 * b));
        } else {
            int nparts = 0;
            k_scale_rows<<<(n * b + 255) / 256, 256, 0, s>>>(sv.q.d(), q3, 2 * b, b, n, g->d_dinv, sv.z.d(), sv.ldz);
            if (b == 4) {
                SCS_TRY(sv.fused_back<4>(&nparts, sv.part2.d()));
            } else {
                SCS_TRY(sv.fused_back<8>(&nparts, sv.part2.d()));
            }
            k_reduce_partials<<<(q3 * q3 + 3) / 4, 256, 0, s>>>(sv.part2.d(), nparts, q3 * q3, G);
            SCS_HIP_CHECK(hipGetLastError());
            SCS_HIP_CHECK(hipMemcpyAsync(qaq_out + (size_t)r * q3 * q3, G, (size_t)q3 * q3 * 8,
                                         hipMemcpyDeviceToHost, s));
        }
        SCS_HIP_CHECK(hipGetLastError());
        SCS_HIP_CHECK(hipMemcpy2DAsync(y_out + (size_t)r * n * b, (size_t)b * 8, sv.aq.d() + 2 * b, (size_t)q3 * 8,
                                       (size_t)b * 8, (size_t)n, hipMemcpyDeviceToHost, s));
        if (sv.part_mode)
            SCS_HIP_CHECK(hipMemcpyAsync(part_out + (size_t)r * n * b, sv.ysend.p, slab, hipMemcpyDeviceToHost, s));
        // (a peer reads this rank's send buffer inside the gather: nothing is refilled before all have met there,
        // and the in-process gather ends with such a meeting)
        SCS_HIP_CHECK(hipStreamSynchronize(s));
    }
    info_out[0] = sv.part_mode ? 1 : 0;
    info_out[1] = path;
    info_out[2] = sv.world;
    info_out[3] = sv.chunk;
    info_out[4] = sv.last_nseg;
    info_out[5] = sv.tri ? sv.tri_ntiles : 0;
    info_out[6] = sv.n_apply32;
    info_out[7] = sv.n_allgather;
    return SCS_OK;
}

// scs_debug_gram on column sub-blocks of wider host panels, with the caller's count of partials
extern "C" int scs_debug_gram_ex(scs_ctx *ctx, const double *a, int32_t lda, int32_t a_col0, int32_t ka,
                                 const double *b, int32_t ldb, int32_t b_col0, int32_t kb, int32_t n,
                                 int32_t use_mfma, int32_t gram_blocks, double *out) {
    SCS_REQUIRE(ctx && a && b && out, "scs_debug_gram_ex: null argument");
    SCS_REQUIRE(n >= 1 && ka >= 1 && ka <= 48 && kb >= 1 && kb <= 48, "scs_debug_gram_ex: bad shape");
    SCS_REQUIRE(a_col0 >= 0 && a_col0 + ka <= lda && b_col0 >= 0 && b_col0 + kb <= ldb,
                "scs_debug_gram_ex: the column block leaves the panel");
    SCS_REQUIRE(gram_blocks >= 1 && gram_blocks <= 1024, "scs_debug_gram_ex: gram_blocks must be in [1, 1024]");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    solver sv;
    sv.bind(ctx, n);
    sv.gram_blocks = gram_blocks;
    const bool same = a == b && lda == ldb;  // two blocks of one panel, as gram(Q, 3b, 2b, R, 3b, b)
    dbuf da, db, dout;
    SCS_TRY(da.alloc((size_t)n * lda * 8));
    if (!same) SCS_TRY(db.alloc((size_t)n * ldb * 8));
    SCS_TRY(dout.alloc((size_t)ka * kb * 8));
    SCS_TRY(sv.part.alloc((size_t)1024 * 48 * 48 * 8));
    SCS_HIP_CHECK(hipMemsetAsync(sv.part.p, 0xFF, (size_t)1024 * 48 * 48 * 8, ctx->stream));
    SCS_HIP_CHECK(hipMemcpyAsync(da.p, a, (size_t)n * lda * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!same) SCS_HIP_CHECK(hipMemcpyAsync(db.p, b, (size_t)n * ldb * 8, hipMemcpyHostToDevice, ctx->stream));
    SCS_TRY(sv.gram(da.d() + a_col0, lda, ka, (same ? da.d() : db.d()) + b_col0, ldb, kb, dout.d(), use_mfma != 0));
    SCS_HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t)ka * kb * 8, hipMemcpyDeviceToHost, ctx->stream));
    SCS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SCS_OK;
}

// one k_update launch on host operands; the whole y panel travels both ways
extern "C" int scs_debug_update(scs_ctx *ctx, double *y, int32_t ldy, int32_t y_col0, int32_t kc, double alpha,
                                const double *a, int32_t lda, int32_t a_col0, int32_t ka, const double *c,
                                int32_t ldc, double sign, int32_t n) {
    SCS_REQUIRE(ctx && y && a && c, "scs_debug_update: null argument");
    SCS_REQUIRE(n >= 1 && kc >= 1 && kc <= MAXB && ka >= 1 && ka <= 3 * MAXB, "scs_debug_update: bad shape");
    SCS_REQUIRE(y_col0 >= 0 && y_col0 + kc <= ldy && a_col0 >= 0 && a_col0 + ka <= lda && ldc >= kc,
                "scs_debug_update: the column block leaves the panel");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    solver sv;
    sv.bind(ctx, n);
    const bool same = a == y && lda == ldy;  // in place, or two blocks of one panel
    dbuf dy, da, dc;
    SCS_TRY(dy.alloc((size_t)n * ldy * 8));
    if (!same) SCS_TRY(da.alloc((size_t)n * lda * 8));
    SCS_TRY(dc.alloc((size_t)ka * ldc * 8));
    SCS_HIP_CHECK(hipMemcpyAsync(dy.p, y, (size_t)n * ldy * 8, hipMemcpyHostToDevice, ctx->stream));
    if (!same) SCS_HIP_CHECK(hipMemcpyAsync(da.p, a, (size_t)n * lda * 8, hipMemcpyHostToDevice, ctx->stream));
    SCS_HIP_CHECK(hipMemcpyAsync(dc.p, c, (size_t)ka * ldc * 8, hipMemcpyHostToDevice, ctx->stream));
    SCS_TRY(sv.update(dy.d() + y_col0, ldy, kc, alpha, (same ? dy.d() : da.d()) + a_col0, lda, ka, dc.d(), ldc, sign));
    SCS_HIP_CHECK(hipMemcpyAsync(y, dy.p, (size_t)n * ldy * 8, hipMemcpyDeviceToHost, ctx->stream));
    SCS_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return SCS_OK;
}

// ---- the loop's small solves and tall panel kernels, one launch each
// Every output and every scratch buffer starts as 0xFF bytes (NaN, -1): what the launch did not write shows.
static int debug_upload(dbuf &d, const void *host, size_t bytes, hipStream_t s) {
    SCS_TRY(d.alloc(bytes));
    SCS_HIP_CHECK(hipMemcpyAsync(d.p, host, bytes, hipMemcpyHostToDevice, s));
    return SCS_OK;
}
static int debug_blank(dbuf &d, size_t bytes, hipStream_t s) {
    SCS_TRY(d.alloc(bytes));
    SCS_HIP_CHECK(hipMemsetAsync(d.p, 0xFF, bytes, s));
    return SCS_OK;
}
static int debug_download(void *host, const dbuf &d, size_t bytes, hipStream_t s) {
    if (host) SCS_HIP_CHECK(hipMemcpyAsync(host, d.p, bytes, hipMemcpyDeviceToHost, s));
    return SCS_OK;
}

// small_rr_body with the register-and-shuffle path switched off: nq = 3b at b = 4, 8 on the general path
__global__ __launch_bounds__(256) void k_debug_small_rr_general(const double *__restrict__ tm, int nparts, int nq,
                                                                 int b, const int *__restrict__ mask,
                                                                 double *__restrict__ c, double *__restrict__ d,
                                                                 double *__restrict__ theta,
                                                                 int *__restrict__ mask_p, double drop_tol,
                                                                 int exact_from) {
    small_rr_body(tm, nparts, nq, b, mask, c, d, theta, mask_p, drop_tol, exact_from, false);
}

// the projected SVQB on the compact layout of one width, declared and called as k_symm_tri_tf does
template <int B>
__global__ __launch_bounds__(256) void k_debug_small_orth_compact(const double *__restrict__ partial, int nparts,
                                                                   double drop_tol, double *__restrict__ coef,
                                                                   int *__restrict__ mask,
                                                                   const double *__restrict__ theta, double *report,
                                                                   double seq) {
    __shared__ orth_small_lds<B> L;
    small_orth_core(L, partial, nparts, B, drop_tol, L.coef, mask, theta, report, seq);
    __syncthreads();
    for (int e = threadIdx.x; e < PANEL_COEF_ROWS<B> * B; e += 256) coef[e] = L.coef[e];
}

extern "C" int scs_debug_small_svqb(scs_ctx *ctx, const double *g, int32_t k, double drop_tol, double *t_out,
                                    int32_t *mask_out) {
    SCS_REQUIRE(ctx && g && t_out && mask_out, "scs_debug_small_svqb: null argument");
    SCS_REQUIRE(k >= 1 && k <= MAXS, "scs_debug_small_svqb: k must be in [1, %d]", MAXS);
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    dbuf dg, dt, dm;
    SCS_TRY(debug_upload(dg, g, (size_t)k * k * 8, s));
    SCS_TRY(debug_blank(dt, (size_t)k * k * 8, s));
    SCS_TRY(debug_blank(dm, (size_t)k * 4, s));
    k_small_svqb<<<1, 256, 0, s>>>(dg.d(), k, drop_tol, dt.d(), (int *)dm.p);
    SCS_HIP_CHECK(hipGetLastError());
    SCS_TRY(debug_download(t_out, dt, (size_t)k * k * 8, s));
    SCS_TRY(debug_download(mask_out, dm, (size_t)k * 4, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    return SCS_OK;
}

extern "C" int scs_debug_small_rr(scs_ctx *ctx, const double *tm, int32_t nparts, int32_t nq, int32_t b,
                                  const int32_t *mask, double drop_tol, int32_t exact_from, int32_t start,
                                  double *c_out, double *d_out, double *theta_out, int32_t *mask_p_out,
                                  int32_t *mask_out) {
    SCS_REQUIRE(ctx && tm && c_out && d_out && theta_out && mask_p_out && mask_out,
                "scs_debug_small_rr: null argument");
    SCS_REQUIRE(start >= 0 && start <= 2, "scs_debug_small_rr: start must be 0 (k_small_rr), 1 (k_small_rr_start) "
                                          "or 2 (k_small_rr's body on the general path)");
    SCS_REQUIRE(b >= 1 && b <= MAXB && nq >= b && nq <= 3 * b, "scs_debug_small_rr: need 1 <= b <= %d, b <= nq <= 3b",
                MAXB);
    SCS_REQUIRE(nparts >= 0 && nparts <= 1024, "scs_debug_small_rr: nparts must be in [0, 1024]");
    SCS_REQUIRE(nparts == 0 || nq <= 24, "scs_debug_small_rr: partials are summed for nq <= 24 only (asked: %d)", nq);
    SCS_REQUIRE(exact_from >= -1 && exact_from <= nq, "scs_debug_small_rr: exact_from must be in [-1, nq]");
    SCS_REQUIRE(start != 1 || (nq == b && nparts == 0 && exact_from < 0),
                "scs_debug_small_rr: k_small_rr_start solves nq = b on one matrix");
    SCS_REQUIRE(start == 1 || mask, "scs_debug_small_rr: null mask");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    const size_t nt = (size_t)std::max(1, nparts) * nq * nq;
    dbuf dtm, dmask, dc, dd, dth, dmp;
    SCS_TRY(debug_upload(dtm, tm, nt * 8, s));
    SCS_TRY(debug_blank(dmask, 48 * 4, s));
    SCS_TRY(debug_blank(dc, (size_t)nq * b * 8, s));
    SCS_TRY(debug_blank(dd, (size_t)nq * b * 8, s));
    SCS_TRY(debug_blank(dth, (size_t)(b + 1) * 8, s));
    SCS_TRY(debug_blank(dmp, (size_t)b * 4, s));
    if (start != 1) SCS_HIP_CHECK(hipMemcpyAsync(dmask.p, mask, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    int *mk = (int *)dmask.p, *mp = (int *)dmp.p;
    if (start == 1)
        k_small_rr_start<<<1, 256, 0, s>>>(dtm.d(), b, mk, dc.d(), dd.d(), dth.d(), drop_tol);
    else if (start == 2)
        k_debug_small_rr_general<<<1, 256, 0, s>>>(dtm.d(), nparts, nq, b, mk, dc.d(), dd.d(), dth.d(), mp, drop_tol,
                                                   exact_from);
    else
        k_small_rr<<<1, 256, 0, s>>>(dtm.d(), nparts, nq, b, mk, dc.d(), dd.d(), dth.d(), mp, drop_tol, exact_from);
    SCS_HIP_CHECK(hipGetLastError());
    SCS_TRY(debug_download(c_out, dc, (size_t)nq * b * 8, s));
    SCS_TRY(debug_download(d_out, dd, (size_t)nq * b * 8, s));
    SCS_TRY(debug_download(theta_out, dth, (size_t)(b + 1) * 8, s));
    SCS_TRY(debug_download(mask_p_out, dmp, (size_t)b * 4, s));
    SCS_TRY(debug_download(mask_out, dmask, 48 * 4, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    return SCS_OK;
}

extern "C" int scs_debug_small_orth(scs_ctx *ctx, const double *partial, int32_t nparts, int32_t b, double drop_tol,
                                    const double *theta, int32_t layout, double *coef_out, int32_t *mask_out,
                                    double *report_out) {
    SCS_REQUIRE(ctx && partial && theta && coef_out && mask_out && report_out, "scs_debug_small_orth: null argument");
    SCS_REQUIRE(layout == 0 || layout == 1, "scs_debug_small_orth: layout must be 0 (general) or 1 (compact)");
    // (orth_lds holds cxp[16][8], gm[9][8]: the projected SVQB exists for the fused loop's widths only)
    SCS_REQUIRE(b >= 1 && b <= 8, "scs_debug_small_orth: the projected SVQB takes block widths up to 8 (asked: %d)", b);
    SCS_REQUIRE(layout == 0 || b == 4 || b == 8, "scs_debug_small_orth: the compact layout is built for widths 4 and 8");
    SCS_REQUIRE(nparts >= 1 && nparts <= 1024, "scs_debug_small_orth: nparts must be in [1, 1024]");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    const size_t nout = (size_t)3 * b * b + b, ncoef = (size_t)(3 * b + 4) * b;
    const double seq = 7.0;
    dbuf dp, dth, dco, dm, drep;
    SCS_TRY(debug_upload(dp, partial, (size_t)nparts * nout * 8, s));
    SCS_TRY(debug_upload(dth, theta, (size_t)(b + 1) * 8, s));
    SCS_TRY(debug_blank(dco, ncoef * 8, s));
    SCS_TRY(debug_blank(dm, (size_t)b * 4, s));
    SCS_TRY(debug_blank(drep, 41 * 8, s));
    if (layout == 0)
        k_small_orth<<<1, 256, 0, s>>>(dp.d(), nparts, b, drop_tol, dco.d(), (int *)dm.p, dth.d(), drep.d(), seq);
    else if (b == 4)
        k_debug_small_orth_compact<4><<<1, 256, 0, s>>>(dp.d(), nparts, drop_tol, dco.d(), (int *)dm.p, dth.d(),
                                                         drep.d(), seq);
    else
        k_debug_small_orth_compact<8><<<1, 256, 0, s>>>(dp.d(), nparts, drop_tol, dco.d(), (int *)dm.p, dth.d(),
                                                         drep.d(), seq);
    SCS_HIP_CHECK(hipGetLastError());
    SCS_TRY(debug_download(coef_out, dco, ncoef * 8, s));
    SCS_TRY(debug_download(mask_out, dm, (size_t)b * 4, s));
    SCS_TRY(debug_download(report_out, drep, 41 * 8, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    return SCS_OK;
}

template <int B>
static int debug_panel_fused(int which, int n, int nb, double *q, double *aq, const double *u, const double *ca,
                             const double *cb, const double *theta, const double *dinv, const double *ypart,
                             int nseg, double *part, double *zt, int64_t ldz, hipStream_t s) {
    switch (which) {
    case 0: k_panel_rr<B><<<nb, 256, 0, s>>>(q, aq, u, ca, cb, theta, n, part); break;
    case 1: k_panel_tf<B, true, false><<<nb, 256, 0, s>>>(q, u, ca, n, part, nullptr, nullptr, 0); break;
    case 2: k_panel_tf<B, false, true><<<nb, 256, 0, s>>>(q, u, ca, n, nullptr, dinv, zt, ldz); break;
    case 3: k_gram_qaq<B, 0><<<nb, 256, 0, s>>>(q, aq, n, nullptr, 0, nullptr, part); break;
    default: k_gram_qaq<B, 1><<<nb, 256, 0, s>>>(q, aq, n, ypart, nseg, dinv, part); break;
    }
    SCS_HIP_CHECK(hipGetLastError());
    return SCS_OK;
}

extern "C" int scs_debug_panel(scs_ctx *ctx, int32_t which, int32_t b, int32_t n, const double *q, const double *aq,
                               const double *u, const double *coef_a, const double *coef_b, const double *theta,
                               const double *dinv, const double *ypart, int32_t nseg, int32_t blocks, double *q_out,
                               double *aq_out, double *partial_out, double *zt_out) {
    SCS_REQUIRE(ctx && q && aq, "scs_debug_panel: null panel");
    SCS_REQUIRE(which >= 0 && which <= 6, "scs_debug_panel: which must be in [0, 6]");
    const bool fused = which <= 4;
    SCS_REQUIRE(fused ? (b == 4 || b == 8) : (b == 4 || b == 8 || b == 12 || b == 16),
                "scs_debug_panel: kernel %d does not take block width %d", which, b);
    SCS_REQUIRE(n >= 1 && n <= (1 << 24), "scs_debug_panel: n must be in [1, 2^24]");
    SCS_REQUIRE(!fused || (blocks >= 1 && blocks <= PANEL_BLOCKS_MAX), "scs_debug_panel: blocks must be in [1, %d]",
                PANEL_BLOCKS_MAX);
    SCS_REQUIRE((which != 0 && which != 1 && which != 2 && which != 5) || coef_a, "scs_debug_panel: null coefficients");
    SCS_REQUIRE((which != 0 && which != 5) || coef_b, "scs_debug_panel: null coefficients");
    SCS_REQUIRE((which != 0 && which != 6) || theta, "scs_debug_panel: null theta");
    SCS_REQUIRE((which != 2 && which != 4) || dinv, "scs_debug_panel: null dinv");
    SCS_REQUIRE(which != 2 || zt_out, "scs_debug_panel: null zt_out");
    SCS_REQUIRE(which != 4 || (ypart && nseg >= 1 && nseg <= 4), "scs_debug_panel: FINISH 1 sums 1 ... 4 segments");
    SCS_REQUIRE(which == 2 || which == 5 || partial_out, "scs_debug_panel: null partial_out");
    SCS_HIP_CHECK(hipSetDevice(ctx->device));
    t_ctx = ctx;
    hipStream_t s = ctx->stream;
    const int pad = SCS_DEBUG_PANEL_PAD;
    const size_t rows = (size_t)n + pad, ld = (size_t)3 * b;
    const size_t ncoef = which == 1 || which == 2 ? (size_t)(3 * b + 4) * b : ld * b;
    const int nb = which == 5 ? (n + 15) / 16 : (which == 6 ? (n + 255) / 256 : blocks);
    const size_t nper = which <= 1 ? (size_t)3 * b * b + b : (which == 6 ? (size_t)b : ld * ld);
    dbuf dq, daq, du, dca, dcb, dth, ddi, dyp, dpart, dzt;
    SCS_TRY(debug_upload(dq, q, rows * ld * 8, s));
    SCS_TRY(debug_upload(daq, aq, rows * ld * 8, s));
    if (u) SCS_TRY(debug_upload(du, u, rows * 8, s));
    if (coef_a) SCS_TRY(debug_upload(dca, coef_a, ncoef * 8, s));
    if (coef_b) SCS_TRY(debug_upload(dcb, coef_b, ncoef * 8, s));
    if (theta) SCS_TRY(debug_upload(dth, theta, (size_t)b * 8, s));
    if (dinv) SCS_TRY(debug_upload(ddi, dinv, rows * 8, s));
    if (which == 4) SCS_TRY(debug_upload(dyp, ypart, ((size_t)nseg * n + pad) * b * 8, s));
    SCS_TRY(debug_blank(dpart, (size_t)nb * nper * 8, s));
    if (which == 2) SCS_TRY(debug_upload(dzt, zt_out, (size_t)b * rows * 8, s));
    const double *up = u ? du.d() : nullptr;
    if (which == 5) {
        k_rr_update<<<nb, 256, 0, s>>>(dq.d(), b, 3 * b, dca.d(), dcb.d(), n);
        SCS_HIP_CHECK(hipGetLastError());
    } else if (which == 6) {
        k_residual<<<nb, 256, 0, s>>>(dq.d(), daq.d(), b, dth.d(), n, dpart.d());
        SCS_HIP_CHECK(hipGetLastError());
    } else if (b == 4) {
        SCS_TRY(debug_panel_fused<4>(which, n, nb, dq.d(), daq.d(), up, dca.d(), dcb.d(), dth.d(), ddi.d(), dyp.d(),
                                     nseg, dpart.d(), dzt.d(), (int64_t)rows, s));
    } else {
        SCS_TRY(debug_panel_fused<8>(which, n, nb, dq.d(), daq.d(), up, dca.d(), dcb.d(), dth.d(), ddi.d(), dyp.d(),
                                     nseg, dpart.d(), dzt.d(), (int64_t)rows, s));
    }
    SCS_TRY(debug_download(q_out, dq, rows * ld * 8, s));
    SCS_TRY(debug_download(aq_out, daq, rows * ld * 8, s));
    if (which != 2 && which != 5) SCS_TRY(debug_download(partial_out, dpart, (size_t)nb * nper * 8, s));
    if (which == 2) SCS_TRY(debug_download(zt_out, dzt, (size_t)b * rows * 8, s));
    SCS_HIP_CHECK(hipStreamSynchronize(s));
    return SCS_OK;
}


// The loop's decision rules on a scripted sequence of residuals (no device): actions_out[i] = 0 go on, 1 stop
// (the NEXT residual of the script is then taken as the confirmation's: the loop ends there or goes on in double
// precision), 2 renew, 3 = ended converged, 4 = ended not converged; entries behind the end are -1.
extern "C" int scs_debug_loop_policy(double tol, int32_t lowp_mode, double lowp_tol, double lowp_tol2,
                                     int32_t image, int32_t n, const double *residuals, int32_t *actions_out) {
    SCS_REQUIRE(residuals && actions_out && n >= 0, "scs_debug_loop_policy: bad arguments");
    scs_loop_policy p;
    p.tol = tol;
    p.lowp_mode = lowp_mode;
    p.lowp_tol = lowp_tol;
    p.lowp_tol2 = lowp_tol2;
    p.lowp_state = image ? 1 : 0;
    bool ended = false;
    for (int32_t i = 0; i < n; ++i) {
        if (ended) {
            actions_out[i] = -1;
            continue;
        }
        const int a = p.step(residuals[i]);
        actions_out[i] = a;
        if (a == scs_loop_policy::STOP) {
            if (!p.begin_confirmation()) {
                actions_out[i] = residuals[i] <= tol ? 3 : 4;
                ended = true;
            } else if (i + 1 < n) {
                bool conv = false;
                ++i;
                if (p.confirm(residuals[i], &conv)) {
                    actions_out[i] = conv ? 3 : 4;
                    ended = true;
                } else {
                    actions_out[i] = 0;
                }
            }
        }
    }
    return SCS_OK;
}
