// Several start vectors at once, the host side: which kernel a block call runs (block_plan, kfsp_block_plan.h), the launches,
// the buffers and the entry points kfsp_set_block / kfsp_spmm / kfsp_block_* (include/kfsp.h, "several vectors at once";
// DESIGN.md 12).  No kernel lives here: layout and arithmetic are kfsp_block.hip's, and every kernel is reached through the
// selectors of kfsp_block_dev.h.
//
// Options, all read at every block call (block_form) and all OPT-IN - at 0 no launch, allocation, byte or report differs:
// block_box (1: k_spmm_box on single-factor boxes; 2: k_spmm_boxg on every other box), adjoint (the transposed kernels),
// block_small (three launches a step where the single-vector path takes its one-launch pass), block_integral (kfsp_set_block
// keeps a second block J, d_bint, and block_combine the kernels that carry it along), block_dia_code and
// block_dia_code_adjoint beside it (k_spmm_diac / k_spmm_diac_t where the single-vector product reads the coded banded image).
// A target set (the target-set mode of kfsp_set_block) adds the mask d_btgt and the TARGET instantiations of the streaming kernels.
//
// Row partitions (option block_partition; DESIGN.md 12, "Row partitions").  At 0 a context with a communicator, a loop-back
// rank and a group head refuse every block call with -12 (existing callers and tests rely on that refusal).  With 1 the
// forward block product of the stored forms runs on the rank's rows: k_spmm takes local rows and addresses X by global row (SpmmArgs::row0), the source column is made visible
// before every product the way the single-vector path does it - the neighbours' strips of halo * kp doubles into the
// column's own margins (exchange_strips with a width), or an all-gather of L * kp doubles into d_bxg - and in halo mode
// the product is split into an interior launch beside the exchange and one boundary launch (overlapped_product, kfsp_host.h).
// Every block-partial sum is all-reduced before the bookkeeping reads it: k_bfinal sums the rank's partials in its fixed
// order into 2 K staging doubles, one comm_allreduce, k_bfinal again with G = 1 on the reduced sums.  The sequence of
// collectives of a call depends on k, m, the options and the agreed exchange mode only - never on a column's beta, its
// breakdown or the rows a rank owns.  Still refused (-12): option adjoint (the transposed banded product reads the
// neighbour's generator rows) and matrix-free boxes; block_small is not taken (small_path excludes partitions).
#include "kfsp_block_plan.h"
#include "kfsp_boxg_dev.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

int kp_of(int k) { return k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)); }

int64_t spmm_trips(const kfsp_ctx *c) { return product_trips(c->nchunks, c->use_dia); }
// rows a product writes, and rows of a block column (margins included).  Under a row partition a column holds the
// block length L plus one 128-row group whatever the rank owns (every rank sends L rows to an all-gather and its last
// halo rows to a neighbour; the padded half-group of a banded rank writes rows [L, L + 64)), and margins that take the
// neighbours' strips (block_margin: the rule of setup_exchange) - sizes every rank agrees on.
int64_t rows_act(const kfsp_ctx *c) { return spmm_trips(c) * (c->use_dia ? 128 : 64); }
int64_t margin_rows(const kfsp_ctx *c) { return block_margin(c->margin); }
int64_t col_rows(const kfsp_ctx *c) { return (c->use_comm ? c->L + 2 * kChunk : rows_act(c)) + 2 * margin_rows(c); }
// doubles of one block column, and its first row
size_t col_len(const kfsp_ctx *c, int kp) { return (size_t)col_rows(c) * (size_t)kp; }
double *bcol(double *base, const kfsp_ctx *c, int kp, int j) { return base + (size_t)j * col_len(c, kp) + (size_t)margin_rows(c) * kp; }
// the gathered source block of a row partition: nranks * L rows between margins; global row 0
size_t xg_len(const kfsp_ctx *c, int kp) { return (size_t)(c->L * c->nranks + 2 * margin_rows(c)) * (size_t)kp; }
double *xg_row0(const kfsp_ctx *c, int kp) { return c->d_bxg.p + (size_t)margin_rows(c) * kp; }
// the context whose block state answers for ctx: rank 0 of a group head, else ctx itself
kfsp_ctx *lead(kfsp_ctx *c) { return c->group ? group_rank0(c) : c; }
// 16-byte pairs the streaming kernels cover: the rows of the SELL-padded block, like act_pairs
int64_t red_pairs(const kfsp_ctx *c, int kp) { return c->nchunks * kChunk * (int64_t)kp / 2; }

int spmm_grid(const kfsp_ctx *c) { return product_grid(spmm_trips(c), c->opt_grid, 1024); }

// grid of the streaming kernels over a block column
int flat_grid(const kfsp_ctx *c, int kp) { return vec_grid(red_pairs(c, kp), c->opt_vgrid); }

// A streaming kernel over a block column of width kp: flat_grid workgroups on the context's stream, the pairs and kp / 2
// in front of the kernel's own arguments.  Returns the grid: that many block partials.
template <class Kern, class... Args>
int launch_flat(kfsp_ctx *ctx, int kp, Kern kern, Args... args)
{
    const int g = flat_grid(ctx, kp);
    hipLaunchKernelGGL(kern, dim3(g), dim3(kBlock), 0, ctx->stream, red_pairs(ctx, kp), kp / 2, args...);
    return g;
}

d2 *pairs(double *p) { return reinterpret_cast<d2 *>(p); }
const d2 *pairs(const double *p) { return reinterpret_cast<const d2 *>(p); }

// grid of the pack / unpack kernels over `items` elements
int pack_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (items + kBlock - 1) / kBlock)); }

// col <- D col for a block column of width kp (row 0 at col; target sets: the row of pair i is i >> kp_index(kp));
// nothing without a set
void target_zero(kfsp_ctx *ctx, int kp, double *col)
{
    if (!ctx->blk_tgt) return;
    hipLaunchKernelGGL(block_kernels().target_zero, dim3(flat_grid(ctx, kp)), dim3(kBlock), 0, ctx->stream, red_pairs(ctx, kp), kp_index(kp),
                       ctx->d_btgt.p, pairs(col));
}

// The refusal the plan makes at this width alone (a box whose entries reach too far for the single-factor kernels).  The
// options are read at every call: a block set under the generic kernels may meet the single-factor ones later.
int box_reach_check(kfsp_ctx *c, int kp)
{
    const BlockPlan p = block_plan(block_form(c, kp));
    return p.where == kRefuseWidth ? fail(c, p.code, p.why) : 0;
}

// One launch of a kernel that stages a table image of `image_bytes` into dynamic LDS.  Every workgroup copies the image
// first, so no more workgroups are launched than are resident at once (the rule of the single-vector product,
// run_product): the runtime says how many fit, asked once per family, width and variant (blk_staged_occ).  The
// reductions of the box kernels reuse the image's LDS: never less than 4 kp doubles of it; the coded banded kernels keep
// their reduction scratch apart (BlockPlan::lds_shared).  staged_lds: the dynamic LDS of the launch.  Returns the grid.
size_t staged_lds(const BlockPlan &p, size_t image_bytes, int kp) { return p.lds_shared ? std::max<size_t>(image_bytes, (size_t)4 * kp * sizeof(double)) : image_bytes; }

template <class... Args>
int launch_staged(kfsp_ctx *ctx, const BlockPlan &p, int kp, bool dots, int64_t trips, size_t lds, void (*kern)(Args...), const Args &...args)
{
    int &occ = ctx->blk_staged_occ[p.staged][kp_index(kp)][dots ? 1 : 0];
    if (occ == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kBlock, lds) != hipSuccess || occ < 1)) occ = 1;
    const int g = product_grid(trips, ctx->opt_grid, std::min<int64_t>(1024, (int64_t)256 * occ));
    hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(kBlock), lds, ctx->stream, args...);
    return g;
}

// What a product leaves for kfsp_block_info, the one place that writes it: how the source travelled (block_exchange_mode)
// and - while option block_dia_code is on - whether a coded kernel ran (9, its dynamic LDS) or not (0, 0); with the option
// off nothing here writes those two slots (the one-launch small pass fills them).
void record_product(kfsp_ctx *ctx, int exchange, bool coded = false, size_t lds = 0)
{
    ctx->blk_info[kInfoExchange] = exchange;
    if (!ctx->opt_block_dia_code) return;
    ctx->blk_info[kInfoFmt] = coded ? 9 : 0;
    ctx->blk_info[kInfoLdsBytes] = coded ? (int64_t)lds : 0;
}
// ... and the direction, by the calls that report one (kfsp_spmm, kfsp_spmm_bench, block_arnoldi - not the flux call)
void record_direction(kfsp_ctx *ctx) { ctx->blk_info[kInfoAdjoint] = ctx->opt_adjoint ? 1 : 0; }

// k_spmm, the one family that runs under a row partition: the source is made visible first - the strips into x's own
// margins, or all blocks gathered into d_bxg - unless x_global says that x is row 0 of a whole block every rank already
// holds (kfsp_spmm).
int spmm_stored(kfsp_ctx *ctx, const BlockPlan &p, int kp, SpmmArgs &a, const double *x, bool dots, int *G, bool x_global)
{
    hipStream_t st = ctx->stream;
    const int g = *G;
    const SpmmFn kern = spmm_kernel(kp, p.fmt, dots, ctx->use_comm);
    auto launch = [&](int grid) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, a); };
    const bool strips = ctx->use_comm && !x_global && ctx->use_halo;
    const ProductSplit ps = strips ? product_split(ctx->halo, ctx->L, a.trips, ctx->use_dia ? 128 : 64, ctx->opt_overlap) : ProductSplit{0, 0, false};
    const int mode = block_exchange_mode(ctx->use_comm, x_global, ctx->use_halo, ps.split, ctx->comm_stream != nullptr);
    record_product(ctx, mode);
    if (ctx->use_comm) a.row0 = ctx->row0;
    if (mode == 2) {
        if (int rc = comm_allgather(ctx, x, xg_row0(ctx, kp), (size_t)ctx->L * kp, st)) return rc;
        a.X = xg_row0(ctx, kp);
    }
    if (mode == 1 || mode == 5) a.X = x - (size_t)ctx->row0 * kp;      // global row g lies at x[(g - row0) * kp]
    if (mode == 1)
        if (int rc = exchange_strips(ctx, x, st, kp)) return rc;
    if (mode != 5) {
        launch(g);
        return 0;
    }
    // the strips travel on the communication stream while the interior trips run (overlapped_product, kfsp_host.h)
    a.trip_order = nullptr;
    auto launch_range = [&](int64_t begin, int64_t end, int64_t split, int64_t jump, int grid, int used) {
        a.part = ctx->d_bpart.p + (size_t)used * K;
        a.trip_begin = begin;
        a.trip_end = end;
        a.trip_split = split;
        a.trip_jump = jump;
        launch(grid);
        return grid;
    };
    return overlapped_product(ctx, ps, a.trips, x, kp, 1024, launch_range, G);
}

// Y = A X, or A^T X under option adjoint (block columns of width kp); dots: partials of ua . Y and ub . Y in *G slots.
// x: row 0 of the source column.  The plan says which family runs, or refuses - before any collective.  The transposed
// kernels take the grid of the forward product of the same form, the families that stage an image theirs from launch_staged.
int spmm(kfsp_ctx *ctx, int kp, const double *x, double *Y, const double *ua, const double *ub, bool dots, int *G, bool x_global = false)
{
    const BlockPlan p = block_plan(block_form(ctx, kp));
    if (p.code) return fail(ctx, p.code, p.why);
    SpmmArgs a{};                                              // (no box tables, row0 = 0, trips from 0 without a jump)
    generator_args(ctx, a.A, a.D);
    a.X = x;
    a.Y = Y;
    a.ua = ua;
    a.ub = ub;
    a.part = ctx->d_bpart.p;
    a.trips = a.trip_end = spmm_trips(ctx);
    a.trip_order = ctx->trip_order_n == a.trips ? ctx->d_trip_order.p : nullptr;
    a.rows_red = ctx->nchunks * kChunk;
    a.trip_split = INT64_MAX;
    if (ctx->box.on) {                                         // the table image, and the single-factor descriptor behind it
        a.box_tab = ctx->d_box.p;
        a.box_ntab = ctx->box.dev.ntab;
        a.box_fast = reinterpret_cast<const BoxFast *>(ctx->d_box.p + (ctx->box.lds_bytes / sizeof(double)));
    }
    const int g = *G = spmm_grid(ctx);
    size_t lds = 0;
    auto launch = [&](auto kern, const auto &...args) { hipLaunchKernelGGL(kern, dim3(g), dim3(kBlock), 0, ctx->stream, args...); };
    auto staged = [&](size_t image_bytes, auto kern, const auto &...args) {
        lds = staged_lds(p, image_bytes, kp);
        *G = launch_staged(ctx, p, kp, dots, a.trips, lds, kern, args...);
    };
    BoxAdjDev b;
    DiaCodeDev C;
    EllAdjDev e;
    switch (p.kernel) {
    case kBlockBox: staged(ctx->box.lds_bytes, spmm_box_kernel(kp, ctx->box.dev.pad, dots), a); break;
    case kBlockBoxT:
        box_adj_build(ctx->box.dev, b);                        // (it builds: the plan asked)
        staged(ctx->box.lds_bytes, spmm_box_t_kernel(kp, ctx->box.dev.pad, dots), a, b);
        break;
    case kBlockBoxg:
    case kBlockBoxgT:                                          // the head and the factor tables only, the box descriptor by value
        a.box_ntab = box_generic_image(ctx->box.dev);
        a.box_fast = nullptr;
        staged((size_t)a.box_ntab * sizeof(double), p.kernel == kBlockBoxg ? spmm_boxg_kernel(kp, dots) : spmm_boxg_t_kernel(kp, dots),
               BoxgArgs{a, ctx->box.dev});
        break;
    case kBlockDiac:
    case kBlockDiacT:                                          // the dictionaries
        dia_code_args(ctx, C);
        staged((size_t)C.doff[ctx->nd] * sizeof(double),
               (p.kernel == kBlockDiac ? spmm_diac_kernel : spmm_diac_t_kernel)(kp, ctx->dia_code_w, ctx->dia_code_rec, dots), a, C);
        break;
    case kBlockT: launch(spmm_t_kernel(kp, dots), a); break;
    case kBlockEllT:
        ell_adj_args(ctx, e);
        launch(spmm_ell_t_kernel(kp, dots), a, e);
        break;
    default: return spmm_stored(ctx, p, kp, a, x, dots, G, x_global);
    }
    record_product(ctx, 0, p.kernel == kBlockDiac || p.kernel == kBlockDiacT, lds);
    return 0;
}

// The scalar stage behind a producer of G block partials.  One rank: one launch, as ever.  Row partition: the rank's
// column sums in the same fixed order, one all-reduce of the 2 K sums, the bookkeeping on the reduced sums - on every
// rank, whatever its columns did.
int finalize(kfsp_ctx *ctx, int stage, int j, int kp, int G, double break_tol = 0.0)
{
    const int64_t off1 = (int64_t)kMaxGrid * K;
    if (!ctx->use_comm) {
        hipLaunchKernelGGL(block_kernels().finish, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, G, ctx->d_bpart.p, off1, ctx->d_bscal.p, break_tol,
                           (double *)nullptr);
        return 0;
    }
    double *sums = ctx->d_bpart.p + (size_t)2 * kMaxGrid * K;
    hipLaunchKernelGGL(block_kernels().finish, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, G, ctx->d_bpart.p, off1, ctx->d_bscal.p, break_tol, sums);
    if (int rc = comm_allreduce(ctx, sums, 2 * K, false, ctx->stream)) return rc;
    hipLaunchKernelGGL(block_kernels().finish, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, 1, sums, (int64_t)K, ctx->d_bscal.p, break_tol,
                       (double *)nullptr);
    return 0;
}

// the scalar and partial buffers of the block path
int ensure_scalars(kfsp_ctx *ctx)
{
    HIP_TRY(ctx->d_bscal.reserve(kScal, true));
    HIP_TRY(ctx->d_bpart.reserve((size_t)2 * kMaxGrid * K + 2 * K, true));    // + the 2 K column sums a row partition all-reduces
    return 0;
}

// `need` doubles in a buffer of block columns laid out for width kp (*laid): zeroed when allocated and whenever the
// width changes - margins, and the rows behind n, must read 0
int reserve_for_width(kfsp_ctx *ctx, DevBuf<double> &buf, int *laid, size_t need, int kp)
{
    if (need > buf.cap) {
        buf.release();
        HIP_TRY(buf.reserve(need, true));
        *laid = kp;
    }
    if (*laid != kp) {
        HIP_TRY(hipMemsetAsync(buf.p, 0, buf.cap * sizeof(double), ctx->stream));
        *laid = kp;
    }
    return 0;
}

// ncols block columns of width kp in d_bv; under a row partition also what it exchanges block columns through - the strip
// buffer at block width and the gathered block; and the scalars
int ensure_basis(kfsp_ctx *ctx, int kp, int ncols)
{
    if (int rc = reserve_for_width(ctx, ctx->d_bv, &ctx->bv_kp, (size_t)ncols * col_len(ctx, kp), kp)) return rc;
    if (ctx->use_comm) {
        if (ctx->use_halo) HIP_TRY(ctx->d_strip.reserve((size_t)(2 * ctx->halo) * (size_t)(ctx->nranks + 1) * (size_t)kp, true));
        if (int rc = reserve_for_width(ctx, ctx->d_bxg, &ctx->bxg_kp, xg_len(ctx, kp), kp)) return rc;
    }
    return ensure_scalars(ctx);
}

// host column-major (caller's order) -> zeroed block column dst (width kp, internal order).  One rank, and the whole
// block every rank of a partition holds (whole: kfsp_spmm's X into d_bxg): n rows through the permutation.  A rank's
// own rows (kfsp_set_block under a communicator): column by column the way kfsp_set_vector takes a vector
// (upload_states: under the internal state order one all-gather per column, on every rank), then packed as they lie.
int upload_block(kfsp_ctx *ctx, int k, int kp, int64_t ld, const double *W, double *col0, bool whole = false)
{
    hipStream_t st = ctx->stream;
    if (ctx->use_comm && !whole) {
        const int64_t nl = ctx->nloc, L = ctx->L;
        HIP_TRY(ctx->d_bstage.reserve((size_t)L * k, false));
        HIP_TRY(hipMemsetAsync(col0 - (size_t)margin_rows(ctx) * kp, 0, col_len(ctx, kp) * sizeof(double), st));
        for (int c = 0; c < k; ++c)
            if (int rc = upload_states(ctx, W ? W + (size_t)c * ld : W, ctx->d_bstage.p + (size_t)c * L, nl)) return rc;
        hipLaunchKernelGGL(block_kernels().pack, dim3(pack_grid(nl * kp)), dim3(kBlock), 0, st, nl, k, kp, ctx->d_bstage.p, L, (const int32_t *)nullptr, col0);
        return 0;
    }
    const int64_t n = ctx->n;
    HIP_TRY(ctx->d_bstage.reserve((size_t)n * k, false));
    if (whole) HIP_TRY(hipMemsetAsync(ctx->d_bxg.p, 0, xg_len(ctx, kp) * sizeof(double), st));
    else HIP_TRY(hipMemsetAsync(col0 - (size_t)margin_rows(ctx) * kp, 0, col_len(ctx, kp) * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_bstage.p, (size_t)n * sizeof(double), W, (size_t)ld * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(block_kernels().pack, dim3(pack_grid(n * kp)), dim3(kBlock), 0, st, n, k, kp, ctx->d_bstage.p, n, ctx->perm_on ? ctx->d_perm.p : nullptr, col0);
    return 0;
}

// ... and back; under a communicator the rank's rows column by column through download_states (L rows staged per
// column: that is what its all-gather sends)
int download_block(kfsp_ctx *ctx, int k, int kp, const double *col0, int64_t ld, double *W)
{
    hipStream_t st = ctx->stream;
    if (ctx->use_comm) {
        const int64_t L = ctx->L;
        HIP_TRY(ctx->d_bstage.reserve((size_t)L * k, false));
        hipLaunchKernelGGL(block_kernels().unpack, dim3(pack_grid(L * k)), dim3(kBlock), 0, st, L, k, kp, col0, (const int32_t *)nullptr, ctx->d_bstage.p, L);
        for (int c = 0; c < k; ++c)
            if (int rc = download_states(ctx, ctx->d_bstage.p + (size_t)c * L, W ? W + (size_t)c * ld : W, ctx->nloc)) return rc;
        return 0;
    }
    const int64_t n = ctx->n;
    HIP_TRY(ctx->d_bstage.reserve((size_t)n * k, false));
    hipLaunchKernelGGL(block_kernels().unpack, dim3(pack_grid(n * k)), dim3(kBlock), 0, st, n, k, kp, col0, ctx->perm_on ? ctx->d_iperm.p : nullptr, ctx->d_bstage.p, n);
    HIP_TRY(hipMemcpy2DAsync(W, (size_t)ld * sizeof(double), ctx->d_bstage.p, (size_t)n * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)k, hipMemcpyDeviceToHost, st));
    return 0;
}

// the block path's fence at the C boundary
template <class F>
int guarded(kfsp_ctx *ctx, F &&body) { return no_throw(ctx, body, "exception inside the block path"); }

}  // namespace

void block_reset(kfsp_ctx *ctx)
{
    for (DevBuf<double> *b : {&ctx->d_blk, &ctx->d_bv, &ctx->d_bstage, &ctx->d_bscal, &ctx->d_bpart, &ctx->d_bxg, &ctx->d_bint, &ctx->d_bcj,
                              &ctx->d_bhit, &ctx->d_bhsum})
        b->release();
    ctx->d_btgt.release();
    reset_block_state(ctx);
}

// The plan's refusal, if it is one that every block call makes before anything else.  A group head answers with its rank 0.
int block_supported(kfsp_ctx *ctx)
{
    if (ctx->group) {
        kfsp_ctx *r0 = group_rank0(ctx);
        if (!r0 || !r0->opt_block_partition) return fail(ctx, -12, kBlockPartMsg);
        const int rc = block_supported(r0);
        if (rc) ctx->err = std::string(r0->err);
        return rc;
    }
    const BlockPlan p = block_plan(block_form(ctx, 2));
    return p.where == kRefuseContext ? fail(ctx, p.code, p.why) : 0;
}

int block_shape(kfsp_ctx *ctx, int *k, int64_t *n)
{
    *k = lead(ctx)->blk_k;
    *n = ctx->n;
    return 0;
}

int block_mmax(kfsp_ctx *ctx)
{
    ctx = lead(ctx);
    return (int)(ctx->v_mmax ? std::min(ctx->v_mmax, ctx->opt_mmax) : ctx->opt_mmax);
}

int block_integral(kfsp_ctx *ctx, int *on)
{
    const kfsp_ctx *l = lead(ctx);
    *on = l->opt_block_integral != 0;
    if (*on && !l->blk_int)
        return fail(ctx, -1, "option block_integral is on but the resident block has no integral beside it: set the option "
                             "before kfsp_set_block");
    return 0;
}

int block_begin(kfsp_ctx *ctx, int m, double *beta)
{
    if (ctx->group) return group_block_begin(ctx, m, beta);
    PhaseTimer timer(ctx, KFSP_T_BEGIN);
    HIP_TRY(hipSetDevice(ctx->device));
    const int kp = ctx->blk_kp;
    if (int rc = ensure_basis(ctx, kp, m + 2)) return rc;
    ctx->blk_begin_m = m;
    if (small_path(ctx)) {
        hipLaunchKernelGGL(block_kernels().begin_small, dim3(kp), dim3(kSmallBlock), 0, ctx->stream, (int)(ctx->nchunks * kChunk), kp,
                           bcol(ctx->d_blk.p, ctx, kp, 0), bcol(ctx->d_bv.p, ctx, kp, 0), ctx->d_bscal.p);
        ctx->blk_info[kInfoBeginLaunches] = 1;
    } else {
        const int g = launch_flat(ctx, kp, block_kernels().copy_nrm[ctx->blk_tgt], pairs(bcol(ctx->d_blk.p, ctx, kp, 0)),
                                  pairs(bcol(ctx->d_bv.p, ctx, kp, 0)), ctx->d_bpart.p, ctx->d_btgt.p, kp_index(kp));
        if (int rc = finalize(ctx, kFinBegin, 1, kp, g)) return rc;
        ctx->blk_info[kInfoBeginLaunches] = 2;
    }
    HIP_TRY(hipMemcpyAsync(beta, ctx->d_bscal.p + kNRM + K, K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int block_arnoldi(kfsp_ctx *ctx, int m, double break_tol, double *hb, double *nrm, int *brk, double *avnorm)
{
    if (ctx->group) return group_block_arnoldi(ctx, m, break_tol, hb, nrm, brk, avnorm);
    PhaseTimer timer(ctx, KFSP_T_ARNOLDI);
    HIP_TRY(hipSetDevice(ctx->device));
    const int kp = ctx->blk_kp;
    if (int rc = ensure_basis(ctx, kp, m + 2)) return rc;
    hipStream_t st = ctx->stream;
    double *V = ctx->d_bv.p;
    auto u = [&](int j) { return bcol(V, ctx, kp, j - 1); };   // u_j, 1-based
    const bool small = small_path(ctx);
    // target set: the update pass and the AVNORM norm mask what the raw product wrote (null: the kernels as they were)
    const uint8_t *tgt = ctx->blk_tgt ? ctx->d_btgt.p : nullptr;
    const int sh = kp_index(kp);
    ctx->blk_info[kInfoOneLaunch] = small ? 1 : 0;
    ctx->blk_info[kInfoFmt] = ctx->blk_info[kInfoLdsBytes] = 0;
    record_direction(ctx);
    ctx->blk_info[kInfoArnoldiLaunches] = small ? 1 : 4 * m + 3;
    if (small) {
        SmallArnoldiArgs sa;
        generator_args(ctx, sa.A, sa.D);
        sa.V = nullptr;
        sa.ldv = (int64_t)col_len(ctx, kp);
        sa.nact = ctx->nchunks * kChunk;
        sa.m = m;
        sa.jold = 1;
        sa.sq = sa.gfin = sa.Hd = nullptr;
        sa.break_tol = break_tol;
        sa.brk_flag = nullptr;
        sa.slots = ctx->use_dia ? 0 : ctx->slots;
        double *sc = ctx->d_bscal.p;
        const SmallBlockArgs sb{u(1), kp, ctx->blk_k, K, sc + kHB, sc + kNRM, sc + kBRK, sc + kAVN, sc + kSQ1};
        int fmt = 0;
        size_t lds = 0;
        if (const int e = launch_barnoldi_small(sa, sb, kp, ctx->use_dia, ctx->opt_small_lds ? ctx->lds_per_block : 0, st, &fmt, &lds))
            return hip_fail(ctx, (hipError_t)e, "hipFuncSetAttribute(k_barnoldi_small)");
        ctx->blk_info[kInfoFmt] = fmt;
        ctx->blk_info[kInfoLdsBytes] = (int64_t)lds;
    }
    for (int j = 1; j <= m && !small; ++j) {
        int g = 0;
        if (int rc = spmm(ctx, kp, u(j), u(j + 1), j >= 2 ? u(j - 1) : nullptr, u(j), true, &g)) return rc;
        if (int rc = finalize(ctx, kFinDots, j, kp, g)) return rc;
        const int gv = launch_flat(ctx, kp, block_kernels().ortho[tgt != nullptr], pairs(u(j + 1)), pairs(j >= 2 ? u(j - 1) : nullptr),
                                   pairs(u(j)), ctx->d_bscal.p + kCO, ctx->d_bpart.p, tgt, sh);
        if (int rc = finalize(ctx, kFinNorm, j, kp, gv, break_tol)) return rc;
    }
    if (!small) {
        // the extra product for AVNORM (:261-263) into the scratch column
        int g = 0;
        if (int rc = spmm(ctx, kp, u(m + 1), u(m + 2), nullptr, nullptr, false, &g)) return rc;
        // (two launches for a const: the set's instantiation writes D z back)
        const int gv = tgt ? launch_flat(ctx, kp, block_kernels().norm_target, pairs(u(m + 2)), ctx->d_bpart.p, tgt, sh)
                           : launch_flat(ctx, kp, block_kernels().norm, pairs(u(m + 2)), ctx->d_bpart.p, tgt, sh);
        if (int rc = finalize(ctx, kFinAvn, m + 1, kp, gv)) return rc;
    }
    std::vector<double> h((size_t)kScal);
    HIP_TRY(hipMemcpyAsync(h.data(), ctx->d_bscal.p, (size_t)kCMB * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(hb, h.data() + kHB, (size_t)(kMMax + 2) * 3 * K * sizeof(double));
    std::memcpy(nrm, h.data() + kNRM, (size_t)(kMMax + 3) * K * sizeof(double));
    std::memcpy(avnorm, h.data() + kAVN, K * sizeof(double));
    for (int c = 0; c < K; ++c) brk[c] = (int)h[(size_t)kBRK + c];
    return 0;
}

int block_combine(kfsp_ctx *ctx, int mx, const double *coef, double *wsum)
{
    if (ctx->group) return group_block_combine(ctx, mx, coef, wsum);
    PhaseTimer timer(ctx, KFSP_T_COMBINE);
    HIP_TRY(hipSetDevice(ctx->device));
    const int kp = ctx->blk_kp;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(ctx->d_bscal.p + kCMB, coef, (size_t)mx * K * sizeof(double), hipMemcpyHostToDevice, st));
    // option block_integral: the same launches with the kernels that carry J along; rows [mx, 2 mx) of coef are J's table
    const bool integral = ctx->opt_block_integral != 0, small = small_path(ctx);
    if (integral) {
        if (!ctx->blk_int) return fail(ctx, -1, "option block_integral: no integral resident (set the option before kfsp_set_block)");
        HIP_TRY(hipMemcpyAsync(ctx->d_bcj.p, coef + (size_t)mx * K, (size_t)mx * K * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const double *U = bcol(ctx->d_bv.p, ctx, kp, 0), *cw = ctx->d_bscal.p + kCMB, *cj = ctx->d_bcj.p;
    double *w = bcol(ctx->d_blk.p, ctx, kp, 0), *J = integral ? bcol(ctx->d_bint.p, ctx, kp, 0) : nullptr;
    const int64_t ldc = (int64_t)col_len(ctx, kp);
    const int clamp = ctx->opt_block_clamp ? 1 : 0;
    if (small) {
        const int nact = (int)(ctx->nchunks * kChunk);
        if (integral) hipLaunchKernelGGL(block_kernels().combine_small_int, dim3(kp), dim3(kSmallBlock), 0, st, nact, kp, U, ldc, mx, cw, cj, w, J, ctx->d_bscal.p, clamp);
        else hipLaunchKernelGGL(block_kernels().combine_small, dim3(kp), dim3(kSmallBlock), 0, st, nact, kp, U, ldc, mx, cw, w, ctx->d_bscal.p, clamp);
    } else {
        const int g = integral ? launch_flat(ctx, kp, block_kernels().combine_int, U, ldc, mx, cw, cj, pairs(w), pairs(J), ctx->d_bpart.p, clamp)
                               : launch_flat(ctx, kp, block_kernels().combine, U, ldc, mx, cw, pairs(w), ctx->d_bpart.p, clamp);
        if (int rc = finalize(ctx, kFinWsum, 0, kp, g)) return rc;
    }
    ctx->blk_info[kInfoCombineLaunches] = small ? 1 : 2;
    HIP_TRY(hipMemcpyAsync(wsum, ctx->d_bscal.p + kWS, K * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace kfsp

using namespace kfsp;

extern "C" {

// Target sets travel through three existing entry points (the exported surface of the library is pinned): option
// "block_target" is the call mode - 1: kfsp_set_block takes flags, 2: kfsp_block_info reports the set, 3: kfsp_block_begin
// is the flux into it (include/kfsp.h, TARGET SETS).  A group head answers with the mode of its rank 0.
static int set_block_target(kfsp_ctx *ctx, int32_t k, int64_t n, int64_t ldf, const double *F);
static int block_target_info(kfsp_ctx *ctx, int64_t *v);
static int block_hit(kfsp_ctx *ctx, int32_t which, double *out);
static int64_t target_mode(kfsp_ctx *ctx)
{
    const kfsp_ctx *l = lead(ctx);
    return l ? l->opt_block_target : 0;
}

// what the calls on a resident block share: a context that takes blocks and holds one
static int block_call_ok(kfsp_ctx *ctx, const char *none = "no block resident (none was set, or the generator changed since)")
{
    if (int rc = block_supported(ctx)) return rc;
    if (lead(ctx)->blk_k == 0) return fail(ctx, -1, none);
    return 0;
}

// n, ldw and W of kfsp_set_block / kfsp_get_block.  A rank's arguments are its own (a caller that gets them wrong on one
// rank only leaves the others waiting, as in kfsp_set_vector); a rank without rows may pass no W.
static int block_args_ok(kfsp_ctx *ctx, int64_t n, int64_t ldw, const double *W)
{
    if (n != (ctx->use_comm ? ctx->nloc : ctx->n))
        return fail(ctx, -3, ctx->use_comm ? "n is not this rank's block size" : "n is not the number of states of the generator");
    if (ldw < n) return fail(ctx, -4, "ldw < n");
    if (!W && !(ctx->use_comm && n == 0)) return fail(ctx, -5, "null W");
    return 0;
}

int kfsp_set_block(kfsp_ctx *ctx, int32_t k, int64_t n, int64_t ldw, const double *W)
{
    if (!ctx) return -1;
    if (target_mode(ctx) == 1) return set_block_target(ctx, k, n, ldw, W);
    return guarded(ctx, [&]() -> int {
        if (int rc = block_supported(ctx)) return rc;
        if (k < 1 || k > kBlockMaxK) return fail(ctx, -2, "k out of range (1 <= k <= 16)");
        if (ctx->group) return group_set_block(ctx, k, n, ldw, W);
        if (int rc = block_args_ok(ctx, n, ldw, W)) return rc;
        HIP_TRY(hipSetDevice(ctx->device));
        const int kp = kp_of(k);
        if (int rc = box_reach_check(ctx, kp)) return rc;
        ctx->blk_k = ctx->blk_begin_m = 0;
        ctx->blk_int = false;
        if (ctx->blk_kp != kp || ctx->d_blk.cap < col_len(ctx, kp)) {
            ctx->d_blk.release();
            ctx->d_bint.release();
            HIP_TRY(ctx->d_blk.reserve(col_len(ctx, kp), false));
        }
        // J (option block_integral) lives and dies with the block: the same shape, +0.0 everywhere
        if (ctx->opt_block_integral) {
            HIP_TRY(ctx->d_bint.reserve(col_len(ctx, kp), false));
            HIP_TRY(hipMemsetAsync(ctx->d_bint.p, 0, col_len(ctx, kp) * sizeof(double), ctx->stream));
            HIP_TRY(ctx->d_bcj.reserve((size_t)(kMMax + 3) * K, true));
        } else {
            ctx->d_bint.release();
            ctx->d_bcj.release();
        }
        ctx->blk_kp = kp;
        if (int rc = upload_block(ctx, k, kp, ldw, W, bcol(ctx->d_blk.p, ctx, kp, 0))) return rc;
        target_zero(ctx, kp, bcol(ctx->d_blk.p, ctx, kp, 0));       // a target set: the block is D W from the start
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->blk_k = k;
        ctx->blk_int = ctx->opt_block_integral != 0;
        return 0;
    });
}

int kfsp_get_block(kfsp_ctx *ctx, int32_t k, int64_t n, int64_t ldw, double *W)
{
    if (!ctx) return -1;
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx)) return rc;
        if (k != lead(ctx)->blk_k) return fail(ctx, -2, "k is not the number of columns of the resident block");
        // option block_integral = 2: the answer is J, by the route W takes
        const bool want_j = lead(ctx)->opt_block_integral == 2;
        if (want_j)
            if (int on = 0; int rc = block_integral(ctx, &on)) return rc;
        if (ctx->group) return group_get_block(ctx, k, n, ldw, W);
        if (int rc = block_args_ok(ctx, n, ldw, W)) return rc;
        HIP_TRY(hipSetDevice(ctx->device));
        if (int rc = download_block(ctx, k, ctx->blk_kp, bcol(want_j ? ctx->d_bint.p : ctx->d_blk.p, ctx, ctx->blk_kp, 0), ldw, W)) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return 0;
    });
}

int kfsp_spmm(kfsp_ctx *ctx, int32_t k, int64_t ld, const double *X, double *Y)
{
    if (!ctx) return -1;
    return guarded(ctx, [&]() -> int {
        if (int rc = block_supported(ctx)) return rc;
        if (k < 1 || k > kBlockMaxK) return fail(ctx, -2, "k out of range (1 <= k <= 16)");
        if (ld < ctx->n) return fail(ctx, -3, "ld < n");
        if (!X) return fail(ctx, -4, "null X");
        if (ctx->group) return group_spmm(ctx, k, ld, X, Y);
        if (!Y && !(ctx->use_comm && ctx->nloc == 0)) return fail(ctx, -5, "null Y");
        HIP_TRY(hipSetDevice(ctx->device));
        const int kp = kp_of(k);
        if (int rc = box_reach_check(ctx, kp)) return rc;
        if (int rc = ensure_basis(ctx, kp, 2)) return rc;
        // under a row partition X is the whole block on every rank (the kfsp_spmv convention): it goes to the gathered
        // block buffer, global row 0 first, and no exchange follows
        const bool whole = ctx->use_comm;
        double *x = whole ? xg_row0(ctx, kp) : bcol(ctx->d_bv.p, ctx, kp, 0), *y = bcol(ctx->d_bv.p, ctx, kp, 1);
        if (int rc = upload_block(ctx, k, kp, ld, X, x, whole)) return rc;
        target_zero(ctx, kp, x);                                    // a target set: Y = D A D X
        int g = 0;
        if (int rc = spmm(ctx, kp, x, y, nullptr, nullptr, false, &g, whole)) return rc;
        target_zero(ctx, kp, y);
        record_direction(ctx);
        if (int rc = download_block(ctx, k, kp, y, ld, Y)) return rc;
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return 0;
    });
}

int kfsp_block_begin(kfsp_ctx *ctx, int32_t m, double *beta)
{
    if (!ctx) return -1;
    if (target_mode(ctx) == 3) return block_hit(ctx, m, beta);
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx)) return rc;
        if (m < 1 || m > kMMax) return fail(ctx, -2, "bad m (need 1 <= m <= 100)");
        if (m > block_mmax(ctx)) return fail(ctx, -2, "m exceeds option m_max");
        if (!beta) return fail(ctx, -3, "null beta");
        return block_begin(ctx, m, beta);
    });
}

int kfsp_block_arnoldi(kfsp_ctx *ctx, int32_t m, double break_tol, double *hb, double *nrm, int32_t *brk, double *avnorm)
{
    if (!ctx) return -1;
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx)) return rc;
        if (m < 1 || m > kMMax) return fail(ctx, -2, "bad m (need 1 <= m <= 100)");
        if (m > block_mmax(ctx)) return fail(ctx, -2, "m exceeds option m_max");
        if (lead(ctx)->blk_begin_m == 0) return fail(ctx, -3, "no kfsp_block_begin since the block was set");
        if (m > lead(ctx)->blk_begin_m) return fail(ctx, -2, "m exceeds the m of kfsp_block_begin (the basis is laid out for that one)");
        if (!hb || !nrm || !brk || !avnorm) return fail(ctx, -4, "null output");
        return block_arnoldi(ctx, m, break_tol, hb, nrm, brk, avnorm);
    });
}

int kfsp_block_combine(kfsp_ctx *ctx, int32_t mx, const double *coef, double *wsum)
{
    if (!ctx) return -1;
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx)) return rc;
        if (lead(ctx)->blk_begin_m == 0) return fail(ctx, -3, "no kfsp_block_begin since the block was set");
        if (mx < 1 || mx > lead(ctx)->blk_begin_m + 2) return fail(ctx, -2, "bad mx (need 1 <= mx <= m + 2 of kfsp_block_begin)");
        if (!coef) return fail(ctx, -4, "null coef");
        if (!wsum) return fail(ctx, -5, "null wsum");
        if (int on = 0; int rc = block_integral(ctx, &on)) return rc;
        return block_combine(ctx, mx, coef, wsum);
    });
}

int kfsp_block_info(kfsp_ctx *ctx, int64_t *v)
{
    if (!ctx) return -1;
    if (!v) return fail(ctx, -2, "null v");
    if (target_mode(ctx) == 2) return block_target_info(ctx, v);
    if (ctx->group) return group_block_info(ctx, v);
    for (int i = 0; i < kInfoSlots; ++i) v[i] = ctx->blk_info[i];
    return 0;
}

static int set_block_target(kfsp_ctx *ctx, int32_t k, int64_t n, int64_t ldf, const double *F)
{
    (void)ldf;                                   // one column: the leading dimension is never used
    return guarded(ctx, [&]() -> int {
        // refused from what every rank shares, before anything else (block_supported's rule)
        if (ctx->group || ctx->use_comm || ctx->nranks > 1 || ctx->loop || ctx->comm)
            return fail(ctx, -12, "kfsp_set_block under block_target = 1 (a target set): not with a row partition (communicator, loop-back rank or group context), "
                                  "with or without option block_partition");
        if (ctx->ldv == 0) return fail(ctx, -1, "no matrix set");
        const bool clear = !F || n == 0;
        if (!clear && k != 1) return fail(ctx, -2, "block_target = 1: the flags are ONE column (k = 1)");
        if (!clear && n != ctx->n) return fail(ctx, -2, "block_target = 1: n is not the number of states of the generator");
        HIP_TRY(hipSetDevice(ctx->device));
        // the resident block is W, not D W (or D' W): it goes with the old set, and its J, as when the generator changes
        block_reset(ctx);
        if (clear) return 0;
        const int64_t rows = ctx->nchunks * kChunk;
        std::vector<uint8_t> flags((size_t)n);
        int64_t cnt = 0;
        for (int64_t i = 0; i < n; ++i) cnt += flags[(size_t)i] = F[i] != 0.0;
        DevBuf<uint8_t> stage;
        HIP_TRY(ctx->d_btgt.reserve((size_t)rows, true));
        hipError_t e = stage.reserve((size_t)n, false);
        if (e == hipSuccess) e = hipMemcpyAsync(stage.p, flags.data(), (size_t)n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(block_kernels().target_pack, dim3(pack_grid(rows)), dim3(kBlock), 0, ctx->stream, n, rows, (const uint8_t *)stage.p,
                               ctx->perm_on ? (const int32_t *)ctx->d_perm.p : nullptr, ctx->d_btgt.p);
            e = hipStreamSynchronize(ctx->stream);
        }
        stage.release();
        if (e != hipSuccess) {
            ctx->d_btgt.release();                     // (the set alone: blk_tgt and btgt_states are still at their defaults)
            HIP_TRY(e);
        }
        ctx->blk_tgt = true;
        ctx->btgt_states = cnt;
        return 0;
    });
}

static int block_target_info(kfsp_ctx *ctx, int64_t *v)
{
    v[0] = ctx->blk_tgt ? 1 : 0;
    v[1] = ctx->btgt_states;
    v[2] = ctx->bhit_launches;
    for (int i = 3; i < 8; ++i) v[i] = 0;
    return 0;
}

static int block_hit(kfsp_ctx *ctx, int32_t which, double *out)
{
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx)) return rc;
        if (!ctx->blk_tgt) return fail(ctx, -1, "block_target = 3: no target set resident (kfsp_set_block under block_target = 1)");
        if (which != 0 && which != 1) return fail(ctx, -2, "block_target = 3: m is 0 (the flux of the block W) or 1 (of its time integral J)");
        if (!out) return fail(ctx, -3, "null out");
        if (ctx->opt_adjoint)
            return fail(ctx, -12, "block_target = 3: the flux into the set is a forward quantity, not with option adjoint "
                                  "(include/kfsp.h, TARGET SETS, has the backward recipe)");
        if (which == 1 && !ctx->blk_int)
            return fail(ctx, -1, "block_target = 3: no integral resident beside the block (option block_integral before kfsp_set_block)");
        HIP_TRY(hipSetDevice(ctx->device));
        const int kp = ctx->blk_kp;
        hipStream_t st = ctx->stream;
        if (int rc = ensure_scalars(ctx)) return rc;
        // the raw product goes to a column of its own: W, J and a basis laid out by kfsp_block_begin stay as they are
        if (ctx->d_bhit.cap < col_len(ctx, kp)) {
            ctx->d_bhit.release();
            HIP_TRY(ctx->d_bhit.reserve(col_len(ctx, kp), true));
        }
        HIP_TRY(ctx->d_bhsum.reserve((size_t)2 * K, true));
        double *y = bcol(ctx->d_bhit.p, ctx, kp, 0);
        int g = 0;
        if (int rc = spmm(ctx, kp, bcol(which ? ctx->d_bint.p : ctx->d_blk.p, ctx, kp, 0), y, nullptr, nullptr, false, &g)) return rc;
        const int gv = launch_flat(ctx, kp, block_kernels().hit, kp_index(kp), ctx->d_btgt.p, pairs(y), ctx->d_bpart.p);
        // the sum stage of k_bfinal alone: the block partials in its fixed order (both of its sums read the same ones)
        hipLaunchKernelGGL(block_kernels().finish, dim3(1), dim3(kBlock), 0, st, (int)kFinWsum, 0, kp, gv, ctx->d_bpart.p, (int64_t)0, ctx->d_bscal.p, 0.0,
                           ctx->d_bhsum.p);
        ctx->bhit_launches = 3;
        double h[K];
        HIP_TRY(hipMemcpyAsync(h, ctx->d_bhsum.p, K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int c = 0; c < K; ++c) out[c] = c < ctx->blk_k ? h[c] : 0.0;
        return 0;
    });
}

int kfsp_spmm_bench(kfsp_ctx *ctx, int reps, float *ms_total)
{
    if (!ctx) return -1;
    return guarded(ctx, [&]() -> int {
        if (int rc = block_call_ok(ctx, "no block resident")) return rc;
        if (reps < 1) return fail(ctx, -2, "reps < 1");
        if (!ms_total) return fail(ctx, -3, "null ms_total");
        if (ctx->group) return group_spmm_bench(ctx, reps, ms_total);
        HIP_TRY(hipSetDevice(ctx->device));
        const int kp = ctx->blk_kp;
        if (int rc = ensure_basis(ctx, kp, 1)) return rc;
        const double *x = bcol(ctx->d_blk.p, ctx, kp, 0);
        double *y = bcol(ctx->d_bv.p, ctx, kp, 0);
        HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
        record_direction(ctx);
        // (under a row partition the source is exchanged before every product, as in the solver)
        for (int r = 0; r < reps; ++r) {
            int g = 0;
            if (int rc = spmm(ctx, kp, x, y, nullptr, nullptr, false, &g)) return rc;
        }
        HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
        HIP_TRY(hipEventSynchronize(ctx->ev1));
        HIP_TRY(hipEventElapsedTime(ms_total, ctx->ev0, ctx->ev1));
        return 0;
    });
}

}  // extern "C"
