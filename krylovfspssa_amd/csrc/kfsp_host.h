// Private: what the host code of every translation unit of libkfsp_hip shares - status codes and texts of failed
// calls, the exception fence of the C boundary, the phase timer, the launch rules of the generator product and of the
// streaming kernels, and the generator's part of the kernel arguments.  Plain inline host code: a stand-alone program
// can call the grid rules without a device (tests/grid_rule_check.cpp).
#pragma once

#include "kfsp_ctx.h"

#include <chrono>
#include <exception>
#include <new>
#include <string>

namespace kfsp {

// (c may be null: an entry point that fails before it has a context still returns its code)
inline int fail(kfsp_ctx *c, int code, const char *what)
{
    if (c) c->err = what;
    return code;
}

inline int hip_fail(kfsp_ctx *c, hipError_t e, const char *where)
{
    if (c) c->err = std::string(where) + ": " + hipGetErrorString(e);
    return 1000 + (int)e;
}

// for functions that return a status code and call their context `ctx`
#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(ctx, e_, #expr); \
    } while (0)

// C++ exceptions (host allocations) end at the C boundary as status codes
template <class F>
int no_throw(kfsp_ctx *c, F &&body, const char *other = "unknown exception")
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(c, 4001, "out of host memory");
    } catch (const std::exception &e) {
        if (c) c->err = std::string("exception: ") + e.what();
        return 4000;
    } catch (...) {
        return fail(c, 4000, other);
    }
}

struct PhaseTimer {
    kfsp_ctx *c;
    int phase;
    std::chrono::steady_clock::time_point t0;
    PhaseTimer(kfsp_ctx *c_, int p) : c(c_), phase(p), t0(std::chrono::steady_clock::now()) {}
    ~PhaseTimer() { c->t_ms[phase] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- the launch rule of the generator product, single vector and block alike
// a wavefront trip covers 64 rows (one SELL chunk) or 128 rows (banded and matrix-free forms, two rows per lane)
inline int64_t product_trips(int64_t nchunks, bool dia) { return dia ? (nchunks + 1) / 2 : nchunks; }

// Workgroups (4 wavefronts, one trip each at a time) for `trips` trips: a multiple of 8, at least 8, at most option
// grid_blocks (opt_grid > 0, rounded up to 8) or else dflt_cap - and never more than kMaxGrid, whatever the option
// says: a producer's block partials go to a slot of kMaxGrid doubles (next_partial, d_bpart).
// dflt_cap of a stored generator is 1024: 4 workgroups per CU already saturate HBM with the 5-9 independent loads a
// lane keeps in flight, and halve the partial sums every consumer has to re-add (measured: profiles/r01_sweep.log).
inline int product_grid(int64_t trips, int64_t opt_grid, int64_t dflt_cap)
{
    const int64_t cap = std::min<int64_t>(opt_grid > 0 ? round_up(opt_grid, 8) : dflt_cap, kMaxGrid);
    return (int)std::max<int64_t>(std::min<int64_t>(round_up((trips + 3) / 4, 8), cap), 8);
}

// ---- the split of a product under the halo exchange, single vector (run_product) and block (kfsp_block.hip) alike
// A rank's block has L rows and reads H rows of either neighbour; a trip covers trip_rows rows.  Trips [lo, hi) read no
// halo row: lo is the first trip whose rows all lie >= H, trips below hi end at or below L - H.  They are launched on
// their own, while the strips travel, only when that pays: three launches and two cross-stream waits cost ~10-15 us, so
// the interior must be several times longer (>= 16384 trips, ~2M rows per rank) - or the caller insists (option
// overlap = 2, used by the tests: >= 64 trips).  overlap = 0: never.
struct ProductSplit {
    int64_t lo, hi;
    bool split;
};
inline ProductSplit product_split(int64_t H, int64_t L, int64_t trips, int64_t trip_rows, int64_t overlap)
{
    ProductSplit s;
    s.lo = (H + trip_rows - 1) / trip_rows;
    s.hi = std::min<int64_t>((L - H) / trip_rows, trips);
    s.split = overlap != 0 && s.hi - s.lo >= (overlap >= 2 ? 64 : 16384);
    return s;
}

// The split product itself.  The strips of `src` (width doubles per row) travel on the communication stream, behind
// everything that produced src, while the interior trips run on the compute stream; the boundary trips follow once the
// halo has landed, as ONE launch: linear trips [0, lo) are themselves, [lo, lo + trips - hi) stand for [hi, trips).
// launch_range(begin, end, split, jump, grid, used) launches the linear trips [begin, end) (SpmvArgs / SpmmArgs:
// trip_split, trip_jump) on `grid` workgroups with its block partials `used` slots into the caller's buffer, and returns
// the slots it took.  The interior keeps 512 of a slot's kMaxGrid partials free for the boundary launch.  *used: the
// slots of both launches.  The caller has set trip_order = nullptr: the ranges are linear.
template <class LaunchRange>
int overlapped_product(kfsp_ctx *ctx, const ProductSplit &ps, int64_t trips, const double *src, int width, int64_t dflt_cap,
                       LaunchRange &&launch_range, int *used)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(hipEventRecord(ctx->ev_src, st));
    HIP_TRY(hipStreamWaitEvent(ctx->comm_stream, ctx->ev_src, 0));
    if (int rc = exchange_strips(ctx, src, ctx->comm_stream, width)) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_halo, ctx->comm_stream));
    const int g1 = std::min(product_grid(ps.hi - ps.lo, ctx->opt_grid, dflt_cap), kMaxGrid - 512);
    *used = launch_range(ps.lo, ps.hi, INT64_MAX, (int64_t)0, g1, 0);
    HIP_TRY(hipStreamWaitEvent(st, ctx->ev_halo, 0));
    const int64_t nb = ps.lo + (trips - ps.hi);
    *used += launch_range((int64_t)0, nb, ps.lo, ps.hi - ps.lo, product_grid(nb, 0, 512), *used);
    return 0;
}

// Rows of margin on either side of every basis column once strips of H rows are exchanged (setup_exchange): the strip,
// a quarter of head room, and 128 rows because the banded kernel works on 128-row groups whose padded half reads up to
// one group beyond the block end.  A multiple of 64.
inline int64_t halo_margin(int64_t H) { return round_up(H + H / 4 + 2 * kChunk, 64); }
// ... and of a block column (kfsp_block.hip): the context's margin, never less than the 64 zero rows the one-rank block
// path has always had round its columns.
constexpr int64_t kBlockMargin = 64;
inline int64_t block_margin(int64_t ctx_margin) { return std::max<int64_t>(kBlockMargin, ctx_margin); }

// Streaming kernels over `pairs` 16-byte pairs: every consumer re-sums the producer's partials, so the grid is kept at
// <= 1024 workgroups (4 per CU; option vec_grid_blocks) with >= 4 pairs per lane; the loops are unrolled so that this
// still keeps > 16 MB of loads in flight.
inline int vec_grid(int64_t pairs, int64_t opt_vgrid)
{
    const int64_t g = (pairs + 4 * kBlock - 1) / (4 * kBlock);
    return (int)std::max<int64_t>(std::min<int64_t>(g, std::min<int64_t>(opt_vgrid > 0 ? opt_vgrid : 1024, kMaxGrid)), 1);
}

// ---- banded or SELL: the one rule, for the device build (build_from_resident_ell) and the host build (maybe_upload_dia)
// A stored diagonal entry costs 8 bytes, zero or not, a SELL slot 12: banded moves fewer bytes while nd * rows <= 1.5 *
// (off-diagonal entries) (+ 1024 of grace).  How nd is counted is each path's own: the device build counts the used reaction
// slots, each ONE constant shift; the host build the distinct column offsets, up to kMaxDiag + 1 (tests/generator_rule_check.cpp).
inline bool banded_pays(int nd, int64_t nloc, int64_t nnz_off, int64_t opt_format)
{ return opt_format != 1 && nloc > 0 && nd > 0 && nd <= kMaxDiag && (double)nd * (double)nloc <= 1.5 * (double)nnz_off + 1024.0; }

// ---- whether a generator of n states gets the internal state order: sorting, relabelling and the extra upload cost what ~20
// products (at 10^6 states) save - worth it only while generators live that long; the one being replaced is the best predictor
inline bool want_state_order(int64_t opt_state_order, int64_t n, int64_t min_n, int64_t products, int64_t min_products)
{ return opt_state_order != 0 && n >= min_n && products >= min_products; }
inline bool want_state_order(const kfsp_ctx *c, int64_t n)
{ return want_state_order(c->opt_state_order, n, c->opt_state_order_min, c->prod_count, c->opt_state_order_products); }

// the generator's stored images as the kernels take them
inline void generator_args(const kfsp_ctx *c, SellDev &A, DiaDev &D)
{
    A = SellDev{c->nloc, c->nchunks, c->d_off.p, c->d_col.p, c->d_val.p, c->d_diag.p,
                c->d_dtab.p, c->d_dtlen.p, c->d_code.p, c->d_codeoff.p};
    D.nd = c->nd;
    for (int d = 0; d < kMaxDiag; ++d) D.delta[d] = c->delta[d];
    D.val = c->d_dia.p;
    D.ld = c->dia_ld;
    D.diag = c->d_diag.p;
    D.nchunks = c->nchunks;
    D.n = c->n;
    D.gmask = c->dia_masked ? c->d_gmask.p : nullptr;
    D.zero = c->d_zero.p;
}

// ---- the dictionary-coded image of the banded values (kernel format 9), single vector and block alike
// the product may read it: banded, stored, the image resident for d_dia, unmasked, single rank
inline bool dia_code_on(const kfsp_ctx *c) { return c->use_dia && !c->box.on && c->dia_coded && !c->dia_masked && !c->use_comm; }

inline void dia_code_args(const kfsp_ctx *c, DiaCodeDev &C)
{
    C.rec = c->d_dcode.p;
    C.dict = c->d_ddict.p;
    for (int d = 0; d <= kMaxDiag; ++d) C.doff[d] = c->dia_doff[d];
    C.w = c->dia_code_w;
    C.rec_bytes = c->dia_code_rec;
}

// the kernel a product on that image runs (dia_code_kernel, kfsp_dia_diag.h); meaningful where dia_code_on
inline DiaCodeKernel dia_code_kernel(const kfsp_ctx *c)
{
    return dia_code_kernel(c->nd, c->dia_code_w, c->dia_code_rec, c->dia_diag.nk, c->dia_diag.ntab, c->dia_doff[c->nd],
                           c->opt_dia_code_lanes != 0, c->opt_dia_code_inner != 0);
}

// Option block_dia_code: the forward block product takes the coded image (k_spmm_diac, kfsp_block_diac.hip) where the
// single-vector product takes it (coded_on = dia_code_on), the option is on, the product is not the transposed one
// (row r of A^T needs code d of row r - delta_d: nd record loads) and the pass is not the one-launch small one (its
// product is compiled into k_barnoldi_small).  Everything else keeps the kernel it had.  Plain flags, so that a
// stand-alone program can walk all combinations (tests/block_dia_code_check.cpp).
inline bool block_dia_code_path(bool coded_on, int64_t opt_block_dia_code, bool adjoint, bool small)
{
    return coded_on && opt_block_dia_code != 0 && !adjoint && !small;
}

// Option block_dia_code_adjoint: beside block_dia_code, the TRANSPOSED block product takes the coded image as well
// (k_spmm_diac_t, kfsp_block_diac_t.hip: one 8-byte record word per diagonal from the source rows' records, which the
// neighbouring rows have just fetched, instead of nd value streams).  OPT-IN on top of the opt-in: block_dia_code = 1 with
// adjoint = 1 alone keeps k_spmm_t.  The one-launch small pass is never taken under adjoint (small_path), so it does not
// enter the rule.  Plain flags (tests/block_dia_code_adjoint_check.cpp).
inline bool block_dia_code_t_path(bool coded_on, int64_t opt_block_dia_code, int64_t opt_block_dia_code_adjoint, bool adjoint)
{
    return coded_on && opt_block_dia_code != 0 && opt_block_dia_code_adjoint != 0 && adjoint;
}

// ---- the kernel format a WHOLE-product launch takes (run_product), from plain flags, so that a stand-alone program can
// walk all combinations (tests/box_plan_check.cpp): 0 SELL-64, 5 with coded columns, 1 banded, 2 with group masks, 9 with
// coded values, 3 matrix-free box, 4 its single-factor form, 8 / 7 that form in slabs / pencils (eligible box, option
// box_pencil, not under box_lds), 6 with the near part of x in LDS (option box_lds, a reach, the ascending trip order).
// kfsp_layout_info reports the same function with trip_order = false - the one input a product can change under a
// resident generator (kfsp_set_trip_order: format 6 then runs as 4) - and 9 as 1.  The launches of a product split
// round the halo exchange take only 0 - 5 and 9: a communicator rules 6, 7 and 8 out.
struct ProductForm {
    bool banded, box;                    // use_dia; a matrix-free box (which is banded)
    bool fast;                           // ... whose single-factor form may be used (fast && !box_generic)
    bool slab, pencil, reach;            // what box_plan found the box eligible for (reach > 0)
    int64_t box_pencil, box_lds;         // the options
    bool comm, trip_order;
    bool coded, masked, sell_coded;      // dia_code_on; dia_masked; sell_coded
    bool force_sell, force_plain_sell;   // kfsp_spmv_bench's variants
};
inline int product_format(const ProductForm &f)
{
    const bool dia = f.banded && !f.force_sell;
    if (!dia) return f.sell_coded && !f.force_plain_sell ? 5 : 0;
    if (!f.box) return f.coded ? 9 : (f.masked ? 2 : 1);
    if (!f.fast) return 3;
    if (f.comm) return 4;
    if (f.slab && f.box_pencil == 2 && f.box_lds == 0) return 8;
    if (f.pencil && f.box_pencil != 0 && f.box_lds == 0) return 7;
    if (f.reach && f.box_lds != 0 && !f.trip_order) return 6;
    return 4;
}
inline ProductForm product_form(const kfsp_ctx *c, bool trip_order, bool force_sell = false, bool force_plain_sell = false)
{
    return ProductForm{c->use_dia, c->box.on, c->box.fast && !c->opt_box_generic, c->box.slab, c->box.pencil, c->box.reach > 0,
                       c->opt_box_pencil, c->opt_box_lds, c->use_comm, trip_order, dia_code_on(c), c->dia_masked, c->sell_coded,
                       force_sell, force_plain_sell};
}

}  // namespace kfsp
