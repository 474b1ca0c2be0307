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

// A tiled order of the 128-row trips over a lexicographic box of n rows (ns species, dims fastest first): rows are cut
// below the slowest stride that is still at most 16 K rows (cut), r = hi * S_cut + lo; blocks of B = 1024 rows of lo; per
// block ALL lines hi back to back.  A row's +-S neighbours for the strides above the cut are then whole lines away - one
// line = B rows = 8 KB of x - instead of whole strides: 22^6 with the cut below species 4: the +-22^3 / 22^4 / 22^5
// neighbours sit 1 / 22 / 484 lines = 8 KB / 180 KB / 4 MB from the row in the order of the sweep.  Empty: keep the
// ascending order - fewer than three species, a cut stride under 2048 rows, or neither `force` nor a box beyond the
// caches.  Its one caller is the base-trip order of the pencil kernel (format 7, kfsp_set_matrix_box: the box is a plane,
// `force` comes from option "box_tile"); tests/box_tile_order_check.cpp calls it without a device.
inline std::vector<int32_t> box_tile_order(int ns, const int32_t *dims, int64_t n, bool force)
{
    std::vector<int32_t> out;
    const int64_t trips = (n + 127) / 128;
    if (ns < 3 || trips < 2 || trips > INT32_MAX) return out;
    int64_t stride = 1, smax = 1;
    int cut = -1;
    int64_t scut = 1;
    for (int s = 0; s < ns; ++s) {
        if (stride <= 16384 && s > 0) {
            cut = s;
            scut = stride;
        }
        smax = stride;
        stride *= dims[s];
    }
    const double mall = 256.0 * 1024 * 1024;
    const bool large = (double)n * 8.0 > mall && 8.0 * 2.0 * (double)smax * 8.0 > mall;
    if (cut < 1 || scut < 2048 || !(force || large)) return out;
    const int64_t B = 1024, nhi = (n + scut - 1) / scut;
    std::vector<std::pair<int64_t, int32_t>> key((size_t)trips);
    for (int64_t c = 0; c < trips; ++c) {
        const int64_t r = c * 128, lo = r % scut, hi = r / scut;
        key[(size_t)c] = {((lo / B) * nhi + hi) * scut + lo, (int32_t)c};
    }
    std::sort(key.begin(), key.end());
    out.resize((size_t)trips);
    for (int64_t c = 0; c < trips; ++c) out[(size_t)c] = key[(size_t)c].second;
    return out;
}

// option "box_tile" -> the `force` of the pencil kernel's base-trip order: -1 a plane beyond 4 MiB, 0 never (no order at
// all, whatever the size), 1 wherever box_tile_order has one to give
inline bool box_tile_wanted(int64_t tile) { return tile != 0; }
inline bool box_tile_force(int64_t tile, int64_t plane_rows) { return tile > 0 || (tile < 0 && plane_rows * 8 > (int64_t)(4 << 20)); }

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
inline bool dia_code_on(const kfsp_ctx *c) { return c->use_dia && !c->use_box && c->dia_coded && !c->dia_masked && !c->use_comm; }

inline void dia_code_args(const kfsp_ctx *c, DiaCodeDev &C)
{
    C.rec = c->d_dcode.p;
    C.dict = c->d_ddict.p;
    for (int d = 0; d <= kMaxDiag; ++d) C.doff[d] = c->dia_doff[d];
    C.w = c->dia_code_w;
    C.rec_bytes = c->dia_code_rec;
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

}  // namespace kfsp
