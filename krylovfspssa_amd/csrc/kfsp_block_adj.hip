// Backward solves on the block path: Y = A^T X for a block X of kp columns (option adjoint; include/kfsp.h, "several
// vectors at once"; DESIGN.md 12, "Backward solves").  A is the FSP-truncated generator exactly as k_spmm / k_spmm_box
// apply it: DIAG is the sum of ALL propensities of a state, those that leave the FSP included.
//
// Three kernels, one per form the generator is resident in.  They share k_spmm's conventions (kfsp_block.hip): SpmmArgs,
// the XCD-aware trip mapping and trip_order, one lane per row, kp accumulators in registers, the DOTS partials in
// block_sum_cols' layout.  Rows in [n, rows_act) are written as +0.0.
//
// Order of operations, per column, fixed: s = -(diag x_r) first (one multiply, k_spmv's sign convention), then ONE
// __builtin_fma per entry -
//   banded   diagonals d ascending: value val[d ld + (r - delta_d)], X row r - delta_d; a source outside [0, n) counts as
//            0.0 against the row's own X row;
//   ELL      slots k ascending: OFFDIAG(k, r) X[ADJ(k, r)]; a missing target as 0.0 against the row's own X row;
//   box      the accumulator starts at +0.0, one fma per slot in species-then-slot order with a_k(x) of the row's own
//            coordinates and X row r + delta_k when x + nu_k lies in the box (else 0.0 against the row's own X row), then
//            fma(-dsum, x_r, acc) - the shape of row_box_blk;
//   generic box (option block_box = 2, k_spmm_boxg_t; the row code is kfsp_boxg_dev.h's): s = -(dsum x_r) with dsum summed
//            in the model's reaction order, then one fma per sorted position p ascending of a_p(x) of the row's own
//            coordinates against X row r - delta_p when x + nu_p lies in the box (else 0.0 against the row's own X row).
// The file is compiled with contraction off: column c of A^T X does not depend on k, kp or the slot it sits in.
#pragma clang fp contract(off)

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"
#include "kfsp_boxg_dev.h"

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

// (finish_row - what every kernel does with a finished row - is kfsp_block_dev.h's: k_spmm_diac_t shares it)

// Banded (formats 1 and 2; a masked context reads the stored zeros of its empty segments).  Row r of A^T gathers
// A(r - delta_d, r) = val[d ld + r - delta_d]: the value streams at shifted rows.  No read of val or X leaves [0, n).
template <int KP, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_t(SpmmArgs a)
{
    __shared__ double red[4 * KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;
    const int64_t cpx = (a.trips + 7) >> 3;
    const int64_t cbeg = (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < a.trips) ? cbeg + cpx : a.trips;
    const int64_t cstep = (int64_t)bx * 4;
    const int64_t n = a.D.n;
    double da[KP], db[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) da[c] = db[c] = 0.0;
    for (int64_t t = cbeg + (int64_t)slot * 4 + wave; t < cend; t += cstep) {
        const int64_t ct = a.trip_order ? (int64_t)__builtin_amdgcn_readfirstlane(a.trip_order[t]) : t;
        for (int h = 0; h < 2; ++h) {
            const int64_t r = (ct << 7) + h * 64 + lane;
            double s[KP];
            if (r < n) {
                double x[KP];
                ld_row<KP>(a.X, r, x);
                diag_row<KP>(a.D.diag[r], x, s);
                for (int d = 0; d < a.D.nd; ++d) {
                    const int64_t src = r - a.D.delta[d];
                    const bool ok = src >= 0 && src < n;
                    const double v = ok ? a.D.val[(int64_t)d * a.D.ld + src] : 0.0;
                    ld_row<KP>(a.X, ok ? src : r, x);
                    fma_row<KP>(v, x, s);
                }
            } else {
#pragma unroll
                for (int c = 0; c < KP; ++c) s[c] = 0.0;
            }
            finish_row<KP, DOTS>(a, r, s, da, db);
        }
    }
    if (DOTS) {
        block_sum_cols<KP>(da, red, a.part + (size_t)blockIdx.x * K);
        block_sum_cols<KP>(db, red, a.part + ((size_t)kMaxGrid + blockIdx.x) * K);
    }
}

// Contexts whose forward image is SELL or coded SELL: lane = state c reads column c of the resident reference arrays
// (the gather row c of A^T), 64 rows per trip as for SELL.
template <int KP, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_ell_t(SpmmArgs a, EllAdjDev e)
{
    __shared__ double red[4 * KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;
    const int64_t cpx = (a.trips + 7) >> 3;
    const int64_t cbeg = (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < a.trips) ? cbeg + cpx : a.trips;
    const int64_t cstep = (int64_t)bx * 4;
    double da[KP], db[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) da[c] = db[c] = 0.0;
    for (int64_t t = cbeg + (int64_t)slot * 4 + wave; t < cend; t += cstep) {
        const int64_t ct = a.trip_order ? (int64_t)__builtin_amdgcn_readfirstlane(a.trip_order[t]) : t;
        const int64_t r = (ct << 6) + lane;
        double s[KP];
        if (r < e.n) {
            double x[KP];
            ld_row<KP>(a.X, r, x);
            diag_row<KP>(e.diag[r], x, s);
            const int32_t *ap = e.adj + r * e.ld;
            const double *op = e.off + r * e.ld;
            for (int k = 0; k < e.bw; ++k) {
                const int64_t tgt = (int64_t)ap[k] - 1;
                const bool ok = tgt >= 0 && tgt < e.n;
                const double v = ok ? op[k] : 0.0;
                ld_row<KP>(a.X, ok ? tgt : r, x);
                fma_row<KP>(v, x, s);
            }
        } else {
#pragma unroll
            for (int c = 0; c < KP; ++c) s[c] = 0.0;
        }
        finish_row<KP, DOTS>(a, r, s, da, db);
    }
    if (DOTS) {
        block_sum_cols<KP>(da, red, a.part + (size_t)blockIdx.x * K);
        block_sum_cols<KP>(db, red, a.part + ((size_t)kMaxGrid + blockIdx.x) * K);
    }
}

// Row r0 + lane of A^T of a single-factor matrix-free box.  Coordinates and dsum as row_box_blk has them; the test word
// has bit 5 s + nu + 2 set when coordinate s moved by nu (-2 .. 2) stays inside [0, dims[s]), so a slot's target x + nu_k
// lies in the box exactly when the word holds all bits of the slot's `need`.  X is addressed as wave base (scalar) +
// 32-bit lane offset like the forward row, with the base below the row by the largest BACKWARD reach of the targets
// (the forward reach of the sources): box_block_reach_ok covers both.
template <int KP, int NS, int PER>
__device__ __forceinline__ void row_box_t_blk(const BoxRegs<NS, PER> &R, const BoxAdjDev &B, const double *__restrict__ X, int64_t r0,
                                              int lane, double (&s)[KP])
{
    const uint64_t xb = reinterpret_cast<uint64_t>(X + r0 * KP) - (uint64_t)(uint32_t)B.bias8 * (uint64_t)KP;
    const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
    const unsigned voff = (unsigned)(8 * KP * lane) + (unsigned)B.bias8 * (unsigned)KP;
    auto ld = [&](unsigned at, double (&x)[KP]) {
#pragma unroll
        for (int q = 0; q < KP / 2; ++q) {
            const box_pair_t t = *(const __attribute__((address_space(1), aligned(16))) box_pair_t *)(xw + at + 16 * q);
            x[2 * q] = t.x;
            x[2 * q + 1] = t.y;
        }
    };
    // coordinates of the row: successive division by the box dimensions (exact: r < 2^31, one correction step)
    int co[6] = {0, 0, 0, 0, 0, 0};
    uint32_t q = (uint32_t)(r0 + lane);
#pragma unroll
    for (int S = 0; S + 1 < NS; ++S) {
        const int d = R.dims[S];
        uint32_t t = (uint32_t)((double)q * R.inv_dim[S]);
        int r = (int)(q - t * (uint32_t)d);
        const int lo = r < 0, hi = r >= d;
        t = t - lo + hi;
        r = r + (lo ? d : 0) - (hi ? d : 0);
        co[S] = r;
        q = t;
    }
    co[NS - 1] = (int)q;
    double dsum;
    unsigned valid;
    box_df<NS, PER>(R, co[0], co[1], co[2], co[3], co[4], co[5], dsum, valid);
    unsigned word = 0;
#pragma unroll
    for (int S = 0; S < NS; ++S) {
#pragma unroll
        for (int nu = -2; nu <= 2; ++nu) {
            const int y = co[S] + nu;
            word |= (y >= 0 && y < R.dims[S]) ? 1u << (5 * S + nu + 2) : 0u;
        }
    }
    double xd[KP], x[KP];
    ld(voff, xd);
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = 0.0;
    const unsigned lds0 = (unsigned)(size_t)(lds_bytes_t)box_lds;
#pragma unroll
    for (int S = 0; S < NS; ++S) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const unsigned need = B.need[S][j];
            const bool ok = (word & need) == need;
            const unsigned at = lds0 + (unsigned)(8 * co[S] + B.aoff8[S][j]);       // a_k(x) ...
            const double a = *(const __attribute__((address_space(3))) double *)(size_t)(ok ? at : lds0);   // ... or 0
            const unsigned vtgt = voff + (unsigned)B.tdelta8[S][j] * (unsigned)KP;
            ld(ok ? vtgt : voff, x);
            fma_row<KP>(a, x, s);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = __builtin_fma(-dsum, xd[c], s[c]);
}

// Matrix-free single-factor box (option block_box): the staged LDS image, box_load and the reductions of k_spmm_box.
template <int KP, int NS, int PER, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_box_t(SpmmArgs a, BoxAdjDev b)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < a.box_ntab; i += kBlock) box_lds[i] = a.box_tab[i];
    __syncthreads();
    BoxRegs<NS, PER> R;
    box_load(a.box_fast, R);
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;
    const int64_t cpx = (a.trips + 7) >> 3;
    const int64_t cbeg = (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < a.trips) ? cbeg + cpx : a.trips;
    const int64_t cstep = (int64_t)bx * 4;
    double da[KP], db[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) da[c] = db[c] = 0.0;
    for (int64_t t = cbeg + (int64_t)slot * 4 + wave; t < cend; t += cstep) {
        const int64_t ct = a.trip_order ? (int64_t)__builtin_amdgcn_readfirstlane(a.trip_order[t]) : t;
        for (int h = 0; h < 2; ++h) {
            const int64_t r0 = (ct << 7) + h * 64;
            const int64_t r = r0 + lane;
            double s[KP];
            if (r < a.D.n) {
                row_box_t_blk<KP, NS, PER>(R, b, a.X, r0, lane, s);
            } else {
#pragma unroll
                for (int c = 0; c < KP; ++c) s[c] = 0.0;
            }
            finish_row<KP, DOTS>(a, r, s, da, db);
        }
    }
    if (DOTS) {
        __syncthreads();
        block_sum_cols<KP>(da, box_lds, a.part + (size_t)blockIdx.x * K);
        block_sum_cols<KP>(db, box_lds, a.part + ((size_t)kMaxGrid + blockIdx.x) * K);
    }
}

// Any matrix-free box (option block_box = 2): the interpreted row, transposed.  The descriptor is the forward product's.
template <int KP, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_boxg_t(BoxgArgs)
{
    spmm_boxg_body<KP, DOTS, true>();
}

}  // namespace

// ---- the kernels by function pointer (kfsp_block_dev.h): kfsp_block.hip launches them
SpmmFn spmm_t_kernel(int kp, bool dots)
{
    return dispatch_kp_dots(kp, dots, [](auto KP, auto DOTS) -> SpmmFn { return k_spmm_t<decltype(KP)::value, decltype(DOTS)::value>; });
}

SpmmEllTFn spmm_ell_t_kernel(int kp, bool dots)
{
    return dispatch_kp_dots(kp, dots, [](auto KP, auto DOTS) -> SpmmEllTFn { return k_spmm_ell_t<decltype(KP)::value, decltype(DOTS)::value>; });
}

SpmmBoxTFn spmm_box_t_kernel(int kp, int inst, bool dots)
{
    return dispatch_kp_dots(kp, dots, [&](auto KP, auto DOTS) {
        return dispatch_box_inst(inst, [](auto NS, auto PER) -> SpmmBoxTFn {
            return k_spmm_box_t<decltype(KP)::value, decltype(NS)::value, decltype(PER)::value, decltype(DOTS)::value>;
        });
    });
}

SpmmBoxgFn spmm_boxg_t_kernel(int kp, bool dots)
{
    return dispatch_kp_dots(kp, dots, [](auto KP, auto DOTS) -> SpmmBoxgFn { return k_spmm_boxg_t<decltype(KP)::value, decltype(DOTS)::value>; });
}

}  // namespace kfsp
