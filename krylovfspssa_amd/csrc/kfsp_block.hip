// Several start vectors at once: exp(tA) W for a block W of k <= 16 columns on one pass over the generator per
// product (include/kfsp.h, "several vectors at once").
//
// Layout.  A block vector holds kp = k rounded up to 2, 4, 8 or 16 doubles per row, row-interleaved: row i of
// column c at X[i * kp + c].  The padding columns are zero and stay zero.  Every block column carries 64 zero rows in
// front and 64 behind its rows (the x clamp of the banded product reads row -1 and row n, like the guard words of
// DevBuf and the column padding of the single-vector path).
//
// SpMM.  One lane per row, kp accumulators in registers, the x of an entry read as kp/2 16-byte loads: the generator
// streams are read once per block.  Column c of a row is summed in EXACTLY the order of the single-vector kernel
// (kfsp_spmv_dev.h: row_sell, row_sell_coded, rows_dia): -DIAG x first (one v_mul_f64), then one fused multiply-add
// per entry in FMATVEC's order (KrylovSolver.f90:598-604).  The fused operations are written out below and the file
// is compiled with contraction off, so no other fusion can creep in: column c of A X is bit-identical to kfsp_spmv of
// column c (tests/test_gpu_block.py).  The banded rows take the operands the two-rows-per-lane kernel takes, clamp
// included.
//
// Arnoldi.  k INDEPENDENT IOP(2) bases (not a block Krylov space): per column its own beta, H, breakdown and AVNORM.
// Dot products and norms are block partials in a fixed layout, summed in a fixed order by one small finishing
// launch: two runs give the same bits.  A column whose H(j+1,j) <= break_tol stops there (its coefficients become 0,
// its H is exact); a column with beta = 0 is skipped from the start and stays exactly 0.
//
// Matrix-free boxes (k_spmm_box below; DESIGN.md 12, "Matrix-free boxes"): the row of a single-factor box is rebuilt once -
// coordinates, {sum, valid} look-ups, one LDS read per entry - and applied to all kp columns, in the operation order of the
// single-vector matrix-free kernels (k_spmv format 4 and the pencil kernel, kfsp_spmv_dev.h, kfsp_spmv_box.hip).  Every other
// box takes the interpreted row of kernel format 3: k_spmm_boxg (kfsp_block_boxg.hip), k_spmm_boxg_t (kfsp_block_adj.hip),
// the row code in kfsp_boxg_dev.h.
//
// Small generators ("Small generators"): one 1024-lane workgroup per block column - k_bbegin_small,
// k_barnoldi_small (kfsp_kernels.hip: the pass of k_arnoldi_small, compiled from the same lines) and k_bcombine_small.
// Time integrals ("Time integrals"): k_bcombine_int / k_bcombine_small_int - the pass over the basis that
// makes W also adds a second linear combination (the table behind coef, kfsp_block_integral.h) to a second block J.
// Target sets ("Target sets").  With a set T (one byte per row of the internal order) every block call works
// on the killed generator Q = D A D, D = diag(1 - 1_T), and no product kernel knows: the raw product's partials u . z are
// already those of Q because every basis column is 0 on T, and the TARGET instantiations of k_bcopy_nrm / k_bortho / k_bnorm
// put +0.0 on T before they sum; k_btarget_zero masks a column, k_bhit sums one raw product over T.
//
// The host side - which kernel a call runs, the launches, the buffers, the entry points - is kfsp_block_host.hip; it reaches
// the kernels of this file through the selectors at its end (kfsp_block_dev.h).
#pragma clang fp contract(off)

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"
#include "kfsp_boxg_dev.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

// SELL-64 row (plain or dictionary-coded columns), the slot order and addresses of row_sell / row_sell_coded
template <int KP, bool CODED>
__device__ __forceinline__ void row_sell_blk(const SellDev &A, const double *__restrict__ X, int64_t row0, int64_t c, int lane,
                                             double (&s)[KP])
{
    const int64_t off = A.off[c];
    const int w = (int)((A.off[c + 1] - off) >> 6);
    const int w2 = w >> 1;
    const int64_t lr = (c << 6) + lane;           // the row among the rank's rows: where its generator lies
    const int64_t r = row0 + lr;                  // ... and among all rows: where its x lies (columns are global)
    double x0[KP], x1[KP];
    ld_row<KP>(X, r, x0);
    diag_row<KP>(A.diag[lr], x0, s);
    const double *vp = A.val + off + 2 * lane;
    const int dtl = CODED ? __builtin_amdgcn_readfirstlane(A.dtlen[c]) : 0;
    if (CODED && dtl != 0) {
        const int tab = lane < dtl ? A.dtab[(c << 6) + lane] : 0;
        const unsigned long long *cp = A.code + A.codeoff[c] + lane;
        unsigned long long cw = *cp;
        int used = 0;
        auto next = [&]() -> int64_t {
            if (used == kSellCodePerWord) {
                cp += 64;
                cw = *cp;
                used = 0;
            }
            const int d = __builtin_amdgcn_ds_bpermute((int)(cw & 63ull) << 2, tab);
            cw >>= kSellCodeBits;
            ++used;
            return r + d;
        };
        for (int k = 0; k < w2; ++k) {
            const d2 v = *reinterpret_cast<const d2 *>(vp + k * 128);
            ld_row<KP>(X, next(), x0);
            ld_row<KP>(X, next(), x1);
            fma_row<KP>(v.x, x0, s);
            fma_row<KP>(v.y, x1, s);
        }
        if (w & 1) {
            ld_row<KP>(X, next(), x0);
            fma_row<KP>(A.val[off + w2 * 128 + lane], x0, s);
        }
        return;
    }
    const int32_t *cp = A.col + off + 2 * lane;
    for (int k = 0; k < w2; ++k) {
        const i2 cc = *reinterpret_cast<const i2 *>(cp + k * 128);
        const d2 v = *reinterpret_cast<const d2 *>(vp + k * 128);
        ld_row<KP>(X, cc.x, x0);
        ld_row<KP>(X, cc.y, x1);
        fma_row<KP>(v.x, x0, s);
        fma_row<KP>(v.y, x1, s);
    }
    if (w & 1) {
        ld_row<KP>(X, A.col[off + w2 * 128 + lane], x0);
        fma_row<KP>(A.val[off + w2 * 128 + lane], x0, s);
    }
}

// Banded row r: the operands rows_dia gives the row as the .x (even r) or .y (odd r) half of its pair - the pair
// start clamped to [-1, n - 1], an empty masked segment read as 0 against the row's own x.  r counts the rank's rows
// (generator), row0 + r all rows (x): the clamp is the one of the GLOBAL index against the global D.n, as in rows_dia.
template <int KP, bool MASKED>
__device__ __forceinline__ void row_dia_blk(const DiaDev &D, const double *__restrict__ X, int64_t row0, int64_t r, unsigned m,
                                            double (&s)[KP])
{
    const int64_t g = row0 + r;
    const int64_t ge = g & ~(int64_t)1;
    const int par = (int)(g & 1);
    const int64_t last = D.n - 1;
    auto xr = [&](int64_t p) -> int64_t { return (p < -1 ? -1 : (p > last ? last : p)) + par; };
    double x0[KP], x1[KP];
    ld_row<KP>(X, xr(ge), x0);
    diag_row<KP>(D.diag[r], x0, s);
    int d = 0;
    for (; d + 2 <= D.nd; d += 2) {
        const bool on0 = !MASKED || ((m >> d) & 1u), on1 = !MASKED || ((m >> (d + 1)) & 1u);
        const double v0 = on0 ? D.val[(int64_t)d * D.ld + r] : 0.0;
        const double v1 = on1 ? D.val[(int64_t)(d + 1) * D.ld + r] : 0.0;
        ld_row<KP>(X, xr(ge + (on0 ? D.delta[d] : 0)), x0);
        ld_row<KP>(X, xr(ge + (on1 ? D.delta[d + 1] : 0)), x1);
        fma_row<KP>(v0, x0, s);
        fma_row<KP>(v1, x1, s);
    }
    for (; d < D.nd; ++d) {
        const bool on0 = !MASKED || ((m >> d) & 1u);
        const double v0 = on0 ? D.val[(int64_t)d * D.ld + r] : 0.0;
        ld_row<KP>(X, xr(ge + (on0 ? D.delta[d] : 0)), x0);
        fma_row<KP>(v0, x0, s);
    }
}

// FMT: 0 SELL-64, 5 SELL-64 with coded columns, 1 banded, 2 banded with group masks.  XCD-aware trip mapping and
// trip order of k_spmv; a banded trip is a 128-row group taken as two 64-row halves.
// PART: the launch of a rank of a row partition - local rows against a globally addressed X (a.row0) and a range of
// linear trips (a.trip_begin .. a.trip_jump).  The one-rank launch is its own instantiation with row 0 and the whole
// range compiled in: with the ranged form alone the k = 8 banded product on c3 came out 19 % slower on the device
// (the compiler's schedule changed: 64 VGPRs instead of 76), DESIGN.md 12 "Row partitions".
template <int KP, int FMT, bool DOTS, bool PART>
__global__ __launch_bounds__(kBlock) void k_spmm(SpmmArgs a)
{
    const int64_t row0 = PART ? a.row0 : 0;
    const int64_t tbeg = PART ? a.trip_begin : 0, tend = PART ? a.trip_end : a.trips;
    constexpr bool DIA = FMT == 1 || FMT == 2;
    __shared__ double red[4 * KP];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;
    // the linear trips [trip_begin, trip_end) of this launch, dealt to the XCDs like the whole range [0, trips)
    const int64_t cpx = (tend - tbeg + 7) >> 3;
    const int64_t cbeg = tbeg + (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < tend) ? cbeg + cpx : tend;
    const int64_t cstep = (int64_t)bx * 4;
    double da[KP], db[KP];
#pragma unroll
    for (int c = 0; c < KP; ++c) da[c] = db[c] = 0.0;
    for (int64_t t = cbeg + (int64_t)slot * 4 + wave; t < cend; t += cstep) {
        const int64_t ct = a.trip_order ? (int64_t)__builtin_amdgcn_readfirstlane(a.trip_order[t]) : (PART && t >= a.trip_split ? t + a.trip_jump : t);
        const unsigned gm = FMT == 2 ? __builtin_amdgcn_readfirstlane(a.D.gmask[ct]) : 0xFFFFFFFFu;
        for (int h = 0; h < (DIA ? 2 : 1); ++h) {
            const int64_t r = DIA ? (ct << 7) + h * 64 + lane : (ct << 6) + lane;
            double s[KP];
            if (DIA) row_dia_blk<KP, FMT == 2>(a.D, a.X, row0, r, gm, s);
            else row_sell_blk<KP, FMT == 5>(a.A, a.X, row0, ct, lane, s);
            st_row<KP>(a.Y, r, s);
            if (DOTS && r < a.rows_red) {
                double u[KP];
                if (a.ua) {
                    ld_row<KP>(a.ua, r, u);
#pragma unroll
                    for (int c = 0; c < KP; ++c) da[c] = __builtin_fma(u[c], s[c], da[c]);
                }
                ld_row<KP>(a.ub, r, u);
#pragma unroll
                for (int c = 0; c < KP; ++c) db[c] = __builtin_fma(u[c], s[c], db[c]);
            }
        }
    }
    if (DOTS) {
        block_sum_cols<KP>(da, red, a.part + (size_t)blockIdx.x * K);
        block_sum_cols<KP>(db, red, a.part + ((size_t)kMaxGrid + blockIdx.x) * K);
    }
}

// Row r0 + lane of a single-factor matrix-free box (BoxFast) applied to the kp columns of X.  Per column the operations of
// rows_box1 (kfsp_spmv_dev.h) as its ISA has them: the accumulator starts at +0.0, ONE v_fma_f64 per entry slot in
// species-then-slot order (the first one against the literal 0, so a leading 0.0 * x of either sign leaves +0.0), then
// fma(-dsum, x_row, acc) with dsum the species' shares added in species order.  An invalid slot reads the 0.0 at the head
// of the LDS image and the row's OWN row of X (the single-vector kernel may read a neighbour's element there: any finite
// number, times 0.0, added to an accumulator that is not -0.0).  X is addressed as wave base (scalar) + 32-bit lane
// offset: box_block_reach_ok checks that the largest reach fits for this kp.
template <int KP, int NS, int PER>
__device__ __forceinline__ void row_box_blk(const BoxRegs<NS, PER> &R, const double *__restrict__ X, int64_t r0, int lane,
                                            double (&s)[KP])
{
    const uint64_t xb = reinterpret_cast<uint64_t>(X + r0 * KP) - (uint64_t)(uint32_t)R.bias8 * (uint64_t)KP;
    const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
    const unsigned voff = (unsigned)(8 * KP * lane) + (unsigned)R.bias8 * (unsigned)KP;
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
    double xd[KP], x[KP];
    ld(voff, xd);
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = 0.0;
    const unsigned lds0 = (unsigned)(size_t)(lds_bytes_t)box_lds;                  // LDS address of the image = of its 0.0
#pragma unroll
    for (int S = 0; S < NS; ++S) {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int m = __builtin_amdgcn_sbfe(valid, S * PER + j, 1);            // -1: the source state lies inside the box
            const unsigned at = lds0 + (unsigned)(8 * co[S] + R.koff8[S][j]);      // a_k(x - nu_k) ...
            const double a = *(const __attribute__((address_space(3))) double *)(size_t)((m & at) | (~m & lds0));   // ... or 0
            const unsigned vsrc = voff + (unsigned)R.delta8[S][j] * (unsigned)KP;
            ld(m ? vsrc : voff, x);
            fma_row<KP>(a, x, s);
        }
    }
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = __builtin_fma(-dsum, xd[c], s[c]);
}

// The block product of a matrix-free box: trips, trip order and partial layout of k_spmm's banded form.  Every workgroup
// stages the table image into dynamic LDS first (as k_spmv<.., 4> does) and reads the descriptor into scalar registers
// once per wavefront.  Rows in [n, rows_act) are written as zeros.  The reductions reuse the image's LDS once all
// wavefronts are done with it (the image may fill the 64 KB a workgroup gets).
template <int KP, int NS, int PER, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_box(SpmmArgs a)
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
                row_box_blk<KP, NS, PER>(R, a.X, r0, lane, s);
            } else {
#pragma unroll
                for (int c = 0; c < KP; ++c) s[c] = 0.0;
            }
            st_row<KP>(a.Y, r, s);
            if (DOTS && r < a.rows_red) {
                double u[KP];
                if (a.ua) {
                    ld_row<KP>(a.ua, r, u);
#pragma unroll
                    for (int c = 0; c < KP; ++c) da[c] = __builtin_fma(u[c], s[c], da[c]);
                }
                ld_row<KP>(a.ub, r, u);
#pragma unroll
                for (int c = 0; c < KP; ++c) db[c] = __builtin_fma(u[c], s[c], db[c]);
            }
        }
    }
    if (DOTS) {
        __syncthreads();
        block_sum_cols<KP>(da, box_lds, a.part + (size_t)blockIdx.x * K);
        block_sum_cols<KP>(db, box_lds, a.part + ((size_t)kMaxGrid + blockIdx.x) * K);
    }
}

// ---- streaming kernels over the flat array of 16-byte pairs: the grid stride is a multiple of kp/2, so a thread
// always holds the same two columns (2q, 2q+1) with q = thread id mod kp/2
__device__ __forceinline__ void flat_sum(double a0, double a1, int half, double *red, double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 32; o >= half; o >>= 1) {
        a0 += __shfl_xor(a0, o);
        a1 += __shfl_xor(a1, o);
    }
    if (lane < half) {
        red[wave * 2 * K + 2 * lane] = a0;
        red[wave * 2 * K + 2 * lane + 1] = a1;
    }
    __syncthreads();
    if (threadIdx.x < 2 * half) {
        const int c = threadIdx.x;
        out[c] = (red[c] + red[2 * K + c]) + (red[4 * K + c] + red[6 * K + c]);
    }
    __syncthreads();
}

// Target sets (the target-set mode of kfsp_set_block; DESIGN.md 12, "Target sets"): TARGET instantiations of the three streaming kernels
// of a pass read one flag byte per row - pair i lies in row i >> sh, sh = log2(kp / 2) - and put +0.0 where the flag is
// set, before anything is summed.  The false instantiations are the kernels as they were: tgt and sh are not read.
//
// U = W, partial: ||W_c||^2.  TARGET: U = D W
template <bool TARGET>
__global__ __launch_bounds__(kBlock) void k_bcopy_nrm(int64_t npairs, int half, const d2 *__restrict__ w, d2 *__restrict__ u,
                                                      double *__restrict__ part, const uint8_t *__restrict__ tgt, int sh)
{
    __shared__ double red[8 * K];
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        d2 v = w[i];
        if (TARGET && tgt[i >> sh]) v.x = v.y = 0.0;
        u[i] = v;
        a0 = __builtin_fma(v.x, v.x, a0);
        a1 = __builtin_fma(v.y, v.y, a1);
    }
    flat_sum(a0, a1, half, red, part + (size_t)blockIdx.x * K);
}

// z <- cz z - c1 u1 - c2 u2 per column; partials ||z||^2 and z . u2.  TARGET: z <- D (...), so the next basis column is
// one of D A D and zero on the set again
template <bool TARGET>
__global__ __launch_bounds__(kBlock) void k_bortho(int64_t npairs, int half, d2 *__restrict__ z, const d2 *__restrict__ u1,
                                                   const d2 *__restrict__ u2, const double *__restrict__ co,
                                                   double *__restrict__ part, const uint8_t *__restrict__ tgt, int sh)
{
    __shared__ double red[8 * K];
    const int q = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) % half);
    const d2 cz = {co[2 * q], co[2 * q + 1]};
    const d2 c1 = {co[K + 2 * q], co[K + 2 * q + 1]};
    const d2 c2 = {co[2 * K + 2 * q], co[2 * K + 2 * q + 1]};
    double s0 = 0.0, s1 = 0.0, g0 = 0.0, g1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        const d2 b = u2[i];
        d2 v = z[i];
        v.x = cz.x * v.x;
        v.y = cz.y * v.y;
        if (u1) {
            const d2 a = u1[i];
            v.x = __builtin_fma(-c1.x, a.x, v.x);
            v.y = __builtin_fma(-c1.y, a.y, v.y);
        }
        v.x = __builtin_fma(-c2.x, b.x, v.x);
        v.y = __builtin_fma(-c2.y, b.y, v.y);
        if (TARGET && tgt[i >> sh]) v.x = v.y = 0.0;
        z[i] = v;
        s0 = __builtin_fma(v.x, v.x, s0);
        s1 = __builtin_fma(v.y, v.y, s1);
        g0 = __builtin_fma(v.x, b.x, g0);
        g1 = __builtin_fma(v.y, b.y, g1);
    }
    flat_sum(s0, s1, half, red, part + (size_t)blockIdx.x * K);
    flat_sum(g0, g1, half, red, part + ((size_t)kMaxGrid + blockIdx.x) * K);
}

// partial: ||z_c||^2.  TARGET: of D z, and z <- D z in place (kfsp_block_combine may read that column: mx = m + 2)
template <bool TARGET>
__global__ __launch_bounds__(kBlock) void k_bnorm(int64_t npairs, int half, typename std::conditional<TARGET, d2, const d2>::type *__restrict__ z,
                                                  double *__restrict__ part, const uint8_t *__restrict__ tgt, int sh)
{
    __shared__ double red[8 * K];
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        d2 v = z[i];
        if constexpr (TARGET) {
            if (tgt[i >> sh]) {
                v.x = v.y = 0.0;
                z[i] = v;
            }
        }
        a0 = __builtin_fma(v.x, v.x, a0);
        a1 = __builtin_fma(v.y, v.y, a1);
    }
    flat_sum(a0, a1, half, red, part + (size_t)blockIdx.x * K);
}

// x <- D x: +0.0 on the rows of the set (kfsp_set_block's W, kfsp_spmm's X and Y)
__global__ __launch_bounds__(kBlock) void k_btarget_zero(int64_t npairs, int sh, const uint8_t *__restrict__ tgt, d2 *__restrict__ x)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock)
        if (tgt[i >> sh]) x[i] = d2{0.0, 0.0};
}

// partial: the sum of y_c over the rows of the set (the flux mode of kfsp_block_begin), in the lane and block order of the kernels above
__global__ __launch_bounds__(kBlock) void k_bhit(int64_t npairs, int half, int sh, const uint8_t *__restrict__ tgt, const d2 *__restrict__ y,
                                                 double *__restrict__ part)
{
    __shared__ double red[8 * K];
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        if (tgt[i >> sh]) {
            const d2 v = y[i];
            a0 += v.x;
            a1 += v.y;
        }
    }
    flat_sum(a0, a1, half, red, part + (size_t)blockIdx.x * K);
}

// the caller's flags (stage[state], any non-zero byte) -> one byte 0 / 1 per row of the internal order; rows in [n, rows)
// read "keep"
__global__ __launch_bounds__(kBlock) void k_btarget_pack(int64_t n, int64_t rows, const uint8_t *__restrict__ stage,
                                                         const int32_t *__restrict__ perm, uint8_t *__restrict__ tgt)
{
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kBlock)
        tgt[r] = r < n && stage[perm ? perm[r] : r] != 0 ? 1 : 0;
}

// W = max(sum_i coef_i u_i, 0) (DGEMV :444, clamp :447-449), partial: sum W (DASUM :450).  clamp = 0 (option block_clamp,
// signed observables of a backward solve): W = sum_i coef_i u_i as it comes out of the same fma chain, partial: sum |W|
__global__ __launch_bounds__(kBlock) void k_bcombine(int64_t npairs, int half, const double *__restrict__ U, int64_t ldc, int mx,
                                                     const double *__restrict__ coef, d2 *__restrict__ w, double *__restrict__ part,
                                                     int clamp)
{
    __shared__ double red[8 * K];
    const int q = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) % half);
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        d2 s = {0.0, 0.0};
        for (int j = 0; j < mx; ++j) {
            const d2 u = reinterpret_cast<const d2 *>(U + (size_t)j * ldc)[i];
            s.x = __builtin_fma(coef[j * K + 2 * q], u.x, s.x);
            s.y = __builtin_fma(coef[j * K + 2 * q + 1], u.y, s.y);
        }
        if (clamp) {
            s.x = s.x > 0.0 ? s.x : 0.0;
            s.y = s.y > 0.0 ? s.y : 0.0;
        }
        w[i] = s;
        a0 += clamp ? s.x : __builtin_fabs(s.x);
        a1 += clamp ? s.y : __builtin_fabs(s.y);
    }
    flat_sum(a0, a1, half, red, part + (size_t)blockIdx.x * K);
}

// k_bcombine, and beside it J <- J + sum_i cj_i u_i (option block_integral: the time integral of the step from the same
// basis).  Per element one pass over j: u is loaded once and feeds two fma chains - s from +0.0 (then W's clamp), r from the
// old J element, j ascending, never clamped.  The partials are those of W alone, summed as k_bcombine sums them.
__global__ __launch_bounds__(kBlock) void k_bcombine_int(int64_t npairs, int half, const double *__restrict__ U, int64_t ldc, int mx,
                                                         const double *__restrict__ coef, const double *__restrict__ cj,
                                                         d2 *__restrict__ w, d2 *__restrict__ jint, double *__restrict__ part, int clamp)
{
    __shared__ double red[8 * K];
    const int q = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) % half);
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        d2 s = {0.0, 0.0};
        d2 r = jint[i];
        for (int j = 0; j < mx; ++j) {
            const d2 u = reinterpret_cast<const d2 *>(U + (size_t)j * ldc)[i];
            s.x = __builtin_fma(coef[j * K + 2 * q], u.x, s.x);
            s.y = __builtin_fma(coef[j * K + 2 * q + 1], u.y, s.y);
            r.x = __builtin_fma(cj[j * K + 2 * q], u.x, r.x);
            r.y = __builtin_fma(cj[j * K + 2 * q + 1], u.y, r.y);
        }
        if (clamp) {
            s.x = s.x > 0.0 ? s.x : 0.0;
            s.y = s.y > 0.0 ? s.y : 0.0;
        }
        w[i] = s;
        jint[i] = r;
        a0 += clamp ? s.x : __builtin_fabs(s.x);
        a1 += clamp ? s.y : __builtin_fabs(s.y);
    }
    flat_sum(a0, a1, half, red, part + (size_t)blockIdx.x * K);
}

// caller's column-major block (stage[c * n + i]) -> row-interleaved rows of the internal order, and back
// (lds: doubles between the columns of stage, >= n)
__global__ __launch_bounds__(kBlock) void k_bpack(int64_t n, int k, int kp, const double *__restrict__ stage, int64_t lds,
                                                  const int32_t *__restrict__ perm, double *__restrict__ X)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n * kp; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / kp;
        const int c = (int)(i - r * kp);
        X[i] = c < k ? stage[(int64_t)c * lds + (perm ? perm[r] : r)] : 0.0;
    }
}

__global__ __launch_bounds__(kBlock) void k_bunpack(int64_t n, int k, int kp, const double *__restrict__ X,
                                                    const int32_t *__restrict__ iperm, double *__restrict__ stage, int64_t lds)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n * k; i += (int64_t)gridDim.x * kBlock) {
        const int64_t c = i / n, r = i - c * n;
        stage[c * lds + r] = X[(iperm ? (int64_t)iperm[r] : r) * kp + c];
    }
}

// The per-column scalar work of a pass, one workgroup: 256 / K threads per column sum the block partials of the
// two quantities in a fixed order, then one thread per column applies the Arnoldi bookkeeping of `stage`.
// The second quantity's partials start off1 doubles behind the first's.  sums != null (a row partition): the sum stage
// alone - the 2 K column sums go to sums[0..K) and sums[K..2K) for the all-reduce, and the bookkeeping follows as a
// second launch on the reduced sums (part = sums, G = 1, off1 = K).
__global__ __launch_bounds__(kBlock) void k_bfinal(int stage, int j, int kp, int G, const double *__restrict__ part, int64_t off1,
                                                   double *__restrict__ sc, double break_tol, double *__restrict__ sums)
{
    constexpr int T = kBlock / K;
    const int c = threadIdx.x / T, i = threadIdx.x % T;
    double s0 = 0.0, s1 = 0.0;
    for (int g = i; g < G; g += T) {
        s0 += part[(size_t)g * K + c];
        s1 += part[(size_t)off1 + (size_t)g * K + c];
    }
    for (int o = T / 2; o >= 1; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
    }
    if (i != 0) return;
    if (sums) {
        sums[c] = s0;
        sums[K + c] = s1;
        return;
    }
    if (c >= kp) return;
    double *hb = sc + kHB, *nrm = sc + kNRM, *co = sc + kCO;
    double &brk = sc[kBRK + c], &gg = sc[kGG + c];
    switch (stage) {
    case kFinBegin: {
        const double n1 = sqrt(s0);
        nrm[K + c] = n1;
        brk = n1 > 0.0 ? 0.0 : -1.0;
        gg = 0.0;
        sc[kSQ1 + c] = s0;
        break;
    }
    case kFinDots: {
        double h1 = 0.0, h2 = 0.0, cz = 0.0, c1 = 0.0, c2 = 0.0;
        if (brk == 0.0) {
            const double nj = nrm[j * K + c];
            if (j >= 2) {
                const double np = nrm[(j - 1) * K + c];
                h1 = s0 / np / nj;                       // v_{j-1} . A v_j
                c1 = h1 / np;
            }
            h2 = s1 / nj / nj - h1 * gg;                 // v_j . (A v_j - h1 v_{j-1})
            cz = 1.0 / nj;
            c2 = h2 / nj;
        }
        hb[(j * 3 + 0) * K + c] = h1;
        hb[(j * 3 + 1) * K + c] = h2;
        co[c] = cz;
        co[K + c] = c1;
        co[2 * K + c] = c2;
        break;
    }
    case kFinNorm: {
        double n1 = 0.0;
        if (brk == 0.0) {
            n1 = sqrt(s0);
            const double nj = nrm[j * K + c];
            gg = n1 > 0.0 ? s1 / n1 / nj : 0.0;
            if (!(n1 > break_tol)) brk = (double)j;     // happy breakdown :249, this column only
        }
        hb[(j * 3 + 2) * K + c] = n1;
        nrm[(j + 1) * K + c] = n1;
        break;
    }
    case kFinAvn:
        sc[kAVN + c] = brk == 0.0 ? sqrt(s0) / nrm[j * K + c] : 0.0;
        break;
    default:
        sc[kWS + c] = s0;
        break;
    }
}

// ---- the small path: one workgroup of 1024 lanes per block column, rows below nact only
// the sum of v over the workgroup, wavefronts in a fixed order
__device__ __forceinline__ double small_sum(double v, double *red)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kSmallBlock / 64; ++w) s += red[w];
    return s;
}

// u_1 = W, beta = ||W_c|| and the start of the column's bookkeeping (k_bcopy_nrm + k_bfinal(kFinBegin))
__global__ __launch_bounds__(kSmallBlock) void k_bbegin_small(int nact, int kp, const double *__restrict__ w, double *__restrict__ u,
                                                              double *__restrict__ sc)
{
    __shared__ double red[kSmallBlock / 64];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int r = threadIdx.x; r < nact; r += kSmallBlock) {
        const double v = w[r * kp + c];
        u[r * kp + c] = v;
        a = __builtin_fma(v, v, a);
    }
    const double s0 = small_sum(a, red);
    if (threadIdx.x != 0) return;
    const double n1 = sqrt(s0);
    sc[kNRM + K + c] = n1;
    sc[kBRK + c] = n1 > 0.0 ? 0.0 : -1.0;
    sc[kGG + c] = 0.0;
    sc[kSQ1 + c] = s0;
}

// W_c = max(sum_i coef_i u_{i+1,c}, 0) and its sum: per element the operations of k_bcombine in its order, clamp included
__global__ __launch_bounds__(kSmallBlock) void k_bcombine_small(int nact, int kp, const double *__restrict__ U, int64_t ldc, int mx,
                                                                const double *__restrict__ coef, double *__restrict__ w,
                                                                double *__restrict__ sc, int clamp)
{
    __shared__ double red[kSmallBlock / 64];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int r = threadIdx.x; r < nact; r += kSmallBlock) {
        double s = 0.0;
        for (int j = 0; j < mx; ++j) s = __builtin_fma(coef[j * K + c], U[(size_t)j * ldc + r * kp + c], s);
        if (clamp) s = s > 0.0 ? s : 0.0;
        w[r * kp + c] = s;
        a += clamp ? s : __builtin_fabs(s);
    }
    const double s0 = small_sum(a, red);
    if (threadIdx.x == 0) sc[kWS + c] = s0;
}

// k_bcombine_small and the J update of k_bcombine_int: per element the same operations in the same order
__global__ __launch_bounds__(kSmallBlock) void k_bcombine_small_int(int nact, int kp, const double *__restrict__ U, int64_t ldc, int mx,
                                                                    const double *__restrict__ coef, const double *__restrict__ cj,
                                                                    double *__restrict__ w, double *__restrict__ jint,
                                                                    double *__restrict__ sc, int clamp)
{
    __shared__ double red[kSmallBlock / 64];
    const int c = blockIdx.x;
    double a = 0.0;
    for (int r = threadIdx.x; r < nact; r += kSmallBlock) {
        double s = 0.0;
        double v = jint[r * kp + c];
        for (int j = 0; j < mx; ++j) {
            const double u = U[(size_t)j * ldc + r * kp + c];
            s = __builtin_fma(coef[j * K + c], u, s);
            v = __builtin_fma(cj[j * K + c], u, v);
        }
        if (clamp) s = s > 0.0 ? s : 0.0;
        w[r * kp + c] = s;
        jint[r * kp + c] = v;
        a += clamp ? s : __builtin_fabs(s);
    }
    const double s0 = small_sum(a, red);
    if (threadIdx.x == 0) sc[kWS + c] = s0;
}

}  // namespace

// ---- what kfsp_block_host.hip launches, by function pointer (kfsp_block_dev.h)
// k_spmm of the stored forms (fmt: BlockPlan::fmt; part: the launch of a rank of a row partition)
SpmmFn spmm_kernel(int kp, int fmt, bool dots, bool part)
{
    return dispatch_kp_dots(kp, dots, [&](auto KP, auto DOTS) {
        return dispatch_bool(part, [&](auto PART) -> SpmmFn {
            switch (fmt) {
            case 1: return k_spmm<decltype(KP)::value, 1, decltype(DOTS)::value, decltype(PART)::value>;
            case 2: return k_spmm<decltype(KP)::value, 2, decltype(DOTS)::value, decltype(PART)::value>;
            case 5: return k_spmm<decltype(KP)::value, 5, decltype(DOTS)::value, decltype(PART)::value>;
            default: return k_spmm<decltype(KP)::value, 0, decltype(DOTS)::value, decltype(PART)::value>;
            }
        });
    });
}

SpmmFn spmm_box_kernel(int kp, int inst, bool dots)
{
    return dispatch_kp_dots(kp, dots, [&](auto KP, auto DOTS) {
        return dispatch_box_inst(inst, [](auto NS, auto PER) -> SpmmFn {
            return k_spmm_box<decltype(KP)::value, decltype(NS)::value, decltype(PER)::value, decltype(DOTS)::value>;
        });
    });
}

const BlockKernels &block_kernels()
{
    static const BlockKernels k{{k_bcopy_nrm<false>, k_bcopy_nrm<true>}, {k_bortho<false>, k_bortho<true>}, k_bnorm<false>, k_bnorm<true>,
                                k_btarget_zero, k_bhit, k_btarget_pack, k_bcombine, k_bcombine_int, k_bpack, k_bunpack, k_bfinal,
                                k_bbegin_small, k_bcombine_small, k_bcombine_small_int};
    return k;
}

}  // namespace kfsp
