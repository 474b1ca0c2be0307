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
// Matrix-free boxes (option block_box, k_spmm_box below; DESIGN.md 12, "Matrix-free boxes"): the row of a single-factor box is rebuilt
// once - coordinates, {sum, valid} look-ups, one LDS read per entry - and applied to all kp columns, in the operation
// order of the single-vector matrix-free kernels (k_spmv format 4 and the pencil kernel, kfsp_spmv_dev.h, kfsp_spmv_box.hip).
// Multi-factor boxes (option block_box = 2; DESIGN.md 12, "Multi-factor boxes"): every other matrix-free box, and any box
// under box_generic = 1, takes the interpreted row of kernel format 3 - k_spmm_boxg (kfsp_block_boxg.hip), k_spmm_boxg_t
// (kfsp_block_adj.hip), the row code in kfsp_boxg_dev.h; box_generic_path() and spmm_staged() below.  Values 0 and 1 of the
// option mean what they always meant.
//
// Small generators (option block_small; DESIGN.md 12, "Small generators"): where the single-vector path takes its
// one-launch pass (<= kSmallRows rows, a banded or plain SELL image, no partition), a block step is three launches of
// one 1024-lane workgroup per block column: k_bbegin_small, k_barnoldi_small (kfsp_kernels.hip: the pass of
// k_arnoldi_small, compiled from the same lines) and k_bcombine_small.
//
// Row partitions (option block_partition; DESIGN.md 12, "Row partitions").  OPT-IN: with the option at its default 0 a
// context with a communicator, a loop-back rank and a group head refuse every block call with -12, as they always have
// (existing callers and tests rely on that refusal).  With 1 the forward block product of the stored forms runs on the
// rank's rows: k_spmm takes local rows and addresses X by global row (SpmmArgs::row0), the source column is made visible
// before every product the way the single-vector path does it - the neighbours' strips of halo * kp doubles into the
// column's own margins (exchange_strips with a width), or an all-gather of L * kp doubles into d_bxg - and in halo mode
// the product is split into an interior launch beside the exchange and one boundary launch (overlapped_product, kfsp_host.h).
// Every block-partial sum is all-reduced before the bookkeeping reads it: k_bfinal sums the rank's partials in its fixed
// order into 2 K staging doubles, one comm_allreduce, k_bfinal again with G = 1 on the reduced sums.  The sequence of
// collectives of a call depends on k, m, the options and the agreed exchange mode only - never on a column's beta, its
// breakdown or the rows a rank owns.  Still refused (-12): option adjoint (the transposed banded product reads the
// neighbour's generator rows) and matrix-free boxes; block_small is not taken (small_path excludes partitions).
//
// Time integrals (option block_integral; DESIGN.md 12, "Time integrals").  While the option is on kfsp_set_block keeps a
// second block J of the block's shape (d_bint, +0.0) and block_combine takes kernels of its own, k_bcombine_int /
// k_bcombine_small_int: the pass over the basis that makes W also adds a second linear combination (the table behind coef,
// kfsp_block_integral.h) to J.  With the option off neither the kernels above nor any allocation or launch changes.
//
// Target sets (the target-set mode of kfsp_set_block; DESIGN.md 12, "Target sets").  While a set T is resident (d_btgt: one byte per row of
// the internal order) every block call works on the killed generator Q = D A D, D = diag(1 - 1_T), and no product kernel
// knows: the raw product's partials u . z are already those of Q because every basis column is 0 on T, and the TARGET
// instantiations of k_bcopy_nrm / k_bortho / k_bnorm put +0.0 on T before they sum.  kfsp_set_block stores D W, kfsp_spmm
// masks X and Y (k_btarget_zero), the flux mode of kfsp_block_begin sums one raw product over T (k_bhit + the sum stage of k_bfinal).  With no
// set resident the false instantiations run: the code as it was, no launch and no allocation more.
//
// Coded banded generators (option block_dia_code; DESIGN.md 12, "Coded banded generators").  OPT-IN: with 1 the forward
// product of a banded generator whose coded image the single-vector product reads (dia_code_on, kfsp_host.h) takes
// k_spmm_diac (kfsp_block_diac.hip) - one record per row and the dictionaries in LDS instead of nd value streams, the
// same bits - unless the call is a transposed one or the one-launch small pass (spmm_diac_for below).  Everything else
// keeps its kernel; with the option at 0 no launch, byte or report changes.  Option block_dia_code_adjoint = 1 beside it
// (OPT-IN as well; DESIGN.md 12, "Coded banded generators, backward") gives the transposed product of such a generator to
// k_spmm_diac_t (kfsp_block_diac_t.hip; spmm_diac_t_for below), the same bits as k_spmm_t; at 0 k_spmm_t runs as ever.
#pragma clang fp contract(off)

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"
#include "kfsp_boxg_dev.h"
#include "kfsp_host.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <type_traits>

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

// per-column scalars of a pass (d_bscal), K entries each
constexpr int kHB = 0;                          // [(kMMax + 2) * 3][K]: H(j-1,j), H(j,j), H(j+1,j) of column j
constexpr int kNRM = kHB + (kMMax + 2) * 3 * K; // [kMMax + 3][K]: ||u_j||
constexpr int kCO = kNRM + (kMMax + 3) * K;     // [3][K]: the update coefficients of the column in progress
constexpr int kGG = kCO + 3 * K;                // [K]: v_j . v_{j-1}
constexpr int kBRK = kGG + K;                   // [K]: 0 running, j broke down after column j, -1 skipped
constexpr int kAVN = kBRK + K;                  // [K]
constexpr int kWS = kAVN + K;                   // [K]
constexpr int kCMB = kWS + K;                   // [kMMax + 3][K]: combine coefficients
constexpr int kSQ1 = kCMB + (kMMax + 3) * K;    // [K]: ||u_1||^2 (what k_barnoldi_small starts from)
constexpr int kScal = kSQ1 + K;
constexpr int kSmallBlock = 1024;               // lanes of a small-path workgroup

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

enum { kFinBegin = 0, kFinDots = 1, kFinNorm = 2, kFinAvn = 3, kFinWsum = 4 };

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

// ---- host side
const char *const kAdjFormMsg = "several vectors at once, option adjoint: the generator is resident in no form the transposed product reads";

int kp_of(int k) { return k <= 2 ? 2 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16)); }

int spmm_fmt(const kfsp_ctx *c) { return c->use_dia ? (c->dia_masked ? 2 : 1) : (c->sell_coded ? 5 : 0); }
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

// The small path is taken where kfsp_arnoldi (qiop = 2) takes k_arnoldi_small on this context (kfsp_api.cpp), short of
// coded SELL columns: those stay on the multi-launch path.  So does every backward pass (option adjoint): k_barnoldi_small
// has the forward product compiled in.  And every pass under a target set (the target-set mode of kfsp_set_block): the masks live in the
// streaming kernels of the general path.
bool small_path(const kfsp_ctx *c)
{
    return c->opt_block_small != 0 && !c->blk_tgt && c->opt_adjoint == 0 && c->opt_small != 0 && c->opt_fused != 0 && !c->use_comm && !c->group && !c->box.on &&
           c->nchunks * kChunk <= kSmallRows && (c->use_dia || (c->have_sell && !c->sell_coded)) && c->slots < (1LL << 31);
}

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
    hipLaunchKernelGGL(k_btarget_zero, dim3(flat_grid(ctx, kp)), dim3(kBlock), 0, ctx->stream, red_pairs(ctx, kp), kp_index(kp),
                       ctx->d_btgt.p, pairs(col));
}

// k_spmm of the stored forms (fmt: spmm_fmt; part: the launch of a rank of a row partition)
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

// Option block_box = 2: the generic kernels (k_spmm_boxg, kfsp_block_boxg.hip; k_spmm_boxg_t, kfsp_block_adj.hip) answer
// for a box without the single-factor form and for any box under box_generic = 1.  Read at every block call.
bool box_generic_path(const kfsp_ctx *c) { return c->box.on && c->opt_block_box == 2 && (!c->box.fast || c->opt_box_generic != 0); }

// In the block layout a reach of delta rows is 8 kp delta bytes, and the single-factor kernels (k_spmm_box, k_spmm_box_t)
// address X as scalar base + unsigned 32-bit lane offset: the backward plus the forward reach plus one 128-row group must
// stay below 2^32 bytes.
bool box_block_reach_ok(const kfsp_ctx *c, int kp)
{
    const int64_t back = std::max<int64_t>(0, -(int64_t)c->delta[0]), fwd = std::max<int64_t>(0, (int64_t)c->delta[c->nd - 1]);
    return (back + fwd + 128) * 8 * (int64_t)kp < (1LL << 32);
}

// ... refused where a block of this width meets those kernels (box_generic is read at every call: a block set under the
// generic kernels, which address X by 64-bit row index, may meet the single-factor ones later)
int box_reach_check(kfsp_ctx *c, int kp)
{
    if (!c->box.on || box_generic_path(c) || box_block_reach_ok(c, kp)) return 0;
    return fail(c, -12, "several vectors at once: the entries of this matrix-free box reach further than 2^32 bytes "
                        "at this block width (fewer columns, or option box_store = 1)");
}

// One launch of a kernel that stages a table image of `image_bytes` into dynamic LDS.  Every workgroup copies the image
// first, so no more workgroups are launched than are resident at once (the rule of the single-vector product,
// run_product): the runtime says how many fit, asked once per family, width and variant (blk_staged_occ).  The
// reductions of the box kernels reuse the image's LDS: never less than 4 kp doubles of it; the coded banded kernel keeps
// its reduction scratch apart (static LDS) and asks for the dictionaries alone (staged_lds: the dynamic LDS of the launch).
// Returns the grid.
size_t staged_lds(StagedFamily fam, size_t image_bytes, int kp)
{
    return fam == kStagedDiac || fam == kStagedDiacT ? image_bytes : std::max<size_t>(image_bytes, (size_t)4 * kp * sizeof(double));
}

template <class... Args>
int launch_staged(kfsp_ctx *ctx, StagedFamily fam, int kp, bool dots, int64_t trips, size_t image_bytes, void (*kern)(Args...),
                  const Args &...args)
{
    const size_t lds = staged_lds(fam, image_bytes, kp);
    int &occ = ctx->blk_staged_occ[fam][kp_index(kp)][dots ? 1 : 0];
    if (occ == 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kBlock, lds) != hipSuccess || occ < 1)) occ = 1;
    const int g = product_grid(trips, ctx->opt_grid, std::min<int64_t>(1024, (int64_t)256 * occ));
    hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(kBlock), lds, ctx->stream, args...);
    return g;
}

// The block product of a matrix-free box, forward or transposed: the table pointers of `a`, then the kernel of the
// family.  The single-factor kernels stage the whole image and read the descriptor behind it; the generic ones stage
// the head and the factor tables only and take the box descriptor by value behind SpmmArgs (BoxgArgs).  -1: the
// descriptor is not one the family can walk (block_supported refuses that first).
int spmm_staged(kfsp_ctx *ctx, int kp, bool dots, bool transposed, SpmmArgs &a)
{
    a.box_tab = ctx->d_box.p;
    if (box_generic_path(ctx)) {
        a.box_ntab = box_generic_image(ctx->box.dev);
        a.box_fast = nullptr;
        if (a.box_ntab == 0) return -1;
        return launch_staged(ctx, transposed ? kStagedBoxgT : kStagedBoxg, kp, dots, a.trips, (size_t)a.box_ntab * sizeof(double),
                             transposed ? spmm_boxg_t_kernel(kp, dots) : spmm_boxg_kernel(kp, dots), BoxgArgs{a, ctx->box.dev});
    }
    a.box_ntab = ctx->box.dev.ntab;
    a.box_fast = reinterpret_cast<const BoxFast *>(ctx->d_box.p + (ctx->box.lds_bytes / sizeof(double)));
    if (!transposed) return launch_staged(ctx, kStagedBox, kp, dots, a.trips, ctx->box.lds_bytes, spmm_box_kernel(kp, ctx->box.dev.pad, dots), a);
    BoxAdjDev b;
    if (!box_adj_build(ctx->box.dev, b)) return -1;
    return launch_staged(ctx, kStagedBoxT, kp, dots, a.trips, ctx->box.lds_bytes, spmm_box_t_kernel(kp, ctx->box.dev.pad, dots), a, b);
}

// The coded banded image is what the coded block kernels walk: records for every row a trip touches, all codes of a row
// inside its record, the dictionaries within the LDS budget.
bool diac_image_walkable(const kfsp_ctx *c, int64_t trips)
{
    const int w = c->dia_code_w, rec = c->dia_code_rec, nd = c->nd;
    if (nd < 1 || nd > kMaxDiag || w < 1 || nd * w > rec * 8 || c->dia_ld < trips * 128) return false;
    return c->dia_doff[nd] >= 1 && (int64_t)c->dia_doff[nd] * 8 <= kDiaCodeLds;
}

// Option block_dia_code: the kernel that reads the coded banded image for this call, or null - the rule of
// block_dia_code_path (kfsp_host.h), a form dispatch_diac knows, and an image the kernel can walk.  Null: the plain
// kernel runs, as it always has.  Read at every block call.
SpmmDiacFn spmm_diac_for(const kfsp_ctx *c, int kp, bool dots, int64_t trips)
{
    if (!block_dia_code_path(dia_code_on(c), c->opt_block_dia_code, c->opt_adjoint != 0, small_path(c))) return nullptr;
    if (!diac_image_walkable(c, trips)) return nullptr;
    return spmm_diac_kernel(kp, c->dia_code_w, c->dia_code_rec, dots);
}

// Option block_dia_code_adjoint: the same for the transposed product - the rule of block_dia_code_t_path (kfsp_host.h),
// the same image guards (k_spmm_diac_t reads records of rows below n only; the bound on dia_ld holds all the more).
// Null: k_spmm_t runs, as it always has.  Read at every block call.
SpmmDiacFn spmm_diac_t_for(const kfsp_ctx *c, int kp, bool dots, int64_t trips)
{
    if (!block_dia_code_t_path(dia_code_on(c), c->opt_block_dia_code, c->opt_block_dia_code_adjoint, c->opt_adjoint != 0)) return nullptr;
    if (!diac_image_walkable(c, trips)) return nullptr;
    return spmm_diac_t_kernel(kp, c->dia_code_w, c->dia_code_rec, dots);
}

// The reference arrays in the order the device keeps its vectors: the relabelled copies under the internal state order.
bool ell_adj_args(const kfsp_ctx *ctx, EllAdjDev &e)
{
    const DevBuf<int32_t> &adj = ctx->perm_on ? ctx->d_ell_adj2 : ctx->d_ell_adj;
    const DevBuf<double> &off = ctx->perm_on ? ctx->d_ell_off2 : ctx->d_ell_off;
    const DevBuf<double> &diag = ctx->perm_on ? ctx->d_ell_diag2 : ctx->d_ell_diag;
    if (!adj.p || !off.p || !diag.p || !ell_adj_resident(ctx->n, ctx->ell_cols, ctx->ell_ld, ctx->ell_bw, adj.cap, off.cap, diag.cap))
        return false;
    e = EllAdjDev{adj.p, off.p, diag.p, ctx->n, ctx->ell_ld, ctx->ell_bw};
    return true;
}

// Y = A X, or A^T X under option adjoint (block columns of width kp); dots: partials of ua . Y and ub . Y in *G slots.
// x: row 0 of the source column.  The transposed product (kfsp_block_adj.hip) takes the grid of the forward product of
// the same form.  Under a row partition (forward stored forms only, block_supported) the source is made visible first -
// the strips into x's own margins, or all blocks gathered into d_bxg - unless x_global says that x is row 0 of a whole
// block every rank already holds (kfsp_spmm).  blk_info[7] records how.
int spmm(kfsp_ctx *ctx, int kp, const double *x, double *Y, const double *ua, const double *ub, bool dots, int *G, bool x_global = false)
{
    SpmmArgs a;
    generator_args(ctx, a.A, a.D);
    a.X = x;
    a.Y = Y;
    a.ua = ua;
    a.ub = ub;
    a.part = ctx->d_bpart.p;
    a.trips = spmm_trips(ctx);
    a.trip_order = ctx->trip_order_n == a.trips ? ctx->d_trip_order.p : nullptr;
    a.rows_red = ctx->nchunks * kChunk;
    a.box_tab = nullptr;
    a.box_ntab = 0;
    a.box_fast = nullptr;
    a.row0 = 0;
    a.trip_begin = 0;
    a.trip_end = a.trips;
    a.trip_split = INT64_MAX;
    a.trip_jump = 0;
    ctx->blk_info[7] = 0;
    // option block_dia_code: slots 1 and 5 say, product by product, whether the coded kernel ran (9, its dynamic LDS) or
    // not (0, 0); with the option off nothing here writes them
    if (ctx->opt_block_dia_code) ctx->blk_info[1] = ctx->blk_info[5] = 0;
    hipStream_t st = ctx->stream;
    const int g = spmm_grid(ctx);
    *G = g;
    if (ctx->box.on) {
        if (int rc = box_reach_check(ctx, kp)) return rc;
        const int gs = spmm_staged(ctx, kp, dots, ctx->opt_adjoint != 0, a);
        if (gs < 0) return fail(ctx, -12, kAdjFormMsg);      // (block_supported refuses those first)
        *G = gs;
        return 0;
    }
    // a coded banded kernel of either direction: the dictionaries staged, slots 1 and 5 say so
    auto launch_coded = [&](StagedFamily fam, SpmmDiacFn coded) {
        DiaCodeDev C;
        dia_code_args(ctx, C);
        const size_t image = (size_t)C.doff[ctx->nd] * sizeof(double);
        *G = launch_staged(ctx, fam, kp, dots, a.trips, image, coded, a, C);
        ctx->blk_info[1] = 9;
        ctx->blk_info[5] = (int64_t)staged_lds(fam, image, kp);
    };
    if (ctx->opt_adjoint) {
        if (ctx->use_dia) {
            if (const SpmmDiacFn coded = spmm_diac_t_for(ctx, kp, dots, a.trips)) {
                launch_coded(kStagedDiacT, coded);           // "fmt 9, adjoint 1": k_spmm_diac_t
                return 0;
            }
            hipLaunchKernelGGL(spmm_t_kernel(kp, dots), dim3(g), dim3(kBlock), 0, st, a);
            return 0;
        }
        EllAdjDev e;
        if (!ell_adj_args(ctx, e)) return fail(ctx, -12, kAdjFormMsg);
        hipLaunchKernelGGL(spmm_ell_t_kernel(kp, dots), dim3(g), dim3(kBlock), 0, st, a, e);
        return 0;
    }
    if (const SpmmDiacFn coded = spmm_diac_for(ctx, kp, dots, a.trips)) {
        launch_coded(kStagedDiac, coded);
        return 0;
    }
    const SpmmFn kern = spmm_kernel(kp, spmm_fmt(ctx), dots, ctx->use_comm);
    auto launch = [&](int grid) { hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), 0, st, a); };
    if (!ctx->use_comm) {
        launch(g);
        return 0;
    }
    a.row0 = ctx->row0;
    if (x_global) {
        launch(g);
        return 0;
    }
    if (!ctx->use_halo) {
        if (int rc = comm_allgather(ctx, x, xg_row0(ctx, kp), (size_t)ctx->L * kp, st)) return rc;
        a.X = xg_row0(ctx, kp);
        ctx->blk_info[7] = 2;
        launch(g);
        return 0;
    }
    a.X = x - (size_t)ctx->row0 * kp;                        // global row g lies at x[(g - row0) * kp]
    ctx->blk_info[7] = 1;
    const ProductSplit ps = product_split(ctx->halo, ctx->L, a.trips, ctx->use_dia ? 128 : 64, ctx->opt_overlap);
    if (!ps.split || ctx->comm_stream == nullptr) {
        if (int rc = exchange_strips(ctx, x, st, kp)) return rc;
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
    if (int rc = overlapped_product(ctx, ps, a.trips, x, kp, 1024, launch_range, G)) return rc;
    ctx->blk_info[7] = 5;
    return 0;
}

// The scalar stage behind a producer of G block partials.  One rank: one launch, as ever.  Row partition: the rank's
// column sums in the same fixed order, one all-reduce of the 2 K sums, the bookkeeping on the reduced sums - on every
// rank, whatever its columns did.
int finalize(kfsp_ctx *ctx, int stage, int j, int kp, int G, double break_tol = 0.0)
{
    const int64_t off1 = (int64_t)kMaxGrid * K;
    if (!ctx->use_comm) {
        hipLaunchKernelGGL(k_bfinal, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, G, ctx->d_bpart.p, off1, ctx->d_bscal.p, break_tol,
                           (double *)nullptr);
        return 0;
    }
    double *sums = ctx->d_bpart.p + (size_t)2 * kMaxGrid * K;
    hipLaunchKernelGGL(k_bfinal, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, G, ctx->d_bpart.p, off1, ctx->d_bscal.p, break_tol, sums);
    if (int rc = comm_allreduce(ctx, sums, 2 * K, false, ctx->stream)) return rc;
    hipLaunchKernelGGL(k_bfinal, dim3(1), dim3(kBlock), 0, ctx->stream, stage, j, kp, 1, sums, (int64_t)K, ctx->d_bscal.p, break_tol,
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
        hipLaunchKernelGGL(k_bpack, dim3(pack_grid(nl * kp)), dim3(kBlock), 0, st, nl, k, kp, ctx->d_bstage.p, L, (const int32_t *)nullptr, col0);
        return 0;
    }
    const int64_t n = ctx->n;
    HIP_TRY(ctx->d_bstage.reserve((size_t)n * k, false));
    if (whole) HIP_TRY(hipMemsetAsync(ctx->d_bxg.p, 0, xg_len(ctx, kp) * sizeof(double), st));
    else HIP_TRY(hipMemsetAsync(col0 - (size_t)margin_rows(ctx) * kp, 0, col_len(ctx, kp) * sizeof(double), st));
    HIP_TRY(hipMemcpy2DAsync(ctx->d_bstage.p, (size_t)n * sizeof(double), W, (size_t)ld * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bpack, dim3(pack_grid(n * kp)), dim3(kBlock), 0, st, n, k, kp, ctx->d_bstage.p, n, ctx->perm_on ? ctx->d_perm.p : nullptr, col0);
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
        hipLaunchKernelGGL(k_bunpack, dim3(pack_grid(L * k)), dim3(kBlock), 0, st, L, k, kp, col0, (const int32_t *)nullptr, ctx->d_bstage.p, L);
        for (int c = 0; c < k; ++c)
            if (int rc = download_states(ctx, ctx->d_bstage.p + (size_t)c * L, W ? W + (size_t)c * ld : W, ctx->nloc)) return rc;
        return 0;
    }
    const int64_t n = ctx->n;
    HIP_TRY(ctx->d_bstage.reserve((size_t)n * k, false));
    hipLaunchKernelGGL(k_bunpack, dim3(pack_grid(n * k)), dim3(kBlock), 0, st, n, k, kp, col0, ctx->perm_on ? ctx->d_iperm.p : nullptr, ctx->d_bstage.p, n);
    HIP_TRY(hipMemcpy2DAsync(W, (size_t)ld * sizeof(double), ctx->d_bstage.p, (size_t)n * sizeof(double), (size_t)n * sizeof(double),
                             (size_t)k, hipMemcpyDeviceToHost, st));
    return 0;
}

// the block path's fence at the C boundary
template <class F>
int guarded(kfsp_ctx *ctx, F &&body) { return no_throw(ctx, body, "exception inside the block path"); }

}  // namespace

void block_release(kfsp_ctx *ctx)
{
    ctx->d_blk.release();
    ctx->d_bv.release();
    ctx->d_bstage.release();
    ctx->d_bscal.release();
    ctx->d_bpart.release();
    ctx->d_bxg.release();
    ctx->d_bint.release();
    ctx->d_bcj.release();
    ctx->d_bhit.release();
    ctx->d_bhsum.release();
    ctx->bhit_launches = 0;
    ctx->blk_int = false;
    ctx->blk_k = ctx->blk_kp = ctx->bv_kp = ctx->bxg_kp = ctx->blk_begin_m = 0;
    std::memset(ctx->blk_info, 0, sizeof(ctx->blk_info));
    std::memset(ctx->blk_staged_occ, 0, sizeof(ctx->blk_staged_occ));
}

void block_target_release(kfsp_ctx *ctx)
{
    ctx->d_btgt.release();
    ctx->blk_tgt = false;
    ctx->btgt_states = 0;
}

// Every refusal below is made from what all ranks of a partition share (options, the kind of generator), before the
// first collective of any block call: a rank that returned alone would leave its peers waiting in one.
int block_supported(kfsp_ctx *ctx)
{
    static const char *const kPartMsg = "several vectors at once: not with a row partition (communicator or group context) "
                                        "unless option block_partition = 1";
    if (ctx->group) {
        kfsp_ctx *r0 = group_rank0(ctx);
        if (!r0 || !r0->opt_block_partition) return fail(ctx, -12, kPartMsg);
        const int rc = block_supported(r0);
        if (rc) ctx->err = std::string(r0->err);
        return rc;
    }
    if (ctx->use_comm || ctx->nranks > 1 || ctx->loop || ctx->comm) {
        if (!ctx->opt_block_partition) return fail(ctx, -12, kPartMsg);
        if (!ctx->use_comm) return fail(ctx, -12, "several vectors at once: this rank's communicator carries no collectives");
        if (ctx->ldv == 0) return fail(ctx, -1, "no matrix set");
        if (ctx->opt_adjoint)
            return fail(ctx, -12, "several vectors at once, option adjoint: not under a row partition (the transposed banded "
                                  "product reads the neighbour's generator rows, not only its rows of X)");
        if (ctx->box.on)
            return fail(ctx, -12, "several vectors at once: not for a matrix-free generator under a row partition "
                                  "(option box_store = 1 stores it)");
    }
    if (ctx->ldv == 0) return fail(ctx, -1, "no matrix set");
    if (ctx->box.on) {
        if (!ctx->opt_block_box)
            return fail(ctx, -12, "several vectors at once: not for a matrix-free generator (option box_store = 1 stores it, "
                                  "option block_box = 1 takes it matrix-free)");
        if (box_generic_path(ctx)) {
            if (box_generic_image(ctx->box.dev) == 0)
                return fail(ctx, -12, "several vectors at once: the descriptor of this matrix-free box is not one the generic block "
                                      "kernels can walk (option box_store = 1 stores it)");
            return 0;
        }
        if (ctx->opt_box_generic)
            return fail(ctx, -12, "several vectors at once: not for the interpreted matrix-free product (option box_generic = 1)");
        if (!ctx->box.fast)
            return fail(ctx, -12, "several vectors at once: this matrix-free box has no single-factor form (option box_store = 1 stores it)");
        return 0;
    }
    if (!ctx->use_dia && !ctx->have_sell) return fail(ctx, -12, "several vectors at once: no stored generator");
    EllAdjDev e;
    if (ctx->opt_adjoint && !ctx->use_dia && !ell_adj_args(ctx, e))
        return fail(ctx, -12, "several vectors at once, option adjoint: the transposed product of a SELL generator reads the reference "
                              "arrays ADJ / OFFDIAG / DIAG, and none are resident for this one (kfsp_set_matrix_ell uploads them; "
                              "option box_store = 1 stores a box as diagonals)");
    return 0;
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
        hipLaunchKernelGGL(k_bbegin_small, dim3(kp), dim3(kSmallBlock), 0, ctx->stream, (int)(ctx->nchunks * kChunk), kp,
                           bcol(ctx->d_blk.p, ctx, kp, 0), bcol(ctx->d_bv.p, ctx, kp, 0), ctx->d_bscal.p);
        ctx->blk_info[2] = 1;
    } else {
        const int g = launch_flat(ctx, kp, ctx->blk_tgt ? k_bcopy_nrm<true> : k_bcopy_nrm<false>, pairs(bcol(ctx->d_blk.p, ctx, kp, 0)),
                                  pairs(bcol(ctx->d_bv.p, ctx, kp, 0)), ctx->d_bpart.p, ctx->d_btgt.p, kp_index(kp));
        if (int rc = finalize(ctx, kFinBegin, 1, kp, g)) return rc;
        ctx->blk_info[2] = 2;
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
    ctx->blk_info[0] = small ? 1 : 0;
    ctx->blk_info[1] = ctx->blk_info[5] = 0;
    ctx->blk_info[6] = ctx->opt_adjoint ? 1 : 0;
    ctx->blk_info[3] = small ? 1 : 4 * m + 3;
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
        ctx->blk_info[1] = fmt;
        ctx->blk_info[5] = (int64_t)lds;
    }
    for (int j = 1; j <= m && !small; ++j) {
        int g = 0;
        if (int rc = spmm(ctx, kp, u(j), u(j + 1), j >= 2 ? u(j - 1) : nullptr, u(j), true, &g)) return rc;
        if (int rc = finalize(ctx, kFinDots, j, kp, g)) return rc;
        const int gv = launch_flat(ctx, kp, tgt ? k_bortho<true> : k_bortho<false>, pairs(u(j + 1)), pairs(j >= 2 ? u(j - 1) : nullptr),
                                   pairs(u(j)), ctx->d_bscal.p + kCO, ctx->d_bpart.p, tgt, sh);
        if (int rc = finalize(ctx, kFinNorm, j, kp, gv, break_tol)) return rc;
    }
    if (!small) {
        // the extra product for AVNORM (:261-263) into the scratch column
        int g = 0;
        if (int rc = spmm(ctx, kp, u(m + 1), u(m + 2), nullptr, nullptr, false, &g)) return rc;
        // (two launches for a const: the set's instantiation writes D z back)
        const int gv = tgt ? launch_flat(ctx, kp, k_bnorm<true>, pairs(u(m + 2)), ctx->d_bpart.p, tgt, sh)
                           : launch_flat(ctx, kp, k_bnorm<false>, pairs(u(m + 2)), ctx->d_bpart.p, tgt, sh);
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
        if (integral) hipLaunchKernelGGL(k_bcombine_small_int, dim3(kp), dim3(kSmallBlock), 0, st, nact, kp, U, ldc, mx, cw, cj, w, J, ctx->d_bscal.p, clamp);
        else hipLaunchKernelGGL(k_bcombine_small, dim3(kp), dim3(kSmallBlock), 0, st, nact, kp, U, ldc, mx, cw, w, ctx->d_bscal.p, clamp);
    } else {
        const int g = integral ? launch_flat(ctx, kp, k_bcombine_int, U, ldc, mx, cw, cj, pairs(w), pairs(J), ctx->d_bpart.p, clamp)
                               : launch_flat(ctx, kp, k_bcombine, U, ldc, mx, cw, pairs(w), ctx->d_bpart.p, clamp);
        if (int rc = finalize(ctx, kFinWsum, 0, kp, g)) return rc;
    }
    ctx->blk_info[4] = small ? 1 : 2;
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
        ctx->blk_info[6] = ctx->opt_adjoint ? 1 : 0;
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
    for (int i = 0; i < 8; ++i) v[i] = ctx->blk_info[i];
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
        // the resident block is W, not D W (or D' W): it goes, and its J, as when the generator changes
        block_release(ctx);
        block_target_release(ctx);
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
            hipLaunchKernelGGL(k_btarget_pack, dim3(pack_grid(rows)), dim3(kBlock), 0, ctx->stream, n, rows, (const uint8_t *)stage.p,
                               ctx->perm_on ? (const int32_t *)ctx->d_perm.p : nullptr, ctx->d_btgt.p);
            e = hipStreamSynchronize(ctx->stream);
        }
        stage.release();
        if (e != hipSuccess) {
            block_target_release(ctx);
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
        const int gv = launch_flat(ctx, kp, k_bhit, kp_index(kp), ctx->d_btgt.p, pairs(y), ctx->d_bpart.p);
        // the sum stage of k_bfinal alone: the block partials in its fixed order (both of its sums read the same ones)
        hipLaunchKernelGGL(k_bfinal, dim3(1), dim3(kBlock), 0, st, (int)kFinWsum, 0, kp, gv, ctx->d_bpart.p, (int64_t)0, ctx->d_bscal.p, 0.0,
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
        ctx->blk_info[6] = ctx->opt_adjoint ? 1 : 0;
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
