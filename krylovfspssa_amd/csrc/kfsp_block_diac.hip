// Several start vectors at once on a banded generator with dictionary-coded values (option block_dia_code; kernel format 9,
// DiaCodeDev in kfsp_internal.h; DESIGN.md 12, "Coded banded generators"): Y = A X with the off-diagonal values taken from
// the row's 8- or 16-byte record and the dictionaries in LDS instead of from nd value streams of 8 bytes per row.
//
// k_spmm_diac is k_spmm<KP, 1, DOTS, false> of kfsp_block.hip line by line - the XCD-aware trip mapping, trip_order, a
// 128-row group as two 64-row halves with one lane per row, kp accumulators, the DOTS partials through block_sum_cols into
// the same slots of a.part - with row_dia_blk's value loads replaced.  A dictionary entry is the very double the plain
// stream holds at that row (build_dia_code), the X rows and their clamp are row_dia_blk's, and the arithmetic is diag_row
// followed by one fma_row per diagonal, d ascending, compiled with contraction off: every column is bit-identical to the
// plain block product and to kfsp_spmv of that column.  Rows in [n, rows_act) are computed from what their records and
// DIAG hold, as the plain kernel computes them from its streams (the records cover all ld = rows_act rows).
//
// This file holds the instantiations on their own, so that the register allocation of the kernels of kfsp_block.hip
// stays what it was.
#pragma clang fp contract(off)

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));

// Banded row r from its record: ONE load of REC bytes brings every code of the row; code d lies where diac_word /
// diac_shift say (coded_vals, kfsp_spmv_dev.h, decodes the same words) and the value is dict[doff[d] + code], from the
// LDS image.  d is the loop counter: word index and shift are uniform.
template <int KP, int W, int REC>
__device__ __forceinline__ void row_diac_blk(const DiaDev &D, const DiaCodeDev &C, const double *__restrict__ X, int64_t r,
                                             double (&s)[KP])
{
    const int64_t ge = r & ~(int64_t)1;
    const int par = (int)(r & 1);
    const int64_t last = D.n - 1;
    auto xr = [&](int64_t p) -> int64_t { return (p < -1 ? -1 : (p > last ? last : p)) + par; };
    unsigned long long w0, w1 = 0ull;
    if (REC == 8) {
        w0 = C.rec[r];
    } else {
        const ull2 t = *reinterpret_cast<const ull2 *>(C.rec + 2 * r);
        w0 = t.x;
        w1 = t.y;
    }
    auto val = [&](int d) -> double {
        const unsigned long long w = (REC == 16 && diac_word(W, d) != 0) ? w1 : w0;
        return box_lds[C.doff[d] + (int)diac_code(W, w, d)];
    };
    double x0[KP], x1[KP];
    ld_row<KP>(X, xr(ge), x0);
    diag_row<KP>(D.diag[r], x0, s);
    int d = 0;
    for (; d + 2 <= D.nd; d += 2) {
        const double v0 = val(d);
        const double v1 = val(d + 1);
        ld_row<KP>(X, xr(ge + D.delta[d]), x0);
        ld_row<KP>(X, xr(ge + D.delta[d + 1]), x1);
        fma_row<KP>(v0, x0, s);
        fma_row<KP>(v1, x1, s);
    }
    for (; d < D.nd; ++d) {
        const double v0 = val(d);
        ld_row<KP>(X, xr(ge + D.delta[d]), x0);
        fma_row<KP>(v0, x0, s);
    }
}

// Every workgroup stages all dictionaries (doff[nd] doubles, <= kDiaCodeLds bytes) into dynamic LDS first; the host
// launches no more workgroups than are resident at once (launch_staged).  The reduction scratch is static LDS of its
// own: it never overlaps the image, so no barrier is owed between the last dictionary read and the first partial.
// amdgpu_waves_per_eu(1, 4): the grid never exceeds 1024 workgroups - 4 wavefronts per SIMD - so registers saved for a
// fifth wavefront buy nothing.  Without the bound the compiler kept the kp = 16 row at 80 VGPRs by recycling three
// 16-byte buffers, three loads of x in flight where the plain kernel (118 VGPRs) has sixteen: 1.23 x the plain time on c3.
// With it: 118 VGPRs, 0.85 x ("Coded banded generators").
template <int KP, int W, int REC, bool DOTS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_spmm_diac(SpmmArgs a, DiaCodeDev C)
{
    __shared__ double red[4 * KP];
    const int nent = C.doff[a.D.nd];
    for (int i = threadIdx.x; i < nent; i += kBlock) box_lds[i] = C.dict[i];
    __syncthreads();
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
        for (int h = 0; h < 2; ++h) {
            const int64_t r = (ct << 7) + h * 64 + lane;
            double s[KP];
            row_diac_blk<KP, W, REC>(a.D, C, a.X, r, s);
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

}  // namespace

SpmmDiacFn spmm_diac_kernel(int kp, int w, int rec, bool dots)
{
    return dispatch_kp_dots(kp, dots, [&](auto KP, auto DOTS) {
        return dispatch_diac(w, rec, [](auto W, auto REC) -> SpmmDiacFn {
            return k_spmm_diac<decltype(KP)::value, decltype(W)::value, decltype(REC)::value, decltype(DOTS)::value>;
        });
    });
}

}  // namespace kfsp
