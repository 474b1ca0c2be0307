// Backward solves on a banded generator with dictionary-coded values (option block_dia_code_adjoint beside block_dia_code
// and adjoint; kernel format 9 with the adjoint flag; DESIGN.md 12, "Coded banded generators, backward"): Y = A^T X with
// the off-diagonal values taken from the records of the SOURCE rows and the dictionaries in LDS instead of from nd value
// streams of 8 bytes per row at shifted rows.
//
// k_spmm_diac_t is k_spmm_t of kfsp_block_adj.hip line by line - the XCD-aware trip mapping, trip_order, a 128-row group
// as two 64-row halves with one lane per row, kp accumulators, finish_row and the DOTS partials through block_sum_cols
// into the same slots of a.part, rows in [n, rows_act) written as +0.0 - with the value loads replaced: entry d of row r
// is A(r - delta_d, r), code d of the record of row r - delta_d (diac_t_src, kfsp_block_dev.h).  Only the ONE 64-bit word
// of that record that holds code d is loaded: 8 bytes per diagonal also where a record has 16.  The nd words of a row
// come from nd different records, but the records a wavefront reads for diagonal d are 64 consecutive ones, those of the
// rows the same or a neighbouring wavefront reads for every other diagonal.  A dictionary entry is the very double the
// plain stream holds (build_dia_code), a source outside [0, n) counts as 0.0 against the row's own X row as in k_spmm_t,
// and the arithmetic is diag_row followed by one fma_row per diagonal, d ascending, compiled with contraction off:
// every column is bit-identical to the plain transposed block product.  DIAG comes from its stream (it stays resident
// also where dia_code_diag folded it into the records).  No read of rec, dict or X leaves the rows [0, n).
//
// This file holds the instantiations on their own, so that the register allocation of the kernels of kfsp_block_adj.hip
// and kfsp_block_diac.hip stays what it was.
#pragma clang fp contract(off)

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"

namespace kfsp {

namespace {

constexpr int K = kBlockMaxK;

// Row r < n of A^T.  A record of REC bytes holds at most REC * 8 / W codes, so the loop over the diagonals is unrolled to
// that count under the (uniform) test d < nd and the record words stay in registers: the loads of all nd words are issued
// together, before the first X row, then the X rows in pairs as row_diac_blk takes them.  A row without a source reads
// the word of its own record (in range) and the value is replaced by 0.0.
template <int KP, int W, int REC>
__device__ __forceinline__ void row_diac_t_blk(const DiaDev &D, const DiaCodeDev &C, const double *__restrict__ X, int64_t r,
                                               double (&s)[KP])
{
    constexpr int MAXD = REC * 8 / W;
    const int64_t n = D.n;
    const int nd = D.nd;
    double x0[KP], x1[KP];
    ld_row<KP>(X, r, x0);
    unsigned long long word[MAXD];
#pragma unroll
    for (int d = 0; d < MAXD; ++d)
        if (d < nd) word[d] = C.rec[diac_t_src(W, REC, r, D.delta[d], n, d).word];
    diag_row<KP>(D.diag[r], x0, s);
    auto val = [&](int d, bool ok) -> double {
        const double v = box_lds[C.doff[d] + (int)diac_code(W, word[d], d)];
        return ok ? v : 0.0;
    };
#pragma unroll
    for (int d = 0; d < MAXD; d += 2) {
        if (d + 1 < nd) {
            const DiacTSrc q0 = diac_t_src(W, REC, r, D.delta[d], n, d);
            const DiacTSrc q1 = diac_t_src(W, REC, r, D.delta[d + 1], n, d + 1);
            const double v0 = val(d, q0.ok);
            const double v1 = val(d + 1, q1.ok);
            ld_row<KP>(X, q0.row, x0);
            ld_row<KP>(X, q1.row, x1);
            fma_row<KP>(v0, x0, s);
            fma_row<KP>(v1, x1, s);
        } else if (d < nd) {
            const DiacTSrc q0 = diac_t_src(W, REC, r, D.delta[d], n, d);
            const double v0 = val(d, q0.ok);
            ld_row<KP>(X, q0.row, x0);
            fma_row<KP>(v0, x0, s);
        }
    }
}

// Staging, the static reduction scratch and amdgpu_waves_per_eu(1, 4) are k_spmm_diac's (kfsp_block_diac.hip): every
// workgroup copies all dictionaries into dynamic LDS first, the host launches no more workgroups than are resident at
// once (launch_staged, family kStagedDiacT), and the grid never exceeds 4 wavefronts per SIMD, so registers saved for a
// fifth would only shorten the run of loads in flight.
template <int KP, int W, int REC, bool DOTS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 4))) void k_spmm_diac_t(SpmmArgs a, DiaCodeDev C)
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
                row_diac_t_blk<KP, W, REC>(a.D, C, a.X, r, s);
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

}  // namespace

SpmmDiacFn spmm_diac_t_kernel(int kp, int w, int rec, bool dots)
{
    return dispatch_kp_dots(kp, dots, [&](auto KP, auto DOTS) {
        return dispatch_diac(w, rec, [](auto W, auto REC) -> SpmmDiacFn {
            return k_spmm_diac_t<decltype(KP)::value, decltype(W)::value, decltype(REC)::value, decltype(DOTS)::value>;
        });
    });
}

}  // namespace kfsp
