// Device pieces of the GENERIC matrix-free block product (option block_box = 2; DESIGN.md 12, "Multi-factor boxes") that
// its two translation units share: kfsp_block_boxg.hip (Y = A X, k_spmm_boxg) and kfsp_block_adj.hip (Y = A^T X,
// k_spmm_boxg_t).  The row is the one of row_box (kfsp_spmv_dev.h, kernel format 3) in its run-time form - any box
// kfsp_set_matrix_box takes: up to 8 species, 16 reactions, 3 factors per propensity, any jump - read from the descriptor
// BoxDev (a uniform kernel argument: every index into it below is a compile-time constant after unrolling, so its fields
// arrive by scalar loads) and from the factor tables staged in LDS (box_lds).  What a row costs in look-ups - coordinates,
// propensities, the in-box tests - is paid once and serves all kp columns.
//
// Order of operations per column, fixed (tests/row_ref.py box_generic_exact; tests/box_generic_t_ref.py for A^T), every
// fused operation written out - the including files are compiled with contraction off:
//   a_k(z) = ((t_0[z] t_1[z]) t_2[z]), every multiply rounded, the factors in descriptor order;
//   dsum   = the sum from 0.0 of a_k(x) in the MODEL's reaction order (BoxDev::dorder);
//   s      = -(dsum X[r]) as one rounded multiply, then ONE fma per sorted position p ascending -
//   A X    : fma(a_p(x - nu_p), X[r + delta_p], s) when x - nu_p lies in the box, else fma(0.0, X[r], s);
//   A^T X  : fma(a_p(x), X[r - delta_p], s) when x + nu_p lies in the box, else fma(0.0, X[r], s).
// X is addressed by 64-bit row index: no reach limit (box_block_reach_ok is the single-factor kernels').  No read of X
// leaves the rows [0, n): an entry is read only when its state lies in the box.
#pragma once

#include "kfsp_block_dev.h"
#include "kfsp_box_dev.h"

namespace kfsp {

#if defined(__HIPCC__)
// The coordinates of a row, one named register each, and the coordinate of species s (uniform) picked by a select chain.
// Not an array: one that is written in a loop is still memory when the optimiser first meets the chain, which then turns
// the selects of its elements into ONE load at a selected address - and the array stays in scratch for good (a first
// build: 48 bytes per lane, a scratch load per look-up).
struct BoxgCo {
    int c0, c1, c2, c3, c4, c5, c6, c7;
};
static_assert(kBoxMaxS == 8, "BoxgCo names 8 species");

__device__ __forceinline__ int boxg_pick(const BoxgCo x, int s)
{
    int v = x.c0;
    v = (s == 1) ? x.c1 : v;
    v = (s == 2) ? x.c2 : v;
    v = (s == 3) ? x.c3 : v;
    v = (s == 4) ? x.c4 : v;
    v = (s == 5) ? x.c5 : v;
    v = (s == 6) ? x.c6 : v;
    v = (s == 7) ? x.c7 : v;
    return v;
}

// one step of the coordinate decode: species S of ns takes q mod dims[S] (q / dims[S] goes on), the last one what is left
__device__ __forceinline__ int boxg_coord(const BoxDev &B, int S, int ns, uint32_t &q)
{
    int c = 0;
    if (S + 1 < ns) {
        const int d = B.dims[S];
        uint32_t t = (uint32_t)((double)q * B.inv_dim[S]);
        int rem = (int)(q - t * (uint32_t)d);
        const int lo = rem < 0, hi = rem >= d;
        t = t - lo + hi;
        c = rem + (lo ? d : 0) - (hi ? d : 0);
        q = t;
    } else if (S + 1 == ns) {
        c = (int)q;
    }
    return c;
}

// Coordinates of row r (successive division by the box dimensions; exact: r < 2^31, one correction step), a_k(x) for the
// sorted positions k < nr and DIAG's dsum.
__device__ __forceinline__ void boxg_head(const BoxDev &B, int64_t r, BoxgCo &x, double (&ax)[kBoxMaxR], double &dsum)
{
    const int ns = B.ns, nr = B.nr;
    uint32_t q = (uint32_t)r;
    x.c0 = boxg_coord(B, 0, ns, q);
    x.c1 = boxg_coord(B, 1, ns, q);
    x.c2 = boxg_coord(B, 2, ns, q);
    x.c3 = boxg_coord(B, 3, ns, q);
    x.c4 = boxg_coord(B, 4, ns, q);
    x.c5 = boxg_coord(B, 5, ns, q);
    x.c6 = boxg_coord(B, 6, ns, q);
    x.c7 = boxg_coord(B, 7, ns, q);
#pragma unroll
    for (int k = 0; k < kBoxMaxR; ++k) {
        ax[k] = 0.0;
        if (k < nr) {
            double a = box_lds[B.dep_off[k][0] + boxg_pick(x, B.dep_s[k][0])];
#pragma unroll
            for (int i = 1; i < kBoxMaxDep; ++i)
                if (i < B.ndep[k]) a = a * box_lds[B.dep_off[k][i] + boxg_pick(x, B.dep_s[k][i])];
            ax[k] = a;
        }
    }
    dsum = 0.0;
#pragma unroll
    for (int q2 = 0; q2 < kBoxMaxR; ++q2) {
        if (q2 < nr) {
            const int k = B.dorder[q2];
            double a = ax[0];
#pragma unroll
            for (int j = 1; j < kBoxMaxR; ++j) a = (k == j) ? ax[j] : a;
            dsum = dsum + a;
        }
    }
}

// Does x + sign * nu_k lie in the box?  (sign = -1: the source state of the forward entry; +1: the target of the transposed)
template <int SIGN>
__device__ __forceinline__ bool boxg_inside(const BoxDev &B, const BoxgCo &x, int k)
{
    bool in = true;
#pragma unroll
    for (int i = 0; i < kBoxMaxDep; ++i) {
        if (i < B.nmov[k]) {
            const int v = boxg_pick(x, B.mov_s[k][i]) + SIGN * (int)B.mov_nu[k][i];
            in = in && v >= 0 && v < B.mov_dim[k][i];
        }
    }
    return in;
}

// Entry k of row r of A: the value a_k(x - nu_k) and the X row r + delta_k, or 0.0 against the row itself.  Where no
// factor species moves the value is a_k(x) as boxg_head made it (the same look-ups, the same bits).  The look-ups of a
// source outside the box go to the row's own coordinates: no LDS read leaves the tables.
__device__ __forceinline__ void boxg_entry(const BoxDev &B, const BoxgCo &x, const double (&ax)[kBoxMaxR], int64_t r, int k,
                                           double &a, int64_t &src)
{
    const bool in = boxg_inside<-1>(B, x, k);
    bool same = true;                                    // uniform: the descriptor is the same for every lane
#pragma unroll
    for (int i = 0; i < kBoxMaxDep; ++i)
        if (i < B.ndep[k]) same = same && B.dep_nu[k][i] == 0;
    double v = ax[k];
    if (!same) {
        v = box_lds[B.dep_off[k][0] + boxg_pick(x, B.dep_s[k][0]) - (in ? (int)B.dep_nu[k][0] : 0)];
#pragma unroll
        for (int i = 1; i < kBoxMaxDep; ++i)
            if (i < B.ndep[k]) v = v * box_lds[B.dep_off[k][i] + boxg_pick(x, B.dep_s[k][i]) - (in ? (int)B.dep_nu[k][i] : 0)];
    }
    a = in ? v : 0.0;
    src = in ? r + B.delta[k] : r;
}

// Entry k of row r of A^T: a_k(x) of the row's own coordinates against the X row of the state x + nu_k, r - delta_k.
__device__ __forceinline__ void boxg_entry_t(const BoxDev &B, const BoxgCo &x, const double (&ax)[kBoxMaxR], int64_t r, int k,
                                             double &a, int64_t &src)
{
    const bool in = boxg_inside<1>(B, x, k);
    a = in ? ax[k] : 0.0;
    src = in ? r - B.delta[k] : r;
}

// Row r applied to the kp columns of X.  The entries go in pairs, so that the X rows of two entries are in flight together
// (as in row_dia_blk); the order of the fmas is the order of the sorted positions.
template <int KP, bool TRANSPOSED>
__device__ __forceinline__ void row_boxg_blk(const BoxDev &B, const double *__restrict__ X, int64_t r, double (&s)[KP])
{
    BoxgCo x;
    double ax[kBoxMaxR], dsum;
    boxg_head(B, r, x, ax, dsum);
    const int nr = B.nr;
    double x0[KP], x1[KP];
    ld_row<KP>(X, r, x0);
    diag_row<KP>(dsum, x0, s);
#pragma unroll
    for (int k = 0; k < kBoxMaxR; k += 2) {
        if (k < nr) {
            double a0, a1;
            int64_t s0, s1;
            if (TRANSPOSED) boxg_entry_t(B, x, ax, r, k, a0, s0);
            else boxg_entry(B, x, ax, r, k, a0, s0);
            if (k + 1 < nr) {
                if (TRANSPOSED) boxg_entry_t(B, x, ax, r, k + 1, a1, s1);
                else boxg_entry(B, x, ax, r, k + 1, a1, s1);
                ld_row<KP>(X, s0, x0);
                ld_row<KP>(X, s1, x1);
                fma_row<KP>(a0, x0, s);
                fma_row<KP>(a1, x1, s);
            } else {
                ld_row<KP>(X, s0, x0);
                fma_row<KP>(a0, x0, s);
            }
        }
    }
}

// The kernel body both products share: k_spmm_box's skeleton (kfsp_block.hip) - the table image staged into dynamic LDS,
// the XCD-aware trip mapping and trip_order, one lane per row, two 64-row halves per 128-row trip, rows in [n, rows_act)
// written as +0.0, the DOTS partials through block_sum_cols in the image's LDS once every wavefront is done with it.
//
// The descriptor is read where it lies, in the kernel-argument segment, through a pointer the compiler is told nothing
// about once per row (the empty asm): left to itself it hoists every field of the descriptor and every scalar derived
// from one - about 1 500 values - out of the trip loop and spills them (a first build reported 1 470 spilled SGPRs and
// 48 bytes of scratch per lane in every instantiation).  Per row the fields arrive by scalar loads from the constant
// cache, next to the row's vector work.
struct BoxgArgs {
    SpmmArgs a;
    BoxDev b;                // by value: uniform, scalar loads
};
static_assert(sizeof(BoxgArgs) <= 4096, "a kernel takes at most 4 KB of arguments");
typedef const __attribute__((address_space(4))) BoxgArgs *boxg_args_t;

template <int KP, bool DOTS, bool TRANSPOSED>
__device__ __forceinline__ void spmm_boxg_body()
{
    constexpr int K = kBlockMaxK;
    const boxg_args_t args = (boxg_args_t)__builtin_amdgcn_kernarg_segment_ptr();   // the kernel's ONE argument, a BoxgArgs
    const SpmmArgs &a = *(const SpmmArgs *)&args->a;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < a.box_ntab; i += kBlock) box_lds[i] = a.box_tab[i];
    __syncthreads();
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
            if (r < a.D.n) {
                const __attribute__((address_space(4))) BoxDev *bp = &args->b;
                asm volatile("" : "+s"(bp));
                row_boxg_blk<KP, TRANSPOSED>(*(const BoxDev *)bp, a.X, r, s);
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
#endif

}  // namespace kfsp
