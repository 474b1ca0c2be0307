// Private: the device helpers the kernel files of the single-vector path share (kfsp_kernels.hip, kfsp_spmv_diac.hip,
// kfsp_spmv_box.hip): lane moves, wavefront and workgroup sums, the finish of a Pending scalar, streaming loads.
#pragma once

#include "kfsp_internal.h"

namespace kfsp {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

// v of a lane CTRL away (DPP: a register-file crossbar move, no LDS traffic); lanes the
// masks exclude and lanes without a source get 0
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_get(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, BANK_MASK, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, true);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_allreduce_sum(double v)
{
    // Sum of the 64 lanes, the same bits in every lane.  Row-shift / row-broadcast DPP
    // steps (the ds_bpermute of a shuffle butterfly goes through the LDS pipeline and is
    // ~5x slower, which the one-launch Arnoldi kernel pays four times per column):
    // prefix sums inside each row of 16 lanes, then lane 15 of every row is folded into
    // the next rows; lane 63 ends with the total, which is read back as a scalar.
    const double v1 = v + dpp_get<0x111, 0xf, 0xf>(v);          // row_shr:1
    const double v2 = v1 + dpp_get<0x112, 0xf, 0xf>(v);         // row_shr:2
    double w = v2 + dpp_get<0x113, 0xf, 0xf>(v);                // row_shr:3 -> sums of 4
    w += dpp_get<0x114, 0xf, 0xe>(w);                           // row_shr:4, banks 1-3
    w += dpp_get<0x118, 0xf, 0xc>(w);                           // row_shr:8, banks 2-3 -> lane 15 = row total
    w += dpp_get<0x142, 0xa, 0xf>(w);                           // row_bcast:15 into rows 1 and 3
    w += dpp_get<0x143, 0xc, 0xf>(w);                           // row_bcast:31 into rows 2 and 3
    const int lo = __builtin_amdgcn_readlane(__double2loint(w), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(w), 63);
    return __hiloint2double(hi, lo);
}

// Sum over the block, result in every thread.  red: 4 doubles of LDS.
__device__ __forceinline__ double block_allreduce_sum(double v, double *red)
{
    v = wave_allreduce_sum(v);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    const double t = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return t;
}

// Three sums with one barrier pair.  red: 12 doubles of LDS.
__device__ __forceinline__ void block_allreduce_sum3(double &a, double &b, double &c, double *red)
{
    a = wave_allreduce_sum(a);
    b = wave_allreduce_sum(b);
    c = wave_allreduce_sum(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wave] = a;
        red[4 + wave] = b;
        red[8 + wave] = c;
    }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[4] + red[5]) + (red[6] + red[7]);
    c = (red[8] + red[9]) + (red[10] + red[11]);
    __syncthreads();
}

// Finish a Pending scalar: every thread of every block performs the same
// additions in the same order.
__device__ __forceinline__ double finish_sum(Pending s, double *red)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < s.n; i += kBlock) a += s.p[i];
    return block_allreduce_sum(a, red);
}

// Three Pending scalars at once (loads of all three in flight together).
__device__ __forceinline__ void finish_sum3(Pending p, Pending q, Pending r, double &a, double &b, double &c,
                                            double *red)
{
    a = 0.0;
    b = 0.0;
    c = 0.0;
    const int n = max(p.n, max(q.n, r.n));
    for (int i = threadIdx.x; i < n; i += kBlock) {
        if (i < p.n) a += p.p[i];
        if (i < q.n) b += q.p[i];
        if (i < r.n) c += r.p[i];
    }
    block_allreduce_sum3(a, b, c, red);
}

template <bool NT>
__device__ __forceinline__ double ld_stream(const double *p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}
template <bool NT>
__device__ __forceinline__ int32_t ld_stream(const int32_t *p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}
template <bool NT>
__device__ __forceinline__ d2 ld_stream2(const double *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const d2 *>(p));
    return *reinterpret_cast<const d2 *>(p);
}
template <bool NT>
__device__ __forceinline__ i2 ld_stream2(const int32_t *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const i2 *>(p));
    return *reinterpret_cast<const i2 *>(p);
}

}  // namespace kfsp
