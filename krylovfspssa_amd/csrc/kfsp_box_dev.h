// Device pieces of the single-factor matrix-free box product (BoxFast, kfsp_internal.h) that more than one
// translation unit needs: the single-vector kernels (kfsp_spmv_dev.h, kfsp_spmv_box.hip) and the block product (kfsp_block.hip).
#pragma once

#include "kfsp_internal.h"

namespace kfsp {

extern __shared__ double box_lds[];   // dynamic LDS: the factor tables of the matrix-free kernels, the dictionaries of the coded banded one

template <int NS, int PER>
struct BoxRegs {
    int koff8[NS][PER];    // byte offset in the LDS image of a_k(x_s - nu_k), less 8 x_s
    int delta8[NS][PER];   // byte offset in x of the source state relative to the row
    int df8[NS];           // byte offset of the species' {sum, valid bits} table
    int dims[NS];
    double inv_dim[NS];
    int bias8;             // bytes the wave's x base lies below its first row (>= the largest backward reach)
};

template <int NS, int PER>
__device__ __forceinline__ void box_load(const BoxFast *__restrict__ F, BoxRegs<NS, PER> &R)
{
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        R.dims[s] = __builtin_amdgcn_readfirstlane(F->dims[s]);
        R.df8[s] = __builtin_amdgcn_readfirstlane(F->df8[s]);
        const double inv = F->inv_dim[s];
        R.inv_dim[s] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(inv)),
                                        __builtin_amdgcn_readfirstlane(__double2loint(inv)));
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            R.koff8[s][j] = __builtin_amdgcn_readfirstlane(F->koff8[s][j]);
            R.delta8[s][j] = __builtin_amdgcn_readfirstlane(F->delta8[s][j]);
        }
    }
    R.bias8 = __builtin_amdgcn_readfirstlane(F->bias8);
}

// byte pointers that keep their address space through integer arithmetic (LDS reads, scalar-base global loads)
typedef const __attribute__((address_space(3))) char *lds_bytes_t;
typedef const __attribute__((address_space(1))) char *global_bytes_t;
typedef double __attribute__((ext_vector_type(2))) box_pair_t;
// One population count of one species in the LDS image, 16 bytes: { double dsum - the sum of the
// propensities that depend on this species; unsigned valid - bit e: entry e's source coordinate of this
// species is inside the box; unsigned pad }.

template <int NS, int PER>
__device__ __forceinline__ void box_df(const BoxRegs<NS, PER> &R, int c0, int c1, int c2, int c3, int c4, int c5,
                                       double &dsum, unsigned &valid)
{
    const lds_bytes_t lds = (lds_bytes_t)box_lds;
    {
        const lds_bytes_t f = lds + R.df8[0] + 16 * c0;
        dsum = *(const __attribute__((address_space(3))) double *)f;
        valid = *(const __attribute__((address_space(3))) unsigned *)(f + 8);
    }
#define KFSP_BOX_DF(S, VAR)                                                                            \
    if (NS > S) {                                                                                      \
        const lds_bytes_t f = lds + R.df8[NS > S ? S : 0] + 16 * VAR;                                  \
        dsum += *(const __attribute__((address_space(3))) double *)f;                                  \
        valid &= *(const __attribute__((address_space(3))) unsigned *)(f + 8);                         \
    }
    KFSP_BOX_DF(1, c1)
    KFSP_BOX_DF(2, c2)
    KFSP_BOX_DF(3, c3)
    KFSP_BOX_DF(4, c4)
    KFSP_BOX_DF(5, c5)
#undef KFSP_BOX_DF
}

}  // namespace kfsp
