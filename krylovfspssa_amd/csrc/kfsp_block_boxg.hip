// Several start vectors at once on ANY matrix-free box (option block_box = 2; include/kfsp.h, "several vectors at once";
// DESIGN.md 12, "Multi-factor boxes"): Y = A X with the interpreted row of kernel format 3 (row_box, kfsp_kernels.hip) -
// propensities of up to three factors, any jump, up to 16 reactions on up to 8 species.  The row code and the kernel
// body are kfsp_boxg_dev.h's, shared with the transposed product (k_spmm_boxg_t, kfsp_block_adj.hip); this file holds the
// forward instantiations on their own, so that the register allocation of the kernels of kfsp_block.hip stays what it was.
// Compiled with contraction off: column c of A X is bit-identical to kfsp_spmv (format 3) of column c, whatever the width.
#pragma clang fp contract(off)

#include "kfsp_boxg_dev.h"

namespace kfsp {

namespace {

template <int KP, bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm_boxg(BoxgArgs)
{
    spmm_boxg_body<KP, DOTS, false>();
}

typedef void (*SpmmBoxgFn)(BoxgArgs);

SpmmBoxgFn spmm_boxg_fn(int kp, bool dots)
{
    switch (kp) {
    case 2: return dots ? k_spmm_boxg<2, true> : k_spmm_boxg<2, false>;
    case 4: return dots ? k_spmm_boxg<4, true> : k_spmm_boxg<4, false>;
    case 8: return dots ? k_spmm_boxg<8, true> : k_spmm_boxg<8, false>;
    default: return dots ? k_spmm_boxg<16, true> : k_spmm_boxg<16, false>;
    }
}

}  // namespace

int spmm_boxg_resident(int kp, bool dots, size_t lds)
{
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, spmm_boxg_fn(kp, dots), kBlock, lds) != hipSuccess) nb = 1;
    return nb > 1 ? nb : 1;
}

void launch_spmm_boxg(int kp, bool dots, int grid, size_t lds, const SpmmArgs &a, const BoxDev &b, hipStream_t st)
{
    hipLaunchKernelGGL(spmm_boxg_fn(kp, dots), dim3((unsigned)grid), dim3(kBlock), lds, st, BoxgArgs{a, b});
}

}  // namespace kfsp
