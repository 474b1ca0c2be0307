// Several start vectors at once on ANY matrix-free box (option block_box = 2; include/kfsp.h, "several vectors at once";
// DESIGN.md 12, "Multi-factor boxes"): Y = A X with the interpreted row of kernel format 3 (row_box, kfsp_spmv_dev.h) -
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

}  // namespace

SpmmBoxgFn spmm_boxg_kernel(int kp, bool dots)
{
    return dispatch_kp_dots(kp, dots, [](auto KP, auto DOTS) -> SpmmBoxgFn { return k_spmm_boxg<decltype(KP)::value, decltype(DOTS)::value>; });
}

}  // namespace kfsp
