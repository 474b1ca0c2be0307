// The single-vector product on dictionary-coded banded generators: k_spmv (kfsp_spmv_dev.h) instantiated for formats 9 and 10.
// Which kernel a product runs is decided on the host by dia_code_kernel (kfsp_dia_diag.h); here that answer becomes the launch.
#include "kfsp_dispatch.h"
#include "kfsp_spmv_dev.h"

namespace kfsp {

void launch_spmv_coded(int mode, int grid, const SpmvArgs &a, bool nt, const DiaCodeKernel &k, hipStream_t st)
{
    const SpmvFn fn = dispatch_mode(mode, [&](auto M) {
        return dispatch_bool(nt, [&](auto NT) -> SpmvFn {
            constexpr int MODE = decltype(M)::value;
            constexpr bool T = decltype(NT)::value;
            if (k.inner == 6) return k_spmv<MODE, T, 10, 8, 8, false, 6>;
            if (k.inner == 4) return k_spmv<MODE, T, 10, 8, 8, false, 4>;
            if (k.fmt == 10)
                return dispatch_bool(k.lanes, [&](auto LANES) -> SpmvFn {
                    if (k.w == 8) return k_spmv<MODE, T, 10, 8, 8, decltype(LANES)::value>;
                    return k_spmv<MODE, T, 10, 16, 8, decltype(LANES)::value>;
                });
            return dispatch_diac(k.w, k.rec, [](auto W, auto REC) -> SpmvFn { return k_spmv<MODE, T, 9, decltype(W)::value, decltype(REC)::value>; });
        });
    });
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), (size_t)k.lds_bytes, st, a);
}

}  // namespace kfsp
