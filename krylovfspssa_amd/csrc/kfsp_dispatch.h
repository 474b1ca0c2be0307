// Private: from run-time variants to kernel instantiations, for the single-vector product (kfsp_kernels.hip, kfsp_spmv_*.hip)
// and the block product (kfsp_block*.hip) alike: every helper hands its callable the case as std::integral_constant
// arguments.  Plain host code without a HIP call (tests/spmv_dispatch_check.cpp, tests/block_dispatch_check.cpp).
#pragma once

#include <type_traits>

namespace kfsp {

template <class F>
decltype(auto) dispatch_bool(bool on, F &&f)
{
    return on ? f(std::true_type{}) : f(std::false_type{});
}

// f(MODE) of a single-vector product kernel: 0 y = A x, 1 with one fused dot product, 2 with the norm of y, and anything
// else 3, two fused dot products (k_spmv, kfsp_spmv_dev.h)
template <class F>
decltype(auto) dispatch_mode(int mode, F &&f)
{
    switch (mode) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
    }
}

// f(species, slots per species) of the single-factor box instantiations that walk planes (pencils and slabs: the species
// count is the model's); inst = species * 16 + slots per species (BoxDev::pad, box_plan), anything else takes the widest one
template <class F>
decltype(auto) dispatch_box_walk_inst(int inst, F &&f)
{
    using std::integral_constant;
    switch (inst) {
    case 3 * 16 + 2: return f(integral_constant<int, 3>{}, integral_constant<int, 2>{});
    case 6 * 16 + 2: return f(integral_constant<int, 6>{}, integral_constant<int, 2>{});
    default: return f(integral_constant<int, 6>{}, integral_constant<int, 4>{});
    }
}

// ... and of every other single-factor box kernel: those, and two species with two slots
template <class F>
decltype(auto) dispatch_box_inst(int inst, F &&f)
{
    if (inst == 2 * 16 + 2) return f(std::integral_constant<int, 2>{}, std::integral_constant<int, 2>{});
    return dispatch_box_walk_inst(inst, f);
}

// f(bits per code, bytes per record) of the coded banded products (k_spmm_diac, kfsp_block_diac.hip; k_spmv format 9,
// kfsp_spmv_diac.hip) for the four forms dia_code_rule can choose.  Anything else reaches NO instantiation: the answer is a
// value-initialised result (a null kernel pointer), and the caller keeps the plain kernel.
template <class F>
auto dispatch_diac(int w, int rec, F &&f) -> decltype(f(std::integral_constant<int, 8>{}, std::integral_constant<int, 8>{}))
{
    using std::integral_constant;
    using R = decltype(f(integral_constant<int, 8>{}, integral_constant<int, 8>{}));
    if (w == 8 && rec == 8) return f(integral_constant<int, 8>{}, integral_constant<int, 8>{});
    if (w == 8 && rec == 16) return f(integral_constant<int, 8>{}, integral_constant<int, 16>{});
    if (w == 16 && rec == 8) return f(integral_constant<int, 16>{}, integral_constant<int, 8>{});
    if (w == 16 && rec == 16) return f(integral_constant<int, 16>{}, integral_constant<int, 16>{});
    return R{};
}

}  // namespace kfsp
