// Stand-alone check of the rule of the block product (block_plan / block_form / block_exchange_mode, csrc/kfsp_block_plan.h) and
// of the block state's record (BlockState, block state reset; csrc/kfsp_ctx.h): every combination of the flags against a literal
// restatement of the code the rule replaced - the refusal ladder of block_supported followed by the branch order of spmm() -
// family, status and text.  Built by tests/test_block_plan.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_block_plan.h"

#include <cstdio>
#include <cstring>

using namespace kfsp;

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            if (failures < 20) std::printf("line %d: %s\n", __LINE__, #x); \
            ++failures;                                             \
        }                                                           \
    } while (0)

struct Want {
    BlockKernel kernel;
    int code;
    const char *why;
};

// ---- the code before the rule, restated.  First block_supported (without the group head's recursion) ...
static Want supported_before(const BlockForm &f, bool generic)
{
    static const char *const kPartMsg = "several vectors at once: not with a row partition (communicator or group context) "
                                        "unless option block_partition = 1";
    if (f.partitioned) {
        if (!f.block_partition) return {kBlockNone, -12, kPartMsg};
        if (!f.collectives) return {kBlockNone, -12, "several vectors at once: this rank's communicator carries no collectives"};
        if (f.no_matrix) return {kBlockNone, -1, "no matrix set"};
        if (f.adjoint)
            return {kBlockNone, -12, "several vectors at once, option adjoint: not under a row partition (the transposed banded "
                                     "product reads the neighbour's generator rows, not only its rows of X)"};
        if (f.box)
            return {kBlockNone, -12, "several vectors at once: not for a matrix-free generator under a row partition "
                                     "(option box_store = 1 stores it)"};
    }
    if (f.no_matrix) return {kBlockNone, -1, "no matrix set"};
    if (f.box) {
        if (!f.block_box)
            return {kBlockNone, -12, "several vectors at once: not for a matrix-free generator (option box_store = 1 stores it, "
                                     "option block_box = 1 takes it matrix-free)"};
        if (generic) {
            if (!f.generic_walkable)
                return {kBlockNone, -12, "several vectors at once: the descriptor of this matrix-free box is not one the generic block "
                                         "kernels can walk (option box_store = 1 stores it)"};
            return {kBlockNone, 0, nullptr};
        }
        if (f.box_generic)
            return {kBlockNone, -12, "several vectors at once: not for the interpreted matrix-free product (option box_generic = 1)"};
        if (!f.box_fast)
            return {kBlockNone, -12, "several vectors at once: this matrix-free box has no single-factor form (option box_store = 1 stores it)"};
        return {kBlockNone, 0, nullptr};
    }
    if (!f.banded && !f.have_sell) return {kBlockNone, -12, "several vectors at once: no stored generator"};
    if (f.adjoint && !f.banded && !f.ell_resident)
        return {kBlockNone, -12, "several vectors at once, option adjoint: the transposed product of a SELL generator reads the reference "
                                 "arrays ADJ / OFFDIAG / DIAG, and none are resident for this one (kfsp_set_matrix_ell uploads them; "
                                 "option box_store = 1 stores a box as diagonals)"};
    return {kBlockNone, 0, nullptr};
}

// ... then spmm(): box_reach_check, spmm_staged, the coded kernels' selection (spmm_diac_for / spmm_diac_t_for), the ladder
static Want before(const BlockForm &f)
{
    static const char *const kAdjFormMsg = "several vectors at once, option adjoint: the generator is resident in no form the transposed product reads";
    const bool generic = f.box && f.block_box == 2 && (!f.box_fast || f.box_generic != 0);      // box_generic_path
    const Want s = supported_before(f, generic);
    if (s.code) return s;
    if (f.box) {
        if (!generic && !f.reach_ok)
            return {kBlockNone, -12, "several vectors at once: the entries of this matrix-free box reach further than 2^32 bytes "
                                     "at this block width (fewer columns, or option box_store = 1)"};
        if (generic) {
            if (!f.generic_walkable) return {kBlockNone, -12, kAdjFormMsg};
            return {f.adjoint ? kBlockBoxgT : kBlockBoxg, 0, nullptr};
        }
        if (!f.adjoint) return {kBlockBox, 0, nullptr};
        if (!f.adj_builds) return {kBlockNone, -12, kAdjFormMsg};
        return {kBlockBoxT, 0, nullptr};
    }
    if (f.adjoint) {
        if (f.banded) {
            if (block_dia_code_t_path(f.coded_on, f.block_dia_code, f.block_dia_code_adjoint, f.adjoint) && f.diac_walkable)
                return {kBlockDiacT, 0, nullptr};
            return {kBlockT, 0, nullptr};
        }
        if (!f.ell_resident) return {kBlockNone, -12, kAdjFormMsg};
        return {kBlockEllT, 0, nullptr};
    }
    if (block_dia_code_path(f.coded_on, f.block_dia_code, f.adjoint, f.small) && f.diac_walkable) return {kBlockDiac, 0, nullptr};
    return {kBlockSpmm, 0, nullptr};
}

static int exchange_before(bool comm, bool x_global, bool halo, bool split, bool has_comm_stream)
{
    int slot = 0;                                    // ctx->blk_info[7] = 0
    if (!comm) return slot;
    if (x_global) return slot;
    if (!halo) return 2;
    slot = 1;
    if (!split || !has_comm_stream) return slot;
    return 5;
}

int main()
{
    // ---- every combination of the flags: 2^21 of the booleans and 0 / 1 options x the 3 values of block_box
    bool reached[kBlockKernels] = {false};
    long cases = 0;
    for (unsigned bits = 0; bits < (1u << 19); ++bits)
        for (int64_t block_box = 0; block_box < 3; ++block_box) {
            auto b = [&](int i) { return (bits >> i & 1u) != 0; };
            const BlockForm f{b(0), b(1), b(2), b(3) ? 1 : 0, b(4), b(5), b(6), block_box, b(7) ? 1 : 0, b(8), b(9), b(10), b(11), b(12), b(13), b(14),
                              b(15), b(16), b(17) ? 1 : 0, b(18) ? 1 : 0, false, false};
            for (int small = 0; small < 2; ++small)
                for (int walk = 0; walk < 2; ++walk) {
                    BlockForm g = f;
                    g.small = small != 0;
                    g.diac_walkable = walk != 0;
                    const BlockPlan p = block_plan(g);
                    const Want w = before(g);
                    ++cases;
                    CHECK(p.kernel == w.kernel && p.code == w.code);
                    CHECK((p.why == nullptr) == (w.why == nullptr) && (!p.why || std::strcmp(p.why, w.why) == 0));
                    CHECK((p.code != 0) == (p.kernel == kBlockNone) && (p.code != 0) == (p.where != kRefuseNot));   // a refusal carries no kernel
                    reached[p.kernel] = true;
                    // what block_supported raises is what it raised, and nothing the product alone raised
                    const Want s = supported_before(g, g.box && g.block_box == 2 && (!g.box_fast || g.box_generic != 0));
                    CHECK((p.where == kRefuseContext) == (s.code != 0));
                    if (p.where == kRefuseWidth) CHECK(std::strcmp(p.why, kBlockReachMsg) == 0 && !g.reach_ok);
                    if (p.where == kRefuseProduct) CHECK(std::strcmp(p.why, kBlockAdjFormMsg) == 0);
                    // the coded kernels exactly where the two rules and the image say so
                    if (p.code == 0 && !g.box) {
                        CHECK((p.kernel == kBlockDiac) == (block_dia_code_path(g.coded_on, g.block_dia_code, g.adjoint, g.small) && g.diac_walkable));
                        CHECK((p.kernel == kBlockDiacT) ==
                              (block_dia_code_t_path(g.coded_on, g.block_dia_code, g.block_dia_code_adjoint, g.adjoint) && g.diac_walkable && g.banded));
                    } else {
                        CHECK(p.kernel != kBlockDiac && p.kernel != kBlockDiacT);
                    }
                    // the occupancy cache: one slot per staging family, the reductions in the image for the boxes alone
                    const bool box_family = p.kernel == kBlockBox || p.kernel == kBlockBoxT || p.kernel == kBlockBoxg || p.kernel == kBlockBoxgT;
                    const int staged = p.kernel == kBlockBox ? kStagedBox : p.kernel == kBlockBoxT ? kStagedBoxT : p.kernel == kBlockBoxg ? kStagedBoxg
                                     : p.kernel == kBlockBoxgT ? kStagedBoxgT : p.kernel == kBlockDiac ? kStagedDiac
                                     : p.kernel == kBlockDiacT ? kStagedDiacT : -1;
                    CHECK(p.staged == staged && p.lds_shared == box_family);
                    if (p.kernel == kBlockSpmm) CHECK(p.fmt == (g.banded ? (g.masked ? 2 : 1) : (g.sell_coded ? 5 : 0)));
                }
        }
    CHECK(cases == 3L * 4L * (1L << 19));
    for (int k = 0; k < kBlockKernels; ++k) CHECK(reached[k]);         // all nine families, and "none"
    static_assert(kBlockKernels == 10, "nine families and none");

    // ---- block_exchange_mode: the four outcomes of the inline code, over all inputs
    for (unsigned bits = 0; bits < 32; ++bits) {
        const bool comm = bits & 1, xg = bits & 2, halo = bits & 4, split = bits & 8, cs = bits & 16;
        CHECK(block_exchange_mode(comm, xg, halo, split, cs) == exchange_before(comm, xg, halo, split, cs));
    }

    // ---- block_form reads the fields it should: a default context, then one field at a time
    {
        kfsp_ctx *c = new kfsp_ctx();
        BlockForm f = block_form(c, 2);
        CHECK(f.no_matrix && !f.partitioned && !f.collectives && f.block_partition == 0 && !f.adjoint && !f.box && !f.box_fast);
        CHECK(f.block_box == 0 && f.box_generic == 0 && !f.generic_walkable && !f.adj_builds && f.reach_ok && !f.banded && !f.masked);
        CHECK(!f.have_sell && !f.sell_coded && !f.ell_resident && !f.coded_on && f.block_dia_code == 0 && f.block_dia_code_adjoint == 0);
        CHECK(!f.small && !f.diac_walkable);
        CHECK(block_plan(f).code == -1 && std::strcmp(block_plan(f).why, "no matrix set") == 0);
        c->ldv = 64;
        CHECK(!block_form(c, 2).no_matrix && block_plan(block_form(c, 2)).code == -12);       // no stored generator
        c->nranks = 2;
        CHECK(block_form(c, 2).partitioned && !block_form(c, 2).collectives);
        c->nranks = 1;
        c->use_comm = true;
        CHECK(block_form(c, 2).partitioned && block_form(c, 2).collectives);
        c->use_comm = false;
        c->opt_block_partition = 1;
        c->opt_adjoint = 1;
        c->opt_block_box = 2;
        c->opt_box_generic = 1;
        c->opt_block_dia_code = 1;
        c->opt_block_dia_code_adjoint = 1;
        f = block_form(c, 2);
        CHECK(f.block_partition == 1 && f.adjoint && f.block_box == 2 && f.box_generic == 1 && f.block_dia_code == 1 && f.block_dia_code_adjoint == 1);
        c->opt_adjoint = 0;
        c->have_sell = true;
        c->sell_coded = true;
        f = block_form(c, 2);
        CHECK(f.have_sell && f.sell_coded && block_plan(f).kernel == kBlockSpmm && block_plan(f).fmt == 5);
        c->opt_adjoint = 1;                                      // a backward SELL call asks for the reference arrays: none here
        CHECK(!block_form(c, 2).ell_resident && block_plan(block_form(c, 2)).code == -12);
        c->opt_adjoint = 0;
        // a coded banded image: 4 diagonals of 8-bit codes in 8-byte records, 128 rows, dictionaries of 40 doubles
        c->use_dia = true;
        c->dia_masked = true;
        CHECK(block_form(c, 2).banded && block_form(c, 2).masked && block_plan(block_form(c, 2)).fmt == 2);
        c->dia_masked = false;
        c->dia_coded = true;
        c->nd = 4;
        c->nchunks = 2;
        c->dia_ld = 128;
        c->dia_code_w = 8;
        c->dia_code_rec = 8;
        for (int d = 0; d <= 4; ++d) c->dia_doff[d] = 10 * d;
        f = block_form(c, 2);
        CHECK(f.coded_on && f.diac_walkable && block_plan(f).kernel == kBlockDiac && block_plan(f).staged == kStagedDiac);
        c->dia_code_w = 12;                                      // no form dispatch_diac knows
        CHECK(!block_form(c, 2).diac_walkable && block_plan(block_form(c, 2)).kernel == kBlockSpmm);
        c->dia_code_w = 8;
        c->dia_ld = 64;                                          // records for half a trip
        CHECK(!block_form(c, 2).diac_walkable);
        c->dia_ld = 128;
        c->opt_adjoint = 1;
        CHECK(block_plan(block_form(c, 2)).kernel == kBlockDiacT);
        c->opt_block_dia_code_adjoint = 0;
        CHECK(block_plan(block_form(c, 2)).kernel == kBlockT);
        c->opt_adjoint = 0;
        // the small pass keeps even kfsp_spmm off the coded kernel
        c->opt_block_small = 1;
        CHECK(small_path(c) && block_form(c, 2).small && block_plan(block_form(c, 2)).kernel == kBlockSpmm);
        c->blk_tgt = true;                                       // ... and a target set keeps every pass off the small one
        CHECK(!block_form(c, 2).small && block_plan(block_form(c, 2)).kernel == kBlockDiac);
        c->blk_tgt = false;
        c->opt_block_small = 0;
        // a box: the reach at this width (2^28 rows forward: 2^32 bytes at kp = 2 already)
        c->box.on = true;
        c->box.fast = true;
        c->opt_box_generic = 0;
        c->opt_block_box = 1;
        c->delta[0] = -1;
        c->delta[3] = 1 << 20;
        CHECK(block_form(c, 16).reach_ok && block_plan(block_form(c, 16)).kernel == kBlockBox);
        c->delta[3] = 1 << 28;
        f = block_form(c, 2);
        CHECK(f.box && f.box_fast && !f.reach_ok && block_plan(f).where == kRefuseWidth);
        CHECK(!f.coded_on);                                      // (dia_code_on excludes boxes)
        delete c;
    }

    // ---- the reset of the block state restores every field of the record
    {
        kfsp_ctx *c = new kfsp_ctx();
        c->blk_k = 3;
        c->blk_kp = 4;
        c->bv_kp = 8;
        c->bxg_kp = 16;
        c->blk_begin_m = 30;
        for (int i = 0; i < kInfoSlots; ++i) c->blk_info[i] = 100 + i;
        for (int a = 0; a < kStagedFamilies; ++a)
            for (int w = 0; w < 4; ++w)
                for (int d = 0; d < 2; ++d) c->blk_staged_occ[a][w][d] = 1 + a + w + d;
        c->blk_int = true;
        c->blk_tgt = true;
        c->btgt_states = 77;
        c->bhit_launches = 3;
        c->nd = 5;                                               // (not block state: stays)
        reset_block_state(c);                                    // the assignment of block_reset
        const BlockState fresh{};
        CHECK(c->blk_k == 0 && c->blk_kp == 0 && c->bv_kp == 0 && c->bxg_kp == 0 && c->blk_begin_m == 0);
        CHECK(std::memcmp(c->blk_info, fresh.blk_info, sizeof(fresh.blk_info)) == 0);
        CHECK(std::memcmp(c->blk_staged_occ, fresh.blk_staged_occ, sizeof(fresh.blk_staged_occ)) == 0);
        CHECK(!c->blk_int && !c->blk_tgt && c->btgt_states == 0 && c->bhit_launches == 0 && c->nd == 5);
        static_assert(sizeof(fresh.blk_info) == 8 * sizeof(int64_t), "the eight slots of kfsp_block_info");
        static_assert(kInfoOneLaunch == 0 && kInfoFmt == 1 && kInfoBeginLaunches == 2 && kInfoArnoldiLaunches == 3 && kInfoCombineLaunches == 4 &&
                      kInfoLdsBytes == 5 && kInfoAdjoint == 6 && kInfoExchange == 7, "the slots as host.py names them");
        delete c;
    }
    if (failures) return 1;
    std::printf("ok %ld cases\n", cases);
    return 0;
}
