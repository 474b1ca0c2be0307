// Private: THE rule of the block product (kfsp_block_host.hip) - which of the nine kernel families a block call runs, or why
// it is refused - from plain flags, the way product_format (kfsp_host.h) decides the single-vector product.  Plain inline
// host code: a stand-alone program walks every combination of the flags (tests/block_plan_check.cpp).
#pragma once

#include "kfsp_block_dev.h"
#include "kfsp_host.h"

namespace kfsp {

// The one-launch small pass is taken where kfsp_arnoldi (qiop = 2) takes k_arnoldi_small on this context (kfsp_api.cpp), short
// of coded SELL columns: those stay on the multi-launch path.  So does every backward pass (option adjoint): k_barnoldi_small
// has the forward product compiled in.  And every pass under a target set: the masks live in the streaming kernels of the
// general path.
inline bool small_path(const kfsp_ctx *c)
{
    return c->opt_block_small != 0 && !c->blk_tgt && c->opt_adjoint == 0 && c->opt_small != 0 && c->opt_fused != 0 && !c->use_comm && !c->group && !c->box.on &&
           c->nchunks * kChunk <= kSmallRows && (c->use_dia || (c->have_sell && !c->sell_coded)) && c->slots < (1LL << 31);
}

// In the block layout a reach of delta rows is 8 kp delta bytes, and the single-factor kernels (k_spmm_box, k_spmm_box_t)
// address X as scalar base + unsigned 32-bit lane offset: the backward plus the forward reach plus one 128-row group must
// stay below 2^32 bytes.  (The generic kernels address X by 64-bit row index.)
inline bool box_block_reach_ok(const kfsp_ctx *c, int kp)
{
    const int64_t back = std::max<int64_t>(0, -(int64_t)c->delta[0]), fwd = std::max<int64_t>(0, (int64_t)c->delta[c->nd - 1]);
    return (back + fwd + 128) * 8 * (int64_t)kp < (1LL << 32);
}

// The coded banded image is what the coded block kernels walk: one of dispatch_diac's forms, records for every row a trip
// touches (k_spmm_diac_t reads records of rows below n only: the bound holds all the more), all codes of a row inside its
// record, the dictionaries within the LDS budget.
inline bool diac_image_walkable(const kfsp_ctx *c)
{
    const int w = c->dia_code_w, rec = c->dia_code_rec, nd = c->nd;
    if (nd < 1 || nd > kMaxDiag || w < 1 || nd * w > rec * 8 || c->dia_ld < product_trips(c->nchunks, c->use_dia) * 128) return false;
    if (!dispatch_diac(w, rec, [](auto, auto) { return true; })) return false;
    return c->dia_doff[nd] >= 1 && (int64_t)c->dia_doff[nd] * 8 <= kDiaCodeLds;
}

// The reference arrays in the order the device keeps its vectors: the relabelled copies under the internal state order.
// False: none are resident for this generator.
inline bool ell_adj_args(const kfsp_ctx *ctx, EllAdjDev &e)
{
    const DevBuf<int32_t> &adj = ctx->perm_on ? ctx->d_ell_adj2 : ctx->d_ell_adj;
    const DevBuf<double> &off = ctx->perm_on ? ctx->d_ell_off2 : ctx->d_ell_off;
    const DevBuf<double> &diag = ctx->perm_on ? ctx->d_ell_diag2 : ctx->d_ell_diag;
    if (!adj.p || !off.p || !diag.p || !ell_adj_resident(ctx->n, ctx->ell_cols, ctx->ell_ld, ctx->ell_bw, adj.cap, off.cap, diag.cap))
        return false;
    e = EllAdjDev{adj.p, off.p, diag.p, ctx->n, ctx->ell_ld, ctx->ell_bw};
    return true;
}

// ---- what the decision depends on, and nothing else.  All of it is what the ranks of a partition share or what one rank
// alone decides (a partitioned call never gets past the flags of the first line and `box`).
struct BlockForm {
    bool no_matrix;                          // ldv == 0
    bool partitioned, collectives;           // a communicator, a loop-back rank or nranks > 1; ... that carries collectives (use_comm)
    int64_t block_partition;
    bool adjoint;
    bool box, box_fast;                      // a matrix-free box; box_plan found its single-factor form
    int64_t block_box, box_generic;
    bool generic_walkable, adj_builds;       // box_generic_image != 0; box_adj_build (asked only where the rule reads them)
    bool reach_ok;                           // box_block_reach_ok at this width
    bool banded, masked, have_sell, sell_coded;
    bool ell_resident;                       // ell_adj_args (asked for a backward SELL call only)
    bool coded_on;                           // dia_code_on
    int64_t block_dia_code, block_dia_code_adjoint;
    bool small;                              // small_path
    bool diac_walkable;                      // diac_image_walkable (asked where coded_on)
};

inline BlockForm block_form(const kfsp_ctx *c, int kp)
{
    BoxAdjDev b;
    EllAdjDev e;
    const bool adj = c->opt_adjoint != 0, box = c->box.on, coded = dia_code_on(c);
    return BlockForm{c->ldv == 0, c->use_comm || c->nranks > 1 || c->loop || c->comm, c->use_comm, c->opt_block_partition, adj,
                     box, c->box.fast, c->opt_block_box, c->opt_box_generic,
                     box && box_generic_image(c->box.dev) != 0, box && adj && box_adj_build(c->box.dev, b), !box || box_block_reach_ok(c, kp),
                     c->use_dia, c->dia_masked, c->have_sell, c->sell_coded, adj && !c->use_dia && ell_adj_args(c, e),
                     coded, c->opt_block_dia_code, c->opt_block_dia_code_adjoint, small_path(c), coded && diac_image_walkable(c)};
}

// ---- the nine kernel families, and where a refusal is raised: by every block call before anything else (block_supported),
// where a call knows its width (box_reach_check: kfsp_set_block, kfsp_spmm), or by the product alone
enum BlockKernel { kBlockNone = 0, kBlockSpmm, kBlockDiac, kBlockT, kBlockEllT, kBlockDiacT, kBlockBox, kBlockBoxT, kBlockBoxg, kBlockBoxgT,
                   kBlockKernels };
enum BlockRefusal { kRefuseNot = 0, kRefuseContext, kRefuseWidth, kRefuseProduct };

struct BlockPlan {
    BlockKernel kernel;      // kBlockNone: refused with
    int code;                // ... this status
    const char *why;         // ... and this text
    BlockRefusal where;
    int fmt;                 // kBlockSpmm: the stored form k_spmm is instantiated for (0 SELL, 5 with coded columns, 1 banded, 2 with group masks)
    int staged;              // a family that stages an image into dynamic LDS: its StagedFamily (the occupancy cache); else -1
    bool lds_shared;         // ... whose reductions reuse the image's LDS: the launch asks for never less than 4 kp doubles
};

constexpr const char *kBlockPartMsg = "several vectors at once: not with a row partition (communicator or group context) unless option block_partition = 1";
constexpr const char *kBlockReachMsg = "several vectors at once: the entries of this matrix-free box reach further than 2^32 bytes at this block width (fewer columns, or option box_store = 1)";
constexpr const char *kBlockAdjFormMsg = "several vectors at once, option adjoint: the generator is resident in no form the transposed product reads";

// Every refusal is made from what all ranks of a partition share (options, the kind of generator), before the first collective
// of any block call: a rank that returned alone would leave its peers waiting in one.
inline BlockPlan block_plan(const BlockForm &f)
{
    auto no = [](int code, const char *why, BlockRefusal where = kRefuseContext) { return BlockPlan{kBlockNone, code, why, where, 0, -1, false}; };
    auto run = [&](BlockKernel k, int staged = -1, bool lds_shared = false) {
        return BlockPlan{k, 0, nullptr, kRefuseNot, f.banded ? (f.masked ? 2 : 1) : (f.sell_coded ? 5 : 0), staged, lds_shared};
    };
    if (f.partitioned) {
        if (!f.block_partition) return no(-12, kBlockPartMsg);
        if (!f.collectives) return no(-12, "several vectors at once: this rank's communicator carries no collectives");
        if (f.no_matrix) return no(-1, "no matrix set");
        if (f.adjoint)
            return no(-12, "several vectors at once, option adjoint: not under a row partition (the transposed banded product reads the neighbour's generator rows, not only its rows of X)");
        if (f.box)
            return no(-12, "several vectors at once: not for a matrix-free generator under a row partition (option box_store = 1 stores it)");
    }
    if (f.no_matrix) return no(-1, "no matrix set");
    if (f.box) {
        if (!f.block_box)
            return no(-12, "several vectors at once: not for a matrix-free generator (option box_store = 1 stores it, option block_box = 1 takes it matrix-free)");
        // option block_box = 2: the generic kernels answer for a box without the single-factor form and for any box under box_generic = 1
        if (f.block_box == 2 && (!f.box_fast || f.box_generic != 0)) {
            if (!f.generic_walkable)
                return no(-12, "several vectors at once: the descriptor of this matrix-free box is not one the generic block kernels can walk (option box_store = 1 stores it)");
            return f.adjoint ? run(kBlockBoxgT, kStagedBoxgT, true) : run(kBlockBoxg, kStagedBoxg, true);
        }
        if (f.box_generic) return no(-12, "several vectors at once: not for the interpreted matrix-free product (option box_generic = 1)");
        if (!f.box_fast)
            return no(-12, "several vectors at once: this matrix-free box has no single-factor form (option box_store = 1 stores it)");
        if (!f.reach_ok) return no(-12, kBlockReachMsg, kRefuseWidth);
        if (!f.adjoint) return run(kBlockBox, kStagedBox, true);
        return f.adj_builds ? run(kBlockBoxT, kStagedBoxT, true) : no(-12, kBlockAdjFormMsg, kRefuseProduct);
    }
    if (!f.banded && !f.have_sell) return no(-12, "several vectors at once: no stored generator");
    if (f.adjoint && !f.banded)
        return f.ell_resident ? run(kBlockEllT)
                              : no(-12, "several vectors at once, option adjoint: the transposed product of a SELL generator reads the reference arrays ADJ / OFFDIAG / DIAG, and none are resident for this one (kfsp_set_matrix_ell uploads them; option box_store = 1 stores a box as diagonals)");
    // the coded banded kernels keep their reduction scratch apart (static LDS) and stage the dictionaries alone
    if (f.adjoint)
        return block_dia_code_t_path(f.coded_on, f.block_dia_code, f.block_dia_code_adjoint, f.adjoint) && f.diac_walkable
                   ? run(kBlockDiacT, kStagedDiacT) : run(kBlockT);
    return block_dia_code_path(f.coded_on, f.block_dia_code, f.adjoint, f.small) && f.diac_walkable ? run(kBlockDiac, kStagedDiac) : run(kBlockSpmm);
}

// How a product under a row partition sees its source (kfsp_block_info, slot kInfoExchange): 0 nothing to exchange (one rank, or
// x is the whole block every rank holds), 2 an all-gather, 1 the neighbours' strips before the product, 5 the strips beside
// the interior trips (overlapped_product: the product splits and a communication stream exists).
inline int block_exchange_mode(bool comm, bool x_global, bool halo, bool split, bool has_comm_stream)
{
    if (!comm || x_global) return 0;
    if (!halo) return 2;
    return split && has_comm_stream ? 5 : 1;
}

}  // namespace kfsp
