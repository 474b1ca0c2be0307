// The row partition's plumbing of libkfsp_hip: the collectives of the data path over RCCL or the loop-back transport,
// the halo exchange of banded (and bounded-reach SELL) generators, and the entry points of include/kfsp.h that attach a
// context to a communicator.
#include "kfsp_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace kfsp {

namespace {

int nccl_fail(kfsp_ctx *c, ncclResult_t r, const char *where)
{
    if (c) c->err = std::string(where) + ": " + ncclGetErrorString(r);
    return 2000 + (int)r;
}

#define NCCL_TRY(expr)                                           \
    do {                                                         \
        ncclResult_t r_ = (expr);                                \
        if (r_ != ncclSuccess) return nccl_fail(ctx, r_, #expr); \
    } while (0)

// ---- the collectives of the data path, over RCCL or the loop-back transport ----
constexpr int kLoopVals = 32;                              // values one all-reduce may carry (the 16 FIND_DROPTOL sums; 2 x 16 column sums of the block path)
constexpr int kLoopScratch = 64 * kLoopVals + kLoopVals;   // doubles: up to 64 ranks x 32 scalars (+ result)

}  // namespace

// buf[0..count) <- sum (or max) over ranks, in place, on stream st
int comm_allreduce(kfsp_ctx *ctx, double *buf, int count, bool take_max, hipStream_t st)
{
    if (!ctx->loop) {
        std::lock_guard<std::mutex> lk(ctx->comm_mu);
        if (ctx->comm_aborted) return fail(ctx, 2999, "the communicator was aborted");
        NCCL_TRY(ncclAllReduce(buf, buf, (size_t)count, ncclDouble, take_max ? ncclMax : ncclSum, ctx->comm, st));
        return 0;
    }
    kfsp::LoopGroup *g = ctx->loop;
    if (count > kLoopVals || g->n > 64) return fail(ctx, -1, "loop-back all-reduce: too many values");
    HIP_TRY(hipStreamSynchronize(st));                  // this rank's contribution is in memory
    g->slot[(size_t)ctx->rank] = buf;
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");
    double *h = ctx->h_loop;
    for (int p = 0; p < g->n; ++p)
        HIP_TRY(hipMemcpyAsync(h + kLoopVals * p, g->slot[(size_t)p], (size_t)count * sizeof(double), hipMemcpyDefault, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");   // everyone has read
    double *r = h + kLoopVals * g->n;
    for (int i = 0; i < count; ++i) {
        double a = h[i];
        for (int p = 1; p < g->n; ++p) a = take_max ? std::max(a, h[kLoopVals * p + i]) : a + h[kLoopVals * p + i];   // rank order: same bits on every rank
        r[i] = a;
    }
    HIP_TRY(hipMemcpyAsync(buf, r, (size_t)count * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// recv[p*count .. (p+1)*count) <- send of rank p, on stream st
int comm_allgather(kfsp_ctx *ctx, const double *send, double *recv, size_t count, hipStream_t st)
{
    if (!ctx->loop) {
        std::lock_guard<std::mutex> lk(ctx->comm_mu);
        if (ctx->comm_aborted) return fail(ctx, 2999, "the communicator was aborted");
        NCCL_TRY(ncclAllGather(send, recv, count, ncclDouble, ctx->comm, st));
        return 0;
    }
    kfsp::LoopGroup *g = ctx->loop;
    HIP_TRY(hipStreamSynchronize(st));
    g->slot[(size_t)ctx->rank] = send;
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");
    for (int p = 0; p < g->n; ++p)
        HIP_TRY(hipMemcpyAsync(recv + (size_t)p * count, g->slot[(size_t)p], count * sizeof(double), hipMemcpyDefault, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");   // nobody reuses its send buffer before all have copied
    return 0;
}

// the same for raw bytes (flags)
int comm_allgather_bytes(kfsp_ctx *ctx, const void *send, void *recv, size_t bytes, hipStream_t st)
{
    if (!ctx->loop) {
        std::lock_guard<std::mutex> lk(ctx->comm_mu);
        if (ctx->comm_aborted) return fail(ctx, 2999, "the communicator was aborted");
        NCCL_TRY(ncclAllGather(send, recv, bytes, ncclUint8, ctx->comm, st));
        return 0;
    }
    kfsp::LoopGroup *g = ctx->loop;
    HIP_TRY(hipStreamSynchronize(st));
    g->slot[(size_t)ctx->rank] = send;
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");
    for (int p = 0; p < g->n; ++p)
        HIP_TRY(hipMemcpyAsync(static_cast<char *>(recv) + (size_t)p * bytes, g->slot[(size_t)p], bytes, hipMemcpyDefault, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");
    return 0;
}

// Called from ANOTHER thread than the one that drives ctx (the watchdog of a group context, kfsp_group.cpp) when a peer
// failed or a deadline expired: the rank may sit in hipStreamSynchronize behind a collective its peers never entered.
// ncclCommAbort makes the collective's kernel give up; the loop-back transport releases its barriers.  The rank's
// pending call then returns an error, later collectives return 2999.  comm_mu keeps the abort from running while
// the driving thread is in the middle of enqueuing on the same communicator.
void comm_abort(kfsp_ctx *ctx)
{
    if (ctx->loop) {
        ctx->loop->abort();
        return;
    }
    std::lock_guard<std::mutex> lk(ctx->comm_mu);
    if (ctx->comm && !ctx->comm_aborted) (void)ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
    ctx->comm_aborted = true;
}

// Banded generator: only the `halo` boundary rows of the two neighbours are ever
// read.  Every rank contributes [its first halo rows | its last halo rows]; one
// all-gather of these strips, then the two strips this rank needs are dropped
// into the margins of the source column itself.  All on stream st.  width: doubles
// per row (1: a vector; kp: a row-interleaved block column, whose caller sized d_strip).
int exchange_strips(kfsp_ctx *ctx, const double *src_local, hipStream_t st, int width)
{
    // (in doubles: a strip of halo rows of a block column is one run of halo * width doubles)
    const int64_t H = ctx->halo * width, L = ctx->L * width;
    double *col = const_cast<double *>(src_local);
    if (ctx->opt_halo_p2p != 0) {
        // Neighbours only, and straight between the columns: a rank's first H rows go into the margin
        // behind the previous rank's block, its last H rows into the margin in front of the next rank's.
        // No staging copies, no strips of ranks that are not neighbours (an all-gather moves
        // nranks * 2H doubles to every rank for the 2H it needs).
        const bool up = ctx->rank > 0, down = ctx->rank + 1 < ctx->nranks;
        if (!ctx->loop) {
            std::lock_guard<std::mutex> lk(ctx->comm_mu);
            if (ctx->comm_aborted) return fail(ctx, 2999, "the communicator was aborted");
            NCCL_TRY(ncclGroupStart());
            if (up) {
                NCCL_TRY(ncclSend(src_local, (size_t)H, ncclDouble, ctx->rank - 1, ctx->comm, st));
                NCCL_TRY(ncclRecv(col - H, (size_t)H, ncclDouble, ctx->rank - 1, ctx->comm, st));
            }
            if (down) {
                NCCL_TRY(ncclSend(src_local + (L - H), (size_t)H, ncclDouble, ctx->rank + 1, ctx->comm, st));
                NCCL_TRY(ncclRecv(col + L, (size_t)H, ncclDouble, ctx->rank + 1, ctx->comm, st));
            }
            NCCL_TRY(ncclGroupEnd());
            return 0;
        }
        kfsp::LoopGroup *g = ctx->loop;
        HIP_TRY(hipStreamSynchronize(st));
        g->slot[(size_t)ctx->rank] = src_local;
        if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");
        if (up)      // the previous rank's LAST rows sit just below row 0
            HIP_TRY(hipMemcpyAsync(col - H, static_cast<const double *>(g->slot[(size_t)ctx->rank - 1]) + (L - H),
                                   (size_t)H * sizeof(double), hipMemcpyDefault, st));
        if (down)    // the next rank's FIRST rows follow row L-1
            HIP_TRY(hipMemcpyAsync(col + L, static_cast<const double *>(g->slot[(size_t)ctx->rank + 1]),
                                   (size_t)H * sizeof(double), hipMemcpyDefault, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!g->barrier()) return fail(ctx, 2999, "loop-back barrier timed out");   // nobody moves on before all have copied
        return 0;
    }
    double *send = ctx->d_strip.p, *recv = ctx->d_strip.p + 2 * H;
    HIP_TRY(hipMemcpyAsync(send, src_local, (size_t)H * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(send + H, src_local + (L - H), (size_t)H * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (int rc = comm_allgather(ctx, send, recv, (size_t)(2 * H), st)) return rc;
    if (ctx->rank > 0)                 // the previous rank's LAST rows sit just below row 0
        HIP_TRY(hipMemcpyAsync(col - H, recv + (size_t)(ctx->rank - 1) * 2 * H + H, (size_t)H * sizeof(double),
                               hipMemcpyDeviceToDevice, st));
    if (ctx->rank + 1 < ctx->nranks)   // the next rank's FIRST rows follow row L-1
        HIP_TRY(hipMemcpyAsync(col + L, recv + (size_t)(ctx->rank + 1) * 2 * H, (size_t)H * sizeof(double),
                               hipMemcpyDeviceToDevice, st));
    return 0;
}

// The source column must be visible in full on every rank before a product.
int gather_source(kfsp_ctx *ctx, const double *src_local, const double **xg)
{
    if (!ctx->use_comm) {
        *xg = src_local - ctx->row0;       // row0 == 0 here
        return 0;
    }
    if (ctx->use_halo) {
        if (int rc = exchange_strips(ctx, src_local, ctx->stream)) return rc;
        *xg = src_local - ctx->row0;       // global index g lives at src_local[g - row0]
        return 0;
    }
    if (int rc = comm_allgather(ctx, src_local, ctx->d_xg.p, (size_t)ctx->L, ctx->stream)) return rc;
    *xg = ctx->d_xg.p;
    return 0;
}

// After a generator was set: agree across ranks on the exchange mode.  Halo
// exchange needs every rank to hold a banded block whose reach max|delta| does
// not exceed one block length (only the two neighbours are involved then).
int setup_exchange(kfsp_ctx *ctx)
{
    ctx->use_halo = false;
    ctx->halo = 0;
    if (!ctx->use_comm) return 0;
    int64_t reach = 0;
    for (int d = 0; d < ctx->nd; ++d) reach = std::max<int64_t>(reach, std::llabs((long long)ctx->delta[d]));
    // a SELL generator with a bounded reach max |col - row| (known from its build; small under the internal
    // lexicographic state order) reads only boundary rows of its neighbours too
    const bool sell_ok = !ctx->use_dia && ctx->have_sell && ctx->sell_reach >= 0 && ctx->opt_halo_sell != 0;
    if (sell_ok) reach = ctx->sell_reach;
    // ranks without rows take part with neutral values
    const bool ok_local = ctx->opt_halo != 0 && (ctx->nloc == 0 || ctx->use_dia || sell_ok);
    double h[2] = {ok_local ? 0.0 : 1.0, (double)reach};          // max over ranks of (not ok, reach)
    double *st = ctx->d_stage.p;
    HIP_TRY(hipMemcpyAsync(st, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = comm_allreduce(ctx, st, 2, true, ctx->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(h, st, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t H = round_up(std::max<int64_t>((int64_t)h[1], 1), 8);
    if (h[0] != 0.0 || H > ctx->L) return 0;                      // someone is not banded, or reach > one block
    ctx->halo = H;
    if (H + 2 * kChunk > ctx->margin) {
        // re-lay the basis with room for the strips (its contents are rebuilt by
        // the next begin_step anyway)
        // + 128: the banded kernel works on 128-row groups, whose padded rows read up
        // to one group beyond the block end
        ctx->margin = halo_margin(H);
        ctx->relayout = true;
        if (int rc = resize(ctx, ctx->n)) return rc;
    }
    HIP_TRY(ctx->d_strip.reserve((size_t)(2 * H) * (size_t)(ctx->nranks + 1), true));
    ctx->use_halo = true;
    return 0;
}

}  // namespace kfsp

using namespace kfsp;

extern "C" {

int kfsp_comm_unique_id(void *id_bytes)
{
    if (!id_bytes) return -1;
    static_assert(sizeof(ncclUniqueId) == KFSP_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return 2000 + (int)r;
    std::memcpy(id_bytes, &id, sizeof(id));
    return 0;
}

int kfsp_comm_init(kfsp_ctx *ctx, int nranks, int rank, const void *id_bytes)
{
    if (!ctx) return -1;
    if (nranks < 1) return fail(ctx, -2, "nranks < 1");
    if (rank < 0 || rank >= nranks) return fail(ctx, -3, "rank out of range");
    if (nranks > 1 && !id_bytes) return fail(ctx, -4, "null unique id");
    if (ctx->group) return fail(ctx, -9, "a group context makes its own communicator");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->comm) {
        // (abort, not destroy: the usual reason to come here twice is a communicator that returned an
        // error on some rank, and destroying one of those can wait for ever)
        (void)ncclCommAbort(ctx->comm);
        ctx->comm = nullptr;
    }
    ctx->loop = nullptr;
    ctx->comm_aborted = false;
    ctx->nranks = nranks;
    ctx->rank = rank;
    // a unique id with nranks == 1 still creates a (one-rank) communicator, so the
    // collective code path can be exercised on a single GPU
    ctx->use_comm = false;
    if (id_bytes) {
        ncclUniqueId id;
        std::memcpy(&id, id_bytes, sizeof(id));
        NCCL_TRY(ncclCommInitRank(&ctx->comm, nranks, id, rank));
        ctx->use_comm = true;
        if (!ctx->comm_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_src, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming));
        }
    }
    ctx->relayout = true;   // new margins / block length: re-lay the basis on the next matrix
    ctx->use_halo = false;
    return 0;
}

int kfsp_loopback_create(int nranks, void **group)
{
    if (nranks < 1 || nranks > 64) return -1;
    if (!group) return -2;
    kfsp::LoopGroup *g = new (std::nothrow) kfsp::LoopGroup;
    if (!g) return 4001;
    g->n = nranks;
    g->slot.assign((size_t)nranks, nullptr);
    *group = g;
    return 0;
}

int kfsp_loopback_destroy(void *group)
{
    delete static_cast<kfsp::LoopGroup *>(group);
    return 0;
}

int kfsp_comm_init_loopback(kfsp_ctx *ctx, void *group, int rank)
{
    if (!ctx) return -1;
    if (!group) return fail(ctx, -2, "null group");
    kfsp::LoopGroup *g = static_cast<kfsp::LoopGroup *>(group);
    if (rank < 0 || rank >= g->n) return fail(ctx, -3, "rank out of range");
    if (ctx->group) return fail(ctx, -9, "a group context makes its own communicator");
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->comm) {
        (void)ncclCommAbort(ctx->comm);   // as kfsp_comm_init: destroying a failed communicator can wait for ever
        ctx->comm = nullptr;
    }
    ctx->loop = g;
    ctx->comm_aborted = false;
    ctx->nranks = g->n;
    ctx->rank = rank;
    ctx->use_comm = true;
    if (!ctx->h_loop)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_loop), (size_t)(kLoopScratch + 8) * sizeof(double), hipHostMallocDefault));
    if (!ctx->comm_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_src, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming));
    }
    ctx->relayout = true;   // new margins / block length: re-lay the basis on the next matrix
    ctx->use_halo = false;
    return 0;
}

}  // extern "C"
