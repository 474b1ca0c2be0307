// Host side of libkfsp_hip: replacing the resident generator.  Every entry point that does - kfsp_set_matrix_ell, _csr, _box,
// kfsp_drop_rebuild and kfsp_expand_resident (kfsp_api.cpp) through rebuild_resident - runs begin_generator (THE reset of
// GeneratorState, sizes, the predecessor's bookkeeping), its build (kfsp_build.hip), finish_generator (exchange, vector, timer).
#include "kfsp_host.h"

#include <algorithm>
#include <vector>

using namespace kfsp;

namespace {

// Upload gather rows given as per-row counts + a fill callback.
struct HostSell {
    std::vector<int64_t> off;
    std::vector<int32_t> col;
    std::vector<double> val, diag;
    int64_t nchunks = 0, nnz = 0;
};

void sell_layout(const std::vector<int32_t> &cnt, int64_t nloc, int64_t row0, HostSell &S)
{
    S.nchunks = (nloc + kChunk - 1) / kChunk;
    S.off.assign((size_t)S.nchunks + 1, 0);
    for (int64_t c = 0; c < S.nchunks; ++c) {
        int w = 0;
        const int64_t r1 = std::min<int64_t>(nloc, (c + 1) * kChunk);
        for (int64_t r = c * kChunk; r < r1; ++r) w = std::max(w, (int)cnt[(size_t)r]);
        S.off[(size_t)c + 1] = S.off[(size_t)c] + (int64_t)w * kChunk;
    }
    const size_t slots = (size_t)S.off[(size_t)S.nchunks];
    S.col.resize(slots);
    S.val.assign(slots, 0.0);
    // padded slots gather the row's own x (always a valid address)
    for (int64_t c = 0; c < S.nchunks; ++c) {
        const int64_t o = S.off[(size_t)c], w = (S.off[(size_t)c + 1] - o) / kChunk;
        for (int64_t k = 0; k < w; ++k)
            for (int l = 0; l < kChunk; ++l) {
                const int64_t r = std::min<int64_t>(c * kChunk + l, nloc > 0 ? nloc - 1 : 0);
                S.col[(size_t)kfsp::sell_pos(o, (int)w, (int)k, l)] = (int32_t)(row0 + r);
            }
    }
    S.diag.assign((size_t)S.nchunks * kChunk, 0.0);
}

int upload_sell(kfsp_ctx *ctx, const HostSell &S)
{
    ctx->nchunks = S.nchunks;
    ctx->slots = S.off[(size_t)S.nchunks];
    ctx->nnz = S.nnz;
    HIP_TRY(ctx->d_off.reserve(S.off.size(), false));
    HIP_TRY(ctx->d_col.reserve(std::max<size_t>(S.col.size(), 64), false));
    HIP_TRY(ctx->d_val.reserve(std::max<size_t>(S.val.size(), 64), false));
    HIP_TRY(ctx->d_diag.reserve(S.diag.size() + 2 * kChunk, false));
    HIP_TRY(hipMemsetAsync(ctx->d_diag.p, 0, (S.diag.size() + 2 * kChunk) * sizeof(double), ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_off.p, S.off.data(), S.off.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (!S.col.empty()) {
        HIP_TRY(hipMemcpyAsync(ctx->d_col.p, S.col.data(), S.col.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemcpyAsync(ctx->d_val.p, S.val.data(), S.val.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (!S.diag.empty())
        HIP_TRY(hipMemcpyAsync(ctx->d_diag.p, S.diag.data(), S.diag.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->have_sell = true;
    return kfsp::build_sell_code(ctx);
}

// Banded form: accepted when the local rows use at most kMaxDiag distinct column offsets and the diagonals are reasonably full.
int maybe_upload_dia(kfsp_ctx *ctx, const HostSell &S, const std::vector<int32_t> &cnt)
{
    const int64_t nloc = ctx->nloc, row0 = ctx->row0;
    int nd = 0;
    int64_t delta[kMaxDiag];
    int64_t nnz_off = 0;
    for (int64_t r = 0; r < nloc && nd <= kMaxDiag; ++r) {
        const int64_t c = r / kChunk, l = r % kChunk, o = S.off[(size_t)c];
        const int w = (int)((S.off[(size_t)c + 1] - o) / kChunk);
        for (int k = 0; k < cnt[(size_t)r]; ++k) {
            const int64_t dl = (int64_t)S.col[(size_t)kfsp::sell_pos(o, w, k, (int)l)] - (row0 + r);
            int d = 0;
            while (d < nd && delta[d] != dl) ++d;
            if (d == nd) {
                if (nd == kMaxDiag) {                           // one offset too many: no need to count the rest
                    nd = kMaxDiag + 1;
                    break;
                }
                delta[nd++] = dl;
            }
            ++nnz_off;
        }
    }
    if (!banded_pays(nd, nloc, nnz_off, ctx->opt_format)) return 0;
    std::sort(delta, delta + nd);
    const int64_t ld = round_up(ctx->nchunks * kChunk, 2 * kChunk);   // the banded kernel works on 128-row groups
    std::vector<double> val((size_t)nd * (size_t)ld, 0.0);
    for (int64_t r = 0; r < nloc; ++r) {
        const int64_t c = r / kChunk, l = r % kChunk, o = S.off[(size_t)c];
        const int w = (int)((S.off[(size_t)c + 1] - o) / kChunk);
        for (int k = 0; k < cnt[(size_t)r]; ++k) {
            const size_t pos = (size_t)kfsp::sell_pos(o, w, k, (int)l);
            const int64_t dl = (int64_t)S.col[pos] - (row0 + r);
            const int d = (int)(std::lower_bound(delta, delta + nd, dl) - delta);
            val[(size_t)d * (size_t)ld + (size_t)r] += S.val[pos];
        }
    }
    HIP_TRY(ctx->d_dia.reserve(val.size(), false));
    HIP_TRY(hipMemcpy(ctx->d_dia.p, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->nd = nd;
    ctx->dia_ld = ld;
    for (int d = 0; d < nd; ++d) ctx->delta[d] = (int32_t)delta[d];
    ctx->use_dia = true;
    if (int rc = kfsp::build_dia_mask(ctx)) return rc;
    return kfsp::build_dia_code(ctx);
}

// A vector compacted on the device (kfsp_drop_compact) becomes the resident w of the generator
// that was just set: caller's order -> the order the device keeps this generator in.  With a communicator the
// pending vector is the FULL compacted vector (every rank holds it) and each rank takes its new block.
int adopt_pending_vector(kfsp_ctx *ctx)
{
    if (!ctx->w_pending) return 0;
    ctx->w_pending = false;
    // (a compaction that dropped EVERY state leaves no vector to carry over - and no generator of 0 states could ever
    // claim it: whatever generator comes next starts from w = 0)
    if (ctx->w_pending_n != ctx->n && ctx->w_pending_n != 0)
        return fail(ctx, -2, "generator size does not match the vector compacted by kfsp_drop_compact");
    HIP_TRY(hipMemsetAsync(ctx->d_w.p, 0, (size_t)ctx->ldv * sizeof(double), ctx->stream));
    if (ctx->w_pending_n == 0) {
        ctx->w_pending_full = false;
        return 0;
    }
    if (ctx->use_comm || ctx->w_pending_full) {
        ctx->w_pending_full = false;
        if (int rc = scatter_from_full(ctx, ctx->d_wfull.p, ctx->d_w.p)) return rc;
    } else if (ctx->perm_on)
        kfsp::launch_gather_index(ctx->n, ctx->d_perm.p, ctx->d_tmp.p, ctx->d_w.p, ctx->stream);
    else
        HIP_TRY(hipMemcpyAsync(ctx->d_w.p, ctx->d_tmp.p, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    // (one context works on one stream: whatever reads the vector next is ordered behind this)
    if (!ctx->opt_build_speculate || ctx->use_comm) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// Where the rows come from decides what a call REFUSED by resize leaves: the reference-array paths keep the product count
// (and kfsp_set_matrix_ell its pending coordinates) for the upload that follows; the caller-layout paths (CSR, box) spend both first.
enum class RowsFrom { kReferenceArrays, kCallerLayout };
// A new generator of n states: THE reset of the old one's form, the sizes, the pending coordinates and product count spent
int begin_generator(kfsp_ctx *ctx, int64_t n, bool perm_on, RowsFrom from)
{
    auto spend = [&] {
        ctx->perm_on = perm_on;
        ctx->perm_pending_n = 0;
        ctx->prod_last = ctx->prod_count;
        ctx->prod_count = 0;
    };
    reset_generator(ctx);
    if (from == RowsFrom::kCallerLayout) {
        spend();
        ctx->ell_cols = 0;
    }
    if (int rc = resize(ctx, n)) return rc;
    if (from == RowsFrom::kReferenceArrays) spend();
    return 0;
}

// ... and is ready, or its build failed with rc (the call counts its time either way): exchange mode, pending vector
int finish_generator(kfsp_ctx *ctx, int rc, std::chrono::steady_clock::time_point t0)
{
    if (!rc) rc = setup_exchange(ctx);
    if (!rc) rc = adopt_pending_vector(ctx);
    ctx->t_ms[KFSP_T_UPLOAD] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace

int kfsp::rebuild_resident(kfsp_ctx *ctx, int32_t n, int32_t bw, int32_t ld, int32_t ns, int32_t cld, int32_t n_prev, bool want_order,
                           bool coords, std::chrono::steady_clock::time_point t0)
{
    const bool spec = ctx->opt_build_speculate != 0;    // (under a row partition too: order and build are rank-local, every rank repeats the same checks)
    // The state order, on the coordinates that stayed here.  The callers differ in what the resident order still gives, and
    // only while speculating: after a drop (n_prev > n) it is compacted with the flags and scan that kfsp_drop_compact and
    // compact_resident_ell left; after an expansion only the appended states' keys are made and merged in.
    ctx->perm_pending_n = 0;
    const bool dropped = n_prev > n;
    bool ordered = false;
    auto order = [&](bool speculate) -> int {
        ordered = false;
        ctx->coords_n = 0;
        if (coords && want_order) {
            int rc = 0;
            if (speculate && dropped && ns == ctx->kc_ns)
                ordered = state_order_after_drop(ctx, n_prev, n, ctx->d_dropflag.p + ctx->d_dropflag.cap / 2, ctx->d_sortidx.p + n_prev, &rc);
            if (!ordered) rc = state_order_from_resident(ctx, n, ns, cld, &ordered, speculate, dropped ? 0 : n_prev);
            if (rc) return rc;
        }
        if (coords) {                                      // (resident whether an order came of them or not)
            ctx->coords_n = n;
            ctx->coords_ld = cld;
            ctx->coords_ns = ns;
        }
        return 0;
    };
    if (int rc = order(spec)) return rc;
    if (int rc = begin_generator(ctx, n, ordered, RowsFrom::kReferenceArrays)) return rc;
    int rc = build_from_resident_ell(ctx, n, bw, ld, spec);
    if (rc == kRedoBuild) {                                // (a speculation did not hold: order and generator again, waiting for every number)
        ++ctx->spec_redone;
        if (int rc2 = order(false)) return rc2;
        ctx->perm_on = ordered;
        rc = build_from_resident_ell(ctx, n, bw, ld);
    }
    return finish_generator(ctx, rc, t0);
}

extern "C" {

static int set_matrix_ell_impl(kfsp_ctx *ctx, int32_t n, int32_t bw, int32_t ld, const int32_t *adj,
                               const double *offdiag, const double *diag, int64_t keep)
{
    return no_throw(ctx, [&]() -> int {
        if (!ctx) return -1;
        if (n < 1) return fail(ctx, -2, "n < 1");
        if (bw < 1) return fail(ctx, -3, "bw < 1");
        if (ld < bw) return fail(ctx, -4, "ld < bw");
        if (!adj) return fail(ctx, -5, "null adj");
        if (!offdiag) return fail(ctx, -6, "null offdiag");
        if (!diag) return fail(ctx, -7, "null diag");
        if (ctx->group) return kfsp::group_update_matrix_ell(ctx, n, bw, ld, adj, offdiag, diag, (int32_t)keep);
        HIP_TRY(hipSetDevice(ctx->device));
        auto t0 = std::chrono::steady_clock::now();
        // coordinates handed over for exactly this generator switch the internal order on
        if (int rc = begin_generator(ctx, n, ctx->perm_pending_n == n && !ctx->opt_host_build, RowsFrom::kReferenceArrays)) return rc;
        const int64_t row0 = ctx->row0, nloc = ctx->nloc;

        if (!ctx->opt_host_build) {
            // the arrays go to HBM verbatim and are transposed there (kfsp_build.hip)
            int rc = build_from_ell_device(ctx, n, bw, ld, adj, offdiag, diag, keep);
            return finish_generator(ctx, rc, t0);
        }

        // host transpose (kept for A/B checks of the device build): the arrays do not become resident
        ctx->ell_cols = 0;
        // in-degree of every local row
        std::vector<int32_t> cnt((size_t)std::max<int64_t>(nloc, 1), 0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t *a = adj + (size_t)i * ld;
            for (int j = 0; j < bw; ++j) {
                const int64_t k = a[j];
                if (k > n) return fail(ctx, -5, "adj entry exceeds n");
                if (k >= 1) {
                    const int64_t r = k - 1 - row0;
                    if (r >= 0 && r < nloc) ++cnt[(size_t)r];
                }
            }
        }
        HostSell S;
        sell_layout(cnt, nloc, row0, S);
        std::vector<int32_t> fill((size_t)std::max<int64_t>(nloc, 1), 0);
        int64_t nnz = nloc;
        // sources in increasing order: each row's entries end up sorted by column,
        // the order in which FMATVEC (:598-604) accumulates them
        for (int64_t i = 0; i < n; ++i) {
            const int32_t *a = adj + (size_t)i * ld;
            const double *o = offdiag + (size_t)i * ld;
            for (int j = 0; j < bw; ++j) {
                const int64_t k = a[j];
                if (k < 1) continue;
                const int64_t r = k - 1 - row0;
                if (r < 0 || r >= nloc) continue;
                const int64_t c = r / kChunk, l = r % kChunk;
                const int64_t pos = kfsp::sell_pos(S.off[(size_t)c], (int)((S.off[(size_t)c + 1] - S.off[(size_t)c]) / kChunk), fill[(size_t)r]++, (int)l);
                S.col[(size_t)pos] = (int32_t)i;
                S.val[(size_t)pos] = o[j];
                ++nnz;
            }
        }
        for (int64_t r = 0; r < nloc; ++r) S.diag[(size_t)r] = diag[(size_t)(row0 + r)];
        S.nnz = nnz;
        int rc = upload_sell(ctx, S);
        if (!rc) rc = maybe_upload_dia(ctx, S, cnt);
        return finish_generator(ctx, rc, t0);
    });
}

int kfsp_set_matrix_ell(kfsp_ctx *ctx, int32_t n, int32_t bw, int32_t ld, const int32_t *adj,
                        const double *offdiag, const double *diag)
{
    return set_matrix_ell_impl(ctx, n, bw, ld, adj, offdiag, diag, 0);
}

int kfsp_update_matrix_ell(kfsp_ctx *ctx, int32_t n, int32_t bw, int32_t ld, const int32_t *adj,
                           const double *offdiag, const double *diag, int32_t n_unchanged)
{
    if (n_unchanged < 0 || n_unchanged > n) return ctx ? fail(ctx, -8, "0 <= n_unchanged <= n") : -1;
    return set_matrix_ell_impl(ctx, n, bw, ld, adj, offdiag, diag, n_unchanged);
}

int kfsp_set_matrix_csr(kfsp_ctx *ctx, int64_t n, int64_t row0, int64_t nrows, const int64_t *rowptr,
                        const int32_t *col, const double *val)
{
    return no_throw(ctx, [&]() -> int {
        if (!ctx) return -1;
        if (n < 1 || n > 2147483647LL - 512) return fail(ctx, -2, "n out of range");
        if (ctx->group) return kfsp::group_set_matrix_csr(ctx, n, row0, nrows, rowptr, col, val);
        HIP_TRY(hipSetDevice(ctx->device));
        if (int rc = begin_generator(ctx, n, false, RowsFrom::kCallerLayout)) return rc;
        if (row0 != std::min(ctx->row0, n)) return fail(ctx, -3, "row0 is not this rank's block start (kfsp_row_block)");
        if (nrows != ctx->nloc) return fail(ctx, -4, "nrows is not this rank's block size (kfsp_row_block)");
        if (!rowptr) return fail(ctx, -5, "null rowptr");
        if (nrows > 0 && (!col || !val)) return fail(ctx, -6, "null col/val");
        if (rowptr[0] != 0) return fail(ctx, -5, "rowptr[0] != 0");
        auto t0 = std::chrono::steady_clock::now();
        const int64_t nloc = ctx->nloc;
        std::vector<int32_t> cnt((size_t)std::max<int64_t>(nloc, 1), 0);
        for (int64_t r = 0; r < nloc; ++r) {
            if (rowptr[r + 1] < rowptr[r]) return fail(ctx, -5, "rowptr not monotone");
            int c = 0;
            for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
                if (col[p] < 0 || col[p] >= n) return fail(ctx, -6, "column index out of range");
                if (col[p] != row0 + r) ++c;
            }
            cnt[(size_t)r] = c;
        }
        HostSell S;
        sell_layout(cnt, nloc, ctx->row0, S);
        for (int64_t r = 0; r < nloc; ++r) {
            const int64_t c = r / kChunk, l = r % kChunk;
            int k = 0;
            double d = 0.0;
            for (int64_t p = rowptr[r]; p < rowptr[r + 1]; ++p) {
                if (col[p] == row0 + r) {
                    d += val[p];
                } else {
                    const int64_t pos = kfsp::sell_pos(S.off[(size_t)c], (int)((S.off[(size_t)c + 1] - S.off[(size_t)c]) / kChunk), k++, (int)l);
                    S.col[(size_t)pos] = col[p];
                    S.val[(size_t)pos] = val[p];
                }
            }
            S.diag[(size_t)r] = -d;   // kept positive like DIAG (StateSpace.f90:16)
        }
        S.nnz = rowptr[nloc];
        int rc = upload_sell(ctx, S);
        if (!rc) rc = maybe_upload_dia(ctx, S, cnt);
        return finish_generator(ctx, rc, t0);
    });
}

int kfsp_set_matrix_box(kfsp_ctx *ctx, int32_t ns, const int32_t *dims, int32_t nr, const int32_t *stoich,
                        const int32_t *ndep, const int32_t *dep_species, const double *tables)
{
    return no_throw(ctx, [&]() -> int {
        if (!ctx) return -1;
        const char *what = "";
        if (int rc = kfsp::box_plan_args(ns, dims, nr, stoich, ndep, dep_species, tables, &what)) return fail(ctx, rc, what);
        if (ctx->group) return kfsp::group_set_matrix_box(ctx, ns, dims, nr, stoich, ndep, dep_species, tables);
        // everything that can refuse the model, before the context changes: a refused call leaves it and its generator alone
        kfsp::BoxPlan P;
        const kfsp::BoxPlanOpts opt{ctx->opt_box_pencil, ctx->opt_box_slab_waves, ctx->opt_box_tile, ctx->opt_box_reach,
                                    ctx->nranks == 1 && !ctx->use_comm};
        if (int rc = kfsp::box_plan(ns, dims, nr, stoich, ndep, dep_species, tables, opt, P, &what)) return fail(ctx, rc, what);
        HIP_TRY(hipSetDevice(ctx->device));
        auto t0 = std::chrono::steady_clock::now();
        if (int rc = begin_generator(ctx, P.n, false, RowsFrom::kCallerLayout)) return rc;
        HIP_TRY(ctx->d_box.reserve(P.image.size() + 8, false));
        HIP_TRY(hipMemcpy(ctx->d_box.p, P.image.data(), P.image.size() * sizeof(double), hipMemcpyHostToDevice));
        if (!P.order.empty()) {
            HIP_TRY(ctx->d_pencil_order.reserve(P.order.size(), false));
            HIP_TRY(hipMemcpy(ctx->d_pencil_order.p, P.order.data(), P.order.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        ctx->box = P.g;
        // the same bookkeeping as a banded generator with one diagonal per reaction
        ctx->nchunks = (ctx->nloc + kChunk - 1) / kChunk;
        ctx->nnz = ctx->nranks == 1 ? P.nnz : 0;           // (per-rank counts are not tracked for boxes)
        ctx->use_dia = true;
        ctx->nd = nr;
        for (int p = 0; p < nr; ++p) ctx->delta[p] = P.g.dev.delta[p];
        ctx->dia_ld = round_up(ctx->nchunks * kChunk, 2 * kChunk);
        HIP_TRY(ctx->d_diag.reserve((size_t)ctx->dia_ld + 2 * kChunk, true));
        int rc = 0;
        if (ctx->opt_box_store) {
            // the same generator as STORED diagonals, written by the device from the tables: from here on an
            // ordinary banded generator (no host arrays of the size of the FSP ever exist)
            rc = kfsp::box_materialize(ctx);
            if (!rc) ctx->box = {};
            if (!rc) rc = kfsp::build_dia_mask(ctx);
            if (!rc) rc = kfsp::build_dia_code(ctx);
        }
        return finish_generator(ctx, rc, t0);
    });
}

int kfsp_drop_rebuild(kfsp_ctx *ctx)
{
    return no_throw(ctx, [&]() -> int {
        if (!ctx) return -1;
        if (ctx->group) return kfsp::group_drop_rebuild(ctx);
        if (!ctx->w_pending) return fail(ctx, -1, "no compaction pending (kfsp_drop_compact)");
        const int64_t n_old = ctx->drop_n, n_new = ctx->w_pending_n;
        if (ctx->drop_ell_cols != n_old || ctx->opt_host_build || n_new < 1)
            return fail(ctx, -9, "the reference arrays of this FSP are not resident on the device: upload the compacted generator");
        HIP_TRY(hipSetDevice(ctx->device));
        auto t0 = std::chrono::steady_clock::now();
        const int bw = ctx->drop_bw, ld = ctx->ell_ld;
        const uint8_t *keep = ctx->d_dropflag.p + ctx->d_dropflag.cap / 2;      // (made by kfsp_drop_compact, caller's order)
        const bool coords = ctx->coords_n == n_old;
        const int cld = ctx->coords_ld, cns = ctx->coords_ns;
        const bool want_order = want_state_order(ctx, n_new);
        if (want_order && !coords)     // the upload path would order this FSP, and the coordinates are not here: let it
            return fail(ctx, -9, "the state coordinates of this FSP are not resident on the device: upload the compacted generator");
        ctx->drop_ell_cols = 0;
        if (int rc = kfsp::compact_resident_ell(ctx, n_old, bw, ld, keep, n_new, coords, cld)) return rc;
        ctx->ell_cols = n_new;
        // order, generator and vector of the compacted FSP: the kept states keep their relative order
        return kfsp::rebuild_resident(ctx, (int32_t)n_new, bw, ld, cns, cld, (int32_t)n_old, want_order, coords, t0);
    });
}

}  // extern "C"
