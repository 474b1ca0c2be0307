// Stand-alone check of the host rules of generator replacement: banded_pays and want_state_order (kfsp_host.h) against
// LITERAL restatements of the copies they replaced - the banded_form lambda of build_from_resident_ell and the tests of
// maybe_upload_dia; the expression that stood in kfsp_set_state_coords, kfsp_drop_rebuild and kfsp_expand_resident - and
// reset_generator (kfsp_ctx.h): what it leaves is a default-constructed GeneratorState, and nothing outside the record
// moves.  Built by tests/test_generator_rule.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_host.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <type_traits>

using namespace kfsp;

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #x);             \
            ++failures;                                             \
        }                                                           \
    } while (0)

// the device build as it stood: `banded` started as the first line, the loop over the reaction slots counted nd (and
// cleared `banded` at a slot with more than one shift, which is not part of the rule), then the two tests
static bool banded_device_before(int nd, int64_t nloc, int64_t nnz_off, int64_t opt_format)
{
    bool banded = opt_format != 1 && nloc > 0;
    if (nd == 0 || nd > kMaxDiag) banded = false;
    if (banded && (double)nd * (double)nloc > 1.5 * (double)nnz_off + 1024.0) banded = false;
    return banded;
}

// the host build as it stood: nd counted the distinct column offsets and the function returned at the first offset
// beyond kMaxDiag (here: nd = kMaxDiag + 1)
static bool banded_host_before(int nd, int64_t nloc, int64_t nnz_off, int64_t opt_format)
{
    if (opt_format == 1 || nloc == 0) return false;
    if (nd > kMaxDiag) return false;
    if (nd == 0 || (double)nd * (double)nloc > 1.5 * (double)nnz_off + 1024.0) return false;
    return true;
}

static void check_banded_pays()
{
    const int64_t rows[] = {0, 1, 63, 64, 1000, 10000000};
    int yes = 0, no = 0;
    for (int64_t fmt = 0; fmt <= 1; ++fmt)
        for (int nd = 0; nd <= kMaxDiag + 1; ++nd)
            for (int64_t nloc : rows) {
                // the smallest count of off-diagonal entries at which nd diagonals of nloc rows still pay, and both sides of it
                int64_t b = ((int64_t)nd * nloc - 1024) * 2 / 3;
                if (b < 0) b = 0;
                for (int64_t nnz = b > 3 ? b - 3 : 0; nnz <= b + 3; ++nnz) {
                    const bool got = banded_pays(nd, nloc, nnz, fmt);
                    CHECK(got == banded_device_before(nd, nloc, nnz, fmt));
                    CHECK(got == banded_host_before(nd, nloc, nnz, fmt));
                    (got ? yes : no) += 1;
                }
                // (the exact boundary: nd * nloc = 1.5 * nnz + 1024 pays, one entry fewer does not)
                if (fmt == 0 && nd >= 1 && nd <= kMaxDiag && (int64_t)nd * nloc > 1024 && ((int64_t)nd * nloc - 1024) % 3 == 0) {
                    const int64_t e = ((int64_t)nd * nloc - 1024) / 3 * 2;
                    CHECK(banded_pays(nd, nloc, e, 0));
                    CHECK(!banded_pays(nd, nloc, e - 1, 0));
                }
            }
    CHECK(yes > 100 && no > 100);
    CHECK(banded_pays(1, 1, 0, 0) && !banded_pays(1, 1, 0, 1) && !banded_pays(0, 1, 100, 0) && !banded_pays(kMaxDiag + 1, 1, 100, 0));
    CHECK(banded_pays(kMaxDiag, 64, 0, 0));        // (64 * kMaxDiag entries fit the 1024 of grace)
}

static void check_want_state_order()
{
    const int64_t vals[] = {0, 1, 47, 48, 49, 32767, 32768, 32769, 1000000};
    for (int64_t on = 0; on <= 2; ++on)
        for (int64_t n : vals)
            for (int64_t min_n : vals)
                for (int64_t prod : vals)
                    for (int64_t min_prod : vals) {
                        const bool before = on && n >= min_n && prod >= min_prod;
                        CHECK(want_state_order(on, n, min_n, prod, min_prod) == before);
                    }
    auto ctx = std::make_unique<kfsp_ctx>();       // the defaults: 32768 states, 48 products
    ctx->prod_count = 48;
    CHECK(want_state_order(ctx.get(), 32768) && !want_state_order(ctx.get(), 32767));
    ctx->prod_count = 47;
    CHECK(!want_state_order(ctx.get(), 32768));
    ctx->prod_count = 48;
    ctx->opt_state_order = 0;
    CHECK(!want_state_order(ctx.get(), 32768));
}

static bool same_state(const GeneratorState &a, const GeneratorState &b)
{
    bool eq = a.nchunks == b.nchunks && a.slots == b.slots && a.nnz == b.nnz && a.use_dia == b.use_dia && a.nd == b.nd &&
              a.dia_ld == b.dia_ld && a.have_sell == b.have_sell && a.sell_coded == b.sell_coded && a.code_words == b.code_words &&
              a.coded_chunks == b.coded_chunks && a.coded_slots == b.coded_slots && a.coded_tab_bytes == b.coded_tab_bytes &&
              a.sell_reach == b.sell_reach && a.dia_coded == b.dia_coded && a.dia_code_w == b.dia_code_w &&
              a.dia_code_rec == b.dia_code_rec && a.dia_masked == b.dia_masked && a.dia_empty_segments == b.dia_empty_segments &&
              a.trip_order_n == b.trip_order_n;
    eq = eq && !std::memcmp(a.delta, b.delta, sizeof(a.delta)) && !std::memcmp(a.dia_doff, b.dia_doff, sizeof(a.dia_doff)) &&
         !std::memcmp(a.dia_distinct, b.dia_distinct, sizeof(a.dia_distinct));
    const DiaDiagDev &g = a.dia_diag, &h = b.dia_diag;
    eq = eq && g.nk == h.nk && g.ntab == h.ntab && g.base == h.base && !std::memcmp(g.size, h.size, sizeof(g.size)) &&
         !std::memcmp(g.stride, h.stride, sizeof(g.stride)) && !std::memcmp(g.toff, h.toff, sizeof(g.toff)) &&
         !std::memcmp(g.magic, h.magic, sizeof(g.magic)) && !std::memcmp(g.shift, h.shift, sizeof(g.shift));
    const BoxGeom &p = a.box, &q = b.box;
    eq = eq && p.on == q.on && p.fast == q.fast && p.pencil == q.pencil && p.simple == q.simple && p.plane_rows == q.plane_rows &&
         p.trips == q.trips && p.order_n == q.order_n && p.planes == q.planes && p.slab == q.slab && p.line_rows == q.line_rows &&
         p.lo_trips == q.lo_trips && p.lines == q.lines && p.waves == q.waves && p.groups == q.groups && p.lds_bytes == q.lds_bytes &&
         p.reach == q.reach && p.dev.ns == q.dev.ns && p.dev.nr == q.dev.nr && p.dev.ntab == q.dev.ntab &&
         !std::memcmp(p.dev.delta, q.dev.delta, sizeof(p.dev.delta));
    return eq;
}

static void check_reset()
{
    static_assert(std::is_base_of<GeneratorState, kfsp_ctx>::value, "the context IS the record: ctx->use_dia reads it");
    static_assert(std::is_trivially_copyable<GeneratorState>::value, "scalars only: no buffer, nothing that owns memory");
    const GeneratorState fresh{};
    CHECK(!fresh.use_dia && !fresh.have_sell && !fresh.box.on && fresh.sell_reach == -1 && fresh.nchunks == 0 && fresh.nd == 0);
    auto ctx = std::make_unique<kfsp_ctx>();
    CHECK(same_state(*ctx, fresh));
    // every byte of the record set (0x01: true, and non-zero everywhere), and what outlives a generator marked
    std::memset(static_cast<void *>(static_cast<GeneratorState *>(ctx.get())), 0x01, sizeof(GeneratorState));
    CHECK(!same_state(*ctx, fresh));
    CHECK(ctx->use_dia && ctx->dia_coded && ctx->dia_masked && ctx->have_sell && ctx->sell_coded && ctx->box.on && ctx->nd != 0);
    ctx->dia_code_us = 7;
    ctx->last_build_sell = true;
    ctx->kc_ok = true;
    ctx->h_build_ready = true;
    ctx->ell_cols = 11;
    ctx->ell_ld = 12;
    ctx->ell_bw = 13;
    ctx->coords_n = 14;
    ctx->order_n = 15;
    ctx->skeys_n = 16;
    ctx->spec_builds = 17;
    ctx->spec_redone = 18;
    ctx->prod_count = 19;
    ctx->prod_last = 20;
    ctx->w_pending = true;
    ctx->w_pending_n = 21;
    ctx->perm_on = true;
    ctx->n = 22;
    ctx->opt_format = 1;
    reset_generator(ctx.get());
    CHECK(same_state(*ctx, fresh));
    CHECK(ctx->dia_code_us == 7 && ctx->last_build_sell && ctx->kc_ok && ctx->h_build_ready && ctx->ell_cols == 11 && ctx->ell_ld == 12 &&
          ctx->ell_bw == 13 && ctx->coords_n == 14 && ctx->order_n == 15 && ctx->skeys_n == 16 && ctx->spec_builds == 17 &&
          ctx->spec_redone == 18 && ctx->prod_count == 19 && ctx->prod_last == 20 && ctx->w_pending && ctx->w_pending_n == 21 &&
          ctx->perm_on && ctx->n == 22 && ctx->opt_format == 1);
    // what reads the record sees "no generator": SELL-64 without coded columns, nothing coded, no box
    CHECK(product_format(product_form(ctx.get(), false)) == 0 && !dia_code_on(ctx.get()));
}

int main()
{
    check_banded_pays();
    check_want_state_order();
    check_reset();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
