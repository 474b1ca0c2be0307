// Stand-alone check of the host planning of a matrix-free box (box_plan, kfsp_box_plan.h) and of the kernel-format rule
// (product_format, kfsp_host.h).  Built by tests/test_box_plan_host.py with -fsanitize=address,undefined.
//   without arguments   walks every flag combination of product_format against the two nested conditionals the rule
//                       replaced (run_product's and kfsp_layout_info's, copied below as the expectation); prints "ok"
//   "plan"              reads models from stdin until it ends and prints the plan of each under each of its option sets,
//                       as text, for the test to compare with its own restatements:
//                         model <null mask> <ns> <nr> <option sets> <lengths of the five arrays>
//                         dims | stoich[k * ns + s] | ndep | dep_species[k * 3 + i] | tables   (one line each)
//                         <box_pencil> <box_slab_waves> <box_tile> <box_reach> <single>        (one line per option set)
//                       null mask: bit 0 dims, 1 stoich, 2 ndep, 3 dep_species, 4 tables are passed as null pointers.
//                       Every array goes to box_plan in a heap block of exactly its length: an overrun is the sanitizer's.
#include "kfsp_host.h"

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace kfsp;

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #x);             \
            ++failures;                                             \
        }                                                           \
    } while (0)

// ---- the rule as it stood before product_format, in its two places
struct Flags {
    bool use_dia, use_box, box_fast, box_slab, box_pencil, use_comm, ordered, coded_on, dia_masked, sell_coded, force_sell, force_plain_sell;
    int box_reach;
    int64_t opt_box_pencil, opt_box_lds, opt_box_generic;
};

static int launch_before(const Flags &c)   // run_product
{
    const bool dia = c.use_dia && !c.force_sell;
    const int fmt = (c.use_box && dia) ? (c.box_fast && !c.opt_box_generic ? 4 : 3)
                                       : (dia ? (c.coded_on ? 9 : (c.dia_masked ? 2 : 1))
                                              : (c.sell_coded && !c.force_plain_sell ? 5 : 0));
    if (fmt == 4 && c.box_slab && c.opt_box_pencil == 2 && !c.use_comm && c.opt_box_lds == 0) return 8;
    if (fmt == 4 && c.box_pencil && c.opt_box_pencil != 0 && !c.use_comm && c.opt_box_lds == 0) return 7;
    if (fmt == 4 && c.box_reach > 0 && c.opt_box_lds != 0 && !c.use_comm && !c.ordered) return 6;
    return fmt;
}

static int report_before(const Flags &c)   // kfsp_layout_info
{
    return c.use_box ? (c.box_fast && !c.opt_box_generic ? (c.box_reach > 0 && c.opt_box_lds && !c.use_comm ? 6 :
                           (c.box_slab && c.opt_box_pencil == 2 && !c.use_comm ? 8 :
                            c.box_pencil && c.opt_box_pencil != 0 && !c.use_comm ? 7 : 4)) : 3) : c.use_dia ? (c.dia_masked ? 2 : 1) : (c.sell_coded ? 5 : 0);
}

static int walk_format_rule()
{
    long walked = 0, reachable = 0, report_differs = 0;
    int seen[10] = {0};
    for (int bits = 0; bits < (1 << 13); ++bits)
        for (int64_t pencil : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2})
            for (int64_t lds : {(int64_t)0, (int64_t)1}) {
                auto bit = [&](int i) { return ((bits >> i) & 1) != 0; };
                Flags c{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9), bit(10), bit(11),
                        bit(12) ? 2 : 0, pencil, lds, 0};
                const ProductForm f{c.use_dia, c.use_box, c.box_fast && !c.opt_box_generic, c.box_slab, c.box_pencil, c.box_reach > 0,
                                    c.opt_box_pencil, c.opt_box_lds, c.use_comm, c.ordered, c.coded_on, c.dia_masked, c.sell_coded,
                                    c.force_sell, c.force_plain_sell};
                const int got = product_format(f);
                ++walked;
                CHECK(got >= 0 && got <= 9);
                CHECK(got == launch_before(c));                       // every combination, reachable or not
                if (got >= 0 && got <= 9) ++seen[got];
                // what a context can be in: a box is banded; the coded image is read only from a stored, unmasked generator
                // without a communicator (dia_code_on); the report knows no forced variant and no trip order
                const bool can_be = (!c.use_box || c.use_dia) && (!c.coded_on || (c.use_dia && !c.use_box && !c.dia_masked && !c.use_comm));
                if (!can_be || c.force_sell || c.force_plain_sell || c.ordered) continue;
                ++reachable;
                const int report = got == 9 ? 1 : got;                  // kfsp_layout_info keeps answering 1 for format 9
                // The report before named 7 / 8 for an eligible box under box_lds = 1 without a reach, where the launch
                // (its tests of 7 and 8 require box_lds = 0) took 4: there the one rule follows the launch.
                const bool stale = c.use_box && c.box_fast && !c.use_comm && c.opt_box_lds != 0 && c.box_reach == 0 &&
                                   ((c.box_slab && c.opt_box_pencil == 2) || (c.box_pencil && c.opt_box_pencil != 0));
                if (stale) {
                    ++report_differs;
                    CHECK(report == 4 && launch_before(c) == 4 && (report_before(c) == 7 || report_before(c) == 8));
                } else {
                    CHECK(report == report_before(c));
                }
            }
    for (int f = 0; f <= 9; ++f) CHECK(seen[f] > 0);
    CHECK(walked == (1L << 13) * 8 && reachable > 0 && report_differs > 0);
    // a trip order is the one input that separates report and launch: format 6 runs as 4
    {
        ProductForm f{true, true, true, false, false, true, -1, 1, false, false, false, false, false, false, false};
        CHECK(product_format(f) == 6);
        f.trip_order = true;
        CHECK(product_format(f) == 4);
    }
    // 7 and 8 are told apart by the option, and 8 wins where both apply
    {
        ProductForm f{true, true, true, true, true, true, 2, 0, false, false, false, false, false, false, false};
        CHECK(product_format(f) == 8);
        f.box_pencil = 1;
        CHECK(product_format(f) == 7);
        f.box_pencil = 2;
        f.slab = false;
        CHECK(product_format(f) == 7);
        f.box_pencil = 0;
        CHECK(product_format(f) == 4);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}

// ---- "plan"
template <class T>
static void line(const char *key, const T *v, size_t n)
{
    std::printf("%s", key);
    for (size_t i = 0; i < n; ++i) std::printf(" %lld", (long long)v[i]);
    std::printf("\n");
}

static void bits_line(const char *key, const double *v, size_t n)
{
    std::printf("%s", key);
    for (size_t i = 0; i < n; ++i) {
        uint64_t u;
        std::memcpy(&u, v + i, 8);
        std::printf(" %016" PRIx64, u);
    }
    std::printf("\n");
}

template <class T>
static bool read_n(std::vector<T> &v, size_t n)
{
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        char tok[64];
        if (std::scanf("%63s", tok) != 1) return false;
        v[i] = (T)std::strtod(tok, nullptr);                         // (integers and hexadecimal doubles alike)
    }
    return true;
}

static int print_plans()
{
    char word[16];
    int model = 0;
    while (std::scanf("%15s", word) == 1) {
        if (std::strcmp(word, "model") != 0) return 2;
        int mask, ns, nr, nsets;
        long len[5];
        if (std::scanf("%d %d %d %d %ld %ld %ld %ld %ld", &mask, &ns, &nr, &nsets, len, len + 1, len + 2, len + 3, len + 4) != 9) return 2;
        std::vector<int32_t> dims, stoich, ndep, dep;
        std::vector<double> tables;
        if (!read_n(dims, (size_t)len[0]) || !read_n(stoich, (size_t)len[1]) || !read_n(ndep, (size_t)len[2]) || !read_n(dep, (size_t)len[3]) ||
            !read_n(tables, (size_t)len[4]))
            return 2;
        for (int j = 0; j < nsets; ++j) {
            long long o[5];
            if (std::scanf("%lld %lld %lld %lld %lld", o, o + 1, o + 2, o + 3, o + 4) != 5) return 2;
            BoxPlanOpts opt;
            opt.box_pencil = o[0];
            opt.box_slab_waves = o[1];
            opt.box_tile = o[2];
            opt.box_reach = o[3];
            opt.single = o[4] != 0;
            std::vector<BoxPlan> plan(1);
            BoxPlan &P = plan[0];
            const char *what = "";
            const int rc = box_plan(ns, mask & 1 ? nullptr : dims.data(), nr, mask & 2 ? nullptr : stoich.data(), mask & 4 ? nullptr : ndep.data(),
                                    mask & 8 ? nullptr : dep.data(), mask & 16 ? nullptr : tables.data(), opt, P, &what);
            std::printf("plan %d %d\nrc %d\n", model, j, rc);
            if (rc != 0) {
                std::printf("what %s\nend\n", what);
                continue;
            }
            const BoxGeom &G = P.g;
            const BoxDev &B = G.dev;
            const long long head[] = {P.n, P.nnz, G.on, G.fast, (long long)G.lds_bytes, G.reach};
            line("n_nnz_on_fast_lds_reach", head, 6);
            const long long pencil[] = {G.pencil, G.simple, G.plane_rows, G.planes, G.trips, G.order_n};
            line("pencil", pencil, 6);
            const long long slab[] = {G.slab, G.line_rows, G.lines, G.groups, G.waves, G.lo_trips};
            line("slab", slab, 6);
            line("order", P.order.data(), P.order.size());
            const long long b[] = {B.ns, B.nr, B.ntab, B.pad};
            line("B", b, 4);
            line("B.dims", B.dims, kBoxMaxS);
            bits_line("B.inv_dim", B.inv_dim, kBoxMaxS);
            line("B.delta", B.delta, kBoxMaxR);
            line("B.dorder", B.dorder, kBoxMaxR);
            line("B.ndep", B.ndep, kBoxMaxR);
            line("B.nmov", B.nmov, kBoxMaxR);
            line("B.dep_s", &B.dep_s[0][0], kBoxMaxR * kBoxMaxDep);
            line("B.dep_nu", &B.dep_nu[0][0], kBoxMaxR * kBoxMaxDep);
            line("B.dep_off", &B.dep_off[0][0], kBoxMaxR * kBoxMaxDep);
            line("B.mov_s", &B.mov_s[0][0], kBoxMaxR * kBoxMaxDep);
            line("B.mov_nu", &B.mov_nu[0][0], kBoxMaxR * kBoxMaxDep);
            line("B.mov_dim", &B.mov_dim[0][0], kBoxMaxR * kBoxMaxDep);
            const BoxFast &F = P.F;
            const long long f[] = {F.ns, F.per, F.bias8, F.pad1};
            line("F", f, 4);
            line("F.dims", F.dims, kBoxFastS);
            bits_line("F.inv_dim", F.inv_dim, kBoxFastS);
            line("F.koff8", &F.koff8[0][0], kBoxFastS * kBoxFastPer);
            line("F.delta8", &F.delta8[0][0], kBoxFastS * kBoxFastPer);
            line("F.df8", F.df8, kBoxFastS);
            // the image ends in the very BoxFast the plan names; its doubles are printed once per model (no option touches them)
            const size_t tail = (sizeof(BoxFast) + 7) / 8;
            const long long img[] = {(long long)P.image.size(), P.image.size() >= tail && std::memcmp(P.image.data() + (P.image.size() - tail), &F, sizeof(F)) == 0};
            line("image_size_tail", img, 2);
            if (j == 0) bits_line("image", P.image.data(), P.image.size() - tail);
            std::printf("end\n");
        }
        ++model;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "plan") == 0) return print_plans();
    return walk_format_rule();
}
