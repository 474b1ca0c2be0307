// Stand-alone host program for the interior trips of the folded banded product (csrc/kfsp_dia_diag.h: dia_inner_trip,
// dia_inner_base, dia_xpair_clamp - the very functions the kernel calls; tests/test_dia_inner_host.py compiles it under
// AddressSanitizer / UBSan and runs it).  For every n in [n0, n1], every 128-row trip and the offset sets {+-1, +-s} and
// {+-1, +-s, +-s t} it plays one wavefront: x is a buffer of exactly n + 2 doubles (the guard word, x[0 .. n), the guard
// word), each holding its own index, so a read outside it is an AddressSanitizer error and a wrong word a wrong value.
//   * where the rule admits the trip: lane l's pair of diagonal delta (0, the row itself, included), read at the uniform
//     index dia_inner_base(g0, delta) plus the lane's 2 l, is the pair ld_xpair reads; no clamp acts; no row belongs to
//     the padding - both flags of dia_diag_value are true and gq == g;
//   * the rule refuses exactly the trips in which some lane's clamp or padding flag acts;
//   * it admits at least one trip once n >= 2 dmax + 384.
// Prints "ok <trips> <admitted> <refused>" (summed over the offset sets); any failure prints what failed and returns 1.
#include "kfsp_dia_diag.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace kfsp;

struct Pair {
    double x, y;
};

// what ld_xpair reads for index p (kfsp_kernels.hip): x[p], x[p + 1] after the clamp
static Pair ld_xpair(const double *x, int64_t p, int64_t last)
{
    p = dia_xpair_clamp(p, last);
    return Pair{x[p], x[p + 1]};
}
// what rows_dia_inner reads: 16 bytes at byte offset 16 l of the uniform address x + base
static Pair ld_lane16(const double *x, int64_t base, int lane)
{
    const char *p = reinterpret_cast<const char *>(x + base) + 16u * (unsigned)lane;
    const double *q = reinterpret_cast<const double *>(p);
    return Pair{q[0], q[1]};
}

static int fail(const char *what, long long n, long long trip, int lane, int delta)
{
    std::printf("FAILED %s: n %lld trip %lld lane %d delta %d\n", what, n, trip, lane, delta);
    return 1;
}

int main(int argc, char **argv)
{
    const long long n0 = argc > 1 ? std::atoll(argv[1]) : 1, n1 = argc > 2 ? std::atoll(argv[2]) : 1100;
    long long trips_all = 0, admitted_all = 0, refused_all = 0;
    for (long long n = n0; n <= n1; ++n) {
        std::vector<double> buf((size_t)n + 2);
        for (long long i = 0; i < n + 2; ++i) buf[(size_t)i] = (double)(i - 1);     // x[i] = i, the guard words -1 and n
        const double *x = buf.data() + 1;
        const int64_t last = n - 1;
        const long long nchunks = (n + 63) / 64, trips = (nchunks + 1) / 2;          // product_trips of the banded form
        std::vector<std::vector<int>> sets;
        for (int s : {2, 3, 7, 16, 31}) {
            sets.push_back({-s, -1, 0, 1, s});
            for (int t : {2, 5}) sets.push_back({-s * t, -s, -1, 0, 1, s, s * t});
        }
        for (const std::vector<int> &delta : sets) {
            const int64_t dmin = delta.front(), dmax = delta.back();
            long long admitted = 0;
            for (long long c = 0; c < trips; ++c) {
                const int64_t g0 = 128 * c;
                const bool inner = dia_inner_trip(g0, n, dmin, dmax);
                ++trips_all;
                bool acts = false;                       // some lane's clamp or padding flag
                for (int l = 0; l < 64; ++l) {
                    const int64_t g = g0 + 2 * l;
                    const bool flag_a = g <= last, flag_b = g < last;             // the in_range flags of the lane's two rows
                    const uint32_t gq = (uint32_t)g < (uint32_t)last ? (uint32_t)g : (uint32_t)last;
                    if (!flag_a || !flag_b) acts = true;
                    if (inner && (!flag_a || !flag_b)) return fail("an admitted trip holds a row of the padding", n, c, l, 0);
                    if (inner && (int64_t)gq != g) return fail("gq differs from g in an admitted trip", n, c, l, 0);
                    for (int d : delta) {
                        const bool clamped = dia_xpair_clamp(g + d, last) != g + d;
                        if (clamped) acts = true;
                        if (!inner) continue;
                        if (clamped) return fail("the clamp acts in an admitted trip", n, c, l, d);
                        const Pair want = ld_xpair(x, g + d, last);
                        const Pair got = ld_lane16(x, dia_inner_base(g0, d), l);
                        if (want.x != (double)(g + d) || want.y != (double)(g + d + 1)) return fail("ld_xpair of an admitted trip reads other words", n, c, l, d);
                        if (got.x != want.x || got.y != want.y) return fail("the base-plus-lane mapping names other words than ld_xpair reads", n, c, l, d);
                    }
                }
                if (inner == acts) return fail(inner ? "an admitted trip in which a clamp or a padding flag acts" : "a refused trip in which nothing acts", n, c, -1, 0);
                admitted += inner ? 1 : 0;
            }
            if (n >= 2 * dmax + 384 && admitted == 0) return fail("no trip admitted although n >= 2 dmax + 384", n, -1, -1, (int)dmax);
            admitted_all += admitted;
            refused_all += trips - admitted;
        }
    }
    std::printf("ok %lld %lld %lld\n", trips_all, admitted_all, refused_all);
    return 0;
}
