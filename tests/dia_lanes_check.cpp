// Stand-alone host program for the lane path of the folded banded product (csrc/kfsp_dia_diag.h: dia_xpair_clamp,
// dia_lanes_trip, dia_lanes_edge - the very functions the kernel calls; tests/test_dia_lanes_host.py compiles it under
// AddressSanitizer / UBSan and runs it).  For every n in [n0, n1], every 128-row trip and the offset sets {+-1, +-s} and
// {+-1, +-s, +-s t} it plays one wavefront: x is a buffer of exactly n + 2 doubles (the guard word, x[0 .. n), the guard
// word), each holding its own index, so a read outside it is an AddressSanitizer error and a wrong word a wrong value.
//   * where the rule admits the lane path: the clamp acts on no lane's own pair nor on its -1 / +1 pairs, and the words the
//     lane mapping names - lane l - 1's second word, lane l + 1's first word, the two edge words - are the words
//     ld_xpair would read;
//   * where it refuses: the trip holds row `last` or rows of the padding;
//   * it refuses at most one trip of a generator.
// Prints "ok <trips> <admitted> <refused>"; any failure prints what failed and returns 1.
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
            sets.push_back({-s, -1, 1, s});
            for (int t : {2, 5}) sets.push_back({-s * t, -s, -1, 1, s, s * t});
        }
        long long refused = 0;
        for (long long c = 0; c < trips; ++c) {
            const int64_t g0 = 128 * c;
            const bool lanes = dia_lanes_trip(g0, n);
            ++trips_all;
            if (!lanes) {
                ++refused;
                const bool has_last = g0 <= last && last <= g0 + 127, has_padding = g0 + 127 > last;
                if (!has_last && !has_padding) return fail("a refused trip holds neither row last nor padding", n, c, -1, 0);
            } else {
                ++admitted_all;
            }
            // the wavefront: every lane's own pair, and the edge words of lanes 0 and 63
            Pair xd[64];
            for (int l = 0; l < 64; ++l) xd[l] = ld_xpair(x, g0 + 2 * l, last);
            double edge[64] = {};
            if (lanes) {
                for (int l : {0, 63}) {
                    const int64_t at = dia_lanes_edge(g0, l);
                    if (at < -1 || at > n) return fail("an edge word outside x and its guard words", n, c, l, 0);
                    edge[l] = x[at];
                }
            }
            for (const std::vector<int> &delta : sets) {
                for (int l = 0; l < 64; ++l) {
                    const int64_t g = g0 + 2 * l;
                    if (lanes && dia_xpair_clamp(g, last) != g) return fail("the clamp acts on xd of an admitted trip", n, c, l, 0);
                    for (int d : delta) {
                        const Pair want = ld_xpair(x, g + d, last);
                        Pair got = want;
                        if (lanes && (d == -1 || d == 1)) {
                            if (dia_xpair_clamp(g + d, last) != g + d) return fail("the clamp acts on a +-1 pair of an admitted trip", n, c, l, d);
                            if (d == -1) got = Pair{l == 0 ? edge[0] : xd[l - 1].y, xd[l].x};
                            else got = Pair{xd[l].y, l == 63 ? edge[63] : xd[l + 1].x};
                            // the words themselves: x holds its own indices
                            if (want.x != (double)(g + d) || want.y != (double)(g + d + 1)) return fail("ld_xpair of an admitted trip reads other words", n, c, l, d);
                        }
                        if (got.x != want.x || got.y != want.y) return fail("the lane mapping names other words than ld_xpair reads", n, c, l, d);
                    }
                }
            }
        }
        if (refused > 1) return fail("more than one trip of a generator refused", n, refused, -1, 0);
        if (refused != (n % 128 != 0 ? 1 : 0)) return fail("the refused trips are not exactly the partial last one", n, refused, -1, 0);
        refused_all += refused;
    }
    std::printf("ok %lld %lld %lld\n", trips_all, admitted_all, refused_all);
    return 0;
}
