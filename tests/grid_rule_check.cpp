// Stand-alone check of the launch rule of the generator product (kfsp_host.h): product_trips and product_grid against
// a plain restatement of the formulas the callers spelled out by hand before there was one rule.  Built by
// tests/test_grid_rule.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_host.h"

#include <cstdint>
#include <cstdio>

using namespace kfsp;

static int failures = 0;
#define CHECK(x)                                                    \
    do {                                                            \
        if (!(x)) {                                                 \
            std::printf("line %d: %s\n", __LINE__, #x);             \
            ++failures;                                             \
        }                                                           \
    } while (0)

static int64_t up8(int64_t a) { return (a + 7) / 8 * 8; }

// the grid as the whole-product launch wrote it: round_up((t + 3) / 4, 8), the cap (option grid_blocks rounded up to 8,
// or the default), at least 8 - and no bound by the partial slot
static int64_t grid_before(int64_t trips, int64_t opt_grid, int64_t dflt_cap)
{
    int64_t g = up8((trips + 3) / 4);
    const int64_t cap = opt_grid > 0 ? up8(opt_grid) : dflt_cap;
    if (g > cap) g = cap;
    return g < 8 ? 8 : g;
}

int main()
{
    CHECK(kMaxGrid == 2048);
    const int64_t trips[] = {1, 3, 4, 31, 32, 33, 4095, 8192, 8193, 16385, 1000000};
    const int64_t grids[] = {0, 1, 8, 24, 768, 1000, 2048, 2049, 4096, (int64_t)1 << 20};
    const int64_t caps[] = {1024, 768, 256, 512};
    int clamped = 0;
    for (int64_t t : trips)
        for (int64_t o : grids)
            for (int64_t c : caps) {
                const int64_t before = grid_before(t, o, c), now = product_grid(t, o, c);
                if (before <= 2048) CHECK(now == before);
                else {
                    CHECK(now == 2048);
                    ++clamped;
                }
                if (now != (before <= 2048 ? before : 2048)) std::printf("trips %lld grid_blocks %lld cap %lld: %lld, before %lld\n",
                                                                         (long long)t, (long long)o, (long long)c, (long long)now, (long long)before);
            }
    CHECK(clamped > 0);                                      // the sweep reaches the case the rule exists for
    // a trip is one 64-row chunk, or two of them in the banded and matrix-free forms
    for (int64_t n : {0, 1, 2, 3, 8193, 1000001}) {
        CHECK(product_trips(n, false) == n);
        CHECK(product_trips(n, true) == (n + 1) / 2);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
