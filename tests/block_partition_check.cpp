// Stand-alone check of the rules the block path shares with the single-vector path under a row partition
// (kfsp_host.h): product_split against the (lo, hi, split?) arithmetic run_product wrote out itself before there was one
// rule, and the margins of a block column (halo_margin, block_margin).  Built by tests/test_block_partition_rule.py with
// -fsanitize=address,undefined; prints "ok".
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

// run_product, as it stood: lo = first trip whose rows all lie >= H, trips [lo, hi) end at or below L - H, and the split
// only where hi - lo reaches 16384 trips (64 under overlap >= 2); overlap = 0 never splits
static void split_before(int64_t H, int64_t L, int64_t trips, int64_t trip_rows, int64_t overlap, int64_t *lo, int64_t *hi, bool *split)
{
    *split = overlap != 0;
    *lo = (H + trip_rows - 1) / trip_rows;
    int64_t h = (L - H) / trip_rows;
    if (h > trips) h = trips;
    *hi = h;
    const int64_t min_trips = overlap >= 2 ? 64 : 16384;
    if (*hi - *lo < min_trips) *split = false;
}

int main()
{
    const int64_t Ls[] = {64, 128, 448, 704, 768, 1024, 8192, 21120, 31680, 2097152, 4194304};
    const int64_t Hs[] = {8, 16, 40, 64, 104, 300, 304, 1000, 4096};
    const int64_t overlaps[] = {0, 1, 2, 3};
    int n_split = 0, n_small = 0, n_full = 0, n_tight = 0;
    for (int64_t L : Ls)
        for (int64_t tr : {(int64_t)64, (int64_t)128})
            for (int64_t Hx : {(int64_t)-1, (int64_t)-2, (int64_t)-3, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)6,
                               (int64_t)7, (int64_t)8}) {
                // H from the list, and the edges: H = L, H just above L - trip_rows, H = L - trip_rows
                const int64_t H = Hx == -1 ? L : (Hx == -2 ? L - tr + 8 : (Hx == -3 ? L - tr : Hs[Hx]));
                if (H < 8 || H > L) continue;                     // setup_exchange agrees on 8 <= H <= L, a multiple of 8
                // trips of a rank that owns all L rows, of a ragged last rank, of an empty one
                const int64_t full = (L + tr - 1) / tr;
                for (int64_t trips : {full, full / 2, (int64_t)63, (int64_t)1, (int64_t)0})
                    for (int64_t ov : overlaps) {
                        int64_t lo, hi;
                        bool sp;
                        split_before(H, L, trips, tr, ov, &lo, &hi, &sp);
                        const ProductSplit ps = product_split(H, L, trips, tr, ov);
                        CHECK(ps.lo == lo);
                        CHECK(ps.hi == hi);
                        CHECK(ps.split == sp);
                        if (ps.split) {
                            ++n_split;
                            // the interior reads no halo row and the boundary ranges fit their launch
                            CHECK(ps.lo * tr >= H);
                            CHECK(ps.hi * tr <= L - H);
                            CHECK(ps.hi <= trips);
                            CHECK(ps.hi - ps.lo >= 64);
                            CHECK(ps.lo + (trips - ps.hi) >= 1);
                        }
                        if (trips < 64) {
                            ++n_small;
                            CHECK(!ps.split);
                        }
                        if (H == L) {
                            ++n_full;
                            CHECK(!ps.split);
                        }
                        if (H > L - tr) {
                            ++n_tight;
                            CHECK(!ps.split);
                        }
                    }
            }
    CHECK(n_split > 0);
    CHECK(n_small > 0);
    CHECK(n_full > 0);
    CHECK(n_tight > 0);
    // the cases the device tests rely on: 247 banded trips of 31680 rows and 165 of 21120, strips of 304 rows
    CHECK(product_split(304, 31680, 248, 128, 2).split && product_split(304, 31680, 248, 128, 2).lo == 3 &&
          product_split(304, 31680, 248, 128, 2).hi == 245);
    CHECK(product_split(304, 21120, 165, 128, 2).split);
    CHECK(!product_split(304, 21120, 165, 128, 1).split);
    // margins: room for the strip plus one 128-row group, a multiple of 64, and a block column never below its 64 rows
    CHECK(kBlockMargin == 64);
    for (int64_t H = 8; H <= 1 << 20; H += (H < 4096 ? 8 : 4088)) {
        const int64_t m = halo_margin(H);
        CHECK(m >= H + 128);
        CHECK(m % 64 == 0);
        CHECK(block_margin(m) == m);
        CHECK(block_margin(m) >= kBlockMargin);
    }
    CHECK(block_margin(0) == kBlockMargin);
    CHECK(block_margin(63) == kBlockMargin);
    CHECK(block_margin(64) == 64);
    CHECK(block_margin(192) == 192);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
