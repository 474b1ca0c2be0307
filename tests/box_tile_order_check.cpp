// Stand-alone check of box_tile_order and of what option "box_tile" asks of it (kfsp_box_plan.h): the order is a permutation
// of the trips or empty, and empty exactly where the rule says so.  With arguments - force, then the dimensions fastest
// first - it prints the order, one trip per line, for tests/test_box_gated_cases.py to compare with its own restatement.
// Built there with -fsanitize=address,undefined; without arguments it prints "ok".
#include "kfsp_host.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static std::vector<int32_t> order_of(const std::vector<int32_t> &dims, bool force)
{
    int64_t n = 1;
    for (int32_t d : dims) n *= d;
    return box_tile_order((int)dims.size(), dims.data(), n, force);
}

static bool is_permutation(const std::vector<int32_t> &o, int64_t trips)
{
    if ((int64_t)o.size() != trips) return false;
    std::vector<char> seen((size_t)trips, 0);
    for (int32_t c : o) {
        if (c < 0 || c >= trips || seen[(size_t)c]) return false;
        seen[(size_t)c] = 1;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc > 2) {
        std::vector<int32_t> dims;
        for (int i = 2; i < argc; ++i) dims.push_back((int32_t)std::atoi(argv[i]));
        for (int32_t c : order_of(dims, std::atoi(argv[1]) != 0)) std::printf("%d\n", (int)c);
        return 0;
    }
    // the planes of the test boxes: a permutation of all base trips, a last trip of 112 rows included
    const std::vector<std::vector<int32_t>> tiled = {{8, 8, 8, 8, 2}, {10, 10, 6, 5, 2}, {6, 8, 8, 8, 3}, {8, 8, 8, 4, 2}, {2048, 3, 5}, {16384, 2, 2}};
    for (const auto &d : tiled) {
        int64_t n = 1;
        for (int32_t v : d) n *= v;
        const std::vector<int32_t> o = order_of(d, true);
        CHECK(is_permutation(o, (n + 127) / 128));
        bool identity = true;
        for (size_t i = 0; i < o.size(); ++i) identity = identity && o[i] == (int32_t)i;
        CHECK(!identity);
        CHECK(order_of(d, false).empty());               // small boxes: only when forced
    }
    // fewer than three species; no stride of a species but the first within 2048 .. 16384 rows; a single trip
    CHECK(order_of({4096, 8}, true).empty());
    CHECK(order_of({4096}, true).empty());
    CHECK(order_of({8, 8, 8, 2, 2}, true).empty());      // the largest stride is 1024
    CHECK(order_of({13, 11, 2}, true).empty());
    CHECK(order_of({20000, 3, 3}, true).empty());        // the only strides are 20000 and 60000
    CHECK(order_of({4, 4, 4}, true).empty());            // 64 rows: one trip
    // not forced, but beyond the caches: 2^28 rows whose slowest stride is 2^24 rows
    {
        const std::vector<int32_t> d = {4096, 4096, 16};
        const std::vector<int32_t> o = order_of(d, false);
        CHECK(is_permutation(o, ((int64_t)1 << 28) / 128));
    }
    // option box_tile: 0 never asks, 1 forces, -1 forces on a plane beyond 4 MiB
    CHECK(!box_tile_wanted(0) && box_tile_wanted(1) && box_tile_wanted(-1));
    CHECK(box_tile_force(1, 64) && !box_tile_force(-1, 64) && !box_tile_force(-1, 524288) && box_tile_force(-1, 524289));
    CHECK(!box_tile_force(0, 524289));
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
