// Stand-alone check of the dispatch helpers of the block product (kfsp_block_dev.h): kp_index, and the constants that
// dispatch_kp, dispatch_bool, dispatch_kp_dots and dispatch_box_inst hand to their callable - against the cases the
// switches they replaced spelled out, `default:` branches included.  Built by tests/test_block_dispatch.py with
// -fsanitize=address,undefined; prints "ok".
#include "kfsp_block_dev.h"

#include <cstdio>
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

// the width a kernel would be instantiated with, as a compile-time constant of the argument's type
static int kp_seen(int kp)
{
    return dispatch_kp(kp, [](auto KP) {
        static_assert(std::is_same<decltype(KP), std::integral_constant<int, decltype(KP)::value>>::value, "a constant, not a value");
        return (int)decltype(KP)::value;
    });
}

int main()
{
    static_assert(kp_index(2) == 0 && kp_index(4) == 1 && kp_index(8) == 2 && kp_index(16) == 3, "log2(kp) - 1");
    const int widths[] = {2, 4, 8, 16};
    for (int i = 0; i < 4; ++i) {
        CHECK(kp_index(widths[i]) == i);
        CHECK((2 << kp_index(widths[i])) == widths[i]);
        CHECK(kp_seen(widths[i]) == widths[i]);
    }
    // anything else is the `default:` of the switches: the widest instantiation
    for (int kp : {-1, 0, 1, 3, 5, 6, 7, 9, 12, 15, 17, 32, 1 << 20}) {
        CHECK(kp_seen(kp) == 16);
        CHECK(kp_index(kp) == 3);
    }
    for (bool on : {false, true}) {
        CHECK(dispatch_bool(on, [](auto B) { return (bool)decltype(B)::value; }) == on);
        for (int kp : {2, 4, 8, 16, 5})
            CHECK(dispatch_kp_dots(kp, on, [](auto KP, auto DOTS) { return 100 * (int)decltype(KP)::value + (decltype(DOTS)::value ? 1 : 0); }) ==
                  100 * (kp == 5 ? 16 : kp) + (on ? 1 : 0));
    }
    // a void callable goes through as well (the launches)
    int hit = 0;
    dispatch_kp(8, [&](auto KP) { hit = decltype(KP)::value; });
    CHECK(hit == 8);
    // the single-factor box instantiations: species * 16 + slots per species, anything else the widest (6 species, 4 slots)
    auto inst_seen = [](int inst) { return dispatch_box_inst(inst, [](auto NS, auto PER) { return 16 * (int)decltype(NS)::value + (int)decltype(PER)::value; }); };
    for (int inst : {2 * 16 + 2, 3 * 16 + 2, 6 * 16 + 2, 6 * 16 + 4}) CHECK(inst_seen(inst) == inst);
    for (int inst : {0, 1 * 16 + 2, 2 * 16 + 4, 4 * 16 + 2, 6 * 16 + 3, 8 * 16 + 2, -1}) CHECK(inst_seen(inst) == 6 * 16 + 4);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
