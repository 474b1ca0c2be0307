// Stand-alone check of the host-side helpers of the transposed block product (kfsp_block_dev.h): box_adj_build and
// ell_adj_resident - and that box_plan (kfsp_box_plan.h) yields the descriptor written by hand below, but for the table
// offsets (the fixture spaces its tables 10 doubles apart, a caller's lie back to back).  Built by
// tests/test_block_adjoint_host.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_block_dev.h"
#include "kfsp_box_plan.h"

#include <cstdio>
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

// a toggle-like box dims (7, 5): reactions sorted by ascending source offset -nu . stride
//   p = 0: species 1 +1 (source offset -7), p = 1: species 0 +1 (-1), p = 2: species 0 -1 (+1), p = 3: species 1 -1 (+7);
//   the propensities of p = 0, 2 depend on species 0, those of p = 1, 3 on species 1
static BoxDev toggle_like()
{
    BoxDev B;
    std::memset(&B, 0, sizeof(B));
    B.ns = 2;
    B.nr = 4;
    B.pad = 2 * 16 + 2;
    B.dims[0] = 7;
    B.dims[1] = 5;
    const int delta[4] = {-7, -1, 1, 7}, dep[4] = {0, 1, 0, 1}, mov[4] = {1, 0, 0, 1}, nu[4] = {1, 1, -1, -1};
    for (int p = 0; p < 4; ++p) {
        B.delta[p] = delta[p];
        B.ndep[p] = 1;
        B.dep_s[p][0] = (int8_t)dep[p];
        B.dep_off[p][0] = 2 + 10 * p;
        B.nmov[p] = 1;
        B.mov_s[p][0] = (int8_t)mov[p];
        B.mov_nu[p][0] = (int8_t)nu[p];
    }
    return B;
}

// the same model planned, the reactions in the order of the fixture: what box_adj_build reads is the hand-written descriptor
static void planned_is_the_hand_written_one()
{
    const std::vector<int32_t> dims = {7, 5}, stoich = {0, 1, 1, 0, -1, 0, 0, -1}, ndep = {1, 1, 1, 1}, dep = {0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0};
    const std::vector<double> tables(7 + 5 + 7 + 5, 0.5);
    std::vector<BoxPlan> plan(1);
    const char *what = "";
    CHECK(box_plan(2, dims.data(), 4, stoich.data(), ndep.data(), dep.data(), tables.data(), BoxPlanOpts(), plan[0], &what) == 0);
    const BoxDev &P = plan[0].g.dev;
    const BoxDev B = toggle_like();
    const int off[4] = {2, 9, 14, 21};                       // tables of 7, 5, 7 and 5 doubles behind the head
    CHECK(plan[0].g.fast && P.ns == B.ns && P.nr == B.nr && P.pad == B.pad && P.dims[0] == B.dims[0] && P.dims[1] == B.dims[1]);
    for (int p = 0; p < 4; ++p) {
        CHECK(P.delta[p] == B.delta[p] && P.dorder[p] == p && P.ndep[p] == B.ndep[p] && P.nmov[p] == B.nmov[p]);
        CHECK(P.dep_s[p][0] == B.dep_s[p][0] && P.dep_off[p][0] == off[p] && P.mov_s[p][0] == B.mov_s[p][0] && P.mov_nu[p][0] == B.mov_nu[p][0]);
    }
    std::vector<BoxAdjDev> out(1);
    CHECK(box_adj_build(P, out[0]) && out[0].bias8 == 8 * 7);
}

int main()
{
    planned_is_the_hand_written_one();
    {
        const BoxDev B = toggle_like();
        std::vector<BoxAdjDev> out(1);                       // on the heap: an overrun is the sanitizer's to find
        CHECK(box_adj_build(B, out[0]));
        const BoxAdjDev &A = out[0];
        CHECK(A.bias8 == 8 * 7);
        CHECK(A.aoff8[0][0] == 8 * 2 && A.tdelta8[0][0] == 8 * 7 && A.need[0][0] == 1u << (5 * 1 + 1 + 2));
        CHECK(A.aoff8[0][1] == 8 * 22 && A.tdelta8[0][1] == -8 * 1 && A.need[0][1] == 1u << (5 * 0 - 1 + 2));
        CHECK(A.aoff8[1][0] == 8 * 12 && A.tdelta8[1][0] == 8 * 1 && A.need[1][0] == 1u << (5 * 0 + 1 + 2));
        CHECK(A.aoff8[1][1] == 8 * 32 && A.tdelta8[1][1] == -8 * 7 && A.need[1][1] == 1u << (5 * 1 - 1 + 2));
        for (int s = 0; s < kBoxFastS; ++s)
            for (int j = 0; j < kBoxFastPer; ++j)
                if (s >= 2 || j >= 2) CHECK(A.need[s][j] == kBoxAdjNever);
    }
    {
        BoxAdjDev A;
        BoxDev B = toggle_like();
        B.pad = 0;                                           // no single-factor form was stored
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.ndep[2] = 2;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.dep_s[1][0] = 0;                                   // three slots on species 0, two per species
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.mov_nu[0][0] = 3;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.mov_s[3][0] = 7;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.dep_s[0][0] = -1;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.nr = kBoxMaxR + 1;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.nmov[1] = kBoxMaxDep + 1;
        CHECK(!box_adj_build(B, A));
        B = toggle_like();
        B.pad = 6 * 16 + 4;                                  // the widest instantiation takes the same box
        CHECK(box_adj_build(B, A));
    }
    CHECK(ell_adj_resident(231, 231, 4, 4, 924, 924, 231));
    CHECK(ell_adj_resident(231, 231, 8, 4, 2000, 1848, 231));
    CHECK(!ell_adj_resident(231, 0, 4, 4, 924, 924, 231));       // nothing resident (CSR upload)
    CHECK(!ell_adj_resident(231, 230, 4, 4, 924, 924, 231));     // another generator's
    CHECK(!ell_adj_resident(231, 231, 4, 4, 923, 924, 231));
    CHECK(!ell_adj_resident(231, 231, 4, 4, 924, 923, 231));
    CHECK(!ell_adj_resident(231, 231, 4, 4, 924, 924, 230));
    CHECK(!ell_adj_resident(231, 231, 3, 4, 924, 924, 231));     // leading dimension below the slot count
    CHECK(!ell_adj_resident(231, 231, 4, 0, 924, 924, 231));
    CHECK(!ell_adj_resident(0, 0, 4, 4, 924, 924, 231));
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
