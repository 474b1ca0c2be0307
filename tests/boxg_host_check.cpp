// Stand-alone check of the host-side helper of the generic matrix-free block product (kfsp_block_dev.h):
// box_generic_image - and that box_plan (kfsp_box_plan.h) yields, field by field, the descriptor written by hand below.
// Built by tests/test_block_boxg_host.py with -fsanitize=address,undefined; prints "ok".
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

// a box of dims (7, 5, 3) as box_plan describes it for kfsp_set_matrix_box, by ascending source offset:
//   p = 0: the conversion x0 -> x1 (delta 1 - 7 = -6) at f(x0) g(x1); p = 1: a birth of species 0 (delta -1) at three factors;
//   p = 2: a death of species 2 (delta 35).  The caller listed the birth first: dorder = (1, 0, 2), and its tables come
//   first behind the head of 2 doubles - 7 + 5 + 3, then the conversion's 7 + 5, then the death's 3: 32 doubles in all
static BoxDev three_species()
{
    BoxDev B;
    std::memset(&B, 0, sizeof(B));
    B.ns = 3;
    B.nr = 3;
    B.dims[0] = 7;
    B.dims[1] = 5;
    B.dims[2] = 3;
    B.ntab = 2 + 30 + 2 * (7 + 5 + 3);                   // a single-factor form's species tables may follow: not read
    B.delta[0] = -6;
    B.delta[1] = -1;
    B.delta[2] = 35;
    B.dorder[0] = 1;
    B.dorder[1] = 0;
    B.dorder[2] = 2;
    // p = 0: x0 -> x1, two factors
    B.ndep[0] = 2;
    B.dep_s[0][0] = 0; B.dep_off[0][0] = 17; B.dep_nu[0][0] = -1;
    B.dep_s[0][1] = 1; B.dep_off[0][1] = 24; B.dep_nu[0][1] = 1;
    B.nmov[0] = 2;
    B.mov_s[0][0] = 0; B.mov_nu[0][0] = -1; B.mov_dim[0][0] = 7;
    B.mov_s[0][1] = 1; B.mov_nu[0][1] = 1; B.mov_dim[0][1] = 5;
    // p = 1: birth of species 0, three factors
    B.ndep[1] = 3;
    B.dep_s[1][0] = 0; B.dep_off[1][0] = 2; B.dep_nu[1][0] = 1;
    B.dep_s[1][1] = 1; B.dep_off[1][1] = 9; B.dep_nu[1][1] = 0;
    B.dep_s[1][2] = 2; B.dep_off[1][2] = 14; B.dep_nu[1][2] = 0;
    B.nmov[1] = 1;
    B.mov_s[1][0] = 0; B.mov_nu[1][0] = 1; B.mov_dim[1][0] = 7;
    // p = 2: death of species 2
    B.ndep[2] = 1;
    B.dep_s[2][0] = 2; B.dep_off[2][0] = 29; B.dep_nu[2][0] = -1;
    B.nmov[2] = 1;
    B.mov_s[2][0] = 2; B.mov_nu[2][0] = -1; B.mov_dim[2][0] = 3;
    return B;
}

// the same model as a caller hands it over - the birth, the conversion, the death - planned: the descriptor above
static void planned_is_the_hand_written_one()
{
    const std::vector<int32_t> dims = {7, 5, 3}, stoich = {1, 0, 0, -1, 1, 0, 0, 0, -1}, ndep = {3, 2, 1}, dep = {0, 1, 2, 0, 1, 0, 2, 0, 0};
    const std::vector<double> tables(30, 1.5);
    std::vector<BoxPlan> plan(1);
    const char *what = "";
    CHECK(box_plan(3, dims.data(), 3, stoich.data(), ndep.data(), dep.data(), tables.data(), BoxPlanOpts(), plan[0], &what) == 0);
    const BoxDev &P = plan[0].g.dev;
    BoxDev B = three_species();
    B.ntab = 32;                                             // three factors: no single-factor form, the image ends behind the tables
    CHECK(P.ns == B.ns && P.nr == B.nr && P.ntab == B.ntab && P.pad == 0 && !plan[0].g.fast && plan[0].g.on && plan[0].n == 105);
    for (int s = 0; s < kBoxMaxS; ++s) CHECK(P.dims[s] == B.dims[s] && P.inv_dim[s] == (s < 3 ? 1.0 / (double)B.dims[s] : 0.0));
    for (int p = 0; p < kBoxMaxR; ++p) {
        CHECK(P.delta[p] == B.delta[p] && P.dorder[p] == B.dorder[p] && P.ndep[p] == B.ndep[p] && P.nmov[p] == B.nmov[p]);
        for (int i = 0; i < kBoxMaxDep; ++i) {
            CHECK(P.dep_s[p][i] == B.dep_s[p][i] && P.dep_nu[p][i] == B.dep_nu[p][i] && P.dep_off[p][i] == B.dep_off[p][i]);
            CHECK(P.mov_s[p][i] == B.mov_s[p][i] && P.mov_nu[p][i] == B.mov_nu[p][i] && P.mov_dim[p][i] == B.mov_dim[p][i]);
        }
    }
    CHECK(box_generic_image(P) == 32);
}

int main()
{
    planned_is_the_hand_written_one();
    std::vector<BoxDev> box(1);                              // on the heap: an overrun is the sanitizer's to find
    box[0] = three_species();
    BoxDev &B = box[0];
    CHECK(box_generic_image(B) == 32);                       // head + factor tables, not the tables behind them
    B.ntab = 32;
    CHECK(box_generic_image(B) == 32);
    B.ntab = 31;                                             // the last table would end outside the image
    CHECK(box_generic_image(B) == 0);
#define BROKEN(STMT)                 \
    B = three_species();             \
    STMT;                            \
    CHECK(box_generic_image(B) == 0)
    BROKEN(B.ns = 0);
    BROKEN(B.ns = kBoxMaxS + 1);
    BROKEN(B.nr = 0);
    BROKEN(B.nr = kBoxMaxR + 1);
    BROKEN(B.dims[1] = 0);
    BROKEN(B.ndep[0] = 0);
    BROKEN(B.ndep[1] = kBoxMaxDep + 1);
    BROKEN(B.nmov[2] = kBoxMaxDep + 1);
    BROKEN(B.nmov[2] = -1);
    BROKEN(B.dorder[1] = 1);                                 // no permutation
    BROKEN(B.dorder[2] = 3);
    BROKEN(B.dorder[0] = -1);
    BROKEN(B.dep_s[1][2] = 3);
    BROKEN(B.dep_s[0][0] = -1);
    BROKEN(B.dep_off[1][0] = 1);                             // inside the head
    BROKEN(B.dep_off[2][0] = 2000000000);
    BROKEN(B.mov_s[0][1] = 3);
    BROKEN(B.mov_dim[0][1] = 7);                             // not the species' dimension
    BROKEN(B.mov_nu[1][0] = 0);
    BROKEN(B.dep_nu[1][0] = 2);                              // the factor list and the move list disagree
    BROKEN(B.dep_nu[1][1] = 1);                              // a factor species that does not move
#undef BROKEN
    B = three_species();
    B.ns = kBoxMaxS;                                         // the widest descriptor: 8 species, 16 reactions, 3 factors each
    B.nr = kBoxMaxR;
    for (int s = 0; s < kBoxMaxS; ++s) B.dims[s] = 4;
    B.ntab = 2 + kBoxMaxR * kBoxMaxDep * 4;
    for (int p = 0; p < kBoxMaxR; ++p) {
        B.dorder[p] = kBoxMaxR - 1 - p;
        B.ndep[p] = kBoxMaxDep;
        B.nmov[p] = kBoxMaxDep;
        for (int i = 0; i < kBoxMaxDep; ++i) {
            B.dep_s[p][i] = B.mov_s[p][i] = (int8_t)((p + i) % kBoxMaxS);
            B.dep_nu[p][i] = B.mov_nu[p][i] = (int8_t)(i == 1 ? -100 : 100);
            B.mov_dim[p][i] = 4;
            B.dep_off[p][i] = 2 + (p * kBoxMaxDep + i) * 4;
        }
    }
    CHECK(box_generic_image(B) == B.ntab);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
