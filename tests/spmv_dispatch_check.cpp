// Stand-alone check of what chooses the single-vector product's kernel on the host: dispatch_mode and
// dispatch_box_walk_inst (kfsp_dispatch.h) against the `if` chains and switches they replaced, and dia_code_kernel
// (kfsp_dia_diag.h) against LITERAL restatements of the two places that used to hold its rule - the if-chain of
// launch_coded and the two expressions of kfsp_dia_code_info - as they stood before the rule was one function: an edit of
// the rule shows here.  Built by tests/test_spmv_dispatch.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_dispatch.h"
#include "kfsp_internal.h"

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

static int mode_seen(int mode)
{
    return dispatch_mode(mode, [](auto M) {
        static_assert(std::is_same<decltype(M), std::integral_constant<int, decltype(M)::value>>::value, "a constant, not a value");
        return (int)decltype(M)::value;
    });
}

// the instantiation a launch took: k_spmv<MODE, NT, fmt, w, rec, lanes, inner> with `lds` bytes of dynamic LDS
struct Launched {
    int fmt, w, rec;
    bool lanes;
    int inner;
    size_t lds;
};

// launch_coded as it stood (a.G.nk, a.C.rec_bytes, a.C.doff[a.D.nd], a.G.ntab, a.D.nd, a.C.w spelled as plain arguments;
// launch_inner_mode<NT, W, ND> launched k_spmv<., NT, 10, W, 8, false, ND>, launch_coded_mode<NT, W, REC, FMT = 9,
// LANES = false> launched k_spmv<., NT, FMT, W, REC, LANES>)
static Launched launch_coded_before(int nd, int w, int rec_bytes, int nk, int ntab, int doff_nd, bool lanes, bool inner)
{
    if (nk > 0 && rec_bytes == 8) {
        const size_t lds = (size_t)(doff_nd + ntab) * sizeof(double);
        const int nd_inner = inner && !lanes ? dia_inner_count(nd, nk, w) : 0;
        if (nd_inner == 6) {
            return Launched{10, 8, 8, false, 6, lds};
        } else if (nd_inner == 4) {
            return Launched{10, 8, 8, false, 4, lds};
        } else if (lanes) {
            if (w == 8) return Launched{10, 8, 8, true, 0, lds};
            else return Launched{10, 16, 8, true, 0, lds};
        } else {
            if (w == 8) return Launched{10, 8, 8, false, 0, lds};
            else return Launched{10, 16, 8, false, 0, lds};
        }
    }
    const size_t lds = (size_t)doff_nd * sizeof(double);
    if (w == 8) {
        if (rec_bytes == 8) return Launched{9, 8, 8, false, 0, lds};
        else return Launched{9, 8, 16, false, 0, lds};
    } else {
        if (rec_bytes == 8) return Launched{9, 16, 8, false, 0, lds};
        else return Launched{9, 16, 16, false, 0, lds};
    }
}

int main()
{
    // ---- dispatch_mode: 0, 1, 2 are themselves, anything else the `else` branch of the chains: 3
    for (int m : {0, 1, 2, 3}) CHECK(mode_seen(m) == m);
    for (int m : {-1, 4, 5, 1 << 20, -(1 << 20)}) CHECK(mode_seen(m) == 3);
    int hit = -1;
    dispatch_mode(2, [&](auto M) { hit = decltype(M)::value; });       // a void callable goes through as well
    CHECK(hit == 2);
    // nested with dispatch_bool, as the launchers use them
    for (int m : {0, 1, 2, 3, 7})
        for (bool on : {false, true})
            CHECK(dispatch_mode(m, [&](auto M) { return dispatch_bool(on, [](auto B) { return 10 * (int)decltype(M)::value + (decltype(B)::value ? 1 : 0); }); }) ==
                  10 * (m > 2 ? 3 : m) + (on ? 1 : 0));

    // ---- the box instantiations of the pencil and slab kernels: there is no <2, 2>, and 2 * 16 + 2 took the `default:`
    auto walk_seen = [](int inst) { return dispatch_box_walk_inst(inst, [](auto NS, auto PER) { return 16 * (int)decltype(NS)::value + (int)decltype(PER)::value; }); };
    for (int inst : {3 * 16 + 2, 6 * 16 + 2, 6 * 16 + 4}) CHECK(walk_seen(inst) == inst);
    for (int inst : {2 * 16 + 2, 0, 1 * 16 + 2, 2 * 16 + 4, 4 * 16 + 2, 6 * 16 + 3, 8 * 16 + 2, -1}) CHECK(walk_seen(inst) == 6 * 16 + 4);

    // ---- dia_code_kernel
    long cases = 0;
    for (int nd = 1; nd <= kMaxDiag; ++nd)
        for (int w : {8, 16, 12})
            for (int rec : {8, 16})
                for (int nk : {0, 2, 3})
                    for (bool opt_lanes : {false, true})
                        for (bool opt_inner : {false, true}) {
                            const int ntab = nk ? 37 + nd : 0, doff_nd = 5 * nd + 1;
                            const DiaCodeKernel k = dia_code_kernel(nd, w, rec, nk, ntab, doff_nd, opt_lanes, opt_inner);
                            const Launched l = launch_coded_before(nd, w, rec, nk, ntab, doff_nd, opt_lanes, opt_inner);
                            CHECK(k.fmt == l.fmt && k.w == l.w && k.rec == l.rec && k.lanes == l.lanes && k.inner == l.inner);
                            CHECK((size_t)k.lds_bytes == l.lds);
                            ++cases;
                            // kfsp_dia_code_info as it stood: v[6] = dia_code_on, v[7] = have && nk > 0 ? ntab * 8 : 0 (dia_code_on
                            // implies have), then v[24] and v[25].  It never looked at the record size: a fold is built on 8-byte
                            // records only (dia_diag_plan), so a state with nk > 0 and 16-byte records does not occur.
                            if (nk > 0 && rec != 8) continue;
                            for (bool on : {false, true}) {
                                const long v6 = on ? 1 : 0;
                                const long v7 = on && nk > 0 ? (long)ntab * 8 : 0;
                                const long v24 = v6 && v7 ? (opt_lanes ? 2 : 1) : 0;
                                const long v25 = v24 == 1 && opt_inner && dia_inner_count(nd, nk, w) != 0 ? 1 : 0;
                                const DiaCodeKernel r = on ? k : DiaCodeKernel{};
                                CHECK(r.info_neighbours() == v24);
                                CHECK(r.info_inner() == v25);
                            }
                        }
    CHECK(cases == 16 * 3 * 2 * 3 * 2 * 2);
    // the interior kernels are reached: 6 diagonals with three digits, 4 with two, 8-bit codes, option on, lanes off
    CHECK(dia_code_kernel(6, 8, 8, 3, 40, 30, false, true).inner == 6);
    CHECK(dia_code_kernel(4, 8, 8, 2, 40, 30, false, true).inner == 4);
    CHECK(dia_code_kernel(6, 8, 8, 3, 40, 30, true, true).inner == 0);
    CHECK(dia_code_kernel(6, 8, 8, 3, 40, 30, true, true).lanes);
    CHECK(dia_code_kernel(6, 8, 8, 0, 0, 30, true, true).fmt == 9 && !dia_code_kernel(6, 8, 8, 0, 0, 30, true, true).lanes);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
