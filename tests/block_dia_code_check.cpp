// Stand-alone check of the host side of option block_dia_code: the selection rule (block_dia_code_path, kfsp_host.h) over all
// flag combinations, dispatch_diac (kfsp_block_dev.h) for the four (bits per code, bytes per record) forms and for values
// outside them, and the record decode the kernel compiles (diac_word / diac_shift / diac_mask / diac_code) against records
// packed by hand, code d in bits [W d, W d + W) of the little-endian record.  Built by tests/test_block_dia_code_host.py with
// -fsanitize=address,undefined; prints "ok".
#include "kfsp_block_dev.h"
#include "kfsp_host.h"

#include <cstdio>
#include <cstring>
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

typedef int (*Fn)();
template <int W, int REC>
static int inst() { return 100 * W + REC; }

// the instantiation dispatch_diac reaches, as the pointer the launch would take; null: none
static Fn fn_seen(int w, int rec)
{
    return dispatch_diac(w, rec, [](auto W, auto REC) -> Fn {
        static_assert(std::is_same<decltype(W), std::integral_constant<int, decltype(W)::value>>::value, "a constant, not a value");
        return inst<decltype(W)::value, decltype(REC)::value>;
    });
}

// a record as build_dia_code's k_dia_encode writes it, byte by byte: code d is the W / 8 bytes at byte d W / 8, little endian
static void pack(int w, int nd, const unsigned *codes, unsigned long long (&rec)[2])
{
    unsigned char bytes[16] = {0};
    for (int d = 0; d < nd; ++d)
        for (int b = 0; b < w / 8; ++b) bytes[d * (w / 8) + b] = (unsigned char)(codes[d] >> (8 * b));
    std::memcpy(rec, bytes, 16);          // (the device and this host are little endian)
}

int main()
{
    // ---- the selection rule: coded image active, option on, not adjoint, not small - and nothing else
    int taken = 0;
    for (int coded = 0; coded < 2; ++coded)
        for (int64_t opt : {(int64_t)0, (int64_t)1})
            for (int adj = 0; adj < 2; ++adj)
                for (int small = 0; small < 2; ++small) {
                    const bool want = coded == 1 && opt == 1 && adj == 0 && small == 0;
                    CHECK(block_dia_code_path(coded != 0, opt, adj != 0, small != 0) == want);
                    taken += block_dia_code_path(coded != 0, opt, adj != 0, small != 0) ? 1 : 0;
                }
    CHECK(taken == 1);

    // ---- the context's part of it: dia_code_on is the rule of the single-vector product
    {
        kfsp_ctx *c = new kfsp_ctx();
        CHECK(c->opt_block_dia_code == 0);                   // opt-in
        CHECK(!dia_code_on(c));
        c->use_dia = true;
        c->dia_coded = true;
        CHECK(dia_code_on(c));
        c->dia_masked = true;
        CHECK(!dia_code_on(c));
        c->dia_masked = false;
        c->use_comm = true;
        CHECK(!dia_code_on(c));
        c->use_comm = false;
        c->box.on = true;
        CHECK(!dia_code_on(c));
        c->box.on = false;
        c->dia_coded = false;
        CHECK(!dia_code_on(c));
        c->dia_coded = true;
        c->use_dia = false;
        CHECK(!dia_code_on(c));
        // the kernel's descriptor is the context's, field by field
        c->dia_code_w = 16;
        c->dia_code_rec = 8;
        for (int d = 0; d <= kMaxDiag; ++d) c->dia_doff[d] = 7 * d;
        DiaCodeDev C;
        dia_code_args(c, C);
        CHECK(C.w == 16 && C.rec_bytes == 8 && C.rec == c->d_dcode.p && C.dict == c->d_ddict.p);
        for (int d = 0; d <= kMaxDiag; ++d) CHECK(C.doff[d] == 7 * d);
        delete c;
    }

    // ---- dispatch_diac: the four forms, and NO instantiation for anything else
    for (int w : {8, 16})
        for (int rec : {8, 16}) {
            const Fn f = fn_seen(w, rec);
            CHECK(f != nullptr);
            if (f) CHECK(f() == 100 * w + rec);
        }
    for (int w : {-8, 0, 1, 4, 7, 9, 12, 15, 17, 24, 32, 64})
        for (int rec : {-1, 0, 4, 8, 12, 16, 24, 32}) CHECK(fn_seen(w, rec) == nullptr);
    for (int w : {8, 16})
        for (int rec : {-16, -8, 0, 1, 4, 7, 9, 12, 15, 17, 24, 32, 64}) CHECK(fn_seen(w, rec) == nullptr);
    CHECK(dispatch_diac(8, 8, [](auto W, auto REC) { return (int)decltype(W)::value + (int)decltype(REC)::value; }) == 16);
    CHECK(dispatch_diac(5, 8, [](auto W, auto REC) { return (int)decltype(W)::value + (int)decltype(REC)::value; }) == 0);

    // ---- the record decode, d = 0 .. 15
    static_assert(diac_mask(8) == 0xFFu && diac_mask(16) == 0xFFFFu, "one code");
    for (int d = 0; d < 16; ++d) {
        CHECK(diac_word(8, d) == d / 8 && diac_shift(8, d) == 8 * (d % 8));
        CHECK(diac_word(16, d) == d / 4 && diac_shift(16, d) == 16 * (d % 4));
        CHECK(diac_shift(8, d) + 8 <= 64 && diac_shift(16, d) + 16 <= 64);
    }
    for (int w : {8, 16}) {
        const int most = 128 / w;                            // codes a 16-byte record holds: 16 of one byte, 8 of two
        for (int nd = 1; nd <= most; ++nd) {
            unsigned codes[16];
            unsigned long long rec[2];
            // codes that differ in every byte, extremes included: a wrong shift or a mask that is too wide shows
            for (int d = 0; d < nd; ++d) codes[d] = (0x9E37u * (unsigned)(d + 1) + 0x51u * (unsigned)nd) & diac_mask(w);
            codes[0] = diac_mask(w);
            if (nd > 1) codes[nd - 1] = 0u;
            pack(w, nd, codes, rec);
            for (int d = 0; d < nd; ++d) {
                CHECK(diac_word(w, d) < 2);
                CHECK(diac_code(w, rec[diac_word(w, d)], d) == codes[d]);
            }
            // an 8-byte record is the first word alone
            if (nd * w <= 64) CHECK(rec[1] == 0ull);
        }
    }
    // all ones round a zero code, and a lone code among zeros
    for (int w : {8, 16})
        for (int d = 0; d < 128 / w; ++d) {
            unsigned codes[16];
            unsigned long long rec[2];
            for (int e = 0; e < 16; ++e) codes[e] = e == d ? 0u : diac_mask(w);
            pack(w, 128 / w, codes, rec);
            CHECK(diac_code(w, rec[diac_word(w, d)], d) == 0u);
            for (int e = 0; e < 16; ++e) codes[e] = e == d ? diac_mask(w) : 0u;
            pack(w, 128 / w, codes, rec);
            for (int e = 0; e < 128 / w; ++e) CHECK(diac_code(w, rec[diac_word(w, e)], e) == (e == d ? diac_mask(w) : 0u));
        }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
