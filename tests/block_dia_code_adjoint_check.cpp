// Stand-alone check of the host side of option block_dia_code_adjoint: the selection rule (block_dia_code_t_path,
// kfsp_host.h) over all flag combinations - and block_dia_code_path as it was - and the index helper the transposed coded
// kernel compiles (diac_t_src, kfsp_block_dev.h) against records packed by hand: which 64-bit word of which row's record
// entry d of row r of A^T reads, and the ok test.  The arrays have exactly the size the kernel may read - n records, n
// rows of X - so that an index outside them is AddressSanitizer's to report.  Built by
// tests/test_block_dia_code_adjoint_host.py with -fsanitize=address,undefined; prints "ok".
#include "kfsp_block_dev.h"
#include "kfsp_host.h"

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

// a record as build_dia_code's k_dia_encode writes it, byte by byte: code d is the W / 8 bytes at byte d W / 8, little
// endian (pack of tests/block_dia_code_check.cpp)
static void pack(int w, int nd, const unsigned *codes, unsigned long long (&rec)[2])
{
    unsigned char bytes[16] = {0};
    for (int d = 0; d < nd; ++d)
        for (int b = 0; b < w / 8; ++b) bytes[d * (w / 8) + b] = (unsigned char)(codes[d] >> (8 * b));
    std::memcpy(rec, bytes, 16);          // (the device and this host are little endian)
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// A banded generator of n = 11 rows made by hand: three diagonals at delta = -4, -1, +2 that carry values, in front of
// them as many further diagonals (deltas beyond the three) as the form needs for a code in the second word of a 16-byte
// record.  val[d * ld + r] is A(r, r + delta_d), 0.0 where r + delta_d leaves [0, n); each diagonal has a dictionary of
// its distinct values and every row a record of its codes.
static void walk(int w, int rec_bytes, int nd)
{
    const int64_t n = 11, ld = n;                        // no padding row: anything past row n - 1 is out of bounds
    CHECK(nd >= 3 && nd * w <= rec_bytes * 8);
    std::vector<int64_t> delta(nd);
    for (int d = 0; d < nd - 3; ++d) delta[d] = 3 + d;   // +3, +4, ... (up to +10: one source row)
    delta[nd - 3] = -4;
    delta[nd - 2] = -1;
    delta[nd - 1] = 2;
    if (rec_bytes == 16) CHECK(diac_word(w, nd - 1) == 1);    // the last diagonals' codes sit in the second word
    std::vector<double> val((size_t)nd * ld, 0.0);
    for (int d = 0; d < nd; ++d)
        for (int64_t r = 0; r < n; ++r)
            if (r + delta[d] >= 0 && r + delta[d] < n) val[(size_t)d * ld + r] = 0.125 * (double)((r * 7 + d * 3) % 5 + 1) + (double)d;
    // dictionaries (first occurrence order, the 0.0 of rows without a target included) and codes
    std::vector<int> doff(nd + 1, 0);
    std::vector<double> dict;
    std::vector<unsigned> code((size_t)nd * n);
    for (int d = 0; d < nd; ++d) {
        doff[d] = (int)dict.size();
        for (int64_t r = 0; r < n; ++r) {
            size_t e = (size_t)doff[d];
            while (e < dict.size() && !same_bits(dict[e], val[(size_t)d * ld + r])) ++e;
            if (e == dict.size()) dict.push_back(val[(size_t)d * ld + r]);
            code[(size_t)d * n + r] = (unsigned)(e - (size_t)doff[d]);
        }
    }
    doff[nd] = (int)dict.size();
    const int words = rec_bytes / 8;
    std::vector<unsigned long long> rec((size_t)words * n);   // exactly n records
    for (int64_t r = 0; r < n; ++r) {
        unsigned codes[16] = {0};
        unsigned long long two[2];
        for (int d = 0; d < nd; ++d) codes[d] = code[(size_t)d * n + r];
        pack(w, nd, codes, two);
        for (int q = 0; q < words; ++q) rec[(size_t)words * r + q] = two[q];
        if (words == 1) CHECK(two[1] == 0ull);
    }
    std::vector<double> X((size_t)n);                         // one column of X: n rows
    for (int64_t r = 0; r < n; ++r) X[(size_t)r] = 1.0 + (double)r;
    int with = 0, without = 0;
    for (int64_t r = 0; r < n; ++r)
        for (int d = 0; d < nd; ++d) {
            const DiacTSrc q = diac_t_src(w, rec_bytes, r, delta[d], n, d);
            const int64_t src = r - delta[d];
            const bool want = 0 <= src && src < n;
            CHECK(q.ok == want);
            // whatever ok says, the word and the X row handed back are read, as the kernel reads them
            const unsigned long long word = rec[(size_t)q.word];
            const double x = X[(size_t)q.row];
            const double entry = dict[(size_t)doff[d] + diac_code(w, word, d)];
            CHECK(q.word >= 0 && q.word < (int64_t)words * n && q.row >= 0 && q.row < n);
            if (q.ok) {
                ++with;
                CHECK(q.row == src && q.word == (int64_t)words * src + diac_word(w, d));
                CHECK(same_bits(entry, val[(size_t)d * ld + src]));
                CHECK(x == 1.0 + (double)src);
            } else {
                ++without;
                CHECK(q.row == r && q.word / words == r);
            }
        }
    CHECK(with > 0 && without > 0);
    // the three diagonals with values reach sources below 0 and at or above n, in the first and in the last rows
    CHECK(!diac_t_src(w, rec_bytes, 0, 2, n, nd - 1).ok && diac_t_src(w, rec_bytes, 2, 2, n, nd - 1).ok);
    CHECK(!diac_t_src(w, rec_bytes, n - 1, -1, n, nd - 2).ok && diac_t_src(w, rec_bytes, n - 2, -1, n, nd - 2).ok);
    CHECK(!diac_t_src(w, rec_bytes, n - 4, -4, n, nd - 3).ok && diac_t_src(w, rec_bytes, n - 5, -4, n, nd - 3).ok);
}

int main()
{
    // ---- the new rule: coded image active, both options on, adjoint - and nothing else
    int taken = 0;
    for (int coded = 0; coded < 2; ++coded)
        for (int64_t opt : {(int64_t)0, (int64_t)1})
            for (int64_t opt_t : {(int64_t)0, (int64_t)1})
                for (int adj = 0; adj < 2; ++adj) {
                    const bool want = coded == 1 && opt == 1 && opt_t == 1 && adj == 1;
                    CHECK(block_dia_code_t_path(coded != 0, opt, opt_t, adj != 0) == want);
                    taken += block_dia_code_t_path(coded != 0, opt, opt_t, adj != 0) ? 1 : 0;
                }
    CHECK(taken == 1);
    CHECK(block_dia_code_t_path(true, 7, -1, true));         // (the options are stored as value != 0; any non-zero counts)
    // ---- the forward rule is what it was
    taken = 0;
    for (int coded = 0; coded < 2; ++coded)
        for (int64_t opt : {(int64_t)0, (int64_t)1})
            for (int adj = 0; adj < 2; ++adj)
                for (int small = 0; small < 2; ++small) {
                    const bool want = coded == 1 && opt == 1 && adj == 0 && small == 0;
                    CHECK(block_dia_code_path(coded != 0, opt, adj != 0, small != 0) == want);
                    taken += block_dia_code_path(coded != 0, opt, adj != 0, small != 0) ? 1 : 0;
                }
    CHECK(taken == 1);
    {
        kfsp_ctx *c = new kfsp_ctx();
        CHECK(c->opt_block_dia_code_adjoint == 0);           // opt-in
        delete c;
    }
    static_assert(kStagedDiacT != kStagedDiac && kStagedDiacT < kStagedFamilies, "a family of its own in the occupancy cache");
    static_assert(sizeof(kfsp_ctx::blk_staged_occ) / sizeof(kfsp_ctx::blk_staged_occ[0]) == kStagedFamilies, "one slot per family");
    static_assert(diac_t_src(8, 8, 5, 2, 11, 0).ok && diac_t_src(8, 8, 5, 2, 11, 0).row == 3, "constexpr: the kernel's lines");

    // ---- the index helper in the four (bits per code, bytes per record) forms
    walk(8, 8, 3);
    walk(8, 16, 11);         // codes 8 - 10 in the second word
    walk(16, 8, 3);
    walk(16, 16, 6);         // codes 4 - 5 in the second word
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
