// Private: DIAG of a coded banded generator folded into the spare bits of its 8-byte row records (option dia_code_diag;
// kernel format 10, kfsp_spmv_dev.h; build_dia_code, kfsp_build.hip).  DIAG is the sum of all
// propensities at the row's state and every propensity depends on one species, so DIAG is - up to rounding - a sum of
// one table entry per mixed-radix digit of the row index.  The record keeps, in bits 48-63, the signed difference
// between the 64-bit pattern of the stored DIAG and that of the predictor, read as integers: pattern(P) + residual is
// the stored pattern, bit for bit, and the 8-byte DIAG stream is not read by the product.
// Plain inline code without a context and without a HIP call: the build kernels, the product kernel and the
// stand-alone host program tests/dia_diag_fold_check.cpp call the SAME functions.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define KFSP_HD __host__ __device__
#else
#define KFSP_HD
#endif

namespace kfsp {

constexpr int kDiagFoldDigits = 3;      // at most three digits (distinct |delta|)
constexpr int kDiagFoldBit = 48;        // the residual's field: bits 48-63 of the record

// Row r = x0 + size[0] (x1 + size[1] x2): digit k has size[k] values and stride[k] rows, fastest first; the slowest
// digit's size is ceil(n / stride).  nk = 0: no fold.
struct DiaDiagDev {
    int32_t nk;
    int32_t size[kDiagFoldDigits];
    int32_t stride[kDiagFoldDigits];
    int32_t toff[kDiagFoldDigits];      // table of digit k starts at toff[k] of the tables (toff[0] = 0)
    uint32_t magic[2];                  // q / size[k] = mul_hi(q, magic[k]) >> shift[k] for q < 2^31 (dia_diag_div)
    int32_t shift[2];
    int32_t ntab;                       // entries of all tables: sum of size[]
    int32_t base;                       // where the tables start in the kernel's LDS image, in doubles (behind the dictionaries)
};

// Exact q / d for q < 2^31 and d >= 2 (Granlund & Montgomery): l = ceil(log2 d), magic = floor(2^(31 + l) / d) + 1 < 2^32,
// q / d = (q * magic) >> (31 + l).
inline void dia_diag_magic(uint32_t d, uint32_t *magic, int32_t *shift)
{
    int l = 0;
    while (((uint64_t)1 << l) < d) ++l;
    *magic = (uint32_t)((((uint64_t)1 << (31 + l)) / d) + 1);
    *shift = l - 1;
}
KFSP_HD inline uint32_t dia_diag_div(uint32_t q, uint32_t magic, int shift)
{
    return (uint32_t)(((uint64_t)q * magic) >> 32) >> shift;
}

// The plan: from the stored diagonals' offsets, the number of rows, the code width, the record size and the LDS bytes
// left beside the dictionaries.  The distinct |delta| ascending are the strides; accepted only when the first is 1,
// every stride is a multiple (>= 2 x) of the one before, there are at most 3, n < 2^31, the record is 8 bytes with
// bits 48-63 free (nd w <= 48) and the tables (8 B per digit value) fit the LDS left.  Anything else: false, *G zeroed.
inline bool dia_diag_plan(int nd, const int32_t *delta, int64_t n, int w, int rec_bytes, int64_t lds_left, DiaDiagDev *G)
{
    *G = DiaDiagDev{};
    if (nd < 1 || nd > 16 || !delta || n < 1 || n >= ((int64_t)1 << 31)) return false;
    if (rec_bytes != 8 || w < 1 || nd * w > kDiagFoldBit) return false;
    int64_t s[kDiagFoldDigits + 1];
    int nk = 0;
    for (int d = 0; d < nd; ++d) {                       // distinct |delta|, ascending (insertion)
        const int64_t a = delta[d] < 0 ? -(int64_t)delta[d] : (int64_t)delta[d];
        int at = 0;
        while (at < nk && s[at] < a) ++at;
        if (at < nk && s[at] == a) continue;
        if (nk == kDiagFoldDigits) return false;
        for (int i = nk; i > at; --i) s[i] = s[i - 1];
        s[at] = a;
        ++nk;
    }
    if (s[0] != 1) return false;
    for (int k = 0; k + 1 < nk; ++k)
        if (s[k + 1] % s[k] != 0 || s[k + 1] / s[k] < 2) return false;
    if (s[nk - 1] >= n) return false;                    // (a diagonal that long has no entry)
    int64_t total = 0;
    DiaDiagDev P{};
    P.nk = nk;
    for (int k = 0; k < nk; ++k) {
        const int64_t size = k + 1 < nk ? s[k + 1] / s[k] : (n + s[k] - 1) / s[k];
        P.size[k] = (int32_t)size;
        P.stride[k] = (int32_t)s[k];
        P.toff[k] = (int32_t)total;
        total += size;
        if (total * 8 > lds_left) return false;
        if (k + 1 < nk) dia_diag_magic((uint32_t)size, &P.magic[k], &P.shift[k]);
    }
    P.ntab = (int32_t)total;
    *G = P;
    return true;
}

// the digits of row g (< 2^31) ...
KFSP_HD inline void dia_diag_digits(const DiaDiagDev &G, uint32_t g, int &x0, int &x1, int &x2)
{
    x0 = (int)g;
    x1 = x2 = 0;
    if (G.nk >= 2) {
        const uint32_t t = dia_diag_div(g, G.magic[0], G.shift[0]);
        x0 = (int)(g - t * (uint32_t)G.size[0]);
        x1 = (int)t;
        if (G.nk == 3) {
            const uint32_t u = dia_diag_div(t, G.magic[1], G.shift[1]);
            x1 = (int)(t - u * (uint32_t)G.size[1]);
            x2 = (int)u;
        }
    }
}
// ... and of the row behind it: + 1 with carry (the slowest digit never wraps)
KFSP_HD inline void dia_diag_next(const DiaDiagDev &G, int &x0, int &x1, int &x2)
{
    ++x0;
    if (G.nk >= 2 && x0 >= G.size[0]) {
        x0 = 0;
        ++x1;
        if (G.nk == 3 && x1 >= G.size[1]) {
            x1 = 0;
            ++x2;
        }
    }
}

// A table entry from DIAG along one axis: the slowest digit carries the value itself, the others their difference to row 0.
KFSP_HD inline double dia_diag_entry(bool slowest, double on_axis, double at_row0) { return slowest ? on_axis : on_axis - at_row0; }

// The predictor: the slowest digit first, additions only.  t: the tables.  The slowest digit is clamped to its table
// (rows of the padding beyond n have no entry; their value is not the predictor's, see dia_diag_value).
KFSP_HD inline double dia_diag_predict(const DiaDiagDev &G, const double *t, int x0, int x1, int x2)
{
    if (G.nk == 3) {
        x2 = x2 < G.size[2] ? x2 : G.size[2] - 1;
        return (t[G.toff[2] + x2] + t[G.toff[1] + x1]) + t[x0];
    }
    if (G.nk == 2) {
        x1 = x1 < G.size[1] ? x1 : G.size[1] - 1;
        return t[G.toff[1] + x1] + t[x0];
    }
    x0 = x0 < G.size[0] ? x0 : G.size[0] - 1;
    return t[x0];
}

KFSP_HD inline uint64_t dia_diag_bits(double v)
{
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return b;
}
KFSP_HD inline double dia_diag_from_bits(uint64_t b)
{
    double v;
    __builtin_memcpy(&v, &b, 8);
    return v;
}

// Decode: pattern(P) + the sign-extended bits 48-63 of the record; rows of the padding (in_range false) hold +0.0.
KFSP_HD inline double dia_diag_value(double p, uint64_t rec, bool in_range)
{
    const uint64_t b = dia_diag_bits(p) + (uint64_t)((int64_t)rec >> kDiagFoldBit);
    return in_range ? dia_diag_from_bits(b) : 0.0;
}

// Encode row r of the ld rows the product computes: *field receives the residual, placed at bits 48-63.  False - the
// fold is refused - when the residual does not fit a signed 16-bit field, when the decode does not give the stored
// pattern back, or when a row of the padding (r >= n) holds anything but +0.0.
KFSP_HD inline bool dia_diag_encode(const DiaDiagDev &G, const double *t, int64_t r, int64_t n, double stored, uint64_t *field)
{
    *field = 0;
    if (r >= n) return dia_diag_bits(stored) == 0;
    int x0, x1, x2;
    dia_diag_digits(G, (uint32_t)r, x0, x1, x2);
    const double p = dia_diag_predict(G, t, x0, x1, x2);
    const int64_t resid = (int64_t)(dia_diag_bits(stored) - dia_diag_bits(p));
    if (resid < -32768 || resid > 32767) return false;
    *field = (uint64_t)resid << kDiagFoldBit;
    return dia_diag_bits(dia_diag_value(p, *field, true)) == dia_diag_bits(stored);
}

// ---- the +-1 neighbours of x from the neighbour lanes instead of from memory (option dia_code_lanes; the folded kernel only) ----
// The banded kernel reads x[p], x[p + 1] as one 16-byte pair (ld_xpair, kfsp_spmv_dev.h) with p clamped to [-1, last]:
// the word in front of x and the one behind row `last` are guard words every device buffer carries.
KFSP_HD inline int64_t dia_xpair_clamp(int64_t p, int64_t last) { return p < -1 ? -1 : (p > last ? last : p); }

// A trip is the 128-row group from global row g0; lane l owns rows g0 + 2 l and g0 + 2 l + 1 and holds their pair
// xd = (x[g0 + 2 l], x[g0 + 2 l + 1]).  The pair of the -1 diagonal, (x[g0 + 2 l - 1], x[g0 + 2 l]), is (lane l - 1's xd.y,
// xd.x) and that of the +1 diagonal, (x[g0 + 2 l + 1], x[g0 + 2 l + 2]), is (xd.y, lane l + 1's xd.x); only lane 0's first
// and lane 63's second word are held by no lane (dia_lanes_edge).  The trip may take them from the lanes when the clamp
// acts on none of the three pairs of any lane: their indices p run over g0 - 1 ... g0 + 127, so g0 >= 0 and
// g0 + 127 <= last = n - 1.  Every trip passes but the one that holds row `last` in front of rows of the padding: at most
// one trip of a generator, none when n is a multiple of 128 (lane 63 of the last trip then reads the guard word x[n]).
KFSP_HD inline bool dia_lanes_trip(int64_t g0, int64_t n) { return g0 >= 0 && g0 + 127 <= n - 1; }
// the x index of the word lane 0 / lane 63 of such a trip reads on its own (the other lanes read none)
KFSP_HD inline int64_t dia_lanes_edge(int64_t g0, int lane) { return lane == 0 ? g0 - 1 : g0 + 128; }

// ---- interior trips of the folded kernel (option dia_code_inner; rows_dia_inner, kfsp_spmv_dev.h) ----
// With dmin <= 0 <= dmax the smallest and the largest stored offset (0, the diagonal, included) the pair indices of a trip
// run over g0 + dmin ... g0 + 126 + dmax.  The trip is interior when the clamp of ld_xpair changes none of them
// (g0 + dmin >= -1 and g0 + 126 + dmax <= last) and no row belongs to the padding (g0 + 127 <= last): then gq == g in
// every lane, both flags of dia_diag_value are true, and a lane's x pair of diagonal delta is the 16 bytes at byte offset
// 16 l of the uniform address x + g0 + delta - no per-lane 64-bit index is needed.  (dmax >= 1 makes the second condition
// follow from the third; it is kept because a generator may store no offset above 0.)
KFSP_HD inline bool dia_inner_trip(int64_t g0, int64_t n, int64_t dmin, int64_t dmax)
{
    const int64_t last = n - 1;
    return g0 + dmin >= -1 && g0 + 127 <= last && g0 + 126 + dmax <= last;
}
// The diagonal counts the interior body is instantiated for, by the folded generator's diagonals nd, digits nk and code
// width w: 6 with three digits (three-species boxes), 4 with two (two-species), 8-bit codes; 0: no instantiation, the
// generator keeps the present kernel.
KFSP_HD inline int dia_inner_count(int nd, int nk, int w)
{
    if (w != 8) return 0;
    return nd == 6 && nk == 3 ? 6 : (nd == 4 && nk == 2 ? 4 : 0);
}
// the index of the first word of lane l's pair of diagonal delta in such a trip: uniform base g0 + delta, lane part 2 l
KFSP_HD inline int64_t dia_inner_base(int64_t g0, int64_t delta) { return g0 + delta; }

// ---- which coded banded kernel a product runs: the one rule (the launch, kfsp_spmv_diac.hip, and kfsp_dia_code_info) ----
// k_spmv's coded formats, NS = bits per code, NE = bytes per row record: 9 reads DIAG from its 8-byte stream; 10 has it
// folded into the records' spare bits (above; 8-byte records only), its tables behind the dictionaries in memory and in LDS.
// Format 10 has two variants, at most one at a time: LANES (option dia_code_lanes), the +-1 neighbours of x from the
// neighbour lanes (dia_lanes_trip), and INNER (option dia_code_inner, not under LANES), the generator's diagonal count,
// 6 or 4, where it has an instantiation (dia_inner_count): interior trips (dia_inner_trip) then run rows_dia_inner.
struct DiaCodeKernel {
    int fmt;             // 9 or 10
    int w, rec;          // the instantiation's bits per code and bytes per record: 8 or 16 each
    bool lanes;
    int inner;           // 0 (every trip runs rows_dia), 4 or 6
    int64_t lds_bytes;   // dynamic LDS: the dictionaries and, folded, the DIAG tables
    // kfsp_dia_code_info: where the folded product takes the +-1 pairs of x from (0 not folded, 1 loads, 2 lanes), and 1
    // where it runs interior trips through rows_dia_inner
    int info_neighbours() const { return fmt == 10 ? (lanes ? 2 : 1) : 0; }
    int info_inner() const { return inner != 0 ? 1 : 0; }
};
// nd diagonals with w-bit codes in records of rec_bytes; nk digits and ntab table entries of the fold (nk = 0: none);
// doff_nd entries of all dictionaries.  A fold exists on 8-byte records only (dia_diag_plan refuses any other, and
// build_dia_code stores no other DiaDiagDev), so `nk > 0` alone says as much as the test below.
inline DiaCodeKernel dia_code_kernel(int nd, int w, int rec_bytes, int nk, int ntab, int doff_nd, bool opt_lanes, bool opt_inner)
{
    DiaCodeKernel k{9, w == 8 ? 8 : 16, rec_bytes == 8 ? 8 : 16, false, 0, (int64_t)doff_nd * 8};
    if (nk > 0 && rec_bytes == 8) {
        k.fmt = 10;
        k.lds_bytes += (int64_t)ntab * 8;
        k.lanes = opt_lanes;
        k.inner = opt_inner && !opt_lanes ? dia_inner_count(nd, nk, w) : 0;   // (4 or 6 diagonals fold with 8-bit codes only)
    }
    return k;
}

}   // namespace kfsp
