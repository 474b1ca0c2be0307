// Private: k_spmv, the single-vector generator product y = (s) A x of every stored and matrix-free format, with its row
// functions.  A translation unit emits the instantiations it launches: kfsp_kernels.hip formats 0 - 5, kfsp_spmv_diac.hip
// the coded banded formats 9 and 10.
#pragma once

#include "kfsp_box_dev.h"
#include "kfsp_dev.h"

namespace kfsp {

// One lane = one row, one wavefront = one 64-row chunk.
//   SELL: slot k of a chunk is one contiguous 256-B (col) + 512-B (val) read.
//   DIA : diagonal d of a chunk is one contiguous 512-B val read; x is read as
//         the same 64 rows shifted by delta[d] (no index traffic at all).
// Work distribution is XCD-aware: workgroups b, b+8, b+16.. share an XCD (and
// its 4 MiB L2), so XCD x sweeps the contiguous chunk range [x*CPX,(x+1)*CPX)
// with its workgroups advancing as one front; the gathered x window of a front
// (rows +- the generator's strides) then stays in that XCD's L2 instead of
// being fetched by all eight.
//
// MODE 0: y = A x                           (FMATVEC seam, DROP_STATES, bench)
// MODE 1: y = s A u ; partial = udot.y      (Arnoldi column, s = 1/||u||)
// MODE 2: y = s A u ; partial = y.y         (the AVNORM product)
// MODE 3: y = s A u ; partial = udot.y, partial2 = udot2.y   (IOP(2) column)

// One SELL row: the slots come in pairs (sell_pos), columns as one 8-byte and values as one 16-byte load
// per pair, summed slot by slot in FMATVEC's order.
template <bool NT>
__device__ __forceinline__ double row_sell(const SellDev &A, const double *__restrict__ xg, int64_t row0,
                                           int64_t c, int lane)
{
    const int64_t off = A.off[c];
    const int w = (int)((A.off[c + 1] - off) >> 6);
    const int w2 = w >> 1;                                   // slot pairs; an odd width ends in a single slot
    const int64_t r = (c << 6) + lane;
    const int32_t *cp = A.col + off + 2 * lane;
    const double *vp = A.val + off + 2 * lane;
    double sum = -ld_stream<NT>(A.diag + r) * xg[row0 + r];
    int k = 0;
    for (; k + 2 <= w2; k += 2) {
        const i2 c0 = ld_stream2<NT>(cp + (k + 0) * 128), c1 = ld_stream2<NT>(cp + (k + 1) * 128);
        const d2 v0 = ld_stream2<NT>(vp + (k + 0) * 128), v1 = ld_stream2<NT>(vp + (k + 1) * 128);
        sum += v0.x * xg[c0.x];
        sum += v0.y * xg[c0.y];
        sum += v1.x * xg[c1.x];
        sum += v1.y * xg[c1.y];
    }
    if (k < w2) {
        const i2 c0 = ld_stream2<NT>(cp + k * 128);
        const d2 v0 = ld_stream2<NT>(vp + k * 128);
        sum += v0.x * xg[c0.x];
        sum += v0.y * xg[c0.y];
    }
    if (w & 1) sum += ld_stream<NT>(A.val + off + w2 * 128 + lane) * xg[ld_stream<NT>(A.col + off + w2 * 128 + lane)];
    return sum;
}

// The same row with dictionary-coded columns (kSellCode*, kfsp_internal.h): the column of an entry is
// row + table[index], the table of the chunk's <= 64 distinct offsets sits one entry per lane in a register and
// an index is turned into its offset by ds_bpermute.  Same values, same order, same addresses as row_sell.
template <bool NT>
__device__ __forceinline__ double row_sell_coded(const SellDev &A, const double *__restrict__ xg, int64_t row0,
                                                 int64_t c, int lane)
{
    const int dtl = __builtin_amdgcn_readfirstlane(A.dtlen[c]);
    if (dtl == 0) return row_sell<NT>(A, xg, row0, c, lane);          // this chunk kept its plain columns (uniform branch)
    const int64_t off = A.off[c];
    const int w = (int)((A.off[c + 1] - off) >> 6);
    const int w2 = w >> 1;
    const int64_t r = (c << 6) + lane;
    const int tab = lane < dtl ? A.dtab[(c << 6) + lane] : 0;
    const unsigned long long *cp = A.code + A.codeoff[c] + lane;
    const double *vp = A.val + off + 2 * lane;
    const double *xr = xg + row0 + r;                                 // x of the row itself; entries are xr[offset]
    unsigned long long cw = __builtin_nontemporal_load(cp);
    int used = 0;
    double sum = -ld_stream<NT>(A.diag + r) * xr[0];
#define KFSP_NEXT_X(XV)                                                                     \
    {                                                                                       \
        if (used == kSellCodePerWord) {                                                     \
            cp += 64;                                                                       \
            cw = __builtin_nontemporal_load(cp);                                            \
            used = 0;                                                                       \
        }                                                                                   \
        const int d_ = __builtin_amdgcn_ds_bpermute((int)(cw & 63ull) << 2, tab);           \
        cw >>= kSellCodeBits;                                                               \
        ++used;                                                                             \
        XV = xr[d_];                                                                        \
    }
    int k = 0;
    for (; k + 2 <= w2; k += 2) {
        const d2 v0 = ld_stream2<NT>(vp + (k + 0) * 128), v1 = ld_stream2<NT>(vp + (k + 1) * 128);
        double x0, x1, x2, x3;
        KFSP_NEXT_X(x0)
        KFSP_NEXT_X(x1)
        KFSP_NEXT_X(x2)
        KFSP_NEXT_X(x3)
        sum += v0.x * x0;
        sum += v0.y * x1;
        sum += v1.x * x2;
        sum += v1.y * x3;
    }
    if (k < w2) {
        const d2 v0 = ld_stream2<NT>(vp + k * 128);
        double x0, x1;
        KFSP_NEXT_X(x0)
        KFSP_NEXT_X(x1)
        sum += v0.x * x0;
        sum += v0.y * x1;
    }
    if (w & 1) {
        double x0;
        KFSP_NEXT_X(x0)
        sum += ld_stream<NT>(A.val + off + w2 * 128 + lane) * x0;
    }
#undef KFSP_NEXT_X
    return sum;
}

// Banded form, TWO consecutive rows per lane (a wavefront covers 128 rows): the
// value streams - the bulk of the traffic - are read 16 B per lane, which is
// worth ~9 % of HBM rate over 8 B per lane (profiles/r01_stream_widths.log).
// x too is read 16 B per lane and diagonal (ld_xpair: shifted by delta, so 8-B aligned in general).
// x[p], x[p + 1] as ONE 16-byte load (8-byte aligned): a CU issues vector-memory instructions at a fixed rate
// whatever their width, so two 8-byte gathers cost twice one 16-byte gather.  p is clamped to [-1, n - 1]: the
// element before x and the one behind it are the guard words / column padding every device buffer carries
// (DevBuf, vcol): finite, and only ever multiplied by a stored 0.
typedef double __attribute__((ext_vector_type(2))) xpair_t;
typedef xpair_t __attribute__((aligned(8))) xpair_u;
__device__ __forceinline__ xpair_t ld_xpair(const double *__restrict__ xg, int64_t p, int64_t last)
{
    p = dia_xpair_clamp(p, last);
    return *reinterpret_cast<const xpair_u *>(xg + p);
}

// Banded form with dictionary-coded values (format 9, DiaCodeDev in kfsp_internal.h).  The records of the lane's two rows are
// adjacent: ONE 16-byte load (REC = 8) or two (REC = 16) bring every code of both rows, whatever the number of diagonals.
// W: bits per code; a record word holds 64 / W codes, diagonal d in word d / (64 / W).
typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
template <int REC>
struct DiaCodes {
    unsigned long long a[REC / 8], b[REC / 8];          // record words of row 2 l and of row 2 l + 1
};
template <bool NT, int REC>
__device__ __forceinline__ DiaCodes<REC> ld_codes(const DiaCodeDev &C, int64_t r)
{
    DiaCodes<REC> k;
    const ull2 *p = reinterpret_cast<const ull2 *>(C.rec + r * (REC / 8));
    if (REC == 8) {
        const ull2 t = NT ? __builtin_nontemporal_load(p) : *p;
        k.a[0] = t.x;
        k.b[0] = t.y;
    } else {
        const ull2 t = NT ? __builtin_nontemporal_load(p) : *p;
        const ull2 u = NT ? __builtin_nontemporal_load(p + 1) : p[1];
        k.a[0] = t.x;
        k.a[REC / 8 - 1] = t.y;
        k.b[0] = u.x;
        k.b[REC / 8 - 1] = u.y;
    }
    return k;
}
// the stored values of diagonal d in the lane's two rows: dict[d][code], from LDS
template <int W, int REC>
__device__ __forceinline__ d2 coded_vals(const DiaCodeDev &C, const DiaCodes<REC> &k, int d)
{
    constexpr int PER = 64 / W;
    const bool hi = REC == 16 && d >= PER;               // (uniform: d is the loop counter)
    const unsigned long long wa = hi ? k.a[REC / 8 - 1] : k.a[0], wb = hi ? k.b[REC / 8 - 1] : k.b[0];
    const int sh = (d & (PER - 1)) * W;
    const unsigned ca = (unsigned)(wa >> sh) & ((1u << W) - 1u), cb = (unsigned)(wb >> sh) & ((1u << W) - 1u);
    const double *t = box_lds + C.doff[d];
    d2 v;
    v.x = t[ca];
    v.y = t[cb];
    return v;
}

// the x pair of the diagonal at offset delta: loaded, or (rows_dia, LANES) the pair xm / xp the trip took from its lanes
template <bool LANES>
__device__ __forceinline__ xpair_t dia_x(const double *__restrict__ xg, int64_t g, int delta, int64_t last, bool lanes,
                                         const xpair_t &xm, const xpair_t &xp)
{
    if (LANES && lanes) {                                // (uniform: the trip and the descriptor sit in SGPRs)
        if (delta == -1) return xm;
        if (delta == 1) return xp;
    }
    return ld_xpair(xg, g + delta, last);
}

// W > 0: the values come from the dictionaries (coded_vals) instead of from the 16-byte value streams; everything else - the
// x pairs, the clamp, the order of the multiply-adds - is the same code, so the sums are the same bits.
// FOLD (W > 0, REC = 8): DIAG is not loaded either.  Its 64-bit pattern is that of the predictor - one table entry (LDS,
// behind the dictionaries) per mixed-radix digit of the row index, added slowest digit first - plus the signed residual in
// bits 48-63 of the row's record (kfsp_dia_diag.h; build_dia_code verified every row): the stored double, bit for bit.
// LANES (with FOLD): the pairs of the -1 and +1 diagonals are not loaded where the trip allows it (dia_lanes_trip: the clamp
// of ld_xpair acts on no lane): their four words are xd's own two and the neighbour lanes' - a whole-wavefront shift by one
// lane in registers (DPP wave_shr:1 / wave_shl:1, no LDS traffic) - but for lane 0's x[g0 - 1] and lane 63's x[g0 + 128],
// which ONE 8-byte load with only those two lanes active brings.  The same doubles from the same memory: the same bits.
// A trip that dia_lanes_trip refuses keeps the loads.  (Measured slower than the loads on c3 and c3x: option dia_code_lanes
// is off by default)
template <bool NT, bool MASKED, int W = 0, int REC = 8, bool FOLD = false, bool LANES = false>
__device__ __forceinline__ d2 rows_dia(const DiaDev &D, const DiaCodeDev &C, const DiaDiagDev &G, const double *__restrict__ xg,
                                       int64_t row0, int64_t c, int lane, unsigned m)
{
    const int64_t r = (c << 7) + 2 * lane;
    const int64_t g = row0 + r;
    const int64_t last = D.n - 1;
    const double *vp = D.val + r;
    const double *zp = D.zero + 2 * lane;
    DiaCodes<REC> codes;
    if (W) codes = ld_codes<NT, REC>(C, r);
    // m: which diagonals have entries in this group (same for the whole wavefront; the
    // caller fetched it one trip ahead, so no load sits in front of the address arithmetic)
    d2 dg;
    if (FOLD) {
        // the digits of row g (< 2^31) by exact division with the uniform radices, those of row g + 1 by increment with carry
        int a0, a1, a2;
        // (rows of the padding take the digits of the last row: the division is exact below 2^31 only, and their value is +0.0)
        const uint32_t gq = (uint32_t)g < (uint32_t)last ? (uint32_t)g : (uint32_t)last;
        dia_diag_digits(G, gq, a0, a1, a2);
        int b0 = a0, b1 = a1, b2 = a2;
        dia_diag_next(G, b0, b1, b2);
        const double *t = box_lds + G.base;
        dg.x = dia_diag_value(dia_diag_predict(G, t, a0, a1, a2), codes.a[0], g <= last);
        dg.y = dia_diag_value(dia_diag_predict(G, t, b0, b1, b2), codes.b[0], g < last);
    } else {
        dg = ld_stream2<NT>(D.diag + r);
    }
    const xpair_t xd = ld_xpair(xg, g, last);
    xpair_t xm = {0.0, 0.0}, xp = {0.0, 0.0};            // the pairs of the -1 and of the +1 diagonal (read only under `lanes`)
    bool lanes = false;
    if (LANES) {
        const int64_t g0 = row0 + (c << 7);
        lanes = dia_lanes_trip(g0, D.n);
        if (lanes) {
            double edge = 0.0;
            if (lane == 0 || lane == 63) edge = xg[dia_lanes_edge(g0, lane)];
            const double below = dpp_get<0x138, 0xf, 0xf>(xd.y);    // wave_shr:1, lane l - 1's second word
            const double above = dpp_get<0x130, 0xf, 0xf>(xd.x);    // wave_shl:1, lane l + 1's first word
            xm.x = lane == 0 ? edge : below;
            xm.y = xd.x;
            xp.x = xd.y;
            xp.y = lane == 63 ? edge : above;
        }
    }
    d2 sum;
    sum.x = -dg.x * xd.x;
    sum.y = -dg.y * xd.y;
    int d = 0;
    for (; d + 2 <= D.nd; d += 2) {
        const bool on0 = !MASKED || ((m >> d) & 1u), on1 = !MASKED || ((m >> (d + 1)) & 1u);
        // an empty segment costs no HBM traffic: zeros from a cached line, x from the row itself
        const d2 v0 = W ? coded_vals<(W ? W : 8), REC>(C, codes, d + 0) : ld_stream2<NT>(on0 ? vp + (int64_t)(d + 0) * D.ld : zp);
        const d2 v1 = W ? coded_vals<(W ? W : 8), REC>(C, codes, d + 1) : ld_stream2<NT>(on1 ? vp + (int64_t)(d + 1) * D.ld : zp);
        const xpair_t x0 = dia_x<LANES>(xg, g, on0 ? D.delta[d + 0] : 0, last, lanes, xm, xp);
        const xpair_t x1 = dia_x<LANES>(xg, g, on1 ? D.delta[d + 1] : 0, last, lanes, xm, xp);
        sum.x += v0.x * x0.x;
        sum.y += v0.y * x0.y;
        sum.x += v1.x * x1.x;
        sum.y += v1.y * x1.y;
    }
    for (; d < D.nd; ++d) {
        const bool on0 = !MASKED || ((m >> d) & 1u);
        const d2 v0 = W ? coded_vals<(W ? W : 8), REC>(C, codes, d) : ld_stream2<NT>(on0 ? vp + (int64_t)d * D.ld : zp);
        const xpair_t x0 = dia_x<LANES>(xg, g, on0 ? D.delta[d] : 0, last, lanes, xm, xp);
        sum.x += v0.x * x0.x;
        sum.y += v0.y * x0.y;
    }
    return sum;
}

// 16 bytes per lane at a uniform 64-bit address plus the lane's unsigned 32-bit byte offset (global_load_dwordx4 with a scalar
// base: no per-lane 64-bit address arithmetic); 8-byte aligned in general
template <typename T, bool NT>
__device__ __forceinline__ T ld_lane16(const void *base, unsigned voff)
{
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const global_bytes_t p = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b) |
                                              (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32);
    const __attribute__((address_space(1), aligned(8))) T *q = (const __attribute__((address_space(1), aligned(8))) T *)(p + voff);
    return NT ? __builtin_nontemporal_load(q) : *q;
}

// The folded kernel's rows (W-bit codes, 8-byte records, FOLD) in an INTERIOR trip (dia_inner_trip, kfsp_dia_diag.h: the clamp
// of ld_xpair acts on no lane's pair of any diagonal and no row belongs to the padding) of a generator with ND diagonals and
// ND / 2 digits, both compile-time.  The same loads of the same words, the same table look-ups and the same order of
// additions and multiply-adds as rows_dia - the same bits - with what an interior trip does not need taken out: every
// address is a uniform 64-bit base plus the lane's 32-bit byte offset (no clamp, no per-lane 64-bit compare, select or
// add) and the diagonal loop is unrolled (delta and doff stay in SGPRs, the codes are extracted with constant shifts).
// The loads go out in TWO groups - the record, xd and the first half of the pairs, then, behind the first half's
// multiply-adds, the second half: with all of them in flight at once the kernel is SLOWER than rows_dia (c3 23.6 against
// 22.5 us, c3x 48.6 against 43.7), in two groups faster (20.8 / 38.2 us).
template <bool NT, int W, int ND>
__device__ __forceinline__ d2 rows_dia_inner(const DiaDev &D, const DiaCodeDev &C, const DiaDiagDev &G0, const double *__restrict__ xg,
                                             int64_t row0, int64_t c, int lane)
{
    constexpr int NFIRST = ND / 2;
    DiaDiagDev G = G0;
    G.nk = ND / 2;                                       // (the dispatch admits ND diagonals with ND / 2 digits only)
    const int64_t g0 = row0 + (c << 7);
    // (the empty statement keeps the offset a 32-bit register of THIS trip: hoisted out of the trip loop as a 64-bit pair it
    // would turn every load back into a per-lane 64-bit address)
    unsigned voff = 16u * (unsigned)lane;
    asm volatile("" : "+v"(voff));
    const ull2 rec = ld_lane16<ull2, NT>(C.rec + (c << 7), voff);
    DiaCodes<8> codes;
    codes.a[0] = rec.x;
    codes.b[0] = rec.y;
    const xpair_t xd = ld_lane16<xpair_t, false>(xg + g0, voff);
    xpair_t xs[ND];
#pragma unroll
    for (int d = 0; d < NFIRST; ++d) xs[d] = ld_lane16<xpair_t, false>(xg + dia_inner_base(g0, D.delta[d]), voff);
    __builtin_amdgcn_sched_barrier(0);                   // (nothing moves across: the second group stays behind the first)
    int a0, a1, a2;
    dia_diag_digits(G, (uint32_t)g0 + 2u * (unsigned)lane, a0, a1, a2);
    int b0 = a0, b1 = a1, b2 = a2;
    dia_diag_next(G, b0, b1, b2);
    const double *t = box_lds + G.base;
    d2 dg;
    dg.x = dia_diag_value(dia_diag_predict(G, t, a0, a1, a2), codes.a[0], true);
    dg.y = dia_diag_value(dia_diag_predict(G, t, b0, b1, b2), codes.b[0], true);
    d2 sum;
    sum.x = -dg.x * xd.x;
    sum.y = -dg.y * xd.y;
#pragma unroll
    for (int d = 0; d < NFIRST; ++d) {
        const d2 v = coded_vals<W, 8>(C, codes, d);
        sum.x += v.x * xs[d].x;
        sum.y += v.y * xs[d].y;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int d = NFIRST; d < ND; ++d) xs[d] = ld_lane16<xpair_t, false>(xg + dia_inner_base(g0, D.delta[d]), voff);
#pragma unroll
    for (int d = NFIRST; d < ND; ++d) {
        const d2 v = coded_vals<W, 8>(C, codes, d);
        sum.x += v.x * xs[d].x;
        sum.y += v.y * xs[d].y;
    }
    return sum;
}

// Matrix-free box generator, two consecutive rows per lane like the banded form.  The descriptor B
// is a kernel argument (uniform: scalar loads), the factor tables sit in LDS, the coordinates of a
// row in registers (NS compile-time for the benchmark models; species picked by select chains, a
// register array indexed by run-time data would spill).  NS = 0 / NR = 0: run-time sizes.
template <int NS>
__device__ __forceinline__ int box_pick(const int *x, int s)
{
    constexpr int N = NS ? NS : kBoxMaxS;
    int v = x[0];
#pragma unroll
    for (int i = 1; i < N; ++i) v = (s == i) ? x[i] : v;
    return v;
}

template <int NS, int NR>
__device__ __forceinline__ double row_box(const BoxDev &B, const double *tab, const int *x, const double *__restrict__ xg,
                                          int64_t g)
{
    constexpr int RMAX = NR ? NR : kBoxMaxR;
    const int nr = NR ? NR : B.nr;
    // a_k at x itself, reaction by reaction in sorted position
    double ax[RMAX];
#pragma unroll
    for (int k = 0; k < RMAX; ++k) {
        ax[k] = 0.0;
        if (k < nr) {
            double a = tab[B.dep_off[k][0] + box_pick<NS>(x, B.dep_s[k][0])];
#pragma unroll
            for (int i = 1; i < kBoxMaxDep; ++i)
                if (i < B.ndep[k]) a *= tab[B.dep_off[k][i] + box_pick<NS>(x, B.dep_s[k][i])];
            ax[k] = a;
        }
    }
    // DIAG = sum of all propensities at x, in the model's reaction order (StateSpace.f90:207-212)
    double dsum = 0.0;
#pragma unroll
    for (int q = 0; q < RMAX; ++q) {
        if (q < nr) {
            const int k = B.dorder[q];
            double a = ax[0];
#pragma unroll
            for (int j = 1; j < RMAX; ++j) a = (k == j) ? ax[j] : a;
            dsum += a;
        }
    }
    double sum = -dsum * xg[g];
#pragma unroll
    for (int k = 0; k < RMAX; ++k) {                    // ascending column offset, as the banded kernel
        if (k < nr) {
            bool in = true;
            bool same = true;                           // the source state has the same factors as x itself
#pragma unroll
            for (int i = 0; i < kBoxMaxDep; ++i) {
                if (i < B.nmov[k]) {
                    const int s = B.mov_s[k][i];
                    const int v = box_pick<NS>(x, s) - B.mov_nu[k][i];
                    in = in && v >= 0 && v < B.mov_dim[k][i];
                }
                if (i < B.ndep[k]) same = same && B.dep_nu[k][i] == 0;
            }
            double a = ax[k];
            if (!same) {                                // uniform branch: B is the same for every lane
                a = 0.0;
                if (in) {
                    a = tab[B.dep_off[k][0] + box_pick<NS>(x, B.dep_s[k][0]) - B.dep_nu[k][0]];
#pragma unroll
                    for (int i = 1; i < kBoxMaxDep; ++i)
                        if (i < B.ndep[k]) a *= tab[B.dep_off[k][i] + box_pick<NS>(x, B.dep_s[k][i]) - B.dep_nu[k][i]];
                }
            }
            sum += (in ? a : 0.0) * xg[in ? g + B.delta[k] : g];
        }
    }
    return sum;
}

template <int NS, int NR>
__device__ __forceinline__ d2 rows_box(const BoxDev &B, const double *tab, const double *__restrict__ xg,
                                       int64_t row0, int64_t nloc, int64_t c, int lane)
{
    constexpr int SMAX = NS ? NS : kBoxMaxS;
    const int ns = NS ? NS : B.ns;
    d2 sum = {0.0, 0.0};
    // rows beyond this rank's block read as zero rows (with more ranks the last 128-row group of a
    // block may reach into the next rank's rows, which are real states of the box)
    const int64_t r0 = (c << 7) + 2 * lane;
    if (r0 >= nloc) return sum;
    const int64_t g = row0 + r0;
    // coordinates of row g: successive division by the box dimensions (exact: g < 2^31, one correction step)
    int x[SMAX];
    uint32_t q = (uint32_t)g;
#pragma unroll
    for (int s = 0; s < SMAX; ++s) {
        x[s] = 0;
        if (s + 1 < ns) {
            const int d = B.dims[s];
            uint32_t t = (uint32_t)((double)q * B.inv_dim[s]);
            int r = (int)(q - t * (uint32_t)d);
            if (r < 0) {
                --t;
                r += d;
            } else if (r >= d) {
                ++t;
                r -= d;
            }
            x[s] = r;
            q = t;
        } else if (s + 1 == ns) {
            x[s] = (int)q;
        }
    }
    sum.x = row_box<NS, NR>(B, tab, x, xg, g);
    if (r0 + 1 < nloc) {
        bool carry = true;                               // next row: +1 with carry
#pragma unroll
        for (int s = 0; s < SMAX; ++s) {
            if (s < ns && carry) {
                const int v = x[s] + 1;
                carry = v >= B.dims[s] && s + 1 < ns;
                x[s] = carry ? 0 : v;
            }
        }
        sum.y = row_box<NS, NR>(B, tab, x, xg, g + 1);
    }
    return sum;
}

// Single-factor fast path (BoxFast): NS species with PER entry slots each, both compile-time, so the
// species and slot of every entry are constants: straight-line code, no branches, all gathers of x and
// table look-ups of a row in flight together.  Per species ONE 16-byte LDS entry gives the sum of its
// propensities at x_s (its share of DIAG, StateSpace.f90:207-212) and a word with one bit per entry:
// "this coordinate lets the entry's source state x - nu lie inside the box"; the AND over the species
// is the row's set of valid entries.  An invalid entry is not branched around: its mask (0 / -1)
// redirects the look-up to the 0.0 at the head of the LDS image.
// A lane owns rows 2l and 2l+1 of the wave's 128, and ONE 16-byte load per entry fetches the source
// elements of both (x[g + delta], x[g + 1 + delta]): the kernel is bound by the number of vector-memory
// instructions a CU can issue, not by bytes.  If only one of the two rows has the entry, the other slot
// holds some other element of x, or the element just before / behind x (every device buffer carries
// guard words, DevBuf): finite, and multiplied by the 0.0.  x is addressed as wave base (scalar) +
// 32-bit lane offset (box_plan checks the reach).  The descriptor is read ONCE per wavefront
// into scalar registers (BoxRegs): left as loads inside the row code they would be re-issued for every
// row, as per-lane vector loads.  BoxRegs, box_load and box_df are shared with the block product: kfsp_box_dev.h.
template <int S, int NS, int PER>
__device__ __forceinline__ void box_species(const BoxRegs<NS, PER> &R, int xa, int xb, unsigned va, unsigned vb,
                                            global_bytes_t xw, unsigned voff, double &acca, double &accb)
{
    const unsigned lds0 = (unsigned)(size_t)(lds_bytes_t)box_lds;                  // LDS address of the image = of its 0.0
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int ma = __builtin_amdgcn_sbfe(va, S * PER + j, 1);                  // -1: source state of row A inside the box
        const int mb = __builtin_amdgcn_sbfe(vb, S * PER + j, 1);
        const unsigned ata = lds0 + (unsigned)(8 * xa + R.koff8[S][j]);           // a_k(x - nu_k) ...
        const unsigned atb = lds0 + (unsigned)(8 * xb + R.koff8[S][j]);
        const double a1a = *(const __attribute__((address_space(3))) double *)(size_t)((ma & ata) | (~ma & lds0));   // ... or 0
        const double a1b = *(const __attribute__((address_space(3))) double *)(size_t)((mb & atb) | (~mb & lds0));
        const unsigned vsrc = voff + (unsigned)R.delta8[S][j];                     // (the same in every trip of the lane)
        const unsigned at = (unsigned)__builtin_amdgcn_bitop3_b32(ma | mb, (int)vsrc, (int)voff, 0xCA);   // either ? vsrc : voff
        const box_pair_t xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + at);
        acca += a1a * xv.x;
        accb += a1b * xv.y;
    }
}

template <int NS, int PER>
__device__ __forceinline__ d2 rows_box1(const BoxRegs<NS, PER> &R, const double *__restrict__ xg,
                                        int64_t row0, int64_t nloc, int64_t c, int lane)
{
    d2 sum = {0.0, 0.0};
    const int64_t r0 = (c << 7) + 2 * lane;
    if (r0 >= nloc) return sum;
    const int64_t g = row0 + r0;
    // x of this wave's 128 rows and everything an entry reaches from them: scalar base + unsigned lane offset
    const uint64_t xb = reinterpret_cast<uint64_t>(xg + (row0 + (c << 7))) - (uint64_t)(int64_t)R.bias8;
    const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
    const unsigned voff = (unsigned)(16 * lane + R.bias8);
    // coordinates of row g: successive division by the box dimensions (exact: g < 2^31, one correction step)
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    uint32_t q = (uint32_t)g;
#define KFSP_BOX_DEC(S, VAR)                                             \
    if (NS > S + 1) {                                                    \
        const int d = R.dims[NS > S ? S : 0];                            \
        uint32_t t = (uint32_t)((double)q * R.inv_dim[NS > S ? S : 0]);  \
        int r = (int)(q - t * (uint32_t)d);                              \
        const int lo = r < 0, hi = r >= d;                               \
        t = t - lo + hi;                                                 \
        r = r + (lo ? d : 0) - (hi ? d : 0);                             \
        VAR = r;                                                         \
        q = t;                                                           \
    } else if (NS == S + 1) {                                            \
        VAR = (int)q;                                                    \
    }
    KFSP_BOX_DEC(0, c0)
    KFSP_BOX_DEC(1, c1)
    KFSP_BOX_DEC(2, c2)
    KFSP_BOX_DEC(3, c3)
    KFSP_BOX_DEC(4, c4)
    KFSP_BOX_DEC(5, c5)
#undef KFSP_BOX_DEC
    // the next row: +1 with carry (the last species never wraps while g + 1 < n)
    int b0 = c0, b1 = c1, b2 = c2, b3 = c3, b4 = c4, b5 = c5, carry = 1;
#define KFSP_BOX_INC(S, VAR)                                             \
    if (NS > S) {                                                        \
        const int v = VAR + carry;                                       \
        const int wrap = (NS > S + 1) && v >= R.dims[NS > S ? S : 0];    \
        VAR = wrap ? 0 : v;                                              \
        carry = wrap;                                                    \
    }
    KFSP_BOX_INC(0, b0)
    KFSP_BOX_INC(1, b1)
    KFSP_BOX_INC(2, b2)
    KFSP_BOX_INC(3, b3)
    KFSP_BOX_INC(4, b4)
    KFSP_BOX_INC(5, b5)
#undef KFSP_BOX_INC
    const bool two = r0 + 1 < nloc;
    if (!two) b0 = b1 = b2 = b3 = b4 = b5 = 0;                 // (no such row: any coordinates inside the tables)
    double dsa, dsb;
    unsigned va, vb;
    box_df<NS, PER>(R, c0, c1, c2, c3, c4, c5, dsa, va);
    box_df<NS, PER>(R, b0, b1, b2, b3, b4, b5, dsb, vb);
    if (!two) vb = 0u;
    const box_pair_t xd = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + voff);
    double acca = 0.0, accb = 0.0;
    box_species<0, NS, PER>(R, c0, b0, va, vb, xw, voff, acca, accb);
    if (NS > 1) box_species<(NS > 1 ? 1 : 0), NS, PER>(R, c1, b1, va, vb, xw, voff, acca, accb);
    if (NS > 2) box_species<(NS > 2 ? 2 : 0), NS, PER>(R, c2, b2, va, vb, xw, voff, acca, accb);
    if (NS > 3) box_species<(NS > 3 ? 3 : 0), NS, PER>(R, c3, b3, va, vb, xw, voff, acca, accb);
    if (NS > 4) box_species<(NS > 4 ? 4 : 0), NS, PER>(R, c4, b4, va, vb, xw, voff, acca, accb);
    if (NS > 5) box_species<(NS > 5 ? 5 : 0), NS, PER>(R, c5, b5, va, vb, xw, voff, acca, accb);
    sum.x = acca - dsa * xd.x;
    sum.y = two ? accb - dsb * xd.y : 0.0;
    return sum;
}

// FMT: 0 SELL-64, 1 banded, 2 banded with group masks, 3 matrix-free box (descriptor interpreted at run time),
// 4 matrix-free box, single-factor fast path with NS species and NE entry slots per species, 5 SELL-64 with coded columns,
// 9 and 10 banded with dictionary-coded values (NS = bits per code, NE = bytes per row record) and their variants LANES and
// INNER: described at the rule that chooses among them, dia_code_kernel (kfsp_dia_diag.h).  INNER kernels are held to the
// occupancy of the loaded path (8 waves per SIMD, 7 with two fused dot products).
template <bool NT, int FMT, int CW, int CREC, bool LANES, int INNER>
__device__ __forceinline__ d2 rows_dia_trip(const DiaDev &D, const DiaCodeDev &C, const DiaDiagDev &G, const double *__restrict__ xg,
                                            int64_t row0, int64_t ct, int lane, unsigned gm, int dmin, int dmax, const DiaDiagDev &Gi)
{
    constexpr bool FOLD = FMT == 10;
    if constexpr (INNER != 0) {
        // uniform: the trip, the row range and the offsets sit in SGPRs
        if (dia_inner_trip(row0 + (ct << 7), D.n, dmin, dmax)) return rows_dia_inner<NT, CW, INNER>(D, C, Gi, xg, row0, ct, lane);
    }
    return rows_dia<NT, FMT == 2, CW, CREC, FOLD, FOLD && LANES>(D, C, G, xg, row0, ct, lane, gm);
}

template <int MODE, bool NT, int FMT, int NS = 0, int NE = 0, bool LANES = false, int INNER = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(INNER ? (MODE == 3 ? 7 : 8) : 1, 8))) void k_spmv(SpmvArgs a)
{
    constexpr bool DIA = FMT != 0 && FMT != 5;
    constexpr bool BOX = FMT == 3 || FMT == 4;
    constexpr bool CODED = FMT == 9 || FMT == 10;
    constexpr bool FOLD = FMT == 10;
    constexpr int CW = CODED ? NS : 0, CREC = CODED && NE == 16 ? 16 : 8;
    __shared__ double red[12];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (MODE != 0) {
        if (*a.brk_flag) return;
    }
    const double *tab = nullptr;
    BoxRegs<(NS ? NS : 1), (NE ? NE : 1)> boxr;
    if (BOX) {
        for (int i = threadIdx.x; i < a.B.ntab; i += kBlock) box_lds[i] = a.box_tab[i];
        __syncthreads();
        tab = box_lds;
        if (FMT == 4) box_load(a.box_fast, boxr);
    }
    if (CODED) {
        // the dictionaries of all diagonals, back to back (<= kDiaCodeLds bytes: 4 workgroups per CU)
        // ... and behind them (FOLD) the DIAG tables, which build_dia_code keeps behind the dictionaries in memory too
        const int nent = a.C.doff[a.D.nd] + (FOLD ? a.G.ntab : 0);
        // All loads of a pass are issued before its first store, 16 bytes per lane: 2048 entries - the whole image of
        // the benchmark's generator - cost ONE trip to memory.  (One entry per lane and pass waited for every load
        // before the next was issued: seven latencies in front of the first row of every workgroup.)
        const int npair = nent >> 1;
        const d2 *src = reinterpret_cast<const d2 *>(a.C.dict);     // (device buffers are 256-byte aligned)
        d2 *dst = reinterpret_cast<d2 *>(box_lds);
        for (int i0 = threadIdx.x; i0 < npair; i0 += 4 * kBlock) {
            d2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * kBlock < npair) v[u] = src[i0 + u * kBlock];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * kBlock < npair) dst[i0 + u * kBlock] = v[u];
        }
        if ((nent & 1) && threadIdx.x == 0) box_lds[nent - 1] = a.C.dict[nent - 1];
        __syncthreads();
    }
    int dmin = 0, dmax = 0;                               // INNER: the smallest and the largest stored offset, 0 included
    DiaDiagDev Gi = DiaDiagDev{};                         // INNER: the fold's descriptor as rows_dia_inner reads it
    if constexpr (INNER != 0) {
        // (the empty statement hides that these are kernel arguments: they stay in SGPRs across the trip loop instead of being
        // fetched again, with a wait, inside every trip)
        Gi = a.G;
        asm volatile("" : "+s"(Gi.magic[0]), "+s"(Gi.magic[1]), "+s"(Gi.shift[0]), "+s"(Gi.shift[1]), "+s"(Gi.size[0]), "+s"(Gi.size[1]),
                          "+s"(Gi.size[2]), "+s"(Gi.toff[1]), "+s"(Gi.toff[2]), "+s"(Gi.base));
#pragma unroll
        for (int d = 0; d < INNER; ++d) {
            dmin = min(dmin, a.D.delta[d]);
            dmax = max(dmax, a.D.delta[d]);
        }
    }

    // SELL: one 64-row chunk per wavefront trip; DIA: one 128-row group
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;                        // workgroups per XCD
    const int64_t cpx = (a.trip_end - a.trip_begin + 7) >> 3;
    const int64_t cbeg = a.trip_begin + (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < a.trip_end) ? cbeg + cpx : a.trip_end;
    const int64_t cstep = (int64_t)bx * 4;
    int64_t c = cbeg + (int64_t)slot * 4 + wave;

    // The first trip's row sums are started before the pending norm is
    // finished: the partial-sum round trip overlaps the first generator loads.
    d2 sum = {0.0, 0.0};
    int64_t ct = c < a.trip_split ? c : c + a.trip_jump;   // actual trip of linear index c
    if (a.trip_order && c < cend) ct = __builtin_amdgcn_readfirstlane(a.trip_order[c]);
    unsigned gm = 0xFFFFFFFFu;                              // group mask of the trip about to be computed
    if (FMT == 2 && c < cend) gm = __builtin_amdgcn_readfirstlane(a.D.gmask[ct]);
    if (c < cend) {
        if (FMT == 4) sum = rows_box1<(NS ? NS : 1), (NE ? NE : 1)>(boxr, a.xg, a.row0, a.A.nrows, ct, lane);
        else if (BOX) sum = rows_box<0, 0>(a.B, tab, a.xg, a.row0, a.A.nrows, ct, lane);
        else if (DIA) sum = rows_dia_trip<NT, FMT, CW, CREC, LANES, INNER>(a.D, a.C, a.G, a.xg, a.row0, ct, lane, gm, dmin, dmax, Gi);
        else if (FMT == 5) sum.x = row_sell_coded<NT>(a.A, a.xg, a.row0, ct, lane);
            else sum.x = row_sell<NT>(a.A, a.xg, a.row0, ct, lane);
    }

    double s = 1.0;
    if (MODE != 0) {
        const double S = finish_sum(a.sq, red);
        const double nrm = sqrt(S);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (a.sq_final) *a.sq_final = S;
            if (a.h_sub) *a.h_sub = nrm;
        }
        if (a.break_tol >= 0.0 && !(nrm > a.break_tol)) {   // happy breakdown :249
            if (blockIdx.x == 0 && threadIdx.x == 0) *a.brk_flag = 1;
            return;
        }
        s = 1.0 / nrm;
    }

    double acc = 0.0, acc2 = 0.0;
    while (c < cend) {
        const int64_t cn = c + cstep;
        int64_t ctn = cn < a.trip_split ? cn : cn + a.trip_jump;
        if (a.trip_order && cn < cend) ctn = __builtin_amdgcn_readfirstlane(a.trip_order[cn]);
        if (FMT == 2 && cn < cend) gm = __builtin_amdgcn_readfirstlane(a.D.gmask[ctn]);
        if (DIA) {
            const int64_t r = (ct << 7) + 2 * lane;
            if (MODE != 0) {
                sum.x *= s;
                sum.y *= s;
            }
            *reinterpret_cast<d2 *>(a.y + r) = sum;
            if (MODE == 1 || MODE == 3) {
                const d2 u = *reinterpret_cast<const d2 *>(a.udot + r);
                acc += u.x * sum.x;
                acc += u.y * sum.y;
            }
            if (MODE == 2) {
                acc += sum.x * sum.x;
                acc += sum.y * sum.y;
            }
            if (MODE == 3) {
                const d2 u = *reinterpret_cast<const d2 *>(a.udot2 + r);
                acc2 += u.x * sum.x;
                acc2 += u.y * sum.y;
            }
        } else {
            const int64_t r = (ct << 6) + lane;
            double v = sum.x;
            if (MODE != 0) v *= s;
            a.y[r] = v;
            if (MODE == 1 || MODE == 3) acc += a.udot[r] * v;
            if (MODE == 2) acc += v * v;
            if (MODE == 3) acc2 += a.udot2[r] * v;
        }
        c = cn;
        ct = ctn;
        if (c < cend) {
            if (FMT == 4) sum = rows_box1<(NS ? NS : 1), (NE ? NE : 1)>(boxr, a.xg, a.row0, a.A.nrows, ct, lane);
            else if (BOX) sum = rows_box<0, 0>(a.B, tab, a.xg, a.row0, a.A.nrows, ct, lane);
            else if (DIA) sum = rows_dia_trip<NT, FMT, CW, CREC, LANES, INNER>(a.D, a.C, a.G, a.xg, a.row0, ct, lane, gm, dmin, dmax, Gi);
            else if (FMT == 5) sum.x = row_sell_coded<NT>(a.A, a.xg, a.row0, ct, lane);
            else sum.x = row_sell<NT>(a.A, a.xg, a.row0, ct, lane);
        }
    }
    if (MODE == 3) {
        double dummy = 0.0;
        block_allreduce_sum3(acc, acc2, dummy, red);
        if (threadIdx.x == 0) {
            a.partial[blockIdx.x] = acc;
            a.partial2[blockIdx.x] = acc2;
        }
    } else if (MODE != 0) {
        const double t = block_allreduce_sum(acc, red);
        if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
    }
}

typedef void (*SpmvFn)(SpmvArgs);

}  // namespace kfsp
