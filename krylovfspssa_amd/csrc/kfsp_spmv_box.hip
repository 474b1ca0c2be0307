// gfx950 kernels of the single-vector product on single-factor matrix-free boxes beyond k_spmv's format 4: format 6 with
// the near part of x in LDS (k_spmv_boxlds), format 7 in pencils (k_spmv_pencil), format 8 in slabs (k_spmv_slab).
#include "kfsp_box_dev.h"
#include "kfsp_dev.h"
#include "kfsp_dispatch.h"

namespace kfsp {

// ---------------------------------------------------------------------------------------------------------------
// Format 6: the single-factor matrix-free product (format 4) with the NEAR part of x staged in LDS.
// Format 4 fetches every entry's x pair with its own 16-byte global gather: a row's x goes through the CU's vector L1 once
// per entry (7 x for the repressilator, 13 x for the 6-species network), and at ~18 wave-instructions per ns chip-wide -
// half the 64 B/clk/CU of the L1 - that, not HBM, is what the kernel waits for (profiles/r03_pmc_summary_boxes_and_fsp.txt:
// the same rate on c3x and on c5s).  The four wavefronts of a workgroup take four consecutive 128-row trips, i.e. 512
// consecutive rows: their x and the `reach` rows on either side are loaded ONCE per workgroup pass (16 B per lane,
// coalesced, two buffers so that the next pass's window is in flight while this one is computed; one barrier per
// pass), and every entry whose shift is within the reach - the diagonal, +-1, +-d1, +-d1 d2 when they fit - reads its
// pair from LDS (ds_read2_b64, conflict-free: consecutive lanes read consecutive pairs).  Far entries keep their
// gathers.  Same table look-ups, same products, same order of additions as format 4: bit-identical results.
template <int S, int NS, int PER>
__device__ __forceinline__ void box_species_lds(const BoxRegs<NS, PER> &R, int xa, int xb, unsigned va, unsigned vb,
                                                global_bytes_t xw, unsigned voff, const double *win, int wrow, int reach8,
                                                double &acca, double &accb)
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
        const int d8 = R.delta8[S][j];
        box_pair_t xv;
        if ((d8 < 0 ? -d8 : d8) <= reach8) {                                      // uniform: the descriptor sits in SGPRs
            const int sh = (ma | mb) ? (d8 >> 3) : 0;                              // neither row has the entry: their own x
            xv.x = win[wrow + sh];
            xv.y = win[wrow + sh + 1];
        } else {
            const unsigned vsrc = voff + (unsigned)d8;
            const unsigned at = (unsigned)__builtin_amdgcn_bitop3_b32(ma | mb, (int)vsrc, (int)voff, 0xCA);   // either ? vsrc : voff
            xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + at);
        }
        acca += a1a * xv.x;
        accb += a1b * xv.y;
    }
}

template <int NS, int PER>
__device__ __forceinline__ d2 rows_box_lds(const BoxRegs<NS, PER> &R, const double *__restrict__ xg, int64_t row0, int64_t nloc,
                                           int64_t c, int lane, const double *win, int wrow, int reach8)
{
    d2 sum = {0.0, 0.0};
    const int64_t r0 = (c << 7) + 2 * lane;
    if (r0 >= nloc) return sum;
    const int64_t g = row0 + r0;
    const uint64_t xb = reinterpret_cast<uint64_t>(xg + (row0 + (c << 7))) - (uint64_t)(int64_t)R.bias8;
    const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                               (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
    const unsigned voff = (unsigned)(16 * lane + R.bias8);
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
    if (!two) b0 = b1 = b2 = b3 = b4 = b5 = 0;
    double dsa, dsb;
    unsigned va, vb;
    box_df<NS, PER>(R, c0, c1, c2, c3, c4, c5, dsa, va);
    box_df<NS, PER>(R, b0, b1, b2, b3, b4, b5, dsb, vb);
    if (!two) vb = 0u;
    const double xda = win[wrow], xdb = win[wrow + 1];
    double acca = 0.0, accb = 0.0;
    box_species_lds<0, NS, PER>(R, c0, b0, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    if (NS > 1) box_species_lds<(NS > 1 ? 1 : 0), NS, PER>(R, c1, b1, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    if (NS > 2) box_species_lds<(NS > 2 ? 2 : 0), NS, PER>(R, c2, b2, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    if (NS > 3) box_species_lds<(NS > 3 ? 3 : 0), NS, PER>(R, c3, b3, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    if (NS > 4) box_species_lds<(NS > 4 ? 4 : 0), NS, PER>(R, c4, b4, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    if (NS > 5) box_species_lds<(NS > 5 ? 5 : 0), NS, PER>(R, c5, b5, va, vb, xw, voff, win, wrow, reach8, acca, accb);
    sum.x = acca - dsa * xda;
    sum.y = two ? accb - dsb * xdb : 0.0;
    return sum;
}

// reach: rows staged on either side of the workgroup's 512 (even); x is readable for global rows [0, a.D.n)
template <int MODE, int NS, int PER>
__global__ __launch_bounds__(kBlock) void k_spmv_boxlds(SpmvArgs a, int reach)
{
    __shared__ double red[12];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (MODE != 0) {
        if (*a.brk_flag) return;
    }
    BoxRegs<NS, PER> boxr;
    for (int i = threadIdx.x; i < a.B.ntab; i += kBlock) box_lds[i] = a.box_tab[i];
    box_load(a.box_fast, boxr);
    const int W = 4 * 128 + 2 * reach;                     // doubles per window
    double *win0 = box_lds + ((a.B.ntab + 1) & ~1);        // two windows behind the table image (16-byte aligned)
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;                        // workgroups per XCD
    const int64_t trips = a.trip_end - a.trip_begin;
    const int64_t cpx = (((trips + 7) >> 3) + 3) & ~(int64_t)3;    // trips per XCD, a multiple of the 4 a workgroup takes per pass
    const int64_t cbeg = a.trip_begin + (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < a.trip_end) ? cbeg + cpx : a.trip_end;
    const int64_t cstep = (int64_t)bx * 4;
    int64_t c0 = cbeg + (int64_t)slot * 4;                // the workgroup's first trip of this pass (uniform)
    const int64_t xn = a.D.n;
    // window of the pass that starts at trip cw: global rows [row0 + 128 cw - reach, row0 + 128 (cw + 4) + reach), zero outside x
    auto stage = [&](double *win, int64_t cw) {
        const int64_t gb = a.row0 + (cw << 7) - reach;
        for (int i = 2 * (int)threadIdx.x; i < W; i += 2 * kBlock) {
            const int64_t g = gb + i;
            d2 v;
            if (g >= 0 && g + 1 < xn) {
                v = *reinterpret_cast<const d2 *>(a.xg + g);
            } else {
                v.x = (g >= 0 && g < xn) ? a.xg[g] : 0.0;
                v.y = (g + 1 >= 0 && g + 1 < xn) ? a.xg[g + 1] : 0.0;
            }
            *reinterpret_cast<d2 *>(win + i) = v;
        }
    };
    if (c0 < cend) stage(win0, c0);
    __syncthreads();                                       // table image + first window
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
    const int reach8 = 8 * reach;
    const int wrow = wave * 128 + 2 * lane + reach;        // this lane's first row inside a window
    double acc = 0.0, acc2 = 0.0;
    int buf = 0;
    while (c0 < cend) {
        const int64_t c0n = c0 + cstep;
        double *win = win0 + buf * W;
        if (c0n < cend) stage(win0 + (buf ^ 1) * W, c0n);  // the next window travels while this one is computed
        const int64_t c = c0 + wave;
        if (c < cend) {
            d2 sum = rows_box_lds<NS, PER>(boxr, a.xg, a.row0, a.A.nrows, c, lane, win, wrow, reach8);
            const int64_t r = (c << 7) + 2 * lane;
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
        }
        __syncthreads();                                   // next window complete, this one free
        c0 = c0n;
        buf ^= 1;
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

// format 6: lds_bytes = table image (rounded to 16 B) + two windows of (512 + 2 reach) doubles; a.B.pad: the instantiation (box_plan)
void launch_spmv_boxlds(int mode, int grid, const SpmvArgs &a, hipStream_t st, size_t lds_bytes, int reach)
{
    const auto fn = dispatch_mode(mode, [&](auto M) {
        return dispatch_box_inst(a.B.pad, [](auto NS, auto PER) { return k_spmv_boxlds<decltype(M)::value, decltype(NS)::value, decltype(PER)::value>; });
    });
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), lds_bytes, st, a, reach);
}
// ------------------------------------------------------------------------------------------------
// Format 7 (round 4): the PENCIL product of a matrix-free box (single-factor fast form, one rank).
//
// Format 4 takes the rows 128 at a time in (some) order of the row index and gathers every entry's source element of x from
// memory.  On the 6-species boxes (BASELINE config 5: 22^6) that is where the time goes: the two entries of the SLOWEST species
// reach +-22^5 rows = 41 MB, no cache holds anything that far, and x crosses the fabric ~6 times per product
// (profiles/r04_pmc_trip_order_tiles.txt: 5.2-5.6 GB read for a 0.9 GB vector, at 0.73-0.80 of the HBM peak - the kernel is bound
// by that traffic; ordering the trips in small tiles moves it by 7 %).
// Here a wavefront owns the 128 rows of a "base trip" of ONE plane of the slowest species and walks the planes: rows
// lo + p * plane_rows, p = 0 .. planes - 1.  Along that walk
//   * the coordinates of the other species, their shares of DIAG, every entry's table value a_k(x - nu) and its validity do not
//     change: they are worked out once per pencil (coordinate decoding, 10 table look-ups) instead of once per 128 rows;
//   * the source elements of the slowest species' own entries are the lane's OWN rows of the previous / next plane: the pair
//     the lane loaded one step ago and the pair it loads one step ahead - registers, no memory access at all;
//   * the slowest species' coordinate is the step number: its table values and valid bits are wave-uniform.
// Per step and lane: 10 gathers + 1 streaming pair load and ~40 vector instructions, against 13 gathers and ~300; and what
// crosses the fabric is x once plus whatever the second-slowest stride misses in the L2 (the base trips are taken in small tiles,
// box_tile_order, so that those neighbours are in flight on the same XCD at the same step).
// Every row is the same sequence of fused multiply-adds over the same operands as in format 4: products are bit-identical
// (tests/test_gpu_box.py, tests/test_gpu_configs.py).  Eligibility (box_plan, kfsp_box_plan.h): the slowest species' entries reach
// exactly one plane, no other entry moves that species, planes have an even number of rows, enough base trips to fill the chip.
// SIMPLE: no entry of another species moves the slowest one (every birth-death / mass-action box whose reactions change one
// species each): the entries served from memory keep their validity along the pencil.  Otherwise their valid bit of the
// slowest species (wave-uniform, from its table at the step's population) is applied step by step.
template <int MODE, int NS, int PER, bool SIMPLE>
__global__ __launch_bounds__(kBlock) void k_spmv_pencil(SpmvArgs a, int64_t plane_rows, int planes, int64_t base_trips,
                                                        const int32_t *__restrict__ order)
{
    constexpr int L = NS - 1;                       // the slowest species
    constexpr int NE = L * PER;                     // entries whose source comes from memory
    __shared__ double red[12];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (MODE != 0) {
        if (*a.brk_flag) return;
    }
    for (int i = threadIdx.x; i < a.B.ntab; i += kBlock) box_lds[i] = a.box_tab[i];
    __syncthreads();
    BoxRegs<NS, PER> R;
    box_load(a.box_fast, R);
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
    const int xcd = blockIdx.x & 7;
    const int slot = blockIdx.x >> 3;
    const int bx = gridDim.x >> 3;
    const int64_t cpx = (base_trips + 7) >> 3;
    const int64_t cbeg = (int64_t)xcd * cpx;
    const int64_t cend = (cbeg + cpx < base_trips) ? cbeg + cpx : base_trips;
    const int64_t cstep = (int64_t)bx * 4;
    const lds_bytes_t lds = (lds_bytes_t)box_lds;
    const unsigned lds0 = (unsigned)(size_t)lds;
    const int64_t plane_bytes = plane_rows * 8;
    double acc = 0.0, acc2 = 0.0;
    for (int64_t c = cbeg + (int64_t)slot * 4 + wave; c < cend; c += cstep) {
        const int64_t ct = order ? (int64_t)__builtin_amdgcn_readfirstlane(order[c]) : c;
        const int64_t r0 = (ct << 7) + 2 * lane;                  // the lane's rows r0, r0 + 1 of every plane
        if (r0 < plane_rows) {                                     // (plane_rows is even: both rows or neither)
            // ---- what does not change along the pencil
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
            uint32_t q = (uint32_t)r0;
#define KFSP_PEN_DEC(S, VAR)                                             \
    if (L > S + 1) {                                                     \
        const int d = R.dims[L > S ? S : 0];                             \
        uint32_t t = (uint32_t)((double)q * R.inv_dim[L > S ? S : 0]);   \
        int r = (int)(q - t * (uint32_t)d);                              \
        const int lo_ = r < 0, hi_ = r >= d;                             \
        t = t - lo_ + hi_;                                               \
        r = r + (lo_ ? d : 0) - (hi_ ? d : 0);                           \
        VAR = r;                                                         \
        q = t;                                                           \
    } else if (L == S + 1) {                                             \
        VAR = (int)q;                                                    \
    }
            KFSP_PEN_DEC(0, c0)
            KFSP_PEN_DEC(1, c1)
            KFSP_PEN_DEC(2, c2)
            KFSP_PEN_DEC(3, c3)
            KFSP_PEN_DEC(4, c4)
#undef KFSP_PEN_DEC
            int b0 = c0, b1 = c1, b2 = c2, b3 = c3, b4 = c4, carry = 1;
#define KFSP_PEN_INC(S, VAR)                                             \
    if (L > S) {                                                         \
        const int v = VAR + carry;                                       \
        const int wrap = (L > S + 1) && v >= R.dims[L > S ? S : 0];      \
        VAR = wrap ? 0 : v;                                              \
        carry = wrap;                                                    \
    }
            KFSP_PEN_INC(0, b0)
            KFSP_PEN_INC(1, b1)
            KFSP_PEN_INC(2, b2)
            KFSP_PEN_INC(3, b3)
            KFSP_PEN_INC(4, b4)
#undef KFSP_PEN_INC
            // shares of DIAG and valid bits of the species below the slowest, in species order (the order format 4 adds them in)
            double dsa0, dsb0;
            unsigned va0, vb0;
            {
                const lds_bytes_t fa = lds + R.df8[0] + 16 * c0, fb = lds + R.df8[0] + 16 * b0;
                dsa0 = *(const __attribute__((address_space(3))) double *)fa;
                va0 = *(const __attribute__((address_space(3))) unsigned *)(fa + 8);
                dsb0 = *(const __attribute__((address_space(3))) double *)fb;
                vb0 = *(const __attribute__((address_space(3))) unsigned *)(fb + 8);
            }
#define KFSP_PEN_DF(S, CA, CB)                                                                       \
    if (L > S) {                                                                                     \
        const lds_bytes_t fa = lds + R.df8[L > S ? S : 0] + 16 * CA, fb = lds + R.df8[L > S ? S : 0] + 16 * CB; \
        dsa0 += *(const __attribute__((address_space(3))) double *)fa;                               \
        va0 &= *(const __attribute__((address_space(3))) unsigned *)(fa + 8);                        \
        dsb0 += *(const __attribute__((address_space(3))) double *)fb;                               \
        vb0 &= *(const __attribute__((address_space(3))) unsigned *)(fb + 8);                        \
    }
            KFSP_PEN_DF(1, c1, b1)
            KFSP_PEN_DF(2, c2, b2)
            KFSP_PEN_DF(3, c3, b3)
            KFSP_PEN_DF(4, c4, b4)
#undef KFSP_PEN_DF
            // table values of the entries served from memory (0.0 where the source state lies outside the box) and where their
            // source pair sits relative to the lane's own pair
            double ta[NE > 0 ? NE : 1], tb[NE > 0 ? NE : 1];
            unsigned off[NE > 0 ? NE : 1];
            const unsigned voff = (unsigned)(16 * lane + R.bias8);
#define KFSP_PEN_ENT(S, CA, CB)                                                                      \
    if (L > S) {                                                                                     \
        _Pragma("unroll") for (int j = 0; j < PER; ++j) {                                            \
            constexpr int e = (L > S ? S : 0) * PER;                                                 \
            const int ma = __builtin_amdgcn_sbfe(va0, e + j, 1), mb = __builtin_amdgcn_sbfe(vb0, e + j, 1); \
            const unsigned ata = lds0 + (unsigned)(8 * CA + R.koff8[L > S ? S : 0][j]);              \
            const unsigned atb = lds0 + (unsigned)(8 * CB + R.koff8[L > S ? S : 0][j]);              \
            ta[e + j] = *(const __attribute__((address_space(3))) double *)(size_t)((ma & ata) | (~ma & lds0)); \
            tb[e + j] = *(const __attribute__((address_space(3))) double *)(size_t)((mb & atb) | (~mb & lds0)); \
            off[e + j] = (ma | mb) ? voff + (unsigned)R.delta8[L > S ? S : 0][j] : voff;             \
        }                                                                                            \
    }
            KFSP_PEN_ENT(0, c0, b0)
            KFSP_PEN_ENT(1, c1, b1)
            KFSP_PEN_ENT(2, c2, b2)
            KFSP_PEN_ENT(3, c3, b3)
            KFSP_PEN_ENT(4, c4, b4)
#undef KFSP_PEN_ENT
            // ---- the walk over the planes
            uint64_t xb = reinterpret_cast<uint64_t>(a.xg + (ct << 7)) - (uint64_t)(int64_t)R.bias8;
            box_pair_t xprev = {0.0, 0.0}, xcur, xnext = {0.0, 0.0};
            {
                const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
                xcur = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + voff);
            }
            int64_t row = r0;
            for (int p = 0; p < planes; ++p) {
                const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
                if (p + 1 < planes) xnext = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + plane_bytes + voff);
                // the slowest species at population p: its share of DIAG and its valid bits are the same for every lane
                const lds_bytes_t fl = lds + R.df8[L] + 16 * p;
                const double dsl = *(const __attribute__((address_space(3))) double *)fl;
                const unsigned vl = *(const __attribute__((address_space(3))) unsigned *)(fl + 8);
                double acca = 0.0, accb = 0.0;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    if (SIMPLE) {
                        const box_pair_t xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + off[e]);
                        acca += ta[e] * xv.x;
                        accb += tb[e] * xv.y;
                    } else {
                        // (the entry moves the slowest species too: whether its source plane exists is this step's bit)
                        const bool here = (vl >> e) & 1u;
                        const box_pair_t xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + (here ? off[e] : voff));
                        acca += (here ? ta[e] : 0.0) * xv.x;
                        accb += (here ? tb[e] : 0.0) * xv.y;
                    }
                }
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int ma = __builtin_amdgcn_sbfe(va0 & vl, L * PER + j, 1), mb = __builtin_amdgcn_sbfe(vb0 & vl, L * PER + j, 1);
                    const unsigned at = lds0 + (unsigned)(8 * p + R.koff8[L][j]);
                    const double a1a = *(const __attribute__((address_space(3))) double *)(size_t)((ma & at) | (~ma & lds0));
                    const double a1b = *(const __attribute__((address_space(3))) double *)(size_t)((mb & at) | (~mb & lds0));
                    // The source pair.  An entry that only moves the slowest species by one: the lane's own rows one plane
                    // down / up - the pair it loaded a step ago / loads a step ahead (format 4 gathers x[g + delta] from
                    // memory).  Any other entry of this species (a propensity that depends on it but moves others): from memory,
                    // as in format 4.  Where neither row has the entry: the own pair (format 4 reads it and multiplies by 0.0).
                    const int d = R.delta8[L][j];
                    box_pair_t xv;
                    if ((int64_t)d == plane_bytes) xv = xnext;
                    else if ((int64_t)d == -plane_bytes) xv = xprev;
                    else xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + ((ma | mb) ? voff + (unsigned)d : voff));
                    if (!(ma | mb)) xv = xcur;
                    acca += a1a * xv.x;
                    accb += a1b * xv.y;
                }
                d2 sum;
                sum.x = acca - (dsa0 + dsl) * xcur.x;
                sum.y = accb - (dsb0 + dsl) * xcur.y;
                if (MODE != 0) {
                    sum.x *= s;
                    sum.y *= s;
                }
                *reinterpret_cast<d2 *>(a.y + row) = sum;
                if (MODE == 1 || MODE == 3) {
                    const d2 u = *reinterpret_cast<const d2 *>(a.udot + row);
                    acc += u.x * sum.x;
                    acc += u.y * sum.y;
                }
                if (MODE == 2) {
                    acc += sum.x * sum.x;
                    acc += sum.y * sum.y;
                }
                if (MODE == 3) {
                    const d2 u = *reinterpret_cast<const d2 *>(a.udot2 + row);
                    acc2 += u.x * sum.x;
                    acc2 += u.y * sum.y;
                }
                xprev = xcur;
                xcur = xnext;
                xb += (uint64_t)plane_bytes;
                row += plane_rows;
            }
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

// format 7 (the instantiations of format 4 whose species count is the model's: 3 and 6 species with two slots, 6 with four)
void launch_spmv_pencil(int mode, int grid, const SpmvArgs &a, hipStream_t st, size_t lds_bytes, int64_t plane_rows, int planes,
                        int64_t base_trips, const int32_t *order, bool simple)
{
    const auto fn = dispatch_mode(mode, [&](auto M) {
        return dispatch_bool(simple, [&](auto SIMPLE) {
            return dispatch_box_walk_inst(a.B.pad, [](auto NS, auto PER) {
                return k_spmv_pencil<decltype(M)::value, decltype(NS)::value, decltype(PER)::value, decltype(SIMPLE)::value>;
            });
        });
    });
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), lds_bytes, st, a, plane_rows, planes, base_trips, order);
}
// ------------------------------------------------------------------------------------------------
// Format 8 (round 4): pencils in SLABS.  Format 7 removed the slowest species' streams; what was left of the traffic on the
// 6-species boxes was the SECOND-slowest species (22^4 rows = 1.9 MB away: the L2 does not hold it across a pencil's 41 MB
// steps).  Here a WORKGROUP owns the same 128 rows (of the index below the second-slowest stride) in W consecutive lines of
// that species - wavefront w walks the pencil of line g W + w - and all its wavefronts take the planes in step, one
// workgroup barrier per step: the second-slowest species' own +-1 entries are then the pair wavefront w -+ 1 holds for the
// same plane, handed over through LDS (16 bytes per lane, two buffers).  Only the first and the last line of a workgroup
// gather such a neighbour from memory (22 lines in two workgroups of 11: 2 of 44 neighbour pairs).  Everything else is
// format 7: invariants hoisted out of the walk, the slowest species' entries from the lane's own previous / next pair.
// Same fused multiply-adds over the same operands: bit-identical products.
template <int MODE, int NS, int PER, bool SIMPLE>
__global__ __launch_bounds__(768) void k_spmv_slab(SpmvArgs a, int64_t plane_rows, int planes, int64_t line_rows, int lines, int groups,
                                                    int64_t lo_trips)
{
    constexpr int L = NS - 1;                       // the slowest species: planes
    constexpr int M = NS - 2;                       // the second slowest: lines
    constexpr int NE = M * PER;                     // entries of the species below them: always gathered from memory
    __shared__ double red[12];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = (int)(blockDim.x >> 6);
    if (MODE != 0) {
        if (*a.brk_flag) return;
    }
    for (int i = threadIdx.x; i < a.B.ntab; i += blockDim.x) box_lds[i] = a.box_tab[i];
    __syncthreads();
    BoxRegs<NS, PER> R;
    box_load(a.box_fast, R);
    // the exchange area behind the table image: two buffers of W x 64 pairs
    box_pair_t *xchg = reinterpret_cast<box_pair_t *>(box_lds + ((a.B.ntab + 1) & ~1));
    double s = 1.0;
    if (MODE != 0) {
        // (finish_sum for a workgroup of W wavefronts, W = 1 .. 12: the four wavefront sums of a 256-thread kernel - lane l of
        // wavefront v adds the partials 64 v + l, + 256, ... - are taken by wavefront v where W >= 4 and shared out over the
        // W wavefronts there are where W < 4; the same additions per lane, the same pairing of the four sums)
        for (int v = wave; v < kBlock / 64; v += W) {
            double t = 0.0;
            for (int i = 64 * v + lane; i < a.sq.n; i += kBlock) t += a.sq.p[i];
            t = wave_allreduce_sum(t);
            if (lane == 0) red[v] = t;
        }
        __syncthreads();
        const double S = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
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
    const lds_bytes_t lds = (lds_bytes_t)box_lds;
    const unsigned lds0 = (unsigned)(size_t)lds;
    const int64_t plane_bytes = plane_rows * 8, line_bytes = line_rows * 8;
    const int64_t total = lo_trips * groups;
    double acc = 0.0, acc2 = 0.0;
    for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
        const int g = (int)(b % groups);
        const int64_t ct = b / groups;
        const int sl = g * W + wave;                               // this wavefront's line
        const int64_t r0 = (ct << 7) + 2 * lane;                   // the lane's rows r0, r0 + 1 of the line (line_rows is even)
        const bool live = sl < lines && r0 < line_rows;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        double dsa0 = 0.0, dsb0 = 0.0;
        unsigned va0 = 0u, vb0 = 0u;
        double ta[NE > 0 ? NE : 1], tb[NE > 0 ? NE : 1];
        unsigned off[NE > 0 ? NE : 1];
        const unsigned voff = (unsigned)(16 * lane + R.bias8);
#pragma unroll
        for (int e = 0; e < (NE > 0 ? NE : 1); ++e) {
            ta[e] = tb[e] = 0.0;
            off[e] = voff;
        }
        if (live) {
            uint32_t q = (uint32_t)r0;
#define KFSP_SLB_DEC(S, VAR)                                             \
    if (M > S + 1) {                                                     \
        const int d = R.dims[M > S ? S : 0];                             \
        uint32_t t = (uint32_t)((double)q * R.inv_dim[M > S ? S : 0]);   \
        int r = (int)(q - t * (uint32_t)d);                              \
        const int lo_ = r < 0, hi_ = r >= d;                             \
        t = t - lo_ + hi_;                                               \
        r = r + (lo_ ? d : 0) - (hi_ ? d : 0);                           \
        VAR = r;                                                         \
        q = t;                                                           \
    } else if (M == S + 1) {                                             \
        VAR = (int)q;                                                    \
    }
            KFSP_SLB_DEC(0, c0)
            KFSP_SLB_DEC(1, c1)
            KFSP_SLB_DEC(2, c2)
            KFSP_SLB_DEC(3, c3)
#undef KFSP_SLB_DEC
            int b0 = c0, b1 = c1, b2 = c2, b3 = c3, carry = 1;
#define KFSP_SLB_INC(S, VAR)                                             \
    if (M > S) {                                                         \
        const int v = VAR + carry;                                       \
        const int wrap = (M > S + 1) && v >= R.dims[M > S ? S : 0];      \
        VAR = wrap ? 0 : v;                                              \
        carry = wrap;                                                    \
    }
            KFSP_SLB_INC(0, b0)
            KFSP_SLB_INC(1, b1)
            KFSP_SLB_INC(2, b2)
            KFSP_SLB_INC(3, b3)
#undef KFSP_SLB_INC
            {
                const lds_bytes_t fa = lds + R.df8[0] + 16 * c0, fb = lds + R.df8[0] + 16 * b0;
                dsa0 = *(const __attribute__((address_space(3))) double *)fa;
                va0 = *(const __attribute__((address_space(3))) unsigned *)(fa + 8);
                dsb0 = *(const __attribute__((address_space(3))) double *)fb;
                vb0 = *(const __attribute__((address_space(3))) unsigned *)(fb + 8);
            }
#define KFSP_SLB_DF(S, CA, CB)                                                                       \
    if (M > S) {                                                                                     \
        const lds_bytes_t fa = lds + R.df8[M > S ? S : 0] + 16 * CA, fb = lds + R.df8[M > S ? S : 0] + 16 * CB; \
        dsa0 += *(const __attribute__((address_space(3))) double *)fa;                               \
        va0 &= *(const __attribute__((address_space(3))) unsigned *)(fa + 8);                        \
        dsb0 += *(const __attribute__((address_space(3))) double *)fb;                               \
        vb0 &= *(const __attribute__((address_space(3))) unsigned *)(fb + 8);                        \
    }
            KFSP_SLB_DF(1, c1, b1)
            KFSP_SLB_DF(2, c2, b2)
            KFSP_SLB_DF(3, c3, b3)
#undef KFSP_SLB_DF
            {
                // the second-slowest species at this wavefront's line: uniform
                const lds_bytes_t fm = lds + R.df8[M] + 16 * sl;
                const double dsm = *(const __attribute__((address_space(3))) double *)fm;
                const unsigned vm = *(const __attribute__((address_space(3))) unsigned *)(fm + 8);
                dsa0 += dsm;
                dsb0 += dsm;
                va0 &= vm;
                vb0 &= vm;
            }
#define KFSP_SLB_ENT(S, CA, CB)                                                                      \
    if (M > S) {                                                                                     \
        _Pragma("unroll") for (int j = 0; j < PER; ++j) {                                            \
            constexpr int e = (M > S ? S : 0) * PER;                                                 \
            const int ma = __builtin_amdgcn_sbfe(va0, e + j, 1), mb = __builtin_amdgcn_sbfe(vb0, e + j, 1); \
            const unsigned ata = lds0 + (unsigned)(8 * CA + R.koff8[M > S ? S : 0][j]);              \
            const unsigned atb = lds0 + (unsigned)(8 * CB + R.koff8[M > S ? S : 0][j]);              \
            ta[e + j] = *(const __attribute__((address_space(3))) double *)(size_t)((ma & ata) | (~ma & lds0)); \
            tb[e + j] = *(const __attribute__((address_space(3))) double *)(size_t)((mb & atb) | (~mb & lds0)); \
            off[e + j] = (ma | mb) ? voff + (unsigned)R.delta8[M > S ? S : 0][j] : voff;             \
        }                                                                                            \
    }
            KFSP_SLB_ENT(0, c0, b0)
            KFSP_SLB_ENT(1, c1, b1)
            KFSP_SLB_ENT(2, c2, b2)
            KFSP_SLB_ENT(3, c3, b3)
#undef KFSP_SLB_ENT
        }
        // ---- the walk over the planes, all wavefronts of the workgroup in step
        uint64_t xb = reinterpret_cast<uint64_t>(a.xg + (int64_t)(sl < lines ? sl : 0) * line_rows + (ct << 7)) - (uint64_t)(int64_t)R.bias8;
        box_pair_t xprev = {0.0, 0.0}, xcur = {0.0, 0.0}, xnext = {0.0, 0.0};
        if (live) {
            const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                                       (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
            xcur = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + voff);
        }
        int64_t row = (int64_t)sl * line_rows + r0;
        for (int p = 0; p < planes; ++p) {
            box_pair_t *buf = xchg + (size_t)(p & 1) * (size_t)W * 64;
            buf[wave * 64 + lane] = xcur;
            __syncthreads();
            if (live) {
                const global_bytes_t xw = (global_bytes_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb) |
                                                           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xb >> 32)) << 32);
                if (p + 1 < planes) xnext = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + plane_bytes + voff);
                const lds_bytes_t fl = lds + R.df8[L] + 16 * p;
                const double dsl = *(const __attribute__((address_space(3))) double *)fl;
                const unsigned vl = *(const __attribute__((address_space(3))) unsigned *)(fl + 8);
                double acca = 0.0, accb = 0.0;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    if (SIMPLE) {
                        const box_pair_t xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + off[e]);
                        acca += ta[e] * xv.x;
                        accb += tb[e] * xv.y;
                    } else {
                        const bool here = (vl >> e) & 1u;
                        const box_pair_t xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + (here ? off[e] : voff));
                        acca += (here ? ta[e] : 0.0) * xv.x;
                        accb += (here ? tb[e] : 0.0) * xv.y;
                    }
                }
                // the second-slowest species' entries: its population is this wavefront's line, so the table value is uniform;
                // an entry that moves only this species by one reads the pair of the wavefront one line down / up - from LDS
                // when that line is in this workgroup, else from memory (as format 4 does for every entry)
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int ma = __builtin_amdgcn_sbfe(va0 & vl, M * PER + j, 1), mb = __builtin_amdgcn_sbfe(vb0 & vl, M * PER + j, 1);
                    const unsigned at = lds0 + (unsigned)(8 * sl + R.koff8[M][j]);
                    const double a1a = *(const __attribute__((address_space(3))) double *)(size_t)((ma & at) | (~ma & lds0));
                    const double a1b = *(const __attribute__((address_space(3))) double *)(size_t)((mb & at) | (~mb & lds0));
                    const int d = R.delta8[M][j];
                    box_pair_t xv;
                    if ((int64_t)d == line_bytes && wave + 1 < W) xv = buf[(wave + 1) * 64 + lane];
                    else if ((int64_t)d == -line_bytes && wave > 0) xv = buf[(wave - 1) * 64 + lane];
                    else xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + ((ma | mb) ? voff + (unsigned)d : voff));
                    if (!(ma | mb)) xv = xcur;
                    acca += a1a * xv.x;
                    accb += a1b * xv.y;
                }
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int ma = __builtin_amdgcn_sbfe(va0 & vl, L * PER + j, 1), mb = __builtin_amdgcn_sbfe(vb0 & vl, L * PER + j, 1);
                    const unsigned at = lds0 + (unsigned)(8 * p + R.koff8[L][j]);
                    const double a1a = *(const __attribute__((address_space(3))) double *)(size_t)((ma & at) | (~ma & lds0));
                    const double a1b = *(const __attribute__((address_space(3))) double *)(size_t)((mb & at) | (~mb & lds0));
                    const int d = R.delta8[L][j];
                    box_pair_t xv;
                    if ((int64_t)d == plane_bytes) xv = xnext;
                    else if ((int64_t)d == -plane_bytes) xv = xprev;
                    else xv = *(const __attribute__((address_space(1), aligned(8))) box_pair_t *)(xw + ((ma | mb) ? voff + (unsigned)d : voff));
                    if (!(ma | mb)) xv = xcur;
                    acca += a1a * xv.x;
                    accb += a1b * xv.y;
                }
                d2 sum;
                sum.x = acca - (dsa0 + dsl) * xcur.x;
                sum.y = accb - (dsb0 + dsl) * xcur.y;
                if (MODE != 0) {
                    sum.x *= s;
                    sum.y *= s;
                }
                *reinterpret_cast<d2 *>(a.y + row) = sum;
                if (MODE == 1 || MODE == 3) {
                    const d2 u = *reinterpret_cast<const d2 *>(a.udot + row);
                    acc += u.x * sum.x;
                    acc += u.y * sum.y;
                }
                if (MODE == 2) {
                    acc += sum.x * sum.x;
                    acc += sum.y * sum.y;
                }
                if (MODE == 3) {
                    const d2 u = *reinterpret_cast<const d2 *>(a.udot2 + row);
                    acc2 += u.x * sum.x;
                    acc2 += u.y * sum.y;
                }
                xprev = xcur;
                xcur = xnext;
            }
            xb += (uint64_t)plane_bytes;
            row += plane_rows;
        }
        __syncthreads();                        // (the next slab's first step writes the buffer the last step may still be read from)
    }
    if (MODE != 0) {
        // W wavefront sums, added in wavefront order by every thread: one partial per workgroup
        __shared__ double wred[2 * 16];   // (W <= 12)
        acc = wave_allreduce_sum(acc);
        acc2 = wave_allreduce_sum(acc2);
        if (lane == 0) {
            wred[wave] = acc;
            wred[16 + wave] = acc2;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0, t2 = 0.0;
            for (int w = 0; w < W; ++w) {
                t += wred[w];
                t2 += wred[16 + w];
            }
            a.partial[blockIdx.x] = t;
            if (MODE == 3) a.partial2[blockIdx.x] = t2;
        }
    }
}

// format 8: waves = wavefronts per workgroup (<= 12: three per SIMD, 170 vector registers each); lds_bytes = table image (rounded to 16 B) + 2 x waves x 1 KB
void launch_spmv_slab(int mode, int grid, int waves, const SpmvArgs &a, hipStream_t st, size_t lds_bytes, int64_t plane_rows, int planes,
                      int64_t line_rows, int lines, int groups, int64_t lo_trips, bool simple)
{
    const auto fn = dispatch_mode(mode, [&](auto M) {
        return dispatch_bool(simple, [&](auto SIMPLE) {
            return dispatch_box_walk_inst(a.B.pad, [](auto NS, auto PER) {
                return k_spmv_slab<decltype(M)::value, decltype(NS)::value, decltype(PER)::value, decltype(SIMPLE)::value>;
            });
        });
    });
    hipLaunchKernelGGL(fn, dim3(grid), dim3(64 * waves), lds_bytes, st, a, plane_rows, planes, line_rows, lines, groups, lo_trips);
}

}  // namespace kfsp
