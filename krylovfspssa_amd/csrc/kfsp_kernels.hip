// gfx950 (MI355X, CDNA4) kernels of the exp(tA)v hot path.
//
// Everything here is bandwidth-bound f64 streaming (<= 0.17 flop/byte), so the
// design rules are: every HBM byte read once and in full 64-lane-wide
// contiguous pieces, the per-row scalar work fused into the pass that already
// holds the row, reductions finished by wavefront shuffles + one LDS hop, and
// no atomics (block partials in a fixed layout, summed by the consumer in a
// fixed order -> bit-reproducible runs).  No MFMA: there is no contraction.
//
// Reference call sites covered (voduchuy/KrylovFspSsa, src/fsp/KrylovSolver.f90):
//   k_spmv          FMATVEC :577-607 (as a row gather) fused with the first
//                   DDOT :243, or with the DNRM2 of :263, and with the DSCAL
//                   :258 of the source column (lazy normalisation)
//   k_ortho         DAXPY :244 fused with the next DDOT :243 / DNRM2 :247
//   k_ortho2        both DDOT/DAXPY pairs of an IOP(2) column + DNRM2 in one pass
//   k_combine       DGEMV :444 + clamp :447-449 + DASUM :450
//   k_copy_nrm2     DCOPY :176 / v1 = w/beta :223-226 + DNRM2 :177,:540
#include "kfsp_dispatch.h"
#include "kfsp_spmv_dev.h"

namespace kfsp {

// formats 0 - 5: the stored generators 0, 1, 2 and 5, the matrix-free box 3 (lds_bytes: its factor tables) and its
// single-factor form 4 by a.B.pad = species count of the instantiation * 16 + slots per species (box_plan, kfsp_box_plan.h);
// the coded banded kernels, fmt 9, are instantiated in kfsp_spmv_diac.hip
void launch_spmv(int mode, int grid, const SpmvArgs &a, const ProductKernel &k, hipStream_t st)
{
    if (k.fmt == 9) return launch_spmv_coded(mode, grid, a, k.nt, k.coded, st);
    const SpmvFn fn = dispatch_mode(mode, [&](auto M) -> SpmvFn {
        constexpr int MODE = decltype(M)::value;
        if (k.fmt == 3) return k_spmv<MODE, false, 3>;
        if (k.fmt == 4) return dispatch_box_inst(a.B.pad, [](auto NS, auto PER) -> SpmvFn { return k_spmv<MODE, false, 4, decltype(NS)::value, decltype(PER)::value>; });
        return dispatch_bool(k.nt, [&](auto NT) -> SpmvFn {
            constexpr bool T = decltype(NT)::value;
            switch (k.fmt) {
            case 2: return k_spmv<MODE, T, 2>;
            case 1: return k_spmv<MODE, T, 1>;
            case 5: return k_spmv<MODE, T, 5>;
            default: return k_spmv<MODE, T, 0>;
            }
        });
    });
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kBlock), k.fmt == 3 || k.fmt == 4 ? k.lds_bytes : 0, st, a);
}

// --------------------------------------------------- orthogonalisation step
// h = (u_i . w) s_i ;  w -= h s_i u_i ;  partial = unext . w  (or w . w)
__global__ __launch_bounds__(kBlock) void k_ortho(OrthoArgs a)
{
    __shared__ double red[4];
    if (*a.brk_flag) return;
    const double si = 1.0 / sqrt(*a.sq_i);
    const double h = finish_sum(a.dot, red) * si;
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.h_out = h;
    const double coef = h * si;
    double2 *w2 = reinterpret_cast<double2 *>(a.w);
    const double2 *u2 = reinterpret_cast<const double2 *>(a.ui);
    const double2 *n2 = reinterpret_cast<const double2 *>(a.unext);
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.npairs; i += (int64_t)gridDim.x * kBlock) {
        double2 w = w2[i];
        const double2 u = u2[i];
        w.x -= coef * u.x;
        w.y -= coef * u.y;
        w2[i] = w;
        if (n2) {
            const double2 v = n2[i];
            acc += v.x * w.x;
            acc += v.y * w.y;
        } else {
            acc += w.x * w.x;
            acc += w.y * w.y;
        }
    }
    const double t = block_allreduce_sum(acc, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

void launch_ortho(int grid, const OrthoArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_ortho, dim3(grid), dim3(kBlock), 0, st, a);
}

// both updates of an IOP(2) column in one pass (see Ortho2Args)
__global__ __launch_bounds__(kBlock) void k_ortho2(Ortho2Args a)
{
    __shared__ double red[12];
    if (*a.brk_flag) return;
    double2 *w2 = reinterpret_cast<double2 *>(a.w);
    const double2 *p1 = reinterpret_cast<const double2 *>(a.u1);
    const double2 *p2 = reinterpret_cast<const double2 *>(a.u2);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // first trip's operands are requested before the scalars are finished, so
    // the partial-sum round trip overlaps the first vector loads
    const bool have0 = i < a.npairs, have1 = i + stride < a.npairs;
    const double2 zero = make_double2(0.0, 0.0);
    double2 wa = have0 ? w2[i] : zero, wb = have1 ? w2[i + stride] : zero;
    double2 ya = have0 ? p2[i] : zero, yb = have1 ? p2[i + stride] : zero;
    double2 xa = zero, xb = zero;
    if (p1) {
        xa = have0 ? p1[i] : zero;
        xb = have1 ? p1[i + stride] : zero;
    }

    const double s2 = 1.0 / sqrt(*a.sq2);
    double c1 = 0.0, h1 = 0.0, h2;
    if (a.u1) {
        const double s1 = 1.0 / sqrt(*a.sq1);
        double sa, sb, g;
        finish_sum3(a.a, a.b, a.g, sa, sb, g, red);
        h1 = sa * s1;
        c1 = h1 * s1;
        h2 = (sb - c1 * g) * s2;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            *a.h1_out = h1;
            if (a.g_final) *a.g_final = g;
        }
    } else {
        h2 = finish_sum(a.b, red) * s2;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.h2_out = h2;
    const double c2 = h2 * s2;
    double asq = 0.0, ag = 0.0;
    for (;;) {
        wa.x -= c1 * xa.x; wa.y -= c1 * xa.y;
        wb.x -= c1 * xb.x; wb.y -= c1 * xb.y;
        wa.x -= c2 * ya.x; wa.y -= c2 * ya.y;
        wb.x -= c2 * yb.x; wb.y -= c2 * yb.y;
        if (have0) w2[i] = wa;
        if (i + stride < a.npairs) w2[i + stride] = wb;
        asq += wa.x * wa.x; asq += wa.y * wa.y;
        asq += wb.x * wb.x; asq += wb.y * wb.y;
        ag += wa.x * ya.x; ag += wa.y * ya.y;
        ag += wb.x * yb.x; ag += wb.y * yb.y;
        i += 2 * stride;
        if (i >= a.npairs) break;
        const bool h1b = i + stride < a.npairs;
        wa = w2[i];
        ya = p2[i];
        wb = h1b ? w2[i + stride] : zero;
        yb = h1b ? p2[i + stride] : zero;
        if (p1) {
            xa = p1[i];
            xb = h1b ? p1[i + stride] : zero;
        }
    }
    double dummy = 0.0;
    block_allreduce_sum3(asq, ag, dummy, red);
    if (threadIdx.x == 0) {
        a.partial_sq[blockIdx.x] = asq;
        a.partial_g[blockIdx.x] = ag;
    }
}

void launch_ortho2(int grid, const Ortho2Args &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_ortho2, dim3(grid), dim3(kBlock), 0, st, a);
}

__global__ __launch_bounds__(kBlock) void k_pass_reset(double *__restrict__ H, int count, int *__restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < count) H[i] = 0.0;
    if (i == 0) *flag = 0;
}

void launch_pass_reset(double *H, int count, int *flag, hipStream_t st)
{
    hipLaunchKernelGGL(k_pass_reset, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, H, count, flag);
}

// ----------------------------------------------- small-N Arnoldi pass, one launch
// One workgroup of 1024 lanes owns every row (<= 4 per lane).  Columns are
// separated by workgroup barriers instead of kernel boundaries, the current
// source vector lives in LDS (32 KB: the x gathers of the product never leave
// the CU), each lane keeps its own rows of the new column in registers between
// the product and the update, and scalars never leave registers.  Per column
// the only global round trip left is the stream of generator entries.  H, the
// squared norms and the breakdown flag are written exactly as the multi-launch
// path writes them, so the host side is unchanged.
constexpr int kSmallBlock = 1024;
constexpr int kSmallTrips = kSmallRows / kSmallBlock;      // rows per lane

// Two block sums with ONE barrier: the caller alternates between the two halves of
// red (64 doubles), so a half is rewritten only after another barrier has separated
// the writers from the last readers.
__device__ __forceinline__ void small_reduce2(double &a, double &b, double *red_half)
{
    a = wave_allreduce_sum(a);
    b = wave_allreduce_sum(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red_half[wave] = a;
        red_half[16 + wave] = b;
    }
    __syncthreads();
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int w = 0; w < kSmallBlock / 64; ++w) {
        sa += red_half[w];
        sb += red_half[16 + w];
    }
    a = sa;
    b = sb;
}

__device__ __forceinline__ double row_dia1(const DiaDev &D, const double *x, int64_t r)
{
    const int64_t last = D.n - 1;
    double sum = -D.diag[r] * x[r < last ? r : last];
    for (int d = 0; d < D.nd; ++d) {
        int64_t i = r + D.delta[d];
        i = i < 0 ? 0 : (i > last ? last : i);
        sum += D.val[(int64_t)d * D.ld + r] * x[i];
    }
    return sum;
}

// row t of this lane: SELL lanes own (chunk = wave + 16 t, lane), DIA lanes own tid + 1024 t
template <bool DIA>
__device__ __forceinline__ int64_t small_row(int t)
{
    if (DIA) return (int64_t)threadIdx.x + (int64_t)t * kSmallBlock;
    return (((int64_t)(threadIdx.x >> 6) + (int64_t)t * (kSmallBlock / 64)) << 6) + (threadIdx.x & 63);
}

// SELL row with the chunk's offset and width already in registers (they do not
// change from column to column, so the dependent off[] load is paid once per pass)
__device__ __forceinline__ double row_sell_pre(const SellDev &A, const double *xs, int64_t r, int64_t off, int w,
                                               double dg)
{
    const int lane = (int)(r & 63);
    const int32_t *cp = A.col + off + 2 * lane;
    const double *vp = A.val + off + 2 * lane;
    double sum = -dg * xs[r];
    for (int k = 0; k < (w >> 1); ++k) {                  // slot pairs (sell_pos)
        const i2 c0 = *reinterpret_cast<const i2 *>(cp + k * 128);
        const d2 v0 = *reinterpret_cast<const d2 *>(vp + k * 128);
        sum += v0.x * xs[c0.x];
        sum += v0.y * xs[c0.y];
    }
    if (w & 1) sum += A.val[off + (w >> 1) * 128 + lane] * xs[A.col[off + (w >> 1) * 128 + lane]];
    return sum;
}

// the same with the chunk's slots copied to LDS (values, and columns as 16-bit numbers:
// there are at most 4096 rows)
__device__ __forceinline__ double row_sell_lds(const double *vs, const unsigned short *cs, double dg,
                                               const double *xs, int64_t r, int64_t off, int w)
{
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const int lane = (int)(r & 63);
    const unsigned short *cp = cs + off + 2 * lane;
    const double *vp = vs + off + 2 * lane;
    double sum = -dg * xs[r];
    for (int k = 0; k < (w >> 1); ++k) {
        const us2 c0 = *reinterpret_cast<const us2 *>(cp + k * 128);
        const d2 v0 = *reinterpret_cast<const d2 *>(vp + k * 128);
        sum += v0.x * xs[c0.x];
        sum += v0.y * xs[c0.y];
    }
    if (w & 1) sum += vs[off + (w >> 1) * 128 + lane] * xs[cs[off + (w >> 1) * 128 + lane]];
    return sum;
}

// FMT: 0 SELL from global memory, 1 banded, 2 SELL from LDS
template <int FMT>
__device__ __forceinline__ double small_product_row(const SmallArnoldiArgs &a, const double *xs, const double *vs,
                                                    const unsigned short *cs, int64_t r, int64_t off, int w, double dg)
{
    if (FMT == 1) return row_dia1(a.D, xs, r);
    if (FMT == 2) return row_sell_lds(vs, cs, dg, xs, r, off, w);
    return row_sell_pre(a.A, xs, r, off, w, dg);
}

// Where the scalars of a pass go.  The single-vector pass writes the H image, the squared norms and the breakdown flag
// of the multi-launch path (kfsp_arnoldi copies them out).
struct SmallSinkSingle {
    double *sq, *gfin, *Hd;
    int *brk_flag;
    int jold, m;
    // what is known about column jold: ||u_jold||^2, u_jold . u_{jold-1}, 1/||u_{jold-1}|| (carried in a register)
    __device__ __forceinline__ void start(double &S, double &g, double &s1) const
    {
        S = sq[jold];
        g = gfin[jold];
        s1 = jold >= 2 ? 1.0 / sqrt(sq[jold - 1]) : 0.0;
    }
    // column j is about to be multiplied: S = ||u_j||^2
    __device__ __forceinline__ void column(int j, double S, double nrm) const
    {
        sq[j] = S;
        if (j > jold) Hd[(size_t)(j - 2) * kMH + (j - 1)] = nrm;           // H(j,j-1)
    }
    __device__ __forceinline__ void h1(int j, double h, double g) const
    {
        Hd[(size_t)(j - 1) * kMH + (j - 2)] = h;                           // H(j-1,j)
        gfin[j] = g;
    }
    __device__ __forceinline__ void h2(int j, double h) const { Hd[(size_t)(j - 1) * kMH + (j - 1)] = h; }   // H(j,j)
    // the column behind the loop (jl = m + 1 when the loop ran)
    __device__ __forceinline__ void last(int jl, bool looped, double S, double nrm, double g) const
    {
        sq[jl] = S;
        if (looped) {
            Hd[(size_t)(m - 1) * kMH + m] = nrm;                           // H(m+1,m)
            gfin[m + 1] = g;
        }
    }
    __device__ __forceinline__ void broke(int) const { *brk_flag = 1; }
    __device__ __forceinline__ void avnorm(double av) const
    {
        Hd[(size_t)kMH * kMH] = av;
        Hd[(size_t)kMH * kMH + 1] = sqrt(av);
    }
};

// The block pass (kfsp_block.hip) keeps per column what block_arnoldi copies out of d_bscal: entry c of rows of sk.
struct SmallSinkBlock {
    double *hb, *nrm, *brk, *avn;      // already offset by the column
    int sk;
    double S1;                         // ||u_1||^2
    __device__ __forceinline__ void start(double &S, double &g, double &s1) const
    {
        S = S1;
        g = s1 = 0.0;
    }
    __device__ __forceinline__ void column(int j, double, double n) const
    {
        nrm[(size_t)j * sk] = n;
        if (j > 1) hb[(size_t)((j - 1) * 3 + 2) * sk] = n;                 // H(j,j-1)
    }
    __device__ __forceinline__ void h1(int j, double h, double) const { hb[(size_t)(j * 3) * sk] = h; }
    __device__ __forceinline__ void h2(int j, double h) const { hb[(size_t)(j * 3 + 1) * sk] = h; }
    __device__ __forceinline__ void last(int jl, bool, double S, double n, double) const { column(jl, S, n); }
    __device__ __forceinline__ void broke(int j) const { *brk = (double)j; }
    __device__ __forceinline__ void avnorm(double av) const { *avn = sqrt(av); }
};

// The pass itself, shared by the single-vector kernel (one workgroup, STRIDED = false: rows are contiguous) and the
// block kernel (one workgroup per block column, rows es doubles apart): the same source lines under the same
// contraction setting, so a column's H, norms and AVNORM are the same bits on both.  V is column 0 of the basis (u_1).
// Returns 0, or j when H(j+1,j) <= break_tol ended the pass (uniform over the workgroup).
template <int FMT, bool STRIDED, class SINK>
__device__ __forceinline__ int small_pass(const SmallArnoldiArgs &a, double *V, int64_t es_in, const SINK &sink)
{
    constexpr bool DIA = FMT == 1;
    // element of row r in a basis column; a block column has at most kSmallRows rows of at most 16 doubles: 32 bits do,
    // and so do the chunk offsets of its generator (launch_barnoldi_small's caller checks the slots)
    auto at = [&](int64_t r) -> int64_t { return STRIDED ? (int64_t)((int)r * (int)es_in) : r; };
    typedef typename std::conditional<STRIDED, int, int64_t>::type chunk_off_t;
    // dynamic LDS: the source column u_j [nact doubles]; FMT 2 also the generator's slots
    // [slots doubles | slots 16-bit columns]
    extern __shared__ double dyn_lds[];
    double *xs = dyn_lds;
    double *vs = dyn_lds + a.nact;
    unsigned short *cs = reinterpret_cast<unsigned short *>(vs + (FMT == 2 ? a.slots : 0));
    __shared__ double red[64];
    int rb = 0;                                        // which half of red the next reduction uses
    const int tid = threadIdx.x;
    if (FMT == 2) {
        for (int64_t i = tid; i < a.slots; i += kSmallBlock) {
            vs[i] = a.A.val[i];
            cs[i] = (unsigned short)a.A.col[i];
        }
    }
    double S, g, s1;
    sink.start(S, g, s1);
    chunk_off_t offs[kSmallTrips];
    int wid[kSmallTrips];
    double dg[kSmallTrips];                            // DIAG of this lane's rows: the same in every column
#pragma unroll
    for (int t = 0; t < kSmallTrips; ++t) {
        const int64_t r = small_row<DIA>(t);
        offs[t] = 0;
        wid[t] = 0;
        dg[t] = 0.0;
        if (!DIA && r < a.nact) {
            offs[t] = (chunk_off_t)a.A.off[r >> 6];
            wid[t] = (int)((a.A.off[(r >> 6) + 1] - offs[t]) >> 6);
            dg[t] = a.A.diag[r];
        }
        if (STRIDED) {                   // a wavefront's lanes share the chunk: scalar registers, the 128 vector ones are short
            offs[t] = (chunk_off_t)__builtin_amdgcn_readfirstlane((int)offs[t]);
            wid[t] = __builtin_amdgcn_readfirstlane(wid[t]);
        }
    }
    {
        const double *src = V + (size_t)(a.jold - 1) * a.ldv;
        for (int64_t r = tid; r < a.nact; r += kSmallBlock) xs[r] = src[at(r)];
    }
    __syncthreads();
    int broke = 0;
    // u_{j-1} on this lane's rows: read once for the first column, then carried over (it is
    // the source column of the previous iteration)
    double v1[kSmallTrips];
#pragma unroll
    for (int t = 0; t < kSmallTrips; ++t) {
        const int64_t r = small_row<DIA>(t);
        v1[t] = (a.jold >= 2 && r < a.nact) ? V[(size_t)(a.jold - 2) * a.ldv + at(r)] : 0.0;
    }
    for (int j = a.jold; j <= a.m; ++j) {
        const bool u1 = j >= 2;
        double *dst = V + (size_t)j * a.ldv;
        const double nrm = sqrt(S);
        if (tid == 0) sink.column(j, S, nrm);
        if (j > a.jold && !(nrm > a.break_tol)) {      // happy breakdown :249 (S is the same in every lane)
            broke = j - 1;
            break;
        }
        const double s2 = 1.0 / nrm;
        double y[kSmallTrips];
        double pa = 0.0, pb = 0.0;
#pragma unroll
        for (int t = 0; t < kSmallTrips; ++t) {
            const int64_t r = small_row<DIA>(t);
            y[t] = 0.0;
            if (r < a.nact) {
                y[t] = s2 * small_product_row<FMT>(a, xs, vs, cs, r, offs[t], wid[t], dg[t]);
                pa += v1[t] * y[t];
                pb += xs[r] * y[t];
            }
        }
        small_reduce2(pa, pb, red + rb);                // (also: every lane is past its gathers from xs)
        rb ^= 32;
        double c1 = 0.0, h2;
        if (u1) {
            const double h1 = pa * s1;
            c1 = h1 * s1;
            h2 = (pb - c1 * g) * s2;
            if (tid == 0) sink.h1(j, h1, g);
        } else {
            h2 = pb * s2;
        }
        if (tid == 0) sink.h2(j, h2);
        const double c2 = h2 * s2;
        double asq = 0.0, ag = 0.0;
#pragma unroll
        for (int t = 0; t < kSmallTrips; ++t) {
            const int64_t r = small_row<DIA>(t);
            if (r < a.nact) {
                const double v2 = xs[r];
                const double w = y[t] - c1 * v1[t] - c2 * v2;
                v1[t] = v2;              // next column's u_{j-1}
                dst[at(r)] = w;
                xs[r] = w;               // own rows only; nobody gathers before the barrier below
                asq += w * w;
                ag += w * v2;
            }
        }
        small_reduce2(asq, ag, red + rb);               // its barrier also publishes the new source column
        rb ^= 32;
        S = asq;
        g = ag;
        s1 = s2;
    }
    if (broke) {
        if (tid == 0) sink.broke(broke);
        return broke;
    }
    // the extra product for AVNORM (:261-263); from column jold when the loop did not run
    const bool looped = a.jold <= a.m;
    const int jl = looped ? a.m + 1 : a.jold;
    double *dst = V + (size_t)jl * a.ldv;
    const double nrm = sqrt(S);
    if (tid == 0) sink.last(jl, looped, S, nrm, g);
    if (looped && !(nrm > a.break_tol)) {
        if (tid == 0) sink.broke(a.m);
        return a.m;
    }
    const double s2 = 1.0 / nrm;
    double av = 0.0, dummy = 0.0;
#pragma unroll
    for (int t = 0; t < kSmallTrips; ++t) {
        const int64_t r = small_row<DIA>(t);
        if (r < a.nact) {
            const double yv = s2 * small_product_row<FMT>(a, xs, vs, cs, r, offs[t], wid[t], dg[t]);
            dst[at(r)] = yv;
            av += yv * yv;
        }
    }
    small_reduce2(av, dummy, red + rb);
    if (tid == 0) sink.avnorm(av);
    return 0;
}

template <int FMT>
__global__ __launch_bounds__(kSmallBlock) void k_arnoldi_small(SmallArnoldiArgs a)
{
    const SmallSinkSingle sink{a.sq, a.gfin, a.Hd, a.brk_flag, a.jold, a.m};
    small_pass<FMT, false>(a, a.V, 1, sink);
}

// The block pass: workgroup c runs the whole pass of block column c (row r of column j at V[j ldv + r es + c]).  Its
// scalars are cleared first (a column that stops early leaves zeros behind it, as the multi-launch path does), and so
// are the basis columns the pass does not reach: u_2 .. u_{m+2} of a skipped (beta = 0) or padding column, the columns
// behind a breakdown.  Only rows below nact are touched.
template <int FMT>
__global__ __launch_bounds__(kSmallBlock) void k_barnoldi_small(SmallArnoldiArgs a, SmallBlockArgs b)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    double *V = b.V + c;
    const SmallSinkBlock sink{b.hb + c, b.nrm + c, b.brk + c, b.avn + c, b.sk, b.sq1[c]};
    const bool skip = c >= b.k || b.brk[c] != 0.0;
    for (int i = 3 + tid; i < (a.m + 2) * 3; i += kSmallBlock) sink.hb[(size_t)i * b.sk] = 0.0;
    for (int i = 2 + tid; i <= a.m + 2; i += kSmallBlock) sink.nrm[(size_t)i * b.sk] = 0.0;
    if (tid == 0) *sink.avn = 0.0;
    __syncthreads();
    const int jb = skip ? 0 : small_pass<FMT, true>(a, V, b.es, sink);
    if (!skip && jb == 0) return;
    for (int j = jb + 2; j <= a.m + 2; ++j) {
        double *col = V + (size_t)(j - 1) * a.ldv;
        for (int64_t r = tid; r < a.nact; r += kSmallBlock) col[r * b.es] = 0.0;
    }
}

// bytes of dynamic LDS the generator-in-LDS variant needs
size_t small_lds_bytes(int64_t nact, int64_t slots, bool with_matrix)
{
    return (size_t)nact * 8 + (with_matrix ? (size_t)slots * 10 + 16 : 0);
}

int launch_arnoldi_small(const SmallArnoldiArgs &a, bool dia, int64_t lds_limit, hipStream_t st)
{
    static bool raised = false;
    const size_t want = small_lds_bytes(a.nact, a.slots, true);
    const bool lmat = !dia && a.slots > 0 && (int64_t)want + 512 <= lds_limit;
    if (lmat && !raised) {
        // more than the default 64 KiB of dynamic LDS has to be asked for once per kernel
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_arnoldi_small<2>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit - 512);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    if (dia) hipLaunchKernelGGL((k_arnoldi_small<1>), dim3(1), dim3(kSmallBlock), small_lds_bytes(a.nact, 0, false), st, a);
    else if (lmat) hipLaunchKernelGGL((k_arnoldi_small<2>), dim3(1), dim3(kSmallBlock), want, st, a);
    else hipLaunchKernelGGL((k_arnoldi_small<0>), dim3(1), dim3(kSmallBlock), small_lds_bytes(a.nact, 0, false), st, a);
    return 0;
}

int launch_barnoldi_small(const SmallArnoldiArgs &a, const SmallBlockArgs &b, int kp, bool dia, int64_t lds_limit, hipStream_t st,
                          int *fmt, size_t *lds)
{
    static bool raised = false;
    const size_t want = small_lds_bytes(a.nact, a.slots, true);
    const bool lmat = !dia && a.slots > 0 && (int64_t)want + 512 <= lds_limit;
    if (lmat && !raised) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_barnoldi_small<2>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit - 512);
        if (e != hipSuccess) return (int)e;
        raised = true;
    }
    *fmt = dia ? 1 : (lmat ? 2 : 0);
    *lds = lmat ? want : small_lds_bytes(a.nact, 0, false);
    if (dia) hipLaunchKernelGGL((k_barnoldi_small<1>), dim3(kp), dim3(kSmallBlock), *lds, st, a, b);
    else if (lmat) hipLaunchKernelGGL((k_barnoldi_small<2>), dim3(kp), dim3(kSmallBlock), *lds, st, a, b);
    else hipLaunchKernelGGL((k_barnoldi_small<0>), dim3(kp), dim3(kSmallBlock), *lds, st, a, b);
    return 0;
}

// ------------------------------------------------------------------ combine
// w = beta * sum_j y_j s_j u_j ; clamp ; partial = sum |w|
__global__ __launch_bounds__(kBlock) void k_combine(CombineArgs a)
{
    __shared__ double red[4];
    __shared__ double coef[kMH];
    for (int j = threadIdx.x; j < a.mx; j += kBlock)
        coef[j] = a.beta * a.y[j] / sqrt(a.sq[j + 1]);
    __syncthreads();
    double2 *w2 = reinterpret_cast<double2 *>(a.w);
    const int64_t ld2 = a.ldv >> 1;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.npairs; i += (int64_t)gridDim.x * kBlock) {
        const double2 *v = reinterpret_cast<const double2 *>(a.V) + i;
        double sx = 0.0, sy = 0.0;
        int j = 0;
        for (; j + 4 <= a.mx; j += 4) {
            const double2 v0 = v[(int64_t)(j + 0) * ld2], v1 = v[(int64_t)(j + 1) * ld2];
            const double2 v2 = v[(int64_t)(j + 2) * ld2], v3 = v[(int64_t)(j + 3) * ld2];
            sx += coef[j] * v0.x; sy += coef[j] * v0.y;
            sx += coef[j + 1] * v1.x; sy += coef[j + 1] * v1.y;
            sx += coef[j + 2] * v2.x; sy += coef[j + 2] * v2.y;
            sx += coef[j + 3] * v3.x; sy += coef[j + 3] * v3.y;
        }
        for (; j < a.mx; ++j) {
            const double2 vj = v[(int64_t)j * ld2];
            sx += coef[j] * vj.x; sy += coef[j] * vj.y;
        }
        sx = sx < 0.0 ? 0.0 : sx;       // FSP non-negativity :447-449 (NaN stays NaN)
        sy = sy < 0.0 ? 0.0 : sy;
        w2[i] = make_double2(sx, sy);
        acc += fabs(sx);
        acc += fabs(sy);
    }
    const double t = block_allreduce_sum(acc, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

void launch_combine(int grid, const CombineArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_combine, dim3(grid), dim3(kBlock), 0, st, a);
}

// --------------------------------------------------------- small streaming ops
__global__ __launch_bounds__(kBlock) void k_copy_nrm2(int64_t npairs, const double2 *__restrict__ w,
                                                      double2 *__restrict__ u, double *__restrict__ partial)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        const double2 v = w[i];
        u[i] = v;
        acc += v.x * v.x;
        acc += v.y * v.y;
    }
    const double t = block_allreduce_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

void launch_copy_nrm2(int grid, int64_t npairs, const double *w, double *u1, double *partial, hipStream_t st)
{
    hipLaunchKernelGGL(k_copy_nrm2, dim3(grid), dim3(kBlock), 0, st, npairs,
                       reinterpret_cast<const double2 *>(w), reinterpret_cast<double2 *>(u1), partial);
}

__global__ __launch_bounds__(kBlock) void k_reduce(int64_t npairs, const double2 *__restrict__ w, int squared,
                                                   double *__restrict__ partial)
{
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        const double2 v = w[i];
        if (squared) {
            acc += v.x * v.x;
            acc += v.y * v.y;
        } else {
            acc += fabs(v.x);
            acc += fabs(v.y);
        }
    }
    const double t = block_allreduce_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

void launch_reduce(int grid, int64_t npairs, const double *w, int squared, double *partial, hipStream_t st)
{
    hipLaunchKernelGGL(k_reduce, dim3(grid), dim3(kBlock), 0, st, npairs, reinterpret_cast<const double2 *>(w),
                       squared, partial);
}

__global__ __launch_bounds__(kBlock) void k_finalize(Pending p, double *out, double *out_sqrt)
{
    __shared__ double red[4];
    const double t = finish_sum(p, red);
    if (threadIdx.x == 0) {
        if (out) *out = t;
        if (out_sqrt) *out_sqrt = sqrt(t);
    }
}

void launch_finalize(Pending p, double *out, double *out_sqrt, hipStream_t st)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(kBlock), 0, st, p, out, out_sqrt);
}

__global__ __launch_bounds__(kBlock) void k_scale_copy(int64_t npairs, const double2 *__restrict__ u,
                                                       const double *__restrict__ sq_u, double beta,
                                                       double2 *__restrict__ w)
{
    const double c = beta / sqrt(*sq_u);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < npairs; i += (int64_t)gridDim.x * kBlock) {
        const double2 v = u[i];
        w[i] = make_double2(c * v.x, c * v.y);
    }
}

void launch_scale_copy(int grid, int64_t npairs, const double *u, const double *sq_u, double beta, double *w,
                       hipStream_t st)
{
    hipLaunchKernelGGL(k_scale_copy, dim3(grid), dim3(kBlock), 0, st, npairs,
                       reinterpret_cast<const double2 *>(u), sq_u, beta, reinterpret_cast<double2 *>(w));
}

// ------------------------------------------------------- counter calibration
// Reads n elements of width W bytes per lane (4, 8 or 16) in the SpMV's own
// access shape (one contiguous 64-lane piece per wave instruction) and folds
// them into one value per block, so the traffic is exactly n*W bytes read.
template <class T>
__global__ __launch_bounds__(kBlock) void k_stream_read(int64_t n, const T *__restrict__ p, double *__restrict__ sink)
{
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const T v = __builtin_nontemporal_load(p + i);
        if constexpr (sizeof(T) == 16) acc += v.x + v.y;
        else acc += (double)v;
    }
    if (acc == 0.12345) sink[blockIdx.x] = acc;   // never true for the zero-filled buffer: keeps the loads alive
}

void launch_stream_read(int grid, int elem_bytes, int64_t nbytes, const void *p, double *sink, hipStream_t st)
{
    if (elem_bytes == 4)
        hipLaunchKernelGGL((k_stream_read<int32_t>), dim3(grid), dim3(kBlock), 0, st, nbytes / 4, (const int32_t *)p, sink);
    else if (elem_bytes == 8)
        hipLaunchKernelGGL((k_stream_read<double>), dim3(grid), dim3(kBlock), 0, st, nbytes / 8, (const double *)p, sink);
    else
        hipLaunchKernelGGL((k_stream_read<d2>), dim3(grid), dim3(kBlock), 0, st, nbytes / 16, (const d2 *)p, sink);
}

}  // namespace kfsp

