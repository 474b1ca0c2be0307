// Private: what the translation units of the block product share - kfsp_block.hip (the kernels of Y = A X and of everything
// behind the product), kfsp_block_host.hip (the host side of all of them), kfsp_block_adj.hip (Y = A^T X, option adjoint),
// kfsp_block_boxg.hip (Y = A X on any matrix-free box, option block_box = 2), kfsp_block_diac.hip (Y = A X from the coded
// banded image, option block_dia_code) and kfsp_block_diac_t.hip (Y = A^T X from it, option block_dia_code_adjoint): the row
// helpers, SpmmArgs and block_sum_cols, the layout of the per-column scalars, the descriptors of the transposed product and
// of the generic matrix-free kernels, and the selectors through which the host file reaches every kernel.
#pragma once

#include "kfsp_block.h"
#include "kfsp_dispatch.h"
#include "kfsp_internal.h"

#include <type_traits>

namespace kfsp {

typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

// ---- from run-time block widths to kernel instantiations (plain host code: tests/block_dispatch_check.cpp; the variants
// every product shares - dispatch_bool, dispatch_box_inst, dispatch_diac - are in kfsp_dispatch.h)
// log2(kp) - 1 for a block width kp in {2, 4, 8, 16}: the slot of the width in a table, and the shift from a 16-byte pair
// of a block column to its row (pair i lies in row i >> kp_index(kp))
constexpr int kp_index(int kp) { return kp == 2 ? 0 : (kp == 4 ? 1 : (kp == 8 ? 2 : 3)); }

// f(std::integral_constant<int, KP>) for the width; anything that is not 2, 4 or 8 takes 16
template <class F>
decltype(auto) dispatch_kp(int kp, F &&f)
{
    switch (kp) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
    }
}

// f(width, std::bool_constant<dots>): what nearly every product kernel is instantiated by
template <class F>
decltype(auto) dispatch_kp_dots(int kp, bool dots, F &&f)
{
    return dispatch_kp(kp, [&](auto KP) { return dots ? f(KP, std::true_type{}) : f(KP, std::false_type{}); });
}

// Where code d of a row lies in its record (DiaCodeDev, kfsp_internal.h; coded_vals, kfsp_spmv_dev.h): a 64-bit record
// word holds 64 / w codes of w bits, diagonal d in word d / (64 / w) at bit w (d mod 64 / w).  Plain code: the kernel
// and tests/block_dia_code_check.cpp read the same lines.
constexpr int diac_word(int w, int d) { return d / (64 / w); }
constexpr int diac_shift(int w, int d) { return (d % (64 / w)) * w; }
constexpr unsigned diac_mask(int w) { return (1u << w) - 1u; }
constexpr unsigned diac_code(int w, unsigned long long word, int d) { return (unsigned)(word >> diac_shift(w, d)) & diac_mask(w); }

// The transposed coded product (k_spmm_diac_t, kfsp_block_diac_t.hip): entry d of row r of A^T is A(r - delta_d, r), whose
// code lies in the record of row r - delta_d.  ok: that source is a row of the generator.  row: the source, or r itself
// when there is none - the row whose X the fma takes and whose record may be read (its code is discarded: the entry counts
// as 0.0).  word: the index in DiaCodeDev::rec of the ONE 64-bit word of that record that holds code d (rec_bytes / 8 words
// per record; a code never straddles words).  For 0 <= r < n neither index leaves the rows [0, n).  Plain code: the kernel
// and tests/block_dia_code_adjoint_check.cpp read the same lines.
struct DiacTSrc {
    bool ok;
    int64_t row, word;
};
constexpr DiacTSrc diac_t_src(int w, int rec_bytes, int64_t r, int64_t delta, int64_t n, int d)
{
    const int64_t src = r - delta;
    const bool ok = src >= 0 && src < n;
    const int64_t row = ok ? src : r;
    return DiacTSrc{ok, row, (int64_t)(rec_bytes / 8) * row + diac_word(w, d)};
}

#if defined(__HIPCC__)
template <int KP>
__device__ __forceinline__ void ld_row(const double *__restrict__ X, int64_t row, double (&x)[KP])
{
    const d2 *p = reinterpret_cast<const d2 *>(X + row * KP);
#pragma unroll
    for (int q = 0; q < KP / 2; ++q) {
        const d2 t = p[q];
        x[2 * q] = t.x;
        x[2 * q + 1] = t.y;
    }
}

template <int KP>
__device__ __forceinline__ void st_row(double *__restrict__ Y, int64_t row, const double (&s)[KP])
{
    d2 *p = reinterpret_cast<d2 *>(Y + row * KP);
#pragma unroll
    for (int q = 0; q < KP / 2; ++q) p[q] = d2{s[2 * q], s[2 * q + 1]};
}

// s = -(diag x): the single-vector kernels' v_mul_f64 of DIAG and x with the sign folded in
template <int KP>
__device__ __forceinline__ void diag_row(double dg, const double (&x)[KP], double (&s)[KP])
{
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = -(dg * x[c]);
}

// s += v x as ONE rounding per column (the single-vector kernels' v_fmac_f64)
template <int KP>
__device__ __forceinline__ void fma_row(double v, const double (&x)[KP], double (&s)[KP])
{
#pragma unroll
    for (int c = 0; c < KP; ++c) s[c] = __builtin_fma(v, x[c], s[c]);
}
#endif

struct SpmmArgs {
    SellDev A;
    DiaDev D;
    const double *X;
    double *Y;
    const double *ua, *ub;   // DOTS: partials of ua . Y (ua may be null) and ub . Y per column
    double *part;            // [2][kMaxGrid][kBlockMaxK]
    int64_t trips;
    const int32_t *trip_order;
    int64_t rows_red;        // rows that enter the reductions
    const double *box_tab;   // matrix-free box: the table image (staged to LDS), its length in doubles and the
    int box_ntab;            // single-factor descriptor behind it
    const BoxFast *box_fast;
    // Row partition (option block_partition; read by k_spmm<.., PART = true> only - the one-rank instantiations, the box
    // and the transposed kernels cover [0, trips) of one rank): rows are local, X is addressed by GLOBAL row - local
    // row r is row row0 + r of X.  The launch covers the linear trips [trip_begin, trip_end); linear trip t stands for
    // trip (t < trip_split ? t : t + trip_jump), so that one launch takes both boundary ranges of a split product
    // (SpmvArgs, kfsp_internal.h).
    int64_t row0;
    int64_t trip_begin, trip_end;
    int64_t trip_split, trip_jump;
};

#if defined(__HIPCC__)
// per-column sums of the block: v[c] summed over the wavefront, then the four wavefronts in a fixed order
template <int KP>
__device__ __forceinline__ void block_sum_cols(double (&v)[KP], double *red, double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < KP; ++c)
        for (int o = 32; o >= 1; o >>= 1) v[c] += __shfl_xor(v[c], o);
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < KP; ++c) red[wave * KP + c] = v[c];
    __syncthreads();
    if (threadIdx.x < KP) {
        const int c = threadIdx.x;
        out[c] = (red[c] + red[KP + c]) + (red[2 * KP + c] + red[3 * KP + c]);
    }
    __syncthreads();
}

// what every transposed kernel does with a finished row: store it, add it to the two dot products
template <int KP, bool DOTS>
__device__ __forceinline__ void finish_row(const SpmmArgs &a, int64_t r, const double (&s)[KP], double (&da)[KP], double (&db)[KP])
{
    st_row<KP>(a.Y, r, s);
    if (DOTS && r < a.rows_red) {
        double u[KP];
        if (a.ua) {
            ld_row<KP>(a.ua, r, u);
#pragma unroll
            for (int c = 0; c < KP; ++c) da[c] = __builtin_fma(u[c], s[c], da[c]);
        }
        ld_row<KP>(a.ub, r, u);
#pragma unroll
        for (int c = 0; c < KP; ++c) db[c] = __builtin_fma(u[c], s[c], db[c]);
    }
}
#endif

// ---- the transposed product (kfsp_block_adj.hip, kfsp_block_diac_t.hip)

// The reference arrays ADJ / OFFDIAG / DIAG as they stay on the device (kfsp_build.hip), in the order the device keeps
// its vectors: column c holds the reactions that LEAVE state c - the gather row c of A^T.
struct EllAdjDev {
    const int32_t *adj;      // [n][ld], 1-based target of slot k of state c at adj[c * ld + k]; outside [1, n]: no target
    const double *off;       // [n][ld] the propensities
    const double *diag;      // [n]
    int64_t n;
    int32_t ld, bw;
};

// Row of A^T of a single-factor box, beside BoxFast (whose image and layout stay as they are): for slot (s, j) of the
// forward form - the j-th reaction, by ascending source offset, whose propensity depends on species s - the offset of the
// propensity at the row's OWN coordinate, the X offset of the TARGET state x + nu and which coordinate tests the target
// has to pass.  Uniform kernel argument.
struct BoxAdjDev {
    int32_t aoff8[kBoxFastS][kBoxFastPer];    // byte offset in the LDS image of the slot's factor table (+ 8 x_s: a_k(x))
    int32_t tdelta8[kBoxFastS][kBoxFastPer];  // 8 * (x index of the target state relative to the row)
    uint32_t need[kBoxFastS][kBoxFastPer];    // bits the row's test word must have: bit 5 s + nu_s + 2 for every species the
                                              // reaction moves; kBoxAdjNever for an unused slot
    int32_t bias8;                            // bytes the wave's x base lies below its first row (>= the largest backward reach)
};
constexpr uint32_t kBoxAdjNever = 1u << 31;   // a bit no test word has

// Fills the descriptor from the box as kfsp_set_matrix_box stored it (reactions by ascending source offset; inst = species
// of the instantiation * 16 + slots per species, BoxDev::pad).  False: the box is not a single-factor one of that shape.
static inline bool box_adj_build(const BoxDev &B, BoxAdjDev &out)
{
    const int ns_inst = B.pad / 16, per = B.pad % 16;
    if (ns_inst < 1 || ns_inst > kBoxFastS || per < 1 || per > kBoxFastPer || B.ns < 1 || B.ns > ns_inst || B.nr < 1 ||
        B.nr > kBoxMaxR)
        return false;
    for (int s = 0; s < kBoxFastS; ++s)
        for (int j = 0; j < kBoxFastPer; ++j) {
            out.aoff8[s][j] = 0;
            out.tdelta8[s][j] = 0;
            out.need[s][j] = kBoxAdjNever;
        }
    int fill[kBoxFastS] = {0};
    int64_t fwd = 0;
    for (int p = 0; p < B.nr; ++p) {
        if (B.ndep[p] != 1) return false;
        const int s = B.dep_s[p][0];
        if (s < 0 || s >= B.ns) return false;
        const int j = fill[s]++;
        if (j >= per) return false;
        uint32_t need = 0;
        if (B.nmov[p] < 0 || B.nmov[p] > kBoxMaxDep) return false;
        for (int i = 0; i < B.nmov[p]; ++i) {
            const int ms = B.mov_s[p][i], nu = B.mov_nu[p][i];
            if (ms < 0 || ms >= B.ns || nu < -2 || nu > 2) return false;
            need |= 1u << (5 * ms + nu + 2);
        }
        out.aoff8[s][j] = 8 * B.dep_off[p][0];
        out.tdelta8[s][j] = -8 * B.delta[p];
        out.need[s][j] = need;
        fwd = B.delta[p] > fwd ? (int64_t)B.delta[p] : fwd;
    }
    out.bias8 = (int32_t)(8 * fwd);
    return true;
}

// The generic matrix-free block kernels (k_spmm_boxg / k_spmm_boxg_t, option block_box = 2) interpret BoxDev as
// kfsp_set_matrix_box stored it and index the LDS image with it: the doubles of the image they read - the head and the
// factor tables, not the single-factor form's species tables behind them - or 0 when the descriptor is not one they can
// walk without leaving the image or their registers (sizes out of range, a species or a table outside the box or the
// image, dorder no permutation of the sorted positions, a stoichiometry that does not match between the factor and the
// move lists).
static inline int32_t box_generic_image(const BoxDev &B)
{
    if (B.ns < 1 || B.ns > kBoxMaxS || B.nr < 1 || B.nr > kBoxMaxR || B.ntab < kBoxImageHead) return 0;
    for (int s = 0; s < B.ns; ++s)
        if (B.dims[s] < 1) return 0;
    int32_t end = kBoxImageHead;
    uint32_t seen = 0;
    for (int p = 0; p < B.nr; ++p) {
        if (B.ndep[p] < 1 || B.ndep[p] > kBoxMaxDep || B.nmov[p] < 0 || B.nmov[p] > kBoxMaxDep) return 0;
        if (B.dorder[p] < 0 || B.dorder[p] >= B.nr || (seen >> B.dorder[p] & 1u)) return 0;
        seen |= 1u << B.dorder[p];
        for (int i = 0; i < B.nmov[p]; ++i) {
            const int s = B.mov_s[p][i];
            if (s < 0 || s >= B.ns || B.mov_dim[p][i] != B.dims[s] || B.mov_nu[p][i] == 0) return 0;
        }
        for (int i = 0; i < B.ndep[p]; ++i) {
            const int s = B.dep_s[p][i];
            if (s < 0 || s >= B.ns) return 0;
            const int64_t last = (int64_t)B.dep_off[p][i] + B.dims[s];
            if (B.dep_off[p][i] < kBoxImageHead || last > B.ntab) return 0;
            end = last > end ? (int32_t)last : end;
            int nu = 0;                                  // what the move list says of this species
            for (int j = 0; j < B.nmov[p]; ++j)
                if (B.mov_s[p][j] == s) nu = B.mov_nu[p][j];
            if (B.dep_nu[p][i] != nu) return 0;
        }
    }
    return end;
}

// The transposed SELL product reads the reference arrays: they must be the current generator's (n columns resident,
// a leading dimension that holds the bw slots) and the buffers as long as that says.
static inline bool ell_adj_resident(int64_t n, int64_t ell_cols, int32_t ell_ld, int32_t ell_bw, size_t cap_adj, size_t cap_off,
                             size_t cap_diag)
{
    if (n < 1 || ell_cols != n || ell_bw < 1 || ell_ld < ell_bw) return false;
    const size_t nent = (size_t)n * (size_t)ell_ld;
    return cap_adj >= nent && cap_off >= nent && cap_diag >= (size_t)n;
}

// ---- per-column scalars of a pass (d_bscal), kBlockMaxK entries each: what the kernels of kfsp_block.hip write and
// kfsp_block_host.hip copies out
constexpr int kHB = 0;                                            // [(kMMax + 2) * 3][K]: H(j-1,j), H(j,j), H(j+1,j) of column j
constexpr int kNRM = kHB + (kMMax + 2) * 3 * kBlockMaxK;          // [kMMax + 3][K]: ||u_j||
constexpr int kCO = kNRM + (kMMax + 3) * kBlockMaxK;              // [3][K]: the update coefficients of the column in progress
constexpr int kGG = kCO + 3 * kBlockMaxK;                         // [K]: v_j . v_{j-1}
constexpr int kBRK = kGG + kBlockMaxK;                            // [K]: 0 running, j broke down after column j, -1 skipped
constexpr int kAVN = kBRK + kBlockMaxK;                           // [K]
constexpr int kWS = kAVN + kBlockMaxK;                            // [K]
constexpr int kCMB = kWS + kBlockMaxK;                            // [kMMax + 3][K]: combine coefficients
constexpr int kSQ1 = kCMB + (kMMax + 3) * kBlockMaxK;             // [K]: ||u_1||^2 (what k_barnoldi_small starts from)
constexpr int kScal = kSQ1 + kBlockMaxK;
constexpr int kSmallBlock = 1024;                                 // lanes of a small-path workgroup
enum { kFinBegin = 0, kFinDots = 1, kFinNorm = 2, kFinAvn = 3, kFinWsum = 4 };   // the stages of k_bfinal

// ---- the kernels, by function pointer: kfsp_block_host.hip launches them (the grid and the LDS are its business).  Hidden:
// the shared object exports nothing new.
struct BoxgArgs;   // kfsp_boxg_dev.h
typedef void (*SpmmFn)(SpmmArgs);
typedef void (*SpmmEllTFn)(SpmmArgs, EllAdjDev);
typedef void (*SpmmBoxTFn)(SpmmArgs, BoxAdjDev);
typedef void (*SpmmBoxgFn)(BoxgArgs);
typedef void (*SpmmDiacFn)(SpmmArgs, DiaCodeDev);
#define KFSP_LOCAL __attribute__((visibility("hidden")))
KFSP_LOCAL SpmmDiacFn spmm_diac_kernel(int kp, int w, int rec, bool dots);   // k_spmm_diac (kfsp_block_diac.hip); null: no such form
KFSP_LOCAL SpmmDiacFn spmm_diac_t_kernel(int kp, int w, int rec, bool dots); // k_spmm_diac_t (kfsp_block_diac_t.hip); null: no such form
KFSP_LOCAL SpmmFn spmm_t_kernel(int kp, bool dots);                    // k_spmm_t (kfsp_block_adj.hip)
KFSP_LOCAL SpmmEllTFn spmm_ell_t_kernel(int kp, bool dots);            // k_spmm_ell_t
KFSP_LOCAL SpmmBoxTFn spmm_box_t_kernel(int kp, int inst, bool dots);  // k_spmm_box_t
KFSP_LOCAL SpmmBoxgFn spmm_boxg_t_kernel(int kp, bool dots);           // k_spmm_boxg_t
KFSP_LOCAL SpmmBoxgFn spmm_boxg_kernel(int kp, bool dots);             // k_spmm_boxg (kfsp_block_boxg.hip)
KFSP_LOCAL SpmmFn spmm_kernel(int kp, int fmt, bool dots, bool part);  // k_spmm (kfsp_block.hip)
KFSP_LOCAL SpmmFn spmm_box_kernel(int kp, int inst, bool dots);        // k_spmm_box
// the streaming, finishing and small kernels of kfsp_block.hip, one member each ([1]: the TARGET instantiation)
struct BlockKernels {
    void (*copy_nrm[2])(int64_t, int, const d2 *, d2 *, double *, const uint8_t *, int);
    void (*ortho[2])(int64_t, int, d2 *, const d2 *, const d2 *, const double *, double *, const uint8_t *, int);
    void (*norm)(int64_t, int, const d2 *, double *, const uint8_t *, int);
    void (*norm_target)(int64_t, int, d2 *, double *, const uint8_t *, int);
    void (*target_zero)(int64_t, int, const uint8_t *, d2 *);
    void (*hit)(int64_t, int, int, const uint8_t *, const d2 *, double *);
    void (*target_pack)(int64_t, int64_t, const uint8_t *, const int32_t *, uint8_t *);
    void (*combine)(int64_t, int, const double *, int64_t, int, const double *, d2 *, double *, int);
    void (*combine_int)(int64_t, int, const double *, int64_t, int, const double *, const double *, d2 *, d2 *, double *, int);
    void (*pack)(int64_t, int, int, const double *, int64_t, const int32_t *, double *);
    void (*unpack)(int64_t, int, int, const double *, const int32_t *, double *, int64_t);
    void (*finish)(int, int, int, int, const double *, int64_t, double *, double, double *);
    void (*begin_small)(int, int, const double *, double *, double *);
    void (*combine_small)(int, int, const double *, int64_t, int, const double *, double *, double *, int);
    void (*combine_small_int)(int, int, const double *, int64_t, int, const double *, const double *, double *, double *, double *, int);
};
KFSP_LOCAL const BlockKernels &block_kernels();
#undef KFSP_LOCAL

// the kernel families that stage an image into dynamic LDS - the table image of a matrix-free box, or the dictionaries
// of the coded banded form (options block_dia_code, block_dia_code_adjoint): first index of the occupancy cache
// (kfsp_ctx::blk_staged_occ)
enum StagedFamily { kStagedBox = 0, kStagedBoxT = 1, kStagedBoxg = 2, kStagedBoxgT = 3, kStagedDiac = 4, kStagedDiacT = 5, kStagedFamilies = 6 };

}  // namespace kfsp
