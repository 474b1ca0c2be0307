// Private: what the block time loop (kfsp_expv_block, kfsp_stepper.cpp) calls in kfsp_block_host.hip.  Plain host arrays
// and the opaque context only, like the rest of the stepper's view of the library.
#pragma once

#include "../../include/kfsp.h"

#include <stdint.h>

namespace kfsp {

constexpr int kBlockMaxK = 16;

// the resident block: k columns (0 when there is none) and the number of states
int block_shape(kfsp_ctx *ctx, int *k, int64_t *n);
// 0, or -12 when the context's generator / partition cannot take a block
int block_supported(kfsp_ctx *ctx);
// the largest Krylov dimension the basis may have now (option m_max)
int block_mmax(kfsp_ctx *ctx);
// *on = option block_integral is on; -1 (and the message) when it is on but kfsp_set_block ran without it, so that no
// J is resident
int block_integral(kfsp_ctx *ctx, int *on);
// u_1 = W and beta[c] = ||W_c||_2 for the kp columns (padding columns included: 0); the basis is laid out for
// dimension m here (block_arnoldi must not ask for more)
int block_begin(kfsp_ctx *ctx, int m, double *beta);
// IOP(2) Arnoldi of dimension m for every column from the u_1 of block_begin, plus the AVNORM product.
// Out, per column c (kBlockMaxK entries each): hb[(j * 3 + t) * kBlockMaxK + c] for j = 1..m holds H(j-1,j), H(j,j),
// H(j+1,j) (t = 0, 1, 2); nrm[j * kBlockMaxK + c] = ||u_j|| for j = 1..m+1; brk[c] = 0 (no breakdown), j (breakdown
// after column j: H(j+1,j) <= break_tol), -1 (beta = 0, column skipped); avnorm[c] = ||A v_{m+1}||.
int block_arnoldi(kfsp_ctx *ctx, int m, double break_tol, double *hb, double *nrm, int *brk, double *avnorm);
// W_c = max(sum_i coef[i * kBlockMaxK + c] u_{i+1,c}, 0) for i < mx and wsum[c] = ||W_c||_1 (c < kp).  With option
// block_integral on, coef holds a second table behind the first - rows [mx, 2 mx) - and J_c += sum_i coef[(mx + i) *
// kBlockMaxK + c] u_{i+1,c} in the same pass over the basis (J: the time integral kept beside the block, never clamped;
// wsum stays W's)
int block_combine(kfsp_ctx *ctx, int mx, const double *coef, double *wsum);

}  // namespace kfsp
