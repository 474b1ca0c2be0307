// Private, host only: the coefficients of the time integral of a block step (option block_integral; DESIGN.md 12,
// "Time integrals").  No device dependency: tests/block_integral_check.cpp builds it with kfsp_padm.cpp alone.
//
// A step holds, per column, beta, the basis V and the augmented Hessenberg matrix Hbar (order mh = MBRKDWN + K1) with
//     exp(tau A) w ~ beta V [exp(tau Hbar) e_1].
// The same basis gives
//     int_0^tau exp(s A) w ds = tau phi_1(tau A) w ~ beta V [tau phi_1(tau Hbar) e_1],
// and tau phi_1(tau Hbar) e_1 is the top of the last column of exp(tau Hhat), Hhat = [[Hbar, e_1], [0, 0]] of order mh + 1:
// one more Pade exponential of the routine that gave exp(tau Hbar).
#pragma once

#include "../../include/kfsp.h"

#include <cstddef>
#include <vector>

namespace kfsp {

// g[0 .. rows) = the top `rows` (<= mh) entries of the last column of exp(tau Hhat), Hhat built on the leading mh x mh part
// of the column-major H (leading dimension ldh).  A null H (A v_1 = 0, which kfsp_padm refuses for exp(tau H) itself) gives
// g = tau e_1 exactly.  work is scratch the caller keeps between calls.  0, or kfsp_padm's error.
inline int block_integral_column(int ideg, int mh, int rows, double tau, const double *H, int ldh, double *g, std::vector<double> &work)
{
    if (mh < 1 || rows < 1 || rows > mh || ldh < mh || !H || !g) return -2;
    bool null_h = true;
    for (int j = 0; j < mh && null_h; ++j)
        for (int i = 0; i < mh; ++i) null_h = null_h && H[(size_t)j * ldh + i] == 0.0;
    if (null_h) {
        for (int i = 0; i < rows; ++i) g[i] = 0.0;
        g[0] = tau;
        return 0;
    }
    const int n = mh + 1;
    work.assign((size_t)2 * n * n, 0.0);
    double *Hh = work.data(), *E = work.data() + (size_t)n * n;
    for (int j = 0; j < mh; ++j)
        for (int i = 0; i < mh; ++i) Hh[(size_t)j * n + i] = H[(size_t)j * ldh + i];
    Hh[(size_t)mh * n] = 1.0;                                   // e_1 in the last column
    if (const int rc = kfsp_padm(ideg, n, tau, Hh, n, E, nullptr, nullptr)) return rc;
    for (int i = 0; i < rows; ++i) g[i] = E[(size_t)mh * n + i];
    return 0;
}

}  // namespace kfsp
