"""TEST HELPER - the block solve kfsp_expv_block restated on the CPU, column by column.

W <- exp(tA) W for k start columns with EXPOKIT's step control of DGEXPV_FSP (KrylovSolver.f90) in the form the header
documents for the block (include/kfsp.h, "several vectors at once"): the Krylov dimension fixed at m (so the M_MAX
branch of :339-346 always proposes the next step: no dimension change, no cost model), one step size for all columns,
accepted iff the worst column passes, no FSP test, no drop / expand.  Each column's Krylov pass and Pade evaluation are
the oracle's (oracle/kfsp_oracle.c: kfo_arnoldi with IOP(2) and BREAK_TOL 1e-7, kfo_padm with IDEG 6), so only the step
control, restated here from the Fortran, lies between the oracle and this module.

Block rules that DGEXPV_FSP has no counterpart for (include/kfsp.h):
  * the first step from the LARGEST beta (:182-187 with BETA = max_c beta_c);
  * a column that broke down is exact: it adds nothing to the error and, when every column broke down, the step takes
    the rest of the interval (:254) and cannot be rejected (K1 = 0 at :375);
  * A v_1 = 0 (an absorbing start state) gives a null H, which DGPADM refuses (dgpadm.f:84): exp(tH) = I;
  * a column with beta = 0 is skipped and stays exactly 0; a block of zeros is its own solution.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import oracle as O

IDEG = 6          # :82
DELTA = 1.2       # :85
GAMMA = 0.9       # :87
BREAK_TOL = 1e-7  # :173
SQR1 = math.sqrt(0.1)


def machine_eps():
    """EPS by the 4/3 trick (:166-170)"""
    p1 = 4.0 / 3.0
    while True:
        p2 = p1 - 1.0
        p3 = p2 + p2 + p2
        eps = abs(p3 - 1.0)
        if eps != 0.0:
            return eps


def int_power(x, k):
    """x**k for an INTEGER k as Fortran compilers expand it (repeated squaring)"""
    e = abs(k)
    r, b = 1.0, float(x)
    while e:
        if e & 1:
            r *= b
        b *= b
        e >>= 1
    return 1.0 / r if k < 0 else r


def _nint(x):
    """Fortran NINT: to the nearest integer, halves away from 0"""
    a = abs(x)
    f = math.floor(a)
    r = f + 1 if a - f >= 0.5 else f
    return int(r) if x >= 0 else -int(r)


def two_digits(t, bias):
    """P1 = 10**(NINT(LOG10(T) - SQR1) - 1); T = AINT(T / P1 + bias) * P1 (bias 0.55: :186-187, :382-383, :548-549;
    bias 0: :344-345)"""
    unit = int_power(10.0, _nint(math.log10(t) - SQR1) - 1)
    return math.trunc(t / unit + bias) * unit


def clamp_step(remaining, t_step, proposal):
    """MIN(T_OUT - T_NOW, MAX(T_STEP / 5, MIN(5 T_STEP, proposal))) (:340-343, :379-381)"""
    return min(remaining, max(t_step / 5.0, min(5.0 * t_step, proposal)))


def krylov_tol(tol):
    """KRYTOL (:171)"""
    eps = machine_eps()
    return math.sqrt(eps) if tol <= eps else tol


def first_step(m, tol, beta):
    """T_NEW before the first step (:182-187, ANORM = 1)"""
    p1 = krylov_tol(tol) * int_power((m + 1) / 2.72, m + 1) * math.sqrt(2.0 * 3.14 * (m + 1))
    return two_digits((p1 / (4.0 * beta)) ** (1.0 / m), 0.55)


@dataclass
class BlockStats:
    """every field of kfsp_block_stats, and the accepted step sizes"""
    nstep: int = 0
    nreject: int = 0
    nmult: int = 0
    n_breakdown_cols: int = 0
    t_now: float = 0.0
    step_min: float = 0.0
    step_max: float = 0.0
    x_error: float = 0.0
    s_error: float = 0.0
    steps: list = field(default_factory=list)


class _Column:
    """one column's Krylov pass (:223-266): the oracle's IOP(2) Arnoldi from w / beta"""

    def __init__(self, A, w, m):
        self.beta = float(np.sqrt(np.dot(w, w)))
        self.E = None
        if self.beta > 0.0:
            self.V, self.H, self.mbrk, self.k1, self.avnorm = O.arnoldi(A, w / self.beta, m, qiop=2, break_tol=BREAK_TOL)

    def expH(self, t_step):
        """exp(t_step H) over MX = MBRKDWN + K1 rows (:272-275)"""
        mx = self.mbrk + self.k1
        Hs = np.array(self.H[:mx, :mx], order="F")
        self.E = O.padm(Hs, t_step, IDEG)[0] if np.any(Hs) else np.eye(mx)   # a null H: exp(tH) = I

    def err_loc(self, m):
        """ERR_LOC of a column that did not break down (:290-305)"""
        p1 = abs(self.E[m, 0]) * self.beta
        p2 = abs(self.E[m + 1, 0]) * self.beta * self.avnorm
        if p1 > 10.0 * p2:
            return p2
        if p1 > p2:
            return (p1 * p2) / (p1 - p2)
        return p1

    def combine(self, clamp=True):
        """W = max(BETA V(:, 1:MX) exp(t H) e_1, 0) over MX = MBRKDWN + MAX(0, K1 - 1) (:438, :444-449); clamp=False
        keeps the signed entries (option block_clamp = 0)"""
        mx = self.mbrk + max(0, self.k1 - 1)
        w = self.beta * (self.V[:, :mx] @ self.E[:mx, 0])
        return np.maximum(w, 0.0) if clamp else w


def _log(x):
    return math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan)


def transpose_ell(adj, off, diag):
    """A^T in the reference's arrays, for the backward solves (option adjoint).  The arrays are column-oriented: column i
    of a matrix holds -DIAG(i) and OFFDIAG(:, i) at the rows ADJ(:, i).  Column i of A^T is row i of A, so adj_T[i] =
    1 + the columns of the off-diagonal entries of row i (ascending by column, then value, then slot: the order of
    tests/row_ref.py), off_T[i] their values, diag_T = diag; the slot count is the longest row's."""
    from tests import row_ref
    rows = row_ref.gather_rows(adj, off, diag)
    n, bw = len(rows), max(1, max(len(r) for r in rows))
    adj_t = np.zeros((n, bw), dtype=np.int32)
    off_t = np.zeros((n, bw))
    for i, row in enumerate(rows):
        for j, (c, v) in enumerate(row):
            adj_t[i, j], off_t[i, j] = c + 1, v
    return adj_t, off_t, np.array(diag, dtype=np.float64)


def expv_block(A, W, t, tol, m, clamp=True):
    """A: oracle.EllMatrix, W: (n, k) start columns -> (W(t) (n, k), wsum[k], BlockStats).  clamp=False: the combine
    keeps signed entries and wsum is the l1 norm of the column (option block_clamp = 0: signed observables)"""
    n = A.n
    W = np.array(W, dtype=np.float64, copy=True)
    k = W.shape[1]
    m = min(int(m), max(n - 1, 1))                   # :211
    krytol = krylov_tol(tol)
    rndoff = machine_eps()                           # EPS * ANORM with ANORM = 1 (:129, :172)
    st = BlockStats(step_min=t)
    wsum = np.zeros(k)
    broke = np.zeros(k, dtype=bool)

    t_now = t_old = omega = omega_old = order = 0.0
    m_old = 0
    orderold = True
    bmax = float(np.sqrt((W * W).sum(axis=0)).max())
    t_new = first_step(m, tol, bmax) if bmax > 0.0 else 0.0
    while bmax > 0.0 and t_now < t:
        t_step = min(t - t_now, t_new)               # :208
        st.nstep += 1
        cols = [_Column(A, W[:, c], m) for c in range(k)]
        st.nmult += m + 1                            # block products: m for the basis, one for AVNORM
        live = [c for c in range(k) if cols[c].beta > 0.0]
        for c in live:
            broke[c] |= cols[c].k1 == 0
        all_broke = all(cols[c].k1 == 0 for c in live)
        if all_broke:
            t_step = t - t_now                       # :254
        ireject = 0
        while True:                                  # label 401
            err = 0.0
            for c in live:
                cols[c].expH(t_step)
                if cols[c].k1 == 0:
                    continue                         # exact: no error
                e = cols[c].err_loc(m)
                if math.isnan(e) or e > err:
                    err = e
                if math.isnan(err):
                    break
            if math.isnan(err):                      # :307-310
                t_step /= 5.0
                continue
            omega_old = omega
            omega = err / (krytol * t_step)          # :314
            if m == m_old and t_step != t_old and ireject >= 1:     # :316-324
                order = max(1.0, _log(omega / omega_old) / _log(t_step / t_old))
                orderold = False
            elif orderold or ireject == 0:
                order = m / 4.0
                orderold = True
            else:
                orderold = True
            t_old = t_step
            m_old = m
            remaining = t - t_now
            prop = GAMMA * t_step * omega ** (-1.0 / order) if omega > 0.0 else math.inf
            t_new = two_digits(clamp_step(remaining, t_step, prop), 0.0)      # :339-346
            if not all_broke and omega > DELTA:      # :375-399
                t_step = two_digits(clamp_step(remaining, t_step, t_new), 0.55)
                ireject += 1
                st.nreject += 1
                continue
            break
        if err < 1.0e-16:                            # :437
            t_new = max(t_new, 2.0 * t_step)
        for c in live:
            W[:, c] = cols[c].combine(clamp)
            wsum[c] = W[:, c].sum() if clamp else np.abs(W[:, c]).sum()   # DASUM :450 of a clamped column / the l1 norm
        t_now += t_step
        st.steps.append(t_step)
        if t_now >= t:                               # :503: the last step enters no statistics
            break
        err = max(err, rndoff)                       # :540-547
        st.step_min = min(st.step_min, t_step)
        st.step_max = max(st.step_max, t_step)
        st.s_error += err
        st.x_error = max(st.x_error, err)
        t_new = two_digits(t_new, 0.55)              # :548-549
        bmax = float(np.sqrt((W * W).sum(axis=0)).max())
    if not bmax > 0.0:
        t_now = t                                    # a block of zeros is its own solution
    st.t_now = t_now
    st.n_breakdown_cols = int(broke.sum())
    return W, wsum, st
