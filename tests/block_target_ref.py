"""TEST HELPER - target sets of the block path (option block_target) restated on the CPU: the killed generator
Q = D A D in the reference's arrays, the flux into the set, the birth chain whose first-passage times are Erlang, and the
bounds the first-passage numbers inherit from the bounds of W and J.

The restated solve is tests/block_integral_ref.expv_block_integral on killed_ell(ell, flags): nothing new is solved here.
"""
import math

import numpy as np

from tests.test_block_integral_host import J_REL_BOUND

W_L1_TOL = 1e-10        # the l1 tolerance of a solved column (tests/test_gpu_block_reference._assert_solve_matches_ref)


def killed_ell(ell, flags):
    """The arrays of D A D, D = diag(1 - flags).  The arrays are column-oriented (column i of A holds -DIAG(i) and
    OFFDIAG(i, :) at the rows ADJ(i, :)): ADJ stays as it is, OFFDIAG is zeroed on the columns of the set and on every
    entry whose target row is in it, DIAG is zeroed on the set.  DIAG off the set keeps the rates INTO the set: that is
    the mass the killed solve loses to it."""
    adj, off, diag = ell
    f = np.asarray(flags).astype(bool)
    n = len(diag)
    adj = np.array(adj, copy=True)
    off = np.array(off, dtype=np.float64, copy=True)
    diag = np.array(diag, dtype=np.float64, copy=True)
    inside = (adj >= 1) & (adj <= n)
    hits = np.zeros(adj.shape, dtype=bool)
    hits[inside] = f[adj[inside] - 1]
    off[hits] = 0.0
    off[f, :] = 0.0
    diag[f] = 0.0
    return adj, off, diag


def hit(A_dense, X, flags):
    """1_T^T A X per column, A the UNMASKED dense generator: the flux into the set"""
    f = np.asarray(flags).astype(bool)
    return (A_dense[f, :] @ X).sum(axis=0)


def amax_T(A_dense, flags):
    """max_j sum_{i in T} A_ij: |1_T^T A x| <= amax_T l1(x) for x supported off T (there the entries A_ij, i in T, are
    rates, >= 0); over all columns, so it also covers rounding-sized entries of x on T"""
    f = np.asarray(flags).astype(bool)
    return float(np.abs(A_dense[f, :]).sum(axis=0).max()) if f.any() else 0.0


def hit_bound_J(A_dense, flags, t, l1w0):
    """|1_T^T A (J - J_exact)| <= amax_T l1(J - J_exact) <= amax_T J_REL_BOUND t l1(w0)"""
    return amax_T(A_dense, flags) * J_REL_BOUND * t * l1w0


def hit_bound_W(A_dense, flags):
    """the same argument on W, whose columns are held to W_L1_TOL in l1"""
    return amax_T(A_dense, flags) * W_L1_TOL


def birth_chain(N, lam):
    """pure birth a(x) = lam on [0, N - 1]: the time from x to the first state >= N0 is Erlang(N0 - x, lam), and the box
    is left (from N - 1) only after every such set was reached"""
    from krylovfspssa_amd import synth
    return synth.BoxModel("birth", (N,), [[1]], lambda r, X: lam + 0.0 * X[0], deps=[(0,)])


def erlang_cdf(k, lam, t):
    """P[Erlang(k, lam) <= t] = 1 - sum_{j < k} exp(-lam t) (lam t)^j / j!; k <= 0: 1"""
    if k <= 0:
        return 1.0
    return 1.0 - math.exp(-lam * t) * sum((lam * t) ** j / math.factorial(j) for j in range(k))


def erlang_pdf(k, lam, t):
    return lam ** k * t ** (k - 1) * math.exp(-lam * t) / math.factorial(k - 1)


def random_set(n, frac=0.3, seed=17):
    return (np.random.default_rng(seed).random(n) < frac).astype(np.uint8)
