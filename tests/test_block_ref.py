"""The CPU restatement of the block solve (tests/block_ref.py) and the analytic birth-death distribution
(tests/bd_truth.py) that the GPU block tests compare with, checked against scipy's dense exponential, the oracle's
single-vector solve and each other.  No GPU needed."""
import numpy as np
import pytest
import scipy.linalg as sl

from tests import bd_truth
from tests import block_ref as BR


def _dense(ell):
    """A of the reference's ELL arrays: column i holds -DIAG(i) and OFFDIAG(:, i) at the rows ADJ(:, i) (FMATVEC)"""
    adj, off, diag = ell
    n = len(diag)
    A = np.diag(-np.asarray(diag, dtype=np.float64))
    for i in range(n):
        for j, v in zip(adj[i], off[i]):
            if j >= 1:
                A[j - 1, i] += v
    return A


def _bd(dims, **kw):
    from krylovfspssa_amd import synth
    return synth.birth_death(dims, **kw)


def _start(n, k, rng):
    W = np.zeros((n, k))
    for c in range(k):
        if c % 3 == 0:
            W[(7 * c + 3) % n, c] = 1.0
        elif c % 3 == 1:
            p = rng.random(n) ** (c + 1)
            W[:, c] = p / p.sum()
        else:
            W[:, c] = 2.5 * rng.random(n)                  # beta > 1: not a probability vector
    return W


def test_dense_operator_is_the_oracle_product(oracle):
    mdl = _bd((9, 7))
    ell = mdl.ell()
    x = np.random.default_rng(0).random(mdl.n)
    assert np.allclose(_dense(ell) @ x, oracle.spmv_ell(oracle.EllMatrix(*ell), x), rtol=1e-14, atol=1e-14)


@pytest.mark.parametrize("case", ["toggle", "stiff_birth_death", "tol_below_eps"])
def test_restatement_matches_dense_expm(oracle, case):
    """exp(tA) W from scipy.  The block solve accepts a step when its error estimate ERR_LOC <= DELTA tol t_step (:314,
    :375), so the 2-norm error over [0, t] is estimated at <= DELTA tol t per column, times the column's beta (ERR_LOC
    carries beta); the l1 error is at most sqrt(n) times the 2-norm error."""
    from krylovfspssa_amd import synth
    if case == "stiff_birth_death":
        mdl, t, tol = _bd((14, 11), k=(400.0, 650.0), g=(50.0, 80.0)), 0.2, 1e-10
    else:
        mdl, t, tol = synth.toggle(14, 12), 0.5, (1e-10 if case == "toggle" else 1e-17)
    ell = mdl.ell()
    A = oracle.EllMatrix(*ell)
    W = _start(mdl.n, 5, np.random.default_rng(3))
    R, ws, st = BR.expv_block(A, W, t, tol, 30)
    ref = np.maximum(sl.expm(t * _dense(ell)) @ W, 0.0)
    krytol = BR.krylov_tol(tol)
    assert st.t_now == pytest.approx(t, rel=1e-15) and st.nstep >= 2
    if case == "stiff_birth_death":
        assert st.nreject >= 1
    for c in range(W.shape[1]):
        beta = np.linalg.norm(W[:, c])
        assert np.abs(R[:, c] - ref[:, c]).sum() <= BR.DELTA * krytol * t * beta * np.sqrt(mdl.n), (case, c)
        assert ws[c] == R[:, c].sum()
    assert st.nmult == st.nstep * 31
    assert st.step_min <= st.step_max and st.x_error <= st.s_error


def test_one_step_is_the_oracle_single_vector_step(oracle):
    """below the first step size the block solve is one Krylov step of every column: oracle.expv_fixed(m, t, 1) - the
    same Arnoldi and Pade, only the combine is summed by numpy here, so rounding is all that separates them"""
    mdl = _bd((20, 15))
    A = oracle.EllMatrix(*mdl.ell())
    W = _start(mdl.n, 6, np.random.default_rng(4))
    m, tol = 20, 1e-9
    t = 0.02                                           # a step the error test accepts at once
    assert t < BR.first_step(m, tol, np.linalg.norm(W, axis=0).max())
    R, ws, st = BR.expv_block(A, W, t, tol, m)
    assert (st.nstep, st.nreject, st.nmult, st.t_now) == (1, 0, m + 1, t)
    assert (st.step_min, st.step_max, st.x_error, st.s_error) == (t, 0.0, 0.0, 0.0)   # the last step enters no statistics
    for c in range(W.shape[1]):
        w1, ws1 = oracle.expv_fixed(A, W[:, c], m, t, 1)
        assert np.abs(R[:, c] - w1).sum() <= 1e-13 * np.abs(W[:, c]).sum()
        assert abs(ws[c] - ws1[0]) <= 1e-14 * ws1[0]


def test_restatement_meets_the_analytic_distribution(oracle):
    """the FSP relation of tests/bd_truth.py on a 2-species box: R <= truth|box up to the solve's tolerance, and the mass
    R lost is the gap"""
    dims, t, tol = (45, 40), 0.8, 1e-10
    k, g = bd_truth.default_rates(2)
    mdl = _bd(dims)
    A = oracle.EllMatrix(*mdl.ell())
    x0s = [(0, 0), (20, 5), (30, 30), (44, 39)]
    W = np.zeros((mdl.n, len(x0s)))
    for c, x0 in enumerate(x0s):
        W[x0[0] + dims[0] * x0[1], c] = 1.0
    R, ws, st = BR.expv_block(A, W, t, tol, 30)
    for c, x0 in enumerate(x0s):
        truth, out = bd_truth.box_pmf(dims, k, g, x0, t)
        d = truth - R[:, c]
        # ERR_LOC <= DELTA tol t_step per accepted step: <= DELTA tol t over the interval (beta = 1 for a unit vector)
        bound = BR.DELTA * tol * t
        assert d.min() >= -bound, (x0, d.min())
        assert abs(d.sum() - (1.0 - ws[c] - out)) <= bound, (x0, d.sum(), 1.0 - ws[c], out)
        assert np.abs(d).sum() <= (1.0 - ws[c] - out) + 2 * bound


def test_pmf_helper_is_the_dense_exponential():
    """bd_truth on a box wide enough that nothing reaches its edge: the dense exp(tA) e_x0 of the same generator"""
    dims, t = (45, 40), 0.8
    k, g = bd_truth.default_rates(2)
    mdl = _bd(dims)
    A = _dense(mdl.ell())
    x0 = (12, 3)
    e = np.zeros(mdl.n)
    e[x0[0] + dims[0] * x0[1]] = 1.0
    ref = sl.expm(t * A) @ e
    truth, out = bd_truth.box_pmf(dims, k, g, x0, t)
    assert out < 1e-14
    assert np.abs(truth - ref).sum() <= 1e-13


def test_zero_and_absorbing_columns(oracle):
    """beta = 0 columns stay exactly 0 with wsum 0; A e_0 = 0 breaks down at once with a null H and comes back e_0;
    a block of zeros is its own solution"""
    N, b, gam = 40, 6.0, 1.0
    # birth-death chain with an absorbing state 0 (no births there), in the reference's ELL layout
    adj = np.zeros((N, 2), dtype=np.int32)
    off = np.zeros((N, 2))
    diag = np.zeros(N)
    for i in range(N):
        if 0 < i < N - 1:
            adj[i, 0], off[i, 0] = i + 2, b
        if i > 0:
            adj[i, 1], off[i, 1] = i, gam * i
        diag[i] = off[i].sum() + (b if i == N - 1 else 0.0)
    A = oracle.EllMatrix(adj, off, diag)
    W = np.zeros((N, 3))
    W[0, 0] = 1.0
    W[20, 2] = 1.0
    R, ws, st = BR.expv_block(A, W, 0.5, 1e-10, 10)
    assert np.array_equal(R[:, 0], W[:, 0]) and ws[0] == 1.0
    assert not R[:, 1].any() and ws[1] == 0.0
    assert st.n_breakdown_cols >= 1
    ref = np.maximum(sl.expm(0.5 * _dense((adj, off, diag))) @ W, 0.0)
    assert np.abs(R[:, 2] - ref[:, 2]).sum() <= BR.DELTA * 1e-10 * 0.5 * np.sqrt(N)
    Z, wz, sz = BR.expv_block(A, np.zeros((N, 2)), 0.5, 1e-10, 10)
    assert not Z.any() and not wz.any() and (sz.nstep, sz.t_now) == (0, 0.5)


def test_transpose_is_the_transpose(oracle):
    """block_ref.transpose_ell against the dense transpose, entry by entry, on an FSP with links that leave it"""
    from tests import block_generators
    from tests.conftest import GOLDEN
    g = block_generators.golden_toggle(GOLDEN)
    ell = (g["adj"], g["offdiag"], g["diag"])
    assert (ell[0] < 1).any()
    assert np.array_equal(_dense(BR.transpose_ell(*ell)), _dense(ell).T)
    x = np.random.default_rng(1).standard_normal(len(g["diag"]))
    assert np.allclose(oracle.spmv_ell(oracle.EllMatrix(*BR.transpose_ell(*ell)), x), _dense(ell).T @ x, rtol=1e-13, atol=1e-13)


def test_backward_restatement_matches_dense_expm(oracle):
    """exp(tA^T) F for signed observables: the restatement on A^T with the clamp off against scipy's dense exponential,
    at the bound of the device's backward test (tests/test_gpu_block_adjoint.py: backward the roles of l1 and max norm
    swap, so column c is held to max|R_c - ref_c| <= 10 tol max|F_c|); wsum is the l1 norm; the clamped default would
    have wiped the negative column out"""
    from krylovfspssa_amd import synth
    mdl = synth.toggle(23, 19)
    t, tol, m = 0.3, 1e-8, 30
    ell = mdl.ell()
    x1, x2 = (c.astype(np.float64) for c in mdl.coords(np.arange(mdl.n, dtype=np.int64)))
    ind = np.zeros(mdl.n)
    ind[mdl.n // 2 + 3] = 1.0
    F = np.column_stack([np.ones(mdl.n), x1, x2, x1 * x2, ind, -x1])
    AT = oracle.EllMatrix(*BR.transpose_ell(*ell))
    R, ws, st = BR.expv_block(AT, F, t, tol, m, clamp=False)
    ref = sl.expm(t * _dense(ell)).T @ F
    assert st.t_now == pytest.approx(t, rel=1e-15) and st.nstep >= 2
    for c in range(F.shape[1]):
        err = np.abs(R[:, c] - ref[:, c]).max()
        print("column", c, "max err", err, "bound", 10 * tol * np.abs(F[:, c]).max())
        assert err <= 10 * tol * np.abs(F[:, c]).max(), c
        assert ws[c] == np.abs(R[:, c]).sum()
    assert np.all(R[:, 5] <= 0.0) and (R[:, 5] < 0.0).any()
    Rc, wc, _ = BR.expv_block(AT, F, t, tol, m)
    assert not Rc[:, 5].any() and wc[5] == 0.0 and np.all(Rc >= 0.0)
