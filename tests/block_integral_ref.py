"""TEST HELPER - the block solve of tests/block_ref.py with the time integral J added (option block_integral), and the
fused combine restated exactly.

expv_block_integral is block_ref.expv_block line for line - the same step control, the same per-column Krylov pass and
Pade evaluation through the oracle - with one addition after every accepted step:

    J_c <- J_c + beta_c V_c[:, :mx_c] g_c[:mx_c],   g_c = the last column of exp(tau Hhat_c),
    Hhat_c = [[Hbar_c, e_1], [0, 0]]  (Hbar_c: the MBRKDWN + K1 square the step used),  mx_c = MBRKDWN + MAX(0, K1 - 1)

(tau phi_1(tau Hbar) e_1 = int_0^tau exp(s Hbar) e_1 ds; a null Hbar gives g = tau e_1).  J enters nothing else: W, wsum
and the statistics are block_ref's.

combine_int_exact is one launch of k_bcombine_int / k_bcombine_small_int element for element: two fma chains over the
same u, j ascending, W from +0.0 with the clamp, J from the old J element without one.
"""
import math

import numpy as np

from oracle import oracle as O
from tests import block_ref as BR
from tests import row_ref


def integral_column(H, tau):
    """g = the top part of the last column of exp(tau [[H, e_1], [0, 0]]) (H square, the step's Hbar): tau phi_1(tau H) e_1"""
    mx = H.shape[0]
    if not np.any(H):
        g = np.zeros(mx)
        g[0] = tau
        return g
    Hh = np.zeros((mx + 1, mx + 1), order="F")
    Hh[:mx, :mx] = H
    Hh[0, mx] = 1.0
    return O.padm(Hh, tau, BR.IDEG)[0][:mx, mx].copy()


def expv_block_integral(A, W, t, tol, m, clamp=True, J=None):
    """-> (W(t), wsum, BlockStats, J): block_ref.expv_block with J <- J + int_0^tau exp(sA) W_step ds beside every accepted
    step.  J=None starts from zeros; a J handed in is continued (two calls accumulate)."""
    n = A.n
    W = np.array(W, dtype=np.float64, copy=True)
    k = W.shape[1]
    J = np.zeros((n, k)) if J is None else np.array(J, dtype=np.float64, copy=True)
    m = min(int(m), max(n - 1, 1))
    krytol = BR.krylov_tol(tol)
    rndoff = BR.machine_eps()
    st = BR.BlockStats(step_min=t)
    wsum = np.zeros(k)
    broke = np.zeros(k, dtype=bool)

    t_now = t_old = omega = omega_old = order = 0.0
    m_old = 0
    orderold = True
    bmax = float(np.sqrt((W * W).sum(axis=0)).max())
    t_new = BR.first_step(m, tol, bmax) if bmax > 0.0 else 0.0
    while bmax > 0.0 and t_now < t:
        t_step = min(t - t_now, t_new)
        st.nstep += 1
        cols = [BR._Column(A, W[:, c], m) for c in range(k)]
        st.nmult += m + 1
        live = [c for c in range(k) if cols[c].beta > 0.0]
        for c in live:
            broke[c] |= cols[c].k1 == 0
        all_broke = all(cols[c].k1 == 0 for c in live)
        if all_broke:
            t_step = t - t_now
        ireject = 0
        while True:
            err = 0.0
            for c in live:
                cols[c].expH(t_step)
                if cols[c].k1 == 0:
                    continue
                e = cols[c].err_loc(m)
                if math.isnan(e) or e > err:
                    err = e
                if math.isnan(err):
                    break
            if math.isnan(err):
                t_step /= 5.0
                continue
            omega_old = omega
            omega = err / (krytol * t_step)
            if m == m_old and t_step != t_old and ireject >= 1:
                order = max(1.0, BR._log(omega / omega_old) / BR._log(t_step / t_old))
                orderold = False
            elif orderold or ireject == 0:
                order = m / 4.0
                orderold = True
            else:
                orderold = True
            t_old = t_step
            m_old = m
            remaining = t - t_now
            prop = BR.GAMMA * t_step * omega ** (-1.0 / order) if omega > 0.0 else math.inf
            t_new = BR.two_digits(BR.clamp_step(remaining, t_step, prop), 0.0)
            if not all_broke and omega > BR.DELTA:
                t_step = BR.two_digits(BR.clamp_step(remaining, t_step, t_new), 0.55)
                ireject += 1
                st.nreject += 1
                continue
            break
        if err < 1.0e-16:
            t_new = max(t_new, 2.0 * t_step)
        for c in live:
            col = cols[c]
            # ---- the addition: the accepted step's time integral from the same basis, never clamped
            mh = col.mbrk + col.k1
            mx = col.mbrk + max(0, col.k1 - 1)
            g = integral_column(np.array(col.H[:mh, :mh], order="F"), t_step)
            J[:, c] += col.beta * (col.V[:, :mx] @ g[:mx])
            # ----
            W[:, c] = col.combine(clamp)
            wsum[c] = W[:, c].sum() if clamp else np.abs(W[:, c]).sum()
        t_now += t_step
        st.steps.append(t_step)
        if t_now >= t:
            break
        err = max(err, rndoff)
        st.step_min = min(st.step_min, t_step)
        st.step_max = max(st.step_max, t_step)
        st.s_error += err
        st.x_error = max(st.x_error, err)
        t_new = BR.two_digits(t_new, 0.55)
        bmax = float(np.sqrt((W * W).sum(axis=0)).max())
    if not bmax > 0.0:
        t_now = t
    st.t_now = t_now
    st.n_breakdown_cols = int(broke.sum())
    return W, wsum, st, J


def combine_int_exact(U, coef, cj, J_old, clamp):
    """U[j]: (n, k) basis columns u_{j+1}, coef / cj: (mx, k), J_old: (n, k) -> (W, J) as lists of rows.  Per element:
    s = fma(coef[j], u, s) from +0.0 and r = fma(cj[j], u, r) from the old J element, j ascending; then W's clamp."""
    mx = len(coef)
    n, k = np.shape(J_old)
    U = [np.asarray(u).tolist() for u in U[:mx]]
    coef, cj, J_old = np.asarray(coef).tolist(), np.asarray(cj).tolist(), np.asarray(J_old).tolist()
    Wn = [[0.0] * k for _ in range(n)]
    Jn = [[0.0] * k for _ in range(n)]
    for i in range(n):
        for c in range(k):
            s, r = 0.0, J_old[i][c]
            for j in range(mx):
                u = U[j][i][c]
                s = row_ref.fma(coef[j][c], u, s)
                r = row_ref.fma(cj[j][c], u, r)
            if clamp:
                s = s if s > 0.0 else 0.0
            Wn[i][c] = s
            Jn[i][c] = r
    return np.array(Wn), np.array(Jn)


def dense_integral(A, W0, t):
    """J_dense = the top block of the last columns of expm(t [[A, W0], [0, 0]]) = int_0^t exp(sA) W0 ds (A dense)"""
    import scipy.linalg as sl
    n, k = W0.shape
    M = np.zeros((n + k, n + k))
    M[:n, :n] = A
    M[:n, n:] = W0
    return sl.expm(t * M)[:n, n:]


# ---- the small generators the accuracy of J is measured on (tests/test_block_integral_host.py) and the device is held
# to (tests/test_gpu_block_integral.py): name -> ELL arrays in the caller's order, and the time of the solve
def dense_of_ell(ell):
    """A of the reference's ELL arrays: column i holds -DIAG(i) and OFFDIAG(:, i) at the rows ADJ(:, i) (FMATVEC)"""
    adj, off, diag = ell
    n = len(diag)
    A = np.diag(-np.asarray(diag, dtype=np.float64))
    for i in range(n):
        for j, v in zip(adj[i], off[i]):
            if 1 <= j <= n:
                A[j - 1, i] += v
    return A


def death_chain(N=201, g=0.5):
    """tests/test_block_adjoint_host.py::death_chain: pure death a(x) = g x on [0, N - 1]; A^T f = -g f for f(x) = x"""
    from krylovfspssa_amd import synth
    return synth.BoxModel("death", (N,), [[-1]], lambda r, X: g * X[0], deps=[(0,)])


def small_cases(golden_dir):
    import os
    from krylovfspssa_amd import synth
    g = np.load(os.path.join(golden_dir, "assembly_toggle_k20.npz"))
    return {"toggle_fsp_231": ((g["adj"], g["offdiag"], g["diag"]), 0.3),
            "toggle_box_21x13": (synth.toggle(21, 13).ell(), 0.3),
            "death_chain": (death_chain().ell(), 1.0)}


def start_block(n, transposed, seed=5):
    """k = 3 (kp = 4, one padding column).  Forward: a unit vector, a probability vector, a column of mixed signs.
    Backward: g = 1 (the exit time), g(x) = the state's index (on the death chain the eigenvector f(x) = x), mixed signs."""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, 3))
    if transposed:
        W[:, 0] = 1.0
        W[:, 1] = np.arange(n, dtype=np.float64)
    else:
        W[n // 3, 0] = 1.0
        p = rng.random(n)
        W[:, 1] = p / p.sum()
    W[:, 2] = rng.standard_normal(n)
    return W


def accuracy(ell, transposed, t, tol, m):
    """the restatement against the dense integral, unclamped -> (max_c l1(J_ref - J_dense)_c / (t l1(w0_c)),
    max_c l1(A J_ref - (W_ref(t) - W0))_c / l1(w0_c), steps)"""
    A = dense_of_ell(ell)
    if transposed:
        A = A.T
        ell = BR.transpose_ell(*ell)
    W0 = start_block(A.shape[0], transposed)
    W, ws, st, J = expv_block_integral(O.EllMatrix(*ell), W0, t, tol, m, clamp=False)
    l1 = np.abs(W0).sum(axis=0)
    err = np.abs(J - dense_integral(A, W0, t)).sum(axis=0) / (t * l1)
    res = np.abs(A @ J - (W - W0)).sum(axis=0) / l1
    return float(err.max()), float(res.max()), st.nstep
