"""Target sets of the block path without a GPU: the CPU restatement of a killed solve - block_integral_ref on the arrays
of D A D (tests/block_target_ref.py) - against the Erlang first-passage law of a birth chain, the mass balance and the
forward / backward duality; and the surface of the new calls.

Bounds (block_target_ref): every number made from J is a sum over the set of A (J - J_exact), at most amax_T l1(J -
J_exact) <= amax_T J_REL_BOUND t l1(w0) with J_REL_BOUND the measured bound of tests/test_block_integral_host.py; every
number made from W the same with the 1e-10 l1 tolerance of a solved column.  The device is held to the same bounds
(tests/test_gpu_block_target.py)."""
import ctypes
import os

import numpy as np
import pytest

from tests import block_integral_ref as IR
from tests import block_ref as BR
from tests import block_target_ref as TR
from tests.conftest import ROOT
from tests.test_block_integral_host import J_REL_BOUND

N, N0, LAM, T_END = 45, 12, 3.0, 2.5
TOL, M = 1e-8, 30


def _solve(oracle, ell, W0, t, transposed=False, J=None):
    if transposed:
        ell = BR.transpose_ell(*ell)
    return IR.expv_block_integral(oracle.EllMatrix(*ell), W0, t, TOL, M, clamp=False, J=J)


def test_killed_arrays_are_D_A_D(golden_dir):
    for name in ("toggle_fsp_231", "toggle_box_21x13"):
        ell, _ = IR.small_cases(golden_dir)[name]
        A = IR.dense_of_ell(ell)
        f = TR.random_set(A.shape[0])
        D = np.diag(1.0 - f)
        Q = IR.dense_of_ell(TR.killed_ell(ell, f))
        assert np.array_equal(Q, D @ A @ D), name
        assert np.array_equal(TR.killed_ell(ell, f)[0], ell[0])          # ADJ untouched
        assert 0 < f.sum() < len(f)


def test_erlang_cdf_and_density(oracle):
    """T = {x >= 12}, start e_0 (and e_5): the hit time is Erlang(12 - x0, 3)"""
    ell = TR.birth_chain(N, LAM).ell()
    A = IR.dense_of_ell(ell)
    f = (np.arange(N) >= N0).astype(np.uint8)
    W0 = np.zeros((N, 2))
    W0[0, 0] = W0[5, 1] = 1.0
    W, ws, st, J = _solve(oracle, TR.killed_ell(ell, f), W0, T_END)
    assert not W[N0:].any() and not J[N0:].any()
    cdf, pdf = TR.hit(A, J, f), TR.hit(A, W, f)
    bj, bw = TR.hit_bound_J(A, f, T_END, 1.0), TR.hit_bound_W(A, f)
    for c, x0 in enumerate((0, 5)):
        ej = abs(cdf[c] - TR.erlang_cdf(N0 - x0, LAM, T_END))
        ew = abs(pdf[c] - TR.erlang_pdf(N0 - x0, LAM, T_END))
        eb = abs(ws[c] + cdf[c] - 1.0)
        print("x0", x0, "cdf", cdf[c], "err/bound", ej / bj, "pdf", pdf[c], "err/bound", ew / bw, "balance err/bound", eb / (bj + TR.W_L1_TOL))
        assert ej <= bj and ew <= bw
        assert eb <= bj + TR.W_L1_TOL                                  # the box is not left before T is reached
    # two solves accumulate to the same CDF value
    W1, _, _, J1 = _solve(oracle, TR.killed_ell(ell, f), W0, 1.0)
    _, _, _, J2 = _solve(oracle, TR.killed_ell(ell, f), W1, 1.5, J=J1)
    assert (np.abs(TR.hit(A, J2, f) - cdf) <= 2 * bj).all()


@pytest.mark.parametrize("name", ["toggle_fsp_231", "toggle_box_21x13"])
def test_mass_balance_and_duality(oracle, golden_dir, name):
    """wsum + hit + leak = 1 with leak = -1^T A J (the mass that left the FSP), and w0 . J_back(g) = hit for g = D A^T 1_T"""
    ell, t = IR.small_cases(golden_dir)[name]
    A = IR.dense_of_ell(ell)
    n = A.shape[0]
    f = TR.random_set(n)
    keep = f == 0
    rng = np.random.default_rng(4)
    W0 = np.zeros((n, 2))
    W0[np.flatnonzero(keep)[n // 5], 0] = 1.0
    p = rng.random(n) * keep
    W0[:, 1] = p / p.sum()
    kell = TR.killed_ell(ell, f)
    W, ws, st, J = _solve(oracle, kell, W0, t)
    assert st.nstep >= 2
    h = TR.hit(A, J, f)
    leak_rate = -A.sum(axis=0)                                     # >= 0: what leaves the FSP per unit of time
    leak = leak_rate @ J
    bj = TR.hit_bound_J(A, f, t, 1.0)
    bal = np.abs(ws + h + leak - 1.0)
    bound_bal = bj + np.abs(leak_rate).max() * J_REL_BOUND * t + TR.W_L1_TOL
    print(name, "hit", h, "leak", leak, "balance err/bound", bal.max() / bound_bal)
    assert (h > 1e-3).all() and (bal <= bound_bal).all()
    # backward: g = D A^T 1_T, the rate into the set per start state
    g = (A.T @ f.astype(np.float64)) * keep
    _, _, _, Jb = _solve(oracle, kell, g[:, None], t, transposed=True)
    dual = W0.T @ Jb[:, 0]
    bound_dual = bj + np.abs(W0).max(axis=0) * J_REL_BOUND * t * np.abs(g).sum()
    print(name, "duality err/bound", (np.abs(dual - h) / bound_dual).max())
    assert (np.abs(dual - h) <= bound_dual).all()


def test_mask_in_the_update_is_arnoldi_on_the_killed_generator():
    """the argument of DESIGN.md 12 "Target sets": IOP(2) Arnoldi with z = A u raw, the dots u . z taken from the raw z and
    the set zeroed in the update only, gives the H and the basis of Arnoldi on the dense D A D - exactly"""
    ell = TR.birth_chain(N, LAM).ell()
    A = IR.dense_of_ell(ell)
    A[np.arange(1, N), np.arange(N - 1)] += np.linspace(0.1, 1.0, N - 1)      # (not nilpotent: no breakdown below)
    A[np.arange(N - 1), np.arange(1, N)] += 0.7
    f = np.zeros(N, dtype=bool)
    f[[3, 17, 18, 40]] = True
    D = np.diag(1.0 - f)
    Q = D @ A @ D

    def iop2(op, mask, m=8):
        u = [None, np.where(f, 0.0, 1.0 / np.arange(1, N + 1))]            # u_1 = D w on both sides
        u[1] = u[1] / np.linalg.norm(u[1])
        H = np.zeros((m + 2, m + 1))
        for j in range(1, m + 1):
            z = op @ u[j]
            for i in (j - 1, j):
                if i >= 1:
                    H[i, j] = u[i] @ z
                    z = z - H[i, j] * u[i]
            z = np.where(mask, 0.0, z)
            H[j + 1, j] = np.linalg.norm(z)
            u.append(z / H[j + 1, j])
        return H, np.array(u[1:])

    Hm, Um = iop2(A, f)
    Hq, Uq = iop2(Q, np.zeros(N, dtype=bool))
    assert np.array_equal(Hm, Hq) and np.array_equal(Um, Uq)
    assert not Um[:, f].any()


def test_surface_is_declared_and_documented():
    hdr = open(os.path.join(ROOT, "include", "kfsp.h")).read()
    api = open(os.path.join(ROOT, "krylovfspssa_amd", "csrc", "kfsp_api.cpp")).read()
    assert "TARGET SETS" in hdr and '"block_target"' in hdr and 'k == "block_target"' in api
    for mode in ('"block_target" = 1, kfsp_set_block(', '"block_target" = 2, kfsp_block_info(', '"block_target" = 3, kfsp_block_begin('):
        assert mode in hdr
    blk = open(os.path.join(ROOT, "krylovfspssa_amd", "csrc", "kfsp_block.hip")).read()
    for kern in ("k_btarget_zero(", "k_bhit(", "template <bool TARGET>"):
        assert kern in blk
    assert "Target sets" in open(os.path.join(ROOT, "DESIGN.md")).read()


class _Recorder:
    def __init__(self):
        self.calls = []

    def kfsp_set_option(self, h, name, value):
        self.calls.append((name.decode(), value))
        return 0

    def kfsp_set_block(self, h, k, n, ld, flags):
        got = None if not flags else np.ctypeslib.as_array(ctypes.cast(flags, ctypes.POINTER(ctypes.c_double)), shape=(n,)).copy()
        self.calls.append((k, n, got))
        return 0


def test_python_hands_over_flags_or_clears_under_the_call_mode():
    from krylovfspssa_amd.host import KfspContext
    c = object.__new__(KfspContext)
    c._lib = _Recorder()
    c._h = ctypes.c_void_p()
    c.n = 5
    c.set_block_target(np.array([0.0, 2.5, 0.0, -1.0, 0.0]))
    c.set_block_target([True, False, False, False, True])
    c.set_block_target(None)
    calls = c._lib.calls
    assert calls[0::3] == [("block_target", 1)] * 3 and calls[2::3] == [("block_target", 0)] * 3    # the mode round each call
    (k1, n1, f1), (k2, n2, f2), (k3, n3, f3) = calls[1::3]
    assert (k1, n1) == (1, 5) and f1.tolist() == [0, 1, 0, 1, 0]
    assert (k2, n2) == (1, 5) and f2.tolist() == [1, 0, 0, 0, 1]
    assert n3 == 0 and f3 is None
