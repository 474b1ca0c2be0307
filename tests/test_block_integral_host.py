"""Option block_integral without a GPU: the CPU restatement of the block solve with the time integral J
(tests/block_integral_ref.py) against dense integrals, the host routine that yields J's coefficients in a program of its
own under the sanitizers, and the option's surface."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

from tests import block_integral_ref as IR
from tests import block_ref as BR
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")

# Measured: the restatement against the dense integral on the three small generators of block_integral_ref.small_cases,
# forward and transposed, unclamped, tol in {1e-8, 1e-5} x m in {30, 10} ("Time integrals", has the table).
# The worst l1(J_ref - J_dense) / (t l1(w0)) was 7.24e-10 (toggle FSP forward, tol 1e-5, m 10), the worst residual
# l1(A J_ref - (W_ref(t) - W0)) / l1(w0) 3.78e-8 (toggle box forward, tol 1e-5, m 10).  Asserted: 4 x, for libm / BLAS
# differences between hosts.  The device is held to the same two numbers (tests/test_gpu_block_integral.py).
J_REL_BOUND = 4 * 7.24e-10
RESIDUAL_BOUND = 4 * 3.78e-8
CONFIGS = ((1e-8, 30), (1e-8, 10), (1e-5, 30), (1e-5, 10))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- 1. the restatement
def test_restatement_leaves_the_block_solve_alone(oracle, golden_dir):
    """W, wsum and every statistic are block_ref's, bit for bit: J enters nothing"""
    ell, t = IR.small_cases(golden_dir)["toggle_box_21x13"]
    A = oracle.EllMatrix(*ell)
    W0 = IR.start_block(A.n, False)
    for clamp in (True, False):
        W, ws, st, J = IR.expv_block_integral(A, W0, t, 1e-8, 30, clamp=clamp)
        Wr, wsr, str_ = BR.expv_block(A, W0, t, 1e-8, 30, clamp=clamp)
        assert np.array_equal(_bits(W), _bits(Wr)) and np.array_equal(_bits(ws), _bits(wsr))
        assert st == str_ and st.nstep >= 2
        assert np.isfinite(J).all() and J[:, 1].min() > -1e-12


def test_fused_combine_restated_exactly():
    """combine_int_exact against numpy's sums to rounding, the clamp on W only, J continued from the old J"""
    rng = np.random.default_rng(2)
    n, k, mx = 37, 3, 5
    U = rng.standard_normal((mx, n, k))
    coef, cj = rng.standard_normal((mx, k)), rng.standard_normal((mx, k))
    cj[2] = 0.0
    J0 = rng.standard_normal((n, k))
    for clamp in (True, False):
        W, J = IR.combine_int_exact(U, coef, cj, J0, clamp)
        w = np.einsum("jc,jnc->nc", coef, U)
        assert np.allclose(W, np.maximum(w, 0.0) if clamp else w, rtol=0, atol=1e-14 * np.abs(coef).sum())
        assert np.allclose(J, J0 + np.einsum("jc,jnc->nc", cj, U), rtol=0, atol=1e-14 * (1 + np.abs(cj).sum()))
        assert (J < 0).any()
    W1, J1 = IR.combine_int_exact(U, coef, np.zeros((mx, k)), J0, True)
    assert np.array_equal(_bits(J1), _bits(J0))               # a table of zeros: fma(0, u, r) = r


# ---- 2. the phi_1 column of the library, in a program of its own under ASan / UBSan
def _band(m, mbrk, k1, rng):
    """an augmented Hessenberg matrix as the block time loop builds it (leading dimension m + 2): the IOP(2) band of
    mbrk columns, H(m+2, m+1) = 1, and for a breakdown (k1 = 0) the exact mbrk x mbrk H"""
    mh = m + 2
    H = np.zeros((mh, mh), order="F")
    for j in range(mbrk):
        H[j, j] = -rng.uniform(1.0, 40.0)
        if j >= 1:
            H[j - 1, j] = rng.uniform(-5.0, 20.0)
        if j + 1 < mbrk or k1:
            H[j + 1, j] = rng.uniform(0.5, 25.0)
    H[m + 1, m] = 1.0
    return H


def _phi_cases():
    rng = np.random.default_rng(12)
    return [  # (m, mbrk, k1, tau, H)
        (3, 3, 2, 0.05, _band(3, 3, 2, rng)),
        (10, 7, 0, 0.2, _band(10, 7, 0, rng)),                 # broke down after column 7
        (30, 30, 2, 0.011, _band(30, 30, 2, rng)),
        (30, 1, 0, 0.37, np.zeros((32, 32), order="F")),        # A v_1 = 0: a null H
    ]


def _hex(x):
    return float(x).hex()


def test_phi1_column_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_integral_check")
    # host code only: the sanitizers go to the host side of the compile and nothing is built for a device
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-I" + CSRC,
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-pthread", os.path.join(ROOT, "tests", "block_integral_check.cpp"), "-x", "c++",
           os.path.join(CSRC, "kfsp_padm.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    cases = _phi_cases()
    inp = tmp_path / "cases.txt"
    with open(inp, "w") as f:
        for m, mbrk, k1, tau, H in cases:
            mh, rows = mbrk + k1, mbrk + max(0, k1 - 1)
            f.write(f"{mh} {rows} {m + 2} {_hex(tau)}\n")
            f.write(" ".join(_hex(x) for x in H[:, :mh].ravel(order="F")) + "\n")
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == "ok"
    for (m, mbrk, k1, tau, H), line in zip(cases, lines):
        mh, rows = mbrk + k1, mbrk + max(0, k1 - 1)
        g = np.array([float.fromhex(x) for x in line.split()[1:]])
        assert line.startswith("g ") and g.shape == (rows,)
        Hh = np.zeros((mh + 1, mh + 1))
        Hh[:mh, :mh] = H[:mh, :mh]
        Hh[0, mh] = 1.0
        ref = sl.expm(tau * Hh)[:mh, mh]
        print("m", m, "mbrk", mbrk, "k1", k1, "max err", np.abs(g - ref[:rows]).max(), "max|column|", np.abs(ref).max())
        assert np.abs(g - ref[:rows]).max() <= 1e-13 * np.abs(ref).max(), (m, mbrk, k1)
        if not H[:mh, :mh].any():
            assert g[0] == tau and not g[1:].any()            # exactly tau e_1
        # the restatement's column is the same quantity
        assert np.abs(IR.integral_column(np.array(H[:mh, :mh], order="F"), tau)[:rows] - ref[:rows]).max() <= 1e-13 * np.abs(ref).max()


# ---- 3. the restatement against the dense integral
@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("name", ["toggle_fsp_231", "toggle_box_21x13", "death_chain"])
def test_restatement_against_the_dense_integral(oracle, golden_dir, name, transposed):
    ell, t = IR.small_cases(golden_dir)[name]
    for tol, m in CONFIGS:
        err, res, nstep = IR.accuracy(ell, transposed, t, tol, m)
        print(name, "transposed" if transposed else "forward", "tol", tol, "m", m, "steps", nstep,
              "l1(J_ref - J_dense) / (t l1(w0))", err, "l1(A J - (W - W0)) / l1(w0)", res)
        assert nstep >= 2
        assert err <= J_REL_BOUND, (name, transposed, tol, m, err)
        assert res <= RESIDUAL_BOUND, (name, transposed, tol, m, res)


def test_special_columns_of_the_restatement(oracle):
    """a zero column keeps J = 0 exactly; the absorbing start state (A v_1 = 0, a null H) gives J = t W0 to an ulp per
    step; a column that breaks down (an eigenvector) is integrated on its exact H: J = 2 (1 - exp(-t / 2)) f on the death
    chain, backward"""
    N, b, gam, t = 40, 6.0, 1.0, 0.5
    adj = np.zeros((N, 2), dtype=np.int32)
    off = np.zeros((N, 2))
    diag = np.zeros(N)
    for i in range(N):
        if 0 < i < N - 1:
            adj[i, 0], off[i, 0] = i + 2, b
        if i > 0:
            adj[i, 1], off[i, 1] = i, gam * i
        diag[i] = off[i].sum() + (b if i == N - 1 else 0.0)
    W0 = np.zeros((N, 3))
    W0[0, 0] = 1.0
    W0[20, 2] = 1.0
    W, ws, st, J = IR.expv_block_integral(oracle.EllMatrix(adj, off, diag), W0, t, 1e-10, 10, clamp=False)
    assert st.nstep >= 2
    assert np.array_equal(_bits(J[:, 1]), _bits(np.zeros(N)))
    assert not J[1:, 0].any() and abs(J[0, 0] - t) <= st.nstep * np.spacing(t)
    Jd = IR.dense_integral(IR.dense_of_ell((adj, off, diag)), W0, t)
    assert np.abs(J[:, 2] - Jd[:, 2]).sum() <= J_REL_BOUND * t

    ell = IR.death_chain().ell()
    f = np.arange(len(ell[2]), dtype=np.float64)[:, None]
    AT = oracle.EllMatrix(*BR.transpose_ell(*ell))
    for t in (0.7, 3.0):
        W, ws, st, J = IR.expv_block_integral(AT, f, t, 1e-8, 30, clamp=False)
        assert st.n_breakdown_cols == 1
        want = 2.0 * (1.0 - np.exp(-t / 2.0)) * f
        assert np.abs(J - want).sum() <= J_REL_BOUND * t * f.sum()


def test_two_calls_accumulate(oracle, golden_dir):
    ell, _ = IR.small_cases(golden_dir)["toggle_box_21x13"]
    A = oracle.EllMatrix(*ell)
    W0 = IR.start_block(A.n, False)
    W1, _, _, J1 = IR.expv_block_integral(A, W0, 0.1, 1e-8, 30, clamp=False)
    W2, _, _, J2 = IR.expv_block_integral(A, W1, 0.2, 1e-8, 30, clamp=False, J=J1)
    Jd = IR.dense_integral(IR.dense_of_ell(ell), W0, 0.1 + 0.2)
    assert (np.abs(J2 - Jd).sum(axis=0) <= J_REL_BOUND * 0.3 * np.abs(W0).sum(axis=0)).all()


# ---- 4. the option's surface
def test_option_is_known_and_documented():
    hdr = open(os.path.join(ROOT, "include", "kfsp.h")).read()
    api = open(os.path.join(CSRC, "kfsp_api.cpp")).read()
    assert '"block_integral"' in hdr and 'k == "block_integral"' in api
    assert "TIME INTEGRALS" in hdr
    from krylovfspssa_amd import build
    before = ["kfsp_api.cpp", "kfsp_comm.cpp", "kfsp_group.cpp", "kfsp_padm.cpp", "kfsp_stepper.cpp", "kfsp_kernels.hip", "kfsp_build.hip",
              "kfsp_drop.hip", "kfsp_expand.hip", "kfsp_prop.hip", "kfsp_ssa.hip", "kfsp_block.hip", "kfsp_block_adj.hip"]
    assert build.SOURCES[:len(before)] == before
    assert "kfsp_block_integral.h" in build.HEADERS
    blk = open(os.path.join(CSRC, "kfsp_block.hip")).read()
    assert "k_bcombine_int(" in blk and "k_bcombine_small_int(" in blk


class _Recorder:
    def __init__(self):
        self.calls = []

    def kfsp_set_option(self, h, name, value):
        self.calls.append((name.decode(), value))
        return 0

    def kfsp_get_block(self, *a):
        self.calls.append(("get_block",))
        return 0

    def kfsp_block_combine(self, h, mx, coef, ws):
        tab = np.ctypeslib.as_array(ctypes.cast(coef, ctypes.POINTER(ctypes.c_double)), shape=(2 * mx, 16)).copy()
        self.calls.append(("combine", mx, tab))
        return 0


def _mirror():
    from krylovfspssa_amd.host import KfspContext
    c = object.__new__(KfspContext)
    c._lib = _Recorder()
    c._h = ctypes.c_void_p()
    c.n = 4
    c.block_k = 3
    return c


def test_get_block_sets_and_restores_the_option():
    c = _mirror()
    c.get_block()
    assert c._lib.calls == [("get_block",)]                    # W: no option is touched
    c._lib.calls.clear()
    c.get_block(integral=True)
    assert c._lib.calls == [("block_integral", 2), ("get_block",), ("block_integral", 0)]
    c._lib.calls.clear()
    c.set_option("block_integral", 1)
    c.get_block(integral=True)
    assert c._lib.calls == [("block_integral", 1), ("block_integral", 2), ("get_block",), ("block_integral", 1)]


def test_block_combine_hands_over_the_second_table_or_refuses():
    c = _mirror()
    coef = np.arange(15, dtype=np.float64).reshape(5, 3) + 1.0
    cj = -coef
    c.block_combine(4, coef, coef_integral=cj)
    (_, mx, tab), = c._lib.calls
    assert mx == 4 and np.array_equal(tab[:4, :3], coef[:4]) and np.array_equal(tab[4:, :3], cj[:4]) and not tab[:, 3:].any()
    c._lib.calls.clear()
    c.block_combine(4, coef)
    assert not c._lib.calls[0][2][4:].any()                    # no table: zeros, J stays as it is
    c._lib.calls.clear()
    for bad in (np.ones((3, 3)), np.ones((5, 2)), np.ones((5, 4)), np.ones(15)):
        with pytest.raises(ValueError, match="coef_integral"):
            c.block_combine(4, coef, coef_integral=bad)
    assert c._lib.calls == []                                  # refused before the library is called
