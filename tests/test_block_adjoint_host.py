"""Backward solves on the block path (option adjoint), the part that needs no GPU: numpy restatements of the three row
definitions of A^T X - banded with the range test, ELL with missing targets, the matrix-free box with the in-box test -
checked against A^T assembled from synth (tests/test_gpu_block_adjoint.py imports them); the library's C surface is what
it was; the host-side descriptor and residency checks run under AddressSanitizer / UBSan in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def _synth():
    from krylovfspssa_amd import synth
    return synth


# ---- A as a host CSR, from the gather rows or from the reference arrays
def csr_of_model(mdl):
    rp, col, val = mdl.csr_rows()
    return sp.csr_matrix((val, col, rp), shape=(mdl.n, mdl.n))


def csr_of_ell(adj, off, diag):
    """A(ADJ(k, c) - 1, c) += OFFDIAG(k, c) for the targets inside [1, n]; A(c, c) -= DIAG(c)"""
    n, bw = adj.shape
    c = np.repeat(np.arange(n), bw)
    t = adj.reshape(-1).astype(np.int64) - 1
    ok = (t >= 0) & (t < n)
    A = sp.coo_matrix((off.reshape(-1)[ok], (t[ok], c[ok])), shape=(n, n)).tocsr()
    return (A - sp.diags(diag)).tocsr()


def bound(A, X, f=1e-13):
    """the tolerance of the forward parity tests, transposed: f (|A|^T |X|) per entry"""
    return f * (abs(A).T @ np.abs(X))


# ---- the three row definitions
def banded_form(mdl):
    """(delta ascending, val[d, r] = A(r, r + delta_d), diag) of a box: what the banded image stores"""
    cols, vals = mdl.rows_at(np.arange(mdl.n, dtype=np.int64))
    delta = np.unique(-mdl.offsets)
    assert len(delta) == mdl.R and 0 not in delta
    val = np.zeros((len(delta), mdl.n))
    diag = np.zeros(mdl.n)
    rows = np.arange(mdl.n)
    big = np.iinfo(np.int64).max
    for j in range(cols.shape[1]):
        c, v = cols[:, j], vals[:, j]
        here = c != big
        own = here & (c == rows)
        diag[own] = -v[own]
        offd = here & ~own
        d = np.searchsorted(delta, c[offd] - rows[offd])
        val[d, rows[offd]] = v[offd]
    return delta, val, diag


def banded_t(delta, val, diag, X):
    """row r: s = -(diag x_r), then per diagonal d ascending src = r - delta_d, ok = 0 <= src < n, the value
    ok ? val[d, src] : 0 against X row ok ? src : r"""
    n = X.shape[0]
    r = np.arange(n)
    s = -(diag[:, None] * X)
    for d in range(len(delta)):
        src = r - delta[d]
        ok = (src >= 0) & (src < n)
        v = np.where(ok, val[d, np.where(ok, src, 0)], 0.0)
        s = s + v[:, None] * X[np.where(ok, src, r)]
    return s


def ell_t(adj, off, diag, X):
    """row c: s = -(diag x_c), then per slot k ascending OFFDIAG(k, c) X[ADJ(k, c)]; a missing target (ADJ outside
    [1, n]) counts as 0 against the row's own X row"""
    n, bw = adj.shape
    c = np.arange(n)
    s = -(diag[:, None] * X)
    for k in range(bw):
        t = adj[:, k].astype(np.int64) - 1
        ok = (t >= 0) & (t < n)
        v = np.where(ok, off[:, k], 0.0)
        s = s + v[:, None] * X[np.where(ok, t, c)]
    return s


def box_t(mdl, X):
    """row r at coordinates x: the accumulator starts at 0; per species s, then per reaction whose propensity depends on
    s by ascending source offset, a_k(x) against X row r + delta_k when x + nu_k lies inside the box (else 0 against the
    row's own row); then -dsum x_r with dsum the species' shares added in species order"""
    r = np.arange(mdl.n, dtype=np.int64)
    C = mdl.coords(r)
    Cf = [c.astype(np.float64) for c in C]
    order = np.argsort(-mdl.offsets, kind="stable")          # ascending source offset
    acc = np.zeros_like(X)
    dsum = np.zeros(mdl.n)
    for s in range(mdl.d):
        share = np.zeros(mdl.n)
        for k in order:
            if tuple(mdl.deps[k])[0] != s:
                continue
            a = mdl.prop(k, Cf) * np.ones(mdl.n)
            ok = np.ones(mdl.n, dtype=bool)
            for q in range(mdl.d):
                y = C[q] + mdl.stoich[q, k]
                ok &= (y >= 0) & (y < mdl.dims[q])
            acc = acc + np.where(ok, a, 0.0)[:, None] * X[np.where(ok, r + mdl.offsets[k], r)]
            share = share + a
        dsum = dsum + share
    return acc + (-dsum)[:, None] * X


def columns(n, k, rng):
    """one all-negative column, one unit vector, one all-positive column; the rest random"""
    X = rng.standard_normal((n, k))
    X[:, 0] = -np.abs(X[:, 0]) - 0.25
    if k > 1:
        X[:, 1] = 0.0
        X[n // 3, 1] = 1.0
    if k > 2:
        X[:, 2] = np.abs(X[:, 2]) + 0.25
    return X


def four_slot_box():
    """tests/test_gpu_block_box.py's box of the 6-species / 4-slot instantiation"""
    st = [[1, -1, 2, -2, 0, 0], [0, 0, 0, 0, 1, -1]]

    def prop(r, X):
        x, y = X
        return (np.full_like(x, 5.0), 0.7 * x, 1.5 + 0.01 * x, 0.02 * x * (x - 1.0), 3.0 + 0.1 * y, 0.9 * y)[r]
    return _synth().BoxModel("four_slot", (37, 29), st, prop, deps=[(0,), (0,), (0,), (0,), (1,), (1,)])


def death_chain(N=201, g=0.5):
    """pure death on [0, N - 1]: a(x) = g x, nothing leaves the box; A^T f = -g f for f(x) = x"""
    return _synth().BoxModel("death", (N,), [[-1]], lambda r, X: g * X[0], deps=[(0,)])


BOXES = {
    "toggle_40x33": lambda: _synth().toggle(40, 33),
    "toggle_70x61": lambda: _synth().toggle(70, 61),
    "toggle_23x19": lambda: _synth().toggle(23, 19),
    "toggle_2x2": lambda: _synth().toggle(60, 50),
    "repressilator_3x2": lambda: _synth().repressilator(dims=(13, 11, 7)),
    "birth_death_6x2": lambda: _synth().birth_death((5, 6, 4, 5, 3, 4)),
    "four_slot_6x4": four_slot_box,
    "one_species": lambda: _synth().birth_death((1000,)),
    "masked_1000x3": lambda: _synth().toggle(1000, 3),
    "death_chain": death_chain,
}


@pytest.mark.parametrize("kind", list(BOXES))
def test_row_definitions_against_the_assembled_transpose(kind):
    mdl = BOXES[kind]()
    A = csr_of_model(mdl)
    X = columns(mdl.n, 5, np.random.default_rng(3))
    ref = A.T @ X
    tol = bound(A, X)
    for name, Y in (("banded", banded_t(*banded_form(mdl), X)), ("ell", ell_t(*mdl.ell(), X)), ("box", box_t(mdl, X))):
        assert np.all(np.abs(Y - ref) <= tol), (kind, name, np.abs(Y - ref).max())
    E = csr_of_ell(*mdl.ell())
    assert abs(E - A).max() <= 1e-13 * abs(A).max()


def test_ell_definition_on_the_golden_fsp(golden_dir):
    """an SSA-grown FSP: targets outside the FSP are missing links"""
    from tests import block_generators
    g = block_generators.golden_toggle(golden_dir)
    adj, off, diag = g["adj"], g["offdiag"], g["diag"]
    assert ((adj < 1) | (adj > len(diag))).any()
    A = csr_of_ell(adj, off, diag)
    X = columns(len(diag), 5, np.random.default_rng(4))
    assert np.all(np.abs(ell_t(adj, off, diag, X) - A.T @ X) <= bound(A, X))
    # nothing enters from outside, the missing links only take mass away: column sums of A are <= 0, so A^T 1 <= 0
    assert np.all(A.T @ np.ones(len(diag)) <= 1e-12)


def test_eigenvector_of_the_death_chain():
    mdl = death_chain()
    f = np.arange(mdl.n, dtype=np.float64)[:, None]
    assert np.array_equal(box_t(mdl, f), -0.5 * f)


# ---- library surface
def test_the_library_exports_no_new_entry_point(golden_dir):
    from krylovfspssa_amd import build
    lib = build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split())
    before = open(os.path.join(golden_dir, "exported_kfsp_symbols.txt")).read().split()
    assert [s for s in names if s.startswith("kfsp_")] == before
    for s in names:
        assert not any(t in s for t in ("spmm_t", "spmm_ell_t", "spmm_box_t", "box_adj_build", "ell_adj_resident")), s


def test_options_are_known_and_documented():
    hdr = open(os.path.join(ROOT, "include", "kfsp.h")).read()
    api = open(os.path.join(CSRC, "kfsp_api.cpp")).read()
    for name in ("adjoint", "block_clamp"):
        assert f'"{name}"' in hdr and f'k == "{name}"' in api, name
    from krylovfspssa_amd import build
    assert "kfsp_block_adj.hip" in build.SOURCES


class _Recorder:
    def __init__(self):
        self.calls = []

    def kfsp_set_option(self, h, name, value):
        self.calls.append((name.decode(), value))
        return 0

    def kfsp_spmm(self, *a):
        self.calls.append(("spmm",))
        return 0

    def kfsp_expv_block(self, *a):
        self.calls.append(("expv",))
        return 0


def test_wrappers_set_and_restore_the_options():
    import ctypes
    from krylovfspssa_amd.host import KfspContext
    c = object.__new__(KfspContext)
    c._lib = _Recorder()
    c._h = ctypes.c_void_p()
    c.n = 4
    c.block_k = 2
    X = np.ones((4, 2))
    c.spmm(X)
    assert c._lib.calls == [("spmm",)]                       # the forward call touches no option
    c._lib.calls.clear()
    c.spmm(X, adjoint=True)
    assert c._lib.calls == [("adjoint", 1), ("spmm",), ("adjoint", 0)]
    c._lib.calls.clear()
    c.expv_block(0.1, 1e-8, adjoint=True, clamp=False)
    assert c._lib.calls == [("adjoint", 1), ("block_clamp", 0), ("expv",), ("adjoint", 0), ("block_clamp", 1)]
    c._lib.calls.clear()
    c.set_option("adjoint", 1)                               # set by hand: stays set round a call that overrides nothing
    c.expv_block(0.1, 1e-8)
    assert c._lib.calls == [("adjoint", 1), ("expv",)]


# ---- the host-side checks under the sanitizers, in a program of their own
def test_host_checks_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "adj_host_check")
    src = os.path.join(ROOT, "tests", "adj_host_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
