"""CPU-side checks of the block pass entry points and option block_small: declared, documented, exported, a null
context is refused, the Python mirror checks before it calls - and the adaptive case of tests/test_gpu_block_small.py
keeps its step decisions when every ERR_LOC moves by 1e-3 relative (the margin DESIGN.md 12 names).  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

ENTRY_POINTS = ("kfsp_block_begin", "kfsp_block_arnoldi", "kfsp_block_combine", "kfsp_block_info")


def _raw_header():
    return open(os.path.join(ROOT, "include", "kfsp.h")).read()


@pytest.fixture(scope="module")
def lib():
    from krylovfspssa_amd import build, host
    build.build_lib()
    return host.load_library()


def test_entry_points_are_declared_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", _raw_header(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in ENTRY_POINTS)


def test_entry_points_and_option_are_documented():
    hdr = _raw_header()
    comments = " ".join(re.findall(r"/\*.*?\*/", hdr, flags=re.S))
    for name in ENTRY_POINTS + ('"block_small"',):
        assert name in comments, name
    src = open(os.path.join(ROOT, "krylovfspssa_amd", "csrc", "kfsp_api.cpp")).read()
    assert 'k == "block_small"' in src


def test_null_context_is_refused(lib):
    w = np.zeros(16 * 3 * 102)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert lib.kfsp_block_begin(None, 30, p) == -1
    assert lib.kfsp_block_arnoldi(None, 30, 1e-7, p, p, p, p) == -1
    assert lib.kfsp_block_combine(None, 31, p, p) == -1
    assert lib.kfsp_block_info(None, p) == -1


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_wrappers_need_a_block_and_check_coef():
    from krylovfspssa_amd.host import KfspContext, KfspError
    c = object.__new__(KfspContext)
    c._lib = _NoCalls()
    c._h = ctypes.c_void_p()
    c.n = 10
    for call in (lambda: c.block_begin(5), lambda: c.block_arnoldi(5), lambda: c.block_combine(2, np.zeros((2, 1)))):
        with pytest.raises(KfspError):
            call()
    c.block_k = 3
    for coef in (np.zeros((2, 2)), np.zeros((1, 3)), np.zeros(3)):
        with pytest.raises(ValueError):
            c.block_combine(2, coef)


def test_adaptive_case_keeps_its_decisions_under_a_1e3_change_of_err_loc(monkeypatch):
    """toggle(60, 50), t = 0.3, tol = 1e-8, m = 30, 6 columns: the GPU's ERR_LOC differ from the restatement's by
    rounding (~5e-6 relative); the counts and the accepted step sizes must not hinge on that"""
    from krylovfspssa_amd import synth
    from oracle import oracle as O
    from tests import block_ref as BR
    from tests.test_gpu_block_small import ADAPTIVE, _start
    t, tol, m, k = ADAPTIVE
    mdl = synth.toggle(60, 50)
    assert mdl.n <= 4096
    A = O.EllMatrix(*mdl.ell())
    W = _start(mdl.n, k, np.random.default_rng(7))
    plain = BR._Column.err_loc
    runs = []
    for f in (1.0, 1.0 + 1e-3, 1.0 - 1e-3):
        monkeypatch.setattr(BR._Column, "err_loc", lambda self, mm, f=f: f * plain(self, mm))
        st = BR.expv_block(A, W, t, tol, m)[2]
        runs.append((st.nstep, st.nreject, st.nmult, tuple(st.steps)))
    assert runs[0][0] >= 2 and runs[0][1] >= 1
    assert runs[1] == runs[0] and runs[2] == runs[0]
