"""CPU-side checks of the block entry points (several start vectors at once): declared, exported, a null context is
refused, and the Python mirror checks shapes and k before it calls the library.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

BLOCK_ENTRY_POINTS = ("kfsp_set_block", "kfsp_get_block", "kfsp_spmm", "kfsp_expv_block", "kfsp_spmm_bench")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kfsp.h")).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from krylovfspssa_amd import build, host
    build.build_lib()
    return host.load_library()


def test_block_entry_points_are_declared_and_exported(lib):
    text = _header()
    for name in BLOCK_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert re.search(r"}\s*kfsp_block_stats\s*;", text)
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in BLOCK_ENTRY_POINTS)


def test_block_stats_layout_matches_the_header():
    from krylovfspssa_amd.host import BlockStats
    body = re.search(r"typedef struct\s*{([^{}]*)}\s*kfsp_block_stats", _header()).group(1)
    ints = re.search(r"int32_t([^;]*);", body).group(1).split(",")
    dbls = re.search(r"double([^;]*);", body).group(1).split(",")
    names = [f[0] for f in BlockStats._fields_]
    assert names == [x.strip() for x in ints] + [x.strip() for x in dbls]
    assert ctypes.sizeof(BlockStats) == 4 * len(ints) + 8 * len(dbls)


def test_null_context_is_refused(lib):
    w = np.zeros(4)
    ms = ctypes.c_float(0.0)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert lib.kfsp_set_block(None, 1, 4, 4, p) == -1
    assert lib.kfsp_get_block(None, 1, 4, 4, p) == -1
    assert lib.kfsp_spmm(None, 1, 4, p, p) == -1
    assert lib.kfsp_expv_block(None, 1.0, 1e-8, 30, p, None) == -1
    assert lib.kfsp_spmm_bench(None, 1, ctypes.byref(ms)) == -1


class _NoCalls:
    """stands in for the library: any call is a test failure"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def _ctx(n):
    from krylovfspssa_amd.host import KfspContext
    c = object.__new__(KfspContext)
    c._lib = _NoCalls()
    c._h = ctypes.c_void_p()
    c.n = n
    return c


@pytest.mark.parametrize("shape", [(10, 0), (10, 17), (9, 3), (10,), (10, 2, 1)])
def test_wrapper_checks_shapes_before_calling(shape):
    c = _ctx(10)
    X = np.zeros(shape)
    with pytest.raises(ValueError):
        c.set_block(X)
    with pytest.raises(ValueError):
        c.spmm(X)


def test_wrapper_needs_a_block_before_solving():
    from krylovfspssa_amd.host import KfspError
    c = _ctx(10)
    with pytest.raises(KfspError):
        c.expv_block(1.0, 1e-8)
    with pytest.raises(KfspError):
        c.get_block()
