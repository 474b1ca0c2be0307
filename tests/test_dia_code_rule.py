"""Host side of the dictionary-coded banded form: the rule that picks the code width from the number
of distinct values per diagonal and the LDS the dictionaries may take.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rule():
    from krylovfspssa_amd import build, host
    build.build_lib()
    lib = host.load_library()

    def f(distinct, lds=-1):
        d = np.ascontiguousarray(distinct, dtype=np.int64)
        w, r = C.c_int32(-1), C.c_int32(-1)
        assert lib.kfsp_dia_code_rule(len(d), d.ctypes.data_as(C.c_void_p), lds, C.byref(w), C.byref(r)) == 0
        return w.value, r.value
    return f


def test_width_follows_the_largest_dictionary(rule):
    assert rule([171] * 6) == (8, 8)                 # the repressilator box 171^3
    assert rule([256] * 8) == (8, 8)
    assert rule([256] * 9) == (8, 16)                # more than 8 one-byte codes: a 16-byte record
    assert rule([256] * 16) == (8, 16)               # 16 x 256 x 8 B = 32 KB: the 8-bit form always fits the 40 KB
    assert rule([257, 3, 3, 3]) == (16, 8)
    assert rule([1000] * 4) == (16, 8)               # toggle 1000 x 1000: 32 KB of dictionaries
    assert rule([500] * 5) == (16, 16)
    assert rule([500] * 8) == (16, 16)


def test_no_coded_image_beyond_the_budget(rule):
    assert rule([1001] * 4) == (16, 8) and rule([1281] * 4) == (0, 0)      # 4 x 1281 x 8 B > 40 KB
    assert rule([5120]) == (16, 8) and rule([5121]) == (0, 0)
    assert rule([65537]) == (0, 0)
    assert rule([65536], lds=1 << 20) == (16, 8) and rule([65537], lds=1 << 20) == (0, 0)
    assert rule([300] * 9) == (0, 0)                 # nine two-byte codes do not fit a 16-byte record
    assert rule([0, 5]) == (0, 0)                    # a diagonal that was not counted
    assert rule([3] * 17) == (0, 0)
    assert rule([1000] * 4, lds=16 * 1024) == (0, 0)
