"""A refused kfsp_set_matrix_box leaves the context and its resident generator alone: box_plan (csrc/kfsp_box_plan.h)
decides everything that can refuse a model before the entry point writes anything.  On a slab box of 16 384 rows with
format 8 resident, and once more with format 7 under its tiled base-trip order: four refused calls straight through the C
entry point - too many factors (-6), a factor species out of range (-7), a reaction that changes four species (-5) and
a smaller two-species box whose tables exceed the 48 KB they may take (-8) - each followed by the four host-side records
unchanged, before anything is launched, and then by one product that must be the restated rows.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import box_cases as BC

pytestmark = pytest.mark.gpu

NAME = "slab_8x8x8x8x2x2"


def _records(k):
    n = C.c_int64(0)
    assert k._lib.kfsp_num_states(k._h, C.byref(n)) == 0
    return dict(num_states=n.value, matrix_info=k.matrix_info(), layout_info=k.layout_info(), build_info=k.build_info())


def _arguments(mdl):
    dims = np.ascontiguousarray(mdl.dims, dtype=np.int32)
    stoich = np.ascontiguousarray(np.asarray(mdl.stoich).T, dtype=np.int32)        # [nr][ns]
    ndep, deps, tables = mdl.factors()
    return [dims, stoich, np.ascontiguousarray(ndep, dtype=np.int32), np.ascontiguousarray(deps, dtype=np.int32),
            np.ascontiguousarray(tables, dtype=np.float64)]


def _refused(mdl):
    """(what, code, text, the five arrays) of the four refused calls"""
    out = []
    a = _arguments(mdl)
    a[2][0] = 4
    out.append(("four factors", -6, "1 <= ndep <= 3 factors per propensity", a))
    a = _arguments(mdl)
    a[3][0, 0] = len(mdl.dims)
    out.append(("a factor species equal to ns", -7, "factor species out of range", a))
    a = _arguments(mdl)
    a[1][0, :4] = 1
    out.append(("a reaction that changes four species", -5, "a reaction changes more than 3 species", a))
    # birth and death of the first of two species: two tables of 3001 entries, 6002 > 6000 - 2; 6002 states
    a = [np.array([3001, 2], dtype=np.int32), np.array([[1, 0], [-1, 0]], dtype=np.int32), np.array([1, 1], dtype=np.int32),
         np.zeros((2, 3), dtype=np.int32), np.ones(6002)]
    out.append(("tables beyond 48 KB", -8, "factor tables exceed the 48 KB they may take in LDS", a))
    return out


@pytest.mark.parametrize("options,fmt,order", [(dict(box_pencil=2), 8, 0), (dict(box_pencil=1, box_tile=1), 7, 64)], ids=["slabs", "tiled-pencils"])
def test_a_refused_box_leaves_context_and_generator_untouched(options, fmt, order):
    from krylovfspssa_amd import KfspContext
    from krylovfspssa_amd.host import _p
    c = BC.gated_case(NAME)
    assert c["n"] == 16384
    with KfspContext(0) as k:
        k.set_option("small_kernel", 0)
        for name, v in options.items():
            k.set_option(name, v)
        k.set_matrix_box(c["mdl"], store=False)
        before = _records(k)
        assert before["num_states"] == c["n"] == before["matrix_info"]["rows"]
        assert before["layout_info"]["format"] == fmt and before["build_info"]["pencil_order"] == order, before
        for what, code, text, (dims, stoich, ndep, deps, tables) in _refused(c["mdl"]):
            rc = k._lib.kfsp_set_matrix_box(k._h, len(dims), _p(dims), stoich.shape[0], _p(stoich), _p(ndep), _p(deps), _p(tables))
            assert rc == code and k._lib.kfsp_last_error(k._h).decode() == text, (what, rc, k._lib.kfsp_last_error(k._h))
            assert _records(k) == before, (what, _records(k), before)            # ... before anything is launched
            bad = BC.mismatches(k.spmv(c["x"]), c["y"])
            assert bad.size == 0, f"{what}: {bad.size} of {c['n']} rows differ from the restatement, first {bad[:5]}"
