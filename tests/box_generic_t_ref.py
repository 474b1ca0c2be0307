"""TEST HELPER - one row of the TRANSPOSED generic matrix-free block product (Y = A^T X under options block_box = 2 and
adjoint; k_spmm_boxg_t, the row code in kfsp_boxg_dev.h), restated with plain lists and row_ref.fma - beside
row_ref.box_generic_exact, which restates the forward row of the same kernel pair.

Row r at coordinates x, per column c:

    s = -(dsum X[r][c])                                   one rounded multiply
    for the sorted positions p ascending:                 (ascending source offset delta_p = -offsets[k], stable by reaction)
        s = fma(a_p(x), X[r - delta_p][c], s)             when x + nu_p lies in the box
        s = fma(0.0,    X[r][c],           s)             otherwise

a_k(x) = ((t_0[x] t_1[x]) t_2[x]) with every multiply rounded and the factors in the order model.factors() lists them; dsum
is the sum from 0.0 of a_k(x) in the MODEL's reaction order - both exactly as the forward row has them.  The propensity is
the one at the row's OWN coordinates; A is the truncated generator as the forward product applies it, so DIAG keeps the
propensities that leave the box.

`descending` takes the entries in the opposite order and `diag_last` starts from +0.0 and applies the diagonal as a closing
fma(-dsum, X[r][c], s): two WRONG kernels, used to show that a test case can tell them from the right one."""
import functools

import numpy as np

from tests.row_ref import _lists, fma


def box_generic_t_rows(mdl):
    """-> per row ([(a, X row)] by sorted position, dsum); no arithmetic on X"""
    stoich, offsets = _lists(mdl.stoich), [int(o) for o in _lists(mdl.offsets)]
    dims, strides = list(mdl.dims), [int(s) for s in _lists(mdl.strides)]
    ndep, dep, tab = (_lists(a) for a in mdl.factors())
    at, tables = 0, []
    for k in range(mdl.R):
        tables.append([])
        for i in range(ndep[k]):
            tables[k].append(tab[at:at + dims[dep[k][i]]])
            at += dims[dep[k][i]]
    order = sorted(range(mdl.R), key=lambda k: (-offsets[k], k))
    out = []
    for r in range(mdl.n):
        x = [(r // strides[s]) % dims[s] for s in range(mdl.d)]
        a = []
        for k in range(mdl.R):
            v = tables[k][0][x[dep[k][0]]]
            for i in range(1, ndep[k]):
                v = v * tables[k][i][x[dep[k][i]]]
            a.append(v)
        dsum = 0.0
        for k in range(mdl.R):
            dsum += a[k]
        ent = []
        for k in order:
            inside = all(0 <= x[q] + stoich[q][k] < dims[q] for q in range(mdl.d))
            ent.append((a[k], r + offsets[k]) if inside else (0.0, r))
        out.append((ent, dsum))
    return out


def box_generic_t_exact(mdl, X, descending=False, diag_last=False):
    """X: n rows of k numbers (lists or an (n, k) array) -> the n rows of A^T X as lists"""
    X = _lists(X)
    Y = []
    for r, (ent, dsum) in enumerate(box_generic_t_rows(mdl)):
        if descending:
            ent = ent[::-1]
        row = []
        for c in range(len(X[r])):
            s = 0.0 if diag_last else -(dsum * X[r][c])
            for a, src in ent:
                s = fma(a, X[src][c], s)
            row.append(fma(-dsum, X[r][c], s) if diag_last else s)
        Y.append(row)
    return Y


LOOP_DIMS = (7, 6, 5, 3, 3, 3)                  # the Goutsias box of 5 670 rows = 45 trips (the trip loop turns under grid_blocks = 8)


@functools.lru_cache(maxsize=None)
def model(name):
    from tests import box_cases as BC
    if name == "goutsias_loop":
        from krylovfspssa_amd import synth
        return synth.goutsias_box(LOOP_DIMS)
    return BC.model(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(mdl, X: adjoint_cases.block (three columns, magnitudes over six decades, one a unit vector), Y: the restated
    rows of A^T X); computed once per process and left alone"""
    from tests import adjoint_cases as AC
    from tests import box_cases as BC
    mdl = model(name)
    names = BC.generic_names() + ("goutsias_loop",) + BC.SMALL
    X = AC.block(mdl.n, 300 + names.index(name))
    Y = np.array(box_generic_t_exact(mdl, X))
    X.setflags(write=False)
    Y.setflags(write=False)
    return dict(mdl=mdl, X=X, Y=Y)
