"""Backward solves on the block path (option adjoint, kfsp_block_adj.hip): Y = A^T X against numpy on every form the
generator can be resident in, column by column independent of the block width on the bits, the forward product untouched,
the transpose identity, whole solves exp(tA^T) F against dense expm and against the forward solve (duality), an exact
eigenvector, the unclamped combine (option block_clamp), refusals and bookkeeping.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

from tests import block_generators
from tests.test_block_adjoint_host import (BOXES, bound, columns, csr_of_ell, csr_of_model, death_chain, ell_t)

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8, 16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


# ---- the forms: name -> setter(ctx, golden_dir) -> (A as host CSR, kfsp_layout_info format or None)
def _banded(kind, **opts):
    def f(ctx, golden_dir):
        mdl = BOXES[kind]()
        ctx.set_option("format", 0)
        ctx.set_option("dia_mask", 0)
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        return csr_of_model(mdl), 1
    return f


def _banded_trip_order(ctx, golden_dir):
    A, fmt = _banded("toggle_70x61")(ctx, golden_dir)
    ctx.set_trip_order(np.random.default_rng(3).permutation((ctx.n + 127) // 128))
    return A, fmt


def _masked(ctx, golden_dir):
    fmt, ell = block_generators.masked(ctx, golden_dir)
    return csr_of_ell(*ell), fmt


def _box(kind, **opts):
    def f(ctx, golden_dir):
        mdl = BOXES[kind]()
        ctx.set_option("block_box", 1)
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_matrix_box(mdl, store=False)
        return csr_of_model(mdl), 4
    return f


def _ell_golden(order):
    def f(ctx, golden_dir):
        g = block_generators.golden_toggle(golden_dir)
        ctx.set_option("format", 1)
        ctx.set_option("sell_code", 0)
        ctx.set_option("state_order", 1 if order else 0)
        if order:
            ctx.set_option("state_order_min", 0)
            ctx.set_option("state_order_products", 0)
            ctx.set_state_coords(g["state"])
        ctx.set_matrix_ell(g["adj"], g["offdiag"], g["diag"])
        assert ctx.state_order_active() == order
        return csr_of_ell(g["adj"], g["offdiag"], g["diag"]), 0
    return f


def _ell_coded(ctx, golden_dir):
    fmt, ell = block_generators.sell_coded(ctx, golden_dir)           # toggle 60 x 50 as coded SELL (format 5)
    return csr_of_ell(*ell), fmt


FORMS = {
    "banded_40x33": _banded("toggle_40x33"),
    "banded_70x61_grid8": _banded("toggle_70x61", grid_blocks=8),
    "banded_70x61_trip_order": _banded_trip_order,
    "masked_banded": _masked,
    "box_toggle_2x2": _box("toggle_2x2"),
    "box_repressilator_3x2": _box("repressilator_3x2"),
    "box_birth_death_6x2": _box("birth_death_6x2"),
    "box_four_slot_6x4": _box("four_slot_6x4"),
    "box_one_species": _box("one_species"),
    "ell_golden": _ell_golden(False),
    "ell_golden_state_order": _ell_golden(True),
    "ell_coded": _ell_coded,
}
ROWS = {"banded_40x33": 1320, "banded_70x61_grid8": 4270, "banded_70x61_trip_order": 4270}


def _setup(ctx, golden_dir, form):
    A, fmt = FORMS[form](ctx, golden_dir)
    if fmt is not None:
        assert ctx.layout_info()["format"] == fmt, (form, ctx.layout_info())
    assert ctx.n == A.shape[0] == ROWS.get(form, ctx.n)
    return A


# ---- 1. the product against numpy
@pytest.mark.parametrize("form", list(FORMS))
def test_product_against_numpy(golden_dir, form):
    with _ctx() as ctx:
        A = _setup(ctx, golden_dir, form)
        rng = np.random.default_rng(5)
        for k in KS:
            X = columns(ctx.n, k, rng)
            Y = ctx.spmm(X, adjoint=True)
            assert ctx.block_info()["adjoint"] == 1
            err, tol = np.abs(Y - A.T @ X), bound(A, X)
            print(form, k, "max err / bound", float((err / np.maximum(tol, 1e-300)).max()))
            assert np.all(err <= tol), (form, k, float(err.max()))


def test_ell_product_is_the_restated_row(golden_dir):
    """the ELL kernel against the numpy restatement of its row (tests/test_block_adjoint_host.py) at the same bound"""
    with _ctx() as ctx:
        A = _setup(ctx, golden_dir, "ell_golden")
        g = block_generators.golden_toggle(golden_dir)
        X = columns(ctx.n, 5, np.random.default_rng(6))
        assert np.all(np.abs(ctx.spmm(X, adjoint=True) - ell_t(g["adj"], g["offdiag"], g["diag"], X)) <= bound(A, X))


# ---- 2. width independence, on the bits
@pytest.mark.parametrize("form", list(FORMS))
def test_column_does_not_depend_on_the_width(golden_dir, form):
    with _ctx() as ctx:
        _setup(ctx, golden_dir, form)
        X = columns(ctx.n, 16, np.random.default_rng(7))
        Y = ctx.spmm(X, adjoint=True)
        for c in range(16):
            assert np.array_equal(_bits(Y[:, c]), _bits(ctx.spmm(X[:, c:c + 1], adjoint=True)[:, 0])), (form, c)


# ---- 3. the forward product is untouched
@pytest.mark.parametrize("form", ["banded_40x33", "masked_banded", "box_four_slot_6x4", "ell_golden_state_order", "ell_coded"])
def test_forward_untouched_after_an_adjoint_call(golden_dir, form):
    with _ctx() as ctx:
        _setup(ctx, golden_dir, form)
        X = columns(ctx.n, 5, np.random.default_rng(8))
        ctx.spmm(X, adjoint=True)
        Y = ctx.spmm(X)
        assert ctx.block_info()["adjoint"] == 0
        for c in range(5):
            assert np.array_equal(_bits(Y[:, c]), _bits(ctx.spmv(X[:, c]))), (form, c)


# ---- 4. transpose identity
@pytest.mark.parametrize("stored", [True, False])
def test_transpose_identity(stored):
    mdl = BOXES["toggle_40x33"]()
    A = csr_of_model(mdl)
    with _ctx(block_box=1) as ctx:
        ctx.set_matrix_box(mdl, store=stored)
        assert ctx.layout_info()["format"] in ((1, 2, 9) if stored else (4,))
        rng = np.random.default_rng(9)
        X, Z = rng.standard_normal((mdl.n, 8)), rng.standard_normal((mdl.n, 8))
        lhs = (Z * ctx.spmm(X)).sum(axis=0)
        rhs = (X * ctx.spmm(Z, adjoint=True)).sum(axis=0)
        tol = 1e-12 * (np.abs(Z) * (abs(A) @ np.abs(X))).sum(axis=0)
        print("transpose identity", stored, np.abs(lhs - rhs) / tol)
        assert np.all(np.abs(lhs - rhs) <= tol)


# ---- 5. whole solves
T, TOL, M = 0.3, 1e-8, 30


def _observables(mdl):
    x1, x2 = (c.astype(np.float64) for c in mdl.coords(np.arange(mdl.n, dtype=np.int64)))
    ind = np.zeros(mdl.n)
    ind[mdl.n // 2 + 3] = 1.0
    return np.column_stack([np.ones(mdl.n), x1, x2, x1 * x2, ind, -x1])


def _toggle_form(ctx, mdl, form):
    if form == "stored":
        ctx.set_matrix_box(mdl, store=True)
    elif form == "matrix_free":
        ctx.set_option("block_box", 1)
        ctx.set_matrix_box(mdl, store=False)
    else:
        ctx.set_option("format", 1)
        ctx.set_option("sell_code", 0)
        ctx.set_matrix_ell(*mdl.ell())
        assert ctx.layout_info()["format"] == 0


@pytest.fixture(scope="module")
def toggle_reference():
    """dense exp(tA) of toggle 23 x 19, computed once and left alone"""
    mdl = BOXES["toggle_23x19"]()
    assert mdl.n == 437
    E = sl.expm(T * csr_of_model(mdl).toarray())
    E.setflags(write=False)
    return mdl, E


@pytest.mark.parametrize("form", ["stored", "matrix_free", "ell"])
def test_backward_solve_matches_dense_expm_and_the_forward_solve(toggle_reference, form):
    """The forward comparisons (tests/test_gpu_block.py, tests/test_gpu_block_small.py) ask l1(R_j - ref_j) <= 10 tol of a
    start column of l1 mass <= 1.  Backward, the roles of l1 and max norm swap - u(x) = <exp(tA) e_x, f> - so column c is
    held to max|R_c - ref_c| <= 10 tol max|F_c|, and the duality to the sum of the two bounds times max|F_c| l1(W_j)."""
    mdl, E = toggle_reference
    F = _observables(mdl)
    with _ctx() as ctx:
        _toggle_form(ctx, mdl, form)
        ctx.set_block(F)
        wsum, st = ctx.expv_block(T, TOL, M, adjoint=True, clamp=False)
        assert ctx.block_info()["adjoint"] == 1
        R = ctx.get_block()
        ref = E.T @ F
        assert st.nstep >= 1 and st.t_now == pytest.approx(T)
        fmax = np.abs(F).max(axis=0)
        for c in range(F.shape[1]):
            err = np.abs(R[:, c] - ref[:, c]).max()
            print(form, "column", c, "max err", err, "bound", 10 * TOL * fmax[c])
            assert err <= 10 * TOL * fmax[c], (form, c)
            assert wsum[c] == pytest.approx(np.abs(R[:, c]).sum(), rel=1e-13)
        assert np.all(R[:, 5] <= 0.0) and (R[:, 5] < 0.0).any()
        assert np.all(R[:, 0] <= 1.0 + 10 * TOL)                      # 1 - u is the exit probability
        # duality with a forward solve of two unit vectors on the same context
        W = np.zeros((mdl.n, 2))
        W[5, 0] = 1.0
        W[mdl.n // 2, 1] = 1.0
        ctx.set_block(W)
        ctx.expv_block(T, TOL, M)
        assert ctx.block_info()["adjoint"] == 0
        P = ctx.get_block()
        for c in range(F.shape[1]):
            for j in range(2):
                d = abs(F[:, c] @ P[:, j] - R[:, c] @ W[:, j])
                assert d <= (10 * TOL + 10 * TOL) * fmax[c] * np.abs(W[:, j]).sum(), (form, c, j, d)


# ---- 6. exact eigenvector
@pytest.mark.parametrize("form", ["stored", "matrix_free"])
def test_eigenvector_breaks_down_alone_and_is_exact(form):
    g, t = 0.5, 1.0
    mdl = death_chain(201, g)
    f = np.arange(mdl.n, dtype=np.float64)
    ind = np.zeros(mdl.n)
    ind[50] = 1.0
    F = np.column_stack([f, ind])
    with _ctx(block_box=1) as ctx:
        ctx.set_matrix_box(mdl, store=(form == "stored"))
        ctx.set_block(F)
        ctx.set_option("adjoint", 1)
        ctx.block_begin(M)
        _, _, brk, _ = ctx.block_arnoldi(M, 1e-7)
        ctx.set_option("adjoint", 0)
        assert list(brk) == [1, 0], brk                                # A^T f = -g f: the column ends after its first vector
        ctx.set_block(F)
        wsum, st = ctx.expv_block(t, TOL, M, adjoint=True, clamp=False)
        R = ctx.get_block()
        assert st.n_breakdown_cols == 1
        want = np.exp(-g * t) * f
        rel = np.abs(R[1:, 0] - want[1:]) / want[1:]
        print(form, "eigenvector: largest relative error", rel.max(), "steps", st.nstep)
        assert R[0, 0] == 0.0 and rel.max() <= 1e-14


# ---- 7. block_clamp
def test_block_clamp():
    """the same pass and the same combine (W = 1 u_1 + 0 u_2 + ... through the whole fma chain) with the clamp off and on"""
    mdl = BOXES["toggle_23x19"]()
    F = _observables(mdl)[:, [1, 5, 4]]                                # x1, -x1, an indicator
    m = 10
    coef = np.zeros((m + 1, 3))
    coef[0] = 1.0
    out = {}
    with _ctx() as ctx:
        ctx.set_matrix_box(mdl, store=True)
        ctx.set_option("adjoint", 1)
        for clamp in (0, 1):
            ctx.set_option("block_clamp", clamp)
            ctx.set_block(F)
            ctx.block_begin(m)
            ctx.block_arnoldi(m, 1e-7)
            ws = ctx.block_combine(m + 1, coef)
            out[clamp] = (ctx.get_block(), ws)
    (R0, ws0), (R1, ws1) = out[0], out[1]
    assert np.array_equal(R0[:, 1], F[:, 1]) and (R0[:, 1] < 0.0).any()        # comes back negative ...
    assert ws0[1] == pytest.approx(np.abs(F[:, 1]).sum(), rel=1e-14)           # ... and wsum is its l1 norm
    assert np.array_equal(_bits(R1[:, 1]), _bits(np.zeros(mdl.n))) and ws1[1] == 0.0   # today's behaviour: clamped at +0.0
    for c in (0, 2):                                                   # the other columns: the same bits either way
        assert np.array_equal(_bits(R0[:, c]), _bits(R1[:, c])) and _bits(ws0[c]) == _bits(ws1[c]), c
        assert np.array_equal(R0[:, c], F[:, c])


# ---- 8. refusals and bookkeeping
def test_refusals():
    from krylovfspssa_amd.host import KfspError, run_loopback_ranks
    mdl = BOXES["toggle_2x2"]()
    W = np.ones((mdl.n, 2))
    with _ctx(format=1) as ctx:                                        # a CSR upload as SELL: no reference arrays
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        assert ctx.layout_info()["format"] in (0, 5)
        ctx.spmm(W)                                                    # forward: taken
        with pytest.raises(KfspError, match=r"-> -12: .*option adjoint.*reference arrays"):
            ctx.spmm(W, adjoint=True)
        ctx.set_block(W)
        with pytest.raises(KfspError, match=r"-> -12: .*option adjoint"):
            ctx.expv_block(0.1, 1e-8, adjoint=True)
        ctx.expv_block(0.01, 1e-8)                                     # and the options are back
    with _ctx() as ctx:                                                # a box without block_box
        ctx.set_matrix_box(mdl, store=False)
        with pytest.raises(KfspError, match=r"-> -12: .*matrix-free generator"):
            ctx.spmm(W, adjoint=True)

    def body(ctx, rank):                                               # a loop-back rank
        ctx.set_option("adjoint", 1)
        r0, nr = ctx.row_block(mdl.n)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows(r0, nr))
        Y = np.empty_like(W)
        rc = ctx._lib.kfsp_spmm(ctx._h, 1, mdl.n, W.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p))
        return rc, ctx._lib.kfsp_last_error(ctx._h).decode()
    for rc, msg in run_loopback_ranks(2, body):
        assert rc == -12 and "row partition" in msg, (rc, msg)


def test_small_path_is_not_taken_backward(golden_dir):
    with _ctx(block_small=1) as ctx:
        block_generators.sell(ctx, golden_dir)
        n = ctx.n
        W = np.ones((n, 3)) / n
        ctx.set_block(W)
        ctx.expv_block(0.01, 1e-8, 30, adjoint=True)
        info = ctx.block_info()
        assert (info["one_launch"], info["adjoint"], info["begin_launches"], info["arnoldi_launches"], info["combine_launches"]) == \
            (0, 1, 2, 4 * 30 + 3, 2), info
        ctx.set_block(W)
        ctx.expv_block(0.01, 1e-8, 30)
        info = ctx.block_info()
        assert (info["one_launch"], info["adjoint"], info["begin_launches"], info["arnoldi_launches"], info["combine_launches"]) == \
            (1, 0, 1, 1, 1), info
