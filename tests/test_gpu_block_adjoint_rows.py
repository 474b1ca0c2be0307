"""Backward block path (option adjoint, kfsp_block_adj.hip) held to what its header promises.

1. Y = A^T X equals the exact rows of tests/row_ref.py (banded_t_exact / ell_t_exact / box_t_exact) on the bits, a zero
   of the restatement by value, on every form the generator can be resident in and at the edges where a transposed
   gather goes wrong (tests/adjoint_cases.py lists them; tests/test_row_ref.py shows on the CPU that every case tells a
   row taken in another order, or with the diagonal term last, from the right one).  k = 3, so kp = 4 with one padding
   column; tests/test_gpu_block_adjoint.py ties every other width to the same bits.  The looser comparison with
   A.T @ X stays beside the bitwise one.
2. The backward Krylov pass (the DOTS instantiations: finish_row's partials, rows_red) against the oracle's Arnoldi on
   A^T at the tolerances of tests/test_gpu_parity.py::test_arnoldi_matches_oracle.  The rows in [n, rows_act) and the
   padding columns of the block cannot be read back through the library; they enter every norm of this pass (the
   streaming kernels sum the whole padded block), so a pad row that is not 0 moves H and the norms.
3. Whole backward solves against tests/block_ref.py on A^T, decision for decision, as the forward solve is held in
   tests/test_gpu_block_reference.py.
Needs a real MI355X."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import adjoint_cases as AC
from tests import block_generators
from tests import block_ref as BR
from tests.test_block_adjoint_host import bound

pytestmark = pytest.mark.gpu

_bits = AC.bits


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- the forms: name -> (case of tests/adjoint_cases.py, setter(ctx, golden_dir))
def _banded(case, **opts):
    def f(ctx, golden_dir):
        mdl = AC.model(case)
        ctx.set_option("format", 0)
        ctx.set_option("dia_mask", 0)
        ctx.set_option("dia_code", 0)
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        # dia_code = 1: the coded image (kernel format 9) is what the single-vector product reads; kfsp_layout_info keeps
        # calling it banded.  The transposed product has no coded kernel: it reads the plain value streams, which stay.
        assert ctx.layout_info()["format"] == 1 and ctx.dia_code_info()["active"] == (1 if opts.get("dia_code") else 0)
    return f


def _banded_trip_order(ctx, golden_dir):
    _banded("banded_70x61")(ctx, golden_dir)
    ctx.set_trip_order(np.random.default_rng(3).permutation((ctx.n + 127) // 128))


def _masked(ctx, golden_dir):
    fmt, _ = block_generators.masked(ctx, golden_dir)
    assert ctx.layout_info()["format"] == fmt == 2


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
        assert ctx.state_order_active() == order and ctx.layout_info()["format"] == 0
    return f


def _ell_coded(ctx, golden_dir):
    fmt, _ = block_generators.sell_coded(ctx, golden_dir)
    assert ctx.layout_info()["format"] == fmt == 5


def _ell_wide(ctx, golden_dir):
    """the upload through the C ABI: the wrapper knows no leading dimension"""
    adj, off, diag, bw = AC.golden_wide()
    n, ld = adj.shape
    assert ld == bw + AC.WIDE_PAD
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 0)
    adj, off, diag = (np.ascontiguousarray(a) for a in (adj, off, diag))
    ctx._chk(ctx._lib.kfsp_set_matrix_ell(ctx._h, n, bw, ld, _p(adj), _p(off), _p(diag)), "kfsp_set_matrix_ell")
    ctx.n = n
    ctx.row0, ctx.nloc = ctx.row_block(n)
    assert ctx.layout_info()["format"] == 0


def _box(case):
    def f(ctx, golden_dir):
        ctx.set_option("block_box", 1)
        ctx.set_matrix_box(AC.model(case), store=False)
        assert ctx.layout_info()["format"] == 4
    return f


FORMS = {
    "banded_40x33": ("banded_40x33", _banded("banded_40x33")),
    "banded_70x61_grid8": ("banded_70x61", _banded("banded_70x61", grid_blocks=8)),
    "banded_70x61_trip_order": ("banded_70x61", _banded_trip_order),
    "masked_banded": ("masked_banded", _masked),
    "banded_40x33_dia_code": ("banded_40x33", _banded("banded_40x33", dia_code=1)),
    "ell_golden": ("ell_golden", _ell_golden(False)),
    "ell_golden_state_order": ("ell_golden", _ell_golden(True)),
    "ell_coded": ("ell_coded", _ell_coded),
    "ell_wide": ("ell_wide", _ell_wide),
    "box_toggle_2x2": ("box_toggle_2x2", _box("box_toggle_2x2")),
    "box_repressilator_3x2": ("box_repressilator_3x2", _box("box_repressilator_3x2")),
    "box_birth_death_6x2": ("box_birth_death_6x2", _box("box_birth_death_6x2")),
    "box_four_slot_6x4": ("box_four_slot_6x4", _box("box_four_slot_6x4")),
    "box_one_species": ("box_one_species", _box("box_one_species")),
}


def _assert_rows(form, Y, c):
    """the loose bound of tests/test_gpu_block_adjoint.py, then the bits"""
    err, tol = np.abs(Y - c["A"].T @ c["X"]), bound(c["A"], c["X"])
    print(form, "max err / bound", float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol), (form, float(err.max()))
    bad = AC.mismatches(Y, c["Y"])
    print(form, "rows off the restatement:", int(bad.any(axis=1).sum()), "of", c["n"], "per column", bad.sum(axis=0).tolist())
    assert not bad.any(), (form, np.argwhere(bad)[:8].tolist(), Y[bad][:4], c["Y"][bad][:4])


def _assert_forward_untouched(form, ctx, X):
    """after an adjoint product the forward spmm of one column still is spmv, on the bits"""
    y = ctx.spmm(X[:, :1])
    assert ctx.block_info()["adjoint"] == 0
    assert np.array_equal(_bits(y[:, 0]), _bits(ctx.spmv(X[:, 0]))), form


# ---- 1. the product on the bits
@pytest.mark.parametrize("form", list(FORMS))
def test_product_is_the_restated_row_on_the_bits(golden_dir, form):
    name, setter = FORMS[form]
    c = AC.case(name)
    with _ctx() as ctx:
        setter(ctx, golden_dir)
        assert ctx.n == c["n"]
        Y = ctx.spmm(c["X"], adjoint=True)
        assert ctx.block_info()["adjoint"] == 1
        _assert_rows(form, Y, c)
        _assert_forward_untouched(form, ctx, c["X"])


@pytest.mark.parametrize("form", ["banded_40x33", "box_four_slot_6x4"])
def test_leading_dimension_above_n(golden_dir, form):
    """X and Y with a leading dimension of n + 5 through the C ABI: NaN in the gap of X (a read would spread it), a
    sentinel in the gap of Y (a write would overwrite it)"""
    name, setter = FORMS[form]
    c = AC.case(name)
    n, k = c["n"], AC.K
    ld = n + 5
    sentinel = -12345.6789
    with _ctx() as ctx:
        setter(ctx, golden_dir)
        Xp = np.full((k, ld), np.nan)
        Xp[:, :n] = c["X"].T
        Yp = np.full((k, ld), sentinel)
        ctx.set_option("adjoint", 1)
        try:
            ctx._chk(ctx._lib.kfsp_spmm(ctx._h, k, ld, _p(Xp), _p(Yp)), "kfsp_spmm")
            assert ctx.block_info()["adjoint"] == 1
        finally:
            ctx.set_option("adjoint", 0)
        _assert_rows(form, Yp[:, :n].T, c)
        assert np.array_equal(_bits(Yp[:, n:]), _bits(np.full((k, 5), sentinel)))
        assert np.isnan(Xp[:, n:]).all() and np.array_equal(_bits(Xp[:, :n]), _bits(c["X"].T))
        _assert_forward_untouched(form, ctx, c["X"])


# ---- 2. the backward Krylov pass against the oracle on A^T
def _observables5(x1, x2, n):
    ind = np.zeros(n)
    ind[n // 2 + 3] = 1.0
    return np.column_stack([np.ones(n), x1, x1 * x2, ind, -x1])


def _model_coords(mdl):
    return tuple(c.astype(np.float64) for c in mdl.coords(np.arange(mdl.n, dtype=np.int64)))


def _krylov_banded(ctx, golden_dir):
    mdl = AC.model("banded_40x33")
    FORMS["banded_40x33"][1](ctx, golden_dir)
    return mdl.ell(), _model_coords(mdl)


def _krylov_ell(ctx, golden_dir):
    FORMS["ell_golden"][1](ctx, golden_dir)
    g = block_generators.golden_toggle(golden_dir)
    return (g["adj"], g["offdiag"], g["diag"]), (g["state"][:, 0].astype(np.float64), g["state"][:, 1].astype(np.float64))


def _krylov_box(ctx, golden_dir):
    mdl = AC.model("box_four_slot_6x4")
    FORMS["box_four_slot_6x4"][1](ctx, golden_dir)
    return mdl.ell(), _model_coords(mdl)


KRYLOV = {"banded": _krylov_banded, "ell": _krylov_ell, "box": _krylov_box}


@pytest.mark.parametrize("form", list(KRYLOV))
def test_backward_arnoldi_matches_the_oracle_on_the_transpose(golden_dir, form):
    """k = 5 observables (kp = 8: three padding columns), m = 20, break_tol 1e-7: every entry of every column's H, the
    norms, AVNORM, beta and the breakdown column against oracle.arnoldi(A^T, F_c / beta_c, 20)"""
    m = 20
    with _ctx() as ctx:
        ell, (x1, x2) = KRYLOV[form](ctx, golden_dir)
        n = ctx.n
        F = _observables5(x1, x2, n)
        ctx.set_block(F)
        ctx.set_option("adjoint", 1)
        try:
            beta = ctx.block_begin(m)
            hb, nrm, brk, avn = ctx.block_arnoldi(m, 1e-7)
            assert ctx.block_info()["adjoint"] == 1
        finally:
            ctx.set_option("adjoint", 0)
    AT = O.EllMatrix(*BR.transpose_ell(*ell))
    for c in range(F.shape[1]):
        bref = float(np.sqrt((F[:, c] * F[:, c]).sum()))
        _, Href, mb, k1, av = O.arnoldi(AT, F[:, c] / bref, m)
        assert beta[c] == pytest.approx(bref, rel=1e-14), (form, c)
        assert brk[c] == (mb if k1 == 0 else 0), (form, c, brk[c], mb, k1)
        H = np.zeros_like(Href)
        for j in range(1, mb + 1):
            H[j - 1, j - 1] = hb[j, 1, c]
            if j >= 2:
                H[j - 2, j - 1] = hb[j, 0, c]
            if j < mb or k1 != 0:
                H[j, j - 1] = hb[j, 2, c]
        band = np.triu(np.tril(np.ones_like(Href), 1), -1)[:mb + 1, :mb] > 0
        Hr = np.where(band, Href[:mb + 1, :mb], 0.0)
        if k1 == 0:
            Hr[mb, mb - 1] = 0.0                                       # a breakdown: H(mb + 1, mb) is below break_tol, not compared
        assert not np.any(np.where(band, 0.0, Href[:mb + 1, :mb])), (form, c)       # IOP(2): nothing outside the band
        hs = np.abs(Href).max()
        worst = np.abs(H[:mb + 1, :mb] - Hr).max() / hs
        print(form, "column", c, "max|H - Href| / max|Href|", worst, "avnorm rel", abs(avn[c] - av) / av if k1 else 0.0)
        assert worst <= 1e-11, (form, c)
        js = np.arange(1, mb + 1 if k1 else mb)
        assert np.array_equal(_bits(nrm[js + 1, c]), _bits(hb[js, 2, c])), (form, c)
        if k1 != 0:
            assert avn[c] == pytest.approx(av, rel=1e-10), (form, c)


# ---- 3. whole backward solves against the restatement on A^T
T, TOL, M = 0.3, 1e-8, 30


def _observables6(mdl):
    x1, x2 = _model_coords(mdl)
    ind = np.zeros(mdl.n)
    ind[mdl.n // 2 + 3] = 1.0
    return np.column_stack([np.ones(mdl.n), x1, x2, x1 * x2, ind, -x1])


def _assert_solve_matches_ref(tag, R, ws, st, Rref, wsref, stref, F):
    """the forward assertions of tests/test_gpu_block_reference.py: the same decisions (all counts exact, the step sizes
    to 1e-12 relative), every column within 1e-10 max(1, l1(F_c)) in l1 - the forward 1e-10 assumes a start column of
    l1 mass <= 1 and observables are not normalised.  wsum is the l1 norm of a column, so it differs by no more than the
    columns do (triangle inequality) plus the rounding of two sums of n terms."""
    assert (st.nstep, st.nreject, st.nmult, st.n_breakdown_cols) == \
        (stref.nstep, stref.nreject, stref.nmult, stref.n_breakdown_cols), (tag, st.nstep, st.nreject, st.nmult, stref)
    for f in ("t_now", "step_min", "step_max"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-12, abs=0), (tag, f)
    for c in range(F.shape[1]):
        scale = max(1.0, np.abs(F[:, c]).sum())
        err = np.abs(R[:, c] - Rref[:, c]).sum()
        print(tag, "column", c, "l1 err / (1e-10 max(1, l1 F))", err / (1e-10 * scale))
        assert err <= 1e-10 * scale, (tag, c)
        assert abs(ws[c] - wsref[c]) <= 1e-10 * scale + 1e-13 * wsref[c], (tag, c)


@pytest.fixture(scope="module")
def toggle_backward_reference():
    """the restatement's backward solve of toggle 23 x 19, computed once and left alone"""
    from krylovfspssa_amd import synth
    mdl = synth.toggle(23, 19)
    F = _observables6(mdl)
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*BR.transpose_ell(*mdl.ell())), F, T, TOL, M, clamp=False)
    for a in (F, Rref, wsref):
        a.setflags(write=False)
    return mdl, F, Rref, wsref, stref


@pytest.mark.parametrize("form", ["stored", "matrix_free", "ell"])
def test_backward_solve_matches_the_restatement(toggle_backward_reference, form):
    mdl, F, Rref, wsref, stref = toggle_backward_reference
    assert stref.nstep >= 2
    with _ctx() as ctx:
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
        ctx.set_block(F)
        ws, st = ctx.expv_block(T, TOL, M, adjoint=True, clamp=False)
        assert ctx.block_info()["adjoint"] == 1
        R = ctx.get_block()
    _assert_solve_matches_ref(form, R, ws, st, Rref, wsref, stref, F)


def test_stiff_backward_solve_rejects_like_the_restatement():
    """the "stiff" birth-death case of tests/test_gpu_block_reference.py, backward: t |A| ~ 20, a rejected step"""
    from krylovfspssa_amd import synth
    mdl = synth.birth_death((30, 20), k=(100.0, 150.0), g=(10.0, 20.0))
    t, tol, m = 0.02, 1e-10, 30
    F = _observables6(mdl)
    with _ctx() as ctx:
        ctx.set_option("dia_mask", 0)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ctx.set_block(F)
        ws, st = ctx.expv_block(t, tol, m, adjoint=True, clamp=False)
        R = ctx.get_block()
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*BR.transpose_ell(*mdl.ell())), F, t, tol, m, clamp=False)
    assert stref.nreject >= 1 and stref.nstep >= 2
    _assert_solve_matches_ref("stiff", R, ws, st, Rref, wsref, stref, F)
