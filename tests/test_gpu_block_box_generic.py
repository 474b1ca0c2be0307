"""Several vectors at once on MULTI-FACTOR matrix-free boxes (option block_box = 2: k_spmm_boxg, kfsp_block_boxg.hip, and
k_spmm_boxg_t, kfsp_block_adj.hip; the row code in kfsp_boxg_dev.h).  The rows of A X and of A^T X on the bits of their
restatements (tests/row_ref.py box_generic_exact, tests/box_generic_t_ref.py) and of kfsp_spmv; the trip loop and a trip
order; the generic kernel told apart from the single-factor one; a leading dimension; the DOTS instantiations against
oracle.arnoldi; whole solves against tests/block_ref.py and tests/block_integral_ref.py decision for decision; and what
stays as it was (the refusals of values 0 and 1, row partitions, the single vector w).  Needs a real MI355X.

Every context below carries a vector w, set before the first block call and compared on the bits when the context closes."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import adjoint_cases as AC
from tests import block_integral_ref as IR
from tests import block_ref as BR
from tests import box_cases as BC
from tests import box_generic_t_ref as GT
from tests import row_ref as RR
from tests.test_block_adjoint_host import csr_of_model

pytestmark = pytest.mark.gpu

_bits = AC.bits
KMAX = max(BC.BLOCK_K)


@contextlib.contextmanager
def _box_ctx(mdl, block_box=2, **opts):
    """a context with mdl resident matrix-free and a vector w that no block call may touch"""
    from krylovfspssa_amd import KfspContext
    with KfspContext(0) as ctx:
        ctx.set_option("block_box", block_box)
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_matrix_box(mdl, store=False)
        w = BC.vector(mdl.n, 1)
        ctx.set_vector(w)
        yield ctx
        assert np.array_equal(_bits(ctx.get_vector()), _bits(w)), "a block call touched w"


@functools.lru_cache(maxsize=None)
def _forward(name, k):
    """-> (X, Y): k columns like box_cases.vector and box_generic_exact of each; computed once, left alone"""
    mdl = GT.model(name)
    X = np.stack([BC.vector(mdl.n, 4000 + 20 * len(name) + j) for j in range(k)], axis=1)
    Y = np.stack([np.array(RR.box_generic_exact(mdl, X[:, j])) for j in range(k)], axis=1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


def _assert_columns_are_spmv(ctx, X, Y, tag):
    for j in range(X.shape[1]):
        assert np.array_equal(_bits(Y[:, j]), _bits(ctx.spmv(X[:, j]))), (tag, j)


# ---- 1. forward rows on the bits (on the parent commit the first spmm below returns -12)
@pytest.mark.parametrize("name", BC.generic_names())
def test_forward_rows_on_the_bits(name):
    mdl = BC.model(name)
    X, Yref = _forward(name, KMAX)
    got = {}
    with _box_ctx(mdl) as ctx:
        assert ctx.layout_info()["format"] == 3, ctx.layout_info()       # the interpreted kernel answers for the single vector
        for k in BC.BLOCK_K:
            Y = got[k] = ctx.spmm(X[:, :k])
            for j in range(k):
                bad = BC.mismatches(Y[:, j], Yref[:, j])
                assert len(bad) == 0, (name, k, j, len(bad), bad[:5])
            _assert_columns_are_spmv(ctx, X[:, :k], Y, (name, k))
    assert np.array_equal(_bits(got[16][:, :5]), _bits(got[5])), name        # a column does not depend on the width
    assert np.array_equal(_bits(got[16][:, :1]), _bits(got[1])), name


# ---- 2. the trip loop
def test_trip_loop_and_trip_order():
    mdl = GT.model("goutsias_loop")
    trips = (mdl.n + 127) // 128
    assert (mdl.n, trips) == (5670, 45) and mdl.n % 128 != 0
    X, Yref = _forward("goutsias_loop", 3)
    X16 = np.stack([BC.vector(mdl.n, 4700 + j) for j in range(16)], axis=1)

    def check(ctx, tag):
        _assert_columns_are_spmv(ctx, X16, ctx.spmm(X16), tag)
        Y = ctx.spmm(X)
        for j in range(3):
            assert len(BC.mismatches(Y[:, j], Yref[:, j])) == 0, (tag, j)
    with _box_ctx(mdl, grid_blocks=8) as ctx:          # 8 workgroups = 32 wavefronts for 45 trips: the trip loop turns
        check(ctx, "grid8")
    with _box_ctx(mdl) as ctx:
        ctx.set_trip_order(np.random.default_rng(3).permutation(trips))
        check(ctx, "order")
        ctx.set_option("grid_blocks", 8)
        check(ctx, "order+grid8")


# ---- 3. the generic kernel on single-factor models
@pytest.mark.parametrize("name", ["decode_49x4x3", "decode_8x49x2", "dup_12x9"])
def test_generic_kernel_on_single_factor_models(name):
    mdl = BC.model(name)
    c = BC.case(name)
    if name.startswith("decode"):
        assert BC.decode_corrections(mdl)[0] > 0                        # rows that take the coordinate decode's correction step
    X = np.stack([np.asarray(c["x"]), BC.vector(mdl.n, 4301), BC.vector(mdl.n, 4302)], axis=1)
    Yg = np.stack([np.asarray(c["yg"])] + [np.array(RR.box_generic_exact(mdl, X[:, j])) for j in (1, 2)], axis=1)
    Yf = np.stack([np.asarray(c["y"])] + [np.array(RR.box_exact(mdl, X[:, j])) for j in (1, 2)], axis=1)
    assert np.any(_bits(Yg) != _bits(Yf))                                # the two definitions differ on the bits here
    with _box_ctx(mdl, box_generic=1) as ctx:
        assert ctx.layout_info()["format"] == 3
        Y = ctx.spmm(X)
        for j in range(3):
            assert len(BC.mismatches(Y[:, j], Yg[:, j])) == 0, (name, "generic", j)
        _assert_columns_are_spmv(ctx, X, Y, (name, "generic"))
        ctx.set_option("box_generic", 0)                                 # read at every block call: k_spmm_box, as under value 1
        Y = ctx.spmm(X)
        for j in range(3):
            assert len(BC.mismatches(Y[:, j], Yf[:, j])) == 0, (name, "single-factor", j)
    with _box_ctx(mdl, block_box=1) as ctx:
        assert np.array_equal(_bits(ctx.spmm(X)), _bits(Y)), name        # the same bits as value 1 gives


# ---- 4. leading dimension
@pytest.mark.parametrize("name", BC.NAMED_GENERIC)
@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_leading_dimension(name, adjoint):
    mdl = BC.model(name)
    n, k, pad = mdl.n, 3, 5
    X = _forward(name, KMAX)[0][:, :k]
    with _box_ctx(mdl) as ctx:
        want = ctx.spmm(X, adjoint=adjoint)
        Xw = np.full((n + pad, k), np.nan, order="F")
        Xw[:n] = X
        Yw = np.full((n + pad, k), -777.0, order="F")
        ctx.set_option("adjoint", 1 if adjoint else 0)
        try:
            rc = ctx._lib.kfsp_spmm(ctx._h, k, n + pad, Xw.ctypes.data_as(ctypes.c_void_p), Yw.ctypes.data_as(ctypes.c_void_p))
        finally:
            ctx.set_option("adjoint", 0)
        assert rc == 0, ctx._lib.kfsp_last_error(ctx._h).decode()
        assert np.array_equal(_bits(Yw[:n]), _bits(want)), (name, adjoint)
        assert np.all(Yw[n:] == -777.0) and not np.isnan(Yw).any()


# ---- 5. backward rows
@pytest.mark.parametrize("name", BC.generic_names() + ("goutsias_loop",))
def test_backward_rows_on_the_bits(name):
    c = GT.case(name)
    mdl, X, Yref = c["mdl"], c["X"], c["Y"]
    opts = dict(grid_blocks=8) if name == "goutsias_loop" else {}
    with _box_ctx(mdl, **opts) as ctx:
        Y = ctx.spmm(X, adjoint=True)
        assert ctx.block_info()["adjoint"] == 1
        bad = AC.mismatches(Y, Yref)
        assert not bad.any(), (name, int(bad.any(axis=1).sum()), np.flatnonzero(bad.any(axis=1))[:5])
        Xf = _forward(name, KMAX)[0][:, :5] if name != "goutsias_loop" else _forward(name, 3)[0]
        Yf = ctx.spmm(Xf)                                                # the forward product after an adjoint call
        assert ctx.block_info()["adjoint"] == 0
        _assert_columns_are_spmv(ctx, Xf, Yf, name)


@pytest.mark.parametrize("name", BC.NAMED_GENERIC)
def test_transpose_identity(name):
    mdl = BC.model(name)
    A = csr_of_model(mdl)
    rng = np.random.default_rng(9)
    X, Z = rng.standard_normal((mdl.n, 8)), rng.standard_normal((mdl.n, 8))
    with _box_ctx(mdl) as ctx:
        lhs = (Z * ctx.spmm(X)).sum(axis=0)
        rhs = (X * ctx.spmm(Z, adjoint=True)).sum(axis=0)
    tol = 1e-12 * (np.abs(Z) * (abs(A) @ np.abs(X))).sum(axis=0)
    print("transpose identity", name, np.abs(lhs - rhs) / tol)
    assert np.all(np.abs(lhs - rhs) <= tol)


# ---- 6. the DOTS instantiations and the padding rows
def _coords(mdl):
    return [c.astype(np.float64) for c in mdl.coords(np.arange(mdl.n, dtype=np.int64))]


def _starts5(mdl):
    """five columns (kp = 8: three padding columns).  Forward: two unit vectors and three probability vectors"""
    n = mdl.n
    rng = np.random.default_rng(11)
    W = np.zeros((n, 5))
    W[7, 0] = 1.0
    W[n // 2 + 5, 1] = 1.0
    for c in (2, 3, 4):
        p = rng.random(n) ** c
        W[:, c] = p / p.sum()
    return W


def _observables5(mdl):
    x = _coords(mdl)
    ind = np.zeros(mdl.n)
    ind[mdl.n // 2 + 3] = 1.0
    return np.column_stack([np.ones(mdl.n), x[0], x[1], x[0] * x[1], ind])


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
def test_arnoldi_matches_the_oracle(adjoint):
    """block_begin / block_arnoldi(m = 20, 1e-7) on goutsias (720 rows: five groups and a ragged sixth) against
    oracle.arnoldi on the model's rows, at the tolerances of the existing block parity tests"""
    m = 20
    mdl = BC.model("goutsias")
    assert mdl.n == 720 and mdl.n % 128 != 0
    F = _observables5(mdl) if adjoint else _starts5(mdl)
    with _box_ctx(mdl) as ctx:
        ctx.set_block(F)
        ctx.set_option("adjoint", 1 if adjoint else 0)
        try:
            beta = ctx.block_begin(m)
            hb, nrm, brk, avn = ctx.block_arnoldi(m, 1e-7)
            assert ctx.block_info()["adjoint"] == (1 if adjoint else 0) and ctx.block_info()["one_launch"] == 0
        finally:
            ctx.set_option("adjoint", 0)
    ell = mdl.ell()
    A = O.EllMatrix(*(BR.transpose_ell(*ell) if adjoint else ell))
    for c in range(F.shape[1]):
        bref = float(np.sqrt((F[:, c] * F[:, c]).sum()))
        _, Href, mb, k1, av = O.arnoldi(A, F[:, c] / bref, m)
        assert beta[c] == pytest.approx(bref, rel=1e-14), c
        assert brk[c] == (mb if k1 == 0 else 0), (c, brk[c], mb, k1)
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
        worst = np.abs(H[:mb + 1, :mb] - Hr).max() / np.abs(Href).max()
        print("adjoint" if adjoint else "forward", "column", c, "max|H - Href| / max|Href|", worst,
              "avnorm rel", abs(avn[c] - av) / av if k1 else 0.0)
        assert worst <= 1e-11, c
        if k1 != 0:
            assert avn[c] == pytest.approx(av, rel=1e-10), c


# ---- 7. whole solves
TOL, M = 1e-8, 30
# On the CPU the restatement takes 4 steps and 1 rejection in either direction, and the same decisions (counts and step
# sizes) with every rate perturbed by 1e-13 relative, either sign: no decision sits on an edge that rounding could move.
# (Forward, the box is nearly empty long before t = 500 - 11 steps, 1 rejection - and the error estimates that pick the
# later step sizes are rounding noise: there the device took a step of 90 where the restatement took 100.)
T_FORWARD, T_BACKWARD = 80.0, 32.0


@functools.lru_cache(maxsize=None)
def _solve_reference(adjoint):
    mdl = BC.model("goutsias")
    ell = mdl.ell()
    if adjoint:
        x = _coords(mdl)
        F = np.column_stack([np.ones(mdl.n), x[0], x[0] * x[1]])       # ones, a count, a product of counts
        A, t, clamp = O.EllMatrix(*BR.transpose_ell(*ell)), T_BACKWARD, False
    else:
        F = np.zeros((mdl.n, 4))                                       # four unit start vectors
        for j, r in enumerate((100, 300, 500, 700)):
            F[r, j] = 1.0
        A, t, clamp = O.EllMatrix(*ell), T_FORWARD, True
    Rref, wsref, stref = BR.expv_block(A, F, t, TOL, M, clamp=clamp)
    Ri, _, sti, Jref = IR.expv_block_integral(A, F, t, TOL, M, clamp=clamp)
    assert (sti.nstep, sti.nreject) == (stref.nstep, stref.nreject) and np.array_equal(Ri, Rref)
    for a in (F, Rref, wsref, Jref):
        a.setflags(write=False)
    return mdl, F, t, clamp, Rref, wsref, stref, Jref


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "backward"])
def test_whole_solve_matches_the_restatement(adjoint):
    mdl, F, t, clamp, Rref, wsref, stref, Jref = _solve_reference(adjoint)
    assert stref.nstep >= 3 and stref.nreject >= 1, (stref.nstep, stref.nreject)
    with _box_ctx(mdl, block_integral=1) as ctx:
        ctx.set_block(F)
        ws, st = ctx.expv_block(t, TOL, M, adjoint=adjoint, clamp=clamp)
        assert ctx.block_info()["adjoint"] == (1 if adjoint else 0)
        R, J = ctx.get_block(), ctx.get_block(integral=True)
    tag = "backward" if adjoint else "forward"
    assert (st.nstep, st.nreject, st.nmult, st.n_breakdown_cols) == \
        (stref.nstep, stref.nreject, stref.nmult, stref.n_breakdown_cols), (tag, st.nstep, st.nreject, st.nmult, stref)
    for f in ("t_now", "step_min", "step_max"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-12, abs=0), (tag, f)
    l1 = np.abs(F).sum(axis=0)
    for c in range(F.shape[1]):
        scale = max(1.0, l1[c])
        err, errj = np.abs(R[:, c] - Rref[:, c]).sum(), np.abs(J[:, c] - Jref[:, c]).sum()
        print(tag, "column", c, "l1 err / (1e-10 max(1, l1 F))", err / (1e-10 * scale), "J:", errj / (1e-10 * t * scale))
        assert err <= 1e-10 * scale, (tag, c)
        assert abs(ws[c] - wsref[c]) <= 1e-10 * scale + 1e-13 * wsref[c], (tag, c)
        assert errj <= 1e-10 * t * scale, (tag, c)


# ---- 8. what stays
def test_row_partitions_are_still_refused():
    from krylovfspssa_amd.host import run_loopback_ranks
    mdl = BC.model("goutsias")
    W = np.ones((mdl.n, 2))

    def body(ctx, rank):
        out = []
        ctx.set_option("block_box", 2)
        for part in (0, 1):
            ctx.set_option("block_partition", part)
            ctx.set_matrix_box(mdl, store=False)
            Y = np.empty_like(W)
            rc = ctx._lib.kfsp_spmm(ctx._h, 2, mdl.n, W.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p))
            out.append((rc, ctx._lib.kfsp_last_error(ctx._h).decode()))
        return out
    for rank in run_loopback_ranks(2, body):
        (rc0, msg0), (rc1, msg1) = rank
        assert rc0 == -12 and "row partition" in msg0, (rc0, msg0)
        assert rc1 == -12 and "matrix-free" in msg1, (rc1, msg1)


def test_values_0_and_1_refuse_as_before():
    from krylovfspssa_amd.host import KfspError
    mdl = BC.model("goutsias")
    W = np.ones((mdl.n, 2))
    for value, what in ((0, "matrix-free generator"), (1, "no single-factor form")):
        with _box_ctx(mdl, block_box=value) as ctx:
            with pytest.raises(KfspError, match=r"-> -12: .*" + what):
                ctx.spmm(W)
            with pytest.raises(KfspError, match=r"-> -12: .*" + what):
                ctx.spmm(W, adjoint=True)
            with pytest.raises(KfspError, match="-> -12"):
                ctx.set_block(W)
    with _box_ctx(BC.model("dup_12x9"), block_box=1, box_generic=1) as ctx:      # the interpreted product under value 1
        with pytest.raises(KfspError, match=r"-> -12: .*box_generic"):
            ctx.spmm(np.ones((ctx.n, 2)))
    with _box_ctx(mdl) as ctx:                                                   # read at every block call
        ctx.spmm(W)
        ctx.set_option("block_box", 1)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.spmm(W)
        ctx.set_option("block_box", 2)
        ctx.spmm(W)


def test_generator_change_discards_the_block():
    from krylovfspssa_amd.host import KfspError
    mdl = BC.model("goutsias")
    W = np.ones((mdl.n, 2))
    with _box_ctx(mdl) as ctx:
        ctx.set_block(W)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W))
        w = ctx.get_vector()
        ctx.set_matrix_box(BC.model("three_factor"), store=False)
        with pytest.raises(KfspError, match="no block resident"):
            ctx.get_block()
        with pytest.raises(KfspError):
            ctx.expv_block(0.1, 1e-8)
        ctx.set_matrix_box(mdl, store=False)
        ctx.set_vector(w)
        ctx.set_block(W)
        ctx.expv_block(0.1, 1e-8)
