"""Several start vectors at once on a MATRIX-FREE box (option block_box, k_spmm_box): the block product is kfsp_spmv column by
column, bit for bit, in every instantiation of the single-factor form; the block solve matches dense exp(tA); its columns
are independent; the single-vector path does not notice; what has no single-factor form stays refused.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

from tests.test_gpu_block import KS, _bits, _dense, _start_block

pytestmark = pytest.mark.gpu


def _ctx():
    from krylovfspssa_amd import KfspContext
    return KfspContext(0)


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _four_slot_box():
    """species 0 drives four reactions (steps +1, -1, +2, -2), species 1 two: the 6-species / 4-slot instantiation"""
    st = [[1, -1, 2, -2, 0, 0], [0, 0, 0, 0, 1, -1]]

    def prop(r, X):
        x, y = X
        return (np.full_like(x, 5.0), 0.7 * x, 1.5 + 0.01 * x, 0.02 * x * (x - 1.0), 3.0 + 0.1 * y, 0.9 * y)[r]
    return _synth().BoxModel("four_slot", (37, 29), st, prop, deps=[(0,), (0,), (0,), (0,), (1,), (1,)])


def _absorbing_box(N=300, b=40.0, g=1.0):
    """the birth-death chain of tests/test_gpu_block.py::_absorbing_chain as a one-species box: nothing leaves state 0"""
    def prop(r, X):
        x = X[0]
        return np.where((x > 0) & (x < N - 1), b, 0.0) if r == 0 else g * x
    return _synth().BoxModel("absorbing", (N,), [[1, -1]], prop, deps=[(0,), (0,)])


BOXES = {
    "toggle_2x2": lambda: _synth().toggle(60, 50),
    "repressilator_3x2": lambda: _synth().repressilator(dims=(13, 11, 7)),
    "birth_death_6x2": lambda: _synth().birth_death((5, 6, 4, 5, 3, 4)),
    "four_slot_6x4": _four_slot_box,
    "one_species": lambda: _synth().birth_death((1000,)),
}
SIZES = {"toggle_2x2": 3000, "repressilator_3x2": 1001, "birth_death_6x2": 7200, "four_slot_6x4": 1073, "one_species": 1000}


def _set_box(ctx, mdl, **options):
    ctx.set_option("block_box", 1)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_matrix_box(mdl, store=False)


def _columns(n, k, rng):
    """negative entries, a unit vector (exact zeros everywhere else), all-positive; the rest random"""
    X = rng.standard_normal((n, k))
    X[:, 0] = -np.abs(X[:, 0])
    if k > 1:
        X[:, 1] = 0.0
        X[n // 3, 1] = 1.0
    if k > 2:
        X[:, 2] = np.abs(X[:, 2]) + 0.25
    return X


def _assert_columns_are_spmv(ctx, tag, ks=KS, seed=5):
    n = ctx.n
    assert n % 128 != 0
    rng = np.random.default_rng(seed)
    for k in ks:
        X = _columns(n, k, rng)
        Y = ctx.spmm(X)
        for j in range(k):
            assert np.array_equal(_bits(Y[:, j]), _bits(ctx.spmv(X[:, j]))), (tag, k, j)


@pytest.mark.parametrize("kind", list(BOXES))
def test_spmm_is_spmv_column_by_column_bit_for_bit(kind):
    mdl = BOXES[kind]()
    assert mdl.n == SIZES[kind]
    if kind == "four_slot_6x4":
        ndep, dep, _ = mdl.factors()
        assert np.all(ndep == 1) and np.bincount(dep[:, 0]).max() == 4          # one factor each, four on species 0
    with _ctx() as ctx:
        _set_box(ctx, mdl)
        assert ctx.layout_info()["format"] == 4, (kind, ctx.layout_info())     # the single-factor matrix-free kernel answers
        _assert_columns_are_spmv(ctx, kind)


def test_spmm_against_the_pencil_kernel():
    """6-species boxes take the pencil kernel by default once they are large; here the option insists"""
    with _ctx() as ctx:
        _set_box(ctx, BOXES["birth_death_6x2"](), box_pencil=1)
        assert ctx.layout_info()["format"] == 7
        _assert_columns_are_spmv(ctx, "pencil", ks=(3, 16))


def test_spmm_trip_loop_and_trip_order():
    mdl = BOXES["birth_death_6x2"]()
    trips = (mdl.n + 127) // 128
    assert trips == 57
    with _ctx() as ctx:                            # 8 workgroups = 32 wavefronts for 57 trips: the trip loop turns
        _set_box(ctx, mdl, grid_blocks=8)
        _assert_columns_are_spmv(ctx, "grid8")
    with _ctx() as ctx:
        _set_box(ctx, mdl)
        ctx.set_trip_order(np.random.default_rng(3).permutation(trips))
        _assert_columns_are_spmv(ctx, "order")
        ctx.set_option("grid_blocks", 8)
        _assert_columns_are_spmv(ctx, "order+grid8", ks=(5,))


def test_option_order_does_not_matter():
    mdl = BOXES["toggle_2x2"]()
    X = _columns(mdl.n, 3, np.random.default_rng(9))
    with _ctx() as ctx:
        ctx.set_matrix_box(mdl, store=False)
        ctx.set_option("block_box", 1)             # after the generator
        Y1 = ctx.spmm(X)
    with _ctx() as ctx:
        _set_box(ctx, mdl)                         # before it
        Y2 = ctx.spmm(X)
    assert np.array_equal(_bits(Y1), _bits(Y2))


def test_expv_block_matches_dense_exponential():
    tol, t = 1e-8, 0.3
    with _ctx() as ctx:
        _set_box(ctx, _synth().toggle(20, 15))
        n = ctx.n
        assert n == 300
        A = _dense(ctx, n)
        W = _start_block(n, np.random.default_rng(1))
        ctx.set_block(W)
        wsum, st = ctx.expv_block(t, tol, m=30)
        R = ctx.get_block()
        ref = np.maximum(sl.expm(t * A) @ W, 0.0)
        assert st.nstep >= 1 and st.t_now == pytest.approx(t)
        for j in range(W.shape[1]):
            assert np.abs(R[:, j] - ref[:, j]).sum() <= 10 * tol, j
            assert np.all(R[:, j] >= 0.0)
            assert wsum[j] <= 1.0 + 1e-12
            if wsum[j] > 0:
                assert wsum[j] == pytest.approx(R[:, j].sum(), rel=1e-14)
        assert np.all(R[:, 5] == 0.0) and wsum[5] == 0.0


def test_absorbing_state_breaks_down_alone():
    tol, t = 1e-8, 0.5
    with _ctx() as ctx:
        _set_box(ctx, _absorbing_box())
        N = ctx.n
        A = _dense(ctx, N)
        assert np.all(A[:, 0] == 0.0)
        W = np.zeros((N, 3))
        W[0, 0] = 1.0
        W[150, 1] = 1.0
        W[:, 2] = 1.0 / N
        ctx.set_block(W)
        wsum, st = ctx.expv_block(t, tol)
        R = ctx.get_block()
        assert st.n_breakdown_cols >= 1
        assert np.array_equal(_bits(R[:, 0]), _bits(W[:, 0])) and wsum[0] == 1.0
        ref = np.maximum(sl.expm(t * A) @ W, 0.0)
        for j in (1, 2):
            assert np.abs(R[:, j] - ref[:, j]).sum() <= 10 * tol
            assert wsum[j] <= 1.0 + 1e-12


def test_columns_are_independent():
    tol, t = 1e-8, 0.3
    with _ctx() as ctx:
        _set_box(ctx, BOXES["toggle_2x2"]())
        n = ctx.n
        rng = np.random.default_rng(2)
        W = np.zeros((n, 6))
        for j in range(5):
            p = rng.random(n) ** (j + 1)
            W[:, j] = p / p.sum()
        ctx.set_block(W)
        ctx.expv_block(t, tol)
        R6 = ctx.get_block()
        for j in range(6):
            ctx.set_block(W[:, j:j + 1])
            ctx.expv_block(t, tol)
            R1 = ctx.get_block()[:, 0]
            assert np.abs(R6[:, j] - R1).sum() <= 10 * tol, j
        assert np.all(R6[:, 5] == 0.0)


def test_single_vector_path_is_untouched():
    mdl = BOXES["toggle_2x2"]()
    n = mdl.n
    w = _synth().poisson_p0(mdl, 20.0)
    runs = []
    for with_block in (False, True):
        with _ctx() as ctx:
            _set_box(ctx, mdl)
            ctx.set_vector(w)
            if with_block:
                ctx.set_block(_start_block(n, np.random.default_rng(7)))
                ctx.expv_block(0.3, 1e-8)
                ctx.spmm(np.ones((n, 3)))
                ctx.spmm_bench(2)
                assert np.array_equal(_bits(ctx.get_vector()), _bits(w))
            ws = ctx.expv_fixed(30, 0.01, 3)
            runs.append((ws, ctx.get_vector()))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_refusals():
    from krylovfspssa_amd.host import KfspError, run_loopback_ranks
    synth = _synth()
    mdl = synth.toggle(60, 50)
    W = np.ones((mdl.n, 2))
    with _ctx() as ctx:                            # the option is off by default
        ctx.set_matrix_box(mdl, store=False)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.set_block(W)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.spmm(W)
    with _ctx() as ctx:                            # two-factor propensities: no single-factor descriptor
        gb = synth.goutsias_box((9, 8, 7, 3, 3, 3))
        _set_box(ctx, gb)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.set_block(np.ones((gb.n, 2)))
        with pytest.raises(KfspError, match="-> -12"):
            ctx.spmm(np.ones((gb.n, 2)))
    with _ctx() as ctx:                            # the interpreted kernel is asked for
        _set_box(ctx, mdl, box_generic=1)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.set_block(W)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.spmm(W)
        ctx.set_option("box_generic", 0)           # read when the block call is made
        ctx.set_block(W)

    def body(ctx, rank):                           # contexts with a communicator
        ctx.set_option("block_box", 1)
        r0, nr = ctx.row_block(mdl.n)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows(r0, nr))
        Y = np.empty_like(W)
        return ctx._lib.kfsp_spmm(ctx._h, 1, mdl.n, W.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p))
    assert run_loopback_ranks(2, body) == [-12, -12]


def test_generator_change_releases_the_block():
    from krylovfspssa_amd.host import KfspError
    mdl = _synth().toggle(60, 50)
    W = np.ones((mdl.n, 2))
    with _ctx() as ctx:
        ctx.set_option("block_box", 1)
        ctx.set_matrix_box(mdl, store=True)        # stored box
        ctx.set_block(W)
        ctx.get_block()
        ctx.set_matrix_box(mdl, store=False)       # the same box matrix-free: the block is gone
        with pytest.raises(KfspError, match="no block resident"):
            ctx.get_block()
        with pytest.raises(KfspError):
            ctx.expv_block(0.1, 1e-8)
        ctx.set_block(W)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W))
        ctx.set_matrix_box(mdl, store=False)       # kfsp_set_matrix_box itself
        with pytest.raises(KfspError, match="no block resident"):
            ctx.get_block()
        ctx.set_block(W)
        ctx.set_matrix_box(mdl, store=True)        # and back to the stored form
        with pytest.raises(KfspError, match="no block resident"):
            ctx.get_block()
