"""Several start vectors at once (kfsp_set_block / kfsp_spmm / kfsp_expv_block): the block product is kfsp_spmv column by
column, bit for bit, on every stored format; the block solve matches dense exp(tA) column by column, its columns are
independent, and nothing of the single-vector path changes.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl

from tests import block_generators

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8, 16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ctx():
    from krylovfspssa_amd import KfspContext
    return KfspContext(0)


def _golden_toggle(golden_dir):
    return block_generators.golden_toggle(golden_dir)


def _csr_of_box(mdl):
    return mdl.csr_rows()


def _dense(ctx, n):
    """A as a dense matrix through the library's own product"""
    return np.column_stack([ctx.spmv(np.eye(n)[:, i]) for i in range(n)])


# ---- generators (tests/block_generators.py), each with the kernel format it must end up in (kfsp_layout_info v[0])
def _sell(ctx, golden_dir):
    return block_generators.sell(ctx, golden_dir)[0]


GENERATORS = block_generators.GENERATORS


@pytest.mark.parametrize("kind", list(GENERATORS))
def test_spmm_is_spmv_column_by_column_bit_for_bit(golden_dir, kind):
    with _ctx() as ctx:
        fmt, _ = GENERATORS[kind](ctx, golden_dir)
        if fmt is not None:
            assert ctx.layout_info()["format"] == fmt, (kind, ctx.layout_info())
        n = ctx.n
        assert n % 128 != 0
        rng = np.random.default_rng(5)
        for k in KS:
            X = rng.standard_normal((n, k))
            X[:, 0] = np.abs(X[:, 0])
            Y = ctx.spmm(X)
            for j in range(k):
                assert np.array_equal(_bits(Y[:, j]), _bits(ctx.spmv(X[:, j]))), (kind, k, j)


def _expm_cols(A, t, W):
    if A.shape[0] <= 3000:
        return sl.expm(t * A) @ W
    import scipy.sparse.linalg as spl
    return spl.expm_multiply(t * A, W)


def _start_block(n, rng):
    W = np.zeros((n, 6))
    W[3, 0] = 1.0                                  # unit vectors e_x
    W[n // 2, 1] = 1.0
    W[n - 1, 2] = 1.0
    p = rng.random(n)
    W[:, 3] = p / p.sum()                          # seeded probability vectors
    q = rng.random(n) ** 4
    W[:, 4] = q / q.sum()
    return W                                       # column 5 stays 0


@pytest.mark.parametrize("case", ["toggle_fsp", "repressilator_box"])
def test_expv_block_matches_dense_exponential(golden_dir, case):
    from krylovfspssa_amd import synth
    tol, t = 1e-8, 0.3
    with _ctx() as ctx:
        if case == "toggle_fsp":
            _sell(ctx, golden_dir)
        else:
            mdl = synth.repressilator(dims=(12, 12, 12))
            ctx.set_matrix_csr(mdl.n, *_csr_of_box(mdl))
        n = ctx.n
        A = _dense(ctx, n)
        W = _start_block(n, np.random.default_rng(1))
        ctx.set_block(W)
        wsum, st = ctx.expv_block(t, tol, m=30)
        R = ctx.get_block()
        ref = np.maximum(_expm_cols(A, t, W), 0.0)
        assert st.nstep >= 1 and st.t_now == pytest.approx(t)
        for j in range(W.shape[1]):
            assert np.abs(R[:, j] - ref[:, j]).sum() <= 10 * tol, (case, j)
            assert np.all(R[:, j] >= 0.0)
            assert wsum[j] <= 1.0 + 1e-12
            if wsum[j] > 0:
                assert wsum[j] == pytest.approx(R[:, j].sum(), rel=1e-14)
        assert np.all(R[:, 5] == 0.0) and wsum[5] == 0.0


def test_columns_are_independent(golden_dir):
    tol, t = 1e-8, 0.3
    with _ctx() as ctx:
        _sell(ctx, golden_dir)
        n = ctx.n
        rng = np.random.default_rng(2)
        W = np.zeros((n, 8))
        for j in range(7):
            p = rng.random(n) ** (j + 1)
            W[:, j] = p / p.sum()
        ctx.set_block(W)
        ctx.expv_block(t, tol)
        R8 = ctx.get_block()
        for j in (0, 4, 7):
            ctx.set_block(W[:, j:j + 1])
            ws1, _ = ctx.expv_block(t, tol)
            R1 = ctx.get_block()[:, 0]
            assert np.abs(R8[:, j] - R1).sum() <= 10 * tol
        assert np.all(R8[:, 7] == 0.0)


def _absorbing_chain(N=300, b=40.0, g=1.0):
    """birth-death chain whose state 0 is absorbing (no births from it): column 0 of A is zero, A e_0 = 0"""
    rows, cols, vals = [], [], []
    birth = lambda i: b if 0 < i < N - 1 else 0.0   # noqa: E731
    death = lambda i: g * i                         # noqa: E731
    for i in range(N):
        ent = []
        if i >= 1 and birth(i - 1) > 0:
            ent.append((i - 1, birth(i - 1)))
        out = birth(i) + death(i)
        if out > 0:
            ent.append((i, -out))
        if i + 1 < N and death(i + 1) > 0:
            ent.append((i + 1, death(i + 1)))
        for c, v in ent:
            rows.append(i)
            cols.append(c)
            vals.append(v)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.add.at(rowptr, np.asarray(rows) + 1, 1)
    return N, np.cumsum(rowptr), np.asarray(cols, dtype=np.int32), np.asarray(vals)


def test_absorbing_state_breaks_down_alone():
    tol, t = 1e-8, 0.5
    with _ctx() as ctx:
        N, rp, col, val = _absorbing_chain()
        ctx.set_matrix_csr(N, rp, col, val)
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


def test_block_solve_is_reproducible(golden_dir):
    with _ctx() as ctx:
        _sell(ctx, golden_dir)
        W = _start_block(ctx.n, np.random.default_rng(4))
        out = []
        for _ in range(2):
            ctx.set_block(W)
            ws, st = ctx.expv_block(0.3, 1e-8)
            out.append((ctx.get_block(), ws, st.nstep))
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
        assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and out[0][2] == out[1][2]


def test_single_vector_path_is_untouched(golden_dir):
    g = _golden_toggle(golden_dir)
    n = len(g["diag"])
    w = np.zeros(n)
    w[0] = 1.0
    runs = []
    for with_block in (False, True):
        with _ctx() as ctx:
            ctx.set_matrix_ell(g["adj"], g["offdiag"], g["diag"])
            ctx.set_vector(w)
            if with_block:
                ctx.set_block(_start_block(n, np.random.default_rng(7)))
                ctx.expv_block(0.3, 1e-8)
                ctx.spmm(np.ones((n, 3)))
                ctx.spmm_bench(2)
                assert np.array_equal(_bits(ctx.get_vector()), _bits(w))
            rc, st, _ = ctx.dgexpv(0.5, 1e-4, 1e-8, int(g["nr"]))
            runs.append((rc, ctx.get_vector(), st.nstep))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2]
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


def test_refusals(golden_dir):
    from krylovfspssa_amd import KfspContext, synth
    from krylovfspssa_amd.host import KfspError
    mdl = synth.toggle(60, 50)
    W = np.ones((mdl.n, 2))
    with _ctx() as ctx:                            # matrix-free box
        ctx.set_matrix_box(mdl, store=False)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.set_block(W)
        with pytest.raises(KfspError, match="-> -12"):
            ctx.spmm(W)
        ctx.set_matrix_box(mdl, store=True)        # the same box stored: accepted
        ctx.set_block(W)
        assert np.allclose(ctx.spmm(W)[:, 0], ctx.spmv(W[:, 0]))
    with KfspContext(0, group=2) as head:          # loop-back group head
        head.set_matrix_csr(mdl.n, *_csr_of_box(mdl))
        with pytest.raises(KfspError, match="-> -12"):
            head.set_block(W)
    from krylovfspssa_amd.host import run_loopback_ranks

    def body(ctx, rank):                           # contexts with a communicator
        r0, nr = ctx.row_block(mdl.n)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows(r0, nr))
        Y = np.empty_like(W)
        return ctx._lib.kfsp_spmm(ctx._h, 1, mdl.n, W.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p))
    assert run_loopback_ranks(2, body) == [-12, -12]
    with _ctx() as ctx:                            # a new generator discards the block
        _sell(ctx, golden_dir)
        ctx.set_block(np.ones((ctx.n, 2)))
        ctx.get_block()
        _sell(ctx, golden_dir)
        with pytest.raises(KfspError):
            ctx.get_block()
        with pytest.raises(KfspError):
            ctx.expv_block(0.1, 1e-8)
