"""Block exp(tA)W (kfsp_set_block / kfsp_spmm / kfsp_expv_block) against references that are not the library itself:
host CSR products, the oracle's single-vector step (oracle/kfsp_oracle.c), the CPU restatement of the block step
control (tests/block_ref.py), dense expm and the analytic birth-death distribution (tests/bd_truth.py).  At sizes where
k_spmm loops over trips and the flat kernels' grid-stride loops turn, for every padded width kp = 2, 4, 8, 16, under a
trip order, and through the C ABI with padded strides.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp

from oracle import oracle as O
from tests import bd_truth
from tests import block_generators
from tests import block_ref as BR

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _synth():
    from krylovfspssa_amd import synth
    return synth


GENERATORS = block_generators.GENERATORS


def _setup(ctx, golden_dir, kind):
    fmt, ell = GENERATORS[kind](ctx, golden_dir)
    if fmt is not None:
        assert ctx.layout_info()["format"] == fmt, (kind, ctx.layout_info())
    return O.EllMatrix(*ell)


def _trips(ctx):
    """wavefront trips of a product (include/kfsp.h, kfsp_set_trip_order): 128 rows banded, 64 rows SELL"""
    lay = ctx.layout_info()
    return (lay["chunks"] + 1) // 2 if lay["format"] in (1, 2) else lay["chunks"]


def _start(n, k, rng):
    """unit vectors, probability vectors and a column of mass 2.5: the betas differ from column to column"""
    W = np.zeros((n, k))
    for c in range(k):
        if c % 3 == 0:
            W[(7919 * c + 3) % n, c] = 1.0
        elif c % 3 == 1:
            p = rng.random(n) ** (c % 5 + 1)
            W[:, c] = p / p.sum()
        else:
            p = rng.random(n)
            W[:, c] = 2.5 * p / p.sum()
    return W


def _assert_product(A, absA, X, Y):
    """row by row within 1e-13 |A||x| of the host CSR product: the kernel and scipy sum a row's at most 7 terms in
    different orders, each rounding at most eps |a_ij x_j| away, so they differ by < 14 eps |A||x| = 3.1e-15 |A||x|;
    one wrong or missing entry moves a row by O(|a_ij x_j|)"""
    ref = A @ X
    bound = 1e-13 * (absA @ np.abs(X))
    bad = np.abs(Y - ref) > bound
    assert not bad.any(), (np.argwhere(bad)[:5], Y[bad][:5], ref[bad][:5])


def _spmm_checks(ctx, A, ks, rng):
    absA = abs(A)
    for k in ks:
        X = rng.standard_normal((ctx.n, k))
        X[:, 0] = np.abs(X[:, 0])
        Y = ctx.spmm(X)
        _assert_product(A, absA, X, Y)
        for j in range(k):
            assert np.array_equal(_bits(Y[:, j]), _bits(ctx.spmv(X[:, j]))), (k, j)


# ---- 1. products at scale
BIG_DIMS = (96, 80, 72)                      # 552 960 states: > 4096 trips of 128 rows, > 8192 trips of 64 rows


@pytest.fixture(scope="module")
def big_box():
    mdl = _synth().birth_death(BIG_DIMS)
    rp, col, val = mdl.csr_rows()
    return mdl, (rp, col, val), sp.csr_matrix((val, col, rp), shape=(mdl.n, mdl.n))


@pytest.mark.parametrize("fmt", ["banded", "sell"])
def test_spmm_at_scale_is_the_host_product_and_spmv(big_box, fmt):
    """spmm_grid caps the grid at 1024 workgroups of 4 wavefronts, 512 per XCD slice of the trips: the banded box's
    4320 trips are 8 slices of 540 (28 wavefronts per slice take a second trip), the SELL one's 8640 are 8 of 1080
    (every wavefront takes two or three)"""
    mdl, csr, A = big_box
    with _ctx() as ctx:
        if fmt == "sell":
            ctx.set_option("format", 1)
            ctx.set_option("sell_code", 0)
            ctx.set_matrix_ell(*mdl.ell())
        else:
            ctx.set_matrix_csr(mdl.n, *csr)
        assert ctx.layout_info()["format"] == (0 if fmt == "sell" else 1)
        assert _trips(ctx) > 4 * 1024
        _spmm_checks(ctx, A, (1, 2, 4, 7, 9, 16), np.random.default_rng(1))


@pytest.mark.parametrize("grid", [8, 24])
@pytest.mark.parametrize("fmt", ["banded", "sell"])
def test_spmm_trip_loop_with_a_small_grid(fmt, grid):
    """option grid_blocks: 8 workgroups (4 wavefronts per XCD slice of 13 banded / 26 SELL trips: each takes 3 to 7)
    or 24 (12 per slice: one banded wavefront, every SELL one takes a second)"""
    mdl = _synth().toggle(120, 110)
    rp, col, val = mdl.csr_rows()
    A = sp.csr_matrix((val, col, rp), shape=(mdl.n, mdl.n))
    with _ctx(grid_blocks=grid) as ctx:
        if fmt == "sell":
            ctx.set_option("format", 1)
            ctx.set_matrix_ell(*mdl.ell())
        else:
            ctx.set_option("dia_mask", 0)
            ctx.set_matrix_csr(mdl.n, rp, col, val)
        assert _trips(ctx) > 4 * grid
        _spmm_checks(ctx, A, (1, 2, 4, 7, 9, 16), np.random.default_rng(2))


# ---- 2. trip order
def _assert_solve_matches_ref(R, ws, st, Rref, wsref, stref, W):
    """the block solve against block_ref: the same decisions (counts exact, step sizes to 1e-12 relative - both sides
    take the same two-digit step sizes, so they are equal unless a decision differs), every column within 1e-10 l1 of
    the restatement, start mass up to 2.5 included (the oracle's Arnoldi and Pade against the kernels' differ by rounding
    only: fixed-order GPU partial sums against sequential BLAS-1), wsum alike"""
    assert (st.nstep, st.nreject, st.nmult, st.n_breakdown_cols) == \
        (stref.nstep, stref.nreject, stref.nmult, stref.n_breakdown_cols), (st, stref)
    for f in ("t_now", "step_min", "step_max"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-12, abs=0), f
    # ERR_LOC is the tail |E(m+1,1)| beta of exp(tH), which the rounding of H moves by up to t |H| eps |exp(tH)|: near
    # the rounding floor (ERR_LOC ~ 1e-15, the small-n runs) that is 5e-6 relative on the GPU, more for stiff H; the
    # error statistics are reports, held to 1e-2 relative
    for f in ("x_error", "s_error"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-2, abs=1e-300), f
    for c in range(W.shape[1]):
        assert np.abs(R[:, c] - Rref[:, c]).sum() <= 1e-10, c
        assert abs(ws[c] - wsref[c]) <= 1e-12, c


@pytest.mark.parametrize("kind", ["sell", "sell_coded", "banded", "masked_banded"])
def test_trip_order_changes_no_bits(golden_dir, kind):
    """rows are independent, so a random order of the trips gives the same bits (include/kfsp.h); the solve under the
    order meets the restatement"""
    t, tol, m = 0.05, 1e-10, 30
    with _ctx() as ctx:
        A = _setup(ctx, golden_dir, kind)
        n = ctx.n
        rng = np.random.default_rng(3)
        X = rng.standard_normal((n, 16))
        plain = {k: ctx.spmm(X[:, :k]) for k in (3, 16)}
        y = ctx.spmv(X[:, 0])
        ctx.set_trip_order(rng.permutation(_trips(ctx)).astype(np.int32))
        for k in (3, 16):
            assert np.array_equal(_bits(ctx.spmm(X[:, :k])), _bits(plain[k])), k
        assert np.array_equal(_bits(ctx.spmv(X[:, 0])), _bits(y))
        W = _start(n, 5, rng)
        ctx.set_block(W)
        ws, st = ctx.expv_block(t, tol, m)
        R = ctx.get_block()
    Rref, wsref, stref = BR.expv_block(A, W, t, tol, m)
    _assert_solve_matches_ref(R, ws, st, Rref, wsref, stref, W)


def test_trip_order_refusals_and_lifetime(golden_dir):
    from krylovfspssa_amd.host import KfspError
    with _ctx() as ctx:
        _setup(ctx, golden_dir, "sell")
        n, T = ctx.n, _trips(ctx)
        lib, h = ctx._lib, ctx._h
        order = np.random.default_rng(4).permutation(T).astype(np.int32)
        longer = np.concatenate([order, [T]]).astype(np.int32)
        assert lib.kfsp_set_trip_order(h, T + 1, _p(longer)) == -2
        assert lib.kfsp_set_trip_order(h, T - 1, _p(order)) == -2
        dup = order.copy()
        dup[1] = dup[0]
        assert lib.kfsp_set_trip_order(h, T, _p(dup)) == -3
        oob = order.copy()
        oob[0] = T
        assert lib.kfsp_set_trip_order(h, T, _p(oob)) == -3
        # What follows checks return codes and that products stay right after each call, nothing more: no result shows
        # which order is in effect.  The products' bits do not depend on it (test_trip_order_changes_no_bits), the
        # solve's did not either on this generator (its Arnoldi dot products came out with the same bits under a
        # random order), and an order whose length is not the trip count is ignored (kfsp_block.hip spmm).  That a
        # new generator drops the order and ntrips = 0 restores ascending is therefore only exercised, not observed.
        X = np.random.default_rng(5).standard_normal((n, 4))
        Y = ctx.spmm(X)
        assert lib.kfsp_set_trip_order(h, T, _p(order)) == 0
        assert lib.kfsp_set_trip_order(h, 0, None) == 0           # ntrips = 0
        assert np.array_equal(_bits(ctx.spmm(X)), _bits(Y))
        ctx.set_trip_order(order)
        _setup(ctx, golden_dir, "sell")                            # a new generator of the same trip count
        assert _trips(ctx) == T
        assert np.array_equal(_bits(ctx.spmm(X)), _bits(Y))
        _setup(ctx, golden_dir, "banded")
        with pytest.raises(KfspError, match="-> -2"):              # an order of another generator's trip count: refused
            ctx.set_trip_order(order)


# ---- 3. one step against the oracle
@pytest.mark.parametrize("kind", list(GENERATORS))
def test_one_step_matches_the_oracle(golden_dir, kind):
    """t far below the first step size: one Krylov step per column, kfo_expv_fixed(A, W_c, m, t, 1) - the reference's
    arithmetic; the single-vector solve is held to the same 1e-10 (tests/test_gpu_parity.py)"""
    m, tol, t = 30, 1e-10, 2e-4
    with _ctx() as ctx:
        A = _setup(ctx, golden_dir, kind)
        n = ctx.n
        rng = np.random.default_rng(6)
        for k in (1, 2, 3, 4, 5, 8, 9, 16):           # kp 2, 4, 8, 16, with and without padding columns
            W = _start(n, k, rng)
            assert t < BR.first_step(m, tol, np.linalg.norm(W, axis=0).max())
            ctx.set_block(W)
            ws, st = ctx.expv_block(t, tol, m)
            R = ctx.get_block()
            assert (st.nstep, st.nreject, st.nmult, st.t_now) == (1, 0, m + 1, t), (k, st.nstep, st.nreject)
            for c in range(k):
                w1, ws1 = O.expv_fixed(A, W[:, c], m, t, 1)
                beta = np.linalg.norm(W[:, c])
                assert np.abs(R[:, c] - w1).sum() <= 1e-10 * beta, (k, c)
                assert abs(ws[c] - ws1[0]) <= 1e-12, (k, c)


# ---- 4. adaptive solves against the restatement
def _bd(dims, **kw):
    return _synth().birth_death(dims, **kw)


ADAPTIVE = {
    # name: (model, t, tol, m, k) - the step counts block_ref gives are in the comments.  Every decision of these cases
    # (and of test_small_and_ragged_n) stays the same when every ERR_LOC of the restatement moves by 1e-3 relative;
    # the GPU's ERR_LOC differ from the restatement's by ~5e-6 relative
    "several_steps": (lambda: _synth().toggle(60, 50), 0.3, 1e-8, 30, 6),             # 4 steps, 2 rejections
    # t |A| ~ 20: rejections.  (A stiffer box, t |A| ~ 270, magnifies the rounding of H until a step size truncated
    # to two digits lands on the other side of a digit on the GPU; this one keeps every decision under a 5 % change of
    # every ERR_LOC in the restatement.)
    "stiff": (lambda: _bd((30, 20), k=(100.0, 150.0), g=(10.0, 20.0)), 0.02, 1e-10, 30, 5),  # 3 steps, 1 rejection
    "tol_below_eps": (lambda: _synth().toggle(60, 50), 0.1, 1e-17, 30, 5),           # krytol = sqrt(eps)
    "m1": (lambda: _bd((10, 8)), 2e-8, 1e-6, 1, 5),                     # 3 steps, 1 rejection
    "m2": (lambda: _bd((10, 8)), 1e-4, 1e-6, 2, 5),                     # 3 steps, 1 rejection
    "m10": (lambda: _bd((30, 20)), 0.1, 1e-10, 10, 5),                 # 7 steps, 4 rejections
    "m_capped_at_n_minus_1": (lambda: _bd((40,)), 1.0, 1e-10, 100, 5),
    "m_max": (lambda: _bd((30, 20)), 2.0, 1e-10, 100, 5),
}


@pytest.mark.parametrize("name", list(ADAPTIVE))
def test_adaptive_solve_matches_the_restatement(name):
    make, t, tol, m, k = ADAPTIVE[name]
    mdl = make()
    ell = mdl.ell()
    W = _start(mdl.n, k, np.random.default_rng(7))
    with _ctx() as ctx:
        ctx.set_option("dia_mask", 0)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ctx.set_block(W)
        ws, st = ctx.expv_block(t, tol, m)
        R = ctx.get_block()
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*ell), W, t, tol, m)
    if name == "stiff":
        assert stref.nreject >= 1
    assert stref.nstep >= 2 or name == "m_max"
    _assert_solve_matches_ref(R, ws, st, Rref, wsref, stref, W)


def test_m_above_the_basis_is_refused(golden_dir):
    from krylovfspssa_amd.host import KfspError
    with _ctx() as ctx:
        _setup(ctx, golden_dir, "sell")
        ctx.set_block(np.ones((ctx.n, 2)) / ctx.n)
        with pytest.raises(KfspError, match="-> -4"):
            ctx.expv_block(0.1, 1e-8, m=101)                      # > M_MAX
        ctx.set_option("m_max", 20)
        with pytest.raises(KfspError, match="-> -4"):
            ctx.expv_block(0.1, 1e-8, m=21)                       # > block_mmax
        ctx.expv_block(0.1, 1e-8, m=20)


# ---- 5. large n against the analytic distribution
LARGE_DIMS = (80, 70, 60)                                         # 336 000 states; kp 16: 5.4M doubles per block column


def _large_solve(W, t, tol, **opts):
    mdl = _bd(LARGE_DIMS)
    with _ctx(**opts) as ctx:
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ctx.set_block(W)
        ws, st = ctx.expv_block(t, tol, 30)
        return ctx.get_block(), ws, st


def test_large_birth_death_meets_the_analytic_distribution():
    """16 start states, default grids and then grid_blocks 8 / vec_grid_blocks 3 (every flat kernel loops ~3500 times
    per thread).  The FSP relation of tests/bd_truth.py per column: the solve accepts ERR_LOC <= DELTA tol t_step per
    step, so R may exceed the truth by at most DELTA tol t in total (beta = 1), and sum(truth - R) is the mass R lost"""
    t, tol = 0.6, 1e-10
    k, g = bd_truth.default_rates(3)
    n = int(np.prod(LARGE_DIMS))
    rng = np.random.default_rng(8)
    x0s = [tuple(int(rng.integers(0, 35)) for _ in range(3)) for _ in range(16)]
    W = np.zeros((n, 16))
    for c, x0 in enumerate(x0s):
        W[x0[0] + LARGE_DIMS[0] * (x0[1] + LARGE_DIMS[1] * x0[2]), c] = 1.0
    bound = BR.DELTA * tol * t
    runs = [_large_solve(W, t, tol), _large_solve(W, t, tol, grid_blocks=8, vec_grid_blocks=3)]
    for R, ws, st in runs:
        assert st.t_now == t
        for c, x0 in enumerate(x0s):
            truth, out = bd_truth.box_pmf(LARGE_DIMS, k, g, x0, t)
            assert out < 1e-14
            d = truth - R[:, c]
            assert d.min() >= -bound, (c, d.min())
            assert abs(d.sum() - (1.0 - ws[c])) <= bound, (c, d.sum(), 1.0 - ws[c])
            assert np.abs(d).sum() <= (1.0 - ws[c]) + 2 * bound, c
    (Ra, wa, sa), (Rb, wb, sb) = runs
    # two partial-sum orders of the same arithmetic: the same decisions, rounding apart
    assert (sa.nstep, sa.nreject) == (sb.nstep, sb.nreject)
    for c in range(16):
        assert np.abs(Ra[:, c] - Rb[:, c]).sum() <= 1e-12, c


# ---- 6. small and ragged n
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("fmt", ["banded", "sell"])
def test_small_and_ragged_n(fmt, n):
    """a one-species birth-death chain: m = 30 is capped at n - 1 (n = 1: m = 1, the space runs out at once; n = 2, 3:
    m = 1, 2 take steps of about (tol / |A|^2)^(1/m), hence the short intervals).  Against dense expm: the solve's error
    is estimated at <= DELTA tol t beta in the 2-norm, at most sqrt(n) times that in l1; against the restatement as in
    the adaptive tests"""
    t, tol = {2: (5e-8, 1e-6), 3: (1e-4, 1e-8)}.get(n, (0.5, 1e-12))
    m = 30
    mdl = _bd((n,))
    rp, col, val = mdl.csr_rows()
    W = np.zeros((n, 3))
    W[0, 0] = 1.0
    W[n - 1, 1] = 1.0
    W[:, 2] = 1.0 / n
    with _ctx() as ctx:
        if fmt == "sell":
            ctx.set_option("format", 1)
            ctx.set_matrix_ell(*mdl.ell())
        else:
            ctx.set_matrix_csr(n, rp, col, val)
        ctx.set_block(W)
        ws, st = ctx.expv_block(t, tol, m)
        R = ctx.get_block()
    A = sp.csr_matrix((val, col, rp), shape=(n, n)).toarray()
    ref = np.maximum(sl.expm(t * A) @ W, 0.0)
    for c in range(3):
        beta = np.linalg.norm(W[:, c])
        assert np.abs(R[:, c] - ref[:, c]).sum() <= BR.DELTA * tol * t * beta * np.sqrt(n) + 1e-14, (c, n)
    if n == 1:
        assert st.n_breakdown_cols == 3
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*mdl.ell()), W, t, tol, m)
    _assert_solve_matches_ref(R, ws, st, Rref, wsref, stref, W)


# ---- 7. columns
@pytest.mark.parametrize("kind", ["sell", "banded"])
def test_duplicate_columns_are_bit_identical(golden_dir, kind):
    """every per-column reduction has the same shape whatever the column's slot in the 16-wide row, so equal start
    columns give equal bits; zero columns stay exactly 0 with wsum 0"""
    with _ctx() as ctx:
        _setup(ctx, golden_dir, kind)
        n = ctx.n
        rng = np.random.default_rng(9)
        p = rng.random(n)
        p /= p.sum()
        q = rng.random(n) ** 3
        q /= q.sum()
        e = np.zeros(n)
        e[n // 3] = 1.0
        z = np.zeros(n)
        src = [p, e, q, z, p, q, e, z, p, e, q, p, z, e, q, p]
        ctx.set_block(np.stack(src, axis=1))
        ws, st = ctx.expv_block(0.3, 1e-8)
        R = ctx.get_block()
    assert st.nstep >= 2
    for s in (p, e, q, z):
        cols = [c for c in range(16) if src[c] is s]
        for c in cols[1:]:
            assert np.array_equal(_bits(R[:, c]), _bits(R[:, cols[0]])), (cols[0], c)
            assert _bits(ws[c]) == _bits(ws[cols[0]])
    for c in (3, 7, 12):
        assert np.array_equal(_bits(R[:, c]), _bits(np.zeros(n))) and _bits(ws[c]) == 0


# ---- 8. ABI contract
def test_padded_leading_dimension_is_neither_read_nor_written(golden_dir):
    """ld = n + 5 with NaN in the gap: a read of the gap would spread NaN into the results, a write would overwrite it"""
    k = 5
    with _ctx() as ctx:
        _setup(ctx, golden_dir, "sell")
        n = ctx.n
        lib, h = ctx._lib, ctx._h
        ld = n + 5
        W = _start(n, k, np.random.default_rng(10))
        ctx.set_block(W)
        ws0, _ = ctx.expv_block(0.2, 1e-8)
        R0 = ctx.get_block()
        Y0 = ctx.spmm(W)

        Wp = np.full((k, ld), np.nan)                  # column j at Wp[j * ld + i]
        Wp[:, :n] = W.T
        assert lib.kfsp_set_block(h, k, n, ld, _p(Wp)) == 0
        Out = np.full((k, ld), np.nan)
        assert lib.kfsp_get_block(h, k, n, ld, _p(Out)) == 0
        assert np.array_equal(_bits(Out[:, :n]), _bits(W.T)) and np.isnan(Out[:, n:]).all()
        ws1, _ = ctx.expv_block(0.2, 1e-8)
        Out[:] = np.nan
        assert lib.kfsp_get_block(h, k, n, ld, _p(Out)) == 0
        assert np.array_equal(_bits(Out[:, :n]), _bits(R0.T)) and np.isnan(Out[:, n:]).all()
        assert np.array_equal(_bits(ws1), _bits(ws0))

        Yp = np.full((k, ld), np.nan)
        assert lib.kfsp_spmm(h, k, ld, _p(Wp), _p(Yp)) == 0
        assert np.array_equal(_bits(Yp[:, :n]), _bits(Y0.T)) and np.isnan(Yp[:, n:]).all()
        assert np.isnan(Wp[:, n:]).all()


def _expect_no_block(ctx):
    from krylovfspssa_amd.host import KfspError
    with pytest.raises(KfspError, match="-> -1"):
        ctx.get_block()
    with pytest.raises(KfspError, match="-> -1"):
        ctx.expv_block(0.1, 1e-8)


def test_update_matrix_ell_discards_the_block():
    mdl = _synth().toggle(60, 50)
    ell = mdl.ell()
    with _ctx() as ctx:
        ctx.set_matrix_ell(*ell)
        ctx.set_block(np.ones((mdl.n, 3)))
        ctx.get_block()
        ctx.update_matrix_ell(*ell, mdl.n)
        _expect_no_block(ctx)


def test_drop_compact_discards_the_block():
    mdl = _synth().toggle(60, 50)
    with _ctx() as ctx:
        ctx.set_matrix_ell(*mdl.ell())
        w = _synth().poisson_p0(mdl, 10.0)                # a Poisson bump: most of the box carries next to nothing
        ctx.set_vector(w)
        ctx.set_block(np.stack([w, w], axis=1))
        ctx.get_block()
        droptol, cnt, nflag = ctx.drop_plan(1e-7)
        assert nflag > 0
        ctx.drop_compact()
        _expect_no_block(ctx)


def test_expand_resident_discards_the_block(golden_dir):
    from tests.expand_helpers import grown, mass_action
    with _ctx() as ctx:
        nu, state, adj = grown(ctx, "toggle_k20", golden_dir, 1)
        nr, ns = nu.shape
        params, progs = mass_action(nu)
        ctx.set_propensity_program(ns, params, progs)
        off, diag = ctx.propensities(state)
        ctx.set_option("keep_coords", 1)
        ctx.set_state_coords(state)
        ctx.set_matrix_ell(adj, off, diag)
        n = len(state)
        ctx.set_vector(np.full(n, 1.0 / n))
        ctx.set_block(np.ones((n, 2)) / n)
        ctx.get_block()
        ctx.expand_resident(2.0 / float(np.mean(diag[diag > 0])), 12345, nu)
        _expect_no_block(ctx)


def test_other_products_leave_the_resident_block_alone(golden_dir):
    """kfsp_spmm with another k (another kp) and kfsp_spmm_bench work in the basis, never in the block"""
    with _ctx() as ctx:
        _setup(ctx, golden_dir, "sell")
        n = ctx.n
        W = _start(n, 5, np.random.default_rng(12))
        ctx.set_block(W)
        ws0, _ = ctx.expv_block(0.2, 1e-8)
        R0 = ctx.get_block()
        ctx.set_block(W)
        X = np.random.default_rng(13).standard_normal((n, 16))
        ctx.spmm(X)
        ctx.spmm(X[:, :2])
        ctx.spmm_bench(3)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W))
        ws1, _ = ctx.expv_block(0.2, 1e-8)
        assert np.array_equal(_bits(ctx.get_block()), _bits(R0)) and np.array_equal(_bits(ws1), _bits(ws0))
