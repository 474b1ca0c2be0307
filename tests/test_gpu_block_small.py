"""Block exp(tA)W on small generators (option block_small): where the single-vector path takes its one-launch Arnoldi
pass, a block step is three launches of one workgroup per block column.  The pass of a column is the single-vector
pass bit for bit (H, norms, AVNORM), columns are independent, a breakdown or a zero column stays that column's
business and leaves nothing stale in the basis, the combine is k_bcombine's element for element, whole solves meet
dense expm, the oracle and the CPU restatement, and without the option nothing changes.  Needs a real MI355X."""
import numpy as np
import pytest
import scipy.linalg as sl

from oracle import oracle as O
from tests import block_generators
from tests import block_ref as BR
from tests.test_gpu_block import _absorbing_chain, _dense, _start_block

pytestmark = pytest.mark.gpu

TOL = 1e-7            # break_tol of every pass here (kfsp_expv_block's)
KS = (1, 3, 8, 16)
MS = (1, 2, 30, 100)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


def _synth():
    from krylovfspssa_amd import synth
    return synth


# ---- generators: name -> (setter(ctx, golden_dir) -> ell, small_lds, FMT of the pass kernel or None when the test
# works it out from the layout)
def _named(kind):
    return lambda ctx, golden_dir: block_generators.GENERATORS[kind](ctx, golden_dir)[1]


def _as_sell(make):
    def f(ctx, golden_dir):
        ell = make().ell()
        ctx.set_option("format", 1)
        ctx.set_option("sell_code", 0)
        ctx.set_matrix_ell(*ell)
        return ell
    return f


def _as_csr(make):
    def f(ctx, golden_dir):
        mdl = make()
        ctx.set_option("format", 0)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        return mdl.ell()
    return f


def _toggle460():
    return _synth().toggle(20, 23)              # 460 rows: more than half of the 1024 lanes own no row


def _rep4096():
    return _synth().repressilator(dims=(16, 16, 16))     # the last eligible size: every lane owns four rows


def _rep4352():
    return _synth().repressilator(dims=(17, 16, 16))     # the first size that falls back


ELIGIBLE = {
    "sell_lds": (_named("sell"), 1, 2),
    "sell_global": (_named("sell"), 0, 0),
    "banded": (_named("banded"), 1, 1),
    "masked": (_named("masked_banded"), 1, 1),
    "toggle460_sell": (_as_sell(_toggle460), 1, None),
    "toggle460_sell_global": (_as_sell(_toggle460), 0, 0),
    "rep4096": (_as_csr(_rep4096), 1, None),
    "rep4096_sell_global": (_as_sell(_rep4096), 0, 0),
}


def _setup(ctx, golden_dir, name):
    setter, lds, fmt = ELIGIBLE[name]
    ctx.set_option("small_lds", lds)
    ell = setter(ctx, golden_dir)
    assert ctx.n <= 4096
    if fmt is None:
        # banded: 1; SELL: from LDS when the image fits beside the source column, which the library decides
        fmt = 1 if ctx.layout_info()["format"] in (1, 2) else None
    return ell, fmt


def _grid_columns(n, rng):
    """16 start columns whose entries are multiples of 1/32 in [0, 8]: every sum of squares is exact in any order, so
    both paths have the same beta.  Unit vectors, dense columns, a column that lives in the last partial chunk."""
    W = np.zeros((n, 16))
    W[0, 0] = 1.0
    W[:, 1] = rng.integers(0, 257, n) / 32.0
    last = ((n - 1) // 64) * 64
    W[last:, 2] = rng.integers(1, 257, n - last) / 32.0
    W[n - 1, 3] = 8.0
    W[n // 2, 4] = 1.0 / 32.0
    for c in range(5, 16):
        W[:, c] = rng.integers(0, 257, n) / 32.0 * (rng.random(n) < (0.05 if c % 2 else 0.6))
        W[(37 * c) % n, c] = 1.0
    return W


def _single_pass(ctx, w, m):
    ctx.set_vector(w)
    beta = ctx.begin_step()
    H, mb, k1, av = ctx.arnoldi(m, 1, 2, TOL)
    return beta, H.copy(), mb, k1, av


def _assert_column_is_single_pass(out, c, ref, m, tag):
    """column c of (beta, hb, nrm, brk, avnorm) against the single-vector pass, on the bits"""
    beta_b, hb, nrm, brk, avn = out
    beta, H, mb, k1, av = ref
    assert _bits(beta_b[c]) == _bits(beta), tag
    assert _bits(nrm[1, c]) == _bits(beta), tag
    assert brk[c] == (mb if k1 == 0 else 0), (tag, brk[c], mb, k1)
    j = np.arange(1, mb + 1)
    assert np.array_equal(_bits(hb[j, 1, c]), _bits(H[j - 1, j - 1])), tag            # H(j,j)
    assert np.array_equal(_bits(hb[j[1:], 0, c]), _bits(H[j[1:] - 2, j[1:] - 1])), tag  # H(j-1,j)
    js = j if k1 != 0 else j[:-1]                                                   # H(j+1,j) = ||u_{j+1}||
    assert np.array_equal(_bits(hb[js, 2, c]), _bits(H[js, js - 1])), tag
    assert np.array_equal(_bits(nrm[js + 1, c]), _bits(H[js, js - 1])), tag
    if k1 != 0:
        assert _bits(avn[c]) == _bits(av), tag
    else:
        assert hb[mb, 2, c] <= TOL and avn[c] == 0.0, tag


def _block_pass(ctx, W, m):
    ctx.set_block(W)
    beta = ctx.block_begin(m)
    hb, nrm, brk, avn = ctx.block_arnoldi(m, TOL)
    return beta, hb, nrm, brk, avn


def _assert_small(ctx, fmt, m):
    info = ctx.block_info()
    assert info["one_launch"] == 1, info
    assert (info["begin_launches"], info["arnoldi_launches"]) == (1, 1), info
    if fmt is not None:
        assert info["fmt"] == fmt, info
    assert info["lds_bytes"] >= ((ctx.n + 63) // 64) * 64 * 8, info


# ---- 1. the path is taken
@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_small_path_is_taken(golden_dir, name):
    with _ctx(block_small=1) as ctx:
        _, fmt = _setup(ctx, golden_dir, name)
        n = ctx.n
        W = _grid_columns(n, np.random.default_rng(1))[:, :5]
        _block_pass(ctx, W, 30)
        _assert_small(ctx, fmt, 30)
        coef = np.zeros((31, 5))
        coef[0] = 1.0
        ctx.block_combine(31, coef)
        assert ctx.block_info()["combine_launches"] == 1
        ctx.set_block(W / W.sum(axis=0))
        ctx.expv_block(0.01, 1e-8, 30)
        info = ctx.block_info()
        assert (info["one_launch"], info["begin_launches"], info["arnoldi_launches"], info["combine_launches"]) == (1, 1, 1, 1)


def test_first_size_above_the_limit_falls_back():
    """4 352 rows: the multi-launch path, and the option changes no bit"""
    mdl = _rep4352()
    assert mdl.n == 4352
    W = _grid_columns(mdl.n, np.random.default_rng(2))[:, :5]
    outs = []
    for opt in (1, 0):
        with _ctx(block_small=opt) as ctx:
            ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
            out = _block_pass(ctx, W, 30)
            info = ctx.block_info()
            assert (info["one_launch"], info["begin_launches"], info["arnoldi_launches"]) == (0, 2, 4 * 30 + 3), info
            ctx.set_block(W / W.sum(axis=0))
            ws, st = ctx.expv_block(0.05, 1e-8, 30)
            assert ctx.block_info()["one_launch"] == 0
            outs.append(list(out) + [ws, ctx.get_block(), np.array([st.nstep, st.nreject])])
    for a, b in zip(*outs):
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


# ---- 2. bit identity with the single-vector pass, 3. independent columns
@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_pass_is_the_single_vector_pass_bit_for_bit(golden_dir, name):
    with _ctx(block_small=1) as ctx:
        _, fmt = _setup(ctx, golden_dir, name)
        n = ctx.n
        W = _grid_columns(n, np.random.default_rng(3))
        for m in MS:
            refs = [_single_pass(ctx, W[:, c], m) for c in range(16)]
            for k in KS:
                out = _block_pass(ctx, W[:, :k], m)
                _assert_small(ctx, fmt, m)
                for c in range(k):
                    _assert_column_is_single_pass(out, c, refs[c], m, (name, m, k, c))


@pytest.mark.parametrize("name", ["sell_lds", "sell_global", "banded"])
def test_columns_are_independent(golden_dir, name):
    """a column alone (k = 1) and in any slot of a 16-wide block: the same bits"""
    m = 30
    with _ctx(block_small=1) as ctx:
        _setup(ctx, golden_dir, name)
        n = ctx.n
        rng = np.random.default_rng(4)
        W = _grid_columns(n, rng)
        w = rng.integers(0, 257, n) / 32.0
        alone = _block_pass(ctx, w[:, None], m)
        for slot in (0, 5, 15):
            X = W.copy()
            X[:, slot] = w
            out = _block_pass(ctx, X, m)
            assert _bits(out[0][slot]) == _bits(alone[0][0])
            for a, b in zip(out[1:], alone[1:]):
                assert np.array_equal(_bits(a[..., slot].astype(np.float64)), _bits(b[..., 0].astype(np.float64))), slot


# ---- 4. per-column breakdown and zero columns
def _absorbing_ctx(**opts):
    ctx = _ctx(**opts)
    N, rp, col, val = _absorbing_chain()
    ctx.set_matrix_csr(N, rp, col, val)
    return ctx, N


def test_breakdown_and_zero_columns_stay_their_own():
    m = 30
    with _absorbing_ctx(block_small=1)[0] as ctx:
        N = ctx.n
        rng = np.random.default_rng(5)
        W = np.zeros((N, 5))
        W[0, 0] = 1.0                                  # the absorbing state: A e_0 = 0
        W[150, 2] = 1.0                                # column 1 stays 0
        W[:, 3] = 1.0 / 32.0
        W[:, 4] = rng.integers(0, 257, N) / 32.0
        out = _block_pass(ctx, W, m)
        _assert_small(ctx, None, m)
        beta, hb, nrm, brk, avn = out
        assert brk[0] == 1 and brk[1] == -1
        assert beta[1] == 0.0 and not hb[:, :, 1].any() and not nrm[:, 1].any() and avn[1] == 0.0
        assert not hb[:, :, 0].any() and not nrm[2:, 0].any() and avn[0] == 0.0       # H = 0: exp(tH) = I
        for c in (0, 2, 3, 4):
            _assert_column_is_single_pass(out, c, _single_pass(ctx, W[:, c], m), m, c)
        ctx.set_block(W)
        ws, st = ctx.expv_block(0.5, 1e-8, m)
        R = ctx.get_block()
        assert ctx.block_info()["one_launch"] == 1
        assert np.array_equal(_bits(R[:, 0]), _bits(W[:, 0])) and ws[0] == 1.0
        assert np.array_equal(_bits(R[:, 1]), _bits(np.zeros(N))) and ws[1] == 0.0
        assert st.n_breakdown_cols >= 1


def test_nothing_stale_survives_in_the_basis():
    """a dense 16-column solve fills every basis column; the next block has a zero column and an absorbing one in
    its middle: their rows of the basis must read 0 again"""
    with _absorbing_ctx(block_small=1)[0] as ctx:
        N = ctx.n
        rng = np.random.default_rng(6)
        D = rng.random((N, 16)) + 0.5
        D /= D.sum(axis=0)
        ctx.set_block(D)
        ctx.expv_block(0.5, 1e-8, 30)
        assert np.isfinite(ctx.get_block()).all()
        W = D.copy()
        W[:, 5] = 0.0
        W[:, 7] = 0.0
        W[0, 7] = 1.0
        ctx.set_block(W)
        ws, st = ctx.expv_block(0.5, 1e-8, 30)
        R = ctx.get_block()
        assert ctx.block_info()["one_launch"] == 1
        assert np.isfinite(R).all() and np.isfinite(ws).all()
        assert np.array_equal(_bits(R[:, 5]), _bits(np.zeros(N))) and ws[5] == 0.0
        assert np.array_equal(_bits(R[:, 7]), _bits(W[:, 7])) and ws[7] == 1.0
        A = _dense(ctx, N)
        ref = np.maximum(sl.expm(0.5 * A) @ W, 0.0)
        for c in range(16):
            assert np.abs(R[:, c] - ref[:, c]).sum() <= 10 * 1e-8, c


# ---- 5. combine
@pytest.mark.parametrize("name", ["sell_lds", "banded", "toggle460_sell", "rep4096"])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_combine_is_k_bcombine_element_for_element(golden_dir, name, k):
    m = 30
    with _ctx(block_small=1) as ctx:
        _setup(ctx, golden_dir, name)
        rng = np.random.default_rng(7)
        W = _grid_columns(ctx.n, rng)[:, :k]
        _block_pass(ctx, W, m)
        coef = rng.standard_normal((m + 1, k)) / 50.0      # both signs: the clamp at 0 takes part
        ws1 = ctx.block_combine(m + 1, coef)
        assert ctx.block_info()["combine_launches"] == 1
        R1 = ctx.get_block()
        ctx.set_option("block_small", 0)
        ws0 = ctx.block_combine(m + 1, coef)
        assert ctx.block_info()["combine_launches"] == 2
        R0 = ctx.get_block()
        assert (R1 > 0).any() and (R1 == 0).any()
        assert np.array_equal(_bits(R1), _bits(R0))
        # sums of the same nonnegative numbers in two orders: (n + 1) eps relative at worst, far below 1e-14 on average
        assert ws1 == pytest.approx(ws0, rel=1e-14, abs=0)


# ---- 6. whole solves
@pytest.mark.parametrize("case", ["toggle_fsp", "repressilator_box"])
def test_expv_block_matches_dense_exponential(golden_dir, case):
    tol, t = 1e-8, 0.3
    with _ctx(block_small=1) as ctx:
        if case == "toggle_fsp":
            block_generators.sell(ctx, golden_dir)
        else:
            mdl = _synth().repressilator(dims=(12, 12, 12))
            ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        n = ctx.n
        A = _dense(ctx, n)
        W = _start_block(n, np.random.default_rng(1))
        out = []
        for _ in range(2):
            ctx.set_block(W)
            wsum, st = ctx.expv_block(t, tol, m=30)
            out.append((ctx.get_block(), wsum, st.nstep))
        assert ctx.block_info()["one_launch"] == 1
        R = out[0][0]
        ref = np.maximum(sl.expm(t * A) @ W, 0.0)
        assert st.nstep >= 1 and st.t_now == pytest.approx(t)
        for j in range(W.shape[1]):
            assert np.abs(R[:, j] - ref[:, j]).sum() <= 10 * tol, (case, j)
            assert np.all(R[:, j] >= 0.0)
            assert wsum[j] <= 1.0 + 1e-12
            if wsum[j] > 0:
                assert wsum[j] == pytest.approx(R[:, j].sum(), rel=1e-14)
        assert np.all(R[:, 5] == 0.0) and wsum[5] == 0.0
        # two identical solves: identical bits
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
        assert np.array_equal(_bits(out[0][1]), _bits(out[1][1])) and out[0][2] == out[1][2]


def _start(n, k, rng):
    """tests/test_gpu_block_reference.py's start block: unit vectors, probability vectors, a column of mass 2.5"""
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


@pytest.mark.parametrize("name", ["sell_lds", "sell_global", "banded", "masked"])
def test_one_step_matches_the_oracle(golden_dir, name):
    """one Krylov step per column against kfo_expv_fixed, at the 1e-10 beta of tests/test_gpu_block_reference.py"""
    m, tol, t = 30, 1e-10, 2e-4
    with _ctx(block_small=1) as ctx:
        ell, _ = _setup(ctx, golden_dir, name)
        A = O.EllMatrix(*ell)
        n = ctx.n
        rng = np.random.default_rng(6)
        for k in (1, 5, 16):
            W = _start(n, k, rng)
            assert t < BR.first_step(m, tol, np.linalg.norm(W, axis=0).max())
            ctx.set_block(W)
            ws, st = ctx.expv_block(t, tol, m)
            R = ctx.get_block()
            assert ctx.block_info()["one_launch"] == 1
            assert (st.nstep, st.nreject, st.nmult, st.t_now) == (1, 0, m + 1, t), (k, st.nstep, st.nreject)
            for c in range(k):
                w1, ws1 = O.expv_fixed(A, W[:, c], m, t, 1)
                beta = np.linalg.norm(W[:, c])
                assert np.abs(R[:, c] - w1).sum() <= 1e-10 * beta, (k, c)
                assert abs(ws[c] - ws1[0]) <= 1e-12, (k, c)


ADAPTIVE = (0.3, 1e-8, 30, 6)         # "several_steps" of tests/test_gpu_block_reference.py: toggle(60, 50), 3 000 rows


def _adaptive_solve(**opts):
    t, tol, m, k = ADAPTIVE
    mdl = _synth().toggle(60, 50)
    W = _start(mdl.n, k, np.random.default_rng(7))
    with _ctx(**opts) as ctx:
        ctx.set_option("dia_mask", 0)
        ctx.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ctx.set_block(W)
        ws, st = ctx.expv_block(t, tol, m)
        return mdl, W, ctx.get_block(), ws, st, ctx.block_info()


def test_adaptive_solve_matches_the_restatement():
    """counts exact, step sizes to 1e-12, columns to 1e-10 (the assertions of tests/test_gpu_block_reference.py; that the
    case's decisions survive a 1e-3 relative change of every ERR_LOC is checked on the CPU, tests/test_block_small_abi.py)"""
    t, tol, m, k = ADAPTIVE
    mdl, W, R, ws, st, info = _adaptive_solve(block_small=1)
    assert info["one_launch"] == 1 and info["fmt"] == 1
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*mdl.ell()), W, t, tol, m)
    assert stref.nstep >= 2 and stref.nreject >= 1
    assert (st.nstep, st.nreject, st.nmult, st.n_breakdown_cols) == \
        (stref.nstep, stref.nreject, stref.nmult, stref.n_breakdown_cols), (st, stref)
    for f in ("t_now", "step_min", "step_max"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-12, abs=0), f
    for f in ("x_error", "s_error"):
        assert getattr(st, f) == pytest.approx(getattr(stref, f), rel=1e-2, abs=1e-300), f
    for c in range(k):
        assert np.abs(R[:, c] - Rref[:, c]).sum() <= 1e-10, c
        assert abs(ws[c] - wsref[c]) <= 1e-12, c


# ---- 7. the off switch
def test_without_the_option_everything_is_multi_launch(golden_dir):
    """option unset: the multi-launch kernels, with the results they gave before the option existed - the same bits as
    after switching the option on and off again, and the single-vector pass to rounding"""
    m = 30
    with _ctx() as ctx:
        _setup(ctx, golden_dir, "sell_lds")
        n = ctx.n
        rng = np.random.default_rng(8)
        W = _grid_columns(n, rng)[:, :5]
        off = _block_pass(ctx, W, m)
        info = ctx.block_info()
        assert (info["one_launch"], info["fmt"], info["begin_launches"], info["arnoldi_launches"], info["lds_bytes"]) == \
            (0, 0, 2, 4 * m + 3, 0), info
        coef = rng.standard_normal((m + 1, 5)) / 50.0
        ws_off = ctx.block_combine(m + 1, coef)
        assert ctx.block_info()["combine_launches"] == 2
        P = W / W.sum(axis=0)
        ctx.set_block(P)
        ws, st = ctx.expv_block(0.3, 1e-8, m)
        R = ctx.get_block()
        info = ctx.block_info()
        assert (info["one_launch"], info["begin_launches"], info["arnoldi_launches"], info["combine_launches"]) == (0, 2, 4 * m + 3, 2)
        # on, then off again: the resident basis and scalars carry nothing over
        ctx.set_option("block_small", 1)
        on = _block_pass(ctx, W, m)
        assert ctx.block_info()["one_launch"] == 1
        ctx.set_option("block_small", 0)
        again = _block_pass(ctx, W, m)
        assert ctx.block_info()["one_launch"] == 0
        for a, b in zip(off, again):
            assert np.array_equal(_bits(a.astype(np.float64)), _bits(b.astype(np.float64)))
        assert np.array_equal(_bits(ctx.block_combine(m + 1, coef)), _bits(ws_off))
        ctx.set_block(P)
        ws2, st2 = ctx.expv_block(0.3, 1e-8, m)
        assert np.array_equal(_bits(ctx.get_block()), _bits(R)) and np.array_equal(_bits(ws2), _bits(ws))
        assert (st2.nstep, st2.nreject) == (st.nstep, st.nreject)
        # the two paths differ by the order of their sums only: the same breakdowns, and two solves that both meet dense
        # expm within 10 tol in l1 (test_expv_block_matches_dense_exponential, here and in tests/test_gpu_block.py) are
        # within 20 tol of each other
        assert np.array_equal(on[3], off[3])
        ctx.set_option("block_small", 1)
        ctx.set_block(P)
        ctx.expv_block(0.3, 1e-8, m)
        assert ctx.block_info()["one_launch"] == 1
        assert np.abs(ctx.get_block() - R).sum(axis=0).max() <= 20 * 1e-8
