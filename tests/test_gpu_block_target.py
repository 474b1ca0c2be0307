"""Target sets of the block path (option block_target: the call modes of kfsp_set_block / kfsp_block_info /
kfsp_block_begin that install a set, report it and give the flux into it): with a set T resident every block call works on
the killed generator Q = D A D, D = diag(1 - 1_T), through TARGET forms of the three streaming kernels of a pass and no
change to any product kernel.  An empty set changes no bit; kfsp_spmm is the masked product on the bits; a pass equals
the pass on the uploaded killed generator; whole solves meet the CPU restatement on the killed arrays
(tests/block_target_ref.py); the birth chain gives the Erlang first-passage law; the flux call is restated; and the
surface.  Every test fails on the parent commit: the option does not exist.  Needs a real MI355X.

Bounds: tests/block_target_ref.py (hit_bound_J, hit_bound_W) and tests/test_block_target_host.py."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import block_generators as BG
from tests import block_integral_ref as IR
from tests import block_ref as BR
from tests import block_target_ref as TR
from tests.test_block_integral_host import J_REL_BOUND
from tests.test_gpu_block_integral import GENS as IGENS
from tests.test_gpu_block_reference import _assert_solve_matches_ref

pytestmark = pytest.mark.gpu

M_PHASE = 6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


def _set_gen(ctx, golden_dir, name):
    """-> the ELL arrays in the caller's order"""
    if name in BG.GENERATORS:
        return BG.GENERATORS[name](ctx, golden_dir)[1]
    if name == "box_multi":
        ctx.set_option("block_box", 2)
        mdl = _smallest_multi_factor()
        ctx.set_matrix_box(mdl, store=False)
        return mdl.ell()
    return IGENS[name](ctx, golden_dir)


def _smallest_multi_factor():
    from tests import box_cases as BC
    from tests import box_generic_t_ref as GT
    return GT.model(min(BC.generic_names(), key=lambda nm: GT.model(nm).n))


def _prob_block(n, k, seed, keep=None):
    """k columns: unit vectors (c % 3 == 0) and probability vectors, supported on keep where given"""
    rng = np.random.default_rng(seed)
    where = np.arange(n) if keep is None else np.flatnonzero(keep)
    W = np.zeros((n, k))
    for c in range(k):
        if c % 3 == 0:
            W[where[(7919 * c + 3) % len(where)], c] = 1.0
        else:
            p = np.zeros(n)
            p[where] = rng.random(len(where)) ** (c % 5 + 1)
            W[:, c] = p / p.sum()
    return W


# ---- 1. an empty set changes no bit
def _everything(ctx, W0, t):
    out = {}
    ctx.set_option("block_integral", 1)
    ctx.set_block(W0)
    out["beta"] = ctx.block_begin(M_PHASE)
    out["hb"], out["nrm"], out["brk"], out["avn"] = ctx.block_arnoldi(M_PHASE)
    out["info"] = ctx.block_info()
    ctx.set_block(W0)
    ws, st = ctx.expv_block(t, 1e-8, 30)
    out["ws"], out["st"] = ws, bytes(st)
    out["W"], out["J"] = ctx.get_block(), ctx.get_block(integral=True)
    out["nstep"] = st.nstep
    return out


@pytest.mark.parametrize("k", [1, 3, 8, 16])
@pytest.mark.parametrize("gen", ["banded", "sell", "banded_4270_grid8"])
def test_empty_set_changes_no_bit(golden_dir, gen, k):
    res = []
    for with_set in (False, True):
        with _ctx() as ctx:
            ell = _set_gen(ctx, golden_dir, gen)
            n = len(ell[2])
            if with_set:
                ctx.set_block_target(np.zeros(n, dtype=np.uint8))
                assert ctx.block_target_info() == {"resident": 1, "states": 0, "hit_launches": 0}
            res.append(_everything(ctx, _prob_block(n, k, 21), 0.2))
    plain, empty = res
    assert plain["nstep"] >= 2 and plain["info"]["arnoldi_launches"] == 4 * M_PHASE + 3
    for key in plain:
        if isinstance(plain[key], np.ndarray) and plain[key].dtype == np.float64:
            assert np.array_equal(_bits(plain[key]), _bits(empty[key])), (gen, k, key)
        elif isinstance(plain[key], np.ndarray):
            assert np.array_equal(plain[key], empty[key]), (gen, k, key)
        else:
            assert plain[key] == empty[key], (gen, k, key)


# ---- 2. the product
def _sets(n):
    one = np.zeros(n, dtype=np.uint8)
    one[n // 3] = 1
    trips = np.zeros(n, dtype=np.uint8)
    trips[60:71] = 1
    trips[120:136] = 1                   # (empty on a box of fewer than 61 states: then the plain product)
    last = np.zeros(n, dtype=np.uint8)
    last[n - 1] = 1                      # the padding rows behind it must stay "keep"
    return {"single": one, "rows 60..70, 120..135": trips, "state n - 1": last, "random 30 %": TR.random_set(n)}


PRODUCTS = [(g, False) for g in list(BG.GENERATORS) + ["box_21x13", "box_multi"]] + \
           [(g, True) for g in ("banded", "sell", "box_21x13")]


@pytest.mark.parametrize("gen,adjoint", PRODUCTS, ids=[g + ("-adjoint" if a else "") for g, a in PRODUCTS])
def test_product_is_the_masked_product(golden_dir, gen, adjoint):
    with _ctx() as plain, _ctx() as tgt:
        ell = _set_gen(plain, golden_dir, gen)
        _set_gen(tgt, golden_dir, gen)
        n = len(ell[2])
        X = np.random.default_rng(6).standard_normal((n, 16))
        for tag, f in _sets(n).items():
            tgt.set_block_target(f)
            on = f != 0
            for k in (3, 16):
                Y0 = plain.spmm(np.where(on[:, None], 0.0, X[:, :k]), adjoint=adjoint)
                Y = tgt.spmm(X[:, :k], adjoint=adjoint)
                assert np.array_equal(_bits(Y[~on]), _bits(Y0[~on])), (gen, adjoint, tag, k)
                assert np.array_equal(_bits(Y[on]), _bits(np.zeros_like(Y[on]))), (gen, adjoint, tag, k)   # +0.0
        tgt.set_block_target(None)
        assert np.array_equal(_bits(tgt.spmm(X[:, :3], adjoint=adjoint)), _bits(plain.spmm(X[:, :3], adjoint=adjoint)))


# ---- 3. the pass equals a pass on the uploaded killed generator
def _set_killed(ctx, golden_dir, gen, f):
    """generator D A D uploaded in the form of `gen`, entry for entry where A has one (killed entries are stored zeros)"""
    if gen == "sell":
        ell = BG.golden_toggle(golden_dir)
        ctx.set_option("format", 1)
        ctx.set_option("sell_code", 0)
        ctx.set_matrix_ell(*TR.killed_ell((ell["adj"], ell["offdiag"], ell["diag"]), f))
        return
    mdl = _synth().toggle(60, 50)
    rp, col, val = mdl.csr_rows()
    row = np.repeat(np.arange(mdl.n), np.diff(rp))
    on = f != 0
    val = np.where(on[row] | on[col], 0.0, val)
    ctx.set_option("format", 0)
    ctx.set_option("dia_mask", 0)
    ctx.set_matrix_csr(mdl.n, rp, col, val)


def _pass(ctx, W0, coef):
    ctx.set_block(W0)
    out = [("beta", ctx.block_begin(M_PHASE))]
    out += list(zip(("hb", "nrm", "brk", "avnorm"), ctx.block_arnoldi(M_PHASE)))
    out.append(("wsum", ctx.block_combine(M_PHASE + 2, coef)))
    out.append(("W", ctx.get_block()))
    out.append(("launches", np.array([ctx.block_info()["arnoldi_launches"]])))
    return out


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("gen", ["sell", "banded"])
def test_pass_is_the_pass_on_the_killed_generator(golden_dir, gen, k):
    """every operation sees the same operands up to the sign of a zero, so the numbers are EQUAL (+-0.0 compare equal)"""
    with _ctx(block_clamp=0) as a, _ctx(block_clamp=0) as b:
        ell = _set_gen(a, golden_dir, gen)
        n = len(ell[2])
        f = TR.random_set(n)
        a.set_block_target(f)
        _set_killed(b, golden_dir, gen, f)
        assert a.layout_info()["format"] == b.layout_info()["format"]
        W0 = np.random.default_rng(8).standard_normal((n, k))
        coef = np.random.default_rng(9).standard_normal((M_PHASE + 2, k))
        pa = _pass(a, W0, coef)
        pb = _pass(b, np.where((f != 0)[:, None], 0.0, W0), coef)
        for (name, x), (_, y) in zip(pa, pb):
            if not np.array_equal(x, y):
                bad = np.argwhere(x != y)[0]
                print("first difference:", name, "at", tuple(bad), x[tuple(bad)], y[tuple(bad)])
            assert np.array_equal(x, y), (gen, k, name)
        assert dict(pa)["launches"][0] == 4 * M_PHASE + 3
        assert not dict(pa)["W"][f != 0].any() and (dict(pa)["brk"] == 0).all()


# ---- 4. whole solves against the restatement
SOLVE_T = {"banded": 0.6, "sell": 0.3, "state_order": 0.05, "box_21x13": 0.3}


@pytest.mark.parametrize("adjoint", [False, True], ids=["forward", "adjoint"])
@pytest.mark.parametrize("gen", list(SOLVE_T))
def test_whole_solves_against_the_restatement(golden_dir, gen, adjoint):
    t, tol, m, k = SOLVE_T[gen], 1e-8, 30, 3
    with _ctx(block_integral=1) as ctx:
        ell = _set_gen(ctx, golden_dir, gen)
        n = len(ell[2])
        f = TR.random_set(n)
        on = f != 0
        ctx.set_block_target(f)
        W0 = np.random.default_rng(12).standard_normal((n, k)) / n if adjoint else _prob_block(n, k, 12)   # l1 about 0.8
        ctx.set_block(W0)
        ws, st = ctx.expv_block(t, tol, m, adjoint=adjoint, clamp=not adjoint)
        W, J = ctx.get_block(), ctx.get_block(integral=True)
        assert ctx.block_info()["arnoldi_launches"] == 4 * min(m, n - 1) + 3
    kell = TR.killed_ell(ell, f)
    if adjoint:
        kell = BR.transpose_ell(*kell)
    W0k = np.where(on[:, None], 0.0, W0)
    Wr, wsr, str_, Jr = IR.expv_block_integral(O.EllMatrix(*kell), W0k, t, tol, m, clamp=not adjoint)
    assert st.nstep >= 2
    _assert_solve_matches_ref(W, ws, st, Wr, wsr, str_, W0)
    l1 = np.abs(W0k).sum(axis=0)
    d = np.abs(J - Jr).sum(axis=0)
    print(gen, "adjoint" if adjoint else "forward", "steps", st.nstep, "l1(J - J_ref) / bound", (d / (J_REL_BOUND * t * l1)).max())
    assert (d <= J_REL_BOUND * t * l1).all(), d
    assert np.array_equal(_bits(W[on]), _bits(np.zeros_like(W[on])))          # exactly +0.0 on T
    assert np.array_equal(_bits(J[on]), _bits(np.zeros_like(J[on])))
    assert np.abs(J[~on]).sum() > 0.0


# ---- 5. analytic: the birth chain
N, N0, LAM = 45, 12, 3.0


def _set_birth(ctx, form):
    mdl = TR.birth_chain(N, LAM)
    if form == "box":
        ctx.set_option("block_box", 1)
        ctx.set_matrix_box(mdl, store=False)
    else:
        ctx.set_matrix_ell(*mdl.ell())
    return IR.dense_of_ell(mdl.ell())


@pytest.mark.parametrize("form", ["stored", "box"])
def test_birth_chain_first_passage_is_erlang(form):
    t = 2.5
    f = (np.arange(N) >= N0).astype(np.uint8)
    W0 = np.zeros((N, 3))
    W0[0, 0] = W0[5, 1] = W0[20, 2] = 1.0               # the third column is supported inside T
    with _ctx(block_integral=1) as ctx:
        A = _set_birth(ctx, form)
        ctx.set_block_target(f)
        bj, bw = TR.hit_bound_J(A, f, t, 1.0), TR.hit_bound_W(A, f)
        ctx.set_block(W0)
        ws, st = ctx.expv_block(t, 1e-8, 30)
        cdf, pdf = ctx.block_hit(integral=True), ctx.block_hit()
        for c, x0 in enumerate((0, 5)):
            ej = abs(cdf[c] - TR.erlang_cdf(N0 - x0, LAM, t))
            ew = abs(pdf[c] - TR.erlang_pdf(N0 - x0, LAM, t))
            eb = abs(ws[c] + cdf[c] - 1.0)
            print(form, "x0", x0, "cdf err / bound", ej / bj, "pdf err / bound", ew / bw, "balance err / bound", eb / bj)
            assert ej <= bj and ew <= bw and eb <= bj
        assert cdf[2] == 0.0 and pdf[2] == 0.0 and ws[2] == 0.0
        assert not ctx.get_block()[:, 2].any()
        # two successive solves trace the CDF: the same value at 2.5
        ctx.set_block(W0)
        ctx.expv_block(1.0, 1e-8, 30)
        mid = ctx.block_hit(integral=True)
        ctx.expv_block(1.5, 1e-8, 30)
        cdf2 = ctx.block_hit(integral=True)
        for c, x0 in enumerate((0, 5)):
            assert abs(mid[c] - TR.erlang_cdf(N0 - x0, LAM, 1.0)) <= bj
            assert abs(cdf2[c] - TR.erlang_cdf(N0 - x0, LAM, t)) <= bj
        # T = {x >= 1}, start e_0: Q e_0 = -lam e_0, a breakdown after the first column
        ctx.set_block_target((np.arange(N) >= 1).astype(np.uint8))
        ctx.set_block(W0[:, :1])
        ws, st = ctx.expv_block(t, 1e-8, 30)
        hit = ctx.block_hit(integral=True)
        assert st.n_breakdown_cols == 1
        assert abs(ws[0] - math.exp(-LAM * t)) <= 1e-12
        assert abs(hit[0] - (1.0 - ws[0])) <= TR.hit_bound_J(A, np.arange(N) >= 1, t, 1.0)


# ---- 6. the flux call (block_hit) restated
def test_block_hit_is_the_sum_over_the_set_and_touches_nothing(golden_dir):
    k = 5
    with _ctx(block_integral=1) as ctx, _ctx() as plain:
        ell = _set_gen(ctx, golden_dir, "banded")
        _set_gen(plain, golden_dir, "banded")
        n = len(ell[2])
        f = TR.random_set(n)
        on = f != 0
        ctx.set_block_target(f)
        assert ctx.block_target_info() == {"resident": 1, "states": int(on.sum()), "hit_launches": 0}
        W0 = _prob_block(n, k, 14, keep=~on)
        coef = np.random.default_rng(15).standard_normal((M_PHASE + 2, k))
        runs = []
        for with_hit in (False, True):
            ctx.set_block(W0)
            ctx.expv_block(0.05, 1e-8, 30)
            W, J = ctx.get_block(), ctx.get_block(integral=True)
            ctx.block_begin(M_PHASE)
            ctx.block_arnoldi(M_PHASE)
            if with_hit:
                h0, h1 = ctx.block_hit(), ctx.block_hit(integral=True)
                assert np.array_equal(_bits(h0), _bits(ctx.block_hit()))                   # two calls: the same bits
                assert np.array_equal(_bits(h1), _bits(ctx.block_hit(integral=True)))
                assert ctx.block_target_info()["hit_launches"] == 3
                assert np.array_equal(_bits(ctx.get_block()), _bits(W))
                assert np.array_equal(_bits(ctx.get_block(integral=True)), _bits(J))
            ws = ctx.block_combine(M_PHASE + 2, coef, coef_integral=coef[::-1])            # reads every basis column
            runs.append((W, J, ws, ctx.get_block(), ctx.get_block(integral=True)))
        for x, y in zip(*runs):
            assert np.array_equal(_bits(x), _bits(y))
        for X, h in ((runs[1][0], h0), (runs[1][1], h1)):
            Y = plain.spmm(X)
            bound = (on.sum() + 4) * 2.0 ** -53 * np.abs(Y[on]).sum(axis=0)
            err = np.abs(h - Y[on].sum(axis=0))
            print("block_hit err / bound", (err / bound).max(), "values", h)
            assert (err <= bound).all() and (h > 0.0).all()
        # raw: entries >= k are 0
        out = np.full(16, np.nan)
        ctx.set_option("block_target", 3)
        assert ctx._lib.kfsp_block_begin(ctx._h, 0, out.ctypes.data_as(ctypes.c_void_p)) == 0
        ctx.set_option("block_target", 0)
        assert np.array_equal(_bits(out[:k]), _bits(ctx.block_hit())) and not out[k:].any()


# ---- 7. the surface
def test_setting_and_clearing_discards_the_block(golden_dir):
    from krylovfspssa_amd.host import KfspError
    with _ctx(block_integral=1) as ctx:
        ell = _set_gen(ctx, golden_dir, "sell")
        n = len(ell[2])
        f = TR.random_set(n)
        W0 = _prob_block(n, 2, 3)
        for flags in (f, None):
            ctx.set_block(W0)
            ctx.get_block()
            ctx.set_block_target(flags)
            with pytest.raises(KfspError, match="no block resident"):
                ctx.get_block()
            with pytest.raises(KfspError, match="no block resident"):
                ctx.get_block(integral=True)
        # a generator change discards the set
        ctx.set_block_target(f)
        assert ctx.block_target_info()["resident"] == 1
        ctx.update_matrix_ell(*ell, n)
        assert ctx.block_target_info() == {"resident": 0, "states": 0, "hit_launches": 0}
        ctx.set_block_target(f)
        ctx.set_matrix_ell(*ell)
        assert ctx.block_target_info()["resident"] == 0
        ctx.set_block(W0)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W0))            # no set: W as it was handed over


def _raw_set(ctx, n, F, k=1):
    """kfsp_set_block under the call mode 1 -> its return code"""
    ctx.set_option("block_target", 1)
    try:
        return ctx._lib.kfsp_set_block(ctx._h, k, n, max(n, 1), None if F is None else F.ctypes.data_as(ctypes.c_void_p))
    finally:
        ctx.set_option("block_target", 0)


def _raw_hit(ctx, which, out):
    """kfsp_block_begin under the call mode 3 -> its return code"""
    ctx.set_option("block_target", 3)
    try:
        return ctx._lib.kfsp_block_begin(ctx._h, which, None if out is None else out.ctypes.data_as(ctypes.c_void_p))
    finally:
        ctx.set_option("block_target", 0)


def test_return_codes(golden_dir):
    from krylovfspssa_amd import host
    with _ctx() as ctx:
        lib, h = ctx._lib, ctx._h
        flags = np.ones(4096)
        out = np.zeros(16)
        assert _raw_set(ctx, 10, flags) == -1                                            # no matrix set
        assert lib.kfsp_set_block(None, 1, 10, 10, flags.ctypes.data_as(ctypes.c_void_p)) == -1
        ell = _set_gen(ctx, golden_dir, "sell")
        n = len(ell[2])
        assert _raw_set(ctx, n + 1, flags) == -2
        assert _raw_set(ctx, n - 1, flags) == -2
        assert _raw_set(ctx, n, flags, k=2) == -2                                        # the flags are one column
        assert lib.kfsp_set_option(h, b"block_target", 4) == -3
        W0 = _prob_block(n, 2, 3)
        ctx.set_block(W0)
        assert _raw_hit(ctx, 0, out) == -1                                               # no set
        f = TR.random_set(n)
        ctx.set_block_target(f)
        assert _raw_hit(ctx, 0, out) == -1                                               # no block
        ctx.set_block(W0)
        assert _raw_hit(ctx, 0, out) == 0
        assert _raw_hit(ctx, 2, out) == -2
        assert _raw_hit(ctx, 0, None) == -3
        assert _raw_hit(ctx, 1, out) == -1                                               # no J resident
        ctx.set_option("adjoint", 1)
        assert _raw_hit(ctx, 0, out) == -12
        assert b"adjoint" in lib.kfsp_last_error(h)
        ctx.set_option("adjoint", 0)
        # mode 0: the three calls are what they were
        assert np.array_equal(_bits(ctx.get_block()), _bits(np.where((f != 0)[:, None], 0.0, W0)))
        assert ctx.block_begin(M_PHASE).shape == (2,) and ctx.block_info()["begin_launches"] == 2
        # clearing with either convention
        assert _raw_set(ctx, 0, flags) == 0
        assert ctx.block_target_info()["resident"] == 0
        ctx.set_block_target(f)
        assert _raw_set(ctx, n, None) == 0
        assert ctx.block_target_info()["resident"] == 0

    def body(rank_ctx, rank):
        rank_ctx.set_option("block_partition", 1)
        rc = _raw_set(rank_ctx, 16, np.ones(16))
        return rc, rank_ctx._lib.kfsp_last_error(rank_ctx._h)

    for rc, msg in host.run_loopback_ranks(2, body):
        assert rc == -12 and b"block_target = 1" in msg and b"kfsp_set_block" in msg


def test_block_small_is_not_taken_under_a_set(golden_dir):
    res = []
    for small in (0, 1):
        with _ctx(block_small=small, block_integral=1) as ctx:
            ell = _set_gen(ctx, golden_dir, "sell")
            n = len(ell[2])
            W0 = _prob_block(n, 3, 5)
            if small:
                ctx.set_block(W0)
                ctx.expv_block(0.1, 1e-8, 30)
                assert ctx.block_info()["one_launch"] == 1                  # without a set the option is taken here
            ctx.set_block_target(TR.random_set(n))
            ctx.set_block(W0)
            ws, st = ctx.expv_block(0.3, 1e-8, 30)
            assert ctx.block_info()["one_launch"] == 0
            res.append((ws, np.frombuffer(bytes(st), dtype=np.uint8), ctx.get_block(), ctx.get_block(integral=True)))
    for x, y in zip(*res):
        assert np.array_equal(x.view(np.uint8) if x.dtype == np.uint8 else _bits(x), y.view(np.uint8) if y.dtype == np.uint8 else _bits(y))


def test_full_set_leaves_nothing(golden_dir):
    with _ctx(block_integral=1) as ctx:
        ell = _set_gen(ctx, golden_dir, "banded")
        n = len(ell[2])
        ctx.set_block_target(np.ones(n, dtype=np.uint8))
        assert ctx.block_target_info()["states"] == n
        ctx.set_block(_prob_block(n, 3, 5))
        t = 0.2
        ws, st = ctx.expv_block(t, 1e-8, 30)
        assert st.t_now == t and not ws.any()
        assert not ctx.get_block().any() and not ctx.get_block(integral=True).any()
        assert not ctx.block_hit().any() and not ctx.block_hit(integral=True).any()
