"""Time integrals of the block solve (option block_integral): J = int_0^t exp(sA) W ds from the Krylov bases the steps
already hold.  The fused combine (k_bcombine_int, k_bcombine_small_int) is held to its exact restatement on the bits, W and
everything the step control sees are untouched by the option, whole solves meet the CPU restatement
(tests/block_integral_ref.py), the dense integral and the identity A J = W(t) - W_0 at the bounds measured on the CPU
(tests/test_block_integral_host.py), and the option rides along under a row partition.  Needs a real MI355X."""
import ctypes
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import block_integral_ref as IR
from tests import block_ref as BR
from tests.test_block_integral_host import J_REL_BOUND, RESIDUAL_BOUND
from tests.test_gpu_block import _absorbing_chain

pytestmark = pytest.mark.gpu

M_PHASE = 6


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _host():
    from krylovfspssa_amd import host
    return host


def _ctx(**opts):
    from krylovfspssa_amd import KfspContext
    ctx = KfspContext(0)
    for key, v in opts.items():
        ctx.set_option(key, v)
    return ctx


_CACHE = {}


def _toggle(dims):
    if dims not in _CACHE:
        mdl = _synth().toggle(*dims)
        _CACHE[dims] = (mdl, mdl.csr_rows(), mdl.ell())
    return _CACHE[dims]


def _golden(golden_dir):
    return IR.small_cases(golden_dir)["toggle_fsp_231"][0]


# ---- the generators: name -> setter(ctx, golden_dir) -> ELL arrays in the caller's order
def _banded_1320(ctx, golden_dir):
    mdl, csr, ell = _toggle((40, 33))                    # 1 320 rows: a ragged last 128-row group
    ctx.set_option("format", 0)
    ctx.set_option("dia_mask", 0)
    ctx.set_matrix_csr(mdl.n, *csr)
    return ell


def _banded_4270(ctx, golden_dir):
    mdl, csr, ell = _toggle((70, 61))                    # 4 270 rows on 8 workgroups: every grid-stride loop turns
    ctx.set_option("format", 0)
    ctx.set_option("dia_mask", 0)
    ctx.set_option("grid_blocks", 8)
    ctx.set_option("vec_grid_blocks", 8)
    ctx.set_matrix_csr(mdl.n, *csr)
    return ell


def _sell_231(ctx, golden_dir):
    ell = _golden(golden_dir)
    ctx.set_option("format", 1)
    ctx.set_option("sell_code", 0)
    ctx.set_matrix_ell(*ell)
    return ell


def _box_21x13(ctx, golden_dir):
    mdl = _synth().toggle(21, 13)
    ctx.set_option("block_box", 1)
    ctx.set_matrix_box(mdl, store=False)
    return mdl.ell()


def _death_box(ctx, golden_dir):
    mdl = IR.death_chain()
    ctx.set_option("block_box", 1)
    ctx.set_matrix_box(mdl, store=False)
    return mdl.ell()


GENS = {"banded_1320": _banded_1320, "banded_4270_grid8": _banded_4270, "sell_231": _sell_231, "box_21x13": _box_21x13,
        "death_box": _death_box}


def _signed(n, k, seed):
    """k columns of mixed signs and moderate size, one of them (when there are three) all zero"""
    W = np.random.default_rng(seed).standard_normal((n, k))
    if k >= 3:
        W[:, 1] = 0.0
    return W


def _tables(mx, k, seed):
    """coef / coef_integral: magnitudes 1e-3 .. 1e3, mixed signs, one zero row in each"""
    rng = np.random.default_rng(seed)
    def one():
        t = 10.0 ** rng.uniform(-3.0, 3.0, (mx, k)) * rng.choice([-1.0, 1.0], (mx, k))
        t[rng.integers(0, mx)] = 0.0
        return t
    return one(), one()


def _assert_exact(got, want, tag):
    """the bits of the restatement; where it is +-0 (its fma does not carry the sign of a zero) the value"""
    nz = want != 0.0
    assert np.array_equal(_bits(got[nz]), _bits(want[nz])), tag
    assert not got[~nz].any(), tag


def _raw_begin(ctx, m):
    beta = np.zeros(16)
    assert ctx._lib.kfsp_block_begin(ctx._h, m, beta.ctypes.data_as(ctypes.c_void_p)) == 0
    return beta


def _phase(ctx, W0, clamp, seed):
    """the phase-level comparison on this context's rows (W0: its rows).  Option off: every u_i through unit tables
    (W = fma(1, u, 0) = u), then the plain combine of the tables; option on, a fresh block: two fused combines."""
    k, m = W0.shape[1], M_PHASE
    out = {}
    ctx.set_option("block_integral", 0)
    ctx.set_option("block_clamp", 0)
    ctx.set_block(W0)
    ctx.block_begin(m)
    ctx.block_arnoldi(m)
    U = []
    for i in range(m + 2):
        e = np.zeros((m + 2, k))
        e[i] = 1.0
        ctx.block_combine(m + 2, e)
        U.append(ctx.get_block())
    out["U"] = U
    ctx.set_option("block_clamp", clamp)
    (c1, j1), (c2, j2) = _tables(m + 2, k, seed), _tables(m - 1, k, seed + 1)
    out["tables"] = ((c1, j1), (c2, j2))
    out["ws_off"] = [ctx.block_combine(m + 2, c1)]
    out["W_off"] = [ctx.get_block()]
    out["info_off"] = ctx.block_info()
    out["ws_off"].append(ctx.block_combine(m - 1, c2))      # mx < m + 2
    out["W_off"].append(ctx.get_block())
    ctx.set_option("block_integral", 1)
    ctx.set_block(W0)
    ctx.block_begin(m)
    ctx.block_arnoldi(m)
    out["J0"] = ctx.get_block(integral=True)
    out["ws_on"], out["W_on"], out["J"] = [], [], []
    for mx, (cf, cj) in ((m + 2, (c1, j1)), (m - 1, (c2, j2))):
        out["ws_on"].append(ctx.block_combine(mx, cf, coef_integral=cj))
        out["info_on"] = ctx.block_info()
        out["W_on"].append(ctx.get_block())
        out["J"].append(ctx.get_block(integral=True))
    out["pad_beta"] = _raw_begin(ctx, m)[k:]
    ctx.set_option("block_clamp", 1)
    ctx.set_option("block_integral", 0)
    return out


def _assert_phase(out, W0, clamp, tag):
    k = W0.shape[1]
    (c1, j1), (c2, j2) = out["tables"]
    assert np.array_equal(_bits(out["J0"]), _bits(np.zeros_like(W0))), tag          # +0.0 after set_block
    for a, b in zip(out["W_on"] + out["ws_on"], out["W_off"] + out["ws_off"]):
        assert np.array_equal(_bits(a), _bits(b)), tag                              # W and wsum: the option-off bits
    U = out["U"]
    _, J1 = IR.combine_int_exact(U, c1, j1, np.zeros_like(W0), clamp)
    W2, J2 = IR.combine_int_exact(U, c2, j2, J1, clamp)                             # continues the chain from J1
    _assert_exact(out["J"][0], J1, tag)
    _assert_exact(out["J"][1], J2, tag)
    _assert_exact(out["W_on"][1], W2, tag)
    assert out["J"][1].shape == (W0.shape[0], k) and not out["pad_beta"].any(), tag
    if k >= 3:
        assert np.array_equal(_bits(out["J"][1][:, 1]), _bits(np.zeros(W0.shape[0]))), tag   # a zero column: +0.0
    assert (out["J"][1] < 0).any() and (clamp == 0 or (out["W_on"][1] == 0).any()), tag
    assert out["info_on"]["combine_launches"] == out["info_off"]["combine_launches"], tag


# ---- 1. fails without the feature
def test_option_is_accepted():
    """(the parent commit: -2, unknown option)"""
    with _ctx() as ctx:
        ctx.set_option("block_integral", 1)
        ctx.set_option("block_integral", 2)
        ctx.set_option("block_integral", 0)


# ---- 2. the fused combine on the bits
@pytest.mark.parametrize("clamp", [1, 0])
@pytest.mark.parametrize("small", [0, 1])
@pytest.mark.parametrize("gen,k", [("sell_231", 16), ("sell_231", 1), ("banded_1320", 3)])
def test_fused_combine_on_the_bits(golden_dir, gen, k, small, clamp):
    with _ctx(block_small=small) as ctx:
        ell = GENS[gen](ctx, golden_dir)
        W0 = _signed(len(ell[2]), k, 3)
        out = _phase(ctx, W0, clamp, 40 + k)
        assert out["info_on"]["combine_launches"] == (1 if small else 2)
        _assert_phase(out, W0, clamp, (gen, k, small, clamp))


# ---- 3. W is untouched by the option
SOLVES = {"forward clamped": ("banded_1320", {}, dict()),
          "backward unclamped": ("banded_1320", {}, dict(adjoint=True, clamp=False)),
          "small": ("sell_231", {"block_small": 1}, dict()),
          "box": ("box_21x13", {}, dict()),
          "grid8": ("banded_4270_grid8", {}, dict())}


@pytest.mark.parametrize("case", list(SOLVES))
def test_w_is_untouched_by_the_option(golden_dir, case):
    gen, opts, kw = SOLVES[case]
    with _ctx(**opts) as ctx:
        ell = GENS[gen](ctx, golden_dir)
        n = len(ell[2])
        W0 = np.abs(_signed(n, 3, 7)) / n if kw.get("clamp", True) else _signed(n, 3, 7)
        res = []
        for opt in (0, 1, 0):
            ctx.set_option("block_integral", opt)
            ctx.set_block(W0)
            ws, st = ctx.expv_block(0.2, 1e-8, 30, **kw)
            res.append((ctx.get_block(), ws, bytes(st), ctx.block_info()))
            if opt:
                assert np.abs(ctx.get_block(integral=True)).sum() > 0.0
        assert st.nstep >= 2
        for r in res[1:]:
            assert np.array_equal(_bits(r[0]), _bits(res[0][0])) and np.array_equal(_bits(r[1]), _bits(res[0][1])), case
            assert r[2] == res[0][2] and r[3] == res[0][3], case


# ---- 4. whole solves
def _solve(ctx, W0, t, tol, m, transposed):
    ctx.set_option("block_integral", 1)
    ctx.set_block(W0)
    ws, st = ctx.expv_block(t, tol, m, adjoint=transposed, clamp=False)
    return ctx.get_block(), ctx.get_block(integral=True), st


def _reference(ell, W0, t, tol, m, transposed, J=None):
    if transposed:
        ell = BR.transpose_ell(*ell)
    return IR.expv_block_integral(O.EllMatrix(*ell), W0, t, tol, m, clamp=False, J=J)


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("gen,small", [("sell_231", 0), ("sell_231", 1), ("box_21x13", 0)])
def test_whole_solves_on_the_measured_cases(golden_dir, gen, small, transposed):
    """the generators the CPU bounds were measured on: J against the restatement, the dense integral, and A J = W(t) - W0"""
    t = 0.3
    with _ctx(block_small=small) as ctx:
        ell = GENS[gen](ctx, golden_dir)
        n = len(ell[2])
        A = IR.dense_of_ell(ell)
        A = A.T if transposed else A
        W0 = IR.start_block(n, transposed)
        l1 = np.abs(W0).sum(axis=0)
        Jd = IR.dense_integral(A, W0, t)
        for tol, m in ((1e-8, 30), (1e-5, 10)):
            W, J, st = _solve(ctx, W0, t, tol, m, transposed)
            assert ctx.block_info()["one_launch"] == (1 if small and not transposed else 0)
            err = np.abs(J - Jd).sum(axis=0) / (t * l1)
            res = np.abs(ctx.spmm(J, adjoint=transposed) - (W - W0)).sum(axis=0) / l1
            print(gen, small, transposed, tol, m, "steps", st.nstep, "J vs dense", err.max(), "residual", res.max())
            assert (err <= J_REL_BOUND).all() and (res <= RESIDUAL_BOUND).all(), (tol, m, err, res)
            if tol == 1e-8:
                Wr, _, str_, Jr = _reference(ell, W0, t, tol, m, transposed)
                assert (st.nstep, st.nreject) == (str_.nstep, str_.nreject)
                d = np.abs(J - Jr).sum(axis=0)
                print("   J vs restatement", d, "bound", 1e-10 * t * np.maximum(1.0, l1))
                assert (d <= 1e-10 * t * np.maximum(1.0, l1)).all(), d


@pytest.mark.parametrize("gen,k", [("banded_1320", 16), ("banded_4270_grid8", 3)])
def test_whole_solves_against_the_restatement(golden_dir, gen, k):
    t, tol, m = 0.3, 1e-8, 30
    with _ctx() as ctx:
        ell = GENS[gen](ctx, golden_dir)
        n = len(ell[2])
        rng = np.random.default_rng(9)
        W0 = np.zeros((n, k))
        for c in range(k):
            if c % 3 == 0:
                W0[(7919 * c + 3) % n, c] = 1.0
            else:
                p = rng.random(n) ** (c % 5 + 1)
                W0[:, c] = (2.5 if c % 3 == 2 else 1.0) * p / p.sum()
        W, J, st = _solve(ctx, W0, t, tol, m, False)
        Wr, _, str_, Jr = _reference(ell, W0, t, tol, m, False)
        assert (st.nstep, st.nreject) == (str_.nstep, str_.nreject) and st.nstep >= 2
        l1 = np.abs(W0).sum(axis=0)
        d = np.abs(J - Jr).sum(axis=0)
        print(gen, "steps", st.nstep, "J vs restatement", d.max())
        assert (d <= 1e-10 * t * np.maximum(1.0, l1)).all(), d
        assert (np.abs(W - Wr).sum(axis=0) <= 1e-10 * np.maximum(1.0, l1)).all()
        # J is an occupation measure: nonnegative to rounding, and its mass is at most t per unit of start mass
        assert J.min() >= -1e-14 and (J.sum(axis=0) <= t * l1 * (1 + 1e-12)).all()


# ---- 5. what it is for
def test_accumulated_observable_of_the_death_chain(golden_dir):
    """backward on pure death a(x) = x / 2: f(x) = x is an exact eigenvector, A^T f = -f / 2, so J = 2 (1 - exp(-t / 2)) f;
    the column of zeros beside it keeps J = +0.0; g = 1 never exits this box: J = t"""
    t = 0.7
    with _ctx() as ctx:
        ell = _death_box(ctx, golden_dir)
        n = len(ell[2])
        F = np.zeros((n, 3))
        F[:, 0] = np.arange(n)
        F[:, 2] = 1.0
        W, J, st = _solve(ctx, F, t, 1e-8, 30, True)
        want = 2.0 * (1.0 - math.exp(-t / 2.0)) * F[:, 0]
        print("death chain: l1 error", np.abs(J[:, 0] - want).sum(), "bound", J_REL_BOUND * t * F[:, 0].sum())
        assert np.abs(J[:, 0] - want).sum() <= J_REL_BOUND * t * F[:, 0].sum()
        assert np.array_equal(_bits(J[:, 1]), _bits(np.zeros(n)))
        assert np.abs(J[:, 2] - t).sum() <= J_REL_BOUND * t * n


def test_absorbing_start_state_accumulates_t():
    """A e_0 = 0: a null H, g = tau e_1, and J = t W0 to one ulp per step taken"""
    t = 0.5
    with _ctx(block_small=1) as ctx:
        N, rp, col, val = _absorbing_chain()
        ctx.set_matrix_csr(N, rp, col, val)
        W0 = np.zeros((N, 3))
        W0[0, 0] = 1.0
        W0[150, 2] = 1.0
        W, J, st = _solve(ctx, W0, t, 1e-8, 30, False)
        assert st.nstep >= 2 and st.n_breakdown_cols >= 1
        assert not J[1:, 0].any() and abs(J[0, 0] - t) <= st.nstep * np.spacing(t), (J[0, 0], st.nstep)
        assert np.array_equal(_bits(J[:, 1]), _bits(np.zeros(N)))
        assert J[:, 2].sum() == pytest.approx(t, rel=1e-7)


# ---- 6. accumulation
def test_two_calls_accumulate_and_set_block_zeroes(golden_dir):
    t1, t2, tol, m = 0.1, 0.2, 1e-8, 30
    with _ctx() as ctx:
        ell = _box_21x13(ctx, golden_dir)
        n = len(ell[2])
        W0 = IR.start_block(n, False)
        ctx.set_option("block_integral", 1)
        ctx.set_block(W0)
        ctx.expv_block(t1, tol, m, clamp=False)
        J1 = ctx.get_block(integral=True)
        ctx.expv_block(t2, tol, m, clamp=False)
        J2 = ctx.get_block(integral=True)
        W1r, _, _, J1r = _reference(ell, W0, t1, tol, m, False)
        _, _, _, J2r = _reference(ell, W1r, t2, tol, m, False, J=J1r)
        l1 = np.maximum(1.0, np.abs(W0).sum(axis=0))
        assert (np.abs(J1 - J1r).sum(axis=0) <= 1e-10 * t1 * l1).all()
        assert (np.abs(J2 - J2r).sum(axis=0) <= 1e-10 * (t1 + t2) * l1).all()
        Jd = IR.dense_integral(IR.dense_of_ell(ell), W0, t1 + t2)
        assert (np.abs(J2 - Jd).sum(axis=0) <= J_REL_BOUND * (t1 + t2) * np.abs(W0).sum(axis=0)).all()
        ctx.set_block(W0)
        assert np.array_equal(_bits(ctx.get_block(integral=True)), _bits(np.zeros_like(W0)))


# ---- 7. row partitions
def _rows(csr, r0, nr):
    rp, col, val = csr
    return rp[r0:r0 + nr + 1] - rp[r0], col[rp[r0]:rp[r0 + nr]], val[rp[r0]:rp[r0 + nr]]


def _partition_setter(kind, golden_dir):
    """-> setter(ctx) for a rank, a head or one context, after block_partition = 1"""
    if kind == "banded_1320":
        mdl, csr, _ = _toggle((40, 33))

        def f(ctx):
            ctx.set_option("format", 0)
            r0, nr = ctx.row_block(mdl.n)
            ctx.set_matrix_csr(mdl.n, *_rows(csr, r0, nr))
            return mdl.n
        return f
    g = np.load(golden_dir + "/assembly_toggle_k20.npz")

    def f(ctx):                                           # SELL under the global internal state order
        for key, v in (("format", 1), ("sell_code", 0), ("state_order", 1), ("state_order_min", 1), ("state_order_products", 0)):
            ctx.set_option(key, v)
        ctx.set_state_coords(g["state"])
        ctx.set_matrix_ell(g["adj"], g["offdiag"], g["diag"])
        assert ctx.state_order_active()
        return len(g["diag"])
    return f


@pytest.mark.parametrize("kind", ["banded_1320", "sell_231_state_order"])
def test_fused_combine_on_two_ranks(golden_dir, kind):
    setter = _partition_setter(kind, golden_dir)
    clamp, k = 1, 3
    box = {}

    def work(ctx, rank):
        ctx.set_option("block_partition", 1)
        n = setter(ctx)
        W0 = _signed(n, k, 13)
        box["W0"] = W0
        r0, nr = ctx.row0, ctx.nloc
        out = _phase(ctx, W0[r0:r0 + nr], clamp, 60)
        out["r0"], out["nr"] = r0, nr
        return out

    res = _host().run_loopback_ranks(2, work)
    W0 = box["W0"]
    assert sum(r["nr"] for r in res) == W0.shape[0] and all(r["nr"] > 0 for r in res)
    for r in res:
        _assert_phase(r, W0[r["r0"]:r["r0"] + r["nr"]], clamp, (kind, r["r0"]))
        assert r["info_on"]["exchange"] == r["info_off"]["exchange"] and r["info_on"]["exchange"] in (1, 2)
        assert r["info_on"] == r["info_off"]
    assert np.array_equal(_bits(res[0]["ws_on"][1]), _bits(res[1]["ws_on"][1]))
    # the rows come back in the caller's order: the ranks' J, stacked, is the restatement on the stacked basis
    U = [np.concatenate([r["U"][i] for r in res], axis=0) for i in range(M_PHASE + 2)]
    (c1, j1), (c2, j2) = res[0]["tables"]
    _, J1 = IR.combine_int_exact(U, c1, j1, np.zeros_like(W0), clamp)
    _assert_exact(np.concatenate([r["J"][0] for r in res], axis=0), J1, kind)


def test_group_head_solve_matches_one_context():
    from krylovfspssa_amd import KfspContext
    mdl, csr, ell = _toggle((40, 33))
    t, tol, m = 0.3, 1e-8, 30
    W0 = np.abs(_signed(mdl.n, 3, 17)) / mdl.n
    out = []
    for group in (None, 2):
        with KfspContext(0, group=group) as ctx:
            ctx.set_option("block_partition", 1)
            ctx.set_option("format", 0)
            ctx.set_matrix_csr(mdl.n, *csr)
            infos = []
            for opt in (0, 1):
                ctx.set_option("block_integral", opt)
                ctx.set_block(W0)
                ws, st = ctx.expv_block(t, tol, m)
                infos.append((ctx.block_info(), ctx.get_block(), ws, bytes(st)))
            assert infos[0][0] == infos[1][0]             # launches and the exchange: unchanged by the option
            assert np.array_equal(_bits(infos[0][1]), _bits(infos[1][1])) and infos[0][3] == infos[1][3]
            assert np.array_equal(_bits(infos[0][2]), _bits(infos[1][2]))
            out.append((ctx.get_block(integral=True), infos[1][0], st.nstep))
    (J1, info1, n1), (J2, info2, n2) = out
    assert n1 == n2 >= 2 and info1["exchange"] == 0 and info2["exchange"] in (1, 2)
    l1 = np.abs(W0).sum(axis=0)
    print("head vs one context", np.abs(J2 - J1).sum(axis=0))
    assert (np.abs(J2 - J1).sum(axis=0) <= 1e-10 * t * np.maximum(1.0, l1)).all()
    assert np.abs(J1).sum() > 0


# ---- 8. lifecycle and refusals
def test_lifecycle_and_refusals(golden_dir):
    from krylovfspssa_amd.host import KfspError
    with _ctx() as ctx:
        ell = _banded_1320(ctx, golden_dir)
        n = len(ell[2])
        p0 = np.abs(_signed(n, 1, 21))[:, 0]
        ctx.set_vector(p0 / p0.sum())
        w = ctx.get_vector()
        W0 = np.abs(_signed(n, 3, 23)) / n
        with pytest.raises(KfspError, match="-3"):
            ctx.set_option("block_integral", 3)
        with pytest.raises(KfspError, match="-3"):
            ctx.set_option("block_integral", -1)
        ctx.set_block(W0)                                  # the option is off: no J beside this block
        ctx.set_option("block_integral", 1)
        with pytest.raises(KfspError, match=r"-1.*block_integral.*kfsp_set_block"):
            ctx.expv_block(0.05, 1e-8, 30)
        ctx.block_begin(6)
        ctx.block_arnoldi(6)
        with pytest.raises(KfspError, match=r"-1.*block_integral.*kfsp_set_block"):
            ctx.block_combine(3, np.ones((3, 3)), coef_integral=np.ones((3, 3)))
        with pytest.raises(KfspError, match=r"-1.*block_integral.*kfsp_set_block"):
            ctx.get_block(integral=True)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W0))       # W is still there and untouched
        ctx.set_block(W0)                                  # now with the option on
        ctx.expv_block(0.05, 1e-8, 30)
        assert np.abs(ctx.get_block(integral=True)).sum() > 0.0
        assert np.array_equal(_bits(ctx.get_vector()), _bits(w))       # w: never touched
        _banded_1320(ctx, golden_dir)                      # a generator change discards the block and J
        with pytest.raises(KfspError, match="-1"):
            ctx.get_block(integral=True)
        with pytest.raises(KfspError, match="-1"):
            ctx.get_block()
        ctx.set_option("block_integral", 0)
        ctx.set_block(W0)                                  # option off again: no J is kept
        ctx.set_option("block_integral", 2)
        with pytest.raises(KfspError, match=r"-1.*block_integral"):
            ctx.get_block()
        ctx.set_option("block_integral", 0)
        assert np.array_equal(_bits(ctx.get_block()), _bits(W0))
