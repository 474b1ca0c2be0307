"""Option block_dia_code: the forward block product on the dictionary-coded image of a banded generator (k_spmm_diac,
csrc/kfsp_block_diac.hip; DESIGN.md 12, "Coded banded generators").  The kernel multiplies the very doubles of the plain
value streams with the same rows of X in the same order, so everything it feeds - products, the fused dot products of a
pass, whole solves, time integrals, first-passage fluxes - must be BIT-IDENTICAL to the plain block kernel (option 0) and
to kfsp_spmv, and every case the option does not cover must keep its kernel.  The generators are the smallest that reach
each (bits per code, bytes per record) instantiation.  Needs a real MI355X."""
import ctypes

import numpy as np
import pytest

from tests import row_ref

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8, 16)

# name -> (model, rows, diagonals, bits per code, bytes per record)
GENS = {
    # last 128-row group half empty (8 000 = 62.5 groups)
    "toggle100x80": (lambda s: s.toggle(100, 80), 8000, 4, 8, 8),
    # n mod 128 = 107, n mod 64 = 43
    "repressilator31x23x19": (lambda s: s.repressilator(dims=(31, 23, 19)), 13547, 6, 8, 8),
    # 12 diagonals of one-byte codes: codes 8 - 11 in the second record word
    "birth_death6": (lambda s: s.birth_death((5, 6, 4, 5, 3, 4)), 7200, 12, 8, 16),
    # 271 distinct values on one diagonal: two-byte codes, four of them in one word
    "toggle270x50": (lambda s: s.toggle(270, 50), 13500, 4, 16, 8),
    # 6 diagonals of two-byte codes: codes 4 - 5 in the second word
    "repressilator300x6x5": (lambda s: s.repressilator(dims=(300, 6, 5)), 9000, 6, 16, 16),
}

_MODELS = {}


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _gen(name):
    if name not in _MODELS:
        mdl = GENS[name][0](_synth())
        _MODELS[name] = (mdl, mdl.csr_rows())
    return _MODELS[name]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ctx(dia_code=1, small_kernel=0, dia_mask=0):
    """the contexts of tests/test_gpu_dia_code.py::_ctx"""
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", small_kernel)
    c.set_option("dia_mask", dia_mask)
    c.set_option("dia_code", dia_code)
    return c


def _load(c, name):
    """the generator through set_matrix_csr; its shape, width and record bytes are what the table above says"""
    mdl, csr = _gen(name)
    _, rows, nd, width, rec = GENS[name]
    c.set_matrix_csr(mdl.n, *csr)
    ci = c.dia_code_info()
    assert mdl.n == rows and c.layout_info()["format"] == 1, (name, mdl.n, c.layout_info())
    assert ci["active"] == 1 and ci["diagonals"] == nd and ci["width"] == width and ci["record_bytes"] == rec, (name, ci)
    assert ci["dict_bytes"] == 8 * sum(ci["distinct"]) <= 40 * 1024
    return mdl, ci


def _mixed(n, k, seed=5):
    """magnitudes in [1e-3, 1e3], mixed signs, and (from two columns on) one unit-vector column"""
    rng = np.random.default_rng(seed)
    X = np.where(rng.random((n, k)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 3.0, (n, k))
    if k >= 2:
        X[:, 1] = 0.0
        X[(3 * n) // 7, 1] = 1.0
    return np.asfortranarray(X)


def _start(n, k, seed=9):
    """probability columns of different mass and one unit vector: the betas differ from column to column"""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, k))
    for c in range(k):
        if c == 1:
            W[(5 * n) // 11, c] = 1.0
        else:
            p = rng.random(n) ** (c % 4 + 1)
            W[:, c] = (1.0 + 0.5 * c) * p / p.sum()
    return np.asfortranarray(W)


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} entries differ on the bits, first {bad[:5]}"


def _coded(c, ci=None):
    """the last product ran k_spmm_diac: slot 1 says 9, slot 5 the dynamic LDS of the launch - the dictionaries"""
    info = c.block_info()
    assert info["fmt"] == 9, info
    if ci is not None:
        assert info["lds_bytes"] == ci["dict_bytes"], (info, ci)


def _plain(c):
    info = c.block_info()
    assert info["fmt"] == 0 and info["lds_bytes"] == 0, info


def _pass(c, W, m):
    """block_begin + block_arnoldi(m) from a fresh block -> what a pass hands back"""
    c.set_block(W)
    beta = c.block_begin(m)
    hb, nrm, brk, avn = c.block_arnoldi(m)
    return dict(beta=beta, H=hb, nrm=nrm, brk=brk.astype(np.float64), avnorm=avn)


def _same_pass(a, b, what):
    for key in a:
        _same(a[key], b[key], (what, key))


def _stats(st):
    return {name: getattr(st, name) for name, _ in st._fields_}


# ---- 1. product bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(GENS))
def test_coded_block_product_is_the_plain_one_on_the_bits(name, k):
    mdl, csr = _gen(name)
    X = _mixed(mdl.n, k)
    with _ctx() as c:
        _, ci = _load(c, name)
        c.set_option("block_dia_code", 1)                 # (the parent commit answers -2: unknown option)
        Y1 = c.spmm(X)
        _coded(c, ci)
        c.set_option("block_dia_code", 0)
        Y0 = c.spmm(X)
        cols = np.stack([c.spmv(X[:, j]) for j in range(k)], axis=1)
    assert np.abs(Y1).max() > 0.0
    _same(Y1, Y0, (name, k, "against option 0"))
    _same(Y1, cols, (name, k, "against kfsp_spmv"))
    if k == 3:
        rows, diag = row_ref.rows_from_csr(mdl.n, *csr)
        for j in range(k):
            want = np.array(row_ref.spmv_exact(rows, diag, X[:, j]))
            zero = want == 0.0                            # (the restatement does not carry the sign of a zero result)
            _same(Y1[~zero, j], want[~zero], (name, "restated rows, column", j))
            assert np.all(Y1[zero, j] == 0.0), (name, j)


# ---- 2. trip loop and order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 16))
def test_trip_loop_and_trip_order_from_one_staged_image(k):
    """13 547 rows are 106 trips: on 8 workgroups every wavefront takes three or four of them from the dictionaries its
    workgroup staged once, ascending and then in a random order"""
    name = "repressilator31x23x19"
    mdl, _ = _gen(name)
    X = _mixed(mdl.n, k, seed=6)
    with _ctx() as c:
        _load(c, name)
        want = c.spmm(X)                                  # option 0, default grid, ascending trips
        W = _start(mdl.n, min(k, 5))
        want_pass = _pass(c, W, 4)
    with _ctx() as c:
        _, ci = _load(c, name)
        c.set_option("grid_blocks", 8)
        c.set_option("block_dia_code", 1)
        _same(c.spmm(X), want, "8 workgroups")
        _coded(c, ci)
        trips = (c.layout_info()["chunks"] + 1) // 2
        assert trips == 106
        c.set_trip_order(np.random.default_rng(12).permutation(trips).astype(np.int32))
        _same(c.spmm(X), want, "8 workgroups, permuted trips")
        _coded(c, ci)
        # the DOTS partials of 8 workgroups are other sums than those of the default grid: against option 0 on this grid
        got = _pass(c, W, 4)
        _coded(c)
        c.set_option("block_dia_code", 0)
        plain8 = _pass(c, W, 4)
        _plain(c)
        _same_pass(got, plain8, "pass on 8 workgroups, permuted trips")
        for key in ("beta", "brk"):
            _same(got[key], want_pass[key], key)


# ---- 3. leading dimension -------------------------------------------------------------------------------------------------
def test_leading_dimension_through_the_c_abi():
    name, k = "toggle100x80", 5
    mdl, _ = _gen(name)
    n, ld = mdl.n, mdl.n + 5
    X = _mixed(n, k, seed=7)
    with _ctx() as c:
        _, ci = _load(c, name)
        Y0 = c.spmm(X)
        c.set_option("block_dia_code", 1)
        Xp = np.full((k, ld), np.nan)                     # column j at Xp[j * ld + i]; a NaN in the gap is never read
        Xp[:, :n] = X.T
        Yp = np.full((k, ld), -7.25)                      # the gap of Y keeps its sentinel
        assert c._lib.kfsp_spmm(c._h, k, ld, _p(Xp), _p(Yp)) == 0
        _coded(c, ci)
    _same(Yp[:, :n], Y0.T, "ld = n + 5")
    assert np.all(Yp[:, n:] == -7.25)
    assert np.isnan(Xp[:, n:]).all() and not np.isnan(Yp).any()


# ---- 4. pass and solve ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3, 5, 16))
@pytest.mark.parametrize("name", list(GENS))
def test_arnoldi_pass_is_bit_equal(name, k):
    """m = 12; k = 5 is kp = 8 with three padding columns.  The DOTS instantiations and the rows in [n, rows_act)"""
    mdl, _ = _gen(name)
    W = _start(mdl.n, k)
    with _ctx() as c:
        _load(c, name)
        c.set_option("block_dia_code", 1)
        got = _pass(c, W, 12)
        _coded(c)
        assert c.block_info()["arnoldi_launches"] == 4 * 12 + 3
        c.set_option("block_dia_code", 0)
        want = _pass(c, W, 12)
        _plain(c)
    assert np.all(got["beta"] > 0.0) and np.all(got["avnorm"] > 0.0)
    _same_pass(got, want, (name, k))


def _solve(c, W, opt, integral=False, target=None):
    c.set_option("block_dia_code", opt)
    c.set_option("block_integral", 1 if integral else 0)
    c.set_block_target(target)
    c.set_block(W)
    wsum, st = c.expv_block(0.05, 1e-8, 20)
    out = dict(wsum=wsum, W=c.get_block(), stats=_stats(st), fmt=c.block_info()["fmt"])
    if integral:
        out["J"] = c.get_block(integral=True)
    if target is not None:
        out["hit"] = c.block_hit()
        out["fmt_hit"] = c.block_info()["fmt"]
    return out


@pytest.mark.parametrize("mode", ("plain", "integral", "target"))
def test_solve_is_bit_equal(mode):
    name, k = "toggle100x80", 6
    mdl, _ = _gen(name)
    W = _start(mdl.n, k, seed=13)
    target = None
    if mode == "target":
        target = np.zeros(mdl.n)
        target[np.random.default_rng(3).choice(mdl.n, 50, replace=False)] = 1.0
    with _ctx() as c:
        _load(c, name)
        res = {opt: _solve(c, W, opt, integral=mode == "integral", target=target) for opt in (1, 0)}
    assert res[1]["fmt"] == 9 and res[0]["fmt"] == 0
    assert res[1]["stats"]["nstep"] >= 1 and res[1]["stats"] == res[0]["stats"], res
    for key in ("wsum", "W") + (("J",) if mode == "integral" else ()) + (("hit",) if mode == "target" else ()):
        _same(res[1][key], res[0][key], (mode, key))
    if mode == "integral":
        assert np.abs(res[1]["J"]).max() > 0.0
    if mode == "target":
        assert res[1]["fmt_hit"] == 9 and res[0]["fmt_hit"] == 0
        assert np.all(res[1]["W"][target != 0.0] == 0.0)


# ---- 5. fallbacks keep their kernel and their bits ------------------------------------------------------------------------
def _both(c, n, k=5, m=6, adjoint=False):
    """product and pass under option 1 and 0 on the generator c holds: slot 1 stays 0 under 1, and the bits are equal"""
    X, W = _mixed(n, k, seed=8), _start(n, k)
    res = {}
    for opt in (1, 0):
        c.set_option("block_dia_code", opt)
        Y = c.spmm(X, adjoint=adjoint)
        _plain(c)
        c.set_option("adjoint", 1 if adjoint else 0)
        try:
            p = _pass(c, W, m)
        finally:
            c.set_option("adjoint", 0)
        _plain(c)
        res[opt] = (Y, p, c.block_info())
    _same(res[1][0], res[0][0], "product")
    _same_pass(res[1][1], res[0][1], "pass")
    assert res[1][2] == res[0][2]
    assert np.abs(res[1][0]).max() > 0.0


def test_fallback_adjoint():
    with _ctx() as c:
        mdl, _ = _load(c, "toggle100x80")                 # the coded image is active; A^T does not read it
        _both(c, mdl.n, adjoint=True)
        assert c.block_info()["adjoint"] == 1


def test_fallback_masked():
    mdl = _synth().toggle(1000, 3)                        # the +-1000 diagonals are empty on most groups: masked
    with _ctx(dia_mask=1) as c:
        c.set_matrix_csr(mdl.n, *mdl.csr_rows())
        assert c.layout_info()["format"] == 2 and c.dia_code_info()["active"] == 0
        _both(c, mdl.n)


def test_fallback_dia_code_off():
    mdl, csr = _gen("toggle100x80")
    with _ctx(dia_code=0) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["active"] == 0
        _both(c, mdl.n)


def test_fallback_generator_that_does_not_code():
    mdl = _synth().toggle(120, 120)
    rowptr, col, val = mdl.csr_rows()
    val = np.random.default_rng(11).random(len(val)) + 0.5
    with _ctx() as c:
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        ci = c.dia_code_info()
        assert c.layout_info()["format"] == 1 and ci["active"] == 0 and ci["width"] == 0
        _both(c, mdl.n)


def test_fallback_loopback_rank_under_block_partition():
    from krylovfspssa_amd import host
    mdl, (rp, col, val) = _gen("toggle100x80")
    n = mdl.n
    X, W = _mixed(n, 5, seed=8), _start(n, 5)

    def work(ctx, rank):
        ctx.set_option("block_partition", 1)
        ctx.set_option("small_kernel", 0)
        ctx.set_option("dia_mask", 0)
        ctx.set_option("dia_code", 1)
        r0, nr = ctx.row_block(n)
        ctx.set_matrix_csr(n, rp[r0:r0 + nr + 1] - rp[r0], col[rp[r0]:rp[r0 + nr]], val[rp[r0]:rp[r0 + nr]])
        assert ctx.dia_code_info()["active"] == 0
        out = {}
        for opt in (1, 0):
            ctx.set_option("block_dia_code", opt)
            Y = ctx.spmm(X)
            fmt = ctx.block_info()["fmt"]
            ctx.set_block(W[r0:r0 + nr])
            beta = ctx.block_begin(6)
            hb, nrm, brk, avn = ctx.block_arnoldi(6)
            out[opt] = (Y, beta, hb, nrm, avn, fmt, ctx.block_info()["fmt"])
        return out

    for out in host.run_loopback_ranks(2, work):
        assert out[1][5] == 0 and out[1][6] == 0
        for a, b in zip(out[1][:5], out[0][:5]):
            _same(a, b, "loop-back rank")


def test_fallback_small_pass():
    mdl = _synth().repressilator(dims=(16, 16, 16))       # 4 096 rows: the last size the one-launch pass takes
    with _ctx(small_kernel=1) as c:
        c.set_matrix_csr(mdl.n, *mdl.csr_rows())
        assert c.layout_info()["format"] == 1 and c.dia_code_info()["active"] == 1
        c.set_option("block_small", 1)
        X, W = _mixed(mdl.n, 5, seed=8), _start(mdl.n, 5)
        res = {}
        for opt in (1, 0):
            c.set_option("block_dia_code", opt)
            Y = c.spmm(X)
            if opt:
                _plain(c)                                 # the product of a context on the small path: the plain kernel
            p = _pass(c, W, 6)
            info = c.block_info()
            assert info["one_launch"] == 1 and info["arnoldi_launches"] == 1, info
            res[opt] = (Y, p, info)
        _same(res[1][0], res[0][0], "product")
        _same_pass(res[1][1], res[0][1], "one-launch pass")
        assert res[1][2] == res[0][2]                     # slots 1 and 5 are the small kernel's, as they were
        # ... and without block_small the same context takes the coded kernel
        c.set_option("block_small", 0)
        c.set_option("block_dia_code", 1)
        _same(c.spmm(X), res[0][0], "coded product")
        _coded(c)


# ---- 6. stale image -------------------------------------------------------------------------------------------------------
def test_update_matrix_ell_leaves_no_stale_image():
    mdl = _synth().repressilator(dims=(20, 18, 16))
    adj, off, diag = mdl.ell()
    off2 = np.array(off, copy=True) * (1.0 + np.arange(off.shape[0]) % 7)[:, None]
    diag2 = np.array(diag, copy=True) * 1.25
    X, W = _mixed(mdl.n, 5, seed=4), _start(mdl.n, 5)
    with _ctx() as c:
        c.set_matrix_ell(adj, off, diag)
        c.set_option("block_dia_code", 1)
        assert c.dia_code_info()["active"] == 1
        before = c.dia_code_info()["distinct"]
        c.set_block(W)
        first = c.spmm(X)
        _coded(c)
        c.update_matrix_ell(adj, off2, diag2, 0)
        ci = c.dia_code_info()
        assert ci["active"] == 1 and ci["distinct"] != before
        got_pass = _pass(c, W, 6)                         # a fresh block on the new generator
        _coded(c)
        got = c.spmm(X)
        _coded(c, ci)
    with _ctx(dia_code=0) as c:
        c.set_matrix_ell(adj, off2, diag2)
        want = c.spmm(X)
        want_pass = _pass(c, W, 6)
    _same(got, want, "the new matrix's product")
    _same_pass(got_pass, want_pass, "the new matrix's pass")
    assert not np.array_equal(first, got)


# ---- 7. option off changes nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_it", (False, True))
def test_option_off_leaves_block_info_as_it_was(set_it):
    name, m = "toggle100x80", 5
    mdl, _ = _gen(name)
    with _ctx() as c:
        _load(c, name)
        if set_it:
            c.set_option("block_dia_code", 0)
        c.spmm(_mixed(mdl.n, 3))
        assert c.block_info() == dict(one_launch=0, fmt=0, begin_launches=0, arnoldi_launches=0, combine_launches=0,
                                      lds_bytes=0, adjoint=0, exchange=0)
        _pass(c, _start(mdl.n, 3), m)
        assert c.block_info() == dict(one_launch=0, fmt=0, begin_launches=2, arnoldi_launches=4 * m + 3, combine_launches=0,
                                      lds_bytes=0, adjoint=0, exchange=0)
