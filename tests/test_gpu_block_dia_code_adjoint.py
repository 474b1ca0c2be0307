"""Option block_dia_code_adjoint: the TRANSPOSED block product on the dictionary-coded image of a banded generator
(k_spmm_diac_t, csrc/kfsp_block_diac_t.hip; DESIGN.md 12, "Coded banded generators, backward").  The kernel multiplies the
very doubles k_spmm_t reads from the plain value streams with the same rows of X in the same order, so everything it feeds
- products, the fused dot products of a backward pass, whole backward solves, time integrals, target sets - must be
BIT-IDENTICAL to the plain transposed kernel (the option at 0), and every case the option does not cover must keep its
kernel.  "Coded" below: dia_code = 1, block_dia_code = 1, block_dia_code_adjoint = 1, adjoint = 1; "plain": the same context
with block_dia_code_adjoint = 0.  The generators are those of tests/test_gpu_block_dia_code.py, one per (bits per code,
bytes per record) form.  Needs a real MI355X."""
import numpy as np
import pytest

from tests import adjoint_cases as AC
from tests import test_gpu_block_dia_code as F

pytestmark = pytest.mark.gpu

OPT = "block_dia_code_adjoint"


def _set(c, coded):
    c.set_option("block_dia_code", 1)
    c.set_option(OPT, 1 if coded else 0)                  # (the parent commit answers -2: unknown option)


def _coded_t(c, ci=None):
    """the last product ran k_spmm_diac_t: format 9 with the adjoint flag, the dynamic LDS of the launch = the dictionaries"""
    info = c.block_info()
    assert info["fmt"] == 9 and info["adjoint"] == 1, info
    if ci is not None:
        assert info["lds_bytes"] == ci["dict_bytes"], (info, ci)


def _plain_t(c):
    info = c.block_info()
    assert info["fmt"] == 0 and info["lds_bytes"] == 0 and info["adjoint"] == 1, info


def _pass_t(c, W, m):
    c.set_option("adjoint", 1)
    try:
        return F._pass(c, W, m)
    finally:
        c.set_option("adjoint", 0)


# ---- 1. product bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", F.KS)
@pytest.mark.parametrize("name", list(F.GENS))
def test_coded_transposed_product_is_the_plain_one_on_the_bits(name, k):
    mdl, _ = F._gen(name)
    X = F._mixed(mdl.n, k)
    with F._ctx() as c:
        _, ci = F._load(c, name)
        _set(c, True)
        Y1 = c.spmm(X, adjoint=True)
        _coded_t(c, ci)
        _set(c, False)
        Y0 = c.spmm(X, adjoint=True)
        _plain_t(c)
    assert np.abs(Y1).max() > 0.0
    F._same(Y1, Y0, (name, k, "against the option at 0"))


# ---- 2. restated rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("banded_40x33", "banded_70x61"))
def test_restated_rows(name):
    """sources r - delta < 0 and >= n in the first and the last group; a ragged last group of 40 rows (banded_40x33)"""
    case = AC.case(name)
    mdl = AC.model(name)
    with F._ctx() as c:
        c.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ci = c.dia_code_info()
        assert c.layout_info()["format"] == 1 and ci["active"] == 1, ci
        _set(c, True)
        Y = c.spmm(case["X"], adjoint=True)
        _coded_t(c, ci)
    bad = AC.mismatches(Y, case["Y"])
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5])


# ---- 3. folded records --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("repressilator31x23x19", "toggle100x80"))
def test_folded_records(name):
    """dia_code_diag = 1: bits 48 - 63 of every record hold the row's DIAG digits; the codes below them are what they were
    and DIAG comes from its stream"""
    mdl, csr = F._gen(name)
    X = F._mixed(mdl.n, 5, seed=15)
    with F._ctx() as c:
        c.set_option("dia_code_diag", 1)
        _, ci = F._load(c, name)
        assert ci["diag_table_bytes"] > 0 and ci["record_bytes"] == 8, ci
        _set(c, True)
        Y1 = c.spmm(X, adjoint=True)
        _coded_t(c, ci)
        _set(c, False)
        Y0 = c.spmm(X, adjoint=True)
        _plain_t(c)
    with F._ctx(dia_code=0) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["active"] == 0
        Yn = c.spmm(X, adjoint=True)
    assert np.abs(Y1).max() > 0.0
    F._same(Y1, Y0, (name, "folded, against the option at 0"))
    F._same(Y1, Yn, (name, "folded, against dia_code = 0"))


# ---- 4. trip loop and order -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 16))
def test_trip_loop_and_trip_order_from_one_staged_image(k):
    """13 547 rows are 106 trips: on 8 workgroups every wavefront takes three or four of them from the dictionaries its
    workgroup staged once, ascending and then in a random order"""
    name = "repressilator31x23x19"
    mdl, _ = F._gen(name)
    X = F._mixed(mdl.n, k, seed=6)
    W = F._start(mdl.n, min(k, 5))
    with F._ctx() as c:
        F._load(c, name)
        want = c.spmm(X, adjoint=True)                    # the plain kernel, default grid, ascending trips
    with F._ctx() as c:
        _, ci = F._load(c, name)
        c.set_option("grid_blocks", 8)
        _set(c, True)
        F._same(c.spmm(X, adjoint=True), want, "8 workgroups")
        _coded_t(c, ci)
        trips = (c.layout_info()["chunks"] + 1) // 2
        assert trips == 106
        c.set_trip_order(np.random.default_rng(12).permutation(trips).astype(np.int32))
        F._same(c.spmm(X, adjoint=True), want, "8 workgroups, permuted trips")
        _coded_t(c, ci)
        # the DOTS partials of 8 workgroups are other sums than those of the default grid: against the plain kernel on this grid
        got = _pass_t(c, W, 4)
        _coded_t(c)
        _set(c, False)
        plain8 = _pass_t(c, W, 4)
        _plain_t(c)
        F._same_pass(got, plain8, "pass on 8 workgroups, permuted trips")


# ---- 5. leading dimension -------------------------------------------------------------------------------------------------
def test_leading_dimension_through_the_c_abi():
    name, k = "toggle100x80", 5
    mdl, _ = F._gen(name)
    n, ld = mdl.n, mdl.n + 5
    X = F._mixed(n, k, seed=7)
    with F._ctx() as c:
        _, ci = F._load(c, name)
        Y0 = c.spmm(X, adjoint=True)
        _set(c, True)
        Xp = np.full((k, ld), np.nan)                     # column j at Xp[j * ld + i]; a NaN in the gap is never read
        Xp[:, :n] = X.T
        Yp = np.full((k, ld), -7.25)                      # the gap of Y keeps its sentinel
        c.set_option("adjoint", 1)
        try:
            assert c._lib.kfsp_spmm(c._h, k, ld, F._p(Xp), F._p(Yp)) == 0
        finally:
            c.set_option("adjoint", 0)
        _coded_t(c, ci)
    F._same(Yp[:, :n], Y0.T, "ld = n + 5")
    assert np.all(Yp[:, n:] == -7.25)
    assert np.isnan(Xp[:, n:]).all() and not np.isnan(Yp).any()


# ---- 6. pass --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (2, 3, 5, 16))
@pytest.mark.parametrize("name", list(F.GENS))
def test_backward_arnoldi_pass_is_bit_equal(name, k):
    """m = 12; k = 5 is kp = 8 with three padding columns.  The DOTS instantiations and the rows in [n, rows_act)"""
    mdl, _ = F._gen(name)
    W = F._start(mdl.n, k)
    with F._ctx() as c:
        F._load(c, name)
        _set(c, True)
        got = _pass_t(c, W, 12)
        _coded_t(c)
        assert c.block_info()["arnoldi_launches"] == 4 * 12 + 3
        _set(c, False)
        want = _pass_t(c, W, 12)
        _plain_t(c)
        assert c.block_info()["arnoldi_launches"] == 4 * 12 + 3
    assert np.all(got["beta"] > 0.0) and np.all(got["avnorm"] > 0.0)
    F._same_pass(got, want, (name, k))


# ---- 7. solves ------------------------------------------------------------------------------------------------------------
def _solve(c, W, coded, integral=False, target=None):
    _set(c, coded)
    c.set_option("block_integral", 1 if integral else 0)
    c.set_block_target(target)
    c.set_block(W)
    wsum, st = c.expv_block(0.05, 1e-8, 20, adjoint=True, clamp=False)
    info = c.block_info()
    out = dict(wsum=wsum, W=c.get_block(), stats=F._stats(st), fmt=info["fmt"], adjoint=info["adjoint"])
    if integral:
        out["J"] = c.get_block(integral=True)
    return out


@pytest.mark.parametrize("mode", ("plain", "integral", "target"))
def test_backward_solve_is_bit_equal(mode):
    name, k = "toggle100x80", 6
    mdl, _ = F._gen(name)
    W = F._start(mdl.n, k, seed=13)
    target = None
    if mode == "target":
        target = np.zeros(mdl.n)
        target[np.random.default_rng(3).choice(mdl.n, 50, replace=False)] = 1.0
    with F._ctx() as c:
        F._load(c, name)
        res = {coded: _solve(c, W, coded, integral=mode == "integral", target=target) for coded in (True, False)}
    assert res[True]["fmt"] == 9 and res[False]["fmt"] == 0 and res[True]["adjoint"] == res[False]["adjoint"] == 1
    assert res[True]["stats"]["nstep"] >= 1 and res[True]["stats"] == res[False]["stats"], res
    for key in ("wsum", "W") + (("J",) if mode == "integral" else ()):
        F._same(res[True][key], res[False][key], (mode, key))
    assert np.abs(res[True]["W"]).max() > 0.0
    if mode == "integral":
        assert np.abs(res[True]["J"]).max() > 0.0
    if mode == "target":
        assert np.all(res[True]["W"][target != 0.0] == 0.0)


# ---- 8. fallbacks keep their kernel and their bits ------------------------------------------------------------------------
def _both_t(c, n, block_dia_code, k=5, m=6):
    """transposed product and backward pass with the new option at 1 and at 0 on the generator c holds: the plain kernel
    either way, and the same bits"""
    X, W = F._mixed(n, k, seed=8), F._start(n, k)
    res = {}
    for opt in (1, 0):
        c.set_option("block_dia_code", block_dia_code)
        c.set_option(OPT, opt)
        Y = c.spmm(X, adjoint=True)
        _plain_t(c)
        p = _pass_t(c, W, m)
        _plain_t(c)
        res[opt] = (Y, p, c.block_info())
    F._same(res[1][0], res[0][0], "product")
    F._same_pass(res[1][1], res[0][1], "pass")
    assert res[1][2] == res[0][2]
    assert np.abs(res[1][0]).max() > 0.0


def test_fallback_block_dia_code_off():
    with F._ctx() as c:
        mdl, _ = F._load(c, "toggle100x80")               # the coded image is active, but the forward option is not on
        _both_t(c, mdl.n, block_dia_code=0)


def test_fallback_masked():
    mdl = F._synth().toggle(1000, 3)                      # the +-1000 diagonals are empty on most groups: masked
    with F._ctx(dia_mask=1) as c:
        c.set_matrix_csr(mdl.n, *mdl.csr_rows())
        assert c.layout_info()["format"] == 2 and c.dia_code_info()["active"] == 0
        _both_t(c, mdl.n, block_dia_code=1)


def test_fallback_dia_code_off():
    mdl, csr = F._gen("toggle100x80")
    with F._ctx(dia_code=0) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["active"] == 0
        _both_t(c, mdl.n, block_dia_code=1)


def test_forward_call_keeps_the_forward_coded_kernel():
    name, k = "toggle100x80", 5
    mdl, _ = F._gen(name)
    X = F._mixed(mdl.n, k, seed=8)
    with F._ctx() as c:
        _, ci = F._load(c, name)
        want = c.spmm(X)                                  # every option at 0
        _set(c, True)
        got = c.spmm(X)
        info = c.block_info()
        assert info["fmt"] == 9 and info["adjoint"] == 0 and info["lds_bytes"] == ci["dict_bytes"], info
    F._same(got, want, "forward, both options on")


# ---- 9. one context, alternating ------------------------------------------------------------------------------------------
def test_one_context_alternating():
    """forward coded, backward coded, backward plain, forward plain, twice round, at kp = 4 and then at kp = 16: the occupancy
    cache and the staged LDS are kept per family and per width"""
    name = "repressilator31x23x19"
    mdl, _ = F._gen(name)
    with F._ctx() as c:
        _, ci = F._load(c, name)
        for k in (3, 16):
            X = F._mixed(mdl.n, k, seed=21)
            first = {}
            for rnd in range(2):
                for what in ("forward coded", "backward coded", "backward plain", "forward plain"):
                    backward, coded = what.startswith("backward"), what.endswith("coded")
                    c.set_option("block_dia_code", 1 if (backward or coded) else 0)
                    c.set_option(OPT, 1 if coded else 0)
                    Y = c.spmm(X, adjoint=backward)
                    info = c.block_info()
                    assert info["adjoint"] == (1 if backward else 0), (what, info)
                    assert info["fmt"] == (9 if coded else 0), (what, info)
                    assert info["lds_bytes"] == (ci["dict_bytes"] if coded else 0), (what, info)
                    if rnd == 0:
                        first[what] = Y
                    else:
                        F._same(Y, first[what], (k, what, "second round"))
            F._same(first["backward coded"], first["backward plain"], (k, "backward"))
            F._same(first["forward coded"], first["forward plain"], (k, "forward"))
            assert not np.array_equal(first["backward coded"], first["forward coded"])
