"""DIAG of a coded banded generator folded into the spare bits of its 8-byte records (option dia_code_diag):
the product kernel rebuilds the stored DIAG - pattern of the predictor plus the record's 16-bit residual - instead of
loading it, and everything behind `dg` is the plain kernel's code.  So every product, fused dot product and whole time step
must be BIT-IDENTICAL to the plain banded kernel (dia_code = 0), where the fold is taken and where it is refused."""
import numpy as np
import pytest

from tests.test_gpu_dia_code import _bits, _everything, _same_bits

pytestmark = pytest.mark.gpu


def _ctx(dia_code, fold, nt=None, **opts):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", 0)      # the one-launch Arnoldi kernel of tiny FSPs has its own product
    c.set_option("dia_mask", 0)          # only the unmasked form has a coded kernel
    c.set_option("dia_code", dia_code)
    if fold is not None:
        c.set_option("dia_code_diag", fold)
    if nt is not None:
        c.set_option("nt_loads", nt)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _off_axis_row(mdl):
    """a row none of the DIAG tables is made from: no digit of it is 0"""
    stride = np.concatenate(([1], np.cumprod(mdl.dims[:-1]))).astype(np.int64)
    return int(sum(int(s) * (2 + i) for i, s in enumerate(stride)))


def _scaled_ell(mdl):
    adj, off, diag = mdl.ell()
    diag = np.array(diag, dtype=np.float64, copy=True)
    diag[_off_axis_row(mdl)] *= 1.25
    return adj, off, diag


# (name, model, how it is uploaded, folds)
CASES = [
    ("repressilator 16^3", lambda s: s.repressilator(dims=(16, 16, 16)), "csr", True),
    ("repressilator 31 x 23 x 19: partial last group, padding rows", lambda s: s.repressilator(dims=(31, 23, 19)), "csr", True),
    ("toggle 100 x 80: two digits", lambda s: s.toggle(100, 80), "csr", True),
    ("toggle 300 x 20: W = 16 with 4 diagonals, no spare bits", lambda s: s.toggle(300, 20), "csr", False),
    ("6 species: 16-byte records", lambda s: s.birth_death((5, 6, 4, 5, 3, 4)), "csr", False),
    ("repressilator 20 x 18 x 16, one DIAG entry x 1.25", lambda s: s.repressilator(dims=(20, 18, 16)), "ell 1.25", False),
]

_MODELS = {}


def _model(case):
    if case not in _MODELS:
        mdl = CASES[case][1](_synth())
        how = CASES[case][2]
        _MODELS[case] = (mdl, mdl.csr_rows() if how == "csr" else _scaled_ell(mdl))
    return _MODELS[case]


def _upload(c, case):
    mdl, arrays = _model(case)
    if CASES[case][2] == "csr":
        c.set_matrix_csr(mdl.n, *arrays)
    else:
        c.set_matrix_ell(*arrays)
    return mdl


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_folded_diag_gives_the_bits_of_the_plain_banded_kernel(case, nt):
    name, _, _, folds = CASES[case]
    res, nbytes, info = {}, {}, {}
    for key in ((0, 0), (1, 0), (1, 1)):
        with _ctx(key[0], key[1], nt) as c:
            mdl = _upload(c, case)
            assert c.layout_info()["format"] == 1, name                # kfsp_layout_info keeps calling it banded
            info[key], nbytes[key] = c.dia_code_info(), c.matrix_bytes()
            rows = c.layout_info()["chunks"] * 64
            res[key] = _everything(c, mdl.n)
    if case == 1:
        assert mdl.n % 128 != 0
    assert info[(0, 0)]["active"] == 0 and info[(0, 0)]["diag_table_bytes"] == 0, name
    assert info[(1, 0)]["active"] == 1 and info[(1, 0)]["diag_table_bytes"] == 0, name
    ci = info[(1, 1)]
    assert ci["active"] == 1, name
    for key in ("width", "record_bytes", "coded_bytes", "dict_bytes", "distinct"):
        assert ci[key] == info[(1, 0)][key], (name, key)               # the fold leaves the coded image what it was
    assert nbytes[(1, 0)] == rows * (24 + ci["record_bytes"]) + ci["dict_bytes"], name
    if folds:
        dims = [int(d) for d in mdl.dims]
        assert ci["diag_table_bytes"] == 8 * sum(dims) > 0, (name, ci)
        assert ci["record_bytes"] == 8 and nbytes[(1, 1)] == rows * 24 + ci["dict_bytes"] + ci["diag_table_bytes"], name
    else:
        assert ci["diag_table_bytes"] == 0 and nbytes[(1, 1)] == nbytes[(1, 0)], (name, ci)
    _same_bits(res[(1, 0)], res[(0, 0)], (name, "coded"))
    _same_bits(res[(1, 1)], res[(0, 0)], (name, "coded, DIAG folded"))
    assert np.abs(res[(1, 1)]["spmv"]).max() > 0.0


def test_one_ulp_off_the_predictor_still_folds():
    mdl = _synth().repressilator(dims=(20, 18, 16))
    adj, off, diag = mdl.ell()
    diag = np.array(diag, dtype=np.float64, copy=True)
    row = _off_axis_row(mdl)
    diag[row] = np.nextafter(diag[row], np.inf)
    x = np.random.default_rng(5).standard_normal(mdl.n)
    ys = {}
    for key in ((0, 0), (1, 1)):
        with _ctx(*key) as c:
            c.set_matrix_ell(adj, off, diag)
            if key[1]:
                assert c.dia_code_info()["diag_table_bytes"] == 8 * (20 + 18 + 16)
            ys[key] = c.spmv(x)
    assert np.array_equal(_bits(ys[(1, 1)]), _bits(ys[(0, 0)]))
    with _ctx(0, 0) as c:                                              # ... and the moved entry is in the product
        c.set_matrix_ell(*mdl.ell())
        assert not np.array_equal(_bits(c.spmv(x))[row], _bits(ys[(0, 0)])[row])


def test_update_matrix_ell_replaces_or_drops_the_fold():
    """the stale-fold check: after kfsp_update_matrix_ell the product is that of the NEW matrix, from new tables and
    residuals where DIAG still fits the predictor and from the DIAG stream where it no longer does"""
    s = _synth()
    mdl = s.repressilator(dims=(20, 18, 16))
    new = s.repressilator(params=(80.0, 120.0, 90.0, 1.0, 2.0, 0.5), dims=(20, 18, 16))
    adj, off, diag = mdl.ell()
    adj2, off2, diag2 = new.ell()
    assert np.array_equal(adj, adj2) and not np.array_equal(diag, diag2)
    diag3 = np.array(diag2, copy=True) * (1.0 + np.random.default_rng(3).random(mdl.n))
    x = np.random.default_rng(8).standard_normal(mdl.n)
    want = []
    for d_, o_ in ((diag, off), (diag2, off2), (diag3, off2)):
        with _ctx(0, 0) as c:
            c.set_matrix_ell(adj, o_, d_)
            want.append(c.spmv(x))
    with _ctx(1, 1) as c:
        c.set_matrix_ell(adj, off, diag)
        assert c.dia_code_info()["diag_table_bytes"] > 0
        first = c.spmv(x)
        c.update_matrix_ell(adj, off2, diag2, 0)
        assert c.dia_code_info()["diag_table_bytes"] > 0
        second = c.spmv(x)
        c.update_matrix_ell(adj, off2, diag3, 0)
        ci = c.dia_code_info()
        assert ci["active"] == 1 and ci["diag_table_bytes"] == 0
        rows = c.layout_info()["chunks"] * 64
        assert c.matrix_bytes() == rows * (24 + 8) + ci["dict_bytes"]
        third = c.spmv(x)
    for got, ref in zip((first, second, third), want):
        assert np.array_equal(_bits(got), _bits(ref))
    assert not np.array_equal(first, second) and not np.array_equal(second, third)


@pytest.mark.parametrize("fold", (None, -1))
def test_default_and_size_gate_do_not_fold_a_small_generator(fold):
    """the gate that keeps the pinned byte counts: dia_code = 1 with dia_code_diag left alone does not fold, and
    dia_code_diag = -1 folds only generators that pass dia_code's own size gate, forced or not"""
    mdl = _synth().repressilator(dims=(16, 16, 16))
    with _ctx(1, fold) as c:
        c.set_matrix_csr(mdl.n, *mdl.csr_rows())
        ci, rows = c.dia_code_info(), c.layout_info()["chunks"] * 64
        assert ci["active"] == 1 and ci["diag_table_bytes"] == 0
        assert c.matrix_bytes() == rows * (24 + ci["record_bytes"]) + ci["dict_bytes"]


def test_block_product_does_not_see_the_spare_bits():
    """with the fold active the records carry residuals above the codes: k_spmm_diac (option block_dia_code) masks them"""
    mdl = _synth().repressilator(dims=(31, 23, 19))
    csr = mdl.csr_rows()
    rng = np.random.default_rng(5)
    X = np.asfortranarray(np.where(rng.random((mdl.n, 3)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 3.0, (mdl.n, 3)))
    with _ctx(0, 0) as c:
        c.set_matrix_csr(mdl.n, *csr)
        want = c.spmm(X)
    with _ctx(1, 1, block_dia_code=1) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["diag_table_bytes"] > 0
        got = c.spmm(X)
        assert c.block_info()["fmt"] == 9
        cols = np.stack([c.spmv(X[:, j]) for j in range(3)], axis=1)
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(cols), _bits(want))
    assert np.abs(got).max() > 0.0
