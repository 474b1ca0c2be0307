"""Banded generator with dictionary-coded values (kernel format 9): per diagonal the distinct doubles
once, per row one 8- or 16-bit code per diagonal, the dictionaries in LDS.  The coded kernel multiplies the very doubles
of the plain value streams in the same order, so everything it feeds - products, the fused dot products of the Arnoldi
columns, whole time steps - must be BIT-IDENTICAL to the plain banded kernel (option dia_code = 0) on the same inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ctx(dia_code):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", 0)      # the one-launch Arnoldi kernel of tiny FSPs has its own product
    c.set_option("dia_mask", 0)          # only the unmasked form has a coded kernel
    c.set_option("dia_code", dia_code)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _everything(c, n, seed=3):
    """products, an Arnoldi pass and fixed steps on the generator c holds"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    p0 = rng.random(n)
    p0 /= p0.sum()
    out = {"spmv": c.spmv(x)}
    c.set_vector(p0)
    out["spmv_w"] = c.spmv_w()
    out["beta"] = np.array([c.begin_step()])
    H, mb, k1, av = c.arnoldi(12)
    out["H"] = H.copy()
    out["avnorm"] = np.array([av, float(mb), float(k1)])
    c.set_vector(p0)
    out["wsum"] = c.expv_fixed(10, 0.01, 3)
    out["w"] = c.get_vector()
    return out


def _same_bits(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _models():
    from krylovfspssa_amd import synth
    return [("tiny repressilator", synth.repressilator(dims=(16, 16, 16)), 8, 8),
            ("toggle 100 x 80", synth.toggle(100, 80), 8, 8),
            ("toggle 1000 x 1000", synth.toggle(1000, 1000), 16, 8),
            ("repressilator, last group partial", synth.repressilator(dims=(31, 23, 19)), 8, 8),
            ("6 species, 12 diagonals: 16-byte records", synth.birth_death((5, 6, 4, 5, 3, 4)), 8, 16),
            ("6 diagonals of two-byte codes: 16-byte records", synth.repressilator(dims=(300, 6, 5)), 16, 16)]


@pytest.mark.parametrize("case", range(6))
def test_coded_values_give_the_bits_of_the_plain_banded_kernel(case):
    name, mdl, width, rec = _models()[case]
    if case == 3:
        assert mdl.n % 128 != 0
    rowptr, col, val = mdl.csr_rows()
    res = {}
    for dc in (0, 1):
        with _ctx(dc) as c:
            c.set_matrix_csr(mdl.n, rowptr, col, val)
            info, ci = c.layout_info(), c.dia_code_info()
            assert info["format"] == 1, name                       # kfsp_layout_info keeps calling it banded
            if dc:
                assert ci["active"] == 1 and ci["width"] == width and ci["record_bytes"] == rec, (name, ci)
                assert max(ci["distinct"]) <= (256 if width == 8 else 65536)
                assert ci["dict_bytes"] == 8 * sum(ci["distinct"]) <= 40 * 1024
            else:
                assert ci["active"] == 0 and ci["width"] == 0, (name, ci)
            res[dc] = _everything(c, mdl.n)
    _same_bits(res[1], res[0], name)
    assert np.abs(res[1]["spmv"]).max() > 0.0


def test_arbitrary_values_fall_back_to_the_plain_kernel():
    """more than 65 536 distinct values per diagonal: no coded image, counting stopped early, same results"""
    from krylovfspssa_amd import synth
    mdl = synth.toggle(300, 300)
    rowptr, col, val = mdl.csr_rows()
    val = np.random.default_rng(11).random(len(val)) + 0.5
    assert len(np.unique(val)) > 65536 * 4
    res, nbytes = {}, {}
    for dc in (0, 1):
        with _ctx(dc) as c:
            c.set_matrix_csr(mdl.n, rowptr, col, val)
            ci = c.dia_code_info()
            assert c.layout_info()["format"] == 1
            assert ci["active"] == 0 and ci["width"] == 0 and ci["coded_bytes"] == 0 and ci["dict_bytes"] == 0
            if dc:
                # the count of a diagonal stops soon after the 5120 entries the LDS budget allows: no full pass, no sort
                assert max(ci["distinct"]) > 5120 and max(ci["distinct"]) < 65536
            nbytes[dc] = c.matrix_bytes()
            res[dc] = _everything(c, mdl.n)
    assert nbytes[0] == nbytes[1]
    _same_bits(res[1], res[0], "random values")


def test_both_zeros_are_dictionary_entries():
    """+0.0 and -0.0 are different 64-bit patterns: both must come back from the dictionary of their diagonal"""
    from krylovfspssa_amd import synth
    mdl = synth.toggle(100, 80)
    adj, off, diag = mdl.ell()
    off = np.array(off, dtype=np.float64, copy=True)
    live = adj >= 1
    rng = np.random.default_rng(2)
    pick = live & (rng.random(off.shape) < 0.2)
    off[pick] = -0.0
    off[live & ~pick & (rng.random(off.shape) < 0.2)] = 0.0
    res = {}
    for dc in (0, 1):
        with _ctx(dc) as c:
            c.set_matrix_ell(adj, off, diag)
            assert c.layout_info()["format"] == 1
            if dc:
                ci = c.dia_code_info()
                assert ci["active"] == 1
                dicts = [_bits(c.dia_code_dict(d)) for d in range(ci["diagonals"])]
                for d, D in enumerate(dicts):
                    assert len(D) == ci["distinct"][d] and np.all(D[1:] > D[:-1])          # ascending, no pattern twice
                    assert 0 in D and (1 << 63) in D, d                                    # +0.0 and -0.0
                stored = set(_bits(off[live]).tolist()) | {0}
                assert set(np.concatenate(dicts).tolist()) == stored
            res[dc] = _everything(c, mdl.n)
    _same_bits(res[1], res[0], "signed zeros")


def test_update_matrix_ell_replaces_the_coded_image():
    """the stale-image check: after kfsp_update_matrix_ell changed the values the product is that of the NEW matrix"""
    from krylovfspssa_amd import synth
    mdl = synth.repressilator(dims=(20, 18, 16))
    adj, off, diag = mdl.ell()
    off2 = np.array(off, copy=True) * (1.0 + np.arange(off.shape[0]) % 7)[:, None]
    diag2 = np.array(diag, copy=True) * 1.25
    x = np.random.default_rng(8).standard_normal(mdl.n)
    ys = {}
    for dc in (0, 1):
        with _ctx(dc) as c:
            c.set_matrix_ell(adj, off, diag)
            first = c.spmv(x)
            if dc:
                assert c.dia_code_info()["active"] == 1
                before = c.dia_code_info()["distinct"]
            c.update_matrix_ell(adj, off2, diag2, 0)
            if dc:
                assert c.dia_code_info()["active"] == 1 and c.dia_code_info()["distinct"] != before
            ys[dc] = (first, c.spmv(x))
    assert np.array_equal(_bits(ys[1][0]), _bits(ys[0][0])) and np.array_equal(_bits(ys[1][1]), _bits(ys[0][1]))
    assert not np.array_equal(ys[1][0], ys[1][1])
    # ... and a generator that no longer codes drops the image
    with _ctx(1) as c:
        c.set_matrix_ell(adj, off, diag)
        assert c.dia_code_info()["active"] == 1
        rnd = np.random.default_rng(4).random(off.shape) + 0.5
        c.update_matrix_ell(adj, rnd, diag, 0)
        assert c.dia_code_info()["active"] == 0 and c.dia_code_info()["width"] == 0
        y = c.spmv(x)
    with _ctx(0) as c:
        c.set_matrix_ell(adj, rnd, diag)
        assert np.array_equal(_bits(c.spmv(x)), _bits(y))


def test_matrix_bytes_counts_what_the_selected_kernel_moves():
    from krylovfspssa_amd import synth
    mdl = synth.repressilator(dims=(40, 40, 40))          # the shape of the benchmark's generator: 6 diagonals, one-byte codes
    rowptr, col, val = mdl.csr_rows()
    with _ctx(1) as c:
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        ci, rows = c.dia_code_info(), c.layout_info()["chunks"] * 64
        assert ci["diagonals"] == 6 and ci["width"] == 8 and ci["record_bytes"] == 8
        assert ci["coded_bytes"] == rows * 8
        assert c.matrix_bytes() == rows * (24 + ci["record_bytes"]) + ci["dict_bytes"]
        coded = c.matrix_bytes()
    with _ctx(0) as c:
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        assert c.matrix_bytes() == rows * 24 + c.matrix_info()["slots"] * 8      # the plain banded figure, as before
        assert coded < 0.5 * c.matrix_bytes()
    with _ctx(-1) as c:                                                          # auto: a generator this small is not coded
        c.set_matrix_csr(mdl.n, rowptr, col, val)
        assert c.dia_code_info()["active"] == 0
