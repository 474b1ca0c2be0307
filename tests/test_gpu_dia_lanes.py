"""The lane path of the folded banded product (option dia_code_lanes): where DIAG is folded into the records
(kernel format 10) the pairs of x of the -1 and +1 diagonals come from the neighbour lanes' registers - a whole-wavefront
shift by one lane - and one 8-byte load of lanes 0 and 63, in every 128-row trip the clamp at the ends of x cannot touch
(dia_lanes_trip, kfsp_dia_diag.h).  They are the same doubles, so every product, fused dot product and whole time step must
be BIT-IDENTICAL to the plain banded kernel (dia_code = 0), with the lane path (dia_code_lanes = 1) and without (0)."""
import numpy as np
import pytest

from tests.test_gpu_dia_code import _bits, _everything, _same_bits

pytestmark = pytest.mark.gpu


def _ctx(dia_code, lanes=None, nt=None, **opts):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", 0)      # the one-launch Arnoldi kernel of tiny FSPs has its own product
    c.set_option("dia_mask", 0)          # only the unmasked form has a coded kernel
    c.set_option("dia_code", dia_code)
    c.set_option("dia_code_diag", 1 if dia_code else 0)
    if lanes is not None:
        c.set_option("dia_code_lanes", lanes)
    if nt is not None:
        c.set_option("nt_loads", nt)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _synth():
    from krylovfspssa_amd import synth
    return synth


# (name, model, rows or None, folds)
CASES = [
    ("repressilator 16^3: a multiple of 128 rows, the last trip is full and takes the lanes", lambda s: s.repressilator(dims=(16, 16, 16)), 4096, True),
    ("repressilator 31 x 23 x 19: partial last trip, padding rows", lambda s: s.repressilator(dims=(31, 23, 19)), 13547, True),
    ("repressilator 8 x 4 x 4: one full trip, lane 0 reads the guard word x[-1]", lambda s: s.repressilator(dims=(8, 4, 4)), 128, True),
    ("repressilator 5 x 5 x 5: one partial trip, loads only", lambda s: s.repressilator(dims=(5, 5, 5)), 125, True),
    ("toggle 100 x 80: two digits", lambda s: s.toggle(100, 80), None, True),
    ("toggle 300 x 20: not folded, format 9 runs", lambda s: s.toggle(300, 20), None, False),
    ("6 species, 16-byte records: not folded, format 9 runs", lambda s: s.birth_death((5, 6, 4, 5, 3, 4)), None, False),
]

_MODELS, _PLAIN = {}, {}


def _model(case):
    if case not in _MODELS:
        mdl = CASES[case][1](_synth())
        _MODELS[case] = (mdl, mdl.csr_rows())
    return _MODELS[case]


def _plain(case):
    """everything from the plain banded kernel (dia_code = 0): computed once per case, never changed"""
    if case not in _PLAIN:
        mdl, csr = _model(case)
        with _ctx(0) as c:
            c.set_matrix_csr(mdl.n, *csr)
            assert c.layout_info()["format"] == 1 and c.dia_code_info()["active"] == 0, CASES[case][0]
            _PLAIN[case] = _everything(c, mdl.n)
    return _PLAIN[case]


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("lanes", (1, 0))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_lane_path_gives_the_bits_of_the_plain_banded_kernel(case, lanes, nt):
    name, _, rows, folds = CASES[case]
    mdl, csr = _model(case)
    if rows is not None:
        assert mdl.n == rows, name
    want = _plain(case)
    with _ctx(1, lanes, nt) as c:
        c.set_matrix_csr(mdl.n, *csr)
        ci = c.dia_code_info()
        assert c.layout_info()["format"] == 1 and ci["active"] == 1, name
        if folds:
            assert ci["diag_table_bytes"] > 0, (name, ci)
            # the slot speaks for the launch (option and fold); which trips take the lanes is dia_lanes_trip's business:
            # the 125-row generator has one partial trip and its product is right through the loads
            assert ci["neighbours"] == ("lanes" if lanes else "loads"), (name, ci)
        else:
            assert ci["diag_table_bytes"] == 0 and ci["neighbours"] == "", (name, ci)
        got = _everything(c, mdl.n)
    _same_bits(got, want, (name, "lanes" if lanes else "loads", nt))
    assert np.abs(got["spmv"]).max() > 0.0


def test_default_is_the_loaded_path_and_the_option_is_read_at_every_launch():
    mdl, csr = _model(0)
    x = np.random.default_rng(9).standard_normal(mdl.n)
    with _ctx(1) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["neighbours"] == "loads"             # the lanes measured slower
        y0 = c.spmv(x)
        c.set_option("dia_code_lanes", 1)
        assert c.dia_code_info()["neighbours"] == "lanes"
        y1 = c.spmv(x)
    assert np.array_equal(_bits(y0), _bits(y1))


@pytest.mark.parametrize("case", (0, 1))
def test_edge_words_of_every_trip(case):
    """unit vectors at the first and last rows of trips (lanes 0 and 63 and their neighbours) and a vector of distinct
    integers: a swapped shift direction or an edge lane that keeps its shifted-in word moves an entry of the product.
    On 16^3 every trip starts a line of the fastest species, where the -1 / +1 entries are stored zeros; on 31 x 23 x 19
    the trips' edges lie inside lines, so the edge words meet stored values that are not zero."""
    mdl, csr = _model(case)
    n = mdl.n
    xs = []
    for j in (126, 127, 128, 129, 255, 256, 257, n - 129, n - 128, n - 1):
        e = np.zeros(n)
        e[j] = 1.0
        xs.append(e)
    xs.append(np.arange(1, n + 1, dtype=np.float64))
    with _ctx(0) as c:
        c.set_matrix_csr(n, *csr)
        want = [c.spmv(x) for x in xs]
    for lanes in (1, 0):
        with _ctx(1, lanes) as c:
            c.set_matrix_csr(n, *csr)
            assert c.dia_code_info()["neighbours"] == ("lanes" if lanes else "loads")
            got = [c.spmv(x) for x in xs]
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(g), _bits(w)), (lanes, i, np.flatnonzero(_bits(g) != _bits(w))[:8])
    assert all(np.count_nonzero(w) >= 1 for w in want)
    if case == 1:
        # e_127 reaches row 128 through lane 0's edge word and e_128 row 127 through lane 63's: neither entry is a stored zero
        assert want[1][128] != 0.0 and want[2][127] != 0.0 and want[1][126] != 0.0 and want[2][129] != 0.0


@pytest.mark.parametrize("grid", (8, 0))
def test_grid_shapes(grid):
    """grid_blocks = 8: 32 wavefronts walk all trips, several trips per wavefront (the loop around rows_dia); 0: the default grid.
    (the partial sums follow the grid, so the plain kernel runs on the same grid)"""
    mdl, csr = _model(1)
    with _ctx(0, grid_blocks=grid) as c:
        c.set_matrix_csr(mdl.n, *csr)
        want = _everything(c, mdl.n)
    with _ctx(1, 1, grid_blocks=grid) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["neighbours"] == "lanes"
        got = _everything(c, mdl.n)
    _same_bits(got, want, ("grid_blocks", grid))


def test_last_trip_keeps_the_clamped_words():
    """The partial last trip must keep the loads: there the clamp of ld_xpair chooses the words.  A one-species generator (only
    the -1 and +1 diagonals, 700 rows: `last` is a lane's second row) with x[last] = inf: row `last` multiplies the stored
    zero of its +1 diagonal with the guard word behind x and stays -inf; a lane path taken one trip too far hands it the
    clamped x[last] of the next lane - 0 x inf, a NaN.  (With more diagonals the far ones clamp to x[last] in both paths.)"""
    mdl = _synth().birth_death((700,))
    csr = mdl.csr_rows()
    n = mdl.n
    assert n == 700
    x = np.random.default_rng(21).standard_normal(n)
    x[n - 1] = np.inf
    with _ctx(0) as c:
        c.set_matrix_csr(n, *csr)
        assert c.layout_info()["format"] == 1
        want = c.spmv(x)
    assert np.isinf(want[n - 1]) and np.isfinite(want[:n - 2]).all()
    for lanes in (1, 0):
        with _ctx(1, lanes) as c:
            c.set_matrix_csr(n, *csr)
            ci = c.dia_code_info()
            assert ci["diag_table_bytes"] > 0 and ci["neighbours"] == ("lanes" if lanes else "loads"), ci
            got = c.spmv(x)
        assert np.array_equal(_bits(got), _bits(want)), (lanes, np.flatnonzero(_bits(got) != _bits(want))[:8])
