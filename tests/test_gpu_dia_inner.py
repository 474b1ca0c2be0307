"""The interior path of the folded banded product (option dia_code_inner): where DIAG is folded into the
records (kernel format 10) and the generator has 6 diagonals on three strides or 4 on two, every 128-row trip in which the
clamp of the x pairs acts on no lane and that holds no row of the padding (dia_inner_trip, kfsp_dia_diag.h) runs a body
without per-lane 64-bit index arithmetic: uniform bases plus 32-bit lane offsets, an unrolled diagonal loop, all loads of the
trip issued together.  The same loads, look-ups and order of additions: every product, fused dot product and whole time step
must be BIT-IDENTICAL to the plain banded kernel (dia_code = 0), with the interior path (dia_code_inner = 1) and without (0)."""
import numpy as np
import pytest

from tests.test_gpu_dia_code import _bits, _everything, _same_bits

pytestmark = pytest.mark.gpu


def _ctx(dia_code, inner=None, nt=None, **opts):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", 0)      # the one-launch Arnoldi kernel of tiny FSPs has its own product
    c.set_option("dia_mask", 0)          # only the unmasked form has a coded kernel
    c.set_option("dia_code", dia_code)
    c.set_option("dia_code_diag", 1 if dia_code else 0)
    c.set_option("dia_code_lanes", 0)
    if inner is not None:
        c.set_option("dia_code_inner", inner)
    if nt is not None:
        c.set_option("nt_loads", nt)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _synth():
    from krylovfspssa_amd import synth
    return synth


# (name, model, rows or None, folds, the diagonal count has an instantiation, interior trips restated or None)
CASES = [
    ("repressilator 16^3: 32 trips, 2 - 29 interior, 0, 1, 30 and 31 at the edges", lambda s: s.repressilator(dims=(16, 16, 16)), 4096, True, True, list(range(2, 30))),
    ("repressilator 31 x 23 x 19: odd strides, partial last trip", lambda s: s.repressilator(dims=(31, 23, 19)), 13547, True, True, list(range(6, 100))),
    ("repressilator 8 x 4 x 4: one trip, not interior", lambda s: s.repressilator(dims=(8, 4, 4)), 128, True, True, []),
    ("repressilator 5 x 5 x 5: one partial trip, not interior", lambda s: s.repressilator(dims=(5, 5, 5)), 125, True, True, []),
    ("toggle 100 x 80: 4 diagonals, two digits", lambda s: s.toggle(100, 80), 8000, True, True, list(range(1, 61))),
    ("one species, 2 diagonals: folded, no instantiation", lambda s: s.birth_death((700,)), 700, True, False, None),
    ("toggle 300 x 20: not folded, format 9 runs", lambda s: s.toggle(300, 20), None, False, False, None),
]

_MODELS, _PLAIN = {}, {}


def _model(case):
    if case not in _MODELS:
        mdl = CASES[case][1](_synth())
        _MODELS[case] = (mdl, mdl.csr_rows())
    return _MODELS[case]


def _interior(mdl):
    """the interior trips, restated: the first pair index of the trip not below -1, its last row a row, its last pair index
    not above n - 1"""
    dmax = int(max(abs(int(o)) for o in mdl.offsets))
    trips = -(-mdl.n // 128)
    return [c for c in range(trips) if 128 * c - dmax >= -1 and 128 * c + 127 <= mdl.n - 1 and 128 * c + 126 + dmax <= mdl.n - 1], dmax


def _plain(case):
    """everything from the plain banded kernel (dia_code = 0): computed once per case, never changed"""
    if case not in _PLAIN:
        mdl, csr = _model(case)
        with _ctx(0) as c:
            c.set_matrix_csr(mdl.n, *csr)
            ci = c.dia_code_info()
            assert c.layout_info()["format"] == 1 and ci["active"] == 0 and ci["inner"] == 0, CASES[case][0]
            _PLAIN[case] = _everything(c, mdl.n)
    return _PLAIN[case]


def _want_info(ci, folds, built, inner, name):
    if folds:
        assert ci["diag_table_bytes"] > 0 and ci["neighbours"] == "loads", (name, ci)
        # the slot speaks for the launch (option, fold and diagonal count); which trips are interior is dia_inner_trip's
        # business: a generator without an interior trip still launches the kernel that has the path
        assert ci["inner"] == (1 if inner and built else 0), (name, ci)
    else:
        assert ci["diag_table_bytes"] == 0 and ci["neighbours"] == "" and ci["inner"] == 0, (name, ci)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_cases_are_what_they_are_called(case):
    name, _, rows, _, built, interior = CASES[case]
    mdl, _ = _model(case)
    if rows is not None:
        assert mdl.n == rows, name
    if interior is not None:
        assert _interior(mdl)[0] == interior, name
        assert len(mdl.offsets) == (4 if "toggle" in name else 6)
    with _ctx(1, 1) as c:
        c.set_matrix_csr(mdl.n, *_model(case)[1])
        _want_info(c.dia_code_info(), CASES[case][3], built, 1, name)


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("inner", (1, 0))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_interior_path_gives_the_bits_of_the_plain_banded_kernel(case, inner, nt):
    name, _, _, folds, built, _ = CASES[case]
    mdl, csr = _model(case)
    want = _plain(case)
    with _ctx(1, inner, nt) as c:
        c.set_matrix_csr(mdl.n, *csr)
        ci = c.dia_code_info()
        assert c.layout_info()["format"] == 1 and ci["active"] == 1, name
        _want_info(ci, folds, built, inner, name)
        got = _everything(c, mdl.n)
    _same_bits(got, want, (name, "inner" if inner else "present", nt))
    assert np.abs(got["spmv"]).max() > 0.0


def test_the_option_is_read_at_every_launch_and_the_lanes_take_precedence():
    mdl, csr = _model(0)
    x = np.random.default_rng(9).standard_normal(mdl.n)
    with _ctx(1, 0) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["inner"] == 0
        y0 = c.spmv(x)
        c.set_option("dia_code_inner", 1)
        assert c.dia_code_info()["inner"] == 1 and c.dia_code_info()["neighbours"] == "loads"
        y1 = c.spmv(x)
        c.set_option("dia_code_lanes", 1)
        ci = c.dia_code_info()
        assert ci["inner"] == 0 and ci["neighbours"] == "lanes", ci
        y2 = c.spmv(x)
    assert np.array_equal(_bits(y0), _bits(y1)) and np.array_equal(_bits(y0), _bits(y2))


@pytest.mark.parametrize("case", (0, 1, 4))
def test_first_and_last_word_of_interior_trips(case):
    """unit vectors at the first and the last x index the first and the last interior trip read (their lanes 0 and 63 on
    the farthest diagonals), at the index just outside on either side, and a vector of distinct integers: a scalar base off
    by one row, two diagonals' shifts swapped or a rule that admits one trip more moves an entry of the product."""
    mdl, csr = _model(case)
    n = mdl.n
    interior, dmax = _interior(mdl)
    assert interior == CASES[case][5] and len(interior) >= 2
    at = set()
    for c in (interior[0], interior[-1]):
        for j in (128 * c - dmax - 1, 128 * c - dmax, 128 * c - dmax + 1, 128 * c, 128 * c + 127,
                  128 * c + 126 + dmax, 128 * c + 127 + dmax, 128 * c + 128 + dmax):
            if 0 <= j < n:
                at.add(j)
    xs = []
    for j in sorted(at):
        e = np.zeros(n)
        e[j] = 1.0
        xs.append(e)
    xs.append(np.arange(1, n + 1, dtype=np.float64))
    with _ctx(0) as c:
        c.set_matrix_csr(n, *csr)
        want = [c.spmv(x) for x in xs]
    for inner in (1, 0):
        with _ctx(1, inner) as c:
            c.set_matrix_csr(n, *csr)
            assert c.dia_code_info()["inner"] == inner
            got = [c.spmv(x) for x in xs]
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(_bits(g), _bits(w)), (inner, i, np.flatnonzero(_bits(g) != _bits(w))[:8])
    assert all(np.count_nonzero(w) >= 1 for w in want)


@pytest.mark.parametrize("grid", (8, 0))
def test_grid_shapes(grid):
    """grid_blocks = 8: 32 wavefronts walk all trips, several trips per wavefront (the loop around the two bodies, interior and
    edge trips in turn); 0: the default grid.  (the partial sums follow the grid, so the plain kernel runs on the same grid)"""
    mdl, csr = _model(1)
    with _ctx(0, grid_blocks=grid) as c:
        c.set_matrix_csr(mdl.n, *csr)
        want = _everything(c, mdl.n)
    with _ctx(1, 1, grid_blocks=grid) as c:
        c.set_matrix_csr(mdl.n, *csr)
        assert c.dia_code_info()["inner"] == 1
        got = _everything(c, mdl.n)
    _same_bits(got, want, ("grid_blocks", grid))


@pytest.mark.parametrize("case", (5, 4))
def test_edge_trips_keep_the_clamped_words(case):
    """x[0] = x[last] = inf: in the edge trips the clamp of ld_xpair chooses the words that meet them - stored zeros times inf
    are NaNs exactly where the plain kernel has them.  A rule that admits an edge trip reads other words there.  Case 5 is the
    one-species generator (no instantiation: `inner` reports 0 and the present kernel runs), case 4 the same vector on a
    generator that runs the interior path."""
    name, _, _, _, built, _ = CASES[case]
    mdl, csr = _model(case)
    n = mdl.n
    x = np.random.default_rng(21).standard_normal(n)
    x[0] = np.inf
    x[n - 1] = np.inf
    with _ctx(0) as c:
        c.set_matrix_csr(n, *csr)
        assert c.layout_info()["format"] == 1
        want = c.spmv(x)
    assert not np.isfinite(want[0]) and not np.isfinite(want[n - 1]) and np.isfinite(want[2:n - 2]).sum() >= n - 4 - 2 * 128
    for inner in (1, 0):
        with _ctx(1, inner) as c:
            c.set_matrix_csr(n, *csr)
            ci = c.dia_code_info()
            assert ci["diag_table_bytes"] > 0 and ci["inner"] == (inner if built else 0), ci
            got = c.spmv(x)
        assert np.array_equal(_bits(got), _bits(want)), (name, inner, np.flatnonzero(_bits(got) != _bits(want))[:8])
