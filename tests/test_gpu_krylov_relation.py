"""The Arnoldi pass and the combine on the device against tests/krylov_ref.py: every column of every
path that computes a pass is checked LOCALLY - the relation per element, the coefficients, the normalisation, AVNORM -
in extended precision on the device's own basis columns and H, with tolerances that count roundings; so are
begin_step, nrm2_w, asum_w, restore_w and combine.  Sizes are the smallest that reach each edge: odd n, 63 / 64 / 65,
both sides of the 4096-row switch to the one-launch kernel, vector grids that make k_ortho2 loop with and without its
second half-trip, and all of it again after a larger generator has been resident.  Run with -s for the ratios."""
import numpy as np
import pytest

from tests import krylov_ref as K

pytestmark = pytest.mark.gpu

WORST = {}          # path -> worst ratio per bound over the module's run


@pytest.fixture(scope="module", autouse=True)
def _table():
    yield
    print("\nworst error / bound per path")
    for path in sorted(WORST):
        print(f"  {path:34s} {K.fmt(WORST[path])}")


def _ctx(opts=None, group=None):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0, group=group)
    for k, v in (opts or {}).items():
        c.set_option(k, v)
    return c


def _done(path, what, r):
    print(f"\n{path:34s} {what:30s} {K.fmt(r)}")
    K.merge(WORST.setdefault(path, {}), {k: v for k, v in r.items() if k not in ("negative",)})
    K.assert_ok(r, f"{path}, {what}")


def _get(kind, n, near=False):
    """general / banded case of size n, or its near-invariant sibling (krylov_ref.near_invariant_case): the only cases
    on which u_j . u_{j-1} - k_ortho2's partial_g, its finish, gfin across a restart - is more than rounding noise"""
    c = K.general_case(n) if kind == "general" else K.banded_case(n)
    return K.near_invariant_case(c) if near else c


class _Basis:
    """get_basis with every column fetched once"""

    def __init__(self, ctx):
        self.ctx, self.cols = ctx, {}

    def __call__(self, k):
        if k not in self.cols:
            self.cols[k] = self.ctx.get_basis(k)
        return self.cols[k]


def _combine(ctx, case, basis, mx, r):
    b, y = K.combine_coefficients(case, mx)
    V = [basis(j + 1) for j in range(mx)]
    ws = ctx.combine(mx, b, y)
    rc = K.check_combine(V, b, y, ctx.get_vector(), ws)
    if mx > 1:                                       # the device's own basis offers what the builder's did
        neg, pos, either = K.combine_fractions(*K.combine_exact(V, b, y))
        assert neg >= 0.1 and pos >= 0.1, (mx, neg, pos)
    K.merge(r, rc)
    r["negative"] = r.get("negative", 0) + rc["negative"]


def _whole_pass(ctx, case, qiop=2, combine=True):
    """set_vector, the reductions, begin_step, one pass of m columns, AVNORM, restore_w (twice), a combine of all
    m + 1 columns: every check of krylov_ref on what the device returns -> ratios"""
    gen, m, w = case.gen(), case.m, case.w
    ctx.set_vector(w)
    got = ctx.get_vector()
    assert np.array_equal(got, w)
    r = K.check_reductions(got, ctx.nrm2_w(), ctx.asum_w())
    beta = ctx.begin_step()
    basis = _Basis(ctx)
    K.merge(r, K.check_begin(w, beta, basis(1)))
    H, mb, k1, av = ctx.arnoldi(m, qiop=qiop)
    assert (mb, k1) == (m, 2) and H[m + 1, m] == 1.0
    if hasattr(case, "min_dot"):                     # a window that is not orthogonal: g decides H(2,2) and H(3,3)
        assert abs(basis(1) @ basis(2)) >= case.min_dot, (basis(1) @ basis(2), case.min_dot)
    K.check_pass(gen, basis, H, 1, m, qiop=qiop, into=r)
    K.merge(r, K.check_avnorm(gen, basis(m + 1), av))
    ctx.restore_w(beta)
    K.merge(r, K.check_restore(ctx.get_vector(), w))
    ctx.restore_w(0.75 * beta)
    K.merge(r, K.check_restore(ctx.get_vector(), w, scale=0.75))
    if combine and case.n >= 63:
        _combine(ctx, case, basis, m + 1, r)
    return r, H, av


def _one_launch_eligible(ctx):
    """kfsp_arnoldi takes k_arnoldi_small when the padded rows fit (chunks x 64 <= 4096) on a stored generator without a
    partition; kfsp_layout_info exposes the inputs of that rule (the timers do not tell the kernels apart)"""
    info = ctx.layout_info()
    return info["chunks"] * 64 <= 4096 and info["format"] in (0, 1, 2, 5) and info["exchange"] == 0


# ---- multi-launch fused: k_spmv MODE 1 (column 1), MODE 3, MODE 2, k_ortho2 --------------------------------------------------
NEAR_N = (65, 2049, 4097, 8193)
GENERAL_AND_NEAR = [(n, False) for n in K.GENERAL_N] + [(n, True) for n in NEAR_N]
BANDED_AND_NEAR = [(n, False) for n in K.BANDED_N] + [(n, True) for n in K.BANDED_N]


@pytest.mark.parametrize("n,near", GENERAL_AND_NEAR)
def test_multi_launch_pass(n, near):
    case = _get("general", n, near)
    with _ctx({"small_kernel": 0}) as c:
        case.upload(c)
        assert c.layout_info()["format"] in (0, 5)
        r, _, _ = _whole_pass(c, case)
    _done("multi-launch SELL", case.name, r)


@pytest.mark.parametrize("n,near", BANDED_AND_NEAR)
def test_multi_launch_pass_banded(n, near):
    case = _get("banded", n, near)
    with _ctx({"small_kernel": 0}) as c:
        case.upload(c)
        assert c.layout_info()["format"] in (1, 2)
        r, _, _ = _whole_pass(c, case)
    _done("multi-launch banded", case.name, r)


@pytest.mark.parametrize("vgrid,grid", [(1, 8), (3, 8), (1, 0)])
@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("n", [4097, 8193])
def test_forced_grids(n, vgrid, grid, near):
    """vec_grid_blocks 1 / 3: k_ortho2 and the streaming kernels stride 256 / 768 pairs over 2080 (n = 4097) or 4128 (8193)
    pairs: 9, 3, 17 and 6 half-trips - five, two, nine and three iterations, the last one without its second half except
    in the last case.  grid_blocks 8: the product kernels stride over their trips.  On the near-invariant siblings the g
    summed over those tails and finished over those partials decides H(2,2)."""
    case = _get("general", n, near)
    opts = {"small_kernel": 0, "vec_grid_blocks": vgrid}
    if grid:
        opts["grid_blocks"] = grid
    with _ctx(opts) as c:
        case.upload(c)
        pairs = c.layout_info()["chunks"] * 32
        half_trips = -(-pairs // (256 * vgrid))
        assert half_trips == {(4097, 1): 9, (4097, 3): 3, (8193, 1): 17, (8193, 3): 6}[(n, vgrid)]
        r, _, _ = _whole_pass(c, case)
    _done("multi-launch, forced grids", f"{case.name} vgrid {vgrid} grid {grid}", r)


@pytest.mark.parametrize("n,near", [(3, False), (65, False), (2049, False), (4097, False), (8193, False), (65, True), (4097, True)])
def test_literal_sequence(n, near):
    """fused_ortho = 0: one k_ortho launch per window column"""
    case = _get("general", n, near)
    with _ctx({"fused_ortho": 0}) as c:
        case.upload(c)
        r, _, _ = _whole_pass(c, case)
    _done("literal sequence (k_ortho)", case.name, r)


@pytest.mark.parametrize("qiop", [0, 1, 3])
@pytest.mark.parametrize("n", [65, 2049, 4097])
def test_other_windows(n, qiop):
    case = K.general_case(n)
    with _ctx() as c:
        case.upload(c)
        r, _, _ = _whole_pass(c, case, qiop=qiop, combine=False)
    _done(f"qiop {qiop} (k_ortho)", case.name, r)


# ---- the one-launch pass ------------------------------------------------------------------------------------------------------
ONE_LAUNCH = [("general", n, False) for n in K.GENERAL_N if n <= 4096] + [("banded", n, False) for n in K.BANDED_N if n <= 4096] + \
             [("general", 65, True), ("general", 2049, True), ("general", 4096, True), ("banded", 4095, True)]


@pytest.mark.parametrize("small_lds", [1, 0])
@pytest.mark.parametrize("kind,n,near", ONE_LAUNCH, ids=[f"{'near_' if nr else ''}{k}{n}" for k, n, nr in ONE_LAUNCH])
def test_one_launch_pass(kind, n, near, small_lds):
    """default options up to 4096 rows.  That k_arnoldi_small ran, and not the multi-launch kernels behind the library's
    back, shows in the bits (neither the timers nor kfsp_layout_info tell): from 63 rows on H and AVNORM differ from the
    same pass with small_kernel = 0, whose dot products are summed in another order.  (At n = 2 and 3 a sum has two or
    three terms and both orders give the same bits: nothing is asked there.)"""
    case = _get(kind, n, near)
    with _ctx({"small_lds": small_lds}) as c:
        case.upload(c)
        assert _one_launch_eligible(c)
        r, H, av = _whole_pass(c, case)
    _done(f"one-launch {'SELL' if kind == 'general' else 'banded'}", f"{case.name} small_lds {small_lds}", r)
    if n >= 63:
        with _ctx({"small_lds": small_lds, "small_kernel": 0}) as c:
            case.upload(c)
            _, H0, av0 = _whole_pass(c, case, combine=False)
        assert not (np.array_equal(H, H0) and av == av0)


@pytest.mark.parametrize("kind,n", [("general", 4095), ("general", 4096), ("general", 4097), ("banded", 4095), ("banded", 4097)])
def test_which_side_of_the_switch_ran(kind, n):
    """default options at the switch: up to 4096 rows the one-launch kernel, 4097 the multi-launch path.  The rule's
    inputs are in kfsp_layout_info; what ran shows in the bits: against the same pass with small_kernel = 0, H and AVNORM
    are the same bits at 4097 (the same kernels) and not below (k_arnoldi_small sums its dot products over 1024 lanes of
    one workgroup, the multi-launch kernels over blocks of 256 and their partials)."""
    case = K.general_case(n) if kind == "general" else K.banded_case(n)
    out = []
    for small in (1, 0):
        with _ctx({"small_kernel": small}) as c:
            case.upload(c)
            assert _one_launch_eligible(c) == (n <= 4096)
            r, H, av = _whole_pass(c, case, combine=False)
            out.append((H.copy(), av))
        _done("default options at the switch", f"{case.name} small_kernel {small}", r)
    same = np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert same == (n > 4096)


# ---- restart and shrink -------------------------------------------------------------------------------------------------------
RESTARTS = [("general", 65, False, 6), ("general", 2049, False, 6), ("banded", 4095, False, 6), ("general", 4097, False, 6),
            ("banded", 4097, False, 6), ("general", 65, True, 2), ("general", 2049, True, 2), ("banded", 4095, True, 2),
            ("general", 4097, True, 2), ("banded", 4097, True, 2), ("general", 8193, True, 2)]


@pytest.mark.parametrize("kind,n,near,first", RESTARTS, ids=[f"{'near_' if nr else ''}{k}{n}-jold{f}" for k, n, nr, f in RESTARTS])
def test_restart_and_shrink(kind, n, near, first):
    """arnoldi(6), arnoldi(9, jold = 6, H) recomputes column 6 and goes on, arnoldi(4, jold = 9) only takes AVNORM from
    column 9: the relation holds for every column across the restart, the shrunk AVNORM is ||A v_9||.  On the
    near-invariant siblings the restart is at column 2: the g it resumes with, u_2 . u_1 kept from the first call (gfin),
    is the one that is not rounding noise and decides H(2,2)."""
    case = _get(kind, n, near)
    gen = case.gen()
    with _ctx() as c:
        case.upload(c)
        path = ("one-launch" if _one_launch_eligible(c) else "multi-launch") + ", restart and shrink"
        c.set_vector(case.w)
        c.begin_step()
        H0, mb, k1, _ = c.arnoldi(first)
        assert (mb, k1) == (first, 2)
        H1 = np.zeros((11, 11), order="F")
        H1[:first + 1, :first] = H0[:first + 1, :first]
        H1, mb, k1, av = c.arnoldi(9, jold=first, H=H1)
        assert (mb, k1) == (9, 2) and np.array_equal(H1[:first, :first - 1], H0[:first, :first - 1])
        basis = _Basis(c)
        if near:
            assert abs(basis(1) @ basis(2)) >= case.min_dot
        r = K.check_pass(gen, basis, H1, 1, 9)
        K.merge(r, K.check_avnorm(gen, basis(10), av))
        H2 = np.zeros((6, 6), order="F")
        _, mb, k1, av2 = c.arnoldi(4, jold=9, H=H2)
        assert (mb, k1) == (4, 2) and H2[5, 4] == 1.0
        r["avnorm after the shrink"] = K.check_avnorm(gen, basis(9), av2)["avnorm"]
        assert np.array_equal(c.get_basis(9), basis(9))
    _done(path, case.name, r)


# ---- stored formats -----------------------------------------------------------------------------------------------------------
# (options, the kernel format kfsp_layout_info must report, dia_code active) per case; small_kernel = 0: the product kernels
# of the multi-launch path are the ones that differ by format
SELL = {"small_kernel": 0, "format": 1, "sell_code": 0}
SELL_CODED = {"small_kernel": 0, "format": 1, "sell_code": 1}
BANDED = {"small_kernel": 0, "dia_mask": 0, "dia_code": 0}
MASKED = {"small_kernel": 0, "dia_mask": 1, "dia_code": 0}
DIA_CODED = {"small_kernel": 0, "dia_mask": 0, "dia_code": 1}
ORDERED = {"state_order": 1, "state_order_min": 1, "state_order_products": 0}
# (bandedq: the 4097-row banded case with 200 distinct values per diagonal, which the one-byte codes of format 9 can hold)
STORED = [("bandedq", 4097, BANDED, 1, 0), ("bandedq", 4097, DIA_CODED, 1, 1), ("banded", 4097, SELL_CODED, 5, 0),
          ("banded", 4095, SELL_CODED, 5, 0),
          ("banded", 131, SELL, 0, 0), ("banded", 131, SELL_CODED, 5, 0), ("banded", 131, BANDED, 1, 0), ("banded", 131, DIA_CODED, 1, 1),
          ("banded", 4095, SELL, 0, 0), ("banded", 4095, BANDED, 1, 0), ("banded", 4095, MASKED, 2, 0),
          ("banded", 4097, SELL, 0, 0), ("banded", 4097, BANDED, 1, 0), ("banded", 4097, MASKED, 2, 0),
          ("golden", 0, SELL, 0, 0), ("golden", 0, dict(SELL_CODED, **ORDERED), 5, 0)]


@pytest.mark.parametrize("i", range(len(STORED)), ids=[f"{k}{n}-fmt{f}{'c' if dc else ''}" for k, n, _, f, dc in STORED])
def test_stored_formats(golden_dir, i):
    kind, n, opts, fmt, coded = STORED[i]
    case = K.banded_case(n) if kind == "banded" else K.banded_case(n, levels=200) if kind == "bandedq" else K.golden_case(golden_dir)
    with _ctx(opts) as c:
        if kind == "golden":
            c.set_state_coords(np.load(f"{golden_dir}/assembly_goutsias_k10.npz")["state"])
        case.upload(c)
        info = c.layout_info()
        assert info["format"] == fmt, info
        assert c.dia_code_info()["active"] == coded
        if fmt == 5:
            assert info["coded_chunks"] > 0
        r, _, _ = _whole_pass(c, case)
    _done(f"stored format {9 if coded else fmt}", case.name, r)


# ---- matrix-free boxes --------------------------------------------------------------------------------------------------------
BOX_FORMS = [("toggle", {"box_generic": 1}, 3), ("toggle", {}, 4), ("toggle", {"box_lds": 1}, 6),
             ("repressilator", {"box_generic": 1}, 3), ("repressilator", {"box_pencil": 0}, 4), ("repressilator", {"box_lds": 1}, 6),
             ("repressilator", {"box_pencil": 1}, 7),
             ("birth_death6", {"box_generic": 1}, 3), ("birth_death6", {"box_pencil": 0}, 4), ("birth_death6", {"box_pencil": 1}, 7),
             # slabs: BOX_DIMS' repressilator has lines of 31 rows, an odd number; its sibling has lines of 30
             ("repressilator_even", {"box_pencil": 2}, 8), ("birth_death6", {"box_pencil": 2}, 8)]


@pytest.mark.parametrize("name,opts,fmt", BOX_FORMS, ids=[f"{n}-fmt{f}" for n, _, f in BOX_FORMS])
def test_matrix_free_boxes(name, opts, fmt):
    """the interpreted form (3), the single-factor form (4), its LDS window (6), pencils (7) and slabs (8); the rows of
    the restatement are the model's own uploaded arrays"""
    case = K.box_case(name)
    with _ctx(opts) as c:
        case.upload(c)
        assert c.layout_info()["format"] == fmt, c.layout_info()
        r, _, _ = _whole_pass(c, case)
    _done(f"matrix-free format {fmt}", case.name, r)


# ---- partitioned pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind,n,near", [("general", 65, False), ("general", 2049, False), ("general", 4097, False), ("banded", 4097, False),
                                         ("general", 2049, True), ("general", 4097, True), ("banded", 4097, True)])
def test_partitioned_pass(kind, n, near, P):
    """a head over P loop-back ranks: ragged blocks of different parity (65 = 33 + 32 = 22 + 22 + 21), every product
    behind an exchange, every scalar - on the near-invariant siblings a g that matters - finished across the ranks; the
    relation on the gathered columns"""
    from krylovfspssa_amd import host
    case = _get(kind, n, near)
    blocks = [host.partition(n, P, p)[1] for p in range(P)]
    assert sum(blocks) == n and (n % P == 0 or len(set(blocks)) > 1)
    with _ctx(group=P) as c:
        case.upload(c)
        assert c.layout_info()["exchange"] != 0
        r, _, _ = _whole_pass(c, case)
    _done(f"partitioned, {P} ranks", case.name, r)


# ---- stale memory -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("small", [1, 0])
def test_nothing_is_left_from_a_larger_generator(small, near):
    """one context, generators 8193 -> 65 -> 4097 -> 3 -> 4096; before each change a vector of 1e3 goes through a whole
    step on the resident generator, so that w, the basis columns, their pad rows and the partial slots hold large
    numbers where the next, smaller generator has pad rows and fewer partials.  The same through the near-invariant
    siblings (2049 in place of 3), where stale partials of g would show in H(2,2)."""
    with _ctx({"small_kernel": small}) as c:
        for n in ((8193, 65, 4097, 2049, 4096) if near else (8193, 65, 4097, 3, 4096)):
            case = _get("general", n, near)
            case.upload(c)
            r, _, _ = _whole_pass(c, case)
            _done(f"after a larger generator, small_kernel {small}", case.name, r)
            c.set_vector(np.full(n, 1.0e3))
            c.begin_step()
            c.arnoldi(case.m)
            c.combine(case.m + 1, 1.0e3, np.ones(case.m + 1))
            assert c.nrm2_w() > 1.0e3


# ---- combine ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [1, 0])
@pytest.mark.parametrize("n", [65, 4097, 8193])
def test_combine_at_every_remainder(n, small):
    """mx = 1, 2, 3, 4, 5, 7, 8 and all 10 columns of the restarted pass (k_combine takes four columns per trip and
    the rest one by one), y of both signs, beta' != beta, after a pass on each Arnoldi path (n = 65: the one-launch
    kernel with small_kernel = 1)"""
    case = K.general_case(n)
    with _ctx({"small_kernel": small}) as c:
        case.upload(c)
        path = "combine after " + ("one-launch" if small and _one_launch_eligible(c) else "multi-launch")
        c.set_vector(case.w)
        c.begin_step()
        H0, mb, k1, _ = c.arnoldi(K.M_PASS)
        H1 = np.zeros((K.M_LONG + 2, K.M_LONG + 2), order="F")
        H1[:K.M_PASS + 1, :K.M_PASS] = H0[:K.M_PASS + 1, :K.M_PASS]
        _, mb, k1, _ = c.arnoldi(K.M_LONG, jold=K.M_PASS, H=H1)
        assert (mb, k1) == (K.M_LONG, 2)
        basis = _Basis(c)
        r = {}
        for mx in K.COMBINE_MX:
            _combine(c, case, basis, mx, r)
    _done(path, case.name, r)
