"""DROP_STATES on the device (kfsp_drop_plan / _flags / _compact / _rebuild) against tests/drop_ref.py at its edges
(DESIGN.md 9).  Every assertion is exact: the same double for droptol, equal integers, equal flag bytes, bit-equal vectors
and lists; no state is left out as "near".  That is possible because of how the inputs are made (tests/drop_ref.py): sums
of dyadic small entries are exact in any order, and a generator with one 1.0 per row moves w without rounding; the general
generators of the form cases satisfy the two margin conditions, which tests/test_drop_ref.py asserts on the CPU - together
with the proof that each case tells the mistakes it is there for from the right answer."""
import numpy as np
import pytest

from tests import box_cases as BC
from tests import drop_ref as D
from tests import row_cases as RC

pytestmark = pytest.mark.gpu


def _ctx(group=None, **options):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0, group=group)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def _order_options(order):
    return dict(keep_coords=1, state_order=order, state_order_min=1, state_order_products=0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {bad.size} entries differ on the bits, first {bad[:5]}"


def _upload(c, case, order=0, coords=None):
    """-> the coordinates handed over (ell) or None"""
    if case["kind"] == "ell":
        coords = RC.made_up_coords(case["n"]) if coords is None else coords
        c.set_state_coords(coords)
        c.set_matrix_ell(case["adj"], case["off"], case["diag"])
        assert c.state_order_active() == bool(order)
        assert c.layout_info()["format"] in (0, 5)
        return coords
    c.set_matrix_csr(case["n"], case["rowptr"], case["col"], case["val"])
    if case["n"] > 1:
        assert c.layout_info()["format"] in (1, 2)
    return None


def _plan(c, w, dsum, want, what):
    """set_vector, drop_plan, drop_flags against expected()"""
    c.set_vector(w)
    _check_plan(c, dsum, want, what)


def _check_plan(c, dsum, want, what):
    tol, count, nflag = c.drop_plan(dsum)
    assert tol == want["tol"], (what, tol, want["tol"])
    assert (count, nflag) == (want["count"], want["nflag"]), (what, count, nflag, want["count"], want["nflag"])
    flags = c.drop_flags()
    bad = np.flatnonzero(flags != want["drop"].astype(np.uint8))
    assert bad.size == 0, f"{what}: {bad.size} flag bytes differ, first {bad[:5]}"


def _lists_are(c, ns, nr, lists, what):
    s, a, o, d = c.download_fsp(ns, nr)
    s2, a2, o2, d2 = lists
    assert np.array_equal(s, s2) and np.array_equal(a, a2), what
    assert np.array_equal(_bits(o), _bits(o2)) and np.array_equal(_bits(d), _bits(d2)), what


# ---- (a) every remainder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("n", D.REMAINDERS)
def test_every_remainder_on_sell(n, order):
    """set_matrix_ell of the cycle generator, the device's own state order off and on (coordinates whose lexicographic order is
    a random permutation of the caller's): plan and flags; then drop_compact and either the upload of the compacted lists or
    drop_rebuild, whose lists must be compact_lists' and whose vector the compacted one, on the bits (with -0.0, the
    smallest subnormal and the entries next to the thresholds among them)"""
    case = D.perm_case("ell", n)
    nk = n - case["nflag"]
    for rebuild in (False, True):
        what = f"sell, n={n}, state order {order}, {'rebuild' if rebuild else 'upload'}"
        with _ctx(format=1, **_order_options(order)) as c:
            coords = _upload(c, case, order)
            _plan(c, case["w"], case["dsum"], case, what)
            assert c.drop_compact() == nk
            s2, a2, o2, d2, w2 = D.compact_lists(coords, case["adj"], case["off"], case["diag"], case["w"], case["keep"])
            if rebuild:
                c.drop_rebuild()
            else:
                c.set_state_coords(s2)
                c.set_matrix_ell(a2, o2, d2)
            assert c.n == nk and c.state_order_active() == bool(order)
            _same_bits(c.get_vector(), w2, what)
            _lists_are(c, 2, 2, (s2, a2, o2, d2), what)
            # the generator that came of it moves w2 like the restatement does
            aw2 = D.moved(w2, D.sources_ell(a2))
            got = c.spmv_w()
            assert np.array_equal(got, aw2), what
            nz = aw2 != 0.0
            assert np.array_equal(_bits(got[nz]), _bits(aw2[nz])), what


@pytest.mark.parametrize("n", D.REMAINDERS)
def test_every_remainder_on_banded(n):
    """set_matrix_csr of the one-diagonal generator (a CSR upload has no internal state order): plan, flags, drop_compact,
    and the compacted vector under the generator of the smaller FSP"""
    case = D.perm_case("csr", n)
    nk = n - case["nflag"]
    what = f"banded, n={n}"
    with _ctx() as c:
        _upload(c, case)
        _plan(c, case["w"], case["dsum"], case, what)
        assert c.drop_compact() == nk
        c.set_matrix_csr(nk, *D.shift_csr(nk))
        assert c.n == nk
        _same_bits(c.get_vector(), case["w"][case["keep"]], what)


# ---- (b) the loops turn --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,order", [("ell", 0), ("ell", 1), ("csr", 0)])
def test_grid_stride_loops_take_a_second_turn(kind, order):
    """262 209 states: k_drop_flags (512 x 256 lanes), k_keep_from_drop, k_flags_to_caller and the select (1024 x 256) all
    go round again, and the specials of the last rows lie in the second turn"""
    case = D.perm_case(kind, D.N_TURN)
    n, nk = case["n"], case["n"] - case["nflag"]
    what = f"{kind}, n={n}, state order {order}"
    with _ctx(**(dict(format=1, **_order_options(order)) if kind == "ell" else {})) as c:
        _upload(c, case, order)
        _plan(c, case["w"], case["dsum"], case, what)
        assert c.drop_compact() == nk
        if kind == "ell":
            c.drop_rebuild()
        else:
            c.set_matrix_csr(nk, *D.shift_csr(nk))
        assert c.n == nk
        _same_bits(c.get_vector(), case["w"][case["keep"]], what)


@pytest.mark.parametrize("vgrid", [1, 3])
@pytest.mark.parametrize("kind", ["ell", "csr"])
def test_threshold_sums_on_a_forced_small_grid(kind, vgrid):
    """vec_grid_blocks 1 and 3 at 8193 states: k_drop_sums strides 256 / 768 pairs over 4128, k_drop_finish sums 1 / 3 partials"""
    case = D.perm_case(kind, D.N_GRID)
    with _ctx(vec_grid_blocks=vgrid, **(dict(format=1, **_order_options(0)) if kind == "ell" else {})) as c:
        _upload(c, case)
        _plan(c, case["w"], case["dsum"], case, f"{kind}, vec_grid_blocks={vgrid}")


# ---- (c) threshold batches and the decision at the edge ---------------------------------------------------------------------
@pytest.mark.parametrize("name", D.BATCH_NAMES)
def test_threshold_batches_and_edges(name):
    """dsum met at the 1st, 16th, 17th and 33rd level; nothing positive at all; positive entries only ON thresholds; and
    exact sums with dsum == S_5 (the search moves on) and one unit in the last place above (it stops)"""
    case = D.batch_case(name)
    with _ctx() as c:
        c.set_matrix_csr(case["n"], *D.shift_csr(case["n"]))
        _plan(c, case["w"], case["dsum"], case, name)
        _same_bits(c.get_vector(), case["w"], name)              # a plan leaves the vector alone


# ---- (d) stale memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["set_vector", "set_matrix_ell", "drop_rebuild"])
@pytest.mark.parametrize("r", D.STALE_R)
def test_nothing_is_left_from_a_larger_generator(r, route):
    """8193 states, 1e-12 everywhere, one whole step; then 4097 + r states arrive by each of the three routes a vector can
    take, and drop_plan answers what the restatement - and a fresh context - answers.  k_drop_sums reads the 63, 62 and 1 rows
    up to the next multiple of 64 as well; dsum2 is so close above the exact S_0 that a single small entry left in any of
    them moves the threshold from 1e-8 to 1e-13 (tests/test_drop_ref.py, with what each route would leave there: the step's
    1e-12 under kfsp_set_vector, small entries of W under the vector adopted after kfsp_drop_compact)"""
    case = D.stale_case(r)
    n, n2 = case["n"], case["n2"]
    what = f"r={r}, {route}"
    with _ctx(format=1, small_kernel=0, **_order_options(0)) as c:
        coords = RC.made_up_coords(n)
        c.set_state_coords(coords)
        c.set_matrix_ell(case["adj"], case["off"], case["diag"])
        c.set_vector(np.full(n, D.STALE_FILL))
        beta = c.begin_step()
        c.arnoldi(4)
        c.combine(1, beta, np.ones(1))
        left = c.get_vector()[n2:n2 + case["pad"]]               # the rows that become pad rows of the smaller FSP
        assert ((left > 2 ** 10 * D.UNIT) & (left < D.TOL0)).all()
        if route == "set_vector":
            c.set_state_coords(coords[case["first"]["keep"]])
            c.set_matrix_ell(case["adj2"], case["off2"], case["diag2"])
            c.set_vector(case["w2"])
        else:
            _plan(c, case["W"], case["dsum1"], case["first"], what + ", first plan")
            _same_bits(c.get_vector()[n2:n2 + case["pad"]], case["stale_pending"], what)
            assert c.drop_compact() == n2
            if route == "drop_rebuild":
                c.drop_rebuild()
            else:
                c.set_state_coords(coords[case["first"]["keep"]])
                c.set_matrix_ell(case["adj2"], case["off2"], case["diag2"])
        assert c.n == n2
        _same_bits(c.get_vector(), case["w2"], what)
        _check_plan(c, case["dsum2"], case["second"], what)
        got = (c.drop_plan(case["dsum2"]), c.drop_flags().tobytes())
    with _ctx(format=1) as fresh:
        fresh.set_matrix_ell(case["adj2"], case["off2"], case["diag2"])
        fresh.set_vector(case["w2"])
        assert (fresh.drop_plan(case["dsum2"]), fresh.drop_flags().tobytes()) == got, what


# ---- (e) every generator form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.FORMS))
def test_every_generator_form(name):
    """A w comes from spmv_plain whatever form the generator is resident in: the product is the restated row on the bits,
    so flags and counts are decide()'s"""
    case = D.form_case(name)
    fmt, coded, folded = case["form"]
    with _ctx(small_kernel=0, **case["options"]) as c:
        if case["how"] == "csr":
            c.set_matrix_csr(case["n"], case["rowptr"], case["col"], case["val"])
        elif case["how"] == "ell":
            c.set_matrix_ell(case["adj"], case["off"], case["diag"])
        else:
            c.set_matrix_box(case["mdl"], store=case["how"] == "box_store")
        info, ci = c.layout_info(), c.dia_code_info()
        print(f"\n{name}: format {info['format']}, coded {ci['active']}, diag tables {ci['diag_table_bytes']} B, "
              f"coded chunks {info['coded_chunks']}")
        if case["how"] == "box_store":
            assert info["format"] in (1, 2) and c.matrix_info()["slots"] > 0, (name, info)
        else:
            assert info["format"] == fmt, (name, info)
        assert ci["active"] == coded and (ci["diag_table_bytes"] > 0) == folded, (name, ci)
        if name == "sell coded":
            assert info["coded_chunks"] > 0
        c.set_vector(case["w"])
        bad = BC.mismatches(c.spmv_w(), case["aw"])
        assert bad.size == 0, f"{name}: {bad.size} rows of A w differ from the restatement, first {bad[:5]}"
        _check_plan(c, case["dsum"], case, name)


# ---- (f) partitions -----------------------------------------------------------------------------------------------------------
PARTITIONED = [("csr", 1), ("csr", 0), ("ell", 1), ("ell", 0)]


def _exchange_is(info, kind, halo, n, what):
    """kfsp_layout_info: 1 halo strips, 2 all-gather.  The banded generator reaches one row: strips of 8 rows.  The SELL
    cycle reaches as far as its random part: within one block of 64 rows at n = 65 (strips of 64 rows), across blocks at
    n = 449 (all-gather)"""
    if not halo:
        want = (2, 0)
    elif kind == "csr":
        want = (1, 8)
    else:
        want = (1, 64) if n == 65 else (2, 0)
    assert (info["exchange"], info["halo_rows"]) == want, (what, info)


@pytest.mark.parametrize("kind,halo", PARTITIONED)
@pytest.mark.parametrize("P", D.PARTITION_P)
@pytest.mark.parametrize("n", D.PARTITION_N)
def test_head_of_a_partition(n, P, kind, halo):
    """a group head over P loop-back ranks: the banded generator with halo strips (drop_plan stages w in the scratch column)
    and with the all-gather, the SELL generator with either setting.  n = 65: trailing ranks own no rows.  Plan, flags of all
    states, and the compacted vector in the partition of the smaller FSP"""
    case = D.perm_case(kind, n)
    nk = n - case["nflag"]
    what = f"{kind}, halo={halo}, n={n}, P={P}"
    with _ctx(group=P, halo=halo, **(dict(format=1, **_order_options(0)) if kind == "ell" else {})) as c:
        coords = _upload(c, case)
        info = c.layout_info()
        print(f"\n{what}: exchange {info['exchange']}, halo rows {info['halo_rows']}")
        _exchange_is(info, kind, halo, n, what)
        _plan(c, case["w"], case["dsum"], case, what)
        assert c.drop_compact() == nk
        if kind == "ell":
            c.drop_rebuild()
            s2, a2, o2, d2, _ = D.compact_lists(coords, case["adj"], case["off"], case["diag"], None, case["keep"])
            _lists_are(c, 2, 2, (s2, a2, o2, d2), what)
        else:
            c.set_matrix_csr(nk, *D.shift_csr(nk))
        assert c.n == nk
        _same_bits(c.get_vector(), case["w"][case["keep"]], what)


@pytest.mark.parametrize("kind,halo", PARTITIONED)
@pytest.mark.parametrize("P", D.PARTITION_P)
@pytest.mark.parametrize("n", D.PARTITION_N)
def test_every_rank_reports_the_same(n, P, kind, halo):
    """P = 2, 3 and 4 ranks, each driven by its own thread: every rank returns the same droptol, count, number of flags and the flags of
    ALL states - also the ranks without rows (n = 65: blocks of 64, 1, 0 and 0 rows over four ranks) -, and afterwards holds its block of the
    compacted vector in the new partition"""
    from krylovfspssa_amd.host import run_loopback_ranks
    case = D.perm_case(kind, n)
    nk = n - case["nflag"]
    w2 = case["w"][case["keep"]]
    what = f"{kind}, halo={halo}, n={n}, P={P}"

    def body(c, rank):
        c.set_option("halo", halo)
        if kind == "ell":
            for k, v in dict(format=1, **_order_options(0)).items():
                c.set_option(k, v)
            c.set_state_coords(RC.made_up_coords(n))
            c.set_matrix_ell(case["adj"], case["off"], case["diag"])
        else:
            row0, nloc = c.row_block(n)
            c.set_matrix_csr(n, *D.shift_csr(n, row0, nloc))
        info = c.layout_info()
        first = (c.row0, c.nloc)
        c.set_vector(case["w"][c.row0:c.row0 + c.nloc])
        plan = c.drop_plan(case["dsum"])
        flags = c.drop_flags()
        n_new = c.drop_compact()
        if kind == "ell":
            c.drop_rebuild()
        else:
            row0, nloc = c.row_block(nk)
            c.set_matrix_csr(nk, *D.shift_csr(nk, row0, nloc))
        return dict(info=info, first=first, plan=plan, flags=flags, n_new=n_new, block=(c.row0, c.nloc), w=c.get_vector())

    out = run_loopback_ranks(P, body)
    assert sum(o["first"][1] for o in out) == n and sum(o["block"][1] for o in out) == nk
    if n == 65:
        assert [o["first"][1] for o in out] == [64, 1, 0, 0][:P]
    for rank, o in enumerate(out):
        _exchange_is(o["info"], kind, halo, n, f"{what}, rank {rank}")
        assert o["plan"] == (case["tol"], case["count"], case["nflag"]), (what, rank, o["plan"])
        assert np.array_equal(o["flags"], case["drop"].astype(np.uint8)), (what, rank)
        assert o["n_new"] == nk
        row0, nloc = o["block"]
        _same_bits(o["w"], w2[row0:row0 + nloc], f"{what}, rank {rank}")


# ---- (g) extremes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.EXTREMES[:3])
def test_extremes_of_the_compaction(name):
    """nothing flagged (drop_compact returns n and the vector keeps its bits), all but the first, all but the last"""
    case = D.extreme_case(name)
    n, nk = case["n"], case["n"] - case["nflag"]
    assert nk == (n if name == "nothing" else 1)
    coords = RC.made_up_coords(n)
    s2, a2, o2, d2, w2 = D.compact_lists(coords, case["adj"], case["off"], case["diag"], case["w"], case["keep"])
    for order in (0, 1):
        for rebuild in (False, True):
            what = f"{name}, state order {order}, {'rebuild' if rebuild else 'upload'}"
            with _ctx(format=1, **_order_options(order)) as c:
                c.set_state_coords(coords)
                c.set_matrix_ell(case["adj"], case["off"], case["diag"])
                _plan(c, case["w"], case["dsum"], case, what)
                assert c.drop_compact() == nk
                if rebuild:
                    c.drop_rebuild()
                else:
                    c.set_state_coords(s2)
                    c.set_matrix_ell(a2, o2, d2)
                assert c.n == nk
                _same_bits(c.get_vector(), w2, what)
                _lists_are(c, 2, 2, (s2, a2, o2, d2), what)


@pytest.mark.parametrize("n_next", [65, 4097])
def test_everything_flagged(n_next):
    """Every state dropped: drop_compact answers 0, drop_rebuild refuses (-9: there is no FSP of 0 states to rebuild), and the
    context takes whatever generator comes next - smaller or larger than any before - with w = 0, then a vector, and
    multiplies correctly.  (Before this was pinned the first generator after such a compaction was refused with -2: the
    pending vector of 0 states matched no generator.)"""
    from krylovfspssa_amd import KfspError
    case = D.extreme_case("everything")
    nxt = D.perm_case("ell", n_next)
    with _ctx(format=1, **_order_options(0)) as c:
        c.set_state_coords(RC.made_up_coords(case["n"]))
        c.set_matrix_ell(case["adj"], case["off"], case["diag"])
        _plan(c, case["w"], case["dsum"], case, "everything")
        assert case["nflag"] == case["n"] and c.drop_compact() == 0
        with pytest.raises(KfspError, match="-9"):
            c.drop_rebuild()
        with pytest.raises(KfspError, match="-1"):
            c.drop_flags()                                       # the plan is spent
        c.set_matrix_ell(nxt["adj"], nxt["off"], nxt["diag"])
        assert c.n == n_next and not c.get_vector().any()
        _plan(c, nxt["w"], nxt["dsum"], nxt, f"after everything was flagged, n={n_next}")
        got = c.spmv(nxt["w"])
        assert np.array_equal(got, nxt["aw"])


# ---- (h) renumbering ---------------------------------------------------------------------------------------------------------
def _raw_upload(c, f, state, adj, off):
    """kfsp_set_state_coords / kfsp_set_matrix_ell with the leading dimensions of the padded arrays"""
    from krylovfspssa_amd.host import _p
    n = f["n"]
    state, adj, off = (np.ascontiguousarray(a) for a in (state, adj, off))
    diag = np.ascontiguousarray(f["diag"])
    c._chk(c._lib.kfsp_set_state_coords(c._h, n, f["ns"], state.shape[1], _p(state)), "kfsp_set_state_coords")
    c._chk(c._lib.kfsp_set_matrix_ell(c._h, n, f["nr"], adj.shape[1], _p(adj), _p(off), _p(diag)), "kfsp_set_matrix_ell")
    c.n = n
    c.row0, c.nloc = c.row_block(n)


def _raw_download(c, n, lds, ld):
    from krylovfspssa_amd.host import _p
    state = np.zeros((n, lds), dtype=np.int32)
    adj = np.zeros((n, ld), dtype=np.int32)
    off = np.zeros((n, ld))
    diag = np.zeros(n)
    c._chk(c._lib.kfsp_download_fsp(c._h, n, _p(state), lds, _p(adj), _p(off), ld, _p(diag)), "kfsp_download_fsp")
    return state, adj, off, diag


def test_renumbering_on_random_fsps():
    """100 random small FSPs through ONE context (each arrives where another was), keep patterns random, first kept / last
    dropped, alternating and a kept block in the middle, the state order off and on in turn: flags are the complement of the
    pattern, drop_rebuild + download_fsp give compact_lists, the vector is compacted, and the rebuilt generator multiplies
    like a fresh upload of the compacted lists, bit for bit.  Every fourth FSP goes through the raw ABI with ld_adj = nr + 3
    and ld_state = ns + 2 and nonsense - positive 'links' among it - in the padding, which must come back untouched."""
    fsps = D.random_fsps()
    rng = np.random.default_rng(4)
    with _ctx(keep_coords=1, state_order_min=1, state_order_products=0) as c, _ctx(state_order=0) as fresh:
        for j, f in enumerate(fsps):
            what = f"FSP {j} ({f['pattern']}, n={f['n']}, ns={f['ns']}, nr={f['nr']})"
            n, ns, nr, keep = f["n"], f["ns"], f["nr"], f["keep"]
            nk = int(keep.sum())
            c.set_option("state_order", (j // 4) % 2)
            want = dict(tol=D.threshold(D.LEVEL), drop=~keep, nflag=n - nk, count=n - nk)     # (nothing is guarded)
            if j % 4 == 3:
                state = D.padded(f["state"], ns + 2, D.PAD_STATE)
                adj = D.padded(f["adj"], nr + 3, D.PAD_ADJ)
                off = D.padded(f["off"], nr + 3, D.PAD_OFF)
                _raw_upload(c, f, state, adj, off)
            else:
                state, adj, off = f["state"], f["adj"], f["off"]
                c.set_state_coords(state)
                c.set_matrix_ell(adj, off, f["diag"])
            _plan(c, f["w"], f["dsum"], want, what)
            assert c.drop_compact() == nk
            c.drop_rebuild()
            assert c.n == nk
            s2, a2, o2, d2, w2 = D.compact_lists(state, adj, off, f["diag"], f["w"], keep, nr=nr)
            _same_bits(c.get_vector(), w2, what)
            s, a, o, d = _raw_download(c, nk, state.shape[1], adj.shape[1])
            assert np.array_equal(s, s2) and np.array_equal(a, a2), what
            assert np.array_equal(_bits(o), _bits(o2)) and np.array_equal(_bits(d), _bits(d2)), what
            x = rng.standard_normal(nk)
            fresh.set_matrix_ell(a2[:, :nr], o2[:, :nr], d2)
            assert np.array_equal(_bits(c.spmv(x)), _bits(fresh.spmv(x))), what
