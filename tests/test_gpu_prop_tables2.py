"""Two-species propensity tables on the device (kfsp_set_propensity_tables2: prop_tab2 of csrc/kfsp_prop_dev.h behind
prop_eval / prop_eval_light) and the protocol of status -16 - "a population lies beyond a table: nothing the caller can see
has changed, enlarge and repeat" (include/kfsp.h) - against the plain restatement of tests/ssa_ref.py (Program with tables2,
walk, expansion), which tests/test_ssa_ref.py holds to hand-made tables, to its own wrong variants and to the round cap of the
caller's loop on the CPU.  Every comparison is np.array_equal: tables hold what the restated interpreter gives, the walk is
defined bit for bit.

Last, pow and the 14 library functions against correctly rounded values (tests/mp_ref.py): the file-wide bound of
tests/test_gpu_prop.py, 4 ulp, now on populations up to 9 999."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mp_ref as M
from tests import ssa_ref as R
from tests.expand_helpers import onestep_py

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _status(err):
    """the status a refused call returned (KfspError, or what pytest.raises caught: '<call> -> <status>: <text>')"""
    return int(str(getattr(err, "value", err)).split("->")[1].split(":")[0])


def _no_tables2(c, nr):
    """a call of kfsp_set_propensity_tables2 that names no table"""
    none = np.full(nr, -1, dtype=np.int32)
    c.set_propensity_tables2(none, none, np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int64), np.zeros(0))


def _raw_propensities(c, states, nr):
    """kfsp_propensities through the raw ABI with ld_state = ns + 3 (nonsense in the padding) and ld_off = nr + 2; every output
    starts as -7 -> (status, offdiag [n][nr + 2], diag [n])"""
    from krylovfspssa_amd.host import _p
    n, ns = states.shape
    st = np.full((n, ns + 3), 2 ** 30 + 12345, dtype=np.int32)
    st[:, ns + 1] = -9
    st[:, :ns] = states
    off = np.full((n, nr + 2), -7.0)
    diag = np.full(n, -7.0)
    rc = c._lib.kfsp_propensities(c._h, n, _p(st), ns + 3, _p(off), nr + 2, _p(diag))
    return rc, off, diag


def _columns_equal(c, states, nr, want, what):
    rc, off, diag = _raw_propensities(c, states, nr)
    assert rc == 0, (what, rc)
    assert np.array_equal(off[:, :nr], want[0]) and np.array_equal(diag, want[1]), what


@pytest.mark.parametrize("ns", [3, 6, 9])
def test_propensities_with_tables_equal_the_restatement(ns):
    """kfsp_propensities on the models of (a) - chains of 1 to 4 operands, a 5-operand product, three two-species tables
    (n1 != n2, s1 > s2 and s1 < s2, offsets descending with NaN between), a chain with a table it must not read, a one-species
    table read before and beyond its end, a zero divisor - at n = 1, 255, 256, 257, 1025 states (kBlock = 256):
    Program.columns; the same bits from the code once the tables are taken away, by a new program and by a second
    kfsp_set_propensity_tables2 that names no table; tables of extent 4 -> -16, the caller's arrays untouched,
    kfsp_propensity_overflow = the restatement's maxima; the next call with adequate tables is right (the flag was reset)."""
    from krylovfspssa_amd import KfspContext
    prog, code, states = R.columns_model(ns)
    honest = R.columns_model(ns, honest=True)[0]
    small = R.columns_model(ns, extent=4)[0]
    small_honest = R.columns_model(ns, extent=4, honest=True)[0]
    nr = prog.nr
    with KfspContext(0) as c:
        for n in R.COLUMN_SIZES:
            st = states[:n]
            want = prog.columns(st)
            assert not prog.missed
            prog.set_on(c)
            _columns_equal(c, st, nr, want, (n, "tables"))
            code.set_on(c)                                          # kfsp_set_propensity_program alone takes the tables away
            _columns_equal(c, st, nr, want, (n, "code"))
            honest.set_on(c)
            _columns_equal(c, st, nr, want, (n, "tables, honest one-species table"))
            _no_tables2(c, nr)                                      # the second call replaces the first: no table now
            _columns_equal(c, st, nr, want, (n, "second call without a table"))
            small_honest.set_on(c)                                  # (tables too small for these states: were they still live
            _no_tables2(c, nr)                                      # after the second call, this would be a -16)
            _columns_equal(c, st, nr, want, (n, "second call without a table, after small tables"))
            small.set_on(c)
            small.reset_misses()
            small.columns(st)
            rc, off, diag = _raw_propensities(c, st, nr)
            if small.missed:
                assert rc == -16, (n, rc)
                assert (off == -7.0).all() and (diag == -7.0).all(), n
                assert c.propensity_overflow(ns).tolist() == small.miss_max, n
            else:                                                   # (the one state of n = 1 may lie inside the small tables)
                assert rc == 0 and np.array_equal(off[:, :nr], want[0]), n
            prog.set_on(c)
            _columns_equal(c, st, nr, want, (n, "after the miss"))
        assert any(v > 0 for v in small.miss_max)


def test_refusals_of_set_propensity_tables2():
    """no program -> -2, wrong nr -> -2, s1 == s2 / a species >= ns / a zero extent / offset + extent beyond len -> -3; each
    leaves the program and the tables that were there working"""
    from krylovfspssa_amd import KfspContext, KfspError
    prog, _, states = R.columns_model(3)
    st = states[:300]
    want = prog.columns(st)
    s1, s2, n1, n2, off, tab2 = prog.tables2
    k = 5                                                           # a tabulated reaction
    assert s1[k] >= 0

    def changed(which, value):
        a = [np.array(v).copy() for v in (s1, s2, n1, n2, off)]
        a[which][k] = value
        return a + [tab2]

    with KfspContext(0) as c:
        with pytest.raises(KfspError) as err:
            c.set_propensity_tables2(*prog.tables2)
        assert _status(err) == -2                                   # no program
        prog.set_on(c)
        _columns_equal(c, st, prog.nr, want, "first")
        bad = [([a[:-1] for a in (s1, s2, n1, n2, off)] + [tab2], -2),              # wrong nr
               (changed(1, s1[k]), -3), (changed(0, 3), -3), (changed(1, 3), -3), (changed(2, 0), -3), (changed(3, 0), -3),
               (changed(4, len(tab2) - int(n1[k]) * int(n2[k]) + 1), -3), (changed(4, -1), -3)]
        for args, status in bad:
            with pytest.raises(KfspError) as err:
                c.set_propensity_tables2(*args)
            assert _status(err) == status, (status, _status(err))
            _columns_equal(c, st, prog.nr, want, ("after a refusal", status))
        # the largest offset that still fits is accepted
        ok = changed(4, len(tab2) - int(n1[k]) * int(n2[k]))
        c.set_propensity_tables2(*ok)
        assert _raw_propensities(c, st, prog.nr)[0] == 0


# ------------------------------------------------------------------------------------------------------------------
# the walk

def _streams(c, case, prog, general, capacity_new=8192):
    """kfsp_ssa_streams through the raw ABI, every output starting as a sentinel -> (status, count, states, offdiag, diag)"""
    from krylovfspssa_amd.host import _p
    prog.set_on(c)
    for k, v in case.options.items():
        c.set_option(k, v)
    if general:
        c.set_option("ssa_general", 1)
    nr, ns = case.nu.shape
    nf = C.c_int32(777)
    st_new = np.full((capacity_new, ns), -7, dtype=np.int32)
    off_new = np.full((capacity_new, nr), -7.0)
    diag_new = np.full(capacity_new, -7.0)
    rc = c._lib.kfsp_ssa_streams(c._h, case.tstep, case.seedmix, ns, nr, _p(case.nu), len(case.state), _p(case.state), ns, _p(case.adj),
                                 _p(case.off), nr, _p(case.diag), case.max_count, capacity_new, C.byref(nf), _p(st_new), _p(off_new), nr,
                                 _p(diag_new))
    return rc, nf.value, st_new, off_new, diag_new


def _untouched(nf, st_new, off_new, diag_new):
    return nf == 777 and (st_new == -7).all() and (off_new == -7.0).all() and (diag_new == -7.0).all()


def _walk_equal(res, ref, what):
    rc, m, s, o, d = res
    assert rc == 0 and m == ref.nnew, (what, rc, m, ref.nnew)
    assert np.array_equal(s[:m], ref.state_new) and np.array_equal(o[:m], ref.off_new) and np.array_equal(d[:m], ref.diag_new), what
    assert (s[m:] == -7).all() and (d[m:] == -7.0).all(), what


def _overflow_in_bounds(missed, prog, max_count, what):
    """at least one species missed; a missed population lies beyond the smallest table of its species and within max_count"""
    extent = {}
    for a, b, e1, e2 in R.spec_of(prog).values():
        extent[a] = min(extent.get(a, e1), e1)
        extent[b] = min(extent.get(b, e2), e2)
    assert any(m > 0 for m in missed), what
    for s, m in enumerate(missed):
        assert m == 0 or (s in extent and extent[s] <= m <= max_count), (what, s, m)


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("i", range(6))
def test_walk_with_tables_and_the_callers_loop(i, general):
    """kfsp_ssa_streams on the models of (b), through the kernel the dispatch chooses once two-species tables switch the
    register path off (the case's name, asserted from its construction) and through k_ssa_walk_any (ssa_general = 1):
      0 k_ssa_walk<2,4,true,false>   1 k_ssa_walk<6,12,true,false>   2 k_ssa_walk<8,16,true,false>
      3 k_ssa_walk<8,16,false,false> 4 k_ssa_walk_any                5 k_ssa_walk<2,4,true,false> beside a one-species table
    Tables of extent exactly max_count + 1 give the restated walk: no propensity is evaluated at an illegal target, no spurious
    -16.  Tables of extent 4 give -16 with every output as it was; the caller's loop (R.callers_loop: grow by what
    kfsp_propensity_overflow reports, at most ns + ceil(log2(max_count + 1)) rounds) ends with the bits of the tight tables."""
    from krylovfspssa_amd import KfspContext
    tight, small = R.walk2_cases()[i]
    ref = tight.ref
    assert R.walk_kernel(tight) == R.WALK2_KERNELS[i] and ref.first_miss is None and ref.reads2 >= 100
    assert small.ref.first_miss is not None
    ns = tight.nu.shape[1]
    with KfspContext(0) as c:
        _walk_equal(_streams(c, tight, tight.program, general), ref, (tight.name, general))
        rc, *outs = _streams(c, small, small.program, general)
        assert rc == -16 and _untouched(*outs), (small.name, rc)
        _overflow_in_bounds(c.propensity_overflow(ns).tolist(), small.program, small.max_count, small.name)

        def attempt(prog):
            res = _streams(c, small, prog, general)
            if res[0] == -16:
                assert _untouched(*res[1:])
                missed = c.propensity_overflow(ns).tolist()
                _overflow_in_bounds(missed, prog, small.max_count, small.name)
                return None, missed
            return res, None

        res, rounds, _ = R.callers_loop(small, attempt)
        assert rounds >= 1
        _walk_equal(res, ref, (small.name, "after the loop", rounds))


# ------------------------------------------------------------------------------------------------------------------
# the sweep on host lists

def _raw_onestep_columns(c, case, prog):
    from krylovfspssa_amd.host import _p
    prog.set_on(c)
    nr, ns = case.nu.shape
    n = len(case.state)
    cap = n * (nr + 1) + 16
    n_new = C.c_int32(777)
    st_new = np.full((cap - n + 1, ns), -7, dtype=np.int32)
    adj_out = np.full((cap, nr), -7, dtype=np.int32)
    off_new = np.full((cap - n + 1, nr), -7.0)
    diag_new = np.full(cap - n + 1, -7.0)
    rc = c._lib.kfsp_onestep_columns(c._h, ns, nr, _p(case.nu), n, _p(case.state), ns, _p(case.adj), nr, case.max_count, cap,
                                     C.byref(n_new), _p(st_new), _p(adj_out), _p(off_new), nr, _p(diag_new))
    return rc, n_new.value, st_new, adj_out, off_new, diag_new


@pytest.mark.parametrize("i", range(2))
def test_onestep_columns_with_tables(i):
    """kfsp_onestep_columns on the models of (c): the restated sweep with the columns of its states; tables of extent 4 ->
    -16 and nothing written; the caller's loop to the tight tables' answer"""
    from krylovfspssa_amd import KfspContext
    tight, small = R.sweep2_cases()[i]
    n = len(tight.state)
    st2, ad2 = onestep_py(tight.nu, tight.state, tight.adj, tight.max_count)
    o2, d2 = tight.program.columns(st2[n:])
    assert not tight.program.missed and len(st2) > n

    def equal(res, what):
        rc, m, s, a, o, d = res
        assert rc == 0 and m == len(st2), (what, rc, m)
        assert np.array_equal(s[:m - n], st2[n:]) and np.array_equal(a[:m], ad2), what
        assert np.array_equal(o[:m - n], o2) and np.array_equal(d[:m - n], d2), what

    with KfspContext(0) as c:
        equal(_raw_onestep_columns(c, tight, tight.program), tight.name)

        def attempt(prog):
            rc, m, s, a, o, d = res = _raw_onestep_columns(c, small, prog)
            if rc == -16:
                assert m == 777 and (s == -7).all() and (a == -7).all() and (o == -7.0).all() and (d == -7.0).all()
                missed = c.propensity_overflow(tight.nu.shape[1]).tolist()
                _overflow_in_bounds(missed, prog, small.max_count, small.name)
                return None, missed
            return res, None

        res, rounds, _ = R.callers_loop(small, attempt)
        assert rounds >= 1
        equal(res, (small.name, rounds))


# ------------------------------------------------------------------------------------------------------------------
# the expansion on the resident lists

def _expand_cases():
    """(tight, small, t_ssa): the walk models with their horizon, the sweep models without a walk (the sweep misses first)
    and under a horizon of one jump (the columns of the walk's new states miss first)"""
    out = [(t, s, None) for t, s in R.walk2_cases()]
    out += [(t, s, 0.0) for t, s in R.sweep2_cases()]
    out += [(t, s, None) for t, s in R.sweep2_cases()]
    return out


@functools.lru_cache(maxsize=None)
def _expansion_ref(j):
    tight, small, t_ssa = _expand_cases()[j]
    want = R.expansion(tight, t_ssa=t_ssa)
    first = R.expansion(small, t_ssa=t_ssa).first_miss
    return want, first


def _resident(c, case, order, general, w):
    for k, v in case.options.items():
        c.set_option(k, v)
    c.set_option("state_order", order)
    c.set_option("state_order_min", 1)
    c.set_option("state_order_products", 0)
    c.set_option("ssa_general", general)
    c.set_option("keep_coords", 1)
    c.set_state_coords(case.state)
    c.set_matrix_ell(case.adj, case.off, case.diag)
    c.set_vector(w)


def _check_unchanged(c, case, snap, what):
    """after a -16: states, offdiag, diag, n, w and the product are the snapshot's; adj differs only where an open link (0) was
    completed to what the sweep over the first n states alone resolves it to - a listed state or -1"""
    nr, ns = case.nu.shape
    n = len(case.state)
    s0, a0, o0, d0, w0, y0, x = snap
    assert c.n == n, what
    s, a, o, d = c.download_fsp(ns, nr)
    assert np.array_equal(s, s0) and np.array_equal(o, o0) and np.array_equal(d, d0), what
    assert np.array_equal(c.get_vector(), w0) and np.array_equal(c.spmv(x), y0), what
    full = onestep_py(case.nu, s0, a0, case.max_count)[1][:n]
    allowed = np.where((a0 == 0) & (full <= n), full, a0)           # (a link to a state the sweep would append stays open)
    assert (a <= n).all() and (a != -2).all(), what
    assert (((a == a0) | (a == allowed))).all(), what


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("j", range(10))
def test_expand_resident_with_tables(j, order):
    """kfsp_expand_resident on (b) and (c): the three places it can return -16 - the walk (cases 0-5), the sweep's new columns
    (6, 7: no walk), the columns of the walk's new states (8, 9: every path ends at its first jump) - each as the restatement
    names it.  Tight tables: the restated walk, then onestep_py, then Program.columns.  Extent 4: -16 and the resident FSP as
    it was (_check_unchanged); then the caller's loop, whose final lists and vector are the tight tables'."""
    from krylovfspssa_amd import KfspContext, KfspError
    tight, small, t_ssa = _expand_cases()[j]
    want, first = _expansion_ref(j)
    assert want.first_miss is None and first == ("walk" if j < 6 else "sweep" if j < 8 else "columns"), (j, first)
    nr, ns = tight.nu.shape
    n = len(tight.state)
    general = (j + order) % 2
    t = tight.tstep if t_ssa is None else t_ssa
    w = np.random.default_rng(5 + j).random(n)
    x = np.random.default_rng(50 + j).random(n)

    def final(c, what):
        assert c.n == len(want.state), what
        s, a, o, d = c.download_fsp(ns, nr)
        assert np.array_equal(s, want.state) and np.array_equal(a, want.adj), what
        assert np.array_equal(o, want.off) and np.array_equal(d, want.diag), what
        assert np.array_equal(c.get_vector(), np.concatenate([w, np.zeros(len(want.state) - n)])), what

    with KfspContext(0) as c:
        tight.program.set_on(c)
        _resident(c, tight, order, general, w)
        n2, nssa = c.expand_resident(t, tight.seedmix, tight.nu, max_count=tight.max_count)
        assert (n2, nssa) == (len(want.state), want.nssa), tight.name
        final(c, tight.name)
    with KfspContext(0) as c:
        small.program.set_on(c)
        _resident(c, small, order, general, w)
        snap = c.download_fsp(ns, nr) + (c.get_vector(), c.spmv(x), x)
        assert c.n == n and np.array_equal(snap[0], small.state) and np.array_equal(snap[1], small.adj)

        def attempt(prog):
            prog.set_on(c)
            try:
                return c.expand_resident(t, small.seedmix, small.nu, max_count=small.max_count), None
            except KfspError as err:
                assert _status(err) == -16, str(err)
            missed = c.propensity_overflow(ns).tolist()
            _overflow_in_bounds(missed, prog, small.max_count, small.name)
            _check_unchanged(c, small, snap, (small.name, missed))
            return None, missed

        (n2, nssa), rounds, _ = R.callers_loop(small, attempt)
        assert rounds >= 1 and (n2, nssa) == (len(want.state), want.nssa), (small.name, rounds)
        final(c, (small.name, rounds))


@pytest.mark.parametrize("partition", [1, 0])
def test_expand_resident_with_tables_under_three_ranks(partition):
    """three loop-back ranks on the 300-seed case: with ssa_partition = 1 rank 0 walks nothing, rank 1 the wavefront whose seeds
    cannot leave the small table, rank 2 the one whose seeds do (tests/test_ssa_ref.py) - every rank must return -16 with the
    same kfsp_propensity_overflow, and after growing hold the restatement's lists"""
    from krylovfspssa_amd import KfspError, host
    small, tight = R.share_case(True), R.share_case(False)
    want = R.expansion(tight)
    assert want.first_miss is None and small.ref.first_miss == "walk"
    nr, ns = small.nu.shape
    n = len(small.state)

    def body(c, rank):
        small.program.set_on(c)
        c.set_option("ssa_partition", partition)
        c.set_option("state_order", 0)
        c.set_option("keep_coords", 1)
        c.set_state_coords(small.state)
        c.set_matrix_ell(small.adj, small.off, small.diag)
        r0, nloc = c.row_block(n)
        c.set_vector(np.full(nloc, 1.0 / n))
        seen = []

        def attempt(prog):
            prog.set_on(c)
            try:
                return c.expand_resident(small.tstep, small.seedmix, small.nu, max_count=small.max_count), None
            except KfspError as err:
                assert _status(err) == -16, str(err)
            seen.append(c.propensity_overflow(ns).tolist())
            return None, seen[-1]

        (n2, nssa), rounds, _ = R.callers_loop(small, attempt)
        return (n2, nssa, rounds, seen) + tuple(c.download_fsp(ns, nr))

    res = host.run_loopback_ranks(3, body)
    for rank, (n2, nssa, rounds, seen, s_r, a_r, o_r, d_r) in enumerate(res):
        assert rounds >= 1 and seen == res[0][3], (rank, seen, res[0][3])
        assert (n2, nssa) == (len(want.state), want.nssa), rank
        assert np.array_equal(s_r, want.state) and np.array_equal(a_r, want.adj), rank
        assert np.array_equal(o_r, want.off) and np.array_equal(d_r, want.diag), rank


def test_one_context_through_a_sequence_of_programs():
    """a program with tables, a miss, larger tables, another program with fewer reactions and no tables, the first program
    again: nothing of an earlier step - table buffers, offsets, the missed populations - may show in a later one"""
    from krylovfspssa_amd import KfspContext
    tight, small = R.walk2_cases()[1]                               # 6 species, 12 reactions
    other = R.variant_cases()[4]                                    # 2 species, 3 reactions, no table
    ns = tight.nu.shape[1]
    prog, _, states = R.columns_model(6)
    with KfspContext(0) as c:
        _walk_equal(_streams(c, tight, tight.program, 0), tight.ref, "tables")
        rc, *outs = _streams(c, small, small.program, 0)
        assert rc == -16 and _untouched(*outs)
        missed = c.propensity_overflow(ns).tolist()
        grown = R.with_tables2(small.plain, R.grow_spec(R.spec_of(small.program), missed, small.max_count))
        res = _streams(c, small, grown, 0)
        if res[0] == 0:
            _walk_equal(res, tight.ref, "larger tables")
        else:
            assert res[0] == -16 and _untouched(*res[1:])
            missed = c.propensity_overflow(ns).tolist()
        _walk_equal(_streams(c, other, other.program, 0), other.ref, "fewer reactions, no tables")
        rc, off, diag = _raw_propensities(c, other.state, other.nu.shape[0])
        assert rc == 0 and np.array_equal(off[:, :3], other.off) and np.array_equal(diag, other.diag)
        assert c.propensity_overflow(ns).tolist() == missed          # (what the LAST -16 left; no later call raised another)
        _walk_equal(_streams(c, tight, tight.program, 0), tight.ref, "the first program again")
        prog.set_on(c)                                              # and a third program with other tables of the same species count
        _columns_equal(c, states[:257], prog.nr, prog.columns(states[:257]), "columns model")
        _walk_equal(_streams(c, tight, tight.program, 1), tight.ref, "the first program, general kernel")


# ------------------------------------------------------------------------------------------------------------------
# library functions

def _ulps(a, b):
    return np.abs(a - b) / (EPS * np.maximum(np.abs(b), np.finfo(np.float64).tiny))


def test_library_functions_against_correctly_rounded_values():
    """pow and the 14 functions, one call per expression on an argument that is exact in binary64, two species on a 40 x 40
    lattice of populations 0 .. 9 999, against mpmath at 100 digits rounded to nearest (tests/mp_ref.py): within the 4 ulp of
    tests/test_gpu_prop.py (measured in units of eps |reference|, as there), and the rules that zero an expression agree
    exactly.  The worst case of each function is printed; DESIGN 11.2 records them."""
    from krylovfspssa_amd import KfspContext
    ex = M.expressions()
    states = M.lattice()
    want = M.reference(states)
    with KfspContext(0) as c:
        c.set_propensity_program(2, [], [(code, imm) for _, code, imm, _ in ex])
        off, diag = c.propensities(states)
    worst = {}
    for j, (name, _, _, _) in enumerate(ex):
        u = _ulps(off[:, j], want[:, j])
        i = int(np.argmax(u))
        worst[name] = (float(u[i]), tuple(states[i].tolist()))
        print(f"{name:9s} worst {u[i]:.3f} ulp at (x, y) = {tuple(states[i].tolist())}")
    for j, (name, _, _, _) in enumerate(ex):
        assert np.array_equal(off[:, j] == 0.0, want[:, j] == 0.0), name
        assert np.isfinite(off[:, j]).all(), name
        assert worst[name][0] <= 4.0, (name, worst[name])
    assert worst["abs"][0] == 0.0 and worst["sqrt"][0] == 0.0          # exact operations
    d = np.zeros(len(states))
    for j in range(len(ex)):
        d = d + off[:, j]
    assert np.array_equal(diag, d)
