"""tests/row_ref.py, the plain restatement of one row of the product, checked without a device: against row sums in
extended precision, against the oracle's product at the tolerance the device tests use - and that every case of
tests/test_gpu_build_rows.py can tell a wrong order from the right one (a comparison of bits that no wrong order
would change proves nothing).  The same for the forward matrix-free rows (box_exact, box_generic_exact) and the
cases of tests/test_gpu_box_rows.py."""
from fractions import Fraction

import numpy as np
import pytest

from tests import adjoint_cases as AC
from tests import box_cases as BC
from tests import row_cases as RC
from tests import row_ref as RR
from tests.test_block_adjoint_host import banded_form, banded_t, bound, box_t, ell_t


def _changed(case, rows):
    """rows whose bits change when `rows` are summed instead of the case's"""
    y = np.array(RR.spmv_exact(rows, case["diag"], case["x"]))
    return int((RC.bits(y) != RC.bits(case["y"])).sum())


def _longdouble(rows, diag, x):
    ld = np.longdouble
    y = np.array([sum((ld(v) * ld(x[c]) for c, v in row), ld(0)) - ld(diag[r]) * ld(x[r]) for r, row in enumerate(rows)])
    mag = np.array([sum(abs(v * x[c]) for c, v in row) + abs(diag[r] * x[r]) for r, row in enumerate(rows)])
    return y, mag


def test_fma_rounds_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30           # a * b = 1 - 2^-60: rounds to 1, so a * b - 1 == 0 in two steps
    assert a * b - 1.0 == 0.0 and RR.fma(a, b, -1.0) == -(2.0 ** -60)
    assert 0.1 * 10.0 - 1.0 == 0.0 and RR.fma(0.1, 10.0, -1.0) == 2.0 ** -54      # the double 0.1 is 2^-54 / 10 above a tenth


def test_rows_are_gathered_in_the_promised_order():
    # states 1..4; state 3 links twice to state 1 (values 5 and 2), state 2 links to state 1, state 4 to itself
    adj = [[0, 3], [1, -1], [1, 1], [4, 0]]
    off = [[9.0, 7.0], [4.0, 9.0], [5.0, 2.0], [6.0, 9.0]]
    rows = RR.gather_rows(adj, off, [0.0] * 4)
    assert rows == [[(1, 4.0), (2, 2.0), (2, 5.0)], [], [(0, 7.0)], [(3, 6.0)]]
    assert RR.gather_rows(adj, off, [0.0] * 4, row0=2, nloc=2) == rows[2:]
    # equal source and value: the slot decides (shown through the sort key, the pairs are the same)
    assert RR.gather_rows([[2, 2], [0, 0]], [[3.0, 3.0], [1.0, 1.0]], [0.0, 0.0])[1] == [(0, 3.0), (0, 3.0)]
    r, d = RR.rows_from_csr(3, [0, 2, 4, 6], [0, 2, 0, 1, 1, 2], [-1.5, 2.0, 3.0, -4.0, 5.0, -6.0])
    assert r == [[(2, 2.0)], [(0, 3.0)], [(1, 5.0)]] and d == [1.5, 4.0, 6.0]
    y = RR.spmv_exact(r, d, [1.0, 10.0, 100.0])
    assert y == [198.5, -37.0, -550.0]
    assert RR.spmv_exact(r[1:], d[1:], [1.0, 10.0, 100.0], row0=1) == y[1:]


@pytest.mark.parametrize("name", list(RC.ELL))
def test_restatement_against_extended_precision_and_the_oracle(oracle, name):
    c = RC.ell_case(name)
    y_ld, mag = _longdouble(c["rows"], c["diag"], c["x"])
    assert np.all(np.abs(c["y"] - y_ld) <= 1e-15 * mag)
    A = oracle.EllMatrix(c["adj"], c["off"], c["diag"])
    assert sum(len(r) for r in c["rows"]) + c["n"] == A.nnz()
    ref = oracle.spmv_ell(A, c["x"])
    scale = oracle.spmv_ell(oracle.EllMatrix(c["adj"], np.abs(c["off"]), -np.abs(c["diag"])), np.abs(c["x"]))
    assert np.all(np.abs(c["y"] - ref) <= 1e-13 * scale + 1e-300)
    # inputs in the range where nothing is subnormal
    assert np.abs(c["off"][c["adj"] > 0]).min() * np.abs(c["x"]).min() > 1e-30
    assert np.abs(c["off"]).max() < 1e3 and np.abs(c["diag"]).max() < 1e3 and np.abs(c["x"]).max() < 1e3


@pytest.mark.parametrize("name", RC.CSR)
def test_restatement_of_csr_rows_against_extended_precision(oracle, name):
    c = RC.csr_case(name)
    y_ld, mag = _longdouble(c["rows"], c["diag"], c["x"])
    assert np.all(np.abs(c["y"] - y_ld) <= 1e-15 * mag)
    ref = oracle.spmv_csr(c["rowptr"], c["col"], c["val"], c["x"])
    assert np.all(np.abs(c["y"] - ref) <= 1e-13 * mag + 1e-300)


# ---- every device case can fail ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.LONG_ROWS)
def test_long_row_cases_have_rows_beyond_their_cap_whose_order_shows(name):
    """>= 20 rows longer than the CAP the slot count selects, and >= 10 of them with other bits when the entries
    from position CAP on - the ones a sort of the first CAP entries never looks at - come in reverse order"""
    c = RC.ell_case(name)
    cap = RC.sort_cap(c["bw"])
    assert cap is not None
    long_rows = sum(len(r) > cap for r in c["rows"])
    changed = _changed(c, RR.reverse_from(c["rows"], cap))
    print(f"{name}: CAP {cap}, {long_rows} rows longer, longest {max(map(len, c['rows']))}, {changed} change bits")
    assert long_rows >= 20 and changed >= 10
    if name == "4097x8":
        assert (long_rows, changed, max(map(len, c["rows"]))) == (474, 57, 18)


def test_the_speculative_bound_is_too_small_for_the_general_generators():
    """rows x slots, what the speculative rebuild reserves, against the SELL slots (64 x the longest row of every
    chunk): the rebuild cases go beyond it, so their rebuild has to be repeated the slow way"""
    for name, want in (("4097x8", (48512, 33280)), ("1000x4", None)):
        c = RC.ell_case(name)
        ln = np.array([len(r) for r in c["rows"]] + [0] * (-c["n"] % 64)).reshape(-1, 64)
        slots, bound = int(ln.max(axis=1).sum()) * 64, ln.size * c["bw"]
        assert slots > bound
        if want:
            assert (slots, bound) == want


def test_the_short_and_wide_cases_show_a_reversed_row():
    """1000 x 4: 140 rows longer than the slot count (none beyond CAP = 8: the case is about the partition and the
    reserved bound); (65, 20) and (1000, 33): the insertion sort.  A row summed backwards has other bits."""
    c = RC.ell_case("1000x4")
    assert sum(len(r) > 4 for r in c["rows"]) == 140 and max(map(len, c["rows"])) <= 8
    for name in ("1000x4", "65x20", "1000x33"):
        c = RC.ell_case(name)
        assert RC.sort_cap(c["bw"]) is None or name == "1000x4"
        assert _changed(c, RR.reverse_from(c["rows"], 0)) >= 10


def test_the_duplicated_links_tie_on_the_key():
    c = RC.ell_case("duplicated links 600x8")
    tied = [r for r, row in enumerate(c["rows"]) if any(a[0] == b[0] for a, b in zip(row, row[1:]))]
    same = [r for r, row in enumerate(c["rows"]) if any(a == b for a, b in zip(row, row[1:]))]
    assert len(tied) >= 20 and len(same) >= 10
    # the tie broken the other way (larger value first) shows in the bits
    other = [sorted(row, key=lambda e: (e[0], -e[1])) for row in c["rows"]]
    assert _changed(c, other) >= 10


@pytest.mark.parametrize("which", ["goutsias", "made up"])
def test_state_order_cases_show_a_row_summed_in_the_internal_order(which):
    """the device keeps the states in lexicographic order of their coordinates; a row sorted by THAT numbering
    instead of the caller's has other bits in >= 10 rows"""
    c = RC.golden_case() if which == "goutsias" else RC.ell_case("4097x8")
    state = c["state"] if which == "goutsias" else RC.made_up_coords(c["n"])
    assert len(np.unique(state, axis=0)) == c["n"]
    rank = RC.lexicographic_rank(state)
    assert not np.array_equal(rank, np.arange(c["n"]))
    internal = [sorted(row, key=lambda e: (rank[e[0]], e[1])) for row in c["rows"]]
    assert _changed(c, internal) >= 10


@pytest.mark.parametrize("name", RC.CSR)
def test_banded_cases_show_a_reversed_row(name):
    c = RC.csr_case(name)
    assert _changed(c, RR.reverse_from(c["rows"], 0)) >= 10


def test_partition_blocks_are_blocks_of_the_whole():
    for name in ("1000x4", "2000x12"):
        c = RC.ell_case(name)
        h = c["n"] // 2 + 7
        rows = RR.gather_rows(c["adj"], c["off"], c["diag"], row0=h, nloc=c["n"] - h)
        assert rows == c["rows"][h:]
        assert RR.spmv_exact(rows, c["diag"][h:], c["x"], row0=h) == c["y"][h:].tolist()


def test_the_drop_vector_flags_about_a_twentieth_and_leaves_long_rows():
    c = RC.ell_case("4097x8")
    n = c["n"]
    w = RC.drop_vector(c["adj"], n)
    aw = np.array(RR.spmv_exact(c["rows"], c["diag"], w))
    assert np.abs(aw - 1e-8).min() > 1e-10                   # no decision hinges on rounding
    flags = (w < 1e-8) & ~(aw > 1e-8)
    assert 0.03 * n <= flags.sum() <= 0.08 * n
    adj2, off2, diag2 = RC.compact(c["adj"], c["off"], c["diag"], ~flags)
    rows = RR.gather_rows(adj2, off2, diag2)
    x = c["x"][~flags]
    y = np.array(RR.spmv_exact(rows, diag2, x))
    y2 = np.array(RR.spmv_exact(RR.reverse_from(rows, 8), diag2, x))
    assert sum(len(r) > 8 for r in rows) >= 20 and int((RC.bits(y) != RC.bits(y2)).sum()) >= 10


# ---- the transposed rows (option adjoint) ---------------------------------------------------------------------------
def test_transposed_rows_by_hand():
    X = [[1.0, 0.5], [10.0, 0.25], [100.0, 2.0]]
    # banded, delta = (-1, 2): A(1, 0) = 2, A(2, 1) = 3 on the first diagonal, A(0, 2) = 4 on the second
    val = [[9.0, 2.0, 3.0], [4.0, 9.0, 9.0]]
    Y = RR.banded_t_exact([-1, 2], val, [1.5, 2.5, 3.5], X)
    assert Y == [[-1.5 + 2.0 * 10.0, -0.75 + 2.0 * 0.25], [-25.0 + 3.0 * 100.0, -0.625 + 3.0 * 2.0], [-350.0 + 4.0, -7.0 + 4.0 * 0.5]]
    # the same matrix as reference arrays: state 0 -> state 2 (rate 4), state 1 -> 0 (2), state 2 -> 1 (3) and a link outside
    adj, off = [[3, 0], [-1, 1], [2, 7]], [[4.0, 9.0], [9.0, 2.0], [3.0, 9.0]]
    Z = RR.ell_t_exact(adj, off, [1.5, 2.5, 3.5], X)
    assert Z == [[-1.5 + 4.0 * 100.0, -0.75 + 4.0 * 2.0], [-25.0 + 2.0 * 1.0, -0.625 + 2.0 * 0.5], [-350.0 + 3.0 * 10.0, -7.0 + 3.0 * 0.25]]
    assert np.array_equal(np.array(Z), ell_t(np.array(adj), np.array(off), np.array([1.5, 2.5, 3.5]), np.array(X)))
    assert RR.ell_t_exact(adj, off, [1.5, 2.5, 3.5], X, diag_last=True) == Z          # exact in both orders at these values


@pytest.mark.parametrize("name", AC.CASES)
def test_transposed_rows_against_the_assembled_transpose_and_can_tell(name):
    """The exact rows against A^T X of the assembled generator and against the numpy statement of the same row (separate
    multiply and add) at the bound of the device tests - and the case can tell a wrong kernel: the rows with their
    entries in descending order, and (banded, ELL) with the diagonal term applied last, differ on the bits from the right
    ones in at least one row and column.  (No case needed another X or shape for that: with magnitudes over six decades
    nearly every row of a random column shows either.)"""
    c = AC.case(name)
    A, X, Y = c["A"], c["X"], c["Y"]
    tol = bound(A, X)
    assert np.all(np.abs(Y - A.T @ X) <= tol)
    if name in AC.BANDED:
        mdl = AC.model(name)
        loose = banded_t(*banded_form(mdl), X)
        delta = banded_form(mdl)[0]
        assert delta.min() < 0 < delta.max() and mdl.n % 128 != 0       # sources on both sides, a ragged last group
    elif name in AC.ELL:
        adj, off, diag = AC.ell_arrays(name)
        loose = ell_t(adj, off, diag, X)
        if name != "ell_coded":
            assert (adj < 1).any() and len(diag) % 64 != 0
        if name == "ell_wide":
            mid = (adj[:, 1] == 0) & (adj[:, 2] > 0)
            assert mid.sum() >= 10                                      # ADJ = 0 with a link behind it in the row
    else:
        loose = box_t(AC.model(name), X)
    assert np.all(np.abs(Y - loose) <= tol)
    assert np.abs(X[X != 0.0]).min() >= 1e-3 and np.abs(X).max() <= 1e3 and (X < 0).any() and (X > 0).any()
    assert np.count_nonzero(X[:, 1]) == 1
    wrong = {"descending": AC.exact(name, X, descending=True)}
    if name not in AC.BOXES:
        wrong["diagonal last"] = AC.exact(name, X, diag_last=True)
    for what, Z in wrong.items():
        bad = AC.mismatches(Z, Y)
        print(f"{name}: {what}: {int(bad.any(axis=1).sum())} of {c['n']} rows change, per column {bad.sum(axis=0).tolist()}")
        assert bad.any(), (name, what)
        assert np.all(np.abs(Z - A.T @ X) <= tol)                      # ... and the loose bound passes both


def test_the_small_boxes_reach_their_edges():
    """one box below a wavefront's 64 rows, one with a dimension of 2, one with nu = +-2"""
    assert AC.model("box_one_species").n < 64
    assert 2 in AC.model("box_repressilator_3x2").dims
    assert np.abs(AC.model("box_four_slot_6x4").stoich).max() == 2
    slots = {name: RR.box_slots(AC.model(name)) for name in AC.BOXES}
    assert [(len(s), max(map(len, s))) for s in slots.values()] == [(2, 2), (3, 2), (6, 2), (2, 4), (1, 2)]


# ---- the forward matrix-free rows (box_exact: formats 4 / 6 / 7 / 8 and k_spmm_box; box_generic_exact: format 3, box_store) -----
U = 2.0 ** -53
# which wrong kernel a case can show, and why the others cannot: (function, flag) -> the cases it applies to
SEVERAL_SPECIES = tuple(n for n in BC.SMALL if n != "box_one_species")        # one species: both entry orders are the same order
# one or two species (the instantiation's padding species share 0.0): a sum of two shares commutes
THREE_SHARES = ("box_repressilator_3x2", "box_birth_death_6x2", "decode_49x4x3", "decode_8x49x2", "decode_2x49x2x2x2x2")
CAN_TELL = {
    ("box_exact", "diag_first"): BC.SMALL,
    ("box_exact", "by_position"): SEVERAL_SPECIES,
    ("box_exact", "tie_swapped"): ("dup_12x9",),                             # no other case has two slots on one offset
    ("box_exact", "shares_reversed"): THREE_SHARES,
    ("box_generic_exact", "diag_last"): BC.SMALL + BC.NAMED_GENERIC,
    ("box_generic_exact", "by_species"): SEVERAL_SPECIES + BC.NAMED_GENERIC,
    ("box_generic_exact", "tie_swapped"): ("dup_12x9",),
    ("box_generic_exact", "factors_reversed"): ("three_factor",),            # a product of two factors commutes
}


def test_forward_box_rows_by_hand():
    """birth at rate 2, death at rate x on {0, 1, 2}: slot order is ascending source offset - the birth (from r - 1)
    before the death (from r + 1); every number exact, so both definitions give the same"""
    from krylovfspssa_amd import synth
    mdl = synth.BoxModel("by hand", (3,), [[1, -1]], lambda r, X: np.full_like(X[0], 2.0) if r == 0 else 1.0 * X[0], deps=[(0,), (0,)])
    x = [1.0, 10.0, 100.0]
    assert RR.box_rows(mdl) == [([(0.0, 0), (1.0, 1)], 2.0), ([(2.0, 0), (2.0, 2)], 3.0), ([(2.0, 1), (0.0, 2)], 4.0)]
    assert RR.box_generic_rows(mdl) == RR.box_rows(mdl)
    assert RR.box_exact(mdl, x) == [8.0, 172.0, -380.0] == RR.box_generic_exact(mdl, x)
    assert RR.box_exact(mdl, x, row0=1, nloc=2) == [172.0, -380.0] == RR.box_generic_exact(mdl, x, row0=1, nloc=2)
    for wrong in ("diag_first", "by_position", "tie_swapped", "shares_reversed"):
        assert RR.box_exact(mdl, x, **{wrong: True}) == [8.0, 172.0, -380.0]
    for wrong in ("diag_last", "by_species", "tie_swapped", "factors_reversed"):
        assert RR.box_generic_exact(mdl, x, **{wrong: True}) == [8.0, 172.0, -380.0]


def _exactly_rounded(rows, x):
    """per row: the Fraction sum of the listed entries and of -dsum x[r], rounded ONCE; sum |a| |x|; present entries"""
    y, mag, cnt = [], [], []
    for r, (ent, dsum) in enumerate(rows):
        t = -Fraction(dsum) * Fraction(x[r])
        m = abs(dsum * x[r])
        for a, src in ent:
            t += Fraction(a) * Fraction(x[src])
            m += abs(a * x[src])
        y.append(float(t))
        mag.append(m)
        cnt.append(sum(a != 0.0 for a, _ in ent))
    return np.array(y), np.array(mag), np.array(cnt)


@pytest.mark.parametrize("name", BC.all_names())
def test_box_restatements_against_the_exactly_rounded_row(name):
    """Both restatements round once per present entry (an fma of 0.0 adds nothing) and once for the diagonal term, each
    time by at most 2^-53 of a partial sum that sum |a| |x| bounds; the exactly rounded row adds half a rounding: within
    (entries + 2) 2^-53 sum |a| |x| of it.  The LISTS the arithmetic runs over are checked against the model itself: the
    off-diagonal entries are synth's gather rows (the same bits with one factor per propensity - a table IS the
    propensity - and to a few roundings of the factor product otherwise) and dsum is DIAG; the two definitions list the
    same entries, in two orders, and their dsum differ by the roundings of R - 1 additions each."""
    c = BC.case(name)
    mdl, x = c["mdl"], c["x"].tolist()
    single = name in BC.FAST
    assert np.abs(c["x"]).min() >= 0.5 and np.abs(c["x"]).max() <= 1.5 and (c["x"] < 0).any() and (c["x"] > 0).any()
    rows_g = RR.box_generic_rows(mdl)
    y, mag, cnt = _exactly_rounded(rows_g, x)
    assert np.all(np.abs(c["yg"] - y) <= (cnt + 2) * U * mag)
    cols, vals = mdl.rows_at(np.arange(mdl.n, dtype=np.int64))
    big = np.iinfo(np.int64).max
    for r, (ent, dsum) in enumerate(rows_g):
        want = sorted((int(cc), float(v)) for cc, v in zip(cols[r], vals[r]) if cc != big and cc != r)
        got = sorted((src, a) for a, src in ent if src != r)
        diag = -float(vals[r][list(cols[r]).index(r)])
        if single:
            assert got == want and dsum == diag, (name, r)
        else:
            assert [s for s, _ in got] == [s for s, _ in want]
            assert np.allclose([a for _, a in got], [a for _, a in want], rtol=3e-15, atol=0.0)
            assert abs(dsum - diag) <= 3e-15 * diag
    if not single:
        return
    rows_f = RR.box_rows(mdl)
    y, mag, cnt = _exactly_rounded(rows_f, x)
    assert np.all(np.abs(c["y"] - y) <= (cnt + 2) * U * mag)
    for r, ((ef, df), (eg, dg)) in enumerate(zip(rows_f, rows_g)):
        assert sorted(e for e in ef if e[1] != r) == sorted(e for e in eg if e[1] != r)
        assert abs(df - dg) <= 2 * (mdl.R - 1) * U * max(df, dg)
    # the two definitions against each other: each within its bound of its own exact row, and the two exact rows differ
    # by (dsum_fast - dsum_generic) x[r]
    dd = np.array([abs(df - dg) for (_, df), (_, dg) in zip(rows_f, rows_g)])
    assert np.all(np.abs(c["y"] - c["yg"]) <= 2 * (cnt + 2) * U * mag + dd * np.abs(c["x"]) * (1 + U))


@pytest.mark.parametrize("name", [n for n in BC.FAST if n != "dup_12x9"])
def test_the_generic_box_row_is_the_stored_row_where_no_offsets_tie(name):
    """single-factor boxes whose reactions have distinct offsets: sorted position IS ascending source, so
    box_generic_exact must be spmv_exact over the box's CSR rows, on the bits - also for a row block"""
    c = BC.case(name)
    mdl = c["mdl"]
    assert len(set(mdl.offsets.tolist())) == mdl.R
    rows, diag = RR.rows_from_csr(mdl.n, *mdl.csr_rows())
    assert RR.spmv_exact(rows, diag, c["x"]) == c["yg"].tolist()
    if name in BC.SMALL:
        r0, nl = mdl.n // 3 + 1, mdl.n // 2
        assert RR.box_generic_exact(mdl, c["x"], row0=r0, nloc=nl) == c["yg"][r0:r0 + nl].tolist()
        assert RR.box_exact(mdl, c["x"], row0=r0, nloc=nl) == c["y"][r0:r0 + nl].tolist()


def test_tied_offsets_need_a_definition_of_their_own():
    """dup_12x9: two births per species on ONE offset.  spmv_exact's rule - by source, then by VALUE - puts the smaller rate
    first; the device goes by reaction.  The two disagree on the bits, which is why box_generic_exact is no spmv_exact."""
    c = BC.case("dup_12x9")
    mdl = c["mdl"]
    assert len(set(mdl.offsets.tolist())) == mdl.R - 2
    rows, diag = RR.rows_from_csr(mdl.n, *mdl.csr_rows())
    by_value = [sorted(row) for row in rows]
    assert sum(a != b for a, b in zip(by_value, rows)) >= 20
    changed = len(BC.mismatches(np.array(RR.spmv_exact(by_value, diag, c["x"])), c["yg"]))
    print(f"dup_12x9: by source then value changes {changed} of {mdl.n} rows")
    assert changed >= 10
    slots = RR.box_slots(mdl)
    assert [[k for k, _ in sp] for sp in slots] == [[0, 1, 2], [3, 4, 5]]       # the births (from r - stride) by reaction, then the death


@pytest.mark.parametrize("fn,flag", list(CAN_TELL))
def test_every_forward_box_case_can_tell_a_wrong_kernel(fn, flag):
    """each wrong variant changes the bits of >= 10 rows of every case it applies to - and of NO row of a case it is
    said not to apply to (one species; two shares; no tied offsets; at most two factors), which is the reason stated
    in CAN_TELL.  The loop_* boxes repeat four of these models at a larger size and the random models are breadth, not
    edges: neither is asked to tell."""
    names = BC.SMALL + (BC.NAMED_GENERIC if fn == "box_generic_exact" else ())
    ref = "y" if fn == "box_exact" else "yg"
    for name in names:
        c = BC.case(name)
        z = np.array(getattr(RR, fn)(c["mdl"], c["x"], **{flag: True}))
        changed = len(BC.mismatches(z, c[ref]))
        print(f"{fn}({flag}) on {name}: {changed} of {c['n']} rows change")
        if name in CAN_TELL[(fn, flag)]:
            assert changed >= 10, (name, fn, flag, changed)
        else:
            assert changed == 0, (name, fn, flag, changed)


def test_the_decode_boxes_take_the_correction_step():
    """the kernel's formula in numpy: rows whose decode comes out one short and takes r >= d.  The r < 0 step needs a
    quotient estimate that is one too LARGE, which q * (1 / d) gives only for q near 2^31: it stays untested at these
    sizes (no box here has a row that takes it)."""
    counts = {name: BC.decode_corrections(BC.model(name)) for name in BC.FAST}
    print(counts)
    assert [counts[n] for n in BC.DECODE] == [(7, 0), (8, 0), (22, 0), (4, 0)]
    assert all(lo == 0 for _, lo in counts.values())
    assert all(hi >= 4 for n, (hi, _) in counts.items() if n in BC.DECODE)
    # ... also inside the row blocks of the partition tests' boxes nothing else turns up
    assert 49.0 * (1.0 / 49.0) < 1.0


def test_the_forward_box_cases_reach_their_edges():
    from krylovfspssa_amd import host
    for name in BC.FAST:
        assert BC.instance_of(BC.model(name)) == BC.INSTANCE[name], name
    assert {BC.INSTANCE[n] for n in BC.SMALL} == {BC.INSTANCE[n] for n in BC.LOOP} == {(2, 2), (3, 2), (6, 2), (6, 4)}
    assert all(BC.model(n).n <= 1600 for n in BC.SMALL + BC.generic_names())
    fmts = {n: (BC.pencil_format(BC.model(n), 1), BC.pencil_format(BC.model(n), 2)) for n in BC.SMALL}
    assert fmts["decode_49x4x3"] == (7, 7) and fmts["decode_8x49x2"] == (7, 8) and fmts["decode_2x49x2x2x2x2"] == (7, 8)
    assert fmts["box_birth_death_6x2"] == (7, 8) and fmts["box_repressilator_3x2"] == (4, 4)       # planes of 143 rows
    assert all(f == (4, 4) for n, f in fmts.items() if BC.model(n).d < 3)
    # grid_blocks = 8: a workgroup's share of the trips is more than its four wavefronts only on the loop boxes
    for name in BC.FAST:
        share = -(-(-(-BC.model(name).n // 128)) // 8)
        assert (share > 4) == (name in BC.LOOP), (name, share)
    gm = BC.model("goutsias")
    assert gm.n == 720 and sorted(map(len, gm.deps)).count(2) == 2 and (np.count_nonzero(gm.stoich, axis=0) == 3).any()
    assert sorted(map(len, BC.model("three_factor").deps)) == [1, 1, 2, 3, 3]
    assert len(BC.generic_names()) >= 6
    # the row partition: blocks of 64-row multiples; one case whose blocks are shorter than its reach (no halo strips:
    # the all-gather), every case with a ragged last block
    for name, P, gather in BC.PARTITIONED:
        mdl = BC.model(name)
        blocks = [host.partition(mdl.n, P, r) for r in range(P)]
        L = blocks[0][2]
        reach = int(np.abs(mdl.offsets).max())
        assert all(nr > 0 for _, nr, _ in blocks) and blocks[-1][1] % 64 != 0 and blocks[-1][1] < L
        assert (-(-reach // 8) * 8 > L) == gather, (name, P, reach, L)
    assert any(g for _, _, g in BC.PARTITIONED) and not all(g for _, _, g in BC.PARTITIONED)
