"""tests/drop_ref.py on the CPU: the restatement of DROP_STATES reproduces what the unmodified reference recorded
(fixtures droptol.npz and drop_*), and every case of tests/test_gpu_drop_edges.py can tell a wrong device from a right one -
its margin and its "no row near the guard" condition hold, and each mistake the case is there for, made in the RESTATEMENT,
changes the case's answer.  No kernel is built or run here."""
import os

import numpy as np
import pytest

from tests import drop_ref as D
from tests import row_ref as RR
from tests.conftest import GOLDEN
from tests.expand_helpers import onestep_py
from tests.expand_helpers import stoich as _stoich


# ---- the restatement against the reference's recorded results ---------------------------------------------------------------
def test_find_droptol_reproduces_the_recorded_thresholds():
    g = np.load(os.path.join(GOLDEN, "droptol.npz"))
    w = D.spread_vector(50000)
    for dsum, want in zip(g["dsum"], g["droptol"]):
        tol, margin = D.find_droptol(w, float(dsum))
        assert tol == want
        assert D.margin_ok(w, float(dsum)), (dsum, margin)       # (what tests/test_gpu_drop.py relies on)


def _pre_drop_fsp(name, k):
    """the FSP of k sweeps.  goutsias k = 12 has no assembly fixture of its own: its states and links are two plain
    sweeps (tests/expand_helpers.py) on the k = 10 assembly, its propensities those of the same states in the k = 16
    assembly, whose list begins with them"""
    if os.path.exists(os.path.join(GOLDEN, f"assembly_{name}_k{k}.npz")):
        a = np.load(os.path.join(GOLDEN, f"assembly_{name}_k{k}.npz"))
        return a["state"], a["adj"], a["offdiag"], a["diag"], _stoich(a)
    assert (name, k) == ("goutsias", 12)
    a10 = np.load(os.path.join(GOLDEN, "assembly_goutsias_k10.npz"))
    a16 = np.load(os.path.join(GOLDEN, "assembly_goutsias_k16.npz"))
    nu = _stoich(a16)
    state, adj = a10["state"], a10["adj"]
    for _ in range(2):
        state, adj = onestep_py(nu, state, adj, 10000)
    n = len(state)
    assert np.array_equal(state, a16["state"][:n])
    return state, adj, a16["offdiag"][:n], a16["diag"][:n], nu


@pytest.mark.parametrize("name,k,dsum", D.RECORDED_DROPS)
def test_decision_and_compaction_reproduce_the_recorded_drop(name, k, dsum):
    """find_droptol, decide (on the exact product: no row of these fixtures is near the guard), the 10 % rule and
    compact_lists, then the sweep the reference runs after DROP_STATES: state list, links and propensities are the
    fixture's, the vector is the compacted one.  Two of the four fixtures are left alone by the 10 % rule; the other
    two tell a dropped link written as -1 and a renumbering that is off by one from the right lists."""
    g = np.load(os.path.join(GOLDEN, D.recorded_drop_name(name, k, dsum)))
    state, adj, off, diag, nu = _pre_drop_fsp(name, k)
    n = len(state)
    w = D.decaying_vector(n)
    assert D.margin_ok(w, dsum)
    aw, mass = D.exact_product(RR.gather_rows(adj, off, diag), diag, w)
    assert D.guard_clear(aw, mass)
    tol, _ = D.find_droptol(w, dsum)
    drop, count, nflag = D.decide(w, [float(x) for x in aw], tol)
    compacts = count / n > 0.1                                  # StateSpace.f90:497
    assert compacts == ((name, k) in (("toggle", 20), ("goutsias", 12)))
    keep = ~drop if compacts else np.ones(n, dtype=bool)
    nk = int(keep.sum())

    def after(**wrong):
        s2, a2, o2, d2, w2 = D.compact_lists(state, adj, off, diag, w, keep, **wrong)
        s3, a3 = onestep_py(nu, s2, np.minimum(a2, nk), 10000)
        return s3, a3, o2, d2, w2

    s3, a3, o2, d2, w2 = after()
    assert np.array_equal(s3, g["state"]) and np.array_equal(a3, g["adj"])
    assert np.array_equal(o2, g["offdiag"][:nk]) and np.array_equal(d2, g["diag"][:nk])
    # (the vector is rebuilt here with numpy's pow, the fixture's with the Fortran runtime's: last-bit differences)
    assert np.all(np.abs(w2 - g["vector"][:nk]) <= 5e-16 * g["vector"][:nk]) and not g["vector"][nk:].any()
    if compacts:
        for wrong in (dict(dropped_as=-1), dict(shift=1)):
            s3, a3 = after(**wrong)[:2]
            assert not (np.array_equal(s3, g["state"]) and np.array_equal(a3, g["adj"])), wrong


# ---- the cases of tests/test_gpu_drop_edges.py ---------------------------------------------------------------------------------
WRONG = {
    "sum <=": (dict(sum_le=True), {}),
    "stop <=": (dict(stop_le=True), {}),
    "no w > 0": (dict(positive_only=False), {}),
    "mark <=": ({}, dict(mark_le=True)),
    "guard >=": ({}, dict(guard_ge=True)),
    "count = nflag": ({}, dict(count_is_nflag=True)),
}


def _answer(c, search=None, decision=None):
    tol, _ = D.find_droptol(c["w"], c["dsum"], **(search or {}))
    drop, count, nflag = D.decide(c["w"], c["aw"], tol, **(decision or {}))
    return tol, drop.tobytes(), count, nflag


def _catches(c, names):
    right = _answer(c)
    assert right == (c["tol"], c["drop"].tobytes(), c["count"], c["nflag"])
    for name in names:
        assert _answer(c, *WRONG[name]) != right, f"the case cannot tell '{name}' from the right answer"


def _moved_is_the_restated_product(c, rows, diag):
    """with one entry of 1.0 per row and a zero diagonal the restated row (tests/row_ref.py) is w[source] on the bits;
    a zero by value (-(0 * x) carries a sign the guard cannot see)"""
    y = np.array(RR.spmv_exact(rows, diag, c["w"]))
    assert np.array_equal(y, c["aw"])
    nz = c["aw"] != 0.0
    assert np.array_equal(y[nz].view(np.uint64), c["aw"][nz].view(np.uint64))


def _perm_rows(c):
    if c["kind"] == "ell":
        return RR.gather_rows(c["adj"], c["off"], c["diag"]), c["diag"]
    return RR.rows_from_csr(c["n"], c["rowptr"], c["col"], c["val"])


PERM = [(kind, n) for kind in ("ell", "csr") for n in D.REMAINDERS + (D.N_GRID,)]


@pytest.mark.parametrize("kind,n", PERM)
def test_remainder_cases(kind, n):
    """(a) and the forced grids of (b): the product is a move of w, the margin holds, and from n = 63 on the case holds
    every special entry and catches the mark, the guard, the missing w > 0 and the counter; n = 1 sits on the mark's
    edge, n = 2 and 3 on the mark's and the guard's"""
    c = D.perm_case(kind, n)
    _moved_is_the_restated_product(c, *_perm_rows(c))
    assert D.margin_ok(c["w"], c["dsum"])
    if n >= 63:
        assert c["tol"] == D.threshold(D.LEVEL)
        for sp in D.specials():
            assert (c["w"].view(np.uint64) == np.float64(sp).view(np.uint64)).any(), sp
        assert 0 < c["nflag"] < n
        _catches(c, ["mark <=", "guard >=", "no w > 0", "count = nflag"])
        tail = c["drop"][-min(n, 32):]                                   # the rows at the end decide both ways
        assert tail.any() and not tail.all()
    else:
        _catches(c, ["mark <="] if n == 1 else ["mark <=", "guard >="])


@pytest.mark.parametrize("kind", ["ell", "csr"])
def test_the_case_whose_loops_turn(kind):
    """(b): 262 209 states; specials lie beyond lane 1024 x 256 of the first turn"""
    c = D.perm_case(kind, D.N_TURN)
    n = c["n"]
    assert n > 1024 * 256 and n % 2 == 1
    assert np.array_equal(c["aw"], D.moved(c["w"], c["src"]))
    assert D.margin_ok(c["w"], c["dsum"]) and c["tol"] == D.threshold(D.LEVEL)
    beyond = np.arange(n) >= 1024 * 256
    w_b = c["w"][beyond].view(np.uint64)
    for sp in D.specials():
        assert (w_b == np.float64(sp).view(np.uint64)).any(), sp
    assert c["drop"][beyond].any() and not c["drop"][beyond].all()
    _catches(c, ["mark <=", "guard >=", "no w > 0", "count = nflag"])
    # a loop that stops after its first turn leaves the flags beyond it unset, and the compacted vector longer
    cut = c["drop"].copy()
    cut[beyond] = False
    assert int(cut.sum()) != c["nflag"]


@pytest.mark.parametrize("name", D.BATCH_NAMES)
def test_threshold_batch_cases(name):
    c = D.batch_case(name)
    levels = []
    tol, _ = D.find_droptol(c["w"], c["dsum"], levels=levels)
    if name.startswith("level "):
        k = int(name.split()[1])
        assert tol == D.threshold(k) and len(levels) == k + 1
        assert D.margin_ok(c["w"], c["dsum"])
        if k > 0:                                                        # (at level 0 a smaller sum ends the search there too)
            _catches(c, ["no w > 0"])
    elif name in ("all zero", "all negative"):
        assert tol == D.TOL0 and levels == [(D.TOL0, 0.0)] and c["nflag"] == c["n"]
        assert D.margin_ok(c["w"], c["dsum"])
    elif name == "on thresholds":
        assert tol == D.TOL0 and D.margin_ok(c["w"], c["dsum"])
        _catches(c, ["sum <=", "mark <="])
    else:
        # the decision AT the edge: exact sums in place of a margin
        assert D.dyadic_exact(c["w"])
        s5 = levels[5][1]
        assert levels[4][1] > s5 > 0.0
        if name == "dyadic, S == dsum":
            assert c["dsum"] == s5 and tol == D.threshold(6)
            _catches(c, ["stop <="])
        else:
            assert c["dsum"] == D.nxt(s5) and tol == D.threshold(5)


@pytest.mark.parametrize("r", D.STALE_R)
def test_stale_memory_cases(r):
    """(d): the first plan flags exactly the states chosen, 4097 + r stay.  The second plan's sums are exact and dsum2 lies
    2^10 units above S_0: one more small entry moves the threshold.  What the device could wrongly add are the rows between
    n2 and the next multiple of 64 - 63, 62 and 1 of them - and nothing else (k_drop_sums reads whole chunks, k_drop_flags
    only states): with what each route would leave there, the threshold moves"""
    c = D.stale_case(r)
    n, n2, pad = c["n"], c["n2"], c["pad"]
    assert pad == {0: 63, 1: 62, 62: 1}[r] and (n2 + pad) % 64 == 0
    assert np.array_equal(c["first"]["drop"], c["chosen"]) and int(c["chosen"].sum()) == n - n2
    assert len(c["w2"]) == n2 and D.dyadic_exact(c["w2"])
    assert D.margin_ok(c["W"], c["dsum1"]) and D.margin_ok(c["w2"], c["dsum2"])
    rows = RR.gather_rows(c["adj2"], c["off2"], c["diag2"])
    y = np.array(RR.spmv_exact(rows, c["diag2"], c["w2"]))
    assert np.array_equal(y, D.moved(c["w2"], c["src2"]))
    assert 0 < c["second"]["nflag"] < n2
    right, _ = D.find_droptol(c["w2"], c["dsum2"])
    assert right == c["second"]["tol"] == D.TOL0
    assert np.array_equal(c["stale_pending"], c["W"][n2:n2 + pad]) and np.array_equal(c["stale_step"], np.full(pad, 1e-12))
    for route, stale in (("kfsp_set_vector", c["stale_step"]), ("adopted after kfsp_drop_compact", c["stale_pending"])):
        assert len(stale) == pad and ((stale > 0) & (stale < D.TOL0)).all(), route
        for rows_left in (stale, stale[:1], stale[-1:]):          # all of them, or any single one
            wrong, _ = D.find_droptol(c["w2"], c["dsum2"], stale=rows_left)
            assert wrong < right, route


@pytest.mark.parametrize("name", list(D.FORMS))
def test_generator_form_cases(name):
    """(e): general generators - the two conditions under which flags are exact whatever order the device sums in"""
    c = D.form_case(name)
    assert D.margin_ok(c["w"], c["dsum"])
    assert D.guard_clear(c["exact"], c["mass"])
    assert np.array_equal(c["aw"] > D.GUARD, np.array([a > D.Fraction(D.GUARD) for a in c["exact"]]))
    assert c["tol"] == D.threshold(D.LEVEL) and 0 < c["nflag"] < c["n"]
    guarded = c["aw"] > D.GUARD
    marked = c["w"] < c["tol"]
    assert (marked & guarded).any() and (marked & ~guarded).any() and (~marked & guarded).any()
    _catches(c, ["count = nflag"])


@pytest.mark.parametrize("n", D.PARTITION_N)
def test_partition_cases(n):
    """(f) runs generators like those of (a) at n = 65 and 449.  Over P = 2, 3 and 4 ranks (blocks of L = ceil(n / P) rounded
    up to 64 rows) every block of more than one row holds flagged and unflagged states; at n = 65 trailing ranks own one
    row or none"""
    for kind in ("ell", "csr"):
        c = D.perm_case(kind, n)
        assert D.margin_ok(c["w"], c["dsum"]) and 0 < c["nflag"] < n
        _catches(c, ["mark <=", "guard >=", "no w > 0", "count = nflag"])
        for P in D.PARTITION_P:
            L = -(-(-(-n // P)) // 64) * 64
            sizes = [max(0, min(L, n - p * L)) for p in range(P)]
            assert sum(sizes) == n
            if n == 65:
                assert sizes == [64, 1, 0, 0][:P]
            else:
                assert min(sizes) > 1
            for p, size in enumerate(sizes):
                block = c["drop"][p * L:p * L + size]
                assert size <= 1 or (block.any() and not block.all()), (kind, P, p)


@pytest.mark.parametrize("name", D.EXTREMES)
def test_extreme_cases(name):
    c = D.extreme_case(name)
    n = c["n"]
    assert D.margin_ok(c["w"], c["dsum"]) and c["tol"] == D.TOL0
    want = {"nothing": np.zeros(n, dtype=bool), "everything": np.ones(n, dtype=bool)}
    if name == "all but the first":
        want[name] = np.arange(n) > 0
    if name == "all but the last":
        want[name] = np.arange(n) < n - 1
    assert np.array_equal(c["drop"], want[name])


def test_renumbering_cases():
    """(h): every FSP flags exactly the complement of its keep pattern, by the two conditions; over the hundred, each
    wrong compaction is caught many times - and with padded leading dimensions the renumbering of padding slots too"""
    fsps = D.random_fsps()
    assert len(fsps) == D.N_RANDOM
    caught = dict(dropped_as=0, shift=0, renumber_all=0)
    for f in fsps:
        rows = RR.gather_rows(f["adj"], f["off"], f["diag"])
        aw, mass = D.exact_product(rows, f["diag"], f["w"])
        assert D.margin_ok(f["w"], f["dsum"]) and D.guard_clear(aw, mass)
        e = D.expected(f["w"], np.array(RR.spmv_exact(rows, f["diag"], f["w"])), f["dsum"])
        assert np.array_equal(e["keep"], f["keep"]) and e["tol"] == D.threshold(D.LEVEL)
        ld = f["nr"] + 3
        adj = D.padded(f["adj"], ld, D.PAD_ADJ)
        off = D.padded(f["off"], ld, D.PAD_OFF)
        right = D.compact_lists(f["state"], adj, off, f["diag"], f["w"], f["keep"], nr=f["nr"])
        assert np.array_equal(right[1][:, f["nr"]:], adj[f["keep"]][:, f["nr"]:])
        assert np.array_equal(right[1][:, :f["nr"]], D.compact_lists(None, f["adj"], None, None, None, f["keep"])[1])
        for wrong in (dict(dropped_as=-1), dict(shift=1), dict(renumber_all=True)):
            got = D.compact_lists(f["state"], adj, off, f["diag"], f["w"], f["keep"], nr=f["nr"], **wrong)
            caught[list(wrong)[0]] += not np.array_equal(got[1], right[1])
    assert min(caught.values()) >= 40, caught


def test_row_cases_compact_is_the_same_restatement():
    from tests import row_cases as RC
    f = D.random_fsps()[0]
    a, o, d = RC.compact(f["adj"], f["off"], f["diag"], f["keep"])
    _, a2, o2, d2, _ = D.compact_lists(None, f["adj"], f["off"], f["diag"], None, f["keep"])
    assert np.array_equal(a, a2) and np.array_equal(o, o2) and np.array_equal(d, d2)
