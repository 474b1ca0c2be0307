"""tests/krylov_ref.py, the local restatement of one Arnoldi column and of the combine, checked without a device
(DESIGN.md 7.2): the CPU oracle's literal modified Gram-Schmidt pass and a numpy combine pass every check on every case
the device tests use, with room to spare - and a wrong pass does not: each mutation below exceeds a bound by a factor of
at least 1000, so a device test that passes says something.  Run with -s to see the ratios."""
import numpy as np
import pytest

from tests import krylov_ref as K

PLAIN = [("general", n) for n in K.GENERAL_N] + [("banded", n) for n in K.BANDED_N] + [("box", b) for b in K.BOXES] + \
        [("golden", "assembly_goutsias_k10.npz")]
# every case that is uploaded as arrays has a near-invariant sibling (krylov_ref.near_invariant_case): same links and
# propensities, another diagonal and start vector
NEAR = [("near_" + k, a) for k, a in PLAIN if k != "box" and (k != "general" or a >= 63)]
CASES = PLAIN + NEAR
IDS = [f"{k}-{a}" for k, a in CASES]


def _case(kind, arg, golden_dir):
    near, kind = kind.startswith("near_"), kind.replace("near_", "")
    c = {"general": K.general_case, "banded": K.banded_case, "box": K.box_case,
         "golden": lambda f: K.golden_case(golden_dir, f)}[kind](arg)
    return K.near_invariant_case(c) if near else c


def _ell(case):
    """the reference's arrays for the oracle; a CSR case is turned into them (one slot per entry of a column)"""
    if hasattr(case, "ell"):
        return case.ell
    rows, diag, n = case._rows, case._diag, case.n
    count = np.zeros(n, dtype=np.int64)
    for row in rows:
        for c, _ in row:
            count[c] += 1
    bw = max(1, int(count.max()))
    adj, off, at = np.zeros((n, bw), dtype=np.int32), np.zeros((n, bw)), np.zeros(n, dtype=np.int64)
    for r, row in enumerate(rows):
        for c, v in row:
            adj[c, at[c]], off[c, at[c]] = r + 1, v
            at[c] += 1
    return adj, off, np.asarray(diag, dtype=np.float64)


def _oracle_pass(oracle, case, m, qiop=2):
    A = oracle.EllMatrix(*_ell(case))
    beta = float(np.sqrt((case.w * case.w).sum()))
    V, H, mb, k1, av = oracle.arnoldi(A, case.w / beta, m, qiop=qiop)
    assert (mb, k1) == (m, 2), "happy breakdown in a case that must not have one"
    return beta, V, H, av


def _combine(V, mx, beta, y, skip_remainder=False, clamp=True):
    """the oracle's combine (kfsp_oracle.c: column sweep, w += (beta y_j) v_j, clamp, sum); the two switches are the
    mutations"""
    w = np.zeros(V.shape[0])
    for j in range(mx - mx % 4 if skip_remainder else mx):
        w = w + (beta * y[j]) * V[:, j]
    if clamp:
        w[w < 0.0] = 0.0
    return w, float(np.abs(w).sum())


def test_extended_precision_is_what_the_header_says():
    assert K.LONG_OK == (np.finfo(np.longdouble).nmant >= 63)
    ar = K.Arith(exact=True)
    assert abs(float(ar.sqrt(2) ** 2 - 2)) < 1e-30 and abs(float(ar.sqrt(K.U ** 4) / K.U ** 2 - 1)) < 1e-30
    assert K.worst(np.array([0.0, 2.0]), np.array([0.0, 4.0])) == 0.5 and K.worst(np.array([1e-300]), np.array([0.0])) == np.inf
    assert K.window(5, 2) == [4, 5] and K.window(1, 2) == [1] and K.window(4, 0) == [1, 2, 3, 4] and K.window(4, 1) == [4]


@pytest.mark.parametrize("kind,arg", CASES, ids=IDS)
def test_the_oracle_passes_every_check(oracle, golden_dir, kind, arg):
    """oracle.arnoldi (literal MGS) over the restarted pass's 9 columns and a numpy combine at every mx"""
    case = _case(kind, arg, golden_dir)
    gen, m = case.gen(), min(K.M_LONG, case.n - 1)
    beta, V, H, av = _oracle_pass(oracle, case, m)
    basis = lambda k: V[:, k - 1]
    r = K.check_begin(case.w, beta, V[:, 0])
    K.check_pass(gen, basis, H, 1, m, into=r)
    K.merge(r, K.check_avnorm(gen, V[:, m], av))
    K.merge(r, K.check_reductions(case.w, float(np.sqrt(case.w @ case.w)), float(np.abs(case.w).sum())))
    K.merge(r, K.check_restore(beta * V[:, 0], case.w))
    if case.n >= 63:
        for mx in K.COMBINE_MX:
            b, y = K.combine_coefficients(case, mx)
            w, ws = _combine(V, mx, b, y)
            rc = K.check_combine([V[:, j] for j in range(mx)], b, y, w, ws)
            neg, pos, either = K.combine_fractions(*K.combine_exact([V[:, j] for j in range(mx)], b, y))
            assert either <= 0.01 and (mx == 1 or (neg >= 0.1 and pos >= 0.1)), (mx, neg, pos, either)
            K.merge(r, rc)
    print(f"\n{case.name:28s} oracle: {K.fmt(r)}")
    K.assert_ok(r, case.name)


@pytest.mark.parametrize("qiop", [0, 1, 3])
@pytest.mark.parametrize("n", [65, 2049, 4097])
def test_the_oracle_passes_with_other_windows(oracle, n, qiop):
    case = K.general_case(n)
    beta, V, H, av = _oracle_pass(oracle, case, case.m, qiop)
    r = K.check_pass(case.gen(), lambda k: V[:, k - 1], H, 1, case.m, qiop=qiop)
    K.merge(r, K.check_avnorm(case.gen(), V[:, case.m], av))
    print(f"\n{case.name:28s} qiop {qiop}: {K.fmt(r)}")
    K.assert_ok(r, f"{case.name} qiop {qiop}")


@pytest.mark.parametrize("n", [3, 65])
def test_exact_rationals_give_the_same_verdict(oracle, n):
    """the Fraction arithmetic (for platforms whose long double is a double) against np.longdouble"""
    case = K.general_case(n)
    beta, V, H, av = _oracle_pass(oracle, case, case.m)
    out = []
    for exact in (False, True):
        gen = case.gen(exact=exact)
        r = K.check_pass(gen, lambda k: V[:, k - 1], H, 1, case.m)
        K.merge(r, K.check_avnorm(gen, V[:, case.m], av))
        K.merge(r, K.check_begin(case.w, beta, V[:, 0], exact=exact))
        if n >= 63:
            b, y = K.combine_coefficients(case, 5)
            w, ws = _combine(V, 5, b, y)
            K.merge(r, K.check_combine([V[:, j] for j in range(5)], b, y, w, ws, exact=exact))
        out.append(r)
    # a long double sum of n products is itself only good to n 2^-64 = 2^-11 n u: that much of a bound, no more
    for k in out[0]:
        assert out[1][k] == pytest.approx(out[0][k], rel=1e-6, abs=2.0 ** -10), k


# ---- mutations ----------------------------------------------------------------------------------------------------------
def _mutants(oracle, case):
    """name -> worst factor by which the mutated output of the oracle exceeds a bound.  V is left as the oracle made
    it; the one scalar a wrong kernel would have got wrong is recomputed from the oracle's own vectors."""
    gen, m = case.gen(), case.m
    beta, V, H, av = _oracle_pass(oracle, case, m)
    A = oracle.EllMatrix(*_ell(case))
    basis = lambda k: V[:, k - 1]
    worst = {}

    def run(name, j, row, value):
        Hm = H.copy()
        Hm[row - 1, j - 1] = value
        r = K.check_column(gen, j, basis, Hm)
        worst[name] = max(worst.get(name, 0.0), max(r.values()))

    for j in range(2, m + 1):
        p = oracle.spmv_ell(A, V[:, j - 1])
        vm, vj = V[:, j - 2], V[:, j - 1]
        w = H[j, j - 1] * V[:, j]                                          # what the norm was taken of
        run("h1 dot without its last element", j, j - 1, float(vm[:-1] @ p[:-1]))
        run("norm without its last element", j, j + 1, float(np.sqrt(w[:-1] @ w[:-1])))
        run("norm with a stale element of 1e-3", j, j + 1, float(np.sqrt(w @ w + 1e-3 * 1e-3)))
        run("h2 classical (v_j . p)", j, j, float(vj @ p))
        if j >= 3:
            # the fused h2 = v_j . p - h1 g (normalised) with g = v_{j-1} . v_{j-2} of the column before
            run("h2 fused with the previous g", j, j, float(vj @ p) - H[j - 2, j - 1] * float(vm @ V[:, j - 3]))
    return worst


GENERIC = [(k, a) for k, a in PLAIN if k != "general" or a >= 63]      # every case with n >= 63 ...
ALL63 = GENERIC + NEAR                                                 # ... and its near-invariant sibling
SHOWN_EVERYWHERE = ("h1 dot without its last element", "norm without its last element", "norm with a stale element of 1e-3")
WINDOW_ONLY = ("h2 classical (v_j . p)", "h2 fused with the previous g")


@pytest.mark.parametrize("kind,arg", ALL63, ids=[f"{k}-{a}" for k, a in ALL63])
def test_mutations_of_the_pass_fail(oracle, golden_dir, kind, arg):
    """The scalar mutations on every case with n >= 63.  The two mutations of h2 change it by h1 (v_j . v_{j-1}).  With
    a generic start vector the window is orthogonal to rounding (krylov_ref.near_invariant_case says why) and the change
    is below every bound - no local check can see it, and nothing on such a case shows a wrong g.  That is why every
    general, banded and golden case has a near-invariant sibling, on which all of them must show; on the generic cases
    (and the matrix-free boxes, whose generator cannot be given another diagonal) the two factors are printed."""
    case = _case(kind, arg, golden_dir)
    f = _mutants(oracle, case)
    print(f"\n{case.name:28s} " + "; ".join(f"{k}: {v:.3g}" for k, v in f.items()))
    for name in SHOWN_EVERYWHERE + (WINDOW_ONLY if kind.startswith("near_") else ()):
        assert f[name] >= 1e3, (name, f[name])


@pytest.mark.parametrize("kind,arg", ALL63, ids=[f"{k}-{a}" for k, a in ALL63])
def test_mutations_of_the_combine_fail(oracle, golden_dir, kind, arg):
    """every mx with a remainder (mx mod 4 != 0) without its remainder columns, every mx > 1 without the clamp"""
    case = _case(kind, arg, golden_dir)
    m = min(K.M_LONG, case.n - 1)
    beta, V, H, av = _oracle_pass(oracle, case, m)
    out = []
    for mx in K.COMBINE_MX:
        b, y = K.combine_coefficients(case, mx)
        cols = [V[:, j] for j in range(mx)]
        if mx % 4:
            w, ws = _combine(V, mx, b, y, skip_remainder=True)
            f = K.check_combine(cols, b, y, w, ws)["combine"]
            out.append(f"mx {mx} remainder skipped: {f:.3g}")
            assert f >= 1e3, (mx, f)
        if mx > 1:
            w, ws = _combine(V, mx, b, y, clamp=False)
            rc = K.check_combine(cols, b, y, w, ws)
            out.append(f"mx {mx} no clamp: {rc['combine']:.3g} ({rc['negative']} negative)")
            assert rc["combine"] >= 1e3 and rc["negative"] >= 0.1 * case.n, (mx, rc)
    print(f"\n{case.name:28s} " + "; ".join(out))
