"""What one column of the Arnoldi pass and one combine ARE, restated locally ("The column, restated").

A whole pass cannot be compared with another implementation more closely than 1e-11: the IOP(2) recurrence amplifies
rounding differences about 4x per column.  A single column can.  Everything here takes the DEVICE'S OWN
inputs to a column - the normalised basis columns as kfsp_get_basis returns them and column j of H - and checks them
against extended-precision arithmetic on those very numbers, so the amplification never enters and every tolerance is a
count of roundings times u = 2^-53.  No device, no oracle library: numpy, np.longdouble (>= 63 mantissa bits, asserted;
fractions.Fraction in object arrays where the platform's long double is a plain double, or with exact=True), and the
generator as the rows tests/row_ref.py makes (gather_rows / rows_from_csr).

With p = A v_j exact, |p| = |A||v_j|, L_i the number of off-diagonal entries of row i, t the number of columns the
window orthogonalises against (min(j, q) for qiop = q > 0, j for q = 0; 2 from column 2 on in the solver's IOP(2)):

relation, per element
    r_i = p_i - sum_{k in window} H(k,j) v_k,i - H(j+1,j) v_{j+1,i}
    |r_i| <= (L_i + 12 + 2 t) u (|p|_i + sum |H(k,j)||v_k,i| + |H(j+1,j)||v_{j+1,i}|)          (= L_i + 16 for t = 2)
  The roundings, next to the lines that make them (kfsp_kernels.hip; small_pass does the same per lane):
    L_i + 1   the row: one rounded diagonal product, one fused multiply-add per entry (row_sell / rows_dia / rows_box),
              on the UNNORMALISED u_j
    1         `sum *= s` / `v *= s` in k_spmv (MODE != 0): the lazy normalisation of the source, s = 1 / sqrt(sq_j)
    1         v_j,k here is fl(s u_j,k), kfsp_get_basis's multiply: p is the exact product of THOSE numbers
    per window column, weighted by its own term only: c = h s (`c1 = h1 * s1`, `c2 = h2 * s2`, `coef = h * si`), the
              product c u, and get_basis's multiply of that column: 3; and one subtraction (`wa.x -= c1 * xa.x`,
              `w.x -= coef * u.x`) on the running value, whose magnitude the sum of all magnitudes bounds: 1
    3         the last term: H(j+1,j) = sqrt(sq_{j+1}), get_basis's 1 / sqrt and its multiply.  sq_{j+1} itself cancels,
              however wrong: it is pinned by the normalisation below.
  Weighted by the magnitudes they act on that is at most (L_i + 3 + t) u times the sum; L_i + 12 + 2 t leaves room
  for a matrix-free box, whose propensities are products of factor-table entries and whose diagonal is summed species
  by species (up to 8 more roundings on an entry than the uploaded arrays of the same box carry).  1/sqrt(sq) is
  computed by the same expression on the device and in get_basis, and both are correctly rounded.

coefficients, in the order of the window (modified Gram-Schmidt)
    |H(k,j) - v_k . q_k| <= (n + 4) u sum_i |v_k,i| Q_k,i,   q_k = p - sum_{l < k in window} H(l,j) v_l,  Q_k = |p| + sum |H(l,j)||v_l|
  (n + 4) u bounds a sum of n products in ANY order - nothing is taken from the kernels' reduction trees - and Q_k
  holds the magnitude of the terms already taken off: the fused h2 = (b - h1 s1 g) s2 of DESIGN.md 4.2 cancels there.

normalisation   |sum_i v_{j+1,i}^2 - 1| <= (n + 6) u : n for the w.w partials and their finish, 2 + 2 for get_basis's
    1 / sqrt squared, 2 for its multiply squared.  Together with the relation this pins H(j+1,j).
AVNORM          |avnorm - ||A v_{m+1}||_2| <= (n + L_max + 6) u || |A||v_{m+1}| ||_2
begin_step, nrm2_w, asum_w: (n + 4) u relative to the exact sums;  restore_w: 4 u |w_i| per element
combine(mx, beta, y), c_i = beta sum_j y_j v_ij exact, B_i = (mx + 6) u |beta| sum_j |y_j||v_ij|:
    |w_i - max(c_i, 0)| <= B_i, an entry with |c_i| < B_i may be 0 or its value ("either way"), w >= 0 everywhere,
    |wsum - sum w_i| <= (n + 4) u sum w_i with w the device's own vector.
  (k_combine: coef = beta y_j / sqrt(sq) is 3 roundings, get_basis's column 3, the product 1, mx - 1 additions.)

Every check returns the ratio error / bound (worst element); a test prints them and asserts <= 1.  The case builders
are here too, so that the CPU tests (tests/test_krylov_ref.py) and the device tests (tests/test_gpu_krylov_relation.py)
see the same generators, start vectors and combine coefficients."""
import math
from fractions import Fraction

import numpy as np

from tests import row_ref as RR

U = 2.0 ** -53
LONG_OK = np.finfo(np.longdouble).nmant >= 63           # x87 extended or better; else exact rationals
M_PASS = 6                                              # m = min(6, n - 1) throughout
M_LONG = 9                                              # the restarted pass: arnoldi(6), then arnoldi(9, jold=6)


# ---- extended / exact arithmetic ---------------------------------------------------------------------------------------
class Arith:
    """arrays in np.longdouble (exact=False, needs LONG_OK) or as object arrays of fractions.Fraction (exact=True)"""

    def __init__(self, exact=None):
        self.exact = (not LONG_OK) if exact is None else bool(exact)
        assert self.exact or LONG_OK, "np.longdouble has fewer than 63 mantissa bits here: use exact=True"

    def arr(self, a):
        a = np.asarray(a, dtype=np.float64)
        if not self.exact:
            return a.astype(np.longdouble)
        return np.array([Fraction(t) for t in a.ravel().tolist()], dtype=object).reshape(a.shape)

    def num(self, x):
        return Fraction(float(x)) if self.exact else np.longdouble(x)

    def zeros(self, n):
        return np.array([Fraction(0)] * n, dtype=object) if self.exact else np.zeros(n, dtype=np.longdouble)

    def sqrt(self, x):
        if not self.exact:
            return np.sqrt(x)
        x = Fraction(x)                                  # to 2^-120 relative: far below u
        sh = 240 + 2 * max(0, -(math.floor(math.log2(x)) if x > 0 else 0))
        return Fraction(math.isqrt(int(x * (1 << sh))), 1 << (sh // 2))


def worst(err, bound):
    """max over the elements of |err| / bound as a float; 0 / 0 counts as 0, anything else over 0 as inf"""
    err, bound = np.atleast_1d(np.abs(err)), np.atleast_1d(bound)
    zero = bound == 0
    if np.any(zero & (err != 0)):
        return math.inf
    if np.all(zero):
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


class Generator:
    """the generator as row_ref's rows [(source, value)] and its diagonal (kept positive, like DIAG of the reference)"""

    def __init__(self, rows, diag, exact=None):
        self.ar = Arith(exact)
        self.n = len(rows)
        assert len(diag) == self.n
        self.L = np.array([len(r) for r in rows], dtype=np.int64)
        self.rr = np.repeat(np.arange(self.n), self.L)
        self.cc = np.array([c for r in rows for c, _ in r], dtype=np.int64)
        self.vv = self.ar.arr([v for r in rows for _, v in r])
        self.diag = self.ar.arr(diag)

    def apply(self, x):
        """(A x, |A||x|) for x in this generator's arithmetic"""
        p, pa = -(self.diag * x), np.abs(self.diag) * np.abs(x)
        if len(self.cc):
            t = self.vv * x[self.cc]
            np.add.at(p, self.rr, t)
            np.add.at(pa, self.rr, np.abs(t))
        return p, pa

    def apply64(self, x):
        """the product in plain doubles (for the case builders' own pass)"""
        p = -(np.asarray(self.diag, dtype=np.float64) * x)
        if len(self.cc):
            np.add.at(p, self.rr, np.asarray(self.vv, dtype=np.float64) * x[self.cc])
        return p


# ---- the checks --------------------------------------------------------------------------------------------------------
def window(j, qiop):
    """the columns column j is orthogonalised against (KrylovSolver.f90:241-246)"""
    return list(range(max(1, j - qiop + 1) if qiop > 0 else 1, j + 1))


def check_column(gen, j, basis, H, qiop=2):
    """Column j of a pass.  basis(k) -> normalised v_k as float64 (k = 1-based), H the (m+2, m+2) Hessenberg image
    (H[k-1, j-1] = H(k,j)).  -> {"relation", "coefficient", "normalisation"}: worst error / bound."""
    ar, n = gen.ar, gen.n
    win = window(j, qiop)
    v = {k: ar.arr(basis(k)) for k in win + [j + 1]}
    p, pa = gen.apply(v[j])
    q, qa = p.copy(), pa.copy()
    coef = 0.0
    for k in win:
        h = ar.num(H[k - 1, j - 1])
        coef = max(coef, worst(h - (v[k] * q).sum(), (n + 4) * U * (np.abs(v[k]) * qa).sum()))
        q = q - h * v[k]
        qa = qa + abs(h) * np.abs(v[k])
    h = ar.num(H[j, j - 1])
    r = q - h * v[j + 1]
    mag = qa + abs(h) * np.abs(v[j + 1])
    return {"relation": worst(r, (gen.L + 12 + 2 * len(win)) * U * mag),
            "coefficient": coef,
            "normalisation": worst((v[j + 1] * v[j + 1]).sum() - 1, (n + 6) * U)}


def check_avnorm(gen, v, avnorm):
    """AVNORM against ||A v||_2 for the normalised column v the product was taken from"""
    ar = gen.ar
    p, pa = gen.apply(ar.arr(v))
    return {"avnorm": worst(ar.num(avnorm) - ar.sqrt((p * p).sum()),
                            (gen.n + int(gen.L.max(initial=0)) + 6) * U * ar.sqrt((pa * pa).sum()))}


def check_begin(w, beta, v1, exact=None):
    """begin_step: beta = ||w||_2; column 1 is w / beta and has norm 1"""
    ar = Arith(exact)
    x, n = ar.arr(w), len(w)
    nrm = ar.sqrt((x * x).sum())
    v = ar.arr(v1)
    return {"beta": worst(ar.num(beta) - nrm, (n + 4) * U * nrm),
            "v1": worst(v * ar.num(beta) - x, 4 * U * np.abs(x)),
            "normalisation": worst((v * v).sum() - 1, (n + 6) * U)}


def check_reductions(w, nrm2, asum, exact=None):
    """nrm2_w and asum_w against the exact sums over the device's own w"""
    ar = Arith(exact)
    x, n = ar.arr(w), len(w)
    nrm, s = ar.sqrt((x * x).sum()), np.abs(x).sum()
    return {"nrm2_w": worst(ar.num(nrm2) - nrm, (n + 4) * U * nrm), "asum_w": worst(ar.num(asum) - s, (n + 4) * U * s)}


def check_restore(w, start, scale=1.0, exact=None):
    """restore_w(scale * beta) per element against scale * start, start the vector begin_step saw (k_scale_copy: the
    caller's product scale * beta, beta' / sqrt(sq_1) and the multiply: 3 roundings)"""
    ar = Arith(exact)
    expected = ar.num(scale) * ar.arr(start)
    return {"restore_w": worst(ar.arr(w) - expected, 4 * U * np.abs(expected))}


def combine_exact(V, beta, y, exact=None):
    """c_i = beta sum_j y_j v_ij and B_i = (mx + 6) u |beta| sum_j |y_j||v_ij| for the columns V[j] (float64)"""
    ar = Arith(exact)
    mx = len(V)
    c, a = ar.zeros(len(V[0])), ar.zeros(len(V[0]))
    for j in range(mx):
        t = ar.num(y[j]) * ar.arr(V[j])
        c, a = c + t, a + np.abs(t)
    return ar.num(beta) * c, (mx + 6) * U * abs(ar.num(beta)) * a


def combine_fractions(c, B):
    """(clamped, positive, either way) as fractions of the entries: what a combine case must offer"""
    either = np.abs(c) < B
    n = len(c)
    return float(((c < 0) & ~either).sum()) / n, float(((c > 0) & ~either).sum()) / n, float(either.sum()) / n


def check_combine(V, beta, y, w, wsum, exact=None):
    """w = max(beta V y, 0) and its sum.  -> {"combine", "wsum", "negative" (count), "either_way" (fraction)}"""
    ar = Arith(exact)
    c, B = combine_exact(V, beta, y, exact)
    x = ar.arr(w)
    clamped = np.where(c < 0, 0 * c, c)
    err = np.abs(x - clamped)
    either = np.abs(c) < B
    if either.any():                                     # 0 or its value: the nearer of the two counts
        err = np.where(either, np.minimum(np.abs(x), np.abs(x - c)), err)
    s = x.sum()
    return {"combine": worst(err, B), "wsum": worst(ar.num(wsum) - s, (len(w) + 4) * U * s),
            "negative": int((np.asarray(w) < 0).sum()), "either_way": combine_fractions(c, B)[2]}


def merge(into, ratios):
    """keep the worst ratio per bound"""
    for k, r in ratios.items():
        into[k] = max(into.get(k, 0.0), r)
    return into


def check_pass(gen, basis, H, first, last, qiop=2, into=None):
    """columns first..last of a pass, worst ratio per bound"""
    out = {} if into is None else into
    for j in range(first, last + 1):
        merge(out, check_column(gen, j, basis, H, qiop))
    return out


def assert_ok(ratios, what=""):
    bad = {k: r for k, r in ratios.items() if k not in ("either_way", "negative") and not r <= 1.0}
    assert not bad, f"{what}: beyond its bound by the factor {bad} (all: {ratios})"
    assert ratios.get("negative", 0) == 0, f"{what}: {ratios['negative']} negative entries after the clamp"
    assert ratios.get("either_way", 0.0) <= 0.01, f"{what}: {ratios['either_way']} of the entries fall under 'either way'"


def fmt(ratios):
    return " ".join(f"{k}={v:.3g}" for k, v in sorted(ratios.items()))


# ---- a pass in plain doubles (the builders' own; the CPU tests mutate it) -------------------------------------------------
def plain_pass(gen, w, m, qiop=2, mutate=None):
    """Literal modified Gram-Schmidt IOP pass in numpy doubles from the start vector w -> (beta, V [n, m + 2], H [m + 2,
    m + 2], avnorm), V's column m + 1 (0-based) the unnormalised A v_{m+1}.  mutate(name, j, ...) may replace a scalar:
    see tests/test_krylov_ref.py."""
    mu = mutate or (lambda name, j, value, **kw: value)
    n = gen.n
    beta = float(np.sqrt((w * w).sum()))
    V = np.zeros((n, m + 2))
    H = np.zeros((m + 2, m + 2))
    V[:, 0] = w / beta
    for j in range(1, m + 1):
        p = gen.apply64(V[:, j - 1])
        x = p.copy()
        for k in window(j, qiop):
            h = mu("h", j, float(V[:, k - 1] @ x), k=k, v=V[:, k - 1], x=x, p=p, V=V, H=H)
            H[k - 1, j - 1] = h
            x = x - h * V[:, k - 1]
        nrm = mu("norm", j, float(np.sqrt(x @ x)), x=x)
        H[j, j - 1] = nrm
        V[:, j] = x / nrm
    V[:, m + 1] = gen.apply64(V[:, m])
    H[m + 1, m] = 1.0
    return beta, V, H, float(np.sqrt(V[:, m + 1] @ V[:, m + 1]))


# ---- cases ---------------------------------------------------------------------------------------------------------------
GENERAL_N = (2, 3, 63, 64, 65, 129, 513, 2047, 2049, 4095, 4096, 4097, 8193)
BANDED_N = (131, 4095, 4097)
BOXES = ("toggle", "repressilator", "birth_death6")
BOX_DIMS = {"toggle": (33, 27), "repressilator": (31, 24, 19), "birth_death6": (5, 6, 4, 5, 4, 7)}
# boxes for the fused modes of the slab kernel (format 8: lines of an even number of rows; BOX_DIMS' repressilator has
# lines of 31) and of the pencil kernel under a tiled base-trip order; (kind, dims).  slab_narrow: 3 lines, so a workgroup
# has at most 3 wavefronts - fewer than the four of the kernels whose sum of the incoming partials it must repeat;
# slab_large: 196 608 rows, whose streaming kernels hand on MORE partials than a wavefront has lanes (box_cases.vec_grid)
GATED_BOXES = {"repressilator_even": ("repressilator", (30, 23, 19)), "slab_narrow": ("birth_death", (8, 8, 8, 4, 3, 2)),
               "slab_large": ("birth_death", (16, 16, 16, 8, 3, 2)), "tile_order": ("birth_death", (8, 8, 8, 8, 2, 2))}
COMBINE_MX = (1, 2, 3, 4, 5, 7, 8, M_LONG + 1)
_cache = {}


class Case:
    """name, n, m, how to upload it (upload(ctx)), its rows for the restatement (gen(), built once), the start vector"""

    def __init__(self, name, n, upload, rows, diag, w):
        self.name, self.n, self.upload, self.w = name, n, upload, w
        self.m = min(M_PASS, n - 1)
        self._rows, self._diag, self._gen = rows, diag, None

    def gen(self, exact=None):
        if exact:
            return Generator(self._rows, self._diag, exact=True)
        if self._gen is None:
            self._gen = Generator(self._rows, self._diag)
        return self._gen

    def reference(self, m=None):
        """the builders' own pass in doubles: (beta, V, H, avnorm)"""
        m = self.m if m is None else m
        key = (self.name, "pass", m)
        if key not in _cache:
            _cache[key] = plain_pass(self.gen(), self.w, m)
        return _cache[key]

    def check_conditions(self):
        """no happy breakdown within the columns a test asks for: every H(j+1,j) far above the solver's 1e-7"""
        m = min(M_LONG, self.n - 1)
        _, _, H, _ = self.reference(m)
        sub = np.array([H[j, j - 1] for j in range(1, m + 1)])
        assert np.all(sub > 1e-4 * np.abs(H).max()), (self.name, sub)
        assert np.all(self.w > 0)


def _start_vector(n, rng):
    return rng.random(n) + 0.05                          # generic and positive


def general_case(n):
    """random reference-layout generator of width 4: propensities 10^-3 .. 10^2, about a fifth of the links absent (0:
    outside the FSP, -1: no such reaction), DIAG the sum over all four slots as the reference assembles it"""
    key = ("general", n)
    if key not in _cache:
        rng = np.random.default_rng(7100 + n)
        adj = rng.integers(1, n + 1, size=(n, 4)).astype(np.int32)
        u = rng.random((n, 4))
        adj[u > 0.8] = 0
        adj[u > 0.9] = -1
        if not (adj > 0).any():
            adj[0, 0] = n                                # (n = 2, 3: keep at least one link)
        off = 10.0 ** rng.uniform(-3.0, 2.0, size=(n, 4))
        diag = off.sum(axis=1)
        c = Case(f"general{n}", n, lambda ctx: ctx.set_matrix_ell(adj, off, diag), RR.gather_rows(adj, off, diag), diag,
                 _start_vector(n, rng))
        c.ell = (adj, off, diag)
        c.check_conditions()
        _cache[key] = c
    return _cache[key]


def banded_case(n, levels=0):
    """random banded CSR generator in the style of _random_banded_csr (tests/test_gpu_edge_cases.py): random offsets, odd
    and even, +-1 among them, nine tenths of every diagonal present.  Six offsets are near (|d| <= 40) and three anywhere
    up to beyond the matrix: far diagonals are short and leave whole 128-row groups empty (the masked form), but too
    many of them and the library keeps the rows as SELL (it stores diagonals while nd * n <= 1.5 * entries + 1024;
    asserted below, so that the banded kernels are what these cases run).  levels > 0: every diagonal takes its values
    from that many distinct ones, which the dictionary-coded banded form (format 9) can hold at 4097 rows."""
    key = ("banded", n, levels)
    if key not in _cache:
        assert n >= 130
        rng = np.random.default_rng(7200 + n)
        deltas = np.unique(np.concatenate([rng.integers(-n - 5, n + 6, 3), rng.integers(-40, 41, 6), [(-1) ** n]]))
        deltas = deltas[deltas != 0]
        rows = np.arange(n)
        cols_l, vals_l = [rows], [-(10.0 ** rng.uniform(-1.0, 2.0, n))]
        for d in deltas:
            c = rows + d
            ok = (c >= 0) & (c < n) & (rng.random(n) < 0.9)
            cols_l.append(np.where(ok, c, -1))
            v = 10.0 ** rng.uniform(-3.0, 2.0, n)
            if levels:                                    # few distinct values per diagonal: what the coded banded form holds
                v = v[:levels][rng.integers(0, levels, n)]
            vals_l.append(np.where(ok, v, 0.0))
        C, V = np.stack(cols_l, 1), np.stack(vals_l, 1)
        order = np.argsort(np.where(C < 0, 1 << 40, C), axis=1, kind="stable")
        C, V = np.take_along_axis(C, order, 1), np.take_along_axis(V, order, 1)
        valid = C >= 0
        rowptr = np.concatenate(([0], np.cumsum(valid.sum(1)))).astype(np.int64)
        col, val = C[valid].astype(np.int32), V[valid]
        used = sum(1 for d in deltas if abs(d) < n)
        assert used * n <= 1.5 * (len(val) - n) + 1024, deltas
        assert n < 512 or any(256 < abs(d) < n for d in deltas), deltas         # a diagonal with empty 128-row groups
        r, dg = RR.rows_from_csr(n, rowptr, col, val)
        c = Case(f"banded{n}" + ("q" if levels else ""), n, lambda ctx: ctx.set_matrix_csr(n, rowptr, col, val), r, dg, _start_vector(n, rng))
        c.csr = (rowptr, col, val)
        c.check_conditions()
        _cache[key] = c
    return _cache[key]


def box_model(name):
    from krylovfspssa_amd import synth
    if name in GATED_BOXES:
        kind, dims = GATED_BOXES[name]
        return synth.repressilator(dims=dims) if kind == "repressilator" else synth.birth_death(dims)
    dims = BOX_DIMS[name]
    return {"toggle": lambda: synth.toggle(*dims), "repressilator": lambda: synth.repressilator(dims=dims),
            "birth_death6": lambda: synth.birth_death(dims)}[name]()


def box_case(name):
    """a small box with odd extents per matrix-free form; the rows are the model's own uploaded arrays (mdl.ell())"""
    key = ("box", name)
    if key not in _cache:
        mdl = box_model(name)
        adj, off, diag = mdl.ell()
        rng = np.random.default_rng(7300 + mdl.n)
        c = Case(f"box_{name}", mdl.n, lambda ctx: ctx.set_matrix_box(mdl), RR.gather_rows(adj, off, diag), diag,
                 _start_vector(mdl.n, rng))
        c.mdl, c.ell = mdl, (adj, off, diag)
        c.check_conditions()
        _cache[key] = c
    return _cache[key]


def golden_case(golden_dir, fixture="assembly_goutsias_k10.npz"):
    """a reference-assembled FSP from tests/golden"""
    import os
    key = ("golden", fixture)
    if key not in _cache:
        g = np.load(os.path.join(golden_dir, fixture))
        adj, off, diag = g["adj"], g["offdiag"], g["diag"]
        n = adj.shape[0]
        c = Case(fixture.split(".")[0], n, lambda ctx: ctx.set_matrix_ell(adj, off, diag), RR.gather_rows(adj, off, diag), diag,
                 _start_vector(n, np.random.default_rng(7400)))
        c.ell = (adj, off, diag)
        c.check_conditions()
        _cache[key] = c
    return _cache[key]


NEAR_MU = 300.0


def near_invariant_case(base, eps=None):
    """Cases on which the window is NOT orthogonal to rounding.  In an IOP pass every column is orthogonalised against
    the columns of its window, so v_j . v_{j-1} is of the order u ||A v_{j-1}|| / H(j,j-1): about 1e-15 on the generic
    cases above, where modified and classical Gram-Schmidt - and the fused h2 with this or the previous column's g -
    differ by h1 (v_j . v_{j-1}), far below any bound, so that nothing there shows a wrong g.  Here it is large: the
    generator is the base case's (a general, banded or golden one: anything uploaded as arrays) with another diagonal, diag_i = (sum_k a_ik x_k) / x_i + 300 for
    a random positive x, which makes x an eigenvector (A x = -300 x to rounding; no eigen-solver, any size), and the
    start vector is x + eps B^T x (B = A + 300 I): positive, A v_1 almost -300 v_1, H(2,1) about min(3e-5, 0.02 / n) (at least
    ten times the solver's breakdown threshold 1e-7; asserted), v_2 . v_1 between 1e-9 and 1e-7.  From column 2 on the pass
    is generic.  min_dot is a tenth of |v_2 . v_1| of the builders' own pass: what a device test asks of the device's."""
    key = ("near_invariant", base.name)
    if key not in _cache:
        n, kind = base.n, "general" if hasattr(base, "ell") else "banded"
        rng = np.random.default_rng(7600 + n)
        x = rng.random(n) + 0.5
        g0 = Generator(base._rows, np.zeros(n))
        diag = g0.apply64(x) / x + NEAR_MU
        if kind == "general":
            adj, off, _ = base.ell
            upload = lambda ctx: ctx.set_matrix_ell(adj, off, diag)
            rows = base._rows
        else:
            rowptr, col, val = base.csr
            val = val.copy()
            val[col == np.repeat(np.arange(n), np.diff(rowptr))] = -diag
            upload = lambda ctx: ctx.set_matrix_csr(n, rowptr, col, val)
            rows, dg = RR.rows_from_csr(n, rowptr, col, val)
            assert np.array_equal(np.asarray(dg), diag)
        # the perturbation: along B^T x, B = A + 300 I.  Then v_2 is along B B^T x and H(1,2) = (B^T v_1) . v_2 is a
        # quadratic form of B, of the size of the propensities - a random direction would leave H(1,2), and with it what
        # a wrong g does to H(2,2), n^-1/2 of that
        d = -g0.apply64(x)                                # - (sum_k a_ik x_k): the diagonal of B times x
        np.add.at(d, g0.cc, np.asarray(g0.vv, dtype=np.float64) * x[g0.rr])
        d *= np.sqrt(x @ x) / np.sqrt(d @ d)
        if eps is None:                                   # H(2,1) is linear in eps: one trial pass sets it
            trial = plain_pass(Generator(rows, diag), x + 1e-4 * d, 1)[2][1, 0]
            eps = 1e-4 * min(3e-5, 0.02 / n) / trial
        c = Case(f"near_{base.name}", n, upload, rows, diag, x + eps * d)
        if kind == "general":
            c.ell = (adj, off, diag)
        else:
            c.csr = (rowptr, col, val)
        _, V, H, _ = c.reference(min(M_LONG, n - 1))
        sub = np.array([H[j, j - 1] for j in range(1, min(M_LONG, n - 1) + 1)])
        c.min_dot = 0.1 * abs(V[:, 0] @ V[:, 1])
        assert sub.min() > 1e-6 and 1e-6 < H[1, 0] < 1e-3 and c.min_dot > 1e-12 and np.all(c.w > 0), (sub, c.min_dot)
        _cache[key] = c
    return _cache[key]


def combine_coefficients(case, mx):
    """(beta', y) for combine(mx): y of both signs and beta' != 1 such that, on the builders' own basis, at least 10 % of
    the exact entries are clamped, at least 10 % stay positive and at most 1 % fall under "either way".  The first
    draw of a fixed sequence that offers this is taken.  mx = 1 has only the positive column v_1 to offer: y_1 > 0, all
    entries positive (no y of one entry gives both)."""
    key = (case.name, "y", mx)
    if key not in _cache:
        m = min(M_LONG, case.n - 1)
        assert mx <= m + 1
        beta, V, _, _ = case.reference(m)
        cols = [V[:, j] for j in range(mx)]
        for draw in range(64):
            rng = np.random.default_rng(7500 + 97 * mx + draw)
            y = rng.standard_normal(mx)
            y[0] = abs(y[0]) * 0.3                       # v_1 is positive and dominates: keep it from deciding every sign
            b = 0.75 * beta
            neg, pos, either = combine_fractions(*combine_exact(cols, b, y))
            if mx == 1 and pos == 1.0 and either == 0.0:
                break
            if neg >= 0.1 and pos >= 0.1 and either <= 0.01 and y.min() < 0 < y.max():
                break
        else:
            raise AssertionError(f"{case.name}: no combine coefficients for mx = {mx}")
        _cache[key] = (b, y)
    return _cache[key]
