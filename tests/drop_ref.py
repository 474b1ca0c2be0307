"""DROP_STATES restated plainly (StateSpace.f90:398-548), and the inputs on which the device is held to it.

The first half is the restatement: plain Python and numpy, nothing of the library.

    find_droptol   thresholds 1e-8, /10, /10, ... (the divisions the library makes, so the same doubles); S(tol) is the
                   sum of the entries with 0 < w < tol; the first tol with S < dsum (:416-426)
    decide         marked = w < tol, guarded = (A w) > 1e-8, dropped = marked and not guarded; the counter of the
                   reference is #marked - #guarded whether or not a guarded state was marked (:475-497)
    compact_lists  kept states move up in order, links are renumbered, a link to a dropped state becomes 0, -1 and 0
                   stay, slots beyond the reaction count are copied untouched (:500-546)
    exact_product  A w as exact rationals, for the margin conditions only

Every function takes keyword flags that make it WRONG in one named way.  They exist so that tests/test_drop_ref.py can
show, on the CPU, that each case of tests/test_gpu_drop_edges.py tells the wrong answer from the right one.

The second half makes those cases.  Two designs keep every comparison exact:

  * small entries are integers (at most 2^20) times 2^-60: any sum of fewer than 2^33 of them is exact in any order;
  * generators whose rows hold one entry of 1.0 and a zero diagonal: (A w)_r is w[source of r] on the bits (a row
    without an entry gives a zero), so the guard compares a number the test knows exactly.

For everything else a case must satisfy margin_ok and guard_clear below, asserted on the CPU from this file alone."""
import functools
import math
from fractions import Fraction

import numpy as np

TOL0 = 1.0e-8                 # the first threshold
GUARD = 1.0e-8                # the derivative guard
UNIT = 2.0 ** -60             # the dyadic unit of the small entries
KMAX = 2 ** 20                # their largest multiple
EPS = 2.0 ** -52


def nxt(x):
    return float(np.nextafter(x, np.inf))


def prv(x):
    return float(np.nextafter(x, -np.inf))


def threshold(level):
    """the double the library reaches after `level` divisions by ten"""
    tol = TOL0
    for _ in range(level):
        tol = tol / 10.0
    return tol


# ---- the restatement ------------------------------------------------------------------------------------------------------
def level_sum(w, tol, sum_le=False, positive_only=True):
    """S(tol): the correctly rounded sum (math.fsum) of the entries with 0 < w < tol.
    Wrong: sum_le - w <= tol; positive_only=False - the condition 0 < w left out"""
    w = np.asarray(w, dtype=np.float64)
    sel = (w <= tol) if sum_le else (w < tol)
    if positive_only:
        sel = sel & (w > 0.0)
    return math.fsum(w[sel].tolist())


def find_droptol(w, dsum, sum_le=False, stop_le=False, positive_only=True, stale=(), levels=None):
    """-> (droptol, margin): the first threshold whose sum is below dsum, and the smallest |S - dsum| over the levels
    visited (a test asserts that this margin is beyond any rounding of a sum taken in another order).  levels: a list
    that receives (tol, S) of every level visited.
    Wrong: sum_le, positive_only (level_sum); stop_le - S <= dsum ends the search; stale - entries left in the pad rows
    of the resident vector by a larger generator, summed as if they were states"""
    assert dsum > 0.0
    w = np.concatenate([np.asarray(w, dtype=np.float64), np.asarray(stale, dtype=np.float64)])
    tol, margin = TOL0, math.inf
    while True:
        s = level_sum(w, tol, sum_le=sum_le, positive_only=positive_only)
        margin = min(margin, abs(s - dsum))
        if levels is not None:
            levels.append((tol, s))
        if (s <= dsum) if stop_le else (s < dsum):
            return tol, margin
        tol = tol / 10.0


def decide(w, aw, tol, mark_le=False, guard_ge=False, count_is_nflag=False):
    """-> (drop, count, nflag): the flags (bool), the reference's DROP_COUNT and the number of flags.
    Wrong: mark_le - w <= tol; guard_ge - (A w) >= 1e-8; count_is_nflag - the counter counts the flags"""
    w, aw = np.asarray(w, dtype=np.float64), np.asarray(aw, dtype=np.float64)
    marked = (w <= tol) if mark_le else (w < tol)
    guarded = (aw >= GUARD) if guard_ge else (aw > GUARD)
    drop = marked & ~guarded
    nflag = int(drop.sum())
    count = nflag if count_is_nflag else int(marked.sum()) - int(guarded.sum())
    return drop, count, nflag


def compact_lists(state, adj, off, diag, w, keep, nr=None, dropped_as=0, shift=0, renumber_all=False):
    """-> (state, adj, off, diag, w) of the kept states, in order (an argument given as None comes back as None).
    adj and off are [state][slot] with at least nr slots (nr=None: all of them are reactions); slot k < nr holds the
    1-based target, 0 (outside the FSP) or -1 (a negative population).  Slots k >= nr - the padding of a leading dimension
    larger than the reaction count - are copied as they are.
    Wrong: dropped_as - what a link to a dropped state becomes (-1 for 0); shift - added to every renumbered link;
    renumber_all - the padding slots renumbered too"""
    keep = np.asarray(keep, dtype=bool)
    n = len(keep)
    newidx = np.full(n + 1, dropped_as, dtype=np.int64)
    newidx[1:][keep] = np.arange(1, int(keep.sum()) + 1) + shift
    adj2 = np.array(adj, dtype=np.int32)[keep]
    cols = adj2.shape[1] if (nr is None or renumber_all) else nr
    part = adj2[:, :cols]
    pos = part > 0
    part[pos] = newidx[np.clip(part[pos], 0, n)]
    pick = lambda a: None if a is None else np.array(a)[keep]        # noqa: E731
    return pick(state), adj2, pick(off), pick(diag), pick(w)


def exact_product(rows, diag, w):
    """rows: per row the (source, value) pairs (tests/row_ref.py gather_rows / rows_from_csr), diag the positive
    diagonal -> (aw, mass): (A w)_r = sum_j a_rj w_j - diag_r w_r and sum_j |a_rj w_j| + |diag_r w_r| as Fractions"""
    wf = [Fraction(float(x)) for x in w]
    aw, mass = [], []
    for r, row in enumerate(rows):
        d = Fraction(float(diag[r])) * wf[r]
        terms = [Fraction(float(v)) * wf[c] for c, v in row]
        aw.append(sum(terms, -d))
        mass.append(sum((abs(t) for t in terms), abs(d)))
    return aw, mass


def margin_ok(w, dsum):
    """|S_k - dsum| > n 2^-52 S_k at every level the search visits: a sum of n positive terms taken in any order is
    within n 2^-52 S of S, so no order of summation moves a decision"""
    levels = []
    find_droptol(w, dsum, levels=levels)
    n = len(w)
    return all(abs(Fraction(s) - Fraction(dsum)) > Fraction(n * EPS) * Fraction(s) for _, s in levels)


def guard_clear(aw, mass):
    """|(A w)_r - 1e-8| > 64 2^-52 sum_j |a_rj w_j| for every row: no product kernel's rounding moves the guard"""
    g = Fraction(GUARD)
    return all(abs(a - g) > Fraction(64 * EPS) * m for a, m in zip(aw, mass))


def dyadic_exact(w, tol=TOL0):
    """every entry that can enter a threshold sum is a multiple (at most 2^20) of 2^-60: the sums are exact"""
    w = np.asarray(w, dtype=np.float64)
    s = w[(w > 0.0) & (w < tol)] / UNIT
    return bool(np.all(s == np.round(s)) and np.all(s <= KMAX) and len(s) < 2 ** 32)


# ---- generators with one entry of 1.0 per row ----------------------------------------------------------------------------
def cycle_ell(n, seed, tail=48):
    """reference arrays (adj, off, diag) of n states and two slots.  Slot 0 of state i links to the next state of one
    cycle through all states (off 1.0) - the cycle runs through the first n - tail states in random order and through
    the last `tail` in index order, so that the rows at the end of the last 64-row chunk have known neighbours.  Slot 1
    never links: 0 and -1 alternate, its off is 0.25.  diag is zero.  n = 1: no link."""
    rng = np.random.default_rng(seed)
    head = max(0, n - tail)
    order = np.concatenate([rng.permutation(head), np.arange(head, n)])
    adj = np.zeros((n, 2), dtype=np.int32)
    if n > 1:
        adj[order, 0] = np.roll(order, -1) + 1
    adj[1::2, 1] = -1
    off = np.empty((n, 2))
    off[:, 0], off[:, 1] = 1.0, 0.25
    return adj, off, np.zeros(n)


def chain_ell(n, up):
    """state i links to i + 1 (up) or to i - 1; the last (first) state links nowhere"""
    adj = np.zeros((n, 2), dtype=np.int32)
    i = np.arange(n)
    adj[:, 0] = np.where(i + 1 < n, i + 2, 0) if up else i        # i - 1, 1-based; state 0: 0
    adj[1::2, 1] = -1
    off = np.empty((n, 2))
    off[:, 0], off[:, 1] = 1.0, 0.25
    return adj, off, np.zeros(n)


def shift_csr(n, row0=0, nloc=None):
    """CSR rows [row0, row0 + nloc) of the generator whose row r holds 1.0 in column r + 1 (the last row holds
    nothing) and an explicit zero on the diagonal: one full diagonal, the banded form"""
    nloc = n - row0 if nloc is None else nloc
    r = np.arange(row0, row0 + nloc, dtype=np.int64)
    full = r + 1 < n
    rowptr = np.concatenate([[0], np.cumsum(1 + full)]).astype(np.int64)
    col = np.empty(int(rowptr[-1]), dtype=np.int32)
    val = np.zeros(int(rowptr[-1]))
    col[rowptr[:-1]] = r
    col[rowptr[:-1][full] + 1] = r[full] + 1
    val[rowptr[:-1][full] + 1] = 1.0
    return rowptr, col, val


def sources_ell(adj, nr=None):
    """src[r] = the one state that links to r, -1 where none does (asserts that no row has two)"""
    adj = np.asarray(adj)[:, :nr]
    n = len(adj)
    src = np.full(n, -1, dtype=np.int64)
    i, k = np.nonzero(adj > 0)
    t = adj[i, k] - 1
    assert len(np.unique(t)) == len(t), "a row with two entries"
    src[t] = i
    return src


def sources_shift(n):
    src = np.arange(1, n + 1, dtype=np.int64)
    src[-1] = -1
    return src


def moved(w, src):
    """(A w) of such a generator: w[src[r]], +0.0 where a row has no entry"""
    w = np.asarray(w, dtype=np.float64)
    return np.where(src >= 0, w[np.maximum(src, 0)], 0.0)


# ---- vectors ----------------------------------------------------------------------------------------------------------------
def specials():
    """the entries a comparison can trip over, the ones the first cases need first"""
    out = [GUARD, nxt(GUARD), prv(GUARD)]
    for level in (2, 1, 3, 4):
        t = threshold(level)
        out += [t, prv(t), nxt(t)]
    return out + [0.0, -0.0, -3.0e-9, 5e-324, 1.0]


def fill_vector(n, rng, small=0.45, nonpositive=True):
    """dyadic small entries, entries in [1e-6, 1), and (nonpositive) a few zeros and negative entries of either size"""
    u = rng.random(n)
    w = np.where(u < small, rng.integers(1, KMAX + 1, size=n) * UNIT, 10.0 ** rng.uniform(-6.0, 0.0, size=n))
    if nonpositive:
        w[(u > 0.90) & (u <= 0.93)] = 0.0
        neg = u > 0.97
        w[neg] = -w[neg]
    return w


def edge_vector(n, src, starts, seed):
    """fill_vector with the specials laid along the chains of sources that begin at `starts`: row, its source, the
    source's source, ... get small, special, small, special, ... - every special is the A w of a marked state (the guard
    meets it) and is itself a state whose own A w is small (the mark meets it, unguarded)"""
    rng = np.random.default_rng(seed)
    w = fill_vector(n, rng)
    if n == 1:
        w[0] = TOL0                   # the one state sits ON the first threshold: not marked
        return w
    used = np.zeros(n, dtype=bool)
    for start in starts:
        x = int(start)
        for sp in specials():
            for value in (int(rng.integers(1, KMAX + 1)) * UNIT, sp):
                if x < 0 or used[x]:
                    break
                w[x], used[x] = value, True
                x = int(src[x])
        if 0 <= x and not used[x]:
            w[x], used[x] = int(rng.integers(1, KMAX + 1)) * UNIT, True
    return w


def pick_dsum(w, level):
    """a dsum half way between S(level - 1) and S(level), so that the search ends at `level` with the widest margin; where
    those two sums are equal, the nearest lower level that has a gap, and twice S(0) (or 1e-9) for level 0"""
    s = [level_sum(w, threshold(k)) for k in range(level + 1)]
    while level > 0 and not s[level - 1] > s[level]:
        level -= 1
    if level == 0:
        return 2.0 * s[0] if s[0] > 0.0 else 1.0e-9
    return s[level] + (s[level - 1] - s[level]) / 2.0


def decade_vector(n, levels, seed):
    """one entry of 3 tol_j for every j in 1..levels (it lies between tol_j and tol_{j-1}), the rest at least 1e-6 or
    negative: S_k = 3 (tol_{k+1} + tol_{k+2} + ...) is about tol_k / 3, so dsum = 2 tol_K is first undercut at level K"""
    rng = np.random.default_rng(seed)
    w = 10.0 ** rng.uniform(-6.0, 0.0, size=n)
    w[rng.random(n) < 0.2] *= -1.0
    at = rng.permutation(n)[:levels]
    for j in range(1, levels + 1):
        w[at[j - 1]] = 3.0 * threshold(j)
    return w


def on_threshold_vector(n, seed):
    """the only positive entries sit exactly on the thresholds of levels 0..5; the rest is zero or negative"""
    rng = np.random.default_rng(seed)
    w = np.where(rng.random(n) < 0.5, 0.0, -(10.0 ** rng.uniform(-12.0, 0.0, size=n)))
    at = rng.permutation(n)[:6]
    for j in range(6):
        w[at[j]] = threshold(j)
    return w


def dyadic_vector(n, seed):
    """every entry k 2^-60 with 1 <= k <= 2^20 (at most 9.1e-13): the sums of levels 0..4 take all of them, level 5
    (1e-13) about a ninth, and each is exact in any order"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, KMAX + 1, size=n) * UNIT


def general_vector(n, seed):
    """for general generators: a third dyadic small entries, a tenth between 2e-10 and 9e-10 (they separate S(1e-9) from
    S(1e-10)), the rest around 1e-3; all positive (tests/row_ref.py wants no subnormal product)"""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    w = np.where(u < 0.35, rng.integers(1, KMAX + 1, size=n) * UNIT, rng.uniform(0.5, 1.5, size=n) * 1.0e-3)
    mid = u > 0.9
    w[mid] = rng.uniform(2.0e-10, 9.0e-10, size=int(mid.sum()))
    return w


# ---- the reference's own vectors and fixtures (oracle/ref_dump.f90) ---------------------------------------------------------
RECORDED_DROPS = (("toggle", 20, 1e-6), ("goutsias", 12, 1e-7), ("goutsias", 16, 1e-12), ("repressilator", 10, 1e-4))


def recorded_drop_name(name, k, dsum):
    """file name of the fixture the reference's DROP_STATES run left (oracle/make_golden.py writes it)"""
    return f"drop_{name}_k{k}_dsum{dsum:g}.npz"


def spread_vector(n):
    """SPREAD_VECTOR + the edits of DO_DROPTOL (1-based strides): the vector of fixture droptol.npz"""
    i = np.arange(1, n + 1, dtype=np.float64)
    u = i * 0.6180339887498949
    u = u - np.trunc(u)
    w = 10.0 ** (-2.0 - 14.0 * u)
    w[6::13] = 0.0
    w[4::17] = -w[4::17]
    w[2::11] = w[2::11] * 1.0e-12
    return w


def decaying_vector(n):
    """the vector of DO_DROP: eighteen decades down the list, every seventh entry a thousand times larger"""
    i = np.arange(1, n + 1, dtype=np.float64)
    w = 10.0 ** (-2.0 - 18.0 * (i - 1.0) / max(n - 1, 1))
    w[6::7] *= 1.0e3
    return w


# ---- the expected answer of a case ------------------------------------------------------------------------------------------
def expected(w, aw, dsum):
    """-> dict(tol, margin, drop, count, nflag, keep) from the restatement"""
    tol, margin = find_droptol(w, dsum)
    drop, count, nflag = decide(w, aw, tol)
    return dict(tol=tol, margin=margin, drop=drop, count=count, nflag=nflag, keep=~drop)


# ---- the cases of tests/test_gpu_drop_edges.py, made once per process and left alone ----------------------------------------
REMAINDERS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 4097)
N_TURN = 262209               # 4 x 65 536 + 65: more than 1024 x 256 lanes, and odd
N_GRID = 8193                 # with vec_grid_blocks 1 and 3 the threshold sums stride over it
LEVEL = 2                     # the level the searches of the permutation cases are aimed at (droptol 1e-10)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def perm_case(kind, n, level=LEVEL):
    """kind "ell": cycle_ell for set_matrix_ell; "csr": shift_csr for set_matrix_csr.  -> the generator, src, w (edge_vector:
    one chain of specials ends in the last rows, from n = 200 on another lies elsewhere), aw, dsum and expected()"""
    if kind == "ell":
        adj, off, diag = cycle_ell(n, seed=n)
        gen = dict(adj=adj, off=off, diag=diag)
        src = sources_ell(adj)
        starts = [n - 1] + ([n - 48] if n >= 200 else [])
    else:
        rowptr, col, val = shift_csr(n)
        gen = dict(rowptr=rowptr, col=col, val=val)
        src = sources_shift(n)
        starts = [max(0, n - 42)] + ([3] if n >= 200 else [])
    w = edge_vector(n, src, starts, seed=1000 + n)
    aw = moved(w, src)
    dsum = pick_dsum(w, level)
    return _frozen(dict(kind=kind, n=n, src=src, w=w, aw=aw, dsum=dsum, **gen, **expected(w, aw, dsum)))


def compacted(case):
    """the kept part of an "ell" perm_case: (adj, off, diag, w) by compact_lists"""
    _, adj, off, diag, w = compact_lists(None, case["adj"], case["off"], case["diag"], case["w"], case["keep"])
    return adj, off, diag, w


# (c) threshold batches: name -> (vector maker, dsum); all on shift_csr(N_BATCH)
N_BATCH = 200
BATCH_LEVELS = (0, 15, 16, 32)          # the 1st, 16th, 17th and 33rd level: the first, second and third batch of sixteen


@functools.lru_cache(maxsize=None)
def batch_case(name):
    n = N_BATCH
    if name.startswith("level "):
        w, dsum = decade_vector(n, 40, seed=5), 2.0 * threshold(int(name.split()[1]))
    elif name == "all zero":
        w, dsum = np.zeros(n), 1.0e-9
    elif name == "all negative":
        w, dsum = -fill_vector(n, np.random.default_rng(6), nonpositive=False), 1.0e-9
    elif name == "on thresholds":
        w, dsum = on_threshold_vector(n, seed=7), 5.0e-9
    else:
        # every S_k exact: dsum ON S_5 (the search must move on: S < dsum is false) and one unit in the last place above
        w = dyadic_vector(n, seed=8)
        s5 = level_sum(w, threshold(5))
        dsum = s5 if name == "dyadic, S == dsum" else nxt(s5)
        assert name in ("dyadic, S == dsum", "dyadic, dsum = next(S)")
    src = sources_shift(n)
    aw = moved(w, src)
    return _frozen(dict(n=n, src=src, w=w, aw=aw, dsum=dsum, **expected(w, aw, dsum)))


BATCH_NAMES = tuple(f"level {k}" for k in BATCH_LEVELS) + ("all zero", "all negative", "on thresholds", "dyadic, S == dsum",
                                                           "dyadic, dsum = next(S)")

# (d) stale memory
N_STALE_BIG = 8193
STALE_FILL = 1.0e-12
STALE_R = (0, 1, 62)


def stale_pad(n2):
    """the pad rows k_drop_sums reads behind n2 states: it sums whole 64-row chunks"""
    return (-n2) % 64


@functools.lru_cache(maxsize=None)
def stale_case(r):
    """The large generator: a cycle through 8193 states in index order (state i links to i + 1, the last to the first).
    W flags exactly 4096 - r chosen states when planned with dsum1: in groups of three - small, 2^-100, 2^-100 - the two
    tiny ones are flagged (their sources are small or tiny, so nothing guards them) and the small one stays: small entries
    are at least 2^11 units, above the 1e-15 the first search ends at.  The groups leave out rows n2 .. n2 + 63, which hold
    small entries, and stop when 4096 - r states are chosen; behind them: small and large entries.
    What is kept are n2 = 4097 + r states; their vector w2 is then planned with dsum2 = S_0(w2) + 2^10 units: the search ends
    at the first level (S_0 is exact), unless ONE more small entry is summed.  k_drop_sums reads the rows up to the next
    multiple of 64, stale_pad(n2) = 63, 62 and 1 rows behind w2; what they would hold if nothing cleared them:
      stale_step     1e-12 each - what the step on the large generator left (the route through kfsp_set_vector);
      stale_pending  W[n2 : n2 + pad], all small - kfsp_set_vector(W) for the first plan wrote them, and the compacted vector
                     is adopted over them (kfsp_drop_compact, then kfsp_set_matrix_ell or kfsp_drop_rebuild)."""
    n, n2 = N_STALE_BIG, 4097 + r
    ndrop = n - n2
    adj = np.zeros((n, 2), dtype=np.int32)
    adj[:, 0] = np.roll(np.arange(n), -1) + 1
    adj[1::2, 1] = -1
    off = np.empty((n, 2))
    off[:, 0], off[:, 1] = 1.0, 0.25
    diag = np.zeros(n)
    rng = np.random.default_rng(90 + r)
    small = rng.integers(2 ** 11, KMAX + 1, size=n) * UNIT
    large = 10.0 ** rng.uniform(-6.0, 0.0, size=n)
    W = np.where(rng.random(n) < 0.5, small, large)
    chosen = np.zeros(n, dtype=bool)
    i, left = 0, ndrop
    while left > 0:
        if n2 - 3 < i < n2 + 64:                         # no group reaches into the window: small entries up to its end
            W[i:n2 + 64] = small[i:n2 + 64]
            i = n2 + 64
            continue
        W[i] = small[i]
        take = min(2, left)
        chosen[i + 1:i + 1 + take] = True
        W[i + 1:i + 3] = small[i + 1:i + 3]
        i, left = i + 3, left - take
    assert i <= n and n2 + 64 <= i
    W[chosen] = 2.0 ** -100
    dsum1 = 1.0e-20
    src = sources_ell(adj)
    first = expected(W, moved(W, src), dsum1)
    _, adj2, off2, diag2, w2 = compact_lists(None, adj, off, diag, W, first["keep"])
    src2 = sources_ell(adj2)
    dsum2 = level_sum(w2, TOL0) + 2 ** 10 * UNIT
    second = expected(w2, moved(w2, src2), dsum2)
    pad = stale_pad(n2)
    return _frozen(dict(n=n, n2=n2, adj=adj, off=off, diag=diag, W=W, dsum1=dsum1, first=first, adj2=adj2, off2=off2,
                        diag2=diag2, w2=w2, src2=src2, dsum2=dsum2, second=second, chosen=chosen, pad=pad,
                        stale_step=np.full(pad, STALE_FILL), stale_pending=W[n2:n2 + pad].copy()))


# (e) every generator form: name -> what to upload, the options that reach the form, and the form expected
#     (layout_info format, dia_code_info active, DIAG folded)
FORMS = {
    "banded plain": ("csr", "toggle 70x61", dict(dia_mask=0, dia_code=0), (1, 0, False)),
    "banded masked": ("csr", "random banded 3", dict(dia_mask=1, dia_code=0), (2, 0, False)),
    "banded coded": ("csr", "toggle 70x61", dict(dia_mask=0, dia_code=1, dia_code_diag=0), (1, 1, False)),
    "banded folded": ("csr", "toggle 70x61", dict(dia_mask=0, dia_code=1, dia_code_diag=1), (1, 1, True)),
    "box matrix-free": ("box", "box_toggle_2x2", dict(box_pencil=0), (4, 0, False)),
    "box stored": ("box_store", "box_toggle_2x2", dict(dia_code=0), (1, 0, False)),
    "sell coded": ("ell", "local 1500x8", dict(sell_code=1, state_order=0), (5, 0, False)),
}


@functools.lru_cache(maxsize=None)
def form_case(name):
    """the product restated row by row (tests/row_ref.py) - the bits the device must produce -, the exact product for the
    guard margin, w = general_vector, dsum aimed at level 2"""
    from tests import box_cases as BC
    from tests import row_cases as RC
    from tests import row_ref as RR
    how, which, options, form = FORMS[name]
    out = dict(how=how, options=options, form=form)
    if how == "csr":
        c = RC.csr_case(which)
        n, rows, diag = c["n"], c["rows"], c["diag"]
        out.update(rowptr=c["rowptr"], col=c["col"], val=c["val"])
        w = general_vector(n, seed=40)
        aw = np.array(RR.spmv_exact(rows, diag, w))
    elif how == "ell":
        c = RC.ell_case(which)
        n, rows, diag = c["n"], c["rows"], c["diag"]
        out.update(adj=c["adj"], off=c["off"], diag=c["diag"])
        w = general_vector(n, seed=41)
        aw = np.array(RR.spmv_exact(rows, diag, w))
    else:
        mdl = BC.model(which)
        n = mdl.n
        out.update(mdl=mdl)
        w = general_vector(n, seed=42)
        if how == "box":
            per_row = RR.box_rows(mdl)
            aw = np.array(RR.box_exact(mdl, w))
        else:
            per_row = RR.box_generic_rows(mdl)
            aw = np.array(RR.box_generic_exact(mdl, w))
        rows = [[(s, a) for a, s in ent] for ent, _ in per_row]
        diag = [d for _, d in per_row]
    exact, mass = exact_product(rows, diag, w)
    dsum = pick_dsum(w, LEVEL)
    return _frozen(dict(n=n, w=w, aw=aw, exact=exact, mass=mass, dsum=dsum, **out, **expected(w, aw, dsum)))


# (f) partitions
PARTITION_N = (65, 449)       # over 4 ranks: blocks 64, 1, 0, 0 and 128, 128, 128, 65
PARTITION_P = (2, 3, 4)

# (g) extremes: name -> (up: the direction of chain_ell, w)
N_EXTREME = 130


@functools.lru_cache(maxsize=None)
def extreme_case(name):
    n = N_EXTREME
    rng = np.random.default_rng(70)
    small = rng.integers(1, KMAX + 1, size=n) * UNIT
    large = 10.0 ** rng.uniform(-6.0, 0.0, size=n)
    up = name == "all but the last"            # the state that stays must feed no row: its 1.0 would guard the row
    w = small.copy()
    if name == "nothing":
        w = large
    elif name == "all but the first":
        w[0] = 1.0
    elif name == "all but the last":
        w[-1] = 1.0
    else:
        assert name == "everything"
    adj, off, diag = chain_ell(n, up)
    src = sources_ell(adj)
    aw = moved(w, src)
    dsum = 1.0                                 # every sum is far below: droptol 1e-8
    return _frozen(dict(n=n, adj=adj, off=off, diag=diag, src=src, w=w, aw=aw, dsum=dsum, **expected(w, aw, dsum)))


EXTREMES = ("nothing", "all but the first", "all but the last", "everything")

# (h) renumbering: 100 random small FSPs
N_RANDOM = 100
PATTERNS = ("random", "first kept, last dropped", "alternating", "a kept block in the middle")


def keep_pattern(which, n, rng):
    i = np.arange(n)
    if which == "random":
        keep = rng.random(n) < rng.uniform(0.2, 0.9)
    elif which == "first kept, last dropped":
        keep = rng.random(n) < 0.5
        keep[0], keep[-1] = True, False
    elif which == "alternating":
        keep = i % 2 == 0
    else:
        lo = int(rng.integers(0, max(1, n // 2)))
        keep = (i >= lo) & (i < lo + max(1, n // 3))
    if not keep.any():
        keep[int(rng.integers(0, n))] = True
    return keep


@functools.lru_cache(maxsize=None)
def random_fsps():
    """drawn as tests/test_gpu_onestep.py draws its random networks: 1-4 species, 1-6 reactions with entries in [-2, 2],
    a random subset of a small box in random order; every link made (-1: a negative population, 0: not listed).  Rates
    in [0.01, 1).  The vector makes the device flag exactly the complement of the keep pattern: a dropped state holds a
    dyadic small entry, a kept one something in [5e-10, 1e-9) - at most six of them flow into a row, so every A w stays
    below 6e-9 and no state is guarded - and dsum lies half way between S(1e-9) and S(1e-10)."""
    rng = np.random.default_rng(177)
    out = []
    for case in range(N_RANDOM):
        ns, nr = int(rng.integers(1, 5)), int(rng.integers(1, 7))
        nu = rng.integers(-2, 3, size=(nr, ns)).astype(np.int32)
        side = int(rng.integers(2, 6))
        box = np.array(np.meshgrid(*[np.arange(side)] * ns, indexing="ij")).reshape(ns, -1).T
        listed = rng.random(len(box)) < rng.uniform(0.2, 1.0)
        listed[int(rng.integers(0, len(box)))] = True
        if listed.sum() < 2:
            listed[:2] = True
        state = box[listed][rng.permutation(int(listed.sum()))].astype(np.int32)
        n = len(state)
        idx = {tuple(s): i + 1 for i, s in enumerate(state.tolist())}
        adj = np.zeros((n, nr), dtype=np.int32)
        for j, s in enumerate(state):
            for k in range(nr):
                y = s + nu[k]
                adj[j, k] = -1 if y.min() < 0 else (0 if not nu[k].any() else idx.get(tuple(y.tolist()), 0))
        off = rng.uniform(0.01, 1.0, size=(n, nr))
        diag = off.sum(axis=1)
        keep = keep_pattern(PATTERNS[case % len(PATTERNS)], n, rng)
        w = np.where(keep, rng.uniform(5.0e-10, 1.0e-9, size=n), rng.integers(1, KMAX + 1, size=n) * UNIT)
        dsum = pick_dsum(w, LEVEL)
        out.append(_frozen(dict(ns=ns, nr=nr, n=n, state=state, adj=adj, off=off, diag=diag, keep=keep, w=w, dsum=dsum,
                                pattern=PATTERNS[case % len(PATTERNS)])))
    return tuple(out)


PAD_ADJ = (1, -7, 2, 1000000, 0, 3, -1)       # nonsense for the padding slots of adj (links that look real among it)
PAD_OFF = (-1.5, 1.0e300, 0.0, 7.25)
PAD_STATE = (-3, 99)


def padded(a, ld, filler):
    """a [n][k] array inside a [n][ld] one whose padding columns hold `filler` values (cycled)"""
    n, k = a.shape
    out = np.empty((n, ld), dtype=a.dtype)
    out[:, :k] = a
    pad = np.resize(np.asarray(filler, dtype=a.dtype), (n, ld - k))
    out[:, k:] = pad
    return out
