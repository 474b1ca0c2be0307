"""TEST HELPER - the independent-stream SSA walk restated in plain Python.

STREAM_PATH / SSA_EXTENDER_STREAMS of krylovfspssa_amd/fortran/kfsp_statespace.f90 are the DEFINITION of the walk: an
integer generator, single IEEE operations, KFSP_PLOG as a fixed sequence, records ordered by (seed state, position on the
path), first occurrence kept.  Everything here is written from that text with Python integers (masked to 64 bits where the
Fortran wraps) and Python floats (IEEE doubles, one operation at a time, never contracted), so the result is the
definition's bit for bit and the device walk (csrc/kfsp_ssa.hip) is compared with it by np.array_equal, no tolerance.

Propensities of unlisted states come from Program: the postfix interpreter of include/kfsp.h restricted to the opcodes
that are exact everywhere (immediate, parameter, species, NEG, + - * /) plus one-species tables.  By the ABI's contract a
table holds a_k at every population it covers, so a reaction whose code is exact may be served from either; Program checks
that contract for product chains (which the library multiplies instead of reading their table) and otherwise reads the
table inside its range and interprets beyond it.  Two-species tables (kfsp_set_propensity_tables2) are restated with their
misses: a population beyond a table gives 0.0, a flag and a per-species maximum - what the library turns into status -16 -
and walk / expansion report the stage at which that first happened (second half of this file; tests/test_gpu_prop_tables2.py).

Also here, because the CPU tests (tests/test_ssa_ref.py) and the GPU tests (tests/test_gpu_ssa_reference.py) must see the
same cases: the model builders and the random family, and the conditions a case must meet to exercise what it claims."""
import functools
import math

import numpy as np

IMM, NEG, ADD, SUB, MUL, DIV = 1, 2, 3, 4, 5, 6

LCG_A = 48271
LCG_M = 2147483647                  # 2^31 - 1
LCG_LOW = 1073741823                # 2^30 - 1
LCG_SCALE = 2.0 ** -54
MASK64 = (1 << 64) - 1

END_RULES = ("absorbing", "negative", "illegal", "earlier", "horizon")
NOTHING_FOUND = "nothing found"


def plog(x):
    m, e = math.frexp(x)                       # x = m 2^e, m in [0.5, 1)
    if m < 0.70710678118654752440:
        m = m + m
        e = e - 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    p = 1.0 / 23.0
    for k in range(21, 2, -2):
        p = p * z
        p = p + 1.0 / float(k)
    p = p * z
    two_s = s + s
    r = two_s + two_s * p
    de = float(e)
    hi = de * 6.93147180369123816490e-01
    lo = de * 1.90821492927058770002e-10
    return hi + (lo + r)


def lehmer_next(rs):
    """RS = MOD(RS * LCG_A, LCG_M)"""
    return (rs * LCG_A) % LCG_M


def seed_stream(seedmix, j0):
    """(SEEDMIX, J0) -> RS: INTEGER(8) arithmetic that wraps, logical shifts"""
    rs = ((seedmix * 2654435761) & MASK64) ^ ((j0 * 40503 + 12345) & MASK64)
    rs = (((rs ^ (rs >> 29)) & 0xFFFFFFFF) * 1181783497) & MASK64
    return 1 + ((rs ^ (rs >> 32)) & 0x7FFFFFFFFFFFFFFF) % (LCG_M - 1)


def uniform(rs):
    """one 54-bit uniform number from two draws -> (u, rs')"""
    g1 = rs
    rs = (rs * LCG_A) % LCG_M
    g2 = rs
    rs = (rs * LCG_A) % LCG_M
    return float(((g1 << 30) | ((g2 - 1) & LCG_LOW)) >> 7) * LCG_SCALE, rs


class Program:
    """the propensity program of kfsp_set_propensity_program: programs[k] = (postfix code, immediates in order of use);
    tables = None or (tab_species [nr], tab [nr][tab_len]); tables2 = None or (s1, s2, n1, n2, off, tab2), the two-species
    tables of kfsp_set_propensity_tables2 (include/kfsp.h): reaction k with s1[k] >= 0 reads
    tab2[off[k] + x[s2[k]] * n1[k] + x[s1[k]]] while 0 <= x[s1] < n1 and 0 <= x[s2] < n2; beyond that the read is a MISS - it
    gives 0.0, raises `missed` and leaves the population in miss_max[species].  reads2 counts the reads (hits and misses).

    variant = None (the definition) or one of VARIANTS2: a restatement made wrong on purpose, to show on the CPU that the
    data can tell that defect (tests/test_ssa_ref.py)."""

    VARIANTS2 = ("transposed", "row_n2", "offset_prev", "precedence")

    def __init__(self, ns, params, programs, tables=None, tables2=None, variant=None):
        self.ns = int(ns)
        self.nr = len(programs)
        self.params = [float(v) for v in params]
        self.programs = [([int(c) for c in code], [float(v) for v in imm]) for code, imm in programs]
        for code, _ in self.programs:
            for c in code:
                assert c in (IMM, NEG, ADD, SUB, MUL, DIV) or 101 <= c <= 100 + self.ns + len(self.params), \
                    "the restatement covers the opcodes that are exact everywhere"
        self.tables = tables
        if tables is None:
            self.tab_species, self.tab, self.tab_len = [-1] * self.nr, None, 0
        else:
            self.tab_species = [int(v) for v in tables[0]]
            self.tab = np.ascontiguousarray(tables[1], dtype=np.float64)
            self.tab_len = self.tab.shape[1]
            for k in range(self.nr):
                s = self.tab_species[k]
                if s >= 0 and self._is_chain(k):               # the contract: the table IS the function
                    x = [0] * self.ns
                    for v in range(self.tab_len):
                        x[s] = v
                        assert self.tab[k, v] == self.interpret(k, x)
        self._tabl = None if self.tab is None else self.tab.tolist()
        assert variant is None or variant in self.VARIANTS2
        self.variant = variant
        self.tables2 = tables2
        self._chain = [self._is_chain(k) for k in range(self.nr)]
        if tables2 is None:
            self.t2 = [None] * self.nr
            self._tab2 = []
        else:
            s1, s2, n1, n2, off, tab2 = tables2
            assert len(s1) == len(s2) == len(n1) == len(n2) == len(off) == self.nr
            self._tab2 = np.asarray(tab2, dtype=np.float64).reshape(-1).tolist()
            self.t2 = [(int(s1[k]), int(s2[k]), int(n1[k]), int(n2[k]), int(off[k])) if s1[k] >= 0 else None for k in range(self.nr)]
            for t in self.t2:
                assert t is None or (0 <= t[0] < self.ns and 0 <= t[1] < self.ns and t[0] != t[1] and t[2] >= 1 and t[3] >= 1
                                     and 0 <= t[4] and t[4] + t[2] * t[3] <= len(self._tab2))
        self.reset_misses()

    def reset_misses(self):
        self.missed = False
        self.miss_max = [0] * self.ns
        self.reads2 = 0

    def _is_chain(self, k):
        """o_1 o_2 MUL o_3 MUL ... of at most four operands (kPropMonoOps): what the library multiplies out itself"""
        code = self.programs[k][0]
        if len(code) % 2 == 0 or len(code) > 7:
            return False
        for i, c in enumerate(code):
            operand = i == 0 or i % 2 == 1
            if operand != (c == IMM or c > 100):
                return False
            if not operand and c != MUL:
                return False
        return True

    def interpret(self, k, x):
        code, imm = self.programs[k]
        st = []
        ii = 0
        for c in code:
            if c == IMM:
                st.append(imm[ii])
                ii += 1
            elif c == NEG:
                st[-1] = -st[-1]
            elif c == ADD:
                b = st.pop()
                st[-1] = st[-1] + b
            elif c == SUB:
                b = st.pop()
                st[-1] = st[-1] - b
            elif c == MUL:
                b = st.pop()
                st[-1] = st[-1] * b
            elif c == DIV:
                b = st.pop()
                if b == 0.0:
                    return 0.0                                  # x / 0 makes the whole expression 0
                st[-1] = st[-1] / b
            else:
                v = c - 101
                st.append(float(x[v]) if v < self.ns else self.params[v - self.ns])
        return st[0] if st else 0.0

    def _read2(self, k, x):
        s1, s2, n1, n2, off = self.t2[k]
        self.reads2 += 1
        v1, v2 = x[s1], x[s2]
        if 0 <= v1 < n1 and 0 <= v2 < n2:
            if self.variant is None:
                a = self._tab2[off + v2 * n1 + v1]
                assert a == a, "a read of the gaps between the tables"
                return a
            if self.variant == "transposed":
                i = off + v1 * n2 + v2
            elif self.variant == "row_n2":
                i = off + v2 * n2 + v1
            elif self.variant == "offset_prev":
                prev = self.t2[(k - 1) % self.nr]
                i = (prev[4] if prev else 0) + v2 * n1 + v1
            else:
                i = off + v2 * n1 + v1
            return self._tab2[i] if i < len(self._tab2) else math.nan
        self.missed = True
        if v1 >= n1:
            self.miss_max[s1] = max(self.miss_max[s1], v1)
        if v2 >= n2:
            self.miss_max[s2] = max(self.miss_max[s2], v2)
        return 0.0

    def eval(self, k, x):
        """a_k(x) in the order of the header: a product chain is multiplied out; else the two-species table (a population
        beyond it is a miss: 0.0); else the one-species table while x < tab_len; else the interpreter"""
        if self._chain[k]:
            return self.interpret(k, x)
        s = self.tab_species[k]
        if self.variant == "precedence" and s >= 0 and 0 <= x[s] < self.tab_len:
            return self._tabl[k][x[s]]
        if self.t2[k] is not None:
            return self._read2(k, x)
        if s >= 0 and 0 <= x[s] < self.tab_len:
            return self._tabl[k][x[s]]
        return self.interpret(k, x)

    def columns(self, states):
        """OFFDIAG(k, i) = a_k(x_i), DIAG(i) = their sum in reaction order"""
        states = np.asarray(states).reshape(-1, self.ns)
        off = np.zeros((len(states), self.nr))
        diag = np.zeros(len(states))
        for i, x in enumerate(states.tolist()):
            d = 0.0
            for k in range(self.nr):
                a = self.eval(k, x)
                off[i, k] = a
                d = d + a
            diag[i] = d
        return off, diag

    def set_on(self, ctx):
        ctx.set_propensity_program(self.ns, np.array(self.params, dtype=np.float64), self.programs, tables=self.tables)
        if self.tables2 is not None:
            ctx.set_propensity_tables2(*self.tables2)


class Walk:
    """what one call gave: new states in order of first occurrence with their columns, and how the paths went"""

    def __init__(self):
        self.state_new = self.off_new = self.diag_new = None
        self.records = 0                    # records in all (duplicates included)
        self.nnew = 0                       # distinct new states
        self.virtual_jumps = 0              # jumps taken FROM an unlisted state
        self.ends = dict.fromkeys(END_RULES, 0)
        self.jumps = None                   # per seed: jumps completed (x moved)
        self.first_reaction = None          # per seed: reaction chosen at the first jump (-1: none)
        self.per_seed = None                # per seed: its records, in path order (only if asked for)
        self.reads2 = 0                     # two-species table reads at unlisted states during the walk (hits and misses)
        self.first_miss = None              # None, or the stage at which a population first lay beyond a two-species table:
        #                                     "walk" (a path), "columns" (the columns of the walk's new states)
        self.miss_max = None                # per species: the largest such population at that stage (0: none)


def walk(tstep, seedmix, nu, state, adj, off, diag, max_count, program, keep_paths=False, seeds=None):
    """SSA_EXTENDER_STREAMS on the lists as given: state [n0][ns], adj / off [n0][nr] (the reference's encoding: successor
    index from 1, 0 not linked, -1 negative population), diag [n0] = A0 of a listed state; seeds = None (a path from every
    listed state) or the 1-based seed states to walk from, ascending (one share of a partitioned walk)"""
    nu_l = np.asarray(nu).tolist()
    nr, ns = len(nu_l), len(nu_l[0])
    st_l = [tuple(r) for r in np.asarray(state).reshape(-1, ns).tolist()]
    adj_l = np.asarray(adj).tolist()
    off_l = np.asarray(off, dtype=np.float64).tolist()
    diag_l = np.asarray(diag, dtype=np.float64).tolist()
    index = {s: i + 1 for i, s in enumerate(st_l)}                  # LOOKUP: listed states, 1-based
    n0 = len(st_l)
    tstep = float(tstep)
    seedmix = int(seedmix) & MASK64
    res = Walk()
    res.jumps = np.zeros(n0, dtype=np.int64)
    res.first_reaction = np.full(n0, -1, dtype=np.int64)
    if keep_paths:
        res.per_seed = []
    ends = res.ends
    first = {}                                                      # new state -> order of first occurrence
    order = []
    program.reset_misses()
    peval = program.eval
    for j0 in (range(1, n0 + 1) if seeds is None else seeds):
        rs = seed_stream(seedmix, j0)
        j = j0
        virtual = False
        x = st_l[j - 1]
        tt = 0.0
        njump = 0
        mine = [] if keep_paths else None
        while True:
            r1, rs = uniform(rs)
            r2, rs = uniform(rs)
            if r1 <= 0.0:
                r1 = LCG_SCALE
            if virtual:
                a0 = 0.0
                pr = []
                for k in range(nr):
                    a = peval(k, x)
                    pr.append(a)
                    a0 = a0 + a
            else:
                a0 = diag_l[j - 1]
                pr = off_l[j - 1]
            if not (a0 > 0.0):
                ends["absorbing"] += 1
                break
            tt = min(tstep, tt + (-plog(r1) / a0))
            acc = pr[0]
            k = 0
            r2a = min(r2 * a0, a0)
            while acc < r2a and k < nr - 1:
                k += 1
                acc = acc + pr[k]
            if njump == 0:
                res.first_reaction[j0 - 1] = k
            y = tuple(a + b for a, b in zip(x, nu_l[k]))
            if min(y) < 0:
                ends["negative"] += 1
                break
            idx = 0
            if not virtual:
                idx = max(adj_l[j - 1][k], 0)
            if idx == 0:
                if max(y) > max_count:                              # LEGAL: every population <= max_count
                    ends["illegal"] += 1
                    break
                idx = index.get(y, 0)
            if virtual:
                res.virtual_jumps += 1
            x = y
            njump += 1
            if idx > 0:
                j = idx
                virtual = False
                if j < j0:
                    ends["earlier"] += 1
                    break
            else:
                virtual = True
                res.records += 1
                if mine is not None:
                    mine.append(y)
                if y not in first:
                    first[y] = len(order)
                    order.append(y)
            if not (tt < tstep):
                ends["horizon"] += 1
                break
        res.jumps[j0 - 1] = njump
        if keep_paths:
            res.per_seed.append(mine)
    res.nnew = len(order)
    res.state_new = np.array(order, dtype=np.int32).reshape(-1, ns)
    res.reads2 = program.reads2
    if program.missed:                                              # (the library stops here with -16: nothing else is made)
        res.first_miss, res.miss_max = "walk", list(program.miss_max)
        program.reset_misses()
    res.off_new, res.diag_new = program.columns(res.state_new)
    if program.missed and res.first_miss is None:
        res.first_miss, res.miss_max = "columns", list(program.miss_max)
    return res


# ------------------------------------------------------------------------------------------------------------------
# models

def links(nu, state, max_count, mode="complete", rng=None):
    """the ADJ columns of listed states: 'complete' (every successor that is listed is linked), 'zero' (nothing is linked:
    every jump goes through the look-up), 'partial' (each correct link made with probability 1/2); a negative target is
    -1 where the link is made"""
    nu = np.asarray(nu)
    nr, ns = nu.shape
    st = np.asarray(state).reshape(-1, ns)
    idx = {tuple(v): i + 1 for i, v in enumerate(st.tolist())}
    adj = np.zeros((len(st), nr), dtype=np.int32)
    if mode == "zero":
        return adj
    for j, v in enumerate(st):
        for k in range(nr):
            if mode == "partial" and rng.random() < 0.5:
                continue
            y = v + nu[k]
            adj[j, k] = -1 if y.min() < 0 else (0 if y.max() > max_count else idx.get(tuple(y.tolist()), 0))
    return adj


def mass_action_program(nu, pad_words=0, rate0=0.05):
    """a_k = c_k * prod of the species reaction k consumes, as the postfix chain  c x MUL y MUL ...; pad_words > 0 appends
    `p0 ADD` (p0 = a parameter that is 0.0) until every reaction has that many more code words - the value is unchanged,
    the program is no chain and needs that much more room"""
    nu = np.asarray(nu)
    nr, ns = nu.shape
    params = [rate0 + 0.01 * k for k in range(nr)] + [0.0]
    progs = []
    for k in range(nr):
        code = [100 + ns + 1 + k]
        for s in range(ns):
            if nu[k, s] < 0:
                code += [100 + s + 1, MUL]
        code += [100 + ns + nr + 1, ADD] * (pad_words // 2)
        progs.append((code, []))
    return Program(ns, params, progs)


class Case:
    """one call of the walk: lists, program, horizon, seed, options for the context"""

    def __init__(self, name, nu, state, program, t_scale, seedmix, max_count=10000, link_mode="complete", options=None, rng=None,
                 adj=None, plain=None):
        """adj: the links as given (else made by link_mode); plain: the program WITHOUT two-species tables that makes the
        columns of the listed states - the caller's arrays come from the host's evaluator, whatever the tables cover"""
        self.name = name
        self.nu = np.ascontiguousarray(nu, dtype=np.int32)
        self.state = np.ascontiguousarray(state, dtype=np.int32).reshape(-1, self.nu.shape[1])
        self.program = program
        self.plain = plain if plain is not None else program
        self.max_count = int(max_count)
        self.adj = links(self.nu, self.state, self.max_count, link_mode, rng) if adj is None else np.ascontiguousarray(adj, dtype=np.int32)
        self.off, self.diag = self.plain.columns(self.state)
        top = float(self.diag.max())
        self.t_scale = float(t_scale)
        self.tstep = float(t_scale) / (top if top > 0.0 else 1.0)
        self.seedmix = int(seedmix)
        self.options = dict(options or {})
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = walk(self.tstep, self.seedmix, self.nu, self.state, self.adj, self.off, self.diag, self.max_count, self.program)
        return self._ref

    def on_device(self, ctx, capacity_new=None, seedmix=None):
        self.program.set_on(ctx)
        for k, v in self.options.items():
            ctx.set_option(k, v)
        return ctx.ssa_streams(self.tstep, self.seedmix if seedmix is None else seedmix, self.nu, self.state, self.adj, self.off, self.diag,
                               max_count=self.max_count, capacity_new=capacity_new)


def _sparse_nu(rng, ns, nr, lo=-2, hi=2, width=3):
    """reaction vectors with at most `width` non-zero entries in [lo, hi] (a mass-action chain of at most that many species)"""
    nu = np.zeros((nr, ns), dtype=np.int32)
    for k in range(nr):
        for s in rng.choice(ns, size=min(ns, int(rng.integers(1, width + 1))), replace=False):
            nu[k, s] = int(rng.integers(lo, hi + 1))
    return nu


def _points(rng, ns, side, n):
    """n distinct random points of [0, side)^ns (fewer if the box is smaller), the origin among them, in random order"""
    n = min(n, side ** ns)
    seen = {(0,) * ns}
    while len(seen) < n:
        seen.add(tuple(int(v) for v in rng.integers(0, side, size=ns)))
    pts = np.array(sorted(seen), dtype=np.int32)
    return pts[rng.permutation(len(pts))]


def triangle(n0):
    """the first n0 points of N^2 ordered by x + y, then x: the last ones are the rim"""
    out = []
    d = 0
    while len(out) < n0:
        out += [(x, d - x) for x in range(d + 1)]
        d += 1
    return np.array(out[:n0], dtype=np.int32)


TWO_SPECIES_NU = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [-1, 1]], dtype=np.int32)


def _chain_model(rng, ns, nr):
    """a network whose every reaction is a chain of at most three operands (the register path's condition) and that both
    grows and shrinks: births, deaths and conversions"""
    nu = np.zeros((nr, ns), dtype=np.int32)
    for k in range(nr):
        kind = k % 3
        a, b = (int(v) for v in rng.choice(ns, size=2, replace=False)) if ns > 1 else (0, 0)
        if kind == 0:
            nu[k, a] = 1                                           # birth (a constant)
        elif kind == 1 or ns == 1:
            nu[k, a] = -1                                          # death (c x)
        else:
            nu[k, a], nu[k, b] = -1, 1                             # conversion (c x), or with a catalyst below
    return nu


@functools.lru_cache(maxsize=None)
def variant_cases():
    """one model per branch of the walk's dispatch; name = the kernel it must reach"""
    rng = np.random.default_rng(20261)
    cases = []

    def chain_case(name, ns, nr, options, n0=700, side=4, pad=0, seed=0):
        nu = _chain_model(rng, ns, nr)
        return Case(name, nu, _points(rng, ns, side, n0), mass_action_program(nu, pad_words=pad), 6.0, 1000 + seed,
                    max_count=side + 2, link_mode="partial", options=options, rng=rng)

    cases.append(chain_case("k_ssa_walk<2,4,true,true>", 2, 4, {}, n0=14, seed=1))
    cases.append(chain_case("k_ssa_walk<6,12,true,true>", 5, 10, {}, seed=2))
    cases.append(chain_case("k_ssa_walk<8,16,true,true> (8 species)", 8, 11, {}, seed=3))
    cases.append(chain_case("k_ssa_walk<8,16,true,true> (14 reactions)", 4, 14, {}, n0=200, seed=4))
    cases.append(chain_case("k_ssa_walk<2,4,true,false>", 2, 3, {"ssa_regs": 0}, n0=12, seed=5))
    cases.append(chain_case("k_ssa_walk<6,12,true,false>", 6, 12, {"ssa_regs": 0}, seed=6))
    cases.append(chain_case("k_ssa_walk<8,16,true,false>", 7, 16, {"ssa_regs": 0}, seed=7))
    # 3 species x 6 reactions x 100 words of padding: more than the 512 code words the light kernels keep in LDS
    cases.append(chain_case("k_ssa_walk<8,16,false,false>", 3, 6, {}, n0=50, pad=100, seed=8))
    cases.append(chain_case("k_ssa_walk_any (ssa_general=1)", 2, 4, {"ssa_general": 1}, n0=14, seed=9))
    cases.append(chain_case("k_ssa_walk_any (12 species)", 12, 9, {}, side=3, seed=10))
    cases.append(chain_case("k_ssa_walk_any (30 reactions)", 4, 30, {}, n0=200, seed=11))
    cases.append(chain_case("k_ssa_walk_any (64 reactions, 16 species)", 16, 64, {}, side=2, seed=12))
    # a coefficient outside a signed byte: bursts of 200 on a lattice of multiples of 200, single steps of the other species
    nu = np.array([[200, 0], [-200, 0], [0, 1], [0, -1], [-200, 1]], dtype=np.int32)
    st = np.array([(200 * a, b) for a in range(5) for b in range(6)], dtype=np.int32)[rng.permutation(30)]
    cases.append(Case("k_ssa_walk_any (coefficient 200)", nu, st, mass_action_program(nu, rate0=0.001), 4.0, 1013, max_count=2000,
                      link_mode="partial", rng=rng))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def random_family():
    """48 random networks: 1-10 species, 1-20 reactions with entries in [-2, 2] and mass-action propensities (a reaction that
    consumes nothing is a constant, one that consumes more than three species is interpreted), random points of a small box as
    listed states in random order, links complete / partial / all zero, horizons from 'ends at the first jump' (1e-6 of the
    fastest state's waiting time) to 'most rim paths leave the FSP' (60 of them), a population cap a little beyond the box.
    Cases 3k + 1 have only consuming reactions, so the origin - always listed - is an absorbing seed.  The last case is the
    designated 'nothing found' one: pure death inside a full box."""
    rng = np.random.default_rng(20262)
    cases = []
    horizons = (1e-6, 0.5, 2.0, 6.0, 20.0, 60.0)
    modes = ("complete", "partial", "zero")
    for c in range(47):
        while True:
            ns, nr = int(rng.integers(1, 11)), int(rng.integers(1, 21))
            nu = _sparse_nu(rng, ns, nr, width=4 if c % 5 == 0 else 3)
            if c % 3 == 1:
                for k in range(nr):                                # every reaction consumes something
                    if not (nu[k] < 0).any():
                        nu[k, int(rng.integers(0, ns))] = -1
            side = int(rng.integers(2, 6))
            state = _points(rng, ns, side, int(rng.integers(1, 400)))
            case = Case(f"random {c}", nu, state, mass_action_program(nu), horizons[c % 6], int(rng.integers(1, 2 ** 31 - 2)),
                        max_count=side + int(rng.integers(0, 4)), link_mode=modes[c % 3], rng=rng)
            if case.ref.nnew > 0:                                  # (a draw whose paths meet nothing new is drawn again)
                break
        cases.append(case)
    nu = np.array([[-1, 0], [0, -1]], dtype=np.int32)
    cases.append(Case(NOTHING_FOUND, nu, _points(rng, 2, 5, 25), mass_action_program(nu), 6.0, 77, max_count=8))
    return tuple(cases)


def family_conditions(cases):
    """what the random family must exercise, from the restatement alone: (cases with duplicate records, rules that ended a
    path somewhere, names of empty cases)"""
    dup = sum(1 for c in cases if c.ref.records > c.ref.nnew)
    fired = {r for c in cases for r in END_RULES if c.ref.ends[r] > 0}
    empty = [c.name for c in cases if c.ref.nnew == 0]
    return dup, fired, empty


def regrow_case(general):
    """every seed leaves the FSP at once: two species, birth of species 1 only at a constant rate, listed states (0, s);
    each path records every state it passes until the horizon - more than 2^18 records in all, so the record list the
    library sizes by a guess is too short and the call is repeated with the counted size"""
    nu = np.array([[1, 0]], dtype=np.int32)
    n0 = 4500
    state = np.array([(0, s) for s in range(n0)], dtype=np.int32)
    prog = Program(2, [2.0], [([103], [])])
    case = Case("regrow", nu, state, prog, 64.0, 20263, max_count=10000, link_mode="zero", options={"ssa_general": 1} if general else {})
    return case


@functools.lru_cache(maxsize=None)
def regrow_ref():
    return regrow_case(False).ref


@functools.lru_cache(maxsize=None)
def edge_case(n0, seedmix=4711, t_scale=2.0):
    """births, deaths and a conversion of two species on a random two thirds (n0 points) of a triangle x + y <= d, listed in a
    random order (a path falls back onto an earlier seed after a few jumps, or steps into a hole or over the rim); the horizon is t_scale mean
    waiting times"""
    big = triangle(n0 + n0 // 2 + 2)
    state = big[np.random.default_rng(n0).permutation(len(big))[:n0]]
    case = Case(f"triangle {n0}", TWO_SPECIES_NU, state, mass_action_program(TWO_SPECIES_NU), 1.0, seedmix, link_mode="complete")
    case.tstep = t_scale / float(np.mean(case.diag[case.diag > 0.0]))
    return case


@functools.lru_cache(maxsize=None)
def table_case(max_count, tab_len=12):
    """a reaction that is no product chain - the saturating decay c x / (K + x) - behind a one-species table of tab_len
    entries made with the interpreter; births push the population to max_count: the table's last entry when
    max_count = tab_len - 1, the code beyond it when larger"""
    nu = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], dtype=np.int32)
    params = [1.5, 0.8, 3.0, 0.4, 0.2]
    progs = [([103], []), ([104, 101, MUL, 105, 101, ADD, DIV], []), ([106], []), ([107, 102, MUL], [])]
    plain = Program(2, params, progs)
    tab = np.zeros((4, tab_len))
    tab[1] = [plain.interpret(1, (v, 0)) for v in range(tab_len)]
    prog = Program(2, params, progs, tables=(np.array([-1, 0, -1, -1], dtype=np.int32), tab))
    state = np.array([(a, b) for a in range(6) for b in range(4)], dtype=np.int32)
    return Case(f"table {max_count}", nu, state, prog, 40.0, 99, max_count=max_count, link_mode="complete")


# ------------------------------------------------------------------------------------------------------------------
# two-species tables (kfsp_set_propensity_tables2): how the tables are laid out, the functions they hold, the caller's
# rule after a miss, the expansion step with its three stages, and the models of tests/test_gpu_prop_tables2.py

def f_ratio(c, u, v):
    """c u / (v + 3) as exact-opcode postfix code (c, u, v: opcodes of a parameter and two species)"""
    return [c, u, MUL, v, IMM, ADD, DIV], [3.0]


def f_pairs(c, u, v):
    """c (u (v + 1) / 2)"""
    return [c, u, v, IMM, ADD, MUL, IMM, DIV, MUL], [1.0, 2.0]


def f_birth(c, u, v):
    """c (u + 1) / (v + 3): positive everywhere (for a reaction that consumes nothing)"""
    return [c, u, IMM, ADD, MUL, v, IMM, ADD, DIV], [1.0, 3.0]


def make_tables2(plain, spec):
    """spec {k: (s1, s2, n1, n2)} -> (s1, s2, n1, n2, off, tab2) with tab2[off[k] + v2 n1 + v1] = the value plain's
    interpreter gives reaction k at x[s1] = v1, x[s2] = v2 (the reaction reads no other species).  The tables lie in
    DESCENDING order of k, with gaps of unequal length before, between and after them; the gaps hold NaN."""
    nr, ns = plain.nr, plain.ns
    s1, s2 = np.full(nr, -1, dtype=np.int32), np.full(nr, -1, dtype=np.int32)
    n1, n2 = np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
    off = np.zeros(nr, dtype=np.int64)
    pos = 5
    for k in sorted(spec, reverse=True):
        a, b, e1, e2 = spec[k]
        assert all(not 101 <= c <= 100 + ns or c - 101 in (a, b) for c in plain.programs[k][0]), "a function of these two species"
        s1[k], s2[k], n1[k], n2[k], off[k] = a, b, e1, e2, pos
        pos += e1 * e2 + 3 + k
    tab2 = np.full(pos + 7, np.nan)
    for k, (a, b, e1, e2) in spec.items():
        x = [0] * ns
        for v2 in range(e2):
            x[b] = v2
            for v1 in range(e1):
                x[a] = v1
                tab2[off[k] + v2 * e1 + v1] = plain.interpret(k, x)
    return s1, s2, n1, n2, off, tab2


def with_tables2(plain, spec, variant=None):
    """plain's program behind the two-species tables of spec"""
    return Program(plain.ns, plain.params, plain.programs, tables=plain.tables, tables2=make_tables2(plain, spec) if spec else None,
                   variant=variant)


def spec_of(program):
    return {k: t[:4] for k, t in enumerate(program.t2) if t is not None}


def grow_spec(spec, missed, max_count=None):
    """the caller's rule after status -16: an extent a missed population lies beyond is doubled, made max_missed + 1 if that is
    more, and - where the model has a population limit - stops at max_count + 1, which serves every legal state"""
    def grown(extent, m):
        if m < extent:
            return extent
        e = max(m + 1, 2 * extent)
        return e if max_count is None else max(m + 1, min(e, max_count + 1))
    return {k: (a, b, grown(e1, int(missed[a])), grown(e2, int(missed[b]))) for k, (a, b, e1, e2) in spec.items()}


def round_cap(ns, max_count):
    """rounds the caller's loop may take: ns + ceil(log2(max_count + 1))"""
    return ns + int(max_count).bit_length()


def tabulated(case, extent, name=None, t_scale=None, variant=None, max_count=None):
    """`case` (mass-action chains, or table_case) with two of its reactions rewritten as functions of TWO species that are
    no product chain, and tabulated: the first reaction that consumes nothing becomes f_birth(c, other species, the species it
    makes), the last that consumes a species and has no one-species table becomes f_ratio(c, that species, the next one).
    The second is tabulated with s1 > s2, the first with s1 < s2.  Rate constant and any padding of the code stay.  extent: one
    number, or a function of the species.  The listed states, their links, the horizon's scale, the seed and the options are the
    case's; the columns of the listed states come from the code."""
    nr, ns = case.nu.shape
    assert ns >= 2
    base = case.plain
    ext = extent if callable(extent) else (lambda s: extent)
    k_b = next(k for k in range(nr) if not (case.nu[k] < 0).any())
    k_a = max(k for k in range(nr) if (case.nu[k] < 0).any() and base.tab_species[k] < 0)
    progs = list(base.programs)
    spec = {}
    for k, form in ((k_b, f_birth), (k_a, f_ratio)):
        code, imm = base.programs[k]
        assert not imm and code[0] > 100 + ns
        chain = 1 + 2 * int((case.nu[k] < 0).sum())
        a = int(np.argmax(case.nu[k] < 0)) if k == k_a else int(np.argmax(case.nu[k] > 0))
        b = (a + 1) % ns
        u, v = (a, b) if k == k_a else (b, a)
        new_code, new_imm = form(code[0], 101 + u, 101 + v)
        progs[k] = (new_code + code[chain:], new_imm)
        lo, hi = min(a, b), max(a, b)
        spec[k] = (hi, lo, ext(hi), ext(lo)) if k == k_a else (lo, hi, ext(lo), ext(hi))
    plain = Program(ns, base.params, progs, tables=base.tables)
    return Case(name or f"{case.name} + tables2", case.nu, case.state, with_tables2(plain, spec, variant),
                case.t_scale if t_scale is None else t_scale, case.seedmix, max_count=max_count or case.max_count,
                options=case.options, adj=case.adj, plain=plain)


def walk_kernel(case):
    """the kernel ssa_streams_core launches for a case whose program has two-species tables (no register path then), from the
    case's construction alone"""
    nr, ns = case.nu.shape
    small = ns <= 8 and nr <= 16 and bool((np.abs(case.nu) <= 127).all()) and not case.options.get("ssa_general")
    if not small:
        return "k_ssa_walk_any"
    if sum(len(code) for code, _ in case.program.programs) > 512:
        return "k_ssa_walk<8,16,false,false>"
    return "k_ssa_walk<%s,true,false>" % ("2,4" if ns <= 2 and nr <= 4 else "6,12" if ns <= 6 and nr <= 12 else "8,16")


WALK2_KERNELS = ("k_ssa_walk<2,4,true,false>", "k_ssa_walk<6,12,true,false>", "k_ssa_walk<8,16,true,false>",
                 "k_ssa_walk<8,16,false,false>", "k_ssa_walk_any", "k_ssa_walk<2,4,true,false>")


@functools.lru_cache(maxsize=None)
def walk2_cases():
    """(b): entries 4 to 8 of variant_cases() and table_case(11), each as (tight, small): tables of extent max_count + 1 in
    both species - they serve every legal state - and of extent 4"""
    out = []
    for i, c in enumerate(variant_cases()[4:9] + (table_case(11),)):
        # (the models of a few dozen seeds get a longer horizon and more room below the population limit: their paths then
        # make the hundred table reads the larger ones make anyway)
        t, mc = (600.0, 14) if len(c.state) < 100 else (None, c.max_count)
        out.append((tabulated(c, mc + 1, name=f"{WALK2_KERNELS[i]} tight ({c.name})", t_scale=t, max_count=mc),
                    tabulated(c, 4, name=f"{WALK2_KERNELS[i]} extent 4 ({c.name})", t_scale=t, max_count=mc)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sweep2_cases():
    """(c): every listed state lies inside tables of extent 4 (a box of side 4), its one-step neighbours at population 4 do
    not: without a walk (t_ssa = 0) the first miss is the sweep's.  (tight, small) as in walk2_cases."""
    rng = np.random.default_rng(20263)
    out = []
    box = np.array([(a, b) for a in range(4) for b in range(4)], dtype=np.int32)[rng.permutation(16)]
    nu3 = _chain_model(rng, 3, 6)
    for name, nu, state in (("sweep 2 species", TWO_SPECIES_NU, box), ("sweep 3 species", nu3, _points(rng, 3, 4, 40))):
        c = Case(name, nu, state, mass_action_program(nu), 1e-6, 31, max_count=6, link_mode="partial", rng=rng)
        out.append((tabulated(c, 7, name=name + " tight"), tabulated(c, 4, name=name + " extent 4")))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def share_case(small=True):
    """300 seeds, two wavefronts of the walk: blocks of 64 seeds are dealt round robin, so wavefront 1 owns seeds 65-128 and
    193-256 (from 1).  Its seeds stand at population 3 of species 0 - one birth from the end of a table of extent 4 - and all
    others at population 0, four births away: under three ranks one share is empty, one cannot miss, one does."""
    nu = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [-1, 1]], dtype=np.int32)
    state = np.array([(3 if (i // 64) % 2 == 1 else 0, i) for i in range(300)], dtype=np.int32)
    c = Case("share", nu, state, mass_action_program(nu, rate0=0.5), 1.5, 808, max_count=340, link_mode="complete")
    return tabulated(c, (lambda s: 4 if s == 0 else 341) if small else 341, name="share " + ("extent 4" if small else "tight"))


SHARE_WAVE1 = [j for j in range(1, 301) if ((j - 1) // 64) % 2 == 1]
SHARE_WAVE0 = [j for j in range(1, 301) if ((j - 1) // 64) % 2 == 0]


class Expansion:
    """kfsp_expand_resident restated: the lists afterwards, or the stage at which a population first lay beyond a table"""

    def __init__(self):
        self.state = self.adj = self.off = self.diag = None
        self.nssa = 0
        self.first_miss = None              # None, "walk", "columns" (of the walk's new states) or "sweep"
        self.miss_max = None
        self.walk = None


def expansion(case, program=None, t_ssa=None):
    """the restated walk (t_ssa = None: the case's horizon; 0: no walk), its states appended with their columns and no
    links, the plain one-step sweep (tests/expand_helpers.onestep_py), the columns of the sweep's states from the program -
    as tests/test_gpu_ssa_reference.py composes them.  Ends at the first stage that met a miss, as the library does."""
    from tests.expand_helpers import onestep_py
    prog = case.program if program is None else program
    nr = case.nu.shape[0]
    e = Expansion()
    st1, ad1, off1, diag1 = case.state, case.adj, case.off, case.diag
    if t_ssa is None or t_ssa > 0.0:
        w = walk(case.tstep if t_ssa is None else t_ssa, case.seedmix, case.nu, case.state, case.adj, case.off, case.diag,
                 case.max_count, prog)
        e.walk = w
        if w.first_miss:
            e.first_miss, e.miss_max = w.first_miss, w.miss_max
            return e
        e.nssa = w.nnew
        st1 = np.concatenate([st1, w.state_new])
        ad1 = np.concatenate([ad1, np.zeros((w.nnew, nr), dtype=np.int32)])
        off1 = np.concatenate([off1, w.off_new])
        diag1 = np.concatenate([diag1, w.diag_new])
    st2, ad2 = onestep_py(case.nu, st1, ad1, case.max_count)
    prog.reset_misses()
    o2, d2 = prog.columns(st2[len(st1):])
    if prog.missed:
        e.first_miss, e.miss_max = "sweep", list(prog.miss_max)
        return e
    e.state, e.adj, e.off, e.diag = st2, ad2, np.concatenate([off1, o2]), np.concatenate([diag1, d2])
    return e


def callers_loop(case, attempt):
    """the caller's side of status -16: attempt(program) -> (result, None) or (None, max_missed per species); after a miss the
    tables grow by grow_spec and the attempt is repeated.  Returns (result, rounds that missed, the last program)."""
    prog = case.program
    rounds = 0
    while True:
        res, missed = attempt(prog)
        if missed is None:
            return res, rounds, prog
        rounds += 1
        assert rounds <= round_cap(case.nu.shape[1], case.max_count), "the caller's loop does not end"
        spec = spec_of(prog)
        new = grow_spec(spec, missed, case.max_count)
        assert new != spec, "a miss that names no table"
        prog = with_tables2(case.plain, new)


# (a): the models of Program.columns / kfsp_propensities

COLUMN_SIZES = (1, 255, 256, 257, 1025)


@functools.lru_cache(maxsize=None)
def columns_model(ns, extent=None, honest=False, variant=None):
    """ns in (3, 6, 9) species, 11 reactions of every kind in one program:
      0 p                         chain of 1            1 p x0                  chain of 2, the constant first
      2 x1 p x_last               chain of 3, middle    3 x0 x1 x2 0.125        chain of 4, last
      4 p x0 x1 x2 x_last         5 operands: no chain for the library, interpreted
      5 f_ratio(p, x_last, x0)    table, s1 = last > s2 = 0, 20 x 23
      6 f_pairs(p, x1, x_last)    table, s1 = 1 < s2 = last, 21 x 20
      7 f_birth(p, x2, x1)        table 22 x 20 - AND a one-species table (species 2) of values that are NOT the function's:
                                  the two-species table goes first (honest = True leaves that row out)
      8 p x_{last-1} x_last       a chain WITH a two-species table of extent 2 x 3: the product goes first, the table is
                                  never read and never missed
      9 p x0 / (p' + x0)          a one-species table of 12 entries; populations run to 19
     10 x0 / (x1 - 3)             a zero divisor at x1 = 3
    extent = None: the extents above (every population is served); a number: tables 5, 6, 7 get that extent in both species.
    Returns (program, the same program as code with the one honest one-species table, states [1025][ns]); the first state has
    distinct populations 1 .. 10, so that each variant changes it."""
    L = ns - 1
    S = lambda i: 101 + i
    P = lambda j: 101 + ns + j
    params = [0.3, 1.7, 0.05, 2.5, 0.9, 4.0]
    progs = [([P(0)], []), ([P(1), S(0), MUL], []), ([S(1), P(2), MUL, S(L), MUL], []),
             ([S(0), S(1), MUL, S(2), MUL, IMM, MUL], [0.125]),
             ([P(3), S(0), MUL, S(1), MUL, S(2), MUL, S(L), MUL], []),
             f_ratio(P(4), S(L), S(0)), f_pairs(P(5), S(1), S(L)), f_birth(P(0), S(2), S(1)),
             ([P(1), S(L - 1), MUL, S(L), MUL], []),
             ([P(2), S(0), MUL, P(3), S(0), ADD, DIV], []),
             ([S(0), S(1), IMM, SUB, DIV], [3.0])]
    code = Program(ns, params, progs)
    ts = np.full(11, -1, dtype=np.int32)
    tab = np.zeros((11, 12))
    ts[9] = 0
    tab[9] = [code.interpret(9, [v] + [0] * L) for v in range(12)]
    code = Program(ns, params, progs, tables=(ts.copy(), tab.copy()))
    if not honest:
        ts[7] = 2
        tab[7] = [-1.0 - v for v in range(12)]
    plain = Program(ns, params, progs, tables=(ts, tab))
    e = (lambda big: big) if extent is None else (lambda big: extent)
    spec = {5: (L, 0, e(20), e(23)), 6: (1, L, e(21), e(20)), 7: (2, 1, e(22), e(20)), 8: (L, L - 1, 2, 3)}
    rng = np.random.default_rng(300 + ns)
    states = rng.integers(0, 20, size=(1025, ns)).astype(np.int32)
    states[0] = [(3 + 2 * i) % 11 + 1 for i in range(ns)]
    return with_tables2(plain, spec, variant), code, states
