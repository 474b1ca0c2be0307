"""The plain restatement of the independent-stream SSA walk (tests/ssa_ref.py) must be trustworthy before a GPU is involved:
its generator against the folded form the device uses, walks that can be checked by hand, the statistics an SSA must have
(bounds derived from the Poisson / binomial laws, not measured), and the conditions the GPU cases
(tests/test_gpu_ssa_reference.py) rely on - duplicates, every end-of-path rule, more than 2^18 records - from the
restatement alone."""
import math

import numpy as np

from tests import ssa_ref as R


def _folded(rs):
    """rs a mod (2^31 - 1) without a division: 2^31 = 1 (mod m), so the high part of the product is folded onto its low 31
    bits twice, then one conditional subtraction (the device's form)"""
    p = rs * 48271
    y = (p & 0x7FFFFFFF) + (p >> 31)
    y = (y & 0x7FFFFFFF) + (y >> 31)
    return y - 0x7FFFFFFF if y >= 0x7FFFFFFF else y


def test_lehmer_step_equals_the_folded_form():
    rng = np.random.default_rng(1)
    m = 2 ** 31 - 1
    edge = [1, 2, m - 1, 44488, 44489, m // 48271, m // 48271 + 1, 2 ** 30, 2 ** 30 - 1, 2 ** 16]
    for rs in edge + rng.integers(1, m, 200000).tolist():
        want = R.lehmer_next(rs)
        assert want == _folded(rs) and 1 <= want <= m - 1, rs
    # the known orbit of the minimal standard generator with multiplier 48271: 1 -> ... -> 399268537 after 10 000 steps
    rs = 1
    for _ in range(10000):
        rs = R.lehmer_next(rs)
    assert rs == 399268537


def test_uniform_numbers_lie_in_the_unit_interval():
    m = 2 ** 31 - 1
    rng = np.random.default_rng(2)
    for rs in [1, 2, m - 1, 44488, 44489] + rng.integers(1, m, 20000).tolist():
        u, nxt = R.uniform(rs)
        assert 0.0 <= u < 1.0 and nxt == R.lehmer_next(R.lehmer_next(rs))
        assert u * 2.0 ** 54 == math.floor(u * 2.0 ** 54)           # a 54-bit number, rounded once to a double
    # the largest pair of draws stays below 1, the smallest is 0 (and is replaced by 2^-54 before the logarithm)
    assert float((((m - 1) << 30) | R.LCG_LOW) >> 7) * R.LCG_SCALE < 1.0
    assert R.plog(R.LCG_SCALE) < 0.0


def test_seed_mixing_lands_in_the_generators_range():
    m = 2 ** 31 - 1
    seen = set()
    for seedmix in (0, 1, m - 1, 2 ** 62 + 12345, -1):
        for j0 in (1, 2, 255, 20000, m):
            rs = R.seed_stream(seedmix & R.MASK64, j0)
            assert 1 <= rs <= m - 1
            seen.add(rs)
    assert len(seen) == 25
    # 64-bit wrap-around: a seedmix whose product with 2654435761 exceeds 2^64 gives what the wrapped product gives
    big = 2 ** 62 + 12345
    wrapped = (big * 2654435761) % 2 ** 64
    assert big * 2654435761 >= 2 ** 64
    rs = wrapped ^ (7 * 40503 + 12345)
    rs = ((rs ^ (rs >> 29)) & 0xFFFFFFFF) * 1181783497
    assert R.seed_stream(big, 7) == 1 + ((rs ^ (rs >> 32)) & (2 ** 63 - 1)) % (m - 1)
    assert R.seed_stream(-1 & R.MASK64, 3) == R.seed_stream(2 ** 64 - 1, 3)


def test_interpreter_and_tables():
    I, N, A, S, M, D = R.IMM, R.NEG, R.ADD, R.SUB, R.MUL, R.DIV
    # a_0 = p0 x (x - 1) / 2, a_1 = -(y - 3.5) / x, a_2 = nothing
    progs = [([103, 101, M, 101, I, S, M, I, D], [1.0, 2.0]), ([102, I, S, N, 101, D], [3.5]), ([], [])]
    p = R.Program(2, [0.3], progs)
    assert p.eval(0, (5, 1)) == ((0.3 * 5.0) * 4.0) / 2.0
    assert p.eval(1, (4, 1)) == 2.5 / 4.0 and p.eval(1, (0, 1)) == 0.0           # x / 0: the whole expression is 0
    assert p.eval(2, (4, 1)) == 0.0
    off, diag = p.columns([(5, 1), (4, 9)])
    assert off.shape == (2, 3) and diag[1] == (off[1, 0] + off[1, 1]) + off[1, 2]
    # a table is read inside its range and the code beyond it
    tab = np.zeros((3, 4))
    tab[0] = [7.0, 8.0, 9.0, 10.0]
    q = R.Program(2, [0.3], progs, tables=(np.array([0, -1, -1]), tab))
    assert [q.eval(0, (v, 0)) for v in (0, 3, 4)] == [7.0, 10.0, p.eval(0, (4, 0))]


def _birth(n0, c, t, max_count, seedmix=5, keep_paths=False):
    """one species, birth at the constant rate c, listed states 0 .. n0 - 1 with complete links"""
    nu = np.array([[1]], dtype=np.int32)
    state = np.arange(n0, dtype=np.int32).reshape(-1, 1)
    prog = R.Program(1, [c], [([102], [])])
    adj = R.links(nu, state, max_count)
    off, diag = prog.columns(state)
    return R.walk(t, seedmix, nu, state, adj, off, diag, max_count, prog, keep_paths=keep_paths)


def test_pure_birth_records_runs_of_consecutive_populations():
    n0, cap = 40, 55
    w = _birth(n0, 1.5, 8.0, cap, keep_paths=True)
    cut = 0
    for j0, (rec, jumps) in enumerate(zip(w.per_seed, w.jumps), start=1):
        # seed j0 is population j0 - 1: it climbs through the listed populations and records n0, n0 + 1, ... without a gap
        assert rec == [(n0 + i,) for i in range(len(rec))]
        assert len(rec) == max(0, int(jumps) - (n0 - j0))         # n0 - j0 jumps stay among the listed populations
        assert not rec or rec[-1][0] <= cap
        cut += bool(rec) and rec[-1][0] == cap
    assert w.ends["illegal"] > 0 and w.ends["horizon"] > 0 and w.ends["illegal"] + w.ends["horizon"] == n0
    assert cut >= w.ends["illegal"]                                  # a path cut by max_count stands at max_count
    assert w.ends["earlier"] == 0 and w.ends["negative"] == 0 and w.ends["absorbing"] == 0
    # first occurrence: the new states are the union of the runs, in ascending order
    top = max(len(r) for r in w.per_seed)
    assert w.state_new[:, 0].tolist() == list(range(n0, n0 + top)) and w.records == sum(len(r) for r in w.per_seed) > w.nnew
    assert np.array_equal(w.off_new, np.full((w.nnew, 1), 1.5)) and np.array_equal(w.diag_new, np.full(w.nnew, 1.5))


def test_pure_death_records_nothing():
    nu = np.array([[-1]], dtype=np.int32)
    state = np.arange(30, dtype=np.int32).reshape(-1, 1)
    prog = R.Program(1, [0.7], [([102], [])])                        # a constant propensity: population 0 still fires
    off, diag = prog.columns(state)
    for mode in ("complete", "zero"):
        w = R.walk(3.0, 9, nu, state, R.links(nu, state, 100, mode), off, diag, 100, prog)
        assert w.records == 0 and w.nnew == 0 and w.state_new.shape == (0, 1)
        assert w.ends["negative"] == 1 and w.ends["earlier"] == 29 and sum(w.ends.values()) == 30
        assert w.jumps.tolist() == [0] + [1] * 29


def test_it_is_an_ssa_poisson_jump_counts():
    """pure birth at rate c: the jump times of a path are a Poisson process, the jump that crosses the horizon is still taken,
    so jumps - 1 ~ Poisson(c t).  The mean over N independent paths has standard deviation sqrt(c t / N); 5 of them."""
    c, t, N = 2.0, 4.0, 4000
    w = _birth(N, c, t, 10 ** 9, seedmix=424242)
    assert w.ends["horizon"] == N
    mean = float(np.mean(w.jumps - 1))
    assert abs(mean - c * t) <= 5.0 * math.sqrt(c * t / N), mean
    # and the variance of a Poisson law is its mean: the sample variance has standard deviation ~ sqrt((2 m^2 + m) / N)
    var = float(np.var(w.jumps - 1, ddof=1))
    m = c * t
    assert abs(var - m) <= 5.0 * math.sqrt((2.0 * m * m + m) / N), var


def test_it_is_an_ssa_reaction_frequencies():
    """two reactions at constant rates a_1, a_2: the first jump of a path takes reaction k with probability a_k / a_0; the
    count over N independent paths is binomial, 5 standard deviations"""
    N = 6000
    nu = np.array([[1, 0], [0, 1]], dtype=np.int32)
    state = np.array([(0, s) for s in range(N)], dtype=np.int32)
    prog = R.Program(2, [0.3, 0.9], [([103], []), ([104], [])])
    off, diag = prog.columns(state)
    w = R.walk(1e-9, 31337, nu, state, R.links(nu, state, 10 ** 6), off, diag, 10 ** 6, prog)
    assert (w.jumps == 1).all()                                     # the horizon ends every path after its first jump
    p = 0.3 / (0.3 + 0.9)
    k0 = int((w.first_reaction == 0).sum())
    assert abs(k0 - N * p) <= 5.0 * math.sqrt(N * p * (1.0 - p)), k0
    assert int((w.first_reaction == 1).sum()) == N - k0


def test_variant_cases_exercise_the_walk():
    """every model built for one branch of the dispatch has paths that leave the FSP and come back: new states, jumps through
    unlisted states (the propensities the kernel under test evaluates itself), duplicates"""
    names = [c.name for c in R.variant_cases()]
    assert len(set(names)) == len(names) == 13
    for c in R.variant_cases():
        nr, ns = c.nu.shape
        assert c.ref.nnew > 0 and c.ref.virtual_jumps > 0 and c.ref.records > c.ref.nnew, c.name
        byte = bool((np.abs(c.nu) <= 127).all())
        small = ns <= 8 and nr <= 16 and byte and not c.options.get("ssa_general")
        assert small != c.name.startswith("k_ssa_walk_any"), c.name
        words = sum(len(code) for code, _ in c.program.programs)
        assert (words > 512) == (c.name == "k_ssa_walk<8,16,false,false>"), (c.name, words)
        if small and words <= 512:
            want = "2,4" if ns <= 2 and nr <= 4 else "6,12" if ns <= 6 and nr <= 12 else "8,16"
            assert c.name.startswith(f"k_ssa_walk<{want},true,{'false' if c.options.get('ssa_regs') == 0 else 'true'}>"), c.name
            # (the register path's condition: chains of at most three operands)
            assert all(len(code) <= 5 for code, _ in c.program.programs), c.name


def test_random_family_conditions():
    fam = R.random_family()
    dup, fired, empty = R.family_conditions(fam)
    assert 3 * dup >= len(fam), dup                                  # first-occurrence order matters in a third of the cases
    assert fired == set(R.END_RULES)
    assert empty == [R.NOTHING_FOUND]
    shapes = [c.nu.shape for c in fam]
    assert max(s[1] for s in shapes) > 8 and max(s[0] for s in shapes) > 16      # the general kernel's models are among them
    assert min(s[1] for s in shapes) == 1 and min(s[0] for s in shapes) <= 2
    assert {c.ref.ends["absorbing"] > 0 for c in fam} == {True, False}           # absorbing seeds
    assert any(c.ref.virtual_jumps == 0 and c.ref.nnew > 0 for c in fam)         # ends at the first jump
    assert any(c.ref.virtual_jumps > 4 * len(c.state) for c in fam)              # most rim paths leave the FSP


# ------------------------------------------------------------------------------------------------------------------
# two-species tables: the restatement of kfsp_set_propensity_tables2 and the conditions tests/test_gpu_prop_tables2.py
# relies on

def test_two_species_table_by_hand():
    """tab2[off + x[s2] n1 + x[s1]] on a 3 x 2 table written out by hand; a miss gives 0.0 and leaves flag and maxima"""
    I, A, D = R.IMM, R.ADD, R.DIV
    progs = [([101, 102, I, A, D], [1.0]), ([103], [])]            # x / (y + 1), and a constant
    nan = math.nan
    tab2 = [nan, nan, 10.0, 11.0, 12.0, 20.0, 21.0, 22.0, nan]    # rows y = 0, 1 of x = 0, 1, 2 (NOT the code's values: the table is read)
    p = R.Program(2, [0.5], progs, tables2=([0, -1], [1, -1], [3, 0], [2, 0], [2, 0], tab2))
    assert [p.eval(0, (x, y)) for y in (0, 1) for x in (0, 1, 2)] == [10.0, 11.0, 12.0, 20.0, 21.0, 22.0]
    assert not p.missed and p.reads2 == 6 and p.eval(1, (9, 9)) == 0.5 and p.reads2 == 6
    assert p.eval(0, (3, 1)) == 0.0 and p.missed and p.miss_max == [3, 0]
    assert p.eval(0, (7, 2)) == 0.0 and p.eval(0, (1, 5)) == 0.0 and p.miss_max == [7, 5] and p.reads2 == 9
    p.reset_misses()
    assert not p.missed and p.miss_max == [0, 0] and p.reads2 == 0
    # the variants read other entries
    # at (1, 1) - transposed: 2 + 1 * 2 + 1 = 5; n2 as the row length: 2 + 1 * 2 + 1 = 5; the offset of reaction k - 1 (none: 0): 0 + 3 + 1 = 4
    for variant, want in (("transposed", 20.0), ("row_n2", 20.0), ("offset_prev", 12.0)):
        q = R.Program(2, [0.5], progs, tables2=([0, -1], [1, -1], [3, 0], [2, 0], [2, 0], tab2), variant=variant)
        assert p.eval(0, (1, 1)) == 21.0 and q.eval(0, (1, 1)) == want, variant
    # make_tables2: descending offsets, gaps of NaN, the interpreter's values
    plain = R.Program(2, [0.5], progs)
    s1, s2, n1, n2, off, t = R.make_tables2(plain, {0: (1, 0, 4, 3)})
    assert (s1[0], s2[0], n1[0], n2[0]) == (1, 0, 4, 3) and s1[1] == -1 and off[0] == 5
    assert np.isnan(t[:5]).all() and np.isnan(t[5 + 12:]).all() and not np.isnan(t[5:17]).any()
    assert t[5 + 2 * 4 + 3] == 2.0 / (3.0 + 1.0)                   # x = x[s2] = 2, y = x[s1] = 3


def _changed(a, b):
    return int((~(np.asarray(a) == np.asarray(b))).sum())         # (a NaN counts as changed)


def test_columns_models_tell_the_variants_apart():
    """(a): on every model and every list of 255 states or more each wrong restatement changes at least 10 entries of
    columns(); the list of ONE state has 12 entries in all, of which a variant can reach at most the three tabulated ones and
    their sum - there every variant must change at least one.  The definition never reads a gap (Program asserts it), the
    tables have n1 != n2, s1 > s2 on two reactions, offsets descending in k with gaps."""
    counts = {}
    for ns in (3, 6, 9):
        prog, code, states = R.columns_model(ns)
        s1, s2, n1, n2, off, tab2 = prog.tables2
        tabd = [k for k in range(prog.nr) if s1[k] >= 0]
        assert len(tabd) == 4 and sum(s1[k] > s2[k] for k in tabd) >= 2 and all(n1[k] != n2[k] for k in tabd)
        assert (np.diff(off[tabd]) < 0).all() and np.isnan(tab2).sum() >= 12
        used = np.zeros(len(tab2), dtype=bool)
        for k in tabd:
            used[off[k]:off[k] + n1[k] * n2[k]] = True
        assert np.array_equal(used, ~np.isnan(tab2))                                # exactly the gaps hold NaN
        want = prog.columns(states)
        assert not prog.missed and prog.miss_max == [0] * ns and not np.isnan(want[0]).any()
        # the same bits from the code (the contract of a table), except where the planted one-species row would be read
        assert np.array_equal(code.columns(states)[0], want[0]) and np.array_equal(code.columns(states)[1], want[1])
        assert (states[:, 0] >= 12).any() and (states[:, 0] < 12).any() and (states[:, 1] == 3).any()
        for variant in R.Program.VARIANTS2:
            bad = R.columns_model(ns, variant=variant)[0]
            for n in R.COLUMN_SIZES:
                o, d = bad.columns(states[:n])
                c = _changed(o, want[0][:n]) + _changed(d, want[1][:n])
                assert c >= (10 if n >= 255 else 1), (ns, variant, n, c)
                counts[ns, variant, n] = c
    print({k: v for k, v in counts.items() if k[2] in (1, 255)})


def test_columns_models_with_small_tables_miss():
    """extent 4: every state is evaluated, so the maxima are the largest populations of the tabulated species beyond 4; the
    species of the chain's never-read table and the species without a table report 0"""
    for ns in (3, 6, 9):
        prog, _, states = R.columns_model(ns, extent=4)
        prog.reset_misses()
        prog.columns(states)
        want = [0] * ns
        for s in {0, 1, 2, ns - 1}:                                                # the species of tables 5, 6, 7
            want[s] = int(states[:, s].max())
        assert prog.missed and prog.miss_max == want and min(want[s] for s in (0, 1, 2, ns - 1)) >= 4, (ns, prog.miss_max)
        # the caller's rule serves every state in one round
        prog2 = R.with_tables2(R.columns_model(ns, extent=4)[0], R.grow_spec(R.spec_of(prog), prog.miss_max))
        prog2.columns(states)
        assert not prog2.missed


def test_walk_models_with_tables():
    """(b): tight tables (extent max_count + 1) serve every state the walk evaluates - no miss -, tables of extent 4 do not;
    at least 100 table reads at unlisted states; the transposed index changes state_new; the kernel each model reaches is
    read off its construction"""
    reads = {}
    for i, (tight, small) in enumerate(R.walk2_cases()):
        assert R.walk_kernel(tight) == R.walk_kernel(small) == R.WALK2_KERNELS[i] and tight.name.startswith(R.WALK2_KERNELS[i])
        spec = R.spec_of(tight.program)
        assert len(spec) == 2 and sorted(a > b for a, b, _, _ in spec.values()) == [False, True]
        assert all(e1 == e2 == tight.max_count + 1 for _, _, e1, e2 in spec.values())
        assert all(e1 == e2 == 4 for _, _, e1, e2 in R.spec_of(small.program).values())
        assert not any(tight.program._chain[k] for k in spec)
        ref = tight.ref
        assert ref.first_miss is None and ref.reads2 >= 100 and ref.nnew > 0 and ref.virtual_jumps > 0, (tight.name, ref.reads2)
        assert small.ref.first_miss is not None and max(small.ref.miss_max) >= 4, small.name
        bad = R.tabulated(R.variant_cases()[4 + i] if i < 5 else R.table_case(11), tight.max_count + 1, t_scale=tight.t_scale,
                          variant="transposed", max_count=tight.max_count)
        assert not np.array_equal(bad.ref.state_new, ref.state_new), tight.name
        reads[tight.name] = ref.reads2
    print(reads)


def test_stage_of_the_first_miss():
    """(d): the restatement shows every stage first somewhere.  The walk: the models of (b) with tables of extent 4.  The
    sweep: the models of (c) without a walk.  The columns of the walk's new states: the models of (c) under a horizon that
    ends every path at its first jump - the state it recorded last is evaluated by no path, only for its column."""
    stages = [small.ref.first_miss for _, small in R.walk2_cases()]
    assert "walk" in stages, stages
    for tight, small in R.sweep2_cases():
        assert R.expansion(tight, t_ssa=0.0).first_miss is None and R.expansion(tight).first_miss is None
        e = R.expansion(small, t_ssa=0.0)
        assert e.first_miss == "sweep" and max(e.miss_max) == 4, small.name
        e = R.expansion(small)
        assert e.first_miss == "columns" and e.walk.reads2 == 0 and e.walk.virtual_jumps == 0, small.name
        # every listed state lies inside the small tables
        assert int(small.state.max()) == 3


def test_callers_loop_stays_within_the_round_cap():
    """after a miss the caller grows the tables by grow_spec and repeats: within ns + ceil(log2(max_count + 1)) rounds (callers_loop
    asserts it) the answer is the tight tables' - for the walk alone, for the sweep alone and for the whole expansion"""
    def attempt_walk(case):
        def f(prog):
            w = R.walk(case.tstep, case.seedmix, case.nu, case.state, case.adj, case.off, case.diag, case.max_count, prog)
            return (None, w.miss_max) if w.first_miss else (w, None)
        return f

    def attempt_expand(case, t_ssa):
        def f(prog):
            e = R.expansion(case, prog, t_ssa)
            return (None, e.miss_max) if e.first_miss else (e, None)
        return f

    assert R.round_cap(2, 6) == 5 and R.round_cap(3, 7) == 6 and R.round_cap(2, 11) == 6
    rounds = {}
    for tight, small in R.walk2_cases():
        w, r, _ = R.callers_loop(small, attempt_walk(small))
        assert r >= 1 and np.array_equal(w.state_new, tight.ref.state_new) and np.array_equal(w.off_new, tight.ref.off_new)
        assert np.array_equal(w.diag_new, tight.ref.diag_new)
        rounds[small.name] = r
    for tight, small in R.sweep2_cases() + R.walk2_cases()[:1] + R.walk2_cases()[5:]:
        for t_ssa in (0.0, None):
            want = R.expansion(tight, t_ssa=t_ssa)
            e, r, _ = R.callers_loop(small, attempt_expand(small, t_ssa))
            assert want.first_miss is None and r >= 1, (small.name, t_ssa)
            assert np.array_equal(e.state, want.state) and np.array_equal(e.adj, want.adj)
            assert np.array_equal(e.off, want.off) and np.array_equal(e.diag, want.diag)
    print(rounds)


def test_share_case_misses_in_one_share_only():
    """300 seeds under three ranks: rank 0 walks no wavefront, rank 1 wavefront 0, rank 2 wavefront 1 - and only the seeds
    of wavefront 1 meet a population beyond the small table"""
    small, tight = R.share_case(True), R.share_case(False)
    args = (small.tstep, small.seedmix, small.nu, small.state, small.adj, small.off, small.diag, small.max_count, small.program)
    assert len(small.state) == 300 and len(R.SHARE_WAVE0) == 172 and len(R.SHARE_WAVE1) == 128
    assert R.walk(*args, seeds=R.SHARE_WAVE0).first_miss != "walk"
    w1 = R.walk(*args, seeds=R.SHARE_WAVE1)
    assert w1.first_miss == "walk" and w1.miss_max[0] >= 4 and w1.miss_max[1] == 0
    assert small.ref.first_miss == "walk" and small.ref.miss_max == w1.miss_max
    assert tight.ref.first_miss is None and tight.ref.nnew > 0 and R.expansion(tight).first_miss is None


def test_regrow_case_counts_more_records_than_the_first_list_holds():
    w = R.regrow_ref()
    assert 2 ** 18 < w.records < 2 ** 19 and w.ends["horizon"] == 4500
