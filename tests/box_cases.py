"""TEST HELPER - the boxes on which the FORWARD matrix-free product is compared with the restated rows of tests/row_ref.py
(box_exact: the single-factor fast path, formats 4 / 6 / 7 / 8 and k_spmm_box; box_generic_exact: format 3 and the
generator box_store writes out), made once per process and shared by tests/test_row_ref.py (CPU: the restatements
themselves, and that every case can tell a wrong kernel from the right one) and tests/test_gpu_box_rows.py (the device).
Every box but the loop_* ones has at most about 1 600 rows; x has both signs and magnitudes in [0.5, 1.5].

  the five boxes of adjoint_cases.BOXES   one per instantiation <2,2> <3,2> <6,2> <6,4>; one under 64 rows, one with a
                      dimension of 2, one with nu = +-2
  decode_*            a 49 in a species that is not the last: 49 * (1 / 49.0) < 1 in binary64, so the coordinate decode
                      (uint32)(q * inv_dim) comes out one short on the multiples of 49 and takes its r >= d correction
                      (and toggle 98 x 6: 98 = 2 * 49).  49x4x3 and 8x49x2 have planes of an even number of rows: the
                      pencil kernels take them too
  dup_12x9            per species two births of the SAME stoichiometry with different factors, and a death: three slots
                      per species (<6,4>), two of them tied on their offset
  goutsias            (5, 4, 3, 3, 2, 2): 720 rows, two reactions of two factors, one moving three species
  three_factor        (7, 6, 5): propensities of three factors, the only models on which the ORDER of the factor
                      multiplies shows (a product of two commutes)
  random*             the two-factor models (every third) of tests/test_gpu_box._random_box, 20 <= n <= 1500
  loop_*              the ONLY boxes above 1 600 rows, one per instantiation, 4 352 - 5 917 rows = 34 - 47 trips: under
                      grid_blocks = 8 a workgroup gets five or six consecutive trips for its four wavefronts, so some
                      wavefronts go round the trip loop - whose row code is a second inlined copy of the first trip's"""
import functools

import numpy as np

from tests import adjoint_cases as AC
from tests import row_ref as RR

bits = AC.bits


def _synth():
    from krylovfspssa_amd import synth
    return synth


def dup_box():
    st = [[1, 1, -1, 0, 0, 0], [0, 0, 0, 1, 1, -1]]

    def prop(r, X):
        x, y = X
        return (5.0 / (1.0 + 0.1 * x), 2.0 + 0.3 * x * x / (2.0 + x), 0.7 * x, 3.0 / (1.0 + 0.07 * y * y), 1.1 + 0.2 * y, 0.9 * y)[r]
    return _synth().BoxModel("dup", (12, 9), st, prop, deps=[(0,), (0,), (0,), (1,), (1,), (1,)])


def three_factor_box():
    """x -> x + 1 at a rate of three factors, a conversion x -> y of three factors listed in another species order, a
    two-factor loss of z and single-factor losses"""
    st = [[1, -1, 0, -1, 0], [0, 1, 0, 0, -1], [0, 0, -1, 0, 0]]

    def f(x):
        return 1.0 / (1.0 + 0.1 * x)

    def g(x):
        return (2.0 + x * x) / 3.0

    def prop(r, X):
        x, y, z = X
        return (4.3 * f(x) * g(y) * f(z), 0.37 * x * f(y) * g(z), 0.21 * z * g(x), 0.8 * x, 0.6 * y)[r]
    return _synth().BoxModel("three_factor", (7, 6, 5), st, prop, deps=[(0, 1, 2), (1, 2, 0), (2, 0), (0,), (1,)])


def _four_slot(dims):
    """adjoint_cases' four-slot box (nu = +-2 on species 0) at other dimensions"""
    m = AC.four_slot_box()
    return _synth().BoxModel("four_slot", dims, m.stoich, m.prop, deps=m.deps)


def six_species_four_slot(dims):
    """six species, the first with the four reactions of the four-slot box (nu = +-1, +-2), the others born and dying:
    the <6,4> instantiation on a box whose species are the instantiation's, which the pencil kernels therefore take"""
    d = len(dims)
    assert d == 6
    st = np.zeros((d, 4 + 2 * (d - 1)), dtype=np.int64)
    st[0, :4] = (1, -1, 2, -2)
    for i in range(1, d):
        st[i, 2 + 2 * i], st[i, 3 + 2 * i] = 1, -1

    def prop(r, X):
        if r < 4:
            x = X[0]
            return (np.full_like(x, 5.0), 0.7 * x, 1.5 + 0.01 * x, 0.02 * x * (x - 1.0))[r]
        i = (r - 2) // 2
        return np.full_like(X[i], 2.0 + 0.5 * i) if r % 2 == 0 else (0.4 + 0.1 * i) * X[i]
    return _synth().BoxModel("six_four_slot", dims, st, prop, deps=[(0,)] * 4 + [((r - 2) // 2,) for r in range(4, st.shape[1])])


def conversion_box(dims):
    """six species born and dying, and a conversion of the first into the last: an entry of species 0 (its propensity
    depends on species 0 alone) that moves the slowest species - the pencil kernels then mask that entry plane by plane
    with the slowest species' valid bit (their SIMPLE = false instantiation); three slots in species 0: <6,4>"""
    d = len(dims)
    assert d == 6
    st = np.zeros((d, 2 * d + 1), dtype=np.int64)
    for i in range(d):
        st[i, 2 * i], st[i, 2 * i + 1] = 1, -1
    st[0, 2 * d], st[d - 1, 2 * d] = -1, 1

    def prop(r, X):
        if r == 2 * d:
            return 0.3 * X[0]
        i = r // 2
        return np.full_like(X[i], 3.0 + 0.25 * i) if r % 2 == 0 else (0.5 + 0.1 * i) * X[i]
    return _synth().BoxModel("conversion", dims, st, prop, deps=[(r // 2,) for r in range(2 * d)] + [(0,)])


@functools.lru_cache(maxsize=None)
def _random_two_factor():
    """name -> model: _random_box's own sequence from a fixed seed, the two-factor models (k % 3 == 2) of a usable size"""
    from tests.test_gpu_box import _random_box
    rng = np.random.default_rng(4242)
    out = {}
    for k in range(60):
        mdl = _random_box(rng, k)
        if k % 3 == 2 and max(len(d) for d in mdl.deps) == 2 and 20 <= mdl.n <= 1500:
            out[f"random{k}"] = mdl
    return out


DECODE = {
    "decode_49x4x3": lambda: _synth().birth_death((49, 4, 3)),
    "decode_8x49x2": lambda: _synth().repressilator(dims=(8, 49, 2)),
    "decode_2x49x2x2x2x2": lambda: _synth().birth_death((2, 49, 2, 2, 2, 2)),
    "decode_toggle_98x6": lambda: _synth().toggle(98, 6),
}
LOOP = {
    "loop_toggle_97x61": lambda: _synth().toggle(97, 61),
    "loop_repressilator_17x16x16": lambda: _synth().repressilator(dims=(17, 16, 16)),
    "loop_birth_death_4x4x4x4x4x5": lambda: _synth().birth_death((4, 4, 4, 4, 4, 5)),
    "loop_four_slot_75x60": lambda: _four_slot((75, 60)),
}
# Boxes for the size-gated variants of the pencil kernels (tests/test_gpu_box_slab_waves.py), instance <6,2> unless named
# otherwise, all with lines of an even number of rows.  slab_*: format 8 with fewer wavefronts than the four a 256-thread
# workgroup has (lines = dims[-2] = 2 or 3), lines of 3000 rows (a last trip with dead lanes) and the 22-line box of
# tests/test_gpu_box.py.  tile_*: planes on which box_tile_order has a tiled base-trip order to give (a cut stride of at
# least 2048 rows); two of them are slab boxes as well.
SLAB = {
    "slab_8x8x8x8x2x2": lambda: _synth().birth_death((8, 8, 8, 8, 2, 2)),
    "slab_8x8x8x4x3x2": lambda: _synth().birth_death((8, 8, 8, 4, 3, 2)),
    "slab_10x10x6x5x2x2": lambda: _synth().birth_death((10, 10, 6, 5, 2, 2)),
    "slab_6x4x3x2x22x3": lambda: _synth().birth_death((6, 4, 3, 2, 22, 3)),
}
TILE = {
    "tile_6x8x8x8x3x2": lambda: _synth().birth_death((6, 8, 8, 8, 3, 2)),
    "tile_four_slot_8x8x8x4x2x2": lambda: six_species_four_slot((8, 8, 8, 4, 2, 2)),
    "tile_small_8x8x8x4x2x2": lambda: _synth().birth_death((8, 8, 8, 4, 2, 2)),
    "tile_conversion_8x8x8x4x2x3": lambda: conversion_box((8, 8, 8, 4, 2, 3)),
}
TILED = ("slab_8x8x8x8x2x2", "slab_10x10x6x5x2x2", "tile_6x8x8x8x3x2")          # the three boxes of the order tests
SLAB_WAVES = (1, 2, 3, 5, 12)
SMALL = tuple(AC.BOXES) + tuple(DECODE) + ("dup_12x9",)
FAST = SMALL + tuple(LOOP)
NAMED_GENERIC = ("goutsias", "three_factor")
BLOCK_K = (1, 5, 16)
# (case, ranks, True: its blocks are shorter than its reach - the all-gather, not halo strips)
PARTITIONED = (("box_toggle_2x2", 2, False), ("box_toggle_2x2", 3, False), ("box_repressilator_3x2", 2, False),
               ("box_repressilator_3x2", 3, True), ("box_birth_death_6x2", 2, False), ("box_birth_death_6x2", 3, False),
               ("goutsias", 2, False), ("goutsias", 3, False))
# the instantiation <species, slots> of each single-factor case (the rule of box_plan, csrc/kfsp_box_plan.h)
INSTANCE = {"box_toggle_2x2": (2, 2), "box_repressilator_3x2": (3, 2), "box_birth_death_6x2": (6, 2), "box_four_slot_6x4": (6, 4),
            "box_one_species": (2, 2), "decode_49x4x3": (3, 2), "decode_8x49x2": (3, 2), "decode_2x49x2x2x2x2": (6, 2),
            "decode_toggle_98x6": (2, 2), "dup_12x9": (6, 4), "loop_toggle_97x61": (2, 2), "loop_repressilator_17x16x16": (3, 2),
            "loop_birth_death_4x4x4x4x4x5": (6, 2), "loop_four_slot_75x60": (6, 4)}


def generic_names():
    return NAMED_GENERIC + tuple(_random_two_factor())


@functools.lru_cache(maxsize=None)
def model(name):
    if name in AC.BOXES:
        return AC.BOXES[name]()
    if name in DECODE:
        return DECODE[name]()
    if name in LOOP:
        return LOOP[name]()
    if name == "dup_12x9":
        return dup_box()
    if name in SLAB:
        return SLAB[name]()
    if name in TILE:
        return TILE[name]()
    if name == "goutsias":
        return _synth().goutsias_box((5, 4, 3, 3, 2, 2))
    if name == "three_factor":
        return three_factor_box()
    return _random_two_factor()[name]


def all_names():
    return FAST + generic_names()


def vector(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)


def instance_of(mdl):
    """<species, slots> the host instantiates for a single-factor model: the `per` / `ns_inst` rule of box_plan
    (csrc/kfsp_box_plan.h) restated; tests/test_box_plan_host.py holds the two against each other"""
    per = max(2, max(map(len, RR.box_slots(mdl))))
    if per > 2:
        per = 4
    return (2 if per == 2 and mdl.d <= 2 else 3 if per == 2 and mdl.d == 3 else 6), per


def pencil_format(mdl, pencil):
    """the kernel format option box_pencil = 1 / 2 selects on a small single-factor box (the eligibility rule of
    box_plan, csrc/kfsp_box_plan.h, restated; tests/test_box_plan_host.py compares them): pencils need the model's
    species to be the instantiation's, at least three of them, planes of an even number of rows and two planes; slabs
    also lines of an even number of rows and two lines"""
    if not pencil:
        return 4
    ns = mdl.d
    plane = int(np.prod(mdl.dims[:-1]))
    if not (ns >= 3 and ns == instance_of(mdl)[0] and plane % 2 == 0 and mdl.dims[-1] >= 2):
        return 4
    line = int(np.prod(mdl.dims[:-2]))
    return 8 if pencil == 2 and line % 2 == 0 and mdl.dims[-2] >= 2 else 7


def slab_geometry(dims, slab_waves=12):
    """(lines, groups, waves, lo_trips) of format 8, the rule of box_plan (csrc/kfsp_box_plan.h) restated: the lines of the
    second-slowest species are shared out over the fewest workgroups of at most min(12, box_slab_waves) wavefronts, and
    evenly over those; a workgroup takes 128 rows of each of its lines"""
    line, lines = int(np.prod(dims[:-2])), int(dims[-2])
    wmax = max(1, min(12, slab_waves))
    groups = -(-lines // wmax)
    waves = -(-lines // groups)
    return lines, groups, waves, -(-line // 128)


def vec_grid(n, vec_grid_blocks=0):
    """workgroups - partial sums - of the streaming kernels over n rows (kfsp_host.h, vec_grid, restated): the rows padded
    to 64-row chunks, two to a pair, 1024 pairs per workgroup, at most 1024 workgroups (or the option) and the 2048 slots"""
    pairs = -(-n // 64) * 32
    return max(1, min(-(-pairs // 1024), vec_grid_blocks if vec_grid_blocks > 0 else 1024, 2048))


def tile_order(dims):
    """box_tile_order(force) of kfsp_box_plan.h - the order box_plan hands to the pencil kernel - restated for the
    species `dims` of a plane (fastest first): () where it gives no order, else the base trips sorted by (1024-row block of the row below the cut, line above the cut, row below the
    cut), the cut being the slowest stride of a species but the first that is at most 16384 rows"""
    n = int(np.prod(dims))
    trips = -(-n // 128)
    strides = [int(np.prod(dims[:s])) for s in range(len(dims))]
    cuts = [st for s, st in enumerate(strides) if s > 0 and st <= 16384]
    if len(dims) < 3 or trips < 2 or not cuts or cuts[-1] < 2048:
        return ()
    scut = cuts[-1]
    return tuple(sorted(range(trips), key=lambda c: ((128 * c % scut) // 1024, 128 * c // scut, 128 * c % scut)))


def decode_corrections(mdl, row0=0, nloc=None):
    """(rows whose coordinate decode takes the r >= d step, rows that take the r < 0 step) with the kernel's own formula:
    t = (uint32)((double) q * (1.0 / d)), r = q - t d, per species but the last"""
    g = np.arange(row0, row0 + (mdl.n - row0 if nloc is None else nloc), dtype=np.int64)
    q = g.copy()
    hi, lo = np.zeros(len(g), dtype=bool), np.zeros(len(g), dtype=bool)
    for d in mdl.dims[:-1]:
        t = (q.astype(np.float64) * (1.0 / float(d))).astype(np.int64)
        r = q - t * d
        hi |= r >= d
        lo |= r < 0
        t = t + (r >= d) - (r < 0)
        assert np.array_equal(t, q // d)                      # one step is enough
        q = t
    return int(hi.sum()), int(lo.sum())


def mismatches(y, ref):
    """rows of y that are not the restatement's: a zero of the restatement by value (row_ref.fma does not carry the sign
    of a zero result), every other row on the bits"""
    return np.flatnonzero(AC.mismatches(y, ref))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(mdl, n, x, y: box_exact (single-factor cases only), yg: box_generic_exact); computed once, left alone"""
    mdl = model(name)
    x = vector(mdl.n, 500 + all_names().index(name))
    out = dict(mdl=mdl, n=mdl.n, x=x, yg=np.array(RR.box_generic_exact(mdl, x)))
    if name in FAST:
        out["y"] = np.array(RR.box_exact(mdl, x))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gated_case(name):
    """a SLAB / TILE box -> dict(mdl, n, x, y: box_exact); computed once (about a second per 10 000 rows), left alone.
    (These boxes stay out of FAST: the CPU tests over FAST restate every box row by row in both forms.)"""
    mdl = model(name)
    x = vector(mdl.n, 700 + (tuple(SLAB) + tuple(TILE)).index(name))
    out = dict(mdl=mdl, n=mdl.n, x=x, y=np.array(RR.box_exact(mdl, x)))
    out["x"].setflags(write=False)
    out["y"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def block(name, k):
    """-> (X, Y): k columns like the case's x, and box_exact of each; the narrower blocks of a test are its leading columns"""
    mdl = model(name)
    X = np.stack([vector(mdl.n, 900 + 20 * all_names().index(name) + j) for j in range(k)], axis=1)
    Y = np.stack([np.array(RR.box_exact(mdl, X[:, j])) for j in range(k)], axis=1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y
