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
SMALL = tuple(AC.BOXES) + tuple(DECODE) + ("dup_12x9",)
FAST = SMALL + tuple(LOOP)
NAMED_GENERIC = ("goutsias", "three_factor")
BLOCK_K = (1, 5, 16)
# (case, ranks, True: its blocks are shorter than its reach - the all-gather, not halo strips)
PARTITIONED = (("box_toggle_2x2", 2, False), ("box_toggle_2x2", 3, False), ("box_repressilator_3x2", 2, False),
               ("box_repressilator_3x2", 3, True), ("box_birth_death_6x2", 2, False), ("box_birth_death_6x2", 3, False),
               ("goutsias", 2, False), ("goutsias", 3, False))
# the instantiation <species, slots> of each single-factor case (the rule of kfsp_set_matrix_box)
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
    """<species, slots> the host instantiates for a single-factor model (kfsp_set_matrix_box)"""
    per = max(2, max(map(len, RR.box_slots(mdl))))
    if per > 2:
        per = 4
    return (2 if per == 2 and mdl.d <= 2 else 3 if per == 2 and mdl.d == 3 else 6), per


def pencil_format(mdl, pencil):
    """the kernel format option box_pencil = 1 / 2 selects on a small single-factor box (the eligibility rule of
    kfsp_set_matrix_box): pencils need the model's species to be the instantiation's, at least three of them, planes of
    an even number of rows and two planes; slabs also lines of an even number of rows and two lines"""
    if not pencil:
        return 4
    ns = mdl.d
    plane = int(np.prod(mdl.dims[:-1]))
    if not (ns >= 3 and ns == instance_of(mdl)[0] and plane % 2 == 0 and mdl.dims[-1] >= 2):
        return 4
    line = int(np.prod(mdl.dims[:-2]))
    return 8 if pencil == 2 and line % 2 == 0 and mdl.dims[-2] >= 2 else 7


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
def block(name, k):
    """-> (X, Y): k columns like the case's x, and box_exact of each; the narrower blocks of a test are its leading columns"""
    mdl = model(name)
    X = np.stack([vector(mdl.n, 900 + 20 * all_names().index(name) + j) for j in range(k)], axis=1)
    Y = np.stack([np.array(RR.box_exact(mdl, X[:, j])) for j in range(k)], axis=1)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y
