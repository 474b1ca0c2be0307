"""TEST HELPER - the generators and blocks on which the transposed product Y = A^T X (option adjoint) is compared with
the exact rows of tests/row_ref.py, made once per process and shared by tests/test_row_ref.py (CPU: the restatement
itself, and that every case can tell a wrong order from the right one) and tests/test_gpu_block_adjoint_rows.py (the
device).  Every generator and block comes from a fixed seed.

The shapes are the smallest that still reach the edge a case is about (each stays below about 10^5 Fraction fmas):
  banded_40x33        1 320 rows: ten 128-row groups and a ragged eleventh of 40 rows; sources at r - delta < 0 and
                      >= n in the first and the last group
  banded_70x61        4 270 rows: 34 trips, more than one per wavefront under grid_blocks = 8, and a trip order
  masked_banded       toggle 1000 x 3: the +-1000 diagonals are empty on a third of the rows each
  ell_golden          an SSA-grown FSP of 231 states: links that leave the FSP (ADJ = 0 / -1), a last chunk of 39 rows
  ell_coded           toggle 60 x 50 as reference arrays (coded SELL on the device)
  ell_wide            the golden arrays in a leading dimension of bw + 3 whose three extra slots hold valid-looking
                      links and rates no product may read, and with ADJ = 0 in the middle of every fifth row (DIAG left
                      as it was: the row takes DIAG as given)
  box_*               one box per instantiation of the matrix-free kernel; one_species has 50 rows (less than a
                      wavefront), repressilator a dimension of 2 (every row a boundary row of that species), four_slot
                      reactions with nu = +-2"""
import functools

import numpy as np

from tests import block_generators
from tests import row_ref as RR
from tests.conftest import GOLDEN
from tests.test_block_adjoint_host import banded_form, csr_of_ell, csr_of_model, four_slot_box

K = 3                                           # kp = 4: one padding column
WIDE_PAD = 3


def _synth():
    from krylovfspssa_amd import synth
    return synth


def block(n, seed):
    """K columns with magnitudes in [1e-3, 1e3] (tests/row_ref.py: no product is subnormal) and mixed signs; column 1
    is a unit vector, so most rows of it run through fmas against 0.0 from a start of -(diag 0.0)"""
    rng = np.random.default_rng(seed)
    X = 10.0 ** rng.uniform(-3.0, 3.0, (n, K)) * np.where(rng.random((n, K)) < 0.5, -1.0, 1.0)
    X[:, 1] = 0.0
    X[n // 3, 1] = 1.0
    return X


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def mismatches(Y, ref):
    """entries of Y that are not the restatement's: a zero of the restatement by value (row_ref.fma does not carry the
    sign of a zero result), every other entry on the bits"""
    Y, ref = np.asarray(Y, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    zero = ref == 0.0
    return np.where(zero, Y != 0.0, bits(Y) != bits(ref))


def golden_wide():
    """(adj, off, diag, ld): the golden toggle arrays, ADJ = 0 in slot 1 of every fifth state, widened to ld = bw + 3"""
    g = block_generators.golden_toggle(GOLDEN)
    adj, off, diag = g["adj"].copy(), g["offdiag"].copy(), g["diag"].copy()
    adj[0::5, 1] = 0
    n, bw = adj.shape
    wide_adj = np.ones((n, bw + WIDE_PAD), dtype=np.int32)            # the extra slots: a link to state 1 at rate 777
    wide_off = np.full((n, bw + WIDE_PAD), 777.0)
    wide_adj[:, :bw], wide_off[:, :bw] = adj, off
    return wide_adj, wide_off, diag, bw


BANDED = {"banded_40x33": (40, 33), "banded_70x61": (70, 61), "masked_banded": (1000, 3)}
BOXES = {
    "box_toggle_2x2": lambda: _synth().toggle(21, 13),                            # 273 rows: two groups and 17 rows
    "box_repressilator_3x2": lambda: _synth().repressilator(dims=(13, 11, 2)),
    "box_birth_death_6x2": lambda: _synth().birth_death((3, 4, 2, 3, 2, 3)),
    "box_four_slot_6x4": four_slot_box,
    "box_one_species": lambda: _synth().birth_death((50,)),
}
ELL = ("ell_golden", "ell_coded", "ell_wide")
CASES = tuple(BANDED) + ELL + tuple(BOXES)


def model(name):
    return _synth().toggle(*BANDED[name]) if name in BANDED else BOXES[name]()


def ell_arrays(name):
    """(adj, off, diag) of an ELL case, bw slots wide"""
    if name == "ell_golden":
        g = block_generators.golden_toggle(GOLDEN)
        return g["adj"], g["offdiag"], g["diag"]
    if name == "ell_coded":
        return _synth().toggle(60, 50).ell()
    adj, off, diag, bw = golden_wide()
    return adj[:, :bw], off[:, :bw], diag


def exact(name, X, **wrong):
    """the restated rows of a case for the block X, as an (n, k) array; wrong: descending / diag_last"""
    if name in BANDED:
        return np.array(RR.banded_t_exact(*banded_form(model(name)), X, **wrong))
    if name in ELL:
        return np.array(RR.ell_t_exact(*ell_arrays(name), X, **wrong))
    return np.array(RR.box_t_exact(model(name), X, **wrong))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(n, A: the generator as a host CSR, X, Y: the restated rows of A^T X); computed once and left alone"""
    A = csr_of_ell(*ell_arrays(name)) if name in ELL else csr_of_model(model(name))
    n = A.shape[0]
    X = block(n, 100 + CASES.index(name))
    Y = exact(name, X)
    X.setflags(write=False)
    Y.setflags(write=False)
    return dict(n=n, A=A, X=X, Y=Y)
