"""The restated row of the transposed generic matrix-free block product (tests/box_generic_t_ref.py; k_spmm_boxg_t under
options block_box = 2 and adjoint) without a GPU: it meets A^T X of the generator assembled from the model's CSR rows at
the bound of the existing adjoint row tests, 1e-13 (|A|^T |X|) per entry, on every multi-factor box of tests/box_cases.py;
and the named cases can tell a wrong kernel - the entries in descending order, the diagonal applied last - from the right
one on the bits."""
import numpy as np
import pytest

from tests import adjoint_cases as AC
from tests import box_cases as BC
from tests import box_generic_t_ref as GT
from tests.test_block_adjoint_host import bound, csr_of_model


def test_rows_by_hand():
    """a 3 x 2 box: a birth x -> x + 1 at the two-factor rate 2^x 4^(y - 1) and a death of y at 7 y.  The factor tables are
    (1, 2, 4) and (0.25, 1); sorted positions: the birth (delta = -1), then the death (delta = 3)"""
    from krylovfspssa_amd import synth
    mdl = synth.BoxModel("by_hand", (3, 2), [[1, 0], [0, -1]], lambda r, X: (2.0 ** X[0] * 4.0 ** (X[1] - 1.0), 7.0 * X[1])[r],
                         deps=[(0, 1), (1,)])
    X = [[1.0], [10.0], [100.0], [0.5], [0.25], [2.0]]
    rows = GT.box_generic_t_rows(mdl)
    # row 0 = (0, 0): the birth goes to row 1 at 1 * 0.25, the death leaves the box; row 4 = (1, 1): birth to row 5 at 2 * 1,
    # death to row 1 at 7; row 2 = (2, 0): the birth leaves the box but stays in DIAG
    assert rows[0] == ([(0.25, 1), (0.0, 0)], 0.25)
    assert rows[4] == ([(2.0, 5), (7.0, 1)], 9.0)
    assert rows[2] == ([(0.0, 2), (0.0, 2)], 1.0)
    Y = GT.box_generic_t_exact(mdl, X)
    assert Y[0] == [-0.25 + 0.25 * 10.0] and Y[4] == [-9.0 * 0.25 + 2.0 * 2.0 + 7.0 * 10.0] and Y[2] == [-100.0]
    A = csr_of_model(mdl)
    assert np.array_equal(np.array(Y), A.T @ np.array(X))            # dyadic values: exact either way
    assert GT.box_generic_t_exact(mdl, X, diag_last=True) == Y and GT.box_generic_t_exact(mdl, X, descending=True) == Y


@pytest.mark.parametrize("name", BC.generic_names())
def test_restatement_meets_the_assembled_transpose(name):
    c = GT.case(name)
    mdl, X, Y = c["mdl"], c["X"], c["Y"]
    assert max(len(d) for d in mdl.deps) >= 2                         # a box the single-factor kernels refuse
    A = csr_of_model(mdl)
    err, tol = np.abs(Y - A.T @ X), bound(A, X)
    print(name, mdl.n, "rows: max err / bound", float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol)


@pytest.mark.parametrize("name", BC.NAMED_GENERIC)
@pytest.mark.parametrize("flag", ["descending", "diag_last"])
def test_the_named_cases_can_tell_a_wrong_kernel(name, flag):
    c = GT.case(name)
    mdl, X, Y = c["mdl"], c["X"], c["Y"]
    Z = np.array(GT.box_generic_t_exact(mdl, X, **{flag: True}))
    bad = AC.mismatches(Z, Y)
    print(f"{name}: {flag}: {int(bad.any(axis=1).sum())} of {mdl.n} rows change, per column {bad.sum(axis=0).tolist()}")
    assert bad.any(), (name, flag)
    A = csr_of_model(mdl)
    assert np.all(np.abs(Z - A.T @ X) <= bound(A, X))                 # ... which the loose bound cannot


def test_the_forward_and_the_transposed_restatement_agree_on_the_generator():
    """<Z, A X> = <A^T Z, X> with both sides from the restated rows (row_ref.box_generic_exact forward)"""
    from tests import row_ref as RR
    c = GT.case("three_factor")
    mdl, X, Y = c["mdl"], c["X"], c["Y"]
    z = BC.vector(mdl.n, 77)
    Az = np.array(RR.box_generic_exact(mdl, z))
    A = csr_of_model(mdl)
    for j in range(X.shape[1]):
        lhs, rhs = float(X[:, j] @ Az), float(Y[:, j] @ z)
        assert abs(lhs - rhs) <= 1e-12 * float(np.abs(X[:, j]) @ (abs(A) @ np.abs(z)))
