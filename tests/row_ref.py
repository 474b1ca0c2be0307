"""What one row of the generator product is, restated plainly ("The row, restated").

    y[r] = fma(v_m, x[c_m], ... fma(v_2, x[c_2], fma(v_1, x[c_1], -(diag[r] * x[r]))) ...)

One rounded multiply for the diagonal term, then one correctly rounded fused multiply-add per entry, the entries
ascending by the CALLER's index of their source state, then by value, then by their position in the caller's arrays
(the order in which FMATVEC's scatter loop reaches them, KrylovSolver.f90:598-604; the header comment of
k_sell_sort_rows promises it).  No device, no oracle library and no numpy in the arithmetic: plain Python lists,
Python floats (IEEE binary64) and fractions.Fraction for the one rounding of the fused multiply-add.  Arrays that
come in as numpy arrays are turned into lists first.

Inputs are expected in roughly [1e-3, 1e3] in magnitude: no product is subnormal there, so the device's handling of
subnormal numbers cannot enter a comparison."""
from fractions import Fraction


def fma(a, b, c):
    """a * b + c with one rounding (Python 3.10 has no math.fma): the exact rational, rounded to nearest even by float()"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _lists(a):
    return a.tolist() if hasattr(a, "tolist") else a


def gather_rows(adj, offdiag, diag, row0=0, nloc=None):
    """The reference's column-oriented arrays (adj[i][j] = 1-based target of slot j of state i, <= 0: no link;
    offdiag[i][j] its rate) -> for every local row r (global row row0 + r) the list of (source, value) pairs, ascending
    by source, then value, then slot.  diag is only asked for its length (the number of states)."""
    adj, offdiag = _lists(adj), _lists(offdiag)
    n = len(diag)
    if nloc is None:
        nloc = n - row0
    found = [[] for _ in range(nloc)]
    for i in range(n):
        ai, oi = adj[i], offdiag[i]
        for j in range(len(ai)):
            k = ai[j]
            if k < 1:
                continue
            assert k <= n, "link beyond the state space"
            r = k - 1 - row0
            if 0 <= r < nloc:
                found[r].append((i, oi[j], j))
    return [[(i, v) for i, v, _ in sorted(row)] for row in found]


def rows_from_csr(n, rowptr, col, val, row0=0):
    """The same form from CSR rows of the local block (rowptr of nloc + 1 entries, global 0-based columns, already
    ascending by column as the CSR and banded uploads require): (rows, diag).  Entries on the diagonal are taken out
    and summed; diag is MINUS that sum (kept positive, like DIAG of the reference)."""
    rowptr, col, val = _lists(rowptr), _lists(col), _lists(val)
    nloc = len(rowptr) - 1
    rows, diag = [], []
    for r in range(nloc):
        row, d = [], 0.0
        for p in range(rowptr[r], rowptr[r + 1]):
            assert 0 <= col[p] < n
            if col[p] == row0 + r:
                d += val[p]
            else:
                assert not row or row[-1][0] <= col[p], "CSR row not ascending by column"
                row.append((col[p], val[p]))
        rows.append(row)
        diag.append(-d)
    return rows, diag


def spmv_exact(rows, diag, x, row0=0):
    """y[r] for the local rows: diag[r] is the diagonal of global row row0 + r (positive), x the whole vector"""
    diag, x = _lists(diag), _lists(x)
    y = []
    for r, row in enumerate(rows):
        s = -(diag[r] * x[row0 + r])
        for c, v in row:
            s = fma(v, x[c], s)
        y.append(s)
    return y


def reverse_from(rows, cap):
    """every row with its entries from position cap on in reverse order: what a sort that stops at cap entries may
    leave behind (used to show that a test case can tell)"""
    return [row[:cap] + row[cap:][::-1] for row in rows]
