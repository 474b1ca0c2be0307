"""What one row of the generator product is, restated plainly ("The row, restated").

    y[r] = fma(v_m, x[c_m], ... fma(v_2, x[c_2], fma(v_1, x[c_1], -(diag[r] * x[r]))) ...)

One rounded multiply for the diagonal term, then one correctly rounded fused multiply-add per entry, the entries
ascending by the CALLER's index of their source state, then by value, then by their position in the caller's arrays
(the order in which FMATVEC's scatter loop reaches them, KrylovSolver.f90:598-604; the header comment of
k_sell_sort_rows promises it).  No device, no oracle library and no numpy in the arithmetic: plain Python lists,
Python floats (IEEE binary64) and fractions.Fraction for the one rounding of the fused multiply-add.  Arrays that
come in as numpy arrays are turned into lists first.

Inputs are expected in roughly [1e-3, 1e3] in magnitude: no product is subnormal there, so the device's handling of
subnormal numbers cannot enter a comparison.

The second half restates one row of the TRANSPOSED block product Y = A^T X (option adjoint) for each of the three forms
the generator can be resident in, as the header of kfsp_block_adj.hip defines them: banded_t_exact, ell_t_exact,
box_t_exact.  fma() does not carry the sign of a zero result, so a result that is zero here is compared by value.

The third part restates one row of the FORWARD matrix-free product, which sums a row in orders no stored form has:
box_exact (the single-factor fast path, kernel formats 4, 6, 7, 8 and k_spmm_box) and box_generic_exact (the interpreted
kernel, format 3, and the generator option box_store has the device write out)."""
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


# ---- the transposed rows (Y = A^T X, option adjoint): the three definitions in the header of kfsp_block_adj.hip -------
# X is a list of rows (or an (n, k) array), the result a list of n rows of k floats.  `descending` takes the entries in
# the opposite order and `diag_last` applies the diagonal term after them (fma(-diag, x_r, s) from s = +0.0): two wrong
# kernels, used to show that a test case can tell them from the right one.  A padded entry - a source outside [0, n), a
# missing target, a target outside the box - is an fma of 0.0 against the row's own X row, as the kernels do it.
def _t_row(entries, dg, X, r, descending, diag_last):
    """entries: [(value, X row)] of row r in the promised order -> the row of k results"""
    if descending:
        entries = entries[::-1]
    out = []
    for c in range(len(X[r])):
        s = 0.0 if diag_last else -(dg * X[r][c])
        for v, src in entries:
            s = fma(v, X[src][c], s)
        if diag_last:
            s = fma(-dg, X[r][c], s)
        out.append(s)
    return out


def banded_t_exact(delta, val, diag, X, descending=False, diag_last=False):
    """banded: val[d][r] = A(r, r + delta[d]) as the image stores it.  Row r: s = -(diag[r] x_r), then one fma per
    diagonal, d ascending, of val[d][r - delta[d]] against X row r - delta[d]"""
    delta, val, diag, X = _lists(delta), _lists(val), _lists(diag), _lists(X)
    n = len(diag)
    Y = []
    for r in range(n):
        ent = []
        for d in range(len(delta)):
            src = r - delta[d]
            ent.append((val[d][src], src) if 0 <= src < n else (0.0, r))
        Y.append(_t_row(ent, diag[r], X, r, descending, diag_last))
    return Y


def ell_t_exact(adj, off, diag, X, descending=False, diag_last=False):
    """the reference arrays: row c: s = -(diag[c] x_c), then one fma per slot k ascending of off[c][k] against X row
    adj[c][k] - 1 (a target outside [1, n] is missing)"""
    adj, off, diag, X = _lists(adj), _lists(off), _lists(diag), _lists(X)
    n = len(diag)
    Y = []
    for c in range(n):
        ent = [(off[c][k], adj[c][k] - 1) if 1 <= adj[c][k] <= n else (0.0, c) for k in range(len(adj[c]))]
        Y.append(_t_row(ent, diag[c], X, c, descending, diag_last))
    return Y


def box_slots(mdl):
    """the slots of a single-factor box in the order the device fills them: [species][slot] -> (reaction, its factor
    table), the reactions whose propensity depends on the species by ascending source offset (ties: by reaction).  The
    tables are model.factors()' - the very doubles the device receives."""
    ndep, dep, tab = mdl.factors()
    ndep, dep, tab = _lists(ndep), _lists(dep), _lists(tab)
    assert all(nd == 1 for nd in ndep), "single-factor boxes only"
    at, tables = 0, []
    for k in range(mdl.R):
        tables.append(tab[at:at + mdl.dims[dep[k][0]]])
        at += mdl.dims[dep[k][0]]
    order = sorted(range(mdl.R), key=lambda k: (-int(mdl.offsets[k]), k))
    return [[(k, tables[k]) for k in order if dep[k][0] == s] for s in range(mdl.d)]


def box_t_exact(mdl, X, descending=False):
    """matrix-free box: the accumulator starts at +0.0; by species, then by slot, one fma of a_k(x) - the slot's table
    at the row's own coordinate - against X row r + delta_k when x + nu_k lies in the box (else 0.0 against the row's
    own row); then fma(-dsum, x_r, acc), dsum the species' shares (each the sum of its slots' a_k(x) from 0.0, in slot
    order) added in species order"""
    X = _lists(X)
    slots = box_slots(mdl)
    stoich, offsets, dims, strides = _lists(mdl.stoich), _lists(mdl.offsets), mdl.dims, _lists(mdl.strides)
    Y = []
    for r in range(mdl.n):
        x = [(r // strides[s]) % dims[s] for s in range(mdl.d)]
        ent, dsum = [], None
        for s in range(mdl.d):
            share = 0.0
            for k, table in slots[s]:
                a = table[x[s]]
                share += a
                inside = all(0 <= x[q] + stoich[q][k] < dims[q] for q in range(mdl.d))
                ent.append((a, r + offsets[k]) if inside else (0.0, r))
            dsum = share if dsum is None else dsum + share
        if descending:
            ent = ent[::-1]
        row = []
        for c in range(len(X[r])):
            acc = 0.0
            for a, src in ent:
                acc = fma(a, X[src][c], acc)
            row.append(fma(-dsum, X[r][c], acc))
        Y.append(row)
    return Y


# ---- the forward matrix-free rows (y = A x on a box that stores no entries) -------------------------------------------
# Two definitions, because the device has two: the single-factor fast path (formats 4, 6, 7, 8 and k_spmm_box; header of
# rows_box1 in kfsp_kernels.hip, header of row_box_blk in kfsp_block.hip) groups a row's entries by species and applies
# the diagonal LAST; the interpreted kernel (format 3, row_box) and the generator that box_store writes out
# (k_box_materialize, then an ordinary banded product) take the entries by sorted position and the diagonal FIRST.  Each
# is split in two: *_rows lists, per row, the entries in the promised order and the double that stands for DIAG - no
# arithmetic on x; *_exact does the fused multiply-adds.  The keyword flags are WRONG kernels, used only to show that a
# test case can tell them from the right one (tests/test_row_ref.py).
def _box_geometry(mdl, row0, nloc):
    stoich, offsets = _lists(mdl.stoich), [int(o) for o in _lists(mdl.offsets)]
    dims, strides = list(mdl.dims), [int(s) for s in _lists(mdl.strides)]
    return stoich, offsets, dims, strides, (mdl.n - row0 if nloc is None else nloc)


def box_rows(mdl, row0=0, nloc=None, by_position=False, tie_swapped=False, shares_reversed=False):
    """single-factor box -> per local row ([(a, source)] in species-then-slot order, dsum).  Slot order: box_slots (ascending
    source offset delta_k = -offsets[k], ties by reaction: the host's fill order).  a = table_k[c_s - nu_k[s]] when the
    source state c - nu_k lies in the box in EVERY species, else the entry is (0.0, the row itself).  dsum = share_0 +
    share_1 + ... in species order, share_s the sum from 0.0, in slot order, of table_k[c_s].
    Wrong: by_position - the entries in format 3's order (sorted position, whatever the species); tie_swapped - equal
    offsets within a species filled in descending reaction order; shares_reversed - the shares added last species first."""
    stoich, offsets, dims, strides, nloc = _box_geometry(mdl, row0, nloc)
    slots = box_slots(mdl)
    if tie_swapped:
        slots = [sorted(sp, key=lambda e: (-offsets[e[0]], -e[0])) for sp in slots]
    out = []
    for g in range(row0, row0 + nloc):
        c = [(g // strides[s]) % dims[s] for s in range(mdl.d)]
        ent, shares = [], []
        for s in range(mdl.d):
            share = 0.0
            for k, table in slots[s]:
                share += table[c[s]]
                inside = all(0 <= c[q] - stoich[q][k] < dims[q] for q in range(mdl.d))
                ent.append((k, table[c[s] - stoich[s][k]], g - offsets[k]) if inside else (k, 0.0, g))
            shares.append(share)
        if by_position:
            ent.sort(key=lambda e: (-offsets[e[0]], e[0]))
        if shares_reversed:
            shares = shares[::-1]
        dsum = shares[0]
        for share in shares[1:]:
            dsum += share
        out.append(([(a, src) for _, a, src in ent], dsum))
    return out


def box_exact(mdl, x, row0=0, nloc=None, diag_first=False, **wrong):
    """formats 4, 6, 7, 8 and every column of k_spmm_box: acc = +0.0; one fma(a, x[source], acc) per entry of box_rows;
    then y = fma(-dsum, x[r], acc).  x is the whole vector, the result the local rows [row0, row0 + nloc).
    Wrong: diag_first - the accumulator starts at -(dsum x[r]) (one rounded multiply) and nothing follows the entries;
    the flags of box_rows."""
    x = _lists(x)
    y = []
    for r, (ent, dsum) in enumerate(box_rows(mdl, row0, nloc, **wrong)):
        acc = -(dsum * x[row0 + r]) if diag_first else 0.0
        for a, src in ent:
            acc = fma(a, x[src], acc)
        y.append(acc if diag_first else fma(-dsum, x[row0 + r], acc))
    return y


def box_generic_rows(mdl, row0=0, nloc=None, by_species=False, tie_swapped=False, factors_reversed=False):
    """any box with 1-3 factors per propensity -> per local row ([(a, source)] by sorted position, dsum).  a_k at
    coordinates z is ((t_0[z] t_1[z]) t_2[z]), every multiply rounded, the factors in the order model.factors() lists
    them.  dsum: the sum from 0.0 of a_k(c) in the MODEL's reaction order.  Entries: ascending delta_k = -offsets[k],
    stable by reaction; the value is a_k at the source coordinates c - nu_k when the source lies in the box (row_box
    reuses a_k(c) where no factor species moves: the same look-ups, the same bits), else (0.0, the row itself).
    Wrong: by_species - the entries grouped by the species of their first factor, as the fast path has them;
    tie_swapped - equal offsets in descending reaction order; factors_reversed - the factors multiplied last first
    (shows only with three factors: a product of two commutes)."""
    stoich, offsets, dims, strides, nloc = _box_geometry(mdl, row0, nloc)
    ndep, dep, tab = mdl.factors()
    ndep, dep, tab = _lists(ndep), _lists(dep), _lists(tab)
    at, tables = 0, []
    for k in range(mdl.R):
        tables.append([])
        for i in range(ndep[k]):
            tables[k].append(tab[at:at + dims[dep[k][i]]])
            at += dims[dep[k][i]]

    def a_k(k, z):
        fac = [tables[k][i][z[dep[k][i]]] for i in range(ndep[k])]
        if factors_reversed:
            fac = fac[::-1]
        a = fac[0]
        for t in fac[1:]:
            a = a * t
        return a

    order = sorted(range(mdl.R), key=lambda k: (-offsets[k], -k if tie_swapped else k))
    if by_species:
        order = sorted(order, key=lambda k: dep[k][0])
    out = []
    for g in range(row0, row0 + nloc):
        c = [(g // strides[s]) % dims[s] for s in range(mdl.d)]
        dsum = 0.0
        for k in range(mdl.R):
            dsum += a_k(k, c)
        ent = []
        for k in order:
            z = [c[q] - stoich[q][k] for q in range(mdl.d)]
            inside = all(0 <= z[q] < dims[q] for q in range(mdl.d))
            ent.append((a_k(k, z), g - offsets[k]) if inside else (0.0, g))
        out.append((ent, dsum))
    return out


def box_generic_exact(mdl, x, row0=0, nloc=None, diag_last=False, **wrong):
    """format 3 and the product of the generator box_store writes out: s = -(dsum x[r]) as ONE rounded multiply, then one
    fma(a, x[source], s) per entry of box_generic_rows.  Where no two reactions share an offset this is spmv_exact over
    the box's CSR rows; with a shared offset spmv_exact would order the pair by value, the device by reaction.
    Wrong: diag_last - from +0.0, the diagonal as a closing fma(-dsum, x[r], s); the flags of box_generic_rows."""
    x = _lists(x)
    y = []
    for r, (ent, dsum) in enumerate(box_generic_rows(mdl, row0, nloc, **wrong)):
        s = 0.0 if diag_last else -(dsum * x[row0 + r])
        for a, src in ent:
            s = fma(a, x[src], s)
        y.append(fma(-dsum, x[row0 + r], s) if diag_last else s)
    return y


def reverse_from(rows, cap):
    """every row with its entries from position cap on in reverse order: what a sort that stops at cap entries may
    leave behind (used to show that a test case can tell)"""
    return [row[:cap] + row[cap:][::-1] for row in rows]
