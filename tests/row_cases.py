"""The generators on which the product is compared with tests/row_ref.py, made once per process and shared by
tests/test_row_ref.py (CPU: the restatement itself, and that every case can tell a wrong order from the right one)
and tests/test_gpu_build_rows.py (the device).  Every generator and vector comes from a fixed seed."""
import functools
import os

import numpy as np

from tests import row_ref as RR
from tests.conftest import GOLDEN
from tests.test_gpu_edge_cases import _random_banded_csr, _random_generator


def sort_cap(bw):
    """rows the register sort of the SELL build ranks in one go (k_sell_rank_rows<CAP>, chosen by the slot count
    bw of the upload while build_speculate = 1); None: the insertion sort"""
    return 8 if bw <= 8 else 12 if bw <= 12 else 16 if bw <= 16 else None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _local_generator(n, bw, rng, noffsets=24, reach=40, fill=0.9):
    """links to near neighbours: every slot of every state draws one of `noffsets` index shifts, so a 64-row chunk
    sees few distinct offsets (its columns can be dictionary-coded), no slot is a constant shift (nothing banded),
    a row has up to `noffsets` (+ repeated) entries, and a state that draws one shift twice links twice to one target"""
    shifts = rng.choice(np.r_[-reach:0, 1:reach + 1], size=noffsets, replace=False)
    tgt = np.arange(n)[:, None] + shifts[rng.integers(0, noffsets, size=(n, bw))]
    adj = np.where((tgt >= 0) & (tgt < n) & (rng.random((n, bw)) < fill), tgt + 1, 0).astype(np.int32)
    off = 0.01 + rng.random((n, bw)) * 10.0
    return adj, off, off.sum(axis=1)


def _duplicated_links(n, bw, rng):
    """the random generator with, in every third state, slot 1 naming the target of slot 0 (another value: the tie on
    the key is broken by the value) and, in every ninth, carrying its value too (the tie is broken by position)"""
    adj, off, diag = _random_generator(n, bw, rng, fill=1.0)
    adj[0::3, 1] = adj[0::3, 0]
    off[0::9, 1] = off[0::9, 0]
    return adj, off, off.sum(axis=1)


# name -> (maker, n, bw, seed).  The first four and their seeds are the ones whose long rows were counted on the CPU;
# (65, 20) and (1000, 33) are those of test_unstructured_generators_any_width.
ELL = {
    "4097x8": (_random_generator, 4097, 8, 3),
    "2000x12": (_random_generator, 2000, 12, 0),
    "2000x16": (_random_generator, 2000, 16, 5),
    "1000x4": (_random_generator, 1000, 4, 1),
    "65x20": (_random_generator, 65, 20, 65 * 131 + 20),
    "1000x33": (_random_generator, 1000, 33, 1000 * 131 + 33),
    "duplicated links 600x8": (_duplicated_links, 600, 8, 11),
    "local 1500x8": (_local_generator, 1500, 8, 7),
}
LONG_ROWS = ("4097x8", "2000x12", "2000x16", "duplicated links 600x8", "local 1500x8")   # rows beyond their CAP


@functools.lru_cache(maxsize=None)
def ell_case(name):
    """-> dict(adj, off, diag, x, rows, y): rows and y are the restatement's (y as a float64 array, computed once)"""
    make, n, bw, seed = ELL[name]
    rng = np.random.default_rng(seed)
    adj, off, diag = make(n, bw, rng)
    x = rng.standard_normal(n)
    rows = RR.gather_rows(adj, off, diag)
    y = np.array(RR.spmv_exact(rows, diag, x))
    for a in (adj, off, diag, x, y):
        a.setflags(write=False)
    return dict(adj=adj, off=off, diag=diag, x=x, rows=rows, y=y, n=n, bw=bw)


def made_up_coords(n, seed=17):
    """two 'species' whose lexicographic order is a random permutation of the caller's order"""
    p = np.random.default_rng(seed).permutation(n)
    return np.stack([p // 64, p % 64], axis=1).astype(np.int32)


def lexicographic_rank(state):
    """rank[i] = position of caller's state i in the lexicographic order of the coordinates (first species slowest)"""
    order = np.lexsort(state.T[::-1])
    rank = np.empty(len(state), dtype=np.int64)
    rank[order] = np.arange(len(state))
    return rank


@functools.lru_cache(maxsize=None)
def golden_case(fixture="assembly_goutsias_k10.npz"):
    g = np.load(os.path.join(GOLDEN, fixture))
    adj, off, diag, state = g["adj"], g["offdiag"], g["diag"], g["state"]
    n = len(diag)
    x = np.random.default_rng(23).standard_normal(n)
    rows = RR.gather_rows(adj, off, diag)
    y = np.array(RR.spmv_exact(rows, diag, x))
    return dict(adj=adj, off=off, diag=diag, state=state, x=x, rows=rows, y=y, n=n, bw=adj.shape[1])


# seeds 0 and 1 are too sparse for stored diagonals (the CSR upload keeps them SELL), seed 3 and the toggle box are banded
CSR = ("random banded 0", "random banded 1", "random banded 3", "toggle 70x61")


# a banded generator whose two row blocks each keep 64 trips clear of the halo strips: under option overlap = 2 a rank's
# product is launched in two parts, interior and boundary (tests/test_gpu_nt_loads.py)
CSR_SPLIT = "toggle 150x120"


@functools.lru_cache(maxsize=None)
def csr_case(name):
    if name.startswith("random banded"):
        n, rowptr, col, val, rng = _random_banded_csr(int(name.split()[-1]))
    else:
        from krylovfspssa_amd import synth
        mdl = synth.toggle(*map(int, name.split()[-1].split("x")))
        n = mdl.n
        rowptr, col, val = mdl.csr_rows()
        rng = np.random.default_rng(29)
    x = rng.standard_normal(n)
    rows, diag = RR.rows_from_csr(n, rowptr, col, val)
    y = np.array(RR.spmv_exact(rows, diag, x))
    return dict(n=n, rowptr=rowptr, col=col, val=val, x=x, rows=rows, diag=np.array(diag), y=y)


def drop_vector(adj, n, seed=31, share=0.05):
    """a vector w for which DROP_STATES flags about `share` of the states of a generator with positive rates: a state
    is dropped when w < droptol = 1e-8 and (A w) <= 1e-8.  The chosen states get 1e-12, every state that links into
    one of them 1e-11 (so that what flows into a chosen state stays below 1e-8), all others 1."""
    rng = np.random.default_rng(seed)
    chosen = rng.random(n) < share
    w = np.ones(n)
    src = (np.where(adj > 0, chosen[np.maximum(adj, 1) - 1], False)).any(axis=1)
    w[src] = 1e-11
    w[chosen] = 1e-12
    return w


def compact(adj, off, diag, keep):
    """DROP_STATES on the lists (StateSpace.f90:500-546): kept states move up in order, links are renumbered, a link
    to a dropped state becomes 0 (tests/drop_ref.py compact_lists, which also has the vector and the coordinates)"""
    from tests import drop_ref
    _, adj2, off2, diag2, _ = drop_ref.compact_lists(None, adj, off, diag, None, keep)
    return adj2, off2, diag2
