"""ctypes mirror of the C ABI in include/kfsp.h (libkfsp_hip.so).

This is plumbing for tests, bench.py and Python drivers: numpy arrays in the
reference's own layouts go in, numpy arrays come out; all arithmetic of the hot
path happens in the HIP library.  There is no CPU fallback: importing works
anywhere (so the symbol table can be checked without a GPU), but creating a
context without a usable MI355X raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

M_MAX = 100
T_NAMES = ("arnoldi", "combine", "begin_step", "fsp_callbacks", "host_pade", "upload", "device_onestep")

_lib = None


class KfspError(RuntimeError):
    pass


def library_path():
    return _build.LIB


def load_library():
    """Load libkfsp_hip.so; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise KfspError(f"{path} is missing: run `python -m krylovfspssa_amd.build` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    sig = {
        "kfsp_create": [C.c_int, C.POINTER(vp)],
        "kfsp_destroy": [vp],
        "kfsp_create_group": [C.c_int, vp, C.POINTER(vp)],
        "kfsp_group_size": [vp, C.POINTER(C.c_int)],
        "kfsp_abi_version": [],
        "kfsp_comm_unique_id": [vp],
        "kfsp_comm_init": [vp, C.c_int, C.c_int, vp],
        "kfsp_loopback_create": [C.c_int, C.POINTER(vp)],
        "kfsp_loopback_destroy": [vp],
        "kfsp_comm_init_loopback": [vp, vp, C.c_int],
        "kfsp_row_block": [vp, i64, C.POINTER(i64), C.POINTER(i64)],
        "kfsp_partition": [i64, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)],
        "kfsp_set_matrix_ell": [vp, i32, i32, i32, vp, vp, vp],
        "kfsp_update_matrix_ell": [vp, i32, i32, i32, vp, vp, vp, i32],
        "kfsp_set_matrix_csr": [vp, i64, i64, i64, vp, vp, vp],
        "kfsp_set_state_coords": [vp, i32, i32, i32, vp],
        "kfsp_update_state_coords": [vp, i32, i32, i32, vp, i32],
        "kfsp_set_matrix_box": [vp, i32, vp, i32, vp, vp, vp, vp],
        "kfsp_state_order_active": [vp, C.POINTER(C.c_int)],
        "kfsp_matrix_info": [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)],
        "kfsp_matrix_bytes": [vp, C.c_int, C.POINTER(i64)],
        "kfsp_num_states": [vp, C.POINTER(i64)],
        "kfsp_layout_info": [vp, vp],
        "kfsp_build_info": [vp, vp],
        "kfsp_dia_code_info": [vp, vp],
        "kfsp_dia_code_dict": [vp, C.c_int32, i64, vp, C.POINTER(i64)],
        "kfsp_dia_code_rule": [C.c_int32, vp, i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
        "kfsp_set_trip_order": [vp, i64, vp],
        "kfsp_onestep": [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, C.POINTER(i32), vp, vp],
        "kfsp_onestep_columns": [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32, i32, C.POINTER(i32), vp, vp, vp, i32, vp],
        "kfsp_set_propensity_program": [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp],
        "kfsp_set_propensity_tables2": [vp, i32, vp, vp, vp, vp, vp, i64, vp],
        "kfsp_propensity_overflow": [vp, i32, vp],
        "kfsp_propensities": [vp, i32, vp, i32, vp, i32, vp],
        "kfsp_ssa_streams": [vp, dbl, i64, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, C.POINTER(i32), vp, vp, i32, vp],
        "kfsp_drop_plan": [vp, dbl, C.POINTER(dbl), C.POINTER(i64), C.POINTER(i64)],
        "kfsp_drop_flags": [vp, i64, vp],
        "kfsp_drop_compact": [vp, C.POINTER(i64)],
        "kfsp_drop_rebuild": [vp],
        "kfsp_expand_resident": [vp, dbl, i64, i32, i32, vp, i32, i32, C.POINTER(i64), C.POINTER(i64)],
        "kfsp_download_fsp": [vp, i32, vp, i32, vp, vp, i32, vp],
        "kfsp_dgexpv": [vp, dbl, dbl, dbl, C.c_int, vp, vp],
        "kfsp_set_vector": [vp, i64, vp],
        "kfsp_get_vector": [vp, i64, vp],
        "kfsp_begin_step": [vp, C.POINTER(dbl)],
        "kfsp_arnoldi": [vp, C.c_int, C.c_int, C.c_int, dbl, vp, C.c_int, C.POINTER(C.c_int),
                         C.POINTER(C.c_int), C.POINTER(dbl)],
        "kfsp_combine": [vp, C.c_int, dbl, vp, C.POINTER(dbl)],
        "kfsp_restore_w": [vp, dbl],
        "kfsp_spmv": [vp, vp, vp],
        "kfsp_spmv_w": [vp, vp],
        "kfsp_nrm2_w": [vp, C.POINTER(dbl)],
        "kfsp_asum_w": [vp, C.POINTER(dbl)],
        "kfsp_get_basis": [vp, C.c_int, i64, vp],
        "kfsp_padm": [C.c_int, C.c_int, dbl, vp, C.c_int, vp, C.POINTER(C.c_int), C.POINTER(dbl)],
        "kfsp_expv_fixed": [vp, C.c_int, dbl, C.c_int, vp],
        "kfsp_spmv_bench": [vp, C.c_int, C.c_int, C.POINTER(C.c_float)],
        "kfsp_selftest_stream": [vp, i64, C.c_int, C.c_int, C.POINTER(C.c_float)],
        "kfsp_exchange_bench": [vp, C.c_int, C.POINTER(C.c_float), C.POINTER(i64)],
        "kfsp_add_timer": [vp, C.c_int, dbl],
        "kfsp_get_timers": [vp, vp, C.c_int],
        "kfsp_set_option": [vp, C.c_char_p, i64],
        "kfsp_set_block": [vp, i32, i64, i64, vp],
        "kfsp_get_block": [vp, i32, i64, i64, vp],
        "kfsp_spmm": [vp, i32, i64, vp, vp],
        "kfsp_expv_block": [vp, dbl, dbl, i32, vp, vp],
        "kfsp_spmm_bench": [vp, C.c_int, C.POINTER(C.c_float)],
        "kfsp_block_begin": [vp, i32, vp],
        "kfsp_block_arnoldi": [vp, i32, dbl, vp, vp, vp, vp],
        "kfsp_block_combine": [vp, i32, vp, vp],
        "kfsp_block_info": [vp, vp],
    }
    for name, args in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = C.c_int
    lib.kfsp_last_error.argtypes = [vp]
    lib.kfsp_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


_DROP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_int64))
_EXPAND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.POINTER(C.c_int64))
_LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int)

EV_BEGIN_IOP, EV_WSUM, EV_STEP, EV_REJECT_STEP, EV_DIM_CHANGE, EV_CALL_SSA = 1, 2, 3, 4, 5, 6


class FspOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("drop", _DROP_FN), ("expand", _EXPAND_FN), ("log", _LOG_FN)]


class SolveStats(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("nmult", "nexph", "nscale", "nstep", "nreject", "ibrkflag", "mbrkdwn",
                                         "n_wsum", "n_expand", "n_drop_calls")] + \
               [(k, C.c_double) for k in ("step_min", "step_max", "x_error", "s_error", "tbrkdwn", "t_now",
                                          "hump", "beta")]


class BlockStats(C.Structure):
    """kfsp_block_stats (include/kfsp.h)"""
    _fields_ = [(k, C.c_int32) for k in ("nstep", "nreject", "nmult", "n_breakdown_cols")] + \
               [(k, C.c_double) for k in ("t_now", "step_min", "step_max", "x_error", "s_error")]


BLOCK_K_MAX = 16
BLOCK_M_MAX = 100          # kMMax: the arrays of kfsp_block_arnoldi are laid out for it whatever m is


def _block_columns(W, n):
    """W of shape (n, k) with 1 <= k <= 16 -> a column-major float64 copy; checked before any library call."""
    W = np.asarray(W, dtype=np.float64)
    if W.ndim != 2 or W.shape[0] != n:
        raise ValueError(f"block must have shape (n, k) with n = {n}, got {W.shape}")
    k = W.shape[1]
    if not 1 <= k <= BLOCK_K_MAX:
        raise ValueError(f"block needs 1 <= k <= {BLOCK_K_MAX} columns, got {k}")
    return np.asfortranarray(W), k


def padm(H, t, ideg=6):
    """Host Pade exponential of the library (dgpadm.f:2-169 semantics)."""
    lib = load_library()
    Hf = np.asfortranarray(H, dtype=np.float64)
    m = Hf.shape[0]
    E = np.empty((m, m), dtype=np.float64, order="F")
    ns, hn = C.c_int(0), C.c_double(0.0)
    rc = lib.kfsp_padm(ideg, m, float(t), _p(Hf), m, _p(E), C.byref(ns), C.byref(hn))
    if rc:
        raise KfspError(f"kfsp_padm -> {rc}")
    return E, ns.value, hn.value


def partition(n, nranks, rank):
    """(row0, nrows, L): the contiguous row block of `rank` and the padded block
    length; global index of local row k of rank p is p*L + k (host arithmetic
    of the library, no GPU needed)."""
    r0, nr, L = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = load_library().kfsp_partition(int(n), int(nranks), int(rank), C.byref(r0), C.byref(nr), C.byref(L))
    if rc:
        raise KfspError(f"kfsp_partition -> {rc}")
    return r0.value, nr.value, L.value


class LoopbackGroup:
    """kfsp_loopback_create: nranks contexts of this process exchanging through device copies
    (one-GPU rehearsal of the row partition; see include/kfsp.h)."""

    def __init__(self, nranks):
        self.handle = C.c_void_p()
        rc = load_library().kfsp_loopback_create(int(nranks), C.byref(self.handle))
        if rc:
            raise KfspError(f"kfsp_loopback_create -> {rc}")
        self.nranks = int(nranks)

    def close(self):
        if self.handle:
            load_library().kfsp_loopback_destroy(self.handle)
            self.handle = C.c_void_p()


def run_loopback_ranks(nranks, body, device=0):
    """body(ctx, rank) on nranks contexts of one loop-back group, one thread per rank (ctypes
    releases the GIL inside the library); returns the list of results, re-raises the first error."""
    import threading
    group = LoopbackGroup(nranks)
    results, errors = [None] * nranks, [None] * nranks

    def work(rank):
        try:
            with KfspContext(device) as ctx:
                ctx.comm_init_loopback(group, rank)
                results[rank] = body(ctx, rank)
        except BaseException as e:   # noqa: BLE001 - reported to the caller below
            errors[rank] = e

    threads = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    group.close()
    for e in errors:
        if e is not None:
            raise e
    return results


class KfspContext:
    """One device context = one rank's share of the solver workspace."""

    def __init__(self, device=0, group=None):
        """group = P (int: P ranks, all on `device`, loop-back) or a list of device ids (distinct: RCCL):
        a head handle over a row partition driven by this one thread (kfsp_create_group); it behaves like
        a one-rank context with whole vectors in and out."""
        self._lib = load_library()
        self._h = C.c_void_p()
        if group is not None:
            devs = [int(device)] * int(group) if isinstance(group, int) else [int(d) for d in group]
            arr = (C.c_int * len(devs))(*devs)
            rc = self._lib.kfsp_create_group(len(devs), arr, C.byref(self._h))
            self.group_size = len(devs)
        else:
            rc = self._lib.kfsp_create(int(device), C.byref(self._h))
            self.group_size = 1
        if rc:
            self._h = C.c_void_p()
            raise KfspError(f"kfsp_create(device={device}, group={group}) -> {rc}: no usable HIP device; "
                            "the exp(tA)v hot path has no CPU fallback")
        self.n = 0
        self.nranks, self.rank = 1, 0

    # -- lifetime
    def close(self):
        if self._h:
            self._lib.kfsp_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            msg = self._lib.kfsp_last_error(self._h)
            raise KfspError(f"{what} -> {rc}: {msg.decode() if msg else ''}")

    # -- partition
    @staticmethod
    def unique_id():
        buf = np.zeros(128, dtype=np.uint8)
        rc = load_library().kfsp_comm_unique_id(_p(buf))
        if rc:
            raise KfspError(f"kfsp_comm_unique_id -> {rc}")
        return buf

    def comm_init(self, nranks, rank, id_bytes=None):
        buf = None if id_bytes is None else np.ascontiguousarray(id_bytes, dtype=np.uint8)
        self._chk(self._lib.kfsp_comm_init(self._h, nranks, rank, None if buf is None else _p(buf)), "kfsp_comm_init")
        self.nranks, self.rank = nranks, rank

    def comm_init_loopback(self, group, rank):
        """Join a LoopbackGroup (ranks = contexts of this process, one host thread each)."""
        self._chk(self._lib.kfsp_comm_init_loopback(self._h, group.handle, int(rank)), "kfsp_comm_init_loopback")
        self.nranks, self.rank = group.nranks, int(rank)

    def row_block(self, n):
        r0, nr = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.kfsp_row_block(self._h, int(n), C.byref(r0), C.byref(nr)), "kfsp_row_block")
        return r0.value, nr.value

    # -- generator
    def set_matrix_ell(self, adj, offdiag, diag):
        """FSP_MATRIX arrays as [state][slot] numpy arrays (= Fortran (slot,state))."""
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        offdiag = np.ascontiguousarray(offdiag, dtype=np.float64)
        diag = np.ascontiguousarray(diag, dtype=np.float64)
        n, bw = adj.shape
        assert offdiag.shape == (n, bw) and diag.shape == (n,)
        self._chk(self._lib.kfsp_set_matrix_ell(self._h, n, bw, bw, _p(adj), _p(offdiag), _p(diag)),
                  "kfsp_set_matrix_ell")
        self.n = n
        self.row0, self.nloc = self.row_block(n)

    def update_matrix_ell(self, adj, offdiag, diag, n_unchanged):
        """set_matrix_ell after the FSP grew: OFFDIAG / DIAG of the first n_unchanged states stay on the device."""
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        offdiag = np.ascontiguousarray(offdiag, dtype=np.float64)
        diag = np.ascontiguousarray(diag, dtype=np.float64)
        n, bw = adj.shape
        self._chk(self._lib.kfsp_update_matrix_ell(self._h, n, bw, bw, _p(adj), _p(offdiag), _p(diag), int(n_unchanged)),
                  "kfsp_update_matrix_ell")
        self.n = n
        self.row0, self.nloc = self.row_block(n)

    def set_state_coords(self, state):
        """FSP%STATE as a [state][species] array, for the next set_matrix_ell of the
        same size (internal lexicographic state order, include/kfsp.h)."""
        state = np.ascontiguousarray(state, dtype=np.int32)
        n, ns = state.shape
        self._chk(self._lib.kfsp_set_state_coords(self._h, n, ns, ns, _p(state)), "kfsp_set_state_coords")

    def update_state_coords(self, state, n_unchanged):
        """set_state_coords after the FSP grew: only the coordinates behind the first n_unchanged states travel"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        n, ns = state.shape
        self._chk(self._lib.kfsp_update_state_coords(self._h, n, ns, ns, _p(state), int(n_unchanged)), "kfsp_update_state_coords")

    def state_order_active(self):
        a = C.c_int(0)
        self._chk(self._lib.kfsp_state_order_active(self._h, C.byref(a)), "kfsp_state_order_active")
        return bool(a.value)

    def set_matrix_csr(self, n, rowptr, col, val, row0=None):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        r0, nr = self.row_block(n)
        if row0 is None:
            row0 = r0
        assert len(rowptr) == nr + 1, (len(rowptr), nr)
        self._chk(self._lib.kfsp_set_matrix_csr(self._h, int(n), int(row0), int(nr), _p(rowptr), _p(col), _p(val)),
                  "kfsp_set_matrix_csr")
        self.n = int(n)
        self.row0, self.nloc = r0, nr

    def set_matrix_box(self, model, store=None):
        """Matrix-free generator of a synth.BoxModel with separable propensities (model.factors()).
        store=True: the device writes the same generator out as stored diagonals (option box_store)."""
        if store is not None:
            self.set_option("box_store", 1 if store else 0)
        dims = np.ascontiguousarray(model.dims, dtype=np.int32)
        stoich = np.ascontiguousarray(np.asarray(model.stoich).T, dtype=np.int32)      # [nr][ns]
        ndep, deps, tables = model.factors()
        ndep = np.ascontiguousarray(ndep, dtype=np.int32)
        deps = np.ascontiguousarray(deps, dtype=np.int32)
        tables = np.ascontiguousarray(tables, dtype=np.float64)
        self._chk(self._lib.kfsp_set_matrix_box(self._h, len(dims), _p(dims), stoich.shape[0], _p(stoich), _p(ndep),
                                                _p(deps), _p(tables)), "kfsp_set_matrix_box")
        self.n = int(model.n)
        self.row0, self.nloc = self.row_block(self.n)

    def matrix_info(self):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.kfsp_matrix_info(self._h, C.byref(a), C.byref(b), C.byref(c)), "kfsp_matrix_info")
        return dict(rows=a.value, slots=b.value, nnz=c.value)

    # -- vectors
    def onestep(self, stoich, state, adj, max_count=10000, capacity=None):
        """ONESTEP_EXTENDER's integer work on the device: (state [n][ns], adj [n][nr]) -> (state', adj')
        of the extended FSP (new states appended in the reference's order, all links completed)."""
        state = np.ascontiguousarray(state, dtype=np.int32)
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        stoich = np.ascontiguousarray(stoich, dtype=np.int32)          # [nr][ns]
        n, ns = state.shape
        nr = adj.shape[1]
        assert stoich.shape == (nr, ns)
        cap = int(capacity) if capacity else n * (nr + 1) + 16
        n_new = C.c_int32(0)
        st_new = np.zeros((cap - n + 1, ns), dtype=np.int32)
        adj_out = np.zeros((cap, nr), dtype=np.int32)
        self._chk(self._lib.kfsp_onestep(self._h, ns, nr, _p(stoich), n, _p(state), ns, _p(adj), nr, int(max_count), cap,
                                         C.byref(n_new), _p(st_new), _p(adj_out)), "kfsp_onestep")
        m = n_new.value
        return np.concatenate([state, st_new[:m - n]]), adj_out[:m].copy()

    def onestep_columns(self, stoich, state, adj, max_count=10000, capacity=None):
        """onestep that also returns the propensity columns (offdiag [m][nr], diag [m]) of the appended states"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        stoich = np.ascontiguousarray(stoich, dtype=np.int32)
        n, ns = state.shape
        nr = adj.shape[1]
        cap = int(capacity) if capacity else n * (nr + 1) + 16
        n_new = C.c_int32(0)
        st_new = np.zeros((cap - n + 1, ns), dtype=np.int32)
        adj_out = np.zeros((cap, nr), dtype=np.int32)
        off_new = np.zeros((cap - n + 1, nr))
        diag_new = np.zeros(cap - n + 1)
        self._chk(self._lib.kfsp_onestep_columns(self._h, ns, nr, _p(stoich), n, _p(state), ns, _p(adj), nr, int(max_count), cap,
                                                 C.byref(n_new), _p(st_new), _p(adj_out), _p(off_new), nr, _p(diag_new)),
                  "kfsp_onestep_columns")
        m = n_new.value
        return np.concatenate([state, st_new[:m - n]]), adj_out[:m].copy(), off_new[:m - n].copy(), diag_new[:m - n].copy()

    def ssa_streams(self, timestep, seedmix, stoich, state, adj, offdiag, diag, max_count=10000, capacity_new=None):
        """the independent-stream SSA walk: (new states [m][ns], offdiag [m][nr], diag [m]) in order of first occurrence"""
        state = np.ascontiguousarray(state, dtype=np.int32)
        adj = np.ascontiguousarray(adj, dtype=np.int32)
        offdiag = np.ascontiguousarray(offdiag, dtype=np.float64)
        diag = np.ascontiguousarray(diag, dtype=np.float64)
        stoich = np.ascontiguousarray(stoich, dtype=np.int32)
        n, ns = state.shape
        nr = adj.shape[1]
        cap = int(capacity_new) if capacity_new else 4 * n + 4096
        nf = C.c_int32(0)
        st_new = np.zeros((cap, ns), dtype=np.int32)
        off_new = np.zeros((cap, nr))
        diag_new = np.zeros(cap)
        self._chk(self._lib.kfsp_ssa_streams(self._h, float(timestep), int(seedmix), ns, nr, _p(stoich), n, _p(state), ns, _p(adj),
                                             _p(offdiag), nr, _p(diag), int(max_count), cap, C.byref(nf), _p(st_new), _p(off_new), nr,
                                             _p(diag_new)), "kfsp_ssa_streams")
        m = nf.value
        return st_new[:m].copy(), off_new[:m].copy(), diag_new[:m].copy()

    def expand_resident(self, t_ssa, seedmix, stoich, max_count=10000, capacity=None):
        """SSA walk (t_ssa > 0) + one-step sweep on the resident lists; returns (n_new, n_from_ssa)"""
        stoich = np.ascontiguousarray(stoich, dtype=np.int32)
        nr, ns = stoich.shape
        cap = int(capacity) if capacity else 2 ** 31 - 2
        n_new, n_ssa = C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.kfsp_expand_resident(self._h, float(t_ssa), int(seedmix), ns, nr, _p(stoich), int(max_count), cap,
                                                 C.byref(n_new), C.byref(n_ssa)), "kfsp_expand_resident")
        self.n = n_new.value
        self.row0, self.nloc = self.row_block(self.n)
        return n_new.value, n_ssa.value

    def download_fsp(self, ns, nr):
        """the resident lists: (state [n][ns], adj [n][nr], offdiag [n][nr], diag [n])"""
        n = self.n
        state = np.zeros((n, ns), dtype=np.int32)
        adj = np.zeros((n, nr), dtype=np.int32)
        off = np.zeros((n, nr))
        diag = np.zeros(n)
        self._chk(self._lib.kfsp_download_fsp(self._h, n, _p(state), ns, _p(adj), _p(off), nr, _p(diag)), "kfsp_download_fsp")
        return state, adj, off, diag

    def set_propensity_program(self, ns, params, programs, tables=None):
        """programs: per reaction (code list, immediates list); tables: None or (tab_species [nr], tab [nr][tab_len])"""
        nr = len(programs)
        code_off = np.concatenate(([0], np.cumsum([len(c) for c, _ in programs]))).astype(np.int32)
        imm_off = np.concatenate(([0], np.cumsum([len(i) for _, i in programs]))).astype(np.int32)
        code = np.array([v for c, _ in programs for v in c] or [0], dtype=np.int32)
        imm = np.array([v for _, i in programs for v in i] or [0.0], dtype=np.float64)
        params = np.ascontiguousarray(params, dtype=np.float64)
        if tables is None:
            ts, tab, tl = np.full(nr, -1, dtype=np.int32), np.zeros(1), 0
        else:
            ts = np.ascontiguousarray(tables[0], dtype=np.int32)
            tab = np.ascontiguousarray(tables[1], dtype=np.float64)
            tl = tab.shape[1]
        self._chk(self._lib.kfsp_set_propensity_program(self._h, int(ns), nr, len(params), _p(params) if len(params) else None,
                                                        _p(code_off), _p(code), _p(imm_off), _p(imm), _p(ts), int(tl), _p(tab)),
                  "kfsp_set_propensity_program")
        self._prop_nr = nr

    def set_propensity_tables2(self, s1, s2, n1, n2, off, tab2):
        """two-species tables of the program just set: reaction k with s1[k] >= 0 reads tab2[off[k] + x[s2[k]] * n1[k] + x[s1[k]]]
        (s1, s2, n1, n2 int32 [nr], off int64 [nr], tab2 float64); a population beyond a table makes the operation that met it
        raise KfspError with status -16 (propensity_overflow says which species went how far)"""
        s1, s2, n1, n2 = (np.ascontiguousarray(a, dtype=np.int32) for a in (s1, s2, n1, n2))
        off = np.ascontiguousarray(off, dtype=np.int64)
        tab2 = np.ascontiguousarray(tab2, dtype=np.float64).reshape(-1)
        nr = len(s1)
        if not (len(s2) == len(n1) == len(n2) == len(off) == nr):
            raise ValueError("s1, s2, n1, n2 and off must have one entry per reaction")
        self._chk(self._lib.kfsp_set_propensity_tables2(self._h, nr, _p(s1), _p(s2), _p(n1), _p(n2), _p(off), len(tab2),
                                                        _p(tab2) if len(tab2) else None), "kfsp_set_propensity_tables2")

    def propensity_overflow(self, ns):
        """after a -16: per species the largest population that lay beyond a two-species table (0: none), int32 [ns]"""
        missed = np.zeros(int(ns), dtype=np.int32)
        self._chk(self._lib.kfsp_propensity_overflow(self._h, int(ns), _p(missed)), "kfsp_propensity_overflow")
        return missed

    def propensities(self, state):
        state = np.ascontiguousarray(state, dtype=np.int32)
        n, ns = state.shape
        off = np.zeros((n, self._prop_nr))
        diag = np.zeros(n)
        self._chk(self._lib.kfsp_propensities(self._h, n, _p(state), ns, _p(off), self._prop_nr, _p(diag)), "kfsp_propensities")
        return off, diag

    def drop_plan(self, dsum):
        """DROP_STATES decision on the device -> (droptol, drop_count, n_flagged)."""
        tol, cnt, nf = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.kfsp_drop_plan(self._h, float(dsum), C.byref(tol), C.byref(cnt), C.byref(nf)), "kfsp_drop_plan")
        return tol.value, cnt.value, nf.value

    def drop_flags(self):
        f = np.zeros(self.n, dtype=np.uint8)
        self._chk(self._lib.kfsp_drop_flags(self._h, int(self.n), _p(f)), "kfsp_drop_flags")
        return f

    def drop_compact(self):
        n = C.c_int64(0)
        self._chk(self._lib.kfsp_drop_compact(self._h, C.byref(n)), "kfsp_drop_compact")
        return n.value

    def drop_rebuild(self):
        """the generator of the compacted FSP from the device's own arrays (after drop_compact)"""
        self._chk(self._lib.kfsp_drop_rebuild(self._h), "kfsp_drop_rebuild")
        n = C.c_int64(0)
        self._lib.kfsp_num_states(self._h, C.byref(n))
        self.n = n.value
        self.row0, self.nloc = self.row_block(self.n)

    def matrix_bytes(self, force_sell=False):
        """force_sell: False / True (the SELL image) / 3 (the SELL image read with plain columns)"""
        b = C.c_int64(0)
        self._chk(self._lib.kfsp_matrix_bytes(self._h, int(force_sell), C.byref(b)), "kfsp_matrix_bytes")
        return b.value

    def set_trip_order(self, order):
        """order of the product's wavefront trips (None: ascending)"""
        if order is None:
            self._chk(self._lib.kfsp_set_trip_order(self._h, 0, None), "kfsp_set_trip_order")
            return
        order = np.ascontiguousarray(order, dtype=np.int32)
        self._chk(self._lib.kfsp_set_trip_order(self._h, len(order), _p(order)), "kfsp_set_trip_order")

    def layout_info(self):
        v = np.zeros(8, dtype=np.int64)
        self._chk(self._lib.kfsp_layout_info(self._h, _p(v)), "kfsp_layout_info")
        keys = ("format", "exchange", "halo_rows", "sell_reach", "coded_chunks", "chunks", "code_words", "state_order")
        return dict(zip(keys, (int(x) for x in v)))

    def dia_code_info(self):
        """the dictionary-coded image of a banded generator's values (kfsp_dia_code_info).  "diag_table_bytes": bytes of the
        DIAG tables when DIAG is folded into the records' spare bits (option "dia_code_diag": -1 - the default - where
        "dia_code"'s size gate passes, 0 never, 1 always try), 0 while DIAG is read as an 8-byte stream.  "neighbours": where the
        product takes the pairs of x of the +-1 diagonals from - "lanes" (the neighbour lanes' registers: DIAG folded and
        option "dia_code_lanes" = 1), "loads" (DIAG folded, "dia_code_lanes" = 0, the default) or "" (no fold: loads, as ever).
        "inner": 1 where the folded product runs its interior 128-row groups on the path without clamps (option
        "dia_code_inner" = 1, "neighbours" = "loads", 6 diagonals on three strides or 4 on two), else 0"""
        v = np.zeros(26, dtype=np.int64)
        self._chk(self._lib.kfsp_dia_code_info(self._h, _p(v)), "kfsp_dia_code_info")
        keys = ("width", "record_bytes", "coded_bytes", "dict_bytes", "diagonals", "build_us", "active", "diag_table_bytes")
        out = dict(zip(keys, (int(x) for x in v[:8])))
        out["distinct"] = [int(x) for x in v[8:8 + out["diagonals"]]]
        out["neighbours"] = ("", "loads", "lanes")[int(v[24])]
        out["inner"] = int(v[25])
        return out

    def dia_code_dict(self, d):
        """dictionary of diagonal d of the coded image, ascending as unsigned 64-bit patterns"""
        n = C.c_int64(0)
        self._chk(self._lib.kfsp_dia_code_dict(self._h, int(d), 0, None, C.byref(n)), "kfsp_dia_code_dict")
        out = np.empty(n.value, dtype=np.float64)
        self._chk(self._lib.kfsp_dia_code_dict(self._h, int(d), n.value, _p(out), C.byref(n)), "kfsp_dia_code_dict")
        return out

    def build_info(self):
        """how the rebuilds of a resident FSP went, and "pencil_order": the length of the tiled base-trip order the pencil
        kernel (format 7) is given for the current box (option box_tile), 0 when it takes them ascending (kfsp_build_info)"""
        v = np.zeros(6, dtype=np.int64)
        self._chk(self._lib.kfsp_build_info(self._h, _p(v)), "kfsp_build_info")
        return dict(zip(("speculative", "repeated", "sell", "key_layout_cached", "orders_carried_over", "pencil_order"), (int(x) for x in v)))

    def set_vector(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self._lib.kfsp_set_vector(self._h, len(w), _p(w)), "kfsp_set_vector")

    def get_vector(self):
        w = np.empty(self.nloc, dtype=np.float64)
        self._chk(self._lib.kfsp_get_vector(self._h, self.nloc, _p(w)), "kfsp_get_vector")
        return w

    def get_basis(self, j):
        v = np.empty(self.nloc, dtype=np.float64)
        self._chk(self._lib.kfsp_get_basis(self._h, int(j), self.nloc, _p(v)), "kfsp_get_basis")
        return v

    # -- hot path
    def begin_step(self):
        b = C.c_double(0.0)
        self._chk(self._lib.kfsp_begin_step(self._h, C.byref(b)), "kfsp_begin_step")
        return b.value

    def arnoldi(self, m, jold=1, qiop=2, break_tol=1e-7, H=None):
        """-> (H[(m+2),(m+2)] F-order, mbrkdwn, k1, avnorm)."""
        mh = m + 2
        if H is None:
            H = np.zeros((mh, mh), dtype=np.float64, order="F")
        assert H.flags.f_contiguous and H.shape[0] >= mh
        mb, k1, av = C.c_int(0), C.c_int(0), C.c_double(0.0)
        self._chk(self._lib.kfsp_arnoldi(self._h, m, jold, qiop, float(break_tol), _p(H), H.shape[0],
                                         C.byref(mb), C.byref(k1), C.byref(av)), "kfsp_arnoldi")
        return H, mb.value, k1.value, av.value

    def combine(self, mx, beta, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert len(y) >= mx
        ws = C.c_double(0.0)
        self._chk(self._lib.kfsp_combine(self._h, int(mx), float(beta), _p(y), C.byref(ws)), "kfsp_combine")
        return ws.value

    def restore_w(self, beta):
        self._chk(self._lib.kfsp_restore_w(self._h, float(beta)), "kfsp_restore_w")

    def spmv(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert len(x) == self.n
        y = np.empty(self.nloc, dtype=np.float64)
        self._chk(self._lib.kfsp_spmv(self._h, _p(x), _p(y)), "kfsp_spmv")
        return y

    def spmv_w(self):
        y = np.empty(self.nloc, dtype=np.float64)
        self._chk(self._lib.kfsp_spmv_w(self._h, _p(y)), "kfsp_spmv_w")
        return y

    def nrm2_w(self):
        o = C.c_double(0.0)
        self._chk(self._lib.kfsp_nrm2_w(self._h, C.byref(o)), "kfsp_nrm2_w")
        return o.value

    def asum_w(self):
        o = C.c_double(0.0)
        self._chk(self._lib.kfsp_asum_w(self._h, C.byref(o)), "kfsp_asum_w")
        return o.value

    def dgexpv(self, t, fsptol, krytol, n_reactions, drop=None, expand=None):
        """The adaptive solver (DGEXPV_FSP, KrylovSolver.f90:151-573) on the resident
        generator and vector.  drop(dsum) / expand(t_ssa) are Python callables that
        return the new number of states (they re-upload through this context).
        -> (return code, SolveStats, log) with log = list of (event, values)."""
        log = []

        def _log(_u, ev, vals, n):
            log.append((ev, [vals[i] for i in range(n)]))

        def _wrap(fn):
            def cb(_u, x, n_new):
                try:
                    r = fn(x)
                    if r is not None:
                        n_new[0] = int(r)
                    return 0
                except Exception as e:      # never let an exception cross the C boundary
                    log.append((-1, repr(e)))
                    return 4000
            return cb
        ops = FspOps(None, _DROP_FN(_wrap(drop)) if drop else _DROP_FN(), _EXPAND_FN(_wrap(expand)) if expand else _EXPAND_FN(),
                     _LOG_FN(_log))
        st = SolveStats()
        rc = self._lib.kfsp_dgexpv(self._h, float(t), float(fsptol), float(krytol), int(n_reactions),
                                   C.byref(ops), C.byref(st))
        if rc not in (0, 10):
            self._chk(rc, "kfsp_dgexpv")
        n = C.c_int64(0)
        self._lib.kfsp_num_states(self._h, C.byref(n))
        self.n = n.value
        self.row0, self.nloc = self.row_block(self.n)
        return rc, st, log

    def expv_fixed(self, m, tau, nsteps):
        ws = np.zeros(max(nsteps, 1), dtype=np.float64)
        self._chk(self._lib.kfsp_expv_fixed(self._h, int(m), float(tau), int(nsteps), _p(ws)), "kfsp_expv_fixed")
        return ws[:nsteps]

    def spmv_bench(self, reps, variant=0):
        ms = C.c_float(0.0)
        self._chk(self._lib.kfsp_spmv_bench(self._h, int(reps), int(variant), C.byref(ms)), "kfsp_spmv_bench")
        return ms.value

    def exchange_bench(self, reps):
        """-> (ms for reps exchanges of the source vector alone, bytes this rank receives per exchange)"""
        ms, b = C.c_float(0.0), C.c_int64(0)
        self._chk(self._lib.kfsp_exchange_bench(self._h, int(reps), C.byref(ms), C.byref(b)), "kfsp_exchange_bench")
        return ms.value, b.value

    def selftest_stream(self, nbytes, elem_bytes, reps=1):
        ms = C.c_float(0.0)
        self._chk(self._lib.kfsp_selftest_stream(self._h, int(nbytes), int(elem_bytes), int(reps), C.byref(ms)),
                  "kfsp_selftest_stream")
        return ms.value

    def timers(self, reset=False):
        t = np.zeros(len(T_NAMES))
        self._chk(self._lib.kfsp_get_timers(self._h, _p(t), int(reset)), "kfsp_get_timers")
        return dict(zip(T_NAMES, t.tolist()))

    # -- several vectors at once
    def _block_rows(self):
        """rows of a block on this context: the rank's nloc; one rank and a head hold all n"""
        return getattr(self, "nloc", self.n)

    def set_block(self, W):
        """k start vectors as the columns of W (shape n x k, 1 <= k <= 16), caller's state order.
        Stored generators; a matrix-free box (set_matrix_box(..., store=False)) only after set_option("block_box", 1) -
        single-factor boxes - or set_option("block_box", 2) - any box: propensities of two or three factors (bimolecular
        reactions), jumps beyond 2, more than four propensities on a species, more than six species.
        On a rank of a row partition (set_option("block_partition", 1) first): this rank's nloc rows, as in set_vector.
        With set_option("block_integral", 1) in force, a second block J of the same shape is kept beside W, zeroed here:
        every accepted step of expv_block adds int_0^tau exp(sA) W_step ds to it (get_block(integral=True)).
        While a target set is resident (set_block_target) the block stored is D W: +0.0 on the states of the set."""
        nloc = self._block_rows()
        Wf, k = _block_columns(W, nloc)
        self._chk(self._lib.kfsp_set_block(self._h, k, nloc, max(nloc, 1), _p(Wf)), "kfsp_set_block")
        self.block_k = k

    def get_block(self, integral=False):
        """The resident block W, n x k in the caller's state order.  integral=True: J instead, the time integral
        int_0^T exp(sA) W_0 ds accumulated over every expv_block since set_block (T = the sum of their t) - forward the
        occupation measure (expected time spent in each state), backward (adjoint=True) the accumulated observable
        E[int_0^min(T, exit) g(X_s) ds | X_0 = x], for g = 1 the truncated mean exit time.  Needs
        set_option("block_integral", 1) before set_block; the option is set to 2 round the call and put back.  J has no
        step control of its own: about T times the error bound of W (include/kfsp.h, TIME INTEGRALS).
        Under a target set W and J are exactly +0.0 on the set; set_block_target discards the block, so this raises
        until the next set_block."""
        k = getattr(self, "block_k", 0)
        if not 1 <= k <= BLOCK_K_MAX:
            raise KfspError("no block was set on this context")
        nloc = self._block_rows()
        W = np.empty((nloc, k), dtype=np.float64, order="F")
        call = lambda: self._chk(self._lib.kfsp_get_block(self._h, k, nloc, max(nloc, 1), _p(W)), "kfsp_get_block")
        if not integral:
            call()
            return W
        old = getattr(self, "_options", {}).get("block_integral", 0)
        self.set_option("block_integral", 2)
        try:
            call()
        finally:
            self.set_option("block_integral", old)
        return W

    def _with_block_options(self, call, adjoint, clamp):
        """call() with option "adjoint" = 1 / "block_clamp" = 0 where asked for; afterwards each option that was changed
        is back at what set_option last set (else the library's default).  A forward, clamped call touches no option."""
        seen = getattr(self, "_options", {})
        todo = []
        if adjoint:
            todo.append(("adjoint", 1, seen.get("adjoint", 0)))
        if not clamp:
            todo.append(("block_clamp", 0, seen.get("block_clamp", 1)))
        for name, v, _ in todo:
            self.set_option(name, v)
        try:
            return call()
        finally:
            for name, _, old in todo:
                self.set_option(name, old)

    def spmm(self, X, adjoint=False):
        """A X for the columns of X (shape n x k, 1 <= k <= 16); column j is bit-identical to spmv(X[:, j]) - also on a
        matrix-free box under set_option("block_box", 1), and on a multi-factor one (or any box under "box_generic" = 1)
        under set_option("block_box", 2).  adjoint=True: A^T X (option "adjoint" round the call).
        On a rank of a row partition X is the whole block (n rows) and the rank's nloc rows of A X come back, as in spmv.
        While a target set is resident: D A D X (D A^T D X), the product with the killed generator - +0.0 on the set.
        Under set_option("block_dia_code", 1) the forward product of a banded generator with a coded image
        (dia_code_info()["active"]) reads one record per row and the dictionaries in LDS instead of the value streams: the
        same bits; block_info() tells which kernel ran.  With set_option("block_dia_code_adjoint", 1) beside it the same holds
        for adjoint=True: A^T X from the records of the source rows (one 8-byte record word per diagonal), bit-identical to
        the plain transposed product, reported as fmt 9 with adjoint 1."""
        Xf, k = _block_columns(X, self.n)
        Y = np.empty((self.n, k), dtype=np.float64, order="F")
        self._with_block_options(lambda: self._chk(self._lib.kfsp_spmm(self._h, k, self.n, _p(Xf), _p(Y)), "kfsp_spmm"),
                                 adjoint, True)
        nloc = self._block_rows()
        return Y if nloc == self.n else np.asfortranarray(Y[:nloc])

    def expv_block(self, t, tol, m=30, adjoint=False, clamp=True):
        """W <- exp(t A) W for the resident block -> (wsum[k], BlockStats).  adjoint=True: the backward solve
        W <- exp(t A^T) W, E[f(X_t); still inside the FSP | X_0 = x] for every state x and observable column f;
        clamp=False: columns are not clamped at 0 after a step (signed observables) and wsum is their l1 norm.  Both are
        the options "adjoint" / "block_clamp", set round the call and put back to forward / clamped.
        Under set_option("block_integral", 1) (in force since before set_block) every accepted step also adds its time
        integral to J (get_block(integral=True)); W, wsum and the statistics are the same bits with and without.
        While a target set is resident the solve is the one of the killed generator Q = D A D: wsum is the survival
        probability, block_hit() the first-passage density and block_hit(integral=True) the probability of having
        reached the set (include/kfsp.h, TARGET SETS)."""
        k = getattr(self, "block_k", 0)
        if not 1 <= k <= BLOCK_K_MAX:
            raise KfspError("no block was set on this context")
        ws = np.zeros(BLOCK_K_MAX, dtype=np.float64)
        st = BlockStats()
        self._with_block_options(lambda: self._chk(self._lib.kfsp_expv_block(self._h, float(t), float(tol), int(m), _p(ws),
                                                                             C.byref(st)), "kfsp_expv_block"), adjoint, clamp)
        return ws[:k].copy(), st

    def _block_k(self):
        k = getattr(self, "block_k", 0)
        if not 1 <= k <= BLOCK_K_MAX:
            raise KfspError("no block was set on this context")
        return k

    def block_begin(self, m):
        """u_1 = W for the resident block -> beta[k] (kfsp_block_begin); the basis is laid out for dimension m."""
        k = self._block_k()
        beta = np.zeros(BLOCK_K_MAX, dtype=np.float64)
        self._chk(self._lib.kfsp_block_begin(self._h, int(m), _p(beta)), "kfsp_block_begin")
        return beta[:k].copy()

    def block_arnoldi(self, m, break_tol=1e-7):
        """IOP(2) Arnoldi of dimension m for every column -> (hb, nrm, brk, avnorm): hb[j, t, c] = H(j-1,j), H(j,j),
        H(j+1,j) (t = 0, 1, 2) of column c for j = 1..m (row 0 is unused), nrm[j, c] = ||u_j|| for j = 1..m+1, brk[c]
        = 0, the column a breakdown ended c after, or -1 (beta = 0), avnorm[c]."""
        k = self._block_k()
        hb = np.zeros(((BLOCK_M_MAX + 2), 3, BLOCK_K_MAX), dtype=np.float64)
        nrm = np.zeros((BLOCK_M_MAX + 3, BLOCK_K_MAX), dtype=np.float64)
        brk = np.zeros(BLOCK_K_MAX, dtype=np.int32)
        avn = np.zeros(BLOCK_K_MAX, dtype=np.float64)
        self._chk(self._lib.kfsp_block_arnoldi(self._h, int(m), float(break_tol), _p(hb), _p(nrm), _p(brk), _p(avn)),
                  "kfsp_block_arnoldi")
        return hb[:m + 1, :, :k].copy(), nrm[:m + 2, :k].copy(), brk[:k].copy(), avn[:k].copy()

    def block_combine(self, mx, coef, coef_integral=None):
        """W_c = max(sum_{i < mx} coef[i, c] u_{i+1,c}, 0) for the resident block -> wsum[k] (of W).
        Under option "block_integral" the library reads a second table behind the first, and in the same pass
        J_c += sum_{i < mx} coef_integral[i, c] u_{i+1,c} (never clamped); coef_integral=None leaves J as it is (a table of
        zeros).  With the option off the second table is not read."""
        k = self._block_k()
        coef = np.asarray(coef, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] < mx or coef.shape[1] != k:
            raise ValueError(f"coef must have shape (>= {mx}, {k}), got {coef.shape}")
        cf = np.zeros((2 * int(mx), BLOCK_K_MAX), dtype=np.float64)
        cf[:mx, :k] = coef[:mx]
        if coef_integral is not None:
            cj = np.asarray(coef_integral, dtype=np.float64)
            if cj.ndim != 2 or cj.shape[0] < mx or cj.shape[1] != k:
                raise ValueError(f"coef_integral must have shape (>= {mx}, {k}), got {cj.shape}")
            cf[mx:, :k] = cj[:mx]
        ws = np.zeros(BLOCK_K_MAX, dtype=np.float64)
        self._chk(self._lib.kfsp_block_combine(self._h, int(mx), _p(cf), _p(ws)), "kfsp_block_combine")
        return ws[:k].copy()

    def block_info(self):
        """how the last block calls ran (kfsp_block_info).  While option "block_dia_code" is on, every block product writes
        "fmt" and "lds_bytes": 9 and the dynamic LDS of the launch (the dictionaries) when the coded kernel ran, else 0 and 0.
        With the option off the two slots are what they always were (the one-launch small pass fills them).  Under "adjoint" the
        coded kernel runs only with option "block_dia_code_adjoint" = 1 as well: "fmt" 9 with "adjoint" 1 is the transposed
        coded kernel; with that option at 0 a transposed product reports 0 and 0."""
        v = np.zeros(8, dtype=np.int64)
        self._chk(self._lib.kfsp_block_info(self._h, _p(v)), "kfsp_block_info")
        return dict(zip(("one_launch", "fmt", "begin_launches", "arnoldi_launches", "combine_launches", "lds_bytes", "adjoint", "exchange"),
                        (int(x) for x in v[:8])))

    def _target_mode(self, mode, call):
        """call() under option "block_target" = mode (the call modes of include/kfsp.h, TARGET SETS), then 0 again"""
        self.set_option("block_target", mode)
        try:
            return call()
        finally:
            self.set_option("block_target", 0)

    def set_block_target(self, flags):
        """Make the states with flags[i] != 0 (n entries, caller's state order) absorbing for the block path: every block
        call then works on Q = D A D, D = diag(1 - flags) - first-passage problems without touching the generator, also
        on matrix-free boxes.  None (or an empty array) clears the set.  Setting or clearing discards the resident block
        and its J; the set lives until it is cleared or the generator changes.  Not under a row partition.
        (kfsp_set_block under option "block_target" = 1: the flags travel as one column of doubles.)"""
        if flags is None or np.size(flags) == 0:
            self._target_mode(1, lambda: self._chk(self._lib.kfsp_set_block(self._h, 1, 0, 1, None), "kfsp_set_block (block_target = 1)"))
        else:
            f = np.ascontiguousarray(np.asarray(flags).reshape(-1) != 0, dtype=np.float64)
            self._target_mode(1, lambda: self._chk(self._lib.kfsp_set_block(self._h, 1, f.size, max(f.size, 1), _p(f)),
                                                   "kfsp_set_block (block_target = 1)"))

    def block_target_info(self):
        """whether a target set is resident, its number of states, launches of the last block_hit (kfsp_block_info under
        option "block_target" = 2)"""
        v = np.zeros(8, dtype=np.int64)
        self._target_mode(2, lambda: self._chk(self._lib.kfsp_block_info(self._h, _p(v)), "kfsp_block_info (block_target = 2)"))
        return {"resident": int(v[0]), "states": int(v[1]), "hit_launches": int(v[2])}

    def block_hit(self, integral=False):
        """The flux into the target set, per column -> hit[k]: sum over the set of (A X)_i with the unmasked A.  X = W
        (default): the first-passage density at the solve's current time.  integral=True: X = J (set_option("block_integral",
        1) before set_block): the probability of having reached the set by the accumulated time; 1 - wsum = hit + leak
        out of the FSP.  Forward only (-12 under option "adjoint").  (kfsp_block_begin under option "block_target" = 3.)"""
        k = self._block_k()
        out = np.zeros(BLOCK_K_MAX, dtype=np.float64)
        self._target_mode(3, lambda: self._chk(self._lib.kfsp_block_begin(self._h, 1 if integral else 0, _p(out)),
                                               "kfsp_block_begin (block_target = 3)"))
        return out[:k].copy()

    def spmm_bench(self, reps):
        """ms for reps block products on the resident block"""
        ms = C.c_float(0.0)
        self._chk(self._lib.kfsp_spmm_bench(self._h, int(reps), C.byref(ms)), "kfsp_spmm_bench")
        return ms.value

    def set_option(self, name, value):
        """kfsp_set_option (include/kfsp.h lists the names), e.g. "block_box" = 1: the block calls take a matrix-free single-factor box;
        2: every matrix-free box (0 and 1 keep their meaning: a multi-factor box is still refused under 1).
        "block_dia_code" = 1 (default 0, read at every block call): the forward block product reads the dictionary-coded image
        of a banded generator where the single-vector product does (option "dia_code"); every other case keeps its kernel.
        "block_dia_code_adjoint" = 1 (default 0, read at every block call, only with "block_dia_code" = 1): under "adjoint" the
        transposed block product of such a generator reads the coded image too - the same bits as the plain transposed
        product; at 0 backward calls keep the plain kernel.
        "dia_code_diag" (-1, default: generators that pass "dia_code"'s size gate; 0 never; 1 always try; read when the generator
        is set): DIAG of a coded banded generator is folded into bits 48-63 of its 8-byte records - the product reads no DIAG
        stream and computes the same bits (dia_code_info()["diag_table_bytes"] > 0 says that it was taken).
        "dia_code_lanes" (0, default / 1; read at every launch): 1, the folded product takes the pairs of x of its +-1 diagonals
        from the neighbour lanes' registers instead of loading them (dia_code_info()["neighbours"]); the same bits, and on
        the benchmark's generator slower than the loads.
        "dia_code_inner" (1, default / 0; read at every launch): 1, the folded product of a generator with 6 diagonals on three
        strides or 4 on two runs every 128-row group the ends of x cannot touch through a body without per-lane 64-bit index
        arithmetic (dia_code_info()["inner"]); the same bits; "dia_code_lanes" = 1 takes precedence."""
        self._chk(self._lib.kfsp_set_option(self._h, name.encode(), int(value)), "kfsp_set_option")
        if not hasattr(self, "_options"):
            self._options = {}
        self._options[name] = int(value)
