"""Several vectors at once under a row partition (option block_partition = 1): loop-back ranks of one process (each a
context with a communicator, driven by its own thread) and a group head against ONE context on the same generator.
Products are the same bits (rows are independent and each is summed in FMATVEC's order), every scalar is the same bits on
every rank, a pass and a whole solve meet the one-context pass and the restatement tests/block_ref.py, and nothing of the
single-vector path moves.  Every test sets block_partition = 1 first.  Needs a real MI355X."""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import block_generators
from tests import block_ref as BR
from tests.test_gpu_block_reference import _assert_solve_matches_ref, _start

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _synth():
    from krylovfspssa_amd import synth
    return synth


def _host():
    from krylovfspssa_amd import host
    return host


# ---- the cases: generator, ranks, options, the kernel formats its ranks may end up in (kfsp_layout_info v[0]), the
# exchange kfsp_layout_info reports and the one kfsp_block_info v[7] must report after a pass (1 strips, 2 all-gather,
# + 4 split into interior and boundary launches)
CASES = {
    # blocks 64, 64, 2, 0: a two-row rank and an empty one
    "toggle13x10 P4": dict(model=(13, 10), P=4, opts={}, fmt=(1, 2), lay=1, blk=1),
    # ragged last 128-row group on both ranks (704 = 5.5 groups, 616 = 4.8)
    "toggle40x33 P2": dict(model=(40, 33), P=2, opts={}, fmt=(1, 2), lay=1, blk=1),
    # L = 448, an odd multiple of 64: the padded half-group spills into the column's margin
    "toggle40x33 P3": dict(model=(40, 33), P=3, opts={}, fmt=(1, 2), lay=1, blk=1),
    "toggle40x33 P3 sell": dict(model=(40, 33), P=3, opts={"format": 1, "sell_code": 0}, fmt=(0,), lay=1, blk=1),
    "toggle40x33 P2 allgather": dict(model=(40, 33), P=2, opts={"halo": 0}, fmt=(1, 2), lay=2, blk=2),
    "toggle40x33 P3 p2p": dict(model=(40, 33), P=3, opts={"halo_p2p": 1}, fmt=(1, 2), lay=1, blk=1),
    "toggle60x50 P2 coded": dict(model=(60, 50), P=2, opts={"format": 1, "sell_code": 1}, fmt=(5,), lay=1, blk=1),
    # masked banded (the ranks whose rows lack a +-1000 diagonal on >= 3 % of their 128-row groups; a rank in the middle
    # has none empty and stays plain banded), L = 1024: the strips (1000 rows) are almost a whole block
    "toggle1000x3 P3": dict(model=(1000, 3), P=3, opts={}, fmt=(1, 2), need=2, lay=1, blk=1),
    # L = 768 < reach 1000: every rank must fall back to the all-gather
    "toggle1000x3 P4": dict(model=(1000, 3), P=4, opts={}, fmt=(1, 2), need=2, lay=2, blk=2),
    # 247 / 165 banded trips per rank under overlap = 2: interior beside the exchange, one boundary launch
    "toggle300x211 P2 split": dict(model=(300, 211), P=2, opts={"overlap": 2}, fmt=(1, 2), lay=1, blk=5),
    "toggle300x211 P3 split p2p": dict(model=(300, 211), P=3, opts={"overlap": 2, "halo_p2p": 1}, fmt=(1, 2), lay=1, blk=5),
}

_MODELS = {}


def _model(dims):
    if dims not in _MODELS:
        mdl = _synth().toggle(*dims)
        _MODELS[dims] = (mdl, mdl.csr_rows())
    return _MODELS[dims]


def _rows(csr, r0, nr):
    rp, col, val = csr
    return rp[r0:r0 + nr + 1] - rp[r0], col[rp[r0]:rp[r0 + nr]], val[rp[r0]:rp[r0 + nr]]


def _set_csr(ctx, n, csr, opts):
    """block_partition first, the case's options, this context's rows of the generator (a head and one context: all)"""
    ctx.set_option("block_partition", 1)
    for key, v in opts.items():
        ctx.set_option(key, v)
    r0, nr = ctx.row_block(n)
    ctx.set_matrix_csr(n, *_rows(csr, r0, nr))
    return r0, nr


def _mixed(n, rng):
    """16 columns of mixed signs, one of them a unit vector"""
    X = rng.standard_normal((n, 16))
    X[:, 2] = 0.0
    X[(3 * n) // 7, 2] = 1.0
    return X


def _one_context(n, csr, opts, body):
    from krylovfspssa_amd import KfspContext
    with KfspContext(0) as ctx:
        _set_csr(ctx, n, csr, opts)
        return body(ctx, 0, n)


def _head(P, n, csr, opts, body):
    from krylovfspssa_amd import KfspContext
    with KfspContext(0, group=P) as ctx:
        _set_csr(ctx, n, csr, opts)
        return body(ctx, 0, n)


def _ranks(P, n, csr, opts, body):
    def work(ctx, rank):
        r0, nr = _set_csr(ctx, n, csr, opts)
        return body(ctx, r0, nr)
    return _host().run_loopback_ranks(P, work)


# ---- 1. products on the bits
def _products(X):
    def body(ctx, r0, nr):
        out = dict(r0=r0, nr=nr, lay=ctx.layout_info())
        out["spmm"] = {k: ctx.spmm(X[:, :k]) for k in KS}
        out["spmv"] = [ctx.spmv(X[:, j]) for j in range(16)]
        ctx.set_block(X[r0:r0 + nr, :3])
        out["back"] = ctx.get_block()
        ctx.block_begin(4)
        ctx.block_arnoldi(2)
        out["binfo"] = ctx.block_info()
        ctx.spmm(X[:, :3])                         # its X is whole on every rank: no exchange
        out["binfo_spmm"] = ctx.block_info()
        assert ctx.spmm_bench(2) > 0.0             # the resident block as source: exchanged before every product
        out["binfo_bench"] = ctx.block_info()
        return out
    return body


@pytest.mark.parametrize("case", list(CASES))
def test_products_on_the_bits(case):
    c = CASES[case]
    mdl, csr = _model(c["model"])
    n, P = mdl.n, c["P"]
    X = _mixed(n, np.random.default_rng(17))
    one = _one_context(n, csr, c["opts"], _products(X))
    res = _ranks(P, n, csr, c["opts"], _products(X))
    head = _head(P, n, csr, c["opts"], _products(X))
    L = _host().partition(n, P, 0)[2]
    assert [r["nr"] for r in res] == [max(0, min(L, n - p * L)) for p in range(P)]
    for r in res:
        if r["nr"] > 0:
            assert r["lay"]["format"] in c["fmt"], r["lay"]
        assert r["lay"]["exchange"] == c["lay"], r["lay"]
        assert r["binfo"]["exchange"] == c["blk"], r["binfo"]
        assert r["binfo_spmm"]["exchange"] == 0 and r["binfo_bench"]["exchange"] == c["blk"]
        assert np.array_equal(_bits(r["back"]), _bits(X[r["r0"]:r["r0"] + r["nr"], :3]))
        for k in KS:
            assert r["spmm"][k].shape == (r["nr"], k)
            for j in range(k):
                assert np.array_equal(_bits(r["spmm"][k][:, j]), _bits(r["spmv"][j])), (case, k, j)
    if "need" in c:
        assert c["need"] in [r["lay"]["format"] for r in res]
    assert head["binfo"]["exchange"] == c["blk"] and head["lay"]["exchange"] == c["lay"]
    assert head["binfo_bench"]["exchange"] == c["blk"] and one["binfo"]["exchange"] == 0 and one["binfo_bench"]["exchange"] == 0
    assert np.array_equal(_bits(head["back"]), _bits(X[:, :3]))
    for k in KS:
        Y = np.concatenate([r["spmm"][k] for r in res], axis=0)
        assert np.array_equal(_bits(Y), _bits(one["spmm"][k])), (case, k)
        assert np.array_equal(_bits(head["spmm"][k]), _bits(one["spmm"][k])), (case, k)


def _golden_fsp(golden_dir):
    a = np.load(os.path.join(golden_dir, "assembly_toggle_k20.npz"))
    return a["adj"], a["offdiag"], a["diag"], a["state"]


@pytest.mark.parametrize("state_order", [0, 1])
def test_products_on_the_bits_reference_layout(golden_dir, state_order):
    """the golden toggle FSP through kfsp_set_matrix_ell (whole arrays on every rank), in discovery order and under the
    global internal state order, where the columns go through upload_states / download_states (one all-gather each)"""
    from krylovfspssa_amd import KfspContext
    adj, off, diag, state = _golden_fsp(golden_dir)
    n = adj.shape[0]
    X = _mixed(n, np.random.default_rng(19))

    def run(ctx, rank=0):
        ctx.set_option("block_partition", 1)
        for key, v in (("state_order", state_order), ("state_order_min", 1), ("state_order_products", 0)):
            ctx.set_option(key, v)
        ctx.set_state_coords(state)
        ctx.set_matrix_ell(adj, off, diag)
        assert ctx.state_order_active() == bool(state_order)
        r0, nr = ctx.row0, ctx.nloc
        out = dict(r0=r0, nr=nr, lay=ctx.layout_info(), spmm={k: ctx.spmm(X[:, :k]) for k in (3, 16)},
                   spmv=[ctx.spmv(X[:, j]) for j in range(16)])
        ctx.set_block(X[r0:r0 + nr, :5])
        out["back"] = ctx.get_block()
        ctx.block_begin(4)
        ctx.block_arnoldi(2)
        out["binfo"] = ctx.block_info()
        return out

    with KfspContext(0) as ctx:
        one = run(ctx)
    res = _host().run_loopback_ranks(2, run)
    with KfspContext(0, group=2) as ctx:
        head = run(ctx)
    for r in res + [head]:
        assert r["lay"]["state_order"] == state_order
        assert r["binfo"]["exchange"] == r["lay"]["exchange"] and r["lay"]["exchange"] in (1, 2)
        assert np.array_equal(_bits(r["back"]), _bits(X[r["r0"]:r["r0"] + r["nr"], :5]))
        for k in (3, 16):
            for j in range(k):
                assert np.array_equal(_bits(r["spmm"][k][:, j]), _bits(r["spmv"][j])), (k, j)
    for k in (3, 16):
        assert np.array_equal(_bits(np.concatenate([r["spmm"][k] for r in res], axis=0)), _bits(one["spmm"][k]))
        assert np.array_equal(_bits(head["spmm"][k]), _bits(one["spmm"][k]))


# ---- 2. + 3. scalars agree; one pass against one context
def _absorbing(csr, n, s):
    """the same gather rows with state s made absorbing: column s of A is 0 (its outflow entries and its diagonal)"""
    rp, col, val = csr
    rows = np.repeat(np.arange(n), np.diff(rp))
    val = val.copy()
    val[(col == s) & (rows == s)] = 0.0
    keep = ~((col == s) & (rows != s))
    rp2 = np.concatenate(([0], np.cumsum(np.bincount(rows[keep], minlength=n)))).astype(np.int64)
    return rp2, col[keep], val[keep]


def _pass(W, m):
    def body(ctx, r0, nr):
        ctx.set_block(W[r0:r0 + nr])
        beta = ctx.block_begin(m)
        hb, nrm, brk, avn = ctx.block_arnoldi(m)
        return dict(beta=beta, hb=hb, nrm=nrm, brk=brk, avn=avn, binfo=ctx.block_info())
    return body


PASS_CASES = {"toggle40x33 P3": ((40, 33), 3, {}), "toggle40x33 P2 sell": ((40, 33), 2, {"format": 1, "sell_code": 0}),
              "toggle13x10 P4": ((13, 10), 4, {}), "toggle300x211 P2 split": ((300, 211), 2, {"overlap": 2}),
              "toggle1000x3 P4 allgather": ((1000, 3), 4, {})}


@pytest.mark.parametrize("case", list(PASS_CASES))
def test_one_pass_against_one_context(case):
    """block_begin + block_arnoldi(12) over P ranks and through a head against one context, with the tolerances of
    tests/test_gpu_group.py::test_head_of_a_partition_behaves_like_one_context per column; a zero column (brk -1) and
    the unit vector of an absorbing state (brk 1) ride along and change nobody's sequence of collectives"""
    dims, P, opts = PASS_CASES[case]
    mdl, csr0 = _model(dims)
    n, m = mdl.n, 12
    s = (5 * n) // 11
    csr = _absorbing(csr0, n, s)
    W = np.zeros((n, 7))
    W[:, :5] = _start(n, 5, np.random.default_rng(23))
    W[s, 6] = 1.0
    one = _one_context(n, csr, opts, _pass(W, m))
    res = _ranks(P, n, csr, opts, _pass(W, m))
    head = _head(P, n, csr, opts, _pass(W, m))
    assert list(one["brk"]) == [0, 0, 0, 0, 0, -1, 1]
    for r in res[1:]:                              # every scalar: the same bits on every rank
        for key in ("beta", "hb", "nrm", "avn"):
            assert np.array_equal(_bits(r[key]), _bits(res[0][key])), key
        assert np.array_equal(r["brk"], res[0]["brk"])
    for key in ("beta", "hb", "nrm", "avn"):       # ... and a head returns them
        assert np.array_equal(_bits(head[key]), _bits(res[0][key])), key
    assert np.array_equal(head["brk"], res[0]["brk"])
    b = res[0]
    assert np.array_equal(b["brk"], one["brk"])
    for c in range(7):
        scale = np.abs(one["hb"][:, :, c]).max()
        print(case, "column", c, "beta", abs(b["beta"][c] - one["beta"][c]), "avnorm", abs(b["avn"][c] - one["avn"][c]),
              "hb", np.abs(b["hb"][:9, :, c] - one["hb"][:9, :, c]).max(), "nrm", np.abs(b["nrm"][:10, c] - one["nrm"][:10, c]).max(),
              "scale", scale)
        assert abs(b["beta"][c] - one["beta"][c]) <= 1e-13 * abs(one["beta"][c])
        assert abs(b["avn"][c] - one["avn"][c]) <= 1e-13 * abs(one["avn"][c])
        assert np.abs(b["hb"][:9, :, c] - one["hb"][:9, :, c]).max() <= 1e-11 * scale
        assert np.abs(b["nrm"][:10, c] - one["nrm"][:10, c]).max() <= 1e-11 * scale
    assert np.all(b["hb"][:, :, 5] == 0.0) and b["beta"][5] == 0.0 and b["avn"][5] == 0.0
    assert b["beta"][6] == 1.0 and np.all(b["hb"][1:, :, 6] == 0.0)


def test_a_failing_rank_in_a_block_call_is_reported_and_does_not_hang():
    """rank 1 of a 3-rank head fails (injected) at the start of kfsp_block_begin while ranks 0 and 2 enter its all-reduce:
    the head's watchdog releases them after the grace period and names rank 1"""
    import time
    from krylovfspssa_amd import KfspContext, KfspError
    mdl, csr = _model((40, 33))
    c = KfspContext(0, group=3)
    try:
        c.set_option("group_grace_ms", 500)
        _set_csr(c, mdl.n, csr, {})
        c.set_block(np.ones((mdl.n, 3)) / mdl.n)
        assert c.block_begin(12)[0] == pytest.approx(1.0 / math.sqrt(mdl.n), rel=1e-13)     # a healthy call first
        c.set_option("group_inject_failure", 1)
        t0 = time.time()
        with pytest.raises(KfspError, match=r"-77.*rank 1: injected failure"):
            c.block_begin(12)
        assert time.time() - t0 < 20.0
    finally:
        c.close()


# ---- 4. an exact check that does not go through the reductions
@pytest.mark.parametrize("case", ["toggle40x33 P3", "toggle13x10 P4", "toggle300x211 P2 split"])
def test_begin_then_combine_is_exact(case):
    """u_1 = W copied, W <- max(coef u_1, 0): one rounding per element whoever owns the row"""
    c = CASES[case]
    mdl, csr = _model(c["model"])
    n, P, k = mdl.n, c["P"], 5
    rng = np.random.default_rng(29)
    W = rng.standard_normal((n, k))
    coef = np.array([[1.5, -0.75, 1.0 / 3.0, 2.0, -1.0]])

    def body(ctx, r0, nr):
        ctx.set_block(W[r0:r0 + nr])
        ctx.block_begin(6)
        ws = ctx.block_combine(1, coef)
        return dict(ws=ws, W=ctx.get_block())

    one = _one_context(n, csr, c["opts"], body)
    res = _ranks(P, n, csr, c["opts"], body)
    head = _head(P, n, csr, c["opts"], body)
    want = np.maximum(coef * W, 0.0)
    assert np.array_equal(_bits(one["W"]), _bits(want + 0.0))
    assert np.array_equal(_bits(np.concatenate([r["W"] for r in res], axis=0)), _bits(one["W"]))
    assert np.array_equal(_bits(head["W"]), _bits(one["W"]))
    for r in res[1:] + [head]:
        assert np.array_equal(_bits(r["ws"]), _bits(res[0]["ws"]))
    for j in range(k):
        exact = math.fsum(want[:, j])
        for ws in (res[0]["ws"], one["ws"]):
            assert abs(ws[j] - exact) <= (n + 4) * 2.0 ** -53 * exact, (j, ws[j], exact)


# ---- 5. whole solves against the restatement
def _solve_generator(ctx, golden_dir, kind):
    """the five generators of tests/block_generators.py; a rank takes its rows of the two box generators"""
    ctx.set_option("block_partition", 1)
    if kind in ("banded", "masked_banded") and ctx.nranks > 1:
        mdl, csr = _model((60, 50) if kind == "banded" else (1000, 3))
        ctx.set_option("format", 0)
        if kind == "banded":
            ctx.set_option("dia_mask", 0)
        r0, nr = ctx.row_block(mdl.n)
        ctx.set_matrix_csr(mdl.n, *_rows(csr, r0, nr))
        return mdl.ell()
    return block_generators.GENERATORS[kind](ctx, golden_dir)[1]


_REF = {}


def _solve_reference(kind, ell, t, tol, m):
    if kind not in _REF:
        n = ell[0].shape[0]
        W = _start(n, 5, np.random.default_rng(31))
        _REF[kind] = (W,) + tuple(BR.expv_block(O.EllMatrix(*ell), W, t, tol, m))
    return _REF[kind]


@pytest.mark.parametrize("how", ["P2", "P3", "head2"])
@pytest.mark.parametrize("kind", list(block_generators.GENERATORS))
def test_solves_match_the_restatement(golden_dir, kind, how):
    from krylovfspssa_amd import KfspContext
    t, tol, m = 0.05, 1e-10, 30
    box = {}

    def run(ctx, rank=0):
        ell = _solve_generator(ctx, golden_dir, kind)
        if rank == 0:
            box["ell"] = ell
        n = ell[0].shape[0]
        W = _start(n, 5, np.random.default_rng(31))
        r0, nr = ctx.row0, ctx.nloc
        ctx.set_block(W[r0:r0 + nr])
        ws, st = ctx.expv_block(t, tol, m)
        return dict(R=ctx.get_block(), ws=ws, st=st)

    if how == "head2":
        with KfspContext(0, group=2) as ctx:
            res = [run(ctx)]
    else:
        res = _host().run_loopback_ranks(int(how[1:]), run)
    W, Rref, wsref, stref = _solve_reference(kind, box["ell"], t, tol, m)
    for r in res[1:]:
        assert np.array_equal(_bits(r["ws"]), _bits(res[0]["ws"]))
        assert bytes(r["st"]) == bytes(res[0]["st"])
    R = np.concatenate([r["R"] for r in res], axis=0)
    _assert_solve_matches_ref(R, res[0]["ws"], res[0]["st"], Rref, wsref, stref, W)


def test_wide_solve_with_split_launches():
    """k = 16 on toggle(300, 211) over 2 ranks with overlap = 2 against the restatement"""
    t, tol, m = 0.05, 1e-10, 30
    mdl, csr = _model((300, 211))
    n = mdl.n
    W = _start(n, 16, np.random.default_rng(37))

    def body(ctx, r0, nr):
        ctx.set_block(W[r0:r0 + nr])
        ws, st = ctx.expv_block(t, tol, m)
        return dict(R=ctx.get_block(), ws=ws, st=st, binfo=ctx.block_info())

    res = _ranks(2, n, csr, {"overlap": 2}, body)
    assert all(r["binfo"]["exchange"] == 5 for r in res)
    assert np.array_equal(_bits(res[1]["ws"]), _bits(res[0]["ws"]))
    Rref, wsref, stref = BR.expv_block(O.EllMatrix(*mdl.ell()), W, t, tol, m)
    _assert_solve_matches_ref(np.concatenate([r["R"] for r in res], axis=0), res[0]["ws"], res[0]["st"], Rref, wsref, stref, W)


# ---- 6. nothing else moved
@pytest.mark.parametrize("case", ["toggle40x33 P3", "toggle40x33 P2 allgather"])
def test_the_single_vector_path_is_left_alone(case):
    """w, its product and an Arnoldi pass from it: the same bits before and after a block solve on the same rank context
    (the block path shares d_xg and the staging buffers with them)"""
    c = CASES[case]
    mdl, csr = _model(c["model"])
    n = mdl.n
    p0 = _synth().poisson_p0(mdl, 6.0)
    W = _start(n, 5, np.random.default_rng(41))

    def single(ctx):
        w = ctx.get_vector()
        y = ctx.spmv_w()
        beta = ctx.begin_step()
        H, mb, k1, av = ctx.arnoldi(12)
        return [w, y, np.array([beta, mb, k1, av]), H.copy()]

    def body(ctx, r0, nr):
        ctx.set_option("small_kernel", 0)
        ctx.set_vector(p0[r0:r0 + nr])
        before = single(ctx)
        ctx.set_block(W[r0:r0 + nr])
        ctx.expv_block(0.02, 1e-8, 20)
        ctx.spmm(W)
        return before, single(ctx)

    for before, after in _ranks(c["P"], n, csr, c["opts"], body):
        for a, b in zip(before, after):
            assert np.array_equal(_bits(a), _bits(b))


def test_refusals_and_lifetime():
    from krylovfspssa_amd.host import KfspError
    mdl, csr = _model((60, 50))
    n = mdl.n
    W = np.ones((n, 2))

    def raw_spmm(ctx):
        Y = np.empty_like(W)
        rc = ctx._lib.kfsp_spmm(ctx._h, 2, n, W.ctypes.data_as(ctypes.c_void_p), Y.ctypes.data_as(ctypes.c_void_p))
        return rc, ctx._lib.kfsp_last_error(ctx._h).decode()

    def body(ctx, r0, nr):
        out = {}
        ctx.set_option("block_partition", 1)           # accepted at all (the parent commit: -2, unknown option) ...
        ctx.set_option("block_partition", 0)           # ... and 0 is the refusal every caller has seen so far
        ctx.set_matrix_csr(n, *_rows(csr, r0, nr))
        out["off"] = raw_spmm(ctx)
        ctx.set_option("block_partition", 1)
        ctx.set_option("adjoint", 1)                   # refused on every rank before any collective
        out["adjoint"] = raw_spmm(ctx)
        ctx.set_option("adjoint", 0)
        ctx.set_matrix_box(mdl, store=False)
        out["box"] = raw_spmm(ctx)
        ctx.set_option("block_box", 1)
        out["block_box"] = raw_spmm(ctx)
        ctx.set_matrix_csr(n, *_rows(csr, r0, nr))
        ctx.set_block(W[r0:r0 + nr])
        ctx.get_block()
        ctx.set_matrix_csr(n, *_rows(csr, r0, nr))     # a new generator discards the block
        try:
            ctx.get_block()
            out["kept"] = True
        except KfspError as e:
            out["kept"] = str(e)
        return out

    def work(ctx, rank):
        r0, nr = ctx.row_block(n)
        return body(ctx, r0, nr)

    for r in _host().run_loopback_ranks(2, work):
        assert r["off"][0] == -12 and "row partition" in r["off"][1]
        assert r["adjoint"][0] == -12 and "adjoint" in r["adjoint"][1]
        assert r["box"][0] == -12 and "matrix-free" in r["box"][1]
        assert r["block_box"][0] == -12 and "matrix-free" in r["block_box"][1]
        assert r["kept"] is not True and "-> -1" in r["kept"]
