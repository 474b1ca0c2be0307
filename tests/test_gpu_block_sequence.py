"""The block path across generator changes (csrc/kfsp_block_host.hip): ONE context takes every form the block product has a
kernel family for in turn, forwards and then backwards, and after each step it must be indistinguishable from a fresh
context that was given only that step - A X and A^T X at two widths bit for bit, one short block solve (the block, its
column sums, the step statistics), and kfsp_block_info after every call.  Whatever the block state keeps of its
predecessor - a width, an occupancy, an info slot, a target set - shows here.  A call that is refused must be refused with
the same text.  The row partition is left out: it needs ranks (tests/test_gpu_block_partition.py)."""
import numpy as np
import pytest

from tests import box_cases as BC
from tests.row_cases import ell_case

pytestmark = pytest.mark.gpu

# what a step may change, and the defaults every step starts from
DEFAULTS = {"host_build": 0, "sell_code": -1, "box_store": 0, "dia_code": -1, "dia_code_diag": -1, "block_dia_code": 0,
            "block_dia_code_adjoint": 0, "block_box": 0, "block_small": 0}
KS = (3, 16)
BOX_FORMATS = (4, 6, 7, 8)                            # what a single-factor matrix-free box reports


def _steps():
    """(name, options, n, put, layout formats, dia_code active, every how-manieth state is a target or 0)"""
    from krylovfspssa_amd import synth
    band = synth.toggle(30, 20)                       # 600 states x 4 reactions: every slot one constant shift
    band_ell = band.ell()
    masked = synth.toggle(12, 11)                     # 132 rows: 4 of them in a second group, so the stored form is masked
    rnd = ell_case("duplicated links 600x8")
    loc = ell_case("local 1500x8")
    box = synth.toggle(16, 8)                         # one 128-row group: stored it is unmasked and can be coded
    three = BC.model("three_factor")
    put_band = lambda c: c.set_matrix_ell(*band_ell)
    return [
        ("a banded", {}, band.n, put_band, (1,), 0, 0),
        ("b stored box, masked", {"box_store": 1}, masked.n, lambda c: c.set_matrix_box(masked), (2,), 0, 0),
        ("c SELL", {}, rnd["n"], lambda c: c.set_matrix_ell(rnd["adj"], rnd["off"], rnd["diag"]), (0,), 0, 0),
        ("d SELL, coded columns", {"sell_code": 1}, loc["n"], lambda c: c.set_matrix_ell(loc["adj"], loc["off"], loc["diag"]), (5,), 0, 0),
        ("e stored box, coded", {"box_store": 1, "dia_code": 1, "dia_code_diag": 1, "block_dia_code": 1}, box.n,
         lambda c: c.set_matrix_box(box), (1,), 1, 0),
        ("f matrix-free box", {"block_box": 1}, box.n, lambda c: c.set_matrix_box(box), BOX_FORMATS, 0, 0),
        ("g matrix-free box, three factors", {"block_box": 2}, three.n, lambda c: c.set_matrix_box(three), (3,), 0, 0),
        ("h banded, small pass", {"block_small": 1}, band.n, put_band, (1,), 0, 0),
        ("i banded, target set", {}, band.n, put_band, (1,), 0, 7),
    ]


def _apply(c, step):
    _, opts, n, put, _, _, every = step
    for k, v in {**DEFAULTS, **opts}.items():
        c.set_option(k, v)
    put(c)
    if every:
        c.set_block_target(np.arange(n) % every == 0)


def _call(f):
    """what a call gave: its value, or the text of its refusal"""
    from krylovfspssa_amd.host import KfspError
    try:
        return f()
    except KfspError as e:
        return "refused: " + str(e)


def _seen(c, X, W, t):
    """every observable of the block path on this context, in a fixed order of calls"""
    out = {"layout": c.layout_info(), "dia_code_active": c.dia_code_info()["active"], "target": c.block_target_info()}
    for k in KS:
        out[f"AX k={k}"] = _call(lambda: c.spmm(X[:, :k]))
        out[f"AX k={k} info"] = c.block_info()
        for coded_t in (0, 1):                        # (read only beside block_dia_code = 1: step e)
            c.set_option("block_dia_code_adjoint", coded_t)
            out[f"ATX k={k} coded_t={coded_t}"] = _call(lambda: c.spmm(X[:, :k], adjoint=True))
            out[f"ATX k={k} coded_t={coded_t} info"] = c.block_info()
        c.set_option("block_dia_code_adjoint", 0)
    out["set_block"] = _call(lambda: c.set_block(W))
    solved = _call(lambda: c.expv_block(t, 1e-8, m=10))
    if isinstance(solved, str):
        out["wsum"] = solved
    else:
        st = solved[1]
        out["wsum"] = solved[0]
        out["stats"] = [getattr(st, name) for name, _ in st._fields_]
    out["W"] = _call(lambda: c.get_block())
    out["solve info"] = c.block_info()
    return out


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and np.array_equal(a, b)
    return a == b


def test_every_block_kernel_family_in_turn_leaves_nothing_behind():
    from krylovfspssa_amd import KfspContext
    steps = _steps()
    rng = np.random.default_rng(47)
    fresh = []
    for step in steps:                                # the references: one fresh context each, made once
        name, opts, n, _, formats, coded, every = step
        X = rng.standard_normal((n, max(KS)))
        W = rng.random((n, 3))
        W /= W.sum(axis=0)
        with KfspContext(0) as f:
            _apply(f, step)
            # a handful of steps: t is a few times 1 / max |a_ii| (the diagonal through the single-vector product)
            diag = np.array([f.spmv(np.eye(1, n, i).ravel())[i] for i in range(0, n, max(1, n // 40))])
            t = 3.0 / np.abs(diag).max()
            want = _seen(f, X, W, t)
            cols = [f.spmv(np.ascontiguousarray(X[:, j])) for j in range(max(KS))]
        # the step ran the form it is here for, not another one that happens to agree
        assert want["layout"]["format"] in formats, (name, want["layout"])
        assert want["dia_code_active"] == coded, (name, want["dia_code_active"])
        assert want["target"]["resident"] == (1 if every else 0) and want["target"]["states"] == (len(range(0, n, every)) if every else 0)
        for k in KS:
            for key in (f"AX k={k}", f"ATX k={k} coded_t=0", f"ATX k={k} coded_t=1"):
                assert isinstance(want[key], np.ndarray) and np.abs(want[key]).max() > 0.0, (name, key, want[key])
            assert want[f"AX k={k} info"]["adjoint"] == 0 and want[f"ATX k={k} coded_t=0 info"]["adjoint"] == 1, name
            if not every:                             # (under a target set the product is D A D X)
                for j in range(k):
                    assert np.array_equal(want[f"AX k={k}"][:, j], cols[j]), (name, k, j)
            # the coded kernels: forward under block_dia_code, transposed only with block_dia_code_adjoint beside it
            assert want[f"AX k={k} info"]["fmt"] == (9 if coded else 0), (name, want[f"AX k={k} info"])
            assert want[f"ATX k={k} coded_t=0 info"]["fmt"] == 0, (name, want[f"ATX k={k} coded_t=0 info"])
            assert want[f"ATX k={k} coded_t=1 info"]["fmt"] == (9 if coded else 0), (name, want[f"ATX k={k} coded_t=1 info"])
            assert np.array_equal(want[f"ATX k={k} coded_t=0"], want[f"ATX k={k} coded_t=1"]), (name, k)
        assert isinstance(want["W"], np.ndarray) and want["stats"][0] >= 1, (name, want["W"], want["wsum"])
        assert want["solve info"]["one_launch"] == (1 if opts.get("block_small") else 0), (name, want["solve info"])
        fresh.append((X, W, t, want))
    order = list(range(len(steps))) + list(range(len(steps) - 2, -1, -1))
    with KfspContext(0) as c:
        for pos, i in enumerate(order):
            _apply(c, steps[i])
            X, W, t, want = fresh[i]
            got = _seen(c, X, W, t)
            where = (pos, steps[i][0], "after " + (steps[order[pos - 1]][0] if pos else "nothing"))
            assert set(got) == set(want), where
            for key in want:
                assert _same(got[key], want[key]), (where, key, got[key], want[key])
