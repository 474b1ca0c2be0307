"""Replacing the resident generator (csrc/kfsp_generator.cpp): ONE context takes every generator form in turn, forwards and
then backwards, and after each step it must be indistinguishable from a fresh context that was given only that
generator - the product bit for bit, and every info call (kfsp_dia_code_info apart from v[5], a time).  Whatever a path
forgot to clear of its predecessor's form shows here.  Then one expansion and one drop of a small resident FSP, with and
without the speculative rebuild and the internal state order, against the two host calls and a fresh upload
(tests/test_gpu_expand.py's own comparison)."""
import numpy as np
import pytest

from tests.expand_helpers import grown as _grown, mass_action as _mass_action
from tests.row_cases import ell_case
from tests.test_gpu_expand import _host_composition

pytestmark = pytest.mark.gpu

# what a step may change, and the defaults every step starts from
DEFAULTS = {"host_build": 0, "sell_code": -1, "box_store": 0, "dia_code": -1, "dia_code_diag": -1}


def _steps():
    from krylovfspssa_amd import synth
    band = synth.toggle(30, 20)                      # 600 states x 4 reactions: every slot one constant shift
    band_ell = band.ell()
    rnd = ell_case("duplicated links 600x8")         # random links: no slot is a constant shift
    loc = ell_case("local 1500x8")                   # near neighbours from few shifts: its chunks' columns can be coded
    small = synth.toggle(25, 20)                     # 500 rows as CSR (banded: the host build stores diagonals)
    rowptr, col, val = small.csr_rows()
    box = synth.toggle(16, 8)                        # one 128-row group: no (diagonal, group) segment is empty, so the stored
                                                     # form is unmasked and can be coded (12 x 11 leaves 4 rows in a second group)
    return [
        ("banded ELL, device build", {}, band.n, lambda c: c.set_matrix_ell(*band_ell), (1, 2)),
        ("random ELL, device build", {}, rnd["n"], lambda c: c.set_matrix_ell(rnd["adj"], rnd["off"], rnd["diag"]), (0,)),
        ("local ELL, coded columns", {"sell_code": 1}, loc["n"], lambda c: c.set_matrix_ell(loc["adj"], loc["off"], loc["diag"]), (5,)),
        ("CSR", {}, small.n, lambda c: c.set_matrix_csr(small.n, rowptr, col, val), (1, 2)),
        ("box", {}, box.n, lambda c: c.set_matrix_box(box), (3, 4, 6, 7, 8)),
        ("box stored and coded", {"box_store": 1, "dia_code": 1, "dia_code_diag": 1}, box.n, lambda c: c.set_matrix_box(box), (1,)),
        ("random ELL, host build", {"host_build": 1}, rnd["n"], lambda c: c.set_matrix_ell(rnd["adj"], rnd["off"], rnd["diag"]), (0,)),
    ]


def _apply(c, opts, put):
    for k, v in {**DEFAULTS, **opts}.items():
        c.set_option(k, v)
    put(c)


def _raw_dia_code_info(c):
    from krylovfspssa_amd.host import _p
    v = np.zeros(26, dtype=np.int64)
    assert c._lib.kfsp_dia_code_info(c._h, _p(v)) == 0
    v[5] = 0                                         # what the last build_dia_code took: a time
    return v.tolist()


def _seen(c, x):
    return dict(y=c.spmv(x), matrix_info=c.matrix_info(), bytes=c.matrix_bytes(), bytes_sell=c.matrix_bytes(True),
                layout=c.layout_info(), dia_code=_raw_dia_code_info(c), order=c.state_order_active())


def test_every_generator_form_in_turn_leaves_nothing_behind():
    from krylovfspssa_amd import KfspContext
    steps = _steps()
    rng = np.random.default_rng(41)
    fresh = []
    for name, opts, n, put, formats in steps:        # the references: one fresh context each, made once
        x = rng.standard_normal(n)
        with KfspContext(0) as f:
            _apply(f, opts, put)
            want = _seen(f, x)
        assert want["layout"]["format"] in formats, (name, want["layout"])
        fresh.append((x, want))
    assert fresh[5][1]["dia_code"][0] > 0 and fresh[5][1]["dia_code"][6] == 1      # the stored box IS coded, and read coded
    assert fresh[5][1]["dia_code"][7] > 0                                          # ... with DIAG folded in
    assert fresh[2][1]["layout"]["coded_chunks"] > 0
    order = list(range(len(steps))) + list(range(len(steps) - 2, -1, -1))
    with KfspContext(0) as c:
        for k, i in enumerate(order):
            name, opts, n, put, _ = steps[i]
            _apply(c, opts, put)
            x, want = fresh[i]
            got = _seen(c, x)
            where = (k, name, "after " + (steps[order[k - 1]][0] if k else "nothing"))
            assert np.array_equal(got.pop("y"), want["y"]), where
            for key in got:
                assert got[key] == want[key], (where, key, got[key], want[key])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("speculate", [0, 1])
def test_one_expansion_and_one_drop_of_a_resident_fsp(golden_dir, speculate, order):
    from krylovfspssa_amd import KfspContext
    rng = np.random.default_rng(43)
    with KfspContext(0) as c, KfspContext(0) as ref:
        nu, state, adj = _grown(c, "toggle_k20", golden_dir, 6)
        nr, ns = nu.shape
        params, progs = _mass_action(nu)
        for x in (c, ref):
            x.set_propensity_program(ns, params, progs)
            x.set_option("state_order", order)
            x.set_option("state_order_min", 64)
            x.set_option("state_order_products", 0)
        ref.set_option("build_speculate", 0)
        ref.set_option("ssa_regs", 0)
        c.set_option("build_speculate", speculate)
        off, diag = c.propensities(state)
        n = len(state)
        t = 2.0 / float(np.mean(diag[diag > 0]))
        seed = 2468
        nssa, state2, adj2, off2, diag2 = _host_composition(ref, t, seed, nu, state, adj, off, diag)
        c.set_option("keep_coords", 1)
        c.set_state_coords(state)
        c.set_matrix_ell(adj, off, diag)
        w = rng.random(n)
        c.set_vector(w)

        def same_as_a_fresh_upload(state, adj, off, diag):
            s_r, a_r, o_r, d_r = c.download_fsp(ns, nr)
            assert np.array_equal(s_r, state) and np.array_equal(a_r, adj) and np.array_equal(o_r, off) and np.array_equal(d_r, diag)
            assert c.state_order_active() == bool(order)
            ref.set_state_coords(state)
            ref.set_matrix_ell(adj, off, diag)
            x = rng.random(len(state))
            assert np.array_equal(c.spmv(x), ref.spmv(x))
            for call in ("matrix_info", "matrix_bytes", "layout_info"):
                assert getattr(c, call)() == getattr(ref, call)(), call
            assert _raw_dia_code_info(c) == _raw_dia_code_info(ref)

        # the expansion
        n2, got_ssa = c.expand_resident(t, seed, nu)
        assert (n2, got_ssa) == (len(state2), nssa) and n2 > n
        assert np.array_equal(c.get_vector(), np.concatenate([w, np.zeros(n2 - n)]))
        same_as_a_fresh_upload(state2, adj2, off2, diag2)
        # the drop: the later half of the list carries next to nothing
        w = rng.random(n2) * np.where(np.arange(n2) >= n2 // 2, 1e-14, 1.0)
        w /= w.sum()
        c.set_vector(w)
        _, _, nflag = c.drop_plan(1e-7)
        assert nflag > n2 // 20
        keep = c.drop_flags() == 0
        nk = c.drop_compact()
        c.drop_rebuild()
        assert nk == int(keep.sum()) == n2 - nflag
        newidx = np.cumsum(keep) * keep                 # the host's compaction of its copy (StateSpace.f90:500-546)
        adj3 = np.where(adj2 > 0, newidx[np.maximum(adj2, 1) - 1], adj2)[keep].astype(np.int32)
        assert np.array_equal(c.get_vector(), w[keep])
        same_as_a_fresh_upload(state2[keep], adj3, off2[keep], diag2[keep])
        info = c.build_info()
        assert info["speculative"] + info["repeated"] == (2 if speculate else 0), info
        assert ref.build_info()["speculative"] == 0


def test_a_repeated_rebuild_whose_order_does_not_pack_keeps_the_coordinates():
    """kfsp_drop_rebuild on the 4097 x 8 generator repeats its speculative build (tests/test_gpu_build_rows.py: it needs more
    entries than rows x slots).  With coordinates whose key needs 69 bits no order comes of either attempt - and the
    coordinates, compacted with the lists, must still be reported resident afterwards, as kfsp_expand_resident's rebuild
    always left them (before the two rebuilds were one function the repeated attempt of the drop left coords_n = 0)."""
    from krylovfspssa_amd import KfspContext
    from tests import row_cases as RC
    g = RC.ell_case("4097x8")
    n = g["n"]
    state = (np.arange(n, dtype=np.int32)[:, None] * np.array([1500, 1700, 1900], dtype=np.int32)).astype(np.int32)   # 23 bits each
    with KfspContext(0) as c:
        c.set_option("sell_code", 0)
        c.set_option("keep_coords", 1)
        c.set_option("state_order", 0)              # the coordinates become resident, no order is asked for
        c.set_state_coords(state)
        c.set_matrix_ell(g["adj"], g["off"], g["diag"])
        c.set_vector(RC.drop_vector(g["adj"], n))
        _, _, nflag = c.drop_plan(1.0)
        keep = c.drop_flags() == 0
        assert 0 < nflag == n - keep.sum()
        c.drop_compact()
        c.set_option("state_order", 1)              # ... and the rebuild does ask
        c.set_option("state_order_min", 64)
        c.set_option("state_order_products", 0)
        c.drop_rebuild()
        info = c.build_info()
        assert (info["speculative"], info["repeated"]) == (1, 1), info
        assert not c.state_order_active()
        s_r, a_r, o_r, d_r = c.download_fsp(3, g["bw"])
        adj2, off2, diag2 = RC.compact(g["adj"], g["off"], g["diag"], keep)
        assert np.array_equal(s_r, state[keep]) and np.array_equal(a_r, adj2) and np.array_equal(o_r, off2) and np.array_equal(d_r, diag2)
