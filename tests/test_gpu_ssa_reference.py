"""The device SSA walk (krylovfspssa_amd/csrc/kfsp_ssa.hip: k_ssa_walk<NS,NR,LIGHT,REGS>, k_ssa_walk_any, the hash builds,
the record sort / first occurrence / gather, the record-list regrow, the partitioned share) against the plain restatement
of its definition (tests/ssa_ref.py, checked on the CPU by tests/test_ssa_ref.py).  The walk is defined bit for bit, so
every comparison is np.array_equal on the new states and their offdiag / diag columns."""
import ctypes as C

import numpy as np
import pytest

from tests import ssa_ref as R
from tests.expand_helpers import onestep_py

pytestmark = pytest.mark.gpu


def _equal(got, ref, what):
    s, o, d = got
    assert s.shape == ref.state_new.shape, (what, s.shape, ref.state_new.shape)
    assert np.array_equal(s, ref.state_new), what
    assert np.array_equal(o, ref.off_new), what
    assert np.array_equal(d, ref.diag_new), what


def _run(case, **kw):
    from krylovfspssa_amd import KfspContext
    with KfspContext(0) as c:
        return case.on_device(c, capacity_new=kw.pop("capacity_new", case.ref.nnew + 64), **kw)


def _status(err):
    """the status a refused call returned (KfspError: '<call> -> <status>: <text>')"""
    return int(str(err.value).split("->")[1].split(":")[0])


@pytest.mark.parametrize("i", range(13))
def test_every_kernel_of_the_dispatch(i):
    """One model per launch of ssa_streams_core; the case's name is the kernel it reaches (a kernel-trace run of this file
    saw all eight):
      0 k_ssa_walk<2,4,true,true>    2 species, 4 reactions, chains
      1 k_ssa_walk<6,12,true,true>   5 species, 10 reactions
      2 k_ssa_walk<8,16,true,true>   8 species, 11 reactions        3 the same kernel through 14 reactions of 4 species
      4 k_ssa_walk<2,4,true,false>   5 k_ssa_walk<6,12,true,false>   6 k_ssa_walk<8,16,true,false>   (ssa_regs = 0)
      7 k_ssa_walk<8,16,false,false> 618 code words (chains padded with `+ p`, p = 0.0): more than the 512 kept in LDS
      8 k_ssa_walk_any               ssa_general = 1      9 12 species     10 30 reactions     11 16 species, 64 reactions
     12 k_ssa_walk_any               a coefficient of +-200 (outside the signed byte of the register kernels)"""
    case = R.variant_cases()[i]
    assert case.ref.nnew > 0 and case.ref.virtual_jumps > 0 and case.ref.records > case.ref.nnew
    _equal(_run(case), case.ref, case.name)


def test_models_beyond_the_limits_are_refused():
    """ns > 16 -> -4, nr > 64 -> -5 (kfsp_ssa_streams), and no output is touched"""
    from krylovfspssa_amd import KfspContext
    from krylovfspssa_amd.host import _p
    with KfspContext(0) as c:
        R.edge_case(64).program.set_on(c)
        for ns, nr, want in ((17, 4, -4), (4, 65, -5)):
            n = 8
            state = np.zeros((n, ns), dtype=np.int32)
            adj = np.zeros((n, nr), dtype=np.int32)
            off = np.ones((n, nr))
            diag = np.full(n, float(nr))
            nu = np.ones((nr, ns), dtype=np.int32)
            nf = C.c_int32(777)
            st_new = np.full((32, ns), -7, dtype=np.int32)
            off_new = np.full((32, nr), -7.0)
            diag_new = np.full(32, -7.0)
            rc = c._lib.kfsp_ssa_streams(c._h, 1.0, 1, ns, nr, _p(nu), n, _p(state), ns, _p(adj), _p(off), nr, _p(diag), 100, 32,
                                         C.byref(nf), _p(st_new), _p(off_new), nr, _p(diag_new))
            assert rc == want, (ns, nr, rc)
            assert nf.value == 777 and (st_new == -7).all() and (off_new == -7.0).all() and (diag_new == -7.0).all()
        # the context is still good for a valid call
        case = R.edge_case(64)
        _equal(case.on_device(c, capacity_new=case.ref.nnew + 1), case.ref, "after the refusals")


@pytest.mark.parametrize("general", [0, 1])
def test_random_networks_against_the_restatement(general):
    """the random family of tests/ssa_ref.py (1-10 species, 1-20 reactions, links complete / partial / zero, absorbing seeds,
    horizons from the first jump to far outside) through the kernel the dispatch chooses and through the general one"""
    from krylovfspssa_amd import KfspContext
    fam = R.random_family()
    dup, fired, empty = R.family_conditions(fam)
    assert 3 * dup >= len(fam) and fired == set(R.END_RULES) and empty == [R.NOTHING_FOUND]
    with KfspContext(0) as c:
        c.set_option("ssa_general", general)
        for case in fam:
            _equal(case.on_device(c, capacity_new=case.ref.nnew + 64), case.ref, case.name)


def test_random_networks_resident_expansion_against_the_restatements():
    """the same family through kfsp_expand_resident: the restated walk, then the plain one-step sweep on its result, the
    columns of every appended state from the restated interpreter"""
    from krylovfspssa_amd import KfspContext
    rng = np.random.default_rng(5)
    for i, case in enumerate(R.random_family()):
        nr, ns = case.nu.shape
        ref = case.ref
        n = len(case.state)
        st1 = np.concatenate([case.state, ref.state_new])
        ad1 = np.concatenate([case.adj, np.zeros((ref.nnew, nr), dtype=np.int32)])
        st2, ad2 = onestep_py(case.nu, st1, ad1, case.max_count)
        o2, d2 = case.program.columns(st2[len(st1):])
        with KfspContext(0) as c:
            case.program.set_on(c)
            c.set_option("state_order", i % 2)
            c.set_option("state_order_min", 1)
            c.set_option("state_order_products", 0)
            c.set_option("ssa_general", (i // 2) % 2)
            c.set_option("keep_coords", 1)
            c.set_state_coords(case.state)
            c.set_matrix_ell(case.adj, case.off, case.diag)
            w = rng.random(n)
            c.set_vector(w)
            n2, nssa = c.expand_resident(case.tstep, case.seedmix, case.nu, max_count=case.max_count)
            assert (n2, nssa) == (len(st2), ref.nnew), case.name
            s_r, a_r, o_r, d_r = c.download_fsp(ns, nr)
            assert np.array_equal(s_r, st2) and np.array_equal(a_r, ad2), case.name
            assert np.array_equal(o_r, np.concatenate([case.off, ref.off_new, o2])), case.name
            assert np.array_equal(d_r, np.concatenate([case.diag, ref.diag_new, d2])), case.name
            assert np.array_equal(c.get_vector(), np.concatenate([w, np.zeros(n2 - n)])), case.name


@pytest.mark.parametrize("n0", [1, 63, 64, 65, 255, 256, 257, 1025, 20000])
def test_seed_dealing(n0):
    """seeds are dealt in blocks of 64 round robin over wavefronts of 256 seeds: one lane, one short of / exactly / one
    beyond a block and a wavefront, a second workgroup (1025), 79 wavefronts (20 000); register and general kernel"""
    case = R.edge_case(n0)
    assert case.ref.nnew > 0
    _equal(_run(case), case.ref, n0)
    from krylovfspssa_amd import KfspContext
    with KfspContext(0) as c:
        c.set_option("ssa_general", 1)
        _equal(case.on_device(c, capacity_new=case.ref.nnew + 64), case.ref, (n0, "general"))


@pytest.mark.parametrize("seedmix", [0, 1, 2 ** 31 - 2, 2 ** 62 + 12345])
def test_seedmix_edges_and_repeatability(seedmix):
    """the product seedmix * 2654435761 wraps 64 bits for the last one; the same call twice gives the same bits"""
    from krylovfspssa_amd import KfspContext
    case = R.edge_case(1025, seedmix=seedmix)
    assert case.ref.nnew > 0
    with KfspContext(0) as c:
        a = case.on_device(c, capacity_new=case.ref.nnew + 64)
        b = case.on_device(c, capacity_new=case.ref.nnew + 64)
    _equal(a, case.ref, seedmix)
    _equal(b, case.ref, seedmix)
    other = R.edge_case(1025, seedmix=seedmix + 1).ref
    assert not np.array_equal(other.state_new, case.ref.state_new)          # (the seed matters)


@pytest.mark.parametrize("max_count", [11, 20])
@pytest.mark.parametrize("regs", [1, 0])
def test_population_cap_and_table_edge(max_count, regs):
    """max_count cuts paths (LEGAL: y <= max_count still walks, max_count + 1 ends the path); a reaction behind a
    12-entry table whose population runs to the last entry (max_count = 11) and into the code beyond it (20)"""
    from krylovfspssa_amd import KfspContext
    case = R.table_case(max_count)
    ref = case.ref
    assert ref.ends["illegal"] > 0 and int(ref.state_new[:, 0].max()) == max_count and ref.virtual_jumps > 100
    with KfspContext(0) as c:
        c.set_option("ssa_regs", regs)
        _equal(case.on_device(c, capacity_new=ref.nnew + 64), ref, (max_count, regs))
        c.set_option("ssa_general", 1)
        _equal(case.on_device(c, capacity_new=ref.nnew + 64), ref, (max_count, "general"))


def test_capacity_exactly_met_and_exceeded_by_one():
    """capacity_new == nnew succeeds; nnew - 1 returns -11 (kfsp_ssa_streams) and the next valid call is right"""
    from krylovfspssa_amd import KfspContext, KfspError
    case = R.edge_case(1025)
    ref = case.ref
    assert ref.nnew > 1
    with KfspContext(0) as c:
        _equal(case.on_device(c, capacity_new=ref.nnew), ref, "capacity met")
        with pytest.raises(KfspError) as err:
            case.on_device(c, capacity_new=ref.nnew - 1)
        assert _status(err) == -11
        _equal(case.on_device(c, capacity_new=ref.nnew), ref, "after the refusal")


@pytest.mark.parametrize("general", [0, 1])
def test_record_list_regrow(general):
    """every seed leaves the FSP at once and records its whole path: more than 2^18 records, so the first list is too short
    and the walk is repeated with the counted size - through the register kernel (which takes the list 64 slots at a time
    and leaves some empty) and through the general one"""
    case = R.regrow_case(bool(general))
    ref = R.regrow_ref()
    assert ref.records > 2 ** 18 and ref.nnew == ref.records
    _equal(_run(case, capacity_new=ref.nnew), ref, general)


@pytest.mark.parametrize("n0", [300, 5000])
@pytest.mark.parametrize("partition", [1, 0])
def test_partitioned_walk_under_three_ranks(n0, partition):
    """three loop-back ranks expand the resident lists: with ssa_partition = 1 each walks its share of the wavefronts (n0 = 300
    has two, so one rank's share is empty) and the records are gathered; every rank must hold the restatement's lists"""
    from krylovfspssa_amd import host
    case = R.edge_case(n0)
    ref = case.ref
    nr, ns = case.nu.shape
    n = len(case.state)
    assert ref.nnew > 0 and (n0 + 255) // 256 == (2 if n0 == 300 else 20)
    st1 = np.concatenate([case.state, ref.state_new])
    ad1 = np.concatenate([case.adj, np.zeros((ref.nnew, nr), dtype=np.int32)])
    st2, ad2 = onestep_py(case.nu, st1, ad1, case.max_count)
    o2, d2 = case.program.columns(st2[len(st1):])

    def body(c, rank):
        case.program.set_on(c)
        c.set_option("ssa_partition", partition)
        c.set_option("state_order", 0)
        c.set_option("keep_coords", 1)
        c.set_state_coords(case.state)
        c.set_matrix_ell(case.adj, case.off, case.diag)
        r0, nloc = c.row_block(n)
        c.set_vector(np.full(nloc, 1.0 / n))
        n2, nssa = c.expand_resident(case.tstep, case.seedmix, case.nu, max_count=case.max_count)
        return (n2, nssa) + tuple(c.download_fsp(ns, nr))

    for rank, (n2, nssa, s_r, a_r, o_r, d_r) in enumerate(host.run_loopback_ranks(3, body)):
        assert (n2, nssa) == (len(st2), ref.nnew), rank
        assert np.array_equal(s_r, st2) and np.array_equal(a_r, ad2), rank
        assert np.array_equal(o_r, np.concatenate([case.off, ref.off_new, o2])), rank
        assert np.array_equal(d_r, np.concatenate([case.diag, ref.diag_new, d2])), rank
