"""The generator product against a statement of what a row IS (tests/row_ref.py: -(diag * x_r) as one multiply, then
one fused multiply-add per entry, entries ascending by the caller's source index, then value), bit for bit, on every
stored form and every way a generator gets built: device-built SELL from general uploads whose rows are longer than
the register sort's cap (with and without build_speculate, built twice), plain and dictionary-coded columns, the
internal state order (and sell_sigma), banded / masked banded / coded banded, a row partition over two loop-back ranks,
and the rebuild of a resident generator after DROP_STATES.  tests/test_row_ref.py shows on the CPU that each of these
cases has rows whose bits change when they are summed in another order.  Needs a real MI355X."""
import numpy as np
import pytest

from tests import row_cases as RC
from tests import row_ref as RR

pytestmark = pytest.mark.gpu


def _ctx(**options):
    from krylovfspssa_amd import KfspContext
    c = KfspContext(0)
    c.set_option("small_kernel", 0)
    for k, v in options.items():
        c.set_option(k, v)
    return c


def _same(y, want, what):
    bad = np.flatnonzero(RC.bits(y) != RC.bits(want))
    assert bad.size == 0, f"{what}: {bad.size} rows differ from the restatement, first {bad[:5]}"


@pytest.mark.parametrize("name", list(RC.ELL))
def test_device_built_sell_rows_are_the_restated_rows(name):
    """set_matrix_ell of a general generator: rows longer than the cap of the register sort (and, for 1000 x 4, than
    the slot count) must come out fully sorted - with the register sort (build_speculate = 1) and with the insertion
    sort (0), and in every build alike: two fresh contexts each"""
    c = RC.ell_case(name)
    for spec in (1, 0):
        for upload in (0, 1):
            with _ctx(build_speculate=spec, sell_code=0) as k:
                k.set_matrix_ell(c["adj"], c["off"], c["diag"])
                assert k.layout_info()["format"] == 0
                assert k.matrix_info()["nnz"] == sum(map(len, c["rows"])) + c["n"]
                _same(k.spmv(c["x"]), c["y"], f"{name}, build_speculate={spec}, upload {upload}")


@pytest.mark.parametrize("name", list(RC.ELL))
def test_plain_and_coded_columns(name):
    """the same generators with the column dictionary off and on (the option pair of tests/test_gpu_sell_code.py):
    kernel formats 0 and 5.  Chunks of the random generators see more than 64 offsets and keep their columns; the
    generator of near links codes, and its rows are as long"""
    c = RC.ell_case(name)
    fmt = {}
    for sc in (0, 1):
        with _ctx(state_order=0, state_order_min=1, state_order_products=0, sell_code=sc) as k:
            k.set_matrix_ell(c["adj"], c["off"], c["diag"])
            info = k.layout_info()
            fmt[sc] = info["format"]
            if sc and name.startswith("local"):
                assert info["coded_chunks"] >= 0.9 * (info["chunks"] - 1)
            _same(k.spmv(c["x"]), c["y"], f"{name}, sell_code={sc}")
    assert fmt[0] == 0 and fmt[1] in (0, 5)
    if name.startswith("local"):
        assert fmt[1] == 5


@pytest.mark.parametrize("sigma", [0, 128])
@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("which", ["goutsias", "made up", "made up, near links"])
def test_internal_state_order_keeps_the_callers_row_order(which, spec, sigma):
    """under the internal (lexicographic) state order - and the SELL-sigma window sort on top of it - a row is still
    summed ascending by the CALLER's index of its sources"""
    if which == "goutsias":
        c = RC.golden_case()
        state = c["state"]
    else:
        c = RC.ell_case("4097x8" if which == "made up" else "local 1500x8")
        state = RC.made_up_coords(c["n"])
    for sc in (0, 1):
        with _ctx(format=1, state_order=1, state_order_min=1, state_order_products=0, sell_code=sc, sell_sigma=sigma,
                  build_speculate=spec) as k:
            k.set_state_coords(state)
            k.set_matrix_ell(c["adj"], c["off"], c["diag"])
            assert k.state_order_active() and k.layout_info()["state_order"] == 1
            _same(k.spmv(c["x"]), c["y"], f"{which}, sigma={sigma}, build_speculate={spec}, sell_code={sc}")


@pytest.mark.parametrize("name", RC.CSR)
def test_banded_forms_sum_a_row_by_ascending_diagonal(name):
    """CSR uploads: stored diagonals (plain, masked, dictionary-coded values) where the banded form is taken, SELL
    where it is not or is forced: diagonals ascending by their shift is ascending by source"""
    c = RC.csr_case(name)
    deltas = {col - r for r, row in enumerate(c["rows"]) for col, _ in row}
    banded = len(deltas) * c["n"] <= 1.5 * sum(map(len, c["rows"])) + 1024           # the rule of the upload
    assert banded == (name in ("random banded 3", "toggle 70x61"))
    seen = set()
    for fmt in (0, 1):
        for mask in (1, 0):
            for code in (0, 1):
                with _ctx(format=fmt, dia_mask=mask, dia_code=code) as k:
                    k.set_matrix_csr(c["n"], c["rowptr"], c["col"], c["val"])
                    f = k.layout_info()["format"]
                    coded = k.dia_code_info()["active"]
                    seen.add((f, coded))
                    assert (f in (1, 2)) == (banded and fmt == 0), (name, fmt, mask, code, f)
                    assert not (coded and (f != 1 or not code))
                    _same(k.spmv(c["x"]), c["y"], f"{name}, format={fmt}, dia_mask={mask}, dia_code={code} -> {f}")
    if name == "toggle 70x61":
        assert (1, 0) in seen and (1, 1) in seen          # propensities: few distinct values per diagonal, coded
    if name == "random banded 3":
        assert (2, 0) in seen and (1, 0) in seen          # far diagonals leave whole row groups empty: masked


@pytest.mark.parametrize("name", ["1000x4", "2000x12"])
def test_row_partition_over_two_ranks(name):
    from krylovfspssa_amd.host import run_loopback_ranks
    c = RC.ell_case(name)

    def body(k, rank):
        k.set_option("small_kernel", 0)
        k.set_matrix_ell(c["adj"], c["off"], c["diag"])
        return k.row0, k.nloc, k.spmv(c["x"])

    out = run_loopback_ranks(2, body)
    assert sum(nloc for _, nloc, _ in out) == c["n"] and out[0][1] > 0 and out[1][1] > 0
    for rank, (row0, nloc, y) in enumerate(out):
        rows = RR.gather_rows(c["adj"], c["off"], c["diag"], row0=row0, nloc=nloc)
        want = np.array(RR.spmv_exact(rows, c["diag"][row0:row0 + nloc], c["x"], row0=row0))
        _same(y, want, f"{name}, rank {rank}")
        assert np.array_equal(RC.bits(want), RC.bits(c["y"][row0:row0 + nloc]))


@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("dropped", ["none", "a twentieth"])
def test_rebuild_of_a_resident_general_generator(dropped, spec):
    """drop_plan / drop_compact / drop_rebuild on the 4097 x 8 generator: the speculative rebuild reserves rows x slots
    entries, this generator needs 48 512 against 33 280 - nothing may be stored beyond the reservation, the build is
    repeated the slow way (build_info: repeated) and the product is that of the compacted lists"""
    c = RC.ell_case("4097x8")
    n = c["n"]
    w = np.ones(n) if dropped == "none" else RC.drop_vector(c["adj"], n)
    with _ctx(build_speculate=spec, sell_code=0) as k:
        k.set_matrix_ell(c["adj"], c["off"], c["diag"])
        k.set_vector(w)
        droptol, _, nflag = k.drop_plan(1.0)
        assert droptol == 1e-8
        keep = ~k.drop_flags().astype(bool)
        assert nflag == n - keep.sum()
        if dropped == "none":
            assert nflag == 0
            want, x = c["y"], c["x"]
        else:
            assert 0.03 * n <= nflag <= 0.08 * n
            adj2, off2, diag2 = RC.compact(c["adj"], c["off"], c["diag"], keep)
            x = c["x"][keep]
            want = np.array(RR.spmv_exact(RR.gather_rows(adj2, off2, diag2), diag2, x))
        assert k.drop_compact() == keep.sum()
        k.drop_rebuild()
        assert k.n == keep.sum()
        info = k.build_info()
        print(f"dropped {nflag} of {n}, build_speculate={spec}: {info}")
        assert (info["speculative"], info["repeated"]) == ((1, 1) if spec else (0, 0))
        assert k.layout_info()["format"] == 0
        _same(k.spmv(x), want, f"rebuild, {dropped} dropped, build_speculate={spec}")
        assert np.array_equal(k.get_vector(), w[keep])
