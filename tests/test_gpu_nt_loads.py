"""The non-temporal instantiations of the stored-generator product, k_spmv<MODE, true, FMT>: the library takes them only
for a generator of more than 192 MiB (use_nt, kfsp_api.cpp), option nt_loads = 1 takes them at any size - the benchmark's
headline kernel k_spmv<0, true, 1> among them.  A non-temporal load is the same load with another cache policy: every
case here builds its generator once and runs nt_loads = 0 and 1 on it; the two must agree bit for bit, and with the
restated row (tests/row_ref.py) where a product is compared, and pass the whole-pass checks of tests/krylov_ref.py where
the fused modes are.  SELL plain and coded (formats 0, 5), banded plain and masked (1, 2), every (code width, record
bytes) form of the coded banded kernel (9), the internal state order, and a row partition over two loop-back ranks whose
products are launched in two parts, interior and boundary.  Needs a real MI355X."""
import numpy as np
import pytest

from tests import krylov_ref as K
from tests import row_cases as RC
from tests import row_ref as RR
from tests.test_gpu_dia_code import _models
from tests.test_gpu_krylov_relation import _get, _whole_pass

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
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}"


def _product(k, x, nt):
    """k.spmv(x) under nt_loads = nt, into an output that the OTHER kernel has just filled with other numbers: a row the
    kernel under test never wrote must not keep the right answer of the run before"""
    k.set_option("nt_loads", 1 - nt)
    k.spmv(np.full(len(x), 3.0))
    k.set_option("nt_loads", nt)
    return k.spmv(x)


def _both(k, x, want, what, rows=slice(None)):
    """the product with plain and with non-temporal loads: the same bits, and those of the restatement (on `rows`)"""
    ys = {}
    for nt in (0, 1):
        ys[nt] = _product(k, x, nt)
        _same(ys[nt][rows], want, f"{what}, nt_loads={nt}")
    _same(ys[1], ys[0], f"{what}, nt_loads 1 against 0")


# ---- mode 0 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.ELL))
def test_sell_products_plain_and_coded_columns(name):
    """formats 0 and 5 on the generators of tests/test_gpu_build_rows.py, the formats asserted as that file asserts them"""
    c = RC.ell_case(name)
    fmt = {}
    for sc in (0, 1):
        with _ctx(state_order=0, state_order_min=1, state_order_products=0, sell_code=sc) as k:
            k.set_matrix_ell(c["adj"], c["off"], c["diag"])
            fmt[sc] = k.layout_info()["format"]
            _both(k, c["x"], c["y"], f"{name}, sell_code={sc} (format {fmt[sc]})")
    assert fmt[0] == 0 and fmt[1] in (0, 5)
    if name.startswith("local"):
        assert fmt[1] == 5


def test_sell_product_under_the_internal_state_order():
    c = RC.ell_case("local 1500x8")
    for sc in (0, 1):
        with _ctx(format=1, state_order=1, state_order_min=1, state_order_products=0, sell_code=sc, sell_sigma=128) as k:
            k.set_state_coords(RC.made_up_coords(c["n"]))
            k.set_matrix_ell(c["adj"], c["off"], c["diag"])
            assert k.state_order_active() and k.layout_info()["state_order"] == 1
            _both(k, c["x"], c["y"], f"internal state order, sell_sigma=128, sell_code={sc}")


@pytest.mark.parametrize("name", RC.CSR)
def test_banded_products_plain_masked_and_coded(name):
    """dia_mask x dia_code on the CSR cases of tests/test_gpu_build_rows.py: formats 1, 2 and 9 where the upload stores
    diagonals, SELL (0 / 5) where it does not"""
    c = RC.csr_case(name)
    seen = set()
    for mask in (1, 0):
        for code in (0, 1):
            with _ctx(dia_mask=mask, dia_code=code) as k:
                k.set_matrix_csr(c["n"], c["rowptr"], c["col"], c["val"])
                f, coded = k.layout_info()["format"], k.dia_code_info()["active"]
                seen.add((f, coded))
                assert (f in (1, 2)) == (name in ("random banded 3", "toggle 70x61")), (name, f)
                _both(k, c["x"], c["y"], f"{name}, dia_mask={mask}, dia_code={code} -> format {f}, coded {coded}")
    if name == "toggle 70x61":
        assert (1, 0) in seen and (1, 1) in seen
    if name == "random banded 3":
        assert (2, 0) in seen and (1, 0) in seen


@pytest.mark.parametrize("case", range(6))
def test_coded_banded_product_in_every_record_form(case):
    """the models of tests/test_gpu_dia_code.py, whose one- and two-byte codes in 8- and 16-byte records are the four
    (W, REC) instantiations of format 9; up to 50 000 rows every row is restated, beyond that the first and the last 8192"""
    name, mdl, width, rec = _models()[case]
    n = mdl.n
    x = np.random.default_rng(40 + case).standard_normal(n)
    blocks = [(0, n)] if n <= 50000 else [(0, 8192), (n - 8192, 8192)]
    want = []
    for r0, nr in blocks:
        rp, cc, vv = mdl.csr_rows(r0, nr)
        rows, diag = RR.rows_from_csr(n, rp, cc, vv, row0=r0)
        want.append(np.array(RR.spmv_exact(rows, diag, x, row0=r0)))
    rowptr, col, val = mdl.csr_rows()
    ys = {}
    for dc in (0, 1):
        with _ctx(dia_mask=0, dia_code=dc) as k:
            k.set_matrix_csr(n, rowptr, col, val)
            ci = k.dia_code_info()
            assert k.layout_info()["format"] == 1 and ci["active"] == dc
            if dc:
                assert (ci["width"], ci["record_bytes"]) == (width, rec), (name, ci)
            for nt in (0, 1):
                ys[(dc, nt)] = _product(k, x, nt)
    for key, y in ys.items():
        _same(y, ys[(0, 0)], f"{name}, (dia_code, nt_loads) = {key} against (0, 0)")
        for (r0, nr), w in zip(blocks, want):
            _same(y[r0:r0 + nr], w, f"{name}, (dia_code, nt_loads) = {key}, rows {r0}..{r0 + nr}")


def test_the_cases_above_cover_the_four_record_forms():
    """each case asserts the (code width, record bytes) it declares: together they are all four instantiations"""
    assert {(w, r) for _, _, w, r in _models()} == {(8, 8), (8, 16), (16, 8), (16, 16)}


# ---- modes 1 - 3 ------------------------------------------------------------------------------------------------------------
PASSES = [("general", 65, False, {}, 2), ("general", 4097, False, {}, 2), ("general", 4097, True, {}, 2), ("general", 4097, False, {}, 1),
          ("general", 4097, False, {"format": 1, "sell_code": 1}, 2)] + \
         [("banded", n, False, {"dia_mask": m, "dia_code": 0}, 2) for n in K.BANDED_N for m in ((0, 1) if n > 131 else (0,))] + \
         [("bandedq", 4097, False, {"dia_mask": 0, "dia_code": 1}, 2), ("banded", 131, False, {"dia_mask": 0, "dia_code": 1}, 2),
          ("banded", 4097, True, {"dia_mask": 0, "dia_code": 0}, 2), ("banded", 4097, False, {"dia_mask": 0, "dia_code": 0}, 1)]


@pytest.mark.parametrize("i", range(len(PASSES)), ids=[f"{'near_' if nr else ''}{k}{n}-{'-'.join(f'{a}{b}' for a, b in o.items())}-qiop{q}"
                                                       for k, n, nr, o, q in PASSES])
def test_whole_pass_with_non_temporal_loads(i):
    """modes 1, 3 and 2 of the NT kernels behind an Arnoldi pass: the checks of krylov_ref on each setting, and the
    same H and AVNORM from both (the same arithmetic on the same numbers)"""
    kind, n, near, opts, qiop = PASSES[i]
    case = K.banded_case(n, levels=200) if kind == "bandedq" else _get(kind, n, near)
    out = {}
    with _ctx(**opts) as c:
        case.upload(c)
        fmt, coded = c.layout_info()["format"], c.dia_code_info()["active"]
        assert fmt in ((0, 5) if kind == "general" else (1, 2)), (fmt, opts)
        if kind != "general":
            assert fmt == (2 if opts["dia_mask"] else 1) and coded == opts["dia_code"], (fmt, coded, opts)
        for nt in (0, 1):
            c.set_option("nt_loads", nt)
            r, H, av = _whole_pass(c, case, qiop=qiop, combine=False)
            print(f"\n{case.name} {opts} qiop {qiop} nt_loads {nt} format {fmt}: {K.fmt(r)}")
            K.assert_ok(r, f"{case.name}, {opts}, nt_loads={nt}")
            out[nt] = (H.copy(), av)
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


# ---- a partition --------------------------------------------------------------------------------------------------------------
def test_split_product_of_two_ranks():
    """a banded generator over two loop-back ranks, halo strips, overlap = 2: a rank's product of its own rows is two
    launches, interior and boundary (tests/test_box_gated_cases.py restates the rule), each with the NT kernel"""
    from krylovfspssa_amd.host import run_loopback_ranks
    c = RC.csr_case(RC.CSR_SPLIT)
    n, x = c["n"], c["x"]

    def body(k, rank):
        k.set_option("small_kernel", 0)
        k.set_option("overlap", 2)
        r0, nr = k.row_block(n)
        rp = c["rowptr"][r0:r0 + nr + 1]
        k.set_matrix_csr(n, rp - rp[0], c["col"][rp[0]:rp[-1]], c["val"][rp[0]:rp[-1]])
        out = {}
        for nt in (0, 1):
            k.set_option("nt_loads", nt)
            k.set_vector(x[r0:r0 + nr])
            out[nt] = (k.spmv(x), k.spmv_w())
        return r0, nr, out, k.layout_info()

    res = run_loopback_ranks(2, body)
    assert sum(nr for _, nr, _, _ in res) == n
    for rank, (r0, nr, out, info) in enumerate(res):
        assert info["format"] in (1, 2) and info["exchange"] == 1, info
        for nt in (0, 1):
            for which, y in zip(("spmv", "spmv_w"), out[nt]):
                _same(y, c["y"][r0:r0 + nr], f"rank {rank}, nt_loads={nt}, {which}")
