"""The matrix-free box product against a statement of what a row IS, bit for bit (tests/row_ref.py).  box_exact: the
single-factor fast path - format 4 and everything pinned to it: the LDS window (6), pencils (7), slabs (8) and every
column of kfsp_spmm under block_box; accumulator from +0.0, one fused multiply-add per slot by species then slot, the
diagonal last.  box_generic_exact: the interpreted kernel (format 3) and the product of the generator that box_store
writes out; -(dsum x_r) as one multiply, then one fused multiply-add per reaction in sorted position.  Under the default
grid, under grid_blocks = 8 (the loop_* boxes: wavefronts go round the trip loop, a second copy of the row code), cut
into row blocks over loop-back ranks (halo strips and the all-gather), and on one context that takes every box in turn.
tests/test_row_ref.py shows on the CPU that the cases have rows whose bits change under a wrong order, a diagonal
applied at the other end, a tie broken the other way, shares or factors taken backwards - and rows whose coordinate
decode needs its correction step.  Needs a real MI355X."""
import numpy as np
import pytest

from tests import box_cases as BC
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
    bad = BC.mismatches(y, want)
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rows differ from the restatement, first {bad[:5]}"


def _lds_format(mdl, reach):
    """format 6 needs an entry within box_reach rows (the default reach takes every entry of these boxes)"""
    return 6 if reach is None or int(np.abs(mdl.offsets).min()) <= reach else 4


@pytest.mark.parametrize("name", BC.SMALL)
def test_single_factor_product_is_the_restated_row_in_every_format(name):
    """formats 4, 6 (also with only the +-1 entries from LDS), 7 and 8 where the eligibility rule of kfsp_set_matrix_box
    admits the box - and format 4, asserted, where it does not"""
    c = BC.case(name)
    mdl = c["mdl"]
    runs = [("gather", dict(box_pencil=0), 4), ("gather, 8 workgroups", dict(box_pencil=0, grid_blocks=8), 4),
            ("lds", dict(box_pencil=0, box_lds=1), _lds_format(mdl, None)),
            ("lds, reach 2", dict(box_pencil=0, box_lds=1, box_reach=2), _lds_format(mdl, 2)),
            ("pencils", dict(box_pencil=1), BC.pencil_format(mdl, 1)), ("slabs", dict(box_pencil=2), BC.pencil_format(mdl, 2)),
            ("pencils, 8 workgroups", dict(box_pencil=1, grid_blocks=8), BC.pencil_format(mdl, 1)),
            ("slabs, 8 workgroups", dict(box_pencil=2, grid_blocks=8), BC.pencil_format(mdl, 2))]
    seen = set()
    for what, options, fmt in runs:
        with _ctx(**options) as k:
            k.set_matrix_box(mdl, store=False)
            assert k.layout_info()["format"] == fmt, (name, what, k.layout_info())
            seen.add(fmt)
            _same(k.spmv(c["x"]), c["y"], f"{name}, {what} (format {fmt})")
    assert {4, 6} <= seen
    if name in ("decode_8x49x2", "decode_2x49x2x2x2x2", "box_birth_death_6x2"):
        assert {7, 8} <= seen
    if name == "decode_49x4x3":
        assert 7 in seen


@pytest.mark.parametrize("name", BC.LOOP)
def test_trip_loop_of_the_single_factor_and_the_interpreted_kernel(name):
    """34 - 47 trips on 8 workgroups: wavefronts 0 (and 1) of a workgroup take a second trip through the loop's own
    copy of the row code - format 4 against box_exact, format 3 against box_generic_exact; and the default grid"""
    c = BC.case(name)
    for grid in (8, 0):
        with _ctx(box_pencil=0, grid_blocks=grid) as k:
            k.set_matrix_box(c["mdl"], store=False)
            assert k.layout_info()["format"] == 4
            _same(k.spmv(c["x"]), c["y"], f"{name}, format 4, grid_blocks={grid}")
        with _ctx(box_generic=1, grid_blocks=grid) as k:
            k.set_matrix_box(c["mdl"], store=False)
            assert k.layout_info()["format"] == 3
            _same(k.spmv(c["x"]), c["yg"], f"{name}, format 3, grid_blocks={grid}")


@pytest.mark.parametrize("name", BC.SMALL + BC.generic_names())
def test_interpreted_kernel_is_the_restated_generic_row(name):
    """format 3: forced (box_generic = 1) on the single-factor boxes, the only form of the others"""
    c = BC.case(name)
    for grid in (0, 8):
        with _ctx(box_generic=1, grid_blocks=grid) as k:
            k.set_matrix_box(c["mdl"], store=False)
            assert k.layout_info()["format"] == 3
            _same(k.spmv(c["x"]), c["yg"], f"{name}, format 3, grid_blocks={grid}")
    if name not in BC.FAST:
        with _ctx() as k:                                        # no option: several factors leave no other kernel
            k.set_matrix_box(c["mdl"], store=False)
            assert k.layout_info()["format"] == 3
            _same(k.spmv(c["x"]), c["yg"], f"{name}, format 3 unasked")


@pytest.mark.parametrize("name", BC.SMALL + BC.generic_names())
def test_generator_written_out_by_the_device_gives_the_restated_generic_row(name):
    """box_store = 1: k_box_materialize writes the factor products and DIAG, an ordinary banded product follows - plain
    and dictionary-coded values, and with option format = 1, which a box ignores (a box written out is banded by
    construction; the format it reports must still be a banded one)"""
    c = BC.case(name)
    for options in (dict(dia_code=0), dict(dia_code=1), dict(dia_code=0, format=1), dict(dia_code=0, dia_mask=0)):
        with _ctx(**options) as k:
            k.set_matrix_box(c["mdl"], store=True)
            info = k.layout_info()
            assert info["format"] in (1, 2) and k.matrix_info()["slots"] > 0, (name, options, info)
            assert not (k.dia_code_info()["active"] and not options["dia_code"])
            _same(k.spmv(c["x"]), c["yg"], f"{name}, box_store, {options} -> format {info['format']}")


@pytest.mark.parametrize("name,P,gather", BC.PARTITIONED)
def test_row_blocks_of_a_matrix_free_box_are_blocks_of_the_restated_rows(name, P, gather):
    """P loop-back ranks, each with its row0 / nloc (a ragged last block everywhere; repressilator over three ranks:
    blocks shorter than the reach, so x travels by all-gather).  Formats 4 and 3; the product of a whole x handed in
    (kfsp_spmv) and of the rank's own rows after the exchange (kfsp_spmv_w); each block against the restatement OF THAT
    BLOCK, which in turn is the block of the whole"""
    from krylovfspssa_amd.host import run_loopback_ranks
    c = BC.case(name)
    mdl, x = c["mdl"], c["x"]
    single = name in BC.FAST
    for generic in ((0, 1) if single else (1,)):
        def body(k, rank):
            k.set_option("small_kernel", 0)
            k.set_option("box_generic", generic)
            k.set_matrix_box(mdl, store=False)
            y = k.spmv(x)
            k.set_vector(x[k.row0:k.row0 + k.nloc])
            return k.row0, k.nloc, y, k.spmv_w(), k.layout_info()

        out = run_loopback_ranks(P, body)
        assert sum(nloc for _, nloc, *_ in out) == mdl.n and all(nloc > 0 for _, nloc, *_ in out)
        for rank, (row0, nloc, y, yw, info) in enumerate(out):
            assert info["format"] == (3 if generic else 4) and info["exchange"] == (2 if gather else 1), (name, P, rank, info)
            fn = RR.box_generic_exact if generic else RR.box_exact
            want = np.array(fn(mdl, x, row0=row0, nloc=nloc))
            assert np.array_equal(BC.bits(want), BC.bits(c["yg" if generic else "y"][row0:row0 + nloc]))
            _same(y, want, f"{name}, {P} ranks, rank {rank}, format {info['format']}, spmv")
            _same(yw, want, f"{name}, {P} ranks, rank {rank}, format {info['format']}, spmv_w")


@pytest.mark.parametrize("name", ["box_toggle_2x2", "box_repressilator_3x2", "box_birth_death_6x2", "box_four_slot_6x4", "dup_12x9",
                                  "decode_49x4x3", "decode_2x49x2x2x2x2", "decode_toggle_98x6"])
def test_block_product_columns_are_the_restated_rows(name):
    """kfsp_spmm under block_box = 1 (k_spmm_box, its own copy of the decode and of the row): every column against
    box_exact itself, not by way of kfsp_spmv; k = 1, 5 and 16 on one box per instantiation, k = 5 on the others"""
    ks = BC.BLOCK_K if name.startswith("box_") else (5,)
    X, Y = BC.block(name, max(ks))
    with _ctx(block_box=1) as k:
        k.set_matrix_box(BC.model(name), store=False)
        assert k.layout_info()["format"] == 4
        for kk in ks:
            Z = k.spmm(X[:, :kk])
            assert Z.shape == (BC.model(name).n, kk)
            for j in range(kk):
                _same(Z[:, j], Y[:, j], f"{name}, k = {kk}, column {j}")
    with _ctx(block_box=1, grid_blocks=8) as k:
        k.set_matrix_box(BC.model(name), store=False)
        kk = ks[-1]
        Z = k.spmm(X[:, :kk])
        for j in range(kk):
            _same(Z[:, j], Y[:, j], f"{name}, 8 workgroups, k = {kk}, column {j}")


def test_one_context_through_every_box_largest_first():
    """every smaller box runs on whatever the previous one left in the buffers and in the table image: the
    single-factor boxes through format 4, then written out (box_store), the others through format 3"""
    names = sorted(BC.SMALL + BC.generic_names(), key=lambda n: -BC.model(n).n)
    assert BC.model(names[0]).n > 10 * BC.model(names[-1]).n
    with _ctx(box_pencil=0) as k:
        for name in names:
            c = BC.case(name)
            k.set_matrix_box(c["mdl"], store=False)
            fmt = k.layout_info()["format"]
            assert fmt == (4 if name in BC.FAST else 3), (name, fmt)
            _same(k.spmv(c["x"]), c["y" if fmt == 4 else "yg"], f"{name} in sequence, format {fmt}")
            _same(k.spmv(c["x"]), c["y" if fmt == 4 else "yg"], f"{name} in sequence, format {fmt}, again")
            k.set_matrix_box(c["mdl"], store=True)
            _same(k.spmv(c["x"]), c["yg"], f"{name} in sequence, written out")
