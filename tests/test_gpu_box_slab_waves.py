"""The pencil kernels where no other test size takes them.  Format 8 (slabs) with a workgroup of 1, 2, 3, 5 and 12
wavefronts (option box_slab_waves, and boxes whose second-slowest species has 2 or 3 counts): the product against the
restated row, bit for bit, and the fused modes - whose prologue sums the producer's partials the way the 256-thread
kernels do, on however many wavefronts there are - through the whole-pass checks of tests/krylov_ref.py.  Format 7
(pencils) with the tiled base-trip order that option box_tile = 1 puts in effect on planes far smaller than the 4 MiB
from which the library chooses it (kfsp_build_info reports its length): same bits in either order.  The shapes and the
restated rules are in tests/box_cases.py and tests/krylov_ref.py; tests/test_box_gated_cases.py shows on the CPU that
they reach what is claimed here.  Needs a real MI355X."""
import numpy as np
import pytest

from tests import box_cases as BC
from tests import krylov_ref as K
from tests.test_gpu_krylov_relation import _whole_pass

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


def _product(k, x, pencil):
    """k.spmv(x) into an output that holds something else: one context runs many settings on the same x, and a row that
    a wrong kernel never wrote would otherwise still hold the right answer of the setting before.  The other numbers come
    from another kernel - format 4, which box_pencil = 0 selects at the launch - so that it writes every row"""
    k.set_option("box_pencil", 0)
    k.spmv(np.full(len(x), 3.0))
    k.set_option("box_pencil", pencil)
    return k.spmv(x)


# ---- format 8, products ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.SLAB) + ["tile_conversion_8x8x8x4x2x3"])
def test_slab_product_is_the_restated_row_at_every_workgroup_width(name):
    """box_slab_waves 1, 2, 3, 5, 12 under the default grid and under grid_blocks = 8 (every workgroup loops over
    slabs); one context, the generator set again after every change of option (the geometry is fixed there).  The
    conversion box: the instantiation that masks entries by the slowest species' valid bit, on two lines"""
    c = BC.gated_case(name)
    with _ctx(box_pencil=2) as k:
        for waves in BC.SLAB_WAVES:
            for grid in (0, 8):
                k.set_option("box_slab_waves", waves)
                k.set_option("grid_blocks", grid)
                k.set_matrix_box(c["mdl"], store=False)
                assert k.layout_info()["format"] == 8, (name, waves, grid, k.layout_info())
                _same(_product(k, c["x"], 2), c["y"], f"{name}, box_slab_waves={waves}, grid_blocks={grid}")


def test_a_box_without_slabs_after_one_with_them():
    """box_pencil = 2 stays set; a two-species box has neither pencils nor slabs and must not be given the previous
    box's: format 4 and the restated rows"""
    big, small = BC.gated_case("slab_8x8x8x4x3x2"), BC.case("box_toggle_2x2")
    with _ctx(box_pencil=2) as k:
        k.set_matrix_box(big["mdl"], store=False)
        assert k.layout_info()["format"] == 8
        _same(k.spmv(big["x"]), big["y"], "slabs")
        k.set_matrix_box(small["mdl"], store=False)
        assert k.layout_info()["format"] == 4, k.layout_info()
        _same(k.spmv(small["x"]), small["y"], "the two-species box after the slabs")


# ---- format 8, fused modes --------------------------------------------------------------------------------------------------
SLAB_PASSES = [("slab_narrow", 1), ("slab_narrow", 2), ("slab_narrow", 3), ("slab_narrow", None), ("slab_large", 1), ("slab_large", 2)]


@pytest.mark.parametrize("name,waves", SLAB_PASSES, ids=[f"{n}-waves{w}" for n, w in SLAB_PASSES])
def test_arnoldi_pass_through_narrow_slabs(name, waves):
    """MODE 1, 3 and 2 of k_spmv_slab on workgroups of fewer than four wavefronts: the norm of the source column is
    finished inside the product from the partials of the kernel before it - 6 of them at 12 288 rows, 96 at 196 608: more
    than one wavefront has lanes - and scales the product and becomes H(j+1,j); the relation and the normalisation of
    krylov_ref pin both"""
    case = K.box_case(name)
    opts = {"small_kernel": 0, "box_pencil": 2}
    if waves is not None:
        opts["box_slab_waves"] = waves
    with _ctx(**opts) as c:
        case.upload(c)
        assert c.layout_info()["format"] == 8, c.layout_info()
        r, _, _ = _whole_pass(c, case)
    print(f"\nslabs, {name}, box_slab_waves {waves}: {K.fmt(r)}")
    K.assert_ok(r, f"format 8, {name}, box_slab_waves {waves}")


# ---- format 7 with a base-trip order ----------------------------------------------------------------------------------------
def _base_trips(mdl):
    return -(-int(np.prod(mdl.dims[:-1])) // 128)


@pytest.mark.parametrize("name", BC.TILED + ("tile_four_slot_8x8x8x4x2x2", "tile_conversion_8x8x8x4x2x3"))
def test_pencil_product_under_the_tiled_base_trip_order(name):
    """box_tile = 0 / 1 (and -1: the default, ascending on a plane this small) under the default grid and with one
    workgroup per XCD range (grid_blocks = 8: every wavefront loops): format 7, the order's length as build_info
    reports it, the restated rows.  Instance <6,2>, <6,4> (four_slot) and <6,4> with an entry of species 0 that moves
    the slowest species (conversion: the kernel's SIMPLE = false instantiation)"""
    c = BC.gated_case(name)
    trips = _base_trips(c["mdl"])
    assert len(BC.tile_order(c["mdl"].dims[:-1])) == trips
    with _ctx(box_pencil=1) as k:
        for tile, want in ((0, 0), (1, trips), (-1, 0)):
            for grid in (0, 8):
                k.set_option("box_tile", tile)
                k.set_option("grid_blocks", grid)
                k.set_matrix_box(c["mdl"], store=False)
                assert k.layout_info()["format"] == 7, (name, tile, grid, k.layout_info())
                assert k.build_info()["pencil_order"] == want, (name, tile, k.build_info())
                _same(_product(k, c["x"], 1), c["y"], f"{name}, box_tile={tile}, grid_blocks={grid}")


def test_order_of_a_larger_box_does_not_survive():
    """one context, box_tile = 1: 64 base trips, then 32 (its own order, of its own length), then a plane of two species
    (no order to give), then the first again with box_tile = 0"""
    seq = [("slab_8x8x8x8x2x2", 1, 64), ("tile_small_8x8x8x4x2x2", 1, 32), ("decode_49x4x3", 1, 0), ("slab_8x8x8x8x2x2", 0, 0)]
    with _ctx(box_pencil=1) as k:
        for name, tile, want in seq:
            c = BC.gated_case(name) if name in BC.SLAB or name in BC.TILE else BC.case(name)
            k.set_option("box_tile", tile)
            k.set_matrix_box(c["mdl"], store=False)
            assert k.layout_info()["format"] == 7
            assert k.build_info()["pencil_order"] == want == (len(BC.tile_order(c["mdl"].dims[:-1])) if tile else 0), (name, k.build_info())
            _same(_product(k, c["x"], 1), c["y"], f"{name} in sequence, box_tile={tile}")


def test_arnoldi_pass_through_ordered_pencils():
    """the fused modes of k_spmv_pencil with the order on"""
    case = K.box_case("tile_order")
    with _ctx(box_pencil=1, box_tile=1) as c:
        case.upload(c)
        assert c.layout_info()["format"] == 7 and c.build_info()["pencil_order"] == 64
        r, _, _ = _whole_pass(c, case)
    print(f"\nordered pencils: {K.fmt(r)}")
    K.assert_ok(r, "format 7 with a base-trip order")
