"""The CPU side of tests/test_gpu_box_slab_waves.py and tests/test_gpu_nt_loads.py: that the shapes of tests/box_cases.py
and tests/krylov_ref.py reach the kernel variants they are there for - by the host's rules restated (the slab geometry
of box_plan, kfsp_box_plan.h, and the streaming grid of kfsp_host.h) -, box_tile_order itself in a stand-alone program
under AddressSanitizer / UBSan against the restatement in box_cases, and that every option kfsp_set_option stores is
read somewhere."""
import glob
import os
import re
import subprocess

import numpy as np

from tests import box_cases as BC
from tests import krylov_ref as K
from tests import row_cases as RC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_slab_boxes_reach_narrow_ragged_and_several_groups():
    seen = {}
    for name in BC.SLAB:
        mdl = BC.model(name)
        assert BC.instance_of(mdl) == (6, 2) and BC.pencil_format(mdl, 2) == 8 and BC.pencil_format(mdl, 1) == 7
        assert int(np.prod(mdl.dims[:-2])) % 2 == 0
        for w in BC.SLAB_WAVES + (12,):
            lines, groups, waves, lo_trips = BC.slab_geometry(mdl.dims, w)
            assert 1 <= waves <= min(w, 12) and groups * waves >= lines > (groups - 1) * waves
            seen[(name, w)] = (lines, groups, waves, lo_trips)
    widths = {g[2] for g in seen.values()}
    assert {1, 2, 3, 5, 11} <= widths                                     # 22 lines in two workgroups of 11
    assert seen[("slab_8x8x8x8x2x2", 12)][1:3] == (1, 2) and seen[("slab_8x8x8x4x3x2", 12)][1:3] == (1, 3)   # no option needed
    assert seen[("slab_8x8x8x4x3x2", 2)][:3] == (3, 2, 2)                 # a ragged last group: one line for two wavefronts
    assert any(l % w != 0 and g > 1 for l, g, w, _ in seen.values())
    assert seen[("slab_6x4x3x2x22x3", 5)][:3] == (22, 5, 5) and seen[("slab_6x4x3x2x22x3", 3)][:3] == (22, 8, 3)
    # lines of 3000 rows: 24 trips, the last with 56 live rows; 144 rows: two trips, the second with 16
    assert seen[("slab_10x10x6x5x2x2", 1)][3] == 24 and 3000 % 128 == 56 and seen[("slab_6x4x3x2x22x3", 1)][3] == 2


def test_fused_slab_cases_hand_on_more_partials_than_a_wavefront_has_lanes():
    """the prologue of the slab kernel re-adds vec_grid partials; with one wavefront of 64 lanes, 96 of them"""
    dims = {n: K.GATED_BOXES[n][1] for n in ("slab_narrow", "slab_large")}
    n = {k: int(np.prod(d)) for k, d in dims.items()}
    assert n == {"slab_narrow": 12288, "slab_large": 196608}
    assert BC.vec_grid(n["slab_large"]) == 96 > 64 and BC.vec_grid(n["slab_narrow"]) == 6
    for d in dims.values():
        assert BC.slab_geometry(d)[:3] == (3, 1, 3) and [BC.slab_geometry(d, w)[2] for w in (1, 2, 3)] == [1, 2, 3]
    for name in ("repressilator_even", "tile_order"):
        d = K.GATED_BOXES[name][1]
        assert int(np.prod(d[:-2])) % 2 == 0 and d[-2] >= 2
    assert int(np.prod(K.BOX_DIMS["repressilator"][:-2])) % 2 == 1 and int(np.prod(K.BOX_DIMS["birth_death6"][:-2])) % 2 == 0


def test_tiled_orders_are_far_from_ascending():
    moved = {}
    for name in BC.TILED:
        dims = BC.model(name).dims
        o = BC.tile_order(dims[:-1])
        assert sorted(o) == list(range(-(-int(np.prod(dims[:-1])) // 128)))
        moved[name] = (len(o), sum(1 for i, c in enumerate(o) if i != c))
    assert moved == {"slab_8x8x8x8x2x2": (64, 48), "slab_10x10x6x5x2x2": (47, 32), "tile_6x8x8x8x3x2": (72, 48)}
    assert 3000 % 128 != 0                                                 # trips that straddle two lines of the plane
    assert len(BC.tile_order((8, 8, 8, 4, 2))) == 32 and BC.tile_order((49, 4)) == () and BC.tile_order((8, 8, 8, 2, 2)) == ()
    assert BC.instance_of(BC.model("tile_four_slot_8x8x8x4x2x2")) == (6, 4) and BC.pencil_format(BC.model("tile_four_slot_8x8x8x4x2x2"), 1) == 7


def test_conversion_box_takes_the_masked_instantiation():
    """the rule of box_plan (kfsp_box_plan.h) restated: a reaction that moves the slowest species and depends on another one
    makes the pencil kernels mask its entry plane by plane; none of the other gated boxes has one"""
    def simple(mdl):
        st = np.asarray(mdl.stoich)
        return all(deps[0] == mdl.d - 1 or st[mdl.d - 1, k] == 0 for k, deps in enumerate(mdl.deps))
    conv = BC.model("tile_conversion_8x8x8x4x2x3")
    assert not simple(conv) and BC.instance_of(conv) == (6, 4) and BC.pencil_format(conv, 1) == 7 and BC.pencil_format(conv, 2) == 8
    assert len(BC.tile_order(conv.dims[:-1])) == 32 and BC.slab_geometry(conv.dims)[:3] == (2, 1, 2)
    assert all(simple(BC.model(n)) for n in list(BC.SLAB) + list(BC.TILE) if n != "tile_conversion_8x8x8x4x2x3")


def test_box_tile_order_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "box_tile_order_check")
    src = os.path.join(ROOT, "tests", "box_tile_order_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
    for dims in [(8, 8, 8, 8, 2), (10, 10, 6, 5, 2), (6, 8, 8, 8, 3), (8, 8, 8, 4, 2), (8, 8, 8, 2, 2), (49, 4), (2048, 3, 5)]:
        for force in (1, 0):
            r = subprocess.run([exe, str(force)] + [str(d) for d in dims], capture_output=True, text=True)
            assert r.returncode == 0, r.stdout + r.stderr
            got = tuple(int(t) for t in r.stdout.split())
            assert got == (BC.tile_order(dims) if force else ()), (dims, force)


def test_split_partition_case_keeps_64_trips_clear_of_the_strips():
    """product_split (kfsp_host.h) restated for the two row blocks of row_cases.CSR_SPLIT under overlap = 2"""
    from krylovfspssa_amd import host
    a, b = map(int, RC.CSR_SPLIT.split()[-1].split("x"))
    n, H = a * b, a
    for rank in (0, 1):
        _, nloc, L = host.partition(n, 2, rank)
        trips = -(-(-(-nloc // 64)) // 2)
        lo, hi = -(-H // 128), min((L - H) // 128, trips)
        assert hi - lo >= 64, (rank, lo, hi)


def test_every_option_the_library_stores_is_read_somewhere():
    """kfsp_set_option: every name sets one member of the context; that member must occur in csrc/ beyond its
    declaration (kfsp_ctx.h) and its setter - an option that is stored and never read does nothing"""
    api = open(os.path.join(CSRC, "kfsp_api.cpp")).read()
    setter = api[api.index("int kfsp_set_option("):]
    setter = setter[:setter.index("\n}\n")]
    members = {}
    for name, body in re.findall(r'k == "([a-z_0-9]+)"\)(.*?)(?=else if \(k == |else return fail)', setter, flags=re.S):
        stored = re.findall(r"ctx->(opt_\w+) = value", body)
        assert len(stored) == 1, (name, body)
        members[name] = stored[0]
    assert len(members) == len(re.findall(r'k == "', setter)) >= 40
    text = {p: open(p).read() for p in glob.glob(os.path.join(CSRC, "*")) if p.endswith((".cpp", ".hip", ".h"))}
    inert = []
    for name, member in members.items():
        uses = sum(len(re.findall(rf"\b{member}\b", t)) for t in text.values())
        declared = len(re.findall(rf"\b{member}\b\s*=[^=;]*;", text[os.path.join(CSRC, "kfsp_ctx.h")]))
        stored = len(re.findall(rf"ctx->{member} = value", setter))
        if member == "opt_mmax":
            stored += len(re.findall(r"value != ctx->opt_mmax", setter))      # (the setter's own comparison is no use of it)
        if uses - declared - stored < 1:
            inert.append(name)
    assert not inert, f"stored and never read: {inert}"
