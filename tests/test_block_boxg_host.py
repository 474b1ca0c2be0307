"""Option block_box = 2 (the generic matrix-free block kernels), the part that needs no GPU: the host-side descriptor check
box_generic_image runs under AddressSanitizer / UBSan in a stand-alone program; the new kernels are in the build, hidden
from the library's surface, and the option is documented where the others are."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_host_check_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "boxg_host_check")
    src = os.path.join(ROOT, "tests", "boxg_host_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_kernels_are_built_and_hidden(golden_dir):
    from krylovfspssa_amd import build
    assert "kfsp_block_boxg.hip" in build.SOURCES and "kfsp_boxg_dev.h" in build.HEADERS
    lib = build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split())
    before = open(os.path.join(golden_dir, "exported_kfsp_symbols.txt")).read().split()
    assert [s for s in names if s.startswith("kfsp_")] == before          # no entry point was added
    for s in names:
        assert not any(t in s for t in ("spmm_boxg", "box_generic_image")), s


def test_the_value_is_documented():
    hdr = open(os.path.join(ROOT, "include", "kfsp.h")).read()
    assert '"block_box" = 2' in hdr
    for doc in ("README.md", "DESIGN.md"):
        assert "block_box = 2" in open(os.path.join(ROOT, doc)).read(), doc
    assert "block_box\", 2" in open(os.path.join(ROOT, "krylovfspssa_amd", "host.py")).read()
