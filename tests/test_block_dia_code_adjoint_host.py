"""Option block_dia_code_adjoint (the transposed block product on the coded banded image), the part that needs no GPU: the
selection rule (kfsp_host.h) and the index helper the kernel compiles (diac_t_src, kfsp_block_dev.h) run under
AddressSanitizer / UBSan in a stand-alone program; the new kernel is in the build and hidden, the library's surface and
kAbiVersion are what they were, and the option is documented where the others are."""
import ctypes
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")
OPTION = "block_dia_code_adjoint"


def test_host_check_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_dia_code_adjoint_check")
    src = os.path.join(ROOT, "tests", "block_dia_code_adjoint_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_kernel_is_built_and_the_surface_is_unchanged(golden_dir):
    from krylovfspssa_amd import build
    assert "kfsp_block_diac_t.hip" in build.SOURCES
    assert os.path.exists(os.path.join(CSRC, "kfsp_block_diac_t.hip"))
    lib = build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split())
    before = open(os.path.join(golden_dir, "exported_kfsp_symbols.txt")).read().split()
    assert [s for s in names if s.startswith("kfsp_")] == before          # no entry point was added
    for s in names:
        assert not any(t in s for t in ("spmm_diac_t", "block_dia_code_t_path")), s
    assert ctypes.CDLL(lib).kfsp_abi_version() == 2


def test_the_option_is_documented():
    for doc in (os.path.join("include", "kfsp.h"), "README.md", "DESIGN.md", os.path.join("krylovfspssa_amd", "host.py")):
        assert OPTION in open(os.path.join(ROOT, doc)).read(), doc
    assert '"' + OPTION + '"' in open(os.path.join(ROOT, "include", "kfsp.h")).read()
    assert "Coded banded generators, backward" in open(os.path.join(ROOT, "DESIGN.md")).read()
    host = open(os.path.join(ROOT, "krylovfspssa_amd", "host.py")).read()
    assert host.count(OPTION) >= 3          # set_option, spmm, block_info
