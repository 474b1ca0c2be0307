"""Option block_dia_code (the block product on the coded banded image), the part that needs no GPU: the selection rule
(kfsp_host.h), dispatch_diac and the record decode the kernel compiles (kfsp_block_dev.h) run under AddressSanitizer / UBSan
in a stand-alone program; the new kernels are in the build and hidden, the library's surface and kAbiVersion are what they
were, and the option is documented where the others are."""
import ctypes
import os
import re
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_host_check_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_dia_code_check")
    src = os.path.join(ROOT, "tests", "block_dia_code_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_kernels_are_built_and_the_surface_is_unchanged(golden_dir):
    from krylovfspssa_amd import build
    assert "kfsp_block_diac.hip" in build.SOURCES
    lib = build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    names = sorted(line.split()[-1] for line in out.splitlines() if line.split())
    before = open(os.path.join(golden_dir, "exported_kfsp_symbols.txt")).read().split()
    assert [s for s in names if s.startswith("kfsp_")] == before          # no entry point was added
    for s in names:
        assert not any(t in s for t in ("spmm_diac", "dispatch_diac", "block_dia_code_path")), s
    # ... and the ABI number stays: nothing a caller links against changed
    api = open(os.path.join(CSRC, "kfsp_api.cpp")).read()
    assert re.search(r"constexpr int kAbiVersion = 2;", api)
    assert ctypes.CDLL(lib).kfsp_abi_version() == 2
    # one copy of the single-vector rule, shared by both translation units
    assert api.count("dia_code_on(const kfsp_ctx") == 0
    assert open(os.path.join(CSRC, "kfsp_host.h")).read().count("inline bool dia_code_on(const kfsp_ctx") == 1


def test_the_option_is_documented():
    hdr = open(os.path.join(ROOT, "include", "kfsp.h")).read()
    assert '"block_dia_code"' in hdr
    for doc in ("README.md", "DESIGN.md", os.path.join("profiles", "README.md")):
        assert "block_dia_code" in open(os.path.join(ROOT, doc)).read(), doc
    assert "Coded banded generators (`block_dia_code`)" in open(os.path.join(ROOT, "DESIGN.md")).read()
    host = open(os.path.join(ROOT, "krylovfspssa_amd", "host.py")).read()
    assert host.count("block_dia_code") >= 3          # set_option, spmm, block_info
