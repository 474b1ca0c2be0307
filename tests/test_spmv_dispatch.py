"""What chooses the single-vector product's kernel on the host - dispatch_mode and the box instantiations of
csrc/kfsp_dispatch.h, and dia_code_kernel (csrc/kfsp_dia_diag.h), the one rule for the coded banded kernel that both the
launch and kfsp_dia_code_info read - in a stand-alone program under AddressSanitizer / UBSan, against literal
restatements of the code it replaced (tests/spmv_dispatch_check.cpp)."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_spmv_dispatch_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "spmv_dispatch_check")
    src = os.path.join(ROOT, "tests", "spmv_dispatch_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_split_sources_are_built():
    from krylovfspssa_amd import build
    assert {"kfsp_kernels.hip", "kfsp_spmv_diac.hip", "kfsp_spmv_box.hip"} <= set(build.SOURCES)
    assert {"kfsp_dispatch.h", "kfsp_dev.h", "kfsp_spmv_dev.h"} <= set(build.HEADERS)
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in build.SOURCES + build.HEADERS)
