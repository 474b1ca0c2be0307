"""The dispatch helpers of the block product (csrc/kfsp_block_dev.h: kp_index, dispatch_kp and its kin) in a stand-alone
program under AddressSanitizer / UBSan: widths 2, 4, 8, 16 map to slots 0 .. 3 and reach the callable as that constant,
anything else as 16 - what the `default:` branches of the switches they replaced did."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_block_dispatch_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_dispatch_check")
    src = os.path.join(ROOT, "tests", "block_dispatch_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
