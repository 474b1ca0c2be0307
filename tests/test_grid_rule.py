"""The launch rule of the generator product (csrc/kfsp_host.h: product_trips, product_grid) against a restatement of
the formulas its callers used to write out, in a stand-alone program under AddressSanitizer / UBSan: equal wherever
the old value fitted a slot of 2048 block partials, exactly 2048 wherever it did not."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_grid_rule_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "grid_rule_check")
    src = os.path.join(ROOT, "tests", "grid_rule_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
