"""The rules the block path shares with the single-vector path under a row partition (csrc/kfsp_host.h: product_split,
halo_margin, block_margin) against a restatement of the arithmetic run_product wrote out itself, in a stand-alone
program under AddressSanitizer / UBSan: (H, L, trips, trip height, overlap) -> (lo, hi, split?) over a grid that holds
H = L, H > L - trip height, fewer than 64 trips and both trip heights; margins >= H + 128, multiples of 64, never
below the 64 rows a block column has always had."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_block_partition_rules_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_partition_check")
    src = os.path.join(ROOT, "tests", "block_partition_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
