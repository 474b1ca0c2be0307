"""The rule of the block product (csrc/kfsp_block_plan.h: block_form, block_plan, block_exchange_mode) and the block state's
record and reset (csrc/kfsp_ctx.h: BlockState) in a stand-alone program under AddressSanitizer / UBSan, against a literal
restatement of the refusal ladder and the branch order they replaced (tests/block_plan_check.cpp); and the split of
kfsp_block.hip into a kernel file and a host file is what the build compiles."""
import os
import re
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_block_plan_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "block_plan_check")
    src = os.path.join(ROOT, "tests", "block_plan_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_split_sources_are_built():
    from krylovfspssa_amd import build
    assert build.SOURCES[-1] == "kfsp_block_host.hip" and "kfsp_block.hip" in build.SOURCES
    assert build.HEADERS[-1] == "kfsp_block_plan.h"
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in build.SOURCES + build.HEADERS)


def test_the_host_file_holds_no_kernel_and_one_writer_per_info_slot():
    host = open(os.path.join(CSRC, "kfsp_block_host.hip")).read()
    kern = open(os.path.join(CSRC, "kfsp_block.hip")).read()
    assert "__global__" not in host and "__device__" not in host
    assert "#pragma clang fp contract(off)" in kern and "hipLaunchKernelGGL" not in kern
    for f in os.listdir(CSRC):                                   # the slots of kfsp_block_info go by name
        assert not re.search(r"blk_info\[[0-9]", open(os.path.join(CSRC, f)).read()), f
    assert host.count("blk_info[kInfoExchange] =") == 1 and host.count("blk_info[kInfoAdjoint] =") == 1
