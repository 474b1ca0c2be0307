"""The host rules of generator replacement - banded_pays and want_state_order (csrc/kfsp_host.h), one function each
where there were two and three copies - and the one reset of what is resident (GeneratorState, csrc/kfsp_ctx.h), in a
stand-alone program under AddressSanitizer / UBSan against literal restatements of the code they replaced
(tests/generator_rule_check.cpp); and the source list: replacing the generator is a translation unit of its own."""
import os
import re
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


def test_generator_rules_under_asan_ubsan(tmp_path):
    from krylovfspssa_amd import build
    exe = str(tmp_path / "generator_rule_check")
    src = os.path.join(ROOT, "tests", "generator_rule_check.cpp")
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_generator_source_is_built():
    from krylovfspssa_amd import build
    assert "kfsp_generator.cpp" in build.SOURCES
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in build.SOURCES + build.HEADERS)


def _code(name):
    """a source file without its comments"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_one_reset_and_no_flag_block_outside_it():
    """What is resident is cleared in ONE place (reset_generator), called from ONE place (begin_generator); the flag blocks
    the paths used to spell out are gone, and the generator entry points live in kfsp_generator.cpp."""
    sources = [f for f in os.listdir(CSRC) if f.endswith((".cpp", ".hip", ".h"))]
    resets = {f: _code(f).count("reset_generator(") for f in sources}
    assert {f: c for f, c in resets.items() if c} == {"kfsp_ctx.h": 1, "kfsp_generator.cpp": 1}
    for f in sources:
        code = _code(f)
        assert "sell_reach = -1" not in code or f in ("kfsp_ctx.h", "kfsp_build.hip")
        for flag in ("use_dia", "have_sell"):
            assert not re.search(r"->%s\s*=\s*false" % flag, code), (f, flag)
    build_hip = _code("kfsp_build.hip")
    # (build_dia_mask, build_dia_code and build_sell_code drop a stale image of their own: one clause each)
    assert len(re.findall(r"->dia_coded\s*=\s*false", build_hip)) == 1
    assert len(re.findall(r"->dia_masked\s*=\s*false", build_hip)) == 1
    assert len(re.findall(r"->sell_coded\s*=\s*false", build_hip)) == 1
    assert build_hip.count("sell_reach = -1") == 1
    api, gen = _code("kfsp_api.cpp"), _code("kfsp_generator.cpp")
    for entry in ("kfsp_set_matrix_ell(", "kfsp_set_matrix_csr(", "kfsp_set_matrix_box(", "kfsp_drop_rebuild("):
        assert "int " + entry in gen and "int " + entry not in api
    assert "build_from_resident_ell" not in api and "finish_generator" not in api
    # the state-order rule and the banded-or-SELL rule: defined once, in kfsp_host.h
    for f in sources:
        if f != "kfsp_host.h":
            assert "prod_count >=" not in _code(f), f
    assert "1.5 *" not in build_hip and "1.5 *" not in gen
    assert "banded_pays(" in build_hip and "banded_pays(" in gen          # both builds ask the one rule
    assert "want_state_order(" in gen and "want_state_order(" in api      # ... and all three callers the other
