"""The lane path of the folded banded product (csrc/kfsp_dia_diag.h: dia_lanes_trip, dia_lanes_edge, dia_xpair_clamp;
DESIGN.md 4.1e) in a stand-alone program under AddressSanitizer / UBSan (tests/dia_lanes_check.cpp): no device, no library.
The program plays one wavefront per 128-row trip with the header's own functions - the ones the kernel calls - on an x of
exactly n + 2 doubles: where the rule admits the lane path every +-1 operand named by the lane mapping is the word ld_xpair
would read and no clamp acts; where it refuses, the trip holds row `last` or the padding; at most one trip per generator
is refused."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from krylovfspssa_amd import build
    out = str(tmp_path_factory.mktemp("dia_lanes") / "dia_lanes_check")
    src = os.path.join(ROOT, "tests", "dia_lanes_check.cpp")
    # a host program only (-x c++): the sanitizers never reach device code
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-I" + CSRC, "-fno-gpu-sanitize", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_lane_mapping_and_rule_on_every_trip(exe):
    r = subprocess.run([exe, "1", "1100"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    word, trips, admitted, refused = r.stdout.split()
    assert word == "ok"
    # restated: a banded product takes ceil(ceil(n / 64) / 2) trips; all are admitted but a partial last one
    ns = range(1, 1101)
    want_trips = sum((-(-n // 64) + 1) // 2 for n in ns)
    want_refused = sum(1 for n in ns if n % 128)
    assert (int(trips), int(admitted), int(refused)) == (want_trips, want_trips - want_refused, want_refused)
    assert all((-(-n // 64) + 1) // 2 == -(-n // 128) for n in ns)
