"""The interior trips of the folded banded product (csrc/kfsp_dia_diag.h: dia_inner_trip, dia_inner_base, dia_xpair_clamp;
DESIGN.md 4.1e) in a stand-alone program under AddressSanitizer / UBSan (tests/dia_inner_check.cpp): no device, no library.
The program plays one wavefront per 128-row trip with the header's own functions - the ones the kernel calls - on an x of
exactly n + 2 doubles: an admitted trip reads, through the uniform-base-plus-lane-offset mapping, exactly the words ld_xpair
reads, no clamp acts and it holds no row of the padding; the refused trips are exactly those in which some lane's clamp or
padding flag acts; the rule admits a trip once n >= 2 dmax + 384."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "krylovfspssa_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from krylovfspssa_amd import build
    out = str(tmp_path_factory.mktemp("dia_inner") / "dia_inner_check")
    src = os.path.join(ROOT, "tests", "dia_inner_check.cpp")
    # a host program only (-x c++): the sanitizers never reach device code
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-I" + CSRC, "-fno-gpu-sanitize", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


def test_interior_rule_and_mapping_on_every_trip(exe):
    r = subprocess.run([exe, "1", "1100"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    word, trips, admitted, refused = r.stdout.split()
    assert word == "ok"
    # restated without the header: trip c of n rows with offsets in [dmin, dmax] is interior iff its first pair index is not
    # below -1, its last row is a row (128 c + 127 <= n - 1) and its last pair index is not above n - 1
    sets = []
    for s in (2, 3, 7, 16, 31):
        sets.append((-s, s))
        sets += [(-s * t, s * t) for t in (2, 5)]
    want_trips = want_admitted = 0
    for n in range(1, 1101):
        t = -(-n // 128)
        for dmin, dmax in sets:
            want_trips += t
            want_admitted += sum(1 for c in range(t) if 128 * c + dmin >= -1 and 128 * c + 127 <= n - 1 and 128 * c + 126 + dmax <= n - 1)
    assert (int(trips), int(admitted), int(refused)) == (want_trips, want_admitted, want_trips - want_admitted)
    assert want_admitted > 0
