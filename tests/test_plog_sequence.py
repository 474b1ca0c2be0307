"""The fixed-sequence logarithm of the independent-stream SSA walk (KFSP_PLOG in krylovfspssa_amd/fortran/kfsp_statespace.f90 =
plog in krylovfspssa_amd/csrc/kfsp_ssa.hip): the waiting times of that opt-in mode are DEFINED through it, so that host and
device produce the same bits (tests/test_fortran_host.py::test_device_ssa_walk_equals_the_host_walk checks that on the GPU).
Here, on the CPU, the same sequence of IEEE operations restated in Python floats (no contraction) is held against math.log:
it must be a logarithm to ~1e-16 on the whole range of the generator's uniform numbers, monotone, and exact at 1."""
import math

import numpy as np

from tests.ssa_ref import plog


def test_fixed_sequence_logarithm_is_a_logarithm():
    rng = np.random.default_rng(2026)
    xs = np.concatenate([rng.random(200000), 2.0 ** -rng.integers(1, 54, 2000) * (1.0 + rng.random(2000)) / 2.0,
                         [2.0 ** -54, 0.5, 0.70710678118654746, 0.70710678118654757, 1.0 - 2.0 ** -53, 1.0]])
    xs = xs[(xs > 0.0) & (xs <= 1.0)]
    worst = 0.0
    for x in xs.tolist():
        got, want = plog(x), math.log(x)
        if want == 0.0:
            assert got == 0.0
            continue
        # relative to |log x|, except next to 1 where |log x| ~ 1 - x and an absolute ulp of the argument is the scale
        err = abs(got - want) / max(abs(want), 2.0 ** -53)
        worst = max(worst, err)
    assert worst < 4.5e-16, worst
    grid = np.sort(rng.random(20000))
    vals = [plog(x) for x in grid.tolist()]
    assert all(b >= a for a, b in zip(vals, vals[1:]))          # monotone: a larger uniform number never waits longer
    assert plog(1.0) == 0.0 and plog(0.5) == -(6.93147180369123816490e-01 + 1.90821492927058770002e-10)
