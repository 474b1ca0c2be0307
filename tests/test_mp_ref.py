"""The correctly rounded reference of the library functions (tests/mp_ref.py) before a GPU is involved: values known exactly,
the rules that zero an expression, and the host's own math library, which is within 1 ulp of it."""
import math

import numpy as np

from tests import mp_ref as M


def test_values_known_exactly_and_the_zero_rules():
    ex = {name: ref for name, _, _, ref in M.expressions()}
    assert len(ex) == 18
    assert ex["abs"](3.0, 10.0) == 7.0 and ex["sqrt"](25.0, 9.0) == 4.0 and ex["sqrt"](9.0, 9.0) == 0.0 and ex["sqrt"](9.0, 10.0) == 0.0
    assert ex["exp"](5.0, 5.0) == 1.0 and ex["log"](8.0, 7.0) == 0.0 and ex["log"](7.0, 7.0) == 0.0 and ex["log"](7.0, 8.0) == 0.0
    assert ex["log10"](600.0, 400.0) == 3.0 and ex["log10"](0.0, 0.0) == 0.0
    assert ex["pow 2.5"](3.0, 1.0) == 32.0 and ex["pow -0.5"](3.0, 5.0) == 0.25 and ex["pow 2.5"](0.0, 0.0) == 0.0
    assert ex["asin"](8192.0, 0.0) == math.pi / 2 and ex["asin"](8193.0, 0.0) == 0.0 and ex["acos"](0.0, 8193.0) == 0.0
    assert ex["acos"](0.0, 8192.0) == math.pi and ex["atan"](4.0, 4.0) == 0.0 and ex["log / y"](5.0, 0.0) == 0.0
    assert ex["log / y"](0.0, 3.0) == 0.0 and ex["cosh"](2.0, 2.0) == 1.0 and ex["tanh"](9999.0, 0.0) == math.tanh(9999.0 / 1024.0)


def test_host_math_library_is_within_one_ulp_of_it():
    states = M.lattice()[::7]
    ref = M.reference(states)
    host = {"exp": lambda x, y: math.exp((x - y) / 16.0), "sin": lambda x, y: math.sin(x + y), "cos": lambda x, y: math.cos(x * y),
            "atan": lambda x, y: math.atan(x - y), "pow 2.5": lambda x, y: (x + y) ** 2.5, "log10": lambda x, y: math.log10(x + y) if x + y > 0 else 0.0}
    names = [e[0] for e in M.expressions()]
    assert np.isfinite(ref).all()
    for name, f in host.items():
        j = names.index(name)
        for (x, y), want in zip(states.tolist(), ref[:, j]):
            got = f(float(x), float(y))
            assert abs(got - want) <= np.spacing(abs(want)), (name, x, y, got, want)
