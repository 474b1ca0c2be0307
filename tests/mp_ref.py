"""TEST HELPER - correctly rounded values of pow and the 14 library functions of the propensity program (include/kfsp.h
opcodes 7 and 11 .. 24), from mpmath at 100 digits rounded to the nearest double.

Each expression has two species and exactly ONE library call whose argument is exact in binary64 (a sum, difference or
product of populations up to 9 999, scaled by a power of two where the function's domain asks for it; pow takes an immediate
exponent, which is the double it is), so the only rounding between the populations and the result is the function's own and
the device's value can be held to the correctly rounded one.  The rules that make a whole expression 0 (log / log10 of
x <= 0, sqrt of x < 0, asin / acos outside [-1, 1], x / 0) are applied here as the header states them."""
import mpmath

import numpy as np

IMM, NEG, ADD, SUB, MUL, DIV, POW = 1, 2, 3, 4, 5, 6, 7
X, Y = 101, 102

SUM = ([X, Y, ADD], [], lambda x, y: x + y)
DIFF = ([X, Y, SUB], [], lambda x, y: x - y)
PROD = ([X, Y, MUL], [], lambda x, y: x * y)


def _scaled(p):
    """(x - y) 2^-p"""
    return [X, Y, SUB, IMM, MUL], [2.0 ** -p], lambda x, y: (x - y) * 2.0 ** -p


def _domain(lo_open=None, lo=None, absmax=None):
    def ok(a):
        return not ((lo_open is not None and a <= lo_open) or (lo is not None and a < lo) or (absmax is not None and abs(a) > absmax))
    return ok


ANY = _domain()

# name -> (function opcode, argument, mpmath function, the arguments the header's rules let through)
UNARY = {
    "abs": (11, DIFF, abs, ANY),
    "exp": (12, _scaled(4), mpmath.exp, ANY),
    "log10": (13, SUM, mpmath.log10, _domain(lo_open=0.0)),
    "log": (14, DIFF, mpmath.log, _domain(lo_open=0.0)),
    "sqrt": (15, DIFF, mpmath.sqrt, _domain(lo=0.0)),
    "sinh": (16, _scaled(4), mpmath.sinh, ANY),
    "cosh": (17, _scaled(4), mpmath.cosh, ANY),
    "tanh": (18, _scaled(10), mpmath.tanh, ANY),
    "sin": (19, SUM, mpmath.sin, ANY),
    "cos": (20, PROD, mpmath.cos, ANY),
    "tan": (21, SUM, mpmath.tan, ANY),
    "asin": (22, _scaled(13), mpmath.asin, _domain(absmax=1.0)),
    "acos": (23, _scaled(13), mpmath.acos, _domain(absmax=1.0)),
    "atan": (24, DIFF, mpmath.atan, ANY),
}
POWERS = {"pow 2.5": (SUM, 2.5), "pow -0.5": (([X, Y, MUL, IMM, ADD], [1.0], lambda x, y: x * y + 1.0), -0.5), "pow 0.3": (PROD, 0.3)}


def rounded(f, *args):
    """f at 100 digits, rounded to the nearest double"""
    with mpmath.workprec(340):
        return float(f(*[mpmath.mpf(a) for a in args]))


def expressions():
    """[(name, postfix code, immediates, reference(x, y) -> float)]: the 14 functions, three powers, and log(x + 1) / y
    for the x / 0 rule (one IEEE division after the one library call)"""
    out = []
    for name, (op, (code, imm, arg), f, ok) in UNARY.items():
        out.append((name, code + [op], imm, (lambda x, y, arg=arg, f=f, ok=ok: rounded(f, arg(x, y)) if ok(arg(x, y)) else 0.0)))
    for name, ((code, imm, arg), e) in POWERS.items():
        out.append((name, code + [IMM, POW], imm + [e], (lambda x, y, arg=arg, e=e: rounded(mpmath.power, arg(x, y), e))))
    out.append(("log / y", [X, IMM, ADD, 14, Y, DIV], [1.0],
                lambda x, y: rounded(mpmath.log, x + 1.0) / y if y != 0.0 else 0.0))
    return out


def lattice():
    """40 populations from 0 to 9 999 - the ends, the small ones, powers of two and their neighbours, the rest spread out -
    and the 1 600 states of their square"""
    v = [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 63, 64, 100, 127, 128, 255, 256, 511, 512, 777, 1000, 1023, 1024,
         2047, 2048, 3000, 4095, 4096, 5000, 6434, 8191, 8192, 9998, 9999]
    assert len(v) == 40 == len(set(v))
    return np.array([(a, b) for a in v for b in v], dtype=np.int32)


def reference(states):
    """[len(states)][number of expressions]"""
    ex = expressions()
    out = np.zeros((len(states), len(ex)))
    for i, (x, y) in enumerate(np.asarray(states).tolist()):
        for j, (_, _, _, ref) in enumerate(ex):
            out[i, j] = ref(float(x), float(y))
    return out
