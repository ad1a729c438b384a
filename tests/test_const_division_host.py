"""The three-operation form of x / C that rt_device.h's div_small_int_exact uses, against IEEE fp32 division, over the whole
domain of every call site: each byte / 255, each signed byte / 127, each signed half / 32767. No GPU: fp32 multiply and fma are
modelled with exact rationals and one round-to-nearest-even, so nothing here depends on the host's float unit or on double rounding.

    r = RN(1 / C);  q = RN(x * r);  rem = RN(-C * q + x);  result = RN(rem * r + q)
"""
from fractions import Fraction

import numpy as np
import pytest


def rn32(v):
    """Fraction -> the nearest fp32 value (ties to even), as a Fraction. Normal and subnormal range; no overflow here."""
    if v == 0:
        return Fraction(0)
    s, a = (-1 if v < 0 else 1), abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^(e-1) <= a < 2^(e+1)
    if a < Fraction(2) ** e:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = a / ulp
    k = n.numerator // n.denominator
    frac = n - k
    if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and (k & 1)):
        k += 1
    return s * k * ulp


def three_op(x, c):
    c, x = Fraction(c), Fraction(x)
    r = rn32(1 / c)
    q = rn32(x * r)
    rem = rn32(-c * q + x)            # one fma: a single rounding of the exact value
    return rn32(rem * r + q)


def test_rn32_agrees_with_numpy_on_representative_values():
    # the fp64 quotient of two fp32 values rounds to fp32 without a double-rounding error (53 >= 2 * 24 + 2)
    for num, den in ((1, 3), (2, 3), (1, 255), (254, 255), (-127, 127), (32766, 32767), (1, 32767), (-5, 7)):
        assert float(rn32(Fraction(num, den))) == float(np.float32(np.float64(num) / np.float64(den)))
    assert rn32(Fraction(16777217)) == 16777216 and rn32(Fraction(16777219)) == 16777220      # ties to even
    assert rn32(Fraction(1, 2 ** 149)) == Fraction(1, 2 ** 149) and rn32(Fraction(1, 2 ** 151)) == 0


@pytest.mark.parametrize("c,lo,hi", [(255, 0, 256), (127, -128, 128), (32767, -32768, 32768)])
def test_three_operation_quotient_is_the_ieee_quotient_on_the_whole_domain(c, lo, hi):
    xs = np.arange(lo, hi, dtype=np.int64)
    ieee = (xs.astype(np.float32) / np.float32(c)).astype(np.float32)            # numpy's fp32 division is IEEE
    bad = []
    for x, w in zip(xs.tolist(), ieee.tolist()):
        exact_rn = rn32(Fraction(x, c))
        got = three_op(x, c)
        if got != exact_rn or float(got) != w:
            bad.append((x, float(got), float(exact_rn), w))
    assert not bad, "x / %d: %d mismatches, first %s" % (c, len(bad), bad[:3])


@pytest.mark.parametrize("c", [255, 127, 32767])
def test_zero_keeps_its_sign(c):
    """0 / C is +0 in IEEE; the three operations give 0 * r = +0, fma(-C, +0, +0) = +0, fma(+0, r, +0) = +0 (an exact zero sum of
    opposite signs is +0 under round-to-nearest), so the form cannot produce -0 where the division gives +0."""
    r = np.float32(1.0) / np.float32(c)
    q = np.float32(0.0) * r
    rem = np.float32(-np.float32(c) * q) + np.float32(0.0)
    out = np.float32(rem * r) + q
    assert out == 0.0 and not np.signbit(out)
