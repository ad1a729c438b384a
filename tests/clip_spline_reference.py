"""The CUBICSPLINE rule of glTF 2.0 (appendix C) in exact arithmetic, for the tests of the library's cubic sampling. It knows the
file's layout (per key an in-tangent, a value, an out-tangent) and the specification's formula, not the library's grouping:
rationals (fractions.Fraction) from the fp32 keys for the fraction and the Hermite sum, decimal at 60 digits for a rotation's
normalisation. Nothing here needs the library or a GPU."""
import decimal
from fractions import Fraction

import numpy as np

decimal.getcontext().prec = 60


def frac(x):
    return Fraction(float(x))          # an fp32 or fp64 value is a rational; exact


def locate(times, time):
    """-> (key i, fraction u as a Fraction, td as a Fraction): clamped below the first and above the last key, u == 0 at a key."""
    t = frac(time)
    ts = [frac(x) for x in times]
    if t <= ts[0]:
        return 0, Fraction(0), Fraction(0)
    if t >= ts[-1]:
        return len(ts) - 1, Fraction(0), Fraction(0)
    i = max(k for k in range(len(ts) - 1) if ts[k] <= t)
    td = ts[i + 1] - ts[i]
    return i, (t - ts[i]) / td, td


def hermite(times, rows, time):
    """rows: [3 * n_keys, comps] float32 as the file holds them. -> (exact values [comps] as Fractions, S [comps]: the sum of the
    absolute values of the four exact products, 0 where the sample is a key's value)."""
    rows = np.asarray(rows, np.float32)
    comps = rows.shape[1]
    i, u, td = locate(times, time)
    if u == 0:
        return [frac(rows[3 * i + 1, c]) for c in range(comps)], [Fraction(0)] * comps
    u2, u3 = u * u, u * u * u
    h00, h10, h01, h11 = 2 * u3 - 3 * u2 + 1, u3 - 2 * u2 + u, -2 * u3 + 3 * u2, u3 - u2
    out, scale = [], []
    for c in range(comps):
        v0, b0 = frac(rows[3 * i + 1, c]), frac(rows[3 * i + 2, c])
        a1, v1 = frac(rows[3 * i + 3, c]), frac(rows[3 * i + 4, c])
        terms = (h00 * v0, h10 * td * b0, h01 * v1, h11 * td * a1)
        out.append(sum(terms))
        scale.append(sum(abs(x) for x in terms))
    return out, scale


def to_decimal(x):
    return decimal.Decimal(x.numerator) / decimal.Decimal(x.denominator)


def normalised(q):
    """A quaternion of Fractions -> its normalisation as Decimals (60 digits); the zero quaternion stays zero."""
    n2 = sum(x * x for x in q)
    if n2 == 0:
        return [decimal.Decimal(0)] * 4
    length = to_decimal(n2).sqrt()
    return [to_decimal(x) / length for x in q]


def round_f32(x):
    """The correctly rounded fp32 of an exact value (Fraction or Decimal): through the nearest double would round twice, so the
    two fp32 neighbours of that double are compared exactly."""
    x = Fraction(x) if not isinstance(x, Fraction) else x
    near = np.float32(float(x))
    best = near
    for cand in (np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))):
        da, db = abs(frac(cand) - x), abs(frac(best) - x)
        if da < db or (da == db and (int(np.float32(cand).view(np.uint32)) & 1) == 0 and (int(np.float32(best).view(np.uint32)) & 1) == 1):
            best = cand
    return np.float32(best)


def ulp(x):
    """The spacing of fp32 at |x| (the least subnormal's at 0)."""
    a = np.abs(np.float32(float(x)))
    return float(np.nextafter(a, np.float32(np.inf)) - a)


def check_component(got, exact, scale, extra_ulps=0):
    """The tests' bound on one component. -> True where `got` is the correctly rounded value; asserts the bound otherwise: within
    half an fp32 ulp of the exact value plus 2^-48 * S (at most 16 double roundings of 2^-53 relative to a partial sum no larger
    than S), plus `extra_ulps` fp32 ulps (a rotation after its normalisation)."""
    exact = Fraction(exact)
    want = round_f32(exact)
    if np.float32(got).view(np.uint32) == want.view(np.uint32) or (float(got) == 0.0 and float(want) == 0.0):
        return True
    bound = Fraction(ulp(exact)) * (Fraction(1, 2) + extra_ulps) + Fraction(1, 2 ** 48) * Fraction(scale)
    assert abs(frac(got) - exact) <= bound, (float(got), float(exact), float(bound))
    return False


def check_sample(got, times, rows, time, rotation=False):
    """One sample of a channel against the rule -> (components that are the correctly rounded value, components compared)."""
    exact, scale = hermite(times, rows, time)
    if not rotation:
        ok = [check_component(g, e, s) for g, e, s in zip(got, exact, scale)]
        return sum(ok), len(ok)
    n2 = sum(x * x for x in exact)
    want = normalised(exact)
    if n2 == 0:
        assert all(float(g) == 0.0 for g in got), got
        return 4, 4
    # The unnormalised sum is not rounded to fp32, so its part of the bound is 2^-48 * S per component. A component of q / |q|
    # moves by at most 1 / |q| per unit of error in any of the four components, so the four parts add up, divided by |q|; the
    # normalisation's own sqrt and divisions in double and the one rounding to fp32 stay within the one more fp32 ulp.
    carried = Fraction(to_decimal(sum(scale)) / to_decimal(n2).sqrt())
    ok = [check_component(g, Fraction(w), carried, extra_ulps=1) for g, w in zip(got, want)]
    return sum(ok), len(ok)
