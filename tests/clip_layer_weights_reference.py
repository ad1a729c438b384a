"""The rule of layered morph weights (clip_rule.h: clip_blend_weight, clip_additive_weight, the effective weight) restated in
pure Python. A Python float is an IEEE double and Python never contracts a * b + c, so each expression below is the rule's, in the
rule's grouping; numpy.float32 does the one rounding per layer. Beside it the exact value of a layer step in fractions.Fraction
and the bound a correctly grouped fp64 evaluation keeps against it. Nothing here needs a GPU or the library."""
from fractions import Fraction

import numpy as np

F32 = np.float32
OVERRIDE, ADDITIVE = 0, 1


def word(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def blend_weight(wa, wb, w):
    """clip_blend_weight: wa, wb float32, w a Python float."""
    if w == 0.0 or word(wa) == word(wb):
        return F32(wa)
    if w == 1.0:
        return F32(wb)
    return F32(float(wa) + w * (float(wb) - float(wa)))


def additive_weight(acc, cur, ref, w):
    """clip_additive_weight."""
    if w == 0.0 or word(cur) == word(ref):
        return F32(acc)
    return F32(float(acc) + w * (float(cur) - float(ref)))


def effective_weight(weight, mask_value):
    """(double)weight * (double)mask_value from the two float32 values: exact."""
    return float(F32(weight)) * float(F32(1.0 if mask_value is None else mask_value))


def layer_weights(cur, rules, ref=None):
    """cur: one float32 vector per layer; rules: (weight, mode, mask value or None) per layer; ref: per layer a vector for an
    additive layer -> the stacked float32 vector, zeros included."""
    n = len(cur[0])
    out = np.zeros(n, F32)
    for k in range(n):
        acc = F32(cur[0][k])
        for l in range(1, len(cur)):
            w = effective_weight(rules[l][0], rules[l][2])
            acc = additive_weight(acc, cur[l][k], ref[l][k], w) if rules[l][1] == ADDITIVE else blend_weight(acc, cur[l][k], w)
        out[k] = acc
    return out


def steps(cur, rules, ref=None):
    """Every layer step of the stack as (acc, cur, x, w, mode, got): the inputs as the rule had them (x: ref for an additive
    layer, acc for an override one) and the rule's float32 result."""
    out = []
    for k in range(len(cur[0])):
        acc = F32(cur[0][k])
        for l in range(1, len(cur)):
            w = effective_weight(rules[l][0], rules[l][2])
            additive = rules[l][1] == ADDITIVE
            got = additive_weight(acc, cur[l][k], ref[l][k], w) if additive else blend_weight(acc, cur[l][k], w)
            out.append((acc, F32(cur[l][k]), F32(ref[l][k]) if additive else acc, w, ADDITIVE if additive else OVERRIDE, got))
            acc = got
    return out


def ulp32(x):
    x = abs(F32(x))
    return float(np.spacing(x if x > 0 else F32(0)))


def step_exact(acc, cur, x, w):
    """acc + w (cur - x), exactly."""
    return Fraction(float(acc)) + Fraction(w) * (Fraction(float(cur)) - Fraction(float(x)))


def step_bound(acc, cur, x, w, got):
    """ulp32(got) / 2 + 2^-51 (|acc| + |w| (|cur| + |x|)): three double roundings (the difference, the product, the sum), each
    at most 2^-53 of its result and so of the sum of magnitudes, then the one rounding to float."""
    return Fraction(ulp32(got)) / 2 + Fraction(1, 2 ** 51) * (abs(Fraction(float(acc))) + abs(Fraction(w)) * (abs(Fraction(float(cur))) + abs(Fraction(float(x)))))
