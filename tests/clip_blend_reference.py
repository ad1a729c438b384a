"""The cross-fade rule of clip_rule.h (clip_blend_record, clip_blend_weight) restated in numpy: float64 / float32 scalars, plain
IEEE operations in the same operand order, no fused multiply-add, sqrt and division correctly rounded. Nothing here needs a GPU
or the library."""
import numpy as np

F64, F32 = np.float64, np.float32
PARTS = (("translation", 3), ("rotation", 4), ("scale", 3))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _normalise(r):
    """clip_normalise: the length as sqrt(((x x + y y) + z z) + w w); the division only where it is > 0."""
    length = np.sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
    return [c / length for c in r] if length > F64(0.0) else r


def blend_record(a, b, weight):
    """Two abi.NODE_TRS records (numpy void scalars) and the share of b as float32 -> the blended record."""
    w = F64(F32(weight))
    out = a.copy()
    if w == 0.0:
        return out
    if w == 1.0:
        return b.copy()
    mask = int(a["animated"]) | int(b["animated"])
    if mask == 0:
        return out
    with np.errstate(all="ignore"):
        for name, n in PARTS:
            if np.array_equal(_bits(a[name]), _bits(b[name])):
                continue                                                     # copied from a
            x, y = [F64(v) for v in a[name]], [F64(v) for v in b[name]]
            if name == "rotation" and ((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3] < 0.0:
                y = [-v for v in y]
            r = [x[c] + w * (y[c] - x[c]) for c in range(n)]
            if name == "rotation":
                r = _normalise(r)
            out[name] = np.array([F32(v) for v in r], np.float32)
    out["animated"] = mask
    return out


def blend_records(trs_a, trs_b, weight):
    out = trs_a.copy()
    for n in range(len(trs_a)):
        out[n] = blend_record(trs_a[n], trs_b[n], weight)
    return out


def blend_weights(wa, wb, weight):
    """Two float32 weight vectors and the share of the second -> the blended weights."""
    w = F64(F32(weight))
    wa, wb = np.ascontiguousarray(wa, np.float32), np.ascontiguousarray(wb, np.float32)
    out = wa.copy()
    with np.errstate(all="ignore"):
        for k in range(len(wa)):
            if w == 0.0 or _bits(wa[k:k + 1])[0] == _bits(wb[k:k + 1])[0]:
                continue
            out[k] = wb[k] if w == 1.0 else F32(F64(wa[k]) + w * (F64(wb[k]) - F64(wa[k])))
    return out
