"""The layer rule of csrc/clip_rule.h restated in numpy float64, independent of the C++: records are twelve uint32 words
(t[3] q[4] s[3], the animated mask, 0); every part is computed in double from the fp32 values with + - * / and sqrt in the
grouping the header writes down, and rounded to fp32 once. IEEE double arithmetic and the fp64 -> fp32 rounding are the same in
numpy as in the library (built without contraction), so the two agree bit for bit."""
import numpy as np

OVERRIDE, ADDITIVE = 0, 1
PARTS = ((0, 3), (3, 4), (7, 3))        # first word and length of translation, rotation, scale


def words(trs):
    """abi.NODE_TRS records -> uint32 [n, 12]."""
    return np.ascontiguousarray(trs).view(np.uint32).reshape(-1, 12).copy()


def f64(w):
    return w.view(np.float32).astype(np.float64)


def f32_words(x):
    return np.asarray(x, np.float64).astype(np.float32).view(np.uint32)


def normalise(q):
    length = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / length if length > 0.0 else q


def quat_mul(p, q):
    """Hamilton product, (x, y, z, w), each component's four terms summed left to right."""
    return np.array([((p[3] * q[0] + p[0] * q[3]) + p[1] * q[2]) - p[2] * q[1],
                     ((p[3] * q[1] - p[0] * q[2]) + p[1] * q[3]) + p[2] * q[0],
                     ((p[3] * q[2] + p[0] * q[1]) - p[1] * q[0]) + p[2] * q[3],
                     ((p[3] * q[3] - p[0] * q[0]) - p[1] * q[1]) - p[2] * q[2]], np.float64)


def blend_record(a, b, w):
    """The cross-fade of two records at the share w of b (clip_blend_record)."""
    mask = a[10] | b[10]
    if w == 0.0 or w == 1.0 or mask == 0:
        return (b if w == 1.0 else a).copy()
    out = a.copy()
    for at, n in PARTS:
        if np.array_equal(a[at:at + n], b[at:at + n]):
            continue
        x, y = f64(a[at:at + n]), f64(b[at:at + n])
        if n == 4 and x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3] < 0.0:
            y = -y
        r = x + w * (y - x)
        out[at:at + n] = f32_words(normalise(r) if n == 4 else r)
    out[10] = mask
    return out


def additive_record(acc, cur, ref, w):
    mask = cur[10] | ref[10]
    if w == 0.0 or mask == 0:
        return acc.copy()
    out = acc.copy()
    for at, n in PARTS:
        if np.array_equal(cur[at:at + n], ref[at:at + n]):
            continue
        a, c, r = f64(acc[at:at + n]), f64(cur[at:at + n]), f64(ref[at:at + n])
        if n == 3:
            out[at:at + n] = f32_words(a + w * (c - r))
            continue
        d = quat_mul(np.array([-r[0], -r[1], -r[2], r[3]]), c)
        if d[3] < 0.0:
            d = -d
        e = normalise(np.array([w * d[0], w * d[1], w * d[2], 1.0 + w * (d[3] - 1.0)]))
        out[at:at + n] = f32_words(normalise(quat_mul(a, e)))
    out[10] = acc[10] | mask
    return out


def layers(cur, rules, ref=None):
    """cur: one abi.NODE_TRS array per layer; rules: (weight, mode, mask float32 [n_nodes] or None) per layer; ref: per layer the
    records at an additive layer's reference time -> uint32 [n_nodes, 12], the final records."""
    cur = [words(c) for c in cur]
    ref = [None if ref is None or r is None else words(r) for r in (ref or [None] * len(cur))]
    out = cur[0].copy()
    for n in range(len(out)):
        acc = cur[0][n]
        for l in range(1, len(cur)):
            weight, mode, mask = rules[l]
            w = float(np.float64(np.float32(weight)) * np.float64(np.float32(1.0) if mask is None else mask[n]))
            acc = additive_record(acc, cur[l][n], ref[l][n], w) if mode == ADDITIVE else blend_record(acc, cur[l][n], w)
        out[n] = acc
    return out
