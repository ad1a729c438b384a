"""The DevLight arithmetic restated in numpy float32, from the shader lines csrc/traverse.h cites for the record
(ray_gen_ris.slang:192-210, rt_utils.slang:278-281), not from the library's host function or its kernel. Every numpy float32 ufunc
rounds once and nothing is contracted, so each line below is one IEEE operation per element:

  transform_point(xform, p) = (dot(row0, (p, 1)), dot(row1, (p, 1)), dot(row2, (p, 1))), a 4-term dot product summed left to right
  edge1 = wv1 - wv0, edge2 = wv2 - wv0, c = cross(edge1, edge2)
  length(c) = sqrt((c.x * c.x + c.y * c.y) + c.z * c.z);  area = 0.5 * length(c);  normal = c * (1 / length(c))

Shares no code with the library or with oracle/."""
import numpy as np

F = np.float32
EMISSIVE_TRIANGLE = np.dtype([("v0", "<f4", 4), ("v1", "<f4", 4), ("v2", "<f4", 4), ("emission", "<f4", 4)])
INDIRECTION = np.dtype([("blas_tri_index", "<u4"), ("entity_id", "<u4")])


def _transform_point(M, p):
    """M [n, 3, 4], p [n, 3] -> three float32 arrays: ((m0 * x + m1 * y) + m2 * z) + m3 * 1.0f per row."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return [((M[:, r, 0] * x + M[:, r, 1] * y) + M[:, r, 2] * z) + M[:, r, 3] * F(1.0) for r in range(3)]


def light_table(transforms, entries, triangles):
    """-> [len(entries), 16] float32: world v0 + area | world v1 + normal x | world v2 + normal y | emission rgb + normal z."""
    T = np.asarray(transforms)
    T = np.ascontiguousarray(T["m"] if T.dtype.names else T, dtype=np.float32).reshape(-1, 3, 4)
    e = np.asarray(entries, dtype=INDIRECTION)
    tri = np.asarray(triangles, dtype=EMISSIVE_TRIANGLE)[e["blas_tri_index"].astype(np.int64)]
    M = T[e["entity_id"].astype(np.int64)]
    out = np.zeros((len(e), 16), dtype=np.float32)
    with np.errstate(all="ignore"):
        w = [_transform_point(M, np.ascontiguousarray(tri[k][:, :3])) for k in ("v0", "v1", "v2")]
        e1 = [w[1][c] - w[0][c] for c in range(3)]
        e2 = [w[2][c] - w[0][c] for c in range(3)]
        c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        length = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        r = F(1.0) / length
        for k in range(3):
            for a in range(3):
                out[:, 4 * k + a] = w[k][a]
        out[:, 3] = F(0.5) * length
        out[:, 7], out[:, 11], out[:, 15] = c[0] * r, c[1] * r, c[2] * r
        out[:, 12:15] = tri["emission"][:, :3]
    for a in w[0] + e1 + c + [length, r]:
        assert a.dtype == np.float32
    return out


def affine(rng, n):
    """n general affine 3x4 transforms, float32: rotation x per-axis scale within 3x x shear, plus a translation."""
    out = np.zeros((n, 12), dtype=np.float32)
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        scale = np.diag(rng.uniform(1.0, 3.0, 3))
        shear = np.eye(3)
        shear[0, 1], shear[0, 2], shear[1, 2] = rng.uniform(-0.5, 0.5, 3)
        m = np.zeros((3, 4))
        m[:, :3] = q @ scale @ shear
        m[:, 3] = rng.uniform(-5.0, 5.0, 3)
        out[i] = m.reshape(12).astype(np.float32)
    return out
