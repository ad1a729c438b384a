"""Independent reference for the mesh frame (sr_scene_set_mesh_frame / sr_scene_update_mesh_positions*): (1) the smoothing groups
and per-vertex runs in plain Python, (2) frame_model, the header's rule restated in numpy float32, operation for operation
(every numpy float32 ufunc rounds once, nothing is contracted, sqrt and divide are correctly rounded), (3) frame_model64, the same
geometry in float64, and (4) the small meshes the tests share. Shares no code with the library or with oracle/."""
import numpy as np

VERTEX = np.dtype([("position", "<f4", 3), ("_pad0", "<f4"), ("normal", "<f4", 3), ("_pad1", "<f4"), ("tangent", "<f4", 4),
                   ("base_color_tex_coord", "<f4", 2), ("metallic_roughness_tex_coord", "<f4", 2), ("normal_tex_coord", "<f4", 2),
                   ("occlusion_tex_coord", "<f4", 2), ("emissive_tex_coord", "<f4", 2), ("_pad3", "<f4", 2)])
assert VERTEX.itemsize == 96
F = np.float32
NORMALS, TANGENTS = 1, 2


# ---- 1. groups and runs -----------------------------------------------------------------------------------------------------------
def adjacency(vertices, indices):
    """-> (offsets [n + 1] uint32, entries uint32, groups: list of the group number of every vertex, numbered by first
    appearance). Two vertices share a group iff the bytes of their position and of their normal are equal; a vertex's run is the
    triangle of every corner (t, c) whose vertex is in its group, in ascending (t, c)."""
    v = np.ascontiguousarray(vertices, dtype=VERTEX)
    idx = [int(i) for i in np.asarray(indices).ravel()]
    assert len(idx) % 3 == 0 and all(0 <= i < len(v) for i in idx)
    number, groups = {}, []
    for i in range(len(v)):
        key = v["position"][i].tobytes() + v["normal"][i].tobytes()
        groups.append(number.setdefault(key, len(number)))
    runs = [[] for _ in number]
    for k, i in enumerate(idx):
        runs[groups[i]].append(k // 3)
    offsets, entries = [0], []
    for i in range(len(v)):
        entries += runs[groups[i]]
        offsets.append(len(entries))
    return np.array(offsets, dtype=np.uint32), np.array(entries, dtype=np.uint32), groups


def _face_vectors(p, indices, dtype):
    i0, i1, i2 = (np.asarray(indices, dtype=np.int64).reshape(-1, 3)[:, c] for c in range(3))
    p = np.asarray(p, dtype=dtype)
    e1, e2 = p[i1] - p[i0], p[i2] - p[i0]
    Fv = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    return e1, e2, Fv


def _accumulate(per_triangle, offsets, entries, dtype):
    """(0, 0, 0), then + per_triangle[t] over each vertex's run, in run order (vectorised over the vertices, one step per place)."""
    n = len(offsets) - 1
    counts = (offsets[1:] - offsets[:-1]).astype(np.int64)
    acc = np.zeros((n, 3), dtype=dtype)
    for j in range(int(counts.max()) if n else 0):
        on = np.flatnonzero(counts > j)
        acc[on] = acc[on] + per_triangle[entries[offsets[:-1][on].astype(np.int64) + j]]
    return acc


def sides(vertices, indices, adj=None):
    """side per vertex: -1 where dot(N_ref, reference normal) < 0, N_ref the rule's own sum over the reference positions."""
    v = np.ascontiguousarray(vertices, dtype=VERTEX)
    offsets, entries, _ = adj or adjacency(v, indices)
    with np.errstate(all="ignore"):
        N = _accumulate(_face_vectors(v["position"], indices, F)[2], offsets, entries, F)
        n = v["normal"]
        d = (N[:, 0] * n[:, 0] + N[:, 1] * n[:, 1]) + N[:, 2] * n[:, 2]
    return np.where(d < 0, F(-1.0), F(1.0)).astype(F)


# ---- 2. the rule in float32 -------------------------------------------------------------------------------------------------------
def _normalised_words(x, y, z):
    len2 = (x * x + y * y) + z * z
    ok = np.isfinite(len2) & (len2 != 0)
    r = F(1.0) / np.sqrt(len2)
    return np.stack([x * r, y * r, z * r], axis=1).astype(F).view(np.uint32), ok


def frame_model(vertices, indices, positions, flags):
    """-> (records, lowest index of a non-finite position or None, mask of normals that fell back to the reference's)."""
    assert flags in (NORMALS, NORMALS | TANGENTS)
    ref = np.ascontiguousarray(vertices, dtype=VERTEX)
    p = np.ascontiguousarray(positions, dtype=F)
    assert p.shape == (len(ref), 3)
    adj = adjacency(ref, indices)
    offsets, entries, _ = adj
    out = ref.copy()
    words = out.view(np.uint32).reshape(len(out), -1)
    rwords = ref.view(np.uint32).reshape(len(ref), -1)
    with np.errstate(all="ignore"):
        e1, e2, Fv = _face_vectors(p, indices, F)
        N = _accumulate(Fv, offsets, entries, F)
        s = sides(ref, indices, adj)
        new, ok = _normalised_words(s * N[:, 0], s * N[:, 1], s * N[:, 2])
        words[:, 0:3] = p.view(np.uint32)
        words[:, 4:7] = np.where(ok[:, None], new, rwords[:, 4:7])
        fallback = ~ok
        if flags & TANGENTS:
            uv = ref["normal_tex_coord"]
            i0, i1, i2 = (np.asarray(indices, dtype=np.int64).reshape(-1, 3)[:, c] for c in range(3))
            a, b = uv[i1] - uv[i0], uv[i2] - uv[i0]
            det = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
            sg = np.where(det > 0, F(1.0), F(-1.0)).astype(F)
            T = sg[:, None] * (e1 * b[:, 1][:, None] - e2 * a[:, 1][:, None])
            T = np.where(((det == 0) | ~np.isfinite(det))[:, None], F(0.0), T).astype(F)
            A = _accumulate(T, offsets, entries, F)
            n = words[:, 4:7].copy().view(F)                     # the new normal, or the reference's where it fell back
            d = (n[:, 0] * A[:, 0] + n[:, 1] * A[:, 1]) + n[:, 2] * A[:, 2]
            newt, okt = _normalised_words(A[:, 0] - n[:, 0] * d, A[:, 1] - n[:, 1] * d, A[:, 2] - n[:, 2] * d)
            words[:, 8:11] = np.where(okt[:, None], newt, rwords[:, 8:11])
    bad = np.flatnonzero(~np.isfinite(p).all(axis=1))
    return out, (int(bad[0]) if len(bad) else None), fallback


# ---- 3. the same geometry in float64 ----------------------------------------------------------------------------------------------
def frame_model64(vertices, indices, positions):
    """-> (unit normals float64 [n, 3], |sum of the face vectors| per vertex, sum of the |face vectors| per vertex): the
    area-weighted normal of every vertex from the float32 positions taken as exact, on the side the float32 rule chose."""
    ref = np.ascontiguousarray(vertices, dtype=VERTEX)
    adj = adjacency(ref, indices)
    offsets, entries, _ = adj
    Fv = _face_vectors(np.asarray(positions, dtype=np.float64), indices, np.float64)[2]
    N = _accumulate(Fv, offsets, entries, np.float64) * sides(ref, indices, adj).astype(np.float64)[:, None]
    length = np.sqrt((N * N).sum(axis=1))
    total = _accumulate(np.repeat(np.sqrt((Fv * Fv).sum(axis=1))[:, None], 3, axis=1), offsets, entries, np.float64)[:, 0]
    with np.errstate(all="ignore"):
        return N / length[:, None], length, total


# ---- 4. meshes --------------------------------------------------------------------------------------------------------------------
def make(pos, nrm, uv=None, idx=()):
    """Records with every word made to count: a unit tangent with a handedness, five different uv sets, arbitrary pad words."""
    v = np.zeros(len(pos), dtype=VERTEX)
    i = np.arange(len(v))
    v["position"], v["normal"] = np.asarray(pos, dtype=F), np.asarray(nrm, dtype=F)
    v["tangent"] = (0.6, 0.0, 0.8, 1.0)
    v["tangent"][i % 3 == 1, 3] = -1.0
    uv = np.asarray(v["position"][:, :2] * F(0.25) + F(0.5) if uv is None else uv, dtype=F)
    for k, name in enumerate(("base_color", "metallic_roughness", "normal", "occlusion", "emissive")):
        v[name + "_tex_coord"] = uv if name == "normal" else uv * F(k + 2)
    w = v.view(np.uint32).reshape(len(v), -1)
    w[:, 3], w[:, 7], w[:, 22], w[:, 23] = 0x7FC00000 + i, 0xFF800000, 0xDEADBEEF, i
    return v, np.asarray(idx, dtype=np.uint32)


def single_triangle():
    return make([(-1, -1, 0), (1, -1, 0.25), (0, 1, 0)], [(0, 0, 1)] * 3, idx=[0, 1, 2])


def cube():
    """24 vertices, four per face with the face's normal: every group is one vertex, the edges stay hard."""
    pos, nrm, uv, idx = [], [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3); n[axis] = sign
            u, w = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3], w[(axis + 2) % 3] = 1.0, sign       # u x w = n
            base = len(pos)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                pos.append(n + a * u + b * w); nrm.append(n); uv.append((0.5 + 0.5 * a, 0.5 + 0.5 * b))
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return make(pos, nrm, uv, idx)


def seam_sphere(segments=12, rings=7, radius=1.0):
    """A uv-sphere as loaders deliver it: (rings + 1) x (segments + 1) vertices, the seam column and the poles duplicated with
    equal position and normal bytes and other uvs. The seam twins and the copies of a pole share a group."""
    pos, uv, idx = [], [], []
    for r in range(rings + 1):
        phi = np.pi * r / rings
        for s in range(segments + 1):
            th = 2 * np.pi * (s % segments) / segments            # the seam twin has the same bits
            y, q = (1.0, 0.0) if r == 0 else ((-1.0, 0.0) if r == rings else (np.cos(phi), np.sin(phi)))
            pos.append((radius * q * np.cos(th), radius * y, radius * q * np.sin(th)) if q else (0.0, radius * y, 0.0))   # no -0 at a pole
            uv.append((s / segments, r / rings))
    at = lambda r, s: r * (segments + 1) + s
    for r in range(rings):
        for s in range(segments):
            a, b, c, d = at(r, s), at(r, s + 1), at(r + 1, s + 1), at(r + 1, s)
            if r > 0:
                idx += [a, b, c]
            if r < rings - 1:
                idx += [a, c, d]
    pos = np.array(pos, dtype=F)
    return make(pos, (pos / np.sqrt((pos.astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(F), uv, idx)


def fan(n=300):
    """A shallow cone: the hub (vertex 0) has n entries, every rim vertex two."""
    th = 2 * np.pi * np.arange(n) / n
    pos = np.concatenate([[(0.0, 0.0, 0.3)], np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)])
    idx = [j for k in range(n) for j in (0, 1 + k, 1 + (k + 1) % n)]
    return make(pos, [(0, 0, 1)] * (n + 1), idx=idx)


def unreferenced_vertex():
    """A quad and a fifth vertex no triangle names: its run is empty, normal and tangent keep the reference's bytes."""
    return make([(-1, -1, 0), (1, -1, 0), (1, 1, 0.2), (-1, 1, 0), (5, 5, 5)], [(0, 0, 1)] * 5, idx=[0, 1, 2, 0, 2, 3])


def repeated_index():
    """Triangles that name a vertex twice (zero face vectors, two entries of one triangle in a run) next to a proper one."""
    return make([(-1, -1, 0), (1, -1, 0), (0, 1, 0.1), (2, 1, 0)], [(0, 0, 1)] * 4, idx=[0, 1, 1, 0, 0, 2, 0, 1, 2, 3, 3, 3, 1, 3, 2])


def grid(nu, nv, flip=False, mirror_uv=False):
    """nu x nv vertices over [-1, 1]^2 in z = 0 with normals +z; flip: the winding gives -z (side is -1 throughout); mirror_uv: u
    runs back over the second half (det < 0 there)."""
    xs, ys = np.meshgrid(np.linspace(-1, 1, nu), np.linspace(-1, 1, nv), indexing="ij")
    pos = np.stack([xs.ravel(), ys.ravel(), np.zeros(nu * nv)], axis=1)
    u = 0.5 + 0.5 * xs.ravel()
    uv = np.stack([np.where(u > 0.5, 1.0 - u, u) if mirror_uv else u, 0.5 + 0.5 * ys.ravel()], axis=1)
    idx = []
    for i in range(nu - 1):
        for j in range(nv - 1):
            a, b, c, d = i * nv + j, (i + 1) * nv + j, (i + 1) * nv + j + 1, i * nv + j + 1
            idx += [a, c, b, a, d, c] if flip else [a, b, c, a, c, d]
    return make(pos, [(0, 0, 1)] * (nu * nv), uv, idx)


def strip(n):
    """A triangle strip of n vertices (n - 2 triangles, the winding kept): any vertex count."""
    k = np.arange(n)
    pos = np.stack([0.1 * (k // 2), (k % 2).astype(np.float64), np.zeros(n)], axis=1)
    idx = [j for t in range(n - 2) for j in ((t, t + 2, t + 1) if t % 2 == 0 else (t, t + 1, t + 2))]
    return make(pos, [(0, 0, 1)] * n, idx=idx)


def displaced(vertices, phase=0.7, amplitude=0.15):
    """Smoothly displaced positions, float32 [n, 3]; vertices at one reference position move alike (a seam stays closed)."""
    p = vertices["position"].astype(np.float64)
    d = np.stack([np.sin(3.1 * p[:, 1] + phase) * np.cos(2.3 * p[:, 2]), np.sin(2.7 * p[:, 2] + 2 * phase) * np.cos(1.9 * p[:, 0]),
                  np.sin(3.7 * p[:, 0] + 3 * phase) * np.cos(2.9 * p[:, 1] + phase)], axis=1)
    return np.ascontiguousarray((p + amplitude * d).astype(F))


def heightfield_patch(n=33):
    """An n x n patch of rolling terrain (y up) with its own smooth normals."""
    v, idx = grid(n, n)
    x, z = v["position"][:, 0].astype(np.float64), v["position"][:, 1].astype(np.float64)
    h = 0.2 * np.sin(2.5 * x) * np.cos(3.5 * z) + 0.05 * np.sin(9 * x + 1)
    v["position"] = np.stack([x, h, z], axis=1)
    tri = np.asarray(idx).reshape(-1, 3)[:, [0, 2, 1]]             # x, z in the plane: the other winding looks up
    v["normal"] = (0, 1, 0)
    return v, np.ascontiguousarray(tri.ravel(), dtype=np.uint32)
