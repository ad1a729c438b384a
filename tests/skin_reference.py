"""Independent references for skinning: (1) skin_model, the header's arithmetic of sr_scene_skin_mesh restated in numpy float32,
operation for operation (every numpy float32 ufunc rounds once, nothing is contracted), and (2) an independent reader of a
.glb's rig and animations with a float64 pose evaluator and a float32 restatement of the loader's matrix chain. Shares no code
with the library or with oracle/."""
import json
import struct

import numpy as np

VERTEX = np.dtype([
    ("position", "<f4", 3), ("_pad0", "<f4"), ("normal", "<f4", 3), ("_pad1", "<f4"),
    ("tangent", "<f4", 4), ("base_color_tex_coord", "<f4", 2), ("metallic_roughness_tex_coord", "<f4", 2),
    ("normal_tex_coord", "<f4", 2), ("occlusion_tex_coord", "<f4", 2), ("emissive_tex_coord", "<f4", 2),
    ("_pad3", "<f4", 2)])
INFLUENCE = np.dtype([("joint", "<u2", 4), ("weight", "<f4", 4)])
F = np.float32


# ---- 1. the skinning arithmetic --------------------------------------------------------------------------------------------------
def blended_matrices(influences, matrices):
    """B[v] = sum over k = 0..3 in order of w_k * M[j_k], from 0.0f, skipping w_k == 0 -> [n, 3, 4] float32."""
    inf = np.asarray(influences, dtype=INFLUENCE)
    M = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 3, 4)
    B = np.zeros((len(inf), 3, 4), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(4):
            w = inf["weight"][:, k]
            use = w != 0
            j = np.where(use, inf["joint"][:, k], 0).astype(np.int64)
            term = w[:, None, None] * M[j]                     # rows of skipped influences are computed and thrown away
            B = np.where(use[:, None, None], B + term, B)
    assert B.dtype == np.float32
    return B


def _apply3(A, x, y, z):
    """((A[r][0] * x + A[r][1] * y) + A[r][2] * z) for r = 0..2 -> three float32 arrays."""
    return [(A[:, r, 0] * x + A[:, r, 1] * y) + A[:, r, 2] * z for r in range(3)]


def _normalised_or_bind(vec, bind_xyz):
    """v * (1 / sqrt(dot(v, v))) where the squared length is finite and not 0, else the bind pose's bytes -> ([n, 3] uint32 words,
    mask of the fallbacks)."""
    x, y, z = vec
    with np.errstate(all="ignore"):
        len2 = (x * x + y * y) + z * z
        ok = np.isfinite(len2) & (len2 != 0)
        r = F(1.0) / np.sqrt(len2)
        out = np.stack([x * r, y * r, z * r], axis=1).astype(np.float32)
    words = np.where(ok[:, None], out.view(np.uint32), np.ascontiguousarray(bind_xyz).view(np.uint32))
    return words, ~ok


def skin_model(bind, influences, matrices):
    """-> (posed vertices, lowest index of a non-finite posed position or None, mask of normals that took the fallback)."""
    bind = np.ascontiguousarray(bind, dtype=VERTEX)
    B = blended_matrices(influences, matrices)
    out = bind.copy()
    with np.errstate(all="ignore"):
        x, y, z = (np.ascontiguousarray(bind["position"][:, c]) for c in range(3))
        p = _apply3(B, x, y, z)
        out["position"] = np.stack([p[r] + B[:, r, 3] for r in range(3)], axis=1)
        a = [B[:, r, :3] for r in range(3)]

        def cross(u, v):
            return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        Cof = np.stack([cross(a[1], a[2]), cross(a[2], a[0]), cross(a[0], a[1])], axis=1)
        n = [np.ascontiguousarray(bind["normal"][:, c]) for c in range(3)]
        t = [np.ascontiguousarray(bind["tangent"][:, c]) for c in range(3)]
        n_words, n_fallback = _normalised_or_bind(_apply3(Cof, *n), bind["normal"])
        t_words, _ = _normalised_or_bind(_apply3(B, *t), bind["tangent"][:, :3])
    words = out.view(np.uint32).reshape(len(out), -1)
    words[:, 4:7] = n_words
    words[:, 8:11] = t_words
    bad = np.flatnonzero(~np.isfinite(out["position"]).all(axis=1))
    return out, (int(bad[0]) if len(bad) else None), n_fallback


# ---- 2. an independent reader of a .glb's rig and animations ----------------------------------------------------------------------
COMPONENT = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
WIDTH = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


class Glb:
    def __init__(self, path):
        data = open(path, "rb").read()
        magic, version, length = struct.unpack_from("<4sII", data, 0)
        assert magic == b"glTF" and version == 2
        pos, self.doc, self.bin = 12, None, b""
        while pos + 8 <= length:
            n, kind = struct.unpack_from("<II", data, pos)
            body = data[pos + 8:pos + 8 + n]
            if kind == 0x4E4F534A:
                self.doc = json.loads(body.decode())
            elif kind == 0x004E4942:
                self.bin = body
            pos += 8 + n
        self.nodes = self.doc.get("nodes", [])

    def accessor(self, i):
        """Accessor i in the file's component type -> [count, components]."""
        a = self.doc["accessors"][i]
        bv = self.doc["bufferViews"][a["bufferView"]]
        dt, w = np.dtype(COMPONENT[a["componentType"]]), WIDTH[a["type"]]
        start = bv.get("byteOffset", 0) + a.get("byteOffset", 0)
        stride = bv.get("byteStride", 0) or dt.itemsize * w
        rows = [np.frombuffer(self.bin, dtype=dt, count=w, offset=start + k * stride) for k in range(a["count"])]
        return np.array(rows, dtype=dt).reshape(a["count"], w)

    # the loader's order of meshes and instances: depth first from the scene's roots, one blas per (POSITION, indices) pair
    def instances(self):
        """-> ([(blas, node)] in instance order, [(node, mesh, primitive)] that first used each blas)."""
        blas_of, inst, first = {}, [], []

        def walk(n):
            node = self.nodes[n]
            if "mesh" in node:
                for p, prim in enumerate(self.doc["meshes"][node["mesh"]]["primitives"]):
                    key = (prim["attributes"]["POSITION"], prim.get("indices"))
                    if key not in blas_of:
                        blas_of[key] = len(first)
                        first.append((n, node["mesh"], p))
                    inst.append((blas_of[key], n))
            for c in node.get("children", []):
                walk(c)
        for r in self.doc["scenes"][self.doc.get("scene", 0)]["nodes"]:
            walk(r)
        return inst, first

    def blas_skin(self, blas):
        """-> (skin index or -1, INFLUENCE array or None)."""
        node, mesh, prim = self.instances()[1][blas]
        skin = self.nodes[node].get("skin", -1)
        if skin < 0:
            return -1, None
        attrs = self.doc["meshes"][mesh]["primitives"][prim]["attributes"]
        joints, weights = self.accessor(attrs["JOINTS_0"]), self.accessor(attrs["WEIGHTS_0"])
        if weights.dtype != np.float32:
            weights = weights.astype(np.float32) / F(np.iinfo(weights.dtype).max)
        n = self.doc["accessors"][attrs["POSITION"]]["count"]
        out = np.zeros(n, dtype=INFLUENCE)
        out["joint"], out["weight"] = joints[:n], weights[:n]
        return skin, out

    def skin(self, i):
        """-> (inverse bind [n_joints, 12] float32 row-major 3x4, joint nodes)."""
        sk = self.doc["skins"][i]
        joints = np.array(sk["joints"], dtype=np.uint32)
        if "inverseBindMatrices" in sk:
            m = self.accessor(sk["inverseBindMatrices"])[:len(joints)].reshape(-1, 4, 4).transpose(0, 2, 1)     # column-major in the file
            ibm = np.ascontiguousarray(m[:, :3, :]).reshape(-1, 12)
        else:
            ibm = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (len(joints), 1))
        return ibm.astype(np.float32), joints

    def animation(self, i):
        """-> (name, duration, channels listed, weights channels)."""
        an = self.doc["animations"][i]
        last = [float(self.accessor(an["samplers"][c["sampler"]]["input"])[-1, 0]) for c in an["channels"]]
        return an.get("name", ""), F(max(last)), len(an["channels"]), sum(c["target"]["path"] == "weights" for c in an["channels"])

    def static_trs(self, n):
        node = self.nodes[n]
        return (np.array(node.get("translation", (0, 0, 0)), np.float32), np.array(node.get("rotation", (0, 0, 0, 1)), np.float32),
                np.array(node.get("scale", (1, 1, 1)), np.float32))

    def sample64(self, anim, time):
        """The float64 model of the sampling -> {node: {"translation" | "rotation" | "scale": float64 vector}}: time clamped to the
        first / last key, STEP holds, LINEAR interpolates, rotations by the textbook slerp (acos of the dot product of the
        normalised keys, the second negated where the dot is negative) and normalised."""
        out = {}
        an = self.doc["animations"][anim]
        for c in an["channels"]:
            path = c["target"]["path"]
            if path == "weights" or "node" not in c["target"]:
                continue
            smp = an["samplers"][c["sampler"]]
            t = self.accessor(smp["input"])[:, 0].astype(np.float64)
            v = self.accessor(smp["output"]).astype(np.float64)
            x = min(max(float(np.float32(time)), t[0]), t[-1])     # the call takes the time as a float
            i = int(np.searchsorted(t, x, side="right")) - 1
            if i >= len(t) - 1 or smp.get("interpolation", "LINEAR") == "STEP" or x == t[i]:
                r = v[min(i, len(t) - 1)].copy()
                if path == "rotation":
                    r /= np.linalg.norm(r)
            else:
                u = (x - t[i]) / (t[i + 1] - t[i])
                if path == "rotation":
                    a, b = v[i] / np.linalg.norm(v[i]), v[i + 1] / np.linalg.norm(v[i + 1])
                    d = float(a @ b)
                    if d < 0:
                        b, d = -b, -d
                    th = np.arccos(min(d, 1.0))
                    r = (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th) if th > 1e-6 else a + u * (b - a)
                    r /= np.linalg.norm(r)
                else:
                    r = v[i] + u * (v[i + 1] - v[i])
            out.setdefault(c["target"]["node"], {})[path] = r
        return out

    # the float32 restatement of the loader's matrix chain
    def local32(self, n, trs=None):
        """Node n's local 4x4 in float32: the file's matrix, or T * R * S with the loader's quaternion formula; trs = (t, q, s)
        float32 overrides both (an animated node composes from TRS)."""
        node = self.nodes[n]
        if trs is None and "matrix" in node:
            return np.array(node["matrix"], dtype=np.float32).reshape(4, 4).T.copy()
        t, q, s = trs if trs is not None else self.static_trs(n)
        x, y, z, w = (F(c) for c in q)
        x2, y2, z2 = x + x, y + y, z + z
        xx2, xy2, xz2, yy2, yz2, zz2 = x2 * x, x2 * y, x2 * z, y2 * y, y2 * z, z2 * z
        sy2, sz2, sx2 = y2 * w, z2 * w, x2 * w
        one = F(1.0)
        R = np.array([[one - yy2 - zz2, xy2 - sz2, xz2 + sy2], [xy2 + sz2, one - xx2 - zz2, yz2 - sx2], [xz2 - sy2, yz2 + sx2, one - xx2 - yy2]], dtype=np.float32)
        m = np.eye(4, dtype=np.float32)
        m[:3, :3] = R * np.asarray(s, dtype=np.float32)[None, :]
        m[:3, 3] = t
        return m

    @staticmethod
    def mul32(a, b):
        """r[i][j] = ((a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]) + a[i][3] * b[3][j], float32."""
        return ((a[:, 0:1] * b[0:1, :] + a[:, 1:2] * b[1:2, :]) + a[:, 2:3] * b[2:3, :]) + a[:, 3:4] * b[3:4, :]

    def globals32(self, trs_of=None):
        """{node: world 4x4 float32} from the scene's roots; trs_of = {node: (t, q, s)} for the animated nodes."""
        out = {}

        def walk(n, parent):
            out[n] = self.mul32(parent, self.local32(n, (trs_of or {}).get(n)))
            for c in self.nodes[n].get("children", []):
                walk(c, out[n])
        for r in self.doc["scenes"][self.doc.get("scene", 0)]["nodes"]:
            walk(r, np.eye(4, dtype=np.float32))
        return out

    @staticmethod
    def inverse_affine(m):
        """The inverse of a float32 affine 4x4 by cofactors in float64, the operations in the library's order, rounded once."""
        M = np.asarray(m, dtype=np.float64)
        a00, a01, a02, a10, a11, a12, a20, a21, a22 = (float(M[r, c]) for r in range(3) for c in range(3))
        c00, c01, c02 = a11 * a22 - a12 * a21, a12 * a20 - a10 * a22, a10 * a21 - a11 * a20
        det = a00 * c00 + a01 * c01 + a02 * c02
        inv_det = 1.0 / det
        R = [[c00 * inv_det, (a02 * a21 - a01 * a22) * inv_det, (a01 * a12 - a02 * a11) * inv_det],
             [c01 * inv_det, (a00 * a22 - a02 * a20) * inv_det, (a02 * a10 - a00 * a12) * inv_det],
             [c02 * inv_det, (a01 * a20 - a00 * a21) * inv_det, (a00 * a11 - a01 * a10) * inv_det]]
        T = [float(M[0, 3]), float(M[1, 3]), float(M[2, 3])]
        out = np.eye(4, dtype=np.float32)
        for r in range(3):
            out[r, :3] = [F(v) for v in R[r]]
            out[r, 3] = F(-(R[r][0] * T[0] + R[r][1] * T[1] + R[r][2] * T[2]))
        return out

    def pose32(self, trs_of, skin):
        """-> (instance transforms [n, 12], joint matrices [n_joints, 12]) in float32, in the loader's operation order: world
        matrices down the hierarchy, then inverse(world(mesh node)) * world(joint node) * inverseBind, left to right."""
        g = self.globals32(trs_of)
        inst = np.array([g[n][:3].reshape(12) for _, n in self.instances()[0]], dtype=np.float32)
        if skin is None:
            return inst, None
        mesh_node = next(n for _, n in self.instances()[0] if self.nodes[n].get("skin", -1) == skin)
        inv = self.inverse_affine(g[mesh_node])
        ibm, joints = self.skin(skin)
        out = []
        for k, j in enumerate(joints):
            ib = np.eye(4, dtype=np.float32)
            ib[:3] = ibm[k].reshape(3, 4)
            out.append(self.mul32(self.mul32(inv, g[int(j)]), ib)[:3].reshape(12))
        return inst, np.array(out, dtype=np.float32)
