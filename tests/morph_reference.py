"""Independent references for morph targets: (1) morph_model, the header's arithmetic of sr_scene_pose_mesh's morph stage restated
in numpy float32, operation for operation (every numpy float32 ufunc rounds once, nothing is contracted, sqrt and divide are
correctly rounded), and (2) an independent reader of a .glb's morph targets and `weights` channels with a float64 model of the
sampling. Shares no code with the library or with oracle/."""
import numpy as np

import skin_reference as sref

VERTEX = sref.VERTEX
DELTA = np.dtype([("position", "<f4", 3), ("_pad0", "<f4"), ("normal", "<f4", 3), ("_pad1", "<f4"), ("tangent", "<f4", 3), ("_pad2", "<f4")])
F = np.float32


# ---- 1. the morph arithmetic ----------------------------------------------------------------------------------------------------
def blended_deltas(deltas, weights, name):
    """s = (0, 0, 0), then for every target whose weight is not 0, in ascending order: s = s + w_k * d_k -> [n_vertices, 3] float32."""
    d = np.asarray(deltas, dtype=DELTA)
    w = np.ascontiguousarray(weights, dtype=np.float32)
    assert d.ndim == 2 and d.shape[0] == len(w)
    s = np.zeros((d.shape[1], 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for k in range(len(w)):
            if w[k] != 0:                                       # -0.0f is a weight of 0 too: the target is not active
                s = s + w[k] * d[name][k]
    assert s.dtype == np.float32
    return s


def morph_model(base, deltas, weights):
    """-> (morphed vertices, lowest index of a non-finite morphed position or None, mask of normals that took the zero-length
    fallback)."""
    base = np.ascontiguousarray(base, dtype=VERTEX)
    out = base.copy()
    words = out.view(np.uint32).reshape(len(out), -1)
    bwords = base.view(np.uint32).reshape(len(base), -1)
    fallback = np.zeros(len(base), dtype=bool)
    with np.errstate(all="ignore"):
        for name, at in (("position", 0), ("normal", 4), ("tangent", 8)):
            s = blended_deltas(deltas, weights, name)
            moved = ~(s == 0).all(axis=1)                       # a NaN in s is not 0: the vector is rewritten (and the position refused)
            b = np.ascontiguousarray(base[name][:, :3])
            v = b + s
            if name == "position":
                new = v.view(np.uint32)
                ok = np.ones(len(base), dtype=bool)
            else:
                x, y, z = v[:, 0], v[:, 1], v[:, 2]
                len2 = (x * x + y * y) + z * z
                ok = np.isfinite(len2) & (len2 != 0)
                r = F(1.0) / np.sqrt(len2)
                new = np.stack([x * r, y * r, z * r], axis=1).astype(np.float32).view(np.uint32)
                if name == "normal":
                    fallback = moved & ~ok
            words[:, at:at + 3] = np.where((moved & ok)[:, None], new, bwords[:, at:at + 3])
    bad = np.flatnonzero(~np.isfinite(out["position"]).all(axis=1))
    return out, (int(bad[0]) if len(bad) else None), fallback


# ---- 2. an independent reader of a .glb's morph targets and weight animations ----------------------------------------------------
class Glb(sref.Glb):
    def accessor(self, i):
        """Accessor i with its sparse substitution resolved (zeros where it has no bufferView) -> [count, components]."""
        a = self.doc["accessors"][i]
        dt, w = np.dtype(sref.COMPONENT[a["componentType"]]), sref.WIDTH[a["type"]]
        out = sref.Glb.accessor(self, i).copy() if "bufferView" in a else np.zeros((a["count"], w), dtype=dt)
        if "sparse" in a:
            sp = a["sparse"]
            iv, vv = self.doc["bufferViews"][sp["indices"]["bufferView"]], self.doc["bufferViews"][sp["values"]["bufferView"]]
            at = np.frombuffer(self.bin, dtype=sref.COMPONENT[sp["indices"]["componentType"]], count=sp["count"],
                               offset=iv.get("byteOffset", 0) + sp["indices"].get("byteOffset", 0))
            val = np.frombuffer(self.bin, dtype=dt, count=sp["count"] * w, offset=vv.get("byteOffset", 0) + sp["values"].get("byteOffset", 0))
            out[at.astype(np.int64)] = val.reshape(-1, w)
        return out

    def blas_morph(self, blas):
        """-> (DELTA array [n_targets, n_vertices], default weights float32 [n_targets]) or (None, None)."""
        node, mesh, prim = self.instances()[1][blas]
        p = self.doc["meshes"][mesh]["primitives"][prim]
        targets = p.get("targets", [])
        if not targets:
            return None, None
        n = self.doc["accessors"][p["attributes"]["POSITION"]]["count"]
        out = np.zeros((len(targets), n), dtype=DELTA)
        for k, t in enumerate(targets):
            for name, acc in t.items():
                out[name.lower()][k] = self.accessor(acc)[:n]
        w = self.nodes[node].get("weights", self.doc["meshes"][mesh].get("weights", [0.0] * len(targets)))
        return out, np.array(w, dtype=np.float32)

    def weights_channel(self, anim, blas):
        """-> (times float32, values float32 [n_keys, n_targets], interpolation) of the `weights` channel on the blas's first node, or None."""
        node = self.instances()[1][blas][0]
        nt = len(self.blas_morph(blas)[1])
        an = self.doc["animations"][anim]
        for c in an["channels"]:
            if c["target"]["path"] == "weights" and c["target"].get("node") == node:
                smp = an["samplers"][c["sampler"]]
                t = self.accessor(smp["input"])[:, 0]
                return t, self.accessor(smp["output"])[:len(t) * nt, 0].reshape(len(t), nt), smp.get("interpolation", "LINEAR")
        return None

    def weights64(self, anim, time, blas):
        """The float64 model of the sampling -> float64 [n_targets]: the default weights without a channel; time clamped to the
        first / last key, STEP holds, LINEAR interpolates."""
        ch = self.weights_channel(anim, blas) if anim >= 0 else None
        if ch is None:
            return self.blas_morph(blas)[1].astype(np.float64)
        t, v, mode = ch[0].astype(np.float64), ch[1].astype(np.float64), ch[2]
        x = min(max(float(np.float32(time)), t[0]), t[-1])         # the call takes the time as a float
        i = int(np.searchsorted(t, x, side="right")) - 1
        if i >= len(t) - 1 or mode == "STEP" or x == t[i]:
            return v[min(i, len(t) - 1)].copy()
        u = (x - t[i]) / (t[i + 1] - t[i])
        return v[i] + u * (v[i + 1] - v[i])
