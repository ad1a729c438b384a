"""Shared by the CUBICSPLINE tests: the fixture, the times a channel is evaluated at, files of the shapes at which the device
kernels can go wrong, and a tool that turns the samplers of any .glb into CUBICSPLINE ones on the same keys. Nothing here needs a
GPU."""
import json
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from gltf_util import GltfBuilder  # noqa: E402

SPLINE_RIG = os.path.join(HERE, "golden", "spline_rig.glb")
SKINNED_BAR = os.path.join(HERE, "golden", "skinned_bar.glb")
MORPH_BAR = os.path.join(HERE, "golden", "morph_bar.glb")
TARGET_COUNTS = (1, 64, 65, 130)        # the chunk boundaries of a 64-lane wave
QUAD_TIMES = (0.25, 0.75, 2.0)          # unevenly spaced


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def f32(a):
    return np.array(a, np.float32)


def channel_times(keys):
    """The time set of one channel: below the first key, every key time, nextafter above each key, a midpoint of every interval,
    nextafter below the last key, above the last key: float32, ascending, each once."""
    keys = f32(keys)
    ts = {float(keys[0]) - 1.0, float(keys[-1]) + 1.5, float(np.nextafter(keys[-1], np.float32(-np.inf)))}
    for k in keys:
        ts.update((float(k), float(np.nextafter(k, np.float32(np.inf)))))
    for a, b in zip(keys[:-1], keys[1:]):
        ts.add(float(a + np.float32(0.5) * (b - a)))
    return sorted({float(np.float32(t)) for t in ts})


def clip_channel_times(clip, blases=()):
    """channel_times over every channel of a clip and the morph sets of `blases`, merged."""
    ts = set()
    for c in range(clip.info.n_channels):
        ts.update(channel_times(clip.channel_keys(c)[0]))
    for b in blases:
        keys = clip.morph_keys(b)[0]
        if len(keys):
            ts.update(channel_times(keys))
    return sorted(ts)


def triangle(b, material, n_targets):
    """A triangle with n_targets POSITION-only morph targets -> mesh index."""
    pos = f32([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.0, 0, 0.5)])
    attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(np.tile(f32((0, 1, 0)), (3, 1)), "VEC3"),
             "TEXCOORD_0": b.accessor(f32([(0, 0), (1, 0), (0.5, 1)]), "VEC2")}
    targets = []
    for k in range(n_targets):
        d = np.zeros((3, 3), np.float32)
        d[:, 1] = 0.001 * (1 + k % 7)
        d[k % 3, 0] = 0.002 * (1 + k % 5)
        targets.append({"POSITION": b.accessor(d, "VEC3")})
    return b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(np.array([0, 2, 1], np.uint32), "SCALAR"), "material": material, "targets": targets}]})


def quad_keys(n_targets):
    """(values, in-tangents, out-tangents), each [3, n_targets], of spline_quad's channel: key 0 is all zeros; key 1 is zero at
    the ends of the chunks of 64 and -0 at target 5 (where there is one); key 2 has no zero. The tangents are large enough to
    overshoot and differ from target to target."""
    k = np.arange(n_targets, dtype=np.float32)
    v = np.zeros((3, n_targets), np.float32)
    v[1] = 0.01 * (k + 1.0)
    for z in (0, 63, 64, 127, 128, 129):
        if z < n_targets and n_targets > 1:
            v[1, z] = 0.0
    if n_targets > 5:
        v[1, 5] = -0.0
    v[2] = 0.25 + 0.005 * k
    a = np.stack([np.zeros(n_targets), 0.5 - 0.01 * k, -1.0 + 0.02 * (k % 7)]).astype(np.float32)
    o = np.stack([1.5 - 0.03 * (k % 11), -0.75 + 0.01 * k, np.zeros(n_targets)]).astype(np.float32)
    return v, a, o


def spline_quad(path, n_targets):
    """Writes a file of one triangle with n_targets morph targets on one root node. Animation 0: a CUBICSPLINE `weights` channel
    of the 3 keys of quad_keys at QUAD_TIMES. Animation 1: the same values on a LINEAR channel (the blend partner)."""
    b = GltfBuilder()
    b.doc["animations"] = []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0]}})
    b.add("nodes", {"name": "tri", "mesh": triangle(b, grey, n_targets)})
    b.add("scenes", {"nodes": [0]})
    b.doc["scene"] = 0
    v, a, o = quad_keys(n_targets)
    rows = np.stack([a, v, o], axis=1).reshape(-1).astype(np.float32)           # per key: in-tangents, values, out-tangents
    times = f32(QUAD_TIMES)
    b.add("animations", {"name": "spline", "samplers": [{"input": b.accessor(times, "SCALAR"), "output": b.accessor(rows, "SCALAR"), "interpolation": "CUBICSPLINE"}],
                         "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]})
    b.add("animations", {"name": "linear", "samplers": [{"input": b.accessor(times, "SCALAR"), "output": b.accessor(v.reshape(-1), "SCALAR"), "interpolation": "LINEAR"}],
                         "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]})
    b.write_glb(path)


def collapsing_rig(path):
    """Writes a rig of a root, one joint and a skinned quad whose mesh node's scale a CUBICSPLINE channel drives through 0 at
    t = 1 (key 1's value is (0, 1, 1)): a singular mesh-node transform at that time and only there."""
    from clip_util import tiny_mesh
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0]}})
    b.doc["nodes"] = [{"name": "root", "children": [1, 2]}, {"name": "joint", "translation": [0.0, 0.5, 0.0]},
                      {"name": "skinned", "mesh": tiny_mesh(b, grey, 1), "skin": 0, "translation": [0.0, 0.5, 0.0]}]
    b.add("skins", {"joints": [1]})
    b.add("scenes", {"nodes": [0]})
    b.doc["scene"] = 0
    v = f32([(1, 1, 1), (0, 1, 1), (1, 1, 1)])
    t = f32([(0, 0, 0), (0.5, 0, 0), (0, 0, 0)])
    rows = np.stack([t, v, -t], axis=1).reshape(-1, 3).astype(np.float32)
    b.add("animations", {"name": "collapse", "samplers": [{"input": b.accessor(f32([0.0, 1.0, 2.0]), "SCALAR"), "output": b.accessor(rows, "VEC3"), "interpolation": "CUBICSPLINE"}],
                         "channels": [{"sampler": 0, "target": {"node": 2, "path": "scale"}}]})
    b.write_glb(path)


def cubic_copy(src, dst, tangent=0.0):
    """Writes `dst`, the .glb `src` with every animation sampler turned into a CUBICSPLINE one on the same key times and values:
    in- and out-tangents are `tangent` times the difference to the neighbouring key's value per second (0.0: the curve rests at
    every key). STEP samplers are left alone. `weights` outputs keep their per-key rows."""
    raw = open(src, "rb").read()
    jlen = struct.unpack_from("<I", raw, 12)[0]
    doc = json.loads(raw[20:20 + jlen])
    blen = struct.unpack_from("<I", raw, 20 + jlen)[0]
    binc = bytearray(raw[28 + jlen:28 + jlen + blen])
    comps = {"SCALAR": 1, "VEC3": 3, "VEC4": 4}

    def read(acc):
        a = doc["accessors"][acc]
        bv = doc["bufferViews"][a["bufferView"]]
        n = a["count"] * comps[a["type"]]
        assert a["componentType"] == 5126 and "byteStride" not in bv
        return np.frombuffer(bytes(binc), np.float32, n, bv.get("byteOffset", 0) + a.get("byteOffset", 0)).copy()

    def append(arr, type_):
        while len(binc) % 4:
            binc.append(0)
        doc["bufferViews"].append({"buffer": 0, "byteOffset": len(binc), "byteLength": arr.nbytes})
        binc.extend(arr.tobytes())
        doc["accessors"].append({"bufferView": len(doc["bufferViews"]) - 1, "componentType": 5126, "count": arr.size // comps[type_], "type": type_})
        return len(doc["accessors"]) - 1
    for an in doc.get("animations", []):
        for s in an["samplers"]:
            if s.get("interpolation", "LINEAR") != "LINEAR":
                continue
            times = read(s["input"])
            type_ = doc["accessors"][s["output"]]["type"]
            v = read(s["output"]).reshape(len(times), -1)
            d = np.zeros_like(v)
            if len(times) > 1:
                d[:-1] = (v[1:] - v[:-1]) / (times[1:] - times[:-1])[:, None]
            rows = np.stack([np.roll(d, 1, axis=0) * np.float32(tangent), v, d * np.float32(tangent)], axis=1).astype(np.float32)
            rows[0, 0] = 0.0
            s["output"] = append(rows.reshape(-1), type_)
            s["interpolation"] = "CUBICSPLINE"
    doc["buffers"] = [{"byteLength": len(binc)}]
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    body = bytes(binc) + b"\0" * (-len(binc) % 4)
    with open(dst, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 28 + len(js) + len(body)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(body), 0x004E4942) + body)
