"""Writes tests/golden/spline_rig.glb, the fixture of the CUBICSPLINE tests: `python tests/golden/make_spline_gltf.py`.

The skeleton is clip_rig.glb's (make_clip_gltf.py) with one more child of the root, node 11 "face": an unskinned bar of 20
vertices with three POSITION morph targets.
  0 rig_root   TRS, children 1, 4, 5, 7, 11
  1 ja0        joint of skin 0, child 2        CUBIC translation of 3 unevenly spaced keys (td 0.75 and 1.0)
  2 ja1        joint of skin 0, child 3        CUBIC rotation of 5 keys: unnormalised values, a neighbouring pair of negative dot,
                                               tangents large enough to overshoot
  3 ja2        joint of skin 0                 an EARLIER LINEAR rotation, then a CUBIC one on the same node and path: the later wins
  4 bar_a      mesh 0, skin 0                  STEP translation of 3 keys
  5 jb0        joint of skin 1, child 6        given by `matrix`, not animated
  6 jb1        joint of skin 1                 CUBIC scale of 3 keys
  7 holder     children 8, 9, 10               CUBIC rotation of 3 keys whose tangents are all zero
  8 bar_b      mesh 1, skin 1
  9 prop       mesh 2 (a quad), unskinned      LINEAR rotation of 3 keys: a leaf, so nothing else hangs on its libm
 10 knob       given by `matrix`               CUBIC translation of ONE key
 11 face       mesh 3, three morph targets     CUBIC `weights` channel of 4 keys: a key of all zeros, a -0, weights below 0 and above 1
Animation 0 "spline" holds all of the above. Animation 1 "linear" has the same channels on the same key times and values as LINEAR
samplers (STEP where animation 0 has STEP): the blend partner. Animation 2 "through_zero" turns ja1 by a CUBIC rotation of the keys
q, -q with zero tangents, whose Hermite sum is the zero quaternion half way. `build(variant)` returns the builder of a broken
variant."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gltf_util import GltfBuilder  # noqa: E402
from make_clip_gltf import translation_matrix, two_joint_weights  # noqa: E402
from make_skinned_gltf import bar, quat_x, quat_z  # noqa: E402

VARIANTS = ("short_output", "nonfinite_tangent", "short_weights")
FACE_NODE, N_TARGETS = 11, 3


def f32(a):
    return np.array(a, np.float32)


def cubic(values, in_tangents, out_tangents):
    """Keys as a CUBICSPLINE output holds them: per key the in-tangent, the value, the out-tangent."""
    v, a, b = f32(values), f32(in_tangents), f32(out_tangents)
    return np.stack([a, v, b], axis=1).reshape(-1, v.shape[-1]).astype(np.float32)


def keys():
    """{name: (times, values, in-tangents, out-tangents)} of the cubic channels of animation 0."""
    t3, t5 = f32([0.25, 1.0, 2.0]), f32([0.0, 0.4, 0.9, 1.3, 2.0])
    five = f32([quat_x(0.0), [2.0 * c for c in quat_x(0.7)], [-c for c in quat_x(1.1)], [0.5 * c for c in quat_z(0.4)], quat_x(-0.3)])
    five_in = f32([(0, 0, 0, 0), (3.0, -1.0, 0.5, 2.0), (-2.5, 0.0, 4.0, 1.0), (0.5, 0.5, -3.0, 0.0), (6.0, 0.0, 0.0, -4.0)])
    five_out = f32([(4.0, 0.0, 0.0, -2.0), (-1.0, 2.0, 0.0, 3.0), (0.0, -5.0, 1.5, 0.0), (1.0, 1.0, 1.0, 1.0), (0, 0, 0, 0)])
    three_z = f32([quat_z(0.0), quat_z(0.9), quat_z(-0.5)])
    tw = f32([0.0, 0.5, 1.25, 2.0])
    w = f32([(0.0, 0.0, 0.0), (1.0, 0.25, -0.0), (0.3, -0.5, 1.0), (0.0, 1.5, 0.6)])
    w_in = f32([(0, 0, 0), (0.5, -1.0, 0.0), (2.0, 0.0, -1.5), (-0.75, 0.25, 0.0)])
    w_out = f32([(1.5, 0.0, 0.0), (-0.5, 2.0, 0.0), (0.0, 1.0, 0.5), (0, 0, 0)])
    return {
        "ja0_translation": (t3, f32([(0, 0, 0), (0.1, 0.25, -0.05), (0.125, 0.5, 0.2)]), f32([(0, 0, 0), (0.4, -0.2, 0.1), (-0.3, 0.6, 0.0)]),
                            f32([(0.5, 0.1, 0.0), (-0.2, 0.3, 0.25), (0, 0, 0)])),
        "ja1_rotation": (t5, five, five_in, five_out),
        "ja2_rotation": (t3, three_z, f32([(0, 0, 0.2, 0), (0, 0, -0.4, 0.3), (0.1, 0, 0, 0)]), f32([(0, 0, 0.5, -0.1), (0, 0.2, 0, 0), (0, 0, 0, 0)])),
        "jb1_scale": (t3, f32([(1, 1, 1), (1.5, 0.75, 1.25), (0.8, 1.2, 1.0)]), f32([(0, 0, 0), (0.6, -0.4, 0.2), (-0.5, 0.3, 0.0)]),
                      f32([(0.25, 0.0, -0.1), (0.0, 0.5, -0.3), (0, 0, 0)])),
        "holder_rotation": (t3, f32([quat_x(0.0), quat_x(0.5), quat_z(0.5)]), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32)),
        "knob_translation": (f32([0.75]), f32([(0.1, 0.6, -0.2)]), f32([(1.0, 2.0, 3.0)]), f32([(-1.0, 0.5, 0.25)])),
        "face_weights": (tw, w, w_in, w_out),
    }


def build(variant=None):
    """variant: None (the fixture) or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.7, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}})
    for n_rings, height, n_joints in ((6, 2.5, 3), (5, 1.5, 2)):
        pos, nrm, uv, idx = bar(n_rings, height, 0.0)
        joints, weights = two_joint_weights(pos, n_joints)
        attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(nrm, "VEC3"), "TEXCOORD_0": b.accessor(uv, "VEC2"),
                 "JOINTS_0": b.accessor(joints, "VEC4"), "WEIGHTS_0": b.accessor(weights, "VEC4")}
        b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(idx, "SCALAR"), "material": grey}]})
    quad = f32([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)])
    up = np.tile(f32((0, 1, 0)), (4, 1))
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(quad, "VEC3"), "NORMAL": b.accessor(up, "VEC3"),
                                                    "TEXCOORD_0": b.accessor(f32([(0, 0), (1, 0), (1, 1), (0, 1)]), "VEC2")},
                                     "indices": b.accessor(np.array([0, 2, 1, 0, 3, 2], np.uint32), "SCALAR"), "material": grey}]})
    pos, nrm, uv, idx = bar(5, 1.0, 0.0)
    y = pos[:, 1:2]
    out = np.concatenate([nrm[:, 0:1], np.zeros_like(y), nrm[:, 2:3]], axis=1)
    targets = [{"POSITION": b.accessor((out * 0.2 * y).astype(np.float32), "VEC3")},
               {"POSITION": b.accessor(np.concatenate([0.3 * y * y, np.zeros_like(y), np.zeros_like(y)], axis=1).astype(np.float32), "VEC3")},
               {"POSITION": b.accessor(np.concatenate([np.zeros_like(y), 0.25 * y, 0.1 * y], axis=1).astype(np.float32), "VEC3")}]
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(nrm, "VEC3"), "TEXCOORD_0": b.accessor(uv, "VEC2")},
                                     "indices": b.accessor(idx, "SCALAR"), "material": grey, "targets": targets}], "weights": [0.25, 0.0, 0.5]})
    b.doc["nodes"] = [
        {"name": "rig_root", "translation": [0.25, 0.5, -0.125], "rotation": quat_z(0.2), "scale": [1.1, 0.9, 1.05], "children": [1, 4, 5, 7, 11]},
        {"name": "ja0", "translation": [0.0, 0.0, 0.0], "children": [2]},
        {"name": "ja1", "translation": [0.0, 1.0, 0.0], "rotation": quat_x(0.1), "children": [3]},
        {"name": "ja2", "translation": [0.0, 1.0, 0.0]},
        {"name": "bar_a", "mesh": 0, "skin": 0, "translation": [0.05, 0.0, 0.1], "scale": [1.0, 1.25, 1.0]},
        {"name": "jb0", "matrix": translation_matrix(1.5, 0.0, 0.25), "children": [6]},
        {"name": "jb1", "translation": [0.0, 1.0, 0.0]},
        {"name": "holder", "translation": [-1.5, 0.0, 0.0], "children": [8, 9, 10]},
        {"name": "bar_b", "mesh": 1, "skin": 1, "rotation": quat_z(-0.15)},
        {"name": "prop", "mesh": 2, "translation": [0.0, 2.0, 0.0], "scale": [0.5, 0.5, 0.5]},
        {"name": "knob", "matrix": translation_matrix(0.0, 0.5, 0.0)},
        {"name": "face", "mesh": 3, "translation": [3.0, 0.0, 0.5]}]
    b.add("scenes", {"nodes": [0]})
    b.doc["scene"] = 0

    def inverse_binds(ys):
        m = np.zeros((len(ys), 4, 4), np.float32)
        for k, yk in enumerate(ys):
            m[k] = np.eye(4, dtype=np.float32)
            m[k][:3, 3] = (0.0, -yk, 0.0)
            m[k] = m[k].T.copy()
        return m.reshape(-1, 16)
    b.add("skins", {"joints": [1, 2, 3], "inverseBindMatrices": b.accessor(inverse_binds((0.0, 1.0, 2.0)), "MAT4")})
    b.add("skins", {"joints": [5, 6], "inverseBindMatrices": b.accessor(inverse_binds((0.0, 1.0)), "MAT4")})

    k = keys()
    t3 = f32([0.25, 1.0, 2.0])
    early = f32([quat_x(0.3), quat_x(0.6), quat_x(0.9)])
    step_t = f32([(0.05, 0.0, 0.1), (0.05, 0.25, 0.1), (0.175, 0.5, 0.1)])
    prop_r = f32([quat_z(0.0), quat_z(0.9), quat_x(-0.5)])
    targets_of = [("ja0_translation", 1, "translation"), ("ja1_rotation", 2, "rotation"), ("ja2_rotation", 3, "rotation"), ("jb1_scale", 6, "scale"),
                  ("holder_rotation", 7, "rotation"), ("knob_translation", 10, "translation"), ("face_weights", FACE_NODE, "weights")]
    for name, spline in (("spline", True), ("linear", False)):
        samplers = [{"input": b.accessor(t3, "SCALAR"), "output": b.accessor(early, "VEC4"), "interpolation": "LINEAR"},
                    {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(step_t, "VEC3"), "interpolation": "STEP"},
                    {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(prop_r, "VEC4"), "interpolation": "LINEAR"}]
        channels = [{"sampler": 0, "target": {"node": 3, "path": "rotation"}}, {"sampler": 1, "target": {"node": 4, "path": "translation"}},
                    {"sampler": 2, "target": {"node": 9, "path": "rotation"}}]
        for key, node, path in targets_of:
            times, v, tin, tout = k[key]
            data = cubic(v, tin, tout) if spline else v
            if spline and variant == "short_output" and key == "jb1_scale":
                data = data[:-1]
            if spline and variant == "nonfinite_tangent" and key == "ja1_rotation":
                data = data.copy()
                data[3 * 2 + 2, 1] = np.inf                   # the out-tangent of key 2
            kind = "SCALAR" if path == "weights" else "VEC4" if path == "rotation" else "VEC3"
            if path == "weights":
                data = data.reshape(-1)                       # per key: N_TARGETS in-tangents, values, out-tangents
                if spline and variant == "short_weights":
                    data = data[:-1]
            samplers.append({"input": b.accessor(times, "SCALAR"), "output": b.accessor(data, kind), "interpolation": "CUBICSPLINE" if spline else "LINEAR"})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": path}})
        b.add("animations", {"name": name, "samplers": samplers, "channels": channels})
    q = f32([quat_x(0.8), [-c for c in quat_x(0.8)]])
    b.add("animations", {"name": "through_zero", "samplers": [
        {"input": b.accessor(f32([0.0, 1.0]), "SCALAR"), "output": b.accessor(cubic(q, np.zeros((2, 4)), np.zeros((2, 4))), "VEC4"), "interpolation": "CUBICSPLINE"}],
        "channels": [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}]})
    return b


if __name__ == "__main__":
    out = os.path.join(HERE, "spline_rig.glb")
    build().write_glb(out)
    print(out, os.path.getsize(out), "bytes")
