"""Writes tests/golden/clip_rig.glb, the fixture of the baked-clip tests: `python tests/golden/make_clip_gltf.py`.

Nodes (the default scene's root is node 0):
  0 rig_root   TRS, children 1, 4, 5, 7
  1 ja0        joint of skin 0, child 2        STEP translation (3 keys); LINEAR rotation of 2 nearly equal keys (theta < 1e-9)
  2 ja1        joint of skin 0, child 3        LINEAR rotation of 5 keys: a pair with negative dot, unnormalised keys
  3 ja2        joint of skin 0                 LINEAR rotation of 3 keys, and an EARLIER channel on the same node and path
  4 bar_a      mesh 0 (24 vertices), skin 0    an animated mesh node: LINEAR translation of 2 keys
  5 jb0        joint of skin 1, child 6        given by `matrix`, not animated
  6 jb1        joint of skin 1                 LINEAR scale of 3 keys
  7 holder     children 8, 9, 10               LINEAR rotation of 3 keys
  8 bar_b      mesh 1 (20 vertices), skin 1
  9 prop       mesh 2 (a quad), unskinned, under the animated node 7
 10 knob       given by `matrix`               a translation channel of ONE key: composes from TRS (the glTF defaults)
Four levels (0 / 1 4 5 7 / 2 6 8 9 10 / 3). Animation 0 "play" holds all of the above; animation 1 "collapse" drives the scale
of the mesh node 4 through 0 at t = 1 (a singular mesh-node transform) and turns ja1. `build(variant)` returns the builder of a
variant that sr_gltf_bake_clip refuses."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from gltf_util import GltfBuilder  # noqa: E402
from make_skinned_gltf import bar, quat_x, quat_z  # noqa: E402

VARIANTS = ("cubic", "joint_outside_scene", "times_not_increasing", "shared_child")


def two_joint_weights(pos, n_joints):
    """Each vertex blends the joint below it and the next one; rows sum to 1."""
    joints, weights = np.zeros((len(pos), 4), np.uint16), np.zeros((len(pos), 4), np.float32)
    for v, p in enumerate(pos):
        t = float(p[1])
        lower = min(int(t), n_joints - 2)
        f = np.float32(min(max(t - lower, 0.0), 1.0))
        joints[v], weights[v] = (lower, lower + 1, 0, 0), (np.float32(1.0) - f, f, 0, 0)
    return joints, weights


def translation_matrix(x, y, z):
    return [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, float(x), float(y), float(z), 1]     # column-major


def build(variant=None):
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.7, 0.7, 0.8, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}})
    for n_rings, height, n_joints in ((6, 2.5, 3), (5, 1.5, 2)):
        pos, nrm, uv, idx = bar(n_rings, height, 0.0)
        joints, weights = two_joint_weights(pos, n_joints)
        attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(nrm, "VEC3"), "TEXCOORD_0": b.accessor(uv, "VEC2"),
                 "JOINTS_0": b.accessor(joints, "VEC4"), "WEIGHTS_0": b.accessor(weights, "VEC4")}
        b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(idx, "SCALAR"), "material": grey}]})
    quad = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)], np.float32)
    up = np.tile(np.array((0, 1, 0), np.float32), (4, 1))
    quad_uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(quad, "VEC3"), "NORMAL": b.accessor(up, "VEC3"), "TEXCOORD_0": b.accessor(quad_uv, "VEC2")},
                                     "indices": b.accessor(np.array([0, 2, 1, 0, 3, 2], np.uint32), "SCALAR"), "material": grey}]})
    b.doc["nodes"] = [
        {"name": "rig_root", "translation": [0.25, 0.5, -0.125], "rotation": quat_z(0.2), "scale": [1.1, 0.9, 1.05], "children": [1, 4, 5, 7]},
        {"name": "ja0", "translation": [0.0, 0.0, 0.0], "children": [2]},
        {"name": "ja1", "translation": [0.0, 1.0, 0.0], "rotation": quat_x(0.1), "children": [3]},
        {"name": "ja2", "translation": [0.0, 1.0, 0.0]},
        {"name": "bar_a", "mesh": 0, "skin": 0, "translation": [0.05, 0.0, 0.1], "scale": [1.0, 1.25, 1.0]},
        {"name": "jb0", "matrix": translation_matrix(1.5, 0.0, 0.25), "children": [6]},
        {"name": "jb1", "translation": [0.0, 1.0, 0.0]},
        {"name": "holder", "translation": [-1.5, 0.0, 0.0], "children": [8, 9, 10]},
        {"name": "bar_b", "mesh": 1, "skin": 1, "rotation": quat_z(-0.15)},
        {"name": "prop", "mesh": 2, "translation": [0.0, 2.0, 0.0], "scale": [0.5, 0.5, 0.5]},
        {"name": "knob", "matrix": translation_matrix(0.0, 0.5, 0.0)}]
    roots = [0]
    if variant == "joint_outside_scene":
        b.doc["nodes"].append({"name": "stray", "translation": [0.0, 3.0, 0.0]})
    if variant == "shared_child":
        b.doc["nodes"][0]["children"].append(10)
    b.add("scenes", {"nodes": roots})
    b.doc["scene"] = 0

    def inverse_binds(ys):
        m = np.zeros((len(ys), 4, 4), np.float32)
        for k, y in enumerate(ys):
            m[k] = np.eye(4, dtype=np.float32)
            m[k][:3, 3] = (0.0, -y, 0.0)
            m[k] = m[k].T.copy()
        return m.reshape(-1, 16)
    b.add("skins", {"joints": [1, 2, 3], "inverseBindMatrices": b.accessor(inverse_binds((0.0, 1.0, 2.0)), "MAT4")})
    b.add("skins", {"joints": [5, 11 if variant == "joint_outside_scene" else 6], "inverseBindMatrices": b.accessor(inverse_binds((0.0, 1.0)), "MAT4")})

    def f32(a):
        return np.array(a, np.float32)
    t2, t3, t5 = f32([0.0, 1.5]), f32([0.25, 1.0, 2.0]), f32([0.0, 0.4, 0.9, 1.3, 2.0])
    if variant == "times_not_increasing":
        t5 = f32([0.0, 0.4, 0.4, 1.3, 2.0])
    near = f32([[0.0, 0.0, 0.0, 1.0], [1e-10, 0.0, 0.0, 1.0]])                                       # theta = 1e-10
    five = f32([quat_x(0.0), [2.0 * c for c in quat_x(0.7)], [-c for c in quat_x(1.1)], [0.5 * c for c in quat_z(0.4)], quat_x(-0.3)])
    three = f32([quat_z(0.0), quat_z(0.9), quat_z(-0.5)])
    three_early = f32([quat_x(0.3), quat_x(0.6), quat_x(0.9)])
    samplers = [
        {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(f32([(0, 0, 0), (0, 0.25, 0), (0.125, 0.5, 0)]), "VEC3"), "interpolation": "STEP"},
        {"input": b.accessor(t2, "SCALAR"), "output": b.accessor(near, "VEC4"), "interpolation": "LINEAR"},
        {"input": b.accessor(t5, "SCALAR"), "output": b.accessor(five, "VEC4")},
        {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(three_early, "VEC4")},
        {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(three, "VEC4"), "interpolation": "CUBICSPLINE" if variant == "cubic" else "LINEAR"},
        {"input": b.accessor(t2, "SCALAR"), "output": b.accessor(f32([(0.05, 0.0, 0.1), (0.3, 0.2, -0.1)]), "VEC3")},
        {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(f32([(1, 1, 1), (1.5, 0.75, 1.25), (0.8, 1.2, 1.0)]), "VEC3")},
        {"input": b.accessor(t3, "SCALAR"), "output": b.accessor(f32([quat_x(0.0), quat_x(0.5), quat_z(0.5)]), "VEC4")},
        {"input": b.accessor(f32([0.75]), "SCALAR"), "output": b.accessor(f32([(0.1, 0.6, -0.2)]), "VEC3")}]
    if variant == "cubic":      # in-tangent, value, out-tangent per key
        samplers[4]["output"] = b.accessor(np.repeat(three, 3, axis=0), "VEC4")
    channels = [{"sampler": 0, "target": {"node": 1, "path": "translation"}}, {"sampler": 1, "target": {"node": 1, "path": "rotation"}},
                {"sampler": 2, "target": {"node": 2, "path": "rotation"}}, {"sampler": 3, "target": {"node": 3, "path": "rotation"}},
                {"sampler": 4, "target": {"node": 3, "path": "rotation"}}, {"sampler": 5, "target": {"node": 4, "path": "translation"}},
                {"sampler": 6, "target": {"node": 6, "path": "scale"}}, {"sampler": 7, "target": {"node": 7, "path": "rotation"}},
                {"sampler": 8, "target": {"node": 10, "path": "translation"}}]
    b.add("animations", {"name": "play", "samplers": samplers, "channels": channels})
    tc = f32([0.0, 1.0, 2.0])
    b.add("animations", {"name": "collapse", "samplers": [
        {"input": b.accessor(tc, "SCALAR"), "output": b.accessor(f32([(1, 1.25, 1), (0, 1.25, 1), (1, 1.25, 1)]), "VEC3")},
        {"input": b.accessor(tc, "SCALAR"), "output": b.accessor(f32([quat_x(0.1), quat_x(0.6), quat_x(0.1)]), "VEC4")}],
        "channels": [{"sampler": 0, "target": {"node": 4, "path": "scale"}}, {"sampler": 1, "target": {"node": 2, "path": "rotation"}}]})
    return b


if __name__ == "__main__":
    out = os.path.join(HERE, "clip_rig.glb")
    build().write_glb(out)
    print(out, os.path.getsize(out), "bytes")
