"""Writes tests/golden/morph_bar.glb, the fixture of the morph-target tests: `python tests/golden/make_morph_gltf.py`.

The rig is that of skinned_bar.glb: node 0 "rig_root" (translated, rotated, non-uniformly scaled), under it the joint chain (nodes
1, 2, 3) and the mesh node 4, which wears skin 0. Mesh 0 is one bar of 200 vertices that is both skinned and morphed: three
targets (0: POSITION only, a bulge; 1: POSITION + NORMAL, a twist; 2: POSITION + NORMAL + TANGENT through sparse accessors that
touch every seventh vertex, one of them without a bufferView) and mesh.weights. Mesh 1 is an unskinned bar of 48 vertices with two
targets and mesh.weights that its node 5 overrides with `weights` of its own. Node 6 is a floor, node 7 an emissive panel.
Animation 0 "talk" turns joint 1 (LINEAR rotation), drives mesh 0's weights with a LINEAR `weights` channel and mesh 1's with a
STEP one; animation 1 "spline" has a CUBICSPLINE `weights` channel on node 4. `build(variant)` returns the builder of a broken
variant for the loader tests."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from gltf_util import GltfBuilder  # noqa: E402
from make_skinned_gltf import JOINT_Y, bar, float_weights, quat_z  # noqa: E402

VARIANTS = ("short_target", "integer_target", "texcoord_target", "short_output", "node_weights_differ", "times_not_increasing", "counts_disagree")


def sparse_accessor(b, count, at, values, with_view):
    """A float VEC3 accessor of `count` elements, zeros (an explicit bufferView of zeros when with_view, none otherwise) with
    `values` substituted at the indices `at` (u16)."""
    acc = {"componentType": 5126, "count": count, "type": "VEC3",
           "sparse": {"count": len(at), "indices": {"bufferView": b.view(np.asarray(at, np.uint16).tobytes()), "componentType": 5123},
                      "values": {"bufferView": b.view(np.ascontiguousarray(values, np.float32).tobytes())}}}
    if with_view:
        acc["bufferView"] = b.view(np.zeros((count, 3), np.float32).tobytes())
    b.doc["accessors"].append(acc)
    return len(b.doc["accessors"]) - 1


def bar_targets(pos, nrm):
    """The deltas of the three targets of the big bar -> (bulge position, twist position, twist normal, sparse indices, sparse
    position / normal / tangent values)."""
    y = pos[:, 1:2]
    out = np.concatenate([nrm[:, 0:1], np.zeros_like(y), nrm[:, 2:3]], axis=1)
    bulge = (out * (0.2 * np.sin(np.pi * y / 3.0))).astype(np.float32)
    a = 0.5 * y / 3.0                                                     # a twist about the bar's axis that grows with the height
    c, s = np.cos(a), np.sin(a)
    rot = lambda v: np.concatenate([c * v[:, 0:1] + s * v[:, 2:3], v[:, 1:2], -s * v[:, 0:1] + c * v[:, 2:3]], axis=1)   # noqa: E731
    twist_p, twist_n = (rot(pos) - pos).astype(np.float32), (rot(nrm) - nrm).astype(np.float32)
    at = np.arange(3, len(pos), 7)
    sp = np.stack([0.05 * np.cos(at), 0.1 + 0.0 * at, 0.05 * np.sin(at)], axis=1).astype(np.float32)
    sn = np.stack([0.0 * at, 0.5 + 0.0 * at, 0.0 * at], axis=1).astype(np.float32)
    st = np.stack([0.0 * at, 0.0 * at, 0.75 + 0.0 * at], axis=1).astype(np.float32)
    return bulge, twist_p, twist_n, at, sp, sn, st


def build(variant=None):
    """variant: None (the fixture) or one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.6, 0.4, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}})
    lamp = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0]}, "emissiveFactor": [1.0, 0.9, 0.8],
                               "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}}})
    # mesh 0: the bar that is skinned and morphed
    pos, nrm, uv, idx = bar(50, 3.0, 0.0)
    tan = np.tile(np.array((0, 1, 0, 1), np.float32), (len(pos), 1))
    joints, weights = float_weights(pos)
    bulge, twist_p, twist_n, at, sp, sn, st = bar_targets(pos, nrm)
    if variant == "short_target":
        twist_n = twist_n[:-3]
    if variant == "counts_disagree":                          # long enough for the mesh, but not the count of the other accessors
        bulge = np.concatenate([bulge, bulge[:2]])
    t0 = {"POSITION": b.accessor(bulge, "VEC3")}
    t1 = {"POSITION": b.accessor(twist_p, "VEC3"), "NORMAL": b.accessor(twist_n, "VEC3")}
    if variant == "integer_target":
        t1["NORMAL"] = b.accessor(np.zeros((len(pos), 3), np.int16), "VEC3", normalized=True)
    t2 = {"POSITION": sparse_accessor(b, len(pos), at, sp, True), "NORMAL": sparse_accessor(b, len(pos), at, sn, False),
          "TANGENT": sparse_accessor(b, len(pos), at, st, True)}
    if variant == "texcoord_target":
        t2["TEXCOORD_0"] = b.accessor(np.zeros((len(pos), 2), np.float32), "VEC2")
    attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(nrm, "VEC3"), "TANGENT": b.accessor(tan, "VEC4"), "TEXCOORD_0": b.accessor(uv, "VEC2"),
             "JOINTS_0": b.accessor(joints, "VEC4"), "WEIGHTS_0": b.accessor(weights, "VEC4")}
    b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(idx, "SCALAR"), "material": grey, "targets": [t0, t1, t2]}],
                     "weights": [0.25, 0.0, 0.5]})
    # mesh 1: the unskinned bar with two targets
    pos1, nrm1, uv1, idx1 = bar(12, 2.0, 0.0)
    lean = np.concatenate([0.3 * (pos1[:, 1:2] / 2.0) ** 2, np.zeros((len(pos1), 2), np.float32)], axis=1).astype(np.float32)
    swell = (np.concatenate([nrm1[:, 0:1], np.zeros((len(pos1), 1), np.float32), nrm1[:, 2:3]], axis=1) * 0.1).astype(np.float32)
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(pos1, "VEC3"), "NORMAL": b.accessor(nrm1, "VEC3"), "TEXCOORD_0": b.accessor(uv1, "VEC2")},
                                     "indices": b.accessor(idx1, "SCALAR"), "material": grey,
                                     "targets": [{"POSITION": b.accessor(lean, "VEC3")}, {"POSITION": b.accessor(swell, "VEC3"), "NORMAL": b.accessor(-0.25 * nrm1, "VEC3")}]}],
                     "weights": [0.125, 0.75]})
    floor_pos = np.array([(-3, -0.5, -3), (3, -0.5, -3), (3, -0.5, 3), (-3, -0.5, 3)], np.float32)
    up = np.tile(np.array((0, 1, 0), np.float32), (4, 1))
    quad_uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(floor_pos, "VEC3"), "NORMAL": b.accessor(up, "VEC3"), "TEXCOORD_0": b.accessor(quad_uv, "VEC2")},
                                     "indices": b.accessor(np.array([0, 2, 1, 0, 3, 2], np.uint32), "SCALAR"), "material": grey}]})
    panel_pos = np.array([(-1, 4.5, -1), (1, 4.5, -1), (1, 4.5, 1), (-1, 4.5, 1)], np.float32)
    b.add("meshes", {"primitives": [{"attributes": {"POSITION": b.accessor(panel_pos, "VEC3"), "NORMAL": b.accessor(-up, "VEC3"), "TEXCOORD_0": b.accessor(quad_uv, "VEC2")},
                                     "indices": b.accessor(np.array([0, 1, 2, 0, 2, 3], np.uint32), "SCALAR"), "material": lamp}]})
    # nodes
    root = {"name": "rig_root", "translation": [0.5, -0.25, 0.1], "rotation": quat_z(0.3), "scale": [1.2, 0.8, 1.1], "children": [1, 4]}
    b.doc["nodes"] = [root, {"name": "joint0", "translation": [0.0, 0.0, 0.0], "children": [2]}, {"name": "joint1", "translation": [0.0, 1.0, 0.0], "children": [3]},
                      {"name": "joint2", "translation": [0.0, 1.0, 0.0]}, {"name": "bar", "mesh": 0, "skin": 0, "translation": [0.1, 0.0, -0.05]},
                      {"name": "plain_bar", "mesh": 1, "translation": [1.4, -0.5, 0.3], "weights": [0.5, 0.25]},
                      {"name": "floor", "mesh": 2}, {"name": "panel", "mesh": 3, "translation": [0.5, 0.0, 0.0]}]
    roots = [0, 5, 6, 7]
    if variant == "node_weights_differ":                      # a second node instances mesh 1 and takes the mesh's own weights
        b.doc["nodes"].append({"name": "plain_bar_again", "mesh": 1, "translation": [-1.4, -0.5, 0.3]})
        roots.append(8)
    b.add("scenes", {"nodes": roots})
    b.doc["scene"] = 0
    ibm = np.zeros((3, 4, 4), np.float32)
    for k, y in enumerate(JOINT_Y):
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = (0.1, -y, -0.05)
        ibm[k] = m.T
    b.add("skins", {"joints": [1, 2, 3], "inverseBindMatrices": b.accessor(ibm.reshape(-1, 16), "MAT4"), "skeleton": 1})
    # animation 0
    t_rot = np.array([0.0, 0.5, 1.25, 2.0], np.float32)
    r1 = np.array([quat_z(0.0), quat_z(0.6), quat_z(-0.4), quat_z(0.0)], np.float32)
    t_w = np.array([0.0, 0.4, 1.1, 2.0], np.float32)
    if variant == "times_not_increasing":
        t_w = np.array([0.0, 1.1, 0.4, 2.0], np.float32)
    w0 = np.array([(0.0, 0.0, 0.0), (1.0, 0.25, 0.0), (0.3, -0.5, 1.0), (0.0, 1.5, 0.6)], np.float32)      # a key of all zeros, weights below 0 and above 1
    if variant == "short_output":
        w0 = w0.reshape(-1)[:-1]
    t_step = np.array([0.25, 1.0, 1.5], np.float32)
    w1 = np.array([(0.0, 1.0), (0.7, 0.0), (1.0, 0.4)], np.float32)
    samplers = [{"input": b.accessor(t_rot, "SCALAR"), "output": b.accessor(r1, "VEC4"), "interpolation": "LINEAR"},
                {"input": b.accessor(t_w, "SCALAR"), "output": b.accessor(w0.reshape(-1), "SCALAR"), "interpolation": "LINEAR"},
                {"input": b.accessor(t_step, "SCALAR"), "output": b.accessor(w1.reshape(-1), "SCALAR"), "interpolation": "STEP"}]
    channels = [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}, {"sampler": 1, "target": {"node": 4, "path": "weights"}},
                {"sampler": 2, "target": {"node": 5, "path": "weights"}}]
    b.add("animations", {"name": "talk", "samplers": samplers, "channels": channels})
    # animation 1: CUBICSPLINE weights (in-tangent, value, out-tangent per key and target)
    t_cs = np.array([0.0, 1.0], np.float32)
    cs = np.zeros((2, 3, 3), np.float32)
    cs[1, 1] = (1.0, 0.5, 0.25)
    b.add("animations", {"name": "spline", "samplers": [{"input": b.accessor(t_cs, "SCALAR"), "output": b.accessor(cs.reshape(-1), "SCALAR"), "interpolation": "CUBICSPLINE"}],
                         "channels": [{"sampler": 0, "target": {"node": 4, "path": "weights"}}]})
    return b


if __name__ == "__main__":
    out = os.path.join(HERE, "morph_bar.glb")
    build().write_glb(out)
    print(out, os.path.getsize(out), "bytes")
