"""Writes tests/golden/skinned_bar.glb, the rigged fixture of the skinning tests: `python tests/golden/make_skinned_gltf.py`.

Node 0 "rig_root" is translated, rotated and non-uniformly scaled; under it hang a chain of three joints (nodes 1, 2, 3) and the
mesh node 4, which has a translation of its own and wears skin 0 (joints 1, 2, 3, with an inverseBindMatrices accessor). Mesh 0
has two primitives: a bar of 200 vertices along y (JOINTS_0 u16, WEIGHTS_0 f32; rings with 1, 2, 3 and 4 non-zero weights in turn)
and a shorter bar of 48 vertices beside it (JOINTS_0 u8, WEIGHTS_0 normalised u8). Node 5 is an unskinned floor, node 6 an
emissive panel. Animation 0 "bend" turns joints 1 and 2 with LINEAR rotation keys and lifts joint 0 with a STEP translation;
animation 1 "spline" has a CUBICSPLINE sampler. `build(variant)` returns the builder of a broken variant for the loader tests."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from gltf_util import GltfBuilder  # noqa: E402

RING = np.array([(-0.15, -0.15), (0.15, -0.15), (0.15, 0.15), (-0.15, 0.15)], dtype=np.float32)
JOINT_Y = (0.0, 1.0, 2.0)        # joint k sits at y = k in the bind pose (object space of the mesh)


def bar(n_rings, height, x0):
    """A square tube along y: 4 vertices per ring, outward normals, uv = (corner / 4, y / height)."""
    pos, nrm, uv, idx = [], [], [], []
    for r in range(n_rings):
        y = height * r / (n_rings - 1)
        for c, (x, z) in enumerate(RING):
            pos.append((x0 + x, y, z))
            nrm.append((np.sign(x) * np.sqrt(0.5), 0.0, np.sign(z) * np.sqrt(0.5)))
            uv.append((c / 4.0, y / height))
    for r in range(n_rings - 1):
        for c in range(4):
            a, b = 4 * r + c, 4 * r + (c + 1) % 4
            idx += [a, a + 4, b, b, a + 4, b + 4]
    return np.array(pos, np.float32), np.array(nrm, np.float32), np.array(uv, np.float32), np.array(idx, np.uint32)


def float_weights(pos):
    """Per ring in turn: one weight, two, three, four (joint 1 named twice). Rows sum to 1."""
    joints, weights = np.zeros((len(pos), 4), np.uint16), np.zeros((len(pos), 4), np.float32)
    for v, p in enumerate(pos):
        ring, t = v // 4, float(p[1])
        lower = min(int(t), 1)
        f = np.float32(min(max(t - lower, 0.0), 1.0))
        kind = ring % 4
        if kind == 0:
            joints[v], weights[v] = (min(int(t + 0.5), 2), 0, 0, 0), (1.0, 0, 0, 0)
        elif kind == 1:
            joints[v], weights[v] = (lower, lower + 1, 0, 0), (np.float32(1.0) - f, f, 0, 0)
        elif kind == 2:
            joints[v], weights[v] = (0, 1, 2, 0), (0.25, 0.5, 0.25, 0)
        else:
            joints[v], weights[v] = (0, 1, 2, 1), (0.125, 0.375, 0.25, 0.25)
    return joints, weights


def byte_weights(pos):
    """Two joints per vertex, weights in 255ths that sum to 255."""
    joints, weights = np.zeros((len(pos), 4), np.uint8), np.zeros((len(pos), 4), np.uint8)
    for v, p in enumerate(pos):
        t = float(p[1])
        lower = min(int(t), 1)
        w = int(round(255 * min(max(t - lower, 0.0), 1.0)))
        joints[v], weights[v] = (lower, lower + 1, 0, 0), (255 - w, w, 0, 0)
    return joints, weights


def quat_z(angle):
    return [0.0, 0.0, float(np.sin(angle / 2)), float(np.cos(angle / 2))]


def quat_x(angle):
    return [float(np.sin(angle / 2)), 0.0, 0.0, float(np.cos(angle / 2))]


def build(variant=None):
    """variant: None (the fixture) or one of "short_joints", "short_weights", "joint_node_out_of_range", "times_not_increasing",
    "empty_sampler", "short_inverse_bind", "joints_1", "weights_without_joints", "two_skins", "weights_channel", "matrix_node",
    "singular_mesh_node", "short_output"."""
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.6, 0.4, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.6}})
    lamp = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [1.0, 1.0, 1.0, 1.0]}, "emissiveFactor": [1.0, 0.9, 0.8],
                               "extensions": {"KHR_materials_emissive_strength": {"emissiveStrength": 12.0}}})
    # mesh 0: the two skinned bars
    prims = []
    for which, (n_rings, height, x0) in enumerate(((50, 3.0, 0.0), (12, 2.0, 0.6))):
        pos, nrm, uv, idx = bar(n_rings, height, x0)
        joints, weights = float_weights(pos) if which == 0 else byte_weights(pos)
        if variant == "short_joints" and which == 0:
            joints = joints[:-5]
        if variant == "short_weights" and which == 1:
            weights = weights[:-1]
        attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(nrm, "VEC3"), "TEXCOORD_0": b.accessor(uv, "VEC2"),
                 "JOINTS_0": b.accessor(joints, "VEC4"), "WEIGHTS_0": b.accessor(weights, "VEC4", normalized=which == 1)}
        if variant == "joints_1" and which == 0:
            attrs["JOINTS_1"], attrs["WEIGHTS_1"] = attrs["JOINTS_0"], attrs["WEIGHTS_0"]
        if variant == "weights_without_joints" and which == 0:
            del attrs["JOINTS_0"]
        prims.append({"attributes": attrs, "indices": b.accessor(idx, "SCALAR"), "material": grey})
    b.add("meshes", {"primitives": prims})
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
    mesh_node = {"name": "bars", "mesh": 0, "skin": 0, "translation": [0.1, 0.0, -0.05]}
    if variant == "singular_mesh_node":
        mesh_node["scale"] = [1.0, 0.0, 1.0]
    joint1 = {"name": "joint1", "translation": [0.0, 1.0, 0.0], "children": [3]}
    if variant == "matrix_node":        # the same bind transform given as a matrix: the animated channel makes it compose from TRS (the defaults)
        joint1 = {"name": "joint1", "matrix": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.0, 1.0, 0.0, 1], "children": [3]}
    b.doc["nodes"] = [root, {"name": "joint0", "translation": [0.0, 0.0, 0.0], "children": [2]}, joint1,
                      {"name": "joint2", "translation": [0.0, 1.0, 0.0]}, mesh_node,
                      {"name": "floor", "mesh": 1}, {"name": "panel", "mesh": 2, "translation": [0.5, 0.0, 0.0]}]
    roots = [0, 5, 6]
    if variant == "two_skins":          # a second node instances the same mesh under another skin
        b.doc["nodes"].append({"name": "bars_again", "mesh": 0, "skin": 1, "translation": [2.0, 0.0, 0.0]})
        roots.append(7)
    b.add("scenes", {"nodes": roots})
    b.doc["scene"] = 0
    # skin 0: inverse bind = inverse(bind transform of the joint in the mesh's object space), here a translation down the bar
    ibm = np.zeros((3, 4, 4), np.float32)
    for k, y in enumerate(JOINT_Y):
        m = np.eye(4, dtype=np.float32)
        m[:3, 3] = (0.1, -y, -0.05)          # the mesh node's own translation comes back in: joint space -> mesh space at bind
        ibm[k] = m.T                         # column-major in the file
    if variant == "short_inverse_bind":
        ibm = ibm[:2]
    skin = {"joints": [1, 2, 3], "inverseBindMatrices": b.accessor(ibm.reshape(-1, 16), "MAT4"), "skeleton": 1}
    if variant == "joint_node_out_of_range":
        skin["joints"] = [1, 2, 40]
    b.add("skins", skin)
    if variant == "two_skins":
        b.add("skins", {"joints": [1, 2, 3]})
    # animation 0
    t_rot = np.array([0.0, 0.5, 1.25, 2.0], np.float32)
    if variant == "times_not_increasing":
        t_rot = np.array([0.0, 0.5, 0.5, 2.0], np.float32)
    r1 = np.array([quat_z(0.0), quat_z(0.6), quat_z(-0.4), quat_z(0.0)], np.float32)
    r2 = np.array([quat_x(0.0), quat_x(-0.5), [-x for x in quat_x(0.9)], quat_x(0.2)], np.float32)      # a negated key: the shorter arc
    t_step = np.array([0.25, 1.0, 1.5], np.float32)
    lift = np.array([(0, 0, 0), (0, 0.25, 0), (0.1, 0.5, 0)], np.float32)
    if variant == "short_output":
        r1 = r1[:3]
    samplers = [{"input": b.accessor(t_rot, "SCALAR"), "output": b.accessor(r1, "VEC4"), "interpolation": "LINEAR"},
                {"input": b.accessor(t_rot, "SCALAR"), "output": b.accessor(r2, "VEC4")},                # LINEAR is the default
                {"input": b.accessor(t_step, "SCALAR"), "output": b.accessor(lift, "VEC3"), "interpolation": "STEP"}]
    if variant == "empty_sampler":
        for key in ("input", "output"):
            b.doc["accessors"][samplers[2][key]]["count"] = 0
    channels = [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}, {"sampler": 1, "target": {"node": 3, "path": "rotation"}},
                {"sampler": 2, "target": {"node": 1, "path": "translation"}}]
    if variant == "weights_channel":
        samplers.append({"input": b.accessor(t_step, "SCALAR"), "output": b.accessor(np.array([0.0, 1.0, 0.0], np.float32), "SCALAR")})
        channels.append({"sampler": 3, "target": {"node": 4, "path": "weights"}})
    b.add("animations", {"name": "bend", "samplers": samplers, "channels": channels})
    # animation 1: CUBICSPLINE (in-tangent, value, out-tangent per key)
    t_cs = np.array([0.0, 1.0], np.float32)
    zero = [0.0, 0.0, 0.0, 0.0]
    cs = np.array([zero, quat_z(0.0), zero, zero, quat_z(0.8), zero], np.float32)
    b.add("animations", {"name": "spline", "samplers": [{"input": b.accessor(t_cs, "SCALAR"), "output": b.accessor(cs, "VEC4"), "interpolation": "CUBICSPLINE"}],
                         "channels": [{"sampler": 0, "target": {"node": 2, "path": "rotation"}}]})
    return b


if __name__ == "__main__":
    out = os.path.join(HERE, "skinned_bar.glb")
    build().write_glb(out)
    print(out, os.path.getsize(out), "bytes")
