"""Shared by the baked-clip tests: the fixture, the times every clip is evaluated at, rigs of a given shape built with GltfBuilder,
and a crowd of copies of a file as a scene description. Nothing here needs a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from gltf_util import GltfBuilder  # noqa: E402

CLIP_RIG = os.path.join(HERE, "golden", "clip_rig.glb")
SKINNED_BAR = os.path.join(HERE, "golden", "skinned_bar.glb")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def clip_times(clip):
    """-1, 0, every key time of the clip, nextafter on both sides of every key, the midpoint and three more points between
    consecutive keys, and beyond the end: float32, ascending, each once."""
    ts = {-1.0, 0.0, float(clip.info.duration_seconds) + 1.5}
    for c in range(clip.info.n_channels):
        keys = clip.channel_keys(c)[0]
        for k in keys:
            ts.update((float(k), float(np.nextafter(k, np.float32(-np.inf))), float(np.nextafter(k, np.float32(np.inf)))))
        for a, b in zip(keys[:-1], keys[1:]):
            for u in (0.5, 0.0625, 0.25, 0.8125):                          # the midpoint, and three more points of the interval
                ts.add(float(a + np.float32(u) * (b - a)))
    return sorted(float(np.float32(t)) for t in ts)


def rotation_classes(clip, time):
    """Per clip node: 0 where the node's rotation is not sampled or is in the bit-equal class at `time` (STEP, clamped, an exact
    key time, a one-key channel), 1 where it is interpolated."""
    nodes, chans, _ = clip.layout()
    out = np.zeros(len(nodes), np.uint32)
    t = np.float64(np.float32(time))
    for c, ch in enumerate(chans):
        if ch["path"] != 1:
            continue
        keys = clip.channel_keys(c)[0].astype(np.float64)
        inside = keys[0] < t < keys[-1] and not (keys == t).any()
        out[ch["node"]] = 1 if inside and ch["interpolation"] == 0 else 0
    return out


def assert_trs_contract(got, want, interpolated, what):
    """The numerics contract of a device TRS against the host rule -> (rotation components not bit equal, interpolated rotation
    components). Everything but an interpolated rotation is bit equal; such a component is the host's, its neighbouring float32,
    or within 2^-44 of it."""
    for name in ("translation", "scale", "animated"):
        assert np.array_equal(bits(got[name]), bits(want[name])), "%s: %s differs from the host rule" % (what, name)
    g, w = got["rotation"], want["rotation"]
    fixed = interpolated == 0
    assert np.array_equal(bits(g[fixed]), bits(w[fixed])), "%s: a rotation of the bit-equal class differs" % what
    gi, wi = g[~fixed], w[~fixed]
    differ = bits(gi) != bits(wi)
    neighbour = (gi == np.nextafter(wi, np.float32(np.inf))) | (gi == np.nextafter(wi, np.float32(-np.inf)))
    close = np.abs(gi.astype(np.float64) - wi.astype(np.float64)) <= 2.0 ** -44
    assert (~differ | neighbour | close).all(), "%s: an interpolated rotation component is neither the host's, its neighbour nor within 2^-44" % what
    return int(differ.sum()), int(differ.size)


def tiny_mesh(b, material, skinned_joints=0):
    """A quad of four vertices; with skinned_joints > 0, every vertex names joints 0 and the last one."""
    pos = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)], np.float32)
    attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(np.tile(np.array((0, 1, 0), np.float32), (4, 1)), "VEC3"),
             "TEXCOORD_0": b.accessor(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32), "VEC2")}
    if skinned_joints:
        joints = np.tile(np.array((0, skinned_joints - 1, 0, 0), np.uint16), (4, 1))
        attrs["JOINTS_0"] = b.accessor(joints, "VEC4")
        attrs["WEIGHTS_0"] = b.accessor(np.tile(np.array((0.75, 0.25, 0, 0), np.float32), (4, 1)), "VEC4")
    return b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(np.array([0, 2, 1, 0, 3, 2], np.uint32), "SCALAR"), "material": material}]})


def quat(axis, angle):
    v = [0.0, 0.0, 0.0, float(np.cos(angle / 2))]
    v[axis] = float(np.sin(angle / 2))
    return v


def shape_rig(path, chain=0, fan=0, joints=0, channels=0, keys=2, plain_mesh=True):
    """Writes a rig of a given shape: node 0 is the root and carries an unskinned quad (plain_mesh); under it a chain of `chain`
    nodes, each the child of the one before, and `fan` more children of the root; with joints > 0 one more child, a skinned quad
    whose skin names `joints` of the chain and fan nodes (round robin). `channels` channels go round the chain and fan nodes (then
    the root), rotation then translation then scale per node, LINEAR with `keys` keys each (rotations: unnormalised, turning
    about changing axes) on key times that differ from channel to channel. -> the number of nodes."""
    b = GltfBuilder()
    b.doc["skins"], b.doc["animations"] = [], []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0]}})
    nodes = [{"name": "root", "translation": [0.1, 0.2, 0.3], "rotation": quat(2, 0.1), "children": []}]
    if plain_mesh:
        nodes[0]["mesh"] = tiny_mesh(b, grey)
    for k in range(chain):
        nodes.append({"name": "c%d" % k, "translation": [0.01, 0.02 + 0.001 * k, 0.0], "rotation": quat(k % 3, 0.02 * (k % 7))})
        nodes[k]["children"] = nodes[k].get("children", []) + [k + 1]
    for k in range(fan):
        nodes.append({"name": "f%d" % k, "translation": [0.05 * k, 0.0, 0.1], "scale": [1.0, 1.0 + 0.01 * (k % 5), 1.0]})
        nodes[0]["children"].append(len(nodes) - 1)
    movers = list(range(1, len(nodes))) or [0]
    if joints:
        mesh_node = {"name": "skinned", "mesh": tiny_mesh(b, grey, joints), "skin": 0, "translation": [0.0, 0.5, 0.0]}
        nodes.append(mesh_node)
        nodes[0]["children"].append(len(nodes) - 1)
        b.add("skins", {"joints": [movers[j % len(movers)] for j in range(joints)]})
    if not nodes[0]["children"]:
        del nodes[0]["children"]
    b.doc["nodes"] = nodes
    b.add("scenes", {"nodes": [0]})
    b.doc["scene"] = 0
    samplers, chans = [], []
    for c in range(channels):
        node, target = movers[c % len(movers)], ("rotation", "translation", "scale")[(c // len(movers)) % 3]
        times = (np.arange(keys, dtype=np.float32) * np.float32(0.125) + np.float32(0.01 * (c % 9))).astype(np.float32)
        if target == "rotation":
            vals = np.array([[(1.0 + 0.25 * (k % 3)) * x for x in quat((c + k) % 3, 0.3 * k - 0.2 * (c % 5))] for k in range(keys)], np.float32)
        else:
            vals = np.array([(1.0 + 0.01 * k, 1.0 - 0.02 * (c % 4), 1.0 + 0.005 * k * (c % 3)) for k in range(keys)], np.float32)
        samplers.append({"input": b.accessor(times, "SCALAR"), "output": b.accessor(vals, "VEC4" if target == "rotation" else "VEC3")})
        chans.append({"sampler": c, "target": {"node": node, "path": target}})
    if channels:
        b.add("animations", {"name": "move", "samplers": samplers, "channels": chans})
    b.write_glb(path)
    return len(nodes)


def crowd(rt, path, copies):
    """`copies` copies of a file as one scene description: keys 1000 * copy + blas + 1 -> (desc, open Gltf, per copy the keys by
    blas, {key: (influences, joint count)} of the skinned meshes, the layout [(key, count)] in key order, the rows of one copy's
    instances in that layout counted from the copy's first row, the skin of every blas or -1, the blas of every instance)."""
    from sunray_amd import scenes
    parsed = rt.gltf_parse(path)
    g = rt.Gltf(path)
    desc = scenes.SceneDesc(os.path.basename(path))
    ib = np.array([b for b, _ in parsed["instances"]], np.uint32)
    order = np.argsort(ib, kind="stable")
    rows = np.zeros(len(ib), np.uint32)
    rows[order] = np.arange(len(ib), dtype=np.uint32)
    skins = [g.blas_skin(b)[0] for b in range(g.n_blases)]
    keys, rigs, layout = [], {}, []
    for c in range(copies):
        keys.append([1000 * c + b + 1 for b in range(g.n_blases)])
        for b, blas in enumerate(parsed["blases"]):
            key = keys[c][b]
            desc.meshes.append(scenes.MeshDesc(key, blas["vertices"], blas["indices"], blas["material"].copy()))
            if skins[b] >= 0:
                rigs[key] = (g.blas_skin(b)[1], len(g.skin(skins[b])[1]))
            xf = [t for bb, t in parsed["instances"] if bb == b]
            desc.instances.append((key, xf))
            layout.append((key, len(xf)))
    return desc, g, keys, rigs, layout, rows, skins, ib
