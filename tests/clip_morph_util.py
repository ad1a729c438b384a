"""Shared by the tests of baked morph-weight sets: the fixture, the times a set is evaluated at, the host's compaction of a weight
vector into an active list, and a generated file whose sets have the shapes at which the device kernel can go wrong. Nothing here
needs a GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from gltf_util import GltfBuilder  # noqa: E402

MORPH_BAR = os.path.join(HERE, "golden", "morph_bar.glb")
UNAVAILABLE = 2                         # abi.CLIP_MORPH_UNAVAILABLE
ZEROS_AT = (0, 63, 64, 127, 128, 129)   # targets of the big set whose weight is exactly 0 at key 1: the ends of the chunks of 64
BIG, ONE, TWO = 0, 1, 2                 # the blases of many_targets(): 130 targets, 1 target, 2 targets
BIG_TIMES = (0.0, 0.5, 1.0, 2.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def available_sets(clip, n_blases):
    """The blases of the clip's available morph sets."""
    out = []
    for b in range(n_blases):
        try:
            if clip.morph(b)["state"] != UNAVAILABLE:
                out.append(b)
        except Exception:
            pass
    return out


def set_times(clip, blas):
    """test_clip_host.py's grid over the set's own keys: -1, 0, every key time, nextafter on both sides of every key, the midpoint
    and three more points between consecutive keys, and beyond the end: float32, ascending, each once."""
    keys = clip.morph_keys(blas)[0]
    ts = {-1.0, 0.0, float(clip.info.duration_seconds) + 1.5, (float(keys[-1]) if len(keys) else 0.0) + 1.5}
    for k in keys:
        ts.update((float(k), float(np.nextafter(k, np.float32(-np.inf))), float(np.nextafter(k, np.float32(np.inf)))))
    for a, b in zip(keys[:-1], keys[1:]):
        for u in (0.5, 0.0625, 0.25, 0.8125):
            ts.add(float(a + np.float32(u) * (b - a)))
    return sorted(float(np.float32(t)) for t in ts)


def compact(weights):
    """The host's active list of a weight vector (check_pose_args of api.cpp): the targets whose weight is not 0, ascending, and
    their weights; +0 and -0 are left out."""
    w = np.ascontiguousarray(weights, np.float32)
    at = np.flatnonzero(w != 0.0).astype(np.uint32)
    return at, w[at]


def big_keys():
    """The 4 x 130 key values of the big set: key 0 all zeros; key 1 zeros at ZEROS_AT and a -0 at target 5; key 2 nothing zero;
    key 3 zeros at the even targets, a -0 at target 66."""
    k = np.arange(130, dtype=np.float32)
    v = np.zeros((4, 130), np.float32)
    v[1] = 0.01 * (k + 1.0)
    v[1, list(ZEROS_AT)] = 0.0
    v[1, 5] = -0.0
    v[2] = 0.25 + 0.005 * k
    v[3] = np.where(k % 2 == 1, -0.125 - 0.001 * k, 0.0)
    v[3, 66] = -0.0
    assert np.signbit(v[1, 5]) and np.signbit(v[3, 66]) and (v[2] != 0).all()
    return v


def quad(b, material, n_targets, salt):
    """A quad of four vertices with n_targets POSITION-only morph targets -> mesh index."""
    pos = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5)], np.float32)
    attrs = {"POSITION": b.accessor(pos, "VEC3"), "NORMAL": b.accessor(np.tile(np.array((0, 1, 0), np.float32), (4, 1)), "VEC3"),
             "TEXCOORD_0": b.accessor(np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32), "VEC2")}
    targets = []
    for k in range(n_targets):
        d = np.zeros((4, 3), np.float32)
        d[:, 1] = 0.001 * (1 + (k + salt) % 7)
        d[k % 4, 0] = 0.002 * (1 + k % 5)
        targets.append({"POSITION": b.accessor(d, "VEC3")})
    return b.add("meshes", {"primitives": [{"attributes": attrs, "indices": b.accessor(np.array([0, 2, 1, 0, 3, 2], np.uint32), "SCALAR"), "material": material,
                                            "targets": targets}]})


def many_targets(path):
    """Writes a file of three morphed quads, each on a root node of its own. Blas BIG has 130 targets (chunks of 64 + 64 + 2) and
    default weights; blas ONE one target; blas TWO two targets. Animation 0: BIG on a LINEAR channel of big_keys() at BIG_TIMES,
    ONE on a one-key channel (the weight 2), TWO on a LINEAR channel of two keys. Animation 1: BIG on a STEP channel of the same
    keys, ONE on a STEP channel of three keys, TWO on no channel (its defaults)."""
    b = GltfBuilder()
    b.doc["animations"] = []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0]}})
    counts = {BIG: 130, ONE: 1, TWO: 2}
    for blas in (BIG, ONE, TWO):
        mesh = quad(b, grey, counts[blas], blas)
        node = {"name": "quad%d" % blas, "mesh": mesh, "translation": [1.5 * blas, 0.0, 0.0]}
        if blas == BIG:
            node["weights"] = [0.0 if k % 3 == 0 else 0.002 * k for k in range(130)]
        if blas == TWO:
            node["weights"] = [0.75, 0.0]
        b.add("nodes", node)
    b.add("scenes", {"nodes": [0, 1, 2]})
    b.doc["scene"] = 0
    big_t, big_v = b.accessor(np.array(BIG_TIMES, np.float32), "SCALAR"), b.accessor(big_keys().reshape(-1), "SCALAR")
    one_key = {"input": b.accessor(np.array([0.75], np.float32), "SCALAR"), "output": b.accessor(np.array([2.0], np.float32), "SCALAR")}
    two_keys = {"input": b.accessor(np.array([0.25, 1.25], np.float32), "SCALAR"), "output": b.accessor(np.array([0.0, 0.5, 1.0, 0.0], np.float32), "SCALAR")}
    step3 = {"input": b.accessor(np.array([0.0, 1.0, 3.0], np.float32), "SCALAR"), "output": b.accessor(np.array([0.5, 0.0, -0.0], np.float32), "SCALAR"),
             "interpolation": "STEP"}
    b.add("animations", {"name": "linear", "samplers": [{"input": big_t, "output": big_v, "interpolation": "LINEAR"}, one_key, two_keys],
                         "channels": [{"sampler": s, "target": {"node": s, "path": "weights"}} for s in range(3)]})
    b.add("animations", {"name": "step", "samplers": [{"input": big_t, "output": big_v, "interpolation": "STEP"}, step3],
                         "channels": [{"sampler": s, "target": {"node": s, "path": "weights"}} for s in range(2)]})
    b.write_glb(path)
    return counts


def one_morphed_quad(path, n_targets, n_keys=4):
    """Writes a file of one quad with n_targets morph targets on one root node, driven by a LINEAR `weights` channel of n_keys keys
    a quarter of a second apart; every key value is other than 0. -> the clip's duration in seconds."""
    b = GltfBuilder()
    b.doc["animations"] = []
    grey = b.add("materials", {"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.8, 0.8, 1.0]}})
    b.add("nodes", {"name": "quad", "mesh": quad(b, grey, n_targets, 0)})
    b.add("scenes", {"nodes": [0]})
    b.doc["scene"] = 0
    times = (0.25 * np.arange(n_keys)).astype(np.float32)
    values = (0.05 + 0.01 * ((np.arange(n_keys)[:, None] * 7 + np.arange(n_targets)[None, :] * 3) % 11)).astype(np.float32)
    b.add("animations", {"name": "flex", "samplers": [{"input": b.accessor(times, "SCALAR"), "output": b.accessor(values.reshape(-1), "SCALAR")}],
                         "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]})
    b.write_glb(path)
    return float(times[-1])
