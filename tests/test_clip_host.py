"""Baked clips on the host (sr_gltf_bake_clip, sr_clip_sample_host, sr_clip_compose_host, sr_clip_pose_host): the flat restatement
of sr_gltf_pose is held to it bit for bit, on both rigged fixtures, for every animation and the static pose, every skin and the
instance transforms, at every key time, next to every key, between the keys and outside them. No GPU."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, runtime as rt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_util import CLIP_RIG, SKINNED_BAR, bits, clip_times, shape_rig  # noqa: E402  (puts tests/golden on the path)
import make_clip_gltf  # noqa: E402

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
SINGULAR = "gltf: the transform of the skinned mesh's node is singular"


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def bakeable(g):
    """(animation, clip) for -1 and every animation of the file that has no CUBICSPLINE sampler."""
    out = [(-1, g.bake_clip(-1))]
    for a in range(g.rig_counts()[1]):
        try:
            out.append((a, g.bake_clip(a)))
        except rt.SunrayError as e:
            assert e.code == ERR_UNSUPPORTED and "CUBICSPLINE" in e.description
    return out


def test_the_committed_fixture_is_what_the_generator_writes(tmp_path):
    path = str(tmp_path / "again.glb")
    make_clip_gltf.build().write_glb(path)
    assert open(path, "rb").read() == open(CLIP_RIG, "rb").read()
    assert os.path.getsize(CLIP_RIG) < 32 * 1024


@pytest.mark.parametrize("path", [SKINNED_BAR, CLIP_RIG], ids=["skinned_bar", "clip_rig"])
def test_pose_host_equals_gltf_pose_bit_for_bit(path):
    g = rt.Gltf(path)
    n_skins = g.rig_counts()[0]
    clips = bakeable(g)
    assert len(clips) == (2 if path == SKINNED_BAR else 3)
    n_times = n_singular = 0
    for a, clip in clips:
        worn = [(s,) + clip.skin(s) for s in range(n_skins)]
        for t in clip_times(clip):
            n_times += 1
            want_xf = g.pose(a, t)[0]
            want, singular = {}, []
            for s, first, n in worn:
                try:
                    want[s] = g.pose(a, t, s)[1]
                except rt.SunrayError as e:
                    assert (e.code, e.description) == (ERR_UNSUPPORTED, "sr_gltf_pose: " + SINGULAR)
                    singular.append(s)
            assert np.array_equal(bits(clip.pose_host(t, joints=False)[1]), bits(want_xf)), (a, t)
            trs = clip.sample_host(t)
            jm, xf, bad = clip.compose_host(trs)
            assert np.array_equal(bits(xf), bits(want_xf)), (a, t)
            if singular:
                n_singular += 1
                assert bad == singular[0] == [s for s, _, _ in worn].index(singular[0])
                assert refused(lambda: clip.pose_host(t)) == (ERR_UNSUPPORTED, "sr_clip_pose_host: " + SINGULAR)
            else:
                assert bad is None
                got, got_xf = clip.pose_host(t)
                assert np.array_equal(bits(got), bits(jm)) and np.array_equal(bits(got_xf), bits(want_xf))
            for s, first, n in worn:
                if s not in singular:
                    assert np.array_equal(bits(jm[first:first + n]), bits(want[s])), (a, t, s)
    assert n_times > (20 if path == SKINNED_BAR else 40)
    assert n_singular == (0 if path == SKINNED_BAR else 1)          # animation 1 of clip_rig at t = 1: the mesh node's scale is 0


@pytest.mark.parametrize("path", [SKINNED_BAR, CLIP_RIG], ids=["skinned_bar", "clip_rig"])
def test_sample_host_equals_sample_node_bit_for_bit(path):
    g = rt.Gltf(path)
    for a, clip in bakeable(g):
        nodes = clip.layout()[0]
        for t in clip_times(clip):
            trs = clip.sample_host(t)
            for n, node in enumerate(nodes):
                tr, q, sc, mask = g.sample_node(a, t, int(node["gltf_node"]))
                assert (bits(trs[n]["translation"]).tolist(), bits(trs[n]["rotation"]).tolist(), bits(trs[n]["scale"]).tolist(), int(trs[n]["animated"])) == (
                    bits(tr).tolist(), bits(q).tolist(), bits(sc).tolist(), mask), (a, t, n)


def mul4(a, b):
    """The loader's product on 4x4, float32, k = 0..3 in order."""
    r = np.zeros((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            r[i, j] = np.float32(np.float32(np.float32(a[i, 0] * b[0, j]) + np.float32(a[i, 1] * b[1, j])) + np.float32(a[i, 2] * b[2, j])) + np.float32(a[i, 3] * b[3, j])
    return r


def test_a_placement_composes_as_mul_does():
    g = rt.Gltf(CLIP_RIG)
    clip = g.bake_clip(0)
    placement = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)
    P = np.vstack([placement.reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)])
    for t in (0.0, 0.37, 1.0):
        jm0, xf0 = clip.pose_host(t)
        jm1, xf1 = clip.pose_host(t, placement=placement)
        assert np.array_equal(bits(jm0), bits(jm1))                     # the joint matrices do not see it
        for i in range(len(xf0)):
            G = np.vstack([xf0[i].reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)])
            assert np.array_equal(bits(mul4(P, G)[:3].reshape(12)), bits(xf1[i])), (t, i)


def test_bake_layout():
    g = rt.Gltf(CLIP_RIG)
    clip = g.bake_clip(0)
    i = clip.info
    assert (i.animation, i.n_nodes, i.n_levels, i.n_channels, i.n_skins, i.n_joints, i.n_instances) == (0, 11, 4, 8, 2, 5, 3)
    assert i.duration_seconds == 2.0 and i.device_bytes % 16 == 0
    nodes, chans, inst = clip.layout()
    assert nodes["gltf_node"].tolist() == [0, 1, 4, 5, 7, 2, 6, 8, 9, 10, 3]             # by level, the walk's order within one
    assert nodes["level"].tolist() == [0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3] and nodes["parent"][0] == abi.CLIP_NO_NODE
    for n in range(1, len(nodes)):
        p = int(nodes["parent"][n])
        assert p < n and nodes["level"][p] + 1 == nodes["level"][n]
    doc_children = {0: [1, 4, 5, 7], 1: [2], 2: [3], 5: [6], 7: [8, 9, 10]}
    for n in range(1, len(nodes)):
        assert int(nodes["gltf_node"][n]) in doc_children[int(nodes["gltf_node"][nodes["parent"][n]])]
    of = {int(gn): n for n, gn in enumerate(nodes["gltf_node"])}
    assert nodes["animated"][[of[k] for k in range(11)]].tolist() == [0, 3, 2, 2, 1, 0, 4, 2, 0, 0, 1]
    assert inst.tolist() == [of[4], of[8], of[9]]
    assert (clip.skin(0), clip.skin(1)) == ((0, 3), (3, 2))
    assert refused(lambda: clip.skin(2))[0] == ERR_INVALID_ARG
    # two channels name node 3's rotation: the later one (turns about z) is kept, the earlier (about x) is gone
    rot3 = [c for c, ch in enumerate(chans) if ch["node"] == of[3] and ch["path"] == 1]
    assert len(rot3) == 1
    times, values = clip.channel_keys(rot3[0])
    assert times.tolist() == [0.25, 1.0, 2.0] and (values[:, 0] == 0).all() and values[1, 2] != 0
    assert sorted(int(ch["n_keys"]) for ch in chans) == [1, 2, 2, 3, 3, 3, 3, 5] and i.n_keys == 22
    assert [int(ch["interpolation"]) for ch in chans if ch["node"] == of[1] and ch["path"] == 0] == [1]      # STEP
    static = g.bake_clip(-1)
    assert (static.info.animation, static.info.n_channels, static.info.n_nodes, static.info.duration_seconds) == (-1, 0, 11, 0.0)
    assert not static.layout()[0]["animated"].any()
    assert np.array_equal(bits(static.pose_host(float("nan"))[1]), bits(g.pose(-1, 0.0)[0]))       # the static pose ignores the time


def test_bake_refusals(tmp_path):
    g = rt.Gltf(CLIP_RIG)
    assert refused(lambda: g.bake_clip(-2)) == (ERR_INVALID_ARG, "sr_gltf_bake_clip: the animation is an index, or -1 for the file's static pose")
    assert refused(lambda: g.bake_clip(2)) == (ERR_INVALID_ARG, "sr_gltf_bake_clip: gltf: animation index out of range")
    clip = g.bake_clip(0)
    for bad in (float("nan"), float("inf")):
        assert refused(lambda: clip.sample_host(bad)) == (ERR_INVALID_ARG, "sr_clip_sample_host: gltf: the time of a pose must be finite")
        assert refused(lambda: clip.pose_host(bad)) == (ERR_INVALID_ARG, "sr_clip_pose_host: gltf: the time of a pose must be finite")
        assert refused(lambda: g.pose(0, bad))[1] == "sr_gltf_pose: gltf: the time of a pose must be finite"
    want = {"cubic": (0, ERR_UNSUPPORTED, "CUBICSPLINE animation samplers are not supported"),
            "joint_outside_scene": (-1, ERR_INVALID_ARG, "a joint node of the skin is not part of the scene"),
            "times_not_increasing": (0, ERR_INVALID_ARG, "animation key times must be finite, not negative and strictly increasing"),
            "shared_child": (-1, ERR_UNSUPPORTED, "a node the scene's roots reach twice is not supported in a baked clip")}
    assert sorted(want) == sorted(make_clip_gltf.VARIANTS)
    for variant, (anim, code, text) in want.items():
        path = str(tmp_path / (variant + ".glb"))
        make_clip_gltf.build(variant).write_glb(path)
        v = rt.Gltf(path)
        assert refused(lambda: v.bake_clip(anim)) == (code, "sr_gltf_bake_clip: gltf: " + text), variant
        if variant in ("cubic", "times_not_increasing"):                   # sr_gltf_pose's own status and words
            assert refused(lambda: v.pose(anim, 0.5)) == (code, "sr_gltf_pose: gltf: " + text)
        if variant == "joint_outside_scene":
            assert refused(lambda: v.pose(-1, 0.0, 1)) == (code, "sr_gltf_pose: gltf: " + text)
        if variant == "cubic":
            assert v.bake_clip(1).info.n_channels == 2                      # the other animation bakes


def test_the_node_cap(tmp_path):
    """The cap is the kernel's static LDS budget: a clip of exactly that many nodes bakes and evaluates, one more is refused with
    both counts. (A hierarchy deeper than 256 levels cannot be opened at all: sr_gltf_open walks it first.)"""
    assert abi.CLIP_MAX_NODES >= 256
    at_cap, over = str(tmp_path / "cap.glb"), str(tmp_path / "over.glb")
    assert shape_rig(at_cap, chain=30, fan=abi.CLIP_MAX_NODES - 32, joints=5, channels=40, keys=3) == abi.CLIP_MAX_NODES
    assert shape_rig(over, chain=30, fan=abi.CLIP_MAX_NODES - 31, joints=5, channels=40, keys=3) == abi.CLIP_MAX_NODES + 1
    g = rt.Gltf(at_cap)
    clip = g.bake_clip(0)
    assert clip.info.n_nodes == abi.CLIP_MAX_NODES and clip.info.n_levels == 31
    for t in (0.0, 0.19):
        jm, xf = clip.pose_host(t)
        assert np.array_equal(bits(xf), bits(g.pose(0, t)[0])) and np.array_equal(bits(jm), bits(g.pose(0, t, 0)[1]))
    assert refused(lambda: rt.Gltf(over).bake_clip(0)) == (
        ERR_UNSUPPORTED, "sr_gltf_bake_clip: gltf: a clip of %d nodes is not supported: the device kernel holds %d nodes" % (abi.CLIP_MAX_NODES + 1, abi.CLIP_MAX_NODES))
