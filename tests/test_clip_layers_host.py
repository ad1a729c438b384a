"""The host rule of layer stacks (sr_clip_layers_host, sr_clip_pose_layers_host, sr_clip_subtree_mask) against the numpy float64
restatement of tests/clip_layers_reference.py, bit for bit, and against the rules it extends: one layer is sr_clip_pose_host, two
unmasked override layers are sr_clip_pose_blend_host. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_layers_reference as ref  # noqa: E402
from clip_util import CLIP_RIG, SKINNED_BAR, clip_times  # noqa: E402
from sunray_amd import abi, runtime as rt  # noqa: E402

F32 = np.float32
ERR_INVALID_ARG = -1
TINY, BELOW_ONE = float(np.nextafter(F32(0), F32(1))), float(np.nextafter(F32(1), F32(0)))
INNER = [TINY, float(F32(1.0) / F32(3.0)), 0.5, BELOW_ONE]       # test_gpu_clip_blend.py's INNER


@pytest.fixture(scope="module")
def clips():
    g = rt.Gltf(CLIP_RIG)
    return {a: g.bake_clip(a) for a in (-1, 0, 1)}


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def random_mask(rng, n):
    """Values in [0, 1] with the edge values among them."""
    m = rng.random(n).astype(F32)
    edge = np.array([0.0, 1.0, TINY, BELOW_ONE], F32)
    at = rng.permutation(n)[:min(n, 4)]
    m[at] = edge[:len(at)]
    return m


def test_the_rule_equals_the_numpy_restatement_bit_for_bit(clips):
    rng = np.random.default_rng(7)
    n = clips[0].info.n_nodes
    times = {a: clip_times(c) for a, c in clips.items()}
    checked = additive_changed = 0
    for k in range(max(len(t) for t in times.values())):
        t0, t1, tm = times[0][k % len(times[0])], times[1][(3 * k + 1) % len(times[1])], times[0][(5 * k + 2) % len(times[0])]
        cur = [clips[0].sample_host(t0), clips[1].sample_host(t1), clips[0].sample_host(tm), clips[1].sample_host(t0), clips[-1].sample_host(0.0)]
        refs = [None, None, clips[0].sample_host(t1), clips[1].sample_host(tm), None]
        masks = [None, random_mask(rng, n), random_mask(rng, n), None, random_mask(rng, n)]
        weights = [1.0, INNER[k % 4], INNER[(k + 1) % 4], (0.0, 1.0, 0.5)[k % 3], (1.0, 0.25)[k % 2]]
        rules = [(weights[l], ("override", "override", "additive", "additive", "override")[l], masks[l]) for l in range(5)]
        for n_layers in (1, 2, 3, 4, 5):
            got = rt.clip_layers_host(cur[:n_layers], rules[:n_layers], refs[:n_layers])
            want = ref.layers(cur[:n_layers], [(w, abi.LAYER_ADDITIVE if m == "additive" else abi.LAYER_OVERRIDE, mk) for w, m, mk in rules[:n_layers]], refs[:n_layers])
            assert np.array_equal(ref.words(got), want), (k, n_layers, t0, t1, tm)
            checked += 1
        additive_changed += int(not same(rt.clip_layers_host(cur[:3], rules[:3], refs[:3]), rt.clip_layers_host(cur[:2], rules[:2])))
    assert checked > 100 and additive_changed > 10           # the grid is not empty and the additive layers do something


def test_one_layer_is_pose_host_and_two_override_layers_are_pose_blend_host(clips):
    placement = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], F32)
    for a, t in ((0, 0.3), (1, 0.7), (-1, 0.0), (0, 1.9)):
        for pl in (None, placement):
            got = clips[a].pose_layers_host([(clips[a], t, 1.0, "override", None, 0.0)], pl)
            want = clips[a].pose_host(t, pl)
            assert same(got[0], want[0]) and same(got[1], want[1]), (a, t)
    for (a, ta), (b, tb) in (((0, 0.3), (1, 0.7)), ((1, 0.25), (0, 1.6)), ((0, 0.9), (-1, 0.0)), ((0, 0.4), (0, 1.2))):
        for w in [0.0, 1.0] + INNER:
            got = clips[a].pose_layers_host([(clips[a], ta, 1.0, "override", None, 0.0), (clips[b], tb, w, "override", None, 0.0)], placement)
            want = clips[a].pose_blend_host(ta, clips[b], tb, w, placement)
            assert same(got[0], want[0]) and same(got[1], want[1]), (a, ta, b, tb, w)


def test_identities_of_the_rule(clips):
    n = clips[0].info.n_nodes
    ones, zeros = np.ones(n, F32), np.zeros(n, F32)
    base, over, add, add_ref = clips[0].sample_host(0.3), clips[1].sample_host(0.7), clips[1].sample_host(0.25), clips[1].sample_host(1.6)
    two = rt.clip_layers_host([base, over], [(1.0, "override", None), (0.5, "override", None)])
    assert not same(two, base)
    # a mask of ones equals no mask
    assert same(rt.clip_layers_host([base, over], [(1.0, "override", None), (0.5, "override", ones)]), two)
    three = rt.clip_layers_host([base, over, add], [(1.0, "override", None), (0.5, "override", None), (0.75, "additive", None)], [None, None, add_ref])
    assert not same(three, two)
    assert same(rt.clip_layers_host([base, over, add], [(1.0, "override", None), (0.5, "override", None), (0.75, "additive", ones)], [None, None, add_ref]), three)
    # a mask of zeros or weight 0 gives the layers below, byte for byte
    for mode, r in (("override", None), ("additive", add_ref)):
        for weight, mask in ((0.0, None), (1.0, zeros), (0.5, zeros), (0.0, ones)):
            assert same(rt.clip_layers_host([base, over, add], [(1.0, "override", None), (0.5, "override", None), (weight, mode, mask)], [None, None, r]), two), (mode, weight)
    # an additive layer at its own reference time is the identity at every weight
    for w in [1.0] + INNER:
        assert same(rt.clip_layers_host([base, over, add], [(1.0, "override", None), (0.5, "override", None), (w, "additive", None)], [None, None, add]), two), w


def test_subtree_mask_against_the_layout(clips):
    clip = clips[0]
    nodes = clip.layout()[0]
    for target in range(len(nodes)):
        got = clip.subtree_mask(int(nodes["gltf_node"][target]), 0.75, 0.125)
        inside = np.zeros(len(nodes), bool)
        for n in range(len(nodes)):
            k = n
            while k != abi.CLIP_NO_NODE and k != target:
                k = int(nodes["parent"][k])
            inside[n] = k == target
        assert inside[target] and same(got, np.where(inside, F32(0.75), F32(0.125)).astype(F32)), target
    root = clip.subtree_mask(int(nodes["gltf_node"][0]))
    assert root[0] == 1.0 and set(root.tolist()) <= {0.0, 1.0}
    missing = int(nodes["gltf_node"].max()) + 1000
    assert refused(lambda: clip.subtree_mask(missing)) == (ERR_INVALID_ARG, "sr_clip_subtree_mask: the clip does not hold this glTF node")


def test_every_refusal_of_the_host_functions(clips):
    import ctypes as C
    L = rt.lib()
    n = clips[0].info.n_nodes
    base, over = clips[0].sample_host(0.3), clips[1].sample_host(0.7)
    ok = (1.0, "override", None)
    W = "sr_clip_layers_host: layer 1: "
    for rule, text in (((-0.1, "override", None), W + "the weight is not in [0, 1]"), ((1.5, "additive", None), W + "the weight is not in [0, 1]"),
                       ((float("nan"), "override", None), W + "the weight is not in [0, 1]"),
                       ((0.5, 2, None), W + "unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)"),
                       ((0.5, "additive", None), W + "null argument (the sampled records)"),
                       ((0.5, "override", np.full(n, 1.5, F32)), W + "the mask has a value that is not in [0, 1]"),
                       ((0.5, "override", np.full(n, -0.0, F32) - F32(1e-9)), W + "the mask has a value that is not in [0, 1]"),
                       ((0.5, "override", np.full(n, np.nan, F32)), W + "the mask has a value that is not in [0, 1]")):
        assert refused(lambda: rt.clip_layers_host([base, over], [ok, rule])) == (ERR_INVALID_ARG, text)
    B = "sr_clip_layers_host: layer 0: the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1"
    for rule in ((0.5, "override", None), (1.0, "additive", None), (1.0, "override", np.ones(n, F32))):
        assert refused(lambda: rt.clip_layers_host([base], [rule], [base])) == (ERR_INVALID_ARG, B)
    count = "sr_clip_layers_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"
    assert refused(lambda: rt.clip_layers_host([], [])) == (ERR_INVALID_ARG, count)
    assert refused(lambda: rt.clip_layers_host([base] * 9, [ok] * 9)) == (ERR_INVALID_ARG, count)
    assert len(rt.clip_layers_host([base] * 8, [ok] * 8)) == n
    out = np.zeros(n, abi.NODE_TRS)
    assert L.sr_clip_layers_host(None, None, None, C.c_uint32(1), C.c_uint32(n), out.ctypes.data_as(C.c_void_p)) == ERR_INVALID_ARG
    # sample, stack, compose
    P = "sr_clip_pose_layers_host: layer 1: "
    first = (clips[0], 0.3, 1.0, "override", None, 0.0)
    for layer, text in (((clips[1], float("inf"), 0.5, "override", None, 0.0), P + "gltf: the time of a pose must be finite"),
                        ((clips[1], 0.5, 0.5, "additive", None, float("nan")), P + "gltf: the time of a pose must be finite"),
                        ((clips[1], 0.5, 1.5, "override", None, 0.0), P + "the weight is not in [0, 1]"),
                        ((clips[1], 0.5, 0.5, 7, None, 0.0), P + "unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)"),
                        ((clips[1], 0.5, 0.5, "override", np.full(n, 2.0, F32), 0.0), P + "the mask has a value that is not in [0, 1]")):
        assert refused(lambda: clips[0].pose_layers_host([first, layer])) == (ERR_INVALID_ARG, text)
    clips[0].pose_layers_host([first, (clips[1], 0.5, 0.5, "override", None, float("nan"))])        # an override layer's reference time is not read
    clips[0].pose_layers_host([first, (clips[-1], float("nan"), 0.5, "override", None, 0.0)])       # the static pose has no time
    assert refused(lambda: clips[0].pose_layers_host([(clips[0], 0.3, 0.5, "override", None, 0.0)])) == \
        (ERR_INVALID_ARG, "sr_clip_pose_layers_host: layer 0: the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1")
    assert refused(lambda: clips[0].pose_layers_host([])) == (ERR_INVALID_ARG, "sr_clip_pose_layers_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]")
    assert refused(lambda: clips[0].pose_layers_host([first] * 9))[0] == ERR_INVALID_ARG
    other = rt.Gltf(SKINNED_BAR).bake_clip(0)
    code, text = refused(lambda: clips[0].pose_layers_host([first, (other, 0.5, 0.5, "override", None, 0.0)]))
    assert code == ERR_INVALID_ARG and text.startswith("sr_clip_blend_compatible: the clips differ in the "), text
    assert L.sr_clip_subtree_mask(None, C.c_uint32(0), C.c_float(1), C.c_float(0), None, C.c_uint32(0)) == ERR_INVALID_ARG
    room = np.zeros(n + 1, F32)
    assert L.sr_clip_subtree_mask(clips[0]._h, C.c_uint32(0), C.c_float(1), C.c_float(0), room.ctypes.data_as(C.c_void_p), C.c_uint32(n + 1)) == ERR_INVALID_ARG
    assert L.sr_clip_pose_layers_host(None, None, None, C.c_uint32(1), None, None, None) == ERR_INVALID_ARG
