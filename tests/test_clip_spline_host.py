"""CUBICSPLINE sampling on the host (sr_gltf_set_cubicspline): the loader and the baked-clip host rule against an exact-arithmetic
reference (clip_spline_reference.py), exactness at the keys and beyond the ends, the bit chain from the loader through the clip's
host rules, the mode leaving every other bake unchanged, and the default refusing as ever. No GPU."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, runtime as rt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import clip_spline_reference as ref  # noqa: E402
import make_clip_gltf  # noqa: E402
import make_spline_gltf  # noqa: E402
from clip_spline_util import MORPH_BAR, SKINNED_BAR, SPLINE_RIG, bits, channel_times, clip_channel_times  # noqa: E402
from clip_util import CLIP_RIG  # noqa: E402

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
FACE_BLAS = 3


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def sampling(path):
    g = rt.Gltf(path)
    g.set_cubicspline(True)
    return g


def cubic_channels(clip):
    """[(channel, gltf node, path, times, rows [3 * n_keys, comps])] of the clip's CUBICSPLINE channels."""
    nodes, chans, _ = clip.layout()
    out = []
    for c, ch in enumerate(chans):
        if ch["interpolation"] == abi.CLIP_CUBICSPLINE:
            times, rows = clip.channel_keys(c)
            out.append((c, int(nodes[ch["node"]]["gltf_node"]), int(ch["path"]), times, rows))
    return out


def compare_file(g, animation, blases=()):
    """Every cubic channel and set of one animation over its time set against the reference -> (correctly rounded, compared)."""
    clip = g.bake_clip(animation)
    right = total = 0
    for _, node, path, times, rows in cubic_channels(clip):
        for t in channel_times(times):
            trs = g.sample_node(animation, t, node)
            r, n = ref.check_sample(trs[path], times, rows, t, rotation=path == 1)
            right, total = right + r, total + n
    for b in blases:
        m = clip.morph(b)
        if m["interpolation"] != abi.CLIP_CUBICSPLINE:
            continue
        times, rows, _ = clip.morph_keys(b)
        for t in channel_times(times):
            r, n = ref.check_sample(g.morph_weights(animation, t, b), times, rows, t)
            right, total = right + r, total + n
    return right, total


def test_samples_equal_the_exact_rule(tmp_path):
    """spline_rig.glb, skinned_bar.glb animation 1, morph_bar.glb animation 1 and the `cubic` variant of make_clip_gltf under
    SAMPLE, every cubic channel and set over its time set. A component is the correctly rounded fp32 of the exact value, or lies
    within half an fp32 ulp plus 2^-48 * S of it (rotations: one more ulp after the normalisation); no more than 1 % of the
    compared components may fail to be the correctly rounded value. First run: 407 of 411 are; the four others are rotation
    components of spline_rig.glb at nextafter below the last key whose exact value is about 1e-14 against S of about 1.1 (the
    next key's component is 0 and h00 = (2u^3 - 3u^2) + 1 cancels at u = 1 - 6e-8), each well inside the bound."""
    cubic = str(tmp_path / "cubic.glb")
    make_clip_gltf.build("cubic").write_glb(cubic)
    right = total = 0
    for path, animation, blases in ((SPLINE_RIG, 0, (FACE_BLAS,)), (SPLINE_RIG, 2, ()), (SKINNED_BAR, 1, ()), (MORPH_BAR, 1, (0,)), (cubic, 0, ())):
        r, n = compare_file(sampling(path), animation, blases)
        assert n >= 24, (path, animation)
        right, total = right + r, total + n
    print("correctly rounded: %d of %d" % (right, total))
    assert total > 400
    assert (total - right) * 100 <= total


def test_keys_and_clamped_times_are_the_keys_value_bytes():
    g = sampling(SPLINE_RIG)
    clip = g.bake_clip(0)
    seen = 0
    for _, node, path, times, rows in cubic_channels(clip):
        values = rows[1::3]
        for k, t in [(0, float(times[0]) - 1.0), (len(times) - 1, float(times[-1]) + 1.5)] + [(k, float(t)) for k, t in enumerate(times)]:
            got = g.sample_node(0, t, node)[path]
            want = values[k]
            if path == 1:                                                  # a rotation: the normalised value, in double, rounded once
                q = want.astype(np.float64)
                want = (q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])).astype(np.float32)
            assert np.array_equal(bits(got), bits(want)), (node, path, t)
            seen += 1
    assert seen >= 6 * 3
    times, rows, _ = clip.morph_keys(FACE_BLAS)
    for k, t in enumerate(times):
        assert np.array_equal(bits(g.morph_weights(0, float(t), FACE_BLAS)), bits(rows[3 * k + 1])), t
    assert np.signbit(g.morph_weights(0, 0.5, FACE_BLAS)[2])              # the -0 of key 1 stays -0


def test_through_zero_is_the_zero_quaternion_and_composes():
    g = sampling(SPLINE_RIG)
    t, q, s, mask = g.sample_node(2, 0.5, 2)
    assert mask == 2 and np.array_equal(bits(q), np.zeros(4, np.uint32))
    xf, joints = g.pose(2, 0.5, 0)
    assert np.isfinite(xf).all() and np.isfinite(joints).all()
    clip = g.bake_clip(2)
    jm, cx = clip.pose_host(0.5)
    assert np.array_equal(bits(cx), bits(xf)) and np.array_equal(bits(jm[:3]), bits(joints))


def chain_file(g, animations, n_skins):
    """The bit chain of one file under SAMPLE: the clip's host rules equal the loader's calls."""
    n = 0
    for a in animations:
        clip = g.bake_clip(a)
        nodes = clip.layout()[0]
        blases = [b for b in range(g.n_blases) if g.blas_morph(b)[0] is not None]
        for t in clip_channel_times(clip, blases) or [0.0]:
            trs = clip.sample_host(t)
            for k, node in enumerate(nodes):
                tt, q, s, mask = g.sample_node(a, t, int(node["gltf_node"]))
                assert np.array_equal(bits(trs[k]["translation"]), bits(tt)) and np.array_equal(bits(trs[k]["rotation"]), bits(q)), (a, t, k)
                assert np.array_equal(bits(trs[k]["scale"]), bits(s)) and trs[k]["animated"] == mask, (a, t, k)
            jm, xf = clip.pose_host(t)
            for skin in range(n_skins):
                gx, gj = g.pose(a, t, skin)
                first, nj = clip.skin(skin)
                assert np.array_equal(bits(xf), bits(gx)) and np.array_equal(bits(jm[first:first + nj]), bits(gj)), (a, t, skin)
            for b in blases:
                assert np.array_equal(bits(clip.weights_host(t, b)), bits(g.morph_weights(a, t, b))), (a, t, b)
            n += 1
    return n


def test_bit_chain_from_the_loader_through_the_clip():
    assert chain_file(sampling(SPLINE_RIG), (0, 1, 2), 2) > 40
    assert chain_file(sampling(SKINNED_BAR), (1,), 1) > 3
    assert chain_file(sampling(MORPH_BAR), (1,), 1) > 3


@pytest.mark.parametrize("variant,code,words", [
    ("short_output", ERR_INVALID_ARG, "gltf: animation sampler output holds fewer values than its input has keys"),
    ("nonfinite_tangent", ERR_INVALID_ARG, "gltf: animation sampler output holds a non-finite value"),
    ("short_weights", ERR_INVALID_ARG, "gltf: CUBICSPLINE animation sampler output holds fewer values than three times its input's keys times the morph targets")])
def test_broken_variants_refuse_in_the_same_words_on_both_sides(tmp_path, variant, code, words):
    path = str(tmp_path / (variant + ".glb"))
    make_spline_gltf.build(variant).write_glb(path)
    g = sampling(path)
    if variant == "short_weights":                                         # the set is kept as unavailable; the bake and the pose go through
        assert refused(lambda: g.morph_weights(0, 0.5, FACE_BLAS)) == (code, "sr_gltf_morph_weights: " + words)
        clip = g.bake_clip(0)
        m = clip.morph(FACE_BLAS)
        assert (m["state"], m["status"], m["error"]) == (abi.CLIP_MORPH_UNAVAILABLE, code, words)
        assert refused(lambda: clip.weights_host(0.5, FACE_BLAS)) == (code, "sr_clip_weights_host: " + words)
        g.pose(0, 0.5, 0)
    else:
        assert refused(lambda: g.pose(0, 0.5, 0)) == (code, "sr_gltf_pose: " + words)
        assert refused(lambda: g.sample_node(0, 0.5, 1)) == (code, "sr_gltf_sample_node: " + words)
        assert refused(lambda: g.bake_clip(0)) == (code, "sr_gltf_bake_clip: " + words)


@pytest.mark.parametrize("pair", ["cubic_linear", "linear_cubic", "cubic_cubic"])
def test_blend_host_rules_at_the_end_weights(pair):
    g = sampling(SPLINE_RIG)
    a, b = g.bake_clip(0 if pair != "linear_cubic" else 1), g.bake_clip(1 if pair == "cubic_linear" else 0)
    assert a.blend_compatible(b)
    for ta, tb in ((0.3, 1.7), (0.625, 0.625), (1.0, 0.25)):
        for w, src, t in ((0.0, a, ta), (1.0, b, tb)):
            jm, xf = a.pose_blend_host(ta, b, tb, w)
            wj, wx = src.pose_host(t)
            assert np.array_equal(bits(jm), bits(wj)) and np.array_equal(bits(xf), bits(wx)), (pair, ta, tb, w)
            assert np.array_equal(bits(a.blend_weights_host(ta, b, tb, w, FACE_BLAS)), bits(src.weights_host(t, FACE_BLAS))), (pair, ta, tb, w)
        mid = a.blend_weights_host(ta, b, tb, 0.5, FACE_BLAS)
        wa, wb = a.weights_host(ta, FACE_BLAS).astype(np.float64), b.weights_host(tb, FACE_BLAS).astype(np.float64)
        assert np.array_equal(bits(mid), bits((wa + 0.5 * (wb - wa)).astype(np.float32)))


def readouts(clip, n_blases):
    nodes, chans, inst = clip.layout()
    out = [tuple(getattr(clip.info, f) for f, _ in abi.SrClipInfo._fields_), nodes.tobytes(), chans.tobytes(), inst.tobytes()]
    for c in range(len(chans)):
        out += [x.tobytes() for x in clip.channel_keys(c)]
    out.append(clip.morph_count())
    for b in range(n_blases):
        try:
            m = clip.morph(b)
        except rt.SunrayError as e:
            out.append((e.code, e.description))
            continue
        out.append(sorted(m.items()))
        if m["state"] != abi.CLIP_MORPH_UNAVAILABLE:
            out += [x.tobytes() for x in clip.morph_keys(b)]
    return out


@pytest.mark.parametrize("path,animation", [(CLIP_RIG, 0), (CLIP_RIG, 1), (CLIP_RIG, -1), (SKINNED_BAR, 0), (MORPH_BAR, 0)])
def test_a_bake_without_cubic_samplers_is_unchanged_by_the_mode(path, animation):
    g = rt.Gltf(path)
    assert g.animation_cubic(max(animation, 0)) == (0, 0) or animation < 0
    before = readouts(g.bake_clip(animation), g.n_blases)
    g.set_cubicspline(True)
    assert readouts(g.bake_clip(animation), g.n_blases) == before
    g.set_cubicspline(False)
    assert readouts(g.bake_clip(animation), g.n_blases) == before


def test_the_default_and_the_mode_set_back_refuse_as_ever():
    g = rt.Gltf(SPLINE_RIG)
    assert g.cubicspline is False
    assert g.animation_cubic(0) == (6, 1) and g.animation_cubic(1) == (0, 0) and g.animation_cubic(2) == (1, 0)

    def all_refuse():
        assert refused(lambda: g.pose(0, 0.5, 0)) == (ERR_UNSUPPORTED, "sr_gltf_pose: " + CUBIC)
        assert refused(lambda: g.sample_node(0, 0.5, 1)) == (ERR_UNSUPPORTED, "sr_gltf_sample_node: " + CUBIC)
        assert refused(lambda: g.morph_weights(0, 0.5, FACE_BLAS)) == (ERR_UNSUPPORTED, "sr_gltf_morph_weights: " + CUBIC)
        assert refused(lambda: g.bake_clip(0)) == (ERR_UNSUPPORTED, "sr_gltf_bake_clip: " + CUBIC)
    all_refuse()
    g.set_cubicspline(True)
    assert g.cubicspline is True
    kept = g.bake_clip(0)
    want = kept.weights_host(0.3, FACE_BLAS).copy()
    g.set_cubicspline(False)
    assert g.cubicspline is False
    all_refuse()
    assert g.animation_cubic(0) == (6, 1)
    assert np.array_equal(bits(kept.weights_host(0.3, FACE_BLAS)), bits(want))          # a clip keeps what it was baked with
    assert kept.morph(FACE_BLAS)["interpolation"] == abi.CLIP_CUBICSPLINE and kept.morph(FACE_BLAS)["state"] == abi.CLIP_MORPH_CHANNEL
    with pytest.raises(rt.SunrayError) as e:
        rt.check(rt.lib().sr_gltf_set_cubicspline(g._h, 2))
    assert e.value.code == ERR_INVALID_ARG
    g.bake_clip(1)                                                                      # the LINEAR animation never needed the mode
