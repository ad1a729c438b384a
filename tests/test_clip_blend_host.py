"""Cross-fades between two baked clips on the host (sr_clip_blend_compatible, sr_clip_blend_host, sr_clip_compose_records_host,
sr_clip_pose_blend_host, sr_clip_blend_weights_host). The record rule and the weight rule are held bit for bit to a numpy
restatement (clip_blend_reference.py: plain IEEE float64 / float32, the same operand order); the end weights and a clip blended
with itself are held to the unblended host rule byte for byte. No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, runtime as rt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_util import CLIP_RIG, SKINNED_BAR, bits, clip_times  # noqa: E402
from clip_morph_util import MORPH_BAR, set_times  # noqa: E402
from clip_blend_reference import blend_record, blend_records, blend_weights  # noqa: E402

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
F32 = np.float32
WEIGHTS = [0.0, 1.0, float(np.nextafter(F32(0), F32(1))), float(np.nextafter(F32(1), F32(0))), 0.5, float(F32(1.0) / F32(3.0))]
TABLES = ("the number of nodes", "the level table", "the instance table", "the node table", "the skin table", "the joint nodes", "the joint skins",
          "the inverse bind matrices")
PLACEMENT = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def record(t, q, s, animated):
    r = np.zeros(1, abi.NODE_TRS)
    r["translation"], r["rotation"], r["scale"], r["animated"] = np.array(t, F32), np.array(q, F32), np.array(s, F32), animated
    return r


@pytest.fixture(scope="module")
def rig():
    g = rt.Gltf(CLIP_RIG)
    return g, {a: g.bake_clip(a) for a in (-1, 0, 1)}


def pose_or_refusal(call):
    """-> (joint matrices, instance transforms) or the refusal's (code, words behind the entry point's name)."""
    try:
        return call()
    except rt.SunrayError as e:
        return e.code, e.description.split(": ", 1)[1]


def assert_same_pose(got, want, what):
    if isinstance(want[0], int):
        assert got == want, what
    else:
        assert same(got[0], want[0]) and same(got[1], want[1]), what


# ---- 1. the record rule against the reference --------------------------------------------------------------------------------------
def hand_made_records():
    q = [0.1, -0.7, 0.2, 0.68]
    unit = (np.array(q, np.float64) / np.linalg.norm(q)).astype(F32)
    tiny, huge = float(np.float32(1e-42)), 3.0e38
    pairs = [
        # equal parts: everything equal; then only the rotation differs; then only the scale
        (record([1, 2, 3], unit, [1, 1, 1], 7), record([1, 2, 3], unit, [1, 1, 1], 7)),
        (record([1, 2, 3], unit, [1, 1, 1], 2), record([1, 2, 3], [0, 0, 0, 1], [1, 1, 1], 2)),
        (record([1, 2, 3], unit, [1, 1, 1], 4), record([1, 2, 3], unit, [1, 0.5, 2], 4)),
        # negative dot, and a pair whose dot is exactly 0
        (record([0, 1, 0], unit, [1, 1, 1], 2), record([0.5, 1, 0], [-0.2, 0.6, -0.1, -0.75], [1, 1, 1], 3)),
        (record([0, 0, 0], [1, 0, 0, 0], [1, 1, 1], 2), record([0, 0, 0], [0, 1, 0, 0], [1, 1, 1], 2)),
        # opposite quaternions, a zero quaternion on either side and on both sides with unequal signs of zero
        (record([0, 0, 0], unit, [1, 1, 1], 2), record([0, 0, 0], -unit, [1, 1, 1], 2)),
        (record([0, 0, 0], [0, 0, 0, 0], [1, 1, 1], 2), record([0, 0, 0], unit, [1, 1, 1], 2)),
        (record([0, 0, 0], unit, [1, 1, 1], 2), record([0, 0, 0], [0, 0, 0, 0], [1, 1, 1], 2)),
        (record([0, 0, 0], [0, 0, 0, 0], [1, 1, 1], 2), record([0, 0, 0], [-0.0, 0, 0, 0], [1, 1, 1], 2)),
        # denormal and huge translations, -0 against +0
        (record([tiny, -tiny, 0.0], unit, [1, 1, 1], 1), record([3 * tiny, tiny, -0.0], unit, [1, 1, 1], 1)),
        (record([huge, -huge, 1.0], unit, [huge, 1, 1], 5), record([-huge, huge, 1.0], unit, [1, huge, 1], 5)),
        (record([huge, 1e-30, 1.0], unit, [1, 1, 1], 1), record([1e-30, huge, 3.0], unit, [1, 1, 1], 1)),
    ]
    out = []
    for a, b in pairs:
        for ma, mb in ((0, 0), (1, 0), (0, 7), (5, 2), (int(a["animated"][0]), int(b["animated"][0]))):
            x, y = a.copy(), b.copy()
            x["animated"], y["animated"] = ma, mb
            out.append((x, y))
    return out


def test_blend_host_equals_the_reference_bit_for_bit():
    cases = hand_made_records()
    trs_a, trs_b = np.concatenate([a for a, _ in cases]), np.concatenate([b for _, b in cases])
    interpolated = 0
    for w in WEIGHTS:
        got, want = rt.clip_blend_host(trs_a, trs_b, w), blend_records(trs_a, trs_b, w)
        for n in range(len(cases)):
            assert same(got[n:n + 1], want[n:n + 1]), (w, n, got[n], want[n])
        interpolated += int((bits(got["rotation"]) != bits(trs_a["rotation"])).any(axis=1).sum())
        if w == 0.0:
            assert same(got, trs_a)
        if w == 1.0:
            assert same(got, trs_b)
    assert interpolated > 20
    # what the rule states, on the reference's side too: the mask, the untouched record where nothing is animated
    got = rt.clip_blend_host(trs_a, trs_b, 0.5)
    masks = trs_a["animated"] | trs_b["animated"]
    assert np.array_equal(got["animated"][masks != 0], masks[masks != 0]) and same(got[masks == 0], trs_a[masks == 0])
    for w in (-0.1, 1.5, float("nan"), float("inf")):
        assert refused(lambda: rt.clip_blend_host(trs_a, trs_b, w)) == (ERR_INVALID_ARG, "sr_clip_blend_host: the weight is not in [0, 1]")


def test_opposite_quaternions_at_one_half_give_the_first():
    unit = np.array([0.6, 0.0, 0.0, 0.8], F32)
    a, b = record([0, 0, 0], unit, [1, 1, 1], 2), record([0, 0, 0], -unit, [1, 1, 1], 2)
    got = rt.clip_blend_host(a, b, 0.5)
    assert same(got, blend_records(a, b, 0.5))
    assert np.allclose(got["rotation"][0], unit, atol=1e-7)


# ---- 2, 3. end weights; the same clip at the same time -------------------------------------------------------------------------------
def test_end_weights_equal_the_unblended_pose(rig):
    g, clips = rig
    n = 0
    for a, b in itertools.product((-1, 0, 1), repeat=2):
        ta, tb = clip_times(clips[a]), clip_times(clips[b])
        for k in range(max(len(ta), len(tb))):
            t_a, t_b = ta[k % len(ta)], tb[(k * 7 + 3) % len(tb)]
            for placement in (None, PLACEMENT):
                want_a = pose_or_refusal(lambda: clips[a].pose_host(t_a, placement))
                want_b = pose_or_refusal(lambda: clips[b].pose_host(t_b, placement))
                assert_same_pose(pose_or_refusal(lambda: clips[a].pose_blend_host(t_a, clips[b], t_b, 0.0, placement)), want_a, (a, t_a, b, t_b, 0))
                assert_same_pose(pose_or_refusal(lambda: clips[a].pose_blend_host(t_a, clips[b], t_b, 1.0, placement)), want_b, (a, t_a, b, t_b, 1))
            assert same(clips[a].pose_blend_host(t_a, clips[b], t_b, 1.0, joints=False)[1], clips[b].pose_host(t_b, joints=False)[1])
            n += 1
    assert n > 300                                                            # the grids are not empty


def test_a_clip_blended_with_itself_is_the_identity(rig):
    g, clips = rig
    for a, clip in clips.items():
        for t in clip_times(clip):
            want = pose_or_refusal(lambda: clip.pose_host(t, PLACEMENT))
            trs = clip.sample_host(t)
            for w in WEIGHTS:
                assert_same_pose(pose_or_refusal(lambda: clip.pose_blend_host(t, clip, t, w, PLACEMENT)), want, (a, t, w))
                assert same(rt.clip_blend_host(trs, trs, w), trs)


# ---- 4. compose_records_host ---------------------------------------------------------------------------------------------------------
def test_compose_records_on_sampled_records_equals_compose_host(rig):
    g, clips = rig
    for a, clip in clips.items():
        for t in clip_times(clip):
            trs = clip.sample_host(t)
            for placement in (None, PLACEMENT):
                want, got = clip.compose_host(trs, placement), clip.compose_records_host(trs, placement)
                assert same(got[0], want[0]) and same(got[1], want[1]) and got[2] == want[2], (a, t)
    # the decision is the record's: with every mask cleared, the static pose's composition from the file's matrices
    clip = clips[0]
    trs = clip.sample_host(0.7)
    trs["animated"] = 0
    static = clips[-1]
    zero = static.sample_host(0.0)
    zero["animated"] = 0
    assert same(clip.compose_records_host(trs)[1], static.compose_records_host(zero)[1])


# ---- 5. the shorter arc ----------------------------------------------------------------------------------------------------------------
def test_the_blend_takes_the_shorter_arc(rig):
    g, clips = rig
    play, collapse = clips[0], clips[1]
    node = int(np.flatnonzero(play.layout()[0]["gltf_node"] == 2)[0])         # ja1
    a, b = play.sample_host(0.9), collapse.sample_host(1.0)
    qa, qb = a["rotation"][node].astype(np.float64), b["rotation"][node].astype(np.float64)
    assert qa @ qb < 0.0
    got = rt.clip_blend_host(a, b, 0.5)
    assert same(got, blend_records(a, b, 0.5))
    r = got["rotation"][node].astype(np.float64)
    assert abs(np.linalg.norm(r) - 1.0) < 1e-6
    assert (r @ qa) * (r @ -qb) > 0.0 and abs(r @ qa) > 0.9 and abs(r @ qb) > 0.9      # between the two, up to sign: not the long way round
    assert r @ qa > 0.0 and r @ -qb > 0.0


# ---- 6. compatibility ------------------------------------------------------------------------------------------------------------------
def test_compatibility(rig):
    g, clips = rig
    for a, b in itertools.product(clips, repeat=2):
        assert clips[a].blend_compatible(clips[b])
    bar = rt.Gltf(SKINNED_BAR)
    for other in (bar.bake_clip(-1), bar.bake_clip(0)):
        for first, second in ((clips[0], other), (other, clips[1])):
            code, text = refused(lambda: first.blend_compatible(second))
            assert code == ERR_INVALID_ARG and text in ["sr_clip_blend_compatible: the clips differ in " + t for t in TABLES], text
            assert refused(lambda: first.pose_blend_host(0.0, second, 0.0, 0.5)) == (code, text)
    assert bar.bake_clip(0).blend_compatible(bar.bake_clip(-1))


def test_refusals_of_the_blended_pose(rig):
    g, clips = rig
    for w in (-0.1, 1.5, float("nan")):
        assert refused(lambda: clips[0].pose_blend_host(0.5, clips[1], 0.5, w)) == (ERR_INVALID_ARG, "sr_clip_pose_blend_host: the weight is not in [0, 1]")
    for ta, tb in ((float("nan"), 0.5), (0.5, float("inf"))):
        assert refused(lambda: clips[0].pose_blend_host(ta, clips[1], tb, 0.5)) == (ERR_INVALID_ARG, "sr_clip_pose_blend_host: gltf: the time of a pose must be finite")
    clips[-1].pose_blend_host(float("nan"), clips[-1], float("inf"), 0.5)      # the static pose ignores the time
    # collapse at t = 1 scales a mesh node to 0: at w = 1 the blend is that pose
    assert refused(lambda: clips[0].pose_blend_host(0.5, clips[1], 1.0, 1.0)) == (ERR_UNSUPPORTED, "sr_clip_pose_blend_host: gltf: the transform of the skinned mesh's node is singular")
    clips[0].pose_blend_host(0.5, clips[1], 1.0, 0.5)


# ---- 7. weights ------------------------------------------------------------------------------------------------------------------------
def test_blended_weights_equal_the_reference():
    g = rt.Gltf(MORPH_BAR)
    talk, static, spline = g.bake_clip(0), g.bake_clip(-1), g.bake_clip(1)
    n = changed = 0
    for blas in (0, 1):
        times = set_times(talk, blas)
        for k, t in enumerate(times):
            t_other = times[(5 * k + 2) % len(times)]
            for a, b in ((talk, static), (static, talk), (talk, talk)):
                wa, wb = a.weights_host(t, blas), b.weights_host(t_other, blas)
                for w in WEIGHTS:
                    got = a.blend_weights_host(t, b, t_other, w, blas)
                    assert same(got, blend_weights(wa, wb, w)), (blas, t, t_other, w)
                    assert w != 0.0 or same(got, wa)
                    assert w != 1.0 or same(got, wb)
                    changed += int(not same(got, wa) and not same(got, wb))
                    n += 1
    assert n > 500 and changed > 50
    for a, b in ((spline, talk), (talk, spline)):
        assert refused(lambda: a.blend_weights_host(0.5, b, 0.5, 0.5, 0)) == (ERR_UNSUPPORTED, "sr_clip_blend_weights_host: " + CUBIC)
    assert same(spline.blend_weights_host(0.5, talk, 0.5, 0.0, 1), spline.weights_host(0.5, 1))
    assert refused(lambda: talk.blend_weights_host(0.5, static, 0.5, 2.0, 0)) == (ERR_INVALID_ARG, "sr_clip_blend_weights_host: the weight is not in [0, 1]")
    assert refused(lambda: talk.blend_weights_host(0.5, static, 0.5, 0.5, 0, n_targets=1))[0] == ERR_INVALID_ARG
