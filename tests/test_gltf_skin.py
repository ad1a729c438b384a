"""The glTF loader's rig and animation read-outs (sr_gltf_rig_counts, sr_gltf_blas_skin, sr_gltf_skin, sr_gltf_animation,
sr_gltf_sample_node, sr_gltf_pose) on tests/golden/skinned_bar.glb, against tests/skin_reference.py: an independent numpy reader
of the same file, a float64 model of the sampling and a float32 restatement of the loader's matrix chain. No GPU."""
import glob
import os
import sys

import numpy as np
import pytest

from sunray_amd import runtime as rt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_skinned_gltf  # noqa: E402
import skin_reference as ref  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "skinned_bar.glb")
ROOMS = sorted(glob.glob(os.path.join(HERE, "golden", "ref_assets", "*.glb")))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
KEY_TIMES = (0.0, 0.25, 0.5, 1.0, 1.25, 1.5, 2.0)
BETWEEN = (0.1, 0.3, 0.49999, 0.7, 0.99, 1.1, 1.3, 1.75, 1.999)
OUTSIDE = (-1.0, -1e-6, 2.000001, 2.5, 100.0)


@pytest.fixture(scope="module")
def files():
    g, G = rt.Gltf(FIXTURE), ref.Glb(FIXTURE)
    yield g, G
    g.close()


def variant(tmp_path, name):
    path = str(tmp_path / (name + ".glb"))
    make_skinned_gltf.build(name).write_glb(path)
    return path


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def test_the_committed_fixture_is_what_the_generator_writes(tmp_path):
    path = str(tmp_path / "again.glb")
    make_skinned_gltf.build().write_glb(path)
    assert open(path, "rb").read() == open(FIXTURE, "rb").read()
    assert os.path.getsize(FIXTURE) < 64 * 1024


def test_rig_read_outs_equal_the_reference_reader(files):
    g, G = files
    assert g.rig_counts() == (len(G.doc["skins"]), len(G.doc["animations"])) == (1, 2)
    inst, first = G.instances()
    assert (g.n_blases, g.n_instances) == (len(first), len(inst)) == (4, 4)
    parsed = rt.gltf_parse(FIXTURE)
    assert [b for b, _ in parsed["instances"]] == [b for b, _ in inst]
    counts = []
    for b in range(g.n_blases):
        want_skin, want = G.blas_skin(b)
        skin, got = g.blas_skin(b)
        assert skin == want_skin
        if want is None:
            assert got is None
            continue
        assert len(got) == len(parsed["blases"][b]["vertices"]) and got.tobytes() == want.tobytes(), b
        counts.append(sorted(set((got["weight"] != 0).sum(axis=1))))
    assert counts == [[1, 2, 3, 4], [1, 2]]                     # the float bar has every count; the u8 bar blends two joints
    u8 = g.blas_skin(1)[1]["weight"]
    assert np.array_equal(u8, np.round(u8 * 255).astype(np.float32) / np.float32(255)) and len(np.unique(u8)) > 10     # k / 255 in fp32
    ibm, joints = g.skin(0)
    want_ibm, want_joints = G.skin(0)
    assert ibm.tobytes() == want_ibm.tobytes() and list(joints) == list(want_joints) == [1, 2, 3]
    for i in range(2):
        assert g.animation(i) == tuple(G.animation(i)), i
    assert g.animation(0) == ("bend", 2.0, 3, 0) and g.animation(1)[0] == "spline"


def test_static_pose_equals_the_load_bit_for_bit(files, tmp_path):
    g, G = files
    for path in [FIXTURE, variant(tmp_path, "matrix_node"), variant(tmp_path, "two_skins")]:
        f = rt.Gltf(path)
        want = np.array([t for _, t in rt.gltf_parse(path)["instances"]], dtype=np.float32)
        got, joints = f.pose(-1, 0.0, 0)
        assert got.tobytes() == want.tobytes(), path
        assert np.abs(joints - np.eye(3, 4, dtype=np.float32).reshape(12)).max() < 1e-6      # the bind pose: identity up to rounding
        again, _ = f.pose(-1, 123.0)                               # the time is not looked at
        assert again.tobytes() == want.tobytes()
        f.close()


@pytest.mark.parametrize("room", ROOMS, ids=[os.path.basename(p) for p in ROOMS])
def test_reference_rooms_have_no_rig_and_pose_as_they_load(room):
    assert len(ROOMS) == 5
    f = rt.Gltf(room)
    assert f.rig_counts() == (0, 0)
    want = np.array([t for _, t in rt.gltf_parse(room)["instances"]], dtype=np.float32)
    assert len(want) == f.n_instances > 0
    assert f.pose(-1, 0.0)[0].tobytes() == want.tobytes()
    for b in range(f.n_blases):
        assert f.blas_skin(b) == (-1, None)
    assert refused(lambda: f.skin(0))[0] == ERR_INVALID_ARG and refused(lambda: f.animation(0))[0] == ERR_INVALID_ARG
    assert refused(lambda: f.pose(0, 0.0))[0] == ERR_INVALID_ARG
    f.close()


def test_sampled_trs_is_within_one_ulp_of_the_float64_model(files):
    """The evaluator works in double from the fp32 keys and rounds once, so against the float64 model only a rounding tie can
    differ: at most 1 fp32 ulp per component. At key times, between keys, before the first key and after the last."""
    g, G = files
    names = {"translation": 0, "rotation": 1, "scale": 2}
    worst, seen = 0.0, set()
    for t in KEY_TIMES + BETWEEN + OUTSIDE:
        model = G.sample64(0, t)
        assert sorted(model) == [1, 2, 3]
        for node, paths in model.items():
            got = g.sample_node(0, t, node)
            assert got[3] == sum(1 << names[p] for p in paths)
            for p, want in paths.items():
                have = got[names[p]].astype(np.float64)
                ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                err = float((np.abs(have - want) / ulp).max())
                worst = max(worst, err)
                assert err <= 1.0, (t, node, p, have, want)
                seen.add((node, p))
            if "rotation" in paths:
                assert abs(float(np.linalg.norm(got[1].astype(np.float64))) - 1.0) < 1e-7
            else:                                                  # what no channel animates is the file's
                assert got[1].tobytes() == G.static_trs(node)[1].tobytes()
    print("worst difference: %.3f ulp" % worst)
    assert seen == {(1, "translation"), (2, "rotation"), (3, "rotation")}
    # STEP holds the earlier key; the clamp holds the first and the last
    assert list(g.sample_node(0, 0.9999, 1)[0]) == [0.0, 0.0, 0.0] and list(g.sample_node(0, 1.0, 1)[0]) == [0.0, 0.25, 0.0]
    assert g.sample_node(0, -5.0, 2)[1].tobytes() == g.sample_node(0, 0.0, 2)[1].tobytes()
    assert g.sample_node(0, 9.0, 3)[1].tobytes() == g.sample_node(0, 2.0, 3)[1].tobytes()
    # the shorter arc: joint 2's third key (a turn of 0.9 about x) is stored negated; half way from the second key (-0.5) the turn
    # is 0.2, not 0.2 + pi
    q = g.sample_node(0, 0.875, 3)[1].astype(np.float64)
    assert abs(q @ np.array(make_skinned_gltf.quat_x(0.2))) > 1.0 - 1e-6
    # an unanimated node reports the file's values and no channel
    t, r, s, mask = g.sample_node(0, 0.7, 0)
    assert mask == 0 and (t.tobytes(), r.tobytes(), s.tobytes()) == tuple(x.tobytes() for x in G.static_trs(0))


def test_matrices_equal_the_float32_chain_bit_for_bit(files, tmp_path):
    """Instance and joint matrices against the same chain restated in numpy float32 in the loader's operation order, fed the
    library's own sampled TRS; the inverse of the mesh node's world transform restated in float64 in the library's order."""
    for path in (FIXTURE, variant(tmp_path, "matrix_node")):
        g, G = rt.Gltf(path), ref.Glb(path)
        moved = 0
        for t in KEY_TIMES + BETWEEN + OUTSIDE:
            trs = {n: g.sample_node(0, t, n)[:3] for n in (1, 2, 3)}
            want_inst, want_joints = G.pose32(trs, 0)
            inst, joints = g.pose(0, t, 0)
            assert inst.tobytes() == want_inst.tobytes(), (path, t)
            assert joints.tobytes() == want_joints.tobytes(), (path, t)
            only_inst, none = g.pose(0, t)
            assert none is None and only_inst.tobytes() == inst.tobytes()
            moved += int(np.abs(joints - np.eye(3, 4, dtype=np.float32).reshape(12)).max() > 0.05)
        assert moved >= 15
        # the skinned mesh's instances keep the transform they have today: no joint moves them
        static = g.pose(-1, 0.0)[0]
        assert g.pose(0, 0.7)[0].tobytes() == static.tobytes()
        g.close()
    # a node the file gives as a matrix composes from TRS (here: the defaults) once a channel animates it
    g = rt.Gltf(variant(tmp_path, "matrix_node"))
    assert list(g.sample_node(0, 0.7, 2)[0]) == [0.0, 0.0, 0.0]
    f = rt.Gltf(FIXTURE)
    assert not np.array_equal(g.pose(0, 0.7, 0)[1][2], f.pose(0, 0.7, 0)[1][2])
    g.close(); f.close()


def test_refusals_come_from_the_new_calls_never_from_open(tmp_path):
    def opened(name):
        path = variant(tmp_path, name)
        parsed = rt.gltf_parse(path)                               # open and every old getter work as for the fixture
        assert len(parsed["blases"]) >= 4
        return rt.Gltf(path)
    g = rt.Gltf(FIXTURE)
    code, text = refused(lambda: g.pose(1, 0.5, 0))
    assert code == ERR_UNSUPPORTED and "CUBICSPLINE" in text
    assert refused(lambda: g.sample_node(1, 0.5, 2))[0] == ERR_UNSUPPORTED
    assert g.animation(1) == ("spline", 1.0, 1, 0)                 # the read-out itself is fine
    for what, call in (("skin index", lambda: g.skin(1)), ("animation index", lambda: g.animation(2)), ("blas index", lambda: g.blas_skin(4)),
                       ("animation index", lambda: g.pose(2, 0.0)), ("node index", lambda: g.sample_node(0, 0.0, 7)),
                       ("finite", lambda: g.pose(0, float("nan"))), ("skin index", lambda: g.pose(0, 0.5, 3))):
        code, text = refused(call)
        assert code == ERR_INVALID_ARG and what in text, (what, text)
    g.close()
    cases = [
        ("short_joints", lambda f: f.blas_skin(0), ERR_INVALID_ARG, "JOINTS_0 shorter"),
        ("short_weights", lambda f: f.blas_skin(1), ERR_INVALID_ARG, "WEIGHTS_0 shorter"),
        ("joints_1", lambda f: f.blas_skin(0), ERR_UNSUPPORTED, "JOINTS_1"),
        ("weights_without_joints", lambda f: f.blas_skin(0), ERR_UNSUPPORTED, "come together"),
        ("two_skins", lambda f: f.blas_skin(0), ERR_UNSUPPORTED, "different skins"),
        ("joint_node_out_of_range", lambda f: f.skin(0), ERR_INVALID_ARG, "joint node"),
        ("joint_node_out_of_range", lambda f: f.blas_skin(0), ERR_INVALID_ARG, "joint node"),
        ("joint_node_out_of_range", lambda f: f.pose(0, 0.5, 0), ERR_INVALID_ARG, "joint node"),
        ("short_inverse_bind", lambda f: f.skin(0), ERR_INVALID_ARG, "fewer matrices"),
        ("times_not_increasing", lambda f: f.animation(0), ERR_INVALID_ARG, "strictly increasing"),
        ("times_not_increasing", lambda f: f.pose(0, 0.5), ERR_INVALID_ARG, "strictly increasing"),
        ("empty_sampler", lambda f: f.animation(0), ERR_INVALID_ARG, "without keys"),
        ("short_output", lambda f: f.pose(0, 0.5), ERR_INVALID_ARG, "fewer values"),
        ("singular_mesh_node", lambda f: f.pose(0, 0.5, 0), ERR_UNSUPPORTED, "singular"),
    ]
    for name, call, status, text in cases:
        f = opened(name)
        code, got = refused(lambda: call(f))
        assert code == status and text in got, (name, code, got)
        f.close()
    # what does not depend on the broken part still works
    f = opened("times_not_increasing")
    assert f.blas_skin(0)[0] == 0 and f.pose(-1, 0.0, 0)[1].shape == (3, 12) and f.animation(1)[0] == "spline"
    f.close()
    f = opened("singular_mesh_node")
    assert f.pose(0, 0.5)[0].shape == (4, 12)                      # instance transforms alone need no inverse
    f.close()
    f = opened("weights_channel")                                  # morph-target channels are counted, not sampled
    assert f.animation(0) == ("bend", 2.0, 4, 1)
    assert f.pose(0, 0.7, 0)[1].tobytes() == rt.Gltf(FIXTURE).pose(0, 0.7, 0)[1].tobytes()
    f.close()
