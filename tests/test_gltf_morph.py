"""The glTF loader's morph-target read-outs (sr_gltf_blas_morph, sr_gltf_morph_weights) on tests/golden/morph_bar.glb, against
tests/morph_reference.py: an independent numpy reader of the same file and a float64 model of the weight sampling. No GPU."""
import glob
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi
from sunray_amd import runtime as rt

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_morph_gltf  # noqa: E402
import morph_reference as ref  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "morph_bar.glb")
SKINNED = os.path.join(HERE, "golden", "skinned_bar.glb")
ROOMS = sorted(glob.glob(os.path.join(HERE, "golden", "ref_assets", "*.glb")))
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
# blas -> (key times of its channel in animation 0, times between keys, times outside)
TIMES = {0: ((0.0, 0.4, 1.1, 2.0), (0.1, 0.39999, 0.7, 1.0, 1.5, 1.999), (-1.0, -1e-6, 2.000001, 50.0)),
         1: ((0.25, 1.0, 1.5), (0.3, 0.99, 1.2, 1.49), (0.0, 0.2, 1.6, 9.0))}


@pytest.fixture(scope="module")
def files():
    g, G = rt.Gltf(FIXTURE), ref.Glb(FIXTURE)
    yield g, G
    g.close()


def variant(tmp_path, name):
    path = str(tmp_path / (name + ".glb"))
    make_morph_gltf.build(name).write_glb(path)
    return path


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def test_the_committed_fixture_is_what_the_generator_writes(tmp_path):
    path = str(tmp_path / "again.glb")
    make_morph_gltf.build().write_glb(path)
    assert open(path, "rb").read() == open(FIXTURE, "rb").read()
    assert os.path.getsize(FIXTURE) < 64 * 1024


def test_deltas_and_default_weights_equal_the_reference_reader(files):
    g, G = files
    inst, first = G.instances()
    assert (g.n_blases, g.n_instances) == (len(first), len(inst)) == (4, 4)
    parsed = rt.gltf_parse(FIXTURE)
    shapes = []
    for b in range(g.n_blases):
        want, want_w = G.blas_morph(b)
        got, got_w = g.blas_morph(b)
        if want is None:
            assert got is None and got_w is None
            assert len(g.morph_weights(-1, 0.0, b)) == 0
            continue
        assert got.dtype == abi.MORPH_DELTA and got.shape == want.shape == (len(want_w), len(parsed["blases"][b]["vertices"]))
        assert got.tobytes() == want.tobytes(), b
        assert got_w.tobytes() == want_w.tobytes(), b
        assert g.morph_weights(-1, 0.0, b).tobytes() == want_w.tobytes()
        shapes.append(got.shape)
    assert shapes == [(3, 200), (2, 48)]
    d, w = g.blas_morph(0)
    assert list(w) == [0.25, 0.0, 0.5]                                    # mesh.weights
    assert list(g.blas_morph(1)[1]) == [0.5, 0.25]                        # node.weights override mesh.weights
    # target 0 has POSITION only, target 1 no TANGENT: absent attributes are zeros; target 2 is sparse: every seventh vertex from 3
    assert d["position"][0].any() and not d["normal"][0].any() and not d["tangent"][0].any()
    assert d["position"][1].any() and d["normal"][1].any() and not d["tangent"][1].any()
    touched = np.flatnonzero(d["tangent"][2].any(axis=1))
    assert list(touched) == list(range(3, 200, 7))
    assert list(np.flatnonzero(d["position"][2].any(axis=1))) == list(touched) == list(np.flatnonzero(d["normal"][2].any(axis=1)))
    # the mesh that is morphed is skinned too, and the skin read-out is untouched by the targets
    assert g.blas_skin(0)[0] == 0 and g.blas_skin(1)[0] == -1


def test_sampled_weights_equal_the_keys_and_the_float64_model(files):
    """At a key time the weights are the key's, bit for bit; outside the keys they are the first / last key's; in between the
    evaluator works in double from the fp32 keys and rounds once, so against the float64 model only a rounding tie can differ: at
    most 1 fp32 ulp."""
    g, G = files
    worst = 0.0
    for blas, (keys, between, outside) in TIMES.items():
        t, v, mode = G.weights_channel(0, blas)
        assert tuple(np.float32(k) for k in keys) == tuple(t) and mode == ("LINEAR" if blas == 0 else "STEP")
        for k, time in enumerate(keys):
            assert g.morph_weights(0, time, blas).tobytes() == v[k].tobytes(), (blas, time)
        for time in outside:
            assert g.morph_weights(0, time, blas).tobytes() == (v[0] if time < keys[0] else v[-1]).tobytes(), (blas, time)
        for time in between:
            got, model = g.morph_weights(0, time, blas), G.weights64(0, time, blas)
            ulp = np.spacing(np.abs(model).astype(np.float32)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - model) / ulp
            worst = max(worst, float(err.max()))
            assert err.max() <= 1.0, (blas, time, got, model)
            if mode == "STEP":
                assert got.tobytes() == v[np.searchsorted(t, np.float32(time), side="right") - 1].tobytes()
            else:
                assert not any(got.tobytes() == row.tobytes() for row in v), (blas, time)      # interpolated, not held
    print("worst error against the float64 model: %.3f ulp" % worst)
    # animation 1 has a channel for node 4 only: blas 1 takes its default weights, blas 0 meets the CUBICSPLINE sampler
    assert g.morph_weights(1, 0.5, 1).tobytes() == g.blas_morph(1)[1].tobytes()
    code, text = refused(lambda: g.morph_weights(1, 0.5, 0))
    assert code == ERR_UNSUPPORTED and "CUBICSPLINE" in text
    assert refused(lambda: g.morph_weights(2, 0.0, 0))[0] == ERR_INVALID_ARG            # no such animation
    assert refused(lambda: g.morph_weights(0, float("nan"), 0))[0] == ERR_INVALID_ARG
    assert refused(lambda: g.blas_morph(4))[0] == ERR_INVALID_ARG
    w = np.zeros(2, np.float32)
    assert rt.lib().sr_gltf_morph_weights(g._h, 0, rt.C.c_float(0.0), 0, w.ctypes.data_as(rt.C.c_void_p), 2) == ERR_INVALID_ARG     # the blas has 3


def test_animation_read_outs_still_count_the_weights_channels_as_ignored(files):
    g, G = files
    assert g.rig_counts() == (1, 2)
    assert g.animation(0) == ("talk", 2.0, 3, 2) and g.animation(1) == ("spline", 0.0, 1, 1)
    for i in range(2):
        assert g.animation(i)[2:] == tuple(G.animation(i))[2:]
    xf, joints = g.pose(1, 0.5, 0)                                        # a CUBICSPLINE weights sampler does not stop sr_gltf_pose
    assert xf.tobytes() == g.pose(-1, 0.0)[0].tobytes() and joints.shape == (3, 12)


BROKEN = {
    # variant -> (blas, call, status, text)
    "short_target": (0, "blas_morph", ERR_INVALID_ARG, "shorter than POSITION"),
    "counts_disagree": (0, "blas_morph", ERR_INVALID_ARG, "disagree"),
    "integer_target": (0, "blas_morph", ERR_UNSUPPORTED, "component type"),
    "texcoord_target": (0, "blas_morph", ERR_UNSUPPORTED, "TEXCOORD_0"),
    "node_weights_differ": (1, "blas_morph", ERR_UNSUPPORTED, "different weights"),
    "short_output": (0, "morph_weights", ERR_INVALID_ARG, "fewer values"),
    "times_not_increasing": (0, "morph_weights", ERR_INVALID_ARG, "strictly increasing"),
}


@pytest.mark.parametrize("name", list(BROKEN))
def test_broken_variants_open_and_are_refused_by_the_new_calls(tmp_path, name):
    assert sorted(BROKEN) == sorted(make_morph_gltf.VARIANTS)
    blas, call, status, text = BROKEN[name]
    f = rt.Gltf(variant(tmp_path, name))                                 # sr_gltf_open reads no morph data
    assert f.n_blases == 4 and len(rt.gltf_parse(variant(tmp_path, name))["blases"][0]["vertices"]) == 200
    assert f.animation(0)[2:] == (3, 2) and f.animation(1)[2:] == (1, 1)  # and the animation read-outs return what they returned
    f.pose(0, 0.5, 0)
    if call == "blas_morph":
        got = refused(lambda: f.blas_morph(blas))
        assert refused(lambda: f.morph_weights(-1, 0.0, blas))[0] == status      # the sampler reads the targets first
    else:
        assert f.blas_morph(blas)[0].shape == (3, 200)
        assert f.morph_weights(-1, 0.0, blas).tobytes() == f.blas_morph(blas)[1].tobytes()
        got = refused(lambda: f.morph_weights(0, 0.5, blas))
    assert got[0] == status and text in got[1], got
    other = 1 - blas                                                      # the other morphed blas of the file is not affected
    assert f.blas_morph(other)[0] is not None and len(f.morph_weights(0, 0.5, other)) == (2 if other else 3)
    f.close()


@pytest.mark.parametrize("path", ROOMS + [SKINNED], ids=[os.path.basename(p) for p in ROOMS + [SKINNED]])
def test_files_without_targets_report_none(path):
    assert len(ROOMS) == 5
    f = rt.Gltf(path)
    assert f.n_blases > 0
    for b in range(f.n_blases):
        assert f.blas_morph(b) == (None, None)
        assert len(f.morph_weights(-1, 0.0, b)) == 0
    f.close()
