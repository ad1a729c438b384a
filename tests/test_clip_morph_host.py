"""The morph sets of a baked clip on the host (sr_clip_morph_count, sr_clip_morph, sr_clip_morph_keys, sr_clip_weights_host): a set
is what sr_gltf_morph_weights derives from the document, flattened, and the host rule over it is held to that call bit for bit, in
its statuses and words too. A set the loader refuses is kept as unavailable and does not refuse the bake. No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from sunray_amd import abi, runtime as rt

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_morph_util import BIG, BIG_TIMES, MORPH_BAR, ONE, TWO, ZEROS_AT, big_keys, bits, compact, many_targets, set_times  # noqa: E402
from clip_util import CLIP_RIG, SKINNED_BAR  # noqa: E402
import make_morph_gltf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sunray_amd", "csrc")
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
NO_SET = "the clip has no morph set for this blas (it has no morph targets)"


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def words(description):
    """A refusal without the entry point's name in front."""
    return description.split(": ", 1)[1]


def target_count(g, blas):
    """The blas's morph targets; None where its morph parse fails."""
    try:
        d = g.blas_morph(blas)[0]
    except rt.SunrayError:
        return None
    return 0 if d is None else len(d)


def assert_host_rule_is_morph_weights(g, animations, min_times):
    """Every blas of every animation (and the static pose): where sr_gltf_morph_weights answers, the set is available and the
    host rule gives its bits over the whole grid; where it refuses, the set is unavailable with that status and those words, and
    the host rule refuses in them. -> (available sets, unavailable sets)."""
    n_ok = n_bad = n_times = 0
    for a in animations:
        clip = g.bake_clip(a)
        n_sets = 0
        for b in range(g.n_blases):
            if target_count(g, b) == 0:
                assert refused(lambda: clip.morph(b)) == (ERR_INVALID_ARG, "sr_clip_morph: " + NO_SET)
                assert refused(lambda: clip.weights_host(0.0, b, 0)) == (ERR_INVALID_ARG, "sr_clip_weights_host: " + NO_SET)
                continue
            n_sets += 1
            m = clip.morph(b)
            try:
                g.morph_weights(a, 0.0, b)
            except rt.SunrayError as e:
                n_bad += 1
                assert (m["state"], m["status"], m["error"]) == (abi.CLIP_MORPH_UNAVAILABLE, e.code, words(e.description)), (a, b)
                assert refused(lambda: clip.weights_host(0.0, b, m["n_targets"])) == (e.code, "sr_clip_weights_host: " + words(e.description))
                assert refused(lambda: clip.morph_keys(b)) == (e.code, "sr_clip_morph_keys: " + words(e.description))
                continue
            n_ok += 1
            assert m["state"] == (abi.CLIP_MORPH_CHANNEL if m["n_keys"] else abi.CLIP_MORPH_DEFAULTS) and (m["status"], m["error"]) == (0, None)
            assert m["blas"] == b and m["n_targets"] == target_count(g, b)
            assert np.array_equal(bits(clip.morph_keys(b)[2]), bits(g.blas_morph(b)[1]))
            for t in set_times(clip, b):
                n_times += 1
                assert np.array_equal(bits(clip.weights_host(t, b)), bits(g.morph_weights(a, t, b))), (a, b, t)
            # the refusals of an available set, in the host's words
            for bad in (float("nan"), float("inf")):
                if a >= 0:
                    want = refused(lambda: g.morph_weights(a, bad, b))
                    assert want[1] == "sr_gltf_morph_weights: gltf: the time of a pose must be finite"
                    assert refused(lambda: clip.weights_host(bad, b)) == (want[0], "sr_clip_weights_host: " + words(want[1]))
                else:
                    assert np.array_equal(bits(clip.weights_host(bad, b)), bits(g.morph_weights(a, bad, b)))      # the static pose ignores the time
            for nt in (m["n_targets"] + 1, m["n_targets"] - 1):
                w = np.zeros(nt + 1, np.float32)
                rc = rt.lib().sr_gltf_morph_weights(g._h, a, rt.C.c_float(0.0), b, rt._p(w), nt)
                want = (rc, rt.lib().sr_last_error().decode())
                assert want == (ERR_INVALID_ARG, "sr_gltf_morph_weights: gltf: another number of weights asked for than the blas has morph targets")
                assert refused(lambda: clip.weights_host(0.0, b, nt)) == (want[0], "sr_clip_weights_host: " + words(want[1]))
        assert clip.morph_count() == n_sets
    assert n_times >= min_times
    return n_ok, n_bad


def test_sets_of_the_fixture():
    g = rt.Gltf(MORPH_BAR)
    talk, static, spline = g.bake_clip(0), g.bake_clip(-1), g.bake_clip(1)            # the CUBICSPLINE weights channel does not refuse the bake
    assert (talk.morph_count(), static.morph_count(), spline.morph_count()) == (2, 2, 2)
    m0, m1 = talk.morph(0), talk.morph(1)
    assert (m0["blas"], m0["gltf_node"], m0["n_targets"], m0["n_keys"], m0["interpolation"], m0["state"]) == (0, 4, 3, 4, 0, abi.CLIP_MORPH_CHANNEL)
    assert (m1["blas"], m1["gltf_node"], m1["n_targets"], m1["n_keys"], m1["interpolation"], m1["state"]) == (1, 5, 2, 3, 1, abi.CLIP_MORPH_CHANNEL)
    times, values, defaults = talk.morph_keys(0)
    assert times.tolist() == [0.0, np.float32(0.4), np.float32(1.1), 2.0] and values.shape == (4, 3) and values[1].tolist() == [1.0, 0.25, 0.0]
    assert defaults.tolist() == [0.25, 0.0, 0.5]
    times, values, defaults = talk.morph_keys(1)
    assert times.tolist() == [0.25, 1.0, 1.5] and values.tolist() == [[0.0, 1.0], [np.float32(0.7), 0.0], [1.0, np.float32(0.4)]]
    assert defaults.tolist() == [0.5, 0.25]                                            # node 5's own `weights`, not the mesh's
    for b, want in ((0, [0.25, 0.0, 0.5]), (1, [0.5, 0.25])):
        m = static.morph(b)
        assert (m["state"], m["n_keys"]) == (abi.CLIP_MORPH_DEFAULTS, 0)
        assert static.morph_keys(b)[0].size == 0 and static.weights_host(123.0, b).tolist() == want
    m = spline.morph(0)
    assert (m["state"], m["status"], m["error"], m["n_targets"], m["n_keys"]) == (abi.CLIP_MORPH_UNAVAILABLE, ERR_UNSUPPORTED, CUBIC, 3, 0)
    assert refused(lambda: spline.weights_host(0.5, 0)) == (ERR_UNSUPPORTED, "sr_clip_weights_host: " + CUBIC)
    assert refused(lambda: g.morph_weights(1, 0.5, 0)) == (ERR_UNSUPPORTED, "sr_gltf_morph_weights: " + CUBIC)
    assert spline.morph(1)["state"] == abi.CLIP_MORPH_DEFAULTS and spline.weights_host(0.5, 1).tolist() == [0.5, 0.25]
    for b in (2, 3):                                                                   # the floor and the panel have no targets
        assert refused(lambda: talk.morph(b)) == (ERR_INVALID_ARG, "sr_clip_morph: " + NO_SET)
    # the figures of the TRS channels do not count the weights channels
    assert (talk.info.n_channels, talk.info.n_keys, talk.info.duration_seconds) == (1, 4, 2.0) and len(talk.layout()[1]) == 1
    assert (spline.info.n_channels, spline.info.n_keys, spline.info.duration_seconds) == (0, 0, 0.0)


def test_host_rule_equals_morph_weights_on_the_fixture():
    g = rt.Gltf(MORPH_BAR)
    assert assert_host_rule_is_morph_weights(g, (-1, 0, 1), 50) == (5, 1)


def test_files_without_targets_bake_as_before():
    """The figures are the parent commit's: the block of a clip without morph sets has not changed."""
    want = {(CLIP_RIG, -1): (-1, 11, 4, 0, 2, 5, 3, 0, 0.0, 1872), (CLIP_RIG, 0): (0, 11, 4, 8, 2, 5, 3, 22, 2.0, 2544),
            (SKINNED_BAR, -1): (-1, 7, 4, 0, 1, 3, 4, 0, 0.0, 1216), (SKINNED_BAR, 0): (0, 7, 4, 3, 1, 3, 4, 11, 2.0, 1536)}
    for (path, a), figures in want.items():
        clip = rt.Gltf(path).bake_clip(a)
        assert clip.morph_count() == 0
        i = clip.info
        got = tuple(getattr(i, name) for name, _ in abi.SrClipInfo._fields_)
        assert got[:-1] == figures[:-1], (path, a)
        assert got[-1] == figures[-1], (path, a)                                   # device_bytes too: nothing was added
        assert refused(lambda: clip.morph(0))[0] == ERR_INVALID_ARG


def test_a_generated_file_of_130_targets_one_key_and_one_target(tmp_path):
    path = str(tmp_path / "many.glb")
    counts = many_targets(path)
    g = rt.Gltf(path)
    assert assert_host_rule_is_morph_weights(g, (-1, 0, 1), 100) == (9, 0)
    lin, step = g.bake_clip(0), g.bake_clip(1)
    assert [lin.morph(b)["n_targets"] for b in (BIG, ONE, TWO)] == [counts[b] for b in (BIG, ONE, TWO)] == [130, 1, 2]
    assert [(lin.morph(b)["n_keys"], lin.morph(b)["interpolation"]) for b in (BIG, ONE, TWO)] == [(4, 0), (1, 0), (2, 0)]
    assert [(step.morph(b)["n_keys"], step.morph(b)["interpolation"]) for b in (BIG, ONE, TWO)] == [(4, 1), (3, 1), (0, 0)]
    assert np.array_equal(bits(lin.morph_keys(BIG)[1]), bits(big_keys())) and lin.morph_keys(BIG)[0].tolist() == list(BIG_TIMES)
    # the shapes the device tests lean on: nothing active at or before key 0, the zeros of key 1 (and its -0) left out at 0.5 and
    # active just after it, everything active at key 2
    assert len(compact(lin.weights_host(0.0, BIG))[0]) == len(compact(lin.weights_host(-1.0, BIG))[0]) == 0
    at = compact(lin.weights_host(0.5, BIG))[0].tolist()
    assert at == [k for k in range(130) if k not in ZEROS_AT + (5,)]
    assert len(compact(lin.weights_host(0.75, BIG))[0]) == len(compact(lin.weights_host(1.0, BIG))[0]) == 130
    assert len(compact(lin.weights_host(0.25, BIG))[0]) == 130 - len(ZEROS_AT) - 1         # 0 + u * (-0 - 0) is +0
    assert compact(step.weights_host(0.75, BIG))[0].tolist() == at and len(compact(step.weights_host(2.0, BIG))[0]) == 65
    assert lin.weights_host(-3.0, ONE).tolist() == [2.0] and step.weights_host(1.0, ONE).tolist() == [0.0]


@pytest.mark.parametrize("variant", make_morph_gltf.VARIANTS)
def test_a_set_the_loader_refuses_is_unavailable_and_the_bake_succeeds(tmp_path, variant):
    path = str(tmp_path / (variant + ".glb"))
    make_morph_gltf.build(variant).write_glb(path)
    g = rt.Gltf(path)
    ok, bad = assert_host_rule_is_morph_weights(g, (-1, 0, 1), 10)
    assert bad >= 1 and ok >= 1, (variant, ok, bad)
    parse = variant in ("short_target", "integer_target", "texcoord_target", "node_weights_differ", "counts_disagree")
    blas = 1 if variant == "node_weights_differ" else 0
    m = g.bake_clip(0).morph(blas)
    assert m["state"] == abi.CLIP_MORPH_UNAVAILABLE and (m["n_targets"] == 0) == parse and (m["gltf_node"] == abi.CLIP_NO_NODE) == parse
    assert m["status"] == (ERR_UNSUPPORTED if variant in ("integer_target", "texcoord_target", "node_weights_differ") else ERR_INVALID_ARG)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bake_and_host_rule_under_sanitizers(tmp_path):
    """tests/native/clip_morph_asan.cpp, a stand-alone program of the loader's host sources and clip_host.cpp, under
    AddressSanitizer + UndefinedBehaviorSanitizer: the fixture, the generated file and the broken variants are baked, every
    read-out is walked, and the host rule runs at the edges against sr_gltf_morph_weights. Nothing is loaded into Python."""
    flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    exe = str(tmp_path / "clip_morph_asan")
    subprocess.check_call(["g++"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "clip_morph_asan.cpp"), os.path.join(CSRC, "gltf_load.cpp"),
                                             os.path.join(CSRC, "clip_host.cpp"), os.path.join(CSRC, "jpeg_decode.cpp"), "-lz", "-o", exe])
    many = str(tmp_path / "many.glb")
    many_targets(many)
    broken = []
    for name in make_morph_gltf.VARIANTS:
        broken.append(str(tmp_path / (name + ".glb")))
        make_morph_gltf.build(name).write_glb(broken[-1])
    out = subprocess.run([exe, MORPH_BAR, many] + broken, capture_output=True, text=True, env=env)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout + out.stderr[-3000:]
    assert "clip morph ok: 2 good files, %d broken variants" % len(make_morph_gltf.VARIANTS) in out.stdout, out.stdout
