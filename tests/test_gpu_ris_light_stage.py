"""The RIS pass keeps the light table in its waves' idle LDS while it draws candidates (kernels.hip, stage_lights). That may not
change a bit: every output of both passes against the oracle over frames 0-2 (frame 0 has no history), on scenes whose light
count sits at and around the capacity of their own launch, at an extent that leaves edge tiles with fewer than 64 lanes, tiles
that are part sky and one that is all sky, with candidate counts that are no power of two or zero (no copy is made then, with
history present), a camera that moves between frames 1 and 2, and in the two-level and textured variants of the kernel.
Run on an MI355X with:  python -m pytest tests/test_gpu_ris_light_stage.py -m gpu -q
"""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from test_gpu_parity import assert_bits_equal, rt  # noqa: E402,F401  (rt: the module's GPU fixture)

W, H = 27, 21                    # 4 x 3 tiles of 8 x 8: the right column is 3 pixels wide, the bottom row 5 high
SKY_DEPTH = 0x7C00               # store_gbuffer's 100000.0 as binary16
MOVE = (0.15, 0.05, -0.1)        # per frame, the translation of test_gpu_parity's moving-camera case


def light_scene(n, textured=False):
    """A floor quad (two triangles, roughness 0.7) under `n` small emissive triangles that face it. The camera looks along the
    floor at the horizon, which crosses the middle tile row; the lights hang left of the view axis, so the top right tiles see
    nothing but sky."""
    s = scenes.SceneDesc("floor_and_%d_lights" % n, camera_pos=(0.0, 1.0, 3.0), camera_target=(0.0, 0.8, -10.0), fov_y=45.0)
    floor = abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.7)
    if textured:
        rng = np.random.default_rng(5)
        s.images.append(rng.integers(0, 256, size=(8, 8, 4), dtype=np.uint8))
        s.samplers.append((1, 1, 0, 0))
        floor = abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.7, textures={"base_color": (0, 0)})
    v, i = scenes.quad((-20, 0, 20), (20, 0, 20), (20, 0, -20), (-20, 0, -20), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(1, v, i, floor))
    s.instances.append((1, [abi.IDENTITY_TRANSFORM.copy()]))
    if n:
        pos = []
        for k in range(n):
            x, z = -3.0 + 0.3 * (k % 10), -1.0 - 0.45 * (k // 10)
            y = 1.8 + 0.01 * (k % 7)
            pos += [(x, y, z), (x, y, z - 0.2), (x + 0.2, y, z)]            # cross(e1, e2) points down, at the floor
        lamp = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5, emissive_factor=(1.0, 0.9, 0.7), emissive_strength=20.0)
        lv = scenes.make_vertices(np.array(pos, dtype=np.float32), np.tile(np.array([[0, -1, 0]], dtype=np.float32), (3 * n, 1)))
        s.meshes.append(scenes.MeshDesc(2, lv, np.arange(3 * n, dtype=np.uint32), lamp))
        s.instances.append((2, [abi.IDENTITY_TRANSFORM.copy()]))
    return s


def camera_pos(desc, f, moving):
    k = f if (moving and f >= 2) else 0          # frames 0 and 1 from one place, frame 2 from another
    return tuple(c + m * k for c, m in zip(desc.camera_pos, MOVE))


_oracle_frames = {}


def oracle_frames(oracle, blue_noise, key, desc, cfg, frames, moving):
    """The oracle's outputs of every frame of a case, computed once per case and left unchanged."""
    if key not in _oracle_frames:
        osc = oracle.OracleScene().load(desc)
        of = oracle.HostFrame(W, H, blue_noise)
        prev, out = None, []
        for f in range(frames):
            om = oracle.camera_matrices(camera_pos(desc, f, moving), desc.camera_target, desc.fov_y, W, H, prev)
            prev = list(om.view_proj)
            osc.trace_ris(of, om, f, cfg); osc.trace_final(of, om, f, cfg)
            out.append({"depth": of.depth.copy(), "normal": of.normal.copy(), "diffuse": of.diffuse.copy(), "motion": of.motion.copy(),
                        "reservoirs": of.reservoirs[f & 1].copy(), "reservoirs_gi": of.reservoirs_gi[f & 1].copy(),
                        "raw_color": of.raw_color.copy()})
        _oracle_frames[key] = out
    return _oracle_frames[key]


def run_case(rt, oracle, blue_noise, key, desc, gsc, cfg=None, frames=3, moving=False):
    cfg = cfg or abi.SrTraceConfig.reference()
    want = oracle_frames(oracle, blue_noise, key, desc, cfg, frames, moving)
    gf = rt.DeviceFrame(W, H, blue_noise)
    prev = None
    for f in range(frames):
        gm = rt.camera_matrices(camera_pos(desc, f, moving), desc.camera_target, desc.fov_y, W, H, prev)
        prev = list(gm.view_proj)
        gsc.trace_ris(gf, gm, f, cfg); gsc.trace_final(gf, gm, f, cfg)
        h = gf.host()
        for name in ("depth", "normal", "diffuse", "motion"):
            assert_bits_equal(want[f][name], h[name], "%s_img f%d" % (name, f))
        assert_bits_equal(want[f]["reservoirs"], h["reservoirs"][f & 1], "reservoirs f%d" % f)
        assert_bits_equal(want[f]["reservoirs_gi"], h["reservoirs_gi"][f & 1], "reservoirs_gi f%d" % f)
        assert_bits_equal(want[f]["raw_color"], h["raw_color"], "raw_color f%d" % f)
    return want


def tiles_of(depth):
    d = np.asarray(depth).reshape(H, W)
    return [d[y:y + 8, x:x + 8] for y in range(0, H, 8) for x in range(0, W, 8)]


def scene_at_capacity(rt, delta):
    """A scene whose light count is the capacity of ITS OWN launch plus delta (the capacity follows the tree's stack need, which
    may grow with the lights): fixed point of n = capacity(scene(n)) + delta."""
    n = 44 + delta
    for _ in range(8):
        desc = light_scene(n)
        gsc = rt.Scene(0).load(desc)
        cap = gsc.light_stage_capacity()
        if n == cap + delta:
            return desc, gsc, cap
        n = cap + delta
    pytest.fail("no scene with capacity %+d lights found" % delta)


@pytest.mark.parametrize("which", ["none", "1", "2", "cap-1", "cap", "cap+1"])
def test_light_counts_around_the_capacity_equal_oracle(rt, oracle, blue_noise, which):
    if which.startswith("cap"):
        delta = {"cap-1": -1, "cap": 0, "cap+1": 1}[which]
        desc, gsc, cap = scene_at_capacity(rt, delta)
        n = cap + delta
    else:
        n = 0 if which == "none" else int(which)
        desc = light_scene(n)
        gsc = rt.Scene(0).load(desc)
        cap = gsc.light_stage_capacity()
        assert n < cap
    assert cap > 0 and cap % 4 == 0                      # whole LDS rows of 256 bytes, 64-byte records
    # an empty light list still has the reference's dummy entry (lib.rs:1075-1081), which is a table of one
    assert gsc.tables()["num_lights"] == max(n, 1)
    want = run_case(rt, oracle, blue_noise, "n=%s" % which, desc, gsc)
    # the launch has what the copy must cope with: an all-sky tile, part-sky tiles, and edge tiles with fewer than 64 lanes
    sky = [(t == SKY_DEPTH) for t in tiles_of(want[0]["depth"])]
    assert any(s.all() for s in sky) and any(s.any() and not s.all() for s in sky)
    assert any(s.size < 64 and not s.all() for s in sky)
    if n:
        assert (want[2]["reservoirs"].view(np.uint32) != 0).any()


@pytest.mark.parametrize("candidates", [0, 1, 5, 16, 17])
def test_candidate_counts_equal_oracle(rt, oracle, blue_noise, candidates):
    desc = light_scene(2)
    cfg = abi.SrTraceConfig.reference()
    cfg.ris_candidates = candidates
    run_case(rt, oracle, blue_noise, "candidates=%d" % candidates, desc, rt.Scene(0).load(desc), cfg=cfg)


def test_moving_camera_between_frames_1_and_2(rt, oracle, blue_noise):
    desc = light_scene(2)
    want = run_case(rt, oracle, blue_noise, "moving", desc, rt.Scene(0).load(desc), moving=True)
    # motion vectors of frame 2: x > 1 marks a pixel without a valid reprojection (inUV + 2); both kinds occur on the floor
    m = np.asarray(want[2]["motion"]).view(np.uint16).reshape(-1, 2)[:, 0].view(np.float16).astype(np.float32)
    floor = np.asarray(want[2]["depth"]).reshape(-1) != SKY_DEPTH
    assert (m[floor] > 1.0).any() and (m[floor] < 1.0).any()


@pytest.mark.parametrize("form", ["two_level", "textured", "two_level_textured"])
def test_two_level_and_textured_variants_equal_oracle(rt, oracle, blue_noise, form):
    desc = light_scene(2, textured="textured" in form)
    gsc = rt.Scene(0, instancing="two_level" if "two_level" in form else None).load(desc)
    assert gsc.two_level() == ("two_level" in form)
    run_case(rt, oracle, blue_noise, form, desc, gsc, frames=2)
