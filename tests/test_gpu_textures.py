"""GPU parity of the textured half of closest-hit shading (sample_texture, wrap_coord, wrap_index, shade_textured and
any_hit_ignores in sunray_amd/csrc/traverse.h) over its whole input space, bit for bit against the oracle, which
tests/test_oracle_texture.py ties to an exact rational model of the filtering equations and a float64 model of the shader.

  * Sampler probe: fabricated hit records with barycentrics (1, 0, 0) on a mesh of loose triangles sample an image at exact
    coordinates chosen by the test (texture_util.probe_mesh), with no tracing: all 18 filter x address-u x address-v samplers
    and two with min_filter != mag_filter, images from 1x1 to 3x4096 and 2048x2 with 1, 3 and 4 channels, the full
    edge x edge product of texture_util.EDGES (zeros of both signs, texel boundaries, image edges, 2^23, 1e30, denormals,
    either side of the 3e38 guard, infinities, NaN) and random coordinates; through shade_closest_hit and any_hit_ignores.
  * UV-set / tangent zoo: five different uv sets, normals and tangents per vertex, tangent w in {1, 0.5, 0, -0.0, -1, -3,
    NaN} disagreeing inside a triangle, zero / cancelling / parallel tangents, a zero normal, rotated, scaled and mirrored
    instances -- in every form of the scene, so that all three producers of the per-slot uv / tangent record are covered:
    host build, device fast build (PLOC and radix tree), in-place update, two-level, two-level after a top-level rebuild.
  * The pass kernels' own instantiation of the textured shading, on a small closed room with the samplers, extents and uv
    ranges the atrium lacks.
Run on an MI355X with:  python -m pytest tests/test_gpu_textures.py -m gpu -q
"""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_util as tu  # noqa: E402
from test_gpu_parity import assert_bits_equal, run_both  # noqa: E402
from test_gpu_two_level import frames_equal_oracle  # noqa: E402

ALPHA_CUTOFFS = [0.5, 0.25, 0.9, 0.0, 1.5]


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: run them with -m gpu on an MI355X")
    from sunray_amd import runtime
    return runtime


def hits_to_device(hits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.float32).reshape(-1, 4).copy()).cuda()


def device_payloads(gsc, hits):
    return gsc.shade_closest_hit(hits_to_device(hits), len(hits)).cpu().numpy().view(np.uint32).reshape(-1).view(abi.RAY_PAYLOAD)


def probe_coordinates(seed):
    rng = np.random.default_rng(seed)
    near = rng.uniform(-3.0, 4.0, size=(2400, 2))
    far = rng.uniform(-3.0, 4.0, size=(600, 2)) * rng.choice([37.0, 1000.0, 65536.0, 1e7], size=(600, 1))
    return np.concatenate([tu.edge_product(), near.astype(np.float32), far.astype(np.float32)])


@pytest.mark.parametrize("ch", tu.CHANNELS)
@pytest.mark.parametrize("extent", tu.EXTENTS, ids=lambda e: "%dx%d" % e)
def test_sampler_probe_equals_oracle(rt, oracle, extent, ch):
    """One scene per image: all 20 samplers, one probe mesh per sampler; base colour, emission, metallic-roughness read the image
    at the probe coordinates and the normal map at the same coordinates in reverse order. shade_closest_hit payloads and
    any_hit_ignores (alpha from the base-colour image, alpha_mode 1, five cutoffs) must equal the oracle's bit for bit."""
    h, w = extent
    img = tu.random_image(h, w, ch, seed=1000 * h + w + ch)
    uvs = probe_coordinates(h + w + ch)
    n = len(uvs)
    fin = uvs[np.isfinite(uvs).all(axis=1)]
    assert ((fin < 0.0) | (fin > 1.0)).any(axis=1).mean() > 0.5                # the clamped samplers really clamp
    desc = tu.probe_scene(img, uvs, alpha_cutoffs=ALPHA_CUTOFFS)
    osc = oracle.OracleScene().load(desc)
    gsc = rt.Scene(0, instancing="flat").load(desc)
    hits = tu.probe_hits(n * len(tu.SAMPLERS))
    want = osc.shade_closest_hit(hits)
    got = device_payloads(gsc, hits)
    for m, smp in enumerate(tu.SAMPLERS):
        sl = slice(m * n, (m + 1) * n)
        for field in ("albedo_packed", "emission", "material_info", "normal_packed"):
            assert_bits_equal(want[field][sl], got[field][sl], "%s, sampler %s, %dx%dx%d" % (field, smp, h, w, ch))
        distinct = len(np.unique(got["albedo_packed"][sl]))
        assert distinct >= (2 if h * w > 1 else 1), (smp, distinct)             # the probe really varies the payload
    assert_bits_equal(want, got, "probe RayPayload %dx%dx%d" % (h, w, ch))
    ignored = gsc.any_hit_ignores(hits_to_device(hits), len(hits)).cpu().numpy().view(np.uint32)
    want_ignored = osc.any_hit_ignores(hits)
    assert np.array_equal(want_ignored, ignored)
    assert ignored.any() and not ignored.all()
    if ch == 4 and h * w > 1:                                                   # a varying alpha channel against a cutoff inside its range
        for m in range(len(tu.SAMPLERS)):
            if ALPHA_CUTOFFS[m % len(ALPHA_CUTOFFS)] in (0.5, 0.25):
                part = ignored[m * n:(m + 1) * n]
                assert part.any() and not part.all(), tu.SAMPLERS[m]


def _zoo_check(oracle, osc, gsc, hits, what):
    want = osc.shade_closest_hit(hits)
    got = device_payloads(gsc, hits)
    for field in ("albedo_packed", "emission", "material_info", "normal_packed", "transmission_ior_packed", "dist"):
        assert_bits_equal(want[field], got[field], "zoo %s (%s)" % (field, what))
    return want, got


def test_zoo_payloads_equal_oracle_in_every_form_of_the_scene(rt, oracle, monkeypatch):
    """The zoo through every producer of the per-slot uv / tangent record: the one-level host build, the device fast build with
    the default (PLOC) and the radix-tree topology, an in-place update, the two-level form's per-mesh tables, and the two-level
    form after a top-level rebuild. Hit records sit on the three corners, the centroid and interior points of every triangle, so
    a producer that permutes vertices, uv sets or tangents, or takes handedness from another vertex, changes a payload."""
    desc, moved = tu.zoo_scene(), tu.zoo_scene(moved=1)
    hits = tu.zoo_hits(desc)
    osc = oracle.OracleScene().load(desc)
    gsc = rt.Scene(0, instancing="flat").load(desc)
    assert not gsc.two_level() and gsc.as_state()[1] == abi.OP_SLOW_BUILD
    want, got = _zoo_check(oracle, osc, gsc, hits, "host build")
    # coverage: the NaN-normal cases were reached (asserted on the oracle payload) and the textures really vary the payload
    per_tri = 10                                                     # records per zoo triangle (tu.zoo_hits)
    zero_n = [k for k, h in enumerate(hits) if int(h["tri"]) in set(tu.zoo_case_gids(desc, (tu.CASE_ZERO_NORMAL,)))]
    assert len(zero_n) == 2 * per_tri and len(set(int(want["normal_packed"][k]) for k in zero_n)) == 1
    par = [k for k, h in enumerate(hits) if int(h["tri"]) in set(tu.zoo_case_gids(desc, (tu.CASE_TANGENT_PARALLEL,)))]
    assert len(par) == 2 * per_tri and not np.isfinite(tu.model_payload(desc, tu.flatten(desc), hits[par[0]])["normal"]).any()
    assert len(np.unique(got["albedo_packed"])) > 500 and len(np.unique(got["normal_packed"])) > 1000
    # only base_color_tex_coord and normal_tex_coord may influence the payload
    other = rt.Scene(0, instancing="flat").load(tu.zoo_scene(uv_seed_shift=1))
    assert_bits_equal(got, device_payloads(other, hits), "payload after changing the metallic-roughness, occlusion and emissive uv sets")
    # device fast build, default topology
    gsc.force_next_op(abi.OP_FAST_BUILD); gsc.set_instances(desc.instances)
    assert gsc.as_state()[1] == abi.OP_FAST_BUILD and gsc.bvh_stats().sah_cost == 0.0
    _zoo_check(oracle, osc, gsc, hits, "device fast build")
    # in-place update of the device-built structure (moved instances)
    gsc.set_instances(moved.instances); osc.set_instances(moved.instances)
    assert gsc.as_state()[1] == abi.OP_UPDATE
    _zoo_check(oracle, osc, gsc, hits, "in-place update")
    osc.set_instances(desc.instances)
    # device fast build, radix-tree topology (the switch is read when the scene is created)
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    rsc = rt.Scene(0, instancing="flat").load(desc)
    monkeypatch.delenv("SR_FAST_BUILD")
    rsc.force_next_op(abi.OP_FAST_BUILD); rsc.set_instances(desc.instances)
    assert rsc.as_state()[1] == abi.OP_FAST_BUILD and rsc.bvh_stats().sah_cost == 0.0
    _zoo_check(oracle, osc, rsc, hits, "device fast build, radix tree")
    # in-place update of the host-built structure
    hsc = rt.Scene(0, instancing="flat").load(desc)
    hsc.set_instances(moved.instances); osc.set_instances(moved.instances)
    assert hsc.as_state()[1] == abi.OP_UPDATE
    _zoo_check(oracle, osc, hsc, hits, "in-place update of the host build")
    osc.set_instances(desc.instances)
    # two-level: per-mesh records, the instance comes from the hit
    tsc = rt.Scene(0, instancing="two_level").load(desc)
    assert tsc.two_level()
    _zoo_check(oracle, osc, tsc, hits, "two-level")
    tsc.set_instances(moved.instances); osc.set_instances(moved.instances)
    assert tsc.two_level()
    _zoo_check(oracle, osc, tsc, hits, "two-level after a top-level rebuild")


def test_zoo_any_hit_equals_oracle(rt, oracle):
    """any_hit_ignores reads the base-colour uv set only, at all three vertices, in the flat and the two-level form."""
    desc = tu.zoo_scene()
    for k, m in enumerate(desc.meshes):
        m.material = m.material.copy()
        m.material["alpha_mode"] = 1
        m.material["alpha_cutoff"] = [0.5, 0.3, 0.7][k % 3]
    hits = tu.zoo_hits(desc)
    osc = oracle.OracleScene().load(desc)
    want = osc.any_hit_ignores(hits)
    assert 0.1 < want.mean() < 0.9
    for form in ("flat", "two_level"):
        gsc = rt.Scene(0, instancing=form).load(desc)
        got = gsc.any_hit_ignores(hits_to_device(hits), len(hits)).cpu().numpy().view(np.uint32)
        assert np.array_equal(want, got), form


def test_room_frames_equal_oracle(rt, oracle, blue_noise):
    """ris_kernel and final_kernel instantiate the textured shading on their own. Three frames of the texture room (NEAREST +
    REPEAT, NEAREST + MIRRORED_REPEAT, LINEAR + CLAMP_TO_EDGE on both axes, 100x37, 1x7 and 7x1 images, negative and > 1000 uv
    scales, a wall with NaN uvs, emissive textured quads, mirrored instances of the zoo mesh): every G-buffer image, reservoir and
    radiance value bit for bit, in the one-level and the two-level form."""
    W, H = 160, 96
    desc = tu.texture_room()
    osc, gsc, of, gf = run_both(rt, oracle, desc, W, H, 3, blue_noise)
    img = gf.host()
    assert len(np.unique(img["diffuse"])) > 300 and len(np.unique(img["normal"])) > 300         # the textures reach the G-buffer
    assert np.isfinite(img["raw_color"]).all() and (img["raw_color"][:, :3].sum(axis=1) > 0).mean() > 0.5
    frames_equal_oracle(rt, oracle, desc, W, H, 2, blue_noise)


def test_room_frames_after_a_device_fast_build(rt, oracle, blue_noise):
    """The same room after a forced device fast build: the pass kernels read the uv / tangent records lbvh_leaves_kernel wrote."""
    W, H = 160, 96
    desc = tu.texture_room()
    osc = oracle.OracleScene().load(desc)
    gsc = rt.Scene(0, instancing="flat").load(desc)
    gsc.force_next_op(abi.OP_FAST_BUILD); gsc.set_instances(desc.instances)
    assert gsc.as_state()[1] == abi.OP_FAST_BUILD and gsc.bvh_stats().sah_cost == 0.0
    of, gf = oracle.HostFrame(W, H, blue_noise), rt.DeviceFrame(W, H, blue_noise)
    prev = None
    for f in range(2):
        om = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        gm = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        prev = list(om.view_proj)
        osc.trace_ris(of, om, f); gsc.trace_ris(gf, gm, f)
        osc.trace_final(of, om, f); gsc.trace_final(gf, gm, f)
        h = gf.host()
        for name, a, b in (("depth", of.depth, h["depth"]), ("normal", of.normal, h["normal"]), ("diffuse", of.diffuse, h["diffuse"]),
                           ("reservoirs", of.reservoirs[f & 1], h["reservoirs"][f & 1]), ("raw_color", of.raw_color, h["raw_color"])):
            assert_bits_equal(a, b, "%s f%d (room, device fast build)" % (name, f))
