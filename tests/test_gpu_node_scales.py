"""The quantised node's three grid scales (csrc/bvh_layout.h: the fp32 numbers 2^e in dwords 3, 10 and 11) through every code
path that writes them — the host collapser, the device build, the device refit, and the per-mesh / top-level trees of the
two-level form — and through the node step that reads them: sr_trace_closest / sr_trace_any against the oracle's brute force,
bit for bit, on a scene whose nodes need scales from the smallest the builders emit (2^-126: an axis without extent) to 2^42.
The rays carry their own tmin (negative, zero, the passes' 0.001, 0.5) and tmax: the ray-list tracers keep per-ray bounds while
the passes compile theirs in (traverse.h FIXED_TMIN / FIXED_TMAX)."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import assert_bits_equal  # noqa: E402
from test_oracle_trace import make_rays  # noqa: E402

N_RAYS = 4096
TMINS = np.array([-1.0, 0.0, 0.001, 0.5], dtype=np.float32)
TINY, HUGE = 1.0e-18, 1.0e15


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def tile_cloud(n_tiles, spread, tile, seed):
    """`n_tiles` square tiles (two triangles each) of edge `tile`, facing random axis directions, scattered over a cube of
    half-width `spread`: a mesh whose extent is ~2 * spread on all three axes while every triangle stays small enough for the
    fp32 triangle test (a triangle with edges of 1e15 overflows it)."""
    rng = np.random.default_rng(seed)
    pos, nrm, idx = [], [], []
    for t in range(n_tiles):
        c = (rng.random(3) * 2 - 1) * spread
        axis = t % 3
        u, v = np.zeros(3), np.zeros(3)
        u[(axis + 1) % 3] = tile; v[(axis + 2) % 3] = tile
        n = np.zeros(3); n[axis] = 1.0
        base = len(pos)
        pos += [c, c + u, c + u + v, c + v]
        nrm += [n] * 4
        idx += [base, base + 1, base + 2, base, base + 2, base + 3]
    return scenes.make_vertices(np.array(pos, dtype=np.float32), np.array(nrm, dtype=np.float32)), np.array(idx, dtype=np.uint32)


def extreme_scene():
    """Three meshes under identity transforms: a sphere of radius 1e-18 at the origin (80 triangles), a cloud of 64 tiles spread
    over +-1e15 (128 triangles), and an axis-aligned quad in the plane y = 0 (no extent on y: its own tree in the two-level form gets the smallest scale there)."""
    s = scenes.SceneDesc("extreme_scales", camera_pos=(0.0, 1.0, 3.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    sv, si = scenes.uv_sphere(TINY, 8, 6)
    s.meshes.append(scenes.MeshDesc(1, sv, si, grey))
    hv, hi = tile_cloud(64, HUGE, 1.0e10, 3)
    s.meshes.append(scenes.MeshDesc(2, hv, hi, grey))
    qv, qi = scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(3, qv, qi, grey))
    assert all(len(m.indices) // 3 <= 200 for m in s.meshes)
    s.instances = [(k, [abi.IDENTITY_TRANSFORM.copy()]) for k in (1, 2, 3)]
    return s


def moved_instances():
    """The tile cloud shifted by exactly representable amounts and the quad slid inside its plane (it keeps y = 0)."""
    return [(1, [abi.IDENTITY_TRANSFORM.copy()]), (2, [scenes.translate(2.0 ** 44, -(2.0 ** 43), 2.0 ** 42)]),
            (3, [scenes.translate(0.125, 0.0, 0.25)])]


def world_triangles(desc, instances):
    """[n, 3, 3] float64 world-space vertices, in the global (instance-major) triangle order; translations only."""
    out = []
    for key, xs in instances:
        m = next(m for m in desc.meshes if m.key == key)
        p = m.vertices["position"].astype(np.float64)[m.indices.reshape(-1, 3)]
        for x in xs:
            x = np.asarray(x, dtype=np.float64)
            out.append(p * x[[0, 5, 10]] + x[[3, 7, 11]])
    return out


def rays_for(desc, instances, seed):
    """N_RAYS rays: per mesh, rays aimed at points of its triangles from origins at that mesh's own scale and from the other
    scales; axis-parallel rays (some inside the quad's plane); tmin drawn from TMINS, tmax from {1e4, 3e38, a short segment}.
    The 1e-18 sphere is shot at along the coordinate axes from 0.5..3 units away (only an axis-parallel ray, whose two other origin
    coordinates are exact, can be aimed at something that small from there). From an origin 1e-18 away a hit on it is ill-posed in
    fp32 whatever the tree: t = dot(e2, cross(tvec, e1)) / det has a numerator of ~1e-54, which underflows to +-0, so every triangle
    the ray's line crosses "hits" at t = 0 and the winner of that tie depends on which of them a traversal may cull after the
    first. Rays that start that close therefore carry tmin >= 0, which excludes t = 0, and hit what lies beyond."""
    rng = np.random.default_rng(seed)
    groups = world_triangles(desc, instances)
    scales = (3.0 * TINY, 4.0 * HUGE, 3.0)
    o, d = [], []
    per = N_RAYS // 4
    for g, tris in enumerate(groups):
        n = per
        tri = tris[rng.integers(0, len(tris), n)]
        b = rng.dirichlet((1.0, 1.0, 1.0), n)
        target = (tri * b[:, :, None]).sum(1)
        own = rng.random(n) < 0.7
        scale = np.where(own, scales[g], np.asarray(scales)[rng.integers(0, 3, n)])
        origin = ((rng.random((n, 3)) * 2 - 1) * scale[:, None]).astype(np.float32).astype(np.float64)
        direction = target - origin
        direction /= np.maximum(np.linalg.norm(direction, axis=1, keepdims=True), 1e-300)
        if g == 0:
            k = rng.integers(0, 3, n)
            side = rng.choice([-1.0, 1.0], n)
            along = np.zeros((n, 3)); along[np.arange(n), k] = 1.0
            axial = target.astype(np.float32).astype(np.float64) * (1.0 - along) + along * (side * (0.5 + 2.5 * rng.random(n)))[:, None]
            use = rng.random(n) < 0.7
            origin[use] = axial[use]
            direction[use] = (-along * side[:, None])[use]
        o.append(origin); d.append(direction)
    n = N_RAYS - 3 * per
    origin = (rng.random((n, 3)) * 2 - 1) * np.asarray(scales)[rng.integers(0, 3, n)][:, None]
    origin[: n // 4, 1] = 0.0                                    # in the quad's plane
    direction = np.zeros((n, 3))
    direction[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    o.append(origin); d.append(direction)
    rays = make_rays(np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32))
    rays["tmin"] = TMINS[rng.integers(0, len(TMINS), N_RAYS)]
    start_tiny = np.abs(rays["origin"]).max(1) < 1.0e-9
    rays["tmin"][start_tiny] = np.maximum(rays["tmin"][start_tiny], np.float32(0.0))
    rays["tmax"] = np.asarray([1.0e4, 3.0e38, 2.5], dtype=np.float32)[rng.integers(0, 3, N_RAYS)]
    far = np.abs(rays["origin"]).max(1) > 1.0e6
    rays["tmax"][far] = 3.0e38                                   # rays of the large scale need the length
    assert len(rays) == N_RAYS
    return rays


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's brute-force answers, computed once: (desc, {instances name: (instances, rays, closest, any)})."""
    desc = extreme_scene()
    out = {}
    for name, inst in (("base", desc.instances), ("moved", moved_instances())):
        osc = oracle.OracleScene().load(desc)
        osc.set_instances(inst)
        osc.set_brute_force(True)
        rays = rays_for(desc, inst, 11 if name == "base" else 12)
        closest, occluded = osc.trace_closest(rays), osc.trace_any(rays)
        osc.close()
        # the rays reach every mesh: global triangle ids are instance-major (sphere 0..79, cloud 80..207, quad 208..209)
        gid = closest["tri"][closest["t"] >= 0]
        assert ((gid < 80).sum() > 20) and (((gid >= 80) & (gid < 208)).sum() > 200) and ((gid >= 208).sum() > 200), np.bincount(np.digitize(gid, [80, 208]))
        assert 0.2 < occluded.mean() < 0.95
        out[name] = (inst, rays, closest, occluded)
    return desc, out


def check(rt, gsc, ref, what):
    _, rays, closest, occluded = ref
    rd = rt.rays_to_device(rays)
    assert_bits_equal(closest, rt.hits_from_device(gsc.trace_closest(rd, len(rays))), "closest hits, " + what)
    assert np.array_equal(occluded, gsc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32)), "occlusion, " + what


def test_host_tree(rt, reference):
    desc, ref = reference
    gsc = rt.Scene(0).load(desc)
    assert gsc.as_state()[1] == abi.OP_SLOW_BUILD and gsc.bvh_stats().sah_cost > 0.0 and not gsc.two_level()
    check(rt, gsc, ref["base"], "host SAH tree")
    gsc.close()


def test_device_built_trees(rt, reference):
    """Trees the device builds: a one-level scene this small is always built by the host (fewer than 4096 triangles), so the device
    builds are the two-level form's — every mesh tree and the top-level tree."""
    desc, ref = reference
    gsc = rt.Scene(0, instancing="two_level").set_mesh_tree_build("device").set_top_level_build("device").load(desc)
    keys = [m.key for m in desc.meshes]
    for k in keys:
        gsc.set_mesh_build_type(k, abi.BUILD_SOMETIMES_CHANGES)
    gsc.force_next_op(abi.OP_FAST_BUILD)
    for m in desc.meshes:
        gsc.update_mesh(m.key, m.vertices)
    gsc.set_instances(desc.instances)
    info = gsc.mesh_tree_info()
    assert (info.built_on_device, info.built_on_host, info.reason) == (len(keys), 0, abi.MESH_TREE_ON_DEVICE)
    assert gsc.two_level() and gsc.top_level_info().on_device
    check(rt, gsc, ref["base"], "device-built trees")
    gsc.close()


def test_device_refit_of_moved_meshes(rt, reference):
    desc, ref = reference
    gsc = rt.Scene(0).load(desc)
    gsc.set_instances(ref["moved"][0])
    assert gsc.as_state()[1] == abi.OP_UPDATE
    check(rt, gsc, ref["moved"], "device refit")
    gsc.close()


def test_two_level_form(rt, reference):
    desc, ref = reference
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    assert gsc.two_level()
    check(rt, gsc, ref["base"], "two-level form")
    gsc.set_instances(ref["moved"][0])
    assert gsc.two_level()
    check(rt, gsc, ref["moved"], "two-level form, moved instances")
    gsc.close()
