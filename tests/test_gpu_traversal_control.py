"""The control skeleton of traverse_ws (loop-top lane masks, the early-exit thresholds, "next node" with its two pops) on the
smallest trees that reach each of its branches, against the oracle's brute force, bit for bit.

Trees: seeded soups of 1, 2, 3, 4, 5, 9 and 40 triangles — a root with 1-4 children, leaves of one and of two triangles, depth
2-3 — half of the seeds with a coincident twin of triangle 0 as the last triangle (the tie rule: smallest t, then lowest id).
Ray counts 1, 63, 64, 65 and 130: a partial wave, a full one, a wave boundary, and lanes without a ray of their own, which take
over other lanes' stack entries. Ray kinds, interleaved so every count holds all of them: rays aimed at a triangle, rays from
outside pointing away (they miss every child of the root: the first pop finds the stack empty), random rays, and segments that end
just short of / just beyond the aimed triangle (existence queries on both sides of the hit). The same soups run in the two-level
form under 2-3 instances, where leaving an instance meets the double pop. Two tiny Cornell-box frames go through both passes.
"""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
from test_gpu_parity import assert_bits_equal, run_both  # noqa: E402
from test_gpu_two_level import frames_equal_oracle  # noqa: E402

SEEDS = 24
COUNTS = (1, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (select them with -m gpu on a machine that has one)")
    from sunray_amd import runtime
    return runtime


def soup(rng, n, twin):
    c = rng.normal(size=(n, 3))
    e = rng.normal(size=(n, 2, 3)) * 0.6
    tri = np.concatenate([c[:, None], c[:, None] + e], axis=1)             # [n, 3, 3]
    if twin and n >= 2:
        tri[-1] = tri[0]
    pos = tri.reshape(-1, 3).astype(np.float32)
    nrm = np.tile(np.array([[0, 1, 0]], np.float32), (3 * n, 1))
    return scenes.make_vertices(pos, nrm), np.arange(3 * n, dtype=np.uint32)


def rigid(rng, shift):
    a, b = rng.uniform(0, 2 * np.pi, 2)
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    M = np.zeros((3, 4)); M[:, :3] = (Rx @ Ry) * rng.uniform(0.5, 1.5); M[:, 3] = shift
    return M.astype(np.float32).reshape(12)


def world_triangles(desc):
    out = []
    m = desc.meshes[0]
    for M in desc.instances[0][1]:
        M = np.asarray(M, np.float64).reshape(3, 4)
        out.append(m.vertices["position"].astype(np.float64) @ M[:, :3].T + M[:, 3])
    return np.concatenate(out).reshape(-1, 3, 3)


def rays_for(rng, tris, n):
    """n rays cycling through the five kinds."""
    r = np.zeros(n, dtype=abi.RAY)
    centre = tris.reshape(-1, 3).mean(axis=0)
    radius = float(np.abs(tris.reshape(-1, 3) - centre).max()) + 1.0
    for i in range(n):
        kind = i % 5
        o = centre + rng.normal(size=3) * radius * 1.5
        tmin, tmax = 0.001, 1.0e4
        t = tris[rng.integers(0, len(tris))]
        w = rng.dirichlet((1.0, 1.0, 1.0))
        aim = w[0] * t[0] + w[1] * t[1] + w[2] * t[2]
        dist = float(np.linalg.norm(aim - o))
        if kind == 0:
            d = aim - o
        elif kind == 1:                                     # from outside the bounds, pointing away from them
            o = centre + (rng.choice([-1.0, 1.0], 3) * radius * 3.0)
            d = o - centre
        elif kind == 2:
            d = rng.normal(size=3)
        elif kind == 3:
            d = aim - o; tmax = dist * (1.0 - 1.0e-3)
        else:
            d = aim - o; tmax = dist * (1.0 + 1.0e-3)
        r["origin"][i] = o.astype(np.float32)
        r["dir"][i] = (d / max(np.linalg.norm(d), 1e-20)).astype(np.float32)
        r["tmin"][i] = tmin; r["tmax"][i] = tmax
    return r


def check_soups(rt, oracle, n_tris, two_level):
    seen_hit = seen_miss = seen_occluded = seen_free = 0
    for seed in range(SEEDS):
        rng = np.random.default_rng(1000 * n_tris + seed)
        desc = scenes.SceneDesc("soup")
        v, i = soup(rng, n_tris, twin=bool(seed & 1))
        desc.meshes.append(scenes.MeshDesc(1, v, i, abi.material()))
        n_inst = (2 + (seed % 2)) if two_level else 1
        desc.instances.append((1, [rigid(rng, (4.0 * k, 0.5 * k, -3.0 * k)) for k in range(n_inst)]))
        osc = oracle.OracleScene().load(desc)
        osc.set_brute_force(True)
        gsc = rt.Scene(0, instancing="two_level").load(desc) if two_level else rt.Scene(0).load(desc)
        assert gsc.two_level() == two_level
        tris = world_triangles(desc)
        for n in COUNTS:
            rays = rays_for(rng, tris, n)
            rd = rt.rays_to_device(rays)
            got = rt.hits_from_device(gsc.trace_closest(rd, n))
            occ = gsc.trace_any(rd, n).cpu().numpy().view(np.uint32)
            want, want_occ = osc.trace_closest(rays), osc.trace_any(rays)
            what = "%d triangles, seed %d, %d rays, %s" % (n_tris, seed, n, "two-level" if two_level else "one-level")
            assert_bits_equal(want, got, "closest hits (%s)" % what)
            assert np.array_equal(want_occ, occ), "existence queries (%s)" % what
            seen_hit += int((want["t"] >= 0).sum()); seen_miss += int((want["t"] < 0).sum())
            seen_occluded += int((want_occ != 0).sum()); seen_free += int((want_occ == 0).sum())
    # the ray kinds did what they are there for
    assert seen_hit > 0 and seen_miss > 0 and seen_occluded > 0 and seen_free > 0


@pytest.mark.parametrize("n_tris", [1, 2, 3, 4, 5, 9, 40])
def test_small_trees_one_level(rt, oracle, n_tris):
    check_soups(rt, oracle, n_tris, two_level=False)


@pytest.mark.parametrize("n_tris", [1, 2, 3, 4, 5, 9, 40])
def test_small_trees_two_level(rt, oracle, n_tris):
    check_soups(rt, oracle, n_tris, two_level=True)


def test_twin_triangles_resolve_to_the_lower_index(rt, oracle):
    """Two coincident triangles in one leaf pair and in different leaves: the hit is the lower global index."""
    for n_tris in (2, 5):
        rng = np.random.default_rng(77 + n_tris)
        desc = scenes.SceneDesc("twins")
        v, i = soup(rng, n_tris, twin=True)
        desc.meshes.append(scenes.MeshDesc(1, v, i, abi.material()))
        desc.instances.append((1, [rigid(rng, (0.0, 0.0, 0.0))]))
        tris = world_triangles(desc)
        aim = tris[0].mean(axis=0)
        o = aim + np.cross(tris[0][1] - tris[0][0], tris[0][2] - tris[0][0]) * 3.0 + 0.01
        rays = np.zeros(65, dtype=abi.RAY)
        rays["origin"] = o.astype(np.float32); rays["dir"] = ((aim - o) / np.linalg.norm(aim - o)).astype(np.float32)
        rays["tmin"] = 0.001; rays["tmax"] = 1.0e4
        osc = oracle.OracleScene().load(desc); osc.set_brute_force(True)
        gsc = rt.Scene(0).load(desc)
        want = osc.trace_closest(rays)
        got = rt.hits_from_device(gsc.trace_closest(rt.rays_to_device(rays), len(rays)))
        assert (want["t"] >= 0).all()
        assert_bits_equal(want, got, "twin triangles (%d)" % n_tris)


@pytest.mark.parametrize("W,H", [(8, 8), (5, 3)])
def test_tiny_frames_one_level(rt, oracle, blue_noise, W, H):
    run_both(rt, oracle, scenes.cornell_box(), W, H, 2, blue_noise)


@pytest.mark.parametrize("W,H", [(8, 8), (5, 3)])
def test_tiny_frames_two_level(rt, oracle, blue_noise, W, H):
    frames_equal_oracle(rt, oracle, scenes.cornell_box(), W, H, 2, blue_noise)
