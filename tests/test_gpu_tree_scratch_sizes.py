"""The scratch of the device tree builder is reserved to the byte (csrc/bvh_gpu.hip TreeScratch: the size functions return the
end of the carve the build itself uses), so a build that needed one byte more than was reserved would fail with
hipErrorOutOfMemory. A scene's scratch buffer only grows: a second build in one scene could hide behind an earlier, larger
reservation. Every case here therefore builds ONE tree on the device in a FRESH scene, at sizes around the 256-byte alignment of the
carve and the 256-thread blocks of the launches, under both topologies of the fast build: mesh trees, the top level, the one-level
form, and the height bound's own arrays.

The issue also asked for a top-level list with a NaN-box row (sorted items > primitives). No list the scene accepts reaches the device
build with one: tl_records_kernel leaves a row without a box only for a mesh of zero triangles, which sr_scene_add_mesh refuses,
and every other boxless record (a baked instance, a box that is not finite) sends the list to the host. That case is left to the
size table of profiles/tree_builder_refactor.json, which covers sorted items > primitives."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_refit import records_equal_numpy, tree_contains_its_triangles  # noqa: E402
from test_gpu_mesh_tree_batch import floor_and, grid_mesh  # noqa: E402
from test_gpu_mesh_tree_build import SEVEN_BOX, TOPOLOGIES, chain_mesh, device_scene, tree_info  # noqa: E402
from test_gpu_mesh_update import push, ray_set, traces_equal_brute_force, with_vertices  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402
from test_gpu_top_level_build import affine_transforms, assert_path, check_structure  # noqa: E402
from test_oracle_trace import make_rays, random_rays  # noqa: E402

F = abi.OP_FAST_BUILD
MESH = abi.TREE_KIND_MESH
CAP = abi.MESH_TREE_STACK_CAP
ON_DEVICE = abi.MESH_TREE_ON_DEVICE


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def few_hundred(rays):
    return np.ascontiguousarray(rays[::32])


# ---- 1. mesh trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("n_tris", [1, 2, 3, 63, 64, 65, 255, 256, 257])
def test_a_fresh_scenes_first_mesh_tree_build_fits_its_scratch(rt, oracle, monkeypatch, topology, n_tris):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = floor_and([grid_mesh(1, n_tris)], "scratch_%d" % n_tris)
    rays = few_hundred(ray_set(oracle, desc, SEVEN_BOX, 31))
    gsc = device_scene(rt, desc, [1]).set_mesh_tree_batch("off")
    desc = scenes.deform(desc, [1], 1.0, amplitude=0.05)
    gsc.force_next_op(F)
    push(gsc, desc, [1])
    assert tree_info(gsc) == (1, 0, ON_DEVICE), tree_info(gsc)
    what = "%s, %d triangles" % (topology, n_tris)
    tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, 1, what), what)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rt.rays_to_device(rays), what)
    gsc.close()


# ---- 2. the top level --------------------------------------------------------------------------------------------------------
def one_triangle_instances(n):
    """n instances of a one-triangle mesh under general affine transforms inside a box of 8 units -> (description, rays: random
    ones and one aimed at a point inside every instance's triangle)"""
    desc = scenes.SceneDesc("one_triangle_x%d" % n, camera_pos=(0.0, 1.0, 9.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    v = scenes.make_vertices(np.array([(0, 0, 0), (1, 0, 0.25), (0, 1.5, 0)], dtype=np.float32), np.tile(np.array((0, 0, 1), dtype=np.float32), (3, 1)))
    desc.meshes.append(scenes.MeshDesc(1, v, np.array([0, 1, 2], dtype=np.uint32), abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)))
    xf = affine_transforms(n, 500 + n, translation=4.0)
    desc.instances = [(1, list(xf))]
    box = ((-6, -6, -6), (6, 6, 6))
    aimed = random_rays(n, 7, box=box)
    inside = xf.reshape(n, 3, 4) @ np.array([0.3, 0.4, 0.075, 1.0], dtype=np.float32)       # a point inside each instance's triangle
    aimed = make_rays(aimed["origin"], (inside - aimed["origin"]).astype(np.float32))
    return desc, np.concatenate([random_rays(300, 8, box=box), aimed])


@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("n", [2, 3, 64, 65, 257])
def test_a_fresh_scenes_first_top_level_build_fits_its_scratch(rt, oracle, monkeypatch, topology, n):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc, rays = one_triangle_instances(n)
    xf = desc.instances[0][1]
    gsc = rt.Scene(0, instancing="two_level").set_top_level_build("device")
    gsc.add_mesh(1, desc.meshes[0].vertices, desc.meshes[0].indices, desc.meshes[0].material)
    gsc.set_instances([(1, xf[:-1])])               # the first list is the quality build on the host
    assert gsc.two_level() and not gsc.top_level_info().on_device
    gsc.set_instances(desc.instances)               # a changed list: the scene's first device build
    info = assert_path(gsc, "device")
    assert info.n_boxes == n and info.n_instances == n
    what = "%s, %d instances" % (topology, n)
    check_structure(rt, gsc, what)
    osc = oracle.OracleScene().load(desc)
    osc.set_brute_force(True)
    rd = rt.rays_to_device(rays)
    want = osc.trace_closest(rays)
    assert (want["t"] >= 0).sum() >= n // 2         # the aimed rays find their triangles
    assert_bits_equal(want, rt.hits_from_device(gsc.trace_closest(rd, len(rays))), "closest hits, " + what)
    assert np.array_equal(osc.trace_any(rays), gsc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32)), "occlusion, " + what
    osc.close()
    gsc.close()


# ---- 3. the one-level form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("n_tris", [4096, 4097])
def test_a_fresh_scenes_first_one_level_fast_build_fits_its_scratch(rt, oracle, monkeypatch, topology, n_tris):
    """After the pattern of test_device_lbvh_fast_build: the forced fast build of a scene at and just above the smallest size the
    device takes."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = scenes.SceneDesc("grid_%d" % n_tris, camera_pos=(0.0, 1.5, 3.0), camera_target=(0.0, 0.0, 0.5), fov_y=45.0)
    desc.meshes.append(grid_mesh(1, n_tris))
    desc.instances = [(1, [scenes.translate(0.0, 0.0, 0.0)])]
    osc = oracle.OracleScene().load(desc)
    gsc = rt.Scene(0).load(desc)
    gsc.force_next_op(F)
    gsc.set_instances(desc.instances)
    st = gsc.bvh_stats()
    assert gsc.as_state()[1] == F and st.n_triangles == n_tris and st.sah_cost == 0.0      # built on the device
    rays = random_rays(400, 9, box=((-1.2, -0.5, -0.7), (1.2, 1.0, 1.7)))
    rd = rt.rays_to_device(rays)
    want = osc.trace_closest(rays)
    assert (want["t"] >= 0).mean() > 0.03
    assert_bits_equal(want, rt.hits_from_device(gsc.trace_closest(rd, len(rays))), "closest hits (%s, %d triangles)" % (topology, n_tris))
    assert np.array_equal(osc.trace_any(rays), gsc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32))
    osc.close()
    gsc.close()


# ---- 4. the height bound -----------------------------------------------------------------------------------------------------
def test_a_fresh_scenes_first_rebalanced_build_fits_its_scratch(rt, oracle, monkeypatch):
    """The 63-triangle chain of test_gpu_tree_height_bound.py, whose radix tree is some 60 levels tall: the rebalancing pass, which
    alone uses the link, position and gap arrays, runs in the scene's first device build."""
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    chain = chain_mesh(9)
    desc = floor_and([chain], "scratch_chain")
    rays = few_hundred(ray_set(oracle, desc, SEVEN_BOX, 33))
    gsc = device_scene(rt, desc, [9]).set_mesh_tree_batch("off").set_tree_height_bound("rebalance")
    moved = chain.vertices.copy()
    moved["normal"] = np.array((0, 1, 0), dtype=np.float32)
    desc = with_vertices(desc, 9, moved)
    gsc.force_next_op(F)
    push(gsc, desc, [9])
    hi = gsc.tree_height_info(MESH)
    assert tree_info(gsc) == (1, 0, ON_DEVICE) and hi.on_device == 1
    assert hi.height_before > CAP and hi.height_after <= CAP and hi.subtrees_rebuilt >= 1 and gsc.mesh_tree_info().max_stack <= CAP
    tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, 9, "the rebalanced chain"), "the rebalanced chain")
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rt.rays_to_device(rays), "the rebalanced chain")
    gsc.close()
