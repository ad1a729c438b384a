"""Device-built trees against the reference builder of tests/tree_build_reference.py, word for word: mesh trees of the two-level form
(per mesh and batched, radix tree and PLOC at three radii, with and without the height bound), their refit, the top level, and the
one-level form. The reference predicts every word of a tree up to the numbers of its nodes (they come from atomic counters), so
both sides are renumbered breadth-first in child order and compared as arrays, together with the leaf order, the node count, the
stack need and the height bound's report. Every comparison is an equality; a tree the reference refuses for its height must be
one the device left to the host.

The check_* functions take arrays only (what the device was given, what it produced): they can be run again on recorded data."""
import dataclasses
import os
import sys
import time

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_build_reference as ref  # noqa: E402
from test_gpu_mesh_tree_batch import floor_and, grid_mesh, repeated_triangle_mesh  # noqa: E402
from test_gpu_mesh_tree_build import chain_mesh, device_scene, seven_meshes, tree_info  # noqa: E402
from test_gpu_mesh_update import push, with_vertices  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402
from test_gpu_top_level_build import affine_transforms, small_mesh_scene  # noqa: E402

F, U = abi.OP_FAST_BUILD, abi.OP_UPDATE
ONE, TOP, MESH = abi.TREE_KIND_ONE_LEVEL, abi.TREE_KIND_TOP_LEVEL, abi.TREE_KIND_MESH
MESH_TOPOLOGIES = ["lbvh", "ploc1", "ploc2", "ploc16"]
TOPOLOGIES = ["lbvh", "ploc16"]
ONE_LEVEL_CAP = 47      # stack entries of the one-level walk (sr_scene_tree_height_info reports it as the build's cap)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def layout(rt):
    return ref.Layout(*rt.bvh_layout(), rt.tree_build_limits(MESH, 1)[0])


def radius_of(topology):
    return 0 if topology == "lbvh" else int(topology[4:])


def height_fields(i):
    return (i.height_before, i.height_after, i.subtrees_rebuilt, i.prims_rebuilt)


def report(kind, what, n_nodes, n_prims, seconds):
    print("tree-build-reference: %-9s %-58s %5d nodes %5d primitives, reference %.3f s" % (kind, what, n_nodes, n_prims, seconds))


# ---- the comparisons: arrays in, assertions out ---------------------------------------------------------------------------------
def check_mesh_tree(layout, what, corners, radius, cap, rebalance, depth, dev):
    """corners [n, 3, 3]: the vertex positions of every primitive. dev: what the scene reports and holds after the build.
    -> the reference's tree (None: refused)."""
    t0 = time.perf_counter()
    lo, hi = ref.boxes_of_vertex_records(corners[:, 0], corners[:, 1], corners[:, 2])
    want = ref.build(lo, hi, layout, radius, min(depth, cap), cap, rebalance=rebalance, single_ok=True)
    seconds = time.perf_counter() - t0
    if want.refused or want.max_stack > cap:
        assert not dev["on_device"], "%s: the reference refuses this tree (binary height %d, cap %d), the device built it" % (what, want.height_before, cap)
        report("mesh", what + " (refused)", 0, len(corners), seconds)
        return None
    assert dev["on_device"], "%s: the device left to the host a tree the reference builds (binary height %d, cap %d)" % (what, want.height_before, cap)
    ref.assert_trees_equal(dev["nodes"], dev["prim_of_slot"], want.nodes, want.order, layout, what, want)
    assert_bits_equal(want.order, dev["prim_of_slot"], "%s: primitives in leaf order" % what)
    assert_bits_equal(want.slot_of_prim, dev["slot_of_prim"], "%s: slot_of_prim" % what)
    assert (dev["n_nodes"], dev["max_stack"]) == (want.n_nodes, want.max_stack), "%s: nodes and stack need" % what
    if len(corners) > 1:
        assert dev["height"] == (want.height_before, want.height_after, want.subtrees_rebuilt, want.prims_rebuilt), "%s: the height bound's report" % what
    report("mesh", what, want.n_nodes, len(corners), seconds)
    return want


def check_refit(layout, what, corners, built_nodes, order, dev):
    """The refitted nodes are the reference quantiser over the same topology and the new vertices."""
    t0 = time.perf_counter()
    lo, hi = ref.boxes_of_vertex_records(corners[:, 0], corners[:, 1], corners[:, 2])
    nodes = built_nodes.copy()
    ref.quantise_tree(nodes, lo[order], hi[order], layout)
    seconds = time.perf_counter() - t0
    ref.assert_trees_equal(dev["nodes"], dev["prim_of_slot"], nodes, order, layout, what)
    assert_bits_equal(order, dev["prim_of_slot"], "%s: primitives in leaf order" % what)
    report("refit", what, len(nodes), len(corners), seconds)


def check_top_level(layout, what, boxes, radius, floor, stack_cap, blas_stack, dev):
    """boxes [n_instances, 6]: a NaN row where the instance has no box."""
    t0 = time.perf_counter()
    has_box = np.isfinite(boxes).all(axis=1)
    cap = stack_cap - blas_stack - layout.leaf_max - 1
    want = ref.build(boxes[:, :3], boxes[:, 3:], layout, radius, floor, cap, spread_ties=True, has_box=has_box)
    seconds = time.perf_counter() - t0
    if want.refused or want.max_stack + layout.leaf_max + blas_stack + 1 > stack_cap:
        assert not dev["on_device"], "%s: the reference refuses this tree, the device built it" % what
        report("top level", what + " (refused)", 0, int(has_box.sum()), seconds)
        return
    assert dev["on_device"], "%s: the device left to the host a tree the reference builds" % what
    ref.assert_trees_equal(dev["nodes"], dev["tl_inst"], want.nodes, want.order, layout, what, want)
    assert_bits_equal(want.order, dev["tl_inst"], "%s: tl_inst" % what)
    assert (dev["n_nodes"], dev["max_stack"], dev["n_boxes"]) == (want.n_nodes, want.max_stack, int(has_box.sum())), "%s: nodes, stack need, boxes" % what
    assert dev["height"] == (want.height_before, want.height_after, 0, 0), "%s: the height bound's report" % what
    report("top level", what, want.n_nodes, int(has_box.sum()), seconds)


def world_records(corners, transforms):
    """(v0, e1, e2) of every flattened triangle: rows of the 3x4 transform dotted with (p, 1) left to right, in float32."""
    out = []
    for c, m in zip(corners, transforms):
        m = np.asarray(m, dtype=np.float32).reshape(3, 4)
        w = ((m[:, 0] * c[..., 0:1] + m[:, 1] * c[..., 1:2]) + m[:, 2] * c[..., 2:3]) + m[:, 3] * np.float32(1.0)
        out.append(np.stack([w[:, 0], w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]], axis=1))
    return np.concatenate(out).astype(np.float32)


def check_one_level(layout, what, records, radius, floor, dev):
    """records [n, 3, 3]: (v0, e1, e2) by global triangle id."""
    t0 = time.perf_counter()
    lo, hi = ref.boxes_of_edge_records(records[:, 0], records[:, 1], records[:, 2])
    want = ref.build(lo, hi, layout, radius, floor, ONE_LEVEL_CAP)
    seconds = time.perf_counter() - t0
    assert not want.refused and dev["on_device"], what
    gid = np.ascontiguousarray(dev["tris"]).view(np.uint32)[:, 9]
    ref.assert_trees_equal(dev["nodes"], gid, want.nodes, want.order, layout, what, want)
    rows = np.zeros((len(records), 12), dtype=np.float32)
    rows[:, :9] = records[want.order].reshape(-1, 9)
    rows.view(np.uint32)[:, 9] = want.order
    assert_bits_equal(rows, dev["tris"], "%s: triangle records in leaf order" % what)
    assert (dev["n_nodes"], dev["max_stack"]) == (want.n_nodes, want.max_stack), "%s: nodes and stack need" % what
    assert dev["height"] == (want.height_before, want.height_after, 0, 0), "%s: the height bound's report" % what
    report("one level", what, want.n_nodes, len(records), seconds)


# ---- mesh trees -----------------------------------------------------------------------------------------------------------------
def corners_of(mesh):
    return np.ascontiguousarray(mesh.vertices["position"][np.asarray(mesh.indices, dtype=np.int64).reshape(-1, 3)], dtype=np.float32)


def planar_mesh(key):
    """100 triangles of the waved grid pressed into the plane y = 0."""
    m = grid_mesh(key, 100)
    v = m.vertices.copy()
    v["position"][:, 1] = np.float32(0.0)
    return dataclasses.replace(m, vertices=v)


def corner_mesh(key):
    """40 small triangles in [-100, 0]^3 and a point triangle at (1, 1, 1): the centre of its padded box lies one ulp of 1 below the
    grid's upper corner, far less than the grid's extent resolves, so (p - lo) / ext is exactly 1 on all three axes."""
    rng = np.random.default_rng(40)
    pos = (rng.uniform(-100.0, -1.0, size=(40, 1, 3)) + rng.uniform(0.0, 1.0, size=(40, 3, 3))).reshape(-1, 3)
    pos = np.concatenate([pos, np.ones((3, 3))]).astype(np.float32)
    v = scenes.make_vertices(pos, np.tile(np.array((0, 1, 0), dtype=np.float32), (len(pos), 1)))
    return scenes.MeshDesc(key, v, np.arange(len(pos), dtype=np.uint32), abi.material(base_color=(0.5, 0.5, 0.9, 1.0), roughness=0.5))


def mesh_cases(leaf_max):
    """(name, mesh): sizes around the leaf, the wave and a block, repeated and degenerate triangles, no extent on an axis, the
    key clamp; the refused ones last (the host then rebuilds every tree of the scene)."""
    seven = seven_meshes().meshes
    cases = [("%d triangles" % (len(m.indices) // 3), m) for m in seven[:5]]
    cases.append(("65 triangles, the last repeats the first", seven[5]))
    cases.append(("960 triangles", seven[6]))
    for k, n in enumerate([leaf_max, leaf_max + 1, 2 * leaf_max + 1, 65, 257]):
        cases.append(("grid of %d triangles" % n, grid_mesh(11 + k, n)))
    cases.append(("planar mesh", planar_mesh(21)))
    cases.append(("a centre on the grid's upper corner", corner_mesh(22)))
    cases.append(("300 copies of one triangle", repeated_triangle_mesh(31, 300, False)))
    cases.append(("300 zero-area triangles", repeated_triangle_mesh(32, 300, True)))
    return cases


def bent(vertices):
    v = vertices.copy()
    p = v["position"]
    v["position"] = (p * np.array([1.07, 0.93, 1.11], dtype=np.float32) + np.float32(0.03) * np.sin(np.float32(5.0) * p[:, [1, 2, 0]])).astype(np.float32)
    return v


def device_mesh_tree(gsc, key):
    tree, info = gsc.read_mesh_tree(key), gsc.mesh_tree_info()
    return {"nodes": tree["nodes"], "prim_of_slot": np.ascontiguousarray(tree["tris"]).view(np.uint32)[:, 9].copy(), "slot_of_prim": tree["slot_of_prim"],
            "n_nodes": info.n_nodes, "max_stack": info.max_stack, "on_device": tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE),
            "height": height_fields(gsc.tree_height_info(MESH))}


def build_and_refit(rt, layout, gsc, desc, mesh, what, radius, cap, rebalance):
    """One forced fast build of one mesh against the reference, then one refit of the tree it left."""
    n = len(mesh.indices) // 3
    gsc.force_next_op(F)
    push(gsc, desc, [mesh.key])
    b = gsc.mesh_tree_batch_info()
    assert b.batched + b.passed_on == b.mode, what      # the batch, where it is on, saw the mesh
    want = check_mesh_tree(layout, what, corners_of(mesh), radius, cap, rebalance, rt.tree_build_limits(MESH, n)[1], device_mesh_tree(gsc, mesh.key))
    if want is None:
        on_device, on_host, reason = tree_info(gsc)      # the host then rebuilds this tree and every tree whose host copy is stale
        assert on_device == 0 and on_host >= 1 and reason == abi.MESH_TREE_HOST_STACK_BUDGET, what
        return
    moved = dataclasses.replace(mesh, vertices=bent(mesh.vertices))
    gsc.force_next_op(U)
    push(gsc, with_vertices(desc, mesh.key, moved.vertices), [mesh.key])
    assert gsc.mesh_update_info().blas_refitted == 1 and gsc.mesh_update_info().blas_rebuilt == 0, what
    check_refit(layout, what + ", refitted", corners_of(moved), want.nodes, want.order, device_mesh_tree(gsc, mesh.key))


def assert_the_edge_meshes_are_edges():
    """The reference's own keys say that the corner mesh reaches the clamp and that the planar mesh has one box on y."""
    corners = corners_of(corner_mesh(22))
    lo, hi = ref.boxes_of_vertex_records(corners[:, 0], corners[:, 1], corners[:, 2])
    keys = ref.morton_keys(ref.centres(lo, hi), *ref.grid_bounds(lo, hi))
    assert keys[-1] == (1 << 63) - 1 and max(keys[:-1]) < keys[-1]
    corners = corners_of(planar_mesh(21))
    lo, hi = ref.boxes_of_vertex_records(corners[:, 0], corners[:, 1], corners[:, 2])
    assert (lo[:, 1] == lo[0, 1]).all() and (hi[:, 1] == hi[0, 1]).all()


@pytest.mark.parametrize("batch", ["off", "on"])
@pytest.mark.parametrize("topology", MESH_TOPOLOGIES)
def test_mesh_trees_equal_the_reference(rt, layout, monkeypatch, topology, batch):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    assert_the_edge_meshes_are_edges()
    cases = mesh_cases(layout.leaf_max)
    desc = floor_and([m for _, m in cases], "tree_build_reference")
    gsc = device_scene(rt, desc, [m.key for _, m in cases], abi.BUILD_RAPIDLY_CHANGING).set_mesh_tree_batch(batch)
    for name, mesh in cases:
        what = "%s, %s, batch %s" % (name, topology, batch)
        build_and_refit(rt, layout, gsc, desc, mesh, what, radius_of(topology), abi.MESH_TREE_STACK_CAP, False)
    gsc.close()


@pytest.mark.parametrize("batch", ["off", "on"])
@pytest.mark.parametrize("topology", MESH_TOPOLOGIES)
def test_rebalanced_mesh_trees_equal_the_reference(rt, layout, monkeypatch, topology, batch):
    """The 63-triangle chain at the library's cap and at a cap just above H(63), the 960-triangle sphere at a cap one below its
    binary height (the reference's), and the two meshes of 300 equal triangles, which PLOC chains one pair at a time."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    radius = radius_of(topology)
    chain, sphere = chain_mesh(9), seven_meshes().meshes[6]
    copies, flat = repeated_triangle_mesh(31, 300, False), repeated_triangle_mesh(32, 300, True)
    desc = floor_and([chain, sphere, copies, flat], "tree_build_reference_rebalance")
    corners = corners_of(sphere)
    free = ref.build(*ref.boxes_of_vertex_records(corners[:, 0], corners[:, 1], corners[:, 2]), layout, radius, abi.MESH_TREE_STACK_CAP, 1 << 20)
    h63, h960 = ref.median_height(63, layout.leaf_max), ref.median_height(960, layout.leaf_max)
    assert h960 <= free.height_before - 1
    gsc = device_scene(rt, desc, [9, 7, 31, 32], abi.BUILD_RAPIDLY_CHANGING).set_mesh_tree_batch(batch)
    for mesh, name, cap in ((chain, "chain of 63", 0), (chain, "chain of 63", h63 + 1), (sphere, "960 triangles", free.height_before - 1),
                            (copies, "300 copies of one triangle", 0), (flat, "300 zero-area triangles", 0)):
        gsc.set_tree_height_bound("rebalance", cap)
        what = "%s under cap %d, %s, batch %s" % (name, cap, topology, batch)
        build_and_refit(rt, layout, gsc, desc, mesh, what, radius, cap or abi.MESH_TREE_STACK_CAP, True)
    gsc.close()


# ---- top level ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("n,identical", [(2, False), (3, False), (5, False), (63, False), (64, False), (65, False), (257, False), (9, True), (64, True), (65, True)])
def test_top_level_trees_equal_the_reference(rt, layout, monkeypatch, topology, n, identical):
    """General affine instances around the leaf, the wave and a block, and identical instances, which the tie rule of instance
    boxes halves every PLOC iteration. A list with a row that has no box does not reach the device's build through any call a
    scene accepts (tests/test_gpu_tree_scratch_sizes.py): that case is held against the reference alone, on the host."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    sc = small_mesh_scene(rt, affine_transforms(n, 300 + n, identical=identical), "device")
    info = sc.top_level_info()
    nodes, tl_inst, _, boxes = sc.read_top_level()
    dev = {"nodes": nodes, "tl_inst": tl_inst, "n_nodes": info.n_nodes, "max_stack": info.max_stack, "n_boxes": info.n_boxes,
           "on_device": info.on_device == 1 and info.reason == abi.TL_ON_DEVICE, "height": height_fields(sc.tree_height_info(TOP))}
    assert info.n_instances == n == len(boxes)
    what = "%d %s instances, %s" % (n, "identical" if identical else "affine", topology)
    check_top_level(layout, what, boxes, radius_of(topology), rt.tree_build_limits(TOP, info.n_boxes)[1], abi.TL_STACK_CAP, info.blas_stack, dev)
    sc.close()


# ---- one-level form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
@pytest.mark.parametrize("extra", [65, 257])
def test_one_level_trees_equal_the_reference(rt, layout, monkeypatch, topology, extra):
    """Two meshes, three instances under rotations and non-uniform scales. The one-level form hands a scene of fewer than 4 096
    flattened triangles to the host's builder, so the totals are 4 096 + 65 and 4 096 + 257, the smallest odd sizes the device takes."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    big, small = grid_mesh(1, 2000), grid_mesh(2, 96 + extra)
    desc = scenes.SceneDesc("one_level_reference", camera_pos=(0.0, 1.0, 6.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    desc.meshes = [big, small]
    desc.instances = [(1, [scenes.scale_rotate_y(0.7, 1.3, 0.6, 0.9, -1.0, 0.2, 0.5), scenes.scale_rotate_y(-1.9, 0.5, 1.4, 1.1, 1.5, -0.4, -0.8)]),
                      (2, [scenes.scale_rotate_y(2.6, 0.8, 1.7, 0.4, 0.3, 0.9, 1.2)])]
    gsc = rt.Scene(0, instancing="flat").load(desc)
    gsc.force_next_op(F)
    push(gsc, desc, [1])
    assert not gsc.two_level() and gsc.as_state()[1] == F
    nodes, tris = gsc.read_bvh()
    stats, hi = gsc.bvh_stats(), gsc.tree_height_info(ONE)
    dev = {"nodes": nodes, "tris": tris, "n_nodes": stats.n_nodes, "max_stack": stats.max_stack, "on_device": hi.on_device == 1, "height": height_fields(hi)}
    records = world_records([corners_of(big), corners_of(big), corners_of(small)], [t for _, ts in desc.instances for t in ts])
    assert len(records) == 4096 + extra == stats.n_triangles and hi.cap == ONE_LEVEL_CAP
    check_one_level(layout, "%d triangles in three instances, %s" % (len(records), topology), records, radius_of(topology), rt.tree_build_limits(ONE, len(records))[1], dev)
    gsc.close()
