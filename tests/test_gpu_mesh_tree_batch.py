"""Batched device build of small mesh trees (sr_scene_set_mesh_tree_batch, SR_BLAS_BATCH; csrc/blas_batch.hip): the pending meshes of
at most SR_BLAS_BATCH_MAX_TRIS triangles that ask for a fast build are built by one launch, a workgroup per mesh. Expected is what
the per-mesh device build and a FRESH scene give: queries against the oracle's brute force, records against a host build of the
same vertices, the tree against its own triangles and against the per-mesh build's tree. Every comparison is bit for bit. Every
scene runs with the batch on, under both topologies of the fast build, unless a test says otherwise."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_refit import Heuristic, records_equal_numpy, state_fields, tree_contains_its_triangles  # noqa: E402
from test_gpu_mesh_tree_build import (SEVEN, SEVEN_BOX, awkward_atrium, device_scene, seven_meshes, tree_info, walk_stack,  # noqa: E402
                                      with_negative_zero)
from test_gpu_mesh_update import mesh_of, push, ray_set, traces_equal_brute_force  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402

U, F = abi.OP_UPDATE, abi.OP_FAST_BUILD
SOMETIMES, RAPIDLY = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING
TOPOLOGIES = ["lbvh", "ploc16"]
MESH = abi.TREE_KIND_MESH
BATCH_BLOCK = 512           # srd::kBlasBatchBlock (csrc/blas_batch.h): threads of the workgroup that builds one mesh
ON_DEVICE = abi.MESH_TREE_ON_DEVICE


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def seven_rays(rt, oracle):
    rays = ray_set(oracle, seven_meshes(), SEVEN_BOX, 21)
    return rays, rt.rays_to_device(rays)


def batch_scene(rt, desc, keys, build_type=SOMETIMES, mode="device", batch="on"):
    return device_scene(rt, desc, keys, build_type, mode).set_mesh_tree_batch(batch)


def batch_fields(gsc):
    i = gsc.mesh_tree_batch_info()
    return (i.batched, i.passed_on, i.launches)


def all_trees(gsc, desc, but=()):
    return {m.key: gsc.read_mesh_tree(m.key) for m in desc.meshes if m.key not in but}


def trees_unchanged(before, after, what):
    for k, tree in before.items():
        for part in ("nodes", "tris", "shade", "shade_tex", "slot_of_prim"):
            assert_bits_equal(np.ascontiguousarray(tree[part]), np.ascontiguousarray(after[k][part]), "%s of mesh %d, %s" % (part, k, what))


# ---- 1. queries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["device", "auto"])
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_batched_meshes_trace_like_a_fresh_scene(rt, oracle, monkeypatch, seven_rays, topology, mode):
    """Ten consecutive deformations of seven SometimesChanges meshes of 1, 2, 3, 63, 64, 65 and 960 triangles: eight refits, the
    ninth step builds all seven trees in one batched launch, the tenth refits the batched trees (their level ranges came back
    right). After each, TraceRay (closest and existence) and closest_hit equal the oracle's brute force and every mesh's state is
    the pure heuristic's. Mode auto with the batch on takes the same path: the opt-in qualifies the small meshes for the device."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    desc = seven_meshes()
    gsc = batch_scene(rt, desc, SEVEN, mode=mode)
    assert gsc.mesh_tree_batch_info().mode == abi.BLAS_BATCH_ON and gsc.mesh_tree_batch_info().max_tris == abi.BLAS_BATCH_MAX_TRIS
    want = {k: Heuristic(SOMETIMES) for k in SEVEN}
    ops = []
    for step in range(1, 11):
        desc = scenes.deform(desc, SEVEN, float(step))
        push(gsc, desc, SEVEN)
        info = gsc.mesh_update_info()
        op = want[1].next_op(True)
        ops.append(op)
        print("%s %s step %d: op %d refitted %d rebuilt %d, mesh trees %s, batch %s" % (topology, mode, step, op, info.blas_refitted, info.blas_rebuilt,
                                                                                       tree_info(gsc), batch_fields(gsc)))
        assert info.dirty_meshes == len(SEVEN) and gsc.two_level()
        if op == U:
            assert (info.blas_refitted, info.blas_rebuilt) == (len(SEVEN), 0) and tree_info(gsc) == (0, 0, ON_DEVICE) and batch_fields(gsc) == (0, 0, 0)
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (0, len(SEVEN)) and tree_info(gsc) == (len(SEVEN), 0, ON_DEVICE)
            assert batch_fields(gsc) == (7, 0, 1)
            assert info.blas_build_ms == 0.0                            # the host built nothing
        for k in SEVEN:
            want[k].done(op)
            bt, st, last = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), last) == (SOMETIMES, want[k].fields(), op), (k, step)
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s %s step %d op %d" % (topology, mode, step, op))
    assert ops == [U] * 8 + [F, U]
    gsc.close()


# ---- 2. records ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_batched_records_are_the_bytes_of_a_host_build(rt, monkeypatch, topology):
    """The awkward atrium (coincident triangles, a zero-area triangle, a -0.0 coordinate, alternating tangent handedness; one mesh
    textured, one plain) after a forced fast build through the batch: every primitive's records at slot_of_prim[p] are the bytes
    of numpy's and of a fresh scene's host build, slot_of_prim is a permutation, top-level boxes and instance records equal the
    fresh scene's."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    base, keys = awkward_atrium()
    gsc = batch_scene(rt, base, keys)
    desc = scenes.deform(base, keys, 1.0, amplitude=0.06)
    for k in keys:
        desc = with_negative_zero(desc, k)
    gsc.force_next_op(F)
    push(gsc, desc, keys)
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (0, 2) and tree_info(gsc) == (2, 0, ON_DEVICE)
    assert batch_fields(gsc) == (2, 0, 1)
    fresh = rt.Scene(0, instancing="two_level").load(desc)
    for k in keys + [m.key for m in desc.meshes if m.key not in keys][:2]:
        tree = records_equal_numpy(gsc, desc, k, "%s mesh %d after a batched build" % (topology, k))      # asserts the permutation too
        want = fresh.read_mesh_tree(k)
        for part in ("tris", "shade", "shade_tex"):
            assert_bits_equal(want[part][want["slot_of_prim"]], tree[part][tree["slot_of_prim"]], "%s of mesh %d by primitive (%s)" % (part, k, topology))
        if k in keys:
            tree_contains_its_triangles(rt, tree, "%s mesh %d" % (topology, k))
    _, _, recs, boxes = gsc.read_top_level()
    _, _, recs2, boxes2 = fresh.read_top_level()
    fresh.close()
    assert_bits_equal(boxes2, boxes, "top-level boxes after a batched build (%s)" % topology)
    for field in ("w2o", "o2w", "pad_a", "pad_b", "tri_offset", "mesh_slot", "flags"):
        assert_bits_equal(np.ascontiguousarray(recs2[field]), np.ascontiguousarray(recs[field]), "instance records: %s (%s)" % (field, topology))
    gsc.close()


# ---- 3. structure and neighbours -----------------------------------------------------------------------------------------------
def stretched(desc, k, step):
    desc = scenes.deform(desc, [k], float(step), amplitude=0.3)
    if k == 7:                                          # far outside the old boxes, and strongly stretched
        v = mesh_of(desc, 7).vertices.copy()
        v["position"] = v["position"] * np.array([6.0, 0.3, 2.0], dtype=np.float32) + np.array([40.0, -7.0, 3.0], dtype=np.float32)
        desc = scenes.with_mesh_vertices(desc, 7, v)
    return desc


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_batched_tree_holds_its_triangles_and_leaves_its_neighbours_alone(rt, monkeypatch, topology):
    """Each of the seven meshes built alone through the batch: the tree contains its triangles, the reported stack need is at most
    26 and at least what a walk of the decoded tree needs, there are fewer nodes than triangles, and read_mesh_tree of every OTHER
    mesh (nodes, records, slot_of_prim: the neighbouring ranges of every resident array) is bit-identical before and after."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = seven_meshes()
    gsc = batch_scene(rt, desc, SEVEN, RAPIDLY)
    for step, k in enumerate(SEVEN, 1):
        desc = stretched(desc, k, step)
        before = all_trees(gsc, desc, but=(k,))
        gsc.force_next_op(F)
        push(gsc, desc, [k])
        assert tree_info(gsc) == (1, 0, ON_DEVICE) and batch_fields(gsc) == (1, 0, 1) and gsc.mesh_as_state(k)[2] == F
        trees_unchanged(before, all_trees(gsc, desc, but=(k,)), "%s, after mesh %d was built" % (topology, k))
        info = gsc.mesh_tree_info()
        tree = records_equal_numpy(gsc, desc, k, "%s mesh %d" % (topology, k))
        n_nodes = tree_contains_its_triangles(rt, tree, "%s mesh %d" % (topology, k))
        need = walk_stack(rt, tree["nodes"])
        print("%s mesh %d: %d triangles, %d nodes, stack %d (a walk needs %d)" % (topology, k, len(tree["tris"]), n_nodes, info.max_stack, need))
        assert n_nodes == info.n_nodes and need <= info.max_stack <= abi.MESH_TREE_STACK_CAP
        assert n_nodes < max(len(tree["tris"]), 2)
    gsc.close()


# ---- 4. same tree as the per-mesh build ----------------------------------------------------------------------------------------
def prim_set_family(rt, tree):
    """The set of primitive-id sets below the nodes and leaves of the decoded tree: the topology without the node numbering."""
    nodes, prim = tree["nodes"], tree["tris"].view(np.uint32)[:, 9]
    family = set()

    def below(i, depth):
        assert depth < 64
        _, _, child = rt.decode_node(nodes[i])
        mine = []
        for ref in child:
            ref = int(ref)
            if ref >= 0:
                mine += below(ref, depth + 1)
            else:
                val = (~ref) & 0xFFFFFFFF
                leaf = [int(p) for p in prim[val >> 3:(val >> 3) + (val & 7)]]
                if leaf:
                    family.add(frozenset(leaf))
                mine += leaf
        family.add(frozenset(mine))
        return mine
    assert sorted(below(0, 0)) == list(range(len(prim)))
    return family


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_batched_tree_is_the_per_mesh_tree(rt, monkeypatch, topology):
    """Two scenes hold the same vertices, one builds each mesh through the batch, the other per mesh with the batch off. Every stage
    is a deterministic function of the sorted order (the library is compiled without FMA contraction, both paths call the same
    per-element functions), only node numbers come from atomic counters: for every mesh the family of primitive-id sets below the
    nodes is equal, and with it node count, stack need and, through the top level, the root box bits."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = seven_meshes()
    a, b = batch_scene(rt, desc, SEVEN, RAPIDLY), batch_scene(rt, desc, SEVEN, RAPIDLY, batch="off")
    for step, k in enumerate(SEVEN, 1):
        desc = stretched(desc, k, step)
        for gsc in (a, b):
            gsc.force_next_op(F)
            push(gsc, desc, [k])
            assert tree_info(gsc) == (1, 0, ON_DEVICE)
        assert batch_fields(a) == (1, 0, 1) and batch_fields(b) == (0, 0, 0)
        ia, ib = a.mesh_tree_info(), b.mesh_tree_info()
        ta, tb = a.read_mesh_tree(k), b.read_mesh_tree(k)
        fa, fb = prim_set_family(rt, ta), prim_set_family(rt, tb)
        print("%s mesh %d: %d nodes, stack %d, %d sets (batched); %d nodes, stack %d, %d sets (per mesh)" % (topology, k, ia.n_nodes, ia.max_stack, len(fa),
                                                                                                       ib.n_nodes, ib.max_stack, len(fb)))
        assert fa == fb, "%s mesh %d: %d sets differ" % (topology, k, len(fa ^ fb))
        assert (ia.n_nodes, ia.max_stack) == (ib.n_nodes, ib.max_stack) and len(ta["nodes"]) == len(tb["nodes"])
    _, _, _, boxes_a = a.read_top_level()
    _, _, _, boxes_b = b.read_top_level()
    assert_bits_equal(boxes_b, boxes_a, "top-level boxes, batched against per mesh (%s)" % topology)
    a.close(); b.close()


# ---- 5. size edges ---------------------------------------------------------------------------------------------------------
def grid_mesh(key, n_tris, colour=(0.4, 0.7, 0.5, 1.0)):
    """A gently waved grid of exactly n_tris triangles, about 2 x 1 units."""
    cols = 64 if n_tris > 1024 else 32
    rows = max(-(-n_tris // (2 * cols)), 1)
    x, y = np.meshgrid(np.arange(cols + 1, dtype=np.float64), np.arange(rows + 1, dtype=np.float64))
    pos = np.stack([2.0 * x / cols - 1.0, 0.2 * np.sin(5.0 * x / cols) * np.cos(4.0 * y / cols), 2.0 * y / cols - 0.5], axis=-1).reshape(-1, 3).astype(np.float32)
    a = (np.arange(rows)[:, None] * (cols + 1) + np.arange(cols)[None, :]).reshape(-1)
    quads = np.stack([a, a + 1, a + cols + 2, a, a + cols + 2, a + cols + 1], axis=-1).reshape(-1).astype(np.uint32)
    v = scenes.make_vertices(pos, np.tile(np.array((0, 1, 0), dtype=np.float32), (len(pos), 1)))
    return scenes.MeshDesc(key, v, np.ascontiguousarray(quads[:3 * n_tris]), abi.material(base_color=colour, roughness=0.5))


def repeated_triangle_mesh(key, n_tris, zero_area):
    """n_tris copies of one triangle (all Morton keys equal, all PLOC distances equal), or of one zero-area triangle."""
    tri = [(-0.5, 0.0, 0.0), (0.5, 0.0, 0.2), (0.5, 0.0, 0.2) if zero_area else (0.0, 1.0, 0.0)]
    v = scenes.make_vertices(np.array(tri, dtype=np.float32), np.tile(np.array((0, 0, 1), dtype=np.float32), (3, 1)))
    return scenes.MeshDesc(key, v, np.tile(np.array([0, 1, 2], dtype=np.uint32), n_tris), abi.material(base_color=(0.8, 0.6, 0.2, 1.0), roughness=0.5))


def floor_and(meshes, name):
    """A static floor quad (key 100) under the given meshes, spread over the box of SEVEN_BOX."""
    s = scenes.SceneDesc(name, camera_pos=(0.0, 1.0, 6.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    qv, qi = scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(100, qv, qi, abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)))
    s.instances = [(100, [scenes.translate(0.0, -1.3, 0.0, 3.0)])]
    for i, m in enumerate(meshes):
        s.meshes.append(m)
        s.instances.append((m.key, [scenes.translate(-1.8 + 1.8 * (i % 3), -0.8 + 0.8 * (i // 3), 1.5 - 1.2 * (i // 3))]))
    return s


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_sizes_around_the_block_and_the_cap(rt, oracle, monkeypatch, topology):
    """Grids of block - 1, block, block + 1, 2 * block + 1, cap - 1, cap and cap + 1 triangles pushed in one call: the batch builds
    all but the last, which the per-mesh build takes in the same call; the queries equal the oracle's brute force."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    probe = rt.Scene(0, instancing="two_level")
    cap = probe.mesh_tree_batch_info().max_tris
    probe.close()
    assert cap == abi.BLAS_BATCH_MAX_TRIS and BATCH_BLOCK * 8 == cap
    sizes = [BATCH_BLOCK - 1, BATCH_BLOCK, BATCH_BLOCK + 1, 2 * BATCH_BLOCK + 1, cap - 1, cap, cap + 1]
    keys = list(range(1, len(sizes) + 1))
    desc = floor_and([grid_mesh(k, n) for k, n in zip(keys, sizes)], "size_edges")
    rays = ray_set(oracle, desc, SEVEN_BOX, 23)[::4]
    rays = np.ascontiguousarray(rays)
    rd = rt.rays_to_device(rays)
    gsc = batch_scene(rt, desc, keys)
    desc = scenes.deform(desc, keys, 1.0, amplitude=0.05)
    gsc.force_next_op(F)
    push(gsc, desc, keys)
    print("%s sizes %s: mesh trees %s, batch %s" % (topology, sizes, tree_info(gsc), batch_fields(gsc)))
    assert tree_info(gsc) == (len(sizes), 0, ON_DEVICE) and batch_fields(gsc) == (len(sizes) - 1, 0, 1)
    for k in keys:
        tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, k, "%s grid %d" % (topology, k)), "%s grid %d" % (topology, k))
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s size edges" % topology)
    desc = scenes.deform(desc, keys, 2.0, amplitude=0.05)               # ... and the trees refit: their level ranges are right
    gsc.force_next_op(U)
    push(gsc, desc, keys)
    assert gsc.mesh_update_info().blas_refitted == len(keys)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s size edges, refitted" % topology)
    gsc.close()


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_degenerate_meshes_are_built_or_passed_on(rt, oracle, monkeypatch, seven_rays, topology):
    """300 copies of one triangle and 300 zero-area triangles next to the seven (static) meshes: the batch either builds the mesh
    within the budget or hands it to the per-mesh build (which may refuse it to the host); either way the queries equal the
    oracle's and no other mesh's tree changed."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    base = seven_meshes()
    extra = [repeated_triangle_mesh(31, 300, False), repeated_triangle_mesh(32, 300, True)]
    desc = dataclasses.replace(base, meshes=list(base.meshes) + extra,
                               instances=list(base.instances) + [(31, [scenes.translate(0.0, 0.3, 1.0)]), (32, [scenes.translate(1.0, 0.5, 0.5)])])
    for k in (31, 32):
        gsc = batch_scene(rt, desc, [k])
        before = all_trees(gsc, desc, but=(k,))
        v = mesh_of(desc, k).vertices.copy()
        v["position"] += np.float32(0.125)
        after = scenes.with_mesh_vertices(desc, k, v)
        gsc.force_next_op(F)
        push(gsc, after, [k])
        b = gsc.mesh_tree_batch_info()
        print("%s mesh %d: mesh trees %s, batch %s" % (topology, k, tree_info(gsc), batch_fields(gsc)))
        assert b.batched + b.passed_on == 1 and b.launches == 1
        assert tree_info(gsc)[:2] in ((1, 0), (0, 1)) and (b.batched == 0 or tree_info(gsc) == (1, 0, ON_DEVICE))
        trees_unchanged(before, all_trees(gsc, after, but=(k,)), "%s, after degenerate mesh %d" % (topology, k))
        records_equal_numpy(gsc, after, k, "%s degenerate mesh %d" % (topology, k))
        traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "%s degenerate mesh %d" % (topology, k))
        gsc.close()


# ---- 6. too tall -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_a_too_tall_tree_is_passed_on_and_rebalanced(rt, oracle, monkeypatch, seven_rays, topology):
    """Under REBALANCE with a cap one below the 960-triangle sphere's binary height (read with the bound off; at least the median
    tree's 9, so the per-mesh build can reach it): the batch hands the sphere back before it has written anything resident, builds
    the other six, and the per-mesh build rebalances the sphere within the same call. Under REFUSE no cap can be set and a tree of
    at most 4096 triangles taller than 26 is not known to exist (the degenerate meshes above come close where they are passed on):
    that the batch then leaves the refusal, the remembering and the all-or-nothing hand-over to the per-mesh loop follows from
    build_mesh_trees_device, where a mesh that is handed back is appended to the very list that loop walks."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    base = seven_meshes()
    desc = scenes.deform(base, SEVEN, 1.0)
    gsc = batch_scene(rt, base, SEVEN)
    gsc.force_next_op(F)
    push(gsc, desc, [7])
    height = gsc.tree_height_info(MESH).height_before
    assert batch_fields(gsc) == (1, 0, 1) and gsc.tree_height_info(MESH).on_device == 1
    gsc.close()
    cap = height - 1
    print("%s: the sphere's binary height is %d, cap %d" % (topology, height, cap))
    assert 9 <= cap < height                                            # median_height(960) == 9 <= cap
    gsc = batch_scene(rt, base, SEVEN).set_tree_height_bound("rebalance", cap)
    gsc.force_next_op(F)
    push(gsc, desc, SEVEN)
    hi = gsc.tree_height_info(MESH)
    print("%s: mesh trees %s, batch %s, height %d -> %d, %d subtrees rebuilt" % (topology, tree_info(gsc), batch_fields(gsc), hi.height_before, hi.height_after,
                                                                            hi.subtrees_rebuilt))
    assert tree_info(gsc) == (7, 0, ON_DEVICE) and batch_fields(gsc) == (6, 1, 1)
    assert (hi.on_device, hi.cap, hi.height_before) == (1, cap, height) and hi.height_after <= cap and hi.subtrees_rebuilt >= 1
    assert gsc.mesh_tree_info().max_stack <= cap
    for k in SEVEN:
        tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, k, "%s mesh %d under cap %d" % (topology, k, cap)), "%s mesh %d" % (topology, k))
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s, sphere passed on and rebalanced" % topology)
    gsc.close()


# ---- 7. mixed call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_a_refit_a_batch_and_a_per_mesh_build_share_one_call(rt, oracle, monkeypatch, topology):
    """Mesh 7 at its third update (refit), meshes 1, 3, 4, 5 and 6 at their ninth (batch) and a grid above the cap at its ninth (per
    mesh) in one set_instances: the host builds nothing, the arrays stay resident (the step after refits all), the queries equal
    the oracle's."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    base = seven_meshes()
    big = grid_mesh(50, abi.BLAS_BATCH_MAX_TRIS + 1)
    desc = dataclasses.replace(base, meshes=list(base.meshes) + [big], instances=list(base.instances) + [(50, [scenes.translate(0.5, 1.2, -1.5)])])
    small = [1, 3, 4, 5, 6]
    gsc = batch_scene(rt, desc, small + [50, 7])
    rays = np.ascontiguousarray(ray_set(oracle, desc, SEVEN_BOX, 25)[::2])
    rd = rt.rays_to_device(rays)
    for step in range(1, 11):
        keys = small + [50] if step <= 6 else small + [50, 7]
        desc = scenes.deform(desc, keys, float(step), amplitude=0.05)
        push(gsc, desc, keys)
        info = gsc.mesh_update_info()
        if step == 9:
            assert (info.blas_refitted, info.blas_rebuilt) == (1, 6) and tree_info(gsc) == (6, 0, ON_DEVICE) and batch_fields(gsc) == (5, 0, 1)
            assert [gsc.mesh_as_state(k)[2] for k in small + [50, 7]] == [F] * 6 + [U] and info.blas_build_ms == 0.0
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (len(keys), 0) and batch_fields(gsc) == (0, 0, 0), step
        if step >= 8:
            traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s mixed call, step %d" % (topology, step))
    gsc.close()


# ---- 8. HBM ----------------------------------------------------------------------------------------------------------------
def test_batched_build_cycles_do_not_grow_hbm(rt):
    """Thirty batched builds of the seven meshes: free device memory after the thirtieth is where it was after the third (node
    ranges are kept, rows, result rows and scratch are reused), measured as test_device_build_cycles_do_not_grow_hbm measures it:
    first against last and the spread of the window both under 1 MiB, the driver's own allocation granule."""
    import torch
    desc = seven_meshes()
    sc = batch_scene(rt, desc, SEVEN, RAPIDLY)
    free = []
    for cycle in range(30):
        desc = scenes.deform(desc, SEVEN, float(cycle), amplitude=0.05)
        sc.force_next_op(F)
        push(sc, desc, SEVEN)
        assert tree_info(sc) == (7, 0, ON_DEVICE) and batch_fields(sc) == (7, 0, 1)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    window = free[2:]
    print("free memory over the window: first %d, last %d, spread %d bytes" % (window[0], window[-1], max(window) - min(window)))
    assert abs(window[-1] - window[0]) < (1 << 20) and max(window) - min(window) < (1 << 20), free
    sc.close()


# ---- 9. Renderer and environment ---------------------------------------------------------------------------------------------
def test_renderer_frames_across_a_batched_build(rt, oracle, monkeypatch):
    """Renderer.set_mesh_tree_batch("on") with set_mesh_tree_build("device"): eleven frames of the blob-and-lamp scene, blob 1 and
    lamp 5 deformed before every frame but the first (eight refits, the batched build at the ninth, a refit of the batched trees);
    output and raw_color of every frame equal the oracle's loop. Mode 2 is refused."""
    from test_gpu_multi_renderer import grab, load
    from sunray_amd._lib import check, lib
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.instanced_field(24)
    W, H = 64, 48
    r = rt.Renderer((W, H))
    with pytest.raises(rt.SunrayError) as e:
        check(lib().sr_renderer_set_mesh_tree_batch(r._h, C.c_uint32(2)))
    assert e.value.code == -1 and "sr_renderer_set_mesh_tree_batch: mode must be" in e.value.description
    load(r, desc)
    r.set_mesh_tree_build("device")
    r.set_mesh_tree_batch("on")
    for k in (1, 5):
        r.set_mesh_build_type(k, RAPIDLY)
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    got, descs, d = [], [], desc
    for f in range(11):
        if f:
            d = scenes.deform(d, [1, 5], float(f))
            for k in (1, 5):
                r.update_mesh(k, mesh_of(d, k).vertices)
        r.wait_frame(r.render(cam, d.instances))
        got.append(grab(rt, hip, r))
        descs.append(d)
        view = r.replica_scene(0)
        info, ti = view.mesh_update_info(), view.mesh_tree_info()
        assert view.two_level() and view.mesh_tree_batch_info().mode == abi.BLAS_BATCH_ON
        if f:
            assert (info.blas_refitted, info.blas_rebuilt, ti.built_on_device, ti.built_on_host) == ((0, 2, 2, 0) if f == 9 else (2, 0, 0, 0)), f
            assert batch_fields(view) == ((2, 0, 1) if f == 9 else (0, 0, 0)), f
    r.close()
    multi = rt.Renderer((W, H), devices=[0, 0])                         # every device slot's scene takes the setting
    load(multi, desc)
    multi.set_mesh_tree_batch("on")
    assert [multi.replica_scene(i).mesh_tree_batch_info().mode for i in range(2)] == [abi.BLAS_BATCH_ON] * 2
    multi.set_mesh_tree_batch("off")
    assert [multi.replica_scene(i).mesh_tree_batch_info().mode for i in range(2)] == [abi.BLAS_BATCH_OFF] * 2
    multi.close()
    of, prev = oracle.HostFrame(W, H, rt.default_noise_texture()), None
    for f, d in enumerate(descs):
        osc = oracle.OracleScene().load(d)
        om = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        prev = list(om.view_proj)
        osc.trace_ris(of, om, f); osc.trace_final(of, om, f); oracle.post_chain(of, f)
        osc.close()
        assert_bits_equal(of.output, got[f][0], "output of frame %d" % f)
        assert_bits_equal(of.raw_color, got[f][1], "raw_color of frame %d" % f)


def test_the_environment_sets_the_initial_mode(rt, monkeypatch):
    for value, mode in (("on", abi.BLAS_BATCH_ON), ("off", abi.BLAS_BATCH_OFF), ("On", abi.BLAS_BATCH_OFF), ("", abi.BLAS_BATCH_OFF), ("1", abi.BLAS_BATCH_OFF)):
        monkeypatch.setenv("SR_BLAS_BATCH", value)      # read when the scene is created; anything unknown means off
        gsc = rt.Scene(0, instancing="two_level")
        assert gsc.mesh_tree_batch_info().mode == mode, value
        gsc.close()
    monkeypatch.delenv("SR_BLAS_BATCH")
    gsc = rt.Scene(0, instancing="two_level")
    assert gsc.mesh_tree_batch_info().mode == abi.BLAS_BATCH_OFF
    assert gsc.set_mesh_tree_batch("on").mesh_tree_batch_info().mode == abi.BLAS_BATCH_ON
    gsc.close()
    monkeypatch.setenv("SR_BLAS_BATCH", "on")
    gsc = rt.Scene(0, instancing="two_level")
    assert gsc.set_mesh_tree_batch("off").mesh_tree_batch_info().mode == abi.BLAS_BATCH_OFF      # the call overrides the environment's choice
    gsc.close()
