"""The height bound of the device fast builds (sr_scene_set_tree_height_bound, SR_FAST_BUILD_HEIGHT; csrc/bvh_gpu.hip "Height
bound"): under SR_HEIGHT_BOUND_REBALANCE a binary tree taller than its stack cap is rebalanced on the device to fit instead of
being refused to the host. Mesh trees of the two-level form, the top level and the one-level form; both topologies of the fast
build where it matters. Every comparison of query results is bit for bit against the oracle's brute force."""
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
from test_gpu_mesh_tree_build import SEVEN, SEVEN_BOX, chain_mesh, device_scene, seven_meshes, tree_info  # noqa: E402
from test_gpu_mesh_update import mesh_of, push, ray_set, traces_equal_brute_force, with_vertices  # noqa: E402
from test_gpu_top_level_build import LEAF_MAX, affine_transforms, check_structure, small_mesh_scene  # noqa: E402

U, F = abi.OP_UPDATE, abi.OP_FAST_BUILD
SOMETIMES, RAPIDLY = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING
TOPOLOGIES = ["lbvh", "ploc16"]
ONE, TOP, MESH = abi.TREE_KIND_ONE_LEVEL, abi.TREE_KIND_TOP_LEVEL, abi.TREE_KIND_MESH
CAP = abi.MESH_TREE_STACK_CAP


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def seven_rays(rt, oracle):
    rays = ray_set(oracle, seven_meshes(), SEVEN_BOX, 11)
    return rays, rt.rays_to_device(rays)


def median_height(k):
    """H(k): the walk height of a median-split tree over k primitives."""
    h = 0
    while k > LEAF_MAX:
        k, h = (k + 1) // 2, h + 1
    return h


def height_fields(i):
    return "cap %d: height %d -> %d, %d subtrees / %d primitives rebuilt, on_device %d" % (i.cap, i.height_before, i.height_after, i.subtrees_rebuilt,
                                                                                         i.prims_rebuilt, i.on_device)


def chain_scene():
    """seven_meshes plus the 63-triangle chain as mesh 9 -> (description, the same with mesh 7 deformed and the chain's normals changed)"""
    base = seven_meshes()
    chain = chain_mesh(9)
    desc = dataclasses.replace(base, meshes=list(base.meshes) + [chain], instances=list(base.instances) + [(9, [scenes.translate(0.0, 0.0, 0.0, 2.0)])])
    moved_chain = chain.vertices.copy()
    moved_chain["normal"] = np.array((0, 1, 0), dtype=np.float32)
    return desc, with_vertices(scenes.deform(desc, [7], 1.0), 9, moved_chain)


def test_median_height_is_the_issues():
    assert (median_height(63), median_height(64), median_height(65), median_height(960)) == (5, 5, 6, 9)


# ---- 1. the refused chain ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_the_refused_chain_is_built_on_the_device(rt, oracle, monkeypatch, seven_rays, topology):
    """The scene of test_fallbacks_name_their_reason_and_equal_the_oracle's last case: the radix tree of the chain is some 60 levels
    tall. Under REBALANCE both meshes are built on the device, within 26 entries; under REFUSE the radix tree still goes to the host."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    desc, after = chain_scene()
    gsc = device_scene(rt, desc, [7, 9]).set_tree_height_bound("rebalance")
    gsc.force_next_op(F)
    push(gsc, after, [7, 9])
    hi, ti = gsc.tree_height_info(MESH), gsc.mesh_tree_info()
    print("%s, chain under rebalance: mesh trees %s, %s, stack %d" % (topology, tree_info(gsc), height_fields(hi), ti.max_stack))
    assert tree_info(gsc) == (2, 0, abi.MESH_TREE_ON_DEVICE)
    assert (hi.mode, hi.mesh_tree_cap, hi.on_device, hi.cap) == (abi.HEIGHT_BOUND_REBALANCE, 0, 1, CAP)
    if topology == "lbvh":
        assert hi.height_before > CAP and hi.height_after <= CAP and hi.subtrees_rebuilt >= 1 and 2 <= hi.prims_rebuilt <= 63
    assert hi.height_after <= CAP and ti.max_stack <= CAP and gsc.bvh_stats().max_stack <= abi.TL_STACK_CAP
    tree = records_equal_numpy(gsc, after, 9, "%s chain after a rebalanced build" % topology)
    tree_contains_its_triangles(rt, tree, "%s chain" % topology)
    assert np.array_equal(np.sort(tree["slot_of_prim"]), np.arange(63))
    traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "%s chain, rebalanced" % topology)
    gsc.close()
    gsc = device_scene(rt, desc, [7, 9])
    assert gsc.tree_height_info(MESH).mode == abi.HEIGHT_BOUND_REFUSE
    gsc.force_next_op(F)
    push(gsc, after, [7, 9])
    if topology == "lbvh":
        assert tree_info(gsc) == (0, 2, abi.MESH_TREE_HOST_STACK_BUDGET)
        hi = gsc.tree_height_info(MESH)
        assert hi.on_device == 0 and hi.height_before > CAP and hi.subtrees_rebuilt == 0
    gsc.close()


def test_the_environment_sets_the_initial_mode(rt, monkeypatch):
    for value, mode in (("rebalance", abi.HEIGHT_BOUND_REBALANCE), ("refuse", abi.HEIGHT_BOUND_REFUSE), ("Rebalance", abi.HEIGHT_BOUND_REFUSE),
                        ("", abi.HEIGHT_BOUND_REFUSE), ("1", abi.HEIGHT_BOUND_REFUSE)):
        monkeypatch.setenv("SR_FAST_BUILD_HEIGHT", value)
        sc = rt.Scene(0)
        for kind in (ONE, TOP, MESH):
            i = sc.tree_height_info(kind)
            assert (i.mode, i.mesh_tree_cap, i.on_device, i.subtrees_rebuilt) == (mode, 0, 0, 0), (value, kind)
        sc.close()
    monkeypatch.delenv("SR_FAST_BUILD_HEIGHT")
    sc = rt.Scene(0)
    assert sc.tree_height_info(MESH).mode == abi.HEIGHT_BOUND_REFUSE
    i = sc.set_tree_height_bound("rebalance", 12).tree_height_info(MESH)
    assert (i.mode, i.mesh_tree_cap) == (abi.HEIGHT_BOUND_REBALANCE, 12)
    with pytest.raises(rt.SunrayError) as e:
        sc.set_tree_height_bound("refuse", 12)
    assert e.value.code == -1 and "sr_scene_set_tree_height_bound" in e.value.description
    assert sc.tree_height_info(MESH).mesh_tree_cap == 12                # a refused call changes nothing
    bounded = sc.mesh_tree_info().auto_threshold                        # under REBALANCE: the measured threshold, a power of two, or never
    assert bounded == 0xFFFFFFFF or (bounded >= 2 and bounded & (bounded - 1) == 0)
    assert sc.set_tree_height_bound("refuse").mesh_tree_info().auto_threshold == 0xFFFFFFFF      # nothing changes under REFUSE
    sc.close()


# ---- 2. caps on a small sphere -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_caps_on_a_small_sphere(rt, oracle, monkeypatch, seven_rays, topology):
    """Mesh 7 (960 triangles, H = 9) held to 9 (the median tree itself), 10 and 12 entries; 8 is refused, and the refusal is
    forgotten when the cap changes."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    assert median_height(960) == 9
    rays, rd = seven_rays
    base = seven_meshes()
    for step, cap in enumerate((9, 10, 12), 1):
        gsc = device_scene(rt, base, [7]).set_tree_height_bound("rebalance", cap)
        desc = scenes.deform(base, [7], float(step))
        gsc.force_next_op(F)
        push(gsc, desc, [7])
        hi, ti = gsc.tree_height_info(MESH), gsc.mesh_tree_info()
        print("%s, 960 triangles: %s, %d nodes, stack %d" % (topology, height_fields(hi), ti.n_nodes, ti.max_stack))
        assert tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE) and (hi.on_device, hi.cap, hi.mesh_tree_cap) == (1, cap, cap)
        assert 9 <= hi.height_after <= cap and ti.max_stack <= cap and hi.height_before >= hi.height_after
        assert (hi.subtrees_rebuilt == 0) == (hi.height_before <= cap) and hi.prims_rebuilt <= 960
        tree = records_equal_numpy(gsc, desc, 7, "%s cap %d" % (topology, cap))
        assert tree_contains_its_triangles(rt, tree, "%s cap %d" % (topology, cap)) == ti.n_nodes
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s cap %d" % (topology, cap))
        gsc.close()
    gsc = device_scene(rt, base, [7]).set_tree_height_bound("rebalance", 8)
    desc = scenes.deform(base, [7], 1.0)
    gsc.force_next_op(F)
    push(gsc, desc, [7])
    assert tree_info(gsc) == (0, 1, abi.MESH_TREE_HOST_STACK_BUDGET) and gsc.tree_height_info(MESH).on_device == 0
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s cap 8: refused" % topology)
    gsc.set_tree_height_bound("rebalance", 10)
    desc = scenes.deform(base, [7], 2.0)
    gsc.force_next_op(F)
    push(gsc, desc, [7])
    hi = gsc.tree_height_info(MESH)
    assert tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE) and hi.on_device == 1 and hi.height_after <= 10, height_fields(hi)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s cap 10 after the refusal under cap 8" % topology)
    gsc.close()


# ---- 3. sizes around a wave and the leaf -------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_sizes_around_a_wave_and_the_leaf(rt, oracle, monkeypatch, seven_rays, topology):
    """The meshes of 1, 2, 3, 63, 64 and 65 triangles under cap 6 = H(65): every one on the device; under cap 5 the 65-triangle
    mesh cannot fit and the call goes to the host. (The 960-triangle mesh has H = 9: no tree over it fits 6 entries, so it is not
    updatable here; test_all_seven_under_cap_9 builds all seven in one call under the smallest cap that admits it.)"""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    base = seven_meshes()
    assert median_height(65) == 6 and median_height(64) == 5
    for cap, want in ((6, (6, 0, abi.MESH_TREE_ON_DEVICE)), (5, (0, 6, abi.MESH_TREE_HOST_STACK_BUDGET))):
        keys = SEVEN[:6]                                # 1, 2, 3, 63, 64 and 65 triangles
        gsc = device_scene(rt, base, keys).set_tree_height_bound("rebalance", cap)
        desc = scenes.deform(base, keys, 1.0)
        gsc.force_next_op(F)
        push(gsc, desc, keys)
        print("%s cap %d: mesh trees %s, last build %s" % (topology, cap, tree_info(gsc), height_fields(gsc.tree_height_info(MESH))))
        assert tree_info(gsc) == want
        for k in keys:
            tree = records_equal_numpy(gsc, desc, k, "%s cap %d mesh %d" % (topology, cap, k))
            tree_contains_its_triangles(rt, tree, "%s cap %d mesh %d" % (topology, cap, k))
        if cap == 6:
            assert gsc.mesh_tree_info().max_stack <= 6 and gsc.tree_height_info(MESH).height_after <= 6
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s cap %d" % (topology, cap))
        gsc.close()


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_all_seven_under_cap_9(rt, oracle, monkeypatch, seven_rays, topology):
    """All seven meshes updatable under the smallest cap the largest admits (H(960) = 9): seven device builds in one call."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    rays, rd = seven_rays
    base = seven_meshes()
    gsc = device_scene(rt, base, SEVEN).set_tree_height_bound("rebalance", 9)
    desc = scenes.deform(base, SEVEN, 1.0)
    gsc.force_next_op(F)
    push(gsc, desc, SEVEN)
    assert tree_info(gsc) == (7, 0, abi.MESH_TREE_ON_DEVICE) and gsc.mesh_tree_info().max_stack <= 9
    for k in SEVEN:
        tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, k, "%s mesh %d" % (topology, k)), "%s mesh %d" % (topology, k))
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s seven meshes under cap 9" % topology)
    gsc.close()


# ---- 4. coincident primitives under PLOC -------------------------------------------------------------------------------------
def test_coincident_primitives_under_ploc(rt, oracle, monkeypatch, seven_rays):
    """200 copies of one triangle in front of the 64-triangle sphere's triangles: equal boxes merge one pair per PLOC iteration,
    a chain far taller than 26. Built on the device whatever the topology's height was."""
    monkeypatch.setenv("SR_FAST_BUILD", "ploc16")
    rays, rd = seven_rays
    base = seven_meshes()
    sphere = mesh_of(base, 5)
    idx = np.concatenate([np.tile(sphere.indices[:3], 200), sphere.indices]).astype(np.uint32)
    desc = dataclasses.replace(base, meshes=list(base.meshes) + [scenes.MeshDesc(10, sphere.vertices, idx, sphere.material)],
                               instances=list(base.instances) + [(10, [scenes.translate(0.3, 1.4, 1.0)])])
    gsc = device_scene(rt, desc, [10]).set_tree_height_bound("rebalance")
    after = scenes.deform(desc, [10], 1.0)
    gsc.force_next_op(F)
    push(gsc, after, [10])
    hi, ti = gsc.tree_height_info(MESH), gsc.mesh_tree_info()
    print("200 coincident + 64 triangles under ploc16: %s, %d nodes, stack %d" % (height_fields(hi), ti.n_nodes, ti.max_stack))
    assert tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE) and hi.on_device == 1 and hi.height_after <= CAP and ti.max_stack <= CAP
    assert (hi.subtrees_rebuilt == 0) == (hi.height_before <= CAP)
    tree = records_equal_numpy(gsc, after, 10, "coincident primitives")
    assert np.array_equal(np.sort(tree["slot_of_prim"]), np.arange(264))
    tree_contains_its_triangles(rt, tree, "coincident primitives")
    traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "coincident primitives")
    gsc.close()


# ---- 5. a tree that fits -----------------------------------------------------------------------------------------------------
def canonical_nodes(nodes):
    """What two collapses of one binary tree share: the collapse numbers the nodes of a level in the order its threads take them
    from an atomic counter, so indices and references to inner nodes differ from run to run; the quantised boxes of every node
    (dwords 0..11) and the leaf references (slot ranges follow from subtree sizes) do not. -> (sorted box rows, sorted leaf references)"""
    boxes = sorted(row.tobytes() for row in np.ascontiguousarray(nodes[:, :12]))
    refs = nodes[:, 12:].astype(np.uint32).reshape(-1)
    return boxes, np.sort(refs[refs >= 0x80000000]).tobytes(), int((refs < 0x80000000).sum())


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_a_tree_that_fits_is_left_alone(rt, monkeypatch, topology):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    base = seven_meshes()
    desc = scenes.deform(base, SEVEN, 1.0)
    seen = {}
    for mode in ("refuse", "rebalance"):
        gsc = device_scene(rt, base, SEVEN).set_tree_height_bound(mode)
        gsc.force_next_op(F)
        push(gsc, desc, SEVEN)
        hi, ti = gsc.tree_height_info(MESH), gsc.mesh_tree_info()
        assert tree_info(gsc) == (7, 0, abi.MESH_TREE_ON_DEVICE) and hi.on_device == 1 and hi.cap == CAP
        assert hi.subtrees_rebuilt == 0 and hi.prims_rebuilt == 0 and hi.height_before == hi.height_after <= CAP
        seen[mode] = (ti.n_nodes, ti.max_stack, hi.height_before, [canonical_nodes(gsc.read_mesh_tree(k)["nodes"]) for k in SEVEN])
        gsc.close()
    assert seen["refuse"] == seen["rebalance"]


# ---- 6. the heuristic cycle --------------------------------------------------------------------------------------------------
def test_the_heuristic_cycle_over_a_rebalanced_tree(rt, oracle, monkeypatch, seven_rays):
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    rays, rd = seven_rays
    desc, _ = chain_scene()
    gsc = device_scene(rt, desc, [7, 9]).set_tree_height_bound("rebalance")
    want = {k: Heuristic(SOMETIMES) for k in (7, 9)}
    ops = []
    for step in range(1, 11):
        desc = scenes.deform(desc, [7], float(step))
        v = mesh_of(desc, 9).vertices.copy()
        v["position"][:, 0] += np.float32(0.0625)       # the chain moves as a whole: still a chain
        desc = with_vertices(desc, 9, v)
        push(gsc, desc, [7, 9])
        info, hi = gsc.mesh_update_info(), gsc.tree_height_info(MESH)
        op = want[7].next_op(True)
        ops.append(op)
        if op == F:
            print("step %d: %s" % (step, height_fields(hi)))
            assert (info.blas_refitted, info.blas_rebuilt) == (0, 2) and tree_info(gsc) == (2, 0, abi.MESH_TREE_ON_DEVICE)
            assert hi.on_device == 1 and hi.height_before > CAP and hi.height_after <= CAP and hi.subtrees_rebuilt >= 1
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (2, 0) and tree_info(gsc) == (0, 0, abi.MESH_TREE_ON_DEVICE), step
        for k in (7, 9):
            assert want[k].next_op(True) == op
            want[k].done(op)
            bt, st, last = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), last) == (SOMETIMES, want[k].fields(), op), (k, step)
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "step %d op %d" % (step, op))
    assert ops == [U] * 8 + [F, U]
    tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, 9, "chain after the refit of its rebalanced tree"), "chain after the refit")
    gsc.close()


# ---- 7. top level ------------------------------------------------------------------------------------------------------------
def test_top_level_chain_is_built_on_the_device(rt, monkeypatch):
    """The 63 instances in geometric progression of test_a_tree_outside_the_stack_budget_is_left_to_the_host under the radix tree."""
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    monkeypatch.setenv("SR_FAST_BUILD_HEIGHT", "rebalance")
    xf = np.zeros((63, 12), dtype=np.float32)
    xf[:, 0] = xf[:, 5] = xf[:, 10] = 1.0e-9
    for j in range(21):
        for a in range(3):
            xf[3 * j + a, 3 + 4 * a] = 2.0 ** -(j + 1)
    sc = small_mesh_scene(rt, xf, "device")
    info, hi = sc.top_level_info(), sc.tree_height_info(TOP)
    print("63 instances in geometric progression under rebalance: on_device %d reason %d, %s; top level %d + leaf %d + mesh tree %d + 1" %
          (info.on_device, info.reason, height_fields(hi), info.max_stack, LEAF_MAX, info.blas_stack))
    assert info.on_device == 1 and info.reason == abi.TL_ON_DEVICE
    assert hi.on_device == 1 and hi.height_before > hi.cap >= hi.height_after and hi.subtrees_rebuilt >= 1
    assert hi.cap == abi.TL_STACK_CAP - info.blas_stack - LEAF_MAX - 1
    check_structure(rt, sc, "geometric progression, rebalanced")
    assert info.max_stack + LEAF_MAX + info.blas_stack + 1 <= abi.TL_STACK_CAP
    assert sc.tree_height_info(ONE).on_device == 0 and sc.tree_height_info(MESH).on_device == 0
    sc.close()
    sc = small_mesh_scene(rt, affine_transforms(4096, 4196), "device")
    info, hi = sc.top_level_info(), sc.tree_height_info(TOP)
    assert info.on_device == 1 and hi.on_device == 1 and hi.subtrees_rebuilt == 0 and hi.height_before == hi.height_after <= hi.cap, height_fields(hi)
    check_structure(rt, sc, "4 096 random instances with the height bound on")
    sc.close()


# ---- 8. one-level form -------------------------------------------------------------------------------------------------------
def test_one_level_chain_is_built_on_the_device(rt, oracle, monkeypatch):
    """A 4 096-triangle sphere inside the chain's box: the radix tree over the flattened scene keeps the chain's levels, more than
    the 47 entries of the one-level walk, so under REFUSE the fast build is the host's; under REBALANCE the device's."""
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    sv, si = scenes.uv_sphere(0.2, 64, 33)
    assert len(si) == 3 * 4096
    sv = sv.copy()
    sv["position"] += np.float32(0.25)
    desc = scenes.SceneDesc("sphere_in_chain", camera_pos=(0.25, 0.3, 1.4), camera_target=(0.25, 0.25, 0.25), fov_y=35.0)
    desc.meshes.append(scenes.MeshDesc(1, sv, si, abi.material(base_color=(0.9, 0.5, 0.3, 1.0), roughness=0.3)))
    desc.meshes.append(chain_mesh(2))
    desc.instances = [(1, [scenes.translate(0.0, 0.0, 0.0)]), (2, [scenes.translate(0.0, 0.0, 0.0)])]
    after = scenes.deform(desc, [1], 1.0, amplitude=0.02)
    rays = ray_set(oracle, desc, ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)), 21)
    rd = rt.rays_to_device(rays)
    for mode in ("refuse", "rebalance"):
        gsc = rt.Scene(0, instancing="flat").set_tree_height_bound(mode).load(desc)
        gsc.force_next_op(F)
        push(gsc, after, [1])
        hi = gsc.tree_height_info(ONE)
        print("one-level form, %s: %s, stack %d" % (mode, height_fields(hi), gsc.bvh_stats().max_stack))
        assert not gsc.two_level() and gsc.as_state()[1] == F and hi.cap == 47 and hi.height_before > 47
        if mode == "refuse":
            assert hi.on_device == 0 and hi.subtrees_rebuilt == 0
        else:
            assert hi.on_device == 1 and hi.height_after <= 47 and hi.subtrees_rebuilt >= 1 and gsc.bvh_stats().max_stack <= 47
        traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "one-level form, " + mode)
        gsc.close()


# ---- 9. Renderer -------------------------------------------------------------------------------------------------------------
def test_renderer_reaches_every_replica_and_renders_the_rebalanced_scene(rt, monkeypatch):
    """Renderer.set_tree_height_bound on two slots of one device; the frame after a forced fast build of the chain scene (the
    resize before it starts the temporal history anew) is the first frame of a fresh renderer loaded with the deformed description."""
    from test_gpu_multi_renderer import assert_equal, grab, load
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    hip = C.CDLL("libamdhip64.so")
    desc, after = chain_scene()
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    W, H = 64, 48
    r = rt.Renderer((W // 2, H // 2), devices=[0, 0])
    load(r, desc)
    r.set_mesh_tree_build("device")
    assert r.set_tree_height_bound("rebalance", 20) is r
    for i in range(2):
        hi = r.replica_scene(i).tree_height_info(MESH)
        assert (hi.mode, hi.mesh_tree_cap) == (abi.HEIGHT_BOUND_REBALANCE, 20), i
    with pytest.raises(rt.SunrayError) as e:
        r.set_tree_height_bound("refuse", 20)
    assert e.value.code == -1 and "sr_renderer_set_tree_height_bound" in e.value.description
    for k in (7, 9):
        r.set_mesh_build_type(k, RAPIDLY)
    r.wait_frame(r.render(cam, desc.instances))
    for k in (7, 9):
        r.update_mesh(k, mesh_of(after, k).vertices)
    for i in range(2):
        r.replica_scene(i).force_next_op(F)
    r.resize((W, H))
    r.wait_frame(r.render(cam, after.instances))
    got = grab(rt, hip, r)
    for i in range(2):
        view = r.replica_scene(i)
        hi = view.tree_height_info(MESH)
        assert view.two_level() and tree_info(view) == (2, 0, abi.MESH_TREE_ON_DEVICE), i
        assert hi.on_device == 1 and hi.cap == 20 and hi.height_before > 20 >= hi.height_after and hi.subtrees_rebuilt >= 1, (i, height_fields(hi))
    r.close()
    fresh = rt.Renderer((W, H))
    load(fresh, after)
    fresh.wait_frame(fresh.render(cam, after.instances))
    want = grab(rt, hip, fresh)
    fresh.close()
    assert_equal(want[0], got[0], "RGBA8 output after a rebalanced device build")


# ---- 10. memory --------------------------------------------------------------------------------------------------------------
def test_rebalanced_build_cycles_do_not_grow_hbm(rt):
    """The window of test_device_build_cycles_do_not_grow_hbm with the height bound on and mesh trees held to 12 entries."""
    import torch
    desc = scenes.instanced_field(10)
    sc = device_scene(rt, desc, [1, 5], RAPIDLY).set_tree_height_bound("rebalance", 12)
    free, built = [], 0
    for cycle in range(9 + 27):
        desc = scenes.deform(desc, [1, 5], float(cycle))
        push(sc, desc, [1, 5])
        built += sc.mesh_tree_info().built_on_device
        assert sc.mesh_tree_info().built_on_host == 0
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    window = free[8:]
    assert len(window) == 28 and built == 2 * 4 and sc.tree_height_info(MESH).height_after <= 12
    print("free memory over the window: first %d, last %d, spread %d bytes" % (window[0], window[-1], max(window) - min(window)))
    assert abs(window[-1] - window[0]) < (1 << 20) and max(window) - min(window) < (1 << 20), free
    sc.close()


# ---- 11. AUTO under the height bound -----------------------------------------------------------------------------------------
def test_auto_mode_uses_the_bounded_threshold(rt, oracle):
    """SR_MESH_TREE_BUILD_AUTO under REBALANCE: a mesh of auto_threshold triangles is built on the device, the 960-triangle mesh
    stays below the threshold; under REFUSE the same large mesh stays on the host (threshold: never)."""
    sv, si = scenes.uv_sphere(1.0, 128, 129)
    assert len(si) == 3 * 32768
    desc = scenes.SceneDesc("auto_sphere", camera_pos=(0.0, 0.5, 4.0), camera_target=(0.0, 0.0, 0.0), fov_y=40.0)
    desc.meshes.append(scenes.MeshDesc(1, sv, si, abi.material(base_color=(0.9, 0.5, 0.3, 1.0), roughness=0.3)))
    bv, bi = scenes.uv_sphere(0.4, 32, 16)
    desc.meshes.append(scenes.MeshDesc(2, bv, bi, abi.material()))
    desc.instances = [(1, [scenes.translate(0.0, 0.0, 0.0)]), (2, [scenes.translate(1.6, 0.0, 0.0)])]
    rays = ray_set(oracle, desc, ((-1.5, -1.5, -1.5), (2.2, 1.5, 1.5)), 31)[:3000]
    rd = rt.rays_to_device(rays)
    gsc = device_scene(rt, desc, [1, 2], mode="auto").set_tree_height_bound("rebalance")
    threshold = gsc.mesh_tree_info().auto_threshold
    if threshold == 0xFFFFFFFF:
        pytest.fail("the measured table qualifies sizes from 32 768 triangles on: the bounded threshold must not be 'never'")
    assert threshold <= 32768
    after = scenes.deform(desc, [2], 1.0)
    gsc.force_next_op(F)
    push(gsc, after, [2])
    assert tree_info(gsc) == (0, 1, abi.MESH_TREE_HOST_BELOW_THRESHOLD)
    after = scenes.deform(after, [1], 1.0, amplitude=0.05)
    gsc.force_next_op(F)
    push(gsc, after, [1])
    hi = gsc.tree_height_info(MESH)
    print("auto, 32 768 triangles: mesh trees %s, %s" % (tree_info(gsc), height_fields(hi)))
    assert tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE) and hi.on_device == 1 and gsc.mesh_tree_info().max_stack <= CAP
    traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "auto mode, device build")
    gsc.set_tree_height_bound("refuse")
    after = scenes.deform(after, [1], 2.0, amplitude=0.05)
    gsc.force_next_op(F)
    push(gsc, after, [1])
    assert tree_info(gsc) == (0, 1, abi.MESH_TREE_HOST_BELOW_THRESHOLD)
    traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "auto mode, host builds")
    gsc.close()
