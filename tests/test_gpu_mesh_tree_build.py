"""Device fast build of a deforming mesh's tree in the two-level form (sr_scene_set_mesh_tree_build, SR_BLAS_BUILD; csrc/bvh_gpu.hip
srk_blas_build; the reference's Blas::rebuild, acceleration_structure/blas.rs:285-310). The ninth update of an updatable mesh asks
for SR_OP_FAST_BUILD: the device builds the tree into the mesh's ranges of the resident arrays. Expected after it is what a FRESH
scene loaded from the deformed description gives: queries and frames against the oracle, the records against a host build of the
same vertices, the tree against its own triangles, the top level against a fresh two-level scene. Every comparison is bit for bit.
Every scene runs in mode DEVICE unless a test says otherwise, under both topologies of the fast build."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_refit import Heuristic, is_textured, records_equal_numpy, state_fields, tree_contains_its_triangles  # noqa: E402
from test_gpu_mesh_update import mesh_of, moved, push, ray_set, traces_equal_brute_force, with_vertices  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402

U, F, S, NONE = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD, abi.OP_NONE
SOMETIMES, RAPIDLY, STATIC = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING, abi.BUILD_STATIC
TOPOLOGIES = ["lbvh", "ploc16"]


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def seven_meshes():
    """Meshes of 1, 2, 3, 63, 64, 65 and 960 triangles (one node; one full leaf; one leaf and a half; around the 64-lane wave; at
    least three node levels). The 65th triangle of mesh 6 repeats its first (equal Morton codes). Meshes 3, 5 and 7 are instanced
    twice under general affine transforms; no built mesh but the first sits at node 0 or triangle 0 of the concatenation."""
    s = scenes.SceneDesc("seven_meshes", camera_pos=(0.0, 1.0, 6.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    up = np.tile(np.array((0, 0, 1), dtype=np.float32), (5, 1))
    tv = scenes.make_vertices(np.array([(-1, 0, 0), (1, 0, 0.25), (0, 1.5, 0)], dtype=np.float32), up[:3])
    s.meshes.append(scenes.MeshDesc(1, tv, np.array([0, 1, 2], dtype=np.uint32), grey))
    qv, qi = scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(2, qv, qi, grey))
    fv = scenes.make_vertices(np.array([(0, 0, 0), (1, 0, 0.1), (0.6, 1, 0), (-0.6, 1, 0.2), (-1, 0, 0)], dtype=np.float32), up)
    s.meshes.append(scenes.MeshDesc(3, fv, np.array([0, 1, 2, 0, 2, 3, 0, 3, 4], dtype=np.uint32), grey))
    sv, si = scenes.uv_sphere(0.7, 8, 5)
    assert len(si) == 3 * 64
    red = abi.material(base_color=(0.9, 0.3, 0.3, 1.0), roughness=0.4)
    s.meshes.append(scenes.MeshDesc(4, sv, np.ascontiguousarray(si[:-3]), red))
    s.meshes.append(scenes.MeshDesc(5, sv, si, red))
    s.meshes.append(scenes.MeshDesc(6, sv, np.concatenate([si, si[:3]]), red))
    bv, bi = scenes.uv_sphere(1.0, 32, 16)
    s.meshes.append(scenes.MeshDesc(7, bv, bi, abi.material(base_color=(0.9, 0.5, 0.3, 1.0), roughness=0.3)))
    s.instances = [(1, [scenes.translate(0.0, 0.2, 2.0)]), (2, [scenes.translate(0.0, -1.3, 0.0, 3.0)]),
                   (3, [scenes.translate(-2.0, 0.5, 1.0), scenes.scale_rotate_y(1.1, 0.7, 1.3, 0.9, 2.0, -0.5, 0.5)]),
                   (4, [scenes.translate(-1.8, -0.3, -1.0)]),
                   (5, [scenes.translate(1.9, 1.2, -0.8), scenes.scale_rotate_y(0.3, 1.2, 0.6, 0.8, 0.0, 1.4, -1.5)]),
                   (6, [scenes.translate(2.0, -0.5, 1.2)]),
                   (7, [scenes.translate(-0.8, 0.0, 0.0), scenes.scale_rotate_y(0.6, 0.5, 0.8, 0.4, 1.4, 0.3, -0.5)])]
    return s


SEVEN = [1, 2, 3, 4, 5, 6, 7]
SEVEN_BOX = ((-3.0, -1.5, -3.0), (3.0, 2.0, 3.0))


def device_scene(rt, desc, keys, build_type=SOMETIMES, mode="device"):
    gsc = rt.Scene(0, instancing="two_level").set_mesh_tree_build(mode).load(desc)
    for k in keys:
        gsc.set_mesh_build_type(k, build_type)
    return gsc


def tree_info(gsc):
    i = gsc.mesh_tree_info()
    return (i.built_on_device, i.built_on_host, i.reason)


# ---- 1. queries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_device_built_meshes_trace_like_a_fresh_scene(rt, oracle, monkeypatch, topology):
    """Ten consecutive deformations of seven SometimesChanges meshes: eight refits, the ninth step builds all seven trees on the
    device, the tenth refits the trees the device built. After each, TraceRay (closest and existence) and closest_hit equal the
    oracle's brute force, the counters say which path ran, and every mesh's state is the pure heuristic's."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = seven_meshes()
    gsc = device_scene(rt, desc, SEVEN)
    want = {k: Heuristic(SOMETIMES) for k in SEVEN}
    rays = ray_set(oracle, desc, SEVEN_BOX, 3)
    rd = rt.rays_to_device(rays)
    ops = []
    for step in range(1, 11):
        desc = scenes.deform(desc, SEVEN, float(step))
        push(gsc, desc, SEVEN)
        info = gsc.mesh_update_info()
        op = want[1].next_op(True)
        ops.append(op)
        print("%s step %d: op %d refitted %d rebuilt %d, mesh trees %s" % (topology, step, op, info.blas_refitted, info.blas_rebuilt, tree_info(gsc)))
        assert info.dirty_meshes == len(SEVEN) and gsc.two_level()
        if op == U:
            assert (info.blas_refitted, info.blas_rebuilt) == (len(SEVEN), 0) and tree_info(gsc) == (0, 0, abi.MESH_TREE_ON_DEVICE)
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (0, len(SEVEN)) and tree_info(gsc) == (len(SEVEN), 0, abi.MESH_TREE_ON_DEVICE)
            assert info.blas_build_ms == 0.0                            # the host built nothing
        for k in SEVEN:
            assert want[k].next_op(True) == op
            want[k].done(op)
            bt, st, last = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), last) == (SOMETIMES, want[k].fields(), op), (k, step)
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s step %d op %d" % (topology, step, op))
    assert ops == [U] * 8 + [F, U]
    gsc.close()


# ---- 2. records ------------------------------------------------------------------------------------------------------------
def awkward_atrium():
    """The small atrium with one textured and one untextured instanced mesh made awkward: triangle 1 coincides with triangle 0,
    triangle 2 has zero area, the tangents' handedness alternates from vertex to vertex. -> (description, the two keys)"""
    desc = scenes.atrium(4, 12, 4, 4, 16, 2)
    instanced = {k for k, _ in desc.instances}
    tex_key = next(m.key for m in desc.meshes if is_textured(m) and m.key in instanced and len(m.indices) >= 30)
    plain_key = next(m.key for m in desc.meshes if not is_textured(m) and m.key in instanced and len(m.indices) >= 30)
    meshes = []
    for m in desc.meshes:
        if m.key in (tex_key, plain_key):
            v, idx = m.vertices.copy(), np.array(m.indices, dtype=np.uint32, copy=True)
            idx[3:6] = idx[0:3]
            idx[6:9] = (idx[6], idx[6], idx[7])
            v["tangent"][:, 3] = np.where(np.arange(len(v)) % 2 == 0, np.float32(1.0), np.float32(-1.0))
            m = scenes.MeshDesc(m.key, v, idx, m.material)
        meshes.append(m)
    return dataclasses.replace(desc, meshes=meshes), [tex_key, plain_key]


def with_negative_zero(desc, key):
    """The first vertex of triangle 3 of the mesh gets x = -0.0."""
    m = mesh_of(desc, key)
    v = m.vertices.copy()
    v["position"][int(m.indices[9]), 0] = np.float32(-0.0)
    return with_vertices(desc, key, v)


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_device_built_records_are_the_bytes_of_a_host_build(rt, monkeypatch, topology):
    """After a device build every primitive's 48 + 48 (+ 96) bytes at slot_of_prim[p] are those a host build of the same vertices
    writes (numpy's, and a fresh scene's), slot_of_prim is a permutation, and the instance boxes and padding numbers that follow
    from root box, max_abs_vertex and max_edge_sum equal the fresh scene's: with a -0.0 coordinate, a zero-area triangle, two
    coincident triangles and a textured mesh whose tangent handedness disagrees between the vertices of a triangle."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    base, keys = awkward_atrium()
    gsc = device_scene(rt, base, keys)
    desc = scenes.deform(base, keys, 1.0, amplitude=0.06)
    for k in keys:
        desc = with_negative_zero(desc, k)
        v = mesh_of(desc, k)
        assert np.signbit(v.vertices["position"][int(v.indices[9]), 0])
    gsc.force_next_op(F)
    push(gsc, desc, keys)
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (0, 2) and tree_info(gsc) == (2, 0, abi.MESH_TREE_ON_DEVICE)
    fresh = rt.Scene(0, instancing="two_level").load(desc)
    for k in keys + [m.key for m in desc.meshes if m.key not in keys][:2]:
        tree = records_equal_numpy(gsc, desc, k, "%s mesh %d after a device build" % (topology, k))
        want = fresh.read_mesh_tree(k)
        for part in ("tris", "shade", "shade_tex"):
            assert_bits_equal(want[part][want["slot_of_prim"]], tree[part][tree["slot_of_prim"]], "%s of mesh %d by primitive (%s)" % (part, k, topology))
        if k in keys:
            tree_contains_its_triangles(rt, tree, "%s mesh %d" % (topology, k))
    _, _, recs, boxes = gsc.read_top_level()
    _, _, recs2, boxes2 = fresh.read_top_level()
    fresh.close()
    assert_bits_equal(boxes2, boxes, "top-level boxes after a device build (%s)" % topology)
    for field in ("w2o", "o2w", "pad_a", "pad_b", "tri_offset", "mesh_slot", "flags"):
        assert_bits_equal(np.ascontiguousarray(recs2[field]), np.ascontiguousarray(recs[field]), "instance records: %s (%s)" % (field, topology))
    gsc.close()


# ---- 3. structure ----------------------------------------------------------------------------------------------------------
def walk_stack(rt, nodes):
    """Worst-case entries a depth-first walk of the tree holds: a node with k children leaves k - 1 behind when it descends."""
    def need(i, depth):
        assert depth < 64
        _, _, child = rt.decode_node(nodes[i])
        k, deepest = 0, 0
        for ref in child:
            ref = int(ref)
            if ref >= 0:
                k += 1
                deepest = max(deepest, need(ref, depth + 1))
            elif (~ref) & 7:
                k += 1
        return max(k - 1, 0) + deepest
    return need(0, 0)


@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_device_built_tree_holds_its_triangles_within_the_stack_budget(rt, monkeypatch, topology):
    """Each of the seven meshes built alone by a forced fast build: every child box contains the padded boxes of the triangles
    below it, every leaf lies inside the mesh's triangle range, every primitive sits in exactly one leaf, and the reported stack
    need is at most 26 and at least what a walk of the decoded tree needs."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = seven_meshes()
    gsc = device_scene(rt, desc, SEVEN, RAPIDLY)
    for step, k in enumerate(SEVEN, 1):
        desc = scenes.deform(desc, [k], float(step), amplitude=0.3)
        if k == 7:                                      # far outside the old boxes, and strongly stretched
            v = mesh_of(desc, 7).vertices.copy()
            v["position"] = v["position"] * np.array([6.0, 0.3, 2.0], dtype=np.float32) + np.array([40.0, -7.0, 3.0], dtype=np.float32)
            desc = with_vertices(desc, 7, v)
        gsc.force_next_op(F)
        push(gsc, desc, [k])
        assert tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE) and gsc.mesh_as_state(k)[2] == F
        info = gsc.mesh_tree_info()
        tree = records_equal_numpy(gsc, desc, k, "%s mesh %d" % (topology, k))
        n_nodes = tree_contains_its_triangles(rt, tree, "%s mesh %d" % (topology, k))
        need = walk_stack(rt, tree["nodes"])
        print("%s mesh %d: %d triangles, %d nodes, stack %d (a walk needs %d)" % (topology, k, len(tree["tris"]), n_nodes, info.max_stack, need))
        assert n_nodes == info.n_nodes and need <= info.max_stack <= abi.MESH_TREE_STACK_CAP
        assert n_nodes < max(len(tree["tris"]), 2)                      # the builder's bound: fewer inner nodes than triangles
    for k in SEVEN:                                     # the other meshes' ranges were left alone by every build
        tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, k, "%s mesh %d at the end" % (topology, k)), "%s mesh %d at the end" % (topology, k))
    gsc.close()


# ---- 4. mixed call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("topology", TOPOLOGIES)
def test_a_refit_and_a_device_build_share_one_call(rt, oracle, monkeypatch, topology):
    """Mesh 5 at its ninth update, mesh 7 at its third: one set_instances refits one and builds the other on the device, the host
    builds nothing, the arrays stay resident (the step after it refits both), and the queries equal the oracle's."""
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    desc = seven_meshes()
    gsc = device_scene(rt, desc, [5, 7])
    rays = ray_set(oracle, desc, SEVEN_BOX, 5)
    rd = rt.rays_to_device(rays)
    for step in range(1, 11):
        keys = [5] if step <= 6 else [5, 7]
        desc = scenes.deform(desc, keys, float(step))
        push(gsc, desc, keys)
        info = gsc.mesh_update_info()
        if step == 9:
            assert (info.blas_refitted, info.blas_rebuilt) == (1, 1) and tree_info(gsc) == (1, 0, abi.MESH_TREE_ON_DEVICE)
            assert (gsc.mesh_as_state(5)[2], gsc.mesh_as_state(7)[2]) == (F, U) and info.blas_build_ms == 0.0
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (len(keys), 0), step
        if step >= 8:
            traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s mixed call, step %d" % (topology, step))
    gsc.close()


# ---- 5. top level ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_top_level_follows_a_device_build_that_grows_the_box(rt, mode):
    """A mesh grown 3.5-fold and built on the device: instance boxes and per-instance padding numbers equal a fresh two-level
    scene's byte for byte, whether the top level is built on the host (from the read-back block) or on the device (from the mesh's
    row, written by the build's finish kernel)."""
    base = scenes.instanced_field(24)
    gsc = device_scene(rt, base, [2, 3]).set_top_level_build(mode)
    desc = base
    for f in (1, 2):
        desc = scenes.deform(desc, [2, 3], float(f))
        if f == 2:
            v = mesh_of(desc, 2).vertices.copy()
            v["position"] *= np.float32(3.5)
            desc = with_vertices(desc, 2, v)
        desc = dataclasses.replace(desc, instances=moved(base, f))
        if f == 2:
            gsc.force_next_op(F)
        push(gsc, desc, [2, 3])
        info, tl = gsc.mesh_update_info(), gsc.top_level_info()
        assert (info.blas_refitted, info.blas_rebuilt) == ((2, 0) if f == 1 else (0, 2))
        assert tree_info(gsc) == ((0, 0, 0) if f == 1 else (2, 0, 0))
        assert tl.on_device == (1 if mode == "device" else 0), tl.reason
        _, _, recs, boxes = gsc.read_top_level()
        fresh = rt.Scene(0, instancing="two_level").load(desc)
        _, _, recs2, boxes2 = fresh.read_top_level()
        fresh.close()
        assert_bits_equal(boxes2, boxes, "top-level boxes (%s, update %d)" % (mode, f))
        for field in ("w2o", "o2w", "pad_a", "pad_b", "tri_offset", "mesh_slot", "flags"):
            assert_bits_equal(np.ascontiguousarray(recs2[field]), np.ascontiguousarray(recs[field]), "instance records: %s (%s, update %d)" % (field, mode, f))
    gsc.close()


# ---- 6. fallbacks ----------------------------------------------------------------------------------------------------------
def chain_mesh(key):
    """63 tiny triangles at (2^-j, 0, 0), (0, 2^-j, 0), (0, 0, 2^-j), j = 1..21: every split of the Morton order peels one
    triangle off, so the radix tree is a chain some 60 levels deep, more than the 26 entries a mesh tree may need."""
    pos = np.zeros((63 * 3, 3), dtype=np.float32)
    tri = np.array([(0, 0, 0), (1e-9, 0, 0), (0, 1e-9, 0)], dtype=np.float32)
    for j in range(21):
        for a in range(3):
            c = np.zeros(3, dtype=np.float32)
            c[a] = 2.0 ** -(j + 1)
            pos[3 * (3 * j + a):3 * (3 * j + a) + 3] = tri + c
    v = scenes.make_vertices(pos, np.tile(np.array((0, 0, 1), dtype=np.float32), (len(pos), 1)))
    return scenes.MeshDesc(key, v, np.arange(len(pos), dtype=np.uint32), abi.material(base_color=(0.5, 0.5, 0.9, 1.0), roughness=0.5))


def test_fallbacks_name_their_reason_and_equal_the_oracle(rt, oracle, monkeypatch):
    base = seven_meshes()
    rays = ray_set(oracle, base, SEVEN_BOX, 6)
    rd = rt.rays_to_device(rays)

    def ninth_step(gsc, desc, keys, what, want_info, forced=F):
        desc = scenes.deform(desc, keys, 1.0)
        if forced is not None:
            gsc.force_next_op(forced)
        push(gsc, desc, keys)
        assert tree_info(gsc) == want_info, what
        assert gsc.mesh_update_info().blas_rebuilt == want_info[0] + want_info[1], what
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, what)
        return desc

    # mode HOST, and the environment's spelling of it
    gsc = device_scene(rt, base, [5, 7], mode="host")
    ninth_step(gsc, base, [5, 7], "mode host", (0, 2, abi.MESH_TREE_HOST_MODE))
    gsc.close()
    for value, mode in (("host", abi.MESH_TREE_BUILD_HOST), ("device", abi.MESH_TREE_BUILD_DEVICE), ("auto", abi.MESH_TREE_BUILD_AUTO),
                        ("Device", abi.MESH_TREE_BUILD_AUTO), ("", abi.MESH_TREE_BUILD_AUTO), ("gpu", abi.MESH_TREE_BUILD_AUTO)):
        monkeypatch.setenv("SR_BLAS_BUILD", value)      # read when the scene is created; anything unknown means auto
        gsc = rt.Scene(0, instancing="two_level")
        assert gsc.mesh_tree_info().mode == mode, value
        gsc.close()
    monkeypatch.delenv("SR_BLAS_BUILD")
    gsc = rt.Scene(0, instancing="two_level")
    assert gsc.mesh_tree_info().mode == abi.MESH_TREE_BUILD_AUTO
    assert gsc.set_mesh_tree_build("device").mesh_tree_info().mode == abi.MESH_TREE_BUILD_DEVICE      # the call overrides the environment's choice
    gsc.close()
    # a Static mesh next to an updatable one
    gsc = device_scene(rt, base, [7])
    ninth_step(gsc, base, [5, 7], "static mesh", (0, 2, abi.MESH_TREE_HOST_STATIC_MESH))
    gsc.close()
    # a forced slow build
    gsc = device_scene(rt, base, [5, 7])
    ninth_step(gsc, base, [5, 7], "forced slow build", (0, 2, abi.MESH_TREE_HOST_SLOW_BUILD), forced=S)
    # ... and the same scene builds on the device right after: the host's upload left the arrays resident
    ninth_step(gsc, base, [5, 7], "device build after a host build", (2, 0, abi.MESH_TREE_ON_DEVICE))
    gsc.close()
    # a baked (singular-transform) instance of the mesh
    squash = np.array([1, 0, 0, 0.5, 0, 0, 0, 1.2, 0, 0, 1, 0.3], dtype=np.float32)
    desc = dataclasses.replace(base, instances=[(k, list(xs) + ([squash] if k == 5 else [])) for k, xs in base.instances])
    gsc = device_scene(rt, desc, [5])
    ninth_step(gsc, desc, [5], "baked instance", (0, 1, abi.MESH_TREE_HOST_BAKED_INSTANCE))
    gsc.close()
    # a mesh added between update and set_instances
    gsc = device_scene(rt, base, [7])
    desc = scenes.deform(base, [7], 1.0)
    gsc.update_mesh(7, mesh_of(desc, 7).vertices)
    sv, si = scenes.uv_sphere(0.5, 10, 5)
    extra = scenes.MeshDesc(78, sv, si, mesh_of(base, 4).material)
    gsc.add_mesh(78, sv, si, extra.material)
    desc = dataclasses.replace(desc, meshes=list(desc.meshes) + [extra], instances=list(desc.instances) + [(78, [scenes.translate(-2.5, 1.5, 0.0)])])
    gsc.force_next_op(F)
    gsc.set_instances(desc.instances)
    assert tree_info(gsc) == (0, 2, abi.MESH_TREE_HOST_NOT_RESIDENT)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "mesh added between update and set_instances")
    gsc.close()
    # a radix tree deeper than a mesh tree may be: refused, the host's depth-limited builder takes over
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    chain = chain_mesh(9)
    desc = dataclasses.replace(base, meshes=list(base.meshes) + [chain], instances=list(base.instances) + [(9, [scenes.translate(0.0, 0.0, 0.0, 2.0)])])
    gsc = device_scene(rt, desc, [7, 9])
    moved_chain = chain.vertices.copy()
    moved_chain["normal"] = np.array((0, 1, 0), dtype=np.float32)
    after = with_vertices(scenes.deform(desc, [7], 1.0), 9, moved_chain)
    gsc.force_next_op(F)
    push(gsc, after, [7, 9])
    print("chain of 63 triangles under lbvh: mesh trees %s" % (tree_info(gsc),))
    assert tree_info(gsc) == (0, 2, abi.MESH_TREE_HOST_STACK_BUDGET)
    assert gsc.bvh_stats().max_stack <= abi.TL_STACK_CAP
    traces_equal_brute_force(rt, oracle, gsc, after, rays, rd, "a tree outside the stack budget")
    gsc.close()


# ---- 7. HBM ----------------------------------------------------------------------------------------------------------------
def test_device_build_cycles_do_not_grow_hbm(rt):
    """Free device memory after the first device build of each mesh (the ninth step) equals free memory after three more nine-step
    cycles: the node range a mesh took at its first build is kept, the builder's scratch is reused. "Equals" is measured as
    the existing leak tests measure it (test_refit_cycles_do_not_grow_hbm): the free memory the driver reports moves in steps of
    its own allocation granule, so first against last and the spread of the window both stay under 1 MiB, far below what one
    leaked node range (64 bytes per triangle) or scratch slab of these meshes would take over 27 cycles."""
    import torch
    desc = scenes.instanced_field(10)
    sc = device_scene(rt, desc, [1, 5], RAPIDLY)
    free, built = [], 0
    for cycle in range(9 + 27):
        desc = scenes.deform(desc, [1, 5], float(cycle))
        push(sc, desc, [1, 5])
        built += sc.mesh_tree_info().built_on_device
        assert sc.mesh_tree_info().built_on_host == 0
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    window = free[8:]
    assert len(window) == 28 and built == 2 * 4
    print("free memory over the window: first %d, last %d, spread %d bytes" % (window[0], window[-1], max(window) - min(window)))
    assert abs(window[-1] - window[0]) < (1 << 20) and max(window) - min(window) < (1 << 20), free
    sc.close()


# ---- 8. Renderer -----------------------------------------------------------------------------------------------------------
def renderer_frames(rt, hip, r, desc, slots):
    """Eleven frames of the blob-and-lamp scene at 64 x 48, blob 1 and lamp 5 deformed before every frame but the first: eight
    refits, the device build at the ninth, a refit of the device-built trees. -> [(output, raw_color)] per frame, descriptions"""
    from test_gpu_multi_renderer import grab, load
    load(r, desc)
    r.set_mesh_tree_build("device")
    for k in (1, 5):
        r.set_mesh_build_type(k, RAPIDLY)
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    out, descs, d = [], [], desc
    for f in range(11):
        if f:
            d = scenes.deform(d, [1, 5], float(f))
            for k in (1, 5):
                r.update_mesh(k, mesh_of(d, k).vertices)
        r.wait_frame(r.render(cam, d.instances))
        out.append(grab(rt, hip, r))
        descs.append(d)
        for i in range(slots):
            view = r.replica_scene(i)
            info, ti = view.mesh_update_info(), view.mesh_tree_info()
            assert view.two_level() and ti.mode == abi.MESH_TREE_BUILD_DEVICE
            if f:
                assert (info.blas_refitted, info.blas_rebuilt, ti.built_on_device, ti.built_on_host) == ((0, 2, 2, 0) if f == 9 else (2, 0, 0, 0)), (f, i)
    assert r.mesh_tree_info().mode == abi.MESH_TREE_BUILD_DEVICE
    return out, descs


def test_renderer_frames_across_a_device_build(rt, oracle, monkeypatch):
    """Renderer.set_mesh_tree_build("device"): output and raw_color of every frame equal the oracle's loop (a fresh oracle scene
    per deformation, one history), and a two-slot renderer on one device gives the single-device frames, output and raw_color."""
    from test_gpu_multi_renderer import assert_equal
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.instanced_field(24)
    W, H = 64, 48
    single = rt.Renderer((W, H))
    with pytest.raises(rt.SunrayError) as e:
        from sunray_amd._lib import check, lib
        check(lib().sr_renderer_set_mesh_tree_build(single._h, C.c_uint32(3)))
    assert e.value.code == -1 and "sr_renderer_set_mesh_tree_build: mode must be" in e.value.description
    want, descs = renderer_frames(rt, hip, single, desc, 1)
    single.close()
    of, prev = oracle.HostFrame(W, H, rt.default_noise_texture()), None
    for f, d in enumerate(descs):
        osc = oracle.OracleScene().load(d)
        om = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        prev = list(om.view_proj)
        osc.trace_ris(of, om, f); osc.trace_final(of, om, f); oracle.post_chain(of, f)
        osc.close()
        assert_bits_equal(of.output, want[f][0], "output of frame %d" % f)
        assert_bits_equal(of.raw_color, want[f][1], "raw_color of frame %d" % f)
    multi = rt.Renderer((W, H), devices=[0, 0])
    got, _ = renderer_frames(rt, hip, multi, desc, 2)
    assert multi.history_overflow() == 0
    multi.close()
    for f, (a, b) in enumerate(zip(want, got)):
        assert_equal(a[0], b[0], "frame %d output" % f)
        assert_equal(a[1], b[1], "frame %d raw_color" % f)
