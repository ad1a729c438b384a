"""Device refit of a deforming mesh's tree in the two-level form (sr_scene_set_mesh_build_type + sr_scene_update_mesh; the
reference's Blas::update for a BLAS built with ALLOW_UPDATE, acceleration_structure/blas.rs:149-161, 292-310). The expected result
after an update is what a FRESH scene loaded from the deformed description gives: queries and frames against the oracle, the
rewritten records against numpy, the refitted boxes against the triangles below them, the top level against a fresh two-level
scene. Every comparison is bit for bit."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_update import (TRACE_SCENES, Sequence, mesh_of, moved, push, ray_set, traces_equal_brute_force,  # noqa: E402
                                  with_vertices)
from test_gpu_parity import assert_bits_equal, ref_any, ref_closest  # noqa: E402
from test_oracle_trace import random_rays  # noqa: E402

U, F, S, NONE = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD, abi.OP_NONE
SOMETIMES, RAPIDLY, STATIC = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING, abi.BUILD_STATIC


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


class Heuristic:
    """The per-mesh AsState as the pure functions drive it (sr_as_state_*): what Scene.mesh_as_state must report."""

    def __init__(self, build_type):
        from sunray_amd._lib import lib
        self.L = lib()
        self.L.sr_as_state_next_op.restype = C.c_uint32
        self.st = abi.SrAsState()
        self.L.sr_as_state_initial(C.c_uint32(build_type), C.byref(self.st))

    def next_op(self, changed):
        return self.L.sr_as_state_next_op(C.byref(self.st), 1 if changed else 0)

    def done(self, op):
        self.L.sr_as_state_mark_built(C.byref(self.st), C.c_uint32(op))

    def fields(self):
        return (self.st.changing, self.st.frames_without_changes, self.st.number_of_updates_since_last_rebuild)


def state_fields(st):
    return (st.changing, st.frames_without_changes, st.number_of_updates_since_last_rebuild)


def three_meshes():
    """One triangle (one node, one leaf), one quad (one full leaf of two triangles), one uv_sphere(1, 32, 16) (960 triangles: at
    least three node levels), the sphere instanced twice under general transforms."""
    s = scenes.SceneDesc("three_meshes", camera_pos=(0.0, 1.0, 6.0), camera_target=(0.0, 0.0, 0.0), fov_y=45.0)
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    tv = scenes.make_vertices(np.array([(-1, 0, 0), (1, 0, 0.25), (0, 1.5, 0)], dtype=np.float32), np.tile(np.array((0, 0, 1), dtype=np.float32), (3, 1)))
    s.meshes.append(scenes.MeshDesc(1, tv, np.array([0, 1, 2], dtype=np.uint32), grey))
    qv, qi = scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(2, qv, qi, grey))
    sv, si = scenes.uv_sphere(1.0, 32, 16)
    s.meshes.append(scenes.MeshDesc(3, sv, si, abi.material(base_color=(0.9, 0.5, 0.3, 1.0), roughness=0.3)))
    s.instances = [(1, [scenes.translate(0.0, 0.2, 2.0)]), (2, [scenes.translate(0.0, -1.3, 0.0, 3.0)]),
                   (3, [scenes.translate(-0.8, 0.0, 0.0), scenes.scale_rotate_y(0.6, 0.5, 0.8, 0.4, 1.4, 0.3, -0.5)])]
    return s


THREE_BOX = ((-3.0, -1.5, -3.0), (3.0, 2.0, 3.0))


# ---- 1. queries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "two"])
@pytest.mark.parametrize("name", list(TRACE_SCENES))
def test_refitted_meshes_trace_like_a_fresh_scene(rt, oracle, name, which):
    """SometimesChanges meshes deformed over ten consecutive updates: eight device refits, the ninth operation is the host
    rebuild, the tenth a refit again. After each, TraceRay (closest and existence) and closest_hit equal the oracle's brute force
    over the deformed description, the counters say which path ran, and the per-mesh state is the pure heuristic's."""
    scene_fn, box, one, two = TRACE_SCENES[name]
    keys = one if which == "one" else two
    desc = scene_fn()
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    for k in keys:
        gsc.set_mesh_build_type(k, SOMETIMES)
    want = {k: Heuristic(SOMETIMES) for k in keys}
    others = [m.key for m in desc.meshes if m.key not in keys]
    rays = ray_set(oracle, desc, box, 3)
    rd = rt.rays_to_device(rays)
    ops = []
    for step in range(1, 11):
        desc = scenes.deform(desc, keys, float(step))
        push(gsc, desc, keys)
        info = gsc.mesh_update_info()
        op = want[keys[0]].next_op(True)
        ops.append(op)
        print("%s %s step %d: op %d refitted %d rebuilt %d" % (name, which, step, op, info.blas_refitted, info.blas_rebuilt))
        assert info.dirty_meshes == len(keys) and gsc.two_level() and gsc.as_state()[1] == F
        if op == U:
            assert (info.blas_refitted, info.blas_rebuilt) == (len(keys), 0)
        else:
            assert (info.blas_refitted, info.blas_rebuilt) == (0, len(keys))
        for k in keys:
            assert want[k].next_op(True) == op
            want[k].done(op)
            bt, st, last = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), last) == (SOMETIMES, want[k].fields(), op), (k, step)
        for k in others:
            bt, st, last = gsc.mesh_as_state(k)
            assert (bt, state_fields(st), last) == (STATIC, (0, 0, 0), NONE), (k, step)
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s %s step %d op %d" % (name, which, step, op))
    assert ops == [U] * 8 + [F, U]
    gsc.close()


def test_forced_ops_and_the_settle_rebuild(rt, oracle):
    """force_next_op(UPDATE) refits whatever the counters say, a forced build rebuilds on the host; 16 quiet frames end in the
    mesh's own quality rebuild (the scene's falls on the same frame here), and the tree built then still answers like the oracle."""
    scene_fn, box, one, _ = TRACE_SCENES["cornell_glass_mirror"]
    desc = scene_fn()
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    gsc.set_mesh_build_type(one[0], RAPIDLY)
    want = Heuristic(RAPIDLY)
    rays = ray_set(oracle, desc, box, 9)
    rd = rt.rays_to_device(rays)
    for step in range(1, 15):                           # steps 4 .. 14 are eleven updates in a row: the heuristic alone would rebuild at the ninth
        desc = scenes.deform(desc, one, float(step))
        forced = F if step == 2 else S if step == 3 else U
        gsc.force_next_op(forced)
        push(gsc, desc, one)
        info = gsc.mesh_update_info()
        assert (info.blas_refitted, info.blas_rebuilt) == ((1, 0) if forced == U else (0, 1)), step
        want.done(forced)
        _, st, last = gsc.mesh_as_state(one[0])
        assert (state_fields(st), last) == (want.fields(), forced), step
        if step in (2, 3, 4, 14):
            traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "forced op %d at step %d" % (forced, step))
    quiet = []
    for _ in range(16):
        op = want.next_op(False)
        gsc.end_frame()
        want.done(op)
        _, st, last = gsc.mesh_as_state(one[0])
        assert (state_fields(st), last) == (want.fields(), op)
        quiet.append(last)
    assert quiet == [NONE] * 15 + [S]
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "after the settle rebuild")
    gsc.close()


# ---- 2. records ------------------------------------------------------------------------------------------------------------
def expected_records(mesh, mesh_slot):
    """The leaf-order records of api.cpp build_blas, by PRIMITIVE, as uint32 words: tris [n, 12], shade [n, 12], shade_tex [n, 24]."""
    v = mesh.vertices
    idx = np.asarray(mesh.indices, dtype=np.int64).reshape(-1, 3)
    n = len(idx)
    tris = np.zeros((n, 12), dtype=np.float32)
    shade = np.zeros((n, 12), dtype=np.float32)
    tex = np.zeros((n, 24), dtype=np.float32)
    for j in range(3):
        tris[:, 3 * j:3 * j + 3] = v["position"][idx[:, j]]
        shade[:, 3 * j:3 * j + 3] = v["normal"][idx[:, j]]
        tex[:, 2 * j:2 * j + 2] = v["base_color_tex_coord"][idx[:, j]]
        tex[:, 6 + 2 * j:8 + 2 * j] = v["normal_tex_coord"][idx[:, j]]
    tex[:, 12:15] = v["tangent"][idx[:, 0], :3]
    tex[:, 15] = np.where(v["tangent"][idx[:, 0], 3] >= 0.0, np.float32(1.0), np.float32(-1.0))
    tex[:, 16:19] = v["tangent"][idx[:, 1], :3]
    tex[:, 19:22] = v["tangent"][idx[:, 2], :3]
    tris, shade, tex = tris.view(np.uint32), shade.view(np.uint32), tex.view(np.uint32)
    tris[:, 9] = np.arange(n, dtype=np.uint32)
    shade[:, 10] = mesh_slot
    return tris, shade, tex


def is_textured(mesh):
    return any(int(mesh.material[k + "_image"]) != abi.NULL_TEXTURE for k in ("base_color", "metallic_roughness", "normal", "occlusion", "emissive"))


def records_equal_numpy(gsc, desc, key, what):
    slot = [m.key for m in desc.meshes].index(key)
    mesh = desc.meshes[slot]
    tree = gsc.read_mesh_tree(key)
    sop = tree["slot_of_prim"]
    n = len(mesh.indices) // 3
    assert len(sop) == n and np.array_equal(np.sort(sop), np.arange(n))
    tris, shade, tex = expected_records(mesh, slot)
    assert_bits_equal(tris, tree["tris"].view(np.uint32)[sop], "triangle records, " + what)
    assert_bits_equal(shade, tree["shade"].view(np.uint32)[sop], "shade records, " + what)
    if not is_textured(mesh):
        tex = np.zeros_like(tex)                        # an untextured mesh keeps zeros, in a textured scene too
    assert_bits_equal(tex, tree["shade_tex"].view(np.uint32)[sop], "shade_tex records, " + what)
    return tree


def test_rewritten_records_are_the_bytes_of_a_host_build(rt):
    """After a refit every primitive's 48 + 48 (+ 96) bytes at slot_of_prim[p] are those build_blas writes for the deformed
    vertices: a textured and an untextured mesh of the atrium, a blob of the (untextured) instanced field, the three small meshes."""
    atrium = scenes.atrium(4, 12, 4, 4, 16, 2)
    tex_keys = [m.key for m in atrium.meshes if is_textured(m) and any(k == m.key for k, _ in atrium.instances)]
    plain_keys = [m.key for m in atrium.meshes if not is_textured(m) and any(k == m.key for k, _ in atrium.instances)]
    assert tex_keys
    cases = [(atrium, tex_keys[:2] + plain_keys[:1], 0.06), (scenes.instanced_field(40), [1, 5], 0.12), (three_meshes(), [1, 2, 3], 0.12)]
    for desc, keys, amplitude in cases:
        gsc = rt.Scene(0, instancing="two_level").load(desc)
        for k in keys:
            gsc.set_mesh_build_type(k, SOMETIMES)
            records_equal_numpy(gsc, desc, k, "%s mesh %d as built" % (desc.name, k))
        for step in (1, 2):
            desc = scenes.deform(desc, keys, float(step), amplitude=amplitude)
            push(gsc, desc, keys)
            info = gsc.mesh_update_info()
            assert (info.blas_refitted, info.blas_rebuilt) == (len(keys), 0)
            for k in keys:
                records_equal_numpy(gsc, desc, k, "%s mesh %d after refit %d" % (desc.name, k, step))
        untouched = [m.key for m in desc.meshes if m.key not in keys][:2]
        for k in untouched:
            records_equal_numpy(gsc, desc, k, "%s untouched mesh %d" % (desc.name, k))
        gsc.close()


# ---- 3. containment --------------------------------------------------------------------------------------------------------
def tree_contains_its_triangles(rt, tree, what):
    """Every child box of every node, decoded as the kernel decodes it, contains in float64 the padded boxes (the triangle's
    extent widened by 4e-6 * (|e1| + |e2|) per axis) of all triangles below it; the root reaches every primitive once."""
    nodes, tris = tree["nodes"], tree["tris"].astype(np.float64)
    v = tris[:, :9].reshape(-1, 3, 3)
    pad = 4e-6 * (np.abs(v[:, 1] - v[:, 0]) + np.abs(v[:, 2] - v[:, 0]))
    tlo, thi = v.min(axis=1) - pad, v.max(axis=1) + pad
    seen = []

    def below(node, depth):
        assert depth < 64
        lo, hi, child = rt.decode_node(nodes[node])
        slots_all = []
        for c in range(len(child)):
            ref = int(child[c])
            if ref >= 0:
                assert 0 < ref < len(nodes)
                slots = below(ref, depth + 1)
            else:
                val = (~ref) & 0xFFFFFFFF
                t0, cnt = val >> 3, val & 7
                slots = list(range(t0, t0 + cnt))
                assert cnt == 0 or t0 + cnt <= len(tris)
                seen.extend(slots)
            if slots:
                assert (lo[c].astype(np.float64) <= tlo[slots].min(axis=0)).all() and (hi[c].astype(np.float64) >= thi[slots].max(axis=0)).all(), \
                    "%s: child %d of node %d does not hold its triangles" % (what, c, node)
            slots_all += slots
        return slots_all
    below(0, 0)
    prims = tree["tris"].view(np.uint32)[seen, 9]
    assert len(seen) == len(tris) and np.array_equal(np.sort(prims), np.arange(len(tris))), what
    return len(nodes)


def test_refitted_boxes_contain_their_triangles(rt):
    desc = three_meshes()
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    keys = [1, 2, 3]
    for k in keys:
        gsc.set_mesh_build_type(k, RAPIDLY)
    assert len(gsc.read_mesh_tree(1)["nodes"]) == 1 and len(gsc.read_mesh_tree(2)["nodes"]) == 1
    for step in range(1, 4):
        desc = scenes.deform(desc, keys, float(step), amplitude=0.3 * step)
        if step == 2:                                   # far outside the old boxes, and strongly stretched
            v = mesh_of(desc, 3).vertices.copy()
            v["position"] = v["position"] * np.array([6.0, 0.3, 2.0], dtype=np.float32) + np.array([40.0, -7.0, 3.0], dtype=np.float32)
            desc = with_vertices(desc, 3, v)
        push(gsc, desc, keys)
        assert gsc.mesh_update_info().blas_refitted == 3
        for k in keys:
            n_nodes = tree_contains_its_triangles(rt, records_equal_numpy(gsc, desc, k, "mesh %d step %d" % (k, step)), "mesh %d step %d" % (k, step))
            assert n_nodes == 1 if k < 3 else n_nodes > 21                 # the sphere: more than 1 + 4 + 16 nodes, so at least three levels
    gsc.close()


def test_three_meshes_trace_like_the_oracle_after_refits(rt, oracle):
    desc = three_meshes()
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    for k in (1, 2, 3):
        gsc.set_mesh_build_type(k, SOMETIMES)
    rays = ray_set(oracle, desc, THREE_BOX, 4)
    rd = rt.rays_to_device(rays)
    for step in range(1, 4):
        desc = scenes.deform(desc, [1, 2, 3], float(step), amplitude=0.2)
        push(gsc, desc, [1, 2, 3])
        assert gsc.mesh_update_info().blas_refitted == 3
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "three meshes step %d" % step)
    gsc.close()


# ---- 4. top level ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_top_level_follows_a_refit_that_grows_the_box(rt, mode):
    """A refitted mesh grown 3.5-fold: the instance boxes and the per-instance padding numbers equal a fresh two-level scene's byte
    for byte, whether the top level is built on the host (from the read-back root box) or on the device (from the mesh's row,
    written by the refit; reachable after a mesh update only because a refit keeps the mesh trees resident)."""
    base = scenes.instanced_field(24)
    gsc = rt.Scene(0, instancing="two_level").load(base)
    gsc.set_top_level_build(mode)
    gsc.set_mesh_build_type(2, SOMETIMES)
    gsc.set_mesh_build_type(3, SOMETIMES)
    desc = base
    for f in (1, 2):
        desc = scenes.deform(desc, [2, 3], float(f))
        if f == 2:
            v = mesh_of(desc, 2).vertices.copy()
            v["position"] *= np.float32(3.5)
            desc = with_vertices(desc, 2, v)
        desc = dataclasses.replace(desc, instances=moved(base, f))
        push(gsc, desc, [2, 3])
        info, tl = gsc.mesh_update_info(), gsc.top_level_info()
        assert (info.blas_refitted, info.blas_rebuilt) == (2, 0)
        assert tl.on_device == (1 if mode == "device" else 0), tl.reason
        _, _, recs, boxes = gsc.read_top_level()
        fresh = rt.Scene(0, instancing="two_level").load(desc)
        _, _, recs2, boxes2 = fresh.read_top_level()
        fresh.close()
        assert_bits_equal(boxes2, boxes, "top-level boxes (%s, update %d)" % (mode, f))
        for field in ("w2o", "o2w", "pad_a", "pad_b", "tri_offset", "mesh_slot", "flags"):
            assert_bits_equal(np.ascontiguousarray(recs2[field]), np.ascontiguousarray(recs[field]), "instance records: %s (%s, update %d)" % (field, mode, f))
    gsc.close()


# ---- 5. frames -------------------------------------------------------------------------------------------------------------
class RefitSequence(Sequence):
    """Sequence of test_gpu_mesh_update without its expectation that every dirty mesh is rebuilt on the host."""

    def frame(self, desc=None, keys=()):
        rt, oracle, d0, W, H = self.rt, self.oracle, self.desc, self.W, self.H
        if desc is not None:
            push(self.gsc, desc, keys)
            assert self.gsc.mesh_update_info().dirty_meshes == len(keys) and self.gsc.two_level()
            self.desc = desc
        osc = oracle.OracleScene().load(self.desc)
        f = self.f
        om = oracle.camera_matrices(d0.camera_pos, d0.camera_target, d0.fov_y, W, H, self.prev)
        gm = rt.camera_matrices(d0.camera_pos, d0.camera_target, d0.fov_y, W, H, self.prev)
        self.prev = list(om.view_proj)
        osc.reset_counters(); self.gsc.reset_counters()
        osc.trace_ris(self.of, om, f); self.gsc.trace_ris(self.gf, gm, f)
        osc.trace_final(self.of, om, f); self.gsc.trace_final(self.gf, gm, f)
        h, of, cur = self.gf.host(), self.of, f & 1
        for name, a, b in (("depth", of.depth, h["depth"]), ("normal", of.normal, h["normal"]), ("diffuse", of.diffuse, h["diffuse"]),
                           ("motion", of.motion, h["motion"]), ("reservoirs", of.reservoirs[cur], h["reservoirs"][cur]),
                           ("reservoirs_gi", of.reservoirs_gi[cur], h["reservoirs_gi"][cur]), ("raw_color", of.raw_color, h["raw_color"])):
            assert_bits_equal(a, b, "%s f%d" % (name, f))
        oc, gc = osc.counters(), self.gsc.counters()
        assert (oc.closest_queries, oc.any_queries) == (ref_closest(gc), ref_any(gc))
        osc.close()
        self.f += 1


def test_frames_with_a_refitted_blob_and_lamp(rt, oracle, blue_noise):
    """A RapidlyChanging blob and the EMISSIVE lamp mesh deform every frame while the instances move, 12 frames at 112 x 64:
    G-buffer, both reservoir sets, raw_color and query counts equal the oracle's. Eight refits, the host rebuild, a refit again;
    one frame in between changes nothing and runs end_frame."""
    base = scenes.instanced_field(24)
    seq = RefitSequence(rt, oracle, blue_noise, base, 112, 64, "two_level")
    for k in (1, 5):
        seq.gsc.set_mesh_build_type(k, RAPIDLY)
    want = Heuristic(RAPIDLY)
    seq.frame()
    desc, ops = base, []
    for f in range(1, 12):
        if f == 6:                                      # nothing changes: the facade's end_frame, then the same scene again
            op = want.next_op(False)
            seq.gsc.end_frame()
            want.done(op)
            assert seq.gsc.mesh_as_state(1)[2] == op == NONE
            seq.frame()
            continue
        desc = dataclasses.replace(scenes.deform(desc, [1, 5], float(f)), instances=moved(base, f))
        op = want.next_op(True)
        seq.frame(desc, [1, 5])
        want.done(op)
        info = seq.gsc.mesh_update_info()
        assert (info.blas_refitted, info.blas_rebuilt) == ((2, 0) if op == U else (0, 2)), f
        for k in (1, 5):
            _, st, last = seq.gsc.mesh_as_state(k)
            assert (state_fields(st), last) == (want.fields(), op), (k, f)
        ops.append(op)
    assert ops == [U] * 8 + [F, U]
    seq.gsc.close()


# ---- 6. fallbacks ----------------------------------------------------------------------------------------------------------
def test_fallbacks_end_in_a_host_rebuild_and_equal_the_oracle(rt, oracle):
    scene_fn, box, _, _ = TRACE_SCENES["instanced_field"]
    base = scene_fn()
    rays = ray_set(oracle, base, box, 6)
    rd = rt.rays_to_device(rays)
    # an updatable mesh with an instance whose transform is singular: that instance walks a baked copy, so the mesh is rebuilt
    squash = np.array([1, 0, 0, 0.5, 0, 0, 0, 1.2, 0, 0, 1, 0.3], dtype=np.float32)
    desc = dataclasses.replace(base, instances=[(k, list(xs) + ([squash] if k == 2 else [])) for k, xs in base.instances])
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    gsc.set_mesh_build_type(2, SOMETIMES)
    for step in (1, 2):
        desc = scenes.deform(desc, [2], float(step))
        push(gsc, desc, [2])
        info = gsc.mesh_update_info()
        assert (info.blas_refitted, info.blas_rebuilt) == (0, 1) and gsc.mesh_as_state(2)[2] == F
        traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "baked instance, update %d" % step)
    # the baked instance leaves the list: the next update is a refit; it comes back: the refitted mesh is rebuilt with the rest
    without = dataclasses.replace(scenes.deform(desc, [2], 3.0), instances=base.instances)
    gsc.set_instances(without.instances)
    push(gsc, without, [2])
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (1, 0)
    traces_equal_brute_force(rt, oracle, gsc, without, rays, rd, "refit after the baked instance left")
    again = dataclasses.replace(without, instances=desc.instances)
    gsc.set_instances(again.instances)
    assert gsc.mesh_update_info().blas_rebuilt == 1                     # the stale host copy was not uploaded again
    traces_equal_brute_force(rt, oracle, gsc, again, rays, rd, "baked instance of a refitted mesh")
    gsc.close()
    # a mesh added between two updates: the re-concatenation must not upload the refitted mesh's stale host copy
    desc = base
    gsc = rt.Scene(0, instancing="two_level").load(desc)
    gsc.set_mesh_build_type(1, RAPIDLY)
    desc = scenes.deform(desc, [1], 1.0, amplitude=0.4)
    push(gsc, desc, [1])
    assert gsc.mesh_update_info().blas_refitted == 1
    sv, si = scenes.uv_sphere(0.8, 12, 6)
    extra = scenes.MeshDesc(77, sv, si, mesh_of(base, 2).material)
    gsc.add_mesh(77, sv, si, extra.material)
    desc = dataclasses.replace(desc, meshes=list(desc.meshes) + [extra], instances=list(desc.instances) + [(77, [scenes.translate(0.5, 2.0, 1.0)])])
    gsc.set_instances(desc.instances)
    info = gsc.mesh_update_info()
    assert (info.blas_refitted, info.blas_rebuilt) == (0, 2)            # the new mesh and the refitted one
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "mesh added after a refit")
    desc = scenes.deform(desc, [1], 2.0, amplitude=0.4)
    gsc.update_mesh(1, mesh_of(desc, 1).vertices)
    sv2, si2 = scenes.uv_sphere(0.5, 10, 5)
    extra2 = scenes.MeshDesc(78, sv2, si2, extra.material)
    gsc.add_mesh(78, sv2, si2, extra2.material)                          # between update_mesh and set_instances
    desc = dataclasses.replace(desc, meshes=list(desc.meshes) + [extra2], instances=list(desc.instances) + [(78, [scenes.translate(-2.5, 1.5, 0.0)])])
    gsc.set_instances(desc.instances)
    info = gsc.mesh_update_info()
    assert (info.blas_refitted, info.blas_rebuilt) == (0, 2)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "mesh added between update and set_instances")
    desc = scenes.deform(desc, [1], 3.0, amplitude=0.4)
    push(gsc, desc, [1])
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (1, 0)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "refit after the additions")
    # a Static mesh (the default, and one set back to it) is never refitted; a form switch rebuilds everything
    desc = scenes.deform(desc, [1, 3], 4.0)
    gsc.set_mesh_build_type(1, STATIC)
    push(gsc, desc, [1, 3])
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (0, 2)
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "static meshes")
    gsc.set_mesh_build_type(1, SOMETIMES)
    desc = scenes.deform(desc, [1], 5.0)
    push(gsc, desc, [1])
    assert gsc.mesh_update_info().blas_refitted == 1
    gsc.set_instancing("flat")
    gsc.set_instances(desc.instances)
    assert not gsc.two_level()
    gsc.set_instancing("two_level")
    gsc.set_instances(desc.instances)
    assert gsc.two_level()
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "through the one-level form and back")
    gsc.close()


def test_per_mesh_state_follows_the_slot(rt, oracle):
    """A refitted mesh with a stale host copy and a pending refit is removed and another mesh takes its slot: the newcomer starts
    as a Static mesh that was never built, nothing of it is refitted, it traces like the oracle in both forms, and its tree is a
    fresh two-level scene's byte for byte."""
    desc = three_meshes()
    gsc = rt.Scene(0, instancing="two_level")
    slots = {m.key: gsc.add_mesh(m.key, m.vertices, m.indices, m.material) for m in desc.meshes}
    gsc.set_instances(desc.instances)
    gsc.set_mesh_build_type(3, SOMETIMES)
    desc = scenes.deform(desc, [3], 1.0, amplitude=0.2)
    push(gsc, desc, [3])
    assert (gsc.mesh_update_info().blas_refitted, gsc.mesh_update_info().blas_rebuilt) == (1, 0)      # refitted: its host copy is stale
    gsc.update_mesh(3, mesh_of(scenes.deform(desc, [3], 2.0, amplitude=0.2), 3).vertices)              # and a refit is pending
    gsc.remove(3)
    sv, si = scenes.uv_sphere(1.2, 10, 5)
    new = scenes.MeshDesc(9, sv, si, mesh_of(desc, 3).material)
    assert gsc.add_mesh(9, sv, si, new.material) == slots[3]                                            # LIFO slot reuse
    bt, st, last = gsc.mesh_as_state(9)
    assert (bt, state_fields(st), last) == (STATIC, (0, 0, 0), NONE)
    desc = dataclasses.replace(desc, meshes=[m for m in desc.meshes if m.key != 3] + [new],
                               instances=[(9 if k == 3 else k, xs) for k, xs in desc.instances])
    rays = ray_set(oracle, desc, THREE_BOX, 5)
    rd = rt.rays_to_device(rays)
    gsc.set_instances(desc.instances)
    assert gsc.mesh_update_info().blas_refitted == 0
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "new mesh in a reused slot")
    gsc.set_instancing("flat")
    gsc.set_instances(desc.instances)
    assert not gsc.two_level()
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "reused slot, one-level form")
    gsc.set_instancing("two_level")
    gsc.set_instances(desc.instances)
    assert gsc.two_level()
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "reused slot, two-level form again")
    tree = gsc.read_mesh_tree(9)
    fresh = rt.Scene(0, instancing="two_level").load(desc)
    want = fresh.read_mesh_tree(9)
    fresh.close()
    for part in ("nodes", "tris", "shade", "shade_tex", "slot_of_prim"):
        assert_bits_equal(want[part], tree[part], "mesh tree in a reused slot: %s" % part)
    gsc.close()


def test_refit_cycles_do_not_grow_hbm(rt):
    """Free device memory is constant over 40 update + set_instances cycles (refits, every ninth a host rebuild); ten cycles come
    first, as in test_update_cycles_do_not_grow_hbm: the refit's scratch and the rebuild's re-upload have then both run."""
    import torch
    desc = scenes.instanced_field(10)
    sc = rt.Scene(0, instancing="two_level").load(desc)
    for k in (1, 5):
        sc.set_mesh_build_type(k, RAPIDLY)
    free, refits = [], 0
    for cycle in range(10 + 40):
        desc = scenes.deform(desc, [1, 5], float(cycle))
        push(sc, desc, [1, 5])
        refits += sc.mesh_update_info().blas_refitted
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    window = free[9:]
    assert len(window) == 41 and refits >= 2 * 40
    assert abs(window[-1] - window[0]) < (1 << 20) and max(window) - min(window) < (1 << 20), free
    sc.close()


# ---- 7. Renderer -----------------------------------------------------------------------------------------------------------
def test_renderer_refit_equals_oracle_loop(rt, oracle, monkeypatch):
    """Renderer.set_mesh_build_type + update_mesh in the two-level form: 16 frames of the original, then of two deformations, one
    history; byte for byte the oracle's render loop with a fresh oracle scene per deformation."""
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    desc = scenes.cornell_box()
    W, H = 96, 80
    noise = rt.default_noise_texture()
    r = rt.Renderer((W, H))
    for m in desc.meshes:
        r.load_mesh(m.key, m.vertices, m.indices, m.material)
    for k in (7, 6):
        r.set_mesh_build_type(k, SOMETIMES)
    with pytest.raises(rt.SunrayError) as e:
        r.set_mesh_build_type(7, 3)
    assert e.value.code == -1 and "sr_scene_set_mesh_build_type" in e.value.description
    with pytest.raises(rt.SunrayError) as e:
        r.set_mesh_build_type(12345, SOMETIMES)
    assert e.value.code == -1 and "no mesh" in e.value.description
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    of, prev, d = oracle.HostFrame(W, H, noise), None, desc
    for step in range(3):
        if step:
            d = scenes.deform(d, [7, 6], float(step))
            for k in (7, 6):
                r.update_mesh(k, mesh_of(d, k).vertices)
        img = r.render_to_host_memory(cam, d.instances)
        view = r.replica_scene(0)
        assert view.two_level()
        if step:
            info = view.mesh_update_info()
            assert (info.blas_refitted, info.blas_rebuilt) == (2, 0)
        osc = oracle.OracleScene().load(d)
        for i in range(16):
            f = 16 * step + i
            om = oracle.camera_matrices(d.camera_pos, d.camera_target, d.fov_y, W, H, prev)
            prev = list(om.view_proj)
            osc.trace_ris(of, om, f); osc.trace_final(of, om, f); oracle.post_chain(of, f)
        osc.close()
        assert_bits_equal(of.output, img.view(np.uint32).reshape(-1), "render_to_host_memory after %d refits" % step)
    r.close()


def test_multi_slot_renderer_refit_equals_single_device(rt, monkeypatch):
    """All slots on one GPU: set_mesh_build_type and update_mesh reach every replica, and every replica refits."""
    from test_gpu_multi_renderer import assert_equal, grab, load
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.cornell_box()
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)

    def run(r, slots):
        load(r, desc)
        r.set_mesh_build_type(7, RAPIDLY)
        out, d = [], desc
        for f in range(6):
            if f in (2, 3, 5):
                d = scenes.deform(d, [7], float(f))
                r.update_mesh(7, mesh_of(d, 7).vertices)
            fr = r.render(cam, d.instances)
            if f in (1, 3, 5):
                r.wait_frame(fr)
                out.append(grab(rt, hip, r))
                for i in range(slots):
                    view = r.replica_scene(i)
                    assert view.two_level() and view.mesh_as_state(7)[0] == RAPIDLY
                    if f > 1:
                        assert (view.mesh_update_info().blas_refitted, view.mesh_update_info().blas_rebuilt) == (1, 0)
        return out
    single = rt.Renderer((96, 80))
    want = run(single, 1)
    single.close()
    multi = rt.Renderer((96, 80), devices=[0, 0])
    got = run(multi, 2)
    assert multi.history_overflow() == 0
    multi.close()
    for i, (a, b) in enumerate(zip(want, got)):
        assert_equal(a[0], b[0], "step %d output" % i)
        assert_equal(a[1], b[1], "step %d raw_color" % i)
    assert not np.array_equal(want[0][1], want[2][1])
