"""Deforming geometry: Scene.update_mesh / Renderer.update_mesh (sr_scene_update_mesh, the reference's Blas::update,
acceleration_structure/blas.rs:285-310) against the oracle. The expected result after an update is, by definition, what a FRESH
oracle scene loaded from the deformed description gives; temporal state lives in the frame buffers, so a sequence keeps one
HostFrame and loads a fresh oracle scene per deformation. Every comparison is bit for bit."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _moving_instances, assert_bits_equal, ref_any, ref_closest, small_atrium  # noqa: E402
from test_oracle_trace import camera_rays, random_rays  # noqa: E402

U, F, S = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD
ERR_INVALID_ARG, ERR_STATE = -1, -4
FORMS = ["flat", "two_level"]


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def mesh_of(desc, key):
    return next(m for m in desc.meshes if m.key == key)


def push(gsc, desc, keys):
    """update_mesh for `keys` with the vertices `desc` holds, then ONE set_instances that applies them all."""
    for k in keys:
        gsc.update_mesh(k, mesh_of(desc, k).vertices)
    gsc.set_instances(desc.instances)


with_vertices = scenes.with_mesh_vertices


def ray_set(oracle, desc, box, seed):
    short = random_rays(3000, seed + 1, box=box)
    short["tmax"] = np.random.default_rng(seed).random(3000).astype(np.float32) * 2 + 0.01
    axis = random_rays(1500, seed + 2, box=box)
    axis["dir"][:500] = (1, 0, 0); axis["dir"][500:1000] = (0, -1, 0); axis["dir"][1000:] = (0, 0, 1)
    return np.concatenate([random_rays(8000, seed, box=box), camera_rays(oracle, desc, 64, 48), short, axis])


def traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, what):
    osc = oracle.OracleScene().load(desc)
    osc.set_brute_force(True)
    hits_t = gsc.trace_closest(rd, len(rays))
    hits = rt.hits_from_device(hits_t)
    want = osc.trace_closest(rays)
    assert (want["t"] >= 0).mean() > 0.03
    assert_bits_equal(want, hits, "closest hits, " + what)
    assert np.array_equal(osc.trace_any(rays), gsc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32)), "occlusion, " + what
    pay = gsc.shade_closest_hit(hits_t, len(hits)).cpu().numpy().view(np.uint32).reshape(-1).view(abi.RAY_PAYLOAD)
    assert_bits_equal(osc.shade_closest_hit(want), pay, "payloads, " + what)
    osc.close()


# (scene, its box for random rays, keys deformed alone, keys deformed together)
TRACE_SCENES = {
    "instanced_field": (lambda: scenes.instanced_field(40), ((-14, -1, -14), (14, 9, 14)), [1], [2, 5]),      # 21 k triangles: device fast build
    "cornell_glass_mirror": (scenes.cornell_glass_mirror, ((-1, 0, -1), (1, 2, 1)), [7], [8, 3]),
}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(TRACE_SCENES))
def test_updated_meshes_trace_like_a_fresh_scene(rt, oracle, name, form):
    """One mesh, then two meshes at once, deformed and applied by each of Update, FastBuild and SlowBuild: TraceRay (closest and
    existence) and closest_hit on random, camera, short and axis-parallel rays equal the oracle's brute force over the deformed
    description. In the two-level form every op is the rebuild of the dirty meshes' trees + the top level."""
    scene_fn, box, one, two = TRACE_SCENES[name]
    desc = scene_fn()
    gsc = rt.Scene(0, instancing=form).load(desc)
    rays = ray_set(oracle, desc, box, 3)
    rd = rt.rays_to_device(rays)
    phase = 0.0
    for op in (U, F, S):
        for keys in (one, two):
            phase += 1.0
            desc = scenes.deform(desc, keys, phase)
            gsc.force_next_op(op)
            push(gsc, desc, keys)
            info, last = gsc.mesh_update_info(), gsc.as_state()[1]
            assert info.dirty_meshes == len(keys)
            if form == "flat":
                assert last == op and info.reshaded == (1 if op == U else 0) and info.blas_rebuilt == 0
            else:
                assert gsc.two_level() and last == F and info.blas_rebuilt == len(keys)      # only the dirty meshes' trees
            traces_equal_brute_force(rt, oracle, gsc, desc, rays, rd, "%s %s op %d keys %s" % (name, form, op, keys))
    gsc.close()


def test_update_applied_by_the_radix_tree_fast_build(rt, oracle, monkeypatch):
    """The other SR_FAST_BUILD topology (binary radix tree instead of PLOC) picks up the new vertices as well."""
    monkeypatch.setenv("SR_FAST_BUILD", "lbvh")
    scene_fn, box, one, two = TRACE_SCENES["instanced_field"]
    desc = scene_fn()
    gsc = rt.Scene(0, instancing="flat").load(desc)
    monkeypatch.delenv("SR_FAST_BUILD")
    rays = ray_set(oracle, desc, box, 5)
    desc = scenes.deform(desc, two, 1.5)
    gsc.force_next_op(F)
    push(gsc, desc, two)
    assert gsc.as_state()[1] == F
    traces_equal_brute_force(rt, oracle, gsc, desc, rays, rt.rays_to_device(rays), "radix-tree fast build")
    gsc.close()


# ---- frames ----------------------------------------------------------------------------------------------------------------
def read_device(hip, ptr, nbytes):
    out = np.zeros(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(int(ptr)), C.c_size_t(nbytes), C.c_int(2)) == 0
    return out


def tables_equal_fresh_scene(rt, gsc, desc, form):
    """sr_scene_get_tables after an update against a scene freshly loaded from the same description: transforms, emissive
    table and indirection byte for byte; of the mesh table the materials and what the vertex / index pointers hold."""
    import torch  # noqa: F401
    hip = C.CDLL("libamdhip64.so")
    fresh = rt.Scene(0, instancing=form).load(desc)
    a, b = gsc.tables(), fresh.tables()
    for k in ("transforms", "indirection", "emissive_triangles"):
        assert_bits_equal(b[k], a[k], "table " + k)
    assert a["num_lights"] == b["num_lights"] and len(a["meshes_info"]) == len(b["meshes_info"]) == len(desc.meshes)
    assert_bits_equal(b["meshes_info"]["material"], a["meshes_info"]["material"], "mesh table materials")
    for slot, m in enumerate(desc.meshes):
        for mi in (a["meshes_info"][slot], b["meshes_info"][slot]):
            assert_bits_equal(m.vertices, read_device(hip, mi["vertices"], m.vertices.nbytes), "device vertices of mesh %d" % m.key)
            assert_bits_equal(np.ascontiguousarray(m.indices, dtype=np.uint32), read_device(hip, mi["indices"], len(m.indices) * 4), "device indices of mesh %d" % m.key)
    fresh.close()


class Sequence:
    """One GPU scene and one pair of frame buffers followed through a sequence of descriptions; every frame's G-buffer,
    both reservoir buffers, raw_color and query counts are compared with a fresh oracle scene of that frame's description."""

    def __init__(self, rt, oracle, blue_noise, desc, W, H, form):
        self.rt, self.oracle, self.form, self.desc, self.W, self.H = rt, oracle, form, desc, W, H
        self.gsc = rt.Scene(0, instancing=form).load(desc)
        self.of, self.gf = oracle.HostFrame(W, H, blue_noise), rt.DeviceFrame(W, H, blue_noise)
        self.prev, self.f, self.ops = None, 0, []

    def frame(self, desc=None, keys=(), op=None, tables=False):
        rt, oracle, d0, W, H = self.rt, self.oracle, self.desc, self.W, self.H
        if desc is not None:
            if op is not None:
                self.gsc.force_next_op(op)
            push(self.gsc, desc, keys)
            assert self.gsc.mesh_update_info().dirty_meshes == len(keys)
            if self.form == "two_level":
                assert self.gsc.two_level() and self.gsc.mesh_update_info().blas_rebuilt == len(keys)
            self.desc = desc
        self.ops.append(self.gsc.as_state()[1])
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
            assert_bits_equal(a, b, "%s f%d (%s, op %d)" % (name, f, self.form, self.ops[-1]))
        oc, gc = osc.counters(), self.gsc.counters()
        assert (oc.closest_queries, oc.any_queries) == (ref_closest(gc), ref_any(gc))
        osc.close()
        if tables:
            tables_equal_fresh_scene(rt, self.gsc, self.desc, self.form)
        self.f += 1
        return h


def moved(desc, f):
    """The blobs of an instanced_field drift and bob; ground and lamps stay (same layout, so an Update can take it)."""
    out = []
    for key, xs in desc.instances:
        ys = []
        for j, x in enumerate(xs):
            y = np.array(x, dtype=np.float32).copy()
            if len(xs) > 4:
                y[3] += np.float32(0.11 * f * ((j % 3) - 1)); y[7] += np.float32(0.05 * f * (j % 2)); y[11] -= np.float32(0.07 * f)
            ys.append(y)
        out.append((key, ys))
    return out


def test_free_heuristic_with_a_deforming_light_and_moving_instances(rt, oracle, blue_noise):
    """A blob and the EMISSIVE lamp mesh deform every frame while the blobs' instances move: light table, NEE and RIS candidates
    follow the emissive arena. The heuristic runs free: 8 Updates (reshading), the device FastBuild, Updates again, then quiet
    frames up to the settle SlowBuild, and the frame after it still equals the oracle."""
    base = scenes.instanced_field(10)                               # 5 284 triangles: the fast build runs on the device
    seq = Sequence(rt, oracle, blue_noise, base, 96, 64, "flat")
    seq.frame()
    desc = base
    for f in range(1, 12):
        desc = dataclasses.replace(scenes.deform(desc, [1, 5], float(f)), instances=moved(base, f))
        seq.frame(desc, [1, 5], tables=f in (1, 9))
        assert seq.gsc.mesh_update_info().reshaded == (1 if seq.ops[-1] == U else 0)
    assert seq.ops == [S] + [U] * 8 + [F] + [U] * 2
    assert seq.gsc.bvh_stats().n_triangles >= 4096
    quiet = []
    for _ in range(16):
        seq.gsc.end_frame(); quiet.append(seq.gsc.as_state()[1])
    assert quiet == [abi.OP_NONE] * 15 + [S] and seq.gsc.as_state()[0].changing == 0
    seq.frame()                                                     # the settled tree was built from the updated vertices
    seq.gsc.close()


@pytest.mark.parametrize("form", FORMS)
def test_textured_atrium_with_changing_uvs_normals_and_tangents(rt, oracle, blue_noise, form):
    """small_atrium: the floor, the instanced columns (uv, normal-map uv, tangents with handedness -1) and an emissive textured lamp
    deform over 7 frames, applied by every op: the shade_tex records are rewritten in place (Update) or rebuilt."""
    base = small_atrium()
    keys = [1, 6, 10]                                               # floor, columns (8 instances), first lamp
    assert mesh_of(base, 6).vertices["tangent"][:, 3].min() == -1.0 and float(mesh_of(base, 10).material["emissive_factor"][3]) > 0
    seq = Sequence(rt, oracle, blue_noise, base, 120, 68, form)
    seq.frame()
    desc = base
    for f, op in enumerate((U, U, F, U, S, U), start=1):
        desc = scenes.deform(desc, keys, float(f), amplitude=0.06)
        seq.frame(desc, keys, op, tables=f == 2)
    if form == "flat":
        assert seq.ops == [S, U, U, F, U, S, U]
    seq.gsc.close()


def test_two_level_grown_box_and_baked_instance(rt, oracle, blue_noise):
    """Two-level form: a mesh whose deformation grows its box several-fold (the per-instance padding numbers and the top-level boxes
    must follow), with an instance list that also holds a zero-scale (baked) instance of the deformed mesh; instances move too."""
    base = field = scenes.instanced_field(24)
    squash = np.array([1, 0, 0, 0.5, 0, 0, 0, 1.2, 0, 0, 1, 0.3], dtype=np.float32)       # y scale 0: baked copy of mesh 2
    base = dataclasses.replace(base, instances=[(k, list(xs) + ([squash] if k == 2 else [])) for k, xs in base.instances])
    seq = Sequence(rt, oracle, blue_noise, base, 112, 64, "two_level")
    seq.frame()
    desc = base
    for f in range(1, 7):
        desc = scenes.deform(desc, [2, 3], float(f))
        if f in (2, 4):                                              # mesh 2 grows 3.5-fold, later shrinks back
            v = mesh_of(desc, 2).vertices.copy()
            v["position"] *= np.float32(3.5 if f == 2 else 1.0 / 3.5)
            desc = with_vertices(desc, 2, v)
        desc = dataclasses.replace(desc, instances=[(k, list(xs) + ([squash] if k == 2 else [])) for k, xs in moved(field, f)])
        seq.frame(desc, [2, 3])
        if f == 2:
            _, _, recs, boxes = seq.gsc.read_top_level()
            fresh = rt.Scene(0, instancing="two_level").load(desc)
            _, _, recs2, boxes2 = fresh.read_top_level()
            assert_bits_equal(recs2, recs, "instance records")
            assert_bits_equal(boxes2, boxes, "top-level boxes")
            fresh.close()
    assert set(seq.ops[1:]) == {F}
    seq.gsc.close()


# ---- edges -----------------------------------------------------------------------------------------------------------------
def one_frame(rt, sc, desc, W, H, blue_noise):
    """Bits of a first frame (frame_count 0, fresh buffers): raw_color, reservoirs, depth."""
    fr = rt.DeviceFrame(W, H, blue_noise)
    m = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H)
    sc.trace_ris(fr, m, 0); sc.trace_final(fr, m, 0)
    h = fr.host()
    return h["raw_color"].copy(), h["reservoirs"][0].copy(), h["depth"].copy()


def one_oracle_frame(oracle, desc, W, H, blue_noise):
    osc = oracle.OracleScene().load(desc)
    fr = oracle.HostFrame(W, H, blue_noise)
    m = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H)
    osc.trace_ris(fr, m, 0); osc.trace_final(fr, m, 0)
    osc.close()
    return fr.raw_color, fr.reservoirs[0], fr.depth


def assert_frames_equal(want, got, what):
    for name, a, b in zip(("raw_color", "reservoirs", "depth"), want, got):
        assert_bits_equal(a, b, "%s, %s" % (name, what))


@pytest.mark.parametrize("form", FORMS)
def test_update_edges_and_refusals(rt, oracle, blue_noise, form):
    W, H = 80, 60
    desc = scenes.cornell_glass_mirror()
    sphere = mesh_of(desc, 7)
    sc = rt.Scene(0, instancing=form).load(desc)
    original = one_frame(rt, sc, desc, W, H, blue_noise)
    assert_frames_equal(one_oracle_frame(oracle, desc, W, H, blue_noise), original, "original")

    def update_equals_oracle(d, keys, op, what):
        sc.force_next_op(op)
        push(sc, d, keys)
        got = one_frame(rt, sc, d, W, H, blue_noise)
        assert_frames_equal(one_oracle_frame(oracle, d, W, H, blue_noise), got, what)
        return got
    # triangles collapsed to zero area (a band of vertices pulled onto one line) and to coincident vertices (a cap pulled to a point)
    v = sphere.vertices.copy()
    v["position"][1:97] = v["position"][1]
    v["position"][200:264, 1] = v["position"][200, 1]; v["position"][200:264, 0] = v["position"][200, 0]
    update_equals_oracle(with_vertices(desc, 7, v), [7], U, "collapsed triangles (update)")
    update_equals_oracle(with_vertices(desc, 7, v), [7], F, "collapsed triangles (fast build)")
    # far outside the old bounds, rigid + uniform scale: the sphere (radius 0.4 around the origin of its object space) becomes a
    # 60-unit sphere 470 units away, where the camera sees it past the right wall
    v = sphere.vertices.copy()
    v["position"] = v["position"] * np.float32(150.0) + np.array([226.0, 40.0, -466.0], dtype=np.float32)
    d_far = with_vertices(desc, 7, v)
    far = update_equals_oracle(d_far, [7], U, "far displacement")
    assert not np.array_equal(far[0], original[0])
    aimed = random_rays(3000, 21, box=((120.0, 0.0, -380.0), (330.0, 90.0, -250.0)))       # from outside the box towards the far sphere
    centre = np.array([226.35, 40.4, -465.9]) + 45.0 * np.random.default_rng(22).normal(size=(3000, 3))
    dirs = centre - aimed["origin"]
    aimed["dir"] = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    traces_equal_brute_force(rt, oracle, sc, d_far, aimed, rt.rays_to_device(aimed), "rays at the displaced sphere")
    # far outside the old bounds, non-rigid: the sphere is drawn out into a horn, its top ring 21 times wider and 50 units away
    # while the bottom stays (triangles up to 90 times longer than high); frame against the oracle, rays against its brute force
    v = sphere.vertices.copy()
    p = v["position"].astype(np.float64)
    t = ((p[:, 1] + 0.4) / 0.8) ** 2
    horn = p * (1.0 + 20.0 * t)[:, None] + t[:, None] * np.array([30.0, 12.0, -40.0])
    v["position"] = horn.astype(np.float32)
    d_horn = with_vertices(desc, 7, v)
    update_equals_oracle(d_horn, [7], U, "non-rigid far displacement")
    aimed = random_rays(3000, 21, box=((-5.0, 0.0, -45.0), (40.0, 25.0, 5.0)))
    target = horn[np.random.default_rng(22).integers(0, len(horn), 3000)] + np.array([0.35, 0.4, 0.1]) + np.random.default_rng(23).normal(size=(3000, 3))
    dirs = target - aimed["origin"]
    aimed["dir"] = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([aimed, camera_rays(oracle, d_horn, 96, 72)])
    traces_equal_brute_force(rt, oracle, sc, d_horn, rays, rt.rays_to_device(rays), "rays at the horn")
    # back to the original vertices: the original frame's bits
    sc.force_next_op(U)
    push(sc, desc, [7])
    assert_frames_equal(original, one_frame(rt, sc, desc, W, H, blue_noise), "back to the original vertices")
    # refusals leave the scene exactly as it was: nothing pending, the next frame is the frame before the call
    bad = sphere.vertices.copy()
    bad["position"][17, 1] = np.nan
    for what, key, verts, word in (("wrong count", 7, sphere.vertices[:-1], b"%d vertices given" % (len(sphere.vertices) - 1)), ("NaN position", 7, bad, b"vertex 17 has a non-finite position"),
                                   ("unknown key", 12345, sphere.vertices, b"no mesh")):
        with pytest.raises(rt.SunrayError) as e:
            sc.update_mesh(key, verts)
        assert e.value.code == ERR_INVALID_ARG and word in e.value.description.encode(), (what, e.value.description)
        assert_frames_equal(original, one_frame(rt, sc, desc, W, H, blue_noise), "after refused " + what)
    with pytest.raises(rt.SunrayError) as e:
        sc.update_mesh(7, sphere.vertices[:-1])
    assert str(len(sphere.vertices) - 1) in e.value.description and str(len(sphere.vertices)) in e.value.description      # names both counts
    # between update_mesh and set_instances the structure is stale: every call that reads it says so
    d1 = scenes.deform(desc, [7], 1.0)
    sc.update_mesh(7, mesh_of(d1, 7).vertices)
    rays = random_rays(64, 1)
    rd = rt.rays_to_device(rays)
    fr = rt.DeviceFrame(W, H, blue_noise)
    m = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H)
    stale_calls = [lambda: sc.trace_closest(rd, len(rays)), lambda: sc.trace_any(rd, len(rays)), lambda: sc.trace_ris(fr, m, 0),
                   lambda: sc.trace_final(fr, m, 0), lambda: sc.shade_closest_hit(rd, 8), lambda: sc.end_frame()]
    if form == "flat":
        stale_calls.append(sc.read_bvh)
    for call in stale_calls:
        with pytest.raises(rt.SunrayError) as e:
            call()
        assert e.value.code == ERR_STATE and "sr_scene_set_instances must follow sr_scene_update_mesh" in e.value.description
    sc.set_instances(desc.instances)
    assert_frames_equal(one_oracle_frame(oracle, d1, W, H, blue_noise), one_frame(rt, sc, d1, W, H, blue_noise), "after the pending update")
    # a mesh without an instance just has its data replaced: nothing is pending; instanced later, it shows the new vertices
    without8 = [(k, xs) for k, xs in d1.instances if k != 8]
    sc.set_instances(without8)
    d2 = scenes.deform(d1, [8], 2.0)
    sc.update_mesh(8, mesh_of(d2, 8).vertices)
    d2_without = dataclasses.replace(d2, instances=without8)
    assert_frames_equal(one_oracle_frame(oracle, d2_without, W, H, blue_noise), one_frame(rt, sc, d2_without, W, H, blue_noise), "uninstanced update")
    sc.set_instances(d2.instances)
    assert_frames_equal(one_oracle_frame(oracle, d2, W, H, blue_noise), one_frame(rt, sc, d2, W, H, blue_noise), "instanced after its update")
    # remove + add_mesh under the same key after updates still works
    sc.remove(7)
    sc.add_mesh(7, sphere.vertices, sphere.indices, sphere.material)
    d3 = with_vertices(d2, 7, sphere.vertices)
    sc.set_instances(d3.instances)
    assert_frames_equal(one_oracle_frame(oracle, d3, W, H, blue_noise), one_frame(rt, sc, d3, W, H, blue_noise), "remove + add after updates")
    sc.close()
    # an update before the first build
    sc = rt.Scene(0, instancing=form)
    for mm in desc.meshes:
        sc.add_mesh(mm.key, mm.vertices, mm.indices, mm.material)
    sc.update_mesh(7, mesh_of(d1, 7).vertices)
    sc.set_instances(d1.instances)
    assert sc.as_state()[1] == S
    assert_frames_equal(one_oracle_frame(oracle, d1, W, H, blue_noise), one_frame(rt, sc, d1, W, H, blue_noise), "update before the first build")
    sc.close()


@pytest.mark.parametrize("form", FORMS)
def test_update_cycles_do_not_grow_hbm(rt, form):
    """Free device memory is constant over 50 update + set_instances cycles, measured as the existing leak tests do. The heuristic
    runs free (updates and fast builds); the device fast build reserves its scratch when it first runs, at the ninth cycle, so ten
    cycles come first and the 50 after them are the ones measured."""
    import torch
    desc = scenes.instanced_field(10)
    sc = rt.Scene(0, instancing=form).load(desc)
    free = []
    for cycle in range(10 + 50):
        desc = scenes.deform(desc, [1, 5], float(cycle))
        push(sc, desc, [1, 5])
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    window = free[9:]                                         # the state after the tenth cycle, then 50 cycles
    assert len(window) == 51
    assert abs(window[-1] - window[0]) < (1 << 20) and max(window) - min(window) < (1 << 20), free
    sc.close()


# ---- Renderer ---------------------------------------------------------------------------------------------------------------
def test_renderer_update_mesh_equals_oracle_loop(rt, oracle):
    """Renderer.update_mesh between render_to_host_memory calls: 16 frames of the original, 16 of the first deformation, 16 of the
    second, one history; byte for byte the oracle's render loop with a fresh oracle scene per deformation."""
    desc = scenes.cornell_box()
    W, H = 96, 80
    noise = rt.default_noise_texture()
    r = rt.Renderer((W, H))
    for m in desc.meshes:
        r.load_mesh(m.key, m.vertices, m.indices, m.material)
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    of, prev, d = oracle.HostFrame(W, H, noise), None, desc
    for step in range(3):
        if step:
            d = scenes.deform(d, [7, 6], float(step))
            for k in (7, 6):
                r.update_mesh(k, mesh_of(d, k).vertices)
        img = r.render_to_host_memory(cam, d.instances)
        osc = oracle.OracleScene().load(d)
        for i in range(16):
            f = 16 * step + i
            om = oracle.camera_matrices(d.camera_pos, d.camera_target, d.fov_y, W, H, prev)
            prev = list(om.view_proj)
            osc.trace_ris(of, om, f); osc.trace_final(of, om, f); oracle.post_chain(of, f)
        osc.close()
        assert_bits_equal(of.output, img.view(np.uint32).reshape(-1), "render_to_host_memory after %d updates" % step)
    with pytest.raises(rt.SunrayError) as e:
        r.update_mesh(7, mesh_of(d, 7).vertices[:-1])
    assert e.value.code == ERR_INVALID_ARG
    r.close()


def test_multi_slot_renderer_update_mesh_equals_single_device(rt):
    """All slots on one GPU (rehearsal): update_mesh reaches every replica, with frames in flight (no wait before the update)."""
    from test_gpu_multi_renderer import assert_equal, grab, load
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.cornell_box()
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)

    def run(r):
        load(r, desc)
        out, d = [], desc
        for f in range(6):
            if f in (2, 3, 5):
                d = scenes.deform(d, [7], float(f))
                r.update_mesh(7, mesh_of(d, 7).vertices)        # the previous frame may still be in flight
            fr = r.render(cam, d.instances)
            if f in (1, 3, 5):
                r.wait_frame(fr)
                out.append(grab(rt, hip, r))
        return out
    single = rt.Renderer((96, 80))
    want = run(single)
    single.close()
    multi = rt.Renderer((96, 80), devices=[0, 0])
    got = run(multi)
    assert multi.history_overflow() == 0
    multi.close()
    for i, (a, b) in enumerate(zip(want, got)):
        assert_equal(a[0], b[0], "step %d output" % i)
        assert_equal(a[1], b[1], "step %d raw_color" % i)
    assert not np.array_equal(want[0][1], want[2][1])


# ---- regression guard --------------------------------------------------------------------------------------------------------
def test_transform_only_update_is_unchanged(rt, oracle, blue_noise):
    """No dirty mesh: the moving-instance sequence still takes the plain flatten (no reshading) and still equals the oracle."""
    desc = scenes.cornell_glass_mirror()
    seq = Sequence(rt, oracle, blue_noise, desc, 96, 72, "flat")
    seq.frame()
    for f in range(1, 5):
        seq.frame(dataclasses.replace(desc, instances=_moving_instances(desc, f)), [])
        info = seq.gsc.mesh_update_info()
        assert (info.dirty_meshes, info.reshaded) == (0, 0)
    assert seq.ops == [S] + [U] * 4
    seq.gsc.close()
