"""The frame's light table built on the device (Scene.set_light_table_build("device"): light_table_kernel and
emissive_positions_kernel of csrc/lights.hip). Every comparison runs two scenes through the same calls: scene A in host mode with
the host route (update_mesh), scene B in device mode with the device route (update_mesh_device / skin_mesh). Equal means bit for
bit; only the zero-area test admits NaN words whose payload differs. No other test's input holds a degenerate emissive triangle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from light_table_reference import affine, light_table as reference_light_table  # noqa: E402
from test_gpu_mesh_update import assert_frames_equal, mesh_of, one_frame  # noqa: E402
from test_gpu_mesh_update_device import (assert_scenes_equal, flags, ray_grid, refused, sphere_and_quad,  # noqa: E402
                                         to_device, traces)
from test_gpu_parity import assert_bits_equal  # noqa: E402

W, H = 80, 60
GLOW = dict(base_color=(1, 1, 1, 1), emissive_factor=(1.0, 0.9, 0.7), emissive_strength=12.0)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def strip(n, emissive=True, y=0.0):
    """A zigzag strip of n triangles (n + 2 vertices) whose vertices leave the plane, so that no triangle is degenerate and no two
    are alike; one emissive entry per triangle in index order."""
    i = np.arange(n + 2)
    pos = np.stack([0.25 * i, y + (i % 2) * 0.75 + 0.05 * np.sin(0.7 * i), 0.2 * np.cos(0.9 * i)], axis=1).astype(np.float32)
    v = scenes.make_vertices(pos, np.tile(np.array((0, 0, 1), dtype=np.float32), (n + 2, 1)))
    idx = np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], axis=1).ravel().astype(np.uint32)
    mat = abi.material(**GLOW) if emissive else abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    return v, idx, mat


def grey_quad(key):
    qv, qi = scenes.quad((-6, -1.5, 6), (6, -1.5, 6), (6, -1.5, -6), (-6, -1.5, -6), (0, 1, 0))
    return scenes.MeshDesc(key, qv, qi, abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5))


def strip_scene(n, n_inst, seed=3):
    s = scenes.SceneDesc("emissive_strip_%d_x%d" % (n, n_inst), camera_pos=(2.0, 1.0, 9.0), camera_target=(2.0, 0.0, 0.0))
    s.meshes.append(scenes.MeshDesc(1, *strip(n)))
    s.meshes.append(grey_quad(2))
    s.instances = [(1, list(affine(np.random.default_rng(seed + n), n_inst))), (2, [scenes.translate(0.0, 0.0, 0.0)])]
    return s


def lamp_keys(desc):
    instanced = {k for k, _ in desc.instances}
    return [m.key for m in desc.meshes if float(m.material["emissive_factor"][3]) > 0 and m.key in instanced]


def device_scene(rt, desc, form=None):
    return rt.Scene(0, instancing=form).set_light_table_build("device").load(desc)


def assert_lights_equal(a, b, what, on_device=True):
    """B's device table against A's, and against the numpy restatement over A's tables; B's info says where it was built."""
    la, lb = a.read_lights(), b.read_lights()
    ta = a.tables()
    assert la.shape == lb.shape == (ta["num_lights"], 16), (what, la.shape, lb.shape)
    assert_bits_equal(la, lb, "%s: lights" % what)
    want = reference_light_table(ta["transforms"], ta["indirection"], ta["emissive_triangles"])
    assert_bits_equal(want, lb, "%s: lights against the restatement" % what)
    ia, ib = a.light_table_info(), b.light_table_info()
    assert (ia.mode, ia.on_device) == (abi.LIGHTS_HOST, 0), what
    assert ib.on_device == (1 if on_device else 0) and ib.num_lights == ia.num_lights == len(lb) and ib.arena_entries == ia.arena_entries, what


def assert_tables_equal(a, b, what):
    ta, tb = a.tables(), b.tables()
    for name in ("transforms", "indirection", "emissive_triangles"):
        assert_bits_equal(ta[name], tb[name], "%s: table %s" % (what, name))
    assert ta["num_lights"] == tb["num_lights"], what


# ---- 1. table parity at the edges of a wave and a block -----------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["flat", "two_level"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_table_parity_at_wave_and_block_edges(rt, n, form):
    """Four lanes per light: 16 lights fill a wave, 64 a block. Strips of n emissive triangles, instanced once and three times."""
    for n_inst in (1, 3):
        desc = strip_scene(n, n_inst)
        a, b = rt.Scene(0, instancing=form).load(desc), device_scene(rt, desc, form)
        what = "%d triangles x %d, %s" % (n, n_inst, form)
        assert a.two_level() == b.two_level() == (form == "two_level")
        assert_lights_equal(a, b, what)
        info = b.light_table_info()
        assert (info.mode, info.num_lights, info.entries_uploaded, info.arena_uploads) == (abi.LIGHTS_DEVICE, n * n_inst, 1, 1), what
        assert np.isfinite(b.read_lights()).all() and (b.read_lights()[:, 3] > 0).all(), what
        assert_tables_equal(a, b, what)
        a.close(); b.close()


@pytest.mark.parametrize("name", ["cornell_box", "instanced_field"])
def test_table_parity_on_the_stock_scenes(rt, blue_noise, name):
    desc = scenes.cornell_box() if name == "cornell_box" else scenes.instanced_field(10)
    a, b = rt.Scene(0).load(desc), device_scene(rt, desc)
    assert_lights_equal(a, b, name)
    assert_tables_equal(a, b, name)
    assert_frames_equal(one_frame(rt, a, desc, W, H, blue_noise), one_frame(rt, b, desc, W, H, blue_noise), name)
    a.close(); b.close()


# ---- 2. the fetch is gone -----------------------------------------------------------------------------------------------------------
def test_emissive_mesh_updated_from_device_memory_never_visits_the_host(rt, blue_noise):
    """test_emissive_mesh_fetches_inside_the_call's scenario with scene B in device mode: no fetch of the vertices, in the call or
    in set_instances; the tables come back from the device arena in one read of 64 bytes per entry."""
    desc = scenes.instanced_field(10)
    lamp = lamp_keys(desc)[0]
    a, b = rt.Scene(0).load(desc), device_scene(rt, desc)
    assert len(a.tables()["emissive_triangles"]) == len(mesh_of(desc, lamp).indices) // 3 > 1
    f0 = one_frame(rt, b, desc, W, H, blue_noise)
    assert_frames_equal(one_frame(rt, a, desc, W, H, blue_noise), f0, "before the update")
    before_tables = a.tables()                                       # (B's are A's: test_table_parity_on_the_stock_scenes)
    assert b.light_table_info().arena_fetches == 0
    before_lights = b.read_lights()
    d1 = scenes.deform(desc, [lamp], 1.0)
    v = mesh_of(d1, lamp).vertices
    a.update_mesh(lamp, v)
    b.update_mesh_device(lamp, to_device(v, as_floats=True))
    assert flags(b, lamp) == (1, 1, 0)
    a.set_instances(d1.instances); b.set_instances(d1.instances)
    assert flags(b, lamp) == (1, 1, 0)
    info = b.light_table_info()
    assert (info.on_device, info.positions_rewritten, info.arena_uploads, info.entries_uploaded) == (1, len(mesh_of(desc, lamp).indices) // 3, 0, 0)
    assert_lights_equal(a, b, "after the emissive update")
    assert not np.array_equal(b.read_lights(), before_lights)
    ta, tb = a.tables(), b.tables()
    assert_bits_equal(ta["emissive_triangles"].view(np.uint32), tb["emissive_triangles"].view(np.uint32), "emissive triangles, w words included")
    assert_bits_equal(ta["indirection"], tb["indirection"], "emissive indirection")
    assert not np.array_equal(tb["emissive_triangles"], before_tables["emissive_triangles"])
    b.tables()
    assert flags(b, lamp) == (1, 1, 0)                               # the refresh is the arena's, counted on its own, once per frame
    assert b.light_table_info().arena_fetches == 1 and a.light_table_info().arena_fetches == 0
    fa, fb = one_frame(rt, a, d1, W, H, blue_noise), one_frame(rt, b, d1, W, H, blue_noise)
    assert_frames_equal(fa, fb, "a frame after the emissive update")
    assert not np.array_equal(fa[0], f0[0])
    assert flags(b, lamp) == (1, 1, 0)
    a.close(); b.close()


# ---- 3. skinned emissive mesh -------------------------------------------------------------------------------------------------------
def test_skinned_emissive_mesh_stays_on_the_device(rt):
    import skin_reference as ref
    from test_gpu_mesh_skin import FIXTURE_RAYS, fixture_scene
    desc, g, rigs = fixture_scene(rt, emissive=True)
    n_joints = len(g.skin(0)[1])
    a, b = rt.Scene(0, instancing="flat").load(desc), device_scene(rt, desc, "flat")
    for key, inf in rigs.items():
        b.set_mesh_skin(key, inf, n_joints)
    rays = ray_grid(*FIXTURE_RAYS)
    rd = rt.rays_to_device(rays)
    first = traces(rt, b, rays, rd)[0]
    for n in range(1, 4):
        joints = g.pose(0, 0.19 * n, 0)[1]
        for key, inf in rigs.items():
            a.update_mesh(key, ref.skin_model(desc.meshes[key - 1].vertices, inf, joints)[0])
            b.skin_mesh(key, joints)
            assert flags(b, key) == (1, 1, 0), (n, key)
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        what = "skinned emissive, step %d" % n
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2, 3, 4], what)
        assert_lights_equal(a, b, what)
        assert b.light_table_info().positions_rewritten == sum(len(desc.meshes[k - 1].indices) // 3 for k in rigs), what
        for key in rigs:
            assert flags(b, key) == (1, 1, 0), (n, key)
    assert not np.array_equal(first, traces(rt, b, rays, rd)[0])
    a.close(); b.close(); g.close()


# ---- 4. arena hazards ---------------------------------------------------------------------------------------------------------------
def test_arena_hazards_in_one_sequence(rt):
    """A slot whose newest positions exist only on the device is never overwritten by an older host value: a grown (reallocated)
    arena, freed slots taken by another mesh, a host update in the same frame as a device update, a switch back to host mode."""
    LAMP, OTHER, GROUND, B, Cc = 1, 2, 3, 10, 11
    lv, li = scenes.grid_patch((-1, 2.5, -1), (2, 0, 0), (0, 0, 2), 3, 2, (0, -1, 0), (1, 0, 0))
    ov, oi, omat = strip(9, y=1.0)
    desc = scenes.SceneDesc("arena_hazards", camera_pos=(1.0, 1.0, 8.0), camera_target=(1.0, 0.5, 0.0))
    desc.meshes = [scenes.MeshDesc(LAMP, lv, li, abi.material(**GLOW)), scenes.MeshDesc(OTHER, ov, oi, omat), grey_quad(GROUND)]
    base = [(LAMP, [scenes.translate(0, 0, 0), scenes.rotate_y(0.5, 2.0, 0.3, -1.0, 0.7)]), (OTHER, [scenes.translate(-1.0, 0.0, 0.5)]),
            (GROUND, [scenes.translate(0, 0, 0)])]
    desc.instances = base
    a, b = rt.Scene(0).load(desc), device_scene(rt, desc)
    n_lamp = len(li) // 3

    def compare(what, on_device=True):
        assert_lights_equal(a, b, what, on_device)
        assert_tables_equal(a, b, what)

    compare("loaded")
    # 1-3. device-update the lamp, then add B: the arena grows and the device arena is reallocated from the host's older values
    v1 = scenes.deform_vertices(lv, li, 1.0)
    a.update_mesh(LAMP, v1); b.update_mesh_device(LAMP, to_device(v1))
    bv, bi, bmat = strip(5, y=2.0)
    for s in (a, b):
        s.add_mesh(B, bv, bi, bmat)
    inst = base + [(B, [scenes.translate(0.5, 0.0, -0.5)])]
    a.set_instances(inst); b.set_instances(inst)
    info = b.light_table_info()
    assert (info.arena_uploads, info.positions_rewritten, info.entries_uploaded) == (1, n_lamp, 1)
    compare("lamp updated, B added")
    # a frame with nothing new: the lamp's slots are rewritten only when something put older values in them
    a.set_instances(inst); b.set_instances(inst)
    info = b.light_table_info()
    assert (info.arena_uploads, info.positions_rewritten, info.entries_uploaded) == (0, 0, 0)
    compare("a quiet frame")
    # 4-6. remove B, add C of another size (B's freed slots are taken, the arena grows again); a host update of another emissive
    # mesh in the same frame as a second device update of the lamp
    cv, ci, cmat = strip(7, y=-0.5)
    for s in (a, b):
        s.remove(B)
        s.add_mesh(Cc, cv, ci, cmat)
    o2 = scenes.deform_vertices(ov, oi, 2.0)
    v2 = scenes.deform_vertices(lv, li, 2.0)
    a.update_mesh(OTHER, o2); b.update_mesh(OTHER, o2)
    a.update_mesh(LAMP, v2); b.update_mesh_device(LAMP, to_device(v2))
    inst = base + [(Cc, [scenes.translate(-0.5, 0.0, 1.0), scenes.translate(1.5, 0.5, 1.0)])]
    a.set_instances(inst); b.set_instances(inst)
    info = b.light_table_info()
    assert (info.arena_uploads, info.positions_rewritten, info.entries_uploaded) == (1, n_lamp, 1)
    assert info.arena_entries == n_lamp + 9 + 7
    compare("B removed, C added, host and device updates in one frame")
    # C sits in B's freed slots in reverse order and two new ones: the slot list of the positions kernel is arbitrary
    c1 = scenes.deform_vertices(cv, ci, 1.0)
    a.update_mesh(Cc, c1); b.update_mesh_device(Cc, to_device(c1))
    a.set_instances(inst); b.set_instances(inst)
    info = b.light_table_info()
    assert (info.arena_uploads, info.positions_rewritten, info.entries_uploaded) == (0, 7, 0)
    compare("C updated from device memory")
    # 7-8. back to host mode: the host arena takes the lamp's slots from the device arena, not from the vertices
    b.set_light_table_build("host")
    a.set_instances(inst); b.set_instances(inst)
    compare("switched to host mode", on_device=False)
    assert b.light_table_info().mode == abi.LIGHTS_HOST
    fetches = flags(b, LAMP)[2]
    # and from here on the host route's rule holds: a device update of an emissive mesh fetches inside the call
    v3 = scenes.deform_vertices(lv, li, 3.0)
    a.update_mesh(LAMP, v3); b.update_mesh_device(LAMP, to_device(v3))
    assert flags(b, LAMP) == (0, 1, fetches + 1)
    a.set_instances(inst); b.set_instances(inst)
    compare("a device update in host mode", on_device=False)
    a.close(); b.close()


# ---- 5. instances only move ---------------------------------------------------------------------------------------------------------
def test_entries_are_uploaded_once_while_only_instances_move(rt):
    desc = strip_scene(70, 3)
    a, b = rt.Scene(0), rt.Scene(0).set_light_table_build("device")
    for s in (a, b):
        for m in desc.meshes:
            s.add_mesh(m.key, m.vertices, m.indices, m.material)
    for step in range(5):
        inst = [(1, list(affine(np.random.default_rng(100 + step), 3))), (2, [scenes.translate(0.0, -0.1 * step, 0.0)])]
        a.set_instances(inst); b.set_instances(inst)
        info = b.light_table_info()
        assert (info.on_device, info.entries_uploaded, info.arena_uploads, info.positions_rewritten) == (1, 1 if step == 0 else 0, 1 if step == 0 else 0, 0), step
        assert_lights_equal(a, b, "step %d" % step)
    a.close(); b.close()


# ---- 6. a caller's emissive list ----------------------------------------------------------------------------------------------------
def test_callers_emissive_list_is_used_as_given(rt):
    gv, gi = scenes.grid_patch((-1, 1, -1), (2, 0, 0), (0, 0, 2), 2, 2, (0, -1, 0), (1, 0, 0))
    em = np.zeros(3, dtype=abi.EMISSIVE_TRIANGLE)                       # three entries for eight triangles, with w words of their own
    rng = np.random.default_rng(9)
    for k in ("v0", "v1", "v2"):
        em[k] = rng.uniform(-1.0, 1.0, (3, 4)).astype(np.float32)
    em["emission"] = rng.uniform(1.0, 9.0, (3, 4)).astype(np.float32)
    ground = grey_quad(2)
    inst = [(1, list(affine(np.random.default_rng(4), 2))), (2, [scenes.translate(0, 0, 0)])]
    a, b = rt.Scene(0), rt.Scene(0).set_light_table_build("device")
    for s in (a, b):
        s.add_blas(1, gv, gi, abi.material(**GLOW), em)
        s.add_mesh(ground.key, ground.vertices, ground.indices, ground.material)
        s.set_instances(inst)
    assert_lights_equal(a, b, "caller's list")
    assert_tables_equal(a, b, "caller's list")
    assert len(b.read_lights()) == 6
    code, text = refused(rt, b, lambda: b.update_mesh_device(1, to_device(gv)))
    assert (code, text) == (-5, "update_mesh: the mesh was loaded with emissive triangles that are not one per triangle")
    a.close(); b.close()


# ---- 7. no emissive mesh ------------------------------------------------------------------------------------------------------------
def test_scene_without_lights_keeps_the_hosts_dummy_record(rt, blue_noise):
    desc = sphere_and_quad()
    desc.camera_pos, desc.camera_target = (0.0, 1.0, 7.0), (0.0, 0.0, 0.0)
    a, b = rt.Scene(0).load(desc), device_scene(rt, desc)
    la, lb = a.read_lights(), b.read_lights()
    assert la.shape == (1, 16) and la.tobytes() == lb.tobytes()          # 64 bytes, the NaN normals of 0 * inf included
    assert np.isnan(la[0, [7, 11, 15]]).all()
    info = b.light_table_info()
    assert (info.mode, info.on_device, info.num_lights, info.arena_entries) == (abi.LIGHTS_DEVICE, 0, 1, 0)
    assert_tables_equal(a, b, "no lights")
    assert_frames_equal(one_frame(rt, a, desc, W, H, blue_noise), one_frame(rt, b, desc, W, H, blue_noise), "no lights")
    a.close(); b.close()


# ---- 8. a zero-area emissive triangle -----------------------------------------------------------------------------------------------
def test_zero_area_triangle_has_nan_normals_on_both(rt):
    """Triangle 1 of the strip has two vertices in one place: cross = 0, length = 0, 1 / 0 = inf, 0 * inf = NaN. Words that are no
    NaN on the host are equal bit for bit; a NaN on the host is a NaN on the device, sign and payload left to each machine."""
    v, idx, mat = strip(5)
    v["position"][3] = v["position"][2]
    desc = scenes.SceneDesc("zero_area")
    desc.meshes = [scenes.MeshDesc(1, v, idx, mat), grey_quad(2)]
    desc.instances = [(1, list(affine(np.random.default_rng(2), 2))), (2, [scenes.translate(0, 0, 0)])]
    a, b = rt.Scene(0).load(desc), device_scene(rt, desc)
    la, lb = a.read_lights(), b.read_lights()
    nan = np.isnan(la)
    assert nan.sum() >= 3 * 2 and (la[:, 3] == 0).sum() >= 2             # at least triangle 1 of both instances
    assert b.light_table_info().on_device == 1
    print("NaN words, host:", sorted({hex(x) for x in la.view(np.uint32)[nan]}), "device:", sorted({hex(x) for x in lb.view(np.uint32)[nan]}))
    assert np.isnan(lb[nan]).all()
    assert np.array_equal(la.view(np.uint32)[~nan], lb.view(np.uint32)[~nan])
    a.close(); b.close()


# ---- 9. Renderer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one slot", "two slots on one GPU"])
def test_renderer_in_device_mode_equals_the_host_route(rt, devices):
    from test_gpu_multi_renderer import assert_equal, grab, load
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.cornell_box()
    lamp = lamp_keys(desc)[0]
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)
    n_slots = len(devices) if devices else 1

    def run(device_route):
        r = rt.Renderer((64, 48), devices=devices)
        if device_route:
            r.set_light_table_build("device")
        load(r, desc)
        out = []
        for f in range(4):
            v = scenes.deform_vertices(mesh_of(desc, lamp).vertices, mesh_of(desc, lamp).indices, 1.0 + f, amplitude=0.3)
            if device_route:
                r.update_mesh_device(lamp, to_device(v))
            else:
                r.update_mesh(lamp, v)
            fr = r.render(cam, desc.instances)
            r.wait_frame(fr)
            out.append(grab(rt, hip, r)[0])
            for slot in range(n_slots):
                info = r.light_table_info(slot)
                assert (info.mode, info.on_device) == ((abi.LIGHTS_DEVICE, 1) if device_route else (abi.LIGHTS_HOST, 0)), (f, slot)
                if device_route:               # the first frame's quality build reads the host copy; the updates in place never do
                    assert info.positions_rewritten == 2 and flags(r.replica_scene(slot), lamp) == ((0, 1, 1) if f == 0 else (1, 1, 1)), (f, slot)
        r.close()
        return out
    want, got = run(False), run(True)
    for f, (x, y) in enumerate(zip(want, got)):
        assert_equal(x, y, "%d slot(s), frame %d output" % (n_slots, f))
    assert not np.array_equal(want[0], want[3])
