"""Scene.pose_meshes / Renderer.pose_meshes / Renderer.set_pose_batch (sr_scene_pose_meshes: many skinned and morphed meshes posed
by one upload, one launch of pose_batch_kernel and one read-back; Scene.skin_mesh and Scene.pose_mesh are batches of one item on
the same path). The references are tests/skin_reference.py and tests/morph_reference.py, the header's arithmetic restated in numpy
float32; a twin scene posed mesh by mesh with pose_mesh runs the same kernel and shows only that the book-keeping agrees. Equal
means byte for byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_reference as mref  # noqa: E402
import skin_reference as sref  # noqa: E402
from test_gpu_mesh_morph import FIXTURE as MORPH_FIXTURE, fixture_scene, model_pose, targets, weight_sets  # noqa: E402
from test_gpu_mesh_skin import (FIXTURE as SKIN_FIXTURE, _hash01, assert_records_equal, device_vertices, matrices, rig,  # noqa: E402
                                rigged_meshes)
from test_gpu_mesh_update_device import ERR_INVALID_ARG, assert_scenes_equal, flags, ray_grid, refused, traces, update_counts  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402

NONE = 0xFFFFFFFF
N_TARGETS, N_JOINTS = 5, 7
# the batch: (key, morph stage, skin stage) in an order that is not the slot order; meshes 2 (4 vertices) and 4 (64) are left out.
# Key 8 has exactly 256 vertices, so key 9's first block is the very next one; key 9 (512) ends on a tile boundary too.
ITEMS = ((8, True, True), (9, False, True), (1, False, True), (7, True, True), (3, True, False), (6, True, False), (5, True, True))
LEFT_OUT = (2, 4)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def hip():
    return C.CDLL("libamdhip64.so")


# ---- the mesh set, its rigs, targets and models: made once, never written afterwards ------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_set():
    """rigged_meshes() (3, 4, 63, 64, 65, 257, 1026 vertices, keys 1..7) and, made to count in the same way, meshes of exactly 256
    and 512 vertices (keys 8, 9) -> (desc, {key: (deltas, influences)})."""
    desc = rigged_meshes()
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    for key, (nu, nv) in ((8, (15, 15)), (9, (15, 31))):
        v, idx = scenes.grid_patch((-1, -1, 0), (2, 0, 0), (0, 2, 0), nu, nv, (0, 0, 1), (1, 0, 0))
        i = np.arange(len(v))
        t = np.stack([_hash01(i, 1) - 0.5, _hash01(i, 2) - 0.5, _hash01(i, 3) + 0.25], axis=1).astype(np.float32)
        v["tangent"][:, :3] = t / np.sqrt((t * t).sum(axis=1, dtype=np.float32))[:, None]
        v["tangent"][:, 3] = np.where(i % 3 == 0, -1.0, 1.0)
        for k, name in enumerate(("base_color", "metallic_roughness", "normal", "occlusion", "emissive")):
            v[name + "_tex_coord"] = np.stack([_hash01(i, 10 + k), _hash01(i, 20 + k)], axis=1)
        w = v.view(np.uint32).reshape(len(v), -1)
        w[:, 3], w[:, 7], w[:, 22], w[:, 23] = 0x7FC00000 + i, 0xFF800000, 0xDEADBEEF, i
        v["normal"][i % 29 == 5] = 0.0
        v["tangent"][i % 31 == 7, :3] = 0.0
        desc.meshes.append(scenes.MeshDesc(key, v, idx, grey))
        desc.instances.append((key, [scenes.translate(3.0 * (key - 1), 0.0, 0.0)]))
    assert [len(m.vertices) for m in desc.meshes] == [3, 4, 63, 64, 65, 257, 1026, 256, 512]
    data = {m.key: (targets(m.vertices, N_TARGETS, 3 * k), rig(len(m.vertices), N_JOINTS, k)) for k, m in enumerate(desc.meshes)}
    return desc, data


def pose_of(step):
    """The weights and joint matrices of animation step `step` (1, 2, ...): every step another pose; joint 1 stays all NaN."""
    w = (weight_sets(N_TARGETS)["negative and above 1"] * np.float32(0.25 * step)).astype(np.float32)
    M = matrices(N_JOINTS)
    M[:, :, 3] += np.float32(0.03125 * (step - 1))
    return w, M


@functools.lru_cache(maxsize=None)
def models(step=1):
    """{key: the model's posed vertices of item `key` at `step`}: morph_model, skin_model or skin_model(morph_model)."""
    desc, data = mesh_set()
    w, M = pose_of(step)
    out = {}
    for key, morph, skin in ITEMS:
        v, (d, inf) = desc.meshes[key - 1].vertices, data[key]
        if morph:
            v, bad, _ = mref.morph_model(v, d, w)
            assert bad is None
        if skin:
            v, bad, _ = sref.skin_model(v, inf, M)
            assert bad is None
        out[key] = v
    return out


def batch_items(step=1, matrices_of=None):
    w, M = pose_of(step)
    return [(key, w if morph else None, (matrices_of or {}).get(key, M) if skin else None) for key, morph, skin in ITEMS]


def rigged_scene(rt, **kw):
    """An empty scene, the mesh set and its (deltas, influences) by key; attach() gives every loaded mesh both."""
    desc, data = mesh_set()
    sc = rt.Scene(0, **kw)
    return sc, desc, data


def attach(sc, desc, data):
    for m in desc.meshes:
        d, inf = data[m.key]
        sc.set_mesh_skin(m.key, inf, N_JOINTS)
        sc.set_mesh_morph(m.key, d)


def pose_infos(sc, keys):
    out = []
    for k in keys:
        mi, si = sc.mesh_morph_info(k), sc.mesh_skin_info(k)
        out.append((k, mi.n_targets, mi.posed, mi.n_active, mi.first_bad, si.n_joints, si.skinned, si.first_bad))
    return out


def all_bytes(hip, sc, desc):
    return [device_vertices(hip, sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)]


def info_tuple(i, times=False):
    t = (i.items, i.blocks, i.vertices, i.morph_only, i.skin_only, i.fused, i.launches, i.read_backs, i.calls, i.refused_item, i.refused_vertex, i.upload_bytes)
    return t + ((i.pose_ms, i.scatter_ms, i.host_ms) if times else ())


def align16(n):
    return (n + 15) & ~15


# ---- 1. bytes, 7. info ---------------------------------------------------------------------------------------------------------------
def test_batch_equals_the_models_and_the_per_mesh_twin(rt, hip):
    sc, desc, data = rigged_scene(rt)
    twin = rt.Scene(0)
    for s in (sc, twin):
        s.load(desc)
        attach(s, desc, data)
    keys = [m.key for m in desc.meshes]
    assert pose_of(1)[0].all() and np.isnan(pose_of(1)[1][1]).all()         # every target is active; the NaN matrix only zero weights name
    sc.pose_meshes(batch_items())
    for key, w, M in batch_items():
        twin.pose_mesh(key, w, M)
    want = models()
    for slot, m in enumerate(desc.meshes):
        got, by_twin = device_vertices(hip, sc, slot, len(m.vertices)), device_vertices(hip, twin, slot, len(m.vertices))
        if m.key in LEFT_OUT:
            assert got.tobytes() == m.vertices.tobytes() and flags(sc, m.key) == (0, 0, 0), m.key
            continue
        stages = [it for it in ITEMS if it[0] == m.key][0]
        assert_records_equal(got, want[m.key], "item of key %d (%d vertices, morph %s, skin %s) against the model" % ((m.key, len(got)) + stages[1:]))
        assert_records_equal(got, by_twin, "item of key %d against pose_mesh" % m.key)
        assert got.tobytes() != m.vertices.tobytes()
        assert flags(sc, m.key) == flags(twin, m.key) == (1, 1, 0)
    assert pose_infos(sc, keys) == pose_infos(twin, keys)
    assert [p[2:4] + p[6:] for p in pose_infos(sc, [8, 9, 3])] == [(1, N_TARGETS, 1, NONE), (0, 0, 1, NONE), (1, N_TARGETS, 0, NONE)]
    # the figures of the call against the plan and the item list
    counts = [len(desc.meshes[key - 1].vertices) for key, _, _ in ITEMS]
    first, base, blocks = rt.pose_batch_plan(counts)
    assert list(first) == [0, 1, 3, 4, 9, 10, 12] and blocks == 13 and int(base[-1]) + counts[-1] == sum(counts)
    n_active = N_TARGETS * sum(1 for _, morph, _ in ITEMS if morph)
    upload = 64 * len(ITEMS) + align16(4 * blocks) + 48 * N_JOINTS * sum(1 for _, _, skin in ITEMS if skin) + 2 * align16(4 * n_active)
    info = sc.pose_batch_info()
    assert info_tuple(info) == (len(ITEMS), blocks, sum(counts), 2, 2, 3, 2, 1, 1, NONE, NONE, upload), info_tuple(info)
    assert (info.pose_ms, info.scatter_ms) == (0.0, 0.0) and info.host_ms > 0.0          # timing is off
    # and the structures built from either scene are the same
    rays = ray_grid((-1.5, -1.5), (3.0 * 8 + 1.5, 1.5), 160, 24)
    rd = rt.rays_to_device(rays)
    sc.set_instances(desc.instances); twin.set_instances(desc.instances)
    assert_scenes_equal(rt, twin, sc, rays, rd, keys, "after one batch")
    sc.close(); twin.close()


# ---- 2. all or nothing ------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_item_refuses_the_whole_batch(rt, hip):
    sc, desc, data = rigged_scene(rt)
    sc.load(desc)
    attach(sc, desc, data)
    sc.set_instances(desc.instances)
    sc.pose_meshes(batch_items())
    sc.set_instances(desc.instances)
    keys = [m.key for m in desc.meshes]
    w, M = pose_of(2)
    bad_M = M.copy()
    bad_M[N_JOINTS - 1, 1, 3] = np.inf            # the last joint is used by every rig
    worst = {}
    for key, morph, skin in ITEMS:
        v, (d, inf) = desc.meshes[key - 1].vertices, data[key]
        if skin:
            worst[key] = sref.skin_model(mref.morph_model(v, d, w)[0] if morph else v, inf, bad_M)[1]
    assert None not in (worst[7], worst[9], worst[5])

    def state():
        u = sc.mesh_update_info()
        return (all_bytes(hip, sc, desc), tuple(getattr(u, f[0]) for f in u._fields_), [p[:4] + p[5:7] for p in pose_infos(sc, keys)],
                [flags(sc, k) for k in keys], bytes(sc.as_state()[0]), sc.as_state()[1], update_counts(sc))
    before = state()
    cases = (("a middle item", {7: bad_M}, 3, 7), ("two items, the lower index is named", {7: bad_M, 5: bad_M}, 3, 7),
             ("two items, the other order of keys", {9: bad_M, 7: bad_M}, 1, 9))
    for n, (what, bad_of, item, key) in enumerate(cases):
        got = refused(rt, sc, lambda: sc.pose_meshes(batch_items(2, bad_of)))
        assert got == (ERR_INVALID_ARG, "pose_meshes: item %d: update_mesh: vertex %d has a non-finite position" % (item, worst[key])), (what, got)
        assert state() == before, what
        info = sc.pose_batch_info()
        assert (info.launches, info.read_backs, info.calls, info.refused_item, info.refused_vertex) == (1, 1, 2 + n, item, worst[key]), what
        for k in bad_of:
            assert sc.mesh_skin_info(k).first_bad == worst[k], (what, k)
    # the next good batch is taken as if nothing had happened
    sc.pose_meshes(batch_items(2))
    for slot, m in enumerate(desc.meshes):
        if m.key not in LEFT_OUT:
            assert_records_equal(device_vertices(hip, sc, slot, len(m.vertices)), models(2)[m.key], "key %d after the refusals" % m.key)
    assert [p[2] for p in pose_infos(sc, [8, 7])] == [2, 2] and sc.mesh_skin_info(7).first_bad == NONE
    sc.close()


# ---- 3. refusals decided on the host ----------------------------------------------------------------------------------------------------
def test_host_refusals_come_before_any_device_work(rt, hip):
    from sunray_amd._lib import lib
    sc, desc, data = rigged_scene(rt)
    sc.load(desc)
    sc.set_mesh_skin(1, data[1][1], N_JOINTS)            # key 1: a skin alone; key 3: a morph alone; key 5: both
    sc.set_mesh_morph(3, data[3][0])
    sc.set_mesh_skin(5, data[5][1], N_JOINTS); sc.set_mesh_morph(5, data[5][0])
    w, M = pose_of(1)
    sc.pose_meshes([(5, w, M)])
    before, bytes_before = info_tuple(sc.pose_batch_info(), times=True), all_bytes(hip, sc, desc)
    assert before[6] == 2 and before[8] == 1
    nan_w = w.copy()
    nan_w[3] = np.nan
    good = (5, w, M)
    cases = {
        "an unknown key": ([good, (99, w, None)], "pose_meshes: item 1: pose_mesh: no mesh is registered under this key"),
        "an unknown key, skin stage alone": ([(99, None, M)], "pose_meshes: item 0: skin_mesh: no mesh is registered under this key"),
        "no morph": ([good, (3, w, None), (1, w, M)], "pose_meshes: item 2: pose_mesh: the mesh has no morph targets (sr_scene_set_mesh_morph attaches them)"),
        "another number of weights": ([(3, w[:4], None)], "pose_meshes: item 0: pose_mesh: 4 weights given, the morph was attached with 5 targets"),
        "no skin": ([good, (3, w, M)], "pose_meshes: item 1: pose_mesh: the mesh has no skin (sr_scene_set_mesh_skin attaches one)"),
        "no skin, skin stage alone": ([(3, None, M)], "pose_meshes: item 0: skin_mesh: the mesh has no skin (sr_scene_set_mesh_skin attaches one)"),
        "another number of joints": ([good, (1, None, M[:3])], "pose_meshes: item 1: skin_mesh: 3 joint matrices given, the skin was attached with 7 joints"),
        "a weight that is not finite": ([(3, w, None), (5, nan_w, M)], "pose_meshes: item 1: pose_mesh: weight 3 is not finite"),
        "a key named twice": ([good, (3, w, None), (5, None, M)], "pose_meshes: item 2: the key is named twice in the batch (first by item 0)"),
    }
    for what, (items, text) in cases.items():
        got = refused(rt, sc, lambda: sc.pose_meshes(items))
        assert got == (ERR_INVALID_ARG, text), (what, got)
        assert info_tuple(sc.pose_batch_info(), times=True) == before, what
    # what the Python layer never passes on: NULL items, an item with neither stage, a NULL scene
    rows, n, keep = rt._pose_items([good, (3, w, None)])
    rows[1].weights = None
    for what, call, text in (("null items", lambda: lib().sr_scene_pose_meshes(sc._h, None, C.c_uint32(2), None), "pose_meshes: null argument (items, with n_items > 0)"),
                             ("neither stage", lambda: lib().sr_scene_pose_meshes(sc._h, rows, n, None),
                              "pose_meshes: item 1: pose_mesh: neither weights nor joint matrices given (one stage at least)"),
                             ("null scene", lambda: lib().sr_scene_pose_meshes(None, rows, n, None), "pose_meshes: null argument (the scene)")):
        assert call() == ERR_INVALID_ARG and lib().sr_last_error().decode() == text, (what, lib().sr_last_error())
        assert info_tuple(sc.pose_batch_info(), times=True) == before, what
    sc.pose_meshes([])                                   # n_items == 0: accepted, nothing happens
    assert lib().sr_scene_pose_meshes(sc._h, None, C.c_uint32(0), None) == 0
    assert info_tuple(sc.pose_batch_info(), times=True) == before and all_bytes(hip, sc, desc) == bytes_before
    assert pose_infos(sc, [5])[0][2:4] + pose_infos(sc, [5])[0][6:] == (1, N_TARGETS, 1, NONE)
    sc.close()


def assert_answers_equal(rt, a, b, rays, rd, what):
    """What assert_scenes_equal compares apart from the node and leaf arrays: from a device fast build on, node numbers come from
    atomic counters (test_gpu_mesh_tree_batch.py), so two builds of the same vertices differ in numbering and in nothing a ray sees."""
    ta, tb = a.tables(), b.tables()
    for name in ("transforms", "indirection", "emissive_triangles"):
        assert_bits_equal(ta[name], tb[name], "%s: table %s" % (what, name))
    assert_bits_equal(a.read_top_level()[3], b.read_top_level()[3], "%s: top-level boxes" % what)
    (ha, oa), (hb, ob) = traces(rt, a, rays, rd), traces(rt, b, rays, rd)
    assert (ha.view(abi.HIT)["t"] >= 0).mean() > 0.03, what
    assert_bits_equal(ha, hb, "%s: closest hits" % what)
    assert_bits_equal(oa, ob, "%s: occlusion" % what)
    assert update_counts(a) == update_counts(b), what


# ---- 4. downstream ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one-level", "two-level, rapidly changing, batched tree build"])
def test_structures_after_a_batch_equal_those_of_the_same_vertices(rt, form):
    """Scene A takes the models' vertices through update_mesh, scene B the same poses through one pose_meshes a step: structure,
    tables, closest-hit and any-hit traces and counts are equal bit for bit (assert_scenes_equal). In the two-level form the steps
    cross refits and the fast build of the ninth update, from which on the node arrays are left out (assert_answers_equal). After the last step a scene that loads the posed vertices fresh answers
    the rays alike: the same distances and the same occlusion bits."""
    two_level = form != "one-level"
    desc, data = mesh_set()
    posed_keys = [key for key, _, _ in ITEMS]
    pair = []
    for _ in range(2):
        sc = rt.Scene(0, instancing="two_level" if two_level else "flat")
        if two_level:
            sc.set_mesh_tree_build("device")
            sc.set_mesh_tree_batch("on")
        sc.load(desc)
        for key in posed_keys if two_level else ():
            sc.set_mesh_build_type(key, abi.BUILD_RAPIDLY_CHANGING)
        pair.append(sc)
    a, b = pair
    attach(b, desc, data)
    rays = ray_grid((-1.5, -1.5), (3.0 * 8 + 1.5, 1.5), 160, 24)
    rd = rt.rays_to_device(rays)
    for s in pair:
        s.set_instances(desc.instances)
    first = traces(rt, b, rays, rd)[0]
    steps = 10 if two_level else 3
    for n in range(1, steps + 1):
        for key in posed_keys:
            a.update_mesh(key, models(n)[key])
        b.pose_meshes(batch_items(n))
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        what = "%s, step %d" % (form, n)
        if two_level and n >= 9:
            assert_answers_equal(rt, a, b, rays, rd, what)
        else:
            assert_scenes_equal(rt, a, b, rays, rd, [m.key for m in desc.meshes], what)
        counts = update_counts(b)
        print(what, counts)
        if two_level:          # refitted while the state asks for updates, built anew after more than 8 of them
            assert counts[2:4] == ((len(ITEMS), 0) if n == 9 else (0, len(ITEMS))), (what, counts)
    last = traces(rt, b, rays, rd)
    assert not np.array_equal(first, last[0])
    fresh_desc = scenes.SceneDesc("posed")
    for m in desc.meshes:
        fresh_desc.meshes.append(scenes.MeshDesc(m.key, models(steps).get(m.key, m.vertices), m.indices, m.material))
    fresh_desc.instances = desc.instances
    fresh = rt.Scene(0, instancing="two_level" if two_level else "flat").load(fresh_desc)
    fresh.set_instances(desc.instances)
    hits, occluded = traces(rt, fresh, rays, rd)
    assert_bits_equal(np.ascontiguousarray(hits.view(abi.HIT)["t"]).view(np.uint32), np.ascontiguousarray(last[0].view(abi.HIT)["t"]).view(np.uint32),
                      form + ": hit distances of a fresh load")
    assert_bits_equal(occluded, last[1], form + ": occlusion of a fresh load")
    a.close(); b.close(); fresh.close()


# ---- 5. lights ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights", ["host", "device"])
def test_emissive_meshes_in_a_batch(rt, lights):
    """The morph fixture with its two morphed meshes emissive (mesh 1 morphs and skins, mesh 2 morphs), posed by one pose_meshes a step
    against a twin posed by pose_mesh: the light tables are equal bit for bit, and under the device table nothing is fetched."""
    desc, g, morphs = fixture_scene(rt, emissive=True)
    n_joints = len(g.skin(0)[1])
    pair = []
    for _ in range(2):
        sc = rt.Scene(0, instancing="flat").set_light_table_build(lights)
        sc.load(desc)
        for key, (d, inf) in morphs.items():
            sc.set_mesh_morph(key, d)
            if inf is not None:
                sc.set_mesh_skin(key, inf, n_joints)
        sc.set_instances(desc.instances)
        pair.append(sc)
    a, b = pair
    rest = b.read_lights().copy()
    for n in (1, 2):
        items = []
        for key in morphs:
            _, w, joints = model_pose(desc, g, morphs, key, 0.19 * n)
            a.pose_mesh(key, w, joints)
            items.append((key, w, joints))
        b.pose_meshes(items[::-1])
        for key in morphs:
            assert flags(b, key) == flags(a, key) == ((1, 1, 0) if lights == "device" else (0, 1, n)), (lights, n, key)
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        la, lb = a.read_lights(), b.read_lights()
        assert len(lb) > 392 and la.shape == lb.shape
        assert_bits_equal(la, lb, "%s lights, step %d" % (lights, n))
        assert_bits_equal(a.tables()["emissive_triangles"], b.tables()["emissive_triangles"], "%s lights, step %d: the arena" % (lights, n))
        assert b.light_table_info().on_device == (1 if lights == "device" else 0)
    assert not np.array_equal(rest, b.read_lights())
    a.close(); b.close(); g.close()


# ---- 6. the facade ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture", [SKIN_FIXTURE, MORPH_FIXTURE], ids=["skinned_bar", "morph_bar"])
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one slot", "two slots on one GPU"])
def test_pose_scene_with_the_batch_equals_pose_scene_without(rt, hip, devices, fixture):
    from test_gpu_multi_renderer import assert_equal, grab
    cam = ((0.8, 1.4, 7.0), (0.8, 1.0, 0.0), 45.0)
    times = [0.3, 0.9, 1.45]

    def run(batch):
        r = rt.Renderer((64, 48), devices=devices)
        r.set_pose_batch(batch)
        g = rt.Gltf(fixture)
        loaded = r.load_scene(g)
        keys = [int(k) for k in loaded.keys]
        sizes = [len(b["vertices"]) for b in rt.gltf_parse(fixture)["blases"]]
        r.attach_skins(g, loaded)
        r.attach_morphs(g, loaded)
        out = []
        for t in times:
            fr = r.render(cam, r.pose_scene(g, loaded, 0, t))
            r.wait_frame(fr)
            out.append(grab(rt, hip, r))
        first = r.replica_scene(0)
        posed = [k for k in keys if first.mesh_skin_info(k).skinned + first.mesh_morph_info(k).posed > 0]
        info = first.pose_batch_info()
        assert len(posed) >= 1 and (info.calls, info.items) == ((len(times), len(posed)) if batch else (0, 0))
        for k in posed:
            assert first.mesh_skin_info(k).skinned + first.mesh_morph_info(k).posed in (len(times), 2 * len(times))
        if devices:
            replica = r.replica_scene(1)
            assert replica.pose_batch_info().calls == 0                      # the first slot's scene poses, once
            for slot, k in enumerate(keys):
                assert device_vertices(hip, replica, slot, sizes[slot]).tobytes() == device_vertices(hip, first, slot, sizes[slot]).tobytes(), k
                assert flags(replica, k)[1] == (1 if k in posed else 0)
        assert r.history_overflow() == 0
        loaded.close(); g.close(); r.close()
        return out
    want, got = run(False), run(True)
    for f, ((xo, xr), (yo, yr)) in enumerate(zip(want, got)):
        assert_equal(xr, yr, "frame %d raw_color" % f)
        assert_equal(xo, yo, "frame %d output" % f)
    assert min((x[0] & 0xFFFFFF != 0).mean() for x in want) > 0.05
    assert not np.array_equal(want[0][0], want[2][0])


# ---- 8. the single entry points are batches of one -------------------------------------------------------------------------------------------
EDGE_SIZES = (3, 255, 256, 257, 513)            # below a tile, one short of it, exactly one, one over, one over two


@functools.lru_cache(maxsize=None)
def edge_meshes():
    """Meshes of EDGE_SIZES vertices, keys 1..5, made as test_gpu_mesh_morph.base_meshes makes its own (scattered positions, unit
    normals and tangents, uv sets, pad canaries; the triangles (i, i + 1, i + 2)), with two morph targets and a rig of two joints
    each -> (desc, {key: (deltas, influences)})."""
    desc = scenes.SceneDesc("tile_edges")
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    for k, n in enumerate(EDGE_SIZES, start=1):
        i = np.arange(n)
        v = np.zeros(n, dtype=abi.VERTEX)
        v["position"] = np.stack([_hash01(i, 31 + k) * 2 - 1, _hash01(i, 32 + k) * 2 - 1, _hash01(i, 33 + k) - 0.5], axis=1)
        for name, salt in (("normal", 40), ("tangent", 50)):
            d = np.stack([_hash01(i, salt) - 0.5, _hash01(i, salt + 1) - 0.5, _hash01(i, salt + 2) + 0.25], axis=1).astype(np.float32)
            v[name][:, :3] = d / np.sqrt((d * d).sum(axis=1, dtype=np.float32))[:, None]
        v["tangent"][:, 3] = np.where(i % 3 == 0, -1.0, 1.0)
        for c, name in enumerate(("base_color", "metallic_roughness", "normal", "occlusion", "emissive")):
            v[name + "_tex_coord"] = np.stack([_hash01(i, 10 + c), _hash01(i, 20 + c)], axis=1)
        w = v.view(np.uint32).reshape(n, -1)
        w[:, 3], w[:, 7], w[:, 22], w[:, 23] = 0x7FC00000 + i, 0xFF800000, 0xDEADBEEF, i
        idx = np.stack([i[:-2], i[:-2] + 1, i[:-2] + 2], axis=1).ravel().astype(np.uint32)
        desc.meshes.append(scenes.MeshDesc(k, v, idx, grey))
        desc.instances.append((k, [scenes.translate(3.0 * (k - 1), 0.0, 0.0)]))
    data = {m.key: (targets(m.vertices, 2, 3 * k), rig(len(m.vertices), 2, k)) for k, m in enumerate(desc.meshes)}
    return desc, data


def test_single_calls_equal_the_models_at_tile_edges(rt, hip):
    """skin_mesh, pose_mesh(weights) and pose_mesh(weights, matrices) are batches of one item on pose_batch_kernel: at every vertex
    count around the tile of 256 the device bytes are the numpy models', record for record, the per-mesh figures are those of a
    single call, and sr_scene_pose_batch_info never hears of them."""
    desc, data = edge_meshes()
    sc = rt.Scene(0).load(desc)
    w, M = np.array([0.625, 0.0], np.float32), matrices(2)
    for slot, m in enumerate(desc.meshes):
        n, (d, inf) = len(m.vertices), data[m.key]
        sc.set_mesh_skin(m.key, inf, 2)
        sc.set_mesh_morph(m.key, d)
        morphed, bad, _ = mref.morph_model(m.vertices, d, w)
        assert bad is None
        ways = (("skin_mesh", lambda: sc.skin_mesh(m.key, M), sref.skin_model(m.vertices, inf, M), (0, 0, 1)),
                ("pose_mesh, morph", lambda: sc.pose_mesh(m.key, w), (morphed, None), (1, 1, 1)),
                ("pose_mesh, morph and skin", lambda: sc.pose_mesh(m.key, w, M), sref.skin_model(morphed, inf, M), (2, 1, 2)))
        for what, call, model, (posed, n_active, skinned) in ways:
            what = "%d vertices, %s" % (n, what)
            assert model[1] is None, what
            call()
            assert_records_equal(device_vertices(hip, sc, slot, n), model[0], what)
            assert device_vertices(hip, sc, slot, n).tobytes() != m.vertices.tobytes(), what
            assert flags(sc, m.key) == (1, 1, 0), what
            mi, si = sc.mesh_morph_info(m.key), sc.mesh_skin_info(m.key)
            assert (mi.n_targets, mi.posed, mi.n_active, mi.first_bad) == (2, posed, n_active, NONE), what
            assert (si.n_joints, si.skinned, si.first_bad) == (2, skinned, NONE), what
            assert sc.pose_batch_info().calls == 0, what
    sc.close()


def test_single_calls_and_batches_interleave_like_batches_alone(rt, hip):
    """One scene takes pose_mesh(A), pose_meshes([B, C]), a pose_mesh(C) refused for a non-finite vertex and skin_mesh(B); its twin
    takes the same poses through pose_meshes alone. After every step the device bytes of all meshes, the per-mesh figures and the
    flags are the twin's and the posed meshes are the models'; the refusal is the single call's, with the model's vertex; only the
    batch of step 2 shows in pose_batch_info; and both scenes build and trace alike."""
    full, _ = mesh_set()
    A, B, C = 6, 8, 9                                                # 257, 256 and 512 vertices
    desc = scenes.SceneDesc("interleaved")
    desc.meshes = [m for m in full.meshes if m.key in (A, B, C)]
    desc.instances = [(key, [scenes.translate(3.0 * k, 0.0, 0.0)]) for k, key in enumerate((A, B, C))]
    keys = [m.key for m in desc.meshes]
    assert keys == [A, B, C] and max(len(m.vertices) for m in desc.meshes) <= 600
    verts = {m.key: m.vertices for m in desc.meshes}
    lean = (300, 450)                                                # two vertices of every mesh lean on joint 2, nothing else does
    rigs, morphs = {}, {}
    for k, key in enumerate(keys):
        inf = rig(len(verts[key]), 2, k).copy()
        inf["joint"][inf["weight"] == 0] = 0
        for v in lean if key == C else ():
            inf["joint"][v], inf["weight"][v] = (2, 0, 0, 0), (1.0, 0, 0, 0)
        rigs[key], morphs[key] = inf, targets(verts[key], 2, 3 * k)
    w = np.array([0.0, -0.75], np.float32)
    M = np.concatenate([matrices(2), matrices(2)[:1]])
    bad_M = M.copy()
    bad_M[2, 1, 3] = np.inf
    sc, tw = rt.Scene(0).load(desc), rt.Scene(0).load(desc)
    for s in (sc, tw):
        for key in keys:
            s.set_mesh_skin(key, rigs[key], 3)
            s.set_mesh_morph(key, morphs[key])
        s.set_instances(desc.instances)

    def model(key, morph, skin, matrices_=M):
        v, bad = verts[key], None
        if morph:
            v, bad, _ = mref.morph_model(v, morphs[key], w)
            assert bad is None
        if skin:
            v, bad, _ = sref.skin_model(v, rigs[key], matrices_)
        return v, bad

    def state(s):
        return ([device_vertices(hip, s, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)], pose_infos(s, keys),
                [flags(s, k) for k in keys])

    def same(what, posed):
        assert state(sc) == state(tw), what
        for key, morph, skin in posed:
            want, bad = model(key, morph, skin)
            assert bad is None
            assert_records_equal(device_vertices(hip, sc, keys.index(key), len(want)), want, "%s: key %d against the model" % (what, key))

    fresh = info_tuple(sc.pose_batch_info(), times=True)
    assert fresh[8] == 0
    sc.pose_mesh(A, w, M); tw.pose_meshes([(A, w, M)])
    same("step 1, pose_mesh(A)", [(A, True, True)])
    assert info_tuple(sc.pose_batch_info(), times=True) == fresh
    sc.pose_meshes([(B, w, None), (C, w, M)]); tw.pose_meshes([(B, w, None), (C, w, M)])
    same("step 2, pose_meshes([B, C])", [(A, True, True), (B, True, False), (C, True, True)])
    batch = info_tuple(sc.pose_batch_info(), times=True)
    assert batch[:3] + batch[6:11] == (2, 3, 256 + 512, 2, 1, 1, NONE, NONE)
    worst = model(C, True, True, bad_M)[1]
    assert worst == lean[0]
    assert refused(rt, sc, lambda: sc.pose_mesh(C, w, bad_M)) == (ERR_INVALID_ARG, "update_mesh: vertex %d has a non-finite position" % worst)
    assert refused(rt, tw, lambda: tw.pose_meshes([(C, w, bad_M)])) == (ERR_INVALID_ARG, "pose_meshes: item 0: update_mesh: vertex %d has a non-finite position" % worst)
    same("step 3, a refused pose_mesh(C)", [(A, True, True), (B, True, False), (C, True, True)])
    assert sc.mesh_skin_info(C).first_bad == worst and sc.mesh_morph_info(C).first_bad == NONE
    assert info_tuple(sc.pose_batch_info(), times=True) == batch
    sc.skin_mesh(B, M); tw.pose_meshes([(B, None, M)])
    same("step 4, skin_mesh(B)", [(A, True, True), (B, False, True), (C, True, True)])
    assert info_tuple(sc.pose_batch_info(), times=True) == batch
    rays = ray_grid((-1.5, -1.5), (3.0 * 2 + 1.5, 1.5), 96, 24)
    rd = rt.rays_to_device(rays)
    sc.set_instances(desc.instances); tw.set_instances(desc.instances)
    assert_scenes_equal(rt, tw, sc, rays, rd, keys, "after the interleaved calls")
    sc.close(); tw.close()


CHILD = """
import sys
from sunray_amd import runtime as rt
r = rt.Renderer((32, 24))
g = rt.Gltf(sys.argv[1])
loaded = r.load_scene(g)
r.attach_skins(g, loaded)
r.pose_scene(g, loaded, 0, 0.4)
i = r.replica_scene(0).pose_batch_info()
print("pose_batch", i.calls, i.items, i.launches)
"""


def test_the_environment_selects_the_batch():
    """SR_POSE_BATCH=on in the environment of a fresh process: pose_scene goes through sr_renderer_pose_meshes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for value, want in (("on", "pose_batch 1 2 2"), ("off", "pose_batch 0 0 0")):
        env = dict(os.environ, SR_POSE_BATCH=value, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-c", CHILD, SKIN_FIXTURE], capture_output=True, text=True, env=env, timeout=120)
        assert out.returncode == 0 and want in out.stdout, (value, out.stdout[-2000:], out.stderr[-2000:])
