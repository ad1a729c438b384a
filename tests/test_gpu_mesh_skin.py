"""Scene.set_mesh_skin / Scene.skin_mesh / Renderer.attach_skins / Renderer.pose_scene (sr_scene_skin_mesh: a rigged mesh posed on
the device by the skin stage of pose_batch_kernel (the call is a batch of one item), its finite-position check fused, the result handed on as sr_scene_update_mesh_device hands on its
caller's vertices). The reference is tests/skin_reference.py: the header's arithmetic restated in numpy float32. Equal means
byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skin_reference as ref  # noqa: E402
from test_gpu_mesh_update_device import (ERR_INVALID_ARG, assert_scenes_equal, check_meshes, flags, ray_grid, refused, traces,  # noqa: E402
                                         update_counts)
from test_gpu_parity import assert_bits_equal  # noqa: E402

NONE = 0xFFFFFFFF
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skinned_bar.glb")


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


def device_vertices(hip, sc, slot, n):
    """The mesh's device buffer, through the address sr_scene_get_tables shows."""
    out = np.zeros(n, dtype=abi.VERTEX)
    addr = int(sc.tables()["meshes_info"][slot]["vertices"])
    assert hip.hipSetDevice(C.c_int(0)) == 0
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(addr), C.c_size_t(out.nbytes), C.c_int(2)) == 0
    return out


def assert_records_equal(got, want, what):
    g, w = got.view(np.uint32).reshape(len(got), -1), want.view(np.uint32).reshape(len(want), -1)
    diff = np.argwhere(g != w)
    assert len(diff) == 0, "%s: %d words differ, first at vertex %d word %d (%08x, model %08x)" % (
        what, len(diff), diff[0][0], diff[0][1], g[tuple(diff[0])], w[tuple(diff[0])])


# ---- the bind poses, rigs and matrices of the kernel test -------------------------------------------------------------------------
def _hash01(i, salt):
    """Deterministic float32 values in [0, 1) (a multiplicative hash of the index: no random state)."""
    x = (np.asarray(i, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) & np.uint64(0xFFFFFFFF)
    x = (x ^ (x >> np.uint64(15))) * np.uint64(2246822519) & np.uint64(0xFFFFFFFF)
    return ((x >> np.uint64(8)).astype(np.float64) / float(1 << 24)).astype(np.float32)


def rigged_meshes():
    """check_meshes() (3, 4, 63, 64, 65, 257 and 1026 vertices) with every word of every record made to count: unit tangents with
    a handedness, uv sets, non-finite and arbitrary pad words; every 29th vertex from 5 has a zero normal, every 31st from 7 a zero
    tangent (the zero-length fallback)."""
    desc = check_meshes()
    for m in desc.meshes:
        v, i = m.vertices, np.arange(len(m.vertices))
        t = np.stack([_hash01(i, 1) - 0.5, _hash01(i, 2) - 0.5, _hash01(i, 3) + 0.25], axis=1).astype(np.float32)
        v["tangent"][:, :3] = t / np.sqrt((t * t).sum(axis=1, dtype=np.float32))[:, None]
        v["tangent"][:, 3] = np.where(i % 3 == 0, -1.0, 1.0)
        for k, name in enumerate(("base_color", "metallic_roughness", "normal", "occlusion", "emissive")):
            v[name + "_tex_coord"] = np.stack([_hash01(i, 10 + k), _hash01(i, 20 + k)], axis=1)
        w = v.view(np.uint32).reshape(len(v), -1)
        w[:, 3] = 0x7FC00000 + i              # _pad0: NaNs with a payload
        w[:, 7] = 0xFF800000                  # _pad1: -Inf
        w[:, 22] = 0xDEADBEEF
        w[:, 23] = i
        v["normal"][i % 29 == 5] = 0.0
        v["tangent"][i % 31 == 7, :3] = 0.0
    return desc


def rig(n_vertices, n_joints, salt):
    """Influences with 1, 2, 3 and 4 non-zero weights that use joint 0 and joint n_joints - 1, sums of 1, 0.75 and 1.5, and on
    every fifth vertex a weight of exactly 0: on joint 1 where the rig has three joints or more (matrices() makes that matrix all
    NaN and nothing else names it), on joint 65535, past the rig, where it has fewer."""
    inf = np.zeros(n_vertices, dtype=abi.SKIN_INFLUENCE)
    last = n_joints - 1
    usable = [j for j in range(n_joints) if not (n_joints >= 3 and j == 1)]
    unused = 1 if n_joints >= 3 else 65535
    weights = {1: [(1.0,), (0.75,), (1.5,)], 2: [(0.5, 0.5), (0.5, 0.25), (0.625, 0.875)], 3: [(0.5, 0.25, 0.25), (0.75, 0.5, 0.25)],
               4: [(0.25, 0.25, 0.25, 0.25), (0.4, 0.3, 0.2, 0.1), (0.5, 0.125, 0.0625, 0.0625)]}
    for i in range(n_vertices):
        count = i % 4 + 1
        ws = weights[count][(i // 4) % len(weights[count])]
        joints = [0, last, usable[(i * 7 + salt) % len(usable)], usable[(i * 13 + 5) % len(usable)]]
        joints = joints[i % 2:] + joints[:i % 2]                       # joint 0 and the last joint take turns in the first place
        first = 1 if i % 5 == 0 and count < 4 else 0                   # every fifth vertex: the zero weight comes before the used ones
        inf["joint"][i] = unused if i % 5 == 0 else 0
        for s, (w, j) in enumerate(zip(ws, joints), start=first):
            inf["joint"][i, s], inf["weight"][i, s] = j, w
    return inf


def matrices(n_joints):
    """Identity, rigid rotations with a translation, non-uniform scales, reflections and a shear, by joint; with three joints or
    more joint 1 is all NaN (only weights of 0 name it)."""
    m = np.zeros((n_joints, 3, 4), dtype=np.float32)
    for j in range(n_joints):
        kind, a = (j + n_joints) % 5, 0.35 + 0.011 * j
        c, s = np.cos(a), np.sin(a)
        if kind == 0:
            m[j] = np.eye(3, 4)
        elif kind == 1:
            m[j] = [[c, -s, 0, 0.25], [s, c, 0, -0.125], [0, 0, 1, 0.5]]
        elif kind == 2:
            m[j] = [[1.5, 0, 0, 0.1], [0, 0.5, 0, 0.2], [0, 0, 2.25 + 0.01 * j, -0.3]]
        elif kind == 3:
            m[j] = [[-1, 0, 0, 0.2], [0, c, -s, 0], [0, s, c, 0.1]]
        else:
            m[j] = [[1, 0.3, 0, 0], [0, 1, -0.2, 0.3], [0.1, 0, 1, 0]]
    if n_joints >= 3:
        m[1] = np.nan
    return m


def attach_all(sc, desc, n_joints):
    rigs = {}
    for k, m in enumerate(desc.meshes):
        rigs[m.key] = rig(len(m.vertices), n_joints, k)
        sc.set_mesh_skin(m.key, rigs[m.key], n_joints)
    return rigs


# ---- 4. the kernel through the entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints", [1, 2, 7, 300])
def test_kernel_equals_the_model_byte_for_byte(rt, hip, n_joints):
    desc = rigged_meshes()
    sc = rt.Scene(0).load(desc)
    rigs, M = attach_all(sc, desc, n_joints), matrices(n_joints)
    moved = fallbacks = total = 0
    for slot, m in enumerate(desc.meshes):
        inf = rigs[m.key]
        nonzero = (inf["weight"] != 0).sum(axis=1)
        if len(inf) >= 63:
            assert set(nonzero) == {1, 2, 3, 4} and len({round(float(s), 4) for s in inf["weight"].sum(axis=1)}) >= 3
            used = inf["joint"][inf["weight"] != 0]
            assert 0 in used and n_joints - 1 in used
            if n_joints >= 3:
                assert 1 not in used and ((inf["joint"] == 1) & (inf["weight"] == 0)).any() and np.isnan(M[1]).all()
            else:
                assert ((inf["joint"] == 65535) & (inf["weight"] == 0)).any()
        want, bad, n_fallback = ref.skin_model(m.vertices, inf, M)
        assert bad is None and np.isfinite(want["position"]).all() and np.isfinite(want["normal"]).all()
        extent = float(np.ptp(m.vertices["position"], axis=0).max())
        moved += int((np.abs(want["position"] - m.vertices["position"]).max(axis=1) > 1e-3 * extent).sum())
        fallbacks += int(n_fallback.sum())
        total += len(want)
        sc.skin_mesh(m.key, M)
        info = sc.mesh_skin_info(m.key)
        assert (info.n_joints, info.skinned, info.first_bad) == (n_joints, 1, NONE)
        assert flags(sc, m.key) == (1, 1, 0)
        sc.set_instances(desc.instances)
        assert_records_equal(device_vertices(hip, sc, slot, len(want)), want, "%d joints, mesh of %d vertices" % (n_joints, len(want)))
    assert 2 * moved >= total and fallbacks >= 1, (moved, total, fallbacks)
    sc.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_non_finite_pose_is_refused_and_nothing_changes(rt, hip):
    desc = rigged_meshes()
    sc = rt.Scene(0).load(desc)
    key, slot, n = 7, 6, 1026
    inf = rig(n, 2, 3)
    inf = inf.copy()
    inf["joint"][inf["weight"] == 0] = 0
    for v in (700, 900):                                       # two vertices lean on joint 2, nothing else does
        inf["joint"][v], inf["weight"][v] = (2, 0, 0, 0), (1.0, 0, 0, 0)
    sc.set_mesh_skin(key, inf, 3)
    good = matrices(2)
    good = np.concatenate([good, good[:1]])
    rays = ray_grid((-1.5, -1.5), (3.0 * 6 + 1.5, 1.5), 160, 24)
    rd = rt.rays_to_device(rays)
    before, bytes_before, info0 = traces(rt, sc, rays, rd), device_vertices(hip, sc, slot, n), flags(sc, key)
    overflow = good.copy()
    overflow[2] = [[3e38, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    to_infinity = good.copy()
    to_infinity[2, 1, 3] = np.inf
    inf_twice = inf.copy()
    inf_twice["weight"][700, 0] = inf_twice["weight"][900, 0] = 2.0   # 2 * 3e38 overflows in the blend
    for what, M, rigging in (("a translation of +Inf", to_infinity, inf), ("a scale that overflows in the blend", overflow, inf_twice)):
        sc.set_mesh_skin(key, rigging, 3)
        assert ref.skin_model(desc.meshes[slot].vertices, rigging, M)[1] == 700, what
        got = refused(rt, sc, lambda: sc.skin_mesh(key, M))
        assert got == (ERR_INVALID_ARG, "update_mesh: vertex 700 has a non-finite position"), (what, got)
        info = sc.mesh_skin_info(key)
        assert (info.n_joints, info.skinned, info.first_bad) == (3, 0, 700), what
        assert flags(sc, key) == info0, what
        assert_records_equal(device_vertices(hip, sc, slot, n), bytes_before, "the mesh's device bytes after " + what)
        after = traces(rt, sc, rays, rd)                       # nothing is pending: no set_instances is needed to trace
        assert_bits_equal(before[0], after[0], "closest hits after " + what)
        assert_bits_equal(before[1], after[1], "occlusion after " + what)
    sc.skin_mesh(key, good)                                    # the next good pose works
    info = sc.mesh_skin_info(key)
    assert (info.skinned, info.first_bad) == (1, NONE)
    sc.set_instances(desc.instances)
    assert_records_equal(device_vertices(hip, sc, slot, n), ref.skin_model(desc.meshes[slot].vertices, inf_twice, good)[0], "the good pose")
    assert not np.array_equal(before[0], traces(rt, sc, rays, rd)[0])
    sc.close()


def test_attach_refusals_name_the_lowest_vertex(rt, hip):
    desc = rigged_meshes()
    sc = rt.Scene(0).load(desc)
    key, slot, n = 5, 4, 65
    good = rig(n, 3, 0)

    def bad(edit):
        a = good.copy()
        edit(a)
        return a

    def poke(a, v, joint=None, weight=None):
        if joint is not None:
            a["joint"][v] = joint
        if weight is not None:
            a["weight"][v] = weight
    cases = [
        ("no mesh is registered", lambda: sc.set_mesh_skin(99, good, 3)),
        ("%d influences given" % (n - 1), lambda: sc.set_mesh_skin(key, good[:-1], 3)),
        ("n_joints is 0", lambda: sc.set_mesh_skin(key, good, 0)),
        ("vertex 11 names joint 3", lambda: sc.set_mesh_skin(key, bad(lambda a: (poke(a, 40, (9, 0, 0, 0), (1, 0, 0, 0)), poke(a, 11, (0, 3, 0, 0), (0.5, 0.5, 0, 0)))), 3)),
        ("vertex 12 has a weight that is negative", lambda: sc.set_mesh_skin(key, bad(lambda a: (poke(a, 30, weight=(np.nan, 0, 0, 0)), poke(a, 12, weight=(1.5, -0.5, 0, 0)))), 3)),
        ("vertex 13 has a weight that is negative or not finite", lambda: sc.set_mesh_skin(key, bad(lambda a: poke(a, 13, weight=(0.5, np.inf, 0, 0))), 3)),
        ("vertex 14 has a weight that is negative or not finite", lambda: sc.set_mesh_skin(key, bad(lambda a: poke(a, 14, weight=(0, 0, 0, np.nan))), 3)),
        ("vertex 15 has four weights of 0", lambda: sc.set_mesh_skin(key, bad(lambda a: (poke(a, 15, weight=(0, 0, 0, 0)), poke(a, 16, weight=(0, 0, 0, 0)))), 3)),
    ]
    M = matrices(3)
    for text, call in cases:
        code, got = refused(rt, sc, call)
        assert code == ERR_INVALID_ARG and text in got, (text, got)
        assert sc.mesh_skin_info(key).n_joints == 0
    code, got = refused(rt, sc, lambda: sc.skin_mesh(key, M))
    assert code == ERR_INVALID_ARG and "no skin" in got
    # a joint index past the rig is free where its weight is 0
    sc.set_mesh_skin(key, bad(lambda a: poke(a, 3, (0, 65535, 2, 2), (1.0, 0.0, 0.0, 0.0))), 3)
    code, got = refused(rt, sc, lambda: sc.skin_mesh(key, matrices(4)))
    assert code == ERR_INVALID_ARG and "4 joint matrices given" in got and "3 joints" in got
    code, got = refused(rt, sc, lambda: sc.skin_mesh(98, M))
    assert code == ERR_INVALID_ARG and "no mesh is registered" in got
    # a refused attach leaves the earlier skin in place
    refused(rt, sc, lambda: sc.set_mesh_skin(key, good, 0))
    assert sc.mesh_skin_info(key).n_joints == 3
    # update_mesh does not move the bind pose; attaching again snapshots it anew
    sc.set_mesh_skin(key, good, 3)
    bind = desc.meshes[slot].vertices
    other = scenes.deform_vertices(bind, desc.meshes[slot].indices, 1.0)
    sc.update_mesh(key, other)
    sc.skin_mesh(key, M)
    sc.set_instances(desc.instances)
    posed = ref.skin_model(bind, good, M)[0]
    assert_records_equal(device_vertices(hip, sc, slot, n), posed, "a pose after update_mesh starts from the bind pose of the attach")
    sc.set_mesh_skin(key, good, 3)
    assert sc.mesh_skin_info(key).skinned == 0
    sc.skin_mesh(key, M)
    sc.set_instances(desc.instances)
    assert_records_equal(device_vertices(hip, sc, slot, n), ref.skin_model(posed, good, M)[0], "a second attach took the posed vertices as its bind pose")
    # detaching frees the skin; removing a skinned mesh is clean
    sc.set_mesh_skin(key, None, 0)
    assert sc.mesh_skin_info(key).n_joints == 0
    assert "no skin" in refused(rt, sc, lambda: sc.skin_mesh(key, M))[1]
    sc.set_mesh_skin(key, good, 3)
    sc.remove(key)
    assert "no mesh is registered" in refused(rt, sc, lambda: sc.mesh_skin_info(key))[1]
    sc.close()


# ---- 5. scene equivalence over the fixture's animation ------------------------------------------------------------------------------
def fixture_scene(rt, emissive=False):
    """The fixture as a SceneDesc (mesh keys = blas index + 1, the file's instance transforms), its open Gltf, and per skinned key
    its influences."""
    parsed = rt.gltf_parse(FIXTURE)
    g = rt.Gltf(FIXTURE)
    desc = scenes.SceneDesc("skinned_bar")
    rigs = {}
    for b, blas in enumerate(parsed["blases"]):
        mat = blas["material"].copy()
        skin, inf = g.blas_skin(b)
        if skin >= 0:
            rigs[b + 1] = inf
            if emissive:
                mat["emissive_factor"] = (1.0, 0.5, 0.25, 3.0)
        desc.meshes.append(scenes.MeshDesc(b + 1, blas["vertices"], blas["indices"], mat))
    for b, t in parsed["instances"]:
        desc.instances.append((b + 1, [t]))
    assert sorted(rigs) == [1, 2] and [len(rigs[k]) for k in (1, 2)] == [200, 48]
    return desc, g, rigs


FIXTURE_RAYS = ((-3.0, -1.0), (3.0, 4.0))
# name -> (form, build type of the skinned meshes or None for Static, mesh-tree build mode, steps, emissive)
SKIN_PATHS = {
    "one-level": ("flat", None, "auto", 3, False),
    "two-level static mesh": ("two_level", None, "auto", 3, False),
    "two-level rapidly changing": ("two_level", abi.BUILD_RAPIDLY_CHANGING, "device", 10, False),
    "one-level emissive": ("flat", None, "auto", 2, True),
}


@pytest.mark.parametrize("path", list(SKIN_PATHS))
def test_skinned_scene_equals_the_host_update(rt, path):
    """Scene A takes the model's posed vertices through update_mesh, scene B the same pose through skin_mesh, over steps of the
    fixture's animation "bend": structure, tables, queries and counts are equal bit for bit."""
    form, build_type, mode, steps, emissive = SKIN_PATHS[path]
    desc, g, rigs = fixture_scene(rt, emissive)
    n_joints = len(g.skin(0)[1])
    pair = []
    for _ in range(2):
        sc = rt.Scene(0, instancing=form).set_mesh_tree_build(mode).load(desc)
        for key in rigs:
            if build_type is not None:
                sc.set_mesh_build_type(key, build_type)
        pair.append(sc)
    a, b = pair
    for key, inf in rigs.items():
        b.set_mesh_skin(key, inf, n_joints)
    if emissive:
        assert len(a.tables()["emissive_triangles"]) > 392
    rays = ray_grid(*FIXTURE_RAYS)
    rd = rt.rays_to_device(rays)
    first = traces(rt, b, rays, rd)[0]
    for n in range(1, steps + 1):
        joints = g.pose(0, 0.19 * n, 0)[1]
        for key, inf in rigs.items():
            posed, bad, _ = ref.skin_model(desc.meshes[key - 1].vertices, inf, joints)
            assert bad is None
            a.update_mesh(key, posed)
            b.skin_mesh(key, joints)
            assert b.mesh_skin_info(key).skinned == n
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        what = "%s, step %d" % (path, n)
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2, 3, 4], what)
        counts = update_counts(b)
        print(what, counts)
        if build_type is not None:          # refitted while the state asks for updates, built anew after more than 8 of them
            assert counts[2:4] == ((2, 0) if n == 9 else (0, 2)), (what, counts)
        elif form == "two_level":
            assert counts[2:4] == (2, 0), (what, counts)
        # the lazy host copy, as with update_mesh_device: an emissive mesh fetches inside the call
        if emissive:
            assert flags(b, 1) == (0, 1, n)
    assert not np.array_equal(first, traces(rt, b, rays, rd)[0])
    a.close(); b.close(); g.close()


# ---- 7. the facade --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one slot", "two slots on one GPU"])
def test_renderer_pose_scene_equals_update_mesh(rt, hip, devices):
    """Renderer.attach_skins + pose_scene over 8 frames of "bend" at 64x48 against a renderer fed the model's vertices through
    update_mesh and the model's instance transforms: the RGBA8 output is equal byte for byte."""
    from test_gpu_multi_renderer import assert_equal, grab
    cam = ((0.8, 1.4, 7.0), (0.8, 1.0, 0.0), 45.0)
    G = ref.Glb(FIXTURE)
    times = [0.05 + 0.23 * f for f in range(8)]

    def run(skinned):
        r = rt.Renderer((64, 48), devices=devices)
        g = rt.Gltf(FIXTURE)
        loaded = r.load_scene(g)
        keys = [int(k) for k in loaded.keys]
        binds = {keys[b]: (rt.gltf_parse(FIXTURE)["blases"][b]["vertices"], g.blas_skin(b)[1]) for b in (0, 1)}
        if skinned:
            r.attach_skins(g, loaded)
        else:
            for k in binds:
                r.set_mesh_build_type(k, abi.BUILD_RAPIDLY_CHANGING)
        out = []
        for t in times:
            if skinned:
                inst = r.pose_scene(g, loaded, 0, t)
            else:
                trs = {n: g.sample_node(0, t, n)[:3] for n in (1, 2, 3)}
                xf, joints = G.pose32(trs, 0)
                for k, (bind, inf) in binds.items():
                    r.update_mesh(k, ref.skin_model(bind, inf, joints)[0])
                inst = loaded.grouped(xf)                          # one instance per blas: the file's order is the loaded scene's
            fr = r.render(cam, inst)
            r.wait_frame(fr)
            out.append(grab(rt, hip, r)[0])
        if skinned:
            for slot in range(len(devices) if devices else 1):
                assert flags(r.replica_scene(slot), keys[0])[1] == 1, slot           # every replica's last update came from the device
            assert r.replica_scene(0).mesh_skin_info(keys[0]).skinned == len(times)
            assert r.history_overflow() == 0
        loaded.close(); g.close(); r.close()
        return out
    want, got = run(False), run(True)
    for f, (x, y) in enumerate(zip(want, got)):
        assert_equal(x, y, "frame %d output" % f)
    lit = [(x & 0xFFFFFF != 0).mean() for x in want]
    assert min(lit) > 0.05, lit                                     # the frames show something: the lit floor alone covers more
    assert not np.array_equal(want[1], want[6])
