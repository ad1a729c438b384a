"""Scene.set_mesh_morph / Scene.pose_mesh / Renderer.attach_morphs / Renderer.pose_scene (sr_scene_pose_mesh: a mesh's morph targets
blended on the device by the morph stage of pose_batch_kernel (the call is a batch of one item), its finite-position check fused,
the skin stage following in the same kernel where the mesh is rigged too, and the result handed on as sr_scene_update_mesh_device
hands on its caller's vertices). The reference is
tests/morph_reference.py: the header's arithmetic restated in numpy float32, composed with tests/skin_reference.py's model where
a skin follows. Equal means byte for byte."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import morph_reference as ref  # noqa: E402
import skin_reference as sref  # noqa: E402
from test_gpu_light_table import assert_lights_equal  # noqa: E402
from test_gpu_mesh_skin import _hash01, assert_records_equal, device_vertices, matrices, rig  # noqa: E402
from test_gpu_mesh_update import assert_frames_equal, one_frame  # noqa: E402
from test_gpu_mesh_update_device import ERR_INVALID_ARG, assert_scenes_equal, flags, ray_grid, refused, traces, update_counts  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402

NONE = 0xFFFFFFFF
ERR_UNSUPPORTED = -5
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph_bar.glb")
# the 64-lane wave edge, the 256-vertex tile edge, one full tile plus a partial one, several tiles
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


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


# ---- the bases, targets and weights of the kernel tests ---------------------------------------------------------------------------
def base_meshes():
    """Meshes of SIZES vertices, keys 1..8, side by side along x, with every word of every record made to count: scattered
    positions, unit normals and tangents with a handedness, uv sets, non-finite and arbitrary pad words (bit-pattern canaries: the
    kernel must carry them through untouched). A mesh of n vertices has the triangles (i, i + 1, i + 2); the single vertex has one
    triangle of its own and is loaded but not instanced."""
    s = scenes.SceneDesc("morph_bases")
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    for k, n in enumerate(SIZES, start=1):
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
        w[:, 3] = 0x7FC00000 + i              # _pad0: NaNs with a payload
        w[:, 7] = 0xFF800000                  # _pad1: -Inf
        w[:, 20] = 0x7F800001 + i             # a uv word that is a signalling NaN
        w[:, 22] = 0xDEADBEEF
        w[:, 23] = i
        idx = (np.stack([i[:-2], i[:-2] + 1, i[:-2] + 2], axis=1).ravel() if n >= 3 else np.zeros(3)).astype(np.uint32)
        s.meshes.append(scenes.MeshDesc(k, v, idx, grey))
        if n >= 3:
            s.instances.append((k, [scenes.translate(3.0 * (k - 1), 0.0, 0.0)]))
    return s


def targets(base, n_targets, salt):
    """Deltas [n_targets, n] in about -0.5..0.5 with the cases of the arithmetic placed by vertex index:
    i % 11 == 3   target 0's position delta has a -0.0f component
    i % 7 == 4    every vector of target 0 is all zeros (+0, -0, +0): a weight below 0 sums to zeros of either sign
    i % 5 == 2    target 1 is exactly minus target 0 (where there are two targets): equal weights cancel, s is 0 with active targets
    i % 13 == 6   target 0's normal delta is exactly minus the base normal: with a weight of 1 alone the morphed normal has length 0"""
    n = len(base)
    i = np.arange(n)
    d = np.zeros((n_targets, n), dtype=abi.MORPH_DELTA)
    for k in range(n_targets):
        for c, name in enumerate(("position", "normal", "tangent")):
            d[name][k] = np.stack([_hash01(i, salt + 7 * k + 100 * c + a) - 0.5 for a in range(3)], axis=1)
        w = d[k].view(np.uint32).reshape(n, -1)
        w[:, 3], w[:, 7], w[:, 11] = 0x7FC00000, 0xFF800000, 0xDEADBEEF          # the pads are never read: non-finite words are free there
    d["position"][0][i % 11 == 3, 1] = -0.0
    for name in ("position", "normal", "tangent"):
        d[name][0][i % 7 == 4] = (0.0, -0.0, 0.0)
    d["normal"][0][i % 13 == 6] = -base["normal"][i % 13 == 6]
    if n_targets >= 2:
        for name in ("position", "normal", "tangent"):
            d[name][1][i % 5 == 2] = -d[name][0][i % 5 == 2]
    return d


def weight_sets(n_targets):
    k = np.arange(n_targets)
    sets = {
        "all zero": np.zeros(n_targets, np.float32),
        "a single one": np.where(k == 0, 1.0, 0.0).astype(np.float32),
        "interleaved zeros": np.where(k % 2 == 0, 0.5 + 0.0625 * k, 0.0).astype(np.float32),
        "negative and above 1": np.where(k % 2 == 0, -0.75 - 0.125 * k, 1.5 + 0.25 * k).astype(np.float32),
        "a weight of -0.0f": np.where(k == n_targets - 1, 0.625 if n_targets > 1 else -0.0, -0.0).astype(np.float32),
        "cancelling targets": np.where(k < 2, 0.75, 0.0).astype(np.float32) if n_targets >= 2 else np.array([-1.0], np.float32),
        "the last target alone": np.where(k == n_targets - 1, 0.875, 0.0).astype(np.float32),
    }
    assert np.signbit(sets["a weight of -0.0f"][0])
    return sets


# ---- 1. the kernel through the entry point ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_targets", [1, 2, 5, 33])
def test_kernel_equals_the_model_byte_for_byte(rt, hip, n_targets):
    desc = base_meshes()
    sc = rt.Scene(0).load(desc)
    seen = {"cancelled": 0, "zero-length normal": 0, "moved": 0}
    for slot, m in enumerate(desc.meshes):
        n = len(m.vertices)
        d = targets(m.vertices, n_targets, 3 * slot)
        sc.set_mesh_morph(m.key, d)
        assert sc.mesh_morph_info(m.key).n_targets == n_targets
        posed = 0
        for what, w in weight_sets(n_targets).items():
            what = "%d targets, %d vertices, %s" % (n_targets, n, what)
            want, bad, fallback = ref.morph_model(m.vertices, d, w)
            assert bad is None, what
            n_active = int((w != 0).sum())
            kept = (want.view(np.uint32).reshape(n, -1)[:, :12] == m.vertices.view(np.uint32).reshape(n, -1)[:, :12]).all(axis=1)
            if n_active == 0:
                assert want.tobytes() == m.vertices.tobytes(), what            # all weights 0: the base byte for byte
            elif "cancelling" in what:
                seen["cancelled"] += int(kept.sum())
            seen["zero-length normal"] += int(fallback.sum())
            seen["moved"] += int((~kept).sum())
            sc.pose_mesh(m.key, w)
            posed += 1
            info = sc.mesh_morph_info(m.key)
            assert (info.n_targets, info.posed, info.n_active, info.first_bad) == (n_targets, posed, n_active, NONE), what
            assert flags(sc, m.key) == (1, 1, 0), what
            assert_records_equal(device_vertices(hip, sc, slot, n), want, what)
        sc.set_instances(desc.instances)
    assert seen["cancelled"] >= 100 and seen["zero-length normal"] >= 50 and seen["moved"] >= 5000, seen
    sc.close()


# ---- 2. a result that is not finite ---------------------------------------------------------------------------------------------------
def test_non_finite_morph_is_refused_and_nothing_changes(rt, hip):
    desc = base_meshes()
    sc = rt.Scene(0).load(desc)
    key, slot, n = 8, 7, 1000
    base = desc.meshes[slot].vertices
    d = targets(base, 2, 5)
    for name in ("position", "normal", "tangent"):
        d[name][1] = 0.0
    d["position"][1][700] = (0.0, 2.0, 0.0)                    # two vertices lean on target 1, nothing else does
    d["position"][1][900] = (2.0, 0.0, 0.0)
    sc.set_mesh_morph(key, d)
    rays = ray_grid((-1.5, -1.5), (3.0 * 7 + 1.5, 1.5), 160, 24)
    rd = rt.rays_to_device(rays)
    before, bytes_before, info0 = traces(rt, sc, rays, rd), device_vertices(hip, sc, slot, n), flags(sc, key)
    tables_before, bvh_before = sc.tables(), sc.read_bvh()
    good = np.array([0.5, 0.25], np.float32)
    overflow = np.array([0.5, 3e38], np.float32)               # 3e38 * 2 overflows to +Inf in the blend
    assert ref.morph_model(base, d, overflow)[1] == 700
    got = refused(rt, sc, lambda: sc.pose_mesh(key, overflow))
    assert got == (ERR_INVALID_ARG, "update_mesh: vertex 700 has a non-finite position"), got
    info = sc.mesh_morph_info(key)
    assert (info.n_targets, info.posed, info.n_active, info.first_bad) == (2, 0, 2, 700)
    assert flags(sc, key) == info0
    assert_records_equal(device_vertices(hip, sc, slot, n), bytes_before, "the mesh's device bytes after the refusal")
    after = traces(rt, sc, rays, rd)                           # nothing is pending: no set_instances is needed to trace
    assert_bits_equal(before[0], after[0], "closest hits after the refusal")
    assert_bits_equal(before[1], after[1], "occlusion after the refusal")
    for name in ("transforms", "indirection", "emissive_triangles", "meshes_info"):
        assert tables_before[name].tobytes() == sc.tables()[name].tobytes(), name
    for x, y in zip(bvh_before, sc.read_bvh()):
        assert x.tobytes() == y.tobytes()
    sc.pose_mesh(key, good)                                    # the next good pose works
    info = sc.mesh_morph_info(key)
    assert (info.posed, info.first_bad) == (1, NONE)
    sc.set_instances(desc.instances)
    assert_records_equal(device_vertices(hip, sc, slot, n), ref.morph_model(base, d, good)[0], "the good pose")
    assert not np.array_equal(before[0], traces(rt, sc, rays, rd)[0])
    sc.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_attach_and_pose_refusals_name_the_lowest_index(rt, hip):
    from sunray_amd._lib import lib
    desc = base_meshes()
    sc = rt.Scene(0).load(desc)
    key, slot, n = 4, 3, 65
    base = desc.meshes[slot].vertices
    good = targets(base, 3, 1)

    def bad(pokes):
        a = good.copy()
        for k, v, name, c, x in pokes:
            a[name][k][v, c] = x
        return a
    attach = [
        ("no mesh is registered", lambda: sc.set_mesh_morph(99, good)),
        ("targets of %d vertices given" % (n - 1), lambda: sc.set_mesh_morph(key, good[:, :-1])),
        ("target 1 has a delta component that is not finite at vertex 11", lambda: sc.set_mesh_morph(key, bad([(2, 3, "position", 0, np.nan), (1, 40, "normal", 1, np.inf), (1, 11, "tangent", 2, -np.inf)]))),
        ("target 0 has a delta component that is not finite at vertex 64", lambda: sc.set_mesh_morph(key, bad([(0, 64, "position", 2, np.nan), (1, 0, "position", 0, np.nan)]))),
    ]
    for text, call in attach:
        code, got = refused(rt, sc, call)
        assert code == ERR_INVALID_ARG and text in got, (text, got)
        assert sc.mesh_morph_info(key).n_targets == 0
    gp = good.ctypes.data_as(C.c_void_p)
    assert lib().sr_scene_set_mesh_morph(sc._h, C.c_uint64(key), gp, C.c_uint32(n), C.c_uint32(0)) == ERR_INVALID_ARG and b"n_targets is 0" in lib().sr_last_error()
    w3, M = np.array([0.5, 0.0, 0.25], np.float32), matrices(3)
    code, got = refused(rt, sc, lambda: sc.pose_mesh(key, w3))
    assert code == ERR_INVALID_ARG and "no morph targets" in got
    sc.set_mesh_morph(key, good)
    bytes_before = device_vertices(hip, sc, slot, n)
    pose = [
        ("no mesh is registered", lambda: sc.pose_mesh(98, w3)),
        ("4 weights given", lambda: sc.pose_mesh(key, np.zeros(4, np.float32))),
        ("weight 1 is not finite", lambda: sc.pose_mesh(key, np.array([0.5, np.nan, np.inf], np.float32))),
        ("weight 2 is not finite", lambda: sc.pose_mesh(key, np.array([0.5, 0.0, -np.inf], np.float32))),
        ("no skin", lambda: sc.pose_mesh(key, w3, M)),
        ("no skin", lambda: sc.pose_mesh(key, None, M)),                  # without weights the call is skin_mesh
    ]
    for text, call in pose:
        code, got = refused(rt, sc, call)
        assert code == ERR_INVALID_ARG and text in got, (text, got)
    assert lib().sr_scene_pose_mesh(sc._h, C.c_uint64(key), None, C.c_uint32(3), None, C.c_uint32(0), None) == ERR_INVALID_ARG and b"neither" in lib().sr_last_error()
    sc.set_mesh_skin(key, rig(n, 3, 0), 3)
    code, got = refused(rt, sc, lambda: sc.pose_mesh(key, w3, matrices(4)))
    assert code == ERR_INVALID_ARG and "4 joint matrices given" in got and "3 joints" in got
    info = sc.mesh_morph_info(key)
    assert (info.n_targets, info.posed) == (3, 0) and flags(sc, key) == (0, 0, 0)
    assert_records_equal(device_vertices(hip, sc, slot, n), bytes_before, "the mesh's device bytes after the refusals")
    # a refused attach leaves the earlier morph in place
    refused(rt, sc, lambda: sc.set_mesh_morph(key, bad([(0, 5, "position", 0, np.nan)])))
    assert sc.mesh_morph_info(key).n_targets == 3
    # an emissive list that is not one per triangle cannot be re-derived from vertices
    qv, qi = scenes.quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), (0, 0, 1))
    one = np.zeros(1, dtype=abi.EMISSIVE_TRIANGLE)
    one["v0"][0, :3], one["v1"][0, :3], one["v2"][0, :3], one["emission"][0] = qv["position"][0], qv["position"][1], qv["position"][2], (1, 1, 1, 1)
    sc.add_blas(50, qv, qi, abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1.0, 1.0, 1.0), emissive_strength=2.0), one)
    sc.set_mesh_morph(50, np.zeros((1, 4), dtype=abi.MORPH_DELTA))
    code, got = refused(rt, sc, lambda: sc.pose_mesh(50, np.ones(1, np.float32)))
    assert code == ERR_UNSUPPORTED and "not one per triangle" in got
    # update_mesh does not move the base; attaching again snapshots it anew
    w = np.array([0.5, -0.25, 1.0], np.float32)
    moved = base.copy()
    moved["position"] += np.float32(0.25)
    sc.update_mesh(key, moved)
    sc.pose_mesh(key, w)
    sc.set_instances(desc.instances)
    posed = ref.morph_model(base, good, w)[0]
    assert_records_equal(device_vertices(hip, sc, slot, n), posed, "a pose after update_mesh starts from the base of the attach")
    sc.set_mesh_morph(key, good)
    assert sc.mesh_morph_info(key).posed == 0
    sc.pose_mesh(key, w)
    sc.set_instances(desc.instances)
    assert_records_equal(device_vertices(hip, sc, slot, n), ref.morph_model(posed, good, w)[0], "a second attach took the posed vertices as its base")
    # detaching frees the morph and leaves the skin; removing a morphed mesh is clean
    sc.set_mesh_morph(key, None)
    assert sc.mesh_morph_info(key).n_targets == 0 and sc.mesh_skin_info(key).n_joints == 3
    assert "no morph targets" in refused(rt, sc, lambda: sc.pose_mesh(key, w))[1]
    sc.set_mesh_morph(key, good)
    sc.remove(key)
    assert "no mesh is registered" in refused(rt, sc, lambda: sc.mesh_morph_info(key))[1]
    sc.close()


# ---- 4. morph, then skin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_joints", [2, 7])
def test_morph_then_skin_equals_the_composed_models(rt, hip, n_joints):
    desc = base_meshes()
    sc = rt.Scene(0).load(desc)
    M = matrices(n_joints)
    n_targets = 5
    w = weight_sets(n_targets)["negative and above 1"]
    for slot, m in enumerate(desc.meshes):
        n = len(m.vertices)
        what = "%d joints, %d vertices" % (n_joints, n)
        d, inf = targets(m.vertices, n_targets, slot), rig(n, n_joints, slot)
        sc.set_mesh_skin(m.key, inf, n_joints)                             # both while the mesh holds its rest vertices
        sc.set_mesh_morph(m.key, d)
        morphed, bad, _ = ref.morph_model(m.vertices, d, w)
        want, bad2, _ = sref.skin_model(morphed, inf, M)
        assert bad is None and bad2 is None, what
        sc.pose_mesh(m.key, w, M)
        mi, si = sc.mesh_morph_info(m.key), sc.mesh_skin_info(m.key)
        assert (mi.posed, mi.n_active, mi.first_bad, si.skinned, si.first_bad) == (1, n_targets, NONE, 1, NONE), what
        assert_records_equal(device_vertices(hip, sc, slot, n), want, what + ", morph then skin")
        assert want.tobytes() != sref.skin_model(m.vertices, inf, M)[0].tobytes() or n == 1, what       # the morph shows in the result
        # the morph stage alone on a rigged mesh, and the skin stage alone: exactly skin_mesh, counted by SrMeshSkinInfo
        sc.pose_mesh(m.key, w)
        assert_records_equal(device_vertices(hip, sc, slot, n), morphed, what + ", the morph stage alone")
        sc.pose_mesh(m.key, None, M)
        by_pose = device_vertices(hip, sc, slot, n)
        assert_records_equal(by_pose, sref.skin_model(m.vertices, inf, M)[0], what + ", the skin stage alone")
        sc.skin_mesh(m.key, M)
        assert_records_equal(device_vertices(hip, sc, slot, n), by_pose, what + ", skin_mesh")
        mi, si = sc.mesh_morph_info(m.key), sc.mesh_skin_info(m.key)
        assert (mi.posed, si.skinned, si.n_joints) == (2, 3, n_joints), what
        sc.set_instances(desc.instances)
    # a vertex the morph sends to infinity is refused with its index whichever stage sees it first
    key, slot, n = 6, 5, 256
    d = targets(desc.meshes[slot].vertices, 2, 9)
    d["position"][1] = 0.0
    d["position"][1][255] = (0.0, 0.0, 2.0)
    sc.set_mesh_morph(key, d)
    got = refused(rt, sc, lambda: sc.pose_mesh(key, np.array([0.0, 3e38], np.float32), M))
    assert got == (ERR_INVALID_ARG, "update_mesh: vertex 255 has a non-finite position"), got
    assert sc.mesh_morph_info(key).first_bad == 255 and sc.mesh_skin_info(key).first_bad == 255
    sc.close()


# ---- 5. scene equivalence over the fixture's animation ----------------------------------------------------------------------------------
def fixture_scene(rt, emissive=False):
    """The fixture as a SceneDesc (mesh keys = blas index + 1, the file's instance transforms), its open Gltf, and per morphed key
    its (deltas, influences or None)."""
    parsed = rt.gltf_parse(FIXTURE)
    g = rt.Gltf(FIXTURE)
    desc = scenes.SceneDesc("morph_bar", camera_pos=(0.8, 1.4, 7.0), camera_target=(0.8, 1.0, 0.0))
    morphs = {}
    for b, blas in enumerate(parsed["blases"]):
        mat = blas["material"].copy()
        d, _ = g.blas_morph(b)
        if d is not None:
            morphs[b + 1] = (d, g.blas_skin(b)[1])
            if emissive:
                mat["emissive_factor"] = (1.0, 0.5, 0.25, 3.0)
        desc.meshes.append(scenes.MeshDesc(b + 1, blas["vertices"], blas["indices"], mat))
    for b, t in parsed["instances"]:
        desc.instances.append((b + 1, [t]))
    assert sorted(morphs) == [1, 2] and [morphs[k][0].shape for k in (1, 2)] == [(3, 200), (2, 48)]
    assert morphs[1][1] is not None and morphs[2][1] is None
    return desc, g, morphs


def model_pose(desc, g, morphs, key, t):
    """-> (the model's posed vertices of mesh `key` at time t of animation 0, its weights, its joint matrices or None)."""
    d, inf = morphs[key]
    w = g.morph_weights(0, t, key - 1)
    posed, bad, _ = ref.morph_model(desc.meshes[key - 1].vertices, d, w)
    assert bad is None
    joints = None
    if inf is not None:
        joints = g.pose(0, t, 0)[1]
        posed, bad, _ = sref.skin_model(posed, inf, joints)
        assert bad is None
    return posed, w, joints


FIXTURE_RAYS = ((-3.0, -1.0), (3.0, 4.0))
# name -> (form, build type of the morphed meshes or None for Static, mesh-tree build mode, steps, emissive, scene B's light table)
MORPH_PATHS = {
    "one-level": ("flat", None, "auto", 3, False, "host"),
    "two-level static mesh": ("two_level", None, "auto", 3, False, "host"),
    "two-level rapidly changing": ("two_level", abi.BUILD_RAPIDLY_CHANGING, "device", 10, False, "host"),
    "one-level emissive": ("flat", None, "auto", 2, True, "host"),
    "one-level emissive, device lights": ("flat", None, "auto", 2, True, "device"),
}


@pytest.mark.parametrize("path", list(MORPH_PATHS))
def test_morphed_scene_equals_the_host_update(rt, blue_noise, path):
    """Scene A takes the model's posed vertices through update_mesh, scene B the same pose through pose_mesh (morph and skin on mesh
    1, morph alone on mesh 2), over steps of the fixture's animation "talk": structure, tables, queries and counts are equal bit
    for bit, and so is one small frame."""
    form, build_type, mode, steps, emissive, lights = MORPH_PATHS[path]
    desc, g, morphs = fixture_scene(rt, emissive)
    n_joints = len(g.skin(0)[1])
    pair = []
    for which in range(2):
        sc = rt.Scene(0, instancing=form).set_mesh_tree_build(mode)
        if which == 1 and lights == "device":
            sc.set_light_table_build("device")
        sc.load(desc)
        for key in morphs:
            if build_type is not None:
                sc.set_mesh_build_type(key, build_type)
        pair.append(sc)
    a, b = pair
    for key, (d, inf) in morphs.items():
        b.set_mesh_morph(key, d)
        if inf is not None:
            b.set_mesh_skin(key, inf, n_joints)
    if emissive:
        assert len(a.tables()["emissive_triangles"]) > 392
    rays = ray_grid(*FIXTURE_RAYS)
    rd = rt.rays_to_device(rays)
    first = traces(rt, b, rays, rd)[0]
    for n in range(1, steps + 1):
        for key in morphs:
            posed, w, joints = model_pose(desc, g, morphs, key, 0.19 * n)
            assert (w != 0).any()
            a.update_mesh(key, posed)
            b.pose_mesh(key, w, joints)
            assert b.mesh_morph_info(key).posed == n
            if lights == "device":          # the arena follows on the device: no fetch
                assert flags(b, key) == (1, 1, 0), (n, key)
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        what = "%s, step %d" % (path, n)
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2, 3, 4], what)
        counts = update_counts(b)
        print(what, counts)
        if build_type is not None:          # refitted while the state asks for updates, built anew after more than 8 of them
            assert counts[2:4] == ((2, 0) if n == 9 else (0, 2)), (what, counts)
        elif form == "two_level":
            assert counts[2:4] == (2, 0), (what, counts)
        if emissive and lights == "host":   # the lazy host copy, as with update_mesh_device: an emissive mesh fetches inside the call
            assert flags(b, 1) == (0, 1, n)
        if lights == "device":
            assert_lights_equal(a, b, what)
    assert not np.array_equal(first, traces(rt, b, rays, rd)[0])
    assert_frames_equal(one_frame(rt, a, desc, 64, 48, blue_noise), one_frame(rt, b, desc, 64, 48, blue_noise), path + ": a frame after the last step")
    a.close(); b.close(); g.close()


# ---- 6. the facade ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one slot", "two slots on one GPU"])
def test_renderer_pose_scene_equals_update_mesh(rt, hip, devices):
    """Renderer.attach_skins + attach_morphs + pose_scene at two times of "talk" at 64x48 against a renderer fed the model's
    vertices through update_mesh and the model's instance transforms: the RGBA8 output is equal byte for byte."""
    from test_gpu_multi_renderer import assert_equal, grab
    cam = ((0.8, 1.4, 7.0), (0.8, 1.0, 0.0), 45.0)
    G = sref.Glb(FIXTURE)
    times = [0.3, 1.45]

    def run(posed_by_library):
        r = rt.Renderer((64, 48), devices=devices)
        g = rt.Gltf(FIXTURE)
        loaded = r.load_scene(g)
        keys = [int(k) for k in loaded.keys]
        parsed = rt.gltf_parse(FIXTURE)
        if posed_by_library:
            r.attach_skins(g, loaded)
            r.attach_morphs(g, loaded)
        else:
            for b in (0, 1):
                r.set_mesh_build_type(keys[b], abi.BUILD_RAPIDLY_CHANGING)
        out = []
        for t in times:
            if posed_by_library:
                inst = r.pose_scene(g, loaded, 0, t)
            else:
                trs = {n: g.sample_node(0, t, n)[:3] for n in (1, 2, 3)}
                xf, joints = G.pose32(trs, 0)
                for b in (0, 1):
                    v = ref.morph_model(parsed["blases"][b]["vertices"], g.blas_morph(b)[0], g.morph_weights(0, t, b))[0]
                    if b == 0:
                        v = sref.skin_model(v, g.blas_skin(0)[1], joints)[0]
                    r.update_mesh(keys[b], v)
                inst = loaded.grouped(xf)                          # one instance per blas: the file's order is the loaded scene's
            fr = r.render(cam, inst)
            r.wait_frame(fr)
            out.append(grab(rt, hip, r)[0])
        if posed_by_library:
            for slot in range(len(devices) if devices else 1):
                for b in (0, 1):
                    assert flags(r.replica_scene(slot), keys[b])[1] == 1, (slot, b)      # every replica's last update came from the device
            first = r.replica_scene(0)
            assert [first.mesh_morph_info(keys[b]).posed for b in range(4)] == [len(times), len(times), 0, 0]
            assert first.mesh_skin_info(keys[0]).skinned == len(times) and first.mesh_morph_info(keys[0]).n_targets == 3
            assert r.history_overflow() == 0
        loaded.close(); g.close(); r.close()
        return out
    want, got = run(False), run(True)
    for f, (x, y) in enumerate(zip(want, got)):
        assert_equal(x, y, "frame %d output" % f)
    lit = [(x & 0xFFFFFF != 0).mean() for x in want]
    assert min(lit) > 0.05, lit
    assert not np.array_equal(want[0], want[1])
