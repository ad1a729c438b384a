"""What the device producers of a mesh's vertices share (api.cpp pose_items / finish_device_update, renderer.cpp
first_scene_poses / first_scene_produces) and no other suite pins: which timing field each call writes, and that pose_mesh without weights is
skin_mesh. Times are compared with 0.0 only, never by magnitude. The meshes are the tile and wave edges of the posing kernels."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_morph import base_meshes, hip, rt, targets  # noqa: E402,F401
from test_gpu_mesh_skin import device_vertices, matrices, rig  # noqa: E402
from test_gpu_mesh_update_device import ERR_INVALID_ARG, flags, refused, to_device  # noqa: E402

SIZES = (1, 63, 64, 65, 255, 256, 257)
N_JOINTS, N_TARGETS = 4, 2
WEIGHTS = np.array([0.5, -0.25], np.float32)
OVERFLOW = np.array([0.0, 3e38], np.float32)        # 3e38 * 2 overflows to +Inf in the blend


def edge_meshes():
    """(slot, mesh, influences, deltas) of base_meshes() at SIZES; target 1 moves the last vertex alone, by 2 along z."""
    out = []
    for slot, m in enumerate(base_meshes().meshes):
        n = len(m.vertices)
        if n not in SIZES:
            continue
        d = targets(m.vertices, N_TARGETS, slot)
        for name in ("position", "normal", "tangent"):
            d[name][1] = 0.0
        d["position"][1][n - 1] = (0.0, 0.0, 2.0)
        out.append((slot, m, rig(n, N_JOINTS, slot), d))
    assert tuple(len(m.vertices) for _, m, _, _ in out) == SIZES
    return out


def times(sc, key):
    """(check_ms, copy_ms, skin_ms, morph_ms, skinned, posed) of one mesh."""
    v, s, m = sc.mesh_vertex_info(key), sc.mesh_skin_info(key), sc.mesh_morph_info(key)
    return (v.check_ms, v.copy_ms, s.skin_ms, m.morph_ms, s.skinned, m.posed)


def update_times(sc):
    i = sc.mesh_update_info()
    assert i.validate_copy_ms >= 0.0 and i.h2d_ms >= 0.0
    return (i.validate_copy_ms, i.h2d_ms)


@pytest.mark.parametrize("timing", [True, False], ids=["timing on", "timing off"])
def test_the_timing_fields_say_which_stage_ran(rt, timing):
    desc = base_meshes()
    sc = rt.Scene(0).load(desc)
    sc.enable_timing(timing)
    M = matrices(N_JOINTS)

    def ran(x):             # a stage that ran shows a time while timing is on, and 0.0 while it is off
        return x > 0.0 if timing else x == 0.0
    for slot, m, inf, d in edge_meshes():
        n, key = len(m.vertices), m.key
        sc.set_mesh_skin(key, inf, N_JOINTS)
        sc.set_mesh_morph(key, d)
        assert times(sc, key) == (0.0, 0.0, 0.0, 0.0, 0, 0), n
        seen = [update_times(sc)]

        def rewritten():
            seen.append(update_times(sc))
            return seen[-1] != seen[-2]       # wall-clock intervals in nanoseconds: two calls do not give the same pair
        sc.update_mesh_device(key, to_device(m.vertices))
        check, copy, skin, morph, skinned, posed = times(sc, key)
        assert ran(check) and ran(copy) and (skin, morph, skinned, posed) == (0.0, 0.0, 0, 0), (n, times(sc, key))
        assert rewritten(), n
        sc.skin_mesh(key, M)
        check, copy, skin, morph_after, skinned, posed = times(sc, key)
        assert ran(skin) and check == 0.0 and ran(copy) and morph_after == morph and (skinned, posed) == (1, 0), (n, times(sc, key))
        assert rewritten(), n
        sc.pose_mesh(key, WEIGHTS)
        check, copy, skin_after, morph, skinned, posed = times(sc, key)
        assert ran(morph) and check == 0.0 and ran(copy) and skin_after == skin and (skinned, posed) == (1, 1), (n, times(sc, key))
        assert rewritten(), n
        sc.pose_mesh(key, WEIGHTS, M)
        check, copy, skin, morph, skinned, posed = times(sc, key)
        assert ran(morph) and skin == 0.0 and check == 0.0 and ran(copy) and (skinned, posed) == (2, 2), (n, times(sc, key))
        assert rewritten(), n
        # every field holds an accepted value that is not 0 (timing on) before the refusal, so a field it touched would show
        sc.skin_mesh(key, M)
        sc.update_mesh_device(key, to_device(m.vertices))
        accepted = times(sc, key)
        assert all(ran(x) for x in accepted[:4]) and accepted[4:] == (3, 2), (n, accepted)
        for call in (lambda: sc.pose_mesh(key, OVERFLOW, M), lambda: sc.pose_mesh(key, OVERFLOW)):
            got = refused(rt, sc, call)
            assert got == (ERR_INVALID_ARG, "update_mesh: vertex %d has a non-finite position" % (n - 1)), (n, got)
            assert times(sc, key) == accepted, (n, times(sc, key), accepted)
            assert sc.mesh_morph_info(key).first_bad == n - 1
        sc.set_instances(desc.instances)
    sc.close()


@pytest.mark.parametrize("timing", [True, False], ids=["timing on", "timing off"])
def test_a_replica_that_takes_the_vertices_times_its_copy_alone(rt, timing):
    """srh::scene_take_device_vertices: the second slot's scene of a renderer on [0, 0] after the first one validated or posed."""
    r = rt.Renderer((64, 48), devices=[0, 0])
    first, second = r.replica_scene(0), r.replica_scene(1)
    first.enable_timing(timing)
    second.enable_timing(timing)
    M = matrices(N_JOINTS)
    for slot, m, inf, d in edge_meshes():
        n, key = len(m.vertices), m.key
        r.load_mesh(key, m.vertices, m.indices, m.material)
        r.set_mesh_skin(key, inf, N_JOINTS)
        r.set_mesh_morph(key, d)
        before = update_times(second)
        calls = (lambda: r.update_mesh_device(key, to_device(m.vertices)), lambda: r.skin_mesh(key, M), lambda: r.pose_mesh(key, WEIGHTS),
                 lambda: r.pose_mesh(key, WEIGHTS, M))
        for k, call in enumerate(calls):
            call()
            check, copy, skin, morph, skinned, posed = times(second, key)
            assert check == 0.0 and (copy > 0.0 if timing else copy == 0.0), (n, k, times(second, key))
            assert (skin, morph, skinned, posed) == (0.0, 0.0, 0, 0), (n, k)      # rig and morph live on the first slot's scene
            assert flags(second, key) == (1, 1, 0), (n, k)
            after = update_times(second)
            assert after != before, (n, k)
            before = after
            c1 = times(first, key)[0]
            assert (c1 > 0.0 if timing and k == 0 else c1 == 0.0), (n, k, c1)     # the first slot's check is a kernel of its own in call 0 only
        assert refused(rt, first, lambda: r.pose_mesh(key, OVERFLOW, M))[1] == "update_mesh: vertex %d has a non-finite position" % (n - 1)
        assert update_times(second) == before and times(second, key)[:2] == (check, copy), n      # a refusal reaches no replica
    first.close(); second.close(); r.close()


def test_pose_mesh_without_weights_is_skin_mesh(rt, hip):
    """On meshes with a morph and a skin attached, scene A poses with pose_mesh(key, None, M), scene B with skin_mesh(key, M)."""
    desc = base_meshes()
    a, b = rt.Scene(0).load(desc), rt.Scene(0).load(desc)
    M = matrices(N_JOINTS)

    def skin_info(sc, key):
        i = sc.mesh_skin_info(key)
        return (i.n_joints, i.skinned, i.first_bad)

    def morph_info(sc, key):
        i = sc.mesh_morph_info(key)
        return (i.n_targets, i.posed, i.n_active, i.first_bad, i.morph_ms)
    for slot, m, inf, d in edge_meshes():
        n, key = len(m.vertices), m.key
        for sc in (a, b):
            sc.set_mesh_skin(key, inf, N_JOINTS)
            sc.set_mesh_morph(key, d)
            sc.pose_mesh(key, WEIGHTS)                  # a morph record that is not the initial one
        morph_before = morph_info(a, key), morph_info(b, key)
        assert morph_before[0][:4] == morph_before[1][:4] == (N_TARGETS, 1, 2, 0xFFFFFFFF), n
        for step in range(2):
            a.pose_mesh(key, None, M)
            b.skin_mesh(key, M)
            got, want = device_vertices(hip, a, slot, n), device_vertices(hip, b, slot, n)
            assert got.tobytes() == want.tobytes(), (n, step)
            assert got.tobytes() != m.vertices.tobytes(), n
            assert skin_info(a, key) == skin_info(b, key) == (N_JOINTS, step + 1, 0xFFFFFFFF), (n, step)
            assert (morph_info(a, key), morph_info(b, key)) == morph_before, (n, step)
            assert flags(a, key) == flags(b, key) == (1, 1, 0), (n, step)
        # the refusals of both spellings are skin_mesh's: a joint count that is not the rig's, then a matrix that is not finite
        texts = [refused(rt, sc, call)[1] for sc, call in ((a, lambda: a.pose_mesh(key, None, matrices(N_JOINTS + 1))), (b, lambda: b.skin_mesh(key, matrices(N_JOINTS + 1))))]
        assert texts[0] == texts[1] and texts[0].startswith("skin_mesh: %d joint matrices given" % (N_JOINTS + 1)), texts
        broken = M.copy()
        broken[0] = np.inf
        got = [refused(rt, sc, call) for sc, call in ((a, lambda: a.pose_mesh(key, None, broken)), (b, lambda: b.skin_mesh(key, broken)))]
        assert got[0] == got[1] and got[0][0] == ERR_INVALID_ARG, got
        assert skin_info(a, key) == skin_info(b, key) and skin_info(a, key)[:2] == (N_JOINTS, 2) and skin_info(a, key)[2] < n, n
        assert (morph_info(a, key), morph_info(b, key)) == morph_before, n
        assert flags(a, key) == flags(b, key) == (1, 1, 0), n
        a.set_instances(desc.instances); b.set_instances(desc.instances)
    for key, text in ((99, "skin_mesh: no mesh is registered under this key"), (8, "skin_mesh: the mesh has no skin")):
        for sc, call in ((a, lambda: a.pose_mesh(key, None, M)), (b, lambda: b.skin_mesh(key, M))):
            got = refused(rt, sc, call)
            assert got[0] == ERR_INVALID_ARG and got[1].startswith(text), got
    a.close(); b.close()
