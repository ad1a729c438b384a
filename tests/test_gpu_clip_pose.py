"""Scene.pose_actors / Renderer.pose_actors (sr_scene_pose_actors: clip_pose_kernel samples every actor's baked clip at its own
time, composes the hierarchy and writes the joint matrices where pose_batch_kernel reads them and the instance transforms where
set_instances_device takes them). The reference is the host rule (sr_clip_sample_host / sr_clip_compose_host, themselves held to
sr_gltf_pose bit for bit by test_clip_host.py) under the numerics contract of the header: everything but an interpolated rotation
is bit equal; such a component is the host's, its neighbouring float32, or within 2^-44 of it, and at most 1 in 1000 of them may be
other than bit equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_util import CLIP_RIG, assert_trs_contract, bits, clip_times, crowd, rotation_classes, shape_rig  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402
from test_gpu_mesh_update_device import assert_scenes_equal, ray_grid  # noqa: E402

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
SINGULAR = "gltf: the transform of the skinned mesh's node is singular"
PLACEMENT = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)
RAYS = ((-2.2, -0.2), (2.4, 3.2))           # the rig's extent: the bars are thin


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


def refused(rt, call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def rigged(rt, path, copies=1):
    """A scene of `copies` copies of a file with every skinned mesh's rig attached -> (scene, the crowd() tuple)."""
    c = crowd(rt, path, copies)
    sc = rt.Scene(0).load(c[0])
    for key, (inf, nj) in c[3].items():
        sc.set_mesh_skin(key, inf, nj)
    return sc, c


def skin_items(c, copy, actor):
    """One item per skinned mesh of copy `copy`, driven by actor `actor`."""
    return [(c[2][copy][b], actor, skin, None) for b, skin in enumerate(c[6]) if skin >= 0]


def tensor_of(n_rows, fill=np.nan):
    import torch
    return torch.full((max(n_rows, 1), 12), float(fill), dtype=torch.float32, device="cuda:0")


def all_bytes(hip, sc, desc):
    return [device_vertices(hip, sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)]


def info_tuple(i):
    return (i.actors, i.items, i.nodes, i.channels, i.upload_bytes, i.launches, i.read_backs, i.calls, i.refused_actor, i.refused_item)


def batch_tuple(i):
    return (i.items, i.blocks, i.vertices, i.launches, i.read_backs, i.calls, i.refused_item, i.refused_vertex, i.upload_bytes)


def evaluate(rt, clip, times, placement=None, sc=None):
    """One pose_actors call with one actor per time, instances only, nodes kept -> per actor (TRS, globals, joint matrices,
    instance transforms) as the device left them."""
    own = sc is None
    sc = sc or rt.Scene(0)
    cid = sc.attach_clip(clip)
    ni, i = clip.info.n_instances, clip.info
    out = tensor_of(ni * len(times))
    sc.pose_actors([(cid, t, placement, None, a * ni) for a, t in enumerate(times)], [], out, keep_nodes=True)
    xf = out.cpu().numpy().reshape(-1, 12)
    got = []
    for a in range(len(times)):
        trs, glob = sc.read_actor_nodes(a, i.n_nodes)
        got.append((trs, glob, sc.read_actor_matrices(a, i.n_joints), xf[a * ni:(a + 1) * ni]))
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.nodes, info.channels, info.launches, info.read_backs) == (len(times), 0, len(times) * i.n_nodes, len(times) * i.n_channels, 3, 1)
    sc.detach_clip(cid)
    if own:
        sc.close()
    return got


def check_against_host(rt, clip, times, placement=None, what=""):
    """Sampling under the contract, composition bit for bit from the device's own TRS -> (rotation components not bit equal, of)."""
    differ = total = 0
    for t, (trs, glob, jm, xf) in zip(times, evaluate(rt, clip, times, placement)):
        d, n = assert_trs_contract(trs, clip.sample_host(t), rotation_classes(clip, t), "%s t = %r" % (what, t))
        differ, total = differ + d, total + n
        want_jm, want_xf, bad = clip.compose_host(trs, placement)
        assert bad is None
        assert np.array_equal(bits(jm), bits(want_jm)), "%s t = %r: joint matrices" % (what, t)
        assert np.array_equal(bits(xf), bits(want_xf)), "%s t = %r: instance transforms" % (what, t)
    return differ, total


# ---- sampling and composition ------------------------------------------------------------------------------------------------------
def test_sampling_contract_and_composition_on_the_fixture(rt):
    g = rt.Gltf(CLIP_RIG)
    differ = total = 0
    for a in (-1, 0, 1):
        clip = g.bake_clip(a)
        times = [t for t in clip_times(clip) if not (a == 1 and t == 1.0)]          # the singular time has a test of its own
        for placement in (None, PLACEMENT):
            d, n = check_against_host(rt, clip, times, placement, "animation %d" % a)
            differ, total = differ + d, total + n
    print("interpolated rotation components not bit equal: %d of %d" % (differ, total))
    assert total > 1000 and differ * 1000 <= total


SHAPES = {"one node": dict(), "chain of 40": dict(chain=40, joints=3, channels=45, keys=3), "70 on a level": dict(fan=69, joints=5, channels=65, keys=2),
          "300 nodes": dict(chain=10, fan=288, joints=67, channels=130, keys=5), "1 joint, 1 key": dict(chain=2, joints=1, channels=3, keys=1),
          "64 keys": dict(chain=3, fan=2, joints=4, channels=9, keys=64), "65 keys": dict(chain=3, fan=2, joints=4, channels=9, keys=65)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(rt, tmp_path, name):
    path = str(tmp_path / "shape.glb")
    shape = SHAPES[name]
    n_nodes = shape_rig(path, **shape)
    g = rt.Gltf(path)
    clip = g.bake_clip(0 if shape.get("channels") else -1)
    i = clip.info
    assert (i.n_nodes, i.n_joints, i.n_channels) == (n_nodes, shape.get("joints", 0), shape.get("channels", 0))
    assert i.n_levels == (shape.get("chain", 0) or (1 if n_nodes > 1 else 0)) + 1
    last = 0.125 * (shape.get("keys", 2) - 1)
    times = [-0.5, 0.0, 0.01, 0.0625, 0.13, 0.5 * last + 0.003, last, last + 0.05, last + 1.0]
    times = [float(np.float32(t)) for t in times]
    for placement in (None, PLACEMENT):
        check_against_host(rt, clip, times, placement, name)
    # and the host rule is sr_gltf_pose here too
    for t in times[:4]:
        jm, xf = clip.pose_host(t)
        assert np.array_equal(bits(xf), bits(g.pose(clip.info.animation, t)[0]))
        if i.n_joints:
            assert np.array_equal(bits(jm), bits(g.pose(clip.info.animation, t, 0)[1]))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def host_step(rt, sc, c, clips_times, matrices_of=None):
    """The existing path for a crowd: per copy sr_gltf_pose (or the given matrices), one pose_meshes, one set_instances."""
    desc, g, keys, rigs, layout, rows, skins, _ = c
    items, instances = [], []
    for copy, (anim, t) in enumerate(clips_times):
        for b, skin in enumerate(skins):
            if skin >= 0:
                items.append((keys[copy][b], None, matrices_of[(copy, skin)] if matrices_of else g.pose(anim, t, skin)[1]))
        xf = g.pose(anim, t)[0]
        for b in range(g.n_blases):
            instances.append((keys[copy][b], [xf[i] for i in range(len(xf)) if c[7][i] == b]))
    sc.pose_meshes(items)
    sc.set_instances(instances)


def device_step(rt, sc, c, ids, clips_times, out, keep_nodes=False):
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ni = len(rows)
    actors = [(ids[anim], t, None, rows + np.uint32(copy * ni), 0) for copy, (anim, t) in enumerate(clips_times)]
    items = [it for copy in range(len(clips_times)) for it in skin_items(c, copy, copy)]
    sc.pose_actors(actors, items, out, keep_nodes=keep_nodes)
    sc.set_instances_device(layout, out)


def test_end_to_end_equals_the_host_fed_path(rt, hip):
    """Bit-equal class (static pose, STEP, exact key times): the same vertex bytes, structures and traced rays as sr_gltf_pose +
    pose_meshes + set_instances. Interpolated times: the same bytes as pose_meshes fed the matrices the device produced."""
    copies = 3
    a_sc, c = rigged(rt, CLIP_RIG, copies)
    b_sc, _ = rigged(rt, CLIP_RIG, copies)
    desc, g, keys = c[0], c[1], c[2]
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: b_sc.attach_clip(clip) for a, clip in clips.items()}
    assert sorted(ids.values()) == [1, 2, 3]
    out = tensor_of(copies * len(c[5]))
    rays = ray_grid(*RAYS)
    rd = rt.rays_to_device(rays)
    all_keys = [m.key for m in desc.meshes]
    # 2.0 is the last key of every channel of animation 0 and past the STEP channel's; 0.0 of animation 1 is a key of both channels
    for step, clips_times in enumerate([[(-1, 0.0), (-1, 5.0), (-1, -1.0)], [(0, 2.0), (0, 7.5), (1, 0.0)], [(0, -1.0), (1, 2.0), (-1, 0.0)]]):
        host_step(rt, a_sc, c, clips_times)
        device_step(rt, b_sc, c, ids, clips_times, out)
        assert all_bytes(hip, a_sc, desc) == all_bytes(hip, b_sc, desc), step
        assert_scenes_equal(rt, a_sc, b_sc, rays, rd, all_keys, "bit-equal class, step %d" % step)
    info = b_sc.actor_pose_info()
    assert info_tuple(info)[:4] == (copies, 2 * copies, sum(clips[a].info.n_nodes for a in (0, 1, -1)), sum(clips[a].info.n_channels for a in (0, 1, -1)))
    assert info_tuple(info)[5:] == (3, 1, 3, NONE, NONE)
    # interpolated times: feed the host path the matrices the device produced
    clips_times = [(0, 0.3), (0, 1.111), (1, 0.4)]
    device_step(rt, b_sc, c, ids, clips_times, out, keep_nodes=True)
    produced = {}
    for copy, (anim, t) in enumerate(clips_times):
        jm = b_sc.read_actor_matrices(copy, clips[anim].info.n_joints)
        for skin in (0, 1):
            first, n = clips[anim].skin(skin)
            produced[(copy, skin)] = jm[first:first + n].copy()
    host_step(rt, a_sc, c, clips_times, matrices_of=produced)
    assert all_bytes(hip, a_sc, desc) == all_bytes(hip, b_sc, desc)
    assert all_bytes(hip, b_sc, desc) != [m.vertices.tobytes() for m in desc.meshes]
    a_sc.close(); b_sc.close()


# ---- actors, clips, items --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_actors", [1, 2, 65, 257])
def test_many_actors_each_at_its_own_time(rt, hip, n_actors):
    """Actors beyond the copies drive no mesh (instances only); the first two drive the two copies' meshes."""
    copies = min(n_actors, 2)
    sc, c = rigged(rt, CLIP_RIG, copies)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clip = g.bake_clip(0)
    cid = sc.attach_clip(clip)
    ni = len(rows)
    times = [float(np.float32(2.0 * a / n_actors)) for a in range(n_actors)]
    out = tensor_of(ni * n_actors)
    perm = np.array([2, 0, 1], np.uint32)                                    # instance rows that permute
    actors = [(cid, t, PLACEMENT if a % 3 == 1 else None, perm + np.uint32(a * ni) if a % 2 else None, a * ni) for a, t in enumerate(times)]
    items = [it for copy in range(copies) for it in skin_items(c, copy, copy)]
    sc.pose_actors(actors, items, out, keep_nodes=True)
    xf = out.cpu().numpy().reshape(-1, 12)
    for a in sorted({0, 1, 63, 64, 65, 255, 256} & set(range(n_actors))):
        trs, _ = sc.read_actor_nodes(a, clip.info.n_nodes)
        assert_trs_contract(trs, clip.sample_host(times[a]), rotation_classes(clip, times[a]), "actor %d" % a)
        want_jm, want_xf, _ = clip.compose_host(trs, PLACEMENT if a % 3 == 1 else None)
        assert np.array_equal(bits(sc.read_actor_matrices(a, clip.info.n_joints)), bits(want_jm)), a
        got = xf[a * ni:(a + 1) * ni]
        assert np.array_equal(bits(got[perm] if a % 2 else got), bits(want_xf)), a
    info = sc.actor_pose_info()
    assert info_tuple(info)[:4] + info_tuple(info)[5:] == (n_actors, len(items), n_actors * clip.info.n_nodes, n_actors * clip.info.n_channels, 3, 1, 1, NONE, NONE)
    # the posed bytes are pose_meshes' fed the device's matrices
    twin, _ = rigged(rt, CLIP_RIG, copies)
    fed = []
    for copy in range(copies):
        jm = sc.read_actor_matrices(copy, clip.info.n_joints)
        fed += [(key, None, jm[clip.skin(skin)[0]:][:clip.skin(skin)[1]].copy()) for key, _, skin, _ in skin_items(c, copy, copy)]
    twin.pose_meshes(fed)
    assert all_bytes(hip, sc, desc) == all_bytes(hip, twin, desc)
    sc.close(); twin.close()


def test_items_of_every_kind_and_no_instance_tensor(rt, hip):
    """Two clips in one call, both skins of one actor, an item without a skin stage (morph only) beside actor-driven ones, a fused
    item (morph + skin), an actor no item names, and no instance tensor at all."""
    sc, c = rigged(rt, CLIP_RIG, 2)
    twin, _ = rigged(rt, CLIP_RIG, 2)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    deltas = {}
    for key in (keys[0][0], keys[1][1], keys[1][2]):                         # bar_a of copy 0 (fused), bar_b of copy 1, the prop of copy 1 (morph only)
        n = len(desc.meshes[[m.key for m in desc.meshes].index(key)].vertices)
        d = np.zeros((2, n), abi.MORPH_DELTA)
        d["position"][0, :, 1] = 0.125 * (1 + np.arange(n) % 3)
        d["position"][1, :, 0] = -0.0625
        d["normal"][1, :, 2] = 0.25
        deltas[key] = d
        for s in (sc, twin):
            s.set_mesh_morph(key, d)
    w = np.array([0.5, -0.25], np.float32)
    clips = [g.bake_clip(0), g.bake_clip(1)]
    ids = [sc.attach_clip(k) for k in clips]
    actors = [(ids[0], 0.77, None, None, 0), (ids[1], 1.6, None, None, 0), (ids[0], 1.9, None, None, 0)]      # the third drives nothing
    items = [(keys[0][0], 0, 0, w), (keys[0][1], 0, 1, None), (keys[1][0], 1, 0, None), (keys[1][1], 1, 1, w), (keys[1][2], 1, None, w)]
    sc.pose_actors(actors, items, None)
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.launches, info.refused_actor) == (3, 5, 3, NONE)
    jm = [sc.read_actor_matrices(a, clips[a].info.n_joints) for a in (0, 1)]
    assert refused(rt, lambda: sc.read_actor_nodes(0, 11))[0] == ERR_STATE        # no nodes were kept
    twin.pose_meshes([(keys[0][0], w, jm[0][0:3].copy()), (keys[0][1], None, jm[0][3:5].copy()), (keys[1][0], None, jm[1][0:3].copy()),
                      (keys[1][1], w, jm[1][3:5].copy()), (keys[1][2], w, None)])
    assert all_bytes(hip, sc, desc) == all_bytes(hip, twin, desc)
    for key in (keys[0][0], keys[1][1]):
        assert (sc.mesh_morph_info(key).posed, sc.mesh_skin_info(key).skinned) == (twin.mesh_morph_info(key).posed, twin.mesh_skin_info(key).skinned) == (1, 1)
    assert (sc.mesh_morph_info(keys[1][2]).posed, sc.mesh_skin_info(keys[0][1]).skinned) == (1, 1)
    # a pose_meshes call takes the staging block: the actor read-out says so
    sc.pose_meshes([(keys[0][1], None, jm[0][3:5].copy())])
    assert refused(rt, lambda: sc.read_actor_matrices(0, 5))[0] == ERR_STATE
    sc.close(); twin.close()


# ---- upload ---------------------------------------------------------------------------------------------------------------------------
def test_the_upload_does_not_grow_with_the_joints(rt, tmp_path):
    figures = []
    for joints in (3, 67):
        path = str(tmp_path / ("j%d.glb" % joints))
        shape_rig(path, chain=4, fan=70, joints=joints, channels=12, keys=3)
        sc, c = rigged(rt, path, 4)
        clip = c[1].bake_clip(0)
        cid = sc.attach_clip(clip)
        out = tensor_of(4 * len(c[5]))
        sc.pose_actors([(cid, 0.1 * a, None, None, a * len(c[5])) for a in range(4)], [it for a in range(4) for it in skin_items(c, a, a)], out)
        sc.pose_meshes([(key, None, clip.pose_host(0.1)[0]) for key in sorted(c[3])])
        figures.append((sc.actor_pose_info().upload_bytes, sc.pose_batch_info().upload_bytes, sc.actor_pose_info().items, sc.pose_batch_info().items))
        sc.close()
    (a3, b3, n3, m3), (a67, b67, n67, m67) = figures
    assert n3 == m3 == n67 == m67 == 4
    assert a3 == a67 == 4 * 64 + 16 + 4 * 80                              # item rows, block table, actor rows: no matrices, no instance rows
    assert b67 - b3 == 4 * 48 * 64 and a3 < b3 and a67 < b67


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_a_singular_actor_refuses_the_whole_call(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 3)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ids = {a: sc.attach_clip(g.bake_clip(a)) for a in (0, 1)}
    out = tensor_of(3 * len(rows))
    device_step(rt, sc, c, ids, [(0, 0.5), (0, 0.6), (0, 0.7)], out)
    sc.pose_meshes([(keys[0][0], None, g.pose(0, 0.25, 0)[1])])
    before = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], batch_tuple(sc.pose_batch_info()),
              sc.read_instance_tables()[1].tobytes())
    ni = len(rows)
    actors = [(ids[0], 0.9, None, None, 0), (ids[1], 1.0, None, None, ni), (ids[1], 1.0, None, None, 2 * ni)]          # animation 1 at t = 1: scale 0
    items = [it for copy in range(3) for it in skin_items(c, copy, copy)]
    assert refused(rt, lambda: sc.pose_actors(actors, items, out)) == (ERR_UNSUPPORTED, "pose_actors: actor 1: " + SINGULAR)
    assert refused(rt, lambda: g.pose(1, 1.0, 0)) == (ERR_UNSUPPORTED, "sr_gltf_pose: " + SINGULAR)
    info = sc.actor_pose_info()
    assert info_tuple(info)[5:] == (2, 1, 2, 1, NONE)
    after = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], batch_tuple(sc.pose_batch_info()),
             sc.read_instance_tables()[1].tobytes())
    assert before == after
    # the scene goes on: the same actors at a time that is not singular
    actors = [(cid, 0.5, None, None, base) for cid, _, _, _, base in actors]
    sc.pose_actors(actors, items, out)
    assert sc.actor_pose_info().launches == 3 and all_bytes(hip, sc, desc) != before[0]
    sc.close()


def test_host_refusals_come_before_any_device_work(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 2)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clip = g.bake_clip(0)
    cid = sc.attach_clip(clip)
    ni = len(rows)
    out = tensor_of(2 * ni, fill=7.0)
    good_actors = [(cid, 0.5, None, None, 0), (cid, 0.75, PLACEMENT, None, ni)]
    good_items = skin_items(c, 0, 0) + skin_items(c, 1, 1)
    sc.pose_actors(good_actors, good_items, out)
    state = (all_bytes(hip, sc, desc), info_tuple(sc.actor_pose_info()), batch_tuple(sc.pose_batch_info()), out.cpu().numpy().tobytes())
    bad_placement = PLACEMENT.copy()
    bad_placement[5] = np.inf
    A, I = "pose_actors: actor 1: ", "pose_actors: item 3: "
    k = good_items[3][0]
    cases = [
        ([good_actors[0], (99, 0.5, None, None, ni)], good_items, out, ERR_INVALID_ARG, A + "no clip is attached under this id"),
        ([good_actors[0], (cid, float("nan"), None, None, ni)], good_items, out, ERR_INVALID_ARG, A + "gltf: the time of a pose must be finite"),
        ([good_actors[0], (cid, 0.5, bad_placement, None, ni)], good_items, out, ERR_INVALID_ARG, A + "the placement has a component that is not finite"),
        ([good_actors[0], (cid, 0.5, None, np.arange(ni, dtype=np.uint32), 0)], good_items, None, ERR_INVALID_ARG, A + "instance rows or an instance base given without device instance transforms"),
        (good_actors, good_items[:3] + [(k, 2, 1, None)], out, ERR_INVALID_ARG, I + "actor 2 named, the call has 2 actors"),
        (good_actors, good_items[:3] + [(k, 1, 5, None)], out, ERR_INVALID_ARG, I + "skin 5 named, no instanced mesh of the actor's clip wears it"),
        (good_actors, good_items[:3] + [(k, 1, 0, None)], out, ERR_INVALID_ARG, I + "skin_mesh: 3 joint matrices given, the skin was attached with 2 joints"),
        (good_actors, good_items[:3] + [(good_items[0][0], 1, 0, None)], out, ERR_INVALID_ARG, I + "the key is named twice in the batch (first by item 0)"),
        (good_actors, good_items[:3] + [(k, 1, None, None)], out, ERR_INVALID_ARG, I + "pose_mesh: neither weights nor joint matrices given (one stage at least)"),
        (good_actors, good_items[:3] + [(12345, 1, 1, None)], out, ERR_INVALID_ARG, I + "skin_mesh: no mesh is registered under this key"),
    ]
    for actors, items, tensor, code, text in cases:
        assert refused(rt, lambda: sc.pose_actors(actors, items, tensor)) == (code, text)
        assert (all_bytes(hip, sc, desc), info_tuple(sc.actor_pose_info()), batch_tuple(sc.pose_batch_info()), out.cpu().numpy().tobytes()) == state, text
    assert refused(rt, lambda: sc.detach_clip(99)) == (ERR_INVALID_ARG, "detach_clip: no clip is attached under this id")
    sc.close()


# ---- interleaving, slots, attach and detach ---------------------------------------------------------------------------------------------
def test_interleaved_with_the_host_fed_calls(rt, hip):
    a_sc, c = rigged(rt, CLIP_RIG, 2)
    b_sc, _ = rigged(rt, CLIP_RIG, 2)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ids = {0: b_sc.attach_clip(g.bake_clip(0))}
    out = tensor_of(2 * len(rows))
    rays = ray_grid(*RAYS)
    rd = rt.rays_to_device(rays)
    jm = g.pose(0, 0.45, 0)[1]
    for step in range(2):
        clips_times = [(0, 2.0 + step), (0, -1.0 - step)]                     # clamped: bit-equal class
        host_step(rt, a_sc, c, clips_times)
        device_step(rt, b_sc, c, ids, clips_times, out)
        for s in (a_sc, b_sc):                                                # then the host-fed calls on both
            s.pose_meshes([(keys[1][0], None, jm)])
            s.skin_mesh(keys[0][1], g.pose(0, 0.3 + step, 1)[1])
        assert all_bytes(hip, a_sc, desc) == all_bytes(hip, b_sc, desc), step
    a_sc.set_instances(desc.instances); b_sc.set_instances(desc.instances)
    assert_scenes_equal(rt, a_sc, b_sc, rays, rd, [m.key for m in desc.meshes], "interleaved")
    assert [a_sc.mesh_skin_info(k).skinned for k in sorted(rigs)] == [b_sc.mesh_skin_info(k).skinned for k in sorted(rigs)]
    a_sc.close(); b_sc.close()


def test_detach_and_attach_again(rt):
    g = rt.Gltf(CLIP_RIG)
    sc = rt.Scene(0)
    clip = g.bake_clip(0)
    first, second = sc.attach_clip(clip), sc.attach_clip(clip)
    assert (first, second) == (1, 2)
    sc.detach_clip(first)
    assert refused(rt, lambda: sc.pose_actors([(first, 0.5, None, None, 0)], [], None))[1] == "pose_actors: actor 0: no clip is attached under this id"
    third = sc.attach_clip(g.bake_clip(1))
    assert third == 3                                                         # ids are not handed out again
    sc.pose_actors([(second, 0.5, None, None, 0), (third, 0.5, None, None, 0)], [], None, keep_nodes=True)
    for a, k in ((0, clip), (1, g.bake_clip(1))):
        assert_trs_contract(sc.read_actor_nodes(a, 11)[0], k.sample_host(0.5), rotation_classes(k, 0.5), "after the re-attach")
    sc.close()


def test_a_renderer_over_two_slots_equals_one(rt):
    import torch
    frames = []
    for devices in ([0], [0, 0]):
        r = rt.Renderer((96, 64), devices=devices)
        g = rt.Gltf(CLIP_RIG)
        loaded = r.load_scene(g)
        r.attach_skins(g, loaded)
        cid = r.attach_clip(g.bake_clip(0))
        keys = [int(k) for k in loaded.keys]
        items = [(keys[b], 0, g.blas_skin(b)[0], None) for b in range(g.n_blases) if g.blas_skin(b)[0] >= 0]
        out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:0")
        camera = ((0.0, 2.0, 7.0), (0.0, 1.0, 0.0), 45.0)
        for t in (0.0, 2.0):
            r.pose_actors([(cid, t, None, loaded.instance_rows(0), 0)], items, out)
            r.wait_frame(r.render_device_transforms(camera, loaded.layout(), out))
        info = r.actor_pose_info()
        assert (info.actors, info.items, info.launches, info.calls) == (1, 2, 3, 2)
        want = loaded.grouped(g.pose(0, 2.0)[0])
        assert np.array_equal(bits(out.cpu().numpy()), bits(np.array([t for _, ts in want for t in ts], np.float32)))
        frames.append(r.render_to_host_memory(camera, want).copy())
        r.close()
    assert np.array_equal(frames[0], frames[1])
