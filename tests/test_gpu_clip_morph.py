"""Morph weights from baked clips on the device (sr_scene_pose_actors with SR_ACTOR_CLIP_WEIGHTS: clip_weights_kernel samples an
item's morph set at its actor's time and compacts the weights that are not 0 into the active list pose_batch_kernel reads). The
reference is the host rule sr_clip_weights_host, itself held to sr_gltf_morph_weights bit for bit by test_clip_morph_host.py, and
the host's compaction of it. The arithmetic is +, -, x, / on fp32 and fp64 with no libm, so the contract is equality: count,
indices and weight bits, with no tolerance and no case left out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_morph_util import BIG, MORPH_BAR, ONE, TWO, available_sets, bits, compact, many_targets, set_times  # noqa: E402
from clip_util import crowd  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402
from test_gpu_mesh_update import assert_frames_equal, one_frame  # noqa: E402
from test_gpu_mesh_update_device import assert_scenes_equal, ray_grid  # noqa: E402

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
RAYS = ((-3.0, -1.0), (3.0, 4.0))


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


@pytest.fixture(scope="module")
def many(rt, tmp_path_factory):
    """The generated file (sets of 130, 1 and 2 targets) as a crowd of 9 copies with every morph attached, its two animations
    baked and attached -> (scene, crowd tuple, {animation: (clip, id)})."""
    path = str(tmp_path_factory.mktemp("clip_morph") / "many.glb")
    many_targets(path)
    sc, c, _ = morphed(rt, path, 9)
    clips = {}
    for a in (0, 1):
        clip = c[1].bake_clip(a)
        clips[a] = (clip, sc.attach_clip(clip))
    yield sc, c, clips
    sc.close()


def refused(rt, call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def morphed(rt, path, copies=1):
    """A scene of `copies` copies of a file with every rig and every morph attached -> (scene, the crowd() tuple, {blas: targets})."""
    c = crowd(rt, path, copies)
    desc, g, keys = c[0], c[1], c[2]
    sc = rt.Scene(0).load(desc)
    for key, (inf, nj) in c[3].items():
        sc.set_mesh_skin(key, inf, nj)
    targets = {}
    for b in range(g.n_blases):
        d = g.blas_morph(b)[0]
        if d is not None:
            targets[b] = len(d)
            for copy in range(copies):
                sc.set_mesh_morph(keys[copy][b], d)
    return sc, c, targets


def tensor_of(n_rows):
    import torch
    return torch.zeros((max(n_rows, 1), 12), dtype=torch.float32, device="cuda:0")


def all_bytes(hip, sc, desc):
    return [device_vertices(hip, sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)]


def info_tuple(i):
    return (i.actors, i.items, i.nodes, i.channels, i.upload_bytes, i.launches, i.read_backs, i.calls, i.refused_actor, i.refused_item, i.weight_items)


def morph_tuple(sc, key):
    i = sc.mesh_morph_info(key)
    return (i.n_targets, i.posed, i.n_active, i.first_bad)


def pose_and_check(rt, sc, clip, cid, plan):
    """One call: an actor and a morph-only clip-weighted item for every (key, blas, time) of the plan. Every item's active list as
    the posing kernel read it is the host's compaction of the host rule: count, indices, weight bits."""
    actors = [(cid, t, None, None, 0) for _, _, t in plan]
    items = [(key, a, None, rt.ClipWeights(b)) for a, (key, b, _) in enumerate(plan)]
    sc.pose_actors(actors, items, None)
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.weight_items, info.launches, info.read_backs, info.refused_item) == (len(plan), len(plan), len(plan), 4, 1, NONE)
    for i, (key, b, t) in enumerate(plan):
        want_at, want_w = compact(clip.weights_host(t, b))
        got_at, got_w = sc.read_item_active(i, clip.morph(b)["n_targets"])
        assert got_at.tolist() == want_at.tolist(), (b, t)
        assert np.array_equal(bits(got_w), bits(want_w)), (b, t)
        assert sc.mesh_morph_info(key).n_active == len(want_at), (b, t)


# ---- the contract ---------------------------------------------------------------------------------------------------------------------
def test_active_lists_equal_the_host_rule_on_the_fixture(rt):
    """Every available set of every animation of morph_bar.glb (and the static pose) over the whole grid of times."""
    copies = 8
    sc, c, targets = morphed(rt, MORPH_BAR, copies)
    g, keys = c[1], c[2]
    assert targets == {0: 3, 1: 2}
    n_cases = 0
    for a in (-1, 0, 1):
        clip = g.bake_clip(a)
        cid = sc.attach_clip(clip)
        sets = available_sets(clip, g.n_blases)
        assert sets == ([1] if a == 1 else [0, 1])
        times = sorted({t for b in sets for t in set_times(clip, b)})
        for first in range(0, len(times), copies):
            plan = [(keys[copy][b], b, t) for copy, t in enumerate(times[first:first + copies]) for b in sets]
            pose_and_check(rt, sc, clip, cid, plan)
            n_cases += len(plan)
    assert n_cases >= 90                                                      # the grid is not empty: 97 (set, time) pairs
    sc.close()


@pytest.mark.parametrize("animation", [0, 1], ids=["LINEAR", "STEP"])
def test_chunks_of_64_and_ordered_compaction(rt, hip, many, animation):
    """The set of 130 targets (chunks of 64 + 64 + 2) whose keys are exactly 0 at targets 0, 63, 64, 127, 128 and 129 at some
    times and not at others, with a -0 key and an all-zero time; the one-target and the one-key sets beside it."""
    sc, c, clips = many
    desc, g, keys = c[0], c[1], c[2]
    clip, cid = clips[animation]
    sets = available_sets(clip, g.n_blases)
    assert sets == [BIG, ONE, TWO]
    times = sorted({t for b in sets for t in set_times(clip, b)})
    assert 0.0 in times and 0.5 in times and 0.75 in times
    for first in range(0, len(times), 9):
        chunk = times[first:first + 9]
        pose_and_check(rt, sc, clip, cid, [(keys[copy][b], b, t) for copy, t in enumerate(chunk) for b in sets])
        for copy, t in enumerate(chunk):
            if t <= 0.0:                                                     # key 0 is all zeros: nothing is active, the posed bytes are the morph base
                slot = [m.key for m in desc.meshes].index(keys[copy][BIG])
                assert sc.mesh_morph_info(keys[copy][BIG]).n_active == 0
                assert device_vertices(hip, sc, slot, 4).tobytes() == desc.meshes[slot].vertices.tobytes()
    # exactly at key 1 the -0 of target 5 and the zeros at the chunk ends are left out
    at = sc_active(rt, sc, clip, cid, keys[0][BIG], BIG, 0.5)
    assert 5 not in at and 63 not in at and 1 in at


def sc_active(rt, sc, clip, cid, key, blas, t):
    sc.pose_actors([(cid, t, None, None, 0)], [(key, 0, None, rt.ClipWeights(blas))], None)
    return sc.read_item_active(0, clip.morph(blas)["n_targets"])[0].tolist()


def test_nine_sets_in_one_call(rt, many):
    """Nine items of the big set: two full blocks of four waves and one wave of a third, each actor at its own time, one before the
    first key and one after the last."""
    sc, c, clips = many
    keys = c[2]
    clip, cid = clips[0]
    times = [-1.0, 0.0, 0.25, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), 0.75, 1.0, 1.5, 3.0]
    pose_and_check(rt, sc, clip, cid, [(keys[copy][BIG], BIG, t) for copy, t in enumerate(times)])
    counts = [sc.mesh_morph_info(keys[copy][BIG]).n_active for copy in range(9)]
    assert counts[:2] == [0, 0] and counts[2] == 123 and counts[3] == 123 and counts[4] == 130 and counts[6] == 130 and counts[8] == 65


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_equals_host_weights(rt, hip, blue_noise):
    """The fused item (mesh 0 on skin 0) and the morph-only item (mesh 1) of morph_bar.glb: scene A takes host weights from
    sr_gltf_morph_weights, scene B the clip's, in the same call otherwise. Vertex bytes, morph figures, structures, traced rays
    and a frame are equal."""
    a_sc, c, _ = morphed(rt, MORPH_BAR)
    b_sc, _, _ = morphed(rt, MORPH_BAR)
    desc, g, keys, layout, rows = c[0], c[1], c[2], c[4], c[5]
    desc.camera_pos, desc.camera_target = (0.8, 1.4, 7.0), (0.8, 1.0, 0.0)
    clip = g.bake_clip(0)
    ids = [s.attach_clip(clip) for s in (a_sc, b_sc)]
    outs = [tensor_of(len(rows)), tensor_of(len(rows))]
    k0, k1 = keys[0][0], keys[0][1]
    rays = ray_grid(*RAYS)
    rd = rt.rays_to_device(rays)
    for step, t in enumerate([0.0, 0.3, 0.4, 1.111, 1.5, 2.5]):
        a_sc.pose_actors([(ids[0], t, None, rows, 0)], [(k0, 0, 0, g.morph_weights(0, t, 0)), (k1, 0, None, g.morph_weights(0, t, 1))], outs[0])
        b_sc.pose_actors([(ids[1], t, None, rows, 0)], [(k0, 0, 0, rt.ClipWeights(0)), (k1, 0, None, rt.ClipWeights(1))], outs[1])
        assert (a_sc.actor_pose_info().launches, b_sc.actor_pose_info().launches) == (3, 4)
        assert all_bytes(hip, a_sc, desc) == all_bytes(hip, b_sc, desc), t
        for key in (k0, k1):
            assert morph_tuple(a_sc, key) == morph_tuple(b_sc, key) and morph_tuple(b_sc, key)[1] == step + 1, (t, key)
        assert a_sc.mesh_skin_info(k0).skinned == b_sc.mesh_skin_info(k0).skinned == step + 1
        assert np.array_equal(bits(outs[0].cpu().numpy()), bits(outs[1].cpu().numpy()))
        a_sc.set_instances_device(layout, outs[0]); b_sc.set_instances_device(layout, outs[1])
        assert_scenes_equal(rt, a_sc, b_sc, rays, rd, [m.key for m in desc.meshes], "t = %r" % t)
    assert all_bytes(hip, b_sc, desc) != [m.vertices.tobytes() for m in desc.meshes]
    assert_frames_equal(one_frame(rt, a_sc, desc, 64, 48, blue_noise), one_frame(rt, b_sc, desc, 64, 48, blue_noise), "a frame after the last step")
    a_sc.close(); b_sc.close()


def test_a_mixed_call(rt, hip):
    """Clip-weighted, host-weighted, skin-only items together: the meshes that do not take clip weights get the bytes of the same
    call without the clip-weighted items; the figures count the weights kernel only where it ran."""
    sc, c, _ = morphed(rt, MORPH_BAR, 3)
    twin, _, _ = morphed(rt, MORPH_BAR, 3)
    desc, g, keys = c[0], c[1], c[2]
    clip = g.bake_clip(0)
    cid, tid = sc.attach_clip(clip), twin.attach_clip(clip)
    times = [0.7, 1.3, 0.4]
    w1, w0 = g.morph_weights(0, 0.9, 1), g.morph_weights(0, 1.7, 0)
    assert len(compact(w1)[0]) == 1 and len(compact(w0)[0]) == 3
    others = [(keys[0][1], 0, None, w1), (keys[1][0], 1, 0, None), (keys[2][0], 2, 0, w0)]        # host-weighted, skin-only, host-weighted and fused
    mixed = [(keys[0][0], 0, 0, rt.ClipWeights(0)), others[0], others[1], (keys[1][1], 1, None, rt.ClipWeights(1)), others[2]]
    sc.pose_actors([(cid, t, None, None, 0) for t in times], mixed, None)
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.launches, info.read_backs, info.weight_items, info.refused_item) == (3, 5, 4, 1, 2, NONE)
    for i, (b, t) in ((0, (0, times[0])), (3, (1, times[1]))):              # the clip-weighted items: the host rule's list
        want_at, want_w = compact(clip.weights_host(t, b))
        got_at, got_w = sc.read_item_active(i, 3)
        assert got_at.tolist() == want_at.tolist() and np.array_equal(bits(got_w), bits(want_w))
    for i, w in ((1, w1), (4, w0)):                                          # the host-weighted items: what the host uploaded
        got_at, got_w = sc.read_item_active(i, 3)
        assert got_at.tolist() == compact(w)[0].tolist() and np.array_equal(bits(got_w), bits(compact(w)[1]))
    assert sc.read_item_active(2, 3)[0].size == 0                             # no morph stage
    twin.pose_actors([(tid, t, None, None, 0) for t in times], others, None)
    assert twin.actor_pose_info().launches == 3 and twin.actor_pose_info().weight_items == 0
    got, want = all_bytes(hip, sc, desc), all_bytes(hip, twin, desc)
    order = [m.key for m in desc.meshes]
    for key, _, _, _ in others:
        assert got[order.index(key)] == want[order.index(key)], key
    for key in (keys[0][0], keys[1][1]):                                      # and the clip-weighted ones were posed
        assert got[order.index(key)] != want[order.index(key)] and sc.mesh_morph_info(key).posed == 1
    # the clip-weighted meshes against host weights of the same times
    twin.pose_actors([(tid, t, None, None, 0) for t in times], [(keys[0][0], 0, 0, g.morph_weights(0, times[0], 0)), (keys[1][1], 1, None, g.morph_weights(0, times[1], 1))], None)
    assert all_bytes(hip, sc, desc) == all_bytes(hip, twin, desc)
    # a call without clip weights afterwards is the call it has always been
    sc.pose_actors([(cid, t, None, None, 0) for t in times], others, None)
    info = sc.actor_pose_info()
    assert (info.launches, info.read_backs, info.weight_items, info.upload_bytes) == (3, 1, 0, twin_upload(twin, tid, times, others))
    sc.close(); twin.close()


def twin_upload(twin, tid, times, items):
    twin.pose_actors([(tid, t, None, None, 0) for t in times], items, None)
    return twin.actor_pose_info().upload_bytes


def test_the_upload_does_not_grow_with_the_targets(rt, many):
    sc, c, clips = many
    keys = c[2]
    clip, cid = clips[0]
    sizes = {}
    for b in (TWO, BIG):
        sc.pose_actors([(cid, 0.75, None, None, 0)], [(keys[0][b], 0, None, rt.ClipWeights(b))], None)
        sizes[b] = sc.actor_pose_info().upload_bytes
        assert len(sc.read_item_active(0, 130)[0]) == (2 if b == TWO else 130)
    assert sizes[TWO] == sizes[BIG] == 64 + 16 + 80 + 32                      # an item row, the block table, an actor row, a weight row: no weights, no slots


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_come_before_any_device_work(rt, hip):
    sc, c, _ = morphed(rt, MORPH_BAR, 2)
    desc, g, keys = c[0], c[1], c[2]
    cid, spline = sc.attach_clip(g.bake_clip(0)), sc.attach_clip(g.bake_clip(1))
    actors = [(cid, 0.5, None, None, 0), (spline, 0.5, None, None, 0)]
    good = [(keys[0][0], 0, 0, rt.ClipWeights(0)), (keys[0][1], 0, None, rt.ClipWeights(1)), (keys[1][1], 1, None, rt.ClipWeights(1))]
    sc.pose_actors(actors, good, None)
    state = lambda: (all_bytes(hip, sc, desc), info_tuple(sc.actor_pose_info()), [morph_tuple(sc, k) for cp in keys for k in cp[:2]])   # noqa: E731
    before = state()
    assert before[1][5:] == (4, 1, 1, NONE, NONE, 3)
    I = "pose_actors: item 2: "
    k = keys[1][0]
    both = rt.ActorArgs(actors, good[:2] + [(k, 1, 0, g.morph_weights(0, 0.5, 0))])
    both.items[2].morph = abi.actor_clip_weights(0)
    cases = [
        (both, ERR_INVALID_ARG, I + "host weights given together with SR_ACTOR_CLIP_WEIGHTS (one source of weights at most)"),
        (good[:2] + [(keys[1][1], 2, None, rt.ClipWeights(1))], ERR_INVALID_ARG, I + "actor 2 named, the call has 2 actors"),
        (good[:2] + [(keys[1][1], 0, None, rt.ClipWeights(2))], ERR_INVALID_ARG, I + "the weights of blas 2 named, the actor's clip has no morph set for it"),
        (good[:2] + [(k, 1, 0, rt.ClipWeights(0))], ERR_UNSUPPORTED, I + CUBIC),
        (good[:2] + [(keys[1][1], 0, None, rt.ClipWeights(0))], ERR_INVALID_ARG, I + "pose_mesh: 3 weights given, the morph was attached with 2 targets"),
        (good[:2] + [(keys[1][2], 0, None, rt.ClipWeights(1))], ERR_INVALID_ARG, I + "pose_mesh: the mesh has no morph targets (sr_scene_set_mesh_morph attaches them)"),
    ]
    for items, code, text in cases:
        call = (lambda: sc.pose_actors(items)) if isinstance(items, rt.ActorArgs) else (lambda: sc.pose_actors(actors, items, None))
        assert refused(rt, call) == (code, text)
        assert state() == before, text
    assert refused(rt, lambda: sc.read_item_active(3))[0] == ERR_INVALID_ARG
    sc.pose_meshes([(keys[0][1], g.morph_weights(0, 0.1, 1), None)])         # another pose call takes the staging block
    assert refused(rt, lambda: sc.read_item_active(0)) == (ERR_STATE, "read_item_active: the staging block does not hold a sr_scene_pose_actors call")
    sc.close()


def test_a_non_finite_morphed_vertex_refuses_the_whole_call(rt, hip, tmp_path):
    """Finite deltas of 3e38 under a clip weight of 2 (the one-key channel of the one-target set): the blend overflows on the
    device, and the call is refused as sr_scene_pose_meshes refuses it. No mesh has changed."""
    path = str(tmp_path / "many.glb")
    many_targets(path)
    sc, c, _ = morphed(rt, path)
    desc, g, keys = c[0], c[1], c[2]
    clip = g.bake_clip(0)
    cid = sc.attach_clip(clip)
    assert clip.weights_host(0.5, ONE).tolist() == [2.0]
    d = np.zeros((1, 4), abi.MORPH_DELTA)
    d["position"][0, :, 1] = 3e38
    d["position"][0, 0, 1] = 1.0                                              # vertex 0 stays finite: the lowest bad vertex is 1
    sc.set_mesh_morph(keys[0][ONE], d)
    want = refused(rt, lambda: sc.pose_meshes([(keys[0][TWO], clip.weights_host(0.5, TWO), None), (keys[0][ONE], np.array([2.0], np.float32), None)]))
    assert want == (ERR_INVALID_ARG, "pose_meshes: item 1: update_mesh: vertex 1 has a non-finite position")
    before = (all_bytes(hip, sc, desc), [morph_tuple(sc, k)[:2] for k in keys[0]])
    assert before[0] == [m.vertices.tobytes() for m in desc.meshes]
    items = [(keys[0][TWO], 0, None, rt.ClipWeights(TWO)), (keys[0][ONE], 0, None, rt.ClipWeights(ONE))]
    got = refused(rt, lambda: sc.pose_actors([(cid, 0.5, None, None, 0)], items, None))
    assert got == (want[0], want[1].replace("pose_meshes", "pose_actors"))
    info = sc.actor_pose_info()
    assert (info.launches, info.read_backs, info.weight_items, info.refused_item, info.refused_actor) == (3, 1, 2, 1, NONE)
    assert sc.mesh_morph_info(keys[0][ONE]).first_bad == 1
    assert (all_bytes(hip, sc, desc), [morph_tuple(sc, k)[:2] for k in keys[0]]) == before          # no mesh has changed, none counts a pose
    sc.pose_actors([(cid, 0.5, None, None, 0)], items[:1], None)              # the scene goes on
    assert sc.actor_pose_info().launches == 4 and sc.mesh_morph_info(keys[0][TWO]).posed == 1
    sc.close()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------
def test_a_renderer_over_two_slots_equals_one(rt):
    import torch
    frames = []
    for devices in ([0], [0, 0]):
        r = rt.Renderer((96, 64), devices=devices)
        g = rt.Gltf(MORPH_BAR)
        loaded = r.load_scene(g)
        r.attach_skins(g, loaded)
        r.attach_morphs(g, loaded)
        cid = r.attach_clip(g.bake_clip(0))
        keys = [int(k) for k in loaded.keys]
        items = [(keys[0], 0, 0, rt.ClipWeights(0)), (keys[1], 0, None, rt.ClipWeights(1))]
        out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:0")
        camera = ((0.8, 1.4, 7.0), (0.8, 1.0, 0.0), 45.0)
        for t in (0.3, 2.0):
            r.pose_actors([(cid, t, None, loaded.instance_rows(0), 0)], items, out)
            r.wait_frame(r.render_device_transforms(camera, loaded.layout(), out))
        info = r.actor_pose_info()
        assert (info.actors, info.items, info.launches, info.weight_items, info.calls) == (1, 2, 4, 2, 2)
        first = r.replica_scene(0)
        assert [first.mesh_morph_info(keys[b]).n_active for b in (0, 1)] == [len(compact(g.morph_weights(0, 2.0, b))[0]) for b in (0, 1)]
        frames.append(r.render_to_host_memory(camera, loaded.grouped(g.pose(0, 2.0)[0])).copy())
        r.close()
    assert np.array_equal(frames[0], frames[1])
    assert (frames[0] != 0).any()
