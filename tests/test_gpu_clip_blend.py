"""Scene.pose_actors_blended / Renderer.pose_actors_blended (sr_scene_pose_actors_blended: clip_blend_kernel samples both of an
actor's clips, blends the per-node records, composes once and writes where clip_pose_kernel writes; clip_blend_weights_kernel
blends the morph weights). The contract, stage by stage:
  - at the end weights a blended call is byte-equal to the plain pose_actors call with the one clip, device against device;
  - each source is sampled under pose_actors' contract against sr_clip_sample_host (at most 1 in 1000 interpolated rotation
    components other than bit equal: the clips and times on which test_gpu_clip_pose.py holds clip_pose_kernel to that cap);
  - the blended records are bit equal to sr_clip_blend_host of the device's own sources, and the globals, joint matrices and instance
    transforms to sr_clip_compose_records_host of the device's own blended records: no libm in those stages, no tolerance;
  - where both sources are in the bit-equal sampling class, the whole chain is bit equal to sr_clip_pose_blend_host;
  - the blended active lists are bit equal to the compaction of sr_clip_blend_weights_host."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_util import CLIP_RIG, SKINNED_BAR, assert_trs_contract, bits, clip_times, crowd, rotation_classes, shape_rig  # noqa: E402
from clip_morph_util import MORPH_BAR, compact, set_times  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402
from test_gpu_mesh_update_device import assert_scenes_equal, ray_grid  # noqa: E402

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
SINGULAR = "gltf: the transform of the skinned mesh's node is singular"
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
PLACEMENT = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)
RAYS = ((-2.2, -0.2), (2.4, 3.2))           # the rig's extent: the bars are thin
F32 = np.float32
INNER = [float(np.nextafter(F32(0), F32(1))), float(F32(1.0) / F32(3.0)), 0.5, float(np.nextafter(F32(1), F32(0)))]


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


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def rigged(rt, path, copies=1, morphs=False):
    """A scene of `copies` copies of a file with every rig (and, asked for, every morph) attached -> (scene, the crowd() tuple)."""
    c = crowd(rt, path, copies)
    sc = rt.Scene(0).load(c[0])
    for key, (inf, nj) in c[3].items():
        sc.set_mesh_skin(key, inf, nj)
    for b in range(c[1].n_blases if morphs else 0):
        d = c[1].blas_morph(b)[0]
        for copy in range(copies if d is not None else 0):
            sc.set_mesh_morph(c[2][copy][b], d)
    return sc, c


def skin_items(c, copy, actor):
    return [(c[2][copy][b], actor, skin, None) for b, skin in enumerate(c[6]) if skin >= 0]


def tensor_of(n_rows, fill=np.nan):
    import torch
    return torch.full((max(n_rows, 1), 12), float(fill), dtype=torch.float32, device="cuda:0")


def all_bytes(hip, sc, desc):
    return [device_vertices(hip, sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)]


def static_class(clip, t):
    """Every rotation of the clip is in the bit-equal sampling class at t."""
    return not rotation_classes(clip, t).any()


def read_actor(sc, a, info, sources=True):
    trs, glob = sc.read_actor_nodes(a, info.n_nodes)
    src = sc.read_actor_sources(a, info.n_nodes) if sources else (None, None)
    return trs, glob, sc.read_actor_matrices(a, info.n_joints), src[0], src[1]


def check_inner_weights(rt, clip_a, clip_b, pairs, weights, what):
    """One call per weight, an actor per (time a, time b) pair, nodes and sources kept: the contract of the module's docstring ->
    (rotation components not bit equal, interpolated rotation components, actors checked against pose_blend_host)."""
    sc = rt.Scene(0)
    ida, idb = sc.attach_clip(clip_a), sc.attach_clip(clip_b)
    i = clip_a.info
    ni = i.n_instances
    differ = total = whole = 0
    want_a = [clip_a.sample_host(ta) for ta, _ in pairs]
    want_b = [clip_b.sample_host(tb) for _, tb in pairs]
    instance_nodes = clip_a.layout()[2]
    for w in weights:
        out = tensor_of(ni * len(pairs))
        actors = [(ida, ta, idb, tb, w, PLACEMENT if k % 2 else None, None, k * ni) for k, (ta, tb) in enumerate(pairs)]
        sc.pose_actors_blended(actors, [], out, keep_nodes=True, keep_sources=True)
        info = sc.actor_pose_info()
        assert (info.actors, info.items, info.nodes, info.channels, info.launches, info.read_backs) == \
            (len(pairs), 0, len(pairs) * i.n_nodes, len(pairs) * (i.n_channels + clip_b.info.n_channels), 3, 1)
        xf = out.cpu().numpy().reshape(-1, 12)
        for k, (ta, tb) in enumerate(pairs):
            label = "%s t = (%r, %r) w = %r" % (what, ta, tb, w)
            placement = PLACEMENT if k % 2 else None
            trs, glob, jm, src_a, src_b = read_actor(sc, k, i)
            for src, want, clip, t in ((src_a, want_a[k], clip_a, ta), (src_b, want_b[k], clip_b, tb)):
                d, n = assert_trs_contract(src, want, rotation_classes(clip, t), label)
                differ, total = differ + d, total + n
            assert same(trs, rt.clip_blend_host(src_a, src_b, w)), label + ": the blended records"
            want_jm, want_xf, bad = clip_a.compose_records_host(trs, placement)
            assert bad is None, label
            assert same(jm, want_jm), label + ": joint matrices"
            assert same(xf[k * ni:(k + 1) * ni], want_xf), label + ": instance transforms"
            assert same(glob[instance_nodes][:, :12], clip_a.compose_records_host(trs)[1]), label + ": globals"
            if static_class(clip_a, ta) and static_class(clip_b, tb):
                host_jm, host_xf = clip_a.pose_blend_host(ta, clip_b, tb, w, placement)
                assert same(jm, host_jm) and same(xf[k * ni:(k + 1) * ni], host_xf), label + ": the whole chain against pose_blend_host"
                whole += 1
    sc.close()
    return differ, total, whole


# ---- 1. end weights, device against device ------------------------------------------------------------------------------------------
def test_end_weights_equal_the_plain_call(rt, hip):
    copies = 8
    scenes = [rigged(rt, CLIP_RIG, copies) for _ in range(2)]
    (blend_sc, c), (plain_sc, _) = scenes
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: blend_sc.attach_clip(clip) for a, clip in clips.items()}
    assert ids == {a: plain_sc.attach_clip(clip) for a, clip in clips.items()}
    ni, i = len(rows), clips[0].info
    times = (0.3, 0.9, 1.6)                                                    # collapse is singular at 1.0: that has a test of its own
    perm = np.array([2, 0, 1], np.uint32)
    blended, plain = [], []
    for a, b in itertools.product((-1, 0, 1), repeat=2):
        for k, t in enumerate(times):
            other = times[(k + 1) % 3]
            for w in (0.0, 1.0):
                n = len(blended)
                placement, inst = (PLACEMENT if n % 2 else None), (perm + np.uint32(n * ni) if n % 4 in (1, 2) else None)
                blended.append((ids[a], t, ids[b], other, w, placement, inst, n * ni))
                plain.append((ids[b], other, placement, inst, n * ni) if w else (ids[a], t, placement, inst, n * ni))
    assert len(blended) == 54
    drivers = list(range(0, 54, 7))                                            # eight of the actors drive the eight copies' meshes
    items = [it for copy, a in enumerate(drivers) for it in skin_items(c, copy, a)]
    outs = [tensor_of(ni * 54), tensor_of(ni * 54)]
    blend_sc.pose_actors_blended(blended, items, outs[0], keep_nodes=True)
    plain_sc.pose_actors(plain, items, outs[1], keep_nodes=True)
    assert same(outs[0].cpu().numpy(), outs[1].cpu().numpy())
    assert not np.isnan(outs[0].cpu().numpy()).any()
    for a in range(54):
        got, want = read_actor(blend_sc, a, i, sources=False), read_actor(plain_sc, a, i, sources=False)
        for name, x, y in zip(("TRS", "globals", "joint matrices"), got, want):
            assert same(x, y), (a, name)
    assert all_bytes(hip, blend_sc, desc) == all_bytes(hip, plain_sc, desc)
    assert all_bytes(hip, blend_sc, desc) != [m.vertices.tobytes() for m in desc.meshes]
    bi, pi = blend_sc.actor_pose_info(), plain_sc.actor_pose_info()
    assert (bi.actors, bi.items, bi.nodes, bi.launches, bi.read_backs, bi.calls, bi.refused_actor) == (pi.actors, pi.items, pi.nodes, pi.launches, pi.read_backs, pi.calls, NONE)
    assert bi.upload_bytes - pi.upload_bytes == 54 * (96 - 80)                 # the rows are all that grows
    assert refused(rt, lambda: blend_sc.read_actor_sources(0, i.n_nodes))[0] == ERR_STATE          # no sources were kept
    blend_sc.close(); plain_sc.close()


# ---- 2. the contract at inner weights ----------------------------------------------------------------------------------------------------
def test_contract_at_inner_weights_on_the_fixture(rt):
    g = rt.Gltf(CLIP_RIG)
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    times = {a: [t for t in clip_times(clip) if not (a == 1 and t == 1.0)] for a, clip in clips.items()}     # the singular time has a test of its own
    differ = total = whole = 0
    for a, b in ((0, 1), (1, 0), (0, -1), (-1, 1), (0, 0)):
        ta, tb = times[a], times[b]
        pairs = [(ta[k % len(ta)], tb[(5 * k + 3) % len(tb)]) for k in range(max(len(ta), len(tb)))]
        d, n, wh = check_inner_weights(rt, clips[a], clips[b], pairs, INNER, "animations %d and %d" % (a, b))
        differ, total, whole = differ + d, total + n, whole + wh
    print("interpolated rotation components of the sources not bit equal: %d of %d; %d actors held to pose_blend_host" % (differ, total, whole))
    assert whole >= 20
    assert total > 1000 and differ * 1000 <= total


# ---- 3. the wide rig: every strided loop runs a second round ---------------------------------------------------------------------------
def test_contract_on_a_rig_wider_than_the_block(rt, tmp_path):
    path = str(tmp_path / "wide.glb")
    n_nodes = shape_rig(path, chain=20, fan=300, joints=90, channels=330, keys=2)
    g = rt.Gltf(path)
    moving, still = g.bake_clip(0), g.bake_clip(-1)
    i = moving.info
    assert 256 < n_nodes == i.n_nodes <= 384 and i.n_channels == 330 and i.n_joints * 3 > 256 and max(np.bincount(moving.layout()[0]["level"])) > 256
    pairs = [(float(F32(0.07)), float(F32(0.3))), (float(F32(0.3)), float(F32(0.07)))]       # between the keys, and past every channel's last key
    weights = [float(F32(1.0) / F32(3.0)), 0.5]
    _, total, whole = check_inner_weights(rt, moving, still, pairs, weights, "moving into still")
    _, total2, whole2 = check_inner_weights(rt, still, moving, pairs, weights, "still into moving")
    assert total > 1000 and total2 > 1000 and whole == 2 and whole2 == 2


# ---- 4. posed geometry -------------------------------------------------------------------------------------------------------------------
def test_posed_geometry_is_pose_meshes_fed_the_blended_matrices(rt, hip):
    copies = 3
    (sc, c), (twin, _) = rigged(rt, CLIP_RIG, copies), rigged(rt, CLIP_RIG, copies)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: sc.attach_clip(clip) for a, clip in clips.items()}
    ni, i = len(rows), clips[0].info
    out = tensor_of(copies * ni)
    actors = [(ids[0], 0.4, ids[1], 0.7, 0.25, None, rows, 0), (ids[-1], 0.0, ids[0], 1.3, 0.5, None, rows + np.uint32(ni), 0),
              (ids[1], 1.9, ids[0], 0.1, float(F32(0.8)), None, rows + np.uint32(2 * ni), 0)]
    items = [it for copy in range(copies) for it in skin_items(c, copy, copy)]
    sc.pose_actors_blended(actors, items, out)
    sc.set_instances_device(layout, out)
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.launches, info.read_backs, info.refused_actor, info.refused_item) == (3, 2 * copies, 3, 1, NONE, NONE)
    fed = []
    for copy in range(copies):
        jm = sc.read_actor_matrices(copy, i.n_joints)
        fed += [(key, None, jm[clips[0].skin(skin)[0]:][:clips[0].skin(skin)[1]].copy()) for key, _, skin, _ in skin_items(c, copy, copy)]
    twin.pose_meshes(fed)
    xf = out.cpu().numpy().reshape(-1, 12)
    instances, row = [], 0
    for key, count in layout:
        instances.append((key, [xf[row + k].copy() for k in range(count)]))
        row += count
    twin.set_instances(instances)
    assert all_bytes(hip, sc, desc) == all_bytes(hip, twin, desc)
    assert all_bytes(hip, sc, desc) != [m.vertices.tobytes() for m in desc.meshes]
    rays = ray_grid(*RAYS)
    assert_scenes_equal(rt, twin, sc, rays, rt.rays_to_device(rays), [m.key for m in desc.meshes], "blended actors")
    sc.close(); twin.close()


# ---- 5. blended clip weights -------------------------------------------------------------------------------------------------------------
def test_blended_active_lists_equal_the_host_rule(rt):
    copies = 8
    sc, c = rigged(rt, MORPH_BAR, copies, morphs=True)
    g, keys = c[1], c[2]
    talk, static = g.bake_clip(0), g.bake_clip(-1)
    ids = {0: sc.attach_clip(talk), -1: sc.attach_clip(static)}
    clips = {0: talk, -1: static}
    sets = (0, 1)
    times = sorted({t for b in sets for t in set_times(talk, b)})
    cases = [(t, times[(3 * k + 1) % len(times)], w) for k, t in enumerate(times) for w in INNER + ([0.0, 1.0] if k % 4 == 0 else [])]
    n = changed = 0
    for a, b in ((0, -1), (-1, 0), (0, 0)):
        for first in range(0, len(cases), copies):
            chunk = cases[first:first + copies]
            actors = [(ids[a], ta, ids[b], tb, w, None, None, 0) for ta, tb, w in chunk]
            items = [(keys[copy][blas], copy, None, rt.ClipWeights(blas)) for copy in range(len(chunk)) for blas in sets]
            sc.pose_actors_blended(actors, items, None)
            info = sc.actor_pose_info()
            assert (info.actors, info.items, info.weight_items, info.launches, info.read_backs, info.refused_item) == (len(chunk), len(items), len(items), 4, 1, NONE)
            got = [sc.read_item_active(k, clips[a].morph(items[k][3].blas)["n_targets"]) for k in range(len(items))]
            ends = [(k, ta if w == 0.0 else tb, a if w == 0.0 else b) for k, (ta, tb, w) in enumerate(chunk) if w in (0.0, 1.0)]
            for k, (key, copy, _, cw) in enumerate(items):
                ta, tb, w = chunk[copy]
                want_at, want_w = compact(clips[a].blend_weights_host(ta, clips[b], tb, w, cw.blas))
                assert got[k][0].tolist() == want_at.tolist() and same(got[k][1], want_w), (a, b, cw.blas, ta, tb, w)
                assert sc.mesh_morph_info(key).n_active == len(want_at)
                changed += int(not same(want_w, compact(clips[a].weights_host(ta, cw.blas))[1]))
                n += 1
            for copy, t, anim in ends:                                         # the end weights: the plain call's lists
                sc.pose_actors([(ids[anim], t, None, None, 0)], [(keys[copy][blas], 0, None, rt.ClipWeights(blas)) for blas in sets], None)
                for blas in sets:
                    plain = sc.read_item_active(blas, clips[anim].morph(blas)["n_targets"])
                    assert plain[0].tolist() == got[2 * copy + blas][0].tolist() and same(plain[1], got[2 * copy + blas][1]), (a, b, blas, t)
    assert n > 300 and changed > 50                                            # the grid is not empty, and most blends are neither source
    sc.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_come_before_any_device_work(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 2)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ids = {a: sc.attach_clip(g.bake_clip(a)) for a in (0, 1)}
    bar = rt.Gltf(SKINNED_BAR)
    other = sc.attach_clip(bar.bake_clip(0))
    ni = len(rows)
    out = tensor_of(2 * ni, fill=7.0)
    good = [(ids[0], 0.5, ids[1], 0.25, 0.5, None, None, 0), (ids[1], 0.75, ids[0], 0.1, 0.25, PLACEMENT, None, ni)]
    good_items = skin_items(c, 0, 0) + skin_items(c, 1, 1)
    sc.pose_actors_blended(good, good_items, out, keep_nodes=True)
    assert refused(rt, lambda: sc.read_actor_sources(0, 11)) == (ERR_STATE, "read_actor_sources: the last call kept no sources (sr_scene_pose_actors_blended with SR_ACTORS_KEEP_SOURCES)")
    sc.read_actor_nodes(0, 11)

    def state():
        i = sc.actor_pose_info()
        return all_bytes(hip, sc, desc), (i.actors, i.items, i.nodes, i.channels, i.upload_bytes, i.launches, i.read_backs, i.calls, i.refused_actor, i.refused_item), out.cpu().numpy().tobytes()

    before = state()
    assert before[1][7] == 1
    A = "pose_actors_blended: actor 1: "

    def second(**change):
        ac = dict(a=ids[1], ta=0.75, b=ids[0], tb=0.1, w=0.25)
        ac.update(change)
        return [good[0], (ac["a"], ac["ta"], ac["b"], ac["tb"], ac["w"], PLACEMENT, None, ni)]

    cases = [(second(w=-0.1), ERR_INVALID_ARG, A + "the weight is not in [0, 1]"), (second(w=1.5), ERR_INVALID_ARG, A + "the weight is not in [0, 1]"),
             (second(w=float("nan")), ERR_INVALID_ARG, A + "the weight is not in [0, 1]"),
             (second(b=99), ERR_INVALID_ARG, A + "no clip is attached under this id"), (second(a=99), ERR_INVALID_ARG, A + "no clip is attached under this id"),
             (second(tb=float("inf")), ERR_INVALID_ARG, A + "gltf: the time of a pose must be finite"),
             (second(ta=float("nan")), ERR_INVALID_ARG, A + "gltf: the time of a pose must be finite")]
    for actors, code, text in cases:
        assert refused(rt, lambda: sc.pose_actors_blended(actors, good_items, out)) == (code, text)
        assert state() == before, text
    for actors in (second(b=other), second(a=other)):
        code, text = refused(rt, lambda: sc.pose_actors_blended(actors, good_items, out))
        assert code == ERR_INVALID_ARG and text.startswith(A + "sr_clip_blend_compatible: the clips differ in the "), text
        assert state() == before, text
    code, text = refused(rt, lambda: sc.pose_actors_blended(good, good_items[:3] + [(good_items[3][0], 1, 5, None)], out))
    assert (code, text) == (ERR_INVALID_ARG, "pose_actors_blended: item 3: skin 5 named, no instanced mesh of the actor's clip wears it") and state() == before
    # the plain entry point reports through the same figures, and takes the kept sources away
    sc.pose_actors_blended(good, good_items, out, keep_sources=True)
    assert sc.actor_pose_info().calls == 2 and len(sc.read_actor_sources(1, 11)[0]) == 11
    assert refused(rt, lambda: sc.read_actor_nodes(0, 11))[0] == ERR_STATE
    sc.pose_actors([(ids[0], 0.5, None, None, 0)], [], out)
    assert sc.actor_pose_info().calls == 3 and refused(rt, lambda: sc.read_actor_sources(0, 11))[0] == ERR_STATE
    sc.close()


def test_an_unavailable_or_missing_morph_set_is_refused(rt, hip):
    sc, c = rigged(rt, MORPH_BAR, 1, morphs=True)
    desc, g, keys = c[0], c[1], c[2]
    talk, spline = sc.attach_clip(g.bake_clip(0)), sc.attach_clip(g.bake_clip(1))
    sc.pose_actors_blended([(talk, 0.5, talk, 1.0, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(0))], None)
    before = (all_bytes(hip, sc, desc), sc.actor_pose_info().calls)
    I = "pose_actors_blended: item 0: "
    for a, b in ((talk, spline), (spline, talk)):
        assert refused(rt, lambda: sc.pose_actors_blended([(a, 0.5, b, 0.5, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(0))], None)) == (ERR_UNSUPPORTED, I + CUBIC)
        assert (all_bytes(hip, sc, desc), sc.actor_pose_info().calls) == before
    assert refused(rt, lambda: sc.pose_actors_blended([(talk, 0.5, spline, 0.5, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(7))], None)) == \
        (ERR_INVALID_ARG, I + "the weights of blas 7 named, the actor's clip has no morph set for it")
    sc.pose_actors_blended([(talk, 0.5, spline, 0.5, 0.5, None, None, 0)], [(keys[0][1], 0, None, rt.ClipWeights(1))], None)      # the set of blas 1 is available in both
    assert sc.actor_pose_info().calls == before[1] + 1
    sc.close()


# ---- 7. a singular blended mesh node ------------------------------------------------------------------------------------------------------
def test_a_singular_blended_actor_refuses_the_whole_call(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 3)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ids = {a: sc.attach_clip(g.bake_clip(a)) for a in (0, 1)}
    ni = len(rows)
    out = tensor_of(3 * ni)
    items = [it for copy in range(3) for it in skin_items(c, copy, copy)]
    sc.pose_actors_blended([(ids[0], 0.5, ids[1], 0.5, 0.5, None, None, k * ni) for k in range(3)], items, out)
    before = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], sc.read_instance_tables()[1].tobytes())
    actors = [(ids[0], 0.9, ids[1], 1.0, 0.5, None, None, 0), (ids[0], 0.9, ids[1], 1.0, 1.0, None, None, ni), (ids[0], 0.9, ids[1], 1.0, 1.0, None, None, 2 * ni)]
    assert refused(rt, lambda: sc.pose_actors_blended(actors, items, out)) == (ERR_UNSUPPORTED, "pose_actors_blended: actor 1: " + SINGULAR)
    info = sc.actor_pose_info()
    assert (info.launches, info.read_backs, info.calls, info.refused_actor, info.refused_item) == (2, 1, 2, 1, NONE)
    after = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], sc.read_instance_tables()[1].tobytes())
    assert before == after
    sc.pose_actors_blended([ac[:4] + (0.5,) + ac[5:] for ac in actors], items, out)         # the scene goes on: half way there the scale is not 0
    assert sc.actor_pose_info().launches == 3 and all_bytes(hip, sc, desc) != before[0]
    sc.close()


# ---- 8. the Renderer twin -------------------------------------------------------------------------------------------------------------------
def test_the_renderer_twin_gives_the_scene_calls_bytes(rt, hip):
    import torch
    g = rt.Gltf(CLIP_RIG)
    clips = [g.bake_clip(0), g.bake_clip(1)]
    camera = ((0.0, 2.0, 7.0), (0.0, 1.0, 0.0), 45.0)
    # the Scene call
    sc, c = rigged(rt, CLIP_RIG, 1)
    ids = [sc.attach_clip(k) for k in clips]
    rows = c[5]
    want = tensor_of(len(rows))
    sc.pose_actors_blended([(ids[0], 0.4, ids[1], 0.7, 0.25, None, rows, 0)], [], want)
    frames = []
    for blended in (True, False):
        r = rt.Renderer((96, 64), devices=[0])
        loaded = r.load_scene(g)
        r.attach_skins(g, loaded)
        rid = [r.attach_clip(k) for k in clips]
        keys = [int(k) for k in loaded.keys]
        items = [(keys[b], 0, g.blas_skin(b)[0], None) for b in range(g.n_blases) if g.blas_skin(b)[0] >= 0]
        out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:0")
        if blended:
            r.pose_actors_blended([(rid[0], 0.4, rid[1], 0.7, 0.25, None, loaded.instance_rows(0), 0)], items, out)
            assert same(out.cpu().numpy(), want.cpu().numpy())
            info = r.actor_pose_info()
            assert (info.actors, info.items, info.launches, info.calls) == (1, 2, 3, 1)
            r.pose_actors_blended([(rid[0], 0.4, rid[1], 0.7, 1.0, None, loaded.instance_rows(0), 0)], items, out)      # at the end weight: the plain call's frame
        else:                                                                  # the same sequence of calls
            r.pose_actors([(rid[0], 0.4, None, loaded.instance_rows(0), 0)], items, out)
            r.pose_actors([(rid[1], 0.7, None, loaded.instance_rows(0), 0)], items, out)
        r.wait_frame(r.render_device_transforms(camera, loaded.layout(), out))
        frames.append(r.render_to_host_memory(camera, loaded.grouped(out.cpu().numpy().reshape(-1, 12))).copy())
        r.close()
    assert np.array_equal(frames[0], frames[1])
    sc.close()
