"""Scene.pose_actors_layered / Renderer.pose_actors_layered (sr_scene_pose_actors_layered: clip_layers_kernel samples an actor's
layers in order, applies the layer rule at each node's effective weight, composes once and writes where clip_pose_kernel writes).
The contract, stage by stage:
  - device against device, bytes: one layer is pose_actors, two unmasked override layers are pose_actors_blended, a mask of ones is
    no mask, and zero weight, a zero mask or an additive layer at its reference time give the stack below;
  - every kept source is sampled under pose_actors' contract against sr_clip_sample_host (at most 1 in 1000 interpolated rotation
    components other than bit equal);
  - the final records are bit equal to sr_clip_layers_host of the device's own sources, and everything composed to
    sr_clip_compose_records_host of the device's own records: no libm in those stages, no tolerance;
  - where every source is in the bit-equal sampling class, the whole chain is bit equal to sr_clip_pose_layers_host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_util import CLIP_RIG, SKINNED_BAR, assert_trs_contract, clip_times, crowd, rotation_classes, shape_rig  # noqa: E402
from clip_morph_util import MORPH_BAR  # noqa: E402
from clip_spline_util import SPLINE_RIG  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5
SINGULAR = "gltf: the transform of the skinned mesh's node is singular"      # sr_gltf_pose's words, as test_gpu_clip_blend.py states them
PLACEMENT = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)
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


def rigged(rt, path, copies=1, morphs=False, cubic=False):
    c = crowd(rt, path, copies)
    if cubic:
        c[1].set_cubicspline(True)
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
    return not rotation_classes(clip, t).any()


def read_actor(sc, a, info):
    trs, glob = sc.read_actor_nodes(a, info.n_nodes)
    return trs, glob, sc.read_actor_matrices(a, info.n_joints)


def base(cid, t):
    return (cid, t, 1.0, "override", None, 0.0)


def check_stacks(rt, sc, clip_of, masks, stacks, what):
    """One call, an actor per stack, nodes and layers kept. A stack is a list of (clip key, time, weight, mode, mask key or None,
    reference time); clip_of maps a clip key to (clip, id), masks a mask key to (host mask, id). The contract of the module's
    docstring -> (rotation components not bit equal, interpolated rotation components, actors held whole to pose_layers_host)."""
    first = clip_of[stacks[0][0][0]][0]
    i, ni = first.info, first.info.n_instances
    instance_nodes = first.layout()[2]
    out = tensor_of(ni * len(stacks))
    actors = [([(clip_of[c][1], t, w, mode, None if m is None else masks[m][1], rt_) for c, t, w, mode, m, rt_ in st], PLACEMENT if k % 2 else None, None, k * ni)
              for k, st in enumerate(stacks)]
    sc.pose_actors_layered(actors, [], out, keep_nodes=True, keep_layers=True)
    info, li = sc.actor_pose_info(), sc.layer_pose_info()
    samples = sum(clip_of[c][0].info.n_channels * (2 if mode == "additive" else 1) for st in stacks for c, _, _, mode, _, _ in st)
    assert (info.actors, info.items, info.nodes, info.channels, info.launches, info.read_backs) == (len(stacks), 0, len(stacks) * i.n_nodes, samples, 3, 1)
    assert (li.layers, li.additive_layers, li.masked_layers, li.max_layers, li.layer_table_bytes) == \
        (sum(len(st) for st in stacks), sum(mode == "additive" for st in stacks for _, _, _, mode, _, _ in st),
         sum(m is not None for st in stacks for _, _, _, _, m, _ in st), max(len(st) for st in stacks), 32 * sum(len(st) for st in stacks))
    xf = out.cpu().numpy().reshape(-1, 12)
    differ = total = whole = 0
    for k, st in enumerate(stacks):
        label = "%s actor %d" % (what, k)
        placement = PLACEMENT if k % 2 else None
        trs, glob, jm = read_actor(sc, k, i)
        cur, ref, rules, classes = [], [], [], True
        for l, (c, t, w, mode, m, rt_) in enumerate(st):
            clip = clip_of[c][0]
            got_cur, got_ref = sc.read_actor_layer(k, l, i.n_nodes)
            d, n = assert_trs_contract(got_cur, clip.sample_host(t), rotation_classes(clip, t), "%s layer %d" % (label, l))
            differ, total, classes = differ + d, total + n, classes and static_class(clip, t)
            if mode == "additive":
                d, n = assert_trs_contract(got_ref, clip.sample_host(rt_), rotation_classes(clip, rt_), "%s layer %d at its reference time" % (label, l))
                differ, total, classes = differ + d, total + n, classes and static_class(clip, rt_)
            cur.append(got_cur); ref.append(got_ref if mode == "additive" else None)
            rules.append((w, mode, None if m is None else masks[m][0]))
        assert same(trs, rt.clip_layers_host(cur, rules, ref)), label + ": the final records"
        want_jm, want_xf, bad = first.compose_records_host(trs, placement)
        assert bad is None, label
        assert same(jm, want_jm), label + ": joint matrices"
        assert same(xf[k * ni:(k + 1) * ni], want_xf), label + ": instance transforms"
        assert same(glob[instance_nodes][:, :12], first.compose_records_host(trs)[1]), label + ": globals"
        if classes:
            host_jm, host_xf = first.pose_layers_host([(clip_of[c][0], t, w, mode, None if m is None else masks[m][0], rt_) for c, t, w, mode, m, rt_ in st], placement)
            assert same(jm, host_jm) and same(xf[k * ni:(k + 1) * ni], host_xf), label + ": the whole chain against pose_layers_host"
            whole += 1
    return differ, total, whole


# ---- 1. device against device, bytes ----------------------------------------------------------------------------------------------------
def test_stacks_equal_the_calls_they_extend_byte_for_byte(rt, hip):
    copies = 4
    (lay_sc, c), (plain_sc, _), (blend_sc, _) = rigged(rt, CLIP_RIG, copies), rigged(rt, CLIP_RIG, copies), rigged(rt, CLIP_RIG, copies)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: lay_sc.attach_clip(clip) for a, clip in clips.items()}
    assert ids == {a: plain_sc.attach_clip(clip) for a, clip in clips.items()} == {a: blend_sc.attach_clip(clip) for a, clip in clips.items()}
    i, ni = clips[0].info, len(rows)
    n = i.n_nodes
    ones, zeros = lay_sc.attach_node_mask(np.ones(n, F32)), lay_sc.attach_node_mask(np.zeros(n, F32))
    arm = lay_sc.attach_node_mask(clips[0].subtree_mask(int(clips[0].layout()[0]["gltf_node"][n // 2]), 0.75, 0.25))
    times = (0.3, 0.9, 1.6)
    perm = np.array([2, 0, 1], np.uint32)
    # every actor is a stack and the blended actor (a, ta, b, tb, w) it must equal; w 0 with a == b at one time is the plain call too
    layered, blended = [], []

    def add(stack, a, ta, b, tb, w):
        k = len(layered)
        placement, inst = (PLACEMENT if k % 2 else None), (perm + np.uint32(k * ni) if k % 4 in (1, 2) else None)
        layered.append((stack, placement, inst, k * ni))
        blended.append((ids[a], ta, ids[b], tb, w, placement, inst, k * ni))

    for a in (-1, 0, 1):                                                        # one layer
        for t in times:
            add([base(ids[a], t)], a, t, a, t, 0.0)
    for k, (a, b) in enumerate(((0, 1), (1, 0), (0, -1), (-1, 1), (0, 0), (1, 1))):      # two unmasked override layers, end and inner weights
        for j, w in enumerate([0.0, 1.0] + INNER):
            ta, tb = times[(k + j) % 3], times[(k + 2 * j + 1) % 3]
            add([base(ids[a], ta), (ids[b], tb, w, "override", None if j % 2 else ones, 0.0)], a, ta, b, tb, w)      # a mask of ones is no mask
    for k, (a, b) in enumerate(((0, 1), (1, 0), (-1, 0))):                        # three and eight layers whose upper layers do nothing
        ta, tb, w = times[k], times[(k + 1) % 3], INNER[k + 1]
        two = [base(ids[a], ta), (ids[b], tb, w, "override", None, 0.0)]
        add(two + [(ids[1], 0.4, 0.0, "override", None, 0.0)], a, ta, b, tb, w)
        add(two + [(ids[0], 0.4, 0.8, "override", zeros, 0.0)], a, ta, b, tb, w)
        add(two + [(ids[0], 0.7, 0.6, "additive", None, 0.7)], a, ta, b, tb, w)           # clip 0's mask bits are in the stack below already
        add(two + [(ids[0], 0.4, 0.5, "additive", zeros, 1.1), (ids[1], 0.2, 0.0, "additive", arm, 1.3), (ids[0], 1.2, 1.0, "additive", arm, 1.2),
                   (ids[-1], 0.0, 0.9, "additive", None, 0.5), (ids[0], 0.4, 0.0, "override", arm, 0.0), (ids[1], 0.4, 1.0, "override", zeros, 0.0)], a, ta, b, tb, w)
    n_actors = len(layered)
    assert n_actors == 57 and {len(ac[0]) for ac in layered} == {1, 2, 3, 8}
    drivers = [3, 12, 40, 56]                                                    # four of the actors drive the four copies' meshes
    items = [it for copy, a in enumerate(drivers) for it in skin_items(c, copy, a)]
    outs = [tensor_of(ni * n_actors) for _ in range(3)]
    lay_sc.pose_actors_layered(layered, items, outs[0], keep_nodes=True)
    blend_sc.pose_actors_blended(blended, items, outs[1], keep_nodes=True)
    plain = [(ac[0], ac[1], ac[5], ac[6], ac[7]) for ac in blended[:9]]
    plain_sc.pose_actors(plain, [], outs[2], keep_nodes=True)
    assert same(outs[0].cpu().numpy(), outs[1].cpu().numpy()) and not np.isnan(outs[0].cpu().numpy()).any()
    assert same(outs[0].cpu().numpy()[:9 * ni], outs[2].cpu().numpy()[:9 * ni])
    for a in range(n_actors):
        for name, x, y in zip(("TRS", "globals", "joint matrices"), read_actor(lay_sc, a, i), read_actor(blend_sc, a, i)):
            assert same(x, y), (a, name)
    for a in range(9):
        for name, x, y in zip(("TRS", "globals", "joint matrices"), read_actor(lay_sc, a, i), read_actor(plain_sc, a, i)):
            assert same(x, y), (a, name)
    assert all_bytes(hip, lay_sc, desc) == all_bytes(hip, blend_sc, desc) != [m.vertices.tobytes() for m in desc.meshes]
    li, bi = lay_sc.actor_pose_info(), blend_sc.actor_pose_info()
    assert (li.actors, li.items, li.nodes, li.launches, li.read_backs, li.calls, li.refused_actor) == (bi.actors, bi.items, bi.nodes, bi.launches, bi.read_backs, bi.calls, NONE)
    n_layer_rows = sum(len(ac[0]) for ac in layered)
    assert li.upload_bytes - bi.upload_bytes == n_actors * (80 - 96) + 32 * n_layer_rows + 64      # the rows, the layer table and the targets
    assert lay_sc.layer_pose_info().layer_table_bytes == 32 * n_layer_rows
    assert refused(rt, lambda: lay_sc.read_actor_layer(0, 0, n))[0] == ERR_STATE                 # no layers were kept
    for sc in (lay_sc, plain_sc, blend_sc):
        sc.close()


# ---- 2. the contract ------------------------------------------------------------------------------------------------------------------------
def test_contract_of_three_and_eight_layers_on_the_fixture(rt):
    g = rt.Gltf(CLIP_RIG)
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    sc = rt.Scene(0)
    clip_of = {a: (clip, sc.attach_clip(clip)) for a, clip in clips.items()}
    nodes = clips[0].layout()[0]
    n = len(nodes)
    rng = np.random.default_rng(11)
    host_masks = {"arm": clips[0].subtree_mask(int(nodes["gltf_node"][n // 2])), "soft": clips[0].subtree_mask(int(nodes["gltf_node"][1]), 0.75, 0.125),
                  "noise": rng.random(n).astype(F32)}
    host_masks["noise"][:4] = [0.0, 1.0, INNER[0], INNER[3]]
    masks = {k: (m, sc.attach_node_mask(m)) for k, m in host_masks.items()}
    times = {a: [t for t in clip_times(clip) if not (a == 1 and t == 1.0)] for a, clip in clips.items()}     # the singular time has a test of its own
    fixed = {a: [t for t in ts if static_class(clips[a], t)] for a, ts in times.items()}      # the bit-equal sampling class
    assert len(fixed[0]) >= 5 and len(fixed[1]) >= 5
    differ = total = whole = 0
    stacks = []
    for k in range(max(len(times[0]), len(times[1]), 48)):                       # base, override under a subtree mask, additive
        t0, t1 = (fixed[0], fixed[1]) if k % 2 else (times[0], times[1])           # every other stack is held whole to the host
        ta, tb, tc, tr = t0[k % len(t0)], t1[(5 * k + 3) % len(t1)], t0[(3 * k + 1) % len(t0)], t0[(7 * k + 2) % len(t0)]
        a, b = ((0, 1), (1, 0))[k % 2]
        stacks.append([(a, ta if a == 0 else tb, 1.0, "override", None, 0.0), (b, tb if a == 0 else ta, INNER[k % 4], "override", ("arm", "soft", "noise")[k % 3], 0.0),
                       (0, tc, (1.0, 0.5, INNER[1])[k % 3], "additive", (None, "noise", "arm")[k % 3], tr)])
    d, m, wh = check_stacks(rt, sc, clip_of, masks, stacks, "three layers")
    differ, total, whole = differ + d, total + m, whole + wh
    stacks = []
    for k in range(12):                                                          # eight layers
        t0, t1 = (fixed[0], fixed[1]) if k % 3 == 0 else (times[0], times[1])
        pick = lambda j: t0[(k * 5 + j * 3) % len(t0)]
        pick1 = lambda j: t1[(k * 7 + j * 2 + 1) % len(t1)]
        stacks.append([(0, pick(0), 1.0, "override", None, 0.0), (1, pick1(1), 0.5, "override", "arm", 0.0), (0, pick(2), INNER[1], "additive", None, pick(3)),
                       (-1, 0.0, 0.25, "override", "soft", 0.0), (1, pick1(4), 1.0, "additive", "noise", pick1(5)), (0, pick(6), INNER[3], "override", "noise", 0.0),
                       (1, pick1(7), INNER[0], "additive", "soft", pick1(8)), (0, pick(9), 0.75, "additive", "arm", pick(10))])
    d, m, wh = check_stacks(rt, sc, clip_of, masks, stacks, "eight layers")
    differ, total, whole = differ + d, total + m, whole + wh
    print("interpolated rotation components of the sources not bit equal: %d of %d; %d actors held to pose_layers_host" % (differ, total, whole))
    assert whole >= 20
    assert total > 1000 and differ * 1000 <= total
    sc.close()


# ---- 3. wider than the block ----------------------------------------------------------------------------------------------------------------
def test_contract_on_a_rig_wider_than_the_block(rt, tmp_path):
    path = str(tmp_path / "wide.glb")
    n_nodes = shape_rig(path, chain=20, fan=300, joints=90, channels=330, keys=2)
    g = rt.Gltf(path)
    moving, still = g.bake_clip(0), g.bake_clip(-1)
    i = moving.info
    assert 256 < n_nodes == i.n_nodes <= 384 and i.n_channels == 330 and i.n_joints * 3 > 256
    sc = rt.Scene(0)
    clip_of = {0: (moving, sc.attach_clip(moving)), -1: (still, sc.attach_clip(still))}
    vary = ((np.arange(n_nodes) * 37 % 101) / 100.0).astype(F32)                 # a mask that varies per node, 0 and 1 among its values
    assert vary.min() == 0.0 and vary.max() == 1.0
    masks = {"vary": (vary, sc.attach_node_mask(vary))}
    ta, tb = float(F32(0.07)), float(F32(0.3))                                    # between the keys, and past every channel's last key
    stacks = [[(-1, 0.0, 1.0, "override", None, 0.0), (0, ta, float(F32(1.0) / F32(3.0)), "override", "vary", 0.0), (0, tb, 0.5, "additive", "vary", ta)],
              [(0, tb, 1.0, "override", None, 0.0), (0, ta, 0.5, "additive", "vary", tb), (0, ta, 0.75, "override", "vary", 0.0)]]
    _, total, whole = check_stacks(rt, sc, clip_of, masks, stacks, "the wide rig")
    assert total > 1000 and whole == 0                                           # ta interpolates: the stages are held one by one
    stacks = [[(0, tb, 1.0, "override", None, 0.0), (0, 0.0, 0.5, "additive", "vary", tb), (0, 0.0, 0.75, "override", "vary", 0.0)]] * 2
    assert check_stacks(rt, sc, clip_of, masks, stacks, "the wide rig at its keys")[2] == 2
    sc.close()


# ---- 4. cubic -------------------------------------------------------------------------------------------------------------------------------
def test_a_cubic_bake_as_an_override_and_as_an_additive_layer_is_bit_equal_to_the_host(rt):
    g = rt.Gltf(SPLINE_RIG)
    g.set_cubicspline(True)
    clips = {a: g.bake_clip(a) for a in (0, 1, 2)}
    n_cubic = {a: int((clip.layout()[1]["interpolation"] == 2).sum()) for a, clip in clips.items()}
    a = max(n_cubic, key=n_cubic.get)
    assert n_cubic[a] > 0, "the fixture has CUBICSPLINE channels"
    sc = rt.Scene(0)
    clip_of = {k: (clip, sc.attach_clip(clip)) for k, clip in clips.items()}
    ts = [t for t in clip_times(clips[a]) if static_class(clips[a], t)]          # a LINEAR rotation beside the cubic channels stays at its keys
    assert len(ts) >= 9
    stacks = []
    for k in range(0, len(ts), 2):
        t, u, v = ts[k], ts[(k + 7) % len(ts)], ts[(2 * k + 1) % len(ts)]
        stacks.append([(a, t, 1.0, "override", None, 0.0), (a, u, INNER[k % 4], "override", None, 0.0), (a, v, 0.5, "additive", None, t)])
    differ, total, whole = check_stacks(rt, sc, clip_of, {}, stacks, "cubic")
    assert differ == 0 and whole == len(stacks) >= 5                             # no libm in a cubic sample: the whole chain, every actor
    assert sc.spline_pose_info().cubic_channels == 4 * n_cubic[a] * len(stacks)
    sc.close()


# ---- 5. items -------------------------------------------------------------------------------------------------------------------------------
def test_posed_geometry_is_pose_meshes_fed_the_layered_matrices(rt, hip):
    copies = 3
    (sc, c), (twin, _) = rigged(rt, CLIP_RIG, copies), rigged(rt, CLIP_RIG, copies)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: sc.attach_clip(clip) for a, clip in clips.items()}
    ni, i = len(rows), clips[0].info
    arm = sc.attach_node_mask(clips[0].subtree_mask(int(clips[0].layout()[0]["gltf_node"][i.n_nodes // 2])))
    out = tensor_of(copies * ni)
    actors = [([base(ids[0], 0.4), (ids[1], 0.7, 0.25, "override", arm, 0.0), (ids[0], 1.1, 0.5, "additive", None, 0.2)], None, rows, 0),
              ([base(ids[-1], 0.0), (ids[0], 1.3, 1.0, "additive", None, 0.0)], None, rows + np.uint32(ni), 0),
              ([base(ids[1], 1.9)], None, rows + np.uint32(2 * ni), 0)]
    items = [it for copy in range(copies) for it in skin_items(c, copy, copy)]
    sc.pose_actors_layered(actors, items, out)
    sc.set_instances_device(layout, out)
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.launches, info.read_backs, info.refused_actor, info.refused_item) == (3, 2 * copies, 3, 1, NONE, NONE)
    fed = []
    for copy in range(copies):
        jm = sc.read_actor_matrices(copy, i.n_joints)
        fed += [(key, None, jm[clips[0].skin(skin)[0]:][:clips[0].skin(skin)[1]].copy()) for key, _, skin, _ in skin_items(c, copy, copy)]
    twin.pose_meshes(fed)
    assert all_bytes(hip, sc, desc) == all_bytes(hip, twin, desc) != [m.vertices.tobytes() for m in desc.meshes]
    sc.close(); twin.close()


def test_a_clip_weighted_items_active_list_is_the_plain_calls_for_the_base_clip(rt):
    sc, c = rigged(rt, MORPH_BAR, 2, morphs=True)
    g, keys = c[1], c[2]
    talk, static = g.bake_clip(0), g.bake_clip(-1)
    ids = {0: sc.attach_clip(talk), -1: sc.attach_clip(static)}
    for t in (0.0, 0.3, 0.77, 1.5):
        items = [(keys[0][blas], 0, None, rt.ClipWeights(blas)) for blas in (0, 1)]
        sc.pose_actors_layered([([base(ids[0], t), (ids[-1], 0.0, 0.5, "override", None, 0.0), (ids[0], 1.0, 0.5, "additive", None, 0.1)], None, None, 0)], items, None)
        info = sc.actor_pose_info()
        assert (info.weight_items, info.launches, info.refused_item) == (2, 4, NONE)
        got = [sc.read_item_active(k, talk.morph(k)["n_targets"]) for k in (0, 1)]
        sc.pose_actors([(ids[0], t, None, None, 0)], items, None)
        for blas in (0, 1):
            want = sc.read_item_active(blas, talk.morph(blas)["n_targets"])
            assert got[blas][0].tolist() == want[0].tolist() and same(got[blas][1], want[1]), (t, blas)
    sc.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_host_refusals_come_before_any_device_work(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 2)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    clips = {a: g.bake_clip(a) for a in (-1, 0, 1)}
    ids = {a: sc.attach_clip(clip) for a, clip in clips.items()}
    other = sc.attach_clip(rt.Gltf(SKINNED_BAR).bake_clip(0))
    n, ni = clips[0].info.n_nodes, len(rows)
    mask = sc.attach_node_mask(np.full(n, 0.5, F32))
    short = sc.attach_node_mask(np.full(n - 1, 0.5, F32))
    out = tensor_of(2 * ni, fill=7.0)
    top = (ids[1], 0.25, 0.5, "override", mask, 0.0)
    good = [([base(ids[0], 0.5), top], None, None, 0), ([base(ids[1], 0.75), (ids[0], 0.1, 0.25, "additive", None, 0.6)], PLACEMENT, None, ni)]
    good_items = skin_items(c, 0, 0) + skin_items(c, 1, 1)
    sc.pose_actors_layered(good, good_items, out, keep_nodes=True)
    assert refused(rt, lambda: sc.read_actor_layer(0, 0, n)) == (ERR_STATE, "read_actor_layer: the last call kept no layers (sr_scene_pose_actors_layered with SR_ACTORS_KEEP_LAYERS)")

    def state():
        i, l = sc.actor_pose_info(), sc.layer_pose_info()
        return (all_bytes(hip, sc, desc), (i.actors, i.items, i.nodes, i.channels, i.upload_bytes, i.launches, i.read_backs, i.calls, i.refused_actor, i.refused_item),
                (l.layers, l.additive_layers, l.masked_layers, l.layer_table_bytes), out.cpu().numpy().tobytes())

    before = state()
    assert before[1][7] == 1 and before[2] == (4, 1, 1, 128)
    A, L0, L1 = "pose_actors_layered: actor 1: ", "pose_actors_layered: actor 1: layer 0: ", "pose_actors_layered: actor 1: layer 1: "
    BASE = L0 + "the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1"
    TIME = "gltf: the time of a pose must be finite"

    def second(layers, placement=PLACEMENT, inst=None, at=ni):
        return [good[0], (layers, placement, inst, at)]

    b, t = base(ids[1], 0.75), (ids[0], 0.1, 0.25, "additive", None, 0.6)
    cases = [(second([]), A + "the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"), (second([b] * 9), A + "the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"),
             (second([b, (99,) + t[1:]]), L1 + "no clip is attached under this id"), (second([(99,) + b[1:], t]), L0 + "no clip is attached under this id"),
             (second([b, t[:2] + (-0.1,) + t[3:]]), L1 + "the weight is not in [0, 1]"), (second([b, t[:2] + (1.5,) + t[3:]]), L1 + "the weight is not in [0, 1]"),
             (second([b, t[:2] + (float("nan"),) + t[3:]]), L1 + "the weight is not in [0, 1]"),
             (second([b, t[:3] + (2,) + t[4:]]), L1 + "unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)"),
             (second([b, t[:4] + (77,) + t[5:]]), L1 + "no node mask is attached under this id"),
             (second([b, t[:4] + (short,) + t[5:]]), L1 + "the mask has %d values, the clip %d nodes" % (n - 1, n)),
             (second([b, (t[0], float("inf")) + t[2:]]), L1 + TIME), (second([b, t[:5] + (float("nan"),)]), L1 + TIME), (second([(b[0], float("nan")) + b[2:], t]), L0 + TIME),
             (second([(b[0], b[1], 0.5) + b[3:], t]), BASE), (second([b[:3] + ("additive",) + b[4:], t]), BASE), (second([b[:4] + (mask,) + b[5:], t]), BASE),
             (second([b, t], placement=np.array([np.inf] + [0.0] * 11, F32)), A + "the placement has a component that is not finite")]
    for actors, text in cases:
        assert refused(rt, lambda: sc.pose_actors_layered(actors, good_items, out)) == (ERR_INVALID_ARG, text)
        assert state() == before, text
    for actors in (second([b, (other,) + t[1:]]), second([(other,) + b[1:], t])):
        code, text = refused(rt, lambda: sc.pose_actors_layered(actors, good_items, out))
        assert code == ERR_INVALID_ARG and text.startswith(L1 + "sr_clip_blend_compatible: the clips differ in the "), text
        assert state() == before, text
    assert refused(rt, lambda: sc.pose_actors_layered(second([b, t], at=5), good_items, None)) == \
        (ERR_INVALID_ARG, A + "instance rows or an instance base given without device instance transforms")
    assert state() == before
    code, text = refused(rt, lambda: sc.pose_actors_layered(good, good_items[:3] + [(good_items[3][0], 1, 5, None)], out))
    assert (code, text) == (ERR_INVALID_ARG, "pose_actors_layered: item 3: skin 5 named, no instanced mesh of the actor's clip wears it") and state() == before
    code, text = refused(rt, lambda: sc.pose_actors_layered(good, good_items[:3] + [(good_items[3][0], 7, good_items[3][2], None)], out))
    assert (code, text) == (ERR_INVALID_ARG, "pose_actors_layered: item 3: actor 7 named, the call has 2 actors") and state() == before
    # a mask value outside [0, 1] is refused at the attach
    for bad in (-0.25, 1.5, float("nan")):
        m = np.full(n, 0.5, F32)
        m[3] = bad
        assert refused(rt, lambda: sc.attach_node_mask(m)) == (ERR_INVALID_ARG, "attach_node_mask: node 3: the value is not in [0, 1]")
    assert refused(rt, lambda: sc.detach_node_mask(1234)) == (ERR_INVALID_ARG, "detach_node_mask: no node mask is attached under this id")
    assert state() == before
    # an override layer's reference time is not read; a detached mask is unknown; the other entry points take the kept layers away
    sc.pose_actors_layered(second([b, (ids[0], 0.1, 0.25, "override", None, float("nan"))]), good_items, out, keep_layers=True)
    assert sc.actor_pose_info().calls == 2 and len(sc.read_actor_layer(1, 1, n)[0]) == n
    assert refused(rt, lambda: sc.read_actor_layer(1, 2, n)) == (ERR_INVALID_ARG, "read_actor_layer: layer index out of range")
    sc.detach_node_mask(mask)
    assert refused(rt, lambda: sc.pose_actors_layered(good, good_items, out))[1] == "pose_actors_layered: actor 0: layer 1: no node mask is attached under this id"
    sc.pose_actors([(ids[0], 0.5, None, None, 0)], [], out)
    assert sc.actor_pose_info().calls == 3 and refused(rt, lambda: sc.read_actor_layer(0, 0, n))[0] == ERR_STATE
    sc.close()


# ---- 7. singular ----------------------------------------------------------------------------------------------------------------------------
def test_a_singular_actor_refuses_the_whole_call(rt, hip):
    sc, c = rigged(rt, CLIP_RIG, 3)
    desc, g, keys, rigs, layout, rows, skins, _ = c
    ids = {a: sc.attach_clip(g.bake_clip(a)) for a in (0, 1)}
    ni = len(rows)
    out = tensor_of(3 * ni)
    items = [it for copy in range(3) for it in skin_items(c, copy, copy)]
    sc.pose_actors_layered([([base(ids[0], 0.5), (ids[1], 0.5, 0.5, "override", None, 0.0)], None, None, k * ni) for k in range(3)], items, out)
    before = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], sc.read_instance_tables()[1].tobytes())

    def actors(w):                                                               # the fixture's `collapse` at t = 1 as the top layer
        return [([base(ids[0], 0.9), (ids[1], 1.0, 0.5, "override", None, 0.0)], None, None, 0)] + \
            [([base(ids[0], 0.9), (ids[0], 0.2, 0.5, "additive", None, 0.4), (ids[1], 1.0, w, "override", None, 0.0)], None, None, k * ni) for k in (1, 2)]

    assert refused(rt, lambda: sc.pose_actors_layered(actors(1.0), items, out)) == (ERR_UNSUPPORTED, "pose_actors_layered: actor 1: " + SINGULAR)
    info = sc.actor_pose_info()
    assert (info.launches, info.read_backs, info.calls, info.refused_actor, info.refused_item) == (2, 1, 2, 1, NONE)
    after = (all_bytes(hip, sc, desc), [(sc.mesh_skin_info(k).skinned, sc.mesh_skin_info(k).first_bad) for k in sorted(rigs)], sc.read_instance_tables()[1].tobytes())
    assert before == after
    sc.pose_actors_layered(actors(0.5), items, out)                              # the scene goes on: half way there the scale is not 0
    assert sc.actor_pose_info().launches == 3 and all_bytes(hip, sc, desc) != before[0]
    sc.close()


# ---- 8. the Renderer twin -------------------------------------------------------------------------------------------------------------------
def test_the_renderer_twin_gives_the_scene_calls_bytes(rt, hip):
    import torch
    g = rt.Gltf(CLIP_RIG)
    clips = [g.bake_clip(0), g.bake_clip(1)]
    mask = clips[0].subtree_mask(int(clips[0].layout()[0]["gltf_node"][clips[0].info.n_nodes // 2]), 1.0, 0.25)
    sc, c = rigged(rt, CLIP_RIG, 1)
    ids, mid = [sc.attach_clip(k) for k in clips], sc.attach_node_mask(mask)
    rows = c[5]
    want = tensor_of(len(rows))
    stack = lambda cid, m: [base(cid[0], 0.4), (cid[1], 0.7, 0.25, "override", m, 0.0), (cid[0], 1.3, 0.5, "additive", None, 0.1)]
    sc.pose_actors_layered([(stack(ids, mid), None, rows, 0)], skin_items(c, 0, 0), want)
    r = rt.Renderer((96, 64), devices=[0])
    loaded = r.load_scene(g)
    r.attach_skins(g, loaded)
    rid, rmid = [r.attach_clip(k) for k in clips], r.attach_node_mask(mask)
    keys = [int(k) for k in loaded.keys]
    items = [(keys[b], 0, g.blas_skin(b)[0], None) for b in range(g.n_blases) if g.blas_skin(b)[0] >= 0]
    out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:0")
    r.pose_actors_layered([(stack(rid, rmid), None, loaded.instance_rows(0), 0)], items, out)
    assert same(out.cpu().numpy(), want.cpu().numpy())
    info = r.actor_pose_info()
    assert (info.actors, info.items, info.launches, info.calls) == (1, len(items), 3, 1)
    r.detach_node_mask(rmid)
    assert refused(rt, lambda: r.pose_actors_layered([(stack(rid, rmid), None, loaded.instance_rows(0), 0)], items, out))[0] == ERR_INVALID_ARG
    r.close(); sc.close()
