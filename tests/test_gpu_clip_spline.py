"""CUBICSPLINE clips on the device (sr_gltf_set_cubicspline, then sr_scene_pose_actors / sr_scene_pose_actors_blended): the cubic
branch of clip_pose_kernel and clip_blend_kernel and the rows of clip_spline_weights_kernel against the host rule
(sr_clip_sample_host, sr_clip_pose_host, sr_clip_weights_host and the blend host rules), which test_clip_spline_host.py holds to an
exact-arithmetic reference. A cubic sample is + - * / and one sqrt in fp64 rounded once, so the contract is equality of bytes with
no tolerance. The one LINEAR rotation of the fixture (node 9 "prop", a leaf) keeps pose_actors' own contract
(clip_util.assert_trs_contract); everything that does not hang on it is byte-equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_morph_util import compact  # noqa: E402
from clip_spline_util import SPLINE_RIG, TARGET_COUNTS, QUAD_TIMES, bits, channel_times, clip_channel_times, collapsing_rig, spline_quad  # noqa: E402
from clip_util import assert_trs_contract, crowd, rotation_classes  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402

NONE = 0xFFFFFFFF
ERR_UNSUPPORTED = -5
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"
SINGULAR = "gltf: the transform of the skinned mesh's node is singular"
PLACEMENT = np.array([0.8, -0.1, 0.2, 3.0, 0.1, 0.9, 0.0, -1.5, -0.2, 0.05, 1.1, 0.25], np.float32)
PROP_NODE, FACE_BLAS, PROP_INSTANCE = 9, 3, 2
PAIRS = {"cubic_linear": (0, 1), "linear_cubic": (1, 0), "cubic_cubic": (0, 0)}


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
def rig(rt):
    """spline_rig.glb under SAMPLE: the open file and its three animations baked -> (gltf, {animation: clip})."""
    g = rt.Gltf(SPLINE_RIG)
    g.set_cubicspline(True)
    return g, {a: g.bake_clip(a) for a in (0, 1, 2)}


@pytest.fixture(scope="module")
def quads(rt, tmp_path_factory):
    """The generated one-triangle files of 1, 64, 65 and 130 targets -> {n_targets: path}."""
    d = tmp_path_factory.mktemp("clip_spline")
    paths = {n: str(d / ("tri%d.glb" % n)) for n in TARGET_COUNTS}
    for n, p in paths.items():
        spline_quad(p, n)
    return paths


def refused(rt, call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def tensor_of(n_rows):
    import torch
    return torch.full((max(n_rows, 1), 12), float("nan"), dtype=torch.float32, device="cuda:0")


def posed_scene(rt, path, copies=1, sample=True):
    """A scene of `copies` copies of a file with every rig and every morph attached, the file opened under SAMPLE ->
    (scene, the crowd() tuple)."""
    c = crowd(rt, path, copies)
    c[1].set_cubicspline(sample)
    sc = rt.Scene(0).load(c[0])
    for key, (inf, nj) in c[3].items():
        sc.set_mesh_skin(key, inf, nj)
    for b in range(c[1].n_blases):
        d = c[1].blas_morph(b)[0]
        for copy in range(copies if d is not None else 0):
            sc.set_mesh_morph(c[2][copy][b], d)
    return sc, c


def all_bytes(hip, sc, desc):
    return [device_vertices(hip, sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(desc.meshes)]


def off_prop(clip):
    """The clip nodes other than the one the LINEAR rotation turns."""
    return clip.layout()[0]["gltf_node"] != PROP_NODE


def check_actor(sc, a, clip, t, xf, placement, what):
    """One kept actor of a plain call against the host rule: the contract of the module's docstring."""
    i = clip.info
    trs, glob = sc.read_actor_nodes(a, i.n_nodes)
    jm = sc.read_actor_matrices(a, i.n_joints)
    want = clip.sample_host(t)
    assert_trs_contract(trs, want, rotation_classes(clip, t), what)
    keep = off_prop(clip)
    assert same(trs[keep], want[keep]), what + ": TRS"
    want_jm, want_xf = clip.pose_host(t, placement)
    assert same(jm, want_jm), what + ": joint matrices"
    others = [k for k in range(i.n_instances) if k != PROP_INSTANCE]
    assert same(xf[others], want_xf[others]), what + ": instance transforms"
    inst = clip.layout()[2]
    assert same(glob[inst[others]][:, :12], clip.pose_host(t)[1][others]), what + ": globals"
    # the prop's own transform: composed on the device from the device's own record, no libm in that
    assert same(xf, clip.compose_host(trs, placement)[1]), what + ": the composition of the device's records"


# ---- 1. the TRS channels ----------------------------------------------------------------------------------------------------------------
def test_cubic_actors_equal_the_host_rule(rt, rig):
    g, clips = rig
    sc = rt.Scene(0)
    for a in (0, 2):
        clip = clips[a]
        cid = sc.attach_clip(clip)
        i = clip.info
        times = clip_channel_times(clip)
        out = tensor_of(i.n_instances * len(times))
        actors = [(cid, t, PLACEMENT if k % 2 else None, None, k * i.n_instances) for k, t in enumerate(times)]
        sc.pose_actors(actors, [], out, keep_nodes=True)
        info, sp = sc.actor_pose_info(), sc.spline_pose_info()
        assert (info.actors, info.launches, info.read_backs, info.refused_actor) == (len(times), 3, 1, NONE)
        n_cubic = int((clip.layout()[1]["interpolation"] == abi.CLIP_CUBICSPLINE).sum())
        assert n_cubic == (6 if a == 0 else 1)
        assert (sp.spline_weight_rows, sp.plain_weight_rows, sp.cubic_channels) == (0, 0, n_cubic * len(times))
        xf = out.cpu().numpy().reshape(len(times), i.n_instances, 12)
        assert np.isfinite(xf).all()
        for k, t in enumerate(times):
            check_actor(sc, k, clip, t, xf[k], PLACEMENT if k % 2 else None, "animation %d t = %r" % (a, t))
        assert len(times) >= (25 if a == 0 else 6)
    # through_zero half way: the zero quaternion, the identity rotation
    sc.pose_actors([(cid, 0.5, None, None, 0)], [], None, keep_nodes=True)
    trs = sc.read_actor_nodes(0, clips[2].info.n_nodes)[0]
    node = int(np.flatnonzero(clips[2].layout()[0]["gltf_node"] == 2)[0])
    assert same(trs[node]["rotation"], np.zeros(4, np.float32)) and same(trs, clips[2].sample_host(0.5))
    sc.close()


# ---- 2. cubic and LINEAR clips in one call --------------------------------------------------------------------------------------------
def test_linear_actors_beside_cubic_ones_keep_their_bytes(rt, rig):
    g, clips = rig
    sc = rt.Scene(0)
    cubic, linear = sc.attach_clip(clips[0]), sc.attach_clip(clips[1])
    i = clips[0].info
    times = [0.1, 0.3, 0.625, 0.95, 1.0, 1.3, 1.999, 2.5]
    mixed = [(cubic if k % 2 == 0 else linear, t, None, None, k * i.n_instances) for k, t in enumerate(times)]
    out = tensor_of(i.n_instances * len(times))
    sc.pose_actors(mixed, [], out, keep_nodes=True)
    assert sc.spline_pose_info().cubic_channels == 6 * 4
    got = [(sc.read_actor_nodes(k, i.n_nodes), sc.read_actor_matrices(k, i.n_joints)) for k in range(len(times))]
    xf = out.cpu().numpy().reshape(len(times), i.n_instances, 12)
    for k, t in enumerate(times):
        if k % 2 == 0:
            check_actor(sc, k, clips[0], t, xf[k], None, "mixed call, cubic actor t = %r" % t)
    alone = [(linear, t, None, None, n * i.n_instances) for n, t in enumerate(times[1::2])]
    out2 = tensor_of(i.n_instances * len(alone))
    sc.pose_actors(alone, [], out2, keep_nodes=True)
    assert sc.spline_pose_info().cubic_channels == 0
    xf2 = out2.cpu().numpy().reshape(len(alone), i.n_instances, 12)
    for n, k in enumerate(range(1, len(times), 2)):
        (trs, glob), jm = got[k]
        trs2, glob2 = sc.read_actor_nodes(n, i.n_nodes)
        assert same(trs, trs2) and same(glob, glob2) and same(jm, sc.read_actor_matrices(n, i.n_joints)) and same(xf[k], xf2[n]), times[k]
    sc.close()


# ---- 3. the weights kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_targets", TARGET_COUNTS)
def test_spline_weight_rows_equal_the_host_rule(rt, quads, n_targets):
    times = channel_times(QUAD_TIMES)
    assert len(times) == 11
    sc, c = posed_scene(rt, quads[n_targets], len(times))
    g, keys = c[1], c[2]
    clip = g.bake_clip(0)
    assert clip.morph(0)["interpolation"] == abi.CLIP_CUBICSPLINE and clip.morph(0)["n_targets"] == n_targets
    cid = sc.attach_clip(clip)
    sc.pose_actors([(cid, t, None, None, 0) for t in times], [(keys[k][0], k, None, rt.ClipWeights(0)) for k in range(len(times))], None)
    info, sp = sc.actor_pose_info(), sc.spline_pose_info()
    assert (info.items, info.weight_items, info.launches, info.read_backs, info.refused_item) == (len(times), len(times), 4, 1, NONE)
    assert (sp.spline_weight_rows, sp.plain_weight_rows) == (len(times), 0)
    counts = []
    for k, t in enumerate(times):
        want_at, want_w = compact(clip.weights_host(t, 0))
        got_at, got_w = sc.read_item_active(k, n_targets)
        assert got_at.tolist() == want_at.tolist(), t
        assert np.array_equal(bits(got_w), bits(want_w)), t
        assert sc.mesh_morph_info(keys[k][0]).n_active == len(want_at), t
        counts.append(len(want_at))
    assert counts[0] == 0 and counts[-1] == n_targets                         # key 0 is all zeros, key 2 has none
    if n_targets > 5:
        assert counts[times.index(0.75)] < n_targets                         # the zeros and the -0 of key 1 are left out
    sc.close()


def test_spline_plain_and_host_weights_in_one_call(rt, quads):
    """Two cubic-set items, a LINEAR-set item and a host-weights item together: three kernels in front of the posing kernel."""
    sc, c = posed_scene(rt, quads[65], 4)
    g, keys = c[1], c[2]
    cubic, linear = g.bake_clip(0), g.bake_clip(1)
    ids = (sc.attach_clip(cubic), sc.attach_clip(linear))
    times = (0.4, 1.1, 0.9)
    host_w = g.morph_weights(1, 1.6, 0)
    actors = [(ids[0], times[0], None, None, 0), (ids[1], times[1], None, None, 0), (ids[0], times[2], None, None, 0)]
    items = [(keys[0][0], 0, None, rt.ClipWeights(0)), (keys[1][0], 1, None, rt.ClipWeights(0)), (keys[2][0], None, None, host_w), (keys[3][0], 2, None, rt.ClipWeights(0))]
    sc.pose_actors(actors, items, None)
    info, sp = sc.actor_pose_info(), sc.spline_pose_info()
    assert (info.items, info.weight_items, info.launches, info.read_backs) == (4, 3, 3 + 2, 1)
    assert (sp.spline_weight_rows, sp.plain_weight_rows, sp.cubic_channels) == (2, 1, 0)
    for k, want in ((0, cubic.weights_host(times[0], 0)), (1, linear.weights_host(times[1], 0)), (2, host_w), (3, cubic.weights_host(times[2], 0))):
        want_at, want_w = compact(want)
        got_at, got_w = sc.read_item_active(k, 65)
        assert got_at.tolist() == want_at.tolist() and np.array_equal(bits(got_w), bits(want_w)), k
    sc.pose_actors(actors[1:2], [(keys[1][0], 0, None, rt.ClipWeights(0))], None)      # without a spline row the call is the one it has always been
    info, sp = sc.actor_pose_info(), sc.spline_pose_info()
    assert (info.launches, sp.spline_weight_rows, sp.plain_weight_rows, sp.spline_weights_ms) == (4, 0, 1, 0.0)
    sc.close()


# ---- 4. cross-fades -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_blended_actors_equal_the_host_blend_rule(rt, hip, rig, pair):
    g, clips = rig
    clip_a, clip_b = clips[PAIRS[pair][0]], clips[PAIRS[pair][1]]
    i = clip_a.info
    fades = [(ta, tb, w) for w in (0.0, 0.5, 1.0) for ta, tb in ((0.3, 1.7), (0.625, 0.625), (1.3, 0.1), (2.5, 0.95))]
    blend_sc, c = posed_scene(rt, SPLINE_RIG, len(fades))
    plain_sc, _ = posed_scene(rt, SPLINE_RIG, len(fades))
    desc, keys, skins = c[0], c[2], c[6]
    ida, idb = blend_sc.attach_clip(clip_a), blend_sc.attach_clip(clip_b)
    assert (ida, idb) == (plain_sc.attach_clip(clip_a), plain_sc.attach_clip(clip_b))
    ni = i.n_instances

    def items_of(copy):
        return [(keys[copy][b], copy, skin, None) for b, skin in enumerate(skins) if skin >= 0] + [(keys[copy][FACE_BLAS], copy, None, rt.ClipWeights(FACE_BLAS))]
    items = [it for copy in range(len(fades)) for it in items_of(copy)]
    out = tensor_of(ni * len(fades))
    blend_sc.pose_actors_blended([(ida, ta, idb, tb, w, None, None, k * ni) for k, (ta, tb, w) in enumerate(fades)], items, out, keep_nodes=True, keep_sources=True)
    info, sp = blend_sc.actor_pose_info(), blend_sc.spline_pose_info()
    assert (info.actors, info.items, info.weight_items, info.launches, info.read_backs, info.refused_actor, info.refused_item) == (len(fades), 3 * len(fades), len(fades), 4, 1, NONE, NONE)
    assert (sp.spline_weight_rows, sp.plain_weight_rows) == (len(fades), 0)
    xf = out.cpu().numpy().reshape(len(fades), ni, 12)
    others = [k for k in range(ni) if k != PROP_INSTANCE]
    keep = off_prop(clip_a)
    for k, (ta, tb, w) in enumerate(fades):
        what = "%s t = (%r, %r) w = %r" % (pair, ta, tb, w)
        trs = blend_sc.read_actor_nodes(k, i.n_nodes)[0]
        jm = blend_sc.read_actor_matrices(k, i.n_joints)
        src_a, src_b = blend_sc.read_actor_sources(k, i.n_nodes)
        want_a, want_b = clip_a.sample_host(ta), clip_b.sample_host(tb)
        assert_trs_contract(src_a, want_a, rotation_classes(clip_a, ta), what)
        assert_trs_contract(src_b, want_b, rotation_classes(clip_b, tb), what)
        assert same(src_a[keep], want_a[keep]) and same(src_b[keep], want_b[keep]), what + ": kept sources"
        assert same(trs, rt.clip_blend_host(src_a, src_b, w)), what + ": the blended records of the device's sources"
        assert same(trs[keep], rt.clip_blend_host(want_a, want_b, w)[keep]), what + ": blended records"
        want_jm, want_xf = clip_a.pose_blend_host(ta, clip_b, tb, w)
        assert same(jm, want_jm), what + ": joint matrices"
        assert same(xf[k][others], want_xf[others]), what + ": instance transforms"
        assert same(xf[k], clip_a.compose_records_host(trs)[1]), what + ": the composition of the device's records"
        want_at, want_w = compact(clip_a.blend_weights_host(ta, clip_b, tb, w, FACE_BLAS))
        got_at, got_w = blend_sc.read_item_active(3 * k + 2, 3)
        assert got_at.tolist() == want_at.tolist() and np.array_equal(bits(got_w), bits(want_w)), what + ": blended weights"
    # the end weights against the plain call, device against device
    ends = [k for k, f in enumerate(fades) if f[2] in (0.0, 1.0)]
    plain = [((idb, fades[k][1]) if fades[k][2] else (ida, fades[k][0])) + (None, None, n * ni) for n, k in enumerate(ends)]
    out2 = tensor_of(ni * len(ends))
    plain_sc.pose_actors(plain, [it for n in range(len(ends)) for it in items_of(n)], out2, keep_nodes=True)
    xf2 = out2.cpu().numpy().reshape(len(ends), ni, 12)
    got, want = all_bytes(hip, blend_sc, desc), all_bytes(hip, plain_sc, desc)
    order = [m.key for m in desc.meshes]
    for n, k in enumerate(ends):
        assert same(xf[k], xf2[n]) and same(blend_sc.read_actor_matrices(k, i.n_joints), plain_sc.read_actor_matrices(n, i.n_joints)), fades[k]
        assert same(blend_sc.read_actor_nodes(k, i.n_nodes)[0], plain_sc.read_actor_nodes(n, i.n_nodes)[0]), fades[k]
        for b in (0, 1, FACE_BLAS):
            assert got[order.index(keys[k][b])] == want[order.index(keys[n][b])], (fades[k], b)
    blend_sc.close(); plain_sc.close()


def test_blended_weight_rows_at_65_targets(rt, quads):
    sc, c = posed_scene(rt, quads[65], 9)
    g, keys = c[1], c[2]
    clips = {0: g.bake_clip(0), 1: g.bake_clip(1)}
    ids = {a: sc.attach_clip(clip) for a, clip in clips.items()}
    fades = [(a, b, ta, tb, w) for (a, b) in sorted(PAIRS.values()) for ta, tb, w in ((0.4, 1.1, 0.0), (0.5, 0.75, 0.5), (1.9, 0.3, 1.0))]
    sc.pose_actors_blended([(ids[a], ta, ids[b], tb, w, None, None, 0) for a, b, ta, tb, w in fades], [(keys[k][0], k, None, rt.ClipWeights(0)) for k in range(9)], None)
    info, sp = sc.actor_pose_info(), sc.spline_pose_info()
    assert (info.weight_items, info.launches) == (9, 4) and (sp.spline_weight_rows, sp.plain_weight_rows) == (9, 0)
    for k, (a, b, ta, tb, w) in enumerate(fades):
        want_at, want_w = compact(clips[a].blend_weights_host(ta, clips[b], tb, w, 0))
        got_at, got_w = sc.read_item_active(k, 65)
        assert got_at.tolist() == want_at.tolist() and np.array_equal(bits(got_w), bits(want_w)), fades[k]
    # a LINEAR pair beside a cubic one: a plain blended row and a spline row, one kernel each
    sc.pose_actors_blended([(ids[1], 0.4, ids[1], 1.1, 0.25, None, None, 0), (ids[0], 0.4, ids[1], 1.1, 0.25, None, None, 0)],
                           [(keys[0][0], 0, None, rt.ClipWeights(0)), (keys[1][0], 1, None, rt.ClipWeights(0))], None)
    info, sp = sc.actor_pose_info(), sc.spline_pose_info()
    assert info.launches == 5 and (sp.spline_weight_rows, sp.plain_weight_rows) == (1, 1)
    for k, a in ((0, 1), (1, 0)):
        want_at, want_w = compact(clips[a].blend_weights_host(0.4, clips[1], 1.1, 0.25, 0))
        got_at, got_w = sc.read_item_active(k, 65)
        assert got_at.tolist() == want_at.tolist() and np.array_equal(bits(got_w), bits(want_w)), k
    sc.close()


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------------
def test_posed_vertices_equal_the_host_route(rt, hip, rig):
    """pose_actors on the cubic clip against pose_meshes with the loader's matrices and weights (sr_gltf_pose and
    sr_gltf_morph_weights under SAMPLE): the vertices of every mesh, byte for byte."""
    g, clips = rig
    dev, c = posed_scene(rt, SPLINE_RIG)
    host, _ = posed_scene(rt, SPLINE_RIG)
    desc, keys, skins = c[0], c[2], c[6]
    cid = dev.attach_clip(clips[0])
    for t in (0.1, 0.625, 1.0, 1.15, 1.999, 3.0):
        dev.pose_actors([(cid, t, None, None, 0)], [(keys[0][0], 0, 0, None), (keys[0][1], 0, 1, None), (keys[0][FACE_BLAS], 0, None, rt.ClipWeights(FACE_BLAS))], None)
        host.pose_meshes([(keys[0][0], None, g.pose(0, t, 0)[1]), (keys[0][1], None, g.pose(0, t, 1)[1]), (keys[0][FACE_BLAS], g.morph_weights(0, t, FACE_BLAS), None)])
        assert all_bytes(hip, dev, desc) == all_bytes(hip, host, desc), t
        assert dev.mesh_morph_info(keys[0][FACE_BLAS]).n_active == host.mesh_morph_info(keys[0][FACE_BLAS]).n_active
    assert all_bytes(hip, dev, desc) != [m.vertices.tobytes() for m in desc.meshes]
    dev.close(); host.close()


def test_a_renderer_frame_equals_the_host_route(rt, rig):
    import torch
    g, clips = rig
    camera = ((0.5, 2.0, 8.0), (0.5, 1.0, 0.0), 45.0)
    t = 1.0                                             # a key of the LINEAR rotation: the prop's transform is in the bit-equal class too
    frames = []
    for device_route in (True, False):
        r = rt.Renderer((64, 48), devices=[0])
        loaded = r.load_scene(g)
        r.attach_skins(g, loaded)
        r.attach_morphs(g, loaded)
        keys = [int(k) for k in loaded.keys]
        out = torch.zeros((loaded.n_transforms, 12), dtype=torch.float32, device="cuda:0")
        want_xf = g.pose(0, t)[0]
        if device_route:
            cid = r.attach_clip(clips[0])
            r.pose_actors([(cid, t, None, loaded.instance_rows(0), 0)], [(keys[0], 0, 0, None), (keys[1], 0, 1, None), (keys[FACE_BLAS], 0, None, rt.ClipWeights(FACE_BLAS))], out)
            sp = r.spline_pose_info()
            assert (sp.spline_weight_rows, sp.plain_weight_rows, sp.cubic_channels) == (1, 0, 6)
            rows = loaded.instance_rows(0)
            assert same(out.cpu().numpy()[rows], want_xf)
        else:
            r.pose_meshes([(keys[0], None, g.pose(0, t, 0)[1]), (keys[1], None, g.pose(0, t, 1)[1]), (keys[FACE_BLAS], g.morph_weights(0, t, FACE_BLAS), None)])
        xf = np.zeros((loaded.n_transforms, 12), np.float32)
        xf[loaded.instance_rows(0)] = want_xf
        frames.append(r.render_to_host_memory(camera, loaded.grouped(xf)).copy())
        r.close()
    assert np.array_equal(frames[0], frames[1])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_clip_baked_under_refuse_still_refuses_its_cubic_set(rt, quads):
    sc, c = posed_scene(rt, quads[65], 1, sample=False)
    g, keys = c[1], c[2]
    kept = g.bake_clip(0)                                                     # the weights channel does not refuse the bake
    assert kept.morph(0)["state"] == abi.CLIP_MORPH_UNAVAILABLE
    cid = sc.attach_clip(kept)
    g.set_cubicspline(True)                                                   # the clip keeps what it was baked with
    call = lambda: sc.pose_actors([(cid, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(0))], None)   # noqa: E731
    assert refused(rt, call) == (ERR_UNSUPPORTED, "pose_actors: item 0: " + CUBIC)
    assert sc.actor_pose_info().calls == 0
    sid = sc.attach_clip(g.bake_clip(0))
    sc.pose_actors([(sid, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(0))], None)
    assert sc.actor_pose_info().calls == 1 and sc.spline_pose_info().spline_weight_rows == 1
    blend = lambda: sc.pose_actors_blended([(sid, 0.5, cid, 0.5, 0.5, None, None, 0)], [(keys[0][0], 0, None, rt.ClipWeights(0))], None)   # noqa: E731
    assert refused(rt, blend) == (ERR_UNSUPPORTED, "pose_actors_blended: item 0: " + CUBIC)
    sc.close()


def test_a_cubic_scale_through_zero_refuses_the_call(rt, hip, tmp_path):
    path = str(tmp_path / "collapse.glb")
    collapsing_rig(path)
    sc, c = posed_scene(rt, path, 2)
    desc, g, keys, skins = c[0], c[1], c[2], c[6]
    clip = g.bake_clip(0)
    assert refused(rt, lambda: g.pose(0, 1.0, 0)) == (ERR_UNSUPPORTED, "sr_gltf_pose: " + SINGULAR)
    cid = sc.attach_clip(clip)
    blas = skins.index(0)
    items = [(keys[k][blas], k, 0, None) for k in range(2)]
    before = all_bytes(hip, sc, desc)
    assert refused(rt, lambda: sc.pose_actors([(cid, 0.5, None, None, 0), (cid, 1.0, None, None, 0)], items, None)) == (ERR_UNSUPPORTED, "pose_actors: actor 1: " + SINGULAR)
    info = sc.actor_pose_info()
    assert (info.launches, info.refused_actor, sc.spline_pose_info().cubic_channels) == (2, 1, 2)
    assert all_bytes(hip, sc, desc) == before
    sc.pose_actors([(cid, 0.5, None, None, 0), (cid, 1.5, None, None, 0)], items, None)       # the scene goes on
    assert sc.actor_pose_info().launches == 3
    sc.close()
