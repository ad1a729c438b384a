"""Morph weights through an actor's layer stack on the device (sr_scene_pose_actors_layered with SR_ACTORS_LAYER_WEIGHTS:
clip_layer_weights_kernel samples every layer's morph set for an item's blas, applies the layer rule and compacts the weights that
are not 0 into the active list pose_batch_kernel reads). The reference is the host rule sr_clip_weights_layers_host, itself held to
a pure-Python restatement and to exact arithmetic by test_clip_layer_weights_host.py, and the host's compaction of it. The
arithmetic is +, -, x, / on fp32 and fp64 with no libm, so the contract is equality: count, indices and weight bits, with no
tolerance and no case left out. Without the flag the call is what it was."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clip_morph_util import BIG, MORPH_BAR, ONE, TWO, ZEROS_AT, bits, compact, many_targets, one_morphed_quad, set_times  # noqa: E402
from clip_util import crowd  # noqa: E402
from test_gpu_mesh_skin import device_vertices  # noqa: E402

NONE = 0xFFFFFFFF
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
F32 = np.float32
BELOW_ONE = float(np.nextafter(F32(1), F32(0)))
WEIGHTS = [0.0, 1.0, 0.25, 0.5, BELOW_ONE]
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"


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


class Rig:
    """A scene of `copies` copies of a file with every rig and morph attached, its clips baked and attached under the keys of
    `animations` (an animation index; "plain": animation 1 baked without cubic mode), and node masks attached by key."""

    def __init__(self, rt, path, copies, animations):
        c = crowd(rt, path, copies)
        self.rt, self.path, self.desc, self.g, self.keys = rt, path, c[0], c[1], c[2]
        self.sc = rt.Scene(0).load(self.desc)
        for key, (inf, nj) in c[3].items():
            self.sc.set_mesh_skin(key, inf, nj)
        self.targets = {}
        for b in range(self.g.n_blases):
            d = self.g.blas_morph(b)[0]
            if d is not None:
                self.targets[b] = len(d)
                for copy in range(copies):
                    self.sc.set_mesh_morph(self.keys[copy][b], d)
        self.clips = {}
        if "plain" in animations:
            self.clips["plain"] = self.g.bake_clip(1)
        self.g.set_cubicspline(True)
        for a in animations:
            if a != "plain":
                self.clips[a] = self.g.bake_clip(a)
        self.ids = {a: self.sc.attach_clip(clip) for a, clip in self.clips.items()}
        self.masks = {}

    def mesh_node(self, blas, clip=None):
        clip = clip or next(iter(self.clips.values()))
        return int(np.flatnonzero(clip.layout()[0]["gltf_node"] == clip.morph(blas)["gltf_node"])[0])

    def add_mask(self, name, host):
        self.masks[name] = (host, self.sc.attach_node_mask(host))

    def node_masks(self, blas):
        """zero / half / one: that value on the blas's mesh node, the opposite end elsewhere; subtree: sr_clip_subtree_mask of the
        mesh node, 0.5 inside and 0 outside."""
        clip = next(iter(self.clips.values()))
        node = self.mesh_node(blas)
        for name, (here, elsewhere) in (("zero", (0.0, 1.0)), ("half", (0.5, 0.0)), ("one", (1.0, 0.0))):
            m = np.full(clip.info.n_nodes, elsewhere, F32)
            m[node] = here
            self.add_mask((name, blas), m)
        self.add_mask(("subtree", blas), clip.subtree_mask(clip.morph(blas)["gltf_node"], 0.5, 0.0))

    def device_stack(self, stack):
        return [(self.ids[c], t, w, mode, None if m is None else self.masks[m][1], r) for c, t, w, mode, m, r in stack]

    def host_stack(self, stack):
        return [(self.clips[c], t, w, mode, None if m is None else self.masks[m][0], r) for c, t, w, mode, m, r in stack]

    def host_weights(self, stack, blas):
        return self.rt.clip_weights_layers_host(self.host_stack(stack), blas)

    def pose(self, plan, flag=True, extra_items=()):
        """One layered call: an actor and a morph-only clip-weighted item for every (key, blas, stack) of the plan."""
        actors = [(self.device_stack(st), None, None, 0) for _, _, st in plan]
        items = list(extra_items) + [(key, a, None, self.rt.ClipWeights(b)) for a, (key, b, _) in enumerate(plan)]
        self.sc.pose_actors_layered(actors, items, None, layer_weights=flag)

    def lists(self, plan, first=0):
        return [self.sc.read_item_active(first + i, self.targets[b]) for i, (_, b, _) in enumerate(plan)]

    def all_bytes(self, hip):
        return [device_vertices(hip, self.sc, slot, len(m.vertices)).tobytes() for slot, m in enumerate(self.desc.meshes)]

    def close(self):
        self.sc.close()


def base(c, t):
    return (c, t, 1.0, "override", None, 0.0)


def refused(rt, call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def same_lists(a, b):
    return len(a) == len(b) and all(x[0].tolist() == y[0].tolist() and np.array_equal(bits(x[1]), bits(y[1])) for x, y in zip(a, b))


def actor_tuple(i, calls=True):
    return (i.actors, i.items, i.nodes, i.channels, i.upload_bytes, i.launches, i.read_backs, i.refused_actor, i.refused_item, i.weight_items) + ((i.calls,) if calls else ())


def spline_tuple(sc):
    i = sc.spline_pose_info()
    return (i.spline_weight_rows, i.plain_weight_rows, i.cubic_channels)


def weights_tuple(sc):
    i = sc.layer_weights_info()
    return (i.rows, i.samples, i.cubic_samples, i.table_bytes)


def check_plan(rig, plan, what):
    """The flagged call of the plan: every item's active list as the posing kernel read it is the host's compaction of the host
    rule (count, indices, weight bits), and the figures count the one new kernel."""
    rig.pose(plan)
    sc = rig.sc
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.weight_items, info.launches, info.read_backs, info.refused_item) == (len(plan), len(plan), len(plan), 4, 1, NONE), what
    n_layers = sum(len(st) for _, _, st in plan)
    samples = sum(2 if mode == "additive" else 1 for _, _, st in plan for _, _, _, mode, _, _ in st)
    cubic = sum((2 if mode == "additive" else 1) for _, b, st in plan for c, _, _, mode, _, _ in st
                if rig.clips[c].morph(b)["n_keys"] and rig.clips[c].morph(b)["interpolation"] == 2)
    assert weights_tuple(sc) == (len(plan), samples, cubic, 32 * len(plan) + 16 * n_layers), what
    assert spline_tuple(sc)[:2] == (0, 0), what
    for i, (key, b, st) in enumerate(plan):
        want_at, want_w = compact(rig.host_weights(st, b))
        got_at, got_w = sc.read_item_active(i, rig.targets[b])
        assert got_at.tolist() == want_at.tolist(), (what, i, b, st)
        assert np.array_equal(bits(got_w), bits(want_w)), (what, i, b, st)
        assert sc.mesh_morph_info(key).n_active == len(want_at), (what, i, b, st)


def batches(rig, cases):
    """(blas, stack) cases -> plans of one case per copy."""
    n = len(rig.keys)
    for first in range(0, len(cases), n):
        yield [(rig.keys[copy][b], b, st) for copy, (b, st) in enumerate(cases[first:first + n])]


@pytest.fixture(scope="module")
def bar(rt):
    rig = Rig(rt, MORPH_BAR, 8, (0, 1, -1, "plain"))
    assert rig.targets == {0: 3, 1: 2}
    for b in (0, 1):
        rig.node_masks(b)
    yield rig
    rig.close()


@pytest.fixture(scope="module")
def many(rt, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("layer_weights") / "many.glb")
    many_targets(path)
    rig = Rig(rt, path, 5, (0, 1, -1))
    assert rig.targets == {BIG: 130, ONE: 1, TWO: 2}
    for b in (BIG, ONE, TWO):
        rig.node_masks(b)
    yield rig
    rig.close()


def bar_times(bar, blas):
    return sorted(set(set_times(bar.clips[0], blas)) | set(set_times(bar.clips[1], blas)))


# ---- without the flag ------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_the_call_is_what_it_was(rt, hip):
    """The same unflagged call on a scene that never used the flag and on one that does in between: active lists, posed bytes and
    figures are equal before and after the flagged call."""
    never, used = Rig(rt, MORPH_BAR, 2, (0, 1, -1)), Rig(rt, MORPH_BAR, 2, (0, 1, -1))
    stacks = [[base(0, 0.3), (1, 0.7, 0.5, "additive", None, 0.0)], [base(1, 0.6), (0, 1.2, 0.25, "override", None, 0.0), (-1, 0.0, 0.5, "additive", None, 0.0)]]
    plan = lambda r: [(r.keys[copy][b], b, stacks[copy]) for copy in (0, 1) for b in (0, 1)]   # noqa: E731
    for step in ("before", "after"):
        never.pose(plan(never), flag=False); used.pose(plan(used), flag=False)
        assert same_lists(never.lists(plan(never)), used.lists(plan(used))), step
        # the weights are the base layer's: a cubic set is a spline row, another a plain row
        assert same_lists(used.lists(plan(used)), [compact(used.clips[st[0][0]].weights_host(st[0][1], b)) for _, b, st in plan(used)])
        assert actor_tuple(never.sc.actor_pose_info(), calls=False) == actor_tuple(used.sc.actor_pose_info(), calls=False), step
        assert spline_tuple(never.sc) == spline_tuple(used.sc) == (1, 3, spline_tuple(never.sc)[2]), step
        assert used.sc.actor_pose_info().launches == 5 and weights_tuple(used.sc) == weights_tuple(never.sc) == (0, 0, 0, 0), step
        assert never.all_bytes(hip) == used.all_bytes(hip), step
        if step == "before":
            used.pose(plan(used))
            assert weights_tuple(used.sc)[0] == 4 and used.sc.actor_pose_info().launches == 4 and spline_tuple(used.sc)[:2] == (0, 0)
            assert never.all_bytes(hip) != used.all_bytes(hip)                   # the layers above the base do something
    assert (never.sc.actor_pose_info().calls, used.sc.actor_pose_info().calls) == (2, 3)
    never.close(); used.close()


def test_the_other_calls_refuse_the_flag(rt, bar):
    from sunray_amd import abi
    args = rt.ActorArgs([(bar.ids[0], 0.3, None, None, 0)], [])
    assert refused(rt, lambda: rt.check(rt.lib().sr_scene_pose_actors(bar.sc._h, args.actors, 1, args.items, 0, None, C.c_uint32(abi.ACTORS_LAYER_WEIGHTS), None))) == \
        (ERR_INVALID_ARG, "pose_actors: unknown flag bits (SR_ACTORS_KEEP_NODES is the flag)")
    blended = rt.BlendedActorArgs([(bar.ids[0], 0.3, bar.ids[1], 0.2, 0.5, None, None, 0)], [])
    assert refused(rt, lambda: rt.check(rt.lib().sr_scene_pose_actors_blended(bar.sc._h, blended.actors, 1, blended.items, 0, None, C.c_uint32(abi.ACTORS_LAYER_WEIGHTS), None))) == \
        (ERR_INVALID_ARG, "pose_actors_blended: unknown flag bits (SR_ACTORS_KEEP_NODES and SR_ACTORS_KEEP_SOURCES are the flags)")
    layered = rt.LayeredActorArgs([([(bar.ids[0], 0.3, 1.0, "override", None, 0.0)], None, None, 0)], [])
    assert refused(rt, lambda: rt.check(rt.lib().sr_scene_pose_actors_layered(bar.sc._h, layered.actors, 1, layered.items, 0, None, C.c_uint32(16), None))) == \
        (ERR_INVALID_ARG, "pose_actors_layered: unknown flag bits (SR_ACTORS_KEEP_NODES, SR_ACTORS_KEEP_LAYERS and SR_ACTORS_LAYER_WEIGHTS are the flags)")


# ---- byte equalities with the flag ------------------------------------------------------------------------------------------------------
def test_one_layer_equals_pose_actors(rt, hip, bar):
    for a in (0, 1, -1):
        for b in (0, 1):
            for plan in batches(bar, [(b, [base(a, t)]) for t in bar_times(bar, b)]):
                bar.sc.pose_actors([(bar.ids[a], st[0][1], None, None, 0) for _, _, st in plan], [(key, i, None, rt.ClipWeights(b)) for i, (key, _, _) in enumerate(plan)], None)
                want, want_bytes = bar.lists(plan), bar.all_bytes(hip)
                bar.pose(plan)
                assert same_lists(bar.lists(plan), want), (a, b)
                assert bar.all_bytes(hip) == want_bytes, (a, b)
                assert weights_tuple(bar.sc)[0] == len(plan)


def test_two_unmasked_override_layers_equal_pose_actors_blended(rt, hip, bar):
    n = 0
    for a, o in ((0, 1), (1, 0), (0, -1), (1, 1)):
        for b in (0, 1):
            times = bar_times(bar, b)
            cases = [(b, [base(a, t), (o, times[(3 * k + 1) % len(times)], WEIGHTS[k % 5], "override", None, 0.0)]) for k, t in enumerate(times)]
            for plan in batches(bar, cases):
                bar.sc.pose_actors_blended([(bar.ids[a], st[0][1], bar.ids[o], st[1][1], st[1][2], None, None, 0) for _, _, st in plan],
                                           [(key, i, None, rt.ClipWeights(b)) for i, (key, _, _) in enumerate(plan)], None)
                want, want_bytes = bar.lists(plan), bar.all_bytes(hip)
                bar.pose(plan)
                assert same_lists(bar.lists(plan), want), (a, o, b)
                assert bar.all_bytes(hip) == want_bytes, (a, o, b)
                n += len(plan)
    assert n > 150


def mixed_stack(k, n_layers, times, mask_names, blas, clip_keys):
    """A stack of n_layers layers: the clips, modes, WEIGHTS, masks and times in turn, from k on."""
    layers = [base(clip_keys[k % len(clip_keys)], times[k % len(times)])]
    for l in range(1, n_layers):
        mask = mask_names[(k + l) % len(mask_names)]
        layers.append((clip_keys[(k + l) % len(clip_keys)], times[(3 * k + 5 * l) % len(times)], WEIGHTS[(k + 2 * l) % 5], "additive" if (k + l) % 2 else "override",
                       None if mask is None else (mask, blas), times[(k + 7 * l) % len(times)]))
    return layers


def test_stacks_of_3_and_8_layers_equal_the_host_rule(rt, bar):
    """LINEAR, STEP, cubic and static clips in one stack, override and additive layers, masks of 0 / 0.5 / 1 on the mesh node and a
    subtree mask."""
    names = [None, "zero", "half", "one", "subtree"]
    n = 0
    for b in (0, 1):
        times = bar_times(bar, b)
        cases = [(b, mixed_stack(k, (3, 8)[k % 2], times, names, b, [0, 1, -1])) for k in range(32)]
        for plan in batches(bar, cases):
            check_plan(bar, plan, "bar blas %d" % b)
            n += len(plan)
    assert n == 64
    # every interpolation is in a stack, and the masks and the additive layers do something
    assert {bar.clips[a].morph(0)["interpolation"] if bar.clips[a].morph(0)["n_keys"] else -1 for a in (0, 1, -1)} == {0, 2, -1}
    assert bar.clips[0].morph(1)["interpolation"] == 1
    st = [base(0, 0.3), (1, 0.7, 0.5, "additive", None, 0.0)]
    assert not np.array_equal(bar.host_weights(st, 0), bar.host_weights(st[:1], 0))
    assert not np.array_equal(bar.host_weights(st, 0), bar.host_weights([st[0], st[1][:4] + (("half", 0), 0.0)], 0))


# ---- chunk edges -----------------------------------------------------------------------------------------------------------------------
def test_chunk_edges_at_63_64_65_targets(rt, tmp_path):
    """One quad of 63, 64 and 65 targets: the base at key times, next to them on both sides and between them, an additive layer of the
    same clip and an override layer of the static pose on top."""
    for nt in (63, 64, 65):
        path = str(tmp_path / ("quad%d.glb" % nt))
        one_morphed_quad(path, nt)
        rig = Rig(rt, path, 5, (0, -1))
        assert rig.targets == {0: nt}
        rig.node_masks(0)
        times = set_times(rig.clips[0], 0)
        cases = [(0, [base(0, t), (0, times[(k + 3) % len(times)], WEIGHTS[k % 5], "additive", (None, ("half", 0))[k % 2], times[(k + 1) % len(times)]),
                      (-1, 0.0, (0.0, 0.25, 1.0)[k % 3], "override", None, 0.0)][:1 + k % 3 if k % 4 else 3]) for k, t in enumerate(times)]
        for plan in batches(rig, cases):
            check_plan(rig, plan, "quad of %d targets" % nt)
        # an override layer of the static pose (no weights) at weight 1: every weight is 0
        plan = [(rig.keys[0][0], 0, [base(0, 0.3), (-1, 0.0, 1.0, "override", None, 0.0)])]
        check_plan(rig, plan, "all zero")
        assert rig.sc.mesh_morph_info(rig.keys[0][0]).n_active == 0 and rig.sc.read_item_active(0, nt)[0].size == 0
        rig.close()


def test_130_targets_with_zeros_at_the_chunk_ends(rt, many):
    times = sorted(set(set_times(many.clips[0], BIG)) | set(set_times(many.clips[1], BIG)))
    names = [None, "half", "zero", "one", "subtree"]
    cases = [(BIG, mixed_stack(k, 1 + k % 4, times, names, BIG, [0, 1, -1])) for k in range(len(times))]
    for plan in batches(many, cases):
        check_plan(many, plan, "130 targets")
    # the result has zeros exactly at targets 0, 63, 64, 127, 128, 129 and a -0 at target 5: from the base under identity layers ...
    at_key = [base(0, 0.5), (1, 1.0, 0.5, "additive", None, 1.0), (1, 2.0, 0.0, "override", None, 0.0), (0, 1.0, 0.75, "override", ("zero", BIG), 0.0)]
    # ... and from an override layer at weight 1 on top of a base that has none
    on_top = [base(0, 1.0), (1, 0.5, 1.0, "override", None, 0.0)]
    # a row whose every weight is 0: key 0 is all zeros
    nothing = [base(0, 0.0), (1, 0.25, 0.5, "additive", None, 0.1)]
    for st in (at_key, on_top):
        w = many.host_weights(st, BIG)
        assert [k for k in range(130) if w[k] == 0] == sorted(ZEROS_AT + (5,)) and np.signbit(w[5])
    assert not many.host_weights(nothing, BIG).any() and many.host_weights([base(0, 1.0)], BIG).all()
    plan = [(many.keys[0][BIG], BIG, at_key), (many.keys[1][BIG], BIG, on_top), (many.keys[2][BIG], BIG, nothing), (many.keys[3][BIG], BIG, [base(0, 1.0)])]
    check_plan(many, plan, "zeros at the chunk ends")
    assert [many.sc.mesh_morph_info(many.keys[c][BIG]).n_active for c in range(4)] == [123, 123, 0, 130]
    assert many.sc.read_item_active(2, 130)[0].size == 0


def test_five_rows_of_different_sizes_and_canaries(rt, hip, many):
    """Five clip-weighted items (two blocks of four waves, the second partly empty) whose sets have 130, 1, 2, 130 and 2 targets in
    neighbouring waves, beside a host-weighted item of three active targets. The host's list lies directly in front of the slots in
    the index array and in the weight array, and, the 3 + 265 entries being a whole number of 16-byte pieces, its first weight lies
    directly behind the last index slot: the word before the first slot of either array and the word after the last index slot are
    the host's own, read back unchanged. Between the slots an item's neighbours are the other items' slots, which hold exactly their
    lists, a full one among them. The posed vertices are those of a twin scene posed by pose_meshes with the host rule's weights."""
    times = set_times(many.clips[0], BIG)
    names = [None, "half", "one"]
    order = [BIG, ONE, TWO, BIG, TWO]
    plan = [(many.keys[copy][b], b, mixed_stack(copy + 2, (3, 8, 2, 5, 4)[copy], times, names, b, [0, 1, -1])) for copy, b in enumerate(order)]
    plan[3] = (plan[3][0], BIG, [base(0, 1.0), (1, 2.0, 0.0, "additive", None, 0.0)])         # a full slot of 130
    host_w = np.zeros(130, F32)
    host_w[[7, 64, 129]] = (0.75, -0.5, 0.125)
    host_key = many.keys[1][BIG]
    assert (3 + sum(many.targets[b] for b in order)) % 4 == 0                 # no pad word between the index array and the weight array
    many.pose(plan, extra_items=[(host_key, None, None, host_w)])
    sc = many.sc
    info = sc.actor_pose_info()
    assert (info.actors, info.items, info.weight_items, info.launches) == (5, 6, 5, 4)
    got = sc.read_item_active(0, 130)
    assert got[0].tolist() == [7, 64, 129] and np.array_equal(bits(got[1]), bits(host_w[[7, 64, 129]]))      # the canaries
    wants = [many.host_weights(st, b) for _, b, st in plan]
    assert same_lists(many.lists(plan, first=1), [compact(w) for w in wants])
    assert len(compact(wants[3])[0]) == 130
    twin = Rig(rt, many.path, 5, ())
    twin.sc.pose_meshes([(key, w, None) for (key, _, _), w in zip(plan, wants)] + [(host_key, host_w, None)])
    order = [m.key for m in many.desc.meshes]
    got, want = many.all_bytes(hip), twin.all_bytes(hip)
    for key, w in [(key, w) for (key, _, _), w in zip(plan, wants)] + [(host_key, host_w)]:   # the scene's other meshes keep earlier tests' poses
        at = order.index(key)
        assert got[at] == want[at], key
        assert (got[at] != many.desc.meshes[at].vertices.tobytes()) == bool(w.any()), key
    assert sum(bool(w.any()) for w in wants) >= 4
    twin.close()


# ---- host refusals ---------------------------------------------------------------------------------------------------------------------
def test_host_refusals_come_before_any_device_work(rt, hip, bar, tmp_path):
    sc = bar.sc
    good = [(bar.keys[0][0], 0, [base(0, 0.5), (1, 0.7, 0.5, "additive", None, 0.0)]), (bar.keys[1][1], 1, [base(1, 0.5), (0, 0.7, 0.5, "override", None, 0.0)])]
    bar.pose(good)
    state = lambda: (bar.all_bytes(hip), actor_tuple(sc.actor_pose_info()), weights_tuple(sc), spline_tuple(sc), [(at.tolist(), w.tobytes()) for at, w in bar.lists(good)],   # noqa: E731
                     [(i.n_targets, i.posed, i.n_active, i.first_bad) for i in (sc.mesh_morph_info(k) for k, _, _ in good)])
    before = state()
    assert before[1][5] == 4 and before[2][0] == 2
    I = "pose_actors_layered: item 1: layer "
    unavailable = [base(1, 0.5), ("plain", 0.7, 0.0, "override", None, 0.0)]             # at weight 0, checked like any other
    cases = [
        ([good[0], (bar.keys[1][0], 0, unavailable)], ERR_UNSUPPORTED, I + "1: " + CUBIC),
        ([good[0], (bar.keys[1][0], 0, [base("plain", 0.5)])], ERR_UNSUPPORTED, I + "0: " + CUBIC),
        ([good[0], (bar.keys[1][1], 2, good[1][2])], ERR_INVALID_ARG, I + "0: the weights of blas 2 named, the layer's clip has no morph set for it"),
        ([good[0], (bar.keys[1][1], 0, good[1][2])], ERR_INVALID_ARG, I + "0: the set has 3 targets, the mesh's morph was attached with 2"),
    ]
    for plan, code, text in cases:
        assert refused(rt, lambda: bar.pose(plan)) == (code, text)
        assert state() == before, text
    # a layer's set whose n_targets differs from the base's: compatible clips of two files that differ in their targets alone
    paths = {}
    for nt in (63, 64):
        paths[nt] = str(tmp_path / ("quad%d.glb" % nt))
        one_morphed_quad(paths[nt], nt)
    rig = Rig(rt, paths[63], 1, (0,))
    other = rt.Gltf(paths[64]).bake_clip(0)
    rig.clips["other"], rig.ids["other"] = other, rig.sc.attach_clip(other)
    ok = [(rig.keys[0][0], 0, [base(0, 0.3)])]
    rig.pose(ok)
    calls = rig.sc.actor_pose_info().calls
    assert refused(rt, lambda: rig.pose([(rig.keys[0][0], 0, [base(0, 0.3), ("other", 0.5, 0.0, "override", None, 0.0)])])) == \
        (ERR_INVALID_ARG, "pose_actors_layered: item 0: layer 1: the set has 64 targets, the base layer's 63")
    assert rig.sc.actor_pose_info().calls == calls == 1
    rig.pose([(rig.keys[0][0], 0, [base(0, 0.3), ("other", 0.5, 0.5, "override", None, 0.0)])], flag=False)      # without the flag the layer's set is not read
    rig.close()


# ---- the facade ------------------------------------------------------------------------------------------------------------------------
def test_the_renderer_passes_the_flag_through(rt):
    r = rt.Renderer((64, 48), devices=[0])
    g = rt.Gltf(MORPH_BAR)
    g.set_cubicspline(True)
    loaded = r.load_scene(g)
    r.attach_skins(g, loaded)
    r.attach_morphs(g, loaded)
    clips = [g.bake_clip(a) for a in (0, 1)]
    ids = [r.attach_clip(c) for c in clips]
    keys = [int(k) for k in loaded.keys]
    stack = [(ids[0], 0.3, 1.0, "override", None, 0.0), (ids[1], 0.7, 0.5, "additive", None, 0.0)]
    r.pose_actors_layered([(stack, None, None, 0)], [(keys[1], 0, None, rt.ClipWeights(1)), (keys[0], 0, 0, rt.ClipWeights(0))], None, layer_weights=True)
    info, wi = r.actor_pose_info(), r.layer_weights_info()
    assert (info.actors, info.items, info.launches, info.weight_items) == (1, 2, 4, 2)
    assert (wi.rows, wi.samples, wi.cubic_samples, wi.table_bytes) == (2, 6, 2, 2 * 32 + 4 * 16)
    first = r.replica_scene(0)
    host = [(clips[0], 0.3, 1.0, "override", None, 0.0), (clips[1], 0.7, 0.5, "additive", None, 0.0)]
    for i, b in ((0, 1), (1, 0)):
        want = compact(rt.clip_weights_layers_host(host, b))
        got = first.read_item_active(i, 3)
        assert got[0].tolist() == want[0].tolist() and np.array_equal(bits(got[1]), bits(want[1]))
    r.close()
