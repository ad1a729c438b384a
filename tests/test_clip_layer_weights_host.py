"""The host rule of layered morph weights (sr_clip_layer_weights_host, sr_clip_weights_layers_host) against the pure-Python
restatement of tests/clip_layer_weights_reference.py, bit for bit, against exact rational arithmetic per layer step, and against
the rules it extends: one layer is sr_clip_weights_host, two unmasked override layers are sr_clip_blend_weights_host. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_layer_weights_reference as ref  # noqa: E402
from clip_morph_util import BIG, MORPH_BAR, ONE, TWO, bits, many_targets, one_morphed_quad, set_times  # noqa: E402
from sunray_amd import abi, runtime as rt  # noqa: E402

F32 = np.float32
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -5
BELOW_ONE = float(np.nextafter(F32(1), F32(0)))
WEIGHTS = [0.0, 1.0, 0.25, 0.5, BELOW_ONE]
CUBIC = "gltf: CUBICSPLINE animation samplers are not supported"


@pytest.fixture(scope="module")
def bar():
    """Bakes of morph_bar.glb: animation 0 (LINEAR on blas 0, STEP on blas 1), animation 1 in cubic mode (cubic on blas 0, defaults
    on blas 1), the static pose, and animation 1 without cubic mode (blas 0 unavailable)."""
    g = rt.Gltf(MORPH_BAR)
    plain = g.bake_clip(1)
    g.set_cubicspline(True)
    return {0: g.bake_clip(0), 1: g.bake_clip(1), -1: g.bake_clip(-1), "plain": plain}


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("layer_weights") / "many.glb")
    many_targets(path)
    g = rt.Gltf(path)
    return {a: g.bake_clip(a) for a in (0, 1, -1)}


@pytest.fixture(scope="module")
def quads(tmp_path_factory):
    out = {}
    for n in (63, 64, 65):
        path = str(tmp_path_factory.mktemp("layer_weights_quad") / ("quad%d.glb" % n))
        one_morphed_quad(path, n)
        g = rt.Gltf(path)
        out[n] = {0: g.bake_clip(0), -1: g.bake_clip(-1)}
    return out


def refused(call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def mesh_node(clip, blas):
    """The clip node of the blas's morph set."""
    return int(np.flatnonzero(clip.layout()[0]["gltf_node"] == clip.morph(blas)["gltf_node"])[0])


def mask_of(clip, blas, value, elsewhere=1.0):
    m = np.full(clip.info.n_nodes, elsewhere, F32)
    m[mesh_node(clip, blas)] = value
    return m


def sampled(stack, blas):
    """A stack of (clip, time, weight, mode, mask, reference time) -> (cur, rules with mask values, ref) as the rule takes them."""
    cur = [c.weights_host(t, blas) for c, t, _, _, _, _ in stack]
    refs = [c.weights_host(rt_, blas) if mode == "additive" else None for c, _, _, mode, _, rt_ in stack]
    rules = [(w, mode, None if m is None else float(m[mesh_node(c, blas)])) for c, _, w, mode, m, _ in stack]
    return cur, rules, refs


def check_stack(stack, blas, what):
    """The two host functions against the restatement, bit for bit, and every layer step against exact arithmetic -> steps checked."""
    cur, rules, refs = sampled(stack, blas)
    coded = [(w, ref.ADDITIVE if mode == "additive" else ref.OVERRIDE, m) for w, mode, m in rules]
    want = ref.layer_weights(cur, coded, refs)
    assert np.array_equal(bits(rt.clip_layer_weights_host(cur, rules, refs)), bits(want)), what
    assert np.array_equal(bits(rt.clip_weights_layers_host(stack, blas)), bits(want)), what
    steps = ref.steps(cur, coded, refs)
    for acc, c, x, w, _, got in steps:
        assert abs(ref.Fraction(float(got)) - ref.step_exact(acc, c, x, w)) <= ref.step_bound(acc, c, x, w, got), (what, acc, c, x, w, got)
    return len(steps)


def stacks_of(clips, blas, times, others):
    """Stacks of 1 to 8 layers over `clips[0]` at each of `times`: the layers above the base cycle through `others` (clip keys),
    both modes, WEIGHTS and the masks 0 / 0.5 / 1 / none on the mesh node."""
    base = clips[0]
    for k, t in enumerate(times):
        layers = [(base, t, 1.0, "override", None, 0.0)]
        for l in range(1, 1 + k % 8):
            c = clips[others[(k + l) % len(others)]]
            mode = "additive" if (k + l) % 2 else "override"
            mask = [None, mask_of(c, blas, 0.5, 0.0), mask_of(c, blas, 1.0, 0.0), mask_of(c, blas, 0.0)][(k + 2 * l) % 4]
            layers.append((c, times[(3 * k + 5 * l) % len(times)], WEIGHTS[(k + l) % 5], mode, mask, times[(k + 7 * l) % len(times)]))
        yield layers


def test_the_rule_equals_the_restatement_and_exact_arithmetic_on_the_fixture(bar):
    n = 0
    for blas in (0, 1):
        times = sorted(set(set_times(bar[0], blas)) | set(set_times(bar[1], blas)))
        for k, stack in enumerate(stacks_of(bar, blas, times, [1, 0, -1])):
            n += check_stack(stack, blas, ("bar", blas, k))
    assert n > 300


def test_the_rule_on_the_generated_files(many, quads):
    n = 0
    for blas in (BIG, ONE, TWO):                               # LINEAR against STEP, 130, 1 and 2 targets, zeros and -0 at chunk ends
        times = sorted(set(set_times(many[0], blas)) | set(set_times(many[1], blas)))
        for k, stack in enumerate(stacks_of(many, blas, times, [1, -1, 0])):
            n += check_stack(stack, blas, ("many", blas, k))
    for nt, clips in quads.items():
        times = set_times(clips[0], 0)
        for k, stack in enumerate(stacks_of(clips, 0, times, [0, -1])):
            n += check_stack(stack, 0, ("quad", nt, k))
    assert n > 5000


def test_zeros_survive_at_the_chunk_ends(many):
    """At key 1 of the big set (t = 0.5) the weights at targets 0, 63, 64, 127, 128, 129 are 0 and target 5 is -0: an additive layer
    at its reference time and an override layer at weight 0 on top keep them so."""
    c = many[0]
    stack = [(c, 0.5, 1.0, "override", None, 0.0), (many[1], 1.0, 0.5, "additive", None, 1.0), (many[1], 2.0, 0.0, "override", None, 0.0)]
    got = rt.clip_weights_layers_host(stack, BIG)
    assert np.array_equal(bits(got), bits(c.weights_host(0.5, BIG)))
    assert [k for k in range(130) if got[k] == 0] == [0, 5, 63, 64, 127, 128, 129] and np.signbit(got[5])


def test_identities(bar, many):
    for clips, blases in ((bar, (0, 1)), (many, (BIG, ONE, TWO))):
        for blas in blases:
            times = set_times(clips[0], blas)
            for k, t in enumerate(times):
                base = (clips[0], t, 1.0, "override", None, 0.0)
                one = clips[0].weights_host(t, blas)
                assert np.array_equal(bits(rt.clip_weights_layers_host([base], blas)), bits(one))
                other, to = clips[1], times[(3 * k + 1) % len(times)]
                for w in WEIGHTS:
                    got = rt.clip_weights_layers_host([base, (other, to, w, "override", None, 0.0)], blas)
                    assert np.array_equal(bits(got), bits(clips[0].blend_weights_host(t, other, to, w, blas))), (blas, t, w)
                    # an additive layer at its reference time is the identity at every weight
                    assert np.array_equal(bits(rt.clip_weights_layers_host([base, (other, to, w, "additive", None, to)], blas)), bits(one))
                    # a mask of 0 on the mesh node is no layer, in either mode
                    zero = mask_of(other, blas, 0.0)
                    for mode in ("override", "additive"):
                        assert np.array_equal(bits(rt.clip_weights_layers_host([base, (other, to, w, mode, zero, 0.0)], blas)), bits(one))
                # an override layer at weight 1 is that layer's cur
                assert np.array_equal(bits(rt.clip_weights_layers_host([base, (other, to, 1.0, "override", None, 0.0)], blas)), bits(other.weights_host(to, blas)))
                # a mask value elsewhere than on the mesh node does not matter
                elsewhere = mask_of(other, blas, 1.0, 0.0)
                assert np.array_equal(bits(rt.clip_weights_layers_host([base, (other, to, 0.5, "additive", elsewhere, 0.0)], blas)),
                                      bits(rt.clip_weights_layers_host([base, (other, to, 0.5, "additive", None, 0.0)], blas)))


def test_the_rule_function_refuses(bar):
    w = np.array([0.5, 0.25, 0.0], F32)
    L = "sr_clip_layer_weights_host: layer "
    ok = [(1.0, "override", None), (0.5, "additive", None)]
    assert refused(lambda: rt.clip_layer_weights_host([], [])) == (ERR_INVALID_ARG, "sr_clip_layer_weights_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]")
    assert refused(lambda: rt.clip_layer_weights_host([w] * 9, [ok[0]] * 9))[1] == "sr_clip_layer_weights_host: the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"
    for bad in (-0.25, 1.5, float("nan")):
        assert refused(lambda: rt.clip_layer_weights_host([w, w], [ok[0], (bad, "override", None)])) == (ERR_INVALID_ARG, L + "1: the weight is not in [0, 1]")
        assert refused(lambda: rt.clip_layer_weights_host([w, w], [ok[0], (0.5, "override", bad)])) == (ERR_INVALID_ARG, L + "1: the mask value is not in [0, 1]")
    assert refused(lambda: rt.clip_layer_weights_host([w, w], [ok[0], (0.5, 2, None)])) == (ERR_INVALID_ARG, L + "1: unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)")
    assert refused(lambda: rt.clip_layer_weights_host([w, w], ok)) == (ERR_INVALID_ARG, L + "1: null argument (the sampled weights)")
    assert refused(lambda: rt.clip_layer_weights_host([w, w], ok, [None, None])) == (ERR_INVALID_ARG, L + "1: null argument (the sampled weights)")
    B = L + "0: the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1"
    for base in ((0.5, "override", None), (1.0, "additive", None), (1.0, "override", 0.5)):
        assert refused(lambda: rt.clip_layer_weights_host([w], [base], [w])) == (ERR_INVALID_ARG, B)
    assert np.array_equal(rt.clip_layer_weights_host([w], [(1.0, "override", 1.0)]), w)       # a mask value of 1 is no mask


def test_sets_of_unequal_targets_are_refused(quads):
    """The one-quad files differ in their morph targets alone, so their clips are compatible; their sets do not stack."""
    a, b = quads[63][0], quads[64][0]
    assert a.blend_compatible(b)
    stack = [(a, 0.25, 1.0, "override", None, 0.0), (b, 0.5, 0.0, "override", None, 0.0)]
    assert refused(lambda: rt.clip_weights_layers_host(stack, 0)) == \
        (ERR_INVALID_ARG, "sr_clip_weights_layers_host: layer 1: the set has 64 targets, the base layer's 63")


def test_the_stack_function_refuses(bar, many):
    W = "sr_clip_weights_layers_host: "
    base = (bar[0], 0.5, 1.0, "override", None, 0.0)
    over = lambda c, **kw: [base, tuple({**dict(zip("ctwmkr", (c, 0.25, 0.5, "additive", None, 0.0))), **kw}[x] for x in "ctwmkr")]   # noqa: E731
    assert refused(lambda: rt.clip_weights_layers_host([base] * 9, 0, 3))[1] == W + "the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1], w=1.5), 0)) == (ERR_INVALID_ARG, W + "layer 1: the weight is not in [0, 1]")
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1], m=3), 0)) == (ERR_INVALID_ARG, W + "layer 1: unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)")
    assert refused(lambda: rt.clip_weights_layers_host([(bar[0], 0.5, 0.5, "override", None, 0.0)], 0)) == \
        (ERR_INVALID_ARG, W + "layer 0: the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1")
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1], t=float("inf")), 0)) == (ERR_INVALID_ARG, W + "layer 1: gltf: the time of a pose must be finite")
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1], r=float("nan")), 0)) == (ERR_INVALID_ARG, W + "layer 1: gltf: the time of a pose must be finite")
    bad_mask = mask_of(bar[1], 0, 1.0)
    bad_mask[0] = 1.5
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1], k=bad_mask), 0)) == (ERR_INVALID_ARG, W + "layer 1: the mask has a value that is not in [0, 1]")
    # sr_clip_weights_host's statuses and words: a missing set, an unavailable one, a wrong n_targets
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1]), 2, 3)) == \
        (ERR_INVALID_ARG, W + "layer 0: the clip has no morph set for this blas (it has no morph targets)")
    assert refused(lambda: bar["plain"].weights_host(0.25, 0)) == (ERR_UNSUPPORTED, "sr_clip_weights_host: " + CUBIC)
    assert refused(lambda: rt.clip_weights_layers_host(over(bar["plain"]), 0)) == (ERR_UNSUPPORTED, W + "layer 1: " + CUBIC)
    assert refused(lambda: rt.clip_weights_layers_host(over(bar["plain"], w=0.0), 0)) == (ERR_UNSUPPORTED, W + "layer 1: " + CUBIC)      # checked at weight 0 too
    assert refused(lambda: rt.clip_weights_layers_host(over(bar[1]), 0, 2)) == \
        (ERR_INVALID_ARG, W + "layer 0: gltf: another number of weights asked for than the blas has morph targets")
    # a layer from another file
    code, text = refused(lambda: rt.clip_weights_layers_host(over(many[0]), 0))
    assert code == ERR_INVALID_ARG and text.startswith("sr_clip_blend_compatible: the clips differ in ")
