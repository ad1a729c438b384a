"""Ids, row layouts and input sets of the helper probe (sr_probe_helper / orc_probe_helper).

One row = one call of one inline helper of sunray_amd/csrc/rt_device.h / traverse.h (or of its twin in oracle/orc_math.h,
orc_utils.h, orc_scene.h): the arguments as dwords (floats by their bits), the results as dwords. input_set(name) builds the
deterministic rows both sides are run on; test_gpu_helper_probe.py compares the two sides on every row, and
test_helper_probe_host.py checks that the sets hold what they claim and compares the oracle's side with independent float64
definitions on the same rows."""
import functools
import os
import sys

import numpy as np

from sunray_amd import abi

sys.path.insert(0, os.path.dirname(__file__))
import brdf_models as bm  # noqa: E402
import post_util  # noqa: E402

IDS = {name: i for i, name in enumerate(abi.PROBE_HELPERS)}

# name -> (input dwords, output dwords, output dwords that are integer-coded: pack results, half bits, seeds, flags, M, indices)
LAYOUT = {
    "sincos": (1, 2, ()), "exp": (1, 1, ()), "log": (1, 1, ()), "pow": (2, 1, ()), "pow5": (1, 1, ()), "smoothstep": (3, 1, ()),
    "f32_to_f16": (1, 1, (0,)), "f16_to_f32": (1, 1, ()), "pack_half_2x16": (2, 1, (0,)), "unpack_half_2x16": (1, 2, ()),
    "pack_snorm_2x16": (2, 1, (0,)), "unpack_snorm_2x16": (1, 2, ()), "pack_unorm_4x8": (4, 1, (0,)), "unpack_unorm_rgb": (1, 3, ()),
    "pack_normal": (3, 1, (0,)), "unpack_normal": (1, 3, ()), "pack_rgba8_snorm": (4, 1, (0,)), "unsnorm8": (1, 1, ()),
    "pack_b10g11r11": (3, 1, (0,)), "unpack_b10g11r11": (1, 3, ()),
    "pcg_hash": (1, 1, (0,)), "init_rng": (4, 1, (0,)), "rnd": (1, 2, (0,)),
    "norm3": (3, 3, ()), "reflect3": (6, 3, ()), "refract3": (7, 3, ()), "build_onb": (3, 6, ()), "smith_v_ggx": (3, 1, ()),
    "smith_g1_ggx": (2, 1, ()), "random_bounce": (5, 3, ()), "sample_ggx_vndf": (9, 3, ()),
    "eval_light": (23, 3, ()), "gi_target_pdf": (16, 1, ()),
    "merge": (26, 13, (7, 8, 10, 12)), "merge_gi": (27, 13, (7, 8, 10, 12)),      # M, light_idx / sample_normal_packed, hit_normal_packed, taken
    "transform_point": (15, 3, ()), "intersect_tri": (17, 4, (0,)),
}
assert set(LAYOUT) == set(IDS)
# input dwords that are not floats (codes, seeds, indices): they take no float classes
INT_INPUTS = {"f16_to_f32": (0,), "unpack_half_2x16": (0,), "unpack_snorm_2x16": (0,), "unpack_unorm_rgb": (0,), "unpack_normal": (0,),
              "unsnorm8": (0,), "unpack_b10g11r11": (0,), "pcg_hash": (0,), "init_rng": (0, 1, 2, 3), "rnd": (0,),
              "merge": (8, 10, 20, 22), "merge_gi": (8, 10, 20, 22)}

F32 = np.float32
SIGN = np.uint32(0x80000000)
GAMMA = F32(1.0) / F32(2.2)          # the tonemap's exponent (post.hip)
EXP_HI, EXP_LO = F32(88.72283935546875), F32(-103.9720840454)   # exp_pinned's cut-offs
TWO_OVER_PI = F32(0.63661977236758134)


# ---- bits and neighbours ----------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).ravel()


def flt(u):
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint32)).view(np.float32)


def f64(u):
    """The float64 values of fp32 bits (a signalling NaN converts without a warning)."""
    with np.errstate(invalid="ignore"):
        return flt(u).astype(np.float64)


def is_nan_bits(u):
    return (np.asarray(u, dtype=np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def _key(u):
    u = np.asarray(u, dtype=np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)


def _unkey(k):
    k = np.clip(k, -0x7F800000, 0x7F800000)
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32)


def around(x, k=1):
    """Bits of every fp32 value of `x` and of its k neighbours on each side, in the order of the reals (clipped at +-inf)."""
    key = _key(bits(x))
    return _unkey((key[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).ravel())


def both_signs(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.concatenate([u, u | SIGN])


@functools.lru_cache(None)
def class_set():
    """+-0, smallest and largest denormal, FLT_MIN, 1, FLT_MAX, inf; quiet and signalling NaNs with five payloads, both signs."""
    finite = [0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000]
    nans = [q | p for q in (0x7FC00000, 0x7F800000) for p in (1, 0x1000, 0x1FFF, 0x2000, 0x3FFFFF)]
    return both_signs(np.array(finite + nans, dtype=np.uint32))


@functools.lru_cache(None)
def stratified():
    """Every sign x every exponent x the mantissas {0, 1, 0x7fffff} u {2^k} u {0x7fffff - 2^k}."""
    m = {0, 1, 0x7FFFFF} | {1 << k for k in range(23)} | {0x7FFFFF - (1 << k) for k in range(23)}
    m = np.array(sorted(m), dtype=np.uint32)
    e = np.arange(256, dtype=np.uint32) << np.uint32(23)
    return both_signs((e[:, None] | m[None, :]).ravel())


def rows_of(*cols):
    """Columns (arrays or scalars of uint32 bits) -> rows; scalars and length-1 columns are repeated."""
    cols = [np.atleast_1d(np.asarray(c, dtype=np.uint32)) for c in cols]
    n = max(len(c) for c in cols)
    return np.stack([np.broadcast_to(c, (n,)) if len(c) == 1 else c for c in cols], axis=1).astype(np.uint32)


def frows(a):
    """float rows (n, w) -> uint32 rows."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return a.view(np.uint32).reshape(a.shape)


def sweep(base, cols, values=None):
    """For each base row and each column of `cols`: that column through `values` (the class set), the rest as in the base row."""
    values = class_set() if values is None else np.asarray(values, dtype=np.uint32)
    base = np.atleast_2d(np.asarray(base, dtype=np.uint32))
    out = []
    for c in cols:
        r = np.repeat(base, len(values), axis=0)
        r[:, c] = np.tile(values, len(base))
        out.append(r)
    return np.concatenate(out)


def cross(*lists):
    """Cartesian product of lists of row fragments (each (k_i, w_i)) -> rows (prod k_i, sum w_i)."""
    lists = [np.atleast_2d(np.asarray(x, dtype=np.uint32)) for x in lists]
    idx = np.indices([len(x) for x in lists]).reshape(len(lists), -1)
    return np.concatenate([x[i] for x, i in zip(lists, idx)], axis=1)


def float_cols(name):
    return [c for c in range(LAYOUT[name][0]) if c not in INT_INPUTS.get(name, ())]


# ---- tie sets of the float-to-code conversions -----------------------------------------------------------------------------
def _ties(values, last_successor):
    """values: ascending non-negative code values (float64, exact in fp32). Each value, the midpoint to its successor, and the
    fp32 neighbours of both."""
    v = np.asarray(values, dtype=np.float64)
    nxt = np.concatenate([v[1:], [last_successor]])
    mid = (v + nxt) / 2
    assert (mid.astype(np.float32).astype(np.float64) == mid).all() and (v.astype(np.float32).astype(np.float64) == v).all()
    return np.concatenate([around(v, 1), around(mid, 1)])


@functools.lru_cache(None)
def half_values():
    """fp32 images of all 65 536 halves."""
    return bits(np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32))


@functools.lru_cache(None)
def half_ties():
    """Every half (NaN codes included), and for every finite one: the midpoint to the next half (65520 after 65504, where the
    successor is the 2^16 that rounds to inf) and the fp32 neighbours of both; both signs."""
    v = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    return np.concatenate([both_signs(_ties(v, 65536.0)), half_values()])


@functools.lru_cache(None)
def ufloat_ties(mant):
    """Every finite code of the unsigned small float with `mant` mantissa bits, the midpoint to its successor (2^16 after the
    largest finite) and the fp32 neighbours of both."""
    return _ties(post_util.ufloat_decode(np.arange(31 << mant), mant), 65536.0)


@functools.lru_cache(None)
def norm_ties(scale, signed):
    """Conversions that round x * scale: the fp32 nearest to every code's value c / scale and to every tie (c + 0.5) / scale
    (neither is exact in fp32 in general) with two neighbours on each side, so both sides of every tie are present; plus the
    clamp edges."""
    c = np.arange(-scale if signed else 0, scale + 1, dtype=np.float64)
    v = np.concatenate([around((c / scale).astype(np.float32), 2), around(((c + 0.5) / scale).astype(np.float32), 2)])
    return np.concatenate([v, around(F32([-1.0, 1.0, 0.0]), 2), bits(F32([-2.0, 2.0, -1e30, 1e30, 0.5, -0.5]))])


def spread(u, k):
    """One set in k columns, each column a different rotation of it: every column sees every value."""
    u = np.asarray(u, dtype=np.uint32)
    return np.stack([np.roll(u, (i * len(u)) // k + i) for i in range(k)], axis=1)


# ---- the RNG's output word, inverted -----------------------------------------------------------------------------------------
def rnd_word(seed):
    """(new seed, output word) of rnd() for one seed, in Python integers."""
    s = (seed * 747796405 + 2891336453) & 0xFFFFFFFF
    w = (((s >> ((s >> 28) + 4)) ^ s) * 277803737) & 0xFFFFFFFF
    return s, ((w >> 22) ^ w) & 0xFFFFFFFF


def seed_for_word(word):
    """The seed whose next rnd() draws `word`: every step of the generator is a bijection of the 32-bit words."""
    w = word ^ (word >> 22)                                   # undo x ^= x >> 22 (22 >= 16: one step)
    w = (w * pow(277803737, -1, 1 << 32)) & 0xFFFFFFFF
    sh = (w >> 28) + 4                                        # the top four bits pass through the xorshift
    s = w
    for _ in range(8):                                        # undo x ^= x >> sh, sh >= 4
        s = w ^ (s >> sh)
    return ((s - 2891336453) * pow(747796405, -1, 1 << 32)) & 0xFFFFFFFF


RND_WORDS = tuple([0, 1, (1 << 24) - 1, (1 << 24) + 1] + [(1 << 24) + (1 << k) for k in range(24)] + [0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF])


# ---- edge lists of the vector and BRDF helpers ------------------------------------------------------------------------------------
def _v(*rows):
    return frows(np.array(rows, dtype=np.float32))


EDGE_NORMALS = _v((0, 0, 1), (0, 0, -1), (0, 0, -0.0), (1, 0, -1e-8), (0, 0, 0), (1, 0, 0), (0, -1, 0), (0.6, 0.8, 0), (0.6, 0, -0.8),
                  (-0.48, 0.6, 0.64))
EDGE_VECTORS = np.concatenate([EDGE_NORMALS, _v((np.nan, 0, 0), (0, np.inf, 0), (3e38, 3e38, 3e38), (1e-40, 0, 1e-45), (0, -np.inf, 1))])
SQRT_001 = F32(np.sqrt(F32(0.001)))          # roughness whose square meets sample_ggx_vndf's max(a, 0.001)
EDGE_ROUGHNESS = np.concatenate([bits(F32([0.0, 1e-4, 1.0])), around(SQRT_001, 1)]).reshape(-1, 1)
EDGE_RANDOM = bits(F32([0.0, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -24, 1.0])).reshape(-1, 1)


def _views(normals):
    """For each normal: V equal to it, opposite to it, and grazing (a unit vector perpendicular to it)."""
    n = flt(normals).astype(np.float64)
    helper = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0, 0]], [[0, 1.0, 0]])
    g = np.cross(n, helper)
    g = g / np.maximum(np.linalg.norm(g, axis=1, keepdims=True), 1e-30)
    return np.concatenate([np.concatenate([normals, frows(v)], axis=1) for v in (n, -n, g)])


def _rand_unit(rng, n):
    return bm.unit(rng.normal(size=(n, 3)))


N_RANDOM = 1 << 16


def _reservoir_rows(gi):
    rng = np.random.default_rng(31 + gi)
    n = N_RANDOM
    w = 27 if gi else 26

    def rec(w_sum, M, W, tag):
        r = np.zeros((len(w_sum), 12), dtype=np.uint32)
        r[:, 0:3] = frows(rng.normal(size=(len(w_sum), 3))); r[:, 3] = bits(w_sum)
        r[:, 4:7] = frows(rng.normal(size=(len(w_sum), 3))); r[:, 7] = bits(M)
        r[:, 8] = tag; r[:, 9] = bits(W); r[:, 10] = rng.integers(0, 1 << 32, len(w_sum), dtype=np.uint32); r[:, 11] = bits(rng.uniform(0, 50, len(w_sum)))
        return r
    rows = np.zeros((n, w), dtype=np.uint32)
    rows[:, 0:12] = rec(rng.uniform(0, 4, n), rng.integers(0, 12, n).astype(np.float64), rng.uniform(0, 3, n), 5)
    rows[:, 12:24] = rec(rng.uniform(0, 4, n), rng.integers(1, 10, n).astype(np.float64), rng.uniform(0, 3, n), 77)
    rows[:, 24] = bits(rng.uniform(0, 2, n))
    if gi:
        rows[:, 25] = bits(rng.uniform(0, 10, n))
    rows[:, w - 1] = bits(rng.random(n))
    # edges: w_sum 0 and around the 0.0001 clamp, W 0 / 1 / inf, M 0 / 1 / 2^24 / huge, p_hat 0 / at the clamp / 1, random 0 / 0.5 / 1.0
    w_sums = np.concatenate([bits(F32([0.0, 1.0])), around(F32(1e-4), 1)])
    e = cross(w_sums.reshape(-1, 1), bits(F32([0.0, 1.0, 16777216.0, 1e30])).reshape(-1, 1),          # r.w_sum, r.M
              bits(F32([0.0, 1.0, np.inf])).reshape(-1, 1), bits(F32([0.0, 1.0, 1e30])).reshape(-1, 1),  # new.W, new.M
              bits(F32([0.0, 1e-4, 1.0])).reshape(-1, 1), bits(F32([0.0, 0.5, 1.0])).reshape(-1, 1))     # p_hat, random
    edge = np.repeat(rows[:1], len(e), axis=0)
    edge[:, 3], edge[:, 7], edge[:, 21], edge[:, 19], edge[:, 24], edge[:, w - 1] = e[:, 0], e[:, 1], e[:, 2], e[:, 3], e[:, 4], e[:, 5]
    if gi:
        edge2 = edge.copy(); edge2[:, 25] = bits(F32(0.0)); edge3 = edge.copy(); edge3[:, 25] = bits(F32(np.inf))
        edge = np.concatenate([edge, edge2, edge3])
    return np.concatenate([rows, edge, sweep(rows[:3], float_cols("merge_gi" if gi else "merge"))])


def tri_math64(rows):
    """Moeller-Trumbore in float64 on intersect_tri rows: (det, u, v, t, tmin, tmax)."""
    r = f64(rows)
    o, d, v0, e1, e2 = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12:15]
    with np.errstate(all="ignore"):
        p = np.cross(d, e2); det = (e1 * p).sum(1); inv = 1.0 / det
        tv = o - v0; u = (tv * p).sum(1) * inv
        q = np.cross(tv, e1); v = (d * q).sum(1) * inv; t = (e2 * q).sum(1) * inv
    return det, u, v, t, r[:, 15], r[:, 16]


def _tri_rows():
    rng = np.random.default_rng(41)
    n = N_RANDOM

    def aimed(v0, e1, e2, o, u, v, tmin=1e-3, tmax=1e4):
        target = v0 + u[:, None] * e1 + v[:, None] * e2
        return frows(np.concatenate([o, target - o, v0, e1, e2, np.full((len(o), 1), tmin), np.full((len(o), 1), tmax)], axis=1))
    v0 = rng.uniform(-2, 2, (n, 3)); e1 = rng.normal(size=(n, 3)); e2 = rng.normal(size=(n, 3)); o = rng.uniform(-4, 4, (n, 3))
    out = [aimed(v0, e1, e2, o, rng.uniform(-0.5, 1.5, n), rng.uniform(-0.5, 1.5, n))]
    # vertices, edge points, and points +-1e-6 * k outside / inside each edge, on 512 triangles each
    m = 512
    s = rng.uniform(0.05, 0.95, m)
    targets = [(np.zeros(m), np.zeros(m)), (np.ones(m), np.zeros(m)), (np.zeros(m), np.ones(m)), (s, np.zeros(m)), (np.zeros(m), s), (s, 1 - s)]
    for k in (0.5, 1.0, 2.0):
        for sg in (-1.0, 1.0):
            dlt = np.full(m, sg * 1e-6 * k)
            targets += [(dlt, s), (s, dlt), (s + dlt / 2, 1 - s + dlt / 2)]
    for u, v in targets:
        out.append(aimed(v0[:m], e1[:m], e2[:m], o[:m], u, v))
    # the same in a frame whose arithmetic is exact: the unit right triangle of z = 0, a ray straight down from z = 1 (t = 1)
    unit_tri = [0, 0, 0, 1, 0, 0, 0, 1, 0]
    for u, v in [(0.25, 0.25), (0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.5, 0), (0, 0.5)] + [(sg * 1e-6 * k, 0.5) for k in (0.5, 1, 2) for sg in (-1, 1)] \
            + [(0.5, sg * 1e-6 * k) for k in (0.5, 1, 2) for sg in (-1, 1)] + [(0.5 + sg * 1e-6 * k, 0.5) for k in (0.5, 1, 2) for sg in (-1, 1)]:
        for tmin, tmax in [(1e-3, 1e4)] + [(a, 1e4) for a in flt(around(F32(1.0), 1))] + [(1e-3, b) for b in flt(around(F32(1.0), 1))]:
            out.append(frows(np.array([[u, v, 1, 0, 0, -1] + unit_tri + [tmin, tmax]])))
    # det = 0: a ray in the triangle's plane, degenerate triangles (parallel edges, a zero edge); denormal edges
    flat = [[0.25, 0.25, 0, 1, 0, 0] + unit_tri + [1e-3, 1e4], [-1, 0.25, 0, 1, 0, 0] + unit_tri + [1e-3, 1e4],
            [0.25, 0.25, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, 2, 0, 0, 1e-3, 1e4], [0.25, 0.25, 1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1e-3, 1e4],
            [0, 0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1e-3, 1e4],
            [0, 0, 1, 0, 0, -1, 0, 0, 0, 1e-40, 0, 0, 0, 1e-40, 0, 1e-3, 1e4], [1e-41, 1e-41, 1, 0, 0, -1, 0, 0, 0, 1e-40, 0, 0, 0, 1e-40, 0, 1e-3, 1e4],
            [0, 0, 1e-30, 0, 0, -1e-30, 0, 0, 0, 1.4e-45, 0, 0, 0, 1.4e-45, 0, 0, 1e4], [0, 0, 1, 0, 0, -1, 0, 0, 0, 1e-20, 0, 0, 0, 1e-20, 0, 1e-3, 1e4]]
    out.append(frows(np.array(flat)))
    base = np.concatenate([out[0][:3], out[-1][:1]])
    out.append(sweep(base, range(17)))                       # non-finite (and every other class of) origin, direction, vertex, edge, range
    return np.concatenate(out)


# ---- the input set of each helper ---------------------------------------------------------------------------------------------------
def _scalar(extra=()):
    return np.concatenate([class_set(), stratified()] + list(extra)).reshape(-1, 1)


def _sincos_rows():
    x = np.concatenate([
        bits(np.linspace(0.0, 2.0 * np.pi * 1.0001, 1 << 20)),
        both_signs(around((np.arange(1, 257) * (np.pi / 4)).astype(np.float32), 2)),
        both_signs(around(F32(2.0 ** 31) / TWO_OVER_PI, 8)),                       # the end of the domain (the filter keeps its inside)
        class_set(), stratified()])
    f = flt(x)
    with np.errstate(all="ignore"):
        inside = np.abs(f * TWO_OVER_PI) < F32(2.0 ** 31)       # the stated domain; inf and NaN stay (NaN out on both sides)
    return x[inside | ~np.isfinite(f)].reshape(-1, 1)


def _exp_rows():
    k = np.arange(-152, 131, dtype=np.float64) + 0.5
    return _scalar([np.arange(0xC2AE0000, 0xC2D00001, dtype=np.uint32),                 # every float of [-104, -87]
                    around(F32([EXP_HI, EXP_LO]), 3), around((k / 1.4426950408889634).astype(np.float32), 2)])


def _log_rows():
    e = np.arange(-149, 129)
    return _scalar([around(np.ldexp(1.0, np.arange(-149, -125)).astype(np.float32), 2),            # every denormal exponent step
                    around(np.ldexp(0.70710678, e[e > -148]).astype(np.float32), 2), around(F32(1.0), 8)])


def _pow_rows():
    x = np.arange(0, 0x3F800001, 64, dtype=np.uint32)
    extra = bits(F32([0.5, 2.0, GAMMA, 2.2, -2.0, 3.0, 10.0, 1e-3, 0.99999994, 1.0000001, 1e10, 1e-10, -0.5, 88.0, -88.0, 104.0, -104.0,
                      1e38, 1e-38, 1e-42, 0.18, 255.0, -1e-3, 5.0, 0.25, 4.0, -4.0, 127.0, -126.0, 1.5]))
    c = np.concatenate([class_set(), extra])
    assert len(c) == 64
    return np.concatenate([rows_of(x, bits(GAMMA)), rows_of(class_set(), bits(GAMMA)), cross(c.reshape(-1, 1), c.reshape(-1, 1))])


def _smoothstep_rows():
    rng = np.random.default_rng(21)
    e = np.concatenate([bits(F32([0.0, -0.0, 0.9, 0.99, 1.0, 0.5, 0.945, 1e-45, np.inf, -np.inf, np.nan, 2.0])), around(F32(0.9), 1), around(F32(0.99), 1)])
    e = e.reshape(-1, 1)
    return np.concatenate([frows(rng.uniform(-0.5, 1.5, (N_RANDOM, 3))), rows_of(bits(F32(0.9)), bits(F32(0.99)), bits(rng.uniform(0.85, 1.05, N_RANDOM))),
                           cross(e, e, e), sweep(frows([[0.9, 0.99, 0.95], [0.0, 1.0, 0.5]]), range(3))])


def _vec_rows(name, rng_seed, gen, edges):
    rng = np.random.default_rng(rng_seed)
    rnd = frows(gen(rng, N_RANDOM))
    return np.concatenate([rnd, edges, sweep(rnd[:4], float_cols(name))])


def _light_edges():
    """Edge normals x V {equal, opposite, grazing} x roughness x metallic {0, 1} x light {at the hit point, behind the surface,
    facing away, 1e-5 and 1e5 away}."""
    hit = np.array([0.25, -0.5, 1.0])
    out = []
    nv = _views(EDGE_NORMALS)
    for nrow in nv:
        n = flt(nrow[0:3]).astype(np.float64)
        up = n if np.linalg.norm(n) > 0 else np.array([0, 0, 1.0])
        lights = [(hit, -up), (hit - up, up), (hit + up, up), (hit + up, -up), (hit + 1e-5 * up, -up), (hit + 1e5 * up, -up)]
        for lp, ln in lights:
            for rough in EDGE_ROUGHNESS[:, 0]:
                for metal in (0.0, 1.0):
                    row = np.zeros(23, dtype=np.uint32)
                    row[0:3] = bits(hit); row[3:9] = nrow; row[9:12] = bits(F32([0.8, 0.5, 0.2])); row[12] = rough; row[13] = bits(F32(metal))[0]
                    row[14:17] = bits(F32([10.0, 8.0, 6.0])); row[17:20] = bits(lp); row[20:23] = bits(ln)
                    out.append(row)
    return np.array(out, dtype=np.uint32)


def _gi_edges():
    hit = np.array([0.25, -0.5, 1.0])
    out = []
    for nrow in EDGE_NORMALS:
        n = flt(nrow).astype(np.float64)
        up = n if np.linalg.norm(n) > 0 else np.array([0, 0, 1.0])
        for sp in (hit, hit - up, hit + up, hit + 1e-5 * up, hit + 1e5 * up, hit + 1e-4 * up):
            for metal in (0.0, 1.0):
                out.append(np.concatenate([bits(hit), nrow, bits(F32([0.8, 0.5, 0.2])), bits(F32(metal)), bits(sp), bits(F32([1.0, 2.0, 0.5]))]))
    return np.array(out, dtype=np.uint32)


def _refract_edges():
    # k = 1 - eta^2 (1 - ni^2): with i grazing (ni = 0), eta = 1 gives k = 0 exactly and its neighbours either side of it
    etas = np.concatenate([around(F32(1.0), 2), bits(F32([1.5, 1.0 / 1.5, 0.0, 2.0, -1.0]))]).reshape(-1, 1)
    return cross(EDGE_VECTORS, EDGE_VECTORS, etas)


_BUILDERS = {
    "sincos": _sincos_rows, "exp": _exp_rows, "log": _log_rows, "pow": _pow_rows, "pow5": _scalar, "smoothstep": _smoothstep_rows,
    "f32_to_f16": lambda: _scalar([half_ties()]),
    "f16_to_f32": lambda: np.concatenate([np.arange(65536, dtype=np.uint32), np.arange(0, 65536, 4099, dtype=np.uint32) | np.uint32(0xABCD0000)]).reshape(-1, 1),
    "pack_half_2x16": lambda: np.concatenate([spread(np.concatenate([half_ties(), class_set()]), 2), cross(class_set().reshape(-1, 1), class_set().reshape(-1, 1))]),
    "unpack_half_2x16": lambda: (np.arange(65536, dtype=np.uint32) | (np.arange(65536, dtype=np.uint32)[::-1] << np.uint32(16))).reshape(-1, 1),
    "pack_snorm_2x16": lambda: np.concatenate([spread(np.concatenate([norm_ties(32767, True), class_set()]), 2),
                                               cross(class_set().reshape(-1, 1), class_set().reshape(-1, 1))]),
    "unpack_snorm_2x16": lambda: (np.arange(65536, dtype=np.uint32) | (np.arange(65536, dtype=np.uint32)[::-1] << np.uint32(16))).reshape(-1, 1),
    "pack_unorm_4x8": lambda: spread(np.concatenate([norm_ties(255, False), class_set(), stratified()]), 4),
    "unpack_unorm_rgb": lambda: (lambda b: (b | (np.roll(b, 85) << np.uint32(8)) | (np.roll(b, 170) << np.uint32(16)) | (np.roll(b, 31) << np.uint32(24))).reshape(-1, 1))(
        np.arange(256, dtype=np.uint32)),
    "pack_normal": lambda: _vec_rows("pack_normal", 22, lambda rng, n: np.concatenate([_rand_unit(rng, n // 2), rng.normal(size=(n // 2, 3)) * 3]),
                                     np.concatenate([EDGE_VECTORS, cross(*[bits(F32([0, -0.0, 1, -1, 1e-8, -1e-8, 0.5, np.inf, np.nan, 1e-45, 3e38])).reshape(-1, 1)] * 3)])),
    "unpack_normal": lambda: (np.arange(65536, dtype=np.uint32)[None, :]
                              | (np.rint(np.linspace(0, 65535, 257)).astype(np.uint32)[:, None] << np.uint32(16))).reshape(-1, 1),
    "pack_rgba8_snorm": lambda: spread(np.concatenate([norm_ties(127, True), class_set(), stratified()]), 4),
    "unsnorm8": lambda: np.concatenate([np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32) | np.uint32(0x5A5A5A00)]).reshape(-1, 1),
    "pack_b10g11r11": lambda: (lambda s6, s5: np.concatenate([
        np.stack([s6, s6[::-1], np.resize(s5, len(s6))], axis=1), sweep(frows([[0.5, 0.25, 0.125]]), range(3), np.concatenate([class_set(), stratified()]))]))(
        ufloat_ties(6), ufloat_ties(5)),
    "unpack_b10g11r11": lambda: (lambda c: (c | (c[::-1] << np.uint32(11)) | ((c & np.uint32(1023)) ^ (c >> np.uint32(1))) << np.uint32(22)).reshape(-1, 1))(
        np.arange(2048, dtype=np.uint32)),
    "pcg_hash": lambda: np.concatenate([np.arange(1 << 20, dtype=np.uint32), np.uint32(0xFFFFFFFF) - np.arange(1 << 10, dtype=np.uint32),
                                        np.uint32(1) << np.arange(32, dtype=np.uint32), np.random.default_rng(23).integers(0, 1 << 32, N_RANDOM, dtype=np.uint32)]).reshape(-1, 1),
    "init_rng": lambda: (lambda rng, e: np.concatenate([
        rng.integers(0, 1 << 32, (N_RANDOM, 4), dtype=np.uint32), cross(e, e, e, e),
        np.stack([rng.integers(0, 3840, N_RANDOM), rng.integers(0, 2160, N_RANDOM), rng.integers(0, 100000, N_RANDOM), np.full(N_RANDOM, 3840)], axis=1).astype(np.uint32)]))(
        np.random.default_rng(24), np.array([0, 1, 0x80000000, 0xFFFFFFFF], dtype=np.uint32).reshape(-1, 1)),
    "rnd": lambda: np.concatenate([np.array([seed_for_word(w) for w in RND_WORDS], dtype=np.uint32), np.arange(1 << 20, dtype=np.uint32) + np.uint32(0x9E3779B9)]).reshape(-1, 1),
    "norm3": lambda: _vec_rows("norm3", 25, lambda rng, n: rng.normal(size=(n, 3)) * np.exp(rng.uniform(-20, 20, (n, 1))),
                               np.concatenate([EDGE_VECTORS, cross(*[bits(F32([0, -0.0, 1, -1, 1e-20, 1e19, 1e-45, np.inf, np.nan, 3e38])).reshape(-1, 1)] * 3)])),
    "reflect3": lambda: _vec_rows("reflect3", 26, lambda rng, n: np.concatenate([_rand_unit(rng, n), _rand_unit(rng, n)], axis=1), cross(EDGE_VECTORS, EDGE_VECTORS)),
    "refract3": lambda: _vec_rows("refract3", 27, lambda rng, n: np.concatenate([_rand_unit(rng, n), _rand_unit(rng, n), rng.choice([1.0 / 1.5, 1.5, 1.0, 1.33], (n, 1))], axis=1),
                                  _refract_edges()),
    "build_onb": lambda: _vec_rows("build_onb", 28, lambda rng, n: _rand_unit(rng, n),
                                   np.concatenate([EDGE_VECTORS, rows_of(bits(F32(1e-4)), bits(F32(-1e-4)), around(F32(-1.0), 4)),
                                                   rows_of(bits(F32(0.0)), bits(F32(0.0)), around(F32(0.0), 2))])),
    "smith_v_ggx": lambda: (lambda e: np.concatenate([
        frows(np.random.default_rng(29).uniform(0, 1, (N_RANDOM, 3))), cross(e, e, e),
        rows_of(around(F32(0.0070710678), 4), around(F32(0.0070710678), 4), bits(F32(0.0))),          # 2 x^2 at the 0.0001 clamp
        rows_of(around(F32(5e-5), 4), around(F32(5e-5), 4), bits(F32(1.0))),                          # 2 x at the clamp
        sweep(frows([[0.7, 0.4, 0.25], [0.001, 1.0, 1e-4]]), range(3))]))(
        np.concatenate([bits(F32([0.0, -0.0, 1e-4, 1e-3, 0.5, 1.0, 1e-45, np.inf, np.nan, -0.5])), around(SQRT_001, 1)]).reshape(-1, 1)),
    "smith_g1_ggx": lambda: (lambda e: np.concatenate([
        frows(np.random.default_rng(30).uniform(0, 1, (N_RANDOM, 2))), cross(e, e),
        rows_of(around(F32(5e-5), 4), bits(F32(0.0))), rows_of(around(F32(1e-4), 4), bits(F32(1.0)))]))(       # x + |x| and x + 1 * ... at the clamp
        np.concatenate([class_set(), bits(F32([1e-4, 1e-3, 0.5, -0.5, 0.25, 2.0])), around(SQRT_001, 1)]).reshape(-1, 1)),
    "random_bounce": lambda: _vec_rows("random_bounce", 32, lambda rng, n: np.concatenate([_rand_unit(rng, n), rng.random((n, 2))], axis=1),
                                       cross(EDGE_NORMALS, EDGE_RANDOM, EDGE_RANDOM)),
    "sample_ggx_vndf": lambda: _vec_rows("sample_ggx_vndf", 33, lambda rng, n: (lambda N, V, r, u1, u2: np.concatenate([N, V, r[:, None], u1[:, None], u2[:, None]], axis=1))(*bm.vndf_inputs(rng, n)),
                                         cross(_views(EDGE_NORMALS), EDGE_ROUGHNESS, EDGE_RANDOM, EDGE_RANDOM)),
    "eval_light": lambda: _vec_rows("eval_light", 34, lambda rng, n: (lambda P, N, V, al, ro, me, Le, X, Nl: np.concatenate([P, N, V, al, ro[:, None], me[:, None], Le, X, Nl], axis=1))(*bm.light_inputs(rng, n)),
                                    _light_edges()),
    "gi_target_pdf": lambda: _vec_rows("gi_target_pdf", 35, lambda rng, n: (lambda P, N, al, me, X, rad: np.concatenate([P, N, al, me[:, None], X, rad], axis=1))(*bm.gi_inputs(rng, n)),
                                       _gi_edges()),
    "merge": lambda: _reservoir_rows(0), "merge_gi": lambda: _reservoir_rows(1),
    "transform_point": lambda: _vec_rows("transform_point", 36, lambda rng, n: np.concatenate([rng.normal(size=(n, 12)) * 2, rng.uniform(-50, 50, (n, 3))], axis=1),
                                         frows(np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 2, 3], [0] * 15, [1, 0, 0, 1e30, 0, 1, 0, -1e30, 0, 0, 1, 0, 1e30, 1e30, 0],
                                                         [1e-40] * 12 + [1e-5, 1, 1e5], [3e38] * 12 + [2, 2, 2]]))),
    "intersect_tri": _tri_rows,
}
assert set(_BUILDERS) == set(IDS)


@functools.lru_cache(None)
def input_set(name):
    """The rows (uint32, n x input dwords) helper `name` is compared on; built once, read-only."""
    rows = np.ascontiguousarray(_BUILDERS[name](), dtype=np.uint32)
    assert rows.ndim == 2 and rows.shape[1] == LAYOUT[name][0], (name, rows.shape)
    rows.setflags(write=False)
    return rows


def mismatch(name, rows, got, want, got_name="device", want_name="oracle"):
    """None if `got` equals `want` under the probe's rule (integer-coded dwords in every bit; float dwords in every bit unless both
    are NaN), else a message naming the helper, the first differing row, its inputs in hex and both outputs."""
    ints = LAYOUT[name][2]
    diff = got != want
    both_nan = is_nan_bits(got) & is_nan_bits(want)
    for c in range(got.shape[1]):
        if c not in ints:
            diff[:, c] &= ~both_nan[:, c]
    bad = np.flatnonzero(diff.any(axis=1))
    if len(bad) == 0:
        return None
    i = int(bad[0])
    hx = lambda a: " ".join("%08x" % x for x in a)
    return "%s: %d of %d rows differ; first row %d: in [%s] %s [%s] %s [%s]" % (name, len(bad), len(rows), i, hx(rows[i]), got_name, hx(got[i]), want_name, hx(want[i]))
