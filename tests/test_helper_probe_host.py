"""CPU half of the helper probe: the input sets of tests/helper_probe.py hold what they claim, and the oracle's side of the probe
(orc_probe_helper) agrees with independent definitions on those same rows — numpy's float16, the arithmetic codecs of
post_util.py, float64 libm, integer arithmetic in Python, the float64 BRDF models of brdf_models.py. test_gpu_helper_probe.py
shows device == oracle on every row of the same sets; together the two pin the device helpers without a tolerance on the GPU side."""
import os
import re
import sys

import numpy as np
import pytest

from sunray_amd import abi

sys.path.insert(0, os.path.dirname(__file__))
import brdf_models as bm  # noqa: E402
import helper_probe as hp  # noqa: E402
import post_util  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def run(oracle):
    cache = {}

    def go(name):
        if name not in cache:
            rows = hp.input_set(name)
            out = oracle.probe_helper(hp.IDS[name], rows)
            out.setflags(write=False)
            cache[name] = (rows, out)
        return cache[name]
    return go


def has(rows, values):
    """Every one of `values` (uint32 bits) occurs in column 0 of `rows`."""
    return np.isin(np.asarray(values, dtype=np.uint32), rows[:, 0]).all()


def test_ids_and_layouts_agree_with_header_and_oracle(oracle):
    header = open(os.path.join(ROOT, "include", "sunray_hip.h")).read()
    enum = header[header.index("typedef enum SrProbeHelper"):header.index("} SrProbeHelper;")]
    names = re.findall(r"\bSR_PROBE_([A-Z0-9_]+)\b", enum)
    assert names[-1] == "COUNT" and tuple(n.lower() for n in names[:-1]) == abi.PROBE_HELPERS
    for name, fn in hp.IDS.items():
        assert oracle.probe_helper_layout(fn) == hp.LAYOUT[name][:2], name
    assert oracle.probe_helper_layout(len(hp.IDS)) is None
    with pytest.raises(ValueError):
        oracle.probe_helper(len(hp.IDS), np.zeros((1, 1), np.uint32))


def test_input_sets_cover_what_they_claim():
    cls = hp.class_set()
    assert len(cls) == 34 and len(np.unique(cls)) == 34 and hp.is_nan_bits(cls).sum() == 20
    for want in (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00800000, 0xBF800000, 0x7F7FFFFF, 0xFF800000, 0x7F800001, 0xFFC01FFF, 0x7FFFFFFF):
        assert want in cls
    strat = hp.stratified()
    assert len(np.unique(strat >> np.uint32(23))) == 512                      # every sign x exponent
    assert len(np.unique(strat & np.uint32(0x7FFFFF))) == 3 + 23 + 23 - 1      # 2^0 = 1 is counted once
    # every float argument of every helper sees every class (one column at a time at least)
    for name in hp.IDS:
        rows = hp.input_set(name)
        for c in hp.float_cols(name):
            if name == "sincos":
                continue                                                       # its domain excludes +-FLT_MAX, checked below
            assert np.isin(cls, rows[:, c]).all(), (name, c)
    # binary16: every half, and both sides of and exactly on the tie above every finite half
    f16 = hp.input_set("f32_to_f16")
    assert has(f16, hp.half_values())
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)
    mid = ((h + np.concatenate([h[1:], [65536.0]])) / 2).astype(np.float32)
    assert mid[-1] == 65520.0
    for sign in (1.0, -1.0):
        for k in (-1, 0, 1):
            assert has(f16, hp._unkey(hp._key(hp.bits(sign * mid)) + k)) and has(f16, hp._unkey(hp._key(hp.bits(sign * h.astype(np.float32))) + k))
    for col in (0, 1):
        assert np.isin(hp.half_ties(), hp.input_set("pack_half_2x16")[:, col]).all()
    # small floats: every finite code and its tie, in the channel of its width
    b = hp.input_set("pack_b10g11r11")
    for col, mant in ((0, 6), (1, 6), (2, 5)):
        v = post_util.ufloat_decode(np.arange(31 << mant), mant)
        t = (v + np.concatenate([v[1:], [65536.0]])) / 2
        assert np.isin(hp.bits(v.astype(np.float32)), b[:, col]).all() and np.isin(hp.bits(t.astype(np.float32)), b[:, col]).all()
    # unorm8 / snorm8 / snorm16: float64 says some row lies strictly on each side of every tie c + 0.5, in every channel
    for name, scale, lo in (("pack_unorm_4x8", 255, 0), ("pack_rgba8_snorm", 127, -127), ("pack_snorm_2x16", 32767, -32767)):
        rows = hp.input_set(name)
        for c in range(rows.shape[1]):
            x = np.sort(hp.f64(rows[:, c])[~hp.is_nan_bits(rows[:, c])]) * scale
            ties = np.arange(lo, scale) + 0.5
            i = np.searchsorted(x, ties)
            below, above = x[i - 1], x[np.minimum(i, len(x) - 1)]
            tol = scale * 2.0 ** -23                                      # one fp32 step of x below 1, in code units
            assert (ties - below <= tol).all() and (above - ties <= tol).all() and (below < ties).all() and (above >= ties).all(), name
    # code-exhaustive sets
    assert has(hp.input_set("f16_to_f32"), np.arange(65536))
    for name in ("unpack_half_2x16", "unpack_snorm_2x16"):
        p = hp.input_set(name)[:, 0]
        assert len(np.unique(p & np.uint32(0xFFFF))) == 65536 and len(np.unique(p >> np.uint32(16))) == 65536
    p = hp.input_set("unpack_b10g11r11")[:, 0]
    assert len(np.unique(p & np.uint32(0x7FF))) == 2048 and len(np.unique((p >> np.uint32(11)) & np.uint32(0x7FF))) == 2048 and len(np.unique(p >> np.uint32(22))) == 1024
    p = hp.input_set("unpack_unorm_rgb")[:, 0]
    assert all(len(np.unique((p >> np.uint32(s)) & np.uint32(0xFF))) == 256 for s in (0, 8, 16))
    assert len(np.unique(hp.input_set("unsnorm8")[:, 0] & np.uint32(0xFF))) == 256 and 0x80 in hp.input_set("unsnorm8")[:, 0]
    p = hp.input_set("unpack_normal")[:, 0]
    assert len(p) == 65536 * 257 and len(np.unique(p)) == len(p) and len(np.unique(p >> np.uint32(16))) == 257
    # exp: the 2 228 225 consecutive floats of [-104, -87], the cut-offs' neighbours, both sides of every change of rint(x log2 e)
    e = hp.input_set("exp")
    lo, hi = hp.bits(F32(-87.0))[0], hp.bits(F32(-104.0))[0]
    assert hi - lo + 1 == 2228225 and has(e, np.arange(lo, hi + 1, dtype=np.uint32))
    assert has(e, hp.around(F32([hp.EXP_HI, hp.EXP_LO]), 3))
    x = np.sort(hp.flt(e[:, 0])[np.isfinite(hp.flt(e[:, 0]))])
    k = np.rint(x[(x > hp.EXP_LO) & (x < hp.EXP_HI)] * F32(1.44269504088896341))
    steps = np.flatnonzero(np.diff(k) == 1)
    assert k.min() == -150 and k.max() == 128 and len(np.unique(k)) == 279
    xs = x[(x > hp.EXP_LO) & (x < hp.EXP_HI)]
    assert (hp._key(hp.bits(xs[steps + 1])) - hp._key(hp.bits(xs[steps])) == 1).sum() >= 270      # adjacent floats on either side of the change
    # sincos: the dense sweep, the neighbours of every multiple of pi/4 up to 64 pi, nothing outside the stated domain
    s = hp.flt(hp.input_set("sincos")[:, 0])
    assert np.isin(hp.bits(np.linspace(0.0, 2.0 * np.pi * 1.0001, 1 << 20)), hp.input_set("sincos")[:, 0]).all()
    assert has(hp.input_set("sincos"), hp.both_signs(hp.around((np.arange(1, 257) * (np.pi / 4)).astype(np.float32), 2)))
    fin = np.isfinite(s)
    assert (np.abs(s[fin].astype(np.float64)) * (2 / np.pi) < 2.0 ** 31).all() and np.isinf(s).sum() == 4 and np.isnan(s).sum() >= 20
    assert np.abs(s[fin]).max() > 3.3e9                                        # ... and it reaches up to the domain's end
    # log: denormal steps, 0.7071 in every binade, 1 +- ulps; pow: the gamma column and the 64 x 64 cross
    lg = hp.input_set("log")
    assert has(lg, hp.bits(np.ldexp(1.0, np.arange(-149, 128)).astype(np.float32))) and has(lg, hp.around(F32(1.0), 8))
    assert has(lg, hp.bits(np.ldexp(0.70710678, np.arange(-147, 129)).astype(np.float32)))
    pw = hp.input_set("pow")
    g = pw[pw[:, 1] == hp.bits(hp.GAMMA)[0]]
    assert has(g, np.arange(0, 0x3F800001, 64, dtype=np.uint32)) and has(g, cls)
    assert len(np.unique(pw[-4096:], axis=0)) == 4096 and np.isin(cls, pw[-4096:, 0]).all() and np.isin(cls, pw[-4096:, 1]).all()
    # rnd: the seeds really draw the listed words, and 2^20 consecutive seeds follow
    r = hp.input_set("rnd")[:, 0]
    assert [hp.rnd_word(int(sd))[1] for sd in r[:len(hp.RND_WORDS)]] == list(hp.RND_WORDS)
    for w in (0, 1, (1 << 24) - 1, (1 << 24) + 1, (1 << 24) + 2, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF):
        assert w in hp.RND_WORDS
    assert (np.diff(r[len(hp.RND_WORDS):].astype(np.int64)) % (1 << 32) == 1).all() and len(r) == len(hp.RND_WORDS) + (1 << 20)
    # intersect_tri: float64 puts rows on each side of each of the five comparisons, and finds the degenerate ones
    t = hp.input_set("intersect_tri")
    det, u, v, tt, tmin, tmax = hp.tri_math64(t)
    uv = np.where(np.isfinite(u) & np.isfinite(v), u, 0.0) + np.where(np.isfinite(u) & np.isfinite(v), v, np.inf)
    eps = float(F32(1e-6))
    ok = np.isfinite(det) & (det != 0) & np.isfinite(u) & np.isfinite(v) & np.isfinite(tt)
    for cond in (u >= -eps, v >= -eps, uv <= 1.0 + eps, tt > tmin, tt < tmax):
        assert (ok & cond).sum() >= 16 and (ok & ~cond).sum() >= 16
    near = lambda a, b: ok & (np.abs(a - b) < 4e-6) & (np.abs(a - b) > 0)
    assert near(u, -eps).sum() >= 512 and near(v, -eps).sum() >= 512 and near(uv, 1 + eps).sum() >= 512     # within a few 1e-6 of the edge, either side
    assert (ok & (tt == tmin)).any() and (ok & (tt == tmax)).any()              # t on the range's ends exactly (the exact frame)
    assert ((det == 0) & np.isfinite(det)).sum() >= 4 and (~np.isfinite(det)).any()
    edges = np.abs(hp.flt(t[:, 9:15]))
    assert ((edges > 0) & (edges < 1.2e-38)).any()                              # denormal edges
    assert (~np.isfinite(hp.flt(t[:, 0:6]))).any(axis=0).all()                  # non-finite origin and direction, every component


def test_binary16_and_small_floats_against_numpy_and_codecs(run):
    rows, out = run("f32_to_f16")
    nan = hp.is_nan_bits(rows[:, 0])
    with np.errstate(over="ignore"):
        want = hp.flt(rows[:, 0]).astype(np.float16).view(np.uint16).astype(np.uint32)
    assert np.array_equal(out[~nan, 0], want[~nan])
    # a NaN keeps its sign and the top ten payload bits and is quiet: the result of v_cvt_f16_f32
    assert np.array_equal(out[nan, 0], ((rows[nan, 0] >> np.uint32(16)) & np.uint32(0x8000)) | np.uint32(0x7E00) | ((rows[nan, 0] >> np.uint32(13)) & np.uint32(0x3FF)))
    rows, out = run("f16_to_f32")
    want = hp.bits((rows[:, 0] & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float32))
    nan = hp.is_nan_bits(want)
    assert np.array_equal(out[~nan, 0], want[~nan]) and hp.is_nan_bits(out[nan, 0]).all() and nan.sum() >= 2046
    rows, out = run("pack_half_2x16")
    with np.errstate(over="ignore"):
        h = [hp.flt(rows[:, c]).astype(np.float16).view(np.uint16).astype(np.uint32) for c in (0, 1)]
    ok = ~hp.is_nan_bits(rows).any(axis=1)
    assert np.array_equal(out[ok, 0], (h[0] | (h[1] << np.uint32(16)))[ok]) and ok.sum() > 400000
    rows, out = run("unpack_half_2x16")
    for c, code in ((0, rows[:, 0] & np.uint32(0xFFFF)), (1, rows[:, 0] >> np.uint32(16))):
        want = hp.bits(code.astype(np.uint16).view(np.float16).astype(np.float32))
        nan = hp.is_nan_bits(want)
        assert np.array_equal(out[~nan, c], want[~nan]) and hp.is_nan_bits(out[nan, c]).all()
    # B10G11R11 against the arithmetic model (nearest code, ties to even, NaN -> the NaN code, negatives -> 0, overflow -> largest finite)
    rows, out = run("pack_b10g11r11")
    assert np.array_equal(out[:, 0], post_util.b10g11r11_encode(hp.f64(rows)))
    rows, out = run("unpack_b10g11r11")
    want = post_util.b10g11r11_decode(rows[:, 0])
    got = hp.f64(out)
    nan = np.isnan(want)
    assert np.array_equal(got[~nan], want[~nan]) and np.isnan(got[nan]).all() and nan.any()


def _norm_code(x, scale, lo):
    """round-half-even(clamp(x, lo, 1) * scale) with a NaN dropped by the clamp's max (-> lo), in float64 on fp32 products."""
    x = np.where(np.isnan(x), F32(lo), np.clip(x, F32(lo), F32(1.0))).astype(np.float32)
    return np.rint((x * F32(scale)).astype(np.float64)).astype(np.int64)


def test_norm_packs_and_unpacks_against_numpy(run):
    rows, out = run("pack_unorm_4x8")
    c = _norm_code(hp.flt(rows), 255, 0.0)
    assert np.array_equal(out[:, 0], (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32))
    rows, out = run("pack_snorm_2x16")
    c = _norm_code(hp.flt(rows), 32767, -1.0) & 0xFFFF
    assert np.array_equal(out[:, 0], (c[:, 0] | (c[:, 1] << 16)).astype(np.uint32))
    rows, out = run("pack_rgba8_snorm")
    c = np.where(hp.is_nan_bits(rows), 0, _norm_code(hp.flt(rows), 127, -1.0)) & 0xFF             # the image store maps NaN to 0
    assert np.array_equal(out[:, 0], (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32))
    rows, out = run("unsnorm8")
    assert np.array_equal(hp.flt(out[:, 0]), post_util.snorm8_decode(rows[:, 0] & np.uint32(0xFF)).astype(np.float32))
    assert hp.flt(out[rows[:, 0] == 0x80, 0]) == -1.0
    rows, out = run("unpack_snorm_2x16")
    for c, code in ((0, rows[:, 0] & np.uint32(0xFFFF)), (1, rows[:, 0] >> np.uint32(16))):
        want = np.maximum(code.astype(np.uint16).view(np.int16).astype(np.float64) / 32767.0, -1.0)
        assert np.array_equal(hp.flt(out[:, c]), want.astype(np.float32))
    rows, out = run("unpack_unorm_rgb")
    for c in range(3):
        assert np.array_equal(hp.flt(out[:, c]), (((rows[:, 0] >> np.uint32(8 * c)) & np.uint32(0xFF)).astype(np.float64) / 255.0).astype(np.float32))
    # the octahedral decode of every code in the set is a unit vector, to the few fp32 roundings of a normalisation
    rows, out = run("unpack_normal")
    assert np.abs(np.linalg.norm(hp.flt(out).astype(np.float64), axis=1) - 1.0).max() < 4 * 2.0 ** -23


def test_rng_against_integer_arithmetic(run):
    rows, out = run("rnd")
    pick = np.concatenate([np.arange(len(hp.RND_WORDS)), np.arange(len(hp.RND_WORDS), len(rows), 997)])
    for i in pick:
        seed, word = hp.rnd_word(int(rows[i, 0]))
        assert out[i, 0] == seed and hp.flt(out[i, 1:2])[0] == F32(word) * F32(2.0 ** -32), i     # (float)word rounds to nearest even
    f = hp.flt(out[:len(hp.RND_WORDS), 1])
    w = dict(zip(hp.RND_WORDS, f))
    assert w[0] == 0.0 and w[0xFFFFFFFF] == 1.0 and w[0xFFFFFF80] == 1.0 and w[0xFFFFFF7F] < 1.0     # the tie at 2^32 - 128 goes up to 1.0
    assert w[(1 << 24) + 1] == F32(2.0 ** -8) and w[(1 << 24) + 2] == F32((2 ** 24 + 2) * 2.0 ** -32)   # 2^24 + 1 ties to even
    py_hash = lambda x: (lambda a: (lambda b: b ^ (b >> 16))((((a ^ (a >> 15)) * 0x846CA68B) & 0xFFFFFFFF)))((((x ^ (x >> 16)) * 0x7FEB352D) & 0xFFFFFFFF))
    rows, out = run("pcg_hash")
    for i in list(range(0, len(rows), 4099)) + [len(rows) - 1]:
        assert out[i, 0] == py_hash(int(rows[i, 0]))
    rows, out = run("init_rng")
    for i in range(0, len(rows), 257):
        px, py, frame, w_ = (int(x) for x in rows[i])
        assert out[i, 0] == py_hash((((py * w_ + px) & 0xFFFFFFFF) ^ py_hash(frame)))


def _ulps(got, want, floor):
    return np.abs(got - want) / np.maximum(np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), floor)


SINCOS_EXACT_REDUCTION = 2.0 ** 16 * np.pi / 2     # |k| < 2^16: k times the 8-bit and 11-bit pieces of pi/2 is exact in fp32


def test_sincos_exp_log_within_2ulp_of_libm_on_the_probe_sets(run):
    """The project's 2 ulp bound (test_oracle_kat.py, same ulp measure) over the probe's sets. Measured on these sets:
    sin / cos 1.54 ulp over the 1 064 924 rows with |x| <= 2^16 pi/2 (the Cody-Waite reduction is exact below that; beyond it the
    function is defined by device == oracle alone, e.g. 4.9e16 ulp at |x| ~ 1e9, and no call site goes beyond 2 pi);
    exp 0.92 ulp over all 2 248 293 finite rows up to the overflow cut-off, 0.70 ulp over [-104, -87] whose results are denormal;
    log 0.63 ulp over the 13 758 positive finite rows."""
    rows, out = run("sincos")
    x = hp.f64(rows[:, 0])
    m = np.isfinite(x) & (np.abs(x) <= SINCOS_EXACT_REDUCTION)
    worst = max(_ulps(hp.flt(out[m, c]).astype(np.float64), fn(x[m]), 2.0 ** -24).max() for c, fn in ((0, np.sin), (1, np.cos)))
    print("sincos: %d rows, worst %.3f ulp" % (m.sum(), worst))
    assert m.sum() > 1060000 and worst <= 2.0, worst
    assert hp.is_nan_bits(out[~np.isfinite(x)]).all()                           # +-inf and NaN give NaN
    rows, out = run("exp")
    x = hp.f64(rows[:, 0])
    got = hp.f64(out[:, 0])
    with np.errstate(over="ignore", under="ignore"):
        want = np.exp(x)
    m = np.isfinite(x) & (x <= float(hp.EXP_HI)) & (want <= float(np.finfo(np.float32).max))
    e = _ulps(got[m], want[m], 1.5e-45)
    dn = (x[m] >= -104.0) & (x[m] <= -87.0)
    print("exp: %d rows, worst %.3f ulp; denormal-result range %d rows, worst %.3f ulp" % (m.sum(), e.max(), dn.sum(), e[dn].max()))
    assert m.sum() > 2240000 and dn.sum() >= 2228225 and e.max() <= 2.0, e.max()
    assert np.isposinf(got[x > float(hp.EXP_HI)]).all() and (got[x < float(hp.EXP_LO)] == 0.0).all() and hp.is_nan_bits(out[np.isnan(x), 0]).all()
    assert np.isposinf(got[np.isfinite(x) & ~m & (x <= float(hp.EXP_HI))]).all()     # the last few floats below the cut-off overflow fp32
    rows, out = run("log")
    x = hp.f64(rows[:, 0])
    got = hp.f64(out[:, 0])
    m = np.isfinite(x) & (x > 0)
    e = _ulps(got[m], np.log(x[m]), 1.5e-45)
    print("log: %d rows, worst %.3f ulp" % (m.sum(), e.max()))
    assert m.sum() > 13000 and e.max() <= 2.0, e.max()
    assert np.isneginf(got[x == 0]).all() and hp.is_nan_bits(out[(x < 0) | np.isnan(x), 0]).all() and np.isposinf(got[np.isposinf(x)]).all()


def test_pow_gamma_within_first_order_bound(run):
    """pow(x, 1/2.2) = exp(a), a = y ln x: exp turns the rounding of a (half an ulp of a, plus y times log's E_log ulp) into a relative
    error of about that many ulp of a — up to 2 |a| (E_log + 0.5) ulp of the result, since ulp(a) <= 2^-23 |a| and an ulp of the result
    is at least 2^-24 of it — on top of exp's own E_exp. With the measured E_exp, E_log (0.75, 0.63) rounded up to 1 the bound is
    1 + 3 |a| ulp per row. Measured over the 16 646 161 positive rows of the gamma column: worst 60.75 ulp at x = 3.49e-33
    (0.61 of its bound), 4.21 ulp on [2^-7, 1]."""
    rows, out = run("pow")
    x = hp.f64(rows[:, 0])
    got = hp.f64(out[:, 0])
    gamma = rows[:, 1] == hp.bits(hp.GAMMA)[0]
    m = gamma & np.isfinite(x) & (x > 0) & (x <= 1.0)
    a = float(hp.GAMMA) * np.log(x[m])
    e = _ulps(got[m], np.exp(a), 1.5e-45)
    bound = 1.0 + 2.0 * np.abs(a) * (1.0 + 0.5)
    hi = x[m] >= 2.0 ** -7
    print("pow: %d rows, worst %.2f ulp, worst share of the bound %.3f, worst on [2^-7, 1] %.2f ulp" % (m.sum(), e.max(), (e / bound).max(), e[hi].max()))
    assert m.sum() > 16600000 and (e <= bound).all(), (e / bound).max()
    assert (got[gamma & (x == 0)] == 0.0).all() and (got[gamma & (x == 1.0)] == 1.0).all() and hp.is_nan_bits(out[gamma & (x < 0), 0]).all()


def test_brdf_rows_against_float64_models(run):
    """The well-conditioned ones of the seeded random rows of the probe sets through the float64 models, at
    test_oracle_independent.py's tolerances. Two fp32 cancellations decide what is well conditioned at those tolerances:
    - eval_unshadowed_light: the GGX denominator 1 - NdotH^2 (1 - a^2) carries about four roundings of 2^-24 absolute, and D has its
      square: rows with a denominator of at least 2^-9 keep D within 8 * 2^-24 / 2^-9 = 2.4e-4 < rtol = 3e-4 (99.9 % of the rows);
    - sample_ggx_vndf: z = sqrt(1 - t1^2 - t2^2) <= sqrt(1 - r1) carries 4 * 2^-24 / (2 z), and un-stretching by a = max(roughness^2,
      0.001) divides the direction's error by a: rows with a * sqrt(1 - r1) >= 2^-9 keep it below 2^-23 / 2^-9 = 6.1e-5 < atol = 2e-4.
    The other rows are still compared device against oracle, bit for bit."""
    n = hp.N_RANDOM
    rows, out = run("eval_light")
    r = hp.flt(rows[:n]).astype(np.float64)
    want = bm.brdf_light(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:12], r[:, 12], r[:, 13], r[:, 14:17], r[:, 17:20], r[:, 20:23])
    got = hp.flt(out[:n])
    Ld = bm.unit(r[:, 17:20] - r[:, 0:3])
    nh = np.einsum("ij,ij->i", r[:, 3:6], bm.unit(r[:, 6:9] + Ld))
    ok = 1.0 - nh ** 2 * (1.0 - r[:, 12] ** 4) >= 2.0 ** -9
    assert (want.max(axis=1) > 0).mean() > 0.3 and ok.mean() > 0.999
    assert np.allclose(got[ok], want[ok], rtol=3e-4, atol=1e-6), np.abs(got[ok] - want[ok]).max()
    rows, out = run("sample_ggx_vndf")
    r = hp.flt(rows[:n]).astype(np.float64)
    want = bm.vndf_sample(r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], r[:, 8])
    got = hp.flt(out[:n])
    ok = np.maximum(r[:, 6] ** 2, 1e-3) * np.sqrt(1.0 - r[:, 7]) >= 2.0 ** -9
    assert ok.mean() > 0.9
    assert np.allclose(got[ok], want[ok], atol=2e-4), np.abs(got[ok] - want[ok]).max()
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    rows, out = run("gi_target_pdf")
    r = hp.flt(rows[:n]).astype(np.float64)
    want, cosv = bm.gi_pdf(r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9], r[:, 10:13], r[:, 13:16])
    got = hp.flt(out[:n, 0])
    assert np.allclose(got, want, rtol=2e-5, atol=1e-7) and (got[cosv == 0.0] == 0.0).all()
    rows, out = run("build_onb")
    nrm = hp.flt(rows[:n]).astype(np.float64)
    t, b = bm.onb(nrm)
    assert np.allclose(hp.flt(out[:n, 0:3]), t, atol=1e-4) and np.allclose(hp.flt(out[:n, 3:6]), b, atol=1e-4)     # 1/(1 + n.z) amplifies near n.z = -1
    ok = nrm[:, 2] > -0.99
    assert np.allclose(hp.flt(out[:n, 0:3])[ok], t[ok], atol=2e-6) and np.allclose(hp.flt(out[:n, 3:6])[ok], b[ok], atol=2e-6)


def test_edge_rows_take_the_branches_they_name(run):
    """The hand-written edges do what they are there for, judged on the oracle's outputs."""
    rows, out = run("refract3")
    e = rows[hp.N_RANDOM:]
    o = hp.flt(out[hp.N_RANDOM:])
    grazing = (e[:, 0:3] == hp.EDGE_VECTORS[5]).all(axis=1) & (e[:, 3:6] == hp.EDGE_VECTORS[6]).all(axis=1)         # i = x, n = -y: ni = 0
    eta = hp.flt(e[:, 6])
    assert (o[grazing & (eta == 1.0)] == [1.0, 0.0, 0.0]).all() and (grazing & (eta == 1.0)).sum() == 1             # k = 0 exactly: sqrt(0), not the early out
    above = grazing & (eta > 1.0) & (eta < 1.001)
    below = grazing & (eta < 1.0) & (eta > 0.999)
    assert above.sum() == 2 and below.sum() == 2 and (o[above] == 0.0).all() and (o[below][:, 0] > 0.99).all() and (o[below][:, 1] > 0).all()
    rows, out = run("pack_normal")
    zero = (hp.flt(rows) == 0).all(axis=1)
    assert zero.sum() >= 8 and len(np.unique(out[zero, 0])) <= 2              # 0 / 0: NaN through the clamp's max -> one fixed code per sign of z
    rows, out = run("build_onb")
    z = hp.flt(rows)
    pole = (z[:, 0] == 0) & (z[:, 1] == 0) & (z[:, 2] == -1.0)
    assert pole.any() and (hp.flt(out[pole]) == [1, 0, 0, 0, -1, 0]).all() or (np.abs(hp.flt(out[pole])) == [1, 0, 0, 0, 1, 0]).all()
    negzero = (rows[:, 0] == 0) & (rows[:, 1] == 0) & (rows[:, 2] == 0x80000000)
    assert negzero.any() and np.isfinite(hp.flt(out[negzero])).all()           # -0.0 >= 0: the positive branch, a = -1
    rows, out = run("merge")
    taken = out[:, 12]
    assert set(np.unique(taken)) == {0, 1} and 0.2 < taken[:hp.N_RANDOM].mean() < 0.8
    assert np.array_equal(out[taken == 1, 8], rows[taken == 1, 20]) and np.array_equal(out[taken == 0, 8], rows[taken == 0, 8])
    rows, out = run("intersect_tri")
    assert 0.05 < out[:hp.N_RANDOM, 0].mean() < 0.8 and set(np.unique(out[:, 0])) == {0, 1}
