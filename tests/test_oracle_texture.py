"""Texture fetch + the textured half of closest_hit in the oracle (SURVEY.md §8a K4/K11 sample_texture,
rt_utils.slang:121-133; closest_hit.slang:34-46,56-72,82-87). The reference holds no texture vectors
(parity unpinned): the KATs below are hand-derived from the Vulkan texel-filtering equations, and an
independent float64 numpy restatement of those equations cross-checks the C code on random coordinates."""
import math

import numpy as np
import pytest

from sunray_amd import abi, scenes

N, L = abi.FILTER_NEAREST, abi.FILTER_LINEAR
REP, MIR, CLAMP = abi.ADDRESS_REPEAT, abi.ADDRESS_MIRRORED_REPEAT, abi.ADDRESS_CLAMP_TO_EDGE


def np_sample(img, mag, mode_u, mode_v, s, t):
    """Vulkan spec texel filtering at LOD 0, float64: (u,v) = (s*w, t*h); NEAREST floor; LINEAR -0.5 shift."""
    h, w = img.shape[:2]

    def wrap(i, n, mode):
        if mode == REP:
            return i % n
        if mode == MIR:
            m = i % (2 * n)
            return m if m < n else 2 * n - 1 - m
        return min(max(i, 0), n - 1)
    u, v = s * w, t * h
    px = img.astype(np.float64) / 255.0
    if mag == N:
        return px[wrap(int(np.floor(v)), h, mode_v), wrap(int(np.floor(u)), w, mode_u)]
    u, v = u - 0.5, v - 0.5
    i0, j0 = int(np.floor(u)), int(np.floor(v))
    a, b = u - i0, v - j0
    g = lambda i, j: px[wrap(j, h, mode_v), wrap(i, w, mode_u)]
    return (g(i0, j0) * (1 - a) + g(i0 + 1, j0) * a) * (1 - b) + (g(i0, j0 + 1) * (1 - a) + g(i0 + 1, j0 + 1) * a) * b


@pytest.fixture()
def tex_scene(oracle):
    s = oracle.OracleScene()
    img = np.array([[[0, 10, 20, 30], [255, 110, 120, 130]],
                    [[40, 50, 60, 70], [80, 90, 100, 200]]], dtype=np.uint8)   # 2x2, row 0 = t in [0, .5)
    s.add_image(img)
    for mag in (N, L):
        for mu in (REP, MIR, CLAMP):
            s.add_sampler(mag, mag, mu, mu)
    return s, img


def smp(mag, mode):
    return (0 if mag == N else 3) + mode


def test_sample_texture_hand_kats(tex_scene):
    s, img = tex_scene
    f = lambda *px: np.array(px, dtype=np.float32) / np.float32(255.0)
    # NEAREST picks the texel whose cell holds (s*w, t*h)
    assert (s.sample_texture(0, smp(N, REP), 0.25, 0.25) == f(0, 10, 20, 30)).all()
    assert (s.sample_texture(0, smp(N, REP), 0.75, 0.25) == f(255, 110, 120, 130)).all()
    assert (s.sample_texture(0, smp(N, REP), 0.25, 0.75) == f(40, 50, 60, 70)).all()
    assert (s.sample_texture(0, smp(N, REP), 1.25, -0.25) == f(40, 50, 60, 70)).all()          # repeat: (0.25, 0.75)
    assert (s.sample_texture(0, smp(N, MIR), 1.25, 0.25) == f(255, 110, 120, 130)).all()       # mirror: 1.25 -> 0.75
    assert (s.sample_texture(0, smp(N, MIR), -0.25, 0.25) == f(0, 10, 20, 30)).all()           # mirror: -0.25 -> 0.25
    assert (s.sample_texture(0, smp(N, CLAMP), 7.0, -3.0) == f(255, 110, 120, 130)).all()      # clamp: last column, first row
    # LINEAR at a texel centre returns that texel; at the image centre the mean of all four
    assert (s.sample_texture(0, smp(L, CLAMP), 0.25, 0.25) == f(0, 10, 20, 30)).all()
    mean = (f(0, 10, 20, 30) * np.float32(0.5) + f(255, 110, 120, 130) * np.float32(0.5)) * np.float32(0.5) + \
           (f(40, 50, 60, 70) * np.float32(0.5) + f(80, 90, 100, 200) * np.float32(0.5)) * np.float32(0.5)
    assert (s.sample_texture(0, smp(L, REP), 0.5, 0.5) == mean).all()
    # LINEAR on the edge: clamp repeats the edge texel, repeat blends with the opposite edge
    assert (s.sample_texture(0, smp(L, CLAMP), 0.0, 0.25) == f(0, 10, 20, 30)).all()
    edge = f(255, 110, 120, 130) * np.float32(0.5) + f(0, 10, 20, 30) * np.float32(0.5)       # i0 = -1 -> 1, i1 = 0, a = .5
    assert (s.sample_texture(0, smp(L, REP), 0.0, 0.25) == edge).all()
    assert (s.sample_texture(0, smp(L, MIR), 0.0, 0.25) == f(0, 10, 20, 30)).all()             # mirror: i0 = -1 -> 0
    # NULL_TEXTURE returns the fallback unchanged (rt_utils.slang:127-129); non-finite coordinates read as 0
    assert (s.sample_texture(abi.NULL_TEXTURE, 0, 0.3, 0.3, (1, 2, 3, 4)) == [1, 2, 3, 4]).all()
    assert (s.sample_texture(0, smp(N, REP), float("nan"), float("inf")) == f(0, 10, 20, 30)).all()


@pytest.mark.parametrize("mag", [N, L])
@pytest.mark.parametrize("mode", [REP, MIR, CLAMP])
def test_sample_texture_matches_float64_equations(oracle, mag, mode):
    rng = np.random.default_rng(5 + mag * 3 + mode)
    img = rng.integers(0, 256, size=(7, 5, 4), dtype=np.uint8)      # non-square, odd sizes
    s = oracle.OracleScene()
    s.add_image(img)
    s.add_sampler(mag, mag, mode, (mode + 1) % 3)                    # different modes per axis
    for u, v in rng.uniform(-3.0, 4.0, size=(400, 2)):
        u, v = float(np.float32(u)), float(np.float32(v))
        got = s.sample_texture(0, 0, u, v)
        want = np_sample(img, mag, mode, (mode + 1) % 3, u, v)
        if mag == N and (abs(u * 5 - round(u * 5)) < 1e-4 or abs(v * 7 - round(v * 7)) < 1e-4):
            continue   # on a texel boundary the fp32 wrap may pick the neighbour
        assert np.abs(got - want).max() < 3e-5, (u, v, got, want)


def test_images_are_widened_with_zero_channels(oracle):
    s = oracle.OracleScene()
    s.add_image(np.array([[200]], dtype=np.uint8))                       # R8 -> (R,0,0,0)   utils.rs:27-43
    s.add_image(np.array([[[10, 20, 30]]], dtype=np.uint8))              # RGB8 -> alpha 0
    s.add_sampler(N, N, REP, REP)
    assert (s.sample_texture(0, 0, 0.5, 0.5) == np.array([200, 0, 0, 0], dtype=np.float32) / np.float32(255)).all()
    assert (s.sample_texture(1, 0, 0.5, 0.5) == np.array([10, 20, 30, 0], dtype=np.float32) / np.float32(255)).all()


def test_textured_closest_hit_payload(oracle):
    """One textured quad facing +z: the payload's albedo / emission / roughness / metallic come from the
    textures at the hit's uv, and a flat normal map leaves the normal (almost) geometric."""
    s = oracle.OracleScene()
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, size=(8, 8, 4), dtype=np.uint8)
    mr = rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)
    flat = np.tile(np.array([128, 128, 255, 255], dtype=np.uint8), (4, 4, 1))
    tilt = np.tile(np.array([255, 128, 128, 255], dtype=np.uint8), (4, 4, 1))   # tangent-space (+1, 0, ~0)
    for im in (base, mr, flat, tilt):
        s.add_image(im)
    s.add_sampler(N, N, CLAMP, CLAMP)
    v, i = scenes.grid_patch((-1, -1, 0), (2, 0, 0), (0, 2, 0), 1, 1, (0, 0, 1), (1, 0, 0))
    mat = abi.material(base_color=(1, 1, 1, 1), roughness=0.8, metallic=0.5, emissive_factor=(1, 1, 1), emissive_strength=2.0,
                       textures={"base_color": (0, 0), "metallic_roughness": (1, 0), "normal": (2, 0), "emissive": (0, 0)})
    s.add_mesh(1, v, i, mat)
    v2 = v.copy(); v2["position"][:, 2] -= 5.0
    s.add_mesh(2, v2, i, abi.material(textures={"normal": (3, 0)}))
    s.set_instances([(1, [abi.IDENTITY_TRANSFORM]), (2, [abi.IDENTITY_TRANSFORM])])
    rays = np.zeros(2, dtype=abi.RAY)
    rays["origin"] = [(0.3, -0.4, 2.0), (0.3, -0.4, -2.0)]
    rays["dir"] = (0, 0, -1); rays["tmin"] = 0.001; rays["tmax"] = 100.0
    hits = s.trace_closest(rays)
    pl = s.shade_closest_hit(hits)
    u, vv = (0.3 + 1) / 2, (-0.4 + 1) / 2            # uv of the hit on the patch
    tx, ty = int(u * 8), int(vv * 8)
    want_rgb = base[ty, tx, :3]
    assert pl["albedo_packed"][0] == int(want_rgb[0]) | int(want_rgb[1]) << 8 | int(want_rgb[2]) << 16 | 0xFF << 24
    assert np.allclose(pl["emission"][0], want_rgb.astype(np.float32) / 255 * 2.0, atol=1e-6)
    rough, metal = np.frombuffer(np.uint32(pl["material_info"][0]).tobytes(), dtype=np.float16)
    assert abs(rough - 0.8 * mr[ty, tx, 1] / 255) < 2e-3 and abs(metal - 0.5 * mr[ty, tx, 2] / 255) < 2e-3
    n0 = oracle.unpack_normal(int(pl["normal_packed"][0]))
    assert np.allclose(n0, [0, 0, 1], atol=0.02)
    # second quad: normal map says tangent-space +x -> world normal leans to the tangent (+x)
    n1 = oracle.unpack_normal(int(pl["normal_packed"][1]))
    assert n1[0] > 0.95


# ---- the exact rational model, the probe mesh and the float64 payload model (helpers in texture_util.py) -----------------------
import os  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_util as tu  # noqa: E402


def _model_cases():
    """(extent, channel count): every extent with one channel count in turn, 7x5 and 64x64 with all three."""
    out = [(e, tu.CHANNELS[k % 3]) for k, e in enumerate(tu.EXTENTS)]
    out += [(e, c) for e in ((7, 5), (64, 64)) for c in tu.CHANNELS if (e, c) not in out]
    return out


@pytest.mark.parametrize("extent,ch", _model_cases())
def test_oracle_sample_texture_matches_exact_model(oracle, extent, ch):
    """The oracle's sample_texture against tu.exact_sample, the Vulkan LOD-0 texel-filtering equations in exact rational
    arithmetic (no coordinate pre-wrap, no rounding: valid at 1e30 and at denormals, where a float64 model loses the -0.5),
    over all 18 filter x address-u x address-v samplers plus two with min_filter != mag_filter, random coordinates in
    [-3, 4]^2 and every edge value of tu.EDGES on each axis. No sample is left out.

    Tolerance of a LINEAR result, derived, not tuned: wrap_coord is exact in fp32 for all three modes (s - floor(s),
    s - 2 * floor(s / 2) and the clamp lose no bits) and its result lies in [-1, 2]. u = wrapped * W and u - 0.5 round once
    each, at magnitudes below 2W, so each is off by at most W * 2^-23 and a filter weight by at most about W * 2^-22
    (H * 2^-22 on the other axis). Texel values lie in [0, 1], so a weight error moves the result by at most itself. The
    remaining operations (byte / 255, 1 - a, three lerps of values in [0, 1]) add a few units of 2^-24. Bound:
    (W + H) * 2^-22 + 2^-21.

    NEAREST: the model's texel, bit for bit, except where the exact u (or v) lies within max(W, H) * 2^-22 of an integer
    without being one: there either texel that meets at that boundary is accepted (tu.nearest_candidates). An exact integer
    u is computed exactly by the fp32 code too, so there only the model's texel passes."""
    h, w = extent
    img = tu.random_image(h, w, ch, seed=100 * h + w + ch)
    s = oracle.OracleScene()
    s.add_image(img)
    for smp in tu.SAMPLERS:
        s.add_sampler(*smp)
    rng = np.random.default_rng(h * 7 + w)
    coords = np.concatenate([rng.uniform(-3.0, 4.0, size=(100, 2)).astype(np.float32), tu.edge_pairs()])
    bound = tu.linear_bound(img)
    worst, in_band = 0.0, 0
    for k, smp in enumerate(tu.SAMPLERS):
        for u, v in coords:
            got = s.sample_texture(0, k, float(u), float(v))
            if smp[1] == N:
                cand = tu.nearest_candidates(img, smp, u, v)
                in_band += len(cand) > 1
                px = tuple(int(c) for c in np.rint(got.astype(np.float64) * 255.0))
                assert px in cand and (got == np.array(px, np.float32) / np.float32(255.0)).all(), (smp, u, v, got, cand)
            else:
                want = np.array([float(c) for c in tu.exact_sample(img, smp, u, v)])
                d = float(np.abs(got.astype(np.float64) - want).max())
                worst = max(worst, d)
                assert d <= bound, (smp, u, v, got, want, d, bound)
    print("%dx%dx%d: worst LINEAR difference %.3g = %.2f x bound; %d NEAREST samples in the accept-either band" % (h, w, ch, worst, worst / bound, in_band))


def test_mag_filter_is_the_one_used(oracle):
    """A sampler whose min_filter differs from its mag_filter filters like the same-filter sampler of its mag_filter."""
    img = tu.random_image(7, 5, 4, seed=9)
    s = oracle.OracleScene()
    s.add_image(img)
    ids = [s.add_sampler(*q) for q in [(N, L, REP, MIR), (L, L, REP, MIR), (N, N, REP, MIR), (L, N, REP, MIR)]]
    differ = 0
    for u, v in np.random.default_rng(4).uniform(-2, 3, size=(60, 2)):
        a, b, c, d = (s.sample_texture(0, i, float(u), float(v)) for i in ids)
        assert (a == b).all() and (c == d).all()
        differ += not (a == c).all()
    assert differ > 50


def test_non_finite_coordinate_kats(oracle):
    """Hand-derived answers for coordinates a glTF file can deliver and Vulkan leaves to the driver. On a 4x1 image with texels
    A B C D along u:
      * |s| >= 3e38, +-inf and NaN read as s = 0: NEAREST gives A; LINEAR + REPEAT at s = 0 has u - 0.5 = -0.5, so texels
        (-1 -> D, 0 -> A) with weight 0.5: the mean of D and A. The largest fp32 below 3e38 is not guarded: it is an integer,
        s - floor(s) = 0, the same answer by another path under REPEAT, but under CLAMP_TO_EDGE it clamps to the last texel
        D where 3e38 itself reads A: the two sides of the guard.
      * s = -1e-45 (the smallest denormal) under REPEAT: s - floor(s) = 1.0 exactly, u = 4. LINEAR: u - 0.5 = 3.5, texels
        (3 -> D, 4 -> A), weight 0.5: the mean of the last and the first texel. NEAREST: floor(4) = 4 -> A, where exact
        arithmetic gives D (the accept-either band of the model test).
      * CLAMP_TO_EDGE at +-inf reads as 0, not as the edge the sign points to."""
    img = np.array([[[10, 0, 0, 255], [50, 0, 0, 255], [90, 0, 0, 255], [250, 0, 0, 255]]], dtype=np.uint8)
    s = oracle.OracleScene()
    s.add_image(img)
    nr, lr, nc = s.add_sampler(N, N, REP, REP), s.add_sampler(L, L, REP, REP), s.add_sampler(N, N, CLAMP, CLAMP)
    f = lambda b: np.float32(b) / np.float32(255.0)
    A, D = f(10), f(250)
    mean_da = D * np.float32(0.5) + A * np.float32(0.5)
    below = float(np.nextafter(np.float32(3e38), np.float32(0)))
    for x in (3e38, -3e38, 3.4e38, float("inf"), float("-inf"), float("nan"), below, -below):
        assert s.sample_texture(0, nr, x, 0.5)[0] == A, x
        assert s.sample_texture(0, lr, x, 0.5)[0] == mean_da, x
        assert s.sample_texture(0, nc, x, 0.5)[0] == (D if x == below else A), x                             # below the guard: clamps
    assert s.sample_texture(0, nc, 1e30, 0.5)[0] == D and s.sample_texture(0, nc, -1e30, 0.5)[0] == A
    assert s.sample_texture(0, lr, -1e-45, 0.5)[0] == mean_da
    assert s.sample_texture(0, nr, -1e-45, 0.5)[0] == A
    assert s.sample_texture(0, nr, 1e-45, 0.5)[0] == A and s.sample_texture(0, nr, float(np.nextafter(np.float32(1), np.float32(0))), 0.5)[0] == D


def _tilt_scene(oracle, w_values):
    """One triangle per w value, normal +z, tangent +x with that w at vertex 0 (and the opposite sign at vertices 1, 2); the
    normal map is one texel saying tangent-space (0, +0.6, 0.8)."""
    s = oracle.OracleScene()
    s.add_image(np.array([[[128, 204, 230, 255]]], dtype=np.uint8))
    s.add_sampler(N, N, REP, REP)
    v, i = tu.probe_mesh(np.zeros((len(w_values), 2)))
    t = v["tangent"].copy()
    for k, w in enumerate(w_values):
        t[3 * k, 3] = w
        t[3 * k + 1:3 * k + 3, 3] = -1.0 if (w >= 0.0) else 1.0
    v["tangent"] = t
    s.add_mesh(1, v, i, abi.material(textures={"normal": (0, 0)}))
    s.set_instances([(1, [abi.IDENTITY_TRANSFORM])])
    return s


def test_handedness_kats(oracle):
    """closest_hit.slang:34: handedness = (vertex 0's tangent.w >= 0) ? 1 : -1, whatever the other vertices say: +1 for 1, 0.5, 0
    and -0.0 (which compares equal to 0), -1 for -1, -3 and NaN (every comparison with NaN is false). With normal +z and tangent
    +x the bitangent is +-y, so a normal-map texel leaning to tangent-space +y tilts the world normal to +-y."""
    ws = [1.0, 0.5, 0.0, -0.0, -1.0, -3.0, float("nan")]
    s = _tilt_scene(oracle, ws)
    for bary in ((0.0, 0.0), (0.25, 0.5)):                    # at vertex 0 and inside: vertex 0 decides everywhere
        h = tu.probe_hits(len(ws)); h["u"], h["v"] = bary
        pl = s.shade_closest_hit(h)
        for k, w in enumerate(ws):
            n = oracle.unpack_normal(int(pl["normal_packed"][k]))
            want = 1.0 if k < 4 else -1.0
            assert abs(n[1] - want * 0.6) < 0.01 and abs(n[0]) < 0.01 and abs(n[2] - 0.8) < 0.01, (w, n)


def test_probe_mesh_reads_exact_coordinates(oracle):
    """The probe of the GPU tests, checked on the oracle: shade_closest_hit on a record (tri = k, u = v = 0) equals the packed
    sample_texture at exactly probe coordinate k, non-finite coordinates, denormals and both zeros included; the normal set reads
    out through normal_packed, the other three lookups use the base-colour set."""
    img = tu.random_image(7, 5, 4, seed=77)
    uvs = np.concatenate([tu.edge_pairs(), np.random.default_rng(8).uniform(-3, 4, size=(200, 2)).astype(np.float32)])
    desc = tu.probe_scene(img, uvs)
    s = oracle.OracleScene().load(desc)
    n = len(uvs)
    lib = oracle.lib()
    for m in (0, 4, 9, 13, 17, 18, 19):
        pl = s.shade_closest_hit(tu.probe_hits(n, first=m * n))
        for k in range(n):
            c = s.sample_texture(0, m, float(uvs[k, 0]), float(uvs[k, 1]))
            assert pl["albedo_packed"][k] == lib.orc_pack_unorm_4x8(float(c[0]), float(c[1]), float(c[2]), 1.0)
            assert (pl["emission"][k] == c[:3] * np.float32(2.0)).all()
            assert pl["material_info"][k] == lib.orc_pack_half_2x16(float(np.float32(0.5) * c[1]), float(np.float32(0.75) * c[2]))
            r = s.sample_texture(0, m, float(uvs[n - 1 - k, 0]), float(uvs[n - 1 - k, 1]))
            sx, sy = r[0] * np.float32(2) - np.float32(1), r[1] * np.float32(2) - np.float32(1)
            sz = np.sqrt(np.float32(min(max(np.float32(1) - (sx * sx + sy * sy), np.float32(0)), np.float32(1))))
            got = oracle.unpack_normal(int(pl["normal_packed"][k])).astype(np.float64)
            want = np.array([sx, sy, sz], dtype=np.float64)
            assert np.abs(got - want / np.linalg.norm(want)).max() < 2e-4, (m, k, got, want)


NORMAL_ANGLE = 2.0 * 2.0 ** -15          # rad


def test_textured_payload_matches_float64_model(oracle):
    """The oracle's shade_closest_hit against tu.model_payload, a float64 restatement of closest_hit.slang:31-90 written from the
    shader (its texture samples come from the exact model), on the zoo scene: five different uv sets per vertex, per-vertex
    normals and tangents, tangent w in {1, 0.5, 0, -0.0, -1, -3, NaN} disagreeing inside a triangle, zero / cancelling /
    parallel tangents, a zero normal, rotated, non-uniformly scaled and mirrored instances; hit records at the three corners,
    the centroid and random interior points of every triangle. Margins, from the packing formats:
      * albedo bytes equal, or +-1 where the model's x * 255 is within 1e-3 of a rounding tie;
      * roughness and metallic halves within one fp16 ulp of the model's value;
      * emission: relative difference within 1e-5;
      * normal: at most NORMAL_ANGLE = 2 * 2^-15 rad between the unpacked oracle normal and the model's normal put through the
        same snorm16 octahedral code (two steps of its grid at the poles).
    Records whose model normal is not finite (zero normal, tangent parallel to the normal) are left to the bit-exact GPU parity
    and counted: they must all lie on the two triangles built for that purpose."""
    desc = tu.zoo_scene()
    s = oracle.OracleScene().load(desc)
    flat = tu.flatten(desc)
    hits = tu.zoo_hits(desc)
    pl = s.shade_closest_hit(hits)
    lib = oracle.lib()
    nan_gids = set(tu.zoo_case_gids(desc, tu.NAN_CASES))
    n_nan, worst = 0, dict(albedo=0.0, half=0.0, emission=0.0, angle=0.0)
    f16 = lambda bits: float(np.array([bits], dtype=np.uint16).view(np.float16)[0])
    for k, h in enumerate(hits):
        m = tu.model_payload(desc, flat, h)
        got_rgb = [(int(pl["albedo_packed"][k]) >> (8 * c)) & 0xFF for c in range(3)]
        assert int(pl["albedo_packed"][k]) >> 24 == 255
        for c in range(3):
            x = min(max(float(m["albedo"][c]), 0.0), 1.0) * 255.0
            near_tie = abs((x % 1.0) - 0.5) < 1e-3
            worst["albedo"] = max(worst["albedo"], abs(got_rgb[c] - x))
            assert got_rgb[c] == math.floor(x + 0.5) or (near_tie and abs(got_rgb[c] - x) < 0.5 + 1e-3), (k, c, got_rgb[c], x)
        for got_bits, want in ((int(pl["material_info"][k]) & 0xFFFF, m["roughness"]), (int(pl["material_info"][k]) >> 16, m["metallic"])):
            ulp = float(np.spacing(np.float16(want))) if want != 0 else 2.0 ** -24
            worst["half"] = max(worst["half"], abs(f16(got_bits) - want) / ulp)
            assert abs(f16(got_bits) - want) <= ulp, (k, f16(got_bits), want)
        for c in range(3):
            rel = abs(float(pl["emission"][k][c]) - m["emission"][c]) / max(abs(m["emission"][c]), 1e-30)
            worst["emission"] = max(worst["emission"], rel)
            assert rel <= 1e-5, (k, c, pl["emission"][k], m["emission"])
        if not np.isfinite(m["normal"]).all():
            n_nan += 1
            assert int(h["tri"]) in nan_gids, (k, h)
            continue
        a = tu.unpack_normal64(int(pl["normal_packed"][k]))
        b = tu.unpack_normal64(lib.orc_pack_normal(*[float(np.float32(x)) for x in m["normal"]]))
        ang = math.acos(min(1.0, float(np.dot(a, b))))
        worst["angle"] = max(worst["angle"], ang)
        assert ang <= NORMAL_ANGLE, (k, h, a, b, ang)
    print("zoo payload model: %d records, %d with a non-finite model normal; worst %s" % (len(hits), n_nan, worst))
    per_tri = 10                                                     # records per zoo triangle (tu.zoo_hits)
    assert 0 < n_nan <= len(nan_gids) * per_tri
    # the NaN cases were really reached: the oracle's normal of a zero vertex normal is the packed NaN pattern, not a direction
    zero_n = [k for k, h in enumerate(hits) if int(h["tri"]) in set(tu.zoo_case_gids(desc, (tu.CASE_ZERO_NORMAL,)))]
    assert len(zero_n) == 2 * per_tri and len(set(int(pl["normal_packed"][k]) for k in zero_n)) == 1
