"""Shared helpers of the post-RT chain tests (test_oracle_post_independent.py, test_gpu_post_kernels.py): exact
codecs of the packed image formats, SrPostParams-shaped host frames, the single a-trous step of the oracle, the impulse
frame of the tap-lattice tests and the seeded adversarial frame generator of the stage tests."""
import ctypes as C
import functools
import types

import numpy as np

from sunray_amd import abi

TAIL = 256                      # canary words behind every image the chain writes
SENTINEL = 0xA5C3E10F

F32_SPECIALS = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7F800000, 0xFF800000, 0xBF800000, 0x80000000, 0x7F7FFFFF,
                         0x47800000, 0x477FE000, 0x00000001, 0x387FFFFF, 0x38800000, 0x30000000, 0x2FFFFFFF, 0x4E6E6B28],
                        np.uint32)   # NaNs, +-inf, -1, -0, fp32 max, 65536, 65504, an fp32 denormal, B10G11R11 denormal edges, 1e9
DEPTH_SPECIALS = np.array([0x70E2, 0x70E1, 0x7C00, 0x7BFF, 0xC000, 0x8000, 0x7E00, 0x7C01, 0xFE00, 0x0001, 0xFC00],
                          np.uint16)  # 10000 (sky), the half below it, +inf (sky), 65504, -2, -0, NaNs, a denormal, -inf
MOTION_SPECIALS = np.array([0x00000000, 0x40004000, 0x00007C00, 0x0000FC00, 0x7C000000, 0xFC000000, 0x00007E00, 0x7E000000,
                            0xFE01FE01], np.uint32)   # zero, +2 (no history), +-inf in x, +-inf in y, NaN in x, in y, in both


# ---- exact decoding of the packed formats, and the nearest code of a float64 value -----------------------------------
def ufloat_decode(code, mant):
    code = np.asarray(code, dtype=np.int64)
    e, m = code >> mant, code & ((1 << mant) - 1)
    v = np.where(e == 0, m * 2.0 ** (-14 - mant), (1.0 + m / float(1 << mant)) * np.exp2(e - 15.0))
    return np.where(e == 31, np.where(m == 0, np.inf, np.nan), v)


def ufloat_encode(x, mant):
    """Nearest code of an unsigned small float (5-bit exponent, bias 15): negative -> 0, above the largest finite ->
    the largest finite, +inf -> inf, NaN -> NaN. Used for the model's side of a comparison and to write inputs."""
    x = np.asarray(x, dtype=np.float64)
    max_finite = (30 << mant) | ((1 << mant) - 1)
    pos = np.isfinite(x) & (x > 0)
    xs = np.where(pos, x, 1.0)
    _, k = np.frexp(xs)                                         # xs = f * 2^k, f in [0.5, 1)
    e = np.maximum(k.astype(np.int64) - 1, -14)                 # binade; below 2^-14 the denormal spacing
    steps = np.rint(np.ldexp(xs, (mant - e).astype(np.int32))).astype(np.int64)   # value in units of its binade's spacing
    code = np.where(e == -14, steps, ((e + 15) << mant) + steps - (1 << mant))
    code = np.where(pos, np.minimum(code, max_finite), 0)
    code = np.where(x == np.inf, 31 << mant, code)
    return np.where(np.isnan(x), (31 << mant) | 1, code)


def b10g11r11_codes(v):
    v = np.asarray(v, dtype=np.uint32).astype(np.int64)
    return np.stack([v & 0x7FF, (v >> 11) & 0x7FF, v >> 22], -1)


def b10g11r11_decode(v):
    c = b10g11r11_codes(v)
    return np.stack([ufloat_decode(c[..., 0], 6), ufloat_decode(c[..., 1], 6), ufloat_decode(c[..., 2], 5)], -1)


def b10g11r11_encode(rgb):
    rgb = np.asarray(rgb, dtype=np.float64)
    c = [ufloat_encode(rgb[..., 0], 6), ufloat_encode(rgb[..., 1], 6), ufloat_encode(rgb[..., 2], 5)]
    return np.asarray(c[0] | (c[1] << 11) | (c[2] << 22)).astype(np.uint32)


def encoded_codes(rgb):
    return b10g11r11_codes(b10g11r11_encode(rgb))


def half_decode(h):
    return np.asarray(h, dtype=np.uint16).view(np.float16).astype(np.float64)


def snorm8_decode(b):
    return np.maximum(np.asarray(b, dtype=np.uint8).view(np.int8).astype(np.float64) / 127.0, -1.0)


# ---- host frames and the oracle's single a-trous step ----------------------------------------------------------------
def post_frame(W, H, extra=0):
    """SrPostParams-shaped host buffers; the images the chain writes are `extra` words longer than W*H."""
    n = W * H
    z = lambda k, dt=np.uint32: np.zeros(k, dtype=dt)
    return types.SimpleNamespace(width=W, height=H, raw_color=np.zeros((n, 4), np.float32), motion=z(n),
                                 depth=z(n, np.uint16), normal=z(n), diffuse=z(n), accum=[z(n + extra), z(n + extra)],
                                 denoise=[z(n + extra), z(n + extra)], output=z(n + extra))


def host_params(fr, frame_count=0, exposure=1.0, passes=4):
    return abi.post_params(fr, frame_count, lambda a: a.ctypes.data, exposure, passes)


def denoise_step(oracle, fr, src, dst, step):
    """One a-trous pass of width `step` of the oracle over `fr`'s G-buffer, from image `src` into `dst` (uint32)."""
    assert src.dtype == np.uint32 and dst.dtype == np.uint32 and src.flags.c_contiguous and dst.flags.c_contiguous
    oracle.lib().orc_post_denoise_step(C.byref(host_params(fr)), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                       C.c_int(step))


def pack_normal_bytes(n, rough_byte):
    b = np.rint(np.clip(n, -1, 1) * 127.0).astype(np.int64) & 0xFF
    return np.asarray(b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (np.asarray(rough_byte, np.int64) << 24)).astype(np.uint32)


# ---- impulse response of one a-trous step ----------------------------------------------------------------------------
BASE_RGB = (0.03125, 0.25, 0.25)         # illumination (0.0625, 0.5, 0.5) over an albedo of 0.5: every product is exact
SPIKE_RGB = (0.75, 0.0361328125, 0.25)   # same luminance to 3e-4, so the luma edge-stop stays ~1; the red jump shows


def impulse_frame(W, H, px, py, extra=0):
    """A uniform rough G-buffer (depth 3, normal +y, roughness 0.5, albedo 0.5) under a constant colour with one
    bright pixel at (px, py), in accum[0]. A pixel whose taps all hold the constant keeps its bits exactly."""
    fr = post_frame(W, H, extra)
    fr.depth[:] = 0x4200
    fr.normal[:] = pack_normal_bytes(np.array([0.0, 1.0, 0.0]), 64)
    fr.diffuse[:] = b10g11r11_encode(np.array([0.5, 0.5, 0.5]))
    fr.accum[0][:W * H] = b10g11r11_encode(np.array(BASE_RGB))
    fr.accum[0][py * W + px] = b10g11r11_encode(np.array(SPIKE_RGB))
    return fr


def impulse_response(W, H, px, py, step):
    """Pixels one pass of `step` must change: (px + i*step, py + j*step), i, j in -2..2, inside the image; the bright
    pixel itself only if one of those others exists."""
    m = np.zeros((H, W), bool)
    for j in range(-2, 3):
        for i in range(-2, 3):
            x, y = px + i * step, py + j * step
            if 0 <= x < W and 0 <= y < H and (i, j) != (0, 0):
                m[y, x] = True
    m[py, px] = m.any()
    return m.reshape(-1)


def impulse_positions(W, H):
    """Centre, corners and edge midpoints."""
    return [(x, y) for y in sorted({0, H // 2, H - 1}) for x in sorted({0, W // 2, W - 1})]


# ---- seeded adversarial frames of the stage tests --------------------------------------------------------------------
def ufloat_codes(rng, n, mant, special):
    """Codes of one B10G11R11 channel: values around 2^-6..2 and, on half the `special` pixels, zero, denormal,
    smallest normal, max-finite, inf and NaN encodings."""
    specials = np.array([0, 1, (1 << mant) - 1, 1 << mant, (30 << mant) | ((1 << mant) - 1), 31 << mant, (31 << mant) | 1,
                         (31 << mant) | ((1 << mant) - 1)], np.int64)
    code = (rng.integers(9, 17, n) << mant) | rng.integers(0, 1 << mant, n)
    pick = special & (rng.random(n) < 0.5)
    code[pick] = rng.choice(specials, int(pick.sum()))
    return code


def packed_colours(rng, smooth, special):
    n = len(smooth)
    adv = ufloat_codes(rng, n, 6, special) | (ufloat_codes(rng, n, 6, special) << 11) | (ufloat_codes(rng, n, 5, special) << 22)
    return np.where(special, adv, b10g11r11_encode(smooth * rng.uniform(0.9, 1.1, (n, 3)))).astype(np.uint32)


def edge_motions(extent):
    """For each coordinate c of an axis `extent` long: the half-float bits of a motion m with (c + 0.5) / extent - m
    exactly 1.0, and of one with it exactly 0.0, in fp32 as the kernel computes it; -1 where no half does it."""
    uv = (np.arange(extent, dtype=np.float32) + np.float32(0.5)) / np.float32(extent)
    out = []
    for target in (1.0, 0.0):
        h = (uv.astype(np.float64) - target).astype(np.float16)
        best = np.full(extent, -1, np.int64)
        for cand in (np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf)), h):
            hit = (uv - cand.astype(np.float32)) == np.float32(target)
            best = np.where(hit, cand.view(np.uint16).astype(np.int64), best)
        out.append(best)
    return out


@functools.lru_cache(maxsize=None)     # one frame per extent: the three stage tests of an extent share it
def make_inputs(W, H):
    """Seeded synthetic frame: smooth images with ~15 % adversarial pixels per buffer, canary tails armed."""
    rng = np.random.default_rng(W * 7919 + H)
    n = W * H
    y, x = np.divmod(np.arange(n), W)
    fx, fy = x / W, y / H
    smooth = np.stack([0.6 + 0.5 * np.sin(7 * fx + 3 * fy), 0.5 + 0.4 * np.cos(5 * fy - 2 * fx), 0.4 + 0.3 * np.sin(4 * (fx + fy))], -1)
    adv = lambda: rng.random(n) < 0.15
    fr = post_frame(W, H, TAIL)
    # raw fp32 colour: NaN, +-inf, negative, huge and denormal values, per channel
    raw = (smooth * rng.uniform(0.8, 1.25, (n, 3))).astype(np.float32).view(np.uint32)
    pick = adv()[:, None] & (rng.random((n, 3)) < 0.5)
    raw[pick] = rng.choice(F32_SPECIALS, int(pick.sum()))
    fr.raw_color.view(np.uint32)[:, :3] = raw
    fr.raw_color[:, 3] = 1.0
    # depth: a ramp with steps of a few half ulps between neighbours; sky (10000 and +inf), negative, NaN
    d = (2.0 + 3.0 * fx + fy).astype(np.float16).view(np.uint16).astype(np.int64) + rng.integers(-2, 3, n)
    d = d.astype(np.uint16)
    a = adv()
    d[a] = rng.choice(DEPTH_SPECIALS, int(a.sum()))
    fr.depth[:] = d
    # normals: a smooth field; -128 bytes; roughness bytes 12 and 13 (0.0945 / 0.1024) around the 0.1 bypass, -128, 0
    nrm = np.stack([0.4 * np.sin(9 * fx), np.ones(n), 0.4 * np.cos(7 * fy)], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    nb = pack_normal_bytes(nrm, rng.choice(np.array([12, 13, 64, 100, 127]), n, p=[0.1, 0.1, 0.3, 0.25, 0.25]))
    nb = nb.view(np.uint8).reshape(n, 4).copy()
    pick = adv()[:, None] & (rng.random((n, 4)) < 0.3)
    nb[pick] = rng.choice(np.array([0x80, 0x00, 12, 13], np.uint8), int(pick.sum()))
    fr.normal[:] = nb.view(np.uint32).reshape(-1)
    # albedo: smooth, zero (the max(albedo, 0.001) clamp), special encodings
    a = adv()
    alb = packed_colours(rng, 0.2 + 0.5 * smooth[:, ::-1], a)
    alb[a & (rng.random(n) < 0.3)] = 0
    fr.diffuse[:] = alb
    # motion: sub-pixel and whole-texel moves, the specials, and moves that land exactly on the screen's edges
    m = rng.uniform(-1.5, 1.5, (n, 2)) / np.array([W, H])
    whole = rng.random(n) < 0.2
    m[whole] = rng.integers(-2, 3, (int(whole.sum()), 2)) / np.array([W, H])
    mh = m.astype(np.float16).view(np.uint16).astype(np.uint32)
    motion = mh[:, 0] | (mh[:, 1] << 16)
    a, kind = adv(), rng.integers(0, 3, n)
    sel = a & (kind == 0)
    motion[sel] = rng.choice(MOTION_SPECIALS, int(sel.sum()))
    for axis, coord, extent in ((0, x, W), (1, y, H)):
        to1, to0 = edge_motions(extent)
        c = np.where(rng.random(n) < 0.5, to1[coord], to0[coord])
        sel = a & (kind == axis + 1) & (c >= 0)
        shift = 16 * axis
        motion[sel] = (motion[sel] & ~np.uint32(0xFFFF << shift)) | (c[sel].astype(np.uint32) << shift)
    fr.motion[:] = motion
    # the images the chain reads and writes: B10G11R11 with specials; the output starts as noise
    fr.accum[0][:n] = packed_colours(rng, smooth, adv())
    fr.accum[1][:n] = packed_colours(rng, smooth[:, ::-1], adv())
    fr.denoise[0][:n] = packed_colours(rng, 3.0 * smooth, adv())
    fr.denoise[1][:n] = packed_colours(rng, 0.3 * smooth, adv())
    fr.output[:n] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for img in fr.accum + fr.denoise + [fr.output]:
        img[n:] = SENTINEL
    return fr
