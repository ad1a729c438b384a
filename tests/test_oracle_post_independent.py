"""Independent float64 models of the post-RT chain: temporal accumulation, one a-trous pass, the ping-pong of N passes,
the tonemap.

The oracle (oracle/orc_post.cpp) and the kernels (sunray_amd/csrc/post.hip) are two restatements of one reading of
temporal_accumulation.slang, denoise.slang and postprocess.slang, and the committed post golden was made by the oracle.
A mistake common to both -- a bilinear history fetch without the half-texel shift, a wrong tap lattice, swapped
edge-stopping terms -- passes every parity test and is pinned by the golden. These models come at the same operations
from their definitions, in vectorised float64 numpy and in a different shape from the C statement order (the bilinear
fetch as a 2x2 stencil of weights, the B3 spline as an outer product, the tap loop as shifted whole images), and are
compared with the fp32 oracle on random, well-conditioned inputs whose packed formats are decoded exactly. The bar, in
format codes (B10G11R11 per channel, RGBA8 per channel): equal, or one quantisation step apart on under 1 % of the
pixels; a larger difference only where one of the model's threshold tests lies within 1e-5 (relative) of its
boundary, and such pixels must be rare.

Also here: the impulse response of one a-trous step, i.e. which pixels a pass of step s may change at all. It checks
the tap geometry itself rather than agreement between two implementations; tests/test_gpu_post_kernels.py runs it on
the GPU. The codecs, frames and generators both files use live in tests/post_util.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from post_util import (b10g11r11_codes, b10g11r11_decode, b10g11r11_encode, denoise_step, encoded_codes,  # noqa: E402
                       half_decode, host_params, impulse_frame, impulse_positions, impulse_response, make_inputs,
                       pack_normal_bytes, post_frame, snorm8_decode)

LUMA = np.array([0.2126, 0.7152, 0.0722])
B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
NEAR = 1e-5          # relative distance to a threshold below which the model's branch may go either way


# ---- the models -------------------------------------------------------------------------------------------------
def temporal_model(cur, hist, motion, frame_count):
    """temporal_accumulation.slang: cur, hist (H, W, 3), motion (H, W, 2). Returns (colour, near-threshold mask, number of
    neighbours the luma gate kept out of each pixel's 3x3 min/max box)."""
    H, W, _ = cur.shape
    win = np.pad(cur, ((1, 1), (1, 1), (0, 0)), mode="edge")          # the 3x3 window, clamped to the image
    lc = cur @ LUMA
    thr = np.maximum(5.0 * lc, 0.08)
    lo, hi, near, gated = cur.copy(), cur.copy(), np.zeros((H, W), bool), np.zeros((H, W), int)
    for dy, dx in [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a, b) != (0, 0)]:
        nb = win[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        d = np.abs(nb @ LUMA - lc)
        take = (d < thr)[..., None]
        gated += ~take[..., 0]
        lo, hi = np.where(take, np.minimum(lo, nb), lo), np.where(take, np.maximum(hi, nb), hi)
        near |= np.abs(d - thr) <= NEAR * thr
    ys, xs = np.mgrid[0:H, 0:W]
    u, v = (xs + 0.5) / W - motion[..., 0], (ys + 0.5) / H - motion[..., 1]
    on = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1)
    near_edge = (np.minimum(np.abs(u), np.abs(u - 1)) <= NEAR) | (np.minimum(np.abs(v), np.abs(v - 1)) <= NEAR)
    # bilinear fetch with clamp-to-edge: texel centres sit at (i + 0.5) / size
    tx, ty = np.where(on, u, 0.5) * W - 0.5, np.where(on, v, 0.5) * H - 0.5
    ix, iy = np.floor(tx).astype(np.int64), np.floor(ty).astype(np.int64)
    ax, ay = (tx - ix)[..., None], (ty - iy)[..., None]
    stencil = {(0, 0): (1 - ax) * (1 - ay), (1, 0): ax * (1 - ay), (0, 1): (1 - ax) * ay, (1, 1): ax * ay}
    h = sum(w * hist[np.clip(iy + j, 0, H - 1), np.clip(ix + i, 0, W - 1)] for (i, j), w in stencil.items())
    blended = 0.86 * np.minimum(np.maximum(h, lo), hi) + 0.14 * cur
    use = on & (frame_count > 2)
    return np.where(use[..., None], blended, cur), (near & use) | (near_edge & (frame_count > 2)), gated


def atrous_model(col, depth, normal, rough, albedo, step):
    """One pass of denoise.slang at `step`: (H, W, 3) colour, depth, normal (H, W, 3), roughness, albedo."""
    H, W, _ = col.shape
    illum = col / np.maximum(albedo, 0.001)
    lum = illum @ LUMA
    r = 2 * step
    pad = lambda a: np.pad(a, ((r, r), (r, r)) + ((0, 0),) * (a.ndim - 2))
    P = {k: pad(a) for k, a in dict(illum=illum, lum=lum, depth=depth, normal=normal, albedo=albedo).items()}
    inside = pad(np.ones((H, W), bool))
    k2 = np.outer(B3, B3)
    num, den = illum * k2[2, 2], np.full((H, W), k2[2, 2])         # the centre enters once by itself ...
    for j in range(5):                                              # ... and once more as the middle tap
        for i in range(5):
            sl = (slice(r + (j - 2) * step, r + (j - 2) * step + H), slice(r + (i - 2) * step, r + (i - 2) * step + W))
            s = {k: a[sl] for k, a in P.items()}
            ratio = np.abs(lum - s["lum"]) / (np.maximum(lum, s["lum"]) * 0.4 + 0.01)
            power = (-8.0 * np.abs(depth - s["depth"]) + 80.0 * (np.sum(normal * s["normal"], -1) - 1.0)
                     - 50.0 * np.linalg.norm(albedo - s["albedo"], axis=-1) - ratio ** 2)
            w = np.where(inside[sl], np.exp(power) * k2[j, i], 0.0)
            num, den = num + w[..., None] * s["illum"], den + w
    out = num / np.maximum(den, 1e-4)[..., None] * albedo
    keep = (depth >= 10000.0) | (rough < 0.1)
    return np.where(keep[..., None], col, out)


def tonemap_model(col, exposure):
    """postprocess.slang: scrub non-finite pixels, exposure, ACES (Narkowicz), gamma 1/2.2, RGBA8_UNORM codes."""
    c = np.where(np.isfinite(col).all(-1, keepdims=True), col, 0.0) * float(np.float32(exposure))
    x = np.clip(c, 0.0, 100.0)
    m = np.clip(x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14), 0.0, 1.0)
    return np.rint(m ** (1 / 2.2) * 255.0).astype(np.int64)


# ---- helpers ----------------------------------------------------------------------------------------------------
def gbuffer_model_inputs(fr):
    """Exact float64 decode of a frame's G-buffer: depth, normal, roughness, albedo as (H, W[, 3])."""
    H, W = fr.height, fr.width
    nb = fr.normal.view(np.uint8).reshape(H, W, 4)
    return (half_decode(fr.depth).reshape(H, W), snorm8_decode(nb[..., :3]), snorm8_decode(nb[..., 3]),
            b10g11r11_decode(fr.diffuse).reshape(H, W, 3))


def assert_close_in_codes(got_codes, want_codes, near, what):
    """Equal, or one code apart on under 1 % of the pixels; more only at pixels flagged `near`, which must be rare."""
    near = np.asarray(near).reshape(-1)
    d = np.abs(got_codes.astype(np.int64) - want_codes.astype(np.int64)).reshape(near.size, -1).max(-1)
    one, far = int((d == 1).sum()), d > 1
    assert one <= 0.01 * d.size, "%s: %d of %d pixels one step off" % (what, one, d.size)
    bad = far & ~near
    assert not bad.any(), "%s: %d pixels more than one step off, first at %d (%d steps)" % (
        what, int(bad.sum()), int(np.flatnonzero(bad)[0]), int(d[bad][0]))
    assert int(far.sum()) <= max(2, 0.002 * d.size), "%s: %d pixels off at threshold boundaries" % (what, int(far.sum()))


def random_colours(rng, shape, lo=0.05, hi=2.0):
    """Colours exactly representable in B10G11R11 (so the raw fp32 colour quantises to itself)."""
    return b10g11r11_decode(b10g11r11_encode(rng.uniform(lo, hi, tuple(shape) + (3,))))


def noisy_colours(rng, H, W):
    """A smooth image with 20 % noise: neighbours are alike enough for the edge-stopping weights to let them in."""
    ys, xs = np.mgrid[0:H, 0:W]
    base = 0.6 + 0.4 * np.stack([np.sin(xs / 20.0), np.cos(ys / 15.0), np.sin((xs - ys) / 25.0)], -1)
    return b10g11r11_decode(b10g11r11_encode(base * rng.uniform(0.8, 1.2, (H, W, 3))))


def random_gbuffer(rng, fr):
    H, W = fr.height, fr.width
    ys, xs = np.mgrid[0:H, 0:W]
    depth = 2.0 + 0.004 * xs + 0.003 * ys + rng.normal(0, 0.005, (H, W))
    depth[rng.random((H, W)) < 0.03] = 20000.0                                  # sky
    fr.depth[:] = depth.astype(np.float16).view(np.uint16).reshape(-1)
    n = np.stack([0.1 * np.sin(xs / 30.0), np.ones((H, W)), 0.1 * np.cos(ys / 25.0)], -1) + rng.normal(0, 0.01, (H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    rough = rng.choice([5, 12, 13, 40, 90, 127], (H, W), p=[.05, .05, .05, .25, .3, .3])   # 12 and 13: either side of 0.1
    fr.normal[:] = pack_normal_bytes(n, rough).reshape(-1)
    albedo = 0.5 + 0.2 * np.stack([np.sin(xs / 30.0), np.cos(ys / 25.0), np.sin((xs + ys) / 40.0)], -1) + rng.normal(0, 0.005, (H, W, 3))
    albedo[rng.random((H, W)) < 0.03] = 0.0                                     # reaches max(albedo, 0.001)
    fr.diffuse[:] = b10g11r11_encode(albedo).reshape(-1)


# ---- temporal ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_count", [0, 2, 3, 4, 7, 0xFFFFFFFF])
def test_temporal_matches_float64_model(oracle, frame_count):
    W, H = 61, 37
    rng = np.random.default_rng(100 + frame_count % 97)
    fr = post_frame(W, H)
    cur = random_colours(rng, (H, W), 0.2, 1.0)
    dark = rng.random((H, W)) < 0.3       # a dark centre's gate (max(5 * luma, 0.08)) keeps its bright neighbours out
    cur[dark] = random_colours(rng, (int(dark.sum()),), 0.002, 0.03)
    fr.raw_color[:, :3] = cur.reshape(-1, 3)
    fr.raw_color[:, 3] = 1.0
    hist = random_colours(rng, (H, W), 0.05, 2.0)
    fr.accum[(frame_count + 1) % 2][:] = b10g11r11_encode(hist).reshape(-1)
    fr.accum[frame_count % 2][:] = 0x12345678
    mv = np.stack([rng.uniform(-2.5, 2.5, (H, W)) / W, rng.uniform(-2.5, 2.5, (H, W)) / H], -1).astype(np.float16)
    mv[rng.random((H, W)) < 0.05] = 2.0                                         # the RIS pass's "no history"
    bits = mv.view(np.uint16).astype(np.uint32)
    fr.motion[:] = (bits[..., 0] | (bits[..., 1] << 16)).reshape(-1)
    history_before = fr.accum[(frame_count + 1) % 2].copy()
    oracle.lib().orc_post_temporal(C.byref(host_params(fr, frame_count)))
    want, near, gated = temporal_model(cur, b10g11r11_decode(history_before).reshape(H, W, 3), mv.astype(np.float64), frame_count)
    assert np.array_equal(fr.accum[(frame_count + 1) % 2], history_before)
    assert_close_in_codes(b10g11r11_codes(fr.accum[frame_count % 2]), encoded_codes(want).reshape(-1, 3), near, "temporal")
    if frame_count > 2:       # the history branch really ran: most pixels are not the current colour
        assert (np.abs(want - cur).max(-1) > 0.02 * cur.max(-1)).mean() > 0.5
        assert (gated[dark] > 0).mean() > 0.5 and (gated[~dark] == 0).mean() > 0.5   # the luma gate really chose


# ---- a-trous ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 4, 8, 16, 32, 64, 128])
def test_atrous_pass_matches_float64_model(oracle, step):
    W, H = 53, 41
    rng = np.random.default_rng(step)
    fr = post_frame(W, H)
    random_gbuffer(rng, fr)
    col = noisy_colours(rng, H, W)
    src, dst = b10g11r11_encode(col).reshape(-1), np.full(W * H, 0xDEADBEEF, np.uint32)
    denoise_step(oracle, fr, src, dst, step)
    want = atrous_model(col, *gbuffer_model_inputs(fr), step)
    assert_close_in_codes(b10g11r11_codes(dst), encoded_codes(want).reshape(-1, 3), np.zeros(W * H, bool), "a-trous step %d" % step)
    if step <= 8:             # the filter really filtered
        assert (b10g11r11_codes(dst) != b10g11r11_codes(src)).any(-1).mean() > 0.5


@pytest.mark.parametrize("passes", range(1, 9))
def test_atrous_ping_pong_matches_float64_model(oracle, passes):
    """N passes: pass k reads what pass k-1 wrote (accum[frame_count % 2] first) at step 2^k; pass N-1 lands in
    denoise[(N-1) % 2] and pass N-2 stays in the other buffer. Each pass is held against the model applied to what the
    oracle's previous pass wrote."""
    W, H = 45, 38
    rng = np.random.default_rng(40 + passes)
    fr = post_frame(W, H)
    random_gbuffer(rng, fr)
    g = gbuffer_model_inputs(fr)
    fc = passes          # odd and even frame counts: both accumulation buffers are read
    fr.accum[fc % 2][:] = b10g11r11_encode(noisy_colours(rng, H, W)).reshape(-1)
    fr.accum[(fc + 1) % 2][:] = 0x0BADF00D
    prev, prev_out = fr.accum[fc % 2].copy(), None
    for n in range(1, passes + 1):
        fr.denoise[0][:] = 0xDEADBEEF
        fr.denoise[1][:] = 0xFEEDFACE
        oracle.lib().orc_post_denoise(C.byref(host_params(fr, fc, passes=n)))
        last, other = fr.denoise[(n - 1) % 2], fr.denoise[n % 2]
        want = atrous_model(b10g11r11_decode(prev).reshape(H, W, 3), *g, 1 << (n - 1))
        assert_close_in_codes(b10g11r11_codes(last), encoded_codes(want).reshape(-1, 3), np.zeros(W * H, bool),
                              "pass %d of %d" % (n, passes))
        if n == 1:
            assert (other == 0xFEEDFACE).all()                      # one pass leaves denoise[1] alone
        else:
            assert np.array_equal(other, prev_out)                  # pass N-2 stays in the other buffer
        prev_out = last.copy()
        prev = last.copy()
    assert (fr.accum[(fc + 1) % 2] == 0x0BADF00D).all()


# ---- tonemap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exposure", [0.0, 0.37, 1.0, 8.0, 1e4])
def test_tonemap_matches_float64_model(oracle, exposure):
    W, H = 97, 31
    rng = np.random.default_rng(7)
    fr = post_frame(W, H)
    n = W * H
    code = lambda mant: (rng.integers(0, 31, n) << mant) | rng.integers(0, 1 << mant, n)   # every finite code
    v = (code(6) | (code(6) << 11) | (code(5) << 22)).astype(np.uint32)
    special = rng.random(n) < 0.05
    v[special] = rng.choice(np.array([31 << 6, (31 << 6) | 5, 31 << 17, (31 << 27) | (3 << 22)], np.uint32), int(special.sum()))
    want = tonemap_model(b10g11r11_decode(v), exposure)
    for passes in (3, 4):                          # odd pass counts end in denoise[0], even ones in denoise[1]
        fr.denoise[(passes - 1) % 2][:] = v
        fr.denoise[passes % 2][:] = 0
        fr.output[:] = 0
        oracle.lib().orc_post_tonemap(C.byref(host_params(fr, 0, exposure, passes)))
        got = fr.output.view(np.uint8).reshape(n, 4).astype(np.int64)
        assert (got[:, 3] == 255).all()
        assert_close_in_codes(got[:, :3], want, np.zeros(n, bool), "tonemap exposure %g passes %d" % (exposure, passes))
        assert not got[special, :3].any()


# ---- impulse response of one a-trous step -----------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(37, 29), (1, 9), (9, 1), (130, 5), (1, 1)])
def test_atrous_impulse_response(oracle, W, H):
    for px, py in impulse_positions(W, H):
        for step in (1, 2, 3, 4, 8, 16, 32, 64, 128):
            fr = impulse_frame(W, H, px, py)
            dst = np.zeros(W * H, np.uint32)
            denoise_step(oracle, fr, fr.accum[0], dst, step)
            changed = dst != fr.accum[0]
            want = impulse_response(W, H, px, py, step)
            assert np.array_equal(changed, want), "impulse at (%d, %d), step %d: changed %s, want %s" % (
                px, py, step, np.flatnonzero(changed)[:12], np.flatnonzero(want)[:12])


def test_synthetic_inputs_reach_the_edge_cases():
    """The generator of tests/test_gpu_post_kernels.py really produces the edge cases those stage tests rely on."""
    fr = make_inputs(16, 16)
    uv = (np.arange(16, dtype=np.float32) + np.float32(0.5)) / np.float32(16)
    mx = (fr.motion & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    pux = uv[np.arange(256) % 16] - mx
    assert (pux == 1.0).any() and (pux == 0.0).any()
    fr = make_inputs(200, 152)
    assert (fr.motion == 0x40004000).any() and (fr.motion == 0x00007E00).any()
    rough = fr.normal >> 24
    assert (rough == 12).any() and (rough == 13).any()
    assert (fr.diffuse == 0).any()
