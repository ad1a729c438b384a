"""Stage-level GPU parity of the post-RT chain (sunray_amd/csrc/post.hip) on synthetic, adversarial buffers.

Each stage -- temporal accumulation, the a-trous denoise, the tonemap -- is called on its own through the C ABI
(sr_post_temporal / sr_post_denoise / sr_post_tonemap) and through the oracle on the same input bytes, and every image
the chain writes is compared byte for byte: both accumulation buffers (the target, and the history, which must stay as
it was), both denoise ping-pong buffers and the RGBA8 output. A mismatch names its stage. Inputs are raw bit patterns:
NaN, infinite, denormal and max-finite encodings per channel, sky, negative and NaN depths, -128 normal bytes,
roughness on either side of the 0.1 bypass, zero albedo, motion vectors that are sub-pixel, whole texels, the "+2"
no-history encoding, infinite, NaN, or that put uv - motion exactly on 0 or 1 -- mixed into smooth, real-looking
images. Extents run from 1x1 to 1920x1080 and 1x1048577 (65 537 workgroups in y). Every image the kernels write is
backed by W*H + 256 words whose tail holds a sentinel that must survive.

Also: the impulse response of the a-trous passes on the GPU, and the whole chain on rendered G-buffers at pass counts
and exposures other than the reference's defaults.
Run on an MI355X with:  python -m pytest tests/test_gpu_post_kernels.py -m gpu -q
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(__file__))
from post_util import (SENTINEL, TAIL, denoise_step, host_params, impulse_frame, impulse_positions,  # noqa: E402
                       impulse_response, make_inputs)

IMAGES = ("accum[0]", "accum[1]", "denoise[0]", "denoise[1]", "output")

EXTENTS = [(1, 1), (1, 7), (7, 1), (5, 3), (15, 16), (16, 16), (17, 17), (33, 9), (129, 3), (3, 129), (200, 152),
           (1920, 1080), (1, 70001), (70001, 1), (1, 1048577), (1048577, 1)]
FRAME_COUNTS = [0, 1, 2, 3, 4, 5, 0xFFFFFFFE, 0xFFFFFFFF]
EXPOSURES = [0.0, 0.37, 1.0, 8.0, 1e4]



@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: run them with -m gpu on an MI355X")
    from sunray_amd import runtime
    return runtime


def to_device(fr):
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    return types.SimpleNamespace(width=fr.width, height=fr.height, raw_color=t(fr.raw_color, np.float32),
                                 motion=t(fr.motion, np.int32), depth=t(fr.depth, np.int16), normal=t(fr.normal, np.int32),
                                 diffuse=t(fr.diffuse, np.int32), accum=[t(a, np.int32) for a in fr.accum],
                                 denoise=[t(a, np.int32) for a in fr.denoise], output=t(fr.output, np.int32))


def written(fr):
    return fr.accum + fr.denoise + [fr.output]


def run_stage(oracle, fr, dev, stage, frame_count=0, passes=4, exposure=1.0):
    """One stage on the oracle and on the GPU, both starting from `fr`'s images. Asserts that the five images are equal
    byte for byte, that the images the stage must not write are as they were, and that every canary tail survived.
    Returns the GPU's images (host copies, tails included)."""
    import torch
    from sunray_amd._lib import lib, check
    W, H = fr.width, fr.height
    n = W * H
    host = types.SimpleNamespace(**vars(fr))
    host.accum, host.denoise, host.output = [a.copy() for a in fr.accum], [a.copy() for a in fr.denoise], fr.output.copy()
    getattr(oracle.lib(), "orc_post_" + stage)(C.byref(host_params(host, frame_count, exposure, passes)))
    for d, s in zip(written(dev), written(fr)):
        d.copy_(torch.from_numpy(s.view(np.int32)))
    p = abi.post_params(dev, frame_count, lambda t: t.data_ptr(), exposure, passes)
    check(getattr(lib(), "sr_post_" + stage)(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = [t.cpu().numpy().view(np.uint32) for t in written(dev)]
    targets = {"temporal": {"accum[%d]" % (frame_count % 2)}, "denoise": {"denoise[0]", "denoise[1]"} if passes > 1 else {"denoise[0]"},
               "tonemap": {"output"}}[stage]
    what = "%s %dx%d, frame_count %d, %d passes, exposure %g" % (stage, W, H, frame_count, passes, exposure)
    for name, g, w, before in zip(IMAGES, got, written(host), written(fr)):
        assert (w[n:] == SENTINEL).all(), "%s: the oracle wrote behind %s" % (what, name)
        nt = int((g[n:] != SENTINEL).sum())
        assert nt == 0, "%s: %d canary words behind %s overwritten, first at +%d" % (what, nt, name, int(np.flatnonzero(g[n:] != SENTINEL)[0]))
        if name not in targets:
            assert np.array_equal(g, before), "%s: %s changed, the stage must not write it" % (what, name)
        nd = np.flatnonzero(g[:n] != w[:n])
        assert nd.size == 0, "%s: %s: %d of %d pixels differ, first (x %d, y %d): GPU %08x, oracle %08x" % (
            what, name, nd.size, n, nd[0] % W, nd[0] // W, g[nd[0]], w[nd[0]])
    return got


def _ids(extents):
    return ["%dx%d" % e for e in extents]


@pytest.mark.parametrize("W,H", EXTENTS, ids=_ids(EXTENTS))
def test_temporal_stage_equals_oracle(rt, oracle, W, H):
    fr = make_inputs(W, H)
    dev = to_device(fr)
    for fc in FRAME_COUNTS:          # <= 2: no history; 0xFFFFFFFE / 0xFFFFFFFF: the ping-pong index wraps
        run_stage(oracle, fr, dev, "temporal", frame_count=fc)


@pytest.mark.parametrize("W,H", EXTENTS, ids=_ids(EXTENTS))
def test_denoise_stage_equals_oracle(rt, oracle, W, H):
    fr = make_inputs(W, H)
    dev = to_device(fr)
    for passes in range(1, 9):       # steps 1..128: beyond W and H, with many empty lattices
        run_stage(oracle, fr, dev, "denoise", frame_count=passes, passes=passes)   # odd / even: both accum buffers are read


@pytest.mark.parametrize("W,H", EXTENTS, ids=_ids(EXTENTS))
def test_tonemap_stage_equals_oracle(rt, oracle, W, H):
    fr = make_inputs(W, H)
    dev = to_device(fr)
    for exposure in EXPOSURES:
        for passes in (3, 4):        # odd pass counts read denoise[0], even ones denoise[1]
            run_stage(oracle, fr, dev, "tonemap", passes=passes, exposure=exposure)


IMPULSE_EXTENTS = [(1, 1), (1, 7), (7, 1), (5, 3), (17, 17), (40, 24), (200, 3)]


@pytest.mark.parametrize("W,H", IMPULSE_EXTENTS, ids=_ids(IMPULSE_EXTENTS))
def test_atrous_impulse_response_on_gpu(rt, oracle, W, H):
    """One pass (step 1) changes exactly the bright pixel's 5x5 lattice inside the image. With N passes, the last one
    (step 2^(N-1), often wider than the image) is exactly one a-trous step of that width on what pass N-2 left in the
    other buffer; and every image equals the oracle's."""
    n = W * H
    for px, py in impulse_positions(W, H):
        fr = impulse_frame(W, H, px, py, TAIL)
        for img in written(fr):
            img[n:] = SENTINEL
        dev = to_device(fr)
        for passes in range(1, 9):
            got = run_stage(oracle, fr, dev, "denoise", frame_count=0, passes=passes)
            last = got[2 + (passes - 1) % 2][:n]
            before = fr.accum[0][:n].copy() if passes == 1 else got[2 + passes % 2][:n].copy()
            if passes == 1:
                assert np.array_equal(last != before, impulse_response(W, H, px, py, 1)), (px, py)
            one_step = np.zeros(n, np.uint32)
            denoise_step(oracle, fr, before, one_step, 1 << (passes - 1))
            assert np.array_equal(one_step, last), "impulse at (%d, %d): pass %d is not one step of %d" % (px, py, passes, 1 << (passes - 1))


def test_post_chain_on_rendered_frames_at_other_settings(rt, oracle, blue_noise):
    """RIS + final + the post chain on the Cornell box (ragged 200x152, slow dolly, 5 frames), with denoise_passes
    1, 2, 3, 5, 8 and exposure 0.37 and 8 after each frame's temporal pass: every image equals the oracle's."""
    import torch
    from sunray_amd._lib import lib, check
    desc = scenes.cornell_box()
    W, H = 200, 152
    osc, gsc = oracle.OracleScene().load(desc), rt.Scene(0).load(desc)
    of, gf = oracle.HostFrame(W, H, blue_noise), rt.DeviceFrame(W, H, blue_noise)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    prev = None
    for f in range(5):
        pos = (desc.camera_pos[0] + 0.02 * f, desc.camera_pos[1], desc.camera_pos[2])
        om = oracle.camera_matrices(pos, desc.camera_target, desc.fov_y, W, H, prev)
        gm = rt.camera_matrices(pos, desc.camera_target, desc.fov_y, W, H, prev)
        prev = list(om.view_proj)
        osc.trace_ris(of, om, f); osc.trace_final(of, om, f)
        gsc.trace_ris(gf, gm, f); gsc.trace_final(gf, gm, f)
        oracle.lib().orc_post_temporal(C.byref(abi.post_params(of, f, lambda a: a.ctypes.data)))
        check(lib().sr_post_temporal(C.byref(abi.post_params(gf, f, lambda t: t.data_ptr())), stream))
        outputs = set()
        for passes in (1, 2, 3, 5, 8):
            for exposure in (0.37, 8.0):
                po = abi.post_params(of, f, lambda a: a.ctypes.data, exposure, passes)
                pg = abi.post_params(gf, f, lambda t: t.data_ptr(), exposure, passes)
                oracle.lib().orc_post_denoise(C.byref(po)); oracle.lib().orc_post_tonemap(C.byref(po))
                check(lib().sr_post_denoise(C.byref(pg), stream)); check(lib().sr_post_tonemap(C.byref(pg), stream))
                h = gf.host()
                what = "frame %d, %d passes, exposure %g" % (f, passes, exposure)
                for name, want, got in (("accum", of.accum[f % 2], h["accum"][f % 2]), ("denoise[0]", of.denoise[0], h["denoise"][0]),
                                        ("denoise[1]", of.denoise[1], h["denoise"][1]), ("output", of.output, h["output"])):
                    nd = int((want != got).sum())
                    assert nd == 0, "%s: %s: %d of %d pixels differ" % (what, name, nd, W * H)
                outputs.add(of.output.tobytes())
        assert len(outputs) == 10           # every setting made a different picture
