"""Moving-camera frame pairs for the tests of the history-reach check (csrc/strip_copy.hip): the oracle's RIS pass with its read
log switched on gives, per pixel, the temporal-history reads the pass really computes and the motion vector it stores; the check's
restatement (tests/strip_reference.py) must cover the former from the latter. Shared by tests/test_history_reads_host.py (CPU) and
tests/test_gpu_strip_kernels.py (the kernel on the device's motion plane of the same frames)."""
import numpy as np

import strip_reference as ref
from sunray_amd import scenes

SLIDES = (2.0, 7.0, 25.0)          # pixels per frame along the tested axis, each in both directions
PROBE = 0.02                       # world units of the calibration slide

_cache = {}


def small_atrium():
    return scenes.atrium(columns_per_side=4, col_segments=16, col_rings=4, floor_div=8, tex=64, n_lamps=6)


SCENES = {"cornell_glass_mirror": scenes.cornell_glass_mirror, "small_atrium": small_atrium}


def camera_frame(desc):
    """(forward, right, up) of the scene's camera."""
    pos, tgt = np.array(desc.camera_pos, dtype=np.float64), np.array(desc.camera_target, dtype=np.float64)
    fwd = (tgt - pos) / np.linalg.norm(tgt - pos)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    return fwd, right, np.cross(right, fwd)


def moved(desc, d_pos, d_tgt):
    pos, tgt = np.array(desc.camera_pos, dtype=np.float64), np.array(desc.camera_target, dtype=np.float64)
    return tuple(pos + d_pos), tuple(tgt + d_tgt)


def ris_pair(oracle, scene_name, W, H, cam1, blue_noise):
    """Frame 0 from the scene's camera, frame 1 from cam1 = (pos, target), RIS pass only (the pass that reads the history and
    stores the motion vectors). Returns (motion [H, W] uint32, read log [H, W, 4] int32) of frame 1."""
    key = (scene_name, W, H, tuple(map(tuple, cam1)))
    if key not in _cache:
        desc = SCENES[scene_name]()
        if ("scene", scene_name) not in _cache:
            _cache[("scene", scene_name)] = oracle.OracleScene().load(desc)
        osc = _cache[("scene", scene_name)]
        of = oracle.HostFrame(W, H, blue_noise)
        m0 = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, None)
        osc.trace_ris(of, m0, 0)
        m1 = oracle.camera_matrices(cam1[0], cam1[1], desc.fov_y, W, H, list(m0.view_proj))
        log = np.zeros((H, W, 4), dtype=np.int32)
        osc.set_read_log(log)
        try:
            osc.trace_ris(of, m1, 1)
        finally:
            osc.set_read_log(None)
        _cache[key] = (of.motion.reshape(H, W).copy(), log)
    return _cache[key]


def axis_motion_pixels(motion, cols):
    """|stored motion| along the axis in pixels, of the pixels that store a motion vector and are not sky (sky stores 0)."""
    H, W = motion.shape
    m = ref.half_bits_to_f32(motion & 0xFFFF if cols else motion >> 16).astype(np.float64)
    kind, _, _ = ref.reach_f32(motion, np.zeros(motion.shape), W if cols else H, cols)
    px = np.abs(m[(kind == ref.IN_RANGE) & (motion != 0)]) * (W if cols else H)
    return px if px.size else np.zeros(1)


def camera_moves(oracle, scene_name, W, H, cols, blue_noise):
    """[(label, (pos, target))]: slides of about 2, 7 and 25 pixels per frame along the axis, both directions, and one frame with a
    dolly and a yaw. "About": the median stored motion of the frame; the slide is scaled from a probe frame and corrected once
    from the frame it gives (image motion is nearly linear in a sideways translation). The yaw turns the view by
    min(5, W / 4) pixels."""
    key = ("moves", scene_name, W, H, cols)
    if key in _cache:
        return _cache[key]
    desc = SCENES[scene_name]()
    fwd, right, up = camera_frame(desc)
    along = right if cols else up

    def median_px(d):
        return float(np.median(axis_motion_pixels(ris_pair(oracle, scene_name, W, H, moved(desc, d * along, d * along), blue_noise)[0], cols)))
    per_unit = median_px(PROBE) / PROBE
    assert per_unit > 0.0
    moves = []
    for px in SLIDES:
        d = px / per_unit
        d *= px / median_px(d)
        for sign in (1.0, -1.0):
            moves.append(("slide %+g px" % (sign * px), moved(desc, sign * d * along, sign * d * along)))
    dist = np.linalg.norm(np.array(desc.camera_target) - np.array(desc.camera_pos))
    focal_px = 0.5 * H / np.tan(np.radians(desc.fov_y) / 2.0)
    moves.append(("dolly and yaw", moved(desc, 0.25 * fwd, min(5.0, W / 4.0) * dist / focal_px * right)))
    _cache[key] = moves
    return moves


def read_slack(motion, log, cols):
    """Checks one frame: every logged read inside the image lies in the restatement's [lo, hi] of its pixel's stored motion vector,
    along x and along y, and a pixel that stores the no-history marker logs no read. Returns (smallest distance, along the axis
    `cols` names, of a read from the nearer end of its range before the clip to the image, number of reads checked); raises
    AssertionError with the first offender."""
    from oracle.binding import NO_READ
    H, W = motion.shape
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    kx, lox, hix = ref.reach_f32(motion, xs, W, True)
    ky, loy, hiy = ref.reach_f32(motion, ys, H, False)
    _, lo_open, hi_open = ref.reach_f32(motion, xs if cols else ys, W if cols else H, cols, clip=False)
    marker = kx == ref.NO_HISTORY
    assert (marker == (ky == ref.NO_HISTORY)).all()
    assert (log[marker] == NO_READ).all(), "a pixel that stores the no-history marker logged a read"
    slack, n = None, 0
    for k in (0, 2):                                             # the DI read, the GI read
        rx, ry = log[..., k].astype(np.int64), log[..., k + 1].astype(np.int64)
        taken = rx != NO_READ
        assert (taken == (ry != NO_READ)).all()
        inside = taken & (rx >= 0) & (ry >= 0) & (rx < W) & (ry < H)
        assert ((kx == ref.IN_RANGE) & (ky == ref.IN_RANGE))[inside].all(), "a read from a pixel without a storable motion vector"
        miss = inside & ((rx < lox) | (rx > hix) | (ry < loy) | (ry > hiy))
        if miss.any():
            y, x = np.argwhere(miss)[0]
            raise AssertionError("pixel (%d, %d), motion 0x%08x: %s read (%d, %d) outside x [%d, %d] / y [%d, %d]" % (
                x, y, motion[y, x], "DI" if k == 0 else "GI", rx[y, x], ry[y, x], lox[y, x], hix[y, x], loy[y, x], hiy[y, x]))
        if inside.any():
            r = rx if cols else ry
            s = np.minimum(r - lo_open, hi_open - r)[inside].min()
            slack = s if slack is None else min(slack, s)
            n += int(inside.sum())
    return slack, n
