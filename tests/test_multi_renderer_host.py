"""CPU-side checks of the multi-device renderer's C ABI (sr_renderer_create_multi and friends): argument errors, the no-GPU
failure, what the strip entry points (sr_strip_pack / sr_strip_unpack / sr_history_reach_check) refuse, the restatement of the
history-reach check (strip_copy.hip; tests/strip_reference.py) on hand-worked cases, and an interval model of the RIS pass's
temporal read that the check's formula must cover."""
import ctypes as C

import numpy as np
import pytest

import strip_reference as ref
from strip_reference import counted, held_region, read_range
from sunray_amd import _lib, abi, runtime as rt


def has_gpu():
    import torch
    return torch.cuda.is_available()


def _devs(*d):
    return (C.c_int * max(len(d), 1))(*d)


def test_create_multi_argument_errors():
    L = _lib.lib()
    h = C.c_void_p()
    assert L.sr_renderer_create_multi(None, 2, 16, 16, 0, C.byref(h)) == -1
    assert L.sr_renderer_create_multi(_devs(0, 0), 2, 16, 16, 0, None) == -1
    assert L.sr_renderer_create_multi(_devs(0), 0, 16, 16, 0, C.byref(h)) == -1 and b"no devices" in L.sr_last_error()
    assert L.sr_renderer_create_multi(_devs(0, 0), 2, 0, 16, 0, C.byref(h)) == -1
    assert L.sr_renderer_create_multi(_devs(0, 0), 2, 16, 0, 0, C.byref(h)) == -1
    assert L.sr_renderer_create_multi(_devs(0, 0), 2, 16, 16, 2, C.byref(h)) == -1 and b"axis" in L.sr_last_error()
    assert L.sr_renderer_create_multi(_devs(0, -1), 2, 16, 16, 0, C.byref(h)) == -1 and b"negative" in L.sr_last_error()
    assert not h.value


def test_multi_entry_points_reject_null_arguments():
    L = _lib.lib()
    b = (C.c_uint32 * 3)(0, 8, 16)
    n, sc = C.c_uint64(), C.c_void_p()
    assert L.sr_renderer_set_strip_bounds(None, b) == -1
    assert L.sr_renderer_set_motion_halo(None, 16) == -1
    assert L.sr_renderer_replica_scene(None, 0, C.byref(sc)) == -1
    assert L.sr_renderer_read_history_overflow(None, C.byref(n)) == -1


def test_python_binding_argument_errors():
    with pytest.raises(ValueError):
        rt.Renderer((32, 32), devices=[0, 0], axis="diagonal")
    with pytest.raises(ValueError):
        rt.Renderer((32, 32), devices=[0, 0], bounds=[0, 32])          # wrong length: 3 cuts for 2 slots
    with pytest.raises(ValueError):
        rt.Renderer((32, 32), bounds=[0, 32])                          # strip options without devices


def test_create_multi_fails_without_gpu():
    if has_gpu():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SunrayError) as e:          # no CPU fallback: creation itself fails without a device
        rt.Renderer((32, 32), devices=[0, 0])
    assert e.value.code == -2
    h = C.c_void_p()
    assert _lib.lib().sr_renderer_create_multi(_devs(0, 0, 0), 3, 16, 16, 1, C.byref(h)) == -2 and not h.value


# ---- restatement of history_reach_check_kernel (strip_copy.hip): tests/strip_reference.py --------------------------------------
def test_held_region_hand_worked():
    b = [0, 40, 80, 120]
    assert held_region(b, 0, 16) == (0, 86)          # 40 + 30 + 16
    assert held_region(b, 1, 16) == (0, 120)         # 40 - 46 clips to 0, 80 + 46 clips to 120
    assert held_region(b, 2, 0) == (50, 120)
    assert held_region([0, 0, 72], 0, 32) == (0, 62)  # an empty strip still names a region; the renderer skips it


def test_read_range_hand_worked():
    # static camera: mv = 0 -> centre p + 0.5, widened by 1 + 0.5 on either side -> [p - 1, p + 2]
    assert read_range(60, 0.0, 120) == (59, 62)
    # a 7-pixel slide to the right in a 120-wide image: mv = -7/120 -> centre p + 7.5, margin 7/1024 + 1
    lo, hi = read_range(60, -7.0 / 120.0, 120)
    assert (lo, hi) == (65, 70)
    # clipped to the image; entirely outside -> no read
    assert read_range(0, 0.5, 120) is None           # centre -59.5: every candidate is negative
    assert read_range(119, -0.5, 120) is None


def test_check_counts_reads_leaving_the_held_region():
    b = [0, 40, 80, 120]
    held = held_region(b, 2, 0)                      # (50, 120): strip 80..120 + 30
    # the RIS rectangle of slot 2 starts at 50; a pixel there moving 7 px to the left reads ~43: outside
    assert counted(50, 7.0 / 120.0, 120, held)
    # with a 16-pixel halo the same read is held
    assert not counted(50, 7.0 / 120.0, 120, held_region(b, 2, 16))
    # a static pixel in the middle of the strip is never counted
    assert not counted(100, 0.0, 120, held)
    # near the edge the check may over-report (margin of one pixel and the half rounding), never under-report
    assert counted(52, 0.0, 120, (52, 120))         # the read is pixel 52 itself, but the margin reaches 51


# ---- the formula itself: does the range the check derives from a stored motion vector cover every read the pass can make? --------
def _all_halves():
    bits = np.arange(65536, dtype=np.uint32)
    with np.errstate(invalid="ignore"):                       # signalling NaN patterns
        return bits, ref.half_bits_to_f32(bits).astype(np.float64)


def _finite_halves_below_one():
    bits, v = _all_halves()
    keep = np.isfinite(v) & (np.abs(v) < 1.0)
    return bits[keep], v[keep]


def _rounding_interval(v):
    """[d_lo, d_hi]: every real that rounds (to nearest) to the half value v, its two ties included."""
    grid = np.unique(_all_halves()[1])
    grid = grid[np.isfinite(grid)]
    i = np.searchsorted(grid, v)
    assert (grid[i] == v).all()
    return (grid[i - 1] + v) / 2.0, (v + grid[i + 1]) / 2.0      # |v| < 1: both neighbours exist


@pytest.mark.parametrize("W", [1, 2, 7, 8, 64, 120, 1920, 3840, 16384])
def test_read_range_covers_every_read_of_the_ris_pass(W):
    """Float64 interval model of the RIS pass's temporal read (kernels.hip; oracle/orc_passes.cpp trace_ris) against the fp32
    restatement of the check. The pass computes prev_u in [0, 1), stores half(inUV - prev_u) with inUV = (p + 0.5) / W, and reads
    pixel (int)(prev_u * W + (j - 0.5)), j in [0, 1). From a stored half value the true difference lies in the half's rounding
    interval. fp32 allowance: W * 2^-21 pixels on prev_u * W, for the three fp32 roundings between the stored vector and the read
    (inUV - prev_u, prev_u * W, the jitter sum), each at most 2^-24 relative on a value of at most W pixels: 3 * W * 2^-24 <
    W * 2^-21. Every integer the read can produce inside the image must lie in the restatement's [lo, hi], and [lo, hi] reaches at
    most 3 + |mv| * W * 2^-9 pixels beyond those integers."""
    bits, v = _finite_halves_below_one()
    d_lo, d_hi = _rounding_interval(v)
    allowance = W * 2.0 ** -21
    min_slack, worst_over = None, 0.0
    for p in sorted({q for q in (0, 1, 2, W // 3, W // 2, W - 2, W - 1) if 0 <= q < W}):
        prev_lo = np.maximum((p + 0.5) - d_hi * W - allowance, 0.0)          # prev_u * W, within [0, W]
        prev_hi = np.minimum((p + 0.5) - d_lo * W + allowance, float(W))
        r_lo = np.maximum(np.trunc(prev_lo - 0.5), 0.0)                      # (int) truncates: (-1, 0) reads pixel 0
        r_hi = np.minimum(np.trunc(prev_hi + 0.5), W - 1.0)
        reads = (prev_lo <= prev_hi) & (r_lo <= r_hi)                        # this half can be stored here and reads inside the image
        kind, lo, hi = ref.reach_f32(bits, np.full(bits.shape, p), W, True)
        assert (kind == ref.IN_RANGE).all()
        missed = reads & ((lo > r_lo) | (hi < r_hi))
        assert not missed.any(), "W %d pixel %d: reads outside [lo, hi] for half patterns %s" % (
            W, p, ["0x%04x" % b for b in bits[missed][:8]])
        slack = np.minimum(r_lo - lo, hi - r_hi)[reads]
        over = (np.maximum(r_lo - lo, hi - r_hi) - (3.0 + np.abs(v) * W * 2.0 ** -9))[reads]
        assert (over <= 0.0).all(), "W %d pixel %d: [lo, hi] over-reports by more than 3 + |mv| W 2^-9 for %s" % (
            W, p, ["0x%04x" % b for b in bits[reads][over > 0.0][:8]])
        if slack.size:
            min_slack = slack.min() if min_slack is None else min(min_slack, slack.min())
            worst_over = max(worst_over, float(np.maximum(r_lo - lo, hi - r_hi)[reads].max()))
    print("W %d: smallest slack %s px, largest over-report %s px" % (W, min_slack, worst_over))
    assert min_slack is not None                                             # not vacuous: some half reads inside the image


def test_fp32_restatement_equals_hand_worked_restatement():
    """reach_counted_f32 (what the GPU tests compare the kernel with) and the scalar read_range / counted above agree wherever
    fp32 and float64 cannot differ: motion vectors that are multiples of 2^-7 in images 128 long (every product is exact)."""
    n = 128
    mvs = np.arange(-127, 128) / 128.0
    bits = np.float16(mvs).view(np.uint16).astype(np.uint32)
    for p in (0, 1, 63, 64, 126, 127):
        for held in ((0, n), (0, 0), (40, 90), (0, 64), (64, n)):
            got = ref.reach_counted_f32(bits, np.full(bits.shape, p), n, True, *held)
            want = np.array([counted(p, m, n, held) for m in mvs])
            assert (got == want).all(), (p, held, mvs[got != want])
            got_rows = ref.reach_counted_f32(bits << 16, np.full(bits.shape, p), n, False, *held)
            assert (got_rows == want).all(), (p, held)


# ---- sr_strip_pack / sr_strip_unpack / sr_history_reach_check refuse what their launchers assume ----------------------------------
IMG, PACKED, MOTION, COUNTER = 0x7000_0000_0000, 0x7000_0010_0000, 0x7000_0020_0000, 0x7000_0030_0000   # never dereferenced


def _refused(call, *args, **kw):
    with pytest.raises(_lib.SunrayError) as e:
        call(*args, stream=0, **kw)
    assert e.value.code == -1 and e.value.description, (args, kw)       # SR_ERR_INVALID_ARG before any launch (a launch: 0 or -2)
    return e.value.description


@pytest.mark.parametrize("call", [rt.strip_pack, rt.strip_unpack])
def test_strip_copy_rejects_bad_arguments(call):
    ok = [(IMG, 16), (IMG + 0x1000, 2)]
    size, rect = (64, 8), (8, 16, 2, 4)
    for n in (0, 6):
        assert "n_planes" in _refused(call, [(IMG, 4)] * n, size, rect, PACKED)
    for bpp in (0, 1, 3, 47):
        assert "bytes per pixel" in _refused(call, [(IMG, 16), (IMG, bpp)], size, rect, PACKED)
    assert "null" in _refused(call, [(IMG, 16), (0, 2)], size, rect, PACKED)
    assert "null" in _refused(call, ok, size, rect, 0)
    L = _lib.lib()
    fn = L.sr_strip_pack if call is rt.strip_pack else L.sr_strip_unpack
    assert fn(None, 2, 64, 8, 8, 16, 2, 4, C.c_void_p(PACKED), None) == -1 and b"null" in L.sr_last_error()
    for bad in ((56, 9, 0, 8), (64, 1, 0, 1), (0, 65, 0, 8), (0, 64, 5, 4), (0, 64, 8, 1), (0, 64, 0, 9),
                (0xFFFFFFFF, 2, 0, 1), (0, 1, 0xFFFFFFFF, 2), (0, 0, 0, 9), (65, 0, 0, 1)):
        assert "leaves the image" in _refused(call, ok, size, bad, PACKED)
    assert "extent" in _refused(call, ok, (0, 8), (0, 0, 0, 0), PACKED)
    assert "extent" in _refused(call, ok, (65536, 32768), rect, PACKED)
    for off in (2, 4, 8):
        assert "aligned" in _refused(call, [(IMG, 16), (IMG + off, 2)], size, rect, PACKED)
        assert "aligned" in _refused(call, ok, size, rect, PACKED + off)
    for empty in ((8, 0, 2, 4), (8, 16, 2, 0), (64, 0, 8, 0)):              # an empty rectangle inside the image: a no-op
        call(ok, size, empty, PACKED, stream=0)


def test_history_reach_check_rejects_bad_arguments():
    size, rect = (64, 8), (8, 16, 2, 4)
    cols, rows = abi.AXIS_COLS, abi.AXIS_ROWS
    chk = rt.history_reach_check
    assert "null" in _refused(chk, 0, size, cols, rect, (0, 64), COUNTER)
    assert "null" in _refused(chk, MOTION, size, cols, rect, (0, 64), 0)
    assert "aligned" in _refused(chk, MOTION + 2, size, cols, rect, (0, 64), COUNTER)
    assert "aligned" in _refused(chk, MOTION, size, cols, rect, (0, 64), COUNTER + 4)
    assert "axis" in _refused(chk, MOTION, size, 2, rect, (0, 8), COUNTER)
    for bad in ((56, 9, 0, 8), (0, 64, 5, 4), (0xFFFFFFFF, 2, 0, 1), (0, 1, 0xFFFFFFFF, 2), (65, 0, 0, 1)):
        assert "leaves the image" in _refused(chk, MOTION, size, cols, bad, (0, 64), COUNTER)
    assert "extent" in _refused(chk, MOTION, (64, 0), cols, (0, 0, 0, 0), (0, 0), COUNTER)
    for axis, held in ((cols, (9, 8)), (cols, (0, 65)), (cols, (65, 65)), (rows, (0, 9)), (rows, (5, 4)), (rows, (0, 64))):
        assert "held" in _refused(chk, MOTION, size, axis, rect, held, COUNTER)
    for empty in ((8, 0, 2, 4), (8, 16, 2, 0)):
        chk(MOTION, size, cols, empty, (0, 64), COUNTER, stream=0)
        chk(MOTION, size, rows, empty, (8, 8), COUNTER, stream=0)


def test_strip_packed_bytes_equals_the_model():
    for bpps in ([2], [16, 2, 4, 4, 4], [48, 48], [8, 2], [4, 4, 4]):
        for w, h in ((1, 1), (3, 1), (7, 9), (65, 3), (200, 9), (0, 5), (5, 0)):
            assert rt.strip_packed_bytes(bpps, w, h) == ref.packed_layout(bpps, w, h)[1], (bpps, w, h)
    L, n = _lib.lib(), C.c_uint64()
    planes = (abi.SrStripPlane * 6)()
    for p in planes:
        p.bpp = 4
    assert L.sr_strip_packed_bytes(planes, 6, 4, 4, C.byref(n)) == -1
    assert L.sr_strip_packed_bytes(planes, 0, 4, 4, C.byref(n)) == -1
    assert L.sr_strip_packed_bytes(planes, 2, 4, 4, None) == -1
    assert L.sr_strip_packed_bytes(None, 2, 4, 4, C.byref(n)) == -1
    planes[1].bpp = 3
    assert L.sr_strip_packed_bytes(planes, 2, 4, 4, C.byref(n)) == -1 and b"bytes per pixel" in L.sr_last_error()
