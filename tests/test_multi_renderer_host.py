"""CPU-side checks of the multi-device renderer's C ABI (sr_renderer_create_multi and friends): argument errors, the no-GPU
failure, and a restatement of the history-reach check's held region and read range (strip_copy.hip) on hand-worked cases."""
import ctypes as C
import math

import numpy as np
import pytest

from sunray_amd import _lib, runtime as rt

SPATIAL_HALO = 30


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


# ---- restatement of history_reach_check_kernel (strip_copy.hip) -------------------------------------------------------------
def held_region(bounds, slot, motion_halo):
    """[lo, hi) along the axis a slot holds exact history for: its strip grown by SR_SPATIAL_HALO + motion_halo, clipped."""
    length = bounds[-1]
    grow = SPATIAL_HALO + motion_halo
    return max(bounds[slot] - grow, 0), min(bounds[slot + 1] + grow, length)


def read_range(p, mv, n):
    """Conservative [lo, hi] pixel range of the temporal read of pixel p (index along the axis) whose stored half-precision motion
    component is mv, in an image n pixels long; None when the range lies outside the image."""
    m = float(np.float32(np.float16(mv)))
    c = (p + 0.5) - m * n
    e = abs(m) * n / 1024.0 + 1.0
    lo, hi = max(math.floor(c - e - 0.5), 0), min(math.ceil(c + e + 0.5), n - 1)
    return (lo, hi) if lo <= hi else None


def counted(p, mv, n, held):
    r = read_range(p, mv, n)
    return r is not None and (r[0] < held[0] or r[1] >= held[1])


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
