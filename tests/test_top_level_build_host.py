"""Host-side checks of the device top-level build's public interface (sr_scene_set_top_level_build, sr_scene_top_level_info,
sr_scene_read_top_level): the exports exist and reject bad arguments, and the Python mirror of the header's struct and
constants is pinned. Nothing here needs a GPU; that SR_TL_BUILD is read when a scene is created needs a scene, so it is checked
in tests/test_gpu_top_level_build.py."""
import ctypes as C
import os
import re

import numpy as np

from sunray_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_ERR_INVALID_ARG = -1


def header():
    return open(os.path.join(ROOT, "include", "sunray_hip.h")).read()


def test_invalid_arg_code_is_the_headers():
    assert int(re.search(r"\bSR_ERR_INVALID_ARG\s*=\s*(-?\d+)", header()).group(1)) == SR_ERR_INVALID_ARG


def test_exports_exist_and_reject_null_and_bad_modes():
    L = _lib.lib()
    for name in ("sr_scene_set_top_level_build", "sr_scene_top_level_info", "sr_scene_read_top_level"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    info = abi.SrTopLevelInfo()
    for mode in (abi.TL_BUILD_AUTO, abi.TL_BUILD_HOST, abi.TL_BUILD_DEVICE, 3, 0xFFFFFFFF):
        assert L.sr_scene_set_top_level_build(None, C.c_uint32(mode)) == SR_ERR_INVALID_ARG
    assert b"sr_scene_set_top_level_build" in L.sr_last_error()
    assert L.sr_scene_top_level_info(None, C.byref(info)) == SR_ERR_INVALID_ARG
    assert L.sr_scene_top_level_info(None, None) == SR_ERR_INVALID_ARG
    assert b"sr_scene_top_level_info" in L.sr_last_error()
    buf = np.zeros(64, dtype=np.uint32)
    assert L.sr_scene_read_top_level(None, buf.ctypes.data_as(C.c_void_p), None, None, None) == SR_ERR_INVALID_ARG
    assert L.sr_scene_read_top_level(None, None, None, None, None) == SR_ERR_INVALID_ARG
    assert b"sr_scene_read_top_level" in L.sr_last_error() and not buf.any()


def test_top_level_info_struct_and_constants_match_the_header():
    h = header()
    body = re.search(r"typedef struct SrTopLevelInfo \{(.*?)\} SrTopLevelInfo;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
    assert [(n, {"uint32_t": C.c_uint32, "double": C.c_double}[t]) for t, n in fields] == list(abi.SrTopLevelInfo._fields_)
    assert C.sizeof(abi.SrTopLevelInfo) == 64 and abi.SrTopLevelInfo.records_ms.offset == 40 and abi.SrTopLevelInfo.build_ms.offset == 56
    assert abi.TL_INSTANCE.itemsize == 128                       # DevTlInstance, csrc/traverse.h
    assert abi.TL_INSTANCE.fields["blas_root"][1] == 96 and abi.TL_INSTANCE.fields["flags"][1] == 120
    defines = {k: int(v) for k, v in re.findall(r"#define (SR_TL_\w+) (\d+)u", h)}
    assert (defines["SR_TL_BUILD_AUTO"], defines["SR_TL_BUILD_HOST"], defines["SR_TL_BUILD_DEVICE"]) == (abi.TL_BUILD_AUTO, abi.TL_BUILD_HOST, abi.TL_BUILD_DEVICE)
    for name in ("ON_DEVICE", "HOST_MODE", "HOST_BELOW_THRESHOLD", "HOST_BAKED_INSTANCE", "HOST_STACK_BUDGET", "HOST_NOT_TWO_LEVEL", "HOST_TOO_FEW",
                 "HOST_QUALITY_BUILD"):
        assert defines["SR_TL_" + name] == getattr(abi, "TL_" + name), name
    assert len(defines) == 11
