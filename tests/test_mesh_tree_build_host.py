"""Host-side checks of the device mesh-tree build's public interface (sr_scene_set_mesh_tree_build, sr_scene_mesh_tree_info,
sr_renderer_set_mesh_tree_build): the exports exist and reject bad arguments, the Python mirror of the header's struct and
constants is pinned, SrMeshUpdateInfo keeps its size. Nothing here needs a GPU; that SR_BLAS_BUILD is read when a scene is created
needs a scene, and no entry point creates one without a device, so every spelling of it is checked in
tests/test_gpu_mesh_tree_build.py (test_fallbacks_name_their_reason_and_equal_the_oracle)."""
import ctypes as C
import os
import re

from sunray_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_ERR_INVALID_ARG = -1
NEW = ("sr_scene_set_mesh_tree_build", "sr_scene_mesh_tree_info", "sr_renderer_set_mesh_tree_build")


def header():
    return open(os.path.join(ROOT, "include", "sunray_hip.h")).read()


def test_exports_exist_and_reject_null_and_bad_modes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    for mode in (abi.MESH_TREE_BUILD_AUTO, abi.MESH_TREE_BUILD_HOST, abi.MESH_TREE_BUILD_DEVICE, 3, 0xFFFFFFFF):
        # the mode is checked before the handle: a bad mode is refused as such, a good one gets as far as the null handle
        what = b"mode must be" if mode > abi.MESH_TREE_BUILD_DEVICE else b"is null"
        assert L.sr_scene_set_mesh_tree_build(None, C.c_uint32(mode)) == SR_ERR_INVALID_ARG
        assert b"sr_scene_set_mesh_tree_build" in L.sr_last_error() and what in L.sr_last_error()
        assert L.sr_renderer_set_mesh_tree_build(None, C.c_uint32(mode)) == SR_ERR_INVALID_ARG
        assert b"sr_renderer_set_mesh_tree_build" in L.sr_last_error() and what in L.sr_last_error()
    info = abi.SrMeshTreeInfo()
    assert L.sr_scene_mesh_tree_info(None, C.byref(info)) == SR_ERR_INVALID_ARG
    assert L.sr_scene_mesh_tree_info(None, None) == SR_ERR_INVALID_ARG
    assert b"sr_scene_mesh_tree_info" in L.sr_last_error()


def test_mesh_tree_info_struct_and_constants_match_the_header():
    h = header()
    body = re.search(r"typedef struct SrMeshTreeInfo \{(.*?)\} SrMeshTreeInfo;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
    assert [(n, {"uint32_t": C.c_uint32, "double": C.c_double}[t]) for t, n in fields] == list(abi.SrMeshTreeInfo._fields_)
    assert C.sizeof(abi.SrMeshTreeInfo) == 40 and abi.SrMeshTreeInfo.reason.offset == 16 and abi.SrMeshTreeInfo.device_build_ms.offset == 32
    defines = {k: int(v) for k, v in re.findall(r"#define (SR_MESH_TREE_\w+) (\d+)u", h)}
    assert (defines["SR_MESH_TREE_BUILD_AUTO"], defines["SR_MESH_TREE_BUILD_HOST"], defines["SR_MESH_TREE_BUILD_DEVICE"]) == \
        (abi.MESH_TREE_BUILD_AUTO, abi.MESH_TREE_BUILD_HOST, abi.MESH_TREE_BUILD_DEVICE) == (0, 1, 2)
    for name in ("ON_DEVICE", "HOST_MODE", "HOST_BELOW_THRESHOLD", "HOST_SLOW_BUILD", "HOST_BAKED_INSTANCE", "HOST_NOT_RESIDENT", "HOST_STACK_BUDGET",
                 "HOST_STATIC_MESH"):
        assert defines["SR_MESH_TREE_" + name] == getattr(abi, "MESH_TREE_" + name), name
    assert len(defines) == 11


def test_update_info_keeps_its_64_bytes_and_the_version_stands():
    assert C.sizeof(abi.SrMeshUpdateInfo) == 64 and abi.SrMeshUpdateInfo.blas_rebuilt.offset == 8 and abi.SrMeshUpdateInfo.blas_build_ms.offset == 56
    body = re.search(r"typedef struct SrMeshUpdateInfo \{(.*?)\} SrMeshUpdateInfo;", header(), re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in abi.SrMeshUpdateInfo._fields_]
    assert _lib.lib().sr_version() == 1             # symbols and a struct were added: no layout changed


def test_no_sentence_denies_the_device_builder_any_more():
    for path in ("sunray_amd/csrc/api.cpp", "include/sunray_hip.h", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "no device builder for mesh trees" not in text and "no device fast build for mesh trees" not in text, path
