"""Host-side checks of the tree height bound's public interface (sr_scene_set_tree_height_bound, sr_scene_tree_height_info,
sr_renderer_set_tree_height_bound): the exports exist and reject bad arguments by name, the Python mirror of the header's struct
and constants is pinned, the version stands. Nothing here needs a GPU; what the switch does to a build is checked in
tests/test_gpu_tree_height_bound.py."""
import ctypes as C
import os
import re

from sunray_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_ERR_INVALID_ARG = -1
NEW = ("sr_scene_set_tree_height_bound", "sr_scene_tree_height_info", "sr_renderer_set_tree_height_bound")


def header():
    return open(os.path.join(ROOT, "include", "sunray_hip.h")).read()


def test_exports_exist_and_reject_bad_arguments_by_name():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    # (mode, cap) -> what the message says; mode and cap are checked before the handle, so a good pair gets as far as the null handle
    cases = [((0, 0), b"is null"), ((1, 0), b"is null"), ((1, 1), b"is null"), ((1, 26), b"is null"),
             ((2, 0), b"mode must be"), ((0xFFFFFFFF, 0), b"mode must be"), ((1, 27), b"mesh_tree_cap"), ((1, 0xFFFFFFFF), b"mesh_tree_cap"),
             ((0, 1), b"mesh_tree_cap"), ((0, 26), b"mesh_tree_cap")]
    for (mode, cap), what in cases:
        for name in ("sr_scene_set_tree_height_bound", "sr_renderer_set_tree_height_bound"):
            assert getattr(L, name)(None, C.c_uint32(mode), C.c_uint32(cap)) == SR_ERR_INVALID_ARG, (name, mode, cap)
            err = L.sr_last_error()
            assert name.encode() in err and what in err, (name, mode, cap, err)
    info = abi.SrTreeHeightInfo()
    for kind in (abi.TREE_KIND_ONE_LEVEL, abi.TREE_KIND_TOP_LEVEL, abi.TREE_KIND_MESH, 3, 0xFFFFFFFF):
        assert L.sr_scene_tree_height_info(None, C.c_uint32(kind), C.byref(info)) == SR_ERR_INVALID_ARG
        err = L.sr_last_error()
        assert b"sr_scene_tree_height_info" in err and (b"kind must be" if kind > abi.TREE_KIND_MESH else b"null") in err, (kind, err)
    assert L.sr_scene_tree_height_info(None, C.c_uint32(0), None) == SR_ERR_INVALID_ARG
    assert b"sr_scene_tree_height_info" in L.sr_last_error()


def test_height_info_struct_and_constants_match_the_header():
    h = header()
    body = re.search(r"typedef struct SrTreeHeightInfo \{(.*?)\} SrTreeHeightInfo;", h, re.S).group(1)
    fields = []
    for names in re.findall(r"^\s*uint32_t\s+([\w,\s]+);", body, re.M):
        fields += [(n.strip(), C.c_uint32) for n in names.split(",")]
    assert fields == list(abi.SrTreeHeightInfo._fields_)
    assert C.sizeof(abi.SrTreeHeightInfo) == 32 and abi.SrTreeHeightInfo.on_device.offset == 8 and abi.SrTreeHeightInfo.prims_rebuilt.offset == 28
    defines = {k: int(v) for k, v in re.findall(r"#define (SR_(?:HEIGHT_BOUND|TREE_KIND)_\w+) (\d+)u", h)}
    assert defines == {"SR_HEIGHT_BOUND_REFUSE": abi.HEIGHT_BOUND_REFUSE, "SR_HEIGHT_BOUND_REBALANCE": abi.HEIGHT_BOUND_REBALANCE,
                       "SR_TREE_KIND_ONE_LEVEL": abi.TREE_KIND_ONE_LEVEL, "SR_TREE_KIND_TOP_LEVEL": abi.TREE_KIND_TOP_LEVEL,
                       "SR_TREE_KIND_MESH": abi.TREE_KIND_MESH}
    assert (abi.HEIGHT_BOUND_REFUSE, abi.HEIGHT_BOUND_REBALANCE) == (0, 1)
    assert (abi.TREE_KIND_ONE_LEVEL, abi.TREE_KIND_TOP_LEVEL, abi.TREE_KIND_MESH) == (0, 1, 2)


def test_the_version_stands():
    assert _lib.lib().sr_version() == 1             # symbols and a struct were added: no layout changed
