"""CPU-side checks of skinning (sr_scene_set_mesh_skin / sr_scene_skin_mesh / sr_scene_mesh_skin_info and their renderer forms):
the symbols load, the structs have their documented size and field order, null arguments fail with a message, the Python wrappers
refuse wrong dtypes and shapes before the library is called, and the compiler's report lists the kernel without scratch."""
import ctypes as C

import numpy as np
import pytest

from sunray_amd import _lib, abi, runtime

NEW_SYMBOLS = ("sr_scene_set_mesh_skin", "sr_scene_skin_mesh", "sr_scene_mesh_skin_info", "sr_renderer_set_mesh_skin", "sr_renderer_skin_mesh")


def test_skin_symbols_load_and_structs_hold():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrSkinInfluence) == 24 and abi.SKIN_INFLUENCE.itemsize == 24
    assert [f[0] for f in abi.SrSkinInfluence._fields_] == ["joint", "weight"] and abi.SrSkinInfluence.weight.offset == 8
    assert abi.SKIN_INFLUENCE.names == ("joint", "weight") and abi.SKIN_INFLUENCE.fields["weight"][1] == 8
    assert C.sizeof(abi.SrMeshSkinInfo) == 24
    assert [f[0] for f in abi.SrMeshSkinInfo._fields_] == ["n_joints", "skinned", "first_bad", "_pad", "skin_ms"]
    assert abi.SrMeshSkinInfo.skin_ms.offset == 16
    # symbols were added, no struct changed
    assert L.sr_version() == 1 and C.sizeof(abi.SrMeshVertexInfo) == 40 and C.sizeof(abi.SrMeshUpdateInfo) == 64 and abi.VERTEX.itemsize == 96


def test_skin_null_arguments_fail_with_a_message():
    L = _lib.lib()
    inf = np.zeros(3, dtype=abi.SKIN_INFLUENCE)
    mats = np.zeros((1, 12), dtype=np.float32)
    ip, mp = inf.ctypes.data_as(C.c_void_p), mats.ctypes.data_as(C.c_void_p)
    assert L.sr_scene_set_mesh_skin(None, C.c_uint64(1), ip, C.c_uint32(3), C.c_uint32(1)) == -1
    assert b"set_mesh_skin" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_skin_mesh(None, C.c_uint64(1), mp, C.c_uint32(1), None) == -1
    assert b"skin_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_skin_mesh(C.c_void_p(0x10), C.c_uint64(1), None, C.c_uint32(1), None) == -1     # the scene is never looked at
    assert b"skin_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    info = abi.SrMeshSkinInfo()
    assert L.sr_scene_mesh_skin_info(None, C.c_uint64(1), C.byref(info)) == -1 and b"sr_scene_mesh_skin_info" in L.sr_last_error()
    assert L.sr_scene_mesh_skin_info(C.c_void_p(0x10), C.c_uint64(1), None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_renderer_set_mesh_skin(None, C.c_uint64(1), ip, C.c_uint32(3), C.c_uint32(1)) == -1
    assert b"set_mesh_skin" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_renderer_skin_mesh(None, C.c_uint64(1), mp, C.c_uint32(1), None) == -1
    assert b"skin_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Handle:
    """A Scene / Renderer shell with no native object behind it."""
    _h = C.c_void_p(0x10)
    device_index = 0
    devices = [0]

    @staticmethod
    def _stream():
        raise AssertionError("the stream was asked for")


@pytest.mark.parametrize("method", [runtime.Scene.set_mesh_skin, runtime.Renderer.set_mesh_skin])
def test_set_mesh_skin_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    n = 5
    cases = {
        "float array of the right byte count": np.zeros((n, 6), dtype=np.float32),
        "bytes": np.zeros(n * 24, dtype=np.uint8),
        "a list of tuples": [((0, 0, 0, 0), (1.0, 0.0, 0.0, 0.0))] * n,
        "joints as u4": np.zeros(n, dtype=np.dtype([("joint", "<u4", 4), ("weight", "<f4", 4)])),
        "weights as f8": np.zeros(n, dtype=np.dtype([("joint", "<u2", 4), ("weight", "<f8", 4)])),
        "two dimensions": np.zeros((n, 2), dtype=abi.SKIN_INFLUENCE),
        "no dimension": np.zeros((), dtype=abi.SKIN_INFLUENCE),
        "empty": np.zeros(0, dtype=abi.SKIN_INFLUENCE),
    }
    for what, a in cases.items():
        with pytest.raises(ValueError):
            method(_Handle(), 7, a, 3)


@pytest.mark.parametrize("method", [runtime.Scene.skin_mesh, runtime.Renderer.skin_mesh])
def test_skin_mesh_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    n = 4
    cases = {
        "float64 matrices": np.zeros((n, 12), dtype=np.float64),
        "4x4 matrices": np.zeros((n, 4, 4), dtype=np.float32),
        "flat floats": np.zeros(n * 12, dtype=np.float32),
        "(n, 4, 3)": np.zeros((n, 4, 3), dtype=np.float32),
        "a list": [[1.0] * 12] * n,
        "no joints": np.zeros((0, 12), dtype=np.float32),
        "transform records in two dimensions": np.zeros((n, 1), dtype=abi.TRANSFORM),
        "integers": np.zeros((n, 12), dtype=np.int32),
    }
    for what, a in cases.items():
        with pytest.raises(ValueError):
            method(_Handle(), 7, a)


def test_skin_kernel_is_in_the_resource_report():
    """The compiler's report for pose_batch.hip, whose pose_batch_kernel skins (sr_scene_skin_mesh is a batch of one item), is kept
    next to the object: the kernel needs no scratch and spills nothing; its LDS is the tile of 256 vertices, seven 16-byte slots each."""
    from sunray_amd import build
    res = build.kernel_resources("pose_batch.hip")
    mine = [r for name, r in res.items() if "pose_batch_kernel" in name]
    assert len(mine) == 1, sorted(res)
    assert mine[0]["scratch"] == 0 and mine[0]["vgpr_spills"] == 0 and mine[0]["sgpr_spills"] == 0, mine[0]
    assert mine[0]["lds"] == 256 * 7 * 16 and mine[0]["occupancy"] >= 4, mine[0]
    assert any("vertex_check_kernel" in name for name in build.kernel_resources("bvh_gpu.hip"))      # that report is still its own
