"""CPU-side checks of morph targets (sr_scene_set_mesh_morph / sr_scene_pose_mesh / sr_scene_mesh_morph_info, their renderer forms
and the loader's read-outs): the symbols load, the structs have their documented size and field order, null arguments fail with a
message, the Python wrappers refuse wrong dtypes and shapes before the library is called, and the compiler's report lists the
kernel without scratch."""
import ctypes as C

import numpy as np
import pytest

from sunray_amd import _lib, abi, runtime

NEW_SYMBOLS = ("sr_scene_set_mesh_morph", "sr_scene_pose_mesh", "sr_scene_mesh_morph_info", "sr_renderer_set_mesh_morph", "sr_renderer_pose_mesh",
               "sr_gltf_blas_morph", "sr_gltf_morph_weights", "sr_renderer_attach_morphs")


def test_morph_symbols_load_and_structs_hold():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrMorphDelta) == 48 and abi.MORPH_DELTA.itemsize == 48
    assert [f[0] for f in abi.SrMorphDelta._fields_] == ["position", "_pad0", "normal", "_pad1", "tangent", "_pad2"]
    assert (abi.SrMorphDelta.position.offset, abi.SrMorphDelta.normal.offset, abi.SrMorphDelta.tangent.offset) == (0, 16, 32)
    assert abi.MORPH_DELTA.names == ("position", "_pad0", "normal", "_pad1", "tangent", "_pad2")
    assert [abi.MORPH_DELTA.fields[n][1] for n in ("position", "normal", "tangent")] == [0, 16, 32]
    # the three pieces lie where the first three pieces of a vertex lie
    assert [abi.VERTEX.fields[n][1] for n in ("position", "normal", "tangent")] == [0, 16, 32]
    assert C.sizeof(abi.SrMeshMorphInfo) == 24
    assert [f[0] for f in abi.SrMeshMorphInfo._fields_] == ["n_targets", "posed", "n_active", "first_bad", "morph_ms"]
    assert abi.SrMeshMorphInfo.morph_ms.offset == 16
    # symbols were added, no struct changed
    assert L.sr_version() == 1 and C.sizeof(abi.SrMeshSkinInfo) == 24 and C.sizeof(abi.SrSkinInfluence) == 24 and abi.VERTEX.itemsize == 96


def test_morph_null_arguments_fail_with_a_message():
    L = _lib.lib()
    deltas = np.zeros((2, 3), dtype=abi.MORPH_DELTA)
    w, mats = np.zeros(2, dtype=np.float32), np.zeros((1, 12), dtype=np.float32)
    dp, wp, mp = (a.ctypes.data_as(C.c_void_p) for a in (deltas, w, mats))
    scene = C.c_void_p(0x10)                                             # never looked at where a null argument decides
    assert L.sr_scene_set_mesh_morph(None, C.c_uint64(1), dp, C.c_uint32(3), C.c_uint32(2)) == -1
    assert b"set_mesh_morph" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_pose_mesh(None, C.c_uint64(1), wp, C.c_uint32(2), mp, C.c_uint32(1), None) == -1
    assert b"pose_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_pose_mesh(scene, C.c_uint64(1), None, C.c_uint32(2), None, C.c_uint32(1), None) == -1
    assert b"pose_mesh" in L.sr_last_error() and b"neither" in L.sr_last_error()
    info = abi.SrMeshMorphInfo()
    assert L.sr_scene_mesh_morph_info(None, C.c_uint64(1), C.byref(info)) == -1 and b"sr_scene_mesh_morph_info" in L.sr_last_error()
    assert L.sr_scene_mesh_morph_info(scene, C.c_uint64(1), None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_renderer_set_mesh_morph(None, C.c_uint64(1), dp, C.c_uint32(3), C.c_uint32(2)) == -1
    assert b"set_mesh_morph" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_renderer_pose_mesh(None, C.c_uint64(1), wp, C.c_uint32(2), None, C.c_uint32(0), None) == -1
    assert b"pose_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    for args in ((None, scene, scene), (scene, None, scene), (scene, scene, None)):
        assert L.sr_renderer_attach_morphs(*args) == -1 and b"attach_morphs" in L.sr_last_error() and b"null" in L.sr_last_error()
    n = C.c_uint32()
    assert L.sr_gltf_blas_morph(None, C.c_uint32(0), C.byref(n), None, None, None) == -1 and b"sr_gltf_blas_morph" in L.sr_last_error()
    assert L.sr_gltf_morph_weights(None, C.c_int32(-1), C.c_float(0.0), C.c_uint32(0), wp, C.c_uint32(2)) == -1
    assert b"sr_gltf_morph_weights" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_gltf_morph_weights(scene, C.c_int32(-1), C.c_float(0.0), C.c_uint32(0), None, C.c_uint32(2)) == -1 and b"null" in L.sr_last_error()
    assert L.sr_gltf_morph_weights(scene, C.c_int32(-2), C.c_float(0.0), C.c_uint32(0), wp, C.c_uint32(2)) == -1 and b"-1" in L.sr_last_error()


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


@pytest.mark.parametrize("method", [runtime.Scene.set_mesh_morph, runtime.Renderer.set_mesh_morph])
def test_set_mesh_morph_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    t, n = 3, 5
    cases = {
        "float array of the right byte count": np.zeros((t, n, 12), dtype=np.float32),
        "bytes": np.zeros((t, n * 48), dtype=np.uint8),
        "vertex records": np.zeros((t, n), dtype=abi.VERTEX),
        "a list": [[(0.0,) * 12] * n] * t,
        "positions as f8": np.zeros((t, n), dtype=np.dtype([(name, "<f8" if name == "position" else "<f4", 3) if not name.startswith("_") else (name, "<f4")
                                                          for name in abi.MORPH_DELTA.names])),
        "one dimension": np.zeros(t * n, dtype=abi.MORPH_DELTA),
        "three dimensions": np.zeros((t, n, 1), dtype=abi.MORPH_DELTA),
        "no targets": np.zeros((0, n), dtype=abi.MORPH_DELTA),
        "no vertices": np.zeros((t, 0), dtype=abi.MORPH_DELTA),
    }
    for what, a in cases.items():
        with pytest.raises(ValueError):
            method(_Handle(), 7, a)


@pytest.mark.parametrize("method", [runtime.Scene.pose_mesh, runtime.Renderer.pose_mesh])
def test_pose_mesh_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    good_w, good_m = np.zeros(3, dtype=np.float32), np.zeros((2, 12), dtype=np.float32)
    cases = {
        "float64 weights": (np.zeros(3, dtype=np.float64), None),
        "a list of weights": ([0.0, 1.0, 0.5], None),
        "weights in two dimensions": (np.zeros((3, 1), dtype=np.float32), None),
        "no weights": (np.zeros(0, dtype=np.float32), None),
        "integer weights": (np.zeros(3, dtype=np.int32), good_m),
        "good weights, float64 matrices": (good_w, np.zeros((2, 12), dtype=np.float64)),
        "good weights, 4x4 matrices": (good_w, np.zeros((2, 4, 4), dtype=np.float32)),
        "no weights given, flat matrices": (None, np.zeros(24, dtype=np.float32)),
        "neither stage": (None, None),
    }
    for what, (w, m) in cases.items():
        with pytest.raises(ValueError):
            method(_Handle(), 7, w, m)


def test_morph_kernel_is_in_the_resource_report():
    """The compiler's report for pose_batch.hip, whose pose_batch_kernel morphs (sr_scene_pose_mesh is a batch of one item), is kept
    next to the object: the kernel needs no scratch and spills nothing; its LDS is the tile of 256 vertices, seven 16-byte slots each."""
    from sunray_amd import build
    res = build.kernel_resources("pose_batch.hip")
    mine = [r for name, r in res.items() if "pose_batch_kernel" in name]
    assert len(mine) == 1, sorted(res)
    assert mine[0]["scratch"] == 0 and mine[0]["vgpr_spills"] == 0 and mine[0]["sgpr_spills"] == 0, mine[0]
    assert mine[0]["lds"] == 256 * 7 * 16 and mine[0]["occupancy"] >= 4, mine[0]
    assert any("vertex_frame_kernel" in name for name in build.kernel_resources("normals.hip"))      # that report is still its own
