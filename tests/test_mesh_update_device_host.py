"""CPU-side checks of the device-pointer mesh update (sr_scene_update_mesh_device / sr_renderer_update_mesh_device and the
read-out sr_scene_mesh_vertex_info): the symbols load, the read-out struct has its documented size, null arguments fail with a
message, and the Python wrappers refuse what is no device tensor of whole vertices before the library is called."""
import ctypes as C

import numpy as np
import pytest
import torch

from sunray_amd import _lib, abi, runtime

NEW_SYMBOLS = ("sr_scene_update_mesh_device", "sr_scene_mesh_vertex_info", "sr_renderer_update_mesh_device")


def test_device_update_symbols_load():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrMeshVertexInfo) == 40
    assert [f[0] for f in abi.SrMeshVertexInfo._fields_] == ["host_stale", "last_from_device", "host_fetches", "_pad", "check_ms", "copy_ms", "fetch_ms"]
    assert abi.SrMeshVertexInfo.check_ms.offset == 16
    assert C.sizeof(abi.SrMeshUpdateInfo) == 64 and L.sr_version() == 1      # symbols were added, no struct changed


def test_device_update_null_arguments_fail_with_a_message():
    L = _lib.lib()
    fake_scene, fake_vertices = C.c_void_p(0), C.c_void_p(0x1000)
    # a null scene and a null renderer, with a pointer that is never looked at
    assert L.sr_scene_update_mesh_device(fake_scene, C.c_uint64(1), fake_vertices, C.c_uint32(3), None) == -1
    assert b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_renderer_update_mesh_device(None, C.c_uint64(1), fake_vertices, C.c_uint32(3), None) == -1
    assert b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    info = abi.SrMeshVertexInfo()
    assert L.sr_scene_mesh_vertex_info(None, C.c_uint64(1), C.byref(info)) == -1 and b"sr_scene_mesh_vertex_info" in L.sr_last_error()


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


class _Handle:
    """A Scene / Renderer shell with no native object behind it."""
    _h = C.c_void_p(0x10)
    device_index = 0
    devices = [0]


def _fake_device_tensor(nbytes, contiguous=True, index=0):
    """What the wrappers look at of a tensor, claiming to be on cuda:`index` (this machine may have no GPU)."""
    class T:
        is_cuda = True
        device = torch.device("cuda", index)

        def is_contiguous(self): return contiguous
        def numel(self): return nbytes
        def element_size(self): return 1
        def data_ptr(self): raise AssertionError("the address was taken")
    return T()


@pytest.mark.parametrize("method", [runtime.Scene.update_mesh_device, runtime.Renderer.update_mesh_device])
def test_python_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    h = _Handle()
    n = 5
    good_bytes = n * abi.VERTEX.itemsize
    cases = {
        "CPU tensor of the right size": torch.zeros(good_bytes, dtype=torch.uint8),
        "CPU float tensor": torch.zeros(good_bytes // 4, dtype=torch.float32),
        "numpy array": np.zeros(n, dtype=abi.VERTEX),
        "one byte short": _fake_device_tensor(good_bytes - 1),
        "one float over": _fake_device_tensor(good_bytes + 4),
        "empty": _fake_device_tensor(0),
        "gaps": _fake_device_tensor(good_bytes, contiguous=False),
        "another device": _fake_device_tensor(good_bytes, index=1),
    }
    for what, t in cases.items():
        with pytest.raises(ValueError):
            method(h, 7, t)


def test_vertex_check_kernel_is_in_the_resource_report():
    """The compiler's report for the builder kernels is kept next to the object like the pass kernels': the check kernel is
    bandwidth-bound and must need no LDS and no scratch."""
    from sunray_amd import build
    res = build.kernel_resources("bvh_gpu.hip")
    mine = [r for name, r in res.items() if "vertex_check_kernel" in name]
    assert len(mine) == 1, sorted(res)
    assert mine[0]["lds"] == 0 and mine[0]["scratch"] == 0 and mine[0]["vgpr_spills"] == 0 and mine[0]["sgpr_spills"] == 0, mine[0]
    assert any("blas_records_kernel" in name for name in res) and any("lbvh_collapse_kernel" in name for name in res)
