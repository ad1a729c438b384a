"""CPU-side checks of the in-place mesh update (sr_scene_update_mesh / sr_renderer_update_mesh, the reference's Blas::update,
acceleration_structure/blas.rs:285-310): the symbols load, null arguments fail with a message, and the deformation helper that
the GPU tests and the measurement script share is deterministic and keeps what an update must keep."""
import ctypes as C

import numpy as np

from sunray_amd import _lib, abi, scenes


def test_update_mesh_symbols_load():
    L = _lib.lib()
    for name in ("sr_scene_update_mesh", "sr_scene_mesh_update_info", "sr_renderer_update_mesh"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrMeshUpdateInfo) == 64
    assert L.sr_version() == 1                      # a symbol was added, no struct changed


def test_update_mesh_null_arguments_fail_with_a_message():
    L = _lib.lib()
    v = np.zeros(3, dtype=abi.VERTEX)
    p = v.ctypes.data_as(C.c_void_p)
    assert L.sr_scene_update_mesh(None, C.c_uint64(1), p, C.c_uint32(3)) == -1
    assert b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_renderer_update_mesh(None, C.c_uint64(1), p, C.c_uint32(3)) == -1
    assert b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    info = abi.SrMeshUpdateInfo()
    assert L.sr_scene_mesh_update_info(None, C.byref(info)) == -1 and b"sr_scene_mesh_update_info" in L.sr_last_error()


def test_deformation_helper_is_deterministic_and_keeps_the_topology():
    for desc, keys in ((scenes.instanced_field(12), [1, 2]), (scenes.cornell_glass_mirror(), [7]), (scenes.atrium(4, 12, 4, 4, 16, 2), [1, 6])):
        before = [m.vertices.tobytes() for m in desc.meshes]
        a, b = scenes.deform(desc, keys, 2.5), scenes.deform(desc, keys, 2.5)
        c = scenes.deform(desc, keys, 3.5)
        assert [m.key for m in a.meshes] == [m.key for m in desc.meshes] and a.instances is desc.instances
        for m0, ma, mb, mc in zip(desc.meshes, a.meshes, b.meshes, c.meshes):
            if m0.key not in keys:
                assert ma is m0                                               # untouched meshes are shared, not copied
                continue
            assert ma.vertices.tobytes() == mb.vertices.tobytes()             # same (mesh, phase) -> same bytes
            assert ma.vertices.tobytes() != mc.vertices.tobytes() and ma.vertices.tobytes() != m0.vertices.tobytes()
            assert ma.indices is m0.indices and ma.material is m0.material and len(ma.vertices) == len(m0.vertices)
            assert ma.vertices.dtype == abi.VERTEX and np.isfinite(ma.vertices["position"]).all()
            assert not np.array_equal(ma.vertices["position"], m0.vertices["position"])
            assert not np.array_equal(ma.vertices["normal"], m0.vertices["normal"])
            assert np.allclose(np.linalg.norm(ma.vertices["normal"], axis=1), 1.0, atol=1e-5)
            if m0.vertices["tangent"].any():                                  # textured meshes: uvs and tangents change too
                assert not np.array_equal(ma.vertices["tangent"], m0.vertices["tangent"])
                assert np.array_equal(ma.vertices["tangent"][:, 3], m0.vertices["tangent"][:, 3])
                assert not np.array_equal(ma.vertices["normal_tex_coord"], m0.vertices["normal_tex_coord"])
        assert before == [m.vertices.tobytes() for m in desc.meshes]          # the input is not modified
