"""CPU-side checks of the per-mesh build type and the mesh-tree refit interface (sr_scene_set_mesh_build_type, sr_scene_mesh_as_state,
sr_scene_read_mesh_tree, sr_renderer_set_mesh_build_type; the reference's BuildType of a BLAS and Blas::update,
acceleration_structure/blas.rs:149-161, 292-310): the symbols load, the public layouts stand, bad arguments fail with a message."""
import ctypes as C

from sunray_amd import _lib, abi

NEW = ("sr_scene_set_mesh_build_type", "sr_scene_mesh_as_state", "sr_scene_read_mesh_tree", "sr_renderer_set_mesh_build_type")


def test_mesh_refit_symbols_load():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_update_info_keeps_its_size_and_the_version_stands():
    assert C.sizeof(abi.SrMeshUpdateInfo) == 64
    assert abi.SrMeshUpdateInfo.blas_refitted.offset == 12 and abi.SrMeshUpdateInfo.blas_refitted.size == 4
    assert abi.SrMeshUpdateInfo.blas_rebuilt.offset == 8 and abi.SrMeshUpdateInfo.validate_copy_ms.offset == 16
    assert _lib.lib().sr_version() == 1             # symbols were added and a padding word got a name: no layout changed


def test_null_scene_and_bad_build_type_fail_with_a_message_naming_the_call():
    L = _lib.lib()
    for bt in (abi.BUILD_RAPIDLY_CHANGING, abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_STATIC, 3):
        assert L.sr_scene_set_mesh_build_type(None, C.c_uint64(1), C.c_uint32(bt)) == -1
        assert b"sr_scene_set_mesh_build_type" in L.sr_last_error()
        assert L.sr_renderer_set_mesh_build_type(None, C.c_uint64(1), C.c_uint32(bt)) == -1
        assert b"sr_renderer_set_mesh_build_type" in L.sr_last_error()
    st, bt, op = abi.SrAsState(), C.c_uint32(), C.c_uint32()
    assert L.sr_scene_mesh_as_state(None, C.c_uint64(1), C.byref(bt), C.byref(st), C.byref(op)) == -1
    assert b"sr_scene_mesh_as_state" in L.sr_last_error()
    n = C.c_uint32()
    assert L.sr_scene_read_mesh_tree(None, C.c_uint64(1), C.byref(n), C.byref(n), None, None, None, None, None) == -1
    assert b"sr_scene_read_mesh_tree" in L.sr_last_error()


def test_the_heuristic_the_meshes_follow_rebuilds_at_the_ninth_update():
    """What the GPU tests expect of an updatable mesh, from the pure functions alone: SometimesChanges takes 8 updates, then the
    rebuild; RapidlyChanging the same; 16 quiet frames end in the quality build."""
    L = _lib.lib()
    L.sr_as_state_next_op.restype = C.c_uint32
    for bt in (abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING):
        st = abi.SrAsState()
        L.sr_as_state_initial(C.c_uint32(bt), C.byref(st))
        ops = []
        for _ in range(10):
            ops.append(L.sr_as_state_next_op(C.byref(st), 1))
            L.sr_as_state_mark_built(C.byref(st), C.c_uint32(ops[-1]))
        assert ops == [abi.OP_UPDATE] * 8 + [abi.OP_FAST_BUILD, abi.OP_UPDATE]
        quiet = []
        for _ in range(16):
            quiet.append(L.sr_as_state_next_op(C.byref(st), 0))
            L.sr_as_state_mark_built(C.byref(st), C.c_uint32(quiet[-1]))
        assert quiet == [abi.OP_NONE] * 15 + [abi.OP_SLOW_BUILD] and st.changing == 0
