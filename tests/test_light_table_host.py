"""CPU-side checks of the light table on the device (sr_scene_set_light_table_build and its companions): the symbols load, the
info struct has its documented size, null arguments and an unknown mode fail with a message, the exported host arithmetic
(sr_light_table) equals the numpy restatement bit for bit, and the compiler's report lists both kernels without scratch."""
import ctypes as C

import numpy as np
import pytest

from sunray_amd import _lib, abi, runtime
from sunray_amd.build import kernel_resources

from light_table_reference import affine, light_table as reference_light_table

NEW_SYMBOLS = ("sr_scene_set_light_table_build", "sr_scene_light_table_info", "sr_scene_read_lights", "sr_light_table",
               "sr_renderer_set_light_table_build", "sr_renderer_light_table_info")


def test_light_table_symbols_load_and_struct_holds():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrLightTableInfo) == 56
    assert [f[0] for f in abi.SrLightTableInfo._fields_] == ["mode", "on_device", "num_lights", "arena_entries", "positions_rewritten", "entries_uploaded",
                                                             "arena_uploads", "arena_fetches", "positions_ms", "table_ms", "host_ms"]
    assert abi.SrLightTableInfo.positions_ms.offset == 32 and (abi.LIGHTS_HOST, abi.LIGHTS_DEVICE) == (0, 1)
    # symbols were added, no struct changed
    assert L.sr_version() == 1 and C.sizeof(abi.SrMeshVertexInfo) == 40 and C.sizeof(abi.SrMeshUpdateInfo) == 64


def test_null_arguments_and_an_unknown_mode_fail_with_a_message():
    L = _lib.lib()
    fake = C.c_void_p(0x10)                                    # never looked at: every refusal below comes first
    assert L.sr_scene_set_light_table_build(None, C.c_uint32(1)) == -1 and b"sr_scene_set_light_table_build" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_set_light_table_build(fake, C.c_uint32(2)) == -1 and b"SR_LIGHTS_HOST or SR_LIGHTS_DEVICE" in L.sr_last_error()
    info = abi.SrLightTableInfo()
    assert L.sr_scene_light_table_info(None, C.byref(info)) == -1 and b"sr_scene_light_table_info" in L.sr_last_error()
    assert L.sr_scene_light_table_info(fake, None) == -1 and b"null" in L.sr_last_error()
    n = C.c_uint32()
    assert L.sr_scene_read_lights(None, None, C.c_uint32(0), C.byref(n)) == -1 and b"sr_scene_read_lights" in L.sr_last_error()
    assert L.sr_scene_read_lights(fake, None, C.c_uint32(0), None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_scene_read_lights(fake, None, C.c_uint32(4), C.byref(n)) == -1 and b"null" in L.sr_last_error()
    assert L.sr_renderer_set_light_table_build(None, C.c_uint32(0)) == -1 and b"sr_renderer_set_light_table_build" in L.sr_last_error()
    assert L.sr_renderer_set_light_table_build(fake, C.c_uint32(7)) == -1 and b"SR_LIGHTS_HOST or SR_LIGHTS_DEVICE" in L.sr_last_error()
    assert L.sr_renderer_light_table_info(None, C.c_uint32(0), C.byref(info)) == -1 and b"sr_renderer_light_table_info" in L.sr_last_error()
    assert L.sr_renderer_light_table_info(fake, C.c_uint32(0), None) == -1 and b"null" in L.sr_last_error()
    t = np.zeros((1, 12), dtype=np.float32)
    e = np.zeros(1, dtype=abi.EMISSIVE_INDIRECTION)
    tri = np.zeros(1, dtype=abi.EMISSIVE_TRIANGLE)
    out = np.zeros((1, 16), dtype=np.float32)
    p = [a.ctypes.data_as(C.c_void_p) for a in (t, e, tri, out)]
    for k in range(4):
        args = list(p)
        args[k] = None
        assert L.sr_light_table(args[0], C.c_uint32(1), args[1], C.c_uint32(1), args[2], C.c_uint32(1), args[3]) == -1
        assert b"sr_light_table" in L.sr_last_error() and b"null" in L.sr_last_error()

    class Handle:
        _h = C.c_void_p(0x10)
    with pytest.raises(KeyError):
        runtime.Scene.set_light_table_build(Handle(), "gpu")   # the wrapper knows "host" and "device"
    with pytest.raises(KeyError):
        runtime.Renderer.set_light_table_build(Handle(), "gpu")


def random_case(seed, n_entries):
    rng = np.random.default_rng(seed)
    n_tris, n_inst = max(1, min(n_entries // 2, 40)), max(1, min(n_entries // 3, 7))       # fewer than the entries: slots and instances repeat
    tri = np.zeros(n_tris, dtype=abi.EMISSIVE_TRIANGLE)
    for k in ("v0", "v1", "v2"):
        tri[k][:, :3] = rng.uniform(-4.0, 4.0, (n_tris, 3)).astype(np.float32)
        tri[k][:, 3] = rng.uniform(-1.0, 1.0, n_tris).astype(np.float32)   # the unused w words must not matter
    tri["emission"] = rng.uniform(0.0, 20.0, (n_tris, 4)).astype(np.float32)
    entries = np.zeros(n_entries, dtype=abi.EMISSIVE_INDIRECTION)
    entries["blas_tri_index"] = rng.integers(0, n_tris, n_entries)
    entries["entity_id"] = rng.integers(0, n_inst, n_entries)
    return affine(rng, n_inst), entries, tri


@pytest.mark.parametrize("n_entries", [1, 2, 65, 1025])
def test_host_light_table_equals_the_numpy_restatement(n_entries):
    transforms, entries, tri = random_case(1000 + n_entries, n_entries)
    got = runtime.light_table(transforms, entries, tri)
    want = reference_light_table(transforms, entries, tri)
    assert got.shape == want.shape == (n_entries, 16) and got.dtype == np.float32
    assert np.isfinite(want).all() and (want[:, 3] > 0).all()                      # no degenerate triangle among the inputs
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]
    if n_entries > 2:
        assert len(np.unique(entries["blas_tri_index"])) < n_entries and len(np.unique(entries["entity_id"])) < n_entries


def test_an_index_out_of_range_is_refused():
    transforms, entries, tri = random_case(5, 9)
    for field, limit in (("blas_tri_index", len(tri)), ("entity_id", len(transforms))):
        bad = entries.copy()
        bad[field][4] = limit
        with pytest.raises(_lib.SunrayError) as e:
            runtime.light_table(transforms, bad, tri)
        assert e.value.code == -1 and "entry 4" in e.value.description
        bad[field][4] = 0xFFFFFFFF
        with pytest.raises(_lib.SunrayError):
            runtime.light_table(transforms, bad, tri)


def test_compiler_report_lists_both_kernels_without_scratch():
    res = kernel_resources("lights.hip")
    for kernel in ("light_table_kernel", "emissive_positions_kernel"):
        rows = [v for k, v in res.items() if kernel in k]
        assert len(rows) == 1, (kernel, list(res))
        r = rows[0]
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (kernel, r)
        assert r["vgprs"] > 0 and r["occupancy"] > 0 and r["lds"] == 0, (kernel, r)
