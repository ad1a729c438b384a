"""Host-side checks of the batched mesh-tree build's public interface (sr_scene_set_mesh_tree_batch, sr_scene_mesh_tree_batch_info,
sr_renderer_set_mesh_tree_batch): the exports exist and reject bad arguments, the Python mirror of the header's struct and constants
is pinned, the version stands, and the documents no longer call the batched build out of scope. Nothing here needs a GPU; that
SR_BLAS_BATCH is read when a scene is created needs a scene, so its spellings are checked in tests/test_gpu_mesh_tree_batch.py."""
import ctypes as C
import os
import re

from sunray_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_ERR_INVALID_ARG = -1
NEW = ("sr_scene_set_mesh_tree_batch", "sr_scene_mesh_tree_batch_info", "sr_renderer_set_mesh_tree_batch")


def header():
    return open(os.path.join(ROOT, "include", "sunray_hip.h")).read()


def test_exports_exist_and_reject_null_and_bad_modes():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    for mode in (abi.BLAS_BATCH_OFF, abi.BLAS_BATCH_ON, 2, 0xFFFFFFFF):
        # the mode is checked before the handle: a bad mode is refused as such, a good one gets as far as the null handle
        what = b"mode must be" if mode > abi.BLAS_BATCH_ON else b"is null"
        assert L.sr_scene_set_mesh_tree_batch(None, C.c_uint32(mode)) == SR_ERR_INVALID_ARG
        assert b"sr_scene_set_mesh_tree_batch" in L.sr_last_error() and what in L.sr_last_error()
        assert L.sr_renderer_set_mesh_tree_batch(None, C.c_uint32(mode)) == SR_ERR_INVALID_ARG
        assert b"sr_renderer_set_mesh_tree_batch" in L.sr_last_error() and what in L.sr_last_error()
    info = abi.SrMeshTreeBatchInfo()
    assert L.sr_scene_mesh_tree_batch_info(None, C.byref(info)) == SR_ERR_INVALID_ARG
    assert L.sr_scene_mesh_tree_batch_info(None, None) == SR_ERR_INVALID_ARG
    assert b"sr_scene_mesh_tree_batch_info" in L.sr_last_error()


def test_batch_info_struct_and_constants_match_the_header():
    h = header()
    body = re.search(r"typedef struct SrMeshTreeBatchInfo \{(.*?)\} SrMeshTreeBatchInfo;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|double)\s+(\w+);", body, re.M)
    assert [(n, {"uint32_t": C.c_uint32, "double": C.c_double}[t]) for t, n in fields] == list(abi.SrMeshTreeBatchInfo._fields_)
    assert C.sizeof(abi.SrMeshTreeBatchInfo) == 32 and abi.SrMeshTreeBatchInfo.batch_ms.offset == 24
    defines = {k: int(v) for k, v in re.findall(r"#define (SR_BLAS_BATCH_\w+) (\d+)u", h)}
    assert defines == {"SR_BLAS_BATCH_OFF": abi.BLAS_BATCH_OFF, "SR_BLAS_BATCH_ON": abi.BLAS_BATCH_ON, "SR_BLAS_BATCH_MAX_TRIS": abi.BLAS_BATCH_MAX_TRIS}
    assert (abi.BLAS_BATCH_OFF, abi.BLAS_BATCH_ON, abi.BLAS_BATCH_MAX_TRIS) == (0, 1, 4096)


def test_the_existing_structs_and_the_version_stand():
    assert C.sizeof(abi.SrMeshTreeInfo) == 40 and C.sizeof(abi.SrMeshUpdateInfo) == 64
    assert _lib.lib().sr_version() == 1             # symbols and a struct were added: no layout changed


def test_the_kernel_is_reported_without_scratch():
    """The compiler's report of blas_batch.hip is kept, and both instantiations (radix tree, PLOC) of the kernel run without scratch
    memory, within the 128 registers a 512-thread workgroup may use, and within a quarter of a compute unit's 160 KB of LDS."""
    from sunray_amd import build
    res = {k: v for k, v in build.kernel_resources("blas_batch.hip").items() if "blas_batch_build_kernel" in k}
    assert len(res) == 2, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["vgprs"] <= 128 and r["lds"] <= 40 * 1024, (name, r)


def test_no_document_calls_the_batched_build_out_of_scope():
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "one batched build for many small meshes is out of scope" not in text, path
        assert "SR_BLAS_BATCH" in text, path
