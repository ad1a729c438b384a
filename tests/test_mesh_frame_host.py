"""CPU-side checks of the mesh frame (sr_mesh_frame_adjacency / sr_mesh_frame_host, sr_scene_set_mesh_frame /
sr_scene_update_mesh_positions* / sr_scene_mesh_frame_info and their renderer forms): the symbols load, the struct has its
documented size and field order, null and invalid arguments fail with a message that names the call, the Python wrappers refuse
wrong dtypes and shapes before the library is called, the host functions equal tests/normals_reference.py (the groups and runs word
for word, the records byte for byte), the float32 rule stays within a stated distance of a float64 model, and the compiler's report
lists both kernels without scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import _lib, abi, runtime

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_reference as ref  # noqa: E402

NEW_SYMBOLS = ("sr_mesh_frame_adjacency", "sr_mesh_frame_host", "sr_scene_set_mesh_frame", "sr_scene_update_mesh_positions_device",
               "sr_scene_update_mesh_positions", "sr_scene_mesh_frame_info", "sr_renderer_set_mesh_frame",
               "sr_renderer_update_mesh_positions_device", "sr_renderer_update_mesh_positions")
ERR_INVALID_ARG = -1
N, NT = ref.NORMALS, ref.NORMALS | ref.TANGENTS


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def lib_adjacency(v, idx):
    L = _lib.lib()
    n = C.c_uint32(0xDEAD)
    assert L.sr_mesh_frame_adjacency(p(v), C.c_uint32(len(v)), p(idx), C.c_uint32(len(idx)), None, None, None, C.byref(n)) == 0, L.sr_last_error()
    offsets, entries, side = np.full(len(v) + 1, 0xAAAAAAAA, dtype=np.uint32), np.full(n.value + 1, 0xAAAAAAAA, dtype=np.uint32), np.full(len(v) + 1, 7.0, dtype=np.float32)
    m = C.c_uint32()
    assert L.sr_mesh_frame_adjacency(p(v), C.c_uint32(len(v)), p(idx), C.c_uint32(len(idx)), p(offsets), p(entries), p(side), C.byref(m)) == 0
    assert m.value == n.value and entries[-1] == 0xAAAAAAAA and side[-1] == 7.0     # nothing is written past the counted sizes
    return offsets, entries[:-1], side[:-1]


def lib_host(v, idx, positions, flags):
    L = _lib.lib()
    out = np.zeros(len(v), dtype=abi.VERTEX)
    bad = C.c_uint32(5)
    pos = np.ascontiguousarray(positions, dtype=np.float32)
    rc = L.sr_mesh_frame_host(p(v), C.c_uint32(len(v)), p(idx), C.c_uint32(len(idx)), p(pos), C.c_uint32(flags), p(out), C.byref(bad))
    return rc, out, bad.value


MESHES = {
    "a single triangle": ref.single_triangle,
    "a cube of 24 vertices": ref.cube,
    "a uv-sphere with a seam column and poles": ref.seam_sphere,
    "a fan whose hub has 300 entries": ref.fan,
    "an unreferenced vertex": ref.unreferenced_vertex,
    "triangles with a repeated index": ref.repeated_index,
    "a winding that opposes the normals": lambda: ref.grid(5, 4, flip=True),
}


def test_frame_symbols_load_and_structs_hold():
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(abi.SrMeshFrameInfo) == 32
    assert [f[0] for f in abi.SrMeshFrameInfo._fields_] == ["flags", "n_groups", "n_entries", "max_valence", "updates", "first_bad", "frame_ms"]
    assert abi.SrMeshFrameInfo.first_bad.offset == 20 and abi.SrMeshFrameInfo.frame_ms.offset == 24
    assert (abi.FRAME_NORMALS, abi.FRAME_TANGENTS) == (1, 2)
    # symbols were added, no struct changed
    assert L.sr_version() == 1 and abi.VERTEX.itemsize == 96 and C.sizeof(abi.SrMeshSkinInfo) == 24 and C.sizeof(abi.SrMeshMorphInfo) == 24
    assert ref.VERTEX == abi.VERTEX


def test_frame_null_and_invalid_arguments_fail_with_a_message():
    L = _lib.lib()
    v, idx = ref.single_triangle()
    pos = np.zeros((3, 3), dtype=np.float32)
    scene = C.c_void_p(0x10)                                             # never looked at where a null argument decides
    n, info = C.c_uint32(), abi.SrMeshFrameInfo()
    assert L.sr_scene_set_mesh_frame(None, C.c_uint64(1), C.c_uint32(1)) == -1
    assert b"set_mesh_frame" in L.sr_last_error() and b"null" in L.sr_last_error()
    for call in (L.sr_scene_update_mesh_positions_device, L.sr_scene_update_mesh_positions):
        assert call(None, C.c_uint64(1), p(pos), C.c_uint32(3), None) == -1 and b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
        assert call(scene, C.c_uint64(1), None, C.c_uint32(3), None) == -1 and b"update_mesh" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_scene_mesh_frame_info(None, C.c_uint64(1), C.byref(info)) == -1 and b"sr_scene_mesh_frame_info" in L.sr_last_error()
    assert L.sr_scene_mesh_frame_info(scene, C.c_uint64(1), None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_renderer_set_mesh_frame(None, C.c_uint64(1), C.c_uint32(1)) == -1 and b"set_mesh_frame" in L.sr_last_error() and b"null" in L.sr_last_error()
    for call in (L.sr_renderer_update_mesh_positions_device, L.sr_renderer_update_mesh_positions):
        assert call(None, C.c_uint64(1), p(pos), C.c_uint32(3), None) == -1 and b"update_mesh_positions" in L.sr_last_error() and b"null" in L.sr_last_error()
    # the two host functions
    assert L.sr_mesh_frame_adjacency(None, C.c_uint32(3), p(idx), C.c_uint32(3), None, None, None, C.byref(n)) == -1
    assert b"sr_mesh_frame_adjacency" in L.sr_last_error() and b"null" in L.sr_last_error()
    assert L.sr_mesh_frame_adjacency(p(v), C.c_uint32(3), None, C.c_uint32(3), None, None, None, C.byref(n)) == -1 and b"null" in L.sr_last_error()
    assert L.sr_mesh_frame_adjacency(p(v), C.c_uint32(3), p(idx), C.c_uint32(2), None, None, None, C.byref(n)) == -1
    assert b"sr_mesh_frame_adjacency" in L.sr_last_error() and b"% 3" in L.sr_last_error()
    two = np.array([0, 1, 2, 0, 7, 9], dtype=np.uint32)
    assert L.sr_mesh_frame_adjacency(p(v), C.c_uint32(3), p(two), C.c_uint32(6), None, None, None, C.byref(n)) == -1
    assert b"index 7" in L.sr_last_error() and b"position 4" in L.sr_last_error()          # the lowest offender
    out = np.zeros(3, dtype=abi.VERTEX)
    for flags, word in ((0, b"flags"), (2, b"needs SR_FRAME_NORMALS"), (4, b"flags"), (7, b"flags")):
        assert L.sr_mesh_frame_host(p(v), C.c_uint32(3), p(idx), C.c_uint32(3), p(pos), C.c_uint32(flags), p(out), None) == -1, flags
        assert b"sr_mesh_frame_host" in L.sr_last_error() and word in L.sr_last_error(), (flags, L.sr_last_error())
    assert L.sr_mesh_frame_host(p(v), C.c_uint32(3), p(idx), C.c_uint32(3), None, C.c_uint32(1), p(out), None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_mesh_frame_host(p(v), C.c_uint32(3), p(idx), C.c_uint32(3), p(pos), C.c_uint32(1), None, None) == -1 and b"null" in L.sr_last_error()
    assert L.sr_mesh_frame_host(p(v), C.c_uint32(3), p(two), C.c_uint32(6), p(pos), C.c_uint32(1), p(out), None) == -1 and b"index 7" in L.sr_last_error()
    assert not out.view(np.uint8).any()
    # an empty mesh is no error: one offset, no entries
    off = np.full(1, 9, dtype=np.uint32)
    assert L.sr_mesh_frame_adjacency(None, C.c_uint32(0), None, C.c_uint32(0), p(off), None, None, C.byref(n)) == 0 and n.value == 0 and off[0] == 0


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


@pytest.mark.parametrize("method", [runtime.Scene.update_mesh_positions, runtime.Renderer.update_mesh_positions])
def test_update_mesh_positions_wrappers_refuse_before_the_library_is_called(monkeypatch, method):
    import torch
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    n = 5
    cases = {
        "float64 positions": np.zeros((n, 3), dtype=np.float64),
        "integer positions": np.zeros((n, 3), dtype=np.int32),
        "flat positions": np.zeros(n * 3, dtype=np.float32),
        "four components": np.zeros((n, 4), dtype=np.float32),
        "three dimensions": np.zeros((n, 3, 1), dtype=np.float32),
        "vertex records": np.zeros(n, dtype=abi.VERTEX),
        "no vertices": np.zeros((0, 3), dtype=np.float32),
        "a list": [[0.0, 0.0, 0.0]] * n,
        "a CPU tensor": torch.zeros((n, 3), dtype=torch.float32),
        "a float64 CPU tensor": torch.zeros((n, 3), dtype=torch.float64),
        "a CPU tensor of another shape": torch.zeros((n, 4), dtype=torch.float32),
        "nothing": None,
    }
    for what, a in cases.items():
        with pytest.raises(ValueError):
            method(_Handle(), 7, a)


@pytest.mark.parametrize("method", [runtime.Scene.set_mesh_frame, runtime.Renderer.set_mesh_frame])
def test_set_mesh_frame_wrappers_refuse_tangents_without_normals(monkeypatch, method):
    monkeypatch.setattr(runtime, "lib", lambda: _NoLibrary())
    with pytest.raises(ValueError):
        method(_Handle(), 7, normals=False, tangents=True)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_adjacency_equals_the_python_adjacency(name):
    v, idx = MESHES[name]()
    offsets, entries, groups = ref.adjacency(v, idx)
    side = ref.sides(v, idx)
    got = lib_adjacency(v, idx)
    assert got[0].tolist() == offsets.tolist() and got[1].tolist() == entries.tolist(), name
    assert got[2].tobytes() == side.tobytes(), name
    counts = np.diff(offsets.astype(np.int64))
    o2, e2, s2 = runtime.mesh_frame_adjacency(v, idx)
    assert (o2.tolist(), e2.tolist(), s2.tobytes()) == (offsets.tolist(), entries.tolist(), side.tobytes())
    # what the case is there for
    if name == "a single triangle":
        assert offsets.tolist() == [0, 1, 2, 3] and entries.tolist() == [0, 0, 0]
    elif name == "a cube of 24 vertices":
        assert len(set(groups)) == 24 and len(entries) == len(idx) and set(counts) == {1, 2} and (side == 1).all()
    elif name.startswith("a uv-sphere"):
        seg, rings = 12, 7
        assert len(set(groups)) == (rings - 1) * seg + 2 and len(entries) > len(idx)
        for r in range(1, rings):                                   # seam twins share their entries
            a, b = r * (seg + 1), r * (seg + 1) + seg
            assert groups[a] == groups[b] and entries[offsets[a]:offsets[a + 1]].tolist() == entries[offsets[b]:offsets[b + 1]].tolist()
        assert len(set(groups[:seg + 1])) == 1 and counts[0] == seg   # the copies of the pole: one group, a corner of every cap triangle
    elif name.startswith("a fan"):
        assert counts[0] == 300 and set(counts[1:]) == {2} and entries[:300].tolist() == list(range(300))
    elif name == "an unreferenced vertex":
        assert counts[4] == 0 and offsets[4] == offsets[5] == len(entries)
    elif name == "triangles with a repeated index":
        assert entries[offsets[0]:offsets[1]].tolist() == [0, 1, 1, 2] and entries[offsets[3]:offsets[4]].tolist() == [3, 3, 3, 4]
    else:
        assert (side == -1).all()


def _inputs(name, v, idx):
    """The positions every mesh is driven with -> {what: (reference records, positions)}."""
    cases = {"displaced": (v, ref.displaced(v)), "the reference positions": (v, np.ascontiguousarray(v["position"]))}
    flat = v.copy()
    flat["normal_tex_coord"] = 0.0
    cases["all-zero uvs"] = (flat, ref.displaced(v, 1.3))
    collapsed = ref.displaced(v, 0.2)
    collapsed[:] = collapsed[0]
    cases["every position in one point"] = (v, collapsed)
    return cases


@pytest.mark.parametrize("name", sorted(MESHES))
def test_host_rule_equals_the_float32_model_byte_for_byte(name):
    v0, idx = MESHES[name]()
    for what, (v, pos) in _inputs(name, v0, idx).items():
        for flags in (N, NT):
            want, bad, fallback = ref.frame_model(v, idx, pos, flags)
            rc, got, first_bad = lib_host(v, idx, pos, flags)
            assert rc == 0 and bad is None and first_bad == 0xFFFFFFFF, (name, what, flags, _lib.lib().sr_last_error())
            assert got.tobytes() == want.tobytes(), (name, what, flags, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])
            other = [n for n in abi.VERTEX.names if n not in ("position", "normal", "tangent")]
            assert all(got[n].tobytes() == v[n].tobytes() for n in other) and got["tangent"][:, 3].tobytes() == v["tangent"][:, 3].tobytes()
            assert got["position"].tobytes() == pos.tobytes()
            if flags == N or what == "all-zero uvs":
                assert got["tangent"].tobytes() == v["tangent"].tobytes(), (name, what)      # the reference's, byte for byte
            if what == "every position in one point":
                assert fallback.all() and got["normal"].tobytes() == v["normal"].tobytes()   # zero area everywhere: the fallback
            if what == "displaced" and name not in ("an unreferenced vertex", "triangles with a repeated index"):
                assert not fallback.any() and np.abs(np.linalg.norm(got["normal"].astype(np.float64), axis=1) - 1).max() < 1e-6
            assert runtime.mesh_frame_host(v, idx, pos, tangents=flags == NT).tobytes() == want.tobytes()


def test_mirrored_uvs_and_a_zero_area_neighbourhood():
    v, idx = ref.grid(9, 7, mirror_uv=True)
    pos = ref.displaced(v, 0.4)
    block = [i * 7 + j for i in (3, 4, 5) for j in (2, 3, 4)]
    pos[block] = pos[4 * 7 + 3]                                       # vertex (4, 3) and its eight neighbours in one point
    want, _, fallback = ref.frame_model(v, idx, pos, NT)
    assert fallback.tolist() == [i == 4 * 7 + 3 for i in range(len(v))]
    uv = v["normal_tex_coord"]
    tri = idx.reshape(-1, 3)
    a, b = uv[tri[:, 1]] - uv[tri[:, 0]], uv[tri[:, 2]] - uv[tri[:, 0]]
    det = a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]
    assert (det < 0).sum() == (det > 0).sum() > 0                   # a mirrored half
    rc, got, _ = lib_host(v, idx, pos, NT)
    assert rc == 0 and got.tobytes() == want.tobytes()
    assert got["normal"][4 * 7 + 3].tobytes() == v["normal"][4 * 7 + 3].tobytes()
    # away from the collapsed block the tangent follows +u on the plain half and the mirrored half alike: x grows with u before
    # the mirror line and falls with it behind it
    t = got["tangent"]
    assert t[1 * 7 + 5, 0] > 0.5 and t[7 * 7 + 5, 0] < -0.5


@pytest.mark.parametrize("bits", [0x7F800000, 0xFF800000, 0x7FC00000])
def test_host_rule_reports_the_lowest_non_finite_position(bits):
    v, idx = ref.grid(5, 4)
    n = len(v)
    for at, first in (([0], 0), ([n - 1], n - 1), ([n - 1, 0], 0), ([7, 3], 3)):
        pos = ref.displaced(v)
        pos.view(np.uint32)[at, 1] = bits
        assert ref.frame_model(v, idx, pos, NT)[1] == first
        rc, _, bad = lib_host(v, idx, pos, NT)
        assert rc == ERR_INVALID_ARG and bad == first, (at, rc, bad)
        assert ("vertex %d has a non-finite position" % first).encode() in _lib.lib().sr_last_error()


def test_planar_grid_keeps_exact_plane_normals():
    """A flat grid in z = 0 displaced in its plane only: every face vector is (±0, ±0, K), so x and y of every normal are ±0 exactly
    and |z| is K * fl(1 / K): two roundings of 2^-24 each, within 2^-22 of 1."""
    v, idx = ref.grid(17, 13)
    pos = ref.displaced(v, 0.9, 0.02)
    pos[:, 2] = 0.0
    rc, got, _ = lib_host(v, idx, pos, NT)
    assert rc == 0 and got.tobytes() == ref.frame_model(v, idx, pos, NT)[0].tobytes()
    n = got["normal"]
    assert (n[:, :2] == 0).all() and (np.abs(np.abs(n[:, 2].astype(np.float64)) - 1.0) <= 2.0 ** -22).all() and (n[:, 2] > 0).all()
    t = got["tangent"]
    assert (t[:, 2] == 0).all() and np.abs(np.linalg.norm(t[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6


MEASURED_ONE_MINUS_DOT = 1.378e-7     # the largest figure test_float32_rule_against_the_float64_model measured (its docstring)


def test_float32_rule_against_the_float64_model():
    """The float32 rule against the float64 model of the same geometry (the float32 positions taken as exact) on the displaced
    seam sphere and the displaced heightfield patch. Measured: the largest 1 - dot(float32 normal, float64 normal) is 1.124e-07 on the
    sphere and 1.378e-07 on the patch (this test prints both; a unit vector of float32 components alone misses length 1 by up to
    about 1e-7). The bound is four times the larger figure, 5.5e-07, the margin for other inputs of the same conditioning. The conditioning is asserted, not assumed: at every compared vertex the float64 model's accumulated length is above
    1e-3 of the summed face lengths, so no near-cancelling sum hides behind the bound."""
    worst = 0.0
    for what, (v, idx) in (("seam sphere", ref.seam_sphere(24, 13)), ("heightfield patch", ref.heightfield_patch(33))):
        pos = ref.displaced(v, 0.5, 0.1)
        n64, length, total = ref.frame_model64(v, idx, pos)
        assert (length > 1e-3 * total).all() and (total > 0).all(), what
        rc, got, _ = lib_host(v, idx, pos, N)
        assert rc == 0 and got.tobytes() == ref.frame_model(v, idx, pos, N)[0].tobytes()
        one_minus_dot = 1.0 - (got["normal"].astype(np.float64) * n64).sum(axis=1)
        print("%s: largest 1 - dot = %.3e" % (what, one_minus_dot.max()))
        worst = max(worst, float(one_minus_dot.max()))
    assert worst <= 4 * MEASURED_ONE_MINUS_DOT, worst


def test_frame_kernels_are_in_the_resource_report():
    """The compiler's report for normals.hip is kept next to the object: both kernels, each with and without tangents, need no
    scratch and spill nothing; the vertex kernel's LDS is the tile of 256 vertices, seven 16-byte slots each."""
    from sunray_amd import build
    res = build.kernel_resources("normals.hip")
    face = [r for name, r in res.items() if "face_frame_kernel" in name]
    vertex = [r for name, r in res.items() if "vertex_frame_kernel" in name]
    assert len(face) == 2 and len(vertex) == 2, sorted(res)
    for r in face + vertex:
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert all(r["lds"] == 256 * 7 * 16 and r["occupancy"] >= 4 for r in vertex) and all(r["lds"] == 0 for r in face)
    assert any("pose_batch_kernel" in name for name in build.kernel_resources("pose_batch.hip"))     # that report is still its own
