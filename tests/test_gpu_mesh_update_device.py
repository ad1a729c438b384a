"""Scene.update_mesh_device / Renderer.update_mesh_device (sr_scene_update_mesh_device: a deforming mesh's vertices taken from
device memory, validated by vertex_check_kernel, copied device to device, the library's host copy left behind until host code
needs it). Every comparison runs two scenes side by side that are loaded alike: scene A takes the new vertices through update_mesh
from numpy, scene B the same bytes through update_mesh_device from a tensor made of those bytes. Equal means bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_mesh_update import assert_frames_equal, mesh_of, one_frame  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402

U, F, S, NONE = abi.OP_UPDATE, abi.OP_FAST_BUILD, abi.OP_SLOW_BUILD, abi.OP_NONE
SOMETIMES, RAPIDLY = abi.BUILD_SOMETIMES_CHANGES, abi.BUILD_RAPIDLY_CHANGING
ERR_INVALID_ARG = -1
VERTEX_WORDS = abi.VERTEX.itemsize // 4


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def to_device(vertices, as_floats=False):
    """A device tensor made of the bytes of `vertices` (uint8, or float32 to show that the dtype is free)."""
    import torch
    v = np.ascontiguousarray(vertices, dtype=abi.VERTEX)
    host = v.view(np.float32).copy() if as_floats else v.view(np.uint8).copy()
    return torch.from_numpy(host).to("cuda:0")


def ray_grid(lo, hi, nx=96, ny=32):
    """Parallel rays down -z over the rectangle lo..hi (x, y) and down -y over the same x range: a fixed grid, no randomness."""
    xs, ys = np.meshgrid(np.linspace(lo[0], hi[0], nx), np.linspace(lo[1], hi[1], ny), indexing="ij")
    r = np.zeros(2 * nx * ny, dtype=abi.RAY)
    n = nx * ny
    r["origin"][:n] = np.stack([xs.ravel(), ys.ravel(), np.full(n, 9.0)], axis=1)
    r["dir"][:n] = (0.0, 0.0, -1.0)
    r["origin"][n:] = np.stack([xs.ravel(), np.full(n, 9.0), ys.ravel() * 0.5], axis=1)
    r["dir"][n:] = (0.0, -1.0, 0.0)
    r["tmin"], r["tmax"] = 1e-3, 100.0
    return r


def traces(rt, sc, rays, rd):
    """Closest hits and occlusion bits of the fixed grid, as words."""
    hits = rt.hits_from_device(sc.trace_closest(rd, len(rays))).view(np.uint32).copy()
    return hits, sc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32).copy()


def vertex_info(sc, key):
    i = sc.mesh_vertex_info(key)
    return (i.host_stale, i.last_from_device, i.host_fetches, i.check_ms, i.copy_ms, i.fetch_ms)


def flags(sc, key):
    return vertex_info(sc, key)[:3]


def update_counts(sc):
    i, t = sc.mesh_update_info(), sc.mesh_tree_info()
    return (i.dirty_meshes, i.reshaded, i.blas_rebuilt, i.blas_refitted, sc.as_state()[1], t.built_on_device, t.built_on_host, t.reason)


def assert_scenes_equal(rt, a, b, rays, rd, keys, what):
    """Structure, tables, queries and counts of scene B (device updates) against scene A (host updates)."""
    assert a.two_level() == b.two_level()
    if a.two_level():
        for k in keys:
            ta, tb = a.read_mesh_tree(k), b.read_mesh_tree(k)
            for name in ("nodes", "tris", "shade", "shade_tex", "slot_of_prim"):
                assert_bits_equal(ta[name], tb[name], "%s: mesh %d tree %s" % (what, k, name))
        for name, x, y in zip(("nodes", "tl_inst", "records", "boxes"), a.read_top_level(), b.read_top_level()):
            if name == "records":       # blas_root / prim_base are positions in each scene's own arrays and are equal too (same loads)
                assert x.tobytes() == y.tobytes(), "%s: top-level records" % what
            else:
                assert_bits_equal(x, y, "%s: top-level %s" % (what, name))
    else:
        for name, x, y in zip(("nodes", "tris"), a.read_bvh(), b.read_bvh()):
            assert_bits_equal(x, y, "%s: bvh %s" % (what, name))
    ta, tb = a.tables(), b.tables()
    for name in ("transforms", "indirection", "emissive_triangles"):
        assert_bits_equal(ta[name], tb[name], "%s: table %s" % (what, name))
    assert ta["num_lights"] == tb["num_lights"]
    assert_bits_equal(ta["meshes_info"]["material"], tb["meshes_info"]["material"], "%s: mesh table materials" % what)
    ha, oa = traces(rt, a, rays, rd)
    hb, ob = traces(rt, b, rays, rd)
    assert (ha.view(abi.HIT)["t"] >= 0).mean() > 0.03, what
    assert_bits_equal(ha, hb, "%s: closest hits" % what)
    assert_bits_equal(oa, ob, "%s: occlusion" % what)
    assert update_counts(a) == update_counts(b), what


# ---- 1. the check kernel through the entry point ---------------------------------------------------------------------------------
def check_meshes():
    """Meshes of 3, 4, 63, 64, 65, 257 and 1026 vertices, keys 1..7, side by side along x. Six 16-byte pieces per vertex: the first
    wave boundary (piece 64) falls inside vertex 10, block boundaries (256 pieces) inside vertices 42, 85, 128, ..."""
    s = scenes.SceneDesc("check_meshes")
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    up = np.tile(np.array((0, 0, 1), dtype=np.float32), (3, 1))
    built = [(scenes.make_vertices(np.array([(-1, -1, 0), (1, -1, 0.25), (0, 1, 0)], dtype=np.float32), up), np.array([0, 1, 2], dtype=np.uint32)),
             scenes.quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0), (0, 0, 1))]
    for nu, nv in ((6, 8), (7, 7), (4, 12)):
        built.append(scenes.grid_patch((-1, -1, 0), (2, 0, 0), (0, 2, 0), nu, nv, (0, 0, 1), (1, 0, 0)))
    built.append(scenes.uv_sphere(1.0, 15, 18))
    built.append(scenes.uv_sphere(1.0, 32, 33))
    assert [len(v) for v, _ in built] == [3, 4, 63, 64, 65, 257, 1026]
    for k, (v, i) in enumerate(built, start=1):
        s.meshes.append(scenes.MeshDesc(k, v, i, grey))
        s.instances.append((k, [scenes.translate(3.0 * (k - 1), 0.0, 0.0)]))
    return s


NON_FINITE = {"NaN": 0x7FC00000, "+Inf": 0x7F800000, "-Inf": 0xFF800000, "NaN with the sign bit": 0xFFC00000, "NaN with the lowest payload bit": 0x7F800001}


def poked(vertices, pokes):
    """A copy with raw words written: pokes = [(vertex, word of the 24-word record, bits)]."""
    v = vertices.copy()
    w = v.view(np.uint32).reshape(len(v), VERTEX_WORDS)
    for i, word, bits in pokes:
        w[i, word] = bits
    return v


def refused(rt, sc, call):
    with pytest.raises(rt.SunrayError) as e:
        call()
    return e.value.code, e.value.description


def test_check_kernel_reports_what_the_host_reports(rt):
    desc = check_meshes()
    a, b = rt.Scene(0).load(desc), rt.Scene(0).load(desc)
    rays = ray_grid((-1.5, -1.5), (3.0 * 6 + 1.5, 1.5), 160, 24)
    rd = rt.rays_to_device(rays)
    before = traces(rt, b, rays, rd)
    assert (before[0].view(abi.HIT)["t"] >= 0).mean() > 0.03
    assert_bits_equal(traces(rt, a, rays, rd)[0], before[0], "the two scenes are loaded alike")
    n_cases = 0
    for m in desc.meshes:
        n = len(m.vertices)
        info0 = vertex_info(b, m.key)
        assert info0[:3] == (0, 0, 0)
        cases = []
        for at in sorted({0, n - 1, 10} & set(range(n))):           # vertex 10: pieces 60..65, across the first wave boundary
            for comp in range(3):
                for name, bits in NON_FINITE.items():
                    cases.append(("%s in component %d of vertex %d" % (name, comp, at), [(at, comp, bits)], at))
        lo, hi = (1, n - 1) if n < 1026 else (50, 1000)             # two offenders: the lower index is reported
        cases.append(("two offenders", [(hi, 0, NON_FINITE["NaN"]), (lo, 2, NON_FINITE["-Inf"])], lo))
        cases.append(("two offenders, the other way round", [(lo, 1, NON_FINITE["+Inf"]), (hi, 2, NON_FINITE["NaN"])], lo))
        for what, pokes, first in cases:
            v = poked(m.vertices, pokes)
            want = refused(rt, a, lambda: a.update_mesh(m.key, v))
            got = refused(rt, b, lambda: b.update_mesh_device(m.key, to_device(v)))
            assert want == (ERR_INVALID_ARG, "update_mesh: vertex %d has a non-finite position" % first), (m.key, what, want)
            assert got == want, (m.key, what, got)
            assert vertex_info(b, m.key) == info0, (m.key, what)
            n_cases += 1
        after = traces(rt, b, rays, rd)                               # nothing is pending: no set_instances is needed to trace
        assert_bits_equal(before[0], after[0], "closest hits after the refusals of mesh %d" % m.key)
        assert_bits_equal(before[1], after[1], "occlusion after the refusals of mesh %d" % m.key)
        assert_bits_equal(before[0], traces(rt, a, rays, rd)[0], "scene A after the refusals of mesh %d" % m.key)
    assert n_cases == 7 * 2 + 15 * (2 + 2 + 5 * 3)
    # every word but the position's three is free: non-finite normals, tangents, uv sets and pad words are accepted by both calls
    for m in desc.meshes:
        n = len(m.vertices)
        pattern = list(NON_FINITE.values())
        v = poked(m.vertices, [(i, w, pattern[(i + w) % len(pattern)]) for i in range(n) for w in range(3, VERTEX_WORDS)])
        assert np.isfinite(v["position"]).all() and not np.isfinite(v["_pad0"]).any() and not np.isfinite(v["_pad3"]).any()
        a.update_mesh(m.key, v)
        b.update_mesh_device(m.key, to_device(v))
        assert flags(b, m.key) == (1, 1, 0) and flags(a, m.key) == (0, 0, 0)
    a.set_instances(desc.instances); b.set_instances(desc.instances)
    for (x, y), name in zip(zip(a.read_bvh(), b.read_bvh()), ("nodes", "tris")):
        assert_bits_equal(x, y, "bvh %s after the accepted update" % name)
    assert_bits_equal(traces(rt, a, rays, rd)[0], traces(rt, b, rays, rd)[0], "closest hits after the accepted update")
    assert_bits_equal(before[0], traces(rt, b, rays, rd)[0], "positions did not change")
    a.close(); b.close()


# ---- 2. every apply path, 3. the lazy host copy ------------------------------------------------------------------------------------
def sphere_and_quad():
    """A deforming sphere of 320 triangles (key 1) over a static quad (key 2)."""
    s = scenes.SceneDesc("sphere_and_quad")
    sv, si = scenes.uv_sphere(1.0, 16, 11)
    assert len(si) == 3 * 320
    s.meshes.append(scenes.MeshDesc(1, sv, si, abi.material(base_color=(0.9, 0.5, 0.3, 1.0), roughness=0.3)))
    qv, qi = scenes.quad((-3, -1.5, 3), (3, -1.5, 3), (3, -1.5, -3), (-3, -1.5, -3), (0, 1, 0))
    s.meshes.append(scenes.MeshDesc(2, qv, qi, abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)))
    s.instances = [(1, [scenes.translate(0.0, 0.0, 0.0), scenes.scale_rotate_y(0.4, 0.6, 0.9, 0.5, 1.8, 0.2, -0.4)]), (2, [scenes.translate(0.0, 0.0, 0.0)])]
    return s


SPHERE_RAYS = ((-3.0, -2.0), (3.0, 2.0))

# name -> (form, build type of the sphere or None for Static, mesh-tree build mode, forced op, fetches of B's host copy per step)
PATHS = {
    "one-level update": ("flat", None, "auto", U, 0),
    "one-level fast build": ("flat", None, "auto", F, 1),          # 324 triangles: below the device builder's floor, the host builds
    "one-level slow build": ("flat", None, "auto", S, 1),
    "two-level static mesh": ("two_level", None, "auto", NONE, 1),
    "two-level device refit": ("two_level", SOMETIMES, "auto", U, 0),
    "two-level device build": ("two_level", SOMETIMES, "device", F, 0),
    "two-level forced slow build": ("two_level", SOMETIMES, "auto", S, 1),
}


def pair(rt, desc, form, build_type, mode, key=1):
    out = []
    for _ in range(2):
        sc = rt.Scene(0, instancing=form).set_mesh_tree_build(mode).load(desc)
        if build_type is not None:
            sc.set_mesh_build_type(key, build_type)
        out.append(sc)
    return out


def step(a, b, desc, op, key=1, as_floats=True):
    """The same bytes into A from the host and into B from the device, then the set_instances that applies them."""
    v = mesh_of(desc, key).vertices
    for sc in (a, b):
        if op != NONE:
            sc.force_next_op(op)
    a.update_mesh(key, v)
    b.update_mesh_device(key, to_device(v, as_floats))
    a.set_instances(desc.instances); b.set_instances(desc.instances)


@pytest.mark.parametrize("path", list(PATHS))
def test_every_apply_path_equals_the_host_update(rt, path):
    form, build_type, mode, op, fetches_per_step = PATHS[path]
    desc = sphere_and_quad()
    a, b = pair(rt, desc, form, build_type, mode)
    rays = ray_grid(*SPHERE_RAYS)
    rd = rt.rays_to_device(rays)
    first = traces(rt, b, rays, rd)[0]
    for n in (1, 2, 3):
        desc = scenes.deform(desc, [1], float(n))
        step(a, b, desc, op)
        what = "%s, step %d" % (path, n)
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2], what)
        counts = update_counts(b)
        print(what, counts, vertex_info(b, 1))
        if path == "one-level update":
            assert counts[:2] == (1, 1) and counts[4] == U
        elif path == "two-level device refit":
            assert counts[2:4] == (0, 1)
        elif path == "two-level device build":
            assert counts[2:4] == (1, 0) and counts[5:] == (1, 0, abi.MESH_TREE_ON_DEVICE)
        elif form == "two_level":
            assert counts[2:4] == (1, 0) and counts[5:7] == (0, 1)
        # the lazy host copy: device paths never fetch, a host build fetches once per update
        assert flags(b, 1) == ((1, 1, 0) if fetches_per_step == 0 else (0, 1, n)), what
        assert flags(a, 1) == (0, 0, 0) and flags(b, 2) == (0, 0, 0)
    assert not np.array_equal(first, traces(rt, b, rays, rd)[0])
    a.close(); b.close()


def test_host_builds_after_a_device_refit_fetch_once(rt):
    """The host copy a device refit left behind is fetched by the next host build of the tree: a forced slow build, and the settle
    rebuild that 16 quiet frames end in. One fetch each, and the tree is scene A's."""
    rays = ray_grid(*SPHERE_RAYS)
    rd = rt.rays_to_device(rays)
    for what in ("forced slow build", "settle rebuild"):
        desc = sphere_and_quad()
        a, b = pair(rt, desc, "two_level", RAPIDLY, "auto")
        for n in (1, 2):
            desc = scenes.deform(desc, [1], float(n))
            step(a, b, desc, U)
        assert update_counts(b)[2:4] == (0, 1) and flags(b, 1) == (1, 1, 0)
        if what == "forced slow build":
            desc = scenes.deform(desc, [1], 3.0)
            step(a, b, desc, S)
            assert update_counts(b)[2:4] == (1, 0)
        else:
            for sc in (a, b):
                last = [(sc.end_frame(), sc.mesh_as_state(1)[2])[1] for _ in range(16)]
                assert last == [NONE] * 15 + [S], last
        assert flags(b, 1) == (0, 1, 1), what
        assert flags(a, 1) == (0, 0, 0)
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2], what)
        a.close(); b.close()


def test_device_host_device_sequence(rt):
    """Device update, host update, device update, different bytes each, all refitted: after each step B equals A (which took the
    same bytes from the host), the flag follows the kind of the last update, and at the end B equals a scene that took only the
    last bytes (a refit is a function of the topology and the vertices at hand)."""
    rays = ray_grid(*SPHERE_RAYS)
    rd = rt.rays_to_device(rays)
    desc = sphere_and_quad()
    a, b = pair(rt, desc, "two_level", SOMETIMES, "auto")
    only_last = pair(rt, desc, "two_level", SOMETIMES, "auto")[0]
    for n, from_device in enumerate((True, False, True), start=1):
        desc = scenes.deform(desc, [1], float(n))
        v = mesh_of(desc, 1).vertices
        for sc in (a, b):
            sc.force_next_op(U)
        a.update_mesh(1, v)
        if from_device:
            b.update_mesh_device(1, to_device(v))
        else:
            b.update_mesh(1, v)
        assert flags(b, 1) == ((1, 1, 0) if from_device else (0, 0, 0)), n
        a.set_instances(desc.instances); b.set_instances(desc.instances)
        assert flags(b, 1) == ((1, 1, 0) if from_device else (0, 0, 0)), n
        assert_scenes_equal(rt, a, b, rays, rd, [1, 2], "sequence step %d" % n)
    only_last.force_next_op(U)
    only_last.update_mesh(1, mesh_of(desc, 1).vertices)
    only_last.set_instances(desc.instances)
    tb, tl = b.read_mesh_tree(1), only_last.read_mesh_tree(1)
    for name in ("nodes", "tris", "shade", "slot_of_prim"):
        assert_bits_equal(tl[name], tb[name], "against the last bytes alone: tree %s" % name)
    assert_bits_equal(traces(rt, only_last, rays, rd)[0], traces(rt, b, rays, rd)[0], "against the last bytes alone: closest hits")
    for sc in (a, b, only_last):
        sc.close()


# ---- 4. emissive mesh --------------------------------------------------------------------------------------------------------------
def test_emissive_mesh_fetches_inside_the_call(rt, blue_noise):
    desc = scenes.instanced_field(10)
    instanced = {k for k, _ in desc.instances}
    lamp = next(m.key for m in desc.meshes if float(m.material["emissive_factor"][3]) > 0 and m.key in instanced)
    a, b = rt.Scene(0).load(desc), rt.Scene(0).load(desc)
    assert len(a.tables()["emissive_triangles"]) == len(mesh_of(desc, lamp).indices) // 3 > 1
    W, H = 80, 60
    f0 = one_frame(rt, b, desc, W, H, blue_noise)
    assert_frames_equal(one_frame(rt, a, desc, W, H, blue_noise), f0, "before the update")
    before_tables = b.tables()
    d1 = scenes.deform(desc, [lamp], 1.0)
    v = mesh_of(d1, lamp).vertices
    a.update_mesh(lamp, v)
    b.update_mesh_device(lamp, to_device(v, as_floats=True))
    assert flags(b, lamp) == (0, 1, 1)                              # fetched inside the call: the light table is host arithmetic
    a.set_instances(d1.instances); b.set_instances(d1.instances)
    assert flags(b, lamp) == (0, 1, 1)
    ta, tb = a.tables(), b.tables()
    assert_bits_equal(ta["emissive_triangles"], tb["emissive_triangles"], "emissive triangles")
    assert_bits_equal(ta["indirection"], tb["indirection"], "emissive indirection")
    assert not np.array_equal(tb["emissive_triangles"], before_tables["emissive_triangles"])
    fa, fb = one_frame(rt, a, d1, W, H, blue_noise), one_frame(rt, b, d1, W, H, blue_noise)
    assert_frames_equal(fa, fb, "a frame after the emissive update")
    assert not np.array_equal(fa[0], f0[0])
    a.close(); b.close()


# ---- 5. refusals the host decides ------------------------------------------------------------------------------------------------
def test_refusals_decided_on_the_host(rt):
    """A wrong count, an unknown key, a range that overlaps the mesh's own buffer, a pointer that is 4 bytes off: refused before
    anything is launched, with the host call's text where the host call has the case, and the scene traces as before."""
    import torch
    from sunray_amd._lib import lib
    desc = sphere_and_quad()
    a, b = rt.Scene(0).load(desc), rt.Scene(0).load(desc)
    rays = ray_grid(*SPHERE_RAYS)
    rd = rt.rays_to_device(rays)
    before = traces(rt, b, rays, rd)
    v = mesh_of(scenes.deform(desc, [1], 1.0), 1).vertices
    n = len(v)
    info0 = vertex_info(b, 1)

    def unchanged(what):
        after = traces(rt, b, rays, rd)
        assert_bits_equal(before[0], after[0], "closest hits after a refused " + what)
        assert_bits_equal(before[1], after[1], "occlusion after a refused " + what)
        assert vertex_info(b, 1) == info0, what
    for what, key, verts in (("wrong count", 1, v[:-1]), ("unknown key", 12345, v)):
        want = refused(rt, a, lambda: a.update_mesh(key, verts))
        got = refused(rt, b, lambda: b.update_mesh_device(key, to_device(verts)))
        assert want[0] == ERR_INVALID_ARG and got == want, (what, want, got)
        unchanged(what)
    assert "%d vertices given" % (n - 1) in refused(rt, b, lambda: b.update_mesh_device(1, to_device(v[:-1])))[1]
    # the mesh's own allocation, as sr_scene_get_tables shows it: the same range, and ranges that reach into it from either side
    own = int(b.tables()["meshes_info"][0]["vertices"])
    for offset in (0, 96, -96, 96 * (n - 1), -96 * (n - 1)):
        rc = lib().sr_scene_update_mesh_device(b._h, C.c_uint64(1), C.c_void_p(own + offset), C.c_uint32(n), None)
        assert rc == ERR_INVALID_ARG and b"overlap" in lib().sr_last_error(), (offset, rc, lib().sr_last_error())
        unchanged("overlapping range at %d" % offset)
    # 4 bytes off: still contiguous and of the right size, so the wrapper passes it on and the library refuses it
    room = torch.zeros(n * 96 + 16, dtype=torch.uint8, device="cuda:0")
    shifted = room[4:4 + n * 96]
    shifted.copy_(to_device(v))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    code, text = refused(rt, b, lambda: b.update_mesh_device(1, shifted))
    assert code == ERR_INVALID_ARG and "16-byte aligned" in text, text
    unchanged("misaligned pointer")
    # the same bytes from an aligned tensor are taken
    b.update_mesh_device(1, to_device(v))
    assert flags(b, 1) == (1, 1, 0)
    a.close(); b.close()


# ---- 6. Renderer -------------------------------------------------------------------------------------------------------------------
def test_renderer_update_mesh_device_equals_update_mesh(rt):
    """Renderer.update_mesh_device against Renderer.update_mesh over six frames with three deformations, frames in flight: with one
    slot, and with two slots on one GPU (rehearsal), where the second replica takes the validated bytes by a device copy."""
    from test_gpu_multi_renderer import assert_equal, grab, load
    hip = C.CDLL("libamdhip64.so")
    desc = scenes.cornell_box()
    cam = (desc.camera_pos, desc.camera_target, desc.fov_y)

    def run(r, from_device):
        load(r, desc)
        out, d = [], desc
        for f in range(6):
            if f in (2, 3, 5):
                d = scenes.deform(d, [7], float(f))
                v = mesh_of(d, 7).vertices
                if from_device:
                    r.update_mesh_device(7, to_device(v, as_floats=f == 3))       # the previous frame may still be in flight
                else:
                    r.update_mesh(7, v)
            fr = r.render(cam, d.instances)
            r.wait_frame(fr)
            out.append(grab(rt, hip, r))
        return out
    for devices in (None, [0, 0]):
        host = rt.Renderer((96, 80), devices=devices)
        want = run(host, False)
        host.close()
        dev = rt.Renderer((96, 80), devices=devices)
        got = run(dev, True)
        assert dev.history_overflow() == 0
        n_slots = len(devices) if devices else 1
        for slot in range(n_slots):
            assert flags(dev.replica_scene(slot), 7)[:2] == (1, 1), slot
        bad = poked(mesh_of(desc, 7).vertices, [(5, 1, NON_FINITE["NaN"])])
        code, text = refused(rt, dev, lambda: dev.update_mesh_device(7, to_device(bad)))
        assert (code, text) == (ERR_INVALID_ARG, "update_mesh: vertex 5 has a non-finite position")
        dev.close()
        for i, (x, y) in enumerate(zip(want, got)):
            assert_equal(x[0], y[0], "%d slot(s), frame %d output" % (n_slots, i))
            assert_equal(x[1], y[1], "%d slot(s), frame %d raw_color" % (n_slots, i))
        assert not np.array_equal(want[1][1], want[5][1])
