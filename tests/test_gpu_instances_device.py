"""Scene.set_instances_device / Renderer.render_device_transforms (sr_scene_set_instances_device: a frame's instance transforms
taken from device memory, instance_tables_kernel of csrc/instances.hip writing the per-instance tables and validating in one
pass, the library's host copy of the transforms left behind until host code needs it). Every comparison runs two scenes side by
side that are loaded alike: scene A takes the numbers through set_instances from numpy, scene B the same bytes through
set_instances_device from a tensor. Equal means bit for bit; only the table words that are NaN on the host admit any NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_multi_renderer import assert_equal, grab  # noqa: E402
from test_gpu_parity import assert_bits_equal  # noqa: E402
from test_gpu_top_level_build import affine_transforms  # noqa: E402
from test_instances_device_host import assert_words_equal_nan_rule, edge_transforms, host_tables  # noqa: E402

ERR_INVALID_ARG = -1
NON_FINITE_TEXT = "frame_instance_data: instance transform holds a non-finite value"
QUAD, SPHERE, LAMP = 1, 2, 3
W, H = 64, 36
CAMERA = ((0.0, 3.0, 14.0), (0.0, 0.0, 0.0), 45.0)


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def hip():
    import torch  # noqa: F401  (the HIP runtime torch loaded)
    return C.CDLL("libamdhip64.so")


def meshes(lamp=False):
    """One quad (2 triangles), one 60-triangle sphere and, with `lamp`, one emissive quad: (key, vertices, indices, material)."""
    grey = abi.material(base_color=(0.8, 0.8, 0.8, 1.0), roughness=0.5)
    out = [(QUAD, *scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 0)), grey), (SPHERE, *scenes.uv_sphere(1.0, 6, 6), grey)]
    assert len(out[0][2]) // 3 == 2 and len(out[1][2]) // 3 == 60
    if lamp:
        out.append((LAMP, *scenes.quad((-1, 0, 1), (1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, -1, 0)),
                    abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1.0, 0.9, 0.7), emissive_strength=12.0)))
    return out


def twins(rt, form, lamp=False, **settings):
    """Scenes A and B loaded alike; settings: top_level_build, light_table_build."""
    out = []
    for _ in range(2):
        sc = rt.Scene(0, instancing=form)
        if "top_level_build" in settings:
            sc.set_top_level_build(settings["top_level_build"])
        if "light_table_build" in settings:
            sc.set_light_table_build(settings["light_table_build"])
        for key, v, idx, mat in meshes(lamp):
            sc.add_mesh(key, v, idx, mat)
        out.append(sc)
    return out


def placed(n, seed, extent=6.0):
    """n affine transforms inside the camera's view."""
    return affine_transforms(n, seed, translation=extent)


def tensor_of(xf):
    import torch
    return torch.from_numpy(np.ascontiguousarray(xf, dtype=np.float32).reshape(-1, 12).copy()).to("cuda:0")


def split(layout, xf):
    """set_instances' argument of a layout [(key, count)] and its [n, 12] transforms."""
    out, at = [], 0
    for key, count in layout:
        out.append((key, list(xf[at:at + count])))
        at += count
    return out


def both(a, b, layout, xf, op=None):
    """The same instance list into A from numpy and into B from a tensor, with the same forced op."""
    if op is not None:
        a.force_next_op(op); b.force_next_op(op)
    a.set_instances(split(layout, xf))
    b.set_instances_device(layout, tensor_of(xf))


def fetch(sc):
    i = sc.instance_update_info()
    return (i.from_device, i.host_stale, i.host_fetches, i.fetch_reason)


@pytest.fixture(scope="module")
def rays(rt):
    """A fixed batch of 4 096 rays towards the instances: a 64 x 64 grid down -z from the camera's side."""
    xs, ys = np.meshgrid(np.linspace(-8, 8, 64), np.linspace(-8, 8, 64), indexing="ij")
    r = np.zeros(4096, dtype=abi.RAY)
    r["origin"] = np.stack([xs.ravel(), ys.ravel(), np.full(4096, 30.0)], axis=1)
    r["dir"] = (0.0, 0.0, -1.0)
    r["tmin"], r["tmax"] = 1e-3, 100.0
    return r, rt.rays_to_device(r)


def structure(sc):
    """The built structure as named arrays: the four arrays of the top level, or the one-level tree."""
    if sc.two_level():
        return dict(zip(("tl_nodes", "tl_inst", "tl_records", "tl_boxes"), sc.read_top_level()))
    return dict(zip(("bvh_nodes", "bvh_tris"), sc.read_bvh()))


def snapshot(rt, sc, rays):
    """Everything a refused call must leave alone and a twin must share: instance tables, structure, lights, query results."""
    r, rd = rays
    dev, flat = sc.read_instance_tables()
    out = {"dev_instances": dev, "flat_instances": flat, "lights": sc.read_lights()}
    out.update(structure(sc))
    out["closest"] = rt.hits_from_device(sc.trace_closest(rd, len(r))).view(np.uint32).copy()
    out["any"] = sc.trace_any(rd, len(r)).cpu().numpy().view(np.uint32).copy()
    return out


def canonical_nodes(nodes):
    """What two device builds of one tree share. The device builder numbers the inner nodes of a level in the order its threads
    take them from an atomic counter, so node indices and the references to inner nodes differ between two runs of the same
    build on the same input (test_gpu_tree_height_bound.canonical_nodes); the quantised boxes of every node (dwords 0..11), the
    leaf references and the number of inner references do not."""
    boxes = sorted(row.tobytes() for row in np.ascontiguousarray(nodes[:, :12]))
    refs = nodes[:, 12:].astype(np.uint32).reshape(-1)
    return boxes, np.sort(refs[refs >= 0x80000000]).tobytes(), int((refs < 0x80000000).sum())


def assert_snapshots_equal(want, got, what, nan_rule=(), device_built=False):
    """Byte for byte; the node array of a structure that each scene built on the device for itself up to the numbering of its
    inner nodes (everything else of it, leaf order included, byte for byte)."""
    assert want.keys() == got.keys(), what
    for name in want:
        if device_built and name in ("bvh_nodes", "tl_nodes"):
            assert want[name].shape == got[name].shape and canonical_nodes(want[name]) == canonical_nodes(got[name]), "%s: %s" % (what, name)
        elif name in nan_rule:
            assert_words_equal_nan_rule(want[name], got[name], "%s: %s" % (what, name))
        else:
            assert want[name].shape == got[name].shape, (what, name)
            assert_bits_equal(want[name], got[name], "%s: %s" % (what, name))


def raw_color(rt, sc, blue_noise):
    fr = rt.DeviceFrame(W, H, blue_noise)
    m = rt.camera_matrices(*CAMERA, W, H)
    sc.trace_ris(fr, m, 0); sc.trace_final(fr, m, 0)
    return fr.host()["raw_color"].copy()


def assert_twins_equal(rt, a, b, rays, blue_noise, what, hits=True, nan_rule=(), device_built=False):
    assert a.two_level() == b.two_level(), what
    sa, sb = snapshot(rt, a, rays), snapshot(rt, b, rays)
    if hits:
        assert (sa["closest"].view(abi.HIT)["t"] >= 0).mean() > 0.01, what
    assert_snapshots_equal(sa, sb, what, nan_rule, device_built)
    assert_bits_equal(raw_color(rt, a, blue_noise), raw_color(rt, b, blue_noise), "%s: raw_color of a RIS + final frame" % what)
    assert a.as_state()[1] == b.as_state()[1], what
    (sta, _), (stb, _) = a.as_state(), b.as_state()
    assert (sta.changing, sta.frames_without_changes, sta.number_of_updates_since_last_rebuild) == (stb.changing, stb.frames_without_changes, stb.number_of_updates_since_last_rebuild), what


# ---- 1. the kernel against the host rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_kernel_tables_equal_the_host_rule_plus_the_layout(rt, n):
    """One partial tile, one full tile, a tail across two and three blocks; every edge transform at the first and the last index.
    The tables are read behind a forced in-place update, which never fetches: they are the kernel's."""
    layout = [(QUAD, n)] if n == 1 else [(QUAD, n // 2), (SPHERE, n - n // 2)]
    slot = np.concatenate([np.full(c, k - 1, dtype=np.uint32) for k, c in layout])              # keys 1, 2 took slots 0, 1
    tri_offset = np.concatenate([[0], np.cumsum(np.where(slot == 0, 2, 60))[:-1]]).astype(np.uint32)
    a, b = twins(rt, "flat")
    base = placed(n, 100 + n)
    a.set_instances(split(layout, base)); b.set_instances(split(layout, base))
    xf = base
    for name, edge in edge_transforms().items():
        xf = base.copy()
        xf[0] = edge; xf[-1] = edge
        b.force_next_op(abi.OP_UPDATE)
        b.set_instances_device(layout, tensor_of(xf))
        assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE) and b.as_state()[1] == abi.OP_UPDATE, name
        dev, flat = b.read_instance_tables()
        assert len(dev) == len(flat) == n
        assert_words_equal_nan_rule(host_tables(xf), dev, "%d instances, %s: DevInstance" % (n, name))
        assert_bits_equal(xf, flat["o2w"], "%d instances, %s: FlatInstance.o2w" % (n, name))
        assert np.array_equal(flat["tri_offset"], tri_offset) and np.array_equal(flat["mesh_slot"], slot) and (flat["_pad"] == 0).all(), name
    a.force_next_op(abi.OP_UPDATE)
    a.set_instances(split(layout, xf))
    (da, fa), (db, fb) = a.read_instance_tables(), b.read_instance_tables()
    assert_words_equal_nan_rule(da, db, "%d instances: DevInstance against the twin" % n)
    assert_bits_equal(fa, fb, "%d instances: FlatInstance against the twin" % n)
    a.close(); b.close()


# ---- 2. refusal on the device -----------------------------------------------------------------------------------------------------
def test_non_finite_components_are_refused_and_the_scene_stays(rt, rays):
    import torch
    n = 257
    layout = [(QUAD, 200), (SPHERE, 54), (LAMP, 3)]
    a, b = twins(rt, "flat", lamp=True)
    xf = placed(n, 7)
    both(a, b, layout, xf)
    before, info0 = snapshot(rt, b, rays), fetch(b)
    good = tensor_of(xf)

    def refused_like_the_host(pokes, bad_index, what):
        bad_np, bad_t = xf.copy(), good.clone()
        for i, c, value in pokes:
            bad_np[i, c] = value
            bad_t[i, c] = float(value)
        with pytest.raises(rt.SunrayError) as want:
            a.set_instances(split(layout, bad_np))
        with pytest.raises(rt.SunrayError) as got:
            b.set_instances_device(layout, bad_t)
        assert (got.value.code, got.value.description) == (want.value.code, want.value.description) == (ERR_INVALID_ARG, NON_FINITE_TEXT), what
        assert b.instance_update_info().bad_index == bad_index and fetch(b) == info0, what
        assert_snapshots_equal(before, snapshot(rt, b, rays), "after a refused " + what)
    for value in (np.float32("nan"), np.float32("inf"), np.float32("-inf")):
        for c in range(12):
            for i in (0, n - 1):
                refused_like_the_host([(i, c, value)], i, "%s in component %d of instance %d" % (value, c, i))
    refused_like_the_host([(200, 3, np.float32("nan")), (77, 10, np.float32("inf")), (256, 0, np.float32("-inf"))], 77, "three bad instances")
    torch.cuda.synchronize()
    # the scene still takes the good list, and equals the twin
    both(a, b, layout, xf)
    assert b.instance_update_info().bad_index == 0xFFFFFFFF
    assert_snapshots_equal(snapshot(rt, a, rays), snapshot(rt, b, rays), "the good list after the refusals")
    a.close(); b.close()


# ---- 3. refusals the host decides -------------------------------------------------------------------------------------------------
def test_pointer_refusals_are_decided_on_the_host(rt, hip, rays):
    import torch
    from sunray_amd._lib import lib
    n = 257
    layout = [(QUAD, 200), (SPHERE, 57)]
    a, b = twins(rt, "flat")
    xf = placed(n, 9)
    both(a, b, layout, xf)
    before, info0 = snapshot(rt, b, rays), fetch(b)
    keys, counts = np.array([QUAD, SPHERE], dtype=np.uint64), np.array([200, 57], dtype=np.uint32)

    def raw(ptr, keys=keys, counts=counts):
        rc = lib().sr_scene_set_instances_device(b._h, keys.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.c_uint32(len(keys)), C.c_void_p(ptr), None)
        return rc, lib().sr_last_error().decode()

    def unchanged(what):
        assert fetch(b) == info0, what
        assert_snapshots_equal(before, snapshot(rt, b, rays), "after a refused " + what)
    host = np.ascontiguousarray(xf)
    rc, text = raw(host.ctypes.data)
    assert rc == ERR_INVALID_ARG and "not device memory of the scene's device" in text, text
    unchanged("host pointer")
    room = torch.zeros(n * 12 + 4, dtype=torch.float32, device="cuda:0")
    shifted = room[1:1 + n * 12]
    shifted.copy_(tensor_of(xf).reshape(-1))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(rt.SunrayError) as e:
        b.set_instances_device(layout, shifted)
    assert e.value.code == ERR_INVALID_ARG and "16-byte aligned" in e.value.description
    unchanged("misaligned pointer")
    short = C.c_void_p()
    assert hip.hipSetDevice(C.c_int(0)) == 0 and hip.hipMalloc(C.byref(short), C.c_size_t((n - 1) * 48)) == 0      # one transform short
    try:
        rc, text = raw(short.value)
        assert rc == ERR_INVALID_ARG and "not device memory of the scene's device for that many instances" in text, text
    finally:
        assert hip.hipFree(short) == 0
    unchanged("tensor one transform short")
    with pytest.raises(ValueError):
        b.set_instances_device(layout, tensor_of(xf[:-1]))                       # the wrapper sees it first
    with pytest.raises(rt.SunrayError) as want:
        a.set_instances([(12345, list(xf))])
    with pytest.raises(rt.SunrayError) as got:
        b.set_instances_device([(12345, n)], tensor_of(xf))
    assert (got.value.code, got.value.description) == (want.value.code, want.value.description) and got.value.code == ERR_INVALID_ARG
    unchanged("unknown key")
    # a null pointer with instances, and null arrays, in the host call's words
    rc, text = raw(None)
    assert rc == ERR_INVALID_ARG and text == "frame_instance_data: transforms is null but instances were given"
    unchanged("null pointer")
    b.set_instances_device(layout, tensor_of(xf))                                # and the scene still takes a good list
    a.close(); b.close()


# ---- 4. twin equality along every downstream path ---------------------------------------------------------------------------------
def test_one_level_host_build_fetches_once(rt, rays, blue_noise):
    a, b = twins(rt, "flat")
    layout, xf = [(QUAD, 3), (SPHERE, 5)], placed(8, 21)
    both(a, b, layout, xf)
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_HOST_BUILD) and b.as_state()[1] == abi.OP_SLOW_BUILD
    assert_twins_equal(rt, a, b, rays, blue_noise, "one-level, 8 instances, host build")
    a.close(); b.close()


def test_one_level_device_fast_build_and_update_never_fetch(rt, rays, blue_noise):
    a, b = twins(rt, "flat")
    layout = [(SPHERE, 80)]                                                       # 4 800 triangles: the device fast build takes them
    both(a, b, layout, placed(80, 31))
    assert fetch(b)[2:] == (1, abi.INST_FETCH_HOST_BUILD)
    both(a, b, layout, placed(80, 32), abi.OP_FAST_BUILD)
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE) and b.as_state()[1] == abi.OP_FAST_BUILD and b.instance_update_info().layout_rebuilt == 0
    assert_twins_equal(rt, a, b, rays, blue_noise, "one-level, 80 x 60 triangles, device fast build", device_built=True)
    both(a, b, layout, placed(80, 33), abi.OP_UPDATE)
    assert b.as_state()[1] == abi.OP_UPDATE
    structure(b); snapshot(rt, b, rays)                                           # the read-backs of the device side fetch nothing
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    assert_twins_equal(rt, a, b, rays, blue_noise, "one-level, forced update", device_built=True)
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    a.close(); b.close()


def standing_two_level(rt, mode, layout, n, seed, lamp=False, **settings):
    """Twins that stand in the two-level form (the first list is the quality build on the host, which fetches)."""
    a, b = twins(rt, "two_level", lamp=lamp, top_level_build=mode, **settings)
    both(a, b, layout, placed(n, seed))
    assert a.two_level() and b.two_level() and b.top_level_info().on_device == 0
    assert fetch(b)[2] == 1
    return a, b


def test_two_level_device_build_never_fetches(rt, rays, blue_noise):
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = standing_two_level(rt, "device", layout, 300, 41)
    both(a, b, layout, placed(300, 42))
    assert b.top_level_info().on_device == 1 and a.top_level_info().on_device == 1
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    assert_twins_equal(rt, a, b, rays, blue_noise, "two-level, device top-level build, 300 instances", device_built=True)
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    a.close(); b.close()


def test_two_level_host_build_fetches_once(rt, rays, blue_noise):
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = standing_two_level(rt, "host", layout, 300, 43)
    both(a, b, layout, placed(300, 44))
    assert (b.top_level_info().on_device, b.top_level_info().reason) == (0, abi.TL_HOST_MODE)
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_HOST_TOP_LEVEL)
    assert_twins_equal(rt, a, b, rays, blue_noise, "two-level, host top-level build")
    a.close(); b.close()


def test_two_level_baked_instance_goes_to_the_host(rt, rays, blue_noise):
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = standing_two_level(rt, "device", layout, 300, 45)
    xf = placed(300, 46)
    xf[150].reshape(3, 4)[:, 1] = 0.0                                             # a zero scale on one axis: no inverse, a baked copy
    both(a, b, layout, xf)
    assert (b.top_level_info().on_device, b.top_level_info().reason) == (0, abi.TL_HOST_BAKED_INSTANCE)
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_HOST_TOP_LEVEL)
    assert b.read_top_level()[2]["flags"][150] == 1
    assert_twins_equal(rt, a, b, rays, blue_noise, "two-level, one baked instance", nan_rule=("dev_instances",))
    a.close(); b.close()


@pytest.mark.parametrize("lights", ["host", "device"])
def test_light_table_of_an_instanced_emissive_quad(rt, rays, blue_noise, lights):
    layout = [(QUAD, 100), (SPHERE, 197), (LAMP, 3)]
    a, b = standing_two_level(rt, "device", layout, 300, 47, lamp=True, light_table_build=lights)
    both(a, b, layout, placed(300, 48))
    assert b.top_level_info().on_device == 1 and len(b.read_lights()) == 6
    assert b.light_table_info().on_device == (1 if lights == "device" else 0)
    assert fetch(b) == ((1, 1, 0, abi.INST_FETCH_NONE) if lights == "device" else (1, 0, 1, abi.INST_FETCH_HOST_LIGHT_TABLE))
    assert_twins_equal(rt, a, b, rays, blue_noise, "lights built on the %s" % lights, device_built=True)
    a.close(); b.close()


# ---- 5. the layout is reused ------------------------------------------------------------------------------------------------------
def test_layout_is_rebuilt_only_when_keys_or_counts_change(rt, rays, blue_noise):
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = standing_two_level(rt, "device", layout, 300, 51)
    assert b.instance_update_info().layout_rebuilt == 1
    both(a, b, layout, placed(300, 52))
    assert b.instance_update_info().layout_rebuilt == 0
    assert_twins_equal(rt, a, b, rays, blue_noise, "the same layout, new transforms", device_built=True)
    changed = [(QUAD, 120), (SPHERE, 180)]
    both(a, b, changed, placed(300, 53))
    assert b.instance_update_info().layout_rebuilt == 1
    assert_twins_equal(rt, a, b, rays, blue_noise, "changed counts", device_built=True)
    # the host entry point keeps the record too: the same layout through it leaves the device's copy of the layout current
    a.set_instances(split(changed, placed(300, 54))); b.set_instances(split(changed, placed(300, 54)))
    both(a, b, changed, placed(300, 55))
    assert b.instance_update_info().layout_rebuilt == 0
    assert_twins_equal(rt, a, b, rays, blue_noise, "after a host call in between", device_built=True)
    a.close(); b.close()


# ---- 6. the stale host copy -------------------------------------------------------------------------------------------------------
def test_get_tables_fetches_the_stale_host_copy_once(rt):
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = standing_two_level(rt, "device", layout, 300, 61)
    xf = placed(300, 62)
    both(a, b, layout, xf)
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    assert_bits_equal(xf, b.tables()["transforms"].view(np.float32).reshape(-1, 12), "transforms of get_tables")
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_GET_TABLES) and b.instance_update_info().fetch_ms > 0
    b.tables()
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_GET_TABLES)
    both(a, b, layout, placed(300, 63))
    assert fetch(b)[1] == 1
    b.set_instances(split(layout, xf))
    assert fetch(b) == (0, 0, 0, abi.INST_FETCH_NONE)
    a.close(); b.close()


# ---- 7. the settle rebuild --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["flat", "two_level"])
def test_settle_rebuild_after_a_device_call_equals_the_twins(rt, rays, blue_noise, form):
    layout = [(SPHERE, 80)]
    a, b = twins(rt, form, top_level_build="device")
    both(a, b, layout, placed(80, 71))
    both(a, b, layout, placed(80, 72), abi.OP_UPDATE if form == "flat" else None)
    assert fetch(b) == (1, 1, 0, abi.INST_FETCH_NONE)
    for _ in range(16):
        a.end_frame(); b.end_frame()
    assert a.as_state()[1] == b.as_state()[1] == abi.OP_SLOW_BUILD
    assert fetch(b) == (1, 0, 1, abi.INST_FETCH_SETTLE)
    assert_twins_equal(rt, a, b, rays, blue_noise, "settle rebuild, %s" % form)
    a.close(); b.close()


# ---- 8. with a deforming mesh -----------------------------------------------------------------------------------------------------
def test_deforming_mesh_and_device_instances_in_one_step(rt, rays, blue_noise):
    import torch
    layout = [(QUAD, 100), (SPHERE, 200)]
    a, b = twins(rt, "two_level", top_level_build="device")
    for sc in (a, b):
        sc.set_mesh_build_type(SPHERE, abi.BUILD_RAPIDLY_CHANGING)
    both(a, b, layout, placed(300, 81))
    v, idx = scenes.uv_sphere(1.0, 6, 6)
    for step in (1, 2):
        moved = scenes.deform_vertices(v, idx, 0.5 * step)
        a.update_mesh(SPHERE, moved)
        b.update_mesh_device(SPHERE, torch.from_numpy(np.ascontiguousarray(moved, dtype=abi.VERTEX).view(np.uint8).copy()).to("cuda:0"))
        both(a, b, layout, placed(300, 81 + step))
        ia, ib = a.mesh_update_info(), b.mesh_update_info()
        assert (ia.blas_refitted, ia.blas_rebuilt) == (ib.blas_refitted, ib.blas_rebuilt)
        assert fetch(b)[0] == 1
        ta, tb = a.read_mesh_tree(SPHERE), b.read_mesh_tree(SPHERE)
        for name in ("nodes", "tris", "shade"):
            assert_bits_equal(ta[name], tb[name], "step %d: sphere tree %s" % (step, name))
        assert_twins_equal(rt, a, b, rays, blue_noise, "deforming sphere and device instances, step %d" % step, device_built=True)
    a.close(); b.close()


# ---- 9. the renderer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_renderer_frames_equal_with_moving_device_transforms(rt, hip, devices):
    layout = [(QUAD, 10), (SPHERE, 20), (LAMP, 2)]
    made = []
    for _ in range(2):
        r = rt.Renderer((W, H)) if devices is None else rt.Renderer((W, H), devices=devices)
        for key, v, idx, mat in meshes(lamp=True):
            r.load_mesh(key, v, idx, mat)
        made.append(r)
    ra, rb = made
    base = placed(32, 91, extent=4.0)
    for f in range(3):
        xf = base.copy()
        xf[:, 3] += np.float32(0.25 * f)
        ra.wait_frame(ra.render(CAMERA, split(layout, xf)))
        rb.wait_frame(rb.render_device_transforms(CAMERA, layout, tensor_of(xf)))
        (oa, raw_a), (ob, raw_b) = grab(rt, hip, ra), grab(rt, hip, rb)
        assert_equal(oa, ob, "RGBA8 of frame %d" % f)
        assert_equal(raw_a, raw_b, "raw_color of frame %d" % f)
        assert len(np.unique(oa)) > 8
    ra.close(); rb.close()
