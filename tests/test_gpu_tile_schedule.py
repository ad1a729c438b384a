"""The passes' tile schedule on the device. The two per-pixel passes render the tile a list tells them to, and the list is
derived (tile_order_kernel) from the measured cost of the previous launch: the one input of the pass path a test cannot
steer through the passes themselves. Here cost maps are injected (Scene.set_tile_costs) and the derived order is read back
(Scene.tile_order):
  * the kernel against the plain reference (tests/tile_schedule_reference.py) at the shapes where it takes another path
    and at cost maps that drive the band cuts into every clamp: first the invariants that make every pixel render exactly
    once (so a failure names the broken one), then equality of the whole array;
  * the passes under injected schedules: rendered bits must not depend on the order;
  * the hooks' argument errors.
Run on an MI355X with:  python -m pytest tests/test_gpu_tile_schedule.py -m gpu -q -s
"""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(__file__))
import tile_schedule_reference as ref  # noqa: E402


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (-m gpu on a machine with an MI355X)")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def bare_scene(rt):
    """A scene without geometry: the schedule hooks need neither a frame nor a structure. Its eight schedule entries are
    recycled over the shapes below, as launches of many geometries recycle them."""
    return rt.Scene(0)


def assert_bits_equal(a, b, what):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    b = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    nd = int((a != b).sum())
    assert nd == 0, "%s: %d of %d bytes differ" % (what, nd, a.size)


# ---- kernel against reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles_x,tiles_y", ref.SHAPES)
def test_tile_order_equals_reference(rt, bare_scene, tiles_x, tiles_y):
    w, h = ref.extent(tiles_x, tiles_y)                   # both extents ragged
    assert abi.TILE_ORDER_NONE == ref.NONE
    cases = mismatches = 0
    failures = []
    for k, (name, costs) in enumerate(ref.cost_maps(tiles_x, tiles_y)):
        which = k & 1
        bare_scene.set_tile_costs(which, 0, w, 0, h, costs)
        assert np.array_equal(bare_scene.tile_costs(which, w, 0, h), costs), "%s: the injected costs are not the schedule's costs" % name
        lists, cap = bare_scene.tile_order(which, 0, w, 0, h)
        assert cap == ref.order_cap(w, h), "%s: order_cap %d, reference %d" % (name, cap, ref.order_cap(w, h))
        b = ref.check_invariants(lists, cap, tiles_x, tiles_y)
        if (tiles_x, tiles_y) in ref.CLAMP_SHAPES and name in ref.CLAMP_MAPS:     # the inputs still reach the clamps
            wd = ref.widths(b)
            assert max(wd) == ref.cap_cols(tiles_x) and min(wd) == 1, (name, wd)
        expect = ref.order(costs, tiles_x, tiles_y)
        cases += 1
        if not np.array_equal(lists, expect):
            mismatches += 1
            failures.append("%s: cuts %s, reference %s; %d entries differ" % (name, b, ref.bands(costs, tiles_x, tiles_y), int((lists != expect).sum())))
    print("tile schedule (%d, %d): %d cases, %d mismatches" % (tiles_x, tiles_y, cases, mismatches))
    assert not failures, failures


def test_tile_order_of_a_rectangle_and_both_passes_are_separate_entries(rt, bare_scene):
    """x0 / y0 and the pass are part of the geometry an order belongs to: four entries of one extent keep four orders."""
    tiles_x, tiles_y = 17, 5
    w, h = ref.extent(tiles_x, tiles_y)
    maps = dict(ref.cost_maps(tiles_x, tiles_y))
    keys = [(0, 0, 0, "col0"), (1, 0, 0, "colLast"), (0, 37, 3, "colMid"), (1, 37, 3, "lastRow")]
    for which, x0, y0, name in keys:
        bare_scene.set_tile_costs(which, x0, w, y0, h, maps[name])
    for which, x0, y0, name in keys:
        lists, cap = bare_scene.tile_order(which, x0, w, y0, h)
        ref.check_invariants(lists, cap, tiles_x, tiles_y)
        assert np.array_equal(lists, ref.order(maps[name], tiles_x, tiles_y)), name


# ---- the passes under an injected schedule --------------------------------------------------------------------------------
INJECTED = ("col0", "colLast", "colMid", "lastRow", "tileRowMid")


def fill_ff(arrays, W, H, x0, x1, y0, y1, torch=None):
    """0xFF bytes into the rectangle's pixels of per-pixel buffers (numpy arrays, or torch tensors)."""
    for a in arrays:
        if torch is None:
            a.view(np.uint8).reshape(H, W, -1)[y0:y1, x0:x1] = 0xFF
        else:
            (a.view(torch.int32) if a.dtype == torch.float32 else a).view(H, W, -1)[y0:y1, x0:x1] = -1


@pytest.mark.parametrize("W,H,tile", [(130, 17, None), (200, 24, (3, 17, 37, 130))], ids=["full_130x17", "rect_130x17_at_37_3_in_200x24"])
def test_passes_equal_oracle_under_injected_schedules(rt, oracle, blue_noise, W, H, tile):
    """Three consecutive frames of the Cornell box (temporal and spatial reuse read real history), a different adversarial
    cost map injected before every launch of either pass: every buffer equals the oracle's bit for bit, i.e. no tile is
    dropped or rendered twice whatever the order. 17 x 3 tiles with a last column 2 pixels wide and a last row 1 pixel high;
    once as the full frame, once as a launch rectangle whose x0 / y0 are no multiples of 8 inside a larger frame (only the
    rectangle is compared). The rectangle's pixels of all output buffers start as 0xFF bytes on both sides, so a dropped
    tile cannot pass by leaving zeros where the oracle wrote zeros (outside the rectangle the buffers stay zero: spatial
    reuse reads those pixels, and what it makes of NaN records is not what this test is about). After each launch the
    order the launch itself derived from the measured costs must keep the invariants."""
    import torch
    desc = scenes.cornell_box()
    y0, rows, x0, cols = tile if tile else (0, H, 0, W)
    x1, y1 = x0 + cols, y0 + rows
    tiles_x, tiles_y = ref.tiles(cols, rows)
    assert (tiles_x, tiles_y) == (17, 3)
    maps = dict(ref.cost_maps(tiles_x, tiles_y))
    osc, gsc = oracle.OracleScene().load(desc), rt.Scene(0).load(desc)
    of, gf = oracle.HostFrame(W, H, blue_noise), rt.DeviceFrame(W, H, blue_noise)
    fill_ff([of.raw_color, of.depth, of.normal, of.diffuse, of.motion] + of.reservoirs + of.reservoirs_gi, W, H, x0, x1, y0, y1)
    fill_ff([gf.raw_color, gf.depth, gf.normal, gf.diffuse, gf.motion] + gf.reservoirs + gf.reservoirs_gi + ([gf.primary] if gf.primary is not None else []),
            W, H, x0, x1, y0, y1, torch)
    cfg = abi.SrTraceConfig.reference()
    injected = 0
    prev = None
    rect = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(H, W, -1)[y0:y1, x0:x1]
    for f in range(3):
        om = oracle.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        gm = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H, prev)
        assert bytes(om) == bytes(gm)
        prev = list(om.view_proj)
        problems = []                    # everything wrong with this frame, so that a failure shows the broken invariant AND its effect

        def check(what, fn, *args):
            try:
                fn(*args)
            except AssertionError as e:
                problems.append("f%d %s: %s" % (f, what, next((ln for ln in str(e).splitlines() if ln.strip()), "differs")))

        for which in (0, 1):
            name = INJECTED[injected % len(INJECTED)]
            injected += 1
            gsc.set_tile_costs(which, x0, cols, y0, rows, maps[name])
            lists, cap = gsc.tile_order(which, x0, cols, y0, rows)
            assert cap == ref.order_cap(cols, rows)
            check("pass %d, injected %s" % (which, name), ref.check_invariants, lists, cap, tiles_x, tiles_y)
            check("pass %d, injected %s, against the reference" % (which, name), np.testing.assert_array_equal, lists, ref.order(maps[name], tiles_x, tiles_y))
            (osc.trace_final if which else osc.trace_ris)(of, om, f, cfg, tile=tile)
            (gsc.trace_final if which else gsc.trace_ris)(gf, gm, f, cfg, tile=tile)
            lists, cap = gsc.tile_order(which, x0, cols, y0, rows)      # re-derived by the launch from the costs it measured
            check("pass %d, order from the measured costs" % which, ref.check_invariants, lists, cap, tiles_x, tiles_y)
        h = gf.host()
        cur = f & 1
        for what, a, b in (("depth_img", of.depth, h["depth"]), ("normal_img", of.normal, h["normal"]), ("diffuse_img", of.diffuse, h["diffuse"]),
                           ("motion_vec_img", of.motion, h["motion"]), ("reservoirs", of.reservoirs[cur], h["reservoirs"][cur]),
                           ("reservoirs_gi", of.reservoirs_gi[cur], h["reservoirs_gi"][cur]), ("raw_color", of.raw_color, h["raw_color"])):
            check(what, assert_bits_equal, rect(a), rect(b), what)
        assert np.isfinite(np.ascontiguousarray(rect(of.raw_color)).view(np.float32)).all(), "the oracle's raw_color f%d is not finite" % f
        assert not problems, problems
    assert injected == 6


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_schedule_hooks_refuse_bad_arguments(rt, bare_scene):
    import ctypes as C
    from sunray_amd._lib import SunrayError, lib
    tiles_x, tiles_y = 9, 4
    w, h = ref.extent(tiles_x, tiles_y)
    costs = np.zeros(tiles_x * tiles_y, dtype=np.uint32)
    sc = rt.Scene(0)
    with pytest.raises(SunrayError, match="no order"):                       # nothing derived yet
        sc.tile_order(0, 0, w, 0, h)
    for n in (tiles_x * tiles_y - 1, tiles_x * tiles_y + 1, 1):
        with pytest.raises(SunrayError, match="number of 8x8 tiles"):
            sc.set_tile_costs(0, 0, w, 0, h, np.zeros(n, dtype=np.uint32))
    with pytest.raises(SunrayError, match="null"):
        sc.set_tile_costs(0, 0, w, 0, h, None)
    with pytest.raises(SunrayError, match="null"):
        check_rc(lib().sr_scene_set_tile_costs(None, 0, C.c_uint32(0), C.c_uint32(w), C.c_uint32(0), C.c_uint32(h), costs.ctypes.data_as(C.c_void_p), C.c_uint32(len(costs))))
    for args in ((0, 0, 0, 0, h), (0, 0, w, 0, 0),                           # no columns / no rows: the passes refuse an unset extent
                 (2, 0, w, 0, h), (-1, 0, w, 0, h),                          # no such pass
                 (0, 1 << 16, w, 1 << 15, h),                                # an image holding it has 2^31 pixels or more
                 (0, 0xFFFFFFFF, w, 0, h)):
        with pytest.raises(SunrayError):
            sc.set_tile_costs(*args, costs)
        with pytest.raises(SunrayError):
            sc.tile_order(*args)
    with pytest.raises(SunrayError, match="no order"):                       # none of the refused calls left an order behind
        sc.tile_order(0, 0, w, 0, h)
    sc.set_tile_costs(0, 0, w, 0, h, costs)
    sc.tile_order(0, 0, w, 0, h)
    for other in ((1, 0, w, 0, h), (0, 8, w, 0, h), (0, 0, w, 8, h), (0, 0, w + 8, 0, h), (0, 0, w, 0, h + 8)):
        with pytest.raises(SunrayError, match="no order"):                   # another pass or rectangle has none
            sc.tile_order(*other)
    out, cap = np.zeros(4, dtype=np.uint32), C.c_uint32()
    with pytest.raises(SunrayError, match="too small"):
        check_rc(lib().sr_scene_read_tile_order(sc._h, 0, C.c_uint32(0), C.c_uint32(w), C.c_uint32(0), C.c_uint32(h), out.ctypes.data_as(C.c_void_p), C.c_uint32(4), C.byref(cap)))
    assert cap.value == ref.order_cap(w, h) and not out.any()
    with pytest.raises(SunrayError, match="null"):
        check_rc(lib().sr_scene_read_tile_order(sc._h, 0, C.c_uint32(0), C.c_uint32(w), C.c_uint32(0), C.c_uint32(h), None, C.c_uint32(1 << 20), C.byref(cap)))


def check_rc(rc):
    from sunray_amd._lib import check
    check(rc)


def test_injected_costs_do_not_count_as_a_launch(rt, blue_noise):
    """A launch re-derives the order after each of the first four uses of a geometry and then every 64th: injecting costs is
    no use. After four launches and any number of injections the fifth launch leaves the injected order in place."""
    desc = scenes.cornell_box()
    W, H = 130, 17
    tiles_x, tiles_y = ref.tiles(W, H)
    maps = dict(ref.cost_maps(tiles_x, tiles_y))
    gsc, gf = rt.Scene(0).load(desc), rt.DeviceFrame(W, H, blue_noise)
    m = rt.camera_matrices(desc.camera_pos, desc.camera_target, desc.fov_y, W, H)
    for k in range(4):
        for name in INJECTED:
            gsc.set_tile_costs(0, 0, W, 0, H, maps[name])
        gsc.trace_ris(gf, m, 0)
        lists, cap = gsc.tile_order(0, 0, W, 0, H)
        ref.check_invariants(lists, cap, tiles_x, tiles_y)
        measured = gsc.tile_costs(0, W, 0, H)
        assert measured.all() and not np.array_equal(measured, maps[INJECTED[-1]])      # the launch measured every tile ...
        assert np.array_equal(lists, ref.order(measured, tiles_x, tiles_y)), "launch %d: order not derived from the measured costs" % k
    gsc.set_tile_costs(0, 0, W, 0, H, maps["col0"])
    gsc.trace_ris(gf, m, 0)
    lists, cap = gsc.tile_order(0, 0, W, 0, H)
    assert np.array_equal(lists, ref.order(maps["col0"], tiles_x, tiles_y))
