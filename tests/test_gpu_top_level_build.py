"""The top level of the two-level form built on the device when the instance list of a standing two-level scene changes
(sr_scene_set_top_level_build, SR_TL_BUILD; csrc/bvh_gpu.hip srk_tl_records / srk_tl_build) against the host path, which is
unchanged: instance records and padded boxes byte for byte, the device-built tree checked structurally (every instance once,
leaf size, conservative quantised boxes on every ancestor, stack budget), queries against the oracle's brute force, frames
against the oracle bit for bit, the fallbacks to the host, and the 10 000 x 10 080-triangle scene. Every scene is built once
with mode HOST and once with mode DEVICE, and top_level_info says which path really ran."""
import os
import re
import sys
import time

import numpy as np
import pytest

from sunray_amd import abi, scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_multi_renderer import assert_equal, grab, load  # noqa: E402
from test_gpu_parity import assert_bits_equal, ref_any, ref_closest  # noqa: E402
from test_gpu_two_level import frames_equal_oracle  # noqa: E402
from test_oracle_trace import camera_rays, random_rays  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAF_MAX = int(re.search(r"#define SR_LEAF_MAX (\d+)", open(os.path.join(ROOT, "sunray_amd", "csrc", "bvh_layout.h")).read()).group(1))


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def hip():
    import ctypes as C
    import torch  # noqa: F401  (the HIP runtime torch loaded)
    return C.CDLL("libamdhip64.so")


def affine_transforms(n, seed, translation=1.0e4, identical=False):
    """n general affine 3x4 transforms: rotation about an arbitrary axis, per-axis scales within a factor of three, a shear,
    translations up to `translation`. `identical`: n copies of the first."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    S = np.zeros((n, 3, 3))
    sc = rng.uniform(0.5, 1.5, size=(n, 3))
    for a in range(3):
        S[:, a, a] = sc[:, a]
    S[:, 0, 1] = rng.uniform(-0.2, 0.2, size=n) * sc[:, 0]
    S[:, 1, 2] = rng.uniform(-0.2, 0.2, size=n) * sc[:, 1]
    t = rng.uniform(-translation, translation, size=(n, 3))
    xf = np.concatenate([R @ S, t[:, :, None]], axis=2).astype(np.float32).reshape(n, 12)
    if identical:
        xf[:] = xf[0]
    return xf


def small_mesh_scene(rt, xf, mode):
    """A standing two-level scene of one 60-triangle mesh whose current instance list is `xf`, set as a CHANGED list (the
    first list, one instance fewer, is the quality build on the host)."""
    v, idx = scenes.uv_sphere(1.0, 6, 6)
    sc = rt.Scene(0, instancing="two_level").set_top_level_build(mode)
    sc.add_mesh(1, v, idx, abi.material())
    sc.set_instances([(1, xf[:-1] if len(xf) > 1 else xf)])
    assert sc.two_level() and not sc.top_level_info().on_device
    sc.set_instances([(1, xf)])
    return sc


def assert_path(sc, mode, reason=None):
    info = sc.top_level_info()
    if mode == "device" and reason is None:
        assert info.on_device == 1 and info.reason == abi.TL_ON_DEVICE, "expected a device build, host reason %d" % info.reason
    else:
        want = reason if reason is not None else abi.TL_HOST_MODE
        assert info.on_device == 0 and info.reason == want, "expected the host path with reason %d, got on_device %d reason %d" % (want, info.on_device, info.reason)
    return info


# ---- 0. the switch ---------------------------------------------------------------------------------------------------
def test_sr_tl_build_is_read_when_a_scene_is_created(rt, monkeypatch):
    """SR_TL_BUILD = host | device | auto, read at sr_scene_create like SR_INSTANCING; an unknown value means auto; the call
    overrides it per scene."""
    for value, mode in (("host", abi.TL_BUILD_HOST), ("device", abi.TL_BUILD_DEVICE), ("auto", abi.TL_BUILD_AUTO), ("gpu", abi.TL_BUILD_AUTO), ("", abi.TL_BUILD_AUTO)):
        monkeypatch.setenv("SR_TL_BUILD", value)
        sc = rt.Scene(0)
        info = sc.top_level_info()
        assert info.mode == mode and info.on_device == 0 and info.reason == abi.TL_HOST_NOT_TWO_LEVEL and info.auto_threshold >= 2
        assert info.auto_threshold & (info.auto_threshold - 1) == 0          # a power of two
        sc.set_top_level_build("device")
        assert sc.top_level_info().mode == abi.TL_BUILD_DEVICE
        with pytest.raises(rt.SunrayError):
            sc.read_top_level()                                            # nothing stands in the two-level form
        sc.close()
    monkeypatch.delenv("SR_TL_BUILD")
    sc = rt.Scene(0)
    assert sc.top_level_info().mode == abi.TL_BUILD_AUTO
    import ctypes as C
    from sunray_amd._lib import lib
    assert lib().sr_scene_set_top_level_build(sc._h, C.c_uint32(3)) == -1 and sc.top_level_info().mode == abi.TL_BUILD_AUTO


# ---- 1. records ------------------------------------------------------------------------------------------------------
def both_modes(rt, build):
    out = {}
    for mode in ("host", "device"):
        sc = build(mode)
        info = assert_path(sc, mode)
        out[mode] = (sc, info, sc.read_top_level())
    return out


def assert_records_equal(out, what):
    (_, hi, (_, _, hrec, hbox)), (_, di, (_, _, drec, dbox)) = out["host"], out["device"]
    assert (hi.n_instances, hi.n_boxes, hi.blas_stack) == (di.n_instances, di.n_boxes, di.blas_stack)
    assert len(hrec) == len(drec) == hi.n_instances
    nd = int((hrec.view(np.uint32).reshape(len(hrec), 32) != drec.view(np.uint32).reshape(len(drec), 32)).any(axis=1).sum())
    assert nd == 0 and hrec.tobytes() == drec.tobytes(), "%s: %d of %d instance records differ" % (what, nd, len(hrec))
    nd = int((hbox.view(np.uint32) != dbox.view(np.uint32)).any(axis=1).sum())
    assert nd == 0, "%s: %d of %d instance boxes differ" % (what, nd, len(hbox))
    assert int(np.isfinite(hbox).all(axis=1).sum()) == hi.n_boxes


def test_records_and_boxes_equal_the_hosts_byte_for_byte(rt):
    desc = scenes.instanced_field(60, nonuniform=True)

    def field(mode):
        sc = rt.Scene(0, instancing="two_level").set_top_level_build(mode).load(desc)
        sc.set_instances(desc.instances)
        return sc
    out = both_modes(rt, field)
    assert_records_equal(out, "instanced_field(60)")
    assert out["host"][1].n_instances == 65 and out["host"][1].n_boxes == 65
    xf = affine_transforms(5000, 17)
    out = both_modes(rt, lambda mode: small_mesh_scene(rt, xf, mode))
    assert_records_equal(out, "5 000 affine instances")
    rec = out["device"][2][2]
    assert np.array_equal(rec["o2w"], xf) and (rec["flags"] == 0).all() and (rec["pad_a"] > 0).all() and (rec["pad_b"] > 0).all()
    # the records invert the transforms: w2o * o2w = identity to fp32 rounding (condition numbers here are below 10)
    M = xf.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    Winv = rec["w2o"].reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    assert np.abs(Winv @ M - np.eye(3)).max() < 1e-5


# ---- 2. structure ----------------------------------------------------------------------------------------------------
def check_structure(rt, sc, what):
    """Decodes the top-level tree and checks it against the instance boxes; returns the worst-case depth-first stack."""
    info = sc.top_level_info()
    nodes, tl_inst, _, boxes = sc.read_top_level()
    has_box = np.isfinite(boxes).all(axis=1)
    assert info.n_boxes == int(has_box.sum()) == len(tl_inst)
    assert np.array_equal(np.sort(tl_inst), np.nonzero(has_box)[0]), "%s: the leaf order is not a permutation of the instances with a box" % what
    n = len(nodes)
    assert n == info.n_nodes and n >= 1
    decoded = [rt.decode_node(nodes[i]) for i in range(n)]
    # breadth-first order from the root: every node is reached exactly once
    order, seen = [0], np.zeros(n, dtype=bool)
    seen[0] = True
    for i in order:
        for ref in decoded[i][2]:
            if ref >= 0:
                assert ref < n and not seen[ref], "%s: node %d is referenced twice or out of range" % (what, ref)
                seen[ref] = True
                order.append(int(ref))
    assert seen.all(), "%s: %d nodes are unreachable" % (what, int((~seen).sum()))
    slots = np.zeros(len(tl_inst), dtype=np.int32)
    lo_u = np.full((n, 3), np.inf, dtype=np.float32)         # exact union of the instance boxes below a node
    hi_u = np.full((n, 3), -np.inf, dtype=np.float32)
    stack = np.zeros(n, dtype=np.int64)
    for i in reversed(order):
        lo, hi, child = decoded[i]
        k, deepest = 0, 0
        for c in range(len(child)):
            ref = int(child[c])
            if ref >= 0:
                clo, chi = lo_u[ref], hi_u[ref]
                deepest = max(deepest, int(stack[ref]))
            else:
                v = (~ref) & 0xFFFFFFFF
                first, cnt = v >> 3, v & 7
                if cnt == 0:
                    continue
                assert cnt <= LEAF_MAX, "%s: a leaf of %d instances" % (what, cnt)
                assert first + cnt <= len(tl_inst)
                slots[first:first + cnt] += 1
                b = boxes[tl_inst[first:first + cnt]]
                clo, chi = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
            k += 1
            assert (lo[c] <= clo).all() and (chi <= hi[c]).all(), "%s: node %d child %d: decoded box %s %s does not hold %s %s" % (what, i, c, lo[c], hi[c], clo, chi)
            lo_u[i] = np.minimum(lo_u[i], clo); hi_u[i] = np.maximum(hi_u[i], chi)
        assert k >= 1
        stack[i] = (k - 1) + deepest                          # k - 1 siblings wait while the deepest child is walked
    assert (slots == 1).all(), "%s: %d leaf positions are not referenced exactly once" % (what, int((slots != 1).sum()))
    assert stack[0] <= info.max_stack, "%s: a depth-first walk needs %d entries, %d reported" % (what, stack[0], info.max_stack)
    assert info.max_stack + LEAF_MAX + info.blas_stack + 1 <= abi.TL_STACK_CAP
    assert sc.bvh_stats().max_stack == info.max_stack + LEAF_MAX + info.blas_stack + 1
    return int(stack[0])


@pytest.mark.parametrize("topology", ["lbvh", "ploc16"])
@pytest.mark.parametrize("n,identical", [(2, False), (3, False), (5, False), (4096, False), (100000, False), (5000, True)])
def test_device_built_tree_is_a_valid_conservative_tree_within_the_stack_budget(rt, monkeypatch, topology, n, identical):
    monkeypatch.setenv("SR_FAST_BUILD", topology)
    xf = affine_transforms(n, 100 + n, translation=300.0 if n > 5000 else 1.0e4, identical=identical)
    sc = small_mesh_scene(rt, xf, "device")
    info = assert_path(sc, "device")
    assert info.n_boxes == n and info.n_instances == n
    depth = check_structure(rt, sc, "%s, %d instances%s" % (topology, n, " (identical)" if identical else ""))
    print("%s n=%d%s: %d nodes, stack %d (reported %d), records %.3f ms, tree %.3f ms" % (topology, n, " identical" if identical else "", info.n_nodes, depth,
                                                                                          info.max_stack, info.records_ms, info.tree_ms))


def test_a_tree_outside_the_stack_budget_is_left_to_the_host(rt, monkeypatch):
    """63 tiny instances at (2^-j, 0, 0), (0, 2^-j, 0), (0, 0, 2^-j), j = 1..21: every split of the Morton order peels one
    instance off, so the radix tree is a chain some 60 levels deep, more than the 47-entry walk has room for. The device
    build refuses it and the host's depth-limited builder takes over; PLOC clusters the three arms bottom-up and may fit.
    Whichever path built the tree, it is a valid one inside the budget."""
    xf = np.zeros((63, 12), dtype=np.float32)
    xf[:, 0] = xf[:, 5] = xf[:, 10] = 1.0e-9
    for j in range(21):
        for a in range(3):
            xf[3 * j + a, 3 + 4 * a] = 2.0 ** -(j + 1)
    for topology in ("lbvh", "ploc16"):
        monkeypatch.setenv("SR_FAST_BUILD", topology)
        sc = small_mesh_scene(rt, xf, "device")
        info = sc.top_level_info()
        print("%s, 63 instances in geometric progression: on_device %d reason %d, top level %d + leaf %d + mesh tree %d + 1" %
              (topology, info.on_device, info.reason, info.max_stack, LEAF_MAX, info.blas_stack))
        assert info.max_stack + LEAF_MAX + info.blas_stack + 1 <= abi.TL_STACK_CAP and sc.bvh_stats().max_stack <= abi.TL_STACK_CAP
        if topology == "lbvh":
            assert_path(sc, "device", abi.TL_HOST_STACK_BUDGET)
        else:
            assert info.on_device == 1 or info.reason == abi.TL_HOST_STACK_BUDGET
        check_structure(rt, sc, topology + ", geometric progression")
        sc.close()


# ---- 3. queries ------------------------------------------------------------------------------------------------------
def test_device_built_top_level_trace_equals_brute_force(rt, oracle):
    """The bar of test_two_level_trace_equals_brute_force on the device-built structure."""
    for desc in (scenes.instanced_field(80), scenes.cornell_glass_mirror()):
        osc = oracle.OracleScene().load(desc)
        osc.set_brute_force(True)
        gsc = rt.Scene(0, instancing="two_level").set_top_level_build("device").load(desc)
        gsc.set_instances(desc.instances)
        assert gsc.two_level() and gsc.bvh_stats().n_triangles == desc.n_triangles()
        assert_path(gsc, "device")
        box = ((-14, -1, -14), (14, 9, 14))
        short = random_rays(6000, 4, box=box)
        short["tmax"] = np.random.default_rng(5).random(6000).astype(np.float32) * 2 + 0.01
        far = random_rays(4000, 9, box=((-900, 300, -900), (900, 700, 900)))
        far["dir"] = ((np.array([0.0, 1.0, 0.0], np.float32) - far["origin"]) / np.float32(600.0) + far["dir"] * np.float32(0.01)).astype(np.float32)
        far["tmax"] = 1.0e4
        axis = random_rays(3000, 11, box=box)
        axis["dir"][:1000] = (1, 0, 0); axis["dir"][1000:2000] = (0, -1, 0); axis["dir"][2000:] = (0, 0, 1)
        rays = np.concatenate([random_rays(20000, 3, box=box), camera_rays(oracle, desc, 96, 64), short, far, axis])
        rd = rt.rays_to_device(rays)
        hits_t = gsc.trace_closest(rd, len(rays))
        hits = rt.hits_from_device(hits_t)
        occ = gsc.trace_any(rd, len(rays)).cpu().numpy().view(np.uint32)
        want = osc.trace_closest(rays)
        assert (want["t"] >= 0).mean() > 0.03
        assert_bits_equal(want, hits, "closest hits (device-built top level, %s)" % desc.name)
        assert np.array_equal(osc.trace_any(rays), occ)
        pay = gsc.shade_closest_hit(hits_t, len(hits)).cpu().numpy().view(np.uint32).reshape(-1).view(abi.RAY_PAYLOAD)
        assert_bits_equal(osc.shade_closest_hit(want), pay, "payloads (device-built top level)")


# ---- 4. frames -------------------------------------------------------------------------------------------------------
class FramePair:
    """An oracle scene and a two-level device scene fed the same lists, rendered frame by frame with frames_equal_oracle's checks."""

    def __init__(self, rt, oracle, desc, W, H, blue_noise, mode):
        self.rt, self.oracle, self.desc, self.W, self.H = rt, oracle, desc, W, H
        self.osc = oracle.OracleScene().load(desc)
        self.gsc = rt.Scene(0, instancing="two_level").set_top_level_build(mode).load(desc)
        assert self.gsc.two_level()
        self.of, self.gf = oracle.HostFrame(W, H, blue_noise), rt.DeviceFrame(W, H, blue_noise)
        self.cfg = abi.SrTraceConfig.reference()
        self.prev, self.f = None, 0

    def set_instances(self, inst):
        self.osc.set_instances(inst); self.gsc.set_instances(inst)
        assert self.gsc.two_level()

    def frame(self, what):
        d, f, cfg = self.desc, self.f, self.cfg
        om = self.oracle.camera_matrices(d.camera_pos, d.camera_target, d.fov_y, self.W, self.H, self.prev)
        gm = self.rt.camera_matrices(d.camera_pos, d.camera_target, d.fov_y, self.W, self.H, self.prev)
        self.prev = list(om.view_proj)
        self.osc.reset_counters(); self.gsc.reset_counters()
        self.osc.trace_ris(self.of, om, f, cfg); self.gsc.trace_ris(self.gf, gm, f, cfg)
        self.osc.trace_final(self.of, om, f, cfg); self.gsc.trace_final(self.gf, gm, f, cfg)
        h, of, cur = self.gf.host(), self.of, f & 1
        for name, a, b in (("depth", of.depth, h["depth"]), ("normal", of.normal, h["normal"]), ("diffuse", of.diffuse, h["diffuse"]),
                           ("motion", of.motion, h["motion"]), ("reservoirs", of.reservoirs[cur], h["reservoirs"][cur]),
                           ("reservoirs_gi", of.reservoirs_gi[cur], h["reservoirs_gi"][cur]), ("raw_color", of.raw_color, h["raw_color"])):
            assert_bits_equal(a, b, "%s f%d (%s)" % (name, f, what))
        oc, gc = self.osc.counters(), self.gsc.counters()
        assert (oc.closest_queries, oc.any_queries) == (ref_closest(gc), ref_any(gc))
        self.f += 1


def moved(base, f):
    out = []
    for key, xs in base:
        m = []
        for j, x in enumerate(xs):
            y = np.array(x, dtype=np.float32).copy()
            if len(xs) > 4:                                   # the blobs drift and bob; ground and lamps stay
                y[3] += np.float32(0.11 * f * ((j % 3) - 1)); y[7] += np.float32(0.05 * f * (j % 2)); y[11] -= np.float32(0.07 * f)
            m.append(y)
        out.append((key, m))
    return out


def test_frames_of_moving_and_changing_instance_lists_equal_the_oracle(rt, oracle, blue_noise, monkeypatch):
    desc = scenes.instanced_field(60, nonuniform=True)
    base = desc.instances
    monkeypatch.setenv("SR_TL_BUILD", "device")
    _, gsc, _, _ = frames_equal_oracle(rt, oracle, desc, 224, 128, 4, blue_noise, instances_of_frame=lambda f: moved(base, f))
    monkeypatch.delenv("SR_TL_BUILD")
    assert gsc.as_state()[1] == abi.OP_FAST_BUILD
    assert_path(gsc, "device")
    # the instance count changes: added, removed, one mesh down to zero instances and back
    p = FramePair(rt, oracle, desc, 160, 96, blue_noise, "device")
    p.frame("first build")
    assert_path(p.gsc, "device", abi.TL_HOST_NOT_TWO_LEVEL)
    k0, xs0 = base[0]
    extra = [scenes.rotate_y(0.3 * j, -6.0 + 1.5 * j, 1.0 + 0.2 * j, 4.0 - j, 0.5) for j in range(9)]
    lists = [("moved", moved(base, 1)),
             ("9 added", [(k0, list(xs0) + extra)] + moved(base, 2)[1:]),
             ("half removed", [(k, list(xs)[:max(1, len(xs) // 2)] if len(xs) > 4 else xs) for k, xs in moved(base, 3)]),
             ("first mesh without instances", moved(base, 4)[1:]),
             ("first mesh back", moved(base, 5))]
    for what, inst in lists:
        p.set_instances(inst)
        assert p.gsc.as_state()[1] == abi.OP_FAST_BUILD
        info = assert_path(p.gsc, "device")
        assert info.n_instances == sum(len(xs) for _, xs in inst)
        p.frame(what)
    # 16 quiet frames: the settle rebuild is the host's quality build
    ops = []
    for _ in range(16):
        p.gsc.end_frame()
        ops.append(p.gsc.as_state()[1])
    assert ops[-1] == abi.OP_SLOW_BUILD and abi.OP_SLOW_BUILD not in ops[:-1], ops
    assert_path(p.gsc, "device", abi.TL_HOST_QUALITY_BUILD)
    p.frame("settled")


# ---- 5. fallbacks ----------------------------------------------------------------------------------------------------
def test_lists_the_device_path_cannot_take_are_built_on_the_host(rt, oracle, blue_noise):
    desc = scenes.instanced_field(40, nonuniform=True)
    base = desc.instances
    p = FramePair(rt, oracle, desc, 96, 64, blue_noise, "device")
    p.frame("first build")
    k0, xs0 = base[0]
    zero_scale = np.array([1, 0, 0, 0.2, 0, 0, 0, 1.0, 0, 0, 1, 0.1], dtype=np.float32)     # y scale 0: cannot be inverted
    step = [0]

    def ordinary(what):
        step[0] += 1
        p.set_instances(moved(base, step[0]))
        assert p.gsc.as_state()[1] == abi.OP_FAST_BUILD
        assert_path(p.gsc, "device")
        p.frame("ordinary list after " + what)
    ordinary("the first build")
    for what, inst, reason in (("a zero-scale instance", [(k0, list(xs0) + [zero_scale])] + base[1:], abi.TL_HOST_BAKED_INSTANCE),
                               ("an empty list", [], abi.TL_HOST_TOO_FEW),
                               ("a one-instance list", [(k0, [xs0[0]])], abi.TL_HOST_TOO_FEW)):
        p.set_instances(inst)
        info = assert_path(p.gsc, "device", reason)
        assert info.n_instances == sum(len(xs) for _, xs in inst)
        p.frame(what)
        ordinary(what)
    # one-level form and back: the first list in the two-level form again is a build from nothing
    p.gsc.set_instancing("flat")
    p.osc.set_instances(moved(base, 7)); p.gsc.set_instances(moved(base, 7))
    assert not p.gsc.two_level() and p.gsc.top_level_info().reason == abi.TL_HOST_NOT_TWO_LEVEL
    p.frame("one-level form")
    p.gsc.set_instancing("two_level")
    p.set_instances(moved(base, 8))
    assert_path(p.gsc, "device", abi.TL_HOST_NOT_TWO_LEVEL)
    p.frame("the switch back to the two-level form")
    ordinary("the switch")
    # mode HOST never leaves the host
    p.gsc.set_top_level_build("host")
    p.set_instances(moved(base, 9))
    assert_path(p.gsc, "host")
    p.frame("mode host")


# ---- 6. scale --------------------------------------------------------------------------------------------------------
def test_ten_thousand_instances_build_on_the_device_without_allocating(rt, blue_noise):
    import torch
    rng = np.random.default_rng(3)
    v, idx = scenes.uv_sphere(1.0, 72, 71)                          # 10 080 triangles
    n = 10000
    xs = np.array([scenes.rotate_y(rng.uniform(0, 2 * np.pi), rng.uniform(-60, 60), rng.uniform(0.3, 6.0), rng.uniform(-60, 60), rng.uniform(0.2, 0.5)) for _ in range(n)],
                  dtype=np.float32).reshape(n, 12)
    xs2 = xs.copy()
    xs2[::2, 7] += np.float32(0.5)
    gv, gi = scenes.quad((-80, 0, -80), (-80, 0, 80), (80, 0, 80), (80, 0, -80), (0, 1, 0))
    lv, li = scenes.quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1), (0, -1, 0))
    rest = [(2, [scenes.translate(0, 0, 0)]), (3, [scenes.translate(20.0 * np.cos(k), 25.0, 20.0 * np.sin(k), 6.0) for k in range(6)])]
    W, H = 640, 360
    images, scs = {}, {}
    for mode in ("host", "device"):
        sc = rt.Scene(0).set_top_level_build(mode)                  # auto instancing: picks the two-level form by itself
        sc.add_mesh(1, v, idx, abi.material(base_color=(0.6, 0.5, 0.4, 1.0), roughness=0.6))
        sc.add_mesh(2, gv, gi, abi.material(base_color=(0.7, 0.7, 0.7, 1.0), roughness=0.8))
        sc.add_mesh(3, lv, li, abi.material(base_color=(1, 1, 1, 1), emissive_factor=(1, 1, 1), emissive_strength=30.0))
        sc.set_instances([(1, xs)] + rest)
        assert sc.two_level() and sc.bvh_stats().n_triangles > 100_000_000
        sc.set_instances([(1, xs2)] + rest)
        info = assert_path(sc, mode)
        assert info.n_boxes == n + 7
        print("10 000 x 10 080, mode %s: set_instances %.2f ms (records %.2f, tree %.2f), %d top-level nodes" % (mode, info.build_ms, info.records_ms, info.tree_ms, info.n_nodes))
        fr = rt.DeviceFrame(W, H, blue_noise)
        prev = None
        for f in range(2):
            m = rt.camera_matrices((0.0, 30.0, 95.0), (0.0, 2.0, 0.0), 45.0, W, H, prev)
            prev = list(m.view_proj)
            sc.trace_ris(fr, m, f); sc.trace_final(fr, m, f)
        images[mode] = fr.host()
        scs[mode] = sc
    for name in ("raw_color", "depth", "normal", "diffuse", "motion"):
        assert_bits_equal(images["host"][name], images["device"][name], "%s, host-built vs device-built top level" % name)
    assert (images["device"]["depth"] < 0x7c00).mean() > 0.5
    scs["host"].close()
    sc = scs["device"]
    free = []
    for k in range(50):
        sc.set_instances([(1, xs if k & 1 else xs2)] + rest)
        assert_path(sc, "device")
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    assert abs(free[-1] - free[1]) < (1 << 20) and max(free[1:]) - min(free[1:]) < (1 << 20), free
    # auto mode: the path follows the threshold top_level_info reports
    sc.set_top_level_build("auto")
    t = sc.top_level_info().auto_threshold
    assert 16 <= t <= n
    for count, want in ((t // 2, 0), (t - 8, 0), (t - 7, 1), (min(2 * t, n), 1)):   # + 7 boxes of the ground and the lamps
        sc.set_instances([(1, xs[:count])] + rest)
        info = sc.top_level_info()
        assert info.n_boxes == count + 7 and info.on_device == want and info.reason == (abi.TL_ON_DEVICE if want else abi.TL_HOST_BELOW_THRESHOLD), (count, t, info.on_device, info.reason)


def test_hundred_thousand_instances_build_faster_on_the_device_than_on_the_host(rt):
    """HOST mode is the code the top level was always built by, so this compares the device build against it in one process:
    the library's own build time and the wall clock around set_instances, median of 5 changed lists each after a warm-up list."""
    xf = [affine_transforms(100000, 7 + k, translation=400.0) for k in range(2)]
    ms = {}
    for mode in ("host", "device"):
        sc = small_mesh_scene(rt, xf[0], mode)
        build, wall = [], []
        for k in range(6):
            t0 = time.perf_counter()
            sc.set_instances([(1, xf[(k + 1) & 1])])
            wall.append((time.perf_counter() - t0) * 1e3)
            build.append(assert_path(sc, mode).build_ms)
        ms[mode] = (float(np.median(build[1:])), float(np.median(wall[1:])))
        info = sc.top_level_info()
        print("100 000 instances, mode %s: build %.2f ms (last: records %.2f, tree %.2f), set_instances call %.2f ms with the Python marshalling (medians of 5)"
              % (mode, ms[mode][0], info.records_ms, info.tree_ms, ms[mode][1]))
        sc.close()
    assert ms["device"][0] < ms["host"][0], ms
    assert ms["device"][1] < ms["host"][1], ms


# ---- 7. renderer -----------------------------------------------------------------------------------------------------
def test_renderer_with_moving_instances_equals_host_mode_byte_for_byte(rt, hip, monkeypatch):
    desc = scenes.instanced_field(60, nonuniform=True)
    base = desc.instances
    W, H, frames = 160, 96, 8
    camera = (desc.camera_pos, desc.camera_target, desc.fov_y)
    monkeypatch.setenv("SR_INSTANCING", "two_level")
    got = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("SR_TL_BUILD", mode)
        r = rt.Renderer((W, H))
        load(r, desc)
        per_frame = []
        for f in range(frames):
            r.wait_frame(r.render(camera, moved(base, f)))
            per_frame.append(grab(rt, hip, r))
            if f > 0:
                assert_path(r.replica_scene(0), mode)
        r.close()
        # the same frames without waiting in between: two frames in flight
        r = rt.Renderer((W, H))
        load(r, desc)
        for f in range(frames):
            last = r.render(camera, moved(base, f))
        r.wait_frame(last)
        in_flight = grab(rt, hip, r)
        assert_path(r.replica_scene(0), mode)
        r.close()
        got[mode] = (per_frame, in_flight)
    for f in range(frames):
        assert_equal(got["host"][0][f][0], got["device"][0][f][0], "frame %d output" % f)
        assert_equal(got["host"][0][f][1], got["device"][0][f][1], "frame %d raw_color" % f)
    for mode in ("host", "device"):
        assert_equal(got["host"][0][-1][0], got[mode][1][0], "last output, two frames in flight, mode " + mode)
        assert_equal(got["host"][0][-1][1], got[mode][1][1], "last raw_color, two frames in flight, mode " + mode)
    assert len(np.unique(got["device"][0][-1][0])) > 200
