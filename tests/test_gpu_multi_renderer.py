"""One frame across several device slots from one Renderer (sr_renderer_create_multi): every comparison is bit for bit, on the
RGBA8 output and on the fp32 radiance, against a single-device Renderer fed the same calls. Rehearsal mode (every slot on
device 0) runs the whole multi-device frame — strips, history exchange, gather, post chain on slot 0 — on one GPU; real
devices are exercised when the box has them."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

from sunray_amd import scenes

pytestmark = pytest.mark.gpu

REF_ASSET_DIR = os.path.join(os.path.dirname(__file__), "golden", "ref_assets")


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


def grab(rt, hip, r):
    """(output RGBA8 as uint32, raw_color fp32 bits as uint32) of the last submitted frame, after waiting for it."""
    from sunray_amd._lib import lib
    outp, rawp = C.c_void_p(), C.c_void_p()
    assert lib().sr_renderer_get(r._h, None, C.byref(outp), C.byref(rawp), None) == 0
    W, H = r.size
    out = np.zeros(W * H, dtype=np.uint32)
    raw = np.zeros(W * H * 4, dtype=np.uint32)
    assert hip.hipSetDevice(C.c_int(r.devices[0])) == 0
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), outp, C.c_size_t(out.nbytes), C.c_int(2)) == 0
    assert hip.hipMemcpy(raw.ctypes.data_as(C.c_void_p), rawp, C.c_size_t(raw.nbytes), C.c_int(2)) == 0
    return out, raw


def assert_equal(a, b, what):
    nd = int((a != b).sum())
    assert nd == 0, "%s: %d of %d words differ" % (what, nd, a.size)


def load(r, desc):
    for m in desc.meshes:
        r.load_mesh(m.key, m.vertices, m.indices, m.material)


def moving_camera(desc, f):
    """Slides sideways a third of a unit per frame (~7 pixels at 120 wide), position and target alike."""
    dx = -0.6 + 0.3 * f
    return ((desc.camera_pos[0] + dx, desc.camera_pos[1], desc.camera_pos[2]),
            (desc.camera_target[0] + dx, desc.camera_target[1], desc.camera_target[2]), desc.fov_y)


def static_camera(desc, f):
    return (desc.camera_pos, desc.camera_target, desc.fov_y)


def frames_of(rt, hip, r, desc, n, camera=static_camera, instances=None):
    got = []
    for f in range(n):
        r.wait_frame(r.render(camera(desc, f), instances(f) if instances else desc.instances))
        got.append(grab(rt, hip, r))
    return got


def counter_sum(r, n_slots):
    tot = np.zeros(4, dtype=np.uint64)
    for i in range(n_slots):
        c = r.replica_scene(i).counters()
        tot += np.array([c.closest_queries, c.any_queries, c.reused_primary_hits, c.reused_visibility_queries], dtype=np.uint64)
    return tot


def compare_runs(rt, hip, devices, W, H, frames, axis="cols", bounds=None, motion_halo=None, camera=static_camera, desc=None):
    desc = desc or scenes.cornell_box()
    single = rt.Renderer((W, H))
    load(single, desc)
    want = frames_of(rt, hip, single, desc, frames, camera)
    want_rays = counter_sum(single, 1)
    single.close()
    multi = rt.Renderer((W, H), devices=devices, axis=axis, bounds=bounds, motion_halo=motion_halo)
    load(multi, desc)
    got = frames_of(rt, hip, multi, desc, frames, camera)
    rays = counter_sum(multi, len(devices))
    overflow = multi.history_overflow()
    multi.close()
    return want, got, want_rays, rays, overflow


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_rehearsal_static_camera_equals_single_device(rt, hip, devices):
    want, got, want_rays, rays, overflow = compare_runs(rt, hip, devices, 96, 80, 6)
    for f in range(6):
        assert_equal(want[f][0], got[f][0], "frame %d output, %d slots" % (f, len(devices)))
        assert_equal(want[f][1], got[f][1], "frame %d raw_color, %d slots" % (f, len(devices)))
    assert overflow == 0
    assert (rays == want_rays).all(), (rays, want_rays)      # halo pixels are traced but not counted


@pytest.mark.parametrize("axis,W,H,bounds", [("rows", 40, 72, [0, 50, 50, 72]), ("cols", 72, 40, [0, 5, 5, 72]),
                                             ("cols", 72, 40, [0, 20, 20, 45, 72])])
def test_uneven_bounds_with_narrow_and_empty_strips(rt, hip, axis, W, H, bounds):
    devices = [0] * (len(bounds) - 1)
    want, got, want_rays, rays, overflow = compare_runs(rt, hip, devices, W, H, 4, axis=axis, bounds=bounds)
    for f in range(4):
        assert_equal(want[f][0], got[f][0], "frame %d output" % f)
        assert_equal(want[f][1], got[f][1], "frame %d raw_color" % f)
    assert overflow == 0 and (rays == want_rays).all()


def test_moving_camera_needs_and_gets_history_exchange(rt, hip):
    want, got, _, _, overflow = compare_runs(rt, hip, [0, 0, 0], 120, 48, 5, motion_halo=16, camera=moving_camera)
    for f in range(5):
        assert_equal(want[f][0], got[f][0], "frame %d output (history exchanged)" % f)
        assert_equal(want[f][1], got[f][1], "frame %d raw_color (history exchanged)" % f)
    assert overflow == 0
    _, stale, _, _, overflow0 = compare_runs(rt, hip, [0, 0, 0], 120, 48, 5, motion_halo=0, camera=moving_camera)
    assert overflow0 > 0                                     # the check sees reads outside strip + spatial halo ...
    assert any((want[f][1] != stale[f][1]).any() for f in range(5))   # ... and they do change the frame


def test_two_frames_in_flight_equal_wait_every_frame(rt, hip):
    desc = scenes.cornell_box()
    W, H, frames = 120, 48, 6
    seq = rt.Renderer((W, H), devices=[0, 0, 0], motion_halo=16)
    load(seq, desc)
    want = frames_of(rt, hip, seq, desc, frames, moving_camera)[-1]
    seq.close()
    r = rt.Renderer((W, H), devices=[0, 0, 0], motion_halo=16)
    load(r, desc)
    prev = None
    for f in range(frames):
        fr = r.render(moving_camera(desc, f), desc.instances)     # frame f+1 is submitted before frame f is waited for
        if prev is not None:
            r.wait_frame(prev)
        prev = fr
    r.wait_frame(prev)
    got = grab(rt, hip, r)
    assert r.history_overflow() == 0
    r.close()
    assert_equal(want[0], got[0], "output, two frames in flight")
    assert_equal(want[1], got[1], "raw_color, two frames in flight")


def test_state_rules_of_bounds_and_halo(rt):
    from sunray_amd._lib import SunrayError
    desc = scenes.cornell_box()
    r = rt.Renderer((64, 48), devices=[0, 0])
    with pytest.raises(SunrayError) as e:
        r.set_strip_bounds([0, 40, 30])                       # not increasing
    assert e.value.code == -1
    with pytest.raises(SunrayError):
        r.set_strip_bounds([0, 10, 60])                       # does not end at the width
    r.set_strip_bounds([0, 10, 64])
    load(r, desc)
    r.wait_frame(r.render(static_camera(desc, 0), desc.instances))
    with pytest.raises(SunrayError) as e:
        r.set_strip_bounds([0, 32, 64])
    assert e.value.code == -4
    with pytest.raises(SunrayError) as e:
        r.set_motion_halo(8)
    assert e.value.code == -4
    with pytest.raises(SunrayError):
        r.replica_scene(2)
    r.resize((80, 48))                                        # a new extent: a new (equal) cut may be set again
    r.set_strip_bounds([0, 70, 80])
    r.close()
    r = rt.Renderer((64, 48))                                 # one slot: the same rules, one strip, nothing to overflow
    r.set_strip_bounds([0, 64])
    r.set_motion_halo(8)
    assert r.history_overflow() == 0
    r.replica_scene(0)
    with pytest.raises(SunrayError):
        r.replica_scene(1)
    load(r, desc)
    r.wait_frame(r.render(static_camera(desc, 0), desc.instances))
    with pytest.raises(SunrayError) as e:
        r.set_strip_bounds([0, 64])
    assert e.value.code == -4
    with pytest.raises(SunrayError) as e:
        r.set_motion_halo(8)
    assert e.value.code == -4
    r.close()


def test_scene_changes_resize_and_gltf(rt, hip):
    desc = scenes.cornell_box()
    moved = [(k, [np.asarray(t, dtype=np.float32).reshape(3, 4) + np.float32(0.05) * np.eye(3, 4, 3, dtype=np.float32) for t in ts])
             for k, ts in desc.instances]
    room_cam = ((13.0, 30.0, 25.0), (0.0, 13.0, 0.0), 45.0)
    noise = rt.decode_image_rgba8(open(os.path.join(REF_ASSET_DIR, "noise.png"), "rb").read())

    def run(r):
        out = []
        r.set_blue_noise(noise)
        load(r, desc)
        cam = static_camera(desc, 0)
        for inst in [desc.instances, desc.instances, moved, moved]:     # moved instances mid-sequence
            r.wait_frame(r.render(cam, inst))
            out.append(grab(rt, hip, r))
        for m in desc.meshes:                                  # the room's keys start at (group 0, index 0) as the box's do
            r.unload_mesh(m.key)
        group, inst = r.load_gltf(os.path.join(REF_ASSET_DIR, "Room.glb"))
        # a new extent restarts the history, so the camera cut to the room reads none (a cut without one is a jump far beyond
        # any motion_halo: the history-reach check reports it)
        r.resize((160, 120))
        for _ in range(3):
            r.wait_frame(r.render(room_cam, inst))
            out.append(grab(rt, hip, r))
        r.unload_scene(group)
        load(r, desc)
        r.resize((96, 80))
        for inst in [moved, desc.instances]:
            r.wait_frame(r.render(cam, inst))
            out.append(grab(rt, hip, r))
        return out

    single = rt.Renderer((96, 80))
    want = run(single)
    single.close()
    multi = rt.Renderer((96, 80), devices=[0, 0, 0])
    got = run(multi)
    overflow = multi.history_overflow()
    multi.close()
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert_equal(a[0], b[0], "step %d output" % i)
        assert_equal(a[1], b[1], "step %d raw_color" % i)
    assert overflow == 0


def test_bench_scene_1080p_four_rehearsal_slots(rt, hip):
    desc = scenes.heightfield(708)
    crcs = []
    for devices in (None, [0, 0, 0, 0]):
        r = rt.Renderer((1920, 1080)) if devices is None else rt.Renderer((1920, 1080), devices=devices)
        load(r, desc)
        got = frames_of(rt, hip, r, desc, 3)
        crcs.append(["%08x" % (zlib.crc32(g[1].tobytes()) & 0xFFFFFFFF) for g in got])
        if devices:
            assert r.history_overflow() == 0
        r.close()
    assert crcs[0] == crcs[1], crcs


@pytest.mark.parametrize("n", [2, 4])
def test_real_devices_equal_single_device(rt, hip, n):
    import torch
    if torch.cuda.device_count() < n:
        pytest.skip("needs %d visible GPUs (%d here)" % (n, torch.cuda.device_count()))
    want, got, want_rays, rays, overflow = compare_runs(rt, hip, list(range(n)), 96, 80, 6)
    for f in range(6):
        assert_equal(want[f][0], got[f][0], "frame %d output, devices 0..%d" % (f, n - 1))
        assert_equal(want[f][1], got[f][1], "frame %d raw_color, devices 0..%d" % (f, n - 1))
    assert overflow == 0 and (rays == want_rays).all()


# ---- history_overflow() == 0 means the frames are equal: a sweep over slide and motion_halo ---------------------------------------
def slide_camera(desc, cols, step):
    """Slides `step` world units per frame along the axis (sideways for column strips, vertically for row strips)."""
    def camera(_, f):
        d = step * (f - 2)
        off = (d, 0.0, 0.0) if cols else (0.0, d, 0.0)
        return (tuple(p + o for p, o in zip(desc.camera_pos, off)), tuple(t + o for t, o in zip(desc.camera_target, off)), desc.fov_y)
    return camera


def largest_axis_motion(rt, desc, W, H, camera, frames, cols, blue_noise):
    """Largest stored motion along the axis, in pixels, over the motion planes of frames 1 .. frames - 1 of this camera path."""
    import strip_reference as ref
    sc = rt.Scene(0).load(desc)
    gf = rt.DeviceFrame(W, H, blue_noise)
    prev, largest = None, 0.0
    for f in range(frames):
        pos, tgt, fov = camera(desc, f)
        m = rt.camera_matrices(pos, tgt, fov, W, H, prev)
        prev = list(m.view_proj)
        sc.trace_ris(gf, m, f)
        if f > 0:
            words = gf.motion.cpu().numpy().view(np.uint32)
            kind, _, _ = ref.reach_f32(words, np.zeros(words.shape), W if cols else H, cols)
            mv = ref.half_bits_to_f32(words & 0xFFFF if cols else words >> 16)[kind == ref.IN_RANGE]
            largest = max(largest, float(np.abs(mv).max()) * (W if cols else H))
    sc.close()
    return largest


@pytest.mark.parametrize("axis,W,H", [("cols", 120, 48), ("rows", 48, 120)])
def test_zero_history_overflow_means_equal_frames(rt, hip, blue_noise, axis, W, H):
    desc = scenes.cornell_box()
    cols, frames = axis == "cols", 5
    probe = 0.1
    per_unit = largest_axis_motion(rt, desc, W, H, slide_camera(desc, cols, probe), frames, cols, blue_noise) / probe
    seen = []                                                # (slide, halo, overflow, differs)
    for target in (2.0, 7.0, 13.0):
        step = target / per_unit
        step *= target / largest_axis_motion(rt, desc, W, H, slide_camera(desc, cols, step), frames, cols, blue_noise)
        camera = slide_camera(desc, cols, step)
        print("%s %dx%d: slide %.4f units per frame, largest stored motion along the axis %.2f px (aimed at %g)" % (
            axis, W, H, step, largest_axis_motion(rt, desc, W, H, camera, frames, cols, blue_noise), target))
        single = rt.Renderer((W, H))
        load(single, desc)
        want = frames_of(rt, hip, single, desc, frames, camera)
        single.close()
        for halo in (0, 4, 8, 16):
            multi = rt.Renderer((W, H), devices=[0, 0, 0], axis=axis, motion_halo=halo)
            load(multi, desc)
            got = frames_of(rt, hip, multi, desc, frames, camera)
            overflow = multi.history_overflow()
            multi.close()
            differs = any((want[f][0] != got[f][0]).any() or (want[f][1] != got[f][1]).any() for f in range(frames))
            print("  motion_halo %2d: overflow %d, frames %s" % (halo, overflow, "differ" if differs else "equal"))
            if overflow == 0:
                for f in range(frames):
                    assert_equal(want[f][0], got[f][0], "%s slide %g px halo %d: overflow 0, frame %d output" % (axis, target, halo, f))
                    assert_equal(want[f][1], got[f][1], "%s slide %g px halo %d: overflow 0, frame %d raw_color" % (axis, target, halo, f))
            seen.append((target, halo, overflow, differs))
    assert any(o == 0 for _, _, o, _ in seen), seen          # not vacuous: some halo suffices for some slide ...
    assert any(o > 0 for _, _, o, _ in seen), seen           # ... some does not ...
    assert any(o > 0 and d for _, _, o, d in seen), seen     # ... and there the frame really differs
