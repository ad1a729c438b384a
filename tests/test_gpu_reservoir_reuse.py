"""The reservoir weights of the two passes reuse the target-function value of the sample the reservoir holds instead of
evaluating eval_unshadowed_light again (kernels.hip: p_hat_held in ris_kernel, f_y_winner in final_kernel). Which value that is
depends on which sample every merge selected, so both passes run for four frames under a moving camera on the Cornell box with
the glass and the mirror sphere (emissive triangles, rough walls, two surfaces with roughness <= 0.2) and the DI reservoirs, the
GI reservoirs and raw_color must equal the oracle's bit for bit on every frame — once with the scene's light list and once with a
light list of a single triangle (every light index clamps to 0). The oracle's own reservoirs show that the frames reach the
cases that matter: pixels whose temporal merge took the history's sample, pixels where it kept the new one, and pixels that ran
RIS without any contributing candidate (w_sum == 0, no sample selected)."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import scenes

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import assert_bits_equal  # noqa: E402

W, H, FRAMES = 64, 48, 4
RIS_CANDIDATES = 16.0         # SrTraceConfig.reference(): M of a reservoir that ran RIS and merged nothing


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def scene(lights):
    desc = scenes.cornell_glass_mirror()
    if lights == "one_triangle":
        lamp = next(m for m in desc.meshes if float(m.material["emissive_factor"][3]) > 0)
        lamp.indices = lamp.indices[:3].copy()
    return desc


def camera(desc, f):
    p = desc.camera_pos
    return (p[0] + 0.05 * f, p[1] + 0.02 * f, p[2] - 0.03 * f), desc.camera_target, desc.fov_y


def key3(a):
    """One hashable per row of a [n, 3] float32 array (its bits)."""
    return [r.tobytes() for r in np.ascontiguousarray(a).view(np.uint32)]


@pytest.fixture(scope="module", params=["scene_lights", "one_triangle"])
def reference(request, oracle, blue_noise):
    """The oracle's four frames, computed once per light list: [(reservoirs, reservoirs_gi, raw_color)] and the description."""
    desc = scene(request.param)
    osc = oracle.OracleScene().load(desc)
    fr = oracle.HostFrame(W, H, blue_noise)
    frames, prev = [], None
    for f in range(FRAMES):
        m = oracle.camera_matrices(*camera(desc, f), W, H, prev)
        prev = list(m.view_proj)
        osc.trace_ris(fr, m, f); osc.trace_final(fr, m, f)
        frames.append((fr.reservoirs[f & 1].copy(), fr.reservoirs_gi[f & 1].copy(), fr.raw_color.copy()))
    osc.close()
    return desc, frames


def test_oracle_frames_reach_both_merge_outcomes_and_empty_reservoirs(reference):
    _, frames = reference
    taken = kept = empty = 0
    for f in range(1, FRAMES):
        cur, hist = frames[f][0], frames[f - 1][0]
        history_samples = set(k for k, w in zip(key3(hist["light_pos"]), hist["w_sum"]) if w > 0)
        merged = (cur["M"] > RIS_CANDIDATES) & (cur["w_sum"] > 0)                  # RIS ran and a history reservoir was merged in
        from_history = np.array([k in history_samples for k in key3(cur["light_pos"])])
        taken += int((merged & from_history).sum())
        kept += int((merged & ~from_history).sum())                               # a fresh candidate: a new random point of a light
    for f in range(FRAMES):
        cur = frames[f][0]
        empty += int(((cur["M"] >= RIS_CANDIDATES) & (cur["w_sum"] == 0)).sum())   # e.g. the ceiling: the lamp faces away from it
    print("temporal merge: history taken on %d pixels, new sample kept on %d; RIS without a contributing candidate on %d" % (taken, kept, empty))
    assert taken > 50 and kept > 50 and empty > 50


def test_passes_equal_oracle_under_a_moving_camera(rt, reference, blue_noise):
    desc, frames = reference
    gsc = rt.Scene(0).load(desc)
    fr = rt.DeviceFrame(W, H, blue_noise)
    prev = None
    for f in range(FRAMES):
        m = rt.camera_matrices(*camera(desc, f), W, H, prev)
        prev = list(m.view_proj)
        gsc.trace_ris(fr, m, f); gsc.trace_final(fr, m, f)
        h = fr.host()
        want_di, want_gi, want_color = frames[f]
        assert_bits_equal(want_di, h["reservoirs"][f & 1], "DI reservoirs f%d" % f)
        assert_bits_equal(want_gi, h["reservoirs_gi"][f & 1], "GI reservoirs f%d" % f)
        assert_bits_equal(want_color, h["raw_color"], "raw_color f%d" % f)
    gsc.close()
