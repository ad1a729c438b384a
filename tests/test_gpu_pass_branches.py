"""ris_kernel and final_kernel on the branches no parity scene reaches (kernels.hip): the cases of tests/pass_branch_cases.py, each
shown by tests/test_pass_branches_host.py to drive the oracle down the outcomes it names — reprojection off every side of the screen,
the dummy light record, draws of exactly 1.0f, denormal denoiser albedos, a view along the normal, walks ended by every exit, and
reservoirs, depths and normals overwritten between the two passes (out-of-range light indices, infinite W, huge M, samples behind the
surface, within 0.002 of it or facing away, a light list that shrinks between the passes). On every frame the depth, normal, diffuse
and motion images, both reservoir buffers and raw_color must equal the oracle's bit for bit, after the RIS pass and after the final
pass, and the ray counters must account for every query the oracle issues — with one-level and with two-level instancing (different
kernel template variants) and once without the primary-hit hand-off."""
import os
import sys

import numpy as np
import pytest

from sunray_amd import abi

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pass_branch_cases as pbc  # noqa: E402
from test_gpu_parity import assert_bits_equal, ref_any, ref_closest  # noqa: E402

CASES = pbc.cases()
SETUPS = [("flat", None), ("two_level", None), ("flat", False)]            # (instancing, primary-hit hand-off: None = with)
RIS_OUTPUTS = ("depth", "normal", "diffuse", "motion", "reservoirs", "reservoirs_gi")


@pytest.fixture(scope="module")
def rt():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from sunray_amd import runtime
    return runtime


def device_buffers(h, f):
    cur = f & 1
    return {"depth": h["depth"], "normal": h["normal"], "diffuse": h["diffuse"], "motion": h["motion"],
            "reservoirs": h["reservoirs"][cur], "reservoirs_gi": h["reservoirs_gi"][cur], "raw_color": h["raw_color"]}


def upload(gf, bufs, f):
    """The buffers a patch may have written, back into the device frame."""
    import torch
    cur = f & 1
    gf.depth.copy_(torch.from_numpy(np.ascontiguousarray(bufs["depth"]).view(np.int16)))
    gf.normal.copy_(torch.from_numpy(np.ascontiguousarray(bufs["normal"]).view(np.int32)))
    gf.reservoirs[cur].copy_(torch.from_numpy(np.ascontiguousarray(bufs["reservoirs"]).view(np.int32).reshape(-1, 12)))
    gf.reservoirs_gi[cur].copy_(torch.from_numpy(np.ascontiguousarray(bufs["reservoirs_gi"]).view(np.int32).reshape(-1, 12)))
    torch.cuda.synchronize()


def render_and_compare(rt, oracle, case, blue_noise, instancing, primary, flags=0):
    """Renders the case's frames on the device as pass_branch_cases.oracle_frames does with the oracle and compares them stage by
    stage. Returns the device's ray counters per frame."""
    want = pbc.oracle_frames(oracle, case, blue_noise)
    desc, W, H = case.scene(), case.W, case.H
    gsc = rt.Scene(0, instancing=instancing).load(desc)
    assert gsc.two_level() == (instancing == "two_level")
    gf = rt.DeviceFrame(W, H, blue_noise, primary=primary)
    prev, counters = None, []
    for i, (fr, rec) in enumerate(zip(case.frames, want)):
        f = fr.frame_count
        cfg = abi.SrTraceConfig.from_buffer_copy(bytes(fr.cfg))
        cfg.flags |= flags
        what = "%s frame %d (%s%s)" % (case.name, i, instancing, "" if primary is None else ", no hand-off")
        if fr.relight is not None:
            gsc.set_instances(desc.instances)
        gm = rt.camera_matrices(fr.camera[0], fr.camera[1], desc.fov_y, W, H, prev)
        assert bytes(gm) == bytes(oracle.camera_matrices(fr.camera[0], fr.camera[1], desc.fov_y, W, H, prev))
        prev = list(gm.view_proj)
        gsc.reset_counters()
        if cfg.enable_restir:
            gsc.trace_ris(gf, gm, f, cfg)
            got = device_buffers(gf.host(), f)
            for name in RIS_OUTPUTS:
                assert_bits_equal(rec["after_ris"][name], got[name], "%s after the RIS pass, %s" % (name, what))
            if fr.patch is not None:
                fr.patch(got)                          # the same bytes as the host frame held: the same patch
                upload(gf, got, f)
        if fr.relight is not None:
            gsc.set_instances(fr.relight)
        gsc.trace_final(gf, gm, f, cfg)
        got = device_buffers(gf.host(), f)
        assert np.isfinite(got["raw_color"]).all(), what
        for name in pbc.BUFFERS:
            assert_bits_equal(rec["after_final"][name], got[name], "%s after the final pass, %s" % (name, what))
        c = gsc.counters()
        assert rec["counters"] == (ref_closest(c), ref_any(c)), what
        hand_off = cfg.enable_restir and cfg.virtual_bounces and gf.primary is not None
        assert c.reused_primary_hits == (W * H if hand_off else 0), what
        if flags & abi.TRACE_FLAG_TRACE_EVERY_QUERY:
            assert c.reused_visibility_queries == 0, what
        counters.append(c)
    gsc.close()
    return counters


@pytest.mark.parametrize("instancing,primary", SETUPS, ids=["flat", "two_level", "flat_no_hand_off"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_equals_oracle(rt, oracle, blue_noise, case, instancing, primary):
    render_and_compare(rt, oracle, case, blue_noise, instancing, primary)


@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith(("injected", "relit"))], ids=repr)
def test_injected_state_with_every_query_traced(rt, oracle, blue_noise, case):
    """The final pass answers the last GI visibility query without a traversal when the sample came from a neighbour
    (gi_sample_seen); SR_TRACE_FLAG_TRACE_EVERY_QUERY makes it traverse. On injected reservoirs too, both give the oracle's bits, and
    the queries traversed plus the queries answered from the neighbour's are the same number either way."""
    short = render_and_compare(rt, oracle, case, blue_noise, "flat", None)
    every = render_and_compare(rt, oracle, case, blue_noise, "flat", None, flags=abi.TRACE_FLAG_TRACE_EVERY_QUERY)
    for a, b in zip(short, every):
        assert b.reused_visibility_queries == 0
        assert a.any_queries + a.reused_visibility_queries == b.any_queries
    if case.name != "injected_close_up":       # there every segment is too short to trace, reused or not
        assert sum(a.reused_visibility_queries for a in short) > 0
