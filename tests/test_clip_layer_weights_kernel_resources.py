"""The compiler's report for the kernel of sunray_amd/csrc/clip_layer_weights.hip: exactly one kernel, no scratch, no spills, no
LDS (the four waves of a block are independent), and at most 128 VGPRs, 4 or more waves a SIMD. The first build reported 34 VGPRs,
65 SGPRs, 8 waves a SIMD; with layers of effective weight 0 skipped before they are sampled it reports 36 and 64
(clip_spline_weights_kernel, whose Hermite form it shares: 61 VGPRs, 8 waves): a lane holds one accumulator, and a layer's headers,
set, key search and effective weight are scalar. No GPU."""
from sunray_amd import build


def test_clip_layer_weights_kernel_has_no_scratch_no_spills_no_lds_and_stays_in_budget():
    res = build.kernel_resources("clip_layer_weights.hip")
    assert len(res) == 1 and "clip_layer_weights_kernel" in list(res)[0], sorted(res)
    r = list(res.values())[0]
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == 0, r
    assert r["vgprs"] <= 128 and r["occupancy"] >= 4, r
