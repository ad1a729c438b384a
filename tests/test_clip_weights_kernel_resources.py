"""The compiler's report for clip_weights_kernel (sunray_amd/csrc/clip_weights.hip): one kernel of that name, no scratch, no
spills, no LDS (the four waves of a block are independent), and a register figure within the budget read from the first build:
22 VGPRs and 30 SGPRs, 8 waves a SIMD. The row, the headers, the set and the key search live in scalar registers; a lane holds two
keys, the fraction, a weight and its place in the list. No GPU."""
from sunray_amd import build


def test_clip_weights_kernel_has_no_scratch_no_lds_and_stays_in_budget():
    res = build.kernel_resources("clip_weights.hip")
    mine = [r for name, r in res.items() if "clip_weights_kernel" in name]
    assert len(mine) == 1, sorted(res)
    r = mine[0]
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == 0, r
    assert r["vgprs"] <= 22 and r["sgprs"] <= 30 and r["occupancy"] >= 8, r
    # the neighbours' reports are still their own
    assert not any("clip_weights_kernel" in name for name in build.kernel_resources("clip_pose.hip"))
    assert not any("clip_weights_kernel" in name for name in build.kernel_resources("pose_batch.hip"))
