"""The compiler's report for clip_spline_weights_kernel (sunray_amd/csrc/clip_spline_weights.hip): one kernel in that file, no
scratch, no spills, no LDS (the four waves of a block are independent), 8 waves a SIMD, and a register figure within the budget
read from the first build: 61 VGPRs and 46 SGPRs. The row, the headers, both sets, the key searches and the eight row pointers
live in scalar registers; a lane holds the Hermite basis of both sources in double, four keys, two weights and its place in the
list. The two LINEAR / STEP weights kernels keep their files to themselves. No GPU."""
from sunray_amd import build


def test_clip_spline_weights_kernel_has_no_scratch_no_lds_and_stays_in_budget():
    res = build.kernel_resources("clip_spline_weights.hip")
    assert len(res) == 1, sorted(res)
    (name, r), = res.items()
    print(r)
    assert "clip_spline_weights_kernel" in name and "clip_weights_kernel" not in name
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == 0, r
    assert r["vgprs"] <= 61 and r["sgprs"] <= 46 and r["occupancy"] >= 8, r
    # the neighbours' reports are still their own
    assert not any("clip_spline_weights_kernel" in n for n in build.kernel_resources("clip_weights.hip"))
    assert not any("clip_spline_weights_kernel" in n for n in build.kernel_resources("clip_blend.hip"))
