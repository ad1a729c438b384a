"""The compiler's report for the kernel of sunray_amd/csrc/clip_layers.hip: no scratch, no spills, and static LDS equal to
clip_pose_kernel's, kClipMaxNodes * (12 + 16) * 4 bytes (the accumulator lies in the TRS array, a layer's sampled records in the
matrices' room, and what the block needs again only after the layers waits in the idle words of that room). The register figures
are the budget read from the first build: 154 VGPRs, 3 waves a SIMD (clip_blend_kernel: 152, 3; clip_pose_kernel: 144, 3). No GPU."""
from sunray_amd import abi, build


def kernel():
    res = build.kernel_resources("clip_layers.hip")
    assert len(res) == 1 and "clip_layers_kernel" in list(res)[0], sorted(res)
    return list(res.values())[0]


def test_clip_layers_kernel_has_no_scratch_no_spills_and_stays_in_budget():
    r = kernel()
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == abi.CLIP_MAX_NODES * (12 + 16) * 4, r
    pose = [p for name, p in build.kernel_resources("clip_pose.hip").items() if "clip_pose_kernel" in name]
    assert len(pose) == 1 and r["lds"] == pose[0]["lds"], (r, pose)
    assert r["vgprs"] <= 154 and r["occupancy"] >= 3, r
