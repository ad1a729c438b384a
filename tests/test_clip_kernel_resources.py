"""The compiler's report for clip_pose_kernel (sunray_amd/csrc/clip_pose.hip): no scratch, no spills, the static LDS the node cap
asks for, and a register figure within the budget read from the first build (144 VGPRs, 3 waves a SIMD: the fp64 sampling and
the fp64 inverse are the long live ranges; the kernel is latency-bound, one block an actor, and three waves a SIMD hold a block
of four waves on every CU several times over). No GPU."""
from sunray_amd import abi, build


def test_clip_pose_kernel_has_no_scratch_and_stays_in_budget():
    res = build.kernel_resources("clip_pose.hip")
    mine = [r for name, r in res.items() if "clip_pose_kernel" in name]
    assert len(mine) == 1, sorted(res)
    r = mine[0]
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == abi.CLIP_MAX_NODES * (12 + 16) * 4, r            # a node's TRS (three pieces) and its matrix (four)
    assert r["lds"] <= 64 * 1024 and r["vgprs"] <= 144 and r["occupancy"] >= 3, r
    assert any("pose_batch_kernel" in name for name in build.kernel_resources("pose_batch.hip"))      # that report is still its own
