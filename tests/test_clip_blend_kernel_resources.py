"""The compiler's report for the two kernels of sunray_amd/csrc/clip_blend.hip: no scratch, no spills; clip_blend_kernel's static
LDS is the formula its comment states, kClipMaxNodes * (12 + 16) * 4 bytes (the second source's records lie in the matrices' room
until the blend is done, so it is clip_pose_kernel's 42 KiB), and clip_blend_weights_kernel has none. The register figures are the
budget read from the first build: clip_blend_kernel 152 VGPRs, 3 waves a SIMD (clip_pose_kernel: 144, 3; the blend stage holds two
records of twelve words, the blended one and a part's fp64 operands at once, on top of the fp64 sampling and inverse); the weights
kernel 30 VGPRs, 8 waves. No GPU."""
from sunray_amd import abi, build


def kernels():
    res = build.kernel_resources("clip_blend.hip")
    blend = [r for name, r in res.items() if "clip_blend_kernel" in name]
    weights = [r for name, r in res.items() if "clip_blend_weights_kernel" in name]
    assert len(blend) == 1 and len(weights) == 1 and len(res) == 2, sorted(res)
    assert not any("clip_pose_kernel" in name for name in res)
    return blend[0], weights[0]


def test_clip_blend_kernel_has_no_scratch_and_stays_in_budget():
    r, _ = kernels()
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == abi.CLIP_MAX_NODES * (12 + 16) * 4, r            # a node's TRS (three pieces) and its matrix (four); B's TRS shares the matrix's room
    assert r["lds"] <= 64 * 1024 and r["vgprs"] <= 152 and r["occupancy"] >= 3, r


def test_clip_blend_weights_kernel_has_no_scratch_no_lds_and_stays_in_budget():
    _, r = kernels()
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, r
    assert r["lds"] == 0, r
    assert r["vgprs"] <= 30 and r["occupancy"] >= 8, r
