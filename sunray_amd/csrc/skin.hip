// Linear-blend skinning of a mesh's bind pose (sr_scene_skin_mesh, include/sunray_hip.h states the arithmetic to the letter).
// fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "skin.h"

#include "pose_device.h"

namespace srd {

// One vertex per thread on the tile of vertex_tile.h (96 + 24 bytes in, 96 out per vertex); the arithmetic is skin_vertex of
// pose_device.h.
__global__ void __launch_bounds__(kTileBlock) skin_kernel(const uint4* __restrict__ bind, const uint2* __restrict__ influences,
                                                          const float4* __restrict__ matrices, uint4* __restrict__ out, uint32_t n_vertices,
                                                          uint32_t* first_bad) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const VertexTile vt(n_vertices);
    const uint32_t t = threadIdx.x, v0 = vt.v0, nv = vt.nv;
    vt.load(tile, bind);
    uint32_t bad = 0xFFFFFFFFu;
    if (t < nv && !skin_vertex(VertexTile::row(tile, t), influences + (size_t)(v0 + t) * 3, matrices)) bad = v0 + t;
    vt.store(tile, out);
    report_first_bad(bad, first_bad);
}

}  // namespace srd

int srk_skin(const SrVertex* bind, const SrSkinInfluence* influences, const SrTransform* joint_matrices, SrVertex* out,
             uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kTileBlock - 1) / srd::kTileBlock);
    srd::skin_kernel<<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)bind, (const uint2*)influences, (const float4*)joint_matrices,
                                                                       (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
