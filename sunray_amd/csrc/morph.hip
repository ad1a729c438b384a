// Morph-target (blend shape) evaluation of a mesh's base vertices (sr_scene_pose_mesh, include/sunray_hip.h states the arithmetic
// to the letter). fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "morph.h"

#include "pose_device.h"

namespace srd {

// One vertex per thread on the tile of vertex_tile.h; the arithmetic is morph_vertex of pose_device.h.
__global__ void __launch_bounds__(kTileBlock) morph_kernel(const uint4* __restrict__ base, const float4* __restrict__ deltas,
                                                            const uint32_t* __restrict__ active_index, const float* __restrict__ active_weight,
                                                            uint32_t n_active, uint4* __restrict__ out, uint32_t n_vertices, uint32_t* first_bad) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const VertexTile vt(n_vertices);
    const uint32_t t = threadIdx.x, v0 = vt.v0, nv = vt.nv;
    vt.load(tile, base);
    uint32_t bad = 0xFFFFFFFFu;
    if (t < nv && !morph_vertex(VertexTile::row(tile, t), deltas, active_index, active_weight, n_active, n_vertices, v0 + t)) bad = v0 + t;
    vt.store(tile, out);
    report_first_bad(bad, first_bad);
}

}  // namespace srd

int srk_morph(const SrVertex* base, const SrMorphDelta* deltas, const uint32_t* active_index, const float* active_weight, uint32_t n_active,
              SrVertex* out, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kTileBlock - 1) / srd::kTileBlock);
    srd::morph_kernel<<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)base, (const float4*)deltas, active_index, active_weight, n_active,
                                                                         (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
