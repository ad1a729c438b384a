// Posing of skinned and morphed meshes in one launch (sr_scene_pose_meshes; sr_scene_skin_mesh and sr_scene_pose_mesh with one
// item): every tile of every item of a batch is one block of one grid. The arithmetic is skin_vertex and morph_vertex of
// pose_device.h, the tile that of vertex_tile.h.
// fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "pose_batch.h"

#include "pose_device.h"

namespace srd {

static_assert(kPoseBatchTile == kTileBlock, "the host plans one block per tile of vertex_tile.h");

// One vertex per thread. The block's item comes from the block table, and everything that is the same for the whole item (its
// row, the active list, the bases) is read at wave-uniform addresses: scalar loads into scalar registers. A fused item's morphed
// position, normal and tangent stay in the thread's row of the LDS tile, where the skin stage reads them: one global read and one
// global write per vertex. A joint index is relative to the item's own slice of the concatenated matrices.
__global__ void __launch_bounds__(kTileBlock) pose_batch_kernel(const PoseBatchItem* __restrict__ items, const uint32_t* __restrict__ block_item,
                                                                 const float4* __restrict__ matrices, const uint32_t* __restrict__ active_index,
                                                                 const float* __restrict__ active_weight, uint4* __restrict__ scratch,
                                                                 uint32_t* check) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const uint32_t i = block_item[blockIdx.x];
    const PoseBatchItem it = items[i];
    const VertexTile vt(it.n_vertices, blockIdx.x - it.first_block);
    const uint32_t t = threadIdx.x, v0 = vt.v0, nv = vt.nv;
    vt.load(tile, (const uint4*)it.src);
    uint32_t bad_morph = 0xFFFFFFFFu, bad_skin = 0xFFFFFFFFu;
    if (t < nv) {
        uint4* row = VertexTile::row(tile, t);
        if ((it.stages & kPoseMorph) && !morph_vertex(row, (const float4*)it.deltas, active_index + it.active_base, active_weight + it.active_base,
                                                      it.n_active, it.n_vertices, v0 + t)) bad_morph = v0 + t;
        if ((it.stages & kPoseSkin) && !skin_vertex(row, (const uint2*)it.influences + (size_t)(v0 + t) * 3, matrices + (size_t)it.matrix_base * 3))
            bad_skin = v0 + t;
    }
    vt.store(tile, scratch + it.vertex_base * kVertexPieces);
    report_first_bad(bad_morph, check + 2 * (size_t)i);
    report_first_bad(bad_skin, check + 2 * (size_t)i + 1);
}

// The same grid, no LDS: a piece goes from the scratch to the same piece of the mesh's own allocation, consecutive lanes on
// consecutive pieces.
__global__ void __launch_bounds__(kTileBlock) pose_batch_scatter_kernel(const PoseBatchItem* __restrict__ items, const uint32_t* __restrict__ block_item,
                                                                         const uint4* __restrict__ scratch) {
    const PoseBatchItem it = items[block_item[blockIdx.x]];
    const VertexTile vt(it.n_vertices, blockIdx.x - it.first_block);
    const uint4* __restrict__ from = scratch + it.vertex_base * kVertexPieces + vt.p0;
    uint4* __restrict__ to = (uint4*)it.dst + vt.p0;
#pragma unroll
    for (uint32_t k = 0; k < kVertexPieces; k++) {
        const uint32_t p = k * kTileBlock + threadIdx.x;
        if (p < vt.np) to[p] = from[p];
    }
}

}  // namespace srd

int srk_pose_batch(const srd::PoseBatchItem* items, const uint32_t* block_item, uint32_t n_blocks, const SrTransform* matrices,
                   const uint32_t* active_index, const float* active_weight, SrVertex* scratch, uint32_t* check, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    srd::pose_batch_kernel<<<dim3(n_blocks), dim3(srd::kTileBlock), 0, stream>>>(items, block_item, (const float4*)matrices, active_index, active_weight,
                                                                                (uint4*)scratch, check);
    return (int)hipGetLastError();
}

int srk_pose_batch_scatter(const srd::PoseBatchItem* items, const uint32_t* block_item, uint32_t n_blocks, const SrVertex* scratch, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    srd::pose_batch_scatter_kernel<<<dim3(n_blocks), dim3(srd::kTileBlock), 0, stream>>>(items, block_item, (const uint4*)scratch);
    return (int)hipGetLastError();
}
