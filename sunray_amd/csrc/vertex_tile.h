// The tile scaffold of the kernels that produce or check a mesh's vertices on the device (pose_batch_kernel,
// vertex_frame_kernel, vertex_check_kernel): constants, the turn of a tile of records through the LDS, and the report of the lowest bad vertex.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sunray_hip.h"

namespace srd {

// One block works on a tile of 256 vertices, one vertex per thread. The producers are memory-bound (a 96-byte record in, one
// out, per vertex), so the records cross global memory as 16-byte pieces, six per vertex, consecutive lanes on consecutive
// pieces (coalesced dwordx4, the walk of vertex_check_kernel), and are turned by the LDS: a thread reads the three pieces of its
// own vertex that posing changes (position, normal, tangent), writes them back in place, and the tile leaves as it came. The uv
// sets and the pads are never in a register of the posing thread: every byte that is not rewritten is the source's. A row of
// the tile is seven pieces, not six: lanes 28 dwords apart fall on sixteen different 16-byte slots of the LDS in every group
// of 16 lanes that one ds_read_b128 serves (24 dwords apart they would share slots in pairs). 28 KiB per block: five blocks a CU.
constexpr uint32_t kTileBlock = 256, kVertexPieces = sizeof(SrVertex) / 16, kTileRow = kVertexPieces + 1;
static_assert(sizeof(SrVertex) == 96 && offsetof(SrVertex, position) == 0 && offsetof(SrVertex, normal) == 16 && offsetof(SrVertex, tangent) == 32,
              "position, normal and tangent are the first three 16-byte pieces of a vertex");

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// v * (1 / sqrt(dot(v, v))) into the first three words of *piece; a squared length that is 0 or not finite leaves the piece alone
__device__ __forceinline__ void store_normalised(uint4* piece, float x, float y, float z) {
    const float len2 = (x * x + y * y) + z * z;
    if (len2 == 0.0f || !finite_bits(len2)) return;
    const float r = 1.0f / sqrtf(len2);
    piece->x = __float_as_uint(x * r); piece->y = __float_as_uint(y * r); piece->z = __float_as_uint(z * r);
}

// A block's tile of a mesh, by default tile blockIdx.x of a kTileBlock-wide launch over ceil(n_vertices / 256) blocks: `tile` is
// kTileBlock * kTileRow pieces of LDS.
struct VertexTile {
    uint32_t v0, nv, np;        // first vertex (v0 < n_vertices), vertices and pieces in this tile
    uint64_t p0;                // first piece: 64-bit (n_vertices * 6 need not fit 32)
    __device__ __forceinline__ explicit VertexTile(uint32_t n_vertices) : VertexTile(n_vertices, blockIdx.x) {}
    // tile `tile_index` of a mesh of n_vertices, for a block that serves one of many meshes (pose_batch_kernel)
    __device__ __forceinline__ VertexTile(uint32_t n_vertices, uint32_t tile_index)
        : v0(tile_index * kTileBlock), nv(min(kTileBlock, n_vertices - v0)), np(nv * kVertexPieces), p0((uint64_t)v0 * kVertexPieces) {}
    // thread t's own row, valid between load() and store() while t < nv
    __device__ __forceinline__ static uint4* row(uint4* tile, uint32_t t) { return tile + t * kTileRow; }
    __device__ __forceinline__ void load(uint4* tile, const uint4* __restrict__ src) const {
        const uint32_t t = threadIdx.x;
        const uint4* __restrict__ from = src + p0;
#pragma unroll
        for (uint32_t k = 0; k < kVertexPieces; k++) {
            const uint32_t p = k * kTileBlock + t;
            if (p < np) tile[p + p / kVertexPieces] = from[p];
        }
        __syncthreads();
    }
    __device__ __forceinline__ void store(const uint4* tile, uint4* __restrict__ out) const {
        const uint32_t t = threadIdx.x;
        __syncthreads();
        uint4* __restrict__ to = out + p0;
#pragma unroll
        for (uint32_t k = 0; k < kVertexPieces; k++) {
            const uint32_t p = k * kTileBlock + t;
            if (p < np) to[p] = tile[p + p / kVertexPieces];
        }
    }
};

// the lowest offending vertex (0xFFFFFFFF: this lane has none): one reduction per wave (cross-lane moves, no LDS), at most one
// atomicMin per wave reaches `first_bad` (preset to 0xFFFFFFFF). Every lane of the wave calls it.
__device__ __forceinline__ void report_first_bad(uint32_t bad, uint32_t* first_bad) {
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o, 64));
    if ((threadIdx.x & 63u) == 0 && bad != 0xFFFFFFFFu) atomicMin(first_bad, bad);
}

}  // namespace srd
