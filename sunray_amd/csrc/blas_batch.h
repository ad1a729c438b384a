// Batched device fast build of many small mesh trees of the two-level form: one launch, one workgroup per mesh (blas_batch.hip).
// Shared by api.cpp and blas_batch.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "bvh_gpu.h"

namespace srd {
// Threads of the workgroup that builds one mesh; the sort holds kBlasBatchItems keys per thread (512 x 8 = SR_BLAS_BATCH_MAX_TRIS).
// tests/test_gpu_mesh_tree_batch.py mirrors the block size as BATCH_BLOCK.
constexpr uint32_t kBlasBatchBlock = 512;
constexpr uint32_t kBlasBatchItems = 8;
constexpr uint32_t kBlasBatchMaxTris = kBlasBatchBlock * kBlasBatchItems;
static_assert(kBlasBatchMaxTris == SR_BLAS_BATCH_MAX_TRIS, "the sort of one workgroup holds exactly the largest batched mesh");
constexpr uint32_t kBlasBatchMaxLevels = 32;      // (first, count) pairs a result row holds; a tree within a stack cap of 26 has fewer

enum : uint32_t { kBlasBatchBuilt = 0, kBlasBatchTooTall = 1, kBlasBatchFailed = 2 };

struct BlasBatchRow {       // 64 B: one mesh of the batch
    uint64_t vertices, indices;      // device addresses: SrVertex[n_vertices], uint32_t[3 * n_tris]
    uint64_t scratch;                // the mesh's slab of the scratch buffer, srk_blas_batch_slab_bytes(n_tris, node_cap) bytes, 256-byte aligned
    uint32_t n_tris, n_vertices;
    uint32_t mesh_slot, textured;    // row of the TlMeshRow table; 1: the mesh has shade_tex records
    uint32_t node_base, node_cap;    // the mesh's range of the concatenated node arrays
    uint32_t tri_base;               // ... and of the leaf-order records (n_tris slots)
    uint32_t stack_floor, stack_cap; // budget of the collapse = max(stack_floor, binary height); too_tall above stack_cap
    uint32_t _pad;
};
struct BlasBatchResult {    // 320 B: what the host reads back per mesh
    uint32_t out[10];                // srk_blas_build's block: root box lo, hi, max_abs_vertex, max_edge_sum (floats), nodes, stack need
    uint32_t status;                 // kBlasBatch*; the mesh's resident ranges and TlMeshRow were written only under kBlasBatchBuilt
    uint32_t height;                 // binary walk height of the topology (valid unless the topology stage itself failed)
    uint32_t n_levels;
    uint32_t reserved[3];
    uint32_t levels[2 * kBlasBatchMaxLevels];     // (first node, count) per level, root level first, local to the mesh's node range
};
static_assert(sizeof(BlasBatchRow) == 64 && sizeof(BlasBatchResult) == 320, "rows the host packs and reads back");
}  // namespace srd

// Bytes of one mesh's scratch slab (a multiple of 256).
size_t srk_blas_batch_slab_bytes(uint32_t n_tris, uint32_t node_cap);
// Builds rows[0 .. n_rows) (device memory), one workgroup each, and fills results[0 .. n_rows) (device memory). `ploc` as TreeBuildTarget's.
// The call only enqueues; every result row is written by its workgroup (the caller presets `status` to something else than built).
int srk_blas_batch_build(const srd::BlasBatchRow* rows, uint32_t n_rows, const srd::BlasBatchArrays& arrays, srd::BlasBatchResult* results, int ploc,
                         hipStream_t stream);
