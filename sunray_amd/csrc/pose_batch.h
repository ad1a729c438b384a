// Batched posing on the device: launch declarations shared by api.cpp and pose_batch.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pose_batch_plan.h"

// The pose path (sr_scene_pose_meshes; sr_scene_skin_mesh and sr_scene_pose_mesh with one item): poses every item of a batch in one launch of `n_blocks` blocks, block b on tile b - first_block of item
// block_item[b], into `scratch` at the item's vertex_base, under morph_vertex and skin_vertex of pose_device.h (a fused item's morphed
// vectors stay in the LDS tile between the stages). check[2 * i] / check[2 * i + 1] (preset to 0xFFFFFFFF by the caller) take the
// lowest vertex of item i whose morphed / skinned position is not finite. An item's joints index `matrices + 3 * matrix_base`
// (float4 rows), its active list is active_index / active_weight + active_base. Every pointer is device memory, 16-byte aligned.
// Returns a hipError_t as int.
int srk_pose_batch(const srd::PoseBatchItem* items, const uint32_t* block_item, uint32_t n_blocks, const SrTransform* matrices,
                   const uint32_t* active_index, const float* active_weight, SrVertex* scratch, uint32_t* check, hipStream_t stream);
// The accepted batch: the same grid copies every item's records, tile by tile, from `scratch` into the item's `dst`.
int srk_pose_batch_scatter(const srd::PoseBatchItem* items, const uint32_t* block_item, uint32_t n_blocks, const SrVertex* scratch, hipStream_t stream);
