// Batched posing (sr_scene_pose_meshes): the host-side layout. Which block of the one launch works on which tile of which item,
// where an item's records sit in the batch scratch, and how the single staging block of a call is laid out.
// No HIP here: a stand-alone program links pose_batch_plan.cpp and brings srh::set_error, the one symbol it needs from outside.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/sunray_hip.h"

namespace srd {

constexpr uint32_t kPoseBatchTile = 256;    // vertices a block: kTileBlock of vertex_tile.h (pose_batch.hip asserts it)
constexpr uint32_t kPoseMorph = 1u, kPoseSkin = 2u;

// One item of a batch as the kernels read it, at wave-uniform addresses. Every pointer is device memory, 16-byte aligned.
struct PoseBatchItem {
    const void* src;            // n_vertices records: the morph base where the item has a morph stage, the bind pose otherwise
    const void* deltas;         // morph stage: target-major delta records
    const void* influences;     // skin stage: n_vertices influence records
    void* dst;                  // the mesh's own vertices (the scatter launch writes them)
    uint64_t vertex_base;       // first record of the item in the batch scratch
    uint32_t n_vertices, first_block;
    uint32_t n_active, active_base;     // morph stage: its slice of the concatenated active lists
    uint32_t matrix_base;       // skin stage: first matrix of its slice of the concatenated joint matrices
    uint32_t stages;            // kPoseMorph | kPoseSkin
};
static_assert(sizeof(PoseBatchItem) == 64, "an item row is four 16-byte pieces");

}  // namespace srd

namespace srh {

int set_error(int code, const std::string& msg);   // the library's error slot (api.cpp); returns `code`

// Byte offsets of the parts of a call's staging block, each 16-byte aligned: the item rows, the block table (one uint32_t per
// block: its item), the joint matrices of all items, the active indices and the active weights of all items.
struct PoseBatchLayout { size_t items, block_table, matrices, active_index, active_weight, bytes; };
PoseBatchLayout pose_batch_layout(uint32_t n_items, uint32_t n_blocks, uint64_t n_matrices, uint64_t n_active);

// table[b] = the item whose tiles hold block b, from the first blocks of sr_pose_batch_plan (an item without vertices has none).
void pose_batch_block_table(const uint32_t* first_block, uint32_t n_items, uint32_t n_blocks, uint32_t* table);

}  // namespace srh
