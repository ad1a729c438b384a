// Batched posing: the host-side layout (pose_batch_plan.h). No HIP in this file.
#include "pose_batch_plan.h"

namespace srh {

namespace {
size_t align16(size_t n) { return (n + 15u) & ~(size_t)15u; }
}  // namespace

PoseBatchLayout pose_batch_layout(uint32_t n_items, uint32_t n_blocks, uint64_t n_matrices, uint64_t n_active) {
    PoseBatchLayout l;
    l.items = 0;
    l.block_table = l.items + sizeof(srd::PoseBatchItem) * (size_t)n_items;
    l.matrices = l.block_table + align16(sizeof(uint32_t) * (size_t)n_blocks);
    l.active_index = l.matrices + sizeof(SrTransform) * (size_t)n_matrices;
    l.active_weight = l.active_index + align16(sizeof(uint32_t) * (size_t)n_active);
    l.bytes = l.active_weight + align16(sizeof(float) * (size_t)n_active);
    return l;
}

void pose_batch_block_table(const uint32_t* first_block, uint32_t n_items, uint32_t n_blocks, uint32_t* table) {
    for (uint32_t i = 0; i < n_items; i++) {
        const uint32_t end = i + 1 < n_items ? first_block[i + 1] : n_blocks;
        for (uint32_t b = first_block[i]; b < end; b++) table[b] = i;
    }
}

}  // namespace srh

extern "C" int sr_pose_batch_plan(const uint32_t* n_vertices, uint32_t n_items, uint32_t* first_block, uint64_t* vertex_base, uint32_t* n_blocks) {
    if (!n_blocks || (n_items && (!n_vertices || !first_block || !vertex_base))) return srh::set_error(SR_ERR_INVALID_ARG, "pose_batch_plan: null argument");
    // the totals first (64-bit: 2^32 items of 2^32 - 1 vertices fit), so that a refused batch writes nothing
    uint64_t blocks = 0, vertices = 0;
    for (uint32_t i = 0; i < n_items; i++) {
        blocks += ((uint64_t)n_vertices[i] + srd::kPoseBatchTile - 1) / srd::kPoseBatchTile;
        vertices += n_vertices[i];
    }
    if (blocks >= (1ull << 31)) return srh::set_error(SR_ERR_UNSUPPORTED, "pose_batch_plan: the batch needs " + std::to_string(blocks) + " blocks, 2^31 or more");
    if (vertices >= (1ull << 32)) return srh::set_error(SR_ERR_UNSUPPORTED, "pose_batch_plan: the batch holds " + std::to_string(vertices) + " vertices, 2^32 or more");
    blocks = 0; vertices = 0;
    for (uint32_t i = 0; i < n_items; i++) {
        first_block[i] = (uint32_t)blocks;
        vertex_base[i] = vertices;
        blocks += ((uint64_t)n_vertices[i] + srd::kPoseBatchTile - 1) / srd::kPoseBatchTile;
        vertices += n_vertices[i];
    }
    *n_blocks = (uint32_t)blocks;
    return SR_OK;
}
