// Device-side acceleration-structure maintenance: launch declarations shared by api.cpp and bvh_gpu.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/sunray_hip.h"

namespace srd {
struct FlatInstance {   // 64 B: what flattening one instance needs
    float o2w[12];      // ObjectToWorld3x4, row-major (EntityTransform, rt_types.slang:101-103)
    uint32_t tri_offset, mesh_slot, _pad[2];
};
struct TlMeshRow {      // 48 B: what one instance record of the two-level form needs of its mesh's tree (by mesh slot)
    float lo[3], hi[3]; // root box of the mesh's tree, object space (padded as the builder pads triangles)
    float max_abs_vertex, max_edge_sum;
    uint32_t max_stack, blas_root, prim_base, n_tris;
};
struct BlasRefitMesh {  // 40 B: one dirty mesh of a mesh-tree refit (two-level form)
    uint64_t vertices, indices;      // device addresses: SrVertex[n_vertices], uint32_t[3 * n_tris]
    uint32_t tri_base, n_tris;       // the mesh's range of the concatenated leaf-order records
    uint32_t n_vertices;
    uint32_t first_thread;           // of blas_records_kernel, a multiple of 64
    uint32_t mesh_slot, textured;    // row of the TlMeshRow table; 1: the mesh has shade_tex records
};
struct DevTlInstance;   // traverse.h
}  // namespace srd

int srk_launch_flatten_slots(float4* tris, const float4* shade, const SrMeshInfo* meshes, const srd::FlatInstance* instances, uint32_t n_tris,
                             hipStream_t stream);
// The same with the slots' shading records rewritten from the (changed) vertices; shade_tex is null where the scene has none.
int srk_launch_flatten_reshade(float4* tris, float4* shade, float4* shade_tex, const SrMeshInfo* meshes, const srd::FlatInstance* instances,
                               uint32_t n_tris, hipStream_t stream);
int srk_launch_refit(uint32_t* nodes, const float4* tris, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host,
                     uint32_t n_levels, hipStream_t stream);

struct LbvhArgs {
    const SrMeshInfo* meshes; const srd::FlatInstance* instances; uint32_t n_instances, n_tris;
    float4* nodes; uint32_t node_cap;                    // node_cap x 64 B
    float4 *tris, *shade, *shade_tex;                    // leaf-order records (shade_tex may be null)
    uint32_t* slot_of_gid; float* node_box;              // n_tris / node_cap x 6 floats
    void* scratch; size_t scratch_bytes;
    uint32_t stack_floor, stack_cap;                     // budget = max(stack_floor, binary height); fail above stack_cap
    int rebalance = 0;                                   // 1: a binary tree taller than stack_cap is rebalanced to fit it instead of refused
    int ploc;                                            // topology: 0 = binary radix tree (LBVH), r > 0 = PLOC with search radius r
    // srk_tl_build only (the primitives are instance boxes; meshes .. slot_of_gid above are unused, n_tris is unused)
    const float* boxes = nullptr; uint32_t n_boxes = 0;  // n_instances x 6 floats, n_boxes of them real (the others are NaN rows)
    uint32_t* tl_inst = nullptr;                         // out: leaf order -> instance index, n_boxes entries
    // srk_blas_build only (the primitives are ONE mesh's object-space triangles; meshes, instances and n_instances above are unused).
    // nodes, node_box, tris, shade, shade_tex and slot_of_gid are the concatenated arrays of all meshes: the tree takes the nodes
    // [node_base, node_base + node_cap) and the leaf-order slots [tri_base, tri_base + n_tris)
    const SrVertex* vertices = nullptr; const uint32_t* indices = nullptr; uint32_t n_vertices = 0;
    uint32_t mesh_slot = 0, textured = 0;                // shade_tex is written only for a textured mesh
    uint32_t node_base = 0, tri_base = 0;
    srd::TlMeshRow* rows = nullptr;                      // out (may be null): the mesh's row of the top-level record table
    uint32_t* out = nullptr;                             // out, 10 dwords: root box lo, hi, max_abs_vertex, max_edge_sum (floats), nodes, stack need
};
struct LbvhResult {
    uint32_t n_nodes = 0, max_stack = 0, max_depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> level_ranges;   // (first node, count) per level, root level first
    // binary walk height of the topology the builder chose / of what was collapsed (set on a refusal for height as well), and what
    // the height bound rebuilt (0, 0 when the tree fitted)
    uint32_t height_before = 0, height_after = 0, subtrees_rebuilt = 0, prims_rebuilt = 0;
};
int srk_lbvh_build(const LbvhArgs& args, LbvhResult* out, hipStream_t stream);
size_t srk_lbvh_scratch_bytes(uint32_t n_tris, uint32_t node_cap);

// Top level of the two-level form. srk_tl_records: DevTlInstance records and padded world boxes of all instances (tl_record.h, as
// the host loop of two_level_build computes them); `result` (device, 3 dwords, zeroed by the call) receives: instances this path cannot take,
// deepest mesh-tree stack, instances with a box. srk_tl_build: the builder above over those boxes; same return convention.
int srk_tl_records(const srd::FlatInstance* instances, const srd::TlMeshRow* meshes, uint32_t n_instances, double max_condition,
                   srd::DevTlInstance* records, float* boxes, uint32_t* result, hipStream_t stream);
int srk_tl_build(const LbvhArgs& args, LbvhResult* out, hipStream_t stream);
size_t srk_tl_scratch_bytes(uint32_t n_instances, uint32_t node_cap);

// Mesh trees of the two-level form after sr_scene_update_mesh. srk_blas_records: the leaf-order records of the dirty meshes
// rewritten from their vertex / index buffers (the bytes of api.cpp build_blas) and, per mesh, root box lo, hi, max_abs_vertex,
// max_edge_sum (build_blas's values, bit for bit) into `out` (8 floats per mesh) and, where `rows` is not null, into the mesh's
// row; `acc` is n_meshes x 8 dwords of scratch, `acc_init` its initial contents (the encoded +inf x 3, -inf x 3, 0, 0 per mesh).
// srk_blas_refit: the quantised nodes of those meshes, one launch per level (lists of global node indices, deepest level first).
int srk_blas_records(const srd::BlasRefitMesh* meshes, uint32_t n_meshes, uint32_t n_threads, float4* tris, float4* shade, float4* shade_tex,
                     uint32_t* acc, const uint32_t* acc_init, srd::TlMeshRow* rows, float* out, hipStream_t stream);
// srk_blas_build: the device fast build of one mesh's tree into its ranges of those arrays (SrAsState asked for SR_OP_FAST_BUILD):
// records, shade, shade_tex and primitive -> slot entries with the bytes of build_blas, references global as the concatenation
// makes them, the eight floats as above. Return convention and scratch size of srk_lbvh_build (n_tris, node_cap).
int srk_blas_build(const LbvhArgs& args, LbvhResult* out, hipStream_t stream);
int srk_blas_refit(uint32_t* nodes, const float4* tris, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host,
                   uint32_t n_levels, hipStream_t stream);

// sr_scene_update_mesh_device: the lowest index of a vertex with a non-finite position (the host's rule: x, y, z only) into
// *first_bad (one device word; 0xFFFFFFFF: none), enqueued on `stream`. `vertices` is 16-byte aligned device memory, read once.
int srk_vertex_check(const SrVertex* vertices, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream);
