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

// The resident concatenated arrays of all mesh trees of the two-level form: where a mesh-tree writer (srk_blas_build, the batched
// build, the refit's record kernel) writes.
namespace srd {
struct BlasBatchArrays {
    uint32_t* nodes; float* node_box;
    float4 *tris, *shade, *shade_tex;             // shade_tex may be null
    uint32_t* slot_of_gid;
    TlMeshRow* rows;                              // may be null
};
}  // namespace srd

// Arguments of the three device tree builders. A struct is built by its constructor alone, which takes every field: a value a
// call site leaves out is a compile error.
struct TreeBuildTarget {          // what the three builders share
    float4* nodes; uint32_t node_cap;                    // node_cap x 64 B
    float* node_box;                                     // node_cap x 6 floats
    void* scratch; size_t scratch_bytes;                 // srk_*_scratch_bytes of the same sizes and topology
    uint32_t stack_floor, stack_cap;                     // budget = max(stack_floor, binary height); fail above stack_cap
    int rebalance;                                       // 1: a binary tree taller than stack_cap is rebalanced to fit it instead of refused
    int ploc;                                            // topology: 0 = binary radix tree (LBVH), r > 0 = PLOC with search radius r
    TreeBuildTarget(float4* nodes, uint32_t node_cap, float* node_box, void* scratch, size_t scratch_bytes, uint32_t stack_floor, uint32_t stack_cap,
                    int rebalance, int ploc)
        : nodes(nodes), node_cap(node_cap), node_box(node_box), scratch(scratch), scratch_bytes(scratch_bytes), stack_floor(stack_floor),
          stack_cap(stack_cap), rebalance(rebalance), ploc(ploc) {}
};
struct TrisBuildArgs : TreeBuildTarget {      // srk_lbvh_build: the primitives are the instances' world-space triangles
    const SrMeshInfo* meshes; const srd::FlatInstance* instances; uint32_t n_instances, n_tris;
    float4 *tris, *shade, *shade_tex;                    // out: leaf-order records, n_tris each (shade_tex null: the scene has none)
    uint32_t* slot_of_gid;                               // out: n_tris
    TrisBuildArgs(const TreeBuildTarget& target, const SrMeshInfo* meshes, const srd::FlatInstance* instances, uint32_t n_instances, uint32_t n_tris,
                  float4* tris, float4* shade, float4* shade_tex, uint32_t* slot_of_gid)
        : TreeBuildTarget(target), meshes(meshes), instances(instances), n_instances(n_instances), n_tris(n_tris), tris(tris), shade(shade),
          shade_tex(shade_tex), slot_of_gid(slot_of_gid) {}
};
struct BoxesBuildArgs : TreeBuildTarget {     // srk_tl_build: the primitives are the instance boxes of a top-level tree
    const float* boxes; uint32_t n_instances, n_boxes;   // n_instances x 6 floats, n_boxes of them real (the others are NaN rows)
    uint32_t* tl_inst;                                   // out: leaf order -> instance index, n_boxes entries
    BoxesBuildArgs(const TreeBuildTarget& target, const float* boxes, uint32_t n_instances, uint32_t n_boxes, uint32_t* tl_inst)
        : TreeBuildTarget(target), boxes(boxes), n_instances(n_instances), n_boxes(n_boxes), tl_inst(tl_inst) {}
};
// srk_blas_build: the primitives are ONE mesh's object-space triangles. The tree takes the nodes [node_base, node_base + node_cap)
// and the leaf-order slots [tri_base, tri_base + n_tris) of `arrays`, whose nodes and node_box are the target's.
struct MeshBuildArgs : TreeBuildTarget {
    srd::BlasBatchArrays arrays;
    const SrVertex* vertices; const uint32_t* indices; uint32_t n_vertices, n_tris;
    uint32_t mesh_slot, textured;                        // shade_tex is written only for a textured mesh
    uint32_t node_base, tri_base;
    uint32_t* out;                                       // out, 10 dwords: root box lo, hi, max_abs_vertex, max_edge_sum (floats), nodes, stack need
    MeshBuildArgs(const srd::BlasBatchArrays& arrays, uint32_t node_base, uint32_t node_cap, uint32_t tri_base, void* scratch, size_t scratch_bytes,
                  uint32_t stack_floor, uint32_t stack_cap, int rebalance, int ploc, const SrVertex* vertices, const uint32_t* indices, uint32_t n_vertices,
                  uint32_t n_tris, uint32_t mesh_slot, uint32_t textured, uint32_t* out)
        : TreeBuildTarget((float4*)arrays.nodes, node_cap, arrays.node_box, scratch, scratch_bytes, stack_floor, stack_cap, rebalance, ploc), arrays(arrays),
          vertices(vertices), indices(indices), n_vertices(n_vertices), n_tris(n_tris), mesh_slot(mesh_slot), textured(textured), node_base(node_base),
          tri_base(tri_base), out(out) {}
};
struct LbvhResult {
    uint32_t n_nodes = 0, max_stack = 0, max_depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> level_ranges;   // (first node, count) per level, root level first
    // binary walk height of the topology the builder chose / of what was collapsed (set on a refusal for height as well), and what
    // the height bound rebuilt (0, 0 when the tree fitted)
    uint32_t height_before = 0, height_after = 0, subtrees_rebuilt = 0, prims_rebuilt = 0;
};
// Return 0, a hipError_t (> 0), or -1 when the tree does not fit the limits (the caller falls back to the host builder). The scratch
// sizes are exact: the end of the one carve the build itself uses (bvh_gpu.hip TreeScratch), for the same sizes and topology.
int srk_lbvh_build(const TrisBuildArgs& args, LbvhResult* out, hipStream_t stream);
size_t srk_lbvh_scratch_bytes(uint32_t n_tris, uint32_t node_cap, int ploc);

// Top level of the two-level form. srk_tl_records: DevTlInstance records and padded world boxes of all instances (tl_record.h, as
// the host loop of two_level_build computes them); `result` (device, 3 dwords, zeroed by the call) receives: instances this path cannot take,
// deepest mesh-tree stack, instances with a box. srk_tl_build: the builder above over those boxes; same return convention.
int srk_tl_records(const srd::FlatInstance* instances, const srd::TlMeshRow* meshes, uint32_t n_instances, double max_condition,
                   srd::DevTlInstance* records, float* boxes, uint32_t* result, hipStream_t stream);
int srk_tl_build(const BoxesBuildArgs& args, LbvhResult* out, hipStream_t stream);
size_t srk_tl_scratch_bytes(uint32_t n_instances, uint32_t n_boxes, uint32_t node_cap, int ploc);

// Mesh trees of the two-level form after sr_scene_update_mesh. srk_blas_records: the leaf-order records of the dirty meshes
// rewritten from their vertex / index buffers (the bytes of api.cpp build_blas) and, per mesh, root box lo, hi, max_abs_vertex,
// max_edge_sum (build_blas's values, bit for bit) into `out` (8 floats per mesh) and, where `rows` is not null, into the mesh's
// row; `acc` is n_meshes x 8 dwords of scratch, `acc_init` its initial contents (the encoded +inf x 3, -inf x 3, 0, 0 per mesh).
// srk_blas_refit: the quantised nodes of those meshes, one launch per level (lists of global node indices, deepest level first).
int srk_blas_records(const srd::BlasRefitMesh* meshes, uint32_t n_meshes, uint32_t n_threads, float4* tris, float4* shade, float4* shade_tex,
                     uint32_t* acc, const uint32_t* acc_init, srd::TlMeshRow* rows, float* out, hipStream_t stream);
// srk_blas_build: the device fast build of one mesh's tree into its ranges of those arrays (SrAsState asked for SR_OP_FAST_BUILD):
// records, shade, shade_tex and primitive -> slot entries with the bytes of build_blas, references global as the concatenation
// makes them, the eight floats as above. Return convention and scratch size of srk_lbvh_build (n_tris, node_cap, ploc).
int srk_blas_build(const MeshBuildArgs& args, LbvhResult* out, hipStream_t stream);
int srk_blas_refit(uint32_t* nodes, const float4* tris, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host,
                   uint32_t n_levels, hipStream_t stream);

// sr_scene_update_mesh_device: the lowest index of a vertex with a non-finite position (the host's rule: x, y, z only) into
// *first_bad (one device word; 0xFFFFFFFF: none), enqueued on `stream`. `vertices` is 16-byte aligned device memory, read once.
int srk_vertex_check(const SrVertex* vertices, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream);
