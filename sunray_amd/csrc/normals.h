// The shading frame of a deforming mesh on the device: launch declaration shared by api.cpp and normals.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sunray_hip.h"
#include "mesh_frame.h"

// sr_scene_update_mesh_positions*: two launches on `stream` under the rule the header states. face_frame_kernel, one thread per
// triangle, gathers the three positions of `indices` (every index is below n_vertices: the attach checked them) from `positions`
// (n_vertices tight float[3]) and writes F, and under SR_FRAME_TANGENTS T from `tri_uv`, into `faces`: one 16-byte piece per
// triangle under SR_FRAME_NORMALS alone, two (F, then T) with tangents. vertex_frame_kernel turns the `reference` records through
// the tile, walks vertex v's run entries[offsets[v] .. offsets[v + 1]) (triangle indices below n_triangles), and writes the new
// records into `out`. The lowest index of a vertex whose position is not finite (the rule of srk_vertex_check: x, y, z only) is
// left in *first_bad (0xFFFFFFFF: none). Every pointer is device memory; reference, faces, tri_uv and out are 16-byte aligned, the
// others 4. Returns a hipError_t as int.
int srk_mesh_frame(const SrVertex* reference, const float* positions, const uint32_t* indices, const srh::FrameTriUv* tri_uv, const uint32_t* offsets,
                   const uint32_t* entries, const float* side, uint32_t flags, float4* faces, SrVertex* out, uint32_t n_vertices, uint32_t n_triangles,
                   uint32_t* first_bad, hipStream_t stream);
