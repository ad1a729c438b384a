// The shading frame of a deforming mesh from its positions alone (sr_scene_set_mesh_frame / sr_scene_update_mesh_positions*,
// include/sunray_hip.h states the rule to the letter): the host side. Smoothing groups and the per-vertex runs of triangles are
// fixed at the attach; sr_mesh_frame_host is the whole rule on the host, operation for operation the one of normals.hip.
// No HIP here: a stand-alone program links mesh_frame.cpp and brings srh::set_error, the one symbol it needs from outside.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sunray_hip.h"

namespace srh {

int set_error(int code, const std::string& msg);   // the library's error slot (api.cpp); returns `code`

// What the face kernel needs of a triangle's uvs, which never change through this path: a.y, b.y and the sign s of
// det = a.x * b.y - b.x * a.y (+1, -1; 0 where det is 0 or not finite: the triangle's T is (+0, +0, +0)). 16 bytes.
struct FrameTriUv { float ay, by, s, _pad; };

// Everything sr_scene_set_mesh_frame uploads, and the figures of SrMeshFrameInfo.
struct MeshFrame {
    std::vector<uint32_t> offsets;      // n_vertices + 1: vertex v's entries are entries[offsets[v] .. offsets[v + 1])
    std::vector<uint32_t> entries;      // triangle indices, ascending (t, c) within a run, one per corner in v's group
    std::vector<float> side;            // per vertex +1 / -1
    std::vector<FrameTriUv> tri_uv;     // per triangle
    uint32_t n_groups = 0, max_valence = 0;
};

// Builds `out` from the reference records. SR_ERR_INVALID_ARG: n_indices % 3 != 0, an index >= n_vertices (the text names the
// lowest offender), a null array that is not empty; SR_ERR_OOM: more than 2^32 - 1 entries. With count_only, entries and side stay
// empty and *n_entries alone tells (the counting call). `who` begins the texts.
int mesh_frame_build(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, bool count_only,
                     MeshFrame& out, uint64_t* n_entries, const char* who);

}  // namespace srh
