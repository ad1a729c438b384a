// Morph-target blending on the device: launch declaration shared by api.cpp and morph.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sunray_hip.h"

// sr_scene_pose_mesh's morph stage: blends `n_vertices` base records with the active targets under the arithmetic the header
// states, into `out`, and leaves the lowest index of a morphed vertex whose position is not finite (the rule of
// srk_vertex_check: x, y, z only) in *first_bad (0xFFFFFFFF: none). `deltas` is target-major: target k's records for vertices
// 0..n_vertices-1 are contiguous, so record (k, v) is deltas[k * n_vertices + v]. `active_index` / `active_weight` list the
// n_active targets whose weight is not 0, in ascending target order; every index is below the attached target count (the host
// compacted the list from it). n_active == 0 copies the base. Every pointer is device memory, 16-byte aligned (the two lists: 4).
// Returns a hipError_t as int.
int srk_morph(const SrVertex* base, const SrMorphDelta* deltas, const uint32_t* active_index, const float* active_weight, uint32_t n_active,
              SrVertex* out, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream);
