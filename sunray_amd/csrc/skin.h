// Linear-blend skinning on the device: launch declaration shared by api.cpp and skin.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sunray_hip.h"

// sr_scene_skin_mesh: poses `n_vertices` bind-pose records with the joint matrices (rows of 3x4, n_joints of them, device
// memory) under the arithmetic the header states, into `out`, and leaves the lowest index of a posed vertex whose position is
// not finite (the rule of srk_vertex_check: x, y, z only) in *first_bad (0xFFFFFFFF: none). Every pointer is device memory,
// 16-byte aligned; `influences` holds n_vertices records whose non-zero weights name joints below n_joints (the attach call
// checked that). Returns a hipError_t as int.
int srk_skin(const SrVertex* bind, const SrSkinInfluence* influences, const SrTransform* joint_matrices, SrVertex* out,
             uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream);
