// The frame's light table built on the device (SR_LIGHTS_DEVICE): launch declarations shared by api.cpp and lights.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sunray_hip.h"
#include "bvh_gpu.h"

// srh::light_table (host_prep.cpp) on the device, operation for operation: one 64-byte DevLight per indirection entry, from the
// entry's arena slot (`arena`, n_arena records) and its instance's ObjectToWorld (`instances`, n_instances records), into
// `lights` (n_entries x 64 bytes). An entry that names a slot or an instance out of range is not written. Every pointer is
// device memory, 16-byte aligned. Returns a hipError_t as int.
int srk_light_table(const SrEmissiveIndirectionEntry* entries, uint32_t n_entries, const SrEmissiveTriangle* arena, uint32_t n_arena,
                    const srd::FlatInstance* instances, uint32_t n_instances, float* lights, hipStream_t stream);

// The positions of a mesh's arena slots from its device vertices, for a mesh whose emissive list is one per triangle in index
// order: x, y, z of v0, v1, v2 of arena[slots[k]] from vertices[indices[3k .. 3k + 2]].position. The w words and the emission
// are not written. A triangle that names a vertex or a slot out of range is not written.
int srk_emissive_positions(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, const uint32_t* slots, uint32_t n_tris,
                           SrEmissiveTriangle* arena, uint32_t n_arena, hipStream_t stream);
