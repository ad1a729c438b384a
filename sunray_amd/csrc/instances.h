// The per-instance tables of a frame from transforms in device memory (sr_scene_set_instances_device): launch declaration
// shared by api.cpp and instances.hip, and the one host definition of the same records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/sunray_hip.h"
#include "bvh_gpu.h"
#include "traverse.h"

namespace srd {
struct InstanceLayout { uint32_t tri_offset, mesh_slot; };   // 8 B: what an instance's records hold beside its transform
}

// upload_instance_tables' loop on the device: for each of `n` 48-byte transforms its DevInstance (w2o[0..8] by
// srh::world_to_object_3x3, operation for operation; o2w[0..8] the 3x3 part; the other words 0) into `dev` and its
// FlatInstance (the transform, then `layout`'s two words, the pad 0) into `flat`. The lowest index of a transform with a
// component that is not finite (all 12, the exponent-bits test) goes into *first_bad (0xFFFFFFFF: none); such an instance's
// records are written all the same, so the caller keeps `dev` and `flat` apart from what frames read until it has the answer.
// Every pointer is device memory, 16-byte aligned but for `layout` (8). Returns a hipError_t as int.
int srk_instance_tables(const SrTransform* transforms, const srd::InstanceLayout* layout, uint32_t n, srd::DevInstance* dev, srd::FlatInstance* flat,
                        uint32_t* first_bad, hipStream_t stream);
