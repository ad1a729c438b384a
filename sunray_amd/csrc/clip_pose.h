// Clips on the device: launch declaration shared by api.cpp and clip_pose.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "../../include/sunray_hip.h"

// sr_scene_pose_actors: one block per actor evaluates the actor's clip (ClipActorRow.clip, a block of clip_rule.h in device
// memory) at the actor's time under the arithmetic of clip_rule.h: samples the channels, composes the hierarchy level by
// level, and writes
//   - the joint matrices of all the clip's skins to matrices + 3 * (matrix_base + joint) (float4 rows), where the posing kernel
//     reads them;
//   - the instance transforms to instance_transforms[row] (row: rows[rows_base + i], or instance_base + i), premultiplied by
//     the placement where the actor has one; instance_transforms == NULL: none;
//   - check[actor] (preset to 0xFFFFFFFF by the caller): the lowest skin of the clip whose mesh-node transform is singular or
//     whose inverse is not finite;
//   - with keep_trs / keep_globals (both or neither): the sampled TRS (SrNodeTrs) and the global matrices (16 floats) of every
//     node, at node_base + node.
// Every pointer is device memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_pose(const srd::ClipActorRow* actors, uint32_t n_actors, const uint32_t* rows, SrTransform* matrices, SrTransform* instance_transforms,
                  uint32_t* check, SrNodeTrs* keep_trs, float* keep_globals, hipStream_t stream);
