// Cross-fades between two baked clips on the device: launch declarations shared by api.cpp and clip_blend.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "pose_batch_plan.h"
#include "../../include/sunray_hip.h"

// sr_scene_pose_actors_blended: what srk_clip_pose is, for an actor of two compatible clips. One block per actor samples clip A at
// time_a and clip B at time_b, blends the two records of every node at the actor's weight (clip_blend_record of clip_rule.h),
// composes the hierarchy once and writes the joint matrices, the instance transforms and check[actor] exactly where
// srk_clip_pose writes them.
//   - with keep_trs / keep_globals (both or neither): the blended TRS and the global matrices of every node, at node_base + node;
//   - with keep_a / keep_b (both or neither): the two sources' sampled TRS, at node_base + node.
// The host has checked every row: the two clips are compatible (sr_clip_blend_compatible) and the weight is in [0, 1]. Every
// pointer is device memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_blend(const srd::ClipBlendActorRow* actors, uint32_t n_actors, const uint32_t* rows, SrTransform* matrices, SrTransform* instance_transforms,
                   uint32_t* check, SrNodeTrs* keep_trs, float* keep_globals, SrNodeTrs* keep_a, SrNodeTrs* keep_b, hipStream_t stream);

// What srk_clip_weights is, for an item of a blended actor: one wave per row samples set_a of clip A and set_b of clip B (equal
// n_targets), blends per target (clip_blend_weight), leaves out the weights that are +-0 and writes the active list and its count
// where srk_clip_weights writes them.
int srk_clip_blend_weights(const srd::ClipBlendWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                           uint32_t* check, hipStream_t stream);
