// Morph weights from baked clips on the device: launch declaration shared by api.cpp and clip_weights.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "pose_batch_plan.h"

// sr_scene_pose_actors, between clip_pose_kernel and the posing kernel: one wave per row samples morph set `set` of the row's
// clip (a block of clip_rule.h in device memory) at the row's time under the arithmetic of clip_rule.h, leaves out the weights
// that are +-0 and writes
//   - the indices and weights of the others, in ascending target order, to active_index / active_weight + active_base (a slot of
//     the set's n_targets entries);
//   - their count to items[item].n_active, where the posing kernel reads it, and to check[check_word].
// The host has checked every row: the set exists and is available, the slot holds n_targets entries. Every pointer is device
// memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_weights(const srd::ClipWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                     uint32_t* check, hipStream_t stream);
