// Morph weights from baked clips with a CUBICSPLINE set on the device: launch declaration shared by api.cpp and
// clip_spline_weights.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "pose_batch_plan.h"

// What srk_clip_weights and srk_clip_blend_weights are, for the items they do not take: a row whose set (clip_b null), or at
// least one of whose two sets, is kClipCubic. One wave per row samples set_a of clip A at time_a and, where clip_b is given,
// set_b of clip B at time_b (equal n_targets) under the arithmetic of clip_rule.h (clip_spline_weight_at for a cubic set,
// clip_weight_at for another), blends the two at the share `weight` of B (clip_blend_weight), leaves out the weights that are +-0
// and writes the list, its count and the check word where srk_clip_weights writes them.
// The host has checked every row: the sets exist and are available, the slot holds n_targets entries. Every pointer is device
// memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_spline_weights(const srd::ClipSplineWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                            uint32_t* check, hipStream_t stream);
