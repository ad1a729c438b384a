// Morph weights through an actor's layer stack on the device: launch declaration shared by api.cpp and clip_layer_weights.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "pose_batch_plan.h"

// What srk_clip_weights is for a layered call with SR_ACTORS_LAYER_WEIGHTS: one wave per row walks the row's actor's layers
// (layers[row.first_layer + l], entries[row.first_entry + l]), samples each layer's set at the layer's time (and at its reference
// time where the layer is additive) under the arithmetic of clip_rule.h, applies clip_blend_weight / clip_additive_weight at the
// effective weight (double)weight * (double)mask[entry.mask_node] (1 without a mask or a node), leaves out the weights that are
// +-0 and writes the list, its count and the check word where srk_clip_weights writes them.
// The host has checked every row: the sets exist, are available and hold equal n_targets, the slot holds n_targets entries, a
// mask node lies inside its mask. Every pointer is device memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_layer_weights(const srd::ClipLayerWeightRow* rows, uint32_t n_rows, const srd::ClipLayerRow* layers, const srd::ClipLayerWeightEntry* entries,
                           srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight, uint32_t* check, hipStream_t stream);
