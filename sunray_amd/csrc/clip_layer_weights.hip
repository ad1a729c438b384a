// Morph weights through an actor's layer stack on the device (sr_scene_pose_actors_layered with SR_ACTORS_LAYER_WEIGHTS), behind
// clip_layers_kernel and in front of the posing kernel. One wave per clip-weighted item walks the item's actor's layers: it samples
// each layer's morph set for the item's blas at the layer's time, and at the reference time too where the layer is additive, and
// applies the rule of clip_rule.h (clip_blend_weight, clip_additive_weight at the effective weight) onto one accumulator per
// target; then it compacts the weights that are not 0 into the item's active list, as clip_weights_kernel does. The sets of a row
// may be LINEAR, STEP, cubic or defaults in any mix. The host rule (sr_clip_weights_layers_host) runs the same functions: fp64 from
// the fp32 values, each layer rounded once, + - * / only, no contraction, no libm. Host and device give the same bits.
// The four waves of a block are independent: no LDS, no barrier.
#include "clip_layer_weights.h"

namespace srd {

constexpr uint32_t kLayerWeightsBlock = 256, kLayerWeightsWave = 64;

// The set of a source, from the block alone. Wave-uniform: scalar loads.
__device__ __forceinline__ ClipMorphSet layer_weights_set(const unsigned char* __restrict__ blk, uint32_t set_at) {
    const uint32_t sets = ((const ClipMorphHeader*)(blk + ((const ClipHeader*)blk)->reserved))->sets;
    return ((const ClipMorphSet*)(blk + sets))[set_at];
}

// Target k of set `set_at` of the clip at `blk` at `time_seconds`. Everything but the last line is wave-uniform, scalar loads and
// scalar arithmetic: the headers, the set, the key search, the fraction. Nothing of it outlives the call, so a layer holds no
// pointer while the next one is sampled; a lane's part is the two or four loads of its target and clip_weight / clip_spline_weight.
__device__ __forceinline__ float layer_weights_sample(const unsigned char* __restrict__ blk, uint32_t set_at, float time_seconds, uint32_t k) {
    const ClipMorphHeader mh = *(const ClipMorphHeader*)(blk + ((const ClipHeader*)blk)->reserved);
    const ClipMorphSet set = ((const ClipMorphSet*)(blk + mh.sets))[set_at];
    const uint32_t n = set.n_targets;
    if (set.n_keys == 0) return ((const float*)(blk + mh.defaults))[set.first_default + k];
    const float* times = (const float*)(blk + mh.times) + set.first_time;
    const float* values = (const float*)(blk + mh.values) + set.first_value;
    uint32_t i = 0;
    double u = 0.0, td = 0.0;
    if (set.interpolation == kClipCubic) {
        clip_spline_key_search(times, set.n_keys, (double)time_seconds, &i, &u, &td);
        return clip_spline_weight_at(values, n, i, u, td, k);
    }
    clip_key_search(times, set.n_keys, set.interpolation, (double)time_seconds, &i, &u);
    return clip_weight_at(values, n, i, u, k);
}

// The row index is made uniform, so the row, the layers, the entries, the headers, the sets and the key searches are scalar. The
// lanes run over the targets in chunks of 64, the layers inside a chunk: a lane holds one accumulator. The scalar work of a layer
// is redone per chunk, so only sets above 64 targets pay it again. The ballot of a chunk orders its survivors: a lane's place is
// the count so far plus the survivors below it.
__global__ void __launch_bounds__(kLayerWeightsBlock) clip_layer_weights_kernel(const ClipLayerWeightRow* __restrict__ rows, uint32_t n_rows,
                                                                                const ClipLayerRow* __restrict__ layers,
                                                                                const ClipLayerWeightEntry* __restrict__ entries,
                                                                                PoseBatchItem* __restrict__ items, uint32_t* __restrict__ active_index,
                                                                                float* __restrict__ active_weight, uint32_t* __restrict__ check) {
    const uint32_t lane = threadIdx.x % kLayerWeightsWave;
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kLayerWeightsBlock / kLayerWeightsWave) + threadIdx.x / kLayerWeightsWave);
    if (r >= n_rows) return;
    const ClipLayerWeightRow row = rows[r];
    const uint32_t n_layers = row.n_layers < kClipMaxLayers ? row.n_layers : kClipMaxLayers;
    uint32_t n_targets = n_layers ? 0xFFFFFFFFu : 0u;        // the smallest set's: equal, the host has checked; never past any set
    for (uint32_t l = 0; l < n_layers; l++) {
        const uint32_t n = layer_weights_set((const unsigned char*)layers[row.first_layer + l].clip, entries[row.first_entry + l].set).n_targets;
        n_targets = n < n_targets ? n : n_targets;
    }
    uint32_t* __restrict__ out_index = active_index + row.active_base;
    float* __restrict__ out_weight = active_weight + row.active_base;
    uint32_t count = 0;
    for (uint32_t k0 = 0; k0 < n_targets; k0 += kLayerWeightsWave) {
        const uint32_t k = k0 + lane;
        float acc = 0.0f;
        if (k < n_targets) {
            for (uint32_t l = 0; l < n_layers; l++) {
                const ClipLayerRow ly = layers[row.first_layer + l];
                const ClipLayerWeightEntry en = entries[row.first_entry + l];
                const unsigned char* blk = (const unsigned char*)ly.clip;
                if (l == 0) { acc = layer_weights_sample(blk, en.set, ly.time_seconds, k); continue; }      // the base
                const float m = ly.mask != nullptr && en.mask_node != kClipNoNode ? ly.mask[en.mask_node] : 1.0f;
                const double w = clip_layer_set_weight(ly.weight, m);
                if (w == 0.0) continue;                                        // wave-uniform; either rule returns acc: the layer is not sampled
                const float cur = layer_weights_sample(blk, en.set, ly.time_seconds, k);
                if (ly.mode == kClipLayerAdditive) acc = clip_additive_weight(acc, cur, layer_weights_sample(blk, en.set, ly.ref_time_seconds, k), w);
                else acc = clip_blend_weight(acc, cur, w);
            }
        }
        const bool active = acc != 0.0f;                                    // +0 and -0 are left out, as the host's compaction leaves them
        const uint64_t mask = __ballot(active);
        if (active) {
            const uint32_t at = count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            out_index[at] = k;
            out_weight[at] = acc;
        }
        count += (uint32_t)__popcll(mask);
    }
    if (lane == 0) { items[row.item].n_active = count; check[row.check_word] = count; }
}

}  // namespace srd

int srk_clip_layer_weights(const srd::ClipLayerWeightRow* rows, uint32_t n_rows, const srd::ClipLayerRow* layers, const srd::ClipLayerWeightEntry* entries,
                           srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight, uint32_t* check, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint32_t per_block = srd::kLayerWeightsBlock / srd::kLayerWeightsWave;
    srd::clip_layer_weights_kernel<<<dim3((n_rows + per_block - 1) / per_block), dim3(srd::kLayerWeightsBlock), 0, stream>>>(rows, n_rows, layers, entries, items,
                                                                                                                             active_index, active_weight, check);
    return (int)hipGetLastError();
}
