// Morph weights of baked clips on the device (sr_scene_pose_actors with SR_ACTOR_CLIP_WEIGHTS), in front of the posing kernel:
// one wave per item samples the item's morph set at its actor's time and compacts the weights that are not 0 into the item's
// active list, which the posing kernel then reads as if the host had uploaded it. The arithmetic is clip_key_search and
// clip_weight of clip_rule.h, which the host rule (sr_clip_weights_host) runs too: fp64 from the fp32 keys, rounded once, no
// contraction, no libm. Host and device give the same bits.
// The four waves of a block are independent: no LDS, no barrier.
#include "clip_weights.h"

namespace srd {

constexpr uint32_t kWeightsBlock = 256, kWeightsWave = 64;

// The row, the clip's headers, the set and the key search are the same for the whole wave: the row index is made uniform, so they
// are scalar loads and scalar arithmetic. The lanes run over the targets in chunks of 64, consecutive lanes on consecutive values
// of the two key rows. The ballot of a chunk orders its survivors: a lane's place is the count so far plus the survivors below it.
__global__ void __launch_bounds__(kWeightsBlock) clip_weights_kernel(const ClipWeightRow* __restrict__ rows, uint32_t n_rows, PoseBatchItem* __restrict__ items,
                                                                     uint32_t* __restrict__ active_index, float* __restrict__ active_weight,
                                                                     uint32_t* __restrict__ check) {
    const uint32_t lane = threadIdx.x % kWeightsWave;
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kWeightsBlock / kWeightsWave) + threadIdx.x / kWeightsWave);
    if (r >= n_rows) return;
    const ClipWeightRow row = rows[r];
    const unsigned char* __restrict__ blk = (const unsigned char*)row.clip;
    const ClipMorphHeader mh = *(const ClipMorphHeader*)(blk + ((const ClipHeader*)blk)->reserved);
    const ClipMorphSet set = ((const ClipMorphSet*)(blk + mh.sets))[row.set];
    const uint32_t n_targets = set.n_targets;
    // the two rows a weight comes from: keys i and i + 1 (or i twice) of the channel, or the defaults twice
    const float* __restrict__ key_a = (const float*)(blk + mh.defaults) + set.first_default;
    const float* __restrict__ key_b = key_a;
    double u = 0.0;
    if (set.n_keys) {
        uint32_t i = 0;
        clip_key_search((const float*)(blk + mh.times) + set.first_time, set.n_keys, set.interpolation, (double)row.time_seconds, &i, &u);
        const float* values = (const float*)(blk + mh.values) + set.first_value;
        key_a = values + (size_t)i * n_targets;
        key_b = values + (size_t)(u > 0.0 ? i + 1 : i) * n_targets;
    }
    uint32_t* __restrict__ out_index = active_index + row.active_base;
    float* __restrict__ out_weight = active_weight + row.active_base;
    uint32_t count = 0;
    for (uint32_t k0 = 0; k0 < n_targets; k0 += kWeightsWave) {
        const uint32_t k = k0 + lane;
        const float w = k < n_targets ? clip_weight(key_a[k], key_b[k], u) : 0.0f;
        const bool active = w != 0.0f;                                      // +0 and -0 are left out, as the host's compaction leaves them
        const uint64_t mask = __ballot(active);
        if (active) {
            const uint32_t at = count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            out_index[at] = k;
            out_weight[at] = w;
        }
        count += (uint32_t)__popcll(mask);
    }
    if (lane == 0) { items[row.item].n_active = count; check[row.check_word] = count; }
}

}  // namespace srd

int srk_clip_weights(const srd::ClipWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                     uint32_t* check, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint32_t per_block = srd::kWeightsBlock / srd::kWeightsWave;
    srd::clip_weights_kernel<<<dim3((n_rows + per_block - 1) / per_block), dim3(srd::kWeightsBlock), 0, stream>>>(rows, n_rows, items, active_index, active_weight, check);
    return (int)hipGetLastError();
}
