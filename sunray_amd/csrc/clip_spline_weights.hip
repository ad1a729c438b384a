// Morph weights of baked clips with a CUBICSPLINE set on the device (sr_scene_pose_actors and sr_scene_pose_actors_blended with
// SR_ACTOR_CLIP_WEIGHTS), in front of the posing kernel: the rows clip_weights_kernel and clip_blend_weights_kernel do not take.
// One wave per item samples the item's set, or its two sets and their cross-fade, and compacts the weights that are not 0 into
// the item's active list, as those kernels do. The arithmetic is clip_spline_key_search, clip_spline_weight (clip_hermite),
// clip_weight and clip_blend_weight of clip_rule.h, which the host rules (sr_clip_weights_host, sr_clip_blend_weights_host)
// run too: fp64 from the fp32 keys, rounded once, + - * / only, no contraction, no libm. Host and device give the same bits.
// It is a kernel of its own because the Hermite form costs registers the two LINEAR / STEP kernels have no use for.
// The four waves of a block are independent: no LDS, no barrier.
#include "clip_spline_weights.h"

namespace srd {

constexpr uint32_t kSplineBlock = 256, kSplineWave = 64;

// One source of a row: the rows a weight comes from, the fraction and the keys' distance. A cubic set: the value and out-tangent
// rows of key i and the value and in-tangent rows of key i + 1 (key i's again where the fraction is 0). Another set: keys i and
// i + 1 (or i twice), or the defaults twice, as in clip_weights_kernel. Wave-uniform: scalar loads and scalar arithmetic.
struct SplineSource { const float* v0; const float* b0; const float* v1; const float* a1; double u, td; uint32_t n_targets, cubic; };
__device__ __forceinline__ SplineSource spline_source(const unsigned char* __restrict__ blk, uint32_t set_at, float time_seconds) {
    const ClipMorphHeader mh = *(const ClipMorphHeader*)(blk + ((const ClipHeader*)blk)->reserved);
    const ClipMorphSet set = ((const ClipMorphSet*)(blk + mh.sets))[set_at];
    const uint32_t n = set.n_targets;
    SplineSource s;
    s.v0 = (const float*)(blk + mh.defaults) + set.first_default;
    s.b0 = s.v1 = s.a1 = s.v0;
    s.u = 0.0; s.td = 0.0; s.n_targets = n; s.cubic = 0;
    if (set.n_keys) {
        const float* times = (const float*)(blk + mh.times) + set.first_time;
        const float* values = (const float*)(blk + mh.values) + set.first_value;
        uint32_t i = 0;
        s.cubic = set.interpolation == kClipCubic ? 1u : 0u;
        if (s.cubic) {
            clip_spline_key_search(times, set.n_keys, (double)time_seconds, &i, &s.u, &s.td);
            const float* key = values + (size_t)i * 3 * n;                      // n in-tangents, values, out-tangents
            const float* next = s.u > 0.0 ? key + (size_t)3 * n : key;
            s.v0 = key + n; s.b0 = key + (size_t)2 * n; s.v1 = next + n; s.a1 = next;
        } else {
            clip_key_search(times, set.n_keys, set.interpolation, (double)time_seconds, &i, &s.u);
            s.v0 = values + (size_t)i * n;
            s.v1 = values + (size_t)(s.u > 0.0 ? i + 1 : i) * n;
        }
    }
    return s;
}
__device__ __forceinline__ float spline_source_weight(const SplineSource& s, uint32_t k) {
    return s.cubic ? clip_spline_weight(s.v0[k], s.b0[k], s.v1[k], s.a1[k], s.u, s.td) : clip_weight(s.v0[k], s.v1[k], s.u);
}

// The row index is made uniform, so the row, the headers, the sets and the key searches are scalar. The lanes run over the targets
// in chunks of 64; the ballot of a chunk orders its survivors: a lane's place is the count so far plus the survivors below it.
__global__ void __launch_bounds__(kSplineBlock) clip_spline_weights_kernel(const ClipSplineWeightRow* __restrict__ rows, uint32_t n_rows,
                                                                           PoseBatchItem* __restrict__ items, uint32_t* __restrict__ active_index,
                                                                           float* __restrict__ active_weight, uint32_t* __restrict__ check) {
    const uint32_t lane = threadIdx.x % kSplineWave;
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kSplineBlock / kSplineWave) + threadIdx.x / kSplineWave);
    if (r >= n_rows) return;
    const ClipSplineWeightRow row = rows[r];
    const bool blended = row.clip_b != nullptr;
    const SplineSource a = spline_source((const unsigned char*)row.clip_a, row.set_a, row.time_a);
    const SplineSource b = blended ? spline_source((const unsigned char*)row.clip_b, row.set_b, row.time_b) : a;
    const uint32_t n_targets = a.n_targets < b.n_targets ? a.n_targets : b.n_targets;          // equal, the host has checked; never past either set
    const double weight = (double)row.weight;
    uint32_t* __restrict__ out_index = active_index + row.active_base;
    float* __restrict__ out_weight = active_weight + row.active_base;
    uint32_t count = 0;
    for (uint32_t k0 = 0; k0 < n_targets; k0 += kSplineWave) {
        const uint32_t k = k0 + lane;
        float w = 0.0f;
        if (k < n_targets) {
            w = spline_source_weight(a, k);
            if (blended) w = clip_blend_weight(w, spline_source_weight(b, k), weight);
        }
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

int srk_clip_spline_weights(const srd::ClipSplineWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                            uint32_t* check, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint32_t per_block = srd::kSplineBlock / srd::kSplineWave;
    srd::clip_spline_weights_kernel<<<dim3((n_rows + per_block - 1) / per_block), dim3(srd::kSplineBlock), 0, stream>>>(rows, n_rows, items, active_index,
                                                                                                                        active_weight, check);
    return (int)hipGetLastError();
}
