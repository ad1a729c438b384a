// Layer stacks of baked clips on the device (sr_scene_pose_actors_layered), in front of the posing kernel: what clip_pose.hip is
// for an actor of one clip and clip_blend.hip for an actor of two, for an actor of 1..kClipMaxLayers layers. One block per actor
// samples the base layer into the accumulator, applies every further layer in order at each node's effective weight
// (weight x mask), composes the hierarchy once (clip_compose_stages) and writes the joint matrices and the instance transforms
// where clip_pose_kernel writes them. The arithmetic is that of clip_rule.h, which the host rule (clip_host.cpp) includes too;
// the layer rule is + - * / and sqrt in fp64 rounded once per part, so that stage is bit equal between host and device without
// exception, and everything composed from the final records is too.
// Static LDS: kClipMaxNodes * (12 + 16) * 4 bytes = 42 KiB, clip_pose_kernel's.
//   - The accumulator lies in the TRS array.
//   - An override layer's sampled records lie in the matrices' room (12 of a node's 16 floats), which is not written before the
//     last layer is done; then a lane a node combines (clip_blend_record), the result going over the accumulator.
//   - An additive layer's records at its reference time lie there too, by the same code. Then the lane that owns a channel
//     samples it at the layer's time in registers and applies the rule to that part of the accumulator in place, against the
//     reference part in the matrices' room. A clip's channels never share a node and path, and a part without a channel has
//     equal bytes at both times, which the rule copies: the channel-wise form gives the node-wise rule's bytes. The record's mask
//     word is the node's own lane's to OR (a lane a node), so no two lanes write one word and no atomic is needed.
//     (Sampling at both times in registers, with no LDS for an additive layer at all, was the first form: two inlined samplings
//     in the layer loop cost 24 spilled scalar registers.)
#include "clip_layers.h"

namespace srd {

constexpr uint32_t kLayersBlock = 256;

__device__ __forceinline__ uint32_t layers_part_at(uint32_t path) { return path == kClipTranslation ? 0u : path == kClipRotation ? 3u : 7u; }

// What the block needs again only after the layers (and, keeping, between them) waits in idle LDS, not in scalar registers: a
// node's slot of 16 floats in the matrices' room holds a record of 12 until the composition, so words 12..15 of the first two
// slots are free until then. The sampling code leaves few scalar registers over, and these values would be spilled.
__device__ __forceinline__ void layers_park(uint32_t* at, const void* p) { at[0] = (uint32_t)(uintptr_t)p; at[1] = (uint32_t)((uintptr_t)p >> 32); }
__device__ __forceinline__ const void* layers_parked(const uint32_t* at) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)at[0]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)at[1]);   // unsigned: no sign extension into the high word
    return (const void*)(uintptr_t)(((uint64_t)hi << 32) | (uint64_t)lo);
}

// The actor row, its layer rows, the call's targets, every layer's clip header, weight and mask base are the same for the whole block: read at
// wave-uniform addresses, they are scalar loads into scalar registers. The tables that the host has found equal across the
// actor's clips (nodes but their masks, levels, skins, joints, instances) are read from the base layer's block.
__global__ void __launch_bounds__(kLayersBlock) clip_layers_kernel(const ClipLayerActorRow* __restrict__ actors, const ClipLayerRow* __restrict__ layers,
                                                                   const ClipLayerTargets* __restrict__ targets) {
    __shared__ __attribute__((aligned(16))) float s_trs[kClipMaxNodes * kClipTrsWords];    // the accumulator; from the skin stage on a skin's inverse (12 floats)
    __shared__ __attribute__((aligned(16))) float s_mat[kClipMaxNodes * 16];               // an override layer's records; then a node's local, then global matrix
    const ClipLayerActorRow& ar = actors[blockIdx.x];
    const ClipLayerRow* __restrict__ stack = layers + ar.first_layer;
    const uint32_t n_layers = ar.n_layers < kClipMaxLayers ? ar.n_layers : kClipMaxLayers;     // the host refuses more
    const unsigned char* __restrict__ blk = (const unsigned char*)stack[0].clip;
    const uint32_t t = threadIdx.x;
    uint32_t* s_row = (uint32_t*)s_mat + 12;                    // parked: the actor's row, the targets, the base clip's block
    uint32_t* s_targets = (uint32_t*)s_mat + 14;
    uint32_t* s_blk = (uint32_t*)s_mat + 16 + 12;
    uint32_t* s_actor = (uint32_t*)s_mat + 16 + 14;             // ... the actor's index, its first layer row
    uint32_t* s_stack = (uint32_t*)s_mat + 32 + 12;
    uint32_t* s_count = (uint32_t*)s_mat + 32 + 14;             // ... and their number
    if (t == 0) { layers_park(s_row, &ar); layers_park(s_targets, targets); layers_park(s_blk, blk); *s_actor = blockIdx.x; layers_park(s_stack, stack); *s_count = n_layers; }
    __syncthreads();
    const uint32_t base_nodes = ((const ClipHeader*)blk)->n_nodes;
    const uint32_t n_nodes = base_nodes < kClipMaxNodes ? base_nodes : kClipMaxNodes;           // the bake refuses more; never past the LDS

    // Layer 0, the base, is sampled straight into the accumulator; every further layer into the matrices' room; an additive layer
    // takes a second pass, at its own time, whose samples are applied as they come. One rolled loop over layers and passes, so the
    // sampling code, the kernel's heaviest user of scalar registers, stands once.
    for (uint32_t l = 0; l < (uint32_t)__builtin_amdgcn_readfirstlane((int)*s_count); l++) {
        // each field of the layer's row is read where it is used: a weight or a mask base held across the sampling would be spilled
#define lr (((const ClipLayerRow*)layers_parked(s_stack))[l])
#define keep (((const ClipLayerTargets*)layers_parked(s_targets))->keep_cur != nullptr)     // SR_ACTORS_KEEP_LAYERS: asked where it matters, not held
        const unsigned char* __restrict__ blk_l = (const unsigned char*)lr.clip;
        const ClipHeader& hl = *(const ClipHeader*)blk_l;
        const ClipNode* __restrict__ nodes_l = (const ClipNode*)(blk_l + hl.nodes);
        const uint32_t n_l = hl.n_nodes < n_nodes ? hl.n_nodes : n_nodes;                       // equal, the host has checked; never past the layer's table
#define additive (l != 0 && lr.mode == kClipLayerAdditive)      // the base is an override layer, the host has checked
        float* s_dst = l ? s_mat : s_trs;
        const uint32_t stride = l ? 16u : kClipTrsWords;
#pragma unroll 1
        for (uint32_t pass = 0; pass < (additive ? 2u : 1u); pass++) {
            const bool apply = pass != 0;
            if (!apply) {
                // the layer's records start from the file's TRS
                for (uint32_t n = t; n < n_l; n += kLayersBlock) {
                    const uint4* src = (const uint4*)nodes_l[n].trs;
                    uint4* dst = (uint4*)(s_dst + n * stride);
                    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
                }
            }
            if (!apply || keep) __syncthreads();                // second pass, keeping: its lanes write the records the node stage has just read
            // a lane a channel: the base or an override layer at its time, an additive layer at its reference time, into the
            // records; an additive layer's second pass at its time, applied to that part of the accumulator in place
            {
                const ClipChannel* __restrict__ channels = (const ClipChannel*)(blk_l + hl.channels);
                const float* __restrict__ times = (const float*)(blk_l + hl.times);
                const float* __restrict__ values = (const float*)(blk_l + hl.values);
                const double time = (double)(additive && !apply ? lr.ref_time_seconds : lr.time_seconds);
                for (uint32_t k = t; k < hl.n_channels; k += kLayersBlock) {
                    const ClipChannel c = channels[k];
                    if (c.node >= n_l) continue;
                    const bool rotation = c.path == kClipRotation;
                    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (rotation) clip_sample_channel<4>(times + c.first_time, values + c.first_value, c.n_keys, c.interpolation, time, v);
                    else clip_sample_channel<3>(times + c.first_time, values + c.first_value, c.n_keys, c.interpolation, time, v);
                    const uint32_t at = layers_part_at(c.path);
                    float* part = s_dst + c.node * stride + at;
                    if (!apply) {
                        part[0] = v[0]; part[1] = v[1]; part[2] = v[2]; if (rotation) part[3] = v[3];
                        continue;
                    }
                    const uint32_t cur[4] = {clip_float_word(v[0]), clip_float_word(v[1]), clip_float_word(v[2]), clip_float_word(v[3])};
                    const uint32_t ref[4] = {clip_float_word(part[0]), clip_float_word(part[1]), clip_float_word(part[2]), rotation ? clip_float_word(part[3]) : 0u};
                    const double w = clip_layer_weight(lr.weight, lr.mask, c.node);
                    if (w != 0.0 && clip_float_word(s_dst[c.node * stride + 10]) != 0u) {
                        uint32_t* acc = (uint32_t*)(s_trs + c.node * kClipTrsWords) + at;
                        if (rotation) clip_additive_rotation(acc, cur, ref, w, acc);
                        else clip_additive_part3(acc, cur, ref, w, acc);
                    }
                    if (keep) { part[0] = v[0]; part[1] = v[1]; part[2] = v[2]; if (rotation) part[3] = v[3]; }      // the record at the layer's time, part by part
                }
            }
            __syncthreads();
            // a lane a node
            if (l == 0 || apply) {
                // the base's records, or an additive layer's at its time, are kept as they lie
                if (keep) {
                    uint4* __restrict__ keep_cur = (uint4*)((const ClipLayerTargets*)layers_parked(s_targets))->keep_cur;
                    const size_t kept_at = (size_t)((const ClipLayerActorRow*)layers_parked(s_row))->layer_node_base + (size_t)(l * n_nodes);
                    for (uint32_t n = t; n < n_l; n += kLayersBlock) {
                        const uint4* rec = (const uint4*)(s_dst + n * stride);
                        uint4* out = keep_cur + (kept_at + n) * 3;
                        out[0] = rec[0]; out[1] = rec[1]; out[2] = rec[2];
                    }
                }
            } else if (!additive) {
                // the combined record, with its effective mask, goes over the accumulator
                uint4* __restrict__ keep_cur = keep ? (uint4*)((const ClipLayerTargets*)layers_parked(s_targets))->keep_cur : nullptr;
                const size_t kept_at = keep ? (size_t)((const ClipLayerActorRow*)layers_parked(s_row))->layer_node_base + (size_t)(l * n_nodes) : 0;
                for (uint32_t n = t; n < n_l; n += kLayersBlock) {
                    uint4* rec_a = (uint4*)(s_trs + n * kClipTrsWords);
                    const uint4* rec_b = (const uint4*)(s_mat + n * 16);
                    const uint4 a0 = rec_a[0], a1 = rec_a[1], a2 = rec_a[2], b0 = rec_b[0], b1 = rec_b[1], b2 = rec_b[2];
                    if (keep) { uint4* out = keep_cur + (kept_at + n) * 3; out[0] = b0; out[1] = b1; out[2] = b2; }
                    const uint32_t a[kClipTrsWords] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
                    const uint32_t b[kClipTrsWords] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
                    uint32_t r[kClipTrsWords];
                    clip_blend_record(a, b, clip_layer_weight(lr.weight, lr.mask, n), r);
                    rec_a[0] = make_uint4(r[0], r[1], r[2], r[3]); rec_a[1] = make_uint4(r[4], r[5], r[6], r[7]); rec_a[2] = make_uint4(r[8], r[9], r[10], r[11]);
                }
            } else {
                // an additive layer's first pass: the accumulator's mask word, and the kept reference records
                uint4* __restrict__ keep_ref = keep ? (uint4*)((const ClipLayerTargets*)layers_parked(s_targets))->keep_ref : nullptr;
                const size_t kept_at = keep ? (size_t)((const ClipLayerActorRow*)layers_parked(s_row))->layer_node_base + (size_t)(l * n_nodes) : 0;
                for (uint32_t n = t; n < n_l; n += kLayersBlock) {
                    const uint4* rec = (const uint4*)(s_mat + n * 16);
                    const uint32_t animated = rec[2].z;         // the clip's mask of the node: word 10 of both of its sampled records
                    uint32_t* word = (uint32_t*)(s_trs + n * kClipTrsWords) + 10;
                    if (animated != 0u && clip_layer_weight(lr.weight, lr.mask, n) != 0.0) *word |= animated;
                    if (keep) { uint4* out = keep_ref + (kept_at + n) * 3; out[0] = rec[0]; out[1] = rec[1]; out[2] = rec[2]; }
                }
            }
        }
        __syncthreads();
#undef lr
#undef keep
#undef additive
    }
    // back from the idle LDS, before the composition writes the matrices over it
    const ClipLayerActorRow& row = *(const ClipLayerActorRow*)layers_parked(s_row);
    const ClipLayerTargets& out = *(const ClipLayerTargets*)layers_parked(s_targets);
    const unsigned char* __restrict__ base = (const unsigned char*)layers_parked(s_blk);
    uint32_t* __restrict__ check_word = out.check + (uint32_t)__builtin_amdgcn_readfirstlane((int)*s_actor);
    __syncthreads();
    const ClipComposeTarget to{row.flags, row.matrix_base, row.instance_base, row.rows_base, row.node_base, row.placement};
    clip_compose_stages<kLayersBlock>(base, n_nodes, to, out.rows, (float4*)out.matrices, (float4*)out.instance_transforms, check_word,
                                      (uint4*)out.keep_trs, (float4*)out.keep_globals, s_trs, s_mat, t);
}

}  // namespace srd

int srk_clip_layers(const srd::ClipLayerActorRow* actors, uint32_t n_actors, const srd::ClipLayerRow* layers, const srd::ClipLayerTargets* targets, hipStream_t stream) {
    if (n_actors == 0) return 0;
    srd::clip_layers_kernel<<<dim3(n_actors), dim3(srd::kLayersBlock), 0, stream>>>(actors, layers, targets);
    return (int)hipGetLastError();
}
