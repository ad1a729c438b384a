// Layer stacks of baked clips on the device: the launch declaration shared by api.cpp and clip_layers.hip, and the composition
// stages of a clip kernel as one __device__ function.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clip_rule.h"
#include "../../include/sunray_hip.h"

// sr_scene_pose_actors_layered: what srk_clip_pose is, for an actor of 1..kClipMaxLayers layers over compatible clips. One block
// per actor samples the base layer into the accumulator, applies every further layer in order (clip_blend_record for an override
// layer, clip_additive_part3 / clip_additive_rotation channel by channel for an additive one, each at the node's effective
// weight), composes the hierarchy once and writes the joint matrices, the instance transforms and check[actor] exactly where
// srk_clip_pose writes them.
//   - with keep_trs / keep_globals (both or neither): the final TRS and the global matrices of every node, at node_base + node;
//   - with keep_cur / keep_ref (both or neither): every layer's sampled records, and for an additive layer those at its reference
//     time, at layer_node_base + layer * n_nodes + node.
// The host has checked every row: the clips of an actor are compatible with its base layer's (sr_clip_blend_compatible), every
// weight and mask value is in [0, 1], a mask has the clip's n_nodes entries, the base layer is an unmasked override at weight 1.
// `targets` (device memory, like the rows) holds where the results go: what srk_clip_pose takes as arguments, and the two
// kept-layers buffers. Every pointer is device memory, 16-byte aligned. Returns a hipError_t as int.
int srk_clip_layers(const srd::ClipLayerActorRow* actors, uint32_t n_actors, const srd::ClipLayerRow* layers, const srd::ClipLayerTargets* targets, hipStream_t stream);

#if defined(__HIPCC__)
namespace srd {

// Where one actor's results go: the fields ClipActorRow, ClipBlendActorRow and ClipLayerActorRow have in common. Wave-uniform.
struct ClipComposeTarget {
    uint32_t flags, matrix_base, instance_base, rows_base, node_base;
    const float* placement;     // the row's twelve floats (read where flags bit 0 is set)
};

// The composition stages of a clip kernel, for a block of BLOCK threads (thread t) that holds the final record of every node in
// s_trs (kClipTrsWords floats a node) and has finished with s_mat (16 floats a node): local matrices (from the TRS where the
// record's mask is not 0, else the file's matrix), globals level by level, skin inverses (into s_trs: the records are dead by
// then), joint matrices, instance transforms; joint matrices and instance transforms as consecutive 16-byte stores. `blk` is the
// clip block whose tables are read (an actor's base clip), n_nodes <= kClipMaxNodes of its nodes. *check_word takes the lowest
// singular skin. The caller has synchronised the block after the last write to s_trs.
template <uint32_t BLOCK>
__device__ __forceinline__ void clip_compose_stages(const unsigned char* __restrict__ blk, uint32_t n_nodes, const ClipComposeTarget& to,
                                                    const uint32_t* __restrict__ rows, float4* __restrict__ matrices, float4* __restrict__ instance_transforms,
                                                    uint32_t* __restrict__ check_word, uint4* __restrict__ keep_trs, float4* __restrict__ keep_globals,
                                                    float* s_trs, float* s_mat, uint32_t t) {
    const ClipHeader h = *(const ClipHeader*)blk;               // wave-uniform: scalar loads
    const ClipNode* __restrict__ nodes = (const ClipNode*)(blk + h.nodes);
    // local matrices: a lane a node
    for (uint32_t n = t; n < n_nodes; n += BLOCK) {
        const float* trs = s_trs + n * kClipTrsWords;
        float4* dst = (float4*)(s_mat + n * 16);
        if (clip_float_word(trs[10])) {
            float tr[3], q[4], sc[3], m[16];
            tr[0] = trs[0]; tr[1] = trs[1]; tr[2] = trs[2]; q[0] = trs[3]; q[1] = trs[4]; q[2] = trs[5]; q[3] = trs[6]; sc[0] = trs[7]; sc[1] = trs[8]; sc[2] = trs[9];
            clip_trs_matrix(tr, q, sc, m);
            dst[0] = make_float4(m[0], m[1], m[2], m[3]); dst[1] = make_float4(m[4], m[5], m[6], m[7]);
            dst[2] = make_float4(m[8], m[9], m[10], m[11]); dst[3] = make_float4(m[12], m[13], m[14], m[15]);
        } else {
            const float4* src = (const float4*)nodes[n].matrix;
            dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
        }
        if (keep_trs) {
            const uint4* src = (const uint4*)trs;
            uint4* out = keep_trs + ((size_t)to.node_base + n) * 3;
            out[0] = src[0]; out[1] = src[1]; out[2] = src[2];
        }
    }
    __syncthreads();
    // globals, level by level: a lane a node of the level; a parent is of an earlier level
    {
        const uint32_t* __restrict__ levels = (const uint32_t*)(blk + h.levels);
        for (uint32_t l = 0; l < h.n_levels; l++) {
            const uint32_t first = levels[l], end = levels[l + 1] < n_nodes ? levels[l + 1] : n_nodes;
            for (uint32_t n = first + t; n < end; n += BLOCK) {
                const uint32_t parent = nodes[n].parent;
                float a[16], b[16], g[16];
                if (parent == kClipNoNode || parent >= n_nodes) clip_identity(a);
                else for (int i = 0; i < 16; i++) a[i] = s_mat[parent * 16 + i];
                for (int i = 0; i < 16; i++) b[i] = s_mat[n * 16 + i];
                clip_mul(a, b, g);
                float4* dst = (float4*)(s_mat + n * 16);
                dst[0] = make_float4(g[0], g[1], g[2], g[3]); dst[1] = make_float4(g[4], g[5], g[6], g[7]);
                dst[2] = make_float4(g[8], g[9], g[10], g[11]); dst[3] = make_float4(g[12], g[13], g[14], g[15]);
            }
            __syncthreads();
        }
    }
    if (keep_globals)
        for (uint32_t p = t; p < n_nodes * 4; p += BLOCK) keep_globals[(size_t)to.node_base * 4 + p] = ((const float4*)s_mat)[p];
    // joint matrices. A lane a skin inverts the mesh node's global; the TRS are dead and their room takes the inverses.
    const ClipSkin* __restrict__ skins = (const ClipSkin*)(blk + h.skins);
    const uint32_t n_skins = h.n_skins < kClipMaxNodes ? h.n_skins : kClipMaxNodes;
    for (uint32_t k = t; k < n_skins; k += BLOCK) {
        const uint32_t mesh_node = skins[k].mesh_node;
        float g[16], inv[12];
        for (int i = 0; i < 16; i++) g[i] = mesh_node < n_nodes ? s_mat[mesh_node * 16 + i] : 0.0f;
        if (!clip_invert_affine(g, inv)) atomicMin(check_word, k);
        float4* dst = (float4*)(s_trs + k * 12);
        dst[0] = make_float4(inv[0], inv[1], inv[2], inv[3]); dst[1] = make_float4(inv[4], inv[5], inv[6], inv[7]); dst[2] = make_float4(inv[8], inv[9], inv[10], inv[11]);
    }
    __syncthreads();
    {
        const uint32_t* __restrict__ joint_nodes = (const uint32_t*)(blk + h.joint_nodes);
        const uint32_t* __restrict__ joint_skins = (const uint32_t*)(blk + h.joint_skins);
        const float4* __restrict__ inverse_bind = (const float4*)(blk + h.inverse_bind);
        float4* __restrict__ out = matrices + (size_t)to.matrix_base * 3;
        for (uint32_t e = t; e < h.n_joints * 3; e += BLOCK) {              // a lane a 16-byte piece: consecutive lanes, consecutive stores
            const uint32_t j = e / 3, row = e - 3 * j;
            const uint32_t node = joint_nodes[j], skin = joint_skins[j];
            if (node >= n_nodes || skin >= n_skins) continue;
            float inv_row[4], g[16], ibm[16], a[4], r[4];
            for (int i = 0; i < 4; i++) inv_row[i] = s_trs[skin * 12 + row * 4 + i];
            for (int i = 0; i < 16; i++) g[i] = s_mat[node * 16 + i];
            const float4 b0 = inverse_bind[j * 3], b1 = inverse_bind[j * 3 + 1], b2 = inverse_bind[j * 3 + 2];
            ibm[0] = b0.x; ibm[1] = b0.y; ibm[2] = b0.z; ibm[3] = b0.w; ibm[4] = b1.x; ibm[5] = b1.y; ibm[6] = b1.z; ibm[7] = b1.w;
            ibm[8] = b2.x; ibm[9] = b2.y; ibm[10] = b2.z; ibm[11] = b2.w; ibm[12] = 0.0f; ibm[13] = 0.0f; ibm[14] = 0.0f; ibm[15] = 1.0f;
            clip_mul_row(inv_row, g, a);            // row `row` of mul(inv, global[joint])
            clip_mul_row(a, ibm, r);                // ... of mul(that, inverse_bind)
            out[e] = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    // instance transforms: a lane a piece
    if (instance_transforms) {
        const uint32_t* __restrict__ inst = (const uint32_t*)(blk + h.instances);
        for (uint32_t e = t; e < h.n_instances * 3; e += BLOCK) {
            const uint32_t i = e / 3, row = e - 3 * i;
            const uint32_t node = inst[i];
            if (node >= n_nodes) continue;
            const uint32_t at = (to.flags & 2u) ? rows[to.rows_base + i] : to.instance_base + i;
            float r[4];
            if (to.flags & 1u) {
                float p_row[4], g[16];
                for (int c = 0; c < 4; c++) p_row[c] = to.placement[row * 4 + c];
                for (int c = 0; c < 16; c++) g[c] = s_mat[node * 16 + c];
                clip_mul_row(p_row, g, r);
            } else
                for (int c = 0; c < 4; c++) r[c] = s_mat[node * 16 + row * 4 + c];
            instance_transforms[(size_t)at * 3 + row] = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

}  // namespace srd
#endif
