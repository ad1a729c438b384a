// Evaluation of baked clips on the device (sr_scene_pose_actors), in front of the posing kernel: one block per actor samples the
// actor's clip at its own time, composes the node hierarchy and writes the joint matrices and the instance transforms. The
// arithmetic is that of clip_rule.h, which the host rule (clip_host.cpp) includes too: fp64 sampling from the fp32 keys rounded
// once, fp32 composition, the inverse in fp64, no contraction.
// A latency-bound kernel of a few hundred fp64 operations an actor: the stages pass their results through the LDS with a barrier
// between them, and every stage loops, so a clip may have more channels, nodes a level or joints than the block has lanes.
#include "clip_pose.h"

namespace srd {

constexpr uint32_t kClipBlock = 256;

// The actor row, the clip header and the tables' bases are the same for the whole block: read at wave-uniform addresses, they
// are scalar loads into scalar registers.
__global__ void __launch_bounds__(kClipBlock) clip_pose_kernel(const ClipActorRow* __restrict__ actors, const uint32_t* __restrict__ rows,
                                                                float4* __restrict__ matrices, float4* __restrict__ instance_transforms,
                                                                uint32_t* __restrict__ check, uint4* __restrict__ keep_trs, float4* __restrict__ keep_globals) {
    __shared__ __attribute__((aligned(16))) float s_trs[kClipMaxNodes * kClipTrsWords];    // a node's TRS; from stage 4 on a skin's inverse (12 floats)
    __shared__ __attribute__((aligned(16))) float s_mat[kClipMaxNodes * 16];               // a node's local, then global matrix
    const ClipActorRow& ar = actors[blockIdx.x];
    const unsigned char* __restrict__ blk = (const unsigned char*)ar.clip;
    const ClipHeader h = *(const ClipHeader*)blk;
    const ClipNode* __restrict__ nodes = (const ClipNode*)(blk + h.nodes);
    const uint32_t t = threadIdx.x;
    const uint32_t n_nodes = h.n_nodes < kClipMaxNodes ? h.n_nodes : kClipMaxNodes;     // the bake refuses more; never past the LDS
    const double time = (double)ar.time_seconds;

    // 0. every node's TRS from the file's
    for (uint32_t n = t; n < n_nodes; n += kClipBlock) {
        const uint4* src = (const uint4*)nodes[n].trs;
        uint4* dst = (uint4*)(s_trs + n * kClipTrsWords);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    }
    __syncthreads();
    // 1. sample: a lane a channel; two channels never share a node and path
    {
        const ClipChannel* __restrict__ channels = (const ClipChannel*)(blk + h.channels);
        const float* __restrict__ times = (const float*)(blk + h.times);
        const float* __restrict__ values = (const float*)(blk + h.values);
        for (uint32_t k = t; k < h.n_channels; k += kClipBlock) {
            const ClipChannel c = channels[k];
            if (c.node >= n_nodes) continue;
            float* dst = s_trs + c.node * kClipTrsWords;
            if (c.path == kClipRotation) {
                float q[4];
                clip_sample_channel<4>(times + c.first_time, values + c.first_value, c.n_keys, c.interpolation, time, q);
                dst[3] = q[0]; dst[4] = q[1]; dst[5] = q[2]; dst[6] = q[3];
            } else {
                float v[3];
                clip_sample_channel<3>(times + c.first_time, values + c.first_value, c.n_keys, c.interpolation, time, v);
                const uint32_t at = c.path == kClipTranslation ? 0u : 7u;
                dst[at] = v[0]; dst[at + 1] = v[1]; dst[at + 2] = v[2];
            }
        }
    }
    __syncthreads();
    // 2. local matrices: a lane a node
    for (uint32_t n = t; n < n_nodes; n += kClipBlock) {
        const float* trs = s_trs + n * kClipTrsWords;
        float4* dst = (float4*)(s_mat + n * 16);
        if (nodes[n].animated) {
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
            uint4* out = keep_trs + ((size_t)ar.node_base + n) * 3;
            out[0] = src[0]; out[1] = src[1]; out[2] = src[2];
        }
    }
    __syncthreads();
    // 3. globals, level by level: a lane a node of the level; a parent is of an earlier level
    {
        const uint32_t* __restrict__ levels = (const uint32_t*)(blk + h.levels);
        for (uint32_t l = 0; l < h.n_levels; l++) {
            const uint32_t first = levels[l], end = levels[l + 1] < n_nodes ? levels[l + 1] : n_nodes;
            for (uint32_t n = first + t; n < end; n += kClipBlock) {
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
        for (uint32_t p = t; p < n_nodes * 4; p += kClipBlock) keep_globals[(size_t)ar.node_base * 4 + p] = ((const float4*)s_mat)[p];
    // 4. joint matrices. A lane a skin inverts the mesh node's global; the TRS are dead and their room takes the inverses.
    const ClipSkin* __restrict__ skins = (const ClipSkin*)(blk + h.skins);
    const uint32_t n_skins = h.n_skins < kClipMaxNodes ? h.n_skins : kClipMaxNodes;
    for (uint32_t k = t; k < n_skins; k += kClipBlock) {
        const uint32_t mesh_node = skins[k].mesh_node;
        float g[16], inv[12];
        for (int i = 0; i < 16; i++) g[i] = mesh_node < n_nodes ? s_mat[mesh_node * 16 + i] : 0.0f;
        if (!clip_invert_affine(g, inv)) atomicMin(check + blockIdx.x, k);
        float4* dst = (float4*)(s_trs + k * 12);
        dst[0] = make_float4(inv[0], inv[1], inv[2], inv[3]); dst[1] = make_float4(inv[4], inv[5], inv[6], inv[7]); dst[2] = make_float4(inv[8], inv[9], inv[10], inv[11]);
    }
    __syncthreads();
    {
        const uint32_t* __restrict__ joint_nodes = (const uint32_t*)(blk + h.joint_nodes);
        const uint32_t* __restrict__ joint_skins = (const uint32_t*)(blk + h.joint_skins);
        const float4* __restrict__ inverse_bind = (const float4*)(blk + h.inverse_bind);
        float4* __restrict__ out = matrices + (size_t)ar.matrix_base * 3;
        for (uint32_t e = t; e < h.n_joints * 3; e += kClipBlock) {       // a lane a 16-byte piece: consecutive lanes, consecutive stores
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
    // 5. instance transforms: a lane a piece
    if (instance_transforms) {
        const uint32_t* __restrict__ inst = (const uint32_t*)(blk + h.instances);
        for (uint32_t e = t; e < h.n_instances * 3; e += kClipBlock) {
            const uint32_t i = e / 3, row = e - 3 * i;
            const uint32_t node = inst[i];
            if (node >= n_nodes) continue;
            const uint32_t to = (ar.flags & 2u) ? rows[ar.rows_base + i] : ar.instance_base + i;
            float r[4];
            if (ar.flags & 1u) {
                float p_row[4], g[16];
                for (int c = 0; c < 4; c++) p_row[c] = ar.placement[row * 4 + c];
                for (int c = 0; c < 16; c++) g[c] = s_mat[node * 16 + c];
                clip_mul_row(p_row, g, r);
            } else
                for (int c = 0; c < 4; c++) r[c] = s_mat[node * 16 + row * 4 + c];
            instance_transforms[(size_t)to * 3 + row] = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

}  // namespace srd

int srk_clip_pose(const srd::ClipActorRow* actors, uint32_t n_actors, const uint32_t* rows, SrTransform* matrices, SrTransform* instance_transforms,
                  uint32_t* check, SrNodeTrs* keep_trs, float* keep_globals, hipStream_t stream) {
    if (n_actors == 0) return 0;
    srd::clip_pose_kernel<<<dim3(n_actors), dim3(srd::kClipBlock), 0, stream>>>(actors, rows, (float4*)matrices, (float4*)instance_transforms, check,
                                                                               (uint4*)keep_trs, (float4*)keep_globals);
    return (int)hipGetLastError();
}
