// Cross-fades between two baked clips on the device (sr_scene_pose_actors_blended), in front of the posing kernel: what
// clip_pose.hip and clip_weights.hip are for an actor of one clip, for an actor of two. One block per actor samples both clips,
// each at its own time, blends the two records of every node at the actor's weight, composes the hierarchy once and writes the
// joint matrices and the instance transforms where clip_pose_kernel writes them. The arithmetic is that of clip_rule.h, which the
// host rule (clip_host.cpp) includes too; the blend (clip_blend_record) is + - * / and sqrt in fp64 rounded once, so that stage is
// bit equal between host and device without exception, and everything composed from the blended records is too.
// Static LDS: kClipMaxNodes * (12 + 16) * 4 bytes = 42 KiB, clip_pose_kernel's. The second source needs no room of its own: the
// node matrices are not written before the blend is done, so until then B's records lie in the matrices' room (12 of a node's 16
// floats), and the blended record goes over A's.
#include "clip_blend.h"

namespace srd {

constexpr uint32_t kBlendBlock = 256;

// One source's channels at its time into an array of `stride` floats a node: a lane a channel; two channels of one clip never
// share a node and path.
__device__ __forceinline__ void blend_sample(const unsigned char* __restrict__ blk, const ClipHeader& h, uint32_t n_nodes, double time, float* s_dst, uint32_t stride,
                                             uint32_t t) {
    const ClipChannel* __restrict__ channels = (const ClipChannel*)(blk + h.channels);
    const float* __restrict__ times = (const float*)(blk + h.times);
    const float* __restrict__ values = (const float*)(blk + h.values);
    for (uint32_t k = t; k < h.n_channels; k += kBlendBlock) {
        const ClipChannel c = channels[k];
        if (c.node >= n_nodes) continue;
        float* dst = s_dst + c.node * stride;
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

// The actor row, both clip headers, the weight and the tables' bases are the same for the whole block: read at wave-uniform
// addresses, they are scalar loads into scalar registers. The tables that the host has found equal in both clips (nodes but
// their masks, levels, skins, joints, instances) are read from A's block.
__global__ void __launch_bounds__(kBlendBlock) clip_blend_kernel(const ClipBlendActorRow* __restrict__ actors, const uint32_t* __restrict__ rows,
                                                                 float4* __restrict__ matrices, float4* __restrict__ instance_transforms,
                                                                 uint32_t* __restrict__ check, uint4* __restrict__ keep_trs, float4* __restrict__ keep_globals,
                                                                 uint4* __restrict__ keep_a, uint4* __restrict__ keep_b) {
    __shared__ __attribute__((aligned(16))) float s_trs[kClipMaxNodes * kClipTrsWords];    // A's TRS, then the blended one; from stage 4 on a skin's inverse (12 floats)
    __shared__ __attribute__((aligned(16))) float s_mat[kClipMaxNodes * 16];               // B's TRS until the blend; then a node's local, then global matrix
    const ClipBlendActorRow& ar = actors[blockIdx.x];
    const unsigned char* __restrict__ blk = (const unsigned char*)ar.clip_a;
    const unsigned char* __restrict__ blk_b = (const unsigned char*)ar.clip_b;
    const ClipHeader h = *(const ClipHeader*)blk;
    const ClipHeader hb = *(const ClipHeader*)blk_b;
    const ClipNode* __restrict__ nodes = (const ClipNode*)(blk + h.nodes);
    const ClipNode* __restrict__ nodes_b = (const ClipNode*)(blk_b + hb.nodes);
    const uint32_t t = threadIdx.x;
    const uint32_t n_a = h.n_nodes < kClipMaxNodes ? h.n_nodes : kClipMaxNodes;         // the bake refuses more; never past the LDS
    const uint32_t n_nodes = hb.n_nodes < n_a ? hb.n_nodes : n_a;                       // equal, the host has checked; never past B's table
    const double weight = (double)ar.weight;

    // 0. every node's TRS from the file's, with each clip's own mask
    for (uint32_t n = t; n < n_nodes; n += kBlendBlock) {
        const uint4* src = (const uint4*)nodes[n].trs;
        const uint4* src_b = (const uint4*)nodes_b[n].trs;
        uint4* dst = (uint4*)(s_trs + n * kClipTrsWords);
        uint4* dst_b = (uint4*)(s_mat + n * 16);
        dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
        dst_b[0] = src_b[0]; dst_b[1] = src_b[1]; dst_b[2] = src_b[2];
    }
    __syncthreads();
    // 1. sample both sources
    blend_sample(blk, h, n_nodes, (double)ar.time_a, s_trs, kClipTrsWords, t);
    blend_sample(blk_b, hb, n_nodes, (double)ar.time_b, s_mat, 16u, t);
    __syncthreads();
    // 2. blend: a lane a node; the blended record, with its effective mask, goes over A's
    for (uint32_t n = t; n < n_nodes; n += kBlendBlock) {
        uint4* rec_a = (uint4*)(s_trs + n * kClipTrsWords);
        const uint4* rec_b = (const uint4*)(s_mat + n * 16);
        const uint4 a0 = rec_a[0], a1 = rec_a[1], a2 = rec_a[2], b0 = rec_b[0], b1 = rec_b[1], b2 = rec_b[2];
        if (keep_a) {
            uint4* out_a = keep_a + ((size_t)ar.node_base + n) * 3;
            uint4* out_b = keep_b + ((size_t)ar.node_base + n) * 3;
            out_a[0] = a0; out_a[1] = a1; out_a[2] = a2;
            out_b[0] = b0; out_b[1] = b1; out_b[2] = b2;
        }
        const uint32_t a[kClipTrsWords] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
        const uint32_t b[kClipTrsWords] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w};
        uint32_t r[kClipTrsWords];
        clip_blend_record(a, b, weight, r);
        rec_a[0] = make_uint4(r[0], r[1], r[2], r[3]); rec_a[1] = make_uint4(r[4], r[5], r[6], r[7]); rec_a[2] = make_uint4(r[8], r[9], r[10], r[11]);
    }
    __syncthreads();
    // 3. local matrices: a lane a node; from the TRS where the record's mask says so, else the file's matrix
    for (uint32_t n = t; n < n_nodes; n += kBlendBlock) {
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
            uint4* out = keep_trs + ((size_t)ar.node_base + n) * 3;
            out[0] = src[0]; out[1] = src[1]; out[2] = src[2];
        }
    }
    __syncthreads();
    // 4. globals, level by level: a lane a node of the level; a parent is of an earlier level
    {
        const uint32_t* __restrict__ levels = (const uint32_t*)(blk + h.levels);
        for (uint32_t l = 0; l < h.n_levels; l++) {
            const uint32_t first = levels[l], end = levels[l + 1] < n_nodes ? levels[l + 1] : n_nodes;
            for (uint32_t n = first + t; n < end; n += kBlendBlock) {
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
        for (uint32_t p = t; p < n_nodes * 4; p += kBlendBlock) keep_globals[(size_t)ar.node_base * 4 + p] = ((const float4*)s_mat)[p];
    // 5. joint matrices. A lane a skin inverts the mesh node's global; the TRS are dead and their room takes the inverses.
    const ClipSkin* __restrict__ skins = (const ClipSkin*)(blk + h.skins);
    const uint32_t n_skins = h.n_skins < kClipMaxNodes ? h.n_skins : kClipMaxNodes;
    for (uint32_t k = t; k < n_skins; k += kBlendBlock) {
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
        for (uint32_t e = t; e < h.n_joints * 3; e += kBlendBlock) {       // a lane a 16-byte piece: consecutive lanes, consecutive stores
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
    // 6. instance transforms: a lane a piece
    if (instance_transforms) {
        const uint32_t* __restrict__ inst = (const uint32_t*)(blk + h.instances);
        for (uint32_t e = t; e < h.n_instances * 3; e += kBlendBlock) {
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

constexpr uint32_t kBlendWeightsBlock = 256, kBlendWave = 64;

// The two key rows a set's weights come from and the fraction between them: keys i and i + 1 (or i twice) of the channel, or the
// defaults twice. Wave-uniform: scalar loads and scalar arithmetic.
struct BlendKeyRows { const float* a; const float* b; double u; uint32_t n_targets; };
__device__ __forceinline__ BlendKeyRows blend_key_rows(const unsigned char* __restrict__ blk, uint32_t set_at, float time_seconds) {
    const ClipMorphHeader mh = *(const ClipMorphHeader*)(blk + ((const ClipHeader*)blk)->reserved);
    const ClipMorphSet set = ((const ClipMorphSet*)(blk + mh.sets))[set_at];
    BlendKeyRows r;
    r.a = (const float*)(blk + mh.defaults) + set.first_default;
    r.b = r.a; r.u = 0.0; r.n_targets = set.n_targets;
    if (set.n_keys) {
        uint32_t i = 0;
        clip_key_search((const float*)(blk + mh.times) + set.first_time, set.n_keys, set.interpolation, (double)time_seconds, &i, &r.u);
        const float* values = (const float*)(blk + mh.values) + set.first_value;
        r.a = values + (size_t)i * set.n_targets;
        r.b = values + (size_t)(r.u > 0.0 ? i + 1 : i) * set.n_targets;
    }
    return r;
}

// One wave per row, no LDS, no barrier, as clip_weights_kernel: the row index is made uniform; the lanes run over the targets in
// chunks of 64, and the ballot of a chunk orders its survivors.
__global__ void __launch_bounds__(kBlendWeightsBlock) clip_blend_weights_kernel(const ClipBlendWeightRow* __restrict__ rows, uint32_t n_rows,
                                                                                PoseBatchItem* __restrict__ items, uint32_t* __restrict__ active_index,
                                                                                float* __restrict__ active_weight, uint32_t* __restrict__ check) {
    const uint32_t lane = threadIdx.x % kBlendWave;
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kBlendWeightsBlock / kBlendWave) + threadIdx.x / kBlendWave);
    if (r >= n_rows) return;
    const ClipBlendWeightRow row = rows[r];
    const BlendKeyRows ka = blend_key_rows((const unsigned char*)row.clip_a, row.set_a, row.time_a);
    const BlendKeyRows kb = blend_key_rows((const unsigned char*)row.clip_b, row.set_b, row.time_b);
    const uint32_t n_targets = ka.n_targets < kb.n_targets ? ka.n_targets : kb.n_targets;      // equal, the host has checked; never past either set
    const double weight = (double)row.weight;
    uint32_t* __restrict__ out_index = active_index + row.active_base;
    float* __restrict__ out_weight = active_weight + row.active_base;
    uint32_t count = 0;
    for (uint32_t k0 = 0; k0 < n_targets; k0 += kBlendWave) {
        const uint32_t k = k0 + lane;
        const float w = k < n_targets ? clip_blend_weight(clip_weight(ka.a[k], ka.b[k], ka.u), clip_weight(kb.a[k], kb.b[k], kb.u), weight) : 0.0f;
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

int srk_clip_blend(const srd::ClipBlendActorRow* actors, uint32_t n_actors, const uint32_t* rows, SrTransform* matrices, SrTransform* instance_transforms,
                   uint32_t* check, SrNodeTrs* keep_trs, float* keep_globals, SrNodeTrs* keep_a, SrNodeTrs* keep_b, hipStream_t stream) {
    if (n_actors == 0) return 0;
    srd::clip_blend_kernel<<<dim3(n_actors), dim3(srd::kBlendBlock), 0, stream>>>(actors, rows, (float4*)matrices, (float4*)instance_transforms, check,
                                                                                 (uint4*)keep_trs, (float4*)keep_globals, (uint4*)keep_a, (uint4*)keep_b);
    return (int)hipGetLastError();
}

int srk_clip_blend_weights(const srd::ClipBlendWeightRow* rows, uint32_t n_rows, srd::PoseBatchItem* items, uint32_t* active_index, float* active_weight,
                           uint32_t* check, hipStream_t stream) {
    if (n_rows == 0) return 0;
    const uint32_t per_block = srd::kBlendWeightsBlock / srd::kBlendWave;
    srd::clip_blend_weights_kernel<<<dim3((n_rows + per_block - 1) / per_block), dim3(srd::kBlendWeightsBlock), 0, stream>>>(rows, n_rows, items, active_index,
                                                                                                                             active_weight, check);
    return (int)hipGetLastError();
}
