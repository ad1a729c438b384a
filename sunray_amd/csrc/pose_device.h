// The per-vertex arithmetic of posing on the device, defined once: pose_batch_kernel (pose_batch.hip), the one
// posing kernel, calls these bodies on a thread's own row of the tile of vertex_tile.h. include/sunray_hip.h
// states the arithmetic to the letter (sr_scene_skin_mesh, sr_scene_pose_mesh). fp32 under the numerics contract of DESIGN.md §3:
// no contraction, correctly rounded divide and sqrt, left to right.
#pragma once
#include "vertex_tile.h"

namespace srd {

// A delta record is the first three pieces of a vertex and nothing else, so a thread reads its own record of every active target
// straight from global memory: three dwordx4 whose 48 bytes join those of the neighbouring lanes into whole cache lines, each
// byte fetched once.
constexpr uint32_t kMorphDeltaPieces = sizeof(SrMorphDelta) / 16;
static_assert(sizeof(SrMorphDelta) == 48 && offsetof(SrMorphDelta, position) == 0 && offsetof(SrMorphDelta, normal) == 16 && offsetof(SrMorphDelta, tangent) == 32,
              "morph_vertex: a delta record is three 16-byte pieces laid out like the first three of a vertex");
static_assert(sizeof(SrSkinInfluence) == 24 && offsetof(SrSkinInfluence, weight) == 8 && sizeof(SrTransform) == 48,
              "skin_vertex: an influence is three 8-byte pieces, a joint matrix three rows of 16 bytes");

// The morph stage of vertex `v` of a mesh of `n_vertices` on its row of the tile (position, normal, tangent: row[0..2], rewritten
// in place). The active list is read at wave-uniform addresses: count, index and weight live in scalar registers. Whether the
// morphed position is finite.
__device__ __forceinline__ bool morph_vertex(uint4* row, const float4* __restrict__ deltas, const uint32_t* __restrict__ active_index,
                                             const float* __restrict__ active_weight, uint32_t n_active, uint32_t n_vertices, uint32_t v) {
    float s[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) { s[c][0] = 0.0f; s[c][1] = 0.0f; s[c][2] = 0.0f; }
    for (uint32_t a = 0; a < n_active; a++) {
        const float w = active_weight[a];
        // 64-bit: n_targets * n_vertices * 3 pieces need not fit 32
        const float4* d = deltas + ((uint64_t)active_index[a] * n_vertices + v) * kMorphDeltaPieces;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float4 q = d[c];
            s[c][0] = s[c][0] + w * q.x; s[c][1] = s[c][1] + w * q.y; s[c][2] = s[c][2] + w * q.z;
        }
    }
    const uint4 P = row[0], N = row[1], T = row[2];
    float px = __uint_as_float(P.x), py = __uint_as_float(P.y), pz = __uint_as_float(P.z);
    if (!(s[0][0] == 0.0f && s[0][1] == 0.0f && s[0][2] == 0.0f)) {     // a sum of ±0 keeps the base's bytes (b + 0 would turn -0 into +0)
        px = px + s[0][0]; py = py + s[0][1]; pz = pz + s[0][2];
        row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
    }
    if (!(s[1][0] == 0.0f && s[1][1] == 0.0f && s[1][2] == 0.0f))
        store_normalised(row + 1, __uint_as_float(N.x) + s[1][0], __uint_as_float(N.y) + s[1][1], __uint_as_float(N.z) + s[1][2]);
    if (!(s[2][0] == 0.0f && s[2][1] == 0.0f && s[2][2] == 0.0f))
        store_normalised(row + 2, __uint_as_float(T.x) + s[2][0], __uint_as_float(T.y) + s[2][1], __uint_as_float(T.z) + s[2][2]);
    return finite_bits(px) && finite_bits(py) && finite_bits(pz);
}

// The skin stage of a vertex on its row of the tile, with the vertex's own influence record `inf` (three 8-byte pieces). The joint
// matrices are gathered from global memory (three dwordx4 per non-zero weight): a rig is a few KiB that the vector L1 and the L2
// hold, and a rig of 65536 joints would fit no LDS. Whether the posed position is finite.
__device__ __forceinline__ bool skin_vertex(uint4* row, const uint2* __restrict__ inf, const float4* __restrict__ matrices) {
    const uint2 j = inf[0], wa = inf[1], wb = inf[2];
    const uint32_t joint[4] = {j.x & 0xFFFFu, j.x >> 16, j.y & 0xFFFFu, j.y >> 16};
    const float weight[4] = {__uint_as_float(wa.x), __uint_as_float(wa.y), __uint_as_float(wb.x), __uint_as_float(wb.y)};
    float B[3][4];
#pragma unroll
    for (int r = 0; r < 3; r++) { B[r][0] = 0.0f; B[r][1] = 0.0f; B[r][2] = 0.0f; B[r][3] = 0.0f; }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (weight[k] != 0.0f) {            // a weight of 0 never reads its matrix: neither a NaN in it nor an index past the rig counts
            const float w = weight[k];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const float4 m = matrices[(size_t)joint[k] * 3 + r];
                B[r][0] = B[r][0] + w * m.x; B[r][1] = B[r][1] + w * m.y; B[r][2] = B[r][2] + w * m.z; B[r][3] = B[r][3] + w * m.w;
            }
        }
    }
    const uint4 P = row[0], N = row[1], T = row[2];
    const float x = __uint_as_float(P.x), y = __uint_as_float(P.y), z = __uint_as_float(P.z);
    const float px = ((B[0][0] * x + B[0][1] * y) + B[0][2] * z) + B[0][3];
    const float py = ((B[1][0] * x + B[1][1] * y) + B[1][2] * z) + B[1][3];
    const float pz = ((B[2][0] * x + B[2][1] * y) + B[2][2] * z) + B[2][3];
    row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
    // rows of the cofactor matrix of B's 3x3 part: a1 x a2, a2 x a0, a0 x a1
    const float c00 = B[1][1] * B[2][2] - B[1][2] * B[2][1], c01 = B[1][2] * B[2][0] - B[1][0] * B[2][2], c02 = B[1][0] * B[2][1] - B[1][1] * B[2][0];
    const float c10 = B[2][1] * B[0][2] - B[2][2] * B[0][1], c11 = B[2][2] * B[0][0] - B[2][0] * B[0][2], c12 = B[2][0] * B[0][1] - B[2][1] * B[0][0];
    const float c20 = B[0][1] * B[1][2] - B[0][2] * B[1][1], c21 = B[0][2] * B[1][0] - B[0][0] * B[1][2], c22 = B[0][0] * B[1][1] - B[0][1] * B[1][0];
    const float nx = __uint_as_float(N.x), ny = __uint_as_float(N.y), nz = __uint_as_float(N.z);
    store_normalised(row + 1, (c00 * nx + c01 * ny) + c02 * nz, (c10 * nx + c11 * ny) + c12 * nz, (c20 * nx + c21 * ny) + c22 * nz);
    const float tx = __uint_as_float(T.x), ty = __uint_as_float(T.y), tz = __uint_as_float(T.z);
    store_normalised(row + 2, (B[0][0] * tx + B[0][1] * ty) + B[0][2] * tz, (B[1][0] * tx + B[1][1] * ty) + B[1][2] * tz,
                     (B[2][0] * tx + B[2][1] * ty) + B[2][2] * tz);
    return finite_bits(px) && finite_bits(py) && finite_bits(pz);
}

}  // namespace srd
