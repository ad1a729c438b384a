// Morph-target (blend shape) evaluation of a mesh's base vertices (sr_scene_pose_mesh, include/sunray_hip.h states the arithmetic
// to the letter). fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "morph.h"

#include "vertex_tile.h"

namespace srd {

// One vertex per thread on the tile of vertex_tile.h. A delta record is the first three pieces of a vertex and nothing else, so a
// thread reads its own record of every active target straight from global memory: three dwordx4 whose 48 bytes join those of
// the neighbouring lanes into whole cache lines, each byte fetched once. The active list is read at wave-uniform addresses:
// count, index and weight live in scalar registers.
constexpr uint32_t kMorphDeltaPieces = sizeof(SrMorphDelta) / 16;
static_assert(sizeof(SrMorphDelta) == 48 && offsetof(SrMorphDelta, position) == 0 && offsetof(SrMorphDelta, normal) == 16 && offsetof(SrMorphDelta, tangent) == 32,
              "morph_kernel: a delta record is three 16-byte pieces laid out like the first three of a vertex");

__global__ void __launch_bounds__(kTileBlock) morph_kernel(const uint4* __restrict__ base, const float4* __restrict__ deltas,
                                                            const uint32_t* __restrict__ active_index, const float* __restrict__ active_weight,
                                                            uint32_t n_active, uint4* __restrict__ out, uint32_t n_vertices, uint32_t* first_bad) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const VertexTile vt(n_vertices);
    const uint32_t t = threadIdx.x, v0 = vt.v0, nv = vt.nv;
    vt.load(tile, base);
    uint32_t bad = 0xFFFFFFFFu;
    if (t < nv) {
        float s[3][3];
#pragma unroll
        for (int c = 0; c < 3; c++) { s[c][0] = 0.0f; s[c][1] = 0.0f; s[c][2] = 0.0f; }
        for (uint32_t a = 0; a < n_active; a++) {
            const float w = active_weight[a];
            // 64-bit: n_targets * n_vertices * 3 pieces need not fit 32
            const float4* d = deltas + ((uint64_t)active_index[a] * n_vertices + (v0 + t)) * kMorphDeltaPieces;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float4 q = d[c];
                s[c][0] = s[c][0] + w * q.x; s[c][1] = s[c][1] + w * q.y; s[c][2] = s[c][2] + w * q.z;
            }
        }
        uint4* row = VertexTile::row(tile, t);
        const uint4 P = row[0], N = row[1], T = row[2];
        float px = __uint_as_float(P.x), py = __uint_as_float(P.y), pz = __uint_as_float(P.z);
        if (!(s[0][0] == 0.0f && s[0][1] == 0.0f && s[0][2] == 0.0f)) {     // a sum of ±0 keeps the base's bytes (b + 0 would turn -0 into +0)
            px = px + s[0][0]; py = py + s[0][1]; pz = pz + s[0][2];
            row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
        }
        if (!(finite_bits(px) && finite_bits(py) && finite_bits(pz))) bad = v0 + t;
        if (!(s[1][0] == 0.0f && s[1][1] == 0.0f && s[1][2] == 0.0f))
            store_normalised(row + 1, __uint_as_float(N.x) + s[1][0], __uint_as_float(N.y) + s[1][1], __uint_as_float(N.z) + s[1][2]);
        if (!(s[2][0] == 0.0f && s[2][1] == 0.0f && s[2][2] == 0.0f))
            store_normalised(row + 2, __uint_as_float(T.x) + s[2][0], __uint_as_float(T.y) + s[2][1], __uint_as_float(T.z) + s[2][2]);
    }
    vt.store(tile, out);
    report_first_bad(bad, first_bad);
}

}  // namespace srd

int srk_morph(const SrVertex* base, const SrMorphDelta* deltas, const uint32_t* active_index, const float* active_weight, uint32_t n_active,
              SrVertex* out, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kTileBlock - 1) / srd::kTileBlock);
    srd::morph_kernel<<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)base, (const float4*)deltas, active_index, active_weight, n_active,
                                                                         (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
