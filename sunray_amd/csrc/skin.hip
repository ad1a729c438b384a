// Linear-blend skinning of a mesh's bind pose (sr_scene_skin_mesh, include/sunray_hip.h states the arithmetic to the letter).
// fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "skin.h"

#include "vertex_tile.h"

namespace srd {

// One vertex per thread on the tile of vertex_tile.h (96 + 24 bytes in, 96 out per vertex). The joint matrices are gathered from
// global memory (three dwordx4 per non-zero weight): a rig is a few KiB that the vector L1 and the L2 hold, and a rig of 65536
// joints would fit no LDS.
static_assert(sizeof(SrSkinInfluence) == 24 && offsetof(SrSkinInfluence, weight) == 8 && sizeof(SrTransform) == 48,
              "skin_kernel: an influence is three 8-byte pieces, a joint matrix three rows of 16 bytes");

__global__ void __launch_bounds__(kTileBlock) skin_kernel(const uint4* __restrict__ bind, const uint2* __restrict__ influences,
                                                          const float4* __restrict__ matrices, uint4* __restrict__ out, uint32_t n_vertices,
                                                          uint32_t* first_bad) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const VertexTile vt(n_vertices);
    const uint32_t t = threadIdx.x, v0 = vt.v0, nv = vt.nv;
    vt.load(tile, bind);
    uint32_t bad = 0xFFFFFFFFu;
    if (t < nv) {
        const uint2* inf = influences + (size_t)(v0 + t) * 3;
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
        uint4* row = VertexTile::row(tile, t);
        const uint4 P = row[0], N = row[1], T = row[2];
        const float x = __uint_as_float(P.x), y = __uint_as_float(P.y), z = __uint_as_float(P.z);
        const float px = ((B[0][0] * x + B[0][1] * y) + B[0][2] * z) + B[0][3];
        const float py = ((B[1][0] * x + B[1][1] * y) + B[1][2] * z) + B[1][3];
        const float pz = ((B[2][0] * x + B[2][1] * y) + B[2][2] * z) + B[2][3];
        row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
        if (!(finite_bits(px) && finite_bits(py) && finite_bits(pz))) bad = v0 + t;
        // rows of the cofactor matrix of B's 3x3 part: a1 x a2, a2 x a0, a0 x a1
        const float c00 = B[1][1] * B[2][2] - B[1][2] * B[2][1], c01 = B[1][2] * B[2][0] - B[1][0] * B[2][2], c02 = B[1][0] * B[2][1] - B[1][1] * B[2][0];
        const float c10 = B[2][1] * B[0][2] - B[2][2] * B[0][1], c11 = B[2][2] * B[0][0] - B[2][0] * B[0][2], c12 = B[2][0] * B[0][1] - B[2][1] * B[0][0];
        const float c20 = B[0][1] * B[1][2] - B[0][2] * B[1][1], c21 = B[0][2] * B[1][0] - B[0][0] * B[1][2], c22 = B[0][0] * B[1][1] - B[0][1] * B[1][0];
        const float nx = __uint_as_float(N.x), ny = __uint_as_float(N.y), nz = __uint_as_float(N.z);
        store_normalised(row + 1, (c00 * nx + c01 * ny) + c02 * nz, (c10 * nx + c11 * ny) + c12 * nz, (c20 * nx + c21 * ny) + c22 * nz);
        const float tx = __uint_as_float(T.x), ty = __uint_as_float(T.y), tz = __uint_as_float(T.z);
        store_normalised(row + 2, (B[0][0] * tx + B[0][1] * ty) + B[0][2] * tz, (B[1][0] * tx + B[1][1] * ty) + B[1][2] * tz,
                         (B[2][0] * tx + B[2][1] * ty) + B[2][2] * tz);
    }
    vt.store(tile, out);
    report_first_bad(bad, first_bad);
}

}  // namespace srd

int srk_skin(const SrVertex* bind, const SrSkinInfluence* influences, const SrTransform* joint_matrices, SrVertex* out,
             uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kTileBlock - 1) / srd::kTileBlock);
    srd::skin_kernel<<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)bind, (const uint2*)influences, (const float4*)joint_matrices,
                                                                       (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
