// Linear-blend skinning of a mesh's bind pose (sr_scene_skin_mesh, include/sunray_hip.h states the arithmetic to the letter).
// fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "skin.h"

#include <cstddef>

namespace srd {

// One block poses a tile of 256 vertices, one vertex per thread. The kernel is memory-bound (96 + 24 bytes in, 96 out per
// vertex), so the records cross global memory as 16-byte pieces, six per vertex, consecutive lanes on consecutive pieces
// (coalesced dwordx4, the walk of vertex_check_kernel), and are turned by the LDS: a thread reads the three pieces of its own
// vertex that skinning changes (position, normal, tangent), writes them back in place, and the tile leaves as it came. The uv
// sets and the pads are never in a register of the posing thread: every byte that is not rewritten is the bind pose's. A row of
// the tile is seven pieces, not six: lanes 28 dwords apart fall on sixteen different 16-byte slots of the LDS in every group
// of 16 lanes that one ds_read_b128 serves (24 dwords apart they would share slots in pairs). 28 KiB per block: five blocks a CU.
// The joint matrices are gathered from global memory (three dwordx4 per non-zero weight): a rig is a few KiB that the
// vector L1 and the L2 hold, and a rig of 65536 joints would fit no LDS.
constexpr uint32_t kSkinBlock = 256, kSkinPieces = sizeof(SrVertex) / 16, kSkinRow = kSkinPieces + 1;
static_assert(sizeof(SrVertex) == 96 && offsetof(SrVertex, position) == 0 && offsetof(SrVertex, normal) == 16 && offsetof(SrVertex, tangent) == 32,
              "skin_kernel: position, normal and tangent are the first three 16-byte pieces of a vertex");
static_assert(sizeof(SrSkinInfluence) == 24 && offsetof(SrSkinInfluence, weight) == 8 && sizeof(SrTransform) == 48,
              "skin_kernel: an influence is three 8-byte pieces, a joint matrix three rows of 16 bytes");

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// v * (1 / sqrt(dot(v, v))) into the first three words of *piece; a squared length that is 0 or not finite leaves the piece alone
__device__ __forceinline__ void store_normalised(uint4* piece, float x, float y, float z) {
    const float len2 = (x * x + y * y) + z * z;
    if (len2 == 0.0f || !finite_bits(len2)) return;
    const float r = 1.0f / sqrtf(len2);
    piece->x = __float_as_uint(x * r); piece->y = __float_as_uint(y * r); piece->z = __float_as_uint(z * r);
}

__global__ void __launch_bounds__(kSkinBlock) skin_kernel(const uint4* __restrict__ bind, const uint2* __restrict__ influences,
                                                          const float4* __restrict__ matrices, uint4* __restrict__ out, uint32_t n_vertices,
                                                          uint32_t* first_bad) {
    __shared__ uint4 tile[kSkinBlock * kSkinRow];
    const uint32_t t = threadIdx.x, v0 = blockIdx.x * kSkinBlock;        // v0 < n_vertices: the grid is ceil(n_vertices / 256)
    const uint32_t nv = min(kSkinBlock, n_vertices - v0), np = nv * kSkinPieces;
    const uint64_t p0 = (uint64_t)v0 * kSkinPieces;                      // piece indices are 64-bit (n_vertices * 6 need not fit 32)
#pragma unroll
    for (uint32_t k = 0; k < kSkinPieces; k++) {
        const uint32_t p = k * kSkinBlock + t;
        if (p < np) tile[p + p / kSkinPieces] = bind[p0 + p];
    }
    __syncthreads();
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
        uint4* row = tile + t * kSkinRow;
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
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kSkinPieces; k++) {
        const uint32_t p = k * kSkinBlock + t;
        if (p < np) out[p0 + p] = tile[p + p / kSkinPieces];
    }
    // the lowest offending vertex: one reduction per wave (cross-lane moves), at most one atomicMin per wave
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o, 64));
    if ((t & 63u) == 0 && bad != 0xFFFFFFFFu) atomicMin(first_bad, bad);
}

}  // namespace srd

int srk_skin(const SrVertex* bind, const SrSkinInfluence* influences, const SrTransform* joint_matrices, SrVertex* out,
             uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kSkinBlock - 1) / srd::kSkinBlock);
    srd::skin_kernel<<<dim3(blocks), dim3(srd::kSkinBlock), 0, stream>>>((const uint4*)bind, (const uint2*)influences, (const float4*)joint_matrices,
                                                                       (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
