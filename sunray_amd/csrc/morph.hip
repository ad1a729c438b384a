// Morph-target (blend shape) evaluation of a mesh's base vertices (sr_scene_pose_mesh, include/sunray_hip.h states the arithmetic
// to the letter). fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "morph.h"

#include <cstddef>

namespace srd {

// The layout of skin_kernel: one block blends a tile of 256 vertices, one vertex per thread. The base records cross global memory
// as 16-byte pieces, six per vertex, consecutive lanes on consecutive pieces (coalesced dwordx4), and are turned by the LDS: a
// thread reads the three pieces of its own vertex that morphing changes (position, normal, tangent), writes them back in place,
// and the tile leaves as it came. The uv sets and the pads are never in a register of the blending thread: every byte that is not
// rewritten is the base's. A row of the tile is seven pieces, not six, for the reason given there (lanes 28 dwords apart fall on
// sixteen different 16-byte slots in every group of 16 lanes that one ds_read_b128 serves). 28 KiB per block: five blocks a CU.
// A delta record is the first three pieces of a vertex and nothing else, so a thread reads its own record of every active target
// straight from global memory: three dwordx4 whose 48 bytes join those of the neighbouring lanes into whole cache lines, each
// byte fetched once. The active list is read at wave-uniform addresses: count, index and weight live in scalar registers.
constexpr uint32_t kMorphBlock = 256, kMorphPieces = sizeof(SrVertex) / 16, kMorphRow = kMorphPieces + 1, kMorphDeltaPieces = sizeof(SrMorphDelta) / 16;
static_assert(sizeof(SrVertex) == 96 && offsetof(SrVertex, position) == 0 && offsetof(SrVertex, normal) == 16 && offsetof(SrVertex, tangent) == 32,
              "morph_kernel: position, normal and tangent are the first three 16-byte pieces of a vertex");
static_assert(sizeof(SrMorphDelta) == 48 && offsetof(SrMorphDelta, position) == 0 && offsetof(SrMorphDelta, normal) == 16 && offsetof(SrMorphDelta, tangent) == 32,
              "morph_kernel: a delta record is three 16-byte pieces laid out like the first three of a vertex");

__device__ __forceinline__ bool morph_finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// v * (1 / sqrt(dot(v, v))) into the first three words of *piece; a squared length that is 0 or not finite leaves the piece alone
__device__ __forceinline__ void morph_store_normalised(uint4* piece, float x, float y, float z) {
    const float len2 = (x * x + y * y) + z * z;
    if (len2 == 0.0f || !morph_finite_bits(len2)) return;
    const float r = 1.0f / sqrtf(len2);
    piece->x = __float_as_uint(x * r); piece->y = __float_as_uint(y * r); piece->z = __float_as_uint(z * r);
}

__global__ void __launch_bounds__(kMorphBlock) morph_kernel(const uint4* __restrict__ base, const float4* __restrict__ deltas,
                                                            const uint32_t* __restrict__ active_index, const float* __restrict__ active_weight,
                                                            uint32_t n_active, uint4* __restrict__ out, uint32_t n_vertices, uint32_t* first_bad) {
    __shared__ uint4 tile[kMorphBlock * kMorphRow];
    const uint32_t t = threadIdx.x, v0 = blockIdx.x * kMorphBlock;      // v0 < n_vertices: the grid is ceil(n_vertices / 256)
    const uint32_t nv = min(kMorphBlock, n_vertices - v0), np = nv * kMorphPieces;
    const uint64_t p0 = (uint64_t)v0 * kMorphPieces;                    // piece indices are 64-bit (n_vertices * 6 need not fit 32)
#pragma unroll
    for (uint32_t k = 0; k < kMorphPieces; k++) {
        const uint32_t p = k * kMorphBlock + t;
        if (p < np) tile[p + p / kMorphPieces] = base[p0 + p];
    }
    __syncthreads();
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
        uint4* row = tile + t * kMorphRow;
        const uint4 P = row[0], N = row[1], T = row[2];
        float px = __uint_as_float(P.x), py = __uint_as_float(P.y), pz = __uint_as_float(P.z);
        if (!(s[0][0] == 0.0f && s[0][1] == 0.0f && s[0][2] == 0.0f)) {     // a sum of ±0 keeps the base's bytes (b + 0 would turn -0 into +0)
            px = px + s[0][0]; py = py + s[0][1]; pz = pz + s[0][2];
            row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
        }
        if (!(morph_finite_bits(px) && morph_finite_bits(py) && morph_finite_bits(pz))) bad = v0 + t;
        if (!(s[1][0] == 0.0f && s[1][1] == 0.0f && s[1][2] == 0.0f))
            morph_store_normalised(row + 1, __uint_as_float(N.x) + s[1][0], __uint_as_float(N.y) + s[1][1], __uint_as_float(N.z) + s[1][2]);
        if (!(s[2][0] == 0.0f && s[2][1] == 0.0f && s[2][2] == 0.0f))
            morph_store_normalised(row + 2, __uint_as_float(T.x) + s[2][0], __uint_as_float(T.y) + s[2][1], __uint_as_float(T.z) + s[2][2]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kMorphPieces; k++) {
        const uint32_t p = k * kMorphBlock + t;
        if (p < np) out[p0 + p] = tile[p + p / kMorphPieces];
    }
    // the lowest offending vertex: one reduction per wave (cross-lane moves), at most one atomicMin per wave
    for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o, 64));
    if ((t & 63u) == 0 && bad != 0xFFFFFFFFu) atomicMin(first_bad, bad);
}

}  // namespace srd

int srk_morph(const SrVertex* base, const SrMorphDelta* deltas, const uint32_t* active_index, const float* active_weight, uint32_t n_active,
              SrVertex* out, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kMorphBlock - 1) / srd::kMorphBlock);
    srd::morph_kernel<<<dim3(blocks), dim3(srd::kMorphBlock), 0, stream>>>((const uint4*)base, (const float4*)deltas, active_index, active_weight, n_active,
                                                                         (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
