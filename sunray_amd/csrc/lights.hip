// The light table of a frame on the device (sr_scene_set_light_table_build, include/sunray_hip.h): srh::light_table
// (host_prep.cpp) restated operation for operation, and the arena positions of a mesh whose newest vertices are on the device.
// fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide and sqrt, left to right.
#include "lights.h"

#include <cstddef>

namespace srd {

constexpr uint32_t kLightBlock = 256, kLightRows = 4;     // a DevLight is four 16-byte rows
static_assert(sizeof(SrEmissiveTriangle) == 64 && offsetof(SrEmissiveTriangle, v1) == 16 && offsetof(SrEmissiveTriangle, v2) == 32 &&
              offsetof(SrEmissiveTriangle, emission) == 48, "light_table_kernel: an arena record is four rows of 16 bytes");
static_assert(sizeof(SrEmissiveIndirectionEntry) == 8 && sizeof(FlatInstance) == 64 && offsetof(FlatInstance, o2w) == 0,
              "light_table_kernel: an entry is 8 bytes, ObjectToWorld the first three rows of an instance record");
static_assert(sizeof(SrVertex) == 96 && offsetof(SrVertex, position) == 0, "emissive_positions_kernel: the position opens a vertex");

// transform_point (rt_utils.slang:278-281), the operation order of srh::light_table
__device__ __forceinline__ void to_world(const float4 m0, const float4 m1, const float4 m2, const float4 v, float w[3]) {
    w[0] = ((m0.x * v.x + m0.y * v.y) + m0.z * v.z) + m0.w * 1.0f;
    w[1] = ((m1.x * v.x + m1.y * v.y) + m1.z * v.z) + m1.w * 1.0f;
    w[2] = ((m2.x * v.x + m2.y * v.y) + m2.z * v.z) + m2.w * 1.0f;
}

// Four lanes per light: lane 4i + r computes light i whole and stores its row r, so a wave's store instruction writes 1024
// contiguous bytes (consecutive lanes on consecutive 16-byte pieces) and nothing is exchanged between lanes. The kernel is
// memory-bound (8 + 64 + 48 bytes in, 64 out per light); the four lanes of a light read the same 8 + 64 + 48 bytes in the same
// instruction, which the memory pipeline serves as one access per distinct address, and the arithmetic (about 60 operations,
// one sqrt, one divide) is repeated four times in lanes that would otherwise idle behind the stores.
__global__ void __launch_bounds__(kLightBlock) light_table_kernel(const uint2* __restrict__ entries, uint32_t n_entries, const float4* __restrict__ arena,
                                                                  uint32_t n_arena, const float4* __restrict__ instances, uint32_t n_instances,
                                                                  float4* __restrict__ lights) {
    const uint64_t piece = (uint64_t)blockIdx.x * kLightBlock + threadIdx.x;      // 64-bit: four pieces per light need not fit 32
    const uint64_t i = piece / kLightRows;
    if (i >= n_entries) return;
    const uint32_t row = (uint32_t)(piece % kLightRows);
    const uint2 e = entries[i];                                                  // x: arena slot, y: instance
    if (e.x >= n_arena || e.y >= n_instances) return;
    const float4* t = arena + (size_t)e.x * 4;
    const float4* m = instances + (size_t)e.y * 4;
    const float4 v0 = t[0], v1 = t[1], v2 = t[2], em = t[3];
    const float4 m0 = m[0], m1 = m[1], m2 = m[2];
    float w0[3], w1[3], w2[3];
    to_world(m0, m1, m2, v0, w0);
    to_world(m0, m1, m2, v1, w1);
    to_world(m0, m1, m2, v2, w2);
    const float e1[3] = {w1[0] - w0[0], w1[1] - w0[1], w1[2] - w0[2]};
    const float e2[3] = {w2[0] - w0[0], w2[1] - w0[1], w2[2] - w0[2]};
    const float c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float dd = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    const float len = sqrtf(dd);
    const float r = 1.0f / len;
    float4 q;                                                                    // DevLight (traverse.h): wv0 area | wv1 nx | wv2 ny | emission nz
    if (row == 0) q = make_float4(w0[0], w0[1], w0[2], 0.5f * len);
    else if (row == 1) q = make_float4(w1[0], w1[1], w1[2], c[0] * r);
    else if (row == 2) q = make_float4(w2[0], w2[1], w2[2], c[1] * r);
    else q = make_float4(em.x, em.y, em.z, c[2] * r);
    lights[piece] = q;
}

// One thread per triangle: three indices (12 contiguous bytes per lane), three positions gathered from 96-byte vertex records,
// three 12-byte stores into the 64-byte arena record of the triangle's slot. The gather sets the pace (a mesh's slots are
// consecutive unless freed slots were reused); the fourth word of each row and the emission row keep what the host uploaded.
__global__ void __launch_bounds__(kLightBlock) emissive_positions_kernel(const float* __restrict__ vertices, uint32_t n_vertices,
                                                                         const uint32_t* __restrict__ indices, const uint32_t* __restrict__ slots,
                                                                         uint32_t n_tris, float* __restrict__ arena, uint32_t n_arena) {
    const uint64_t k = (uint64_t)blockIdx.x * kLightBlock + threadIdx.x;
    if (k >= n_tris) return;
    const uint32_t slot = slots[k];
    const uint32_t i0 = indices[3 * k], i1 = indices[3 * k + 1], i2 = indices[3 * k + 2];
    if (slot >= n_arena || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) return;
    const uint32_t idx[3] = {i0, i1, i2};
    float* t = arena + (size_t)slot * 16;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float* p = vertices + (size_t)idx[j] * 24;
        const float x = p[0], y = p[1], z = p[2];
        t[4 * j] = x; t[4 * j + 1] = y; t[4 * j + 2] = z;
    }
}

}  // namespace srd

int srk_light_table(const SrEmissiveIndirectionEntry* entries, uint32_t n_entries, const SrEmissiveTriangle* arena, uint32_t n_arena,
                    const srd::FlatInstance* instances, uint32_t n_instances, float* lights, hipStream_t stream) {
    if (n_entries == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_entries * srd::kLightRows + srd::kLightBlock - 1) / srd::kLightBlock);
    srd::light_table_kernel<<<dim3(blocks), dim3(srd::kLightBlock), 0, stream>>>((const uint2*)entries, n_entries, (const float4*)arena, n_arena,
                                                                              (const float4*)instances, n_instances, (float4*)lights);
    return (int)hipGetLastError();
}

int srk_emissive_positions(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, const uint32_t* slots, uint32_t n_tris,
                           SrEmissiveTriangle* arena, uint32_t n_arena, hipStream_t stream) {
    if (n_tris == 0) return 0;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_tris + srd::kLightBlock - 1) / srd::kLightBlock);
    srd::emissive_positions_kernel<<<dim3(blocks), dim3(srd::kLightBlock), 0, stream>>>((const float*)vertices, n_vertices, indices, slots, n_tris,
                                                                                     (float*)arena, n_arena);
    return (int)hipGetLastError();
}
