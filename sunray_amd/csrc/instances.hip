// The per-instance tables of a frame on the device (sr_scene_set_instances_device, include/sunray_hip.h): what
// upload_instance_tables (api.cpp) fills on the host, from transforms that are already in device memory, with the host call's
// finite check fused in. fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly rounded divide, the
// operation order of srh::world_to_object_3x3 (host_prep.cpp).
#include "instances.h"

#include <cstddef>

#include "vertex_tile.h"

namespace srd {

// One block per tile of 256 instances, one instance per thread. The kernel is memory-bound (48 bytes in, 96 + 64 out per
// instance), so every record crosses global memory as 16-byte pieces, consecutive lanes on consecutive pieces, and is turned by
// the LDS as vertex_tile.h turns vertices. The transforms come in three pieces per instance and stay packed: lanes 12 dwords
// apart fall on sixteen different 16-byte slots in every group of 16 lanes one ds_read_b128 serves (3 is odd). A DevInstance
// leaves as six pieces from rows of seven (28 dwords apart, the row of vertex_tile.h). A FlatInstance needs no tile of its own:
// its first three pieces are the transform's, still in the input tile, and the fourth is the instance's layout entry.
// 12 + 28 KiB of LDS per block: four blocks a CU.
constexpr uint32_t kInstBlock = 256, kXformPieces = 3, kDevPieces = 6, kDevRow = kDevPieces + 1, kFlatPieces = 4;
static_assert(sizeof(SrTransform) == 48 && sizeof(DevInstance) == 96 && offsetof(DevInstance, o2w) == 48 && sizeof(FlatInstance) == 64 &&
              offsetof(FlatInstance, o2w) == 0 && offsetof(FlatInstance, tri_offset) == 48 && offsetof(FlatInstance, mesh_slot) == 52 &&
              sizeof(InstanceLayout) == 8, "instance_tables_kernel: 3 pieces in, 6 + 4 out, the layout words open the fourth piece of a FlatInstance");

__global__ void __launch_bounds__(kInstBlock) instance_tables_kernel(const uint4* __restrict__ transforms, const uint2* __restrict__ layout, uint32_t n,
                                                                     uint4* __restrict__ dev, uint4* __restrict__ flat, uint32_t* first_bad) {
    __shared__ uint4 in_tile[kInstBlock * kXformPieces];
    __shared__ uint4 dev_tile[kInstBlock * kDevRow];
    const uint32_t t = threadIdx.x;
    const uint32_t i0 = blockIdx.x * kInstBlock;                  // < n
    const uint32_t ni = min(kInstBlock, n - i0);
    {
        const uint4* __restrict__ from = transforms + (uint64_t)i0 * kXformPieces;     // 64-bit: n * 3 need not fit 32
#pragma unroll
        for (uint32_t k = 0; k < kXformPieces; k++) {
            const uint32_t p = k * kInstBlock + t;
            if (p < ni * kXformPieces) in_tile[p] = from[p];
        }
    }
    __syncthreads();
    uint32_t bad = 0xFFFFFFFFu;
    if (t < ni) {
        const uint4 r0 = in_tile[t * kXformPieces], r1 = in_tile[t * kXformPieces + 1], r2 = in_tile[t * kXformPieces + 2];
        const float a00 = __uint_as_float(r0.x), a01 = __uint_as_float(r0.y), a02 = __uint_as_float(r0.z), t0 = __uint_as_float(r0.w);
        const float a10 = __uint_as_float(r1.x), a11 = __uint_as_float(r1.y), a12 = __uint_as_float(r1.z), t1 = __uint_as_float(r1.w);
        const float a20 = __uint_as_float(r2.x), a21 = __uint_as_float(r2.y), a22 = __uint_as_float(r2.z), t2 = __uint_as_float(r2.w);
        const float all[12] = {a00, a01, a02, t0, a10, a11, a12, t1, a20, a21, a22, t2};
        uint32_t finite = 1u;                                     // no branch: every component is tested
#pragma unroll
        for (int c = 0; c < 12; c++) finite &= finite_bits(all[c]) ? 1u : 0u;
        bad = finite ? bad : i0 + t;
        // srh::world_to_object_3x3: adjugate / determinant
        const float c00 = a11 * a22 - a12 * a21;
        const float c01 = a12 * a20 - a10 * a22;
        const float c02 = a10 * a21 - a11 * a20;
        const float det = (a00 * c00 + a01 * c01) + a02 * c02;
        const float r = 1.0f / det;
        const float w0 = c00 * r, w1 = (a02 * a21 - a01 * a22) * r, w2 = (a01 * a12 - a02 * a11) * r;
        const float w3 = c01 * r, w4 = (a00 * a22 - a02 * a20) * r, w5 = (a02 * a10 - a00 * a12) * r;
        const float w6 = c02 * r, w7 = (a01 * a20 - a00 * a21) * r, w8 = (a00 * a11 - a01 * a10) * r;
        uint4* row = dev_tile + t * kDevRow;
        row[0] = make_uint4(__float_as_uint(w0), __float_as_uint(w1), __float_as_uint(w2), __float_as_uint(w3));
        row[1] = make_uint4(__float_as_uint(w4), __float_as_uint(w5), __float_as_uint(w6), __float_as_uint(w7));
        row[2] = make_uint4(__float_as_uint(w8), 0u, 0u, 0u);
        row[3] = make_uint4(r0.x, r0.y, r0.z, r1.x);              // (float3x3)ObjectToWorld3x4, row-major
        row[4] = make_uint4(r1.y, r1.z, r2.x, r2.y);
        row[5] = make_uint4(r2.z, 0u, 0u, 0u);
    }
    report_first_bad(bad, first_bad);
    __syncthreads();
    {
        uint4* __restrict__ to = dev + (uint64_t)i0 * kDevPieces;
#pragma unroll
        for (uint32_t k = 0; k < kDevPieces; k++) {
            const uint32_t p = k * kInstBlock + t;
            if (p < ni * kDevPieces) to[p] = dev_tile[p + p / kDevPieces];
        }
    }
    {
        uint4* __restrict__ to = flat + (uint64_t)i0 * kFlatPieces;
        const uint2* __restrict__ lay = layout + i0;
#pragma unroll
        for (uint32_t k = 0; k < kFlatPieces; k++) {
            const uint32_t p = k * kInstBlock + t;
            if (p >= ni * kFlatPieces) continue;
            const uint32_t i = p / kFlatPieces, piece = p % kFlatPieces;
            uint4 q;
            if (piece < kXformPieces) q = in_tile[i * kXformPieces + piece];
            else { const uint2 l = lay[i]; q = make_uint4(l.x, l.y, 0u, 0u); }
            to[p] = q;
        }
    }
}

}  // namespace srd

int srk_instance_tables(const SrTransform* transforms, const srd::InstanceLayout* layout, uint32_t n, srd::DevInstance* dev, srd::FlatInstance* flat,
                        uint32_t* first_bad, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n == 0) return 0;
    const uint32_t blocks = (n + srd::kInstBlock - 1) / srd::kInstBlock;
    srd::instance_tables_kernel<<<dim3(blocks), dim3(srd::kInstBlock), 0, stream>>>((const uint4*)transforms, (const uint2*)layout, n, (uint4*)dev, (uint4*)flat, first_bad);
    return (int)hipGetLastError();
}
