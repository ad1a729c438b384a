// Area-weighted normals and uv-aligned tangents of a mesh from new positions alone (sr_scene_update_mesh_positions*,
// include/sunray_hip.h states the rule to the letter). fp32 under the numerics contract of DESIGN.md §3: no contraction, correctly
// rounded divide and sqrt, grouping as written. No float atomics: a store pass per triangle, then a sum pass per vertex in the
// order the attach fixed, so the bytes are the same from run to run and equal sr_mesh_frame_host's (mesh_frame.cpp).
#include "normals.h"

#include "vertex_tile.h"

namespace srd {

static_assert(sizeof(srh::FrameTriUv) == 16, "face_frame_kernel reads a triangle's uv terms as one 16-byte piece");

// One triangle per thread. The three positions are gathered as dwords (12-byte records: no wider load is aligned); the locality
// is the index buffer's. The results leave as whole 16-byte pieces, consecutive lanes on consecutive triangles.
template <bool kTangents>
__global__ void __launch_bounds__(kTileBlock) face_frame_kernel(const float* __restrict__ positions, const uint32_t* __restrict__ indices,
                                                                 const float4* __restrict__ tri_uv, float4* __restrict__ faces, uint32_t n_triangles) {
    const uint32_t t = blockIdx.x * kTileBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const uint32_t* ix = indices + (uint64_t)t * 3;
    const float* p0 = positions + (uint64_t)ix[0] * 3;
    const float* p1 = positions + (uint64_t)ix[1] * 3;
    const float* p2 = positions + (uint64_t)ix[2] * 3;
    const float x0 = p0[0], y0 = p0[1], z0 = p0[2];
    const float e1x = p1[0] - x0, e1y = p1[1] - y0, e1z = p1[2] - z0;
    const float e2x = p2[0] - x0, e2y = p2[1] - y0, e2z = p2[2] - z0;
    const float4 F = make_float4(e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x, 0.0f);
    if (!kTangents) { faces[t] = F; return; }
    const float4 uv = tri_uv[t];                             // a.y, b.y, s
    float4 T = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (uv.z != 0.0f) { T.x = uv.z * (e1x * uv.y - e2x * uv.x); T.y = uv.z * (e1y * uv.y - e2y * uv.x); T.z = uv.z * (e1z * uv.y - e2z * uv.x); }
    faces[(uint64_t)t * 2] = F;
    faces[(uint64_t)t * 2 + 1] = T;
}

// One vertex per thread on the tile of vertex_tile.h, like pose_batch_kernel: the reference records are turned by the
// LDS and every byte this kernel does not write is the reference's. A thread reads its own position (12 bytes, the lanes of a wave
// together whole cache lines), walks its run and gathers one or two dwordx4 per entry. The sums are the thread's own, in run order.
template <bool kTangents>
__global__ void __launch_bounds__(kTileBlock) vertex_frame_kernel(const uint4* __restrict__ reference, const float* __restrict__ positions,
                                                                   const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ entries,
                                                                   const float* __restrict__ side, const float4* __restrict__ faces,
                                                                   uint4* __restrict__ out, uint32_t n_vertices, uint32_t* first_bad) {
    __shared__ uint4 tile[kTileBlock * kTileRow];
    const VertexTile vt(n_vertices);
    const uint32_t t = threadIdx.x, v = vt.v0 + t;
    vt.load(tile, reference);
    uint32_t bad = 0xFFFFFFFFu;
    if (t < vt.nv) {
        const float* p = positions + (uint64_t)v * 3;
        const float px = p[0], py = p[1], pz = p[2];
        if (!(finite_bits(px) && finite_bits(py) && finite_bits(pz))) bad = v;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, ax = 0.0f, ay = 0.0f, az = 0.0f;
        const uint32_t end = offsets[v + 1];
        for (uint32_t e = offsets[v]; e < end; e++) {
            const uint64_t f = (uint64_t)entries[e] * (kTangents ? 2 : 1);
            const float4 F = faces[f];
            nx = nx + F.x; ny = ny + F.y; nz = nz + F.z;
            if (kTangents) {
                const float4 T = faces[f + 1];
                ax = ax + T.x; ay = ay + T.y; az = az + T.z;
            }
        }
        const float s = side[v];
        uint4* row = VertexTile::row(tile, t);
        row[0].x = __float_as_uint(px); row[0].y = __float_as_uint(py); row[0].z = __float_as_uint(pz);
        store_normalised(row + 1, s * nx, s * ny, s * nz);
        if (kTangents) {
            const uint4 N = row[1];                          // the new normal, or the reference's where it fell back
            const float mx = __uint_as_float(N.x), my = __uint_as_float(N.y), mz = __uint_as_float(N.z);
            const float d = (mx * ax + my * ay) + mz * az;
            store_normalised(row + 2, ax - mx * d, ay - my * d, az - mz * d);
        }
    }
    vt.store(tile, out);
    report_first_bad(bad, first_bad);
}

}  // namespace srd

int srk_mesh_frame(const SrVertex* reference, const float* positions, const uint32_t* indices, const srh::FrameTriUv* tri_uv, const uint32_t* offsets,
                   const uint32_t* entries, const float* side, uint32_t flags, float4* faces, SrVertex* out, uint32_t n_vertices, uint32_t n_triangles,
                   uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const bool tangents = (flags & SR_FRAME_TANGENTS) != 0;
    const uint32_t face_blocks = (uint32_t)(((uint64_t)n_triangles + srd::kTileBlock - 1) / srd::kTileBlock);
    const uint32_t blocks = (uint32_t)(((uint64_t)n_vertices + srd::kTileBlock - 1) / srd::kTileBlock);
    if (face_blocks) {
        if (tangents) srd::face_frame_kernel<true><<<dim3(face_blocks), dim3(srd::kTileBlock), 0, stream>>>(positions, indices, (const float4*)tri_uv, faces, n_triangles);
        else srd::face_frame_kernel<false><<<dim3(face_blocks), dim3(srd::kTileBlock), 0, stream>>>(positions, indices, (const float4*)tri_uv, faces, n_triangles);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    }
    if (tangents) srd::vertex_frame_kernel<true><<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)reference, positions, offsets, entries, side, faces, (uint4*)out, n_vertices, first_bad);
    else srd::vertex_frame_kernel<false><<<dim3(blocks), dim3(srd::kTileBlock), 0, stream>>>((const uint4*)reference, positions, offsets, entries, side, faces, (uint4*)out, n_vertices, first_bad);
    return (int)hipGetLastError();
}
