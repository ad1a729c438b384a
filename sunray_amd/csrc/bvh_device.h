// The per-element arithmetic of the device tree builders, shared by the kernels that run one launch per stage (bvh_gpu.hip) and the
// kernel that runs every stage of many small meshes in one launch, a workgroup per mesh (blas_batch.hip). Each function here is the
// body one thread of a stage executes for one element; the __global__ kernels are loops over them. The library is compiled with
// -ffp-contract=off, so the same function gives the same bits wherever it is inlined. Counters and encoded bounds are passed as
// pointers: global words in the per-stage kernels, LDS words in the batched one.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "bvh_gpu.h"
#include "bvh_layout.h"

namespace srd {

// The per-slot shading records of one triangle: `shade` = the three object-space vertex normals + (instance, mesh slot, 0) as
// `tail`; `shade_tex` (scenes with a textured material) = uv, normal-map uv, tangents, handedness of the first vertex
// (closest_hit.slang:34). The one definition of the device side: the fast build's leaves and the reshading update write the
// same bytes as the host builds (api.cpp full_build / build_blas).
__device__ __forceinline__ void write_shade(float4* shade, const SrVertex* const v[3], float tail_y, float tail_z, float tail_w) {
    shade[0] = make_float4(v[0]->normal[0], v[0]->normal[1], v[0]->normal[2], v[1]->normal[0]);
    shade[1] = make_float4(v[1]->normal[1], v[1]->normal[2], v[2]->normal[0], v[2]->normal[1]);
    shade[2] = make_float4(v[2]->normal[2], tail_y, tail_z, tail_w);
}
__device__ __forceinline__ void write_shade_tex(float4* q, const SrVertex* const v[3]) {
    q[0] = make_float4(v[0]->base_color_tex_coord[0], v[0]->base_color_tex_coord[1], v[1]->base_color_tex_coord[0], v[1]->base_color_tex_coord[1]);
    q[1] = make_float4(v[2]->base_color_tex_coord[0], v[2]->base_color_tex_coord[1], v[0]->normal_tex_coord[0], v[0]->normal_tex_coord[1]);
    q[2] = make_float4(v[1]->normal_tex_coord[0], v[1]->normal_tex_coord[1], v[2]->normal_tex_coord[0], v[2]->normal_tex_coord[1]);
    q[3] = make_float4(v[0]->tangent[0], v[0]->tangent[1], v[0]->tangent[2], v[0]->tangent[3] >= 0.0f ? 1.0f : -1.0f);
    q[4] = make_float4(v[1]->tangent[0], v[1]->tangent[1], v[1]->tangent[2], v[2]->tangent[0]);
    q[5] = make_float4(v[2]->tangent[1], v[2]->tangent[2], 0.0f, 0.0f);
}

// Padded box of one triangle record, as the host builder bounds it (bvh_build.cpp: fattened by the triangle
// test's barycentric slack, then one ulp each way).
__device__ __forceinline__ void tri_box(const float4* tris, uint32_t slot, float lo[3], float hi[3]) {
    const float4 a = tris[(size_t)slot * 3 + 0], b = tris[(size_t)slot * 3 + 1], c = tris[(size_t)slot * 3 + 2];
    const float v0[3] = {a.x, a.y, a.z}, e1[3] = {a.w, b.x, b.y}, e2[3] = {b.z, b.w, c.x};
    for (int k = 0; k < 3; k++) {
        const float p1 = v0[k] + e1[k], p2 = v0[k] + e2[k];
        const float pad = 4e-6f * (fabsf(e1[k]) + fabsf(e2[k]));
        const float l = fminf(v0[k], fminf(p1, p2)) - pad, h = fmaxf(v0[k], fmaxf(p1, p2)) + pad;
        lo[k] = fminf(lo[k], nextafterf(l, -INFINITY));
        hi[k] = fmaxf(hi[k], nextafterf(h, INFINITY));
    }
}

// What the builder's stages bound a primitive by: the padded box of a triangle record, or one of the instance boxes of a
// top-level tree (`map` takes the stage's index to the box: leaf position -> instance in the refit, null where the stage
// already holds the instance index).
struct TriPrims {
    const float4* tris;
    __device__ __forceinline__ void add(uint32_t i, float lo[3], float hi[3]) const { tri_box(tris, i, lo, hi); }
};
struct BoxPrims {
    const float* boxes;      // 6 floats per instance: lo, hi (a NaN row: the instance has no box)
    const uint32_t* map;
    __device__ __forceinline__ void add(uint32_t i, float lo[3], float hi[3]) const {
        const float* b = boxes + (size_t)(map ? map[i] : i) * 6;
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b[a]); hi[a] = fmaxf(hi[a], b[3 + a]); }
    }
};

// The (v0, v1, v2, prim) records of the mesh trees of the two-level form (api.cpp build_blas): tri_box with e1 = v1 - v0 and
// e2 = v2 - v0, the edges the host builder bounds the same triangle with; the vertices themselves are added as well, so the box
// also holds what build_blas takes for the mesh's root box (v1 and v0 + (v1 - v0) can differ in the last place).
struct VertPrims {
    const float4* tris;
    __device__ __forceinline__ void add(uint32_t i, float lo[3], float hi[3]) const {
        const float4 a = tris[(size_t)i * 3 + 0], b = tris[(size_t)i * 3 + 1], c = tris[(size_t)i * 3 + 2];
        const float v0[3] = {a.x, a.y, a.z}, v1[3] = {a.w, b.x, b.y}, v2[3] = {b.z, b.w, c.x};
        for (int k = 0; k < 3; k++) {
            const float e1 = v1[k] - v0[k], e2 = v2[k] - v0[k];
            const float p1 = v0[k] + e1, p2 = v0[k] + e2;
            const float pad = 4e-6f * (fabsf(e1) + fabsf(e2));
            const float l = fminf(fminf(v0[k], fminf(p1, p2)), fminf(v1[k], v2[k])) - pad;
            const float h = fmaxf(fmaxf(v0[k], fmaxf(p1, p2)), fmaxf(v1[k], v2[k])) + pad;
            lo[k] = fminf(lo[k], nextafterf(l, -INFINITY));
            hi[k] = fmaxf(hi[k], nextafterf(h, INFINITY));
        }
    }
};

// Refit of one 4-wide node: child boxes from the primitives (leaf children) or from the already refitted child nodes
// (node_box), then the same quantisation the host collapser applies (bvh_build.cpp Collapser::emit): origin = the next float below
// node min - extent / 2048 (about 1/8 cell), per axis the smallest power-of-two grid from frexp(extent / 255) on at which every
// child's upper plane fits in a byte, every plane the nearest cell that covers its box with a guard band of 1/32 cell, corrected
// against the decode expression fmaf(q, 2^e, origin).
constexpr double kGuardCells = 1.0 / 32.0;   // guard band around every quantised plane (see bvh_build.cpp, traverse.h)

template <class Prims>
__device__ __forceinline__ void refit_node(uint32_t* nodes, const Prims prims, float* node_box, uint32_t node) {
    constexpr int W = srl::kBvhWidth;
    uint32_t* q = nodes + (size_t)node * srl::kNodeDwords;
    float lo[W][3], hi[W][3];
    bool real[W];
    float lo_n[3] = {INFINITY, INFINITY, INFINITY}, hi_n[3] = {-INFINITY, -INFINITY, -INFINITY};
    int n_real = 0;
    for (int c = 0; c < W; c++) {
        const int ref = (int)q[srl::kChildOffset + c];
        for (int a = 0; a < 3; a++) { lo[c][a] = INFINITY; hi[c][a] = -INFINITY; }
        real[c] = false;
        if (ref >= 0) {
            const float* b = node_box + (size_t)ref * 6;
            for (int a = 0; a < 3; a++) { lo[c][a] = b[a]; hi[c][a] = b[3 + a]; }
            real[c] = lo[c][0] <= hi[c][0];
        } else {
            const uint32_t v = ~(uint32_t)ref, t0 = v >> 3, cnt = v & 7u;
            for (uint32_t t = 0; t < cnt; t++) prims.add(t0 + t, lo[c], hi[c]);
            real[c] = cnt != 0u;
        }
        if (!real[c]) continue;
        n_real++;
        for (int a = 0; a < 3; a++) { lo_n[a] = fminf(lo_n[a], lo[c][a]); hi_n[a] = fmaxf(hi_n[a], hi[c][a]); }
    }
    uint32_t plane[6 * srl::kPlaneDwords], scale_bits[3] = {0u, 0u, 0u};   // the fp32 number 2^e per axis
    for (int k = 0; k < 6 * srl::kPlaneDwords; k++) plane[k] = 0u;
    float origin[3] = {0.0f, 0.0f, 0.0f};
    if (n_real > 0) {
        for (int a = 0; a < 3; a++) {
            origin[a] = nextafterf(lo_n[a] - (hi_n[a] - lo_n[a]) * (1.0f / 2048.0f), -INFINITY);   // ~1/8 cell below the minimum
            const float ext = hi_n[a] - origin[a];
            int e = -126;
            if (ext > 0.0f && ext < INFINITY && ext / 255.0f > 0.0f) { int fe; (void)frexpf(ext / 255.0f, &fe); e = max(fe, -126); }
            if (!(ext < INFINITY)) e = 127;
            for (; e < 127; e++) {   // grow the grid until every child's upper plane fits in a byte
                const float scale = ldexpf(1.0f, e);
                bool ok = true;
                for (int c = 0; c < W && ok; c++) {
                    if (!real[c]) continue;
                    int qh = (int)ceil(((double)hi[c][a] - (double)origin[a]) / (double)scale + kGuardCells);
                    qh = max(qh, 0);
                    while (qh <= 255 && fmaf((float)qh, scale, origin[a]) < hi[c][a]) qh++;
                    if (qh > 255) ok = false;
                }
                if (ok) break;
            }
            const float scale = ldexpf(1.0f, e);
            scale_bits[a] = (uint32_t)(e + 127) << 23;   // e in [-126, 127]: a normal number, the bits of `scale`
            for (int c = 0; c < W; c++) {
                uint32_t ql = 255u, qh = 0u;   // inverted box for unused children
                if (real[c]) {
                    int l = (int)floor(((double)lo[c][a] - (double)origin[a]) / (double)scale - kGuardCells);
                    l = min(max(l, 0), 255);
                    while (l > 0 && fmaf((float)l, scale, origin[a]) > lo[c][a]) l--;
                    int h = (int)ceil(((double)hi[c][a] - (double)origin[a]) / (double)scale + kGuardCells);
                    h = min(max(h, 0), 255);
                    while (h < 255 && fmaf((float)h, scale, origin[a]) < hi[c][a]) h++;
                    ql = (uint32_t)l; qh = (uint32_t)h;
                }
                plane[a * srl::kPlaneDwords + c / 4] |= ql << (8 * (c % 4));
                plane[(3 + a) * srl::kPlaneDwords + c / 4] |= qh << (8 * (c % 4));
            }
        }
    } else {
        for (int a = 0; a < 3; a++) {
            for (int d = 0; d < srl::kPlaneDwords; d++) { plane[a * srl::kPlaneDwords + d] = 0xFFFFFFFFu; plane[(3 + a) * srl::kPlaneDwords + d] = 0u; }
            scale_bits[a] = 127u << 23;
        }
    }
    q[0] = __float_as_uint(origin[0]); q[1] = __float_as_uint(origin[1]); q[2] = __float_as_uint(origin[2]);
    q[srl::kScaleOffset[0]] = scale_bits[0]; q[srl::kScaleOffset[1]] = scale_bits[1]; q[srl::kScaleOffset[2]] = scale_bits[2];
    for (int k = 0; k < 6 * srl::kPlaneDwords; k++) q[srl::kPlaneOffset + k] = plane[k];
    float* b = node_box + (size_t)node * 6;
    for (int a = 0; a < 3; a++) { b[a] = lo_n[a]; b[3 + a] = hi_n[a]; }
}

// Order-preserving encoding of a float as an unsigned word: atomicMin / atomicMax on the encoding are fminf / fmaxf.
__device__ __forceinline__ uint32_t enc_f(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float dec_f(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }
// Word k of the eight a mesh's root box and padding numbers start from: the encoded +inf x 3, -inf x 3, 0, 0.
__host__ __device__ constexpr uint32_t mesh_acc_seed(int k) { return k < 3 ? 0xFF800000u : k < 6 ? 0x007FFFFFu : 0x80000000u; }

// ---- primitives of one mesh (srk_blas_build, the batched build) ------------------------------------------------------------
// What a thread accumulates over its primitives: the box the tree bounds them by (the Morton grid), build_blas's root box and the
// two padding numbers. fminf / fmaxf are exact, so the order of accumulation and reduction does not show in the result.
struct BlasPrimAcc {
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float max_abs = 0.0f, max_edge = 0.0f;
};

// One primitive: the (v0, v1, v2, prim) record straight from the positions, the centroid of its padded box, and its share of `r`.
__device__ __forceinline__ void blas_prim_one(const SrVertex* vtx, const uint32_t* idx, uint32_t n_vertices, uint32_t prim, float4* W, float4* cent,
                                              BlasPrimAcc& r) {
    const float* w[3];
    for (int j = 0; j < 3; j++) { const uint32_t vi = idx[3 * (size_t)prim + j]; w[j] = vtx[vi < n_vertices ? vi : 0u].position; }
    W[(size_t)prim * 3 + 0] = make_float4(w[0][0], w[0][1], w[0][2], w[1][0]);
    W[(size_t)prim * 3 + 1] = make_float4(w[1][1], w[1][2], w[2][0], w[2][1]);
    W[(size_t)prim * 3 + 2] = make_float4(w[2][2], __uint_as_float(prim), 0.0f, 0.0f);
    float blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    VertPrims{W}.add(prim, blo, bhi);
    cent[prim] = make_float4(0.5f * blo[0] + 0.5f * bhi[0], 0.5f * blo[1] + 0.5f * bhi[1], 0.5f * blo[2] + 0.5f * bhi[2], 0.0f);
    for (int a = 0; a < 3; a++) {      // build_blas: the padded triangle box and the two padding numbers
        r.blo[a] = fminf(r.blo[a], blo[a]); r.bhi[a] = fmaxf(r.bhi[a], bhi[a]);
        const float e1 = w[1][a] - w[0][a], e2 = w[2][a] - w[0][a];
        r.max_edge = fmaxf(r.max_edge, fabsf(e1) + fabsf(e2));
        for (int j = 0; j < 3; j++) r.max_abs = fmaxf(r.max_abs, fabsf(w[j][a]));
        const float pad = 4e-6f * (fabsf(e1) + fabsf(e2));
        const float l = fminf(w[0][a], fminf(w[1][a], w[2][a])) - pad;
        const float h = fmaxf(w[0][a], fmaxf(w[1][a], w[2][a])) + pad;
        r.lo[a] = fminf(r.lo[a], nextafterf(l, -INFINITY)); r.hi[a] = fmaxf(r.hi[a], nextafterf(h, INFINITY));
    }
}

// Every lane of the wave calls this: the wave reduces (cross-lane moves), lane 0 folds the result into the encoded words
// bounds_enc[0..5] (Morton grid) and acc[0..7] (root box lo, hi, max_abs_vertex, max_edge_sum).
__device__ __forceinline__ void blas_prims_reduce(BlasPrimAcc r, uint32_t* bounds_enc, uint32_t* acc) {
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) {
            r.blo[a] = fminf(r.blo[a], __shfl_xor(r.blo[a], o)); r.bhi[a] = fmaxf(r.bhi[a], __shfl_xor(r.bhi[a], o));
            r.lo[a] = fminf(r.lo[a], __shfl_xor(r.lo[a], o)); r.hi[a] = fmaxf(r.hi[a], __shfl_xor(r.hi[a], o));
        }
        r.max_abs = fmaxf(r.max_abs, __shfl_xor(r.max_abs, o)); r.max_edge = fmaxf(r.max_edge, __shfl_xor(r.max_edge, o));
    }
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; a++)
            if (r.blo[a] <= r.bhi[a]) { atomicMin(bounds_enc + a, enc_f(r.blo[a])); atomicMax(bounds_enc + 3 + a, enc_f(r.bhi[a])); }
        if (r.lo[0] <= r.hi[0]) {
            for (int a = 0; a < 3; a++) { atomicMin(acc + a, enc_f(r.lo[a])); atomicMax(acc + 3 + a, enc_f(r.hi[a])); }
            atomicMax(acc + 6, enc_f(r.max_abs)); atomicMax(acc + 7, enc_f(r.max_edge));
        }
    }
}

// ---- Morton keys ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long spread21(uint32_t v) {   // 21 bits -> every third bit
    unsigned long long x = v & 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// 63-bit Morton code of a point in the grid the encoded bounds span (21 bits per axis).
__device__ __forceinline__ unsigned long long morton_key(const float p[3], const uint32_t* bounds_enc) {
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const float lo = dec_f(bounds_enc[a]), hi = dec_f(bounds_enc[3 + a]);
        const float ext = hi - lo;
        float t = ext > 0.0f ? (p[a] - lo) / ext : 0.0f;
        t = fminf(fmaxf(t, 0.0f), 1.0f);                      // NaN -> 0
        q[a] = min((uint32_t)(t * 2097152.0f), 2097151u);
    }
    return spread21(q[0]) | (spread21(q[1]) << 1) | (spread21(q[2]) << 2);
}

// ---- binary radix tree (Karras 2012) ------------------------------------------------------------------------------------------
// delta(i, j): length of the common prefix of the sorted codes, ties broken by the index (Karras 2012, section 4)
__device__ __forceinline__ int lbvh_delta(const unsigned long long* keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    const unsigned long long a = keys[i], b = keys[j];
    if (a != b) return __clzll((long long)(a ^ b));
    return 64 + __clz(i ^ j);
}

// Inner node i (0 <= i < n - 1): its range, split and children; the parents of its children.
__device__ __forceinline__ void lbvh_hierarchy_node(const unsigned long long* keys, int n, int i, int2* children, uint32_t* parent_of_inner,
                                                    uint32_t* parent_of_leaf, uint2* range) {
    const int d = lbvh_delta(keys, n, i, i + 1) - lbvh_delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
    const int dmin = lbvh_delta(keys, n, i, i - d);
    int lmax = 2;
    while (lbvh_delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1) if (lbvh_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = lbvh_delta(keys, n, i, j);
    int s = 0;
    for (int t = l;;) {
        t = (t + 1) >> 1;
        if (lbvh_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
        if (t <= 1) break;
    }
    const int gamma = i + s * d + min(d, 0);
    const int first = min(i, j), last = max(i, j);
    int2 ch;
    ch.x = first == gamma ? ~gamma : gamma;               // leaf k is encoded ~k
    ch.y = last == gamma + 1 ? ~(gamma + 1) : gamma + 1;
    children[i] = ch;
    range[i] = make_uint2((uint32_t)first, (uint32_t)last);
    if (ch.x >= 0) parent_of_inner[ch.x] = (uint32_t)i; else parent_of_leaf[~ch.x] = (uint32_t)i;
    if (ch.y >= 0) parent_of_inner[ch.y] = (uint32_t)i; else parent_of_leaf[~ch.y] = (uint32_t)i;
    if (i == 0) parent_of_inner[0] = 0xFFFFFFFFu;
}

// Bottom-up fit from leaf i: boxes of the radix nodes and the stack height of a purely binary walk below each (0 for subtrees that
// will become leaves), second arriver at a node continues (the first one's writes are visible after the fence). A node's size is
// its Morton range where the tree has one (`range`, the radix tree), the sum of its children's otherwise (a rebalanced tree).
template <class Prims>
__device__ __forceinline__ void lbvh_fit_from_leaf(const Prims prims, const uint32_t* sorted_gid, int i, const int2* children, const uint32_t* parent_of_inner,
                                                   const uint32_t* parent_of_leaf, const uint2* range, float* bin_box, uint32_t* bin_height,
                                                   uint32_t* bin_size, uint32_t* flags) {
    uint32_t node = parent_of_leaf[i];
    while (node != 0xFFFFFFFFu) {
        __threadfence();
        if (atomicAdd(flags + node, 1u) == 0u) return;
        __threadfence();
        const int2 ch = children[node];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        uint32_t h = 0, size = 0;
        const int cc[2] = {ch.x, ch.y};
        for (int c = 0; c < 2; c++) {
            if (cc[c] < 0) { prims.add(sorted_gid[~cc[c]], lo, hi); size += 1u; }
            else {
                const volatile float* b = bin_box + (size_t)cc[c] * 6;
                for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], b[a]); hi[a] = fmaxf(hi[a], b[3 + a]); }
                h = max(h, ((const volatile uint32_t*)bin_height)[cc[c]]);
                if (!range) size += ((const volatile uint32_t*)bin_size)[cc[c]];
            }
        }
        if (range) { const uint2 r = range[node]; size = r.y - r.x + 1u; }      // radix tree: the node's Morton range
        float* b = bin_box + (size_t)node * 6;
        for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
        bin_size[node] = size;
        bin_height[node] = (size <= srl::kLeafMax) ? 0u : h + 1u;
        node = parent_of_inner[node];
    }
}

// ---- PLOC (Meister & Bittner 2018), one cluster of one iteration --------------------------------------------------------------
template <class Prims>
__device__ __forceinline__ void ploc_init_one(const Prims prims, const uint32_t* sorted_gid, uint32_t i, int* cid, float* cbox) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    prims.add(sorted_gid[i], lo, hi);
    cid[i] = ~(int)i;
    float* b = cbox + (size_t)i * 6;
    for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
}

// The neighbour of cluster i within `radius` whose union with it has the smallest surface area.
// SPREAD_TIES (instance boxes): among candidates of equal area the nearest one in the order wins, and of the two at the same
// distance the partner i ^ 1. The rule is symmetric in (i, j), so the best pair overall is still mutual and every iteration
// merges; coincident boxes then pair up (0,1), (2,3), ... and halve each iteration instead of merging one pair at a time.
template <bool SPREAD_TIES>
__device__ __forceinline__ uint32_t ploc_nn_one(const float* cbox, uint32_t m, uint32_t radius, uint32_t i) {
    const float* b = cbox + (size_t)i * 6;
    const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
    const uint32_t j0 = i > radius ? i - radius : 0u, j1 = min(m - 1u, i + radius);
    float best = INFINITY; uint32_t best_j = i, best_rank = 0xFFFFFFFFu;
    for (uint32_t j = j0; j <= j1; j++) {
        if (j == i) continue;
        const float* c = cbox + (size_t)j * 6;
        const float dx = fmaxf(hi[0], c[3]) - fminf(lo[0], c[0]), dy = fmaxf(hi[1], c[4]) - fminf(lo[1], c[1]), dz = fmaxf(hi[2], c[5]) - fminf(lo[2], c[2]);
        const float area = dx * dy + dy * dz + dz * dx;
        if (SPREAD_TIES) {
            const uint32_t rank = 2u * (j > i ? j - i : i - j) + (j == (i ^ 1u) ? 0u : 1u);
            if (area < best || (area == best && rank < best_rank)) { best = area; best_j = j; best_rank = rank; }
        } else if (area < best) { best = area; best_j = j; }        // ties: the lower index (scan order)
    }
    return best_j;
}

// Mutual nearest neighbours merge (the lower index keeps the merged cluster, the higher one is dropped).
__device__ __forceinline__ void ploc_merge_one(const uint32_t* nn, uint32_t i, int* cid, float* cbox, uint32_t* valid, int2* children, float* bin_box,
                                               uint32_t* bin_size, uint32_t* bin_height, uint32_t* node_counter) {
    const uint32_t j = nn[i];
    if (j == i || nn[j] != i) { valid[i] = 1u; return; }
    if (j < i) { valid[i] = 0u; return; }
    const int ci = cid[i], cj = cid[j];
    const uint32_t node = atomicAdd(node_counter, 1u);
    const uint32_t si = ci < 0 ? 1u : bin_size[ci], sj = cj < 0 ? 1u : bin_size[cj];
    const uint32_t hi_ = ci < 0 ? 0u : bin_height[ci], hj = cj < 0 ? 0u : bin_height[cj];
    children[node] = make_int2(ci, cj);
    bin_size[node] = si + sj;
    bin_height[node] = (si + sj <= srl::kLeafMax) ? 0u : max(hi_, hj) + 1u;
    float* bi = cbox + (size_t)i * 6;
    const float* bj = cbox + (size_t)j * 6;
    float* nb = bin_box + (size_t)node * 6;
    for (int a = 0; a < 3; a++) { bi[a] = fminf(bi[a], bj[a]); bi[3 + a] = fmaxf(bi[3 + a], bj[3 + a]); nb[a] = bi[a]; nb[3 + a] = bi[3 + a]; }
    cid[i] = (int)node;
    valid[i] = 1u;
}

// A surviving cluster i moves to position p of the other buffer.
__device__ __forceinline__ void ploc_compact_one(const int* cid, const float* cbox, uint32_t i, uint32_t p, int* cid_out, float* cbox_out) {
    cid_out[p] = cid[i];
    for (int a = 0; a < 6; a++) cbox_out[(size_t)p * 6 + a] = cbox[(size_t)i * 6 + a];
}

// ---- collapse to 4-wide nodes ---------------------------------------------------------------------------------------------
// A child of a 4-wide node during the collapse: `ref` is a binary-tree reference (>= 0: binary node, < 0: single triangle
// ~sorted index); subtrees of at most kLeafMax triangles become leaves.
struct LbvhKid { int ref; uint32_t size; float area; uint32_t need; bool inner; };

__device__ __forceinline__ LbvhKid lbvh_kid(int ref, const uint32_t* bin_size, const float* bin_box, const uint32_t* bin_height) {
    LbvhKid k;
    k.ref = ref; k.area = 0.0f; k.need = 0; k.inner = false;
    if (ref < 0) { k.size = 1; return k; }
    k.size = bin_size[ref];
    if (k.size <= srl::kLeafMax) return k;
    const float* b = bin_box + (size_t)ref * 6;
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    k.area = dx * dy + dy * dz + dz * dx; k.need = bin_height[ref]; k.inner = true;
    return k;
}

// Eight entries addressed by compare and select, so that the stack lives in registers wherever the function is inlined.
struct SmallStack {
    int a, b, c, d, e, f, g, h;
    __device__ __forceinline__ int get(int i) const { return i == 0 ? a : i == 1 ? b : i == 2 ? c : i == 3 ? d : i == 4 ? e : i == 5 ? f : i == 6 ? g : h; }
    __device__ __forceinline__ void set(int i, int x) {
        a = i == 0 ? x : a; b = i == 1 ? x : b; c = i == 2 ? x : c; d = i == 3 ? x : d;
        e = i == 4 ? x : e; f = i == 5 ? x : f; g = i == 6 ? x : g; h = i == 7 ? x : h;
    }
};

// The 4-wide node `self` of the current level. counters: [0] = nodes allocated, [1] = max stack, [2] = overflow flag.
// Leaf slots: a node owns the slot range [first_of_node, first_of_node + size) of the leaf-order arrays; its children take
// consecutive sub-ranges in child order, and the triangles of a leaf child get their slots here (slot_of_sorted), so the
// binary tree's subtrees need not be contiguous in Morton order (they are for the radix tree, not for PLOC).
__device__ __forceinline__ void lbvh_collapse_node(uint32_t* nodes, uint32_t self, uint32_t node_cap, int* bin_of_node, uint32_t* budget_of_node,
                                                   uint32_t* prefix_of_node, uint32_t* first_of_node, const int2* children, const uint32_t* bin_size,
                                                   const float* bin_box, const uint32_t* bin_height, uint32_t* slot_of_sorted, uint32_t* counters) {
    const int bin = bin_of_node[self];
    const uint32_t budget = budget_of_node[self];
    constexpr int W = srl::kBvhWidth;
    LbvhKid kids[W];
    int nk = 0;
    const int2 ch = children[bin];
    kids[nk++] = lbvh_kid(ch.x, bin_size, bin_box, bin_height);
    kids[nk++] = lbvh_kid(ch.y, bin_size, bin_box, bin_height);
    // kids[] is only ever indexed by an unrolled loop counter (compare and select for the opened child), so it stays in registers
#pragma unroll
    for (int round = 0; round < W - 2; round++) {
        if (nk >= W) break;
        int best = -1, best_ref = 0; float best_area = -1.0f;
#pragma unroll
        for (int i = 0; i < W; i++) if (i < nk && kids[i].inner && kids[i].area > best_area) { best_area = kids[i].area; best = i; best_ref = kids[i].ref; }
        if (best < 0) break;
        const int2 cb = children[best_ref];
        const LbvhKid ka = lbvh_kid(cb.x, bin_size, bin_box, bin_height), kb = lbvh_kid(cb.y, bin_size, bin_box, bin_height);
        bool fits = ka.need + (uint32_t)nk <= budget && kb.need + (uint32_t)nk <= budget;   // with nk+1 children every subtree gets budget - nk entries
#pragma unroll
        for (int i = 0; i < W; i++) if (i < nk && i != best && kids[i].need + (uint32_t)nk > budget) fits = false;
        if (!fits) break;
#pragma unroll
        for (int i = 0; i < W; i++) { if (i == best) kids[i] = ka; else if (i == nk) kids[i] = kb; }
        nk++;
    }
    uint32_t* q = nodes + (size_t)self * srl::kNodeDwords;
    for (int k = 0; k < srl::kNodeDwords; k++) q[k] = 0u;
    const uint32_t mine = prefix_of_node[self] + (uint32_t)(nk - 1);
    atomicMax(counters + 1, mine);
    uint32_t first = first_of_node[self];
#pragma unroll
    for (int i = 0; i < W; i++) {
        uint32_t ref = 0xFFFFFFFFu;                              // leaf_ref(0, 0): unused child
        if (i < nk) {
            if (kids[i].inner) {
                const uint32_t idx = atomicAdd(counters + 0, 1u);
                if (idx < node_cap) {
                    bin_of_node[idx] = kids[i].ref;
                    budget_of_node[idx] = budget - (uint32_t)(nk - 1);
                    prefix_of_node[idx] = mine;
                    first_of_node[idx] = first;
                    ref = idx;
                } else { atomicExch(counters + 2, 1u); }
            } else {
                ref = ~((first << 3) | kids[i].size);
                // slots of the leaf's triangles: walk the (at most kLeafMax-triangle) binary subtree
                SmallStack stack = {0, 0, 0, 0, 0, 0, 0, 0}; int sp = 0; uint32_t slot = first;
                stack.set(sp++, kids[i].ref);
                while (sp > 0) {
                    const int r = stack.get(--sp);
                    if (r < 0) slot_of_sorted[~r] = slot++;
                    else { const int2 c2 = children[r]; if (sp < 7) { stack.set(sp++, c2.y); stack.set(sp++, c2.x); } }
                }
            }
            first += kids[i].size;
        }
        q[srl::kChildOffset + i] = ref;
    }
}

// ---- one mesh's records, references and result ---------------------------------------------------------------------------------
// Leaf-order records of one triangle of a mesh (by sorted index): record, shade, shade_tex at tri_base + slot, primitive -> slot.
__device__ __forceinline__ void blas_leaf_one(const float4* W, const uint32_t* sorted_gid, const uint32_t* slot_of_sorted, uint32_t s_idx, uint32_t n_tris,
                                              const SrVertex* vtx, const uint32_t* idx, uint32_t n_vertices, uint32_t mesh_slot, uint32_t tri_base,
                                              float4* tris, float4* shade, float4* shade_tex, uint32_t* slot_of_gid) {
    const uint32_t local = slot_of_sorted[s_idx], prim = sorted_gid[s_idx];
    if (local >= n_tris || prim >= n_tris) return;      // cannot happen for a tree the collapse finished; never index out of the mesh's range
    const size_t slot = (size_t)tri_base + local;
    for (int k = 0; k < 3; k++) tris[slot * 3 + k] = W[(size_t)prim * 3 + k];
    slot_of_gid[(size_t)tri_base + prim] = tri_base + local;
    const SrVertex* v[3];
    for (int j = 0; j < 3; j++) { const uint32_t vi = idx[3 * (size_t)prim + j]; v[j] = vtx + (vi < n_vertices ? vi : 0u); }
    write_shade(shade + slot * 3, v, 0.0f, __uint_as_float(mesh_slot), 0.0f);      // no instance: it comes from the walk (build_blas)
    if (shade_tex) write_shade_tex(shade_tex + slot * 6, v);
}

// The child references of one node (q: its kChildOffset words) become global as BlasCat::append (api.cpp) makes them.
__device__ __forceinline__ void blas_place_node(uint32_t* q, uint32_t node_base, uint32_t tri_base) {
    for (int c = 0; c < srl::kBvhWidth; c++) {
        const int ref = (int)q[c];
        if (ref >= 0) q[c] = (uint32_t)ref + node_base;
        else { const uint32_t lv = ~(uint32_t)ref, cnt = lv & 7u; if (cnt) q[c] = ~((((lv >> 3) + tri_base) << 3) | cnt); }
    }
}

// counters: the collapse's ([0] nodes allocated, [1] max stack). out: 8 floats, then node count and stack need as dwords.
__device__ __forceinline__ void blas_build_finish(const uint32_t* acc, const uint32_t* counters, uint32_t mesh_slot, uint32_t node_base, uint32_t tri_base,
                                                  uint32_t n_tris, TlMeshRow* rows, uint32_t* out) {
    float f[8];
    for (int k = 0; k < 8; k++) { f[k] = dec_f(acc[k]); out[k] = __float_as_uint(f[k]); }
    out[8] = counters[0]; out[9] = counters[1];
    if (rows) {
        TlMeshRow* r = rows + mesh_slot;
        for (int a = 0; a < 3; a++) { r->lo[a] = f[a]; r->hi[a] = f[3 + a]; }
        r->max_abs_vertex = f[6]; r->max_edge_sum = f[7];
        r->max_stack = counters[1]; r->blas_root = node_base; r->prim_base = tri_base; r->n_tris = n_tris;
    }
}

}  // namespace srd
