// Device side of the acceleration-structure maintenance: what the reference gets from
// vkCmdBuildAccelerationStructuresKHR in UPDATE mode (tlas.rs:124-140, accel.rs:263-267) — new instance
// transforms, same topology — done here as (1) re-flattening the instances' triangles to world space, in the
// same operation order as the host (bvh_build.cpp flatten_instances) so the records are bit-identical to a
// rebuild's, and (2) a bottom-up refit of the quantised 4-wide nodes. Box culling is conservative on every
// side, so query results do not depend on which tree answers them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <type_traits>
#include <utility>

#include <hipcub/hipcub.hpp>

#include <vector>

#include "bvh_device.h"
#include "bvh_gpu.h"
#include "bvh_layout.h"
#include "tl_record.h"
#include "traverse.h"
#include "vertex_tile.h"

namespace srd {

__device__ __forceinline__ void triangle_vertices(const SrMeshInfo* meshes, const FlatInstance& inst, uint32_t prim, const SrVertex* v[3]) {
    const SrMeshInfo mi = meshes[inst.mesh_slot];
    const uint32_t* idx = (const uint32_t*)(uintptr_t)mi.indices;
    const SrVertex* vtx = (const SrVertex*)(uintptr_t)mi.vertices;
    for (int j = 0; j < 3; j++) v[j] = vtx + idx[3 * prim + j];
}

__device__ __forceinline__ void world_triangle(const SrMeshInfo* meshes, const FlatInstance& inst, uint32_t prim, float v0[3], float e1[3], float e2[3],
                                               const SrVertex* v[3]) {
    triangle_vertices(meshes, inst, prim, v);
    const float* m = inst.o2w;
    float w[3][3];
    for (int j = 0; j < 3; j++) {
        const float* q = v[j]->position;
        // transform_point (rt_utils.slang:278-281): rows dotted with (p, 1), left to right
        w[j][0] = ((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]) + m[3] * 1.0f;
        w[j][1] = ((m[4] * q[0] + m[5] * q[1]) + m[6] * q[2]) + m[7] * 1.0f;
        w[j][2] = ((m[8] * q[0] + m[9] * q[1]) + m[10] * q[2]) + m[11] * 1.0f;
    }
    for (int a = 0; a < 3; a++) { v0[a] = w[0][a]; e1[a] = w[1][a] - w[0][a]; e2[a] = w[2][a] - w[0][a]; }
}

// One thread per leaf-order slot: the slot keeps its triangle (global id), only the world-space record changes.
// RESHADE (a mesh's vertices changed, sr_scene_update_mesh): the slot's shading records are rewritten as well, from the same
// three vertex records the positions come from (normals, uvs and tangents sit next to the position in the 96-byte SrVertex);
// the instance and mesh-slot words of `shade` are kept. TEX: the scene has shade_tex records.
template <bool RESHADE, bool TEX>
__global__ void flatten_slots_kernel(float4* tris, typename std::conditional<RESHADE, float4*, const float4*>::type shade, const SrMeshInfo* meshes,
                                     const FlatInstance* instances, uint32_t n_tris, float4* shade_tex) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_tris) return;
    const uint32_t gid = __float_as_uint(tris[(size_t)slot * 3 + 2].y);   // record: (v0, e1, e2, gid, 0, 0), bvh_build.cpp
    float4 tail = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (RESHADE) tail = shade[(size_t)slot * 3 + 2]; else tail.y = shade[(size_t)slot * 3 + 2].y;
    const uint32_t ii = __float_as_uint(tail.y);
    const FlatInstance inst = instances[ii];
    if (gid < inst.tri_offset) return;      // cannot happen for a tree built from this layout; never index out of bounds
    float v0[3], e1[3], e2[3];
    const SrVertex* v[3];
    world_triangle(meshes, inst, gid - inst.tri_offset, v0, e1, e2, v);
    tris[(size_t)slot * 3 + 0] = make_float4(v0[0], v0[1], v0[2], e1[0]);
    tris[(size_t)slot * 3 + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    tris[(size_t)slot * 3 + 2] = make_float4(e2[2], __uint_as_float(gid), 0.0f, 0.0f);
    if constexpr (RESHADE) {
        write_shade(shade + (size_t)slot * 3, v, tail.y, tail.z, tail.w);
        if constexpr (TEX) write_shade_tex(shade_tex + (size_t)slot * 6, v);
    }
}

// One thread per node of one tree level (deepest level first): child boxes from the primitives (leaf children) or
// from the already refitted child nodes (node_box), then the quantisation of refit_node (bvh_device.h), the one
// the host collapser applies (bvh_build.cpp Collapser::emit).
template <class Prims>
__global__ void refit_level_kernel(uint32_t* nodes, const Prims prims, float* node_box, const uint32_t* level_nodes, uint32_t first, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t node = level_nodes ? level_nodes[first + i] : first + i;   // null list: the level is the index range itself
    refit_node(nodes, prims, node_box, node);
}


// ---------------------------------------------------------------------------------------------------------------
// OpType::FastBuild on the device (PREFER_FAST_BUILD, acceleration_structure/mod.rs:33-35): a linear BVH.
//   prims      world-space triangle records + centroids of their padded boxes, scene bounds (wave-reduced atomics)
//   morton     63-bit Morton code of the centroid (21 bits per axis), radix-sorted with the triangle id (hipCUB)
//   hierarchy  binary radix tree over the sorted codes (Karras 2012; equal codes are split by index)
//   fit        bottom-up: box and "binary walk height" of every radix node (second arriver continues upward)
//   collapse   top-down, one launch per level: radix subtrees of <= kLeafMax triangles become leaves (their triangles are
//              consecutive in sorted order = leaf order), inner nodes take up to 4 children by repeatedly opening
//              the child with the largest box while the stack budget allows (same rule as bvh_build.cpp's Collapser)
//   leaves     triangle / shade / shade_tex records in leaf order, slot_of_gid
//   refit      the kernel above computes the boxes of the 4-wide nodes and quantises them, deepest level first
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t find_instance(const FlatInstance* inst, uint32_t n_inst, uint32_t gid) {
    uint32_t lo = 0, hi = n_inst;            // last instance whose tri_offset <= gid
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (inst[mid].tri_offset <= gid) lo = mid; else hi = mid; }
    return lo;
}
__global__ void lbvh_prims_kernel(const SrMeshInfo* meshes, const FlatInstance* instances, uint32_t n_inst, uint32_t n_tris, float4* W, float4* cent,
                                  uint32_t* bounds_enc) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (gid < n_tris) {
        const uint32_t ii = find_instance(instances, n_inst, gid);
        const FlatInstance inst = instances[ii];
        float v0[3], e1[3], e2[3];
        const SrVertex* v[3];
        world_triangle(meshes, inst, gid - inst.tri_offset, v0, e1, e2, v);
        W[(size_t)gid * 3 + 0] = make_float4(v0[0], v0[1], v0[2], e1[0]);
        W[(size_t)gid * 3 + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
        W[(size_t)gid * 3 + 2] = make_float4(e2[2], __uint_as_float(gid), 0.0f, 0.0f);
        tri_box(W, gid, lo, hi);
        cent[gid] = make_float4(0.5f * lo[0] + 0.5f * hi[0], 0.5f * lo[1] + 0.5f * hi[1], 0.5f * lo[2] + 0.5f * hi[2], __uint_as_float(ii));
    }
    for (int a = 0; a < 3; a++) {
        float l = lo[a], h = hi[a];
        for (int o = 32; o > 0; o >>= 1) { l = fminf(l, __shfl_xor(l, o)); h = fmaxf(h, __shfl_xor(h, o)); }
        if ((threadIdx.x & 63) == 0) {
            if (l <= h) { atomicMin(bounds_enc + a, enc_f(l)); atomicMax(bounds_enc + 3 + a, enc_f(h)); }
        }
    }
}

__global__ void lbvh_morton_kernel(const float4* cent, const uint32_t* bounds_enc, uint32_t n_tris, unsigned long long* keys, uint32_t* vals) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_tris) return;
    const float4 c = cent[gid];
    const float p[3] = {c.x, c.y, c.z};
    keys[gid] = morton_key(p, bounds_enc);
    vals[gid] = gid;
}

__global__ void lbvh_hierarchy_kernel(const unsigned long long* keys, int n, int2* children, uint32_t* parent_of_inner, uint32_t* parent_of_leaf, uint2* range) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n - 1) return;
    lbvh_hierarchy_node(keys, n, i, children, parent_of_inner, parent_of_leaf, range);
}

// Bottom-up fit: boxes of the radix nodes and the stack height of a purely binary walk below each (0 for subtrees that
// will become leaves), second arriver at a node continues (the first one's writes are visible after the fence). A node's size is
// its Morton range where the tree has one (`range`, the radix tree), the sum of its children's otherwise (a rebalanced tree).
template <class Prims>
__global__ void lbvh_fit_kernel(const Prims prims, const uint32_t* sorted_gid, int n, const int2* children, const uint32_t* parent_of_inner,
                                const uint32_t* parent_of_leaf, const uint2* range, float* bin_box, uint32_t* bin_height, uint32_t* bin_size,
                                uint32_t* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lbvh_fit_from_leaf(prims, sorted_gid, i, children, parent_of_inner, parent_of_leaf, range, bin_box, bin_height, bin_size, flags);
}

// ---------------------------------------------------------------------------------------------------------------
// Height bound (TreeBuildTarget::rebalance): a binary tree whose walk height h(root) exceeds the stack cap is rewritten so that it
// fits, between the topology stage and the collapse. H(k) is the walk height of a median-split tree over k primitives. The
// root's allowance is A = stack_cap, a child's its parent's minus one. At a node v: h(v) <= A(v): the subtree is kept whole;
// otherwise, if both children c have H(size(c)) <= A(v) - 1, v's split is kept and the rule goes on in the children; otherwise
// v's subtree is rebuilt as a median-split tree over its own leaves in depth-first order, on its own inner node ids. By
// induction H(size(v)) <= A(v) wherever the rule arrives, so afterwards h(root) <= stack_cap, and the builder's topology
// survives everywhere except below the deepest, smallest offending nodes. Every kernel reads only what an earlier launch wrote:
//   links      one thread per inner node: parent, left-sibling size of both children; own h, 1 + max H(size(child)), left size
//   walk       one thread per leaf and per inner node, twice up the parent links (depth first, then the rule with the depths
//              known): the topmost ancestor the rule rebuilds, the node's depth-first position (leaf) or in-order gap (inner
//              node: position of the last leaf of its left subtree) -> leaf_at_pos, inner_at_gap, the subtree's range
//   rebuild    one thread per inner node of a rebuilt subtree: down the implicit median tree over the range to the node whose
//              split gap is its own (<= 32 steps), children from the two arrays alone (never from children[], which it writes);
//              the subtree's old root re-points its parent's reference, or the root id, to the holder of the median gap
//   parents    parent arrays of the rewritten tree for lbvh_fit_kernel, which then recomputes box, size and height of every node
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kNoNode = 0xFFFFFFFFu;
constexpr int kMaxBinaryWalk = 4096 + 64;      // a radix tree is < 100 levels tall, a PLOC tree at most its iteration count (4096)

__device__ __forceinline__ bool binary_ref_ok(int ref, uint32_t n) { return ref < 0 ? (uint32_t)~ref < n : (uint32_t)ref + 1u < n; }

__host__ __device__ __forceinline__ uint32_t median_height(uint32_t k) {      // H(k)
    uint32_t h = 0;
    for (int i = 0; i < 32 && k > srl::kLeafMax; i++) { k = (k + 1u) >> 1; h++; }
    return h;
}

// link[u] = (parent, h(u) | (1 + max H(size(child))) << 16, size of u's left sibling (0: u is a left child or the root), size of
// u's left child); leaf_link[k] = (parent, size of the left sibling). A thread writes .y and .w of its own node and .x and .z
// of its children: every word has one writer.
__global__ void rebalance_links_kernel(const int2* children, const uint32_t* bin_size, const uint32_t* bin_height, uint32_t n, uint32_t root, uint4* link,
                                       uint2* leaf_link) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u + 1u >= n) return;
    const int2 ch = children[u];
    if (!binary_ref_ok(ch.x, n) || !binary_ref_ok(ch.y, n)) return;      // cannot happen; the walk then reports the broken chain
    const uint32_t sl = ch.x < 0 ? 1u : bin_size[ch.x], sr = ch.y < 0 ? 1u : bin_size[ch.y];
    if (ch.x < 0) leaf_link[~ch.x] = make_uint2(u, 0u); else { link[ch.x].x = u; link[ch.x].z = 0u; }
    if (ch.y < 0) leaf_link[~ch.y] = make_uint2(u, sl); else { link[ch.y].x = u; link[ch.y].z = sl; }
    link[u].y = min(bin_height[u], 0xFFFFu) | (1u + max(median_height(sl), median_height(sr))) << 16;
    link[u].w = sl;
    if (u == root) { link[u].x = kNoNode; link[u].z = 0u; }
}

// rb_range[x] = (first position, size) of the rebuilt subtree inner node x lies in ((0, 0): none); rb_gap[x] = its in-order gap,
// bit 31 set for the subtree's root.
__global__ void rebalance_walk_kernel(const uint4* link, const uint2* leaf_link, const uint32_t* bin_size, uint32_t n, int cap, uint32_t* leaf_at_pos,
                                      uint32_t* inner_at_gap, uint2* rb_range, uint32_t* rb_gap, uint32_t* error) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2u * n - 1u) return;
    const bool leaf = t < n;
    const uint32_t x = leaf ? t : t - n;
    const uint32_t u0 = leaf ? leaf_link[x].x : x;      // first inner node of the chain to the root
    if (!leaf) rb_range[x] = make_uint2(0u, 0u);
    int depth = 0;                                       // of u0
    uint32_t cur = u0;
    for (; depth < kMaxBinaryWalk; depth++) {
        if (cur >= n - 1u) { atomicExch(error, 1u); return; }
        const uint32_t p = link[cur].x;
        if (p == kNoNode) break;
        cur = p;
    }
    if (depth >= kMaxBinaryWalk) { atomicExch(error, 1u); return; }
    // second walk: `acc` = first position of x relative to the first leaf of `cur`'s subtree
    uint32_t acc = leaf ? leaf_link[x].y : 0u, r = kNoNode, rel = 0u;
    cur = u0;
    for (int d = depth; d >= 0; d--) {
        const uint4 L = link[cur];
        const int allowance = cap - d, h = (int)(L.y & 0xFFFFu), need = (int)(L.y >> 16);
        if (h <= allowance) r = kNoNode;                 // kept whole, with everything below
        else if (need > allowance) { r = cur; rel = acc; }
        acc += L.z;
        cur = L.x;
    }
    if (r == kNoNode) return;
    if (leaf) { if (acc < n) leaf_at_pos[acc] = x; return; }
    const uint32_t gap = acc + link[x].w - 1u;
    if (gap >= n - 1u) { atomicExch(error, 1u); return; }
    inner_at_gap[gap] = x;
    rb_range[x] = make_uint2(acc - rel, bin_size[r]);
    rb_gap[x] = gap | (r == x ? 0x80000000u : 0u);
}

// The node of the median tree over the positions [lo, hi) (hi - lo >= 2) splits behind position lo + ceil((hi - lo) / 2) - 1.
__device__ __forceinline__ uint32_t median_gap(uint32_t lo, uint32_t hi) { return lo + ((hi - lo + 1u) >> 1) - 1u; }
__device__ __forceinline__ int median_child(uint32_t lo, uint32_t hi, const uint32_t* leaf_at_pos, const uint32_t* inner_at_gap) {
    return hi - lo == 1u ? ~(int)leaf_at_pos[lo] : (int)inner_at_gap[median_gap(lo, hi)];
}

// stat: [0] root id (rewritten if the root's subtree is rebuilt), [1] subtrees rebuilt, [2] primitives in them, [4] error flag
__global__ void rebalance_rebuild_kernel(const uint4* link, const uint2* rb_range, const uint32_t* rb_gap, const uint32_t* leaf_at_pos,
                                         const uint32_t* inner_at_gap, uint32_t n, int2* children, uint32_t* stat) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x + 1u >= n) return;
    const uint2 R = rb_range[x];
    if (R.y < 2u || (uint64_t)R.x + R.y > n) return;
    const uint32_t g = rb_gap[x] & 0x7FFFFFFFu;
    uint32_t lo = R.x, hi = R.x + R.y;
    for (int i = 0; i < 64 && hi - lo >= 2u; i++) {
        const uint32_t m = median_gap(lo, hi);
        if (g == m) break;
        if (g < m) hi = m + 1u; else lo = m + 1u;
    }
    if (hi - lo < 2u || median_gap(lo, hi) != g) return;      // cannot happen: every gap of the range is some node's split
    const uint32_t mid = g + 1u;
    const int2 ch = make_int2(median_child(lo, mid, leaf_at_pos, inner_at_gap), median_child(mid, hi, leaf_at_pos, inner_at_gap));
    if (!binary_ref_ok(ch.x, n) || !binary_ref_ok(ch.y, n)) { atomicExch(stat + 4, 1u); return; }
    children[x] = ch;
    if (rb_gap[x] & 0x80000000u) {                             // the subtree's old root: hand the new one to the parent
        const uint32_t top = inner_at_gap[median_gap(R.x, R.x + R.y)];
        const uint4 L = link[x];
        if (top + 1u >= n || (L.x != kNoNode && L.x + 1u >= n)) { atomicExch(stat + 4, 1u); return; }
        if (L.x == kNoNode) stat[0] = top;
        else ((int*)children)[2 * (size_t)L.x + (L.z ? 1 : 0)] = (int)top;
        atomicAdd(stat + 1, 1u);
        atomicAdd(stat + 2, R.y);
    }
}

__global__ void rebalance_parents_kernel(const int2* children, uint32_t n, const uint32_t* root, uint32_t* parent_of_inner, uint32_t* parent_of_leaf) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u + 1u >= n) return;
    const int2 ch = children[u];
    if (!binary_ref_ok(ch.x, n) || !binary_ref_ok(ch.y, n)) return;
    if (ch.x >= 0) parent_of_inner[ch.x] = u; else parent_of_leaf[~ch.x] = u;
    if (ch.y >= 0) parent_of_inner[ch.y] = u; else parent_of_leaf[~ch.y] = u;
    if (u == *root) parent_of_inner[u] = kNoNode;
}

// stat[3] = walk height of the rewritten tree
__global__ void rebalance_finish_kernel(const uint32_t* bin_height, uint32_t n, uint32_t* stat) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    stat[3] = stat[0] + 1u < n ? bin_height[stat[0]] : kNoNode;
}

// One thread per 4-wide node of the current level. counters: [0] = nodes allocated, [1] = max stack, [2] = overflow flag.
// Leaf slots: a node owns the slot range [first_of_node, first_of_node + size) of the leaf-order arrays; its children take
// consecutive sub-ranges in child order, and the triangles of a leaf child get their slots here (slot_of_sorted), so the
// binary tree's subtrees need not be contiguous in Morton order (they are for the radix tree, not for PLOC).
__global__ void lbvh_collapse_kernel(uint32_t* nodes, uint32_t level_first, uint32_t level_count, uint32_t node_cap, int* bin_of_node, uint32_t* budget_of_node,
                                     uint32_t* prefix_of_node, uint32_t* first_of_node, const int2* children, const uint32_t* bin_size, const float* bin_box,
                                     const uint32_t* bin_height, uint32_t* slot_of_sorted, uint32_t* counters) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= level_count) return;
    lbvh_collapse_node(nodes, level_first + t, node_cap, bin_of_node, budget_of_node, prefix_of_node, first_of_node, children, bin_size, bin_box, bin_height,
                       slot_of_sorted, counters);
}

// Leaf-order records of one triangle (by sorted index): its slot was assigned by the collapse.
__global__ void lbvh_leaves_kernel(const float4* W, const float4* cent, const uint32_t* sorted_gid, const uint32_t* slot_of_sorted, uint32_t n_tris,
                                   const SrMeshInfo* meshes, const FlatInstance* instances, float4* tris, float4* shade, float4* shade_tex, uint32_t* slot_of_gid) {
    const uint32_t s_idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (s_idx >= n_tris) return;
    const uint32_t slot = slot_of_sorted[s_idx];
    const uint32_t gid = sorted_gid[s_idx];
    for (int k = 0; k < 3; k++) tris[(size_t)slot * 3 + k] = W[(size_t)gid * 3 + k];
    slot_of_gid[gid] = slot;
    const uint32_t ii = __float_as_uint(cent[gid].w);
    const FlatInstance inst = instances[ii];
    const SrVertex* v[3];
    triangle_vertices(meshes, inst, gid - inst.tri_offset, v);
    write_shade(shade + (size_t)slot * 3, v, __uint_as_float(ii), __uint_as_float(inst.mesh_slot), 0.0f);
    if (shade_tex) write_shade_tex(shade_tex + (size_t)slot * 6, v);
}

// ---------------------------------------------------------------------------------------------------------------
// PLOC (parallel locally-ordered clustering, Meister & Bittner 2018) as the topology of the fast build: bottom-up
// agglomeration of the Morton-ordered clusters. Every iteration each cluster finds, among its `radius` neighbours on
// either side, the one whose union with it has the smallest surface area; mutual nearest neighbours merge into a binary
// node (box, size and binary-walk height are known at once), the survivors are compacted in order, until one is left.
// Build quality is close to the top-down SAH build at a small multiple of the radix tree's cost.
// ---------------------------------------------------------------------------------------------------------------

template <class Prims>
__global__ void ploc_init_kernel(const Prims prims, const uint32_t* sorted_gid, uint32_t n, int* cid, float* cbox) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ploc_init_one(prims, sorted_gid, i, cid, cbox);
}

// SPREAD_TIES (instance boxes): among candidates of equal area the nearest one in the order wins, and of the two at the same
// distance the partner i ^ 1. The rule is symmetric in (i, j), so the best pair overall is still mutual and every iteration
// merges; coincident boxes then pair up (0,1), (2,3), ... and halve each iteration instead of merging one pair at a time.
template <bool SPREAD_TIES>
__global__ void ploc_nn_kernel(const float* cbox, uint32_t m, uint32_t radius, uint32_t* nn) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    nn[i] = ploc_nn_one<SPREAD_TIES>(cbox, m, radius, i);
}

// Mutual nearest neighbours merge (the lower index keeps the merged cluster, the higher one is dropped).
__global__ void ploc_merge_kernel(const uint32_t* nn, uint32_t m, int* cid, float* cbox, uint32_t* valid, int2* children, float* bin_box, uint32_t* bin_size,
                                  uint32_t* bin_height, uint32_t* node_counter) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    ploc_merge_one(nn, i, cid, cbox, valid, children, bin_box, bin_size, bin_height, node_counter);
}

__global__ void ploc_compact_kernel(const int* cid, const float* cbox, const uint32_t* valid, const uint32_t* pos, uint32_t m, int* cid_out, float* cbox_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !valid[i]) return;
    ploc_compact_one(cid, cbox, i, pos[i], cid_out, cbox_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Top level of the two-level form on the device (the reference rebuilds its TLAS on the GPU every frame, tlas.rs:155-191):
//   records    one thread per instance: the DevTlInstance record and the padded world box, by the function the host loop
//              (api.cpp two_level_build) calls as well: tl_record.h holds the one definition of that arithmetic
//   tree       the builder above over the boxes instead of triangles: Morton code of the box centre (instances without a
//              box sort behind all others and stay out of the tree), radix tree or PLOC, fit, collapse, tl_inst, refit
// ---------------------------------------------------------------------------------------------------------------
// result: [0] instances this path cannot take (the host would bake them, or the box is not finite), [1] deepest mesh-tree stack
// among the instances with a box, [2] instances with a box
__global__ void tl_records_kernel(const FlatInstance* instances, const TlMeshRow* meshes, uint32_t n_inst, double max_condition, DevTlInstance* recs,
                                  float* boxes, uint32_t* result) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0, stack = 0, has_box = 0;
    if (i < n_inst) {
        const FlatInstance in = instances[i];
        const TlMeshRow b = meshes[in.mesh_slot];
        const float* M = in.o2w;
        DevTlInstance r;
        for (int k = 0; k < 12; k++) { r.w2o[k] = 0.0f; r.o2w[k] = M[k]; }
        r.blas_root = 0u; r.tri_offset = in.tri_offset; r.pad_a = 0.0f; r.pad_b = 0.0f;
        r.mesh_slot = in.mesh_slot; r.prim_base = 0u; r.flags = 0u; r._pad = 0u;
        float bx[6];
        for (int k = 0; k < 6; k++) bx[k] = __uint_as_float(0x7FC00000u);
        TlRecordResult res = kTlRecordOk;
        if (b.n_tris != 0u) {
            res = tl_record(M, b.lo, b.hi, b.max_abs_vertex, b.max_edge_sum, max_condition, r.w2o, bx, bx + 3, &r.pad_a, &r.pad_b);
            if (res == kTlRecordOk) { has_box = 1u; stack = b.max_stack; } else bad = 1u;
        }
        if (res != kTlRecordBaked) { r.blas_root = b.blas_root; r.prim_base = b.prim_base; }      // the host gives a baked instance a copy of its mesh
        recs[i] = r;
        for (int k = 0; k < 6; k++) boxes[(size_t)i * 6 + k] = bx[k];
    }
    for (int o = 32; o > 0; o >>= 1) { bad += __shfl_xor(bad, o); has_box += __shfl_xor(has_box, o); stack = max(stack, __shfl_xor(stack, o)); }
    if ((threadIdx.x & 63) == 0) {
        if (bad) atomicAdd(result + 0, bad);
        if (stack) atomicMax(result + 1, stack);
        if (has_box) atomicAdd(result + 2, has_box);
    }
}

__global__ void tl_bounds_kernel(const float* boxes, uint32_t n, uint32_t* bounds_enc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) BoxPrims{boxes, nullptr}.add(i, lo, hi);            // fminf / fmaxf drop the NaN rows
    for (int a = 0; a < 3; a++) {
        float l = lo[a], h = hi[a];
        for (int o = 32; o > 0; o >>= 1) { l = fminf(l, __shfl_xor(l, o)); h = fmaxf(h, __shfl_xor(h, o)); }
        if ((threadIdx.x & 63) == 0) {
            if (l <= h) { atomicMin(bounds_enc + a, enc_f(l)); atomicMax(bounds_enc + 3 + a, enc_f(h)); }
        }
    }
}

// Centre of the box as the host's build_bvh_boxes takes it; an instance without a box gets the largest key.
__global__ void tl_morton_kernel(const float* boxes, const uint32_t* bounds_enc, uint32_t n, unsigned long long* keys, uint32_t* vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* b = boxes + (size_t)i * 6;
    unsigned long long key = 0xFFFFFFFFFFFFFFFFull;
    if (b[0] <= b[3]) {
        uint32_t q[3];
        for (int a = 0; a < 3; a++) {
            const float lo = dec_f(bounds_enc[a]), hi = dec_f(bounds_enc[3 + a]);
            const float ext = hi - lo;
            float t = ext > 0.0f ? ((0.5f * b[a] + 0.5f * b[3 + a]) - lo) / ext : 0.0f;
            t = fminf(fmaxf(t, 0.0f), 1.0f);
            q[a] = min((uint32_t)(t * 2097152.0f), 2097151u);
        }
        key = spread21(q[0]) | (spread21(q[1]) << 1) | (spread21(q[2]) << 2);
    }
    keys[i] = key;
    vals[i] = i;
}

// Leaf order -> instance index (the slot was assigned by the collapse).
__global__ void tl_leaves_kernel(const uint32_t* sorted_gid, const uint32_t* slot_of_sorted, uint32_t n, uint32_t* tl_inst) {
    const uint32_t s_idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (s_idx >= n) return;
    tl_inst[slot_of_sorted[s_idx]] = sorted_gid[s_idx];
}

// ---------------------------------------------------------------------------------------------------------------
// Refit of the mesh trees of the two-level form after sr_scene_update_mesh (Blas::update, blas.rs:292-310, for a BLAS built
// with ALLOW_UPDATE). Topology, leaf order and slot_of_prim stay; what follows from the vertices is rewritten in place:
//   records    one thread per leaf-order slot of the dirty meshes (every mesh's thread range starts at a multiple of 64, so a
//              wave works on one mesh): the slot keeps its primitive, the (v0, v1, v2, prim) record, `shade` and, for a textured
//              mesh, `shade_tex` get the bytes build_blas writes; the mesh's root box and padding numbers are reduced in the
//              wave and leave it as one atomic per value on the order-preserving encoding
//   finish     one thread per dirty mesh: the eight floats go into the mesh's TlMeshRow and into the read-back block
//   refit      refit_level_kernel over VertPrims, one launch per level for all dirty meshes together
// ---------------------------------------------------------------------------------------------------------------
__global__ void blas_records_kernel(const BlasRefitMesh* meshes, uint32_t n_meshes, uint32_t n_threads, float4* tris, float4* shade, float4* shade_tex,
                                    uint32_t* acc) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lo_m = 0, hi_m = n_meshes;       // last mesh whose first_thread <= t (wave-uniform: ranges start at multiples of 64)
    while (hi_m - lo_m > 1) { const uint32_t mid = (lo_m + hi_m) >> 1; if (meshes[mid].first_thread <= t) lo_m = mid; else hi_m = mid; }
    const BlasRefitMesh m = meshes[lo_m];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float max_abs = 0.0f, max_edge = 0.0f;
    const uint32_t local = t - m.first_thread;
    if (t < n_threads && local < m.n_tris) {
        const size_t slot = (size_t)m.tri_base + local;
        const uint32_t prim = __float_as_uint(tris[slot * 3 + 2].y);
        if (prim < m.n_tris) {                 // always, for records build_blas wrote; never index out of bounds
            const uint32_t* idx = (const uint32_t*)(uintptr_t)m.indices;
            const SrVertex* vtx = (const SrVertex*)(uintptr_t)m.vertices;
            const SrVertex* v[3];
            for (int j = 0; j < 3; j++) { const uint32_t vi = idx[3 * (size_t)prim + j]; v[j] = vtx + (vi < m.n_vertices ? vi : 0u); }
            const float* w[3] = {v[0]->position, v[1]->position, v[2]->position};
            tris[slot * 3 + 0] = make_float4(w[0][0], w[0][1], w[0][2], w[1][0]);
            tris[slot * 3 + 1] = make_float4(w[1][1], w[1][2], w[2][0], w[2][1]);
            tris[slot * 3 + 2] = make_float4(w[2][2], __uint_as_float(prim), 0.0f, 0.0f);
            const float4 tail = shade[slot * 3 + 2];
            write_shade(shade + slot * 3, v, tail.y, tail.z, tail.w);
            if (m.textured && shade_tex) write_shade_tex(shade_tex + slot * 6, v);
            for (int a = 0; a < 3; a++) {      // build_blas: the padded triangle box and the two padding numbers
                const float e1 = w[1][a] - w[0][a], e2 = w[2][a] - w[0][a];
                max_edge = fmaxf(max_edge, fabsf(e1) + fabsf(e2));
                for (int j = 0; j < 3; j++) max_abs = fmaxf(max_abs, fabsf(w[j][a]));
                const float pad = 4e-6f * (fabsf(e1) + fabsf(e2));
                const float l = fminf(w[0][a], fminf(w[1][a], w[2][a])) - pad;
                const float h = fmaxf(w[0][a], fmaxf(w[1][a], w[2][a])) + pad;
                lo[a] = nextafterf(l, -INFINITY); hi[a] = nextafterf(h, INFINITY);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o)); }
        max_abs = fmaxf(max_abs, __shfl_xor(max_abs, o)); max_edge = fmaxf(max_edge, __shfl_xor(max_edge, o));
    }
    if ((threadIdx.x & 63) == 0 && t < n_threads && lo[0] <= hi[0]) {
        uint32_t* q = acc + (size_t)lo_m * 8;
        for (int a = 0; a < 3; a++) { atomicMin(q + a, enc_f(lo[a])); atomicMax(q + 3 + a, enc_f(hi[a])); }
        atomicMax(q + 6, enc_f(max_abs)); atomicMax(q + 7, enc_f(max_edge));
    }
}

__global__ void blas_finish_kernel(const BlasRefitMesh* meshes, uint32_t n_meshes, const uint32_t* acc, TlMeshRow* rows, float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_meshes) return;
    float f[8];
    for (int k = 0; k < 8; k++) f[k] = dec_f(acc[(size_t)i * 8 + k]);
    for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = f[k];
    if (rows) {
        TlMeshRow* r = rows + meshes[i].mesh_slot;
        for (int a = 0; a < 3; a++) { r->lo[a] = f[a]; r->hi[a] = f[3 + a]; }
        r->max_abs_vertex = f[6]; r->max_edge_sum = f[7];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// FastBuild of ONE mesh's tree of the two-level form on the device (Blas::rebuild, blas.rs:285-310): the builder above over
// the mesh's object-space triangles, written into the mesh's ranges of the concatenated arrays.
//   prims      one thread per primitive: the (v0, v1, v2, prim) record straight from the positions (the vertex's bits: no
//              identity transform, which would turn -0.0 into +0.0), the centroid of its padded box, the bounds of the Morton
//              grid, and the mesh's root box and padding numbers by blas_records_kernel's expressions and encoding
//   tree       sort, radix tree or PLOC, collapse: unchanged, with references local to the mesh (nodes from the range's start)
//   leaves     one thread per sorted primitive: record, shade, shade_tex at tri_base + slot, primitive -> slot (global)
//   place      one thread per built node: references become global as BlasCat::append (api.cpp) makes them
//   refit      refit_level_kernel over VertPrims on the global arrays, deepest level first
//   finish     the eight floats, stack need, root and node count into the mesh's TlMeshRow and the read-back block
// ---------------------------------------------------------------------------------------------------------------
__global__ void blas_prims_kernel(const SrVertex* vtx, const uint32_t* idx, uint32_t n_vertices, uint32_t n_tris, float4* W, float4* cent,
                                  uint32_t* bounds_enc, uint32_t* acc) {
    const uint32_t prim = blockIdx.x * blockDim.x + threadIdx.x;
    BlasPrimAcc r;
    if (prim < n_tris) blas_prim_one(vtx, idx, n_vertices, prim, W, cent, r);
    blas_prims_reduce(r, bounds_enc, acc);
}

__global__ void blas_leaves_kernel(const float4* W, const uint32_t* sorted_gid, const uint32_t* slot_of_sorted, uint32_t n_tris, const SrVertex* vtx,
                                   const uint32_t* idx, uint32_t n_vertices, uint32_t mesh_slot, uint32_t tri_base, float4* tris, float4* shade,
                                   float4* shade_tex, uint32_t* slot_of_gid) {
    const uint32_t s_idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (s_idx >= n_tris) return;
    blas_leaf_one(W, sorted_gid, slot_of_sorted, s_idx, n_tris, vtx, idx, n_vertices, mesh_slot, tri_base, tris, shade, shade_tex, slot_of_gid);
}

__global__ void blas_place_kernel(uint32_t* nodes, uint32_t n_nodes, uint32_t node_base, uint32_t tri_base) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    blas_place_node(nodes + ((size_t)node_base + i) * srl::kNodeDwords + srl::kChildOffset, node_base, tri_base);
}

// counters: the collapse's ([0] nodes allocated, [1] max stack). out: 8 floats, then node count and stack need as dwords.
__global__ void blas_build_finish_kernel(const uint32_t* acc, const uint32_t* counters, uint32_t mesh_slot, uint32_t node_base, uint32_t tri_base,
                                         uint32_t n_tris, TlMeshRow* rows, uint32_t* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    blas_build_finish(acc, counters, mesh_slot, node_base, tri_base, n_tris, rows, out);
}

// sr_scene_update_mesh_device's validation: the lowest vertex whose position is not finite under the host's rule (std::isfinite
// of x, y and z; normals, tangents, uv sets and pad words are free), as the exponent-bits test on the raw words. The source is
// read once as 16-byte pieces, six per 96-byte vertex, consecutive lanes on consecutive pieces (coalesced dwordx4); the lane
// whose piece opens a vertex tests its first three words. The grid is a multiple of three blocks of 256, so the stride is a
// multiple of six pieces: a thread keeps its place inside the vertex over the whole loop and its vertex index advances by a
// constant. Piece indices are 64-bit (n_vertices * 6 need not fit 32). Every lane keeps its own minimum, the wave reduces once
// after the loop (report_first_bad, vertex_tile.h).
constexpr uint32_t kVertexCheckBlock = 256, kVertexCheckMaxBlocks = 2046;     // about eight blocks per CU; a multiple of three
static_assert(sizeof(SrVertex) == 96 && offsetof(SrVertex, position) == 0 && (kVertexCheckBlock * 3) % kVertexPieces == 0 && kVertexCheckMaxBlocks % 3 == 0,
              "vertex_check_kernel: six pieces per vertex, the position in the first, a stride of whole vertices");
__global__ void __launch_bounds__(kVertexCheckBlock) vertex_check_kernel(const uint4* pieces, uint64_t n_pieces, uint32_t* first_bad) {
    const uint32_t t = blockIdx.x * kVertexCheckBlock + threadIdx.x;          // < 2046 * 256
    const uint32_t stride = gridDim.x * kVertexCheckBlock, v_step = stride / kVertexPieces;
    const uint32_t exponent = t % kVertexPieces == 0 ? 0x7F800000u : 0u;      // a piece inside a vertex never matches: no branch in the loop
    uint32_t v = t / kVertexPieces, bad = 0xFFFFFFFFu;
    for (uint64_t p = t; p < n_pieces; p += stride, v += v_step) {
        const uint4 w = pieces[p];
        const bool hit = ((w.x & exponent) == 0x7F800000u) | ((w.y & exponent) == 0x7F800000u) | ((w.z & exponent) == 0x7F800000u);
        bad = hit ? min(bad, v) : bad;
    }
    report_first_bad(bad, first_bad);
}

}  // namespace srd

using namespace srd;

int srk_vertex_check(const SrVertex* vertices, uint32_t n_vertices, uint32_t* first_bad, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(first_bad, 0xFF, 4, stream);
    if (e != hipSuccess) return (int)e;
    if (n_vertices == 0) return 0;
    const uint64_t n_pieces = (uint64_t)n_vertices * kVertexPieces;
    const uint64_t want = (n_pieces + kVertexCheckBlock - 1) / kVertexCheckBlock;
    const uint32_t blocks = want >= kVertexCheckMaxBlocks ? kVertexCheckMaxBlocks : (uint32_t)((want + 2) / 3 * 3);
    vertex_check_kernel<<<dim3(blocks), dim3(kVertexCheckBlock), 0, stream>>>((const uint4*)vertices, n_pieces, first_bad);
    return (int)hipGetLastError();
}

int srk_launch_flatten_slots(float4* tris, const float4* shade, const SrMeshInfo* meshes, const FlatInstance* instances, uint32_t n_tris, hipStream_t stream) {
    if (n_tris == 0) return 0;
    flatten_slots_kernel<false, false><<<dim3((n_tris + 255) / 256), dim3(256), 0, stream>>>(tris, shade, meshes, instances, n_tris, nullptr);
    return (int)hipGetLastError();
}

int srk_launch_flatten_reshade(float4* tris, float4* shade, float4* shade_tex, const SrMeshInfo* meshes, const FlatInstance* instances, uint32_t n_tris,
                               hipStream_t stream) {
    if (n_tris == 0) return 0;
    const dim3 grid((n_tris + 255) / 256), block(256);
    if (shade_tex) flatten_slots_kernel<true, true><<<grid, block, 0, stream>>>(tris, shade, meshes, instances, n_tris, shade_tex);
    else flatten_slots_kernel<true, false><<<grid, block, 0, stream>>>(tris, shade, meshes, instances, n_tris, nullptr);
    return (int)hipGetLastError();
}

// One launch per tree level, deepest level first. level(l) -> (first, count) of level l in that order: a range of the list
// `level_nodes`, or of the node indices themselves where the list is null.
template <class Prims, class Level>
static void refit_levels(uint32_t* nodes, const Prims prims, float* node_box, const uint32_t* level_nodes, uint32_t n_levels, Level level, hipStream_t stream) {
    for (uint32_t l = 0; l < n_levels; l++) {
        const std::pair<uint32_t, uint32_t> r = level(l);
        if (r.second == 0) continue;
        refit_level_kernel<<<dim3((r.second + 63) / 64), dim3(64), 0, stream>>>(nodes, prims, node_box, level_nodes, r.first, r.second);
    }
}
template <class Prims>      // level_offsets_host[l] .. [l+1]: deepest level first (srk_blas_refit: all dirty meshes together)
static int refit_listed_levels(uint32_t* nodes, const Prims prims, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host,
                               uint32_t n_levels, hipStream_t stream) {
    refit_levels(nodes, prims, node_box, level_nodes, n_levels,
                 [&](uint32_t l) { return std::make_pair(level_offsets_host[l], level_offsets_host[l + 1] - level_offsets_host[l]); }, stream);
    return (int)hipGetLastError();
}
int srk_launch_refit(uint32_t* nodes, const float4* tris, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host,
                     uint32_t n_levels, hipStream_t stream) {
    return refit_listed_levels(nodes, TriPrims{tris}, node_box, level_nodes, level_offsets_host, n_levels, stream);
}
int srk_blas_refit(uint32_t* nodes, const float4* tris, float* node_box, const uint32_t* level_nodes, const uint32_t* level_offsets_host, uint32_t n_levels,
                   hipStream_t stream) {
    return refit_listed_levels(nodes, VertPrims{tris}, node_box, level_nodes, level_offsets_host, n_levels, stream);
}

int srk_blas_records(const BlasRefitMesh* meshes, uint32_t n_meshes, uint32_t n_threads, float4* tris, float4* shade, float4* shade_tex, uint32_t* acc,
                     const uint32_t* acc_init, TlMeshRow* rows, float* out, hipStream_t stream) {
    if (n_meshes == 0 || n_threads == 0) return 0;
    hipError_t e = hipMemcpyAsync(acc, acc_init, (size_t)n_meshes * 32, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return (int)e;
    blas_records_kernel<<<dim3((n_threads + 255) / 256), dim3(256), 0, stream>>>(meshes, n_meshes, n_threads, tris, shade, shade_tex, acc);
    blas_finish_kernel<<<dim3((n_meshes + 63) / 64), dim3(64), 0, stream>>>(meshes, n_meshes, acc, rows, out);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// The device tree build. All outputs are device buffers owned by the caller; `scratch` is reused across builds. Three kinds of
// primitive go through the same stages (build_tree):
//   TrisBuildArgs   the instances' world-space triangles (srk_lbvh_build)
//   BoxesBuildArgs  the instance boxes of a top-level tree (srk_tl_build): all n_instances rows are keyed and sorted, the n_boxes
//                   real ones come first and are the tree's primitives
//   MeshBuildArgs   the object-space triangles of one mesh of the two-level form (srk_blas_build); nodes and records go to the
//                   mesh's ranges of the concatenated arrays (node_base, tri_base), with global references
// ---------------------------------------------------------------------------------------------------------------
enum { kBuildTris = 0, kBuildBoxes = 1, kBuildMesh = 2 };
template <class Args>
constexpr int kind_of = std::is_same<Args, BoxesBuildArgs>::value ? kBuildBoxes : std::is_same<Args, MeshBuildArgs>::value ? kBuildMesh : kBuildTris;

// The words of the scratch that kernels reduce and count in. Every wave of blas_prims_kernel reduces into `bounds` and into `acc`:
// the two sit in cache lines of their own (in one line the atomics of a 1M-triangle mesh cost its build 0.7 ms of 17).
struct TreeSmall {
    uint32_t bounds[6];                   // Morton grid: lo, hi, encoded
    alignas(32) uint32_t counters[3];     // the collapse's: nodes allocated (the root is), max stack, overflow flag
    alignas(16) uint32_t ploc_nodes;      // binary nodes PLOC allocated
    alignas(64) uint32_t acc[8];          // srk_blas_build: the mesh's root box lo, hi, max_abs_vertex, max_edge_sum, encoded
    alignas(64) uint32_t stat[5];         // the height bound's (rebalance_rebuild_kernel); set when the pass runs, not by the seed
};
static TreeSmall small_seed() {
    TreeSmall s{};
    for (int k = 0; k < 3; k++) s.bounds[k] = 0xFFFFFFFFu;
    s.counters[0] = 1u;
    for (int k = 0; k < 8; k++) s.acc[k] = mesh_acc_seed(k);
    return s;
}
static const TreeSmall kSmallSeed = small_seed();

// Every array of the builder's scratch. carve_tree_scratch is the one definition of the layout: build_tree carves the caller's
// buffer with it, the srk_*_scratch_bytes functions return its end for a null base.
struct TreeScratch {
    uint32_t n_keys, n;                                  // sorted items; primitives of the tree
    float4 *W, *cent;                                    // records and centroids of the triangles (null for boxes)
    unsigned long long *keys_a, *keys_b; uint32_t *vals_a, *vals_b;      // the sort's input and output
    int2* children; uint2* range;                        // range: radix tree only; PLOC: nn | valid
    uint32_t *parent_inner, *parent_leaf;                // radix tree and height bound; parent_inner under PLOC: scan output
    float* bin_box; uint32_t *bin_height, *bin_size, *flags, *slot_of_sorted;
    int* bin_of_node; uint32_t *budget_of_node, *prefix_of_node, *first_of_node;      // the collapse's queues, by 4-wide node
    TreeSmall* small;
    int* cid[2]; float* cbox[2];                         // PLOC clusters, double-buffered (null without PLOC)
    uint4* link; uint2* leaf_link; uint32_t *leaf_at_pos, *inner_at_gap;    // the height bound's own arrays
    uint2* rb_range; uint32_t* rb_gap;                   // ... its per-node range and gap live in the sort's input, which is dead by then
    char* tmp; size_t sort_bytes, scan_bytes;            // hipCUB's temporary storage, shared by the sort and PLOC's scan
};
static size_t carve_tree_scratch(void* base, int kind, uint32_t n_keys, uint32_t n, uint32_t node_cap, bool ploc, size_t sort_bytes, size_t scan_bytes,
                                 TreeScratch* s) {
    size_t off = 0;      // consecutive 256-byte aligned arrays; with a null base only the offsets count
    auto take = [&](auto** p, size_t count) { *p = (std::remove_reference_t<decltype(**p)>*)((uintptr_t)base + off); off += (count * sizeof(**p) + 255) & ~(size_t)255; };
    s->n_keys = n_keys; s->n = n;
    s->W = s->cent = nullptr;
    if (kind != kBuildBoxes) { take(&s->W, (size_t)n * 3); take(&s->cent, n); }
    take(&s->keys_a, n_keys); take(&s->keys_b, n_keys); take(&s->vals_a, n_keys); take(&s->vals_b, n_keys);
    take(&s->children, n); take(&s->range, n); take(&s->parent_inner, n); take(&s->parent_leaf, n);
    take(&s->bin_box, (size_t)n * 6); take(&s->bin_height, n); take(&s->bin_size, n); take(&s->flags, n); take(&s->slot_of_sorted, n);
    take(&s->bin_of_node, node_cap); take(&s->budget_of_node, node_cap); take(&s->prefix_of_node, node_cap); take(&s->first_of_node, node_cap);
    take(&s->small, 1);
    for (int k = 0; k < 2; k++) { s->cid[k] = nullptr; s->cbox[k] = nullptr; if (ploc) { take(&s->cid[k], n); take(&s->cbox[k], (size_t)n * 6); } }
    take(&s->link, n); take(&s->leaf_link, n); take(&s->leaf_at_pos, n); take(&s->inner_at_gap, n);
    s->rb_range = (uint2*)s->keys_a; s->rb_gap = s->vals_a;
    s->sort_bytes = sort_bytes; s->scan_bytes = scan_bytes;
    take(&s->tmp, sort_bytes > scan_bytes ? sort_bytes : scan_bytes);
    return off;
}
// The key of an instance without a box has every bit set; a Morton code has 63.
static hipError_t tree_temp_bytes(int kind, uint32_t n_keys, uint32_t n, bool ploc, size_t* sort_bytes, size_t* scan_bytes, hipStream_t stream) {
    *sort_bytes = *scan_bytes = 0;
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, *sort_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                            (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n_keys, 0, kind == kBuildBoxes ? 64 : 63, stream);
    if (e != hipSuccess || !ploc) return e;
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, stream);
}
static size_t tree_scratch_bytes(int kind, uint32_t n_keys, uint32_t n, uint32_t node_cap, int ploc) {
    size_t sort_bytes, scan_bytes;
    (void)tree_temp_bytes(kind, n_keys, n, ploc != 0, &sort_bytes, &scan_bytes, nullptr);     // a failure shows in the build, which asks again
    TreeScratch s;
    return carve_tree_scratch(nullptr, kind, n_keys, n, node_cap, ploc != 0, sort_bytes, scan_bytes, &s);
}
size_t srk_lbvh_scratch_bytes(uint32_t n_tris, uint32_t node_cap, int ploc) { return tree_scratch_bytes(kBuildTris, n_tris, n_tris, node_cap, ploc); }
size_t srk_tl_scratch_bytes(uint32_t n_instances, uint32_t n_boxes, uint32_t node_cap, int ploc) {
    return tree_scratch_bytes(kBuildBoxes, n_instances, n_boxes, node_cap, ploc);
}

#define TREE_TRY(call) do { const int rc_ = (int)(call); if (rc_ != 0) return rc_; } while (0)

// "Copy these words to the host and wait": every value the host steers the build by comes through here.
struct HostCopy { void* dst; const void* src; size_t bytes; };
static hipError_t read_back(hipStream_t stream, std::initializer_list<HostCopy> copies) {
    for (const HostCopy& c : copies)
        if (const hipError_t e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream); e != hipSuccess) return e;
    return hipStreamSynchronize(stream);
}

static const dim3 kBuildBlock(256);
static dim3 build_grid(uint32_t n) { return dim3((n + 255) / 256); }

// What a stage bounds a primitive by: prims_of by sorted value (triangle id / instance index), leaf_prims_of by leaf position.
static TriPrims prims_of(const TrisBuildArgs&, const TreeScratch& s) { return TriPrims{s.W}; }
static BoxPrims prims_of(const BoxesBuildArgs& a, const TreeScratch&) { return BoxPrims{a.boxes, nullptr}; }
static VertPrims prims_of(const MeshBuildArgs&, const TreeScratch& s) { return VertPrims{s.W}; }
static TriPrims leaf_prims_of(const TrisBuildArgs& a) { return TriPrims{a.tris}; }
static BoxPrims leaf_prims_of(const BoxesBuildArgs& a) { return BoxPrims{a.boxes, a.tl_inst}; }
static VertPrims leaf_prims_of(const MeshBuildArgs& a) { return VertPrims{a.arrays.tris}; }
static uint32_t node_base_of(const TreeBuildTarget&) { return 0u; }      // the collapse's node 0 in the caller's node array
static uint32_t node_base_of(const MeshBuildArgs& a) { return a.node_base; }

// ---- keys and sort: the seed of the small block, primitives (records, centroids) and the bounds of the Morton grid, keys, the sort
template <class Args>
static int stage_keys_and_sort(const Args& a, const TreeScratch& s, hipStream_t stream) {
    constexpr int KIND = kind_of<Args>;
    const dim3 gk = build_grid(s.n_keys), gt = build_grid(s.n);
    TREE_TRY(hipMemcpyAsync(s.small, &kSmallSeed, offsetof(TreeSmall, stat), hipMemcpyHostToDevice, stream));
    if constexpr (KIND == kBuildBoxes) {
        tl_bounds_kernel<<<gk, kBuildBlock, 0, stream>>>(a.boxes, s.n_keys, s.small->bounds);
        tl_morton_kernel<<<gk, kBuildBlock, 0, stream>>>(a.boxes, s.small->bounds, s.n_keys, s.keys_a, s.vals_a);
    } else {
        if constexpr (KIND == kBuildMesh) blas_prims_kernel<<<gt, kBuildBlock, 0, stream>>>(a.vertices, a.indices, a.n_vertices, s.n, s.W, s.cent, s.small->bounds, s.small->acc);
        else lbvh_prims_kernel<<<gt, kBuildBlock, 0, stream>>>(a.meshes, a.instances, a.n_instances, s.n, s.W, s.cent, s.small->bounds);
        lbvh_morton_kernel<<<gt, kBuildBlock, 0, stream>>>(s.cent, s.small->bounds, s.n, s.keys_a, s.vals_a);
    }
    size_t sort_bytes = s.sort_bytes;
    return (int)hipcub::DeviceRadixSort::SortPairs(s.tmp, sort_bytes, s.keys_a, s.keys_b, s.vals_a, s.vals_b, (int)s.n_keys, 0, KIND == kBuildBoxes ? 64 : 63, stream);
}

// ---- binary topology. One triangle (a mesh): no binary tree; the root is one node with one leaf child.
static int topology_single_triangle(uint32_t* tree_nodes, const TreeScratch& s, LbvhResult* out, hipStream_t stream) {
    uint32_t node[srl::kNodeDwords];
    for (int k = 0; k < srl::kNodeDwords; k++) node[k] = k >= srl::kChildOffset ? 0xFFFFFFFFu : 0u;
    node[srl::kChildOffset] = ~((0u << 3) | 1u);
    TREE_TRY(hipMemcpyAsync(tree_nodes, node, sizeof(node), hipMemcpyHostToDevice, stream));
    TREE_TRY(hipMemsetAsync(s.slot_of_sorted, 0, 4, stream));
    out->level_ranges.assign(1, std::make_pair(0u, 1u));
    out->n_nodes = 1; out->max_stack = 0;
    return 0;
}
template <class Prims>      // the radix tree over the sorted keys; its root is binary node 0
static int topology_radix_tree(const Prims prims, const TreeScratch& s, hipStream_t stream) {
    const dim3 gt = build_grid(s.n);
    TREE_TRY(hipMemsetAsync(s.flags, 0, (size_t)s.n * 4, stream));
    lbvh_hierarchy_kernel<<<gt, kBuildBlock, 0, stream>>>(s.keys_b, (int)s.n, s.children, s.parent_inner, s.parent_leaf, s.range);
    lbvh_fit_kernel<<<gt, kBuildBlock, 0, stream>>>(prims, s.vals_b, (int)s.n, s.children, s.parent_inner, s.parent_leaf, s.range, s.bin_box, s.bin_height, s.bin_size, s.flags);
    return 0;
}
template <bool SPREAD_TIES, class Prims>      // PLOC: one stream wait per iteration (the number of clusters left), one for the root
static int topology_ploc(const Prims prims, uint32_t radius, const TreeScratch& s, int* root_bin, hipStream_t stream) {
    uint32_t* const nn = (uint32_t*)s.range;
    uint32_t* const valid = nn + s.n;
    uint32_t* const pos = s.parent_inner;
    int* const* cid = s.cid;
    float* const* cbox = s.cbox;
    ploc_init_kernel<<<build_grid(s.n), kBuildBlock, 0, stream>>>(prims, s.vals_b, s.n, cid[0], cbox[0]);
    uint32_t m = s.n;
    int cur = 0, guard = 0;
    while (m > 1) {
        const dim3 gm = build_grid(m);
        ploc_nn_kernel<SPREAD_TIES><<<gm, kBuildBlock, 0, stream>>>(cbox[cur], m, radius, nn);
        ploc_merge_kernel<<<gm, kBuildBlock, 0, stream>>>(nn, m, cid[cur], cbox[cur], valid, s.children, s.bin_box, s.bin_size, s.bin_height, &s.small->ploc_nodes);
        size_t scan_bytes = s.scan_bytes;
        TREE_TRY(hipcub::DeviceScan::ExclusiveSum(s.tmp, scan_bytes, valid, pos, (int)m, stream));
        ploc_compact_kernel<<<gm, kBuildBlock, 0, stream>>>(cid[cur], cbox[cur], valid, pos, m, cid[cur ^ 1], cbox[cur ^ 1]);
        uint32_t tail[2];      // new count = pos[m-1] + valid[m-1]
        TREE_TRY(read_back(stream, {{&tail[0], pos + (m - 1), 4}, {&tail[1], valid + (m - 1), 4}}));
        const uint32_t m_new = tail[0] + tail[1];
        if (m_new >= m || ++guard > 4096) return -1;     // no progress: cannot happen (the closest pair is always mutual)
        m = m_new;
        cur ^= 1;
    }
    TREE_TRY(read_back(stream, {{root_bin, cid[cur], 4}}));
    return *root_bin < 0 ? -1 : 0;
}
template <class Args>
static int stage_topology(const Args& a, const TreeScratch& s, bool single, LbvhResult* out, int* root_bin, hipStream_t stream) {
    *root_bin = 0;
    if (single) return topology_single_triangle((uint32_t*)a.nodes + (size_t)node_base_of(a) * srl::kNodeDwords, s, out, stream);
    if (!a.ploc) return topology_radix_tree(prims_of(a, s), s, stream);
    return topology_ploc<kind_of<Args> == kBuildBoxes>(prims_of(a, s), (uint32_t)a.ploc, s, root_bin, stream);
}

// ---- height bound: the binary root's walk height (one stream wait); above the cap the tree is refused or, under `rebalance`,
// rewritten to fit (the pass described above rebalance_links_kernel; one more stream wait)
template <class Args>
static int stage_height_bound(const Args& a, const TreeScratch& s, int* root_bin, uint32_t* root_height, LbvhResult* out, hipStream_t stream) {
    const uint32_t n = s.n;
    TREE_TRY(read_back(stream, {{root_height, s.bin_height + *root_bin, 4}}));
    out->height_before = out->height_after = *root_height;
    if (*root_height <= a.stack_cap) return 0;
    if (!a.rebalance || median_height(n) > a.stack_cap) return -1;      // refused; no tree over n primitives fits
    const auto prims = prims_of(a, s);
    uint32_t* const stat = s.small->stat;
    uint32_t st[5] = {(uint32_t)*root_bin, 0u, 0u, 0u, 0u};
    const dim3 gt = build_grid(n), gw = build_grid(2 * n - 1);
    TREE_TRY(hipMemcpyAsync(stat, st, sizeof(st), hipMemcpyHostToDevice, stream));
    rebalance_links_kernel<<<gt, kBuildBlock, 0, stream>>>(s.children, s.bin_size, s.bin_height, n, (uint32_t)*root_bin, s.link, s.leaf_link);
    rebalance_walk_kernel<<<gw, kBuildBlock, 0, stream>>>(s.link, s.leaf_link, s.bin_size, n, (int)a.stack_cap, s.leaf_at_pos, s.inner_at_gap, s.rb_range, s.rb_gap, stat + 4);
    rebalance_rebuild_kernel<<<gt, kBuildBlock, 0, stream>>>(s.link, s.rb_range, s.rb_gap, s.leaf_at_pos, s.inner_at_gap, n, s.children, stat);
    rebalance_parents_kernel<<<gt, kBuildBlock, 0, stream>>>(s.children, n, stat, s.parent_inner, s.parent_leaf);
    TREE_TRY(hipMemsetAsync(s.flags, 0, (size_t)n * 4, stream));
    lbvh_fit_kernel<<<gt, kBuildBlock, 0, stream>>>(prims, s.vals_b, (int)n, s.children, s.parent_inner, s.parent_leaf, (const uint2*)nullptr, s.bin_box, s.bin_height, s.bin_size, s.flags);
    rebalance_finish_kernel<<<dim3(1), dim3(64), 0, stream>>>(s.bin_height, n, stat);
    TREE_TRY(hipGetLastError());
    TREE_TRY(read_back(stream, {{st, stat, sizeof(st)}}));
    if (st[4] || st[0] + 1u >= n || st[3] > a.stack_cap) return -1;     // cannot happen for a tree the topology stage finished
    *root_bin = (int)st[0]; *root_height = st[3];
    out->height_after = st[3]; out->subtrees_rebuilt = st[1]; out->prims_rebuilt = st[2];
    return 0;
}

// ---- collapse levels: the root of the 4-wide tree is the binary root, its budget the binary height, at least the regular stack
// size; then one launch and one stream wait per level (the nodes the level allocated are the next one)
static int stage_collapse(const TreeBuildTarget& a, const TreeScratch& s, uint32_t* tree_nodes, int root_bin, uint32_t root_height, LbvhResult* out,
                          hipStream_t stream) {
    const uint32_t floor = a.rebalance ? (a.stack_floor < a.stack_cap ? a.stack_floor : a.stack_cap) : a.stack_floor;
    const uint32_t budget = root_height > floor ? root_height : floor;
    const uint32_t zero = 0;
    TREE_TRY(hipMemcpyAsync(s.bin_of_node, &root_bin, 4, hipMemcpyHostToDevice, stream));
    TREE_TRY(hipMemcpyAsync(s.budget_of_node, &budget, 4, hipMemcpyHostToDevice, stream));
    TREE_TRY(hipMemcpyAsync(s.prefix_of_node, &zero, 4, hipMemcpyHostToDevice, stream));
    TREE_TRY(hipMemcpyAsync(s.first_of_node, &zero, 4, hipMemcpyHostToDevice, stream));
    out->level_ranges.clear();
    uint32_t level_first = 0, level_count = 1;
    while (level_count) {
        out->level_ranges.emplace_back(level_first, level_count);
        lbvh_collapse_kernel<<<dim3((level_count + 63) / 64), dim3(64), 0, stream>>>(tree_nodes, level_first, level_count, a.node_cap, s.bin_of_node,
                                                                                       s.budget_of_node, s.prefix_of_node, s.first_of_node, s.children, s.bin_size,
                                                                                       s.bin_box, s.bin_height, s.slot_of_sorted, s.small->counters);
        uint32_t c[3];
        TREE_TRY(read_back(stream, {{c, s.small->counters, sizeof(c)}}));
        if (c[2] || c[0] > a.node_cap) return -1;
        level_first += level_count;
        level_count = c[0] - level_first;
        out->n_nodes = c[0];
        out->max_stack = c[1];
        if (out->level_ranges.size() > 128) return -1;
    }
    return 0;
}

// ---- leaves and placing: the leaf-order outputs of the kind; a mesh's node references become global
template <class Args>
static void stage_leaves(const Args& a, const TreeScratch& s, const LbvhResult& out, hipStream_t stream) {
    constexpr int KIND = kind_of<Args>;
    const dim3 gt = build_grid(s.n);
    if constexpr (KIND == kBuildBoxes) tl_leaves_kernel<<<gt, kBuildBlock, 0, stream>>>(s.vals_b, s.slot_of_sorted, s.n, a.tl_inst);
    else if constexpr (KIND == kBuildMesh) {
        const BlasBatchArrays& A = a.arrays;
        blas_leaves_kernel<<<gt, kBuildBlock, 0, stream>>>(s.W, s.vals_b, s.slot_of_sorted, s.n, a.vertices, a.indices, a.n_vertices, a.mesh_slot, a.tri_base, A.tris,
                                                            A.shade, a.textured ? A.shade_tex : nullptr, A.slot_of_gid);
        blas_place_kernel<<<build_grid(out.n_nodes), kBuildBlock, 0, stream>>>(A.nodes, out.n_nodes, a.node_base, a.tri_base);
    } else lbvh_leaves_kernel<<<gt, kBuildBlock, 0, stream>>>(s.W, s.cent, s.vals_b, s.slot_of_sorted, s.n, a.meshes, a.instances, a.tris, a.shade, a.shade_tex, a.slot_of_gid);
}

// ---- finish: a mesh's row and read-back block; the launches' errors; the build's last stream wait
template <class Args>
static int stage_finish(const Args& a, const TreeScratch& s, hipStream_t stream) {
    if constexpr (kind_of<Args> == kBuildMesh)
        blas_build_finish_kernel<<<dim3(1), dim3(64), 0, stream>>>(s.small->acc, s.small->counters, a.mesh_slot, a.node_base, a.tri_base, s.n, a.arrays.rows, a.out);
    TREE_TRY(hipGetLastError());
    return (int)hipStreamSynchronize(stream);
}

// Launches and stream waits of one build, with I PLOC iterations (radix tree: none) and L collapse levels. Host-to-device copies:
// the small block's seed, the four words of the collapse's root. Launches: 2 (primitives, keys), the sort's, the topology's (radix
// tree: a memset and 2; PLOC: 1 + I x (3 and the scan's)), L collapses, the leaves (a mesh: and 1 placing), L refits, a mesh's
// finish. Stream waits: I + 1 under PLOC, 1 for the root height, L, and the last one: L + 2 with the radix tree, I + L + 3 with PLOC.
// A rebalanced tree adds one copy, a memset, six launches and one wait; a mesh of one triangle is two copies, a memset, three
// launches, its refit and finish, and one wait.
template <class Args>
static int build_tree(const Args& a, uint32_t n_keys, uint32_t n, LbvhResult* out, hipStream_t stream) {
    constexpr int KIND = kind_of<Args>;
    if (KIND == kBuildBoxes && (n < 2 || n > n_keys)) return -1;
    if (KIND == kBuildMesh && (n < 1 || a.node_cap < 1)) return -1;
    const uint32_t node_base = node_base_of(a);
    uint32_t* const tree_nodes = (uint32_t*)a.nodes + (size_t)node_base * srl::kNodeDwords;
    size_t sort_bytes, scan_bytes;
    TREE_TRY(tree_temp_bytes(KIND, n_keys, n, a.ploc != 0, &sort_bytes, &scan_bytes, stream));
    TreeScratch s;
    if (carve_tree_scratch(a.scratch, KIND, n_keys, n, a.node_cap, a.ploc != 0, sort_bytes, scan_bytes, &s) > a.scratch_bytes) return (int)hipErrorOutOfMemory;

    const bool single = KIND == kBuildMesh && n == 1;
    int root_bin = 0;
    uint32_t root_height = 0;
    TREE_TRY(stage_keys_and_sort(a, s, stream));
    TREE_TRY(stage_topology(a, s, single, out, &root_bin, stream));
    if (!single) {
        TREE_TRY(stage_height_bound(a, s, &root_bin, &root_height, out, stream));
        TREE_TRY(stage_collapse(a, s, tree_nodes, root_bin, root_height, out, stream));
    }
    out->max_depth = (uint32_t)out->level_ranges.size();
    stage_leaves(a, s, *out, stream);
    const std::vector<std::pair<uint32_t, uint32_t>>& levels = out->level_ranges;      // root level first, local to the tree
    refit_levels((uint32_t*)a.nodes, leaf_prims_of(a), a.node_box, nullptr, (uint32_t)levels.size(),
                 [&](uint32_t l) { const auto& r = levels[levels.size() - 1 - l]; return std::make_pair(node_base + r.first, r.second); }, stream);
    return stage_finish(a, s, stream);
}

int srk_lbvh_build(const TrisBuildArgs& a, LbvhResult* out, hipStream_t stream) { return build_tree(a, a.n_tris, a.n_tris, out, stream); }
int srk_tl_build(const BoxesBuildArgs& a, LbvhResult* out, hipStream_t stream) { return build_tree(a, a.n_instances, a.n_boxes, out, stream); }
int srk_blas_build(const MeshBuildArgs& a, LbvhResult* out, hipStream_t stream) { return build_tree(a, a.n_tris, a.n_tris, out, stream); }

int srk_tl_records(const FlatInstance* instances, const TlMeshRow* meshes, uint32_t n_instances, double max_condition, DevTlInstance* records,
                   float* boxes, uint32_t* result, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(result, 0, 12, stream);
    if (e != hipSuccess) return (int)e;
    if (n_instances == 0) return 0;
    tl_records_kernel<<<dim3((n_instances + 255) / 256), dim3(256), 0, stream>>>(instances, meshes, n_instances, max_condition, records, boxes, result);
    return (int)hipGetLastError();
}
