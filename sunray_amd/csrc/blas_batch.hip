// Batched device fast build of small mesh trees of the two-level form (sr_scene_set_mesh_tree_batch): what build_tree over MeshBuildArgs
// (bvh_gpu.hip) does with a launch per stage and a stream wait per PLOC iteration and collapse level, done for every mesh of the
// batch by ONE workgroup inside ONE launch. A mesh of at most SR_BLAS_BATCH_MAX_TRIS triangles fits one workgroup: a launch boundary
// or host read-back of the per-mesh path is a __syncthreads() here, the counters the host read back live in LDS. The arithmetic of
// every stage is the shared per-element function of bvh_device.h, so both paths build the same tree from the same sorted order
// (node numbers, which come from atomic counters in both, aside).
//   where things live   LDS: the block sort's / scan's storage, the encoded bounds and root box, the collapse and PLOC counters,
//                       status, cluster count, level table. The mesh's slab of the scratch buffer (global memory, ~300 B per
//                       triangle, written and re-read by the same compute unit, so it is served from its L1 / the L2): records,
//                       centroids, sorted keys, the binary tree, PLOC clusters, the collapse's queues and the 4-wide nodes
//                       before placing. The resident arrays are written only once the tree is known to fit.
//   no hang             every loop whose trip count comes from data (PLOC rounds, collapse levels) carries a cap and reads its
//                       condition from LDS words one thread wrote before a barrier: all threads leave it together.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include <hipcub/hipcub.hpp>

#include "blas_batch.h"
#include "bvh_device.h"
#include "bvh_gpu.h"
#include "bvh_layout.h"

namespace srd {

constexpr uint32_t kBatchMaxRounds = kBlasBatchMaxTris;      // every PLOC round merges at least one pair: fewer rounds than clusters

// The arrays of one mesh's slab. The layout is this kernel's own: defined together with the per-stage builder's (bvh_gpu.hip TreeScratch)
// it changed this kernel's register allocation (SGPR spills 32 -> 23 and 13 -> 11), so the two stay apart.
struct BatchSlab {
    float4 *W, *cent;
    unsigned long long* keys; uint32_t* vals;           // sorted
    int2* children; uint2* range;                       // range: radix tree only; PLOC: nn | valid
    uint32_t *parent_inner, *parent_leaf;
    float* bin_box; uint32_t *bin_height, *bin_size, *flags, *slot_of_sorted;
    int* bin_of_node; uint32_t *budget_of_node, *prefix_of_node, *first_of_node;
    int *cid0, *cid1; float *cbox0, *cbox1;            // PLOC clusters, double-buffered
    uint32_t* nodes;                                    // the 4-wide nodes with local references, before placing
};
__host__ __device__ inline size_t batch_carve(char* base, uint32_t n, uint32_t node_cap, BatchSlab* s) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += (bytes + 255) & ~(size_t)255; return (void*)p; };
    s->W = (float4*)take((size_t)n * 48); s->cent = (float4*)take((size_t)n * 16);
    s->keys = (unsigned long long*)take((size_t)n * 8); s->vals = (uint32_t*)take((size_t)n * 4);
    s->children = (int2*)take((size_t)n * 8); s->range = (uint2*)take((size_t)n * 8);
    s->parent_inner = (uint32_t*)take((size_t)n * 4); s->parent_leaf = (uint32_t*)take((size_t)n * 4);
    s->bin_box = (float*)take((size_t)n * 24);
    s->bin_height = (uint32_t*)take((size_t)n * 4); s->bin_size = (uint32_t*)take((size_t)n * 4);
    s->flags = (uint32_t*)take((size_t)n * 4); s->slot_of_sorted = (uint32_t*)take((size_t)n * 4);
    s->bin_of_node = (int*)take((size_t)node_cap * 4); s->budget_of_node = (uint32_t*)take((size_t)node_cap * 4);
    s->prefix_of_node = (uint32_t*)take((size_t)node_cap * 4); s->first_of_node = (uint32_t*)take((size_t)node_cap * 4);
    s->cid0 = (int*)take((size_t)n * 4); s->cbox0 = (float*)take((size_t)n * 24);
    s->cid1 = (int*)take((size_t)n * 4); s->cbox1 = (float*)take((size_t)n * 24);
    s->nodes = (uint32_t*)take((size_t)node_cap * srl::kNodeBytes);
    return off;
}

using BatchSort = hipcub::BlockRadixSort<unsigned long long, (int)kBlasBatchBlock, (int)kBlasBatchItems, uint32_t>;
using BatchScan = hipcub::BlockScan<uint32_t, (int)kBlasBatchBlock>;

struct BatchShared {
    union { typename BatchSort::TempStorage sort; typename BatchScan::TempStorage scan; } u;
    uint32_t bounds[6];          // Morton grid, encoded
    uint32_t acc[8];             // root box lo, hi, max_abs_vertex, max_edge_sum, encoded
    uint32_t counters[3];        // the collapse's: nodes allocated, max stack, overflow flag
    uint32_t ploc_nodes;         // binary nodes PLOC allocated
    uint32_t m, cur;             // PLOC: clusters left, the buffer they are in
    uint32_t status, height;
    int root_bin;
    uint32_t level_first, level_count, n_levels;
    uint32_t levels[2 * kBlasBatchMaxLevels];
};

// Thread 0 of a workgroup that gives its mesh back: nothing but the slab and this row was written.
__device__ __forceinline__ void batch_give_back(BlasBatchResult* res, const BatchShared& s, uint32_t status) {
    for (int k = 0; k < 10; k++) res->out[k] = 0u;
    res->status = status; res->height = s.height; res->n_levels = 0u;
}

template <bool PLOC>
__global__ void __launch_bounds__(kBlasBatchBlock) blas_batch_build_kernel(const BlasBatchRow* rows, uint32_t n_rows, const BlasBatchArrays A, BlasBatchResult* results,
                                                                          uint32_t radius) {
    __shared__ BatchShared s;
    constexpr uint32_t B = kBlasBatchBlock, ITEMS = kBlasBatchItems;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x >= n_rows) return;
    const BlasBatchRow row = rows[blockIdx.x];
    BlasBatchResult* const res = results + blockIdx.x;
    const uint32_t n = row.n_tris, node_cap = row.node_cap;
    if (tid == 0) {
        s.bounds[0] = s.bounds[1] = s.bounds[2] = 0xFFFFFFFFu; s.bounds[3] = s.bounds[4] = s.bounds[5] = 0u;
        for (int k = 0; k < 8; k++) s.acc[k] = mesh_acc_seed(k);
        s.counters[0] = 1u; s.counters[1] = 0u; s.counters[2] = 0u;
        s.ploc_nodes = 0u; s.m = n; s.cur = 0u; s.status = kBlasBatchBuilt; s.height = 0u; s.root_bin = 0;
        s.level_first = 0u; s.level_count = 0u; s.n_levels = 0u;
    }
    if (n < 1u || n > kBlasBatchMaxTris || node_cap < 1u || row.scratch == 0u) {       // a row this kernel does not take (block-uniform)
        __syncthreads();
        if (tid == 0) batch_give_back(res, s, kBlasBatchFailed);
        return;
    }
    BatchSlab sl;
    (void)batch_carve((char*)(uintptr_t)row.scratch, n, node_cap, &sl);
    const SrVertex* const vtx = (const SrVertex*)(uintptr_t)row.vertices;
    const uint32_t* const idx = (const uint32_t*)(uintptr_t)row.indices;
    __syncthreads();

    // ---- primitives: records, centroids, Morton grid, root box and padding numbers (blas_prims_kernel)
    {
        BlasPrimAcc r;
        for (uint32_t p = tid; p < n; p += B) blas_prim_one(vtx, idx, row.n_vertices, p, sl.W, sl.cent, r);
        blas_prims_reduce(r, s.bounds, s.acc);
    }
    __syncthreads();

    // ---- Morton keys and the stable sort (lbvh_morton_kernel, DeviceRadixSort): blocked arrangement, ascending triangle id;
    // places past n carry the largest key (bit 63, which no Morton code has) and sort behind everything
    {
        unsigned long long keys[ITEMS];
        uint32_t vals[ITEMS];
        for (uint32_t k = 0; k < ITEMS; k++) {
            const uint32_t p = tid * ITEMS + k;
            keys[k] = 0xFFFFFFFFFFFFFFFFull; vals[k] = 0xFFFFFFFFu;
            if (p < n) { const float4 c = sl.cent[p]; const float q[3] = {c.x, c.y, c.z}; keys[k] = morton_key(q, s.bounds); vals[k] = p; }
        }
        BatchSort(s.u.sort).Sort(keys, vals, 0, 64);
        for (uint32_t k = 0; k < ITEMS; k++) {
            const uint32_t p = tid * ITEMS + k;
            if (p < n) { sl.keys[p] = keys[k]; sl.vals[p] = vals[k] < n ? vals[k] : 0u; }
        }
    }
    __syncthreads();

    // ---- binary topology
    const VertPrims prims{sl.W};
    if (n == 1u) {       // one triangle: no binary tree; the root is one node with one leaf child (build_tree writes it from the host)
        if (tid == 0) {
            for (int k = 0; k < srl::kNodeDwords; k++) sl.nodes[k] = k >= srl::kChildOffset ? 0xFFFFFFFFu : 0u;
            sl.nodes[srl::kChildOffset] = ~((0u << 3) | 1u);
            sl.slot_of_sorted[0] = 0u;
            s.levels[0] = 0u; s.levels[1] = 1u; s.n_levels = 1u;
        }
    } else if (!PLOC) {
        for (uint32_t i = tid; i < n; i += B) sl.flags[i] = 0u;
        for (uint32_t i = tid; i + 1u < n; i += B) lbvh_hierarchy_node(sl.keys, (int)n, (int)i, sl.children, sl.parent_inner, sl.parent_leaf, sl.range);
        __syncthreads();
        for (uint32_t i = tid; i < n; i += B)
            lbvh_fit_from_leaf(prims, sl.vals, (int)i, sl.children, sl.parent_inner, sl.parent_leaf, sl.range, sl.bin_box, sl.bin_height, sl.bin_size, sl.flags);
    } else {
        uint32_t* const nn = (uint32_t*)sl.range;
        uint32_t* const valid = nn + n;
        for (uint32_t i = tid; i < n; i += B) ploc_init_one(prims, sl.vals, i, sl.cid0, sl.cbox0);
        __syncthreads();
        for (uint32_t round = 0; round < kBatchMaxRounds; round++) {
            const uint32_t m = s.m, cur = s.cur;                    // written by thread 0 before the last barrier
            if (m <= 1u || s.status != kBlasBatchBuilt) break;
            int* const cid = cur ? sl.cid1 : sl.cid0; float* const cbox = cur ? sl.cbox1 : sl.cbox0;
            int* const cid_out = cur ? sl.cid0 : sl.cid1; float* const cbox_out = cur ? sl.cbox0 : sl.cbox1;
            for (uint32_t i = tid; i < m; i += B) nn[i] = ploc_nn_one<false>(cbox, m, radius, i);
            __syncthreads();
            for (uint32_t i = tid; i < m; i += B) ploc_merge_one(nn, i, cid, cbox, valid, sl.children, sl.bin_box, sl.bin_size, sl.bin_height, &s.ploc_nodes);
            __syncthreads();
            // compaction in order: a thread owns ITEMS consecutive clusters, the block scan places its survivors
            const uint32_t i0 = tid * ITEMS, i1 = min(i0 + ITEMS, m);
            uint32_t mine = 0u, before = 0u, total = 0u;
            for (uint32_t i = i0; i < i1; i++) mine += valid[i];
            BatchScan(s.u.scan).ExclusiveSum(mine, before, total);
            for (uint32_t i = i0; i < i1; i++)
                if (valid[i]) ploc_compact_one(cid, cbox, i, before++, cid_out, cbox_out);
            __syncthreads();
            if (tid == 0) {
                if (total >= m || total == 0u || round + 1u >= kBatchMaxRounds) s.status = kBlasBatchFailed;     // no progress: cannot happen (the closest pair is always mutual)
                s.m = total; s.cur = cur ^ 1u;
            }
            __syncthreads();
        }
        if (tid == 0 && s.status == kBlasBatchBuilt) {
            const int root = (s.cur ? sl.cid1 : sl.cid0)[0];
            if (s.m != 1u || root < 0 || (uint32_t)root + 1u >= n) s.status = kBlasBatchFailed; else s.root_bin = root;
        }
    }
    __syncthreads();
    if (n > 1u) {
        // ---- the binary height is known here, before anything resident is written
        if (tid == 0 && s.status == kBlasBatchBuilt) {
            const uint32_t h = ((const volatile uint32_t*)sl.bin_height)[s.root_bin];
            s.height = h;
            if (h > row.stack_cap) s.status = kBlasBatchTooTall;      // the height bound's rebalancing stays with the per-mesh build
            else {
                sl.bin_of_node[0] = s.root_bin;
                sl.budget_of_node[0] = h > row.stack_floor ? h : row.stack_floor;
                sl.prefix_of_node[0] = 0u; sl.first_of_node[0] = 0u;
                s.level_first = 0u; s.level_count = 1u;
            }
        }
        __syncthreads();
        // ---- the budgeted 4-wide collapse, level by level, into the slab
        for (uint32_t level = 0; level <= kBlasBatchMaxLevels; level++) {
            const uint32_t first = s.level_first, count = s.level_count;      // written by thread 0 before the last barrier
            if (count == 0u || s.status != kBlasBatchBuilt) break;
            for (uint32_t t = tid; t < count; t += B)
                lbvh_collapse_node(sl.nodes, first + t, node_cap, sl.bin_of_node, sl.budget_of_node, sl.prefix_of_node, sl.first_of_node, sl.children,
                                   sl.bin_size, sl.bin_box, sl.bin_height, sl.slot_of_sorted, s.counters);
            __syncthreads();
            if (tid == 0) {
                const uint32_t made = s.counters[0];
                if (s.counters[2] || made > node_cap || made < first + count || level >= kBlasBatchMaxLevels) s.status = kBlasBatchFailed;
                else {
                    s.levels[2 * level] = first; s.levels[2 * level + 1] = count; s.n_levels = level + 1u;
                    s.level_first = first + count; s.level_count = made - (first + count);
                }
            }
            __syncthreads();
        }
        if (tid == 0 && s.status == kBlasBatchBuilt && (s.level_count != 0u || s.counters[1] > row.stack_cap)) s.status = s.level_count ? kBlasBatchFailed : kBlasBatchTooTall;
        __syncthreads();
    }
    const uint32_t status = s.status;
    if (status != kBlasBatchBuilt) {         // block-uniform; the mesh goes to the per-mesh build with its ranges as they were
        if (tid == 0) batch_give_back(res, s, status);
        return;
    }

    // ---- from here on the tree fits: leaf-order records (blas_leaves_kernel) and the nodes with global references (blas_place_kernel)
    const uint32_t n_nodes = s.counters[0], n_levels = s.n_levels;      // n_nodes <= node_cap, every level inside [0, n_nodes)
    for (uint32_t i = tid; i < n; i += B)
        blas_leaf_one(sl.W, sl.vals, sl.slot_of_sorted, i, n, vtx, idx, row.n_vertices, row.mesh_slot, row.tri_base, A.tris, A.shade,
                      row.textured ? A.shade_tex : nullptr, A.slot_of_gid);
    for (uint32_t i = tid; i < n_nodes && i < node_cap; i += B) {
        uint32_t* const q = A.nodes + ((size_t)row.node_base + i) * srl::kNodeDwords;
        for (int k = 0; k < srl::kNodeDwords; k++) q[k] = sl.nodes[(size_t)i * srl::kNodeDwords + k];
        blas_place_node(q + srl::kChildOffset, row.node_base, row.tri_base);
    }
    __syncthreads();
    // ---- bottom-up refit of the quantised nodes and node_box, deepest level first (refit_level_kernel over VertPrims)
    const VertPrims leaf_prims{A.tris};
    for (uint32_t l = n_levels; l-- > 0u;) {
        const uint32_t first = s.levels[2 * l], count = s.levels[2 * l + 1];
        for (uint32_t i = tid; i < count && first + i < node_cap; i += B) refit_node(A.nodes, leaf_prims, A.node_box, row.node_base + first + i);
        __syncthreads();
    }
    // ---- the finish row (blas_build_finish_kernel) and the rest of the result
    if (tid == 0) {
        blas_build_finish(s.acc, s.counters, row.mesh_slot, row.node_base, row.tri_base, n, A.rows, res->out);
        res->height = s.height; res->n_levels = n_levels;
        for (uint32_t k = 0; k < 2u * n_levels; k++) res->levels[k] = s.levels[k];
        res->status = kBlasBatchBuilt;
    }
}

}  // namespace srd

using namespace srd;

size_t srk_blas_batch_slab_bytes(uint32_t n_tris, uint32_t node_cap) {
    BatchSlab s;
    return batch_carve(nullptr, n_tris, node_cap, &s);
}

int srk_blas_batch_build(const BlasBatchRow* rows, uint32_t n_rows, const BlasBatchArrays& arrays, BlasBatchResult* results, int ploc, hipStream_t stream) {
    if (n_rows == 0) return 0;
    if (ploc) blas_batch_build_kernel<true><<<dim3(n_rows), dim3(kBlasBatchBlock), 0, stream>>>(rows, n_rows, arrays, results, (uint32_t)ploc);
    else blas_batch_build_kernel<false><<<dim3(n_rows), dim3(kBlasBatchBlock), 0, stream>>>(rows, n_rows, arrays, results, 0u);
    return (int)hipGetLastError();
}
