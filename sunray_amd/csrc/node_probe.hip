// Test hook: the node step of traverse_ws on one hand-made node per ray (sr_probe_node_step in include/sunray_hip.h,
// tests/test_gpu_node_step.py), and ord_f32 / unord_f32 on raw floats.
//
// Whole queries are compared with brute force and the builders' boxes with their geometry; this unit lets a test hold the box
// tests in between — the slab arithmetic, box_dir / ray_setup, the instance entry, the padded test of the two-level form — against
// exact arithmetic, row by row. Every lane walks a scene of its own: DevScene pointers at its row's node, triangle and instance
// record, so traverse_ws itself runs, from node 0, and nothing is restated here. A translation unit of its own so that the object
// code of the pass kernels is what it was without it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "node_probe.h"
#include "traverse.h"

namespace {
using namespace srd;

static_assert(sizeof(DevTlInstance) == 128 && offsetof(DevTlInstance, blas_root) == 4 * srh::kNodeProbeBlasRootDword &&
                  offsetof(DevTlInstance, tri_offset) == 4 * srh::kNodeProbeTriOffsetDword,
              "node_probe.h addresses the instance record by dwords");

constexpr int kProbeBlock = 256;   // the ray-list tracers' workgroup: one wave per 64 rows, four waves
// LDS stack entries per lane, by the scene layer's rule for a tree that needs two (api.cpp: max(need, 3) + 1 spare level of the
// branch-free push, rounded up to a multiple of 4). A finite ray pushes nothing here; a ray with a non-finite origin can find
// all four slots of a node "not culled" and push three references of unused slots, which the four levels hold.
constexpr int kProbeStackNeed = 2;
constexpr int kProbeStackEntries = ((kProbeStackNeed > 3 ? kProbeStackNeed : 3) + 1 + 3) & ~3;

template <bool ANY, bool TL>
__global__ void __launch_bounds__(kProbeBlock)
node_step_probe_kernel(const SrRay* __restrict__ rays, const float4* __restrict__ nodes, const float4* __restrict__ tris,
                       const float4* __restrict__ mesh_nodes, const DevTlInstance* __restrict__ instances,
                       const uint32_t* __restrict__ tl_inst, uint32_t n, SrNodeProbeOut* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) int s_stack[];   // [rows of traverse_ws + stack entries][kProbeBlock]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t base = (blockIdx.x * (kProbeBlock / 64) + (threadIdx.x >> 6)) * 64u;
    if (base >= n) return;                                          // wave-uniform
    const uint32_t i = base + lane;
    const uint32_t ic = i < n ? i : n - 1u;                         // rows past n in the last wave run with want = false
    DevScene sc = {};
    sc.nodes = nodes + (size_t)ic * 4;
    sc.tris = tris + (size_t)ic * 3;
    if (TL) {
        sc.blas_nodes = mesh_nodes + (size_t)ic * 4;
        sc.tl_inst = tl_inst + ic;
        sc.tl_instances = instances + ic;
        sc.n_instances = 1u;
    }
    sc.n_tris = 1u;
    const float4 ra = reinterpret_cast<const float4*>(rays)[(size_t)ic * 2 + 0];
    const float4 rb = reinterpret_cast<const float4*>(rays)[(size_t)ic * 2 + 1];
    TravStats st; st.boxes = 0; st.tris = 0;
    TravHit h;
    const bool found = traverse_ws<ANY, true, TL>(sc, i < n, mk3(ra.x, ra.y, ra.z), mk3(rb.x, rb.y, rb.z), ra.w, rb.w, h, s_stack + threadIdx.x,
                                                  kProbeBlock, st);
    if (i < n) {
        SrNodeProbeOut o;
        o.boxes = st.boxes; o.tris = st.tris;
        if (ANY) { o.hit.t = 0.0f; o.hit.u = 0.0f; o.hit.v = 0.0f; o.hit.tri = found ? 1u : 0u; }
        else { o.hit.t = h.t; o.hit.u = h.u; o.hit.v = h.v; o.hit.tri = h.gid; }
        out[i] = o;
    }
}

__global__ void __launch_bounds__(kProbeBlock) key_probe_kernel(const SrRay* __restrict__ rays, uint32_t n, SrNodeProbeOut* __restrict__ out) {
    const uint32_t i = blockIdx.x * kProbeBlock + threadIdx.x;
    if (i >= n) return;
    const float f = rays[i].origin[0];
    const uint32_t key = __float_as_uint(rays[i].origin[1]);
    SrNodeProbeOut o;
    o.boxes = ord_f32(f);
    o.tris = __float_as_uint(unord_f32(o.boxes));
    o.hit.t = 0.0f; o.hit.u = 0.0f; o.hit.v = 0.0f;
    o.hit.tri = __float_as_uint(unord_f32(key));
    out[i] = o;
}

// Device memory of one call, freed on every way out.
struct DeviceArrays {
    void* p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~DeviceArrays() { for (void* q : p) if (q) (void)hipFree(q); }
    // SR_OK, or the HIP error in the library's slot
    int upload(int k, const void* src, size_t bytes) {
        if (bytes == 0) return SR_OK;
        hipError_t e = hipMalloc(&p[k], bytes);
        if (e == hipSuccess && src) e = hipMemcpy(p[k], src, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? SR_OK : srh::set_error(SR_ERR_HIP, std::string("sr_probe_node_step: upload: ") + hipGetErrorString(e));
    }
};

}  // namespace

extern "C" {

int sr_probe_node_step(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, SrNodeProbeOut* out) {
    int rc = srh::node_probe_validate(kind, rows, n, out);
    if (rc != SR_OK) return rc;
    if (n == 0) return SR_OK;
    srh::NodeProbeArrays a;
    srh::node_probe_pack(kind, rows, n, a);
    DeviceArrays d;
    const auto bytes = [](const std::vector<uint32_t>& v) { return v.size() * sizeof(uint32_t); };
    if ((rc = d.upload(0, a.rays.data(), a.rays.size() * sizeof(SrRay))) != SR_OK) return rc;
    if ((rc = d.upload(6, nullptr, (size_t)n * sizeof(SrNodeProbeOut))) != SR_OK) return rc;
    if (kind != SR_NODE_PROBE_KEY) {
        if ((rc = d.upload(1, a.nodes.data(), bytes(a.nodes))) != SR_OK) return rc;
        if ((rc = d.upload(2, a.tris.data(), bytes(a.tris))) != SR_OK) return rc;
        if ((rc = d.upload(3, a.mesh_nodes.data(), bytes(a.mesh_nodes))) != SR_OK) return rc;
        if ((rc = d.upload(4, a.instances.data(), bytes(a.instances))) != SR_OK) return rc;
        if ((rc = d.upload(5, a.tl_inst.data(), bytes(a.tl_inst))) != SR_OK) return rc;
    }
    const dim3 grid((n + kProbeBlock - 1) / kProbeBlock), block(kProbeBlock);
    const bool tl = kind == SR_NODE_PROBE_CLOSEST_TL || kind == SR_NODE_PROBE_ANY_TL;
    const size_t lds = (size_t)(kProbeStackEntries + (tl ? kWsRowsTl : kWsRows)) * kProbeBlock * sizeof(int);
    const SrRay* rays_d = (const SrRay*)d.p[0];
    const float4* nodes_d = (const float4*)d.p[1];
    const float4* tris_d = (const float4*)d.p[2];
    const float4* mesh_d = (const float4*)d.p[3];
    const DevTlInstance* inst_d = (const DevTlInstance*)d.p[4];
    const uint32_t* tl_inst_d = (const uint32_t*)d.p[5];
    SrNodeProbeOut* out_d = (SrNodeProbeOut*)d.p[6];
    switch (kind) {
        case SR_NODE_PROBE_CLOSEST: node_step_probe_kernel<false, false><<<grid, block, lds, 0>>>(rays_d, nodes_d, tris_d, mesh_d, inst_d, tl_inst_d, n, out_d); break;
        case SR_NODE_PROBE_ANY: node_step_probe_kernel<true, false><<<grid, block, lds, 0>>>(rays_d, nodes_d, tris_d, mesh_d, inst_d, tl_inst_d, n, out_d); break;
        case SR_NODE_PROBE_CLOSEST_TL: node_step_probe_kernel<false, true><<<grid, block, lds, 0>>>(rays_d, nodes_d, tris_d, mesh_d, inst_d, tl_inst_d, n, out_d); break;
        case SR_NODE_PROBE_ANY_TL: node_step_probe_kernel<true, true><<<grid, block, lds, 0>>>(rays_d, nodes_d, tris_d, mesh_d, inst_d, tl_inst_d, n, out_d); break;
        default: key_probe_kernel<<<grid, block, 0, 0>>>(rays_d, n, out_d); break;
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return srh::set_error(SR_ERR_HIP, std::string("sr_probe_node_step: kernel: ") + hipGetErrorString(e));
    std::vector<SrNodeProbeOut> host(n);
    e = hipMemcpy(host.data(), out_d, (size_t)n * sizeof(SrNodeProbeOut), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return srh::set_error(SR_ERR_HIP, std::string("sr_probe_node_step: read back: ") + hipGetErrorString(e));
    for (uint32_t i = 0; i < n; i++) out[i] = host[i];
    return SR_OK;
}

}  // extern "C"
