// Host side of sr_probe_node_step (node_probe.h): row validation and packing. No HIP.
#include "node_probe.h"

#include <cstring>

namespace srh {

namespace {
bool one_leaf_child(const uint32_t* node) {
    int leaves = 0, unused = 0;
    for (int c = 0; c < 4; c++) {
        const uint32_t ref = node[kNodeProbeChildDword + c];
        leaves += ref == kNodeProbeLeaf ? 1 : 0;
        unused += ref == kNodeProbeUnused ? 1 : 0;
    }
    return leaves == 1 && unused == 3;
}
}  // namespace

int node_probe_validate(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, const SrNodeProbeOut* out) {
    if (kind >= SR_NODE_PROBE_COUNT) return set_error(SR_ERR_INVALID_ARG, "sr_probe_node_step: unknown kind " + std::to_string(kind));
    if (n && (!rows || !out)) return set_error(SR_ERR_INVALID_ARG, "sr_probe_node_step: null pointer");
    if (kind == SR_NODE_PROBE_KEY) return SR_OK;
    const bool tl = kind == SR_NODE_PROBE_CLOSEST_TL || kind == SR_NODE_PROBE_ANY_TL;
    for (uint32_t i = 0; i < n; i++) {
        if (!one_leaf_child(rows[i].node) || (tl && !one_leaf_child(rows[i].mesh_node)))
            return set_error(SR_ERR_INVALID_ARG, "sr_probe_node_step: row " + std::to_string(i) +
                                                     ": a node's children must be one leaf of triangle 0 alone and three unused slots");
    }
    return SR_OK;
}

void node_probe_pack(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, NodeProbeArrays& a) {
    const bool tl = kind == SR_NODE_PROBE_CLOSEST_TL || kind == SR_NODE_PROBE_ANY_TL;
    a.rays.resize(n);
    a.nodes.resize((size_t)n * 16);
    a.tris.resize((size_t)n * 12);
    a.mesh_nodes.resize(tl ? (size_t)n * 16 : 0);
    a.instances.resize(tl ? (size_t)n * 32 : 0);
    a.tl_inst.assign(tl ? n : 0, 0u);
    for (uint32_t i = 0; i < n; i++) {
        a.rays[i] = rows[i].ray;
        memcpy(&a.nodes[(size_t)i * 16], rows[i].node, 64);
        memcpy(&a.tris[(size_t)i * 12], rows[i].tri, 48);
        if (!tl) continue;
        memcpy(&a.mesh_nodes[(size_t)i * 16], rows[i].mesh_node, 64);
        uint32_t* rec = &a.instances[(size_t)i * 32];
        memcpy(rec, rows[i].instance, 128);
        rec[kNodeProbeBlasRootDword] = 0u;     // the row's own mesh node, whatever the record says
        rec[kNodeProbeTriOffsetDword] = 0u;
    }
}

}  // namespace srh
