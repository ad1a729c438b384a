// The node-step probe (sr_probe_node_step): the host side. Which rows the hook takes, and how a call's rows are laid out as
// the arrays the kernel reads — copies only, no arithmetic.
// No HIP here: a stand-alone program links node_probe_rows.cpp and brings srh::set_error, the one symbol it needs from outside.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/sunray_hip.h"

namespace srh {

int set_error(int code, const std::string& msg);   // the library's error slot (api.cpp); returns `code`

constexpr uint32_t kNodeProbeLeaf = ~((0u << 3) | 1u);   // the one child reference a probed node may use: triangle 0, one triangle
constexpr uint32_t kNodeProbeUnused = 0xFFFFFFFFu;       // -1: an unused slot
constexpr int kNodeProbeChildDword = 12;                 // child[4] of a 64-byte node (csrc/bvh_layout.h)
// of the 128-byte instance record (srd::DevTlInstance): where its tree starts, the global index of its primitive 0
constexpr int kNodeProbeBlasRootDword = 24, kNodeProbeTriOffsetDword = 25;

// SR_OK, or SR_ERR_INVALID_ARG with the reason in the error slot: an unknown kind, a null pointer with n > 0, a node whose
// child dwords are not kNodeProbeLeaf in one slot and kNodeProbeUnused in the other three (the two-level kinds: of either node).
int node_probe_validate(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, const SrNodeProbeOut* out);

// A call's rows as the kernel reads them: array k holds part k of every row, row i at i * (the part's size).
struct NodeProbeArrays {
    std::vector<SrRay> rays;
    std::vector<uint32_t> nodes, tris;             // 16 / 12 dwords a row
    std::vector<uint32_t> mesh_nodes, instances;   // two-level kinds only: 16 / 32 dwords a row
    std::vector<uint32_t> tl_inst;                 // two-level kinds only: leaf position 0 of every row's top-level tree -> instance 0
};
void node_probe_pack(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, NodeProbeArrays& a);

}  // namespace srh
