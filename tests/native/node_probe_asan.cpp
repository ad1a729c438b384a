// Stand-alone driver of csrc/node_probe_rows.cpp for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_node_probe_sanitizers.py): the host side of sr_probe_node_step — row validation and packing — on hand-made rows.
// Every row array is allocated on the heap at its exact size, so a read past the last row or a write past a packed array is an
// error the sanitizer reports. Row counts around the wave and workgroup sizes, every kind, every refusal the hook knows, seeded
// random child words. Exit status 0 and "node_probe ok" when everything held.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "node_probe.h"

static std::string g_error;
int srh::set_error(int code, const std::string& msg) { g_error = msg; return code; }   // the library's error slot, here the program's

static int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_error.c_str()); g_failures++; } \
    } while (0)

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

// a row of random words whose nodes keep the rule: one leaf of triangle 0 in slot c, -1 elsewhere
static SrNodeProbeRow valid_row(uint32_t c_top, uint32_t c_mesh) {
    SrNodeProbeRow r;
    uint32_t* w = reinterpret_cast<uint32_t*>(&r);
    for (size_t k = 0; k < sizeof(r) / 4; k++) w[k] = rnd();
    for (uint32_t c = 0; c < 4; c++) {
        r.node[srh::kNodeProbeChildDword + c] = c == c_top ? srh::kNodeProbeLeaf : srh::kNodeProbeUnused;
        r.mesh_node[srh::kNodeProbeChildDword + c] = c == c_mesh ? srh::kNodeProbeLeaf : srh::kNodeProbeUnused;
    }
    return r;
}

static bool is_tl(uint32_t kind) { return kind == SR_NODE_PROBE_CLOSEST_TL || kind == SR_NODE_PROBE_ANY_TL; }

static void run_valid(uint32_t kind, uint32_t n) {
    std::vector<SrNodeProbeRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = valid_row(rnd() & 3u, rnd() & 3u);
    std::vector<SrNodeProbeOut> out(n);
    CHECK(srh::node_probe_validate(kind, n ? rows.data() : nullptr, n, n ? out.data() : nullptr) == SR_OK);
    srh::NodeProbeArrays a;
    srh::node_probe_pack(kind, rows.data(), n, a);
    const bool tl = is_tl(kind);
    CHECK(a.rays.size() == n && a.nodes.size() == (size_t)n * 16 && a.tris.size() == (size_t)n * 12);
    CHECK(a.mesh_nodes.size() == (tl ? (size_t)n * 16 : 0) && a.instances.size() == (tl ? (size_t)n * 32 : 0) && a.tl_inst.size() == (tl ? n : 0));
    for (uint32_t i = 0; i < n; i++) {
        CHECK(memcmp(&a.rays[i], &rows[i].ray, sizeof(SrRay)) == 0);
        CHECK(memcmp(&a.nodes[(size_t)i * 16], rows[i].node, 64) == 0 && memcmp(&a.tris[(size_t)i * 12], rows[i].tri, 48) == 0);
        if (!tl) continue;
        CHECK(memcmp(&a.mesh_nodes[(size_t)i * 16], rows[i].mesh_node, 64) == 0 && a.tl_inst[i] == 0u);
        for (int k = 0; k < 32; k++) {      // the record as it is, but for where its tree and its triangles start
            const bool zeroed = k == srh::kNodeProbeBlasRootDword || k == srh::kNodeProbeTriOffsetDword;
            CHECK(a.instances[(size_t)i * 32 + k] == (zeroed ? 0u : rows[i].instance[k]));
        }
    }
}

static void run_refused(uint32_t kind) {
    const uint32_t n = 65;
    std::vector<SrNodeProbeOut> out(n);
    const bool tl = is_tl(kind);
    const uint32_t bad[] = {0u, 1u, ~((0u << 3) | 2u), ~((1u << 3) | 1u), 0x7fffffffu};   // inner nodes, two triangles, triangle 1, the sentinel
    for (uint32_t where = 0; where < 2; where++) {              // in the node, in the mesh node
        for (uint32_t row : {0u, 31u, n - 1u}) {
            for (uint32_t slot = 0; slot < 4; slot++) {
                for (uint32_t b : bad) {
                    std::vector<SrNodeProbeRow> rows(n);
                    for (uint32_t i = 0; i < n; i++) rows[i] = valid_row(i & 3u, (i >> 2) & 3u);
                    (where ? rows[row].mesh_node : rows[row].node)[srh::kNodeProbeChildDword + slot] = b;
                    g_error.clear();
                    const int rc = srh::node_probe_validate(kind, rows.data(), n, out.data());
                    if (kind == SR_NODE_PROBE_KEY || (where == 1 && !tl)) CHECK(rc == SR_OK);      // not a node this kind walks
                    else CHECK(rc == SR_ERR_INVALID_ARG && g_error.find("row " + std::to_string(row)) != std::string::npos);
                }
            }
            // a second leaf, and no leaf at all
            std::vector<SrNodeProbeRow> rows(n);
            for (uint32_t i = 0; i < n; i++) rows[i] = valid_row(i & 3u, (i >> 2) & 3u);
            uint32_t* node = where ? rows[row].mesh_node : rows[row].node;
            node[srh::kNodeProbeChildDword + ((row + 1u) & 3u)] = node[srh::kNodeProbeChildDword + ((row + 2u) & 3u)] = srh::kNodeProbeLeaf;
            int rc = srh::node_probe_validate(kind, rows.data(), n, out.data());
            CHECK((rc == SR_OK) == (kind == SR_NODE_PROBE_KEY || (where == 1 && !tl)));
            for (uint32_t c = 0; c < 4; c++) node[srh::kNodeProbeChildDword + c] = srh::kNodeProbeUnused;
            rc = srh::node_probe_validate(kind, rows.data(), n, out.data());
            CHECK((rc == SR_OK) == (kind == SR_NODE_PROBE_KEY || (where == 1 && !tl)));
        }
    }
    std::vector<SrNodeProbeRow> rows(n);
    for (uint32_t i = 0; i < n; i++) rows[i] = valid_row(i & 3u, (i >> 2) & 3u);
    CHECK(srh::node_probe_validate(kind, nullptr, n, out.data()) == SR_ERR_INVALID_ARG);
    CHECK(srh::node_probe_validate(kind, rows.data(), n, nullptr) == SR_ERR_INVALID_ARG);
    CHECK(srh::node_probe_validate(kind, nullptr, 0, nullptr) == SR_OK);
}

int main() {
    const uint32_t counts[] = {0u, 1u, 63u, 64u, 65u, 257u, 3000u};
    unsigned calls = 0;
    for (uint32_t kind = 0; kind < SR_NODE_PROBE_COUNT; kind++) {
        for (uint32_t n : counts) { run_valid(kind, n); calls++; }
        run_refused(kind);
    }
    std::vector<SrNodeProbeRow> rows(4);
    std::vector<SrNodeProbeOut> out(4);
    for (auto& r : rows) r = valid_row(0, 0);
    CHECK(srh::node_probe_validate(SR_NODE_PROBE_COUNT, rows.data(), 4, out.data()) == SR_ERR_INVALID_ARG);
    CHECK(srh::node_probe_validate(0xFFFFFFFFu, rows.data(), 4, out.data()) == SR_ERR_INVALID_ARG);
    if (g_failures) { printf("node_probe: %d checks failed\n", g_failures); return 1; }
    printf("node_probe ok: %u packed calls over %u kinds\n", calls, (unsigned)SR_NODE_PROBE_COUNT);
    return 0;
}
