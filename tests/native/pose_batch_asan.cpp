// The host side of batched posing (sr_pose_batch_plan, srh::pose_batch_layout, srh::pose_batch_block_table: csrc/pose_batch_plan.cpp)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: exact-size heap arrays, so a write past a plan's
// outputs or a block table is caught; the counts of the tests, adversarial ones, and seeded random batches.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pose_batch_plan.h"

namespace srh {
static std::string g_error;
int set_error(int code, const std::string& msg) { g_error = msg; return code; }
}  // namespace srh

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

// Plans `counts`, fills a block table and a staging layout of exact size, and checks every figure against a direct count.
static int run(const std::vector<uint32_t>& counts, bool expect_ok) {
    const uint32_t n = (uint32_t)counts.size();
    std::vector<uint32_t> first(n, 0xCDCDCDCDu);
    std::vector<uint64_t> base(n, 0xCDCDCDCDCDCDCDCDull);
    uint32_t n_blocks = 0xCDCDCDCDu;
    const int rc = sr_pose_batch_plan(counts.data(), n, first.data(), base.data(), &n_blocks);
    if (!expect_ok) {
        CHECK(rc == SR_ERR_UNSUPPORTED && !srh::g_error.empty() && n_blocks == 0xCDCDCDCDu);
        for (uint32_t i = 0; i < n; i++) CHECK(first[i] == 0xCDCDCDCDu && base[i] == 0xCDCDCDCDCDCDCDCDull);
        return 0;
    }
    CHECK(rc == SR_OK);
    uint64_t blocks = 0, vertices = 0;
    for (uint32_t i = 0; i < n; i++) {
        CHECK(first[i] == blocks && base[i] == vertices);
        blocks += ((uint64_t)counts[i] + 255) / 256;
        vertices += counts[i];
    }
    CHECK(n_blocks == blocks);
    if (blocks > (1u << 22)) return 0;                       // the table of a huge plan is not allocated here
    std::vector<uint32_t> table(n_blocks, 0xCDCDCDCDu);
    srh::pose_batch_block_table(first.data(), n, n_blocks, table.data());
    for (uint32_t b = 0; b < n_blocks; b++) {
        const uint32_t i = table[b];
        CHECK(i < n && b >= first[i] && (uint64_t)(b - first[i]) * 256 < counts[i]);      // block b holds a tile of item i that has vertices
    }
    const uint64_t n_matrices = 3ull * n + 1, n_active = 5ull * n + 3;
    const srh::PoseBatchLayout l = srh::pose_batch_layout(n, n_blocks, n_matrices, n_active);
    CHECK(l.items == 0 && l.block_table == 64ull * n && l.matrices >= l.block_table + 4ull * n_blocks && l.active_index == l.matrices + 48 * n_matrices);
    CHECK(l.active_weight >= l.active_index + 4 * n_active && l.bytes >= l.active_weight + 4 * n_active);
    CHECK(l.block_table % 16 == 0 && l.matrices % 16 == 0 && l.active_index % 16 == 0 && l.active_weight % 16 == 0 && l.bytes % 16 == 0);
    std::vector<unsigned char> stage(l.bytes);               // every part is written to its end inside the block
    memset(stage.data() + l.block_table, 1, 4ull * n_blocks);
    memset(stage.data() + l.matrices, 2, 48 * n_matrices);
    memset(stage.data() + l.active_index, 3, 4 * n_active);
    memset(stage.data() + l.active_weight, 4, 4 * n_active);
    return 0;
}

int main(int argc, char** argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 200;
    const std::vector<std::vector<uint32_t>> good = {
        {3, 4, 63, 64, 65, 257, 1026, 256, 512}, std::vector<uint32_t>(1000, 1), {255, 256, 257}, {257, 256, 255}, {256, 255, 257}, {},
        {0}, {0, 0, 0}, {0, 1, 0, 256, 0, 257, 0}, {0xFFFFFFFFu}, {0x7FFFFFFFu, 0x7FFFFFFFu, 1u}, {0xFFFFFF00u, 0xFFu},
    };
    const std::vector<std::vector<uint32_t>> refused = {
        {0x80000000u, 0x80000000u}, {0xFFFFFFFFu, 1u}, std::vector<uint32_t>(128, 0xFFFFFFFFu), std::vector<uint32_t>(4096, 0xFFFFFFFFu),
        {0xFFFFFFFFu, 0u, 0u, 1u},
    };
    for (const auto& c : good) if (run(c, true)) return 1;
    for (const auto& c : refused) if (run(c, false)) return 1;
    uint32_t n_blocks = 0;
    if (sr_pose_batch_plan(nullptr, 3, nullptr, nullptr, &n_blocks) != SR_ERR_INVALID_ARG || sr_pose_batch_plan(nullptr, 0, nullptr, nullptr, nullptr) != SR_ERR_INVALID_ARG ||
        sr_pose_batch_plan(nullptr, 0, nullptr, nullptr, &n_blocks) != SR_OK || n_blocks != 0) { printf("FAILED: null arguments\n"); return 1; }
    uint32_t seed = 12345u;
    for (int k = 0; k < n_random; k++) {
        std::vector<uint32_t> c;
        seed = seed * 1664525u + 1013904223u;
        const uint32_t n = (seed >> 16) % 40;
        for (uint32_t i = 0; i < n; i++) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t kind = (seed >> 28) & 3u, r = (seed >> 8) & 0xFFFFu;
            c.push_back(kind == 0 ? 0u : kind == 1 ? 256u * (r % 5) : kind == 2 ? r % 1200 : 256u * (r % 9) + (r & 1u ? 1u : 255u));
        }
        if (run(c, true)) return 1;
    }
    printf("pose_batch ok: %zu plans, %zu refusals, %d random batches\n", good.size(), refused.size(), n_random);
    return 0;
}
