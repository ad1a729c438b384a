// The host side of sr_scene_set_instances_device under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program
// (g++, host_prep.cpp alone): srh::instance_tables_host (what sr_instance_tables_host forwards to), the layout half and the
// transform half of frame_instance_data, and the size limits both entry points apply. n = 0, n = 1, a large n, counts that sum
// to just under and to exactly 2^28 instances (the limit check runs on the counts alone: nothing of that size is allocated).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host.h"

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

srh::HostMesh mesh_of(uint64_t key, uint32_t n_tris, uint32_t n_emissive, uint32_t first_slot) {
    srh::HostMesh m;
    m.key = key; m.n_vertices = 3 * n_tris; m.n_indices = 3 * n_tris;
    for (uint32_t k = 0; k < n_emissive; k++) m.emissive_slots.push_back(first_slot + k);
    return m;
}

SrTransform transform_of(uint32_t i) {
    const float s = 0.5f + 0.001f * (float)(i % 1000), t = (float)i * 0.25f;
    return SrTransform{{s, 0.1f, 0, t, 0, s * 2, 0.2f, -t, 0.3f, 0, s * 3, 1.0f}};
}

void check_tables(const std::vector<SrTransform>& xf) {
    std::vector<float> out(xf.size() * 24 + 1, 77.0f);          // one word behind the table: must stay
    srh::instance_tables_host(xf.data(), xf.size(), out.data());
    EXPECT(out[xf.size() * 24] == 77.0f);
    for (size_t i = 0; i < xf.size(); i++) {
        float w[9];
        srh::world_to_object_3x3(xf[i], w);
        const float* q = &out[i * 24];
        EXPECT(memcmp(q, w, 36) == 0);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) EXPECT(q[12 + 3 * r + c] == xf[i].m[4 * r + c]);
        for (int k = 9; k < 12; k++) EXPECT(q[k] == 0.0f && q[12 + k] == 0.0f);
    }
}

void check_layout(const std::vector<srh::HostMesh>& meshes, const std::map<uint64_t, uint32_t>& slots, const std::vector<uint64_t>& keys,
                  const std::vector<uint32_t>& counts) {
    uint64_t n_inst = 0, n_tri = 0;
    srh::instance_list_sizes(meshes, slots, keys.data(), counts.data(), (uint32_t)keys.size(), &n_inst, &n_tri);
    std::string err;
    EXPECT(srh::instance_list_limits(n_inst, n_tri, true, err) == SR_OK);
    srh::FrameInstanceData layout, whole;
    EXPECT(srh::frame_instance_layout(meshes, slots, keys.data(), counts.data(), (uint32_t)keys.size(), layout, err));
    EXPECT(layout.instances.size() == n_inst && layout.n_triangles == n_tri);
    EXPECT(layout.transforms.size() == (n_inst ? n_inst : 1) && !layout.emissive_entries.empty());
    std::vector<SrTransform> xf(n_inst);
    for (uint32_t i = 0; i < n_inst; i++) xf[i] = transform_of(i);
    srh::frame_instance_transforms(xf.data(), layout);
    EXPECT(srh::frame_instance_data(meshes, slots, keys.data(), counts.data(), (uint32_t)keys.size(), xf.data(), whole, err));
    EXPECT(whole.instances.size() == layout.instances.size() && whole.n_triangles == layout.n_triangles);
    EXPECT(whole.transforms.size() == layout.transforms.size() && memcmp(whole.transforms.data(), layout.transforms.data(), sizeof(SrTransform) * whole.transforms.size()) == 0);
    EXPECT(whole.emissive_entries.size() == layout.emissive_entries.size() &&
           memcmp(whole.emissive_entries.data(), layout.emissive_entries.data(), sizeof(SrEmissiveIndirectionEntry) * whole.emissive_entries.size()) == 0);
    uint32_t at = 0, tri = 0;
    for (size_t k = 0; k < keys.size(); k++)
        for (uint32_t c = 0; c < counts[k]; c++, at++) {
            const uint32_t slot = slots.at(keys[k]);
            EXPECT(layout.instances[at].mesh_slot == slot && layout.instances[at].tri_offset == tri);
            EXPECT(memcmp(&layout.instances[at].o2w, &xf[at], sizeof(SrTransform)) == 0 && memcmp(&whole.instances[at].o2w, &xf[at], sizeof(SrTransform)) == 0);
            tri += meshes[slot].n_indices / 3;
        }
    check_tables(xf);
}
}  // namespace

int main() {
    const std::vector<srh::HostMesh> meshes = {mesh_of(10, 2, 0, 0), mesh_of(20, 60, 0, 0), mesh_of(30, 2, 2, 0)};
    const std::map<uint64_t, uint32_t> slots = {{10, 0}, {20, 1}, {30, 2}};
    check_layout(meshes, slots, {}, {});                                       // n = 0
    check_layout(meshes, slots, {10}, {0});                                    // a key without instances
    check_layout(meshes, slots, {20}, {1});                                    // n = 1
    check_layout(meshes, slots, {10, 20, 30, 10}, {257, 513, 3, 1});
    check_layout(meshes, slots, {10, 30}, {(1u << 20) - 3, 3});                // a large n
    std::string err;
    srh::FrameInstanceData fid;
    const uint64_t unknown = 99; const uint32_t one = 1;
    EXPECT(!srh::frame_instance_layout(meshes, slots, &unknown, &one, 1, fid, err) && err == "frame_instance_data: instance references a BLAS key that was never loaded");
    // the limits, on counts alone
    uint64_t n_inst = 0, n_tri = 0;
    const std::vector<uint64_t> keys = {10, 10, 10};
    std::vector<uint32_t> counts = {1u << 27, (1u << 27) - 2, 1};              // 2^28 - 1 instances of two triangles: 2^29 - 2 triangles
    srh::instance_list_sizes(meshes, slots, keys.data(), counts.data(), 3, &n_inst, &n_tri);
    EXPECT(n_inst == (1ull << 28) - 1 && n_tri == (1ull << 29) - 2);
    EXPECT(srh::instance_list_limits(n_inst, n_tri, false, err) == SR_OK);
    EXPECT(srh::instance_list_limits(n_inst, n_tri, true, err) == SR_ERR_UNSUPPORTED && err.find("2^28 triangles") != std::string::npos);
    counts[2] = 2;
    srh::instance_list_sizes(meshes, slots, keys.data(), counts.data(), 3, &n_inst, &n_tri);
    EXPECT(n_inst == (1ull << 28) && srh::instance_list_limits(n_inst, n_tri, false, err) == SR_ERR_UNSUPPORTED && err == "scene exceeds 2^28 instances");
    counts = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};                          // sums that need 64 bits
    srh::instance_list_sizes(meshes, slots, keys.data(), counts.data(), 3, &n_inst, &n_tri);
    EXPECT(n_inst == 3ull * 0xFFFFFFFFull && srh::instance_list_limits(n_inst, n_tri, false, err) == SR_ERR_UNSUPPORTED && err.find("2^32 - 1 triangles") != std::string::npos);
    if (failures) return 1;
    printf("instances ok: layouts of 0, 0, 1, 774 and 1048576 instances, limits at 2^28\n");
    return 0;
}
