// Stand-alone driver of csrc/mesh_frame.cpp for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_mesh_frame_sanitizers.py):
// hand-made meshes, the inputs that must be refused, counting calls with NULL outputs, and seeded random small meshes whose
// positions and normals come from a few values so that groups of several vertices form. Every output array is allocated at its
// exact size, so a write past it is an error the sanitizer reports. Exit status 0 and "mesh_frame ok" when everything held.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mesh_frame.h"

static std::string g_error;
int srh::set_error(int code, const std::string& msg) { g_error = msg; return code; }   // the library's error slot, here the program's

static int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #cond, g_error.c_str()); g_failures++; } \
    } while (0)

struct Mesh { std::vector<SrVertex> v; std::vector<uint32_t> i; };

static SrVertex vertex(float x, float y, float z, float nx, float ny, float nz, float u, float w) {
    SrVertex r;
    memset(&r, 0, sizeof(r));
    r.position[0] = x; r.position[1] = y; r.position[2] = z;
    r.normal[0] = nx; r.normal[1] = ny; r.normal[2] = nz;
    r.tangent[0] = 1.0f; r.tangent[3] = -1.0f;
    r.normal_tex_coord[0] = u; r.normal_tex_coord[1] = w;
    return r;
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// the whole surface on one valid mesh: count, fill at exact sizes, the invariants of the runs, the host rule under both flag sets
static void run_valid(const Mesh& m) {
    const uint32_t nv = (uint32_t)m.v.size(), ni = (uint32_t)m.i.size();
    uint32_t n = 0xFFFFFFFFu, n2 = 0;
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, nullptr, nullptr, nullptr, &n) == SR_OK);
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, nullptr, nullptr, nullptr, nullptr) == SR_OK);   // nothing asked for
    CHECK(n >= ni || nv == 0);
    std::vector<uint32_t> offsets((size_t)nv + 1), entries(n);
    std::vector<float> side(nv);
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, offsets.data(), entries.data(), side.data(), &n2) == SR_OK);
    CHECK(n2 == n && offsets[0] == 0 && offsets[nv] == n);
    for (uint32_t k = 0; k < nv; k++) {
        CHECK(offsets[k] <= offsets[k + 1] && (side[k] == 1.0f || side[k] == -1.0f));
        for (uint32_t e = offsets[k]; e + 1 < offsets[k + 1]; e++) CHECK(entries[e] <= entries[e + 1]);
    }
    for (uint32_t e : entries) CHECK(e < ni / 3);
    // each out pointer alone
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, offsets.data(), nullptr, nullptr, nullptr) == SR_OK);
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, nullptr, entries.data(), nullptr, &n2) == SR_OK);
    CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, nullptr, nullptr, side.data(), nullptr) == SR_OK);
    std::vector<float> pos((size_t)nv * 3);
    for (uint32_t k = 0; k < nv; k++)
        for (int c = 0; c < 3; c++) pos[3 * (size_t)k + c] = m.v[k].position[c] + 0.05f * (float)((k * 7 + c * 3) % 5);
    for (uint32_t flags : {SR_FRAME_NORMALS, SR_FRAME_NORMALS | SR_FRAME_TANGENTS}) {
        std::vector<SrVertex> out(nv);
        uint32_t bad = 5;
        CHECK(sr_mesh_frame_host(m.v.data(), nv, m.i.data(), ni, pos.data(), flags, out.data(), &bad) == SR_OK && bad == 0xFFFFFFFFu);
        for (uint32_t k = 0; k < nv; k++) {
            CHECK(memcmp(out[k].position, &pos[3 * (size_t)k], 12) == 0 && memcmp(&out[k].tangent[3], &m.v[k].tangent[3], sizeof(SrVertex) - offsetof(SrVertex, tangent) - 12) == 0);
            const float* q = out[k].normal;
            const float len2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
            CHECK(memcmp(q, m.v[k].normal, 12) == 0 || std::fabs(len2 - 1.0f) < 1e-5f);
            if (flags == SR_FRAME_NORMALS) CHECK(memcmp(out[k].tangent, m.v[k].tangent, 16) == 0);
        }
        if (nv) {
            pos[3 * (size_t)(nv - 1) + 1] = INFINITY;
            CHECK(sr_mesh_frame_host(m.v.data(), nv, m.i.data(), ni, pos.data(), flags, out.data(), &bad) == SR_ERR_INVALID_ARG && bad == nv - 1);
            CHECK(sr_mesh_frame_host(m.v.data(), nv, m.i.data(), ni, pos.data(), flags, out.data(), nullptr) == SR_ERR_INVALID_ARG);
            pos[3 * (size_t)(nv - 1) + 1] = 0.5f;
        }
    }
}

static void run_refused(const Mesh& good) {
    const uint32_t nv = (uint32_t)good.v.size(), ni = (uint32_t)good.i.size();
    uint32_t n = 77;
    std::vector<uint32_t> offsets((size_t)nv + 1, 9u), entries(ni, 9u);
    std::vector<float> side(nv, 9.0f), pos((size_t)nv * 3, 0.25f);
    std::vector<SrVertex> out(nv);
    // an index out of range, first, in the middle and last; the lowest is named
    for (uint32_t at : {0u, ni / 2, ni - 1}) {
        Mesh m = good;
        m.i[at] = nv;
        m.i[ni - 1] = 0xFFFFFFFFu;
        CHECK(sr_mesh_frame_adjacency(m.v.data(), nv, m.i.data(), ni, offsets.data(), entries.data(), side.data(), &n) == SR_ERR_INVALID_ARG);
        char want[64];
        snprintf(want, sizeof(want), "position %u of", at);
        CHECK(g_error.find(want) != std::string::npos && n == 77 && offsets[0] == 9u && entries[0] == 9u && side[0] == 9.0f);
        CHECK(sr_mesh_frame_host(m.v.data(), nv, m.i.data(), ni, pos.data(), SR_FRAME_NORMALS, out.data(), nullptr) == SR_ERR_INVALID_ARG);
    }
    for (uint32_t cut : {1u, 2u}) {
        CHECK(sr_mesh_frame_adjacency(good.v.data(), nv, good.i.data(), ni - cut, offsets.data(), entries.data(), side.data(), &n) == SR_ERR_INVALID_ARG);
        CHECK(sr_mesh_frame_host(good.v.data(), nv, good.i.data(), ni - cut, pos.data(), 3, out.data(), nullptr) == SR_ERR_INVALID_ARG);
    }
    // zero vertices: no index is in range; with no indices either the mesh is empty and fine
    CHECK(sr_mesh_frame_adjacency(good.v.data(), 0, good.i.data(), ni, offsets.data(), entries.data(), side.data(), &n) == SR_ERR_INVALID_ARG);
    CHECK(sr_mesh_frame_adjacency(nullptr, 0, good.i.data(), 3, nullptr, nullptr, nullptr, &n) == SR_ERR_INVALID_ARG);
    CHECK(sr_mesh_frame_adjacency(nullptr, 0, nullptr, 0, offsets.data(), nullptr, nullptr, &n) == SR_OK && n == 0 && offsets[0] == 0);
    CHECK(sr_mesh_frame_host(nullptr, 0, nullptr, 0, nullptr, SR_FRAME_NORMALS, nullptr, nullptr) == SR_OK);
    CHECK(sr_mesh_frame_adjacency(good.v.data(), nv, nullptr, 0, offsets.data(), nullptr, side.data(), &n) == SR_OK && n == 0 && offsets[nv] == 0);   // vertices, no triangle
    CHECK(sr_mesh_frame_adjacency(nullptr, nv, good.i.data(), ni, nullptr, nullptr, nullptr, &n) == SR_ERR_INVALID_ARG);
    CHECK(sr_mesh_frame_adjacency(good.v.data(), nv, nullptr, ni, nullptr, nullptr, nullptr, &n) == SR_ERR_INVALID_ARG);
    for (uint32_t flags : {0u, 2u, 4u, 0x80000001u})
        CHECK(sr_mesh_frame_host(good.v.data(), nv, good.i.data(), ni, pos.data(), flags, out.data(), nullptr) == SR_ERR_INVALID_ARG);
    CHECK(sr_mesh_frame_host(good.v.data(), nv, good.i.data(), ni, nullptr, 1, out.data(), nullptr) == SR_ERR_INVALID_ARG);
    CHECK(sr_mesh_frame_host(good.v.data(), nv, good.i.data(), ni, pos.data(), 1, nullptr, nullptr) == SR_ERR_INVALID_ARG);
}

int main(int argc, char** argv) {
    const int n_random = argc > 1 ? atoi(argv[1]) : 300;
    std::vector<Mesh> meshes;
    {   // a single triangle
        Mesh m;
        m.v = {vertex(-1, -1, 0, 0, 0, 1, 0, 0), vertex(1, -1, 0.25f, 0, 0, 1, 1, 0), vertex(0, 1, 0, 0, 0, 1, 0, 1)};
        m.i = {0, 1, 2};
        meshes.push_back(m);
    }
    {   // two quads folded along a hard edge: equal positions, other normals
        Mesh m;
        m.v = {vertex(0, 0, 0, 0, 0, 1, 0, 0), vertex(1, 0, 0, 0, 0, 1, 1, 0), vertex(1, 1, 0, 0, 0, 1, 1, 1), vertex(0, 1, 0, 0, 0, 1, 0, 1),
               vertex(1, 0, 0, 1, 0, 0, 0, 0), vertex(1, 0, -1, 1, 0, 0, 1, 0), vertex(1, 1, -1, 1, 0, 0, 1, 1), vertex(1, 1, 0, 1, 0, 0, 0, 1)};
        m.i = {0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7};
        meshes.push_back(m);
    }
    {   // a closed strip with a uv seam: the first column again at the end, equal position and normal, other u; the winding opposes the normals
        Mesh m;
        const int seg = 9;
        for (int s = 0; s <= seg; s++) {
            const float a = 6.2831853f * (float)(s % seg) / seg, c = std::cos(a), sn = std::sin(a);
            m.v.push_back(vertex(c, 0, sn, -c, 0, -sn, (float)s / seg, 0));
            m.v.push_back(vertex(c, 1, sn, -c, 0, -sn, (float)s / seg, 1));
        }
        for (uint32_t s = 0; s < (uint32_t)seg; s++) { const uint32_t a = 2 * s; for (uint32_t k : {a, a + 1, a + 3, a, a + 3, a + 2}) m.i.push_back(k); }
        meshes.push_back(m);
    }
    {   // a fan whose hub has 300 entries
        Mesh m;
        const uint32_t n = 300;
        m.v.push_back(vertex(0, 0, 0.3f, 0, 0, 1, 0.5f, 0.5f));
        for (uint32_t k = 0; k < n; k++) { const float a = 6.2831853f * (float)k / n; m.v.push_back(vertex(std::cos(a), std::sin(a), 0, 0, 0, 1, 0.5f + 0.5f * std::cos(a), 0.5f + 0.5f * std::sin(a))); }
        for (uint32_t k = 0; k < n; k++) { m.i.push_back(0); m.i.push_back(1 + k); m.i.push_back(1 + (k + 1) % n); }
        meshes.push_back(m);
    }
    {   // an unreferenced vertex, repeated indices, all-zero uvs, a NaN normal
        Mesh m;
        m.v = {vertex(-1, -1, 0, 0, 0, 1, 0, 0), vertex(1, -1, 0, 0, 0, 1, 0, 0), vertex(1, 1, 0.2f, 0, 0, 1, 0, 0), vertex(-1, 1, 0, NAN, 0, 1, 0, 0), vertex(5, 5, 5, 0, 0, 1, 0, 0)};
        m.i = {0, 1, 2, 0, 2, 3, 0, 0, 1, 2, 2, 2};
        meshes.push_back(m);
    }
    for (const Mesh& m : meshes) run_valid(m);
    run_refused(meshes[1]);
    for (int r = 0; r < n_random; r++) {
        Mesh m;
        const uint32_t nv = 1 + rnd() % 24, nt = rnd() % 40;
        for (uint32_t k = 0; k < nv; k++) {
            const float x = (float)(rnd() % 4), y = (float)(rnd() % 3), z = 0.5f * (float)(rnd() % 3);
            m.v.push_back(vertex(x, y, z, 0, (rnd() % 3) ? 1.0f : -1.0f, 0, 0.25f * (float)(rnd() % 5), 0.25f * (float)(rnd() % 5)));
        }
        for (uint32_t k = 0; k < 3 * nt; k++) m.i.push_back(rnd() % nv);
        run_valid(m);
    }
    if (g_failures) { printf("mesh_frame: %d checks failed\n", g_failures); return 1; }
    printf("mesh_frame ok: %d hand-made meshes, %d random meshes\n", (int)meshes.size(), n_random);
    return 0;
}
