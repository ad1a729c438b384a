// Host side of the mesh-frame producer (mesh_frame.h): smoothing groups, the per-vertex runs, and the whole rule on the host.
// fp32 under the numerics contract of DESIGN.md §3 (built with -ffp-contract=off): every operation below is one IEEE operation,
// grouped as include/sunray_hip.h writes it, and normals.hip does the same operations in the same order.
#include "mesh_frame.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace {

struct V3 { float x, y, z; };

V3 sub3(const float* a, const float* b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
V3 cross3(const V3& a, const V3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 add3(const V3& a, const V3& b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// F and T of triangle t from positions `p` (`stride` floats from one vertex to the next)
void face_vectors(const float* p, size_t stride, const uint32_t* indices, uint32_t t, const srh::FrameTriUv& uv, V3* F, V3* T) {
    const float* p0 = p + stride * indices[3 * (size_t)t];
    const V3 e1 = sub3(p + stride * indices[3 * (size_t)t + 1], p0), e2 = sub3(p + stride * indices[3 * (size_t)t + 2], p0);
    *F = cross3(e1, e2);
    if (!T) return;
    if (uv.s == 0.0f) { *T = {0.0f, 0.0f, 0.0f}; return; }
    *T = {uv.s * (e1.x * uv.by - e2.x * uv.ay), uv.s * (e1.y * uv.by - e2.y * uv.ay), uv.s * (e1.z * uv.by - e2.z * uv.ay)};
}

// v * (1 / sqrt(dot(v, v))) into dst[0..2]; a squared length that is 0 or not finite leaves dst alone (store_normalised, vertex_tile.h)
void store_normalised(float* dst, float x, float y, float z) {
    const float len2 = (x * x + y * y) + z * z;
    if (len2 == 0.0f || !std::isfinite(len2)) return;
    const float r = 1.0f / sqrtf(len2);
    dst[0] = x * r; dst[1] = y * r; dst[2] = z * r;
}

int check_arrays(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, const char* who) {
    char buf[200];
    if ((n_vertices && !vertices) || (n_indices && !indices)) return srh::set_error(SR_ERR_INVALID_ARG, std::string(who) + ": null argument (an array that is not empty)");
    if (n_indices % 3 != 0) {
        snprintf(buf, sizeof(buf), "%s: %u indices are not a triangle list (n_indices %% 3 != 0)", who, n_indices);
        return srh::set_error(SR_ERR_INVALID_ARG, buf);
    }
    for (uint32_t k = 0; k < n_indices; k++)
        if (indices[k] >= n_vertices) {
            snprintf(buf, sizeof(buf), "%s: index %u (at position %u of the index buffer) is out of range for %u vertices", who, indices[k], k, n_vertices);
            return srh::set_error(SR_ERR_INVALID_ARG, buf);
        }
    return SR_OK;
}

}  // namespace

int srh::mesh_frame_build(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, bool count_only,
                          MeshFrame& out, uint64_t* n_entries, const char* who) {
    if (const int rc = check_arrays(vertices, n_vertices, indices, n_indices, who); rc != SR_OK) return rc;
    out = MeshFrame();
    // groups: equal 12 bytes of position and 12 bytes of normal; the group's number follows its lowest vertex
    std::vector<uint32_t> order(n_vertices), group(n_vertices);
    std::iota(order.begin(), order.end(), 0u);
    const auto key_cmp = [&](uint32_t a, uint32_t b) {
        const int p = memcmp(vertices[a].position, vertices[b].position, 12);
        return p != 0 ? p : memcmp(vertices[a].normal, vertices[b].normal, 12);
    };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { const int c = key_cmp(a, b); return c != 0 ? c < 0 : a < b; });
    uint32_t n_groups = 0;
    for (uint32_t k = 0; k < n_vertices; k++) {
        if (k == 0 || key_cmp(order[k - 1], order[k]) != 0) n_groups++;
        group[order[k]] = n_groups - 1;
    }
    out.n_groups = n_groups;
    // the corners of every group, ascending (t, c): the index buffer is walked in that order
    std::vector<uint32_t> g_off((size_t)n_groups + 1, 0);
    for (uint32_t k = 0; k < n_indices; k++) g_off[(size_t)group[indices[k]] + 1]++;
    for (uint32_t g = 0; g < n_groups; g++) g_off[(size_t)g + 1] += g_off[g];
    uint64_t total = 0;
    for (uint32_t v = 0; v < n_vertices; v++) {
        const uint32_t c = g_off[(size_t)group[v] + 1] - g_off[group[v]];
        total += c;
        out.max_valence = std::max(out.max_valence, c);
    }
    if (n_entries) *n_entries = total;
    if (total > 0xFFFFFFFFull) return srh::set_error(SR_ERR_OOM, std::string(who) + ": the runs of all vertices together exceed 2^32 - 1 entries");
    if (count_only) return SR_OK;
    std::vector<uint32_t> g_entries(n_indices), fill(g_off.begin(), g_off.end() - 1);
    for (uint32_t k = 0; k < n_indices; k++) g_entries[fill[group[indices[k]]]++] = k / 3;
    const uint32_t n_tris = n_indices / 3;
    out.tri_uv.resize(n_tris);
    for (uint32_t t = 0; t < n_tris; t++) {
        const float* u0 = vertices[indices[3 * (size_t)t]].normal_tex_coord;
        const float* u1 = vertices[indices[3 * (size_t)t + 1]].normal_tex_coord;
        const float* u2 = vertices[indices[3 * (size_t)t + 2]].normal_tex_coord;
        const float ax = u1[0] - u0[0], ay = u1[1] - u0[1], bx = u2[0] - u0[0], by = u2[1] - u0[1];
        const float det = ax * by - bx * ay;
        out.tri_uv[t] = {ay, by, (det == 0.0f || !std::isfinite(det)) ? 0.0f : (det > 0.0f ? 1.0f : -1.0f), 0.0f};
    }
    // side, per group from the reference positions by the rule's own accumulation
    std::vector<float> g_side(n_groups, 1.0f);
    std::vector<uint32_t> g_first(n_groups, 0xFFFFFFFFu);
    for (uint32_t v = n_vertices; v-- > 0;) g_first[group[v]] = v;
    for (uint32_t g = 0; g < n_groups; g++) {
        V3 N = {0.0f, 0.0f, 0.0f}, F;
        for (uint32_t e = g_off[g]; e < g_off[(size_t)g + 1]; e++) {
            face_vectors(vertices[0].position, sizeof(SrVertex) / 4, indices, g_entries[e], out.tri_uv[g_entries[e]], &F, nullptr);
            N = add3(N, F);
        }
        const float* n = vertices[g_first[g]].normal;
        if ((N.x * n[0] + N.y * n[1]) + N.z * n[2] < 0.0f) g_side[g] = -1.0f;
    }
    out.offsets.resize((size_t)n_vertices + 1);
    out.entries.resize((size_t)total);
    out.side.resize(n_vertices);
    out.offsets[0] = 0;
    for (uint32_t v = 0; v < n_vertices; v++) {
        const uint32_t g = group[v], c = g_off[(size_t)g + 1] - g_off[g];
        if (c) memcpy(&out.entries[out.offsets[v]], &g_entries[g_off[g]], 4 * (size_t)c);
        out.offsets[(size_t)v + 1] = out.offsets[v] + c;
        out.side[v] = g_side[g];
    }
    return SR_OK;
}

extern "C" {

int sr_mesh_frame_adjacency(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, uint32_t* offsets_out,
                            uint32_t* entries_out, float* side_out, uint32_t* n_entries_out) {
    srh::MeshFrame f;
    uint64_t total = 0;
    const bool count_only = !offsets_out && !entries_out && !side_out;
    const int rc = srh::mesh_frame_build(vertices, n_vertices, indices, n_indices, count_only, f, &total, "sr_mesh_frame_adjacency");
    if (rc != SR_OK) return rc;
    if (n_entries_out) *n_entries_out = (uint32_t)total;
    if (offsets_out) memcpy(offsets_out, f.offsets.data(), 4 * f.offsets.size());
    if (entries_out && !f.entries.empty()) memcpy(entries_out, f.entries.data(), 4 * f.entries.size());
    if (side_out && !f.side.empty()) memcpy(side_out, f.side.data(), 4 * f.side.size());
    return SR_OK;
}

int sr_mesh_frame_host(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, const float* positions,
                       uint32_t flags, SrVertex* out_vertices, uint32_t* first_bad_out) {
    const char* const who = "sr_mesh_frame_host";
    if (first_bad_out) *first_bad_out = 0xFFFFFFFFu;
    if (n_vertices && (!positions || !out_vertices)) return srh::set_error(SR_ERR_INVALID_ARG, std::string(who) + ": null argument (positions or out_vertices)");
    if (flags == 0 || (flags & ~(SR_FRAME_NORMALS | SR_FRAME_TANGENTS))) return srh::set_error(SR_ERR_INVALID_ARG, std::string(who) + ": flags must be SR_FRAME_NORMALS, with or without SR_FRAME_TANGENTS");
    if (!(flags & SR_FRAME_NORMALS)) return srh::set_error(SR_ERR_INVALID_ARG, std::string(who) + ": SR_FRAME_TANGENTS needs SR_FRAME_NORMALS (the tangent is made orthogonal to the new normal)");
    srh::MeshFrame f;
    int rc = srh::mesh_frame_build(vertices, n_vertices, indices, n_indices, false, f, nullptr, who);
    if (rc != SR_OK) return rc;
    for (uint32_t v = 0; v < n_vertices; v++)
        if (!finite3(positions + 3 * (size_t)v)) {
            if (first_bad_out) *first_bad_out = v;
            char buf[120];
            snprintf(buf, sizeof(buf), "%s: vertex %u has a non-finite position", who, v);
            return srh::set_error(SR_ERR_INVALID_ARG, buf);
        }
    const bool tangents = (flags & SR_FRAME_TANGENTS) != 0;
    const uint32_t n_tris = n_indices / 3;
    std::vector<V3> F(n_tris), T(tangents ? n_tris : 0);
    for (uint32_t t = 0; t < n_tris; t++) face_vectors(positions, 3, indices, t, f.tri_uv[t], &F[t], tangents ? &T[t] : nullptr);
    for (uint32_t v = 0; v < n_vertices; v++) {
        V3 N = {0.0f, 0.0f, 0.0f}, A = {0.0f, 0.0f, 0.0f};
        for (uint32_t e = f.offsets[v]; e < f.offsets[(size_t)v + 1]; e++) {
            N = add3(N, F[f.entries[e]]);
            if (tangents) A = add3(A, T[f.entries[e]]);
        }
        SrVertex o = vertices[v];
        memcpy(o.position, positions + 3 * (size_t)v, 12);
        const float side = f.side[v];
        store_normalised(o.normal, side * N.x, side * N.y, side * N.z);
        if (tangents) {
            const float* n = o.normal;                       // the new normal, or the reference's where it fell back
            const float d = (n[0] * A.x + n[1] * A.y) + n[2] * A.z;
            store_normalised(o.tangent, A.x - n[0] * d, A.y - n[1] * d, A.z - n[2] * d);
        }
        out_vertices[v] = o;
    }
    return SR_OK;
}

}  // extern "C"
