// Sanitizer driver for CUBICSPLINE sampling (tests/test_clip_spline_sanitizers.py): the loader under SR_CUBICSPLINE_SAMPLE and
// the host rule over baked cubic clips. Built with g++ -fsanitize=address,undefined from the loader's host sources and
// clip_host.cpp; usage: clip_spline_asan SPLINE_RIG SKINNED_BAR MORPH_BAR
//   SPLINE_RIG   refused by default and again once the mode is set back; under SAMPLE the bit chain: sr_clip_sample_host ==
//                sr_gltf_sample_node, sr_clip_pose_host == sr_gltf_pose, sr_clip_weights_host == sr_gltf_morph_weights, and the
//                blend host rules at the end weights against the unblended ones for (cubic, linear), (linear, cubic), (cubic, cubic)
//   SKINNED_BAR  animation 1 (a cubic rotation): the chain
//   MORPH_BAR    animation 1 (cubic weights): the chain; a clip baked under REFUSE keeps the set unavailable
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
static std::string g_words;
namespace srh { int set_error(int code, const std::string& msg) { g_words = msg; return code; } }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_words.c_str()); return 1; } } while (0)

static const char* kCubic = "CUBICSPLINE animation samplers are not supported";
static unsigned g_samples = 0, g_weights = 0;

// The four calls refuse animation `anim` of `g` in the kept words.
static int refuses(SrGltf* g, int32_t anim, uint32_t morphed_blas, uint32_t n_targets) {
    float t[3], q[4], s[3], w[8];
    std::vector<SrTransform> xf(64);
    SrClip* clip = nullptr;
    g_words.clear();
    CHECK(sr_gltf_pose(g, anim, 0.5f, xf.data(), 0, nullptr) == SR_ERR_UNSUPPORTED && g_words.find(kCubic) != std::string::npos);
    CHECK(sr_gltf_sample_node(g, anim, 0.5f, 1, t, q, s, nullptr) == SR_ERR_UNSUPPORTED && g_words.find(kCubic) != std::string::npos);
    CHECK(sr_gltf_morph_weights(g, anim, 0.5f, morphed_blas, w, n_targets) == SR_ERR_UNSUPPORTED && g_words.find(kCubic) != std::string::npos);
    CHECK(sr_gltf_bake_clip(g, anim, &clip) == SR_ERR_UNSUPPORTED && clip == nullptr && g_words.find(kCubic) != std::string::npos);
    return 0;
}

// The chain for one animation of one file under SAMPLE over a grid of times.
static int chain(SrGltf* g, int32_t anim, uint32_t n_skins, uint32_t n_blases) {
    SrClip* clip = nullptr;
    CHECK(sr_gltf_bake_clip(g, anim, &clip) == 0);
    SrClipInfo info;
    CHECK(sr_clip_info(clip, &info) == 0);
    std::vector<SrClipNodeInfo> nodes(info.n_nodes + 1);
    CHECK(sr_clip_layout(clip, nodes.data(), nullptr, nullptr) == 0);
    std::vector<SrNodeTrs> trs(info.n_nodes + 1);
    std::vector<SrTransform> jm(info.n_joints + 1), xf(info.n_instances + 1), gx(info.n_instances + 1), gj(info.n_joints + 1);
    std::vector<float> times = {-1.0f, 0.0f, info.duration_seconds + 1.5f};
    for (uint32_t c = 0; c < info.n_channels; c++) {
        const float* kt = nullptr; const float* kv = nullptr;
        std::vector<SrClipChannelInfo> chans(info.n_channels);
        CHECK(sr_clip_layout(clip, nullptr, chans.data(), nullptr) == 0 && sr_clip_channel_keys(clip, c, &kt, &kv) == 0);
        for (uint32_t k = 0; k < chans[c].n_keys; k++) {
            times.push_back(kt[k]); times.push_back(std::nextafter(kt[k], INFINITY)); times.push_back(std::nextafter(kt[k], -INFINITY));
            if (k + 1 < chans[c].n_keys) times.push_back(kt[k] + 0.5f * (kt[k + 1] - kt[k]));
        }
    }
    for (float t : times) {
        CHECK(sr_clip_sample_host(clip, t, trs.data()) == 0);
        for (uint32_t n = 0; n < info.n_nodes; n++) {
            float tr[3], q[4], s[3]; uint32_t mask = 0;
            CHECK(sr_gltf_sample_node(g, anim, t, nodes[n].gltf_node, tr, q, s, &mask) == 0);
            CHECK(memcmp(tr, trs[n].translation, 12) == 0 && memcmp(q, trs[n].rotation, 16) == 0 && memcmp(s, trs[n].scale, 12) == 0 && mask == trs[n].animated);
            g_samples++;
        }
        CHECK(sr_clip_pose_host(clip, t, nullptr, jm.data(), xf.data()) == 0);
        for (uint32_t skin = 0; skin < n_skins; skin++) {
            uint32_t first = 0, nj = 0;
            CHECK(sr_clip_skin(clip, skin, &first, &nj) == 0);
            CHECK(sr_gltf_pose(g, anim, t, gx.data(), skin, gj.data()) == 0);
            CHECK(memcmp(gx.data(), xf.data(), 48 * (size_t)info.n_instances) == 0 && memcmp(gj.data(), jm.data() + first, 48 * (size_t)nj) == 0);
        }
        for (uint32_t b = 0; b < n_blases; b++) {
            uint32_t nt = 0;
            CHECK(sr_gltf_blas_morph(g, b, &nt, nullptr, nullptr, nullptr) == 0);
            if (!nt) continue;
            std::vector<float> wa(nt), wb(nt);
            CHECK(sr_gltf_morph_weights(g, anim, t, b, wa.data(), nt) == 0 && sr_clip_weights_host(clip, t, b, wb.data(), nt) == 0);
            CHECK(memcmp(wa.data(), wb.data(), 4 * (size_t)nt) == 0);
            g_weights++;
        }
    }
    sr_clip_destroy(clip);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: clip_spline_asan SPLINE_RIG SKINNED_BAR MORPH_BAR\n"); return 2; }
    SrGltf* rig = nullptr; SrGltf* bar = nullptr; SrGltf* morph = nullptr;
    CHECK(sr_gltf_open(argv[1], &rig) == 0 && sr_gltf_open(argv[2], &bar) == 0 && sr_gltf_open(argv[3], &morph) == 0);
    uint32_t n_blases = 0, mode = 7, n_trs = 0, n_w = 0;
    CHECK(sr_gltf_counts(rig, &n_blases, nullptr, nullptr, nullptr, nullptr) == 0 && n_blases == 4);
    CHECK(sr_gltf_cubicspline(rig, &mode) == 0 && mode == SR_CUBICSPLINE_REFUSE);
    CHECK(sr_gltf_animation_cubic(rig, 0, &n_trs, &n_w) == 0 && n_trs == 6 && n_w == 1);
    CHECK(sr_gltf_animation_cubic(rig, 1, &n_trs, &n_w) == 0 && n_trs == 0 && n_w == 0);
    CHECK(sr_gltf_set_cubicspline(rig, 2) == SR_ERR_INVALID_ARG && sr_gltf_set_cubicspline(nullptr, 1) == SR_ERR_INVALID_ARG);
    if (refuses(rig, 0, 3, 3)) return 1;
    CHECK(sr_gltf_set_cubicspline(rig, SR_CUBICSPLINE_SAMPLE) == 0 && sr_gltf_cubicspline(rig, &mode) == 0 && mode == SR_CUBICSPLINE_SAMPLE);
    for (int32_t anim : {0, 1, 2, -1}) if (chain(rig, anim, 2, n_blases)) return 1;
    // the blend host rules at the end weights, for the three pairings
    SrClip* cubic = nullptr; SrClip* linear = nullptr;
    CHECK(sr_gltf_bake_clip(rig, 0, &cubic) == 0 && sr_gltf_bake_clip(rig, 1, &linear) == 0);
    SrClipInfo info;
    CHECK(sr_clip_info(cubic, &info) == 0);
    SrClip* pairs[3][2] = {{cubic, linear}, {linear, cubic}, {cubic, cubic}};
    for (auto& p : pairs) {
        CHECK(sr_clip_blend_compatible(p[0], p[1]) == 0);
        std::vector<SrTransform> jm(info.n_joints), xf(info.n_instances), wj(info.n_joints), wx(info.n_instances);
        float got[3], want[3];
        for (float ta : {0.3f, 0.625f, 1.0f, 2.5f}) for (float tb : {-1.0f, 0.25f, 1.7f}) for (int end = 0; end < 2; end++) {
            CHECK(sr_clip_pose_blend_host(p[0], ta, p[1], tb, (float)end, nullptr, jm.data(), xf.data()) == 0);
            CHECK(sr_clip_pose_host(p[end], end ? tb : ta, nullptr, wj.data(), wx.data()) == 0);
            CHECK(memcmp(jm.data(), wj.data(), 48 * jm.size()) == 0 && memcmp(xf.data(), wx.data(), 48 * xf.size()) == 0);
            CHECK(sr_clip_blend_weights_host(p[0], ta, p[1], tb, (float)end, 3, got, 3) == 0 && sr_clip_weights_host(p[end], end ? tb : ta, 3, want, 3) == 0);
            CHECK(memcmp(got, want, 12) == 0);
            CHECK(sr_clip_pose_blend_host(p[0], ta, p[1], tb, 0.5f, nullptr, jm.data(), xf.data()) == 0);
            CHECK(sr_clip_blend_weights_host(p[0], ta, p[1], tb, 1.0f / 3.0f, 3, got, 3) == 0);
        }
    }
    // the mode set back: refused again; the clips keep what they were baked with
    CHECK(sr_gltf_set_cubicspline(rig, SR_CUBICSPLINE_REFUSE) == 0);
    if (refuses(rig, 0, 3, 3)) return 1;
    { float w[3]; CHECK(sr_clip_weights_host(cubic, 0.7f, 3, w, 3) == 0); }
    sr_clip_destroy(cubic); sr_clip_destroy(linear);
    // the other two fixtures
    CHECK(sr_gltf_set_cubicspline(bar, SR_CUBICSPLINE_SAMPLE) == 0);
    CHECK(sr_gltf_counts(bar, &n_blases, nullptr, nullptr, nullptr, nullptr) == 0);
    if (chain(bar, 1, 1, n_blases)) return 1;
    SrClip* refused_set = nullptr;
    SrClipMorphInfo mi;
    CHECK(sr_gltf_bake_clip(morph, 1, &refused_set) == 0 && sr_clip_morph(refused_set, 0, &mi) == 0 && mi.state == SR_CLIP_MORPH_UNAVAILABLE);
    CHECK(sr_gltf_set_cubicspline(morph, SR_CUBICSPLINE_SAMPLE) == 0);
    CHECK(sr_gltf_counts(morph, &n_blases, nullptr, nullptr, nullptr, nullptr) == 0);
    if (chain(morph, 1, 1, n_blases)) return 1;
    { float w[3]; g_words.clear(); CHECK(sr_clip_weights_host(refused_set, 0.5f, 0, w, 3) == SR_ERR_UNSUPPORTED && g_words.find(kCubic) != std::string::npos); }
    sr_clip_destroy(refused_set);
    sr_gltf_close(rig); sr_gltf_close(bar); sr_gltf_close(morph);
    printf("clip spline ok: %u node samples, %u weight vectors\n", g_samples, g_weights);
    return 0;
}
