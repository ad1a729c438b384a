// Sanitizer driver for cross-fades between baked clips (tests/test_clip_blend_sanitizers.py): sr_clip_blend_compatible and the
// host rule of the blend. Built with g++ -fsanitize=address,undefined from the loader's host sources and clip_host.cpp; usage:
// clip_blend_asan CLIP_RIG SKINNED_BAR MORPH_BAR
//   CLIP_RIG     every ordered pair of its bakes (-1, 0, 1) is compatible; at the end weights sr_clip_pose_blend_host gives
//                sr_clip_pose_host's bytes for the one clip, and a clip blended with itself at one time gives them at every
//                weight; weights outside [0, 1], NaN and times that are not finite are refused
//   SKINNED_BAR  its bakes are refused against CLIP_RIG's, in words that name a table
//   MORPH_BAR    the blended weights at the end weights are sr_clip_weights_host's; the CUBICSPLINE set is refused as either source
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
static std::string g_words;
namespace srh { int set_error(int code, const std::string& msg) { g_words = msg; return code; } }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Pose { int rc; std::vector<SrTransform> jm, xf; };
static bool same(const Pose& a, const Pose& b) {
    if (a.rc != b.rc) return false;
    if (a.rc != 0) return true;
    return memcmp(a.jm.data(), b.jm.data(), 48 * a.jm.size()) == 0 && memcmp(a.xf.data(), b.xf.data(), 48 * a.xf.size()) == 0;
}
static Pose plain(const SrClip* c, float t, const SrTransform* placement, const SrClipInfo& i) {
    Pose p{0, std::vector<SrTransform>(i.n_joints + 1), std::vector<SrTransform>(i.n_instances + 1)};
    p.rc = sr_clip_pose_host(c, t, placement, p.jm.data(), p.xf.data());
    return p;
}
static Pose blended(const SrClip* a, float ta, const SrClip* b, float tb, float w, const SrTransform* placement, const SrClipInfo& i) {
    Pose p{0, std::vector<SrTransform>(i.n_joints + 1), std::vector<SrTransform>(i.n_instances + 1)};
    p.rc = sr_clip_pose_blend_host(a, ta, b, tb, w, placement, p.jm.data(), p.xf.data());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: clip_blend_asan CLIP_RIG SKINNED_BAR MORPH_BAR\n"); return 2; }
    SrGltf* rig = nullptr; SrGltf* bar = nullptr; SrGltf* morph = nullptr;
    CHECK(sr_gltf_open(argv[1], &rig) == 0 && sr_gltf_open(argv[2], &bar) == 0 && sr_gltf_open(argv[3], &morph) == 0);
    SrClip* clips[3]; SrClipInfo info[3];
    for (int a = 0; a < 3; a++) { CHECK(sr_gltf_bake_clip(rig, a - 1, &clips[a]) == 0); sr_clip_info(clips[a], &info[a]); }
    const SrTransform placement = {{1, 0, 0, 2, 0, 1, 0, -1, 0, 0, 1, 0.5f}};
    const float weights[] = {0.0f, 1.0f, std::nextafter(0.0f, 1.0f), std::nextafter(1.0f, 0.0f), 0.5f, 1.0f / 3.0f};
    unsigned n_poses = 0;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
        CHECK(sr_clip_blend_compatible(clips[a], clips[b]) == 0);
        const float times_a[] = {-1.0f, 0.0f, 0.37f * info[a].duration_seconds, 0.9f, info[a].duration_seconds, 2.0f * info[a].duration_seconds + 1.0f};
        const float times_b[] = {0.25f, 1.0f, 0.61f * info[b].duration_seconds, info[b].duration_seconds + 3.0f};      // 1.0: animation 1 is singular there
        for (float ta : times_a) for (float tb : times_b) for (const SrTransform* pl : {(const SrTransform*)nullptr, &placement}) {
            CHECK(same(blended(clips[a], ta, clips[b], tb, 0.0f, pl, info[a]), plain(clips[a], ta, pl, info[a])));      // item 2: the end weights
            CHECK(same(blended(clips[a], ta, clips[b], tb, 1.0f, pl, info[a]), plain(clips[b], tb, pl, info[b])));
            for (float w : weights) { blended(clips[a], ta, clips[b], tb, w, pl, info[a]); n_poses++; }
        }
        for (float ta : times_a) for (float w : weights)                                                             // item 3: the same clip at the same time
            CHECK(same(blended(clips[a], ta, clips[a], ta, w, &placement, info[a]), plain(clips[a], ta, &placement, info[a])));
        // the refusals
        std::vector<SrTransform> xf(info[a].n_instances + 1);
        for (float w : {-0.1f, 1.5f, NAN, INFINITY}) CHECK(sr_clip_pose_blend_host(clips[a], 0.5f, clips[b], 0.5f, w, nullptr, nullptr, xf.data()) == SR_ERR_INVALID_ARG);
        if (a > 0) CHECK(sr_clip_pose_blend_host(clips[a], NAN, clips[b], 0.5f, 0.5f, nullptr, nullptr, xf.data()) == SR_ERR_INVALID_ARG);
        if (b > 0) CHECK(sr_clip_pose_blend_host(clips[a], 0.5f, clips[b], INFINITY, 0.5f, nullptr, nullptr, xf.data()) == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_pose_blend_host(clips[a], 0.5f, nullptr, 0.5f, 0.5f, nullptr, nullptr, xf.data()) == SR_ERR_INVALID_ARG);
    }
    // records: the rule over a sampled pair, composed from the records' own masks
    {
        std::vector<SrNodeTrs> ta(info[1].n_nodes + 1), tb(info[1].n_nodes + 1), out(info[1].n_nodes + 1);
        std::vector<SrTransform> jm(info[1].n_joints + 1), xf(info[1].n_instances + 1), jm2(info[1].n_joints + 1), xf2(info[1].n_instances + 1);
        CHECK(sr_clip_sample_host(clips[1], 0.9f, ta.data()) == 0 && sr_clip_sample_host(clips[2], 0.25f, tb.data()) == 0);
        CHECK(sr_clip_compose_host(clips[1], ta.data(), &placement, jm.data(), xf.data(), nullptr) == 0);
        CHECK(sr_clip_compose_records_host(clips[1], ta.data(), &placement, jm2.data(), xf2.data(), nullptr) == 0);
        CHECK(memcmp(jm.data(), jm2.data(), 48 * (size_t)info[1].n_joints) == 0 && memcmp(xf.data(), xf2.data(), 48 * (size_t)info[1].n_instances) == 0);
        for (float w : weights) {
            uint32_t bad = 0;
            CHECK(sr_clip_blend_host(ta.data(), tb.data(), info[1].n_nodes, w, out.data()) == 0);
            CHECK(sr_clip_compose_records_host(clips[1], out.data(), nullptr, jm.data(), xf.data(), &bad) == 0 && bad == 0xFFFFFFFFu);
        }
        CHECK(sr_clip_blend_host(ta.data(), tb.data(), 0, 0.5f, nullptr) == 0);
        CHECK(sr_clip_blend_host(ta.data(), nullptr, 1, 0.5f, out.data()) == SR_ERR_INVALID_ARG);
    }
    // item 6: another file's bakes are refused, and the words name a table
    for (int32_t anim : {-1, 0}) {
        SrClip* other = nullptr;
        CHECK(sr_gltf_bake_clip(bar, anim, &other) == 0);
        for (int a = 0; a < 3; a++) {
            g_words.clear();
            CHECK(sr_clip_blend_compatible(clips[a], other) == SR_ERR_INVALID_ARG && g_words.find("sr_clip_blend_compatible: the clips differ in the ") == 0);
            CHECK(sr_clip_blend_compatible(other, clips[a]) == SR_ERR_INVALID_ARG);
            std::vector<SrTransform> xf(info[a].n_instances + 8);
            CHECK(sr_clip_pose_blend_host(clips[a], 0.5f, other, 0.5f, 0.5f, nullptr, nullptr, xf.data()) == SR_ERR_INVALID_ARG);
        }
        CHECK(sr_clip_blend_compatible(other, other) == 0);
        sr_clip_destroy(other);
    }
    CHECK(sr_clip_blend_compatible(clips[0], nullptr) == SR_ERR_INVALID_ARG);
    // morph weights: the end weights, the inner weights, the refusals
    SrClip* talk = nullptr; SrClip* still = nullptr; SrClip* spline = nullptr;
    CHECK(sr_gltf_bake_clip(morph, 0, &talk) == 0 && sr_gltf_bake_clip(morph, -1, &still) == 0 && sr_gltf_bake_clip(morph, 1, &spline) == 0);
    unsigned n_weights = 0;
    for (uint32_t blas = 0; blas < 2; blas++) {
        SrClipMorphInfo mi;
        CHECK(sr_clip_morph(talk, blas, &mi) == 0);
        const uint32_t nt = mi.n_targets;
        std::vector<float> wa(nt), wb(nt), got(nt);
        for (float ta : {-1.0f, 0.0f, 0.3f, 1.0f, 1.7f, 9.0f}) for (float tb : {0.0f, 0.9f}) {
            CHECK(sr_clip_weights_host(talk, ta, blas, wa.data(), nt) == 0 && sr_clip_weights_host(still, tb, blas, wb.data(), nt) == 0);
            CHECK(sr_clip_blend_weights_host(talk, ta, still, tb, 0.0f, blas, got.data(), nt) == 0 && memcmp(got.data(), wa.data(), 4 * (size_t)nt) == 0);
            CHECK(sr_clip_blend_weights_host(talk, ta, still, tb, 1.0f, blas, got.data(), nt) == 0 && memcmp(got.data(), wb.data(), 4 * (size_t)nt) == 0);
            for (float w : weights) { CHECK(sr_clip_blend_weights_host(still, tb, talk, ta, w, blas, got.data(), nt) == 0); n_weights++; }
        }
        CHECK(sr_clip_blend_weights_host(talk, 0.5f, still, 0.5f, 0.5f, blas, got.data(), nt + 1) == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_blend_weights_host(talk, 0.5f, still, 0.5f, -1.0f, blas, got.data(), nt) == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_blend_weights_host(talk, NAN, still, 0.5f, 0.5f, blas, got.data(), nt) == SR_ERR_INVALID_ARG);
    }
    {
        float got[8];
        SrClipMorphInfo mi;
        CHECK(sr_clip_morph(talk, 0, &mi) == 0 && mi.n_targets <= 8);
        g_words.clear();
        CHECK(sr_clip_blend_weights_host(spline, 0.5f, talk, 0.5f, 0.5f, 0, got, mi.n_targets) == SR_ERR_UNSUPPORTED && g_words.find("CUBICSPLINE") != std::string::npos);
        CHECK(sr_clip_blend_weights_host(talk, 0.5f, spline, 0.5f, 0.5f, 0, got, mi.n_targets) == SR_ERR_UNSUPPORTED);
        CHECK(sr_clip_blend_weights_host(talk, 0.5f, still, 0.5f, 0.5f, 77, got, 1) == SR_ERR_INVALID_ARG);
    }
    for (SrClip* c : {talk, still, spline, clips[0], clips[1], clips[2]}) sr_clip_destroy(c);
    sr_gltf_close(rig); sr_gltf_close(bar); sr_gltf_close(morph);
    printf("clip blend ok: %u poses, %u weight vectors\n", n_poses, n_weights);
    return 0;
}
