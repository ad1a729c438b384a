// Sanitizer driver for layer stacks of baked clips (tests/test_clip_layers_sanitizers.py): sr_clip_subtree_mask, sr_clip_layers_host
// and sr_clip_pose_layers_host. Built with g++ -fsanitize=address,undefined from the loader's host sources and clip_host.cpp; usage:
// clip_layers_asan CLIP_RIG SKINNED_BAR
//   CLIP_RIG     one layer gives sr_clip_pose_host's bytes, two unmasked override layers sr_clip_pose_blend_host's; a mask of ones
//                is no mask; a mask of zeros, weight 0 and an additive layer at its reference time give the stack below; stacks of
//                1..8 layers with subtree masks and additive layers run over exactly sized buffers; the refusals
//   SKINNED_BAR  its bake is refused as a layer over CLIP_RIG's
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
static std::string g_words;
namespace srh { int set_error(int code, const std::string& msg) { g_words = msg; return code; } }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_words.c_str()); return 1; } } while (0)

struct Pose { int rc; std::vector<SrTransform> jm, xf; };
static bool same(const Pose& a, const Pose& b) {
    return a.rc == 0 && b.rc == 0 && memcmp(a.jm.data(), b.jm.data(), 48 * a.jm.size()) == 0 && memcmp(a.xf.data(), b.xf.data(), 48 * a.xf.size()) == 0;
}
static SrClipLayer layer(float t, float w, uint32_t mode, float ref_t) { return SrClipLayer{0, t, w, mode, SR_LAYER_NO_MASK, ref_t, {0, 0}}; }
static Pose stacked(const std::vector<const SrClip*>& clips, const std::vector<SrClipLayer>& layers, const std::vector<const float*>& masks, const SrTransform* placement,
                    const SrClipInfo& i) {
    Pose p{0, std::vector<SrTransform>(i.n_joints), std::vector<SrTransform>(i.n_instances)};       // exactly sized: a write past the end is caught
    p.rc = sr_clip_pose_layers_host(clips.data(), layers.data(), masks.empty() ? nullptr : masks.data(), (uint32_t)layers.size(), placement, p.jm.data(), p.xf.data());
    return p;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: clip_layers_asan CLIP_RIG SKINNED_BAR\n"); return 2; }
    SrGltf* rig = nullptr; SrGltf* bar = nullptr;
    CHECK(sr_gltf_open(argv[1], &rig) == 0 && sr_gltf_open(argv[2], &bar) == 0);
    SrClip* clips[3]; SrClipInfo info[3];
    for (int a = 0; a < 3; a++) { CHECK(sr_gltf_bake_clip(rig, a - 1, &clips[a]) == 0); sr_clip_info(clips[a], &info[a]); }
    const uint32_t n = info[0].n_nodes;
    const SrTransform placement = {{1, 0, 0, 2, 0, 1, 0, -1, 0, 0, 1, 0.5f}};
    const float weights[] = {0.0f, 1.0f, std::nextafter(0.0f, 1.0f), std::nextafter(1.0f, 0.0f), 0.5f, 1.0f / 3.0f};
    const float times[] = {-1.0f, 0.0f, 0.3f, 0.9f, 1.6f, 7.0f};               // 1.0 is left out: animation 1 is singular there
    std::vector<float> ones(n, 1.0f), zeros(n, 0.0f), subtree(n);
    std::vector<SrClipNodeInfo> nodes(n);
    CHECK(sr_clip_layout(clips[1], nodes.data(), nullptr, nullptr) == 0);
    unsigned n_poses = 0;
    // one layer; two override layers
    for (int a = 0; a < 3; a++) for (float t : times) for (const SrTransform* pl : {(const SrTransform*)nullptr, &placement}) {
        Pose want{0, std::vector<SrTransform>(info[a].n_joints), std::vector<SrTransform>(info[a].n_instances)};
        want.rc = sr_clip_pose_host(clips[a], t, pl, want.jm.data(), want.xf.data());
        CHECK(same(stacked({clips[a]}, {layer(t, 1.0f, SR_LAYER_OVERRIDE, 0.0f)}, {}, pl, info[a]), want));
        for (int b = 0; b < 3; b++) for (float w : weights) {
            Pose blend{0, std::vector<SrTransform>(info[a].n_joints), std::vector<SrTransform>(info[a].n_instances)};
            blend.rc = sr_clip_pose_blend_host(clips[a], t, clips[b], 0.7f, w, pl, blend.jm.data(), blend.xf.data());
            const std::vector<SrClipLayer> two = {layer(t, 1.0f, SR_LAYER_OVERRIDE, 0.0f), layer(0.7f, w, SR_LAYER_OVERRIDE, 0.0f)};
            CHECK(same(stacked({clips[a], clips[b]}, two, {}, pl, info[a]), blend));
            CHECK(same(stacked({clips[a], clips[b]}, two, {nullptr, ones.data()}, pl, info[a]), blend));                       // a mask of ones is no mask
            // what gives the stack below: a mask of zeros, weight 0, an additive layer at its reference time
            std::vector<SrClipLayer> three = two;
            three.push_back(layer(0.4f, 0.5f, SR_LAYER_OVERRIDE, 0.0f));
            CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {nullptr, nullptr, zeros.data()}, pl, info[a]), blend));
            three[2] = layer(0.4f, 0.0f, SR_LAYER_ADDITIVE, 1.3f);
            CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {}, pl, info[a]), blend));
            three[2] = layer(0.4f, w, SR_LAYER_ADDITIVE, 0.4f);
            CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {}, pl, info[a]), blend));
            n_poses += 5;
        }
    }
    // stacks of 1..8 layers with subtree masks and additive layers
    for (uint32_t target = 0; target < n; target++) {
        CHECK(sr_clip_subtree_mask(clips[1], nodes[target].gltf_node, 0.75f, 0.125f, subtree.data(), n) == 0);
        CHECK(subtree[target] == 0.75f);
        for (uint32_t k = 0; k < n; k++) CHECK(subtree[k] == 0.75f || subtree[k] == 0.125f);
        for (uint32_t n_layers = 1; n_layers <= SR_CLIP_MAX_LAYERS; n_layers++) {
            std::vector<const SrClip*> cs; std::vector<SrClipLayer> ls; std::vector<const float*> ms;
            for (uint32_t l = 0; l < n_layers; l++) {
                cs.push_back(clips[(l + target) % 3]);
                ls.push_back(l == 0 ? layer(0.3f, 1.0f, SR_LAYER_OVERRIDE, 0.0f) : layer(times[(l + target) % 6], weights[(l + target) % 6], l % 2 ? SR_LAYER_ADDITIVE : SR_LAYER_OVERRIDE, 0.25f * l));
                ms.push_back(l % 3 == 1 ? subtree.data() : nullptr);
            }
            CHECK(stacked(cs, ls, ms, target % 2 ? &placement : nullptr, info[0]).rc == 0);
            n_poses++;
        }
    }
    // the record rule over exactly sized records
    {
        std::vector<SrNodeTrs> a(n), b(n), c(n), r(n), out(n);
        CHECK(sr_clip_sample_host(clips[1], 0.9f, a.data()) == 0 && sr_clip_sample_host(clips[2], 0.25f, b.data()) == 0);
        CHECK(sr_clip_sample_host(clips[2], 0.6f, c.data()) == 0 && sr_clip_sample_host(clips[2], 1.4f, r.data()) == 0);
        const SrNodeTrs* cur[3] = {a.data(), b.data(), c.data()};
        const SrNodeTrs* ref[3] = {nullptr, nullptr, r.data()};
        SrClipLayerRule rule[3] = {{1.0f, SR_LAYER_OVERRIDE, nullptr}, {0.5f, SR_LAYER_OVERRIDE, subtree.data()}, {0.75f, SR_LAYER_ADDITIVE, nullptr}};
        CHECK(sr_clip_layers_host(cur, ref, rule, 3, n, out.data()) == 0);
        CHECK(sr_clip_layers_host(cur, nullptr, rule, 2, n, out.data()) == 0);
        CHECK(sr_clip_layers_host(cur, nullptr, rule, 3, n, out.data()) == SR_ERR_INVALID_ARG);       // an additive layer without its reference records
        CHECK(sr_clip_layers_host(cur, ref, rule, 0, n, out.data()) == SR_ERR_INVALID_ARG && sr_clip_layers_host(cur, ref, rule, 9, n, out.data()) == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_layers_host(cur, ref, rule, 3, 0, nullptr) == 0);
        for (float w : {-0.1f, 1.5f, NAN, INFINITY}) { rule[1].weight = w; CHECK(sr_clip_layers_host(cur, ref, rule, 3, n, out.data()) == SR_ERR_INVALID_ARG); }
        rule[1].weight = 0.5f; rule[1].mode = 2;
        CHECK(sr_clip_layers_host(cur, ref, rule, 3, n, out.data()) == SR_ERR_INVALID_ARG);
        rule[1].mode = SR_LAYER_OVERRIDE;
        std::vector<float> bad(n, 0.5f);
        for (float v : {-0.5f, 1.0001f, NAN}) { bad[n - 1] = v; rule[1].mask = bad.data(); CHECK(sr_clip_layers_host(cur, ref, rule, 3, n, out.data()) == SR_ERR_INVALID_ARG); }
        rule[1].mask = nullptr; rule[0].weight = 0.5f;
        CHECK(sr_clip_layers_host(cur, ref, rule, 3, n, out.data()) == SR_ERR_INVALID_ARG);
    }
    // the refusals of sample, stack, compose
    {
        const std::vector<SrClipLayer> two = {layer(0.3f, 1.0f, SR_LAYER_OVERRIDE, 0.0f), layer(0.7f, 0.5f, SR_LAYER_OVERRIDE, 0.0f)};
        std::vector<SrClipLayer> l = two;
        l[1].time_seconds = INFINITY;
        CHECK(stacked({clips[1], clips[2]}, l, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);
        l = two; l[1].mode = SR_LAYER_ADDITIVE; l[1].ref_time_seconds = NAN;
        CHECK(stacked({clips[1], clips[2]}, l, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);
        l = two; l[0].mode = SR_LAYER_ADDITIVE;
        CHECK(stacked({clips[1], clips[2]}, l, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);
        CHECK(stacked({clips[1], clips[2]}, two, {ones.data(), nullptr}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);             // a masked base
        CHECK(stacked({clips[1], nullptr}, two, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);
        CHECK(stacked({clips[1], clips[2]}, {}, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_subtree_mask(clips[1], 0xFFFFFFF0u, 1.0f, 0.0f, subtree.data(), n) == SR_ERR_INVALID_ARG);
        CHECK(sr_clip_subtree_mask(clips[1], nodes[0].gltf_node, 1.0f, 0.0f, subtree.data(), n - 1) == SR_ERR_INVALID_ARG);
        SrClip* other = nullptr;
        CHECK(sr_gltf_bake_clip(bar, 0, &other) == 0);
        g_words.clear();
        CHECK(stacked({clips[1], other}, two, {}, nullptr, info[1]).rc == SR_ERR_INVALID_ARG && g_words.find("sr_clip_blend_compatible: the clips differ in the ") == 0);
        sr_clip_destroy(other);
    }
    for (SrClip* c : clips) sr_clip_destroy(c);
    sr_gltf_close(rig); sr_gltf_close(bar);
    printf("clip layers ok: %u poses\n", n_poses);
    return 0;
}
