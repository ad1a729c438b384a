// Sanitizer driver for layered morph weights (tests/test_clip_layer_weights_sanitizers.py): sr_clip_layer_weights_host and
// sr_clip_weights_layers_host. Built with g++ -fsanitize=address,undefined from the loader's host sources and clip_host.cpp; usage:
// clip_layer_weights_asan MORPH_BAR CLIP_RIG
//   MORPH_BAR  bakes of animation 0 (LINEAR on blas 0, STEP on blas 1), animation 1 in cubic mode (cubic on blas 0, defaults on
//              blas 1) and the static pose: one layer gives sr_clip_weights_host's bytes, two unmasked override layers
//              sr_clip_blend_weights_host's; an additive layer at its reference time, weight 0 and a mask of 0 on the mesh node give
//              the stack below; stacks of 1..8 layers in every mode / mask / clip mix run over exactly sized buffers; the refusals,
//              the bake of animation 1 without cubic mode (an unavailable set) among them
//   CLIP_RIG   its bake is refused as a layer over MORPH_BAR's
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
static std::string g_words;
namespace srh { int set_error(int code, const std::string& msg) { g_words = msg; return code; } }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s (%s)\n", __LINE__, #cond, g_words.c_str()); return 1; } } while (0)

struct Weights { int rc; std::vector<float> w; };
static bool same(const Weights& a, const Weights& b) { return a.rc == 0 && b.rc == 0 && a.w.size() == b.w.size() && memcmp(a.w.data(), b.w.data(), 4 * a.w.size()) == 0; }
static SrClipLayer layer(float t, float w, uint32_t mode, float ref_t) { return SrClipLayer{0, t, w, mode, SR_LAYER_NO_MASK, ref_t, {0, 0}}; }
static Weights stacked(const std::vector<const SrClip*>& clips, const std::vector<SrClipLayer>& layers, const std::vector<const float*>& masks, uint32_t blas, uint32_t n_targets) {
    Weights r{0, std::vector<float>(n_targets)};               // exactly sized: a write past the end is caught
    r.rc = sr_clip_weights_layers_host(clips.data(), layers.data(), masks.empty() ? nullptr : masks.data(), (uint32_t)layers.size(), blas, r.w.data(), n_targets);
    return r;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: clip_layer_weights_asan MORPH_BAR CLIP_RIG\n"); return 2; }
    SrGltf* bar = nullptr; SrGltf* rig = nullptr;
    CHECK(sr_gltf_open(argv[1], &bar) == 0 && sr_gltf_open(argv[2], &rig) == 0);
    SrClip* plain = nullptr;
    CHECK(sr_gltf_bake_clip(bar, 1, &plain) == 0);              // blas 0's set is kept unavailable
    CHECK(sr_gltf_set_cubicspline(bar, SR_CUBICSPLINE_SAMPLE) == 0);
    SrClip* clips[3];                                           // the static pose, animation 0, animation 1 (cubic)
    for (int a = 0; a < 3; a++) CHECK(sr_gltf_bake_clip(bar, a - 1, &clips[a]) == 0);
    SrClipInfo info;
    CHECK(sr_clip_info(clips[1], &info) == 0);
    const uint32_t n_nodes = info.n_nodes;
    std::vector<SrClipNodeInfo> nodes(n_nodes);
    CHECK(sr_clip_layout(clips[1], nodes.data(), nullptr, nullptr) == 0);
    const float weights[] = {0.0f, 1.0f, 0.25f, 0.5f, std::nextafter(1.0f, 0.0f), std::nextafter(0.0f, 1.0f)};
    const float times[] = {-1.0f, 0.0f, 0.3f, 0.5f, 0.9f, 1.0f, 1.6f, 7.0f};
    unsigned n_stacks = 0;
    for (uint32_t blas = 0; blas < 2; blas++) {
        SrClipMorphInfo mi;
        CHECK(sr_clip_morph(clips[1], blas, &mi) == 0);
        const uint32_t nt = mi.n_targets;
        uint32_t mesh_node = 0xFFFFFFFFu;
        for (uint32_t n = 0; n < n_nodes; n++) if (nodes[n].gltf_node == mi.gltf_node && mesh_node == 0xFFFFFFFFu) mesh_node = n;
        CHECK(mesh_node != 0xFFFFFFFFu);
        std::vector<float> zero_here(n_nodes, 1.0f), half_here(n_nodes, 0.0f), one_here(n_nodes, 0.0f);
        zero_here[mesh_node] = 0.0f; half_here[mesh_node] = 0.5f; one_here[mesh_node] = 1.0f;
        const float* mask_of[4] = {nullptr, zero_here.data(), half_here.data(), one_here.data()};
        // one layer; two override layers; what gives the stack below
        for (int a = 0; a < 3; a++) for (float t : times) {
            Weights want{0, std::vector<float>(nt)};
            want.rc = sr_clip_weights_host(clips[a], t, blas, want.w.data(), nt);
            const SrClipLayer base = layer(t, 1.0f, SR_LAYER_OVERRIDE, 0.0f);
            CHECK(same(stacked({clips[a]}, {base}, {}, blas, nt), want));
            for (int b = 0; b < 3; b++) for (float w : weights) {
                Weights blend{0, std::vector<float>(nt)};
                blend.rc = sr_clip_blend_weights_host(clips[a], t, clips[b], 0.7f, w, blas, blend.w.data(), nt);
                const std::vector<SrClipLayer> two = {base, layer(0.7f, w, SR_LAYER_OVERRIDE, 0.0f)};
                CHECK(same(stacked({clips[a], clips[b]}, two, {}, blas, nt), blend));
                CHECK(same(stacked({clips[a], clips[b]}, two, {nullptr, one_here.data()}, blas, nt), blend));                 // 1 on the mesh node is no mask
                std::vector<SrClipLayer> three = two;
                three.push_back(layer(0.4f, 0.5f, SR_LAYER_OVERRIDE, 0.0f));
                CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {nullptr, nullptr, zero_here.data()}, blas, nt), blend));
                three[2] = layer(0.4f, 0.5f, SR_LAYER_ADDITIVE, 1.3f);
                CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {nullptr, nullptr, zero_here.data()}, blas, nt), blend));
                three[2] = layer(0.4f, 0.0f, SR_LAYER_ADDITIVE, 1.3f);
                CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {}, blas, nt), blend));
                three[2] = layer(0.4f, w, SR_LAYER_ADDITIVE, 0.4f);
                CHECK(same(stacked({clips[a], clips[b], clips[2]}, three, {}, blas, nt), blend));
                n_stacks += 6;
            }
        }
        // stacks of 1..8 layers: every mode, mask and clip in turn
        for (uint32_t salt = 0; salt < 24; salt++) for (uint32_t n_layers = 1; n_layers <= SR_CLIP_MAX_LAYERS; n_layers++) {
            std::vector<const SrClip*> cs; std::vector<SrClipLayer> ls; std::vector<const float*> ms;
            for (uint32_t l = 0; l < n_layers; l++) {
                cs.push_back(clips[(l + salt) % 3]);
                ls.push_back(l == 0 ? layer(times[salt % 8], 1.0f, SR_LAYER_OVERRIDE, 0.0f)
                                    : layer(times[(l + salt) % 8], weights[(l + salt) % 6], (l + salt / 3) % 2 ? SR_LAYER_ADDITIVE : SR_LAYER_OVERRIDE, times[(3 * l + salt) % 8]));
                ms.push_back(l == 0 ? nullptr : mask_of[(l + salt / 2) % 4]);
            }
            CHECK(stacked(cs, ls, ms, blas, nt).rc == 0);
            n_stacks++;
        }
        // the rule over exactly sized vectors
        {
            std::vector<float> a(nt), b(nt), c(nt), r(nt), out(nt);
            CHECK(sr_clip_weights_host(clips[1], 0.9f, blas, a.data(), nt) == 0 && sr_clip_weights_host(clips[2], 0.25f, blas, b.data(), nt) == 0);
            CHECK(sr_clip_weights_host(clips[2], 0.6f, blas, c.data(), nt) == 0 && sr_clip_weights_host(clips[2], 1.4f, blas, r.data(), nt) == 0);
            const float* cur[3] = {a.data(), b.data(), c.data()};
            const float* ref[3] = {nullptr, nullptr, r.data()};
            float weight[3] = {1.0f, 0.5f, 0.75f}, mask_value[3] = {1.0f, 0.5f, 1.0f};
            uint32_t mode[3] = {SR_LAYER_OVERRIDE, SR_LAYER_OVERRIDE, SR_LAYER_ADDITIVE};
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, mask_value, 3, nt, out.data()) == 0);
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 3, nt, out.data()) == 0);
            CHECK(sr_clip_layer_weights_host(cur, nullptr, weight, mode, nullptr, 2, nt, out.data()) == 0);
            CHECK(sr_clip_layer_weights_host(cur, nullptr, weight, mode, nullptr, 3, nt, out.data()) == SR_ERR_INVALID_ARG);     // an additive layer without its reference weights
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 0, nt, out.data()) == SR_ERR_INVALID_ARG);
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 9, nt, out.data()) == SR_ERR_INVALID_ARG);
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 3, 0, nullptr) == 0);
            CHECK(sr_clip_layer_weights_host(nullptr, ref, weight, mode, nullptr, 3, nt, out.data()) == SR_ERR_INVALID_ARG);
            for (float w : {-0.1f, 1.5f, NAN, INFINITY}) { weight[1] = w; CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 3, nt, out.data()) == SR_ERR_INVALID_ARG); }
            weight[1] = 0.5f;
            for (float v : {-0.5f, 1.0001f, NAN}) { mask_value[2] = v; CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, mask_value, 3, nt, out.data()) == SR_ERR_INVALID_ARG); }
            mask_value[2] = 1.0f; mode[1] = 2;
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, nullptr, 3, nt, out.data()) == SR_ERR_INVALID_ARG);
            mode[1] = SR_LAYER_OVERRIDE; mask_value[0] = 0.5f;
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, mask_value, 3, nt, out.data()) == SR_ERR_INVALID_ARG);    // a masked base
            mask_value[0] = 1.0f; weight[0] = 0.5f;
            CHECK(sr_clip_layer_weights_host(cur, ref, weight, mode, mask_value, 3, nt, out.data()) == SR_ERR_INVALID_ARG);
        }
        // the refusals of sample, resolve, stack
        {
            const std::vector<SrClipLayer> two = {layer(0.3f, 1.0f, SR_LAYER_OVERRIDE, 0.0f), layer(0.7f, 0.5f, SR_LAYER_OVERRIDE, 0.0f)};
            std::vector<SrClipLayer> l = two;
            l[1].time_seconds = INFINITY;
            CHECK(stacked({clips[1], clips[2]}, l, {}, blas, nt).rc == SR_ERR_INVALID_ARG);
            l = two; l[1].mode = SR_LAYER_ADDITIVE; l[1].ref_time_seconds = NAN;
            CHECK(stacked({clips[1], clips[2]}, l, {}, blas, nt).rc == SR_ERR_INVALID_ARG);
            l = two; l[0].mode = SR_LAYER_ADDITIVE;
            CHECK(stacked({clips[1], clips[2]}, l, {}, blas, nt).rc == SR_ERR_INVALID_ARG);
            CHECK(stacked({clips[1], clips[2]}, two, {one_here.data(), nullptr}, blas, nt).rc == SR_ERR_INVALID_ARG);          // a masked base
            CHECK(stacked({clips[1], nullptr}, two, {}, blas, nt).rc == SR_ERR_INVALID_ARG);
            CHECK(stacked({clips[1], clips[2]}, {}, {}, blas, nt).rc == SR_ERR_INVALID_ARG);
            CHECK(stacked({clips[1], clips[2]}, two, {}, blas, nt + 1).rc == SR_ERR_INVALID_ARG);                                 // a wrong n_targets
            CHECK(stacked({clips[1], clips[2]}, two, {}, 7, nt).rc == SR_ERR_INVALID_ARG);                                      // no set for the blas
            std::vector<float> bad(n_nodes, 0.5f);
            bad[n_nodes - 1] = 1.5f;
            CHECK(stacked({clips[1], clips[2]}, two, {nullptr, bad.data()}, blas, nt).rc == SR_ERR_INVALID_ARG);
            l = two; l[1].weight = 0.0f;                           // a layer at weight 0 is checked like any other
            g_words.clear();
            const int rc = stacked({clips[1], plain}, l, {}, blas, nt).rc;
            if (blas == 0) CHECK(rc == SR_ERR_UNSUPPORTED && g_words.find("sr_clip_weights_layers_host: layer 1: ") == 0);
            else CHECK(rc == 0);                                    // blas 1's set of that bake is its defaults
            SrClip* other = nullptr;
            CHECK(sr_gltf_bake_clip(rig, 0, &other) == 0);
            g_words.clear();
            CHECK(stacked({clips[1], other}, two, {}, blas, nt).rc == SR_ERR_INVALID_ARG && g_words.find("sr_clip_blend_compatible: the clips differ in the ") == 0);
            sr_clip_destroy(other);
        }
    }
    for (SrClip* c : clips) sr_clip_destroy(c);
    sr_clip_destroy(plain);
    sr_gltf_close(bar); sr_gltf_close(rig);
    printf("clip layer weights ok: %u stacks\n", n_stacks);
    return 0;
}
