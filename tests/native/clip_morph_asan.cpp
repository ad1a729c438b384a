// Sanitizer driver for the morph sets of baked clips (tests/test_clip_morph_host.py): sr_gltf_bake_clip, the set read-outs and the
// host rule sr_clip_weights_host. Built with g++ -fsanitize=address,undefined from the loader's host sources and clip_host.cpp;
// usage: clip_morph_asan GOOD GOOD BROKEN...
//   GOOD      files whose sets sr_gltf_morph_weights answers for, except for a CUBICSPLINE channel: every animation and the static
//             pose bake; every set is read through the read-outs, and the host rule runs at, next to and outside every key, at
//             times that are not finite and with other target counts, and is compared with sr_gltf_morph_weights in status and
//             bytes
//   BROKEN... variants whose bake must succeed all the same and keep at least one set as unavailable
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
namespace srh { int set_error(int code, const std::string&) { return code; } }

// Bakes everything of one open file and walks every set; returns the number of unavailable sets, or -1 where a bake is refused
// or the host rule disagrees with sr_gltf_morph_weights.
static int exercise(SrGltf* g) {
    int unavailable = 0;
    volatile double sink = 0.0;
    uint32_t n_blases = 0, n_skins = 0, n_anims = 0;
    sr_gltf_counts(g, &n_blases, nullptr, nullptr, nullptr, nullptr);
    sr_gltf_rig_counts(g, &n_skins, &n_anims);
    for (int32_t a = -1; a < (int32_t)n_anims; a++) {
        SrClip* clip = nullptr;
        if (sr_gltf_bake_clip(g, a, &clip) != 0) return -1;
        uint32_t n_sets = 0, seen = 0;
        sr_clip_morph_count(clip, &n_sets);
        for (uint32_t b = 0; b < n_blases + 1; b++) {                   // one past the end: no set
            SrClipMorphInfo m;
            if (sr_clip_morph(clip, b, &m) != 0) continue;
            seen++;
            const float* times = nullptr; const float* values = nullptr; const float* defaults = nullptr;
            const int krc = sr_clip_morph_keys(clip, b, &times, &values, &defaults);
            std::vector<float> got(m.n_targets + 2, 7.0f), want(m.n_targets + 2, 7.0f);
            if (m.state == SR_CLIP_MORPH_UNAVAILABLE) {
                unavailable++;
                if (krc == 0 || m.status == 0) return -1;
                if (sr_clip_weights_host(clip, 0.5f, b, got.data(), m.n_targets) != sr_gltf_morph_weights(g, a, 0.5f, b, want.data(), m.n_targets) && m.n_targets) return -1;
                if (sr_clip_weights_host(clip, 0.5f, b, got.data(), m.n_targets) == 0) return -1;
                continue;
            }
            if (krc != 0) return -1;
            for (uint32_t t = 0; t < m.n_targets; t++) sink = sink + defaults[t];
            std::vector<float> at = {-1.0f, 0.0f, 1e30f, NAN, INFINITY, -INFINITY};
            for (uint32_t k = 0; k < m.n_keys; k++) {
                sink = sink + times[k];
                for (uint32_t t = 0; t < m.n_targets; t++) sink = sink + values[(size_t)k * m.n_targets + t];
                at.push_back(times[k]); at.push_back(nextafterf(times[k], -INFINITY)); at.push_back(nextafterf(times[k], INFINITY));
                if (k + 1 < m.n_keys) at.push_back(0.5f * (times[k] + times[k + 1]));
            }
            for (float time : at) {
                const int rc = sr_clip_weights_host(clip, time, b, got.data(), m.n_targets);
                const int wrc = sr_gltf_morph_weights(g, a, time, b, want.data(), m.n_targets);
                if (rc != wrc || (rc == 0 && memcmp(got.data(), want.data(), 4 * (size_t)m.n_targets) != 0)) return -1;
                if (got[m.n_targets] != 7.0f) return -1;                // nothing past the targets
            }
            for (uint32_t other : {0u, m.n_targets - 1, m.n_targets + 1})
                if (other != m.n_targets && sr_clip_weights_host(clip, 0.0f, b, got.data(), other) != sr_gltf_morph_weights(g, a, 0.0f, b, want.data(), other)) return -1;
        }
        if (seen != n_sets) return -1;
        sr_clip_destroy(clip);
    }
    (void)sink;
    return unavailable;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: clip_morph_asan GOOD GOOD BROKEN...\n"); return 2; }
    for (int i = 1; i < argc; i++) {
        SrGltf* g = nullptr;
        if (sr_gltf_open(argv[i], &g) != 0) { fprintf(stderr, "%s does not open\n", argv[i]); return 1; }
        const int e = exercise(g);
        sr_gltf_close(g);
        if (e < 0) { fprintf(stderr, "%s: a bake was refused, or the host rule differs from sr_gltf_morph_weights\n", argv[i]); return 1; }
        if (i == 1 && e != 1) { fprintf(stderr, "%s: %d unavailable sets, 1 expected (the CUBICSPLINE channel)\n", argv[i], e); return 1; }
        if (i == 2 && e != 0) { fprintf(stderr, "%s: %d unavailable sets, none expected\n", argv[i], e); return 1; }
        if (i > 2 && e == 0) { fprintf(stderr, "%s: no set is unavailable\n", argv[i]); return 1; }
    }
    printf("clip morph ok: 2 good files, %d broken variants\n", argc - 3);
    return 0;
}
