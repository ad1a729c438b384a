// Sanitizer driver for baked clips (tests/test_clip_sanitizers.py): sr_gltf_bake_clip and the host rule. Built with
// g++ -fsanitize=address,undefined from the loader's host sources and clip_host.cpp; usage: clip_asan FIXTURE TMP ITERS BROKEN...
//   FIXTURE   tests/golden/clip_rig.glb: every animation and the static pose bake; every table is read through the read-outs and
//             the host rule is evaluated at times inside, on and outside the keys, and compared with sr_gltf_pose byte for byte
//   BROKEN... variants sr_gltf_bake_clip must refuse for at least one animation
//   ITERS     mutants of the fixture (byte flips, 32-bit overwrites, truncation; TMP is the scratch file) go through the same
//             calls: any status is fine, a crash or a sanitizer report is not
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/sunray_hip.h"
namespace srh { int set_error(int code, const std::string&) { return code; } }

// Bakes and evaluates everything of one open file; returns the number of refused bakes, or -1 where a baked clip disagrees with
// sr_gltf_pose.
static int exercise(SrGltf* g, bool compare) {
    int refused = 0;
    volatile double sink = 0.0;
    uint32_t ni = 0, n_skins = 0, n_anims = 0;
    sr_gltf_counts(g, nullptr, &ni, nullptr, nullptr, nullptr);
    sr_gltf_rig_counts(g, &n_skins, &n_anims);
    if (n_anims > 16) n_anims = 16;
    if (n_skins > 16) n_skins = 16;
    for (int32_t a = -1; a < (int32_t)n_anims + 1; a++) {               // one past the end: refused
        SrClip* clip = nullptr;
        if (sr_gltf_bake_clip(g, a, &clip) != 0) { refused += a < (int32_t)n_anims; continue; }
        SrClipInfo info;
        sr_clip_info(clip, &info);
        std::vector<SrClipNodeInfo> nodes(info.n_nodes + 1);
        std::vector<SrClipChannelInfo> chans(info.n_channels + 1);
        std::vector<uint32_t> inst(info.n_instances + 1);
        sr_clip_layout(clip, nodes.data(), chans.data(), inst.data());
        for (uint32_t n = 0; n < info.n_nodes; n++) sink = sink + nodes[n].parent + nodes[n].gltf_node + nodes[n].level;
        for (uint32_t c = 0; c < info.n_channels + 1; c++) {
            const float* times = nullptr; const float* values = nullptr;
            if (sr_clip_channel_keys(clip, c, &times, &values) != 0) continue;
            for (uint32_t k = 0; k < chans[c].n_keys; k++) { sink = sink + times[k]; for (uint32_t v = 0; v < (chans[c].path == 1 ? 4u : 3u); v++) sink = sink + values[k * (chans[c].path == 1 ? 4 : 3) + v]; }
        }
        std::vector<SrNodeTrs> trs(info.n_nodes + 1);
        std::vector<SrTransform> jm(info.n_joints + 1), xf(info.n_instances + 1), want_xf(ni + 1);
        const SrTransform placement = {{1, 0, 0, 2, 0, 1, 0, -1, 0, 0, 1, 0.5f}};
        const float times[] = {-1.0f, 0.0f, 0.37f * info.duration_seconds, info.duration_seconds, 2.0f * info.duration_seconds + 1.0f, NAN, INFINITY};
        for (float t : times) {
            if (sr_clip_sample_host(clip, t, trs.data()) != 0) continue;
            uint32_t bad = 0;
            sr_clip_compose_host(clip, trs.data(), nullptr, jm.data(), xf.data(), &bad);
            sr_clip_compose_host(clip, trs.data(), &placement, nullptr, xf.data(), nullptr);
            const int rc = sr_clip_pose_host(clip, t, nullptr, jm.data(), xf.data());
            for (uint32_t i = 0; i < info.n_instances; i++) for (int c = 0; c < 12; c++) sink = sink + xf[i].m[c];
            if (!compare) continue;
            if (sr_gltf_pose(g, a, t, want_xf.data(), 0, nullptr) != 0 || ni != info.n_instances || memcmp(want_xf.data(), xf.data(), 48 * (size_t)ni) != 0) return -1;
            for (uint32_t s = 0; s < n_skins; s++) {
                uint32_t first = 0, nj = 0;
                if (sr_clip_skin(clip, s, &first, &nj) != 0) continue;
                std::vector<SrTransform> want(nj + 1);
                const int wrc = sr_gltf_pose(g, a, t, nullptr, s, want.data());
                if (wrc == 0 && rc == 0 && memcmp(want.data(), jm.data() + first, 48 * (size_t)nj) != 0) return -1;
                if (wrc != 0 && rc == 0) return -1;
            }
        }
        sr_clip_destroy(clip);
    }
    (void)sink;
    return refused;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: clip_asan FIXTURE TMP ITERS BROKEN...\n"); return 2; }
    SrGltf* g = nullptr;
    if (sr_gltf_open(argv[1], &g) != 0) { fprintf(stderr, "the fixture does not open\n"); return 1; }
    const int e0 = exercise(g, true);
    sr_gltf_close(g);
    if (e0 != 0) { fprintf(stderr, "the fixture: %d (0 refused bakes and no difference expected)\n", e0); return 1; }
    for (int i = 4; i < argc; i++) {
        if (sr_gltf_open(argv[i], &g) != 0) { fprintf(stderr, "%s does not open\n", argv[i]); return 1; }
        const int e = exercise(g, false);
        sr_gltf_close(g);
        if (e <= 0) { fprintf(stderr, "%s: no bake was refused\n", argv[i]); return 1; }
    }
    std::vector<unsigned char> seed;
    FILE* f = fopen(argv[1], "rb"); fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET); seed.resize(n);
    if (fread(seed.data(), 1, n, f) != (size_t)n) return 1;
    fclose(f);
    unsigned iters = atoi(argv[3]), rng = 2463534242u, opened = 0;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; };
    for (unsigned it = 0; it < iters; it++) {
        std::vector<unsigned char> m = seed;
        const unsigned k = 1 + next() % 6;
        for (unsigned j = 0; j < k; j++) {
            const unsigned pos = next() % m.size();
            switch (next() % 4) {
                case 0: m[pos] = (unsigned char)next(); break;
                case 1: m[pos] ^= 1u << (next() % 8); break;
                case 2: if (pos + 4 <= m.size()) { unsigned v = next() % 3 == 0 ? 0xFFFFFFFFu : next(); memcpy(&m[pos], &v, 4); } break;
                case 3: if (m.size() > 64) m.resize(m.size() - next() % 32); break;
            }
        }
        FILE* o = fopen(argv[2], "wb"); fwrite(m.data(), 1, m.size(), o); fclose(o);
        if (sr_gltf_open(argv[2], &g) == 0) { opened++; exercise(g, false); sr_gltf_close(g); }
    }
    printf("clip ok: %d broken variants, %u mutants, %u opened\n", argc - 4, iters, opened);
    return 0;
}
