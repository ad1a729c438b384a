// Sanitizer driver for the glTF loader's rig read-outs and sr_gltf_pose (tests/test_pose_sanitizers.py). Built with
// g++ -fsanitize=address,undefined from the loader's host sources; usage: pose_asan FIXTURE TMP ITERS BROKEN...
//   FIXTURE   tests/golden/skinned_bar.glb: every new getter and sr_gltf_pose must succeed on it (the CUBICSPLINE animation
//             alone is refused), and every byte they hand out is read
//   BROKEN... variants of the fixture with one rig defect each (accessor counts too short for the vertex count, joint node
//             indices out of range, key times not increasing, empty samplers, ...): sr_gltf_open must succeed and at least one
//             of the new calls must return an error status
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

// Calls everything on one open file; returns the number of calls that reported an error. Every array handed out is summed.
static unsigned exercise(SrGltf* g) {
    unsigned errors = 0;
    volatile double sink = 0.0;
    uint32_t nb = 0, ni = 0, n_skins = 0, n_anims = 0;
    sr_gltf_counts(g, &nb, &ni, nullptr, nullptr, nullptr);
    if (sr_gltf_rig_counts(g, &n_skins, &n_anims) != 0) errors++;
    if (n_skins > 64) n_skins = 64;
    if (n_anims > 64) n_anims = 64;
    for (uint32_t b = 0; b < nb + 1; b++) {                       // one past the end: refused
        int32_t skin = -1; const SrSkinInfluence* inf = nullptr; uint32_t nv = 0;
        if (sr_gltf_blas_skin(g, b, &skin, &inf, &nv) != 0) { errors += b < nb; continue; }
        if (inf) for (uint32_t v = 0; v < nv; v++) for (int k = 0; k < 4; k++) sink = sink + inf[v].joint[k] + inf[v].weight[k];
    }
    std::vector<uint32_t> joints_of(n_skins + 1, 0);
    for (uint32_t s = 0; s < n_skins + 1; s++) {
        uint32_t nj = 0; const SrTransform* ibm = nullptr; const uint32_t* nodes = nullptr;
        if (sr_gltf_skin(g, s, &nj, &ibm, &nodes) != 0) { errors += s < n_skins; continue; }
        joints_of[s] = nj;
        for (uint32_t j = 0; j < nj; j++) { sink = sink + nodes[j]; for (int c = 0; c < 12; c++) sink = sink + ibm[j].m[c]; }
    }
    std::vector<SrTransform> inst(ni + 1);
    for (int32_t a = -1; a < (int32_t)n_anims + 1; a++) {
        float duration = 1.0f;
        if (a >= 0) {
            const char* name = nullptr; uint32_t nc = 0, nw = 0;
            if (sr_gltf_animation(g, (uint32_t)a, &name, &duration, &nc) != 0) { errors += a < (int32_t)n_anims; duration = 1.0f; }
            else sink = sink + strlen(name) + nc;
            if (sr_gltf_animation_ignored_channels(g, (uint32_t)a, &nw) != 0) errors += a < (int32_t)n_anims;
        }
        const float times[] = {-1.0f, 0.0f, 0.37f * duration, duration, 2.0f * duration + 1.0f, NAN, INFINITY};
        for (float t : times) {
            if (sr_gltf_pose(g, a, t, inst.data(), 0, nullptr) != 0) errors += a < (int32_t)n_anims && std::isfinite(t);
            else for (uint32_t i = 0; i < ni; i++) for (int c = 0; c < 12; c++) sink = sink + inst[i].m[c];
            for (uint32_t s = 0; s < n_skins + 1; s++) {
                std::vector<SrTransform> jm(joints_of[s] + 1);
                if (sr_gltf_pose(g, a, t, nullptr, s, jm.data()) != 0) errors += a < (int32_t)n_anims && s < n_skins && std::isfinite(t);
                else for (uint32_t j = 0; j < joints_of[s]; j++) for (int c = 0; c < 12; c++) sink = sink + jm[j].m[c];
            }
            for (uint32_t node = 0; node < 12; node++) {
                float tr[3], q[4], sc[3]; uint32_t mask = 0;
                if (sr_gltf_sample_node(g, a, t, node, tr, q, sc, &mask) == 0) sink = sink + tr[0] + q[3] + sc[2] + mask;
            }
        }
    }
    (void)sink;
    return errors;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: pose_asan FIXTURE TMP ITERS BROKEN...\n"); return 2; }
    SrGltf* g = nullptr;
    if (sr_gltf_open(argv[1], &g) != 0) { fprintf(stderr, "the fixture does not open\n"); return 1; }
    // the fixture: animation 1 is CUBICSPLINE, so its poses are refused: 5 finite times x (instances + 1 skin) = 10 errors, no other
    const unsigned e0 = exercise(g);
    sr_gltf_close(g);
    if (e0 != 10) { fprintf(stderr, "the fixture reported %u errors, 10 (the CUBICSPLINE poses) expected\n", e0); return 1; }
    for (int i = 4; i < argc; i++) {
        if (sr_gltf_open(argv[i], &g) != 0) { fprintf(stderr, "%s: sr_gltf_open must not report a rig defect\n", argv[i]); return 1; }
        const unsigned e = exercise(g);
        sr_gltf_close(g);
        if (e <= 10) { fprintf(stderr, "%s: no call reported its defect (%u errors)\n", argv[i], e); return 1; }
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
        if (sr_gltf_open(argv[2], &g) == 0) { opened++; exercise(g); sr_gltf_close(g); }
    }
    printf("pose ok: %d broken variants, %u mutants, %u opened\n", argc - 4, iters, opened);
    return 0;
}
