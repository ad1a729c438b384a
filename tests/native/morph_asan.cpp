// Sanitizer driver for the glTF loader's morph read-outs (tests/test_morph_sanitizers.py). Built with
// g++ -fsanitize=address,undefined from the loader's host sources; usage: morph_asan FIXTURE TMP ITERS BROKEN...
//   FIXTURE   tests/golden/morph_bar.glb: sr_gltf_blas_morph and sr_gltf_morph_weights must succeed on it (the CUBICSPLINE
//             weights channel of animation 1 alone is refused), and every byte they hand out is read
//   BROKEN... variants of the fixture with one morph defect each (a target accessor too short for the vertex count, an integer
//             component type, a TEXCOORD_0 target, a short output accessor, ...): sr_gltf_open must succeed and at least one of the
//             new calls must return an error status
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
    uint32_t nb = 0, n_anims = 0;
    sr_gltf_counts(g, &nb, nullptr, nullptr, nullptr, nullptr);
    if (sr_gltf_rig_counts(g, nullptr, &n_anims) != 0) errors++;
    if (n_anims > 64) n_anims = 64;
    for (uint32_t b = 0; b < nb + 1; b++) {                       // one past the end: refused
        uint32_t nt = 0, nv = 0; const SrMorphDelta* d = nullptr; const float* dw = nullptr;
        if (sr_gltf_blas_morph(g, b, &nt, &d, &nv, &dw) != 0) { errors += b < nb; nt = 0; }
        for (size_t i = 0; i < (size_t)nt * nv; i++) for (int c = 0; c < 3; c++) sink = sink + d[i].position[c] + d[i].normal[c] + d[i].tangent[c] + d[i]._pad0;
        for (uint32_t k = 0; k < nt; k++) sink = sink + dw[k];
        std::vector<float> w(nt + 1);
        for (int32_t a = -1; a < (int32_t)n_anims + 1; a++) {
            float duration = 1.0f;
            if (a >= 0 && a < (int32_t)n_anims && sr_gltf_animation(g, (uint32_t)a, nullptr, &duration, nullptr) != 0) duration = 1.0f;
            const float times[] = {-1.0f, 0.0f, 0.37f * duration, duration, 2.0f * duration + 1.0f, NAN, INFINITY};
            for (float t : times) {
                if (sr_gltf_morph_weights(g, a, t, b, w.data(), nt) != 0) errors += b < nb && a < (int32_t)n_anims && std::isfinite(t);
                else for (uint32_t k = 0; k < nt; k++) sink = sink + w[k];
                if (sr_gltf_morph_weights(g, a, t, b, w.data(), nt + 1) == 0) errors += 1000;     // another count than the blas's is always refused
            }
        }
    }
    (void)sink;
    return errors;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: morph_asan FIXTURE TMP ITERS BROKEN...\n"); return 2; }
    SrGltf* g = nullptr;
    if (sr_gltf_open(argv[1], &g) != 0) { fprintf(stderr, "the fixture does not open\n"); return 1; }
    // the fixture: animation 1 has a CUBICSPLINE weights channel on blas 0's node: its 5 finite times are refused, nothing else
    const unsigned e0 = exercise(g);
    sr_gltf_close(g);
    if (e0 != 5) { fprintf(stderr, "the fixture reported %u errors, 5 (the CUBICSPLINE weights) expected\n", e0); return 1; }
    for (int i = 4; i < argc; i++) {
        if (sr_gltf_open(argv[i], &g) != 0) { fprintf(stderr, "%s: sr_gltf_open must not report a morph defect\n", argv[i]); return 1; }
        const unsigned e = exercise(g);
        sr_gltf_close(g);
        if (e <= 5 || e >= 1000) { fprintf(stderr, "%s: no call reported its defect, or a wrong count was accepted (%u errors)\n", argv[i], e); return 1; }
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
    printf("morph ok: %d broken variants, %u mutants, %u opened\n", argc - 4, iters, opened);
    return 0;
}
