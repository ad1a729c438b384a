// ORACLE — TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Parity status: UNPINNED (see orc_math.h).
// extern "C" surface of the oracle for the ctypes binding in oracle/binding.py. Only tests/,
// __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
#include <cstring>

#include <omp.h>

#include "orc_scene.h"

using namespace orc;
namespace orc {
void post_temporal(const SrPostParams&); void post_denoise(const SrPostParams&); void post_tonemap(const SrPostParams&);
void post_denoise_step(const SrPostParams&, const uint32_t*, uint32_t*, int);
}

extern "C" {

void orc_set_threads(int n) { if (n > 0) omp_set_num_threads(n); }
int orc_get_max_threads() { return omp_get_max_threads(); }
void* orc_scene_create() { return new Scene(); }
void orc_scene_destroy(void* s) { delete (Scene*)s; }
int orc_scene_add_mesh(void* s, uint64_t key, const SrVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, const SrMaterial* m) {
    return ((Scene*)s)->add_mesh(key, v, nv, idx, ni, m);
}
int orc_scene_add_blas(void* s, uint64_t key, const SrVertex* v, uint32_t nv, const uint32_t* idx, uint32_t ni, const SrMaterial* m,
                       const SrEmissiveTriangle* et, uint32_t n_et) {
    return ((Scene*)s)->add_blas(key, v, nv, idx, ni, m, et, n_et);
}
void orc_scene_remove(void* s, uint64_t key) { ((Scene*)s)->remove(key); }
int orc_scene_add_image(void* s, const uint8_t* data, uint32_t w, uint32_t h, uint32_t channels) {
    return ((Scene*)s)->add_image(data, w, h, channels);
}
int orc_scene_add_sampler(void* s, const SrSamplerDesc* d) { return ((Scene*)s)->add_sampler(d); }
// KAT hook: one texture fetch
void orc_sample_texture(void* s, uint32_t image, uint32_t sampler, float u, float v, const float* fallback4, float* out4) {
    V4 r = ((Scene*)s)->sample_texture(image, sampler, u, v, V4{fallback4[0], fallback4[1], fallback4[2], fallback4[3]});
    out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}
int orc_scene_set_instances(void* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* xf) {
    return ((Scene*)s)->set_instances(keys, counts, n_keys, xf);
}
void orc_scene_set_brute_force(void* s, int on) { ((Scene*)s)->use_brute_force = on != 0; }
// Test aid: 4 * width * height ints that the following orc_trace_ris calls fill (orc_scene.h, read_log); NULL switches it off.
void orc_scene_set_read_log(void* s, int32_t* log) { ((Scene*)s)->read_log = log; }
// Test aid: 2 * width * height words that the following orc_trace_ris / orc_trace_final calls fill (orc_scene.h, branch_log); NULL switches it off.
void orc_scene_set_branch_log(void* s, uint32_t* log) { ((Scene*)s)->branch_log = log; }
void orc_scene_get_tables(void* sp, const SrTransform** transforms, uint32_t* n_instances,
                          const SrEmissiveIndirectionEntry** indirection, uint32_t* num_lights,
                          const SrEmissiveTriangle** emissive, uint32_t* n_emissive, uint32_t* n_triangles) {
    Scene* s = (Scene*)sp;
    *transforms = s->transforms.data(); *n_instances = (uint32_t)s->transforms.size();
    *indirection = s->indirection.data(); *num_lights = (uint32_t)s->indirection.size();
    *emissive = s->emissive_tris.data(); *n_emissive = (uint32_t)s->emissive_tris.size();
    *n_triangles = (uint32_t)s->tris.size();
}
void orc_scene_bvh_info(void* sp, uint64_t* n_nodes, uint64_t* n_tris) {
    Scene* s = (Scene*)sp; *n_nodes = s->nodes.size(); *n_tris = s->tris.size();
}

void orc_trace_closest(void* sp, const SrRay* rays, uint32_t n, SrHit* hits) {
    Scene* s = (Scene*)sp;
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const SrRay& r = rays[i];
        Hit h = s->closest(v3(r.origin[0], r.origin[1], r.origin[2]), v3(r.dir[0], r.dir[1], r.dir[2]), r.tmin, r.tmax, nullptr);
        hits[i] = SrHit{h.t, h.u, h.v, h.tri};
    }
}
void orc_trace_any(void* sp, const SrRay* rays, uint32_t n, uint32_t* occluded) {
    Scene* s = (Scene*)sp;
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const SrRay& r = rays[i];
        occluded[i] = s->any(v3(r.origin[0], r.origin[1], r.origin[2]), v3(r.dir[0], r.dir[1], r.dir[2]), r.tmin, r.tmax, nullptr) ? 1u : 0u;
    }
}
void orc_shade_closest_hit(void* sp, const SrHit* hits, uint32_t n, SrRayPayload* out) {
    Scene* s = (Scene*)sp;
    for (uint32_t i = 0; i < n; i++) out[i] = s->shade_hit(Hit{hits[i].t, hits[i].u, hits[i].v, hits[i].t < 0.0f ? 0xFFFFFFFFu : hits[i].tri});
}
void orc_trace_ris(void* sp, const SrRtParams* p) { trace_ris(*(Scene*)sp, *p); }
void orc_trace_final(void* sp, const SrRtParams* p) { trace_final(*(Scene*)sp, *p); }
void orc_post_temporal(const SrPostParams* p) { post_temporal(*p); }
void orc_post_denoise(const SrPostParams* p) { post_denoise(*p); }
void orc_post_denoise_step(const SrPostParams* p, const uint32_t* src, uint32_t* dst, int step_width) { post_denoise_step(*p, src, dst, step_width); }
void orc_post_tonemap(const SrPostParams* p) { post_tonemap(*p); }
float orc_log(float x) { return log_f(x); }
float orc_pow(float x, float y) { return pow_f(x, y); }
void orc_reset_counters(void* sp) { ((Scene*)sp)->counters = Counters{}; }
void orc_read_counters(void* sp, SrRayCounters* out) {
    const Counters& c = ((Scene*)sp)->counters;
    out->closest_queries = c.closest; out->any_queries = c.any; out->boxes_tested = c.boxes; out->tris_tested = c.tris;
    out->reused_visibility_queries = 0;
    out->reused_primary_hits = 0;   // the oracle issues every TraceRay of the reference: SrRtParams.primary_payload is ignored here
}

// ---- host-side helpers ------------------------------------------------------------------------
void orc_camera_matrices(const float* pos, const float* target, float fov, uint32_t w, uint32_t h, const float* prev, SrMatrices* out) {
    camera_matrices(pos, target, fov, w, h, prev, out);
}
void orc_material_new(const float* bc, float metallic, float roughness, const float* ef, float es, float tr, float ior, SrMaterial* out) {
    material_new(bc, metallic, roughness, ef, es, tr, ior, out);
}
void orc_inverse3x3(const SrTransform* t, float* out9) { inverse3x3(*t, out9); }

// ---- known-answer-test hooks (rt_utils.slang) -----------------------------------------------
uint32_t orc_pcg_hash(uint32_t x) { return pcg_hash(x); }
uint32_t orc_init_rng(uint32_t px, uint32_t py, uint32_t frame, uint32_t w) { return init_rng(px, py, frame, w).seed; }
// n draws from `seed`: raw 32-bit results (before the float conversion) and the floats.
uint32_t orc_rnd_stream(uint32_t seed, uint32_t n, uint32_t* words, float* vals) {
    Rng r{seed};
    for (uint32_t i = 0; i < n; i++) {
        Rng t = r;
        t.seed = t.seed * 747796405u + 2891336453u;
        uint32_t word = ((t.seed >> ((t.seed >> 28u) + 4u)) ^ t.seed) * 277803737u;
        words[i] = (word >> 22u) ^ word;
        vals[i] = rnd(r);
    }
    return r.seed;
}
uint32_t orc_pack_normal(float x, float y, float z) { return pack_normal(v3(x, y, z)); }
void orc_unpack_normal(uint32_t p, float* out) { V3 n = unpack_normal(p); out[0] = n.x; out[1] = n.y; out[2] = n.z; }
uint32_t orc_pack_unorm_4x8(float x, float y, float z, float w) { return pack_unorm_4x8(x, y, z, w); }
void orc_unpack_unorm_4x8(uint32_t p, float* o) { V4 v = unpack_unorm_4x8(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
uint32_t orc_pack_half_2x16(float x, float y) { return pack_half_2x16(x, y); }
void orc_unpack_half_2x16(uint32_t p, float* o) { V2 v = unpack_half_2x16(p); o[0] = v.x; o[1] = v.y; }
uint32_t orc_pack_snorm_2x16(float x, float y) { return pack_snorm_2x16(x, y); }
uint32_t orc_f32_to_f16(float f) { return f32_to_f16(f); }
float orc_f16_to_f32(uint32_t h) { return f16_to_f32(h); }
uint32_t orc_pack_rgba8_snorm(float x, float y, float z, float w) { return pack_rgba8_snorm(x, y, z, w); }
uint32_t orc_pack_b10g11r11(float r, float g, float b) { return pack_b10g11r11(r, g, b); }
void orc_unpack_b10g11r11(uint32_t v, float* o) { o[0] = from_ufloat(v & 0x7ffu, 6); o[1] = from_ufloat((v >> 11) & 0x7ffu, 6); o[2] = from_ufloat(v >> 22, 5); }
void orc_sincos(float x, float* s, float* c) { sincos_f(x, s, c); }
float orc_exp(float x) { return exp_f(x); }
void orc_build_onb(const float* n, float* t, float* b) { V3 T, B; build_onb(v3(n[0], n[1], n[2]), T, B); t[0] = T.x; t[1] = T.y; t[2] = T.z; b[0] = B.x; b[1] = B.y; b[2] = B.z; }
void orc_get_random_bounce(const float* n, float r1, float r2, float* o) { V3 d = get_random_bounce(v3(n[0], n[1], n[2]), r1, r2); o[0] = d.x; o[1] = d.y; o[2] = d.z; }
void orc_sample_ggx_vndf(const float* n, const float* v, float rough, float r1, float r2, float* o) {
    V3 h = sample_ggx_vndf(v3(n[0], n[1], n[2]), v3(v[0], v[1], v[2]), rough, r1, r2); o[0] = h.x; o[1] = h.y; o[2] = h.z;
}
void orc_eval_unshadowed_light(const float* hp, const float* hn, const float* vv, const float* alb, float rough, float metal,
                               const float* emission, const float* lp, const float* ln, float* o) {
    V3 f = eval_unshadowed_light(v3(hp[0], hp[1], hp[2]), v3(hn[0], hn[1], hn[2]), v3(vv[0], vv[1], vv[2]), v3(alb[0], alb[1], alb[2]),
                                 rough, metal, v3(emission[0], emission[1], emission[2]), v3(lp[0], lp[1], lp[2]), v3(ln[0], ln[1], ln[2]));
    o[0] = f.x; o[1] = f.y; o[2] = f.z;
}
float orc_gi_target_pdf(const float* sp, const float* sn, const float* alb, float metallic, const float* xp, const float* rad) {
    return gi_target_pdf(v3(sp[0], sp[1], sp[2]), v3(sn[0], sn[1], sn[2]), v3(alb[0], alb[1], alb[2]), metallic, v3(xp[0], xp[1], xp[2]), v3(rad[0], rad[1], rad[2]));
}
void orc_merge_reservoirs(SrReservoir* r, const SrReservoir* new_r, float p_hat_new, float random_val) { merge_reservoirs(*r, *new_r, p_hat_new, random_val); }
void orc_merge_reservoirs_gi(SrReservoirGI* r, const SrReservoirGI* new_r, float p_hat_new, float jacobian, float random_val) {
    merge_reservoirs_gi(*r, *new_r, p_hat_new, jacobian, random_val);
}
float orc_smith_v_ggx(float a, float b, float c) { return smith_v_ggx(a, b, c); }
float orc_smith_g1_ggx(float a, float b) { return smith_g1_ggx(a, b); }
float orc_smoothstep(float a, float b, float x) { return smoothstep(a, b, x); }
void orc_refract(const float* i, const float* n, float eta, float* o) { V3 r = refract(v3(i[0], i[1], i[2]), v3(n[0], n[1], n[2]), eta); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
void orc_reflect(const float* i, const float* n, float* o) { V3 r = reflect(v3(i[0], i[1], i[2]), v3(n[0], n[1], n[2])); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
// any_hit.slang:11-43 alpha test as a pure helper (never invoked by traversal: geometry is OPAQUE,
// blas.rs:276). Returns 1 if the hit would be ignored.
int orc_any_hit_ignores(uint32_t alpha_mode, float alpha_cutoff, float base_alpha) {
    if (alpha_mode == 0) return 0;
    return base_alpha < alpha_cutoff ? 1 : 0;
}
// The whole shader on hit records (the CPU side of sr_any_hit_ignores): MeshInfo -> indices -> vertices -> uv ->
// sample_texture -> alpha test, any_hit.slang:14-42.
void orc_any_hit(void* sp, const SrHit* hits, uint32_t n, uint32_t* ignored) {
    Scene* s = (Scene*)sp;
    for (uint32_t i = 0; i < n; i++) ignored[i] = s->any_hit_ignores(Hit{hits[i].t, hits[i].u, hits[i].v, hits[i].t < 0.0f ? 0xFFFFFFFFu : hits[i].tri}) ? 1u : 0u;
}
// the canonical triangle test, for direct unit tests
int orc_intersect_tri(const float* o, const float* d, const float* v0, const float* v1, const float* v2, float tmin, float tmax, float* tuv) {
    V3 a = v3(v0[0], v0[1], v0[2]), b = v3(v1[0], v1[1], v1[2]), c = v3(v2[0], v2[1], v2[2]);
    WTri t{a, b - a, c - a, 0, 0};
    return intersect_tri(v3(o[0], o[1], o[2]), v3(d[0], d[1], d[2]), t, tmin, tmax, tuv[0], tuv[1], tuv[2]) ? 1 : 0;
}


// ---- helper probe: the CPU side of sr_probe_helper (include/sunray_hip.h) ------------------------------------------------
// Same ids, same rows of dwords; each case calls the oracle's own function of orc_math.h / orc_utils.h / orc_scene.h.
static const uint32_t kProbeWidth[SR_PROBE_COUNT][2] = {
    {1, 2}, {1, 1}, {1, 1}, {2, 1}, {1, 1}, {3, 1},                     // sincos exp log pow pow5 smoothstep
    {1, 1}, {1, 1}, {2, 1}, {1, 2}, {2, 1}, {1, 2}, {4, 1}, {1, 3},     // f32->f16 f16->f32 half2x16 snorm2x16 unorm4x8
    {3, 1}, {1, 3}, {4, 1}, {1, 1}, {3, 1}, {1, 3},                     // normal rgba8_snorm unsnorm8 b10g11r11
    {1, 1}, {4, 1}, {1, 2},                                             // pcg_hash init_rng rnd
    {3, 3}, {6, 3}, {7, 3}, {3, 6}, {3, 1}, {2, 1}, {5, 3}, {9, 3},     // norm3 reflect refract onb smith_v smith_g1 bounce vndf
    {23, 3}, {16, 1}, {26, 13}, {27, 13}, {15, 3}, {17, 4},             // eval_light gi_pdf merge merge_gi transform_point intersect_tri
};
int orc_probe_helper_layout(uint32_t fn, uint32_t* in_dwords, uint32_t* out_dwords) {
    if (fn >= SR_PROBE_COUNT) return -1;
    *in_dwords = kProbeWidth[fn][0]; *out_dwords = kProbeWidth[fn][1];
    return 0;
}
static void probe_row(uint32_t fn, const uint32_t* a, uint32_t* o) {
#define F(k) u2f(a[k])
#define V(k) v3(F(k), F((k) + 1), F((k) + 2))
#define OF(k, val) o[k] = f2u(val)
#define O3(k, vec) do { V3 v_ = (vec); OF(k, v_.x); OF((k) + 1, v_.y); OF((k) + 2, v_.z); } while (0)
    switch (fn) {
        case SR_PROBE_SINCOS: { float s, c; sincos_f(F(0), &s, &c); OF(0, s); OF(1, c); break; }
        case SR_PROBE_EXP: OF(0, exp_f(F(0))); break;
        case SR_PROBE_LOG: OF(0, log_f(F(0))); break;
        case SR_PROBE_POW: OF(0, pow_f(F(0), F(1))); break;
        case SR_PROBE_POW5: OF(0, pow5(F(0))); break;
        case SR_PROBE_SMOOTHSTEP: OF(0, smoothstep(F(0), F(1), F(2))); break;
        case SR_PROBE_F32_TO_F16: o[0] = f32_to_f16(F(0)); break;
        case SR_PROBE_F16_TO_F32: OF(0, f16_to_f32(a[0] & 0xFFFFu)); break;
        case SR_PROBE_PACK_HALF_2X16: o[0] = pack_half_2x16(F(0), F(1)); break;
        case SR_PROBE_UNPACK_HALF_2X16: { V2 r = unpack_half_2x16(a[0]); OF(0, r.x); OF(1, r.y); break; }
        case SR_PROBE_PACK_SNORM_2X16: o[0] = pack_snorm_2x16(F(0), F(1)); break;
        case SR_PROBE_UNPACK_SNORM_2X16: { V2 r = unpack_snorm_2x16(a[0]); OF(0, r.x); OF(1, r.y); break; }
        case SR_PROBE_PACK_UNORM_4X8: o[0] = pack_unorm_4x8(F(0), F(1), F(2), F(3)); break;
        case SR_PROBE_UNPACK_UNORM_RGB: { V4 r = unpack_unorm_4x8(a[0]); OF(0, r.x); OF(1, r.y); OF(2, r.z); break; }
        case SR_PROBE_PACK_NORMAL: o[0] = pack_normal(V(0)); break;
        case SR_PROBE_UNPACK_NORMAL: O3(0, unpack_normal(a[0])); break;
        case SR_PROBE_PACK_RGBA8_SNORM: o[0] = pack_rgba8_snorm(F(0), F(1), F(2), F(3)); break;
        case SR_PROBE_UNSNORM8: OF(0, unsnorm8(a[0])); break;
        case SR_PROBE_PACK_B10G11R11: o[0] = pack_b10g11r11(F(0), F(1), F(2)); break;
        case SR_PROBE_UNPACK_B10G11R11: OF(0, from_ufloat(a[0] & 0x7ffu, 6)); OF(1, from_ufloat((a[0] >> 11) & 0x7ffu, 6)); OF(2, from_ufloat(a[0] >> 22, 5)); break;
        case SR_PROBE_PCG_HASH: o[0] = pcg_hash(a[0]); break;
        case SR_PROBE_INIT_RNG: o[0] = init_rng(a[0], a[1], a[2], a[3]).seed; break;
        case SR_PROBE_RND: { Rng r{a[0]}; float x = rnd(r); o[0] = r.seed; OF(1, x); break; }
        case SR_PROBE_NORM3: O3(0, normalize(V(0))); break;
        case SR_PROBE_REFLECT3: O3(0, reflect(V(0), V(3))); break;
        case SR_PROBE_REFRACT3: O3(0, refract(V(0), V(3), F(6))); break;
        case SR_PROBE_BUILD_ONB: { V3 t, b; build_onb(V(0), t, b); O3(0, t); O3(3, b); break; }
        case SR_PROBE_SMITH_V_GGX: OF(0, smith_v_ggx(F(0), F(1), F(2))); break;
        case SR_PROBE_SMITH_G1_GGX: OF(0, smith_g1_ggx(F(0), F(1))); break;
        case SR_PROBE_RANDOM_BOUNCE: O3(0, get_random_bounce(V(0), F(3), F(4))); break;
        case SR_PROBE_SAMPLE_GGX_VNDF: O3(0, sample_ggx_vndf(V(0), V(3), F(6), F(7), F(8))); break;
        case SR_PROBE_EVAL_LIGHT: O3(0, eval_unshadowed_light(V(0), V(3), V(6), V(9), F(12), F(13), V(14), V(17), V(20))); break;
        case SR_PROBE_GI_TARGET_PDF: OF(0, gi_target_pdf(V(0), V(3), V(6), F(9), V(10), V(13))); break;
        case SR_PROBE_MERGE: {
            SrReservoir r, nr;
            memcpy(&r, a, sizeof r); memcpy(&nr, a + 12, sizeof nr);
            const bool taken = merge_reservoirs(r, nr, F(24), F(25));
            memcpy(o, &r, sizeof r); o[12] = taken ? 1u : 0u;
            break;
        }
        case SR_PROBE_MERGE_GI: {
            SrReservoirGI r, nr;
            memcpy(&r, a, sizeof r); memcpy(&nr, a + 12, sizeof nr);
            const bool taken = merge_reservoirs_gi(r, nr, F(24), F(25), F(26));
            memcpy(o, &r, sizeof r); o[12] = taken ? 1u : 0u;
            break;
        }
        case SR_PROBE_TRANSFORM_POINT: { SrTransform x; memcpy(x.m, a, sizeof x.m); O3(0, transform_point(x, V(12))); break; }
        case SR_PROBE_INTERSECT_TRI: {
            WTri tr{V(6), V(9), V(12), 0, 0};
            float t, u, v;
            const bool hit = intersect_tri(V(0), V(3), tr, F(15), F(16), t, u, v);
            o[0] = hit ? 1u : 0u; OF(1, t); OF(2, u); OF(3, v);
            break;
        }
        default: break;
    }
#undef F
#undef V
#undef OF
#undef O3
}
int orc_probe_helper(uint32_t fn, const uint32_t* in, uint32_t n, uint32_t* out) {
    if (fn >= SR_PROBE_COUNT || (n && (!in || !out))) return -1;
    const size_t iw = kProbeWidth[fn][0], ow = kProbeWidth[fn][1];
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) probe_row(fn, in + (size_t)i * iw, out + (size_t)i * ow);
    return 0;
}

}  // extern "C"
