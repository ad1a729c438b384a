// Test hook: the inline helpers of rt_device.h / traverse.h, one call per thread, on raw rows of dwords.
//
// The pass kernels and the oracle are compared frame by frame; this unit lets a test compare the small functions under those
// frames one by one, on inputs no frame reaches (sr_probe_helper in include/sunray_hip.h, tests/test_gpu_helper_probe.py).
// Every case calls the header's own function: nothing is restated here. It is a translation unit of its own so that the
// object code of the pass kernels is what it was without it.
#include <hip/hip_runtime.h>

#include <string>

#include "traverse.h"

namespace srh {
int set_error(int code, const std::string& msg);   // the library's error slot (api.cpp); returns `code`
}

namespace {
using namespace srd;

// ids and row widths (dwords in, dwords out); tests/helper_probe.py and oracle/orc_api.cpp hold the same table
struct Width { uint32_t in, out; };
constexpr Width kWidth[SR_PROBE_COUNT] = {
    {1, 2},   // SR_PROBE_SINCOS            x -> sin, cos
    {1, 1},   // SR_PROBE_EXP
    {1, 1},   // SR_PROBE_LOG
    {2, 1},   // SR_PROBE_POW               x, y
    {1, 1},   // SR_PROBE_POW5
    {3, 1},   // SR_PROBE_SMOOTHSTEP        a, b, x
    {1, 1},   // SR_PROBE_F32_TO_F16        float -> half bits
    {1, 1},   // SR_PROBE_F16_TO_F32        half bits -> float
    {2, 1},   // SR_PROBE_PACK_HALF_2X16
    {1, 2},   // SR_PROBE_UNPACK_HALF_2X16
    {2, 1},   // SR_PROBE_PACK_SNORM_2X16
    {1, 2},   // SR_PROBE_UNPACK_SNORM_2X16
    {4, 1},   // SR_PROBE_PACK_UNORM_4X8
    {1, 3},   // SR_PROBE_UNPACK_UNORM_RGB
    {3, 1},   // SR_PROBE_PACK_NORMAL
    {1, 3},   // SR_PROBE_UNPACK_NORMAL
    {4, 1},   // SR_PROBE_PACK_RGBA8_SNORM
    {1, 1},   // SR_PROBE_UNSNORM8
    {3, 1},   // SR_PROBE_PACK_B10G11R11
    {1, 3},   // SR_PROBE_UNPACK_B10G11R11
    {1, 1},   // SR_PROBE_PCG_HASH
    {4, 1},   // SR_PROBE_INIT_RNG          px, py, frame, launch width
    {1, 2},   // SR_PROBE_RND               seed -> new seed, float
    {3, 3},   // SR_PROBE_NORM3
    {6, 3},   // SR_PROBE_REFLECT3          i, n
    {7, 3},   // SR_PROBE_REFRACT3          i, n, eta
    {3, 6},   // SR_PROBE_BUILD_ONB         n -> t, b
    {3, 1},   // SR_PROBE_SMITH_V_GGX       NdotV, NdotL, alpha
    {2, 1},   // SR_PROBE_SMITH_G1_GGX      NdotX, alpha
    {5, 3},   // SR_PROBE_RANDOM_BOUNCE     normal, r1, r2
    {9, 3},   // SR_PROBE_SAMPLE_GGX_VNDF   normal, V, roughness, r1, r2
    {23, 3},  // SR_PROBE_EVAL_LIGHT        hit_pos, hit_normal, V, albedo, roughness, metallic, emission, light_pos, light_normal
    {16, 1},  // SR_PROBE_GI_TARGET_PDF     shade_pos, shade_normal, albedo, metallic, sample_pos, sample_radiance
    {26, 13}, // SR_PROBE_MERGE             SrReservoir r, SrReservoir new, p_hat, random -> r, taken
    {27, 13}, // SR_PROBE_MERGE_GI          SrReservoirGI r, SrReservoirGI new, p_hat, jacobian, random -> r, taken
    {15, 3},  // SR_PROBE_TRANSFORM_POINT   m[12], p
    {17, 4},  // SR_PROBE_INTERSECT_TRI     o, d, v0, e1, e2, tmin, tmax -> hit, t, u, v
};

constexpr int kProbeBlock = 256;

__global__ void __launch_bounds__(kProbeBlock)
helper_probe_kernel(uint32_t fn, const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out, uint32_t in_w, uint32_t out_w) {
    const size_t row = (size_t)blockIdx.x * kProbeBlock + threadIdx.x;
    if (row >= n) return;
    const uint32_t* a = in + row * in_w;
    uint32_t* o = out + row * out_w;
#define F(k) __uint_as_float(a[k])
#define V(k) mk3(F(k), F((k) + 1), F((k) + 2))
#define OF(k, val) o[k] = __float_as_uint(val)
#define O3(k, vec) do { f3 v_ = (vec); OF(k, v_.x); OF((k) + 1, v_.y); OF((k) + 2, v_.z); } while (0)
    switch (fn) {
        case SR_PROBE_SINCOS: { float s, c; sincos_pinned(F(0), s, c); OF(0, s); OF(1, c); break; }
        case SR_PROBE_EXP: OF(0, exp_pinned(F(0))); break;
        case SR_PROBE_LOG: OF(0, log_pinned(F(0))); break;
        case SR_PROBE_POW: OF(0, pow_pinned(F(0), F(1))); break;
        case SR_PROBE_POW5: OF(0, pow5f(F(0))); break;
        case SR_PROBE_SMOOTHSTEP: OF(0, smoothstepf(F(0), F(1), F(2))); break;
        case SR_PROBE_F32_TO_F16: o[0] = f32_to_f16_bits(F(0)); break;
        case SR_PROBE_F16_TO_F32: OF(0, f16_bits_to_f32(a[0])); break;
        case SR_PROBE_PACK_HALF_2X16: o[0] = pack_half_2x16(F(0), F(1)); break;
        case SR_PROBE_UNPACK_HALF_2X16: { f2 r = unpack_half_2x16(a[0]); OF(0, r.x); OF(1, r.y); break; }
        case SR_PROBE_PACK_SNORM_2X16: o[0] = pack_snorm_2x16(F(0), F(1)); break;
        case SR_PROBE_UNPACK_SNORM_2X16: { f2 r = unpack_snorm_2x16(a[0]); OF(0, r.x); OF(1, r.y); break; }
        case SR_PROBE_PACK_UNORM_4X8: o[0] = pack_unorm_4x8(F(0), F(1), F(2), F(3)); break;
        case SR_PROBE_UNPACK_UNORM_RGB: O3(0, unpack_unorm_rgb(a[0])); break;
        case SR_PROBE_PACK_NORMAL: o[0] = pack_normal(V(0)); break;
        case SR_PROBE_UNPACK_NORMAL: O3(0, unpack_normal(a[0])); break;
        case SR_PROBE_PACK_RGBA8_SNORM: o[0] = pack_rgba8_snorm(F(0), F(1), F(2), F(3)); break;
        case SR_PROBE_UNSNORM8: OF(0, unsnorm8(a[0])); break;
        case SR_PROBE_PACK_B10G11R11: o[0] = pack_b10g11r11(F(0), F(1), F(2)); break;
        case SR_PROBE_UNPACK_B10G11R11: O3(0, unpack_b10g11r11(a[0])); break;
        case SR_PROBE_PCG_HASH: o[0] = pcg_hash(a[0]); break;
        case SR_PROBE_INIT_RNG: o[0] = init_rng(a[0], a[1], a[2], a[3]); break;
        case SR_PROBE_RND: { uint32_t seed = a[0]; float r = rnd(seed); o[0] = seed; OF(1, r); break; }
        case SR_PROBE_NORM3: O3(0, norm3(V(0))); break;
        case SR_PROBE_REFLECT3: O3(0, reflect3(V(0), V(3))); break;
        case SR_PROBE_REFRACT3: O3(0, refract3(V(0), V(3), F(6))); break;
        case SR_PROBE_BUILD_ONB: { f3 t, b; build_onb(V(0), t, b); O3(0, t); O3(3, b); break; }
        case SR_PROBE_SMITH_V_GGX: OF(0, smith_v_ggx(F(0), F(1), F(2))); break;
        case SR_PROBE_SMITH_G1_GGX: OF(0, smith_g1_ggx(F(0), F(1))); break;
        case SR_PROBE_RANDOM_BOUNCE: O3(0, get_random_bounce(V(0), F(3), F(4))); break;
        case SR_PROBE_SAMPLE_GGX_VNDF: O3(0, sample_ggx_vndf(V(0), V(3), F(6), F(7), F(8))); break;
        case SR_PROBE_EVAL_LIGHT: O3(0, eval_unshadowed_light(V(0), V(3), V(6), V(9), F(12), F(13), V(14), V(17), V(20))); break;
        case SR_PROBE_GI_TARGET_PDF: OF(0, gi_target_pdf(V(0), V(3), V(6), F(9), V(10), V(13))); break;
        case SR_PROBE_MERGE: {
            SrReservoir r = *(const SrReservoir*)a;
            const SrReservoir nr = *(const SrReservoir*)(a + 12);
            const bool taken = merge_reservoirs(r, nr, F(24), F(25));
            *(SrReservoir*)o = r;
            o[12] = taken ? 1u : 0u;
            break;
        }
        case SR_PROBE_MERGE_GI: {
            SrReservoirGI r = *(const SrReservoirGI*)a;
            const SrReservoirGI nr = *(const SrReservoirGI*)(a + 12);
            const bool taken = merge_reservoirs_gi(r, nr, F(24), F(25), F(26));
            *(SrReservoirGI*)o = r;
            o[12] = taken ? 1u : 0u;
            break;
        }
        case SR_PROBE_TRANSFORM_POINT: {
            float m[12];
            for (int k = 0; k < 12; k++) m[k] = F(k);
            O3(0, transform_point(m, V(12)));
            break;
        }
        case SR_PROBE_INTERSECT_TRI: {
            float t, u, v;
            const bool hit = intersect_tri(V(0), V(3), V(6), V(9), V(12), F(15), F(16), t, u, v);
            o[0] = hit ? 1u : 0u; OF(1, t); OF(2, u); OF(3, v);
            break;
        }
        default: break;   // the entry point refuses an unknown fn before it launches
    }
#undef F
#undef V
#undef OF
#undef O3
}

}  // namespace

extern "C" {

int sr_probe_helper_layout(uint32_t fn, uint32_t* in_dwords, uint32_t* out_dwords) {
    if (fn >= SR_PROBE_COUNT) return srh::set_error(SR_ERR_INVALID_ARG, "sr_probe_helper_layout: unknown helper " + std::to_string(fn));
    if (!in_dwords || !out_dwords) return srh::set_error(SR_ERR_INVALID_ARG, "sr_probe_helper_layout: null pointer");
    *in_dwords = kWidth[fn].in;
    *out_dwords = kWidth[fn].out;
    return SR_OK;
}

int sr_probe_helper(uint32_t fn, const uint32_t* in, uint32_t n, uint32_t* out, void* stream) {
    if (fn >= SR_PROBE_COUNT) return srh::set_error(SR_ERR_INVALID_ARG, "sr_probe_helper: unknown helper " + std::to_string(fn));
    if (n && (!in || !out)) return srh::set_error(SR_ERR_INVALID_ARG, "sr_probe_helper: null pointer");
    if (n == 0) return SR_OK;
    helper_probe_kernel<<<dim3((uint32_t)(((uint64_t)n + kProbeBlock - 1) / kProbeBlock)), dim3(kProbeBlock), 0, (hipStream_t)stream>>>(
        fn, in, n, out, kWidth[fn].in, kWidth[fn].out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return srh::set_error(SR_ERR_HIP, std::string("helper probe kernel launch: ") + hipGetErrorString(e));
    return SR_OK;
}

}  // extern "C"
