// Strip movement of a multi-device renderer (csrc/multi_renderer.cpp): pack a rectangle of several per-pixel
// planes into one contiguous buffer (the source of one peer copy), unpack it again on the other side, and the guard that makes
// the exactness of the temporal-history exchange checkable.
//
//   strip_pack_kernel / strip_unpack_kernel   one launch per direction for every plane of a rectangle. A rectangle is the full
//       extent across the strip axis and [start, start + size) along it; with column strips (the default axis) a row segment of
//       a plane is only size x bpp bytes, so every (plane, row) segment gets one whole wave whose lanes walk the segment with the
//       widest access its alignment allows (16 B, else 8, 4 or 2): coalesced on both sides.
//   history_reach_check_kernel   after a slot's RIS pass, over its RIS rectangle: from the stored half-precision motion vector,
//       the conservative range of history pixels the pass may have read (kernels.hip, temporal reuse of the DI and GI
//       reservoirs); a pixel whose range leaves what the slot held is counted (one vector atomic per wave).
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "strip_copy.h"

namespace srd {

struct StripArgs {
    uint8_t* img[kStripMaxPlanes];
    uint64_t off[kStripMaxPlanes];     // byte offset of the plane's block in the packed buffer (16-byte aligned)
    uint32_t bpp[kStripMaxPlanes];
    uint32_t unit[kStripMaxPlanes];    // access width in bytes every row segment of the plane is aligned to: 16, 8, 4 or 2
    uint32_t n_planes, W, x0, w, y0, h;
    uint8_t* packed;
};

template <typename T, bool PACK>
SRD void copy_segment(uint8_t* img, uint8_t* buf, uint32_t bytes, uint32_t lane) {
    T* a = reinterpret_cast<T*>(img);
    T* b = reinterpret_cast<T*>(buf);
    const uint32_t n = bytes / (uint32_t)sizeof(T);
    for (uint32_t i = lane; i < n; i += 64u) {
        if (PACK) b[i] = a[i];
        else a[i] = b[i];
    }
}

// one wave per (plane, row) segment, four waves per block
template <bool PACK>
SRD void strip_copy(const StripArgs& a) {
    const uint32_t seg = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t plane = seg / a.h, row = seg - plane * a.h;
    if (plane >= a.n_planes) return;
    const uint32_t bpp = a.bpp[plane], bytes = a.w * bpp;
    uint8_t* img = a.img[plane] + ((uint64_t)(a.y0 + row) * a.W + a.x0) * bpp;
    uint8_t* buf = a.packed + a.off[plane] + (uint64_t)row * bytes;
    switch (a.unit[plane]) {
        case 16: copy_segment<uint4, PACK>(img, buf, bytes, lane); break;
        case 8: copy_segment<uint2, PACK>(img, buf, bytes, lane); break;
        case 4: copy_segment<uint32_t, PACK>(img, buf, bytes, lane); break;
        default: copy_segment<uint16_t, PACK>(img, buf, bytes, lane); break;
    }
}

__global__ __launch_bounds__(256) void strip_pack_kernel(StripArgs a) { strip_copy<true>(a); }
__global__ __launch_bounds__(256) void strip_unpack_kernel(StripArgs a) { strip_copy<false>(a); }

// The RIS pass reads last frame's reservoirs at pcx = (int)(prev_u * W + j - 0.5), j in [0, 1), and stores the motion vector
// inUV - prev_u as half precision (an invalid reprojection as inUV + 2, which reads no history). From the stored value: prev_u * W,
// widened by |mv| * W * 2^-10 + 1 pixels (the half rounding is at most |mv| * 2^-11), then the integer range of the read, clipped
// to the image. Along the strip axis only (x with column strips, y with row strips); across it a slot holds the full extent.
__global__ __launch_bounds__(256) void history_reach_check_kernel(const uint32_t* __restrict__ motion, uint32_t W, uint32_t H,
                                                                  uint32_t axis, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                                                                  int held_lo, int held_hi, unsigned long long* counter) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool outside = false;
    if (i < w * h) {
        const uint32_t px = x0 + i % w, py = y0 + i / w;
        const f2 mv = unpack_half_2x16(motion[(size_t)py * W + px]);
        if (!(mv.x > 1.5f || mv.y > 1.5f)) {
            const bool cols = axis == SR_AXIS_COLS;
            const float m = cols ? mv.x : mv.y;
            const int n = (int)(cols ? W : H);
            const float c = ((float)(cols ? px : py) + 0.5f) - m * (float)n;
            const float e = fabsf(m) * (float)n * (1.0f / 1024.0f) + 1.0f;
            if (!(fabsf(m) <= 1.5f)) {
                outside = true;                                  // not a motion vector the pass can store: count it
            } else {
                int lo = (int)floorf(c - e - 0.5f), hi = (int)ceilf(c + e + 0.5f);
                lo = lo < 0 ? 0 : lo;
                hi = hi > n - 1 ? n - 1 : hi;
                outside = lo <= hi && (lo < held_lo || hi >= held_hi);
            }
        }
    }
    const unsigned long long mask = __ballot(outside);
    if (mask != 0ull && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)mask) - 1)) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

}  // namespace srd

namespace {

uint32_t access_unit(uint64_t a, uint64_t b, uint64_t c) {
    for (uint32_t u = 16; u > 2; u >>= 1)
        if (a % u == 0 && b % u == 0 && c % u == 0) return u;
    return 2;
}

int fill_args(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h, void* packed,
              srd::StripArgs& a) {
    if (n == 0 || n > srd::kStripMaxPlanes || !packed) return -1;
    a = srd::StripArgs{};
    uint64_t off = 0;
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t bpp = planes[p].bpp;
        if (!planes[p].img || bpp == 0 || bpp % 2 != 0) return -1;
        a.img[p] = static_cast<uint8_t*>(planes[p].img);
        a.bpp[p] = bpp;
        a.off[p] = off;
        a.unit[p] = access_unit((uint64_t)x0 * bpp, (uint64_t)W * bpp, (uint64_t)w * bpp);
        off += ((uint64_t)w * h * bpp + 15u) & ~uint64_t(15);
    }
    a.n_planes = n; a.W = W; a.x0 = x0; a.w = w; a.y0 = y0; a.h = h;
    a.packed = static_cast<uint8_t*>(packed);
    return 0;
}

template <bool PACK>
int launch_strip_copy(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                      void* packed, hipStream_t stream) {
    if (w == 0 || h == 0) return 0;
    srd::StripArgs a;
    if (fill_args(planes, n, W, x0, w, y0, h, packed, a) != 0) return -1;
    const uint64_t segments = (uint64_t)n * h;
    const dim3 grid((unsigned)((segments + 3) / 4)), block(256);
    if (PACK) srd::strip_pack_kernel<<<grid, block, 0, stream>>>(a);
    else srd::strip_unpack_kernel<<<grid, block, 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace

size_t srk_strip_packed_bytes(const SrkStripPlane* planes, uint32_t n, uint32_t w, uint32_t h) {
    size_t bytes = 0;
    for (uint32_t p = 0; p < n; p++) bytes += ((size_t)w * h * planes[p].bpp + 15u) & ~size_t(15);
    return bytes;
}

int srk_launch_strip_pack(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                          void* packed, hipStream_t stream) {
    return launch_strip_copy<true>(planes, n, W, x0, w, y0, h, packed, stream);
}

int srk_launch_strip_unpack(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                            const void* packed, hipStream_t stream) {
    return launch_strip_copy<false>(planes, n, W, x0, w, y0, h, const_cast<void*>(packed), stream);
}

int srk_launch_history_reach_check(const uint32_t* motion, uint32_t W, uint32_t H, uint32_t axis, uint32_t x0, uint32_t w,
                                   uint32_t y0, uint32_t h, uint32_t held_lo, uint32_t held_hi, unsigned long long* counter,
                                   hipStream_t stream) {
    const uint64_t n = (uint64_t)w * h;
    if (n == 0) return 0;
    srd::history_reach_check_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(
        motion, W, H, axis, x0, w, y0, h, (int)held_lo, (int)held_hi, counter);
    return (int)hipGetLastError();
}
