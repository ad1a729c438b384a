// Host-side launchers of strip_copy.hip (pack / unpack of strip rectangles, the history-reach check) for multi_renderer.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sunray_hip.h"

namespace srd {
constexpr uint32_t kStripMaxPlanes = 5;   // raw_color, depth, normal, diffuse, motion
}

// One per-pixel plane of a full-size image: device pointer and bytes per pixel (even).
struct SrkStripPlane {
    void* img;
    uint32_t bpp;
};

// Size of the packed form of a w x h rectangle of these planes: plane after plane, rows in order, each plane's block padded to 16 B.
size_t srk_strip_packed_bytes(const SrkStripPlane* planes, uint32_t n, uint32_t w, uint32_t h);
// Rectangle [x0, x0 + w) x [y0, y0 + h) of images W pixels wide <-> `packed`, one launch each. 0 or a hipError_t (-1: bad arguments).
int srk_launch_strip_pack(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                          void* packed, hipStream_t stream);
int srk_launch_strip_unpack(const SrkStripPlane* planes, uint32_t n, uint32_t W, uint32_t x0, uint32_t w, uint32_t y0, uint32_t h,
                            const void* packed, hipStream_t stream);
// Adds to *counter the pixels of the RIS rectangle whose temporal-history read may lie outside [held_lo, held_hi) along `axis`.
int srk_launch_history_reach_check(const uint32_t* motion, uint32_t W, uint32_t H, uint32_t axis, uint32_t x0, uint32_t w,
                                   uint32_t y0, uint32_t h, uint32_t held_lo, uint32_t held_hi, unsigned long long* counter,
                                   hipStream_t stream);
