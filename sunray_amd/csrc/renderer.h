// SrRenderer and its device slots, with the error helpers and the few functions that renderer.cpp and multi_renderer.cpp share.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "host.h"

// What one device holds of a renderer: a replica of the scene, the images the two ray-tracing passes write and read, the noise
// texture, two streams. The only owner of per-device state: a renderer on one device is a renderer with one slot.
struct Slot {
    int device = 0;
    SrScene* scene = nullptr;
    // frame buffers (the reference's transient G-buffer images + temporal resources, lib.rs:320-331,1492-1516)
    // MAX_FRAMES_IN_FLIGHT = 2 (lib.rs:71): the images one frame writes and reads are double-buffered, so raytracing_ris of
    // frame f+1 (own stream) overlaps raytracing_final + the post chain of frame f. The reservoir ping-pong carries history
    // from frame to frame and stays a single set.
    float* raw_color[2] = {nullptr, nullptr};
    uint16_t* depth[2] = {nullptr, nullptr};
    uint32_t *normal[2] = {nullptr, nullptr}, *diffuse[2] = {nullptr, nullptr}, *motion[2] = {nullptr, nullptr};
    SrReservoir* reservoirs[2] = {nullptr, nullptr};
    SrReservoirGI* reservoirs_gi[2] = {nullptr, nullptr};
    SrRayPayload* primary[2] = {nullptr, nullptr};   // primary-hit hand-off RIS -> final (SrRtParams.primary_payload), part of the per-frame set
    uint8_t* blue_noise = nullptr;
    uint32_t noise_w = 128, noise_h = 128;
    hipStream_t s_ris = nullptr, s_final = nullptr;
    // ev_done[k] of slot 0 is the completion of the frame last rendered into image set k (after the post chain); of a
    // further slot, the end of its own work on that set
    hipEvent_t ev_ris[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    // strip extras: only where a renderer has several slots (a lone slot holds the whole frame and moves nothing)
    hipEvent_t ev_copy[2] = {nullptr, nullptr};       // this slot's gather copy of image set k has landed on devices[0]
    unsigned long long* overflow = nullptr;           // history-reach counter, on this slot's device
    uint8_t* gather_pack[2] = {nullptr, nullptr};     // packed strip, on this slot's device (slots >= 1)
    uint8_t* gather_stage[2] = {nullptr, nullptr};    // its landing buffer on devices[0]
    size_t gather_bytes = 0;
};

// one entry of the history-exchange plan with its buffers (double-buffered by k on both ends) and completion events
struct Xfer {
    SrStripTransfer t;
    size_t bytes = 0;
    uint8_t* src_buf[2] = {nullptr, nullptr};         // on the source slot's device
    uint8_t* dst_buf[2] = {nullptr, nullptr};         // on the destination slot's device
    hipEvent_t ev[2] = {nullptr, nullptr};            // recorded on the source's s_ris after the copy
};

struct SrRenderer {
    int device = 0;
    std::vector<Slot> slot;                          // never empty; slot[0] is on `device` and runs the post chain
    uint32_t width = 0, height = 0;
    // what exists once per renderer, on `device`: the accumulation and denoise ping-pongs (history, single sets) and the
    // output of each image set
    uint32_t *accum[2] = {nullptr, nullptr}, *denoise[2] = {nullptr, nullptr};
    uint32_t* output[2] = {nullptr, nullptr};
    int primary_reuse = 1;                           // SR_PRIMARY_REUSE=0 in the environment: the final pass traces its camera ray itself (A/B)
    uint32_t pose_batch = SR_POSE_BATCH_OFF;         // sr_renderer_set_pose_batch / SR_POSE_BATCH in the environment: pose_scene poses by one sr_renderer_pose_meshes
    hipEvent_t ev_in = nullptr;
    int last_set = 0;
    // per-frame state
    float prev_view_proj[16];       // zero on the first frame (lib.rs:410), NOT reset by resize
    uint32_t relative_frame_count = 0;
    uint64_t absolute_frame_count = 0;
    SrTraceConfig config;
    std::vector<uint64_t> last_keys;
    std::vector<uint32_t> last_counts;
    std::vector<SrTransform> last_transforms;
    bool instances_valid = false;
    // asset groups of load_scene (lib.rs:802-828): group -> BLAS keys and image slots (both freed by unload_scene)
    uint64_t next_group = 0;
    std::map<uint64_t, std::vector<uint64_t>> scene_groups;
    std::map<uint64_t, std::vector<uint32_t>> scene_images;
    // frame / resize callbacks (lib.rs:537-554): (due frame, fn, user); start-of-frame and end-of-frame ones run once
    struct FrameCb { uint64_t frame; SrFrameCallback fn; void* user; };
    std::vector<FrameCb> start_of_frame_callbacks, end_of_frame_callbacks;
    std::vector<std::pair<SrResizeCallback, void*>> resize_callbacks;
    uint64_t frame_of_set[2] = {0, 0};       // absolute frame number last rendered into image set k (its completion = slot[0].ev_done[k])
    uint64_t completed_frame = 0;            // highest frame known complete on the GPU (frames complete in order)
    std::map<std::array<uint32_t, 4>, uint32_t> sampler_slots;   // dedup like ResourceManager::sampler_slot (resource_manager.rs:491-499)
    int default_sampler = -1;                                    // LINEAR / CLAMP_TO_EDGE (resource_manager.rs:128-136)
    // the cut of the frame into one strip per slot, and what moves between the strips
    SrPartition* part = nullptr;
    uint32_t strip_axis = SR_AXIS_COLS;                          // strip bounds run along it
    uint32_t motion_halo = 32;
    std::vector<Xfer> xfers;
    bool plan_dirty = true;            // partition or halo changed: gather / exchange buffers are rebuilt before the next frame
};

inline int rfail(int code, const std::string& msg) { return srh::set_error(code, msg); }
#define R_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return rfail(e_ == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define R_RC(expr) do { int rc_ = (expr); if (rc_ != SR_OK) return rc_; } while (0)
#define R_LAUNCH(expr) do { int e_ = (expr); if (e_ != 0) return rfail(SR_ERR_HIP, std::string(#expr) + ": " + (e_ < 0 ? "bad arguments" : hipGetErrorString((hipError_t)e_))); } while (0)

namespace srr {
// device_wait_idle on every slot's device, in slot order (renderer.cpp).
int sync_all(SrRenderer* r);
// One frame on every slot into image set k: trace, exchange, check, gather, post chain on slot 0, whose ev_done[k] it records
// (multi_renderer.cpp).
int render_frame(SrRenderer* r, const SrMatrices& m, int k, hipStream_t caller_stream);
// Frees the gather and exchange buffers of the current plan; the caller has waited for every device (multi_renderer.cpp).
void free_transfers(SrRenderer* r);
}  // namespace srr
