// SrRenderer (renderer.cpp) and the multi-device slots behind it (multi_renderer.cpp), shared by the two files.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <vector>

#include "host.h"

struct SrMulti;   // the device slots of a multi-device renderer beyond the first (multi_renderer.cpp); null with one slot

struct SrRenderer {
    int device = 0;
    SrScene* scene = nullptr;
    uint32_t width = 0, height = 0;
    // frame buffers (the reference's transient G-buffer images + temporal resources, lib.rs:320-331,1492-1516)
    // MAX_FRAMES_IN_FLIGHT = 2 (lib.rs:71): the images one frame writes and reads are double-buffered, so raytracing_ris of
    // frame f+1 (own stream) overlaps raytracing_final + the post chain of frame f. The reservoir, accumulation and denoise
    // ping-pongs carry history from frame to frame and stay single sets.
    float* raw_color[2] = {nullptr, nullptr};
    uint16_t* depth[2] = {nullptr, nullptr};
    uint32_t *normal[2] = {nullptr, nullptr}, *diffuse[2] = {nullptr, nullptr}, *motion[2] = {nullptr, nullptr};
    SrReservoir* reservoirs[2] = {nullptr, nullptr};
    SrReservoirGI* reservoirs_gi[2] = {nullptr, nullptr};
    uint32_t *accum[2] = {nullptr, nullptr}, *denoise[2] = {nullptr, nullptr};
    uint32_t* output[2] = {nullptr, nullptr};
    SrRayPayload* primary[2] = {nullptr, nullptr};   // primary-hit hand-off RIS -> final (SrRtParams.primary_payload), part of the per-frame set
    int primary_reuse = 1;                           // SR_PRIMARY_REUSE=0 in the environment: the final pass traces its camera ray itself (A/B)
    hipStream_t s_ris = nullptr, s_final = nullptr;
    hipEvent_t ev_in = nullptr, ev_ris[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    int last_set = 0;
    uint8_t* blue_noise = nullptr;
    uint32_t noise_w = 128, noise_h = 128;
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
    uint64_t frame_of_set[2] = {0, 0};       // absolute frame number last rendered into image set k (its completion = ev_done[k])
    uint64_t completed_frame = 0;            // highest frame known complete on the GPU (frames complete in order)
    std::map<std::array<uint32_t, 4>, uint32_t> sampler_slots;   // dedup like ResourceManager::sampler_slot (resource_manager.rs:491-499)
    int default_sampler = -1;                                    // LINEAR / CLAMP_TO_EDGE (resource_manager.rs:128-136)
    SrMulti* multi = nullptr;                                    // sr_renderer_create_multi with n_devices > 1
    uint32_t strip_axis = SR_AXIS_COLS;                          // axis of sr_renderer_create_multi (strip bounds run along it)
};

// ---- multi-device slots (multi_renderer.cpp); every function here is a no-op / the identity for a one-slot renderer
namespace srmr {
// Every scene the scene-changing calls fan out to: slot 0's (r->scene), then each replica's, in slot order.
std::vector<SrScene*> scenes(const SrRenderer* r);
// After a call that handed out an image / sampler slot on every scene: SR_ERR_STATE unless they are all equal.
int check_same_slots(const std::vector<uint32_t>& slots, const char* what);
// One frame on every slot: trace, exchange, check, gather, post on slot 0; records r->ev_done[k] like the single path.
int render_frame(SrRenderer* r, const SrMatrices& m, int k, hipStream_t caller_stream);
// The replicas follow slot 0: new extent (equal cut), new noise texture, teardown.
int resize(SrRenderer* r, uint32_t width, uint32_t height);
int set_blue_noise(SrRenderer* r, const uint8_t* rgba8, uint32_t w, uint32_t h);
void destroy(SrRenderer* r);
// Waits for every replica's device (device_wait_idle of the other slots).
int synchronize(SrRenderer* r);
}  // namespace srmr
