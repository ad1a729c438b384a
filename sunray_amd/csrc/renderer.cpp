// Renderer facade: the reference's `Renderer<K>` method surface for the built
// path, layered purely on this library's own C ABI (sr_scene_*, sr_trace_*, sr_post_*):
//   new / resize / load_mesh / unload_mesh / render / wait_frame / render_to_host_memory
// (src/lib.rs:212-446, 586-639, 873-973, 984-1238, 1908-1934). Keys are u64 (the reference's generic
// ResourceKey, lib.rs:54-58). One Renderer = one caller thread (the reference is !Send) and one device slot per GPU it
// renders on (renderer.h): one from sr_renderer_create, one per device from sr_renderer_create_multi.
// Here: the lifetime of the renderer and its slots, the scene-changing calls fanned out to every slot, frame submission and its
// bookkeeping (multi_renderer.cpp: the frame itself on the slots).
#include <hip/hip_runtime.h>

#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host.h"
#include "renderer.h"


struct SrLoadedScene {
    uint64_t group = 0;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> counts;
    std::vector<SrTransform> transforms;
};

namespace {

template <typename T>
void free_ptr(T*& p) { if (p) (void)hipFree(p); p = nullptr; }

template <typename T>
int alloc_zero(T** p, size_t n) {
    R_HIP(hipMalloc((void**)p, n * sizeof(T)));
    R_HIP(hipMemset(*p, 0, n * sizeof(T)));
    return SR_OK;
}

// The frame buffers of slot `s`: what the two passes write and read; with slot 0, the renderer's post-chain images.
void free_images(SrRenderer* r, Slot& s) {
    for (int k = 0; k < 2; k++) {
        free_ptr(s.raw_color[k]); free_ptr(s.depth[k]); free_ptr(s.normal[k]); free_ptr(s.diffuse[k]); free_ptr(s.motion[k]);
        free_ptr(s.reservoirs[k]); free_ptr(s.reservoirs_gi[k]); free_ptr(s.primary[k]);
        if (&s == &r->slot[0]) { free_ptr(r->accum[k]); free_ptr(r->denoise[k]); free_ptr(r->output[k]); }
    }
}

int alloc_images(SrRenderer* r, Slot& s, uint32_t w, uint32_t h) {
    const size_t n = (size_t)w * h;
    const bool post = &s == &r->slot[0];
    R_HIP(hipSetDevice(s.device));
    for (int k = 0; k < 2; k++) {                                  // the two per-frame sets ...
        R_RC(alloc_zero(&s.raw_color[k], n * 4)); R_RC(alloc_zero(&s.depth[k], n)); R_RC(alloc_zero(&s.normal[k], n));
        R_RC(alloc_zero(&s.diffuse[k], n)); R_RC(alloc_zero(&s.motion[k], n));
        if (post) R_RC(alloc_zero(&r->output[k], n));
        if (r->primary_reuse) R_RC(alloc_zero(&s.primary[k], n));
    }
    for (int k = 0; k < 2; k++) {                                  // ... then the ping-pongs that carry history
        R_RC(alloc_zero(&s.reservoirs[k], n)); R_RC(alloc_zero(&s.reservoirs_gi[k], n));
        if (post) { R_RC(alloc_zero(&r->accum[k], n)); R_RC(alloc_zero(&r->denoise[k], n)); }
    }
    return SR_OK;
}

// A noise texture of the caller's (host memory) in place of the one slot `s` holds; s.device is the current device.
int upload_noise(Slot& s, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    uint8_t* fresh = nullptr;
    const size_t bytes = (size_t)w * h * 4;
    R_HIP(hipMalloc((void**)&fresh, bytes));
    if (hipMemcpy(fresh, rgba8, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(fresh); return rfail(SR_ERR_HIP, "Renderer: blue-noise upload failed"); }
    free_ptr(s.blue_noise);
    s.blue_noise = fresh; s.noise_w = w; s.noise_h = h;
    return SR_OK;
}

// Slot `s` on s.device: its scene, frame buffers at the renderer's extent, the noise texture, streams and events.
int create_slot(SrRenderer* r, Slot& s, const std::vector<uint8_t>& noise) {
    R_RC(sr_scene_create(s.device, &s.scene));
    R_RC(alloc_images(r, s, r->width, r->height));
    R_RC(upload_noise(s, noise.data(), 128, 128));
    R_HIP(hipStreamCreateWithFlags(&s.s_ris, hipStreamNonBlocking));
    R_HIP(hipStreamCreateWithFlags(&s.s_final, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        R_HIP(hipEventCreateWithFlags(&s.ev_ris[k], hipEventDisableTiming));
        R_HIP(hipEventCreateWithFlags(&s.ev_done[k], hipEventDisableTiming));
    }
    return SR_OK;
}

// Everything create_slot and create_strip_extras made, or as much of it as there is; the slot's device is idle.
void destroy_slot(SrRenderer* r, Slot& s) {
    (void)hipSetDevice(s.device);
    free_images(r, s);
    free_ptr(s.blue_noise);
    free_ptr(s.overflow);
    for (hipEvent_t e : {s.ev_ris[0], s.ev_ris[1], s.ev_done[0], s.ev_done[1], s.ev_copy[0], s.ev_copy[1]}) if (e) (void)hipEventDestroy(e);
    if (s.s_ris) (void)hipStreamDestroy(s.s_ris);
    if (s.s_final) (void)hipStreamDestroy(s.s_final);
    sr_scene_destroy(s.scene);
}

// Peer access between every pair of distinct devices the slots use, where the platform allows it ("already enabled" is fine).
int enable_peer_access(const SrRenderer* r) {
    for (const Slot& sa : r->slot)
        for (const Slot& sb : r->slot) {
            const int a = sa.device, b = sb.device;
            if (a == b) continue;
            int can = 0;
            R_HIP(hipDeviceCanAccessPeer(&can, a, b));
            if (!can) continue;
            R_HIP(hipSetDevice(a));
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else if (e != hipSuccess) return rfail(SR_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        }
    return SR_OK;
}

// The history-reach counters of a renderer with several slots start again from zero (create, resize).
int reset_overflow(SrRenderer* r) {
    for (Slot& s : r->slot) {
        if (!s.overflow) continue;
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipMemset(s.overflow, 0, sizeof(unsigned long long)));
    }
    return SR_OK;
}

// What only a renderer with several slots needs of each: the history-reach counter and the gather-copy events.
int create_strip_extras(SrRenderer* r) {
    for (Slot& s : r->slot) {
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipMalloc((void**)&s.overflow, sizeof(unsigned long long)));
        for (int k = 0; k < 2; k++) R_HIP(hipEventCreateWithFlags(&s.ev_copy[k], hipEventDisableTiming));
    }
    return reset_overflow(r);
}

// All of a new renderer that can fail, slot 0 first; what a failure leaves half made, sr_renderer_destroy takes down.
int create_slots(SrRenderer* r) {
    std::vector<uint8_t> noise(128 * 128 * 4);
    sr_default_noise_texture(128, 128, 7, noise.data());
    R_RC(create_slot(r, r->slot[0], noise));
    R_HIP(hipEventCreateWithFlags(&r->ev_in, hipEventDisableTiming));
    R_RC(enable_peer_access(r));
    for (size_t i = 1; i < r->slot.size(); i++) R_RC(create_slot(r, r->slot[i], noise));
    if (r->slot.size() > 1) R_RC(create_strip_extras(r));
    R_RC(sr_partition_create(r->width, r->height, (uint32_t)r->slot.size(), r->strip_axis, nullptr, &r->part));
    R_HIP(hipSetDevice(r->device));
    return SR_OK;
}

// Renderer::new((w, h), RGBA8_UNORM) (lib.rs:212-446) on one slot per entry of `devices` (the same device may hold several).
int create_renderer(const int* devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t axis, SrRenderer** out) {
    SrRenderer* r = new SrRenderer();
    r->device = devices[0];
    r->width = width; r->height = height;
    r->strip_axis = axis;
    r->slot.resize(n_devices);
    for (uint32_t i = 0; i < n_devices; i++) r->slot[i].device = devices[i];
    memset(r->prev_view_proj, 0, sizeof(r->prev_view_proj));
    sr_trace_config_default(&r->config);
    if (const char* ev = getenv("SR_PRIMARY_REUSE")) r->primary_reuse = atoi(ev) != 0;
    if (const char* ev = getenv("SR_POSE_BATCH")) r->pose_batch = !strcmp(ev, "on") ? SR_POSE_BATCH_ON : SR_POSE_BATCH_OFF;
    const int rc = create_slots(r);
    if (rc != SR_OK) {
        const std::string msg = sr_last_error();
        sr_renderer_destroy(r);
        return rfail(rc, msg);
    }
    *out = r;
    return SR_OK;
}

// After a call that handed out an image / sampler slot on every scene: SR_ERR_STATE unless they are all equal.
int check_same_slots(const std::vector<uint32_t>& slots, const char* what) {
    for (uint32_t s : slots)
        if (s != slots[0]) return rfail(SR_ERR_STATE, std::string(what) + " slots differ between the replicas");
    return SR_OK;
}

// `call` on every slot's scene in slot order, stopping at the first refusal. The replicas hold the same meshes and settings,
// so what one refuses on validation the first one refuses, and none has changed.
template <class Call>
int each_scene(SrRenderer* r, Call call) {
    for (Slot& s : r->slot)
        if (const int rc = call(s.scene); rc != SR_OK) return rc;
    return SR_OK;
}

// Device-produced vertices for every replica: `produce` runs on the first slot's scene, which validates once; the further
// replicas take the validated bytes (srh::scene_take_device_vertices: device-to-device or peer copy, the same state, no host
// staging) from `src`, or with src == NULL from that scene's scratch buffer, where the mesh-frame producer leaves them.
// What the first scene refuses changes none, and leaves the instance list as valid as it was.
template <class Produce>
int first_scene_produces(SrRenderer* r, uint64_t key, const SrVertex* src, uint32_t n_vertices, Produce produce) {
    int rc = produce(r->slot[0].scene);
    if (rc != SR_OK) return rc;
    r->instances_valid = false;
    if (!src) src = srh::scene_mesh_frame_vertices(r->slot[0].scene, key, &n_vertices);
    for (size_t i = 1; rc == SR_OK && i < r->slot.size(); i++) rc = srh::scene_take_device_vertices(r->slot[i].scene, key, src, n_vertices, r->device);
    return rc;
}

// The same for the pose calls: `pose` runs on the first slot's scene, which poses and validates every item once; the further
// replicas take item k's records (the mesh key_of(k)) from that scene's batch scratch, mesh by mesh.
template <class KeyOf, class Pose>
int first_scene_poses(SrRenderer* r, uint32_t n_items, KeyOf key_of, Pose pose) {
    int rc = pose(r->slot[0].scene);
    if (rc != SR_OK || n_items == 0) return rc;
    r->instances_valid = false;
    for (size_t i = 1; i < r->slot.size(); i++)
        for (uint32_t k = 0; k < n_items; k++) {
            uint32_t n_vertices = 0;
            const SrVertex* src = srh::scene_pose_batch_vertices(r->slot[0].scene, k, &n_vertices);
            if ((rc = srh::scene_take_device_vertices(r->slot[i].scene, key_of(k), src, n_vertices, r->device)) != SR_OK) return rc;
        }
    return SR_OK;
}

// What attach_skins, attach_morphs and pose_scene (`who`) refuse first: a loaded scene that does not come from this file. The
// file's mesh count into *n_blases; its instance count is compared, and given, only where n_instances is not NULL.
int check_scene_of_file(const SrRenderer* r, const SrGltf* g, const SrLoadedScene* ls, const char* who, uint32_t* n_blases, uint32_t* n_instances) {
    if (!r || !g || !ls) return rfail(SR_ERR_INVALID_ARG, std::string(who) + ": null argument");
    uint32_t ni = 0;
    const int rc = sr_gltf_counts(g, n_blases, &ni, nullptr, nullptr, nullptr);
    if (rc != SR_OK) return rc;
    if (*n_blases != ls->keys.size() || (n_instances && ni != ls->transforms.size()))
        return rfail(SR_ERR_INVALID_ARG, std::string(who) + ": the loaded scene does not come from this file (another number of meshes" + (n_instances ? " or instances)" : ")"));
    if (n_instances) *n_instances = ni;
    return SR_OK;
}

uint32_t pcg_hash(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

}  // namespace

int srr::sync_all(SrRenderer* r) {
    for (const Slot& s : r->slot) {
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipDeviceSynchronize());
    }
    return SR_OK;
}

extern "C" {

// Stand-in for the reference's embedded 128x128 blue-noise PNG (lib.rs:281-309), which is an asset and is
// not copied: a hashed white-noise RGBA8 texture (grey replicated to rgb, alpha 255). Same generator as
// sunray_amd.scenes.white_noise_rgba8.
int sr_default_noise_texture(uint32_t w, uint32_t h, uint32_t seed, uint8_t* out_rgba8) {
    if (!out_rgba8 || w == 0 || h == 0) return rfail(SR_ERR_INVALID_ARG, "sr_default_noise_texture: bad argument");
    const uint32_t salt = (uint32_t)(((uint64_t)seed * 2654435761ull) & 0xFFFFFFFFull);
    for (uint32_t i = 0; i < h; i++)
        for (uint32_t j = 0; j < w; j++) {
            const uint8_t v = (uint8_t)(pcg_hash((i * w + j) ^ salt) >> 24);
            uint8_t* q = out_rgba8 + ((size_t)i * w + j) * 4;
            q[0] = q[1] = q[2] = v; q[3] = 255;
        }
    return SR_OK;
}

// Renderer::new((w, h), RGBA8_UNORM) (lib.rs:212-446)
int sr_renderer_create(int device, uint32_t width, uint32_t height, SrRenderer** out) {
    if (!out || width == 0 || height == 0) return rfail(SR_ERR_INVALID_ARG, "Renderer::new: empty extent or null out");
    return create_renderer(&device, 1, width, height, SR_AXIS_COLS, out);
}

// The same on one slot per entry of `devices`, the frame cut into strips along `axis`.
int sr_renderer_create_multi(const int* devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t axis, SrRenderer** out) {
    if (!devices || !out || n_devices == 0 || width == 0 || height == 0)
        return rfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: null argument, no devices or empty extent");
    if (axis != SR_AXIS_COLS && axis != SR_AXIS_ROWS) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: axis must be SR_AXIS_COLS or SR_AXIS_ROWS");
    for (uint32_t i = 0; i < n_devices; i++)
        if (devices[i] < 0) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: negative device index");
    return create_renderer(devices, n_devices, width, height, axis, out);
}

int sr_renderer_set_blue_noise(SrRenderer* r, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    if (!r || !rgba8 || w == 0 || h == 0 || w > 16384 || h > 16384) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_blue_noise: bad argument");
    for (Slot& s : r->slot) {
        if (hipSetDevice(s.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return rfail(SR_ERR_HIP, "sr_renderer_set_blue_noise: device");
        R_RC(upload_noise(s, rgba8, w, h));
    }
    R_HIP(hipSetDevice(r->device));
    return SR_OK;
}

int sr_renderer_destroy(SrRenderer* r) {
    if (!r) return SR_OK;
    for (const Slot& s : r->slot)
        if (hipSetDevice(s.device) == hipSuccess) (void)hipDeviceSynchronize();
    srr::free_transfers(r);
    for (Slot& s : r->slot) destroy_slot(r, s);
    if (r->ev_in) (void)hipEventDestroy(r->ev_in);
    sr_partition_destroy(r->part);
    delete r;
    return SR_OK;
}

// Renderer::resize (lib.rs:586-639): new temporal resources, relative_frame_count = 0; the strips are cut equally again
int sr_renderer_resize(SrRenderer* r, uint32_t width, uint32_t height) {
    if (!r || width == 0 || height == 0) return rfail(SR_ERR_INVALID_ARG, "Renderer::resize: bad argument");
    if (!(width == r->width && height == r->height)) {            // resize_internal_images returns early for an unchanged extent (lib.rs:598-600)
        R_RC(srr::sync_all(r));                                   // device_wait_idle (lib.rs:604), on every slot's device
        srr::free_transfers(r);
        r->width = r->height = 0;                                 // a failure below leaves no extent: nothing renders until a resize succeeds
        for (Slot& s : r->slot) {
            free_images(r, s);
            R_RC(alloc_images(r, s, width, height));
        }
        SrPartition* p = nullptr;
        R_RC(sr_partition_create(width, height, (uint32_t)r->slot.size(), r->strip_axis, nullptr, &p));
        sr_partition_destroy(r->part);
        r->part = p;
        r->plan_dirty = true;
        r->width = width; r->height = height;
        R_RC(reset_overflow(r));
        R_HIP(hipSetDevice(r->device));
        r->relative_frame_count = 0;
    }
    for (auto& cb : r->resize_callbacks) cb.first(cb.second, width, height);   // every resize call, changed extent or not (lib.rs:590-592)
    return SR_OK;
}

// Renderer::add_start_of_frame_callback / add_end_of_frame_callback / add_resize_callback (lib.rs:537-554)
int sr_renderer_add_start_of_frame_callback(SrRenderer* r, SrFrameCallback fn, void* user) {
    if (!r || !fn) return rfail(SR_ERR_INVALID_ARG, "add_start_of_frame_callback: null argument");
    r->start_of_frame_callbacks.push_back({r->absolute_frame_count + 1, fn, user});
    return SR_OK;
}
int sr_renderer_add_end_of_frame_callback(SrRenderer* r, SrFrameCallback fn, void* user) {
    if (!r || !fn) return rfail(SR_ERR_INVALID_ARG, "add_end_of_frame_callback: null argument");
    r->end_of_frame_callbacks.push_back({r->absolute_frame_count + 1, fn, user});
    return SR_OK;
}
int sr_renderer_add_resize_callback(SrRenderer* r, SrResizeCallback fn, void* user) {
    if (!r || !fn) return rfail(SR_ERR_INVALID_ARG, "add_resize_callback: null argument");
    r->resize_callbacks.push_back({fn, user});
    return SR_OK;
}

namespace {
// run_start_of_frame_callbacks (lib.rs:558-568) and run_due_end_of_frame_callbacks (:572-583), in registration order.
// A callback may register further callbacks (they are tagged with a later frame and stay queued).
void run_frame_callbacks(SrRenderer* r, uint64_t upcoming_frame) {
    for (size_t i = 0; i < r->start_of_frame_callbacks.size();) {
        if (r->start_of_frame_callbacks[i].frame <= upcoming_frame) {
            const SrRenderer::FrameCb cb = r->start_of_frame_callbacks[i];
            r->start_of_frame_callbacks.erase(r->start_of_frame_callbacks.begin() + (long)i);
            cb.fn(cb.user);
        } else i++;
    }
    // the frame timeline: frames complete in order; a set's ev_done is the completion of the frame last rendered into it
    for (int k = 0; k < 2; k++)
        if (r->frame_of_set[k] > r->completed_frame && hipEventQuery(r->slot[0].ev_done[k]) == hipSuccess) r->completed_frame = r->frame_of_set[k];
    for (size_t i = 0; i < r->end_of_frame_callbacks.size();) {
        if (r->end_of_frame_callbacks[i].frame <= r->completed_frame) {
            const SrRenderer::FrameCb cb = r->end_of_frame_callbacks[i];
            r->end_of_frame_callbacks.erase(r->end_of_frame_callbacks.begin() + (long)i);
            cb.fn(cb.user);
        } else i++;
    }
}
}  // namespace

// Renderer::load_mesh (lib.rs:873-954)
int sr_renderer_load_mesh(SrRenderer* r, uint64_t key, const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                          uint32_t n_indices, const SrMaterial* material) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "load_mesh: renderer is null");
    r->instances_valid = false;
    return each_scene(r, [&](SrScene* sc) { return sr_scene_add_mesh(sc, key, vertices, n_vertices, indices, n_indices, material, nullptr); });
}

int sr_renderer_set_config(SrRenderer* r, const SrTraceConfig* cfg) {
    if (!r || !cfg) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_config: null argument");
    r->config = *cfg;
    return SR_OK;
}

namespace {
int render_passes(SrRenderer* r, const float cam_pos[3], const float cam_target[3], float fov_y, void* stream, uint64_t* out_frame);
}

// Renderer::render (lib.rs:984-1232): one frame = TLAS (re)build when the instance list changed ->
// raytracing_ris -> raytracing_final -> temporal_accumulation -> denoise_0..3 -> postprocess, enqueued on the
// renderer's own streams (two per slot, srr::render_frame) after whatever the caller has enqueued on `stream`; returns the frame number to wait
// on. Two frames may be in flight (MAX_FRAMES_IN_FLIGHT, lib.rs:71): submit frame f+1 before waiting for frame f and
// its RIS pass overlaps frame f's final pass and post chain. Results equal back-to-back execution.
int sr_renderer_render(SrRenderer* r, const float cam_pos[3], const float cam_target[3], float fov_y, const uint64_t* keys,
                       const uint32_t* counts, uint32_t n_keys, const SrTransform* transforms, void* stream, uint64_t* out_frame) {
    if (!r || !cam_pos || !cam_target) return rfail(SR_ERR_INVALID_ARG, "Renderer::render: null argument");
    R_HIP(hipSetDevice(r->device));
    run_frame_callbacks(r, r->absolute_frame_count + 1);            // start of frame (lib.rs:1004-1010)
    // instances: the acceleration structure follows the caller's list — update in place / fast rebuild / settle as
    // AsState decides (tlas.rs:155-191, acceleration_structure/mod.rs:62-148); an identical list is a quiet frame
    uint32_t n_xf = 0;
    for (uint32_t k = 0; k < n_keys; k++) n_xf += counts[k];
    const bool same = r->instances_valid && r->last_keys.size() == n_keys && r->last_transforms.size() == n_xf &&
                      (n_keys == 0 || (memcmp(r->last_keys.data(), keys, n_keys * 8) == 0 && memcmp(r->last_counts.data(), counts, n_keys * 4) == 0)) &&
                      (n_xf == 0 || memcmp(r->last_transforms.data(), transforms, n_xf * sizeof(SrTransform)) == 0);
    if (!same) {
        // every replica, in slot order (host BVH build per replica)
        if (const int rc = each_scene(r, [&](SrScene* sc) { return sr_scene_set_instances(sc, keys, counts, n_keys, transforms); }); rc != SR_OK) return rc;
        r->last_keys.assign(keys, keys + n_keys);
        r->last_counts.assign(counts, counts + n_keys);
        r->last_transforms.assign(transforms, transforms + n_xf);
        r->instances_valid = true;
    } else {
        if (const int rc = each_scene(r, sr_scene_end_frame); rc != SR_OK) return rc;    // quiet frame: the heuristic may settle with a quality rebuild
    }
    return render_passes(r, cam_pos, cam_target, fov_y, stream, out_frame);
}

// sr_renderer_render with the instance list taken from device memory on the first slot's GPU: that slot's scene validates the
// transforms once (sr_scene_set_instances_device), the further replicas take them device to device. The list always counts as
// changed: there is no host copy to compare, and the cached one is void.
int sr_renderer_render_device_transforms(SrRenderer* r, const float cam_pos[3], const float cam_target[3], float fov_y, const uint64_t* keys,
                                         const uint32_t* counts, uint32_t n_keys, const SrTransform* d_transforms, void* stream, uint64_t* out_frame) {
    if (!r || !cam_pos || !cam_target) return rfail(SR_ERR_INVALID_ARG, "Renderer::render: null argument");
    R_HIP(hipSetDevice(r->device));
    run_frame_callbacks(r, r->absolute_frame_count + 1);
    r->instances_valid = false;
    r->last_transforms.clear();
    int rc = sr_scene_set_instances_device(r->slot[0].scene, keys, counts, n_keys, d_transforms, stream);
    for (size_t i = 1; rc == SR_OK && i < r->slot.size(); i++) rc = srh::scene_set_instances_from(r->slot[i].scene, keys, counts, n_keys, d_transforms, r->device);
    if (rc != SR_OK) return rc;
    R_HIP(hipSetDevice(r->device));
    return render_passes(r, cam_pos, cam_target, fov_y, stream, out_frame);
}

namespace {
// The frame behind its instance list (the rest of Renderer::render): camera, the passes on every slot (srr::render_frame), frame counters.
int render_passes(SrRenderer* r, const float cam_pos[3], const float cam_target[3], float fov_y, void* stream, uint64_t* out_frame) {
    SrMatrices m;
    int rc = sr_camera_matrices(cam_pos, cam_target, fov_y, r->width, r->height, r->prev_view_proj, &m);   // lib.rs:1017-1048
    if (rc != SR_OK) return rc;
    memcpy(r->prev_view_proj, m.view_proj, sizeof(r->prev_view_proj));                                     // history for the NEXT frame
    const int k = (int)(r->relative_frame_count & 1u);              // image set of this frame
    if ((rc = srr::render_frame(r, m, k, (hipStream_t)stream)) != SR_OK) return rc;
    r->last_set = k;
    r->relative_frame_count += 1;                                    // lib.rs:1438-1439
    r->absolute_frame_count += 1;
    r->frame_of_set[k] = r->absolute_frame_count;
    if (out_frame) *out_frame = r->absolute_frame_count;
    return SR_OK;
}
}  // namespace

// Renderer::wait_frame (lib.rs:1234-1238): frames complete in order; waits for the latest submitted one.
int sr_renderer_wait_frame(SrRenderer* r, uint64_t frame) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "wait_frame: renderer is null");
    if (frame > r->absolute_frame_count) return rfail(SR_ERR_INVALID_ARG, "wait_frame: frame was never submitted");
    if (frame + 1 >= r->absolute_frame_count && r->absolute_frame_count > 0) {
        // the last submitted frame used image set last_set, the one before it the other set; older frames are long done
        const int k = frame == r->absolute_frame_count ? r->last_set : (r->last_set ^ 1);
        R_HIP(hipEventSynchronize(r->slot[0].ev_done[k]));
    }
    return SR_OK;
}

// Renderer::render_to_host_memory (lib.rs:1908-1934): WARMUP_FRAMES = 16 x (render + wait_frame), then the
// RGBA8 image without padding (W*H*4 bytes).
int sr_renderer_render_to_host_memory(SrRenderer* r, const float cam_pos[3], const float cam_target[3], float fov_y, const uint64_t* keys,
                                      const uint32_t* counts, uint32_t n_keys, const SrTransform* transforms, uint8_t* out_rgba8) {
    if (!r || !out_rgba8) return rfail(SR_ERR_INVALID_ARG, "render_to_host_memory: null argument");
    const uint32_t WARMUP_FRAMES = 16;
    for (uint32_t i = 0; i < WARMUP_FRAMES; i++) {
        uint64_t frame = 0;
        int rc = sr_renderer_render(r, cam_pos, cam_target, fov_y, keys, counts, n_keys, transforms, nullptr, &frame);
        if (rc != SR_OK) return rc;
        if ((rc = sr_renderer_wait_frame(r, frame)) != SR_OK) return rc;
    }
    R_HIP(hipMemcpy(out_rgba8, r->output[r->last_set], (size_t)r->width * r->height * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

// ---- scene loading (lib.rs:779-857, resource_manager.rs:372-413) -------------------------------------------
namespace {
int sampler_slot(SrRenderer* r, const SrSamplerDesc& d, uint32_t* out) {
    const std::array<uint32_t, 4> k = {d.min_filter, d.mag_filter, d.address_mode_u, d.address_mode_v};
    auto it = r->sampler_slots.find(k);
    if (it != r->sampler_slots.end()) { *out = it->second; return SR_OK; }
    std::vector<uint32_t> slots;
    for (Slot& s : r->slot) {
        int rc = sr_scene_add_sampler(s.scene, &d, out);
        if (rc != SR_OK) return rc;
        slots.push_back(*out);
    }
    int rc = check_same_slots(slots, "load_scene: sampler");
    if (rc == SR_OK) r->sampler_slots[k] = *out;
    return rc;
}
}  // namespace

// Renderer::load_scene: uploads the parsed scene's images, samplers and BLASes under fresh keys of a new group.
int sr_renderer_load_scene(SrRenderer* r, const SrGltf* g, SrLoadedScene** out) {
    if (!r || !g || !out) return rfail(SR_ERR_INVALID_ARG, "load_scene: null argument");
    R_RC(srr::sync_all(r));                              // device_wait_idle (lib.rs:800), on every slot's device
    uint32_t n_blases = 0, n_instances = 0, n_images = 0, n_samplers = 0, n_textures = 0;
    int rc = sr_gltf_counts(g, &n_blases, &n_instances, &n_images, &n_samplers, &n_textures);
    if (rc != SR_OK) return rc;
    const uint64_t group = r->next_group++;
    std::vector<uint32_t> image_slots(n_images), smp_slots(n_samplers);
    std::vector<uint32_t>& group_images = r->scene_images[group];     // freed again by unload_scene (also after a failed load)
    std::vector<Slot>& scs = r->slot;                                // parsed once, uploaded to every replica
    for (uint32_t i = 0; i < n_images; i++) {
        const uint8_t* px; uint32_t w, h, ch;
        std::vector<uint32_t> slots;
        if ((rc = sr_gltf_image(g, i, &px, &w, &h, &ch)) == SR_OK)
            for (Slot& s : scs) {
                uint32_t sl = 0;
                if ((rc = sr_scene_add_image(s.scene, px, w, h, ch, &sl)) != SR_OK) break;
                slots.push_back(sl);
            }
        if (rc == SR_OK) rc = check_same_slots(slots, "load_scene: image");
        if (rc != SR_OK) {
            for (size_t j = 0; j < slots.size(); j++) sr_scene_remove_image(scs[j].scene, slots[j]);
            for (uint32_t sl : group_images) for (Slot& s : scs) sr_scene_remove_image(s.scene, sl);
            r->scene_images.erase(group);
            return rc;
        }
        image_slots[i] = slots[0];
        group_images.push_back(image_slots[i]);
    }
    for (uint32_t i = 0; i < n_samplers; i++) {
        SrSamplerDesc d;
        if ((rc = sr_gltf_sampler(g, i, &d)) != SR_OK || (rc = sampler_slot(r, d, &smp_slots[i])) != SR_OK) return rc;
    }
    if (r->default_sampler < 0) {
        const SrSamplerDesc d = {SR_FILTER_LINEAR, SR_FILTER_LINEAR, SR_ADDRESS_CLAMP_TO_EDGE, SR_ADDRESS_CLAMP_TO_EDGE};
        uint32_t slot;
        if ((rc = sampler_slot(r, d, &slot)) != SR_OK) return rc;
        r->default_sampler = (int)slot;
    }
    SrLoadedScene* ls = new SrLoadedScene();
    ls->group = group;
    std::vector<uint64_t> group_keys;
    for (uint32_t b = 0; b < n_blases; b++) {
        const SrVertex* v; const uint32_t* idx; const SrEmissiveTriangle* et; uint32_t nv, ni, ne;
        SrMaterial m;
        if ((rc = sr_gltf_blas(g, b, &v, &nv, &idx, &ni, &m, &et, &ne)) != SR_OK) { delete ls; return rc; }
        uint32_t* slots = &m.base_color_image;             // Material::new's `resolve` (resource_manager.rs:388-398)
        for (int k = 0; k < 10; k += 2) {
            if (slots[k] == SR_NULL_TEXTURE) continue;
            int32_t smp; uint32_t src;
            if ((rc = sr_gltf_texture(g, slots[k], &smp, &src)) != SR_OK) { delete ls; return rc; }
            slots[k] = image_slots[src];
            slots[k + 1] = smp >= 0 ? smp_slots[smp] : (uint32_t)r->default_sampler;
        }
        const uint64_t key = (group << 32) | (uint64_t)b;   // ResourceKey{group, index}
        for (size_t j = 0; j < scs.size() && rc == SR_OK; j++)
            if ((rc = sr_scene_add_blas(scs[j].scene, key, v, nv, idx, ni, &m, et, ne, nullptr)) != SR_OK)
                for (size_t i = 0; i < j; i++) sr_scene_remove(scs[i].scene, key);
        if (rc != SR_OK) {
            for (uint64_t k : group_keys) for (Slot& s : scs) sr_scene_remove(s.scene, k);
            delete ls;
            return rc;
        }
        group_keys.push_back(key);
        ls->keys.push_back(key);
    }
    // group the per-instance transforms by BLAS key, preserving order (lib.rs:830-834)
    std::vector<std::vector<SrTransform>> grouped(n_blases);
    for (uint32_t i = 0; i < n_instances; i++) {
        uint32_t b; SrTransform t;
        if ((rc = sr_gltf_instance(g, i, &b, &t)) != SR_OK) { delete ls; return rc; }
        grouped[b].push_back(t);
    }
    for (uint32_t b = 0; b < n_blases; b++) {
        ls->counts.push_back((uint32_t)grouped[b].size());
        ls->transforms.insert(ls->transforms.end(), grouped[b].begin(), grouped[b].end());
    }
    r->scene_groups[group] = group_keys;
    r->instances_valid = false;
    *out = ls;
    return SR_OK;
}

// Renderer::load_gltf (lib.rs:779-786)
int sr_renderer_load_gltf(SrRenderer* r, const char* path, SrLoadedScene** out) {
    if (!r || !path || !out) return rfail(SR_ERR_INVALID_ARG, "load_gltf: null argument");
    SrGltf* g = nullptr;
    int rc = sr_gltf_open(path, &g);
    if (rc != SR_OK) return rc;
    rc = sr_renderer_load_scene(r, g, out);
    sr_gltf_close(g);
    return rc;
}

int sr_loaded_scene_get(const SrLoadedScene* ls, uint64_t* group, const uint64_t** keys, const uint32_t** counts, uint32_t* n_keys,
                        const SrTransform** transforms, uint32_t* n_transforms) {
    if (!ls) return rfail(SR_ERR_INVALID_ARG, "sr_loaded_scene_get: null argument");
    if (group) *group = ls->group;
    if (keys) *keys = ls->keys.data();
    if (counts) *counts = ls->counts.data();
    if (n_keys) *n_keys = (uint32_t)ls->keys.size();
    if (transforms) *transforms = ls->transforms.data();
    if (n_transforms) *n_transforms = (uint32_t)ls->transforms.size();
    return SR_OK;
}
int sr_loaded_scene_destroy(SrLoadedScene* ls) { delete ls; return SR_OK; }

// Renderer::unload_scene (lib.rs:849-857): frees every asset the load created — the BLASes and, as
// ResourceManager::remove does (resource_manager.rs:459-472), the images; instances of those keys must no longer be
// passed to render. Loading and unloading a scene repeatedly leaks no HBM.
int sr_renderer_unload_scene(SrRenderer* r, uint64_t group) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "unload_scene: renderer is null");
    R_RC(srr::sync_all(r));                                          // device_wait_idle (lib.rs:850), on every slot's device
    auto it = r->scene_groups.find(group);
    if (it != r->scene_groups.end()) {
        for (uint64_t k : it->second) R_RC(each_scene(r, [&](SrScene* sc) { return sr_scene_remove(sc, k); }));
        r->scene_groups.erase(it);
    }
    auto im = r->scene_images.find(group);
    if (im != r->scene_images.end()) {
        for (uint32_t sl : im->second) R_RC(each_scene(r, [&](SrScene* sc) { return sr_scene_remove_image(sc, sl); }));
        r->scene_images.erase(im);
    }
    r->instances_valid = false;
    return SR_OK;
}

// Renderer::unload_mesh (lib.rs:965-973). The reference defers the removal past the frames in flight; here the
// scene waits for the device, so it is immediate.
int sr_renderer_unload_mesh(SrRenderer* r, uint64_t key) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "unload_mesh: renderer is null");
    r->instances_valid = false;
    return each_scene(r, [&](SrScene* sc) { return sr_scene_remove(sc, key); });
}

// Blas::update (blas.rs:285-310) through the facade: every replica takes the new vertices; the next render re-submits the
// instance list, and that sr_scene_set_instances applies the update. Frames in flight: each sr_scene_update_mesh waits for
// its scene's device (hipDeviceSynchronize) before the device copy of the vertices changes, so the passes of the frames
// submitted before have finished; no wait_frame is needed from the caller. The replicas hold the same meshes, so a call the
// first one refuses on validation changes none of them (only those refusals are all-or-nothing: a device error on a later
// replica leaves the earlier ones updated, and the instance list is re-submitted in any case).
int sr_renderer_update_mesh(SrRenderer* r, uint64_t key, const SrVertex* vertices, uint32_t n_vertices) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "update_mesh: renderer is null");
    r->instances_valid = false;
    return each_scene(r, [&](SrScene* sc) { return sr_scene_update_mesh(sc, key, vertices, n_vertices); });
}

// The same for vertices on the first slot's device: sr_scene_update_mesh_device validates them there, once, and the further
// replicas take them straight from the caller's buffer. This call re-submits the instance list also where it refuses.
int sr_renderer_update_mesh_device(SrRenderer* r, uint64_t key, const SrVertex* d_vertices, uint32_t n_vertices, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "update_mesh: renderer is null");
    r->instances_valid = false;
    return first_scene_produces(r, key, d_vertices, n_vertices, [&](SrScene* sc) { return sr_scene_update_mesh_device(sc, key, d_vertices, n_vertices, stream); });
}

// A mesh's rig lives on the first slot's scene only: that scene poses, the further replicas take the posed vertices.
int sr_renderer_set_mesh_skin(SrRenderer* r, uint64_t key, const SrSkinInfluence* influences, uint32_t n_vertices, uint32_t n_joints) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "set_mesh_skin: null argument (the renderer)");
    return sr_scene_set_mesh_skin(r->slot[0].scene, key, influences, n_vertices, n_joints);
}

// sr_scene_skin_mesh on the first slot's scene, which poses and validates once (first_scene_poses, one item).
int sr_renderer_skin_mesh(SrRenderer* r, uint64_t key, const SrTransform* joint_matrices, uint32_t n_joints, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "skin_mesh: null argument (the renderer)");
    return first_scene_poses(r, 1, [&](uint32_t) { return key; }, [&](SrScene* sc) { return sr_scene_skin_mesh(sc, key, joint_matrices, n_joints, stream); });
}

// A mesh's morph lives on the first slot's scene only, like its rig.
int sr_renderer_set_mesh_morph(SrRenderer* r, uint64_t key, const SrMorphDelta* deltas, uint32_t n_vertices, uint32_t n_targets) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "set_mesh_morph: null argument (the renderer)");
    return sr_scene_set_mesh_morph(r->slot[0].scene, key, deltas, n_vertices, n_targets);
}

// sr_scene_pose_mesh on the first slot's scene, which morphs, skins and validates once (first_scene_poses, one item).
int sr_renderer_pose_mesh(SrRenderer* r, uint64_t key, const float* weights, uint32_t n_targets, const SrTransform* joint_matrices, uint32_t n_joints, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "pose_mesh: null argument (the renderer)");
    return first_scene_poses(r, 1, [&](uint32_t) { return key; }, [&](SrScene* sc) { return sr_scene_pose_mesh(sc, key, weights, n_targets, joint_matrices, n_joints, stream); });
}

// sr_scene_pose_meshes on the first slot's scene, which poses and validates the whole batch once; the further replicas take each
// item's records from that scene's batch scratch, mesh by mesh (first_scene_poses).
int sr_renderer_pose_meshes(SrRenderer* r, const SrPoseItem* items, uint32_t n_items, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "pose_meshes: null argument (the renderer)");
    return first_scene_poses(r, n_items, [&](uint32_t k) { return items[k].key; }, [&](SrScene* sc) { return sr_scene_pose_meshes(sc, items, n_items, stream); });
}

// Clips live on the first slot's scene only: that scene evaluates them and poses, the further replicas take the posed records
// (first_scene_poses), and the instance transforms the clip kernel wrote belong to the first device.
int sr_renderer_attach_clip(SrRenderer* r, const SrClip* clip, uint32_t* clip_id) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "attach_clip: null argument (the renderer)");
    return sr_scene_attach_clip(r->slot[0].scene, clip, clip_id);
}

int sr_renderer_detach_clip(SrRenderer* r, uint32_t clip_id) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "detach_clip: null argument (the renderer)");
    return sr_scene_detach_clip(r->slot[0].scene, clip_id);
}

int sr_renderer_pose_actors(SrRenderer* r, const SrClipActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items, SrTransform* d_instance_transforms,
                            uint32_t flags, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "pose_actors: null argument (the renderer)");
    if (n_items && !items) return rfail(SR_ERR_INVALID_ARG, "pose_actors: null argument (actors or items, with a count > 0)");
    return first_scene_poses(r, n_items, [&](uint32_t k) { return items[k].key; },
                             [&](SrScene* sc) { return sr_scene_pose_actors(sc, actors, n_actors, items, n_items, d_instance_transforms, flags, stream); });
}

int sr_renderer_pose_actors_blended(SrRenderer* r, const SrClipBlendActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                    SrTransform* d_instance_transforms, uint32_t flags, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "pose_actors_blended: null argument (the renderer)");
    if (n_items && !items) return rfail(SR_ERR_INVALID_ARG, "pose_actors_blended: null argument (actors or items, with a count > 0)");
    return first_scene_poses(r, n_items, [&](uint32_t k) { return items[k].key; },
                             [&](SrScene* sc) { return sr_scene_pose_actors_blended(sc, actors, n_actors, items, n_items, d_instance_transforms, flags, stream); });
}

// Node masks live on the first slot's scene only, as the clips do.
int sr_renderer_attach_node_mask(SrRenderer* r, const float* weights, uint32_t n_nodes, uint32_t* mask_id) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "attach_node_mask: null argument (the renderer)");
    return sr_scene_attach_node_mask(r->slot[0].scene, weights, n_nodes, mask_id);
}

int sr_renderer_detach_node_mask(SrRenderer* r, uint32_t mask_id) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "detach_node_mask: null argument (the renderer)");
    return sr_scene_detach_node_mask(r->slot[0].scene, mask_id);
}

int sr_renderer_pose_actors_layered(SrRenderer* r, const SrClipLayerActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                    SrTransform* d_instance_transforms, uint32_t flags, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "pose_actors_layered: null argument (the renderer)");
    if (n_items && !items) return rfail(SR_ERR_INVALID_ARG, "pose_actors_layered: null argument (actors or items, with a count > 0)");
    return first_scene_poses(r, n_items, [&](uint32_t k) { return items[k].key; },
                             [&](SrScene* sc) { return sr_scene_pose_actors_layered(sc, actors, n_actors, items, n_items, d_instance_transforms, flags, stream); });
}

int sr_renderer_actor_pose_info(const SrRenderer* r, SrActorPoseInfo* out) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_actor_pose_info: null argument (the renderer)");
    return sr_scene_actor_pose_info(r->slot[0].scene, out);
}

int sr_renderer_spline_pose_info(const SrRenderer* r, SrSplinePoseInfo* out) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_spline_pose_info: null argument (the renderer)");
    return sr_scene_spline_pose_info(r->slot[0].scene, out);
}

int sr_renderer_layer_weights_info(const SrRenderer* r, SrLayerWeightsInfo* out) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_layer_weights_info: null argument (the renderer)");
    return sr_scene_layer_weights_info(r->slot[0].scene, out);
}

// How sr_renderer_pose_scene poses (SR_POSE_BATCH_*).
int sr_renderer_set_pose_batch(SrRenderer* r, uint32_t mode) {
    if (mode > SR_POSE_BATCH_ON) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_pose_batch: mode must be SR_POSE_BATCH_OFF or SR_POSE_BATCH_ON");
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_pose_batch: renderer is null");
    r->pose_batch = mode;
    return SR_OK;
}

// A mesh's frame lives on the first slot's scene only, like its rig.
int sr_renderer_set_mesh_frame(SrRenderer* r, uint64_t key, uint32_t flags) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "set_mesh_frame: null argument (the renderer)");
    return sr_scene_set_mesh_frame(r->slot[0].scene, key, flags);
}

// sr_scene_update_mesh_positions* on the first slot's scene, which produces the records and validates once (first_scene_produces).
int sr_renderer_update_mesh_positions_device(SrRenderer* r, uint64_t key, const float* d_positions, uint32_t n_vertices, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "update_mesh_positions: null argument (the renderer)");
    return first_scene_produces(r, key, nullptr, 0, [&](SrScene* sc) { return sr_scene_update_mesh_positions_device(sc, key, d_positions, n_vertices, stream); });
}
int sr_renderer_update_mesh_positions(SrRenderer* r, uint64_t key, const float* positions, uint32_t n_vertices, void* stream) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "update_mesh_positions: null argument (the renderer)");
    return first_scene_produces(r, key, nullptr, 0, [&](SrScene* sc) { return sr_scene_update_mesh_positions(sc, key, positions, n_vertices, stream); });
}

// The morph targets of a loaded scene, as sr_renderer_attach_skins attaches its rigs.
int sr_renderer_attach_morphs(SrRenderer* r, const SrGltf* g, const SrLoadedScene* ls) {
    uint32_t n_blases = 0;
    int rc = check_scene_of_file(r, g, ls, "attach_morphs", &n_blases, nullptr);
    if (rc != SR_OK) return rc;
    for (uint32_t b = 0; b < n_blases; b++) {
        const SrMorphDelta* deltas = nullptr; uint32_t nv = 0, n_targets = 0;
        if ((rc = sr_gltf_blas_morph(g, b, &n_targets, &deltas, &nv, nullptr)) != SR_OK) return rc;
        if (n_targets == 0) continue;
        if ((rc = sr_renderer_set_mesh_morph(r, ls->keys[b], deltas, nv, n_targets)) != SR_OK) return rc;
        if ((rc = sr_renderer_set_mesh_build_type(r, ls->keys[b], SR_BUILD_RAPIDLY_CHANGING)) != SR_OK) return rc;
    }
    return SR_OK;
}

// The rigs of a loaded scene: keys are in blas order (sr_renderer_load_scene), so blas b of the file is loaded->keys[b].
int sr_renderer_attach_skins(SrRenderer* r, const SrGltf* g, const SrLoadedScene* ls) {
    uint32_t n_blases = 0;
    int rc = check_scene_of_file(r, g, ls, "attach_skins", &n_blases, nullptr);
    if (rc != SR_OK) return rc;
    for (uint32_t b = 0; b < n_blases; b++) {
        int32_t skin = -1; const SrSkinInfluence* inf = nullptr; uint32_t nv = 0, n_joints = 0;
        if ((rc = sr_gltf_blas_skin(g, b, &skin, &inf, &nv)) != SR_OK) return rc;
        if (skin < 0) continue;
        if ((rc = sr_gltf_skin(g, (uint32_t)skin, &n_joints, nullptr, nullptr)) != SR_OK) return rc;
        if ((rc = sr_renderer_set_mesh_skin(r, ls->keys[b], inf, nv, n_joints)) != SR_OK) return rc;
        if ((rc = sr_renderer_set_mesh_build_type(r, ls->keys[b], SR_BUILD_RAPIDLY_CHANGING)) != SR_OK) return rc;
    }
    return SR_OK;
}

int sr_renderer_pose_scene(SrRenderer* r, const SrGltf* g, const SrLoadedScene* ls, int32_t animation, float time_seconds, SrTransform* instance_transforms_out, void* stream) {
    uint32_t n_blases = 0, n_instances = 0;
    int rc = check_scene_of_file(r, g, ls, "pose_scene", &n_blases, &n_instances);
    if (rc != SR_OK) return rc;
    std::vector<SrTransform> posed(n_instances), joints;
    if ((rc = sr_gltf_pose(g, animation, time_seconds, posed.data(), 0, nullptr)) != SR_OK) return rc;
    std::vector<float> weights;
    // SR_POSE_BATCH_ON: the same meshes with the same arguments, collected (the arrays stay alive until the call) and posed at once
    const bool batch = r->pose_batch == SR_POSE_BATCH_ON;
    std::vector<std::vector<SrTransform>> item_joints;
    std::vector<std::vector<float>> item_weights;
    std::vector<SrPoseItem> items;
    for (uint32_t b = 0; b < n_blases; b++) {
        // a mesh with a morph attached (sr_renderer_attach_morphs) is posed by sr_renderer_pose_mesh, with its joint matrices where
        // it is skinned too; the file's targets are not even parsed for a mesh without one, so a scene on which attach_morphs
        // was never called is posed as before
        SrMeshMorphInfo mi;
        if ((rc = sr_scene_mesh_morph_info(r->slot[0].scene, ls->keys[b], &mi)) != SR_OK) return rc;
        int32_t skin = -1; uint32_t n_joints = 0;
        if ((rc = sr_gltf_blas_skin(g, b, &skin, nullptr, nullptr)) != SR_OK) return rc;
        if (skin < 0 && mi.n_targets == 0) continue;
        if (skin >= 0) {
            if ((rc = sr_gltf_skin(g, (uint32_t)skin, &n_joints, nullptr, nullptr)) != SR_OK) return rc;
            joints.resize(n_joints);
            if ((rc = sr_gltf_pose(g, animation, time_seconds, nullptr, (uint32_t)skin, joints.data())) != SR_OK) return rc;
        }
        if (batch) {
            item_joints.emplace_back(skin >= 0 ? joints : std::vector<SrTransform>());
            item_weights.emplace_back(mi.n_targets);
            if (mi.n_targets && (rc = sr_gltf_morph_weights(g, animation, time_seconds, b, item_weights.back().data(), mi.n_targets)) != SR_OK) return rc;
            items.push_back(SrPoseItem{ls->keys[b], nullptr, nullptr, mi.n_targets, n_joints});      // the pointers once the vectors stand still
            continue;
        }
        if (mi.n_targets == 0) {
            if ((rc = sr_renderer_skin_mesh(r, ls->keys[b], joints.data(), n_joints, stream)) != SR_OK) return rc;
            continue;
        }
        weights.resize(mi.n_targets);
        if ((rc = sr_gltf_morph_weights(g, animation, time_seconds, b, weights.data(), mi.n_targets)) != SR_OK) return rc;
        if ((rc = sr_renderer_pose_mesh(r, ls->keys[b], weights.data(), mi.n_targets, skin >= 0 ? joints.data() : nullptr, n_joints, stream)) != SR_OK) return rc;
    }
    for (size_t k = 0; k < items.size(); k++) {
        items[k].weights = items[k].n_targets ? item_weights[k].data() : nullptr;
        items[k].joint_matrices = items[k].n_joints ? item_joints[k].data() : nullptr;
    }
    if (!items.empty() && (rc = sr_renderer_pose_meshes(r, items.data(), (uint32_t)items.size(), stream)) != SR_OK) return rc;
    if (instance_transforms_out) {              // grouped by blas, the order of the file kept within a group (sr_renderer_load_scene)
        size_t o = 0;
        for (uint32_t b = 0; b < n_blases; b++)
            for (uint32_t i = 0; i < n_instances; i++) {
                uint32_t bi = 0;
                if ((rc = sr_gltf_instance(g, i, &bi, nullptr)) != SR_OK) return rc;
                if (bi == b) instance_transforms_out[o++] = posed[i];
            }
    }
    return SR_OK;
}

// BuildType of a mesh's tree on every replica (the replicas hold the same meshes: one that refuses, refuses first).
int sr_renderer_set_mesh_build_type(SrRenderer* r, uint64_t key, uint32_t build_type) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_mesh_build_type: renderer is null");
    return each_scene(r, [&](SrScene* sc) { return sr_scene_set_mesh_build_type(sc, key, build_type); });
}

// Where updatable meshes' trees are built (SR_MESH_TREE_BUILD_*), on every replica.
int sr_renderer_set_mesh_tree_build(SrRenderer* r, uint32_t mode) {
    if (mode > SR_MESH_TREE_BUILD_DEVICE) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_mesh_tree_build: mode must be SR_MESH_TREE_BUILD_AUTO, _HOST or _DEVICE");
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_mesh_tree_build: renderer is null");
    return each_scene(r, [&](SrScene* sc) { return sr_scene_set_mesh_tree_build(sc, mode); });
}

// Whether small pending meshes are built by one batched launch (SR_BLAS_BATCH_*), on every replica.
int sr_renderer_set_mesh_tree_batch(SrRenderer* r, uint32_t mode) {
    if (mode > SR_BLAS_BATCH_ON) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_mesh_tree_batch: mode must be SR_BLAS_BATCH_OFF or SR_BLAS_BATCH_ON");
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_mesh_tree_batch: renderer is null");
    return each_scene(r, [&](SrScene* sc) { return sr_scene_set_mesh_tree_batch(sc, mode); });
}

// What a device fast build does with a tree taller than its stack cap (SR_HEIGHT_BOUND_*), on every replica.
int sr_renderer_set_tree_height_bound(SrRenderer* r, uint32_t mode, uint32_t mesh_tree_cap) {
    if (mode > SR_HEIGHT_BOUND_REBALANCE || mesh_tree_cap > 26u || (mesh_tree_cap != 0 && mode == SR_HEIGHT_BOUND_REFUSE))
        return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_tree_height_bound: mode must be SR_HEIGHT_BOUND_REFUSE or _REBALANCE, mesh_tree_cap 0 or, under _REBALANCE, 1..26");
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_tree_height_bound: renderer is null");
    return each_scene(r, [&](SrScene* sc) { return sr_scene_set_tree_height_bound(sc, mode, mesh_tree_cap); });
}

// Where the light table is built (SR_LIGHTS_*), on every replica; the figures of one replica's last sr_scene_set_instances.
int sr_renderer_set_light_table_build(SrRenderer* r, uint32_t mode) {
    if (mode > SR_LIGHTS_DEVICE) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_light_table_build: mode must be SR_LIGHTS_HOST or SR_LIGHTS_DEVICE");
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_light_table_build: renderer is null");
    return each_scene(r, [&](SrScene* sc) { return sr_scene_set_light_table_build(sc, mode); });
}
int sr_renderer_light_table_info(SrRenderer* r, uint32_t slot, SrLightTableInfo* out) {
    if (!r || !out) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_light_table_info: null argument");
    if (slot >= r->slot.size()) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_light_table_info: no such slot");
    return sr_scene_light_table_info(r->slot[slot].scene, out);
}

// Access for harnesses: the scene (counters, stats), the device output image and the frame counter.
int sr_renderer_get(SrRenderer* r, SrScene** scene, const uint32_t** output_rgba8_device, const float** raw_color_device, uint32_t* relative_frame_count) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_get: renderer is null");
    if (scene) *scene = r->slot[0].scene;
    if (output_rgba8_device) *output_rgba8_device = r->output[r->last_set];     // of the last submitted frame
    if (raw_color_device) *raw_color_device = r->slot[0].raw_color[r->last_set];
    if (relative_frame_count) *relative_frame_count = r->relative_frame_count;
    return SR_OK;
}

}  // extern "C"
