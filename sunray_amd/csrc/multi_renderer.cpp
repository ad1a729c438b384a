// One frame on several device slots from one SrRenderer: one process, N slots, peer copies.
//
// Slot 0 is the renderer itself (renderer.cpp: its scene, frame buffers, streams, the accumulation / denoise / output images).
// Every further slot holds a replica of the scene, full-size frame buffers, its own primary-payload hand-off and reservoir
// ping-pong, a copy of the noise texture and two streams. A frame, enqueued from the caller's thread:
//   1. every slot: sr_strip_trace_ris over its strip + spatial halo (s_ris), then the history-reach check (strip_copy.hip)
//   2. the reservoir bands of sr_history_exchange_plan: pack on the source slot, one peer copy, unpack on the destination
//   3. every slot: sr_strip_trace_final over its strip (s_final); slots >= 1 pack their strip of raw_color, depth, normal,
//      diffuse and motion and copy it with one peer copy into a staging buffer on devices[0]
//   4. slot 0 (s_final): unpack every strip into its image set k, then temporal -> denoise -> tonemap on the whole frame, as
//      the single-device path does: the output is the single-device output bit for bit
// Two frames may be in flight: see the hazard list in DESIGN.md §7 (and the comments at each wait below). The same device may
// hold several slots (rehearsal mode): the copies are then device-to-device and the waits same-device waits.
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "host.h"
#include "renderer.h"
#include "strip_copy.h"

namespace {

struct Slot {
    int device = 0;
    SrScene* scene = nullptr;
    float* raw_color[2] = {nullptr, nullptr};
    uint16_t* depth[2] = {nullptr, nullptr};
    uint32_t *normal[2] = {nullptr, nullptr}, *diffuse[2] = {nullptr, nullptr}, *motion[2] = {nullptr, nullptr};
    SrReservoir* reservoirs[2] = {nullptr, nullptr};
    SrReservoirGI* reservoirs_gi[2] = {nullptr, nullptr};
    SrRayPayload* primary[2] = {nullptr, nullptr};
    uint8_t* blue_noise = nullptr;
    uint32_t noise_w = 128, noise_h = 128;
    hipStream_t s_ris = nullptr, s_final = nullptr;
    hipEvent_t ev_ris[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    // owned by the multi state for every slot (slot 0 included)
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

}  // namespace

struct SrMulti {
    std::vector<Slot> slot;            // slot[0] aliases the renderer's own buffers and streams (refreshed before every frame)
    uint32_t axis = SR_AXIS_COLS;
    uint32_t motion_halo = 32;
    SrPartition* part = nullptr;
    std::vector<Xfer> xfers;
    bool plan_dirty = true;            // partition or halo changed: gather / exchange buffers are rebuilt before the next frame
};

namespace {

int mfail(int code, const std::string& msg) { return srh::set_error(code, msg); }
#define M_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mfail(e_ == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
#define M_RC(expr) do { int rc_ = (expr); if (rc_ != SR_OK) return rc_; } while (0)
#define M_LAUNCH(expr) do { int e_ = (expr); if (e_ != 0) return mfail(SR_ERR_HIP, std::string(#expr) + ": " + (e_ < 0 ? "bad arguments" : hipGetErrorString((hipError_t)e_))); } while (0)

template <typename T>
int alloc_zero(T** p, size_t n) {
    M_HIP(hipMalloc((void**)p, n * sizeof(T)));
    M_HIP(hipMemset(*p, 0, n * sizeof(T)));
    return SR_OK;
}

void free_ptr(void* p) { if (p) (void)hipFree(p); }

// frame buffers of a replica (slot >= 1): what the two passes write and read; post-chain images stay with slot 0
void free_replica_images(Slot& s) {
    for (int k = 0; k < 2; k++) {
        for (void* p : {(void*)s.raw_color[k], (void*)s.depth[k], (void*)s.normal[k], (void*)s.diffuse[k], (void*)s.motion[k],
                        (void*)s.reservoirs[k], (void*)s.reservoirs_gi[k], (void*)s.primary[k]}) free_ptr(p);
        s.raw_color[k] = nullptr; s.depth[k] = nullptr; s.normal[k] = s.diffuse[k] = s.motion[k] = nullptr;
        s.reservoirs[k] = nullptr; s.reservoirs_gi[k] = nullptr; s.primary[k] = nullptr;
    }
}

int alloc_replica_images(Slot& s, uint32_t w, uint32_t h, bool primary) {
    const size_t n = (size_t)w * h;
    M_HIP(hipSetDevice(s.device));
    for (int k = 0; k < 2; k++) {
        M_RC(alloc_zero(&s.raw_color[k], n * 4)); M_RC(alloc_zero(&s.depth[k], n)); M_RC(alloc_zero(&s.normal[k], n));
        M_RC(alloc_zero(&s.diffuse[k], n)); M_RC(alloc_zero(&s.motion[k], n));
        M_RC(alloc_zero(&s.reservoirs[k], n)); M_RC(alloc_zero(&s.reservoirs_gi[k], n));
        if (primary) M_RC(alloc_zero(&s.primary[k], n));
    }
    return SR_OK;
}

void refresh_slot0(SrRenderer* r) {
    Slot& s = r->multi->slot[0];
    s.device = r->device; s.scene = r->scene;
    for (int k = 0; k < 2; k++) {
        s.raw_color[k] = r->raw_color[k]; s.depth[k] = r->depth[k]; s.normal[k] = r->normal[k]; s.diffuse[k] = r->diffuse[k];
        s.motion[k] = r->motion[k]; s.reservoirs[k] = r->reservoirs[k]; s.reservoirs_gi[k] = r->reservoirs_gi[k];
        s.primary[k] = r->primary[k]; s.ev_ris[k] = r->ev_ris[k]; s.ev_done[k] = r->ev_done[k];
    }
    s.blue_noise = r->blue_noise; s.noise_w = r->noise_w; s.noise_h = r->noise_h;
    s.s_ris = r->s_ris; s.s_final = r->s_final;
}

int sync_all(SrMulti* m) {
    for (const Slot& s : m->slot) {
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipDeviceSynchronize());
    }
    return SR_OK;
}

// rectangle (x0, w, y0, h) of positions [a0, a0 + n) along the axis, full extent across it
void axis_rect(const SrRenderer* r, uint32_t axis, uint32_t a0, uint32_t n, uint32_t& x0, uint32_t& w, uint32_t& y0, uint32_t& h) {
    if (axis == SR_AXIS_COLS) { x0 = a0; w = n; y0 = 0; h = r->height; }
    else { x0 = 0; w = r->width; y0 = a0; h = n; }
}

// the five gather planes of image set k of a slot: 16 + 2 + 4 + 4 + 4 = 30 bytes per pixel
void gather_planes(const Slot& s, int k, SrkStripPlane out[5]) {
    out[0] = {s.raw_color[k], 16}; out[1] = {s.depth[k], 2}; out[2] = {s.normal[k], 4}; out[3] = {s.diffuse[k], 4}; out[4] = {s.motion[k], 4};
}
// the two exchange planes of reservoir buffer `cur`: 48 + 48 bytes per pixel
void exchange_planes(const Slot& s, int cur, SrkStripPlane out[2]) {
    out[0] = {s.reservoirs[cur], (uint32_t)sizeof(SrReservoir)}; out[1] = {s.reservoirs_gi[cur], (uint32_t)sizeof(SrReservoirGI)};
}

void free_transfers(SrMulti* m) {
    for (Slot& s : m->slot) {
        for (int k = 0; k < 2; k++) {
            free_ptr(s.gather_pack[k]); free_ptr(s.gather_stage[k]);
            s.gather_pack[k] = s.gather_stage[k] = nullptr;
        }
        s.gather_bytes = 0;
    }
    for (Xfer& x : m->xfers)
        for (int k = 0; k < 2; k++) {
            free_ptr(x.src_buf[k]); free_ptr(x.dst_buf[k]);
            if (x.ev[k]) (void)hipEventDestroy(x.ev[k]);
        }
    m->xfers.clear();
}

// (Re)builds the gather and exchange buffers of the current partition and halo; every device is idle first.
int prepare_transfers(SrRenderer* r) {
    SrMulti* m = r->multi;
    M_RC(sync_all(m));
    free_transfers(m);
    const int dev0 = m->slot[0].device;
    SrkStripPlane planes[5];
    for (uint32_t i = 1; i < m->slot.size(); i++) {
        Slot& s = m->slot[i];
        uint32_t a0, n, x0, w, y0, h;
        M_RC(sr_partition_span(m->part, i, 0, &a0, &n));
        if (n == 0) continue;
        axis_rect(r, m->axis, a0, n, x0, w, y0, h);
        gather_planes(s, 0, planes);
        s.gather_bytes = srk_strip_packed_bytes(planes, 5, w, h);
        for (int k = 0; k < 2; k++) {
            M_HIP(hipSetDevice(s.device));
            M_HIP(hipMalloc((void**)&s.gather_pack[k], s.gather_bytes));
            M_HIP(hipSetDevice(dev0));
            M_HIP(hipMalloc((void**)&s.gather_stage[k], s.gather_bytes));
        }
    }
    uint32_t count = 0;
    M_RC(sr_history_exchange_plan(m->part, m->motion_halo, nullptr, 0, &count));
    std::vector<SrStripTransfer> plan(count);
    if (count) M_RC(sr_history_exchange_plan(m->part, m->motion_halo, plan.data(), count, &count));
    m->xfers.resize(count);
    for (uint32_t e = 0; e < count; e++) {
        Xfer& x = m->xfers[e];
        x.t = plan[e];
        uint32_t x0, w, y0, h;
        axis_rect(r, m->axis, x.t.start, x.t.size, x0, w, y0, h);
        exchange_planes(m->slot[x.t.src], 0, planes);
        x.bytes = srk_strip_packed_bytes(planes, 2, w, h);
        for (int k = 0; k < 2; k++) {
            M_HIP(hipSetDevice(m->slot[x.t.src].device));
            M_HIP(hipMalloc((void**)&x.src_buf[k], x.bytes));
            M_HIP(hipEventCreateWithFlags(&x.ev[k], hipEventDisableTiming));
            M_HIP(hipSetDevice(m->slot[x.t.dst].device));
            M_HIP(hipMalloc((void**)&x.dst_buf[k], x.bytes));
        }
    }
    m->plan_dirty = false;
    return SR_OK;
}

int reset_overflow(SrMulti* m) {
    for (Slot& s : m->slot) {
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipMemset(s.overflow, 0, sizeof(unsigned long long)));
    }
    return SR_OK;
}

// Peer access between every pair of distinct devices the slots use, where the platform allows it ("already enabled" is fine).
int enable_peer_access(const std::vector<int>& devices) {
    for (int a : devices)
        for (int b : devices) {
            if (a == b) continue;
            int can = 0;
            M_HIP(hipDeviceCanAccessPeer(&can, a, b));
            if (!can) continue;
            M_HIP(hipSetDevice(a));
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
            else if (e != hipSuccess) return mfail(SR_ERR_HIP, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
        }
    return SR_OK;
}

int create_replica(SrRenderer* r, Slot& s) {
    M_HIP(hipSetDevice(s.device));
    M_RC(sr_scene_create(s.device, &s.scene));
    M_RC(alloc_replica_images(s, r->width, r->height, r->primary_reuse != 0));
    std::vector<uint8_t> noise((size_t)r->noise_w * r->noise_h * 4);
    M_HIP(hipSetDevice(r->device));
    M_HIP(hipMemcpy(noise.data(), r->blue_noise, noise.size(), hipMemcpyDeviceToHost));
    M_HIP(hipSetDevice(s.device));
    M_HIP(hipMalloc((void**)&s.blue_noise, noise.size()));
    M_HIP(hipMemcpy(s.blue_noise, noise.data(), noise.size(), hipMemcpyHostToDevice));
    s.noise_w = r->noise_w; s.noise_h = r->noise_h;
    M_HIP(hipStreamCreateWithFlags(&s.s_ris, hipStreamNonBlocking));
    M_HIP(hipStreamCreateWithFlags(&s.s_final, hipStreamNonBlocking));
    for (int k = 0; k < 2; k++) {
        M_HIP(hipEventCreateWithFlags(&s.ev_ris[k], hipEventDisableTiming));
        M_HIP(hipEventCreateWithFlags(&s.ev_done[k], hipEventDisableTiming));
    }
    return SR_OK;
}

bool before_first_frame(const SrRenderer* r) { return r->relative_frame_count == 0; }

}  // namespace

namespace srmr {

std::vector<SrScene*> scenes(const SrRenderer* r) {
    std::vector<SrScene*> out{r->scene};
    if (r->multi)
        for (size_t i = 1; i < r->multi->slot.size(); i++) out.push_back(r->multi->slot[i].scene);
    return out;
}

int check_same_slots(const std::vector<uint32_t>& slots, const char* what) {
    for (uint32_t s : slots)
        if (s != slots[0]) return mfail(SR_ERR_STATE, std::string(what) + " slots differ between the replicas");
    return SR_OK;
}

int synchronize(SrRenderer* r) { return r->multi ? sync_all(r->multi) : SR_OK; }

void destroy(SrRenderer* r) {
    SrMulti* m = r->multi;
    if (!m) return;
    for (const Slot& s : m->slot)
        if (hipSetDevice(s.device) == hipSuccess) (void)hipDeviceSynchronize();
    free_transfers(m);
    for (size_t i = 0; i < m->slot.size(); i++) {
        Slot& s = m->slot[i];
        (void)hipSetDevice(s.device);
        free_ptr(s.overflow);
        for (int k = 0; k < 2; k++) if (s.ev_copy[k]) (void)hipEventDestroy(s.ev_copy[k]);
        if (i == 0) continue;                         // slot 0's buffers, streams and events are the renderer's
        free_replica_images(s);
        free_ptr(s.blue_noise);
        for (int k = 0; k < 2; k++) {
            if (s.ev_ris[k]) (void)hipEventDestroy(s.ev_ris[k]);
            if (s.ev_done[k]) (void)hipEventDestroy(s.ev_done[k]);
        }
        if (s.s_ris) (void)hipStreamDestroy(s.s_ris);
        if (s.s_final) (void)hipStreamDestroy(s.s_final);
        if (s.scene) sr_scene_destroy(s.scene);
    }
    sr_partition_destroy(m->part);
    delete m;
    r->multi = nullptr;
    (void)hipSetDevice(r->device);
}

// slot 0 has been reallocated at the new extent by the caller; the replicas follow, with an equal cut
int resize(SrRenderer* r, uint32_t width, uint32_t height) {
    SrMulti* m = r->multi;
    M_RC(sync_all(m));
    free_transfers(m);
    for (size_t i = 1; i < m->slot.size(); i++) {
        free_replica_images(m->slot[i]);
        M_RC(alloc_replica_images(m->slot[i], width, height, r->primary_reuse != 0));
    }
    SrPartition* p = nullptr;
    M_RC(sr_partition_create(width, height, (uint32_t)m->slot.size(), m->axis, nullptr, &p));
    sr_partition_destroy(m->part);
    m->part = p;
    m->plan_dirty = true;
    M_RC(reset_overflow(m));
    M_HIP(hipSetDevice(r->device));
    return SR_OK;
}

int set_blue_noise(SrRenderer* r, const uint8_t* rgba8, uint32_t w, uint32_t h) {
    SrMulti* m = r->multi;
    const size_t bytes = (size_t)w * h * 4;
    for (size_t i = 1; i < m->slot.size(); i++) {
        Slot& s = m->slot[i];
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipDeviceSynchronize());
        uint8_t* fresh = nullptr;
        M_HIP(hipMalloc((void**)&fresh, bytes));
        if (hipMemcpy(fresh, rgba8, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(fresh); return mfail(SR_ERR_HIP, "sr_renderer_set_blue_noise: upload failed"); }
        free_ptr(s.blue_noise);
        s.blue_noise = fresh; s.noise_w = w; s.noise_h = h;
    }
    M_HIP(hipSetDevice(r->device));
    return SR_OK;
}

int render_frame(SrRenderer* r, const SrMatrices& mats, int k, hipStream_t caller_stream) {
    SrMulti* m = r->multi;
    refresh_slot0(r);
    if (m->plan_dirty) M_RC(prepare_transfers(r));
    const uint32_t n_slots = (uint32_t)m->slot.size();
    const uint32_t fc = r->relative_frame_count;
    const int cur = (int)(fc & 1u);                   // the reservoir buffer this frame's RIS pass writes
    const bool restir = r->config.enable_restir != 0;
    Slot& s0 = m->slot[0];
    M_HIP(hipSetDevice(s0.device));
    M_HIP(hipEventRecord(r->ev_in, caller_stream));  // whatever the caller enqueued on `stream` comes first, on every slot
    auto params = [&](const Slot& s) {
        SrRtParams p;
        memset(&p, 0, sizeof(p));
        p.scene = s.scene;
        p.raw_color = s.raw_color[k]; p.depth_img = s.depth[k]; p.normal_img = s.normal[k]; p.diffuse_img = s.diffuse[k]; p.motion_vec_img = s.motion[k];
        p.matrices = &mats;
        p.blue_noise_tex = s.blue_noise; p.blue_noise_w = s.noise_w; p.blue_noise_h = s.noise_h;
        p.reservoirs[0] = s.reservoirs[0]; p.reservoirs[1] = s.reservoirs[1];
        p.reservoirs_gi[0] = s.reservoirs_gi[0]; p.reservoirs_gi[1] = s.reservoirs_gi[1];
        p.primary_payload = s.primary[k];
        p.frame_count = fc;
        p.width = r->width; p.height = r->height;
        p.config = r->config;
        return p;
    };
    // 1. RIS pass of every strip (+ spatial halo), then the history-reach check over the same rectangle
    for (uint32_t i = 0; i < n_slots; i++) {
        Slot& s = m->slot[i];
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipStreamWaitEvent(s.s_ris, r->ev_in, 0));
        M_HIP(hipStreamWaitEvent(s.s_ris, s.ev_done[k], 0));       // frame f-2 no longer reads this image set (slot 0: post; others: pack)
        const SrRtParams p = params(s);
        M_RC(sr_strip_trace_ris(&p, m->part, i, s.s_ris));
        SrStripRects rc;
        M_RC(sr_strip_rects(m->part, i, &rc));
        if (restir && fc > 0 && !rc.empty) {
            uint32_t h0, hn;
            M_RC(sr_partition_span(m->part, i, SR_SPATIAL_HALO + m->motion_halo, &h0, &hn));
            M_LAUNCH(srk_launch_history_reach_check(s.motion[k], r->width, r->height, m->axis, rc.ris_x0, rc.ris_w, rc.ris_y0, rc.ris_h,
                                                    h0, h0 + hn, s.overflow, s.s_ris));
        }
    }
    // 2. history exchange: pack on the source, one peer copy per plan entry ...
    SrkStripPlane planes[5];
    if (restir) {
        for (Xfer& x : m->xfers) {
            Slot& src = m->slot[x.t.src];
            Slot& dst = m->slot[x.t.dst];
            uint32_t x0, w, y0, h;
            axis_rect(r, m->axis, x.t.start, x.t.size, x0, w, y0, h);
            M_HIP(hipSetDevice(src.device));
            exchange_planes(src, cur, planes);
            M_LAUNCH(srk_launch_strip_pack(planes, 2, r->width, x0, w, y0, h, x.src_buf[k], src.s_ris));
            M_HIP(hipStreamWaitEvent(src.s_ris, dst.ev_ris[k], 0));  // dst unpacked dst_buf[k] of frame f-2 (its ev_ris[k] is not re-recorded yet)
            M_HIP(hipMemcpyPeerAsync(x.dst_buf[k], dst.device, x.src_buf[k], src.device, x.bytes, src.s_ris));
            M_HIP(hipEventRecord(x.ev[k], src.s_ris));
        }
        // ... and unpack on the destination, before its ev_ris[k]: its final(f) and RIS(f+1) see the band
        for (Xfer& x : m->xfers) {
            Slot& dst = m->slot[x.t.dst];
            uint32_t x0, w, y0, h;
            axis_rect(r, m->axis, x.t.start, x.t.size, x0, w, y0, h);
            M_HIP(hipSetDevice(dst.device));
            M_HIP(hipStreamWaitEvent(dst.s_ris, x.ev[k], 0));
            exchange_planes(dst, cur, planes);
            M_LAUNCH(srk_launch_strip_unpack(planes, 2, r->width, x0, w, y0, h, x.dst_buf[k], dst.s_ris));
        }
    }
    for (Slot& s : m->slot) {
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipEventRecord(s.ev_ris[k], s.s_ris));
    }
    // 3. final pass of every strip; slots >= 1 pack their strip and copy it to devices[0]
    for (uint32_t i = 0; i < n_slots; i++) {
        Slot& s = m->slot[i];
        M_HIP(hipSetDevice(s.device));
        M_HIP(hipStreamWaitEvent(s.s_final, s.ev_ris[k], 0));
        const SrRtParams p = params(s);
        M_RC(sr_strip_trace_final(&p, m->part, i, s.s_final));
        if (i == 0) continue;
        if (s.gather_bytes) {
            uint32_t a0, n, x0, w, y0, h;
            M_RC(sr_partition_span(m->part, i, 0, &a0, &n));
            axis_rect(r, m->axis, a0, n, x0, w, y0, h);
            gather_planes(s, k, planes);
            M_LAUNCH(srk_launch_strip_pack(planes, 5, r->width, x0, w, y0, h, s.gather_pack[k], s.s_final));
            M_HIP(hipStreamWaitEvent(s.s_final, s0.ev_done[k], 0));  // slot 0 unpacked gather_stage[k] of frame f-2 (post(f-2) follows it)
            M_HIP(hipMemcpyPeerAsync(s.gather_stage[k], s0.device, s.gather_pack[k], s.device, s.gather_bytes, s.s_final));
            M_HIP(hipEventRecord(s.ev_copy[k], s.s_final));
        }
        M_HIP(hipEventRecord(s.ev_done[k], s.s_final));          // RIS(f+2) of this slot waits for the pack of frame f
    }
    // 4. slot 0: unpack every strip into image set k, then the post chain on the whole frame
    M_HIP(hipSetDevice(s0.device));
    for (uint32_t i = 1; i < n_slots; i++) {
        Slot& s = m->slot[i];
        if (!s.gather_bytes) continue;
        uint32_t a0, n, x0, w, y0, h;
        M_RC(sr_partition_span(m->part, i, 0, &a0, &n));
        axis_rect(r, m->axis, a0, n, x0, w, y0, h);
        M_HIP(hipStreamWaitEvent(s0.s_final, s.ev_copy[k], 0));
        gather_planes(s0, k, planes);
        M_LAUNCH(srk_launch_strip_unpack(planes, 5, r->width, x0, w, y0, h, s.gather_stage[k], s0.s_final));
    }
    SrPostParams q;                                   // as sr_renderer_render's single-device path
    memset(&q, 0, sizeof(q));
    q.raw_color = r->raw_color[k]; q.motion_vec_img = r->motion[k]; q.depth_img = r->depth[k]; q.normal_img = r->normal[k]; q.diffuse_img = r->diffuse[k];
    q.accum[0] = r->accum[0]; q.accum[1] = r->accum[1]; q.denoise[0] = r->denoise[0]; q.denoise[1] = r->denoise[1];
    q.output_rgba8 = r->output[k];
    q.frame_count = fc; q.width = r->width; q.height = r->height;
    q.exposure = 1.0f;
    q.denoise_passes = 4;
    M_RC(sr_post_temporal(&q, s0.s_final));
    M_RC(sr_post_denoise(&q, s0.s_final));
    M_RC(sr_post_tonemap(&q, s0.s_final));
    M_HIP(hipEventRecord(r->ev_done[k], s0.s_final));  // after every slot's work of this frame: wait_frame and callbacks cover it
    return SR_OK;
}

}  // namespace srmr

extern "C" {

int sr_renderer_create_multi(const int* devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t axis, SrRenderer** out) {
    if (!devices || !out || n_devices == 0 || width == 0 || height == 0)
        return mfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: null argument, no devices or empty extent");
    if (axis != SR_AXIS_COLS && axis != SR_AXIS_ROWS) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: axis must be SR_AXIS_COLS or SR_AXIS_ROWS");
    for (uint32_t i = 0; i < n_devices; i++)
        if (devices[i] < 0) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_create_multi: negative device index");
    SrRenderer* r = nullptr;
    int rc = sr_renderer_create(devices[0], width, height, &r);
    if (rc != SR_OK) return rc;
    r->strip_axis = axis;
    if (n_devices == 1) { *out = r; return SR_OK; }
    SrMulti* m = new SrMulti();
    r->multi = m;
    m->axis = axis;
    m->slot.resize(n_devices);
    for (uint32_t i = 0; i < n_devices; i++) m->slot[i].device = devices[i];
    refresh_slot0(r);
    std::vector<int> devs(devices, devices + n_devices);
    if ((rc = enable_peer_access(devs)) == SR_OK)
        for (uint32_t i = 1; i < n_devices && rc == SR_OK; i++) rc = create_replica(r, m->slot[i]);
    for (uint32_t i = 0; i < n_devices && rc == SR_OK; i++) {
        Slot& s = m->slot[i];
        if (hipSetDevice(s.device) != hipSuccess || hipMalloc((void**)&s.overflow, sizeof(unsigned long long)) != hipSuccess ||
            hipEventCreateWithFlags(&s.ev_copy[0], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s.ev_copy[1], hipEventDisableTiming) != hipSuccess)
            rc = mfail(SR_ERR_HIP, "sr_renderer_create_multi: per-slot counters / events");
    }
    if (rc == SR_OK) rc = reset_overflow(m);
    if (rc == SR_OK) rc = sr_partition_create(width, height, n_devices, axis, nullptr, &m->part);
    if (rc == SR_OK && hipSetDevice(r->device) != hipSuccess) rc = mfail(SR_ERR_HIP, "sr_renderer_create_multi: hipSetDevice");
    if (rc != SR_OK) {
        const std::string msg = sr_last_error();
        sr_renderer_destroy(r);
        return mfail(rc, msg);
    }
    *out = r;
    return SR_OK;
}

int sr_renderer_set_strip_bounds(SrRenderer* r, const uint32_t* bounds) {
    if (!r || !bounds) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_set_strip_bounds: null argument");
    if (!before_first_frame(r)) return mfail(SR_ERR_STATE, "sr_renderer_set_strip_bounds: only before the first frame after create / resize");
    const uint32_t n = r->multi ? (uint32_t)r->multi->slot.size() : 1u;
    SrPartition* p = nullptr;
    int rc = sr_partition_create(r->width, r->height, n, r->strip_axis, bounds, &p);
    if (rc != SR_OK) return rc;
    if (!r->multi) { sr_partition_destroy(p); return SR_OK; }
    sr_partition_destroy(r->multi->part);
    r->multi->part = p;
    r->multi->plan_dirty = true;
    return SR_OK;
}

int sr_renderer_set_motion_halo(SrRenderer* r, uint32_t pixels) {
    if (!r) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_set_motion_halo: renderer is null");
    if (!before_first_frame(r)) return mfail(SR_ERR_STATE, "sr_renderer_set_motion_halo: only before the first frame after create / resize");
    if (r->multi && r->multi->motion_halo != pixels) { r->multi->motion_halo = pixels; r->multi->plan_dirty = true; }
    return SR_OK;
}

int sr_renderer_replica_scene(SrRenderer* r, uint32_t slot, SrScene** out) {
    if (!r || !out) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_replica_scene: null argument");
    const std::vector<SrScene*> scs = srmr::scenes(r);
    if (slot >= scs.size()) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_replica_scene: no such slot");
    *out = scs[slot];
    return SR_OK;
}

int sr_renderer_read_history_overflow(SrRenderer* r, uint64_t* pixels) {
    if (!r || !pixels) return mfail(SR_ERR_INVALID_ARG, "sr_renderer_read_history_overflow: null argument");
    uint64_t total = 0;
    if (r->multi) {
        M_RC(sync_all(r->multi));
        for (const Slot& s : r->multi->slot) {
            unsigned long long v = 0;
            M_HIP(hipSetDevice(s.device));
            M_HIP(hipMemcpy(&v, s.overflow, sizeof(v), hipMemcpyDeviceToHost));
            total += v;
        }
        M_HIP(hipSetDevice(r->device));
    }
    *pixels = total;
    return SR_OK;
}

}  // extern "C"
