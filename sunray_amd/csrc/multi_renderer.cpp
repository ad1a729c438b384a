// Here: one frame on the renderer's device slots, the transfer plan behind it and the strip settings (renderer.cpp: lifetimes, scene changes).
//
// One frame on 1..N device slots from one SrRenderer: one process, N slots, peer copies.
//
// Every slot (renderer.h) holds a replica of the scene, full-size frame buffers, its own primary-payload hand-off and reservoir
// ping-pong, a copy of the noise texture and two streams; the renderer holds the accumulation / denoise / output images, on
// slot 0's device. A frame, enqueued from the caller's thread:
//   1. every slot: sr_strip_trace_ris over its strip + spatial halo (s_ris), then the history-reach check (strip_copy.hip)
//   2. the reservoir bands of sr_history_exchange_plan: pack on the source slot, one peer copy, unpack on the destination
//   3. every slot: sr_strip_trace_final over its strip (s_final); slots >= 1 pack their strip of raw_color, depth, normal,
//      diffuse and motion and copy it with one peer copy into a staging buffer on devices[0]
//   4. slot 0 (s_final): unpack every strip into its image set k, then temporal -> denoise -> tonemap on the whole frame: the
//      output is the one-slot output bit for bit
// A lone slot's strip is the whole frame: the plan is empty, nothing is checked, packed or copied, and what is left of the
// four steps is raytracing_ris -> raytracing_final -> post chain on that slot's two streams.
// Two frames may be in flight: see the hazard list in DESIGN.md §7 (and the comments at each wait below). The same device may
// hold several slots (rehearsal mode): the copies are then device-to-device and the waits same-device waits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "host.h"
#include "renderer.h"
#include "strip_copy.h"

namespace {

void free_ptr(void* p) { if (p) (void)hipFree(p); }

// rectangle (x0, w, y0, h) of positions [a0, a0 + n) along the axis, full extent across it
void axis_rect(const SrRenderer* r, uint32_t a0, uint32_t n, uint32_t& x0, uint32_t& w, uint32_t& y0, uint32_t& h) {
    if (r->strip_axis == SR_AXIS_COLS) { x0 = a0; w = n; y0 = 0; h = r->height; }
    else { x0 = 0; w = r->width; y0 = a0; h = n; }
}
// the rectangle of slot i's strip
int strip_rect(const SrRenderer* r, uint32_t i, uint32_t& x0, uint32_t& w, uint32_t& y0, uint32_t& h) {
    uint32_t a0, n;
    R_RC(sr_partition_span(r->part, i, 0, &a0, &n));
    axis_rect(r, a0, n, x0, w, y0, h);
    return SR_OK;
}

// the five gather planes of image set k of a slot: 16 + 2 + 4 + 4 + 4 = 30 bytes per pixel
void gather_planes(const Slot& s, int k, SrkStripPlane out[5]) {
    out[0] = {s.raw_color[k], 16}; out[1] = {s.depth[k], 2}; out[2] = {s.normal[k], 4}; out[3] = {s.diffuse[k], 4}; out[4] = {s.motion[k], 4};
}
// the two exchange planes of reservoir buffer `cur`: 48 + 48 bytes per pixel
void exchange_planes(const Slot& s, int cur, SrkStripPlane out[2]) {
    out[0] = {s.reservoirs[cur], (uint32_t)sizeof(SrReservoir)}; out[1] = {s.reservoirs_gi[cur], (uint32_t)sizeof(SrReservoirGI)};
}

// (Re)builds the gather and exchange buffers of the current partition and halo; every device is idle first. A lone slot has
// no buffers to rebuild and nothing to wait for.
int prepare_transfers(SrRenderer* r) {
    if (r->slot.size() > 1) R_RC(srr::sync_all(r));
    srr::free_transfers(r);
    const int dev0 = r->slot[0].device;
    SrkStripPlane planes[5];
    for (uint32_t i = 1; i < r->slot.size(); i++) {
        Slot& s = r->slot[i];
        uint32_t x0, w, y0, h;
        R_RC(strip_rect(r, i, x0, w, y0, h));
        if (w == 0 || h == 0) continue;
        gather_planes(s, 0, planes);
        s.gather_bytes = srk_strip_packed_bytes(planes, 5, w, h);
        for (int k = 0; k < 2; k++) {
            R_HIP(hipSetDevice(s.device));
            R_HIP(hipMalloc((void**)&s.gather_pack[k], s.gather_bytes));
            R_HIP(hipSetDevice(dev0));
            R_HIP(hipMalloc((void**)&s.gather_stage[k], s.gather_bytes));
        }
    }
    uint32_t count = 0;
    R_RC(sr_history_exchange_plan(r->part, r->motion_halo, nullptr, 0, &count));
    std::vector<SrStripTransfer> plan(count);
    if (count) R_RC(sr_history_exchange_plan(r->part, r->motion_halo, plan.data(), count, &count));
    r->xfers.resize(count);
    for (uint32_t e = 0; e < count; e++) {
        Xfer& x = r->xfers[e];
        x.t = plan[e];
        uint32_t x0, w, y0, h;
        axis_rect(r, x.t.start, x.t.size, x0, w, y0, h);
        exchange_planes(r->slot[x.t.src], 0, planes);
        x.bytes = srk_strip_packed_bytes(planes, 2, w, h);
        for (int k = 0; k < 2; k++) {
            R_HIP(hipSetDevice(r->slot[x.t.src].device));
            R_HIP(hipMalloc((void**)&x.src_buf[k], x.bytes));
            R_HIP(hipEventCreateWithFlags(&x.ev[k], hipEventDisableTiming));
            R_HIP(hipSetDevice(r->slot[x.t.dst].device));
            R_HIP(hipMalloc((void**)&x.dst_buf[k], x.bytes));
        }
    }
    r->plan_dirty = false;
    return SR_OK;
}

// What both passes of this frame take on slot `s`: the whole frame; sr_strip_trace_* cut the slot's strip out of it.
SrRtParams rt_params(const SrRenderer* r, const Slot& s, const SrMatrices& mats, int k) {
    SrRtParams p;
    memset(&p, 0, sizeof(p));
    p.scene = s.scene;
    p.raw_color = s.raw_color[k]; p.depth_img = s.depth[k]; p.normal_img = s.normal[k]; p.diffuse_img = s.diffuse[k]; p.motion_vec_img = s.motion[k];
    p.matrices = &mats;
    p.blue_noise_tex = s.blue_noise; p.blue_noise_w = s.noise_w; p.blue_noise_h = s.noise_h;
    p.reservoirs[0] = s.reservoirs[0]; p.reservoirs[1] = s.reservoirs[1];
    p.reservoirs_gi[0] = s.reservoirs_gi[0]; p.reservoirs_gi[1] = s.reservoirs_gi[1];
    p.primary_payload = s.primary[k];
    p.frame_count = r->relative_frame_count;
    p.width = r->width; p.height = r->height;
    p.config = r->config;
    return p;
}

// temporal_accumulation -> denoise_0..3 -> postprocess of image set k on slot 0's s_final, then the frame's completion event.
int post_chain(SrRenderer* r, int k) {
    const Slot& s0 = r->slot[0];
    SrPostParams q;
    memset(&q, 0, sizeof(q));
    q.raw_color = s0.raw_color[k]; q.motion_vec_img = s0.motion[k]; q.depth_img = s0.depth[k]; q.normal_img = s0.normal[k]; q.diffuse_img = s0.diffuse[k];
    q.accum[0] = r->accum[0]; q.accum[1] = r->accum[1]; q.denoise[0] = r->denoise[0]; q.denoise[1] = r->denoise[1];
    q.output_rgba8 = r->output[k];
    q.frame_count = r->relative_frame_count; q.width = r->width; q.height = r->height;
    q.exposure = 1.0f;        // EXPOSURE (lib.rs:44)
    q.denoise_passes = 4;     // DENOISE_PASSES (lib.rs:42)
    R_RC(sr_post_temporal(&q, s0.s_final));
    R_RC(sr_post_denoise(&q, s0.s_final));
    R_RC(sr_post_tonemap(&q, s0.s_final));
    R_HIP(hipEventRecord(s0.ev_done[k], s0.s_final));  // after every slot's work of this frame: wait_frame and callbacks cover it
    return SR_OK;
}

bool before_first_frame(const SrRenderer* r) { return r->relative_frame_count == 0; }

}  // namespace

namespace srr {

void free_transfers(SrRenderer* r) {
    for (Slot& s : r->slot) {
        for (int k = 0; k < 2; k++) {
            free_ptr(s.gather_pack[k]); free_ptr(s.gather_stage[k]);
            s.gather_pack[k] = s.gather_stage[k] = nullptr;
        }
        s.gather_bytes = 0;
    }
    for (Xfer& x : r->xfers)
        for (int k = 0; k < 2; k++) {
            free_ptr(x.src_buf[k]); free_ptr(x.dst_buf[k]);
            if (x.ev[k]) (void)hipEventDestroy(x.ev[k]);
        }
    r->xfers.clear();
}

// The orderings that remain between frames: RIS(f) -> final(f) -> post(f), RIS(f) -> RIS(f+1) and post(f-2) -> RIS(f).
int render_frame(SrRenderer* r, const SrMatrices& mats, int k, hipStream_t caller_stream) {
    if (r->plan_dirty) R_RC(prepare_transfers(r));
    const uint32_t n_slots = (uint32_t)r->slot.size();
    const uint32_t fc = r->relative_frame_count;
    const int cur = (int)(fc & 1u);                   // the reservoir buffer this frame's RIS pass writes
    const bool restir = r->config.enable_restir != 0;
    Slot& s0 = r->slot[0];
    R_HIP(hipSetDevice(s0.device));
    R_HIP(hipEventRecord(r->ev_in, caller_stream));  // whatever the caller enqueued on `stream` comes first, on every slot
    // 1. RIS pass of every strip (+ spatial halo), then the history-reach check over the same rectangle
    for (uint32_t i = 0; i < n_slots; i++) {
        Slot& s = r->slot[i];
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipStreamWaitEvent(s.s_ris, r->ev_in, 0));
        R_HIP(hipStreamWaitEvent(s.s_ris, s.ev_done[k], 0));       // frame f-2 no longer reads this image set (slot 0: post; others: pack)
        const SrRtParams p = rt_params(r, s, mats, k);
        R_RC(sr_strip_trace_ris(&p, r->part, i, s.s_ris));
        SrStripRects rc;
        R_RC(sr_strip_rects(r->part, i, &rc));
        if (n_slots > 1 && restir && fc > 0 && !rc.empty) {        // a lone slot holds the whole frame: no read can leave it
            uint32_t h0, hn;
            R_RC(sr_partition_span(r->part, i, SR_SPATIAL_HALO + r->motion_halo, &h0, &hn));
            R_LAUNCH(srk_launch_history_reach_check(s.motion[k], r->width, r->height, r->strip_axis, rc.ris_x0, rc.ris_w, rc.ris_y0, rc.ris_h,
                                                    h0, h0 + hn, s.overflow, s.s_ris));
        }
    }
    // 2. history exchange: pack on the source, one peer copy per plan entry ...
    SrkStripPlane planes[5];
    if (restir) {
        for (Xfer& x : r->xfers) {
            Slot& src = r->slot[x.t.src];
            Slot& dst = r->slot[x.t.dst];
            uint32_t x0, w, y0, h;
            axis_rect(r, x.t.start, x.t.size, x0, w, y0, h);
            R_HIP(hipSetDevice(src.device));
            exchange_planes(src, cur, planes);
            R_LAUNCH(srk_launch_strip_pack(planes, 2, r->width, x0, w, y0, h, x.src_buf[k], src.s_ris));
            R_HIP(hipStreamWaitEvent(src.s_ris, dst.ev_ris[k], 0));  // dst unpacked dst_buf[k] of frame f-2 (its ev_ris[k] is not re-recorded yet)
            R_HIP(hipMemcpyPeerAsync(x.dst_buf[k], dst.device, x.src_buf[k], src.device, x.bytes, src.s_ris));
            R_HIP(hipEventRecord(x.ev[k], src.s_ris));
        }
        // ... and unpack on the destination, before its ev_ris[k]: its final(f) and RIS(f+1) see the band
        for (Xfer& x : r->xfers) {
            Slot& dst = r->slot[x.t.dst];
            uint32_t x0, w, y0, h;
            axis_rect(r, x.t.start, x.t.size, x0, w, y0, h);
            R_HIP(hipSetDevice(dst.device));
            R_HIP(hipStreamWaitEvent(dst.s_ris, x.ev[k], 0));
            exchange_planes(dst, cur, planes);
            R_LAUNCH(srk_launch_strip_unpack(planes, 2, r->width, x0, w, y0, h, x.dst_buf[k], dst.s_ris));
        }
    }
    for (Slot& s : r->slot) {
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipEventRecord(s.ev_ris[k], s.s_ris));
    }
    // 3. final pass of every strip; slots >= 1 pack their strip and copy it to devices[0]
    for (uint32_t i = 0; i < n_slots; i++) {
        Slot& s = r->slot[i];
        R_HIP(hipSetDevice(s.device));
        R_HIP(hipStreamWaitEvent(s.s_final, s.ev_ris[k], 0));
        const SrRtParams p = rt_params(r, s, mats, k);
        R_RC(sr_strip_trace_final(&p, r->part, i, s.s_final));
        if (i == 0) continue;                                    // slot 0's ev_done[k] follows the post chain
        if (s.gather_bytes) {
            uint32_t x0, w, y0, h;
            R_RC(strip_rect(r, i, x0, w, y0, h));
            gather_planes(s, k, planes);
            R_LAUNCH(srk_launch_strip_pack(planes, 5, r->width, x0, w, y0, h, s.gather_pack[k], s.s_final));
            R_HIP(hipStreamWaitEvent(s.s_final, s0.ev_done[k], 0));  // slot 0 unpacked gather_stage[k] of frame f-2 (post(f-2) follows it)
            R_HIP(hipMemcpyPeerAsync(s.gather_stage[k], s0.device, s.gather_pack[k], s.device, s.gather_bytes, s.s_final));
            R_HIP(hipEventRecord(s.ev_copy[k], s.s_final));
        }
        R_HIP(hipEventRecord(s.ev_done[k], s.s_final));          // RIS(f+2) of this slot waits for the pack of frame f
    }
    // 4. slot 0: unpack every strip into image set k, then the post chain on the whole frame
    R_HIP(hipSetDevice(s0.device));
    for (uint32_t i = 1; i < n_slots; i++) {
        Slot& s = r->slot[i];
        if (!s.gather_bytes) continue;
        uint32_t x0, w, y0, h;
        R_RC(strip_rect(r, i, x0, w, y0, h));
        R_HIP(hipStreamWaitEvent(s0.s_final, s.ev_copy[k], 0));
        gather_planes(s0, k, planes);
        R_LAUNCH(srk_launch_strip_unpack(planes, 5, r->width, x0, w, y0, h, s.gather_stage[k], s0.s_final));
    }
    return post_chain(r, k);
}

}  // namespace srr

extern "C" {

int sr_renderer_set_strip_bounds(SrRenderer* r, const uint32_t* bounds) {
    if (!r || !bounds) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_strip_bounds: null argument");
    if (!before_first_frame(r)) return rfail(SR_ERR_STATE, "sr_renderer_set_strip_bounds: only before the first frame after create / resize");
    SrPartition* p = nullptr;
    R_RC(sr_partition_create(r->width, r->height, (uint32_t)r->slot.size(), r->strip_axis, bounds, &p));
    sr_partition_destroy(r->part);
    r->part = p;
    r->plan_dirty = true;
    return SR_OK;
}

int sr_renderer_set_motion_halo(SrRenderer* r, uint32_t pixels) {
    if (!r) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_set_motion_halo: renderer is null");
    if (!before_first_frame(r)) return rfail(SR_ERR_STATE, "sr_renderer_set_motion_halo: only before the first frame after create / resize");
    if (r->motion_halo != pixels) { r->motion_halo = pixels; r->plan_dirty = true; }
    return SR_OK;
}

int sr_renderer_replica_scene(SrRenderer* r, uint32_t slot, SrScene** out) {
    if (!r || !out) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_replica_scene: null argument");
    if (slot >= r->slot.size()) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_replica_scene: no such slot");
    *out = r->slot[slot].scene;
    return SR_OK;
}

int sr_renderer_read_history_overflow(SrRenderer* r, uint64_t* pixels) {
    if (!r || !pixels) return rfail(SR_ERR_INVALID_ARG, "sr_renderer_read_history_overflow: null argument");
    uint64_t total = 0;
    if (r->slot.size() > 1) {                         // a lone slot has no counter: 0, and no wait
        R_RC(srr::sync_all(r));
        for (const Slot& s : r->slot) {
            unsigned long long v = 0;
            R_HIP(hipSetDevice(s.device));
            R_HIP(hipMemcpy(&v, s.overflow, sizeof(v), hipMemcpyDeviceToHost));
            total += v;
        }
        R_HIP(hipSetDevice(r->device));
    }
    *pixels = total;
    return SR_OK;
}

}  // extern "C"
