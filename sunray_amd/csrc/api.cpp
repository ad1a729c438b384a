// C ABI of the MI355X ray-tracing hot path (include/sunray_hip.h). Each entry point cites the
// reference interface it replaces in the header; this file is the thin host layer between that ABI,
// the host-side data preparation (host_prep.cpp, bvh_build.cpp) and the HIP kernels (kernels.hip).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <cmath>
#include <limits>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <chrono>
#include <vector>

#include "host.h"
#include "blas_batch.h"
#include "bvh_device.h"
#include "bvh_gpu.h"
#include "bvh_layout.h"
#include "kernels.h"
#include "instances.h"
#include "lights.h"
#include "normals.h"
#include "pose_batch.h"
#include "clip.h"
#include "clip_pose.h"
#include "clip_weights.h"
#include "clip_blend.h"
#include "clip_layers.h"
#include "clip_spline_weights.h"
#include "clip_layer_weights.h"
#include "tl_record.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
}  // namespace
namespace srh {
int set_error(int code, const std::string& msg) { return fail(code, msg); }   // shared with renderer.cpp
}
namespace {
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP,                            \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                             \
    } while (0)

// what the calls that read the structure answer between sr_scene_update_mesh and the sr_scene_set_instances that applies it
const char* const kStaleGeometry = "a mesh of the built structure was updated: sr_scene_set_instances must follow sr_scene_update_mesh before this call";

enum PassKind { kRis = 0, kFinal = 1, kClosest = 2, kAny = 3, kNumKinds = 4 };

// Named profiler ranges around every pass, the counterpart of the debug-utils label the reference's render graph puts around
// each pass (render_graph/graph.rs:1097-1118: a named scope in a capture, a no-op otherwise): rocTX push / pop around the
// enqueue, visible in `rocprofv3 --marker-trace`. The rocTX library is looked up at first use (no link-time dependency);
// without it, or with SR_PASS_LABELS=0 in the environment, the ranges are no-ops.
struct PassLabel {
    typedef int (*PushFn)(const char*);
    typedef int (*PopFn)(void);
    static void resolve(PushFn& push, PopFn& pop) {
        static PushFn s_push = nullptr;
        static PopFn s_pop = nullptr;
        static bool tried = false;
        if (!tried) {
            tried = true;
            const char* ev = getenv("SR_PASS_LABELS");
            if (!(ev && atoi(ev) == 0)) {
                void* h = nullptr;
                for (const char* name : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"})   // rocprofv3 listens to the first
                    if ((h = dlopen(name, RTLD_LAZY | RTLD_LOCAL))) break;
                if (h) { s_push = (PushFn)dlsym(h, "roctxRangePushA"); s_pop = (PopFn)dlsym(h, "roctxRangePop"); }
                if (!s_push || !s_pop) { s_push = nullptr; s_pop = nullptr; }
            }
        }
        push = s_push; pop = s_pop;
    }
    PopFn pop = nullptr;
    explicit PassLabel(const char* name) {
        PushFn push;
        resolve(push, pop);
        if (push) push(name);
    }
    ~PassLabel() { if (pop) pop(); }
};

// One device allocation: grows on demand, frees itself, moves (TileSchedule lives in a std::vector) and cannot be copied.
struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    int reserve(size_t n) {
        if (n > bytes || p == nullptr) {
            release();
            HIP_TRY(hipMalloc(&p, n ? n : 16));
            bytes = n ? n : 16;
        }
        return SR_OK;
    }
    int upload(const void* src, size_t n) {
        const int rc = reserve(n);
        if (rc != SR_OK) return rc;
        if (n) HIP_TRY(hipMemcpy(p, src, n, hipMemcpyHostToDevice));
        return SR_OK;
    }
    // Grows to n bytes and keeps the first `keep` bytes (device-to-device); the caller has waited for whatever reads the old allocation.
    int grow_keep(size_t n, size_t keep) {
        if (p && n <= bytes) return SR_OK;
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, n ? n : 16));
        if (p && keep) {
            const hipError_t e = hipMemcpy(q, p, std::min(keep, bytes), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { (void)hipFree(q); return fail(SR_ERR_HIP, std::string("device-to-device copy of a growing buffer: ") + hipGetErrorString(e)); }
        }
        release();
        p = q; bytes = n ? n : 16;
        return SR_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// First vertex with a non-finite position / first index out of range; the count where there is none.
uint32_t first_non_finite_vertex(const SrVertex* v, uint32_t n) {
    uint32_t i = 0;
    while (i < n && std::isfinite(v[i].position[0]) && std::isfinite(v[i].position[1]) && std::isfinite(v[i].position[2])) i++;
    return i;
}
uint32_t first_index_out_of_range(const uint32_t* indices, uint32_t n_indices, uint32_t n_vertices) {
    uint32_t i = 0;
    while (i < n_indices && indices[i] < n_vertices) i++;
    return i;
}

// The 24-float textured shade record of one triangle (uv, normal-map uv, tangents), as bvh_gpu.hip write_shade_tex writes it.
void pack_shade_tex(float* q, const SrVertex* const v[3]) {
    for (int j = 0; j < 3; j++) { memcpy(q + 2 * j, v[j]->base_color_tex_coord, 8); memcpy(q + 6 + 2 * j, v[j]->normal_tex_coord, 8); }
    memcpy(q + 12, v[0]->tangent, 12);
    q[15] = v[0]->tangent[3] >= 0.0f ? 1.0f : -1.0f;   // handedness from the first vertex only (closest_hit.slang:34)
    memcpy(q + 16, v[1]->tangent, 12);
    memcpy(q + 19, v[2]->tangent, 12);
}

}  // namespace

constexpr size_t kCounterBytes = (size_t)srd::kCounterSlots * srd::kCounterStride * 8;   // the copies of the ray counters (traverse.h)

struct SrScene {
    int device = 0;
    std::vector<srh::HostMesh> meshes;
    std::map<uint64_t, uint32_t> slots;
    std::vector<SrEmissiveTriangle> emissive_tris;       // the emissive arena (resource_manager.rs:433-443)
    std::vector<SrEmissiveTriangle> emissive_table;      // what a frame sees: the arena, or one zero entry if it is empty
    std::vector<uint32_t> free_mesh_slots, free_emissive_slots;   // LIFO reuse, like the reference's arenas (buffer/arena_core.rs)
    std::vector<SrMeshInfo> mesh_infos;
    srh::FrameInstanceData fid;
    std::vector<srh::BuildTri> world_tris;
    struct DeviceImage { void* d_texels = nullptr; uint32_t w = 0, h = 0; };
    std::vector<DeviceImage> images;        // image slot order (Material::*_image); a removed image leaves d_texels == nullptr
    std::vector<uint32_t> free_image_slots; // slots of removed images, reused by the next sr_scene_add_image
    std::vector<SrSamplerDesc> samplers;    // sampler slot order (Material::*_sampler)
    DeviceBuffer d_nodes, d_tris, d_shade, d_mesh_const, d_slot_of_gid, d_instances, d_lights, d_misc;
    DeviceBuffer d_shade_tex, d_mesh_tex, d_textures;
    // two-level form (optional): one tree per mesh in object space (built once per mesh, kept on the host until the set of
    // meshes changes) + a top-level tree over the instances, rebuilt from the instance list — nothing here scales with
    // instances x triangles
    struct HostBlas {
        bool valid = false;
        std::vector<uint32_t> nodes;        // 4-wide quantised tree, references local to the mesh
        std::vector<float> tris, shade, shade_tex;   // 12 / 12 / 24 floats per triangle, leaf order
        std::vector<uint32_t> slot_of_prim;
        uint32_t n_tris = 0, n_nodes = 0, max_stack = 0, max_depth = 0;
        // The root block, eight words: root box (object space) and the padding numbers. The device build's ten-word result and a
        // srd::TlMeshRow begin with it, and the refit reads back one per mesh: it is copied as a whole in either direction.
        struct RootBlock { float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, max_abs_vertex = 0.0f, max_edge_sum = 0.0f; };
        RootBlock root;
        double build_ms = 0.0;
        bool host_stale = false;            // refitted or built on the device since: nodes / tris / shade / shade_tex above hold the old vertices
                                            // (after a refit, topology, slot_of_prim, counts, max_stack and the read-back lo, hi, max_* are current)
        bool device_built = false;          // built on the device since (implies host_stale): nodes' topology and slot_of_prim above are stale too;
                                            // n_nodes, max_stack, max_depth, lo, hi, max_* are the read-back, the levels are level_ranges
        std::vector<std::pair<uint32_t, uint32_t>> level_ranges;   // of a device-built tree: (first node, count) per level, root level first, local to the mesh
    };
    // Everything the scene keeps per mesh slot beside the mesh itself: its tree, where the tree sits in the concatenated device
    // arrays, and its maintenance (Blas::plan_op / mark_built, blas.rs:245-310): build type, heuristic state, what the last
    // sr_scene_set_instances / sr_scene_end_frame did to the tree
    struct MeshState {
        HostBlas tree;
        uint32_t node_base = 0, tri_base = 0;    // of the concatenated device arrays (upload_mesh_trees)
        int device_refused = -1;                 // >= 0: the device build refused this mesh's tree for depth under that SR_FAST_BUILD topology
                                                 // (fast_build_ploc): later fast builds go to the host without another attempt
        uint32_t node_cap = 0;                   // > 0: the mesh owns the node range [node_base, node_base + node_cap) behind the concatenation, taken
                                                 // at its first device build and kept for later ones; 0: the compact range the concatenation gave it
        uint32_t build_type = SR_BUILD_STATIC;   // Renderer::load_mesh builds Static (lib.rs:937)
        SrAsState state{0, 0, 0, 0};
        uint32_t last_op = SR_OP_NONE;
        bool refit_pending = false;         // updated (sr_scene_update_mesh) while its tree was valid: the next sr_scene_set_instances refits or rebuilds it
        bool built_once = false, rebuilt_now = false, refit_now = false;
        bool dirty = false;                 // sr_scene_update_mesh: vertices changed since the built structure, which instances it, last took them
        // sr_scene_set_mesh_skin: the bind pose (a snapshot of the mesh's vertices at the attach) and one SrSkinInfluence per vertex,
        // owned by the mesh (freed with this record: detach, sr_scene_remove, sr_scene_destroy); n_joints == 0: no skin
        struct Skin { DeviceBuffer d_bind, d_influences; uint32_t n_joints = 0, skinned = 0, first_bad = 0xFFFFFFFFu; double skin_ms = 0.0; };
        Skin skin;
        // sr_scene_set_mesh_morph: the morph base (a snapshot of the mesh's vertices at the attach) and the target-major delta records,
        // owned by the mesh like the skin's buffers; n_targets == 0: no morph
        struct Morph { DeviceBuffer d_base, d_deltas; uint32_t n_targets = 0, posed = 0, n_active = 0, first_bad = 0xFFFFFFFFu; double morph_ms = 0.0; };
        Morph morph;
        // sr_scene_set_mesh_frame: the reference records (a snapshot of the mesh's vertices at the attach), the runs (offsets, entries),
        // the sides and the per-triangle uv terms of mesh_frame.h, owned by the mesh like the skin's buffers; flags == 0: no frame
        struct Frame {
            DeviceBuffer d_reference, d_offsets, d_entries, d_side, d_tri_uv;
            uint32_t flags = 0, n_groups = 0, n_entries = 0, max_valence = 0, updates = 0, first_bad = 0xFFFFFFFFu;
            double frame_ms = 0.0;
        };
        Frame frame;
        // light table on the device (SR_LIGHTS_DEVICE). arena_stale: the newest positions of this mesh's arena slots exist only on
        // the device (its d_vertices, and the device arena once arena_pending is served); emissive_tris holds older ones.
        // arena_pending: emissive_positions_kernel has to rewrite its slots of the device arena before the next table is built.
        bool arena_stale = false, arena_pending = false;
        DeviceBuffer d_emissive_slots;      // the mesh's emissive_slots, uploaded at the first such rewrite
    };
    std::vector<MeshState> mesh_state;      // by mesh slot, one per entry of `meshes`: grows in sr_scene_add_blas only
    // The concatenated mesh trees on the device: every live mesh's tree, then the baked copies of the instance list at hand
    // (upload_mesh_trees), then the node ranges device-built meshes took (MeshState::node_cap); d_tris, d_shade, d_shade_tex and
    // d_slot_of_gid are the triangle side. blas_device_current (the arrays match the current set of meshes) is set by
    // upload_mesh_trees alone and cleared by what adds, removes or invalidates a tree; the rest is read only behind it.
    // blas_node_end covers every node range handed out (d_blas_node_box, allocated at the first refit or device build, has as many
    // rows), tl_blas_nodes the nodes really in use. While tl_mesh_rows_current, d_tl_mesh_rows (srd::TlMeshRow by mesh slot) holds
    // every tree's root block, stack need and bases: device refits and builds write their rows, upload_mesh_trees moves the bases and
    // clears it, top_level_build_device uploads them anew. Where bases move or a node list changes (a device build), `refit` is void.
    struct MeshTrees {
        DeviceBuffer d_blas_nodes, d_blas_node_box, d_tl_mesh_rows;
        uint64_t blas_node_end = 0, tl_blas_nodes = 0, tl_blas_tris = 0;
        bool blas_device_current = false, tl_mesh_rows_current = false, any_textured_tl = false, tl_baked = false;
        std::vector<uint32_t> tl_baked_node_base, tl_baked_tri_base;
        // the builder's bound on a device-built tree's nodes; a mesh's own range of that size, at its first device build; the rows a writer keeps current, or null
        static uint32_t range_bound(uint32_t n_tris) { return n_tris + 64u; }
        void take_range(MeshState& ms) { if (ms.node_cap == 0) { ms.node_base = (uint32_t)blas_node_end; ms.node_cap = range_bound(ms.tree.n_tris); blas_node_end += ms.node_cap; } }
        srd::TlMeshRow* rows_dev(size_t n_meshes) const { return (tl_mesh_rows_current && d_tl_mesh_rows.bytes >= n_meshes * sizeof(srd::TlMeshRow)) ? (srd::TlMeshRow*)d_tl_mesh_rows.p : nullptr; }
    } trees;
    // The set of meshes the device refitted last (an animation refits the same set every frame) with its rewrite-kernel rows, node
    // lists by level (global indices, deepest level first) and accumulators. An empty `set` is void.
    struct RefitSet { DeviceBuffer d_meshes, d_nodes, d_acc, d_acc_init, d_out; std::vector<uint32_t> set, level_offsets; uint32_t threads = 0; } refit;
    int blas_build_mode = SR_MESH_TREE_BUILD_AUTO;   // sr_scene_set_mesh_tree_build / SR_BLAS_BUILD in the environment
    SrMeshTreeInfo mt_info{};               // mesh-tree builds of the last sr_scene_set_instances
    bool static_mesh_updated = false;       // a Static mesh was updated since the last sr_scene_set_instances (its tree goes to the host)
    DeviceBuffer d_blas_build_out;          // read-back block of a device mesh-tree build
    uint32_t blas_batch_mode = SR_BLAS_BATCH_OFF;    // sr_scene_set_mesh_tree_batch / SR_BLAS_BATCH in the environment
    SrMeshTreeBatchInfo batch_info{};       // the batched builds of the last sr_scene_set_instances
    DeviceBuffer d_batch_rows, d_batch_results;      // rows and result rows of a batched mesh-tree build (blas_batch.hip)
    DeviceBuffer d_vertex_check;            // the check word the validation kernel and the frame kernels answer in (checked_launch)
    // the pose path (sr_scene_skin_mesh, sr_scene_pose_mesh: one item; sr_scene_pose_meshes): the staging block of the last call
    // (pose_batch_plan.h lays it out), its check words (two per item) and the scratch every item's posed records go to; the keys
    // and scratch offsets of the last accepted call (the replicas of a renderer take the records from there; empty after a
    // refused one), and the figures of the last sr_scene_pose_meshes that reached the device
    DeviceBuffer d_pose_stage, d_pose_check, d_pose_scratch;
    std::vector<uint64_t> pose_batch_keys, pose_batch_vertex_base;
    SrPoseBatchInfo pose_info{0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0.0, 0.0, 0.0};
    // clips on the device (sr_scene_attach_clip, sr_scene_pose_actors): every attached clip's host copy and its one device block,
    // by id (ids count up and are never handed out again); the figures of the last sr_scene_pose_actors that reached the device;
    // where that call left each actor's joint matrices in the staging block (while actor_stage_current: no other pose call has
    // used the block since) and, after SR_ACTORS_KEEP_NODES, its nodes in the kept-nodes buffers
    struct AttachedClip { SrClip host; DeviceBuffer d_block; };
    std::map<uint32_t, AttachedClip> clips;
    uint32_t next_clip_id = 1;
    SrActorPoseInfo actor_info{0, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0.0, 0.0, 0.0, 0.0};
    SrSplinePoseInfo spline_info{0, 0, 0, 0.0, 0};
    struct ActorRecord { uint64_t matrix_byte; uint32_t n_joints, node_base, n_nodes; };
    std::vector<ActorRecord> actor_records;
    // ... and each item's row and its slice of the active arrays (sr_scene_read_item_active); capacity: the entries of the slice
    struct ItemActiveRecord { uint64_t row_byte, index_byte, weight_byte; uint32_t capacity; };
    std::vector<ItemActiveRecord> item_active_records;
    bool actor_stage_current = false, actor_nodes_kept = false;
    DeviceBuffer d_actor_trs, d_actor_globals;
    // after a sr_scene_pose_actors_blended with SR_ACTORS_KEEP_SOURCES: both sources' sampled TRS, at the kept nodes' places
    bool actor_sources_kept = false;
    DeviceBuffer d_actor_source_a, d_actor_source_b;
    // layer stacks (sr_scene_pose_actors_layered): every attached node mask's host copy and device floats, by id (ids count up and
    // are never handed out again); the figures of the last such call that reached the device; after SR_ACTORS_KEEP_LAYERS every
    // layer's sampled records (and those at an additive layer's reference time), at layer_base + layer * n_nodes of its actor
    struct AttachedMask { std::vector<float> host; DeviceBuffer d_weights; };
    std::map<uint32_t, AttachedMask> node_masks;
    uint32_t next_mask_id = 1;
    SrLayerPoseInfo layer_info{0, 0, 0, 0, 0, 0};
    SrLayerWeightsInfo layer_weights_info{0, 0, 0, 0, 0, 0.0};      // ... with SR_ACTORS_LAYER_WEIGHTS: its clip-weighted items
    struct ActorLayerRecord { uint64_t layer_base; uint32_t n_layers, additive; };      // additive: bit l set where layer l is
    std::vector<ActorLayerRecord> actor_layer_records;
    bool actor_layers_kept = false;
    DeviceBuffer d_actor_layer_cur, d_actor_layer_ref;
    // sr_scene_update_mesh_positions*: the face vectors of the last call (one or two 16-byte pieces per triangle), the uploaded
    // positions of the host-pointer form, and the records the mesh-frame producer wrote (scratch: the replicas of a renderer take
    // them from there)
    DeviceBuffer d_frame_faces, d_frame_positions, d_frame_out;
    DeviceBuffer d_tl_inst, d_tl_instances;
    // top level built on the device (bvh_gpu.hip srk_tl_*): the instance boxes, its result block (the per-mesh rows are trees.d_tl_mesh_rows)
    DeviceBuffer d_tl_boxes, d_tl_result;
    int tl_build_mode = SR_TL_BUILD_AUTO;   // sr_scene_set_top_level_build / SR_TL_BUILD in the environment
    SrTopLevelInfo tl_info{};               // of the last top-level build
    std::vector<float> tl_boxes_host;       // the instance boxes of a host-built top level (sr_scene_read_top_level)
    int instancing = SR_INSTANCING_AUTO;    // sr_scene_set_instancing / SR_INSTANCING in the environment
    bool two_level = false;                 // form of the structure that is built right now
    // acceleration-structure maintenance (update in place): per-level node lists, exact node boxes, flatten inputs
    DeviceBuffer d_level_nodes, d_node_box, d_mesh_infos, d_flat_instances, d_scratch;
    // cost-ordered tile schedules of the two passes (kernels.hip thread_pixel), one per launch geometry
    struct TileSchedule { int which = -1; uint32_t width = 0 /* columns of the launch rectangle */, y0 = 0, y1 = 0, x0 = 0; DeviceBuffer cost, order; bool have_order = false; uint64_t last_use = 0; uint32_t uses = 0; };
    std::vector<TileSchedule> schedules;
    uint64_t schedule_clock = 0;
    int tile_scheduling = 1;                // SR_TILE_SCHEDULING=0 in the environment disables it (A/B)
    int fast_build_ploc = 16;               // device fast build: PLOC with this search radius (default), 0 = radix tree (SR_FAST_BUILD=lbvh | ploc<r>)
    uint32_t height_bound = SR_HEIGHT_BOUND_REFUSE, mesh_tree_cap = 0;   // sr_scene_set_tree_height_bound / SR_FAST_BUILD_HEIGHT in the environment
    SrTreeHeightInfo height_info[3]{};      // the last device fast build of each SR_TREE_KIND_*
    uint32_t forced_op = SR_OP_NONE;        // sr_scene_force_next_op (test / bench hook)
    bool last_build_on_device = false;
    std::vector<uint32_t> level_offsets;
    std::vector<uint32_t> shape;            // mesh slot of every instance of the built tree: an UPDATE needs the same layout
    SrAsState as_state{0, 0, 0, 0};         // SometimesChanges -> Optimal (resource_manager.rs:119-126, mod.rs:86-91)
    uint32_t last_op = SR_OP_NONE;
    srd::DevScene dev{};
    SrBvhStats stats{};
    bool built = false;
    bool built_once = false;
    bool geometry_stale = false;            // the built structure instances a dirty mesh: it shows stale geometry until the next sr_scene_set_instances
    SrMeshUpdateInfo mu_info{};
    // sr_scene_set_instances_device. keys / counts: the layout `fid` holds (the last successful call through either entry point;
    // layout_valid is cleared by what adds or removes a mesh, since a key may then name another mesh). d_layout: that layout's
    // srd::InstanceLayout records while layout_on_device. d_instances_next / d_flat_next: the set of tables the kernel writes, which
    // changes places with d_instances / d_flat_instances once the call is accepted. host_stale: the transforms of fid.transforms and
    // fid.instances[].o2w are older than d_flat_instances, which fetch_host_transforms reads back.
    struct InstanceSource {
        std::vector<uint64_t> keys;
        std::vector<uint32_t> counts;
        bool layout_valid = false, layout_on_device = false, host_stale = false;
        DeviceBuffer d_layout, d_instances_next, d_flat_next, d_replica_transforms;
        SrInstanceUpdateInfo info{0, 0, 0, SR_INST_FETCH_NONE, 0, 0, 0xFFFFFFFFu, 0, 0.0, 0.0};
    } inst;
    // Light table on the device. d_arena mirrors emissive_tris (arena_device_entries records). The invariant that keeps an older
    // host value from overwriting a newer device one: a mesh whose arena_stale is set has its newest vertices in its d_vertices,
    // so its slots of d_arena are a function of device memory alone; arena_host_dirty (anything wrote emissive_tris since the last
    // upload: add, host update) re-uploads the WHOLE arena, which also serves a reallocation, and every upload sets arena_pending
    // on every arena_stale mesh, so the kernel rewrites their slots afterwards. Host code reads the positions of an arena_stale
    // mesh from emissive_tris only behind refresh_host_arena, which clears the flag.
    int light_mode = SR_LIGHTS_HOST;        // sr_scene_set_light_table_build / SR_LIGHT_TABLE in the environment
    DeviceBuffer d_arena, d_light_entries;
    uint32_t arena_device_entries = 0;
    bool arena_host_dirty = true;
    std::vector<SrEmissiveIndirectionEntry> entries_on_device;   // what d_light_entries holds
    bool lights_on_device = false;          // the last sr_scene_set_instances chose the kernel: upload_instance_tables builds the table from d_arena
    bool emissive_table_stale = false;      // ... and emissive_table has not been read back from d_arena since (sr_scene_get_tables does)
    SrLightTableInfo lt_info{};
    int instrumented = 0;
    int timing = 0;
    int n_cus = 256;
    int stack_entries = 8;   // LDS traversal-stack entries per lane this scene's tree needs (multiple of 4)
    int light_stage = 1;     // the RIS pass may keep the light table in its waves' LDS between queries (SR_LIGHT_STAGE=0: never; A/B runs)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events[kNumKinds];
    size_t events_used[kNumKinds] = {0, 0, 0, 0};
    ~SrScene() { for (auto& pool : events) for (auto& e : pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); } }
};

namespace {

int bind_device(const SrScene* s) {
    HIP_TRY(hipSetDevice(s->device));
    return SR_OK;
}

// Record a start/stop event pair around a launch when timing is on (bench.py's roofline leg).
struct ScopedTiming {
    SrScene* s; int kind; hipStream_t stream; hipEvent_t stop = nullptr;
    ScopedTiming(SrScene* s_, int kind_, hipStream_t st) : s(s_), kind(kind_), stream(st) {
        if (!s->timing) return;
        auto& pool = s->events[kind];
        size_t& used = s->events_used[kind];
        if (used == pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
            pool.emplace_back(a, b);
        }
        (void)hipEventRecord(pool[used].first, stream);
        stop = pool[used].second;
        used++;
    }
    ~ScopedTiming() { if (stop) (void)hipEventRecord(stop, stream); }
};

// Times of two consecutive stretches of kernels on the null stream, only while sr_scene_enable_timing is on: mark() before,
// between and after them, then read() the two intervals (it waits for the last mark).
struct ThreeMarkTimer {
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int marks = 0;
    bool on = false;
    explicit ThreeMarkTimer(const SrScene* s) {
        if (s->timing) for (auto& e : ev) if (hipEventCreate(&e) != hipSuccess) e = nullptr;
        on = ev[0] && ev[1] && ev[2];
    }
    ~ThreeMarkTimer() { for (auto& e : ev) if (e) (void)hipEventDestroy(e); }
    void mark() { if (on) (void)hipEventRecord(ev[marks], nullptr); marks++; }
    void read(double* first_ms, double* second_ms) {
        float a = 0.0f, b = 0.0f;
        if (on && hipEventSynchronize(ev[2]) == hipSuccess && hipEventElapsedTime(&a, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&b, ev[1], ev[2]) == hipSuccess) { *first_ms = a; *second_ms = b; }
    }
};

// A start / stop event pair that exists only while sr_scene_enable_timing is on. begin() and end() record on the stream the timed
// work goes to; ms() is read once that stream has been waited for and is 0.0 while timing is off or where an event call failed.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    explicit EventPair(const SrScene* s) { if (s->timing && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) release(); }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    ~EventPair() { release(); }
    void release() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
    void begin(hipStream_t st) { if (b) (void)hipEventRecord(a, st); }
    void end(hipStream_t st) { if (b) (void)hipEventRecord(b, st); }
    double ms() const { float t = 0.0f; return b && hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }
};

// The slot of `key` into *slot, or the refusal in the words of the entry point `who`.
int find_mesh(const SrScene* s, uint64_t key, const char* who, uint32_t* slot) {
    const auto it = s->slots.find(key);
    if (it == s->slots.end()) return fail(SR_ERR_INVALID_ARG, std::string(who) + ": no mesh is registered under this key");
    *slot = it->second;
    return SR_OK;
}

// This mesh's tree no longer matches its vertices: the next build rebuilds it on the host (upload_mesh_trees) and
// re-concatenates the device arrays; a pending refit is dropped with it. Every caller gets all five assignments, also where
// one is a no-op there, because of what holds everywhere: refit_pending implies a valid tree of an updatable mesh; a tree that
// is not valid is rebuilt into a fresh HostBlas (host_stale = false, refit_pending = false) before anything reads it; and
// tl_mesh_rows_current is read only behind blas_device_current, which only upload_mesh_trees sets, clearing the former.
void invalidate_mesh_tree(SrScene* s, uint32_t slot) {
    SrScene::MeshState& ms = s->mesh_state[slot];
    ms.tree.valid = false; ms.tree.host_stale = false; ms.refit_pending = false;
    s->trees.blas_device_current = false; s->trees.tl_mesh_rows_current = false;
}
void invalidate_mesh_trees(SrScene* s, bool pending) {     // every mesh with a stale host copy and, with `pending`, every mesh with a pending update
    for (size_t m = 0; m < s->mesh_state.size(); m++)
        if ((pending && s->mesh_state[m].refit_pending) || s->mesh_state[m].tree.host_stale) invalidate_mesh_tree(s, (uint32_t)m);
}

// The host copy of a mesh's vertices, brought up to date where sr_scene_update_mesh_device left it behind: one device-to-host
// copy of the mesh's buffer. Everything on the host that reads HostMesh::vertices calls this first; the device paths (in-place
// update, device fast build, mesh-tree refit and device build of a mesh without emissive entries) never do.
int fetch_host_vertices(SrScene* s, uint32_t slot) {
    srh::HostMesh& m = s->meshes[slot];
    if (!m.host_stale) return SR_OK;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpy(m.vertices.data(), m.d_vertices, sizeof(SrVertex) * (size_t)m.n_vertices, hipMemcpyDeviceToHost));
    m.host_stale = false;
    m.host_fetches++;
    m.fetch_ms = ms_between(t0, std::chrono::steady_clock::now());
    return SR_OK;
}

// The host copy of the instance transforms, brought up to date where sr_scene_set_instances_device left it behind: one
// device-to-host copy out of the FlatInstance table (48 of every 64 bytes). Everything on the host that reads fid.transforms
// or an instance's o2w calls this first, with the SR_INST_FETCH_* it is; the device paths (the top-level build on the device,
// in-place update, device fast build, the device light table) never do.
int fetch_host_transforms(SrScene* s, uint32_t reason) {
    if (!s->inst.host_stale) return SR_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = s->fid.instances.size();
    HIP_TRY(hipSetDevice(s->device));
    if (n) HIP_TRY(hipMemcpy2D(s->fid.transforms.data(), sizeof(SrTransform), s->d_flat_instances.p, sizeof(srd::FlatInstance), sizeof(SrTransform), n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) s->fid.instances[i].o2w = s->fid.transforms[i];
    s->inst.host_stale = false;
    SrInstanceUpdateInfo& ii = s->inst.info;
    ii.host_stale = 0; ii.host_fetches++; ii.fetch_reason = reason;
    ii.fetch_ms = ms_between(t0, std::chrono::steady_clock::now());
    return SR_OK;
}

// What the two update calls refuse before anything else happens, with one text each: the slot of `key` into *slot.
int check_mesh_update(SrScene* s, uint64_t key, const void* vertices, uint32_t n_vertices, uint32_t* slot) {
    if (!s || !vertices) return fail(SR_ERR_INVALID_ARG, "update_mesh: null argument");
    if (const int rc = find_mesh(s, key, "update_mesh", slot); rc != SR_OK) return rc;
    const srh::HostMesh& m = s->meshes[*slot];
    if (n_vertices != m.n_vertices) {
        char buf[160];
        snprintf(buf, sizeof(buf), "update_mesh: %u vertices given, the mesh was loaded with %u (the vertex count cannot change)", n_vertices, m.n_vertices);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    return SR_OK;
}
// Whether the HIP runtime reports [p, p + bytes) as device memory of the scene's device (bound by the caller). A pointer it does not
// is never handed to a kernel.
bool device_range_of_scene(const SrScene* s, const void* p, size_t bytes) {
    hipPointerAttribute_t attr;
    memset(&attr, 0, sizeof(attr));
    void* base = nullptr;
    size_t size = 0;
    const uintptr_t a = (uintptr_t)p;
    bool ok = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == s->device;
    ok = ok && hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)p) == hipSuccess &&
         a >= (uintptr_t)base && a - (uintptr_t)base <= size && bytes <= size - (a - (uintptr_t)base);
    if (!ok) (void)hipGetLastError();                         // an address the runtime does not know leaves its error behind
    return ok;
}
int fail_non_finite_vertex(uint32_t i) {
    char buf[120];
    snprintf(buf, sizeof(buf), "update_mesh: vertex %u has a non-finite position", i);
    return fail(SR_ERR_INVALID_ARG, buf);
}
// the emissive entries are one per triangle in index order (load_mesh, the glTF path) or none; any other list came from
// the caller of sr_scene_add_blas and cannot be re-derived from vertices
int check_emissive_list(const srh::HostMesh& m) {
    if (!m.emissive_slots.empty() && m.emissive_slots.size() != m.n_indices / 3)
        return fail(SR_ERR_UNSUPPORTED, "update_mesh: the mesh was loaded with emissive triangles that are not one per triangle");
    return SR_OK;
}

// ---- light table on the device (SR_LIGHTS_DEVICE; the invariant is stated at SrScene::light_mode) ---------------------------
// The device arena brought up to date on the null stream: host-side changes first (the whole arena, which also serves a grown
// one), then the positions of every pending mesh from its device vertices. The caller has bound the device and synchronises.
int sync_device_arena(SrScene* s, uint32_t* rewritten, uint32_t* uploaded) {
    const uint32_t n = (uint32_t)s->emissive_tris.size();
    int rc;
    if (s->arena_host_dirty || s->arena_device_entries != n) {
        if ((rc = s->d_arena.upload(s->emissive_tris.data(), sizeof(SrEmissiveTriangle) * (size_t)n)) != SR_OK) return rc;
        s->arena_device_entries = n; s->arena_host_dirty = false;
        for (SrScene::MeshState& ms : s->mesh_state) if (ms.arena_stale) ms.arena_pending = true;   // the upload put older positions in their slots
        if (uploaded) *uploaded += 1;
    }
    for (size_t slot = 0; slot < s->mesh_state.size(); slot++) {
        SrScene::MeshState& ms = s->mesh_state[slot];
        if (!ms.arena_pending) continue;
        const srh::HostMesh& m = s->meshes[slot];
        const uint32_t n_tris = (uint32_t)m.emissive_slots.size();             // one per triangle in index order (check_emissive_list)
        if (!ms.d_emissive_slots.p && (rc = ms.d_emissive_slots.upload(m.emissive_slots.data(), sizeof(uint32_t) * (size_t)n_tris)) != SR_OK) return rc;
        const int e = srk_emissive_positions((const SrVertex*)m.d_vertices, m.n_vertices, (const uint32_t*)m.d_indices, (const uint32_t*)ms.d_emissive_slots.p,
                                             n_tris, (SrEmissiveTriangle*)s->d_arena.p, n, nullptr);
        if (e != 0) return fail(SR_ERR_HIP, std::string("arena position launch failed: ") + hipGetErrorString((hipError_t)e));
        ms.arena_pending = false;
        if (rewritten) *rewritten += n_tris;
    }
    return SR_OK;
}

// sr_scene_get_tables returns the arena the last sr_scene_set_instances saw: where that table was built on the device, this is
// the device arena as it stands until something writes it again, read back once (64 bytes per entry, not the vertices).
int fetch_emissive_table(SrScene* s) {
    if (!s->emissive_table_stale) return SR_OK;
    HIP_TRY(hipSetDevice(s->device));
    s->emissive_table.resize(s->arena_device_entries);
    HIP_TRY(hipMemcpy(s->emissive_table.data(), s->d_arena.p, sizeof(SrEmissiveTriangle) * (size_t)s->arena_device_entries, hipMemcpyDeviceToHost));
    s->emissive_table_stale = false;
    s->lt_info.arena_fetches++;
    return SR_OK;
}

// Before host code reads emissive_tris (the host light table, a switch to SR_LIGHTS_HOST) or a mesh's slots are freed: the
// slots of every arena_stale mesh from the device arena, brought up to date first. Nothing to do where no mesh is stale.
int refresh_host_arena(SrScene* s) {
    bool any = false;
    for (const SrScene::MeshState& ms : s->mesh_state) any = any || ms.arena_stale;
    if (!any) return SR_OK;
    int rc = fetch_emissive_table(s);                        // what the last sr_scene_set_instances saw, before the arena moves on
    if (rc != SR_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = sync_device_arena(s, nullptr, nullptr)) != SR_OK) return rc;
    std::vector<SrEmissiveTriangle> dev(s->arena_device_entries);
    HIP_TRY(hipMemcpy(dev.data(), s->d_arena.p, sizeof(SrEmissiveTriangle) * dev.size(), hipMemcpyDeviceToHost));   // null stream: behind the kernels
    s->lt_info.arena_fetches++;
    for (size_t slot = 0; slot < s->mesh_state.size(); slot++) {
        if (!s->mesh_state[slot].arena_stale) continue;
        for (uint32_t es : s->meshes[slot].emissive_slots) s->emissive_tris[es] = dev[es];
        s->mesh_state[slot].arena_stale = false;
    }
    return SR_OK;
}

// The frame's light table by the kernel: arena, entries (only where they differ from the device's copy), table. Null stream,
// like the other kernels of sr_scene_set_instances, and waited for here: the passes run on streams of their own.
int device_light_table(SrScene* s) {
    SrLightTableInfo& li = s->lt_info;
    EventPair positions(s), table(s);
    positions.begin(nullptr);
    int rc = sync_device_arena(s, &li.positions_rewritten, &li.arena_uploads);
    if (rc != SR_OK) return rc;
    positions.end(nullptr);
    const std::vector<SrEmissiveIndirectionEntry>& entries = s->fid.emissive_entries;
    const size_t entry_bytes = sizeof(SrEmissiveIndirectionEntry) * entries.size();
    if (s->entries_on_device.size() != entries.size() || memcmp(s->entries_on_device.data(), entries.data(), entry_bytes) != 0) {
        if ((rc = s->d_light_entries.upload(entries.data(), entry_bytes)) != SR_OK) return rc;
        s->entries_on_device = entries;
        li.entries_uploaded = 1;
    }
    if ((rc = s->d_lights.reserve(entries.size() * 64)) != SR_OK) return rc;
    table.begin(nullptr);
    const int e = srk_light_table((const SrEmissiveIndirectionEntry*)s->d_light_entries.p, (uint32_t)entries.size(), (const SrEmissiveTriangle*)s->d_arena.p,
                                  s->arena_device_entries, (const srd::FlatInstance*)s->d_flat_instances.p, (uint32_t)s->fid.instances.size(),
                                  (float*)s->d_lights.p, nullptr);
    if (e != 0) return fail(SR_ERR_HIP, std::string("light table launch failed: ") + hipGetErrorString((hipError_t)e));
    table.end(nullptr);
    HIP_TRY(hipStreamSynchronize(nullptr));
    li.positions_ms += positions.ms(); li.table_ms += table.ms();
    li.on_device = 1;
    return SR_OK;
}

// What follows a mesh's new vertices once they are in its device allocation (and, for a mesh with emissive entries whose arena
// slots the host keeps, in the host copy): the positions of its arena slots, then which trees and structures are stale.
void mesh_vertices_changed(SrScene* s, uint32_t slot) {
    const srh::HostMesh& m = s->meshes[slot];
    const bool host_positions = !s->mesh_state[slot].arena_stale;       // arena_stale: the host copy is old, the device rewrites the slots
    if (host_positions && !m.emissive_slots.empty()) s->arena_host_dirty = true;
    for (size_t k = 0; host_positions && k < m.emissive_slots.size(); k++) {   // positions only: emission follows the material, which stays
        SrEmissiveTriangle& et = s->emissive_tris[m.emissive_slots[k]];
        memcpy(et.v0, m.vertices[m.indices[3 * k]].position, 12);
        memcpy(et.v1, m.vertices[m.indices[3 * k + 1]].position, 12);
        memcpy(et.v2, m.vertices[m.indices[3 * k + 2]].position, 12);
    }
    // two-level form: this mesh's object-space tree, root box and padding numbers are stale; the other meshes keep theirs. An
    // updatable mesh (sr_scene_set_mesh_build_type) with a valid tree keeps it: the next sr_scene_set_instances refits it on the
    // or builds it on the device where it can (maintain_mesh_trees) and invalidates it otherwise
    if (s->mesh_state[slot].build_type != SR_BUILD_STATIC && s->mesh_state[slot].tree.valid) s->mesh_state[slot].refit_pending = true;
    else { invalidate_mesh_tree(s, slot); s->static_mesh_updated = s->static_mesh_updated || s->mesh_state[slot].build_type == SR_BUILD_STATIC; }
    if (s->built) {
        bool instanced = false;
        for (const auto& in : s->fid.instances) if (in.mesh_slot == slot) { instanced = true; break; }
        if (instanced) { s->mesh_state[slot].dirty = true; s->geometry_stale = true; }
    }
}

// What follows validated vertices that a copy or a kernel has just put into a mesh's device allocation in `copy_ms`: the host
// copy left behind, and for a mesh with emissive entries the fetch at once under SR_LIGHTS_HOST (the light table is then host
// arithmetic on every sr_scene_set_instances) or, under SR_LIGHTS_DEVICE, the mark that its arena slots are to be rewritten on
// the device. mesh_vertices_changed comes after it.
int device_vertices_taken(SrScene* s, uint32_t slot, double copy_ms) {
    srh::HostMesh& m = s->meshes[slot];
    m.copy_ms = copy_ms;
    m.host_stale = true; m.last_from_device = true;
    if (m.emissive_slots.empty()) return SR_OK;
    if (s->light_mode == SR_LIGHTS_DEVICE) {                 // the arena positions follow on the device (sync_device_arena): no fetch
        s->mesh_state[slot].arena_stale = true; s->mesh_state[slot].arena_pending = true;
        return SR_OK;
    }
    return fetch_host_vertices(s, slot);
}

// The copy of validated device vertices into a mesh's allocation (sr_scene_update_mesh_device, the mesh frame and the replicas
// of a renderer): the device wait (frames in flight read the old vertices), the copy on the null stream, then
// device_vertices_taken.
int take_device_vertices(SrScene* s, uint32_t slot, const SrVertex* d_vertices, int src_device) {
    srh::HostMesh& m = s->meshes[slot];
    const size_t bytes = sizeof(SrVertex) * (size_t)m.n_vertices;
    HIP_TRY(hipDeviceSynchronize());
    EventPair timer(s);
    timer.begin(nullptr);
    hipError_t e = src_device == s->device ? hipMemcpyAsync(m.d_vertices, d_vertices, bytes, hipMemcpyDeviceToDevice, nullptr)
                                           : hipMemcpyPeerAsync(m.d_vertices, s->device, d_vertices, src_device, bytes, nullptr);
    timer.end(nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) m.copy_ms = 0.0;
    HIP_TRY(e);
    return device_vertices_taken(s, slot, timer.ms());
}

// SrMeshUpdateInfo of an update that entered at t0, copied between t1 and t2 and ends now.
void note_update_times(SrScene* s, std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1, std::chrono::steady_clock::time_point t2) {
    s->mu_info.validate_copy_ms = ms_between(t0, t1) + ms_between(t2, std::chrono::steady_clock::now());
    s->mu_info.h2d_ms = ms_between(t1, t2);
}

// The middle of a device producer. `upload()` puts what the kernels read on `st`, `enqueue(check)` the producer's kernels; each
// answers in a word of `check` (the srk_* launches preset theirs to 0xFFFFFFFF). Both return a hipError_t as int: not 0, nothing
// more is enqueued. The timing pair brackets the kernels and the one read-back of `n_words` words into `bad`, the stream is
// waited for, and *ms is the bracketed time (0.0 with timing off). A HIP failure is refused in the caller's words `what`.
template <class Upload, class Enqueue>
int checked_launch(SrScene* s, hipStream_t st, uint32_t n_words, uint32_t* bad, double* ms, const char* what, Upload upload, Enqueue enqueue) {
    EventPair timer(s);
    int e = upload();
    timer.begin(st);
    if (e == 0) e = enqueue((uint32_t*)s->d_vertex_check.p);
    if (e == 0) e = (int)hipMemcpyAsync(bad, s->d_vertex_check.p, 4 * (size_t)n_words, hipMemcpyDeviceToHost, st);
    timer.end(st);
    if (e == 0) e = (int)hipStreamSynchronize(st);
    if (e != 0) return fail(SR_ERR_HIP, std::string(what) + hipGetErrorString((hipError_t)e));
    *ms = timer.ms();
    return SR_OK;
}

// The tail of every path that hands a mesh vertices already validated on a device (sr_scene_update_mesh_device, the mesh frame,
// the replicas of a renderer): the copy into the mesh's allocation, check_ms (the time of a validation kernel of its own, 0.0
// where the check was part of the producer or ran on another scene), what follows from new vertices, and SrMeshUpdateInfo of a
// call that entered at t0. The next device producer is its own refusals and kernels, checked_launch and this.
int finish_device_update(SrScene* s, uint32_t slot, const SrVertex* d_vertices, int src_device, double check_ms, std::chrono::steady_clock::time_point t0) {
    const auto t1 = std::chrono::steady_clock::now();
    const int rc = take_device_vertices(s, slot, d_vertices, src_device);
    if (rc != SR_OK) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    s->meshes[slot].check_ms = check_ms;
    mesh_vertices_changed(s, slot);
    note_update_times(s, t0, t1, t2);
    return SR_OK;
}

// What sr_scene_set_mesh_skin and sr_scene_set_mesh_morph share. Detaching waits for whatever reads the record's buffers.
template <class Record>
int detach_record(Record& r) {
    HIP_TRY(hipDeviceSynchronize());
    r = Record();
    return SR_OK;
}
// The snapshot of a mesh's vertices as they stand on the device (the bind pose, the morph base) into a buffer not yet attached.
int snapshot_vertices(const srh::HostMesh& m, DeviceBuffer& dst) {
    const size_t bytes = sizeof(SrVertex) * (size_t)m.n_vertices;
    const int rc = dst.reserve(bytes);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());                          // whatever still writes the mesh's vertices has finished
    HIP_TRY(hipMemcpy(dst.p, m.d_vertices, bytes, hipMemcpyDeviceToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return SR_OK;
}

}  // namespace

extern "C" {

const char* sr_last_error(void) { return g_last_error.c_str(); }
int sr_version(void) { return 1; }

int sr_camera_matrices(const float position[3], const float target[3], float fov_y_degrees, uint32_t width,
                       uint32_t height, const float* prev_view_proj16, SrMatrices* out) {
    if (!position || !target || !out || width == 0 || height == 0) return fail(SR_ERR_INVALID_ARG, "sr_camera_matrices: null argument or empty extent");
    srh::Camera cam;
    memcpy(cam.position, position, 12);
    memcpy(cam.target, target, 12);
    cam.fov_y = fov_y_degrees;
    if (!cam.as_matrices(width, height, prev_view_proj16, out)) return fail(SR_ERR_INVALID_ARG, "sr_camera_matrices: singular view/projection matrix");
    return SR_OK;
}

int sr_material_new(const float base_color[4], float metallic, float roughness, const float emissive_factor[3],
                    float emissive_strength, float transmission, float ior, SrMaterial* out) {
    if (!base_color || !emissive_factor || !out) return fail(SR_ERR_INVALID_ARG, "sr_material_new: null argument");
    srh::material_new(base_color, metallic, roughness, emissive_factor, emissive_strength, transmission, ior, out);
    return SR_OK;
}

int sr_emissive_triangles_from_mesh(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                                    uint32_t n_indices, const SrMaterial* material, SrEmissiveTriangle* out,
                                    uint32_t cap, uint32_t* out_count) {
    if (!vertices || !indices || !material || !out_count) return fail(SR_ERR_INVALID_ARG, "sr_emissive_triangles_from_mesh: null argument");
    if (!out && cap > 0) return fail(SR_ERR_INVALID_ARG, "sr_emissive_triangles_from_mesh: out is null but cap > 0 (pass cap = 0 to query the count)");
    if (first_index_out_of_range(indices, n_indices, n_vertices) < n_indices) return fail(SR_ERR_INVALID_ARG, "sr_emissive_triangles_from_mesh: index out of range");
    std::vector<SrEmissiveTriangle> v;
    srh::emissive_triangles_from_mesh(vertices, indices, n_indices, *material, v);
    *out_count = (uint32_t)v.size();
    if (out) memcpy(out, v.data(), sizeof(SrEmissiveTriangle) * std::min<size_t>(cap, v.size()));
    return SR_OK;
}

void sr_trace_config_default(SrTraceConfig* out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->max_bounces = 10;
    out->shadow_bounces = 5;
    out->ris_candidates = 16;
    out->virtual_bounces = 20;
    out->enable_restir = 1;
}

int sr_scene_create(int device, SrScene** out) {
    if (!out) return fail(SR_ERR_INVALID_ARG, "sr_scene_create: out is null");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(SR_ERR_INVALID_ARG, "sr_scene_create: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    SrScene* s = new SrScene();
    s->device = device;
    if (const char* ev = getenv("SR_TILE_SCHEDULING")) s->tile_scheduling = atoi(ev) != 0;
    if (const char* ev = getenv("SR_INSTANCING")) s->instancing = !strcmp(ev, "two_level") ? SR_INSTANCING_TWO_LEVEL : (!strcmp(ev, "flat") ? SR_INSTANCING_FLAT : SR_INSTANCING_AUTO);
    if (const char* ev = getenv("SR_TL_BUILD")) s->tl_build_mode = !strcmp(ev, "host") ? SR_TL_BUILD_HOST : (!strcmp(ev, "device") ? SR_TL_BUILD_DEVICE : SR_TL_BUILD_AUTO);
    if (const char* ev = getenv("SR_BLAS_BATCH")) s->blas_batch_mode = !strcmp(ev, "on") ? SR_BLAS_BATCH_ON : SR_BLAS_BATCH_OFF;
    if (const char* ev = getenv("SR_BLAS_BUILD")) s->blas_build_mode = !strcmp(ev, "host") ? SR_MESH_TREE_BUILD_HOST : (!strcmp(ev, "device") ? SR_MESH_TREE_BUILD_DEVICE : SR_MESH_TREE_BUILD_AUTO);
    if (const char* ev = getenv("SR_LIGHT_STAGE")) s->light_stage = atoi(ev) != 0;
    if (const char* ev = getenv("SR_LIGHT_TABLE")) s->light_mode = !strcmp(ev, "device") ? SR_LIGHTS_DEVICE : SR_LIGHTS_HOST;
    if (const char* ev = getenv("SR_FAST_BUILD_HEIGHT")) s->height_bound = !strcmp(ev, "rebalance") ? SR_HEIGHT_BOUND_REBALANCE : SR_HEIGHT_BOUND_REFUSE;
    if (const char* ev = getenv("SR_FAST_BUILD")) s->fast_build_ploc = !strcmp(ev, "lbvh") ? 0 : (!strncmp(ev, "ploc", 4) && atoi(ev + 4) > 0 ? atoi(ev + 4) : 16);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) s->n_cus = prop.multiProcessorCount;
    // the copies of the ray counters, in one small allocation of their own
    const std::vector<unsigned char> zeros(kCounterBytes, 0);
    int rc = s->d_misc.upload(zeros.data(), zeros.size());
    if (rc != SR_OK) { delete s; return rc; }
    *out = s;
    return SR_OK;
}

int sr_scene_destroy(SrScene* s) {
    if (!s) return SR_OK;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    for (auto& m : s->meshes) { if (m.d_vertices) (void)hipFree(m.d_vertices); if (m.d_indices) (void)hipFree(m.d_indices); }
    for (auto& im : s->images) if (im.d_texels) (void)hipFree(im.d_texels);
    delete s;
    return SR_OK;
}

// ResourceManager::add_blas (resource_manager.rs:417-447): the mesh-info slot becomes the instance custom index, the
// local emissive triangles go to the emissive arena.
int sr_scene_add_blas(SrScene* s, uint64_t key, const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                      uint32_t n_indices, const SrMaterial* material, const SrEmissiveTriangle* emissive, uint32_t n_emissive,
                      uint32_t* out_slot) {
    if (!s || !vertices || !indices || !material || (n_emissive && !emissive)) return fail(SR_ERR_INVALID_ARG, "load_mesh: null argument");
    if (s->slots.count(key)) return fail(SR_ERR_INVALID_ARG, "load_mesh: an asset is already registered under this key");
    if (n_vertices == 0 || n_indices == 0 || (n_indices % 3) != 0) {
        char buf[200];
        snprintf(buf, sizeof(buf), "load_mesh: invalid mesh (%u vertices, %u indices — need non-empty vertices and a triangle-list index count)", n_vertices, n_indices);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    if (const uint32_t i = first_index_out_of_range(indices, n_indices, n_vertices); i < n_indices) {
        char buf[120];
        snprintf(buf, sizeof(buf), "load_mesh: index %u out of range for %u vertices", indices[i], n_vertices);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    // Vulkan treats a triangle with a NaN position as inactive; the builders quantise positions (a non-finite one would
    // be undefined behaviour there), so such meshes are refused instead
    if (const uint32_t i = first_non_finite_vertex(vertices, n_vertices); i < n_vertices) {
        char buf[120];
        snprintf(buf, sizeof(buf), "load_mesh: vertex %u has a non-finite position", i);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    const uint32_t* tex = &material->base_color_image;   // five (image, sampler) slot pairs (resources/material.rs:33-42)
    for (int i = 0; i < 10; i += 2)
        if (tex[i] != SR_NULL_TEXTURE && (tex[i] >= s->images.size() || tex[i + 1] >= s->samplers.size() || !s->images[tex[i]].d_texels))
            return fail(SR_ERR_INVALID_ARG, "load_mesh: material refers to an image or sampler slot that was never added");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    srh::HostMesh m;
    m.key = key;
    m.vertices.assign(vertices, vertices + n_vertices);
    m.indices.assign(indices, indices + n_indices);
    m.n_vertices = n_vertices; m.n_indices = n_indices;
    m.material = *material;
    {
        hipError_t e = hipMalloc(&m.d_vertices, sizeof(SrVertex) * (size_t)n_vertices);
        if (e == hipSuccess) e = hipMemcpy(m.d_vertices, vertices, sizeof(SrVertex) * (size_t)n_vertices, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc(&m.d_indices, sizeof(uint32_t) * (size_t)n_indices);
        if (e == hipSuccess) e = hipMemcpy(m.d_indices, indices, sizeof(uint32_t) * (size_t)n_indices, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (m.d_vertices) (void)hipFree(m.d_vertices);
            if (m.d_indices) (void)hipFree(m.d_indices);
            return fail(e == hipErrorOutOfMemory ? SR_ERR_OOM : SR_ERR_HIP, std::string("load_mesh: geometry upload failed: ") + hipGetErrorString(e));
        }
    }
    for (uint32_t i = 0; i < n_emissive; i++) {
        uint32_t es;
        if (!s->free_emissive_slots.empty()) { es = s->free_emissive_slots.back(); s->free_emissive_slots.pop_back(); s->emissive_tris[es] = emissive[i]; }
        else { es = (uint32_t)s->emissive_tris.size(); s->emissive_tris.push_back(emissive[i]); }
        m.emissive_slots.push_back(es);
    }
    if (n_emissive) s->arena_host_dirty = true;
    SrMeshInfo mi;
    mi.vertices = (uint64_t)(uintptr_t)m.d_vertices;
    mi.indices = (uint64_t)(uintptr_t)m.d_indices;
    mi.material = *material;
    uint32_t slot;
    if (!s->free_mesh_slots.empty()) {
        slot = s->free_mesh_slots.back(); s->free_mesh_slots.pop_back();
        s->mesh_infos[slot] = mi;
        s->meshes[slot] = std::move(m);
    } else {
        slot = (uint32_t)s->meshes.size();
        s->mesh_infos.push_back(mi);
        s->meshes.push_back(std::move(m));
        s->mesh_state.emplace_back();
    }
    s->slots[key] = slot;
    s->built = false;
    s->inst.layout_valid = false;             // a key may name another mesh from here on
    s->mesh_state[slot] = SrScene::MeshState();
    s->trees.blas_device_current = false;
    if (out_slot) *out_slot = slot;
    return SR_OK;
}

int sr_scene_add_mesh(SrScene* s, uint64_t key, const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices,
                      uint32_t n_indices, const SrMaterial* material, uint32_t* out_slot) {
    if (!s || !vertices || !indices || !material) return fail(SR_ERR_INVALID_ARG, "load_mesh: null argument");
    std::vector<SrEmissiveTriangle> et;
    if (n_indices % 3 == 0) {
        if (first_index_out_of_range(indices, n_indices, n_vertices) == n_indices) srh::emissive_triangles_from_mesh(vertices, indices, n_indices, *material, et);   // lib.rs:901-925
    }
    return sr_scene_add_blas(s, key, vertices, n_vertices, indices, n_indices, material, et.data(), (uint32_t)et.size(), out_slot);
}

// ResourceManager::remove (resource_manager.rs:459-487) for a BLAS key: frees the mesh-info slot and the emissive
// slots (reused LIFO by later loads) and the geometry. The reference defers the reclaim by MAX_FRAMES_IN_FLIGHT
// frames; here the device is idle-waited instead. Instances of the key must no longer be passed to set_instances.
int sr_scene_remove(SrScene* s, uint64_t key) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "ResourceManager::remove: scene is null");
    auto it = s->slots.find(key);
    if (it == s->slots.end()) return SR_OK;     // removing an unknown key is a no-op in the reference
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const uint32_t slot = it->second;
    if (s->mesh_state[slot].arena_stale && (rc = refresh_host_arena(s)) != SR_OK) return rc;   // the freed slots keep the mesh's newest positions
    srh::HostMesh& m = s->meshes[slot];
    if (m.d_vertices) (void)hipFree(m.d_vertices);
    if (m.d_indices) (void)hipFree(m.d_indices);
    for (uint32_t es : m.emissive_slots) s->free_emissive_slots.push_back(es);
    m = srh::HostMesh();
    s->mesh_state[slot] = SrScene::MeshState();
    s->trees.blas_device_current = false;
    s->free_mesh_slots.push_back(slot);
    s->slots.erase(it);
    s->built = false;
    s->inst.layout_valid = false;
    return SR_OK;
}

// Blas::update (blas.rs:285-310) for one mesh: the vertex contents change, everything that depends on the topology stays
// (slot, indices, material, emissive slots, device allocations, the built structure and its AsState). What follows from the
// vertices is brought up to date by the next sr_scene_set_instances; until then a structure that instances the mesh is stale.
int sr_scene_update_mesh(SrScene* s, uint64_t key, const SrVertex* vertices, uint32_t n_vertices) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t slot = 0;
    int rc = check_mesh_update(s, key, vertices, n_vertices, &slot);
    if (rc != SR_OK) return rc;
    srh::HostMesh& m = s->meshes[slot];
    if (const uint32_t i = first_non_finite_vertex(vertices, n_vertices); i < n_vertices) return fail_non_finite_vertex(i);
    if ((rc = check_emissive_list(m)) != SR_OK) return rc;
    if ((rc = bind_device(s)) != SR_OK) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    HIP_TRY(hipDeviceSynchronize());                          // launches in flight read the old vertices (as sr_scene_remove waits)
    HIP_TRY(hipMemcpy(m.d_vertices, vertices, sizeof(SrVertex) * (size_t)n_vertices, hipMemcpyHostToDevice));
    const auto t2 = std::chrono::steady_clock::now();
    m.vertices.assign(vertices, vertices + n_vertices);
    m.host_stale = false; m.last_from_device = false;         // the host copy is the device buffer's contents again
    s->mesh_state[slot].arena_stale = s->mesh_state[slot].arena_pending = false;   // and the arena slots are the host's again
    mesh_vertices_changed(s, slot);
    note_update_times(s, t0, t1, t2);
    return SR_OK;
}

// The same for vertices that are already on the scene's device (work on `stream` produced them): no host round trip. Every
// refusal the host can decide comes before anything is launched, and a pointer the runtime does not report as memory of this
// device, `n_vertices` records long, is never handed to a kernel. The positions are validated on the device (vertex_check_kernel,
// the host call's rule), and only then is the mesh's buffer written: check, 4-byte read-back, copy. The host copy is left
// behind (HostMesh::host_stale) and fetched by whatever host code reads it next.
int sr_scene_update_mesh_device(SrScene* s, uint64_t key, const SrVertex* d_vertices, uint32_t n_vertices, void* stream) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t slot = 0;
    int rc = check_mesh_update(s, key, d_vertices, n_vertices, &slot);
    if (rc != SR_OK) return rc;
    srh::HostMesh& m = s->meshes[slot];
    const size_t bytes = sizeof(SrVertex) * (size_t)n_vertices;
    const uintptr_t a = (uintptr_t)d_vertices, own = (uintptr_t)m.d_vertices;
    if (a & 15u) return fail(SR_ERR_INVALID_ARG, "update_mesh: the device vertex pointer is not 16-byte aligned");
    if (a < own + bytes && own < a + bytes) return fail(SR_ERR_INVALID_ARG, "update_mesh: the device vertices overlap the mesh's own vertex buffer");
    if ((rc = check_emissive_list(m)) != SR_OK) return rc;
    if ((rc = bind_device(s)) != SR_OK) return rc;
    if (!device_range_of_scene(s, d_vertices, bytes)) return fail(SR_ERR_INVALID_ARG, "update_mesh: the vertex pointer is not device memory of the scene's device for that many vertices");
    if ((rc = s->d_vertex_check.reserve(16)) != SR_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint32_t first_bad = 0xFFFFFFFFu;
    double check_ms = 0.0;
    rc = checked_launch(s, st, 1, &first_bad, &check_ms, "update_mesh: vertex validation failed: ", [] { return 0; },
                        [&](uint32_t* check) { return srk_vertex_check(d_vertices, n_vertices, check, st); });
    if (rc != SR_OK) return rc;
    if (first_bad < n_vertices) return fail_non_finite_vertex(first_bad);
    return finish_device_update(s, slot, d_vertices, s->device, check_ms, t0);
}

int sr_scene_mesh_vertex_info(const SrScene* s, uint64_t key, SrMeshVertexInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_vertex_info: null argument");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_mesh_vertex_info", &slot); rc != SR_OK) return rc;
    const srh::HostMesh& m = s->meshes[slot];
    memset(out, 0, sizeof(*out));
    out->host_stale = m.host_stale ? 1u : 0u; out->last_from_device = m.last_from_device ? 1u : 0u; out->host_fetches = m.host_fetches;
    out->check_ms = m.check_ms; out->copy_ms = m.copy_ms; out->fetch_ms = m.fetch_ms;
    return SR_OK;
}

// Attaches (or, with influences == NULL, detaches) a mesh's rig. Everything is validated and both buffers are filled before the
// mesh's record changes, so a refusal or a failed allocation leaves an earlier skin in place.
int sr_scene_set_mesh_skin(SrScene* s, uint64_t key, const SrSkinInfluence* influences, uint32_t n_vertices, uint32_t n_joints) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "set_mesh_skin: null argument (the scene)");
    uint32_t slot = 0;
    int rc = find_mesh(s, key, "set_mesh_skin", &slot);
    if (rc != SR_OK || (rc = bind_device(s)) != SR_OK) return rc;
    const srh::HostMesh& m = s->meshes[slot];
    if (!influences) return detach_record(s->mesh_state[slot].skin);
    char buf[200];
    if (n_vertices != m.n_vertices) {
        snprintf(buf, sizeof(buf), "set_mesh_skin: %u influences given, the mesh was loaded with %u vertices", n_vertices, m.n_vertices);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    if (n_joints == 0) return fail(SR_ERR_INVALID_ARG, "set_mesh_skin: a skin needs at least one joint (n_joints is 0)");
    for (uint32_t i = 0; i < n_vertices; i++) {
        const SrSkinInfluence& f = influences[i];
        bool any = false;
        for (int k = 0; k < 4; k++) {
            if (!std::isfinite(f.weight[k]) || f.weight[k] < 0.0f) {
                snprintf(buf, sizeof(buf), "set_mesh_skin: vertex %u has a weight that is negative or not finite (weight %d)", i, k);
                return fail(SR_ERR_INVALID_ARG, buf);
            }
            if (f.weight[k] == 0.0f) continue;
            any = true;
            if (f.joint[k] >= n_joints) {
                snprintf(buf, sizeof(buf), "set_mesh_skin: vertex %u names joint %u with a weight that is not 0, the skin has %u joints", i, (unsigned)f.joint[k], n_joints);
                return fail(SR_ERR_INVALID_ARG, buf);
            }
        }
        if (!any) {
            snprintf(buf, sizeof(buf), "set_mesh_skin: vertex %u has four weights of 0", i);
            return fail(SR_ERR_INVALID_ARG, buf);
        }
    }
    SrScene::MeshState::Skin skin;
    if ((rc = skin.d_influences.upload(influences, sizeof(SrSkinInfluence) * (size_t)n_vertices)) != SR_OK || (rc = snapshot_vertices(m, skin.d_bind)) != SR_OK) return rc;
    skin.n_joints = n_joints;
    s->mesh_state[slot].skin = std::move(skin);
    return SR_OK;
}

namespace {

// What the pose path refuses on the host, before any device work, in the words of the entry point `who`: the mesh's slot into
// *slot and the active list into `active` (2 * n_targets words: the indices of the targets whose weight is not 0, ascending,
// then from word n_targets on their weights) and *n_active. With `clip_targets` the morph stage takes its weights on the device,
// from a morph set of *clip_targets targets: the mesh's morph is checked against that count, the list stays empty.
int check_pose_args(SrScene* s, uint64_t key, const float* weights, uint32_t n_targets, bool joint_matrices, uint32_t n_joints, const char* who,
                    uint32_t* slot, std::vector<uint32_t>& active, uint32_t* n_active, const uint32_t* clip_targets = nullptr) {
    int rc = find_mesh(s, key, who, slot);
    if (rc != SR_OK) return rc;
    const SrScene::MeshState::Morph& morph = s->mesh_state[*slot].morph;
    const SrScene::MeshState::Skin& skin = s->mesh_state[*slot].skin;
    char buf[200];
    if (clip_targets) n_targets = *clip_targets;
    if (weights || clip_targets) {
        if (morph.n_targets == 0) return fail(SR_ERR_INVALID_ARG, "pose_mesh: the mesh has no morph targets (sr_scene_set_mesh_morph attaches them)");
        if (n_targets != morph.n_targets) {
            snprintf(buf, sizeof(buf), "pose_mesh: %u weights given, the morph was attached with %u targets", n_targets, morph.n_targets);
            return fail(SR_ERR_INVALID_ARG, buf);
        }
    }
    if (joint_matrices) {
        if (skin.n_joints == 0) return fail(SR_ERR_INVALID_ARG, std::string(who) + ": the mesh has no skin (sr_scene_set_mesh_skin attaches one)");
        if (n_joints != skin.n_joints) {
            snprintf(buf, sizeof(buf), "%s: %u joint matrices given, the skin was attached with %u joints", who, n_joints, skin.n_joints);
            return fail(SR_ERR_INVALID_ARG, buf);
        }
    }
    active.assign(weights ? 2 * (size_t)n_targets : 0, 0u);
    *n_active = 0;
    for (uint32_t k = 0; weights && k < n_targets; k++) {
        if (!std::isfinite(weights[k])) {
            snprintf(buf, sizeof(buf), "pose_mesh: weight %u is not finite", k);
            return fail(SR_ERR_INVALID_ARG, buf);
        }
        if (weights[k] != 0.0f) { active[*n_active] = k; memcpy(&active[(size_t)n_targets + *n_active], &weights[k], 4); (*n_active)++; }
    }
    return check_emissive_list(s->meshes[*slot]);
}

}  // namespace

int sr_scene_mesh_skin_info(const SrScene* s, uint64_t key, SrMeshSkinInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_skin_info: null argument");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_mesh_skin_info", &slot); rc != SR_OK) return rc;
    const SrScene::MeshState::Skin& skin = s->mesh_state[slot].skin;
    memset(out, 0, sizeof(*out));
    out->n_joints = skin.n_joints; out->skinned = skin.skinned; out->first_bad = skin.first_bad; out->skin_ms = skin.skin_ms;
    return SR_OK;
}

// Attaches (or, with deltas == NULL, detaches) a mesh's morph targets, as sr_scene_set_mesh_skin attaches a rig: everything is
// validated and both buffers are filled before the mesh's record changes, so a refusal or a failed allocation leaves an earlier
// morph in place.
int sr_scene_set_mesh_morph(SrScene* s, uint64_t key, const SrMorphDelta* deltas, uint32_t n_vertices, uint32_t n_targets) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "set_mesh_morph: null argument (the scene)");
    uint32_t slot = 0;
    int rc = find_mesh(s, key, "set_mesh_morph", &slot);
    if (rc != SR_OK) return rc;
    const srh::HostMesh& m = s->meshes[slot];
    if (!deltas) return (rc = bind_device(s)) != SR_OK ? rc : detach_record(s->mesh_state[slot].morph);
    char buf[200];
    if (n_vertices != m.n_vertices) {
        snprintf(buf, sizeof(buf), "set_mesh_morph: targets of %u vertices given, the mesh was loaded with %u vertices", n_vertices, m.n_vertices);
        return fail(SR_ERR_INVALID_ARG, buf);
    }
    if (n_targets == 0) return fail(SR_ERR_INVALID_ARG, "set_mesh_morph: a morph needs at least one target (n_targets is 0)");
    for (uint32_t k = 0; k < n_targets; k++)
        for (uint32_t i = 0; i < n_vertices; i++) {
            const SrMorphDelta& d = deltas[(size_t)k * n_vertices + i];
            bool ok = true;
            for (int c = 0; c < 3; c++) ok = ok && std::isfinite(d.position[c]) && std::isfinite(d.normal[c]) && std::isfinite(d.tangent[c]);
            if (!ok) {
                snprintf(buf, sizeof(buf), "set_mesh_morph: target %u has a delta component that is not finite at vertex %u", k, i);
                return fail(SR_ERR_INVALID_ARG, buf);
            }
        }
    if ((rc = bind_device(s)) != SR_OK) return rc;
    SrScene::MeshState::Morph morph;
    if ((rc = morph.d_deltas.upload(deltas, sizeof(SrMorphDelta) * (size_t)n_vertices * n_targets)) != SR_OK || (rc = snapshot_vertices(m, morph.d_base)) != SR_OK) return rc;
    morph.n_targets = n_targets;
    s->mesh_state[slot].morph = std::move(morph);
    return SR_OK;
}

int sr_scene_mesh_morph_info(const SrScene* s, uint64_t key, SrMeshMorphInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_morph_info: null argument");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_mesh_morph_info", &slot); rc != SR_OK) return rc;
    const SrScene::MeshState::Morph& morph = s->mesh_state[slot].morph;
    memset(out, 0, sizeof(*out));
    out->n_targets = morph.n_targets; out->posed = morph.posed; out->n_active = morph.n_active; out->first_bad = morph.first_bad; out->morph_ms = morph.morph_ms;
    return SR_OK;
}

namespace {

// What sr_scene_pose_actors adds to a batch: the actors' rows for clip_pose_kernel (matrix_base counted from the first matrix the
// kernel writes; pose_items moves it behind the upload), the instance rows of the actors that gave some, and per item its first
// matrix among those the kernel writes (0xFFFFFFFF: the item has no skin stage).
static_assert(sizeof(SrClipActor) == 32 && sizeof(SrActorPoseItem) == 32 && sizeof(SrActorPoseInfo) == 88 && sizeof(SrClipInfo) == 40 && sizeof(SrSplinePoseInfo) == 32, "the header states these sizes");
struct ActorFeed {
    uint32_t n_actors = 0, flags = 0;
    std::vector<srd::ClipActorRow> rows;
    std::vector<uint32_t> instance_rows, item_matrix, actor_joints, actor_nodes;
    // an item whose weights come from its actor's clip: its place among such items, which is its check word's (0xFFFFFFFF: the
    // weights are the host's, or none), and the set's n_targets; the rows (item, active_base and check_word are pose_items' to
    // fill). A row is a plain one, for clip_weights_kernel (or the blended one), or where a set of the item is kClipCubic a spline
    // row, for clip_spline_weights_kernel: item_row_at is the row's position in its own list.
    std::vector<uint32_t> item_weight_row, item_clip_targets, item_row_at;
    std::vector<char> item_spline;
    std::vector<srd::ClipWeightRow> weight_rows;
    std::vector<srd::ClipSplineWeightRow> spline_rows;
    uint64_t n_matrices = 0, n_nodes = 0, n_channels = 0, n_cubic_channels = 0;
    SrTransform* d_instance_transforms = nullptr;
    SrActorPoseInfo* info = nullptr;
    // a blended feed (sr_scene_pose_actors_blended): its rows for clip_blend_kernel and clip_blend_weights_kernel stand where
    // `rows` and `weight_rows` stand in the upload, and the two kernels run where clip_pose_kernel and clip_weights_kernel run
    bool blended = false;
    std::vector<srd::ClipBlendActorRow> blend_rows;
    std::vector<srd::ClipBlendWeightRow> blend_weight_rows;
    // a layered feed (sr_scene_pose_actors_layered): its actor rows for clip_layers_kernel stand where `rows` stand, the layer
    // table travels behind the weight rows, and its clip-weighted items are plain ones, built from the base layers
    bool layered = false;
    std::vector<srd::ClipLayerActorRow> layer_actor_rows;
    std::vector<srd::ClipLayerRow> layer_rows;
    std::vector<SrScene::ActorLayerRecord> layer_records;
    uint64_t n_layer_nodes = 0;
    SrLayerPoseInfo layer_info{0, 0, 0, 0, 0, 0};
    // ... with SR_ACTORS_LAYER_WEIGHTS: its clip-weighted items are rows for clip_layer_weights_kernel, which stand where
    // `weight_rows` stand (there are no spline rows), and their entries, one per row and layer, travel behind the layer table
    bool layer_weights = false;
    std::vector<srd::ClipLayerWeightRow> layer_weight_rows;
    std::vector<srd::ClipLayerWeightEntry> layer_weight_entries;
    SrLayerWeightsInfo layer_weights_info{0, 0, 0, 0, 0, 0.0};
    uint32_t n_plain_rows() const { return (uint32_t)(blended ? blend_weight_rows.size() : layer_weights ? layer_weight_rows.size() : weight_rows.size()); }
    uint32_t n_weight_rows() const { return n_plain_rows() + (uint32_t)spline_rows.size(); }
    void add_weight_item(uint32_t i, uint32_t n_targets, bool spline) {
        item_weight_row[i] = n_weight_rows(); item_clip_targets[i] = n_targets; item_spline[i] = spline ? 1 : 0;
        item_row_at[i] = spline ? (uint32_t)spline_rows.size() : n_plain_rows();
    }
    void count_cubic_channels(const SrClip& clip) {
        for (uint32_t k = 0; k < clip.header().n_channels; k++) n_cubic_channels += clip.channels()[k].interpolation == srd::kClipCubic ? 1u : 0u;
    }
    size_t actor_row_bytes() const { return blended ? sizeof(srd::ClipBlendActorRow) : layered ? sizeof(srd::ClipLayerActorRow) : sizeof(srd::ClipActorRow); }
    const void* actor_row_data() const { return blended ? (const void*)blend_rows.data() : layered ? (const void*)layer_actor_rows.data() : (const void*)rows.data(); }
    size_t weight_row_bytes() const { return blended ? sizeof(srd::ClipBlendWeightRow) : layer_weights ? sizeof(srd::ClipLayerWeightRow) : sizeof(srd::ClipWeightRow); }
    const void* weight_row_data() const { return blended ? (const void*)blend_weight_rows.data() : layer_weights ? (const void*)layer_weight_rows.data() : (const void*)weight_rows.data(); }
    uint32_t& matrix_base(uint32_t a) { return blended ? blend_rows[a].matrix_base : layered ? layer_actor_rows[a].matrix_base : rows[a].matrix_base; }
    uint32_t node_base(uint32_t a) const { return blended ? blend_rows[a].node_base : layered ? layer_actor_rows[a].node_base : rows[a].node_base; }
};

// The one posing path: sr_scene_pose_meshes (`batch`) and, with a list of one item, sr_scene_skin_mesh and sr_scene_pose_mesh.
// Many meshes posed by one upload, one launch and one read-back (the header states the contract). Host checks for every item
// first (check_pose_args), then the plan and the staging block, the posing launch into the batch scratch, and for an accepted
// call the device wait, the scatter launch and the per-mesh host tail. *out takes the figures of a call that reached the
// device (calls: one more than it held) and is left alone otherwise. What differs between the callers is stated here:
//   - the words: the batch puts "pose_meshes: item <i>: " before every refusal of an item and names itself for a HIP failure; a
//     single call refuses with no prefix and in the entry point's own words;
//   - what a refusal for a non-finite vertex records: the batch the first_bad of the stages that reported, and no more; a single
//     call the first_bad of every stage that ran (0xFFFFFFFF where that stage did not report) and n_active.
// With a `feed` (sr_scene_pose_actors) the call is a batch whose words say "pose_actors", whose items may take their matrices
// from the slice clip_pose_kernel writes instead of a host pointer, and which may have no item at all: the actors' rows and
// instance rows travel behind the batch's parts in the one upload, the clip kernel runs in front of the posing kernel, one more
// check word per actor comes back in the one read-back (a singular mesh-node transform refuses like a non-finite vertex, before
// it), and *feed->info takes the call's figures where *out takes the batch's.
// An item of a feed may take its weights from its actor's clip (feed->item_weight_row): it has a morph stage without host weights.
// Its row for clip_weights_kernel travels behind the actors' rows in the one upload, the kernel runs between the clip kernel and
// the posing kernel and writes the item's active list into a slot of n_targets entries and its count into the uploaded item row,
// and one more check word per such item brings the count back. In a call where no item has host weights the active arrays lie
// behind everything else in the staging block, outside the upload, so the upload does not grow with the targets; where some
// have, the slots follow the host's lists inside the arrays. A call without such an item is laid out and launched as ever.
// Such an item with a kClipCubic set is a spline row: the spline rows travel behind the plain rows in the same upload and
// clip_spline_weights_kernel runs behind the plain rows' kernel; either kernel is launched only where it has a row.
int pose_items(SrScene* s, const SrPoseItem* items, uint32_t n_items, void* stream, bool batch, SrPoseBatchInfo* out, ActorFeed* feed = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::string who = feed ? (feed->blended ? "pose_actors_blended" : feed->layered ? "pose_actors_layered" : "pose_actors") : batch ? "pose_meshes" : items[0].weights ? "pose_mesh" : "skin_mesh";
    const auto prefix = [batch, &who](uint32_t i) { return batch ? who + ": item " + std::to_string(i) + ": " : std::string(); };
    // an item's skin stage: its matrices come from the caller's host pointer, or from the slice the clip kernel writes
    const auto fed = [feed](uint32_t i) { return feed && feed->item_matrix[i] != 0xFFFFFFFFu; };
    const auto skin_stage = [items, &fed](uint32_t i) { return items[i].joint_matrices != nullptr || fed(i); };
    const auto clip_weighted = [feed](uint32_t i) { return feed && feed->item_weight_row[i] != 0xFFFFFFFFu; };
    const auto morph_stage = [items, &clip_weighted](uint32_t i) { return items[i].weights != nullptr || clip_weighted(i); };
    const uint32_t n_weight_items = feed ? feed->n_weight_rows() : 0;
    uint64_t n_slots = 0;                                     // entries of the clip-weighted items' slots
    std::vector<uint32_t> slots(n_items), counts(n_items), n_active(n_items), active_index, active;
    std::vector<float> active_weight;
    std::map<uint64_t, uint32_t> seen;
    uint64_t n_matrices = 0;
    int rc;
    for (uint32_t i = 0; i < n_items; i++) {
        const SrPoseItem& it = items[i];
        if (!morph_stage(i) && !skin_stage(i)) return fail(SR_ERR_INVALID_ARG, prefix(i) + "pose_mesh: neither weights nor joint matrices given (one stage at least)");
        rc = check_pose_args(s, it.key, it.weights, it.n_targets, skin_stage(i), it.n_joints, morph_stage(i) ? "pose_mesh" : "skin_mesh", &slots[i], active, &n_active[i],
                             clip_weighted(i) ? &feed->item_clip_targets[i] : nullptr);
        if (rc != SR_OK) return fail(rc, prefix(i) + g_last_error);
        if (clip_weighted(i)) n_slots += feed->item_clip_targets[i];
        const auto first = seen.emplace(it.key, i);
        if (!first.second) return fail(SR_ERR_INVALID_ARG, prefix(i) + "the key is named twice in the batch (first by item " + std::to_string(first.first->second) + ")");
        counts[i] = s->meshes[slots[i]].n_vertices;
        active_index.insert(active_index.end(), active.begin(), active.begin() + n_active[i]);
        for (uint32_t a = 0; a < n_active[i]; a++) { float w; memcpy(&w, &active[(size_t)it.n_targets + a], 4); active_weight.push_back(w); }
        if (it.joint_matrices) n_matrices += it.n_joints;
    }
    if (n_matrices >= (1ull << 32) || active_index.size() + n_slots >= (1ull << 32)) return fail(SR_ERR_UNSUPPORTED, "pose_meshes: the batch holds 2^32 joint matrices or active targets or more");
    std::vector<uint32_t> first_block(n_items);
    std::vector<uint64_t> vertex_base(n_items);
    uint32_t n_blocks = 0;
    if ((rc = sr_pose_batch_plan(counts.data(), n_items, first_block.data(), vertex_base.data(), &n_blocks)) != SR_OK) return rc;
    const uint64_t n_vertices = n_items ? vertex_base[n_items - 1] + counts[n_items - 1] : 0;
    const size_t n_host_active = active_index.size();
    const bool slots_outside = n_weight_items && n_host_active == 0;      // the active arrays are the slots alone: behind the staging block's other parts
    srh::PoseBatchLayout lay = srh::pose_batch_layout(n_items, n_blocks, n_matrices, slots_outside ? 0 : n_host_active + n_slots);
    // Actors add their rows and their instance rows behind the batch's parts: that is the upload. The matrices the clip kernel
    // writes follow it, outside the uploaded bytes, a whole number of matrices from lay.matrices so that matrix_base reaches them.
    const uint32_t n_actors = feed ? feed->n_actors : 0;
    const size_t actor_rows_at = lay.bytes, weight_rows_at = actor_rows_at + (feed ? feed->actor_row_bytes() : 0) * (size_t)n_actors;
    const uint32_t n_plain_rows = feed ? feed->n_plain_rows() : 0, n_spline_rows = n_weight_items - n_plain_rows;
    const size_t spline_rows_at = weight_rows_at + (feed ? feed->weight_row_bytes() : 0) * (size_t)n_plain_rows;
    const size_t layer_rows_at = spline_rows_at + sizeof(srd::ClipSplineWeightRow) * (size_t)n_spline_rows;      // a layered feed's layer table
    const size_t layer_targets_at = layer_rows_at + sizeof(srd::ClipLayerRow) * (feed ? feed->layer_rows.size() : 0);   // ... and where its results go
    const size_t layer_entries_at = layer_targets_at + (feed && feed->layered ? sizeof(srd::ClipLayerTargets) : 0);    // ... and its layer-weight entries
    const size_t inst_rows_at = layer_entries_at + sizeof(srd::ClipLayerWeightEntry) * (feed ? feed->layer_weight_entries.size() : 0);
    const size_t upload_bytes = inst_rows_at + ((4 * (feed ? feed->instance_rows.size() : 0) + 15u) & ~(size_t)15u);
    const uint64_t fed_first = (upload_bytes - lay.matrices + sizeof(SrTransform) - 1) / sizeof(SrTransform);
    size_t stage_bytes = feed ? lay.matrices + sizeof(SrTransform) * (size_t)(fed_first + feed->n_matrices) : lay.bytes;
    if (feed && fed_first + feed->n_matrices >= (1ull << 32)) return fail(SR_ERR_UNSUPPORTED, who + ": the call holds 2^32 joint matrices or more");
    if (slots_outside) {
        const size_t slot_bytes = (4 * (size_t)n_slots + 15u) & ~(size_t)15u;
        lay.active_index = (stage_bytes + 15u) & ~(size_t)15u; lay.active_weight = lay.active_index + slot_bytes;
        stage_bytes = lay.active_weight + slot_bytes;
    }
    const size_t n_check = 2 * (size_t)n_items + n_actors + n_weight_items;
    if ((rc = bind_device(s)) != SR_OK) return rc;
    if ((rc = s->d_pose_stage.reserve(stage_bytes)) != SR_OK || (rc = s->d_pose_check.reserve(4 * n_check)) != SR_OK ||
        (rc = s->d_pose_scratch.reserve(sizeof(SrVertex) * (size_t)n_vertices)) != SR_OK) return rc;
    const bool keep_nodes = feed && (feed->flags & SR_ACTORS_KEEP_NODES);
    if (keep_nodes && ((rc = s->d_actor_trs.reserve(sizeof(SrNodeTrs) * (size_t)feed->n_nodes)) != SR_OK || (rc = s->d_actor_globals.reserve(64 * (size_t)feed->n_nodes)) != SR_OK)) return rc;
    const bool keep_sources = feed && feed->blended && (feed->flags & SR_ACTORS_KEEP_SOURCES);
    if (keep_sources && ((rc = s->d_actor_source_a.reserve(sizeof(SrNodeTrs) * (size_t)feed->n_nodes)) != SR_OK ||
                         (rc = s->d_actor_source_b.reserve(sizeof(SrNodeTrs) * (size_t)feed->n_nodes)) != SR_OK)) return rc;
    const bool keep_layers = feed && feed->layered && (feed->flags & SR_ACTORS_KEEP_LAYERS);
    if (keep_layers && ((rc = s->d_actor_layer_cur.reserve(sizeof(SrNodeTrs) * (size_t)feed->n_layer_nodes)) != SR_OK ||
                        (rc = s->d_actor_layer_ref.reserve(sizeof(SrNodeTrs) * (size_t)feed->n_layer_nodes)) != SR_OK)) return rc;
    // the staging block: rows, block table, matrices, active lists; then the actors' rows and instance rows
    std::vector<unsigned char> stage(upload_bytes, 0);
    srd::PoseBatchItem* rows = (srd::PoseBatchItem*)(stage.data() + lay.items);
    SrPoseBatchInfo info{n_items, n_blocks, n_vertices, 0, 0, 0, 0, 0, out->calls + 1, 0xFFFFFFFFu, 0xFFFFFFFFu, lay.bytes, 0.0, 0.0, 0.0};
    uint32_t matrix_base = 0, active_base = 0;
    for (uint32_t i = 0; i < n_items; i++) {
        const SrPoseItem& it = items[i];
        const SrScene::MeshState& ms = s->mesh_state[slots[i]];
        srd::PoseBatchItem& row = rows[i];
        row.src = morph_stage(i) ? ms.morph.d_base.p : ms.skin.d_bind.p;
        row.deltas = morph_stage(i) ? ms.morph.d_deltas.p : nullptr;
        row.influences = skin_stage(i) ? ms.skin.d_influences.p : nullptr;
        row.dst = s->meshes[slots[i]].d_vertices;
        row.vertex_base = vertex_base[i];
        row.n_vertices = counts[i]; row.first_block = first_block[i];
        row.n_active = n_active[i]; row.active_base = active_base;
        row.matrix_base = fed(i) ? (uint32_t)fed_first + feed->item_matrix[i] : matrix_base;
        row.stages = (morph_stage(i) ? srd::kPoseMorph : 0u) | (skin_stage(i) ? srd::kPoseSkin : 0u);
        if (it.joint_matrices) { memcpy(stage.data() + lay.matrices + sizeof(SrTransform) * (size_t)matrix_base, it.joint_matrices, sizeof(SrTransform) * (size_t)it.n_joints); matrix_base += it.n_joints; }
        active_base += n_active[i];
        (row.stages == 3u ? info.fused : morph_stage(i) ? info.morph_only : info.skin_only)++;
    }
    for (uint32_t i = 0; i < n_items; i++) {                  // the slots follow the host's lists; the kernel writes n_active (0 until then)
        if (!clip_weighted(i)) continue;
        const uint32_t check_word = (uint32_t)(2 * (size_t)n_items + n_actors + feed->item_weight_row[i]);
        if (feed->item_spline[i]) { srd::ClipSplineWeightRow& wr = feed->spline_rows[feed->item_row_at[i]]; wr.item = i; wr.active_base = active_base; wr.check_word = check_word; }
        else if (feed->blended) { srd::ClipBlendWeightRow& wr = feed->blend_weight_rows[feed->item_row_at[i]]; wr.item = i; wr.active_base = active_base; wr.check_word = check_word; }
        else if (feed->layer_weights) { srd::ClipLayerWeightRow& wr = feed->layer_weight_rows[feed->item_row_at[i]]; wr.item = i; wr.active_base = active_base; wr.check_word = check_word; }
        else { srd::ClipWeightRow& wr = feed->weight_rows[feed->item_row_at[i]]; wr.item = i; wr.active_base = active_base; wr.check_word = check_word; }
        rows[i].active_base = active_base;
        active_base += feed->item_clip_targets[i];
    }
    srh::pose_batch_block_table(first_block.data(), n_items, n_blocks, (uint32_t*)(stage.data() + lay.block_table));
    if (!active_index.empty()) {
        memcpy(stage.data() + lay.active_index, active_index.data(), 4 * active_index.size());
        memcpy(stage.data() + lay.active_weight, active_weight.data(), 4 * active_weight.size());
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* d_stage = (const unsigned char*)s->d_pose_stage.p;
    const srd::PoseBatchItem* d_rows = (const srd::PoseBatchItem*)(d_stage + lay.items);
    const uint32_t* d_table = (const uint32_t*)(d_stage + lay.block_table);
    std::vector<uint32_t> bad(n_check, 0xFFFFFFFFu);
    EventPair pose_timer(s), scatter_timer(s), clip_timer(s), spline_timer(s), layer_weights_timer(s);
    if (feed) {
        for (uint32_t a = 0; a < n_actors; a++) feed->matrix_base(a) += (uint32_t)fed_first;
        if (n_actors) memcpy(stage.data() + actor_rows_at, feed->actor_row_data(), feed->actor_row_bytes() * (size_t)n_actors);
        if (!feed->layer_rows.empty()) memcpy(stage.data() + layer_rows_at, feed->layer_rows.data(), sizeof(srd::ClipLayerRow) * feed->layer_rows.size());
        if (feed->layered) {                                  // what srk_clip_pose takes as arguments, clip_layers_kernel reads from the upload
            srd::ClipLayerTargets to{};
            to.rows = (const uint32_t*)(d_stage + inst_rows_at);
            to.matrices = (unsigned char*)s->d_pose_stage.p + lay.matrices;
            to.instance_transforms = feed->d_instance_transforms;
            to.check = (uint32_t*)s->d_pose_check.p + 2 * (size_t)n_items;
            to.keep_trs = keep_nodes ? s->d_actor_trs.p : nullptr; to.keep_globals = keep_nodes ? s->d_actor_globals.p : nullptr;
            to.keep_cur = keep_layers ? s->d_actor_layer_cur.p : nullptr; to.keep_ref = keep_layers ? s->d_actor_layer_ref.p : nullptr;
            memcpy(stage.data() + layer_targets_at, &to, sizeof(to));
        }
        if (n_plain_rows)
            memcpy(stage.data() + weight_rows_at, feed->weight_row_data(), feed->weight_row_bytes() * (size_t)n_plain_rows);
        if (!feed->layer_weight_entries.empty())
            memcpy(stage.data() + layer_entries_at, feed->layer_weight_entries.data(), sizeof(srd::ClipLayerWeightEntry) * feed->layer_weight_entries.size());
        if (n_spline_rows) memcpy(stage.data() + spline_rows_at, feed->spline_rows.data(), sizeof(srd::ClipSplineWeightRow) * (size_t)n_spline_rows);
        if (!feed->instance_rows.empty()) memcpy(stage.data() + inst_rows_at, feed->instance_rows.data(), 4 * feed->instance_rows.size());
    }
    s->actor_stage_current = false;                          // the block changes hands
    int e = (int)hipMemsetAsync(s->d_pose_check.p, 0xFF, 4 * n_check, st);
    if (e == 0) e = (int)hipMemcpyAsync(s->d_pose_stage.p, stage.data(), upload_bytes, hipMemcpyHostToDevice, st);
    if (feed) {
        clip_timer.begin(st);
        SrTransform* fed_matrices = (SrTransform*)(s->d_pose_stage.p ? (unsigned char*)s->d_pose_stage.p + lay.matrices : nullptr);
        uint32_t* actor_check = (uint32_t*)s->d_pose_check.p + 2 * (size_t)n_items;
        SrNodeTrs* kept_trs = keep_nodes ? (SrNodeTrs*)s->d_actor_trs.p : nullptr;
        float* kept_globals = keep_nodes ? (float*)s->d_actor_globals.p : nullptr;
        if (e == 0 && feed->blended)
            e = srk_clip_blend((const srd::ClipBlendActorRow*)(d_stage + actor_rows_at), n_actors, (const uint32_t*)(d_stage + inst_rows_at), fed_matrices, feed->d_instance_transforms,
                               actor_check, kept_trs, kept_globals, keep_sources ? (SrNodeTrs*)s->d_actor_source_a.p : nullptr,
                               keep_sources ? (SrNodeTrs*)s->d_actor_source_b.p : nullptr, st);
        else if (e == 0 && feed->layered)
            e = srk_clip_layers((const srd::ClipLayerActorRow*)(d_stage + actor_rows_at), n_actors, (const srd::ClipLayerRow*)(d_stage + layer_rows_at),
                                (const srd::ClipLayerTargets*)(d_stage + layer_targets_at), st);
        else if (e == 0)
            e = srk_clip_pose((const srd::ClipActorRow*)(d_stage + actor_rows_at), n_actors, (const uint32_t*)(d_stage + inst_rows_at), fed_matrices, feed->d_instance_transforms,
                              actor_check, kept_trs, kept_globals, st);
        if (e == 0 && n_plain_rows && feed->blended)
            e = srk_clip_blend_weights((const srd::ClipBlendWeightRow*)(d_stage + weight_rows_at), n_plain_rows, (srd::PoseBatchItem*)((unsigned char*)s->d_pose_stage.p + lay.items),
                                       (uint32_t*)((unsigned char*)s->d_pose_stage.p + lay.active_index), (float*)((unsigned char*)s->d_pose_stage.p + lay.active_weight),
                                       (uint32_t*)s->d_pose_check.p, st);
        else if (n_plain_rows && feed->layer_weights) {
            layer_weights_timer.begin(st);
            if (e == 0)
                e = srk_clip_layer_weights((const srd::ClipLayerWeightRow*)(d_stage + weight_rows_at), n_plain_rows, (const srd::ClipLayerRow*)(d_stage + layer_rows_at),
                                           (const srd::ClipLayerWeightEntry*)(d_stage + layer_entries_at), (srd::PoseBatchItem*)((unsigned char*)s->d_pose_stage.p + lay.items),
                                           (uint32_t*)((unsigned char*)s->d_pose_stage.p + lay.active_index), (float*)((unsigned char*)s->d_pose_stage.p + lay.active_weight),
                                           (uint32_t*)s->d_pose_check.p, st);
            layer_weights_timer.end(st);
        } else if (e == 0 && n_plain_rows)
            e = srk_clip_weights((const srd::ClipWeightRow*)(d_stage + weight_rows_at), n_plain_rows, (srd::PoseBatchItem*)((unsigned char*)s->d_pose_stage.p + lay.items),
                                 (uint32_t*)((unsigned char*)s->d_pose_stage.p + lay.active_index), (float*)((unsigned char*)s->d_pose_stage.p + lay.active_weight),
                                 (uint32_t*)s->d_pose_check.p, st);
        if (n_spline_rows) {
            spline_timer.begin(st);
            if (e == 0)
                e = srk_clip_spline_weights((const srd::ClipSplineWeightRow*)(d_stage + spline_rows_at), n_spline_rows, (srd::PoseBatchItem*)((unsigned char*)s->d_pose_stage.p + lay.items),
                                            (uint32_t*)((unsigned char*)s->d_pose_stage.p + lay.active_index), (float*)((unsigned char*)s->d_pose_stage.p + lay.active_weight),
                                            (uint32_t*)s->d_pose_check.p, st);
            spline_timer.end(st);
        }
        clip_timer.end(st);                                   // the clip kernels
    }
    pose_timer.begin(st);
    if (e == 0) e = srk_pose_batch(d_rows, d_table, n_blocks, (const SrTransform*)(d_stage + lay.matrices), (const uint32_t*)(d_stage + lay.active_index),
                                   (const float*)(d_stage + lay.active_weight), (SrVertex*)s->d_pose_scratch.p, (uint32_t*)s->d_pose_check.p, st);
    if (e == 0) e = (int)hipMemcpyAsync(bad.data(), s->d_pose_check.p, 4 * n_check, hipMemcpyDeviceToHost, st);
    pose_timer.end(st);
    if (e == 0) e = (int)hipStreamSynchronize(st);
    if (e != 0) return fail(SR_ERR_HIP, who + (batch ? ": the posing kernel failed: " : items[0].weights ? ": a posing kernel failed: " : ": the skinning kernel failed: ") +
                                        hipGetErrorString((hipError_t)e));
    info.launches = 1; info.read_backs = 1; info.pose_ms = pose_timer.ms();
    const uint32_t weight_launches = (n_plain_rows ? 1u : 0u) + (n_spline_rows ? 1u : 0u);
    if (feed) {                                               // what the read-outs find, and the figures of a call that reached the device
        s->actor_records.clear();
        for (uint32_t a = 0; a < n_actors; a++)
            s->actor_records.push_back(SrScene::ActorRecord{lay.matrices + sizeof(SrTransform) * (uint64_t)feed->matrix_base(a), feed->actor_joints[a], feed->node_base(a), feed->actor_nodes[a]});
        s->item_active_records.clear();
        for (uint32_t i = 0; i < n_items; i++) {
            n_active[i] = clip_weighted(i) ? std::min(bad[2 * (size_t)n_items + n_actors + feed->item_weight_row[i]], feed->item_clip_targets[i]) : n_active[i];   // the count that came back
            s->item_active_records.push_back(SrScene::ItemActiveRecord{lay.items + sizeof(srd::PoseBatchItem) * (uint64_t)i, lay.active_index + 4 * (uint64_t)rows[i].active_base,
                                                                       lay.active_weight + 4 * (uint64_t)rows[i].active_base,
                                                                       clip_weighted(i) ? feed->item_clip_targets[i] : morph_stage(i) ? n_active[i] : 0u});
        }
        s->actor_stage_current = true; s->actor_nodes_kept = keep_nodes; s->actor_sources_kept = keep_sources;
        s->actor_layers_kept = keep_layers;
        s->actor_layer_records = feed->layer_records;
        if (feed->layered) {
            s->layer_info = feed->layer_info; s->layer_info.layer_table_bytes = sizeof(srd::ClipLayerRow) * (uint64_t)feed->layer_rows.size();
            s->layer_weights_info = feed->layer_weights_info;
            s->layer_weights_info.table_bytes = sizeof(srd::ClipLayerWeightRow) * (uint64_t)feed->layer_weight_rows.size() + sizeof(srd::ClipLayerWeightEntry) * (uint64_t)feed->layer_weight_entries.size();
            s->layer_weights_info.weights_ms = feed->layer_weight_rows.empty() ? 0.0 : layer_weights_timer.ms();
        }
        SrActorPoseInfo& ai = *feed->info;
        ai = SrActorPoseInfo{n_actors, n_items, feed->n_nodes, feed->n_channels, upload_bytes, 2u + weight_launches, 1, ai.calls + 1, 0xFFFFFFFFu, 0xFFFFFFFFu, n_weight_items, clip_timer.ms(), info.pose_ms, 0.0, 0.0};
        s->spline_info = SrSplinePoseInfo{n_spline_rows, feed->layer_weights ? 0u : n_plain_rows, feed->n_cubic_channels, n_spline_rows ? spline_timer.ms() : 0.0, 0};
        for (uint32_t a = 0; a < n_actors && ai.refused_actor == 0xFFFFFFFFu; a++) if (bad[2 * (size_t)n_items + a] != 0xFFFFFFFFu) ai.refused_actor = a;
        if (ai.refused_actor != 0xFFFFFFFFu) {                // a singular mesh-node transform: nothing has changed but the scratch
            s->pose_batch_keys.clear(); s->pose_batch_vertex_base.clear();
            ai.host_ms = ms_between(t0, std::chrono::steady_clock::now());
            return fail(SR_ERR_UNSUPPORTED, who + ": actor " + std::to_string(ai.refused_actor) + ": gltf: the transform of the skinned mesh's node is singular");
        }
    }
    // all or nothing: the lowest item with a bad vertex refuses the call
    for (uint32_t i = 0; i < n_items; i++) {
        const uint32_t bm = bad[2 * (size_t)i], bs = bad[2 * (size_t)i + 1];
        if (std::min(bm, bs) < counts[i] && info.refused_item == 0xFFFFFFFFu) { info.refused_item = i; info.refused_vertex = std::min(bm, bs); }
    }
    if (info.refused_item != 0xFFFFFFFFu) {
        for (uint32_t i = 0; i < n_items; i++) {                  // the two rules of the comment above
            SrScene::MeshState& ms = s->mesh_state[slots[i]];
            const uint32_t bm = bad[2 * (size_t)i], bs = bad[2 * (size_t)i + 1];
            if (bm < counts[i] || (!batch && items[i].weights)) ms.morph.first_bad = bm < counts[i] ? bm : 0xFFFFFFFFu;
            if (bs < counts[i] || (!batch && skin_stage(i))) ms.skin.first_bad = bs < counts[i] ? bs : 0xFFFFFFFFu;
            if (!batch && items[i].weights) ms.morph.n_active = n_active[i];
        }
        s->pose_batch_keys.clear(); s->pose_batch_vertex_base.clear();      // the scratch holds a refused call
        info.host_ms = ms_between(t0, std::chrono::steady_clock::now());
        *out = info;
        if (feed) { feed->info->refused_item = info.refused_item; feed->info->host_ms = info.host_ms; }
        fail_non_finite_vertex(info.refused_vertex);
        return fail(SR_ERR_INVALID_ARG, prefix(info.refused_item) + g_last_error);
    }
    const auto t1 = std::chrono::steady_clock::now();
    s->pose_batch_keys.clear(); s->pose_batch_vertex_base.clear();
    HIP_TRY(hipDeviceSynchronize());                          // frames in flight read the old vertices
    scatter_timer.begin(nullptr);
    e = srk_pose_batch_scatter(d_rows, d_table, n_blocks, (const SrVertex*)s->d_pose_scratch.p, nullptr);
    scatter_timer.end(nullptr);
    if (e == 0) e = (int)hipStreamSynchronize(nullptr);
    if (e != 0) return fail(SR_ERR_HIP, who + ": the scatter kernel failed: " + hipGetErrorString((hipError_t)e));
    info.launches = 2; info.scatter_ms = scatter_timer.ms();
    const auto t2 = std::chrono::steady_clock::now();
    for (uint32_t i = 0; i < n_items; i++) {                   // the tail of finish_device_update, item by item
        const uint32_t slot = slots[i];
        SrScene::MeshState& ms = s->mesh_state[slot];
        // check_ms 0.0: the check is part of the posing kernel, whose time is SrMeshMorphInfo.morph_ms or SrMeshSkinInfo.skin_ms
        if ((rc = device_vertices_taken(s, slot, info.scatter_ms)) != SR_OK) return rc;
        s->meshes[slot].check_ms = 0.0;
        mesh_vertices_changed(s, slot);
        if (morph_stage(i)) { ms.morph.first_bad = 0xFFFFFFFFu; ms.morph.n_active = n_active[i]; ms.morph.morph_ms = info.pose_ms; ms.morph.posed++; }
        if (skin_stage(i)) { ms.skin.first_bad = 0xFFFFFFFFu; ms.skin.skin_ms = morph_stage(i) ? 0.0 : info.pose_ms; ms.skin.skinned++; }
        s->pose_batch_keys.push_back(items[i].key); s->pose_batch_vertex_base.push_back(vertex_base[i]);
    }
    note_update_times(s, t0, t1, t2);
    info.host_ms = ms_between(t0, std::chrono::steady_clock::now());
    *out = info;
    if (feed) { feed->info->launches = 3 + weight_launches; feed->info->scatter_ms = info.scatter_ms; feed->info->host_ms = info.host_ms; }
    return SR_OK;
}

// A single call is a batch of one item whose figures are dropped: sr_scene_pose_batch_info reads as before it.
int pose_one(SrScene* s, const SrPoseItem& item, void* stream) {
    SrPoseBatchInfo dropped{};
    return pose_items(s, &item, 1, stream, false, &dropped);
}

}  // namespace

int sr_scene_skin_mesh(SrScene* s, uint64_t key, const SrTransform* joint_matrices, uint32_t n_joints, void* stream) {
    if (!s || !joint_matrices) return fail(SR_ERR_INVALID_ARG, "skin_mesh: null argument");
    return pose_one(s, SrPoseItem{key, nullptr, joint_matrices, 0, n_joints}, stream);
}

// The one per-frame call of a mesh with a morph, a skin or both; without weights it is sr_scene_skin_mesh.
int sr_scene_pose_mesh(SrScene* s, uint64_t key, const float* weights, uint32_t n_targets, const SrTransform* joint_matrices, uint32_t n_joints, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "pose_mesh: null argument (the scene)");
    return pose_one(s, SrPoseItem{key, weights, joint_matrices, n_targets, n_joints}, stream);
}

int sr_scene_pose_meshes(SrScene* s, const SrPoseItem* items, uint32_t n_items, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "pose_meshes: null argument (the scene)");
    if (n_items == 0) return SR_OK;
    if (!items) return fail(SR_ERR_INVALID_ARG, "pose_meshes: null argument (items, with n_items > 0)");
    return pose_items(s, items, n_items, stream, true, &s->pose_info);
}

int sr_scene_pose_batch_info(const SrScene* s, SrPoseBatchInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_pose_batch_info: null argument");
    *out = s->pose_info;
    return SR_OK;
}

// ---- clips on the device ---------------------------------------------------------------------------------------------------------
int sr_scene_attach_clip(SrScene* s, const SrClip* clip, uint32_t* clip_id) {
    if (!s || !clip || !clip_id) return fail(SR_ERR_INVALID_ARG, "attach_clip: null argument");
    if (s->next_clip_id == 0xFFFFFFFFu) return fail(SR_ERR_UNSUPPORTED, "attach_clip: the scene has handed out 2^32 - 2 clip ids");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    SrScene::AttachedClip a;
    a.host = *clip;
    if ((rc = a.d_block.upload(clip->block.data(), 4 * clip->block.size())) != SR_OK) return rc;
    *clip_id = s->next_clip_id++;
    s->clips.emplace(*clip_id, std::move(a));
    return SR_OK;
}

int sr_scene_detach_clip(SrScene* s, uint32_t clip_id) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "detach_clip: null argument (the scene)");
    const auto it = s->clips.find(clip_id);
    if (it == s->clips.end()) return fail(SR_ERR_INVALID_ARG, "detach_clip: no clip is attached under this id");
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());                          // a clip kernel in flight reads the block
    s->clips.erase(it);
    return SR_OK;
}

// sr_scene_pose_meshes with the joint matrices named rather than given: the actors and what they name are checked here, on the
// host; the rest is pose_items, which takes an actor-driven item's matrices from the slice clip_pose_kernel writes. An item may
// name a morph set of its actor's clip as well (SR_ACTOR_CLIP_WEIGHTS): the set is looked up and checked here, and pose_items has
// clip_weights_kernel write the item's active list on the device.
int sr_scene_pose_actors(SrScene* s, const SrClipActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items, SrTransform* d_instance_transforms,
                         uint32_t flags, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "pose_actors: null argument (the scene)");
    if (flags & ~SR_ACTORS_KEEP_NODES) return fail(SR_ERR_INVALID_ARG, "pose_actors: unknown flag bits (SR_ACTORS_KEEP_NODES is the flag)");
    if (n_actors == 0 && n_items == 0) return SR_OK;
    if ((n_actors && !actors) || (n_items && !items)) return fail(SR_ERR_INVALID_ARG, "pose_actors: null argument (actors or items, with a count > 0)");
    if (((uintptr_t)d_instance_transforms & 15u) != 0) return fail(SR_ERR_INVALID_ARG, "pose_actors: the instance transforms are not 16-byte aligned");
    ActorFeed feed;
    feed.n_actors = n_actors; feed.flags = flags; feed.d_instance_transforms = d_instance_transforms; feed.info = &s->actor_info;
    std::vector<const SrScene::AttachedClip*> clip_of(n_actors);
    std::vector<uint32_t> first_matrix(n_actors);
    for (uint32_t a = 0; a < n_actors; a++) {
        const SrClipActor& ac = actors[a];
        const auto prefix = [a](const char* text) { return "pose_actors: actor " + std::to_string(a) + ": " + text; };
        const auto it = s->clips.find(ac.clip_id);
        if (it == s->clips.end()) return fail(SR_ERR_INVALID_ARG, prefix("no clip is attached under this id"));
        const SrClip& clip = it->second.host;
        const srd::ClipHeader& h = clip.header();
        if (clip.animation >= 0 && !std::isfinite(ac.time_seconds)) return fail(SR_ERR_INVALID_ARG, prefix("gltf: the time of a pose must be finite"));
        if (!d_instance_transforms && (ac.instance_rows || ac.instance_base)) return fail(SR_ERR_INVALID_ARG, prefix("instance rows or an instance base given without device instance transforms"));
        for (int c = 0; ac.placement && c < 12; c++)
            if (!std::isfinite(ac.placement->m[c])) return fail(SR_ERR_INVALID_ARG, prefix("the placement has a component that is not finite"));
        if (!ac.instance_rows && (uint64_t)ac.instance_base + h.n_instances > 0xFFFFFFFFull) return fail(SR_ERR_INVALID_ARG, prefix("the instance base plus the clip's instances passes 2^32 rows"));
        srd::ClipActorRow row{};
        row.clip = it->second.d_block.p; row.time_seconds = ac.time_seconds;
        row.flags = (ac.placement ? 1u : 0u) | (ac.instance_rows ? 2u : 0u);
        row.matrix_base = (uint32_t)feed.n_matrices; row.instance_base = ac.instance_base; row.rows_base = (uint32_t)feed.instance_rows.size();
        row.node_base = (uint32_t)feed.n_nodes;
        if (ac.placement) memcpy(row.placement, ac.placement->m, 48);
        if (ac.instance_rows) feed.instance_rows.insert(feed.instance_rows.end(), ac.instance_rows, ac.instance_rows + h.n_instances);
        feed.rows.push_back(row);
        feed.actor_joints.push_back(h.n_joints); feed.actor_nodes.push_back(h.n_nodes);
        clip_of[a] = &it->second; first_matrix[a] = (uint32_t)feed.n_matrices;
        feed.n_matrices += h.n_joints; feed.n_nodes += h.n_nodes; feed.n_channels += h.n_channels;
        feed.count_cubic_channels(clip);
        if (feed.n_matrices >= (1ull << 32) || feed.n_nodes >= (1ull << 32) || feed.instance_rows.size() >= (1ull << 32)) return fail(SR_ERR_UNSUPPORTED, "pose_actors: the call holds 2^32 joint matrices, nodes or instance rows or more");
    }
    std::vector<SrPoseItem> pose(n_items);
    feed.item_matrix.assign(n_items, 0xFFFFFFFFu);
    feed.item_weight_row.assign(n_items, 0xFFFFFFFFu); feed.item_clip_targets.assign(n_items, 0u);
    feed.item_row_at.assign(n_items, 0u); feed.item_spline.assign(n_items, 0);
    for (uint32_t i = 0; i < n_items; i++) {
        const SrActorPoseItem& it = items[i];
        const auto prefix = [i]() { return "pose_actors: item " + std::to_string(i) + ": "; };
        pose[i] = SrPoseItem{it.key, it.weights, nullptr, it.n_targets, 0};
        if (it.morph && it.weights) return fail(SR_ERR_INVALID_ARG, prefix() + "host weights given together with SR_ACTOR_CLIP_WEIGHTS (one source of weights at most)");
        if (it.skin == SR_ACTOR_NO_SKIN && !it.morph) continue;
        if (it.actor >= n_actors) return fail(SR_ERR_INVALID_ARG, prefix() + "actor " + std::to_string(it.actor) + " named, the call has " + std::to_string(n_actors) + " actors");
        if (it.morph) {                                          // the weights of a morph set of the actor's clip, at the actor's time
            const SrClip& clip = clip_of[it.actor]->host;
            const uint32_t blas = it.morph - 1;
            const int k = clip.find_morph_set(blas);
            if (k < 0) return fail(SR_ERR_INVALID_ARG, prefix() + "the weights of blas " + std::to_string(blas) + " named, the actor's clip has no morph set for it");
            const srd::ClipMorphSet& set = clip.morph_sets()[k];
            if (set.state == srd::kClipMorphUnavailable) return fail((int32_t)set.status, prefix() + clip.morph_errors[k]);
            const bool spline = set.n_keys && set.interpolation == srd::kClipCubic;
            feed.add_weight_item(i, set.n_targets, spline);
            if (spline) {
                srd::ClipSplineWeightRow row{};
                row.clip_a = clip_of[it.actor]->d_block.p; row.time_a = actors[it.actor].time_seconds; row.set_a = (uint32_t)k;
                feed.spline_rows.push_back(row);
            } else {
                srd::ClipWeightRow row{};
                row.clip = clip_of[it.actor]->d_block.p; row.time_seconds = actors[it.actor].time_seconds; row.set = (uint32_t)k;
                feed.weight_rows.push_back(row);
            }
        }
        if (it.skin == SR_ACTOR_NO_SKIN) continue;
        uint32_t first = 0, n_joints = 0;
        if (sr_clip_skin(&clip_of[it.actor]->host, it.skin, &first, &n_joints) != SR_OK) return fail(SR_ERR_INVALID_ARG, prefix() + "skin " + std::to_string(it.skin) + " named, no instanced mesh of the actor's clip wears it");
        pose[i].n_joints = n_joints;
        feed.item_matrix[i] = first_matrix[it.actor] + first;
    }
    SrPoseBatchInfo dropped{};                                // sr_scene_pose_batch_info reads as before the call
    return pose_items(s, pose.data(), n_items, stream, true, &dropped, &feed);
}

// sr_scene_pose_actors for actors that cross-fade between two attached clips: the same checks, for both clips, and the pair's
// compatibility (each pair of ids is compared once a call); the rest is pose_items with a blended feed.
static_assert(sizeof(SrClipBlendActor) == 48, "the header states this size");
int sr_scene_pose_actors_blended(SrScene* s, const SrClipBlendActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                 SrTransform* d_instance_transforms, uint32_t flags, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "pose_actors_blended: null argument (the scene)");
    if (flags & ~(SR_ACTORS_KEEP_NODES | SR_ACTORS_KEEP_SOURCES)) return fail(SR_ERR_INVALID_ARG, "pose_actors_blended: unknown flag bits (SR_ACTORS_KEEP_NODES and SR_ACTORS_KEEP_SOURCES are the flags)");
    if (n_actors == 0 && n_items == 0) return SR_OK;
    if ((n_actors && !actors) || (n_items && !items)) return fail(SR_ERR_INVALID_ARG, "pose_actors_blended: null argument (actors or items, with a count > 0)");
    if (((uintptr_t)d_instance_transforms & 15u) != 0) return fail(SR_ERR_INVALID_ARG, "pose_actors_blended: the instance transforms are not 16-byte aligned");
    ActorFeed feed;
    feed.n_actors = n_actors; feed.flags = flags; feed.d_instance_transforms = d_instance_transforms; feed.info = &s->actor_info; feed.blended = true;
    std::vector<const SrScene::AttachedClip*> clip_a(n_actors), clip_b(n_actors);
    std::vector<uint32_t> first_matrix(n_actors);
    std::set<std::pair<uint32_t, uint32_t>> compatible;
    for (uint32_t a = 0; a < n_actors; a++) {
        const SrClipBlendActor& ac = actors[a];
        const auto prefix = [a](const std::string& text) { return "pose_actors_blended: actor " + std::to_string(a) + ": " + text; };
        const auto ia = s->clips.find(ac.clip_id), ib = s->clips.find(ac.clip_id_b);
        if (ia == s->clips.end() || ib == s->clips.end()) return fail(SR_ERR_INVALID_ARG, prefix("no clip is attached under this id"));
        const SrClip& clip = ia->second.host;
        const SrClip& other = ib->second.host;
        const srd::ClipHeader& h = clip.header();
        if ((clip.animation >= 0 && !std::isfinite(ac.time_seconds)) || (other.animation >= 0 && !std::isfinite(ac.time_seconds_b)))
            return fail(SR_ERR_INVALID_ARG, prefix("gltf: the time of a pose must be finite"));
        if (!(ac.weight >= 0.0f && ac.weight <= 1.0f)) return fail(SR_ERR_INVALID_ARG, prefix("the weight is not in [0, 1]"));
        if (!d_instance_transforms && (ac.instance_rows || ac.instance_base)) return fail(SR_ERR_INVALID_ARG, prefix("instance rows or an instance base given without device instance transforms"));
        for (int c = 0; ac.placement && c < 12; c++)
            if (!std::isfinite(ac.placement->m[c])) return fail(SR_ERR_INVALID_ARG, prefix("the placement has a component that is not finite"));
        if (!ac.instance_rows && (uint64_t)ac.instance_base + h.n_instances > 0xFFFFFFFFull) return fail(SR_ERR_INVALID_ARG, prefix("the instance base plus the clip's instances passes 2^32 rows"));
        if (ac.clip_id != ac.clip_id_b && !compatible.count({ac.clip_id, ac.clip_id_b})) {
            const int rc = sr_clip_blend_compatible(&clip, &other);
            if (rc != SR_OK) return fail(rc, prefix(g_last_error));
            compatible.insert({ac.clip_id, ac.clip_id_b});
        }
        srd::ClipBlendActorRow row{};
        row.clip_a = ia->second.d_block.p; row.clip_b = ib->second.d_block.p;
        row.time_a = ac.time_seconds; row.time_b = ac.time_seconds_b; row.weight = ac.weight;
        row.flags = (ac.placement ? 1u : 0u) | (ac.instance_rows ? 2u : 0u);
        row.matrix_base = (uint32_t)feed.n_matrices; row.instance_base = ac.instance_base; row.rows_base = (uint32_t)feed.instance_rows.size();
        row.node_base = (uint32_t)feed.n_nodes;
        if (ac.placement) memcpy(row.placement, ac.placement->m, 48);
        if (ac.instance_rows) feed.instance_rows.insert(feed.instance_rows.end(), ac.instance_rows, ac.instance_rows + h.n_instances);
        feed.blend_rows.push_back(row);
        feed.actor_joints.push_back(h.n_joints); feed.actor_nodes.push_back(h.n_nodes);
        clip_a[a] = &ia->second; clip_b[a] = &ib->second; first_matrix[a] = (uint32_t)feed.n_matrices;
        feed.n_matrices += h.n_joints; feed.n_nodes += h.n_nodes; feed.n_channels += (uint64_t)h.n_channels + other.header().n_channels;
        feed.count_cubic_channels(clip); feed.count_cubic_channels(other);
        if (feed.n_matrices >= (1ull << 32) || feed.n_nodes >= (1ull << 32) || feed.instance_rows.size() >= (1ull << 32))
            return fail(SR_ERR_UNSUPPORTED, "pose_actors_blended: the call holds 2^32 joint matrices, nodes or instance rows or more");
    }
    std::vector<SrPoseItem> pose(n_items);
    feed.item_matrix.assign(n_items, 0xFFFFFFFFu);
    feed.item_weight_row.assign(n_items, 0xFFFFFFFFu); feed.item_clip_targets.assign(n_items, 0u);
    feed.item_row_at.assign(n_items, 0u); feed.item_spline.assign(n_items, 0);
    for (uint32_t i = 0; i < n_items; i++) {
        const SrActorPoseItem& it = items[i];
        const auto prefix = [i]() { return "pose_actors_blended: item " + std::to_string(i) + ": "; };
        pose[i] = SrPoseItem{it.key, it.weights, nullptr, it.n_targets, 0};
        if (it.morph && it.weights) return fail(SR_ERR_INVALID_ARG, prefix() + "host weights given together with SR_ACTOR_CLIP_WEIGHTS (one source of weights at most)");
        if (it.skin == SR_ACTOR_NO_SKIN && !it.morph) continue;
        if (it.actor >= n_actors) return fail(SR_ERR_INVALID_ARG, prefix() + "actor " + std::to_string(it.actor) + " named, the call has " + std::to_string(n_actors) + " actors");
        if (it.morph) {                                          // the blended weights of a morph set both clips have, each at its own time
            const uint32_t blas = it.morph - 1;
            int k[2];
            for (int side = 0; side < 2; side++) {
                const SrClip& clip = (side ? clip_b : clip_a)[it.actor]->host;
                k[side] = clip.find_morph_set(blas);
                if (k[side] < 0) return fail(SR_ERR_INVALID_ARG, prefix() + "the weights of blas " + std::to_string(blas) + " named, the actor's clip has no morph set for it");
                if (clip.morph_sets()[k[side]].state == srd::kClipMorphUnavailable) return fail((int32_t)clip.morph_sets()[k[side]].status, prefix() + clip.morph_errors[k[side]]);
            }
            const uint32_t n_targets = clip_a[it.actor]->host.morph_sets()[k[0]].n_targets;
            if (n_targets != clip_b[it.actor]->host.morph_sets()[k[1]].n_targets)
                return fail(SR_ERR_INVALID_ARG, prefix() + "the morph sets of blas " + std::to_string(blas) + " have another number of targets in the actor's two clips");
            const SrClipBlendActor& ac = actors[it.actor];
            bool spline = false;                                 // a cubic set in at least one source
            for (int side = 0; side < 2; side++) {
                const srd::ClipMorphSet& set = (side ? clip_b : clip_a)[it.actor]->host.morph_sets()[k[side]];
                spline = spline || (set.n_keys && set.interpolation == srd::kClipCubic);
            }
            feed.add_weight_item(i, n_targets, spline);
            if (spline) {
                srd::ClipSplineWeightRow row{};
                row.clip_a = clip_a[it.actor]->d_block.p; row.clip_b = clip_b[it.actor]->d_block.p;
                row.time_a = ac.time_seconds; row.time_b = ac.time_seconds_b; row.weight = ac.weight;
                row.set_a = (uint32_t)k[0]; row.set_b = (uint32_t)k[1];
                feed.spline_rows.push_back(row);
            } else {
                srd::ClipBlendWeightRow row{};
                row.clip_a = clip_a[it.actor]->d_block.p; row.clip_b = clip_b[it.actor]->d_block.p;
                row.time_a = ac.time_seconds; row.time_b = ac.time_seconds_b; row.weight = ac.weight;
                row.set_a = (uint32_t)k[0]; row.set_b = (uint32_t)k[1];
                feed.blend_weight_rows.push_back(row);
            }
        }
        if (it.skin == SR_ACTOR_NO_SKIN) continue;
        uint32_t first = 0, n_joints = 0;
        if (sr_clip_skin(&clip_a[it.actor]->host, it.skin, &first, &n_joints) != SR_OK) return fail(SR_ERR_INVALID_ARG, prefix() + "skin " + std::to_string(it.skin) + " named, no instanced mesh of the actor's clip wears it");
        pose[i].n_joints = n_joints;
        feed.item_matrix[i] = first_matrix[it.actor] + first;
    }
    SrPoseBatchInfo dropped{};                                // sr_scene_pose_batch_info reads as before the call
    return pose_items(s, pose.data(), n_items, stream, true, &dropped, &feed);
}

int sr_scene_read_actor_sources(const SrScene* s, uint32_t actor, SrNodeTrs* trs_a, SrNodeTrs* trs_b) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "read_actor_sources: null argument (the scene)");
    if (!s->actor_sources_kept) return fail(SR_ERR_STATE, "read_actor_sources: the last call kept no sources (sr_scene_pose_actors_blended with SR_ACTORS_KEEP_SOURCES)");
    if (actor >= s->actor_records.size()) return fail(SR_ERR_INVALID_ARG, "read_actor_sources: actor index out of range");
    const SrScene::ActorRecord& r = s->actor_records[actor];
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (trs_a && r.n_nodes) HIP_TRY(hipMemcpy(trs_a, (const SrNodeTrs*)s->d_actor_source_a.p + r.node_base, sizeof(SrNodeTrs) * (size_t)r.n_nodes, hipMemcpyDeviceToHost));
    if (trs_b && r.n_nodes) HIP_TRY(hipMemcpy(trs_b, (const SrNodeTrs*)s->d_actor_source_b.p + r.node_base, sizeof(SrNodeTrs) * (size_t)r.n_nodes, hipMemcpyDeviceToHost));
    return SR_OK;
}

// ---- layer stacks ------------------------------------------------------------------------------------------------------------------
int sr_scene_attach_node_mask(SrScene* s, const float* weights, uint32_t n_nodes, uint32_t* mask_id) {
    if (!s || !weights || !mask_id) return fail(SR_ERR_INVALID_ARG, "attach_node_mask: null argument");
    if (n_nodes == 0 || n_nodes > SR_CLIP_MAX_NODES) return fail(SR_ERR_INVALID_ARG, "attach_node_mask: the number of nodes is not in [1, SR_CLIP_MAX_NODES]");
    for (uint32_t n = 0; n < n_nodes; n++)
        if (!(weights[n] >= 0.0f && weights[n] <= 1.0f)) return fail(SR_ERR_INVALID_ARG, "attach_node_mask: node " + std::to_string(n) + ": the value is not in [0, 1]");
    if (s->next_mask_id == 0xFFFFFFFFu) return fail(SR_ERR_UNSUPPORTED, "attach_node_mask: the scene has handed out 2^32 - 2 mask ids");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    SrScene::AttachedMask m;
    m.host.assign(weights, weights + n_nodes);
    if ((rc = m.d_weights.upload(weights, 4 * (size_t)n_nodes)) != SR_OK) return rc;
    *mask_id = s->next_mask_id++;
    s->node_masks.emplace(*mask_id, std::move(m));
    return SR_OK;
}

int sr_scene_detach_node_mask(SrScene* s, uint32_t mask_id) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "detach_node_mask: null argument (the scene)");
    const auto it = s->node_masks.find(mask_id);
    if (it == s->node_masks.end()) return fail(SR_ERR_INVALID_ARG, "detach_node_mask: no node mask is attached under this id");
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());                          // a clip kernel in flight reads the mask
    s->node_masks.erase(it);
    return SR_OK;
}

// sr_scene_pose_actors for actors that are stacks of layers: the same checks, for every layer's clip, the stack's own (the rule's
// constraints, the masks, the compatibility with the base clip: each pair of ids is compared once a call); the rest is pose_items
// with a layered feed. Every table the kernel reads beside the layers' channels is the base clip's. A clip-weighted item is the
// plain call's, from the base layer: morph weights are not layered. With SR_ACTORS_LAYER_WEIGHTS such an item is a row for
// clip_layer_weights_kernel instead: every layer's set for the blas is looked up and checked here, the mask's node resolved.
int sr_scene_pose_actors_layered(SrScene* s, const SrClipLayerActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                 SrTransform* d_instance_transforms, uint32_t flags, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "pose_actors_layered: null argument (the scene)");
    if (flags & ~(SR_ACTORS_KEEP_NODES | SR_ACTORS_KEEP_LAYERS | SR_ACTORS_LAYER_WEIGHTS))
        return fail(SR_ERR_INVALID_ARG, "pose_actors_layered: unknown flag bits (SR_ACTORS_KEEP_NODES, SR_ACTORS_KEEP_LAYERS and SR_ACTORS_LAYER_WEIGHTS are the flags)");
    if (n_actors == 0 && n_items == 0) return SR_OK;
    if ((n_actors && !actors) || (n_items && !items)) return fail(SR_ERR_INVALID_ARG, "pose_actors_layered: null argument (actors or items, with a count > 0)");
    if (((uintptr_t)d_instance_transforms & 15u) != 0) return fail(SR_ERR_INVALID_ARG, "pose_actors_layered: the instance transforms are not 16-byte aligned");
    ActorFeed feed;
    feed.n_actors = n_actors; feed.flags = flags; feed.d_instance_transforms = d_instance_transforms; feed.info = &s->actor_info; feed.layered = true;
    feed.layer_weights = (flags & SR_ACTORS_LAYER_WEIGHTS) != 0;
    struct StackLayer { const SrClip* clip; bool masked; };   // what a layer-weight row asks of a layer: beside feed.layer_rows, with the flag only
    std::vector<StackLayer> stack;
    std::vector<const SrScene::AttachedClip*> base_of(n_actors);
    std::vector<uint32_t> first_matrix(n_actors);
    std::set<std::pair<uint32_t, uint32_t>> compatible;
    for (uint32_t a = 0; a < n_actors; a++) {
        const SrClipLayerActor& ac = actors[a];
        const auto prefix = [a](const std::string& text) { return "pose_actors_layered: actor " + std::to_string(a) + ": " + text; };
        if (ac.n_layers == 0 || ac.n_layers > SR_CLIP_MAX_LAYERS) return fail(SR_ERR_INVALID_ARG, prefix("the number of layers is not in [1, SR_CLIP_MAX_LAYERS]"));
        if (!ac.layers) return fail(SR_ERR_INVALID_ARG, prefix("null argument (the layers)"));
        SrScene::ActorLayerRecord record{feed.n_layer_nodes, ac.n_layers, 0u};
        const SrScene::AttachedClip* base = nullptr;
        for (uint32_t l = 0; l < ac.n_layers; l++) {
            const SrClipLayer& ly = ac.layers[l];
            const auto layer = [a, l](const std::string& text) { return "pose_actors_layered: actor " + std::to_string(a) + ": layer " + std::to_string(l) + ": " + text; };
            const auto ic = s->clips.find(ly.clip_id);
            if (ic == s->clips.end()) return fail(SR_ERR_INVALID_ARG, layer("no clip is attached under this id"));
            const SrClip& clip = ic->second.host;
            if (l == 0) base = &ic->second;
            if (!(ly.weight >= 0.0f && ly.weight <= 1.0f)) return fail(SR_ERR_INVALID_ARG, layer("the weight is not in [0, 1]"));
            if (ly.mode != SR_LAYER_OVERRIDE && ly.mode != SR_LAYER_ADDITIVE) return fail(SR_ERR_INVALID_ARG, layer("unknown mode (SR_LAYER_OVERRIDE and SR_LAYER_ADDITIVE are the modes)"));
            const bool additive = ly.mode == SR_LAYER_ADDITIVE;
            if (l == 0 && (additive || ly.mask_id != SR_LAYER_NO_MASK || ly.weight != 1.0f))
                return fail(SR_ERR_INVALID_ARG, layer("the base layer must be SR_LAYER_OVERRIDE, without a mask, at weight 1"));
            if (clip.animation >= 0 && (!std::isfinite(ly.time_seconds) || (additive && !std::isfinite(ly.ref_time_seconds))))
                return fail(SR_ERR_INVALID_ARG, layer("gltf: the time of a pose must be finite"));
            if (l && ly.clip_id != ac.layers[0].clip_id && !compatible.count({ac.layers[0].clip_id, ly.clip_id})) {
                const int rc = sr_clip_blend_compatible(&base->host, &clip);
                if (rc != SR_OK) return fail(rc, layer(g_last_error));
                compatible.insert({ac.layers[0].clip_id, ly.clip_id});
            }
            const float* d_mask = nullptr;
            if (feed.layer_weights) stack.push_back(StackLayer{&clip, ly.mask_id != SR_LAYER_NO_MASK});
            if (ly.mask_id != SR_LAYER_NO_MASK) {
                const auto im = s->node_masks.find(ly.mask_id);
                if (im == s->node_masks.end()) return fail(SR_ERR_INVALID_ARG, layer("no node mask is attached under this id"));
                if (im->second.host.size() != clip.header().n_nodes)
                    return fail(SR_ERR_INVALID_ARG, layer("the mask has " + std::to_string(im->second.host.size()) + " values, the clip " + std::to_string(clip.header().n_nodes) + " nodes"));
                d_mask = (const float*)im->second.d_weights.p;
                feed.layer_info.masked_layers++;
            }
            srd::ClipLayerRow row{};
            row.clip = ic->second.d_block.p; row.mask = d_mask;
            row.time_seconds = ly.time_seconds; row.ref_time_seconds = additive ? ly.ref_time_seconds : 0.0f; row.weight = ly.weight; row.mode = ly.mode;
            feed.layer_rows.push_back(row);
            feed.n_channels += (uint64_t)clip.header().n_channels * (additive ? 2u : 1u);
            feed.count_cubic_channels(clip);
            if (additive) { feed.count_cubic_channels(clip); feed.layer_info.additive_layers++; record.additive |= 1u << l; }
        }
        const srd::ClipHeader& h = base->host.header();
        if (!d_instance_transforms && (ac.instance_rows || ac.instance_base)) return fail(SR_ERR_INVALID_ARG, prefix("instance rows or an instance base given without device instance transforms"));
        for (int c = 0; ac.placement && c < 12; c++)
            if (!std::isfinite(ac.placement->m[c])) return fail(SR_ERR_INVALID_ARG, prefix("the placement has a component that is not finite"));
        if (!ac.instance_rows && (uint64_t)ac.instance_base + h.n_instances > 0xFFFFFFFFull) return fail(SR_ERR_INVALID_ARG, prefix("the instance base plus the clip's instances passes 2^32 rows"));
        srd::ClipLayerActorRow row{};
        row.first_layer = (uint32_t)(feed.layer_rows.size() - ac.n_layers); row.n_layers = ac.n_layers;
        row.flags = (ac.placement ? 1u : 0u) | (ac.instance_rows ? 2u : 0u);
        row.matrix_base = (uint32_t)feed.n_matrices; row.instance_base = ac.instance_base; row.rows_base = (uint32_t)feed.instance_rows.size();
        row.node_base = (uint32_t)feed.n_nodes; row.layer_node_base = (uint32_t)feed.n_layer_nodes;
        if (ac.placement) memcpy(row.placement, ac.placement->m, 48);
        if (ac.instance_rows) feed.instance_rows.insert(feed.instance_rows.end(), ac.instance_rows, ac.instance_rows + h.n_instances);
        feed.layer_actor_rows.push_back(row);
        feed.layer_records.push_back(record);
        feed.actor_joints.push_back(h.n_joints); feed.actor_nodes.push_back(h.n_nodes);
        base_of[a] = base; first_matrix[a] = (uint32_t)feed.n_matrices;
        feed.n_matrices += h.n_joints; feed.n_nodes += h.n_nodes; feed.n_layer_nodes += (uint64_t)h.n_nodes * ac.n_layers;
        feed.layer_info.layers += ac.n_layers; feed.layer_info.max_layers = std::max(feed.layer_info.max_layers, ac.n_layers);
        if (feed.n_matrices >= (1ull << 32) || feed.n_layer_nodes >= (1ull << 32) || feed.instance_rows.size() >= (1ull << 32))
            return fail(SR_ERR_UNSUPPORTED, "pose_actors_layered: the call holds 2^32 joint matrices, layer nodes or instance rows or more");
    }
    std::vector<SrPoseItem> pose(n_items);
    feed.item_matrix.assign(n_items, 0xFFFFFFFFu);
    feed.item_weight_row.assign(n_items, 0xFFFFFFFFu); feed.item_clip_targets.assign(n_items, 0u);
    feed.item_row_at.assign(n_items, 0u); feed.item_spline.assign(n_items, 0);
    for (uint32_t i = 0; i < n_items; i++) {
        const SrActorPoseItem& it = items[i];
        const auto prefix = [i]() { return "pose_actors_layered: item " + std::to_string(i) + ": "; };
        pose[i] = SrPoseItem{it.key, it.weights, nullptr, it.n_targets, 0};
        if (it.morph && it.weights) return fail(SR_ERR_INVALID_ARG, prefix() + "host weights given together with SR_ACTOR_CLIP_WEIGHTS (one source of weights at most)");
        if (it.skin == SR_ACTOR_NO_SKIN && !it.morph) continue;
        if (it.actor >= n_actors) return fail(SR_ERR_INVALID_ARG, prefix() + "actor " + std::to_string(it.actor) + " named, the call has " + std::to_string(n_actors) + " actors");
        if (it.morph && feed.layer_weights) {                    // the stack's weights: every layer's set for the blas, checked here
            const uint32_t blas = it.morph - 1;
            const SrClipLayer* layers = actors[it.actor].layers;
            srd::ClipLayerWeightRow row{};
            row.first_layer = feed.layer_actor_rows[it.actor].first_layer; row.n_layers = feed.layer_actor_rows[it.actor].n_layers;
            row.first_entry = (uint32_t)feed.layer_weight_entries.size();
            uint32_t n_targets = 0;
            for (uint32_t l = 0; l < row.n_layers; l++) {
                const auto layer = [i, l](const std::string& text) { return "pose_actors_layered: item " + std::to_string(i) + ": layer " + std::to_string(l) + ": " + text; };
                const SrClip& clip = *stack[row.first_layer + l].clip;
                const int k = clip.find_morph_set(blas);
                if (k < 0) return fail(SR_ERR_INVALID_ARG, layer("the weights of blas " + std::to_string(blas) + " named, the layer's clip has no morph set for it"));
                const srd::ClipMorphSet& set = clip.morph_sets()[k];
                if (set.state == srd::kClipMorphUnavailable) return fail((int32_t)set.status, layer(clip.morph_errors[k]));
                if (l == 0) {                                    // the base's set against the mesh's attached morph (a mesh without one is pose_items' to refuse)
                    n_targets = set.n_targets;
                    const auto im = s->slots.find(it.key);
                    const uint32_t attached = im == s->slots.end() ? 0u : s->mesh_state[im->second].morph.n_targets;
                    if (attached && attached != n_targets)
                        return fail(SR_ERR_INVALID_ARG, layer("the set has " + std::to_string(n_targets) + " targets, the mesh's morph was attached with " + std::to_string(attached)));
                }
                if (set.n_targets != n_targets)
                    return fail(SR_ERR_INVALID_ARG, layer("the set has " + std::to_string(set.n_targets) + " targets, the base layer's " + std::to_string(n_targets)));
                const bool additive = layers[l].mode == SR_LAYER_ADDITIVE, cubic = set.n_keys && set.interpolation == srd::kClipCubic;
                feed.layer_weights_info.samples += additive ? 2u : 1u;
                feed.layer_weights_info.cubic_samples += cubic ? (additive ? 2u : 1u) : 0u;
                feed.layer_weight_entries.push_back(srd::ClipLayerWeightEntry{(uint32_t)k, stack[row.first_layer + l].masked ? clip.find_node(set.gltf_node) : srd::kClipNoNode, {0u, 0u}});
            }
            if (feed.layer_weight_entries.size() >= (1ull << 32)) return fail(SR_ERR_UNSUPPORTED, "pose_actors_layered: the call holds 2^32 layer-weight entries or more");
            feed.add_weight_item(i, n_targets, false);
            feed.layer_weight_rows.push_back(row);
            feed.layer_weights_info.rows++;
        } else if (it.morph) {                                   // the weights of a morph set of the base layer's clip, at the base layer's time
            const SrClip& clip = base_of[it.actor]->host;
            const float time_seconds = actors[it.actor].layers[0].time_seconds;
            const uint32_t blas = it.morph - 1;
            const int k = clip.find_morph_set(blas);
            if (k < 0) return fail(SR_ERR_INVALID_ARG, prefix() + "the weights of blas " + std::to_string(blas) + " named, the actor's clip has no morph set for it");
            const srd::ClipMorphSet& set = clip.morph_sets()[k];
            if (set.state == srd::kClipMorphUnavailable) return fail((int32_t)set.status, prefix() + clip.morph_errors[k]);
            const bool spline = set.n_keys && set.interpolation == srd::kClipCubic;
            feed.add_weight_item(i, set.n_targets, spline);
            if (spline) {
                srd::ClipSplineWeightRow row{};
                row.clip_a = base_of[it.actor]->d_block.p; row.time_a = time_seconds; row.set_a = (uint32_t)k;
                feed.spline_rows.push_back(row);
            } else {
                srd::ClipWeightRow row{};
                row.clip = base_of[it.actor]->d_block.p; row.time_seconds = time_seconds; row.set = (uint32_t)k;
                feed.weight_rows.push_back(row);
            }
        }
        if (it.skin == SR_ACTOR_NO_SKIN) continue;
        uint32_t first = 0, n_joints = 0;
        if (sr_clip_skin(&base_of[it.actor]->host, it.skin, &first, &n_joints) != SR_OK) return fail(SR_ERR_INVALID_ARG, prefix() + "skin " + std::to_string(it.skin) + " named, no instanced mesh of the actor's clip wears it");
        pose[i].n_joints = n_joints;
        feed.item_matrix[i] = first_matrix[it.actor] + first;
    }
    SrPoseBatchInfo dropped{};                                // sr_scene_pose_batch_info reads as before the call
    return pose_items(s, pose.data(), n_items, stream, true, &dropped, &feed);
}

int sr_scene_layer_weights_info(const SrScene* s, SrLayerWeightsInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_layer_weights_info: null argument");
    *out = s->layer_weights_info;
    return SR_OK;
}

int sr_scene_layer_pose_info(const SrScene* s, SrLayerPoseInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_layer_pose_info: null argument");
    *out = s->layer_info;
    return SR_OK;
}

int sr_scene_read_actor_layer(const SrScene* s, uint32_t actor, uint32_t layer, SrNodeTrs* cur, SrNodeTrs* ref) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "read_actor_layer: null argument (the scene)");
    if (!s->actor_layers_kept) return fail(SR_ERR_STATE, "read_actor_layer: the last call kept no layers (sr_scene_pose_actors_layered with SR_ACTORS_KEEP_LAYERS)");
    if (actor >= s->actor_layer_records.size() || actor >= s->actor_records.size()) return fail(SR_ERR_INVALID_ARG, "read_actor_layer: actor index out of range");
    const SrScene::ActorLayerRecord& lr = s->actor_layer_records[actor];
    if (layer >= lr.n_layers) return fail(SR_ERR_INVALID_ARG, "read_actor_layer: layer index out of range");
    const uint32_t n_nodes = s->actor_records[actor].n_nodes;
    const size_t at = (size_t)lr.layer_base + (size_t)layer * n_nodes;
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (cur && n_nodes) HIP_TRY(hipMemcpy(cur, (const SrNodeTrs*)s->d_actor_layer_cur.p + at, sizeof(SrNodeTrs) * (size_t)n_nodes, hipMemcpyDeviceToHost));
    if (ref && n_nodes && (lr.additive >> layer & 1u)) HIP_TRY(hipMemcpy(ref, (const SrNodeTrs*)s->d_actor_layer_ref.p + at, sizeof(SrNodeTrs) * (size_t)n_nodes, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_scene_actor_pose_info(const SrScene* s, SrActorPoseInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_actor_pose_info: null argument");
    *out = s->actor_info;
    return SR_OK;
}

int sr_scene_spline_pose_info(const SrScene* s, SrSplinePoseInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_spline_pose_info: null argument");
    *out = s->spline_info;
    return SR_OK;
}

int sr_scene_read_actor_nodes(const SrScene* s, uint32_t actor, SrNodeTrs* trs, float* globals16) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "read_actor_nodes: null argument (the scene)");
    if (!s->actor_nodes_kept) return fail(SR_ERR_STATE, "read_actor_nodes: the last sr_scene_pose_actors kept no nodes (SR_ACTORS_KEEP_NODES)");
    if (actor >= s->actor_records.size()) return fail(SR_ERR_INVALID_ARG, "read_actor_nodes: actor index out of range");
    const SrScene::ActorRecord& r = s->actor_records[actor];
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (trs && r.n_nodes) HIP_TRY(hipMemcpy(trs, (const SrNodeTrs*)s->d_actor_trs.p + r.node_base, sizeof(SrNodeTrs) * (size_t)r.n_nodes, hipMemcpyDeviceToHost));
    if (globals16 && r.n_nodes) HIP_TRY(hipMemcpy(globals16, (const float*)s->d_actor_globals.p + 16 * (size_t)r.node_base, 64 * (size_t)r.n_nodes, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_scene_read_actor_matrices(const SrScene* s, uint32_t actor, SrTransform* joint_matrices) {
    if (!s || !joint_matrices) return fail(SR_ERR_INVALID_ARG, "read_actor_matrices: null argument");
    if (!s->actor_stage_current) return fail(SR_ERR_STATE, "read_actor_matrices: the staging block does not hold a sr_scene_pose_actors call");
    if (actor >= s->actor_records.size()) return fail(SR_ERR_INVALID_ARG, "read_actor_matrices: actor index out of range");
    const SrScene::ActorRecord& r = s->actor_records[actor];
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (r.n_joints) HIP_TRY(hipMemcpy(joint_matrices, (const unsigned char*)s->d_pose_stage.p + r.matrix_byte, sizeof(SrTransform) * (size_t)r.n_joints, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_scene_read_item_active(const SrScene* s, uint32_t item, uint32_t* index_out, float* weight_out, uint32_t* n_active) {
    if (!s || !n_active) return fail(SR_ERR_INVALID_ARG, "read_item_active: null argument");
    if (!s->actor_stage_current) return fail(SR_ERR_STATE, "read_item_active: the staging block does not hold a sr_scene_pose_actors call");
    if (item >= s->item_active_records.size()) return fail(SR_ERR_INVALID_ARG, "read_item_active: item index out of range");
    const SrScene::ItemActiveRecord& r = s->item_active_records[item];
    const int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    const unsigned char* stage = (const unsigned char*)s->d_pose_stage.p;
    srd::PoseBatchItem row;
    HIP_TRY(hipMemcpy(&row, stage + r.row_byte, sizeof(row), hipMemcpyDeviceToHost));
    const uint32_t n = (row.stages & srd::kPoseMorph) ? std::min(row.n_active, r.capacity) : 0u;      // never past the item's slice
    if (index_out && n) HIP_TRY(hipMemcpy(index_out, stage + r.index_byte, 4 * (size_t)n, hipMemcpyDeviceToHost));
    if (weight_out && n) HIP_TRY(hipMemcpy(weight_out, stage + r.weight_byte, 4 * (size_t)n, hipMemcpyDeviceToHost));
    *n_active = n;
    return SR_OK;
}

// Attaches (or, with flags == 0, detaches) a mesh's frame, as sr_scene_set_mesh_skin attaches a rig: every buffer is filled before
// the mesh's record changes, so a refusal or a failed allocation leaves an earlier frame in place. The groups come from the host
// copy, which is the device buffer's contents once fetched: the reference records snapshotted below are those same bytes.
int sr_scene_set_mesh_frame(SrScene* s, uint64_t key, uint32_t flags) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "set_mesh_frame: null argument (the scene)");
    uint32_t slot = 0;
    int rc = find_mesh(s, key, "set_mesh_frame", &slot);
    if (rc != SR_OK) return rc;
    if (flags & ~(SR_FRAME_NORMALS | SR_FRAME_TANGENTS)) return fail(SR_ERR_INVALID_ARG, "set_mesh_frame: unknown flag bits (SR_FRAME_NORMALS and SR_FRAME_TANGENTS are the flags)");
    if (flags == SR_FRAME_TANGENTS) return fail(SR_ERR_INVALID_ARG, "set_mesh_frame: SR_FRAME_TANGENTS needs SR_FRAME_NORMALS (the tangent is made orthogonal to the new normal)");
    if ((rc = bind_device(s)) != SR_OK) return rc;
    if (flags == 0) return detach_record(s->mesh_state[slot].frame);
    if ((rc = fetch_host_vertices(s, slot)) != SR_OK) return rc;
    const srh::HostMesh& m = s->meshes[slot];
    srh::MeshFrame f;
    if ((rc = srh::mesh_frame_build(m.vertices.data(), m.n_vertices, m.indices.data(), m.n_indices, false, f, nullptr, "set_mesh_frame")) != SR_OK) return rc;
    SrScene::MeshState::Frame frame;
    if ((rc = frame.d_offsets.upload(f.offsets.data(), 4 * f.offsets.size())) != SR_OK || (rc = frame.d_entries.upload(f.entries.data(), 4 * f.entries.size())) != SR_OK ||
        (rc = frame.d_side.upload(f.side.data(), 4 * f.side.size())) != SR_OK || (rc = frame.d_tri_uv.upload(f.tri_uv.data(), sizeof(srh::FrameTriUv) * f.tri_uv.size())) != SR_OK ||
        (rc = snapshot_vertices(m, frame.d_reference)) != SR_OK) return rc;
    frame.flags = flags; frame.n_groups = f.n_groups; frame.n_entries = (uint32_t)f.entries.size(); frame.max_valence = f.max_valence;
    s->mesh_state[slot].frame = std::move(frame);
    return SR_OK;
}

namespace {

// sr_scene_update_mesh_positions_device and sr_scene_update_mesh_positions (`on_device`: where `positions` lives):
// sr_scene_update_mesh_device with the frame kernels in front. The host form uploads its 12 bytes a vertex on the stream first.
int update_mesh_positions(SrScene* s, uint64_t key, const float* positions, uint32_t n_vertices, void* stream, bool on_device) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t slot = 0;
    int rc = check_mesh_update(s, key, positions, n_vertices, &slot);
    if (rc != SR_OK) return rc;
    srh::HostMesh& m = s->meshes[slot];
    SrScene::MeshState::Frame& frame = s->mesh_state[slot].frame;
    if (frame.flags == 0) return fail(SR_ERR_INVALID_ARG, "update_mesh_positions: the mesh has no frame (sr_scene_set_mesh_frame attaches one)");
    const size_t bytes = 12 * (size_t)n_vertices, record_bytes = sizeof(SrVertex) * (size_t)n_vertices;
    const uintptr_t a = (uintptr_t)positions, own = (uintptr_t)m.d_vertices;
    if (a & 3u) return fail(SR_ERR_INVALID_ARG, "update_mesh_positions: the position pointer is not 4-byte aligned");
    if (on_device && a < own + record_bytes && own < a + bytes) return fail(SR_ERR_INVALID_ARG, "update_mesh_positions: the device positions overlap the mesh's own vertex buffer");
    if ((rc = check_emissive_list(m)) != SR_OK || (rc = bind_device(s)) != SR_OK) return rc;
    if (on_device && !device_range_of_scene(s, positions, bytes))
        return fail(SR_ERR_INVALID_ARG, "update_mesh_positions: the position pointer is not device memory of the scene's device for that many vertices");
    const bool tangents = (frame.flags & SR_FRAME_TANGENTS) != 0;
    const uint32_t n_triangles = m.n_indices / 3;
    if ((rc = s->d_frame_out.reserve(record_bytes)) != SR_OK || (rc = s->d_vertex_check.reserve(16)) != SR_OK ||
        (rc = s->d_frame_faces.reserve(16 * (size_t)n_triangles * (tangents ? 2 : 1))) != SR_OK) return rc;
    if (!on_device && (rc = s->d_frame_positions.reserve(bytes)) != SR_OK) return rc;
    const float* d_positions = on_device ? positions : (const float*)s->d_frame_positions.p;
    hipStream_t st = (hipStream_t)stream;
    uint32_t bad = 0xFFFFFFFFu;
    double ms = 0.0;
    rc = checked_launch(s, st, 1, &bad, &ms, "update_mesh_positions: a frame kernel failed: ",
                        [&] { return on_device ? 0 : (int)hipMemcpyAsync(s->d_frame_positions.p, positions, bytes, hipMemcpyHostToDevice, st); },
                        [&](uint32_t* check) {
                            return srk_mesh_frame((const SrVertex*)frame.d_reference.p, d_positions, (const uint32_t*)m.d_indices, (const srh::FrameTriUv*)frame.d_tri_uv.p,
                                                  (const uint32_t*)frame.d_offsets.p, (const uint32_t*)frame.d_entries.p, (const float*)frame.d_side.p, frame.flags,
                                                  (float4*)s->d_frame_faces.p, (SrVertex*)s->d_frame_out.p, n_vertices, n_triangles, check, st);
                        });
    if (rc != SR_OK) return rc;
    frame.first_bad = bad < n_vertices ? bad : 0xFFFFFFFFu;
    if (bad < n_vertices) return fail_non_finite_vertex(bad);
    // check_ms 0.0: the check is part of the vertex kernel, whose time is SrMeshFrameInfo.frame_ms
    if ((rc = finish_device_update(s, slot, (const SrVertex*)s->d_frame_out.p, s->device, 0.0, t0)) != SR_OK) return rc;
    frame.frame_ms = ms; frame.updates++;
    return SR_OK;
}

}  // namespace

int sr_scene_update_mesh_positions_device(SrScene* s, uint64_t key, const float* d_positions, uint32_t n_vertices, void* stream) {
    return update_mesh_positions(s, key, d_positions, n_vertices, stream, true);
}

int sr_scene_update_mesh_positions(SrScene* s, uint64_t key, const float* positions, uint32_t n_vertices, void* stream) {
    return update_mesh_positions(s, key, positions, n_vertices, stream, false);
}

int sr_scene_mesh_frame_info(const SrScene* s, uint64_t key, SrMeshFrameInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_frame_info: null argument");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_mesh_frame_info", &slot); rc != SR_OK) return rc;
    const SrScene::MeshState::Frame& frame = s->mesh_state[slot].frame;
    memset(out, 0, sizeof(*out));
    out->flags = frame.flags; out->n_groups = frame.n_groups; out->n_entries = frame.n_entries; out->max_valence = frame.max_valence;
    out->updates = frame.updates; out->first_bad = frame.first_bad; out->frame_ms = frame.frame_ms;
    return SR_OK;
}

int sr_scene_mesh_update_info(const SrScene* s, SrMeshUpdateInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_update_info: null argument");
    *out = s->mu_info;
    return SR_OK;
}

int sr_scene_add_image(SrScene* s, const uint8_t* data, uint32_t width, uint32_t height, uint32_t channels, uint32_t* out_image_slot) {
    if (!s || !data || width == 0 || height == 0) return fail(SR_ERR_INVALID_ARG, "Image::new_from_data: null argument or empty extent");
    if (channels < 1 || channels > 4) return fail(SR_ERR_INVALID_ARG, "Image::new_from_data: 1..4 channels of 8 bits are supported");
    if ((uint64_t)width * height >= (1ull << 30)) return fail(SR_ERR_UNSUPPORTED, "Image::new_from_data: image too large");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    const size_t n = (size_t)width * height;
    std::vector<uint32_t> rgba(n);
    for (size_t i = 0; i < n; i++) {       // utils::realign_data (utils.rs:27-43): missing channels are 0x00
        uint32_t p = 0;
        for (uint32_t c = 0; c < channels; c++) p |= (uint32_t)data[i * channels + c] << (8 * c);
        rgba[i] = p;
    }
    SrScene::DeviceImage im;
    im.w = width; im.h = height;
    HIP_TRY(hipMalloc(&im.d_texels, n * 4));
    const hipError_t ce = hipMemcpy(im.d_texels, rgba.data(), n * 4, hipMemcpyHostToDevice);
    if (ce != hipSuccess) { (void)hipFree(im.d_texels); return fail(SR_ERR_HIP, std::string("Image::new_from_data: ") + hipGetErrorString(ce)); }
    uint32_t slot;
    if (!s->free_image_slots.empty()) { slot = s->free_image_slots.back(); s->free_image_slots.pop_back(); s->images[slot] = im; }
    else { slot = (uint32_t)s->images.size(); s->images.push_back(im); }
    if (out_image_slot) *out_image_slot = slot;
    return SR_OK;
}

// ResourceManager::remove drops a group's images with its BLASes (resource_manager.rs:472). The caller must have removed
// (or be about to remove) every mesh whose material names the slot; meshes still naming it are rejected at the next
// sr_scene_set_instances. Waits for the device: a launch in flight may still sample the texels.
int sr_scene_remove_image(SrScene* s, uint32_t image_slot) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_remove_image: scene is null");
    if (image_slot >= s->images.size() || !s->images[image_slot].d_texels) return fail(SR_ERR_INVALID_ARG, "sr_scene_remove_image: no image in this slot");
    for (const auto& m : s->meshes) {
        if (m.n_vertices == 0) continue;
        const uint32_t* tex = &m.material.base_color_image;
        for (int i = 0; i < 10; i += 2)
            if (tex[i] == image_slot) return fail(SR_ERR_STATE, "sr_scene_remove_image: a registered mesh still uses this image (remove the mesh first)");
    }
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(s->images[image_slot].d_texels));
    s->images[image_slot] = SrScene::DeviceImage();
    s->free_image_slots.push_back(image_slot);
    return SR_OK;
}

int sr_scene_add_sampler(SrScene* s, const SrSamplerDesc* d, uint32_t* out_sampler_slot) {
    if (!s || !d) return fail(SR_ERR_INVALID_ARG, "Sampler::new: null argument");
    if (d->min_filter > SR_FILTER_LINEAR || d->mag_filter > SR_FILTER_LINEAR || d->address_mode_u > SR_ADDRESS_CLAMP_TO_EDGE ||
        d->address_mode_v > SR_ADDRESS_CLAMP_TO_EDGE)
        return fail(SR_ERR_INVALID_ARG, "Sampler::new: filter must be NEAREST/LINEAR, address mode REPEAT/MIRRORED_REPEAT/CLAMP_TO_EDGE");
    s->samplers.push_back(*d);
    if (out_sampler_slot) *out_sampler_slot = (uint32_t)s->samplers.size() - 1;
    return SR_OK;
}

namespace {

// Per-instance device tables (closest_hit's WorldToObject / ObjectToWorld, the flatten inputs) and the light table:
// everything that follows the instance transforms without touching the tree.
// The two tables themselves are the host's to fill unless sr_scene_set_instances_device's kernel has written them and the host
// copy of the transforms is still behind (a host copy that was fetched since fills them again, with the same bytes).
int upload_instance_tables(SrScene* s) {
    int rc;
    if (!s->inst.host_stale) {
        const size_t ni = s->fid.instances.size();
        std::vector<srd::DevInstance> dinst(ni ? ni : 1);
        static_assert(sizeof(srd::DevInstance) == 96, "srh::instance_tables_host writes 24 floats per instance");
        srh::instance_tables_host(s->fid.transforms.data(), ni, (float*)dinst.data());
        if (ni == 0) memset(dinst.data(), 0, sizeof(srd::DevInstance));
        std::vector<srd::FlatInstance> flat(dinst.size());
        memset(flat.data(), 0, flat.size() * sizeof(srd::FlatInstance));
        for (size_t i = 0; i < ni; i++) {
            memcpy(flat[i].o2w, s->fid.instances[i].o2w.m, 48);
            flat[i].tri_offset = s->fid.instances[i].tri_offset;
            flat[i].mesh_slot = s->fid.instances[i].mesh_slot;
        }
        if ((rc = s->d_instances.upload(dinst.data(), dinst.size() * sizeof(srd::DevInstance))) != SR_OK) return rc;
        if ((rc = s->d_flat_instances.upload(flat.data(), flat.size() * sizeof(srd::FlatInstance))) != SR_OK) return rc;
    }
    SrLightTableInfo& li = s->lt_info;                        // reset by sr_scene_set_instances: a path that comes here twice adds up
    li.num_lights = (uint32_t)s->fid.emissive_entries.size(); li.arena_entries = (uint32_t)s->emissive_tris.size();
    if (s->lights_on_device) {
        if ((rc = device_light_table(s)) != SR_OK) return rc;
    } else {
        // the one dummy record of an empty arena reads the first transform alone, which a device call brings along
        if (!s->emissive_tris.empty() && (rc = fetch_host_transforms(s, SR_INST_FETCH_HOST_LIGHT_TABLE)) != SR_OK) return rc;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<float> lights;
        srh::light_table(s->fid, s->emissive_table, lights);
        if ((rc = s->d_lights.upload(lights.data(), lights.size() * 4)) != SR_OK) return rc;
        if (s->timing) li.host_ms += ms_between(t0, std::chrono::steady_clock::now());
    }
    s->dev.instances = (const srd::DevInstance*)s->d_instances.p;
    s->dev.lights = (const srd::DevLight*)s->d_lights.p;
    s->dev.num_lights = (uint32_t)s->fid.emissive_entries.size();
    s->dev.n_instances = (uint32_t)s->fid.instances.size();
    return SR_OK;
}

// Per-mesh payload constants, the texture side of the materials and the image table (independent of the tree).
int upload_mesh_tables(SrScene* s, bool* any_textured_out) {
    int rc;
    std::vector<srd::DevMeshConst> mconst(s->meshes.size() ? s->meshes.size() : 1);
    memset(mconst.data(), 0, mconst.size() * sizeof(srd::DevMeshConst));
    for (size_t i = 0; i < s->meshes.size(); i++) {
        if (s->meshes[i].n_vertices == 0) continue;      // freed slot (sr_scene_remove)
        const SrMaterial& m = s->meshes[i].material;
        for (int k = 0; k < 3; k++) mconst[i].emission[k] = m.emissive_factor[k] * m.emissive_factor[3];
        mconst[i].albedo_packed = srh::pack_unorm_4x8(m.base_color_value[0], m.base_color_value[1], m.base_color_value[2], 1.0f);
        mconst[i].material_info = srh::pack_half_2x16(m.roughness_factor, m.metallic_factor);
        mconst[i].transmission_ior_packed = srh::pack_half_2x16(m.transmission_factor, m.ior);
    }
    // texture side: per-mesh factors + resolved slots, per-slot uv/tangent records, the image table. Occlusion
    // textures are carried in SrMaterial but no shader on the path samples them.
    std::vector<srd::DevMeshTex> mtex(mconst.size());
    memset(mtex.data(), 0, mtex.size() * sizeof(srd::DevMeshTex));
    bool any_textured = false;
    auto sampler_code = [&](uint32_t image, uint32_t sampler) -> uint32_t {
        if (image == SR_NULL_TEXTURE) return 0u;
        const SrSamplerDesc& d = s->samplers[sampler];
        return (d.mag_filter & 1u) | (d.address_mode_u << 1) | (d.address_mode_v << 3);
    };
    for (size_t i = 0; i < s->meshes.size(); i++) {
        if (s->meshes[i].n_vertices == 0) continue;
        const SrMaterial& m = s->meshes[i].material;
        srd::DevMeshTex& t = mtex[i];
        memcpy(t.base_color, m.base_color_value, 16);
        memcpy(t.emissive_factor, m.emissive_factor, 12);
        t.emissive_strength = m.emissive_factor[3];
        t.roughness = m.roughness_factor; t.metallic = m.metallic_factor;
        t.alpha_mode = m.alpha_mode; t.alpha_cutoff = m.alpha_cutoff;
        t.img_base = m.base_color_image; t.img_mr = m.metallic_roughness_image; t.img_normal = m.normal_image; t.img_emissive = m.emissive_image;
        t.samplers = sampler_code(m.base_color_image, m.base_color_sampler) | (sampler_code(m.metallic_roughness_image, m.metallic_roughness_sampler) << 8) |
                     (sampler_code(m.normal_image, m.normal_sampler) << 16) | (sampler_code(m.emissive_image, m.emissive_sampler) << 24);
        mconst[i].textured = (t.img_base != SR_NULL_TEXTURE || t.img_mr != SR_NULL_TEXTURE || t.img_normal != SR_NULL_TEXTURE || t.img_emissive != SR_NULL_TEXTURE) ? 1u : 0u;
        any_textured = any_textured || mconst[i].textured;
    }
    std::vector<srd::DevTexture> textures(s->images.size() ? s->images.size() : 1);
    memset(textures.data(), 0, textures.size() * sizeof(srd::DevTexture));
    for (size_t i = 0; i < s->images.size(); i++) { textures[i].texels = (const uint32_t*)s->images[i].d_texels; textures[i].w = s->images[i].w; textures[i].h = s->images[i].h; }
    if ((rc = s->d_mesh_const.upload(mconst.data(), mconst.size() * sizeof(srd::DevMeshConst))) != SR_OK) return rc;
    if ((rc = s->d_mesh_tex.upload(mtex.data(), mtex.size() * sizeof(srd::DevMeshTex))) != SR_OK) return rc;
    if ((rc = s->d_textures.upload(textures.data(), textures.size() * sizeof(srd::DevTexture))) != SR_OK) return rc;
    s->dev.mesh_const = (const srd::DevMeshConst*)s->d_mesh_const.p;
    s->dev.mesh_tex = (const srd::DevMeshTex*)s->d_mesh_tex.p;
    s->dev.textures = (const srd::DevTexture*)s->d_textures.p;
    *any_textured_out = any_textured;
    return SR_OK;
}

// OpType::Update: same instance layout, new transforms. The triangles are re-flattened on the device into their
// existing leaf slots and the quantised nodes are refitted bottom-up; topology, shade records and mesh tables stay.
// With `reshade` (a mesh of the tree was updated, sr_scene_update_mesh) the flatten also rewrites the slots' shade / shade_tex
// records from the new vertices; the light table follows the emissive arena through upload_instance_tables either way.
int update_in_place(SrScene* s, bool reshade) {
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipDeviceSynchronize());
    int rc = upload_instance_tables(s);
    if (rc != SR_OK) return rc;
    s->mu_info.tables_ms = ms_between(t0, std::chrono::steady_clock::now());
    ThreeMarkTimer timer(s);
    timer.mark();
    int e = reshade ? srk_launch_flatten_reshade((float4*)s->d_tris.p, (float4*)s->d_shade.p, (float4*)s->d_shade_tex.p, (const SrMeshInfo*)s->d_mesh_infos.p,
                                                 (const srd::FlatInstance*)s->d_flat_instances.p, s->fid.n_triangles, nullptr)
                    : srk_launch_flatten_slots((float4*)s->d_tris.p, (const float4*)s->d_shade.p, (const SrMeshInfo*)s->d_mesh_infos.p,
                                               (const srd::FlatInstance*)s->d_flat_instances.p, s->fid.n_triangles, nullptr);
    timer.mark();
    if (e == 0) {
        e = srk_launch_refit((uint32_t*)s->d_nodes.p, (const float4*)s->d_tris.p, (float*)s->d_node_box.p, (const uint32_t*)s->d_level_nodes.p,
                             s->level_offsets.data(), (uint32_t)s->level_offsets.size() - 1, nullptr);
        if (e != 0) fail(SR_ERR_HIP, std::string("refit launch failed: ") + hipGetErrorString((hipError_t)e));
    } else fail(SR_ERR_HIP, std::string("flatten launch failed: ") + hipGetErrorString((hipError_t)e));
    timer.mark();
    const hipError_t se = hipDeviceSynchronize();
    if (e == 0 && se == hipSuccess) timer.read(&s->mu_info.flatten_ms, &s->mu_info.refit_ms);
    if (e != 0) return SR_ERR_HIP;
    HIP_TRY(se);
    s->mu_info.reshaded = reshade ? 1u : 0u;
    s->stats.build_ms = ms_between(t0, std::chrono::steady_clock::now());
    return SR_OK;
}

int full_build(SrScene* s);

// What a builder hands over once its arrays are on the device.
struct BuiltStructure {
    uint64_t n_nodes = 0;        // all nodes: of the one tree, or of the top-level tree and the mesh trees together
    uint64_t tri_bytes = 0;
    uint32_t max_depth = 0;
    uint32_t stack_need = 0;     // worst-case traversal stack entries
    float sah_cost = 0.0f;
    double build_ms = 0.0;
    bool two_level = false, on_device = false;
};

// The built structure becomes the one the kernels see: device pointers, statistics, LDS stack size, form.
void publish(SrScene* s, const BuiltStructure& b) {
    s->dev.nodes = (const float4*)s->d_nodes.p;
    s->dev.blas_nodes = b.two_level ? (const float4*)s->trees.d_blas_nodes.p : nullptr;
    s->dev.tl_inst = b.two_level ? (const uint32_t*)s->d_tl_inst.p : nullptr;
    s->dev.tl_instances = b.two_level ? (const srd::DevTlInstance*)s->d_tl_instances.p : nullptr;
    s->dev.tris = (const float4*)s->d_tris.p;
    s->dev.shade = (const float4*)s->d_shade.p;
    s->dev.shade_tex = (const float4*)s->d_shade_tex.p;
    s->dev.slot_of_gid = (const uint32_t*)s->d_slot_of_gid.p;
    s->dev.counters = (unsigned long long*)s->d_misc.p;
    s->dev.n_tris = s->fid.n_triangles;
    s->stats.n_triangles = s->fid.n_triangles;
    s->stats.n_nodes = b.n_nodes;
    s->stats.node_bytes = b.n_nodes * srl::kNodeBytes;
    s->stats.tri_bytes = b.tri_bytes;
    s->stats.max_depth = b.max_depth;
    s->stats.max_stack = b.stack_need;
    s->stack_entries = (int)((std::max(b.stack_need, 3u) + 1u + 3u) & ~3u);   // + the spare level of the branch-free push, a multiple of 4
    s->stats.sah_cost = b.sah_cost;
    s->stats.build_ms = b.build_ms;
    s->built = true;
    s->two_level = b.two_level;
    s->last_build_on_device = b.on_device;
    // the tree in use is of one form; a host build leaves no device-built tree of its kind in use
    s->height_info[b.two_level ? SR_TREE_KIND_ONE_LEVEL : SR_TREE_KIND_TOP_LEVEL].on_device = 0u;
    if (!b.on_device) s->height_info[b.two_level ? SR_TREE_KIND_TOP_LEVEL : SR_TREE_KIND_ONE_LEVEL].on_device = 0u;
}

// What sr_scene_tree_height_info reports of one device fast build (mode and cap in force are filled in by the query).
void note_tree_height(SrScene* s, uint32_t kind, uint32_t cap, const LbvhResult& r, bool taken) {
    SrTreeHeightInfo& h = s->height_info[kind];
    h.on_device = taken ? 1u : 0u; h.cap = cap;
    h.height_before = r.height_before; h.height_after = r.height_after;
    h.subtrees_rebuilt = r.subtrees_rebuilt; h.prims_rebuilt = r.prims_rebuilt;
}

// ---- two-level form -------------------------------------------------------------------------------------------------
// The reference instances BLASes through a TLAS it rebuilds or updates every frame (tlas.rs:155-191,
// resource_manager.rs:236-251). The one-level form copies every instance's triangles into one world-space tree — memory and
// update cost O(instances x triangles). This form keeps one tree per MESH in object space and a top-level tree over padded
// instance boxes: a changed instance list costs a top-level rebuild (host, O(instances log instances)) and one 128-byte record
// per instance, whatever the meshes hold. Hits are those of the one-level form bit for bit (traverse.h: traverse_ws with TL = true).
constexpr uint32_t kTlStackCap = 47;     // LDS stack entries a two-level walk may need (top-level + pending instances of a leaf + marker + mesh
                                         // tree): with the spare level and the 8 work rows, 56 rows = 56 KB for the 256-thread queue tracers
// what a walk needs (top-level entries + pending instances of a leaf + mesh tree + 1), and what the deepest mesh tree leaves the top-level tree
uint32_t tl_stack_need(uint32_t max_stack, uint32_t blas_stack) { return max_stack + srl::kLeafMax + blas_stack + 1u; }
uint32_t tl_stack_left(uint32_t blas_stack) { return kTlStackCap > blas_stack + srl::kLeafMax + 1u ? kTlStackCap - blas_stack - srl::kLeafMax - 1u : 0u; }

constexpr double kTlMaxCondition = 100.0;    // ||W2O||_inf * ||O2W||_inf above which an instance is baked (rotation + uniform scale: <= 3)

uint32_t min_depth_for(uint64_t n_items) {   // binary depth a median split needs to reach leaves of <= 2 items
    uint32_t need = 2;
    for (uint64_t c = (n_items + 1) / 2; c > 1; c = (c + 1) / 2) need++;
    return need;
}
uint32_t depth_for(uint64_t n_items) {       // ... with slack for SAH splits (the collapse widens nodes until the budget is used)
    return std::max(6u, std::min((uint32_t)srd::kMaxBinaryDepth, min_depth_for(n_items) + 6u));
}

// Object-space tree of one mesh (OpType::SlowBuild of a BLAS, blas.rs:178): same builder, same triangle padding. With `bake` the
// positions are first taken to world space by that transform (transform_point's operation order, as the one-level form flattens):
// the private copy an instance gets whose transform cannot be inverted (see two_level_build).
int build_blas(SrScene* s, uint32_t mesh_slot, const SrTransform* bake, SrScene::HostBlas& b) {
    const int rc = fetch_host_vertices(s, mesh_slot);
    if (rc != SR_OK) return rc;
    const srh::HostMesh& mesh = s->meshes[mesh_slot];
    const uint32_t n = mesh.n_indices / 3;
    std::vector<float> pos((size_t)mesh.n_vertices * 3);
    for (uint32_t i = 0; i < mesh.n_vertices; i++) {
        const float* q = mesh.vertices[i].position;
        float* w = &pos[(size_t)i * 3];
        if (bake) {
            const float* m = bake->m;
            w[0] = ((m[0] * q[0] + m[1] * q[1]) + m[2] * q[2]) + m[3] * 1.0f;
            w[1] = ((m[4] * q[0] + m[5] * q[1]) + m[6] * q[2]) + m[7] * 1.0f;
            w[2] = ((m[8] * q[0] + m[9] * q[1]) + m[10] * q[2]) + m[11] * 1.0f;
        } else { w[0] = q[0]; w[1] = q[1]; w[2] = q[2]; }
    }
    std::vector<srh::BuildTri> tris(n);
    float max_edge = 0.0f, max_abs = 0.0f;
    for (uint32_t p = 0; p < n; p++) {
        const float* v[3];
        for (int j = 0; j < 3; j++) v[j] = &pos[(size_t)mesh.indices[3 * p + j] * 3];
        srh::BuildTri& t = tris[p];
        for (int a = 0; a < 3; a++) {
            t.v0[a] = v[0][a]; t.e1[a] = v[1][a] - v[0][a]; t.e2[a] = v[2][a] - v[0][a];
            max_edge = std::max(max_edge, std::fabs(t.e1[a]) + std::fabs(t.e2[a]));
            for (int j = 0; j < 3; j++) max_abs = std::max(max_abs, std::fabs(v[j][a]));
        }
        t.prim = p; t.inst = 0; t.gid = p;
    }
    srh::BvhResult bvh;
    srh::build_bvh(tris, std::min(depth_for(n), 26u), bvh);          // leaves the top-level tree at least 18 of the kTlStackCap entries
    b.nodes.swap(bvh.nodes);
    b.n_tris = n; b.n_nodes = bvh.n_nodes; b.max_stack = bvh.max_stack; b.max_depth = bvh.max_depth; b.build_ms = bvh.build_ms;
    b.root.max_edge_sum = max_edge; b.root.max_abs_vertex = max_abs;
    b.tris.assign((size_t)n * 12, 0.0f);
    b.shade.assign((size_t)n * 12, 0.0f);
    b.slot_of_prim.assign(n ? n : 1, 0u);
    const bool textured = [&] { const uint32_t* tex = &mesh.material.base_color_image; for (int i = 0; i < 10; i += 2) if (tex[i] != SR_NULL_TEXTURE) return true; return false; }();
    if (textured) b.shade_tex.assign((size_t)n * 24, 0.0f); else b.shade_tex.clear();
    for (int a = 0; a < 3; a++) { b.root.lo[a] = INFINITY; b.root.hi[a] = -INFINITY; }
    for (uint32_t sl = 0; sl < n; sl++) {
        const uint32_t p = bvh.order[sl];
        const SrVertex* v[3];
        const float* w[3];
        for (int j = 0; j < 3; j++) { v[j] = &mesh.vertices[mesh.indices[3 * p + j]]; w[j] = &pos[(size_t)mesh.indices[3 * p + j] * 3]; }
        float* q = &b.tris[(size_t)sl * 12];
        for (int j = 0; j < 3; j++) memcpy(q + 3 * j, w[j], 12);                    // v0, v1, v2 (object space; world space when baked)
        memcpy(q + 9, &p, 4);                                                       // primitive index
        float* sh = &b.shade[(size_t)sl * 12];
        for (int j = 0; j < 3; j++) memcpy(sh + 3 * j, v[j]->normal, 12);
        memcpy(sh + 10, &mesh_slot, 4);                                             // mesh slot; the instance comes from the walk
        if (textured) pack_shade_tex(&b.shade_tex[(size_t)sl * 24], v);
        b.slot_of_prim[p] = sl;
        const srh::BuildTri& t = tris[p];
        for (int a = 0; a < 3; a++) {                                               // the padded triangle box, as the builder bounds it
            const float pad = 4e-6f * (std::fabs(t.e1[a]) + std::fabs(t.e2[a]));
            const float lo = std::min(w[0][a], std::min(w[1][a], w[2][a])) - pad;
            const float hi = std::max(w[0][a], std::max(w[1][a], w[2][a])) + pad;
            b.root.lo[a] = std::min(b.root.lo[a], std::nextafter(lo, -INFINITY)); b.root.hi[a] = std::max(b.root.hi[a], std::nextafter(hi, INFINITY));
        }
    }
    b.valid = true;
    return SR_OK;
}

// The host build of one mesh's tree: the first build, the settle rebuild, every build of a Static mesh, and whatever the device
// build (build_mesh_trees_device) does not take.
int rebuild_mesh_tree(SrScene* s, uint32_t m) {
    SrScene::MeshState& ms = s->mesh_state[m];
    ms.tree = SrScene::HostBlas();
    int rc = build_blas(s, m, nullptr, ms.tree);
    if (rc != SR_OK) return rc;
    s->mu_info.blas_rebuilt++; s->mu_info.blas_build_ms += ms.tree.build_ms;
    ms.rebuilt_now = true; ms.refit_pending = false;
    return SR_OK;
}

// Appends one tree with its triangle / shade / primitive -> slot records to the concatenated host arrays (references become global).
struct BlasCat {
    std::vector<uint32_t> nodes, slot_of_prim;
    std::vector<float> tris, shade, shade_tex;
    bool textured = false;
    void append(const SrScene::HostBlas& b, uint32_t* node_base, uint32_t* tri_base) {
        const uint32_t nb = (uint32_t)(nodes.size() / srl::kNodeDwords), tb = (uint32_t)(tris.size() / 12);
        *node_base = nb; *tri_base = tb;
        nodes.resize(nodes.size() + (size_t)b.n_nodes * srl::kNodeDwords);
        for (uint32_t i = 0; i < b.n_nodes; i++) {
            uint32_t* q = &nodes[((size_t)nb + i) * srl::kNodeDwords];
            memcpy(q, &b.nodes[(size_t)i * srl::kNodeDwords], srl::kNodeBytes);
            for (int c = 0; c < srl::kBvhWidth; c++) {
                const int ref = (int)q[srl::kChildOffset + c];
                if (ref >= 0) q[srl::kChildOffset + c] = (uint32_t)(ref + (int)nb);
                else { const uint32_t lv = ~(uint32_t)ref; const uint32_t cnt = lv & 7u; if (cnt) q[srl::kChildOffset + c] = ~((((lv >> 3) + tb) << 3) | cnt); }
            }
        }
        tris.insert(tris.end(), b.tris.begin(), b.tris.end());
        shade.insert(shade.end(), b.shade.begin(), b.shade.end());
        if (textured) {
            shade_tex.resize((size_t)tb * 24, 0.0f);
            if (!b.shade_tex.empty()) shade_tex.insert(shade_tex.end(), b.shade_tex.begin(), b.shade_tex.end());
            else shade_tex.resize(((size_t)tb + b.n_tris) * 24, 0.0f);
        }
        for (uint32_t p = 0; p < b.n_tris; p++) slot_of_prim.push_back(tb + b.slot_of_prim[p]);
    }
};

// Every live mesh's records, one after the other (cached on the host per mesh), then the baked copies of the instance list at hand.
int upload_mesh_trees(SrScene* s, const std::vector<SrScene::HostBlas>& baked) {
    int rc;
    const size_t nm = s->meshes.size();
    BlasCat cat;
    for (size_t m = 0; m < nm; m++) {
        if (s->meshes[m].n_vertices == 0) continue;
        // a host copy that a device refit left behind holds the old vertices: it is rebuilt before it is uploaded again
        const SrScene::MeshState& ms = s->mesh_state[m];
        if (!ms.tree.valid || ms.tree.host_stale || ms.refit_pending) { if ((rc = rebuild_mesh_tree(s, (uint32_t)m)) != SR_OK) return rc; }
        cat.textured = cat.textured || !ms.tree.shade_tex.empty();
    }
    for (size_t m = 0; m < nm; m++) {
        s->mesh_state[m].node_cap = 0;        // the ranges behind the concatenation are given up: a later device build takes a new one
        if (s->meshes[m].n_vertices) cat.append(s->mesh_state[m].tree, &s->mesh_state[m].node_base, &s->mesh_state[m].tri_base);
    }
    s->trees.tl_baked_node_base.assign(baked.size(), 0u); s->trees.tl_baked_tri_base.assign(baked.size(), 0u);
    for (size_t k = 0; k < baked.size(); k++) cat.append(baked[k], &s->trees.tl_baked_node_base[k], &s->trees.tl_baked_tri_base[k]);
    if (cat.tris.size() / 12 >= (1ull << 28) || cat.nodes.size() / srl::kNodeDwords >= (1ull << 31)) return fail(SR_ERR_UNSUPPORTED, "the meshes together exceed 2^28 triangles (leaf reference encoding)");
    if (cat.textured) cat.shade_tex.resize(cat.tris.size() / 12 * 24, 0.0f);
    if (cat.slot_of_prim.empty()) cat.slot_of_prim.push_back(0u);
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = s->trees.d_blas_nodes.upload(cat.nodes.data(), cat.nodes.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_tris.upload(cat.tris.data(), cat.tris.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_shade.upload(cat.shade.data(), cat.shade.size() * 4)) != SR_OK) return rc;
    if (cat.textured) { if ((rc = s->d_shade_tex.upload(cat.shade_tex.data(), cat.shade_tex.size() * 4)) != SR_OK) return rc; }
    else s->d_shade_tex.release();
    if ((rc = s->d_slot_of_gid.upload(cat.slot_of_prim.data(), cat.slot_of_prim.size() * 4)) != SR_OK) return rc;
    s->trees.any_textured_tl = cat.textured;
    s->trees.tl_blas_nodes = cat.nodes.size() / srl::kNodeDwords; s->trees.tl_blas_tris = cat.tris.size() / 12;
    s->trees.blas_node_end = s->trees.tl_blas_nodes;
    s->trees.blas_device_current = true;
    s->trees.tl_baked = !baked.empty();
    s->trees.tl_mesh_rows_current = false;
    s->refit.set.clear();                     // void: the bases moved (MeshTrees)
    return SR_OK;
}

// Instance boxes from which SR_TL_BUILD_AUTO builds the top level on the device: the smallest measured instance count at which
// the device build beats the host's by more than the spread of 20 calls, rounded up to a power of two. Measured on an MI355X
// (scripts/gpu_top_level_build.py -> profiles/top_level_build.json, table in DESIGN.md section 4), sr_scene_set_instances in ms,
// host / device: 1 000: 0.66 / 1.83, 2 048: 1.36 / 2.07, 4 096: 2.51 / 2.30, 10 000: 6.19 / 2.71, 100 000: 60 / 5.6.
constexpr uint32_t kTlDeviceMinBoxes = 4096;
static_assert(sizeof(SrTopLevelInfo) == 64 && sizeof(srd::TlMeshRow) == 48 && sizeof(srd::DevTlInstance) == 128, "layouts the harness and the record kernel rely on");
using RootBlock = SrScene::HostBlas::RootBlock;      // copied whole: both sides hold lo, hi, max_abs_vertex, max_edge_sum in this order
static_assert(sizeof(RootBlock) == 32 && offsetof(RootBlock, hi) == 12 && offsetof(RootBlock, max_abs_vertex) == 24 && offsetof(RootBlock, max_edge_sum) == 28 &&
              offsetof(srd::TlMeshRow, hi) == 12 && offsetof(srd::TlMeshRow, max_abs_vertex) == 24 && offsetof(srd::TlMeshRow, max_edge_sum) == 28, "a TlMeshRow begins with the root block");

// Why the top-level choice leaves this many instances (or instance boxes) to the host, or SR_TL_ON_DEVICE.
uint32_t tl_count_reason(const SrScene* s, uint32_t count) {
    return count < 2 ? SR_TL_HOST_TOO_FEW : s->tl_build_mode == SR_TL_BUILD_AUTO && count < kTlDeviceMinBoxes ? SR_TL_HOST_BELOW_THRESHOLD : SR_TL_ON_DEVICE;
}
// What both top-level builders end in: the structure becomes the one the kernels see, and `info` (but for build_ms) what sr_scene_top_level_info reports.
void publish_two_level(SrScene* s, SrTopLevelInfo info, uint32_t max_depth, float sah_cost, std::chrono::steady_clock::time_point t0) {
    BuiltStructure built;
    built.n_nodes = info.n_nodes + s->trees.tl_blas_nodes; built.tri_bytes = s->trees.tl_blas_tris * 48;
    built.max_depth = max_depth; built.stack_need = tl_stack_need(info.max_stack, info.blas_stack); built.sah_cost = sah_cost;
    built.build_ms = ms_between(t0, std::chrono::steady_clock::now());
    built.two_level = true; built.on_device = info.on_device != 0u;
    publish(s, built);
    s->shape.clear();
    info.build_ms = s->stats.build_ms;
    s->tl_info = info;
}

// The changed instance list of a scene that is already built in the two-level form, on the device (bvh_gpu.hip): instance
// records and padded boxes by srk_tl_records (tl_record.h, as the host loop in two_level_build), the tree over the boxes by
// srk_tl_build. *reason stays SR_TL_ON_DEVICE when the build is done; any other value: the host build below does the whole
// job (what this function has rewritten by then, it rewrote after the device-wide wait, and the host build writes it again).
int top_level_build_device(SrScene* s, std::chrono::steady_clock::time_point t0, uint32_t* reason) {
    const uint32_t ni = (uint32_t)s->fid.instances.size();
    if (!s->built || !s->two_level || !s->trees.blas_device_current) { *reason = SR_TL_HOST_NOT_TWO_LEVEL; return SR_OK; }   // also: meshes added or removed since
    if (s->tl_build_mode == SR_TL_BUILD_HOST) { *reason = SR_TL_HOST_MODE; return SR_OK; }
    if ((*reason = tl_count_reason(s, ni)) != SR_TL_ON_DEVICE) return SR_OK;
    int rc;
    HIP_TRY(hipDeviceSynchronize());          // frames in flight read the tables that are rewritten from here on
    if (s->trees.tl_baked && (rc = upload_mesh_trees(s, {})) != SR_OK) return rc;   // the previous list had baked copies behind the mesh trees
    if (!s->trees.tl_mesh_rows_current) {
        std::vector<srd::TlMeshRow> rows(s->meshes.size() ? s->meshes.size() : 1);
        memset(rows.data(), 0, rows.size() * sizeof(srd::TlMeshRow));
        for (size_t m = 0; m < s->meshes.size(); m++) {
            if (s->meshes[m].n_vertices == 0 || !s->mesh_state[m].tree.valid) continue;
            const SrScene::HostBlas& b = s->mesh_state[m].tree;
            srd::TlMeshRow& r = rows[m];
            memcpy(&r, &b.root, sizeof(RootBlock));
            r.max_stack = b.max_stack; r.blas_root = s->mesh_state[m].node_base; r.prim_base = s->mesh_state[m].tri_base; r.n_tris = b.n_tris;
        }
        if ((rc = s->trees.d_tl_mesh_rows.upload(rows.data(), rows.size() * sizeof(srd::TlMeshRow))) != SR_OK) return rc;
        s->trees.tl_mesh_rows_current = true;
    }
    if ((rc = upload_instance_tables(s)) != SR_OK) return rc;
    if ((rc = s->d_tl_instances.reserve((size_t)ni * sizeof(srd::DevTlInstance))) != SR_OK || (rc = s->d_tl_boxes.reserve((size_t)ni * 24)) != SR_OK ||
        (rc = s->d_tl_result.reserve(16)) != SR_OK) return rc;
    int e = srk_tl_records((const srd::FlatInstance*)s->d_flat_instances.p, (const srd::TlMeshRow*)s->trees.d_tl_mesh_rows.p, ni, kTlMaxCondition,
                           (srd::DevTlInstance*)s->d_tl_instances.p, (float*)s->d_tl_boxes.p, (uint32_t*)s->d_tl_result.p, nullptr);
    if (e != 0) return fail(SR_ERR_HIP, std::string("instance record launch failed: ") + hipGetErrorString((hipError_t)e));
    uint32_t res[3] = {0, 0, 0};              // instances the host would bake, deepest mesh tree in use, instances with a box
    HIP_TRY(hipMemcpy(res, s->d_tl_result.p, sizeof(res), hipMemcpyDeviceToHost));
    const auto t1 = std::chrono::steady_clock::now();
    const uint32_t nb = res[2], blas_stack = res[1];
    if (res[0] != 0) { *reason = SR_TL_HOST_BAKED_INSTANCE; return SR_OK; }
    if ((*reason = tl_count_reason(s, nb)) != SR_TL_ON_DEVICE) return SR_OK;
    const uint32_t left = tl_stack_left(blas_stack);
    if (left < min_depth_for(nb)) { *reason = SR_TL_HOST_STACK_BUDGET; return SR_OK; }      // the host build reports the error
    const uint32_t node_cap = nb + 64;        // inner nodes of a tree with >= 2 children per node and >= 1 box per leaf: < nb
    if ((rc = s->d_nodes.reserve((size_t)node_cap * srl::kNodeBytes)) != SR_OK || (rc = s->d_node_box.reserve((size_t)node_cap * 24)) != SR_OK ||
        (rc = s->d_tl_inst.reserve((size_t)nb * 4)) != SR_OK || (rc = s->d_scratch.reserve(srk_tl_scratch_bytes(ni, nb, node_cap, s->fast_build_ploc))) != SR_OK) return rc;
    const TreeBuildTarget target((float4*)s->d_nodes.p, node_cap, (float*)s->d_node_box.p, s->d_scratch.p, s->d_scratch.bytes, min_depth_for(nb), left,
                                 s->height_bound == SR_HEIGHT_BOUND_REBALANCE, s->fast_build_ploc);
    const BoxesBuildArgs a(target, (const float*)s->d_tl_boxes.p, ni, nb, (uint32_t*)s->d_tl_inst.p);
    LbvhResult r;
    e = srk_tl_build(a, &r, nullptr);
    if (e > 0) return fail(SR_ERR_HIP, std::string("device top-level build failed: ") + hipGetErrorString((hipError_t)e));
    const uint32_t need = tl_stack_need(r.max_stack, blas_stack);            // as the host build counts it
    note_tree_height(s, SR_TREE_KIND_TOP_LEVEL, left, r, e == 0 && need <= kTlStackCap);
    if (e < 0 || need > kTlStackCap) { *reason = SR_TL_HOST_STACK_BUDGET; return SR_OK; }
    SrTopLevelInfo info{};
    info.on_device = 1u; info.reason = SR_TL_ON_DEVICE;
    info.n_nodes = r.n_nodes; info.n_boxes = nb; info.n_instances = ni; info.max_stack = r.max_stack; info.blas_stack = blas_stack;
    info.records_ms = ms_between(t0, t1);
    info.tree_ms = ms_between(t1, std::chrono::steady_clock::now());
    publish_two_level(s, info, r.max_depth, 0.0f, t0);
    s->tl_boxes_host.clear();
    return SR_OK;
}

// Whether two_level_build gives an instance with this transform a baked copy of its mesh (the test comes before anything that reads the mesh).
bool instance_is_baked(const float* M) {
    const float unit_lo[3] = {0.0f, 0.0f, 0.0f}, unit_hi[3] = {1.0f, 1.0f, 1.0f};
    float w2o[12], lo[3], hi[3], pad_a, pad_b;
    return srd::tl_record(M, unit_lo, unit_hi, 0.0f, 0.0f, kTlMaxCondition, w2o, lo, hi, &pad_a, &pad_b) == srd::kTlRecordBaked;
}

// Triangles of a mesh from which SR_MESH_TREE_BUILD_AUTO builds its tree on the device: the smallest measured size at which the
// device build beats both the host build and the library before this path by more than the two spreads of 20 calls combined,
// rounded up to a power of two (the rule kTlDeviceMinBoxes was set by), provided the device takes a measured size at or above
// that threshold. Measured on an MI355X (scripts/gpu_mesh_tree_build.py -> profiles/mesh_tree_build.json, table in DESIGN.md
// section 4): the device loses at 1 024 and 4 096 triangles (launch-bound: a stream wait per PLOC iteration and per collapse level),
// wins at 20 992 (3.6 against 10.4 ms), and the default PLOC trees of the 65 536-, 250 000- and 1 000 000-triangle spheres are deeper
// than kBlasStackCap and are refused. The rule's threshold would be 32 768, and no measured size from there on is built on the
// device: no size qualifies, so AUTO stays on the host everywhere (0xFFFFFFFF = never); the device build runs in mode DEVICE only.
constexpr uint32_t kBlasDeviceMinTris = 0xFFFFFFFFu;
// The same under SR_HEIGHT_BOUND_REBALANCE (scripts/gpu_mesh_tree_build.py --leg rebalance -> profiles/mesh_tree_rebalance.json, table
// in DESIGN.md section 4), host / parent commit / device in ms: 4 096: 2.13 / 2.10 / 2.79, 20 992: 11.0 / 10.5 / 3.61, 65 536: 69.6 / 69.6 / 5.25,
// 250 000: 129 / 129 / 8.34, 1 000 000: 406 / 416 / 17.3. The device wins by more than the combined spreads from 20 992 triangles on,
// which rounds up to 32 768, and every measured size above that is now built on the device: the rule yields 32 768.
constexpr uint32_t kBlasDeviceMinTrisBounded = 32768;
// Bytes of scratch slabs one batched launch may hold (sr_scene_set_mesh_tree_batch): 256 MiB, some 220 meshes of
// SR_BLAS_BATCH_MAX_TRIS triangles or thousands of smaller ones; a larger batch takes ceil(bytes / limit) launches.
constexpr size_t kBlasBatchScratchBytes = (size_t)256 << 20;
constexpr uint32_t kBlasStackCap = 26;       // build_blas's limit: leaves the top-level tree at least 18 of the kTlStackCap entries
static_assert(sizeof(SrMeshTreeInfo) == 40 && sizeof(SrMeshTreeBatchInfo) == 32 && sizeof(SrMeshUpdateInfo) == 64 && sizeof(SrTreeHeightInfo) == 32 && sizeof(SrMeshVertexInfo) == 40 && sizeof(SrLightTableInfo) == 56, "layouts the harness relies on");
uint32_t blas_device_min_tris(const SrScene* s) { return s->height_bound == SR_HEIGHT_BOUND_REBALANCE ? kBlasDeviceMinTrisBounded : kBlasDeviceMinTris; }

// Where a mesh-tree writer (batched build, per-mesh build, the refit's record kernel) writes; read once the call has grown the buffers.
srd::BlasBatchArrays mesh_tree_arrays(const SrScene* s) {     // nodes, node_box, tris, shade, shade_tex, slot_of_gid, rows
    return {(uint32_t*)s->trees.d_blas_nodes.p, (float*)s->trees.d_blas_node_box.p, (float4*)s->d_tris.p, (float4*)s->d_shade.p,
            s->trees.any_textured_tl ? (float4*)s->d_shade_tex.p : nullptr, (uint32_t*)s->d_slot_of_gid.p, s->trees.rows_dev(s->meshes.size())};
}
// The host's book-keeping of one tree the device built, from the ten-word block (root block, nodes, stack need); the caller sets the level ranges.
void note_built(SrScene* s, SrScene::HostBlas& b, const uint32_t* out, uint32_t max_depth) {
    s->trees.tl_blas_nodes = s->trees.tl_blas_nodes - b.n_nodes + out[8];
    memcpy(&b.root, out, sizeof(b.root));
    b.n_nodes = out[8]; b.max_stack = out[9]; b.max_depth = max_depth;
    b.host_stale = true; b.device_built = true;
}

// The batched step of build_mesh_trees_device. *rest receives what the batch does not take and what it hands back, in the set's
// order, so that the per-mesh builds keep theirs.
int batch_build_mesh_trees(SrScene* s, const std::vector<uint32_t>& set, const srd::BlasBatchArrays& arrays, uint32_t cap,
                           std::chrono::steady_clock::time_point t0, std::vector<uint32_t>* rest) {
    int rc;
    std::vector<uint32_t> small;
    for (uint32_t m : set) if (s->mesh_state[m].tree.n_tris >= 1u && s->mesh_state[m].tree.n_tris <= SR_BLAS_BATCH_MAX_TRIS) small.push_back(m);
    std::vector<srd::BlasBatchResult> results(small.size());
    if (!small.empty()) {
        // one launch per kBlasBatchScratchBytes of slabs (a mesh's slab is ~0.3 KB per triangle: a launch holds hundreds of
        // the largest meshes), all enqueued behind each other on one stream, so they may share the scratch buffer
        std::vector<srd::BlasBatchRow> rows(small.size());
        std::vector<uint32_t> launch_first(1, 0u);
        size_t used = 0, most = 0;
        for (size_t k = 0; k < small.size(); k++) {
            const uint32_t m = small[k];
            SrScene::MeshState& ms = s->mesh_state[m];
            const uint32_t n = ms.tree.n_tris;
            s->trees.take_range(ms);
            const size_t slab = srk_blas_batch_slab_bytes(n, ms.node_cap);
            if (used != 0 && used + slab > kBlasBatchScratchBytes) { launch_first.push_back((uint32_t)k); used = 0; }
            srd::BlasBatchRow& r = rows[k];
            r.vertices = (uint64_t)(uintptr_t)s->meshes[m].d_vertices; r.indices = (uint64_t)(uintptr_t)s->meshes[m].d_indices;
            r.scratch = (uint64_t)used;                   // offset for now: the buffer may still move
            r.n_tris = n; r.n_vertices = s->meshes[m].n_vertices;
            r.mesh_slot = m; r.textured = ms.tree.shade_tex.empty() ? 0u : 1u;
            r.node_base = ms.node_base; r.node_cap = ms.node_cap; r.tri_base = ms.tri_base;
            r.stack_floor = std::min(depth_for(n), cap); r.stack_cap = cap; r._pad = 0u;
            used += slab; most = std::max(most, used);
        }
        launch_first.push_back((uint32_t)small.size());
        if ((rc = s->d_scratch.reserve(most)) != SR_OK || (rc = s->d_batch_rows.reserve(rows.size() * sizeof(srd::BlasBatchRow))) != SR_OK ||
            (rc = s->d_batch_results.reserve(results.size() * sizeof(srd::BlasBatchResult))) != SR_OK) return rc;
        for (srd::BlasBatchRow& r : rows) r.scratch += (uint64_t)(uintptr_t)s->d_scratch.p;
        HIP_TRY(hipMemcpyAsync(s->d_batch_rows.p, rows.data(), rows.size() * sizeof(srd::BlasBatchRow), hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipMemsetAsync(s->d_batch_results.p, 0xFF, results.size() * sizeof(srd::BlasBatchResult), nullptr));      // a status no workgroup writes
        for (size_t l = 0; l + 1 < launch_first.size(); l++) {
            const int e = srk_blas_batch_build((const srd::BlasBatchRow*)s->d_batch_rows.p + launch_first[l], launch_first[l + 1] - launch_first[l], arrays,
                                               (srd::BlasBatchResult*)s->d_batch_results.p + launch_first[l], s->fast_build_ploc, nullptr);
            if (e != 0) return fail(SR_ERR_HIP, std::string("batched mesh-tree build failed: ") + hipGetErrorString((hipError_t)e));
        }
        HIP_TRY(hipMemcpy(results.data(), s->d_batch_results.p, results.size() * sizeof(srd::BlasBatchResult), hipMemcpyDeviceToHost));   // the only wait
        s->batch_info.launches = (uint32_t)launch_first.size() - 1u;
        if (s->timing) s->batch_info.batch_ms = ms_between(t0, std::chrono::steady_clock::now());
    }
    size_t k = 0;
    for (uint32_t m : set) {
        if (k >= small.size() || small[k] != m) { rest->push_back(m); continue; }
        const srd::BlasBatchResult& r = results[k++];
        SrScene::HostBlas& b = s->mesh_state[m].tree;
        if (r.status != srd::kBlasBatchBuilt || r.n_levels == 0u || r.n_levels > srd::kBlasBatchMaxLevels || r.out[9] > cap) {
            s->batch_info.passed_on++; rest->push_back(m); continue;      // too tall or failed: its ranges are as they were
        }
        LbvhResult h;
        h.height_before = h.height_after = r.height;
        note_tree_height(s, SR_TREE_KIND_MESH, cap, h, true);
        note_built(s, b, r.out, r.n_levels);
        b.level_ranges.clear();
        for (uint32_t l = 0; l < r.n_levels; l++) b.level_ranges.emplace_back(r.levels[2 * l], r.levels[2 * l + 1]);
        s->batch_info.batched++;
    }
    return SR_OK;
}

// The per-mesh step of build_mesh_trees_device. A tree deeper than `cap` is refused through *reason and remembered with the topology it
// was refused under (the attempt is not repeated); the mesh's book-keeping is then as it was.
int build_mesh_tree_device(SrScene* s, uint32_t m, const srd::BlasBatchArrays& arrays, uint32_t cap, uint32_t* reason) {
    SrScene::MeshState& ms = s->mesh_state[m];
    SrScene::HostBlas& b = ms.tree;
    const uint32_t n = b.n_tris;
    s->trees.take_range(ms);
    if (const int rc = s->d_scratch.reserve(srk_lbvh_scratch_bytes(n, ms.node_cap, s->fast_build_ploc)); rc != SR_OK) return rc;
    const MeshBuildArgs a(arrays, ms.node_base, ms.node_cap, ms.tri_base, s->d_scratch.p, s->d_scratch.bytes, std::min(depth_for(n), cap), cap,
                          s->height_bound == SR_HEIGHT_BOUND_REBALANCE, s->fast_build_ploc, (const SrVertex*)s->meshes[m].d_vertices,
                          (const uint32_t*)s->meshes[m].d_indices, s->meshes[m].n_vertices, n, m, b.shade_tex.empty() ? 0u : 1u, (uint32_t*)s->d_blas_build_out.p);
    LbvhResult r;
    const int e = srk_blas_build(a, &r, nullptr);
    if (e > 0) return fail(SR_ERR_HIP, std::string("device mesh-tree build failed: ") + hipGetErrorString((hipError_t)e));
    note_tree_height(s, SR_TREE_KIND_MESH, cap, r, e == 0 && r.max_stack <= cap);
    if (e < 0 || r.max_stack > cap) { ms.device_refused = s->fast_build_ploc; *reason = SR_MESH_TREE_HOST_STACK_BUDGET; return SR_OK; }
    uint32_t out[10];
    HIP_TRY(hipMemcpy(out, s->d_blas_build_out.p, sizeof(out), hipMemcpyDeviceToHost));
    note_built(s, b, out, r.max_depth);
    b.level_ranges = r.level_ranges;
    return SR_OK;
}

// Blas::rebuild (blas.rs:285-310) on the device for the meshes of `set` (pending updatable meshes whose state asked for
// SR_OP_FAST_BUILD): srk_blas_build writes each tree into the mesh's ranges of the concatenated arrays, which stay resident.
// The triangle-side ranges stay where they are (only the leaf order inside them changes). A device-built tree has another node
// count than the tree it replaces, and references are indices into d_blas_nodes, so at its first device build a mesh takes a node
// range of the builder's proven bound (fewer inner nodes than triangles) behind everything in use, and keeps it for later builds;
// the buffer grows by a device-to-device copy. *reason != SR_MESH_TREE_ON_DEVICE: a tree was refused and the host builds them all.
// With the batch on (sr_scene_set_mesh_tree_batch) the meshes of at most SR_BLAS_BATCH_MAX_TRIS triangles are first built by
// srk_blas_batch_build, one workgroup per mesh, with one read-back of all result rows; what is larger, and what the batch hands back
// (too tall, failed: its ranges are as they were), then goes through srk_blas_build as without the batch.
int build_mesh_trees_device(SrScene* s, const std::vector<uint32_t>& set, uint32_t* reason) {
    int rc;
    uint64_t end = s->trees.blas_node_end;
    for (uint32_t m : set) if (s->mesh_state[m].node_cap == 0) end += SrScene::MeshTrees::range_bound(s->mesh_state[m].tree.n_tris);
    if (end >= (1ull << 31)) return fail(SR_ERR_UNSUPPORTED, "the mesh trees together exceed 2^31 nodes");
    HIP_TRY(hipDeviceSynchronize());          // frames in flight read the arrays that are rewritten (and may move) from here on
    if ((rc = s->trees.d_blas_nodes.grow_keep((size_t)end * srl::kNodeBytes, (size_t)s->trees.blas_node_end * srl::kNodeBytes)) != SR_OK ||
        (rc = s->trees.d_blas_node_box.reserve((size_t)end * 24)) != SR_OK || (rc = s->d_blas_build_out.reserve(64)) != SR_OK) return rc;
    const srd::BlasBatchArrays arrays = mesh_tree_arrays(s);
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t cap = s->height_bound == SR_HEIGHT_BOUND_REBALANCE && s->mesh_tree_cap ? s->mesh_tree_cap : kBlasStackCap;      // binds device builds only
    std::vector<uint32_t> rest;               // what the per-mesh build takes: everything, or what the batch does not take or hands back
    if (s->blas_batch_mode != SR_BLAS_BATCH_ON) rest = set;
    else if ((rc = batch_build_mesh_trees(s, set, arrays, cap, t0, &rest)) != SR_OK) return rc;
    for (uint32_t m : rest)                   // a refusal returns at once: the caller's invalidation also takes what was built so far
        if ((rc = build_mesh_tree_device(s, m, arrays, cap, reason)) != SR_OK || *reason != SR_MESH_TREE_ON_DEVICE) return rc;
    if (!set.empty()) { s->mt_info.n_nodes = s->mesh_state[set.back()].tree.n_nodes; s->mt_info.max_stack = s->mesh_state[set.back()].tree.max_stack; }
    if (s->timing) s->mt_info.device_build_ms = ms_between(t0, std::chrono::steady_clock::now());   // every build ends with a wait for its stream
    for (uint32_t m : set) {                  // all were taken: they count as built (mark_mesh_trees: SR_OP_FAST_BUILD)
        SrScene::MeshState& ms = s->mesh_state[m];
        ms.refit_pending = false; ms.rebuilt_now = true;
        s->mu_info.blas_rebuilt++; s->mt_info.built_on_device++;
    }
    s->refit.set.clear();                     // void: the node lists of these meshes changed (MeshTrees)
    return SR_OK;
}

struct PendingMeshTrees {                     // the classification of maintain_mesh_trees
    std::vector<uint32_t> refits, builds;     // pending meshes that ask for SR_OP_UPDATE / SR_OP_FAST_BUILD (more than 8 updates since its rebuild)
    bool slow = false, any_pending = false, any_stale = false;    // one asks for anything else; any is pending; any has a stale host copy
};
void classify_pending_mesh_trees(SrScene* s, uint32_t forced, PendingMeshTrees& p) {
    for (size_t m = 0; m < s->meshes.size(); m++) {
        SrScene::MeshState& ms = s->mesh_state[m];
        ms.rebuilt_now = ms.refit_now = false;
        if (s->meshes[m].n_vertices == 0) continue;
        p.any_stale = p.any_stale || ms.tree.host_stale;
        if (!ms.refit_pending) continue;
        p.any_pending = true;
        const uint32_t op = forced != SR_OP_NONE ? forced : srh::as_state_next_op(ms.state, true);
        if (op == SR_OP_UPDATE) p.refits.push_back((uint32_t)m);
        else if (op == SR_OP_FAST_BUILD) p.builds.push_back((uint32_t)m);
        else p.slow = true;
    }
}

// SR_MESH_TREE_ON_DEVICE or why the host takes all. First anything that makes the build re-concatenate the mesh trees: the form, meshes added or
// removed, an updated Static mesh, baked copies behind the mesh trees now or in the new list; then what the pending meshes themselves ask for.
uint32_t mesh_tree_host_reason(const SrScene* s, const PendingMeshTrees& p) {
    if (!s->built || !s->two_level || !s->trees.blas_device_current) return s->static_mesh_updated ? SR_MESH_TREE_HOST_STATIC_MESH : SR_MESH_TREE_HOST_NOT_RESIDENT;
    if (s->trees.tl_baked) return SR_MESH_TREE_HOST_BAKED_INSTANCE;
    for (const srh::HostInstance& in : s->fid.instances) if (instance_is_baked(in.o2w.m)) return SR_MESH_TREE_HOST_BAKED_INSTANCE;
    if (p.slow) return SR_MESH_TREE_HOST_SLOW_BUILD;
    for (uint32_t m : p.builds) {
        const uint32_t n = s->mesh_state[m].tree.n_tris;
        if (s->blas_build_mode == SR_MESH_TREE_BUILD_HOST) return SR_MESH_TREE_HOST_MODE;
        if (s->blas_build_mode == SR_MESH_TREE_BUILD_AUTO && n < blas_device_min_tris(s) &&
            !(s->blas_batch_mode == SR_BLAS_BATCH_ON && n <= SR_BLAS_BATCH_MAX_TRIS)) return SR_MESH_TREE_HOST_BELOW_THRESHOLD;      // the batch is an opt-in for small meshes
        if (s->mesh_state[m].device_refused == s->fast_build_ploc) return SR_MESH_TREE_HOST_STACK_BUDGET;     // refused before
    }
    return SR_MESH_TREE_ON_DEVICE;
}

// Another set of meshes than the device refitted last: its rows, node lists and accumulator init into the cached refit set.
int prepare_refit_set(SrScene* s, const std::vector<uint32_t>& set) {
    std::vector<srd::BlasRefitMesh> rows(set.size());
    std::vector<std::vector<uint32_t>> by_depth;
    uint32_t threads = 0;
    for (size_t k = 0; k < set.size(); k++) {
        const uint32_t m = set[k];
        const SrScene::HostBlas& b = s->mesh_state[m].tree;
        srd::BlasRefitMesh& r = rows[k];
        r.vertices = (uint64_t)(uintptr_t)s->meshes[m].d_vertices; r.indices = (uint64_t)(uintptr_t)s->meshes[m].d_indices;
        r.tri_base = s->mesh_state[m].tri_base; r.n_tris = b.n_tris; r.n_vertices = s->meshes[m].n_vertices;
        r.first_thread = threads; r.mesh_slot = m; r.textured = b.shade_tex.empty() ? 0u : 1u;
        threads += (b.n_tris + 63u) & ~63u;
        const uint32_t nb = s->mesh_state[m].node_base;
        if (b.device_built) {             // the host copy's topology is stale: the levels the device build returned
            if (by_depth.size() < b.level_ranges.size()) by_depth.resize(b.level_ranges.size());
            for (size_t d = 0; d < b.level_ranges.size(); d++)
                for (uint32_t q = 0; q < b.level_ranges[d].second; q++) by_depth[d].push_back(nb + b.level_ranges[d].first + q);
            continue;
        }
        std::vector<uint32_t> nodes, offsets;       // deepest level first
        srh::tree_levels(b.nodes, nodes, offsets);
        const size_t levels = offsets.size() - 1;
        if (by_depth.size() < levels) by_depth.resize(levels);
        for (size_t l = 0; l < levels; l++)
            for (uint32_t q = offsets[l]; q < offsets[l + 1]; q++) by_depth[levels - 1 - l].push_back(nb + nodes[q]);
    }
    std::vector<uint32_t> list;
    s->refit.level_offsets.assign(1, 0u);
    for (size_t d = by_depth.size(); d-- > 0;) { list.insert(list.end(), by_depth[d].begin(), by_depth[d].end()); s->refit.level_offsets.push_back((uint32_t)list.size()); }
    std::vector<uint32_t> init(set.size() * 8);
    for (size_t k = 0; k < init.size(); k++) init[k] = srd::mesh_acc_seed((int)(k & 7));
    int rc;
    if ((rc = s->refit.d_meshes.upload(rows.data(), rows.size() * sizeof(srd::BlasRefitMesh))) != SR_OK ||
        (rc = s->refit.d_nodes.upload(list.data(), list.size() * 4)) != SR_OK ||
        (rc = s->refit.d_acc_init.upload(init.data(), init.size() * 4)) != SR_OK ||
        (rc = s->refit.d_acc.reserve(init.size() * 4)) != SR_OK || (rc = s->refit.d_out.reserve(init.size() * 4)) != SR_OK) return rc;
    s->refit.set = set;
    s->refit.threads = threads;
    return SR_OK;
}

// The device refit of the cached set: two kinds of launch, one read-back of the root blocks (32 bytes per mesh), the per-mesh marks.
int refit_mesh_trees(SrScene* s) {
    const std::vector<uint32_t>& set = s->refit.set;
    if (const int rc = s->trees.d_blas_node_box.reserve((size_t)s->trees.blas_node_end * 24); rc != SR_OK) return rc;
    const srd::BlasBatchArrays arrays = mesh_tree_arrays(s);
    ThreeMarkTimer timer(s);
    timer.mark();
    int e = srk_blas_records((const srd::BlasRefitMesh*)s->refit.d_meshes.p, (uint32_t)set.size(), s->refit.threads, arrays.tris, arrays.shade, arrays.shade_tex,
                             (uint32_t*)s->refit.d_acc.p, (const uint32_t*)s->refit.d_acc_init.p, arrays.rows, (float*)s->refit.d_out.p, nullptr);
    timer.mark();
    if (e == 0) e = srk_blas_refit(arrays.nodes, arrays.tris, arrays.node_box, (const uint32_t*)s->refit.d_nodes.p,
                                   s->refit.level_offsets.data(), (uint32_t)s->refit.level_offsets.size() - 1, nullptr);
    timer.mark();
    std::vector<float> out(set.size() * 8);
    const hipError_t ce = e == 0 ? hipMemcpy(out.data(), s->refit.d_out.p, out.size() * 4, hipMemcpyDeviceToHost) : hipSuccess;   // waits for the launches above
    if (e == 0 && ce == hipSuccess) timer.read(&s->mu_info.flatten_ms, &s->mu_info.refit_ms);
    if (e != 0) return fail(SR_ERR_HIP, std::string("mesh-tree refit launch failed: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(ce);
    for (size_t k = 0; k < set.size(); k++) {
        SrScene::MeshState& a = s->mesh_state[set[k]];
        memcpy(&a.tree.root, &out[k * 8], sizeof(a.tree.root));
        a.tree.host_stale = true;
        a.refit_pending = false; a.refit_now = true; a.last_op = SR_OP_UPDATE;
        srh::as_state_mark_built(a.state, SR_OP_UPDATE);
        s->mu_info.blas_refitted++;
    }
    return SR_OK;
}

// Blas::update / Blas::rebuild (blas.rs:285-310) for the meshes updated since the last sr_scene_set_instances whose build type
// allows it (refit_pending). The op each mesh's own SrAsState picks (or the forced one) decides: SR_OP_UPDATE: the device rewrites
// its leaf-order records and root box and refits its nodes in place; SR_OP_FAST_BUILD: the device builds its tree anew
// (build_mesh_trees_device); both kinds may run in one call, and the concatenated arrays stay current. All or nothing remains
// only towards the HOST: if anything in the call needs it (a slow build, a baked instance in the old or new list, arrays that
// are not resident, mode HOST or a mesh below the auto threshold, a refused device build) every pending mesh's tree is invalidated
// and the build that follows rebuilds them on the host, as it does for a Static mesh. A host rebuild re-concatenates and
// re-uploads every mesh's host copy, so it also takes the meshes an earlier refit or device build left with a stale host copy.
// Runs before two_level_build, which then sees current root boxes and stack needs.
int maintain_mesh_trees(SrScene* s, uint32_t forced) {
    s->mu_info.blas_refitted = 0;
    SrMeshTreeInfo& ti = s->mt_info;
    ti.built_on_device = ti.built_on_host = 0; ti.reason = SR_MESH_TREE_ON_DEVICE; ti.device_build_ms = 0.0;
    s->batch_info.batched = s->batch_info.passed_on = s->batch_info.launches = 0u; s->batch_info.batch_ms = 0.0;
    PendingMeshTrees p;
    classify_pending_mesh_trees(s, forced, p);
    if (!p.any_pending && !p.any_stale) { if (s->static_mesh_updated) ti.reason = SR_MESH_TREE_HOST_STATIC_MESH; return SR_OK; }
    int rc;
    if ((rc = fetch_host_transforms(s, SR_INST_FETCH_MESH_TREES)) != SR_OK) return rc;     // mesh_tree_host_reason tests every instance's transform
    uint32_t reason = mesh_tree_host_reason(s, p);
    if (reason == SR_MESH_TREE_ON_DEVICE && !p.builds.empty() && (rc = build_mesh_trees_device(s, p.builds, &reason)) != SR_OK) return rc;
    if (reason != SR_MESH_TREE_ON_DEVICE) {
        invalidate_mesh_trees(s, true);
        ti.reason = reason;
        if (!p.builds.empty()) s->height_info[SR_TREE_KIND_MESH].on_device = 0u;      // the host takes the trees that asked for a fast build
        return SR_OK;
    }
    if (p.refits.empty()) return SR_OK;
    if (p.refits != s->refit.set && (rc = prepare_refit_set(s, p.refits)) != SR_OK) return rc;
    return refit_mesh_trees(s);
}

// What the build of a sr_scene_set_instances in the two-level form did to every mesh's tree, into the per-mesh heuristic states.
void mark_mesh_trees(SrScene* s, uint32_t forced) {
    for (size_t m = 0; m < s->meshes.size(); m++) {
        if (s->meshes[m].n_vertices == 0) continue;
        SrScene::MeshState& a = s->mesh_state[m];
        if (a.rebuilt_now) {
            const uint32_t op = (!a.built_once || forced == SR_OP_SLOW_BUILD) ? SR_OP_SLOW_BUILD : SR_OP_FAST_BUILD;
            if (a.build_type != SR_BUILD_STATIC && a.built_once) srh::as_state_mark_built(a.state, op);
            a.last_op = op; a.built_once = true;
        } else if (!a.refit_now) {
            if (a.build_type != SR_BUILD_STATIC) srh::as_state_mark_built(a.state, SR_OP_NONE);
            a.last_op = SR_OP_NONE;
        }
        a.rebuilt_now = a.refit_now = false;
    }
}

struct HostTlRecords {                        // what the host record loop computes of an instance list
    std::vector<srd::DevTlInstance> recs;     // one per instance
    std::vector<srh::BuildBox> boxes;         // padded world-space boxes of the instances that have one
    std::vector<SrScene::HostBlas> baked;     // private world-space copies: instances whose transform cannot be inverted (well)
    std::vector<uint32_t> box_inst, baked_inst;   // the instance of every box / baked copy
    uint32_t blas_stack = 0;                  // stack need of the deepest mesh tree or baked copy in use
};
int host_tl_records(SrScene* s, HostTlRecords& h) {
    int rc;
    if ((rc = fetch_host_transforms(s, SR_INST_FETCH_HOST_TOP_LEVEL)) != SR_OK) return rc;
    const size_t ni = s->fid.instances.size();
    h.recs.resize(ni ? ni : 1);
    memset(h.recs.data(), 0, h.recs.size() * sizeof(srd::DevTlInstance));
    h.boxes.reserve(ni); h.box_inst.reserve(ni);
    for (size_t i = 0; i < ni; i++) {
        const srh::HostInstance& in = s->fid.instances[i];
        const SrScene::HostBlas& b = s->mesh_state[in.mesh_slot].tree;
        if (!b.valid) { if ((rc = rebuild_mesh_tree(s, in.mesh_slot)) != SR_OK) return rc; s->trees.blas_device_current = false; }
        srd::DevTlInstance& r = h.recs[i];
        const float* M = in.o2w.m;
        memcpy(r.o2w, M, 48);
        r.tri_offset = in.tri_offset;
        r.mesh_slot = in.mesh_slot;
        if (b.n_tris == 0) continue;
        srh::BuildBox bx;
        // the record's arithmetic is tl_record.h's, shared with the device build. An instance whose transform cannot be inverted
        // (well) gets a private world-space copy of its mesh's tree and is walked without a ray transform
        if (srd::tl_record(M, b.root.lo, b.root.hi, b.root.max_abs_vertex, b.root.max_edge_sum, kTlMaxCondition, r.w2o, bx.lo, bx.hi, &r.pad_a, &r.pad_b) == srd::kTlRecordBaked) {
            memset(r.w2o, 0, sizeof(r.w2o));
            r.w2o[0] = r.w2o[5] = r.w2o[10] = 1.0f;
            r.flags = 1u;
            h.baked.emplace_back();
            if ((rc = build_blas(s, in.mesh_slot, &in.o2w, h.baked.back())) != SR_OK) return rc;
            h.baked_inst.push_back((uint32_t)i);
            const SrScene::HostBlas& wb = h.baked.back();
            bool box_ok = true;
            for (int a = 0; a < 3; a++) { bx.lo[a] = wb.root.lo[a]; bx.hi[a] = wb.root.hi[a]; box_ok = box_ok && std::isfinite(bx.lo[a]) && std::isfinite(bx.hi[a]); }
            h.blas_stack = std::max(h.blas_stack, wb.max_stack);
            if (box_ok) { h.boxes.push_back(bx); h.box_inst.push_back((uint32_t)i); }
            continue;
        }
        h.blas_stack = std::max(h.blas_stack, b.max_stack);
        // a box that is not finite goes to the builder like any other (the device path leaves such a list to this loop)
        h.boxes.push_back(bx);
        h.box_inst.push_back((uint32_t)i);
    }
    return SR_OK;
}
// Where each record's tree starts in the concatenated arrays, once these stand as the build leaves them.
void patch_tl_records(const SrScene* s, HostTlRecords& h) {
    for (size_t i = 0; i < s->fid.instances.size(); i++) {
        srd::DevTlInstance& r = h.recs[i];
        if (r.flags & 1u) continue;
        r.blas_root = s->mesh_state[r.mesh_slot].node_base;
        r.prim_base = s->mesh_state[r.mesh_slot].tri_base;
    }
    for (size_t k = 0; k < h.baked.size(); k++) { h.recs[h.baked_inst[k]].blas_root = s->trees.tl_baked_node_base[k]; h.recs[h.baked_inst[k]].prim_base = s->trees.tl_baked_tri_base[k]; }
}

// The two-level structure of the instance list at hand: on the device where top_level_build_device takes a changed list; else the host's
// records, the concatenated mesh trees anew where they are not current or hold (or get) baked copies, and the host's top-level tree.
int two_level_build(SrScene* s, bool list_changed) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    bool any_textured = false;
    if ((rc = upload_mesh_tables(s, &any_textured)) != SR_OK) return rc;
    SrTopLevelInfo info{};
    info.reason = SR_TL_HOST_QUALITY_BUILD;
    if (list_changed) {
        info.reason = SR_TL_ON_DEVICE;
        if ((rc = top_level_build_device(s, t0, &info.reason)) != SR_OK) return rc;
        if (info.reason == SR_TL_ON_DEVICE) return SR_OK;
    }
    HostTlRecords h;
    if ((rc = host_tl_records(s, h)) != SR_OK) return rc;
    if (!s->trees.blas_device_current || !s->two_level || s->trees.tl_baked || !h.baked.empty()) {
        if ((rc = upload_mesh_trees(s, h.baked)) != SR_OK) return rc;
    }
    patch_tl_records(s, h);
    const uint32_t left = tl_stack_left(h.blas_stack);
    if (left < min_depth_for(h.boxes.size())) return fail(SR_ERR_UNSUPPORTED, "two-level structure: instance count and mesh size together need a deeper traversal stack than the kernels provide");
    info.records_ms = ms_between(t0, std::chrono::steady_clock::now());
    srh::BvhResult tl;
    srh::build_bvh_boxes(h.boxes, std::min(depth_for(h.boxes.size()), left), tl);
    std::vector<uint32_t> tl_inst(tl.order.size() ? tl.order.size() : 1, 0u);
    for (size_t k = 0; k < tl.order.size(); k++) tl_inst[k] = h.box_inst[tl.order[k]];
    if (tl_stack_need(tl.max_stack, h.blas_stack) > kTlStackCap) return fail(SR_ERR_STATE, "two-level structure needs a deeper traversal stack than the kernels provide");
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = upload_instance_tables(s)) != SR_OK) return rc;
    if ((rc = s->d_nodes.upload(tl.nodes.data(), tl.nodes.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_tl_inst.upload(tl_inst.data(), tl_inst.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_tl_instances.upload(h.recs.data(), h.recs.size() * sizeof(srd::DevTlInstance))) != SR_OK) return rc;
    const size_t ni = s->fid.instances.size();
    info.n_nodes = tl.n_nodes; info.n_boxes = (uint32_t)h.boxes.size(); info.n_instances = (uint32_t)ni; info.max_stack = tl.max_stack; info.blas_stack = h.blas_stack;
    info.tree_ms = tl.build_ms;
    publish_two_level(s, info, tl.max_depth, tl.sah_cost, t0);
    s->tl_boxes_host.assign((ni ? ni : 1) * 6, std::numeric_limits<float>::quiet_NaN());
    for (size_t k = 0; k < h.boxes.size(); k++) { memcpy(&s->tl_boxes_host[(size_t)h.box_inst[k] * 6], h.boxes[k].lo, 12); memcpy(&s->tl_boxes_host[(size_t)h.box_inst[k] * 6 + 3], h.boxes[k].hi, 12); }
    return SR_OK;
}

// The form this instance list is built in: on request, or (auto) where instancing really shares geometry and the flattened copy
// would be large — more than 2^24 flattened triangles and at least four times the meshes' own.
bool wants_two_level(const SrScene* s) {
    if (s->instancing == SR_INSTANCING_TWO_LEVEL) return true;
    if (s->instancing == SR_INSTANCING_FLAT) return false;
    uint64_t own = 0;
    std::vector<char> seen(s->meshes.size(), 0);
    for (const auto& in : s->fid.instances) if (!seen[in.mesh_slot]) { seen[in.mesh_slot] = 1; own += s->meshes[in.mesh_slot].n_indices / 3; }
    return s->fid.n_triangles > (1u << 24) && (uint64_t)s->fid.n_triangles >= 4ull * own;
}

// OpType::FastBuild: linear BVH built on the device (bvh_gpu.hip). Falls back to the host builder for small scenes
// and for trees that would need a deeper traversal stack than one workgroup's LDS share.
constexpr uint32_t kDeviceBuildMinTris = 4096;
constexpr uint32_t kDeviceStackCap = 47;
int fast_build(SrScene* s) {
    const uint32_t n = s->fid.n_triangles;
    if (n < kDeviceBuildMinTris) return full_build(s);
    const auto t0 = std::chrono::steady_clock::now();
    int rc;
    HIP_TRY(hipDeviceSynchronize());
    bool any_textured = false;
    if ((rc = upload_mesh_tables(s, &any_textured)) != SR_OK) return rc;
    if ((rc = upload_instance_tables(s)) != SR_OK) return rc;
    if ((rc = s->d_mesh_infos.upload(s->mesh_infos.data(), s->mesh_infos.size() * sizeof(SrMeshInfo))) != SR_OK) return rc;
    const uint32_t node_cap = n + 1024;   // inner nodes of a tree with >= 2 children per node and >= 1 triangle per leaf: < n
    if ((rc = s->d_nodes.reserve((size_t)node_cap * srl::kNodeBytes)) != SR_OK || (rc = s->d_node_box.reserve((size_t)node_cap * 24)) != SR_OK ||
        (rc = s->d_tris.reserve((size_t)n * 48)) != SR_OK || (rc = s->d_shade.reserve((size_t)n * 48)) != SR_OK ||
        (rc = s->d_slot_of_gid.reserve((size_t)n * 4)) != SR_OK) return rc;
    if (any_textured) { if ((rc = s->d_shade_tex.reserve((size_t)n * 96)) != SR_OK) return rc; }
    else s->d_shade_tex.release();
    if ((rc = s->d_scratch.reserve(srk_lbvh_scratch_bytes(n, node_cap, s->fast_build_ploc))) != SR_OK) return rc;
    const TreeBuildTarget target((float4*)s->d_nodes.p, node_cap, (float*)s->d_node_box.p, s->d_scratch.p, s->d_scratch.bytes, (uint32_t)srd::kStackMax,
                                 kDeviceStackCap, s->height_bound == SR_HEIGHT_BOUND_REBALANCE, s->fast_build_ploc);
    const TrisBuildArgs a(target, (const SrMeshInfo*)s->d_mesh_infos.p, (const srd::FlatInstance*)s->d_flat_instances.p, (uint32_t)s->fid.instances.size(), n,
                          (float4*)s->d_tris.p, (float4*)s->d_shade.p, (float4*)s->d_shade_tex.p, (uint32_t*)s->d_slot_of_gid.p);
    LbvhResult r;
    const int e = srk_lbvh_build(a, &r, nullptr);
    if (e > 0) return fail(SR_ERR_HIP, std::string("device BVH build failed: ") + hipGetErrorString((hipError_t)e));
    note_tree_height(s, SR_TREE_KIND_ONE_LEVEL, kDeviceStackCap, r, e == 0);
    if (e < 0) return full_build(s);                      // tree outside the limits: quality build on the host instead
    std::vector<uint32_t> level_nodes;
    s->level_offsets.assign(1, 0u);
    for (size_t l = r.level_ranges.size(); l-- > 0;) {
        for (uint32_t k = 0; k < r.level_ranges[l].second; k++) level_nodes.push_back(r.level_ranges[l].first + k);
        s->level_offsets.push_back((uint32_t)level_nodes.size());
    }
    if ((rc = s->d_level_nodes.upload(level_nodes.data(), level_nodes.size() * 4)) != SR_OK) return rc;
    s->shape.resize(s->fid.instances.size());
    for (size_t i = 0; i < s->shape.size(); i++) s->shape[i] = s->fid.instances[i].mesh_slot;
    BuiltStructure built;
    built.n_nodes = r.n_nodes; built.tri_bytes = (uint64_t)n * 48;
    built.max_depth = r.max_depth; built.stack_need = r.max_stack;
    built.build_ms = ms_between(t0, std::chrono::steady_clock::now());
    built.on_device = true;
    publish(s, built);
    return SR_OK;
}

const char* const kNonFiniteTransform = "frame_instance_data: instance transform holds a non-finite value";

// What both sr_scene_set_instances entry points refuse first, with one text each, sizes in 64 bits: the instance count into *n_inst.
int check_instance_list(const SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const void* transforms, uint64_t* n_inst) {
    if (!s || (n_keys && (!keys || !counts))) return fail(SR_ERR_INVALID_ARG, "frame_instance_data: null argument");
    uint64_t n_tri = 0;
    srh::instance_list_sizes(s->meshes, s->slots, keys, counts, n_keys, n_inst, &n_tri);
    if (*n_inst && !transforms) return fail(SR_ERR_INVALID_ARG, "frame_instance_data: transforms is null but instances were given");
    std::string err;
    const int rc = srh::instance_list_limits(*n_inst, n_tri, s->instancing == SR_INSTANCING_FLAT, err);
    return rc == SR_OK ? SR_OK : fail(rc, err);
}

bool same_instance_layout(const SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys) {
    const SrScene::InstanceSource& in = s->inst;
    return in.layout_valid && in.keys.size() == n_keys && (n_keys == 0 || (memcmp(in.keys.data(), keys, 8 * (size_t)n_keys) == 0 && memcmp(in.counts.data(), counts, 4 * (size_t)n_keys) == 0));
}
// `fid` now holds the layout of these keys and counts: what the device's copy of the layout is worth, and the record of it.
void note_instance_layout(SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys) {
    if (same_instance_layout(s, keys, counts, n_keys)) return;
    s->inst.keys.assign(keys, keys + n_keys); s->inst.counts.assign(counts, counts + n_keys);
    s->inst.layout_valid = true; s->inst.layout_on_device = false;
}

int apply_instance_list(SrScene* s);

}  // namespace

// Test hook (tests/node_step_reference.py): the instance record host_tl_records writes for one transform — tl_record with the
// library's baking limit, the same words set around it — without a scene. Host only.
int sr_probe_tl_record(const float* o2w, const float* mesh_lo, const float* mesh_hi, float max_abs_vertex, float max_edge_sum,
                       void* record_out, uint32_t* result_out) {
    if (!o2w || !mesh_lo || !mesh_hi || !record_out || !result_out) return fail(SR_ERR_INVALID_ARG, "sr_probe_tl_record: null pointer");
    srd::DevTlInstance r;
    memset(&r, 0, sizeof(r));
    memcpy(r.o2w, o2w, 48);
    float lo[3], hi[3];
    const srd::TlRecordResult res = srd::tl_record(o2w, mesh_lo, mesh_hi, max_abs_vertex, max_edge_sum, kTlMaxCondition, r.w2o, lo, hi, &r.pad_a, &r.pad_b);
    if (res == srd::kTlRecordBaked) {
        memset(r.w2o, 0, sizeof(r.w2o));
        r.w2o[0] = r.w2o[5] = r.w2o[10] = 1.0f;
        r.flags = 1u;
    }
    memcpy(record_out, &r, sizeof(r));
    *result_out = (uint32_t)res;
    return SR_OK;
}

int sr_scene_set_instances(SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* transforms) {
    uint64_t n_inst = 0;
    int rc = check_instance_list(s, keys, counts, n_keys, transforms, &n_inst);
    if (rc != SR_OK) return rc;
    for (uint64_t i = 0; i < n_inst; i++)
        for (int c = 0; c < 12; c++)
            if (!std::isfinite(transforms[i].m[c])) return fail(SR_ERR_INVALID_ARG, kNonFiniteTransform);
    if ((rc = bind_device(s)) != SR_OK) return rc;
    std::string err;
    srh::FrameInstanceData fid;
    if (!srh::frame_instance_data(s->meshes, s->slots, keys, counts, n_keys, transforms, fid, err)) return fail(SR_ERR_INVALID_ARG, err);
    s->fid = std::move(fid);
    note_instance_layout(s, keys, counts, n_keys);
    s->inst.host_stale = false;
    s->inst.info = SrInstanceUpdateInfo{0, 0, 0, SR_INST_FETCH_NONE, 0, (uint32_t)n_inst, 0xFFFFFFFFu, 0, 0.0, 0.0};
    return apply_instance_list(s);
}

// sr_scene_set_instances for transforms in device memory (header): the host's refusals, the layout where it changed, the kernel
// into the second set of tables with its answer, and only for an accepted call the wait, the exchange of the two sets, the new
// layout into `fid` and everything sr_scene_set_instances does from there (apply_instance_list).
namespace {
int set_instances_device(SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* d_transforms, hipStream_t st) {
    uint64_t n_inst = 0;
    int rc = check_instance_list(s, keys, counts, n_keys, d_transforms, &n_inst);
    if (rc != SR_OK) return rc;
    if ((uintptr_t)d_transforms & 15u) return fail(SR_ERR_INVALID_ARG, "frame_instance_data: the device transform pointer is not 16-byte aligned");
    const bool new_layout = !same_instance_layout(s, keys, counts, n_keys);
    std::string err;
    srh::FrameInstanceData staged;
    if (new_layout && !srh::frame_instance_layout(s->meshes, s->slots, keys, counts, n_keys, staged, err)) return fail(SR_ERR_INVALID_ARG, err);
    if ((rc = bind_device(s)) != SR_OK) return rc;
    if (n_inst && !device_range_of_scene(s, d_transforms, sizeof(SrTransform) * (size_t)n_inst))
        return fail(SR_ERR_INVALID_ARG, "frame_instance_data: the transform pointer is not device memory of the scene's device for that many instances");
    SrScene::InstanceSource& in = s->inst;
    const uint32_t n = (uint32_t)n_inst;
    const bool upload_layout = new_layout || !in.layout_on_device;
    if (upload_layout) {                      // d_layout is read by the kernel alone: a refused call leaves it marked as not current
        const std::vector<srh::HostInstance>& from = new_layout ? staged.instances : s->fid.instances;
        std::vector<srd::InstanceLayout> layout(n);
        for (uint32_t i = 0; i < n; i++) layout[i] = srd::InstanceLayout{from[i].tri_offset, from[i].mesh_slot};
        in.layout_on_device = false;
        if ((rc = in.d_layout.upload(layout.data(), sizeof(srd::InstanceLayout) * (size_t)n)) != SR_OK) return rc;
    }
    const size_t slots = n ? n : 1;           // a list without instances keeps one zero record, as the host's tables do
    if ((rc = in.d_instances_next.reserve(slots * sizeof(srd::DevInstance))) != SR_OK || (rc = in.d_flat_next.reserve(slots * sizeof(srd::FlatInstance))) != SR_OK ||
        (rc = s->d_vertex_check.reserve(16)) != SR_OK) return rc;
    uint32_t first_bad = 0xFFFFFFFFu;
    double tables_ms = 0.0;
    SrTransform first{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
    rc = checked_launch(s, st, 1, &first_bad, &tables_ms, "frame_instance_data: instance table kernel failed: ", [] { return 0; }, [&](uint32_t* check) {
        int e = 0;
        if (n == 0) {
            e = (int)hipMemsetAsync(in.d_instances_next.p, 0, sizeof(srd::DevInstance), st);
            if (e == 0) e = (int)hipMemsetAsync(in.d_flat_next.p, 0, sizeof(srd::FlatInstance), st);
        }
        if (e == 0) e = srk_instance_tables(d_transforms, (const srd::InstanceLayout*)in.d_layout.p, n, (srd::DevInstance*)in.d_instances_next.p, (srd::FlatInstance*)in.d_flat_next.p, check, st);
        if (e == 0 && n) e = (int)hipMemcpyAsync(&first, d_transforms, sizeof(first), hipMemcpyDeviceToHost, st);   // the dummy light record's
        return e;
    });
    if (rc != SR_OK) return rc;
    if (first_bad < n) { in.info.bad_index = first_bad; return fail(SR_ERR_INVALID_ARG, kNonFiniteTransform); }
    HIP_TRY(hipDeviceSynchronize());          // frames in flight read the tables that change places here
    std::swap(s->d_instances, in.d_instances_next);
    std::swap(s->d_flat_instances, in.d_flat_next);
    s->dev.instances = (const srd::DevInstance*)s->d_instances.p;
    if (new_layout) s->fid = std::move(staged);
    note_instance_layout(s, keys, counts, n_keys);
    in.layout_on_device = true;
    if (n) { s->fid.transforms[0] = first; s->fid.instances[0].o2w = first; }
    in.host_stale = n > 0;
    in.info = SrInstanceUpdateInfo{1, n > 0 ? 1u : 0u, 0, SR_INST_FETCH_NONE, upload_layout ? 1u : 0u, n, 0xFFFFFFFFu, 0, tables_ms, 0.0};
    return apply_instance_list(s);
}
}  // namespace

int sr_scene_set_instances_device(SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* d_transforms, void* stream) {
    return set_instances_device(s, keys, counts, n_keys, d_transforms, (hipStream_t)stream);
}

namespace {
// Everything that follows the instance list in `fid`, whichever entry point put it there: the light table's source, the form,
// mesh-tree maintenance and the top-level build, or the one-level op the heuristic picks.
int apply_instance_list(SrScene* s) {
    int rc;
    // meshes updated since the structure last took their vertices (sr_scene_update_mesh): every path below applies them
    const bool reshade = s->geometry_stale;
    s->mu_info.dirty_meshes = (uint32_t)std::count_if(s->mesh_state.begin(), s->mesh_state.end(), [](const SrScene::MeshState& ms) { return ms.dirty; });
    s->mu_info.reshaded = 0; s->mu_info.blas_rebuilt = 0; s->mu_info.blas_refitted = 0;
    s->mu_info.tables_ms = s->mu_info.flatten_ms = s->mu_info.refit_ms = s->mu_info.blas_build_ms = 0.0;
    auto built_with = [s](uint32_t op) {      // how either form ends: the scene's heuristic state takes the op, the updates count as applied
        if (s->built_once) srh::as_state_mark_built(s->as_state, op);
        s->built_once = true; s->last_op = op;
        for (auto& ms : s->mesh_state) ms.dirty = false;
        s->geometry_stale = false; s->static_mesh_updated = false;
        return SR_OK;
    };
    // the light table's source: the device arena (SR_LIGHTS_DEVICE; upload_instance_tables builds the table with the kernel, and
    // the copy below is skipped: sr_scene_get_tables reads the device arena back when asked) or this frame's copy of the host
    // arena. The one dummy record of an empty arena, and of a scene without instances, is host arithmetic in either mode.
    s->lights_on_device = s->emissive_table_stale = s->light_mode == SR_LIGHTS_DEVICE && !s->emissive_tris.empty() && !s->fid.instances.empty();
    { const uint32_t fetches = s->lt_info.arena_fetches; memset(&s->lt_info, 0, sizeof(s->lt_info)); s->lt_info.arena_fetches = fetches; }
    if (!s->lights_on_device) {
        if ((rc = refresh_host_arena(s)) != SR_OK) return rc;
        s->emissive_table = s->emissive_tris;
        if (s->emissive_table.empty()) { SrEmissiveTriangle z; memset(&z, 0, sizeof(z)); s->emissive_table.push_back(z); }
    }
    // Two-level form (a tree per mesh + a top-level tree over the instances): on request or where the flattened copy would be
    // large. A changed instance list is then a top-level rebuild, reported as a fast build (Tlas::queue_build rebuilds in kind).
    if (wants_two_level(s) || s->fid.n_triangles >= (1u << 28)) {
        const uint32_t op = s->built_once ? SR_OP_FAST_BUILD : SR_OP_SLOW_BUILD;
        const uint32_t forced = s->forced_op;
        s->forced_op = SR_OP_NONE;
        if (!s->two_level) s->built = false;
        if ((rc = maintain_mesh_trees(s, forced)) != SR_OK) { s->built = false; return rc; }      // updatable meshes: Blas::update / Blas::rebuild on the device
        rc = two_level_build(s, true);
        if (rc != SR_OK) { s->built = false; return rc; }
        mark_mesh_trees(s, forced);
        s->mt_info.built_on_host = s->mu_info.blas_rebuilt - s->mt_info.built_on_device;
        return built_with(op);
    }
    invalidate_mesh_trees(s, true);           // the one-level form has no mesh trees to refit
    if (s->two_level) {                       // back to the one-level form: everything is rebuilt
        s->two_level = false; s->built = false;
        s->forced_op = s->forced_op == SR_OP_NONE ? SR_OP_SLOW_BUILD : s->forced_op;
    }
    // Tlas::queue_build (tlas.rs:155-191): the instance data is new, so the heuristic is asked with inputs_changed =
    // true; an UPDATE needs the same instance layout (here: the same mesh per instance and unchanged meshes),
    // anything else is a rebuild. The very first build is the quality build (Tlas::new).
    bool can_update = s->built && s->shape.size() == s->fid.instances.size() && s->fid.n_triangles > 0;
    for (size_t i = 0; can_update && i < s->shape.size(); i++) can_update = s->shape[i] == s->fid.instances[i].mesh_slot;
    uint32_t op;
    if (!s->built_once) op = SR_OP_SLOW_BUILD;
    else {
        op = srh::as_state_next_op(s->as_state, true);
        if (op == SR_OP_UPDATE && !can_update) op = SR_OP_FAST_BUILD;
    }
    if (s->forced_op != SR_OP_NONE) { op = (s->forced_op == SR_OP_UPDATE && !can_update) ? SR_OP_FAST_BUILD : s->forced_op; s->forced_op = SR_OP_NONE; }
    rc = op == SR_OP_UPDATE ? update_in_place(s, reshade) : op == SR_OP_FAST_BUILD ? fast_build(s) : full_build(s);
    if (rc != SR_OK) { s->built = false; return rc; }
    return built_with(op);
}
}  // namespace

int sr_scene_instance_update_info(const SrScene* s, SrInstanceUpdateInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_instance_update_info: null argument");
    *out = s->inst.info;
    return SR_OK;
}

int sr_scene_read_instance_tables(const SrScene* s, void* dev_instances, void* flat_instances) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_instance_tables: scene is null");
    if (!s->built) return fail(SR_ERR_STATE, "sr_scene_read_instance_tables: call sr_scene_set_instances first");
    const size_t n = s->fid.instances.size();
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    if (dev_instances && n) HIP_TRY(hipMemcpy(dev_instances, s->d_instances.p, n * sizeof(srd::DevInstance), hipMemcpyDeviceToHost));
    if (flat_instances && n) HIP_TRY(hipMemcpy(flat_instances, s->d_flat_instances.p, n * sizeof(srd::FlatInstance), hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_instance_tables_host(const SrTransform* transforms, uint32_t n, void* dev_instances) {
    if (n && (!transforms || !dev_instances)) return fail(SR_ERR_INVALID_ARG, "sr_instance_tables_host: null argument");
    srh::instance_tables_host(transforms, n, (float*)dev_instances);
    return SR_OK;
}

int sr_scene_end_frame(SrScene* s) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_end_frame: scene is null");
    if (!s->built) { s->last_op = SR_OP_NONE; return SR_OK; }
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string("sr_scene_end_frame: ") + kStaleGeometry);
    const uint32_t op = srh::as_state_next_op(s->as_state, false);
    // two-level form: a quiet frame for every updatable mesh as well (Blas::plan_op with inputs_changed = false); one that asks
    // for its settle rebuild has its tree invalidated, and the build below rebuilds it on the host
    bool mesh_settles = false;
    std::vector<uint32_t> mesh_ops;
    if (s->two_level) {
        mesh_ops.assign(s->meshes.size(), SR_OP_NONE);
        for (size_t m = 0; m < s->meshes.size(); m++) {
            SrScene::MeshState& a = s->mesh_state[m];
            a.rebuilt_now = a.refit_now = false;
            if (s->meshes[m].n_vertices == 0 || a.build_type == SR_BUILD_STATIC || !a.built_once || a.refit_pending) continue;
            mesh_ops[m] = srh::as_state_next_op(a.state, false);
            if (mesh_ops[m] == SR_OP_SLOW_BUILD) { invalidate_mesh_tree(s, (uint32_t)m); mesh_settles = true; }
        }
    }
    if (op == SR_OP_SLOW_BUILD || mesh_settles) {
        int rc = bind_device(s);
        if (rc != SR_OK) return rc;
        if (s->lights_on_device && (rc = fetch_emissive_table(s)) != SR_OK) return rc;   // the rebuild may move the device arena on (a pending mesh)
        if ((rc = fetch_host_transforms(s, SR_INST_FETCH_SETTLE)) != SR_OK) return rc;   // both rebuilds are the host's
        if (s->two_level && !s->trees.blas_device_current) invalidate_mesh_trees(s, false);      // the re-concatenation takes the stale host copies of refitted meshes along
        if ((rc = s->two_level ? two_level_build(s, false) : full_build(s)) != SR_OK) { s->built = false; return rc; }
    }
    for (size_t m = 0; m < mesh_ops.size(); m++) {
        SrScene::MeshState& a = s->mesh_state[m];
        if (s->meshes[m].n_vertices == 0) continue;
        if (a.build_type != SR_BUILD_STATIC && a.built_once && !a.refit_pending) {
            const uint32_t done = a.rebuilt_now ? SR_OP_SLOW_BUILD : mesh_ops[m];     // rebuilt along with a settling mesh: a quality build too
            srh::as_state_mark_built(a.state, done);
            a.last_op = done;
        } else a.last_op = a.rebuilt_now ? SR_OP_SLOW_BUILD : SR_OP_NONE;
        a.rebuilt_now = false;
    }
    srh::as_state_mark_built(s->as_state, op);
    s->last_op = op;
    return SR_OK;
}

int sr_scene_set_instancing(SrScene* s, uint32_t mode) {
    if (!s || mode > SR_INSTANCING_TWO_LEVEL) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_instancing: bad argument");
    s->instancing = (int)mode;
    return SR_OK;
}
int sr_scene_instancing(const SrScene* s, uint32_t* mode, uint32_t* two_level_now) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_instancing: scene is null");
    if (mode) *mode = (uint32_t)s->instancing;
    if (two_level_now) *two_level_now = (s->built && s->two_level) ? 1u : 0u;
    return SR_OK;
}

int sr_scene_set_top_level_build(SrScene* s, uint32_t mode) {
    if (!s || mode > SR_TL_BUILD_DEVICE) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_top_level_build: bad argument");
    s->tl_build_mode = (int)mode;
    return SR_OK;
}
int sr_scene_top_level_info(const SrScene* s, SrTopLevelInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_top_level_info: null argument");
    *out = s->tl_info;
    out->mode = (uint32_t)s->tl_build_mode;
    out->auto_threshold = kTlDeviceMinBoxes;
    if (!(s->built && s->two_level)) {       // nothing stands in the two-level form: the figures of an earlier build do not apply
        const uint32_t mode = out->mode;
        memset(out, 0, sizeof(*out));
        out->mode = mode; out->auto_threshold = kTlDeviceMinBoxes; out->reason = SR_TL_HOST_NOT_TWO_LEVEL;
    }
    return SR_OK;
}
int sr_scene_set_mesh_tree_batch(SrScene* s, uint32_t mode) {
    if (mode > SR_BLAS_BATCH_ON) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_tree_batch: mode must be SR_BLAS_BATCH_OFF or SR_BLAS_BATCH_ON");
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_tree_batch: scene is null");
    s->blas_batch_mode = mode;
    return SR_OK;
}

int sr_scene_mesh_tree_batch_info(const SrScene* s, SrMeshTreeBatchInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_tree_batch_info: scene or out is null");
    *out = s->batch_info;
    out->mode = s->blas_batch_mode; out->max_tris = SR_BLAS_BATCH_MAX_TRIS; out->reserved = 0u;
    return SR_OK;
}

int sr_scene_set_mesh_tree_build(SrScene* s, uint32_t mode) {
    if (mode > SR_MESH_TREE_BUILD_DEVICE) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_tree_build: mode must be SR_MESH_TREE_BUILD_AUTO, _HOST or _DEVICE");
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_tree_build: scene is null");
    s->blas_build_mode = (int)mode;
    return SR_OK;
}
int sr_scene_mesh_tree_info(const SrScene* s, SrMeshTreeInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_tree_info: null argument");
    *out = s->mt_info;
    out->mode = (uint32_t)s->blas_build_mode;
    out->auto_threshold = blas_device_min_tris(s);
    return SR_OK;
}
int sr_scene_set_light_table_build(SrScene* s, uint32_t mode) {
    if (mode > SR_LIGHTS_DEVICE) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_light_table_build: mode must be SR_LIGHTS_HOST or SR_LIGHTS_DEVICE");
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_light_table_build: scene is null");
    if (mode == SR_LIGHTS_HOST && s->light_mode == SR_LIGHTS_DEVICE) {      // the host arena takes over: its stale slots from the device arena
        int rc = bind_device(s);
        if (rc != SR_OK || (rc = fetch_emissive_table(s)) != SR_OK || (rc = refresh_host_arena(s)) != SR_OK) return rc;
        s->lights_on_device = false;                          // a rebuild by sr_scene_end_frame reads emissive_table, which is current now
    }
    s->light_mode = (int)mode;
    return SR_OK;
}
int sr_scene_light_table_info(const SrScene* s, SrLightTableInfo* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_light_table_info: null argument");
    *out = s->lt_info;
    out->mode = (uint32_t)s->light_mode;
    return SR_OK;
}
int sr_scene_read_lights(const SrScene* s, float* out, uint32_t cap_lights, uint32_t* n_lights) {
    if (!s || !n_lights || (!out && cap_lights)) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_lights: null argument");
    if (!s->built) return fail(SR_ERR_STATE, "sr_scene_read_lights: call sr_scene_set_instances first");
    *n_lights = s->dev.num_lights;
    const size_t n = std::min(cap_lights, s->dev.num_lights);
    if (n == 0) return SR_OK;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, s->d_lights.p, n * 64, hipMemcpyDeviceToHost));
    return SR_OK;
}
int sr_light_table(const SrTransform* transforms, uint32_t n_transforms, const SrEmissiveIndirectionEntry* entries, uint32_t n_entries,
                   const SrEmissiveTriangle* triangles, uint32_t n_triangles, float* out) {
    if (!transforms || !entries || !triangles || !out) return fail(SR_ERR_INVALID_ARG, "sr_light_table: null argument");
    for (uint32_t i = 0; i < n_entries; i++)
        if (entries[i].blas_tri_index >= n_triangles || entries[i].entity_id >= n_transforms) {
            char buf[200];
            snprintf(buf, sizeof(buf), "sr_light_table: entry %u names triangle %u of %u, transform %u of %u", i, entries[i].blas_tri_index, n_triangles,
                     entries[i].entity_id, n_transforms);
            return fail(SR_ERR_INVALID_ARG, buf);
        }
    srh::FrameInstanceData fid;
    fid.transforms.assign(transforms, transforms + n_transforms);
    fid.emissive_entries.assign(entries, entries + n_entries);
    const std::vector<SrEmissiveTriangle> tris(triangles, triangles + n_triangles);
    std::vector<float> lights;
    srh::light_table(fid, tris, lights);
    memcpy(out, lights.data(), lights.size() * 4);
    return SR_OK;
}
int sr_scene_set_tree_height_bound(SrScene* s, uint32_t mode, uint32_t mesh_tree_cap) {
    if (mode > SR_HEIGHT_BOUND_REBALANCE) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tree_height_bound: mode must be SR_HEIGHT_BOUND_REFUSE or SR_HEIGHT_BOUND_REBALANCE");
    if (mesh_tree_cap > kBlasStackCap) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tree_height_bound: mesh_tree_cap must be 0 (the library's 26) or 1..26");
    if (mesh_tree_cap != 0 && mode == SR_HEIGHT_BOUND_REFUSE) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tree_height_bound: a mesh_tree_cap needs SR_HEIGHT_BOUND_REBALANCE");
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tree_height_bound: scene is null");
    s->height_bound = mode; s->mesh_tree_cap = mesh_tree_cap;
    for (SrScene::MeshState& ms : s->mesh_state) ms.device_refused = -1;      // a refusal held for the mode and cap it was made under
    return SR_OK;
}
int sr_scene_tree_height_info(const SrScene* s, uint32_t kind, SrTreeHeightInfo* out) {
    if (kind > SR_TREE_KIND_MESH) return fail(SR_ERR_INVALID_ARG, "sr_scene_tree_height_info: kind must be SR_TREE_KIND_ONE_LEVEL, _TOP_LEVEL or _MESH");
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_tree_height_info: null argument");
    *out = s->height_info[kind];
    out->mode = s->height_bound; out->mesh_tree_cap = s->mesh_tree_cap;
    if (!s->built) out->on_device = 0u;
    return SR_OK;
}
int sr_scene_read_top_level(const SrScene* s, uint32_t* nodes, uint32_t* tl_inst, void* records, float* boxes) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_top_level: scene is null");
    if (!s->built || !s->two_level) return fail(SR_ERR_STATE, "sr_scene_read_top_level: the scene is not built in the two-level form");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    const SrTopLevelInfo& info = s->tl_info;
    if (nodes && info.n_nodes) HIP_TRY(hipMemcpy(nodes, s->d_nodes.p, (size_t)info.n_nodes * srl::kNodeBytes, hipMemcpyDeviceToHost));
    if (tl_inst && info.n_boxes) HIP_TRY(hipMemcpy(tl_inst, s->d_tl_inst.p, (size_t)info.n_boxes * 4, hipMemcpyDeviceToHost));
    if (records && info.n_instances) HIP_TRY(hipMemcpy(records, s->d_tl_instances.p, (size_t)info.n_instances * sizeof(srd::DevTlInstance), hipMemcpyDeviceToHost));
    if (boxes && info.n_instances) {
        if (info.on_device) HIP_TRY(hipMemcpy(boxes, s->d_tl_boxes.p, (size_t)info.n_instances * 24, hipMemcpyDeviceToHost));
        else memcpy(boxes, s->tl_boxes_host.data(), (size_t)info.n_instances * 24);
    }
    return SR_OK;
}

int sr_scene_force_next_op(SrScene* s, uint32_t op) {
    if (!s || op > SR_OP_UPDATE) return fail(SR_ERR_INVALID_ARG, "sr_scene_force_next_op: bad argument");
    s->forced_op = op;
    return SR_OK;
}

int sr_scene_as_state(const SrScene* s, SrAsState* state, uint32_t* last_op) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_as_state: scene is null");
    if (state) *state = s->as_state;
    if (last_op) *last_op = s->last_op;
    return SR_OK;
}

int sr_scene_set_mesh_build_type(SrScene* s, uint64_t key, uint32_t build_type) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_build_type: scene is null");
    if (build_type > SR_BUILD_STATIC) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_mesh_build_type: build type must be SR_BUILD_RAPIDLY_CHANGING, SR_BUILD_SOMETIMES_CHANGES or SR_BUILD_STATIC");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_set_mesh_build_type", &slot); rc != SR_OK) return rc;
    SrScene::MeshState& a = s->mesh_state[slot];
    if (build_type == SR_BUILD_STATIC && a.refit_pending) invalidate_mesh_tree(s, slot);       // a Static mesh is never refitted: its pending update becomes a rebuild
    a.build_type = build_type;
    srh::as_state_initial(build_type, &a.state);
    return SR_OK;
}

int sr_scene_mesh_as_state(const SrScene* s, uint64_t key, uint32_t* build_type, SrAsState* state, uint32_t* last_op) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_mesh_as_state: scene is null");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_mesh_as_state", &slot); rc != SR_OK) return rc;
    const SrScene::MeshState& a = s->mesh_state[slot];
    if (build_type) *build_type = a.build_type;
    if (state) *state = a.state;
    if (last_op) *last_op = a.last_op;
    return SR_OK;
}

int sr_scene_read_mesh_tree(const SrScene* s, uint64_t key, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* nodes, float* tris, float* shade,
                            float* shade_tex, uint32_t* slot_of_prim) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_mesh_tree: scene is null");
    uint32_t slot = 0;
    if (const int rc = find_mesh(s, key, "sr_scene_read_mesh_tree", &slot); rc != SR_OK) return rc;
    if (!s->built || !s->two_level) return fail(SR_ERR_STATE, "sr_scene_read_mesh_tree: the scene is not built in the two-level form");
    const SrScene::MeshState& ms = s->mesh_state[slot];
    if (!s->trees.blas_device_current || !ms.tree.valid)
        return fail(SR_ERR_STATE, "sr_scene_read_mesh_tree: the mesh's tree is not on the device (sr_scene_set_instances builds it)");
    if (s->geometry_stale || ms.refit_pending) return fail(SR_ERR_STATE, std::string("sr_scene_read_mesh_tree: ") + kStaleGeometry);
    const uint32_t nb = ms.node_base, tb = ms.tri_base, nn = ms.tree.n_nodes, nt = ms.tree.n_tris;
    if (n_nodes) *n_nodes = nn;
    if (n_tris) *n_tris = nt;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    if (nodes && nn) {
        HIP_TRY(hipMemcpy(nodes, (const char*)s->trees.d_blas_nodes.p + (size_t)nb * srl::kNodeBytes, (size_t)nn * srl::kNodeBytes, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < nn; i++)         // references local to the mesh (the inverse of the concatenation)
            for (int c = 0; c < srl::kBvhWidth; c++) {
                uint32_t& q = nodes[(size_t)i * srl::kNodeDwords + srl::kChildOffset + c];
                const int ref = (int)q;
                if (ref >= 0) q = (uint32_t)(ref - (int)nb);
                else { const uint32_t lv = ~(uint32_t)ref; const uint32_t cnt = lv & 7u; if (cnt) q = ~((((lv >> 3) - tb) << 3) | cnt); }
            }
    }
    if (tris && nt) HIP_TRY(hipMemcpy(tris, (const char*)s->d_tris.p + (size_t)tb * 48, (size_t)nt * 48, hipMemcpyDeviceToHost));
    if (shade && nt) HIP_TRY(hipMemcpy(shade, (const char*)s->d_shade.p + (size_t)tb * 48, (size_t)nt * 48, hipMemcpyDeviceToHost));
    if (shade_tex && nt) {
        if (s->trees.any_textured_tl) HIP_TRY(hipMemcpy(shade_tex, (const char*)s->d_shade_tex.p + (size_t)tb * 96, (size_t)nt * 96, hipMemcpyDeviceToHost));
        else memset(shade_tex, 0, (size_t)nt * 96);       // the scene has no textured records
    }
    if (slot_of_prim && nt) {
        HIP_TRY(hipMemcpy(slot_of_prim, (const char*)s->d_slot_of_gid.p + (size_t)tb * 4, (size_t)nt * 4, hipMemcpyDeviceToHost));
        for (uint32_t p = 0; p < nt; p++) slot_of_prim[p] -= tb;
    }
    return SR_OK;
}

void sr_as_state_initial(uint32_t build_type, SrAsState* out) { if (out) srh::as_state_initial(build_type, out); }
uint32_t sr_as_state_next_op(const SrAsState* state, int inputs_changed) { return state ? srh::as_state_next_op(*state, inputs_changed != 0) : SR_OP_NONE; }
void sr_as_state_mark_built(SrAsState* state, uint32_t completed_op) { if (state) srh::as_state_mark_built(*state, completed_op); }

int sr_bvh_layout(uint32_t* width, uint32_t* node_dwords, uint32_t* plane_offset, uint32_t* child_offset) {
    if (width) *width = (uint32_t)srl::kBvhWidth;
    if (node_dwords) *node_dwords = (uint32_t)srl::kNodeDwords;
    if (plane_offset) *plane_offset = (uint32_t)srl::kPlaneOffset;
    if (child_offset) *child_offset = (uint32_t)srl::kChildOffset;
    return SR_OK;
}

int sr_tree_build_limits(uint32_t kind, uint64_t n_prims, uint32_t* leaf_max, uint32_t* stack_floor) {
    if (kind > SR_TREE_KIND_MESH) return fail(SR_ERR_INVALID_ARG, "sr_tree_build_limits: kind must be SR_TREE_KIND_ONE_LEVEL, _TOP_LEVEL or _MESH");
    if (leaf_max) *leaf_max = (uint32_t)srl::kLeafMax;
    if (stack_floor) *stack_floor = kind == SR_TREE_KIND_MESH ? depth_for(n_prims) : kind == SR_TREE_KIND_TOP_LEVEL ? min_depth_for(n_prims) : (uint32_t)srd::kStackMax;
    return SR_OK;
}

int sr_scene_read_bvh(const SrScene* s, uint32_t* nodes_out, float* tris_out) {
    if (!s || !s->built) return fail(SR_ERR_STATE, "sr_scene_read_bvh: scene not built");
    if (s->two_level) return fail(SR_ERR_UNSUPPORTED, "sr_scene_read_bvh: the scene is built in the two-level form");
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string("sr_scene_read_bvh: ") + kStaleGeometry);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    if (nodes_out) HIP_TRY(hipMemcpy(nodes_out, s->d_nodes.p, (size_t)s->stats.n_nodes * srl::kNodeBytes, hipMemcpyDeviceToHost));
    if (tris_out && s->fid.n_triangles) HIP_TRY(hipMemcpy(tris_out, s->d_tris.p, (size_t)s->fid.n_triangles * 48, hipMemcpyDeviceToHost));
    return SR_OK;
}

namespace {
// OpType::SlowBuild / FastBuild: the whole structure from the current instance list.
int full_build(SrScene* s) {
    int rc;
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = fetch_host_transforms(s, SR_INST_FETCH_HOST_BUILD)) != SR_OK) return rc;
    for (const auto& in : s->fid.instances)       // the flatten and the record packing below read the host copies
        if ((rc = fetch_host_vertices(s, in.mesh_slot)) != SR_OK) return rc;
    srh::flatten_instances(s->meshes, s->fid, s->world_tris);
    srh::BvhResult bvh;
    srh::build_bvh(s->world_tris, (uint32_t)srd::kMaxBinaryDepth, bvh);
    if (bvh.max_stack > (uint32_t)srd::kStackMax) return fail(SR_ERR_STATE, "BVH needs a deeper traversal stack than the kernels provide");
    // shade records (object-space vertex normals + instance + mesh slot) in leaf order, slot lookup
    const uint32_t n_tris = s->fid.n_triangles;
    std::vector<float> shade((size_t)n_tris * 12, 0.0f);
    std::vector<uint32_t> slot_of_gid(n_tris ? n_tris : 1, 0u);
    for (uint32_t slot = 0; slot < n_tris; slot++) {
        const srh::BuildTri& t = s->world_tris[bvh.order[slot]];
        const srh::HostInstance& inst = s->fid.instances[t.inst];
        const srh::HostMesh& mesh = s->meshes[inst.mesh_slot];
        float* q = &shade[(size_t)slot * 12];
        for (int j = 0; j < 3; j++) memcpy(q + 3 * j, mesh.vertices[mesh.indices[3 * t.prim + j]].normal, 12);
        memcpy(q + 9, &t.inst, 4);
        memcpy(q + 10, &inst.mesh_slot, 4);
        slot_of_gid[t.gid] = slot;
    }
    bool any_textured = false;
    if ((rc = upload_mesh_tables(s, &any_textured)) != SR_OK) return rc;
    std::vector<float> shade_tex;
    if (any_textured) {
        shade_tex.assign((size_t)n_tris * 24, 0.0f);
        for (uint32_t slot = 0; slot < n_tris; slot++) {
            const srh::BuildTri& t = s->world_tris[bvh.order[slot]];
            const srh::HostMesh& mesh = s->meshes[s->fid.instances[t.inst].mesh_slot];
            const SrVertex* v[3];
            for (int j = 0; j < 3; j++) v[j] = &mesh.vertices[mesh.indices[3 * t.prim + j]];
            pack_shade_tex(&shade_tex[(size_t)slot * 24], v);
        }
    }
    // device upload (synchronous, like the reference's scene-load BLAS build: blas.rs:178)
    HIP_TRY(hipDeviceSynchronize());
    if ((rc = upload_instance_tables(s)) != SR_OK) return rc;
    // inputs of later in-place updates: per-level node lists, exact node boxes (filled by the first refit), mesh table
    std::vector<uint32_t> level_nodes;
    srh::tree_levels(bvh.nodes, level_nodes, s->level_offsets);
    if ((rc = s->d_level_nodes.upload(level_nodes.data(), level_nodes.size() * 4)) != SR_OK) return rc;
    std::vector<float> node_box((size_t)bvh.n_nodes * 6, 0.0f);
    if ((rc = s->d_node_box.upload(node_box.data(), node_box.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_mesh_infos.upload(s->mesh_infos.data(), s->mesh_infos.size() * sizeof(SrMeshInfo))) != SR_OK) return rc;
    s->shape.resize(s->fid.instances.size());
    for (size_t i = 0; i < s->shape.size(); i++) s->shape[i] = s->fid.instances[i].mesh_slot;
    if ((rc = s->d_nodes.upload(bvh.nodes.data(), bvh.nodes.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_tris.upload(bvh.tris.data(), bvh.tris.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_shade.upload(shade.data(), shade.size() * 4)) != SR_OK) return rc;
    if ((rc = s->d_slot_of_gid.upload(slot_of_gid.data(), slot_of_gid.size() * 4)) != SR_OK) return rc;
    if (any_textured) { if ((rc = s->d_shade_tex.upload(shade_tex.data(), shade_tex.size() * 4)) != SR_OK) return rc; }
    else s->d_shade_tex.release();
    BuiltStructure built;
    built.n_nodes = bvh.n_nodes; built.tri_bytes = (uint64_t)s->fid.n_triangles * 48;
    built.max_depth = bvh.max_depth; built.stack_need = bvh.max_stack; built.sah_cost = bvh.sah_cost;
    built.build_ms = bvh.build_ms;
    publish(s, built);
    return SR_OK;
}
}  // namespace

int sr_scene_get_tables(const SrScene* s, const SrTransform** transforms, uint32_t* n_instances,
                        const SrEmissiveIndirectionEntry** indirection, uint32_t* num_lights,
                        const SrEmissiveTriangle** emissive_triangles, uint32_t* n_emissive,
                        const SrMeshInfo** meshes_info, uint32_t* n_meshes) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_get_tables: scene is null");
    if (!s->built) return fail(SR_ERR_STATE, "sr_scene_get_tables: call sr_scene_set_instances first");
    if (emissive_triangles || n_emissive) { const int rc = fetch_emissive_table(const_cast<SrScene*>(s)); if (rc != SR_OK) return rc; }
    if (transforms) { const int rc = fetch_host_transforms(const_cast<SrScene*>(s), SR_INST_FETCH_GET_TABLES); if (rc != SR_OK) return rc; }
    if (transforms) *transforms = s->fid.transforms.data();
    if (n_instances) *n_instances = (uint32_t)s->fid.transforms.size();
    if (indirection) *indirection = s->fid.emissive_entries.data();
    if (num_lights) *num_lights = (uint32_t)s->fid.emissive_entries.size();
    if (emissive_triangles) *emissive_triangles = s->emissive_table.data();
    if (n_emissive) *n_emissive = (uint32_t)s->emissive_table.size();
    if (meshes_info) *meshes_info = s->mesh_infos.data();
    if (n_meshes) *n_meshes = (uint32_t)s->mesh_infos.size();
    return SR_OK;
}

int sr_scene_bvh_stats(const SrScene* s, SrBvhStats* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_bvh_stats: null argument");
    if (!s->built) return fail(SR_ERR_STATE, "sr_scene_bvh_stats: call sr_scene_set_instances first");
    *out = s->stats;
    return SR_OK;
}

int sr_scene_resolve_triangle(const SrScene* s, uint32_t tri, uint32_t* instance, uint32_t* primitive) {
    if (!s || !s->built) return fail(SR_ERR_STATE, "sr_scene_resolve_triangle: scene not built");
    if (tri >= s->fid.n_triangles) return fail(SR_ERR_INVALID_ARG, "sr_scene_resolve_triangle: triangle index out of range");
    size_t lo = 0, hi = s->fid.instances.size();
    while (hi - lo > 1) { size_t mid = (lo + hi) / 2; if (s->fid.instances[mid].tri_offset <= tri) lo = mid; else hi = mid; }
    if (instance) *instance = (uint32_t)lo;
    if (primitive) *primitive = tri - s->fid.instances[lo].tri_offset;
    return SR_OK;
}

static int trace_list(SrScene* s, const SrRay* rays, uint32_t n, SrHit* hits, uint32_t* occluded, int any, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_trace: scene is null");
    if (!s->built) return fail(SR_ERR_STATE, "sr_trace: call sr_scene_set_instances first (TLAS not built)");
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string("sr_trace: ") + kStaleGeometry);
    if (n && (!rays || (any ? (void*)occluded : (void*)hits) == nullptr)) return fail(SR_ERR_INVALID_ARG, "sr_trace: null ray/output pointer");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    if (n > (1u << 31)) return fail(SR_ERR_UNSUPPORTED, "sr_trace: more than 2^31 rays in one call (ray indices are 32-bit)");
    hipStream_t st = (hipStream_t)stream;
    ScopedTiming tm(s, any ? kAny : kClosest, st);
    int e = srk_launch_trace(s->dev, rays, n, hits, occluded, any, s->instrumented, s->two_level ? 1 : 0, s->stack_entries, st);
    if (e != 0) return fail(SR_ERR_HIP, std::string("trace kernel launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}

int sr_trace_closest(const SrScene* s, const SrRay* rays, uint32_t n, SrHit* hits, void* stream) {
    return trace_list(const_cast<SrScene*>(s), rays, n, hits, nullptr, 0, stream);
}
int sr_trace_any(const SrScene* s, const SrRay* rays, uint32_t n, uint32_t* occluded, void* stream) {
    return trace_list(const_cast<SrScene*>(s), rays, n, nullptr, occluded, 1, stream);
}

int sr_shade_closest_hit(const SrScene* s, const SrHit* hits, uint32_t n, SrRayPayload* payloads, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_shade_closest_hit: scene is null");
    if (!s->built) return fail(SR_ERR_STATE, "sr_shade_closest_hit: scene not built");
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string("sr_shade_closest_hit: ") + kStaleGeometry);
    if (n && (!hits || !payloads)) return fail(SR_ERR_INVALID_ARG, "sr_shade_closest_hit: null pointer");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    int e = srk_launch_shade(s->dev, hits, n, payloads, (hipStream_t)stream);
    if (e != 0) return fail(SR_ERR_HIP, std::string("shade kernel launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}

int sr_any_hit_ignores(const SrScene* s, const SrHit* hits, uint32_t n, uint32_t* ignored, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_any_hit_ignores: scene is null");
    if (!s->built) return fail(SR_ERR_STATE, "sr_any_hit_ignores: scene not built");
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string("sr_any_hit_ignores: ") + kStaleGeometry);
    if (n && (!hits || !ignored)) return fail(SR_ERR_INVALID_ARG, "sr_any_hit_ignores: null pointer");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    int e = srk_launch_any_hit(s->dev, hits, n, ignored, (hipStream_t)stream);
    if (e != 0) return fail(SR_ERR_HIP, std::string("any_hit kernel launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}

// The tile-schedule entry of pass `which` and launch rectangle (x0, cols, y0 .. y1): the one this geometry already has, or a
// new one in a free slot / in place of the least recently used entry (costs zeroed on `st`, no order yet). Marks it used now.
static int schedule_entry(SrScene* s, int which, uint32_t x0, uint32_t cols, uint32_t y0, uint32_t y1, hipStream_t st, SrScene::TileSchedule** out) {
    SrScene::TileSchedule* sched = nullptr;
    for (auto& ts : s->schedules) if (ts.which == which && ts.width == cols && ts.x0 == x0 && ts.y0 == y0 && ts.y1 == y1) sched = &ts;
    if (!sched) {
        if (s->schedules.size() < 8) s->schedules.emplace_back();
        sched = &s->schedules[0];
        for (auto& ts : s->schedules) if (ts.which < 0 || ts.last_use < sched->last_use) sched = &ts;
        if (sched->which >= 0) HIP_TRY(hipDeviceSynchronize());            // recycling an entry a launch on ANY stream may still read
        const size_t bytes = (size_t)srk_pass_tile_count(cols, y1 - y0) * 4;
        int rc;
        if ((rc = sched->cost.reserve(bytes)) != SR_OK || (rc = sched->order.reserve((size_t)srk_pass_order_cap(cols, y1 - y0) * 8 * 4)) != SR_OK) return rc;
        HIP_TRY(hipMemsetAsync(sched->cost.p, 0, bytes, st));
        sched->which = which; sched->width = cols; sched->x0 = x0; sched->y0 = y0; sched->y1 = y1; sched->have_order = false; sched->uses = 0;
    }
    sched->last_use = ++s->schedule_clock;
    *out = sched;
    return SR_OK;
}

static int run_pass(const SrRtParams* p, int which, void* stream) {
    const char* name = which == 0 ? "raytracing_ris" : "raytracing_final";
    if (!p || !p->scene) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": params or scene is null");
    SrScene* s = const_cast<SrScene*>(p->scene);
    if (!s->built) return fail(SR_ERR_STATE, std::string(name) + ": TLAS not built (call sr_scene_set_instances)");
    if (s->geometry_stale) return fail(SR_ERR_STATE, std::string(name) + ": " + kStaleGeometry);
    if (p->width == 0 || p->height == 0) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": trace_extent not set");
    if (!p->matrices) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": matrices is null");
    const bool need_restir = p->config.enable_restir != 0;
    if (which == 0 || need_restir) {
        if (!p->depth_img || !p->normal_img || !p->diffuse_img || !p->motion_vec_img)
            return fail(SR_ERR_INVALID_ARG, std::string(name) + ": G-buffer image pointer is null");
        if (!p->reservoirs[0] || !p->reservoirs[1] || !p->reservoirs_gi[0] || !p->reservoirs_gi[1])
            return fail(SR_ERR_INVALID_ARG, std::string(name) + ": reservoir buffer pointer is null");
    }
    if (which == 1) {
        if (!p->raw_color) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": raw_color is null");
        if (!p->blue_noise_tex || p->blue_noise_w == 0 || p->blue_noise_h == 0)
            return fail(SR_ERR_INVALID_ARG, std::string(name) + ": blue-noise texture missing");
    }
    if ((uint64_t)p->width * p->height >= (1ull << 31)) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": extent too large");
    if (p->config.max_bounces > SR_MAX_BOUNCES || p->config.virtual_bounces > SR_MAX_BOUNCES)
        return fail(SR_ERR_INVALID_ARG, std::string(name) + ": max_bounces / virtual_bounces above SR_MAX_BOUNCES");
    uint32_t y0 = 0, y1 = p->height;
    if (p->tile_h) {
        if (p->tile_y0 >= p->height) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": tile outside the image");
        y0 = p->tile_y0;
        y1 = std::min(p->height, p->tile_y0 + p->tile_h);
    }
    uint32_t x0 = 0, x1 = p->width;
    if (p->tile_w) {
        if (p->tile_x0 >= p->width) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": tile outside the image");
        x0 = p->tile_x0;
        x1 = std::min(p->width, p->tile_x0 + p->tile_w);
    }
    const uint32_t cols = x1 - x0;
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    srd::PassArgs a;
    memset(&a, 0, sizeof(a));
    a.sc = s->dev;
    a.mats = *p->matrices;
    a.raw_color = p->raw_color; a.depth_img = p->depth_img; a.normal_img = p->normal_img;
    a.diffuse_img = p->diffuse_img; a.motion_vec_img = p->motion_vec_img;
    a.blue_noise_tex = p->blue_noise_tex; a.blue_noise_w = p->blue_noise_w; a.blue_noise_h = p->blue_noise_h;
    a.reservoirs[0] = p->reservoirs[0]; a.reservoirs[1] = p->reservoirs[1];
    a.reservoirs_gi[0] = p->reservoirs_gi[0]; a.reservoirs_gi[1] = p->reservoirs_gi[1];
    // primary-hit hand-off: written by the RIS pass at virtual bounce 0, read by the final pass at bounce 0 — only where a RIS pass ran
    a.primary_payload = (need_restir && p->config.virtual_bounces > 0) ? p->primary_payload : nullptr;
    a.frame_count = p->frame_count;
    a.width = p->width; a.height = p->height;
    a.y0 = y0; a.y1 = y1; a.x0 = x0; a.x1 = x1;
    a.cfg = p->config;
    a.light_lds_bytes = s->light_stage ? 0xFFFFFFFFu : 0u;   // srk_launch_pass lowers it to the launch's LDS size
    hipStream_t st = (hipStream_t)stream;
    // tile schedule of this launch geometry: order from the previous launch's costs, costs of this launch for the next
    SrScene::TileSchedule* sched = nullptr;
    if (s->tile_scheduling) {
        if ((rc = schedule_entry(s, which, x0, cols, y0, y1, st, &sched)) != SR_OK) return rc;
        a.tile_cost = (uint32_t*)sched->cost.p;
        a.tile_order = sched->have_order ? (const uint32_t*)sched->order.p : nullptr;
    }
    int e;
    PassLabel label(name);
    {
        ScopedTiming tm(s, which == 0 ? kRis : kFinal, st);      // times the pass kernel only
        e = srk_launch_pass(a, which, s->instrumented, s->dev.shade_tex != nullptr, s->two_level ? 1 : 0, s->stack_entries, st);
    }
    if (e != 0) return fail(SR_ERR_HIP, std::string(name) + " launch: " + hipGetErrorString((hipError_t)e));
    // The schedule changes rarely (it follows where the expensive rows and columns are): re-derive it after the first launches
    // of a geometry and then every 64th, not after every launch (the kernel is eight workgroups of mostly serial work,
    // 70-100 us at 1080p, in the stream between two passes: every 16th launch cost 1.3 % of the bench's frame time).
    if (sched && (sched->uses++ < 4 || (sched->uses & 63u) == 0u)) {
        e = srk_launch_tile_order((const uint32_t*)sched->cost.p, (uint32_t*)sched->order.p, cols, y1 - y0, st);
        if (e != 0) return fail(SR_ERR_HIP, std::string(name) + " tile schedule: " + hipGetErrorString((hipError_t)e));
        sched->have_order = true;
    }
    return SR_OK;
}

// Measured cost (shader cycles summed over the tiles of each 8-pixel tile row) of the last launch of pass `which` with
// this geometry: what the tile schedule is derived from; tile-parallel hosts use it to cut strips of equal cost.
int sr_scene_read_tile_row_costs(SrScene* s, int which, uint32_t width, uint32_t y0, uint32_t rows, double* out, uint32_t cap, uint32_t* n_tile_rows) {
    if (!s || !out || !n_tile_rows) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_row_costs: null argument");
    SrScene::TileSchedule* sched = nullptr;
    for (auto& ts : s->schedules) if (ts.which == which && ts.width == width && ts.x0 == 0 && ts.y0 == y0 && ts.y1 == y0 + rows) sched = &ts;
    if (!sched) return fail(SR_ERR_STATE, "sr_scene_read_tile_row_costs: no launch of this pass with this geometry yet");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    const uint32_t n_tiles = srk_pass_tile_count(width, rows);
    const uint32_t tiles_y = srk_pass_tile_count(1, rows), tiles_x = n_tiles / std::max(tiles_y, 1u);
    *n_tile_rows = tiles_y;
    if (cap < tiles_y) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_row_costs: output too small");
    std::vector<uint32_t> cost(n_tiles);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cost.data(), sched->cost.p, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < tiles_y; r++) {                    // cost slots are absolute tile indices (thread_pixel, kernels.hip)
        double sum = 0.0;
        for (uint32_t x = 0; x < tiles_x; x++) sum += (double)cost[(size_t)r * tiles_x + x];
        out[r] = sum;
    }
    return SR_OK;
}

// The same data per tile, row-major (ty * tiles_x + tx): tuning diagnostics.
int sr_scene_read_tile_costs(SrScene* s, int which, uint32_t width, uint32_t y0, uint32_t rows, uint32_t* out, uint32_t cap, uint32_t* n_tiles_out) {
    if (!s || !out || !n_tiles_out) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_costs: null argument");
    SrScene::TileSchedule* sched = nullptr;
    for (auto& ts : s->schedules) if (ts.which == which && ts.width == width && ts.x0 == 0 && ts.y0 == y0 && ts.y1 == y0 + rows) sched = &ts;
    if (!sched) return fail(SR_ERR_STATE, "sr_scene_read_tile_costs: no launch of this pass with this geometry yet");
    const uint32_t n_tiles = srk_pass_tile_count(width, rows);
    *n_tiles_out = n_tiles;
    if (cap < n_tiles) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_costs: output too small");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, sched->cost.p, (size_t)n_tiles * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

// Test hooks of the tile schedule: the pass path's only input the caller cannot steer is the measured cost the order is derived
// from. The first puts a cost map of the caller's in its place (and derives the order from it, as run_pass does after a launch),
// the second reads the order the next launch of that geometry would run in. Neither needs a frame or a pass launch.
static int check_schedule_rect(const char* name, SrScene* s, int which, uint32_t x0, uint32_t width, uint32_t y0, uint32_t rows) {
    if (!s) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": scene is null");
    if (which != 0 && which != 1) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": which must be 0 (raytracing_ris) or 1 (raytracing_final)");
    if (width == 0 || rows == 0) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": empty launch rectangle");
    // run_pass clips its rectangle to an image of fewer than 2^31 pixels
    if (((uint64_t)x0 + width) * ((uint64_t)y0 + rows) >= (1ull << 31)) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": launch rectangle outside any image the passes accept");
    if (!s->tile_scheduling) return fail(SR_ERR_STATE, std::string(name) + ": tile scheduling is disabled (SR_TILE_SCHEDULING=0)");
    return SR_OK;
}

int sr_scene_set_tile_costs(SrScene* s, int which, uint32_t x0, uint32_t width, uint32_t y0, uint32_t rows, const uint32_t* costs, uint32_t n) {
    int rc = check_schedule_rect("sr_scene_set_tile_costs", s, which, x0, width, y0, rows);
    if (rc != SR_OK) return rc;
    if (!costs) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tile_costs: costs is null");
    if (n != srk_pass_tile_count(width, rows)) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_tile_costs: n is not the number of 8x8 tiles of the rectangle");
    if ((rc = bind_device(s)) != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());                                    // a launch on any stream may still write the costs or read the order
    SrScene::TileSchedule* sched = nullptr;
    if ((rc = schedule_entry(s, which, x0, width, y0, y0 + rows, nullptr, &sched)) != SR_OK) return rc;
    HIP_TRY(hipMemcpy(sched->cost.p, costs, (size_t)n * 4, hipMemcpyHostToDevice));
    int e = srk_launch_tile_order((const uint32_t*)sched->cost.p, (uint32_t*)sched->order.p, width, rows, nullptr);
    if (e != 0) return fail(SR_ERR_HIP, std::string("sr_scene_set_tile_costs tile schedule: ") + hipGetErrorString((hipError_t)e));
    HIP_TRY(hipDeviceSynchronize());                                    // ... and the next launch may be on any stream
    sched->have_order = true;                                           // sched->uses stays: an injected map is no launch
    return SR_OK;
}

int sr_scene_read_tile_order(SrScene* s, int which, uint32_t x0, uint32_t width, uint32_t y0, uint32_t rows, uint32_t* out, uint32_t cap, uint32_t* order_cap) {
    int rc = check_schedule_rect("sr_scene_read_tile_order", s, which, x0, width, y0, rows);
    if (rc != SR_OK) return rc;
    if (!out || !order_cap) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_order: null argument");
    SrScene::TileSchedule* sched = nullptr;
    for (auto& ts : s->schedules) if (ts.which == which && ts.width == width && ts.x0 == x0 && ts.y0 == y0 && ts.y1 == y0 + rows) sched = &ts;
    if (!sched || !sched->have_order) return fail(SR_ERR_STATE, "sr_scene_read_tile_order: no order derived for this pass and geometry yet");
    *order_cap = srk_pass_order_cap(width, rows);
    if (cap < (uint64_t)*order_cap * 8) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_tile_order: output too small");
    if ((rc = bind_device(s)) != SR_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, sched->order.p, (size_t)*order_cap * 8 * 4, hipMemcpyDeviceToHost));
    return SR_OK;
}

int sr_scene_light_stage_capacity(const SrScene* s, uint32_t* lights) {
    if (!s || !lights) return fail(SR_ERR_INVALID_ARG, "sr_scene_light_stage_capacity: null argument");
    if (!s->built) return fail(SR_ERR_STATE, "sr_scene_light_stage_capacity: call sr_scene_set_instances first");
    *lights = s->light_stage ? (uint32_t)srk_lds_rows(s->stack_entries, s->two_level ? 1 : 0) * 64u * 4u / 64u : 0u;   // rows of 64 ints, 64-byte records
    return SR_OK;
}

int sr_trace_ris(const SrRtParams* params, void* stream) { return run_pass(params, 0, stream); }
int sr_trace_final(const SrRtParams* params, void* stream) { return run_pass(params, 1, stream); }

static int check_post(const SrPostParams* p, const char* name, bool need_rt, bool need_gbuffer) {
    if (!p) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": params is null");
    if (p->width == 0 || p->height == 0) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": extent not set");
    if ((uint64_t)p->width * p->height >= (1ull << 31)) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": extent too large");
    if (!p->accum[0] || !p->accum[1] || !p->denoise[0] || !p->denoise[1]) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": ping-pong image pointer is null");
    if (need_rt && (!p->raw_color || !p->motion_vec_img)) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": raw_color / motion_vec_img is null");
    if (need_gbuffer && (!p->depth_img || !p->normal_img || !p->diffuse_img)) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": G-buffer image pointer is null");
    if (p->denoise_passes == 0 || p->denoise_passes > 8) return fail(SR_ERR_INVALID_ARG, std::string(name) + ": denoise_passes must be 1..8");
    return SR_OK;
}

int sr_post_temporal(const SrPostParams* p, void* stream) {
    int rc = check_post(p, "temporal_accumulation", true, false);
    if (rc != SR_OK) return rc;
    PassLabel label("temporal_accumulation");
    int e = srk_launch_post_temporal(*p, (hipStream_t)stream);
    if (e != 0) return fail(SR_ERR_HIP, std::string("temporal_accumulation launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}
int sr_post_denoise(const SrPostParams* p, void* stream) {
    int rc = check_post(p, "denoise", false, true);
    if (rc != SR_OK) return rc;
    PassLabel label("denoise");                                    // the reference's denoise_0 .. denoise_3 (lib.rs:1800-1870), one call here
    int e = srk_launch_post_denoise(*p, (hipStream_t)stream);
    if (e != 0) return fail(SR_ERR_HIP, std::string("denoise launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}
int sr_post_tonemap(const SrPostParams* p, void* stream) {
    int rc = check_post(p, "postprocess", false, false);
    if (rc != SR_OK) return rc;
    if (!p->output_rgba8) return fail(SR_ERR_INVALID_ARG, "postprocess: output image pointer is null");
    PassLabel label("postprocess");
    int e = srk_launch_post_tonemap(*p, (hipStream_t)stream);
    if (e != 0) return fail(SR_ERR_HIP, std::string("postprocess launch: ") + hipGetErrorString((hipError_t)e));
    return SR_OK;
}

int sr_scene_reset_counters(SrScene* s, void* stream) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_reset_counters: scene is null");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_misc.p, 0, kCounterBytes, (hipStream_t)stream));
    return SR_OK;
}

int sr_scene_read_counters(SrScene* s, void* stream, SrRayCounters* out) {
    if (!s || !out) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_counters: null argument");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    std::vector<unsigned long long> copies(kCounterBytes / 8);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    HIP_TRY(hipMemcpy(copies.data(), s->d_misc.p, kCounterBytes, hipMemcpyDeviceToHost));
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t slot = 0; slot < srd::kCounterSlots; slot++)
        for (int k = 0; k < 6; k++) v[k] += copies[(size_t)slot * srd::kCounterStride + k];
    out->closest_queries = v[0]; out->any_queries = v[1]; out->boxes_tested = v[2]; out->tris_tested = v[3]; out->reused_primary_hits = v[4]; out->reused_visibility_queries = v[5];
    return SR_OK;
}

int sr_scene_set_instrumented(SrScene* s, int on) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_set_instrumented: scene is null");
    s->instrumented = on ? 1 : 0;
    return SR_OK;
}

int sr_scene_enable_timing(SrScene* s, int enable) {
    if (!s) return fail(SR_ERR_INVALID_ARG, "sr_scene_enable_timing: scene is null");
    if (enable && !s->timing) for (int k = 0; k < kNumKinds; k++) s->events_used[k] = 0;
    s->timing = enable ? 1 : 0;
    return SR_OK;
}

int sr_scene_read_timing(SrScene* s, int kind, double* total_ms, uint32_t* n_launches) {
    if (!s || kind < 0 || kind >= kNumKinds) return fail(SR_ERR_INVALID_ARG, "sr_scene_read_timing: bad argument");
    int rc = bind_device(s);
    if (rc != SR_OK) return rc;
    double total = 0.0;
    for (size_t i = 0; i < s->events_used[kind]; i++) {
        HIP_TRY(hipEventSynchronize(s->events[kind][i].second));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, s->events[kind][i].first, s->events[kind][i].second));
        total += ms;
    }
    if (total_ms) *total_ms = total;
    if (n_launches) *n_launches = (uint32_t)s->events_used[kind];
    s->events_used[kind] = 0;
    return SR_OK;
}

struct SrHostBvhImpl { srh::BvhResult r; uint32_t n; };

int sr_host_bvh_build(const float* v, uint32_t n, SrHostBvh** out) {
    if (!out || (n && !v)) return fail(SR_ERR_INVALID_ARG, "sr_host_bvh_build: null argument");
    if (n >= (1u << 28)) return fail(SR_ERR_UNSUPPORTED, "sr_host_bvh_build: too many triangles");
    std::vector<srh::BuildTri> t(n);
    for (uint32_t i = 0; i < n; i++) {
        memcpy(t[i].v0, v + (size_t)i * 9, 12); memcpy(t[i].e1, v + (size_t)i * 9 + 3, 12); memcpy(t[i].e2, v + (size_t)i * 9 + 6, 12);
        t[i].prim = i; t[i].inst = 0; t[i].gid = i;
    }
    auto* h = new SrHostBvhImpl();
    h->n = n;
    srh::build_bvh(t, (uint32_t)srd::kMaxBinaryDepth, h->r);
    *out = reinterpret_cast<SrHostBvh*>(h);
    return SR_OK;
}
int sr_host_bvh_get(const SrHostBvh* bvh, const uint32_t** nodes, uint32_t* n_nodes, const float** tris, uint32_t* n_triangles, uint32_t* max_depth, uint32_t* max_stack) {
    if (!bvh) return fail(SR_ERR_INVALID_ARG, "sr_host_bvh_get: null handle");
    const auto* h = reinterpret_cast<const SrHostBvhImpl*>(bvh);
    if (nodes) *nodes = h->r.nodes.data();
    if (n_nodes) *n_nodes = h->r.n_nodes;
    if (tris) *tris = h->r.tris.data();
    if (n_triangles) *n_triangles = h->n;
    if (max_depth) *max_depth = h->r.max_depth;
    if (max_stack) *max_stack = h->r.max_stack;
    return SR_OK;
}
int sr_host_bvh_destroy(SrHostBvh* bvh) { delete reinterpret_cast<SrHostBvhImpl*>(bvh); return SR_OK; }

}  // extern "C"

int srh::scene_take_device_vertices(SrScene* s, uint64_t key, const SrVertex* d_vertices, uint32_t n_vertices, int src_device) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t slot = 0;
    int rc = check_mesh_update(s, key, d_vertices, n_vertices, &slot);
    if (rc != SR_OK || (rc = check_emissive_list(s->meshes[slot])) != SR_OK || (rc = bind_device(s)) != SR_OK) return rc;
    return finish_device_update(s, slot, d_vertices, src_device, 0.0, t0);      // check_ms 0.0: validated once, on the first scene
}

const SrVertex* srh::scene_mesh_frame_vertices(const SrScene* s, uint64_t key, uint32_t* n_vertices) {
    auto it = s->slots.find(key);
    *n_vertices = it == s->slots.end() ? 0u : s->meshes[it->second].n_vertices;
    return (const SrVertex*)s->d_frame_out.p;
}

const SrVertex* srh::scene_pose_batch_vertices(const SrScene* s, uint32_t item, uint32_t* n_vertices) {
    if (item >= s->pose_batch_keys.size()) { *n_vertices = 0; return nullptr; }
    *n_vertices = s->meshes[s->slots.at(s->pose_batch_keys[item])].n_vertices;
    return (const SrVertex*)s->d_pose_scratch.p + s->pose_batch_vertex_base[item];
}

// A further replica of a renderer takes transforms that sr_scene_set_instances_device has accepted on `src_device`: a copy into a
// buffer of its own (peer copy across devices), then the same call on the null stream.
int srh::scene_set_instances_from(SrScene* s, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* d_transforms, int src_device) {
    uint64_t n_inst = 0;
    int rc = check_instance_list(s, keys, counts, n_keys, d_transforms, &n_inst);
    if (rc != SR_OK) return rc;
    if ((rc = bind_device(s)) != SR_OK) return rc;
    const size_t bytes = sizeof(SrTransform) * (size_t)n_inst;
    if ((rc = s->inst.d_replica_transforms.reserve(bytes)) != SR_OK) return rc;
    if (bytes) HIP_TRY(src_device == s->device ? hipMemcpyAsync(s->inst.d_replica_transforms.p, d_transforms, bytes, hipMemcpyDeviceToDevice, nullptr)
                                               : hipMemcpyPeerAsync(s->inst.d_replica_transforms.p, s->device, d_transforms, src_device, bytes, nullptr));
    return set_instances_device(s, keys, counts, n_keys, (const SrTransform*)s->inst.d_replica_transforms.p, nullptr);
}
