/*
 * sunray_hip.h — C ABI of the MI355X-native ray-tracing hot path
 * (ray_gen -> BVH traversal -> ray/triangle intersect -> closest_hit / any_hit / miss shading).
 *
 * This header is the drop-in boundary. Every entry point replaces one interface
 * of the reference (kalsifer-742/sunray, paths relative to its repo root); the reference-side
 * binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no C++/torch types cross this boundary.
 *   - Every function returns an int status: 0 = SR_OK, negative = SrStatus. The text of the last
 *     error on the calling thread is available from sr_last_error() (mirrors SrError{source,
 *     description}, src/error.rs:6-46). Nothing throws or aborts across the ABI.
 *   - "device pointer" = HIP device memory of the GPU the scene was created on (hipMalloc, a torch
 *     tensor's data_ptr(), ...). The caller owns every frame buffer; the library owns only the
 *     scene (mesh tables, BVH) — the ownership split of src/lib.rs:131-153 / 788-793.
 *   - All launches are asynchronous on the caller's hipStream_t (passed as void*); the caller
 *     synchronises, as the reference's caller does with wait_frame (src/lib.rs:1227-1229).
 *   - One context/scene per GPU; single caller thread per scene (the reference's Renderer is
 *     !Send, src/vulkan_abstraction/core/mod.rs:25).
 *
 * Struct layouts T1..T9 are byte-exact mirrors of shaders/rt_types.slang and of the #[repr(C)]
 * Rust structs that feed them; static asserts at the bottom pin the sizes.
 */
#ifndef SUNRAY_HIP_H
#define SUNRAY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* Status codes — mirror ErrorSource (src/error.rs:11-22)                                       */
/* ------------------------------------------------------------------------------------------ */
typedef enum SrStatus {
    SR_OK = 0,
    SR_ERR_INVALID_ARG = -1, /* ErrorSource::Custom: builder/loader misuse (pass_builder.rs:258-294, lib.rs:880-901) */
    SR_ERR_HIP = -2,         /* ErrorSource::Vulkan counterpart: a HIP runtime call failed            */
    SR_ERR_OOM = -3,         /* ErrorSource::GpuAllocator                                            */
    SR_ERR_STATE = -4,       /* ErrorSource::RenderGraph: call order violated (e.g. trace before build) */
    SR_ERR_UNSUPPORTED = -5  /* input outside the built scope (16-bit images, CMYK JPEG, > 2^28 triangles) */
} SrStatus;

#define SR_NULL_TEXTURE 0xFFFFFFFFu /* rt_types.slang:192, resources/material.rs:49 */

/* ------------------------------------------------------------------------------------------ */
/* T1  VertexAttributes (rt_types.slang:24-36) / Vertex (gltf/vertex.rs:1-35) — 96 B            */
/* ------------------------------------------------------------------------------------------ */
typedef struct SrVertex {
    float position[3];
    float _pad0;
    float normal[3];
    float _pad1;
    float tangent[4];
    float base_color_tex_coord[2];
    float metallic_roughness_tex_coord[2];
    float normal_tex_coord[2];
    float occlusion_tex_coord[2];
    float emissive_tex_coord[2];
    float _pad3[2];
} SrVertex;

/* Material (resources/material.rs:15-44) — 112 B, the inlined material_* half of MeshInfo. */
typedef struct SrMaterial {
    float base_color_value[4];
    float metallic_factor;
    float roughness_factor;
    float _pad_mid[2];
    float emissive_factor[4]; /* rgb + strength */
    uint32_t alpha_mode;      /* always 0 in the reference (material.rs:74) */
    float alpha_cutoff;
    float transmission_factor;
    float ior;
    uint32_t base_color_image, base_color_sampler;
    uint32_t metallic_roughness_image, metallic_roughness_sampler;
    uint32_t normal_image, normal_sampler;
    uint32_t occlusion_image, occlusion_sampler;
    uint32_t emissive_image, emissive_sampler;
    uint32_t _pad_end[2];
} SrMaterial;

/* T2  MeshInfo (rt_types.slang:61-86) / EntityGpuData (resources/entity.rs:8-13) — 128 B */
typedef struct SrMeshInfo {
    uint64_t vertices; /* device address of SrVertex[]  */
    uint64_t indices;  /* device address of uint32_t[]  */
    SrMaterial material;
} SrMeshInfo;

/* T3  EmissiveTriangle (rt_types.slang:89-94, gltf/emissive_triangle.rs:6-13) — 64 B */
typedef struct SrEmissiveTriangle {
    float v0[4], v1[4], v2[4]; /* local space, w unused */
    float emission[4];         /* rgb = factor * strength */
} SrEmissiveTriangle;

/* T4  EmissiveIndirectionEntry (rt_types.slang:96-99) — 8 B */
typedef struct SrEmissiveIndirectionEntry {
    uint32_t blas_tri_index; /* slot in the emissive-triangle table */
    uint32_t entity_id;      /* instance index into the transform table */
} SrEmissiveIndirectionEntry;

/* Sampler parameters the path can observe (image/sampler.rs:14-22,77-94; scene.rs:68-83). The
 * enumerators are VkFilter / VkSamplerAddressMode values. Every texture has ONE mip level and the
 * shaders call SampleLevel(.., 0) with min_lod = max_lod = 0 (rt_utils.slang:121-133), so the
 * MAGNIFICATION filter is the one applied; min_filter is carried for completeness only. — 16 B */
#define SR_FILTER_NEAREST 0u
#define SR_FILTER_LINEAR 1u
#define SR_ADDRESS_REPEAT 0u
#define SR_ADDRESS_MIRRORED_REPEAT 1u
#define SR_ADDRESS_CLAMP_TO_EDGE 2u
typedef struct SrSamplerDesc {
    uint32_t min_filter, mag_filter;
    uint32_t address_mode_u, address_mode_v;
} SrSamplerDesc;

/* T5  EntityTransform (rt_types.slang:101-103) = VkTransformMatrixKHR, row-major 3x4 (utils.rs:67-74) — 48 B */
typedef struct SrTransform {
    float m[12];
} SrTransform;

/* T6  Matrices (rt_types.slang:115-120) — 256 B. Each float[16] holds the four ROWS of the
 * matrix (the host uploads the transpose of nalgebra's column-major storage, lib.rs:1023-1047). */
typedef struct SrMatrices {
    float view_inverse[16];
    float proj_inverse[16];
    float view_proj[16];
    float prev_view_proj[16];
} SrMatrices;

/* T7  Reservoir / ReservoirGI (rt_types.slang:123-143, resources/reservoir.rs:6-54) — 48 B each */
typedef struct SrReservoir {
    float light_pos[3];
    float w_sum;
    float light_normal[3];
    float M;
    uint32_t light_idx;
    float W;
    uint32_t hit_normal_packed;
    float depth;
} SrReservoir;

typedef struct SrReservoirGI {
    float sample_pos[3];
    float w_sum;
    float sample_radiance[3];
    float M;
    uint32_t sample_normal_packed;
    float W;
    uint32_t hit_normal_packed;
    float depth;
} SrReservoirGI;

/* T8  RayPayload (rt_types.slang:9-16) — 32 B */
typedef struct SrRayPayload {
    float emission[3];
    float dist;
    uint32_t albedo_packed;
    uint32_t normal_packed;
    uint32_t material_info;
    uint32_t transmission_ior_packed;
} SrRayPayload;

/* RayDesc as passed to TraceRay (ray_gen_ris.slang:70-75) — 32 B */
typedef struct SrRay {
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} SrRay;

/* Committed-hit attributes of one closest-hit query — 16 B.
 * t < 0 (exactly -1.0f) = miss (ray_miss.slang:10-13). tri = global triangle index in
 * instance-major order (instance i's triangles follow instance i-1's); u,v = barycentric weights
 * of vertex 1 and 2 (BuiltInTriangleIntersectionAttributes, closest_hit.slang:15-17). */
typedef struct SrHit {
    float t;
    float u;
    float v;
    uint32_t tri;
} SrHit;

/* Compile-time constants of the reference exposed as knobs (SURVEY.md §5 "Config / flags").
 * sr_trace_config_default() fills the reference values. max_bounces and virtual_bounces above
 * SR_MAX_BOUNCES are refused (SR_ERR_INVALID_ARG): the passes count a pixel's queries in packed fields. */
#define SR_MAX_BOUNCES 8192u
typedef struct SrTraceConfig {
    uint32_t max_bounces;     /* BOUNCES = 10            ray_gen_final.slang:41  */
    uint32_t shadow_bounces;  /* SHADOW_BOUNCES = 5      ray_gen_final.slang:42  */
    uint32_t ris_candidates;  /* RIS_CANDIDATES = 16     ray_gen_ris.slang:187   */
    uint32_t virtual_bounces; /* 20                      ray_gen_ris.slang:69    */
    uint32_t enable_restir;   /* 1 = reference behaviour. 0 = ReSTIR block disabled: the final pass
                                 starts with restir_evaluated = true, so every rough bounce takes the
                                 plain NEE branch (ray_gen_final.slang:328-382); the RIS pass is not
                                 needed (BASELINE.json configs 2, 3, 5).                           */
    uint32_t flags;           /* SR_TRACE_FLAG_* */
    uint32_t count_y0;        /* with count_rows != 0: only pixels of rows [count_y0, count_y0 + count_rows) add  */
    uint32_t count_rows;      /* their rays to the scene's counters — a strip traced together with its halo rows  */
    uint32_t count_x0;        /* same for columns: with count_cols != 0 only pixels of columns                    */
    uint32_t count_cols;      /* [count_x0, count_x0 + count_cols) count (column strips)              */
} SrTraceConfig;

/* Do not add this launch's rays to the scene's ray counters: used for the halo rows a GPU re-traces
 * for its neighbours' spatial reuse in tile-parallel rendering, so that counted rays are
 * exactly the rays of the equivalent single-GPU frame. */
#define SR_TRACE_FLAG_UNCOUNTED 1u
/* Trace every query the reference issues, also where its answer is known from an identical query of the same pixel in the same
 * pass (SrRayCounters.reused_visibility_queries stays 0). Same results either way; for accounting and A/B. */
#define SR_TRACE_FLAG_TRACE_EVERY_QUERY 2u

typedef struct SrScene SrScene; /* opaque: mesh tables + instance tables + BVH ("TLAS") on one GPU */

/* T9  RaytracingPC (rt_types.slang:151-190) / RaytracingHeapPushConstant
 * (pipelines/ray_tracing_pipeline.rs:28-60), with every heap handle replaced by a pointer and the
 * dispatch extent (pass_builder.rs:311-320 trace_extent) made explicit. The same params struct is
 * handed to both passes, as the reference pushes identical bytes to both (lib.rs:1626-1652).
 *
 * Image storage follows the reference's formats (lib.rs:1492-1516), one element per pixel, row 0 =
 * top of the image:
 *   raw_color      float[4]  fp32 RGBA (reference: B10G11R11_UFLOAT; kept fp32 here)
 *   depth_img      uint16    R16_SFLOAT bits
 *   normal_img     uint32    R8G8B8A8_SNORM, normal.xyz + roughness in .a
 *   diffuse_img    uint32    B10G11R11_UFLOAT_PACK32
 *   motion_vec_img uint32    R16G16_SFLOAT
 * meshes_info / emissive_triangles / emissive_indirection / entity_transforms / tlas of the
 * reference struct are owned by `scene` (sr_scene_* below). */
typedef struct SrRtParams {
    const SrScene* scene;
    float* raw_color;                /* device, 4*W*H floats  */
    uint16_t* depth_img;             /* device, W*H           */
    uint32_t* normal_img;            /* device, W*H           */
    uint32_t* diffuse_img;           /* device, W*H           */
    uint32_t* motion_vec_img;        /* device, W*H           */
    const SrMatrices* matrices;      /* HOST pointer, copied into the launch like push data */
    const uint8_t* blue_noise_tex;   /* device, RGBA8 texels, blue_noise_w*blue_noise_h*4 bytes (lib.rs:281-309) */
    uint32_t blue_noise_w, blue_noise_h;
    SrReservoir* reservoirs[2];      /* device, W*H each; ping-pong by frame_count & 1 (rt_utils.slang:241-242) */
    SrReservoirGI* reservoirs_gi[2]; /* device, W*H each */
    /* Primary-hit hand-off (optional, device, W*H records, caller-owned like the G-buffer images). Both reference passes
     * start with the SAME query: ray_gen_final.slang:80 at bounce 0 is ray_gen_ris.slang:75 at virtual bounce 0 (same
     * pixel, same matrices, same TLAS), and TraceRay is a pure function of its arguments. With a buffer here sr_trace_ris
     * stores that query's 32-byte RayPayload (T8, closest_hit / miss applied) per pixel and sr_trace_final, enqueued
     * after it for the same frame, reads it back instead of traversing and shading again — same bits, one traversal
     * fewer per pixel (counted in SrRayCounters.reused_primary_hits, not in closest_queries). NULL: sr_trace_final traces
     * the query itself. Ignored when config.enable_restir == 0 (no RIS pass ran) or config.virtual_bounces == 0. Part of
     * the per-frame image set: double-buffer it with the G-buffer when two frames are in flight. */
    SrRayPayload* primary_payload;
    uint32_t frame_count;            /* relative_frame_count (lib.rs:1355,1386) */
    uint32_t use_srgb;               /* carried, unused by the shaders */
    uint32_t width, height;          /* trace_extent[0], [1]; also the image size */
    /* Sub-rectangle of the image this launch covers, for tile-parallel multi-GPU.
     * Pixels are keyed by their GLOBAL coordinates (RNG, camera), so any tiling gives identical
     * values. tile_h == 0 means all rows, tile_w == 0 all columns. Buffers are always full-size W*H. */
    uint32_t tile_y0, tile_h;
    uint32_t tile_x0, tile_w;
    SrTraceConfig config;
} SrRtParams;

/* Ray counters accumulated by the kernels (rays are counted, not estimated). */
typedef struct SrRayCounters {
    uint64_t closest_queries; /* TraceRay(RAY_FLAG_NONE) traversed         */
    uint64_t any_queries;     /* TraceRay(ACCEPT_FIRST_HIT|SKIP_CLOSEST) traversed */
    uint64_t boxes_tested;    /* child boxes tested (32 B each), only in the instrumented build */
    uint64_t tris_tested;     /* triangle records tested (48 B each), only in the instrumented build */
    uint64_t reused_primary_hits; /* TraceRay(RAY_FLAG_NONE) calls of the reference's final pass answered from
                                     SrRtParams.primary_payload without a traversal: the reference issues
                                     closest_queries + reused_primary_hits closest-hit queries */
    uint64_t reused_visibility_queries; /* TraceRay(ACCEPT_FIRST_HIT) calls of the reference's final pass answered without a traversal:
                                     ray_gen_final.slang:304-316 when the combined GI reservoir's sample is a spatial neighbour's, whose
                                     identical ray (:276-286) was found unoccluded a moment before. The reference issues
                                     any_queries + reused_visibility_queries existence queries */
} SrRayCounters;

/* ------------------------------------------------------------------------------------------ */
/* Errors                                                                                       */
/* ------------------------------------------------------------------------------------------ */
const char* sr_last_error(void); /* SrError::description of the last failure on this thread */
int sr_version(void);

/* ------------------------------------------------------------------------------------------ */
/* Host-side data preparation — pure CPU, no GPU needed                     */
/* ------------------------------------------------------------------------------------------ */

/* H1/H2: Camera::as_matrices (src/camera.rs:33-63) followed by the transposed upload of
 * Renderer::render (src/lib.rs:1017-1048). prev_view_proj16 = the previous frame's view_proj rows
 * as returned in out->view_proj by the previous call, or NULL on the first frame (zero matrix,
 * lib.rs:410). */
int sr_camera_matrices(const float position[3], const float target[3], float fov_y_degrees,
                       uint32_t width, uint32_t height, const float* prev_view_proj16,
                       SrMatrices* out);

/* H6: Material::new for a runtime mesh (resources/material.rs:52-92 with the NULL-texture
 * resolver of lib.rs:937-943): factors copied, alpha_mode = 0, alpha_cutoff = 0, all textures NULL. */
int sr_material_new(const float base_color[4], float metallic, float roughness,
                    const float emissive_factor[3], float emissive_strength, float transmission,
                    float ior, SrMaterial* out);

/* H5: emissive-triangle derivation of Renderer::load_mesh (src/lib.rs:901-925).
 * Writes at most cap entries, returns the total count through *out_count. */
int sr_emissive_triangles_from_mesh(const SrVertex* vertices, uint32_t n_vertices,
                                    const uint32_t* indices, uint32_t n_indices,
                                    const SrMaterial* material, SrEmissiveTriangle* out,
                                    uint32_t cap, uint32_t* out_count);

void sr_trace_config_default(SrTraceConfig* out);

/* ------------------------------------------------------------------------------------------ */
/* Scene = ResourceManager + BLAS/TLAS (resource_manager.rs, acceleration_structure/)           */
/* ------------------------------------------------------------------------------------------ */

/* Renderer::new's resource half (lib.rs:212-446, resource_manager.rs:84-155) on HIP device `device`. */
int sr_scene_create(int device, SrScene** out);
int sr_scene_destroy(SrScene* scene);

/* Renderer::load_mesh (src/lib.rs:873-954) + ResourceManager::add_blas (resource_manager.rs:417-447):
 * validates like the reference (non-empty, index count % 3 == 0, indices in range, key unused),
 * uploads vertices/indices, assigns the next mesh-info slot (the instance custom index,
 * closest_hit.slang:18-19) and appends the mesh's emissive triangles to the emissive table.
 * vertices/indices are HOST pointers. *out_slot may be NULL. */
int sr_scene_add_mesh(SrScene* scene, uint64_t key, const SrVertex* vertices, uint32_t n_vertices,
                      const uint32_t* indices, uint32_t n_indices, const SrMaterial* material,
                      uint32_t* out_slot);

/* ------------------------------------------------------------------------------------------ */
/* Acceleration-structure maintenance                                            */
/* ------------------------------------------------------------------------------------------ */
/* BuildType / OpType / AsState (acceleration_structure/mod.rs:22-148): the rebuild-vs-update heuristic shared by
 * the reference's BLAS and TLAS — update in place at most 8 times, then a fast rebuild; after 16 quiet frames one
 * quality rebuild and back to Optimal. Pure logic, exposed for the host that drives the scene. */
#define SR_BUILD_RAPIDLY_CHANGING 0u
#define SR_BUILD_SOMETIMES_CHANGES 1u
#define SR_BUILD_STATIC 2u
#define SR_OP_NONE 0u
#define SR_OP_SLOW_BUILD 1u
#define SR_OP_FAST_BUILD 2u
#define SR_OP_UPDATE 3u
typedef struct SrAsState {
    uint32_t changing; /* 0 = AsState::Optimal, 1 = AsState::Changing(Dynamic) */
    uint32_t frames_without_changes;
    uint32_t number_of_updates_since_last_rebuild;
    uint32_t _pad;
} SrAsState;
void sr_as_state_initial(uint32_t build_type, SrAsState* out);
uint32_t sr_as_state_next_op(const SrAsState* state, int inputs_changed);
void sr_as_state_mark_built(SrAsState* state, uint32_t completed_op);
/* The scene's own state (it is built as SometimesChanges, like the reference's TLAS, resource_manager.rs:119-126)
 * and the operation sr_scene_set_instances / sr_scene_end_frame last performed (SR_OP_*). */
int sr_scene_as_state(const SrScene* scene, SrAsState* state, uint32_t* last_op);
/* A frame whose instance list did not change (Tlas::mark_built(None) + the settle rebuild, tlas.rs:155-191 with
 * inputs_changed = false): advances the quiet-frame counter and, when AsState asks for it, performs the quality
 * rebuild. The Renderer facade calls it for every frame that skips sr_scene_set_instances. */
int sr_scene_end_frame(SrScene* scene);
/* Test / bench hook: the next sr_scene_set_instances performs `op` (SR_OP_SLOW_BUILD = host binned-SAH build,
 * SR_OP_FAST_BUILD = device LBVH build, SR_OP_UPDATE = in-place update if the layout allows) instead of the
 * heuristic's choice. The heuristic state is still advanced with the op performed. */
int sr_scene_force_next_op(SrScene* scene, uint32_t op);
/* Form of the acceleration structure. The reference instances BLASes through a TLAS (tlas.rs:155-191, resource_manager.rs:236-251).
 * SR_INSTANCING_FLAT copies every instance's triangles into ONE world-space tree (no ray transform in the walk, work stealing inside the
 * wave; memory and update cost grow with instances x triangles); SR_INSTANCING_TWO_LEVEL keeps one tree per mesh in object space plus a
 * top-level tree over the instances (a changed instance list costs a top-level rebuild whatever the meshes hold; the walk transforms
 * the ray per instance). Both answer every query with the same bits: in the two-level walk the object-space ray only steers box
 * culling, triangles are tested in world space. SR_INSTANCING_AUTO (default): two-level where the flattened copy would exceed 2^24
 * triangles and at least four times the meshes' own, or 2^28 in any case. Takes effect at the next sr_scene_set_instances.
 * SR_INSTANCING = flat | two_level | auto in the environment sets the initial mode. */
#define SR_INSTANCING_AUTO 0u
#define SR_INSTANCING_FLAT 1u
#define SR_INSTANCING_TWO_LEVEL 2u
int sr_scene_set_instancing(SrScene* scene, uint32_t mode);
int sr_scene_instancing(const SrScene* scene, uint32_t* mode, uint32_t* two_level_now);
/* Where the top-level tree of the two-level form is built when the instance list of a scene ALREADY built in that form changes
 * (the reference rebuilds its TLAS on the GPU every frame, tlas.rs:155-191). SR_TL_BUILD_DEVICE: the instance records, their padded
 * world boxes (byte for byte the host's) and the tree (Morton sort + SR_FAST_BUILD topology + budgeted 4-wide collapse over the
 * boxes) come from device kernels; SR_TL_BUILD_HOST: the host binned-SAH builder, always; SR_TL_BUILD_AUTO (default): the device
 * from SrTopLevelInfo.auto_threshold instance boxes on. The first build, the settle rebuild of sr_scene_end_frame, lists with
 * fewer than two instance boxes, lists with an instance whose transform cannot be inverted well (it gets a baked copy of its
 * mesh) and trees outside the traversal-stack budget are built on the host in every mode. Queries give the same bits either way.
 * SR_TL_BUILD = host | device | auto in the environment sets the initial mode (anything else: auto). */
#define SR_TL_BUILD_AUTO 0u
#define SR_TL_BUILD_HOST 1u
#define SR_TL_BUILD_DEVICE 2u
int sr_scene_set_top_level_build(SrScene* scene, uint32_t mode);
/* Why the last top-level build ran on the host (SrTopLevelInfo.reason; SR_TL_ON_DEVICE: it did not). */
#define SR_TL_ON_DEVICE 0u
#define SR_TL_HOST_MODE 1u             /* SR_TL_BUILD_HOST */
#define SR_TL_HOST_BELOW_THRESHOLD 2u  /* auto mode, fewer instance boxes than auto_threshold */
#define SR_TL_HOST_BAKED_INSTANCE 3u   /* an instance of the list needs a baked copy of its mesh */
#define SR_TL_HOST_STACK_BUDGET 4u     /* the device tree would need more traversal-stack entries than the mesh trees leave (SR_HEIGHT_BOUND_REBALANCE below bounds it instead) */
#define SR_TL_HOST_NOT_TWO_LEVEL 5u    /* nothing stood in the two-level form: first build, form switch, meshes added or removed since */
#define SR_TL_HOST_TOO_FEW 6u          /* fewer than two instance boxes */
#define SR_TL_HOST_QUALITY_BUILD 7u    /* the settle rebuild of sr_scene_end_frame */
typedef struct SrTopLevelInfo {
    uint32_t on_device;       /* 1: the last top-level build ran on the device */
    uint32_t reason;          /* SR_TL_ON_DEVICE or SR_TL_HOST_* */
    uint32_t mode;            /* SR_TL_BUILD_* in force */
    uint32_t auto_threshold;  /* instance boxes from which auto mode builds on the device */
    uint32_t n_nodes;         /* nodes of the top-level tree */
    uint32_t n_boxes;         /* instances with a box = entries of the leaf order */
    uint32_t n_instances;
    uint32_t max_stack;       /* worst-case stack entries of the top-level tree alone */
    uint32_t blas_stack;      /* ... of the deepest mesh tree in use: max_stack + leaf size + blas_stack + 1 = SrBvhStats.max_stack */
    uint32_t _pad;
    double records_ms;        /* instance records + boxes (device: including the upload of the instance tables) */
    double tree_ms;           /* top-level tree */
    double build_ms;          /* the whole build as sr_scene_set_instances saw it */
} SrTopLevelInfo;             /* 64 bytes */
int sr_scene_top_level_info(const SrScene* scene, SrTopLevelInfo* out);
/* Harness read-back of the top level of a scene built in the two-level form, whichever path built it (the counterpart of
 * sr_scene_read_bvh): n_nodes x 16 dwords, n_boxes dwords (leaf order -> instance index), n_instances x 128 bytes (the
 * instance records the walk reads), n_instances x 6 floats (padded world box lo, hi; a row of NaN: the instance has no box).
 * Counts as in SrTopLevelInfo; any pointer may be NULL. */
int sr_scene_read_top_level(const SrScene* scene, uint32_t* nodes, uint32_t* tl_inst, void* records, float* boxes);
/* Node layout of the quantised wide BVH this build uses (csrc/bvh_layout.h): children per node, dwords per node, first
 * plane dword, first child dword. */
int sr_bvh_layout(uint32_t* width, uint32_t* node_dwords, uint32_t* plane_offset, uint32_t* child_offset);
/* What the device tree builders shape a tree of `n_prims` primitives of one SR_TREE_KIND_* by: primitives per leaf
 * (csrc/bvh_layout.h) and the stack floor of the collapse before the build's cap bounds it (mesh: the host builder's depth for
 * that size; top level: the median tree's depth; one level: the regular stack size). Either pointer may be NULL. */
int sr_tree_build_limits(uint32_t kind, uint64_t n_prims, uint32_t* leaf_max, uint32_t* stack_floor);
/* Debug read-back of the device tree: n_nodes x node_dwords dwords, n_triangles x 12 floats (either may be NULL). */
int sr_scene_read_bvh(const SrScene* scene, uint32_t* nodes_out, float* tris_out);

/* ResourceManager::add_blas (resource_manager.rs:417-447): sr_scene_add_mesh with the local-space emissive
 * triangles supplied by the caller instead of derived from the material — the glTF path marks a primitive
 * emissive under a different rule than load_mesh (gltf/mod.rs:272 vs lib.rs:907). */
int sr_scene_add_blas(SrScene* scene, uint64_t key, const SrVertex* vertices, uint32_t n_vertices,
                      const uint32_t* indices, uint32_t n_indices, const SrMaterial* material,
                      const SrEmissiveTriangle* emissive, uint32_t n_emissive, uint32_t* out_slot);
/* ResourceManager::remove (resource_manager.rs:459-487): frees the mesh-info slot and the emissive slots of
 * `key` (later loads reuse them LIFO, as the reference's arenas do). Unknown key: no-op. Waits for the device. */
int sr_scene_remove(SrScene* scene, uint64_t key);
/* Blas::update (acceleration_structure/blas.rs:285-310): new vertex contents (positions, normals, tangents, every uv set) for a
 * loaded mesh — same key, same vertex count, same indices, same material. Validated before anything is touched (unknown key,
 * another vertex count, a non-finite position: SR_ERR_INVALID_ARG and the scene is as it was). Replaces the host copy, copies
 * into the mesh's existing device allocation (waits for the device) and rewrites the positions of its entries of the emissive
 * table in their slots. The structure is not reset: several meshes may be updated, then ONE sr_scene_set_instances applies them
 * all with the operation the heuristic picks (SR_OP_UPDATE re-flattens, rewrites the per-slot shading records and refits on
 * the device; the builds read the new vertices anyway; in the two-level form the trees of the updated meshes are refitted on the
 * device where sr_scene_set_mesh_build_type allows it and rebuilt on the host otherwise). Between the update of a mesh that the built structure instances and that sr_scene_set_instances, the tracing calls,
 * sr_scene_read_bvh and sr_scene_end_frame return SR_ERR_STATE. `vertices` is a HOST pointer. */
int sr_scene_update_mesh(SrScene* scene, uint64_t key, const SrVertex* vertices, uint32_t n_vertices);
/* Figures of the last sr_scene_update_mesh and of the sr_scene_set_instances that applied it. The kernel times are taken with
 * events only while sr_scene_enable_timing is on (0 otherwise); the other times are host wall-clock milliseconds. */
typedef struct SrMeshUpdateInfo {
    uint32_t dirty_meshes;     /* meshes of the built structure that were updated and that the last sr_scene_set_instances applied */
    uint32_t reshaded;         /* 1: its SR_OP_UPDATE ran the variant that rewrites the shading records */
    uint32_t blas_rebuilt;     /* two-level form: per-mesh trees it built, on the host (the invalidated ones: every mesh updated since its
                                * tree was built, instanced at the time or not; baked copies of single instances not counted) or on the
                                * device (SrMeshTreeInfo) */
    uint32_t blas_refitted;    /* two-level form: per-mesh trees it refitted on the device (sr_scene_set_mesh_build_type) */
    double validate_copy_ms;   /* sr_scene_update_mesh: validation + host copy + emissive entries */
    double h2d_ms;             /* sr_scene_update_mesh: device wait + copy into the device allocation */
    double tables_ms;          /* SR_OP_UPDATE: instance tables + light table, built and uploaded */
    double flatten_ms;         /* SR_OP_UPDATE: flatten (+ reshade) kernel; mesh-tree refit: the record-rewrite kernel */
    double refit_ms;           /* SR_OP_UPDATE: refit kernels, all levels; mesh-tree refit: its refit launches */
    double blas_build_ms;      /* two-level form: host builds of the per-mesh trees counted in blas_rebuilt */
} SrMeshUpdateInfo;
int sr_scene_mesh_update_info(const SrScene* scene, SrMeshUpdateInfo* out);
/* sr_scene_update_mesh for vertices that already are in device memory of the scene's GPU (a skinning or simulation kernel, a
 * torch tensor): `d_vertices` holds n_vertices SrVertex records, is 16-byte aligned, and was produced by work on `stream`. The
 * contract is sr_scene_update_mesh's, with these differences. Refused on the host before anything is launched: a null scene or
 * pointer, an unknown key, another vertex count, a misaligned pointer, a range that overlaps the mesh's own device allocation
 * (SrMeshInfo.vertices of sr_scene_get_tables), a pointer the HIP runtime does not report as device memory of the scene's
 * device for that many vertices (all SR_ERR_INVALID_ARG; such a pointer is never dereferenced), an emissive list that is not
 * one per triangle (SR_ERR_UNSUPPORTED). The positions are then validated ON THE DEVICE under the host call's rule (x, y, z
 * finite; nothing else is looked at): the lowest offending index is reported with the host call's text and status, and the
 * scene is exactly as it was, since the mesh's buffer is written only afterwards (check, 4-byte read-back, device wait,
 * device-to-device copy). The library's HOST copy of the vertices is not touched and becomes stale; host code that needs it (a
 * host build of the mesh's tree or of the one-level tree) fetches it with one device-to-host copy, the device paths (SR_OP_UPDATE,
 * the device fast build, the device refit and device build of an updatable mesh's tree) never do. A mesh with emissive entries
 * fetches inside the call while the scene builds its light table on the host (SR_LIGHTS_HOST, the default), and never under
 * SR_LIGHTS_DEVICE (sr_scene_set_light_table_build). A later sr_scene_update_mesh replaces the copy. SrMeshUpdateInfo.validate_copy_ms / h2d_ms: host
 * wall clock of the call without, and of, its wait-and-copy section. */
int sr_scene_update_mesh_device(SrScene* scene, uint64_t key, const SrVertex* d_vertices, uint32_t n_vertices, void* stream);
typedef struct SrMeshVertexInfo {
    uint32_t host_stale;       /* 1: the host copy is older than the device buffer */
    uint32_t last_from_device; /* 1: the last update of this mesh came through the device entry point */
    uint32_t host_fetches;     /* device-to-host refreshes of the host copy since the mesh was loaded */
    uint32_t _pad;
    double check_ms;           /* last device update: validation kernel + read-back (events, only while sr_scene_enable_timing is on) */
    double copy_ms;            /* last device update: the device-to-device copy (events, only while sr_scene_enable_timing is on) */
    double fetch_ms;           /* the last host fetch (wall clock) */
} SrMeshVertexInfo;            /* 40 bytes */
int sr_scene_mesh_vertex_info(const SrScene* scene, uint64_t key, SrMeshVertexInfo* out);
/* Where sr_scene_set_instances builds the frame's light table (one 64-byte record per emissive triangle x instance: the world
 * vertices, area, normal and emission the passes sample). SR_LIGHTS_HOST (default; SR_LIGHT_TABLE=host|device in the environment
 * sets the initial mode): host arithmetic over the emissive arena, uploaded whole. SR_LIGHTS_DEVICE: the arena has a device
 * mirror, the indirection entries are uploaded only when they changed, and a kernel writes the table with the host's arithmetic
 * operation for operation (the records are equal bit for bit wherever the host's words are not NaN; a zero-area triangle has NaN
 * normals on both, with the payload of each machine). Under it sr_scene_update_mesh_device and sr_scene_skin_mesh never fetch
 * the vertices of a mesh with emissive entries: a kernel rewrites the positions of its arena slots from the mesh's device
 * vertices at the next sr_scene_set_instances. sr_scene_get_tables and a switch back to SR_LIGHTS_HOST read the device arena
 * back where the host's is older (64 bytes per arena entry, counted in SrLightTableInfo.arena_fetches, not in
 * SrMeshVertexInfo.host_fetches). A scene whose arena is empty, or that has no instance, builds its one dummy record on the
 * host in either mode. Unknown mode: SR_ERR_INVALID_ARG. */
#define SR_LIGHTS_HOST 0u
#define SR_LIGHTS_DEVICE 1u
int sr_scene_set_light_table_build(SrScene* scene, uint32_t mode);
/* The light table of the last sr_scene_set_instances. The kernel times are taken with events, the host time with the wall
 * clock, all three only while sr_scene_enable_timing is on (0 otherwise). */
typedef struct SrLightTableInfo {
    uint32_t mode;               /* SR_LIGHTS_* in force */
    uint32_t on_device;          /* 1: the table was built by the kernel */
    uint32_t num_lights;         /* records of the table (the dummy record included) */
    uint32_t arena_entries;      /* entries of the emissive arena */
    uint32_t positions_rewritten;/* arena triangles whose positions the device rewrote from device vertices */
    uint32_t entries_uploaded;   /* 1: the indirection entries differed from the device's copy and were uploaded */
    uint32_t arena_uploads;      /* 1: host-side changes of the arena (add, remove, sr_scene_update_mesh) were uploaded */
    uint32_t arena_fetches;      /* device-to-host reads of the device arena since the scene was created (running count) */
    double positions_ms;         /* the arena-position kernels */
    double table_ms;             /* the table kernel */
    double host_ms;              /* the host path: arithmetic + upload */
} SrLightTableInfo;              /* 56 bytes */
int sr_scene_light_table_info(const SrScene* scene, SrLightTableInfo* out);
/* Debug read-back of the device light table (next to sr_scene_read_bvh), whichever mode built it: *n_lights records, of which
 * the first min(cap_lights, *n_lights) are copied to `out` (may be NULL with cap_lights == 0), 16 floats each in the order the
 * passes read them:
 *   [0..2] world v0   [3]  area = 0.5 * |(v1 - v0) x (v2 - v0)|
 *   [4..6] world v1   [7]  unit normal x
 *   [8..10] world v2  [11] unit normal y
 *   [12..14] emission rgb (factor * strength)   [15] unit normal z */
int sr_scene_read_lights(const SrScene* scene, float* out, uint32_t cap_lights, uint32_t* n_lights);
/* The host arithmetic of the light table on its own (no scene, no device): out[16 * i ..] from entries[i] = (slot into
 * `triangles`, index into `transforms`). An entry out of range: SR_ERR_INVALID_ARG, nothing written. */
int sr_light_table(const SrTransform* transforms, uint32_t n_transforms, const SrEmissiveIndirectionEntry* entries, uint32_t n_entries,
                   const SrEmissiveTriangle* triangles, uint32_t n_triangles, float* out);
/* Skinning (glTF 2.0 linear blend): the producer of sr_scene_update_mesh_device's vertices that lives in the library. One
 * influence record per vertex: up to four joints and their weights, used as given (no renormalisation). */
typedef struct SrSkinInfluence {
    uint16_t joint[4];
    float weight[4];
} SrSkinInfluence;             /* 24 bytes */
/* Attaches a rig to a loaded mesh: snapshots the mesh's CURRENT device vertices as the bind pose (a device-to-device copy the
 * mesh owns; waits for the device) and uploads `influences` (HOST pointer, n_vertices records). Refused with
 * SR_ERR_INVALID_ARG before anything is touched: a null scene, an unknown key, another vertex count than the mesh's,
 * n_joints == 0, and, with a message that names the lowest offending vertex, a joint index >= n_joints on an influence whose
 * weight is not 0, a weight that is negative or not finite, a vertex whose four weights are all 0. influences == NULL detaches
 * the skin and frees its buffers (n_vertices and n_joints are not looked at); sr_scene_remove frees them too. Later
 * sr_scene_update_mesh* calls do not move the bind pose; attaching again snapshots it anew. */
int sr_scene_set_mesh_skin(SrScene* scene, uint64_t key, const SrSkinInfluence* influences, uint32_t n_vertices, uint32_t n_joints);
/* Poses a skinned mesh. The call is a batch of one item on the path of sr_scene_pose_meshes (below): `joint_matrices` (HOST
 * pointer, n_joints rows of 3x4, object space of the mesh) go up asynchronously on `stream` in the staging block, the posing
 * kernel skins the bind pose with the influences into a scratch buffer the scene owns, and a scatter launch copies the records
 * into the mesh's allocation, which leaves what sr_scene_update_mesh_device leaves: the posed vertices are applied by the next
 * sr_scene_set_instances, with the same SR_ERR_STATE window, the same stale host copy and the same emissive handling. The
 * finite-position check (x, y, z of the posed position; nothing else is looked at) is part of the kernel: on a bad vertex the
 * call returns sr_scene_update_mesh's status and text with the lowest offending index, and the scene is exactly as it was
 * (only SrMeshSkinInfo.first_bad tells). Refused on the host before anything is launched: a null scene or matrices, an unknown
 * key, a mesh with no skin, another n_joints than the skin's (SR_ERR_INVALID_ARG), an emissive list that is not one per
 * triangle (SR_ERR_UNSUPPORTED).
 * The arithmetic, fp32 under the numerics contract (no contraction, correctly rounded divide and sqrt, left to right), per
 * vertex with bind position (x, y, z), bind normal n, bind tangent (t, w), joints j_k and weights w_k, k = 0..3:
 *   B[r][c]   = 0.0f, then for k = 0, 1, 2, 3 in order, where w_k != 0:  B[r][c] = B[r][c] + w_k * M[j_k][r][c]      (r < 3, c < 4;
 *               an influence with w_k == 0 is skipped: its matrix is never read, so a NaN in it or an index past the rig is free)
 *   position' = ((B[r][0] * x + B[r][1] * y) + B[r][2] * z) + B[r][3]
 *   C         = the cofactor matrix of B's 3x3 part, its rows the cross products a1 x a2, a2 x a0, a0 x a1 of B's rows a_r, with
 *               a x b = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x)
 *   normal'   = normalise((C[r][0] * n.x + C[r][1] * n.y) + C[r][2] * n.z)       (correct under non-uniform scale; a reflection
 *               turns the normal with the winding)
 *   tangent'  = (normalise((B[r][0] * t.x + B[r][1] * t.y) + B[r][2] * t.z), w)
 *   normalise(v) = v * (1.0f / sqrt((v.x * v.x + v.y * v.y) + v.z * v.z)); where that squared length is 0 or not finite, the
 *               bind pose's bytes are written for that vector.
 * Every other byte of the record (the five uv sets, the pads) is the bind pose's. */
int sr_scene_skin_mesh(SrScene* scene, uint64_t key, const SrTransform* joint_matrices, uint32_t n_joints, void* stream);
typedef struct SrMeshSkinInfo {
    uint32_t n_joints;         /* joints of the attached skin; 0: the mesh has none */
    uint32_t skinned;          /* poses taken since the skin was attached */
    uint32_t first_bad;        /* the last sr_scene_skin_mesh: lowest vertex posed to a non-finite position, 0xFFFFFFFF: none */
    uint32_t _pad;
    double skin_ms;            /* the last accepted pose: the posing kernel + read-back; 0.0 where a morph stage ran: morph_ms has it (events, only while sr_scene_enable_timing is on) */
} SrMeshSkinInfo;              /* 24 bytes */
int sr_scene_mesh_skin_info(const SrScene* scene, uint64_t key, SrMeshSkinInfo* out);
/* Morph targets (glTF 2.0 blend shapes): the other producer of posed vertices that lives in the library. One delta record per
 * (target, vertex): three 16-byte pieces laid out like the first three of SrVertex; the pads are never read. */
typedef struct SrMorphDelta {
    float position[3], _pad0;
    float normal[3], _pad1;
    float tangent[3], _pad2;
} SrMorphDelta;                /* 48 bytes */
/* Attaches morph targets to a loaded mesh: snapshots the mesh's CURRENT device vertices as the morph base (a device-to-device
 * copy the mesh owns; waits for the device) and uploads `deltas` (HOST pointer, n_targets * n_vertices records, target-major:
 * target k's records for vertices 0..n_vertices-1 are contiguous). Refused with SR_ERR_INVALID_ARG before anything is touched: a
 * null scene, an unknown key, another vertex count than the mesh's, n_targets == 0, and, with a message that names the lowest
 * (target, vertex), a delta component (position, normal or tangent; not the pads) that is not finite. A failed allocation
 * returns SR_ERR_OOM and leaves an earlier morph in place. deltas == NULL detaches the morph and frees its buffers (n_vertices
 * and n_targets are not looked at); sr_scene_remove and sr_scene_destroy free them too. Later sr_scene_update_mesh* calls do not
 * move the base; attaching again snapshots it anew. A mesh may carry a morph and a skin: attach both while the mesh holds its
 * rest vertices, in either order. */
int sr_scene_set_mesh_morph(SrScene* scene, uint64_t key, const SrMorphDelta* deltas, uint32_t n_vertices, uint32_t n_targets);
/* The one per-frame call of a mesh that has a morph, a skin or both, in glTF's order: morph first, then skin.
 * weights == NULL skips the morph stage: the call is then exactly sr_scene_skin_mesh(scene, key, joint_matrices, n_joints, stream).
 * joint_matrices == NULL skips the skin stage. Both NULL: SR_ERR_INVALID_ARG.
 * Like sr_scene_skin_mesh the call is a batch of one item on the path of sr_scene_pose_meshes (below). The morph stage compacts
 * the weights that are not 0 into an active list (ascending target order; a target of weight 0 costs no traffic) and starts
 * from the morph base. With a skin stage the one posing kernel keeps the morphed position, normal and tangent on chip and skins
 * them in place of the bind pose (the snapshot of sr_scene_set_mesh_skin is not read then); the bytes are those of
 * morph-then-skin through memory. The result goes the way of sr_scene_skin_mesh's: applied by the next sr_scene_set_instances,
 * with the same SR_ERR_STATE window, the same stale host copy and the same emissive handling. Each stage has a finite-position
 * check word of its own (x, y, z of the stage's position; nothing else is looked at); both are read back once, after the
 * kernel: on a bad vertex the call returns sr_scene_update_mesh's status and text with the lowest offending index of either
 * stage, and the scene is exactly as it was (only SrMeshMorphInfo / SrMeshSkinInfo tell: first_bad of every stage that ran,
 * 0xFFFFFFFF where that stage found none, and n_active). Refused on the host before anything is launched: a null scene, an unknown key, a stage asked
 * for that the mesh has nothing attached for, another n_targets or n_joints than attached, a weight that is not finite (the
 * message names the lowest index) (SR_ERR_INVALID_ARG), an emissive list that is not one per triangle (SR_ERR_UNSUPPORTED).
 * The morph arithmetic, fp32 under the numerics contract (no contraction, correctly rounded divide and sqrt, left to right), for
 * each of the three vectors (position, normal, tangent) of a vertex, with base vector b (tangent: b.xyz and b.w), the active
 * targets k in ascending order, their weights w_k and their delta vectors d_k:
 *   s = (0.0f, 0.0f, 0.0f), then for each active k in order:  s = s + w_k * d_k                          (per component)
 *   where every component of s is +0 or -0, the base's bytes are written for that vector (all 16 of its piece); otherwise
 *   position' = b + s
 *   normal'   = normalise(b + s)
 *   tangent'  = (normalise(b.xyz + s), b.w)
 *   normalise(v) = v * (1.0f / sqrt((v.x * v.x + v.y * v.y) + v.z * v.z)); where that squared length is 0 or not finite, the
 *               base's bytes are written for that vector.
 * Every other byte of the record (the fourth word of the three pieces, the five uv sets, the pads) is the base's; with all
 * weights 0 the output is the base byte for byte. */
int sr_scene_pose_mesh(SrScene* scene, uint64_t key, const float* weights, uint32_t n_targets, const SrTransform* joint_matrices, uint32_t n_joints,
                       void* stream);
typedef struct SrMeshMorphInfo {
    uint32_t n_targets;        /* targets of the attached morph; 0: the mesh has none */
    uint32_t posed;            /* accepted sr_scene_pose_mesh calls with a morph stage since the morph was attached */
    uint32_t n_active;         /* the last morph stage: weights that were not 0 */
    uint32_t first_bad;        /* the last morph stage: lowest vertex morphed to a non-finite position, 0xFFFFFFFF: none */
    double morph_ms;           /* the last accepted pose: the posing kernel (morph, and skin where asked) + read-back (events, only while sr_scene_enable_timing is on) */
} SrMeshMorphInfo;             /* 24 bytes */
int sr_scene_mesh_morph_info(const SrScene* scene, uint64_t key, SrMeshMorphInfo* out);
/* Batched posing: many meshes posed by one upload, one launch and one read-back (a crowd of small deforming meshes, in front of
 * the batched tree build of SR_BLAS_BATCH_ON). For each item the result is exactly what
 * sr_scene_pose_mesh(scene, key, weights, n_targets, joint_matrices, n_joints, stream) would leave: the same bytes in the mesh's
 * device vertices, the same mesh state, the same posed / skinned / n_active / first_bad figures. What differs:
 *   - Every host refusal of sr_scene_pose_mesh is decided for ALL items before any device work, with its status and its text
 *     behind "pose_meshes: item <i>: ". Refused as well (SR_ERR_INVALID_ARG): items == NULL with n_items > 0, a key named by two
 *     items, an item with neither stage; SR_ERR_UNSUPPORTED: a batch sr_pose_batch_plan refuses. n_items == 0 is SR_OK and does
 *     nothing.
 *   - One staging block (item rows, block table, all joint matrices, all active-target lists) is uploaded on `stream`, the check
 *     words (two per item: morph stage, skin stage) are preset once, ONE kernel poses every tile of every item into a scratch
 *     buffer the scene owns, and all check words come back in one read. An item with both stages keeps its morphed position,
 *     normal and tangent on chip between the stages; the bytes are those of morph-then-skin through memory.
 *   - All or nothing: if any item posed a vertex to a non-finite position the call returns sr_scene_update_mesh's status and text
 *     (behind the item prefix) for the lowest such item and that item's lowest such vertex of either stage, and no mesh of the
 *     batch has changed: neither bytes nor state nor counters. Only the first_bad of every stage that reported is recorded
 *     (the single calls record every stage that ran, as said above).
 *   - Accepted: one device wait (frames in flight read the old vertices), one scatter launch that copies every item's records
 *     from the scratch into its mesh's allocation, one wait, then, per item in item order, what sr_scene_update_mesh_device leaves
 *     behind on the host (stale host copy, the emissive handling of either SR_LIGHTS_* mode, the tree and structure marks).
 *     SrMeshMorphInfo.morph_ms / SrMeshSkinInfo.skin_ms of every item take the time of the one posing launch. */
typedef struct SrPoseItem {            /* one mesh of a batch; what sr_scene_pose_mesh takes, by value */
    uint64_t key;
    const float* weights;              /* host, n_targets floats, or NULL: no morph stage */
    const SrTransform* joint_matrices; /* host, n_joints x 48 bytes, or NULL: no skin stage */
    uint32_t n_targets, n_joints;
} SrPoseItem;                          /* 32 bytes */
int sr_scene_pose_meshes(SrScene* scene, const SrPoseItem* items, uint32_t n_items, void* stream);
typedef struct SrPoseBatchInfo {       /* the last sr_scene_pose_meshes that reached the device (a host refusal leaves it alone, and
                                        * so do sr_scene_skin_mesh and sr_scene_pose_mesh) */
    uint32_t items, blocks;            /* items of the call; blocks of the posing launch (256 vertices a block) */
    uint64_t vertices;                 /* records posed */
    uint32_t morph_only, skin_only, fused;   /* items by their stages */
    uint32_t launches;                 /* kernel launches: 2 accepted (pose, scatter), 1 refused */
    uint32_t read_backs;               /* device-to-host copies: 1 (all check words) */
    uint32_t calls;                    /* calls that reached the device since the scene was created */
    uint32_t refused_item, refused_vertex;   /* a non-finite refusal: the item and vertex named; 0xFFFFFFFF: accepted */
    uint64_t upload_bytes;             /* the staging block */
    double pose_ms, scatter_ms;        /* posing launch + read-back, scatter launch (events, only while sr_scene_enable_timing is on) */
    double host_ms;                    /* the whole call, wall clock */
} SrPoseBatchInfo;                     /* 80 bytes */
int sr_scene_pose_batch_info(const SrScene* scene, SrPoseBatchInfo* out);
/* The layout of a batch, host only: item i's first block of the posing launch (ceil(n_vertices[i] / 256) blocks an item, in item
 * order), its first record in the scratch, and the number of blocks in all. SR_ERR_UNSUPPORTED, with nothing written: 2^31
 * blocks or more, else 2^32 vertices or more. */
int sr_pose_batch_plan(const uint32_t* n_vertices, uint32_t n_items, uint32_t* first_block, uint64_t* vertex_base, uint32_t* n_blocks);
/* The mesh frame: the third producer of device vertices that lives in the library, for callers that know only the new POSITIONS
 * (a simulation, any torch code). It recomputes area-weighted normals, and uv-aligned tangents where asked, from the positions
 * and the mesh's own topology, and hands the records on as sr_scene_update_mesh_device does its caller's. The pose path
 * (sr_scene_skin_mesh, sr_scene_pose_mesh) is untouched and does not consult the frame: a mesh may carry a skin, a morph and a
 * frame, three independent producers, and the last accepted call of any of them is what the next sr_scene_set_instances applies.
 * The rule, fp32 under the numerics contract (no contraction, correctly rounded divide and sqrt, grouping as written). The
 * REFERENCE RECORDS are the mesh's vertices as they stand at the attach.
 *   Smoothing groups (fixed at the attach): two vertices belong to one group iff the 12 bytes of their reference position and the
 *     12 bytes of their reference normal are equal. Equal position and normal with another uv is a uv seam and is smoothed across;
 *     equal position with another normal is an authored hard edge and stays hard.
 *   Entries of vertex v: the corners (t, c) of the index buffer whose vertex is in v's group, in ascending (t, c) order, one entry
 *     per corner (a triangle with two corners in the group appears twice); the entry stores t.
 *   Face vectors of triangle t with indices i0, i1, i2 in index-buffer order (the same bits whichever vertex asks):
 *     e1 = p[i1] - p[i0], e2 = p[i2] - p[i0], F = e1 x e2 with a x b as written under sr_scene_skin_mesh;
 *     a = uv[i1] - uv[i0], b = uv[i2] - uv[i0] over the reference records' normal_tex_coord, det = a.x * b.y - b.x * a.y;
 *     det 0 or not finite: T = (+0, +0, +0); otherwise T.c = s * (e1.c * b.y - e2.c * a.y), s = +1.0f where det > 0, else -1.0f.
 *   Per vertex: N = (0, 0, 0), then N = N + F[t] over its entries in order; A likewise from the T[t].
 *     side = -1.0f where (N_ref.x * n.x + N_ref.y * n.y) + N_ref.z * n.z < 0 for N_ref, this same sum over the reference positions,
 *     and the reference normal n; else +1.0f. Computed once at the attach: the face side the mesh's own normals chose, whatever
 *     its winding.
 *     position' = x, y, z of the input
 *     normal'   = normalise(side * N)
 *     d         = (n'.x * A.x + n'.y * A.y) + n'.z * A.z, with n' the reference normal where the normal fell back
 *     tangent'  = (normalise(A.c - n'.c * d), reference w)
 *     normalise(v) = v * (1.0f / sqrt((v.x * v.x + v.y * v.y) + v.z * v.z)); where that squared length is 0 or not finite, the
 *     reference record's 16-byte piece is written for that vector.
 *   Every other byte of the record (the fourth word of the three pieces, the five uv sets, the pads) is the reference record's.
 *   Without SR_FRAME_TANGENTS the tangent piece is the reference's, byte for byte. */
#define SR_FRAME_NORMALS 1u
#define SR_FRAME_TANGENTS 2u  /* needs SR_FRAME_NORMALS: flags of 2 alone are refused */
/* The groups, runs and sides of the rule on their own (no scene, no device), as CSR: offsets_out takes n_vertices + 1 words,
 * entries_out *n_entries_out triangle indices (the sum over the vertices of their group's corner count: n_indices where every
 * group is one vertex), side_out n_vertices floats. Any out pointer may be NULL; with all three NULL the call only counts.
 * SR_ERR_INVALID_ARG: n_indices % 3 != 0, an index >= n_vertices (the text names the lowest offender), a null array that is not
 * empty. SR_ERR_OOM: more than 2^32 - 1 entries. */
int sr_mesh_frame_adjacency(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, uint32_t* offsets_out,
                            uint32_t* entries_out, float* side_out, uint32_t* n_entries_out);
/* The whole rule on the host, operation for operation the device's (the bytes are equal): `vertices` are the reference records,
 * `positions` n_vertices tight float[3], out_vertices n_vertices records. A position that is not finite: SR_ERR_INVALID_ARG, the
 * lowest such vertex in *first_bad_out (0xFFFFFFFF otherwise; may be NULL), out_vertices not written. Also refused: what
 * sr_mesh_frame_adjacency refuses, flags of 0, unknown flag bits, SR_FRAME_TANGENTS alone. */
int sr_mesh_frame_host(const SrVertex* vertices, uint32_t n_vertices, const uint32_t* indices, uint32_t n_indices, const float* positions,
                       uint32_t flags, SrVertex* out_vertices, uint32_t* first_bad_out);
/* Attaches a frame to a loaded mesh: fetches the host copy of its vertices where it is stale, builds groups, runs, sides and the
 * per-triangle uv terms from them, uploads those and snapshots the mesh's CURRENT device vertices as the reference records (a
 * device-to-device copy the mesh owns; waits for the device). Refused with SR_ERR_INVALID_ARG before anything is touched: a null
 * scene, an unknown key, unknown flag bits, SR_FRAME_TANGENTS without SR_FRAME_NORMALS. A failed allocation returns SR_ERR_OOM and
 * leaves an earlier frame in place. flags == 0 detaches the frame and frees its buffers; sr_scene_remove and sr_scene_destroy free
 * them too. Later sr_scene_update_mesh* calls do not move the reference records; attaching again snapshots them anew. */
int sr_scene_set_mesh_frame(SrScene* scene, uint64_t key, uint32_t flags);
/* New positions for a mesh with a frame, already in device memory of the scene's GPU: `d_positions` holds n_vertices tightly
 * packed float[3] (a contiguous [n, 3] float32 torch tensor), is 4-byte aligned, and was produced by work on `stream`. Two
 * kernels on `stream` write the new records into a scratch buffer the scene owns, which goes the way of
 * sr_scene_update_mesh_device: applied by the next sr_scene_set_instances, with the same SR_ERR_STATE window, the same stale host
 * copy and the same emissive handling. Refused on the host before anything is launched: a null scene or pointer, an unknown key,
 * a mesh with no frame, another vertex count, a misaligned pointer, a range that overlaps the mesh's own device allocation, a
 * pointer the HIP runtime does not report as device memory of the scene's device for that many positions (all
 * SR_ERR_INVALID_ARG; such a pointer is never dereferenced), an emissive list that is not one per triangle (SR_ERR_UNSUPPORTED).
 * The finite-position check (x, y, z) is part of the vertex kernel: on a bad position the call returns sr_scene_update_mesh's
 * status and text with the lowest offending index, and the scene is exactly as it was (only SrMeshFrameInfo.first_bad tells). */
int sr_scene_update_mesh_positions_device(SrScene* scene, uint64_t key, const float* d_positions, uint32_t n_vertices, void* stream);
/* The same with a HOST pointer: 12 bytes a vertex are uploaded asynchronously on `stream` into a scratch buffer of the scene
 * (sr_scene_update_mesh uploads 96), then the same kernels run. The bytes are those of the device call. */
int sr_scene_update_mesh_positions(SrScene* scene, uint64_t key, const float* positions, uint32_t n_vertices, void* stream);
typedef struct SrMeshFrameInfo {
    uint32_t flags;            /* SR_FRAME_* of the attached frame; 0: the mesh has none */
    uint32_t n_groups;         /* smoothing groups */
    uint32_t n_entries;        /* entries of all runs together */
    uint32_t max_valence;      /* the longest run */
    uint32_t updates;          /* accepted sr_scene_update_mesh_positions* calls since the frame was attached */
    uint32_t first_bad;        /* the last such call: lowest vertex with a non-finite position, 0xFFFFFFFF: none */
    double frame_ms;           /* the last accepted call: both kernels + 4-byte read-back (events, only while sr_scene_enable_timing is on) */
} SrMeshFrameInfo;             /* 32 bytes */
int sr_scene_mesh_frame_info(const SrScene* scene, uint64_t key, SrMeshFrameInfo* out);
/* BuildType of one mesh's tree (blas.rs:149-161: RapidlyChanging and SometimesChanges are built with ALLOW_UPDATE, Static is not).
 * Every loaded mesh starts as SR_BUILD_STATIC (Renderer::load_mesh, lib.rs:937): it is never refitted, every update rebuilds its
 * tree on the host. An updatable mesh holds an SrAsState of its own (reset to sr_as_state_initial(build_type) by this call), driven
 * as Blas::plan_op / mark_built drive it. In the two-level form the sr_scene_set_instances that applies an update refits the
 * mesh's tree on the device (Blas::update, blas.rs:292-310) while the state asks for SR_OP_UPDATE: leaf-order records, root box
 * and padding numbers are rewritten from the new vertices with the bytes a host build writes, the quantised nodes are refitted
 * bottom-up; topology, leaf order and stack need stay, and the top level may then be built on the device (SR_TL_BUILD_*). After
 * more than 8 updates since its last rebuild the state asks for SR_OP_FAST_BUILD: the device builds the mesh's tree anew
 * (Blas::rebuild; SR_MESH_TREE_BUILD_* below) or the host does. Refits and device builds of different meshes run in one call. The
 * host build takes over, silently and counted in blas_rebuilt, where the scene does not stand in the two-level form with its
 * mesh trees resident, where the previous or the new instance list holds an instance that needs a baked copy of its mesh, where
 * a pending mesh asks for SR_OP_SLOW_BUILD or its device build is not taken (SrMeshTreeInfo.reason), and for every refitted or
 * device-built mesh whenever the mesh trees are uploaded again (a host build, a mesh added or removed, a form switch): device
 * work and host rebuilds do not mix within one call. sr_scene_end_frame counts a quiet frame for every updatable mesh and
 * rebuilds the tree of one that asks for its settle build, on the host (the quality build). sr_scene_force_next_op(SR_OP_UPDATE)
 * forces the refit of the updated updatable meshes whatever their counters say, SR_OP_FAST_BUILD their fast build, SR_OP_SLOW_BUILD
 * the host rebuild. The type has no effect in the one-level form, which updates in place whatever the type: it is accepted and
 * remembered there. Unknown key or a type above SR_BUILD_STATIC: SR_ERR_INVALID_ARG. */
int sr_scene_set_mesh_build_type(SrScene* scene, uint64_t key, uint32_t build_type);
/* The mesh's build type, its own heuristic state and the operation the last sr_scene_set_instances / sr_scene_end_frame performed
 * on its tree in the two-level form (SR_OP_UPDATE: device refit, SR_OP_FAST_BUILD: device or host build, SR_OP_SLOW_BUILD: host
 * build). Any pointer may be NULL. */
int sr_scene_mesh_as_state(const SrScene* scene, uint64_t key, uint32_t* build_type, SrAsState* state, uint32_t* last_op);
/* Where the tree of an updatable mesh of the two-level form is built when its SrAsState asks for SR_OP_FAST_BUILD (the ninth update
 * since its last rebuild, or sr_scene_force_next_op; the reference rebuilds a BLAS on the GPU, blas.rs:285-310).
 * SR_MESH_TREE_BUILD_DEVICE: device kernels build it from the mesh's device vertex / index buffers (Morton sort + SR_FAST_BUILD
 * topology + budgeted 4-wide collapse, as the one-level fast build) into the mesh's part of the resident arrays: leaf-order
 * records, shading records, root box and padding numbers are byte for byte a host build's, the topology is not (the settle
 * rebuild restores the SAH tree). SR_MESH_TREE_BUILD_HOST: the host binned-SAH builder, always, followed by the upload of every
 * mesh's records. SR_MESH_TREE_BUILD_AUTO (default): the device from SrMeshTreeInfo.auto_threshold triangles per mesh on;
 * as measured no size qualifies and the threshold is 0xFFFFFFFF, never: auto is the host build. A device
 * tree deeper than 26 stack entries is refused (measured under the default topology: spheres of 65 536 triangles and more), so in
 * mode DEVICE too the fast build of a large mesh is the host's, with its cost, unless the height bound is switched on
 * (SR_HEIGHT_BOUND_REBALANCE below: the device then makes such a tree fit instead of refusing it). The first build, the settle rebuild, Static meshes and whatever sr_scene_set_mesh_build_type lists go to
 * the host in every mode. Queries give the same bits either way. SR_BLAS_BUILD = host | device | auto in the environment sets the
 * initial mode (anything else: auto). A mode above SR_MESH_TREE_BUILD_DEVICE: SR_ERR_INVALID_ARG. */
#define SR_MESH_TREE_BUILD_AUTO 0u
#define SR_MESH_TREE_BUILD_HOST 1u
#define SR_MESH_TREE_BUILD_DEVICE 2u
int sr_scene_set_mesh_tree_build(SrScene* scene, uint32_t mode);
/* Why the pending mesh trees of the last sr_scene_set_instances went to the host (SrMeshTreeInfo.reason). */
#define SR_MESH_TREE_ON_DEVICE 0u             /* they did not (or nothing was pending) */
#define SR_MESH_TREE_HOST_MODE 1u             /* SR_MESH_TREE_BUILD_HOST */
#define SR_MESH_TREE_HOST_BELOW_THRESHOLD 2u  /* auto mode, a mesh with fewer triangles than auto_threshold */
#define SR_MESH_TREE_HOST_SLOW_BUILD 3u       /* a mesh asked for SR_OP_SLOW_BUILD */
#define SR_MESH_TREE_HOST_BAKED_INSTANCE 4u   /* the previous or the new instance list needs a baked copy of a mesh */
#define SR_MESH_TREE_HOST_NOT_RESIDENT 5u     /* the mesh trees on the device do not match the set of meshes: first build, form switch, mesh added or removed */
#define SR_MESH_TREE_HOST_STACK_BUDGET 6u     /* the device tree would be deeper than the traversal stack allows a mesh tree (remembered per mesh: tried once) */
#define SR_MESH_TREE_HOST_STATIC_MESH 7u      /* a Static mesh was updated */
typedef struct SrMeshTreeInfo {
    uint32_t mode;             /* SR_MESH_TREE_BUILD_* in force */
    uint32_t auto_threshold;   /* triangles of a mesh from which auto mode builds on the device */
    uint32_t built_on_device;  /* mesh trees the last sr_scene_set_instances built on the device ... */
    uint32_t built_on_host;    /* ... and on the host: together SrMeshUpdateInfo.blas_rebuilt */
    uint32_t reason;           /* SR_MESH_TREE_ON_DEVICE or SR_MESH_TREE_HOST_* */
    uint32_t n_nodes;          /* nodes ... */
    uint32_t max_stack;        /* ... and worst-case stack entries of the last device-built tree */
    uint32_t _pad;
    double device_build_ms;    /* the device builds of that call, launch to completion (only while sr_scene_enable_timing is on) */
} SrMeshTreeInfo;              /* 40 bytes */
int sr_scene_mesh_tree_info(const SrScene* scene, SrMeshTreeInfo* out);

/* Batched device build of small mesh trees (off by default). After eight refits an updatable mesh's ninth update is a fast build;
 * the per-mesh device build above runs a launch per stage and a stream wait per PLOC iteration and collapse level, which makes
 * it the slowest path for a small mesh. With SR_BLAS_BATCH_ON the pending meshes of at most SR_BLAS_BATCH_MAX_TRIS triangles
 * are built by one launch, one workgroup per mesh (a few launches where the batch's scratch exceeds 256 MiB), with one
 * read-back for all of them: the same sort, the SR_FAST_BUILD topology, collapse, records and refit as the per-mesh build, so
 * the trees are the same up to node numbering. A mesh the kernel hands back (its binary tree is taller than the stack cap, or a
 * guard tripped) and every larger mesh go through the per-mesh build in the same call and behave as without the batch (refused
 * and remembered, or rebalanced under SR_HEIGHT_BOUND_REBALANCE). With the batch on, SR_MESH_TREE_BUILD_AUTO sends meshes of
 * at most SR_BLAS_BATCH_MAX_TRIS triangles to the device (larger ones below auto_threshold still send the call to the host);
 * SR_MESH_TREE_BUILD_HOST ignores the batch. SR_BLAS_BATCH=on|off in the environment sets the initial mode when the scene is
 * created (anything else: off). SrMeshTreeInfo.built_on_device counts batched and per-mesh builds together. mode > 1:
 * SR_ERR_INVALID_ARG, checked before the handle. */
#define SR_BLAS_BATCH_OFF 0u
#define SR_BLAS_BATCH_ON 1u
#define SR_BLAS_BATCH_MAX_TRIS 4096u
int sr_scene_set_mesh_tree_batch(SrScene* scene, uint32_t mode);
typedef struct SrMeshTreeBatchInfo {
    uint32_t mode;        /* SR_BLAS_BATCH_* in force */
    uint32_t max_tris;    /* SR_BLAS_BATCH_MAX_TRIS */
    uint32_t batched;     /* mesh trees the last sr_scene_set_instances built in batched launches */
    uint32_t passed_on;   /* meshes small enough for the batch that it handed to the per-mesh build (too tall, failed) */
    uint32_t launches;    /* batched launches of that call */
    uint32_t reserved;
    double batch_ms;      /* upload + launches + read-back, with timing on */
} SrMeshTreeBatchInfo;    /* 32 bytes */
int sr_scene_mesh_tree_batch_info(const SrScene* scene, SrMeshTreeBatchInfo* out);
/* What a device fast build does with a binary tree that is taller than its stack cap (26 entries for a mesh tree, what the mesh
 * trees leave of 47 for the top level, 47 for the one-level form). SR_HEIGHT_BOUND_REFUSE (default): the build is refused and the
 * host builds (SR_MESH_TREE_HOST_STACK_BUDGET, SR_TL_HOST_STACK_BUDGET, the host SAH build of the one-level form).
 * SR_HEIGHT_BOUND_REBALANCE: between the topology and the 4-wide collapse the device rebuilds the deepest, smallest offending
 * subtrees as median-split trees over their own leaves, so that the tree fits; the rest of the topology is kept, a tree that fits
 * costs nothing extra, and queries give the same bits either way. A build is then refused only where no tree over the primitives
 * fits the cap. mesh_tree_cap: 0 = the library's 26, or 1..26: the cap device builds of mesh trees are held to (the host builder
 * keeps 26); under REBALANCE SR_MESH_TREE_BUILD_AUTO uses a threshold of its own (SrMeshTreeInfo.auto_threshold reports the one in
 * force). The call forgets every remembered refusal. SR_FAST_BUILD_HEIGHT = refuse | rebalance in the environment sets the initial
 * mode (anything else: refuse). SR_ERR_INVALID_ARG: a mode above 1, a cap above 26, a non-zero cap under REFUSE. */
#define SR_HEIGHT_BOUND_REFUSE 0u
#define SR_HEIGHT_BOUND_REBALANCE 1u
int sr_scene_set_tree_height_bound(SrScene* scene, uint32_t mode, uint32_t mesh_tree_cap);
#define SR_TREE_KIND_ONE_LEVEL 0u
#define SR_TREE_KIND_TOP_LEVEL 1u
#define SR_TREE_KIND_MESH 2u
typedef struct SrTreeHeightInfo {      /* the last device fast build of that kind */
    uint32_t mode, mesh_tree_cap;      /* in force */
    uint32_t on_device;                /* 1: it produced the tree in use; 0: none yet, or the host took over */
    uint32_t cap;                      /* stack_cap it was held to */
    uint32_t height_before, height_after;   /* binary walk height of the topology / of what was collapsed */
    uint32_t subtrees_rebuilt, prims_rebuilt; /* 0, 0 when the tree fitted */
} SrTreeHeightInfo;                    /* 32 bytes */
int sr_scene_tree_height_info(const SrScene* scene, uint32_t kind, SrTreeHeightInfo* out);
/* Harness read-back of one mesh's part of the concatenated device arrays of a scene built in the two-level form (the counterpart
 * of sr_scene_read_top_level): n_nodes x 16 dwords with references local to the mesh, then per leaf-order slot 12 floats
 * (v0, v1, v2, primitive, 0, 0), 12 floats of `shade`, 24 floats of `shade_tex` (zeros where the scene has no textured
 * records), and per primitive its slot. Any pointer may be NULL (the counts alone size the arrays). SR_ERR_STATE when the scene
 * is not built in the two-level form or an update of the mesh is pending. */
int sr_scene_read_mesh_tree(const SrScene* scene, uint64_t key, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* nodes, float* tris,
                            float* shade, float* shade_tex, uint32_t* slot_of_prim);

/* Image::new_from_data (image/mod.rs:82-111): `channels` = 1..4 bytes per texel; fewer than 4 are
 * widened to R8G8B8A8_UNORM with the missing channels 0x00 (utils.rs:27-43), no sRGB decode. Host
 * pointer, w*h*channels bytes. Returns the image slot materials refer to (Material::*_image). */
int sr_scene_add_image(SrScene* scene, const uint8_t* data, uint32_t width, uint32_t height, uint32_t channels,
                       uint32_t* out_image_slot);
/* Frees an image added with sr_scene_add_image (ResourceManager::remove drops a key's images with its BLAS,
 * resource_manager.rs:459-472); the slot is handed out again by a later sr_scene_add_image. SR_ERR_STATE while a registered
 * mesh's material still names the slot. Waits for the device. */
int sr_scene_remove_image(SrScene* scene, uint32_t image_slot);

/* Sampler::new (image/sampler.rs:44-67). Returns the sampler slot (Material::*_sampler). */
int sr_scene_add_sampler(SrScene* scene, const SrSamplerDesc* desc, uint32_t* out_sampler_slot);
/* ResourceManager::frame_instance_data (resource_manager.rs:216-267) + the dummy-entry padding of
 * Renderer::render (lib.rs:1058-1081) + the TLAS build it queues (resource_manager.rs:346-363):
 * keys[i] is instanced counts[i] times with the next counts[i] row-major 3x4 transforms taken from
 * `transforms`. Instance order, transform table and emissive-indirection order follow the
 * reference loop exactly. Builds the world-space BVH over every instance's triangles (the
 * replacement for vkCmdBuildAccelerationStructuresKHR, accel.rs:134-138) and uploads it.
 * Unknown key -> SR_ERR_INVALID_ARG (resource_manager.rs:227-231). */
int sr_scene_set_instances(SrScene* scene, const uint64_t* keys, const uint32_t* counts,
                           uint32_t n_keys, const SrTransform* transforms);
/* The same for transforms that are already in device memory of the scene's device (work on `stream` produced them: rigid
 * bodies, particles, a crowd, a [n, 3, 4] tensor): no host round trip. `keys` and `counts` are host arrays as above;
 * `d_transforms` holds sum(counts) transforms. Refused before anything is launched, the pointer never dereferenced, with
 * SR_ERR_INVALID_ARG: a null scene or null arrays, an unknown key (the text of sr_scene_set_instances), a pointer that is not
 * 16-byte aligned, a pointer the HIP runtime does not report as device memory of the scene's device for that many bytes; and
 * with the statuses and texts of sr_scene_set_instances its size limits. One kernel (instances.hip) then writes the
 * per-instance device tables (WorldToObject by the host's arithmetic, operation for operation) into a second set of tables
 * and validates in the same pass: a component that is not finite is SR_ERR_INVALID_ARG with the text of
 * sr_scene_set_instances, the lowest such instance in SrInstanceUpdateInfo.bad_index, and the scene exactly as it was. Only
 * after the answer is read back and the device has been waited for do the two sets change places. What follows is what
 * sr_scene_set_instances does, with the same SrAsState accounting and the same reports: mesh-tree maintenance and the
 * top-level build in the two-level form; update in place, device fast build or host build in the one-level form; the light
 * table. The layout (mesh slot and triangle offset of each instance, the emissive entries) is built on the host and uploaded
 * only when keys or counts differ from the last successful call through either entry point: an unchanged layout costs
 * O(n_keys) on the host. The host copy of the transforms is left behind (SrInstanceUpdateInfo.host_stale) and fetched by
 * whatever host code reads it next: the host top-level records, a host one-level build, the host light table of a
 * non-empty arena, the baked-instance test of mesh-tree maintenance while a mesh has a pending update, the settle rebuild of
 * sr_scene_end_frame, sr_scene_get_tables when it is asked for transforms. The device paths never fetch; the first transform
 * alone (48 bytes, for the dummy light record of an empty arena) comes back with the validation word. */
int sr_scene_set_instances_device(SrScene* scene, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys,
                                  const SrTransform* d_transforms, void* stream);
/* Why the host copy of the transforms was fetched last (SrInstanceUpdateInfo.fetch_reason). */
enum {
    SR_INST_FETCH_NONE = 0,
    SR_INST_FETCH_HOST_TOP_LEVEL = 1,     /* host_tl_records: any SR_TL_HOST_* outcome, a baked instance included */
    SR_INST_FETCH_HOST_BUILD = 2,         /* the host one-level build (also below the device fast build's threshold) */
    SR_INST_FETCH_HOST_LIGHT_TABLE = 3,   /* SR_LIGHTS_HOST with a non-empty arena */
    SR_INST_FETCH_SETTLE = 4,             /* the settle rebuild of sr_scene_end_frame */
    SR_INST_FETCH_GET_TABLES = 5,         /* sr_scene_get_tables asked for transforms */
    SR_INST_FETCH_MESH_TREES = 6          /* mesh-tree maintenance with a pending or stale mesh looks for baked instances */
};
/* The last sr_scene_set_instances / sr_scene_set_instances_device and the fetches since. tables_ms is taken with events and
 * only while sr_scene_enable_timing is on (the kernel and its read-back); fetch_ms is wall clock. A refused device call
 * changes bad_index alone. */
typedef struct SrInstanceUpdateInfo {
    uint32_t from_device;      /* 1: the transforms came from device memory */
    uint32_t host_stale;       /* 1: the host copy of the transforms is older than the device tables */
    uint32_t host_fetches;     /* fetches of the host copy since that call (at most one) */
    uint32_t fetch_reason;     /* SR_INST_FETCH_* of the last one */
    uint32_t layout_rebuilt;   /* 1: the call built the layout on the host and / or uploaded it */
    uint32_t n_instances;
    uint32_t bad_index;        /* lowest instance with a non-finite component of the last refused device call; 0xFFFFFFFF: none */
    uint32_t _pad;
    double tables_ms, fetch_ms;
} SrInstanceUpdateInfo;          /* 48 bytes */
int sr_scene_instance_update_info(const SrScene* scene, SrInstanceUpdateInfo* out);
/* Harness read-back of the per-instance device tables, whichever path wrote them: n x 96 bytes (DevInstance: w2o[12],
 * o2w[12], the 3x3 parts in words 0..8) and n x 64 bytes (FlatInstance: the transform, tri_offset, mesh_slot, two pad words),
 * n = n_instances of sr_scene_get_tables; either pointer may be null. Waits for the device. */
int sr_scene_read_instance_tables(const SrScene* scene, void* dev_instances, void* flat_instances);
/* The host rule of the first of those tables on its own (no scene, no device): n x 96 bytes from n transforms. The host
 * entry point fills its table with it, and instances.hip restates it. */
int sr_instance_tables_host(const SrTransform* transforms, uint32_t n, void* dev_instances);

/* Introspection of the tables frame_instance_data produced (host copies; pointers valid until the
 * next sr_scene_set_instances / destroy). num_lights is the emissive_indirection length the
 * shaders read through GetDimensions (ray_gen_ris.slang:185-186), i.e. >= 1 because of the dummy. */
int sr_scene_get_tables(const SrScene* scene, const SrTransform** transforms, uint32_t* n_instances,
                        const SrEmissiveIndirectionEntry** indirection, uint32_t* num_lights,
                        const SrEmissiveTriangle** emissive_triangles, uint32_t* n_emissive,
                        const SrMeshInfo** meshes_info, uint32_t* n_meshes);

/* BVH statistics for roofline accounting. */
typedef struct SrBvhStats {
    uint64_t n_triangles;
    uint64_t n_nodes;     /* 4-wide nodes with quantised child boxes, 64 B each */
    uint64_t node_bytes;
    uint64_t tri_bytes;   /* 48 B per triangle record */
    uint32_t max_depth;   /* of the 4-wide tree */
    float sah_cost;
    uint32_t max_stack;   /* worst-case traversal stack entries (sizes the kernels' LDS stack) */
    uint32_t _pad;
    double build_ms;
} SrBvhStats;
int sr_scene_bvh_stats(const SrScene* scene, SrBvhStats* out);

/* global triangle index (SrHit.tri) -> (instance index, primitive index) */
int sr_scene_resolve_triangle(const SrScene* scene, uint32_t tri, uint32_t* instance,
                              uint32_t* primitive);

/* Host-only access to the BVH builder (no GPU needed): builds the same BVH sr_scene_set_instances
 * would build over n world-space triangles given as 9 floats each (v0, e1, e2), for structural
 * checks on machines without a device. nodes: 16 dwords per 4-wide quantised node, tris: 12 floats
 * per triangle in leaf order (layout: sunray_amd/csrc/traverse.h). max_stack: worst-case traversal
 * stack entries. */
typedef struct SrHostBvh SrHostBvh;
int sr_host_bvh_build(const float* v0_e1_e2, uint32_t n_triangles, SrHostBvh** out);
int sr_host_bvh_get(const SrHostBvh* bvh, const uint32_t** nodes, uint32_t* n_nodes, const float** tris,
                    uint32_t* n_triangles, uint32_t* max_depth, uint32_t* max_stack);
int sr_host_bvh_destroy(SrHostBvh* bvh);

/* ------------------------------------------------------------------------------------------ */
/* The hot path                                                                                 */
/* ------------------------------------------------------------------------------------------ */

/* TraceRay(tlas, RAY_FLAG_NONE, 0xFF, 0,0,0, ray, prd) minus the closest-hit shader
 * (ray_gen_ris.slang:75,332; ray_gen_final.slang:80): nearest triangle with tmin < t < tmax,
 * two-sided (resource_manager.rs:249), all geometry opaque (blas.rs:276).
 * rays/hits are device pointers to n elements. */
int sr_trace_closest(const SrScene* scene, const SrRay* rays, uint32_t n, SrHit* hits, void* stream);

/* TraceRay(tlas, ACCEPT_FIRST_HIT_AND_END_SEARCH | SKIP_CLOSEST_HIT_SHADER, ...)
 * (ray_gen_ris.slang:285-300,372-385; ray_gen_final.slang:203-216,274-287,304-319,361-373):
 * occluded[i] = 1 if any triangle has tmin < t < tmax, else 0 (the miss shader ran). */
int sr_trace_any(const SrScene* scene, const SrRay* rays, uint32_t n, uint32_t* occluded, void* stream);

/* closest_hit (closest_hit.slang:12-91) / ray_miss (ray_miss.slang:10-13) applied to hit records:
 * payloads[i] = the 32-byte RayPayload the reference shader would produce. Device pointers. */
int sr_shade_closest_hit(const SrScene* scene, const SrHit* hits, uint32_t n, SrRayPayload* payloads,
                         void* stream);

/* any_hit (any_hit.slang:11-43) applied to hit records: ignored[i] = 1 where the shader would call IgnoreHit() (the
 * mesh's material has alpha_mode != 0 and the base-colour alpha sampled at the hit's interpolated uv is below
 * alpha_cutoff), else 0. The traversal never runs it: every BLAS geometry carries the OPAQUE flag (blas.rs:276) and
 * Material::new forces alpha_mode = 0 (material.rs:74) — this hook exists so that the shader's lines have a device
 * counterpart with a parity test. Misses (t < 0) give 0. Device pointers. */
int sr_any_hit_ignores(const SrScene* scene, const SrHit* hits, uint32_t n, uint32_t* ignored, void* stream);

/* The inline helpers under the passes (the pinned transcendentals, the pack / unpack routines, the RNG, the BRDF and reservoir
 * helpers, the triangle test), one at a time on raw rows — this hook exists so that each of them has a device counterpart
 * with a parity test of its own, on inputs no frame reaches. Row i of `in` holds helper `fn`'s arguments as dwords (floats by
 * their bits, vectors as x y z, records as they lie in memory), row i of `out` receives its results; the widths of both rows
 * come from sr_probe_helper_layout. in / out are device pointers to n rows; an unknown fn, or a null pointer with n > 0, is
 * SR_ERR_INVALID_ARG and nothing is written. */
typedef enum SrProbeHelper {
    SR_PROBE_SINCOS = 0,        /* x -> sin, cos */
    SR_PROBE_EXP,
    SR_PROBE_LOG,
    SR_PROBE_POW,               /* x, y */
    SR_PROBE_POW5,
    SR_PROBE_SMOOTHSTEP,        /* a, b, x */
    SR_PROBE_F32_TO_F16,        /* float -> half bits */
    SR_PROBE_F16_TO_F32,        /* half bits -> float */
    SR_PROBE_PACK_HALF_2X16,
    SR_PROBE_UNPACK_HALF_2X16,
    SR_PROBE_PACK_SNORM_2X16,
    SR_PROBE_UNPACK_SNORM_2X16,
    SR_PROBE_PACK_UNORM_4X8,
    SR_PROBE_UNPACK_UNORM_RGB,
    SR_PROBE_PACK_NORMAL,
    SR_PROBE_UNPACK_NORMAL,
    SR_PROBE_PACK_RGBA8_SNORM,
    SR_PROBE_UNSNORM8,
    SR_PROBE_PACK_B10G11R11,
    SR_PROBE_UNPACK_B10G11R11,
    SR_PROBE_PCG_HASH,
    SR_PROBE_INIT_RNG,          /* px, py, frame, launch width -> seed */
    SR_PROBE_RND,               /* seed -> new seed, float */
    SR_PROBE_NORM3,
    SR_PROBE_REFLECT3,          /* i, n */
    SR_PROBE_REFRACT3,          /* i, n, eta */
    SR_PROBE_BUILD_ONB,         /* n -> t, b */
    SR_PROBE_SMITH_V_GGX,       /* NdotV, NdotL, alpha */
    SR_PROBE_SMITH_G1_GGX,      /* NdotX, alpha */
    SR_PROBE_RANDOM_BOUNCE,     /* normal, r1, r2 */
    SR_PROBE_SAMPLE_GGX_VNDF,   /* normal, V, roughness, r1, r2 */
    SR_PROBE_EVAL_LIGHT,        /* hit_pos, hit_normal, V, albedo, roughness, metallic, emission, light_pos, light_normal */
    SR_PROBE_GI_TARGET_PDF,     /* shade_pos, shade_normal, albedo, metallic, sample_pos, sample_radiance */
    SR_PROBE_MERGE,             /* SrReservoir r, SrReservoir new, p_hat, random -> r, taken */
    SR_PROBE_MERGE_GI,          /* SrReservoirGI r, SrReservoirGI new, p_hat, jacobian, random -> r, taken */
    SR_PROBE_TRANSFORM_POINT,   /* m[12], p */
    SR_PROBE_INTERSECT_TRI,     /* o, d, v0, e1, e2, tmin, tmax -> hit, t, u, v */
    SR_PROBE_COUNT
} SrProbeHelper;
int sr_probe_helper(uint32_t fn, const uint32_t* in, uint32_t n, uint32_t* out, void* stream);
int sr_probe_helper_layout(uint32_t fn, uint32_t* in_dwords, uint32_t* out_dwords);

/* The node step of the traversal on hand-made nodes, one per ray — a test hook (tests/test_gpu_node_step.py): the box tests of a
 * quantised node, the ray set-up, the entry into an instance and the padded box tests of the two-level form are reached by no
 * other hook. Row i is a whole scene of its own: a tree of ONE node whose single used child is a leaf of ONE triangle (the
 * two-level kinds: a top-level node whose leaf holds one instance, the root node of that instance's mesh, the raw instance
 * record). Every child dword of every node must be ~((0 << 3) | 1) in exactly one slot and -1 in the other three, or the call
 * is refused: such a walk pushes nothing, so `tris` of a row is 1 exactly when every box test on the way to the leaf accepted,
 * else 0, and `boxes` is 4 per node stepped. The traversal is the ray-list tracers' (per-ray tmin / tmax, counting variant).
 * rows / out are HOST pointers to n records; the call validates, uploads the rows as they are (blas_root and tri_offset of the
 * instance record are uploaded as 0), launches once and copies the results back. A refused call (unknown kind, null pointer
 * with n > 0, a node that breaks the rule above) returns SR_ERR_INVALID_ARG, launches nothing and writes nothing.
 * SR_NODE_PROBE_KEY runs no traversal: it applies the order-preserving key of the closest-hit minimum (ord_f32 / unord_f32) to
 * ray.origin[0] (a float) and ray.origin[1] (a key, by its bits): boxes = ord(f), tris = bits of unord(ord(f)), hit.tri = bits
 * of unord(key). */
typedef enum SrNodeProbeKind {
    SR_NODE_PROBE_CLOSEST = 0,
    SR_NODE_PROBE_ANY,
    SR_NODE_PROBE_CLOSEST_TL,
    SR_NODE_PROBE_ANY_TL,
    SR_NODE_PROBE_KEY,
    SR_NODE_PROBE_COUNT
} SrNodeProbeKind;
typedef struct SrNodeProbeRow {   /* 336 B */
    SrRay ray;
    uint32_t node[16];        /* the tree's only node (two-level kinds: the top-level tree's) */
    uint32_t tri[12];         /* the leaf's triangle record: v0, e1, e2, global index (two-level kinds: v0, v1, v2 in object space) */
    uint32_t mesh_node[16];   /* two-level kinds: the root node of the mesh's tree */
    uint32_t instance[32];    /* two-level kinds: the instance record as it lies in device memory (sr_scene_read_top_level) */
} SrNodeProbeRow;
typedef struct SrNodeProbeOut {   /* 24 B */
    uint32_t boxes, tris;     /* the row's traversal counters */
    SrHit hit;                /* closest kinds: the committed hit (t = -1, tri = 0xFFFFFFFF: miss); any kinds: tri = occluded, t u v = 0 */
} SrNodeProbeOut;
int sr_probe_node_step(uint32_t kind, const SrNodeProbeRow* rows, uint32_t n, SrNodeProbeOut* out);
/* The instance record of the two-level form for one transform (host only): csrc/tl_record.h's arithmetic with the library's own
 * baking limit, as the host and the device build call it. record_out: 128 bytes (w2o, o2w, pad_a, pad_b and — baked — flags
 * bit 0 and the identity w2o are set as the host build sets them; the other words 0); result_out: 0 = ok, 1 = no finite box,
 * 2 = baked. */
int sr_probe_tl_record(const float* o2w, const float* mesh_lo, const float* mesh_hi, float max_abs_vertex, float max_edge_sum,
                       void* record_out, uint32_t* result_out);
/* The "raytracing_ris" pass (lib.rs:1662-1705): one ray_gen_ris invocation per pixel
 * (ray_gen_ris.slang:12-440): G-buffer + ReSTIR-DI reservoir + ReSTIR-GI initial reservoir. */
int sr_trace_ris(const SrRtParams* params, void* stream);

/* The "raytracing_final" pass (lib.rs:1714-1755): one ray_gen_final invocation per pixel
 * (ray_gen_final.slang:11-436): writes raw_color. Must be enqueued after sr_trace_ris on the same
 * stream when config.enable_restir != 0 (the reservoir hand-off edge, lib.rs:1688-1690). */
int sr_trace_final(const SrRtParams* params, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Post-RT compute chain: what turns raw_color into the presented RGBA8 image    */
/* ------------------------------------------------------------------------------------------ */

/* The compute passes Renderer::build_unified_graph appends after the two ray-tracing passes
 * (src/lib.rs:1576-1615). Images keep the reference's formats (lib.rs:452-461,1492-1516): the
 * accumulation and denoise ping-pong images are B10G11R11_UFLOAT_PACK32, the output R8G8B8A8_UNORM.
 * raw_color is this library's fp32 RGBA radiance; it is rounded to B10G11R11 when read, which is
 * where the reference quantises it (its raw_color image has that format). All device pointers. */
typedef struct SrPostParams {
    const float* raw_color;          /* 4*W*H floats, written by sr_trace_final                     */
    const uint32_t* motion_vec_img;  /* R16G16_SFLOAT, written by sr_trace_ris                      */
    const uint16_t* depth_img;       /* R16_SFLOAT                                                   */
    const uint32_t* normal_img;      /* R8G8B8A8_SNORM (roughness in .a)                             */
    const uint32_t* diffuse_img;     /* B10G11R11                                                    */
    uint32_t* accum[2];              /* temporal ping-pong: target = frame_count % 2 (lib.rs:1360-1361) */
    uint32_t* denoise[2];            /* a-trous ping-pong a / b (lib.rs:1817-1826)                    */
    uint32_t* output_rgba8;          /* W*H, R8G8B8A8_UNORM                                          */
    uint32_t frame_count;            /* relative_frame_count                                         */
    uint32_t width, height;
    float exposure;                  /* EXPOSURE = 1.0 (lib.rs:44)                                   */
    uint32_t denoise_passes;         /* DENOISE_PASSES = 4 (lib.rs:42); step width 1 << pass          */
    uint32_t _pad;
} SrPostParams;

/* "temporal_accumulation" (shaders/temporal_accumulation.slang:60-132, lib.rs:1761-1798):
 * 3x3 luma-gated neighbourhood clamp of the bilinearly reprojected history, lerp 0.14. */
int sr_post_temporal(const SrPostParams* params, void* stream);
/* "denoise_0..N-1" (shaders/denoise.slang:29-116, lib.rs:1800-1870): 5x5 a-trous B-spline with
 * depth / normal / albedo / luma edge stopping on albedo-demodulated illumination. Pass 0 reads
 * accum[frame_count % 2]; the result of the last pass is in denoise[(denoise_passes - 1) % 2]. */
int sr_post_denoise(const SrPostParams* params, void* stream);
/* "postprocess" (shaders/postprocess.slang:22-42, lib.rs:1872-1906): NaN/Inf scrub, exposure,
 * ACES (Narkowicz), gamma 1/2.2, RGBA8 store. Reads denoise[(denoise_passes - 1) % 2]. */
int sr_post_tonemap(const SrPostParams* params, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Renderer facade: the reference's Renderer<K> method surface for the built path */
/* ------------------------------------------------------------------------------------------ */
typedef struct SrRenderer SrRenderer;

/* Renderer::new((w, h), RGBA8_UNORM) (src/lib.rs:212-446): scene + G-buffer + temporal resources
 * (reservoir, accumulation and denoise ping-pongs, lib.rs:320-331) + the noise texture. */
int sr_renderer_create(int device, uint32_t width, uint32_t height, SrRenderer** out);
int sr_renderer_destroy(SrRenderer* renderer);
/* Renderer::resize (lib.rs:586-639): waits for the device, recreates every image at the new extent,
 * relative_frame_count = 0. Same extent: no-op (lib.rs:598-600). */
int sr_renderer_resize(SrRenderer* renderer, uint32_t width, uint32_t height);

/* Frame / resize callbacks (src/lib.rs:537-554). A start-of-frame callback runs once, on the caller's thread, at the
 * start of the next sr_renderer_render (before any per-frame work); an end-of-frame callback runs once the next
 * rendered frame has COMPLETED ON THE GPU — checked at the start of later sr_renderer_render calls, as the reference
 * drains them there (lib.rs:1004-1010) — the deferred-deallocation hook; a resize callback is persistent and runs on
 * every sr_renderer_resize call with the new extent (lib.rs:586-594). Callbacks run in registration order. */
typedef void (*SrFrameCallback)(void* user);
typedef void (*SrResizeCallback)(void* user, uint32_t width, uint32_t height);
int sr_renderer_add_start_of_frame_callback(SrRenderer* renderer, SrFrameCallback callback, void* user);
int sr_renderer_add_end_of_frame_callback(SrRenderer* renderer, SrFrameCallback callback, void* user);
int sr_renderer_add_resize_callback(SrRenderer* renderer, SrResizeCallback callback, void* user);
/* Renderer::load_mesh (lib.rs:873-954); host pointers. */
int sr_renderer_load_mesh(SrRenderer* renderer, uint64_t key, const SrVertex* vertices, uint32_t n_vertices,
                          const uint32_t* indices, uint32_t n_indices, const SrMaterial* material);
/* Knobs for the ray-tracing passes (defaults = the reference's constants). */
int sr_renderer_set_config(SrRenderer* renderer, const SrTraceConfig* config);
/* Renderer::render(camera, instances) (lib.rs:984-1232): enqueues one whole frame (acceleration-structure update /
 * rebuild if the instance list changed, raytracing_ris, raytracing_final, temporal_accumulation, denoise_0..3,
 * postprocess) on the renderer's OWN two streams, ordered after whatever is already enqueued on `stream`, and returns
 * its frame number. Two frames may be in flight (MAX_FRAMES_IN_FLIGHT, lib.rs:71): per-frame images are double-buffered
 * and the RIS pass of frame f+1 overlaps the final pass and post chain of frame f when the caller submits f+1 before
 * waiting for f. Frames complete in order; results equal back-to-back execution. */
int sr_renderer_render(SrRenderer* renderer, const float cam_pos[3], const float cam_target[3], float fov_y_degrees,
                       const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* transforms,
                       void* stream, uint64_t* out_frame);
/* sr_renderer_render with the instance list taken from device memory on the first device slot's GPU (work on `stream` produced
 * it): sr_scene_set_instances_device there, which validates the transforms once; the further replicas take them by a
 * device-to-device (peer) copy, as with sr_renderer_update_mesh_device. The list always counts as changed (there is no host
 * copy to compare with, and the one a later sr_renderer_render compares against is void). A refusal changes no replica. */
int sr_renderer_render_device_transforms(SrRenderer* renderer, const float cam_pos[3], const float cam_target[3], float fov_y_degrees,
                                         const uint64_t* keys, const uint32_t* counts, uint32_t n_keys, const SrTransform* d_transforms,
                                         void* stream, uint64_t* out_frame);
/* Renderer::wait_frame (lib.rs:1234-1238). */
int sr_renderer_wait_frame(SrRenderer* renderer, uint64_t frame);
/* Renderer::render_to_host_memory (lib.rs:1908-1934): 16 x (render + wait_frame), then the RGBA8 image
 * (width*height*4 bytes, no padding) copied to out_rgba8 (host). */
int sr_renderer_render_to_host_memory(SrRenderer* renderer, const float cam_pos[3], const float cam_target[3],
                                      float fov_y_degrees, const uint64_t* keys, const uint32_t* counts, uint32_t n_keys,
                                      const SrTransform* transforms, uint8_t* out_rgba8);
/* ------------------------------------------------------------------------------------------ */
/* glTF ingest                                                                  */
/* ------------------------------------------------------------------------------------------ */
/* Host-side parse: Gltf::new + create_default_scene (gltf/mod.rs:57-373) and the CPU side of
 * Scene::load_into_gpu (scene.rs:52-176). `.glb` or `.gltf` (+ external / data: buffers); images: 8-bit PNG and JPEG
 * (baseline, extended sequential, progressive; what `gltf::import` hands on as R8 / RG8 / RGB8 / RGBA8; JPEG texels are
 * decoder-defined within a few units: parity unpinned, csrc/jpeg_decode.cpp). 16-bit PNG (the reference stops there too,
 * image/mod.rs:98-104), CMYK / arithmetic-coded JPEG, camera/light nodes -> SR_ERR_UNSUPPORTED. Sparse accessors are resolved
 * (zeros or the bufferView, with `count` elements substituted), as the gltf crate's readers do. No device needed. */
typedef struct SrGltf SrGltf;
/* The loader's image decoder on its own: extent + channels, and the pixels when `pixels` != NULL (cap >= w*h*channels). */
int sr_decode_image(const uint8_t* data, size_t n, uint32_t* width, uint32_t* height, uint32_t* channels, uint8_t* pixels, size_t cap);
/* image::load_from_memory(bytes).to_rgba8() — lib.rs:281-283 (the embedded blue-noise texture, a 16-bit greyscale PNG) and the png
 * example's host side: any PNG / JPEG above plus 16-bit PNG, widened to RGBA8 (grey -> r = g = b, no alpha -> 255, 16-bit sample v ->
 * (v + 128) / 257 as image-rs 0.25 narrows it). `pixels` may be NULL to query the extent; cap >= w * h * 4. */
int sr_decode_image_rgba8(const uint8_t* data, size_t n, uint32_t* width, uint32_t* height, uint8_t* pixels, size_t cap);
int sr_gltf_open(const char* path, SrGltf** out);
int sr_gltf_close(SrGltf* gltf);
int sr_gltf_counts(const SrGltf* gltf, uint32_t* n_blases, uint32_t* n_instances, uint32_t* n_images,
                   uint32_t* n_samplers, uint32_t* n_textures);
/* One unique BLAS (scene.rs:16-24). `material` is UNRESOLVED like the reference's gltf::Material: its *_image
 * fields hold glTF texture indices (or SR_NULL_TEXTURE), its *_sampler fields SR_NULL_TEXTURE. */
int sr_gltf_blas(const SrGltf* gltf, uint32_t i, const SrVertex** vertices, uint32_t* n_vertices,
                 const uint32_t** indices, uint32_t* n_indices, SrMaterial* material,
                 const SrEmissiveTriangle** emissive, uint32_t* n_emissive);
/* i-th (blas index, world transform) of LoadedScene::instances (scene.rs:31-33), node-traversal order. */
int sr_gltf_instance(const SrGltf* gltf, uint32_t i, uint32_t* blas_index, SrTransform* transform);
int sr_gltf_image(const SrGltf* gltf, uint32_t i, const uint8_t** pixels, uint32_t* width, uint32_t* height,
                  uint32_t* channels);
int sr_gltf_sampler(const SrGltf* gltf, uint32_t i, SrSamplerDesc* out);
/* textures[i] = {sampler: Option<usize> (-1 = none -> the default LINEAR / CLAMP_TO_EDGE sampler,
 * resource_manager.rs:128-136,393), source image}. */
int sr_gltf_texture(const SrGltf* gltf, uint32_t i, int32_t* sampler, uint32_t* source);

/* Rig and animation of the file (glTF 2.0 skins and animations). sr_gltf_open returns for every file what it returned before
 * these existed; skins and animations are parsed and validated when one of the calls below first asks for them, and a malformed
 * one is reported by that call (SR_ERR_INVALID_ARG, or SR_ERR_UNSUPPORTED where stated), never by sr_gltf_open. Pointers handed
 * out stay valid until sr_gltf_close. */
int sr_gltf_rig_counts(const SrGltf* gltf, uint32_t* n_skins, uint32_t* n_animations);
/* The skin of blas i: that of the first node that instances it (*skin_index = -1, *influences = NULL: none), and one
 * SrSkinInfluence per vertex of sr_gltf_blas, in its order, from JOINTS_0 (u8 / u16) and WEIGHTS_0 (f32, or normalised u8 / u16
 * divided by 255 / 65535 in fp32), as given: nothing is renormalised or checked against the skin's joint count
 * (sr_scene_set_mesh_skin does that). SR_ERR_UNSUPPORTED: a primitive instanced by nodes with different skins, JOINTS_1 /
 * WEIGHTS_1 present, WEIGHTS_0 without JOINTS_0 or the reverse. */
int sr_gltf_blas_skin(const SrGltf* gltf, uint32_t blas_index, int32_t* skin_index, const SrSkinInfluence** influences, uint32_t* n_vertices);
/* Skin i: its joint count, the inverse bind matrices (n_joints rows of 3x4; identity where the file has no accessor) and the
 * node index of every joint. */
int sr_gltf_skin(const SrGltf* gltf, uint32_t i, uint32_t* n_joints, const SrTransform** inverse_bind, const uint32_t** joint_nodes);
/* Animation i: its name ("" when the file gives none), the last key time of its samplers, and the number of channels the file
 * lists. `weights` channels (morph targets) are among them but are not sampled by sr_gltf_pose (sr_gltf_morph_weights samples
 * them): sr_gltf_animation_ignored_channels counts them. */
int sr_gltf_animation(const SrGltf* gltf, uint32_t i, const char** name, float* duration_seconds, uint32_t* n_channels);
int sr_gltf_animation_ignored_channels(const SrGltf* gltf, uint32_t i, uint32_t* n_weights_channels);
/* CUBICSPLINE samplers, per opened file. SR_CUBICSPLINE_REFUSE (the default) answers them as ever: sr_gltf_pose,
 * sr_gltf_sample_node, sr_gltf_morph_weights and sr_gltf_bake_clip return SR_ERR_UNSUPPORTED, and a cubic `weights` channel makes
 * a clip's morph set SR_CLIP_MORPH_UNAVAILABLE. Under SR_CUBICSPLINE_SAMPLE the four calls sample them (the rule: sr_gltf_pose).
 * The mode is read where a call meets such a sampler; what the file's animations parsed to does not depend on it, so it may be
 * switched back and forth. A clip keeps what it was baked with. No environment variable selects it. Another value:
 * SR_ERR_INVALID_ARG. sr_gltf_animation_cubic: how many translation / rotation / scale channels and how many `weights` channels
 * of animation i name a CUBICSPLINE sampler (either may be NULL), in either mode: 0 and 0 where the animation needs no mode. */
#define SR_CUBICSPLINE_REFUSE 0u
#define SR_CUBICSPLINE_SAMPLE 1u
int sr_gltf_set_cubicspline(SrGltf* gltf, uint32_t mode);
int sr_gltf_cubicspline(const SrGltf* gltf, uint32_t* mode);
int sr_gltf_animation_cubic(const SrGltf* gltf, uint32_t i, uint32_t* n_cubic_trs_channels, uint32_t* n_cubic_weights_channels);
/* The file's nodes at `time_seconds` of animation `animation` (-1: the file's static pose, time ignored): the world transform
 * of every instance of sr_gltf_instance, in its order, into instance_transforms (n_instances, may be NULL), and the joint matrices
 * of skin `skin` into joint_matrices (that skin's n_joints, may be NULL; `skin` is not looked at then).
 * Sampling: every translation / rotation / scale channel at time_seconds clamped to its sampler's first / last key; STEP and LINEAR
 * (rotations: spherical linear interpolation along the shorter arc between the normalised keys, the result normalised), computed
 * in double from the fp32 keys and rounded once to fp32 TRS; a CUBICSPLINE sampler anywhere in the animation: SR_ERR_UNSUPPORTED,
 * unless sr_gltf_set_cubicspline(gltf, SR_CUBICSPLINE_SAMPLE) has been called. Then a cubic sampler, whose output holds per key
 * an in-tangent a_k, a value v_k and an out-tangent b_k, is sampled between keys i and i + 1 at u = (time - t_i) / td,
 * td = t_{i+1} - t_i, per component as
 *   u2 = u*u; u3 = u2*u;  h00 = (2*u3 - 3*u2) + 1;  h10 = (u3 - 2*u2) + u;  h01 = 3*u2 - 2*u3;  h11 = u3 - u2;
 *   r = ((h00*v_i + h10*(td*b_i)) + h01*v_{i+1}) + h11*(td*a_{i+1})
 * in double with this grouping, rounded once; at a key, below the first and above the last (u == 0) r is the key's value. The
 * keys of a cubic rotation are taken as the file gives them, neither normalised nor sign-flipped; r is normalised in every case,
 * and a zero r stays zero, which composes as the identity rotation.
 * Composition: a node with an animated channel composes from its TRS (the file's, or the glTF defaults) even if the file gave it a
 * `matrix`; local and world matrices are composed as the load composes them, in fp32 and in the same order, so the static pose
 * returns the transforms of sr_gltf_instance bit for bit.
 * Joint matrices: inverse(world(mesh node)) * world(joint node) * inverseBind, multiplied left to right in fp32 by the load's
 * matrix product, where the mesh node is the first instanced node that names the skin and the inverse is the double-precision
 * inverse of the two-level form's instance records rounded to fp32 (a singular mesh-node transform: SR_ERR_UNSUPPORTED). Posing
 * the mesh's vertices with them and keeping the instance's own transform gives the world-space result of the glTF specification,
 * in which a skinned mesh's node transform does not count. */
int sr_gltf_pose(const SrGltf* gltf, int32_t animation, float time_seconds, SrTransform* instance_transforms, uint32_t skin,
                 SrTransform* joint_matrices);
/* The translation, rotation (x, y, z, w) and scale that sr_gltf_pose composes node `node` from at that time: the sampled values
 * of its animated channels (*animated: bit 0 translation, bit 1 rotation, bit 2 scale; may be NULL), the file's (or the glTF
 * defaults) for the others. For a node without an animated channel that is informative only: such a node composes from its
 * `matrix` where the file gives one. */
int sr_gltf_sample_node(const SrGltf* gltf, int32_t animation, float time_seconds, uint32_t node, float translation[3], float rotation[4],
                        float scale[3], uint32_t* animated);
/* Morph targets of the file, parsed and validated like the rig: when one of the two calls below first asks, never by
 * sr_gltf_open; sr_gltf_animation and sr_gltf_animation_ignored_channels return what they returned before these existed.
 * The targets of blas i: those of the primitive of the first node that instances it. *deltas is target-major (n_targets *
 * n_vertices records, sr_scene_set_mesh_morph's layout) in the vertex order of sr_gltf_blas, from the POSITION, NORMAL and TANGENT
 * accessors of every target (float VEC3; sparse accessors resolved; an absent attribute gives zeros; the pads are 0);
 * *default_weights is node.weights of that first node, else mesh.weights, else zeros. *n_targets == 0 with NULL pointers: the
 * blas has no targets. SR_ERR_UNSUPPORTED: another component type than float, a target attribute other than those three
 * (TEXCOORD_n, COLOR_n), nodes instancing the blas whose weights differ. SR_ERR_INVALID_ARG: an accessor shorter than POSITION,
 * accessors of the primitive's targets whose counts disagree, a `weights` array that is not n_targets finite numbers. */
int sr_gltf_blas_morph(const SrGltf* gltf, uint32_t blas_index, uint32_t* n_targets, const SrMorphDelta** deltas, uint32_t* n_vertices,
                       const float** default_weights);
/* The weights of blas i's targets at `time_seconds` of animation `animation` into weights_out (n_targets must be the blas's):
 * the first `weights` channel that targets the blas's first instancing node, under sr_gltf_pose's sampling rules: time clamped to
 * the sampler's first / last key, STEP and LINEAR, computed in double from the fp32 keys and rounded once to fp32; a CUBICSPLINE
 * sampler on that channel: SR_ERR_UNSUPPORTED, or under SR_CUBICSPLINE_SAMPLE sr_gltf_pose's cubic rule per target, its output
 * accessor holding 3 * n_keys * n_targets float scalars (per key n_targets in-tangents, values, out-tangents; a shorter one:
 * SR_ERR_INVALID_ARG). The output accessor holds n_keys * n_targets float scalars; a shorter one, key
 * times that are not finite, negative or not strictly increasing, a value that is not finite: SR_ERR_INVALID_ARG. animation == -1,
 * or no such channel: the default weights of sr_gltf_blas_morph. */
int sr_gltf_morph_weights(const SrGltf* gltf, int32_t animation, float time_seconds, uint32_t blas_index, float* weights_out, uint32_t n_targets);

/* A baked clip: an immutable flat form of everything sr_gltf_pose re-derives from the document on every call, for one animation
 * of the file (-1: the file's static pose). It does not refer to `gltf` afterwards. It holds
 *   nodes      the nodes sr_gltf_pose reaches from the default scene's roots, parent before child, grouped by depth level (a
 *              level table): parent, glTF node index, animated mask, the file's TRS, and the node's matrix as the load reads it;
 *   channels   the translation / rotation / scale channels that target such a node: clip node, path, interpolation, and their
 *              slice of the key times and values (the file's fp32 bytes). Of two channels on one node and path the later one
 *              is kept, which is what sr_gltf_pose's loop leaves;
 *   skins      every skin an instanced node wears, in file order: joint nodes, inverse bind matrices, the mesh node (the first
 *              instanced node wearing it) and its offset in the clip's concatenated joint list;
 *   instances  the clip node of every instance, in sr_gltf_instance order.
 * A CUBICSPLINE channel is baked under SR_CUBICSPLINE_SAMPLE only, with three rows a key (in-tangent, value, out-tangent, the
 * file's order); the clip keeps it whatever the file's mode becomes later, and a clip without such a channel is byte for byte
 * the block it is under SR_CUBICSPLINE_REFUSE.
 * Refused in sr_gltf_pose's statuses and words behind "sr_gltf_bake_clip: ": a CUBICSPLINE sampler (SR_ERR_UNSUPPORTED), a joint
 * node that is not part of the scene, a hierarchy that is too deep, every sampler error the loader reports. Refused as well
 * (SR_ERR_UNSUPPORTED): a node the roots reach twice, and a clip of more than SR_CLIP_MAX_NODES nodes (the text gives both
 * counts): the device kernel keeps a clip's nodes in static LDS. */
#define SR_CLIP_MAX_NODES 384u
typedef struct SrClip SrClip;
typedef struct SrClipInfo {
    int32_t animation;                 /* as baked; -1: the static pose */
    uint32_t n_nodes, n_levels, n_channels, n_skins, n_joints /* of all skins */, n_instances, n_keys /* of all channels */;
    float duration_seconds;            /* the last key time of the kept channels; 0 without channels */
    uint32_t device_bytes;             /* the one block sr_scene_attach_clip uploads */
} SrClipInfo;                          /* 40 bytes */
typedef struct SrClipNodeInfo { uint32_t parent /* clip node, 0xFFFFFFFF: a root */, gltf_node, animated, level; } SrClipNodeInfo;
typedef struct SrClipChannelInfo { uint32_t node /* clip node */, path /* 0 translation, 1 rotation, 2 scale */, interpolation /* SR_CLIP_LINEAR 0, SR_CLIP_STEP 1, SR_CLIP_CUBICSPLINE 2 */, n_keys; } SrClipChannelInfo;
#define SR_CLIP_LINEAR 0u
#define SR_CLIP_STEP 1u
#define SR_CLIP_CUBICSPLINE 2u
int sr_gltf_bake_clip(const SrGltf* gltf, int32_t animation, SrClip** out);
int sr_clip_destroy(SrClip* clip);
int sr_clip_info(const SrClip* clip, SrClipInfo* out);
/* Skin `skin` (the file's index) of the clip: its first matrix in the clip's concatenated joint list, and its joint count.
 * SR_ERR_INVALID_ARG: no instanced node wears that skin. */
int sr_clip_skin(const SrClip* clip, uint32_t skin, uint32_t* first_matrix, uint32_t* n_joints);
/* The layout, for inspection: n_nodes node records, n_channels channel records, the clip node of every instance (any may be NULL). */
int sr_clip_layout(const SrClip* clip, SrClipNodeInfo* nodes, SrClipChannelInfo* channels, uint32_t* instance_nodes);
/* Channel `channel`'s keys as the clip holds them: n_keys times and n_keys x 3 (rotation: x 4) values; a SR_CLIP_CUBICSPLINE
 * channel: n_keys x 3 rows of that width, per key its in-tangent, value and out-tangent; valid until sr_clip_destroy. */
int sr_clip_channel_keys(const SrClip* clip, uint32_t channel, const float** times, const float** values);
/* The morph sets of a clip: one for every blas of the file that has morph targets, holding what
 * sr_gltf_morph_weights(gltf, animation, t, blas, ...) derives from the document: the blas and its first instancing node, the
 * default weights, and where the baked animation has a `weights` channel on that node (the first one) its interpolation, key
 * times and n_keys x n_targets values, the file's fp32 bytes. They are further tables of the clip's one block. SrClipInfo's
 * n_channels, n_keys and duration_seconds and sr_clip_layout count the translation / rotation / scale channels only.
 * A set sr_gltf_morph_weights would refuse (a CUBICSPLINE sampler on that channel, a sampler error, a short output accessor, the
 * morph parse of the blas failing) does not refuse the bake: it is kept as SR_CLIP_MORPH_UNAVAILABLE with the loader's status and
 * words, and naming it later refuses in those.
 * sr_clip_morph_count: the number of sets. sr_clip_morph: the set of blas `blas`; for an unavailable set the call succeeds and
 * sr_last_error() holds the loader's words. A blas without morph targets: SR_ERR_INVALID_ARG.
 * sr_clip_morph_keys: the set's n_keys times and n_keys x n_targets values (NULL without a channel) and its n_targets default
 * weights, valid until sr_clip_destroy; an unavailable set refuses with its status and words. A SR_CLIP_CUBICSPLINE set (a cubic
 * `weights` channel baked under SR_CUBICSPLINE_SAMPLE; under SR_CUBICSPLINE_REFUSE it is unavailable) is SR_CLIP_MORPH_CHANNEL
 * and holds n_keys x 3 x n_targets values: per key n_targets in-tangents, values, out-tangents.
 * sr_clip_weights_host: the host rule, sr_gltf_morph_weights restated over the set and held to it bit for bit, in its statuses
 * and words too (a time that is not finite, another n_targets). The device kernel (clip_weights_kernel) includes the same
 * arithmetic (csrc/clip_rule.h): +, -, x, / on fp32 and fp64 only, so the device equals it bit for bit without exception. */
#define SR_CLIP_MORPH_CHANNEL 0u       /* a LINEAR or STEP `weights` channel, or a CUBICSPLINE one baked under SR_CUBICSPLINE_SAMPLE */
#define SR_CLIP_MORPH_DEFAULTS 1u      /* no channel (or the static pose): the default weights at every time */
#define SR_CLIP_MORPH_UNAVAILABLE 2u
typedef struct SrClipMorphInfo {
    uint32_t blas, gltf_node /* 0xFFFFFFFF: the morph parse failed */, n_targets, n_keys;
    uint32_t interpolation;            /* SR_CLIP_LINEAR 0, SR_CLIP_STEP 1, SR_CLIP_CUBICSPLINE 2 */
    uint32_t state;                    /* SR_CLIP_MORPH_* */
    int32_t status;                    /* SR_OK, or what refused an unavailable set */
    uint32_t reserved;
} SrClipMorphInfo;                     /* 32 bytes */
int sr_clip_morph_count(const SrClip* clip, uint32_t* n_sets);
int sr_clip_morph(const SrClip* clip, uint32_t blas, SrClipMorphInfo* out);
int sr_clip_morph_keys(const SrClip* clip, uint32_t blas, const float** times, const float** values, const float** default_weights);
int sr_clip_weights_host(const SrClip* clip, float time_seconds, uint32_t blas, float* weights_out, uint32_t n_targets);
/* The host rule: sr_gltf_pose restated over the baked clip, held to it bit for bit. The device kernel includes the same
 * arithmetic (csrc/clip_rule.h); host and device are built without contraction.
 * sr_clip_sample_host: n_nodes records, clip-node order: every node's TRS at time_seconds (sr_gltf_sample_node's values for the
 * node's glTF index) and its animated mask. A time that is not finite: SR_ERR_INVALID_ARG, unless the clip is the static pose.
 * sr_clip_compose_host: from such records, the joint matrices of all skins (n_joints of SrClipInfo, each skin at its
 * sr_clip_skin offset; may be NULL) and the instance transforms (n_instances; may be NULL), premultiplied by *placement where
 * given (the joint matrices are not). A singular mesh-node transform, looked for only where joint matrices are asked for:
 * SR_ERR_UNSUPPORTED in sr_gltf_pose's words, with the lowest such skin (position in the clip) in *singular_skin (may be NULL;
 * 0xFFFFFFFF otherwise); the instance transforms and the other skins' matrices are written all the same. sr_clip_pose_host
 * runs both. */
typedef struct SrNodeTrs { float translation[3], rotation[4], scale[3]; uint32_t animated, reserved; } SrNodeTrs;   /* 48 bytes */
int sr_clip_sample_host(const SrClip* clip, float time_seconds, SrNodeTrs* out);
int sr_clip_compose_host(const SrClip* clip, const SrNodeTrs* trs, const SrTransform* placement, SrTransform* joint_matrices,
                         SrTransform* instance_transforms, uint32_t* singular_skin);
int sr_clip_pose_host(const SrClip* clip, float time_seconds, const SrTransform* placement, SrTransform* joint_matrices,
                      SrTransform* instance_transforms);
/* Clips on a scene. sr_scene_attach_clip uploads the clip's tables once, as one device block, and hands out an id; ids count up
 * and are not handed out again while the scene lives. sr_scene_detach_clip frees the block (it waits for the device).
 * sr_scene_pose_actors is sr_scene_pose_meshes with the joint matrices named rather than given: one kernel in front of the posing
 * kernel (clip_pose_kernel, one block per actor) samples every actor's clip at the actor's own time, composes the hierarchy, and
 * writes the joint matrices where the posing kernel reads them and the instance transforms into d_instance_transforms (DEVICE
 * memory, or NULL: none are written), which sr_scene_set_instances_device takes. Opt-in: nothing selects it.
 * On `stream`: the check words are preset; ONE upload (item rows, block table, active lists, actor rows, instance rows; no joint
 * matrices: the region the clip kernel writes lies outside the uploaded bytes); clip_pose_kernel; the posing kernel; ONE
 * read-back (two words per item, one per actor).
 * Morph weights from the clip: an item whose `morph` is SR_ACTOR_CLIP_WEIGHTS(blas) takes the weights of that morph set of its
 * actor's clip at the actor's time, evaluated on the device: clip_weights_kernel (one wave per such item, launched between the
 * two kernels above and only when an item asks for it) samples the set, leaves out the weights that are +-0 and writes the
 * item's active list (ascending target order) and its count where the posing kernel reads them. The upload then holds one more
 * row of 32 bytes per such item and no weights; each such item has a slot of n_targets entries in the active arrays, outside
 * the uploaded bytes unless the call also has items with host weights; the read-back takes one more word per such item, the
 * count, which SrMeshMorphInfo.n_active reports. The active list is bit equal to the compaction of sr_clip_weights_host.
 * sr_scene_read_item_active reads an item's list back as the posing kernel read it.
 * Numerics: translation, scale and STEP samples, samples at clamped and exact key times and everything composed from a TRS are
 * bit equal to sr_clip_pose_host. An interpolated rotation passes through atan2 and sin, where the device's libm and the host's
 * are not bit-identical: a component is the host's, its neighbouring fp32 value, or within 2^-44 of it. Cubic samples
 * (SR_CLIP_CUBICSPLINE channels and sets) need + - * / and one sqrt only: they are bit equal without exception.
 * Cubic morph sets: an item whose set is SR_CLIP_CUBICSPLINE is a spline row; clip_spline_weights_kernel (one wave per such row)
 * runs behind clip_weights_kernel, which keeps the other rows, and writes what that kernel writes. Both kinds of row travel in
 * the one upload; each kernel is launched only where it has a row. SrSplinePoseInfo counts them.
 * Refused on the host before any device work, behind "pose_actors: actor <i>: " or "pose_actors: item <i>: ": an unknown clip id,
 * a time that is not finite (sr_gltf_pose's words), instance_rows or instance_base without d_instance_transforms, an actor or
 * skin index out of range, a skin whose joint count is not that of the mesh's attached rig, a key named twice, an item with
 * neither stage, and everything sr_scene_pose_meshes refuses for an item; for an item with clip weights: `weights` given as
 * well, an actor out of range, a blas the clip has no set for, an unavailable set (its kept status and the loader's words), a set
 * whose n_targets is not that of the mesh's attached morph, a mesh without a morph. The instance rows are the caller's to keep
 * inside d_instance_transforms.
 * Refused on the device, all or nothing: a singular mesh-node transform (the actor's check word): sr_gltf_pose's status and
 * words for the lowest such actor; no mesh has changed. d_instance_transforms MAY HAVE BEEN WRITTEN by then: do not hand it to
 * sr_scene_set_instances_device after a refusal. A non-finite posed vertex refuses as in sr_scene_pose_meshes. */
typedef struct SrClipActor {           /* one character: a clip at a time. 32 bytes */
    uint32_t clip_id; float time_seconds;
    const SrTransform* placement;      /* host, or NULL; premultiplied onto the instance transforms only */
    const uint32_t* instance_rows;     /* host, the clip's n_instances rows of d_instance_transforms, or NULL: instance_base + i */
    uint32_t instance_base, reserved;
} SrClipActor;
typedef struct SrActorPoseItem {       /* one mesh: what SrPoseItem is, with the joint matrices named rather than given. 32 bytes */
    uint64_t key; uint32_t actor, skin;        /* skin: the file's skin index, or SR_ACTOR_NO_SKIN: no skin stage */
    const float* weights; uint32_t n_targets, morph;      /* morph stage as in SrPoseItem: host weights, or NULL; morph 0, or */
} SrActorPoseItem;                                        /* SR_ACTOR_CLIP_WEIGHTS(blas): the actor's clip gives the weights (weights NULL) */
#define SR_ACTOR_NO_SKIN 0xFFFFFFFFu
#define SR_ACTOR_CLIP_WEIGHTS(blas) ((uint32_t)(blas) + 1u)
#define SR_ACTORS_KEEP_NODES 1u        /* flags: also store every actor's sampled TRS and global matrices (sr_scene_read_actor_nodes) */
typedef struct SrActorPoseInfo {       /* the last sr_scene_pose_actors that reached the device (a host refusal leaves it alone) */
    uint32_t actors, items;
    uint64_t nodes, channels;          /* nodes evaluated, channels sampled, over all actors */
    uint64_t upload_bytes;             /* the one upload */
    uint32_t launches;                 /* 3 accepted (clip, pose, scatter), 2 refused; one more for each weights kernel that ran
                                        * (clip_weights_kernel or the blended one, clip_spline_weights_kernel) */
    uint32_t read_backs;               /* 1 */
    uint32_t calls;                    /* calls that reached the device since the scene was created */
    uint32_t refused_actor, refused_item;      /* 0xFFFFFFFF: none */
    uint32_t weight_items;             /* items whose weights came from their actor's clip, plain and spline rows */
    double clip_ms, pose_ms, scatter_ms;   /* events, only while sr_scene_enable_timing is on; clip_ms: clip_pose_kernel and, where they
                                            * ran, clip_weights_kernel and clip_spline_weights_kernel; pose_ms includes the read-back */
    double host_ms;                    /* the whole call, wall clock */
} SrActorPoseInfo;                     /* 88 bytes */
int sr_scene_attach_clip(SrScene* scene, const SrClip* clip, uint32_t* clip_id);
int sr_scene_detach_clip(SrScene* scene, uint32_t clip_id);
int sr_scene_pose_actors(SrScene* scene, const SrClipActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                         SrTransform* d_instance_transforms, uint32_t flags, void* stream);
int sr_scene_actor_pose_info(const SrScene* scene, SrActorPoseInfo* out);
/* The cubic side of the last sr_scene_pose_actors or sr_scene_pose_actors_blended that reached the device. */
typedef struct SrSplinePoseInfo {
    uint32_t spline_weight_rows;       /* clip-weighted items that clip_spline_weights_kernel evaluated: a cubic set, or for a blended item
                                        * a cubic set in at least one source */
    uint32_t plain_weight_rows;        /* those clip_weights_kernel or clip_blend_weights_kernel evaluated */
    uint64_t cubic_channels;           /* SR_CLIP_CUBICSPLINE channels among SrActorPoseInfo.channels */
    double spline_weights_ms;          /* clip_spline_weights_kernel alone; events, only while sr_scene_enable_timing is on */
    uint64_t reserved;
} SrSplinePoseInfo;                    /* 32 bytes */
int sr_scene_spline_pose_info(const SrScene* scene, SrSplinePoseInfo* out);
/* After a call with SR_ACTORS_KEEP_NODES that reached the device: actor `actor`'s sampled TRS (n_nodes records) and global
 * matrices (n_nodes x 16 floats, row-major), clip-node order. Either may be NULL. SR_ERR_STATE: the last call kept no nodes.
 * sr_scene_read_actor_matrices: after any call that reached the device, the actor's joint matrices as the posing kernel read
 * them (the clip's n_joints, each skin at its sr_clip_skin offset). SR_ERR_STATE: another pose call has used the staging
 * block since. Both wait for the device. */
int sr_scene_read_actor_nodes(const SrScene* scene, uint32_t actor, SrNodeTrs* trs, float* globals16);
int sr_scene_read_actor_matrices(const SrScene* scene, uint32_t actor, SrTransform* joint_matrices);
/* After a sr_scene_pose_actors that reached the device: item `item`'s active list as the posing kernel read it, whether the host
 * or clip_weights_kernel wrote it: *n_active, then that many target indices and weights (room for the mesh's n_targets each;
 * either may be NULL). An item without a morph stage has 0. SR_ERR_STATE under the rule of sr_scene_read_actor_matrices. */
int sr_scene_read_item_active(const SrScene* scene, uint32_t item, uint32_t* index_out, float* weight_out, uint32_t* n_active);
/* Cross-fades: an actor between two baked clips, each at its own time, at the share `weight` of the second.
 * The rule (csrc/clip_rule.h, shared by host and device, + - * / and sqrt in fp64 from the fp32 values, rounded once, no libm): two
 * node records blend into one. weight 0: A's record, whole, its `animated` mask included; weight 1: B's, whole; so a blended call
 * at the end weights is byte-equal to the plain call with that clip. Otherwise the mask is A's | B's; where that is 0 the record
 * is A's and the node keeps composing from the file's matrix; where it is not, each of translation, rotation and scale is taken
 * whole: a part whose bytes are equal in both records is copied (a clip blended with itself at one time is the identity at every
 * weight), otherwise translation and scale are (float)(a + w (b - a)) and the rotation is a normalised lerp along the shorter arc
 * (b negated where dot(a, b) < 0, r = a + w (b - a), normalised). nlerp and not slerp, on purpose: it keeps atan2 and sin out of
 * the stage. A node's local matrix comes from its TRS where the record's mask is not 0, and from the file's matrix otherwise: a
 * node the file gives by `matrix` that only one clip animates therefore jumps between its matrix and the glTF default TRS at the
 * end weights (glTF forbids animating such nodes). Morph weights blend per target in the same form.
 * sr_clip_blend_compatible: SR_OK where the two clips' blocks have equal n_nodes, level table and instance table, per node equal
 * parent, gltf_node, level, file TRS and matrix (the animated masks may differ), and equal skins, joint nodes, joint skins and
 * inverse bind matrices: in practice, bakes of one file. Otherwise SR_ERR_INVALID_ARG, the words naming the first table that
 * differs.
 * sr_clip_blend_host: the record rule over n_nodes records. sr_clip_compose_records_host: sr_clip_compose_host with each node's
 * TRS-or-matrix decision taken from trs[n].animated in place of the clip's own mask (on sr_clip_sample_host's records: the same
 * bytes). sr_clip_pose_blend_host: sample, sample, blend, compose (the clips must be compatible). sr_clip_blend_weights_host: the
 * blended weights of the morph set of `blas`, which both clips must have available, in sr_clip_weights_host's statuses and words.
 * A weight outside [0, 1] or NaN: SR_ERR_INVALID_ARG. */
int sr_clip_blend_compatible(const SrClip* a, const SrClip* b);
int sr_clip_blend_host(const SrNodeTrs* trs_a, const SrNodeTrs* trs_b, uint32_t n_nodes, float weight, SrNodeTrs* out);
int sr_clip_compose_records_host(const SrClip* clip, const SrNodeTrs* trs, const SrTransform* placement, SrTransform* joint_matrices,
                                 SrTransform* instance_transforms, uint32_t* singular_skin);
int sr_clip_pose_blend_host(const SrClip* a, float time_a, const SrClip* b, float time_b, float weight, const SrTransform* placement,
                            SrTransform* joint_matrices, SrTransform* instance_transforms);
int sr_clip_blend_weights_host(const SrClip* a, float time_a, const SrClip* b, float time_b, float weight, uint32_t blas, float* weights_out,
                               uint32_t n_targets);
/* sr_scene_pose_actors_blended is sr_scene_pose_actors for such actors: clip_blend_kernel (one block per actor) stands where
 * clip_pose_kernel stands: it samples both clips, blends the per-node records, composes the hierarchy once and writes the joint
 * matrices and the instance transforms exactly where sr_scene_pose_actors writes them; for an item with SR_ACTOR_CLIP_WEIGHTS,
 * clip_blend_weights_kernel stands where clip_weights_kernel stands and writes the blended weights' active list. Everything else is
 * sr_scene_pose_actors': the one upload (an actor's row is 96 bytes, a clip-weighted item's 48), the launch sequence, the check
 * words, the one read-back, all-or-nothing refusal, SrActorPoseInfo (`channels` counts A's plus B's; sr_scene_actor_pose_info
 * reports the last call of either entry point) and the read-outs (the kept TRS is the blended record).
 * Numerics: each source is sampled under sr_scene_pose_actors' contract against sr_clip_sample_host; the blended records are bit
 * equal to sr_clip_blend_host of the device's own sources, and the globals, joint matrices and instance transforms to
 * sr_clip_compose_records_host of the device's own blended records, without exception. The blended active list is bit equal to
 * the compaction of sr_clip_blend_weights_host.
 * Refused on the host before any device work, behind "pose_actors_blended: actor <i>: " or "pose_actors_blended: item <i>: ":
 * everything sr_scene_pose_actors refuses, for both clips; a weight outside [0, 1] or NaN; clips that are not compatible
 * (sr_clip_blend_compatible's words); for a clip-weighted item, either clip lacking the set, either set unavailable (its kept
 * status and the loader's words), or sets of unequal n_targets. Refused on the device as sr_scene_pose_actors refuses.
 * SR_ACTORS_KEEP_SOURCES: also store both sources' sampled TRS per actor; sr_scene_read_actor_sources reads them (n_nodes records
 * each, either may be NULL; SR_ERR_STATE: the last call kept none). */
typedef struct SrClipBlendActor {      /* one character between two clips. 48 bytes */
    uint32_t clip_id; float time_seconds;          /* source A */
    uint32_t clip_id_b; float time_seconds_b;      /* source B */
    float weight; uint32_t reserved;               /* the share of B, in [0, 1] */
    const SrTransform* placement;      /* as SrClipActor's */
    const uint32_t* instance_rows;
    uint32_t instance_base, reserved2;
} SrClipBlendActor;
#define SR_ACTORS_KEEP_SOURCES 2u      /* flags of sr_scene_pose_actors_blended: also store both sources' sampled TRS per actor */
int sr_scene_pose_actors_blended(SrScene* scene, const SrClipBlendActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                 SrTransform* d_instance_transforms, uint32_t flags, void* stream);
int sr_scene_read_actor_sources(const SrScene* scene, uint32_t actor, SrNodeTrs* trs_a, SrNodeTrs* trs_b);
/* Layers: an actor as a stack of 1..SR_CLIP_MAX_LAYERS layers over compatible clips (sr_clip_blend_compatible with layer 0's),
 * applied in order onto one accumulated record per node: a walk on the legs while the arms wave (an override layer under a node
 * mask), a breathing or hit-reaction clip added on top of whatever plays (an additive layer), more than two sources at once.
 * The rule (csrc/clip_rule.h, shared by host and device; + - * / and sqrt in fp64 from the fp32 values, rounded once per part, no
 * libm, so host and device agree bit for bit without exception):
 *   Node n of layer l has the effective weight w = (double)weight_l * (double)mask_l[n] (exact); mask_l[n] is 1 without a mask.
 *   Layer 0 is the base: its sampled records are the accumulator. It must be SR_LAYER_OVERRIDE, without a mask, at weight 1.
 *   SR_LAYER_OVERRIDE: acc[n] = the cross-fade rule above (sr_clip_blend_host's) of acc[n] and cur[n] at w; cur is the layer's
 *   clip sampled at time_seconds.
 *   SR_LAYER_ADDITIVE: with ref the same clip sampled at ref_time_seconds: where w == 0 or the clip does not animate the node,
 *   acc[n] stays, whole. Otherwise each of translation, rotation and scale is taken whole; a part whose bytes are equal in cur
 *   and ref is copied from acc (an additive layer at its own reference time is the identity at every weight); translation and
 *   scale are (float)(acc + w (cur - ref)) per component (a sum for scale too, on purpose: no division); the rotation is
 *   acc (x) e normalised, with d = conj(ref) (x) cur negated where d.w < 0 and e = (w d.x, w d.y, w d.z, 1 + w (d.w - 1))
 *   normalised, (x) the Hamilton product with each component's four terms summed left to right. The record's mask becomes
 *   acc's | cur's | ref's.
 * Morph weights: without SR_ACTORS_LAYER_WEIGHTS they are not layered: an item with SR_ACTOR_CLIP_WEIGHTS(blas) takes its weights
 * from the base layer's clip at the base layer's time, by clip_weights_kernel / clip_spline_weights_kernel as in
 * sr_scene_pose_actors. With the flag they go through the stack (see SR_ACTORS_LAYER_WEIGHTS below).
 * Node masks: sr_scene_attach_node_mask uploads one float per clip node, in clip-node order, each in [0, 1] (anything else, a
 * NaN included: SR_ERR_INVALID_ARG), once, and hands out an id; sr_scene_detach_node_mask frees it (it waits for the device). A
 * mask belongs to no clip: its length is checked against the clip's n_nodes where a layer names it. sr_clip_subtree_mask fills
 * `out` (n_nodes floats, the clip's n_nodes) with `inside` for the clip node of glTF node `gltf_node` and everything below it in
 * the clip's parent table and `outside` elsewhere; a node the clip does not hold: SR_ERR_INVALID_ARG.
 * sr_clip_layers_host: the record rule over caller-given sampled records: cur[l] and ref[l] are n_nodes records each (ref[l] is
 * read for additive layers only and may be NULL otherwise; `ref` itself may be NULL where no layer is additive). It refuses
 * n_layers 0 or above SR_CLIP_MAX_LAYERS, a weight or a mask value outside [0, 1] or NaN, an unknown mode, an additive layer
 * without ref, and a base layer that is additive, masked or not at weight 1.
 * sr_clip_pose_layers_host: sample, stack, compose: clips[l] is layer l's clip; masks[l] its host mask or NULL (`masks` may be
 * NULL); clip_id and mask_id of the layers are not read. It refuses what sr_clip_layers_host refuses, a time that is not finite
 * (time_seconds, and ref_time_seconds of an additive layer; unless the clip is the static pose) and a clip that is not compatible
 * with clips[0]. One layer: sr_clip_pose_host's bytes; two unmasked override layers: sr_clip_pose_blend_host's.
 * sr_scene_pose_actors_layered is sr_scene_pose_actors for such actors: clip_layers_kernel (one block per actor) stands where
 * clip_pose_kernel stands: it samples the layers in order, applies the rule, composes the hierarchy once and writes the joint
 * matrices and the instance transforms exactly where sr_scene_pose_actors writes them. Everything else is sr_scene_pose_actors':
 * the one upload (an actor's row is 80 bytes; the layers travel as a table of their own, 32 bytes a layer, in the same upload, and 64 bytes more
 * tell the kernel where its results go), the
 * launch sequence (3 launches accepted), the check words, the one read-back, all-or-nothing refusal, SrActorPoseInfo (`channels`
 * counts every sample taken, so an additive layer's clip counts twice) and the read-outs (the kept TRS is the final record).
 * Numerics: each sampled source is under sr_scene_pose_actors' contract against sr_clip_sample_host; the final records are bit
 * equal to sr_clip_layers_host of the device's own sources, and everything composed to sr_clip_compose_records_host of the
 * device's own records, without exception.
 * Refused on the host before any device work, behind "pose_actors_layered: actor <i>: layer <l>: " ("actor <i>: " for what is the
 * actor's, "item <i>: " for items); the scene is unchanged: everything sr_scene_pose_actors refuses, for every layer's clip;
 * n_layers 0 or above SR_CLIP_MAX_LAYERS; a clip not compatible with layer 0's (sr_clip_blend_compatible's words); a weight
 * outside [0, 1] or NaN; an unknown mode; an unknown mask id, or a mask whose length is not the clip's n_nodes; a time_seconds, or
 * an additive layer's ref_time_seconds, that is not finite; a base layer that is additive, masked or not at weight 1.
 * SR_ACTORS_KEEP_LAYERS: also store every layer's sampled `cur`, and `ref` for additive layers; sr_scene_read_actor_layer reads
 * them (n_nodes records each, either may be NULL; `ref` of an override layer is left alone; SR_ERR_STATE: the last call kept
 * none). */
#define SR_CLIP_MAX_LAYERS 8u
#define SR_LAYER_OVERRIDE 0u
#define SR_LAYER_ADDITIVE 1u
#define SR_LAYER_NO_MASK 0xFFFFFFFFu
typedef struct SrClipLayer {           /* one layer of an actor. 32 bytes */
    uint32_t clip_id; float time_seconds;
    float weight; uint32_t mode;       /* weight in [0, 1]; SR_LAYER_OVERRIDE or SR_LAYER_ADDITIVE */
    uint32_t mask_id;                  /* sr_scene_attach_node_mask's, or SR_LAYER_NO_MASK */
    float ref_time_seconds;            /* SR_LAYER_ADDITIVE: the clip's reference time */
    uint32_t reserved[2];
} SrClipLayer;
typedef struct SrClipLayerActor {      /* one character as a stack of layers. 40 bytes */
    const SrClipLayer* layers;         /* host, n_layers of them; layers[0] is the base */
    uint32_t n_layers, instance_base;  /* instance_base as SrClipActor's */
    const SrTransform* placement;      /* as SrClipActor's */
    const uint32_t* instance_rows;     /* as SrClipActor's, with the base clip's n_instances */
    uint64_t reserved;
} SrClipLayerActor;
typedef struct SrClipLayerRule {       /* one layer of sr_clip_layers_host. 16 bytes */
    float weight; uint32_t mode;
    const float* mask;                 /* host, n_nodes floats in [0, 1], or NULL */
} SrClipLayerRule;
typedef struct SrLayerPoseInfo {       /* the last sr_scene_pose_actors_layered that reached the device. 32 bytes */
    uint32_t layers, additive_layers, masked_layers;   /* over all actors; the base layers are among `layers` */
    uint32_t max_layers;               /* the tallest stack of the call */
    uint64_t layer_table_bytes;        /* the layer table's share of SrActorPoseInfo.upload_bytes */
    uint64_t reserved;
} SrLayerPoseInfo;
#define SR_ACTORS_KEEP_LAYERS 4u       /* flags of sr_scene_pose_actors_layered: also store every layer's sampled records */
int sr_clip_subtree_mask(const SrClip* clip, uint32_t gltf_node, float inside, float outside, float* out, uint32_t n_nodes);
int sr_clip_layers_host(const SrNodeTrs* const* cur, const SrNodeTrs* const* ref, const SrClipLayerRule* rule, uint32_t n_layers, uint32_t n_nodes,
                        SrNodeTrs* out);
int sr_clip_pose_layers_host(const SrClip* const* clips, const SrClipLayer* layers, const float* const* masks, uint32_t n_layers,
                             const SrTransform* placement, SrTransform* joint_matrices, SrTransform* instance_transforms);
int sr_scene_attach_node_mask(SrScene* scene, const float* weights, uint32_t n_nodes, uint32_t* mask_id);
int sr_scene_detach_node_mask(SrScene* scene, uint32_t mask_id);
int sr_scene_pose_actors_layered(SrScene* scene, const SrClipLayerActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                                 SrTransform* d_instance_transforms, uint32_t flags, void* stream);
int sr_scene_layer_pose_info(const SrScene* scene, SrLayerPoseInfo* out);
int sr_scene_read_actor_layer(const SrScene* scene, uint32_t actor, uint32_t layer, SrNodeTrs* cur, SrNodeTrs* ref);
/* Layered morph weights. SR_ACTORS_LAYER_WEIGHTS is a flag of sr_scene_pose_actors_layered and sr_renderer_pose_actors_layered
 * only (the plain and blended calls refuse the bit). With it every item whose `morph` is SR_ACTOR_CLIP_WEIGHTS(blas) takes the
 * stack's weights for that blas: a blink, a breath or a viseme clip as an additive layer over whatever the body plays. Without it
 * the call is byte for byte what it was: same rows, same kernels, same launch count, same info.
 * The rule (csrc/clip_rule.h, shared by host and device, no libm), per morph set (per blas) and per target k, on fp32 weights, in
 * fp64 in exactly this grouping, each layer's result rounded to fp32 once:
 *   cur_l[k] is layer l's clip's set for the blas sampled at time_seconds as sr_clip_weights_host samples it (LINEAR, STEP,
 *   CUBICSPLINE, or the defaults where the set has no keys); an additive layer also has ref_l[k], sampled at ref_time_seconds.
 *   w_l = (double)weight_l * (double)m (exact), m the layer's mask value at the clip node whose gltf_node is the set's gltf_node;
 *   m is 1 where the layer has no mask or the clip holds no such node.
 *   acc = cur_0. SR_LAYER_OVERRIDE: acc[k] = the cross-fade rule of sr_clip_blend_weights_host of acc[k] and cur_l[k] at w_l.
 *   SR_LAYER_ADDITIVE: acc[k] stays where w_l == 0 or cur_l[k] and ref_l[k] are the same word (an additive layer at its own
 *   reference time is the identity at every weight); otherwise (float)(acc[k] + w_l (cur_l[k] - ref_l[k])).
 *   After the last layer the targets whose weight is +0 or -0 are left out, the rest kept in ascending target order.
 * sr_clip_layer_weights_host: the rule over caller-given weight vectors: cur[l] and ref[l] are n_targets floats each (ref[l] is
 * read for additive layers only and may be NULL otherwise; `ref` itself may be NULL where no layer is additive); weight, mode and
 * mask_value are arrays of n_layers; mask_value may be NULL: all 1. It refuses what sr_clip_layers_host refuses, with "mask value"
 * for a mask: a mask value outside [0, 1] or NaN, and a base layer whose mask value is not 1.
 * sr_clip_weights_layers_host: sample, resolve each mask's node, stack: clips, layers and masks as sr_clip_pose_layers_host takes
 * them. A clip without a set for the blas, an unavailable set and a wrong n_targets are refused in sr_clip_weights_host's statuses
 * and words behind "layer <l>: "; so are a clip not compatible with clips[0] and sets of unequal n_targets across the layers. One
 * layer: sr_clip_weights_host's bytes; two unmasked override layers: sr_clip_blend_weights_host's.
 * On the device clip_layer_weights_kernel (one wave per item, one launch per call, behind clip_layers_kernel and in front of the
 * posing kernel) stands where clip_weights_kernel and clip_spline_weights_kernel stand: a row of 32 bytes per item and an entry of
 * 16 bytes per item and layer travel in the one upload. SrActorPoseInfo.weight_items counts the rows, `launches` is 4 for an
 * accepted call with a row, and SrSplinePoseInfo reports 0 plain and 0 spline rows, since neither older kernel ran. The active
 * lists are bit equal to the compaction of sr_clip_weights_layers_host, without exception; sr_scene_read_item_active reads them.
 * Refused on the host before any device work, behind "pose_actors_layered: item <i>: layer <l>: ": a layer's clip without a set
 * for the blas, or with the set unavailable (its kept status and the loader's words); the base layer's set ("layer 0: ") whose
 * n_targets is not the mesh's attached morph's; a layer's set whose n_targets is not the base layer's. A layer at weight 0 is
 * checked like any other (the kernel does not sample it). A mesh without a morph is refused in sr_scene_pose_actors' words.
 * SrLayerWeightsInfo: the figures of the last layered call that reached the device (all 0 where it had no flag or no such item). */
#define SR_ACTORS_LAYER_WEIGHTS 8u     /* flags of sr_scene_pose_actors_layered: clip-weighted items take the stack's weights */
typedef struct SrLayerWeightsInfo {    /* 32 bytes */
    uint32_t rows;                     /* items posed with the stack's weights */
    uint32_t samples, cubic_samples;   /* set samples taken (an additive layer counts twice); those of CUBICSPLINE sets */
    uint32_t reserved;
    uint64_t table_bytes;              /* the rows' and entries' share of SrActorPoseInfo.upload_bytes */
    double weights_ms;                 /* clip_layer_weights_kernel, from events; 0 unless sr_scene_enable_timing is on */
} SrLayerWeightsInfo;
int sr_clip_layer_weights_host(const float* const* cur, const float* const* ref, const float* weight, const uint32_t* mode, const float* mask_value,
                               uint32_t n_layers, uint32_t n_targets, float* out);
int sr_clip_weights_layers_host(const SrClip* const* clips, const SrClipLayer* layers, const float* const* masks, uint32_t n_layers, uint32_t blas,
                                float* weights_out, uint32_t n_targets);
int sr_scene_layer_weights_info(const SrScene* scene, SrLayerWeightsInfo* out);

/* What Renderer::load_gltf / load_scene return (lib.rs:779-846): the asset group and the scene's instances
 * grouped per BLAS key in BLAS order. Keys are ResourceKey{group, index} packed as group << 32 | index
 * (lib.rs:54-58); BLASes take indices 0..n-1, images the following ones (resource_manager.rs:400-410). */
typedef struct SrLoadedScene SrLoadedScene;
int sr_renderer_load_gltf(SrRenderer* renderer, const char* path, SrLoadedScene** out);
int sr_renderer_load_scene(SrRenderer* renderer, const SrGltf* gltf, SrLoadedScene** out);
int sr_loaded_scene_get(const SrLoadedScene* loaded, uint64_t* group, const uint64_t** keys, const uint32_t** counts,
                        uint32_t* n_keys, const SrTransform** transforms, uint32_t* n_transforms);
int sr_loaded_scene_destroy(SrLoadedScene* loaded);
/* Renderer::unload_scene (lib.rs:849-857) / unload_mesh (lib.rs:965-973). */
int sr_renderer_unload_scene(SrRenderer* renderer, uint64_t group);
int sr_renderer_unload_mesh(SrRenderer* renderer, uint64_t key);
/* sr_scene_update_mesh on every device slot's scene; the next sr_renderer_render re-submits its instance list, which applies
 * the update. Each scene waits for its device, so frames in flight have finished reading the old vertices before they change. */
int sr_renderer_update_mesh(SrRenderer* renderer, uint64_t key, const SrVertex* vertices, uint32_t n_vertices);
/* sr_scene_update_mesh_device through the facade: `d_vertices` lives on the first device slot's GPU and is validated once,
 * there; every further slot's replica takes the vertices by a device-to-device (peer) copy into its own allocation and ends in
 * the same state. A refusal changes no replica. */
int sr_renderer_update_mesh_device(SrRenderer* renderer, uint64_t key, const SrVertex* d_vertices, uint32_t n_vertices, void* stream);
/* sr_scene_set_mesh_skin / sr_scene_skin_mesh through the facade: the rig is attached on the first device slot's scene only and
 * the mesh is posed there, once; every further slot's replica takes the validated posed vertices from that scene's batch
 * scratch by a device-to-device (peer) copy, as with sr_renderer_pose_meshes. A refusal changes no replica. */
int sr_renderer_set_mesh_skin(SrRenderer* renderer, uint64_t key, const SrSkinInfluence* influences, uint32_t n_vertices, uint32_t n_joints);
int sr_renderer_skin_mesh(SrRenderer* renderer, uint64_t key, const SrTransform* joint_matrices, uint32_t n_joints, void* stream);
/* Attaches the rig of every skinned blas of a loaded scene (sr_gltf_blas_skin, sr_gltf_skin -> sr_renderer_set_mesh_skin) and
 * declares those meshes SR_BUILD_RAPIDLY_CHANGING. `gltf` is the file `loaded` was loaded from. sr_renderer_load_scene itself
 * attaches nothing. */
int sr_renderer_attach_skins(SrRenderer* renderer, const SrGltf* gltf, const SrLoadedScene* loaded);
/* One frame of an animation for a loaded scene: for every skinned blas the joint matrices of sr_gltf_pose and
 * sr_renderer_skin_mesh, then the posed instance transforms into instance_transforms_out (the order and count of
 * sr_loaded_scene_get's transforms; may be NULL) for the caller's next sr_renderer_render. */
int sr_renderer_pose_scene(SrRenderer* renderer, const SrGltf* gltf, const SrLoadedScene* loaded, int32_t animation, float time_seconds,
                           SrTransform* instance_transforms_out, void* stream);
/* sr_scene_set_mesh_morph / sr_scene_pose_mesh through the facade, as the skin calls above: the morph is attached on the first
 * device slot's scene only and the mesh is posed there, once (morph, then skin where joint matrices are given); every further
 * slot's replica takes the validated posed vertices from that scene's batch scratch by a device-to-device (peer) copy. A refusal
 * changes no replica. */
int sr_renderer_set_mesh_morph(SrRenderer* renderer, uint64_t key, const SrMorphDelta* deltas, uint32_t n_vertices, uint32_t n_targets);
int sr_renderer_pose_mesh(SrRenderer* renderer, uint64_t key, const float* weights, uint32_t n_targets, const SrTransform* joint_matrices,
                          uint32_t n_joints, void* stream);
/* Attaches the morph targets of every blas of a loaded scene that has some (sr_gltf_blas_morph -> sr_renderer_set_mesh_morph) and
 * declares those meshes SR_BUILD_RAPIDLY_CHANGING. From then on sr_renderer_pose_scene poses them too: the weights of
 * sr_gltf_morph_weights into sr_renderer_pose_mesh, with the joint matrices where the mesh is skinned as well. A scene on which
 * this was never called is posed by sr_renderer_pose_scene as before. Call it, like sr_renderer_attach_skins, while the meshes
 * hold the vertices they were loaded with. */
int sr_renderer_attach_morphs(SrRenderer* renderer, const SrGltf* gltf, const SrLoadedScene* loaded);
/* sr_scene_pose_meshes through the facade: the first device slot's scene poses and validates the whole batch once; every further
 * slot's replica takes each item's posed records from that scene's batch scratch by a device-to-device (peer) copy, mesh by mesh.
 * A refusal changes no replica. */
int sr_renderer_pose_meshes(SrRenderer* renderer, const SrPoseItem* items, uint32_t n_items, void* stream);
/* sr_scene_attach_clip / sr_scene_detach_clip / sr_scene_pose_actors / sr_scene_actor_pose_info through the facade. The clip is
 * attached to the first device slot's scene, which suffices: that scene poses and validates once, and every further slot's
 * replica takes each item's posed records from its batch scratch, as with sr_renderer_pose_meshes. d_instance_transforms lives
 * on the first slot's device; sr_renderer_render_device_transforms takes it from there. A refusal changes no replica. */
int sr_renderer_attach_clip(SrRenderer* renderer, const SrClip* clip, uint32_t* clip_id);
int sr_renderer_detach_clip(SrRenderer* renderer, uint32_t clip_id);
int sr_renderer_pose_actors(SrRenderer* renderer, const SrClipActor* actors, uint32_t n_actors, const SrActorPoseItem* items, uint32_t n_items,
                            SrTransform* d_instance_transforms, uint32_t flags, void* stream);
/* sr_scene_pose_actors_blended through the facade, by the same per-slot path as sr_renderer_pose_actors. */
int sr_renderer_pose_actors_blended(SrRenderer* renderer, const SrClipBlendActor* actors, uint32_t n_actors, const SrActorPoseItem* items,
                                    uint32_t n_items, SrTransform* d_instance_transforms, uint32_t flags, void* stream);
/* sr_scene_attach_node_mask / sr_scene_detach_node_mask / sr_scene_pose_actors_layered through the facade: the masks live on the
 * first device slot's scene, as the clips do, and the call takes the same per-slot path as sr_renderer_pose_actors. */
int sr_renderer_attach_node_mask(SrRenderer* renderer, const float* weights, uint32_t n_nodes, uint32_t* mask_id);
int sr_renderer_detach_node_mask(SrRenderer* renderer, uint32_t mask_id);
int sr_renderer_pose_actors_layered(SrRenderer* renderer, const SrClipLayerActor* actors, uint32_t n_actors, const SrActorPoseItem* items,
                                    uint32_t n_items, SrTransform* d_instance_transforms, uint32_t flags, void* stream);
int sr_renderer_actor_pose_info(const SrRenderer* renderer, SrActorPoseInfo* out);
int sr_renderer_layer_weights_info(const SrRenderer* renderer, SrLayerWeightsInfo* out);
int sr_renderer_spline_pose_info(const SrRenderer* renderer, SrSplinePoseInfo* out);
/* How sr_renderer_pose_scene poses a loaded scene's rigged and morphed meshes: SR_POSE_BATCH_OFF (the default), one
 * sr_renderer_skin_mesh / sr_renderer_pose_mesh per mesh (each a batch of one item); SR_POSE_BATCH_ON, all of them by one sr_renderer_pose_meshes.
 * SR_POSE_BATCH=on|off in the environment sets the initial mode when the renderer is created. */
#define SR_POSE_BATCH_OFF 0u
#define SR_POSE_BATCH_ON 1u
int sr_renderer_set_pose_batch(SrRenderer* renderer, uint32_t mode);
/* sr_scene_set_mesh_frame / sr_scene_update_mesh_positions_device / sr_scene_update_mesh_positions through the facade, as the
 * skin calls above: the frame is attached on the first device slot's scene only and the records are produced there, once
 * (`d_positions` lives on that slot's GPU); every further slot's replica takes the validated records by a device-to-device (peer)
 * copy. A refusal changes no replica. */
int sr_renderer_set_mesh_frame(SrRenderer* renderer, uint64_t key, uint32_t flags);
int sr_renderer_update_mesh_positions_device(SrRenderer* renderer, uint64_t key, const float* d_positions, uint32_t n_vertices, void* stream);
int sr_renderer_update_mesh_positions(SrRenderer* renderer, uint64_t key, const float* positions, uint32_t n_vertices, void* stream);
/* sr_scene_set_mesh_build_type on every device slot's scene. */
int sr_renderer_set_mesh_build_type(SrRenderer* renderer, uint64_t key, uint32_t build_type);
/* sr_scene_set_mesh_tree_build on every device slot's scene. */
int sr_renderer_set_mesh_tree_build(SrRenderer* renderer, uint32_t mode);
/* sr_scene_set_mesh_tree_batch on every device slot's scene. */
int sr_renderer_set_mesh_tree_batch(SrRenderer* renderer, uint32_t mode);
/* sr_scene_set_tree_height_bound on every device slot's scene. */
int sr_renderer_set_tree_height_bound(SrRenderer* renderer, uint32_t mode, uint32_t mesh_tree_cap);
/* sr_scene_set_light_table_build on every device slot's scene, and sr_scene_light_table_info of one slot's scene. */
int sr_renderer_set_light_table_build(SrRenderer* renderer, uint32_t mode);
int sr_renderer_light_table_info(SrRenderer* renderer, uint32_t slot, SrLightTableInfo* out);

/* Harness access: inner scene (counters, stats), device pointers of the RGBA8 output and the fp32 radiance OF THE LAST
 * SUBMITTED FRAME (valid after sr_renderer_wait_frame of that frame), and relative_frame_count. Any out pointer may be NULL.
 * Meshes of a renderer are updated through sr_renderer_update_mesh: after sr_scene_update_mesh on the inner scene the renderer
 * does not know that its instance list must be re-submitted, and sr_renderer_render with an unchanged list returns SR_ERR_STATE
 * (from sr_scene_end_frame). */
int sr_renderer_get(SrRenderer* renderer, SrScene** scene, const uint32_t** output_rgba8_device,
                    const float** raw_color_device, uint32_t* relative_frame_count);
/* Stand-in for the reference's embedded 128x128 blue-noise PNG (lib.rs:281-309; an input asset, not
 * copied): hashed white noise, RGBA8, grey in rgb, alpha 255. Host pointer, w*h*4 bytes. */
int sr_default_noise_texture(uint32_t w, uint32_t h, uint32_t seed, uint8_t* out_rgba8);
/* Replaces the noise texture of the passes (lib.rs:281-309 builds it once, in Renderer::new, from the PNG embedded in the crate: a host
 * that owns that asset decodes it with sr_decode_image_rgba8 and hands it over here). RGBA8 texels in host memory, w * h * 4 bytes.
 * Waits for the frames in flight; the temporal history is kept. */
int sr_renderer_set_blue_noise(SrRenderer* r, const uint8_t* rgba8, uint32_t w, uint32_t h);

/* Measured cost of the last launch of pass `which` (0 = raytracing_ris, 1 = raytracing_final) with this launch
 * geometry, summed per tile row (8 pixel rows), in shader cycles: the data the library's own tile schedule uses.
 * A tile-parallel host cuts its strips of equal cost from it (sunray_amd/distributed.py). out: cap doubles. */
int sr_scene_read_tile_row_costs(SrScene* scene, int which, uint32_t width, uint32_t y0, uint32_t rows, double* out,
                                 uint32_t cap, uint32_t* n_tile_rows);

/* The same measurement per tile (8x8 pixels), row-major (tile row * tiles per row + tile column): tuning diagnostics. */
int sr_scene_read_tile_costs(SrScene* scene, int which, uint32_t width, uint32_t y0, uint32_t rows, uint32_t* out,
                             uint32_t cap, uint32_t* n_tiles);

/* Test hook: puts a cost map of the caller's in place of the measured one of pass `which` and the launch rectangle of `width`
 * columns from x0 and `rows` rows from y0 (what the passes clip tile_* of SrRtParams to), and derives the tile schedule from it,
 * so that the next launch of that pass with that rectangle runs in the order these costs give. costs: n host values, one per
 * 8x8 tile, row-major as above; n must be the rectangle's tile count. Needs no frame and no earlier launch (the schedule entry
 * is created as a launch would create it); does not count as a launch for the cadence at which launches re-derive the order.
 * Waits for the device. */
int sr_scene_set_tile_costs(SrScene* scene, int which, uint32_t x0, uint32_t width, uint32_t y0, uint32_t rows,
                            const uint32_t* costs, uint32_t n);
/* Test hook: the tile order the next launch of pass `which` with that rectangle would run in: 8 lists (one per XCD, i.e. per
 * column band) of *order_cap entries each, absolute tile indices (tile row * tiles per row + tile column), 0xFFFFFFFF after a
 * list's last tile. out: cap values, at least 8 * *order_cap (*order_cap is set before that is checked). SR_ERR_STATE while no
 * order has been derived for that geometry (no launch, no sr_scene_set_tile_costs). Waits for the device. */
int sr_scene_read_tile_order(SrScene* scene, int which, uint32_t x0, uint32_t width, uint32_t y0, uint32_t rows, uint32_t* out,
                             uint32_t cap, uint32_t* order_cap);
/* Test hook: the largest light table (emissive triangles of the instance list) that a wave of the RIS pass keeps in its LDS while
 * it draws its candidates; a longer table is read from global memory, with the same results. It follows from the LDS a launch of
 * this scene's passes takes (traversal stack of the built structure), so it can change with sr_scene_set_instances; 0 when the
 * scene never stages (SR_LIGHT_STAGE=0 in the environment at sr_scene_create). */
int sr_scene_light_stage_capacity(const SrScene* scene, uint32_t* lights);

/* ------------------------------------------------------------------------------------------ */
/* Tile-parallel rendering across the GPUs of a node                               */
/* ------------------------------------------------------------------------------------------ */
/* The reference renders on one device (src/lib.rs:1166). A multi-GPU host creates one scene / renderer context per GPU
 * (scene replicated), cuts the frame into `world` contiguous strips and has every context trace its strip into full-size
 * buffers; pixels are keyed by global coordinates (tile_* of SrRtParams), so the strips of N contexts are the single-GPU
 * frame bit for bit. ReSTIR's spatial reuse reads a 30-pixel neighbourhood (ray_gen_final.slang:160-188,228-247): the RIS
 * pass of a strip also covers a 30-pixel halo on either side (recomputed, rays counted for the strip only). Temporal reuse
 * under camera motion needs the reservoir bands sr_history_exchange_plan lists, from the ranks that own them. The only
 * data-path collective is the gather of the radiance strips, which stays with the caller (RCCL: ncclAllGather over the
 * per-rank raw_color strips). Everything here is deterministic host arithmetic: every rank derives the
 * same partition and plans from the same inputs. */
#define SR_AXIS_COLS 0u      /* column strips (default: image cost varies mostly with the row, columns hand every GPU the same mix) */
#define SR_AXIS_ROWS 1u
#define SR_SPATIAL_HALO 30u  /* SPATIAL_RADIUS (ray_gen_final.slang:161) >= GI_SPATIAL_RADIUS (:229) */
typedef struct SrPartition SrPartition;
/* `bounds`: world + 1 increasing cut positions along the axis from 0 to its length (e.g. from sr_balanced_bounds), or NULL for
 * equal strips. A partition must stay the same for a whole frame sequence: a rank owns the temporal history of its strip + halo. */
int sr_partition_create(uint32_t width, uint32_t height, uint32_t world, uint32_t axis, const uint32_t* bounds, SrPartition** out);
int sr_partition_destroy(SrPartition* partition);
int sr_partition_get(const SrPartition* partition, uint32_t* width, uint32_t* height, uint32_t* world, uint32_t* axis, const uint32_t** bounds);
/* (start, size) along the axis of rank's strip grown by `grow` positions on both sides, clipped to the image. */
int sr_partition_span(const SrPartition* partition, uint32_t rank, uint32_t grow, uint32_t* start, uint32_t* size);
/* Cuts a per-position cost profile into `world` strips of (nearly) equal summed cost, each at least min_size positions and at
 * most max_share * length / world (the gather pads strips to the largest): bounds_out receives world + 1 cuts. */
int sr_balanced_bounds(const double* cost, uint32_t length, uint32_t world, uint32_t min_size, double max_share, uint32_t* bounds_out);
/* Per-column / per-row cost profile (length entries) from per-tile costs (sr_scene_read_tile_costs, tiles_y x tiles_x, 8x8 pixels). */
int sr_axis_cost_from_tiles(const double* tile_costs, uint32_t tiles_x, uint32_t tiles_y, uint32_t axis, uint32_t length, double* out);
/* One point-to-point transfer of the temporal-history exchange: positions [start, start + size) along the axis, full extent
 * across it, of BOTH current reservoir buffers (reservoirs[frame_count & 1], reservoirs_gi[frame_count & 1]), src -> dst. */
typedef struct SrStripTransfer {
    uint32_t src, dst, start, size;
} SrStripTransfer;
/* The transfers needed after every RIS pass when temporal reprojection can move a pixel by up to motion_halo positions along
 * the axis between frames (0 = static camera: none). Writes at most cap entries, returns the total through *count. */
int sr_history_exchange_plan(const SrPartition* partition, uint32_t motion_halo, SrStripTransfer* out, uint32_t cap, uint32_t* count);
/* Launch rectangles of rank's share of a frame: what sr_strip_trace_ris / sr_strip_trace_final put into SrRtParams.tile_* and
 * SrTraceConfig.count_* (count_window == 0: no counting window, every traced pixel counts). */
typedef struct SrStripRects {
    uint32_t ris_y0, ris_h, ris_x0, ris_w;          /* raytracing_ris: strip + spatial halo (world > 1) */
    uint32_t final_y0, final_h, final_x0, final_w;  /* raytracing_final: the strip */
    uint32_t count_y0, count_rows, count_x0, count_cols;
    uint32_t count_window;
    uint32_t empty;                                 /* the rank's strip has no pixels: nothing to launch */
} SrStripRects;
int sr_strip_rects(const SrPartition* partition, uint32_t rank, SrStripRects* out);
/* sr_trace_ris / sr_trace_final of rank's share: `params` describes the whole frame on this rank's device (full-size buffers);
 * its tile_* and config.count_* fields are replaced. Same stream rules as sr_trace_*; between the two calls the host performs
 * the transfers of sr_history_exchange_plan (if any) on the same stream. */
int sr_strip_trace_ris(const SrRtParams* params, const SrPartition* partition, uint32_t rank, void* stream);
int sr_strip_trace_final(const SrRtParams* params, const SrPartition* partition, uint32_t rank, void* stream);

/* Strip movement on its own: what a multi-device caller outside the Renderer uses to move the rectangles of sr_strip_rects and
 * sr_history_exchange_plan between devices, and to check the exactness of its own history exchange. Device pointers and a
 * stream, like sr_post_*; every call launches on the current device. One per-pixel plane of a full-size image: */
typedef struct SrStripPlane {
    void* img;      /* width * height * bpp bytes, 16-byte aligned */
    uint32_t bpp;   /* bytes per pixel: non-zero and even */
    uint32_t _pad;
} SrStripPlane;
#define SR_STRIP_MAX_PLANES 5u
/* Packed form of a w x h rectangle of n_planes planes: plane after plane, rows in order within a plane, every plane's block
 * padded to 16 bytes. *bytes receives its size (only bpp of every plane is read). */
int sr_strip_packed_bytes(const SrStripPlane* planes, uint32_t n_planes, uint32_t w, uint32_t h, uint64_t* bytes);
/* Rectangle [x0, x0 + w) x [y0, y0 + h) of images width x height pixels -> `packed` (sr_strip_packed_bytes bytes, 16-byte
 * aligned; the padding keeps its bytes), and back: unpack writes the rectangle and nothing else. One launch each. Refused with
 * SR_ERR_INVALID_ARG, nothing launched: n_planes outside 1..SR_STRIP_MAX_PLANES, a bpp that is zero or odd, a null pointer, a
 * rectangle that leaves the image, an image or packed pointer that is not 16-byte aligned. w == 0 or h == 0 is a no-op. */
int sr_strip_pack(const SrStripPlane* planes, uint32_t n_planes, uint32_t width, uint32_t height, uint32_t x0, uint32_t w,
                  uint32_t y0, uint32_t h, void* packed, void* stream);
int sr_strip_unpack(const SrStripPlane* planes, uint32_t n_planes, uint32_t width, uint32_t height, uint32_t x0, uint32_t w,
                    uint32_t y0, uint32_t h, const void* packed, void* stream);
/* After a RIS pass over [x0, x0 + w) x [y0, y0 + h): ADDS to *counter (device) the pixels whose temporal-history read, bounded
 * from the stored motion vector (motion_vec_img, R16G16_SFLOAT), may lie outside [held_lo, held_hi) along `axis`. It may
 * over-report near an edge of the held region and never misses. Refused as above; also held_lo > held_hi or
 * held_hi beyond the axis length, and an axis that is neither SR_AXIS_COLS nor SR_AXIS_ROWS. */
int sr_history_reach_check(const uint32_t* motion_vec_img, uint32_t width, uint32_t height, uint32_t axis, uint32_t x0, uint32_t w,
                           uint32_t y0, uint32_t h, uint32_t held_lo, uint32_t held_hi, uint64_t* counter, void* stream);

/* Ray counters since the last reset (device-side atomics, read back synchronously). */
int sr_scene_reset_counters(SrScene* scene, void* stream);
int sr_scene_read_counters(SrScene* scene, void* stream, SrRayCounters* out);

/* Instrumented kernels (count child boxes / triangle records tested, SURVEY §8d B_ray accounting).
 * Off by default: the counting costs registers and time. */
int sr_scene_set_instrumented(SrScene* scene, int on);

/* Per-launch device timing: when enabled every sr_trace_* launch is bracketed by a HIP event pair
 * recorded on the launch's own stream. sr_scene_read_timing waits for the recorded launches of one
 * kind, returns their summed elapsed time and count, and clears that kind's list.
 * kind: 0 = sr_trace_ris, 1 = sr_trace_final, 2 = sr_trace_closest, 3 = sr_trace_any. */
int sr_scene_enable_timing(SrScene* scene, int enable);
int sr_scene_read_timing(SrScene* scene, int kind, double* total_ms, uint32_t* n_launches);

/* ---- One frame on several devices from one Renderer ----------------------------------
 * A multi-device renderer is an SrRenderer with more than one device slot; every sr_renderer_* call keeps its meaning on it.
 * Each slot holds a replica of the scene and traces its strip of the frame (sr_strip_trace_ris / _final); the temporal-history
 * bands of sr_history_exchange_plan and the radiance / G-buffer strips move between slots as device-to-device peer copies, and
 * the post chain runs on the gathered frame on devices[0], so the output is the single-device output bit for bit whenever
 * sr_renderer_read_history_overflow reads 0. Two frames may be in flight, as with one device. */
/* devices[0..n): one slot per entry; the same device may repeat (all slots on one GPU = rehearsal mode). Output, the post
 * chain and the SrScene returned by sr_renderer_get live on devices[0]. n_devices == 1 is exactly sr_renderer_create. */
int sr_renderer_create_multi(const int* devices, uint32_t n_devices, uint32_t width, uint32_t height, uint32_t axis,
                             SrRenderer** out);
/* n_devices + 1 cuts (sr_partition_create rules). Allowed only before the first frame after create / resize, else SR_ERR_STATE. */
int sr_renderer_set_strip_bounds(SrRenderer* r, const uint32_t* bounds);
/* Temporal-history band exchanged after every RIS pass (sr_history_exchange_plan's motion_halo). Default 32 pixels.
 * Allowed only before the first frame after create / resize, else SR_ERR_STATE. */
int sr_renderer_set_motion_halo(SrRenderer* r, uint32_t pixels);
/* The replica scene of slot i (tests read per-slot ray counters through it). Slot 0's is the scene of sr_renderer_get. */
int sr_renderer_replica_scene(SrRenderer* r, uint32_t slot, SrScene** out);
/* Synchronising. Counts pixels, since create / resize, whose temporal-history read may have landed outside what their slot
 * held. 0 means every frame so far equals the single-device frame. Always 0 for one slot. */
int sr_renderer_read_history_overflow(SrRenderer* r, uint64_t* pixels);

#ifdef __cplusplus
}
#endif

#if defined(__cplusplus)
static_assert(sizeof(SrVertex) == 96, "T1");
static_assert(sizeof(SrMaterial) == 112, "Material");
static_assert(sizeof(SrMeshInfo) == 128, "T2");
static_assert(sizeof(SrEmissiveTriangle) == 64, "T3");
static_assert(sizeof(SrEmissiveIndirectionEntry) == 8, "T4");
static_assert(sizeof(SrTransform) == 48, "T5");
static_assert(sizeof(SrMatrices) == 256, "T6");
static_assert(sizeof(SrReservoir) == 48 && sizeof(SrReservoirGI) == 48, "T7");
static_assert(sizeof(SrRayPayload) == 32, "T8");
static_assert(sizeof(SrRay) == 32 && sizeof(SrHit) == 16, "ray/hit");
static_assert(sizeof(SrTraceConfig) == 40 && sizeof(SrRtParams) == 184, "T9");
static_assert(sizeof(SrPostParams) == 104, "post params");
static_assert(sizeof(SrStripTransfer) == 16 && sizeof(SrStripRects) == 56 && sizeof(SrStripPlane) == 16, "strip plans");
static_assert(sizeof(SrNodeProbeRow) == 336 && sizeof(SrNodeProbeOut) == 24, "node probe rows");
#endif

#endif /* SUNRAY_HIP_H */
