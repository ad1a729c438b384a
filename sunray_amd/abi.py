"""Python mirror of include/sunray_hip.h: numpy dtypes and ctypes structures of the C ABI.

Pure data definitions (no library is loaded here). Layouts follow the reference's GPU structs
(shaders/rt_types.slang) byte for byte; see the header for the file:line of each.
"""
import ctypes as C

import numpy as np

NULL_TEXTURE = 0xFFFFFFFF
TRACE_FLAG_UNCOUNTED = 1
TRACE_FLAG_TRACE_EVERY_QUERY = 2
MAX_BOUNCES = 8192          # SR_MAX_BOUNCES
TILE_ORDER_NONE = 0xFFFFFFFF  # entry of a tile list past its last tile (sr_scene_read_tile_order)

# T1 VertexAttributes (rt_types.slang:24-36) — 96 B
VERTEX = np.dtype([
    ("position", "<f4", 3), ("_pad0", "<f4"), ("normal", "<f4", 3), ("_pad1", "<f4"),
    ("tangent", "<f4", 4), ("base_color_tex_coord", "<f4", 2), ("metallic_roughness_tex_coord", "<f4", 2),
    ("normal_tex_coord", "<f4", 2), ("occlusion_tex_coord", "<f4", 2), ("emissive_tex_coord", "<f4", 2),
    ("_pad3", "<f4", 2)])
# Material (resources/material.rs:15-44) — 112 B
MATERIAL = np.dtype([
    ("base_color_value", "<f4", 4), ("metallic_factor", "<f4"), ("roughness_factor", "<f4"),
    ("_pad_mid", "<f4", 2), ("emissive_factor", "<f4", 4), ("alpha_mode", "<u4"), ("alpha_cutoff", "<f4"),
    ("transmission_factor", "<f4"), ("ior", "<f4"),
    ("base_color_image", "<u4"), ("base_color_sampler", "<u4"),
    ("metallic_roughness_image", "<u4"), ("metallic_roughness_sampler", "<u4"),
    ("normal_image", "<u4"), ("normal_sampler", "<u4"),
    ("occlusion_image", "<u4"), ("occlusion_sampler", "<u4"),
    ("emissive_image", "<u4"), ("emissive_sampler", "<u4"), ("_pad_end", "<u4", 2)])
MESH_INFO = np.dtype([("vertices", "<u8"), ("indices", "<u8"), ("material", MATERIAL)])  # T2, 128 B
EMISSIVE_TRIANGLE = np.dtype([("v0", "<f4", 4), ("v1", "<f4", 4), ("v2", "<f4", 4), ("emission", "<f4", 4)])  # T3
EMISSIVE_INDIRECTION = np.dtype([("blas_tri_index", "<u4"), ("entity_id", "<u4")])  # T4
TRANSFORM = np.dtype([("m", "<f4", 12)])  # T5 row-major 3x4
RESERVOIR = np.dtype([("light_pos", "<f4", 3), ("w_sum", "<f4"), ("light_normal", "<f4", 3), ("M", "<f4"),
                      ("light_idx", "<u4"), ("W", "<f4"), ("hit_normal_packed", "<u4"), ("depth", "<f4")])  # T7
RESERVOIR_GI = np.dtype([("sample_pos", "<f4", 3), ("w_sum", "<f4"), ("sample_radiance", "<f4", 3), ("M", "<f4"),
                         ("sample_normal_packed", "<u4"), ("W", "<f4"), ("hit_normal_packed", "<u4"), ("depth", "<f4")])
RAY_PAYLOAD = np.dtype([("emission", "<f4", 3), ("dist", "<f4"), ("albedo_packed", "<u4"), ("normal_packed", "<u4"),
                        ("material_info", "<u4"), ("transmission_ior_packed", "<u4")])  # T8
RAY = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("dir", "<f4", 3), ("tmax", "<f4")])
HIT = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4")])

assert VERTEX.itemsize == 96 and MATERIAL.itemsize == 112 and MESH_INFO.itemsize == 128
assert EMISSIVE_TRIANGLE.itemsize == 64 and EMISSIVE_INDIRECTION.itemsize == 8 and TRANSFORM.itemsize == 48
assert RESERVOIR.itemsize == 48 and RESERVOIR_GI.itemsize == 48 and RAY_PAYLOAD.itemsize == 32
assert RAY.itemsize == 32 and HIT.itemsize == 16


class SrMatrices(C.Structure):  # T6, 256 B; every float[16] = 4 rows
    _fields_ = [("view_inverse", C.c_float * 16), ("proj_inverse", C.c_float * 16),
                ("view_proj", C.c_float * 16), ("prev_view_proj", C.c_float * 16)]


class SrTraceConfig(C.Structure):
    _fields_ = [("max_bounces", C.c_uint32), ("shadow_bounces", C.c_uint32), ("ris_candidates", C.c_uint32),
                ("virtual_bounces", C.c_uint32), ("enable_restir", C.c_uint32), ("flags", C.c_uint32),
                ("count_y0", C.c_uint32), ("count_rows", C.c_uint32), ("count_x0", C.c_uint32), ("count_cols", C.c_uint32)]

    @staticmethod
    def reference():
        """The reference's compile-time constants (ray_gen_final.slang:40-42, ray_gen_ris.slang:69,187)."""
        return SrTraceConfig(10, 5, 16, 20, 1, 0, 0, 0, 0, 0)


class SrRtParams(C.Structure):  # T9
    _fields_ = [("scene", C.c_void_p), ("raw_color", C.c_void_p), ("depth_img", C.c_void_p),
                ("normal_img", C.c_void_p), ("diffuse_img", C.c_void_p), ("motion_vec_img", C.c_void_p),
                ("matrices", C.POINTER(SrMatrices)), ("blue_noise_tex", C.c_void_p),
                ("blue_noise_w", C.c_uint32), ("blue_noise_h", C.c_uint32),
                ("reservoirs", C.c_void_p * 2), ("reservoirs_gi", C.c_void_p * 2), ("primary_payload", C.c_void_p),
                ("frame_count", C.c_uint32), ("use_srgb", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("tile_y0", C.c_uint32), ("tile_h", C.c_uint32),
                ("tile_x0", C.c_uint32), ("tile_w", C.c_uint32), ("config", SrTraceConfig)]


class SrPostParams(C.Structure):  # post-RT compute chain (temporal accumulation, a-trous denoise, tonemap)
    _fields_ = [("raw_color", C.c_void_p), ("motion_vec_img", C.c_void_p), ("depth_img", C.c_void_p),
                ("normal_img", C.c_void_p), ("diffuse_img", C.c_void_p), ("accum", C.c_void_p * 2),
                ("denoise", C.c_void_p * 2), ("output_rgba8", C.c_void_p), ("frame_count", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("exposure", C.c_float),
                ("denoise_passes", C.c_uint32), ("_pad", C.c_uint32)]


def post_params(frame, frame_count, ptr, exposure=1.0, denoise_passes=4):
    """SrPostParams over a HostFrame / DeviceFrame; `ptr(buffer)` gives the address of a buffer.
    Defaults are the reference's EXPOSURE and DENOISE_PASSES (src/lib.rs:42,44)."""
    p = SrPostParams()
    p.raw_color, p.motion_vec_img = ptr(frame.raw_color), ptr(frame.motion)
    p.depth_img, p.normal_img, p.diffuse_img = ptr(frame.depth), ptr(frame.normal), ptr(frame.diffuse)
    p.accum[0], p.accum[1] = ptr(frame.accum[0]), ptr(frame.accum[1])
    p.denoise[0], p.denoise[1] = ptr(frame.denoise[0]), ptr(frame.denoise[1])
    p.output_rgba8 = ptr(frame.output)
    p.frame_count, p.width, p.height = frame_count, frame.width, frame.height
    p.exposure, p.denoise_passes = exposure, denoise_passes
    return p


class SrRayCounters(C.Structure):
    _fields_ = [("closest_queries", C.c_uint64), ("any_queries", C.c_uint64),
                ("boxes_tested", C.c_uint64), ("tris_tested", C.c_uint64), ("reused_primary_hits", C.c_uint64), ("reused_visibility_queries", C.c_uint64)]


class SrBvhStats(C.Structure):
    _fields_ = [("n_triangles", C.c_uint64), ("n_nodes", C.c_uint64), ("node_bytes", C.c_uint64),
                ("tri_bytes", C.c_uint64), ("max_depth", C.c_uint32), ("sah_cost", C.c_float),
                ("max_stack", C.c_uint32), ("_pad", C.c_uint32), ("build_ms", C.c_double)]


def material(base_color=(0.8, 0.8, 0.8, 1.0), metallic=0.0, roughness=0.5, emissive_factor=(0.0, 0.0, 0.0),
             emissive_strength=0.0, transmission=0.0, ior=1.5, textures=None):
    """Material::new (resources/material.rs:52-92). Runtime meshes have all textures NULL (lib.rs:937-943);
    `textures` = {"base_color"|"metallic_roughness"|"normal"|"occlusion"|"emissive": (image slot, sampler slot)}
    is what the glTF path's `resolve` closure fills in."""
    m = np.zeros((), dtype=MATERIAL)
    m["base_color_value"] = base_color
    m["metallic_factor"] = metallic
    m["roughness_factor"] = roughness
    m["emissive_factor"] = tuple(emissive_factor) + (emissive_strength,)
    m["transmission_factor"] = transmission
    m["ior"] = ior
    for k in ("base_color", "metallic_roughness", "normal", "occlusion", "emissive"):
        m[k + "_image"] = NULL_TEXTURE
        m[k + "_sampler"] = NULL_TEXTURE
    for k, (img, smp) in (textures or {}).items():
        m[k + "_image"] = img
        m[k + "_sampler"] = smp
    return m


FILTER_NEAREST, FILTER_LINEAR = 0, 1
ADDRESS_REPEAT, ADDRESS_MIRRORED_REPEAT, ADDRESS_CLAMP_TO_EDGE = 0, 1, 2


class SrSamplerDesc(C.Structure):
    _fields_ = [("min_filter", C.c_uint32), ("mag_filter", C.c_uint32), ("address_mode_u", C.c_uint32), ("address_mode_v", C.c_uint32)]


IDENTITY_TRANSFORM = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)


class SrAsState(C.Structure):
    _fields_ = [("changing", C.c_uint32), ("frames_without_changes", C.c_uint32), ("number_of_updates_since_last_rebuild", C.c_uint32),
                ("_pad", C.c_uint32)]


BUILD_RAPIDLY_CHANGING, BUILD_SOMETIMES_CHANGES, BUILD_STATIC = 0, 1, 2


class SrTopLevelInfo(C.Structure):  # the last top-level build of a two-level scene (sr_scene_top_level_info)
    _fields_ = [("on_device", C.c_uint32), ("reason", C.c_uint32), ("mode", C.c_uint32), ("auto_threshold", C.c_uint32),
                ("n_nodes", C.c_uint32), ("n_boxes", C.c_uint32), ("n_instances", C.c_uint32), ("max_stack", C.c_uint32),
                ("blas_stack", C.c_uint32), ("_pad", C.c_uint32), ("records_ms", C.c_double), ("tree_ms", C.c_double),
                ("build_ms", C.c_double)]


class SrMeshUpdateInfo(C.Structure):  # the last sr_scene_update_mesh and the sr_scene_set_instances that applied it
    _fields_ = [("dirty_meshes", C.c_uint32), ("reshaded", C.c_uint32), ("blas_rebuilt", C.c_uint32), ("blas_refitted", C.c_uint32),
                ("validate_copy_ms", C.c_double), ("h2d_ms", C.c_double), ("tables_ms", C.c_double), ("flatten_ms", C.c_double),
                ("refit_ms", C.c_double), ("blas_build_ms", C.c_double)]


class SrMeshVertexInfo(C.Structure):  # one mesh's host copy against its device buffer (sr_scene_mesh_vertex_info), 40 B
    _fields_ = [("host_stale", C.c_uint32), ("last_from_device", C.c_uint32), ("host_fetches", C.c_uint32), ("_pad", C.c_uint32),
                ("check_ms", C.c_double), ("copy_ms", C.c_double), ("fetch_ms", C.c_double)]


class SrLightTableInfo(C.Structure):  # the light table of the last sr_scene_set_instances (sr_scene_light_table_info), 56 B
    _fields_ = [("mode", C.c_uint32), ("on_device", C.c_uint32), ("num_lights", C.c_uint32), ("arena_entries", C.c_uint32),
                ("positions_rewritten", C.c_uint32), ("entries_uploaded", C.c_uint32), ("arena_uploads", C.c_uint32), ("arena_fetches", C.c_uint32),
                ("positions_ms", C.c_double), ("table_ms", C.c_double), ("host_ms", C.c_double)]


LIGHTS_HOST, LIGHTS_DEVICE = 0, 1


class SrInstanceUpdateInfo(C.Structure):  # the last set_instances / set_instances_device and the fetches since (sr_scene_instance_update_info), 48 B
    _fields_ = [("from_device", C.c_uint32), ("host_stale", C.c_uint32), ("host_fetches", C.c_uint32), ("fetch_reason", C.c_uint32),
                ("layout_rebuilt", C.c_uint32), ("n_instances", C.c_uint32), ("bad_index", C.c_uint32), ("_pad", C.c_uint32),
                ("tables_ms", C.c_double), ("fetch_ms", C.c_double)]


# SrInstanceUpdateInfo.fetch_reason
INST_FETCH_NONE, INST_FETCH_HOST_TOP_LEVEL, INST_FETCH_HOST_BUILD, INST_FETCH_HOST_LIGHT_TABLE, INST_FETCH_SETTLE, INST_FETCH_GET_TABLES, INST_FETCH_MESH_TREES = range(7)
# the per-instance device tables (sr_scene_read_instance_tables): DevInstance 96 B, FlatInstance 64 B
DEV_INSTANCE = np.dtype([("w2o", np.float32, (12,)), ("o2w", np.float32, (12,))])
FLAT_INSTANCE = np.dtype([("o2w", np.float32, (12,)), ("tri_offset", np.uint32), ("mesh_slot", np.uint32), ("_pad", np.uint32, (2,))])


class SrSkinInfluence(C.Structure):  # one vertex's joints and weights (sr_scene_set_mesh_skin), 24 B
    _fields_ = [("joint", C.c_uint16 * 4), ("weight", C.c_float * 4)]


SKIN_INFLUENCE = np.dtype([("joint", "<u2", 4), ("weight", "<f4", 4)])
assert SKIN_INFLUENCE.itemsize == 24 == C.sizeof(SrSkinInfluence)


class SrMeshSkinInfo(C.Structure):  # one mesh's skin and its last pose (sr_scene_mesh_skin_info), 24 B
    _fields_ = [("n_joints", C.c_uint32), ("skinned", C.c_uint32), ("first_bad", C.c_uint32), ("_pad", C.c_uint32), ("skin_ms", C.c_double)]


class SrMorphDelta(C.Structure):  # one (target, vertex) record of sr_scene_set_mesh_morph: the first three pieces of a vertex, 48 B
    _fields_ = [("position", C.c_float * 3), ("_pad0", C.c_float), ("normal", C.c_float * 3), ("_pad1", C.c_float),
                ("tangent", C.c_float * 3), ("_pad2", C.c_float)]


MORPH_DELTA = np.dtype([("position", "<f4", 3), ("_pad0", "<f4"), ("normal", "<f4", 3), ("_pad1", "<f4"), ("tangent", "<f4", 3), ("_pad2", "<f4")])
assert MORPH_DELTA.itemsize == 48 == C.sizeof(SrMorphDelta)


class SrMeshMorphInfo(C.Structure):  # one mesh's morph and its last pose (sr_scene_mesh_morph_info), 24 B
    _fields_ = [("n_targets", C.c_uint32), ("posed", C.c_uint32), ("n_active", C.c_uint32), ("first_bad", C.c_uint32), ("morph_ms", C.c_double)]


class SrPoseItem(C.Structure):  # one mesh of a batch (sr_scene_pose_meshes): the arguments of sr_scene_pose_mesh by value, 32 B
    _fields_ = [("key", C.c_uint64), ("weights", C.c_void_p), ("joint_matrices", C.c_void_p), ("n_targets", C.c_uint32), ("n_joints", C.c_uint32)]


class SrPoseBatchInfo(C.Structure):  # the last sr_scene_pose_meshes that reached the device (sr_scene_pose_batch_info), 80 B
    _fields_ = [("items", C.c_uint32), ("blocks", C.c_uint32), ("vertices", C.c_uint64), ("morph_only", C.c_uint32), ("skin_only", C.c_uint32),
                ("fused", C.c_uint32), ("launches", C.c_uint32), ("read_backs", C.c_uint32), ("calls", C.c_uint32), ("refused_item", C.c_uint32),
                ("refused_vertex", C.c_uint32), ("upload_bytes", C.c_uint64), ("pose_ms", C.c_double), ("scatter_ms", C.c_double), ("host_ms", C.c_double)]


POSE_BATCH_OFF, POSE_BATCH_ON, POSE_BATCH_TILE = 0, 1, 256  # sr_renderer_set_pose_batch; vertices a block of the posing launch


class SrClipInfo(C.Structure):  # a baked clip (sr_clip_info), 40 B
    _fields_ = [("animation", C.c_int32), ("n_nodes", C.c_uint32), ("n_levels", C.c_uint32), ("n_channels", C.c_uint32), ("n_skins", C.c_uint32),
                ("n_joints", C.c_uint32), ("n_instances", C.c_uint32), ("n_keys", C.c_uint32), ("duration_seconds", C.c_float), ("device_bytes", C.c_uint32)]


CLIP_NODE_INFO = np.dtype([("parent", "<u4"), ("gltf_node", "<u4"), ("animated", "<u4"), ("level", "<u4")])  # sr_clip_layout
CLIP_CHANNEL_INFO = np.dtype([("node", "<u4"), ("path", "<u4"), ("interpolation", "<u4"), ("n_keys", "<u4")])
NODE_TRS = np.dtype([("translation", "<f4", 3), ("rotation", "<f4", 4), ("scale", "<f4", 3), ("animated", "<u4"), ("reserved", "<u4")])  # SrNodeTrs, 48 B
assert NODE_TRS.itemsize == 48
CLIP_MAX_NODES, CLIP_NO_NODE, ACTOR_NO_SKIN, ACTORS_KEEP_NODES = 384, 0xFFFFFFFF, 0xFFFFFFFF, 1
CLIP_MORPH_CHANNEL, CLIP_MORPH_DEFAULTS, CLIP_MORPH_UNAVAILABLE = 0, 1, 2  # SrClipMorphInfo.state
CLIP_LINEAR, CLIP_STEP, CLIP_CUBICSPLINE = 0, 1, 2  # SrClipChannelInfo.interpolation, SrClipMorphInfo.interpolation
CUBICSPLINE_REFUSE, CUBICSPLINE_SAMPLE = 0, 1  # sr_gltf_set_cubicspline


def actor_clip_weights(blas):
    """SR_ACTOR_CLIP_WEIGHTS(blas): SrActorPoseItem.morph of an item whose weights are that morph set of its actor's clip."""
    return int(blas) + 1


class SrClipMorphInfo(C.Structure):  # one morph set of a baked clip (sr_clip_morph), 32 B
    _fields_ = [("blas", C.c_uint32), ("gltf_node", C.c_uint32), ("n_targets", C.c_uint32), ("n_keys", C.c_uint32), ("interpolation", C.c_uint32),
                ("state", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_uint32)]


assert C.sizeof(SrClipMorphInfo) == 32


class SrClipActor(C.Structure):  # one character of sr_scene_pose_actors: a clip at a time, 32 B
    _fields_ = [("clip_id", C.c_uint32), ("time_seconds", C.c_float), ("placement", C.c_void_p), ("instance_rows", C.c_void_p),
                ("instance_base", C.c_uint32), ("reserved", C.c_uint32)]


class SrActorPoseItem(C.Structure):  # one mesh of sr_scene_pose_actors: SrPoseItem with the joint matrices named, 32 B
    _fields_ = [("key", C.c_uint64), ("actor", C.c_uint32), ("skin", C.c_uint32), ("weights", C.c_void_p), ("n_targets", C.c_uint32), ("morph", C.c_uint32)]


class SrActorPoseInfo(C.Structure):  # the last sr_scene_pose_actors that reached the device (sr_scene_actor_pose_info), 88 B
    _fields_ = [("actors", C.c_uint32), ("items", C.c_uint32), ("nodes", C.c_uint64), ("channels", C.c_uint64), ("upload_bytes", C.c_uint64),
                ("launches", C.c_uint32), ("read_backs", C.c_uint32), ("calls", C.c_uint32), ("refused_actor", C.c_uint32), ("refused_item", C.c_uint32),
                ("weight_items", C.c_uint32), ("clip_ms", C.c_double), ("pose_ms", C.c_double), ("scatter_ms", C.c_double), ("host_ms", C.c_double)]


assert C.sizeof(SrClipInfo) == 40 and C.sizeof(SrClipActor) == 32 and C.sizeof(SrActorPoseItem) == 32 and C.sizeof(SrActorPoseInfo) == 88


class SrSplinePoseInfo(C.Structure):  # the cubic side of the last pose_actors / pose_actors_blended that reached the device, 32 B
    _fields_ = [("spline_weight_rows", C.c_uint32), ("plain_weight_rows", C.c_uint32), ("cubic_channels", C.c_uint64),
                ("spline_weights_ms", C.c_double), ("reserved", C.c_uint64)]


assert C.sizeof(SrSplinePoseInfo) == 32


class SrClipBlendActor(C.Structure):  # one character of sr_scene_pose_actors_blended: between two clips, 48 B
    _fields_ = [("clip_id", C.c_uint32), ("time_seconds", C.c_float), ("clip_id_b", C.c_uint32), ("time_seconds_b", C.c_float), ("weight", C.c_float),
                ("reserved", C.c_uint32), ("placement", C.c_void_p), ("instance_rows", C.c_void_p), ("instance_base", C.c_uint32), ("reserved2", C.c_uint32)]


ACTORS_KEEP_SOURCES = 2  # SR_ACTORS_KEEP_SOURCES
assert C.sizeof(SrClipBlendActor) == 48


class SrClipLayer(C.Structure):  # one layer of an actor of sr_scene_pose_actors_layered, 32 B
    _fields_ = [("clip_id", C.c_uint32), ("time_seconds", C.c_float), ("weight", C.c_float), ("mode", C.c_uint32), ("mask_id", C.c_uint32),
                ("ref_time_seconds", C.c_float), ("reserved", C.c_uint32 * 2)]


class SrClipLayerActor(C.Structure):  # one character as a stack of layers, 40 B
    _fields_ = [("layers", C.c_void_p), ("n_layers", C.c_uint32), ("instance_base", C.c_uint32), ("placement", C.c_void_p), ("instance_rows", C.c_void_p),
                ("reserved", C.c_uint64)]


class SrClipLayerRule(C.Structure):  # one layer of sr_clip_layers_host, 16 B
    _fields_ = [("weight", C.c_float), ("mode", C.c_uint32), ("mask", C.c_void_p)]


class SrLayerPoseInfo(C.Structure):  # the last sr_scene_pose_actors_layered that reached the device (sr_scene_layer_pose_info), 32 B
    _fields_ = [("layers", C.c_uint32), ("additive_layers", C.c_uint32), ("masked_layers", C.c_uint32), ("max_layers", C.c_uint32),
                ("layer_table_bytes", C.c_uint64), ("reserved", C.c_uint64)]


CLIP_MAX_LAYERS, LAYER_OVERRIDE, LAYER_ADDITIVE, LAYER_NO_MASK, ACTORS_KEEP_LAYERS = 8, 0, 1, 0xFFFFFFFF, 4
assert C.sizeof(SrClipLayer) == 32 and C.sizeof(SrClipLayerActor) == 40 and C.sizeof(SrClipLayerRule) == 16 and C.sizeof(SrLayerPoseInfo) == 32


class SrLayerWeightsInfo(C.Structure):  # the clip-weighted items of the last layered call that reached the device (sr_scene_layer_weights_info), 32 B
    _fields_ = [("rows", C.c_uint32), ("samples", C.c_uint32), ("cubic_samples", C.c_uint32), ("reserved", C.c_uint32),
                ("table_bytes", C.c_uint64), ("weights_ms", C.c_double)]


ACTORS_LAYER_WEIGHTS = 8  # SR_ACTORS_LAYER_WEIGHTS
assert C.sizeof(SrLayerWeightsInfo) == 32


class SrMeshFrameInfo(C.Structure):  # one mesh's frame and its last position update (sr_scene_mesh_frame_info), 32 B
    _fields_ = [("flags", C.c_uint32), ("n_groups", C.c_uint32), ("n_entries", C.c_uint32), ("max_valence", C.c_uint32),
                ("updates", C.c_uint32), ("first_bad", C.c_uint32), ("frame_ms", C.c_double)]


FRAME_NORMALS, FRAME_TANGENTS = 1, 2  # sr_scene_set_mesh_frame: tangents need normals


class SrMeshTreeInfo(C.Structure):  # the mesh-tree builds of the last sr_scene_set_instances (sr_scene_mesh_tree_info)
    _fields_ = [("mode", C.c_uint32), ("auto_threshold", C.c_uint32), ("built_on_device", C.c_uint32), ("built_on_host", C.c_uint32),
                ("reason", C.c_uint32), ("n_nodes", C.c_uint32), ("max_stack", C.c_uint32), ("_pad", C.c_uint32), ("device_build_ms", C.c_double)]


class SrMeshTreeBatchInfo(C.Structure):  # the batched mesh-tree builds of the last sr_scene_set_instances (sr_scene_mesh_tree_batch_info)
    _fields_ = [("mode", C.c_uint32), ("max_tris", C.c_uint32), ("batched", C.c_uint32), ("passed_on", C.c_uint32), ("launches", C.c_uint32),
                ("reserved", C.c_uint32), ("batch_ms", C.c_double)]


class SrTreeHeightInfo(C.Structure):  # the last device fast build of one kind of tree (sr_scene_tree_height_info)
    _fields_ = [("mode", C.c_uint32), ("mesh_tree_cap", C.c_uint32), ("on_device", C.c_uint32), ("cap", C.c_uint32),
                ("height_before", C.c_uint32), ("height_after", C.c_uint32), ("subtrees_rebuilt", C.c_uint32), ("prims_rebuilt", C.c_uint32)]


HEIGHT_BOUND_REFUSE, HEIGHT_BOUND_REBALANCE = 0, 1
TREE_KIND_ONE_LEVEL, TREE_KIND_TOP_LEVEL, TREE_KIND_MESH = 0, 1, 2
MESH_TREE_BUILD_AUTO, MESH_TREE_BUILD_HOST, MESH_TREE_BUILD_DEVICE = 0, 1, 2
BLAS_BATCH_OFF, BLAS_BATCH_ON, BLAS_BATCH_MAX_TRIS = 0, 1, 4096  # sr_scene_set_mesh_tree_batch
(MESH_TREE_ON_DEVICE, MESH_TREE_HOST_MODE, MESH_TREE_HOST_BELOW_THRESHOLD, MESH_TREE_HOST_SLOW_BUILD, MESH_TREE_HOST_BAKED_INSTANCE,
 MESH_TREE_HOST_NOT_RESIDENT, MESH_TREE_HOST_STACK_BUDGET, MESH_TREE_HOST_STATIC_MESH) = range(8)
MESH_TREE_STACK_CAP = 26  # stack entries a mesh tree of the two-level form may need (csrc/api.cpp)
TL_BUILD_AUTO, TL_BUILD_HOST, TL_BUILD_DEVICE = 0, 1, 2
(TL_ON_DEVICE, TL_HOST_MODE, TL_HOST_BELOW_THRESHOLD, TL_HOST_BAKED_INSTANCE, TL_HOST_STACK_BUDGET, TL_HOST_NOT_TWO_LEVEL,
 TL_HOST_TOO_FEW, TL_HOST_QUALITY_BUILD) = range(8)
TL_STACK_CAP = 47  # LDS stack entries a two-level walk may need: top level + leaf size + deepest mesh tree + 1 (csrc/api.cpp)
# DevTlInstance (csrc/traverse.h), 128 bytes: what sr_scene_read_top_level returns per instance
TL_INSTANCE = np.dtype([("w2o", np.float32, 12), ("o2w", np.float32, 12), ("blas_root", np.uint32), ("tri_offset", np.uint32),
                        ("pad_a", np.float32), ("pad_b", np.float32), ("mesh_slot", np.uint32), ("prim_base", np.uint32),
                        ("flags", np.uint32), ("_pad", np.uint32)])
OP_NONE, OP_SLOW_BUILD, OP_FAST_BUILD, OP_UPDATE = 0, 1, 2, 3


class SrStripTransfer(C.Structure):  # one point-to-point transfer of the temporal-history exchange
    _fields_ = [("src", C.c_uint32), ("dst", C.c_uint32), ("start", C.c_uint32), ("size", C.c_uint32)]


class SrStripRects(C.Structure):  # launch rectangles + counting window of one rank's share of a frame
    _fields_ = [("ris_y0", C.c_uint32), ("ris_h", C.c_uint32), ("ris_x0", C.c_uint32), ("ris_w", C.c_uint32),
                ("final_y0", C.c_uint32), ("final_h", C.c_uint32), ("final_x0", C.c_uint32), ("final_w", C.c_uint32),
                ("count_y0", C.c_uint32), ("count_rows", C.c_uint32), ("count_x0", C.c_uint32), ("count_cols", C.c_uint32),
                ("count_window", C.c_uint32), ("empty", C.c_uint32)]


class SrStripPlane(C.Structure):  # one per-pixel plane of a full-size image (sr_strip_pack / sr_strip_unpack)
    _fields_ = [("img", C.c_void_p), ("bpp", C.c_uint32), ("_pad", C.c_uint32)]


AXIS_COLS, AXIS_ROWS, SPATIAL_HALO, STRIP_MAX_PLANES = 0, 1, 30, 5

# SrProbeHelper, in the header's order: the id of a helper is its index (sr_probe_helper / sr_probe_helper_layout)
PROBE_HELPERS = ("sincos", "exp", "log", "pow", "pow5", "smoothstep", "f32_to_f16", "f16_to_f32", "pack_half_2x16", "unpack_half_2x16",
                 "pack_snorm_2x16", "unpack_snorm_2x16", "pack_unorm_4x8", "unpack_unorm_rgb", "pack_normal", "unpack_normal",
                 "pack_rgba8_snorm", "unsnorm8", "pack_b10g11r11", "unpack_b10g11r11", "pcg_hash", "init_rng", "rnd", "norm3", "reflect3",
                 "refract3", "build_onb", "smith_v_ggx", "smith_g1_ggx", "random_bounce", "sample_ggx_vndf", "eval_light", "gi_target_pdf",
                 "merge", "merge_gi", "transform_point", "intersect_tri")

# SrNodeProbeKind, and the host rows of sr_probe_node_step: SrNodeProbeRow 336 B, SrNodeProbeOut 24 B
NODE_PROBE_CLOSEST, NODE_PROBE_ANY, NODE_PROBE_CLOSEST_TL, NODE_PROBE_ANY_TL, NODE_PROBE_KEY, NODE_PROBE_COUNT = range(6)
NODE_PROBE_ROW = np.dtype([("origin", np.float32, 3), ("tmin", np.float32), ("dir", np.float32, 3), ("tmax", np.float32),
                           ("node", np.uint32, 16), ("tri", np.uint32, 12), ("mesh_node", np.uint32, 16), ("instance", np.uint32, 32)])
NODE_PROBE_OUT = np.dtype([("boxes", np.uint32), ("tris", np.uint32), ("t", np.float32), ("u", np.float32), ("v", np.float32),
                           ("tri", np.uint32)])
TL_RECORD_OK, TL_RECORD_NO_FINITE_BOX, TL_RECORD_BAKED = 0, 1, 2   # sr_probe_tl_record's result (csrc/tl_record.h)
