"""Loader of the in-tree HIP library (sunray_amd/libsunray_hip.so). There is NO fallback path: if
the library is missing or fails to load, every product entry point raises."""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SUNRAY_HIP_LIB") or os.path.join(_HERE, "libsunray_hip.so")   # override: kernel-tuning variants only
_lib = None

# every symbol include/sunray_hip.h declares
SYMBOLS = [
    "sr_last_error", "sr_version", "sr_camera_matrices", "sr_material_new", "sr_emissive_triangles_from_mesh",
    "sr_trace_config_default", "sr_scene_create", "sr_scene_destroy", "sr_as_state_initial", "sr_as_state_next_op", "sr_as_state_mark_built", "sr_scene_as_state", "sr_scene_end_frame",
    "sr_bvh_layout", "sr_tree_build_limits", "sr_scene_read_bvh", "sr_scene_force_next_op", "sr_scene_add_mesh", "sr_scene_add_blas", "sr_scene_remove", "sr_scene_add_image", "sr_scene_remove_image", "sr_scene_add_sampler", "sr_scene_set_instances",
    "sr_scene_get_tables", "sr_scene_bvh_stats", "sr_scene_resolve_triangle", "sr_host_bvh_build", "sr_host_bvh_get",
    "sr_host_bvh_destroy", "sr_trace_closest", "sr_trace_any", "sr_shade_closest_hit", "sr_any_hit_ignores", "sr_trace_ris", "sr_trace_final", "sr_post_temporal", "sr_post_denoise", "sr_post_tonemap", "sr_renderer_create", "sr_renderer_destroy",
    "sr_renderer_resize", "sr_renderer_add_start_of_frame_callback", "sr_renderer_add_end_of_frame_callback", "sr_renderer_add_resize_callback", "sr_renderer_load_mesh", "sr_renderer_set_config", "sr_renderer_render", "sr_renderer_wait_frame",
    "sr_renderer_render_to_host_memory", "sr_renderer_get", "sr_decode_image", "sr_decode_image_rgba8", "sr_renderer_set_blue_noise", "sr_gltf_open", "sr_gltf_close", "sr_gltf_counts", "sr_gltf_blas", "sr_gltf_instance", "sr_gltf_image",
    "sr_gltf_sampler", "sr_gltf_texture", "sr_renderer_load_gltf", "sr_renderer_load_scene", "sr_loaded_scene_get", "sr_loaded_scene_destroy",
    "sr_renderer_unload_scene", "sr_renderer_unload_mesh", "sr_default_noise_texture",
    "sr_scene_read_tile_row_costs", "sr_scene_read_tile_costs", "sr_scene_set_tile_costs", "sr_scene_read_tile_order", "sr_scene_reset_counters", "sr_scene_read_counters", "sr_scene_set_instrumented", "sr_scene_enable_timing",
    "sr_scene_read_timing",
    "sr_partition_create", "sr_partition_destroy", "sr_partition_get", "sr_partition_span", "sr_balanced_bounds", "sr_axis_cost_from_tiles",
    "sr_history_exchange_plan", "sr_strip_rects", "sr_strip_trace_ris", "sr_strip_trace_final",
    "sr_strip_packed_bytes", "sr_strip_pack", "sr_strip_unpack", "sr_history_reach_check", "sr_scene_set_instancing", "sr_scene_instancing",
    "sr_renderer_create_multi", "sr_renderer_set_strip_bounds", "sr_renderer_set_motion_halo", "sr_renderer_replica_scene",
    "sr_renderer_read_history_overflow",
    "sr_scene_set_top_level_build", "sr_scene_top_level_info", "sr_scene_read_top_level",
    "sr_scene_update_mesh", "sr_scene_mesh_update_info", "sr_renderer_update_mesh",
    "sr_scene_set_mesh_build_type", "sr_scene_mesh_as_state", "sr_scene_read_mesh_tree", "sr_renderer_set_mesh_build_type",
    "sr_scene_set_mesh_tree_build", "sr_scene_mesh_tree_info", "sr_renderer_set_mesh_tree_build",
    "sr_scene_set_mesh_tree_batch", "sr_scene_mesh_tree_batch_info", "sr_renderer_set_mesh_tree_batch",
    "sr_scene_set_tree_height_bound", "sr_scene_tree_height_info", "sr_renderer_set_tree_height_bound",
    "sr_scene_update_mesh_device", "sr_scene_mesh_vertex_info", "sr_renderer_update_mesh_device",
    "sr_scene_set_mesh_skin", "sr_scene_skin_mesh", "sr_scene_mesh_skin_info", "sr_renderer_set_mesh_skin", "sr_renderer_skin_mesh",
    "sr_gltf_rig_counts", "sr_gltf_blas_skin", "sr_gltf_skin", "sr_gltf_animation", "sr_gltf_animation_ignored_channels", "sr_gltf_pose", "sr_gltf_sample_node",
    "sr_renderer_attach_skins", "sr_renderer_pose_scene",
    "sr_scene_set_mesh_morph", "sr_scene_pose_mesh", "sr_scene_mesh_morph_info", "sr_renderer_set_mesh_morph", "sr_renderer_pose_mesh",
    "sr_gltf_blas_morph", "sr_gltf_morph_weights", "sr_renderer_attach_morphs",
    "sr_mesh_frame_adjacency", "sr_mesh_frame_host", "sr_scene_set_mesh_frame", "sr_scene_update_mesh_positions_device", "sr_scene_update_mesh_positions",
    "sr_scene_mesh_frame_info", "sr_renderer_set_mesh_frame", "sr_renderer_update_mesh_positions_device", "sr_renderer_update_mesh_positions",
    "sr_scene_set_light_table_build", "sr_scene_light_table_info", "sr_scene_read_lights", "sr_light_table",
    "sr_renderer_set_light_table_build", "sr_renderer_light_table_info",
    "sr_scene_set_instances_device", "sr_scene_instance_update_info", "sr_scene_read_instance_tables", "sr_instance_tables_host",
    "sr_renderer_render_device_transforms",
    "sr_probe_helper", "sr_probe_helper_layout", "sr_probe_node_step", "sr_probe_tl_record", "sr_scene_light_stage_capacity",
    "sr_scene_pose_meshes", "sr_scene_pose_batch_info", "sr_pose_batch_plan", "sr_renderer_pose_meshes", "sr_renderer_set_pose_batch",
    "sr_gltf_bake_clip", "sr_clip_destroy", "sr_clip_info", "sr_clip_skin", "sr_clip_layout", "sr_clip_channel_keys","sr_clip_sample_host", "sr_clip_compose_host", "sr_clip_pose_host",
    "sr_clip_morph_count", "sr_clip_morph", "sr_clip_morph_keys", "sr_clip_weights_host", "sr_scene_read_item_active",
    "sr_scene_attach_clip", "sr_scene_detach_clip", "sr_scene_pose_actors", "sr_scene_actor_pose_info", "sr_scene_read_actor_nodes", "sr_scene_read_actor_matrices",
    "sr_renderer_attach_clip", "sr_renderer_detach_clip", "sr_renderer_pose_actors", "sr_renderer_actor_pose_info",
    "sr_clip_blend_compatible", "sr_clip_blend_host", "sr_clip_compose_records_host", "sr_clip_pose_blend_host", "sr_clip_blend_weights_host",
    "sr_scene_pose_actors_blended", "sr_scene_read_actor_sources", "sr_renderer_pose_actors_blended",
    "sr_gltf_set_cubicspline", "sr_gltf_cubicspline", "sr_gltf_animation_cubic", "sr_scene_spline_pose_info", "sr_renderer_spline_pose_info",
    "sr_clip_subtree_mask", "sr_clip_layers_host", "sr_clip_pose_layers_host", "sr_scene_attach_node_mask", "sr_scene_detach_node_mask",
    "sr_scene_pose_actors_layered", "sr_scene_layer_pose_info", "sr_scene_read_actor_layer",
    "sr_renderer_attach_node_mask", "sr_renderer_detach_node_mask", "sr_renderer_pose_actors_layered",
    "sr_clip_layer_weights_host", "sr_clip_weights_layers_host", "sr_scene_layer_weights_info", "sr_renderer_layer_weights_info",
]


class SunrayError(RuntimeError):
    """SrError (src/error.rs:6-46): status code + description."""

    def __init__(self, code, description):
        super().__init__("sunray_hip error %d: %s" % (code, description))
        self.code = code
        self.description = description


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "sunray_amd: %s is missing — build it with `python -m sunray_amd.build` (or "
                "__graft_entry__.build()). There is no CPU fallback for the product path." % LIB_PATH)
        # The harnesses hand torch tensors to the library, so both must talk to ONE HIP runtime. torch ships its own copy of
        # libamdhip64; loading ours first would bring in /opt/rocm's as a second runtime (and the later one finds "no
        # ROCm-capable device"). Importing torch first makes the dynamic linker reuse its runtime for this library.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.sr_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SunrayError(rc, lib().sr_last_error().decode("utf-8", "replace"))
