"""ctypes mirror of include/rtcore.h (the C ABI of libmyrt.so).

Field order and types follow the header exactly; `tests/test_abi.py` checks the
struct sizes against the compiled library.
"""
from __future__ import annotations

import ctypes as C

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)


class rt_vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]


class rt_material(C.Structure):
    _fields_ = [("ambient", rt_vec3), ("diffuse", rt_vec3), ("specular", rt_vec3), ("mirror", rt_vec3),
                ("absorption", rt_vec3), ("phong", C.c_double), ("ior", C.c_double),
                ("absorption_index", C.c_double), ("roughness", C.c_double), ("type", C.c_int32),
                ("_pad", C.c_int32)]


class rt_point_light(C.Structure):
    _fields_ = [("position", rt_vec3), ("intensity", rt_vec3)]


class rt_area_light(C.Structure):
    _fields_ = [("position", rt_vec3), ("normal", rt_vec3), ("radiance", rt_vec3), ("size", C.c_double)]


class rt_camera(C.Structure):
    _fields_ = [("type", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("num_samples", C.c_int32),
                ("position", rt_vec3), ("gaze_point", rt_vec3), ("gaze", rt_vec3), ("up", rt_vec3),
                ("fovy", C.c_double), ("near_distance", C.c_double), ("near_plane", C.c_double * 4),
                ("aperture_size", C.c_double), ("focus_distance", C.c_double)]


class rt_object(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material_id", C.c_int32), ("smooth", C.c_int32), ("id", C.c_int32),
                ("base_mesh_id", C.c_int32), ("indices_one_based", C.c_int32),
                ("transform", C.c_double * 16), ("motion_blur", rt_vec3),
                ("ply_path", C.c_char_p),
                ("positions", c_double_p), ("num_positions", C.c_int64),
                ("indices", c_int32_p), ("num_indices", C.c_int64),
                ("normals", c_double_p),
                ("v", rt_vec3 * 3), ("center", rt_vec3), ("normal", rt_vec3), ("radius", C.c_double),
                ("num_normals", C.c_int64)]


class rt_scene_desc(C.Structure):
    _fields_ = [("background_color", rt_vec3), ("ambient_light", rt_vec3),
                ("shadow_ray_epsilon", C.c_double), ("intersection_test_epsilon", C.c_double),
                ("max_recursion_depth", C.c_int32), ("num_materials", C.c_int32),
                ("materials", C.POINTER(rt_material)),
                ("num_point_lights", C.c_int32), ("num_area_lights", C.c_int32),
                ("point_lights", C.POINTER(rt_point_light)), ("area_lights", C.POINTER(rt_area_light)),
                ("num_objects", C.c_int32), ("num_cameras", C.c_int32),
                ("objects", C.POINTER(rt_object)), ("cameras", C.POINTER(rt_camera))]


RT_RENDER_FRAME_LAYOUT = 1
RT_RENDER_KERNEL_TIME = 2
RT_SCENE_DYNAMIC = 1
RT_SCENE_FORMAT_AUTO, RT_SCENE_FORMAT_JSON, RT_SCENE_FORMAT_XML = 0, 1, 2


class rt_stats(C.Structure):
    _fields_ = [("meshes", C.c_int64), ("triangles", C.c_int64), ("spheres", C.c_int64), ("planes", C.c_int64),
                ("primary_rays", C.c_int64), ("shadow_rays", C.c_int64), ("secondary_rays", C.c_int64),
                ("milliseconds", C.c_double), ("kernel_ms", C.c_double),
                ("shadow_rays_traced", C.c_int64), ("rewalked", C.c_int64)]


class rt_scene_info(C.Structure):
    _fields_ = [("meshes", C.c_int64), ("triangles", C.c_int64), ("spheres", C.c_int64), ("planes", C.c_int64),
                ("instances", C.c_int64), ("blas_nodes", C.c_int64), ("tlas_nodes", C.c_int64),
                ("max_depth", C.c_int64), ("build_ms", C.c_double), ("upload_ms", C.c_double),
                ("device_bytes", C.c_int64), ("scratch_bytes", C.c_int64)]


class rt_commit_stats(C.Structure):
    _fields_ = [("instances_moved", C.c_int64), ("bounds_ms", C.c_double), ("refit_ms", C.c_double),
                ("total_ms", C.c_double)]


RT_SCENE_DEFORMABLE = 2          # rt_scene_create_ex flag; implies RT_SCENE_DYNAMIC
RT_POSITIONS_DEVICE = 1          # rt_scene_set_mesh_positions: positions / normals are device pointers


class rt_deform_stats(C.Structure):
    _fields_ = [("meshes_deformed", C.c_int64), ("triangles", C.c_int64), ("instances_rebounded", C.c_int64),
                ("validate_ms", C.c_double), ("deform_ms", C.c_double), ("blas_refit_ms", C.c_double)]


# ---- rebuilding the flattened instance tree (appended under ABI 5: detected by symbol) ----
RT_COMMIT_REBUILD_FIT = 1        # rt_scene_commit_ex flag
(RT_REBUILD_NONE, RT_REBUILD_NO_TREE, RT_REBUILD_BLOCKED, RT_REBUILD_TOO_DEEP, RT_REBUILD_TOO_LARGE,
 RT_REBUILD_NO_MEMORY) = range(6)


class rt_rebuild_stats(C.Structure):
    _fields_ = [("rebuilt", C.c_int32), ("reason", C.c_int32), ("pairs", C.c_int64),
                ("nodes_before", C.c_int64), ("nodes_after", C.c_int64),
                ("depth_before", C.c_int64), ("depth_after", C.c_int64),
                ("sort_ms", C.c_double), ("build_ms", C.c_double), ("total_ms", C.c_double)]


REBUILD_SYMBOLS = ["rt_scene_commit_ex", "rt_scene_last_rebuild_stats"]

# ---- the clustered builder, the detail record and the tree cost (appended under ABI 5: detected by symbol) ----
RT_COMMIT_REBUILD_FIT_CLUSTERED = 8   # rt_scene_commit_ex flag, alone or with RT_COMMIT_REBUILD_FIT
RT_BUILDER_NONE, RT_BUILDER_MORTON, RT_BUILDER_CLUSTERED = range(3)   # rt_rebuild_detail.builder


class rt_rebuild_detail(C.Structure):
    _fields_ = [("builder", C.c_int32), ("iterations", C.c_int32), ("fell_back", C.c_int32), ("pad", C.c_int32),
                ("cluster_ms", C.c_double), ("cost_before", C.c_double), ("cost_after", C.c_double)]


REBUILD_DETAIL_SYMBOLS = ["rt_scene_last_rebuild_detail", "rt_scene_fit_cost"]


# ---- instance visibility (appended under ABI 5: detected by symbol) ----
class rt_visibility_stats(C.Structure):
    _fields_ = [("instances", C.c_int64), ("visible", C.c_int64), ("shown", C.c_int64), ("hidden", C.c_int64),
                ("pairs", C.c_int64), ("pairs_visible", C.c_int64), ("pairs_in_tree", C.c_int64),
                ("forced_rebuild", C.c_int32), ("fit_complete", C.c_int32)]


VISIBILITY_SYMBOLS = ["rt_scene_set_instance_visible", "rt_scene_set_instances_visible", "rt_scene_instance_visible",
                      "rt_scene_last_visibility_stats"]


class rt_wide_dump(C.Structure):
    """rt_debug_wide_build / rt_debug_wide_read (rtcore.h): counts and scalars out, capacities in,
    caller-sized buffers."""
    _fields_ = [("wnodes", C.c_int64), ("wide_copy", C.c_int64), ("tris", C.c_int64), ("pairs", C.c_int64),
                ("instances", C.c_int64), ("tw_tlas_nodes", C.c_int64), ("fit_nodes", C.c_int64),
                ("marker_base", C.c_int64), ("tlas_leaf_base", C.c_int64),
                ("wide_root", C.c_int32), ("fit_root", C.c_int32), ("identity", C.c_int32),
                ("fit_blocked", C.c_int32), ("wide_coord", C.c_double), ("fit_coord", C.c_double),
                ("cap_wnodes", C.c_int64), ("cap_tris", C.c_int64), ("cap_pairs", C.c_int64),
                ("cap_instances", C.c_int64),
                ("nodes", C.c_void_p), ("lbox", c_double_p), ("fpairs", c_int32_p), ("l2w", c_double_p),
                ("tbox", c_double_p), ("wroot", c_int32_p), ("bcoord", c_double_p), ("inst_bounds", c_double_p),
                ("tri_prim", c_int32_p), ("tri_last", C.POINTER(C.c_uint8))]


class rt_work_counters(C.Structure):
    _fields_ = [("records_fetched", C.c_int64), ("tri_tests", C.c_int64), ("normal_fetches", C.c_int64),
                ("instance_entries", C.c_int64), ("pixels", C.c_int64),
                ("ref_node_fetches", C.c_int64), ("ref_tri_tests", C.c_int64),
                ("ref_smooth_hits", C.c_int64), ("ref_pixels", C.c_int64),
                ("lane_steps_closest", C.c_int64), ("wave_steps_closest", C.c_int64),
                ("lane_steps_shadow", C.c_int64), ("wave_steps_shadow", C.c_int64),
                ("divergent_lane_loads", C.c_int64), ("divergent_distinct_records", C.c_int64),
                ("iter_wave_inner", C.c_int64 * 2), ("iter_wave_leaf", C.c_int64 * 2),
                ("iter_wave_scalar", C.c_int64 * 2), ("iter_lane_inner", C.c_int64 * 2),
                ("iter_lane_leaf", C.c_int64 * 2)]


class rt_ply_mesh(C.Structure):
    _fields_ = [("positions", c_double_p), ("num_positions", C.c_int64),
                ("normals", c_double_p), ("num_normals", C.c_int64),
                ("texcoords", C.POINTER(C.c_float)), ("num_texcoords", C.c_int64),
                ("indices", c_int32_p), ("num_indices", C.c_int64)]


RT_PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32)

# status codes (rtcore.h)
RT_OK = 0
RT_ERR_INVALID_CAMERA = -10
RT_ERR_NO_SCENE = -20
RT_ERR_BUSY = -32
RT_MAX_IN_FLIGHT = 16
RT_ERR_NO_RENDERER = -21
RT_ERR_INVALID_ARG = -30
RT_ERR_UNSUPPORTED = -31
RT_ERR_PLY = -40
RT_ERR_SCENE_FILE = -41
RT_ERR_DEVICE = -50
RT_ERR_OOM = -51
RT_ERR_CANCELLED = -60
RT_ERR_STACK = -61

# ---- ray queries (rtcore.h "ray queries"; appended under ABI 5: detected by symbol) ----
RT_QUERY_DEVICE = 1
RT_HIT_VALID, RT_HIT_OUT_OF_BOUNDS, RT_HIT_NON_FINITE = 1, 2, 4


class rt_ray_batch(C.Structure):
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("tlimit", C.c_void_p), ("time", C.c_void_p)]


class rt_hit_batch(C.Structure):
    _fields_ = [("t", C.c_void_p), ("uv", C.c_void_p), ("ids", C.c_void_p), ("point", C.c_void_p),
                ("normal", C.c_void_p), ("flags", C.c_void_p)]


class rt_query_bounds(C.Structure):
    _fields_ = [("origin_reach", C.c_double), ("origin_coord", C.c_double), ("dir_norm", C.c_double)]


class rt_query_counts(C.Structure):
    _fields_ = [("rays", C.c_int64), ("hits", C.c_int64), ("out_of_bounds", C.c_int64), ("non_finite", C.c_int64),
                ("launches", C.c_int64), ("reduced", C.c_int32), ("walk", C.c_int32), ("bounds", rt_query_bounds)]


class rt_query_tables(C.Structure):
    _fields_ = [("tris", C.c_int64), ("instances", C.c_int64), ("face", c_int32_p), ("tri_object", c_int32_p),
                ("verts", c_double_p), ("inst_object", c_int32_p)]


QUERY_SYMBOLS = ["rt_query_closest", "rt_query_occluded", "rt_query_stats", "rt_debug_query_tables"]

# ---- first-hit buffers (rtcore.h "first-hit buffers"; appended under ABI 5: detected by symbol) ----
RT_GBUFFER_DEVICE, RT_GBUFFER_PIXEL_CENTRE, RT_GBUFFER_FRAME_LAYOUT = 1, 2, 4


class rt_gbuffer(C.Structure):
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("tmin", C.c_void_p), ("time", C.c_void_p),
                ("hits", rt_hit_batch)]


GBUFFER_SYMBOLS = ["rt_render_gbuffer"]

# ---- ray masks (rtcore.h "ray masks"; appended under ABI 5: detected by symbol) ----


class rt_ray_masks(C.Structure):
    _fields_ = [("per_ray", C.c_void_p), ("all", C.c_uint32), ("pad", C.c_uint32)]


MASK_SYMBOLS = ["rt_scene_set_instance_masks", "rt_scene_instance_mask", "rt_query_closest_masked",
                "rt_query_occluded_masked", "rt_render_gbuffer_masked"]

RT_MAT = {"": 0, "default": 0, "mirror": 1, "dielectric": 2, "conductor": 3}
RT_CAM_LOOKAT, RT_CAM_NEARPLANE = 0, 1
RT_OBJ_MESH, RT_OBJ_TRIANGLE, RT_OBJ_SPHERE, RT_OBJ_PLANE, RT_OBJ_MESH_INSTANCE = 0, 1, 2, 3, 4

# every symbol include/rtcore.h declares (tests check the .so exports them all)
EXPORTED_SYMBOLS = [
    "rt_scene_create", "rt_scene_destroy", "rt_scene_info_get", "rt_render", "rt_render_device",
    "rt_stats_collect", "rt_rows_for_chunks", "rt_render_device_counted", "rt_last_error", "rt_version",
    "rt_ply_load", "rt_ply_free", "rt_debug_bvh_hash", "rt_debug_host_build", "rt_debug_fit_build",
    "rt_debug_trace_rays", "rt_debug_occluded_rays", "rt_host_alloc", "rt_host_free", "rt_debug_wave_times",
    "rt_debug_rcp", "rt_render_submit", "rt_render_wait",
    "rt_render_ex", "rt_host_register", "rt_host_unregister",
    "rt_scene_file_load", "rt_scene_file_parse", "rt_scene_file_desc", "rt_scene_file_image_name",
    "rt_scene_file_last_error", "rt_scene_file_destroy", "rt_scene_set_option", "rt_scene_get_option",
    "rt_scene_set_unsafe_option",
    "rt_scene_create_ex", "rt_scene_instance_of_object", "rt_scene_set_instance_transform", "rt_scene_set_camera",
    "rt_scene_instance_bounds", "rt_scene_commit", "rt_debug_wide_build", "rt_debug_wide_read",
    "rt_scene_mesh_vertex_count", "rt_scene_set_mesh_positions", "rt_scene_last_deform_stats",
    "rt_query_closest", "rt_query_occluded", "rt_query_stats", "rt_debug_query_tables",
    "rt_scene_commit_ex", "rt_scene_last_rebuild_stats",
    *REBUILD_DETAIL_SYMBOLS,
    *VISIBILITY_SYMBOLS,
    *GBUFFER_SYMBOLS,
    *MASK_SYMBOLS,
]
RT_ABI_VERSION = 5


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restype to every exported function."""
    P = C.POINTER
    lib.rt_scene_create.argtypes = [P(rt_scene_desc), c_int32_p, C.c_int32, P(C.c_void_p)]
    lib.rt_scene_create.restype = C.c_int32
    lib.rt_scene_destroy.argtypes = [C.c_void_p]
    lib.rt_scene_destroy.restype = None
    lib.rt_scene_info_get.argtypes = [C.c_void_p, P(rt_scene_info)]
    lib.rt_scene_info_get.restype = C.c_int32
    lib.rt_render.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, P(C.c_uint8),
                              P(rt_stats), RT_PROGRESS_FN, C.c_void_p]
    lib.rt_render.restype = C.c_int32
    lib.rt_render_ex.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, P(C.c_uint8),
                                 C.c_uint32, P(rt_stats), RT_PROGRESS_FN, C.c_void_p]
    lib.rt_render_ex.restype = C.c_int32
    lib.rt_scene_file_load.argtypes = [C.c_char_p, C.c_int32, P(C.c_void_p)]
    lib.rt_scene_file_load.restype = C.c_int32
    lib.rt_scene_file_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_char_p, P(C.c_void_p)]
    lib.rt_scene_file_parse.restype = C.c_int32
    lib.rt_scene_file_desc.argtypes = [C.c_void_p]
    lib.rt_scene_file_desc.restype = P(rt_scene_desc)
    lib.rt_scene_file_image_name.argtypes = [C.c_void_p, C.c_int32]
    lib.rt_scene_file_image_name.restype = C.c_char_p
    lib.rt_scene_file_last_error.argtypes = []
    lib.rt_scene_file_last_error.restype = C.c_char_p
    lib.rt_scene_file_destroy.argtypes = [C.c_void_p]
    lib.rt_scene_file_destroy.restype = None
    lib.rt_host_register.argtypes = [C.c_void_p, C.c_uint64]
    lib.rt_host_register.restype = C.c_int32
    lib.rt_host_unregister.argtypes = [C.c_void_p]
    lib.rt_host_unregister.restype = C.c_int32
    lib.rt_render_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    lib.rt_render_device.restype = C.c_int32
    lib.rt_stats_collect.argtypes = [C.c_void_p, C.c_int32, P(rt_stats)]
    lib.rt_stats_collect.restype = C.c_int32
    lib.rt_rows_for_chunks.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.rt_rows_for_chunks.restype = C.c_int32
    lib.rt_render_device_counted.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, P(rt_work_counters)]
    lib.rt_render_device_counted.restype = C.c_int32
    lib.rt_last_error.argtypes = []
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_version.argtypes = []
    lib.rt_version.restype = C.c_char_p
    lib.rt_ply_load.argtypes = [C.c_char_p, P(rt_ply_mesh)]
    lib.rt_ply_load.restype = C.c_int32
    lib.rt_ply_free.argtypes = [P(rt_ply_mesh)]
    lib.rt_ply_free.restype = None
    lib.rt_host_alloc.argtypes = [C.c_uint64, P(C.c_void_p)]
    lib.rt_host_alloc.restype = C.c_int32
    lib.rt_host_free.argtypes = [C.c_void_p]
    lib.rt_host_free.restype = None
    lib.rt_debug_wave_times.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        P(C.c_uint64), C.c_int64, P(C.c_int64)]
    lib.rt_debug_wave_times.restype = C.c_int32
    lib.rt_debug_rcp.argtypes = [C.c_int32, c_double_p, c_double_p, c_double_p]
    lib.rt_debug_rcp.restype = C.c_int32
    lib.rt_render_submit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, C.POINTER(C.c_uint8),
                                     C.c_uint32, C.POINTER(C.c_int64)]
    lib.rt_render_submit.restype = C.c_int32
    lib.rt_render_wait.argtypes = [C.c_void_p, C.c_int64, C.POINTER(rt_stats)]
    lib.rt_render_wait.restype = C.c_int32
    lib.rt_debug_bvh_hash.argtypes = [C.c_void_p, C.c_int32]
    lib.rt_debug_bvh_hash.restype = C.c_uint64
    lib.rt_debug_host_build.argtypes = [P(rt_scene_desc), P(C.c_uint64), C.c_int32, c_int32_p, P(rt_scene_info)]
    lib.rt_debug_host_build.restype = C.c_int32
    if hasattr(lib, "rt_debug_fit_build"):   # round 6 (an older build may be loaded for an A/B, MYRT_LIB)
        lib.rt_debug_fit_build.argtypes = [P(rt_scene_desc), P(C.c_int64)]
        lib.rt_debug_fit_build.restype = C.c_int32
    if hasattr(lib, "rt_debug_wide_build"):   # the four-wide trees read back (an older build may be loaded, MYRT_LIB)
        lib.rt_debug_wide_build.argtypes = [P(rt_scene_desc), C.c_uint32, P(rt_wide_dump)]
        lib.rt_debug_wide_build.restype = C.c_int32
        lib.rt_debug_wide_read.argtypes = [C.c_void_p, C.c_int32, P(rt_wide_dump)]
        lib.rt_debug_wide_read.restype = C.c_int32
    lib.rt_debug_trace_rays.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p,
                                        c_double_p, c_double_p, c_double_p, c_double_p, c_int32_p]
    lib.rt_debug_trace_rays.restype = C.c_int32
    lib.rt_debug_occluded_rays.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p,
                                           c_double_p, P(C.c_uint8)]
    lib.rt_debug_occluded_rays.restype = C.c_int32
    if hasattr(lib, "rt_scene_set_option"):   # ABI >= 3 (an older build may be loaded for an A/B, MYRT_LIB)
        lib.rt_scene_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.rt_scene_set_option.restype = C.c_int32
        lib.rt_scene_get_option.argtypes = [C.c_void_p, C.c_char_p, P(C.c_int64)]
        lib.rt_scene_get_option.restype = C.c_int32
    if hasattr(lib, "rt_scene_set_unsafe_option"):   # ABI >= 4 (test hooks, not for production)
        lib.rt_scene_set_unsafe_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        lib.rt_scene_set_unsafe_option.restype = C.c_int32
    if hasattr(lib, "rt_scene_commit"):   # ABI >= 5 (dynamic scenes)
        lib.rt_scene_create_ex.argtypes = [P(rt_scene_desc), c_int32_p, C.c_int32, C.c_uint32, P(C.c_void_p)]
        lib.rt_scene_create_ex.restype = C.c_int32
        lib.rt_scene_instance_of_object.argtypes = [C.c_void_p, C.c_int32, c_int32_p]
        lib.rt_scene_instance_of_object.restype = C.c_int32
        lib.rt_scene_set_instance_transform.argtypes = [C.c_void_p, C.c_int32, c_double_p]
        lib.rt_scene_set_instance_transform.restype = C.c_int32
        lib.rt_scene_set_camera.argtypes = [C.c_void_p, C.c_int32, P(rt_camera)]
        lib.rt_scene_set_camera.restype = C.c_int32
        lib.rt_scene_instance_bounds.argtypes = [C.c_void_p, C.c_int32, c_double_p, c_double_p]
        lib.rt_scene_instance_bounds.restype = C.c_int32
        lib.rt_scene_commit.argtypes = [C.c_void_p, P(rt_commit_stats)]
        lib.rt_scene_commit.restype = C.c_int32
    if hasattr(lib, "rt_scene_set_mesh_positions"):   # deforming meshes (appended under ABI 5: detected by symbol)
        lib.rt_scene_mesh_vertex_count.argtypes = [C.c_void_p, C.c_int32, P(C.c_int64)]
        lib.rt_scene_mesh_vertex_count.restype = C.c_int32
        lib.rt_scene_set_mesh_positions.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32]
        lib.rt_scene_set_mesh_positions.restype = C.c_int32
        lib.rt_scene_last_deform_stats.argtypes = [C.c_void_p, P(rt_deform_stats)]
        lib.rt_scene_last_deform_stats.restype = C.c_int32
    if hasattr(lib, "rt_scene_commit_ex"):   # fit-tree rebuild (appended under ABI 5: detected by symbol)
        lib.rt_scene_commit_ex.argtypes = [C.c_void_p, C.c_uint32, P(rt_commit_stats)]
        lib.rt_scene_commit_ex.restype = C.c_int32
        lib.rt_scene_last_rebuild_stats.argtypes = [C.c_void_p, P(rt_rebuild_stats)]
        lib.rt_scene_last_rebuild_stats.restype = C.c_int32
    if hasattr(lib, "rt_scene_fit_cost"):   # clustered rebuild, detail, tree cost (appended under ABI 5: detected by symbol)
        lib.rt_scene_last_rebuild_detail.argtypes = [C.c_void_p, P(rt_rebuild_detail)]
        lib.rt_scene_last_rebuild_detail.restype = C.c_int32
        lib.rt_scene_fit_cost.argtypes = [C.c_void_p, c_double_p]
        lib.rt_scene_fit_cost.restype = C.c_int32
    if hasattr(lib, "rt_scene_set_instance_visible"):   # instance visibility (appended under ABI 5: detected by symbol)
        lib.rt_scene_set_instance_visible.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        lib.rt_scene_set_instance_visible.restype = C.c_int32
        lib.rt_scene_set_instances_visible.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P(C.c_uint8)]
        lib.rt_scene_set_instances_visible.restype = C.c_int32
        lib.rt_scene_instance_visible.argtypes = [C.c_void_p, C.c_int32, c_int32_p]
        lib.rt_scene_instance_visible.restype = C.c_int32
        lib.rt_scene_last_visibility_stats.argtypes = [C.c_void_p, P(rt_visibility_stats)]
        lib.rt_scene_last_visibility_stats.restype = C.c_int32
    if hasattr(lib, "rt_query_closest"):   # ray queries (appended under ABI 5: detected by symbol)
        lib.rt_query_closest.argtypes = [C.c_void_p, C.c_int32, C.c_int64, P(rt_ray_batch), P(rt_hit_batch),
                                         P(rt_query_bounds), C.c_uint32, C.c_void_p]
        lib.rt_query_closest.restype = C.c_int32
        lib.rt_query_occluded.argtypes = [C.c_void_p, C.c_int32, C.c_int64, P(rt_ray_batch), C.c_void_p,
                                          P(rt_query_bounds), C.c_uint32, C.c_void_p]
        lib.rt_query_occluded.restype = C.c_int32
        lib.rt_query_stats.argtypes = [C.c_void_p, C.c_int32, P(rt_query_counts)]
        lib.rt_query_stats.restype = C.c_int32
        lib.rt_debug_query_tables.argtypes = [P(rt_scene_desc), C.c_uint32, P(rt_query_tables)]
        lib.rt_debug_query_tables.restype = C.c_int32
    if hasattr(lib, "rt_render_gbuffer"):   # first-hit buffers (appended under ABI 5: detected by symbol)
        lib.rt_render_gbuffer.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(rt_gbuffer),
                                          C.c_uint32, C.c_void_p]
        lib.rt_render_gbuffer.restype = C.c_int32
    if hasattr(lib, "rt_scene_set_instance_masks"):   # ray masks (appended under ABI 5: detected by symbol)
        lib.rt_scene_set_instance_masks.argtypes = [C.c_void_p, C.c_int32, C.c_int32, P(C.c_uint32)]
        lib.rt_scene_set_instance_masks.restype = C.c_int32
        lib.rt_scene_instance_mask.argtypes = [C.c_void_p, C.c_int32, P(C.c_uint32)]
        lib.rt_scene_instance_mask.restype = C.c_int32
        lib.rt_query_closest_masked.argtypes = [C.c_void_p, C.c_int32, C.c_int64, P(rt_ray_batch), P(rt_hit_batch),
                                                P(rt_query_bounds), C.c_uint32, C.c_void_p, P(rt_ray_masks)]
        lib.rt_query_closest_masked.restype = C.c_int32
        lib.rt_query_occluded_masked.argtypes = [C.c_void_p, C.c_int32, C.c_int64, P(rt_ray_batch), C.c_void_p,
                                                 P(rt_query_bounds), C.c_uint32, C.c_void_p, P(rt_ray_masks)]
        lib.rt_query_occluded_masked.restype = C.c_int32
        lib.rt_render_gbuffer_masked.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(rt_gbuffer),
                                                 C.c_uint32, C.c_void_p, C.c_uint32]
        lib.rt_render_gbuffer_masked.restype = C.c_int32
    return lib
