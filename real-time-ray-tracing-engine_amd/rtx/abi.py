"""ctypes mirror of include/rt_api.h (the C ABI of the HIP hot path).

Field order and types must match the header exactly; tests/test_abi.py checks
sizes against the compiled library's own view (rt_abi_sizes) when available.
"""
import ctypes as C

RT_ABI_VERSION = 5  # include/rt_api.h; rtx/lib.py refuses a library of another version

RT_OK = 0
RT_ERR_INVALID = -1
RT_ERR_DEVICE = -2
RT_ERR_OOM = -3
RT_ERR_UNSUPPORTED = -4

RT_TEX_SOLID, RT_TEX_CHECKER, RT_TEX_NOISE = 0, 1, 2
RT_MAT_LAMBERTIAN, RT_MAT_METAL, RT_MAT_DIELECTRIC, RT_MAT_DIFFUSE_LIGHT, RT_MAT_ISOTROPIC = range(5)
RT_OBJ_SPHERE, RT_OBJ_QUAD, RT_OBJ_LIST, RT_OBJ_ROTATE_Y, RT_OBJ_TRANSLATE, RT_OBJ_MEDIUM = range(6)
RT_STORED_FORM = 2  # rt_object_desc.moving: sphere displacement / rotate_y (sin, cos) as stored
RT_OUT_SCALED, RT_OUT_SUM = 0, 1
RT_PERLIN_POINTS = 256


class Vec3(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("z", C.c_double)]

    @staticmethod
    def of(v):
        return Vec3(float(v[0]), float(v[1]), float(v[2]))

    def tolist(self):
        return [self.x, self.y, self.z]


class TextureDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("even", C.c_int32), ("odd", C.c_int32),
                ("perlin", C.c_int32), ("scale", C.c_double), ("color", Vec3)]


class PerlinDesc(C.Structure):
    _fields_ = [("rand_vec", Vec3 * RT_PERLIN_POINTS),
                ("perm_x", C.c_int32 * RT_PERLIN_POINTS),
                ("perm_y", C.c_int32 * RT_PERLIN_POINTS),
                ("perm_z", C.c_int32 * RT_PERLIN_POINTS)]


class MaterialDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texture", C.c_int32), ("albedo", Vec3),
                ("fuzz", C.c_double), ("refraction_index", C.c_double)]


class ObjectDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("child", C.c_int32),
                ("count", C.c_int32), ("a", Vec3), ("b", Vec3), ("c", Vec3),
                ("s", C.c_double), ("moving", C.c_int32), ("phase", C.c_int32)]


class SceneDesc(C.Structure):
    _fields_ = [("textures", C.POINTER(TextureDesc)), ("n_textures", C.c_int32),
                ("n_perlin", C.c_int32), ("perlin", C.POINTER(PerlinDesc)),
                ("materials", C.POINTER(MaterialDesc)), ("n_materials", C.c_int32),
                ("n_objects", C.c_int32), ("objects", C.POINTER(ObjectDesc)),
                ("children", C.POINTER(C.c_int32)), ("n_children", C.c_int32),
                ("world", C.c_int32), ("lights", C.c_int32), ("use_bvh", C.c_int32),
                ("bvh_builder", C.c_int32), ("bvh_arity", C.c_int32)]


RT_BVH_AUTO, RT_BVH_HOST, RT_BVH_DEVICE, RT_BVH_DEVICE_SAH = 0, 1, 2, 3
# kernel instance bits (rt_scene_info.features)
RT_FEAT_MEDIA, RT_FEAT_XFORM, RT_FEAT_LIGHTS, RT_FEAT_NOISE, RT_FEAT_FLAT, RT_FEAT_BVH4 = 1, 2, 4, 8, 16, 32
RT_FEAT_DIFFUSE = 64  # above the instance key: every material is Lambertian with a solid colour


class CameraDesc(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("samples_per_pixel", C.c_int32),
                ("max_depth", C.c_int32), ("_pad0", C.c_int32),
                ("aspect_ratio", C.c_double), ("vfov", C.c_double),
                ("defocus_angle", C.c_double), ("focus_dist", C.c_double),
                ("lookfrom", Vec3), ("lookat", Vec3), ("vup", Vec3), ("background", Vec3)]


class Frame(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32),
                ("sqrt_spp", C.c_int32), ("max_depth", C.c_int32),
                ("center", Vec3), ("pixel00_loc", Vec3), ("pixel_delta_u", Vec3),
                ("pixel_delta_v", Vec3), ("u", Vec3), ("v", Vec3), ("w", Vec3),
                ("defocus_disk_u", Vec3), ("defocus_disk_v", Vec3),
                ("defocus_angle", C.c_double), ("pixel_samples_scale", C.c_double),
                ("background", Vec3)]


class RenderParams(C.Structure):
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("sample_begin", C.c_int32), ("sample_count", C.c_int32),
                ("seed", C.c_uint64), ("output", C.c_int32), ("accumulate", C.c_int32),
                ("tile_first", C.c_int32), ("tile_stride", C.c_int32),
                ("layout", C.c_int32), ("strata_chunks", C.c_int32)]


RT_LAYOUT_FRAME, RT_LAYOUT_TILES = 0, 1
RT_GUIDE_CHANNELS = 8  # rt_render_guides_device: albedo r,g,b; normal x,y,z; depth; hits
RT_CHUNKS_AUTO = -1  # strata_chunks: the library's units for a tile subset, per-tile sums out


class PathStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "samples", "segments", "node_visits", "sphere_tests", "quad_tests",
        "other_tests", "light_tests", "shade_events",
        "wave_trips", "wave_node_iters", "wave_leaf_iters", "wave_shade_iters",
        "cyc_loop", "cyc_regen", "cyc_trace", "cyc_media", "cyc_shade", "cyc_lights",
        "model_trace_max", "model_trace_pair_max", "noise_evals", "wave_noise_iters",
        "medium_box_tests", "medium_box_deferred")]


class SceneInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_leaf_refs", C.c_int32),
                ("n_spheres", C.c_int32), ("n_quads", C.c_int32),
                ("n_objects", C.c_int32), ("n_light_leaves", C.c_int32),
                ("bvh_depth", C.c_int32), ("node_bytes", C.c_int32),
                ("sphere_bytes", C.c_int32), ("quad_bytes", C.c_int32),
                ("device_bytes", C.c_int64), ("features", C.c_int32), ("lds_nodes", C.c_int32),
                ("bvh_builder", C.c_int32), ("bvh_arity", C.c_int32),
                ("stack_depth", C.c_int32), ("lds_fixed_bytes", C.c_int32),
                ("lds_block_budget", C.c_int32), ("waves_per_simd", C.c_int32),
                ("lds_nodes_persistent", C.c_int32), ("lds_prims_persistent", C.c_int32),
                ("persistent_block_waves", C.c_int32), ("lds_perlin", C.c_int32),
                ("lds_node_bytes", C.c_int32)]


class Tuning(C.Structure):
    """rt_tuning: a scene's work-unit plan, LDS staging and BVH-builder
    overrides, passed at creation (zero-filled = the default plan)."""
    _fields_ = [("chunk_target", C.c_int32), ("head_strata", C.c_int32),
                ("tail_split", C.c_int32), ("no_uniform_tail", C.c_int32),
                ("no_persistent", C.c_int32), ("grid_cap", C.c_int32),
                ("tail_tiles", C.c_double),
                ("lds_nodes", C.c_int32), ("lds_nodes_pc", C.c_int32),
                ("no_lds_prims", C.c_int32), ("no_lds_perlin", C.c_int32),
                ("lds_cap", C.c_int32), ("pc_waves", C.c_int32),
                ("sah_stack_budget", C.c_int32), ("lbvh_max_depth", C.c_int32),
                ("sah_leaf_max", C.c_int32), ("sah_leaf_split", C.c_int32),
                ("sah_trav_x4", C.c_int32), ("sah_bins", C.c_int32),
                ("extra_features", C.c_int32),
                ("sub_head_strata", C.c_int32), ("sub_tail_split", C.c_int32),
                ("sub_tail_permille", C.c_int32), ("no_tile_order", C.c_int32),
                ("probe_strata", C.c_int32), ("reserved", C.c_int32 * 2)]


class DenoiseParams(C.Structure):
    """rt_denoise_params: zero-filled = every default (include/rt_api.h
    RT_DENOISE_*); a negative sigma switches its term off, passes < 0 the filter."""
    _fields_ = [("passes", C.c_int32), ("reserved", C.c_int32),
                ("sigma_normal", C.c_double), ("sigma_depth", C.c_double),
                ("sigma_hit", C.c_double), ("sigma_color", C.c_double)]


# include/rt_api.h RT_DENOISE_*: the shipped defaults (tests/test_denoise.py reads
# the header's values and compares)
RT_DENOISE_PASSES, RT_DENOISE_MAX_PASSES = 5, 8
RT_DENOISE_SIGMA_NORMAL, RT_DENOISE_SIGMA_DEPTH = 0.2, 0.01
RT_DENOISE_SIGMA_HIT, RT_DENOISE_SIGMA_COLOR = 0.1, 64.0


def denoise_params(p=None):
    """A DenoiseParams from None (the defaults), a DenoiseParams, or a dict of its fields."""
    if p is None or isinstance(p, DenoiseParams):
        return p
    out = DenoiseParams()
    for k, v in dict(p).items():
        if k not in dict(DenoiseParams._fields_):
            raise KeyError("unknown rt_denoise_params field %r" % k)
        setattr(out, k, v)
    return out


class DenoiseVarianceParams(C.Structure):
    """rt_denoise_variance_params: zero-filled = every default (include/rt_api.h
    RT_DENOISE_*); a negative sigma switches its term off, passes < 0 the
    filter; min_batches below 2 counts as 2."""
    _fields_ = [("passes", C.c_int32), ("min_batches", C.c_int32),
                ("sigma_normal", C.c_double), ("sigma_depth", C.c_double),
                ("sigma_hit", C.c_double), ("sigma_lum", C.c_double)]


# include/rt_api.h: the variance-guided filter's own defaults (tests/test_variance.py
# reads the header's values and compares)
RT_DENOISE_SIGMA_LUM, RT_DENOISE_MIN_BATCHES = 4.0, 4


def denoise_variance_params(p=None):
    """A DenoiseVarianceParams from None (the defaults), a DenoiseVarianceParams, or a dict of its fields."""
    if p is None or isinstance(p, DenoiseVarianceParams):
        return p
    out = DenoiseVarianceParams()
    for k, v in dict(p).items():
        if k not in dict(DenoiseVarianceParams._fields_):
            raise KeyError("unknown rt_denoise_variance_params field %r" % k)
        setattr(out, k, v)
    return out


class TemporalParams(C.Structure):
    """rt_temporal_params: zero-filled = every default (include/rt_api.h
    RT_TEMPORAL_*); a negative sigma switches its test off, a negative hit_min
    admits every pixel."""
    _fields_ = [("max_history", C.c_int32), ("reserved", C.c_int32),
                ("sigma_depth", C.c_double), ("sigma_normal", C.c_double), ("hit_min", C.c_double)]


# include/rt_api.h RT_TEMPORAL_*: the shipped defaults (tests/test_temporal.py
# reads the header's values and compares)
RT_TEMPORAL_MAX_HISTORY = 64
RT_TEMPORAL_SIGMA_DEPTH, RT_TEMPORAL_SIGMA_NORMAL, RT_TEMPORAL_HIT_MIN = 0.5, -1.0, 0.75


def temporal_params(p=None):
    """A TemporalParams from None (the defaults), a TemporalParams, or a dict of its fields."""
    if p is None or isinstance(p, TemporalParams):
        return p
    out = TemporalParams()
    for k, v in dict(p).items():
        if k not in dict(TemporalParams._fields_):
            raise KeyError("unknown rt_temporal_params field %r" % k)
        setattr(out, k, v)
    return out


# include/rt_api.h RT_GUIDED_*: the guided selection's defaults (tests/test_guided.py
# reads the header's values and compares)
RT_GUIDED_FLOOR, RT_GUIDED_MIN_COUNT = 1e-2, 8


class Ray(C.Structure):
    """rt_ray (64 B): t_max <= 0 or +inf: no limit; NaN: a miss."""
    _fields_ = [("origin", C.c_double * 3), ("direction", C.c_double * 3),
                ("time", C.c_double), ("t_max", C.c_double)]


class RayHit(C.Structure):
    """rt_ray_hit (72 B).  A miss: t = +inf, p = n = 0, object = chain_object =
    material = -1, front = 0."""
    _fields_ = [("t", C.c_double), ("p", C.c_double * 3), ("n", C.c_double * 3),
                ("object", C.c_int32), ("chain_object", C.c_int32),
                ("material", C.c_int32), ("front", C.c_int32)]


class Motion(C.Structure):
    """rt_motion (64 B).  A miss: d = dn = 0, t = +inf, object = chain_object = -1."""
    _fields_ = [("d", C.c_double * 3), ("dn", C.c_double * 3), ("t", C.c_double),
                ("object", C.c_int32), ("chain_object", C.c_int32)]


class RadianceParams(C.Structure):
    """rt_radiance_params (56 B)."""
    _fields_ = [("seed", C.c_uint64), ("first_key", C.c_uint32), ("first_sample", C.c_int32),
                ("samples", C.c_int32), ("max_depth", C.c_int32), ("accumulate", C.c_int32),
                ("_reserved", C.c_int32), ("background", Vec3)]


def tuning(t=None):
    """A Tuning from None (the default), a Tuning, or a dict of its fields."""
    if t is None or isinstance(t, Tuning):
        return t
    out = Tuning()
    for k, v in dict(t).items():
        if k not in dict(Tuning._fields_):
            raise KeyError("unknown rt_tuning field %r" % k)
        setattr(out, k, v)
    return out


# Every symbol include/rt_api.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_camera_setup",
    "rt_scene_create", "rt_scene_info_get", "rt_scene_destroy", "rt_render",
    "rt_render_device", "rt_render_stats", "rt_last_kernel_ms", "rt_to_bytes_device",
    "rt_multi_create", "rt_multi_render", "rt_multi_shard_ms", "rt_multi_destroy",
    "rt_scene_bvh_cost", "rt_tiles_sum_device", "rt_tiles_to_frame_device", "rt_multi_gather_ms",
    "rt_scene_create_tuned", "rt_multi_create_tuned",
    "rt_render_tiles_device", "rt_adaptive_update_device", "rt_adaptive_select_device",
    "rt_to_bytes_tiles_device",
    "rt_render_guides_device", "rt_denoise_workspace_bytes", "rt_denoise_device",
    "rt_history_bytes", "rt_temporal_device",
    "rt_denoise_variance_workspace_bytes", "rt_denoise_variance_device",
    "rt_history_variance_bytes", "rt_temporal_variance_device", "rt_denoise_given_variance_device",
    "rt_guided_select_device",
    "rt_scene_move_spheres", "rt_scene_move_spheres_device", "rt_multi_move_spheres",
    "rt_scene_rebuild_bvh", "rt_multi_rebuild_bvh",
    "rt_scene_set_transforms", "rt_scene_set_transforms_device", "rt_multi_set_transforms",
    "rt_scene_move_quads", "rt_scene_move_quads_device", "rt_multi_move_quads", "rt_rotate_y_sincos",
    "rt_trace_device", "rt_trace", "rt_multi_trace", "rt_pixel_ray",
    "rt_occluded_device", "rt_occluded", "rt_multi_occluded", "rt_segment_ray",
    "rt_radiance_device", "rt_radiance", "rt_multi_radiance", "rt_camera_rays",
    "rt_scene_pose_bytes", "rt_scene_pose_device", "rt_motion_device",
    "rt_temporal_motion_device", "rt_temporal_variance_motion_device",
)
