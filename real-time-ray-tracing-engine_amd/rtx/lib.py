"""Loader for the HIP hot-path library (build/librtx_hip.so, C ABI in include/rt_api.h).

There is no fallback: if the library is missing or a call fails, an exception
is raised.  Build with `make -C real-time-ray-tracing-engine_amd`.
"""
import ctypes as C
import os

from . import abi

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RTX_LIB", os.path.join(PKG_DIR, "build", "librtx_hip.so"))

_lib = None


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("HIP library %s is not built (run `make -C %s`)" % (LIB_PATH, PKG_DIR))
    # One HIP runtime per process: torch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7, found via libamdhip64.so), and whichever copy is loaded
    # first serves every later NEEDED libamdhip64.so.7.  Loading torch first makes
    # our library share torch's runtime (and so its streams, memory and RCCL).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.rt_abi_version.restype = C.c_int
    L.rt_last_error.restype = C.c_char_p
    L.rt_device_count.argtypes = [P(C.c_int32)]
    L.rt_camera_setup.argtypes = [P(abi.CameraDesc), P(abi.Frame)]
    L.rt_scene_create.argtypes = [P(abi.SceneDesc), C.c_int32, P(C.c_void_p)]
    L.rt_scene_create_tuned.argtypes = [P(abi.SceneDesc), C.c_int32, P(abi.Tuning), P(C.c_void_p)]
    L.rt_scene_info_get.argtypes = [C.c_void_p, P(abi.SceneInfo)]
    L.rt_scene_destroy.argtypes = [C.c_void_p]
    L.rt_render.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), P(C.c_double)]
    L.rt_render_device.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), C.c_void_p,
                                   C.c_void_p]
    L.rt_render_stats.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), P(abi.PathStats)]
    L.rt_last_kernel_ms.argtypes = [C.c_void_p, P(C.c_double)]
    L.rt_to_bytes_device.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
    L.rt_multi_create.argtypes = [P(abi.SceneDesc), P(C.c_int32), C.c_int32, C.c_int32,
                                  P(C.c_void_p)]
    L.rt_multi_create_tuned.argtypes = [P(abi.SceneDesc), P(C.c_int32), C.c_int32, C.c_int32,
                                        P(abi.Tuning), P(C.c_void_p)]
    L.rt_multi_render.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), P(C.c_double)]
    L.rt_multi_shard_ms.argtypes = [C.c_void_p, P(C.c_double)]
    L.rt_multi_destroy.argtypes = [C.c_void_p]
    L.rt_scene_bvh_cost.argtypes = [C.c_void_p, P(C.c_double)]
    L.rt_tiles_sum_device.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.rt_tiles_to_frame_device.argtypes = [C.c_void_p, C.c_int32, C.c_int64, P(abi.Frame),
                                           P(abi.RenderParams), C.c_void_p, C.c_void_p]
    L.rt_multi_gather_ms.argtypes = [C.c_void_p, P(C.c_double)]
    L.rt_render_tiles_device.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p]
    L.rt_adaptive_update_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, P(abi.Frame),
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_adaptive_select_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, P(abi.Frame),
                                            C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_to_bytes_tiles_device.argtypes = [C.c_void_p, C.c_void_p, P(abi.Frame), C.c_void_p, C.c_void_p]
    L.rt_render_guides_device.argtypes = [C.c_void_p, P(abi.Frame), P(abi.RenderParams), C.c_void_p,
                                          C.c_void_p]
    L.rt_denoise_workspace_bytes.argtypes = [P(abi.Frame), P(C.c_int64)]
    L.rt_denoise_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                    P(abi.DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_history_bytes.argtypes = [P(abi.Frame), P(C.c_int64)]
    L.rt_temporal_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_int32, P(abi.Frame), C.c_void_p, P(abi.TemporalParams), C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    L.rt_denoise_variance_workspace_bytes.argtypes = [P(abi.Frame), P(C.c_int64)]
    L.rt_denoise_variance_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                             P(abi.DenoiseVarianceParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]
    L.rt_history_variance_bytes.argtypes = [P(abi.Frame), P(C.c_int64)]
    L.rt_temporal_variance_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                              C.c_void_p, C.c_int32, P(abi.Frame), C.c_void_p, C.c_void_p,
                                              P(abi.TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    L.rt_scene_pose_bytes.argtypes = [C.c_void_p, P(C.c_int64)]
    L.rt_scene_pose_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_motion_device.argtypes = [C.c_void_p, P(abi.Frame), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_temporal_motion_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_int32, P(abi.Frame), C.c_void_p, C.c_void_p, P(abi.TemporalParams),
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_temporal_variance_motion_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                                     C.c_void_p, C.c_int32, P(abi.Frame), C.c_void_p, C.c_void_p,
                                                     C.c_void_p, P(abi.TemporalParams), C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p]
    L.rt_denoise_given_variance_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.c_void_p, P(abi.DenoiseVarianceParams),
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_guided_select_device.argtypes = [P(abi.Frame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double,
                                          C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_scene_move_spheres.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_double)]
    L.rt_scene_move_spheres_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_multi_move_spheres.argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_double)]
    L.rt_scene_rebuild_bvh.argtypes = [C.c_void_p, P(C.c_int32)]
    L.rt_multi_rebuild_bvh.argtypes = [C.c_void_p, P(C.c_int32)]
    for edit in ("set_transforms", "move_quads"):
        getattr(L, "rt_scene_" + edit).argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_double)]
        getattr(L, "rt_scene_" + edit + "_device").argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(L, "rt_multi_" + edit).argtypes = [C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_double)]
    L.rt_rotate_y_sincos.argtypes = [C.c_double, P(C.c_double), P(C.c_double)]
    L.rt_trace_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_trace.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.rt_multi_trace.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.rt_pixel_ray.argtypes = [P(abi.Frame), C.c_double, C.c_double, P(abi.Ray)]
    L.rt_occluded_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rt_occluded.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.rt_multi_occluded.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.rt_segment_ray.argtypes = [P(C.c_double), P(C.c_double), C.c_double, P(abi.Ray)]
    L.rt_radiance_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, P(abi.RadianceParams), C.c_void_p, C.c_void_p]
    L.rt_radiance.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, P(abi.RadianceParams), C.c_void_p]
    L.rt_multi_radiance.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, P(abi.RadianceParams), C.c_void_p]
    L.rt_camera_rays.argtypes = [P(abi.Frame), C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    for name in abi.EXPORTS:
        getattr(L, name).restype = C.c_char_p if name == "rt_last_error" else C.c_int
    if L.rt_abi_version() != abi.RT_ABI_VERSION:
        raise RuntimeError("rt ABI version mismatch: library %d, bindings %d"
                           % (L.rt_abi_version(), abi.RT_ABI_VERSION))
    _lib = L
    return L


def check(rc):
    if rc != abi.RT_OK:
        msg = load().rt_last_error()
        raise RtError(rc, msg.decode() if msg else "")
    return rc


def device_count():
    n = C.c_int32(0)
    rc = load().rt_device_count(C.byref(n))
    return n.value if rc == abi.RT_OK else 0
