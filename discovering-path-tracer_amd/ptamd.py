"""ptamd — Python binding of the MI355X path tracer's C ABI (include/pathtracer.h).

A thin ctypes layer over libptamd.so, mirroring the reference's host-side
objects: Scene (OBJ ingest + BVH, src/BoundingVolumeHierarchy.h), pack_light
(src/Light.cpp), default_camera (src/Camera.cpp) and Renderer — the
replacement for VulkanRayTracer's upload/dispatch/readback
(src/Vulkan/VulkanRayTracer.cpp).  There is no fallback: if the library is
missing or the GPU is absent, calls raise.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTAMD_LIB") or os.path.join(HERE, "libptamd.so")   # override: A/B of builds

PT_OK = 0
PT_NODES_INT_BITS = 0x1
PT_OPT_SCENE_IN_LDS = 1
PT_OPT_SAMPLE_LANES = 2
PT_OPT_FRESH_BATCH0 = 3
PT_OPT_KERNEL = 4
PT_OPT_SM_BATCH = 5
PT_OPT_PRIMARY_CULL = 6
PT_OPT_WF_PATHS = 7
PT_OPT_ITEM_ORDER = 8
PT_OPT_LAUNCH_TIMING = 9
PT_OPT_COUNT_TRACED = 10
PT_OPT_PAIRS = 11
PT_OPT_WIDE = 12
PT_OPT_WF_STREAMS = 13
PT_OPT_WIDE_BUILD = 14
PT_OPT_WF_FUSE = 15
PT_OPT_WIDE_NODE = 16
PT_OPT_WF_TAIL = 17
PT_OPT_GROUP_EXCHANGE = 18
PT_OPT_GROUP_CHECK = 19
PT_OPT_WF_GRID = 20
PT_OPT_WF_REFILL = 21
PT_OPT_MIXED_LANES = 22
PT_OPT_DENOISE_LDS = 23
PT_OPT_SMALL_SWEEP = 24
PT_OPT_CULL_TIGHT = 25
PT_OPT_SWEEP_HULL = 26
PT_OPT_MOMENTS = 27
PT_OPT_EXIT_SKIP = 28
PT_OPT_SEED_BASE = 29
PT_OPT_SWEEP_CUBE = 30
PT_OPT_ADAPTIVE_WF = 31
PT_OPT_RAYS_REFILL = 32
PT_OPT_CULL_FOOTPRINT = 33
PT_OPT_RADIANCE_CHUNK = 34
RAYS_CLOSEST, RAYS_ANY = 0, 1
# pt_ray and pt_hit as numpy sees them (32 B each)
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("limit", "<f4"), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("tri", "<i4"), ("u", "<f4"), ("v", "<f4"), ("n", "<f4", 3), ("reserved", "<u4")])
KERNEL_AUTO, KERNEL_RECURSIVE, KERNEL_WAVEFRONT = 0, 1, 3   # 2 (lane state machine) was removed

# Every symbol include/pathtracer.h declares (tests check the .so exports them).
EXPORTS = [
    "pt_abi_version", "pt_last_error", "pt_create", "pt_destroy", "pt_set_stream", "pt_synchronize",
    "pt_upload_scene", "pt_upload_lights", "pt_set_camera", "pt_set_params", "pt_resize_and_clear",
    "pt_bind_accum", "pt_clear_accum", "pt_accum_device_ptr", "pt_read_accum", "pt_dispatch", "pt_render",
    "pt_set_partition", "pt_tiles_owned", "pt_tiles_pack", "pt_tiles_unpack", "pt_set_option", "pt_last_kernel", "pt_set_stats_mode", "pt_get_stats", "pt_reset_stats", "pt_last_launch_ms",
    "pt_launch_times_ms", "pt_reset_launch_times", "pt_selftest_math", "pt_selftest_exhaustive",
    "pt_scene_load_obj", "pt_scene_parse_obj", "pt_scene_from_arrays", "pt_scene_build_bvh",
    "pt_scene_counts", "pt_scene_copy", "pt_scene_upload", "pt_scene_free", "pt_pack_light",
    "pt_default_camera", "pt_primary_cull_rects", "pt_primary_cull_rects_r", "pt_scene_save", "pt_scene_load_cache",
    "pt_progressive_camera", "pt_progressive_advance", "pt_readback_begin", "pt_readback_end", "pt_write_image",
    "pt_items_live", "pt_items_pack", "pt_items_unpack_all", "pt_render_packed", "pt_launch_span_ms",
    "pt_set_partition_slots", "pt_get_traced", "pt_wide_info", "pt_partition_items",
    "pt_dist_unique_id", "pt_dist_init", "pt_dist_run", "pt_dist_slot_floats", "pt_dist_finalize",
    "pt_dist_set_streams", "pt_dist_wait", "pt_dist_abort", "pt_create_multi", "pt_group_info",
    "pt_group_check", "pt_dist_info", "pt_mixed_info", "pt_sweep_info", "pt_sweep_walk",
    "pt_primary_cull_footprints", "pt_primary_cull_sure", "pt_cull_info",
    "pt_denoise_default_params", "pt_guide_ray", "pt_render_guide", "pt_guide_device_ptr", "pt_read_guide",
    "pt_denoise", "pt_read_denoised", "pt_denoise_host",
    "pt_moments_device_ptr", "pt_read_moments", "pt_denoise_var_default_params", "pt_denoise_var",
    "pt_denoise_var_host", "pt_denoise_var_plane_host",
    "pt_temporal_default_params", "pt_reproject", "pt_reproject_host", "pt_temporal_advance", "pt_temporal_reset",
    "pt_temporal_info", "pt_temporal_device_ptr", "pt_read_temporal", "pt_temporal_denoise",
    "pt_spatial_var_default_params", "pt_spatial_variance_host", "pt_spatial_variance", "pt_temporal_denoise_spatial",
    "pt_adaptive_default_params", "pt_adaptive_select_host", "pt_adaptive_select", "pt_adaptive_begin",
    "pt_adaptive_advance", "pt_adaptive_info", "pt_adaptive_read_counts", "pt_adaptive_read_live",
    "pt_adaptive_device_ptr", "pt_adaptive_denoise",
    "pt_display_default_params", "pt_display", "pt_display_device_ptr", "pt_read_display", "pt_display_exposure",
    "pt_display_reset", "pt_display_readback_begin", "pt_display_readback_end", "pt_display_host", "pt_write_png8",
    "pt_trace_rays", "pt_trace_rays_sync", "pt_trace_rays_host",
    "pt_upsample_default_params", "pt_upsample_host", "pt_upsample_images", "pt_upsample", "pt_upsampled_device_ptr",
    "pt_read_upsampled", "pt_upsample_guide_device_ptr", "pt_upsample_info", "pt_upsample_display",
    "pt_display_upsampled_device_ptr", "pt_read_display_upsampled",
    "pt_radiance_default_params", "pt_trace_radiance", "pt_trace_radiance_sync", "pt_trace_radiance_host",
    "pt_camera_rays", "pt_camera_rays_host",
]


class PTError(RuntimeError):
    pass


class Params(ctypes.Structure):
    _fields_ = [("max_depth", ctypes.c_int), ("sss_bounces", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("leaf_tests", ctypes.c_uint64),
                ("samples", ctypes.c_uint64)]


class Traced(ctypes.Structure):
    _fields_ = [("closest_walks", ctypes.c_uint64), ("shadow_walks", ctypes.c_uint64), ("nodes", ctypes.c_uint64),
                ("tri_tests", ctypes.c_uint64), ("primaries", ctypes.c_uint64)]


class DenoiseParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_depth", ctypes.c_float)]


class DenoiseVarParams(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int), ("sigma_lum", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_depth", ctypes.c_float)]


class TemporalParams(ctypes.Structure):
    _fields_ = [("max_history", ctypes.c_uint32), ("alpha_min", ctypes.c_float), ("normal_min", ctypes.c_float),
                ("depth_rel", ctypes.c_float)]


class SpatialVarParams(ctypes.Structure):
    _fields_ = [("below", ctypes.c_uint32), ("radius", ctypes.c_int), ("sigma_normal", ctypes.c_float),
                ("sigma_depth", ctypes.c_float)]


class AdaptiveParams(ctypes.Structure):
    _fields_ = [("min_batches", ctypes.c_uint32), ("max_batches", ctypes.c_uint32), ("step", ctypes.c_uint32),
                ("threshold", ctypes.c_float), ("lum_floor", ctypes.c_float)]


class DisplayParams(ctypes.Structure):
    _fields_ = [("tonemap", ctypes.c_int), ("exposure", ctypes.c_float), ("auto_exposure", ctypes.c_int),
                ("key", ctypes.c_float), ("white", ctypes.c_float), ("adapt", ctypes.c_float)]


TONEMAP_CLAMP, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2


class UpsampleParams(ctypes.Structure):
    _fields_ = [("scale", ctypes.c_int), ("sigma_normal", ctypes.c_float), ("sigma_depth", ctypes.c_float)]


class RadianceParams(ctypes.Structure):
    _fields_ = [("n_samples", ctypes.c_uint32), ("seed_stride", ctypes.c_uint32)]


class ReprojectImages(ctypes.Structure):
    """pt_reproject_images: device pointers for pt_reproject, host pointers
    for pt_reproject_host."""
    _fields_ = [(k, ctypes.c_void_p) for k in (
        "color", "moments", "guide", "hist_color", "hist_moments", "hist_length", "hist_guide",
        "out_color", "out_moments", "out_length", "out_variance")]


_lib = None


def lib():
    """Load libptamd.so (build it with `make -C discovering-path-tracer_amd`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PTError(f"{LIB_PATH} not built; run __graft_entry__.build() or make -C {HERE}")
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
        psz = ctypes.POINTER(sz)
        sig = {
            "pt_abi_version": ([], i32), "pt_last_error": ([], ctypes.c_char_p),
            "pt_create": ([i32, ctypes.POINTER(vp)], i32), "pt_destroy": ([vp], i32),
            "pt_create_multi": ([vp, i32, ctypes.POINTER(vp)], i32),
            "pt_group_info": ([vp, ctypes.POINTER(i32), vp, i32, ctypes.POINTER(i32)], i32),
            "pt_group_check": ([vp, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_float),
                                ctypes.POINTER(ctypes.c_float)], i32),
            "pt_dist_info": ([vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
            "pt_set_stream": ([vp, vp], i32), "pt_synchronize": ([vp], i32),
            "pt_upload_scene": ([vp, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, u32], i32),
            "pt_upload_lights": ([vp, vp, sz], i32), "pt_set_camera": ([vp, vp], i32),
            "pt_set_params": ([vp, ctypes.POINTER(Params)], i32),
            "pt_resize_and_clear": ([vp, i32, i32], i32), "pt_bind_accum": ([vp, vp, i32, i32], i32),
            "pt_clear_accum": ([vp], i32), "pt_accum_device_ptr": ([vp], vp),
            "pt_read_accum": ([vp, vp, sz], i32), "pt_dispatch": ([vp, u32], i32),
            "pt_render": ([vp, u32, u32], i32), "pt_set_partition": ([vp, i32, i32], i32),
            "pt_set_partition_slots": ([vp, i32, i32, vp], i32),
            "pt_set_stats_mode": ([vp, i32], i32), "pt_set_option": ([vp, i32, i32], i32), "pt_last_kernel": ([vp, ctypes.POINTER(ctypes.c_int)], i32),
            "pt_tiles_owned": ([vp, ctypes.POINTER(i32)], i32), "pt_tiles_pack": ([vp, vp], i32),
            "pt_tiles_unpack": ([vp, vp, i32, vp], i32), "pt_get_stats": ([vp, ctypes.POINTER(Stats)], i32),
            "pt_reset_stats": ([vp], i32), "pt_get_traced": ([vp, ctypes.POINTER(Traced)], i32),
            "pt_wide_info": ([vp, ctypes.POINTER(ctypes.c_int)], i32),
            "pt_mixed_info": ([vp, ctypes.POINTER(ctypes.c_int)], i32),
            "pt_sweep_info": ([vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], i32),
            "pt_sweep_walk": ([vp, ctypes.POINTER(ctypes.c_int)], i32),
            "pt_cull_info": ([vp, vp], i32),
            "pt_primary_cull_footprints": ([vp, i32, i32, vp, vp, vp, i32, ctypes.c_double, vp, i32,
                                            ctypes.POINTER(i32)], i32),
            "pt_primary_cull_sure": ([vp, i32, i32, vp, vp, vp, i32, ctypes.c_double, vp, i32, ctypes.POINTER(i32)], i32),
            "pt_partition_items": ([i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, psz, vp, psz, vp], i32),
            "pt_dist_unique_id": ([vp, sz], i32), "pt_dist_init": ([vp, vp, i32, i32], i32),
            "pt_dist_run": ([vp, u32, i32, i32, vp, i32], i32), "pt_dist_slot_floats": ([vp, psz], i32),
            "pt_dist_finalize": ([vp], i32), "pt_dist_set_streams": ([vp, vp, vp, vp], i32),
            "pt_dist_wait": ([vp, i32], i32), "pt_dist_abort": ([vp], i32), "pt_last_launch_ms": ([vp, ctypes.POINTER(ctypes.c_float)], i32),
            "pt_launch_times_ms": ([vp, vp, sz, psz], i32), "pt_reset_launch_times": ([vp], i32),
            "pt_launch_span_ms": ([vp, ctypes.POINTER(ctypes.c_float), psz], i32),
            "pt_selftest_math": ([i32, i32, vp, vp, sz], i32),
            "pt_selftest_exhaustive": ([i32, i32, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(u32)], i32),
            "pt_scene_load_obj": ([ctypes.c_char_p, ctypes.POINTER(vp)], i32),
            "pt_scene_parse_obj": ([ctypes.c_char_p, sz, ctypes.POINTER(vp)], i32),
            "pt_scene_from_arrays": ([vp, sz, vp, sz, ctypes.POINTER(vp)], i32),
            "pt_scene_build_bvh": ([vp, u32, i32], i32),
            "pt_scene_counts": ([vp, psz, psz, psz, psz, psz], i32),
            "pt_scene_copy": ([vp, vp, vp, vp, vp, vp], i32), "pt_scene_upload": ([vp, vp], i32),
            "pt_scene_free": ([vp], i32), "pt_pack_light": ([vp, vp, vp, vp, vp], i32),
            "pt_default_camera": ([vp], i32),
            "pt_primary_cull_rects": ([vp, i32, i32, vp, vp, vp, i32, vp, i32, ctypes.POINTER(i32)], i32),
            "pt_primary_cull_rects_r": ([vp, i32, i32, vp, vp, vp, i32, ctypes.c_double, vp, i32, ctypes.POINTER(i32),
                                         ctypes.POINTER(ctypes.c_float)], i32),
            "pt_scene_save": ([vp, ctypes.c_char_p], i32),
            "pt_progressive_camera": ([vp, vp, ctypes.POINTER(i32)], i32),
            "pt_progressive_advance": ([vp, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
            "pt_readback_begin": ([vp, ctypes.POINTER(i32)], i32),
            "pt_readback_end": ([vp, i32, vp, sz], i32),
            "pt_write_image": ([ctypes.c_char_p, vp, i32, i32, i32], i32),
            "pt_items_live": ([vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
            "pt_items_pack": ([vp, vp], i32),
            "pt_items_unpack_all": ([vp, vp, sz, vp], i32),
            "pt_render_packed": ([vp, u32, vp, vp, sz, vp], i32),
            "pt_scene_load_cache": ([ctypes.c_char_p, ctypes.POINTER(vp)], i32),
            "pt_denoise_default_params": ([ctypes.POINTER(DenoiseParams)], i32),
            "pt_guide_ray": ([vp, i32, i32, i32, i32, vp, vp], i32),
            "pt_render_guide": ([vp], i32), "pt_guide_device_ptr": ([vp], vp),
            "pt_read_guide": ([vp, vp, sz], i32),
            "pt_denoise": ([vp, ctypes.POINTER(DenoiseParams), vp, vp], i32),
            "pt_read_denoised": ([vp, vp, sz], i32),
            "pt_denoise_host": ([vp, vp, i32, i32, ctypes.POINTER(DenoiseParams), vp], i32),
            "pt_moments_device_ptr": ([vp], vp),
            "pt_read_moments": ([vp, vp, sz, ctypes.POINTER(u32)], i32),
            "pt_denoise_var_default_params": ([ctypes.POINTER(DenoiseVarParams)], i32),
            "pt_denoise_var": ([vp, ctypes.POINTER(DenoiseVarParams), vp], i32),
            "pt_denoise_var_host": ([vp, vp, u32, vp, i32, i32, ctypes.POINTER(DenoiseVarParams), vp], i32),
            "pt_denoise_var_plane_host": ([vp, vp, vp, i32, i32, ctypes.POINTER(DenoiseVarParams), vp], i32),
            "pt_temporal_default_params": ([ctypes.POINTER(TemporalParams)], i32),
            "pt_reproject": ([vp, vp, vp, i32, i32, u32, ctypes.POINTER(ReprojectImages),
                              ctypes.POINTER(TemporalParams)], i32),
            "pt_reproject_host": ([vp, vp, i32, i32, u32, ctypes.POINTER(ReprojectImages),
                                   ctypes.POINTER(TemporalParams)], i32),
            "pt_temporal_advance": ([vp, vp, u32], i32), "pt_temporal_reset": ([vp], i32),
            "pt_temporal_info": ([vp, ctypes.POINTER(u32), ctypes.POINTER(u32)], i32),
            "pt_temporal_device_ptr": ([vp, i32], vp), "pt_read_temporal": ([vp, vp, vp, vp], i32),
            "pt_temporal_denoise": ([vp, ctypes.POINTER(DenoiseVarParams), vp], i32),
            "pt_spatial_var_default_params": ([ctypes.POINTER(SpatialVarParams)], i32),
            "pt_spatial_variance_host": ([vp, vp, vp, vp, i32, i32, ctypes.POINTER(SpatialVarParams), vp], i32),
            "pt_spatial_variance": ([vp, vp, vp, vp, vp, i32, i32, ctypes.POINTER(SpatialVarParams), vp], i32),
            "pt_temporal_denoise_spatial": ([vp, ctypes.POINTER(DenoiseVarParams), ctypes.POINTER(SpatialVarParams),
                                             vp], i32),
            "pt_adaptive_default_params": ([ctypes.POINTER(AdaptiveParams)], i32),
            "pt_adaptive_select_host": ([vp, vp, i32, i32, ctypes.POINTER(AdaptiveParams), vp, vp], i32),
            "pt_adaptive_select": ([vp, vp, vp, i32, i32, ctypes.POINTER(AdaptiveParams), vp, vp], i32),
            "pt_adaptive_begin": ([vp, ctypes.POINTER(AdaptiveParams)], i32),
            "pt_adaptive_advance": ([vp, u32], i32),
            "pt_adaptive_info": ([vp, ctypes.POINTER(u32), ctypes.POINTER(u32),
                                  ctypes.POINTER(ctypes.c_ulonglong)], i32),
            "pt_adaptive_read_counts": ([vp, vp, vp, sz], i32),
            "pt_adaptive_read_live": ([vp, vp, sz, ctypes.POINTER(u32)], i32),
            "pt_adaptive_device_ptr": ([vp, i32], vp),
            "pt_adaptive_denoise": ([vp, ctypes.POINTER(DenoiseVarParams), vp], i32),
            "pt_display_default_params": ([ctypes.POINTER(DisplayParams)], i32),
            "pt_display": ([vp, ctypes.POINTER(DisplayParams), vp, vp], i32),
            "pt_display_device_ptr": ([vp], vp), "pt_read_display": ([vp, vp, sz], i32),
            "pt_display_exposure": ([vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(u32)], i32),
            "pt_display_reset": ([vp], i32),
            "pt_display_readback_begin": ([vp, ctypes.POINTER(DisplayParams), vp, ctypes.POINTER(i32)], i32),
            "pt_display_readback_end": ([vp, i32, vp, sz], i32),
            "pt_display_host": ([vp, i32, i32, ctypes.POINTER(DisplayParams), ctypes.POINTER(ctypes.c_float), vp], i32),
            "pt_write_png8": ([ctypes.c_char_p, vp, i32, i32], i32),
            "pt_trace_rays": ([vp, i32, vp, sz, vp], i32), "pt_trace_rays_sync": ([vp, i32, vp, sz, vp], i32),
            "pt_trace_rays_host": ([vp, sz, vp, sz, vp, sz, u32, i32, vp, sz, vp, i32], i32),
            "pt_upsample_default_params": ([ctypes.POINTER(UpsampleParams)], i32),
            "pt_upsample_host": ([vp, i32, i32, vp, ctypes.POINTER(UpsampleParams), vp], i32),
            "pt_upsample_images": ([vp, ctypes.POINTER(UpsampleParams), vp, i32, i32, vp, vp], i32),
            "pt_upsample": ([vp, ctypes.POINTER(UpsampleParams), vp, vp], i32),
            "pt_upsampled_device_ptr": ([vp], vp), "pt_read_upsampled": ([vp, vp, sz], i32),
            "pt_upsample_guide_device_ptr": ([vp], vp), "pt_upsample_info": ([vp, ctypes.POINTER(i32)], i32),
            "pt_upsample_display": ([vp, ctypes.POINTER(UpsampleParams), ctypes.POINTER(DisplayParams), vp, vp], i32),
            "pt_display_upsampled_device_ptr": ([vp], vp), "pt_read_display_upsampled": ([vp, vp, sz], i32),
            "pt_radiance_default_params": ([ctypes.POINTER(RadianceParams)], i32),
            "pt_trace_radiance": ([vp, ctypes.POINTER(RadianceParams), vp, sz, vp], i32),
            "pt_trace_radiance_sync": ([vp, ctypes.POINTER(RadianceParams), vp, sz, vp], i32),
            "pt_trace_radiance_host": ([vp, sz, vp, sz, vp, sz, u32, vp, sz, i32, i32, ctypes.POINTER(RadianceParams),
                                        vp, sz, vp, i32], i32),
            "pt_camera_rays": ([vp, u32, vp, sz, vp], i32),
            "pt_camera_rays_host": ([vp, i32, i32, u32, vp, sz, vp], i32),
        }
        for name, (args, res) in sig.items():
            if not hasattr(L, name):   # older library (A/B timing); calls to it fail loudly
                continue
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _lib = L
    return _lib


def _check(rc, what):
    if rc != PT_OK:
        raise PTError(f"{what} failed ({rc}): {lib().pt_last_error().decode()}")


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class Scene:
    """OBJ (or raw arrays) + BVH, built by the native host layer."""

    def __init__(self, handle):
        self._h = ctypes.c_void_p(handle) if not isinstance(handle, ctypes.c_void_p) else handle

    @classmethod
    def load_obj(cls, path):
        h = ctypes.c_void_p()
        _check(lib().pt_scene_load_obj(path.encode(), ctypes.byref(h)), "pt_scene_load_obj")
        return cls(h)

    @classmethod
    def parse_obj(cls, text: bytes):
        h = ctypes.c_void_p()
        _check(lib().pt_scene_parse_obj(text, len(text), ctypes.byref(h)), "pt_scene_parse_obj")
        return cls(h)

    @classmethod
    def from_arrays(cls, vertices, indices):
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        h = ctypes.c_void_p()
        _check(lib().pt_scene_from_arrays(_ptr(v), v.size, _ptr(i), i.size, ctypes.byref(h)), "pt_scene_from_arrays")
        return cls(h)

    @classmethod
    def load_cache(cls, path):
        """pt_scene_load_cache: a scene written by save() (BVH included)."""
        h = ctypes.c_void_p()
        _check(lib().pt_scene_load_cache(str(path).encode(), ctypes.byref(h)), "pt_scene_load_cache")
        return cls(h)

    def save(self, path):
        _check(lib().pt_scene_save(self._h, str(path).encode()), "pt_scene_save")
        return self

    def build_bvh(self, int_bits=False, threads=0):
        self.int_bits = int_bits
        _check(lib().pt_scene_build_bvh(self._h, PT_NODES_INT_BITS if int_bits else 0, threads), "pt_scene_build_bvh")
        return self

    def counts(self):
        c = [ctypes.c_size_t() for _ in range(5)]
        _check(lib().pt_scene_counts(self._h, *[ctypes.byref(x) for x in c]), "pt_scene_counts")
        return tuple(x.value for x in c)

    def arrays(self):
        """(vertices, indices [BVH order once built], nodes (N,8) float32, uvs, mat_indices)."""
        nvf, ni, nn, nuv, nmat = self.counts()
        v = np.zeros(nvf, np.float32)
        i = np.zeros(ni, np.uint32)
        n = np.zeros((nn, 8), np.float32)
        uv = np.zeros(nuv, np.float32)
        m = np.zeros(nmat, np.uint32)
        _check(lib().pt_scene_copy(self._h, _ptr(v), _ptr(i), _ptr(n), _ptr(uv), _ptr(m)), "pt_scene_copy")
        return v, i, n, uv, m

    def close(self):
        if self._h:
            lib().pt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_light(position, normal, intensity, size):
    """Light::packData (src/Light.cpp:16-33) -> 16 float32."""
    out = np.zeros(16, np.float32)
    args = [np.ascontiguousarray(a, np.float32) for a in (position, normal, intensity, size)]
    _check(lib().pt_pack_light(*[a.ctypes.data for a in args], out.ctypes.data), "pt_pack_light")
    return out


def reference_light():
    """The scene light of VulkanRayTracer.cpp:149-162."""
    return pack_light([0, 2, 0], [0, -1, 0], [10, 10, 10], [2.5, 2.5])


def device_math(fn, x, device=0):
    """Evaluate the kernel's math function `fn` on the GPU (pt_selftest_math)."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    _check(lib().pt_selftest_math(device, fn, x.ctypes.data, y.ctypes.data, x.size), "pt_selftest_math")
    return y


def device_math_exhaustive(fn, device=0):
    """pt_selftest_exhaustive: (mismatching inputs, smallest such bit pattern)
    of the device's fast-quotient fn (0 rcp, 1 log, 2 exp, 3 acos)
    against its IEEE definition over all 2^32 inputs; 4 sqrt, 5 rcp and
    7 x / 1.5f check the unguarded fast form wherever its range predicate
    holds, 6 sincos against sin and cos."""
    bad = ctypes.c_ulonglong(0)
    first = ctypes.c_uint32(0)
    _check(lib().pt_selftest_exhaustive(device, fn, ctypes.byref(bad), ctypes.byref(first)),
           "pt_selftest_exhaustive")
    return bad.value, first.value


def partition_slot_positions(nranks, rank, slots=None):
    """(m, positions) of rank's slots in a period of the slotted partition
    (pt_api.cpp part_of): slots ordered by (k + 1/2) / slots[r] for each
    rank's k-th slot, ties by rank."""
    s = [1] * nranks if slots is None else [int(x) for x in slots]
    seq = sorted(((k + 0.5) / s[r], r) for r in range(nranks) for k in range(s[r]))
    return len(seq), [v for v, (_, r) in enumerate(seq) if r == rank]


def partition_owned(width, height, nranks, rank, slots=None):
    """Pixels a rank renders under pt_set_partition(_slots): 16x16 blocks,
    block (bx, by) is tile b = by*blocks_x + (bx - by) mod blocks_x (rows
    rotated); the rank owns tile b iff b % m is one of its slot positions
    (partition_slot_positions; one slot per rank: b % nranks == rank).
    Returns a (H, W) bool mask."""
    m, pos = partition_slot_positions(nranks, rank, slots)
    nbx = (width + 15) // 16
    ys, xs = np.mgrid[0:height, 0:width]
    by, bx = ys // 16, xs // 16
    return np.isin((by * nbx + (bx - by) % nbx) % m, pos)


def partition_items(width, height, sample_lanes, nranks, rank, slots=None, cull_rects=None, item_order=1):
    """pt_partition_items: the product's item tables for `rank` (host only).
    Returns (live, culled, pixel_of) -- live and culled item ids in launch /
    table order, and pixel_of[(len(live) + len(culled)), 256 // sample_lanes]
    with the pixel index y*W+x of each item slot (-1 past the frame edge)."""
    sl = None if slots is None else np.ascontiguousarray(slots, np.int32)
    if cull_rects is None:
        cr, nc = None, -1
    else:
        cr = np.ascontiguousarray(cull_rects, np.float32).reshape(-1, 4)
        nc = cr.shape[0]
    nl, nu = ctypes.c_size_t(0), ctypes.c_size_t(0)
    args = (width, height, sample_lanes, nranks, rank, None if sl is None else sl.ctypes.data,
            None if cr is None else cr.ctypes.data, nc, item_order)
    _check(lib().pt_partition_items(*args, None, ctypes.byref(nl), None, ctypes.byref(nu), None), "pt_partition_items")
    live = np.zeros(max(nl.value, 1), np.int32)
    culled = np.zeros(max(nu.value, 1), np.int32)
    per = 256 // sample_lanes
    pix = np.zeros(max((nl.value + nu.value) * per, 1), np.int32)
    _check(lib().pt_partition_items(*args, live.ctypes.data, ctypes.byref(nl), culled.ctypes.data, ctypes.byref(nu),
                                    pix.ctypes.data), "pt_partition_items")
    return live[:nl.value], culled[:nu.value], pix[:(nl.value + nu.value) * per].reshape(-1, per)


def primary_cull_rects(camera_ubo, width, height, root_min, root_max, lights16, max_rects=8):
    """pt_primary_cull_rects: NDC rectangles {x0,x1,y0,y1} outside which no
    primary ray reaches the root box or a light; None when not derivable."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(16)
    lo = np.ascontiguousarray(root_min, np.float32).reshape(3)
    hi = np.ascontiguousarray(root_max, np.float32).reshape(3)
    l = np.ascontiguousarray(lights16, np.float32).reshape(-1)
    out = np.zeros((max_rects, 4), np.float32)
    n = ctypes.c_int(0)
    _check(lib().pt_primary_cull_rects(cam.ctypes.data, width, height, lo.ctypes.data, hi.ctypes.data,
                                       l.ctypes.data if l.size else None, l.size // 16, out.ctypes.data,
                                       max_rects, ctypes.byref(n)), "pt_primary_cull_rects")
    return None if n.value < 0 else out[:n.value].copy()


def primary_cull_rects_r(camera_ubo, width, height, root_min, root_max, lights16, radius_bound=-1.0, max_rects=8):
    """pt_primary_cull_rects_r: (rectangles or None, u0) -- the rectangles
    outside which no primary ray whose two Box-Muller radii are at most
    radius_bound (negative: the kernel's tight bound) reaches the root box or
    a light, and the kernel's threshold on the radius draws."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(16)
    lo = np.ascontiguousarray(root_min, np.float32).reshape(3)
    hi = np.ascontiguousarray(root_max, np.float32).reshape(3)
    l = np.ascontiguousarray(lights16, np.float32).reshape(-1)
    out = np.zeros((max_rects, 4), np.float32)
    n = ctypes.c_int(0)
    u0 = ctypes.c_float(0.0)
    _check(lib().pt_primary_cull_rects_r(cam.ctypes.data, width, height, lo.ctypes.data, hi.ctypes.data,
                                         l.ctypes.data if l.size else None, l.size // 16, float(radius_bound),
                                         out.ctypes.data, max_rects, ctypes.byref(n), ctypes.byref(u0)),
           "pt_primary_cull_rects_r")
    return (None if n.value < 0 else out[:n.value].copy()), float(u0.value)


def primary_cull_footprints(camera_ubo, width, height, root_min, root_max, lights16, radius_bound=-1.0, max_footprints=8):
    """pt_primary_cull_footprints: (n, 16) floats or None -- per object
    {x0, x1, y0, y1} and four half-planes {a, b, c} (inside: a*x + b*y <= c),
    outside all of which no primary ray whose two Box-Muller radii are at most
    radius_bound (negative: the kernel's tight bound) reaches the root box or
    a light (PT_OPT_CULL_FOOTPRINT)."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(16)
    lo = np.ascontiguousarray(root_min, np.float32).reshape(3)
    hi = np.ascontiguousarray(root_max, np.float32).reshape(3)
    l = np.ascontiguousarray(lights16, np.float32).reshape(-1)
    out = np.zeros((max_footprints, 16), np.float32)
    n = ctypes.c_int(0)
    _check(lib().pt_primary_cull_footprints(cam.ctypes.data, width, height, lo.ctypes.data, hi.ctypes.data,
                                            l.ctypes.data if l.size else None, l.size // 16, float(radius_bound),
                                            out.ctypes.data, max_footprints, ctypes.byref(n)),
           "pt_primary_cull_footprints")
    return None if n.value < 0 else out[:n.value].copy()


def primary_cull_sure(camera_ubo, width, height, root_min, root_max, lights16, radius_bound=-1.0):
    """pt_primary_cull_sure: (one region of 16 floats per light, in a
    footprint's layout, empty (x0 > x1) where none is derived; the count of
    non-empty ones), or (None, -1) without footprints.  Every primary ray with
    radii of at most radius_bound from a pixel inside hits that light."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(16)
    lo = np.ascontiguousarray(root_min, np.float32).reshape(3)
    hi = np.ascontiguousarray(root_max, np.float32).reshape(3)
    l = np.ascontiguousarray(lights16, np.float32).reshape(-1)
    nl = l.size // 16
    out = np.zeros((max(nl, 1), 16), np.float32)
    n = ctypes.c_int(0)
    _check(lib().pt_primary_cull_sure(cam.ctypes.data, width, height, lo.ctypes.data, hi.ctypes.data,
                                      l.ctypes.data if l.size else None, nl, float(radius_bound), out.ctypes.data,
                                      max(nl, 1), ctypes.byref(n)), "pt_primary_cull_sure")
    return (None, -1) if n.value < 0 else (out[:nl].copy(), n.value)


def write_image(path, rgba, width, height, fmt="png"):
    """pt_write_image: PFM (float) or 8-bit sRGB PNG of an accumulation image."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1)
    if a.size != width * height * 4:
        raise PTError("rgba must hold width*height*4 floats")
    _check(lib().pt_write_image(str(path).encode(), a.ctypes.data, width, height, 1 if fmt == "png" else 0),
           "pt_write_image")


def write_png8(path, rgba8, width, height):
    """pt_write_png8: the PNG of (H, W, 4) uint8 pixels (display's), alpha dropped."""
    a = np.ascontiguousarray(rgba8, np.uint8).reshape(-1)
    if a.size != width * height * 4:
        raise PTError("rgba8 must hold width*height*4 bytes")
    _check(lib().pt_write_png8(str(path).encode(), a.ctypes.data, width, height), "pt_write_png8")


def display_default_params():
    """pt_display_default_params as a DisplayParams."""
    p = DisplayParams()
    _check(lib().pt_display_default_params(ctypes.byref(p)), "pt_display_default_params")
    return p


def _display_params(params):
    """None (the library's defaults), a DisplayParams, or (tonemap, exposure,
    auto_exposure, key, white, adapt) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, DisplayParams):
        return ctypes.byref(params)
    tm, ex, au, key, white, adapt = params
    return ctypes.byref(DisplayParams(int(tm), float(ex), int(au), float(key), float(white), float(adapt)))


def display_host(rgba, width, height, params=None, auto_scale=0.0):
    """pt_display_host: ((H, W, 4) uint8, the auto scale the call used).
    auto_scale: the previous scale, 0.0 for none (read only when metering)."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1)
    if a.size != width * height * 4:
        raise PTError("rgba must hold width*height*4 floats")
    out = np.empty(a.size, np.uint8)
    scale = ctypes.c_float(auto_scale)
    _check(lib().pt_display_host(a.ctypes.data, width, height, _display_params(params), ctypes.byref(scale),
                                 out.ctypes.data), "pt_display_host")
    return out.reshape(height, width, 4), scale.value


def upsample_default_params():
    """pt_upsample_default_params as an UpsampleParams."""
    p = UpsampleParams()
    _check(lib().pt_upsample_default_params(ctypes.byref(p)), "pt_upsample_default_params")
    return p


def _upsample_params(params):
    """None (the library's defaults), an UpsampleParams, a scale alone, or
    (scale, sigma_normal, sigma_depth) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, UpsampleParams):
        return ctypes.byref(params)
    if isinstance(params, int):
        p = upsample_default_params()
        p.scale = params
        return ctypes.byref(p)
    s, sn, sz = params
    return ctypes.byref(UpsampleParams(int(s), float(sn), float(sz)))


def _upsample_scale(params):
    """The scale of what _upsample_params takes."""
    if params is None:
        return upsample_default_params().scale
    return params.scale if isinstance(params, UpsampleParams) else params if isinstance(params, int) else int(params[0])


def upsample_host(src, width, height, guide_full, params=None):
    """pt_upsample_host: the (height, width, 4) image src onto the grid of the
    (s*height, s*width, 4) guide, as (s*height, s*width, 4) float32."""
    s = _upsample_scale(params)
    a = np.ascontiguousarray(src, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide_full, np.float32).reshape(-1)
    if a.size != width * height * 4 or g.size != a.size * s * s:
        raise PTError("src must hold width*height*4 floats, guide_full scale*scale as many")
    out = np.empty(g.size, np.float32)
    _check(lib().pt_upsample_host(a.ctypes.data, width, height, g.ctypes.data, _upsample_params(params),
                                  out.ctypes.data), "pt_upsample_host")
    return out.reshape(height * s, width * s, 4)


def default_camera():
    ubo = np.zeros(16, np.float32)
    _check(lib().pt_default_camera(ubo.ctypes.data), "pt_default_camera")
    return ubo


def denoise_default_params():
    """pt_denoise_default_params as a DenoiseParams."""
    p = DenoiseParams()
    _check(lib().pt_denoise_default_params(ctypes.byref(p)), "pt_denoise_default_params")
    return p


def _denoise_params(params):
    """None (the library's defaults), a DenoiseParams, or (iterations,
    sigma_color, sigma_normal, sigma_depth) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, DenoiseParams):
        return ctypes.byref(params)
    it, sc, sn, sz = params
    return ctypes.byref(DenoiseParams(int(it), float(sc), float(sn), float(sz)))


def guide_ray(camera_ubo, width, height, x, y):
    """pt_guide_ray: (origin, direction) of pixel (x, y)'s guide ray (host only)."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(16)
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    _check(lib().pt_guide_ray(cam.ctypes.data, width, height, x, y, o.ctypes.data, d.ctypes.data), "pt_guide_ray")
    return o, d


def denoise_host(rgba, guide, width, height, params=None):
    """pt_denoise_host: the a-trous filter on the host, (H, W, 4) float32."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide, np.float32).reshape(-1)
    if a.size != width * height * 4 or g.size != a.size:
        raise PTError("rgba and guide must hold width*height*4 floats")
    out = np.empty(a.size, np.float32)
    _check(lib().pt_denoise_host(a.ctypes.data, g.ctypes.data, width, height, _denoise_params(params),
                                 out.ctypes.data), "pt_denoise_host")
    return out.reshape(height, width, 4)


def denoise_var_default_params():
    """pt_denoise_var_default_params as a DenoiseVarParams."""
    p = DenoiseVarParams()
    _check(lib().pt_denoise_var_default_params(ctypes.byref(p)), "pt_denoise_var_default_params")
    return p


def _denoise_var_params(params):
    """None (the library's defaults), a DenoiseVarParams, or (iterations,
    sigma_lum, sigma_normal, sigma_depth) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, DenoiseVarParams):
        return ctypes.byref(params)
    it, sl, sn, sz = params
    return ctypes.byref(DenoiseVarParams(int(it), float(sl), float(sn), float(sz)))


def denoise_var_host(rgba, moments, n_samples, guide, width, height, params=None):
    """pt_denoise_var_host: the variance-guided filter on the host, (H, W, 4)
    float32 from the colours, the moments {m1, m2} of n_samples samples and
    the guide."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1)
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide, np.float32).reshape(-1)
    if a.size != width * height * 4 or g.size != a.size or m.size != width * height * 2:
        raise PTError("rgba and guide must hold width*height*4 floats, moments width*height*2")
    out = np.empty(a.size, np.float32)
    _check(lib().pt_denoise_var_host(a.ctypes.data, m.ctypes.data, int(n_samples), g.ctypes.data, width, height,
                                     _denoise_var_params(params), out.ctypes.data), "pt_denoise_var_host")
    return out.reshape(height, width, 4)


def denoise_var_plane_host(rgba, variance, guide, width, height, params=None):
    """pt_denoise_var_plane_host: the variance-guided filter on the host from
    an explicit (H, W) variance plane, (H, W, 4) float32."""
    a = np.ascontiguousarray(rgba, np.float32).reshape(-1)
    v = np.ascontiguousarray(variance, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide, np.float32).reshape(-1)
    if a.size != width * height * 4 or g.size != a.size or v.size != width * height:
        raise PTError("rgba and guide must hold width*height*4 floats, variance width*height")
    out = np.empty(a.size, np.float32)
    _check(lib().pt_denoise_var_plane_host(a.ctypes.data, v.ctypes.data, g.ctypes.data, width, height,
                                           _denoise_var_params(params), out.ctypes.data), "pt_denoise_var_plane_host")
    return out.reshape(height, width, 4)


def temporal_default_params():
    """pt_temporal_default_params as a TemporalParams."""
    p = TemporalParams()
    _check(lib().pt_temporal_default_params(ctypes.byref(p)), "pt_temporal_default_params")
    return p


def _temporal_params(params):
    """None (the library's defaults), a TemporalParams, or (max_history,
    alpha_min, normal_min, depth_rel) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, TemporalParams):
        return ctypes.byref(params)
    mh, am, nm, dr = params
    return ctypes.byref(TemporalParams(int(mh), float(am), float(nm), float(dr)))


def reproject_host(cam_cur, cam_prev, width, height, n, color, moments, guide, history=None, params=None):
    """pt_reproject_host: temporal reprojection on the host.  history: None or
    (colour, moments, length, guide) of the previous frame.  Returns (colour
    (H, W, 4), moments (H, W, 2), length (H, W), variance (H, W)), float32."""
    cc = np.ascontiguousarray(cam_cur, np.float32).reshape(16)
    cp = np.ascontiguousarray(cam_prev, np.float32).reshape(16)
    npx = width * height
    c = np.ascontiguousarray(color, np.float32).reshape(-1)
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide, np.float32).reshape(-1)
    if c.size != npx * 4 or g.size != npx * 4 or m.size != npx * 2:
        raise PTError("colour and guide must hold width*height*4 floats, moments width*height*2")
    hist = [None] * 4
    if history is not None:
        hist = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in history]
        if [a.size for a in hist] != [npx * 4, npx * 2, npx, npx * 4]:
            raise PTError("history: colour width*height*4 floats, moments *2, length *1, guide *4")
    oc, om = np.empty(npx * 4, np.float32), np.empty(npx * 2, np.float32)
    ol, ov = np.empty(npx, np.float32), np.empty(npx, np.float32)
    im = ReprojectImages(c.ctypes.data, m.ctypes.data, g.ctypes.data, *[_ptr(a) for a in hist],
                         oc.ctypes.data, om.ctypes.data, ol.ctypes.data, ov.ctypes.data)
    _check(lib().pt_reproject_host(cc.ctypes.data, cp.ctypes.data, width, height, int(n), ctypes.byref(im),
                                   _temporal_params(params)), "pt_reproject_host")
    return (oc.reshape(height, width, 4), om.reshape(height, width, 2), ol.reshape(height, width),
            ov.reshape(height, width))


def spatial_var_default_params():
    """pt_spatial_var_default_params as a SpatialVarParams."""
    p = SpatialVarParams()
    _check(lib().pt_spatial_var_default_params(ctypes.byref(p)), "pt_spatial_var_default_params")
    return p


def _spatial_var_params(params):
    """None (the library's defaults), a SpatialVarParams, or (below, radius,
    sigma_normal, sigma_depth) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, SpatialVarParams):
        return ctypes.byref(params)
    below, radius, sn, sz = params
    return ctypes.byref(SpatialVarParams(int(below), int(radius), float(sn), float(sz)))


def spatial_variance_host(moments, length, variance, guide, width, height, params=None):
    """pt_spatial_variance_host: the variance plane with the pixels whose
    length is below params.below estimated from their neighbourhood's moments,
    (H, W) float32."""
    npx = width * height
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    l = np.ascontiguousarray(length, np.float32).reshape(-1)
    v = np.ascontiguousarray(variance, np.float32).reshape(-1)
    g = np.ascontiguousarray(guide, np.float32).reshape(-1)
    if m.size != npx * 2 or l.size != npx or v.size != npx or g.size != npx * 4:
        raise PTError("moments must hold width*height*2 floats, length and variance width*height, guide width*height*4")
    out = np.empty(npx, np.float32)
    _check(lib().pt_spatial_variance_host(m.ctypes.data, l.ctypes.data, v.ctypes.data, g.ctypes.data, width, height,
                                          _spatial_var_params(params), out.ctypes.data), "pt_spatial_variance_host")
    return out.reshape(height, width)


def adaptive_default_params():
    """pt_adaptive_default_params as an AdaptiveParams."""
    p = AdaptiveParams()
    _check(lib().pt_adaptive_default_params(ctypes.byref(p)), "pt_adaptive_default_params")
    return p


def _adaptive_params(params):
    """None (the library's defaults), an AdaptiveParams, or (min_batches,
    max_batches, step, threshold, lum_floor) -> what ctypes passes."""
    if params is None:
        return None
    if isinstance(params, AdaptiveParams):
        return ctypes.byref(params)
    lo, hi, step, thr, floor = params
    return ctypes.byref(AdaptiveParams(int(lo), int(hi), int(step), float(thr), float(floor)))


def adaptive_tiles(width, height):
    """16x16 tiles of a frame: (blocks_x, blocks_y)."""
    return (width + 15) // 16, (height + 15) // 16


def adaptive_select_host(moments, counts, width, height, params=None):
    """pt_adaptive_select_host: the stopping rule per 16x16 tile (raster
    order) -> (next counts uint32, errors E_T float32)."""
    bx, by = adaptive_tiles(width, height)
    m = np.ascontiguousarray(moments, np.float32).reshape(-1)
    n = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    if m.size != width * height * 2 or n.size != bx * by:
        raise PTError("moments must hold width*height*2 floats, counts one per 16x16 tile")
    nxt, err = np.empty(n.size, np.uint32), np.empty(n.size, np.float32)
    _check(lib().pt_adaptive_select_host(m.ctypes.data, n.ctypes.data, width, height, _adaptive_params(params),
                                         nxt.ctypes.data, err.ctypes.data), "pt_adaptive_select_host")
    return nxt, err


def _rays_in(rays):
    """n rays as a contiguous (n, 8) float32 array {o, d, limit, -}: from that layout or from RAY_DTYPE records."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32)
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 8)
    return a


def _rays_out(kind, n):
    if kind not in (RAYS_CLOSEST, RAYS_ANY):
        raise PTError(f"kind is RAYS_CLOSEST or RAYS_ANY, not {kind!r}")
    return np.zeros(n, HIT_DTYPE if kind == RAYS_CLOSEST else np.uint32)


def trace_rays_host(vertices, indices, nodes, rays, kind=RAYS_CLOSEST, int_bits=False, threads=0):
    """pt_trace_rays_host: the host statement of Renderer.trace_rays on the arrays of upload_scene.
    Returns HIT_DTYPE records (RAYS_CLOSEST) or uint32 0 / 1 (RAYS_ANY)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    n = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    r = _rays_in(rays)
    out = _rays_out(kind, r.shape[0])
    _check(lib().pt_trace_rays_host(_ptr(v), v.size, _ptr(i), i.size, _ptr(n), n.size // 8,
                                    PT_NODES_INT_BITS if int_bits else 0, kind, _ptr(r), r.shape[0], _ptr(out), threads),
           "pt_trace_rays_host")
    return out


def _radiance_params(samples, seed_stride):
    return ctypes.byref(RadianceParams(int(samples), int(seed_stride) & 0xFFFFFFFF))


def radiance_queries(origins, directions, seeds=0):
    """RAY_DTYPE records for trace_radiance: n origins, n directions (taken as given) and the paths' seeds."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    q = np.zeros(len(o), RAY_DTYPE)
    q["o"], q["d"] = o, np.asarray(directions, np.float32).reshape(-1, 3)
    q["limit"], q["reserved"] = 1e30, np.asarray(seeds, np.uint32)
    return q


def trace_radiance_host(vertices, indices, nodes, lights, rays, samples=1, seed_stride=1, max_depth=4, sss_bounces=3,
                        int_bits=False, threads=0):
    """pt_trace_radiance_host: the host statement of Renderer.trace_radiance on the arrays of upload_scene and
    upload_lights (16 floats a light; None or empty: no light).  rays as trace_rays takes them, the seed in
    `reserved`.  Returns (n, 4) float32."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    n = np.ascontiguousarray(nodes, np.float32).reshape(-1)
    L = np.ascontiguousarray(lights if lights is not None else [], np.float32).reshape(-1)
    if L.size % 16:
        raise PTError("lights hold 16 floats each")
    r = _rays_in(rays)
    out = np.zeros((r.shape[0], 4), np.float32)
    _check(lib().pt_trace_radiance_host(_ptr(v), v.size, _ptr(i), i.size, _ptr(n), n.size // 8,
                                        PT_NODES_INT_BITS if int_bits else 0, _ptr(L), L.size // 16, max_depth,
                                        sss_bounces, _radiance_params(samples, seed_stride), _ptr(r), r.shape[0],
                                        _ptr(out), threads), "pt_trace_radiance_host")
    return out


def camera_rays_host(camera_ubo, width, height, batch, pixels=None):
    """pt_camera_rays_host: main()'s own rays of a camera block, a frame size and a sample batch as RAY_DTYPE
    records, for the pixels y * width + x listed (None: every pixel in raster order)."""
    cam = np.ascontiguousarray(camera_ubo, np.float32).reshape(-1)
    if cam.size != 16:
        raise PTError("the camera block holds 16 floats")
    px = None if pixels is None else np.ascontiguousarray(pixels, np.int32).reshape(-1)
    n = width * height if px is None else px.size
    rays = np.zeros(n, RAY_DTYPE)
    _check(lib().pt_camera_rays_host(_ptr(cam), width, height, int(batch) & 0xFFFFFFFF, _ptr(px) if px is not None else None,
                                     n, _ptr(rays)), "pt_camera_rays_host")
    return rays


class Renderer:
    """One GPU's path tracer: upload, dispatch/render, read back."""

    def __init__(self, device=0, devices=None):
        """One GPU (pt_create), or with `devices` (a list of ordinals) one
        context over all of them (pt_create_multi: tile split, the frame on
        devices[0])."""
        self._c = ctypes.c_void_p()
        if devices is None:
            _check(lib().pt_create(device, ctypes.byref(self._c)), "pt_create")
        else:
            d = np.ascontiguousarray(devices, np.int32)
            _check(lib().pt_create_multi(d.ctypes.data, d.size, ctypes.byref(self._c)), "pt_create_multi")
        self.width = self.height = 0
        self._device = device if devices is None else int(devices[0])

    def group_info(self):
        """(device ordinals, members store straight into the frame)."""
        n, peer = ctypes.c_int(0), ctypes.c_int(0)
        devs = np.zeros(64, np.int32)
        _check(lib().pt_group_info(self._c, ctypes.byref(n), devs.ctypes.data, devs.size, ctypes.byref(peer)),
               "pt_group_info")
        return [int(x) for x in devs[:n.value]], bool(peer.value)

    def group_check(self):
        """The peer-store check (PT_OPT_GROUP_CHECK): (state, ms_peer,
        ms_staged); state -2 armed, -1 not run, 0 matched, 1 mismatch (staged
        copies in force)."""
        st, a, b = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_float(0)
        _check(lib().pt_group_check(self._c, ctypes.byref(st), ctypes.byref(a), ctypes.byref(b)), "pt_group_check")
        return st.value, a.value, b.value

    def upload_scene(self, vertices, indices, nodes, uvs=None, mat=None, int_bits=False):
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        n = np.ascontiguousarray(nodes, np.float32).reshape(-1)
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(-1)
        m = None if mat is None else np.ascontiguousarray(mat, np.uint32).reshape(-1)
        _check(lib().pt_upload_scene(self._c, _ptr(v), v.size, _ptr(i), i.size, _ptr(n), n.size // 8,
                                     _ptr(uv), 0 if uv is None else uv.size, _ptr(m), 0 if m is None else m.size,
                                     PT_NODES_INT_BITS if int_bits else 0), "pt_upload_scene")

    def upload(self, scene: Scene):
        _check(lib().pt_scene_upload(self._c, scene._h), "pt_scene_upload")

    def upload_lights(self, lights16):
        l = np.ascontiguousarray(lights16, np.float32).reshape(-1)
        _check(lib().pt_upload_lights(self._c, _ptr(l), l.size // 16), "pt_upload_lights")

    def set_camera(self, ubo16):
        u = np.ascontiguousarray(ubo16, np.float32).reshape(16)
        _check(lib().pt_set_camera(self._c, u.ctypes.data), "pt_set_camera")

    def set_params(self, max_depth=4, sss_bounces=3):
        p = Params(max_depth, sss_bounces)
        _check(lib().pt_set_params(self._c, ctypes.byref(p)), "pt_set_params")

    def set_partition(self, nranks, rank, slots=None):
        """Tile split over nranks (pt_set_partition); `slots` (one int per
        rank) gives unequal shares (pt_set_partition_slots)."""
        if slots is None:
            _check(lib().pt_set_partition(self._c, nranks, rank), "pt_set_partition")
            return
        sl = np.ascontiguousarray(slots, np.int32)
        if sl.size != nranks:
            raise PTError("one slot count per rank")
        _check(lib().pt_set_partition_slots(self._c, nranks, rank, sl.ctypes.data), "pt_set_partition_slots")

    def tiles_owned(self):
        n = ctypes.c_int()
        _check(lib().pt_tiles_owned(self._c, ctypes.byref(n)), "pt_tiles_owned")
        return n.value

    def tiles_pack(self, dst_device_ptr):
        _check(lib().pt_tiles_pack(self._c, dst_device_ptr), "pt_tiles_pack")

    def tiles_unpack(self, src_device_ptr, src_rank, frame_device_ptr):
        _check(lib().pt_tiles_unpack(self._c, src_device_ptr, src_rank, frame_device_ptr), "pt_tiles_unpack")

    def progressive_camera(self, ubo16):
        """Camera for the progressive loop; True if it reset the sample counter."""
        u = np.ascontiguousarray(ubo16, np.float32).reshape(16)
        reset = ctypes.c_int(0)
        _check(lib().pt_progressive_camera(self._c, u.ctypes.data, ctypes.byref(reset)), "pt_progressive_camera")
        return bool(reset.value)

    def progressive_advance(self, max_new, limit=1024):
        first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().pt_progressive_advance(self._c, max_new, limit, ctypes.byref(first), ctypes.byref(count)),
               "pt_progressive_advance")
        return first.value, count.value

    def readback_begin(self):
        t = ctypes.c_int(0)
        _check(lib().pt_readback_begin(self._c, ctypes.byref(t)), "pt_readback_begin")
        return t.value

    def readback_end(self, ticket):
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_readback_end(self._c, ticket, out.ctypes.data, out.size), "pt_readback_end")
        return out

    def items_live(self, rank):
        """(live items of `rank` in the last rendered frame, pixels per item)."""
        n, per = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().pt_items_live(self._c, rank, ctypes.byref(n), ctypes.byref(per)), "pt_items_live")
        return n.value, per.value

    def items_pack(self, dst_ptr):
        _check(lib().pt_items_pack(self._c, dst_ptr), "pt_items_pack")

    def render_packed(self, n_batches, dst_ptr, gathered_ptr=None, slot_floats=0, frame_ptr=None):
        """Fresh frame's live items into dst; optionally assemble the previous
        frame's gathered slots into frame in the same launch."""
        _check(lib().pt_render_packed(self._c, n_batches, dst_ptr, gathered_ptr, slot_floats, frame_ptr),
               "pt_render_packed")

    def items_unpack_all(self, src_ptr, slot_floats, frame_ptr):
        _check(lib().pt_items_unpack_all(self._c, src_ptr, slot_floats, frame_ptr), "pt_items_unpack_all")

    def set_option(self, key, value):
        _check(lib().pt_set_option(self._c, key, value), "pt_set_option")

    def last_kernel(self):
        """Kernel of the last render: KERNEL_RECURSIVE or KERNEL_WAVEFRONT."""
        k = ctypes.c_int(0)
        _check(lib().pt_last_kernel(self._c, ctypes.byref(k)), "pt_last_kernel")
        return k.value

    def set_stream(self, stream_handle):
        _check(lib().pt_set_stream(self._c, stream_handle), "pt_set_stream")

    def resize_and_clear(self, w, h):
        _check(lib().pt_resize_and_clear(self._c, w, h), "pt_resize_and_clear")
        self.width, self.height = w, h

    def bind_accum(self, device_ptr, w, h):
        _check(lib().pt_bind_accum(self._c, device_ptr, w, h), "pt_bind_accum")
        self.width, self.height = w, h

    def clear(self):
        _check(lib().pt_clear_accum(self._c), "pt_clear_accum")

    def accum_ptr(self):
        return lib().pt_accum_device_ptr(self._c)

    def dispatch(self, sample_batch):
        _check(lib().pt_dispatch(self._c, sample_batch), "pt_dispatch")

    def render(self, first_batch, n_batches):
        _check(lib().pt_render(self._c, first_batch, n_batches), "pt_render")

    def synchronize(self):
        _check(lib().pt_synchronize(self._c), "pt_synchronize")

    def read_accum(self):
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_accum(self._c, out.ctypes.data, out.size), "pt_read_accum")
        return out

    def render_guide(self):
        """Enqueue the first-hit guide image {n.xyz, t} of the current inputs."""
        _check(lib().pt_render_guide(self._c), "pt_render_guide")

    def guide_ptr(self):
        return lib().pt_guide_device_ptr(self._c)

    def read_guide(self):
        """The guide image, (H, W, 4) float32."""
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_guide(self._c, out.ctypes.data, out.size), "pt_read_guide")
        return out.reshape(self.height, self.width, 4)

    def denoise(self, params=None, src_ptr=None, dst_ptr=None):
        """pt_denoise: filter src (default: the accumulation image) into dst;
        with dst_ptr None the library-owned result is read back and returned
        as (H, W, 4) float32."""
        _check(lib().pt_denoise(self._c, _denoise_params(params), src_ptr, dst_ptr), "pt_denoise")
        if dst_ptr is not None:
            return None
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_denoised(self._c, out.ctypes.data, out.size), "pt_read_denoised")
        return out.reshape(self.height, self.width, 4)

    def moments_ptr(self):
        """pt_moments_device_ptr: None when the moments are off or invalid."""
        return lib().pt_moments_device_ptr(self._c)

    def read_moments(self):
        """pt_read_moments: ((H, W, 2) float32 {m1, m2}, n_samples) (PT_OPT_MOMENTS)."""
        out = np.empty(self.width * self.height * 2, np.float32)
        n = ctypes.c_uint32(0)
        _check(lib().pt_read_moments(self._c, out.ctypes.data, out.size, ctypes.byref(n)), "pt_read_moments")
        return out.reshape(self.height, self.width, 2), int(n.value)

    def denoise_var(self, params=None, dst_ptr=None):
        """pt_denoise_var: the variance-guided filter of the accumulation image
        and its moments; with dst_ptr None the library-owned result is read
        back and returned as (H, W, 4) float32."""
        _check(lib().pt_denoise_var(self._c, _denoise_var_params(params), dst_ptr), "pt_denoise_var")
        if dst_ptr is not None:
            return None
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_denoised(self._c, out.ctypes.data, out.size), "pt_read_denoised")
        return out.reshape(self.height, self.width, 4)

    def reproject(self, cam_cur, cam_prev, width, height, n, images, params=None):
        """pt_reproject: enqueue the temporal reprojection of device images;
        `images` is a ReprojectImages of device pointers."""
        cc = np.ascontiguousarray(cam_cur, np.float32).reshape(16)
        cp = np.ascontiguousarray(cam_prev, np.float32).reshape(16)
        _check(lib().pt_reproject(self._c, cc.ctypes.data, cp.ctypes.data, width, height, int(n), ctypes.byref(images),
                                  _temporal_params(params)), "pt_reproject")

    def temporal_advance(self, ubo16, n_batches):
        """pt_temporal_advance: one frame of the temporal loop (PT_OPT_MOMENTS 1)."""
        u = np.ascontiguousarray(ubo16, np.float32).reshape(16)
        _check(lib().pt_temporal_advance(self._c, u.ctypes.data, int(n_batches)), "pt_temporal_advance")

    def temporal_reset(self):
        _check(lib().pt_temporal_reset(self._c), "pt_temporal_reset")

    def temporal_info(self):
        """(frames, samples) since the last reset."""
        f, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(lib().pt_temporal_info(self._c, ctypes.byref(f), ctypes.byref(s)), "pt_temporal_info")
        return int(f.value), int(s.value)

    def temporal_ptr(self, which):
        """pt_temporal_device_ptr: 0 colour, 1 moments, 2 length, 3 variance; None when there is none."""
        return lib().pt_temporal_device_ptr(self._c, which)

    def read_temporal(self):
        """pt_read_temporal: (colour (H, W, 4), moments (H, W, 2), length (H, W)) float32."""
        n = self.width * self.height
        c, m, l = np.empty(n * 4, np.float32), np.empty(n * 2, np.float32), np.empty(n, np.float32)
        _check(lib().pt_read_temporal(self._c, c.ctypes.data, m.ctypes.data, l.ctypes.data), "pt_read_temporal")
        return (c.reshape(self.height, self.width, 4), m.reshape(self.height, self.width, 2),
                l.reshape(self.height, self.width))

    def temporal_denoise(self, params=None, dst_ptr=None):
        """pt_temporal_denoise: the variance-guided filter of the temporal
        result; with dst_ptr None the library-owned result is read back and
        returned as (H, W, 4) float32."""
        _check(lib().pt_temporal_denoise(self._c, _denoise_var_params(params), dst_ptr), "pt_temporal_denoise")
        if dst_ptr is not None:
            return None
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_denoised(self._c, out.ctypes.data, out.size), "pt_read_denoised")
        return out.reshape(self.height, self.width, 4)

    def spatial_variance(self, moments_ptr, length_ptr, variance_ptr, guide_ptr, width, height, out_ptr, params=None):
        """pt_spatial_variance: enqueue the spatial variance estimate of device
        images (float2 moments, float length and variance, float4 guide) into
        the float plane at out_ptr."""
        _check(lib().pt_spatial_variance(self._c, moments_ptr, length_ptr, variance_ptr, guide_ptr, width, height,
                                         _spatial_var_params(params), out_ptr), "pt_spatial_variance")

    def temporal_denoise_spatial(self, params=None, spatial_params=None, dst_ptr=None):
        """pt_temporal_denoise_spatial: pt_temporal_denoise with the variance
        of short histories estimated spatially first; with dst_ptr None the
        library-owned result is read back and returned as (H, W, 4) float32."""
        _check(lib().pt_temporal_denoise_spatial(self._c, _denoise_var_params(params),
                                                 _spatial_var_params(spatial_params), dst_ptr),
               "pt_temporal_denoise_spatial")
        if dst_ptr is not None:
            return None
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_denoised(self._c, out.ctypes.data, out.size), "pt_read_denoised")
        return out.reshape(self.height, self.width, 4)

    def adaptive_select(self, moments_ptr, counts_ptr, width, height, next_ptr, errors_ptr, params=None):
        """pt_adaptive_select: enqueue the stopping rule over device images
        (float2 moments, uint32 counts per tile) into next_ptr and errors_ptr."""
        _check(lib().pt_adaptive_select(self._c, moments_ptr, counts_ptr, width, height, _adaptive_params(params),
                                        next_ptr, errors_ptr), "pt_adaptive_select")

    def adaptive_begin(self, params=None):
        """pt_adaptive_begin: clear, then round 0 (every tile renders min_batches)."""
        _check(lib().pt_adaptive_begin(self._c, _adaptive_params(params)), "pt_adaptive_begin")

    def adaptive_advance(self, rounds=1):
        """pt_adaptive_advance: enqueue up to `rounds` rounds of rule + render."""
        _check(lib().pt_adaptive_advance(self._c, int(rounds)), "pt_adaptive_advance")

    def adaptive_info(self):
        """pt_adaptive_info: waits; (rounds done, live tiles, samples spent)."""
        r, l, s = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_ulonglong(0)
        _check(lib().pt_adaptive_info(self._c, ctypes.byref(r), ctypes.byref(l), ctypes.byref(s)), "pt_adaptive_info")
        return int(r.value), int(l.value), int(s.value)

    def adaptive_counts(self):
        """pt_adaptive_read_counts: (counts uint32, errors float32), each (blocks_y, blocks_x)."""
        bx, by = adaptive_tiles(self.width, self.height)
        n, e = np.empty(bx * by, np.uint32), np.empty(bx * by, np.float32)
        _check(lib().pt_adaptive_read_counts(self._c, n.ctypes.data, e.ctypes.data, n.size), "pt_adaptive_read_counts")
        return n.reshape(by, bx), e.reshape(by, bx)

    def adaptive_live(self):
        """pt_adaptive_read_live: the last round's live list, (n, 4) int32
        rows {x0, y0, first_batch, n_batches}."""
        bx, by = adaptive_tiles(self.width, self.height)
        ent, n = np.zeros((bx * by, 4), np.int32), ctypes.c_uint32(0)
        _check(lib().pt_adaptive_read_live(self._c, ent.ctypes.data, bx * by, ctypes.byref(n)), "pt_adaptive_read_live")
        return ent[:n.value].copy()

    def adaptive_ptr(self, which):
        """pt_adaptive_device_ptr: 0 counts, 1 errors, 2 variance plane; None when there is none."""
        return lib().pt_adaptive_device_ptr(self._c, which)

    def adaptive_denoise(self, params=None, dst_ptr=None):
        """pt_adaptive_denoise: the variance-guided filter of the adaptive
        result; with dst_ptr None the library-owned result is read back and
        returned as (H, W, 4) float32."""
        _check(lib().pt_adaptive_denoise(self._c, _denoise_var_params(params), dst_ptr), "pt_adaptive_denoise")
        if dst_ptr is not None:
            return None
        out = np.empty(self.width * self.height * 4, np.float32)
        _check(lib().pt_read_denoised(self._c, out.ctypes.data, out.size), "pt_read_denoised")
        return out.reshape(self.height, self.width, 4)

    def display(self, params=None, src_ptr=None, dst_ptr=None):
        """pt_display: src (default: the accumulation image) through exposure,
        tone map and the sRGB encode into dst; with dst_ptr None the
        library-owned result is read back and returned as (H, W, 4) uint8."""
        _check(lib().pt_display(self._c, _display_params(params), src_ptr, dst_ptr), "pt_display")
        if dst_ptr is not None:
            return None
        return self.read_display()

    def display_ptr(self):
        return lib().pt_display_device_ptr(self._c)

    def read_display(self):
        out = np.empty(self.width * self.height * 4, np.uint8)
        _check(lib().pt_read_display(self._c, out.ctypes.data, out.size), "pt_read_display")
        return out.reshape(self.height, self.width, 4)

    def display_exposure(self):
        """(auto scale the last metering display used, pixels it metered); waits."""
        s, n = ctypes.c_float(0), ctypes.c_uint32(0)
        _check(lib().pt_display_exposure(self._c, ctypes.byref(s), ctypes.byref(n)), "pt_display_exposure")
        return s.value, n.value

    def display_reset(self):
        _check(lib().pt_display_reset(self._c), "pt_display_reset")

    def display_readback_begin(self, params=None, src_ptr=None):
        t = ctypes.c_int(0)
        _check(lib().pt_display_readback_begin(self._c, _display_params(params), src_ptr, ctypes.byref(t)),
               "pt_display_readback_begin")
        return t.value

    def display_readback_end(self, ticket):
        out = np.empty(self.width * self.height * 4, np.uint8)
        _check(lib().pt_display_readback_end(self._c, ticket, out.ctypes.data, out.size), "pt_display_readback_end")
        return out.reshape(self.height, self.width, 4)

    def upsample_info(self):
        """pt_upsample_info: {"scale", "guide_size", "guide_launches", "size", "display_size"} (sizes as (W, H))."""
        info = (ctypes.c_int * 8)()
        _check(lib().pt_upsample_info(self._c, info), "pt_upsample_info")
        return {"scale": info[0], "guide_size": (info[1], info[2]), "guide_launches": info[3],
                "size": (info[4], info[5]), "display_size": (info[6], info[7])}

    def read_upsampled(self):
        """The library-owned upsampled image, (H, W, 4) float32 at the full size."""
        W, H = self.upsample_info()["size"]
        out = np.empty(W * H * 4, np.float32)
        _check(lib().pt_read_upsampled(self._c, out.ctypes.data, out.size), "pt_read_upsampled")
        return out.reshape(H, W, 4)

    def upsample(self, params=None, src_ptr=None, dst_ptr=None):
        """pt_upsample: src (default: the accumulation image) of the context's
        render size onto the full grid under the full-size guide the context
        renders and keeps; with dst_ptr None the library-owned result is read
        back and returned as (s*H, s*W, 4) float32."""
        _check(lib().pt_upsample(self._c, _upsample_params(params), src_ptr, dst_ptr), "pt_upsample")
        return self.read_upsampled() if dst_ptr is None else None

    def upsample_images(self, src_ptr, width, height, guide_full_ptr, dst_ptr=None, params=None):
        """pt_upsample_images: the same on explicit device images (no scene needed)."""
        _check(lib().pt_upsample_images(self._c, _upsample_params(params), src_ptr, width, height, guide_full_ptr,
                                        dst_ptr), "pt_upsample_images")
        return self.read_upsampled() if dst_ptr is None else None

    def upsampled_ptr(self):
        return lib().pt_upsampled_device_ptr(self._c)

    def upsample_guide_ptr(self):
        """pt_upsample_guide_device_ptr: the full-size guide pt_upsample keeps, or None."""
        return lib().pt_upsample_guide_device_ptr(self._c)

    def upsample_display(self, params=None, display_params=None, src_ptr=None, dst_ptr=None):
        """pt_upsample_display: upsampling and the display transform in one
        kernel; with dst_ptr None the library-owned result is read back and
        returned as (s*H, s*W, 4) uint8.  Metering sees the rendered pixels."""
        _check(lib().pt_upsample_display(self._c, _upsample_params(params), _display_params(display_params), src_ptr,
                                         dst_ptr), "pt_upsample_display")
        return self.read_display_upsampled() if dst_ptr is None else None

    def display_upsampled_ptr(self):
        return lib().pt_display_upsampled_device_ptr(self._c)

    def read_display_upsampled(self):
        W, H = self.upsample_info()["display_size"]
        out = np.empty(W * H * 4, np.uint8)
        _check(lib().pt_read_display_upsampled(self._c, out.ctypes.data, out.size), "pt_read_display_upsampled")
        return out.reshape(H, W, 4)

    def trace_rays(self, rays, kind=RAYS_CLOSEST):
        """The caller's own rays against the uploaded scene (needs nothing else): closest hits or occlusion.
        A numpy array ((n, 8) float32 {o, d, limit, -} or RAY_DTYPE records) goes through pt_trace_rays_sync
        and returns HIT_DTYPE records (RAYS_CLOSEST) or uint32 0 / 1 (RAYS_ANY).  A torch tensor on the device
        ((n, 8) float32, contiguous) goes through pt_trace_rays, enqueued on the context's stream (set_stream)
        and not waited for, and returns a tensor on the same device: (n, 8) float32 holding pt_hit records
        (view it as int32 for `tri`) or (n,) int32."""
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
                raise PTError("trace_rays: a contiguous float32 device tensor of n x 8 floats")
            n = rays.numel() // 8
            if kind not in (RAYS_CLOSEST, RAYS_ANY):
                raise PTError(f"kind is RAYS_CLOSEST or RAYS_ANY, not {kind!r}")
            out = (torch.empty((n, 8), dtype=torch.float32, device=rays.device) if kind == RAYS_CLOSEST
                   else torch.empty((n,), dtype=torch.int32, device=rays.device))
            _check(lib().pt_trace_rays(self._c, kind, rays.data_ptr() if n else None, n, out.data_ptr() if n else None),
                   "pt_trace_rays")
            return out
        r = _rays_in(rays)
        out = _rays_out(kind, r.shape[0])
        _check(lib().pt_trace_rays_sync(self._c, kind, _ptr(r), r.shape[0], _ptr(out)), "pt_trace_rays_sync")
        return out

    def trace_radiance(self, rays, samples=1, seed_stride=1):
        """The radiance arriving along the caller's own rays: pathTrace from each ray's origin, direction and seed
        (`reserved`) in the uploaded scene under the uploaded lights and parameters, `samples` samples a query
        from the seeds seed + s * seed_stride, folded by the shader's running mean.  A numpy array ((n, 8)
        float32 or RAY_DTYPE records, radiance_queries) goes through pt_trace_radiance_sync and returns (n, 4)
        float32; a torch tensor on the device ((n, 8) float32, contiguous) goes through pt_trace_radiance,
        enqueued on the context's stream and not waited for, and returns an (n, 4) tensor on the same device."""
        params = _radiance_params(samples, seed_stride)
        if type(rays).__module__.split(".")[0] == "torch":
            import torch
            if not rays.is_cuda or rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8:
                raise PTError("trace_radiance: a contiguous float32 device tensor of n x 8 floats")
            n = rays.numel() // 8
            out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            _check(lib().pt_trace_radiance(self._c, params, rays.data_ptr() if n else None, n,
                                           out.data_ptr() if n else None), "pt_trace_radiance")
            return out
        r = _rays_in(rays)
        out = np.zeros((r.shape[0], 4), np.float32)
        _check(lib().pt_trace_radiance_sync(self._c, params, _ptr(r), r.shape[0], _ptr(out)), "pt_trace_radiance_sync")
        return out

    def camera_rays(self, batch, pixels=None):
        """pt_camera_rays: main()'s own rays of the context's camera and frame size for a sample batch, as an
        (n, 8) float32 tensor on the device (the seed's bits in column 7), enqueued on the context's stream.
        pixels: an int32 device tensor of y * width + x, or None for every pixel in raster order."""
        import torch
        W, H = self.width, self.height
        if pixels is None:
            n, pp = W * H, None
        else:
            if not pixels.is_cuda or pixels.dtype != torch.int32 or not pixels.is_contiguous():
                raise PTError("camera_rays: pixels is a contiguous int32 device tensor")
            n, pp = pixels.numel(), pixels.data_ptr() if pixels.numel() else None
        out = torch.empty((n, 8), dtype=torch.float32, device=f"cuda:{self._device}" if pixels is None else pixels.device)
        _check(lib().pt_camera_rays(self._c, int(batch) & 0xFFFFFFFF, pp, n, out.data_ptr() if n else None),
               "pt_camera_rays")
        return out

    def set_stats_mode(self, on):
        _check(lib().pt_set_stats_mode(self._c, 1 if on else 0), "pt_set_stats_mode")

    def reset_stats(self):
        _check(lib().pt_reset_stats(self._c), "pt_reset_stats")

    def stats(self):
        s = Stats()
        _check(lib().pt_get_stats(self._c, ctypes.byref(s)), "pt_get_stats")
        return {"rays": s.rays, "nodes": s.nodes, "leaf_tests": s.leaf_tests, "samples": s.samples}

    # ---- native multi-GPU step loop (pt_dist_*) ----
    @staticmethod
    def dist_unique_id():
        """128-byte RCCL communicator id (rank 0 makes it, every rank gets a copy)."""
        buf = (ctypes.c_char * 128)()
        _check(lib().pt_dist_unique_id(buf, 128), "pt_dist_unique_id")
        return bytes(buf)

    def dist_init(self, uid, nranks, rank):
        b = (ctypes.c_char * 128).from_buffer_copy(uid)
        _check(lib().pt_dist_init(self._c, b, nranks, rank), "pt_dist_init")

    def dist_info(self):
        """(ranks the RCCL communicator reports via ncclCommCount, or -1;
        nranks and rank given to pt_dist_init)."""
        c, n, r = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().pt_dist_info(self._c, ctypes.byref(c), ctypes.byref(n), ctypes.byref(r)), "pt_dist_info")
        return c.value, n.value, r.value

    def dist_run(self, n_batches, n_frames, frames_ptr=None, n_frame_bufs=1, n_streams=2):
        _check(lib().pt_dist_run(self._c, n_batches, n_frames, n_streams, frames_ptr, n_frame_bufs), "pt_dist_run")

    def dist_set_streams(self, render0=None, render1=None, gather=None):
        _check(lib().pt_dist_set_streams(self._c, render0, render1, gather), "pt_dist_set_streams")

    def dist_slot_floats(self):
        n = ctypes.c_size_t(0)
        _check(lib().pt_dist_slot_floats(self._c, ctypes.byref(n)), "pt_dist_slot_floats")
        return n.value

    def dist_wait(self, timeout_ms):
        _check(lib().pt_dist_wait(self._c, timeout_ms), "pt_dist_wait")

    def dist_abort(self):
        _check(lib().pt_dist_abort(self._c), "pt_dist_abort")

    def dist_finalize(self):
        _check(lib().pt_dist_finalize(self._c), "pt_dist_finalize")

    def traced(self):
        """Work the fast kernels actually did while PT_OPT_COUNT_TRACED was on
        (pt_get_traced), since the last reset_stats."""
        t = Traced()
        _check(lib().pt_get_traced(self._c, ctypes.byref(t)), "pt_get_traced")
        return {k: int(getattr(t, k)) for k, _ in Traced._fields_}

    def wide_info(self):
        """(wide nodes, stack bound) of the culled wide walk, or (0, 0, reason)."""
        info = (ctypes.c_int * 2)()
        _check(lib().pt_wide_info(self._c, info), "pt_wide_info")
        if info[0] == 0:
            return 0, 0, lib().pt_last_error().decode()
        return info[0], info[1]

    def sweep_info(self):
        """(distinct boxes, leaves) of the sweep walk's table when it is in
        force (PT_OPT_SMALL_SWEEP), else (0, 0)."""
        b, n = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().pt_sweep_info(self._c, ctypes.byref(b), ctypes.byref(n)), "pt_sweep_info")
        return b.value, n.value

    def cull_info(self):
        """(tight rectangles, footprints among them, non-empty sure regions) the
        per-sample skip of the next launch decides by, as the options stand
        (PT_OPT_CULL_FOOTPRINT)."""
        info = (ctypes.c_int * 3)()
        _check(lib().pt_cull_info(self._c, info), "pt_cull_info")
        return info[0], info[1], info[2]

    def sweep_walk(self):
        """Which walk the launches run as the options stand: 0 the threaded
        walk, 1 the sweep that keeps nothing from the root's test, 2 the sweep
        with hull faces (PT_OPT_SWEEP_HULL), 3 the straight-line sweep of a
        cube table (PT_OPT_SWEEP_CUBE)."""
        w = ctypes.c_int(0)
        _check(lib().pt_sweep_walk(self._c, ctypes.byref(w)), "pt_sweep_walk")
        return w.value

    def mixed_info(self):
        """(schedule, live workgroups, measured launches) of the last launch:
        schedule 0 none, 1 static, 2 measured (PT_OPT_MIXED_LANES)."""
        info = (ctypes.c_int * 3)()
        _check(lib().pt_mixed_info(self._c, info), "pt_mixed_info")
        return info[0], info[1], info[2]

    def last_launch_ms(self):
        ms = ctypes.c_float()
        _check(lib().pt_last_launch_ms(self._c, ctypes.byref(ms)), "pt_last_launch_ms")
        return ms.value

    def launch_times_ms(self):
        n = ctypes.c_size_t()
        out = np.zeros(512, np.float32)
        _check(lib().pt_launch_times_ms(self._c, out.ctypes.data, out.size, ctypes.byref(n)), "pt_launch_times_ms")
        return out[: n.value].copy()

    def launch_span_ms(self):
        """(device ms from the first launch's start to the last end, launches)
        since reset_launch_times -- the busy span of overlapping launches."""
        ms, n = ctypes.c_float(), ctypes.c_size_t()
        _check(lib().pt_launch_span_ms(self._c, ctypes.byref(ms), ctypes.byref(n)), "pt_launch_span_ms")
        return ms.value, n.value

    def reset_launch_times(self):
        _check(lib().pt_reset_launch_times(self._c), "pt_reset_launch_times")

    def close(self):
        if self._c:
            lib().pt_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
