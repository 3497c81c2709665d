"""raytracing_gpu_amd — MI355X (gfx950) drop-in for the per-pixel render path of
daRoyalCacti/Raytracing_GPU.

Host mirror of the reference's interface for that path (names and argument meaning kept):

  * ``render_settings``  — render.h:21-50 (image_width, samples_per_pixel_per_fb, no_fb, ...)
  * ``scene`` / ``Scene.builtin(name)`` — struct scene and its subclasses, scenes.h:36-621
  * ``draw(scene, settings)`` — render.h:118-174 (render_init, no_fb render launches, per-fb
    quantise + square-average); returns the PNG raster instead of writing ./image.png
  * ``draw_progressive(scene, settings, every=..., on_image=..., checkpoint=...)`` — the same draw
    cut after any frame buffer (the reference keeps tmp/<id>.ppm per fb, render.h:152-162):
    previews, stop and resume through ``Context.accumulator`` / ``Accumulator`` / ``read_checkpoint``;
    ``until_noise=`` stops the draw once the per-pixel noise estimate of ``Accumulator.noise_monitor``
    (``NoiseMonitor``, ``read_noise``) says the 8-bit image has converged
  * ``draw_adaptive(scene, settings, every=..., until_noise=..., checkpoint=...)`` — the same draw
    rendering only the 16 x 16 tiles that are still noisy (``Context.adaptive`` / ``AdaptiveAccumulator``,
    ``Context.render_tiles``); it can be stopped, resumed and refined (``read_adaptive_checkpoint``)
  * ``Context.render_init / render / resolve`` — the kernels render_init (render.h:84-92) and
    render (render.h:94-113) behind the C ABI of include/rt_hip.h

Everything is computed by librt_hip.so (hand-written HIP for gfx950).  There is no CPU fallback:
if the library is missing or the device call fails, the call raises.
"""
from __future__ import annotations

import ctypes
import math
import sys
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_uint64, c_void_p
from dataclasses import dataclass

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_HIP_LIB") or os.path.join(_PKG, "librt_hip.so")  # override: experiments

RT_CAM_REF_SLOT0 = 0
RT_CAM_PER_PIXEL = 1
RT_FLAG_EXACT_TRAVERSAL = 1
RT_FLAG_AUDIT = 2
RT_FLAG_NO_LDS = 4
RT_FLAG_WIDEST = 8
RT_FLAG_NO_STEP = 16
RT_FLAG_NO_SCHEDULE = 32
RT_FLAG_NO_CAMERA_BINS = 64
RT_FLAG_NO_SPLIT = 128
RT_FLAG_FRESH = 256
RT_SCHED_PREVIOUS = 1
RT_SCHED_SPLIT_REPLAY = 2
RT_SCHED_PROBE = 4
# rt_schedule_read's arrays and their element types
RT_SCHED_ITEM_COST, RT_SCHED_PERM, RT_SCHED_PROBE_RAW, RT_SCHED_PROBE_SMOOTH, RT_SCHED_SPLIT_LEN, RT_SCHED_ORDER = range(6)
SCHED_DTYPES = ("<u2", "<u4", "<u2", "<u2", "u1", "<u4")
# rt_camera_tiles_read's arrays and their element types
RT_CTILES_COUNT, RT_CTILES_ENTRIES, RT_CTILES_MASK, RT_CTILES_SPHERES, RT_CTILES_IDS = range(5)
CTILES_DTYPES = ("<i4", "<i4", "<u4", "<f4", "<i4")

PRIM_SPHERE, PRIM_MOVING_SPHERE, PRIM_RECT_XY, PRIM_RECT_XZ, PRIM_RECT_YZ, PRIM_TRIANGLE, PRIM_BOX = range(7)
OBJ_PRIM, OBJ_LIST, OBJ_BVH, OBJ_XFORM, OBJ_MEDIUM = range(5)
MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC, MAT_DIFFUSE_LIGHT, MAT_ISOTROPIC = range(5)

BUILTIN_SCENES = ("basic", "first", "big1", "two_spheres", "two_perlin", "cornell", "cornell_smoke")


# ---------------------------------------------------------------- C structs (include/rt_hip.h)
class rt_camera(ctypes.Structure):
    _fields_ = [("origin", c_float * 3), ("lower_left", c_float * 3), ("horizontal", c_float * 3),
                ("vertical", c_float * 3), ("u", c_float * 3), ("v", c_float * 3), ("w", c_float * 3),
                ("lens_radius", c_float), ("time0", c_float), ("time1", c_float)]


class rt_prim(ctypes.Structure):
    _fields_ = [("p", c_float * 10), ("type", c_int32), ("material", c_int32)]


class rt_bvh_node(ctypes.Structure):
    _fields_ = [("lo", c_float * 3), ("leaf_a", c_int32), ("hi", c_float * 3), ("leaf_b", c_int32)]


class rt_object(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("a", c_int32), ("b", c_int32), ("c", c_int32), ("f", c_float * 8)]


class rt_material(ctypes.Structure):
    _fields_ = [("type", c_int32), ("texture", c_int32), ("param", c_float), ("pad", c_int32)]


class rt_texture(ctypes.Structure):
    _fields_ = [("type", c_int32), ("a", c_int32), ("b", c_int32), ("pad", c_int32),
                ("color", c_float * 3), ("scale", c_float)]


class rt_scene_soa(ctypes.Structure):
    _fields_ = [("camera", rt_camera), ("background", c_float * 3), ("aspect", c_float),
                ("world", POINTER(c_int32)), ("n_world", c_int32),
                ("objects", POINTER(rt_object)), ("n_objects", c_int32),
                ("prims", POINTER(rt_prim)), ("n_prims", c_int32),
                ("triangles", c_void_p), ("n_triangles", c_int32),
                ("nodes", POINTER(rt_bvh_node)), ("n_nodes", c_int32),
                ("materials", POINTER(rt_material)), ("n_materials", c_int32),
                ("textures", POINTER(rt_texture)), ("n_textures", c_int32),
                ("perlins", c_void_p), ("n_perlins", c_int32),
                ("images", c_void_p), ("n_images", c_int32),
                ("texels", c_void_p), ("n_texels", c_int64)]


class rt_render_args(ctypes.Structure):
    _fields_ = [("width", c_int32), ("height", c_int32), ("spp", c_int32), ("fb_first", c_int32),
                ("fb_count", c_int32), ("max_depth", c_int32), ("cam_mode", c_int32),
                ("band_rows", c_int32), ("band_first", c_int32), ("band_stride", c_int32),
                ("stats", c_int32), ("flags", c_int32), ("seed", c_uint64)]


class rt_ctx_options(ctypes.Structure):
    """include/rt_hip.h rt_ctx_options: implementation choices that change no pixel (defaults from
    rt_ctx_options_default, the measured product configuration)."""
    _fields_ = [("world_tree", c_int32), ("quantized_tree", c_int32), ("merged_search", c_int32),
                ("merge_order", c_int32), ("dedup_triangles", c_int32), ("shade_min", c_int32),
                ("bins_min_items_per_lane", c_float), ("split_min_segments", c_float), ("split_order", c_int32),
                ("cost_shift", c_int32), ("long_pct", c_float), ("probe_schedule", c_int32),
                ("probe_max_items_per_lane", c_float), ("probe_depth", c_int32),
                ("spread_first", c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


RT_MERGE_ON, RT_MERGE_OFF, RT_MERGE_FALLBACK_ALL = range(3)
RT_ORDER_DISTANCE, RT_ORDER_LIST, RT_ORDER_REVERSED = range(3)
# Options every new Context starts from, on top of the library defaults (tests force the camera-ray
# tile lists on through this; the product leaves it empty).
DEFAULT_OPTIONS: dict = {}


class rt_counters(ctypes.Structure):
    _fields_ = [("segments", c_uint64), ("node_tests", c_uint64), ("prim_tests", c_uint64),
                ("samples", c_uint64), ("fallbacks", c_uint64)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class rt_schedule_info(ctypes.Structure):
    """include/rt_hip.h rt_schedule_info: the item schedule a context holds after its last render."""
    _fields_ = [("items", c_int64), ("n_long", c_int64), ("n_split", c_int64), ("rest_n", c_int64), ("pitems", c_int64),
                ("spread_waves", c_int64), ("split_state", c_int32), ("order_ok", c_int32), ("perm_kind", c_int32),
                ("shift", c_int32), ("spp", c_int32), ("ps", c_int32), ("prow", c_int32), ("pw", c_int32),
                ("spread_ran", c_int32), ("spread_top", c_int32), ("perm_key_valid", c_int32), ("pending_key_valid", c_int32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class rt_camera_tiles_info(ctypes.Structure):
    """include/rt_hip.h rt_camera_tiles_info: the camera-ray culling table a context holds."""
    _fields_ = [(k, c_int32) for k in ("kind", "width", "height", "tiles_x", "tiles_y", "cap", "tile_shift", "n", "n_kind",
                                       "last_used")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class rt_accum_info(ctypes.Structure):
    """include/rt_hip.h rt_accum_info: args.fb_count = frame buffers folded in so far."""
    _fields_ = [("args", rt_render_args), ("n_values", c_int64), ("scene_fp", c_uint64)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self.args, k)) for k, _ in rt_render_args._fields_}
        d["n_values"] = int(self.n_values)
        d["scene_fp"] = int(self.scene_fp)
        return d


class rt_noise_report(ctypes.Structure):
    """include/rt_hip.h rt_noise_report."""
    _fields_ = [("fbs", c_int32), ("tiles_x", c_int32), ("tiles_y", c_int32), ("pad", c_int32),
                ("pixels", c_int64), ("pixels_above", c_int64), ("threshold", c_float), ("max_noise", c_float)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k in ("fbs", "tiles_x", "tiles_y", "pixels", "pixels_above")}
        d["threshold"] = float(self.threshold)
        d["max_noise"] = float(self.max_noise)
        return d


class rt_adapt_report(ctypes.Structure):
    """include/rt_hip.h rt_adapt_report."""
    _fields_ = [("fbs", c_int32), ("tiles_x", c_int32), ("tiles_y", c_int32), ("tiles_active", c_int32),
                ("pixels", c_int64), ("pixels_active", c_int64), ("pixel_fbs", c_int64), ("pixels_above", c_int64),
                ("threshold", c_float), ("max_noise", c_float)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[:8]}
        d["threshold"] = float(self.threshold)
        d["max_noise"] = float(self.max_noise)
        return d


class rt_denoise_params(ctypes.Structure):
    """include/rt_hip.h rt_denoise_params."""
    _fields_ = [("search_radius", c_int32), ("patch_radius", c_int32), ("k", c_float), ("alpha", c_float),
                ("eps", c_float), ("pad", c_int32)]

    def as_dict(self) -> dict:
        return {"search_radius": int(self.search_radius), "patch_radius": int(self.patch_radius), "k": float(self.k),
                "alpha": float(self.alpha), "eps": float(self.eps)}


NOISE_MAX_FBS = 32768  # frame buffers a noise monitor accepts (include/rt_hip.h)

class rt_guide_hit(ctypes.Structure):
    """include/rt_hip.h rt_guide_hit (64 bytes)."""
    _fields_ = [("t", c_float), ("p", c_float * 3), ("n", c_float * 3), ("albedo", c_float * 3), ("u", c_float), ("v", c_float),
                ("prim", c_int32), ("material", c_int32), ("front", c_int32), ("pad", c_int32)]


GUIDE_HIT_DTYPE = np.dtype([("t", "<f4"), ("p", "<f4", 3), ("n", "<f4", 3), ("albedo", "<f4", 3), ("u", "<f4"), ("v", "<f4"),
                            ("prim", "<i4"), ("material", "<i4"), ("front", "<i4"), ("pad", "<i4")])


class rt_guide_params(ctypes.Structure):
    """include/rt_hip.h rt_guide_params."""
    _fields_ = [("normal_gain", c_float), ("albedo_gain", c_float), ("depth_gain", c_float), ("pad", c_int32)]

    def as_dict(self) -> dict:
        return {"normal_gain": float(self.normal_gain), "albedo_gain": float(self.albedo_gain), "depth_gain": float(self.depth_gain)}


class rt_aov_params(ctypes.Structure):
    """include/rt_hip.h rt_aov_params (16 bytes)."""
    _fields_ = [("samples", c_int32), ("lens", c_int32), ("footprint", c_int32), ("shutter", c_int32)]

    def as_dict(self) -> dict:
        return {"samples": int(self.samples), "lens": int(self.lens), "footprint": int(self.footprint), "shutter": int(self.shutter)}


class rt_spec_params(ctypes.Structure):
    """include/rt_hip.h rt_spec_params (16 bytes)."""
    _fields_ = [("max_bounces", c_int32), ("max_fuzz", c_float), ("glass", c_int32), ("reserved", c_int32)]

    def as_dict(self) -> dict:
        return {"max_bounces": int(self.max_bounces), "max_fuzz": float(self.max_fuzz), "glass": int(self.glass)}


class rt_spec_path(ctypes.Structure):
    """include/rt_hip.h rt_spec_path (32 bytes)."""
    _fields_ = [("bounces", c_int32), ("status", c_int32), ("first_prim", c_int32), ("first_material", c_int32),
                ("throughput", c_float * 3), ("depth", c_float)]


SPEC_PATH_DTYPE = np.dtype([("bounces", "<i4"), ("status", "<i4"), ("first_prim", "<i4"), ("first_material", "<i4"),
                            ("throughput", "<f4", 3), ("depth", "<f4")])
SPEC_MISS, SPEC_SURFACE, SPEC_ESCAPED, SPEC_LIMIT, SPEC_ABSORBED = range(5)  # rt_spec_status


# Every entry point of include/rt_hip.h: name -> (restype, argtypes)
ABI = {
    "rt_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "rt_ctx_destroy": (c_int, [c_void_p]),
    "rt_last_error": (c_char_p, [c_void_p]),
    "rt_ctx_options_default": (None, [POINTER(rt_ctx_options)]),
    "rt_ctx_set_options": (c_int, [c_void_p, POINTER(rt_ctx_options)]),
    "rt_ctx_get_options": (c_int, [c_void_p, POINTER(rt_ctx_options)]),
    "rt_owned_rows": (c_int32, [POINTER(rt_render_args), POINTER(c_int32)]),
    "rt_scene_validate": (c_int, [POINTER(rt_scene_soa), c_char_p, c_size_t]),
    "rt_scene_upload": (c_int, [c_void_p, POINTER(rt_scene_soa)]),
    "rt_render_init": (c_int, [c_void_p, c_int32, c_int32, c_uint64]),
    "rt_read_states": (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    "rt_render": (c_int, [c_void_p, POINTER(rt_render_args), c_void_p, POINTER(rt_counters)]),
    "rt_last_render_ms": (c_float, [c_void_p]),
    "rt_last_kernel_ms": (c_float, [c_void_p]),
    "rt_last_render_kernel": (ctypes.c_char_p, [c_void_p]),
    "rt_last_render_schedule": (c_int32, [c_void_p]),
    "rt_last_render_body": (c_int32, [c_void_p]),
    "rt_schedule_get_info": (c_int, [c_void_p, POINTER(rt_schedule_info)]),
    "rt_schedule_read": (c_int, [c_void_p, c_int32, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_camera_tiles_get_info": (c_int, [c_void_p, POINTER(rt_camera_tiles_info)]),
    "rt_camera_tiles_read": (c_int, [c_void_p, c_int32, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_audit_log": (c_int, [c_void_p, POINTER(c_float), c_int32]),
    "rt_resolve": (c_int, [c_void_p, POINTER(rt_render_args), c_void_p, c_void_p]),
    "rt_draw": (c_int, [c_void_p, POINTER(rt_render_args), POINTER(c_uint8), POINTER(rt_counters)]),
    "rt_accum_create": (c_int, [c_void_p, POINTER(rt_render_args), c_int32, POINTER(c_void_p)]),
    "rt_accum_add": (c_int, [c_void_p, c_int32, POINTER(rt_counters)]),
    "rt_accum_add_fbs": (c_int, [c_void_p, c_void_p, c_int32]),
    "rt_accum_image": (c_int, [c_void_p, c_void_p, c_int32]),
    "rt_accum_get_info": (c_int, [c_void_p, POINTER(rt_accum_info)]),
    "rt_accum_last_add_ms": (c_float, [c_void_p]),
    "rt_accum_last_image_ms": (c_float, [c_void_p]),
    "rt_accum_destroy": (c_int, [c_void_p]),
    "rt_accum_save": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_accum_load": (c_int, [c_void_p, c_void_p, c_size_t, c_int32, POINTER(c_void_p)]),
    "rt_accum_blob_info": (c_int, [c_void_p, c_size_t, POINTER(rt_accum_info)]),
    "rt_accum_blob_image": (c_int, [c_void_p, c_size_t, c_void_p]),
    "rt_accum_blob_pack": (c_int, [POINTER(rt_accum_info), c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_noise_create": (c_int, [c_void_p, POINTER(c_void_p)]),
    "rt_noise_measure": (c_int, [c_void_p, c_float, POINTER(rt_noise_report), c_void_p, c_void_p]),
    "rt_noise_map": (c_int, [c_void_p, c_void_p]),
    "rt_noise_save": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_noise_load": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_void_p)]),
    "rt_noise_last_measure_ms": (c_float, [c_void_p]),
    "rt_noise_destroy": (c_int, [c_void_p]),
    "rt_noise_blob_info": (c_int, [c_void_p, c_size_t, POINTER(rt_accum_info)]),
    "rt_noise_blob_pack": (c_int, [POINTER(rt_accum_info), c_void_p, c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_noise_blob_measure": (c_int, [c_void_p, c_size_t, c_float, POINTER(rt_noise_report), c_void_p, c_void_p, c_void_p]),
    "rt_render_tiles": (c_int, [c_void_p, POINTER(rt_render_args), c_void_p, c_int32, c_void_p, POINTER(rt_counters)]),
    "rt_adapt_create": (c_int, [c_void_p, POINTER(rt_render_args), c_int32, POINTER(c_void_p)]),
    "rt_adapt_add": (c_int, [c_void_p, c_int32, POINTER(rt_counters)]),
    "rt_adapt_retire": (c_int, [c_void_p, c_float, c_int32, POINTER(rt_adapt_report)]),
    "rt_adapt_image": (c_int, [c_void_p, c_void_p, c_int32]),
    "rt_adapt_counts": (c_int, [c_void_p, c_void_p]),
    "rt_adapt_noise_map": (c_int, [c_void_p, c_void_p]),
    "rt_adapt_get_report": (c_int, [c_void_p, c_float, POINTER(rt_adapt_report)]),
    "rt_adapt_last_add_ms": (c_float, [c_void_p]),
    "rt_adapt_last_retire_ms": (c_float, [c_void_p]),
    "rt_adapt_destroy": (c_int, [c_void_p]),
    "rt_adaptive_add": (c_int, [c_void_p, c_int32, c_int32, POINTER(rt_counters)]),
    "rt_adaptive_retire": (c_int, [c_void_p, c_float, c_int32, c_int32, POINTER(rt_adapt_report)]),
    "rt_adaptive_reopen": (c_int, [c_void_p, c_float, c_int32, c_int32, POINTER(rt_adapt_report)]),
    "rt_adaptive_active": (c_int, [c_void_p, c_void_p]),
    "rt_adaptive_save": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]),
    "rt_adaptive_load": (c_int, [c_void_p, c_void_p, c_size_t, c_int32, POINTER(c_void_p)]),
    "rt_adaptive_blob_info": (c_int, [c_void_p, c_size_t, POINTER(rt_accum_info)]),
    "rt_adaptive_blob_tiles": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "rt_adaptive_blob_image": (c_int, [c_void_p, c_size_t, c_void_p]),
    "rt_adaptive_blob_measure": (c_int, [c_void_p, c_size_t, c_float, POINTER(rt_adapt_report), c_void_p, c_void_p, c_void_p]),
    "rt_adaptive_blob_pack": (c_int, [POINTER(rt_accum_info), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, POINTER(c_size_t)]),
    "rt_denoise_params_default": (None, [POINTER(rt_denoise_params)]),
    "rt_denoise_monitor": (c_int, [c_void_p, POINTER(rt_denoise_params), c_void_p, c_void_p, c_int32]),
    "rt_denoise_adaptive": (c_int, [c_void_p, POINTER(rt_denoise_params), c_void_p, c_void_p, c_int32]),
    "rt_denoise_monitor_last_ms": (c_float, [c_void_p]),
    "rt_denoise_adaptive_last_ms": (c_float, [c_void_p]),
    "rt_denoise_monitor_blob": (c_int, [c_void_p, c_size_t, POINTER(rt_denoise_params), c_void_p, c_void_p]),
    "rt_denoise_adaptive_blob": (c_int, [c_void_p, c_size_t, POINTER(rt_denoise_params), c_void_p, c_void_p]),
    "rt_guide_create": (c_int, [POINTER(rt_scene_soa), c_int, POINTER(c_void_p)]),
    "rt_guide_destroy": (c_int, [c_void_p]),
    "rt_guide_cast": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, c_void_p]),
    "rt_guide_render": (c_int, [c_void_p, c_int32, c_int32]),
    "rt_guide_planes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32]),
    "rt_guide_image": (c_int, [c_void_p, c_int32, c_void_p, c_int32]),
    "rt_guide_last_ms": (c_float, [c_void_p]),
    "rt_guide_cast_host": (c_int, [POINTER(rt_scene_soa), c_void_p, ctypes.c_longlong, c_void_p]),
    "rt_guide_render_host": (c_int, [POINTER(rt_scene_soa), c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_guide_params_default": (None, [POINTER(rt_guide_params)]),
    "rt_guide_denoise_monitor": (c_int, [c_void_p, c_void_p, POINTER(rt_denoise_params), POINTER(rt_guide_params), c_void_p,
                                         c_void_p, c_int32]),
    "rt_guide_denoise_adaptive": (c_int, [c_void_p, c_void_p, POINTER(rt_denoise_params), POINTER(rt_guide_params), c_void_p,
                                          c_void_p, c_int32]),
    "rt_guide_denoise_monitor_blob": (c_int, [c_void_p, c_size_t, POINTER(rt_denoise_params), POINTER(rt_guide_params), c_void_p,
                                              c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rt_guide_denoise_adaptive_blob": (c_int, [c_void_p, c_size_t, POINTER(rt_denoise_params), POINTER(rt_guide_params), c_void_p,
                                               c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "rt_aov_params_default": (None, [POINTER(rt_aov_params)]),
    "rt_aov_pattern": (c_int, [POINTER(rt_aov_params), c_void_p]),
    "rt_aov_render": (c_int, [c_void_p, c_int32, c_int32, POINTER(rt_aov_params)]),
    "rt_aov_coverage": (c_int, [c_void_p, c_void_p, c_int32]),
    "rt_aov_render_host": (c_int, [POINTER(rt_scene_soa), c_int32, c_int32, POINTER(rt_aov_params), c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "rt_aov_last_ms": (c_float, [c_void_p]),
    "rt_spec_params_default": (None, [POINTER(rt_spec_params)]),
    "rt_spec_cast": (c_int, [c_void_p, c_void_p, ctypes.c_longlong, POINTER(rt_spec_params), c_void_p, c_void_p]),
    "rt_spec_render": (c_int, [c_void_p, c_int32, c_int32, POINTER(rt_aov_params), POINTER(rt_spec_params)]),
    "rt_spec_cast_host": (c_int, [POINTER(rt_scene_soa), c_void_p, ctypes.c_longlong, POINTER(rt_spec_params), c_void_p, c_void_p]),
    "rt_spec_render_host": (c_int, [POINTER(rt_scene_soa), c_int32, c_int32, POINTER(rt_aov_params), POINTER(rt_spec_params),
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "rt_spec_last_ms": (c_float, [c_void_p]),
    "rt_scene_build": (c_int, [c_char_p, POINTER(c_void_p)]),
    "rt_scene_build_ex": (c_int, [c_char_p, c_void_p, POINTER(c_void_p)]),
    "rt_obj_load": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
    "rt_obj_view": (c_void_p, [c_void_p]),
    "rt_obj_free": (None, [c_void_p]),
    "rt_image_decode": (c_int, [c_void_p, ctypes.c_int64, POINTER(c_void_p)]),
    "rt_image_load": (c_int, [c_char_p, POINTER(c_void_p)]),
    "rt_image_view": (c_void_p, [c_void_p]),
    "rt_image_free": (None, [c_void_p]),
    "rt_scene_view": (POINTER(rt_scene_soa), [c_void_p]),
    "rt_scene_free": (None, [c_void_p]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load librt_hip.so (raises if it has not been built: there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `python -m raytracing_gpu_amd._build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # torch (device memory, streams, RCCL) bundles its own libamdhip64.so.7: load it first so
        # this library binds to the same HIP runtime instance instead of a second copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


RT_OK, RT_ERR_ARG, RT_ERR_HIP, RT_ERR_STATE, RT_ERR_SCENE, RT_ERR_NOMEM = range(6)


def denoise_params(params=None, **kw) -> rt_denoise_params:
    """The denoiser's parameters (include/rt_hip.h): the shipped defaults, or a copy of params (an
    rt_denoise_params, a dict of its fields, True or None for the defaults), with the fields of kw set."""
    p = rt_denoise_params()
    if isinstance(params, rt_denoise_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    else:
        lib().rt_denoise_params_default(ctypes.byref(p))
        if isinstance(params, dict):
            kw = {**params, **kw}
    for k, v in kw.items():
        if k not in ("search_radius", "patch_radius", "k", "alpha", "eps"):
            raise TypeError(f"rt_denoise_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _denoise_call(check, fn, what, handle, params, rows, width, png_order, gain):
    """fn(handle, params, image, gain or NULL, png_order) into fresh arrays: image, or (image, gain)."""
    p = denoise_params(params)
    img = np.zeros((rows, width, 3), np.uint8)
    g = np.zeros((rows, width), np.float32) if gain else None
    check(fn(handle, ctypes.byref(p), img.ctypes.data, g.ctypes.data if gain else None, 1 if png_order else 0), what)
    return (img, g) if gain else img


def guide_params(params=None, **kw) -> rt_guide_params:
    """The gains of the guided denoise (include/rt_hip.h): the shipped defaults, or a copy of params (an
    rt_guide_params, a dict of its fields, True or None for the defaults), with the fields of kw set."""
    p = rt_guide_params()
    if isinstance(params, rt_guide_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    else:
        lib().rt_guide_params_default(ctypes.byref(p))
        if isinstance(params, dict):
            kw = {**params, **kw}
    for k, v in kw.items():
        if k not in ("normal_gain", "albedo_gain", "depth_gain"):
            raise TypeError(f"rt_guide_params has no field {k!r}")
        setattr(p, k, v)
    return p


def aov_params(params=None, **kw) -> rt_aov_params:
    """The sample pattern of the averaged feature planes (include/rt_hip.h): the shipped defaults, or a copy of
    params (an rt_aov_params, a dict of its fields or None for the defaults), with the fields of kw set; a switch
    may be a bool."""
    p = rt_aov_params()
    if isinstance(params, rt_aov_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    else:
        lib().rt_aov_params_default(ctypes.byref(p))
        if isinstance(params, dict):
            kw = {**params, **kw}
    for k, v in kw.items():
        if k not in ("samples", "lens", "footprint", "shutter"):
            raise TypeError(f"rt_aov_params has no field {k!r}")
        setattr(p, k, int(v))
    return p


def spec_params(params=None, **kw) -> rt_spec_params:
    """How casts and planes follow mirrors and glass (include/rt_hip.h): the shipped defaults, or a copy of params
    (an rt_spec_params, a dict of its fields, an int for max_bounces, True or None for the defaults), with the
    fields of kw set."""
    p = rt_spec_params()
    if isinstance(params, rt_spec_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    else:
        lib().rt_spec_params_default(ctypes.byref(p))
        if isinstance(params, dict):
            kw = {**params, **kw}
        elif params is not None and not isinstance(params, bool):
            kw = {"max_bounces": params, **kw}
    for k, v in kw.items():
        if k not in ("max_bounces", "max_fuzz", "glass"):
            raise TypeError(f"rt_spec_params has no field {k!r}")
        setattr(p, k, float(v) if k == "max_fuzz" else int(v))
    return p


def _centre_or(samples, lens, footprint, shutter):
    """The rt_aov_params pointer of a specular render: NULL (the centre ray) without samples."""
    return None if samples is None else ctypes.byref(aov_params(samples=samples, lens=lens, footprint=footprint, shutter=shutter))


def aov_pattern(params=None, **kw) -> np.ndarray:
    """The (samples, 5) float32 table du, dv, lx, ly, f of aov_params(params, **kw) (rt_aov_pattern: host only)."""
    p = aov_params(params, **kw)
    out = np.zeros((max(0, min(int(p.samples), 256)), 5), np.float32)
    rc = lib().rt_aov_pattern(ctypes.byref(p), out.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_aov_pattern failed ({rc})", rc)
    return out


def _guided(fn, guide, guide_params_):
    """fn(handle, guide, params, gains, image, gain, png_order) in the shape _denoise_call calls."""
    gp = guide_params(guide_params_)
    return lambda h, p, img, g, order: fn(h, guide._h, p, ctypes.byref(gp), img, g, order)


class RtError(RuntimeError):
    """A nonzero rt_status of the C ABI (`status`; None where no call returned one)."""

    def __init__(self, msg: str, status: int | None = None):
        super().__init__(msg)
        self.status = status


# ---------------------------------------------------------------- render_settings (render.h:21-50)
@dataclass
class render_settings:
    aspect_ratio: float = 16.0 / 9.0
    image_width: int = 1200
    image_height: int = 0
    samples_per_pixel_per_fb: int = 100
    no_fb: int = 10
    threads_x: int = 8  # kept for interface parity; the gfx950 kernel sizes its own launch
    threads_y: int = 8
    max_depth: int = 50
    rays_per_pixel: int = 0
    num_pixels: int = 0

    def calc_height(self) -> None:
        # static_cast<int>(image_width / aspect_ratio) with a double aspect (H18)
        self.image_height = int(self.image_width / float(np.float32(self.aspect_ratio)))

    def calc_rays_per_pixel(self) -> None:
        self.rays_per_pixel = self.samples_per_pixel_per_fb * self.no_fb

    def calc_num_pixels(self) -> None:
        self.num_pixels = self.image_width * self.image_height

    def calc_all(self) -> None:
        self.calc_height()
        self.calc_rays_per_pixel()
        self.calc_num_pixels()


# ---------------------------------------------------------------- scenes (scenes.h)
class Scene:
    """A flattened host scene built by the C++ scene library (rt_scene_build)."""

    def __init__(self, handle: c_void_p, name: str):
        self._h = handle
        self.name = name
        self.soa = lib().rt_scene_view(self._h).contents

    @classmethod
    def builtin(cls, name: str, images=None, meshes=None) -> "Scene":
        """Build a reference scene.  images: HxWxC uint8 arrays (decoded textures, stbi_load layout);
        meshes: raytracing_gpu_amd.assets.Mesh objects (24 floats per triangle).  Scenes that read
        files in the reference ("earth", "door", "cup", "final") need them; see assets.py."""
        h = c_void_p()
        if images is None and meshes is None:
            rc = lib().rt_scene_build(name.encode(), ctypes.byref(h))
        else:
            from .assets import pack_assets

            keep, ptr = pack_assets(images or [], meshes or [])
            rc = lib().rt_scene_build_ex(name.encode(), ptr, ctypes.byref(h))
            del keep
        if rc != 0:
            raise RtError(f"rt_scene_build({name!r}) failed with status {rc}")
        return cls(h, name)

    @property
    def aspect(self) -> float:
        return float(self.soa.aspect)

    @property
    def background(self) -> tuple:
        return tuple(self.soa.background)

    def prims(self) -> np.ndarray:
        """(n, 12) float32 view of the primitive records (type/material as raw int bits)."""
        n = self.soa.n_prims
        buf = ctypes.cast(self.soa.prims, POINTER(c_float * (12 * n))).contents
        return np.frombuffer(buf, dtype=np.float32).reshape(n, 12).copy()

    def close(self) -> None:
        if self._h:
            lib().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene(name: str) -> Scene:
    return Scene.builtin(name)


def validate_scene(soa: rt_scene_soa) -> tuple[int, str]:
    """rt_scene_validate on the host (no context, no GPU): (status, reason)."""
    buf = ctypes.create_string_buffer(256)
    rc = lib().rt_scene_validate(ctypes.byref(soa), buf, len(buf))
    return int(rc), buf.value.decode()


# ---------------------------------------------------------------- context (C ABI wrapper)
def make_args(width: int, height: int, spp: int, fb_first: int = 0, fb_count: int = 1, max_depth: int = 50,
              cam_mode: int = RT_CAM_REF_SLOT0, band_rows: int = 0, band_first: int = 0, band_stride: int = 1,
              stats: bool = False, seed: int = 1984, exact: bool = False, audit: bool = False,
              lds: bool = True, widest: bool = False, step: bool = True, schedule: bool = True,
              bins: bool = True, split: bool = True, fresh: bool = False) -> rt_render_args:
    flags = (RT_FLAG_EXACT_TRAVERSAL if exact else 0) | (RT_FLAG_AUDIT if audit else 0) | (0 if lds else RT_FLAG_NO_LDS)
    flags |= RT_FLAG_WIDEST if widest else 0
    flags |= 0 if step else RT_FLAG_NO_STEP
    flags |= 0 if schedule else RT_FLAG_NO_SCHEDULE
    flags |= 0 if bins else RT_FLAG_NO_CAMERA_BINS
    flags |= 0 if split else RT_FLAG_NO_SPLIT
    flags |= RT_FLAG_FRESH if fresh else 0
    return rt_render_args(width, height, spp, fb_first, fb_count, max_depth, cam_mode,
                          band_rows if band_rows > 0 else height, band_first, band_stride,
                          1 if stats else 0, flags, seed)


def owned_rows(args: rt_render_args) -> np.ndarray:
    n = lib().rt_owned_rows(ctypes.byref(args), None)
    rows = (c_int32 * max(n, 1))()
    lib().rt_owned_rows(ctypes.byref(args), rows)
    return np.frombuffer(rows, dtype=np.int32)[:n].copy()


class Context:
    """One HIP device: owns the device copy of a scene, the RNG states and a stream."""

    def __init__(self, device: int = 0):
        L = lib()
        self._c = c_void_p()
        rc = L.rt_ctx_create(device, ctypes.byref(self._c))
        if rc != 0:
            raise RtError(f"rt_ctx_create(device={device}) failed with status {rc}")
        self.device = device
        if DEFAULT_OPTIONS:
            self.set_options(**DEFAULT_OPTIONS)

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            msg = lib().rt_last_error(self._c)
            raise RtError(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)

    def options(self) -> dict:
        o = rt_ctx_options()
        self._check(lib().rt_ctx_get_options(self._c, ctypes.byref(o)), "rt_ctx_get_options")
        return o.as_dict()

    def set_options(self, reset: bool = False, **kw) -> dict:
        """Change context options (include/rt_hip.h rt_ctx_options); reset=True starts from the
        library defaults.  Upload-time options apply from the next upload.  Returns the options before."""
        before = self.options()
        o = rt_ctx_options()
        if reset:
            lib().rt_ctx_options_default(ctypes.byref(o))
        else:
            self._check(lib().rt_ctx_get_options(self._c, ctypes.byref(o)), "rt_ctx_get_options")
        for k, v in kw.items():
            if k not in before:
                raise KeyError(f"unknown context option {k!r}")
            setattr(o, k, v)
        self._check(lib().rt_ctx_set_options(self._c, ctypes.byref(o)), "rt_ctx_set_options")
        return before

    def upload(self, scene: Scene) -> None:
        self._check(lib().rt_scene_upload(self._c, ctypes.byref(scene.soa)), "rt_scene_upload")

    def render_init(self, width: int, height: int, seed: int = 1984) -> None:
        self._check(lib().rt_render_init(self._c, width, height, seed), "rt_render_init")

    def read_states(self, first: int, count: int) -> np.ndarray:
        out = np.zeros((count, 6), np.uint32)
        self._check(lib().rt_read_states(self._c, first, count, out.ctypes.data), "rt_read_states")
        return out

    def _after_torch(self) -> None:
        """The C ABI runs on the context's own HIP stream and expects device buffers that are ready:
        wait for work torch has queued on its current stream (e.g. the fill of a torch.zeros output)."""
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_initialized():
            torch.cuda.current_stream(self.device).synchronize()

    def render(self, args: rt_render_args, fb_dev_ptr: int) -> dict:
        self._after_torch()
        cnt = rt_counters()
        self._check(lib().rt_render(self._c, ctypes.byref(args), c_void_p(fb_dev_ptr), ctypes.byref(cnt)),
                    "rt_render")
        return cnt.as_dict()

    def render_tiles(self, args: rt_render_args, tiles, fb_dev_ptr: int) -> dict:
        """rt_render_tiles: render() for the pixels of the listed 16 x 16 tiles only (the noise monitor's
        tiles, id = ty * tiles_x + tx over (owned-row index, column)); every other float of the frame
        buffer (a device or host address) stays as it is.  Returns the counters of the rendered items."""
        self._after_torch()
        t = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1)
        cnt = rt_counters()
        self._check(lib().rt_render_tiles(self._c, ctypes.byref(args), t.ctypes.data, len(t), c_void_p(fb_dev_ptr),
                                          ctypes.byref(cnt)), "rt_render_tiles")
        return cnt.as_dict()

    def adaptive(self, args: rt_render_args, chunk_fbs: int = 1) -> "AdaptiveAccumulator":
        """An adaptive progressive draw of args' configuration starting at args.fb_first (args.fb_count
        is ignored): see AdaptiveAccumulator."""
        h = c_void_p()
        self._check(lib().rt_adapt_create(self._c, ctypes.byref(args), chunk_fbs, ctypes.byref(h)), "rt_adapt_create")
        return AdaptiveAccumulator(self, h, args)

    def resolve(self, args: rt_render_args, fb_dev_ptr: int, out_dev_ptr: int) -> None:
        self._after_torch()
        self._check(lib().rt_resolve(self._c, ctypes.byref(args), c_void_p(fb_dev_ptr), c_void_p(out_dev_ptr)),
                    "rt_resolve")

    def last_render_ms(self) -> float:
        """Device time of the last render call (a first launch's probe and schedule included)."""
        return float(lib().rt_last_render_ms(self._c))

    def last_kernel_ms(self) -> float:
        """Device time of the last render call's render kernel alone (rocprof's duration of it)."""
        return float(lib().rt_last_kernel_ms(self._c))

    def last_render_kernel(self) -> str:
        """rocprof name stem of the kernel the last render launched."""
        return lib().rt_last_render_kernel(self._c).decode()

    def last_render_schedule(self) -> int:
        """RT_SCHED_* bits of the last render launch (0: cold, nothing reused from an earlier launch)."""
        return int(lib().rt_last_render_schedule(self._c))

    def last_render_body(self) -> int:
        """Body of render_step_kernel the last render launch ran: 1 plain, 0 general (and every other kernel)."""
        return int(lib().rt_last_render_body(self._c))

    def schedule_info(self) -> dict:
        """rt_schedule_get_info: the item schedule the context holds after the last render (debug view)."""
        o = rt_schedule_info()
        self._check(lib().rt_schedule_get_info(self._c, ctypes.byref(o)), "rt_schedule_get_info")
        return o.as_dict()

    def schedule_read(self, which: int) -> np.ndarray:
        """rt_schedule_read: one device array of the schedule (RT_SCHED_ITEM_COST ... RT_SCHED_ORDER) as a
        numpy array of its element type; RtError (RT_ERR_STATE) when the context holds no such array."""
        need = c_size_t(0)
        self._check(lib().rt_schedule_read(self._c, which, None, 0, ctypes.byref(need)), "rt_schedule_read")
        out = np.zeros(need.value, np.uint8)
        self._check(lib().rt_schedule_read(self._c, which, out.ctypes.data, out.size, ctypes.byref(need)), "rt_schedule_read")
        return out.view(SCHED_DTYPES[which])

    def camera_tiles_info(self) -> dict:
        """rt_camera_tiles_get_info: the camera-ray culling table the context holds and what the last render
        launch used of it (debug view)."""
        o = rt_camera_tiles_info()
        self._check(lib().rt_camera_tiles_get_info(self._c, ctypes.byref(o)), "rt_camera_tiles_get_info")
        return o.as_dict()

    def camera_tiles_read(self, which: int) -> np.ndarray:
        """rt_camera_tiles_read: one array of the table (RT_CTILES_COUNT ... RT_CTILES_IDS) as a flat numpy array
        of its element type; RtError (RT_ERR_STATE) when the context holds no such array."""
        need = c_size_t(0)
        self._check(lib().rt_camera_tiles_read(self._c, which, None, 0, ctypes.byref(need)), "rt_camera_tiles_read")
        out = np.zeros(need.value, np.uint8)
        self._check(lib().rt_camera_tiles_read(self._c, which, out.ctypes.data, out.size, ctypes.byref(need)),
                    "rt_camera_tiles_read")
        return out.view(CTILES_DTYPES[which])

    def audit_log(self, cap: int = 4096) -> tuple[int, np.ndarray]:
        """(number of disagreements, [min(n, cap), 16] float32 entries) of the last audit render."""
        buf = np.zeros((cap, 16), np.float32)
        n = lib().rt_audit_log(self._c, buf.ctypes.data_as(POINTER(c_float)), cap)
        if n < 0:
            raise RtError("rt_audit_log failed")
        return n, buf[: min(n, cap)].copy()

    def draw_args(self, args: rt_render_args) -> tuple[np.ndarray, dict]:
        img = np.zeros((args.height, args.width, 3), dtype=np.uint8)
        cnt = rt_counters()
        self._check(lib().rt_draw(self._c, ctypes.byref(args), img.ctypes.data_as(POINTER(c_uint8)),
                                  ctypes.byref(cnt)), "rt_draw")
        return img, cnt.as_dict()

    def accumulator(self, args: rt_render_args, chunk_fbs: int = 1) -> "Accumulator":
        """A progressive draw of args' configuration starting at args.fb_first (args.fb_count is
        ignored): frame buffers are rendered chunk_fbs per launch and folded into float sums on the
        device; see Accumulator."""
        h = c_void_p()
        self._check(lib().rt_accum_create(self._c, ctypes.byref(args), chunk_fbs, ctypes.byref(h)), "rt_accum_create")
        return Accumulator(self, h)

    def close(self) -> None:
        for acc in list(getattr(self, "_accums", ())):  # an accumulator does not outlive its context
            acc.close()
        if getattr(self, "_c", None):
            lib().rt_ctx_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Accumulator:
    """rt_accum of include/rt_hip.h: draw() one frame buffer at a time.  The reference writes
    tmp/<id>.ppm after each frame buffer (render.h:152-162) and folds the files at the end
    (average_images, color.h:57-170); here the float sums stay on the device, so after any add()
    there is an image(), and save() / load() continue bit-identically in another process."""

    def __init__(self, ctx: Context, handle: c_void_p):
        import weakref

        self.ctx = ctx
        self._h = handle
        if not hasattr(ctx, "_accums"):
            ctx._accums = weakref.WeakSet()
        ctx._accums.add(self)

    @classmethod
    def load(cls, ctx: Context, path: str, chunk_fbs: int = 1) -> "Accumulator":
        """Continue from a checkpoint file; RtError with status RT_ERR_STATE when the context's scene
        is not the one the checkpoint was rendered from, RT_ERR_ARG for a malformed file."""
        with open(path, "rb") as f:
            blob = f.read()
        h = c_void_p()
        ctx._check(lib().rt_accum_load(ctx._c, blob, len(blob), chunk_fbs, ctypes.byref(h)), "rt_accum_load")
        return cls(ctx, h)

    def info(self) -> dict:
        i = rt_accum_info()
        self.ctx._check(lib().rt_accum_get_info(self._h, ctypes.byref(i)), "rt_accum_get_info")
        return i.as_dict()

    @property
    def done(self) -> int:
        """Frame buffers folded in so far."""
        return self.info()["fb_count"]

    def add(self, count: int = 1) -> dict:
        """Render and fold in the next count frame buffers; returns this call's counters."""
        self.ctx._after_torch()
        cnt = rt_counters()
        self.ctx._check(lib().rt_accum_add(self._h, count, ctypes.byref(cnt)), "rt_accum_add")
        return cnt.as_dict()

    def add_fbs(self, ptr: int, count: int) -> None:
        """Fold in count frame buffers [count][owned_rows][width][3] float32 at a device or host address."""
        self.ctx._after_torch()
        self.ctx._check(lib().rt_accum_add_fbs(self._h, c_void_p(ptr), count), "rt_accum_add_fbs")

    def image(self, png_order: bool = False) -> np.ndarray:
        """The image so far: (owned_rows, width, 3) uint8, owned rows ascending (rt_resolve's layout), or
        with png_order the whole image top row first (rt_draw's)."""
        i = self.info()
        img = np.zeros((i["n_values"] // (3 * i["width"]), i["width"], 3), np.uint8)
        self.ctx._check(lib().rt_accum_image(self._h, img.ctypes.data, 1 if png_order else 0), "rt_accum_image")
        return img

    def image_into(self, out_ptr: int, png_order: bool = False) -> None:
        """image() into caller memory (a device address with png_order False, or a host address)."""
        self.ctx._after_torch()
        self.ctx._check(lib().rt_accum_image(self._h, c_void_p(out_ptr), 1 if png_order else 0), "rt_accum_image")

    def last_add_ms(self) -> float:
        """Device time of the last accumulate launch (the last chunk of add(), or add_fbs())."""
        return float(lib().rt_accum_last_add_ms(self._h))

    def last_image_ms(self) -> float:
        """Device time of the last image() kernel."""
        return float(lib().rt_accum_last_image_ms(self._h))

    def blob(self) -> bytes:
        need = c_size_t()
        self.ctx._check(lib().rt_accum_save(self._h, None, 0, ctypes.byref(need)), "rt_accum_save")
        buf = ctypes.create_string_buffer(need.value)
        self.ctx._check(lib().rt_accum_save(self._h, buf, need.value, None), "rt_accum_save")
        return buf.raw

    def save(self, path: str) -> None:
        """Write the checkpoint to path: to a temporary name beside it first, then renamed over it."""
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(self.blob())
        os.replace(tmp, path)

    def noise_monitor(self) -> "NoiseMonitor":
        """Attach a noise monitor (rt_noise_create): only to an accumulator that has folded in no
        frame buffer and has none yet (RT_ERR_STATE otherwise).  From here on every add() / add_fbs()
        also updates its integer moments; the image and the checkpoint stay byte-identical."""
        h = c_void_p()
        self.ctx._check(lib().rt_noise_create(self._h, ctypes.byref(h)), "rt_noise_create")
        return NoiseMonitor(self, h)

    def close(self) -> None:
        """Destroys the accumulator; its noise monitor, if any, is closed first."""
        mon = getattr(self, "_monitor", None)
        if mon is not None:
            mon.close()
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_c", None):
                lib().rt_accum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NoiseMonitor:
    """rt_noise of include/rt_hip.h: per accumulator value the exact integer moments of c^2 over the
    frame buffers folded in, from which measure() / map() give the standard error of every pixel in
    8-bit output levels.  Integer sums: the same whatever the chunking, checkpointing or band tiling."""

    def __init__(self, acc: Accumulator, handle: c_void_p):
        self.acc = acc
        self._h = handle
        acc._monitor = self
        i = acc.info()
        self._rows, self._width = i["n_values"] // (3 * i["width"]), i["width"]

    @classmethod
    def load(cls, acc: Accumulator, path: str) -> "NoiseMonitor":
        """Attach the monitor saved at path to acc: RtError with status RT_ERR_STATE unless the file's
        header equals acc.info() in every field (frame buffers done and scene included), RT_ERR_ARG
        for a malformed file."""
        with open(path, "rb") as f:
            blob = f.read()
        h = c_void_p()
        acc.ctx._check(lib().rt_noise_load(acc._h, blob, len(blob), ctypes.byref(h)), "rt_noise_load")
        return cls(acc, h)

    def _check(self, rc: int, what: str) -> None:
        self.acc.ctx._check(rc, what)

    def measure(self, threshold: float) -> tuple[dict, np.ndarray, np.ndarray]:
        """(report, tile_max, tile_above): the report as a dict (fbs, tiles_x, tiles_y, pixels,
        pixels_above = pixels with noise > threshold, threshold, max_noise) and the per-tile maximum
        (float32) and count (int32) as (tiles_y, tiles_x) arrays over 16 x 16 pixel tiles.  Needs two
        frame buffers (RT_ERR_STATE before)."""
        ty, tx = (self._rows + 15) // 16, (self._width + 15) // 16
        tile_max, tile_above = np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.int32)
        rep = rt_noise_report()
        self._check(lib().rt_noise_measure(self._h, threshold, ctypes.byref(rep), tile_max.ctypes.data,
                                           tile_above.ctypes.data), "rt_noise_measure")
        return rep.as_dict(), tile_max, tile_above

    def map(self) -> np.ndarray:
        """The noise of every owned pixel, (owned_rows, width) float32, owned rows ascending."""
        out = np.zeros((self._rows, self._width), np.float32)
        self._check(lib().rt_noise_map(self._h, out.ctypes.data), "rt_noise_map")
        return out

    def map_into(self, out_ptr: int) -> None:
        """map() into caller memory (a device or host address)."""
        self.acc.ctx._after_torch()
        self._check(lib().rt_noise_map(self._h, c_void_p(out_ptr)), "rt_noise_map")

    def last_measure_ms(self) -> float:
        """Device time of the last measure() / map() kernel."""
        return float(lib().rt_noise_last_measure_ms(self._h))

    def denoise(self, params=None, png_order: bool = True, gain: bool = False, guide=None, guide_params=None):
        """The denoised image of the frame buffers so far (rt_denoise_monitor: a variance-guided NL-means
        filter on the monitor's moments; needs two frame buffers and the whole-image tiling): (rows, width, 3)
        uint8, top row first with png_order, and with gain=True also the (rows, width) float32 number of
        pixels' worth every pixel was averaged over.  params: see denoise_params().  Changes no state.
        guide: a Guide of the same scene that has rendered planes of the image's size (rt_guide_denoise_monitor:
        the feature-guided weights), with guide_params as guide_params() takes them."""
        if guide is not None:
            return _denoise_call(self._check, _guided(lib().rt_guide_denoise_monitor, guide, guide_params),
                                 "rt_guide_denoise_monitor", self._h, params, self._rows, self._width, png_order, gain)
        return _denoise_call(self._check, lib().rt_denoise_monitor, "rt_denoise_monitor", self._h, params, self._rows,
                             self._width, png_order, gain)

    def denoise_into(self, out_ptr: int, gain_ptr: int = 0, params=None, png_order: bool = False) -> None:
        """denoise() into caller memory (device addresses with png_order False, or host addresses)."""
        self.acc.ctx._after_torch()
        p = denoise_params(params)
        self._check(lib().rt_denoise_monitor(self._h, ctypes.byref(p), c_void_p(out_ptr), c_void_p(gain_ptr or None),
                                             1 if png_order else 0), "rt_denoise_monitor")

    def last_denoise_ms(self) -> float:
        """Device time of the last denoise()'s kernels."""
        return float(lib().rt_denoise_monitor_last_ms(self._h))

    def blob(self) -> bytes:
        need = c_size_t()
        self._check(lib().rt_noise_save(self._h, None, 0, ctypes.byref(need)), "rt_noise_save")
        buf = ctypes.create_string_buffer(need.value)
        self._check(lib().rt_noise_save(self._h, buf, need.value, None), "rt_noise_save")
        return buf.raw

    def save(self, path: str) -> None:
        """Write the monitor's side file to path: to a temporary name beside it first, then renamed."""
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(self.blob())
        os.replace(tmp, path)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().rt_noise_destroy(self._h)
            self._h = None
        if getattr(self.acc, "_monitor", None) is self:
            self.acc._monitor = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AdaptiveAccumulator:
    """rt_adapt of include/rt_hip.h: a progressive draw that renders only the 16 x 16 tiles that are
    still noisy.  add() renders and folds in frame buffers for the active tiles, retire() stops every
    active tile with at most max_above pixels above the threshold (and, with dilate, no failing active
    tile nearby), reopen() makes failing tiles active again.  Tile t of image() is byte-identical to draw()
    with no_fb = counts()[t]; save() / load() continue bit-identically in another process."""

    def __init__(self, ctx: Context, handle: c_void_p, args: rt_render_args):
        import weakref

        self.ctx = ctx
        self._h = handle
        self._rows, self._width = len(owned_rows(args)), args.width
        if not hasattr(ctx, "_accums"):
            ctx._accums = weakref.WeakSet()
        ctx._accums.add(self)

    @classmethod
    def load(cls, ctx: Context, path: str, chunk_fbs: int = 1) -> "AdaptiveAccumulator":
        """Continue from a checkpoint file (chunk_fbs need not be the saved draw's); RtError with status
        RT_ERR_STATE when the context's scene is not the checkpoint's, RT_ERR_ARG for a malformed file."""
        with open(path, "rb") as f:
            blob = f.read()
        return cls.from_blob(ctx, blob, chunk_fbs)

    @classmethod
    def from_blob(cls, ctx: Context, blob: bytes, chunk_fbs: int = 1) -> "AdaptiveAccumulator":
        """load() from the bytes blob() returned."""
        h = c_void_p()
        ctx._check(lib().rt_adaptive_load(ctx._c, blob, len(blob), chunk_fbs, ctypes.byref(h)), "rt_adaptive_load")
        i = rt_accum_info()
        lib().rt_adaptive_blob_info(blob, len(blob), ctypes.byref(i))
        return cls(ctx, h, i.args)

    def add(self, count: int = 1, limit: int | None = None) -> dict:
        """Render the next count frame buffers of every active tile and fold them in, no tile beyond limit
        frame buffers (a tile at the limit receives nothing and stays active); this call's counters."""
        self.ctx._after_torch()
        cnt = rt_counters()
        if limit is None:
            self.ctx._check(lib().rt_adapt_add(self._h, count, ctypes.byref(cnt)), "rt_adapt_add")
        else:
            self.ctx._check(lib().rt_adaptive_add(self._h, count, limit, ctypes.byref(cnt)), "rt_adaptive_add")
        return cnt.as_dict()

    def retire(self, threshold: float, max_above: int = 0, dilate: int = 0) -> dict:
        """Retire the active tiles with at most max_above pixels of noise > threshold, except those within
        dilate tiles (Chebyshev, over the tile grid) of an active tile that fails; the report after."""
        rep = rt_adapt_report()
        self.ctx._check(lib().rt_adaptive_retire(self._h, threshold, max_above, dilate, ctypes.byref(rep)),
                        "rt_adaptive_retire")
        return rep.as_dict()

    def reopen(self, threshold: float, max_above: int = 0, dilate: int = 0) -> dict:
        """Make every tile with more than max_above pixels of noise > threshold, and the tiles within dilate
        of one, active again; none retires.  A reopened tile continues from its own count.  The report after."""
        rep = rt_adapt_report()
        self.ctx._check(lib().rt_adaptive_reopen(self._h, threshold, max_above, dilate, ctypes.byref(rep)),
                        "rt_adaptive_reopen")
        return rep.as_dict()

    def active(self) -> np.ndarray:
        """(tiles_y, tiles_x) bool: the tiles still rendered."""
        out = np.zeros(((self._rows + 15) // 16, (self._width + 15) // 16), np.uint8)
        self.ctx._check(lib().rt_adaptive_active(self._h, out.ctypes.data), "rt_adaptive_active")
        return out.astype(bool)

    def blob(self) -> bytes:
        need = c_size_t()
        self.ctx._check(lib().rt_adaptive_save(self._h, None, 0, ctypes.byref(need)), "rt_adaptive_save")
        buf = ctypes.create_string_buffer(need.value)
        self.ctx._check(lib().rt_adaptive_save(self._h, buf, need.value, None), "rt_adaptive_save")
        return buf.raw

    def save(self, path: str) -> None:
        """Write the checkpoint to path: to a temporary name beside it first, then renamed over it."""
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(self.blob())
        os.replace(tmp, path)

    def report(self, threshold: float) -> dict:
        """retire()'s report without retiring anything."""
        rep = rt_adapt_report()
        self.ctx._check(lib().rt_adapt_get_report(self._h, threshold, ctypes.byref(rep)), "rt_adapt_get_report")
        return rep.as_dict()

    def image(self, png_order: bool = False) -> np.ndarray:
        """(owned_rows, width, 3) uint8, owned rows ascending, or with png_order the whole image top row first."""
        img = np.zeros((self._rows, self._width, 3), np.uint8)
        self.ctx._check(lib().rt_adapt_image(self._h, img.ctypes.data, 1 if png_order else 0), "rt_adapt_image")
        return img

    def counts(self) -> np.ndarray:
        """(tiles_y, tiles_x) int32: the frame buffers folded into every tile."""
        out = np.zeros(((self._rows + 15) // 16, (self._width + 15) // 16), np.int32)
        self.ctx._check(lib().rt_adapt_counts(self._h, out.ctypes.data), "rt_adapt_counts")
        return out

    def noise_map(self) -> np.ndarray:
        """(owned_rows, width) float32: every pixel's noise at its own tile's frame-buffer count."""
        out = np.zeros((self._rows, self._width), np.float32)
        self.ctx._check(lib().rt_adapt_noise_map(self._h, out.ctypes.data), "rt_adapt_noise_map")
        return out

    def last_add_ms(self) -> float:
        """Device time of the last fold kernel."""
        return float(lib().rt_adapt_last_add_ms(self._h))

    def last_retire_ms(self) -> float:
        """Device time of the last retire()'s measure kernel."""
        return float(lib().rt_adapt_last_retire_ms(self._h))

    def denoise(self, params=None, png_order: bool = True, gain: bool = False, guide=None, guide_params=None):
        """NoiseMonitor.denoise() with every pixel at its own tile's count (rt_denoise_adaptive; every tile
        needs two frame buffers): tiles that retired early at a higher noise are smoothed more.  guide,
        guide_params: as NoiseMonitor.denoise() (rt_guide_denoise_adaptive)."""
        if guide is not None:
            return _denoise_call(self.ctx._check, _guided(lib().rt_guide_denoise_adaptive, guide, guide_params),
                                 "rt_guide_denoise_adaptive", self._h, params, self._rows, self._width, png_order, gain)
        return _denoise_call(self.ctx._check, lib().rt_denoise_adaptive, "rt_denoise_adaptive", self._h, params, self._rows,
                             self._width, png_order, gain)

    def last_denoise_ms(self) -> float:
        """Device time of the last denoise()'s kernels."""
        return float(lib().rt_denoise_adaptive_last_ms(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_c", None):
                lib().rt_adapt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_noise(path: str, threshold: float) -> tuple[dict, np.ndarray, np.ndarray, np.ndarray]:
    """(report, tile_max, tile_above, map) of a monitor's side file, by the host-only rt_noise_blob_*
    functions (no context, no GPU); the report also carries the header's fields, as Accumulator.info()."""
    with open(path, "rb") as f:
        blob = f.read()
    i = rt_accum_info()
    rc = lib().rt_noise_blob_info(blob, len(blob), ctypes.byref(i))
    if rc != 0:
        raise RtError(f"rt_noise_blob_info({path!r}) failed ({rc})", rc)
    d = i.as_dict()
    rows, width = d["n_values"] // (3 * d["width"]), d["width"]
    ty, tx = (rows + 15) // 16, (width + 15) // 16
    tile_max, tile_above = np.zeros((ty, tx), np.float32), np.zeros((ty, tx), np.int32)
    nmap = np.zeros((rows, width), np.float32)
    rep = rt_noise_report()
    rc = lib().rt_noise_blob_measure(blob, len(blob), threshold, ctypes.byref(rep), tile_max.ctypes.data,
                                     tile_above.ctypes.data, nmap.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_noise_blob_measure({path!r}) failed ({rc})", rc)
    return {**d, **rep.as_dict()}, tile_max, tile_above, nmap


def _denoise_file(path: str, info_fn, fn, what: str, params, gain: bool, guide=None, guide_params_=None):
    with open(path, "rb") as f:
        blob = f.read()
    if guide is not None:  # planes as Guide.planes(png_order=False) / guide_host() give them
        nrm, alb, dep = (np.ascontiguousarray(guide[k], np.float32) for k in ("normal", "albedo", "depth"))
        if nrm.shape != dep.shape + (3,) or alb.shape != nrm.shape or dep.ndim != 2:
            raise ValueError("guide planes: normal and albedo (rows, width, 3), depth (rows, width)")
        gp, plain = guide_params(guide_params_), fn
        fn = lambda b, n, p, img, g: plain(b, n, p, ctypes.byref(gp), nrm.ctypes.data, alb.ctypes.data, dep.ctypes.data,  # noqa: E731
                                           dep.shape[1], dep.shape[0], img, g)
    i = rt_accum_info()
    rc = info_fn(blob, len(blob), ctypes.byref(i))
    if rc != 0:
        raise RtError(f"{what}({path!r}): malformed file ({rc})", rc)

    def check(rc, what):
        if rc != 0:
            raise RtError(f"{what}({path!r}) failed ({rc})", rc)

    return _denoise_call(check, lambda _, p, img, g, __: fn(blob, len(blob), p, img, g), what, None, params,
                         i.n_values // (3 * i.args.width), i.args.width, False, gain)


def denoise_checkpoint(path: str, params=None, gain: bool = False, guide=None, guide_params=None):
    """NoiseMonitor.denoise() of a monitor's side file (the checkpoint's ".noise"), by the host-only
    rt_denoise_monitor_blob (no context, no GPU), byte-identical to the device's: (rows, width, 3) uint8 with
    rows ascending (bottom row first), and with gain=True the (rows, width) float32 gain too.  guide: a dict of
    the planes "normal", "albedo", "depth" with rows ascending (guide_host(), Guide.planes(png_order=False)):
    the guided denoise, by rt_guide_denoise_monitor_blob."""
    if guide is not None:
        return _denoise_file(path, lib().rt_noise_blob_info, lib().rt_guide_denoise_monitor_blob, "rt_guide_denoise_monitor_blob",
                             params, gain, guide, guide_params)
    return _denoise_file(path, lib().rt_noise_blob_info, lib().rt_denoise_monitor_blob, "rt_denoise_monitor_blob", params, gain)


def denoise_adaptive_checkpoint(path: str, params=None, gain: bool = False, guide=None, guide_params=None):
    """AdaptiveAccumulator.denoise() of an adaptive checkpoint file, by the host-only rt_denoise_adaptive_blob
    (with guide planes: rt_guide_denoise_adaptive_blob, see denoise_checkpoint)."""
    if guide is not None:
        return _denoise_file(path, lib().rt_adaptive_blob_info, lib().rt_guide_denoise_adaptive_blob,
                             "rt_guide_denoise_adaptive_blob", params, gain, guide, guide_params)
    return _denoise_file(path, lib().rt_adaptive_blob_info, lib().rt_denoise_adaptive_blob, "rt_denoise_adaptive_blob", params,
                         gain)


# ---------------------------------------------------------------- ray casts and feature buffers
def _soa_of(scene) -> rt_scene_soa:
    return getattr(scene, "soa", scene)  # a Scene (or anything that carries its rt_scene_soa), or the struct itself


def _rays(rays) -> np.ndarray:
    r = np.ascontiguousarray(rays, np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError("rays: (n, 8) float32 -- o[3], d[3], time, unused")
    return r


class Guide:
    """rt_guide of include/rt_hip.h: ray casts into a scene (a Scene or an rt_scene_soa) and the noise-free
    feature planes of its camera -- normal, albedo, depth, primitive id -- for picking, AOV images and the
    guided denoise (NoiseMonitor.denoise(guide=...)).  It holds its own copy of the scene on the device."""

    def __init__(self, scene, device: int = 0):
        h = c_void_p()
        rc = lib().rt_guide_create(ctypes.byref(_soa_of(scene)), device, ctypes.byref(h))
        if rc != 0:
            raise RtError(f"rt_guide_create failed ({rc})", rc)
        self._h = h
        self.width = self.height = 0

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            raise RtError(f"{what} failed ({rc})", rc)

    def cast(self, rays) -> np.ndarray:
        """The first hit of every ray ((n, 8) float32: o, d, time, unused) as a structured array of
        GUIDE_HIT_DTYPE: t, p, n, albedo, u, v, prim (-1: a miss), material, front."""
        r = _rays(rays)
        out = np.zeros(len(r), GUIDE_HIT_DTYPE)
        self._check(lib().rt_guide_cast(self._h, r.ctypes.data, len(r), out.ctypes.data), "rt_guide_cast")
        return out

    def cast_into(self, rays_ptr: int, n: int, out_ptr: int) -> None:
        """cast() between caller memory (device or host addresses)."""
        self._check(lib().rt_guide_cast(self._h, c_void_p(rays_ptr), n, c_void_p(out_ptr)), "rt_guide_cast")

    def trace(self, rays, **spec) -> tuple[np.ndarray, np.ndarray]:
        """cast() through mirrors and glass (rt_spec_cast): (hits, paths), the last surface of every ray's chain as
        GUIDE_HIT_DTYPE and the chain as SPEC_PATH_DTYPE: bounces, status (SPEC_*), first_prim, first_material,
        throughput, depth.  spec: the fields of spec_params()."""
        r, p = _rays(rays), spec_params(**spec)
        hits, paths = np.zeros(len(r), GUIDE_HIT_DTYPE), np.zeros(len(r), SPEC_PATH_DTYPE)
        self._check(lib().rt_spec_cast(self._h, r.ctypes.data, len(r), ctypes.byref(p), hits.ctypes.data, paths.ctypes.data),
                    "rt_spec_cast")
        return hits, paths

    def render(self, width: int, height: int, samples: int | None = None, lens: bool = True, footprint: bool = True,
               shutter: bool = True, specular=None) -> "Guide":
        """The centre ray of every pixel into the guide's planes; with samples=S the average of S rays per pixel
        spread over the lens, the pixel's footprint and the shutter (rt_aov_render), which also keeps coverage().
        specular=True, a bounce limit or what spec_params() takes: the planes of what mirrors and glass show
        (rt_spec_render; coverage() is kept); None or False changes nothing."""
        if specular is not None and specular is not False:
            sp = spec_params(specular)
            self._check(lib().rt_spec_render(self._h, width, height, _centre_or(samples, lens, footprint, shutter), ctypes.byref(sp)),
                        "rt_spec_render")
        elif samples is None:
            self._check(lib().rt_guide_render(self._h, width, height), "rt_guide_render")
        else:
            p = aov_params(samples=samples, lens=lens, footprint=footprint, shutter=shutter)
            self._check(lib().rt_aov_render(self._h, width, height, ctypes.byref(p)), "rt_aov_render")
        self.width, self.height = width, height
        return self

    def coverage(self, png_order: bool = True) -> np.ndarray:
        """(H, W) float32: the share of a pixel's samples that hit something, of the last render(samples=S)."""
        out = np.zeros((self.height, self.width), np.float32)
        self._check(lib().rt_aov_coverage(self._h, out.ctypes.data, 1 if png_order else 0), "rt_aov_coverage")
        return out

    def planes(self, png_order: bool = False) -> dict:
        """{"normal", "albedo": (H, W, 3) float32, "depth": (H, W) float32, "prim": (H, W) int32} of the last
        render(); row 0 the bottom row unless png_order."""
        H, W = self.height, self.width
        d = {"normal": np.zeros((H, W, 3), np.float32), "albedo": np.zeros((H, W, 3), np.float32),
             "depth": np.zeros((H, W), np.float32), "prim": np.zeros((H, W), np.int32)}
        self._check(lib().rt_guide_planes(self._h, d["normal"].ctypes.data, d["albedo"].ctypes.data, d["depth"].ctypes.data,
                                          d["prim"].ctypes.data, 1 if png_order else 0), "rt_guide_planes")
        return d

    def image(self, which: str, png_order: bool = True) -> np.ndarray:
        """The 8-bit picture of the "normal" or "albedo" plane, (H, W, 3) uint8."""
        if which not in ("normal", "albedo"):
            raise ValueError('which: "normal" or "albedo"')
        out = np.zeros((self.height, self.width, 3), np.uint8)
        self._check(lib().rt_guide_image(self._h, 0 if which == "normal" else 1, out.ctypes.data, 1 if png_order else 0),
                    "rt_guide_image")
        return out

    def last_ms(self) -> float:
        """Device time of the last cast() / render() kernel."""
        return float(lib().rt_guide_last_ms(self._h))

    def last_spec_ms(self) -> float:
        """Device time of the last trace() / render(specular=...) kernel."""
        return float(lib().rt_spec_last_ms(self._h))

    def last_aov_ms(self) -> float:
        """Device time of the last render(samples=S) kernel."""
        return float(lib().rt_aov_last_ms(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().rt_guide_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cast_host(scene, rays) -> np.ndarray:
    """Guide.cast() on the host (rt_guide_cast_host: no GPU), bit-identical to the device's."""
    r = _rays(rays)
    out = np.zeros(len(r), GUIDE_HIT_DTYPE)
    rc = lib().rt_guide_cast_host(ctypes.byref(_soa_of(scene)), r.ctypes.data, len(r), out.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_guide_cast_host failed ({rc})", rc)
    return out


def trace_host(scene, rays, **spec) -> tuple[np.ndarray, np.ndarray]:
    """Guide.trace() on the host (rt_spec_cast_host: no GPU), bit-identical to the device's."""
    r, p = _rays(rays), spec_params(**spec)
    hits, paths = np.zeros(len(r), GUIDE_HIT_DTYPE), np.zeros(len(r), SPEC_PATH_DTYPE)
    rc = lib().rt_spec_cast_host(ctypes.byref(_soa_of(scene)), r.ctypes.data, len(r), ctypes.byref(p), hits.ctypes.data,
                                 paths.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_spec_cast_host failed ({rc})", rc)
    return hits, paths


def guide_host(scene, width: int, height: int, samples: int | None = None, lens: bool = True, footprint: bool = True,
               shutter: bool = True, specular=None) -> dict:
    """Guide.render(width, height).planes() on the host (rt_guide_render_host: no GPU); with samples=S
    Guide.render(width, height, S, ...)'s (rt_aov_render_host), and "coverage" (H, W) float32 beside them; with
    specular=... Guide.render(..., specular=...)'s (rt_spec_render_host), with "coverage" too."""
    d = {"normal": np.zeros((height, width, 3), np.float32), "albedo": np.zeros((height, width, 3), np.float32),
         "depth": np.zeros((height, width), np.float32), "prim": np.zeros((height, width), np.int32)}
    if specular is not None and specular is not False:
        d["coverage"] = np.zeros((height, width), np.float32)
        sp = spec_params(specular)
        rc = lib().rt_spec_render_host(ctypes.byref(_soa_of(scene)), width, height, _centre_or(samples, lens, footprint, shutter),
                                       ctypes.byref(sp), d["normal"].ctypes.data, d["albedo"].ctypes.data, d["depth"].ctypes.data,
                                       d["prim"].ctypes.data, d["coverage"].ctypes.data)
        if rc != 0:
            raise RtError(f"rt_spec_render_host failed ({rc})", rc)
        return d
    if samples is not None:
        d["coverage"] = np.zeros((height, width), np.float32)
        p = aov_params(samples=samples, lens=lens, footprint=footprint, shutter=shutter)
        rc = lib().rt_aov_render_host(ctypes.byref(_soa_of(scene)), width, height, ctypes.byref(p), d["normal"].ctypes.data,
                                      d["albedo"].ctypes.data, d["depth"].ctypes.data, d["prim"].ctypes.data,
                                      d["coverage"].ctypes.data)
        if rc != 0:
            raise RtError(f"rt_aov_render_host failed ({rc})", rc)
        return d
    rc = lib().rt_guide_render_host(ctypes.byref(_soa_of(scene)), width, height, d["normal"].ctypes.data, d["albedo"].ctypes.data,
                                    d["depth"].ctypes.data, d["prim"].ctypes.data)
    if rc != 0:
        raise RtError(f"rt_guide_render_host failed ({rc})", rc)
    return d


def read_checkpoint(path: str) -> tuple[dict, np.ndarray]:
    """(info, image) of a checkpoint file, by the host-only rt_accum_blob_* functions (no context, no
    GPU): info as Accumulator.info(), image (owned_rows, width, 3) uint8 with owned rows ascending
    (bottom row first for a whole image)."""
    with open(path, "rb") as f:
        blob = f.read()
    i = rt_accum_info()
    rc = lib().rt_accum_blob_info(blob, len(blob), ctypes.byref(i))
    if rc != 0:
        raise RtError(f"rt_accum_blob_info({path!r}) failed ({rc})", rc)
    d = i.as_dict()
    img = np.zeros((d["n_values"] // (3 * d["width"]), d["width"], 3), np.uint8)
    rc = lib().rt_accum_blob_image(blob, len(blob), img.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_accum_blob_image({path!r}) failed ({rc})", rc)
    return d, img


def read_adaptive_checkpoint(path: str, threshold: float | None = None) -> tuple:
    """(info, image, counts, active) of an adaptive checkpoint file and, with a threshold, (..., report,
    noise map) too, by the host-only rt_adaptive_blob_* functions (no context, no GPU).  info as
    Accumulator.info() with fb_count = the largest count; image (owned_rows, width, 3) uint8 with owned rows
    ascending (None before the first frame buffer); counts int32 and active bool, (tiles_y, tiles_x)."""
    with open(path, "rb") as f:
        blob = f.read()
    i = rt_accum_info()
    rc = lib().rt_adaptive_blob_info(blob, len(blob), ctypes.byref(i))
    if rc != 0:
        raise RtError(f"rt_adaptive_blob_info({path!r}) failed ({rc})", rc)
    d = i.as_dict()
    rows, width = d["n_values"] // (3 * d["width"]), d["width"]
    ty, tx = (rows + 15) // 16, (width + 15) // 16
    counts, active = np.zeros((ty, tx), np.int32), np.zeros((ty, tx), np.uint8)
    rc = lib().rt_adaptive_blob_tiles(blob, len(blob), counts.ctypes.data, active.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_adaptive_blob_tiles({path!r}) failed ({rc})", rc)
    img = None
    if d["fb_count"] > 0:
        img = np.zeros((rows, width, 3), np.uint8)
        rc = lib().rt_adaptive_blob_image(blob, len(blob), img.ctypes.data)
        if rc != 0:
            raise RtError(f"rt_adaptive_blob_image({path!r}) failed ({rc})", rc)
    if threshold is None:
        return d, img, counts, active.astype(bool)
    rep = rt_adapt_report()
    nmap = np.zeros((rows, width), np.float32)
    rc = lib().rt_adaptive_blob_measure(blob, len(blob), threshold, ctypes.byref(rep), None, None, nmap.ctypes.data)
    if rc != 0:
        raise RtError(f"rt_adaptive_blob_measure({path!r}) failed ({rc})", rc)
    return d, img, counts, active.astype(bool), rep.as_dict(), nmap


def _final_denoise(target, denoise, curr_scene: Scene, settings: render_settings, device: int):
    """target.denoise(denoise).  A dict with guide=True (and, if wanted, guide_params=...) beside the denoiser's
    fields takes the guided filter: a Guide of the scene on the draw's device, rendered at the image's size; with
    guide_samples=S its planes are the averages of S rays per pixel (Guide.render(..., samples=S)), with
    guide_specular=... they follow mirrors and glass (Guide.render(..., specular=...))."""
    if isinstance(denoise, dict) and any(k in denoise for k in ("guide", "guide_params", "guide_samples", "guide_specular")):
        fields = dict(denoise)
        use, gains, samples = fields.pop("guide", False), fields.pop("guide_params", None), fields.pop("guide_samples", None)
        specular = fields.pop("guide_specular", None)
        if use:
            g = Guide(curr_scene, device)
            try:
                g.render(settings.image_width, settings.image_height, samples, specular=specular)
                return target.denoise(fields, guide=g, guide_params=gains)
            finally:
                g.close()
        denoise = fields
    return target.denoise(denoise)


def draw_progressive(curr_scene: Scene, settings: render_settings, ctx: Context | None = None, every: int = 1,
                     on_image=None, checkpoint: str | None = None, chunk_fbs: int | None = None,
                     cam_mode: int = RT_CAM_REF_SLOT0, seed: int = 1984, until_noise: float | None = None,
                     noisy_fraction: float = 0.01, min_fbs: int = 2, on_noise=None, denoise=None) -> tuple[np.ndarray, dict]:
    """draw() of render.h:118-174 in steps of `every` frame buffers: after each step
    on_image(image, fbs_done) gets the PNG-order image so far (the reference leaves tmp/<id>.ppm
    behind, render.h:152-162) and, with a checkpoint path, the state is saved there (temporary name,
    then rename).  An existing checkpoint of the same scene and settings is continued; one of another
    scene or other settings raises.  Returns (final image, counters of the frame buffers rendered by
    this call); the image is byte-identical to draw()'s.  chunk_fbs: frame buffers per render launch
    (default: every).

    until_noise=T attaches a noise monitor (NoiseMonitor; None changes nothing).  After each step
    with done >= max(2, min_fbs) frame buffers it is measured with threshold T (8-bit output levels),
    on_noise(report, done) is called, and the draw stops early once pixels_above <=
    floor(noisy_fraction * pixels); settings.no_fb stays the upper limit.  The image returned after
    `done` frame buffers is byte-identical to draw() with no_fb = done.  With a checkpoint the monitor
    is saved to checkpoint + ".noise" before the checkpoint itself, and a resumed draw is measured
    before it renders anything (a draw that had converged stays stopped).  Resuming needs that side
    file: a missing one, or one whose header differs from the checkpoint's, raises RtError -- the
    statistics are never silently restarted from a later frame buffer.

    denoise=True (the shipped parameters) or parameters as denoise_params() takes them (a dict may also hold
    guide=True for the feature-guided filter, guide_params, guide_samples=S for planes averaged over S rays
    per pixel and guide_specular=... for planes that follow mirrors and glass): a noise monitor is
    attached if until_noise has not attached one (it never stops the draw then), and the image returned is
    NoiseMonitor.denoise() of the final state instead of the plain one (needs two frame buffers); on_image
    still gets the plain images.  None leaves the function exactly as it is without it."""
    if settings.image_height <= 0:
        settings.aspect_ratio = curr_scene.aspect
        settings.calc_all()
    if every < 1:
        raise ValueError("every < 1")
    want_mon = until_noise is not None or denoise is not None
    if want_mon and settings.no_fb > NOISE_MAX_FBS:
        raise ValueError(f"a noise monitor accepts at most {NOISE_MAX_FBS} frame buffers")
    own = ctx is None
    ctx = ctx or Context(0)
    acc = mon = None

    def converged() -> bool:
        if until_noise is None or acc.done < max(2, min_fbs):
            return False
        report = mon.measure(until_noise)[0]
        if on_noise is not None:
            on_noise(report, acc.done)
        return report["pixels_above"] <= math.floor(noisy_fraction * report["pixels"])

    try:
        ctx.upload(curr_scene)
        args = make_args(settings.image_width, settings.image_height, settings.samples_per_pixel_per_fb,
                         0, 1, settings.max_depth, cam_mode, seed=seed)
        chunk = chunk_fbs or every
        if checkpoint and os.path.exists(checkpoint):
            acc = Accumulator.load(ctx, checkpoint, chunk)
            got, want = acc.info(), rt_accum_info(args, 0, 0).as_dict()
            differ = [k for k in want if k not in ("fb_count", "n_values", "scene_fp") and got[k] != want[k]]
            if differ or got["fb_count"] > settings.no_fb:
                raise RtError(f"checkpoint {checkpoint!r} is of another draw: {differ or 'more frame buffers'}")
            if want_mon:
                side = checkpoint + ".noise"
                if not os.path.exists(side):
                    raise RtError(f"checkpoint {checkpoint!r} has no noise side file {side!r}: the draw cannot "
                                  "continue with until_noise or denoise (the statistics must cover every frame buffer)")
                mon = NoiseMonitor.load(acc, side)
        else:
            acc = ctx.accumulator(args, chunk)
            if want_mon:
                mon = acc.noise_monitor()
        total = rt_counters().as_dict()
        img = acc.image(png_order=True) if acc.done else None
        stop = acc.done > 0 and converged()
        while acc.done < settings.no_fb and not stop:
            cnt = acc.add(min(every, settings.no_fb - acc.done))
            total = {k: total[k] + cnt[k] for k in total}
            img = acc.image(png_order=True)
            if checkpoint:
                if mon is not None:
                    mon.save(checkpoint + ".noise")
                acc.save(checkpoint)
            stop = converged()
            if on_image is not None:
                on_image(img, acc.done)
        if denoise is not None:
            img = _final_denoise(mon, denoise, curr_scene, settings, ctx.device)
        return img, total
    finally:
        if acc is not None:
            acc.close()
        if own:
            ctx.close()


def draw_adaptive(curr_scene: Scene, settings: render_settings, ctx: Context | None = None, every: int = 1,
                  until_noise: float = 0.5, max_above: int = 0, min_fbs: int = 4, on_image=None, on_step=None,
                  cam_mode: int = RT_CAM_REF_SLOT0, seed: int = 1984, chunk_fbs: int | None = None,
                  checkpoint: str | None = None, dilate: int = 0,
                  reopen: bool = False, denoise=None) -> tuple[np.ndarray, dict, np.ndarray]:
    """draw() that stops rendering a 16 x 16 tile once at most max_above of its pixels have a noise
    estimate above until_noise (8-bit output levels; NoiseMonitor's definition), and goes on with the
    others.  Each step adds `every` frame buffers to the active tiles, none beyond settings.no_fb; from
    max(2, min_fbs) frame buffers on it then retires tiles and calls on_step(report, done); on_image(image,
    done) gets the PNG-order image after every step.  Ends when no tile is active or every active tile is at
    settings.no_fb.  Returns (image, counters of everything rendered by this call, counts): tile t of the
    image is byte-identical to draw() with no_fb = counts[t].  Stopping a tile on its own samples' spread
    biases it slightly towards stopping while it happens to look smooth; min_fbs guards against that, and
    dilate = r keeps the passing tiles within r tiles of a failing one active too.

    With a checkpoint path the state is saved there after every step (temporary name, then rename).  An
    existing checkpoint of the same scene and settings is continued, byte-identically to a draw that never
    stopped; one of another scene, of other settings or with more frame buffers than settings.no_fb raises
    RtError.  reopen=True on a resumed draw first makes the tiles that fail until_noise / max_above (and
    their neighbours within dilate) active again, each from its own count: a finished draw refined to a
    tighter threshold.

    denoise=True (the shipped parameters) or parameters as denoise_params() takes them (a dict may also hold
    guide=True for the feature-guided filter, guide_params, guide_samples=S for planes averaged over S rays
    per pixel and guide_specular=... for planes that follow mirrors and glass): the image returned is
    AdaptiveAccumulator.denoise() of the final state, every pixel at its own tile's count, instead of the plain
    one (every tile needs two frame buffers); on_image still gets the plain images."""
    if settings.image_height <= 0:
        settings.aspect_ratio = curr_scene.aspect
        settings.calc_all()
    if every < 1:
        raise ValueError("every < 1")
    if settings.no_fb > NOISE_MAX_FBS:
        raise ValueError(f"an adaptive draw accepts at most {NOISE_MAX_FBS} frame buffers")
    own = ctx is None
    ctx = ctx or Context(0)
    ad = None
    try:
        ctx.upload(curr_scene)
        args = make_args(settings.image_width, settings.image_height, settings.samples_per_pixel_per_fb,
                         0, 1, settings.max_depth, cam_mode, seed=seed)
        done, active = 0, True
        if checkpoint and os.path.exists(checkpoint):
            ad = AdaptiveAccumulator.load(ctx, checkpoint, chunk_fbs or every)
            got, want = read_adaptive_checkpoint(checkpoint)[0], rt_accum_info(args, 0, 0).as_dict()
            differ = [k for k in want if k not in ("fb_count", "n_values", "scene_fp") and got[k] != want[k]]
            if differ or got["fb_count"] > settings.no_fb:
                raise RtError(f"checkpoint {checkpoint!r} is of another draw: {differ or 'more frame buffers'}")
            done = got["fb_count"]
            if reopen and done >= 2:
                ad.reopen(until_noise, max_above, dilate)
            act = ad.active()
            active = bool((act & (ad.counts() < settings.no_fb)).any())
        else:
            ad = ctx.adaptive(args, chunk_fbs or every)
        total = rt_counters().as_dict()
        img = None
        while active:
            cnt = ad.add(every, limit=settings.no_fb)
            counts = ad.counts()
            done = int(counts.max())
            total = {k: total[k] + cnt[k] for k in total}
            act = ad.active()
            if done >= max(2, min_fbs):
                report = ad.retire(until_noise, max_above, dilate)
                act = ad.active()
            active = bool((act & (counts < settings.no_fb)).any())
            if checkpoint:
                ad.save(checkpoint)
            if done >= max(2, min_fbs) and on_step is not None:
                on_step(report, done)
            if on_image is not None:
                on_image(ad.image(png_order=True), done)
        if done:
            img = ad.image(png_order=True) if denoise is None else _final_denoise(ad, denoise, curr_scene, settings, ctx.device)
        return img, total, ad.counts()
    finally:
        if ad is not None:
            ad.close()
        if own:
            ctx.close()


def draw(curr_scene: Scene, settings: render_settings, ctx: Context | None = None,
         cam_mode: int = RT_CAM_REF_SLOT0, seed: int = 1984) -> tuple[np.ndarray, dict]:
    """draw() of render.h:118-174: returns (PNG-order HxWx3 uint8 image, counters)."""
    if settings.image_height <= 0:
        settings.aspect_ratio = curr_scene.aspect
        settings.calc_all()
    own = ctx is None
    ctx = ctx or Context(0)
    try:
        ctx.upload(curr_scene)
        args = make_args(settings.image_width, settings.image_height, settings.samples_per_pixel_per_fb,
                         0, settings.no_fb, settings.max_depth, cam_mode, seed=seed)
        return ctx.draw_args(args)
    finally:
        if own:
            ctx.close()


def write_png(path: str, img: np.ndarray) -> None:
    from PIL import Image

    Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8), "RGB").save(path)
