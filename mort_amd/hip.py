"""ctypes binding of libmort_hip.so (include/mort_hip.h): the gfx950 render path.

There is no CPU fallback: if the library is missing or no MI355X is present
every call raises.  The four call sites of the reference this replaces are
world::toDevice() (world.cuh:98-102), setup_rng<<<>>> (mort.cu:709), the
per-bounce scratch allocations (mort.cu:712-725) and renderKernel<<<>>>
(mort.cu:106).
"""
import ctypes as C
import os

import numpy as np

from . import structs as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MORT_HIP_LIB") or os.path.join(_HERE, "lib", "libmort_hip.so")  # override: debug builds only
_lib = None

MODE_MEGA = 0
MODE_WAVE = 1
MODE_THROUGHPUT = 2  # non-parity: one stream per (pixel, stratum row); see include/mort_hip.h

EXPORTS = [
    "mort_hip_strerror", "mort_hip_last_error", "mort_hip_init", "mort_hip_shutdown", "mort_hip_upload_world",
    "mort_hip_set_partition", "mort_hip_rng_seed", "mort_hip_rng_load", "mort_hip_rng_store", "mort_hip_render",
    "mort_hip_render_device", "mort_hip_local_rows", "mort_hip_global_row", "mort_hip_rng_seed_host", "mort_hip_render_host",
    "mort_hip_comm_id", "mort_hip_comm_init", "mort_hip_comm_destroy", "mort_hip_render_gather", "mort_hip_comm_selftest",
    "mort_hip_calib_valu", "mort_hip_calib_hbm_copy",
    "mort_hip_denoise_defaults", "mort_hip_render_features", "mort_hip_render_features_device", "mort_hip_denoise",
    "mort_hip_denoise_device", "mort_hip_render_features_host", "mort_hip_denoise_host",
    "mort_hip_temporal_defaults", "mort_hip_temporal", "mort_hip_temporal_device", "mort_hip_temporal_host",
    "mort_hip_svgf_defaults", "mort_hip_svgf", "mort_hip_svgf_device", "mort_hip_svgf_host",
    "mort_hip_view_defaults", "mort_hip_view_check_params", "mort_hip_view_create", "mort_hip_view_destroy", "mort_hip_view_reset",
    "mort_hip_view_frame", "mort_hip_view_frame_device", "mort_hip_view_read",
    "mort_hip_query_closest", "mort_hip_query_closest_device", "mort_hip_query_closest_host",
    "mort_hip_query_occluded", "mort_hip_query_occluded_device", "mort_hip_query_occluded_host",
    "mort_hip_radiance_params_from_camera", "mort_hip_query_radiance", "mort_hip_query_radiance_device", "mort_hip_query_radiance_host",
    "mort_hip_probe_directions", "mort_hip_probe_bake", "mort_hip_probe_bake_device", "mort_hip_probe_bake_host", "mort_hip_sh9_irradiance",
    "mort_hip_volume_probes", "mort_hip_volume_pack", "mort_hip_volume_pack_device", "mort_hip_volume_pack_host",
    "mort_hip_volume_sample", "mort_hip_volume_sample_device", "mort_hip_volume_sample_host",
    "mort_hip_probe_depth_bake", "mort_hip_probe_depth_bake_device", "mort_hip_probe_depth_bake_host",
    "mort_hip_volume_sample_visible", "mort_hip_volume_sample_visible_device", "mort_hip_volume_sample_visible_host",
    "mort_hip_query_radiance_cached", "mort_hip_query_radiance_cached_device", "mort_hip_query_radiance_cached_host",
    "mort_hip_render_cached", "mort_hip_render_cached_device", "mort_hip_render_cached_host", "mort_hip_view_set_cache",
    "mort_hip_view_set_cache_host",
    "mort_hip_volume_refresh", "mort_hip_volume_refresh_device", "mort_hip_volume_refresh_host", "mort_hip_probe_directions_round",
    "mort_hip_view_update_cache", "mort_hip_view_update_cache_host",
    "mort_hip_query_radiance_cached_direct", "mort_hip_query_radiance_cached_direct_device", "mort_hip_query_radiance_cached_direct_host",
    "mort_hip_render_cached_direct", "mort_hip_render_cached_direct_device", "mort_hip_render_cached_direct_host",
    "mort_hip_view_set_cache_direct", "mort_hip_view_set_cache_direct_host",
    "mort_hip_volume_refresh_direct", "mort_hip_volume_refresh_direct_device", "mort_hip_volume_refresh_direct_host",
    "mort_hip_debug_tile_state", "mort_hip_debug_tile_sort", "mort_hip_debug_heavy_count", "mort_hip_debug_deinterleave",
]
TILE_COUNTERS = 96
TEMPORAL_HISTORY_FLOATS = 12
FILTER_NONE, FILTER_DENOISE, FILTER_SVGF = 0, 1, 2
# mort_hip_view_read: name -> (MORT_VIEW_* code, floats per pixel)
VIEW_BUFFERS = {"raw_accum": (0, 3), "accum": (1, 3), "filtered": (2, 3), "variance": (3, 1), "albedo": (4, 3), "normal": (5, 3),
                "depth": (6, 1), "history": (7, TEMPORAL_HISTORY_FLOATS), "ends": (8, 1), "lit": (9, 1)}
HOST_TREE = 1
# ray queries (mort_ray, mort_hit of include/mort_hip.h)
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("dir", "<f4", (3,)), ("time", "<f4"), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("p", "<f4", (3,)), ("normal", "<f4", (3,)), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("mat_type", "<i4"),
                      ("mat_idx", "<i4"), ("flags", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 48
HIT_HIT, HIT_FRONT_FACE, HIT_MEDIUM = 1, 2, 4


class RADIANCE_PARAMS(C.Structure):
    """mort_radiance_params of include/mort_hip.h"""
    _fields_ = [("bounce_limit", C.c_int), ("samples", C.c_int), ("background", C.c_float * 3),
                ("light_obj_type", C.c_int), ("light_obj_idx", C.c_int)]


# light probes (mort_probe, mort_probe_params of include/mort_hip.h)
PROBE_DTYPE = np.dtype([("position", "<f4", (3,)), ("time", "<f4")])
assert PROBE_DTYPE.itemsize == 16
SH9_FLOATS = 27


class PROBE_PARAMS(C.Structure):
    """mort_probe_params of include/mort_hip.h"""
    _fields_ = [("rp", RADIANCE_PARAMS), ("directions", C.c_int)]

    def __init__(self, rp=None, directions=256):
        super().__init__()
        if rp is not None:
            C.memmove(C.byref(self.rp), C.byref(rp), C.sizeof(RADIANCE_PARAMS))
        self.directions = directions


# irradiance volumes (mort_volume_grid, mort_volume_point of include/mort_hip.h)
VOLUME_POINT_DTYPE = np.dtype([("p", "<f4", (3,)), ("normal", "<f4", (3,))])
assert VOLUME_POINT_DTYPE.itemsize == 24
VOLUME_RECORD_FLOATS = 32
VOLUME_MAX_COUNT = 4096


class VOLUME_GRID(C.Structure):
    """mort_volume_grid of include/mort_hip.h: probe (ix, iy, iz) sits at origin + i * spacing, index (iz * ny + iy) * nx + ix"""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("count", C.c_int32 * 3), ("time", C.c_float)]

    def __init__(self, origin=(0, 0, 0), spacing=(1, 1, 1), count=(1, 1, 1), time=0.0):
        super().__init__()
        for a in range(3):
            self.origin[a], self.spacing[a], self.count[a] = origin[a], spacing[a], count[a]
        self.time = time

    @property
    def probes(self):
        return self.count[0] * self.count[1] * self.count[2]


# visibility-weighted irradiance volumes (mort_depth_params, mort_volume_vis_params of include/mort_hip.h)
DEPTH_RES = 8
DEPTH_FLOATS = 200


class DEPTH_PARAMS(C.Structure):
    """mort_depth_params of include/mort_hip.h: s x s rays per texel, distances capped at max_distance"""
    _fields_ = [("subsamples", C.c_int), ("max_distance", C.c_float)]

    def __init__(self, subsamples=2, max_distance=1.0):
        super().__init__()
        self.subsamples, self.max_distance = subsamples, max_distance


class VOLUME_VIS_PARAMS(C.Structure):
    """mort_volume_vis_params of include/mort_hip.h"""
    _fields_ = [("normal_bias", C.c_float), ("min_visibility", C.c_float)]

    def __init__(self, normal_bias=0.0, min_visibility=0.05):
        super().__init__()
        self.normal_bias, self.min_visibility = normal_bias, min_visibility


# cached radiance queries (mort_cached_params of include/mort_hip.h)
CACHED_VISIBLE = 1


class CACHED_PARAMS(C.Structure):
    """mort_cached_params of include/mort_hip.h: a radiance query whose paths end in the volume `grid` from bounce cache_depth on;
    vis (VOLUME_VIS_PARAMS) sets MORT_CACHED_VISIBLE"""
    _fields_ = [("path", RADIANCE_PARAMS), ("cache_depth", C.c_int32), ("flags", C.c_uint32), ("grid", VOLUME_GRID),
                ("vis", VOLUME_VIS_PARAMS)]

    def __init__(self, path=None, cache_depth=1, grid=None, vis=None):
        super().__init__()
        if path is not None:
            C.memmove(C.byref(self.path), C.byref(path), C.sizeof(RADIANCE_PARAMS))
        if grid is not None:
            C.memmove(C.byref(self.grid), C.byref(grid), C.sizeof(VOLUME_GRID))
        self.cache_depth = cache_depth
        self.vis.normal_bias, self.vis.min_visibility = (vis.normal_bias, vis.min_visibility) if vis is not None else (0.0, 0.0)
        self.flags = CACHED_VISIBLE if vis is not None else 0


class CACHED_FRAME_PARAMS(C.Structure):
    """mort_cached_frame_params of include/mort_hip.h: a render whose paths end in the volume `grid` from bounce cache_depth on;
    vis (VOLUME_VIS_PARAMS) sets MORT_CACHED_VISIBLE.  Bounce limit, background, light object and samples are the camera's."""
    _fields_ = [("cache_depth", C.c_int32), ("flags", C.c_uint32), ("grid", VOLUME_GRID), ("vis", VOLUME_VIS_PARAMS)]

    def __init__(self, cache_depth=1, grid=None, vis=None):
        super().__init__()
        if grid is not None:
            C.memmove(C.byref(self.grid), C.byref(grid), C.sizeof(VOLUME_GRID))
        self.cache_depth = cache_depth
        self.vis.normal_bias, self.vis.min_visibility = (vis.normal_bias, vis.min_visibility) if vis is not None else (0.0, 0.0)
        self.flags = CACHED_VISIBLE if vis is not None else 0


class REFRESH_PARAMS(C.Structure):
    """mort_refresh_params of include/mort_hip.h: the probes first, first + step, ... of cached.grid re-baked through the volume
    (cached: CACHED_PARAMS, its path.samples the paths per direction) along `directions` directions and blended under `hysteresis`"""
    _fields_ = [("cached", CACHED_PARAMS), ("directions", C.c_int32), ("hysteresis", C.c_float), ("first", C.c_uint32), ("step", C.c_uint32)]

    def __init__(self, cached=None, directions=256, hysteresis=0.9, first=0, step=1):
        super().__init__()
        if cached is not None:
            C.memmove(C.byref(self.cached), C.byref(cached), C.sizeof(CACHED_PARAMS))
        self.directions, self.hysteresis, self.first, self.step = directions, hysteresis, first, step

    def selected(self):
        """how many probes first, first + step, ... the grid holds"""
        P = self.cached.grid.probes
        return (P - 1 - self.first) // self.step + 1 if self.step and self.first < P else 0


class Partition(C.Structure):
    _fields_ = [("rank", C.c_int), ("nranks", C.c_int), ("rows_per_block", C.c_int)]


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("segments", C.c_uint64), ("pixels", C.c_uint64),
                ("eff_samples", C.c_uint64), ("rng_draws", C.c_uint64), ("algorithmic_hbm_bytes", C.c_uint64),
                ("scene_in_lds", C.c_int), ("local_rows", C.c_int), ("kernel_vgprs", C.c_int),
                ("kernel_lds_bytes", C.c_int), ("reference_walks", C.c_uint64), ("kernel_name", C.c_char * 64), ("gather_seconds", C.c_double)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["kernel_name"] = d["kernel_name"].decode()
        return d


class CalibValu(C.Structure):
    _fields_ = [("waves_per_simd", C.c_int), ("kind", C.c_int), ("seconds", C.c_double), ("cycles_per_wave", C.c_double),
                ("clock_ghz", C.c_double), ("valu_per_wave", C.c_double), ("simds_seen", C.c_int), ("resident_waves_per_simd", C.c_double),
                ("cycles_per_valu_per_wave", C.c_double), ("cycles_per_valu_per_simd", C.c_double)]


class DenoiseParams(C.Structure):
    """mort_denoise_params: DenoiseParams() holds the tuned defaults (mort_hip_denoise_defaults); keyword arguments override them."""
    _fields_ = [("iterations", C.c_int), ("sigma_color", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("normal_log2_power", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mort_hip_denoise_defaults(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TemporalParams(C.Structure):
    """mort_temporal_params: TemporalParams() holds the tuned defaults (mort_hip_temporal_defaults); keyword arguments override them."""
    _fields_ = [("max_samples", C.c_int), ("motion_max_samples", C.c_int), ("depth_tolerance", C.c_float), ("normal_min", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib().mort_hip_temporal_defaults(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SvgfParams(C.Structure):
    """mort_svgf_params: SvgfParams() holds the tuned defaults (mort_hip_svgf_defaults); keyword arguments override them."""
    _fields_ = [("iterations", C.c_int), ("sigma_luminance", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("normal_log2_power", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().mort_hip_svgf_defaults(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ViewParams(C.Structure):
    """mort_view_params: ViewParams(width, height) holds mort_hip_view_defaults (temporal on, SVGF, the three stages' defaults);
    keyword arguments override them -- temporal, filter, tp / dp / sp (the stages' parameter structures)."""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("temporal", C.c_int), ("filter", C.c_int), ("tp", TemporalParams),
                ("dp", DenoiseParams), ("sp", SvgfParams)]

    def __init__(self, width=0, height=0, **kw):
        super().__init__()
        lib().mort_hip_view_defaults(C.byref(self))
        self.width, self.height = width, height
        for k, v in kw.items():
            setattr(self, k, v)


class ViewStats(C.Structure):
    """mort_view_stats"""
    _fields_ = [("render", Stats), ("features_seconds", C.c_double), ("temporal_seconds", C.c_double), ("filter_seconds", C.c_double),
                ("device_seconds", C.c_double), ("frame", C.c_int), ("features_reused", C.c_int), ("history_reset", C.c_int)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["render"] = self.render.asdict()
        return d


class TileState(C.Structure):
    """mort_tile_state: the last render launch's tile order as the host recorded it (Context.tile_state)"""
    _fields_ = [("ordered", C.c_int32), ("probed", C.c_int32), ("tiles", C.c_int32), ("tiles_x", C.c_int32), ("grid", C.c_int32),
                ("block", C.c_int32), ("key_sum", C.c_int32), ("spread_shift", C.c_int32), ("gen_tiles", C.c_int32),
                ("heavy", C.c_int32 * 4), ("has_head", C.c_int32), ("head", C.c_uint32), ("pad_", C.c_uint32),
                ("frame_total", C.c_uint64 * TILE_COUNTERS)]


assert C.sizeof(TileState) == 64 + 8 * TILE_COUNTERS


class MortHipError(RuntimeError):
    def __init__(self, status, what, detail=""):
        self.status = status
        super().__init__(f"{what}: {status} ({lib().mort_hip_strerror(status).decode()}) {detail}".strip())


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `make hip` (or __graft_entry__.build()); "
                               "there is no CPU fallback for the render path")
        L = C.CDLL(LIB_PATH)
        ctx = C.c_void_p
        L.mort_hip_strerror.argtypes = [C.c_int]; L.mort_hip_strerror.restype = C.c_char_p
        L.mort_hip_last_error.argtypes = [ctx]; L.mort_hip_last_error.restype = C.c_char_p
        L.mort_hip_init.argtypes = [C.c_int, C.POINTER(ctx)]; L.mort_hip_init.restype = C.c_int
        L.mort_hip_shutdown.argtypes = [ctx]; L.mort_hip_shutdown.restype = None
        L.mort_hip_upload_world.argtypes = [ctx, C.POINTER(S.World)]; L.mort_hip_upload_world.restype = C.c_int
        L.mort_hip_set_partition.argtypes = [ctx, C.POINTER(Partition)]; L.mort_hip_set_partition.restype = C.c_int
        L.mort_hip_rng_seed.argtypes = [ctx, C.c_uint64, C.c_int, C.c_int]; L.mort_hip_rng_seed.restype = C.c_int
        L.mort_hip_rng_load.argtypes = [ctx, C.c_void_p, C.c_int, C.c_int]; L.mort_hip_rng_load.restype = C.c_int
        L.mort_hip_rng_store.argtypes = [ctx, C.c_void_p, C.c_int, C.c_int]; L.mort_hip_rng_store.restype = C.c_int
        L.mort_hip_render.argtypes = [ctx, C.POINTER(S.Camera), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.POINTER(Stats)]
        L.mort_hip_render.restype = C.c_int
        L.mort_hip_render_device.argtypes = [ctx, C.POINTER(S.Camera), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(Stats)]
        L.mort_hip_render_device.restype = C.c_int
        L.mort_hip_local_rows.argtypes = [ctx, C.c_int]; L.mort_hip_local_rows.restype = C.c_int
        L.mort_hip_global_row.argtypes = [ctx, C.c_int]; L.mort_hip_global_row.restype = C.c_int
        L.mort_hip_rng_seed_host.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]; L.mort_hip_rng_seed_host.restype = C.c_int
        L.mort_hip_render_host.argtypes = [C.POINTER(S.World), C.POINTER(S.Camera), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mort_hip_render_host.restype = C.c_int
        L.mort_hip_calib_valu.argtypes = [ctx, C.c_int, C.c_int, C.POINTER(CalibValu)]; L.mort_hip_calib_valu.restype = C.c_int
        L.mort_hip_calib_hbm_copy.argtypes = [ctx, C.c_size_t, C.c_int, C.POINTER(C.c_double)]; L.mort_hip_calib_hbm_copy.restype = C.c_int
        vp, dp, fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(DenoiseParams)
        L.mort_hip_denoise_defaults.argtypes = [fp]; L.mort_hip_denoise_defaults.restype = C.c_int
        L.mort_hip_render_features.argtypes = [ctx, C.POINTER(S.Camera), vp, vp, vp, dp]; L.mort_hip_render_features.restype = C.c_int
        L.mort_hip_render_features_device.argtypes = [ctx, C.POINTER(S.Camera), vp, vp, vp, vp, dp]
        L.mort_hip_render_features_device.restype = C.c_int
        L.mort_hip_denoise.argtypes = [ctx, fp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_denoise.restype = C.c_int
        L.mort_hip_denoise_device.argtypes = [ctx, fp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_denoise_device.restype = C.c_int
        L.mort_hip_render_features_host.argtypes = [C.POINTER(S.World), C.POINTER(S.Camera), C.c_int, C.c_int, vp, vp, vp, dp]
        L.mort_hip_render_features_host.restype = C.c_int
        L.mort_hip_denoise_host.argtypes = [fp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_denoise_host.restype = C.c_int
        tp, cp = C.POINTER(TemporalParams), C.POINTER(S.Camera)
        L.mort_hip_temporal_defaults.argtypes = [tp]; L.mort_hip_temporal_defaults.restype = C.c_int
        L.mort_hip_temporal.argtypes = [ctx, tp, cp, cp, C.c_int, C.c_int] + [vp] * 8 + [dp]; L.mort_hip_temporal.restype = C.c_int
        L.mort_hip_temporal_device.argtypes = [ctx, tp, cp, cp, C.c_int, C.c_int] + [vp] * 9 + [dp]; L.mort_hip_temporal_device.restype = C.c_int
        L.mort_hip_temporal_host.argtypes = [tp, cp, cp, C.c_int, C.c_int, C.c_int] + [vp] * 8 + [dp]; L.mort_hip_temporal_host.restype = C.c_int
        sp = C.POINTER(SvgfParams)
        L.mort_hip_svgf_defaults.argtypes = [sp]; L.mort_hip_svgf_defaults.restype = C.c_int
        L.mort_hip_svgf.argtypes = [ctx, sp, C.c_int, C.c_int] + [vp] * 8 + [dp]; L.mort_hip_svgf.restype = C.c_int
        L.mort_hip_svgf_device.argtypes = [ctx, sp, C.c_int, C.c_int] + [vp] * 9 + [dp]; L.mort_hip_svgf_device.restype = C.c_int
        L.mort_hip_svgf_host.argtypes = [sp, C.c_int, C.c_int, C.c_int] + [vp] * 8 + [dp]; L.mort_hip_svgf_host.restype = C.c_int
        wp, view = C.POINTER(ViewParams), C.c_void_p
        L.mort_hip_view_defaults.argtypes = [wp]; L.mort_hip_view_defaults.restype = C.c_int
        L.mort_hip_view_check_params.argtypes = [wp]; L.mort_hip_view_check_params.restype = C.c_int
        L.mort_hip_view_create.argtypes = [ctx, wp, C.POINTER(view)]; L.mort_hip_view_create.restype = C.c_int
        L.mort_hip_view_destroy.argtypes = [view]; L.mort_hip_view_destroy.restype = None
        L.mort_hip_view_reset.argtypes = [view]; L.mort_hip_view_reset.restype = C.c_int
        L.mort_hip_view_frame.argtypes = [view, cp, C.c_int, vp, C.POINTER(ViewStats)]; L.mort_hip_view_frame.restype = C.c_int
        L.mort_hip_view_frame_device.argtypes = [view, cp, C.c_int, vp, vp, C.POINTER(ViewStats)]; L.mort_hip_view_frame_device.restype = C.c_int
        L.mort_hip_view_read.argtypes = [view, C.c_int, vp]; L.mort_hip_view_read.restype = C.c_int
        wd, sz = C.POINTER(S.World), C.c_size_t
        L.mort_hip_query_closest.argtypes = [ctx, sz, vp, vp, vp, dp]; L.mort_hip_query_closest.restype = C.c_int
        L.mort_hip_query_closest_device.argtypes = [ctx, sz, vp, vp, vp, vp, dp]; L.mort_hip_query_closest_device.restype = C.c_int
        L.mort_hip_query_closest_host.argtypes = [wd, sz, vp, vp, C.c_int, C.c_int, vp, dp]; L.mort_hip_query_closest_host.restype = C.c_int
        L.mort_hip_query_occluded.argtypes = [ctx, sz, vp, vp, dp]; L.mort_hip_query_occluded.restype = C.c_int
        L.mort_hip_query_occluded_device.argtypes = [ctx, sz, vp, vp, vp, dp]; L.mort_hip_query_occluded_device.restype = C.c_int
        L.mort_hip_query_occluded_host.argtypes = [wd, sz, vp, C.c_int, C.c_int, vp, dp]; L.mort_hip_query_occluded_host.restype = C.c_int
        rp = C.POINTER(RADIANCE_PARAMS)
        L.mort_hip_radiance_params_from_camera.argtypes = [vp, rp]; L.mort_hip_radiance_params_from_camera.restype = C.c_int
        L.mort_hip_query_radiance.argtypes = [ctx, rp, sz, vp, vp, vp, dp]; L.mort_hip_query_radiance.restype = C.c_int
        L.mort_hip_query_radiance_device.argtypes = [ctx, rp, sz, vp, vp, vp, vp, dp]; L.mort_hip_query_radiance_device.restype = C.c_int
        L.mort_hip_query_radiance_host.argtypes = [wd, rp, sz, vp, vp, C.c_int, C.c_int, vp, dp]; L.mort_hip_query_radiance_host.restype = C.c_int
        L.mort_hip_debug_radiance_lds_levels.argtypes = []; L.mort_hip_debug_radiance_lds_levels.restype = C.c_int
        pp = C.POINTER(PROBE_PARAMS)
        L.mort_hip_probe_directions.argtypes = [C.c_int, vp]; L.mort_hip_probe_directions.restype = C.c_int
        L.mort_hip_probe_bake.argtypes = [ctx, pp, sz, vp, vp, vp, vp, dp]; L.mort_hip_probe_bake.restype = C.c_int
        L.mort_hip_probe_bake_device.argtypes = [ctx, pp, sz, vp, vp, vp, vp, vp, dp]; L.mort_hip_probe_bake_device.restype = C.c_int
        L.mort_hip_probe_bake_host.argtypes = [wd, pp, sz, vp, vp, vp, C.c_int, C.c_int, vp, dp]; L.mort_hip_probe_bake_host.restype = C.c_int
        L.mort_hip_sh9_irradiance.argtypes = [vp, vp, vp]; L.mort_hip_sh9_irradiance.restype = C.c_int
        gp = C.POINTER(VOLUME_GRID)
        L.mort_hip_volume_probes.argtypes = [gp, vp]; L.mort_hip_volume_probes.restype = C.c_int
        L.mort_hip_volume_pack.argtypes = [ctx, sz, vp, vp, vp, dp]; L.mort_hip_volume_pack.restype = C.c_int
        L.mort_hip_volume_pack_device.argtypes = [ctx, sz, vp, vp, vp, vp, dp]; L.mort_hip_volume_pack_device.restype = C.c_int
        L.mort_hip_volume_pack_host.argtypes = [sz, vp, vp, C.c_int, vp, dp]; L.mort_hip_volume_pack_host.restype = C.c_int
        L.mort_hip_volume_sample.argtypes = [ctx, gp, vp, sz, vp, sz, vp, dp]; L.mort_hip_volume_sample.restype = C.c_int
        L.mort_hip_volume_sample_device.argtypes = [ctx, gp, vp, sz, vp, sz, vp, vp, dp]; L.mort_hip_volume_sample_device.restype = C.c_int
        L.mort_hip_volume_sample_host.argtypes = [gp, vp, sz, vp, sz, C.c_int, vp, dp]; L.mort_hip_volume_sample_host.restype = C.c_int
        kp, qp = C.POINTER(DEPTH_PARAMS), C.POINTER(VOLUME_VIS_PARAMS)
        L.mort_hip_probe_depth_bake.argtypes = [ctx, kp, sz, vp, vp, dp]; L.mort_hip_probe_depth_bake.restype = C.c_int
        L.mort_hip_probe_depth_bake_device.argtypes = [ctx, kp, sz, vp, vp, vp, dp]; L.mort_hip_probe_depth_bake_device.restype = C.c_int
        L.mort_hip_probe_depth_bake_host.argtypes = [wd, kp, sz, vp, C.c_int, C.c_int, vp, dp]; L.mort_hip_probe_depth_bake_host.restype = C.c_int
        L.mort_hip_volume_sample_visible.argtypes = [ctx, gp, vp, vp, qp, sz, vp, sz, vp, dp]; L.mort_hip_volume_sample_visible.restype = C.c_int
        L.mort_hip_volume_sample_visible_device.argtypes = [ctx, gp, vp, vp, qp, sz, vp, sz, vp, vp, dp]
        L.mort_hip_volume_sample_visible_device.restype = C.c_int
        L.mort_hip_volume_sample_visible_host.argtypes = [gp, vp, vp, qp, sz, vp, sz, C.c_int, vp, dp]
        L.mort_hip_volume_sample_visible_host.restype = C.c_int
        cp = C.POINTER(CACHED_PARAMS)
        L.mort_hip_query_radiance_cached.argtypes = [ctx, cp, sz, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_query_radiance_cached.restype = C.c_int
        L.mort_hip_query_radiance_cached_device.argtypes = [ctx, cp, sz, vp, vp, vp, vp, vp, vp, vp, dp]
        L.mort_hip_query_radiance_cached_device.restype = C.c_int
        L.mort_hip_query_radiance_cached_host.argtypes = [wd, cp, sz, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, dp]
        L.mort_hip_query_radiance_cached_host.restype = C.c_int
        L.mort_hip_query_radiance_cached_direct.argtypes = [ctx, cp, sz, vp, vp, vp, vp, vp, vp, vp, dp]
        L.mort_hip_query_radiance_cached_direct.restype = C.c_int
        L.mort_hip_query_radiance_cached_direct_device.argtypes = [ctx, cp, sz, vp, vp, vp, vp, vp, vp, vp, vp, dp]
        L.mort_hip_query_radiance_cached_direct_device.restype = C.c_int
        L.mort_hip_query_radiance_cached_direct_host.argtypes = [wd, cp, sz, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, dp]
        L.mort_hip_query_radiance_cached_direct_host.restype = C.c_int
        fp = C.POINTER(CACHED_FRAME_PARAMS)
        L.mort_hip_render_cached.argtypes = [ctx, C.POINTER(S.Camera), fp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.mort_hip_render_cached.restype = C.c_int
        L.mort_hip_render_cached_device.argtypes = [ctx, C.POINTER(S.Camera), fp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.mort_hip_render_cached_device.restype = C.c_int
        L.mort_hip_render_cached_host.argtypes = [wd, C.POINTER(S.Camera), vp, C.c_int, C.c_int, fp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.mort_hip_render_cached_host.restype = C.c_int
        L.mort_hip_render_cached_direct.argtypes = [ctx, C.POINTER(S.Camera), fp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.mort_hip_render_cached_direct.restype = C.c_int
        L.mort_hip_render_cached_direct_device.argtypes = [ctx, C.POINTER(S.Camera), fp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
        L.mort_hip_render_cached_direct_device.restype = C.c_int
        L.mort_hip_render_cached_direct_host.argtypes = [wd, C.POINTER(S.Camera), vp, C.c_int, C.c_int, fp, vp, vp, vp, vp, vp, vp, vp,
                                                         C.POINTER(Stats)]
        L.mort_hip_render_cached_direct_host.restype = C.c_int
        L.mort_hip_view_set_cache_direct.argtypes = [view, fp, vp, vp]; L.mort_hip_view_set_cache_direct.restype = C.c_int
        L.mort_hip_view_set_cache_direct_host.argtypes = [view, fp, vp, vp]; L.mort_hip_view_set_cache_direct_host.restype = C.c_int
        L.mort_hip_view_set_cache.argtypes = [view, fp, vp, vp]; L.mort_hip_view_set_cache.restype = C.c_int
        L.mort_hip_view_set_cache_host.argtypes = [view, fp, vp, vp]; L.mort_hip_view_set_cache_host.restype = C.c_int
        xp = C.POINTER(REFRESH_PARAMS)
        L.mort_hip_volume_refresh.argtypes = [ctx, xp, sz, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_volume_refresh.restype = C.c_int
        L.mort_hip_volume_refresh_device.argtypes = [ctx, xp, sz, vp, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_volume_refresh_device.restype = C.c_int
        L.mort_hip_volume_refresh_host.argtypes = [wd, xp, sz, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, dp]
        L.mort_hip_volume_refresh_host.restype = C.c_int
        L.mort_hip_volume_refresh_direct.argtypes = [ctx, xp, sz, vp, vp, vp, vp, vp, vp, vp, dp]; L.mort_hip_volume_refresh_direct.restype = C.c_int
        L.mort_hip_volume_refresh_direct_device.argtypes = [ctx, xp, sz, vp, vp, vp, vp, vp, vp, vp, vp, dp]
        L.mort_hip_volume_refresh_direct_device.restype = C.c_int
        L.mort_hip_volume_refresh_direct_host.argtypes = [wd, xp, sz, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, dp]
        L.mort_hip_volume_refresh_direct_host.restype = C.c_int
        L.mort_hip_probe_directions_round.argtypes = [C.c_int, C.c_uint32, vp]; L.mort_hip_probe_directions_round.restype = C.c_int
        L.mort_hip_view_update_cache.argtypes = [view, vp, vp]; L.mort_hip_view_update_cache.restype = C.c_int
        L.mort_hip_view_update_cache_host.argtypes = [view, vp, vp]; L.mort_hip_view_update_cache_host.restype = C.c_int
        L.mort_hip_debug_tile_state.argtypes = [ctx, C.POINTER(TileState), vp, vp, vp, sz]; L.mort_hip_debug_tile_state.restype = C.c_int
        L.mort_hip_debug_tile_sort.argtypes = [C.c_int, vp, sz, vp, vp]; L.mort_hip_debug_tile_sort.restype = C.c_int
        L.mort_hip_debug_heavy_count.argtypes = [C.c_int, vp, sz, C.c_uint32, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint32)]
        L.mort_hip_debug_heavy_count.restype = C.c_int
        L.mort_hip_debug_deinterleave.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_size_t)]
        L.mort_hip_debug_deinterleave.restype = C.c_int
        _lib = L
    return _lib


class Context:
    """One mort_ctx: one GPU, one partition, one uploaded world."""

    def __init__(self, device=0):
        self._views = []  # the View objects alive on this context
        self._h = C.c_void_p()
        st = lib().mort_hip_init(device, C.byref(self._h))
        if st != 0:
            self._h = None
            raise MortHipError(st, "mort_hip_init")

    def _chk(self, st, what):
        if st != 0:
            raise MortHipError(st, what, lib().mort_hip_last_error(self._h).decode())

    def close(self):
        if self._h:
            for v in self._views:  # mort_hip_shutdown frees them: their handles must not be used again
                v._h = None
            self._views = []
            lib().mort_hip_shutdown(self._h)
            self._h = None

    def view(self, width, height, params=None, **kw):
        """A View of this context (mort_hip_view_create): the whole frame chain kept on the device.  params: a ViewParams, or
        keyword arguments for one (temporal, filter, tp, dp, sp)."""
        return View(self, width, height, params, **kw)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def upload_world(self, world):
        self._chk(lib().mort_hip_upload_world(self._h, world.ptr), "mort_hip_upload_world")

    def set_partition(self, rank, nranks, rows_per_block=8):
        p = Partition(rank, nranks, rows_per_block)
        self._chk(lib().mort_hip_set_partition(self._h, C.byref(p)), "mort_hip_set_partition")

    def rng_seed(self, seed, width, height):
        self._chk(lib().mort_hip_rng_seed(self._h, seed, width, height), "mort_hip_rng_seed")

    def rng_load(self, states, width, height):
        assert states.nbytes == width * height * 48
        self._chk(lib().mort_hip_rng_load(self._h, states.ctypes.data, width, height), "mort_hip_rng_load")

    def rng_store(self, width, height, dtype=None):
        out = np.zeros(width * height * 48, dtype=np.uint8)
        self._chk(lib().mort_hip_rng_store(self._h, out.ctypes.data, width, height), "mort_hip_rng_store")
        return out.view(dtype) if dtype is not None else out

    def local_rows(self, height):
        return lib().mort_hip_local_rows(self._h, height)

    def global_row(self, local_row):
        return lib().mort_hip_global_row(self._h, local_row)

    def render(self, cam, mode=MODE_MEGA, want_accum=True, want_segments=False):
        """Renders the owned rows into full-size host arrays (rows not owned stay zero)."""
        W, H = cam.image_width, cam.image_height
        rgba = np.zeros((H, W, 4), dtype=np.uint8)
        accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
        seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
        st = Stats()
        self._chk(lib().mort_hip_render(self._h, C.byref(cam), mode, rgba.ctypes.data,
                                        accum.ctypes.data if accum is not None else None,
                                        seg.ctypes.data if seg is not None else None, C.byref(st)), "mort_hip_render")
        return dict(rgba=rgba, accum=accum, segments_px=seg, stats=st.asdict())

    def tile_state(self):
        """The tile scheduler's state of this context's last render launch (mort_hip_debug_tile_state), after waiting for its stream:
        the scalars of mort_tile_state, heavy = (mod, num, cap, percent), head and frame_total (the 96 saved counters heavy_count_kernel
        read) or None when heavy waves were off, and -- None unless ordered -- keys and order (what the launch was ordered by) and cost
        (what it left for the next launch), uint32 arrays of `tiles` words."""
        ts = TileState()
        self._chk(lib().mort_hip_debug_tile_state(self._h, C.byref(ts), None, None, None, 0), "mort_hip_debug_tile_state")
        out = {k: int(getattr(ts, k)) for k in ("ordered", "probed", "tiles", "tiles_x", "grid", "block", "key_sum", "spread_shift", "gen_tiles")}
        out["heavy"] = tuple(int(v) for v in ts.heavy)
        out["head"] = int(ts.head) if ts.has_head else None
        out["frame_total"] = np.array(ts.frame_total, dtype=np.uint64) if ts.has_head else None
        out["keys"] = out["order"] = out["cost"] = None
        if ts.ordered and ts.tiles > 0:
            keys, order, cost = (np.full(ts.tiles, 0xdeadbeef, dtype=np.uint32) for _ in range(3))
            self._chk(lib().mort_hip_debug_tile_state(self._h, C.byref(ts), keys.ctypes.data, order.ctypes.data, cost.ctypes.data, ts.tiles),
                      "mort_hip_debug_tile_state")
            out["keys"], out["order"], out["cost"] = keys, order, cost
        return out

    def render_device(self, cam, d_rgba, d_accum=0, stream=0, mode=MODE_MEGA, sync=True):
        """Render into caller-owned device buffers (packed owned rows); d_* are raw device addresses."""
        st = Stats()
        self._chk(lib().mort_hip_render_device(self._h, C.byref(cam), mode, d_rgba, d_accum or None, stream or None,
                                               C.byref(st) if sync else None), "mort_hip_render_device")
        return st.asdict() if sync else None

    def render_features(self, cam):
        """First-hit feature buffers of the owned rows (full-size arrays, other rows stay zero): albedo (H, W, 3), normal (H, W, 3),
        depth (H, W) -- depth 0 = no hit.  Needs an uploaded world, no RNG."""
        W, H = cam.image_width, cam.image_height
        f = _feature_arrays(W, H)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_render_features(self._h, C.byref(cam), f["albedo"].ctypes.data, f["normal"].ctypes.data,
                                                 f["depth"].ctypes.data, C.byref(sec)), "mort_hip_render_features")
        f["seconds"] = sec.value
        return f

    def render_features_device(self, cam, albedo, normal, depth, sync=False):
        """Feature pass into torch tensors on this context's device (packed owned rows: local_rows * W * 3 / * 3 / * 1 float32),
        on the current torch stream.  Asynchronous unless sync (then returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        lr = self.local_rows(cam.image_height)
        _check_tensors(torch, ((albedo, 3), (normal, 3), (depth, 1)), lr * cam.image_width)
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, albedo.device, sync)
        self._chk(lib().mort_hip_render_features_device(self._h, C.byref(cam), albedo.data_ptr(), normal.data_ptr(), depth.data_ptr(),
                                                        stream, C.byref(sec) if sync else None), "mort_hip_render_features_device")
        return sec.value if sync else None

    def denoise(self, accum, albedo, normal, depth, params=None):
        """A-trous denoise of full-image host arrays on the GPU: dict(accum (H, W, 3) f32, rgba (H, W, 4) u8, seconds)."""
        params = params if params is not None else DenoiseParams()
        H, W = np.asarray(depth).shape[:2]
        ins = [np.ascontiguousarray(a, dtype=np.float32) for a in (accum, albedo, normal, depth)]
        out_acc = np.zeros((H, W, 3), dtype=np.float32)
        rgba = np.zeros((H, W, 4), dtype=np.uint8)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_denoise(self._h, C.byref(params), W, H, *[a.ctypes.data for a in ins], out_acc.ctypes.data,
                                         rgba.ctypes.data, C.byref(sec)), "mort_hip_denoise")
        return dict(accum=out_acc, rgba=rgba, seconds=sec.value)

    def denoise_device(self, width, height, accum, albedo, normal, depth, accum_out=None, rgba_out=None, params=None, sync=False):
        """The denoiser on torch tensors of the whole image (float32: W*H*3, *3, *3, *1; rgba_out uint8 W*H*4), on the current torch
        stream.  Outputs may be None.  Asynchronous unless sync (then returns
        the device seconds) or torch runs on its legacy default stream."""
        import torch
        params = params if params is not None else DenoiseParams()
        n = width * height
        _check_tensors(torch, ((accum, 3), (albedo, 3), (normal, 3), (depth, 1)), n)
        if accum_out is not None:
            _check_tensors(torch, ((accum_out, 3),), n)
        if rgba_out is not None:
            assert rgba_out.dtype == torch.uint8 and rgba_out.is_contiguous() and rgba_out.numel() == 4 * n and rgba_out.device == accum.device
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, accum.device, sync)
        self._chk(lib().mort_hip_denoise_device(self._h, C.byref(params), width, height, accum.data_ptr(), albedo.data_ptr(), normal.data_ptr(),
                                                depth.data_ptr(), accum_out.data_ptr() if accum_out is not None else None,
                                                rgba_out.data_ptr() if rgba_out is not None else None,
                                                stream, C.byref(sec) if sync else None), "mort_hip_denoise_device")
        return sec.value if sync else None

    def temporal(self, prev_cam, cam, accum, normal, depth, hist_in, hist_out=None, params=None):
        """One temporal step of full-image host arrays on the GPU (include/mort_hip.h): prev_cam None = reset (then hist_in must be
        None).  hist_out (3, H, W, 4) f32 is filled in (allocated when None).  dict(accum (H, W, 3) f32, rgba (H, W, 4) u8,
        variance (H, W) f32, history, seconds)."""
        params = params if params is not None else TemporalParams()
        ins, outs = _temporal_arrays(cam, accum, normal, depth, hist_in, hist_out)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_temporal(self._h, C.byref(params), C.byref(prev_cam) if prev_cam is not None else None, C.byref(cam),
                                          cam.image_width, cam.image_height, *[_ptr(a) for a in ins], *[_ptr(a) for a in outs],
                                          C.byref(sec)), "mort_hip_temporal")
        return dict(history=outs[0], accum=outs[1], variance=outs[2], rgba=outs[3], seconds=sec.value)

    def temporal_device(self, prev_cam, cam, accum, normal, depth, hist_in, hist_out, accum_out=None, variance_out=None, rgba_out=None,
                        params=None, sync=False):
        """One temporal step on torch tensors of the whole image (float32: W*H*3, *3, *1; history 12*W*H each; variance_out W*H;
        rgba_out uint8 W*H*4), on the current torch stream.  Outputs other than hist_out may be None; hist_in None iff prev_cam None.
        Asynchronous unless sync (then returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        params = params if params is not None else TemporalParams()
        n = cam.image_width * cam.image_height
        pairs = ((accum, 3), (normal, 3), (depth, 1), (hist_in, TEMPORAL_HISTORY_FLOATS), (hist_out, TEMPORAL_HISTORY_FLOATS), (accum_out, 3),
                 (variance_out, 1))
        _check_tensors(torch, [(t, ch) for t, ch in pairs if t is not None], n)
        if rgba_out is not None:
            assert rgba_out.dtype == torch.uint8 and rgba_out.is_contiguous() and rgba_out.numel() == 4 * n and rgba_out.device == accum.device
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, accum.device, sync)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._chk(lib().mort_hip_temporal_device(self._h, C.byref(params), C.byref(prev_cam) if prev_cam is not None else None, C.byref(cam),
                                                 cam.image_width, cam.image_height, ptr(accum), ptr(normal), ptr(depth), ptr(hist_in),
                                                 ptr(hist_out), ptr(accum_out), ptr(variance_out), ptr(rgba_out), stream,
                                                 C.byref(sec) if sync else None), "mort_hip_temporal_device")
        return sec.value if sync else None

    def svgf(self, accum, albedo, normal, depth, variance=None, params=None):
        """The SVGF filter stage on full-image host arrays on the GPU (include/mort_hip.h): variance (H, W) as Context.temporal
        returns it, None = the spatial estimate everywhere.  dict(accum (H, W, 3) f32, variance (H, W) f32, rgba (H, W, 4) u8,
        seconds)."""
        params = params if params is not None else SvgfParams()
        W, H, ins, outs = _svgf_arrays(accum, albedo, normal, depth, variance)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_svgf(self._h, C.byref(params), W, H, *[_ptr(a) for a in ins], *[_ptr(a) for a in outs], C.byref(sec)),
                  "mort_hip_svgf")
        return dict(accum=outs[0], variance=outs[1], rgba=outs[2], seconds=sec.value)

    def svgf_device(self, width, height, accum, albedo, normal, depth, variance=None, accum_out=None, variance_out=None, rgba_out=None,
                    params=None, sync=False):
        """The SVGF filter stage on torch tensors of the whole image (float32: W*H*3, *3, *3, *1; variance and variance_out W*H;
        rgba_out uint8 W*H*4), on the current torch stream.  variance and the outputs may be None.  Asynchronous unless sync (then
        returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        params = params if params is not None else SvgfParams()
        n = width * height
        pairs = ((accum, 3), (albedo, 3), (normal, 3), (depth, 1), (variance, 1), (accum_out, 3), (variance_out, 1))
        _check_tensors(torch, [(t, ch) for t, ch in pairs if t is not None], n)
        if rgba_out is not None:
            assert rgba_out.dtype == torch.uint8 and rgba_out.is_contiguous() and rgba_out.numel() == 4 * n and rgba_out.device == accum.device
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, accum.device, sync)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._chk(lib().mort_hip_svgf_device(self._h, C.byref(params), width, height, ptr(accum), ptr(albedo), ptr(normal), ptr(depth),
                                             ptr(variance), ptr(accum_out), ptr(variance_out), ptr(rgba_out), stream,
                                             C.byref(sec) if sync else None), "mort_hip_svgf_device")
        return sec.value if sync else None

    def query_closest(self, rays, states=None):
        """Closest hit of every ray on the GPU (mort_hip_query_closest): rays RAY_DTYPE (n,) or float32 (n, 8); states None = media
        passed over, else (n,) 48-byte XORWOW streams, advanced IN PLACE.  dict(hits HIT_DTYPE (n,), seconds)."""
        rays, st8 = _query_rays(rays), _query_states(states, rays)
        hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_query_closest(self._h, rays.shape[0], rays.ctypes.data, _ptr(st8), hits.ctypes.data, C.byref(sec)),
                  "mort_hip_query_closest")
        return dict(hits=hits, seconds=sec.value)

    def query_occluded(self, rays):
        """Is a solid hit in [0.001, t_max], per ray, on the GPU (mort_hip_query_occluded): dict(occluded uint8 (n,), seconds)."""
        rays = _query_rays(rays)
        out = np.zeros(rays.shape[0], dtype=np.uint8)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_query_occluded(self._h, rays.shape[0], rays.ctypes.data, out.ctypes.data, C.byref(sec)),
                  "mort_hip_query_occluded")
        return dict(occluded=out, seconds=sec.value)

    def query_closest_device(self, rays, hits, states=None, sync=False):
        """The closest-hit query on torch tensors on this context's device, on the current torch stream: rays float32 of 8 n
        elements, hits of 48 n bytes (any dtype), states None or 48 n bytes, advanced in place.  Asynchronous unless sync (then
        returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        n = _check_query_tensors(torch, rays, ((hits, 48), (states, 48)))
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, rays.device, sync)
        self._chk(lib().mort_hip_query_closest_device(self._h, n, rays.data_ptr(), states.data_ptr() if states is not None else None,
                                                      hits.data_ptr(), stream, C.byref(sec) if sync else None), "mort_hip_query_closest_device")
        return sec.value if sync else None

    def query_occluded_device(self, rays, occluded, sync=False):
        """The occlusion query on torch tensors: rays as for query_closest_device, occluded uint8 of n elements."""
        import torch
        n = _check_query_tensors(torch, rays, ((occluded, 1),))
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, rays.device, sync)
        self._chk(lib().mort_hip_query_occluded_device(self._h, n, rays.data_ptr(), occluded.data_ptr(), stream, C.byref(sec) if sync else None),
                  "mort_hip_query_occluded_device")
        return sec.value if sync else None

    def query_radiance(self, params, rays, states):
        """Path-traced colour along every ray on the GPU (mort_hip_query_radiance): params RADIANCE_PARAMS, rays as for
        query_closest (t_max is ignored), states (n,) 48-byte XORWOW streams, advanced IN PLACE.  dict(rgb float32 (n, 3), seconds):
        the fp32 sum of params.samples paths per ray, unscaled, NaN kept."""
        rays = _query_rays(rays)
        st8 = _query_states(states, rays)
        rgb = np.zeros((rays.shape[0], 3), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_query_radiance(self._h, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), rgb.ctypes.data,
                                                C.byref(sec)), "mort_hip_query_radiance")
        return dict(rgb=rgb, seconds=sec.value)

    def query_radiance_device(self, params, rays, states, rgb, sync=False):
        """The radiance query on torch tensors: rays and states as for query_closest_device (states required), rgb of 12 n bytes."""
        import torch
        n = _check_query_tensors(torch, rays, ((states, 48), (rgb, 12)))
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, rays.device, sync)
        self._chk(lib().mort_hip_query_radiance_device(self._h, C.byref(params), n, rays.data_ptr(), states.data_ptr() if states is not None else None,
                                                       rgb.data_ptr() if rgb is not None else None, stream, C.byref(sec) if sync else None),
                  "mort_hip_query_radiance_device")
        return sec.value if sync else None

    def query_radiance_cached(self, params, rays, states, records, depth=None, want_ends=True):
        """The cached radiance query on the GPU (mort_hip_query_radiance_cached): params CACHED_PARAMS, rays and states as for
        query_radiance (the streams advanced IN PLACE), records float32 (probes, 32) of params.grid, depth float32 (probes, 200) with
        CACHED_VISIBLE and None without.  dict(rgb float32 (n, 3), ends uint32 (n,) or None, seconds): ends counts the paths of a
        ray that ended in the volume."""
        rays, st8, records, depth, rgb, ends = _cached_arrays(params, rays, states, records, depth, want_ends)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_query_radiance_cached(self._h, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), _ptr(records),
                                                       _ptr(depth), rgb.ctypes.data, _ptr(ends), C.byref(sec)), "mort_hip_query_radiance_cached")
        return dict(rgb=rgb, ends=ends, seconds=sec.value)

    def query_radiance_cached_device(self, params, rays, states, records, depth, rgb, ends=None, sync=False):
        """The cached radiance query on torch tensors: rays, states and rgb as for query_radiance_device, records of 128 bytes and
        depth (or None) of 800 bytes per probe of params.grid, ends None or 4 n bytes."""
        import torch
        n = _check_query_tensors(torch, rays, ((states, 48), (rgb, 12), (ends, 4)))
        for t, size in ((records, 128 * params.grid.probes), (depth, 4 * DEPTH_FLOATS * params.grid.probes)):
            if t is not None and (not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != rays.device):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {rays.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, rays.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None
        self._chk(lib().mort_hip_query_radiance_cached_device(self._h, C.byref(params), n, rays.data_ptr(), dptr(states), dptr(records), dptr(depth),
                                                              dptr(rgb), dptr(ends), stream, C.byref(sec) if sync else None),
                  "mort_hip_query_radiance_cached_device")
        return sec.value if sync else None

    def query_radiance_cached_direct(self, params, rays, states, records, depth=None, want_ends=True, want_lit=True):
        """The direct-light cached radiance query on the GPU (mort_hip_query_radiance_cached_direct): query_radiance_cached's
        arguments over records of INDIRECT light (probe_bake_indirect); a path that ends in the volume adds one sampled shadow
        segment toward params.path's light object.  query_radiance_cached's dict plus lit uint32 (n,) or None: the paths of a ray
        whose shadow segment returned a non-zero emission."""
        rays, st8, records, depth, rgb, ends = _cached_arrays(params, rays, states, records, depth, want_ends)
        lit = np.zeros(rays.shape[0], dtype=np.uint32) if want_lit else None
        sec = C.c_double(0)
        self._chk(lib().mort_hip_query_radiance_cached_direct(self._h, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), _ptr(records),
                                                              _ptr(depth), rgb.ctypes.data, _ptr(ends), _ptr(lit), C.byref(sec)),
                  "mort_hip_query_radiance_cached_direct")
        return dict(rgb=rgb, ends=ends, lit=lit, seconds=sec.value)

    def query_radiance_cached_direct_device(self, params, rays, states, records, depth, rgb, ends=None, lit=None, sync=False):
        """The direct-light cached radiance query on torch tensors: query_radiance_cached_device's arguments and lit, None or 4 n
        bytes."""
        import torch
        n = _check_query_tensors(torch, rays, ((states, 48), (rgb, 12), (ends, 4), (lit, 4)))
        for t, size in ((records, 128 * params.grid.probes), (depth, 4 * DEPTH_FLOATS * params.grid.probes)):
            if t is not None and (not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != rays.device):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {rays.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, rays.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None
        self._chk(lib().mort_hip_query_radiance_cached_direct_device(self._h, C.byref(params), n, rays.data_ptr(), dptr(states), dptr(records),
                                                                     dptr(depth), dptr(rgb), dptr(ends), dptr(lit), stream,
                                                                     C.byref(sec) if sync else None),
                  "mort_hip_query_radiance_cached_direct_device")
        return sec.value if sync else None

    def probe_bake_indirect(self, params, probes, states, dirs=None):
        """The three bakes of an indirect-light volume on the GPU (probe_bake_indirect_host has the composition): dict(sh_full,
        sh_emit, sh_ind float32 (n, 9, 3), seconds of both bakes); states are advanced IN PLACE by the full bake."""
        return _bake_indirect(lambda pp, st: self.probe_bake(pp, probes, st, dirs), params, states)

    def render_cached(self, cam, params, records, depth=None, want_accum=True, want_segments=False, want_ends=True):
        """A cached frame on the GPU (mort_hip_render_cached): Context.render in MODE_MEGA whose paths end in the volume.  params
        CACHED_FRAME_PARAMS, records and depth as for query_radiance_cached.  Context.render's dict plus ends_px uint32 (H, W) or
        None: the paths of a pixel that ended in the volume."""
        W, H = cam.image_width, cam.image_height
        records, depth = _cached_volume_arrays(params, records, depth)
        rgba = np.zeros((H, W, 4), dtype=np.uint8)
        accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
        seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
        ends = np.zeros((H, W), dtype=np.uint32) if want_ends else None
        st = Stats()
        self._chk(lib().mort_hip_render_cached(self._h, C.byref(cam), C.byref(params), _ptr(records), _ptr(depth), rgba.ctypes.data, _ptr(accum),
                                               _ptr(seg), _ptr(ends), C.byref(st)), "mort_hip_render_cached")
        return dict(rgba=rgba, accum=accum, segments_px=seg, ends_px=ends, stats=st.asdict())

    def render_cached_device(self, cam, params, records, depth, rgba, accum=None, ends=None, sync=False):
        """The cached frame on torch tensors, on the current torch stream: records of 128 bytes and depth (or None) of 800 bytes per
        probe of params.grid; rgba of at least 4, accum (or None) of at least 12 and ends (or None) of at least 4 bytes per pixel,
        written from their heads.  Asynchronous (returns None) unless sync (then returns the stats)."""
        import torch
        npx = cam.image_width * cam.image_height
        for t, size, exact in ((records, 128 * params.grid.probes, True), (depth, 4 * DEPTH_FLOATS * params.grid.probes, True),
                               (rgba, 4 * npx, False), (accum, 12 * npx, False), (ends, 4 * npx, False)):
            if t is None:
                continue
            have = t.numel() * t.element_size()
            if not t.is_contiguous() or t.device != rgba.device or (have != size if exact else have < size):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {rgba.device}")
        stream, sync = _torch_stream(torch, rgba.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None
        st = Stats()
        self._chk(lib().mort_hip_render_cached_device(self._h, C.byref(cam), C.byref(params), dptr(records), dptr(depth), dptr(rgba), dptr(accum),
                                                      dptr(ends), stream, C.byref(st) if sync else None), "mort_hip_render_cached_device")
        return st.asdict() if sync else None

    def render_cached_direct(self, cam, params, records, depth=None, want_accum=True, want_segments=False, want_ends=True, want_lit=True):
        """A direct-light cached frame on the GPU (mort_hip_render_cached_direct): render_cached over a volume of indirect light
        whose paths add one shadow segment toward cam's light object where they end.  render_cached's dict plus lit_px uint32 (H, W)
        or None: the paths of a pixel whose shadow segment returned a non-zero emission."""
        W, H = cam.image_width, cam.image_height
        records, depth = _cached_volume_arrays(params, records, depth)
        rgba = np.zeros((H, W, 4), dtype=np.uint8)
        accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
        seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
        ends = np.zeros((H, W), dtype=np.uint32) if want_ends else None
        lit = np.zeros((H, W), dtype=np.uint32) if want_lit else None
        st = Stats()
        self._chk(lib().mort_hip_render_cached_direct(self._h, C.byref(cam), C.byref(params), _ptr(records), _ptr(depth), rgba.ctypes.data,
                                                      _ptr(accum), _ptr(seg), _ptr(ends), _ptr(lit), C.byref(st)), "mort_hip_render_cached_direct")
        return dict(rgba=rgba, accum=accum, segments_px=seg, ends_px=ends, lit_px=lit, stats=st.asdict())

    def render_cached_direct_device(self, cam, params, records, depth, rgba, accum=None, ends=None, lit=None, sync=False):
        """The direct-light cached frame on torch tensors, on the current torch stream: render_cached_device's arguments and lit (or
        None) of at least 4 bytes per pixel, written from its head.  Asynchronous (returns None) unless sync (then returns the stats)."""
        import torch
        npx = cam.image_width * cam.image_height
        for t, size, exact in ((records, 128 * params.grid.probes, True), (depth, 4 * DEPTH_FLOATS * params.grid.probes, True),
                               (rgba, 4 * npx, False), (accum, 12 * npx, False), (ends, 4 * npx, False), (lit, 4 * npx, False)):
            if t is None:
                continue
            have = t.numel() * t.element_size()
            if not t.is_contiguous() or t.device != rgba.device or (have != size if exact else have < size):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {rgba.device}")
        stream, sync = _torch_stream(torch, rgba.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None
        st = Stats()
        self._chk(lib().mort_hip_render_cached_direct_device(self._h, C.byref(cam), C.byref(params), dptr(records), dptr(depth), dptr(rgba),
                                                             dptr(accum), dptr(ends), dptr(lit), stream, C.byref(st) if sync else None),
                  "mort_hip_render_cached_direct_device")
        return st.asdict() if sync else None

    def volume_refresh(self, params, states, records_in, depth=None, records_out=None, ends=True, dirs=None, m=None):
        """A volume refresh on the GPU (mort_hip_volume_refresh): params REFRESH_PARAMS; states the P * D 48-byte streams of the whole
        grid, advanced IN PLACE for the selected probes; records_in float32 (P, 32), depth float32 (P, 200) with CACHED_VISIBLE and
        None without; records_out a writeable float32 (P, 32) whose selected records are written in place, or None for a new array
        of zeros; ends a writeable uint32 (P,) written in place, True for a new one, None for no counts; dirs as for probe_bake;
        m the number of selected probes, None = as many as the grid holds.  dict(records, ends, seconds)."""
        m, dirs, records_in, depth, records_out, ends = _refresh_arrays(params, states, records_in, depth, records_out, ends, dirs, m)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_volume_refresh(self._h, C.byref(params), m, _ptr(dirs), _ptr(states), _ptr(records_in), _ptr(depth),
                                                _ptr(records_out), _ptr(ends), C.byref(sec)), "mort_hip_volume_refresh")
        return dict(records=records_out, ends=ends, seconds=sec.value)

    def volume_refresh_device(self, params, states, records_in, depth, records_out, ends=None, dirs=None, m=None, sync=False):
        """The refresh on torch tensors on this context's device, on the current torch stream: states of at least 48 P D bytes,
        records_in of 128 P and depth (or None) of 800 P bytes, records_out of at least 128 P and ends (or None) of at least 4 P
        bytes, written from their heads, dirs None or float32 of 3 D elements.  Asynchronous unless sync (then returns the device
        seconds) or torch runs on its legacy default stream."""
        import torch
        P, D = params.cached.grid.probes, params.directions
        if records_in.device.type != "cuda":
            raise ValueError("expected tensors on the GPU")
        for t, size, exact in ((states, 48 * P * D, False), (records_in, 128 * P, True), (depth, 4 * DEPTH_FLOATS * P, True),
                               (records_out, 128 * P, False), (ends, 4 * P, False), (dirs, 12 * D, True)):
            if t is None:
                continue
            have = t.numel() * t.element_size()
            if not t.is_contiguous() or t.device != records_in.device or (have != size if exact else have < size):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {records_in.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, records_in.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._chk(lib().mort_hip_volume_refresh_device(self._h, C.byref(params), params.selected() if m is None else m, dptr(dirs), dptr(states),
                                                       dptr(records_in), dptr(depth), dptr(records_out), dptr(ends), stream,
                                                       C.byref(sec) if sync else None), "mort_hip_volume_refresh_device")
        return sec.value if sync else None

    def volume_refresh_direct(self, params, states, records_in, depth=None, records_out=None, ends=True, lit=True, dirs=None, m=None):
        """A direct-light volume refresh on the GPU (mort_hip_volume_refresh_direct): Context.volume_refresh over records of
        INDIRECT light, the paths the direct cached query's and a primary hit on an emitter counted as 0; lit as ends: a writeable
        uint32 (P,) written in place, True for a new one, None for no counts.  dict(records, ends, lit, seconds)."""
        m, dirs, records_in, depth, records_out, ends = _refresh_arrays(params, states, records_in, depth, records_out, ends, dirs, m)
        lit = _refresh_counts(params, lit)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_volume_refresh_direct(self._h, C.byref(params), m, _ptr(dirs), _ptr(states), _ptr(records_in), _ptr(depth),
                                                       _ptr(records_out), _ptr(ends), _ptr(lit), C.byref(sec)), "mort_hip_volume_refresh_direct")
        return dict(records=records_out, ends=ends, lit=lit, seconds=sec.value)

    def volume_refresh_direct_device(self, params, states, records_in, depth, records_out, ends=None, lit=None, dirs=None, m=None, sync=False):
        """The direct refresh on torch tensors, as volume_refresh_device: lit (or None) of at least 4 P bytes, written from its head."""
        import torch
        P, D = params.cached.grid.probes, params.directions
        if records_in.device.type != "cuda":
            raise ValueError("expected tensors on the GPU")
        for t, size, exact in ((states, 48 * P * D, False), (records_in, 128 * P, True), (depth, 4 * DEPTH_FLOATS * P, True),
                               (records_out, 128 * P, False), (ends, 4 * P, False), (lit, 4 * P, False), (dirs, 12 * D, True)):
            if t is None:
                continue
            have = t.numel() * t.element_size()
            if not t.is_contiguous() or t.device != records_in.device or (have != size if exact else have < size):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {records_in.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, records_in.device, sync)
        dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._chk(lib().mort_hip_volume_refresh_direct_device(self._h, C.byref(params), params.selected() if m is None else m, dptr(dirs),
                                                              dptr(states), dptr(records_in), dptr(depth), dptr(records_out), dptr(ends),
                                                              dptr(lit), stream, C.byref(sec) if sync else None),
                  "mort_hip_volume_refresh_direct_device")
        return sec.value if sync else None

    def probe_bake(self, params, probes, states, dirs=None):
        """SH9 light probes on the GPU (mort_hip_probe_bake): params PROBE_PARAMS, probes PROBE_DTYPE (n,) or float32 (n, 4) =
        position, time; states n * D 48-byte XORWOW streams, advanced IN PLACE; dirs None = the library's own set, else float32
        (D, 3), used as given.  dict(sh float32 (n, 9, 3), seconds)."""
        probes, dirs = _probe_records(probes), _probe_dirs(dirs, params.directions)
        st8 = _probe_states(states, probes.shape[0], params.directions)
        sh = np.zeros((probes.shape[0], 9, 3), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_probe_bake(self._h, C.byref(params), probes.shape[0], probes.ctypes.data, _ptr(dirs), _ptr(st8),
                                            sh.ctypes.data, C.byref(sec)), "mort_hip_probe_bake")
        return dict(sh=sh, seconds=sec.value)

    def probe_bake_device(self, params, probes, states, sh, dirs=None, sync=False):
        """The bake on torch tensors on this context's device, on the current torch stream: probes float32 of 4 n elements, states
        of 48 n D bytes (advanced in place), sh of 108 n bytes, dirs None or float32 of 3 D elements.  Asynchronous unless sync
        (then returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        if probes.dtype != torch.float32 or not probes.is_contiguous() or probes.numel() % 4 or probes.device.type != "cuda":
            raise ValueError("expected a contiguous float32 tensor of 4 floats per probe on the GPU")
        n, D = probes.numel() // 4, params.directions
        for t, size in ((states, 48 * n * D), (sh, 4 * SH9_FLOATS * n), (dirs, 12 * D)):
            if t is not None and (not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != probes.device):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {probes.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, probes.device, sync)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._chk(lib().mort_hip_probe_bake_device(self._h, C.byref(params), n, probes.data_ptr(), ptr(dirs), ptr(states), ptr(sh), stream,
                                                   C.byref(sec) if sync else None), "mort_hip_probe_bake_device")
        return sec.value if sync else None

    def volume_pack(self, sh, weight=None):
        """Probe records of an irradiance volume on the GPU (mort_hip_volume_pack): sh float32 of 27 floats per probe as the bake
        returns them, weight None = 1.0 or float32 (n,).  dict(records float32 (n, 32), seconds)."""
        sh, weight = _volume_sh(sh, weight)
        n = sh.size // SH9_FLOATS
        rec = np.zeros((n, VOLUME_RECORD_FLOATS), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_volume_pack(self._h, n, sh.ctypes.data, _ptr(weight), rec.ctypes.data, C.byref(sec)), "mort_hip_volume_pack")
        return dict(records=rec, seconds=sec.value)

    def volume_pack_device(self, sh, records, weight=None, sync=False):
        """The packing on torch tensors on this context's device, on the current torch stream: sh float32 of 27 n elements,
        records of 128 n bytes, weight None or float32 of n elements.  Asynchronous unless sync (then returns the device seconds)
        or torch runs on its legacy default stream."""
        import torch
        if sh.dtype != torch.float32 or not sh.is_contiguous() or sh.numel() % SH9_FLOATS or sh.device.type != "cuda":
            raise ValueError("expected a contiguous float32 tensor of 27 floats per probe on the GPU")
        n = sh.numel() // SH9_FLOATS
        for t, size in ((records, 128 * n), (weight, 4 * n)):
            if t is not None and (not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != sh.device):
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {sh.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, sh.device, sync)
        self._chk(lib().mort_hip_volume_pack_device(self._h, n, sh.data_ptr(), weight.data_ptr() if weight is not None else None,
                                                    records.data_ptr(), stream, C.byref(sec) if sync else None), "mort_hip_volume_pack_device")
        return sec.value if sync else None

    def volume_sample(self, grid, records, points, stride=None):
        """Irradiance at every point on the GPU (mort_hip_volume_sample): grid VOLUME_GRID, records float32 (probes, 32) as
        volume_pack returns them, points VOLUME_POINT_DTYPE / HIT_DTYPE (n,) or float32 (n, 6) = position, normal, or with
        `stride` any contiguous array of n records of `stride` bytes that begin with them.  dict(out float32 (n, 4) = E_rgb and
        the weights' sum, seconds)."""
        records, points, n, stride = _volume_inputs(grid, records, points, stride)
        out = np.zeros((n, 4), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_volume_sample(self._h, C.byref(grid), records.ctypes.data, n, points.ctypes.data, stride, out.ctypes.data,
                                               C.byref(sec)), "mort_hip_volume_sample")
        return dict(out=out, seconds=sec.value)

    def volume_sample_device(self, grid, records, points, out, stride=24, sync=False):
        """The sampler on torch tensors on this context's device, on the current torch stream: records of 128 bytes per probe of
        the grid, points a contiguous tensor of n records of `stride` bytes (24 = packed points, 48 = the hits tensor of
        query_closest_device, no copy), out of 16 n bytes.  Asynchronous unless sync (then returns the device seconds) or torch
        runs on its legacy default stream."""
        import torch
        nbytes = points.numel() * points.element_size()
        if not points.is_contiguous() or points.device.type != "cuda" or stride <= 0 or nbytes % stride:
            raise ValueError(f"expected a contiguous tensor of records of {stride} bytes on the GPU")
        n = nbytes // stride
        for t, size in ((records, 128 * grid.probes), (out, 16 * n)):
            if not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != points.device:
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {points.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, points.device, sync)
        self._chk(lib().mort_hip_volume_sample_device(self._h, C.byref(grid), records.data_ptr(), n, points.data_ptr(), stride, out.data_ptr(),
                                                      stream, C.byref(sec) if sync else None), "mort_hip_volume_sample_device")
        return sec.value if sync else None

    def probe_depth_bake(self, params, probes):
        """Depth maps of light probes on the GPU (mort_hip_probe_depth_bake): params DEPTH_PARAMS, probes as for probe_bake.
        dict(depth float32 (n, 200) = 10 x 10 texels of (m1, m2), seconds)."""
        probes = _probe_records(probes)
        depth = np.zeros((probes.shape[0], DEPTH_FLOATS), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_probe_depth_bake(self._h, C.byref(params), probes.shape[0], probes.ctypes.data, depth.ctypes.data, C.byref(sec)),
                  "mort_hip_probe_depth_bake")
        return dict(depth=depth, seconds=sec.value)

    def probe_depth_bake_device(self, params, probes, depth, sync=False):
        """The depth bake on torch tensors on this context's device, on the current torch stream: probes float32 of 4 n elements,
        depth of 800 n bytes.  Asynchronous unless sync (then returns the device seconds) or torch runs on its legacy default
        stream."""
        import torch
        if probes.dtype != torch.float32 or not probes.is_contiguous() or probes.numel() % 4 or probes.device.type != "cuda":
            raise ValueError("expected a contiguous float32 tensor of 4 floats per probe on the GPU")
        n = probes.numel() // 4
        if not depth.is_contiguous() or depth.numel() * depth.element_size() != 4 * DEPTH_FLOATS * n or depth.device != probes.device:
            raise ValueError(f"expected a contiguous tensor of {4 * DEPTH_FLOATS * n} bytes on {probes.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, probes.device, sync)
        self._chk(lib().mort_hip_probe_depth_bake_device(self._h, C.byref(params), n, probes.data_ptr(), depth.data_ptr(),
                                                         stream, C.byref(sec) if sync else None), "mort_hip_probe_depth_bake_device")
        return sec.value if sync else None

    def volume_sample_visible(self, grid, records, depth, params, points, stride=None):
        """The visibility-weighted sampler on the GPU (mort_hip_volume_sample_visible): volume_sample's arguments, depth float32
        (probes, 200) as probe_depth_bake returns it for the grid's probes, params VOLUME_VIS_PARAMS.  dict(out, seconds)."""
        records, points, n, stride = _volume_inputs(grid, records, points, stride)
        depth = _volume_depth(grid, depth)
        out = np.zeros((n, 4), dtype=np.float32)
        sec = C.c_double(0)
        self._chk(lib().mort_hip_volume_sample_visible(self._h, C.byref(grid), records.ctypes.data, depth.ctypes.data, C.byref(params), n,
                                                       points.ctypes.data, stride, out.ctypes.data, C.byref(sec)), "mort_hip_volume_sample_visible")
        return dict(out=out, seconds=sec.value)

    def volume_sample_visible_device(self, grid, records, depth, params, points, out, stride=24, sync=False):
        """The visibility-weighted sampler on torch tensors: volume_sample_device's arguments and depth of 800 bytes per probe of
        the grid.  Asynchronous unless sync (then returns the device seconds) or torch runs on its legacy default stream."""
        import torch
        nbytes = points.numel() * points.element_size()
        if not points.is_contiguous() or points.device.type != "cuda" or stride <= 0 or nbytes % stride:
            raise ValueError(f"expected a contiguous tensor of records of {stride} bytes on the GPU")
        n = nbytes // stride
        for t, size in ((records, 128 * grid.probes), (depth, 4 * DEPTH_FLOATS * grid.probes), (out, 16 * n)):
            if not t.is_contiguous() or t.numel() * t.element_size() != size or t.device != points.device:
                raise ValueError(f"expected a contiguous tensor of {size} bytes on {points.device}")
        sec = C.c_double(0)
        stream, sync = _torch_stream(torch, points.device, sync)
        self._chk(lib().mort_hip_volume_sample_visible_device(self._h, C.byref(grid), records.data_ptr(), depth.data_ptr(), C.byref(params), n,
                                                              points.data_ptr(), stride, out.data_ptr(), stream, C.byref(sec) if sync else None),
                  "mort_hip_volume_sample_visible_device")
        return sec.value if sync else None

    def calib_valu(self, waves_per_simd, kind=0):
        """Shader cycles one SIMD needs per wave64 VALU instruction at `waves_per_simd` resident waves (include/mort_hip.h)."""
        r = CalibValu()
        self._chk(lib().mort_hip_calib_valu(self._h, waves_per_simd, kind, C.byref(r)), "mort_hip_calib_valu")
        return {k: getattr(r, k) for k, _ in r._fields_}

    def calib_hbm_copy(self, nbytes=1 << 30, reps=3):
        """GB/s (read + write) of a float4 copy of `nbytes` per buffer: the HBM rate this box reaches."""
        g = C.c_double(0)
        self._chk(lib().mort_hip_calib_hbm_copy(self._h, nbytes, reps, C.byref(g)), "mort_hip_calib_hbm_copy")
        return g.value


class View:
    """One mort_view (include/mort_hip.h): render -> features -> [temporal] -> [denoise | SVGF] -> uchar4, resident
    on the GPU across frames.  A context manager; closing the Context closes its views."""

    def __init__(self, ctx, width, height, params=None, **kw):
        self.ctx = ctx
        self.params = ViewParams.from_buffer_copy(params) if params is not None else ViewParams(**kw)
        self.params.width, self.params.height = width, height
        self.width, self.height = width, height
        self._h = C.c_void_p()
        st = lib().mort_hip_view_create(ctx._h, C.byref(self.params), C.byref(self._h))
        if st != 0:
            self._h = None
            ctx._chk(st, "mort_hip_view_create")
        ctx._views.append(self)

    def _handle(self):
        if not self._h:
            raise RuntimeError("the view (or its context) has been closed")
        return self._h

    def close(self):
        if self._h:
            lib().mort_hip_view_destroy(self._h)
            self._h = None
            self.ctx._views.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        """Forget the history: the next frame starts over.  RNG states are not touched."""
        self.ctx._chk(lib().mort_hip_view_reset(self._handle()), "mort_hip_view_reset")

    def set_cache(self, params=None, records=None, depth=None, direct=False):
        """The view's frames become cached frames: params CACHED_FRAME_PARAMS; records and depth (or None) either torch tensors on
        the GPU as for Context.render_cached_device, kept alive by the view (mort_hip_view_set_cache), or numpy arrays, which the
        view copies to the device (mort_hip_view_set_cache_host).  direct: direct-light cached frames over a volume of indirect
        light (mort_hip_view_set_cache_direct[_host]), after which read("lit") works.  params None detaches the cache.  Either way
        the history is forgotten, as by reset()."""
        name = "mort_hip_view_set_cache_direct" if direct else "mort_hip_view_set_cache"
        if params is not None and isinstance(records, np.ndarray):
            records, depth = _cached_volume_arrays(params, records, depth)
            self.ctx._chk(getattr(lib(), name + "_host")(self._handle(), C.byref(params), _ptr(records), _ptr(depth)), name + "_host")
            self._cache = None
            return
        dptr = lambda t: t.data_ptr() if t is not None else None
        self.ctx._chk(getattr(lib(), name)(self._handle(), C.byref(params) if params is not None else None, dptr(records), dptr(depth)), name)
        self._cache = (records, depth) if params is not None else None

    def update_cache(self, records, depth=None):
        """New records and maps for the attached cache, under the same params (mort_hip_view_update_cache[_host]): torch tensors on
        the GPU, kept alive by the view, or numpy arrays, which the view copies to the device.  The history is kept."""
        if isinstance(records, np.ndarray):
            records = np.ascontiguousarray(records, dtype=np.float32)
            depth = np.ascontiguousarray(depth, dtype=np.float32) if depth is not None else None
            self.ctx._chk(lib().mort_hip_view_update_cache_host(self._handle(), _ptr(records), _ptr(depth)), "mort_hip_view_update_cache_host")
            self._cache = None
            return
        dptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self.ctx._chk(lib().mort_hip_view_update_cache(self._handle(), dptr(records), dptr(depth)), "mort_hip_view_update_cache")
        self._cache = (records, depth)

    def frame(self, cam, mode=MODE_MEGA):
        """One frame, one host wait: dict(rgba (H, W, 4) u8, stats)."""
        rgba = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        st = ViewStats()
        self.ctx._chk(lib().mort_hip_view_frame(self._handle(), C.byref(cam), mode, rgba.ctypes.data, C.byref(st)), "mort_hip_view_frame")
        return dict(rgba=rgba, stats=st.asdict())

    def frame_device(self, cam, rgba, mode=MODE_MEGA, sync=False):
        """One frame into a torch uint8 tensor of W*H*4 elements on this context's device, on the current torch stream.
        Asynchronous (returns None) unless sync (then returns the stats) or torch runs on its legacy default stream."""
        import torch
        if rgba.dtype != torch.uint8 or not rgba.is_contiguous() or rgba.numel() != 4 * self.width * self.height or rgba.device.type != "cuda":
            raise ValueError(f"expected a contiguous uint8 tensor of {4 * self.width * self.height} elements on the GPU")
        stream, sync = _torch_stream(torch, rgba.device, sync)
        st = ViewStats()
        self.ctx._chk(lib().mort_hip_view_frame_device(self._handle(), C.byref(cam), mode, rgba.data_ptr(), stream, C.byref(st) if sync else None),
                      "mort_hip_view_frame_device")
        return st.asdict() if sync else None

    def read(self, name):
        """One buffer of the last frame as a numpy array (VIEW_BUFFERS): raw_accum / accum / filtered / albedo / normal (H, W, 3),
        variance / depth (H, W), history (3, H, W, 4); "ends" (uint32 (H, W)) with a cache attached, "lit" (the same) with a direct one."""
        code, ch = VIEW_BUFFERS[name]
        shape = (3, self.height, self.width, 4) if name == "history" else (self.height, self.width, ch) if ch > 1 else (self.height, self.width)
        out = np.zeros(shape, dtype=np.float32)
        self.ctx._chk(lib().mort_hip_view_read(self._handle(), code, out.ctypes.data), f"mort_hip_view_read({name})")
        return out.view(np.uint32) if name in ("ends", "lit") else out  # MORT_VIEW_ENDS and MORT_VIEW_LIT hold counts


def seed_states_host(seed, width, height, dtype=None):
    """curand_init(seed, x + y*W, 0) for every pixel, on the host (mort_hip_rng_seed_host): W*H 48-byte records."""
    out = np.zeros(width * height * 48, dtype=np.uint8)
    st = lib().mort_hip_rng_seed_host(seed, width, height, out.ctypes.data)
    if st != 0:
        raise MortHipError(st, "mort_hip_rng_seed_host")
    return out.view(dtype) if dtype is not None else out


def render_host(world, cam, states=None, seed=S.DEFAULT_SEED, nthreads=1, tree=False, want_accum=True, want_segments=True):
    """`mort --mode host`: the kernel body as a host loop (mort_hip_render_host).  No GPU involved.  Returns the same
    dict as Context.render plus the final states (raw uint8 view of the 48-byte records)."""
    W, H = cam.image_width, cam.image_height
    st8 = seed_states_host(seed, W, H) if states is None else np.ascontiguousarray(states).view(np.uint8).reshape(-1).copy()
    assert st8.nbytes == W * H * 48
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
    seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
    stt = Stats()
    rc = lib().mort_hip_render_host(world.ptr, C.byref(cam), st8.ctypes.data, nthreads, HOST_TREE if tree else 0, rgba.ctypes.data,
                                    accum.ctypes.data if accum is not None else None, seg.ctypes.data if seg is not None else None, C.byref(stt))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_render_host")
    return dict(rgba=rgba, accum=accum, segments_px=seg, stats=stt.asdict(), states=st8)


def _cached_volume_arrays(params, records, depth):
    """records and depth maps of a cached call as contiguous float32, their sizes checked against params.grid where that is legal"""
    probes = params.grid.probes if all(0 < c <= VOLUME_MAX_COUNT for c in params.grid.count) else None
    if records is not None:
        records = np.ascontiguousarray(records, dtype=np.float32)
        if probes is not None and records.size != VOLUME_RECORD_FLOATS * probes:
            raise ValueError(f"expected {probes} records of 32 floats")
    if depth is not None:
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if probes is not None and depth.size != DEPTH_FLOATS * probes:
            raise ValueError(f"expected {probes} depth maps of 200 floats")
    return records, depth


def render_cached_host(world, cam, params, records, depth=None, states=None, seed=S.DEFAULT_SEED, nthreads=1, tree=False, want_accum=True,
                       want_segments=True, want_ends=True):
    """The cached frame as a host loop (mort_hip_render_cached_host), no GPU: render_host's arguments and dict (final states
    included) with Context.render_cached's params, records, depth and ends_px."""
    W, H = cam.image_width, cam.image_height
    st8 = seed_states_host(seed, W, H) if states is None else np.ascontiguousarray(states).view(np.uint8).reshape(-1).copy()
    assert st8.nbytes == W * H * 48
    records, depth = _cached_volume_arrays(params, records, depth)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
    seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
    ends = np.zeros((H, W), dtype=np.uint32) if want_ends else None
    stt = Stats()
    rc = lib().mort_hip_render_cached_host(world.ptr, C.byref(cam), st8.ctypes.data, nthreads, HOST_TREE if tree else 0, C.byref(params),
                                           _ptr(records), _ptr(depth), rgba.ctypes.data, _ptr(accum), _ptr(seg), _ptr(ends), C.byref(stt))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_render_cached_host")
    return dict(rgba=rgba, accum=accum, segments_px=seg, ends_px=ends, stats=stt.asdict(), states=st8)


def render_cached_direct_host(world, cam, params, records, depth=None, states=None, seed=S.DEFAULT_SEED, nthreads=1, tree=False, want_accum=True,
                              want_segments=True, want_ends=True, want_lit=True):
    """The direct-light cached frame as a host loop (mort_hip_render_cached_direct_host), no GPU: render_cached_host's arguments and
    dict with Context.render_cached_direct's lit_px."""
    W, H = cam.image_width, cam.image_height
    st8 = seed_states_host(seed, W, H) if states is None else np.ascontiguousarray(states).view(np.uint8).reshape(-1).copy()
    assert st8.nbytes == W * H * 48
    records, depth = _cached_volume_arrays(params, records, depth)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    accum = np.zeros((H, W, 3), dtype=np.float32) if want_accum else None
    seg = np.zeros((H, W), dtype=np.uint32) if want_segments else None
    ends = np.zeros((H, W), dtype=np.uint32) if want_ends else None
    lit = np.zeros((H, W), dtype=np.uint32) if want_lit else None
    stt = Stats()
    rc = lib().mort_hip_render_cached_direct_host(world.ptr, C.byref(cam), st8.ctypes.data, nthreads, HOST_TREE if tree else 0, C.byref(params),
                                                  _ptr(records), _ptr(depth), rgba.ctypes.data, _ptr(accum), _ptr(seg), _ptr(ends), _ptr(lit),
                                                  C.byref(stt))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_render_cached_direct_host")
    return dict(rgba=rgba, accum=accum, segments_px=seg, ends_px=ends, lit_px=lit, stats=stt.asdict(), states=st8)


def debug_own_tree(world):
    """mort_hip_debug_own_tree (host only): dict of the nine facts of this build's own trees over the world (debug.hip)."""
    fn = lib().mort_hip_debug_own_tree
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    out = (C.c_int * 9)()
    st = fn(C.cast(world.ptr, C.c_void_p), out)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_own_tree")
    return dict(zip(("n2", "leaves", "depth2", "n4", "stack4", "reached", "bad", "slots", "same"), list(out)))


def debug_bvh_images(world):
    """mort_hip_debug_bvh_images (host only): what mort_hip_upload_world and the launch of mega_bvh_kernel will decide for the world --
    dict(sphere_bvh, four_wide, fast_bytes, trav_bytes, limit, fits, stack_levels, wide_fits) (debug.hip)."""
    fn = lib().mort_hip_debug_bvh_images
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    out = (C.c_int * 8)()
    st = fn(C.cast(world.ptr, C.c_void_p), out)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_bvh_images")
    return dict(zip(("sphere_bvh", "four_wide", "fast_bytes", "trav_bytes", "limit", "fits", "stack_levels", "wide_fits"), list(out)))


def debug_gen_reach(world):
    """mort_hip_debug_gen_reach (host only): dict(tree, lo (3,), hi (3,), reach) -- whether the world has a unified tree, the box
    of its solids and how far from that box a ray origin may lie for the walk (float32, as the kernels compare them)."""
    fn = lib().mort_hip_debug_gen_reach
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_void_p]
    out = np.zeros(8, dtype=np.float32)
    st = fn(C.cast(world.ptr, C.c_void_p), out.ctypes.data)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_gen_reach")
    return dict(tree=bool(out[0]), lo=out[1:4].copy(), hi=out[4:7].copy(), reach=out[7])


def debug_gen_tree(world):
    """mort_hip_debug_gen_tree (host only): the unified tree of a world and what mort_hip_upload_world decides from it --
    dict(tree, nodes, entries, depth, chains (chain ids, id 0 = no transform included), image_bytes (the LDS image before the
    primitives), prim_bytes, prims_in_lds, lds_bytes (the LDS part of the image), fits (within image_max), image_max,
    prims_lds_max (the limit on image + primitives), capped (nodes whose split the depth cap chose), R, mnear, kmin, reach (float32), centre (3,))."""
    fn = lib().mort_hip_debug_gen_tree
    fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
    iout = (C.c_int * 13)()
    fout = np.zeros(7, dtype=np.float32)
    st = fn(C.cast(world.ptr, C.c_void_p), iout, fout.ctypes.data)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_gen_tree")
    d = dict(zip(("tree", "nodes", "entries", "depth", "chains", "image_bytes", "prim_bytes", "prims_in_lds", "lds_bytes", "fits",
                  "image_max", "prims_lds_max", "capped"), list(iout)))
    for key in ("tree", "prims_in_lds", "fits"):
        d[key] = bool(d[key])
    d.update(R=fout[0], mnear=fout[1], kmin=fout[2], reach=fout[3], centre=fout[4:7].copy())
    return d


DIMAGE_DTYPE = np.dtype([("offset", "<u4"), ("width", "<i4"), ("height", "<i4"), ("pad", "<i4")])  # DImage of dev_scene.h


def debug_math_shapes():
    """mort_hip_debug_math_shape (host only) walked to its end: [(in_words, out_words)] per function number of debug.hip's math table."""
    fn = lib().mort_hip_debug_math_shape
    fn.restype = C.c_int; fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    shapes = []
    a, b = C.c_int(), C.c_int()
    while fn(len(shapes), C.byref(a), C.byref(b)) == 0:
        shapes.append((a.value, b.value))
    return shapes


def _debug_math(name, lead, fnum, records, noise, images, texels, out):
    shapes = debug_math_shapes()
    if not 0 <= fnum < len(shapes):
        raise MortHipError(-1, name, f"no function {fnum}")
    iw, ow = shapes[fnum]
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize not in (4, 8) or rec.size * (rec.dtype.itemsize // 4) % iw:
        raise MortHipError(-1, name, f"function {fnum} takes records of {iw} words")
    words = rec.reshape(-1).view(np.uint32)
    n = words.size // iw
    if out is None:
        out = np.empty(n * ow, dtype=np.uint32)
    if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < n * ow:
        raise MortHipError(-1, name, f"out: {n * ow} contiguous uint32 words")
    noise = np.ascontiguousarray(noise).reshape(-1).view(np.uint8) if noise is not None else None
    images = np.ascontiguousarray(images, dtype=DIMAGE_DTYPE) if images is not None else None
    texels = np.ascontiguousarray(texels, dtype=np.uint8).reshape(-1) if texels is not None else None
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    fn = getattr(lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(lead) + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    st = fn(*lead, fnum, words.ctypes.data, n, out.ctypes.data, ptr(noise), noise.size if noise is not None else 0,
            ptr(images), images.size if images is not None else 0, ptr(texels), texels.size if texels is not None else 0)
    if st != 0:
        raise MortHipError(st, name)
    return out


def debug_math_host(fnum, records, noise=None, images=None, texels=None, out=None):
    """mort_hip_debug_math_host (host only): function `fnum` of debug.hip's math table over records (float32, uint32 or float64 array,
    in_words 32-bit words per record), hipcc's host compile.  noise: the bytes of mort_noise_texture records (noise_value); images
    (DIMAGE_DTYPE) and texels (uint8) for image_value.  Returns the results as raw uint32 words, out_words per record (`out` if given)."""
    return _debug_math("mort_hip_debug_math_host", (), fnum, records, noise, images, texels, out)


def debug_math_device(fnum, records, noise=None, images=None, texels=None, out=None, device=0):
    """mort_hip_debug_math_device: the same on `device`, one launch of math_kernel; arguments and result as debug_math_host."""
    return _debug_math("mort_hip_debug_math_device", (device,), fnum, records, noise, images, texels, out)


LIGHT_SHAPES = ((8, 1), (11, 10))  # mort_hip_debug_light_shape: (in_words, out_words) of light_pdf_value and light_random


def _debug_light(name, handle, fnum, records, out):
    if fnum not in (0, 1):
        raise MortHipError(-1, name, f"no light function {fnum}")
    iw, ow = LIGHT_SHAPES[fnum]
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize != 4 or rec.size % iw:
        raise MortHipError(-1, name, f"light function {fnum} takes records of {iw} 32-bit words")
    words = rec.reshape(-1).view(np.uint32)
    n = words.size // iw
    if out is None:
        out = np.empty(n * ow, dtype=np.uint32)
    if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < n * ow:
        raise MortHipError(-1, name, f"out: {n * ow} contiguous uint32 words")
    fn = getattr(lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    st = fn(handle, fnum, words.ctypes.data, n, out.ctypes.data)
    if st != 0:
        raise MortHipError(st, name)
    return out


def debug_light_host(world, fnum, records, out=None):
    """mort_hip_debug_light_host (host only): light function `fnum` of debug.hip over records of 32-bit words against `world`, hipcc's
    host compile.  fnum 0: light_pdf_value over (type, idx, origin[3], direction[3]) -> the pdf; fnum 1: light_random over (six XORWOW
    words, type, idx, origin[3]) -> direction[3], the six final words, the draw count.  A record that names no acceptable light object
    fails the call.  Returns the results as raw uint32 words (`out` if given)."""
    return _debug_light("mort_hip_debug_light_host", C.cast(world.ptr, C.c_void_p), fnum, records, out)


def debug_light_device(ctx, fnum, records, out=None):
    """mort_hip_debug_light_device: the same on the GPU of `ctx`, over the scene of its uploaded world, one launch of light_kernel;
    arguments and result as debug_light_host."""
    return _debug_light("mort_hip_debug_light_device", ctx._h, fnum, records, out)


SHADE_SHAPE = (16, 22)  # mort_hip_debug_shade_shape: (in_words, out_words) of the shade step (fn 0)


def _debug_shade(name, args, fnum, records, out):
    iw, ow = SHADE_SHAPE
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize != 4 or rec.size % iw:
        raise MortHipError(-1, name, f"the shade step takes records of {iw} 32-bit words")
    words = rec.reshape(-1).view(np.uint32)
    n = words.size // iw
    if out is None:
        out = np.empty(n * ow, dtype=np.uint32)
    if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < n * ow:
        raise MortHipError(-1, name, f"out: {n * ow} contiguous uint32 words")
    fn = getattr(lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_int] * (len(args) - 1) + [C.c_void_p, C.c_size_t, C.c_void_p]
    st = fn(args[0], fnum, *args[1:], words.ctypes.data, n, out.ctypes.data)
    if st != 0:
        raise MortHipError(st, name)
    return out


def debug_shade_host(world, records, tree=False, fnum=0, out=None):
    """mort_hip_debug_shade_host (host only): one iteration of ray_color's loop body -- the closest-hit search of a radiance query's
    segment (tree: over the unified tree where the world has one) and shade_hit -- over records of 16 32-bit words (six XORWOW words, ray
    origin[3], direction[3], time, ray_time0, light_type, light_idx) against `world`, hipcc's host compile.  22 words per record come
    back: status (0 miss, 1 the path ends, 2 scatter, 3 identity scatter), k[3], rp, final_value[3], the ray afterwards (7), the six final
    stream words, the draw count.  A record that names no acceptable light object fails the call.  Returns raw uint32 words (`out` if given)."""
    return _debug_shade("mort_hip_debug_shade_host", (C.cast(world.ptr, C.c_void_p), HOST_TREE if tree else 0), fnum, records, out)


def debug_shade_device(ctx, records, fnum=0, out=None):
    """mort_hip_debug_shade_device: the same on the GPU of `ctx`, over the scene of its uploaded world, one launch of shade_kernel (the
    search is the radiance queries': the unified tree where the world has one); arguments and result as debug_shade_host."""
    return _debug_shade("mort_hip_debug_shade_device", (ctx._h,), fnum, records, out)


CAMERA_SHAPES = ((30, 14), (30, 14), (4, 4))  # mort_hip_debug_camera_shape: (in_words, out_words) of get_ray<RenderArgs>, get_ray<CamView>, the pixel finish


def _debug_camera(name, lead, fnum, records, out):
    if fnum not in (0, 1, 2):
        raise MortHipError(-1, name, f"no camera function {fnum}")
    iw, ow = CAMERA_SHAPES[fnum]
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize != 4 or rec.size % iw:
        raise MortHipError(-1, name, f"camera function {fnum} takes records of {iw} 32-bit words")
    words = rec.reshape(-1).view(np.uint32)
    n = words.size // iw
    if out is None:
        out = np.empty(n * ow, dtype=np.uint32)
    if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < n * ow:
        raise MortHipError(-1, name, f"out: {n * ow} contiguous uint32 words")
    fn = getattr(lib(), name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * len(lead) + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    st = fn(*lead, fnum, words.ctypes.data, n, out.ctypes.data)
    if st != 0:
        raise MortHipError(st, name)
    return out


def debug_camera_host(fnum, records, out=None):
    """mort_hip_debug_camera_host (host only): camera function `fnum` of debug.hip over records of 32-bit words, hipcc's host compile.
    fnum 0 / 1: get_ray<RenderArgs> / get_ray<CamView> over (six XORWOW words, x, y, s_i, s_j, recip_sqrt_spp, defocus_angle, center,
    pixel00, du, dv, defocus_u, defocus_v) -> origin[3], direction[3], time, the six final words, the draw count; fnum 2: pixel_finish and
    pixel_rgba over (scale, sum[3]) -> the accumulator[3] and the uchar4 as one word.  Returns raw uint32 words (`out` if given)."""
    return _debug_camera("mort_hip_debug_camera_host", (), fnum, records, out)


def debug_camera_device(fnum, records, out=None, device=0):
    """mort_hip_debug_camera_device: the same on `device`, one launch of camera_kernel (fnum 1: a record's CamView is written into LDS by the neighbouring lane and read by get_ray after a barrier); arguments and
    result as debug_camera_host."""
    return _debug_camera("mort_hip_debug_camera_device", (device,), fnum, records, out)


def debug_random_float_device(device=0):
    """mort_hip_debug_random_float_device: random_float against (float)(1.0 - (double)u) for all 2^32 generator outputs on `device` --
    dict(differ, lowest, visited)."""
    fn = lib().mort_hip_debug_random_float_device
    fn.restype = C.c_int; fn.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
    out = (C.c_ulonglong * 3)()
    st = fn(device, out)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_random_float_device")
    return dict(differ=out[0], lowest=out[1], visited=out[2])


def debug_tile_sort(cost, device=0):
    """mort_hip_debug_tile_sort: the render's device argsort (tile_sort.hip mort_tile_sort_desc) of n uint32 costs -- (keys, order)."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32).reshape(-1)
    keys, order = np.full(cost.size, 0xdeadbeef, np.uint32), np.full(cost.size, 0xdeadbeef, np.uint32)
    st = lib().mort_hip_debug_tile_sort(device, cost.ctypes.data, cost.size, keys.ctypes.data, order.ctypes.data)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_tile_sort")
    return keys, order


def debug_heavy_count(keys, percent, max_r, counters, lanes, device=0):
    """mort_hip_debug_heavy_count: the heavy-wave head heavy_count_kernel decides from n sorted keys, the threshold `percent`, the cap
    max_r, the 96 saved counters (None: no counters) and the launch's lane count."""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    if counters is not None:
        counters = np.ascontiguousarray(counters, dtype=np.uint64).reshape(-1)
        assert counters.size == TILE_COUNTERS
    head = C.c_uint32(0)
    st = lib().mort_hip_debug_heavy_count(device, keys.ctypes.data, keys.size, percent, max_r,
                                          counters.ctypes.data if counters is not None else None, lanes, C.byref(head))
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_heavy_count")
    return int(head.value)


def debug_gather_stride(width, height, nranks, rows_per_block):
    """pixels between two ranks' tiles in the frame gather's buffer (comm_rccl.hip gather_tile_px); host only"""
    px = C.c_size_t(0)
    st = lib().mort_hip_debug_deinterleave(0, None, width, height, nranks, rows_per_block, None, C.byref(px))
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_deinterleave")
    return int(px.value)


def debug_deinterleave(gathered, width, height, nranks, rows_per_block, device=0):
    """mort_hip_debug_deinterleave: the frame gather's de-interleave kernel over `gathered` (uint8, nranks * stride * 4 bytes with
    stride = debug_gather_stride(...)) -- the (height, width, 4) uint8 frame."""
    gathered = np.ascontiguousarray(gathered, dtype=np.uint8).reshape(-1)
    assert gathered.size == nranks * debug_gather_stride(width, height, nranks, rows_per_block) * 4
    frame = np.zeros((height, width, 4), dtype=np.uint8)
    st = lib().mort_hip_debug_deinterleave(device, gathered.ctypes.data, width, height, nranks, rows_per_block, frame.ctypes.data, None)
    if st != 0:
        raise MortHipError(st, "mort_hip_debug_deinterleave")
    return frame


def _query_rays(rays):
    """rays as a contiguous RAY_DTYPE (n,) array: RAY_DTYPE already, or float32 (n, 8) = origin, direction, time, t_max"""
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
    return np.ascontiguousarray(rays).reshape(-1)


def _query_states(states, rays):
    """the caller's streams as the bytes the library advances in place (no copy), or None"""
    if states is None:
        return None
    if not (isinstance(states, np.ndarray) and states.flags.c_contiguous and states.flags.writeable and states.nbytes == 48 * rays.shape[0]):
        raise ValueError(f"expected a contiguous writeable array of {rays.shape[0]} 48-byte streams")
    return states


def _check_query_tensors(torch, rays, outs):
    if rays.dtype != torch.float32 or not rays.is_contiguous() or rays.numel() % 8 or rays.device.type != "cuda":
        raise ValueError("expected a contiguous float32 tensor of 8 floats per ray on the GPU")
    n = rays.numel() // 8
    for t, size in outs:
        if t is not None and (not t.is_contiguous() or t.numel() * t.element_size() != size * n or t.device != rays.device):
            raise ValueError(f"expected a contiguous tensor of {size * n} bytes on {rays.device}")
    return n


def query_closest_host(world, rays, states=None, tree=False, nthreads=1):
    """The closest-hit query as a host loop (mort_hip_query_closest_host), no GPU: arguments and result as Context.query_closest."""
    rays, st8 = _query_rays(rays), _query_states(states, _query_rays(rays))
    hits = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
    sec = C.c_double(0)
    rc = lib().mort_hip_query_closest_host(world.ptr, rays.shape[0], rays.ctypes.data, _ptr(st8), nthreads, HOST_TREE if tree else 0,
                                           hits.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_query_closest_host")
    return dict(hits=hits, seconds=sec.value)


def query_occluded_host(world, rays, tree=False, nthreads=1):
    """The occlusion query as a host loop (mort_hip_query_occluded_host), no GPU: result as Context.query_occluded."""
    rays = _query_rays(rays)
    out = np.zeros(rays.shape[0], dtype=np.uint8)
    sec = C.c_double(0)
    rc = lib().mort_hip_query_occluded_host(world.ptr, rays.shape[0], rays.ctypes.data, nthreads, HOST_TREE if tree else 0,
                                            out.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_query_occluded_host")
    return dict(occluded=out, seconds=sec.value)


def radiance_params_from_camera(cam, samples=1):
    """RADIANCE_PARAMS with the camera's bounce limit, background and light object (mort_hip_radiance_params_from_camera)."""
    p = RADIANCE_PARAMS()
    rc = lib().mort_hip_radiance_params_from_camera(C.cast(C.byref(cam), C.c_void_p), C.byref(p))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_radiance_params_from_camera")
    p.samples = samples
    return p


def radiance_lds_levels():
    """mort_hip_debug_radiance_lds_levels (host only): the bounce-stack levels the radiance kernels keep in LDS."""
    return lib().mort_hip_debug_radiance_lds_levels()


def query_radiance_host(world, params, rays, states, tree=False, nthreads=1):
    """The radiance query as a host loop (mort_hip_query_radiance_host), no GPU: arguments and result as Context.query_radiance."""
    rays = _query_rays(rays)
    st8 = _query_states(states, rays)
    rgb = np.zeros((rays.shape[0], 3), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_query_radiance_host(world.ptr, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), nthreads,
                                            HOST_TREE if tree else 0, rgb.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_query_radiance_host")
    return dict(rgb=rgb, seconds=sec.value)


def _cached_arrays(params, rays, states, records, depth, want_ends):
    """the arrays of a cached radiance query: inputs as contiguous float32, the outputs new"""
    rays = _query_rays(rays)
    st8 = _query_states(states, rays)
    records, depth = _cached_volume_arrays(params, records, depth)
    rgb = np.zeros((rays.shape[0], 3), dtype=np.float32)
    ends = np.zeros(rays.shape[0], dtype=np.uint32) if want_ends else None
    return rays, st8, records, depth, rgb, ends


def query_radiance_cached_host(world, params, rays, states, records, depth=None, want_ends=True, tree=False, nthreads=1):
    """The cached radiance query as a host loop (mort_hip_query_radiance_cached_host), no GPU: arguments and result as
    Context.query_radiance_cached."""
    rays, st8, records, depth, rgb, ends = _cached_arrays(params, rays, states, records, depth, want_ends)
    sec = C.c_double(0)
    rc = lib().mort_hip_query_radiance_cached_host(world.ptr, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), _ptr(records),
                                                   _ptr(depth), nthreads, HOST_TREE if tree else 0, rgb.ctypes.data, _ptr(ends), C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_query_radiance_cached_host")
    return dict(rgb=rgb, ends=ends, seconds=sec.value)


def query_radiance_cached_direct_host(world, params, rays, states, records, depth=None, want_ends=True, want_lit=True, tree=False, nthreads=1):
    """The direct-light cached radiance query as a host loop (mort_hip_query_radiance_cached_direct_host), no GPU: arguments and
    result as Context.query_radiance_cached_direct."""
    rays, st8, records, depth, rgb, ends = _cached_arrays(params, rays, states, records, depth, want_ends)
    lit = np.zeros(rays.shape[0], dtype=np.uint32) if want_lit else None
    sec = C.c_double(0)
    rc = lib().mort_hip_query_radiance_cached_direct_host(world.ptr, C.byref(params), rays.shape[0], rays.ctypes.data, _ptr(st8), _ptr(records),
                                                          _ptr(depth), nthreads, HOST_TREE if tree else 0, rgb.ctypes.data, _ptr(ends), _ptr(lit),
                                                          C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_query_radiance_cached_direct_host")
    return dict(rgb=rgb, ends=ends, lit=lit, seconds=sec.value)


def _refresh_arrays(params, states, records_in, depth, records_out, ends, dirs, m):
    """the arrays of a volume refresh: inputs as contiguous float32, the outputs the caller's own (written in place) or new"""
    sized = all(0 < c <= VOLUME_MAX_COUNT for c in params.cached.grid.count)
    P = params.cached.grid.probes if sized else 0
    records_in, depth = _cached_volume_arrays(params.cached, records_in, depth)
    dirs = _probe_dirs(dirs, params.directions)
    if states is not None and not (isinstance(states, np.ndarray) and states.flags.c_contiguous and states.flags.writeable):
        raise ValueError("expected a contiguous writeable array of 48-byte streams")
    if sized and states is not None and 0 < params.directions <= 4096 and states.nbytes != 48 * P * params.directions:
        raise ValueError(f"expected {P * params.directions} 48-byte streams")
    if records_out is None:
        records_out = np.zeros((P, VOLUME_RECORD_FLOATS), dtype=np.float32)
    elif not (isinstance(records_out, np.ndarray) and records_out.dtype == np.float32 and records_out.flags.c_contiguous and
              records_out.flags.writeable and (not sized or records_out.size == VOLUME_RECORD_FLOATS * P)):
        raise ValueError(f"expected a contiguous writeable float32 array of {P} records of 32 floats")
    if ends is True:
        ends = np.zeros(P, dtype=np.uint32)
    elif ends is False:
        ends = None
    elif ends is not None and not (isinstance(ends, np.ndarray) and ends.dtype == np.uint32 and ends.flags.c_contiguous and ends.flags.writeable and
                                   (not sized or ends.size == P)):
        raise ValueError(f"expected a contiguous writeable uint32 array of {P} counts")
    return (params.selected() if m is None else m), dirs, records_in, depth, records_out, ends


def volume_refresh_host(world, params, states, records_in, depth=None, records_out=None, ends=True, dirs=None, m=None, tree=False, nthreads=1):
    """The refresh as a host loop (mort_hip_volume_refresh_host), no GPU: arguments and result as Context.volume_refresh."""
    m, dirs, records_in, depth, records_out, ends = _refresh_arrays(params, states, records_in, depth, records_out, ends, dirs, m)
    sec = C.c_double(0)
    rc = lib().mort_hip_volume_refresh_host(world.ptr, C.byref(params), m, _ptr(dirs), _ptr(states), _ptr(records_in), _ptr(depth), nthreads,
                                            HOST_TREE if tree else 0, _ptr(records_out), _ptr(ends), C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_refresh_host")
    return dict(records=records_out, ends=ends, seconds=sec.value)


def _refresh_counts(params, counts):
    """one more count array of a refresh, by _refresh_arrays' rule for ends"""
    sized = all(0 < c <= VOLUME_MAX_COUNT for c in params.cached.grid.count)
    P = params.cached.grid.probes if sized else 0
    if counts is True:
        return np.zeros(P, dtype=np.uint32)
    if counts is False or counts is None:
        return None
    if not (isinstance(counts, np.ndarray) and counts.dtype == np.uint32 and counts.flags.c_contiguous and counts.flags.writeable and
            (not sized or counts.size == P)):
        raise ValueError(f"expected a contiguous writeable uint32 array of {P} counts")
    return counts


def volume_refresh_direct_host(world, params, states, records_in, depth=None, records_out=None, ends=True, lit=True, dirs=None, m=None,
                               tree=False, nthreads=1):
    """The direct refresh as a host loop (mort_hip_volume_refresh_direct_host), no GPU: arguments and result as
    Context.volume_refresh_direct."""
    m, dirs, records_in, depth, records_out, ends = _refresh_arrays(params, states, records_in, depth, records_out, ends, dirs, m)
    lit = _refresh_counts(params, lit)
    sec = C.c_double(0)
    rc = lib().mort_hip_volume_refresh_direct_host(world.ptr, C.byref(params), m, _ptr(dirs), _ptr(states), _ptr(records_in), _ptr(depth),
                                                   nthreads, HOST_TREE if tree else 0, _ptr(records_out), _ptr(ends), _ptr(lit), C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_refresh_direct_host")
    return dict(records=records_out, ends=ends, lit=lit, seconds=sec.value)


def probe_directions_round(D, round):
    """The direction set of refresh round `round` (mort_hip_probe_directions_round, needs no GPU): round 0 is probe_directions(D), a
    later round that set rotated; float32 (D, 3)."""
    out = np.zeros((max(int(D), 0), 3), dtype=np.float32)
    rc = lib().mort_hip_probe_directions_round(D, round, out.ctypes.data)
    if rc != 0:
        raise MortHipError(rc, "mort_hip_probe_directions_round")
    return out


def _probe_records(probes):
    """probes as a contiguous PROBE_DTYPE (n,) array: PROBE_DTYPE already, or float32 (n, 4) = position, time"""
    probes = np.asarray(probes)
    if probes.dtype != PROBE_DTYPE:
        probes = np.ascontiguousarray(probes, dtype=np.float32).reshape(-1, 4).view(PROBE_DTYPE).reshape(-1)
    return np.ascontiguousarray(probes).reshape(-1)


def _probe_dirs(dirs, D):
    if dirs is None:
        return None
    dirs = np.ascontiguousarray(dirs, dtype=np.float32)
    if dirs.size != 3 * D:
        raise ValueError(f"expected {D} directions of 3 floats")
    return dirs


def _probe_states(states, n, D):
    """the caller's streams as the bytes the library advances in place (no copy)"""
    if not (isinstance(states, np.ndarray) and states.flags.c_contiguous and states.flags.writeable and states.nbytes == 48 * n * D):
        raise ValueError(f"expected a contiguous writeable array of {n * D} 48-byte streams")
    return states


def probe_params_from_camera(cam, directions=256, samples=1):
    """PROBE_PARAMS with the camera's bounce limit, background and light object"""
    return PROBE_PARAMS(radiance_params_from_camera(cam, samples), directions)


def probe_directions(D):
    """The library's own direction set (mort_hip_probe_directions, needs no GPU): the D spherical Fibonacci points, float32 (D, 3)."""
    out = np.zeros((max(int(D), 0), 3), dtype=np.float32)
    rc = lib().mort_hip_probe_directions(D, out.ctypes.data)
    if rc != 0:
        raise MortHipError(rc, "mort_hip_probe_directions")
    return out


def probe_bake_host(world, params, probes, states, dirs=None, tree=False, nthreads=1):
    """The bake as a host loop (mort_hip_probe_bake_host), no GPU: arguments and result as Context.probe_bake."""
    probes, dirs = _probe_records(probes), _probe_dirs(dirs, params.directions)
    st8 = _probe_states(states, probes.shape[0], params.directions)
    sh = np.zeros((probes.shape[0], 9, 3), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_probe_bake_host(world.ptr, C.byref(params), probes.shape[0], probes.ctypes.data, _ptr(dirs), _ptr(st8), nthreads,
                                        HOST_TREE if tree else 0, sh.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_probe_bake_host")
    return dict(sh=sh, seconds=sec.value)


def emission_probe_params(params):
    """params (PROBE_PARAMS) as the emission-only bake of an indirect volume takes them: bounce limit 1, a black background, one
    path per direction -- at limit 1 a path returns its first hit's emission or 0"""
    p = PROBE_PARAMS.from_buffer_copy(params)
    p.rp.bounce_limit = 1
    p.rp.samples = 1
    for k in range(3):
        p.rp.background[k] = 0.0
    return p


def _bake_indirect(bake, params, states):
    """bake(params, states) -> probe_bake's dict, run twice: the full bake on the caller's streams, the emission-only bake on a copy
    of the streams the full bake started from; sh_ind = sh_full - sh_emit, one float32 subtraction per float"""
    start = np.array(states, copy=True)
    full = bake(params, states)
    emit = bake(emission_probe_params(params), start)
    with np.errstate(invalid="ignore", over="ignore"):
        ind = (full["sh"] - emit["sh"]).astype(np.float32)
    return dict(sh_full=full["sh"], sh_emit=emit["sh"], sh_ind=ind, seconds=full["seconds"] + emit["seconds"])


def probe_bake_indirect_host(world, params, probes, states, dirs=None, tree=False, nthreads=1):
    """The bakes of an indirect-light volume as host loops, no GPU.  "Indirect" is the radiance arriving at a probe with the
    emission of directly seen emitters taken out; the background and every reflected bounce stay in.  No new kernel: sh_full is
    probe_bake_host under params; sh_emit is probe_bake_host over the same probes and directions, from a copy of the streams sh_full
    started from, under emission_probe_params(params); sh_ind = sh_full - sh_emit.  dict(sh_full, sh_emit, sh_ind float32
    (n, 9, 3), seconds); states are advanced IN PLACE by the full bake."""
    return _bake_indirect(lambda pp, st: probe_bake_host(world, pp, probes, st, dirs, tree=tree, nthreads=nthreads), params, states)


def sh9_irradiance(sh, normal):
    """Irradiance at a surface of unit normal `normal` from one probe's coefficients (9, 3) (mort_hip_sh9_irradiance, host only):
    float32 (3,)."""
    sh = np.ascontiguousarray(sh, dtype=np.float32)
    nrm = np.ascontiguousarray(normal, dtype=np.float32)
    if sh.size != SH9_FLOATS or nrm.size != 3:
        raise ValueError("expected 27 coefficients and a normal of 3 floats")
    out = np.zeros(3, dtype=np.float32)
    rc = lib().mort_hip_sh9_irradiance(sh.ctypes.data, nrm.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise MortHipError(rc, "mort_hip_sh9_irradiance")
    return out


def volume_probes(grid):
    """The probes of a grid in index order (mort_hip_volume_probes, needs no GPU): PROBE_DTYPE (probes,), ready for the bake."""
    sized = all(0 < c <= VOLUME_MAX_COUNT for c in grid.count) and grid.probes <= 0x7fffffff  # else the library refuses the grid
    out = np.zeros(grid.probes if sized else 0, dtype=PROBE_DTYPE)
    rc = lib().mort_hip_volume_probes(C.byref(grid), out.ctypes.data)
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_probes")
    return out


def _volume_sh(sh, weight):
    sh = np.ascontiguousarray(sh, dtype=np.float32)
    if sh.size % SH9_FLOATS:
        raise ValueError("expected 27 coefficients per probe")
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        if weight.size != sh.size // SH9_FLOATS:
            raise ValueError(f"expected {sh.size // SH9_FLOATS} weights")
    return sh, weight


def _volume_inputs(grid, records, points, stride):
    """(records, points, n, stride): the records of the whole grid, the points as contiguous memory of n records of stride bytes"""
    records = np.ascontiguousarray(records, dtype=np.float32)
    if all(0 < c <= VOLUME_MAX_COUNT for c in grid.count) and records.size != VOLUME_RECORD_FLOATS * grid.probes:
        raise ValueError(f"expected {grid.probes} records of 32 floats")
    points = np.asarray(points)
    if stride is None:
        if points.dtype.fields is None:
            points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 6)
            stride = 24
        else:
            stride = points.dtype.itemsize
    points = np.ascontiguousarray(points)
    if stride <= 0 or points.nbytes % stride:
        raise ValueError(f"expected records of {stride} bytes")
    return records, points, points.nbytes // stride, stride


def volume_pack_host(sh, weight=None, nthreads=1):
    """The packing as a host loop (mort_hip_volume_pack_host), no GPU: arguments and result as Context.volume_pack."""
    sh, weight = _volume_sh(sh, weight)
    n = sh.size // SH9_FLOATS
    rec = np.zeros((n, VOLUME_RECORD_FLOATS), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_volume_pack_host(n, sh.ctypes.data, _ptr(weight), nthreads, rec.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_pack_host")
    return dict(records=rec, seconds=sec.value)


def volume_sample_host(grid, records, points, stride=None, nthreads=1):
    """The sampler as a host loop (mort_hip_volume_sample_host), no GPU: arguments and result as Context.volume_sample."""
    records, points, n, stride = _volume_inputs(grid, records, points, stride)
    out = np.zeros((n, 4), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_volume_sample_host(C.byref(grid), records.ctypes.data, n, points.ctypes.data, stride, nthreads, out.ctypes.data,
                                           C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_sample_host")
    return dict(out=out, seconds=sec.value)


def _volume_depth(grid, depth):
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if all(0 < c <= VOLUME_MAX_COUNT for c in grid.count) and depth.size != DEPTH_FLOATS * grid.probes:
        raise ValueError(f"expected {grid.probes} depth maps of 200 floats")
    return depth


def probe_depth_bake_host(world, params, probes, tree=False, nthreads=1):
    """The depth bake as a host loop (mort_hip_probe_depth_bake_host), no GPU: arguments and result as Context.probe_depth_bake."""
    probes = _probe_records(probes)
    depth = np.zeros((probes.shape[0], DEPTH_FLOATS), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_probe_depth_bake_host(world.ptr, C.byref(params), probes.shape[0], probes.ctypes.data, nthreads, HOST_TREE if tree else 0,
                                              depth.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_probe_depth_bake_host")
    return dict(depth=depth, seconds=sec.value)


def volume_sample_visible_host(grid, records, depth, params, points, stride=None, nthreads=1):
    """The visibility-weighted sampler as a host loop (mort_hip_volume_sample_visible_host), no GPU: arguments and result as
    Context.volume_sample_visible."""
    records, points, n, stride = _volume_inputs(grid, records, points, stride)
    depth = _volume_depth(grid, depth)
    out = np.zeros((n, 4), dtype=np.float32)
    sec = C.c_double(0)
    rc = lib().mort_hip_volume_sample_visible_host(C.byref(grid), records.ctypes.data, depth.ctypes.data, C.byref(params), n, points.ctypes.data,
                                                   stride, nthreads, out.ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_volume_sample_visible_host")
    return dict(out=out, seconds=sec.value)


def _feature_arrays(W, H):
    return dict(albedo=np.zeros((H, W, 3), dtype=np.float32), normal=np.zeros((H, W, 3), dtype=np.float32),
                depth=np.zeros((H, W), dtype=np.float32))


def _torch_stream(torch, device, sync):
    """(stream handle for the C ABI, sync).  torch's legacy default stream has handle 0, which the ABI reads as "the context's
    stream" (a non-blocking one): the call then waits for torch's queued work first and is made blocking."""
    s = torch.cuda.current_stream(device).cuda_stream
    if s:
        return s, sync
    torch.cuda.current_stream(device).synchronize()
    return None, True


def _check_tensors(torch, pairs, npx):
    dev = pairs[0][0].device
    for t, ch in pairs:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != ch * npx or t.device != dev or t.device.type != "cuda":
            raise ValueError(f"expected a contiguous float32 tensor of {ch * npx} elements on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def render_features_host(world, cam, nthreads=1, tree=False):
    """The feature pass as a host loop (mort_hip_render_features_host), no GPU: dict(albedo, normal, depth, seconds)."""
    W, H = cam.image_width, cam.image_height
    f = _feature_arrays(W, H)
    sec = C.c_double(0)
    rc = lib().mort_hip_render_features_host(world.ptr, C.byref(cam), nthreads, HOST_TREE if tree else 0, f["albedo"].ctypes.data,
                                             f["normal"].ctypes.data, f["depth"].ctypes.data, C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_render_features_host")
    f["seconds"] = sec.value
    return f


def denoise_host(accum, albedo, normal, depth, params=None, nthreads=1):
    """The a-trous denoiser as a host loop (mort_hip_denoise_host), no GPU: dict(accum (H, W, 3) f32, rgba (H, W, 4) u8, seconds)."""
    params = params if params is not None else DenoiseParams()
    H, W = np.asarray(depth).shape[:2]
    ins = [np.ascontiguousarray(a, dtype=np.float32) for a in (accum, albedo, normal, depth)]
    for a, ch in zip(ins, (3, 3, 3, 1)):
        assert a.size == W * H * ch
    out_acc = np.zeros((H, W, 3), dtype=np.float32)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    sec = C.c_double(0)
    rc = lib().mort_hip_denoise_host(C.byref(params), W, H, nthreads, *[a.ctypes.data for a in ins], out_acc.ctypes.data, rgba.ctypes.data,
                                     C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_denoise_host")
    return dict(accum=out_acc, rgba=rgba, seconds=sec.value)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def history_array(width, height):
    """An empty temporal history: three float4 planes, (3, H, W, 4) float32."""
    return np.zeros((3, height, width, 4), dtype=np.float32)


def _temporal_arrays(cam, accum, normal, depth, hist_in, hist_out):
    W, H = cam.image_width, cam.image_height
    ins = [np.ascontiguousarray(a, dtype=np.float32) for a in (accum, normal, depth)]
    for a, ch in zip(ins, (3, 3, 1)):
        if a.size != W * H * ch:
            raise ValueError(f"expected {W * H * ch} floats, got {a.size}")
    if hist_in is not None:
        hist_in = np.ascontiguousarray(hist_in, dtype=np.float32)
        if hist_in.size != W * H * TEMPORAL_HISTORY_FLOATS:
            raise ValueError("history of the wrong size")
    if hist_out is None:
        hist_out = history_array(W, H)
    assert hist_out.dtype == np.float32 and hist_out.flags.c_contiguous and hist_out.size == W * H * TEMPORAL_HISTORY_FLOATS
    outs = [hist_out, np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W), dtype=np.float32), np.zeros((H, W, 4), dtype=np.uint8)]
    return ins + [hist_in], outs


def temporal_host(prev_cam, cam, accum, normal, depth, hist_in, hist_out=None, params=None, nthreads=1):
    """One temporal step as a host loop (mort_hip_temporal_host), no GPU: dict(accum, rgba, variance, history, seconds) as
    Context.temporal."""
    params = params if params is not None else TemporalParams()
    ins, outs = _temporal_arrays(cam, accum, normal, depth, hist_in, hist_out)
    sec = C.c_double(0)
    rc = lib().mort_hip_temporal_host(C.byref(params), C.byref(prev_cam) if prev_cam is not None else None, C.byref(cam), cam.image_width,
                                      cam.image_height, nthreads, *[_ptr(a) for a in ins], *[_ptr(a) for a in outs], C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_temporal_host")
    return dict(history=outs[0], accum=outs[1], variance=outs[2], rgba=outs[3], seconds=sec.value)


def _svgf_arrays(accum, albedo, normal, depth, variance):
    H, W = np.asarray(depth).shape[:2]
    ins = [np.ascontiguousarray(a, dtype=np.float32) for a in (accum, albedo, normal, depth)]
    ins.append(np.ascontiguousarray(variance, dtype=np.float32) if variance is not None else None)
    for a, ch in zip(ins, (3, 3, 3, 1, 1)):
        if a is not None and a.size != W * H * ch:
            raise ValueError(f"expected {W * H * ch} floats, got {a.size}")
    outs = [np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W), dtype=np.float32), np.zeros((H, W, 4), dtype=np.uint8)]
    return W, H, ins, outs


def svgf_host(accum, albedo, normal, depth, variance=None, params=None, nthreads=1):
    """The SVGF filter stage as a host loop (mort_hip_svgf_host), no GPU: dict(accum, variance, rgba, seconds) as Context.svgf."""
    params = params if params is not None else SvgfParams()
    W, H, ins, outs = _svgf_arrays(accum, albedo, normal, depth, variance)
    sec = C.c_double(0)
    rc = lib().mort_hip_svgf_host(C.byref(params), W, H, nthreads, *[_ptr(a) for a in ins], *[_ptr(a) for a in outs], C.byref(sec))
    if rc != 0:
        raise MortHipError(rc, "mort_hip_svgf_host")
    return dict(accum=outs[0], variance=outs[1], rgba=outs[2], seconds=sec.value)


class TemporalHistory:
    """Frame-to-frame state of temporal accumulation: the two ping-ponged history buffers and the previous camera.

    backend: None = the host loop (numpy arrays), a Context = its GPU (numpy arrays through mort_hip_temporal), or
    ("device", ctx) = torch tensors on ctx's device (mort_hip_temporal_device on the current torch stream).  step() takes one
    frame's accumulators and features and returns dict(accum, rgba, variance, samples) -- samples = the effective sample count
    per pixel (H, W) -- as arrays / tensors of the backend; the returned buffers are reused by the next step."""

    def __init__(self, width, height, params=None, backend=None, nthreads=1):
        self.width, self.height = width, height
        self.params = params if params is not None else TemporalParams()
        self.backend, self.nthreads = backend, nthreads
        self.device = isinstance(backend, tuple) and backend[0] == "device"
        n = width * height
        if self.device:
            import torch
            dev = torch.device("cuda", torch.cuda.current_device())
            z = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
            self._hist = [z(TEMPORAL_HISTORY_FLOATS * n), z(TEMPORAL_HISTORY_FLOATS * n)]
            self._out = dict(accum=z(3 * n), variance=z(n), rgba=z(4 * n, torch.uint8))
        else:
            self._hist = [history_array(width, height), history_array(width, height)]
        self.prev_cam = None
        self.frames = 0

    def reset(self):
        """Forget the history: the next step starts over."""
        self.prev_cam = None
        self.frames = 0

    @property
    def history(self):
        """The history the last step wrote (three float4 planes)."""
        return self._hist[0]

    def step(self, accum, normal, depth, cam, sync=False):
        """One frame; "seconds" in the result is the kernel's device time (host loop: wall time; device backend: None unless sync)."""
        assert cam.image_width == self.width and cam.image_height == self.height
        prev = self.prev_cam
        hin, hout = (self._hist[0] if prev is not None else None), self._hist[1]
        if self.device:
            o = self._out
            sec = self.backend[1].temporal_device(prev, cam, accum, normal, depth, hin, hout, accum_out=o["accum"], variance_out=o["variance"],
                                                  rgba_out=o["rgba"], params=self.params, sync=sync)
            r = dict(o, seconds=sec)
            samples = hout.view(3, self.height, self.width, 4)[0, ..., 3]
        else:
            if self.backend is None:
                r = temporal_host(prev, cam, accum, normal, depth, hin, hout, params=self.params, nthreads=self.nthreads)
            else:
                r = self.backend.temporal(prev, cam, accum, normal, depth, hin, hout, params=self.params)
            samples = hout[0, ..., 3]
        self._hist.reverse()
        self.prev_cam = S.Camera.from_buffer_copy(cam)
        self.frames += 1
        return dict(accum=r["accum"], rgba=r["rgba"], variance=r["variance"], samples=samples, seconds=r["seconds"])
