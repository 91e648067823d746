/*
 * mort_internal.h -- functions shared between the translation units of libmort_hip.so (not part of the C ABI).
 */
#ifndef MORT_INTERNAL_H
#define MORT_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <cstdio>
#include <cstdlib>

#include "mort_hip.h"

/* ---- tuning variables (MORT_*): read with getenv where they apply, on every call, so a process may change them between renders.
 * These parse the text getenv gave (null: the variable is not set): each leaves v as it is unless the text is there and accepted,
 * and says whether it wrote v ---- */
/* a switch: on iff the text begins with '1' */
static inline bool knob_flag(const char *e, bool &v) { if (e) v = e[0] == '1'; return e != nullptr; }
/* any integer, as atoi reads it (text that is no number: 0) */
static inline bool knob_int(const char *e, int &v) { if (e) v = std::atoi(e); return e != nullptr; }
/* an integer in [lo, hi] */
static inline bool knob_int_in(const char *e, int lo, int hi, int &v) { int x = 0; if (!knob_int(e, x) || x < lo || x > hi) return false; v = x; return true; }
/* "a,b,..": n <= 4 integers, each at least min (text after the n-th is not looked at) */
static inline bool knob_ints(const char *e, int n, int min, int *v) {
    int x[4] = {0, 0, 0, 0};
    if (!e || std::sscanf(e, "%d,%d,%d,%d", &x[0], &x[1], &x[2], &x[3]) < n) return false;
    for (int k = 0; k < n; k++) if (x[k] < min) return false;
    for (int k = 0; k < n; k++) v[k] = x[k];
    return true;
}

/* context.hip: MORT_MODE_THROUGHPUT's (pixel, stratum row) streams for this image, partition and sqrt_spp, seeded on `s` when they are not yet */
int mort_ensure_substates(mort_ctx *c, int W, int H, int S, hipStream_t s);

/* tile_sort.hip */
size_t mort_tile_sort_temp_bytes(int n);
hipError_t mort_tile_sort_desc(const unsigned *d_cost, unsigned *d_keys_out, unsigned *d_iota, unsigned *d_order, void *d_temp,
                               size_t temp_bytes, int n, hipStream_t s);
hipError_t mort_tile_heavy_count(const unsigned *d_keys_desc, int n, unsigned percent, unsigned max_r, const unsigned long long *d_frame_total,
                                 unsigned long long lanes, unsigned *d_out, hipStream_t s);

/* denoise.hip, temporal.hip, svgf.hip: the parameter checks of the stage calls, for mort_hip_view_check_params */
bool mort_denoise_params_ok(const mort_denoise_params *p);
bool mort_temporal_params_ok(const mort_temporal_params *p);
bool mort_svgf_params_ok(const mort_svgf_params *p);

/* radiance.hip, volume.hip: the checks and the launch parameters of the radiance and volume calls, for the cached radiance queries
 * (cached.hip) */
struct RadianceArgs;
int mort_radiance_check(const mort_radiance_params *p, size_t n, const void *rays, void *states, void *rgb);
void mort_radiance_args_params(RadianceArgs &a, const mort_radiance_params *p);
bool mort_volume_grid_ok(const mort_volume_grid *g);
bool mort_volume_vis_params_ok(const mort_volume_vis_params *p);

/* cached.hip: the checks of the cached queries' own fields (cache_depth, flags, grid, vis, records, depth with and without the flag)
 * and their volume as the kernels take it by value, for the cached frames (cached_frame.hip) */
struct VolumeArgs;
struct VolumeVisArgs;
bool mort_cached_volume_ok(int32_t cache_depth, uint32_t flags, const mort_volume_grid *grid, const mort_volume_vis_params *vis, const void *records,
                           const void *depth);
void mort_cached_volume(VolumeArgs &v, const mort_volume_grid &grid, const void *records);
void mort_cached_volume(VolumeVisArgs &v, const mort_volume_grid &grid, const mort_volume_vis_params &vis, const void *records, const void *depth);

/* probe.hip: the context's device copy of the library's own set of D directions, for the volume refresh (refresh.hip) */
int mort_probe_own_directions(mort_ctx *c, int D, hipStream_t s, const float **d_dirs);

/* view.hip: mort_hip_shutdown frees the views still alive on the context */
void mort_views_free(mort_ctx *c);

#endif
