/*
 * cached.hip -- cached radiance queries: radiance queries whose paths end in an irradiance volume.  A path runs
 * its first cache_depth bounces as the path tracer runs them; at the first Lambertian hit after that it returns
 * albedo * E(p, n) / pi from the probe grid (with MORT_CACHED_VISIBLE 4.18) instead of tracing on.
 *
 * Kernel (gfx950, wave64, 256-thread groups, one lane per ray, 1-D grid):
 *   query_radiance_cached_kernel<TREE, VISIBLE>   query_radiance_kernel<TREE> (radiance.hip) with the shortcut in its bounce loop:
 *                                 the same loads and stores, the same LDS (the walk column and MORT_RADIANCE_LDS_LEVELS bounce-stack
 *                                 levels), one more 4-byte store per ray where the caller wants the counts.  The grid descriptor and
 *                                 1 / spacing are kernel arguments (scalar registers).  VISIBLE is a template parameter: the plain
 *                                 form carries neither the depth maps' pointer nor the tap code.
 *
 * The host form (mort_hip_query_radiance_cached_host) runs the same per-ray body (dev_cached.h) on host threads and makes no HIP
 * runtime call.  Nothing here reads or writes the render's pixel states, tile-cost cache or counters, or looks at the partition.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "mort_hip.h"
#include "dev_cached.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* 3 waves per SIMD, as query_radiance_kernel: the resource check of the build holds these kernels to the same rule */
template <bool TREE, bool VISIBLE>
__global__ void __launch_bounds__(QUERY_BLOCK, 3) query_radiance_cached_kernel(const CachedArgs<VISIBLE> c) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * QUERY_BLOCK];
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= c.r.q.n) return;
    cached_ray<TREE, VISIBLE>(c, i, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK, bounce_stack + threadIdx.x, MORT_RADIANCE_LDS_LEVELS, QUERY_BLOCK);
}

/* ====================================================================== host */

/* ---- what the cached frames (cached_frame.hip) share with the queries: the checks of the new fields and the volume by value ---- */

bool mort_cached_volume_ok(int32_t cache_depth, uint32_t flags, const mort_volume_grid *grid, const mort_volume_vis_params *vis, const void *records,
                           const void *depth) {
    if (!records || cache_depth < 0 || cache_depth > MORT_MAX_BOUNCE_LIMIT || (flags & ~MORT_CACHED_VISIBLE)) return false;
    const bool visible = (flags & MORT_CACHED_VISIBLE) != 0;
    if (visible != (depth != nullptr)) return false;
    return mort_volume_grid_ok(grid) && (!visible || mort_volume_vis_params_ok(vis));
}

void mort_cached_volume(VolumeArgs &v, const mort_volume_grid &grid, const void *records) {
    std::memset(&v, 0, sizeof v);
    v.g = grid;
    for (int k = 0; k < 3; k++) v.inv[k] = 1.0f / grid.spacing[k];
    v.records = (const float *)records;
}
void mort_cached_volume(VolumeVisArgs &v, const mort_volume_grid &grid, const mort_volume_vis_params &vis, const void *records, const void *depth) {
    mort_cached_volume(v.v, grid, records);
    v.depth = (const float *)depth; v.normal_bias = vis.normal_bias; v.min_visibility = vis.min_visibility;
}

namespace {

constexpr size_t kRecordBytes = MORT_VOLUME_RECORD_FLOATS * sizeof(float);
constexpr size_t kDepthBytes = MORT_DEPTH_FLOATS * sizeof(float);

size_t cached_probes(const mort_cached_params *p) { return (size_t)p->grid.count[0] * (size_t)p->grid.count[1] * (size_t)p->grid.count[2]; }

/* what the three forms check before they look at a world: the radiance calls' checks, the volume calls', and the new fields */
int cached_check(const mort_cached_params *p, size_t n, const void *rays, void *states, const void *records, const void *depth, void *rgb, void *ends) {
    if (!p || !records) return MORT_ERR_INVALID;
    const int st = mort_radiance_check(&p->path, n, rays, states, rgb);
    if (st != MORT_OK) return st;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, records, depth)) return MORT_ERR_INVALID;
    const size_t probes = cached_probes(p);
    const void *ins[3] = {rays, records, depth};
    const size_t in_bytes[3] = {n * sizeof(mort_ray), probes * kRecordBytes, probes * kDepthBytes};
    void *outs[3] = {states, rgb, ends};
    const size_t out_bytes[3] = {n * sizeof(mort_rng_state), n * 3 * sizeof(float), n * sizeof(uint32_t)};
    return buffers_disjoint(ins, in_bytes, 3, outs, out_bytes, 3) ? MORT_OK : MORT_ERR_INVALID;
}


/* everything of the arguments but the scene (c.r.q: query_args_device / query_args_host come first, they clear it) */
template <bool VISIBLE>
void cached_args(CachedArgs<VISIBLE> &c, const mort_cached_params *p, size_t n, const void *rays, void *states, const void *records, const void *depth,
                 void *rgb, void *ends) {
    mort_radiance_args_params(c.r, &p->path);
    c.r.q.n = n; c.r.q.rays = (const mort_ray *)rays; c.r.q.states = (mort_rng_state *)states; c.r.rgb = (float *)rgb;
    c.cache_depth = p->cache_depth; c.ends = (uint32_t *)ends;
    if constexpr (VISIBLE) mort_cached_volume(c.vol.v, p->grid, p->vis, records, depth);
    else mort_cached_volume(c.vol.v, p->grid, records);
}

template <bool VISIBLE>
void cached_launch(const mort_ctx *ctx, CachedArgs<VISIBLE> &c, hipStream_t s) {
    const dim3 grid((unsigned)((c.r.q.n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    if (ctx->gen_ok) hipLaunchKernelGGL((query_radiance_cached_kernel<true, VISIBLE>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((query_radiance_cached_kernel<false, VISIBLE>), grid, block, 0, s, c);
}

template <bool VISIBLE> struct CachedHostJob { CachedArgs<VISIBLE> c; bool tree; };
template <bool VISIBLE>
void cached_host_chunk(void *p, int chunk) {
    const CachedHostJob<VISIBLE> *j = (const CachedHostJob<VISIBLE> *)p;
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const size_t n = j->c.r.q.n, i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < n ? i0 + kHostChunk : n;
    for (size_t i = i0; i < i1; i++) {
        if (j->tree) cached_ray<true, VISIBLE>(j->c, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
        else cached_ray<false, VISIBLE>(j->c, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
    }
}

template <bool VISIBLE>
void cached_host_run(const SceneBlob &sb, bool tree, const mort_cached_params *p, size_t n, const mort_ray *rays, mort_rng_state *states,
                     const float *records, const float *depth, int nthreads, float *rgb, uint32_t *ends) {
    CachedHostJob<VISIBLE> job;
    job.tree = tree;
    query_args_host(sb, tree, job.c.r.q);
    cached_args(job.c, p, n, rays, states, records, depth, rgb, ends);
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, cached_host_chunk<VISIBLE>, &job);
}

} // namespace

extern "C" int mort_hip_query_radiance_cached_device(mort_ctx *c, const mort_cached_params *p, size_t n, const void *d_rays, void *d_states,
                                                     const void *d_records, const void *d_depth, void *d_rgb_out, void *d_ends_out, void *stream,
                                                     double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = cached_check(p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_rays) || !aligned16(d_states) || !aligned16(d_records) || !aligned16(d_depth) || !aligned16(d_rgb_out) || !aligned16(d_ends_out))
        return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    if (p->flags & MORT_CACHED_VISIBLE) {
        CachedArgs<true> a;
        query_args_device(c, a.r.q);
        cached_args(a, p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out);
        cached_launch(c, a, s);
    } else {
        CachedArgs<false> a;
        query_args_device(c, a.r.q);
        cached_args(a, p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out);
        cached_launch(c, a, s);
    }
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: rays, streams, records and maps up, the _device call on the context's stream, colours, streams and counts down */
extern "C" int mort_hip_query_radiance_cached(mort_ctx *c, const mort_cached_params *p, size_t n, const mort_ray *rays, mort_rng_state *states,
                                              const float *records, const float *depth, float *rgb_out, uint32_t *ends_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = cached_check(p, n, rays, states, records, depth, rgb_out, ends_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t probes = cached_probes(p);
    StagePlane pl[6] = {{rays, nullptr, n * sizeof(mort_ray)}, {states, states, n * sizeof(mort_rng_state)}, {records, nullptr, probes * kRecordBytes},
                        {depth, nullptr, probes * kDepthBytes}, {nullptr, rgb_out, n * 3 * sizeof(float)}, {nullptr, ends_out, n * sizeof(uint32_t)}};
    if ((st = stage_upload(c, pl, 6)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_query_radiance_cached_device(c, p, n, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, c->stream, &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 6);
}

extern "C" int mort_hip_query_radiance_cached_host(const mort_world *world, const mort_cached_params *p, size_t n, const mort_ray *rays,
                                                   mort_rng_state *states, const float *records, const float *depth, int nthreads, int flags,
                                                   float *rgb_out, uint32_t *ends_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = cached_check(p, n, rays, states, records, depth, rgb_out, ends_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    const bool tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    const double t0 = now_s();
    if (p->flags & MORT_CACHED_VISIBLE) cached_host_run<true>(sb, tree, p, n, rays, states, records, depth, nthreads, rgb_out, ends_out);
    else cached_host_run<false>(sb, tree, p, n, rays, states, records, depth, nthreads, rgb_out, ends_out);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
