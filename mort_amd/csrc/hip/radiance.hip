/*
 * radiance.hip -- radiance queries: the path-traced colour arriving along batches of the caller's rays, by the
 * render's own bounce loop, shading and traversal.
 *
 * Kernel (gfx950, wave64, 256-thread groups, one lane per ray, 1-D grid):
 *   query_radiance_kernel<TREE>   `samples` times ray_color(ray, bounce_limit) from the lane's stream, summed in fp32: a ray as
 *                                 two 16-byte loads, the stream loaded once and stored once, the sum as one 12-byte store.
 *                                 TREE: every segment is searched as a closest-hit query searches (reach test per origin, the
 *                                 unified-tree walk with its pending children in LDS, 16 x 256 x 2 B, the scan for the rest),
 *                                 else world::hit's item loop as mega_kernel runs it (the threaded reference walk for BVH worlds:
 *                                 the known slow path).  The first MORT_RADIANCE_LDS_LEVELS bounce-stack levels are in LDS as
 *                                 [level][thread] float4, the deeper ones in private memory.
 *
 * The host form (mort_hip_query_radiance_host) runs the same per-ray body (dev_radiance.h) on host threads and makes no HIP
 * runtime call.  Nothing here reads or writes the render's pixel states, tile-cost cache or counters, or looks at the partition.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "mort_hip.h"
#include "dev_radiance.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* 3 waves per SIMD: the body takes 145 (item loop) and 158 (tree) registers and nothing spills.  Bound to four (128 registers), as
 * mega_kernel is, the tree form spills 137 registers, some of them inside the walk */
#ifndef MORT_RADIANCE_WAVES
#define MORT_RADIANCE_WAVES 3
#endif
template <bool TREE>
__global__ void __launch_bounds__(QUERY_BLOCK, MORT_RADIANCE_WAVES) query_radiance_kernel(const RadianceArgs a) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * QUERY_BLOCK];
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= a.q.n) return;
    radiance_ray<TREE>(a, i, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK, bounce_stack + threadIdx.x, MORT_RADIANCE_LDS_LEVELS, QUERY_BLOCK);
}

/* ====================================================================== host */

namespace {

/* no output (the streams are one: they are advanced in place) overlaps the rays or the other output */
bool radiance_buffers_ok(size_t n, const void *rays, void *states, void *rgb) {
    const void *ins[1] = {rays};
    const size_t in_bytes[1] = {n * sizeof(mort_ray)};
    void *outs[2] = {states, rgb};
    const size_t out_bytes[2] = {n * sizeof(mort_rng_state), n * 3 * sizeof(float)};
    return buffers_disjoint(ins, in_bytes, 1, outs, out_bytes, 2);
}

void radiance_args_params(RadianceArgs &a, const mort_radiance_params *p) {
    a.bounce_limit = p->bounce_limit; a.samples = p->samples;
    a.background = mk(p->background[0], p->background[1], p->background[2]);
    a.light_type = p->light_obj_type; a.light_idx = p->light_obj_idx;
}

struct RadianceHostJob { RadianceArgs a; bool tree; };
void radiance_host_chunk(void *p, int chunk) {
    const RadianceHostJob *j = (const RadianceHostJob *)p;
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const size_t n = j->a.q.n, i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < n ? i0 + kHostChunk : n;
    for (size_t i = i0; i < i1; i++) {
        if (j->tree) radiance_ray<true>(j->a, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
        else radiance_ray<false>(j->a, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
    }
}

/* what the three forms check before they look at a world */
int radiance_check(const mort_radiance_params *p, size_t n, const void *rays, void *states, void *rgb) {
    if (!p || !rays || !states || !rgb) return MORT_ERR_INVALID;
    if (p->samples < 1 || n > kMaxRays || !radiance_buffers_ok(n, rays, states, rgb)) return MORT_ERR_INVALID;
    if (p->bounce_limit < 0 || p->bounce_limit > MORT_MAX_BOUNCE_LIMIT) return MORT_ERR_CAPACITY;
    return MORT_OK;
}

} // namespace

int mort_radiance_check(const mort_radiance_params *p, size_t n, const void *rays, void *states, void *rgb) { return radiance_check(p, n, rays, states, rgb); }
void mort_radiance_args_params(RadianceArgs &a, const mort_radiance_params *p) { radiance_args_params(a, p); }

/* for the tests: the bounce-stack levels the kernels keep in LDS; needs no device */
extern "C" int mort_hip_debug_radiance_lds_levels(void) { return MORT_RADIANCE_LDS_LEVELS; }

extern "C" int mort_hip_radiance_params_from_camera(const mort_camera *cam, mort_radiance_params *out) {
    if (!cam || !out) return MORT_ERR_INVALID;
    out->bounce_limit = cam->bounce_limit; out->samples = 1;
    for (int k = 0; k < 3; k++) out->background[k] = cam->background.e[k];
    out->light_obj_type = cam->light_obj_type; out->light_obj_idx = cam->light_obj_idx;
    return MORT_OK;
}

extern "C" int mort_hip_query_radiance_device(mort_ctx *c, const mort_radiance_params *p, size_t n, const void *d_rays, void *d_states,
                                              void *d_rgb_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = radiance_check(p, n, d_rays, d_states, d_rgb_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_rays) || !aligned16(d_states) || !aligned16(d_rgb_out)) return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->light_obj_type, p->light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    RadianceArgs a;
    query_args_device(c, a.q);
    radiance_args_params(a, p);
    a.q.n = n; a.q.rays = (const mort_ray *)d_rays; a.q.states = (mort_rng_state *)d_states; a.rgb = (float *)d_rgb_out;
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    const dim3 grid((unsigned)((n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    if (c->gen_ok) hipLaunchKernelGGL(query_radiance_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(query_radiance_kernel<false>, grid, block, 0, s, a);
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: rays and streams up, the _device call on the context's stream, colours and streams down */
extern "C" int mort_hip_query_radiance(mort_ctx *c, const mort_radiance_params *p, size_t n, const mort_ray *rays, mort_rng_state *states,
                                       float *rgb_out, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = radiance_check(p, n, rays, states, rgb_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->light_obj_type, p->light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    StagePlane pl[3] = {{rays, nullptr, n * sizeof(mort_ray)}, {states, states, n * sizeof(mort_rng_state)}, {nullptr, rgb_out, n * 3 * sizeof(float)}};
    if ((st = stage_upload(c, pl, 3)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_query_radiance_device(c, p, n, pl[0].dev, pl[1].dev, pl[2].dev, c->stream, &sec)) != MORT_OK) return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 3);
}

extern "C" int mort_hip_query_radiance_host(const mort_world *world, const mort_radiance_params *p, size_t n, const mort_ray *rays,
                                            mort_rng_state *states, int nthreads, int flags, float *rgb_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = radiance_check(p, n, rays, states, rgb_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, p->light_obj_type, p->light_obj_idx)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    RadianceHostJob job;
    job.tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    query_args_host(sb, job.tree, job.a.q);
    radiance_args_params(job.a, p);
    job.a.q.n = n; job.a.q.rays = rays; job.a.q.states = states; job.a.rgb = rgb_out;
    const double t0 = now_s();
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, radiance_host_chunk, &job);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
