/*
 * cached_direct.hip -- direct-light cached radiance queries: cached radiance queries (cached.hip) over a volume
 * that holds indirect light only.  A path that ends in the volume adds one sampled shadow segment toward the light object, so
 * the emitters' own light keeps its shadows and its fall-off, which an SH9 record cannot hold.
 *
 * Kernel (gfx950, wave64, 256-thread groups, one lane per ray, 1-D grid):
 *   query_radiance_cached_direct_kernel<TREE, VISIBLE>   query_radiance_cached_kernel<TREE, VISIBLE> with the direct terminal in its
 *                                 bounce loop: the same loads and stores, the same LDS, one more 4-byte store per ray where the
 *                                 caller wants the lit counts.  The shadow segment takes one more turn of the loop, through the
 *                                 same search call as the path's segments.
 *
 * The host form (mort_hip_query_radiance_cached_direct_host) runs the same per-ray body (dev_cached_direct.h) on host threads and
 * makes no HIP runtime call.  Nothing here reads or writes the render's pixel states, tile-cost cache or counters, or looks at the
 * partition.
 */
#include <hip/hip_runtime.h>

#include <cstring>

#include "mort_hip.h"
#include "dev_cached_direct.h"
#include "scene_blob.h"
#include "mort_ctx.h"
#include "mort_internal.h"
#include "stage_common.h"
#include "query_common.h"

#pragma clang fp contract(off)

/* ====================================================================== device */

/* waves per SIMD the kernels are compiled for.  The light sample and the pending terminal ride on top of
 * query_radiance_cached_kernel<true, true>'s 168 registers, the last count for three waves: held to three, the two TREE kernels spill
 * (2 and 1 vector registers), so they take two waves (181 and 191 registers, no spill); the scan kernels fit three as they are
 * (DESIGN.md 4.22 has the table).  MORT_CACHED_DIRECT_WAVES overrides both, for that table */
#ifdef MORT_CACHED_DIRECT_WAVES
#define CACHED_DIRECT_WAVES(TREE) MORT_CACHED_DIRECT_WAVES
#else
#define CACHED_DIRECT_WAVES(TREE) ((TREE) ? 2 : 3)
#endif
template <bool TREE, bool VISIBLE>
__global__ void __launch_bounds__(QUERY_BLOCK, CACHED_DIRECT_WAVES(TREE)) query_radiance_cached_direct_kernel(const CachedDirectArgs<VISIBLE> d) {
    __shared__ unsigned short walk_stack[TREE ? MORT_OWN_STACK * QUERY_BLOCK : 1];
    __shared__ float4 bounce_stack[MORT_RADIANCE_LDS_LEVELS * QUERY_BLOCK];
    const size_t i = (size_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= d.c.r.q.n) return;
    cached_direct_ray<TREE, VISIBLE>(d, i, &walk_stack[TREE ? threadIdx.x : 0], QUERY_BLOCK, bounce_stack + threadIdx.x, MORT_RADIANCE_LDS_LEVELS, QUERY_BLOCK);
}

/* ====================================================================== host */

namespace {

constexpr size_t kRecordBytes = MORT_VOLUME_RECORD_FLOATS * sizeof(float);
constexpr size_t kDepthBytes = MORT_DEPTH_FLOATS * sizeof(float);

size_t direct_probes(const mort_cached_params *p) { return (size_t)p->grid.count[0] * (size_t)p->grid.count[1] * (size_t)p->grid.count[2]; }

/* the cached queries' checks, with lit as one more output */
int direct_check(const mort_cached_params *p, size_t n, const void *rays, void *states, const void *records, const void *depth, void *rgb, void *ends,
                 void *lit) {
    if (!p || !records) return MORT_ERR_INVALID;
    const int st = mort_radiance_check(&p->path, n, rays, states, rgb);
    if (st != MORT_OK) return st;
    if (!mort_cached_volume_ok(p->cache_depth, p->flags, &p->grid, &p->vis, records, depth)) return MORT_ERR_INVALID;
    const size_t probes = direct_probes(p);
    const void *ins[3] = {rays, records, depth};
    const size_t in_bytes[3] = {n * sizeof(mort_ray), probes * kRecordBytes, probes * kDepthBytes};
    void *outs[4] = {states, rgb, ends, lit};
    const size_t out_bytes[4] = {n * sizeof(mort_rng_state), n * 3 * sizeof(float), n * sizeof(uint32_t), n * sizeof(uint32_t)};
    return buffers_disjoint(ins, in_bytes, 3, outs, out_bytes, 4) ? MORT_OK : MORT_ERR_INVALID;
}

/* everything of the arguments but the scene (d.c.r.q: query_args_device / query_args_host come first, they clear it) */
template <bool VISIBLE>
void direct_args(CachedDirectArgs<VISIBLE> &d, const mort_cached_params *p, size_t n, const void *rays, void *states, const void *records,
                 const void *depth, void *rgb, void *ends, void *lit) {
    CachedArgs<VISIBLE> &c = d.c;
    mort_radiance_args_params(c.r, &p->path);
    c.r.q.n = n; c.r.q.rays = (const mort_ray *)rays; c.r.q.states = (mort_rng_state *)states; c.r.rgb = (float *)rgb;
    c.cache_depth = p->cache_depth; c.ends = (uint32_t *)ends;
    if constexpr (VISIBLE) mort_cached_volume(c.vol.v, p->grid, p->vis, records, depth);
    else mort_cached_volume(c.vol.v, p->grid, records);
    d.lit = (uint32_t *)lit;
}

template <bool VISIBLE>
void direct_launch(const mort_ctx *ctx, CachedDirectArgs<VISIBLE> &d, hipStream_t s) {
    const dim3 grid((unsigned)((d.c.r.q.n + QUERY_BLOCK - 1) / QUERY_BLOCK)), block(QUERY_BLOCK);
    if (ctx->gen_ok) hipLaunchKernelGGL((query_radiance_cached_direct_kernel<true, VISIBLE>), grid, block, 0, s, d);
    else hipLaunchKernelGGL((query_radiance_cached_direct_kernel<false, VISIBLE>), grid, block, 0, s, d);
}

template <bool VISIBLE> struct DirectHostJob { CachedDirectArgs<VISIBLE> d; bool tree; };
template <bool VISIBLE>
void direct_host_chunk(void *p, int chunk) {
    const DirectHostJob<VISIBLE> *j = (const DirectHostJob<VISIBLE> *)p;
    unsigned short walk[MORT_OWN_STACK];
    float4 first_levels[MORT_RADIANCE_LDS_LEVELS]; /* the kernel's LDS levels: the host runs the same seam */
    const size_t n = j->d.c.r.q.n, i0 = (size_t)chunk * kHostChunk, i1 = i0 + kHostChunk < n ? i0 + kHostChunk : n;
    for (size_t i = i0; i < i1; i++) {
        if (j->tree) cached_direct_ray<true, VISIBLE>(j->d, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
        else cached_direct_ray<false, VISIBLE>(j->d, i, walk, 1, first_levels, MORT_RADIANCE_LDS_LEVELS, 1);
    }
}

template <bool VISIBLE>
void direct_host_run(const SceneBlob &sb, bool tree, const mort_cached_params *p, size_t n, const mort_ray *rays, mort_rng_state *states,
                     const float *records, const float *depth, int nthreads, float *rgb, uint32_t *ends, uint32_t *lit) {
    DirectHostJob<VISIBLE> job;
    job.tree = tree;
    query_args_host(sb, tree, job.d.c.r.q);
    direct_args(job.d, p, n, rays, states, records, depth, rgb, ends, lit);
    run_rows((int)((n + kHostChunk - 1) / kHostChunk), nthreads, direct_host_chunk<VISIBLE>, &job);
}

} // namespace

extern "C" int mort_hip_query_radiance_cached_direct_device(mort_ctx *c, const mort_cached_params *p, size_t n, const void *d_rays, void *d_states,
                                                            const void *d_records, const void *d_depth, void *d_rgb_out, void *d_ends_out,
                                                            void *d_lit_out, void *stream, double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = direct_check(p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out, d_lit_out);
    if (st != MORT_OK) return st;
    if (!aligned16(d_rays) || !aligned16(d_states) || !aligned16(d_records) || !aligned16(d_depth) || !aligned16(d_rgb_out) || !aligned16(d_ends_out) ||
        !aligned16(d_lit_out))
        return MORT_ERR_INVALID;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    hipStream_t s;
    if ((st = stage_begin(c, stream, 0, seconds, &s)) != MORT_OK) return st;
    if (p->flags & MORT_CACHED_VISIBLE) {
        CachedDirectArgs<true> a;
        query_args_device(c, a.c.r.q);
        direct_args(a, p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out, d_lit_out);
        direct_launch(c, a, s);
    } else {
        CachedDirectArgs<false> a;
        query_args_device(c, a.c.r.q);
        direct_args(a, p, n, d_rays, d_states, d_records, d_depth, d_rgb_out, d_ends_out, d_lit_out);
        direct_launch(c, a, s);
    }
    HIPCHK(c, hipGetLastError());
    return stage_end(c, s, seconds);
}

/* the host-buffer form: rays, streams, records and maps up, the _device call on the context's stream, colours, streams and both counts down */
extern "C" int mort_hip_query_radiance_cached_direct(mort_ctx *c, const mort_cached_params *p, size_t n, const mort_ray *rays, mort_rng_state *states,
                                                     const float *records, const float *depth, float *rgb_out, uint32_t *ends_out, uint32_t *lit_out,
                                                     double *seconds) {
    if (!c) return MORT_ERR_INVALID;
    int st = direct_check(p, n, rays, states, records, depth, rgb_out, ends_out, lit_out);
    if (st != MORT_OK) return st;
    if (!c->have_world) return MORT_ERR_NO_WORLD;
    if ((st = check_light(c, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (n == 0) { if (seconds) *seconds = 0; return MORT_OK; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, switch_stream(c, c->stream));
    const size_t probes = direct_probes(p);
    StagePlane pl[7] = {{rays, nullptr, n * sizeof(mort_ray)}, {states, states, n * sizeof(mort_rng_state)}, {records, nullptr, probes * kRecordBytes},
                        {depth, nullptr, probes * kDepthBytes}, {nullptr, rgb_out, n * 3 * sizeof(float)}, {nullptr, ends_out, n * sizeof(uint32_t)},
                        {nullptr, lit_out, n * sizeof(uint32_t)}};
    if ((st = stage_upload(c, pl, 7)) != MORT_OK) return st;
    double sec = 0;
    if ((st = mort_hip_query_radiance_cached_direct_device(c, p, n, pl[0].dev, pl[1].dev, pl[2].dev, pl[3].dev, pl[4].dev, pl[5].dev, pl[6].dev, c->stream,
                                                           &sec)) != MORT_OK)
        return st;
    if (seconds) *seconds = sec;
    return stage_download(c, pl, 7);
}

extern "C" int mort_hip_query_radiance_cached_direct_host(const mort_world *world, const mort_cached_params *p, size_t n, const mort_ray *rays,
                                                          mort_rng_state *states, const float *records, const float *depth, int nthreads, int flags,
                                                          float *rgb_out, uint32_t *ends_out, uint32_t *lit_out, double *seconds) {
    if (!world) return MORT_ERR_INVALID;
    int st = direct_check(p, n, rays, states, records, depth, rgb_out, ends_out, lit_out);
    if (st != MORT_OK) return st;
    SceneBlob sb;
    if ((st = build_scene_blob(world, sb)) != MORT_OK) return st;
    if ((st = check_light_object(sb.comp, world->objs.num_hittable_list, p->path.light_obj_type, p->path.light_obj_idx)) != MORT_OK) return st;
    if (seconds) *seconds = 0;
    if (n == 0) return MORT_OK;
    const bool tree = (flags & MORT_HOST_TREE) && sb.comp.g_ok;
    const double t0 = now_s();
    if (p->flags & MORT_CACHED_VISIBLE) direct_host_run<true>(sb, tree, p, n, rays, states, records, depth, nthreads, rgb_out, ends_out, lit_out);
    else direct_host_run<false>(sb, tree, p, n, rays, states, records, depth, nthreads, rgb_out, ends_out, lit_out);
    if (seconds) *seconds = now_s() - t0;
    return MORT_OK;
}
